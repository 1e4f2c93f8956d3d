"""The monitor surface the nine ``*FitState`` classes inherit from ``fitmonitor.Monitored``, on the GPU: what ``monitor()`` returns between
``start_monitor`` and the first ``validate`` (two rules, per state), the growth of CoOp's history through the shared ``History.slot``, and
the one validation-set cache on the device.  Geometry ``tiny``; 3 classes, 5 validation rows, 7 bins, batches of 4."""
import functools
import math

import numpy as np
import pytest
import torch

import cocoopfit_ref
import coopfit_ref
import prodafit_ref
from test_gpu_blockmonitor import Method as ImageMethod

pytestmark = pytest.mark.gpu

from clip_calibration_amd import adapterfit, cocoopfit, coopfit, prodafit, synthetic as syn, taskresfit  # noqa: E402
from clip_calibration_amd.model import build_model  # noqa: E402

C, N_VAL, BINS, BATCH, N_CTX = 3, 5, 7, 4, 4
GRAD_SCALE = 256.0     # tests/test_gpu_coopfit.py: the synthetic weights' gradients are large
E = syn.GEOMETRIES["tiny"].embed_dim
SUMMARY_BEFORE_THE_FIRST_VALIDATE = ("coop", "kgcoop", "adapter", "taskres")
STATES = SUMMARY_BEFORE_THE_FIRST_VALIDATE + ("cocoop", "proda", "vpt", "maple", "promptsrc")


@functools.lru_cache(maxsize=None)
def text_model():
    return build_model(dict(coopfit_ref.state_dict("tiny")), {"trainer": "CoOp"}).cuda()


@functools.lru_cache(maxsize=None)
def rows():
    """Train and validation features around C centres, the frozen text features and CLIP-Adapter's weights."""
    g = torch.Generator().manual_seed(31)
    centres = torch.randn(C, E, generator=g)
    y, vy = torch.arange(2 * BATCH) % C, torch.arange(N_VAL) % C
    text = centres + 0.5 * torch.randn(C, E, generator=g)
    return dict(f=(centres[y] + 0.3 * torch.randn(2 * BATCH, E, generator=g)).cuda(), y=y, vf=(centres[vy] + 0.6 * torch.randn(N_VAL, E, generator=g)).cuda(),
                vy=vy, base=text.cuda(), text=(text / text.norm(dim=1, keepdim=True)).cuda(), w1=torch.randn(32, E, generator=g) / math.sqrt(3 * E),
                w2=torch.randn(E, 32, generator=g) / math.sqrt(3 * 32))


@functools.lru_cache(maxsize=None)
def image_method(name):
    return ImageMethod(name, C, BATCH)


def new_state(name):
    r = rows()
    if name in ("coop", "kgcoop"):
        c = coopfit_ref.make_case("tiny", C, N_CTX, BATCH)
        kw = dict(method="kgcoop", teacher=r["text"]) if name == "kgcoop" else {}
        return coopfit.CoOpFitState(text_model(), c["ids"], c["ctx"], grad_scale=GRAD_SCALE, **kw)
    if name == "adapter":
        return adapterfit.AdapterFitState(r["text"], r["w1"], r["w2"])
    if name == "taskres":
        return taskresfit.TaskResFitState(r["base"], optimizer="sgd")
    if name == "cocoop":
        c = cocoopfit_ref.make_case("tiny", C, N_CTX, BATCH)
        return cocoopfit.CoCoOpFitState(text_model(), c["ids"], c["params"], grad_scale=GRAD_SCALE)
    if name == "proda":
        c = prodafit_ref.make_case("tiny", C, N_CTX, 8, 2, BATCH)
        return prodafit.ProDAFitState(text_model(), c["ids"], c["ctx"], prompt_bs=2, grad_scale=GRAD_SCALE, generator=torch.Generator().manual_seed(5))
    m = image_method(name)
    return m.state(m.start.reshape(-1))


@pytest.mark.parametrize("name", STATES)
def test_monitor_before_the_first_validate(name):
    """Two rules, as they were before the states shared one mix-in: CoOp, CLIP-Adapter and TaskRes return the started history's own
    summary, the other six ``empty_monitor()``."""
    st = new_state(name)
    st.start_monitor(2, BINS, select=True)
    mon = st.monitor()
    assert mon["records"] == [] and all(mon[k].shape == (0,) for k in ("accuracy", "nll", "ece"))
    if name in SUMMARY_BEFORE_THE_FIRST_VALIDATE:
        assert mon["bins"].shape == (0, 3, BINS + 1) and mon["best_epoch"] == -1
    else:
        assert mon["bins"].shape == (0, 3, 11) and mon["best_epoch"] is None
    assert st.monitor_records().shape[0] == 2


def test_coop_history_grows_through_the_shared_slot():
    r = rows()
    st = new_state("coop")
    st.start_monitor(1)
    vl = r["vy"].cuda()
    st.validate(r["vf"], vl, 0)
    first = st.monitor_records()[0].clone()
    st.step(r["f"][:BATCH], r["y"][:BATCH], 2e-3)
    st.validate(r["vf"], vl, 2)
    assert st.monitor_records().shape[0] == 3 and torch.equal(st.monitor_records()[0], first)
    mon = st.monitor()
    assert len(mon["records"]) == 3 and mon["records"][0]["n"] == mon["records"][2]["n"] == N_VAL and mon["records"][1]["n"] == 0
    assert st.val_logits().shape == (N_VAL, C) and torch.isfinite(st.val_logits()).all()


@pytest.mark.parametrize("name", ["coop", "proda"])
def test_the_validation_set_is_prepared_once_per_set(name):
    r = rows()
    st = new_state(name)
    vf, vl = r["vf"].clone(), r["vy"].cuda()
    st.validate(vf, vl, 0)
    made = st._mon.val[1]
    if name == "coop":      # the cached features are the normalised ones, a tensor of the monitor's own
        assert made.data_ptr() != vf.data_ptr() and np.allclose(made.norm(dim=1).cpu().numpy(), 1.0, atol=1e-5)
    st.validate(vf, vl, 1)
    assert st._mon.val[1] is made and st._mon.val[1].data_ptr() == made.data_ptr()
    records = st.monitor_records()[:2].clone()
    assert torch.equal(records[0], records[1])
    vf.add_(0)              # same values, a new version: the set is prepared again
    st.validate(vf, vl, 1)
    assert st._mon.val[1] is not made
    assert torch.equal(st.monitor_records()[:2], records)
