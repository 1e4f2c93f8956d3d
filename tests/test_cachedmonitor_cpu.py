"""Per-epoch validation of the CLIP-Adapter and TaskRes fits, the part that needs no GPU: the new symbols, what the entry points refuse
before any launch, the argument checks of fit_adapter / fit_residuals and of the trainers, and the logits bound of
tests/cachedmonitor_ref.py held against torch's own fp32 forward."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import cachedmonitor_ref as ref
import fitmonitor_ref

from clip_calibration_amd import _lib, adapterfit, coopfit, fitmonitor, ops, taskresfit
from clip_calibration_amd.trainers import _fit

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = ctypes.c_void_p(4096)
SYMBOLS = ("clipmi_adapter_val_logits", "clipmi_taskres_val_logits", "clipmi_adapter_fit_monitored", "clipmi_taskres_fit_monitored",
           "clipmi_adapter_fit_monitored_workspace_bytes", "clipmi_taskres_fit_monitored_workspace_bytes")


def test_symbols_exist_and_the_abi_version_stays():
    text = open(os.path.join(ROOT, "include", "clipmi.h")).read()
    exported = set(_lib.exported_symbols())
    for name in SYMBOLS:
        assert name in exported and re.search(r"\b%s\(" % name, text), name
    assert re.search(r"#define CLIPMI_ABI_VERSION 16\b", text) and _lib.ABI_VERSION == 16 and _lib.lib.clipmi_abi_version() == 16
    for name in ("adapter_val_logits", "taskres_val_logits", "fit_monitor"):
        assert callable(getattr(ops, name))
    for cls, best in ((adapterfit.AdapterFitState, "best_weights"), (taskresfit.TaskResFitState, "best_residuals")):
        for method in ("validate", "start_monitor", "monitor", best):
            assert callable(getattr(cls, method))
    assert coopfit.empty_monitor is fitmonitor.empty_monitor and coopfit.FINAL_MODELS == ("last_step", "best_val")


def test_val_logits_refuse_before_any_launch():
    L = _lib.lib

    def adapter(feats=P, ld=512, text=P, w1=P, w2=P, n=65, E=512, H=128, C=100, ratio=0.2, scale=100.0, out=P):
        return L.clipmi_adapter_val_logits(feats, ld, text, w1, w2, n, E, H, C, ratio, scale, out, None)

    def taskres(feats=P, ld=512, base=P, res=P, n=65, E=512, C=100, alpha=0.5, scale=100.0, out=P):
        return L.clipmi_taskres_val_logits(feats, ld, base, res, n, E, C, alpha, scale, out, None)

    for f, ptrs in ((adapter, ("feats", "text", "w1", "w2", "out")), (taskres, ("feats", "base", "res", "out"))):
        for null in ptrs:
            assert f(**{null: None}) == _lib.ERR_ARG and "null" in _lib.last_error(), null
            assert f(**{null: ctypes.c_void_p(4098)}) == _lib.ERR_ARG and "aligned" in _lib.last_error(), null
        assert f(out=ctypes.c_void_p(4100)) == _lib.ERR_ARG and "16-byte" in _lib.last_error()
        assert f(n=0) == _lib.ERR_SHAPE and "N_val=0" in _lib.last_error()
        assert f(ld=511) == _lib.ERR_SHAPE and "ld=511" in _lib.last_error()
        assert f(C=1) == _lib.ERR_SHAPE and "C=1" in _lib.last_error()
        assert f(E=0, ld=0) == _lib.ERR_SHAPE
        assert f(scale=float("inf")) == _lib.ERR_ARG
    assert adapter(H=0) == _lib.ERR_SHAPE and adapter(E=16384, ld=16384) == _lib.ERR_SHAPE and "LDS" in _lib.last_error()
    assert adapter(ratio=float("nan")) == _lib.ERR_ARG and taskres(alpha=float("nan")) == _lib.ERR_ARG
    if not torch.cuda.is_available():
        assert adapter() == _lib.ERR_HIP and taskres() == _lib.ERR_HIP


@pytest.mark.parametrize("which", ["adapter", "taskres"])
def test_monitored_fits_refuse_before_any_launch(which):
    L = _lib.lib
    big = 1 << 26
    EH = 512 * 128
    W1 = ctypes.c_void_p(1 << 20)
    W2 = ctypes.c_void_p((1 << 20) + 4 * EH)
    need = getattr(L, f"clipmi_{which}_fit_monitored_workspace_bytes")
    score = L.clipmi_val_score_workspace_bytes(65, 10)
    assert need(65, 100, 10) == (4 * 65 * 100 + 255) // 256 * 256 + score + L.clipmi_best_select_workspace_bytes(1)
    assert need(0, 100, 10) == 0 and need(65, 1, 10) == 0 and need(65, 100, 0) == 0 and need(65, 100, 65) == 0

    def fit(vf=P, vld=512, vl=P, n_val=65, n_bins=10, records=P, criterion=0, block=P, best=P, mws=P, mws_bytes=big, w1=W1, w2=W2, epochs=0,
            res=P, ws_bytes=big):
        tail = (vf, vld, vl, n_val, n_bins, records, criterion, block, best, mws, mws_bytes, None)
        if which == "adapter":
            return L.clipmi_adapter_fit_monitored(P, 512, P, None, P, w1, w2, P, P, 70, 512, 128, 100, 32, epochs, 0, 0.2, 100.0, P, 1, 0.9, 0.0, 5e-4,
                                                  0, None, P, ws_bytes, *tail)
        return L.clipmi_taskres_fit_monitored(P, 512, P, None, P, res, P, P, 70, 512, 100, 32, epochs, 0, 0.5, 100.0, P, 1, 0, 5e-4, 0.9, 0.0, 0,
                                              0.9, 0.999, 1e-8, None, P, ws_bytes, *tail)

    assert fit() == _lib.OK                                  # no epoch: every check passes and nothing is launched
    assert fit(block=None, best=None) == _lib.OK             # no selection
    for null in ("vf", "vl", "records", "mws"):
        assert fit(**{null: None}) == _lib.ERR_ARG and "null" in _lib.last_error(), null
    assert fit(block=None) == _lib.ERR_ARG and "together" in _lib.last_error()
    assert fit(best=None) == _lib.ERR_ARG and "together" in _lib.last_error()
    assert fit(vf=ctypes.c_void_p(4098)) == _lib.ERR_ARG and "aligned" in _lib.last_error()
    for odd in ("vl", "records", "block"):
        assert fit(**{odd: ctypes.c_void_p(4100)}) == _lib.ERR_ARG and "8-byte" in _lib.last_error(), odd
    assert fit(best=ctypes.c_void_p(4104)) == _lib.ERR_ARG and "16-byte" in _lib.last_error()
    assert fit(mws=ctypes.c_void_p(4096 + 128)) == _lib.ERR_ARG and "256-byte" in _lib.last_error()
    assert fit(n_val=0) == _lib.ERR_SHAPE and "N_val=0" in _lib.last_error()
    assert fit(vld=511) == _lib.ERR_SHAPE and "ld=511" in _lib.last_error()
    for bins in (0, 65):
        assert fit(n_bins=bins) == _lib.ERR_ARG and "n_bins" in _lib.last_error()
    assert fit(criterion=2) == _lib.ERR_ARG and "criterion" in _lib.last_error()
    assert fit(mws_bytes=need(65, 100, 10) - 1) == _lib.ERR_WORKSPACE and "needed" in _lib.last_error()
    assert fit(mws_bytes=need(65, 100, 10)) == _lib.OK
    assert fit(ws_bytes=16) == _lib.ERR_WORKSPACE            # the unmonitored call's checks come first and stay
    if which == "adapter":
        assert fit(w2=P) == _lib.ERR_ARG and "[w1 | w2]" in _lib.last_error()
        assert fit(w2=P, block=None, best=None) == _lib.OK   # split weights are fine while nothing is selected
    else:
        assert fit(res=ctypes.c_void_p(4100)) == _lib.ERR_ARG and "16-byte" in _lib.last_error()
    if not torch.cuda.is_available():
        assert fit(epochs=1) == _lib.ERR_HIP and _lib.last_error()


def _adapter_args(E=8, H=2, C=3, N=6):
    g = torch.Generator().manual_seed(0)
    return (torch.randn(N, E, generator=g), torch.arange(N) % C, torch.randn(C, E, generator=g), torch.randn(H, E, generator=g),
            torch.randn(E, H, generator=g))


def _taskres_args(E=8, C=3, N=6):
    g = torch.Generator().manual_seed(0)
    return torch.randn(N, E, generator=g), torch.arange(N) % C, torch.randn(C, E, generator=g)


@pytest.mark.parametrize("fit,args", [(adapterfit.fit_adapter, _adapter_args()), (taskresfit.fit_residuals, _taskres_args())],
                         ids=["adapter", "taskres"])
def test_fit_arguments_are_checked_before_the_first_launch(fit, args):
    """On CPU tensors: every refusal below comes before the fit asks for a GPU."""
    val = (torch.randn(5, 8), torch.arange(5) % 3)
    with pytest.raises(ValueError, match="final_model='best_val' needs val"):
        fit(*args, final_model="best_val")
    with pytest.raises(ValueError, match="final_model='best' must be one of"):
        fit(*args, val=val, final_model="best")
    with pytest.raises(ValueError, match="val_criterion='ece' must be one of"):
        fit(*args, val=val, val_criterion="ece")
    with pytest.raises(ValueError, match=r"val must be \(val_features, val_labels\)"):
        fit(*args, val=val[0])
    with pytest.raises(ValueError, match="n_bins=0"):
        fit(*args, val=val, val_bins=0)
    with pytest.raises(ValueError, match="val_features must be"):
        fit(*args, val=(torch.randn(5, 7), val[1]))
    with pytest.raises(ValueError, match=r"labels span \[0, 3\], outside the 3 classes"):
        fit(*args, val=(val[0], torch.tensor([0, 1, 2, 3, 0])))
    with pytest.raises(ValueError, match="5 validation rows need 5 labels"):
        fit(*args, val=(val[0], torch.arange(4) % 3))
    with pytest.raises(RuntimeError, match="on the GPU"):      # everything about val was accepted: the features are asked for next
        fit(*args, val=val, final_model="best_val")


def test_trainers_refuse_two_validation_sets():
    with pytest.raises(ValueError, match="fit_adapter: val_loader and val are two ways"):
        _fit.validation_set("fit_adapter", None, {"val_loader": [], "val": (1, 2)})
    with pytest.raises(ValueError, match="final_model='best_val' needs val"):
        _fit.split_monitor_args("fit_residuals", {"final_model": "best_val"}, 3, 8)
    args = {"val": (torch.randn(5, 8), [0, 1, 2, 0, 1]), "val_bins": 7, "return_monitor": True, "momentum": 0.5}
    watch = _fit.split_monitor_args("fit_adapter", args, 3, 8)
    val = watch.pop("val")
    assert watch == {"val_bins": 7, "final_model": "last_step", "val_criterion": "accuracy", "return_monitor": True} and args == {"momentum": 0.5}
    assert val[1].dtype == torch.int64 and val[1].tolist() == [0, 1, 2, 0, 1]


def test_pack_and_the_empty_monitor():
    a, b = torch.zeros(1), torch.ones(1)
    assert fitmonitor.pack(a, None, None, False, False) is a
    assert fitmonitor.pack((a, b), "h", "m", True, True) == (a, b, "h", "m")
    assert fitmonitor.pack(a, "h", "m", False, True) == (a, "m")
    m = fitmonitor.empty_monitor(7)
    assert m["bins"].shape == (0, 3, 8) and m["best_epoch"] is None and m["records"] == []


SHAPES = [(65, 128, 32, 257), (130, 512, 128, 3), (65, 512, 128, 1000)]


@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_the_logits_bound_holds_torch_fp32_and_is_not_vacuous(shape):
    """The reference's fp32 forward against its float64 forward, per element, under the bound the GPU tests use: within it (the bound is
    not too tight for an honest fp32 evaluation in another summation order) and the bound itself far below the logits' spread and below
    a thousandth of the scale (it is not vacuous: a wrong operand or a dropped term breaks it)."""
    N, E, H, C = shape
    s = 100.0
    c = ref.adapter_val_case(N, E, H, C)
    z, tz = ref.adapter_logits_bound(c["f"], c["T"], c["w1"], c["w2"], ref.RATIO, s)
    z32 = ref.adapter_logits(c["f"], c["T"], c["w1"], c["w2"], ref.RATIO, s, torch.float32).double()
    assert torch.allclose(z, ref.adapter_logits(c["f"], c["T"], c["w1"], c["w2"], ref.RATIO, s), rtol=1e-13, atol=1e-13)
    r = float(((z32 - z).abs() / tz).max())
    print(f"cachedmonitor: adapter {shape} torch fp32 / bound {r:.3f}, max bound {float(tz.max()):.3e}, logits' std {float(z.std()):.3f}")
    assert r <= 1.0 and float(tz.max()) < 1e-3 * s and float(tz.max()) < 1e-2 * float(z.std())
    t = ref.taskres_val_case(N, E, C)
    z, tz = ref.taskres_logits_bound(t["f"], t["base"], t["r"], ref.ALPHA, s)
    z32 = ref.taskres_logits(t["f"], t["base"], t["r"], ref.ALPHA, s, torch.float32).double()
    assert torch.allclose(z, ref.taskres_logits(t["f"], t["base"], t["r"], ref.ALPHA, s), rtol=1e-13, atol=1e-13)
    r = float(((z32 - z).abs() / tz).max())
    print(f"cachedmonitor: taskres {shape} torch fp32 / bound {r:.3f}, max bound {float(tz.max()):.3e}, logits' std {float(z.std()):.3f}")
    assert r <= 1.0 and float(tz.max()) < 1e-3 * s and float(tz.max()) < 1e-2 * float(z.std())
    # one dropped term of the E-term dot is far outside the bound
    short = np.array(t["f"])
    short[:, -1] = 0
    bad = ref.taskres_logits(short, t["base"], t["r"], ref.ALPHA, s)
    assert float(((bad - z).abs() / tz).max()) > 10.0


def test_clear_of_ties_and_edges_is_a_real_precondition():
    z = np.array([[2.0, 0.0, -1.0], [1.0, 1.0 + 1e-9, 0.0]])
    tz = np.full_like(z, 1e-6)
    assert ref.clear_of_ties_and_edges(z[:1], tz[:1], 10) and not ref.clear_of_ties_and_edges(z, tz, 10)
    conf = fitmonitor_ref.score_rows(z[:1], np.array([0]))[2]
    assert not ref.clear_of_ties_and_edges(z[:1], np.full((1, 3), abs(conf[0] - 0.8) * 1.01), 10)
