"""The trainers' validation routes on the GPU (trainers/{vpt,maple,promptsrc}.py with ``val_loader=`` / ``val=``), ``transform=None`` and
``transform=TrainPreprocess``: the fitted block equals the run without ``val`` bit for bit, record e is the record a fresh state writes at
the block of a hand-written loop truncated behind epoch e (PromptSRC: the GPA work before the validation, so the last record scores the
aggregate), ``best_val`` returns that epoch's block, the result is packed (fitted, losses, monitor), and the returned block is installed
in the model's parameters.  Geometry ``tiny``."""
import math

import numpy as np
import pytest
import torch

import augment_ref as aref
import fitmonitor_ref as ref
import maplefit_ref as mref
import promptsrcfit_ref as pref
from clip_calibration_amd import maplefit, ops, promptsrcfit, synthetic as syn, vptfit
from clip_calibration_amd.augment import TrainPreprocess
from clip_calibration_amd.model import build_model
from clip_calibration_amd.preprocess import pack_images
from clip_calibration_amd.trainers import MaPLeCLIP, PromptSRCCLIP, VPTCLIP
from clip_calibration_amd.trainers.promptsrc import teacher_features

pytestmark = pytest.mark.gpu

GEOM, C, E = "tiny", 5, 3
RATES = [0.004, 0.003, 0.002]
GPA = (1.0, 1.0)
SEED = 23


class Trainer:
    """One trainer behind one face: ``fit`` (the trainer's fit; the parameters are put back to their starting values first), ``state``
    (a fresh fit state at a block, or at the starting parameters), ``packed`` and ``installed``."""

    def __init__(self, name):
        self.name = name
        if name == "vpt":
            n_ctx, depth = 3, 2
            self.model = build_model(dict(syn.synthetic_state_dict(GEOM, seed=0)), {"trainer": "VPT", "vision_depth": depth, "vision_ctx": n_ctx,
                                                                                     "language_depth": 0, "language_ctx": 0}).cuda()
            self.tr = VPTCLIP(self.model, syn.synthetic_token_ids(C, GEOM, seed=0))
            shallow, deep = self.model.ivlp_vision_prompts()
            self.params = {str(i): p for i, p in enumerate([shallow] + list(deep))}
        elif name == "maple":
            self.n_ctx, self.depth = 2, 2
            self.model = build_model(dict(syn.synthetic_state_dict(GEOM, seed=0)), mref.design(self.n_ctx)).cuda()
            self.ids = mref.cref.prompt_ids(GEOM, C, self.n_ctx)
            self.tr = MaPLeCLIP(self.model, self.ids, n_ctx=self.n_ctx, prompt_depth=self.depth, seed=4)
            self.params = self.tr.learner_params()
        else:
            nt, dt, nv, dv = 2, 2, 3, 2
            self.model = build_model(dict(syn.synthetic_state_dict(GEOM, seed=0)), pref.design(nt, dt, nv, dv)).cuda()
            self.ids = pref.cref.prompt_ids(GEOM, C, nt)
            self.tr = PromptSRCCLIP(self.model, self.ids, n_ctx=nt)
            self.teacher = teacher_features(self.model, torch.stack([self.ids, pref.cref.prompt_ids(GEOM, C, nt, seed=5)], dim=1))
            self.params = self.tr.prompt_params()
        self.start = {k: v.detach().clone() for k, v in self.params.items()}

    def restore(self):
        with torch.no_grad():
            for k, p in self.params.items():
                p.copy_(self.start[k])

    def fit(self, loader, **kw):
        self.restore()
        run = dict(epochs=E, lr_per_epoch=RATES, **kw)
        if self.name == "vpt":
            out = self.tr.fit_prompts(loader, **run)
        elif self.name == "maple":
            out = self.tr.fit_prompt_learner(loader, **run)
        else:
            out = self.tr.fit_prompts(loader, self.teacher, gpa=GPA, **run)
        torch.cuda.synchronize()
        return out

    def state(self, block=None):
        """A fresh state at ``block`` (packed fp32), or at the parameters' starting values."""
        self.restore()
        if self.name == "vpt":
            prompts = None if block is None else block.view(len(self.params), *self.start["0"].shape)
            return vptfit.VPTFitState(self.model, self.tr.text_features.float(), math.log(self.tr.scale), prompts)
        if self.name == "maple":
            g = syn.GEOMETRIES[GEOM]
            named = self.params if block is None else maplefit.unpack_block(block, self.n_ctx, self.depth, g.transformer_width, g.vision_width)
            return maplefit.MaPLeFitState(self.model, self.ids, named, math.log(self.tr.scale))
        st = promptsrcfit.PromptSRCFitState(self.model, self.ids, self.params, self.teacher, math.log(self.tr.scale))
        if block is not None:
            st.block.copy_(block)
        return st

    def packed(self, fitted):
        if self.name == "vpt":
            return fitted.reshape(-1)
        return maplefit.pack_block(fitted, self.depth, "cuda") if self.name == "maple" else promptsrcfit.pack_block(fitted, "cuda")

    def installed(self, fitted):
        named = {str(i): v for i, v in enumerate(fitted)} if self.name == "vpt" else fitted
        return all(torch.equal(p.detach(), named[k].to(p.dtype)) for k, p in self.params.items())

    def hand_loop(self, loader, transform=None):
        """The block behind every epoch of a hand-written loop: steps, then PromptSRC's GPA work (the aggregate loaded behind the last
        epoch).  With it, the last epoch's block before the aggregate was loaded."""
        st = self.state()
        w = promptsrcfit.gpa_weights(E, *GPA)
        blocks, before = [], None
        for e in range(E):
            for images, y in loader:
                st.step(images if transform is None else transform(images), y, RATES[e])
            if self.name == "promptsrc":
                st.end_epoch(float(w[e]))
                if e == E - 1:
                    before = st._master().clone().reshape(-1)
                    st.apply_gpa()
            blocks.append(st._master().clone().reshape(-1))
        torch.cuda.synchronize()
        return blocks, before

    def record_at(self, block, val_loader):
        st = self.state(block)
        st.validate(val_loader, None, 0)
        return st.monitor_records()[0].cpu().numpy()


def val_batches():
    gen = torch.Generator().manual_seed(91)
    R = syn.GEOMETRIES[GEOM].image_resolution
    vi, vl = torch.randn(7, 3, R, R, generator=gen).cuda(), torch.randint(0, C, (7,), generator=gen)
    return [(vi[:4], vl[:4]), (vi[4:], vl[4:])]


def plain_loader():
    images = syn.synthetic_images(8, GEOM, seed=3).cuda()
    labels = torch.arange(8) % C
    return [(images[:4], labels[:4]), (images[4:], labels[4:])], None


def decoded_loader():
    sizes = [(80, 100), (64, 64), (70, 51), (120, 90), (66, 97), (100, 100), (45, 80), (90, 64)]
    imgs = [aref.synthetic_image(h, w, 70 + i) for i, (h, w) in enumerate(sizes)]
    labels = torch.arange(8) % C
    return [(pack_images(imgs[i:i + 4]).pin_memory(), labels[i:i + 4]) for i in (0, 4)], SEED


@pytest.mark.parametrize("route", ["plain", "transform"])
@pytest.mark.parametrize("name", ["vpt", "maple", "promptsrc"])
def test_a_trainers_fit_with_validation(name, route):
    t = Trainer(name)
    loader, seed = plain_loader() if route == "plain" else decoded_loader()
    tp = lambda: {} if seed is None else {"transform": TrainPreprocess.for_model(t.model, generator=torch.Generator().manual_seed(seed))}
    val = val_batches()
    blocks, before = t.hand_loop(loader, tp().get("transform"))
    assert all(torch.isfinite(b).all() for b in blocks) and not torch.equal(blocks[0], blocks[1]) and not torch.equal(blocks[1], blocks[2])

    # without val: the hand-written loop's block
    fitted0, losses0 = t.fit(loader, return_history=True, **tp())
    assert torch.equal(t.packed(fitted0).view(torch.int32), blocks[-1].view(torch.int32)) and losses0.shape == (2 * E,)

    # with val_loader, last_step: the same bits, (fitted, losses, monitor) in this order, every record the fresh state's
    out = t.fit(loader, val_loader=val, return_history=True, return_monitor=True, **tp())
    assert isinstance(out, tuple) and len(out) == 3
    fitted, losses, mon = out
    assert torch.equal(t.packed(fitted).view(torch.int32), blocks[-1].view(torch.int32)), "the fit with val differs from the fit without"
    assert np.array_equal(losses, losses0) and t.installed(fitted)
    assert mon["best_epoch"] is None and len(mon["records"]) == E and all(r["n"] == 7 for r in mon["records"])
    got = ops.encode_val_records(mon["records"], 10)
    for e in range(E):
        assert np.array_equal(t.record_at(blocks[e], val), got[e]), f"record {e} is not the fresh state's at the truncated run's block"
    if name == "promptsrc":      # the GPA work comes before the validation: the last record scores the aggregate
        assert not torch.equal(before, blocks[-1])
        assert not np.array_equal(t.record_at(before, val), got[-1])

    # best_val under both criteria, val= given as the pair: the best epoch's block, installed; without history the pair (fitted, monitor)
    for criterion in ("accuracy", "nll"):
        fitted, mon = t.fit(loader, val=(val, None), final_model="best_val", val_criterion=criterion, return_monitor=True, **tp())
        b = mon["best_epoch"]
        assert b == ref.best_epoch(mon["records"], criterion) and np.array_equal(ops.encode_val_records(mon["records"], 10), got)
        assert 0 <= b < E
        assert torch.equal(t.packed(fitted).view(torch.int32), blocks[b].view(torch.int32)), f"{criterion}: best_val did not return epoch {b}'s block"
        assert t.installed(fitted), "the selected block is not in the model's parameters"
    fitted = t.fit(loader, val_loader=val, final_model="best_val", **tp())
    assert not isinstance(fitted, tuple) and t.installed(fitted)
    with pytest.raises(ValueError, match="two ways"):
        t.fit(loader, val_loader=val, val=(val, None), **tp())
    with pytest.raises(ValueError, match="final_model='best_val' needs val="):
        t.fit(loader, final_model="best_val", **tp())
