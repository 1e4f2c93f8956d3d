"""``optimizer="adam" | "adamw"`` on the eight prompt fits (CoOp -- generic and class-specific --, KgCoOp, ProGrad, ProDA, CoCoOp, VPT,
MaPLe, PromptSRC / IVLP) on the GPU, on the tiny towers of the sibling fit tests: ``"sgd"`` given explicitly changes nothing; an Adam step
equals ``ops.block_step_adam`` on the gradient the fit's own ``context_gradient`` / ``gradients`` / ``prompt_gradient`` returns, bit for
bit, over two steps; AdamW, Adam and SGD give different blocks; the dynamic loss scale gives the static bits; a monitored fit returns the
block of the epoch its monitor names; the trainers pass the argument on."""
import functools

import numpy as np
import pytest
import torch

import cocoopfit_ref
import coopfit_ref
import maplefit_ref
import prodafit_ref
import promptsrcfit_ref
import vptfit_ref

pytestmark = pytest.mark.gpu

from clip_calibration_amd import cocoopfit, coopfit, fitloop, maplefit, ops, prodafit, promptsrcfit, vptfit  # noqa: E402
from clip_calibration_amd.model import build_model  # noqa: E402

GRAD_SCALE = 256.0          # as the sibling fit tests: the synthetic weights give gradients far larger than ViT-B/16's
RATES = [2e-3, 1e-3]
WD = 5e-4
BETAS, EPS = (0.9, 0.999), 1e-8
C, B = 5, 4


def same(a, b):
    return a.detach().cpu().contiguous().view(torch.int32).equal(b.detach().cpu().contiguous().view(torch.int32))


class Fit:
    """One fit on one tiny case: its state, its one batch, its master block and the gradient its own diagnostic entry point returns for
    the state's current parameters, as a flat block in the master's layout."""

    def __init__(self, name):
        self.name, self.step_kw = name, {}
        if name in ("coop", "coop_csc", "kgcoop", "prograd"):
            c = coopfit_ref.make_case("tiny", C, 4, B, csc=name == "coop_csc")
            m = build_model(dict(coopfit_ref.state_dict("tiny")), {"trainer": "CoOp"}).cuda()
            method = "coop" if name.startswith("coop") else name
            extra = {}
            if method != "coop":
                extra = dict(method=method, teacher=(torch.randn(C, m.geometry.embed_dim, generator=torch.Generator().manual_seed(3)) * 2.0).cuda())
            x, y = c["feats"].cuda(), c["labels"].cuda()
            self.make = lambda **kw: coopfit.CoOpFitState(m, c["ids"], c["ctx"], coopfit_ref.LOGIT_SCALE, **dict(dict(grad_scale=GRAD_SCALE), **kw), **extra)
            self.block = lambda st: st.ctx
            self.grad = lambda st: coopfit.context_gradient(m, c["ids"], st.ctx, x, y, coopfit_ref.LOGIT_SCALE, GRAD_SCALE, **extra)[1]
            self.fit = lambda **kw: coopfit.fit_context(x, y, m, c["ids"], c["ctx"], logit_scale=coopfit_ref.LOGIT_SCALE, grad_scale=GRAD_SCALE,
                                                        batch_size=B, **extra, **kw)
        elif name == "proda":
            c = prodafit_ref.make_case("tiny", C, 4, 8, 4, B)
            m = build_model(dict(coopfit_ref.state_dict("tiny")), {"trainer": "CoOp"}).cuda()
            x, y = c["feats"].cuda(), c["labels"].cuda()
            sel = np.array([0, 3, 5, 6])
            self.step_kw = {"sel": sel}
            self.make = lambda **kw: prodafit.ProDAFitState(m, c["ids"], c["ctx"], prompt_bs=4, logit_scale=prodafit_ref.LOGIT_SCALE,
                                                            **dict(dict(grad_scale=GRAD_SCALE), **kw))
            self.block = lambda st: st.ctx
            self.grad = lambda st: prodafit.context_gradient(m, c["ids"], st.ctx, x, y, sel=sel, alpha=st.alpha, logit_scale=prodafit_ref.LOGIT_SCALE,
                                                             grad_scale=GRAD_SCALE)[1]
        elif name == "cocoop":
            c = cocoopfit_ref.make_case("tiny", C, 4, B)
            m = build_model(dict(coopfit_ref.state_dict("tiny")), {"trainer": "CoOp"}).cuda()
            x, y = c["feats"].cuda(), c["labels"].cuda()
            self.make = lambda **kw: cocoopfit.CoCoOpFitState(m, c["ids"], c["params"], logit_scale=cocoopfit_ref.LOGIT_SCALE,
                                                              **dict(dict(grad_scale=GRAD_SCALE), **kw))
            self.block = lambda st: st.block
            self.grad = lambda st: cocoopfit._master_block(
                cocoopfit.gradients(m, c["ids"], st.params(), x, y, cocoopfit_ref.LOGIT_SCALE, GRAD_SCALE)[1], st.n_ctx, st.D, st.E, st.H, x.device)
            self.fit = lambda **kw: cocoopfit.fit_prompt_learner(x, y, m, c["ids"], c["params"], logit_scale=cocoopfit_ref.LOGIT_SCALE,
                                                                 grad_scale=GRAD_SCALE, batch_size=B, **kw)
            self.flat = lambda out: torch.cat([out[k].reshape(-1) for k in cocoopfit.NAMES])
        elif name == "vpt":
            c = vptfit_ref.make_case("tiny", 2, 2, B, C)
            m = build_model(dict(c["sd"]), {"trainer": "VPT", "vision_depth": 2, "vision_ctx": 2, "language_depth": 0, "language_ctx": 0}).cuda()
            x, y, text = c["images"].cuda(), c["labels"].cuda(), c["text"].cuda()
            self.make = lambda **kw: vptfit.VPTFitState(m, text, vptfit_ref.LOGIT_SCALE, c["prompts"], **dict(dict(grad_scale=GRAD_SCALE), **kw))
            self.block = lambda st: st.prompts
            self.grad = lambda st: vptfit.prompt_gradient(m, st.prompts, x, y, text, vptfit_ref.LOGIT_SCALE, GRAD_SCALE)[1]
            self.fit = lambda **kw: vptfit.fit_prompts(x, y, m, text, c["prompts"], logit_scale=vptfit_ref.LOGIT_SCALE, grad_scale=GRAD_SCALE,
                                                       batch_size=B, **kw)
        elif name == "maple":
            c = maplefit_ref.make_case("tiny3", 2, 1, C, B)
            m = build_model(dict(c["sd"]), maplefit_ref.design(1)).cuda()
            rows = maplefit_ref.live_rows(c["ids"], False)
            x, y = c["images"].cuda(), c["labels"].cuda()
            self.make = lambda **kw: maplefit.MaPLeFitState(m, c["ids"], c["pl"], maplefit_ref.LOGIT_SCALE, seq_rows=rows,
                                                            **dict(dict(grad_scale=GRAD_SCALE), **kw))
            self.block = lambda st: st.block
            self.grad = lambda st: maplefit.pack_block(maplefit.gradients(m, st.params(), x, y, c["ids"], maplefit_ref.LOGIT_SCALE, GRAD_SCALE, rows)[1],
                                                       st.towers.depth, x.device)
            self.model, self.case, self.rows = m, c, rows
        else:
            c = promptsrcfit_ref.make_case("tiny", 2, 2, 3, 2, C, B)
            m = build_model(dict(c["sd"]), promptsrcfit_ref.design(3, 2, 2, 2)).cuda()
            rows = promptsrcfit_ref.live_rows(c["ids"], True)
            x, y, teacher = c["images"].cuda(), c["labels"].cuda(), c["teacher"].cuda()
            self.make = lambda **kw: promptsrcfit.PromptSRCFitState(m, c["ids"], c["p"], teacher, promptsrcfit_ref.LOGIT_SCALE, seq_rows=rows, method=name,
                                                                    **dict(dict(grad_scale=GRAD_SCALE), **kw))
            self.block = lambda st: st.block
            self.grad = lambda st: promptsrcfit.pack_block(
                promptsrcfit.gradients(m, st.params(), x, y, c["ids"], teacher, promptsrcfit_ref.LOGIT_SCALE, grad_scale=GRAD_SCALE, seq_rows=rows,
                                       method=name)[1], x.device)
        self.batch = (x, y)

    def run(self, steps=2, **kw):
        """``steps`` steps on the batch at RATES: (the master block, the state)."""
        st = self.make(**kw)
        lr = torch.tensor(RATES, dtype=torch.float32).cuda()
        for k in range(steps):
            st.step(*self.batch, lr[k:k + 1], **self.step_kw)
        torch.cuda.synchronize()
        return self.block(st).detach().cpu().clone(), st


@functools.lru_cache(maxsize=None)
def fit(name):
    return Fit(name)


FITS = ["coop", "coop_csc", "kgcoop", "prograd", "proda", "cocoop", "vpt", "maple", "promptsrc", "ivlp"]


@pytest.mark.parametrize("name", FITS)
def test_sgd_given_explicitly_changes_nothing(name):
    f = fit(name)
    default, st = f.run()
    named, _ = f.run(optimizer="sgd")
    assert st.optimizer == "sgd" and st._adam is None and same(default, named)
    assert torch.isfinite(default).all() and not same(default, f.block(f.make()))


@pytest.mark.parametrize("name", FITS)
def test_adam_step_is_block_step_adam_on_the_fits_own_gradient(name):
    f = fit(name)
    st = f.make(optimizer="adam")
    ref = f.block(st).detach().clone().reshape(-1)
    m, v = torch.zeros_like(ref), torch.zeros_like(ref)
    table = torch.from_numpy(fitloop.adam_bias_table(BETAS, 4)).cuda()
    lr = torch.tensor(RATES, dtype=torch.float32).cuda()
    for k in range(2):
        grad = f.grad(st).reshape(-1).contiguous()
        assert torch.isfinite(grad).all() and grad.abs().max() > 0
        ops.block_step_adam(grad, ref, m, v, lr[k:k + 1], k + 1, table, 1.0, BETAS, EPS, WD, want_grad=False)
        st.step(*f.batch, lr[k:k + 1], **f.step_kw)
        assert same(f.block(st).reshape(-1), ref), k
        assert same(st._adam.exp_avg.reshape(-1), m) and same(st._adam.exp_avg_sq.reshape(-1), v), k
    assert st._adam.steps_taken == 2 and st.steps == 2


@pytest.mark.parametrize("name", FITS)
def test_adamw_adam_and_sgd_give_different_blocks(name):
    f = fit(name)
    sgd, _ = f.run()
    adam, _ = f.run(optimizer="adam", weight_decay=0.01)
    adamw, st = f.run(optimizer="adamw", weight_decay=0.01)
    assert st._adam.decoupled and torch.isfinite(adam).all() and torch.isfinite(adamw).all()
    assert not same(adam, adamw) and not same(adam, sgd) and not same(adamw, sgd)
    with pytest.raises(ValueError, match="one_call=True with optimizer='adamw'"):
        st.step(*f.batch, RATES[0], one_call=True, **f.step_kw)


@pytest.mark.parametrize("optimizer", ["adam", "adamw"])
@pytest.mark.parametrize("name", [n for n in FITS if n != "prograd"])
def test_dynamic_scale_without_overflow_gives_the_static_bits(name, optimizer):
    f = fit(name)
    static, _ = f.run(optimizer=optimizer)
    dynamic, st = f.run(optimizer=optimizer, grad_scale="dynamic", scaler={"init_scale": GRAD_SCALE, "growth_interval": 1000})
    assert st.scaler_state() == {"scale": GRAD_SCALE, "growth_tracker": 2, "skipped_steps": 0, "applied_steps": 2, "found_inf": 0}
    assert same(dynamic, static)


def test_prograd_keeps_its_static_scale_under_adam():
    with pytest.raises(ValueError, match="ProGrad keeps a static scale"):
        fit("prograd").make(optimizer="adam", grad_scale="dynamic")


@pytest.mark.parametrize("name", ["coop", "vpt", "cocoop"])
def test_monitored_adam_fit_returns_the_block_of_the_epoch_its_monitor_names(name):
    f = fit(name)
    x, y = f.batch
    flat = getattr(f, "flat", lambda out: out.reshape(-1))
    kw = dict(optimizer="adam", epochs=3, lr_per_epoch=[2e-3, 2e-3, 2e-3], val=(x, y), return_monitor=True)
    best, mon = f.fit(final_model="best_val", **kw)
    e = int(mon["best_epoch"])
    assert 0 <= e < 3
    upto, _ = f.fit(final_model="last_step", **dict(kw, epochs=e + 1, lr_per_epoch=[2e-3] * (e + 1)))
    assert same(flat(best), flat(upto))


def test_trainers_pass_the_optimizer_on():
    import math
    from clip_calibration_amd.trainers import coop as coop_trainer, maple as maple_trainer
    c = coopfit_ref.make_case("tiny", C, 4, B)
    m = build_model(dict(coopfit_ref.state_dict("tiny")), {"trainer": "CoOp"}).cuda()
    x, y = c["feats"].cuda(), c["labels"].cuda()
    clip = coop_trainer.CustomCLIP(m, c["ids"], n_ctx=4)
    start = clip.prompt_learner.ctx.detach().clone()
    args = dict(epochs=2, lr_per_epoch=[2e-3, 1e-3], batch_size=B, grad_scale=GRAD_SCALE, optimizer="adam")
    want = coopfit.fit_context(x, y, m, clip.prompt_learner.tokenized_prompts, start, logit_scale=math.log(clip.scale), **args)
    try:        # the loader's "images" are cached features, passed through by a stand-in for the image tower (tests/test_gpu_coopfit.py)
        m.image_features_f32 = lambda image: image
        got = clip.fit_context([(x, y)], **args)
    finally:
        del m.image_features_f32
    assert same(got, want) and not same(got, start.float())
    f = fit("maple")                            # tests/maplefit_ref.py's case: one context vector, two layers of prompts
    xi, yi = f.batch
    tr = maple_trainer.CustomCLIP(f.model, f.case["ids"], n_ctx=1, prompt_depth=2, seed=2)
    ids, params = tr.prompt_learner.tokenized_prompts, {k: v.detach().clone() for k, v in tr.learner_params().items()}
    args = dict(epochs=2, lr_per_epoch=[2e-3, 1e-3], grad_scale=GRAD_SCALE, optimizer="adamw")
    want = maplefit.fit_prompt_learner([(xi, yi)], None, f.model, ids, params, logit_scale=math.log(tr.scale), **args)
    got = tr.fit_prompt_learner([(xi, yi)], **args)
    assert set(got) == set(want) and all(same(got[k], want[k]) for k in want)
    assert any(not same(got[k], params[k].float()) for k in want)
