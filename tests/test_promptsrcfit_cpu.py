"""PromptSRC's / IVLP's training path without a GPU: tests/promptsrcfit_ref.py's autograd-free float64 restatement -- the splices on both
towers, the four-term head, the master block's layout and the prompt aggregation -- against torch autograd through the oracle and the
reference's own loss expression, for every parameter tensor; ``gpa_weights`` against the closed form; the refusals."""
import math

import numpy as np
import pytest
import torch

import promptsrcfit_ref as ref
from clip_calibration_amd import promptsrcfit as fit
from clip_calibration_amd import synthetic as syn
from clip_calibration_amd.model import build_model

# As test_maplefit_cpu.py: on the island towers what is left between the restatement and the oracle's autograd is float64 rounding.
RTOL = 1e-9
PLAIN_TOL, PLAIN_LOSS_TOL = 3e-6, 1e-5
_CACHE = {}


def case(*key):
    if key not in _CACHE:
        c = ref.make_case(*key[:7])
        c["loss64"], c["grad64"] = ref.oracle_loss_grads(c["sd"], c["ids"], c["p"], c["images"], c["labels"], c["teacher"])
        _CACHE[key] = c
    return _CACHE[key]


@pytest.mark.parametrize("geom,dt,dv,nt,nv,C,B,cut", ref.CASES)
def test_restatement_equals_autograd_for_every_parameter(geom, dt, dv, nt, nv, C, B, cut):
    """Float64 rounding, every parameter tensor and every loss term: the autograd-free restatement on the island towers against autograd."""
    c = case(geom, dt, dv, nt, nv, C, B, cut)
    losses, grads = ref.loss_and_grads(c["sd"], c["ids"], c["p"], c["images"], c["labels"], c["teacher"], islands=True)
    for i in range(5):
        assert abs(float(losses[i] - c["loss64"][i])) <= RTOL * abs(float(c["loss64"][i])), i
    assert sorted(grads) == sorted(ref.param_names(dt, dv)) == sorted(c["grad64"])
    for name in ref.param_names(dt, dv):
        want = c["grad64"][name]
        assert grads[name].shape == want.shape == c["p"][name].shape, name
        assert float(want.norm()) > 0, name          # no tensor of these cases is cut off from the loss
        err = ref.rel_fro(grads[name], want)
        print(f"\npromptsrcfit-cpu: {geom} depths=({dt},{dv}) n=({nt},{nv}) C={C} B={B} {name}: grad rel {err:.2e} (bound {RTOL:.0e})")
        assert err <= RTOL, name


@pytest.mark.parametrize("geom,dt,dv,nt,nv,C,B,cut", ref.CASES[:2])
def test_plain_float64_formulas_stay_within_the_oracles_fp32_islands(geom, dt, dv, nt, nv, C, B, cut):
    """The formulas without the islands, on the live rows the case's GPU run computes, within the oracle's fp32 round-off -- where no
    L1 sign sits closer to zero than that round-off (asserted: a condition on the case)."""
    c = case(geom, dt, dv, nt, nv, C, B, cut)
    rows = ref.live_rows(c["ids"], cut) or None
    losses, grads, ft = ref.loss_and_grads(c["sd"], c["ids"], c["p"], c["images"], c["labels"], c["teacher"], rows=rows, return_features=True)
    assert min(ref.margins(ft["feats"], ft["zs"], ft["text"], c["teacher"].double())) > 1e-5
    assert abs(float(losses[0] - c["loss64"][0])) <= PLAIN_LOSS_TOL * max(1.0, abs(float(c["loss64"][0])))
    for name in ref.param_names(dt, dv):
        assert ref.rel_fro(grads[name], c["grad64"][name]) <= PLAIN_TOL, name


def test_zero_weights_are_maples_joint_head_and_ivlp():
    g = torch.Generator().manual_seed(6)
    f, zs = torch.randn(3, 64, generator=g).double(), torch.randn(3, 64, generator=g).double()
    t, o = torch.randn(5, 64, generator=g).double(), torch.randn(5, 64, generator=g).double()
    y = torch.randint(0, 5, (3,), generator=g)
    losses, d_feats, d_text = ref.head(f, zs, t, o, y, 100.0, (0.0, 0.0, 0.0))
    l, want_feats, want_text = ref.mref.joint_head(f, y, t, 100.0)
    assert abs(float(losses[0] - l)) <= 1e-14 and float(losses[0]) == float(losses[1])
    assert ref.rel_fro(d_feats, want_feats) <= 1e-14 and ref.rel_fro(d_text, want_text) <= 1e-14


def test_head_against_autograd_term_by_term():
    """Each weight alone and all together: the hand-written gradients of the four terms against autograd on the same expression."""
    g = torch.Generator().manual_seed(7)
    f, zs = torch.randn(3, 64, generator=g).double(), torch.randn(3, 64, generator=g).double()
    t, o = torch.randn(5, 64, generator=g).double(), torch.randn(5, 64, generator=g).double()
    y = torch.randint(0, 5, (3,), generator=g)
    F = torch.nn.functional
    for w in [(25.0, 0.0, 0.0), (0.0, 10.0, 0.0), (0.0, 0.0, 1.0), ref.WEIGHTS]:
        fa, ta = f.clone().requires_grad_(True), t.clone().requires_grad_(True)
        x, u = fa / fa.norm(dim=-1, keepdim=True), ta / ta.norm(dim=-1, keepdim=True)
        yy, oo = zs / zs.norm(dim=-1, keepdim=True), o / o.norm(dim=-1, keepdim=True)
        z, zz = 100.0 * x @ u.t(), 100.0 * yy @ oo.t()
        terms = [F.cross_entropy(z, y), F.l1_loss(u, oo), F.l1_loss(x, yy),
                 F.kl_div(F.log_softmax(z, 1), F.log_softmax(zz, 1), reduction="sum", log_target=True) / z.numel()]
        total = terms[0] + w[0] * terms[1] + w[1] * terms[2] + w[2] * terms[3]
        total.backward()
        losses, d_feats, d_text = ref.head(f, zs, t, o, y, 100.0, w)
        for i, want in enumerate([total] + terms):
            assert abs(float(losses[i] - want.detach())) <= 1e-12 * max(1.0, abs(float(want.detach()))), (w, i)
        assert ref.rel_fro(d_feats, fa.grad) <= 1e-12 and ref.rel_fro(d_text, ta.grad) <= 1e-12, w


def test_sign_of_zero_is_zero():
    """A teacher that equals the student contributes no L1 gradient and no L1 loss."""
    g = torch.Generator().manual_seed(8)
    f, t = torch.randn(2, 64, generator=g).double(), torch.randn(3, 64, generator=g).double()
    y = torch.tensor([0, 2])
    a = ref.head(f, f, t, t, y, 100.0, (25.0, 10.0, 0.0))
    b = ref.head(f, f, t, t, y, 100.0, (0.0, 0.0, 0.0))
    assert float(a[0][2]) == 0.0 and float(a[0][3]) == 0.0
    assert torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])


def test_master_block_layout():
    nt, dt, Dt, nv, dv, Dv = 2, 3, 64, 3, 2, 192
    p = ref.make_params("tiny3", nt, dt, nv, dv)
    block = ref.pack(p)
    assert block.numel() == ref.block_floats(nt, dt, Dt, nv, dv, Dv) == dt * nt * Dt + dv * nv * Dv
    back = ref.unpack(block, nt, dt, Dt, nv, dv, Dv)
    assert list(back) == ref.param_names(dt, dv) == fit.param_names(dt, dv)
    for name in back:
        assert torch.equal(back[name], p[name]), name
    # the text part is the [ctx; deep] pair, the image part the image tower's [dv, nv, Dv] block with visual.VPT in slot 0
    tpart = block[:dt * nt * Dt].reshape(dt, nt, Dt)
    assert torch.equal(tpart[0], p["ctx"]) and torch.equal(tpart[2], p["transformer.resblocks.2.VPT_shallow"])
    vpart = block[dt * nt * Dt:].reshape(dv, nv, Dv)
    assert torch.equal(vpart[0], p["visual.VPT"]) and torch.equal(vpart[1], p["visual.transformer.resblocks.1.VPT_shallow"])
    assert torch.equal(vpart, ref.vis_block(p, torch.float32))
    # the package's own packing agrees
    assert torch.equal(fit.pack_block(p, "cpu"), block)
    mine = fit.unpack_block(block, nt, dt, Dt, nv, dv, Dv)
    assert list(mine) == list(back) and all(torch.equal(mine[k], back[k]) for k in back)
    assert syn.GEOMETRIES["tiny3"].transformer_width == Dt and syn.GEOMETRIES["tiny3"].vision_width == Dv


@pytest.mark.parametrize("epochs,mean,std", [(50, 30.0, 30.0), (50, 45.0, 5.0), (3, 2.0, 1.0), (1, 30.0, 30.0)])
def test_gpa_weights_against_the_closed_form(epochs, mean, std):
    w = fit.gpa_weights(epochs, mean, std)
    assert w.dtype == np.float64 and w.shape == (epochs,)
    assert abs(w.sum() - 1.0) <= 1e-15
    assert np.allclose(w, ref.gpa_weights(epochs, mean, std), rtol=1e-14, atol=0)
    # the reference's own expression (promptsrc.py:267-271, 359-361)
    gauss = np.array([(1 / (std * np.sqrt(2 * np.pi))) * np.exp(-0.5 * ((a - mean) / std) ** 2) for a in range(1, epochs + 1)])
    assert np.allclose(w, gauss / sum(gauss), rtol=1e-14, atol=0)
    if epochs > 1:
        assert int(np.argmax(w)) == min(epochs, max(1, int(round(mean)))) - 1


def test_gpa_weights_refusals():
    for bad in [(0, 30.0, 30.0), (5, 30.0, 0.0), (5, float("nan"), 1.0), (5, 1.0, float("inf"))]:
        with pytest.raises(ValueError):
            fit.gpa_weights(*bad)


def test_gpa_and_sgd_restatements():
    """The aggregation is the weighted sum of the epochs' blocks; SGD's restatement equals torch.optim.SGD in float64."""
    g = torch.Generator().manual_seed(9)
    blocks = [torch.randn(50, generator=g) for _ in range(3)]
    w = ref.gpa_weights(3, 2.0, 1.0)
    assert torch.allclose(ref.gpa(blocks, w), w[0] * blocks[0].double() + w[1] * blocks[1].double() + w[2] * blocks[2].double(), rtol=1e-15, atol=0)
    for kw in [dict(), dict(momentum=0.9, weight_decay=5e-4), dict(momentum=0.9, nesterov=True), dict(momentum=0.5, dampening=0.1, weight_decay=1e-2)]:
        pt = torch.randn(20, generator=g).double().requires_grad_(True)
        opt = torch.optim.SGD([pt], lr=0.1, **kw)
        mine, buf = pt.detach().clone(), None
        for _ in range(3):
            grad = torch.randn(20, generator=g).double()
            pt.grad = grad.clone()
            opt.step()
            mine, buf = ref.sgd_step(mine, grad, buf, 0.1, **kw)
        assert torch.allclose(mine, pt.detach(), rtol=1e-13, atol=1e-15), kw


# ------------------------------------------------------------------------------------------------------------------------- the refusals
def _model(geom="tiny3", design=None):
    return build_model(dict(syn.synthetic_state_dict(geom, seed=0)), design or ref.design(2, 3, 3, 2))


def test_refusals_of_the_design():
    who = "t"
    good = _model()
    p = ref.make_params("tiny3", 2, 3, 3, 2)
    assert fit._check_design(who, good, p) == (2, 3, 3, 2)
    assert list(fit.model_params(good, p["ctx"])) == fit.param_names(3, 2)
    with pytest.raises(ValueError, match="IVLP"):
        fit._check_design(who, _model(design={"trainer": "MaPLe", "vision_depth": 0, "language_depth": 0, "vision_ctx": 0, "language_ctx": 0,
                                              "maple_length": 2}), p)
    with pytest.raises(ValueError, match="language_ctx"):
        fit._check_design(who, good, dict(p, ctx=torch.zeros(3, 64), **{f"transformer.resblocks.{i}.VPT_shallow": torch.zeros(3, 64) for i in (1, 2)}))
    with pytest.raises(ValueError, match="vision_depth"):
        fit._check_design(who, _model(design=ref.design(2, 3, 3, 0)), p)
    with pytest.raises(ValueError, match="'end'"):
        fit._check_design(who, good, p, "middle")
    with pytest.raises(ValueError, match="layers"):      # deeper than the text tower
        fit._check_design(who, good, dict(p, **{"transformer.resblocks.3.VPT_shallow": torch.zeros(2, 64)}))
    with pytest.raises(ValueError, match="layers"):      # a design deeper than the towers
        fit._check_design(who, _model(design=ref.design(2, 9, 3, 2)), p)
    with pytest.raises(ValueError, match="must be a floating-point tensor"):
        fit._check_design(who, good, dict(p, **{"visual.transformer.resblocks.1.VPT_shallow": torch.zeros(2, 192)}))
    with pytest.raises(ValueError, match="at most 224"):
        many = ref.design(2, 3, 220, 2)
        fit._check_design(who, _model(design=many), dict(p, **{"visual.VPT": torch.zeros(220, 192), "visual.transformer.resblocks.1.VPT_shallow": torch.zeros(220, 192)}))
    with pytest.raises(ValueError, match="ViT"):
        fit._check_design(who, type("M", (), {"is_resnet": True})(), p)


def test_refusals_of_the_arguments():
    with pytest.raises(ValueError, match="method"):
        fit._method_weights("t", "coop", 1.0, 1.0, 1.0)
    assert fit._method_weights("t", "ivlp", 25.0, 10.0, 1.0) == (0.0, 0.0, 0.0)
    assert fit._method_weights("t", "promptsrc", 25, 10, 1) == (25.0, 10.0, 1.0)
    for bad in [(-1.0, 0.0, 0.0), (0.0, float("nan"), 0.0), (0.0, 0.0, float("inf"))]:
        with pytest.raises(ValueError):
            fit._check_weights("t", *bad)
    with pytest.raises(ValueError, match="gpa"):
        fit._gpa_for("t", [0.5, 0.5, 0.0], 2)
    assert fit._gpa_for("t", None, 5) is None
    assert np.allclose(fit._gpa_for("t", (30.0, 30.0), 50), fit.gpa_weights(50))
    good = _model()
    ids = ref.cref.prompt_ids("tiny3", 3, 2)
    assert fit._check_ids("t", good, ids, 2)[0] == 3
    with pytest.raises(ValueError, match="does not fit"):
        fit._check_ids("t", good, ids, int(ids.argmax(dim=-1).min()))


def test_defaults_restate_the_config():
    import inspect
    d = {k: v.default for k, v in inspect.signature(fit.fit_prompts).parameters.items()}
    assert (d["lr"], d["epochs"], d["batch_size"], d["w_text"], d["w_image"], d["w_logit"], d["gpa"]) == (0.0025, 50, 4, 25.0, 10.0, 1.0, (30.0, 30.0))
    assert (d["momentum"], d["weight_decay"], d["method"]) == (0.9, 5e-4, "promptsrc")
    assert math.frexp(fit.DEFAULT_GRAD_SCALE)[0] == 0.5
