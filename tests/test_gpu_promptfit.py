"""KgCoOp's and ProGrad's training on the GPU (clip_calibration_amd/coopfit.py with ``method=``, csrc/prompt_train.hip) on the `tiny` and
`tiny3` geometries against the float64 restatement and float64 autograd through the oracle (tests/promptfit_ref.py).

The bounds are computed here, at run time, by the rules of the CoOp tests.  Operator level: 4 x the distance of torch's own fp32
evaluation of the same formulas from float64, with the floor test_gpu_text_backward.py::test_coop_head derives.  End to end: the relative
Frobenius error against float64 autograd within FACTOR = 2 x the same error of the oracle's autograd at float16 (the reference's own
precision), per loss.  Every test prints its figures on lines that start with "promptfit-parity:"; profiles/promptfit_parity.txt is one
run's lines."""
import functools
import math

import numpy as np
import pytest
import torch

import coopfit_ref as ref
import promptfit_ref as pref

pytestmark = pytest.mark.gpu

from clip_calibration_amd import coopfit, ops, synthetic as syn  # noqa: E402
from clip_calibration_amd.model import build_model  # noqa: E402
from clip_calibration_amd.trainers import kgcoop, prograd  # noqa: E402

FACTOR = 2.0
GRAD_SCALE = 256.0          # as tests/test_gpu_coopfit.py: the synthetic weights give gradients far larger than ViT-B/16's
U32 = 2.0 ** -24
W = 8.0


def say(line):
    print("promptfit-parity: " + line)


def ident(v):
    return "-".join(str(x) for x in v) if isinstance(v, tuple) else str(v)


@functools.lru_cache(maxsize=None)
def model(geom):
    return build_model(dict(ref.state_dict(geom)), {"trainer": "CoOp"}).cuda()


@functools.lru_cache(maxsize=None)
def oracle(key, teacher="random", eta=0.05, T=1.0):
    """(case, float64 parts, float16 parts, how the float16 ones were made), computed once per case."""
    c = pref.case(key, teacher, eta)
    args = (c["sd"], c["ids"], c["ctx"], c["feats"], c["labels"], c["teacher"], W, T)
    yard, how = pref.yardstick_parts(*args)
    return c, pref.oracle_parts(*args), yard, how


def device_parts(c, geom, method, **kw):
    kw.setdefault("grad_scale", GRAD_SCALE)
    loss, grad, parts = coopfit.context_gradient(model(geom), c["ids"], c["ctx"], c["feats"].cuda(), c["labels"], ref.LOGIT_SCALE, method=method,
                                                 teacher=c["teacher"].cuda(), return_parts=True, **kw)
    return float(loss.cpu()[0]), grad.cpu(), {k: v.cpu() for k, v in parts.items()}


# ------------------------------------------------------------------------------------------------------------------- 1. the head
@pytest.mark.parametrize("w,T", [(8.0, 1.0), (0.0, 2.0)])
@pytest.mark.parametrize("strided", [False, True])
@pytest.mark.parametrize("B,C,E", ref.HEAD_CASES)
def test_prompt_head(B, C, E, strided, w, T):
    g = torch.Generator().manual_seed(B * 100 + C)
    wide = torch.randn(B, E + 24, generator=g)
    f = wide[:, 8:8 + E]
    text = torch.randn(C, E, generator=g) * 0.3
    teacher = torch.randn(C, E, generator=g) * 2.0           # not normalised: the head does that
    y = torch.randint(0, C, (B,), generator=g)
    scale, gs = 100.0, 4.0
    kg64 = pref.kgcoop_head(f.double(), y, text.double(), teacher.double(), scale, w)
    kg32 = pref.kgcoop_head(f.float().contiguous(), y, text, teacher, scale, w)
    pg64 = pref.prograd_head(f.double(), y, text.double(), teacher.double(), scale, T)
    pg32 = pref.prograd_head(f.float().contiguous(), y, text, teacher, scale, T)
    fd = wide.cuda()[:, 8:8 + E] if strided else f.contiguous().cuda()
    # The yardstick of test_coop_head: 4 x the distance of torch's fp32 evaluation from float64.  Its floors: a logit carries about eight
    # fp32 roundings, dz = 8 u scale; a cross-entropy moves by at most 2 dz and every gradient entry by at most 2 dz of the largest entry
    # (test_coop_head's derivation).  A cosine of two normalised rows carries the same eight roundings without the scale: 8 u per class,
    # so the score's floor is 8 u and the total's 2 dz + w 8 u; its gradient term is below the cross-entropy's floor.  The distillation
    # loss T^2 sum_c p_tea (log S - (z - m) / T): softmax(z / T) moves by 2 dz / T relative, so p_tea's move weighs at most max |log p|
    # and log p's own move 2 dz / T: 2 dz T (1 + max |log softmax(z / T)|), the maximum taken from the float64 restatement.  dz_kl =
    # T (p - p_tea) / B moves by 2 dz (p + p_tea) / B, twice a cross-entropy entry's move: 4 dz of the larger of the two gradients' largest
    # entries (p - p_tea may cancel, its error does not).
    dz = 8 * U32 * scale
    z64 = scale * pref.unit(f.double()) @ pref.unit(text.double()).t()
    max_logp = float(torch.log_softmax(z64 / T, dim=-1).abs().max())

    def tol(v32, v64, floor):
        return max(4 * float((torch.as_tensor(v32).double() - v64).abs().max()), floor)

    def err(got, v64):
        return float((got.double() - v64).abs().max())

    losses, d_text, none = ops.prompt_head(fd, y.cuda(), text.cuda(), scale, gs, "kgcoop", teacher.cuda(), w, T)
    assert none is None
    losses = losses.cpu()
    tols = [tol(kg32[0], kg64[0], 2 * dz + w * 8 * U32), tol(kg32[1], kg64[1], 2 * dz), tol(kg32[2], kg64[2], 8 * U32)]
    tol_d = tol(kg32[3], kg64[3], 2 * dz * float(kg64[3].abs().max()))
    errs = [err(losses[i], kg64[i]) for i in range(3)]
    err_d = err(d_text.cpu() / gs, kg64[3])
    say(f"head kgcoop B={B} C={C} E={E} strided={strided} w={w}: d(total, ce, score) " + ", ".join(f"{e:.2e} (tol {t:.2e})" for e, t in zip(errs, tols)) +
        f"; dgrad {err_d:.2e} (tol {tol_d:.2e})")
    assert all(e <= t for e, t in zip(errs, tols)) and err_d <= tol_d
    if w == 0.0:
        coop_loss, coop_d = ops.coop_head(fd, y.cuda(), text.cuda(), scale, gs)
        assert torch.equal(d_text, coop_d) and torch.equal(losses[1:2], coop_loss.cpu())     # w = 0 is CoOp's head, bit for bit
    again = ops.prompt_head(fd, y.cuda(), text.cuda(), scale, gs, "kgcoop", teacher.cuda(), w, T)
    assert torch.equal(again[0].cpu(), losses) and torch.equal(again[1], d_text)              # the same inputs, the same bits

    losses, d_xe, d_kl = ops.prompt_head(fd, y.cuda(), text.cuda(), scale, gs, "prograd", teacher.cuda(), w, T)
    losses = losses.cpu()
    big = max(float(pg64[2].abs().max()), float(pg64[3].abs().max()))
    tols = [tol(pg32[0], pg64[0], 2 * dz), tol(pg32[1], pg64[1], 2 * dz * T * (1 + max_logp)), tol(pg32[2], pg64[2], 2 * dz * float(pg64[2].abs().max())),
            tol(pg32[3], pg64[3], 4 * dz * big)]
    errs = [err(losses[0], pg64[0]), err(losses[1], pg64[1]), err(d_xe.cpu() / gs, pg64[2]), err(d_kl.cpu() / gs, pg64[3])]
    say(f"head prograd B={B} C={C} E={E} strided={strided} T={T}: d(xe, kl, grad_xe, grad_kl) " +
        ", ".join(f"{e:.2e} (tol {t:.2e})" for e, t in zip(errs, tols)))
    assert all(e <= t for e, t in zip(errs, tols))
    coop_loss, coop_d = ops.coop_head(fd, y.cuda(), text.cuda(), scale, gs)
    assert torch.equal(d_xe, coop_d) and torch.equal(losses[0:1], coop_loss.cpu())            # the cross-entropy half is CoOp's head
    again = ops.prompt_head(fd, y.cuda(), text.cuda(), scale, gs, "prograd", teacher.cuda(), w, T)
    assert torch.equal(again[0].cpu(), losses) and torch.equal(again[1], d_xe) and torch.equal(again[2], d_kl)


def test_prompt_head_bad_label_and_zero_teacher_row_poison():
    g = torch.Generator().manual_seed(2)
    f, text, teacher = (torch.randn(n, 64, generator=g).cuda() for n in (4, 3, 3))
    bad = torch.tensor([0, 5, 1, -1]).cuda()
    losses, d_text, _ = ops.prompt_head(f, bad, text, 100.0, 1.0, "kgcoop", teacher)
    assert torch.isnan(losses.cpu()[:2]).all() and torch.isnan(d_text.cpu()).any()
    losses, d_xe, d_kl = ops.prompt_head(f, bad, text, 100.0, 1.0, "prograd", teacher)
    assert torch.isnan(losses.cpu()[0]) and torch.isnan(d_xe.cpu()).any()
    assert torch.isfinite(losses.cpu()[1]) and torch.isfinite(d_kl.cpu()).all()                # the labels reach xe only
    teacher[1] = 0.0
    losses, d_text, _ = ops.prompt_head(f, torch.tensor([0, 2, 1, 1]).cuda(), text, 100.0, 1.0, "kgcoop", teacher)
    d = d_text.cpu()
    assert torch.isnan(losses.cpu()[0]) and torch.isnan(d[1]).all() and torch.isfinite(d[0]).all() and torch.isfinite(d[2]).all()


# ------------------------------------------------------------------------------------------------------- 2. the context gradients
@pytest.mark.parametrize("seq_rows", [None, 0], ids=["cut", "full"])
@pytest.mark.parametrize("key", ref.GRADIENT_CASES, ids=ident)
def test_context_gradients_against_float64(key, seq_rows):
    c, want, yard, how = oracle(key)
    loss, grad, parts = device_parts(c, key[0], "kgcoop", seq_rows=seq_rows, w=W)
    y = ref.rel_fro(yard["grad_kgcoop"], want["grad_kgcoop"])
    e = ref.rel_fro(grad, want["grad_kgcoop"])
    say(f"gradient kgcoop {key} seq_rows={seq_rows} loss {loss:.6f} vs {want['kgcoop']:.6f} (ce {float(parts['ce']):.6f}, score {float(parts['score']):.6f}); "
        f"rel. Frobenius error {e:.3e}, yardstick ({how}) {y:.3e}, ratio {e / y:.2f}")
    assert grad.shape == c["ctx"].shape and torch.isfinite(grad).all()
    assert abs(loss - want["kgcoop"]) <= FACTOR * y * max(1.0, abs(want["kgcoop"]))
    assert abs(float(parts["ce"]) - want["ce"]) <= FACTOR * y * max(1.0, abs(want["ce"])) and abs(float(parts["score"]) - want["score"]) <= FACTOR * y
    assert e <= FACTOR * y
    loss, grad, parts = device_parts(c, key[0], "prograd", seq_rows=seq_rows)
    assert loss == float(parts["xe"]) and grad.shape == c["ctx"].shape
    for name in ("xe", "kl"):
        y = ref.rel_fro(yard["grad_" + name], want["grad_" + name])
        e = ref.rel_fro(parts["grad_" + name], want["grad_" + name])
        say(f"gradient prograd {name} {key} seq_rows={seq_rows} loss {float(parts[name]):.6f} vs {want[name]:.6f}; rel. Frobenius error {e:.3e}, "
            f"yardstick ({how}) {y:.3e}, ratio {e / y:.2f}")
        assert torch.isfinite(parts["grad_" + name]).all()
        assert abs(float(parts[name]) - want[name]) <= FACTOR * y * max(1.0, abs(want[name]))
        assert e <= FACTOR * y


# --------------------------------------------------------------------------------------------------------- 3. ProGrad's decision
def projected_yardstick(want, yard, lam):
    """(float64 applied gradient, its decision, the float16 oracle's distance from it)."""
    g64, did = pref.project(want["grad_xe"], want["grad_kl"], lam)
    g16, _ = pref.project(yard["grad_xe"], yard["grad_kl"], lam)
    return g64, did, ref.rel_fro(g16, g64)


@pytest.mark.parametrize("lam", [1.0, 0.5])
@pytest.mark.parametrize("key,eta", pref.CONFLICT_CASES, ids=ident)
def test_prograd_projects_when_the_gradients_conflict(key, eta, lam):
    """The applied gradient g = a - lam (a.b / b.b) b has g.b = (1 - lam) a.b, so cos(g, b) = (1 - lam) cos(a, b) |a| / |g|: zero at
    lam = 1.  (|a| / |g| is 1 only at lam = 0; it is taken from the float64 oracle.)"""
    c, want, yard, how = oracle(key, "conflict", eta)
    cos64 = pref.cosine(want["grad_xe"], want["grad_kl"])
    assert cos64 <= -pref.MIN_ABS_COS, cos64                    # the float64 reference is well away from the boundary
    g64, did, y = projected_yardstick(want, yard, lam)
    assert did
    _, grad, parts = device_parts(c, key[0], "prograd", lam=lam)
    a, b = parts["grad_xe"].double(), parts["grad_kl"].double()
    dots = parts["dots"].numpy()
    e = ref.rel_fro(grad, g64)
    cos_gb = pref.cosine(grad.double(), b)
    target = (1.0 - lam) * cos64 * float(want["grad_xe"].norm() / g64.norm())
    say(f"decision conflict {key} eta={eta} lam={lam}: cos(a, b) {pref.cosine(a, b):+.4f} vs {cos64:+.4f}, projected {int(parts['projected'])}; applied gradient "
        f"error {e:.3e}, yardstick ({how}) {y:.3e}, ratio {e / y:.2f}; cos(g, b) {cos_gb:+.3e} vs {target:+.3e}")
    assert int(parts["projected"]) == 1
    aa, bb, ab = float((a * a).sum()), float((b * b).sum()), float((a * b).sum())
    assert np.allclose(dots, [aa, bb, ab], rtol=1e-12, atol=1e-12 * math.sqrt(aa * bb))      # float64 sums of the fp32 a and b
    assert e <= FACTOR * y
    assert abs(cos_gb - target) <= FACTOR * y


@pytest.mark.parametrize("key", pref.AGREE_CASES, ids=ident)
def test_prograd_keeps_the_gradient_when_they_agree(key):
    c, want, yard, how = oracle(key)
    cos64 = pref.cosine(want["grad_xe"], want["grad_kl"])
    assert cos64 >= pref.MIN_ABS_COS, cos64
    g64, did, y = projected_yardstick(want, yard, 1.0)
    assert not did
    _, grad, parts = device_parts(c, key[0], "prograd")
    e = ref.rel_fro(grad, g64)
    say(f"decision agree {key}: cos(a, b) {pref.cosine(parts['grad_xe'].double(), parts['grad_kl'].double()):+.4f} vs {cos64:+.4f}, projected "
        f"{int(parts['projected'])}; applied gradient error {e:.3e}, yardstick ({how}) {y:.3e}, ratio {e / y:.2f}")
    assert int(parts["projected"]) == 0 and torch.equal(grad, parts["grad_xe"])
    assert e <= FACTOR * y


@pytest.mark.parametrize("key", [("tiny", 3, 4, 8, False), ("tiny3", 37, 4, 1, True)], ids=ident)
def test_prograd_with_its_own_features_as_teacher_is_coop(key):
    """The teacher is the device's own text features, bit for bit, and T = 1: student and teacher logits are the same bits, the
    distillation gradient is exactly zero, nothing is projected (the reference's comparison is NaN < 0) and the step is CoOp's."""
    c = dict(ref.make_case(*key))
    m = model(key[0])
    c["teacher"] = coopfit.text_features(m, c["ids"], c["ctx"]).cpu()
    _, grad, parts = device_parts(c, key[0], "prograd")
    assert float(parts["grad_kl"].abs().max()) == 0.0 and float(parts["dots"][1]) == 0.0 and float(parts["dots"][2]) == 0.0
    assert int(parts["projected"]) == 0
    f, y, lr = c["feats"].cuda(), c["labels"].cuda(), torch.tensor([2e-3]).cuda()
    opt = dict(momentum=0.9, weight_decay=5e-4, grad_scale=GRAD_SCALE)
    coop = coopfit.CoOpFitState(m, c["ids"], c["ctx"], ref.LOGIT_SCALE, **opt)
    loss_c = coop.step(f, y, lr, want_loss=True)
    for one_call in (False, True):
        pg = coopfit.CoOpFitState(m, c["ids"], c["ctx"], ref.LOGIT_SCALE, method="prograd", teacher=c["teacher"].cuda(), **opt)
        loss_p = pg.step(f, y, lr, want_loss=True, one_call=one_call)
        assert torch.equal(pg.ctx, coop.ctx) and torch.equal(pg.buf, coop.buf) and torch.equal(loss_p, loss_c)
    assert not torch.equal(coop.ctx.cpu(), c["ctx"])


# ------------------------------------------------------------------------------------------------------------------ 4. three steps
RATES = [2e-3, 1e-3, 5e-4]
SGD = dict(momentum=0.9, dampening=0.0, nesterov=False, weight_decay=5e-4)


def three_steps(c, geom, how, method, **kw):
    m = model(geom)
    f, y = c["feats"].cuda(), c["labels"].cuda()
    kw = dict(kw, method=method, teacher=c["teacher"].cuda(), grad_scale=GRAD_SCALE, **SGD)
    if how == "fit":
        ctx, hist = coopfit.fit_context(f, c["labels"], m, c["ids"], c["ctx"], epochs=3, batch_size=f.shape[0], lr_per_epoch=RATES, return_history=True, **kw)
        return ctx.cpu(), hist
    st = coopfit.CoOpFitState(m, c["ids"], c["ctx"], ref.LOGIT_SCALE, **kw)
    lr = torch.tensor(RATES, dtype=torch.float32).cuda()
    losses = [st.step(f, y, lr[k:k + 1], want_loss=True, one_call=(how == "one_call")) for k in range(3)]
    return st.ctx.cpu(), torch.cat(losses).cpu().numpy()


TRAJECTORIES = [("kgcoop", ("tiny", 3, 4, 8, False), "random"), ("kgcoop", ("tiny3", 37, 4, 1, True), "random"),
                ("prograd", ("tiny", 3, 4, 8, False), "random"), ("prograd", ("tiny3", 37, 4, 1, True), "random"),
                ("prograd", ("tiny", 3, 4, 8, False), "conflict")]


@pytest.mark.parametrize("method,key,teacher", TRAJECTORIES, ids=ident)
def test_three_steps_same_bits_every_way(method, key, teacher):
    c = pref.case(key, teacher)
    a, la = three_steps(c, key[0], "step", method)
    b, lb = three_steps(c, key[0], "fit", method)
    d, ld = three_steps(c, key[0], "one_call", method)
    e, le = three_steps(c, key[0], "step", method)
    assert torch.isfinite(a).all() and not torch.equal(a, c["ctx"])
    assert torch.equal(a, b) and np.array_equal(la, lb)
    assert torch.equal(a, d) and np.array_equal(la, ld)
    assert torch.equal(a, e) and np.array_equal(la, le)          # two runs, the same bits


def float64_trajectory(c, method, lam=1.0):
    """(the context after three float64 SGD steps on the oracle, the smallest |cos(a, b)| met on the way (ProGrad))."""
    w, buf, least = c["ctx"].double(), None, math.inf
    for k, lr in enumerate(RATES):
        p = pref.oracle_parts(c["sd"], c["ids"], w, c["feats"], c["labels"], c["teacher"], W, 1.0, which=(method,))
        if method == "kgcoop":
            grad = p["grad_kgcoop"]
        else:
            least = min(least, abs(pref.cosine(p["grad_xe"], p["grad_kl"])))
            grad, _ = pref.project(p["grad_xe"], p["grad_kl"], lam)
        w, buf = ref.sgd_step(w, buf, grad, lr, SGD["momentum"], SGD["dampening"], SGD["weight_decay"], SGD["nesterov"], k == 0)
    return w, least


# (method, key, teacher, eta).  ProGrad's cases are those on which the float64 oracle keeps |cos(a, b)| >= 0.1 over all three steps,
# measured on the CPU: -0.66, -0.33, -0.37 with the conflicting teacher and +0.90, +0.71, +0.76 with the agreeing one.  (On
# ("tiny", 3, 4, 8, False), the CoOp test's case, both teachers pass within 0.05 of the boundary by the third step.)
FLOAT64_TRAJECTORIES = [("kgcoop", ("tiny", 3, 4, 8, False), "random", 0.05), ("prograd", ("tiny", 37, 4, 33, False), "random", 0.05),
                        ("prograd", ("tiny3", 3, 16, 33, False), "conflict", 0.05)]


def test_three_steps_against_float64_sgd():
    """Three SGD steps with momentum and weight decay follow float64 SGD on the oracle within 3 x the single-gradient bound, relative to
    the distance the context travels (the CoOp test's rule).  ProGrad's decision is discontinuous: a trajectory on which the oracle's
    |cos(a, b)| falls under 0.1 is not compared (the reason is printed); at most one of the two may go that way."""
    skipped = 0
    for method, key, teacher, eta in FLOAT64_TRAJECTORIES:
        c, want, yard, _ = oracle(key, teacher, eta)
        if method == "kgcoop":
            y = ref.rel_fro(yard["grad_kgcoop"], want["grad_kgcoop"])
        else:
            y = projected_yardstick(want, yard, 1.0)[2]
        w, least = float64_trajectory(c, method)
        if method == "prograd" and least < pref.MIN_ABS_COS:
            say(f"three steps {method} {teacher} {key}: not compared, the oracle's |cos(a, b)| falls to {least:.3f} < {pref.MIN_ABS_COS}")
            skipped += 1
            continue
        got, _ = three_steps(c, key[0], "step", method)
        moved = float((w - c["ctx"].double()).norm())
        e = float((got.double() - w).norm()) / moved
        say(f"three steps {method} {teacher} {key}: error {e:.3e} of the distance travelled, yardstick {y:.3e}" +
            (f", least |cos(a, b)| {least:.3f}" if method == "prograd" else ""))
        assert e <= 3 * FACTOR * y
    assert skipped <= 1


# --------------------------------------------------------------------------------------------------------------------- 5. trainers
def separable_batch(C, E, per_class, seed=0):
    g = torch.Generator().manual_seed(seed)
    centres = torch.randn(C, E, generator=g)
    labels = torch.arange(C).repeat_interleave(per_class)
    return centres[labels] + 0.1 * torch.randn(C * per_class, E, generator=g), labels


def fit_trainer(clip, m, **kw):
    """fit_context on the separable batch; the loader's "images" are the features themselves, passed through by a stand-in for the
    image tower, so that the trainer's own plumbing runs as it does with images (tests/test_gpu_coopfit.py)."""
    feats, labels = separable_batch(3, 128, 8)
    loader = [(feats.cuda(), labels)]
    try:
        m.image_features_f32 = lambda image: image
        return clip.fit_context(loader, epochs=20, lr=0.002, lr_per_epoch=[0.002] * 20, batch_size=24, momentum=0.9, weight_decay=5e-4,
                                grad_scale=GRAD_SCALE, return_history=True, **kw)
    finally:
        del m.image_features_f32


@pytest.mark.parametrize("which", ["kgcoop", "prograd"])
def test_trainer_fit_context_lowers_the_loss(which):
    m = model("tiny")
    ids, ids_zs = ref.prompt_ids("tiny", 3, 4), syn.synthetic_token_ids(3, "tiny", seed=7)
    mod = kgcoop if which == "kgcoop" else prograd
    clip = mod.CustomCLIP(m, ids, zeroshot_tokenized_prompts=ids_zs, n_ctx=4)
    before_ctx = clip.prompt_learner.ctx.detach().clone()
    before_text = clip.text_features().clone()
    fitted, hist = fit_trainer(clip, m)
    say(f"{which}.CustomCLIP.fit_context: loss {hist[0]:.5f} -> {hist[-1]:.5f} over {len(hist)} steps")
    assert len(hist) == 20 and np.isfinite(hist).all() and hist[-1] < hist[0]
    assert torch.equal(clip.prompt_learner.ctx.detach().float().cpu(), fitted.to(clip.prompt_learner.ctx.dtype).float().cpu())
    assert not torch.equal(clip.prompt_learner.ctx.detach(), before_ctx)
    assert not torch.equal(clip.text_features(), before_text)          # the cache retired with the parameter's version


def test_kgcoop_weight_holds_the_features_near_the_zero_shot_ones():
    m = model("tiny")
    ids, ids_zs = ref.prompt_ids("tiny", 3, 4), syn.synthetic_token_ids(3, "tiny", seed=7)
    near = {}
    for w in (64.0, 0.0):
        clip = kgcoop.CustomCLIP(m, ids, zeroshot_tokenized_prompts=ids_zs, n_ctx=4, w=w)
        fit_trainer(clip, m)
        near[w] = float((clip.text_features() * clip.ori_embedding).sum(-1).mean())
    say(f"kgcoop mean cosine to ori_embedding after 20 steps: w=64 {near[64.0]:.5f}, w=0 {near[0.0]:.5f}")
    assert near[64.0] > near[0.0]


def test_trainers_without_zero_shot_prompts_refuse():
    m = model("tiny")
    ids = ref.prompt_ids("tiny", 3, 4)
    with pytest.raises(ValueError, match="zeroshot_tokenized_prompts"):
        kgcoop.CustomCLIP(m, ids, n_ctx=4).fit_context([])
    with pytest.raises(ValueError, match="zeroshot_tokenized_prompts"):
        prograd.CustomCLIP(m, ids, n_ctx=4).fit_context([])


# ------------------------------------------------------------------------------------------------------------ 6. defaults unchanged
@pytest.mark.parametrize("key", [("tiny", 3, 4, 8, False), ("tiny3", 37, 4, 1, True)], ids=ident)
def test_coop_defaults_are_unchanged(key):
    c = ref.make_case(*key)
    m = model(key[0])
    f, y = c["feats"].cuda(), c["labels"].cuda()
    lr = torch.tensor(RATES, dtype=torch.float32).cuda()
    out = []
    for kw in ({}, {"method": "coop"}, {"method": "coop", "teacher": None, "w": 3.0, "T": 2.0, "lam": 0.5}):
        for one_call in (False, True):
            st = coopfit.CoOpFitState(m, c["ids"], c["ctx"], ref.LOGIT_SCALE, grad_scale=GRAD_SCALE, **SGD, **kw)
            losses = [st.step(f, y, lr[k:k + 1], want_loss=True, one_call=one_call) for k in range(3)]
            out.append((st.ctx.cpu(), torch.cat(losses).cpu()))
    for ctx, losses in out[1:]:
        assert torch.equal(ctx, out[0][0]) and torch.equal(losses, out[0][1])
    loss, grad = coopfit.context_gradient(m, c["ids"], c["ctx"], f, c["labels"], ref.LOGIT_SCALE, grad_scale=GRAD_SCALE)
    loss2, grad2, parts = coopfit.context_gradient(m, c["ids"], c["ctx"], f, c["labels"], ref.LOGIT_SCALE, grad_scale=GRAD_SCALE, method="coop",
                                                   return_parts=True)
    assert torch.equal(loss, loss2) and torch.equal(grad, grad2) and parts == {}
