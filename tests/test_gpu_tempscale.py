"""TempScaling's fit on the GPU (csrc/tempscale.hip, clip_calibration_amd/tempfit.py) against the float64 restatement of
tests/tempscale_ref.py, which tests/test_tempscale_cpu.py holds to torch's own step.  Every test prints its measured figures on lines
that start with "tempscale-parity:"; profiles/tempscale_parity.txt is one run's lines."""
import functools
import math

import numpy as np
import pytest
import torch

import tempscale_ref as ref

pytestmark = pytest.mark.gpu

from clip_calibration_amd import ops, tempfit  # noqa: E402

INIT = 4.6052
SCHED = ref.cosine_warmup_schedule(0.005, 3)   # 1e-5 for the warm-up epoch, then 0.00375 and 0.00125
FLOOR_ULP = 4                                  # the floor of the fit tolerance, in fp32 ulp of theta (test_fit_* docstring)


def cuda(a):
    return torch.from_numpy(np.array(a)).cuda()             # a copy: the cached cases are read-only


def say(line):
    print("tempscale-parity: " + line)


@functools.lru_cache(maxsize=None)
def case(n, C, seed=11, label_is_argmax=0.7):
    c, y = ref.make_case(n, C, seed, label_is_argmax)
    c.setflags(write=False)
    y.setflags(write=False)
    return c, y


def device_batch(c, y, theta, rows=None, wide=0):
    if wide:
        buf = torch.full((c.shape[0], c.shape[1] + wide), 7.0, dtype=torch.float32).cuda()   # what lies behind a row must not be read
        buf[:, :c.shape[1]] = cuda(c)
        ct = buf[:, :c.shape[1]]
        assert ct.stride(0) == c.shape[1] + wide
    else:
        ct = cuda(c)
    out = ops.tempscale_batch(ct, cuda(y), torch.tensor([theta], dtype=torch.float32).cuda(), None if rows is None else cuda(rows))
    return [float(v) for v in out.cpu()]


@pytest.mark.parametrize("theta", [0.0, INIT, 6.5])
@pytest.mark.parametrize("rows,C,wide", [(1, 2, 0), (3, 37, 0), (32, 100, 0), (100, 500, 0), (7, 1000, 0), (64, 1001, 0), (32, 100, 11)])
def test_batch_entry(rows, C, wide, theta):
    """One batch's (mean loss, mean d loss / d theta) against the float64 restatement at the same fp32 theta, inside the first-order bound
    that tests/tempscale_ref.py batch_error_bound derives from the kernel's arithmetic: each exponential's argument carries the roundings
    of s = expf(theta), of s c_j and of the subtraction of the maximum, __expf adds |z - max| 2^-24 relative per term, and the sums, logf,
    the division and the last operations add a few ulp.  theta = 6.5 is s = 665: exp(s c) overflows fp32 without the shift by the maximum.
    One shape reads its rows out of a wider matrix (ld = C + 11)."""
    c, y = case(rows, C)
    th = float(np.float32(theta))
    got = device_batch(c, y, th, wide=wide)
    want, bound = ref.batch_loss_grad(c, y, th), ref.batch_error_bound(c, y, th)
    err = [abs(g - w) for g, w in zip(got, want)]
    say(f"batch rows={rows} C={C} ld=C+{wide} theta={theta}: loss {want[0]:.6g} err {err[0]:.3e} (bound {bound[0]:.3e}), "
        f"grad {want[1]:.6g} err {err[1]:.3e} (bound {bound[1]:.3e})")
    assert all(math.isfinite(g) for g in got)
    assert err[0] <= bound[0] and err[1] <= bound[1]


@pytest.mark.parametrize("theta", [INIT, 6.5])
def test_batch_entry_where_every_label_is_the_argmax(theta):
    """Every row right: the gradient is a small difference of the row's mean cosine and the label's; the same bound, which is absolute."""
    c, y = case(64, 300, 12, 1.0)
    assert np.array_equal(c.argmax(axis=1), y)
    th = float(np.float32(theta))
    got = device_batch(c, y, th)
    want, bound = ref.batch_loss_grad(c, y, th), ref.batch_error_bound(c, y, th)
    say(f"batch all-argmax theta={theta}: loss {want[0]:.6g} err {abs(got[0] - want[0]):.3e} (bound {bound[0]:.3e}), "
        f"grad {want[1]:.6g} err {abs(got[1] - want[1]):.3e} (bound {bound[1]:.3e})")
    assert abs(got[0] - want[0]) <= bound[0] and abs(got[1] - want[1]) <= bound[1]


def test_batch_entry_takes_a_row_selection():
    c, y = case(100, 500)
    rows = np.array([99, 0, 41, 41, 7], np.int32)
    th = float(np.float32(INIT))
    got = device_batch(c, y, th, rows=rows)
    want, bound = ref.batch_loss_grad(c[rows], y[rows], th), ref.batch_error_bound(c[rows], y[rows], th)
    assert abs(got[0] - want[0]) <= bound[0] and abs(got[1] - want[1]) <= bound[1]


def _order(n, seed=5, epochs=3):
    rng = np.random.default_rng(seed)
    return np.stack([rng.permutation(n) for _ in range(epochs)]).astype(np.int32)


FIT_SHAPES = [(n, C, b, 0.9, 5e-4, False, "seq") for n in (257, 300) for C in (37, 500) for b in (1, 32, 100, None)]
FIT_OPTIM = [(300, 37, 32, m, wd, nes, "seq") for m, nes in ((0.0, False), (0.9, False), (0.9, True)) for wd in (0.0, 5e-4)
             if (m, wd, nes) != (0.9, 5e-4, False)]
FIT_BATCHING = [(300, 37, 128, 0.9, 5e-4, False, "drop_last"), (257, 500, 100, 0.9, 5e-4, False, "order"),
                (300, 37, 32, 0.9, 5e-4, True, "order")]


@functools.lru_cache(maxsize=None)
def fit_case(n, C, batch, momentum, weight_decay, nesterov, batching):
    """(kwargs, float64 restatement, torch's own fp32 CPU run of the same loop), computed once per case."""
    c, y = case(n, C)
    kw = dict(momentum=momentum, weight_decay=weight_decay, nesterov=nesterov, drop_last=batching == "drop_last",
              order=_order(n) if batching == "order" else None)
    return kw, ref.fit(c, y, INIT, SCHED, batch, **kw), ref.torch_fit(c, y, INIT, SCHED, batch, dtype="float32", **kw)


def device_fit(n, C, batch, kw):
    c, y = case(n, C)
    return tempfit.fit_logit_scale(cuda(c), y, init=INIT, epochs=3, batch_size=batch, lr_per_epoch=SCHED, return_history=True, **kw)


@pytest.mark.parametrize("n,C,batch,momentum,weight_decay,nesterov,batching", FIT_SHAPES + FIT_OPTIM + FIT_BATCHING)
def test_fit_is_the_restatement_within_torchs_own_fp32_distance(n, C, batch, momentum, weight_decay, nesterov, batching):
    """Three epochs on the device against the float64 restatement.  The tolerance is measured: d is the distance of torch's own fp32 CPU
    run of the same loop (F.cross_entropy, backward, SGD.step) from the restatement; the device, whose exp and whose fixed summation order
    are not torch's, gets 4 d plus a floor of FLOOR_ULP fp32 ulp of theta.  The ulp is that of the larger of |init| and |theta|: every
    step rounds theta where it then is, and the runs start at 4.6052 wherever they end.  The floor is there because d itself is the
    end of a walk of such roundings and is at times a small fraction of one ulp (batch = N: three steps, d = 0.14 ulp measured), which
    no other fp32 run can be held to; in the recorded run (profiles/tempscale_parity.txt) the largest ratio is 1.41, half of the cases
    end on torch's own bits and none needed the floor.  First and last entry of the loss history: the batch-entry bound, for the last entry plus |d loss / d theta| times the
    theta tolerance, since it is taken at the theta of the step before the last.  Two runs of the same inputs return the same bits."""
    batch = n if batch is None else batch
    kw, (theta64, losses64), (theta32, _) = fit_case(n, C, batch, momentum, weight_decay, nesterov, batching)
    theta, losses = device_fit(n, C, batch, kw)
    theta2, losses2 = device_fit(n, C, batch, kw)
    ulp = float(np.spacing(np.float32(max(abs(INIT), abs(theta64)))))
    d, dist = abs(theta32 - theta64), abs(theta - theta64)
    tol = 4 * d + FLOOR_ULP * ulp
    say(f"fit n={n} C={C} batch={batch} momentum={momentum} wd={weight_decay} nesterov={nesterov} {batching}: theta64 {theta64:.7f} "
        f"device {dist:.3e} ({dist / ulp:.2f} ulp)  torch-fp32 d {d:.3e} ({d / ulp:.2f} ulp)  ratio {dist / d if d else math.inf:.2f}  "
        f"tolerance {tol:.3e}")
    assert len(losses) == len(losses64) and losses.dtype == np.float32
    assert theta == theta2 and np.array_equal(losses, losses2)
    assert dist <= tol
    c, y = case(n, C)
    idx = list(ref.batches(n, batch, 3, kw["order"], kw["drop_last"]))
    first, last = idx[0][1], idx[-1][1]
    assert abs(float(losses[0]) - losses64[0]) <= ref.batch_error_bound(c[first], y[first], INIT)[0]
    # the restatement's theta before its last step: undo nothing, run it again without that step
    theta_before = _theta_before_last_step(n, C, batch, kw)
    slope = abs(ref.batch_loss_grad(c[last], y[last], theta_before)[1])
    assert abs(float(losses[-1]) - losses64[-1]) <= ref.batch_error_bound(c[last], y[last], theta_before)[0] + slope * tol


def _theta_before_last_step(n, C, batch, kw):
    c, y = case(n, C)
    c64 = np.asarray(c, np.float64)
    theta, buf, step = INIT, 0.0, 0
    steps = list(ref.batches(n, batch, 3, kw["order"], kw["drop_last"]))
    for e, idx in steps[:-1]:
        _, g = ref.batch_loss_grad(c64[idx], y[idx], theta)
        theta, buf = ref.sgd_step(theta, buf, step, g, SCHED[e], kw["momentum"], 0.0, kw["weight_decay"], kw["nesterov"])
        step += 1
    return theta


def test_fit_defaults_and_a_continued_state():
    """The default schedule is cosine_warmup_schedule(lr, epochs); a state carried over continues the run: two epochs and then one more
    (ops.tempscale_fit on the same state) give the bits of three epochs in one call."""
    c, y = case(300, 37)
    ct, yt = cuda(c), cuda(y)
    got = tempfit.fit_logit_scale(ct, yt, epochs=3, lr=0.005, batch_size=100)
    want = tempfit.fit_logit_scale(ct, yt, epochs=3, lr_per_epoch=tempfit.cosine_warmup_schedule(0.005, 3), batch_size=100)
    assert got == want
    lr = torch.tensor(np.repeat(np.asarray(SCHED, np.float32), 3)).cuda()
    whole = torch.tensor([INIT, 0, 0, 0], dtype=torch.float32).cuda()
    ops.tempscale_fit(ct, yt, whole, lr, 100, 3, momentum=0.9, weight_decay=5e-4)
    parts = torch.tensor([INIT, 0, 0, 0], dtype=torch.float32).cuda()
    ops.tempscale_fit(ct, yt, parts, lr[:6], 100, 2, momentum=0.9, weight_decay=5e-4)
    ops.tempscale_fit(ct, yt, parts, lr[6:].clone(), 100, 1, momentum=0.9, weight_decay=5e-4)
    assert torch.equal(whole.view(torch.int32), parts.view(torch.int32)) and int(whole.view(torch.int32)[2]) == 9
    assert float(whole[0]) == want


def test_fit_scale_end_to_end_equals_the_autograd_route():
    """The tiny geometry of test_tempscaling_sgd_step_matches_reference_gradient (12 images, 9 classes, CoOp cosine base):
    CustomCLIPCalibration.fit_scale over a loader of three batches for two epochs against the autograd route on the same batches on the
    GPU -- forward_train, F.cross_entropy, backward, torch.optim.SGD.step.  Tolerance as in the fit test, with the autograd route's fp32
    run in the place of the restatement: d is the distance of torch's fp32 CPU loop from the float64 restatement, both on the cosine
    logits the device formed.  scale_learner.logit_scale holds the result, forward applies exp of it, and no tower parameter acquires a
    gradient."""
    import torch.nn.functional as F
    from clip_calibration_amd import synthetic as syn
    from clip_calibration_amd.model import build_model
    from clip_calibration_amd.trainers import CoOpCLIP, CustomCLIPCalibration
    sd = syn.synthetic_state_dict("tiny", seed=0)
    model = build_model(dict(sd), {"trainer": "CoOp"}).cuda()
    Cn, B = 9, 12
    ids = syn.synthetic_token_ids(Cn, "tiny", seed=21, n_ctx_placeholders=4)
    images = syn.synthetic_images(B, "tiny", seed=21)
    labels = torch.arange(B) % Cn
    loader = [(images[i:i + 4], labels[i:i + 4]) for i in range(0, B, 4)]
    sched = [0.004, 0.002]
    opt_kw = dict(momentum=0.9, weight_decay=5e-4)
    base = CoOpCLIP(model, ids, n_ctx=4, logit_scale=1.0, seed=5)
    auto = CustomCLIPCalibration(base).cuda()
    opt = torch.optim.SGD(auto.scale_learner.parameters(), lr=1.0, **opt_kw)
    for lr in sched:
        opt.param_groups[0]["lr"] = lr
        for img, lab in loader:
            logits, _, _ = auto.forward_train(img.cuda())
            loss = F.cross_entropy(logits, lab.cuda())
            opt.zero_grad()
            loss.backward()
            opt.step()
    theta_auto = float(auto.scale_learner.logit_scale.detach())
    assert all(p.grad is None for p in model.parameters())
    calib = CustomCLIPCalibration(base).cuda()
    theta = calib.fit_scale(loader, epochs=2, lr_per_epoch=sched, batch_size=4, **opt_kw)
    assert isinstance(theta, float) and float(calib.scale_learner.logit_scale.detach()) == theta
    assert all(p.grad is None for p in model.parameters()) and calib.scale_learner.logit_scale.grad is None
    cosine = torch.cat([calib.cosine_logits(img.cuda())[0] for img, _ in loader]).cpu().numpy()
    theta64, _ = ref.fit(cosine, labels.numpy(), INIT, sched, 4, **opt_kw)
    theta32, _ = ref.torch_fit(cosine, labels.numpy(), INIT, sched, 4, dtype="float32", **opt_kw)
    ulp = float(np.spacing(np.float32(INIT)))
    d = abs(theta32 - theta64)
    tol = 4 * d + FLOOR_ULP * ulp
    say(f"end to end tiny: theta64 {theta64:.7f}  fit_scale {abs(theta - theta64):.3e}  autograd on the GPU {abs(theta_auto - theta64):.3e}  "
        f"torch-fp32 d {d:.3e}  fit_scale vs autograd {abs(theta - theta_auto):.3e}  tolerance {tol:.3e}")
    assert abs(theta - INIT) > 1e-4
    assert abs(theta - theta_auto) <= tol and abs(theta - theta64) <= tol
    img = images[:4].cuda()
    scaled = calib(img)[0]
    want = math.exp(theta) * calib.cosine_logits(img)[0]
    assert torch.allclose(scaled, want, rtol=1e-5, atol=1e-5)


def test_fit_temperature_takes_any_cosine_callable():
    from clip_calibration_amd import runner
    c, y = case(300, 37)
    ct = cuda(c)
    loader = [(torch.arange(i, min(i + 128, 300)), torch.from_numpy(y[i:i + 128].copy())) for i in range(0, 300, 128)]
    infer = lambda image: (ct[image], None, None)        # "images" are row numbers here
    got = runner.fit_temperature(infer, loader, epochs=3, lr_per_epoch=SCHED, batch_size=100)
    assert got == tempfit.fit_logit_scale(ct, y, epochs=3, lr_per_epoch=SCHED, batch_size=100)
