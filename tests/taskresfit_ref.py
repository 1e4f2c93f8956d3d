"""Oracle of TaskRes' training step (reference trainers/classification/taskres.py:96-210) for the tests of
clip_calibration_amd/taskresfit.py and csrc/taskres_train.hip.  It does not import the package.

* ``torch_forward`` restates the forward in torch in a chosen dtype; ``torch_step`` takes its gradient from autograd and ``torch_fit``
  its steps from torch.optim.Adam / torch.optim.SGD.  In float64 that is the oracle; in float32 it is the yardstick of the device's
  tolerance.
* ``backward`` is the hand-derived backward the kernels implement, in numpy float64, and ``adam_rule`` the optimiser rule of
  include/clipmi.h; tests/test_taskresfit_cpu.py holds both to torch.
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

LOGIT_SCALE = 4.6052
ALPHA = 0.5
FACTOR = 4.0                # the device may be FACTOR times as far from float64 as torch's fp32 CPU run is: tests/adapterfit_ref.py's rule and
                            # its factor, measured there for the same kind of arithmetic (fp32 dots of up to 512 terms in another fixed
                            # order, __expf).  Measured here (profiles/taskresfit_parity.txt): ratios 0.19 to 2.46 over the 14 one-step
                            # quantities (median 1.2), 1.00 to 1.33 over the 8 trajectory quantities: the factor stays ...
FLOOR = 2.0 ** -22          # ... with a floor of FLOOR * max|value|, for entries where torch's fp32 happens to be exact

# (B, E, C) of the operator tests: ragged E and C tiles, B below, across and at the batch tile of 64, the production E and B
SHAPES = ((1, 64, 2), (5, 64, 3), (3, 70, 5), (33, 128, 65), (40, 96, 130), (256, 512, 100))
# the CPU test of the formulas adds the production width at a full batch tile
CPU_SHAPES = SHAPES + ((64, 512, 100),)


def scale_of(logit_scale=LOGIT_SCALE):
    """s = exp(logit_scale) as the host hands it to the kernels: rounded to fp32 once."""
    return float(np.float32(math.exp(logit_scale)))


def make_case(B, E, C, seed, label_is_argmax=0.5, zero_residuals=False):
    """Seeded fp32 inputs: raw features f [B, E] ~ N(0, 1), base text features [C, E] ~ N(0, 1) (not normalised, as the mean of a class's
    template features is not), residuals r [C, E] ~ N(0, 0.1^2) (or zeros) and labels y [B].  In a share ``label_is_argmax`` of the rows
    the label is the class whose base + ALPHA * r is closest to f in cosine."""
    rng = np.random.default_rng(seed)
    f = rng.normal(size=(B, E)).astype(np.float32)
    base = rng.normal(size=(C, E)).astype(np.float32)
    r = np.zeros((C, E), np.float32) if zero_residuals else (0.1 * rng.normal(size=(C, E))).astype(np.float32)
    y = rng.integers(0, C, B).astype(np.int64)
    sharp = np.flatnonzero(rng.uniform(size=B) < label_is_argmax)
    t = base.astype(np.float64) + ALPHA * r
    y[sharp] = (f[sharp].astype(np.float64) @ (t / np.linalg.norm(t, axis=1, keepdims=True)).T).argmax(axis=1)
    return dict(f=f, y=y, base=base, r=r)


def torch_forward(f, base, r, alpha, s):
    """Logits [B, C] in the dtype of the operands."""
    x = f / f.norm(dim=-1, keepdim=True)
    t = base + alpha * r
    u = t / t.norm(dim=-1, keepdim=True)
    return s * x @ u.t()


def _tensors(case, dtype):
    dt = getattr(torch, dtype)
    return tuple(torch.from_numpy(np.array(case[k])).to(dt) for k in ("f", "base", "r")) + (torch.from_numpy(np.array(case["y"])),)


def torch_step(case, alpha, s, dtype="float64"):
    """One batch through torch's own autograd: dict of numpy arrays dr (of the mean loss), row_loss, z."""
    f, base, r, y = _tensors(case, dtype)
    r.requires_grad_(True)
    z = torch_forward(f, base, r, alpha, s)
    row_loss = F.cross_entropy(z, y, reduction="none")
    row_loss.mean().backward()
    return dict(dr=r.grad.numpy(), row_loss=row_loss.detach().numpy(), z=z.detach().numpy())


def backward(case, alpha, s):
    """The hand-derived backward of csrc/taskres_train.hip in numpy float64: dict of dr, row_loss, u."""
    f, base, r = (np.asarray(case[k], np.float64) for k in ("f", "base", "r"))
    y = np.asarray(case["y"])
    B = f.shape[0]
    x = f / np.linalg.norm(f, axis=1, keepdims=True)
    t = base + alpha * r
    n = np.linalg.norm(t, axis=1, keepdims=True)
    u = t / n
    z = s * x @ u.T
    m = z.max(axis=1, keepdims=True)
    e = np.exp(z - m)
    S = e.sum(axis=1, keepdims=True)
    row_loss = np.log(S[:, 0]) - (z[np.arange(B), y] - m[:, 0])
    dz = e / S
    dz[np.arange(B), y] -= 1.0
    dz /= B
    du = s * dz.T @ x
    dr = alpha * (du - u * (u * du).sum(axis=1, keepdims=True)) / n
    return dict(dr=dr, row_loss=row_loss, u=u)


def adam_rule(w, g, m, v, t, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0):
    """torch.optim.Adam's rule (no amsgrad) as include/clipmi.h states it, step number t >= 1: returns (w, m, v)."""
    b1, b2 = betas
    g = g + weight_decay * w
    m = m + (g - m) * (1 - b1)
    v = b2 * v + (1 - b2) * g * g
    w = w - (lr / (1 - b1 ** t)) * m / (np.sqrt(v) / math.sqrt(1 - b2 ** t) + eps)
    return w, m, v


def batches(n, batch, epochs, order=None, drop_last=False):
    """Yields (epoch, sample indices): order[e, k * batch : (k + 1) * batch], order None = 0 .. n-1 in every epoch."""
    per_epoch = n // batch if drop_last else -(-n // batch)
    for e in range(epochs):
        idx = np.arange(n) if order is None else np.asarray(order)[e]
        for k in range(per_epoch):
            yield e, idx[k * batch:(k + 1) * batch]


def torch_fit(case, alpha, s, lr_per_epoch, batch, optimizer="adam", betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, momentum=0.0, dampening=0.0,
              nesterov=False, order=None, drop_last=False, dtype="float64"):
    """The reference's loop on cached features by torch itself on the CPU in ``dtype``: forward, F.cross_entropy, backward, one
    torch.optim.Adam / SGD step on the residuals, the group's lr set per epoch.  Returns (r, [every step's batch loss]) as numpy."""
    f, base, r, y = _tensors(case, dtype)
    r = torch.nn.Parameter(r)
    if optimizer == "adam":
        opt = torch.optim.Adam([r], lr=1.0, betas=betas, eps=eps, weight_decay=weight_decay)
    else:
        opt = torch.optim.SGD([r], lr=1.0, momentum=momentum, dampening=dampening, weight_decay=weight_decay, nesterov=nesterov)
    losses = []
    for e, idx in batches(f.shape[0], batch, len(lr_per_epoch), order, drop_last):
        opt.param_groups[0]["lr"] = lr_per_epoch[e]
        idx = torch.from_numpy(np.ascontiguousarray(idx).astype(np.int64))
        loss = F.cross_entropy(torch_forward(f[idx], base, r, alpha, s), y[idx])
        opt.zero_grad()
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    return r.detach().numpy(), np.asarray(losses)


def tolerance(torch32, oracle64):
    """(tolerance, torch's own distance) for one compared quantity: FACTOR times the largest |torch fp32 - float64| over the compared
    entries, at least FLOOR * max|float64 value|."""
    want = np.asarray(oracle64, np.float64)
    d = np.abs(np.asarray(torch32, np.float64) - want)
    dist = float(d.max()) if d.size else 0.0
    return max(FACTOR * dist, FLOOR * (float(np.abs(want).max()) if want.size else 0.0)), dist
