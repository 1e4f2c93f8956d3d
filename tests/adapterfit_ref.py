"""Oracle of CLIP-Adapter's training step (reference trainers/classification/clip_adapter.py:138-187) for the tests of
clip_calibration_amd/adapterfit.py and csrc/adapter_train.hip.  It does not import the package.

* ``torch_forward`` restates the forward in torch in a chosen dtype; ``torch_step`` takes its gradients from autograd and ``torch_fit``
  its steps from torch.optim.SGD.  In float64 that is the oracle; in float32 it is the yardstick of the device's tolerance.
* ``backward`` is the hand-derived backward the kernels implement, in numpy float64; tests/test_adapterfit_cpu.py holds it to autograd.
* ``kinks`` reports the (row, unit) pairs whose pre-activation sits at a ReLU's kink, and ``excluded`` the gradient entries that depend
  on their masks.
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

LOGIT_SCALE = 4.6052
KINK = 1e-4                 # a pre-activation below KINK * max|p| may have another sign in fp32 than in float64
FACTOR = 4.0                # the device may be FACTOR times as far from float64 as torch's fp32 CPU run is (for another, fixed summation
                            # order over up to 512 terms and for __expf; measured, profiles/adapterfit_parity.txt: ratios 0.20 to 3.18 over 20 of 21 one-step quantities, median 0.66, one of
                            # 12.3 where torch's run is within 0.2 ulp and the floor holds the device's 2 ulp; 0.43 to 1.00 over the
                            # trajectories: neither too tight nor absurdly loose, the factor stays) ...
FLOOR = 2.0 ** -22          # ... with a floor of FLOOR * max|value|, for entries where torch's fp32 happens to be exact

# (B, E, H, C) of the operator tests, each with the seed whose float64 pre-activations keep the excluded share below the cap
# (tests/test_adapterfit_cpu.py::test_seeds_keep_the_kink_exclusion_below_the_cap runs the same generator)
SHAPES = {(5, 64, 16, 3): 1, (33, 128, 32, 65): 13, (32, 512, 128, 100): 41, (1, 64, 16, 2): 1,
          # the kernel's other paths: H > 3 E (dh in a buffer of its own), H >= 1024 and E >= 1024 (one thread per column, no split of
          # the depth); the first two leave out the dW1 rows behind one and two hidden units at their kink
          (3, 64, 256, 4): 1, (2, 32, 1056, 3): 1, (2, 1040, 8, 3): 2}
EXCLUDED_CAP = 0.01


def scale_of(logit_scale=LOGIT_SCALE):
    """s = exp(logit_scale) as the host hands it to the kernels: rounded to fp32 once."""
    return float(np.float32(math.exp(logit_scale)))


def make_case(B, E, H, C, seed, label_is_argmax=0.5):
    """Seeded fp32 inputs: raw features f [B, E] ~ N(0, 1), labels y [B], L2-normalised text features T [C, E], W1 [H, E] ~ N(0, 1 / E),
    W2 [E, H] ~ N(0, 1 / H).  In a share ``label_is_argmax`` of the rows the label is the class whose text feature is closest to f."""
    rng = np.random.default_rng(seed)
    f = rng.normal(size=(B, E)).astype(np.float32)
    T = rng.normal(size=(C, E))
    T = (T / np.linalg.norm(T, axis=1, keepdims=True)).astype(np.float32)
    w1 = (rng.normal(size=(H, E)) / math.sqrt(E)).astype(np.float32)
    w2 = (rng.normal(size=(E, H)) / math.sqrt(H)).astype(np.float32)
    y = rng.integers(0, C, B).astype(np.int64)
    sharp = np.flatnonzero(rng.uniform(size=B) < label_is_argmax)
    y[sharp] = (f[sharp].astype(np.float64) @ T.astype(np.float64).T).argmax(axis=1)
    return dict(f=f, y=y, T=T, w1=w1, w2=w2)


def torch_forward(f, T, w1, w2, ratio, s):
    """(logits [B, C], p1 [B, H], p2 [B, E]) in the dtype of the operands."""
    p1 = f @ w1.t()
    p2 = torch.relu(p1) @ w2.t()
    g = ratio * torch.relu(p2) + (1 - ratio) * f
    u = g / g.norm(dim=-1, keepdim=True)
    return s * u @ T.t(), p1, p2


def _tensors(case, dtype):
    dt = getattr(torch, dtype)
    return tuple(torch.from_numpy(np.array(case[k])).to(dt) for k in ("f", "T", "w1", "w2")) + (torch.from_numpy(np.array(case["y"])),)


def torch_step(case, ratio, s, dtype="float64"):
    """One batch through torch's own autograd: dict of numpy arrays dw1, dw2 (of the mean loss), row_loss, p1, p2."""
    f, T, w1, w2, y = _tensors(case, dtype)
    w1.requires_grad_(True)
    w2.requires_grad_(True)
    z, p1, p2 = torch_forward(f, T, w1, w2, ratio, s)
    row_loss = F.cross_entropy(z, y, reduction="none")
    row_loss.mean().backward()
    return dict(dw1=w1.grad.numpy(), dw2=w2.grad.numpy(), row_loss=row_loss.detach().numpy(), p1=p1.detach().numpy(), p2=p2.detach().numpy())


def backward(case, ratio, s):
    """The hand-derived backward of csrc/adapter_train.hip in numpy float64: dict of dw1, dw2, row_loss."""
    f, T, w1, w2 = (np.asarray(case[k], np.float64) for k in ("f", "T", "w1", "w2"))
    y = np.asarray(case["y"])
    B = f.shape[0]
    p1 = f @ w1.T
    h = np.maximum(p1, 0.0)
    p2 = h @ w2.T
    a = np.maximum(p2, 0.0)
    g = ratio * a + (1 - ratio) * f
    n = np.linalg.norm(g, axis=1, keepdims=True)
    u = g / n
    z = s * u @ T.T
    m = z.max(axis=1, keepdims=True)
    e = np.exp(z - m)
    S = e.sum(axis=1, keepdims=True)
    row_loss = np.log(S[:, 0]) - (z[np.arange(B), y] - m[:, 0])
    dz = e / S
    dz[np.arange(B), y] -= 1.0
    dz /= B
    du = s * dz @ T
    dg = (du - u * (u * du).sum(axis=1, keepdims=True)) / n
    da = ratio * dg * (p2 > 0)
    dw2 = da.T @ h
    dh = (da @ w2) * (p1 > 0)
    dw1 = dh.T @ f
    return dict(dw1=dw1, dw2=dw2, row_loss=row_loss)


def kinks(p1, p2):
    """[("p1" | "p2", row, unit)] of the float64 pre-activations below KINK * max|p| of their matrix."""
    out = []
    for name, p in (("p1", p1), ("p2", p2)):
        rows, units = np.nonzero(np.abs(p) < KINK * np.abs(p).max())
        out += [(name, int(r), int(k)) for r, k in zip(rows, units)]
    return out


def excluded(kink_list, E, H):
    """Boolean masks (dw1 [H, E], dw2 [E, H]) of the gradient entries that depend on the ReLU mask of a unit in ``kink_list``: the mask
    of p1[b, k] gates dh[b, k], which feeds row k of dW1; the mask of p2[b, e] gates da[b, e], which feeds row e of dW2 and, through
    dh[b, :] = da[b, :] W2, every entry of dW1.  (The forward is continuous at a kink: losses and the other entries move by the size of
    the pre-activation, which is inside every tolerance here.)"""
    x1, x2 = np.zeros((H, E), bool), np.zeros((E, H), bool)
    for name, _, unit in kink_list:
        if name == "p1":
            x1[unit, :] = True
        else:
            x2[unit, :] = True
            x1[:, :] = True
    return x1, x2


def excluded_share(x1, x2):
    return (int(x1.sum()) + int(x2.sum())) / (x1.size + x2.size)


def batches(n, batch, epochs, order=None, drop_last=False):
    """Yields (epoch, sample indices): order[e, k * batch : (k + 1) * batch], order None = 0 .. n-1 in every epoch."""
    per_epoch = n // batch if drop_last else -(-n // batch)
    for e in range(epochs):
        idx = np.arange(n) if order is None else np.asarray(order)[e]
        for k in range(per_epoch):
            yield e, idx[k * batch:(k + 1) * batch]


def torch_fit(case, ratio, s, lr_per_epoch, batch, momentum=0.0, dampening=0.0, weight_decay=0.0, nesterov=False, order=None, drop_last=False,
              dtype="float64"):
    """The reference's loop on cached features by torch itself on the CPU in ``dtype``: forward, F.cross_entropy, backward,
    torch.optim.SGD.step on both matrices, the group's lr set per epoch.  Returns (w1, w2, [every step's batch loss]) as numpy."""
    f, T, w1, w2, y = _tensors(case, dtype)
    w1, w2 = torch.nn.Parameter(w1), torch.nn.Parameter(w2)
    opt = torch.optim.SGD([w1, w2], lr=1.0, momentum=momentum, dampening=dampening, weight_decay=weight_decay, nesterov=nesterov)
    losses = []
    for e, idx in batches(f.shape[0], batch, len(lr_per_epoch), order, drop_last):
        opt.param_groups[0]["lr"] = lr_per_epoch[e]
        idx = torch.from_numpy(np.ascontiguousarray(idx).astype(np.int64))
        loss = F.cross_entropy(torch_forward(f[idx], T, w1, w2, ratio, s)[0], y[idx])
        opt.zero_grad()
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    return w1.detach().numpy(), w2.detach().numpy(), np.asarray(losses)


def tolerance(torch32, oracle64, keep=None):
    """(tolerance, torch's own distance) for one compared quantity: FACTOR times the largest |torch fp32 - float64| over the compared
    entries, at least FLOOR * max|float64 value|."""
    want = np.asarray(oracle64, np.float64)
    d = np.abs(np.asarray(torch32, np.float64) - want)
    if keep is not None:
        d, want = d[keep], want[keep]
    dist = float(d.max()) if d.size else 0.0
    return max(FACTOR * dist, FLOOR * (float(np.abs(want).max()) if want.size else 0.0)), dist
