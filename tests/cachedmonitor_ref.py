"""The validation forwards of the CLIP-Adapter and TaskRes fits (clipmi_adapter_val_logits, clipmi_taskres_val_logits) restated in torch,
parameterised by dtype, with the element-wise bound on their fp32 logits.  Scoring and selection are tests/fitmonitor_ref.py's.  It does
not import the package's kernels.

The bound, u = 2^-24, is tests/cached_fit_ref.py's derivation for the two training forwards, taken up to the logits (that file keeps it
inside ``adapter_bound`` / ``taskres_bound``, tied to its own cases; the validation kernels run the same device code, so the rounding points
are the same) and evaluated on the float64 reference alone -- nothing the device returns enters it:

CLIP-Adapter, n64(n) = ceil(n / 64), wave_dot a lane-strided chain of n64 terms and a six-level tree, (n64 + 6) u sum |terms|:
  tp1 = (n64(E) + 6) u sum_e |w1 f|;  th = tp1 [p1 > -tp1];  tp2 = sum_k |w2| th + (n64(H) + 6) u sum_k |w2 h|;  ta = tp2 [p2 > -tp2];
  g = fl(fl(ratio a) + fl(fl(1 - ratio) f)):  tg = ratio ta + u |ratio a| + 2 u |(1 - ratio) f| + u |g|;
  n = sqrtf(wave sum of g^2):  en = ((n64(E) + 6) u + 2 sum |g| tg / n^2) / 2 + u;  u = fl(g / n):  tu = tg / n + (en + u) |u|;
  z_c = fl(scale wave_dot(T_c, u)):  tz = scale (sum_e |T_ce| tu_e + (n64(E) + 6) u sum_e |T u|) + u |z|.
TaskRes, n16 = ceil(E / 16):
  t_e = fl(base_e + fl(alpha r_e)):  tt = u (|alpha r| + |t|);  ef = ((n16 + 4) / 2 + 1) u;  en_c = ((n16 + 4) u + 2 sum |t| tt / n_c^2) / 2 + u;
  acc one fmaf chain of depth E:  tacc = E u sum |f t| + sum |f| tt;  z = fl(scale fl(fl(acc / nf) / n)):  tz = scale tacc / (nf n) + (3 u + ef + en_c) |z|.
ReLU is 1-Lipschitz, so the logits are continuous in the pre-activations: no entry is left out."""
import functools
import math

import numpy as np
import torch

import adapterfit_ref
import taskresfit_ref
from head_ref import U, ceil_div

RATIO = float(np.float32(0.2))
ALPHA = taskresfit_ref.ALPHA
W2_GAIN = 0.125            # tests/cached_fit_ref.py: the adapter's branch is the small correction to f it is when a fit starts


def adapter_logits(f, T, w1, w2, ratio, s, dtype=torch.float64):
    f, T, w1, w2 = (torch.from_numpy(np.array(v)).to(dtype) for v in (f, T, w1, w2))
    return adapterfit_ref.torch_forward(f, T, w1, w2, ratio, s)[0]


def taskres_logits(f, base, r, alpha, s, dtype=torch.float64):
    f, base, r = (torch.from_numpy(np.array(v)).to(dtype) for v in (f, base, r))
    return taskresfit_ref.torch_forward(f, base, r, alpha, s)


def _t64(a):
    return torch.from_numpy(np.array(a)).double()


def adapter_logits_bound(f, T, w1, w2, ratio, s):
    """(z float64 [N, C], tz) -- module docstring."""
    f, T, w1, w2 = _t64(f), _t64(T), _t64(w1), _t64(w2)
    E, H = f.shape[1], w1.shape[0]
    kE, kH = (ceil_div(E, 64) + 6) * U, (ceil_div(H, 64) + 6) * U
    p1 = f @ w1.t()
    tp1 = kE * (f.abs() @ w1.abs().t())
    h = p1.clamp(min=0)
    p2 = h @ w2.t()
    th = tp1 * (p1 > -tp1)
    tp2 = th @ w2.abs().t() + kH * (h @ w2.abs().t())
    a = p2.clamp(min=0)
    ta = tp2 * (p2 > -tp2)
    om = float(np.float32(1.0) - np.float32(ratio))
    g = ratio * a + (1 - ratio) * f
    tg = ratio * ta + U * (ratio * a).abs() + 2 * U * (om * f).abs() + U * g.abs()
    n = g.norm(dim=1, keepdim=True)
    en = (kE + 2 * (g.abs() * tg).sum(1, keepdim=True) / n ** 2) / 2 + U
    u = g / n
    tu = tg / n + (en + U) * u.abs()
    z = s * (u @ T.t())
    return z, abs(s) * (tu @ T.abs().t() + kE * (u.abs() @ T.abs().t())) + U * z.abs()


def taskres_logits_bound(f, base, r, alpha, s):
    """(z float64 [N, C], tz) -- module docstring."""
    f, base, r = _t64(f), _t64(base), _t64(r)
    E = f.shape[1]
    n16 = ceil_div(E, 16)
    t = base + alpha * r
    tt = U * ((alpha * r).abs() + t.abs())
    nf, n = f.norm(dim=1, keepdim=True), t.norm(dim=1, keepdim=True)
    ef = ((n16 + 4) / 2 + 1) * U
    en = ((n16 + 4) * U + 2 * (t.abs() * tt).sum(1, keepdim=True) / n ** 2) / 2 + U
    tacc = E * U * (f.abs() @ t.abs().t()) + f.abs() @ tt.t()
    z = s * (f @ t.t()) / nf / n.t()
    return z, abs(s) * tacc / nf / n.t() + (3 * U + ef + en.t()) * z.abs()


@functools.lru_cache(maxsize=None)
def adapter_val_case(N, E, H, C, seed=5):
    """Read-only fp32 inputs of one validation: f [N, E], T [C, E] normalised, W1, W2 at torch.nn.Linear's spread (W2 times W2_GAIN)."""
    c = adapterfit_ref.make_case(N, E, H, C, seed=seed)
    c["w1"] = (c["w1"] / math.sqrt(3.0)).astype(np.float32)
    c["w2"] = (c["w2"] * (W2_GAIN / math.sqrt(3.0))).astype(np.float32)
    for v in c.values():
        v.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def taskres_val_case(N, E, C, seed=5):
    c = taskresfit_ref.make_case(N, E, C, seed=seed)
    for v in c.values():
        v.setflags(write=False)
    return c


def clear_of_ties_and_edges(z64, tz, n_bins):
    """True when, in the float64 logits, every row's top-two margin exceeds twice the row's largest bound and its confidence lies further
    from every edge of linspace(0, 1, n_bins + 1) than that bound (|d conf| <= 2 conf (1 - conf) max|dz| <= max|dz| / 2): the device's fp32
    logits then give the float64 reference's arg-max and bin in every row."""
    z = np.asarray(z64, np.float64)
    d = np.asarray(tz, np.float64).max(axis=1)
    top = np.sort(z, axis=1)[:, -2:]
    if z.shape[1] > 1 and not bool(((top[:, 1] - top[:, 0]) > 2 * d).all()):
        return False
    m = z.max(axis=1, keepdims=True)
    conf = 1.0 / np.exp(z - m).sum(axis=1)
    edges = np.linspace(0, 1, n_bins + 1)
    return bool((np.abs(conf[:, None] - edges[None, :]) > d[:, None]).all())
