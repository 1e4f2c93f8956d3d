"""What the row-score kernels (csrc/row_scores.hip) are held to: seeded inputs, the float64 restatement (clip_calibration_amd/metrics.py),
element-wise bounds derived from the fp32 format -- never from what the kernel gives -- and an fp32 emulation of the kernel's rounding
points on the CPU.

The kernel's arithmetic on a row of C logits z (all fp32, u = 2^-24 the unit roundoff; expf and logf are held to the OpenCL accuracy table
the device's math library follows, 3 ulp, which is a relative f = 6u at worst -- numpy's float32 exp and log, used by the emulation, are
no 1-ulp functions either):
  d_c = fl(z_c - m)                     m = max z exact;  |d_c| <= 2 zmax, so the ARGUMENT of exp is off by at most a = 2 zmax u
  e_c = expf(d_c)                       relative error a + f
  S   = sum_c e_c                       a lane adds ceil(C / 64) terms, then 6 butterfly steps: s = ceil(C / 64) + 6 roundings on the longest
                                        path, all terms positive: relative error (a + f) + s u =: eps_S
  nll = fl(logf(S) - fl(z_y - m))       |log S| <= log C:  eps_S + f log C  (the logarithm)  + a  (z_y - m)  + u |nll|  (the difference)
  p_c = fl(e_c * fl(1 / S))             relative error eps_p = (a + f) + eps_S + 2u
  brier = sum_c fl(fl(p_c - t_c)^2)     with g_c = p_c - t_c: each term is off by 2 |g_c| (eps_p p_c + u |g_c|) + u g_c^2, the sum by s u brier
For probabilities as given p is exact, nll = -logf(max(p_y, FLT_MIN)) is off by f |nll| and the Brier terms keep the u parts alone.
Second-order terms are dropped; they are below 1e-5 of the sums above at these sizes (a <= 2e-6) and SLACK = 1.01 covers them.
"""
import numpy as np

from clip_calibration_amd import metrics

U = 2.0 ** -24
F = 6 * U      # a 3-ulp function
SLACK = 1.01
NS = (1, 7, 64, 65, 257)
CS = (1, 2, 63, 64, 65, 257, 1000)
BINS = (1, 10, 15)
LOGIT_SPREAD = 2.5     # small enough that no seeded row puts a probability within fp32 rounding of 1.0


def case_seed(N, C):
    return 7919 * N + C


def case_inputs(N, C, from_probs=False):
    """(rows fp32 [N, C], labels int64 [N]) of the seeded case: logits ~ 2.5 N(0, 1) with a shifted label column, or, ``from_probs``, their
    float64 softmax times a per-row factor in [0.6, 1] -- calibrated rows need not sum to 1 -- rounded to fp32."""
    rng = np.random.default_rng(case_seed(N, C))
    z = LOGIT_SPREAD * rng.standard_normal((N, C))
    labels = rng.integers(0, C, N).astype(np.int64)
    z[np.arange(N), labels] += 1.5 * rng.uniform(size=N)
    z = z.astype(np.float32)
    if not from_probs:
        return z, labels
    p = metrics.row_probabilities(z) * rng.uniform(0.6, 1.0, (N, 1))
    return p.astype(np.float32), labels


def adds(C):
    return -(-C // 64) + 6


def eps_sum(C, zmax):
    return (2 * zmax * U + F) + adds(C) * U


def eps_prob(C, zmax, from_probs=False):
    """Relative error bound of one fp32 probability; a given probability is exact, and so is C = 1: z - m = 0, expf(0) = 1, S = 1."""
    return 0.0 if from_probs or C == 1 else SLACK * ((2 * zmax * U + F) + eps_sum(C, zmax) + 2 * U)


def nll_bound(nll64, C, zmax, from_probs=False):
    nll64 = np.abs(np.asarray(nll64, np.float64))
    if from_probs:
        return SLACK * F * nll64 + 1e-45
    return SLACK * (eps_sum(C, zmax) + F * np.log(max(C, 1)) + 2 * zmax * U + U * nll64) + 1e-45


def brier_bound(p64, labels, C, zmax, from_probs=False):
    p64 = np.asarray(p64, np.float64)
    t = np.zeros_like(p64)
    t[np.arange(p64.shape[0]), labels] = 1.0
    g = np.abs(p64 - t)
    ep = 0.0 if from_probs else eps_prob(C, zmax) / SLACK
    per_term = 2 * g * (ep * p64 + U * g) + U * g * g
    return SLACK * (per_term.sum(axis=1) + adds(C) * U * (g * g).sum(axis=1)) + 1e-45


def near_edge(p64, n_bins, rel):
    """bool [N, C]: elements whose float64 probability lies within ``rel * p`` of an inner or the upper bin edge."""
    p64 = np.asarray(p64, np.float64)
    edges = np.linspace(0, 1, n_bins + 1)[1:]
    return (np.abs(p64[..., None] - edges) <= rel * p64[..., None]).any(axis=-1)


def conf_sum_bound(p64, which, n_bins, rel):
    """int-valued bound [C, n_bins + 1] on |device conf_sum - restated conf_sum|: per element its probability error in 2^-32 units
    plus one unit for the rounding to fixed point on either side."""
    N, C = p64.shape
    out = np.zeros((C, n_bins + 1))
    np.add.at(out, (np.broadcast_to(np.arange(C), (N, C)), which), rel * p64 * metrics.CONF_FIXED_ONE + 1.0)
    return np.ceil(out)


def _wave_sum(x):
    """fp32 [C] -> the kernel's sum: lane l adds x[l], x[l + 64], ... in ascending order, then the xor butterfly."""
    C = x.shape[0]
    pad = np.zeros(-(-C // 64) * 64, np.float32)
    pad[:C] = x
    lanes = np.zeros(64, np.float32)
    for k in range(pad.shape[0] // 64):
        lanes = (lanes + pad[64 * k: 64 * k + 64]).astype(np.float32)
    off = 1
    while off < 64:
        lanes = (lanes + lanes[np.arange(64) ^ off]).astype(np.float32)
        off <<= 1
    return lanes[0]


def emulate_fp32(rows, labels, from_probs=False):
    """The kernel's rounding points in numpy float32 (numpy's expf / logf stand in for the device's): (nll fp32 [N], brier fp32 [N],
    p fp32 [N, C])."""
    z = np.asarray(rows, np.float32)
    N, C = z.shape
    nll, brier, p = np.zeros(N, np.float32), np.zeros(N, np.float32), np.zeros((N, C), np.float32)
    tiny = np.float32(np.finfo(np.float32).tiny)
    for i in range(N):
        y = int(labels[i])
        if from_probs:
            p[i] = z[i]
            nll[i] = -np.log(np.maximum(z[i, y], tiny))
        else:
            m = z[i].max()
            e = np.exp((z[i] - m).astype(np.float32)).astype(np.float32)
            S = _wave_sum(e)
            p[i] = (e * (np.float32(1.0) / S)).astype(np.float32)
            nll[i] = np.float32(np.log(S)) - np.float32(z[i, y] - m)
        t = np.zeros(C, np.float32)
        t[y] = 1.0
        g = (p[i] - t).astype(np.float32)
        brier[i] = _wave_sum((g * g).astype(np.float32))
    return nll, brier, p


def reference(rows, labels, n_bins, from_probs=False):
    """The float64 restatement on the device's own fp32 inputs: dict(nll [N], brier [N], p [N, C], which [N, C], acc int64 [3, C, n_bins + 1],
    zmax)."""
    rows = np.asarray(rows, np.float32)
    nll, brier = metrics.row_scores(rows, labels, from_probs)
    p = metrics.row_probabilities(rows, from_probs)
    bad = metrics.unscorable_rows(rows, from_probs)
    which = np.maximum(metrics.digitize_bins(p, n_bins), 0)
    which[bad] = n_bins
    finite = rows[np.isfinite(rows)]
    return {"nll": nll, "brier": brier, "p": p, "which": which, "acc": metrics.classwise_fixed_point(p, labels, n_bins, bad),
            "zmax": float(np.abs(finite).max()) if finite.size else 0.0}


def compare_case(rows, labels, n_bins, from_probs, row_out, acc):
    """Hold one device result (row_out fp32 [N, 2], acc int64 [3, C, n_bins + 1], both numpy) to the restatement; returns
    dict(nll_ratio, brier_ratio, excluded, conf_ratio) -- the worst error over its bound -- after asserting every check."""
    rows = np.asarray(rows, np.float32)
    N, C = rows.shape
    ref = reference(rows, labels, n_bins, from_probs)
    zmax = ref["zmax"]
    nb, bb = nll_bound(ref["nll"], C, zmax, from_probs), brier_bound(ref["p"], labels, C, zmax, from_probs)
    nll_ratio = float((np.abs(row_out[:, 0].astype(np.float64) - ref["nll"]) / nb).max())
    brier_ratio = float((np.abs(row_out[:, 1].astype(np.float64) - ref["brier"]) / bb).max())
    print(f"rowscores N={N} C={C} bins={n_bins} probs={int(from_probs)}: nll err/bound {nll_ratio:.3f}, brier err/bound {brier_ratio:.3f}")
    assert nll_ratio <= 1.0 and brier_ratio <= 1.0, (nll_ratio, brier_ratio)
    want = ref["acc"]
    assert acc.shape == want.shape and acc.dtype == np.int64
    assert np.array_equal(acc[0].sum(axis=1), np.full(C, N)), "every element counts once in its class"
    rel = eps_prob(C, zmax, from_probs)
    near = near_edge(ref["p"], n_bins, rel) if rel else np.zeros((N, C), bool)
    excluded = int(near.sum())
    assert excluded <= 1e-3 * N * C, f"{excluded} of {N * C} elements within fp32 rounding of a bin edge"
    conf_ratio = 0.0
    if from_probs:      # the probabilities are the inputs: every plane bit for bit
        assert np.array_equal(acc, want)
    else:
        touched = np.zeros((C, n_bins + 1), bool)      # (class, bin) cells an excluded element may have moved in or out of
        for i, c in zip(*np.nonzero(near)):
            touched[c, max(ref["which"][i, c] - 1, 0): ref["which"][i, c] + 2] = True
        assert np.array_equal(acc[0][~touched], want[0][~touched]), "counts"
        assert np.array_equal(acc[2][~touched], want[2][~touched]), "hits"
        bound = conf_sum_bound(ref["p"], ref["which"], n_bins, rel)
        diff = np.abs(acc[1] - want[1])[~touched]
        assert (diff <= bound[~touched]).all(), "conf_sum beyond the fixed-point bound"
        conf_ratio = float((diff / np.maximum(bound[~touched], 1.0)).max()) if diff.size else 0.0
    return {"nll_ratio": nll_ratio, "brier_ratio": brier_ratio, "excluded": excluded, "conf_ratio": conf_ratio}
