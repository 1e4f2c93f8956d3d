"""Reference, element-wise bounds and a CPU emulation of the two kernels every prompt fit sends each block's gradient through:
``ln_backward_kernel`` and ``quickgelu_backward_kernel`` (csrc/text_backward.hip).  It does not call the library.

Three things live here.  (1) The float64 values: the formulas of tests/coopfit_ref.py, reused.  (2) ``ln_backward_bound`` and
``quickgelu_backward_bound``: a tolerance per element, derived term by term from the kernels' arithmetic in the docstrings below and
never from what a kernel returns.  (3) ``emulate_ln_backward``: the LayerNorm kernel's fp32 arithmetic in numpy, rounding point by
rounding point, with named defects (``MUTANTS``) that tests/test_lnback_ref_cpu.py shows the bound to catch.  The case lists of the
CPU and the GPU test are at the bottom."""
import functools
import math

import numpy as np
import torch

import coopfit_ref as cref

U32, U16 = 2.0 ** -24, 2.0 ** -11          # unit roundoffs of fp32 and fp16
EPS = 1e-5
LANES, QUAD, TRIP = 64, 4, 256             # lane l owns the elements 4 l + 256 i .. + 3
ULP_RSQ = 1.0                              # v_rsq_f32 and v_exp_f32: 1 ulp each, as the CDNA instruction-set reference lists them (the
ULP_EXP = 1.0                              # project's kernel guides give no figure); rsqrtf and __expf compile to exactly these
SAFETY = 2.0                               # the project's factor for another summation order and the fast rsqrt (test_gpu_vision_train.py)


def trips(D):
    return (D + TRIP - 1) // TRIP


# ------------------------------------------------------------------------------------------------------------------ LayerNorm backward
def ln_backward(x, gamma, dy, g0=None, eps=EPS):
    """g0 + dX in float64: coopfit_ref.ln_backward on the inputs as the kernel reads them (fp32 x and gamma, fp32 or fp16 dy)."""
    dx = cref.ln_backward(x.double(), gamma.double(), dy.double(), eps)
    return dx if g0 is None else g0.double() + dx


def ln_backward_bound(x, gamma, dy, g0=None, eps=EPS, fp16_copy=False):
    """The tolerance [rows, D] of the kernel's ``g`` against ``ln_backward``; with ``fp16_copy`` that of ``g16``.

    Notation: u = 2^-24, n = ceil(D / 256) trips of a lane, mean() over the row, and the exact float64 quantities mu, xc = x - mu,
    var = mean(xc^2), r = (var + eps)^-1/2, xhat = r xc, t = dy gamma, m1 = mean(t), m2 = mean(t xhat), dX = r (t - m1 - xhat m2).
    A sum that a lane accumulates over k additions and the wave then reduces by the six-level butterfly carries at most k + 6
    roundings on every term; ``inv_d`` adds two (the rounding of 1 / D and of the product).  First order in u throughout: the second
    order is smaller by a factor of the order of rho + 75 u (step 4; D = 4096) and vanishes in the factor on top, except the one
    squared term kept below.

    1. The mean.  A trip adds (v0 + v1) + (v2 + v3) to the lane's sum: 2 + n additions at most, then 6 levels, then inv_d.
           dmu = (n + 10) u mean|x|
    2. x - mean.  c_j = fl(x_j - mean) = xc_j + (mu - mean) + u |xc_j|: the error of xhat_j is r dmu + u |xhat_j| and grows with
       r max|x|, the conditioning of the subtraction, not with max|xhat|.
    3. The variance about the mean.  sum c_j^2 by an fma chain of 4 n steps and 6 levels.  The shift (mu - mean) is the same in every
       element and sum xc_j = 0, so it enters squared only: mean(c^2) - var = dmu^2 + 2 u var + 4 u dmu mean|xc|.  That squared term
       is what a row with a large common offset costs (12 u at offset 100, spread 0.1, n = 2) and cannot be dropped.  With the chain,
       the levels and inv_d (4 n + 6 + 2 roundings on top of the 2 u above) and the rounding of the sum with eps:
           dvar = (4 n + 10) u var + 4 u dmu mean|xc| + dmu^2 + u (var + eps) + |fp32(eps) - eps|
       The kernel receives eps as fp32; the last term is what that costs against the float64 eps of the reference.
    4. rstd.  rsqrt halves a relative error of its argument and adds its own: 1 ulp = 2 u (ULP_RSQ above names the source).
           rho = dvar r^2 / 2 + 2 u ULP_RSQ
    5. t_j = fl(dy_j gamma_j): u |t_j|.  m1: a chain of 4 n additions, 6 levels, inv_d, and the rounding of t.
           dm1 = (4 n + 9) u mean|t|
    6. m2 = mean(t_j h_j), h_j = fl(c_j rstd) = xhat_j + r (mu - mean) + (rho + 2 u) |xhat_j|.  The shift and rstd's error are
       common factors, so they meet m1 and m2 themselves and not the means of magnitudes; the per-element roundings (c_j, h_j, t_j),
       the fma chain, the levels and inv_d meet mean|t xhat|:
           dm2 = r dmu |m1| + rho |m2| + (4 n + 11) u mean|t xhat|
    7. The result rstd ((t_j - m1) - h_j m2), every operation rounded (a contraction into fma has fewer roundings, not more):
           a_j = fl(t_j - m1)     : u |t_j| + dm1 + u |t_j - m1|
           b_j = fl(h_j m2)       : (r dmu + (rho + 2 u) |xhat_j|) |m2| + |xhat_j| dm2 + u |xhat_j m2|
           a_j - b_j, times rstd  : u |t_j - m1 - xhat_j m2|, then (rho + u) |dX_j|
           d(dX_j) = r (a_j's + b_j's + u |t_j - m1 - xhat_j m2|) + (rho + u) |dX_j|
    8. The rounding into g: u |g0_j + dX_j|; absent when g0 is None (a zero stream: fl(0 + v) = v).
    9. g16 is the fp16 rounding of g, which the tests hold bit for bit against the returned g; against float64 it adds u16 |g_j|,
       or half a subnormal step 2^-25 (``fp16_copy``).
    SAFETY = 2 goes on top of 1..8."""
    x, gamma, dy = x.double(), gamma.double(), dy.double()
    D = x.shape[-1]
    n, u = trips(D), U32
    mean = lambda v: v.mean(-1, keepdim=True)
    mu = mean(x)
    xc = x - mu
    var = mean(xc * xc)
    r = torch.rsqrt(var + eps)
    xhat = xc * r
    t = dy * gamma
    m1, m2 = mean(t), mean(t * xhat)
    inner = t - m1 - xhat * m2
    dx = r * inner
    dmu = (n + 10) * u * mean(x.abs())
    dvar = (4 * n + 10) * u * var + 4 * u * dmu * mean(xc.abs()) + dmu * dmu + u * (var + eps) + abs(float(np.float32(eps)) - eps)
    rho = dvar * r * r / 2 + 2 * u * ULP_RSQ
    dm1 = (4 * n + 9) * u * mean(t.abs())
    dm2 = r * dmu * m1.abs() + rho * m2.abs() + (4 * n + 11) * u * mean((t * xhat).abs())
    da = u * t.abs() + dm1 + u * (t - m1).abs()
    db = (r * dmu + (rho + 2 * u) * xhat.abs()) * m2.abs() + xhat.abs() * dm2 + u * (xhat * m2).abs()
    tol = r * (da + db + u * inner.abs()) + (rho + u) * dx.abs()
    want = dx
    if g0 is not None:
        want = g0.double() + dx
        tol = tol + u * want.abs()
    tol = SAFETY * tol
    if fp16_copy:
        tol = tol + torch.clamp(U16 * want.abs(), min=2.0 ** -25) + U16 * tol
    return tol


# the six levels of wave_sum (csrc/common.h) as lane permutations: quad_perm xor 1, xor 2, row_half_mirror, row_mirror, the swaps of
# the 16-lane rows and of the halves
_L = np.arange(LANES)
BUTTERFLY = (_L ^ 1, _L ^ 2, (_L & ~7) | (7 - (_L & 7)), (_L & ~15) | (15 - (_L & 15)), _L ^ 16, _L ^ 32)

MUTANTS = ("drop_second_trip", "one_pass_variance", "no_eps", "m1_zero", "m2_uncentred", "inv_d_off_by_one", "g16_from_dx",
           "dy_by_target_row")

f32 = np.float32


def _fma(a, b, c):
    """fmaf on fp32 arrays: the product is exact in float64; the sum is rounded to 53 bits and then to 24 (a double rounding that
    differs from the fused one only on ties of the 53-bit value, about one case in 2^29)."""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(f32)


def _wave_sum(s):
    for perm in BUTTERFLY:
        s = s + s[:, perm]
    return s[:, :1]                                    # every lane holds the same bits: fp32 addition commutes


def _lanes(a, D, n):
    """[R, D] -> [R, n, 64, 4]: trip i, lane l, element j is column 256 i + 4 l + j (zeros behind D)."""
    out = np.zeros((a.shape[0], n * TRIP), dtype=f32)
    out[:, :D] = a
    return out.reshape(a.shape[0], n, LANES, QUAD)


def emulate_ln_backward(x, gamma, dy, g0, eps=EPS, row_idx=None, mutant=None):
    """The kernel's fp32 arithmetic in numpy: (g, g16) as torch tensors, g of g0's shape.  ``x`` and ``g0`` are [R, D], ``dy`` [rows, D]
    in call order, row r of the call reads x[row(r)] and updates g[row(r)], row(r) = row_idx[r] or r.  ``mutant`` turns on one defect
    of MUTANTS."""
    assert mutant is None or mutant in MUTANTS, mutant
    xs = x.numpy().astype(f32)
    gam = gamma.numpy().astype(f32)
    d_all = dy.float().numpy()                         # an fp16 dy converts exactly
    g = g0.numpy().astype(f32).copy()
    rows, D = d_all.shape
    src = np.arange(rows) if row_idx is None else row_idx.numpy().astype(np.int64)
    n = trips(D)
    xr = _lanes(xs[src], D, n)
    dyr = _lanes(d_all[src % rows] if mutant == "dy_by_target_row" else d_all, D, n)      # the defect reads behind dy: wrapped here
    gm = _lanes(np.broadcast_to(gam, (rows, D)), D, n)
    live = (TRIP * np.arange(n)[:, None] + QUAD * np.arange(LANES)[None, :]) < D          # [n, 64]: whole quads, D % 4 == 0
    if mutant == "drop_second_trip":
        live = live & (np.arange(n)[:, None] == 0)
    live = live[None]
    inv_d = f32(1.0) / f32(D - 1 if mutant == "inv_d_off_by_one" else D)
    zero = np.zeros((rows, LANES), dtype=f32)

    s = zero.copy()
    for i in range(n):
        v = xr[:, i]
        s = np.where(live[:, i], s + ((v[..., 0] + v[..., 1]) + (v[..., 2] + v[..., 3])), s)
    mean = _wave_sum(s) * inv_d                        # [rows, 1]
    s = zero.copy()
    for i in range(n):
        for j in range(QUAD):
            v = xr[:, i, :, j]
            c = v if mutant == "one_pass_variance" else v - mean
            s = np.where(live[:, i], _fma(c, c, s), s)
    var = _wave_sum(s) * inv_d
    if mutant == "one_pass_variance":
        var = var - mean * mean
    if mutant != "no_eps":
        var = var + f32(eps)
    with np.errstate(divide="ignore", invalid="ignore"):
        rstd = (1.0 / np.sqrt(var.astype(np.float64))).astype(f32)
    centre = f32(0.0) if mutant == "m2_uncentred" else mean
    s1, s2 = zero.copy(), zero.copy()
    with np.errstate(over="ignore", invalid="ignore"):
        for i in range(n):
            for j in range(QUAD):
                t = dyr[:, i, :, j] * gm[:, i, :, j]
                s1 = np.where(live[:, i], s1 + t, s1)
                s2 = np.where(live[:, i], _fma(t, (xr[:, i, :, j] - centre) * rstd, s2), s2)
        m1, m2 = _wave_sum(s1) * inv_d, _wave_sum(s2) * inv_d
        if mutant == "m1_zero":
            m1 = np.zeros_like(m1)
        m1, m2, mean4, rstd4 = (a[:, None, :, None] for a in (m1, m2, mean, rstd))
        dx = rstd4 * ((dyr * gm - m1) - (xr - mean4) * rstd4 * m2)            # [rows, n, 64, 4]
        dx = dx.reshape(rows, n * TRIP)[:, :D]
        g[src] = g[src] + dx                           # the rows of one call are distinct
        g = torch.from_numpy(g)
        g16 = g.half()
        if mutant == "g16_from_dx":
            g16[torch.from_numpy(src)] = torch.from_numpy(dx).half()
    return g, g16


# ------------------------------------------------------------------------------------------------------------------ the LayerNorm cases
LN_WIDTHS = (4, 8, 252, 256, 260, 320, 768, 1024, 1280, 4096)
DY_DTYPES = (torch.float32, torch.float16)
KINDS = ("random", "bigmean", "outlier", "below_eps", "constant", "dy_is_xhat", "t_constant", "basis")


class Group:
    """Rows that share one gamma, hence one launch: x, dy [rows, D], and the kind of every row."""

    def __init__(self, name, gamma, rows):
        self.name, self.gamma = name, gamma
        self.kinds = [k for k, _, _ in rows]
        self.x = torch.stack([x for _, x, _ in rows])
        self.dy = torch.stack([d for _, _, d in rows])

    def rows_of(self, kind):
        return [i for i, k in enumerate(self.kinds) if k == kind]


def row_kinds(D, seed=0):
    """Two groups that together hold every kind of KINDS at least twice; neither row count is a multiple of 4 (four rows share a
    workgroup and the last one must be partial).  dy is fp32 here; the fp16 cases round it."""
    g = torch.Generator().manual_seed(1000 * D + seed)
    rand = lambda: torch.randn(D, generator=g) * 1.5 + 0.3                     # the distribution of test_gpu_text_backward.py
    dyr = lambda: torch.randn(D, generator=g)
    gamma = 1.0 + 0.2 * torch.randn(D, generator=g)
    gamma[1 % D], gamma[D - 2] = 0.0, -0.7                                     # a dead channel and a negative one
    a = [("random", rand(), dyr()), ("random", rand(), dyr())]
    a += [("bigmean", 100.0 + 0.1 * torch.randn(D, generator=g), dyr()) for _ in range(2)]
    for at in (2, D - 3 if D > TRIP else D - 1):                               # in the first quad; in a later trip where D has one
        x = rand()
        x[at] = 300.0
        a.append(("outlier", x, dyr()))
    for at in (0, D - 1):
        x = torch.full((D,), 3.0)
        x[at] += 2.0 ** -20
        a.append(("below_eps", x, dyr()))
    a += [("constant", torch.full((D,), c), dyr()) for c in (0.3, -7.0)]
    for e0 in sorted({min(e, D - 1) for e in (0, 3, 4, 255, 256, D - 1)}):
        d = torch.zeros(D)
        d[e0] = 1.0
        a.append(("basis", rand(), d))
    b = []
    for x in (rand(), 100.0 + 0.1 * torch.randn(D, generator=g)):
        xd = x.double()
        xc = xd - xd.mean()
        b.append(("dy_is_xhat", x, (xc * torch.rsqrt((xc * xc).mean() + EPS)).float()))
    b += [("t_constant", rand(), torch.full((D,), c)) for c in (1.0, -0.375)]
    b.append(("random", rand(), dyr()))
    for rows in (a, b):
        if len(rows) % 4 == 0:
            rows.append(("random", rand(), dyr()))
    return [Group("gamma_random", gamma, a), Group("gamma_one", torch.ones(D), b)]


def scatter_case(D, seed=0):
    """The EOT scatter of the tail with strided rows: x is a column slice of ``wide`` [R, D + 8], row_idx a non-monotone subset of
    g's R rows with row 0 and the last one, dy dense in call order."""
    g = torch.Generator().manual_seed(77 * D + seed)
    R = 11
    wide = torch.randn(R, D + 8, generator=g) * 1.5 + 0.3
    idx = torch.tensor([4, 0, R - 1, 7, 2], dtype=torch.int32)
    gamma = 1.0 + 0.2 * torch.randn(D, generator=g)
    dy = torch.randn(idx.numel(), D, generator=g)
    g0 = torch.randn(R, D, generator=g)
    return wide, idx, gamma, dy, g0


SCATTER_WIDTHS = (768, 260)


@functools.lru_cache(maxsize=None)
def ln_groups(D):
    return row_kinds(D)


@functools.lru_cache(maxsize=None)
def ln_case(D, dt, gi):
    """Launch ``gi`` of width D with dy of dtype ``dt``: the inputs, a random g0, the float64 value and the tolerances of g and of
    its fp16 copy -- computed once and shared by the tests, which leave them unchanged."""
    grp = ln_groups(D)[gi]
    dy = grp.dy.to(dt)
    g0 = torch.randn(grp.x.shape, generator=torch.Generator().manual_seed(D + gi))
    return dict(kinds=grp.kinds, x=grp.x, gamma=grp.gamma, dy=dy, g0=g0, idx=None, want=ln_backward(grp.x, grp.gamma, dy, g0),
                tol=ln_backward_bound(grp.x, grp.gamma, dy, g0), tol16=ln_backward_bound(grp.x, grp.gamma, dy, g0, fp16_copy=True))


@functools.lru_cache(maxsize=None)
def ln_scatter(D):
    """``scatter_case`` with its expectation over all R rows of g; the bound of an indexed row comes from x[row_idx[r]] and dy[r]."""
    wide, idx, gamma, dy, g0 = scatter_case(D)
    x, rows = wide[:, :D], idx.long()
    want, tol = g0.double().clone(), torch.full(g0.shape, 1e-300, dtype=torch.float64)          # rows not indexed keep their bits
    tol16 = torch.clamp(U16 * want.abs(), min=2.0 ** -25)                                         # and their copy is their rounding
    want[rows] = ln_backward(x[rows], gamma, dy, g0[rows])
    tol[rows] = ln_backward_bound(x[rows], gamma, dy, g0[rows])
    tol16[rows] = ln_backward_bound(x[rows], gamma, dy, g0[rows], fp16_copy=True)
    return dict(kinds=["scatter"] * g0.shape[0], wide=wide, x=x, gamma=gamma, dy=dy, g0=g0, idx=idx, want=want, tol=tol, tol16=tol16)


def ratio(got, want, tol):
    """The worst error / tolerance; infinite where the result is not finite."""
    got = got.double()
    if not torch.isfinite(got).all():
        return math.inf
    return float(((got - want).abs() / tol).max())


# ------------------------------------------------------------------------------------------------------------------ QuickGELU backward
C1702 = 1.702
D_C = abs(float(np.float32(C1702)) - C1702) / C1702                               # the kernel's constants are fp32
D_LOG2E = abs(float(np.float32(math.log2(math.e))) - math.log2(math.e)) / math.log2(math.e)


def quickgelu_backward(h, d_a):
    return cref.quickgelu_backward(h.double(), d_a.double())


def quickgelu_backward_bound(h, d_a, want):
    """The tolerance of ``fp16(d_a (s + z s (1 - s)))``, z = 1.702 h, s = 1 / (1 + exp(-z)), evaluated in fp32 from fp16 inputs.

    The last step is one rounding to fp16: u16 |want|, or half a subnormal step 2^-25 below the normal range.  On top, the fp32
    evaluation, first order in u = 2^-24 (the second order is below 2^-10 of it at the largest |z| that matters and is covered by the
    factor (1 + 2^-10) at the end):

    * __expf(a) is exp2 of the ROUNDED product a log2(e) (one v_exp_f32 behind one multiplication: its definition in the HIP headers,
      which is also what the compiler emits; the project's kernel guides give no error figure, the CDNA instruction-set reference
      gives v_exp_f32 1 ulp = 2 u).  a = fl(-1.702f h) carries u and the constant's D_C; the product adds u and D_LOG2E.  An error
      of the exponent is a relative error of the value times |z|:
          rho_e = |z| (2 u + D_C + D_LOG2E) + 2 u ULP_EXP
    * s = fl(1 / fl(1 + e)), ds / s = -(1 - s) de / e.  Both roundings are to nearest and 1 is a float, so neither moves its
      result further than 1 lies: fl(1 + e) errs by min(u, e / (1 + e)) = min(u, 1 - s) relatively, the quotient by min(u, 2 (1 - s)).
      Without the second arm the tolerance would grow like |z| u where s is exactly 1:
          rho_s = (1 - s) rho_e + min(2 u, 3 (1 - s))
    * q = fl(1 - s): the subtraction is exact up to u, but s's error enters absolutely, which is why a relative bound on the
      derivative cannot hold:                                                          dq = s rho_s + u (1 - s)
    * p = fl(fl(fl(1.702f h) s) q): three roundings and D_C:                           dp = |z| (s (1 - s) (3 u + D_C + rho_s) + s dq)
    * f = fl(s + p) and the product with d_a: u |f| each.                              df = s rho_s + dp + 2 u |f|
    Near the derivative's zero (z = -1.278, h = -0.751) s and p cancel and |f| is small, but df is not: it stays a multiple of u
    there (3.9 u; it peaks at 38 u near z = 17, where 1 - s is a few u), so the tolerance is absolute in |d_a|, E = |d_a| df.  The
    fp16 rounding of the perturbed value adds u16 E."""
    h, d_a, want = h.double(), d_a.double(), want.double()
    u = U32
    z = C1702 * h
    s = torch.sigmoid(z)
    q = torch.sigmoid(-z)                                                      # 1 - s without the cancellation
    rho_e = z.abs() * (2 * u + D_C + D_LOG2E) + 2 * u * ULP_EXP
    rho_s = q * rho_e + torch.clamp(3 * q, max=2 * u)
    dq = s * rho_s + u * q
    dp = z.abs() * (s * q * (3 * u + D_C + rho_s) + s * dq)
    f = s + z * s * q
    df = s * rho_s + dp + 2 * u * f.abs()
    e32 = d_a.abs() * df * (1 + 2.0 ** -10)
    return torch.clamp(U16 * want.abs(), min=2.0 ** -25) + (1 + U16) * e32


def emulate_quickgelu_backward(h, d_a):
    """The kernel's expression in numpy fp32, np.exp standing in for the fast exponential; the fp16 result as a torch tensor."""
    hf, df = h.float().numpy(), d_a.float().numpy()
    with np.errstate(over="ignore"):
        s = f32(1.0) / (f32(1.0) + np.exp(f32(-1.702) * hf))
        out = df * (s + f32(1.702) * hf * s * (f32(1.0) - s))
    return torch.from_numpy(out).half()


GELU_D_A = (1.0, -1.0, 2.0 ** -14, 2.0 ** -24, 1.0 / 3.0, 32768.0, -32768.0)     # 1 / 3 is rounded to fp16 by the sweep
GELU_LENGTHS = (1, 7, 8, 9, 2047, 2048, 2049)                                   # one workgroup covers 2048 elements, eight per thread
GELU_FILLER = 3


def every_fp16():
    """All 63 488 finite fp16 values, both zeros and the subnormals included, in bit-pattern order."""
    bits = torch.arange(0, 1 << 16, dtype=torch.int32)
    bits = bits[(bits & 0x7C00) != 0x7C00]
    return bits.to(torch.int16).view(torch.float16)


def gelu_sweep():
    """(h, d_a): every finite h paired with every GELU_D_A, behind GELU_FILLER elements; the length is 3 mod 8, so the last three
    elements take the kernel's scalar tail."""
    hs = every_fp16()
    fill_h, fill_d = torch.tensor([0.5, -0.75, 2.0]).half(), torch.tensor([1.0, 1.0, -1.0]).half()
    h = torch.cat([fill_h] + [hs] * len(GELU_D_A))
    d = torch.cat([fill_d] + [torch.full((hs.numel(),), v).half() for v in GELU_D_A])
    assert h.numel() % 8 == 3 and hs.numel() == 63488
    return h, d
