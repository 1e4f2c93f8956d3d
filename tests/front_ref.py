"""Plain references of LayerNorm (csrc/layernorm.hip) and of the image tower's front end (csrc/patch_embed.hip: the fp32 -> fp16 pixel cast,
the im2col patch GEMM with the positional epilogue, ln_pre over the class / patch / prompt rows; csrc/elementwise.hip: patchify) -- the oracle
of tests/test_front_ref_cpu.py and tests/test_gpu_front_ops.py.  numpy / torch-CPU, float64 wherever there is arithmetic, written from the
formulas of the kernel headers and the reference lines they cite:

* clip/model.py:153-159 (LayerNorm with fp32 statistics, eps inside the square root);
* clip/model.py:394-402 (conv1 with stride = kernel = P, reshape, permute, class embedding, positional embedding) and :413 (ln_pre);
* clip/model.py:459-460 (the shallow prompt rows, appended after the positional embedding is added);
* clip/model.py:597-598 (image.type(dtype): one round-to-nearest-even fp32 -> fp16 cast of the pixels).

Data movers return the exact fp16 / fp32 result (a copy, one IEEE round-to-nearest-even rounding -- which torch's .half() is -- or one IEEE
fp32 addition, which has one answer everywhere).  Arithmetic ones return ``(value, bound)``, both float64: ``bound`` is the data-dependent
forward error bound of the kernel's fp32 arithmetic BEFORE its output rounding; the ``tol_*`` functions add that rounding.  The case tables and
seeded input generators at the end are shared by the CPU test (which holds an fp32 emulation of each kernel's order of operations to the same
tolerances, and shows that plausible wrong kernels break them) and the GPU test: same seeds, same tensors.

Notation: U32 = 2^-24, U16 = 2^-11 (unit roundoffs), gamma(n) = n U32 / (1 - n U32) (n fp32 roundings compounded).

LayerNorm rows (layernorm_kernel, embed_ln_kernel: one wave per row, lane ``l`` holds float4 groups c = l + 64 i, i < NV; NV = 4 for
D <= 1024, else 16; a row of width D fills groups(D) = ceil(D / 256) <= NV of them)
-----------------------------------------------------------------------------------------------------------------------------------------
mean.  Each lane adds its groups as s += (v0 + v1) + (v2 + v3): two tree levels and one serial addition per group; the xor butterfly adds six
levels; the division by D rounds once.  The longest chain behind the mean is SUM_DEPTH(D) = groups(D) + 8 additions, so
    |mean^ - mean| <= gamma(C_MEAN) mean|x|,      C_MEAN(D) = groups(D) + 9.
Every output moves by that error times rstd |gamma_i|: the first term of the bound.  Its size relative to the row's spread,
    E = gamma(C_MEAN) mean|x| rstd,
is the row's conditioning: it is what a large common offset makes large.

variance.  d_i = fl(x_i - mean^) carries one rounding, d_i^2 three (twice d_i's and the product's); each lane adds up to 4 groups(D) squares
serially, the butterfly adds six levels, the division by D and the addition of eps round once each:
    C_VAR(D) = 4 groups(D) + 11   relative roundings on var + eps   (all terms are non-negative, so relative errors do not amplify).
Because the second pass is taken around mean^ and not around the mean, the sum of squares is that of the exact deviations plus D (mean^ - mean)^2
(the cross term vanishes): var + eps grows by the factor 1 + E^2 at most, and rstd shrinks by 1 - (1 + E^2)^(-1/2) <= E^2 / 2.  The term is kept
although it is of second order in U32, because E is not small for an offset row.

rstd.  rsqrtf is an approximate device instruction.  HIP's math API reference lists rsqrtf with a maximum error of 1 ulp, and the CDNA
instruction set guide gives V_RSQ_F32 1 ulp of accuracy: RSQRT_ULPS = 1, and one ulp is at most 2 U32 relative.  With the square root halving
the relative error of its argument:  |rstd^ - rstd| / rstd <= C_VAR / 2 U32 + 2 RSQRT_ULPS U32 + E^2 / 2.

output.  o_i = fl(fl(fl(d_i rstd^) gamma_i) + beta_i): the subtraction's rounding, rstd's error, two multiplications, and the final
addition, whose rounding is relative to |t + beta_i| <= |t| + |beta_i|:
    C_DEV(D) = 1 + C_VAR / 2 + 2 RSQRT_ULPS + 2 + 1 = 2 groups(D) + 11.5
    bound_i = gamma(C_MEAN) mean|x| rstd |gamma_i|  +  (gamma(C_DEV) + E^2 / 2) |x_i - mean| rstd |gamma_i|  +  U32 |beta_i|
(a fused multiply-add in place of a multiplication and an addition only removes a rounding).  groups = 1: C_MEAN 10, C_DEV 13.5; groups = 4
(D = 1024): 13 and 19.5; groups = 16 (D = 4096): 25 and 43.5.

Fold row sums (the (sum, sum of squares) of the fp32 OUTPUT row that the LayerNorm-folded in-projection consumes)
-----------------------------------------------------------------------------------------------------------------------------------------
os += (o0 + o1) + (o2 + o3), oq += (o0 o0 + o1 o1) + (o2 o2 + o3 o3), then the same butterfly: SUM_DEPTH(D) additions behind either sum and
one more rounding, the product's, behind the squares.  One depth serves both: FOLD_DEPTH(D) = groups(D) + 9, with
    |os^ - sum o| <= gamma(FOLD_DEPTH) sum |o|,      |oq^ - sum o^2| <= gamma(FOLD_DEPTH) sum o^2.
At D = 4096 that is 25 U32 = 1.5e-6 relative to sum |o|.  The sums of the fp16 ROUNDINGS of o differ from these by up to U16 sum |o| (3e-4 relative
when the roundings share a sign, about U16 / sqrt(3 D) relative when they do not): the bound tells the two apart.

Patch GEMM (gemm_pp_kernel<..., IM2COL>, EPI_PATCH_POS)
-----------------------------------------------------------------------------------------------------------------------------------------
The product of two fp16 numbers has 22 significant bits and is exact in fp32.  The K products of an output are added to its fp32 accumulator 32
at a time (v_mfma_f32_16x16x32_f16, K / 32 dependent instructions).  The order of the additions inside one instruction is not documented, so the
model is the order-free one -- any summation of K terms makes K - 1 additions, and an error of at most gamma(K - 1) sum |t| when each rounds
to nearest -- and the instruction set guide does not promise round-to-nearest for the partial sums inside the instruction, so every addition is
allowed one whole ulp (2 U32) instead of half:
    GAMMA_K(K) = 2 K U32 / (1 - 2 K U32):     K = 192: 2.3e-5,  K = 768: 9.2e-5,  K = 3072: 3.7e-4   (times sum_k |a_k| |w_k|)
The epilogue adds pos in fp32, one rounding relative to |acc + pos| <= sum |a| |w| + |pos|, whose first part GAMMA_K's spare addition pays for:
    tol = GAMMA_K sum |a| |w| + U32 |pos| + one output rounding.
"""
from __future__ import annotations

import collections
import itertools

import torch

U16 = 2.0 ** -11      # unit roundoff of fp16
U32 = 2.0 ** -24      # unit roundoff of fp32; also the smallest fp16 subnormal
RSQRT_ULPS = 1        # documented accuracy of rsqrtf / V_RSQ_F32 (module docstring)

MAX_D = 4096          # row width limit of layernorm_kernel / embed_ln_kernel
ROWS_PER_BLOCK = 4    # one wave per row, four waves per workgroup


def _f64(t):
    return t.detach().cpu().to(torch.float64)


def gamma_n(n):
    """n fp32 roundings compounded."""
    return n * U32 / (1.0 - n * U32)


# ------------------------------------------------------------------------------------------------------------------- csrc/layernorm.hip
def ln_nv(D):
    """float4 groups per lane the dispatch instantiates (NV): 4 while D / 4 <= 256, else 16."""
    return 4 if D // 4 <= 64 * 4 else 16


def ln_groups(D):
    """float4 groups per lane a row of width D fills (<= NV)."""
    return -(-D // 256)


def sum_depth(D):
    return ln_groups(D) + 8


def c_mean(D):
    return sum_depth(D) + 1


def c_var(D):
    return 4 * ln_groups(D) + 11


def c_dev(D):
    return 1 + 0.5 * c_var(D) + 2 * RSQRT_ULPS + 2 + 1


def fold_depth(D):
    return sum_depth(D) + 1


def ln_source_rows(x, D, rows=None, in_stride=None):
    """The rows LayerNorm reads: row r starts at element (rows[r] if rows is given else r) * in_stride of the flat buffer x (in_stride None:
    x is [n, D] and in_stride = D).  Returns them in x's dtype, [n, D]."""
    flat = x.detach().cpu().reshape(-1)
    stride = D if in_stride is None else int(in_stride)
    idx = torch.arange(flat.numel() // stride) if rows is None else torch.as_tensor(rows).long()
    return torch.stack([flat[int(i) * stride:int(i) * stride + D] for i in idx])


def layer_norm_rows(x, gamma, beta, eps, rows=None, in_stride=None):
    """clip/model.py:153-159 -> (value, bound), float64 [n, D]; addressing as ln_source_rows, bound as derived in the module docstring."""
    D = gamma.numel()
    v = _f64(ln_source_rows(x, D, rows, in_stride))
    g, b = _f64(gamma), _f64(beta)
    mean = v.mean(dim=1, keepdim=True)
    dev = v - mean
    rstd = 1.0 / torch.sqrt((dev * dev).mean(dim=1, keepdim=True) + float(eps))
    val = dev * rstd * g + b
    mean_term = gamma_n(c_mean(D)) * v.abs().mean(dim=1, keepdim=True) * rstd          # E of the docstring, per row
    bound = mean_term * g.abs() + (gamma_n(c_dev(D)) + 0.5 * mean_term ** 2) * dev.abs() * rstd * g.abs() + U32 * b.abs()
    return val, bound


def _out_rounding(val, bound, dtype):
    """One round-to-nearest-even rounding of the computed value (within ``bound`` of ``val``); an fp16 subnormal is 2^-24 apart from the next."""
    if dtype == torch.float16:
        return U16 * (val.abs() + bound) + 0.5 * U32
    return U32 * (val.abs() + bound)


def tol_ln(val, bound, out_dtype):
    return bound + _out_rounding(val, bound, out_dtype)


def embed_rows(x0, cls, pos, shallow, L, tokens0, add_pos):
    """The rows ln_pre sees (clip/model.py:398-402, 459-460), exactly: fp32 [B * L, D].  Row l == 0 is cls + pos[0] and rows l >= tokens0 are
    shallow[l - tokens0]: neither reads x0.  Patch rows are x0 as the GEMM left it (fp16 or fp32), + pos[l] when add_pos; each sum is one
    IEEE fp32 addition."""
    D = cls.numel()
    rows = x0.detach().cpu().float().reshape(-1, L, D).clone()
    if add_pos:
        rows[:, 1:tokens0] += pos.detach().cpu().float()[1:tokens0]
    rows[:, 0] = cls.detach().cpu().float() + pos.detach().cpu().float()[0]
    if L > tokens0:
        rows[:, tokens0:] = shallow.detach().cpu().float()[:L - tokens0]
    return rows.reshape(-1, D)


def fold_row_sums(o):
    """o [n, D] -> (sum, sum of squares, bound of the sum, bound of the squares), float64 [n]: FOLD_DEPTH of the module docstring."""
    v = _f64(o)
    g = gamma_n(fold_depth(v.shape[1]))
    q = (v * v).sum(dim=1)
    return v.sum(dim=1), q, g * v.abs().sum(dim=1), g * q


def tol_fold_of_reference(val, bound):
    """The fold sums of a computed row that lies within ``bound`` of ``val``, against the sums of ``val``: (tol of the sum, tol of the squares)."""
    hi = val.abs() + bound
    _, _, bs, bq = fold_row_sums(hi)
    return bs + bound.sum(dim=1), bq + (2.0 * val.abs() * bound + bound * bound).sum(dim=1)


# ------------------------------------------------------------------------------------- csrc/patch_embed.hip, csrc/elementwise.hip (patchify)
def patchify(image, P, kpad):
    """image [B,3,R,R] fp32|fp16 -> fp16 [B*G*G, kpad]: column c P^2 + ky P + kx of row (b, py, px) = fp16(image[b, c, py P + ky, px P + kx])
    (clip/model.py:598, 395-397), zero in the padding columns.  An explicit gather, one coordinate at a time."""
    B, C, R, _ = image.shape
    G = R // P
    src = image.detach().cpu().half()
    col = torch.zeros(B, G, G, kpad, dtype=torch.float16)
    for c in range(C):
        for ky in range(P):
            for kx in range(P):
                col[:, :, :, c * P * P + ky * P + kx] = src[:, c, ky::P, kx::P]
    return col.reshape(B * G * G, kpad)


def gamma_k(K):
    return 2.0 * K * U32 / (1.0 - 2.0 * K * U32)


def patch_x0_rows(B, G, tokens):
    """Row of x0 [B * tokens, D] that patch p of image b lands in: b * tokens + 1 + p."""
    return (torch.arange(B)[:, None] * tokens + 1 + torch.arange(G * G)[None, :]).reshape(-1)


def patch_rows(image, w, pos, P, tokens):
    """conv1 + reshape / permute + pos (clip/model.py:395-401) from the fp16-rounded pixels and weights -> (value, sum_k |a| |w|, x0 rows):
    float64 [B*G*G, D] twice and the index of each row in x0 [B * tokens, D].  w fp16 [D, 3 P^2]; pos fp32 [1 + G*G, D] or None."""
    B, _, R, _ = image.shape
    G = R // P
    a = _f64(patchify(image, P, 3 * P * P))
    W = _f64(w.detach().cpu().half())
    val = a @ W.t()
    S = a.abs() @ W.abs().t()
    if pos is not None:
        val = val + _f64(pos)[1:1 + G * G].repeat(B, 1)
    return val, S, patch_x0_rows(B, G, tokens)


def tol_patch(val, S, pos, B, K, out_dtype):
    bound = gamma_k(K) * S
    if pos is not None:
        bound = bound + U32 * _f64(pos)[1:].abs().repeat(B, 1)
    return bound + _out_rounding(val, bound, out_dtype)


# ------------------------------------------------------------------------------------------------ pixel coding of the address-map test
CODE_PRIME = 2039                                   # the largest prime below 2048: every code is an integer fp16 holds exactly
CODE_WEIGHTS = (1, 37, 211, 401, 809, 1201)         # of (kx, ky, px, py, c, b): distinct residues


def code_value(b, c, py, px, ky, kx):
    """Exchanging the values of any two coordinates i, j changes the code by (w_i - w_j) (v_i - v_j) mod p, which is non-zero for distinct
    weights and distinct values below the prime p (tests/test_front_ref_cpu.py checks it by enumeration)."""
    w = CODE_WEIGHTS
    return (w[0] * kx + w[1] * ky + w[2] * px + w[3] * py + w[4] * c + w[5] * b) % CODE_PRIME


def coded_image(B, R, P, dtype):
    """[B,3,R,R] with pixel (b, c, y, x) = code_value(b, c, y // P, x // P, y % P, x % P)."""
    b, c, y, x = torch.meshgrid(torch.arange(B), torch.arange(3), torch.arange(R), torch.arange(R), indexing="ij")
    return code_value(b, c, y // P, x // P, y % P, x % P).to(dtype)


# (B, R, P): D = K = 3 P^2, one-hot weights; G = 2 and two images, so that every coordinate takes two values at least
ADDRESS_CASES = [(2, 16, 8), (2, 32, 16), (2, 64, 32)]


def tie_image(B, R):
    """fp32 pixels that sit on fp16 rounding ties, 1 + (2 j + 1) 2^-11 (round-to-nearest-even goes down for even j, up for odd j; truncation
    always down), their negatives, and pixels beyond the largest fp16 number that still round to it, 65504 < |x| < 65520 (from 65520 on the
    cast gives infinity, and 0 * inf = NaN in every output of the row: no exact test can hold those)."""
    n = B * 3 * R * R
    j = torch.arange(n, dtype=torch.float64) % 1024
    v = 1.0 + (2.0 * j + 1.0) * 2.0 ** -11
    v[1::7] *= -1.0
    big = 65504.0 + 1.0 + (torch.arange(n, dtype=torch.float64) % 14)
    v[3::5] = big[3::5]
    v[4::10] = -big[4::10]
    return v.to(torch.float32).reshape(B, 3, R, R)


# ----------------------------------------------------------------------------------------- cases and inputs (CPU and GPU tests share them)
def _gen(*key):
    return torch.Generator().manual_seed(sum((i + 1) * 1000003 * int(k) for i, k in enumerate(key)) % (2 ** 31))


DTYPES = (torch.float16, torch.float32)
IN_SENTINEL = {torch.float16: 65504.0, torch.float32: 3.0e38}      # what a kernel must not read: huge and finite, it would wreck the row

LN_D = [4, 8, 252, 256, 260, 1020, 1024, 1028, 2052, 4092, 4096]   # D = 4; a partly filled 64-lane group (252, 260, ...); NV 4 -> 16 behind 1024; the limit
LN_ROWS = [1, 3, 4, 5, 9]                                           # four rows per workgroup
# contiguous; in_stride = L D (ln_post: one class row per sequence); padded output rows; int32 gather (ln_final); gather and in_stride
LN_FORMS = ["contig", "in2", "in7", "out4", "out64", "gather", "gather_in2", "gather_in7"]
LN_EPS = [1e-5, 1e-12, 1e-3]
# adversarial rows; the offset rows exist per input dtype (fp32: mean 1e3, spread 1e-2; fp16: the largest offset with a non-zero spread)
LN_KINDS = ["constant", "offset", "spike", "alternating", "tiny_var", "zero", "random"]

LnCase = collections.namedtuple("LnCase", "D rows dt_in dt_out form eps kind")


def _ln_cases():
    cases, n = [], 0
    combos = list(itertools.product(DTYPES, DTYPES))
    for iD, D in enumerate(LN_D):                                   # every width in every dtype combination, contiguous, rows cycling
        for idt, (di, do) in enumerate(combos):
            cases.append(LnCase(D, LN_ROWS[(iD + idt) % len(LN_ROWS)], di, do, "contig", 1e-5, "random"))
    for form in LN_FORMS[1:]:                                       # every other form in every dtype combination on either side of the NV switch
        for di, do in combos:
            for D in (260, 1028):
                cases.append(LnCase(D, LN_ROWS[n % len(LN_ROWS)], di, do, form, LN_EPS[n % len(LN_EPS)], "random"))
                n += 1
    for D in (252, 1028, 4096):                                     # the adversarial rows, one row per kind
        for di, do in combos:
            cases.append(LnCase(D, len(LN_KINDS), di, do, "contig", 1e-5, "adversarial"))
    for D in (260, 4096):                                           # ... as ln_final and ln_post read them
        cases.append(LnCase(D, len(LN_KINDS), torch.float16, torch.float32, "gather_in2", 1e-5, "adversarial"))
        cases.append(LnCase(D, len(LN_KINDS), torch.float32, torch.float16, "in7", 1e-3, "adversarial"))
    return cases


LN_CASES = _ln_cases()


def ln_case_id(c):
    return f"D{c.D}-r{c.rows}-{'h' if c.dt_in == torch.float16 else 'f'}{'h' if c.dt_out == torch.float16 else 'f'}-{c.form}-{c.eps:g}-{c.kind}"


def adversarial_row(kind, D, dtype, g):
    """One row of width D (float64 values that ``dtype`` holds exactly once cast)."""
    r = torch.randn(D, generator=g, dtype=torch.float64)
    if kind == "constant":
        return torch.full((D,), 3.3, dtype=torch.float64)
    if kind == "offset":
        if dtype == torch.float16:                                  # fp16 numbers are 32 apart from 32768 on: 65440 + 32 {-2 .. 2}
            return 65440.0 + 32.0 * torch.randint(-2, 3, (D,), generator=g).double()
        return 1.0e3 + 1.0e-2 * r
    if kind == "spike":                                             # one massive activation, 1e4 times the rest
        r[int(torch.randint(0, D, (1,), generator=g))] = 1.0e4
        return r
    if kind == "alternating":
        return 65504.0 * (1.0 - 2.0 * (torch.arange(D) % 2).double())
    if kind == "tiny_var":                                          # variance 2^-24 and less, eps from 1e-5
        return 0.5 + 2.0 ** -11 * torch.randint(0, 2, (D,), generator=g).double()
    if kind == "zero":
        return torch.zeros(D, dtype=torch.float64)
    return 3.0 * r + 0.5


def ln_input(c):
    """-> dict(x, in_stride, gather, gamma, beta, out_stride, eps): x is the flat source buffer of c.dt_in; rows the kernel must not read hold
    IN_SENTINEL.  gather (int32 [rows] or None) has a repeated, descending and last-row index."""
    g = _gen(c.D, c.rows, DTYPES.index(c.dt_in), DTYPES.index(c.dt_out), LN_FORMS.index(c.form), LN_KINDS.index(c.kind) if c.kind in LN_KINDS else 99)
    D = c.D
    if c.kind == "adversarial":
        data = torch.stack([adversarial_row(k, D, c.dt_in, g) for k in LN_KINDS])
    else:
        data = torch.randn(c.rows, D, generator=g, dtype=torch.float64) * 3 + 0.5
    data = data.to(c.dt_in)
    L = {"in2": 2, "in7": 7, "gather_in2": 2, "gather_in7": 7}.get(c.form, 1)
    gather = None
    n_src = c.rows
    if c.form.startswith("gather"):
        n_src = c.rows + 3
        idx = [n_src - 1, n_src - 1] + list(range(n_src - 3, -1, -1))          # last row, repeated, then descending
        gather = torch.tensor(idx[:c.rows], dtype=torch.int32)
    x = torch.full((n_src, L, D), IN_SENTINEL[c.dt_in], dtype=c.dt_in)
    if gather is None:
        x[:, 0] = data
    else:
        x[:, 0] = (torch.randn(n_src, D, generator=g, dtype=torch.float64) * 2 - 0.25).to(c.dt_in)
        x[gather.long(), 0] = data                                   # (a repeated index keeps the last assignment: both reads see the same row)
    gamma = (1 + 0.1 * torch.randn(D, generator=g)).float()
    beta = (0.1 * torch.randn(D, generator=g)).float()
    out_stride = D + {"out4": 4, "out64": 64}.get(c.form, 0)
    return dict(x=x.reshape(-1), in_stride=L * D, gather=gather, gamma=gamma, beta=beta, out_stride=out_stride, eps=c.eps)


# (D, stride, what): every rejection returns CLIPMI_ERR_SHAPE (include/clipmi.h: D % 4 == 0, D <= 4096; layernorm.hip: strides % 4 == 0 and >= D)
LN_REJECTS = [(6, 8, "D % 4"), (4100, 4100, "D > 4096"), (64, 60, "stride < D"), (64, 66, "stride % 4")]

EMBED_D = [4, 252, 260, 1024, 1028, 4096]
EMBED_SHAPES = [(1, 1, 0), (3, 5, 0), (2, 5, 3), (5, 17, 2)]        # (B, L0, n_ctx): B * L is not a multiple of the four rows of a workgroup
EMBED_OUTS = ["y", "y16", "both"]
EmbedCase = collections.namedtuple("EmbedCase", "D dt B L0 n_ctx kind")
# "biased": beta sits 3/8 of an fp16 ulp above an fp16 number and gamma is 2^-16, so every output rounds DOWN to fp16: the sums of the
# roundings are D * 3/8 * 2^-10 away from the sums of the outputs
EMBED_CASES = ([EmbedCase(D, dt, B, L0, n, "random") for D in EMBED_D for dt in DTYPES for (B, L0, n) in EMBED_SHAPES] +
               [EmbedCase(D, dt, 3, 5, 1, "biased") for D in (1028, 4096) for dt in DTYPES])


def embed_case_id(c):
    return f"D{c.D}-{'h' if c.dt == torch.float16 else 'f'}-B{c.B}-L{c.L0}+{c.n_ctx}-{c.kind}"


def embed_input(c):
    """-> dict(x0, cls, pos, shallow, gamma, beta, L, tokens0): x0 [B * L, D] of c.dt, its class and prompt rows hold IN_SENTINEL."""
    g = _gen(c.D, DTYPES.index(c.dt), c.B, c.L0, c.n_ctx, c.kind == "biased")
    D, L = c.D, c.L0 + c.n_ctx
    x0 = (torch.randn(c.B, L, D, generator=g) * 2 + 0.5).to(c.dt)
    x0[:, 0] = IN_SENTINEL[c.dt]
    x0[:, c.L0:] = IN_SENTINEL[c.dt]
    cls, pos = torch.randn(D, generator=g), torch.randn(c.L0, D, generator=g) * 0.2
    shallow = torch.randn(max(c.n_ctx, 1), D, generator=g)
    if c.kind == "biased":
        gamma = torch.full((D,), 2.0 ** -16)
        beta = 1.0 + (torch.randint(0, 512, (D,), generator=g).float() + 0.375) * 2.0 ** -10
    else:
        gamma, beta = torch.rand(D, generator=g) + 0.5, torch.randn(D, generator=g) * 0.1
    return dict(x0=x0.reshape(c.B * L, D), cls=cls, pos=pos, shallow=shallow, gamma=gamma, beta=beta, L=L, tokens0=c.L0)


PatchCase = collections.namedtuple("PatchCase", "B R P D n_ctx")
PATCH_CASES = [PatchCase(1, 8, 8, 8, 0),         # M = 1, the smallest N
               PatchCase(20, 64, 16, 264, 0),    # M = 320: one full row tile exactly; N just past the 256-column tile
               PatchCase(21, 64, 16, 248, 0),    # M = 336: one row tile and 16 rows; N just under 256
               PatchCase(2, 40, 8, 256, 0),      # G = 5
               PatchCase(3, 96, 32, 72, 0),      # K = 3072
               PatchCase(7, 96, 16, 200, 3)]     # image seams inside a tile; prompt rows stay untouched
PATCH_LEAK_CASE = PatchCase(3, 32, 16, 72, 0)    # image 1 all zero between two images of pixels near 6e4


def patch_case_id(c):
    return f"B{c.B}-R{c.R}-P{c.P}-D{c.D}+{c.n_ctx}"


def patch_input(c, dtype, leak=False):
    """-> (image [B,3,R,R] of dtype, w fp16 [D, 3 P^2], pos fp32 [1 + G^2, D]).  leak: image 1 is zero, its neighbours hold pixels near 6e4 and
    the weights are scaled down so that the outputs of those stay far inside fp16."""
    g = _gen(c.B, c.R, c.P, c.D, c.n_ctx, leak)
    K, G = 3 * c.P * c.P, c.R // c.P
    image = torch.randn(c.B, 3, c.R, c.R, generator=g)
    w = torch.randn(c.D, K, generator=g) * K ** -0.5
    if leak:
        image = 6.0e4 * torch.sign(image) * (1.0 - 0.05 * torch.rand(c.B, 3, c.R, c.R, generator=g))
        image[1] = 0.0
        w = w * 0.05
    pos = torch.randn(1 + G * G, c.D, generator=g) * 0.3
    return image.to(dtype), w.half(), pos


# (B, R, P, kpad or None for the default, dtype): an explicit kpad larger than the default, G = 1 with R = P = 14, a patch size that is no multiple of 8
PATCHIFY_CASES = [(2, 32, 16, 832, torch.float32), (3, 14, 14, None, torch.float16), (1, 14, 14, 704, torch.float32), (2, 28, 14, 640, torch.float16),
                  (1, 16, 8, 256, torch.float16)]


def patchify_input(B, R, P, kpad, dtype):
    return torch.randn(B, 3, R, R, generator=_gen(B, R, P, kpad or 0)).to(dtype)


def default_kpad(P):
    return (3 * P * P + 63) // 64 * 64
