"""The LayerNorm fold and the QuickGELU epilogue at operator level (csrc/gemm.hip "LayerNorm folded into the GEMMs", quick_gelu_h / gelu_uop).

The consumer GEMM (in-proj / c_fc behind a fold producer) computes ``rstd * (x16 @ W_f^T) - rstd * mean * g + c`` with mean / variance from the
producer's fp32 row partials, ``var = E[x^2] - mean^2`` in fp64.  Each path of the consumer is run on rows of several statistical classes and
compared ROW BY ROW against two CPU references built from the same stream values:
  exact  fp64 LayerNorm -> Linear (-> QuickGELU) in fp64;
  ref16  the reference's own GPU arithmetic: F.layer_norm in fp32 -> .half() -> fp32-accumulated Linear -> .half() -> QuickGELU in fp32 -> .half().
Error of a row = max |kernel - exact| / max |exact| over the row.  Per class: max over the class <= 2 x that of ref16 and <= 2e-3.

Classes with ``|mean| / std`` >= 300, constant rows and rows with ``var ~ eps`` are the degenerate end: E[x^2] - mean^2 cancels to the rounding
noise of the fp32 partials and ``acc - mean * g`` is amplified by rstd.  Error model (u = 2^-24):
  * a partial is an fp32 sum of <= 256 terms in a tree of depth < 32: |error| <= 32 u sum|terms| = 2^-19 sum|terms|;
  * ln_inv_d = fp32(1 / D) carries one rounding (u): |d mean| <= 2^-19 mean|x| + 2^-23 |mean|, and mean^2 takes that error twice over:
    |d var| <= 2^-19 E[x^2] + 2 |mean| |d mean| + 2^-22 mean^2;
  * the MFMA's fp32 accumulation over K: |d acc[n]| <= 2^-19 sum_k |x_k W_f[n,k]|;
  => |d y[n]| <= rstd_max (d acc[n] + |d mean| |g[n]|) + max|rstd' / rstd - 1| |exact LayerNorm part[n]|, rstd' over var +- d var,
plus what the non-degenerate criterion allows (2e-3 of the row's max).  The degenerate classes assert that bound per row, and finiteness,
and print the measured error.  The bound is worst case (every rounding at its limit, in the same direction): at |mean| / std = 300 d var is
about half of var; at 1000 it exceeds var, rstd' can reach 1 / sqrt(eps) and the bound says little -- mu1000 is in effect held to finiteness.  Needs a real MI355X."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from clip_calibration_amd import _lib

pytestmark = pytest.mark.gpu

EPS = 1e-5
STRICT = ["n01", "mu1", "mu10", "mu30", "mu100", "outlier", "big"]
DEGENERATE = ["mu300", "mu1000", "const", "eps_var"]
CLASSES = STRICT + DEGENERATE
BLOCK = 32          # rows per class block; blocks cycle through CLASSES, so every class lands in every tile row and round
PER_CLASS = 256     # sampled rows per class and path (fp64 references: <= ~3k rows per case)
GELU, BIAS = _lib.EPI_BIAS_QUICKGELU, _lib.EPI_BIAS


@pytest.fixture(scope="module")
def ops():
    from clip_calibration_amd import ops as _ops
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return _ops


def class_rows(M, D, seed, device="cuda"):
    """fp32 [M, D] rows; row m belongs to CLASSES[(m // BLOCK) % len(CLASSES)]."""
    g = torch.Generator(device=device).manual_seed(seed)
    z = torch.randn(M, D, generator=g, device=device)
    cls = (torch.arange(M, device=device) // BLOCK) % len(CLASSES)
    sgn = torch.where(torch.rand(M, 1, generator=g, device=device) < 0.5, -1.0, 1.0)
    x = z.clone()
    for i, name in enumerate(CLASSES):
        r = cls == i
        if name.startswith("mu"):
            x[r] = z[r] + sgn[r] * float(name[2:])
        elif name == "outlier":     # 1..4 channels 100x the rest
            zr = z[r]
            k = torch.randint(1, 5, (zr.shape[0],), generator=g, device=device)
            ch = torch.randint(0, D, (zr.shape[0], 4), generator=g, device=device)
            for j in range(4):
                sel = k > j
                zr[sel, ch[sel, j]] *= 100.0
            x[r] = zr
        elif name == "big":         # |x| up to ~3e4
            x[r] = (z[r] * 7000.0).clamp(-3e4, 3e4)
        elif name == "const":
            x[r] = sgn[r] * 3.0 + 0.0 * z[r]
        elif name == "eps_var":     # var ~ eps around mean 1.5
            x[r] = sgn[r] * 1.5 + z[r] * EPS ** 0.5
    return x, cls


def partials(x, parts):
    """fp32 row partials [parts, M, 2] of x over `parts` equal column slices (what a producer with D / parts-column tiles writes)."""
    M, D = x.shape
    xs = x.float().view(M, parts, D // parts)
    return torch.stack([xs.sum(-1), (xs * xs).sum(-1)], -1).transpose(0, 1).contiguous()


def sample_rows(cls, M, seed, per=PER_CLASS):
    g = torch.Generator().manual_seed(seed)
    cls = cls.cpu()
    out = {}
    for i, name in enumerate(CLASSES):
        idx = torch.nonzero(cls == i).flatten()
        out[name] = idx[torch.randperm(idx.numel(), generator=g)[:per]].sort().values
    return out


class Weights:
    def __init__(self, N, D, seed):
        g = torch.Generator().manual_seed(seed)
        self.W = (torch.randn(N, D, generator=g) * D ** -0.5).half().float()   # the product's Linear weights are fp16
        self.b = torch.randn(N, generator=g) * 0.1
        self.gamma = 1.0 + 0.2 * torch.randn(D, generator=g)
        self.beta = 0.1 * torch.randn(D, generator=g)


def references(x_rows, Wt, epi):
    """(exact fp64, ref16 as fp32 tensor, LayerNorm part in fp64, rstd fp64) for fp32 rows x_rows [R, D] (the values the stream holds)."""
    x64 = x_rows.double()
    mu = x64.mean(1, keepdim=True)
    var = ((x64 - mu) ** 2).mean(1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + EPS)
    ln = (x64 - mu) * rstd
    lnpart = (ln * Wt.gamma.double()) @ Wt.W.double().t()
    pre = lnpart + Wt.beta.double() @ Wt.W.double().t() + Wt.b.double()
    exact = pre * torch.sigmoid(1.702 * pre) if epi == GELU else pre
    y16 = F.layer_norm(x_rows.float(), (x_rows.shape[1],), Wt.gamma, Wt.beta, EPS).half()
    r = (y16.float() @ Wt.W.t() + Wt.b).half()
    if epi == GELU:
        r = (r.float() * torch.sigmoid(1.702 * r.float())).half()
    return exact, r.float(), lnpart, rstd


def row_err(got, exact):
    return ((got.double() - exact).abs().amax(1) / exact.abs().amax(1).clamp_min(1e-30))


def degenerate_bound(x_rows, a16_rows, Wt, wf, gsum, lnpart, rstd, epi):
    """Per-row bound of the module docstring's error model for kernel rows computed from operand a16_rows and partials of x_rows."""
    x64, a64 = x_rows.double(), a16_rows.double()
    D = x64.shape[1]
    u19, u22, u23 = 2.0 ** -19, 2.0 ** -22, 2.0 ** -23
    mu = x64.mean(1, keepdim=True)
    var = ((x64 - mu) ** 2).mean(1, keepdim=True)
    ex2 = (x64 * x64).mean(1, keepdim=True)
    dmu = u19 * x64.abs().mean(1, keepdim=True) + u23 * mu.abs()
    dvar = u19 * ex2 + 2.0 * mu.abs() * dmu + u22 * mu * mu
    r_hi = 1.0 / torch.sqrt((var + EPS - dvar).clamp_min(EPS))
    r_lo = 1.0 / torch.sqrt(var + EPS + dvar)
    rho = torch.maximum(r_hi / rstd - 1.0, 1.0 - r_lo / rstd)
    dacc = u19 * (a64.abs() @ wf.double().abs().t())
    d = r_hi * (dacc + dmu * gsum.double().abs()[None, :]) + rho * lnpart.abs()
    # the operand's own difference from the stream values (fp32 stream: x16 = fp16(x)) enters like an accumulation error
    d = d + r_hi * ((a64 - x64).abs() @ wf.double().abs().t())
    if epi == GELU:
        d = d * 1.13   # max |d/dh h sigmoid(1.702 h)|
    return d.amax(1)


def make_refs(x_rows, a16_rows, Wt, wf, gsum, epi):
    """The references of a set of sampled rows (computed once; several kernels are checked on the same rows): exact, ref16 and the
    degenerate classes' per-row bound (absolute)."""
    exact, r16, lnpart, rstd = references(x_rows, Wt, epi)
    return dict(exact=exact, r16=r16, bound=degenerate_bound(x_rows, a16_rows, Wt, wf, gsum, lnpart, rstd, epi))


def check_classes(tag, got_rows, refs, idx_by_class, extra=None):
    """The per-class criterion on sampled rows (refs from make_refs on the same rows, in idx_by_class order); returns
    {class: (kernel err, ref16 err)} for the record."""
    rec = {}
    exact, r16, dbound = refs["exact"], refs["r16"], refs["bound"]
    e_k = row_err(got_rows, exact)
    e_r = row_err(r16, exact)
    assert bool(torch.isfinite(got_rows).all()), f"{tag}: non-finite outputs"
    scale = exact.abs().amax(1)
    bound = dbound / scale + 2e-3
    off = 0
    for name, idx in idx_by_class.items():
        sl = slice(off, off + idx.numel())
        off += idx.numel()
        ek, er = float(e_k[sl].max()), float(e_r[sl].max())
        rec[name] = (ek, er)
        print(f"{tag:28s} {name:8s} kernel {ek:.3e}  ref16 {er:.3e}")
        if name in STRICT and extra is None:
            assert ek <= max(2.0 * er, 0.0) and ek <= 2e-3, f"{tag} {name}: row error {ek:.3e} vs ref16 {er:.3e}"
        elif name in STRICT:
            # fp32 stream: the consumer's operand is fp16(x) while its statistics are those of x -- allowed on top: that term's exact value
            q = float((e_k[sl] - extra[sl]).max())
            assert q <= max(2.0 * er, 0.0) and q <= 2e-3, f"{tag} {name}: row error {ek:.3e} less the fp16-operand term: {q:.3e} vs ref16 {er:.3e}"
        else:
            assert bool((e_k[sl] <= bound[sl]).all()), f"{tag} {name}: row error {ek:.3e} above the error-model bound {float(bound[sl].min()):.3e}"
    return rec


# -------------------------------------------------------------------------------------------------------------- consumer paths
D0, N0, M0 = 768, 3072, 10240   # c_fc of a width-768 tower: 40 x 12 tiles = 1.9 rounds of the streamed kernel


@pytest.fixture(scope="module")
def fold_case(ops):
    Wt = Weights(N0, D0, 1)
    wf, gsum, c = ops.fold_layernorm_linear(Wt.W.cuda(), Wt.b.cuda(), Wt.gamma.cuda(), Wt.beta.cuda())
    x, cls = class_rows(M0, D0, 2)
    x16 = x.half()
    st4 = partials(x16.float(), 4)                                     # 4 partials of 192 columns: RAW mode (the streamed kernel's table holds 4)
    st5 = torch.cat([st4, torch.zeros_like(st4[:1])]).contiguous()    # + an all-zero 5th: the same fp64 sums through ln_finalize_kernel
    idx = sample_rows(cls, M0, 3)
    rows = torch.cat(list(idx.values()))
    return dict(Wt=Wt, wf=wf, gsum=gsum, c=c, x16=x16, st4=st4, st5=st5, idx=idx, rows=rows,
                x_rows=x16[rows.cuda()].float().cpu())


def _gelu_close(x, ref, what):
    """QuickGELU outputs of the streamed and the tile kernels.  Their fp16 pre-activations can differ by one ulp: gelu_preact's last fused
    multiply-add is rounded once, straight to fp16, where hipcc fuses it with the conversion (v_fma_mixlo_f16: the tile kernels) and twice where it
    does not (most of the streamed kernel's); the activation's product likewise (quick_gelu_h_tile once, the streamed kernel twice).  The
    activation's slope turns a pre-activation ulp into up to a few output ulps in the negative tail, so -- as in test_gpu_ops.py -- at most 2^-8
    apart, on fewer than 1e-4 of the elements."""
    d = (x.float() - ref.float()).abs()
    assert float(d.max()) <= 2.0 ** -8, f"{what}: {float(d.max()):.3e} apart"
    assert float((x != ref).float().mean()) < 1e-4, f"{what}: {float((x != ref).float().mean()):.2e} of the elements differ"


def _ulp_close(x, ref, what, frac=1e-4):
    d = (x.float() - ref.float()).abs()
    tol = torch.clamp(ref.float().abs() * (1.05 * 2.0 ** -10), min=2.0 ** -24)
    assert bool((d <= tol).all()), f"{what}: more than one fp16 ulp apart (max {float((d / tol).max()):.2f} x)"
    assert float((x != ref).float().mean()) <= frac, f"{what}: {float((x != ref).float().mean()):.2e} of the elements differ"


@pytest.mark.parametrize("epi", [GELU, BIAS], ids=["gelu", "bias"])
def test_fold_consumer_paths(ops, clipmi_option, fold_case, epi):
    """One input (every row class), every consumer path: the streamed kernel in RAW mode (4 partials); the streamed kernel behind
    ln_finalize_kernel (5 partials, the 5th all zero, ln_rows given) -- BITWISE equal to RAW: the fp64 sums are the same and
    ln_params_from_sums is one arithmetic wherever it is inlined; the tile kernels (5 partials, no scratch) and forced variants 0 / 1 / 10:
    within one fp16 ulp of the stream with BIAS, as close as _gelu_close allows with QuickGELU (1 and 10 share the epilogue code: bitwise);
    fp32 output.  Each checked per row
    class against the fp64 reference."""
    f = fold_case
    args = (f["wf"], f["c"], f["gsum"])
    run = lambda st, parts, **kw: ops.gemm_ln_fold(f["x16"], *args, st, parts, D0, EPS, epilogue=epi, **kw)
    raw = run(f["st4"], 4)
    scratch = torch.empty(M0, 2, device="cuda")
    fin = run(f["st5"], 5, ln_rows=scratch)
    assert torch.equal(raw, fin), "streamed kernel: RAW mode and ln_finalize_kernel rows differ"
    tile = run(f["st5"], 5)
    close = _ulp_close if epi == BIAS else _gelu_close
    close(tile, raw, "tile kernels (no scratch) vs streamed kernel")
    outs = {}
    for v in (0, 1, 10):
        clipmi_option("gemm_variant", v)
        outs[v] = run(f["st4"], 4)
    clipmi_option("gemm_variant", -1)
    assert torch.equal(outs[1], outs[10]), "variants 1 and 10 differ"
    close(outs[0], outs[1], "variant 0 vs 1")
    out32 = run(f["st4"], 4, out_dtype=torch.float32)
    rows = f["rows"].cuda()
    refs = make_refs(f["x_rows"], f["x_rows"], f["Wt"], f["wf"].cpu(), f["gsum"].cpu(), epi)
    for tag, out in (("stream RAW", raw), ("tile kernels", tile), ("variant 0", outs[0]), ("variant 10", outs[10])):
        check_classes(f"{tag} {'gelu' if epi == GELU else 'bias'}", out[rows].cpu(), refs, f["idx"])
    # fp32 output: nothing rounded to fp16 on the way out -- at least as close as the fp16 output
    exact = refs["exact"]
    e16 = row_err(raw[rows].cpu(), exact)
    e32 = row_err(out32[rows].cpu(), exact)
    assert bool(torch.isfinite(out32).all())
    strict = torch.cat([torch.full((f["idx"][n].numel(),), n in STRICT) for n in CLASSES])
    assert float(e32[strict].max()) <= float(e16[strict].max()) + 2.0 ** -11


@pytest.mark.parametrize("rem", [77, 200])
def test_fold_ragged_rows(ops, clipmi_option, rem):
    """A ragged last row of tiles: M % 256 = 77 goes to the tile kernels as a launch of its own (gemm_split_rows 1; the tail's partials are
    offset by the head's rows), 200 is not split.  BIAS: bitwise against the single launch; QuickGELU: _gelu_close; both per class vs fp64."""
    M = 64 * 256 + rem
    Wt = Weights(N0, D0, 4)
    wf, gsum, c = ops.fold_layernorm_linear(Wt.W.cuda(), Wt.b.cuda(), Wt.gamma.cuda(), Wt.beta.cuda())
    x, cls = class_rows(M, D0, 5)
    x16 = x.half()
    st = partials(x16.float(), 3)
    tail = torch.arange(M - rem, M)
    for epi in (BIAS, GELU):
        clipmi_option("gemm_split_rows", 0)
        one = ops.gemm_ln_fold(x16, wf, c, gsum, st, 3, D0, EPS, epilogue=epi)
        clipmi_option("gemm_split_rows", 1)
        two = ops.gemm_ln_fold(x16, wf, c, gsum, st, 3, D0, EPS, epilogue=epi)
        if epi == BIAS:
            assert torch.equal(one, two)
        else:
            _gelu_close(two, one, "split vs single launch")
        idx = sample_rows(cls, M, 6, per=96)
        idx = {n: torch.cat([i, tail[cls[tail].cpu() == k]]).unique() for k, (n, i) in enumerate(idx.items())}   # every tail row
        rows = torch.cat(list(idx.values()))
        xr = x16[rows.cuda()].float().cpu()
        check_classes(f"ragged {rem} {'gelu' if epi == GELU else 'bias'}", two[rows.cuda()].cpu(), make_refs(xr, xr, Wt, wf.cpu(), gsum.cpu(), epi), idx)


def test_fold_class_rows_plane_and_stride(ops, fold_case):
    """The class-row form of the image tower's last block: statistics in a [parts][n L] plane, the consumer on rows n L (ln_plane = n L,
    ln_row_stride = L) -- bitwise equal to the same launch on compacted statistics (plane = n, stride 1), and per class vs fp64."""
    f = fold_case
    L, n = 197, 48
    x, cls = class_rows(n * L, D0, 7)
    x16 = x.half()
    st = partials(x16.float(), 3)
    a = x16[::L].contiguous()
    strided = ops.gemm_ln_fold(a, f["wf"], f["c"], f["gsum"], st, 3, D0, EPS, ln_plane=n * L, ln_row_stride=L, epilogue=GELU)
    compact = ops.gemm_ln_fold(a, f["wf"], f["c"], f["gsum"], st[:, ::L].contiguous(), 3, D0, EPS, epilogue=GELU)
    assert torch.equal(strided, compact)
    idx = {name: torch.nonzero(cls[::L].cpu() == k).flatten() for k, name in enumerate(CLASSES)}
    rows = torch.cat(list(idx.values()))
    xr = a[rows.cuda()].float().cpu()
    check_classes("class rows", strided[rows.cuda()].cpu(), make_refs(xr, xr, f["Wt"], f["wf"].cpu(), f["gsum"].cpu(), GELU), idx)


def test_fold_beyond_one_descriptor(ops):
    """A consumer beyond the 2 GiB one descriptor addresses (270 000 x 4096 fp16 outputs): consecutive streamed launches over row ranges, each
    with the statistics pointer offset by the range's first row (ln_M stays the producer's M).  Rows +-300 around the range boundary per class
    vs fp64; a streamed window of 8192 rows across the boundary (statistics + 2 r0, ln_plane = M) bitwise equal to those rows."""
    M, D, N = 270000, 1024, 4096
    Wt = Weights(N, D, 8)
    wf, gsum, c = ops.fold_layernorm_linear(Wt.W.cuda(), Wt.b.cuda(), Wt.gamma.cuda(), Wt.beta.cuda())
    x, cls = class_rows(M, D, 9)
    x16 = x.half()
    del x
    st = partials(x16.float(), 4)
    out = ops.gemm_ln_fold(x16, wf, c, gsum, st, 4, D, EPS, epilogue=GELU)
    assert out.numel() * 2 > 2 ** 31
    # rows per launch: the formula of launch_one in csrc/gemm.hip (the range that keeps a matrix inside one descriptor, capped by the
    # traversal's tile-id limit) -- mirrored here so that the rows checked below straddle the real boundary; change both together
    step = min((((2 ** 31 - 2 ** 25) // (2 * max(D, N))) - 256) // 256 * 256, (1 << 16) // ((N + 255) // 256) * 256)
    assert 8192 < step < M - 4096
    r0, Wn = step - 4096, 8192
    win = ops.gemm_ln_fold(x16[r0:r0 + Wn], wf, c, gsum, st.view(-1)[2 * r0:], 4, D, EPS, ln_plane=M, epilogue=GELU)
    assert torch.equal(win, out[r0:r0 + Wn])
    near = torch.arange(step - 300, step + 300)
    idx = {name: near[cls[near].cpu() == k] for k, name in enumerate(CLASSES)}
    rows = torch.cat(list(idx.values()))
    xr = x16[rows.cuda()].float().cpu()
    check_classes("beyond one descriptor", out[rows.cuda()].cpu(), make_refs(xr, xr, Wt, wf.cpu(), gsum.cpu(), GELU), idx)
    assert torch.isfinite(out[::1009]).all()


# -------------------------------------------------------------------------------------------------------------- producer -> consumer
@pytest.mark.parametrize("stream", ["f32", "f16"])
def test_fold_producer_chain(ops, fold_case, stream):
    """Producer -> consumer with the producer's own partials.  The residual update a @ W_p^T + b_p is subtracted from the class rows up front,
    so the updated stream holds the row classes.
    fp32 stream (clipmi_gemm_residual_fold): x16 == fp16(x) bitwise; x within fp32 rounding of fp64; the partials match fp64 sums of the FP32
    row (what the epilogue sums), not of the rounded one.  The consumer then multiplies fp16(x) by W_f while its mean comes from x: the
    difference rstd * (fp16(x) - x) @ W_f^T grows like 2^-11 |mean| rstd ~ 2^-11 |mean| / std -- 5e-3 of a row at |mean| / std = 10, more than
    the 2e-3 criterion.  That term is computed exactly per row in fp64 and allowed on top of the criterion; the rest must meet it.
    fp16 stream (clipmi_gemm_residual_f16): partials of the rounded row; the usual per-class criterion."""
    f = fold_case
    M, D = M0, D0
    g = torch.Generator().manual_seed(10)
    a = (torch.randn(M, D, generator=g) * 0.5).half().cuda()
    Wp = (torch.randn(D, D, generator=g) * 0.02).half().cuda()
    bp = (torch.randn(D, generator=g) * 0.05).cuda()
    target, cls = class_rows(M, D, 11)
    upd = a.float() @ Wp.float().t() + bp
    if stream == "f32":
        x_old = (target - upd).contiguous()
        x = x_old.clone()
        x16, st, parts = ops.gemm_residual_fold(a, Wp, bp, x)
        assert parts in (3, 6)   # 256-column tiles, or 128 where the dispatcher picks the 128 x 128 kernel
        assert torch.equal(x16, x.half())
    else:
        x16_old = (target - upd).half()
        x16 = x16_old.clone()
        st, parts = ops.gemm_residual_f16(a, Wp, bp, x16)
        assert parts in (3, 6)
        x = x16.float()
    idx = sample_rows(cls, M, 12)
    rows = torch.cat(list(idx.values()))
    rc = rows.cuda()
    xr = x[rc].cpu()
    if stream == "f32":
        x64 = x_old[rc].double().cpu() + a[rc].double().cpu() @ Wp.double().cpu().t() + bp.double().cpu()
        tol = 2.0 ** -23 * x64.abs() + 2.0 ** -19 * ((a[rc].double().abs() @ Wp.double().abs().t()).cpu() + x_old[rc].double().abs().cpu() + bp.double().abs().cpu())
        assert bool(((xr.double() - x64).abs() <= tol).all()), "fp32 stream: x further from fp64 than fp32 rounding allows"
        xs = xr.double().view(-1, parts, D // parts)
        s64, ss64 = xs.sum(-1), (xs * xs).sum(-1)
        stc = st[:parts, rc].double().cpu().transpose(0, 1)
        assert bool(((stc[..., 0] - s64).abs() <= 2.0 ** -19 * xs.abs().sum(-1)).all()), "fp32 stream: row sums are not those of the fp32 row"
        assert bool(((stc[..., 1] - ss64).abs() <= 2.0 ** -19 * ss64).all()), "fp32 stream: row sums of squares are not those of the fp32 row"
    out = ops.gemm_ln_fold(x16, f["wf"], f["c"], f["gsum"], st, parts, D, EPS, epilogue=GELU)
    a16 = x16[rc].float().cpu()
    extra = None
    if stream == "f32":
        exact = references(xr, f["Wt"], GELU)[0]
        mu = xr.double().mean(1, keepdim=True)
        rstd = 1.0 / torch.sqrt(((xr.double() - mu) ** 2).mean(1, keepdim=True) + EPS)
        q = (rstd * ((a16.double() - xr.double()) @ f["wf"].cpu().double().t())).abs() * 1.13
        extra = q.amax(1) / exact.abs().amax(1)
    check_classes(f"producer {stream} -> consumer", out[rc].cpu(), make_refs(xr, a16, f["Wt"], f["wf"].cpu(), f["gsum"].cpu(), GELU), idx, extra=extra)


# -------------------------------------------------------------------------------------------------------------- QuickGELU, every fp16 input
def _quick_gelu_lut():
    """Correctly rounded fp16 of h sigmoid(1.702 h) = h / (1 + exp(-1.702 h)) for all 65 536 fp16 patterns (fp64, one rounding)."""
    h = np.arange(65536, dtype=np.uint32).astype(np.uint16).view(np.float16).astype(np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        y = h / (1.0 + np.exp(-1.702 * h))
    return torch.from_numpy(y.astype(np.float16).view(np.int16).astype(np.int32) & 0xFFFF)


def test_quick_gelu_every_finite_fp16_preactivation(ops, clipmi_option):
    """Every finite fp16 pre-activation through every form of the QuickGELU epilogue.  a[m, k] = 1 for k = m mod 64 (else 0), K = 512,
    w[n, 0..63] = the 63 488 finite fp16 bit patterns (cycled over n), bias 0: output (m, n) is the activation of exactly w[n, m mod 64].
    (inf / NaN cannot be placed: inf * 0 is NaN in the zero terms of the dot product; -0 arrives as +0: the accumulator starts at +0.)
    c_fc's shape 50432 x 3072: ~89 % of the tiles take the streamed kernel's in-loop inline-asm sequence (gelu_uop), the rest its last-tile tail
    (quick_gelu_h1).  Also: gemm_stream 0 (tile kernels), variants 0 / 1 / 10, the split tail (M % 256 = 77), and the folded entry with one
    partial (sum 0, sum of squares 512, ln_dim 512, eps 0): mean = 0 and var = 1 EXACTLY, rsqrtf(1) = 1, so the pre-activation is unchanged.
    Against a LUT of correctly rounded fp64 results, on every path: <= 1 fp16 ulp, the sign of a zero equal to the LUT's, no NaN.  Bitwise:
    every 64-row group of the streamed kernel's output (in-loop and tail tiles alike) is the same and the folded entry equals it; the tile
    kernels equal each other (they round the product once, the streamed kernel twice: the count of differing outputs is printed); the split
    launch's head equals the streamed kernel, its tail the tile kernels."""
    M, N, K = 50432, 3072, 512
    pats = torch.arange(65536, dtype=torch.int32)
    pats = pats[(pats & 0x7C00) != 0x7C00]
    assert pats.numel() == 63488
    wbits = pats[torch.arange(N * 64) % 63488].view(N, 64)
    w = torch.zeros(N, K, dtype=torch.float16)
    w[:, :64] = wbits.to(torch.int16).view(torch.float16)
    eff = torch.where(wbits == 0x8000, torch.zeros_like(wbits), wbits)          # -0 -> +0
    lut = _quick_gelu_lut()
    expect = lut[eff.t()].cuda()                                                # [64, N]: expected bits of output row m at m % 64
    a = torch.zeros(M, K, dtype=torch.float16)
    a[torch.arange(M), torch.arange(M) % 64] = 1.0
    a, w = a.cuda(), w.cuda()
    zero = torch.zeros(N, device="cuda")

    def bits(out):
        return out.view(torch.int16).to(torch.int32) & 0xFFFF

    ordv = lambda b: torch.where(b >= 0x8000, -(b & 0x7FFF), b)                 # fp16 bits -> ordinal (+-0 -> 0)

    def against_lut(out, what):
        got = bits(out).view(-1, 64, N)
        ex = expect[None].expand_as(got)
        assert not bool(torch.isnan(out).any()), f"{what}: NaN from a finite pre-activation"
        far = (ordv(got) - ordv(ex)).abs() > 1
        assert not bool(far.any()), f"{what}: {int(far.sum())} outputs more than one fp16 ulp from the correctly rounded activation"
        zero_bits = ((got & 0x7FFF) == 0) | ((ex & 0x7FFF) == 0)
        wrong_sign = int((zero_bits & ((got ^ ex) & 0x8000 != 0)).sum())
        assert wrong_sign == 0, f"{what}: {wrong_sign} zeros of the wrong sign"
        print(f"QuickGELU {what}: {int((got != ex).sum())} of {got.numel()} outputs 1 ulp from the correctly rounded result")
        return got

    base = ops.gemm_f16(a, w, zero, epilogue=GELU, out_dtype=torch.float16)
    groups = against_lut(base, "streamed kernel")
    same = (groups == groups[:1]).flatten(1).all(1)
    assert bool(same.all()), f"streamed kernel: {int((~same).sum())} of {same.numel()} 64-row groups differ from the first (in-loop vs tail form)"
    del groups, same
    st = torch.zeros(1, M, 2, device="cuda")
    st[..., 1] = float(K)
    g = w.float().sum(1)
    fold = ops.gemm_ln_fold(a, w, zero, g, st, 1, K, 0.0, epilogue=GELU)
    assert torch.equal(bits(fold), bits(base)), "folded entry (rstd 1, mean 0): QuickGELU bits differ from the plain streamed kernel's"
    tile = None
    for name, opt in (("gemm_stream 0", ("gemm_stream", 0)), ("variant 0", ("gemm_variant", 0)), ("variant 1", ("gemm_variant", 1)),
                      ("variant 10", ("gemm_variant", 10))):
        clipmi_option(*opt)
        out = ops.gemm_f16(a, w, zero, epilogue=GELU, out_dtype=torch.float16)
        clipmi_option(opt[0], 1 if opt[0] == "gemm_stream" else -1)   # back to the default dispatch
        against_lut(out, name)
        if tile is None:
            tile = out
            print(f"QuickGELU tile kernels vs streamed kernel: {int((bits(tile) != bits(base)).sum())} outputs differ (one rounding of the product against two)")
        assert torch.equal(bits(out), bits(tile)), f"{name}: QuickGELU bits differ between the tile kernels"
    Ms = 64 * 256 + 77
    split = ops.gemm_f16(a[:Ms], w, zero, epilogue=GELU, out_dtype=torch.float16)
    head = Ms // 256 * 256
    assert torch.equal(bits(split[:head]), bits(base[:head])), "split tail: the streamed head's QuickGELU bits differ"
    assert torch.equal(bits(split[head:]), bits(tile[head:Ms])), "split tail: the tail launch's bits differ from the tile kernels'"
