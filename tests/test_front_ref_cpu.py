"""tests/front_ref.py on the CPU: each reference agrees with an independent torch form in float64, an fp32 emulation of each kernel's
arithmetic IN THE KERNEL'S ORDER (a lane's float4 partials, then the xor butterfly, two-pass statistics; the K products 32 at a time) stays
inside the derived bound on every case of the shared tables -- that is what licenses the bounds the GPU test applies -- and the bounds are not
slack: emulations of plausible wrong kernels (a one-pass variance, a tail guard that is off by one float4, a truncating fp16 cast, fold sums
taken of the fp16 roundings) break them.  No GPU."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import front_ref as ref

WORST = {}          # operator -> worst observed error / tolerance of the emulation (printed at the end of the module: pytest -s)


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for k in sorted(WORST):
        print(f"\nemulation, worst error / tolerance: {k}: {WORST[k]:.3f}")


def _ratio(got, val, tol):
    """max |got - val| / tol, 0 / 0 = 0; NaN or anything over a zero tolerance -> inf."""
    err = (torch.as_tensor(np.asarray(got, dtype=np.float64)) - val).abs()
    r = torch.where(err == 0, torch.zeros_like(err), err / tol)
    r = torch.where(torch.isnan(r), torch.full_like(r, float("inf")), r)
    return float(r.max()) if r.numel() else 0.0


def _hold(name, got, val, tol):
    r = _ratio(got, val, tol)
    WORST[name] = max(WORST.get(name, 0.0), r)
    assert r <= 1.0, f"{name}: error / tolerance = {r}"


# ------------------------------------------------------------------------------------------------- fp32 emulations in the kernels' order
LANES = np.arange(64)


def _butterfly(s):
    """ln_wave_sum: v += shfl_xor(v, o) for o = 32 .. 1, on [n, 64] float32; every lane ends with the same bits."""
    for o in (32, 16, 8, 4, 2, 1):
        s = s + s[:, LANES ^ o]
    return s[:, :1]


def _to_f16(o, trunc):
    """fp32 -> fp16: IEEE round-to-nearest-even, or (mutant) truncation towards zero."""
    h = o.astype(np.float16)
    if trunc:
        up = np.abs(h.astype(np.float32)) > np.abs(o)
        h = np.where(up, np.nextafter(h, np.float16(0)), h)
    return h


def emulate_ln(rows, gamma, beta, eps, out_dtype=torch.float32, one_pass=False, drop_last=False, trunc=False, stats_of_fp16=False):
    """layernorm_kernel / embed_ln_kernel on fp32 rows [n, D] -> (output of out_dtype, fp16 copy, stats [n, 2]).  Mutants: one_pass (variance as
    E[x^2] - mean^2), drop_last (the statistics' guard reads c < nvec - 1), trunc (the fp16 cast truncates), stats_of_fp16 (the fold sums
    are those of the fp16 copy)."""
    x = np.ascontiguousarray(rows, dtype=np.float32)
    n, D = x.shape
    nv, nvec = ref.ln_nv(D), D // 4
    assert nvec <= nv * 64

    def lanes(a):                                         # [n, D] -> [n, NV, 64, 4]: float4 group c = lane + 64 i
        v = np.zeros((n, nv * 64, 4), np.float32)
        v[:, :nvec] = a.reshape(n, nvec, 4)
        return v.reshape(n, nv, 64, 4)

    v = lanes(x)
    live = (np.arange(nv * 64) < (nvec - 1 if drop_last else nvec)).reshape(nv, 64)      # the statistics' guard
    f0, fD = np.float32(0), np.float32(D)
    s = np.zeros((n, 64), np.float32)
    for i in range(nv):
        part = (v[:, i, :, 0] + v[:, i, :, 1]) + (v[:, i, :, 2] + v[:, i, :, 3])
        s = s + np.where(live[i], part, f0)
    mean = _butterfly(s) / fD
    q = np.zeros((n, 64), np.float32)
    for i in range(nv):
        for e in range(4):
            d = v[:, i, :, e] if one_pass else v[:, i, :, e] - mean
            q = q + np.where(live[i], d * d, f0)
    var = _butterfly(q) / fD
    if one_pass:
        var = var - mean * mean
    with np.errstate(invalid="ignore", divide="ignore"):
        rstd = (1.0 / np.sqrt((var + np.float32(eps)).astype(np.float64))).astype(np.float32)      # a correctly rounded rsqrt
        o = ((x - mean) * rstd) * gamma.numpy().astype(np.float32) + beta.numpy().astype(np.float32)
    o16 = _to_f16(o, trunc)
    w = lanes(o16.astype(np.float32) if stats_of_fp16 else o)
    os_, oq = np.zeros((n, 64), np.float32), np.zeros((n, 64), np.float32)
    for i in range(nv):
        os_ = os_ + ((w[:, i, :, 0] + w[:, i, :, 1]) + (w[:, i, :, 2] + w[:, i, :, 3]))
        oq = oq + ((w[:, i, :, 0] * w[:, i, :, 0] + w[:, i, :, 1] * w[:, i, :, 1]) + (w[:, i, :, 2] * w[:, i, :, 2] + w[:, i, :, 3] * w[:, i, :, 3]))
    stats = np.concatenate([_butterfly(os_), _butterfly(oq)], axis=1)
    return (o16 if out_dtype == torch.float16 else o), o16, stats


def emulate_patch(image, w, pos, P, out_dtype, trunc=False):
    """cast_image_kernel + the im2col GEMM: fp16 pixels and weights, their products added to an fp32 accumulator 32 at a time, pos added in
    fp32, one rounding."""
    K = 3 * P * P
    px = _to_f16(image.float().numpy(), trunc) if image.dtype == torch.float32 else image.numpy()
    a = ref.patchify(torch.from_numpy(px), P, K).float().numpy()
    W = w.float().numpy()
    acc = np.zeros((a.shape[0], W.shape[0]), np.float32)
    for k0 in range(0, K, 32):
        acc = acc + a[:, k0:k0 + 32] @ W[:, k0:k0 + 32].T
    if pos is not None:
        acc = acc + np.tile(pos.numpy()[1:], (image.shape[0], 1))
    return _to_f16(acc, trunc) if out_dtype == torch.float16 else acc


def _ln_run(c, **mutant):
    i = ref.ln_input(c)
    val, bound = ref.layer_norm_rows(i["x"], i["gamma"], i["beta"], i["eps"], rows=i["gather"], in_stride=i["in_stride"])
    rows = ref.ln_source_rows(i["x"], c.D, i["gather"], i["in_stride"]).float().numpy()
    out, _, _ = emulate_ln(rows, i["gamma"], i["beta"], i["eps"], c.dt_out, **mutant)
    return out, val, ref.tol_ln(val, bound, c.dt_out)


# ------------------------------------------------------------------------------------------------- the references against independent forms
@pytest.mark.parametrize("c", ref.LN_CASES, ids=ref.ln_case_id)
def test_layer_norm_rows_vs_torch(c):
    i = ref.ln_input(c)
    val, bound = ref.layer_norm_rows(i["x"], i["gamma"], i["beta"], i["eps"], rows=i["gather"], in_stride=i["in_stride"])
    src = i["x"].reshape(-1, i["in_stride"])[:, :c.D]
    if i["gather"] is not None:
        src = src[i["gather"].long()]
    assert src.shape[0] == c.rows and float(src.double().abs().max()) < ref.IN_SENTINEL[torch.float16] + 1      # no sentinel row among them
    want = F.layer_norm(src.double(), (c.D,), i["gamma"].double(), i["beta"].double(), i["eps"])
    assert val.shape == want.shape and bool((bound >= 0).all())
    # two float64 evaluations of a formula whose condition number is mean|x| rstd: 2^-53 times that, with a factor for the D-term sums
    cond = src.double().abs().mean(1, keepdim=True) / torch.sqrt(src.double().var(1, unbiased=False, keepdim=True) + i["eps"])
    assert bool(((val - want).abs() <= 2.0 ** -53 * 64 * (cond + 1) * (want.abs() + i["gamma"].double().abs() + 1)).all())


def test_ln_case_table_covers_what_it_names():
    cs = ref.LN_CASES
    assert {c.D for c in cs if c.form == "contig" and c.kind == "random"} == set(ref.LN_D)
    assert {c.rows for c in cs if c.kind == "random"} == set(ref.LN_ROWS)
    for form in ref.LN_FORMS:
        assert {(c.dt_in, c.dt_out) for c in cs if c.form == form} == {(a, b) for a in ref.DTYPES for b in ref.DTYPES}
        assert {ref.ln_nv(c.D) for c in cs if c.form == form} == {4, 16}
    assert {c.eps for c in cs} == set(ref.LN_EPS)
    g = ref.ln_input(next(c for c in cs if c.form == "gather" and c.rows >= 3))["gather"].tolist()
    assert g[0] == g[1] == max(g) and g[1:] == sorted(g[1:], reverse=True)        # last row, repeated, descending
    assert ref.ln_nv(1024) == 4 and ref.ln_nv(1028) == 16 and ref.ln_groups(4096) == 16 and ref.ln_groups(4) == 1


@pytest.mark.parametrize("c", ref.EMBED_CASES, ids=ref.embed_case_id)
@pytest.mark.parametrize("add_pos", [0, 1])
def test_embed_rows_vs_cat(c, add_pos):
    i = ref.embed_input(c)
    got = ref.embed_rows(i["x0"], i["cls"], i["pos"], i["shallow"], i["L"], i["tokens0"], add_pos)
    x = i["x0"].float().reshape(c.B, i["L"], c.D)[:, 1:c.L0]                                                # clip/model.py:398-401, 459-460
    x = torch.cat([(i["cls"] + i["pos"][0]).expand(c.B, 1, c.D), x + i["pos"][1:] if add_pos else x], dim=1)
    if c.n_ctx:
        x = torch.cat([x, i["shallow"][:c.n_ctx].expand(c.B, -1, -1)], dim=1)
    assert got.dtype == torch.float32 and torch.equal(got, x.reshape(-1, c.D))
    assert float(got.abs().max()) < 100                                                                     # the sentinel rows were not read


@pytest.mark.parametrize("c", ref.PATCH_CASES + [ref.PATCH_LEAK_CASE], ids=ref.patch_case_id)
@pytest.mark.parametrize("dt", ref.DTYPES)
def test_patch_rows_vs_conv2d(c, dt):
    image, w, pos = ref.patch_input(c, dt, leak=c == ref.PATCH_LEAK_CASE)
    G, tokens = c.R // c.P, 1 + (c.R // c.P) ** 2 + c.n_ctx
    val, S, rows = ref.patch_rows(image, w, pos, c.P, tokens)
    conv = F.conv2d(image.half().double(), w.double().reshape(c.D, 3, c.P, c.P), stride=c.P)                # clip/model.py:395-401
    want = conv.reshape(c.B, c.D, G * G).permute(0, 2, 1) + pos.double()[1:]
    assert bool(((val - want.reshape(-1, c.D)).abs() <= 2.0 ** -53 * 3 * c.P * c.P * (S + 1)).all())
    assert bool((S >= val.abs() - pos.double()[1:].abs().repeat(c.B, 1) - 1e-9).all())
    bare, _, _ = ref.patch_rows(image, w, None, c.P, tokens)
    assert torch.equal(bare, val - pos.double()[1:].repeat(c.B, 1)) or bool(((bare + pos.double()[1:].repeat(c.B, 1) - val).abs() <= 1e-12 * (S + 1)).all())
    assert rows.tolist() == [b * tokens + 1 + p for b in range(c.B) for p in range(G * G)]


@pytest.mark.parametrize("B,R,P,kpad,dt", ref.PATCHIFY_CASES + [(2, 224, 16, None, torch.float32), (2, 64, 32, None, torch.float32)])
def test_patchify_vs_reshape_permute(B, R, P, kpad, dt):
    img = ref.patchify_input(B, R, P, kpad, dt)
    kp, G, K = kpad or ref.default_kpad(P), R // P, 3 * P * P
    col = ref.patchify(img, P, kp)
    want = img.float().reshape(B, 3, G, P, G, P).permute(0, 2, 4, 1, 3, 5).reshape(B * G * G, K).half()
    assert col.shape == (B * G * G, kp) and torch.equal(col[:, :K], want) and bool((col[:, K:] == 0).all())


def test_pixel_code_tells_every_exchange():
    """Exchanging the values of any two of (b, c, py, px, ky, kx) changes the code wherever the two values differ, every code is an integer
    fp16 holds, and the coded image is what the formula says."""
    n = 32                                                               # every coordinate value that occurs (ky, kx < P <= 32)
    grids = torch.meshgrid(*[torch.arange(n if k >= 4 else 3) for k in range(6)], indexing="ij")      # b, c, py, px < 3; ky, kx < 32
    base = ref.code_value(*grids)
    assert int(base.min()) >= 0 and int(base.max()) < 2048
    for i in range(6):
        for j in range(i + 1, 6):
            sw = list(grids)
            sw[i], sw[j] = sw[j], sw[i]
            differ = grids[i] != grids[j]
            assert bool((ref.code_value(*sw)[differ] != base[differ]).all()), (i, j)
    for B, R, P in ref.ADDRESS_CASES:
        img = ref.coded_image(B, R, P, torch.float16)
        assert torch.equal(img.float(), ref.coded_image(B, R, P, torch.float32)) and float(img.max()) < 2048
        assert float(img[1, 2, P + 3, 5]) == ref.code_value(1, 2, 1, 0, 3, 5)


def test_tie_image_is_what_it_claims():
    t = ref.tie_image(2, 16).double().reshape(-1)
    small = t[t.abs() < 2]
    j = ((small.abs() - 1.0) * 2.0 ** 11 - 1.0) / 2.0
    assert small.numel() > 500 and torch.equal(j, j.round()) and {int(v) % 2 for v in j.tolist()} == {0, 1}      # ties, towards even both ways
    big = t[t.abs() >= 2]
    assert big.numel() > 100 and bool(((big.abs() > 65504) & (big.abs() < 65520)).all()) and bool((big < 0).any())
    h = ref.tie_image(2, 16).half()
    assert bool(torch.isfinite(h).all())
    assert np.array_equal(h.numpy(), ref.tie_image(2, 16).numpy().astype(np.float16))                           # torch's .half() is IEEE RNE
    assert not np.array_equal(_to_f16(ref.tie_image(2, 16).numpy(), True), h.numpy())                           # a truncating cast is told apart


# ------------------------------------------------------------------------------------------------- the emulations stay inside the bounds
@pytest.mark.parametrize("c", ref.LN_CASES, ids=ref.ln_case_id)
def test_ln_emulation_within_bound(c):
    out, val, tol = _ln_run(c)
    _hold(f"layernorm -> {'fp16' if c.dt_out == torch.float16 else 'fp32'}", out, val, tol)


@pytest.mark.parametrize("c", ref.EMBED_CASES, ids=ref.embed_case_id)
@pytest.mark.parametrize("add_pos", [0, 1])
def test_embed_ln_emulation_within_bound(c, add_pos):
    i = ref.embed_input(c)
    rows = ref.embed_rows(i["x0"], i["cls"], i["pos"], i["shallow"], i["L"], i["tokens0"], add_pos)
    val, bound = ref.layer_norm_rows(rows, i["gamma"], i["beta"], 1e-5)
    y, y16, stats = emulate_ln(rows.numpy(), i["gamma"], i["beta"], 1e-5)
    _hold("embed_ln y", y, val, ref.tol_ln(val, bound, torch.float32))
    _hold("embed_ln y16", y16, val, ref.tol_ln(val, bound, torch.float16))
    s, q, bs, bq = ref.fold_row_sums(torch.from_numpy(y))                      # "both": the sums of the fp32 output itself
    _hold("embed_ln stats of y", stats[:, 0], s, bs)
    _hold("embed_ln stats of y", stats[:, 1], q, bq)
    s, q, _, _ = ref.fold_row_sums(val)                                        # y16 only: against the reference's sums
    ts, tq = ref.tol_fold_of_reference(val, bound)
    _hold("embed_ln stats of the reference", stats[:, 0], s, ts)
    _hold("embed_ln stats of the reference", stats[:, 1], q, tq)


@pytest.mark.parametrize("c", ref.PATCH_CASES + [ref.PATCH_LEAK_CASE], ids=ref.patch_case_id)
@pytest.mark.parametrize("dt_in", ref.DTYPES)
@pytest.mark.parametrize("dt_out", ref.DTYPES)
@pytest.mark.parametrize("with_pos", [False, True])
def test_patch_emulation_within_bound(c, dt_in, dt_out, with_pos):
    image, w, pos = ref.patch_input(c, dt_in, leak=c == ref.PATCH_LEAK_CASE)
    pos = pos if with_pos else None
    val, S, _ = ref.patch_rows(image, w, pos, c.P, 1 + (c.R // c.P) ** 2 + c.n_ctx)
    got = emulate_patch(image, w, pos, c.P, dt_out)
    _hold(f"patch_embed -> {'fp16' if dt_out == torch.float16 else 'fp32'}", got, val, ref.tol_patch(val, S, pos, c.B, 3 * c.P * c.P, dt_out))
    if c == ref.PATCH_LEAK_CASE:                                               # the zero image: nothing but pos, rounded once
        G2 = (c.R // c.P) ** 2
        assert bool((S[G2:2 * G2] == 0).all()) and float(S[:G2].min()) > 100


def test_address_map_emulation_is_exact():
    for B, R, P in ref.ADDRESS_CASES:
        K = 3 * P * P
        for dt in ref.DTYPES:
            img = ref.coded_image(B, R, P, dt)
            for dt_out in ref.DTYPES:
                got = emulate_patch(img, torch.eye(K).half(), None, P, dt_out)
                assert np.array_equal(got.astype(np.float32), ref.patchify(img, P, K).float().numpy())


# ------------------------------------------------------------------------------------------------- the bounds are not slack: mutants break them
ADVERSARIAL = [c for c in ref.LN_CASES if c.kind == "adversarial"]


def _breaks(cases, **mutant):
    worst = 0.0
    for c in cases:
        out, val, tol = _ln_run(c, **mutant)
        worst = max(worst, _ratio(out, val, tol))
    return worst


def test_mutant_one_pass_variance_breaks_the_bound():
    for dt in ref.DTYPES:                                                      # the offset row of either input dtype
        assert _breaks([c for c in ADVERSARIAL if c.dt_in == dt], one_pass=True) > 1.0
    assert _breaks(ADVERSARIAL) <= 1.0


def test_mutant_dropped_last_float4_breaks_the_bound():
    for nv in (4, 16):                                                         # in either instantiation
        assert _breaks([c for c in ref.LN_CASES if ref.ln_nv(c.D) == nv and c.kind == "adversarial"], drop_last=True) > 1.0
    widest = [c for c in ref.LN_CASES if c.D == ref.MAX_D and c.kind == "random"]      # 4 of 4096 elements, random rows
    assert len(widest) == 4 and all(_breaks([c], drop_last=True) > 1.0 for c in widest)


def test_mutant_truncating_cast_breaks_the_bound():
    h = [c for c in ADVERSARIAL if c.dt_out == torch.float16]
    assert _breaks(h, trunc=True) > 1.0 and _breaks(h) <= 1.0
    broke = []
    for c in ref.PATCH_CASES:                                                  # the cast of the pixels and of the output, with pos and without
        image, w, pos = ref.patch_input(c, torch.float32)
        for p in (pos, None):
            val, S, _ = ref.patch_rows(image, w, p, c.P, 1 + (c.R // c.P) ** 2 + c.n_ctx)
            tol = ref.tol_patch(val, S, p, c.B, 3 * c.P * c.P, torch.float16)
            broke.append(_ratio(emulate_patch(image, w, p, c.P, torch.float16, trunc=True), val, tol) > 1.0)
    # the summation term gamma_K sum |a| |w| grows with K and covers an fp16 ulp of the output from K = 768 on: the K = 192 cases tell
    assert any(broke) and all(b for b, c in zip(broke[::2], ref.PATCH_CASES) if c.P == 8)


def test_mutant_fold_sums_of_the_fp16_roundings_break_the_bound():
    """At the widest D: the sums of fp16(o) are not the sums of o, within the bound that the sums of o keep."""
    seen = 0
    for c in ref.EMBED_CASES:
        if c.D != ref.MAX_D:
            continue
        i = ref.embed_input(c)
        rows = ref.embed_rows(i["x0"], i["cls"], i["pos"], i["shallow"], i["L"], i["tokens0"], 1)
        y, _, good = emulate_ln(rows.numpy(), i["gamma"], i["beta"], 1e-5)
        _, _, bad = emulate_ln(rows.numpy(), i["gamma"], i["beta"], 1e-5, stats_of_fp16=True)
        s, q, bs, bq = ref.fold_row_sums(torch.from_numpy(y))
        assert _ratio(good[:, 0], s, bs) <= 1.0 and _ratio(good[:, 1], q, bq) <= 1.0
        if c.kind == "biased":
            assert _ratio(bad[:, 0], s, bs) > 100 and _ratio(bad[:, 1], q, bq) > 100
        elif c.B * (c.L0 + c.n_ctx) > 4:                                       # random roundings: a walk of 4096 steps, some row leaves the bound
            assert max(_ratio(bad[:, 0], s, bs), _ratio(bad[:, 1], q, bq)) > 1.0
        seen += 1
    assert seen >= 6
