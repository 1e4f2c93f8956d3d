"""Reference of the training text tower's two drivers, clipmi_text_encoder_train and clipmi_text_encoder_backward (the bottom of
csrc/text_backward.hip), stage by stage -- the oracle of tests/test_towertrain_cpu.py and tests/test_gpu_towertrain.py.  It does not
import the package but for weights and geometry (clip_calibration_amd.synthetic), as the other *_ref.py files do.

What lives here:
* StashLayout: the byte layout of the stash as include/clipmi.h states it, as views into a uint8 tensor.
* Towers: ``tiny`` and ``tiny3`` as they are, and a pass-through variant of each in which attn.out_proj.weight and mlp.c_proj.weight of
  every block are zero (the biases stay): the backward through the blocks then adds exact zeros, so d_embed is the tail alone.
* CASES, and the inputs of a case (prompts, ctx, eot, positional rows).
* Float64 stage references, each evaluated FROM THE STASHED INPUT OF THAT STAGE, so that every stage is judged alone, each with a bound
  per element that is derived from the formats and the summation (none measured):
    LayerNorm -> fp16 -> GEMM with fp16 weights (in-projection, c_fc, ln_final + text_projection):
        front_ref.layer_norm_rows / tol_ln for the fp16 LayerNorm output y, then, as tests/text_ref.py states it,
        |got - (y W^T + b)| <= sum_k tol_ln(y)_k |W_nk| + gamma_k(K + 1) (sum_k |y_k W_nk| + |b_n|), and one output rounding (fp16: u16
        relative + half a subnormal step, front_ref's _out_rounding; fp32: contained in gamma_k);
    attention -> out-projection + bias + residual: attention_ref.attention's per-element bound of the fp16 attention output o, then
        sum_k tol(o)_k |W_nk| + gamma_k(K + 2) (sum_k |o_k W_nk| + |b_n| + |x_in|), fp32 output;
    QuickGELU -> c_proj + bias + residual: a = fp16(h sigmoid(1.702 h)) of the STASHED fp16 h is within one fp16 ulp of the correctly
        rounded value (the criterion of tests/test_gpu_ln_fold.py's QuickGELU test: 2 u16 |a| + 2^-24 covers one ulp), then as above, K = 4 D.
* backward64: coopfit_ref.block_backward chained over the layers plus the tail, from a stash (StashView) and a d_out, the full stream
  g [C L, D].
* emulate_backward: the device's backward on the CPU in fp32 with the device's fp16 rounding points (dfeat16, g16, d_a, d_h, d_att, dqkv,
  P and dS) -- the yardstick of the whole-backward test: the device may miss float64 by FACTOR times what this emulation misses it by.
* emulate_forward: the forward stages in fp32 with the same rounding points, and its mutants (MUTANTS).

``gelu on the unrounded pre-activation`` is deliberately not among the mutants: neither a = QuickGELU(h) nor the fp32 pre-activation
is stashed, so the only witness is x_in(i + 1) = x_mid + a W^T + b behind a K = 4 D fp32 accumulation, and the mutant moves a by at most
one fp16 ulp per element -- the very slack the derived bound of that stage must grant the correct kernel (see tol of ``stage_x_out``).
"""
from __future__ import annotations

import collections
import functools

import torch

import attention_ref
import coopfit_ref as cref
import front_ref
from clip_calibration_amd import synthetic as syn     # weights and geometry only
from front_ref import gamma_k

F16, F32 = torch.float16, torch.float32
U16, U32 = 2.0 ** -11, 2.0 ** -24
EPS = 1e-5
FACTOR = 2.0            # the project's factor between a CPU emulation's error and the device's (fast exponential, other summation order)
STATS_GRID = 1024 * 256  # operand_stats_kernel: elements one sweep of its grid covers


def align256(n):
    return (n + 255) // 256 * 256


# ------------------------------------------------------------------------------------------------------------------- the stash layout
class StashLayout:
    """include/clipmi.h, clipmi_text_encoder_train: offsets in bytes, and views into a uint8 tensor that holds a stash."""

    def __init__(self, C, L, D, layers):
        self.C, self.L, self.D, self.layers, self.M = C, L, D, layers, C * L
        self.x_bytes = align256(self.M * D * 4)
        self.qkv_bytes = align256(self.M * D * 6)
        self.h_bytes = align256(self.M * D * 8)
        self.qkv_off = (2 * layers + 1) * self.x_bytes
        self.h_off = self.qkv_off + layers * self.qkv_bytes
        self.idx_off = self.h_off + layers * self.h_bytes
        self.bytes = self.idx_off + align256(C * 8)

    def _view(self, buf, off, n, dtype, cols):
        return buf[off:off + n * torch.empty(0, dtype=dtype).element_size()].view(dtype).reshape(-1, cols)

    def x(self, buf, k):
        """fp32 [M, D]: slab k of x_in(0), x_mid(0), x_in(1), ..., the input of ln_final (k = 2 layers)."""
        return self._view(buf, k * self.x_bytes, self.M * self.D, F32, self.D)

    def qkv(self, buf, i):
        return self._view(buf, self.qkv_off + i * self.qkv_bytes, self.M * 3 * self.D, F16, 3 * self.D)

    def h(self, buf, i):
        return self._view(buf, self.h_off + i * self.h_bytes, self.M * 4 * self.D, F16, 4 * self.D)

    def idx(self, buf):
        return self._view(buf, self.idx_off, self.C, torch.int32, 1).reshape(-1)

    def pack(self, xs, qkvs, hs, idx):
        """A stash from its parts (the CPU emulation's): uint8 [bytes], the padding zero."""
        buf = torch.zeros(self.bytes, dtype=torch.uint8)
        for k, t in enumerate(xs):
            self.x(buf, k).copy_(t)
        for i in range(self.layers):
            self.qkv(buf, i).copy_(qkvs[i])
            self.h(buf, i).copy_(hs[i])
        self.idx(buf).copy_(idx)
        return buf


# ---------------------------------------------------------------------------------------------------------------------------- towers
TOWERS = ("tiny", "tiny3", "tiny-pass", "tiny3-pass", "tiny-pass-quiet", "tiny3-pass-quiet")
PASS_THROUGH = ("attn.out_proj.weight", "mlp.c_proj.weight")
QUIET = 2.0 ** -8       # "-quiet": text_projection scaled down (and rounded to fp16 again), so that a d_out element of 65504 -- the operand
#                         statistics' largest fp16 number -- leaves a gradient stream that fp16 still holds: an infinity in g16 times a zero
#                         weight is a NaN, and the c_fc and qkv gradients of a pass-through tower would no longer be zeros


def base(tower):
    return tower.split("-")[0]


def geometry(tower):
    return syn.GEOMETRIES[base(tower)]


@functools.lru_cache(maxsize=None)
def state_dict(tower):
    """Cached: callers copy the dict, never edit its tensors."""
    sd = {k: v.clone() for k, v in cref.state_dict(base(tower)).items()}
    if "-pass" in tower:
        for i in range(geometry(tower).transformer_layers):
            for k in PASS_THROUGH:
                sd[f"transformer.resblocks.{i}.{k}"].zero_()
    if tower.endswith("-quiet"):
        sd["text_projection"] = (sd["text_projection"] * QUIET).half().float()
    return sd


def long_state_dict(rows=88):
    """``tiny`` with a positional embedding of ``rows`` rows: a tower whose live rows exceed the attention backward's 80."""
    sd = dict(state_dict("tiny"))
    g = torch.Generator().manual_seed(88)
    sd["positional_embedding"] = (0.01 * torch.randn(rows, sd["positional_embedding"].shape[1], generator=g)).half().float()
    return sd


# ----------------------------------------------------------------------------------------------------------------------------- cases
# ctx: "shared" [n_ctx, D] | "class" [C, n_ctx, D] | None (ctx = NULL: the prompts' own rows 1..n_ctx stay);  seq_rows 0: the whole context
Case = collections.namedtuple("Case", "tower C n_ctx seq_rows dtype ctx far")
CASES = [
    Case("tiny", 3, 4, 16, F16, "shared", False),
    Case("tiny", 3, 4, 0, F16, "shared", False),          # the same uncut: the pair of the cut-against-uncut test
    Case("tiny", 2, 1, 8, F32, "class", False),
    Case("tiny", 37, 4, 16, F16, "class", False),         # M 4D = 303 104 > 1024 * 256: operand_stats_kernel strides its grid twice
    Case("tiny", 3, 4, 16, F32, None, False),
    Case("tiny3", 3, 16, 24, F32, "shared", False),
    Case("tiny3", 3, 16, 0, F32, "shared", False),        # its uncut pair
    Case("tiny3", 2, 7, 8, F16, "class", False),          # n_ctx = L - 1: the context fills every live row but SOT
    Case("tiny3", 3, 4, 0, F16, "shared", True),          # the last prompt's EOT on row L - 1 = 76
    Case("tiny3", 37, 4, 16, F32, "shared", False),
]
UNCUT_PAIRS = [(CASES[0], CASES[1]), (CASES[5], CASES[6])]


def case_id(c):
    return (f"{c.tower}-C{c.C}-n{c.n_ctx}-r{c.seq_rows}-{'h' if c.dtype == F16 else 'f'}-{c.ctx or 'null'}" + ("-far" if c.far else ""))


def on_tower(c, tower):
    return c._replace(tower=tower)


def live_rows(c):
    Lc = geometry(c.tower).context_length
    return c.seq_rows if 0 < c.seq_rows < Lc else Lc


@functools.lru_cache(maxsize=None)
def case_input(c):
    """dict: prompts [C, context, D] of c.dtype (token embeddings, no positional rows; fp32 ones are moved off the fp16 grid), ctx fp32 or
    None, eot int32 [C], pos fp32 [context, D], d_out fp32 [C, E].  Rows behind the cut hold a sentinel the kernels must not read."""
    g = geometry(c.tower)
    sd = state_dict(c.tower)
    L, D = live_rows(c), g.transformer_width
    gen = front_ref._gen(g.transformer_width, c.C, c.n_ctx, c.dtype == F16, len(c.ctx or ""), c.far)      # not of seq_rows: a cut changes the cut alone
    ids = cref.prompt_ids(base(c.tower), c.C, c.n_ctx, 0, c.far)
    eot = ids.argmax(dim=-1).to(torch.int32)
    if c.n_ctx == L - 1:                      # no name fits: the EOT is the caller's variable, a context row or SOT stands in for it
        eot = (torch.arange(c.C, dtype=torch.int32) * 3 + L - 1) % L
    assert int(eot.max()) < L
    prompts = sd["token_embedding.weight"][ids].float()
    if c.dtype == F32:
        prompts = prompts + 1e-4 * torch.randn(prompts.shape, generator=gen)
    prompts = prompts.to(c.dtype)
    prompts[:, L:] = front_ref.IN_SENTINEL[c.dtype]
    shape = {"shared": (c.n_ctx, D), "class": (c.C, c.n_ctx, D), None: None}[c.ctx]
    ctx = None if shape is None else 0.02 * torch.randn(*shape, generator=gen)
    d_out = torch.randn(c.C, g.embed_dim, generator=gen)
    return dict(prompts=prompts, ctx=ctx, eot=eot, pos=sd["positional_embedding"].float(), d_out=d_out)


# ------------------------------------------------------------------------------------------------------- stage 0: the embedding, exact
def embed(c, inp, mutant=None):
    """x_in(0) fp32 [C L, D], exact: float(prompt) + pos by ONE IEEE fp32 addition, the context in rows 1..n_ctx.  Mutants: ctx_prev_class,
    ctx_shift, pos_stride (MUTANTS)."""
    L, D = live_rows(c), inp["pos"].shape[1]
    v = inp["prompts"][:, :L].float().clone()
    if inp["ctx"] is not None:
        ctx = inp["ctx"] if inp["ctx"].dim() == 3 else inp["ctx"][None].expand(c.C, -1, -1)
        if mutant == "ctx_prev_class":
            ctx = ctx.roll(1, dims=0)
        lo = 0 if mutant == "ctx_shift" else 1
        v[:, lo:lo + c.n_ctx] = ctx
    pos = inp["pos"][:L][None].expand(c.C, -1, -1)
    if mutant == "pos_stride":                # the row of the flat index taken modulo the context, not modulo the live rows
        Lc = inp["pos"].shape[0]
        pos = inp["pos"][torch.arange(c.C * L) % Lc].reshape(c.C, L, D)
    return (v + pos).reshape(c.C * L, D)


def eot_rows(c, inp):
    L = live_rows(c)
    return (torch.arange(c.C, dtype=torch.int32) * L + inp["eot"].clamp(0, L - 1)).to(torch.int32)


# ------------------------------------------------------------------------------------------------- float64 stage references and bounds
def _w(sd, i, dtype=torch.float64):
    return cref.block_weights(sd, i, dtype)


def _ln_gemm(x, gamma, beta, W, bias, out_dtype):
    """fp16(LayerNorm(x)) @ W^T + bias -> (value, tol) float64 (module docstring).  W [N, K]: fp16 numbers."""
    y, b = front_ref.layer_norm_rows(x, gamma, beta, EPS)
    tol_y = front_ref.tol_ln(y, b, F16)
    Wd = W.double()
    assert torch.equal(W.half().double(), Wd)
    val = y @ Wd.t()
    mag = y.abs() @ Wd.abs().t()
    if bias is not None:
        val, mag = val + bias.double(), mag + bias.double().abs()
    tol = tol_y @ Wd.abs().t() + gamma_k(W.shape[1] + 1) * mag
    if out_dtype == F16:
        tol = tol + U16 * (val.abs() + tol) + 0.5 * U32
    return val, tol


def _gemm_residual(a, tol_a, W, bias, res):
    """res + a @ W^T + bias in fp32 from an fp16 operand known within tol_a -> (value, tol) float64."""
    Wd, r = W.double(), res.double()
    val = r + a @ Wd.t() + bias.double()
    tol = tol_a @ Wd.abs().t() + gamma_k(W.shape[1] + 2) * (a.abs() @ Wd.abs().t() + bias.double().abs() + r.abs())
    return val, tol


def stage_qkv(sd, i, x_in):
    w = _w(sd, i)
    return _ln_gemm(x_in, w["ln_1.weight"], w["ln_1.bias"], w["attn.in_proj_weight"], w["attn.in_proj_bias"], F16)


def stage_x_mid(sd, i, qkv, x_in, C, L, H):
    w = _w(sd, i)
    o, tol_o = attention_ref.attention(qkv, C, L, H, True)
    D = 64 * H
    return _gemm_residual(o.reshape(C * L, D), tol_o.reshape(C * L, D), w["attn.out_proj.weight"], w["attn.out_proj.bias"], x_in)


def stage_h(sd, i, x_mid):
    w = _w(sd, i)
    return _ln_gemm(x_mid, w["ln_2.weight"], w["ln_2.bias"], w["mlp.c_fc.weight"], w["mlp.c_fc.bias"], F16)


def stage_x_out(sd, i, h, x_mid):
    w = _w(sd, i)
    a = cref.quickgelu(h.double()).half().double()                 # the correctly rounded activation of the stashed fp16 h
    return _gemm_residual(a, 2 * U16 * a.abs() + U32, w["mlp.c_proj.weight"], w["mlp.c_proj.bias"], x_mid)


def stage_features(sd, x_last, idx):
    return _ln_gemm(x_last[idx.long()], sd["ln_final.weight"], sd["ln_final.bias"], sd["text_projection"].t(), None, F32)


def forward_stages(tower, C, L, stash, lay):
    """[(name, stashed value, reference, tol)] of every stage behind the embedding, each from the stash's own input of that stage; the
    last entry is ("features", None, reference, tol)."""
    sd = state_dict(tower)
    H = geometry(tower).transformer_heads
    out = []
    for i in range(lay.layers):
        x_in, x_mid, x_out = lay.x(stash, 2 * i), lay.x(stash, 2 * i + 1), lay.x(stash, 2 * i + 2)
        qkv, h = lay.qkv(stash, i), lay.h(stash, i)
        out.append((f"qkv({i})", qkv) + stage_qkv(sd, i, x_in))
        out.append((f"x_mid({i})", x_mid) + stage_x_mid(sd, i, qkv, x_in, C, L, H))
        out.append((f"h({i})", h) + stage_h(sd, i, x_mid))
        out.append((f"x_in({i + 1})", x_out) + stage_x_out(sd, i, h, x_mid))
    out.append(("features", None) + stage_features(sd, lay.x(stash, 2 * lay.layers), lay.idx(stash)))
    return out


def worst_ratio(got, want, tol):
    r = (got.double().reshape(want.shape) - want).abs() / tol
    r[torch.isnan(r)] = float("inf")
    return float(r.max())


# -------------------------------------------------------------------------------------------------------- fp32 emulation of the forward
MUTANTS = ("resid_x_in",        # c_proj's residual taken from x_in instead of x_mid
           "no_b_out",          # out-proj's bias dropped
           "ctx_prev_class",    # the context of class c - 1 under per-class
           "ctx_shift",         # context rows shifted by one: rows 0 .. n_ctx - 1
           "pos_stride",        # the positional row taken with stride context_length under the cut
           "ln2_from_x_in",     # ln_2's statistics taken from x_in
           "eot_late")          # the EOT scatter one row late


def _ln32(x, gamma, beta, stats_of=None):
    s = x if stats_of is None else stats_of
    mean = s.mean(-1, keepdim=True)
    rstd = torch.rsqrt(((s - mean) ** 2).mean(-1, keepdim=True) + EPS)
    return ((x - mean) * rstd * gamma + beta).half()


def _gelu32(h16):
    h = h16.float()
    return (h * torch.sigmoid(1.702 * h)).half()


def emu_qkv(sd, i, x_in):
    w = _w(sd, i, F32)
    return (_ln32(x_in, w["ln_1.weight"], w["ln_1.bias"]).float() @ w["attn.in_proj_weight"].t() + w["attn.in_proj_bias"]).half()


def emu_x_mid(sd, i, qkv, x_in, C, L, H, mutant=None):
    w = _w(sd, i, F32)
    o = attention_ref.emulate(qkv, C, L, H, True).reshape(C * L, 64 * H).float()
    y = o @ w["attn.out_proj.weight"].t()
    if mutant != "no_b_out":
        y = y + w["attn.out_proj.bias"]
    return x_in + y


def emu_h(sd, i, x_mid, x_in, mutant=None):
    w = _w(sd, i, F32)
    y = _ln32(x_mid, w["ln_2.weight"], w["ln_2.bias"], x_in if mutant == "ln2_from_x_in" else None)
    return (y.float() @ w["mlp.c_fc.weight"].t() + w["mlp.c_fc.bias"]).half()


def emu_x_out(sd, i, h, x_mid, x_in, mutant=None):
    w = _w(sd, i, F32)
    return (x_in if mutant == "resid_x_in" else x_mid) + (_gelu32(h).float() @ w["mlp.c_proj.weight"].t() + w["mlp.c_proj.bias"])


def emu_features(sd, x_last, idx, mutant=None):
    rows = idx.long()
    if mutant == "eot_late":
        rows = (rows + 1).clamp_max(x_last.shape[0] - 1)
    y = _ln32(x_last[rows], sd["ln_final.weight"].float(), sd["ln_final.bias"].float())
    return y.float() @ sd["text_projection"].half().float()


def emulate_forward(c, inp):
    """-> (stash uint8, features fp32 [C, E], layout): the forward in fp32 with the device's rounding points."""
    g = geometry(c.tower)
    sd = state_dict(c.tower)
    L, H, layers = live_rows(c), g.transformer_heads, g.transformer_layers
    lay = StashLayout(c.C, L, g.transformer_width, layers)
    xs, qkvs, hs = [embed(c, inp)], [], []
    for i in range(layers):
        qkvs.append(emu_qkv(sd, i, xs[-1]))
        xs.append(emu_x_mid(sd, i, qkvs[-1], xs[-1], c.C, L, H))
        hs.append(emu_h(sd, i, xs[-1], xs[-2]))
        xs.append(emu_x_out(sd, i, hs[-1], xs[-1], xs[-2]))
    idx = eot_rows(c, inp)
    return lay.pack(xs, qkvs, hs, idx), emu_features(sd, xs[-1], idx), lay


# ------------------------------------------------------------------------------------------------------------------ the two backwards
class StashView:
    """What the backwards read of a stash: x(k), qkv(i), h(i), idx() and the sizes."""

    def __init__(self, stash, lay):
        self.stash, self.lay = stash, lay
        self.C, self.L, self.M, self.D, self.layers = lay.C, lay.L, lay.M, lay.D, lay.layers

    def x(self, k):
        return self.lay.x(self.stash, k)

    def qkv(self, i):
        return self.lay.qkv(self.stash, i)

    def h(self, i):
        return self.lay.h(self.stash, i)

    def idx(self):
        return self.lay.idx(self.stash).long()


class Stash64(StashView):
    """The same of an unrounded float64 forward (coopfit_ref.block_forward) from x_in(0) [C L, D]: no device format holds it."""

    def __init__(self, tower, x0, idx, C, L):
        sd = state_dict(tower)
        g = geometry(tower)
        self.C, self.L, self.M, self.D, self.layers = C, L, C * L, g.transformer_width, g.transformer_layers
        self._x, self._qkv, self._h, self._idx = [x0.double()], [], [], idx.long()
        for i in range(self.layers):
            out, st = cref.block_forward(self._x[-1], _w(sd, i), C, L, g.transformer_heads)
            self._x += [st["x_mid"], out]
            self._qkv.append(st["qkv"])
            self._h.append(st["h"])

    def x(self, k):
        return self._x[k]

    def qkv(self, i):
        return self._qkv[i]

    def h(self, i):
        return self._h[i]

    def idx(self):
        return self._idx


def tail64(tower, st, d_feat):
    """ln_final's backward of d_feat [C, E] (float64) text_projection^T on the EOT rows -> (rows [C, D], the row indices)."""
    sd = state_dict(tower)
    idx = st.idx()
    x = st.x(2 * st.layers).double()[idx]
    return cref.ln_backward(x, sd["ln_final.weight"].double(), d_feat @ sd["text_projection"].double().t()), idx


def backward64(tower, st, d_out):
    """The gradient stream g [C L, D] float64 of the stash's forward for the upstream d_out [C, E]: coopfit_ref.block_backward chained
    over the layers, behind the tail."""
    sd = state_dict(tower)
    H = geometry(tower).transformer_heads
    rows, idx = tail64(tower, st, d_out.double())
    g = torch.zeros(st.M, st.D, dtype=torch.float64)
    g[idx] = rows
    for i in reversed(range(st.layers)):
        s64 = {"x_in": st.x(2 * i).double(), "x_mid": st.x(2 * i + 1).double(), "qkv": st.qkv(i).double(), "h": st.h(i).double()}
        g = cref.block_backward(g, s64, _w(sd, i), st.C, st.L, H)
    return g


def _attention_backward_emu(qkv, d_att, N, L, H, hi, lo):
    """Scores and softmax in ``hi``, P and dS rounded to ``lo`` in front of their products, accumulation in ``hi``, one rounding of dqkv."""
    D = 64 * H
    r = lambda t: t.to(lo).to(hi)  # noqa: E731
    q, k, v = (cref.split_heads(t, N, L, H) for t in qkv.to(hi).reshape(N * L, 3 * D).split(D, dim=-1))
    do = cref.split_heads(d_att.to(hi), N, L, H)
    p = cref.attention_probs(q, k)
    dv = r(p).transpose(-1, -2) @ do
    dp = do @ v.transpose(-1, -2)
    ds = r(p * (dp - (dp * p).sum(-1, keepdim=True)))
    dq = ds @ k / 8.0
    dk = ds.transpose(-1, -2) @ q / 8.0
    return r(torch.cat([t.transpose(1, 2).reshape(N * L, D) for t in (dq, dk, dv)], dim=-1))


def emulate_backward(tower, st, d_out, hi=F32, lo=F16):
    """g [C L, D] of dtype ``hi``: clipmi_text_encoder_backward's steps (include/clipmi.h) in ``hi`` with a rounding to ``lo`` wherever the
    device writes fp16: dfeat16, g16, d_a, d_h, d_att, dqkv, and P and dS inside the attention backward.  hi = lo = float64 is the same
    sequence of steps without any rounding (tests/test_towertrain_cpu.py holds it against autograd)."""
    sd = state_dict(tower)
    H = geometry(tower).transformer_heads
    r = lambda t: t.to(lo).to(hi)  # noqa: E731
    idx = st.idx()
    dxf = r(d_out.to(hi)) @ r(sd["text_projection"].to(hi)).t()
    g = torch.zeros(st.M, st.D, dtype=hi)
    g[idx] = cref.ln_backward(st.x(2 * st.layers).to(hi)[idx], sd["ln_final.weight"].to(hi), dxf)
    for i in reversed(range(st.layers)):
        w = _w(sd, i, hi)
        d_a = r(r(g) @ w["mlp.c_proj.weight"])
        d_h = r(cref.quickgelu_backward(st.h(i).to(hi), d_a))
        g = g + cref.ln_backward(st.x(2 * i + 1).to(hi), w["ln_2.weight"], d_h @ w["mlp.c_fc.weight"])
        d_att = r(r(g) @ w["attn.out_proj.weight"])
        dqkv = _attention_backward_emu(st.qkv(i), d_att, st.C, st.L, H, hi, lo)
        g = g + cref.ln_backward(st.x(2 * i).to(hi), w["ln_1.weight"], dqkv @ w["attn.in_proj_weight"])
    return g


# ----------------------------------------------------------------------------------------------------------- row sets and error measure
def row_sets(c, inp):
    """per prompt {"live": rows 0 .. eot, "plain": row 0 and rows n_ctx + 1 .. eot (no context row)}: index tensors into the L rows.  Rows
    behind the EOT carry no gradient (they are asserted to be exactly zero) and are in neither set."""
    out = []
    for p in range(c.C):
        e = int(inp["eot"][p])
        live = torch.arange(0, e + 1)
        out.append({"live": live, "plain": live[(live == 0) | (live > c.n_ctx)]})
    return out


def prompt_errors(g, want, c, inp):
    """{"live": [C], "plain": [C]}: per prompt, the relative Frobenius error of g against want over the row set."""
    L = live_rows(c)
    g, want = g.double().reshape(c.C, L, -1), want.reshape(c.C, L, -1)
    out = {"live": [], "plain": []}
    for p, sets in enumerate(row_sets(c, inp)):
        for k, rows in sets.items():
            out[k].append(float((g[p, rows] - want[p, rows]).norm() / want[p, rows].norm()))
    return out


def tail_tolerance(tower, st, d_out):
    """(value, tol) [C, D] of the tail alone: ln_backward(x_last[eot], gamma, half(d_out) @ half(proj)^T).  The product is accumulated
    in fp32 over E (gamma_k(E) on absolute values); LayerNorm's backward is linear in its upstream, so that error passes through its
    formula on absolute values; on top the LayerNorm-backward bound of tests/test_gpu_text_backward.py (32 u32 on the terms of dX, 2 u32
    on the accumulated value)."""
    sd = state_dict(tower)
    d16, P = d_out.float().half().double(), sd["text_projection"].half().double()
    val, idx = tail64(tower, st, d16)
    gamma = sd["ln_final.weight"].double()
    x = st.x(2 * st.layers).double()[idx]
    rstd = torch.rsqrt(x.var(-1, unbiased=False, keepdim=True) + EPS)
    xhat = (x - x.mean(-1, keepdim=True)) * rstd
    dy = d16 @ P.t()
    dt = gamma_k(P.shape[1]) * (d16.abs() @ P.abs().t()) * gamma.abs()
    through = rstd * (dt + dt.mean(-1, keepdim=True) + xhat.abs() * (dt * xhat.abs()).mean(-1, keepdim=True))
    t = (dy * gamma).abs().amax(-1, keepdim=True)
    tol = through + 32 * U32 * (rstd * t * (2 + xhat.abs().amax(-1, keepdim=True))) + 2 * U32 * val.abs()
    return val, tol, idx


# ------------------------------------------------------------------------------------------------------------------ operand statistics
def half_bits(t16):
    return t16.contiguous().view(torch.int16).to(torch.int32) & 0xFFFF


def operand_counts(t16):
    """(elements, zeros, subnormals, largest magnitude bits; 0x7fff for a NaN) of an fp16 tensor, as include/clipmi.h defines them."""
    a = half_bits(t16) & 0x7FFF
    mx = 0x7FFF if bool((a > 0x7C00).any()) else int(a.max())
    return t16.numel(), int((a == 0).sum()), int(((a != 0) & (a < 0x0400)).sum()), mx


def passthrough_stats(d_out, d_embed, layers, M, D):
    """The four words after ONE backward on a pass-through tower: the cast of d_out, half(d_embed) twice per layer (the stream never
    changes behind the tail), and all-zero c_fc (4 D) and qkv (3 D) gradients."""
    n0, z0, s0, m0 = operand_counts(d_out.float().half())
    n1, z1, s1, m1 = operand_counts(d_embed.float().half())
    return [n0 + 9 * layers * M * D, z0 + layers * (2 * z1 + 7 * M * D), s0 + 2 * layers * s1, max(m0, m1)]


def special_d_out(C, E, seed=0):
    """d_out whose fp16 cast holds +0, -0, the smallest subnormal, the largest subnormal, the smallest normal and 65504."""
    d = 1e-3 * torch.randn(C, E, generator=torch.Generator().manual_seed(700 + seed))
    d[0, :6] = torch.tensor([0.0, -0.0, 2.0 ** -24, 2.0 ** -14 - 2.0 ** -24, 2.0 ** -14, 65504.0])
    return d
