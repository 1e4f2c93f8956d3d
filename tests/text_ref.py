"""Plain references of the text tower's plumbing kernels (csrc/elementwise.hip: embed_kernel, eot_kernel, rows_from_eot_kernel, add_pos_kernel,
rows_out_kernel, cast_kernel, cast16_kernel, overwrite_kernel, row_stats_kernel) as clipmi_encode_text, clipmi_text_encoder and
clipmi_text_blocks (csrc/capi.hip) reach them -- the oracle of tests/test_text_ref_cpu.py and tests/test_gpu_text_ops.py.

Pass-through blocks.  The kernels have no entry point of their own.  They are isolated by a state dict in which attn.out_proj and mlp.c_proj
(weight and bias) of every text block are zero: both residual GEMMs of a block then add exactly zero (x + 0 = x in the fp32 stream, in the
fp16 stream and inside the K loop of the row-range kernel), while every launch of the block still runs.  What leaves the tower is what the
plumbing kernels put there:

* clipmi_text_blocks: y[c, l] = cast(x[c, l]) for l < L (fp32 stream) or cast(fp16(x[c, l])) (fp16 stream: row_stats_kernel's fp16 copy IS the
  stream), zero behind L; with a hook rows 1..n_ctx are the last applied deep prompt, deep[n_deep - 1].  Bit-exact (values: -0 == +0).
* clipmi_encode_text / clipmi_text_encoder: the feature of prompt c is ln_final(row) @ text_projection on the single row e = eot[c], with
  row = table[clamp(id[c, e])] + pos[e] (encode_text), prompt[c, e] + pos[e] (text_encoder), or the deep prompt row when e lies in 1..n_ctx.
  The sum is ONE IEEE fp32 addition (one answer everywhere); in the fp16 stream the row is then rounded to fp16 once.

Tolerance of a feature (none measured).  ln_final writes fp16: front_ref.layer_norm_rows / tol_ln (its derivation: tests/front_ref.py).  The
projection multiplies those fp16 numbers with the fp16 weights W (products exact in fp32) and accumulates K = D of them in fp32
(front_ref.gamma_k: every addition allowed one whole ulp), the output is the fp32 accumulator:
    |got - y W^T| <= sum_k tol_ln(y)_k |W_ek| + gamma_k(D) sum_k |y_k W_ek|          (y: the float64 LayerNorm row).

Embeddings.  Every row of the token table and of the positional embedding has its own large mean (1 + 0.03 r, 0.5 + 0.02 l; prompts 1.5 and
more) and a spread of 0.02, as token embeddings have: LayerNorm removes the mean, so a detour of the row through fp16 (up to half an fp16 ulp of
the MEAN, 2^-10 for a mean between 2 and 4) shows against the SPREAD -- 3 % of an output of order one, 70 times the output's own fp16
rounding -- while the random part tells every token row and every position apart.  All values are fp32 numbers that fp16 does not hold.

Case 6 (live_*): the statistics row_stats_kernel writes for overwritten rows are the one thing pass-through blocks cannot see (the in-projection
that reads them is multiplied by zero).  A live two-layer tower of width 512 with deep prompts of mean 2 against token rows of 0.02 does.
"""
from __future__ import annotations

import collections
import functools

import numpy as np
import torch

import front_ref
from clip_calibration_amd import synthetic as syn
from front_ref import IN_SENTINEL, _gen

F16, F32 = torch.float16, torch.float32
STREAM_F32, STREAM_F16 = 1, 2                  # CLIPMI_CALL_STREAM_F32 / _F16 (include/clipmi.h)
VOCAB = 97
ID_SENTINEL = -(2 ** 62)                       # an id behind the row bound: never the maximum of its prompt, so it must not matter
EPS = 1e-5

Tower = collections.namedtuple("Tower", "width ctx layers embed")
# width 320: D / 4 = 80, a 256-thread block straddles rows and a 64-lane group is partly filled; width 512: two statistics partials
TOWERS = {"w64": Tower(64, 77, 1, 16), "w128": Tower(128, 9, 3, 64), "w320": Tower(320, 77, 3, 16), "w512": Tower(512, 77, 1, 64),
          "w512x3": Tower(512, 9, 3, 16)}


def geometry(t: Tower) -> syn.ClipGeometry:
    """tiny's vision tower (unused), the text tower of ``t``."""
    return syn.ClipGeometry(t.embed, 64, 2, 128, 16, t.ctx, VOCAB, t.width, t.width // 64, t.layers)


PASS_THROUGH = ("attn.out_proj.weight", "attn.out_proj.bias", "mlp.c_proj.weight", "mlp.c_proj.bias")


@functools.lru_cache(maxsize=None)
def state_dict(name: str):
    """Pass-through state dict of TOWERS[name] (module docstring).  Cached: callers copy the dict, never edit its tensors."""
    t = TOWERS[name]
    sd = syn.synthetic_state_dict(geometry(t), seed=11 + sorted(TOWERS).index(name))
    for i in range(t.layers):
        for k in PASS_THROUGH:
            sd[f"transformer.resblocks.{i}.{k}"].zero_()
    g = _gen(t.width, t.ctx, t.layers, t.embed)

    def noise(n):                                        # spread 0.02 around a mean of zero, row by row
        r = torch.randn(n, t.width, generator=g)
        return 0.02 * (r - r.mean(dim=1, keepdim=True))

    sd["token_embedding.weight"] = (1.0 + 0.03 * torch.arange(VOCAB))[:, None] + noise(VOCAB)
    sd["positional_embedding"] = (0.5 + 0.02 * torch.arange(t.ctx))[:, None] + noise(t.ctx)
    return sd


def live_rows(ctx, seq_rows):
    """Token rows per prompt the tower computes (include/clipmi.h: seq_rows <= 0 or >= L is the whole context)."""
    return seq_rows if 0 < seq_rows < ctx else ctx


def deep_prompts(t: Tower, n_ctx, seed):
    """fp32 [layers, n_ctx, D]: layer k, row j has mean 2 (k + 1) + 0.5 j and spread 0.25 -- a code per layer and row; one layer more than any hook
    may apply, so that the neighbour of every layer exists.  Not fp16-representable: the fp32 stream must hand them on unrounded."""
    g = _gen(t.width, n_ctx, seed, 77)
    k, j = torch.arange(t.layers)[:, None, None], torch.arange(n_ctx)[None, :, None]
    return (2.0 * (k + 1) + 0.5 * j + 0.25 * torch.randn(t.layers, n_ctx, t.width, generator=g)).float()


# ------------------------------------------------------------------------------------------------------------------ clipmi_text_blocks
# hook = (n_ctx, n_deep) or None
BlocksCase = collections.namedtuple("BlocksCase", "tower C seq_rows dtype stream fold hook")


def _blocks_cases():
    c = []
    # every row (cast_kernel / cast16_kernel, both output types) and a row bound (the four rows_out_kernel instantiations), per width
    for tower, C, rows in (("w64", 3, 30), ("w128", 37, 7), ("w320", 3, 66), ("w512", 1, 5), ("w512x3", 37, 6)):
        for dt in (F16, F32):
            for stream in (STREAM_F32, STREAM_F16):
                c.append(BlocksCase(tower, C, 0, dt, stream, 1, None))
                c.append(BlocksCase(tower, C, rows, dt, stream, 1, None))
    # seq_rows: 0 and the bounds above; the context itself, beyond it, negative, one row, no multiple of 4, one short of the context
    for rows in (77, 100, -3, 1, 31, 76):
        c.append(BlocksCase("w320", 3, rows, F32, STREAM_F32, 1, None))
        c.append(BlocksCase("w64", 37, rows, F16, STREAM_F16, 1, None))
    # separate LayerNorm kernels (fp32 stream only)
    for tower, C, rows in (("w64", 37, 0), ("w128", 3, 5), ("w320", 1, 66), ("w512", 3, 9)):
        for dt in (F16, F32):
            c.append(BlocksCase(tower, C, rows, dt, STREAM_F32, 0, None))
    # the hook on the three-layer towers
    for tower, C, rows in (("w128", 3, 0), ("w320", 3, 9), ("w512x3", 37, 7)):
        for n_ctx in (1, 2, 4):
            for n_deep in (0, 1, 2):
                for dt, stream, fold in ((F32, STREAM_F32, 1), (F16, STREAM_F16, 1), (F32, STREAM_F16, 1), (F16, STREAM_F32, 0)):
                    if (n_ctx + n_deep + (dt == F16) + stream) % 2 == 0 or n_ctx == 2:      # half of the grid, n_ctx = 2 in full
                        c.append(BlocksCase(tower, C, rows, dt, stream, fold, (n_ctx, n_deep)))
    return c


BLOCKS_CASES = _blocks_cases()


def _dt(d):
    return "h" if d == F16 else "f"


def blocks_case_id(c):
    hook = "" if c.hook is None else f"-ctx{c.hook[0]}deep{c.hook[1]}"
    return f"{c.tower}-C{c.C}-r{c.seq_rows}-{_dt(c.dtype)}-s{'16' if c.stream == STREAM_F16 else '32'}-fold{c.fold}{hook}"


def tie_values(n):
    """fp32 numbers a hair above an fp16 rounding tie, 1 + (2 j + 1) 2^-11 + 2^-20: one rounding goes up; a rounding to 13 bits first lands ON the
    tie and the second, to nearest even, goes down for even j."""
    j = torch.arange(n, dtype=torch.float64) % 512
    v = 1.0 + (2.0 * j + 1.0) * 2.0 ** -11 + 2.0 ** -20
    v[1::3] *= -1.0
    return v.to(F32)


def blocks_input(c):
    """-> dict(x [C, ctx, D] of c.dtype, deep fp32 [layers, n_ctx, D] or None).  Rows at or behind the bound hold IN_SENTINEL; every seventh
    element is a tie_values number, and there are zeros of either sign."""
    t = TOWERS[c.tower]
    g = _gen(t.width, t.ctx, c.C, c.seq_rows if c.seq_rows > 0 else 1000 - c.seq_rows, c.dtype == F16, c.stream, c.fold)
    x = torch.randn(c.C, t.ctx, t.width, generator=g)
    flat = x.reshape(-1)
    flat[::7] = tie_values(flat[::7].numel())
    flat[3::11] = 0.0
    flat[5::22] = -0.0
    x = x.to(c.dtype)
    L = live_rows(t.ctx, c.seq_rows)
    x[:, L:] = IN_SENTINEL[c.dtype]
    deep = deep_prompts(t, c.hook[0], 5) if c.hook else None
    return dict(x=x, deep=deep)


def round_twice(v):
    """Mutant: fp32 -> 13 significant bits -> fp16 (round to nearest even both times)."""
    a = v.detach().float().numpy().astype(np.float32)
    m, e = np.frexp(a.astype(np.float64))
    a13 = np.ldexp(np.rint(m * 2.0 ** 13), e - 13)                # rint: ties to even
    return torch.from_numpy(a13.astype(np.float32)).half()


def blocks_expected(c, inp, deep_shift=0, double_round=False):
    """-> y [C, ctx, D] of c.dtype, exact.  Mutants: deep_shift (the deep prompt of the neighbouring layer), double_round (every fp32 -> fp16
    conversion rounds twice)."""
    t = TOWERS[c.tower]
    L = live_rows(t.ctx, c.seq_rows)
    v = inp["x"][:, :L].float().clone()
    if c.hook and c.hook[1] > 0:
        n_ctx, n_deep = c.hook
        k = n_deep - 1 + deep_shift
        v[:, 1:1 + n_ctx] = inp["deep"][k if 0 <= k < t.layers else n_deep]
    half = round_twice if double_round else (lambda a: a.half())
    if c.stream == STREAM_F16:
        v = half(v).float()
    y = torch.zeros(c.C, t.ctx, t.width, dtype=c.dtype)
    y[:, :L] = half(v) if c.dtype == F16 else v
    return y


# ------------------------------------------------------------------------------------------- clipmi_encode_text / clipmi_text_encoder
# entry "ids" (encode_text) | "prompts" (text_encoder); dtype: of the prompts; pattern: how the ids / EOT indices are made (enc_input)
EncCase = collections.namedtuple("EncCase", "entry tower C seq_rows dtype stream fold hook pattern")


def _enc_cases():
    c = []
    # 1. address map: three calls of 37 prompts put every vocabulary row on an EOT position once; every width, both streams, fold off
    for tower in TOWERS:
        for v in range(3):
            c.append(EncCase("ids", tower, 37, 0, None, STREAM_F32 if (v + len(tower)) % 2 else STREAM_F16, 1, None, f"addr{v}"))
    c.append(EncCase("ids", "w320", 37, 0, None, STREAM_F32, 0, None, "addr1"))
    c.append(EncCase("ids", "w512", 37, 0, None, STREAM_F32, 0, None, "addr2"))
    # 2. EOT selection: ties, a constant row, ids outside the vocabulary
    for tower, stream in (("w64", STREAM_F32), ("w320", STREAM_F16), ("w128", STREAM_F32)):
        c.append(EncCase("ids", tower, 37, 0, None, stream, 1, None, "ties"))
    # 4. seq_rows: tightest bound (the pattern always puts an EOT on the last live row), no multiple of 4, the context, beyond, negative
    for rows in (66, 30, 7, 1, 77, 100, -3):
        c.append(EncCase("ids", "w320", 3, rows, None, STREAM_F32, 1, None, "addr0"))
        c.append(EncCase("prompts", "w64", 37, rows, F32 if rows % 2 else F16, STREAM_F16 if rows % 3 else STREAM_F32, 1, None, "eot"))
    c.append(EncCase("ids", "w512", 1, 5, None, STREAM_F16, 1, None, "addr1"))
    c.append(EncCase("ids", "w512x3", 37, 6, None, STREAM_F32, 0, None, "ties"))
    # text_encoder, every width, both input types
    for tower, C in (("w64", 3), ("w128", 37), ("w320", 1), ("w512", 3), ("w512x3", 3)):
        for dt in (F16, F32):
            c.append(EncCase("prompts", tower, C, 0, dt, STREAM_F32 if dt == F16 else STREAM_F16, 1, None, "eot"))
    c.append(EncCase("prompts", "w512", 37, 66, F32, STREAM_F32, 0, None, "eot"))
    # 3. the caller's eot outside [0, L - 1]
    for tower, rows, dt in (("w64", 0, F32), ("w64", 30, F16), ("w128", 5, F32), ("w320", 66, F16)):
        c.append(EncCase("prompts", tower, 37, rows, dt, STREAM_F32, 1, None, "clamp"))
    # 5. hook: an EOT inside 1..n_ctx sees the overwrite
    for tower, C, rows in (("w128", 3, 0), ("w320", 37, 9), ("w512x3", 3, 7)):
        for n_ctx in (1, 2, 4):
            for n_deep in (0, 1, 2):
                stream = STREAM_F16 if (n_ctx + n_deep) % 2 else STREAM_F32
                c.append(EncCase("prompts", tower, C, rows, F32 if n_deep else F16, stream, 1, (n_ctx, n_deep), "eot"))
    c.append(EncCase("prompts", "w320", 3, 9, F32, STREAM_F32, 0, (2, 2), "eot"))
    return c


ENC_CASES = _enc_cases()


def enc_case_id(c):
    hook = "" if c.hook is None else f"-ctx{c.hook[0]}deep{c.hook[1]}"
    return (f"{c.entry}-{c.tower}-C{c.C}-r{c.seq_rows}-{'' if c.dtype is None else _dt(c.dtype) + '-'}s{'16' if c.stream == STREAM_F16 else '32'}"
            f"-fold{c.fold}{hook}-{c.pattern}")


def eot_positions(ctx, L, C):
    """EOT index of every prompt: 0, 63 and 64 (eot_kernel's lane wrap), the last live row, the last row of the context, rows 1 and 2 (inside a
    hook's tokens) and others, those below L, in turn."""
    cand = [L - 1, 0, 63, 64, ctx - 1, 1, 2, L // 2, 5, 62, 65, 33, 3]
    pos = [p for i, p in enumerate(cand) if 0 <= p < L and p not in cand[:i]]
    return [pos[c % len(pos)] for c in range(C)]


def _id_row(ctx, L, e, tok, g):
    """A prompt whose only maximum, ``tok``, sits on index e: the other live ids are drawn from [tok - VOCAB, tok - 1] (negative ones included,
    which the table lookup clamps to row 0); ids behind the bound are ID_SENTINEL."""
    row = tok - 1 - torch.randint(0, VOCAB, (ctx,), generator=g)
    row[e] = tok
    row[L:] = ID_SENTINEL
    return row


def _tie_rows(ctx, L):
    """[(ids row, what)]: the maximum two and three times -- in the same lane of different 64-id strides, in different lanes of one stride, across
    strides -- a constant row, ids at and beyond the vocabulary, ids beyond 2^32, a row of negative ids."""
    rows = []

    def make(at, top, base=7, what=""):
        r = torch.full((ctx,), base, dtype=torch.int64)
        for p in at:
            if p < L:
                r[p] = top
        r[L:] = ID_SENTINEL
        rows.append((r, what))

    make((5, 69), 50, what="twice, same lane, strides 0 and 1")
    make((5, 9), 50, what="twice, one stride")
    make((70, 67), 50, what="twice, stride 1")
    make((66, 3), 50, what="twice, the later lane first")
    make((2, 66, 70), 60, what="three times, across strides")
    make((4, 5, 6), 60, what="three times, neighbours")
    make((64, 65, 76), 60, what="three times, stride 1")
    make((L - 1, L - 2), 96, what="twice, the last live rows")
    make((), 7, what="constant")
    make((), 0, base=0, what="constant zero")
    make((3,), VOCAB, what="id == vocab")
    make((6, 8), 1000, what="id beyond the vocabulary, twice")
    make((4,), 2 ** 40 + 3, base=2 ** 40 + 1, what="ids beyond 2^32: a 32-bit compare sees 3 and 1, a 32-bit table index wraps")
    make((2,), -1, base=-5, what="negative ids")
    make((1,), -2 ** 33, base=-2 ** 33 - 1, what="ids below -2^32")
    return rows


def enc_input(c):
    """-> dict(ids int64 [C, ctx] | prompts [C, ctx, D] of c.dtype and eot int32 [C], deep or None).  Prompt rows at or behind the bound hold
    IN_SENTINEL, ids there ID_SENTINEL."""
    t = TOWERS[c.tower]
    L = live_rows(t.ctx, c.seq_rows)
    g = _gen(t.width, t.ctx, c.C, c.seq_rows if c.seq_rows > 0 else 1000 - c.seq_rows, c.entry == "ids", len(c.pattern), ord(c.pattern[-1]))
    pos = eot_positions(t.ctx, L, c.C)
    out = dict(deep=deep_prompts(t, c.hook[0], 9) if c.hook else None)
    if c.entry == "ids":
        shift = 37 * int(c.pattern[-1]) if c.pattern.startswith("addr") else 11
        ids = torch.stack([_id_row(t.ctx, L, pos[i], (i + shift) % VOCAB, g) for i in range(c.C)])
        if c.pattern == "ties":
            for i, (r, _) in enumerate(_tie_rows(t.ctx, L)):
                ids[i] = r
        out["ids"] = ids
        return out
    k = (torch.arange(c.C)[:, None] * t.ctx + torch.arange(t.ctx)[None, :]) % 311
    p = (1.5 + 0.01 * k)[:, :, None] + 0.02 * torch.randn(c.C, t.ctx, t.width, generator=g)
    p = p.to(c.dtype)
    p[:, L:] = IN_SENTINEL[c.dtype]
    eot = torch.tensor(pos, dtype=torch.int32)
    if c.pattern == "clamp":
        outside = [-1, -1000, L, L + 5, t.ctx, t.ctx + 1, 2 ** 30, -2 ** 31, 2 ** 31 - 1]
        for i, v in enumerate(outside):
            eot[(3 * i) % c.C] = v
    out.update(prompts=p, eot=eot)
    return out


def _clamp(v, lo, hi, off):
    """clamp into [lo, hi]; mutant ``off``: the bounds that replace an outside value are one step inside."""
    if v < lo:
        return lo + off
    if v > hi:
        return hi - off
    return v


def enc_rows(c, inp, pos_shift=0, last_max=False, clamp_off=0, deep_shift=0):
    """-> (rows fp32 [C, D], plan): the one row of every prompt that reaches ln_final, as the stream holds it (one fp32 addition; fp16 stream:
    rounded to fp16 once), and plan = [(e, source)] for the report.  Mutants: pos_shift (the positional row of a neighbouring token), last_max
    (ties go to the last maximum), clamp_off (a clamp that is off by one), deep_shift (the neighbouring layer's deep prompt)."""
    t = TOWERS[c.tower]
    sd = state_dict(c.tower)
    table, pos = sd["token_embedding.weight"], sd["positional_embedding"]
    L = live_rows(t.ctx, c.seq_rows)
    rows, plan = [], []
    for i in range(c.C):
        if c.entry == "ids":
            ids = inp["ids"][i].numpy()
            e = int(np.argmax(ids))                                           # the first maximum, over the whole context, of the raw ids
            if last_max:
                e = int(len(ids) - 1 - np.argmax(ids[::-1]))
            e = _clamp(e, 0, L - 1, 0)
            tok = _clamp(int(ids[e]), 0, VOCAB - 1, clamp_off)
            src, what = table[tok], f"table[{tok}]"
        else:
            e = _clamp(int(inp["eot"][i]), 0, L - 1, clamp_off if L > 1 else 0)
            src, what = inp["prompts"][i, e].float(), f"prompt[{i}, {e}]"
        pe = e + pos_shift if 0 <= e + pos_shift < t.ctx else e - pos_shift
        row = src + pos[pe]                                                   # torch fp32 addition: IEEE
        if c.hook and c.hook[1] > 0 and 1 <= e <= c.hook[0]:
            k = c.hook[1] - 1 + deep_shift
            k = k if 0 <= k < t.layers else c.hook[1]
            row, what = inp["deep"][k, e - 1].clone(), f"deep[{k}, {e - 1}]"
        rows.append(row)
        plan.append((e, what, pe))
    rows = torch.stack(rows).float()
    if c.stream == STREAM_F16:
        rows = rows.half().float()
    return rows, plan


def enc_features(c, rows):
    """ln_final + text_projection of the rows in float64 -> (value, tol) [C, E] (module docstring)."""
    sd = state_dict(c.tower)
    D = TOWERS[c.tower].width
    val, bound = front_ref.layer_norm_rows(rows, sd["ln_final.weight"], sd["ln_final.bias"], EPS)
    tol_y = front_ref.tol_ln(val, bound, F16)
    W = sd["text_projection"].half().double().t()                            # [E, D], the fp16 operand
    feat = val @ W.t()
    tol = tol_y @ W.abs().t() + front_ref.gamma_k(D) * (val.abs() @ W.abs().t())
    return feat, tol


# ------------------------------------------------------------------------- case 6: the statistics of overwritten rows, on a live tower
LIVE_TOWER = Tower(512, 77, 2, 64)
LIVE_C, LIVE_ROWS, LIVE_N_CTX = 3, 16, 2
LIVE_OFFSET = 2.0                                # mean of the deep prompt rows; token rows are about 0.02
LIVE_EOT = (5, 9, 15)
STALE_COLS = slice(256, 512)                     # the second 256-column partial of a 512-wide row


@functools.lru_cache(maxsize=None)
def live_input():
    """-> dict(sd, ids [3, 77], prompts fp32 [3, 77, 512] (token embeddings, no positional embedding), eot, deep fp32 [1, 2, 512])."""
    sd = syn.synthetic_state_dict(geometry(LIVE_TOWER), seed=23)
    g = _gen(512, 77, 6)
    ids = torch.zeros(LIVE_C, LIVE_TOWER.ctx, dtype=torch.int64)
    for i, e in enumerate(LIVE_EOT):
        ids[i, :e] = torch.randint(1, VOCAB - 2, (e,), generator=g)
        ids[i, 0], ids[i, e] = VOCAB - 2, VOCAB - 1
    prompts = sd["token_embedding.weight"][ids].float()
    deep = (LIVE_OFFSET + 0.02 * torch.randn(1, LIVE_N_CTX, 512, generator=g)).half().float()      # as the callers hand them over
    return dict(sd=sd, ids=ids, prompts=prompts, eot=torch.tensor(LIVE_EOT, dtype=torch.int32), deep=deep)


def live_reference(stale=False):
    """The hooked tower with the oracle's own blocks (oracle/clip_oracle.py, fp32) -> features [3, 64].  stale: the mutant -- ln_1 of block 1 takes,
    for the overwritten rows, (sum, sum of squares) to which the second partial of the rows they replaced (block 0's output, STALE_COLS) is
    added; mean and variance from the sums as the folded GEMM forms them (E[x^2] - mean^2 in double, clamped at 0)."""
    from oracle import clip_oracle as orc
    inp = live_input()
    sd = inp["sd"]
    x = inp["prompts"] + sd["positional_embedding"].float()
    mask = orc.causal_mask(x.shape[1])
    heads = LIVE_TOWER.width // 64
    x = orc.residual_block(x, sd, "transformer.resblocks.0.", heads, mask)
    old = x[:, 1:1 + LIVE_N_CTX].double()
    x = torch.cat([x[:, :1], inp["deep"][0].expand(LIVE_C, -1, -1), x[:, 1 + LIVE_N_CTX:]], dim=1)
    p = "transformer.resblocks.1."
    w = lambda k: sd[p + k].float()  # noqa: E731
    h = orc.layer_norm(x, sd[p + "ln_1.weight"], sd[p + "ln_1.bias"])
    if stale:
        new = x[:, 1:1 + LIVE_N_CTX].double()
        s = new.sum(-1, keepdim=True) + old[..., STALE_COLS].sum(-1, keepdim=True)
        q = (new * new).sum(-1, keepdim=True) + (old[..., STALE_COLS] ** 2).sum(-1, keepdim=True)
        mean = s / 512
        var = (q / 512 - mean * mean).clamp_min(0.0)
        h[:, 1:1 + LIVE_N_CTX] = ((new - mean) / torch.sqrt(var + EPS) * w("ln_1.weight").double() + w("ln_1.bias").double()).float()
    x = x + orc.multi_head_attention(h, w("attn.in_proj_weight"), w("attn.in_proj_bias"), w("attn.out_proj.weight"), w("attn.out_proj.bias"), heads, mask)
    h = orc.layer_norm(x, sd[p + "ln_2.weight"], sd[p + "ln_2.bias"])
    x = x + (orc.quick_gelu(h @ w("mlp.c_fc.weight").t() + w("mlp.c_fc.bias")) @ w("mlp.c_proj.weight").t() + w("mlp.c_proj.bias"))
    x = orc.layer_norm(x, sd["ln_final.weight"], sd["ln_final.bias"])
    return x[torch.arange(LIVE_C), inp["ids"].argmax(-1)] @ sd["text_projection"].float()


LIVE_COS_TOL, LIVE_MAG_TOL, LIVE_FOLD_TOL = 1e-3, 5e-3, 5e-4      # test_gpu_model.py: _feat_close (hooked towers), test_layernorm_fold_path


def cos_table(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    a = a / np.linalg.norm(a, axis=-1, keepdims=True)
    b = b / np.linalg.norm(b, axis=-1, keepdims=True)
    return a @ b.T
