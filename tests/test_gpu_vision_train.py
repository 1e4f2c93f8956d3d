"""The image tower in training mode stage by stage (csrc/vision_backward.hip), as tests/test_gpu_towertrain.py is for the text tower: every
stash slab against float64 evaluated on the device's OWN previous slab, the splice rows exactly, a pass-through tower whose gradient is
exactly predictable, the rows zeroed at a splice, and the stash untouched by the backward.  The stash is read by the byte layout
include/clipmi.h documents.

Tolerances come from the formats, element by element, with the project's factor 2 on top (fast exponential, other summation order):
* a GEMM whose operand a is rounded to fp16 and whose weights are fp16 values: U16 (|a| |W|^T) for the operand's rounding, plus the output's
  own rounding (U16 |want| for an fp16 slab, 2^-23 |want| for an fp32 one) and 2^-20 (|a| |W|^T) for the fp32 accumulation and LayerNorm;
* attention's output: P is rounded to fp16 (U16 per element), the exponential is the fast one (2 ulp of fp32 on the argument, below
  U16) and the output is fp16: 3 U16 (P |v|);   * QuickGELU's output is fp16 of an fp32 evaluation: U16 |a| with the same slack.
U16 = 2^-11, the unit round-off of fp16."""
import numpy as np
import pytest
import torch

import coopfit_ref as cref
import vptfit_ref as ref
from clip_calibration_amd import vptfit
from clip_calibration_amd.model import build_model

pytestmark = pytest.mark.gpu
U16, FACTOR = 2.0 ** -11, 2.0


def align256(n):
    return (n + 255) // 256 * 256


class Stash:
    """The byte layout of clipmi_vision_encoder_train's stash (include/clipmi.h)."""

    def __init__(self, raw, B, L, D, layers, n_ctx):
        self.raw, self.M, self.D, self.layers = raw.cpu().numpy(), B * L, D, layers
        self.xb, self.qb, self.hb = align256(self.M * D * 4), align256(self.M * D * 6), align256(self.M * D * 8)
        self.idx_off = (2 * layers + 1) * self.xb + layers * (self.qb + self.hb)
        self.pr_off = self.idx_off + align256(B * 8)
        self.B, self.n_ctx = B, n_ctx

    def _view(self, off, count, dtype, shape):
        return torch.from_numpy(self.raw[off:off + count * np.dtype(dtype).itemsize].view(dtype).reshape(shape).copy())

    def x(self, k):
        return self._view(k * self.xb, self.M * self.D, np.float32, (self.M, self.D))

    def qkv(self, i):
        return self._view((2 * self.layers + 1) * self.xb + i * self.qb, self.M * 3 * self.D, np.float16, (self.M, 3 * self.D))

    def h(self, i):
        return self._view((2 * self.layers + 1) * self.xb + self.layers * self.qb + i * self.hb, self.M * 4 * self.D, np.float16, (self.M, 4 * self.D))

    def idx(self):
        return self._view(self.idx_off, 2 * self.B, np.int32, (2 * self.B,))

    def prompts(self, depth):
        return self._view(self.pr_off, depth * self.n_ctx * self.D, np.float32, (depth, self.n_ctx, self.D))


def run_case(geom, n_ctx, depth, B, C, edit=None, seed=0):
    c = ref.make_case(geom, n_ctx, depth, B, C, seed=seed)
    if edit:
        edit(c["sd"])
    m = build_model(dict(c["sd"]), {"trainer": "VPT", "vision_depth": depth, "vision_ctx": n_ctx, "language_depth": 0, "language_ctx": 0}).cuda()
    g = ref.geometry(geom)
    t = vptfit._Tower("test", m, depth, n_ctx)
    master = c["prompts"].cuda().contiguous()
    feats = t.forward(c["images"].cuda(), master).cpu()
    torch.cuda.synchronize()
    L = (g.image_resolution // g.vision_patch_size) ** 2 + 1 + n_ctx
    c.update(model=m, tower=t, feats=feats, L=L, L0=L - n_ctx, D=g.vision_width, E=g.embed_dim, layers=g.vision_layers, B=B, depth=depth, n_ctx=n_ctx)
    c["stash"] = Stash(t.stash, B, L, g.vision_width, g.vision_layers, n_ctx)
    return c


def held(name, got, want, tol):
    err = (got.double() - want).abs()
    worst = float((err / tol).max())
    print(f"\nvision-train: {name}: worst error / tolerance {worst:.3f}")
    assert torch.isfinite(got.float()).all() and worst <= 1.0, name


def linear_tol(a, W, want, fp16_out):
    reach = a.abs() @ W.abs().t()
    return FACTOR * (U16 * reach + (U16 if fp16_out else 2.0 ** -23) * want.abs() + 2.0 ** -20 * reach) + 2.0 ** -24


STAGE_CASES = [("tiny", 8, 2, 3, 5), ("tiny3", 1, 2, 2, 4), ("tiny3", 8, 3, 2, 4), ("custom", 8, 2, 1, 3)]


@pytest.mark.parametrize("geom,n_ctx,depth,B,C", STAGE_CASES)
def test_every_slab_from_the_device_previous_slab(geom, n_ctx, depth, B, C):
    c = run_case(geom, n_ctx, depth, B, C)
    st, sd, L, L0, D, H, layers = c["stash"], c["sd"], c["L"], c["L0"], c["D"], c["D"] // 64, c["layers"]
    f64 = torch.float64
    pr = c["prompts"].half().float()
    assert torch.equal(st.prompts(depth), pr), "the stash keeps the masters rounded through fp16"
    idx = st.idx()
    assert idx[:B].tolist() == [b * L for b in range(B)] and idx[B:].tolist() == [0] * B
    # x_in(0): the prompt rows are ln_pre of the rounded shallow prompt, the same in every image
    x0 = st.x(0).reshape(B, L, D)
    want0 = cref.ln_forward(pr[0].double(), sd["visual.ln_pre.weight"].double(), sd["visual.ln_pre.bias"].double())
    for b in range(B):
        held(f"{geom} x_in(0) prompt rows image {b}", x0[b, L0:], want0, FACTOR * 2.0 ** -20 * (want0.abs() + 1.0))
    truth, _ = ref.forward(sd, c["images"], c["prompts"])
    assert ref.rel_fro(c["feats"], truth) <= 5e-3
    for i in range(layers):
        w = ref.vblock_weights(sd, i, f64)
        x_in, x_mid, x_out = st.x(2 * i).double(), st.x(2 * i + 1).double(), st.x(2 * i + 2).double()
        qkv, h = st.qkv(i), st.h(i)
        if 0 < i < depth:
            assert torch.equal(st.x(2 * i).reshape(B, L, D)[:, L0:], pr[i].expand(B, -1, -1)), f"block {i}: the prompt rows are the prompt, exactly"
        ln1 = cref.ln_forward(x_in, w["ln_1.weight"], w["ln_1.bias"])
        want = ln1 @ w["attn.in_proj_weight"].t() + w["attn.in_proj_bias"]
        held(f"{geom} qkv({i})", qkv, want, linear_tol(ln1, w["attn.in_proj_weight"], want, True))
        q, k, v = (cref.split_heads(t, B, L, H) for t in qkv.double().split(D, dim=-1))
        p = ref.attention_probs_full(q, k)
        att = (p @ v).transpose(1, 2).reshape(B * L, D)
        att_tol = 3 * U16 * (p @ v.abs()).transpose(1, 2).reshape(B * L, D)
        want = x_in + att @ w["attn.out_proj.weight"].t() + w["attn.out_proj.bias"]
        tol = FACTOR * (att_tol @ w["attn.out_proj.weight"].abs().t() + 2.0 ** -20 * (att.abs() @ w["attn.out_proj.weight"].abs().t()) + 2.0 ** -23 * want.abs()) + 2.0 ** -24
        held(f"{geom} x_mid({i})", st.x(2 * i + 1), want, tol)
        ln2 = cref.ln_forward(x_mid, w["ln_2.weight"], w["ln_2.bias"])
        want = ln2 @ w["mlp.c_fc.weight"].t() + w["mlp.c_fc.bias"]
        held(f"{geom} h({i})", h, want, linear_tol(ln2, w["mlp.c_fc.weight"], want, True))
        a = cref.quickgelu(h.double())
        want = x_mid + a @ w["mlp.c_proj.weight"].t() + w["mlp.c_proj.bias"]
        got = st.x(2 * i + 2).clone()
        if i + 1 < depth:                       # the slab is block i + 1's input: its prompt rows were overwritten in place
            keep = torch.ones(B, L, dtype=torch.bool)
            keep[:, L0:] = False
            keep = keep.reshape(B * L)
            got, want, a = got[keep], want[keep], a[keep]
        held(f"{geom} x_out({i})", got, want, linear_tol(a, w["mlp.c_proj.weight"], want, False))
    cls = st.x(2 * layers).double().reshape(B, L, D)[:, 0]
    lnp = cref.ln_forward(cls, sd["visual.ln_post.weight"].double(), sd["visual.ln_post.bias"].double())
    want = lnp @ sd["visual.proj"].double()
    held(f"{geom} features", c["feats"], want, linear_tol(lnp, sd["visual.proj"].double().t(), want, False))


def zero(sd, i, *names):
    for n in names:
        sd[f"visual.transformer.resblocks.{i}.{n}"] = torch.zeros_like(sd[f"visual.transformer.resblocks.{i}.{n}"])


def backward(c, seed=0):
    g = torch.Generator().manual_seed(40 + seed)
    d_feats = (torch.randn(c["B"], c["E"], generator=g) * 8.0).cuda()
    before = c["tower"].stash.clone()
    d = c["tower"].backward(d_feats).cpu()
    torch.cuda.synchronize()
    assert torch.equal(c["tower"].stash, before), "the backward wrote the stash"
    return d


def stream(c):
    """The fp32 gradient stream the backward left in the workspace: behind the shared tower workspace (csrc/model.h carve_ws)."""
    M, B, D, E = c["B"] * c["L"], c["B"], c["D"], c["E"]
    off = sum(align256(n) for n in (M * D * 2, M * D * 2, M * D * 8, M * D * 6, M * D * 4, B * D * 2, B * E * 2, B * D * 4))
    raw = c["tower"].ws.cpu().numpy()
    return torch.from_numpy(raw[off:off + M * D * 4].view(np.float32).reshape(B, c["L"], D).copy())


@pytest.mark.parametrize("geom,n_ctx,depth,B", [("tiny", 8, 2, 3), ("tiny3", 1, 3, 2), ("tiny3", 8, 1, 2)])
def test_pass_through_tower(geom, n_ctx, depth, B):
    """Out-projection and c_proj zero in every block: a block returns its input, so every slab repeats x_in(0) but for the spliced rows,
    the class row never sees a prompt and d_prompts is exactly zero; the stream carries ln_post's gradient on the class rows alone."""
    def edit(sd):
        for i in range(ref.n_layers(sd)):
            zero(sd, i, "attn.out_proj.weight", "attn.out_proj.bias", "mlp.c_proj.weight", "mlp.c_proj.bias")
    c = run_case(geom, n_ctx, depth, B, 4, edit)
    st, L0 = c["stash"], c["L0"]
    x0 = st.x(0).reshape(B, c["L"], c["D"])
    pr = c["prompts"].half().float()
    for i in range(c["layers"]):
        want = x0.clone()
        j = min(i, depth - 1)
        if j > 0:
            want[:, L0:] = pr[j]
        assert torch.equal(st.x(2 * i).reshape_as(want), want) and torch.equal(st.x(2 * i + 1).reshape_as(want), want), i
    d = backward(c)
    assert d.shape == (depth, n_ctx, c["D"]) and (d == 0).all()
    g = stream(c)
    assert (g[:, 1:] == 0).all() and (g[:, 0] != 0).any()


@pytest.mark.parametrize("geom,n_ctx,B", [("tiny", 8, 3), ("tiny3", 1, 2)])
def test_rows_zeroed_at_a_splice_stay_zero_below_it(geom, n_ctx, B):
    """depth 2; block 0 keeps its MLP but has a dead attention path (out-projection zero), so its backward is row-local.  The prompt rows'
    gradient is taken out at block 1's splice; below it they are exactly zero in the stream only if BOTH the fp32 stream and its fp16 copy
    were cleared (the copy feeds c_proj's dgrad GEMM first), and then slot 0's gradient is exactly zero while slot 1's is not."""
    c = run_case(geom, n_ctx, 2, B, 4, lambda sd: zero(sd, 0, "attn.out_proj.weight", "attn.out_proj.bias"))
    d = backward(c)
    g = stream(c)
    assert (g[:, c["L0"]:] == 0).all(), "a row zeroed at the splice carries gradient below it"
    assert (g[:, :c["L0"]] != 0).any()
    assert (d[0] == 0).all() and torch.isfinite(d[1]).all() and float(d[1].abs().max()) > 0
    assert torch.equal(backward(c), d)          # the same bits again


@pytest.mark.parametrize("geom,n_ctx,depth,B,C", [STAGE_CASES[0], STAGE_CASES[2]])
def test_backward_from_the_device_stash(geom, n_ctx, depth, B, C):
    """d_prompts against the float64 restatement evaluated on the device's own stash, within FACTOR x an fp32 emulation with the device's
    fp16 rounding points (g16, d_a, d_h, d_att, dqkv, P and dS) of the same stash."""
    c = run_case(geom, n_ctx, depth, B, C)
    st, sd, L, L0, D, H = c["stash"], c["sd"], c["L"], c["L0"], c["D"], c["D"] // 64
    g = torch.Generator().manual_seed(40)
    d_feats = torch.randn(B, c["E"], generator=g) * 8.0
    got = c["tower"].backward(d_feats.cuda()).cpu().double()

    def restate(hi, lo):
        r = (lambda t: t) if lo is None else (lambda t: t.to(lo).to(hi))
        pr = st.prompts(depth).to(hi)
        gs = torch.zeros(B, L, D, dtype=hi)
        cls = st.x(2 * c["layers"]).to(hi).reshape(B, L, D)[:, 0]
        gs[:, 0] = cref.ln_backward(cls, sd["visual.ln_post.weight"].to(hi), r(d_feats.to(hi)) @ sd["visual.proj"].to(hi).t())
        gs = gs.reshape(B * L, D)
        out = torch.zeros(depth, n_ctx, D, dtype=hi)
        for i in range(c["layers"] - 1, -1, -1):
            w = ref.vblock_weights(sd, i, hi)
            d_h = r(cref.quickgelu_backward(st.h(i).to(hi), r(r(gs) @ w["mlp.c_proj.weight"])))
            gs = gs + cref.ln_backward(st.x(2 * i + 1).to(hi), w["ln_2.weight"], d_h @ w["mlp.c_fc.weight"])
            dqkv = ref.attention_backward_full(st.qkv(i).to(hi), r(r(gs) @ w["attn.out_proj.weight"]), B, L, H, lo)
            gs = gs + cref.ln_backward(st.x(2 * i).to(hi), w["ln_1.weight"], dqkv @ w["attn.in_proj_weight"])
            if 1 <= i < depth:
                g3 = gs.reshape(B, L, D).clone()
                out[i] = g3[:, L0:].sum(0)
                g3[:, L0:] = 0
                gs = g3.reshape(B * L, D)
        out[0] = cref.ln_backward(pr[0], sd["visual.ln_pre.weight"].to(hi), gs.reshape(B, L, D)[:, L0:].sum(0))
        return out.double()

    want, emu = restate(torch.float64, None), restate(torch.float32, torch.float16)
    for i in range(depth):
        e_dev, e_emu = ref.rel_fro(got[i], want[i]), ref.rel_fro(emu[i], want[i])
        print(f"\nvision-train: {geom} d_prompts[{i}] device {e_dev:.3e} emulation {e_emu:.3e} ratio {e_dev / e_emu:.2f}")
        assert e_dev <= FACTOR * e_emu
