"""MaPLe's training path without a GPU: tests/maplefit_ref.py's autograd-free float64 restatement -- the text splice and its reduction, the
coupling functions forward and backward, the joint head, the master block's layout -- against torch autograd through the oracle's
``maple_prompt_learner`` + ``text_encoder(deep_prompts=...)`` + ``encode_image(shared_ctx, deep_prompts)``, for every parameter tensor."""
import math

import pytest
import torch

import coopfit_ref as cref
import maplefit_ref as ref
import vptfit_ref as vref
from clip_calibration_amd import synthetic as syn

# The oracle keeps fp32 inside its float64 run (its LayerNorm and its attention softmax are evaluated in fp32, as the reference evaluates
# them).  The restatement is therefore held to it on maplefit_ref's island towers, which restate those two islands operation by operation
# (prodafit_ref's blocks, the splice between them): what is left is float64 rounding, bounded by test_prodafit_cpu.py's 1e-9 for every
# parameter tensor and the loss.  The plain float64 formulas (no islands; what the GPU tests use as their float64 stages) differ from the
# oracle by that fp32 round-off carried through the blocks: test_vptfit_cpu.py's 3e-6 (1e-5 on the loss).
RTOL = 1e-9
PLAIN_TOL, PLAIN_LOSS_TOL = 3e-6, 1e-5
_CACHE = {}


def case(*key):
    if key not in _CACHE:
        c = ref.make_case(*key[:5])
        c["loss64"], c["grad64"] = ref.oracle_loss_grads(c["sd"], c["ids"], c["pl"], c["images"], c["labels"])
        _CACHE[key] = c
    return _CACHE[key]


@pytest.mark.parametrize("geom,depth,n_ctx,C,B,cut", ref.CASES)
def test_restatement_equals_autograd_for_every_parameter(geom, depth, n_ctx, C, B, cut):
    """Float64 rounding, every parameter tensor: the autograd-free restatement on the island towers against autograd through the oracle."""
    c = case(geom, depth, n_ctx, C, B, cut)
    loss, grads = ref.loss_and_grads(c["sd"], c["ids"], c["pl"], c["images"], c["labels"], islands=True)
    assert abs(float(loss - c["loss64"])) <= RTOL * abs(float(c["loss64"]))
    assert sorted(grads) == sorted(ref.param_names(depth)) == sorted(c["grad64"])
    for name in ref.param_names(depth):
        want = c["grad64"][name]
        assert grads[name].shape == want.shape == c["pl"][name].shape, name
        assert float(want.norm()) > 0, name          # no tensor of these cases is cut off from the loss
        assert grads[name] is not want
        err = ref.rel_fro(grads[name], want)
        print(f"\nmaplefit-cpu: {geom} depth={depth} n_ctx={n_ctx} C={C} B={B} {name}: grad rel {err:.2e} (bound {RTOL:.0e})")
        assert err <= RTOL, name


@pytest.mark.parametrize("geom,depth,n_ctx,C,B,cut", ref.CASES)
def test_plain_float64_formulas_stay_within_the_oracles_fp32_islands(geom, depth, n_ctx, C, B, cut):
    """The formulas without the islands, on the live rows the case's GPU run computes, within the oracle's fp32 round-off."""
    c = case(geom, depth, n_ctx, C, B, cut)
    rows = ref.live_rows(c["ids"], cut) or None
    loss, grads = ref.loss_and_grads(c["sd"], c["ids"], c["pl"], c["images"], c["labels"], rows=rows)
    assert abs(float(loss - c["loss64"])) <= PLAIN_LOSS_TOL * max(1.0, abs(float(c["loss64"])))
    for name in ref.param_names(depth):
        assert ref.rel_fro(grads[name], c["grad64"][name]) <= PLAIN_TOL, name


def test_an_island_mistake_is_seen_at_the_bound():
    """The bound bites: a deep prompt spliced without its fp16 rounding (a wrong rounding point, 2^-12 relative on n_ctx rows) leaves it."""
    c = case(*ref.CASES[2])
    keep, ref.h = ref.h, (lambda t: t)
    try:
        _, grads = ref.loss_and_grads(c["sd"], c["ids"], c["pl"], c["images"], c["labels"], islands=True)
    finally:
        ref.h = keep
    assert max(ref.rel_fro(grads[n], c["grad64"][n]) for n in grads) > 1e3 * RTOL


def test_the_live_row_cut_changes_nothing():
    c = case(*ref.CASES[2])
    whole = ref.loss_and_grads(c["sd"], c["ids"], c["pl"], c["images"], c["labels"], rows=None)
    cut = ref.loss_and_grads(c["sd"], c["ids"], c["pl"], c["images"], c["labels"], rows=ref.live_rows(c["ids"], True))
    assert abs(float(whole[0] - cut[0])) <= 1e-12
    for name in whole[1]:
        assert ref.rel_fro(cut[1][name], whole[1][name]) <= 1e-12, name


def test_splice_and_its_reduction():
    """The splice writes half(deep) over rows 1 .. n_ctx of every prompt and nothing else; its reduction sums those rows over the prompts
    and zeroes them; the stash of block i holds the spliced rows; an EOT row directly behind the context rows is untouched."""
    c = case(*ref.CASES[2])
    sd, ids, pl = c["sd"], c["ids"], c["pl"]
    n_ctx, C = 3, ids.shape[0]
    assert int(ids[0].argmax()) == 1 + n_ctx
    deep = [pl["compound_prompts_text.0"], pl["compound_prompts_text.1"]]
    _, st = ref.text_forward(sd, ids, pl["ctx"], deep)
    _, plain = ref.text_forward(sd, ids, pl["ctx"], [])
    L = st["L"]
    for i in (1, 2):
        x = st["blocks"][i]["x_in"].reshape(C, L, -1)
        assert torch.equal(x[:, 1:1 + n_ctx], ref.h(deep[i - 1].double()).expand(C, -1, -1))
    x1, p1 = st["blocks"][1]["x_in"].reshape(C, L, -1), plain["blocks"][1]["x_in"].reshape(C, L, -1)
    assert torch.equal(x1[:, 0], p1[:, 0]) and torch.equal(x1[:, 1 + n_ctx:], p1[:, 1 + n_ctx:])      # block 0 ran on the same rows
    g = torch.randn(C * L, 64, dtype=torch.float64, generator=torch.Generator().manual_seed(3))
    out, g0 = ref.splice_reduce(g, C, L, n_ctx)
    g3 = g.reshape(C, L, -1)
    assert torch.allclose(out, sum(g3[k, 1:1 + n_ctx] for k in range(C)), rtol=0, atol=1e-15)
    assert not g0.reshape(C, L, -1)[:, 1:1 + n_ctx].any() and torch.equal(g0.reshape(C, L, -1)[:, 1 + n_ctx:], g3[:, 1 + n_ctx:])


@pytest.mark.parametrize("depth,n_ctx", [(1, 2), (3, 1), (3, 3)])
def test_coupling_forward_and_backward_against_autograd(depth, n_ctx):
    pl = ref.make_params("tiny3", n_ctx, depth, seed=4)
    vis = ref.couple_forward(pl)
    assert vis.shape == (depth, n_ctx, 192)
    p = {k: v.double().clone().requires_grad_(True) for k, v in pl.items()}
    hv = vref._HalfValue.apply
    want = [hv(p["ctx"]) @ hv(p["proj.weight"]).t() + hv(p["proj.bias"])]
    want += [p[f"compound_prompts_text.{i}"] @ p[f"compound_prompt_projections.{i}.weight"].t() + p[f"compound_prompt_projections.{i}.bias"]
             for i in range(depth - 1)]
    want = torch.stack(want)
    assert torch.equal(vis, want.detach())
    d_vis = torch.randn(depth, n_ctx, 192, dtype=torch.float64, generator=torch.Generator().manual_seed(5))
    (want * d_vis).sum().backward()
    got = ref.couple_backward(pl, d_vis)
    assert sorted(got) == sorted(ref.param_names(depth))
    for name in got:
        assert ref.rel_fro(got[name], p[name].grad) <= 1e-14, name
    # the oracle's own learner gives the same values where nothing is rounded (every slot but 0) and slot 0 up to proj's fp16 operands
    sd, ids = cref.state_dict("tiny3"), cref.prompt_ids("tiny3", 3, n_ctx)
    _, shared, _, deep_v = orc_learner(sd, ids, pl)
    for i in range(depth - 1):
        assert torch.equal(vis[1 + i], deep_v[i])
    assert ref.rel_fro(vis[0], shared) <= 2.0 ** -9


def orc_learner(sd, ids, pl):
    from oracle import clip_oracle as orc
    return orc.maple_prompt_learner(sd, ids, {k: v.double() for k, v in pl.items()}, torch.float64)


def test_joint_head_is_both_heads():
    g = torch.Generator().manual_seed(6)
    f, t = torch.randn(3, 64, generator=g).double(), torch.randn(5, 64, generator=g).double()
    y = torch.randint(0, 5, (3,), generator=g)
    loss, d_feats, d_text = ref.joint_head(f, y, t, 100.0)
    l1, want_text, _ = cref.head(f, y, t, 100.0)
    l2, want_feats, _ = vref.head_image(f, y, t, 100.0)
    assert float(loss) == float(l1) == float(l2)
    assert torch.equal(d_text, want_text) and torch.equal(d_feats, want_feats)


def test_master_block_layout():
    n_ctx, depth, Dt, Dv = 2, 3, 64, 192
    pl = ref.make_params("tiny3", n_ctx, depth)
    block = ref.pack(pl)
    assert block.numel() == ref.block_floats(n_ctx, depth, Dt, Dv) == depth * n_ctx * Dt + depth * (Dv * Dt + Dv)
    back = ref.unpack(block, n_ctx, depth, Dt, Dv)
    assert list(back) == ref.param_names(depth)
    for name in back:
        assert torch.equal(back[name], pl[name]), name
    # the text-side prompts are one [depth, n_ctx, Dt] array at the front, ctx first: what the text tower and the coupling kernel index
    t = block[:depth * n_ctx * Dt].reshape(depth, n_ctx, Dt)
    assert torch.equal(t[0], pl["ctx"]) and torch.equal(t[2], pl["compound_prompts_text.1"])
    at = depth * n_ctx * Dt
    assert torch.equal(block[at:at + Dv * Dt].reshape(Dv, Dt), pl["proj.weight"]) and torch.equal(block[at + Dv * Dt:at + Dv * Dt + Dv], pl["proj.bias"])
    assert torch.equal(block[-(depth - 1) * Dv:].reshape(depth - 1, Dv)[1], pl["compound_prompt_projections.1.bias"])
    assert ref.depth_of(pl) == depth and math.prod(pl["ctx"].shape) == n_ctx * Dt
    assert syn.GEOMETRIES["tiny3"].transformer_width == Dt and syn.GEOMETRIES["tiny3"].vision_width == Dv
