"""CPU checks of the class-sharded ProDA fit (``shard=`` on clip_calibration_amd/prodafit.py, csrc/proda_train.hip): the float64
restatement of the sharded step (tests/prodashard_ref.py) against tests/prodafit_ref.py's unsharded gradient, the dealing of the no-class
prompts, every refusal by its message before any device call, and the new symbols in the header and the binding."""
import numpy as np
import pytest
import torch

import coopfit_ref
import prodafit_ref as dref
import prodashard_ref as sref

from clip_calibration_amd import _lib, coopfit, prodafit, shard  # noqa: E402
from clip_calibration_amd.model import build_model  # noqa: E402
from clip_calibration_amd.parallel import shard_bounds  # noqa: E402

P, PB, N_CTX, L, D = 8, 4, 4, 12, 6
POS = dref.positions(P)
SEL = dref.ordered((1, 6, 2, 5), POS)


# (C, G): an uneven split (3 | 2 and 2 | 2 | 1), one class per rank (C = G), and one rank
@pytest.mark.parametrize("C,G", [(5, 1), (5, 2), (5, 3), (2, 2), (3, 3)])
def test_float64_sharded_step_is_the_unsharded_gradient(C, G):
    """Partials per rank, the rank-ordered sum, the no-class row last: in float64 a regrouping of the unsharded chain's additions, so
    within 1e-9 (relative to the largest element) of prodafit_ref.ctx_reduce on the same stream."""
    rng = np.random.RandomState(10 * C + G)
    name_lens = np.arange(C) % 4
    d_embed = rng.standard_normal((C * PB + P, L, D)) * 10.0 ** rng.uniform(-2, 2, (C * PB + P, 1, 1))
    want = dref.ctx_reduce(torch.from_numpy(d_embed), SEL, POS, name_lens, C, P, N_CTX).numpy()
    got = sref.sharded_gradient(d_embed, SEL, POS, name_lens, C, P, N_CTX, G)
    assert got.dtype == np.float64 and np.abs(got - want).max() <= 1e-9 * np.abs(want).max()
    blocks = sref.send_blocks(d_embed, SEL, POS, name_lens, C, P, N_CTX, G)
    assert blocks.shape == (G, PB + -(-P // G), N_CTX, D)
    assert int(np.isnan(blocks).all((-1, -2)).sum()) == G * -(-P // G) - P                  # the padding slots, and only they
    unselected = [p for p in range(P) if p not in SEL]
    assert np.array_equal(got[unselected], d_embed[C * PB:, 1:1 + N_CTX][unselected])       # 0 + the no-class row alone
    if G == 1:                                                                              # one rank: the unsharded chain itself, in fp32 too
        d32 = d_embed.astype(np.float32)
        want32 = dref.ctx_reduce(torch.from_numpy(d32), SEL, POS, name_lens, C, P, N_CTX).numpy()
        assert np.array_equal(sref.sharded_gradient(d32, SEL, POS, name_lens, C, P, N_CTX, 1), want32)


def test_the_restatement_distinguishes_the_rank_order():
    blocks = np.zeros((3, 1 + 1, 1, 1), np.float32)
    blocks[:, 0, 0, 0] = (2.0 ** 24, 1.0, -2.0 ** 24)
    sel = np.array([0])
    assert sref.reduce_blocks(blocks, sel, 3)[0, 0, 0] == 0.0 and sref.reduce_blocks(blocks[[0, 2, 1]], sel, 3)[0, 0, 0] == 1.0


@pytest.mark.parametrize("G,want", [(3, [(0, 3), (3, 6), (6, 8)]), (8, [(p, p + 1) for p in range(8)])])
def test_no_class_prompts_are_dealt_out(G, want):
    """P = 8: contiguous ranges, the first P mod G ranks one more, every prompt owned once -- never replicated."""
    bounds = [shard_bounds(8, r, G) for r in range(G)]
    assert bounds == want == sref.split(8, G)
    assert sorted(p for lo, hi in bounds for p in range(lo, hi)) == list(range(8))
    for p in range(8):
        r, lo = sref.owner(p, 8, G)
        assert bounds[r][0] == lo <= p < bounds[r][1]
    text = np.arange((5 * 2 + 8) * 3, dtype=np.float32).reshape(-1, 3)
    if G == 3:                                                                              # the text gather's layout and its padding
        g = sref.gathered_text(text, 5, 2, 8, G)
        assert g.shape == (3, 2 * 2 + 3, 3) and int(np.isnan(g).all(-1).sum()) == 3 * 7 - 18
        assert np.array_equal(g[2, :2], text[8:10]) and np.array_equal(g[2, 2:4], text[16:18])


# ----------------------------------------------------------------------------------------------------------------------- refusals
@pytest.fixture(scope="module")
def cpu_model():
    return build_model(dict(coopfit_ref.state_dict("tiny")), {"trainer": "CoOp"})


def test_refusals_name_their_cause_before_any_device_call(cpu_model):
    """A CPU model: a call that passes every check gets as far as needing the GPU (RuntimeError); a refused one raises ValueError
    before that -- nothing was enqueued."""
    c = dref.make_case("tiny", 5, 4, 8, 4, 2)
    ids, ctx, f, y = c["ids"], c["ctx"], c["feats"], c["labels"]
    two = lambda: coopfit.Shard(2, 0, coopfit.LocalGather(2))
    calls = {"fit_context": lambda **kw: prodafit.fit_context(f, y, cpu_model, ids, ctx, prompt_bs=4, epochs=1, **kw),
             "ProDAFitState": lambda **kw: prodafit.ProDAFitState(cpu_model, ids, ctx, prompt_bs=4, **kw),
             "context_gradient": lambda **kw: prodafit.context_gradient(cpu_model, ids, ctx, f, y, sel=(1, 6, 2, 5), **kw)}
    for who, call in calls.items():
        with pytest.raises(ValueError, match=f"{who}: shard must be a coopfit.Shard"):
            call(shard=(2, 0))
        with pytest.raises(ValueError, match=f"{who}: shard: C=5 classes cannot be split over world=8 ranks"):
            call(shard=coopfit.Shard(8, 3, coopfit.LocalGather(8)))
        with pytest.raises(RuntimeError, match="GPU"):
            call(shard=two())                                            # everything checks out: the call needs the device
    ids16 = dref.prompt_ids("tiny", 16, 4)
    few = dict(ctx=ctx, ids=ids16, y=torch.zeros(2, dtype=torch.int64))
    sixteen = lambda: coopfit.Shard(16, 0, coopfit.LocalGather(16))
    with pytest.raises(ValueError, match="fit_context: shard: P=8 no-class prompts cannot be dealt out to world=16 ranks"):
        prodafit.fit_context(f, few["y"], cpu_model, ids16, ctx, prompt_bs=4, epochs=1, shard=sixteen())
    with pytest.raises(ValueError, match="ProDAFitState: shard: P=8 no-class prompts cannot be dealt out to world=16 ranks"):
        prodafit.ProDAFitState(cpu_model, ids16, ctx, prompt_bs=4, shard=sixteen())
    with pytest.raises(ValueError, match="context_gradient: shard: P=8 no-class prompts cannot be dealt out to world=16 ranks"):
        prodafit.context_gradient(cpu_model, ids16, ctx, f, few["y"], shard=sixteen())
    for who in ("fit_context", "ProDAFitState"):
        for opt in ("adam", "adamw"):
            with pytest.raises(ValueError, match=f"{who}: shard with optimizer='{opt}': the class-sharded fit stays SGD"):
                calls[who](shard=two(), optimizer=opt)
        with pytest.raises(RuntimeError, match="GPU"):                   # both loss scales pass the checks
            calls[who](shard=two(), grad_scale="dynamic", scaler={"init_scale": 2.0 ** 12})
    with pytest.raises(ValueError, match="fit_context: shard has no validation: val="):
        calls["fit_context"](shard=two(), val=(f, y))
    with pytest.raises(ValueError, match="fit_context: shard has no validation: val=.*best_val"):
        calls["fit_context"](shard=two(), val=(f, y), final_model="best_val")
    with pytest.raises(ValueError, match=r"context_gradient: shard returns no operand statistics \(return_operand_stats=True\)"):
        calls["context_gradient"](shard=two(), return_operand_stats=True)
    with pytest.raises(RuntimeError, match="GPU"):                       # without shard the statistics are an argument like any other
        calls["context_gradient"](return_operand_stats=True)
    # the trainer refuses before either tower runs: this loader cannot be iterated
    from clip_calibration_amd import trainers
    clip = trainers.ProDACLIP(cpu_model, ids, n_ctx=4, n_prompt=8)
    with pytest.raises(ValueError, match="fit_context: shard has no validation"):
        clip.fit_context(object(), shard=two(), val_loader=object())
    with pytest.raises(ValueError, match="fit_context: shard: C=5 classes cannot be split over world=8"):
        clip.fit_context(object(), shard=coopfit.Shard(8, 0, coopfit.LocalGather(8)))
    # shard.check itself: the one-call step, which only ProDAFitState.step takes (tests/test_gpu_prodashard.py steps a state)
    with pytest.raises(ValueError, match=r"f: shard has no one-call step \(one_call=True\)"):
        shard.check("f", two(), n_cls=5, n_prompt=8, one_call=True)
    with pytest.raises(ValueError, match="f: shard has no validation"):
        shard.check("f", two(), n_cls=5, n_prompt=8, final_model="best_val")


def test_header_and_binding_carry_the_entry_points():
    header = open(_lib.HEADER_PATH).read()
    names = ("clipmi_proda_embed_shard", "clipmi_proda_shard_compact", "clipmi_proda_ctx_partial", "clipmi_proda_ctx_step_gathered",
             "clipmi_proda_ctx_reduce_gathered_scaled")
    for name in names:
        assert name in _lib._SIGNATURES and name in _lib.exported_symbols() and hasattr(_lib.lib, name) and f" {name}(" in header
    assert _lib.ABI_VERSION == 16 and _lib.lib.clipmi_abi_version() == 16
    # argument checks come before the first launch and need no device
    lib = _lib.lib
    assert lib.clipmi_proda_shard_compact(256, 512, 3, 2, 8, 4, 8, None) == _lib.ERR_SHAPE and "C >= G" in _lib.last_error()
    assert lib.clipmi_proda_shard_compact(256, 512, 8, 2, 3, 4, 8, None) == _lib.ERR_SHAPE                                       # P < G
    assert lib.clipmi_proda_ctx_partial(256, 512, 768, 768, 768, 2, 2, 8, 9, 16, 8, 4, None) == _lib.ERR_SHAPE                    # Pn > P
    assert lib.clipmi_proda_ctx_partial(256, 512, None, 768, 768, 2, 2, 8, 4, 16, 8, 4, None) == _lib.ERR_ARG
    step = lambda stride, lr, G=2: lib.clipmi_proda_ctx_step_gathered(256, G, stride, 512, None, None, 768, 2, 8, 8, 4, 1.0, lr, 1, 0.0, 0.0, 0.0, 0, None)
    assert step((2 + 4) * 32 - 1, 1024) == _lib.ERR_SHAPE and "rank_stride" in _lib.last_error()
    assert step((2 + 4) * 32, None) == _lib.ERR_ARG                                                                            # a step without lr
    assert step(4096, 1024, G=9) == _lib.ERR_SHAPE                                                                             # P < G
    assert lib.clipmi_proda_ctx_reduce_gathered_scaled(256, 2, 4096, 512, None, None, 768, 2, 8, 8, 4, None, 2.0, 0.5, 10, 1024, 0.0, 0.0, 0.0, 0, 2048, 1 << 20,
                                                       None) == _lib.ERR_ARG                                                      # no state block
    assert lib.clipmi_proda_embed_shard(256, 256, _lib.F32, 256, 256, 256, 256, 256, 256, 256, 1, 2, 8, 6, 3, 16, 16, 8, 4, None) == _lib.ERR_SHAPE
    assert "leave the P=8 contexts" in _lib.last_error()
