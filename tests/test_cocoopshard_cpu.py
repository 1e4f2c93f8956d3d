"""CPU checks of the class-sharded CoCoOp fit (``shard=`` on clip_calibration_amd/cocoopfit.py, csrc/cocoop_train.hip): the float64
restatement of the sharded step (tests/cocoopshard_ref.py) against tests/cocoopfit_ref.py's unsharded gradients, the layouts of the two
gathers, every refusal by its message before any device call, and the new symbols in the header and the binding."""
import numpy as np
import pytest
import torch

import cocoopfit_ref as cref
import cocoopshard_ref as sref
import coopfit_ref

from clip_calibration_amd import _lib, cocoopfit, coopfit, shard  # noqa: E402
from clip_calibration_amd.model import build_model  # noqa: E402

B, N_CTX, L, D, E, H = 2, 4, 9, 6, 5, 3


def stream(C, seed, dtype=np.float64):
    rng = np.random.RandomState(seed)
    d_embed = rng.standard_normal((B * C, L, D)) * 10.0 ** rng.uniform(-2, 2, (B * C, 1, 1))
    x, hid, w2 = rng.standard_normal((B, E)), np.maximum(rng.standard_normal((B, H)), 0), rng.standard_normal((D, H))
    return tuple(a.astype(dtype) for a in (d_embed, x, hid, w2))


# (C, G): an uneven split (3 | 2 and 2 | 2 | 1), one class per rank (C = G), and one rank
@pytest.mark.parametrize("C,G", [(5, 1), (5, 2), (5, 3), (2, 2), (3, 3)])
def test_float64_sharded_step_is_the_unsharded_gradient(C, G):
    """Partials per rank, the rank-ordered sum, the meta-net's backward: in float64 a regrouping of the unsharded chain's additions, so
    within 1e-9 (relative to the largest element) of cocoopfit_ref.reduce on the same stream, for every one of the five tensors."""
    d_embed, x, hid, w2 = stream(C, 10 * C + G)
    t = torch.from_numpy
    want = cref.reduce(t(d_embed), t(x), t(hid), t(w2), B, C, N_CTX)
    got = sref.sharded_gradient(d_embed, x, hid, w2, B, C, N_CTX, G)
    for k in cref.NAMES:
        assert got[k].dtype == np.float64 and np.abs(got[k] - want[k].numpy()).max() <= 1e-9 * np.abs(want[k].numpy()).max(), k
    blocks = sref.partials(d_embed, B, C, N_CTX, G, extra=3)
    assert blocks.shape == (G, B * N_CTX * D + 3) and int(np.isnan(blocks).sum()) == 3 * G          # the padded stride, and only it
    if G == 1:                                                                                      # one rank: the unsharded chain itself, in fp32 too
        d32, x32, h32, w32 = stream(C, 10 * C + G, np.float32)
        want32 = cref.reduce(t(d32), t(x32), t(h32), t(w32), B, C, N_CTX)
        got32 = sref.sharded_gradient(d32, x32, h32, w32, B, C, N_CTX, 1)
        for k in cref.NAMES:
            assert got32[k].dtype == np.float32 and np.array_equal(got32[k], want32[k].numpy()), k


def test_the_restatement_distinguishes_the_rank_order():
    blocks = np.zeros((3, 2), np.float32)
    blocks[:, 0] = (2.0 ** 24, 1.0, -2.0 ** 24)
    assert sref.reduce_partials(blocks, 2)[0] == 0.0 and sref.reduce_partials(blocks[[0, 2, 1]], 2)[0] == 1.0
    # and a rank's partial the class order
    d = np.zeros((3, 2, 1), np.float32)
    d[:, 1, 0] = (2.0 ** 24, 1.0, -2.0 ** 24)
    assert sref.partial(d, 1, 1)[0, 0, 0] == 0.0 and sref.partial(d[[0, 2, 1]], 1, 1)[0, 0, 0] == 1.0


@pytest.mark.parametrize("C,G", [(5, 2), (5, 3), (3, 3), (7, 1)])
def test_gather_layouts(C, G):
    """The text gather: rank r's block starts with its [B, C_r, E]; NaN in the padding rows and in a padded stride; compact undoes it."""
    text = np.arange(B * C * E, dtype=np.float32).reshape(B * C, E)
    g = sref.gathered_text(text, B, C, G, extra=2)
    assert g.shape == (G, B * sref.pad(C, G) * E + 2)
    assert int(np.isnan(g).sum()) == G * (B * sref.pad(C, G) * E + 2) - text.size
    assert np.array_equal(sref.compact(g, B, C, E), text)
    for r, (lo, hi) in enumerate(sref.split(C, G)):
        assert (lo, hi) == coopfit.shard_classes(C, G, r)
        own = sref.own_rows(text, B, C, lo, hi)
        assert np.array_equal(g[r, :own.size], own.reshape(-1)) and np.array_equal(own[hi - lo], text[C + lo])      # image 1, the rank's first class


# ----------------------------------------------------------------------------------------------------------------------- refusals
@pytest.fixture(scope="module")
def cpu_model():
    return build_model(dict(coopfit_ref.state_dict("tiny")), {"trainer": "CoOp"})


def test_refusals_name_their_cause_before_any_device_call(cpu_model):
    """A CPU model: a call that passes every check gets as far as needing the GPU (RuntimeError); a refused one raises ValueError
    before that -- nothing was enqueued."""
    c = cref.make_case("tiny", 5, 4, 2)
    ids, p, f, y = c["ids"], c["params"], c["feats"], c["labels"]
    two = lambda: coopfit.Shard(2, 0, coopfit.LocalGather(2))
    calls = {"fit_prompt_learner": lambda **kw: cocoopfit.fit_prompt_learner(f, y, cpu_model, ids, p, epochs=1, **kw),
             "CoCoOpFitState": lambda **kw: cocoopfit.CoCoOpFitState(cpu_model, ids, p, **kw),
             "gradients": lambda **kw: cocoopfit.gradients(cpu_model, ids, p, f, y, **kw)}
    for who, call in calls.items():
        with pytest.raises(ValueError, match=f"{who}: shard must be a coopfit.Shard"):
            call(shard=(2, 0))
        with pytest.raises(ValueError, match=f"{who}: shard: C=5 classes cannot be split over world=8 ranks"):
            call(shard=coopfit.Shard(8, 3, coopfit.LocalGather(8)))
        with pytest.raises(RuntimeError, match="GPU"):
            call(shard=two())                                            # everything checks out: the call needs the device
    for who in ("fit_prompt_learner", "CoCoOpFitState"):                 # neither Adam nor the dynamic scale is refused
        for kw in (dict(optimizer="adam"), dict(optimizer="adamw"), dict(grad_scale="dynamic", scaler={"init_scale": 2.0 ** 10}),
                   dict(optimizer="adam", grad_scale="dynamic")):
            with pytest.raises(RuntimeError, match="GPU"):
                calls[who](shard=two(), **kw)
    with pytest.raises(ValueError, match="fit_prompt_learner: shard has no validation: val="):
        calls["fit_prompt_learner"](shard=two(), val=(f, y))
    with pytest.raises(ValueError, match="fit_prompt_learner: shard has no validation: val=.*best_val"):
        calls["fit_prompt_learner"](shard=two(), val=(f, y), final_model="best_val")
    with pytest.raises(ValueError, match=r"gradients: shard returns no operand statistics \(return_operand_stats=True\)"):
        calls["gradients"](shard=two(), return_operand_stats=True)
    # the trainer refuses before either tower runs: this loader cannot be iterated
    from clip_calibration_amd import trainers
    clip = trainers.CoCoOpCLIP(cpu_model, ids, n_ctx=4)
    with pytest.raises(ValueError, match="fit_prompt_learner: shard has no validation"):
        clip.fit_prompt_learner(object(), shard=two(), val_loader=object())
    with pytest.raises(ValueError, match="fit_prompt_learner: shard has no validation"):
        clip.fit_prompt_learner(object(), shard=two(), val=(f, y))
    with pytest.raises(ValueError, match="fit_prompt_learner: shard: C=5 classes cannot be split over world=8"):
        clip.fit_prompt_learner(object(), shard=coopfit.Shard(8, 0, coopfit.LocalGather(8)))
    with pytest.raises(ValueError, match=r"fit_prompt_learner: shard has no one-call step \(one_call=True\)"):
        clip.fit_prompt_learner(object(), shard=two(), one_call=True)
    with pytest.raises(ValueError, match="fit_prompt_learner: shard must be a coopfit.Shard"):
        clip.fit_prompt_learner(object(), shard="two")
    # shard.check itself: the one-call step, which only CoCoOpFitState.step takes (tests/test_gpu_cocoopshard.py steps a state)
    with pytest.raises(ValueError, match=r"f: shard has no one-call step \(one_call=True\)"):
        shard.check("f", two(), n_cls=5, one_call=True)
    with pytest.raises(ValueError, match="f: shard has no validation"):
        shard.check("f", two(), n_cls=5, final_model="best_val")


def test_header_and_binding_carry_the_entry_points():
    header = open(_lib.HEADER_PATH).read()
    names = ("clipmi_cocoop_embed_classes", "clipmi_cocoop_shard_compact", "clipmi_cocoop_shard_rows", "clipmi_cocoop_dcs_partial",
             "clipmi_cocoop_reduce_gathered")
    for name in names:
        assert name in _lib._SIGNATURES and name in _lib.exported_symbols() and hasattr(_lib.lib, name) and f" {name}(" in header
    # argument checks come before the first launch and need no device
    lib = _lib.lib
    assert lib.clipmi_cocoop_shard_compact(256, 512, 2, 3, 8, 4, 1 << 20, None) == _lib.ERR_SHAPE and "C >= G" in _lib.last_error()
    assert lib.clipmi_cocoop_shard_compact(256, 512, 2, 5, 2, 4, 2 * 3 * 4 - 1, None) == _lib.ERR_SHAPE and "rank_stride" in _lib.last_error()
    assert lib.clipmi_cocoop_shard_compact(None, 512, 2, 5, 2, 4, 24, None) == _lib.ERR_ARG
    assert lib.clipmi_cocoop_shard_rows(256, 512, 2, 5, 3, 3, 4, None) == _lib.ERR_SHAPE and "non-empty range" in _lib.last_error()
    assert lib.clipmi_cocoop_shard_rows(256, 512, 2, 5, 3, 6, 4, None) == _lib.ERR_SHAPE
    assert lib.clipmi_cocoop_shard_rows(256, None, 2, 5, 3, 5, 4, None) == _lib.ERR_ARG
    assert lib.clipmi_cocoop_dcs_partial(256, 512, 2, 0, 8, 8, 4, None) == _lib.ERR_SHAPE
    assert lib.clipmi_cocoop_dcs_partial(256, 512, 2, 1, 4, 8, 4, None) == _lib.ERR_SHAPE and "SOS and the context" in _lib.last_error()
    assert lib.clipmi_cocoop_dcs_partial(None, 512, 2, 1, 8, 8, 4, None) == _lib.ERR_ARG
    red = lambda stride, ws_bytes, G=2, gs=1.0: lib.clipmi_cocoop_reduce_gathered(256, G, stride, 256, 256, 256, 256, 2, 8, 16, 4, 4, gs, 256, ws_bytes, None)
    need = lib.clipmi_cocoop_reduce_workspace_bytes(2, 4, 8, 4)
    assert red(2 * 4 * 8 - 1, need) == _lib.ERR_SHAPE and "rank_stride" in _lib.last_error()
    assert red(64, need - 1) == _lib.ERR_WORKSPACE
    assert red(64, need, G=0) == _lib.ERR_SHAPE and red(64, need, gs=0.0) == _lib.ERR_ARG
    emb = lambda lo, hi, C=5: lib.clipmi_cocoop_embed_classes(256, _lib.F32, 256, 256, 256, 256, 256, 2, C, lo, hi, 8, 16, 8, 4, None)
    assert emb(2, 2) == _lib.ERR_SHAPE and "non-empty range" in _lib.last_error()
    assert emb(4, 6) == _lib.ERR_SHAPE and emb(-1, 2) == _lib.ERR_SHAPE
    assert lib.clipmi_cocoop_embed(256, _lib.F32, 256, 256, 256, 256, 256, 2, 1, 8, 16, 8, 4, None) == _lib.ERR_SHAPE      # the unsharded call keeps C >= 2
