"""CPU checks of the class-sharded CoOp fit (clip_calibration_amd/coopfit.py ``shard=``, csrc/shard_train.hip): the split rule, the
padded gather layout and its compaction map, the restatement of the reduced gradient (tests/shardfit_ref.py) against
tests/coopfit_ref.py's, and what the first version refuses -- each before any device call: this file runs without a GPU."""
import numpy as np
import pytest
import torch

import coopfit_ref as ref
import shardfit_ref as sref

from clip_calibration_amd import _lib, coopfit  # noqa: E402
from clip_calibration_amd.model import build_model  # noqa: E402


# ------------------------------------------------------------------------------------------------------------------ 1. the split rule
@pytest.mark.parametrize("G", [1, 2, 3, 8])
@pytest.mark.parametrize("C", [5, 7, 1000])
def test_split_is_contiguous_balanced_and_covers_every_class_once(C, G):
    if C < G:
        for r in range(G):
            with pytest.raises(ValueError, match=f"C={C}"):
                coopfit.shard_classes(C, G, r)
        with pytest.raises(ValueError):
            sref.split(C, G)
        return
    bounds = [coopfit.shard_classes(C, G, r) for r in range(G)]
    assert bounds == sref.split(C, G)
    assert bounds[0][0] == 0 and bounds[-1][1] == C
    assert all(bounds[r][1] == bounds[r + 1][0] for r in range(G - 1))                       # contiguous, every class exactly once
    sizes = [hi - lo for lo, hi in bounds]
    assert sizes == [C // G + 1] * (C % G) + [C // G] * (G - C % G)                          # the first C mod G ranks one class more
    assert max(sizes) == -(-C // G)


# ------------------------------------------------------------------------------------------------------------- 2. the gathered layout
@pytest.mark.parametrize("G", [1, 2, 3, 8])
@pytest.mark.parametrize("C", [8, 13, 1000])
def test_padded_layout_and_compaction_map(C, G):
    E = 6
    full = np.arange(C * E, dtype=np.float32).reshape(C, E)
    blocks = [full[lo:hi] for lo, hi in sref.split(C, G)]
    gathered = sref.padded(blocks)
    assert gathered.shape == (G, -(-C // G), E)
    assert int(np.isnan(gathered).all(-1).sum()) == G * (-(-C // G)) - C                     # the padding rows, and only they
    out = sref.compact(gathered, C)
    assert np.array_equal(out, np.concatenate(blocks)) and np.array_equal(out, full)
    for c, (r, i) in enumerate(sref.compact_map(C, G)):
        lo, hi = coopfit.shard_classes(C, G, r)
        assert lo <= c < hi and i == c - lo


# ------------------------------------------------------------------------------------------------------------ 3. the reduced gradient
def stream(C, L, n_ctx, D, seed, integers=False):
    rng = np.random.RandomState(seed)
    g = rng.randint(-8, 9, size=(C * L, D)).astype(np.float32) if integers else (rng.standard_normal((C * L, D)) * 10.0 ** rng.uniform(-3, 3, (C * L, 1)))
    return g.astype(np.float32)


@pytest.mark.parametrize("C,L,n_ctx,D", [(5, 7, 4, 16), (37, 9, 4, 8)])
def test_one_shard_is_the_unsharded_gradient_exactly(C, L, n_ctx, D):
    """G = 1: one chain over all the classes in ascending order.  On integer-valued rows no addition rounds, so the restatement must equal
    coopfit_ref's gradient exactly whatever order that one adds in; on random rows it is the plain ascending fp32 loop, bit for bit."""
    g = stream(C, L, n_ctx, D, 0, integers=True)
    want = ref.ctx_gradient(torch.from_numpy(g).double(), C, L, n_ctx, False).numpy()
    rows = g.reshape(C, L, D)[:, 1:1 + n_ctx]
    assert np.array_equal(sref.reduced_gradient(rows, 1).astype(np.float64), want)
    g = stream(C, L, n_ctx, D, 1)
    rows = g.reshape(C, L, D)[:, 1:1 + n_ctx]
    s = np.zeros((n_ctx, D), np.float32)
    for c in range(C):
        s = s + rows[c]
    assert s.dtype == np.float32 and np.array_equal(sref.reduced_gradient(rows, 1), s)
    assert np.array_equal(sref.reduced_gradient(rows, 1, 256.0), s * np.float32(1 / 256.0))   # a power of two: exact


@pytest.mark.parametrize("G", [1, 2, 3, 8])
@pytest.mark.parametrize("C,L,n_ctx,D", [(8, 7, 4, 16), (37, 9, 4, 8), (1000, 6, 4, 4)])
def test_reduced_gradient_stays_within_fp32_summation_error(C, L, n_ctx, D, G):
    """The sum over ranks, in rank order, of the per-rank ascending sums: within fp32 summation error of coopfit_ref's float64 gradient.
    The bound is shardfit_ref.sum_bound's, from the number of rounded additions a term passes through and fp32's unit roundoff."""
    g = stream(C, L, n_ctx, D, 2)
    rows = g.reshape(C, L, D)[:, 1:1 + n_ctx]
    want = ref.ctx_gradient(torch.from_numpy(g).double(), C, L, n_ctx, False).numpy()
    got = sref.reduced_gradient(rows, G)
    parts = sref.partials(rows, G)
    assert parts.shape == (G, n_ctx, D) and np.array_equal(got, sref.rank_sum(parts))
    err, bound = np.abs(got.astype(np.float64) - want), sref.sum_bound(rows, G)
    assert (err <= bound).all(), float((err / bound).max())
    if G > 1 and C >= 37:
        assert not np.array_equal(got, sref.reduced_gradient(rows, 1))                       # the result depends on G: the chains differ


def test_rank_order_matters_where_the_partials_cancel():
    """One large and one tiny value per rank: only the rank-ordered sum gives the restatement's bits."""
    parts = np.array([[2.0 ** 24], [1.0], [-2.0 ** 24]], np.float32)
    assert sref.rank_sum(parts)[0] == 0.0 and sref.rank_sum(parts[[0, 2, 1]])[0] == 1.0


# ----------------------------------------------------------------------------------------------------------------------- 4. refusals
@pytest.fixture(scope="module")
def cpu_model():
    return build_model(dict(ref.state_dict("tiny")), {"trainer": "CoOp"})


def test_refusals_name_their_cause_before_any_device_call(cpu_model):
    c = ref.make_case("tiny", 5, 4, 4)
    ids, ctx, f, y = c["ids"], c["ctx"], c["feats"], c["labels"]
    two = coopfit.Shard(2, 0, coopfit.LocalGather(2))
    eight = coopfit.Shard(8, 3, coopfit.LocalGather(8))
    calls = [lambda **kw: coopfit.fit_context(f, y, cpu_model, ids, ctx, epochs=1, **kw),
             lambda **kw: coopfit.CoOpFitState(cpu_model, ids, ctx, **kw),
             lambda **kw: coopfit.context_gradient(cpu_model, ids, ctx, f, y, **kw)]
    for call in calls:
        with pytest.raises(ValueError, match="C=5 classes cannot be split over world=8"):
            call(shard=eight)
        with pytest.raises(ValueError, match="class_token_position='end' only, not 'middle'"):
            call(shard=two, class_token_position="middle")
        with pytest.raises(ValueError, match="coopfit.Shard"):
            call(shard=(2, 0))
    for call in calls[:2]:
        with pytest.raises(ValueError, match="shard needs a static grad_scale"):
            call(shard=two, grad_scale="dynamic")
    with pytest.raises(ValueError, match="shard has no validation"):
        calls[0](shard=two, val=(f, y))
    with pytest.raises(ValueError, match="shard has no validation"):
        calls[0](shard=two, val=(f, y), final_model="best_val")
    with pytest.raises(ValueError, match="operand statistics"):
        calls[2](shard=two, return_operand_stats=True)
    with pytest.raises(RuntimeError, match="GPU"):
        calls[0](shard=two)                                   # everything checks out: the call needs the device
    with pytest.raises(ValueError, match="outside world"):
        coopfit.Shard(2, 2, coopfit.LocalGather(2))
    with pytest.raises(ValueError, match="LocalGather was made for 3"):
        coopfit.Shard(2, 0, coopfit.LocalGather(3))
    with pytest.raises(ValueError, match="callable"):
        coopfit.Shard(2, 0, None)


def test_header_and_binding_carry_the_entry_points():
    header = open(_lib.HEADER_PATH).read()
    for name in ("clipmi_shard_compact", "clipmi_ctx_partial", "clipmi_ctx_step_gathered", "clipmi_shard_prograd_workspace_bytes",
                 "clipmi_shard_prograd_dots", "clipmi_shard_prograd_apply"):
        assert name in _lib._SIGNATURES and name in _lib.exported_symbols() and hasattr(_lib.lib, name) and f" {name}(" in header
    # argument checks come before the first launch and need no device
    assert _lib.lib.clipmi_shard_compact(256, 512, 3, 4, 8, None) == _lib.ERR_SHAPE and "C >= G" in _lib.last_error()
    assert _lib.lib.clipmi_ctx_partial(256, 512, 2, 4, 8, 4, None) == _lib.ERR_SHAPE
    assert _lib.lib.clipmi_ctx_step_gathered(256, 2, 16, 512, None, None, 8, 4, 1.0, 768, 1, 0.0, 0.0, 0.0, 0, None) == _lib.ERR_SHAPE   # stride < n_ctx D
    assert _lib.lib.clipmi_ctx_step_gathered(256, 2, 32, 512, None, None, 8, 4, 1.0, None, 1, 0.0, 0.0, 0.0, 0, None) == _lib.ERR_ARG    # a step without lr
    assert _lib.lib.clipmi_shard_prograd_workspace_bytes(0) == 0 and _lib.lib.clipmi_shard_prograd_workspace_bytes(100) >= 3 * 256 * 8 + 800


# ------------------------------------------------------------------------------------------------------- 5. starting and ending ranks
def test_rank_env_indexes_the_visible_devices_it_is_given():
    from clip_calibration_amd.parallel import rank_env
    assert rank_env(1, env={})["HIP_VISIBLE_DEVICES"] == "1" and "MASTER_PORT" not in rank_env(1, env={})
    e = rank_env(1, 4321, env={"HIP_VISIBLE_DEVICES": "4,5", "OTHER": "x"})
    assert e["HIP_VISIBLE_DEVICES"] == "5" and e["MASTER_ADDR"] == "127.0.0.1" and e["MASTER_PORT"] == "4321" and e["OTHER"] == "x"
    e = rank_env(0, env={"CUDA_VISIBLE_DEVICES": "2, 3"})
    assert e["CUDA_VISIBLE_DEVICES"] == "2" and "HIP_VISIBLE_DEVICES" not in e                # the parent's restriction is never widened
    with pytest.raises(ValueError, match="outside HIP_VISIBLE_DEVICES=4,5"):
        rank_env(2, env={"HIP_VISIBLE_DEVICES": "4,5"})


def test_end_session_ends_the_process_under_the_timeout_wrapper():
    """What the rank tests and the bench do when a rank fails: the OTHER ranks are ended, and that means the process under ``timeout``,
    not the wrapper alone."""
    import subprocess
    import sys
    from clip_calibration_amd.parallel import end_session
    p = subprocess.Popen(["timeout", "-k", "10", "60", sys.executable, "-c", "import os, time; print(os.getpid(), flush=True); time.sleep(60)"],
                         stdout=subprocess.PIPE, text=True, start_new_session=True)
    pid = int(p.stdout.readline())
    assert pid != p.pid and p.poll() is None
    end_session(p)
    p.stdout.close()
    assert p.returncode is not None
    import time
    deadline = time.monotonic() + 10.0                      # SIGKILL has been sent to the group; the kernel delivers it in its own time
    while True:
        try:                                                # gone, or a zombie that waits for its reaper: not running either way
            state = open(f"/proc/{pid}/stat").read().rsplit(")", 1)[1].split()[0]
        except (FileNotFoundError, ProcessLookupError):
            state = None
        if state in (None, "Z", "X") or time.monotonic() > deadline:
            break
        time.sleep(0.01)
    assert state in (None, "Z", "X"), state
    end_session(p)                                          # a child that has ended is left alone
