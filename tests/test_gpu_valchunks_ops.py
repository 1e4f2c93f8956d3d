"""The row-chunked validation score on the GPU (csrc/fit_monitor.hip; ops.val_score_rows, ops.val_score_finish): for every chunking of
tests/blockmonitor_ref.py the record equals clipmi_val_score's record on the whole matrix byte for byte, the row results equal the
one-chunk row results byte for byte, and two runs give the same bytes.  The sums are held to float64 by the bound of
tests/test_gpu_fitmonitor_ops.py (its ``hold_sums``: 2 x torch's own fp32 distance, floor ``fitmonitor_ref.FLOOR``)."""
import functools

import numpy as np
import pytest
import torch

import blockmonitor_ref as bref
import fitmonitor_ref as ref
from test_gpu_fitmonitor_ops import hold_sums

pytestmark = pytest.mark.gpu

from clip_calibration_amd import _lib, ops  # noqa: E402

GUARD = 0xA5
N_BINS = 10


@functools.lru_cache(maxsize=None)
def clean(N, C):
    return ref.clean_logits(N, C, N_BINS, seed=1000 * N + C)


def whole_record(zt, yt, n_bins=N_BINS):
    return ops.val_score(zt, yt, n_bins).cpu().numpy().copy()


def chunked(zt, yt, sizes, n_bins=N_BINS, tail=3):
    """(record bytes, row-result bytes) of the set scored chunk by chunk into a buffer with ``tail`` guard rows behind row N; every chunk
    is checked to have written its own rows alone."""
    N = zt.shape[0]
    rows = torch.full((N + tail, ops.VAL_ROW_BYTES), GUARD, dtype=torch.uint8, device="cuda")
    lo = 0
    for s in sizes:
        before = rows.clone()
        ops.val_score_rows(zt[lo:lo + s], yt[lo:lo + s], n_bins, rows, lo)
        keep = torch.ones(N + tail, dtype=torch.bool, device="cuda")
        keep[lo:lo + s] = False
        assert torch.equal(rows[keep], before[keep]), "a chunk wrote outside its rows"
        lo += s
    assert lo == N and bool((rows[N:] == GUARD).all())
    rec = ops.val_score_finish(rows[:N], n_bins)
    return rec.cpu().numpy().copy(), rows[:N].cpu().numpy().copy()


def every_chunking(zt, yt, tag, n_bins=N_BINS):
    want = whole_record(zt, yt, n_bins)
    one_rec, one_rows = chunked(zt, yt, [zt.shape[0]], n_bins)
    for name, sizes in bref.chunkings(zt.shape[0]).items():
        rec, rows = chunked(zt, yt, sizes, n_bins)
        assert np.array_equal(rec, want), f"{tag} {name}: the record differs from clipmi_val_score's"
        assert np.array_equal(rows, one_rows), f"{tag} {name}: the row results differ from the one-chunk row results"
    again, rows_again = chunked(zt, yt, bref.chunkings(zt.shape[0])["straddle"], n_bins)
    assert np.array_equal(again, want) and np.array_equal(rows_again, one_rows), f"{tag}: two runs differ"
    return want, one_rows


@pytest.mark.parametrize("C", [1, 2, 63, 64, 65, 1000])
@pytest.mark.parametrize("N", [1, 63, 64, 65, 129, 257])
def test_every_chunking_gives_val_scores_record(N, C):
    z, y = clean(N, C)
    zt, yt = torch.from_numpy(z).cuda(), torch.from_numpy(y).cuda()
    raw, rows = every_chunking(zt, yt, f"N={N} C={C}")
    got = ops.decode_val_records(raw, N_BINS)[0]
    want = ref.record(z, y, N_BINS)
    worst = hold_sums(f"chunked N={N} C={C}", got, want, z, y, N_BINS)
    print(f"blockmonitor-parity: N={N} C={C} chunked record against float64, worst ratio to the bound {worst:.3f}")
    # the row results against the restatement: hit and bin exactly (no confidence lies near an edge)
    r, w = ops.decode_val_row_results(rows), bref.row_results(z, y, N_BINS)
    assert np.array_equal(r["hit"], w["hit"]) and np.array_equal(r["bin"], w["bin"])


def test_a_row_stride():
    """ld = C + 3: the chunks are row slices of a column slice, read in place."""
    N, C = 129, 13
    z, y = ref.clean_logits(N, C, N_BINS, seed=77, scale=3.0)
    wide = torch.full((N, C + 3), float("nan"), device="cuda")
    wide[:, :C] = torch.from_numpy(z).cuda()
    view = wide[:, :C]
    assert view.stride(0) == C + 3 and not view.is_contiguous()
    yt = torch.from_numpy(y).cuda()
    raw, _ = every_chunking(view, yt, "strided")
    assert np.array_equal(raw, whole_record(torch.from_numpy(z).cuda(), yt))
    hold_sums("chunked strided", ops.decode_val_records(raw, N_BINS)[0], ref.record(z, y, N_BINS), z, y, N_BINS)
    # the call itself with ld = C + 3, the row pointer 16-byte aligned
    L, s = _lib.lib, torch.cuda.current_stream().cuda_stream
    wide4 = torch.full((8, 7), float("nan"), device="cuda")      # ld = 7: rows 0 and 4 start on 16-byte boundaries
    wide4[:, :4] = torch.from_numpy(z[:8, :4]).cuda()
    rr = ops.new_val_row_results(4, "cuda")
    assert L.clipmi_val_score_rows(wide4[4:].data_ptr(), 7, yt[4:].data_ptr(), 4, 4, N_BINS, rr.data_ptr(), s) == _lib.OK
    dense = ops.val_score_rows(torch.from_numpy(z[4:8, :4]).cuda(), yt[4:8], N_BINS)
    assert torch.equal(rr, dense)


def special(N, C, shift):
    """Clean logits with the special rows at rows 0, 63, 64 and N - 1, rotated by ``shift``: a NaN row; a label out of range; an exact
    two-way tie with the label on the higher index; a row with conf == 1.0.  ``shift`` runs over 0 .. 7: 0 .. 3 put the label -1 on
    every spot in turn, 4 .. 7 the label C."""
    z, y = clean(N, C)
    z, y = z.copy(), y.copy()
    spots = [0, 63, 64, N - 1]
    kinds = ["nan", "label", "tie", "one"]
    for k, kind in enumerate(kinds):
        r = spots[(k + shift) % 4]
        if kind == "nan":
            z[r, C // 2] = np.nan
        elif kind == "label":
            y[r] = -1 if shift < 4 else C
        elif kind == "tie":
            z[r] = -50.0
            z[r, 0] = z[r, C - 1] = 40.0
            y[r] = C - 1
        else:
            z[r] = -np.inf
            z[r, C - 1] = 3.0
            y[r] = C - 1
    return z, y, dict(zip(kinds, [spots[(k + shift) % 4] for k in range(4)]))


@pytest.mark.parametrize("shift", range(8))
@pytest.mark.parametrize("N,C", [(66, 2), (129, 65)])
def test_special_rows_at_the_seams(N, C, shift):
    z, y, where = special(N, C, shift)
    zt, yt = torch.from_numpy(z).cuda(), torch.from_numpy(y).cuda()
    assert yt.dtype == torch.int64
    raw, rows = every_chunking(zt, yt, f"special N={N} C={C} shift={shift}")
    r = ops.decode_val_row_results(rows)
    assert np.isnan(r["conf"][where["nan"]]) and np.isnan(r["nll"][where["nan"]]) and r["hit"][where["nan"]] == 0 and r["bin"][where["nan"]] == N_BINS
    assert np.isnan(r["nll"][where["label"]]) and r["hit"][where["label"]] == 0 and np.isfinite(r["conf"][where["label"]])
    assert r["hit"][where["tie"]] == 0 and r["conf"][where["tie"]] == 0.5 and abs(r["nll"][where["tie"]] - np.log(2.0)) < 1e-6
    assert r["conf"][where["one"]] == 1.0 and r["hit"][where["one"]] == 1 and r["bin"][where["one"]] == N_BINS and r["nll"][where["one"]] == 0.0
    got, want = ops.decode_val_records(raw, N_BINS)[0], ref.record(z, y, N_BINS)
    assert got["n"] == N and got["correct"] == want["correct"] and np.isnan(got["nll_sum"]) and np.isnan(want["nll_sum"])
    assert np.array_equal(got["count"], want["count"]) and np.array_equal(got["hits"], want["hits"])
    # the rows that are none of the four: every field within the bound
    keep = ~np.isin(np.arange(N), list(where.values()))
    zk, yk = np.ascontiguousarray(z[keep]), y[keep]
    rk, _ = every_chunking(torch.from_numpy(zk).cuda(), torch.from_numpy(yk).cuda(), "the other rows")
    hold_sums("chunked, the other rows", ops.decode_val_records(rk, N_BINS)[0], ref.record(zk, yk, N_BINS), zk, yk, N_BINS)


def test_other_bin_counts():
    N, C = 129, 37
    for n_bins in (1, 15, 64):
        z, y = ref.clean_logits(N, C, n_bins, seed=5 + n_bins, scale=3.0)
        zt, yt = torch.from_numpy(z).cuda(), torch.from_numpy(y).cuda()
        raw, _ = every_chunking(zt, yt, f"n_bins={n_bins}", n_bins)
        hold_sums(f"chunked n_bins={n_bins}", ops.decode_val_records(raw, n_bins)[0], ref.record(z, y, n_bins), z, y, n_bins)


def test_refusals_on_the_device_write_nothing():
    L, s = _lib.lib, torch.cuda.current_stream().cuda_stream
    z = torch.zeros(4, 8, device="cuda")
    yl = torch.zeros(4, dtype=torch.int64, device="cuda")
    rr = torch.full((8, 16), GUARD, dtype=torch.uint8, device="cuda")
    rec = torch.full((ops.val_record_bytes(N_BINS),), GUARD, dtype=torch.uint8, device="cuda")
    ws = torch.full((512,), GUARD, dtype=torch.uint8, device="cuda")
    rows = lambda **k: L.clipmi_val_score_rows(k.get("z", z.data_ptr()), k.get("ld", 8), k.get("y", yl.data_ptr()), k.get("rows", 4), k.get("C", 8),
                                               k.get("bins", N_BINS), k.get("rr", rr.data_ptr()), s)
    assert rows(z=None) == _lib.ERR_ARG and rows(y=None) == _lib.ERR_ARG and rows(rr=None) == _lib.ERR_ARG
    assert rows(z=z.data_ptr() + 4) == _lib.ERR_ARG and rows(y=yl.data_ptr() + 4) == _lib.ERR_ARG and rows(rr=rr.data_ptr() + 8) == _lib.ERR_ARG
    assert rows(rows=0) == _lib.ERR_SHAPE and rows(C=0) == _lib.ERR_SHAPE and rows(ld=7) == _lib.ERR_SHAPE
    assert rows(bins=0) == _lib.ERR_ARG and rows(bins=65) == _lib.ERR_ARG
    need = L.clipmi_val_score_finish_workspace_bytes(4, N_BINS)
    fin = lambda **k: L.clipmi_val_score_finish(k.get("rr", rr.data_ptr()), k.get("N", 4), k.get("bins", N_BINS), k.get("rec", rec.data_ptr()),
                                                k.get("ws", ws.data_ptr()), k.get("wsb", 512), s)
    assert fin(rr=None) == _lib.ERR_ARG and fin(rec=None) == _lib.ERR_ARG and fin(ws=None) == _lib.ERR_ARG
    assert fin(rr=rr.data_ptr() + 8) == _lib.ERR_ARG and fin(rec=rec.data_ptr() + 4) == _lib.ERR_ARG and fin(ws=ws.data_ptr() + 128) == _lib.ERR_ARG
    assert fin(N=0) == _lib.ERR_SHAPE and fin(bins=0) == _lib.ERR_ARG and fin(bins=65) == _lib.ERR_ARG and fin(wsb=need - 1) == _lib.ERR_WORKSPACE
    torch.cuda.synchronize()
    assert bool((rr == GUARD).all()) and bool((rec == GUARD).all()) and bool((ws == GUARD).all()), "a refused call wrote"
    assert rows() == _lib.OK and fin() == _lib.OK
    torch.cuda.synchronize()
    assert bool((rr[4:] == GUARD).all()) and not bool((rr[:4] == GUARD).all()) and not bool((rec == GUARD).all())
    with pytest.raises(ValueError, match="outside"):
        ops.val_score_rows(z, yl, N_BINS, rr, 5)
    with pytest.raises(ValueError, match="labels"):
        ops.val_score_rows(z, yl[:3], N_BINS, rr, 0)
