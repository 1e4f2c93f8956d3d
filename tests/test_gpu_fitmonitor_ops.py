"""The fit monitor's two entry points on the GPU (csrc/fit_monitor.hip; ops.val_score, ops.best_select) against the float64
restatement of tests/fitmonitor_ref.py.

Integer fields are held exactly -- the inputs are built so that no confidence lies within 2^-20 (relative) of a bin edge without lying
on it; a row that does is drawn again, none is left out.  The two fp32 sums, nll_sum and every bin's conf_sum, are held to
2 x the distance of torch's own fp32 computation on the same GPU from float64 (F.cross_entropy and softmax().max() in fp32, summed in
float64), with a floor of 2^-22 relative.  Every figure goes out on a line that starts with "fitmonitor-parity:";
profiles/fitmonitor_parity.txt is one run's lines."""
import functools

import numpy as np
import pytest
import torch

import fitmonitor_ref as ref

pytestmark = pytest.mark.gpu

from clip_calibration_amd import _lib, ops  # noqa: E402

GUARD = 0xA5
ROWS_PER_WORKGROUP = 64      # csrc/fit_monitor.hip VS_ROWS


def say(line):
    print("fitmonitor-parity: " + line)


def guarded(nbytes, pad=256):
    """(whole uint8 buffer filled with the guard byte, the view of ``nbytes`` in its middle)."""
    whole = torch.full((nbytes + 2 * pad,), GUARD, dtype=torch.uint8, device="cuda")
    return whole, whole[pad:pad + nbytes]


def guards_intact(whole, nbytes, pad=256):
    w = whole.cpu().numpy()
    return bool((w[:pad] == GUARD).all() and (w[pad + nbytes:] == GUARD).all())


def device_record(z, y, n_bins):
    """(decoded record, raw bytes) with guard words around the record and the workspace."""
    zt, yt = torch.from_numpy(z).cuda(), torch.from_numpy(y).cuda()
    nb = ops.val_record_bytes(n_bins)
    need = _lib.lib.clipmi_val_score_workspace_bytes(z.shape[0], n_bins)
    rec_whole, rec = guarded(nb)
    ws_whole, ws = guarded(need)
    out = ops.val_score(zt, yt, n_bins, rec, ws)
    assert out.data_ptr() == rec.data_ptr()
    torch.cuda.synchronize()
    assert guards_intact(rec_whole, nb) and guards_intact(ws_whole, need)
    raw = rec.cpu().numpy().copy()
    return ops.decode_val_records(raw, n_bins)[0], raw


def torch_fp32_sums(z, y, which, n_bins, with_nll=True):
    """torch's own fp32 computation on the GPU, summed in float64: (nll_sum, conf_sum per bin of the restatement's bins)."""
    zt, yt = torch.from_numpy(z).cuda(), torch.from_numpy(y).cuda()
    nll = torch.nn.functional.cross_entropy(zt, yt, reduction="none").double().sum().item() if with_nll else float("nan")
    conf = torch.softmax(zt, dim=1).max(dim=1).values.double().cpu().numpy()
    sums = np.zeros(n_bins + 1)
    np.add.at(sums, which, conf)
    return nll, sums


def hold_sums(tag, got, want, z, y, n_bins, with_nll=True):
    """The integer fields exactly; the two kinds of fp32 sums within max(2 x torch's fp32 distance, 2^-22 relative)."""
    assert got["n"] == want["n"] and got["correct"] == want["correct"], tag
    assert np.array_equal(got["count"], want["count"]) and np.array_equal(got["hits"], want["hits"]), tag
    from clip_calibration_amd import metrics
    which = metrics.digitize_bins(ref.score_rows(z, y)[2], n_bins)
    t_nll, t_conf = torch_fp32_sums(z, y, which, n_bins, with_nll)
    pairs = [("nll_sum", got["nll_sum"], want["nll_sum"], t_nll)] if with_nll else []
    pairs += [(f"conf_sum[{b}]", got["conf_sum"][b], want["conf_sum"][b], t_conf[b]) for b in range(n_bins + 1) if want["count"][b]]
    worst = 0.0
    for name, g, w, t in pairs:
        bound = max(2.0 * abs(t - w), ref.FLOOR * abs(w))
        err = abs(g - w)
        say(f"{tag} {name}: device {err:.3e}, torch fp32 {abs(t - w):.3e}, floor {ref.FLOOR * abs(w):.3e}, ratio to the bound "
            f"{err / bound if bound else 0.0:.3f}")
        worst = max(worst, err / bound if bound else (0.0 if err == 0 else np.inf))
        assert err <= bound, (tag, name, g, w, t)
    for b in range(n_bins + 1):
        if not want["count"][b]:
            assert got["conf_sum"][b] == 0.0
    return worst


@functools.lru_cache(maxsize=None)
def clean(N, C, n_bins):
    return ref.clean_logits(N, C, n_bins, seed=1000 * N + C)


@pytest.mark.parametrize("C", [1, 2, 63, 64, 65, 1000])
@pytest.mark.parametrize("N", [1, 67, ROWS_PER_WORKGROUP + 1])
def test_val_score_shapes_at_scale_100(N, C):
    n_bins = 10
    z, y = clean(N, C, n_bins)
    conf = ref.score_rows(z, y)[2]
    if N > 1:
        assert (conf == 1.0).any(), "no saturated row: the last bin is not exercised"
    want = ref.record(z, y, n_bins)
    got, raw = device_record(z, y, n_bins)
    hold_sums(f"N={N} C={C}", got, want, z, y, n_bins)
    if N > 1 and C > 1:
        assert want["count"][n_bins] >= 1 and 0 < want["correct"] < N
    _, again = device_record(z, y, n_bins)
    assert np.array_equal(raw, again), "two runs differ"


def test_val_score_more_workgroups_and_a_row_stride():
    """Several workgroups with a short last one, 15 bins, a small logit scale (no saturation), logits that are a column slice."""
    n_bins, N, C = 15, 3 * ROWS_PER_WORKGROUP + 5, 37
    z, y = ref.clean_logits(N, C, n_bins, seed=11, scale=3.0)
    wide = torch.full((N, C + 11), float("nan"), device="cuda")
    wide[:, 4:4 + C] = torch.from_numpy(z).cuda()
    view = wide[:, 4:4 + C]
    assert view.data_ptr() % 16 == 0 and view.stride(0) == C + 11
    rec = ops.decode_val_records(ops.val_score(view, torch.from_numpy(y).cuda(), n_bins), n_bins)[0]
    want = ref.record(z, y, n_bins)
    got, _ = device_record(z, y, n_bins)
    hold_sums("strided", got, want, z, y, n_bins)
    assert rec["nll_sum"] == got["nll_sum"] and np.array_equal(rec["conf_sum"], got["conf_sum"]) and np.array_equal(rec["count"], got["count"])
    assert sum(1 for c in want["count"] if c) >= 4


def test_val_score_ties_equal_rows_and_minus_inf():
    n_bins, N, C = 15, 67, 65
    z, y = ref.clean_logits(N, C, n_bins, seed=5, scale=4.0)
    z[3, 7] = z[3, 40] = z[3].max() + 30.0          # a tie at the maximum, far above the rest: the lower index wins, conf = 1/2
    y[3] = 7
    z[4, 9] = z[4, 64] = z[4].max() + 30.0
    y[4] = 64                                       # the label on the higher index of the tie: wrong
    z[5, :] = -2.5                                  # a row of equal values: index 0, conf = 1/65
    y[5] = 0
    z[6, :] = 1.0
    y[6] = 1
    z[7, ::2] = -np.inf                             # -inf entries, the label on one of them: an infinite nll
    y[7] = 2
    z[8, 1:] = -np.inf                              # everything but one entry: conf = 1
    y[8] = 0
    hit, nll, conf = ref.score_rows(z, y)
    assert ref.off_the_edges(conf, n_bins)
    assert hit[3] and not hit[4] and hit[5] and not hit[6] and not hit[7] and hit[8] and np.isinf(nll[7]) and conf[8] == 1.0
    want = ref.record(z, y, n_bins)
    got, _ = device_record(z, y, n_bins)
    assert got["n"] == N and got["correct"] == want["correct"]
    assert np.array_equal(got["count"], want["count"]) and np.array_equal(got["hits"], want["hits"])
    assert got["nll_sum"] == np.inf == want["nll_sum"]
    # the finite part of the sums: the same rows without the infinite one
    keep = np.arange(N) != 7
    hold_sums("ties", device_record(z[keep], y[keep], n_bins)[0], ref.record(z[keep], y[keep], n_bins), z[keep], y[keep], n_bins)


def test_val_score_nan_row_and_labels_out_of_range():
    n_bins, N, C = 10, 67, 63
    z, y = clean(N, C, n_bins)
    z, y = z.copy(), y.copy()
    z[10, 5] = np.nan
    y[10] = int(np.nanargmax(z[10]))
    y[20], y[21], y[22] = C, -1, 2 ** 40
    want = ref.record(z, y, n_bins)
    got, _ = device_record(z, y, n_bins)
    assert got["n"] == N and got["correct"] == want["correct"] and np.isnan(got["nll_sum"]) and np.isnan(want["nll_sum"])
    assert np.array_equal(got["count"], want["count"]) and np.array_equal(got["hits"], want["hits"])
    assert np.isnan(got["conf_sum"][n_bins])                      # the NaN confidence sorts into the last bin
    # without the NaN row: the out-of-range labels alone still make nll_sum NaN and count as wrong
    keep = np.arange(N) != 10
    got2, _ = device_record(z[keep], y[keep], n_bins)
    want2 = ref.record(z[keep], y[keep], n_bins)
    assert np.isnan(got2["nll_sum"]) and np.isnan(want2["nll_sum"]) and np.isfinite(got2["conf_sum"]).all()
    hold_sums("labels out of range", got2, want2, z[keep], y[keep], n_bins, with_nll=False)
    # and the rows that are neither: every field
    keep = ~np.isin(np.arange(N), (10, 20, 21, 22))
    hold_sums("the other rows", device_record(z[keep], y[keep], n_bins)[0], ref.record(z[keep], y[keep], n_bins), z[keep], y[keep], n_bins)


# ---------------------------------------------------------------------------------------------------------------------- best_select
def guarded_floats(n, fill):
    whole = torch.full((n + 8,), fill, dtype=torch.float32, device="cuda")
    return whole, whole[4:4 + n]


def run_sequence(seq, criterion, n_floats):
    """The best block and best_params after every epoch of ``seq``; the params of epoch e are e + 1 + arange / 2^20."""
    recs = torch.from_numpy(ops.encode_val_records([{"n": 8, "correct": c, "nll_sum": v} for c, v in seq], 10)).cuda()
    block = ops.new_best_block("cuda")
    whole, best = guarded_floats(n_floats, -7.0)
    ramp = torch.arange(n_floats, dtype=torch.float32, device="cuda") / 2 ** 20
    out = []
    for e in range(len(seq)):
        _, params = guarded_floats(n_floats, 0.0)
        params.copy_(ramp + (e + 1))
        ops.best_select(recs[e], block, criterion, e, params, best)
        w = whole.cpu()
        assert (w[:4] == -7.0).all() and (w[4 + n_floats:] == -7.0).all(), "guard words around best_params"
        out.append((ops.decode_best_block(block), best.cpu().clone()))
    return out, ramp.cpu()


@pytest.mark.parametrize("criterion", ["accuracy", "nll"])
@pytest.mark.parametrize("name,seq,want_acc,want_nll", ref.SEQUENCES, ids=[s[0] for s in ref.SEQUENCES])
def test_best_select_sequences(name, seq, want_acc, want_nll, criterion):
    n = 257
    steps = ref.select([{"correct": c, "nll_sum": v} for c, v in seq], criterion)
    got, ramp = run_sequence(seq, criterion, n)
    for e, ((blk, best), (be, bc, bn, better)) in enumerate(zip(got, steps)):
        assert blk["best_epoch"] == be and blk["epochs_seen"] == e + 1
        if be >= 0:
            assert blk["best_correct"] == bc and (blk["best_nll_sum"] == bn or (np.isnan(bn) and np.isnan(blk["best_nll_sum"])))
            assert torch.equal(best, ramp + (be + 1)), "best_params is not the picked epoch's params"
        else:
            assert (best == -7.0).all(), "best_params written without a better epoch"
    assert got[-1][0]["best_epoch"] == (want_acc if criterion == "accuracy" else want_nll)


@pytest.mark.parametrize("n_floats", [1, 255, 257, 1000, 1024 * 256 + 77])
def test_best_select_sizes(n_floats):
    """Exactly n_floats floats are written, by one short workgroup, by several, and by the grid-stride loop beyond the launch's grid."""
    got, ramp = run_sequence([(3, 9.0), (5, 7.0), (4, 8.0)], "accuracy", n_floats)
    assert [g[0]["best_epoch"] for g in got] == [0, 1, 1]
    assert torch.equal(got[0][1], ramp + 1) and torch.equal(got[1][1], ramp + 2) and torch.equal(got[2][1], ramp + 2)


def test_best_select_refusals_on_the_device():
    L = _lib.lib
    rec = ops.new_val_records(1, 10, "cuda")[0]
    blk = ops.new_best_block("cuda")
    p = torch.zeros(16, device="cuda")
    b = torch.zeros(16, device="cuda")
    ws = torch.zeros(256, dtype=torch.uint8, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    call = lambda **k: L.clipmi_best_select(k.get("rec", rec.data_ptr()), blk.data_ptr(), k.get("crit", 0), k.get("epoch", 0), k.get("p", p.data_ptr()),
                                            k.get("b", b.data_ptr()), k.get("n", 8), ws.data_ptr(), k.get("wsb", 256), s)
    assert call(rec=None) == _lib.ERR_ARG and call(b=None) == _lib.ERR_ARG
    assert call(p=p.data_ptr() + 4) == _lib.ERR_ARG and call(b=b.data_ptr() + 8) == _lib.ERR_ARG
    assert call(crit=2) == _lib.ERR_ARG and call(epoch=-1) == _lib.ERR_ARG
    assert call(n=0) == _lib.ERR_SHAPE and call(wsb=0) == _lib.ERR_WORKSPACE
    z = torch.zeros(4, 8, device="cuda")
    yl = torch.zeros(4, dtype=torch.int64, device="cuda")
    score = lambda **k: L.clipmi_val_score(k.get("z", z.data_ptr()), k.get("ld", 8), yl.data_ptr(), k.get("N", 4), k.get("C", 8), k.get("bins", 10),
                                           rec.data_ptr(), ws.data_ptr(), k.get("wsb", 256), s)
    assert score(z=z.data_ptr() + 4) == _lib.ERR_ARG and score(bins=0) == _lib.ERR_ARG and score(bins=65) == _lib.ERR_ARG
    assert score(N=0) == _lib.ERR_SHAPE and score(C=0) == _lib.ERR_SHAPE and score(ld=7) == _lib.ERR_SHAPE and score(wsb=0) == _lib.ERR_WORKSPACE
    torch.cuda.synchronize()
    assert ops.decode_best_block(blk)["epochs_seen"] == 0 and float(b.abs().sum()) == 0.0       # nothing was launched
    assert call() == _lib.OK and score() == _lib.OK
