"""The PTS entry points of csrc/pts.hip at C ABI level against tests/pts_ref.py: the selection bit for bit, the apply's division bit for
bit, one batch's loss and gradient and a whole fit under the project's FACTOR rule (tests/test_gpu_attention_backward_full.py): the device's
error against the float64 restatement may be FACTOR x the error of the fp32 CPU yardstick on the same inputs, plus one fp32 ulp of the
tensor's largest magnitude.  Every measured ratio is printed on a line that starts with "pts-parity:"; profiles/ptsfit_parity.txt is one
run's lines."""
import functools

import numpy as np
import pytest
import torch

import pts_ref as ref

pytestmark = pytest.mark.gpu

from clip_calibration_amd import _lib, ops  # noqa: E402

FACTOR = 2.0
DEFAULT = (2, 5, 10)
NETS = [DEFAULT, (0, 32, 10), (4, 32, 10)]
EVAL_SHAPES = [(1, 10), (5, 65), (7, 129), (33, 1000)]
# no hidden pre-activation of the float64 run may lie within MARGIN of zero, and no |t| below 1e-3: a ReLU that flips between two precisions
# is another function, not an error.  The seeds of eval_case meet this for every shape and net (checked on the CPU, asserted there).
MARGIN = 1e-4


def say(line):
    print("pts-parity: " + line)


def cuda(a):
    return torch.from_numpy(np.array(a)).cuda()


@functools.lru_cache(maxsize=None)
def eval_case(N, C, net):
    """(block, z, y, float64 (loss, grad), fp32 CPU yardstick (loss, grad, T), float64 t), computed once; zero rows are excluded."""
    L, n, K = net
    z, y = ref.make_case(N, C, 100)
    block = ref.make_params(L, n, K, 200)
    loss, grad, margin, t = ref.autograd(block, z, y, L, n, K)
    assert margin > MARGIN and float(np.abs(t).min()) > 1e-3, (margin, float(np.abs(t).min()))
    for a in (z, y, grad, t):
        a.setflags(write=False)
    return block, z, y, (loss, grad), ref.hand(block, z, y, L, n, K, torch.float32), t


# ---- top-k -----------------------------------------------------------------------------------------------------------------------------
def raw_topk(zt, K):
    """clipmi_pts_topk into a NaN-prefilled region with canaries on both sides; returns the [N, K] region."""
    N, C = zt.shape
    buf = torch.full((N * K + 128,), 12345.0, dtype=torch.float32).cuda()
    buf[64:64 + N * K] = float("nan")
    _lib.check(_lib.lib.clipmi_pts_topk(zt.data_ptr(), zt.stride(0), N, C, K, buf[64:].data_ptr(), torch.cuda.current_stream().cuda_stream),
               "clipmi_pts_topk")
    torch.cuda.synchronize()
    assert bool((buf[:64] == 12345.0).all()) and bool((buf[64 + N * K:] == 12345.0).all())
    return buf[64:64 + N * K].view(N, K).clone()


def topk_input(N, C, variant, seed):
    rng = np.random.default_rng(seed)
    z = (30 * rng.uniform(-1, 1, (N, C))).astype(np.float32)
    if variant == "duplicates":            # the maximum several times over, and few distinct values at all
        z = np.round(z / 10).astype(np.float32) * 10 + np.float32(0.0)     # + 0.0: no -0.0, whose order beside +0.0 no sort defines
        z[:, rng.integers(0, C, 3)] = z.max()
    elif variant == "neg_inf":
        z[:, rng.permutation(C)[:max(1, C // 2)]] = -np.inf
        z[0, :] = -np.inf                   # a whole row of them
    return z


@pytest.mark.parametrize("K", [1, 10, 32])
@pytest.mark.parametrize("variant", ["plain", "wide", "duplicates", "neg_inf"])
def test_topk_is_sorts_first_columns_bit_for_bit(K, variant):
    """C in {K, K + 1, 63, 64, 65, 129, 1000} (the wave's seams) x N in {1, 4, 5} (the workgroup's): the values equal torch.sort's first K
    columns bit for bit, out of a wider matrix too, with the maximum repeated and with -inf entries; nothing is written outside [N, K]
    and nothing inside is left unwritten; two runs give the same bits."""
    for C in sorted({max(K, 2), max(K, 2) + 1, 63, 64, 65, 129, 1000}):
        if C < K:
            continue
        for N in (1, 4, 5):
            z = topk_input(N, C, variant, 7 * C + N)
            if variant == "wide":
                buf = torch.full((N, C + 13), 1e30, dtype=torch.float32).cuda()      # what lies behind a row would win every round
                buf[:, :C] = cuda(z)
                zt = buf[:, :C]
                assert zt.stride(0) == C + 13
            else:
                zt = cuda(z)
            got = raw_topk(zt, K)
            want = torch.sort(zt, dim=1, descending=True).values[:, :K]
            assert torch.equal(got.view(torch.int32), want.contiguous().view(torch.int32)), (C, N)
            assert torch.equal(raw_topk(zt, K).view(torch.int32), got.view(torch.int32))
            assert torch.equal(ops.pts_topk(zt, K).view(torch.int32), got.view(torch.int32))


def test_topk_nan_row_and_empty_input():
    z = topk_input(5, 129, "plain", 3)
    z[2, 77] = np.nan
    got = raw_topk(cuda(z), 10)
    want = torch.sort(cuda(z), dim=1, descending=True).values[:, :10]
    assert bool(got[2].isnan().all())
    keep = [0, 1, 3, 4]
    assert torch.equal(got[keep], want[keep])
    assert ops.pts_topk(torch.empty(0, 20, dtype=torch.float32).cuda(), 10).shape == (0, 10)


# ---- apply -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("net", NETS, ids=str)
@pytest.mark.parametrize("N,C", EVAL_SHAPES)
def test_apply_divides_by_the_rows_temperature(N, C, net):
    """out[i, c] is fp32 z[i, c] / T_i bit for bit with the T the call reports, in place and out of place alike, out of and into wider
    matrices; T against the float64 restatement under the FACTOR rule."""
    L, n, K = net
    block, z, y, _, (_, _, T32), t64 = eval_case(N, C, net)
    wide = torch.full((N, C + 5), 7.0, dtype=torch.float32).cuda()
    wide[:, :C] = cuda(z)
    zt, pt = wide[:, :C], block.cuda()
    out, T = ops.pts_apply(zt, pt, L, n, K, want_temperature=True)
    assert torch.equal(out.view(torch.int32), (zt / T[:, None]).contiguous().view(torch.int32))
    e_dev, e_yard, bound = ref.held(T.cpu().numpy(), T32, np.abs(t64))
    say(f"apply T {(N, C)} net {net}: device err {e_dev:.3e}, fp32 CPU err {e_yard:.3e}, bound {bound:.3e}")
    assert e_dev <= bound
    same = ops.pts_apply(zt, pt, L, n, K, out=zt)
    assert same.data_ptr() == zt.data_ptr() and torch.equal(zt.contiguous().view(torch.int32), out.view(torch.int32))
    assert bool((wide[:, C:] == 7.0).all())
    assert ops.pts_apply(torch.empty(0, C, dtype=torch.float32).cuda(), pt, L, n, K).shape == (0, C)


def test_apply_clamps_t_zero_to_the_lower_bound():
    L, n, K = DEFAULT
    z, _ = ref.make_case(3, 12, 0)
    block = ref.make_params(L, n, K, 0)
    p = ref.split(block, L, n, K)
    p["w_out"].zero_()
    p["b_out"].zero_()
    out, T = ops.pts_apply(cuda(z), block.cuda(), L, n, K, want_temperature=True)
    assert bool((T == torch.tensor(1e-12, dtype=torch.float32)).all())
    assert torch.equal(out.cpu(), torch.from_numpy(z) / torch.tensor(1e-12, dtype=torch.float32))


# ---- eval ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("net", NETS, ids=str)
@pytest.mark.parametrize("N,C", EVAL_SHAPES)
def test_eval_loss_and_gradients_under_the_factor_rule(N, C, net):
    L, n, K = net
    block, z, y, (loss64, grad64), (loss32, grad32, _), _ = eval_case(N, C, net)
    zt, yt, pt = cuda(z), cuda(y), block.cuda()
    feat = ops.pts_topk(zt, K)
    got = ops.pts_eval(feat, zt, yt, pt, L, n, K).cpu().numpy().astype(np.float64)
    assert np.isfinite(got).all()
    e_dev, e_yard, bound = ref.held(got[:1], [loss32], [loss64])
    say(f"eval {(N, C)} net {net} loss: device err {e_dev:.3e}, fp32 CPU err {e_yard:.3e}, ratio to bound {e_dev / bound:.3f}")
    assert e_dev <= bound
    dev, yard, want = (ref.split(g, L, n, K) for g in (got[1:], grad32, grad64))
    for name, _ in ref.shapes(L, n, K):
        e_dev, e_yard, bound = ref.held(dev[name], yard[name], want[name])
        say(f"eval {(N, C)} net {net} d{name}: device err {e_dev:.3e}, fp32 CPU err {e_yard:.3e}, ratio to bound {e_dev / bound:.3f}")
        assert e_dev <= bound, name
    again = ops.pts_eval(feat, zt, yt, pt, L, n, K)
    assert torch.equal(again.view(torch.int32), torch.from_numpy(got.astype(np.float32)).cuda().view(torch.int32))


def test_eval_takes_a_row_selection_and_a_range():
    L, n, K = DEFAULT
    block, z, y, _, _, _ = eval_case(7, 129, DEFAULT)
    zt, yt, pt = cuda(z), cuda(y), block.cuda()
    feat = ops.pts_topk(zt, K)
    rows = np.array([6, 0, 3, 3], np.int32)
    got = ops.pts_eval(feat, zt, yt, pt, L, n, K, rows=cuda(rows)).cpu().numpy().astype(np.float64)
    loss64, grad64, _, _ = ref.autograd(block, z[rows], y[rows], L, n, K)
    loss32, grad32, _ = ref.hand(block, z[rows], y[rows], L, n, K, torch.float32)
    for d, yd, w in [(got[:1], [loss32], [loss64]), (got[1:], grad32, grad64)]:
        e_dev, _, bound = ref.held(d, yd, w)
        assert e_dev <= bound
    part = ops.pts_eval(feat, zt, yt, pt, L, n, K, first=2, n_rows=3)
    same = ops.pts_eval(feat, zt, yt, pt, L, n, K, rows=cuda(np.array([2, 3, 4], np.int32)))
    assert torch.equal(part.view(torch.int32), same.view(torch.int32))


# ---- fit -------------------------------------------------------------------------------------------------------------------------------
SCHED = [0.01, 0.05, 0.02]
FIT_CASES = [(7, 37, 3, False, False), (7, 37, 3, True, False), (64, 65, 100, False, False), (64, 65, 24, False, True)]


def _order(N, epochs=3, seed=5):
    rng = np.random.default_rng(seed)
    return np.stack([rng.permutation(N) for _ in range(epochs)]).astype(np.int32)


@functools.lru_cache(maxsize=None)
def fit_case(N, C, batch, drop_last, ordered, optimizer):
    L, n, K = DEFAULT
    z, y = ref.make_case(N, C, 31 + N)
    block = ref.make_params(L, n, K, 41 + N)
    kw = dict(optimizer=optimizer, drop_last=drop_last, order=_order(N) if ordered else None)
    return block, z, y, kw, ref.torch_fit(block, z, y, L, n, K, SCHED, batch, torch.float64, **kw), ref.torch_fit(block, z, y, L, n, K, SCHED, batch,
                                                                                                                  torch.float32, **kw)


def device_fit(block, z, y, batch, kw, epochs=3, state=None, lr=None, order=None):
    L, n, K = DEFAULT
    N = z.shape[0]
    P = ref.count(L, n, K)
    per_epoch = N // batch if kw["drop_last"] else -(-N // batch)
    if state is None:
        state = torch.zeros(3 * P + 2, dtype=torch.float32).cuda()
        state[:P] = block.cuda()
    if lr is None:
        lr = torch.from_numpy(np.repeat(np.asarray(SCHED[:epochs], np.float32), per_epoch)).cuda()
    if order is None and kw["order"] is not None:
        order = cuda(kw["order"][:epochs])
    losses = ops.pts_fit(cuda(z), cuda(y), state, L, n, K, lr, batch, epochs, _lib.OPTIM_SGD if kw["optimizer"] == "sgd" else _lib.OPTIM_ADAM,
                         momentum=0.9, weight_decay=5e-4, order=order, drop_last=kw["drop_last"], want_losses=True)
    return state, losses


@pytest.mark.parametrize("optimizer", ["sgd", "adam"])
@pytest.mark.parametrize("N,C,batch,drop_last,ordered", FIT_CASES)
def test_fit_is_the_float64_loop_within_torchs_own_fp32_distance(N, C, batch, drop_last, ordered, optimizer):
    """Three epochs (batches of 3 over 7 rows with and without the short one, one short batch of 64, an explicit order) with both
    optimisers: per-step losses and every final parameter tensor against torch.optim's float64 loop, the yardstick torch's own fp32 CPU
    loop.  Two runs give identical bits, a run continued from its state equals the uninterrupted one, and no epochs return the start."""
    L, n, K = DEFAULT
    P = ref.count(L, n, K)
    block, z, y, kw, (loss64, final64), (loss32, final32) = fit_case(N, C, batch, drop_last, ordered, optimizer)
    state, losses = device_fit(block, z, y, batch, kw)
    steps = len(loss64)
    assert losses.shape == (steps,) and int(state.view(torch.int32)[3 * P]) == steps and float(state[3 * P + 1]) == float(losses[-1])
    e_dev, e_yard, bound = ref.held(losses.cpu().numpy(), loss32, loss64, FACTOR)
    say(f"fit {optimizer} {(N, C, batch)} drop_last={drop_last} order={ordered} losses: device err {e_dev:.3e}, torch fp32 err {e_yard:.3e}, "
        f"ratio to bound {e_dev / bound:.3f}")
    assert e_dev <= bound
    dev, yard, want = (ref.split(b, L, n, K) for b in (state[:P].cpu().numpy().astype(np.float64), final32, final64))
    for name, _ in ref.shapes(L, n, K):
        e_dev, e_yard, bound = ref.held(dev[name], yard[name], want[name], FACTOR)
        say(f"fit {optimizer} {(N, C, batch)} drop_last={drop_last} order={ordered} {name}: device err {e_dev:.3e}, torch fp32 err {e_yard:.3e}, "
            f"ratio to bound {e_dev / bound:.3f}")
        assert e_dev <= bound, name
    assert float(np.abs(final64 - block.numpy()).max()) > 1e-4                     # the run moved the parameters
    state2, losses2 = device_fit(block, z, y, batch, kw)
    assert torch.equal(state.view(torch.int32), state2.view(torch.int32)) and torch.equal(losses.view(torch.int32), losses2.view(torch.int32))
    per_epoch = steps // 3
    part, first = device_fit(block, z, y, batch, kw, epochs=1)
    lr_rest = torch.from_numpy(np.repeat(np.asarray(SCHED[1:], np.float32), per_epoch)).cuda()
    _, rest = device_fit(block, z, y, batch, kw, epochs=2, state=part, lr=lr_rest, order=None if kw["order"] is None else cuda(kw["order"][1:]))
    assert torch.equal(part.view(torch.int32), state.view(torch.int32))
    assert torch.equal(torch.cat([first, rest]).view(torch.int32), losses.view(torch.int32))
    start = torch.zeros(3 * P + 2, dtype=torch.float32).cuda()
    start[:P] = block.cuda()
    none = ops.pts_fit(cuda(z), cuda(y), start, L, n, K, torch.empty(0, dtype=torch.float32).cuda(), batch, 0, want_losses=True)
    assert none.shape == (0,) and torch.equal(start[:P].cpu(), block) and not bool(start[P:].any())


def test_fit_poisons_the_parameters_on_a_label_out_of_range():
    """The C entry point, past the host's check: a label outside [0, C) is not used as an address, the loss and the parameters are NaN."""
    L, n, K = DEFAULT
    P = ref.count(L, n, K)
    z, y = ref.make_case(7, 37, 2)
    y = y.copy()
    y[4] = 37
    state = torch.zeros(3 * P + 2, dtype=torch.float32).cuda()
    state[:P] = ref.make_params(L, n, K, 3).cuda()
    lr = torch.full((1,), 0.01, dtype=torch.float32).cuda()
    losses = ops.pts_fit(cuda(z), cuda(y), state, L, n, K, lr, 7, 1, want_losses=True)
    assert bool(losses.isnan().all()) and bool(state[:P].isnan().any())


def test_refusals_on_the_device():
    L, n, K = DEFAULT
    z, y = ref.make_case(4, 20, 0)
    zt, yt, pt = cuda(z), cuda(y), ref.make_params(L, n, K, 0).cuda()
    with pytest.raises(ValueError):
        ops.pts_topk(zt[:, :8], 10)                        # C < K
    with pytest.raises(ValueError):
        ops.pts_topk(zt, 33)
    with pytest.raises(ValueError):
        ops.pts_apply(zt, pt[:-1], L, n, K)
    with pytest.raises(ValueError):
        ops.pts_apply(zt, pt, 5, n, K)
    with pytest.raises(TypeError):
        ops.pts_apply(zt.double(), pt, L, n, K)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.pts_apply(zt.cpu(), pt, L, n, K)
    with pytest.raises(ValueError):
        ops.pts_eval(ops.pts_topk(zt, K)[:, :5], zt, yt, pt, L, n, K)
    with pytest.raises(ValueError):
        ops.pts_eval(ops.pts_topk(zt, K), zt, yt, pt, L, n, K, first=3, n_rows=2)
    with pytest.raises(ValueError):
        ops.pts_fit(zt, yt, torch.zeros(10, dtype=torch.float32).cuda(), L, n, K, torch.zeros(2, dtype=torch.float32).cuda(), 2, 1)
    rc = _lib.lib.clipmi_pts_apply(zt.data_ptr(), 20, 4, 20, None, L, n, K, zt.data_ptr(), 20, None, None)
    assert rc == _lib.ERR_ARG and "null pointer" in _lib.last_error()
