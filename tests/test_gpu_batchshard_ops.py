"""clipmi_block_rank_mean and clipmi_block_step_gathered (clip_calibration_amd/csrc/shard_train.hip) on the GPU, bit for bit against
tests/batchshard_ref.py: every total at which the kernel changes path (fewer floats than a vector, a vector with and without head and
tail, one workgroup and the floats either side of it, more than one), packed and padded rank strides, non-finite values at every seam,
the order of the ranks, and every refusal of the C entry point."""
import numpy as np
import pytest
import torch

import batchshard_ref as ref
import blockscaler_ref as bref

pytestmark = pytest.mark.gpu

from clip_calibration_amd import _lib, ops, vptfit  # noqa: E402

lib = _lib.lib
TOTALS = (1, 3, 4, 5, 255, 256, 257, 1000, 1027)
WORLDS = (1, 2, 3, 8)


def values(G, width, seed):
    """fp32 [G, width]: normal draws, and among them exact zeros, a denormal and the magnitudes 1e-8 and 1e4."""
    rng = np.random.RandomState(seed)
    g = rng.standard_normal((G, width)).astype(np.float32)
    special = np.array([0.0, -0.0, 1e-40, 1e-8, -1e-8, 1e4, -1e4], np.float32)
    for r in range(G):
        at = rng.randint(0, width, size=min(width, len(special)))
        g[r, at] = special[:len(at)]
    return g


def seams(total):
    """Element 0, the last one, and both sides of every vector seam near the ends and of the workgroup seams at 256 floats and 256 vectors."""
    return sorted({i for i in (0, 1, 3, 4, 5, 7, 8, 255, 256, 257, 1023, 1024, total - 5, total - 4, total - 2, total - 1) if 0 <= i < total})


def device_mean(gathered, total):
    return ops.block_rank_mean(torch.from_numpy(gathered).cuda(), total).cpu().numpy()


@pytest.mark.parametrize("G", WORLDS)
@pytest.mark.parametrize("total", TOTALS)
def test_rank_mean_is_the_restatement_bit_for_bit(total, G):
    """``stride == total`` (for most totals no multiple of four: the scalar path) and ``stride = total + 3`` with the padding NaN, which
    must not be read; a 16-byte-aligned stride (the vector path) is the next case's."""
    g = values(G, total, 100 * G + total)
    want = ref.rank_mean(g)
    assert ref.same_bits(device_mean(g, total), want)
    wide = np.full((G, total + 3), np.nan, np.float32)
    wide[:, :total] = g
    got = device_mean(wide, total)
    assert not np.isnan(got).any() and ref.same_bits(got, want)
    if G == 1:
        assert got.tobytes() == g[0].tobytes()                          # x * 1.0f: the input itself


@pytest.mark.parametrize("G", WORLDS)
@pytest.mark.parametrize("total", TOTALS)
def test_vector_path_with_heads_tails_and_offsets(total, G):
    """A stride that is a multiple of four floats, NaN in its padding, and the block started 0 .. 3 floats behind a 16-byte boundary
    (``out`` on the same phase or on another one: the vector path with a head, or the scalar path): the same bits every time."""
    stride = (total + 3) // 4 * 4 + 4
    g = values(G, total, 7 * G + total)
    want = ref.rank_mean(g)
    for off in range(4):
        flat = torch.full((G * stride + 8,), float("nan")).cuda()
        rows = flat[off:off + G * stride].view(G, stride)
        rows[:, :total] = torch.from_numpy(g).cuda()
        for out_off in (off, (off + 1) % 4):
            out = torch.full((total + 8,), 7.0).cuda()
            ops.block_rank_mean(rows, total, out[out_off:out_off + total])
            got = out.cpu().numpy()
            assert ref.same_bits(got[out_off:out_off + total], want), (off, out_off)
            assert (got[:out_off] == 7.0).all() and (got[out_off + total:] == 7.0).all(), (off, out_off)     # nothing written outside


@pytest.mark.parametrize("total", (5, 257, 1027))
def test_inf_and_nan_propagate_to_exactly_their_elements(total):
    G, stride = 3, (total + 3) // 4 * 4
    base = values(G, total, total)
    for bad in (np.inf, -np.inf, np.nan):
        for aligned in (True, False):
            g = np.zeros((G, stride if aligned else total), np.float32)
            g[:, :total] = base
            at = seams(total)
            g[1, at] = bad
            got = device_mean(g, total)
            hit = np.zeros(total, bool)
            hit[at] = True
            assert np.array_equal(~np.isfinite(got), hit), (bad, aligned)
            assert ref.same_bits(got, ref.rank_mean(g, total)), (bad, aligned)


def test_the_rank_order_shows():
    g = np.zeros((3, 9), np.float32)
    g[:, 4] = ref.ORDER_TRIPLE
    got, back = device_mean(g, 9), device_mean(g[::-1].copy(), 9)
    assert got[4] == np.float32(1.0) * np.float32(1.0 / 3) and back[4] == 0.0
    assert ref.same_bits(got, ref.rank_mean(g)) and ref.same_bits(back, ref.rank_mean(g[::-1]))


def test_every_refusal_precedes_the_launch():
    G, total = 2, 8
    src = torch.zeros(G, total).cuda()
    out = torch.full((total,), 5.0).cuda()
    st = ops._stream()
    bad = [((None, G, total, total, out.data_ptr()), _lib.ERR_ARG), ((src.data_ptr(), G, total, total, None), _lib.ERR_ARG),
           ((src.data_ptr() + 2, G, total, total - 1, out.data_ptr()), _lib.ERR_ARG), ((src.data_ptr(), G, total, total, out.data_ptr() + 1), _lib.ERR_ARG),
           ((src.data_ptr(), 0, total, total, out.data_ptr()), _lib.ERR_SHAPE), ((src.data_ptr(), -1, total, total, out.data_ptr()), _lib.ERR_SHAPE),
           ((src.data_ptr(), G, total, 0, out.data_ptr()), _lib.ERR_SHAPE), ((src.data_ptr(), 1, 2 ** 39, 2 ** 39, out.data_ptr()), _lib.ERR_SHAPE),
           ((src.data_ptr(), G, total - 1, total, out.data_ptr()), _lib.ERR_SHAPE),
           ((src.data_ptr(), G, total, total, src.data_ptr() + 4 * total), _lib.ERR_ARG),            # out is rank 1's block
           ((src.data_ptr(), G, total, total, src.data_ptr() + 4 * (2 * total - 1)), _lib.ERR_ARG)]  # out begins on the last float
    for args, rc in bad:
        assert lib.clipmi_block_rank_mean(*args, st) == rc, (args, _lib.last_error())
    torch.cuda.synchronize()
    assert (out == 5.0).all() and (src == 0.0).all()
    with pytest.raises(ValueError, match="total=9"):
        ops.block_rank_mean(src, 9)
    with pytest.raises(TypeError, match="unit element stride"):
        ops.block_rank_mean(src.t(), 2)
    with pytest.raises(TypeError, match="fp32"):
        ops.block_rank_mean(src.double(), 2)
    with pytest.raises(_lib.ClipmiError, match="overlaps"):
        ops.block_rank_mean(src, total, src.view(-1)[total:])
    assert lib.clipmi_block_step_gathered(src.data_ptr(), G, total, total, 0.0, out.data_ptr(), None, None, out.data_ptr(), 1, 0.0, 0.0, 0.0, 0, st) == _lib.ERR_ARG
    assert lib.clipmi_block_step_gathered(src.data_ptr(), G, total, total, 1.0, None, None, None, None, 1, 0.0, 0.0, 0.0, 0, st) == _lib.ERR_ARG
    assert lib.clipmi_block_step_gathered(src.data_ptr(), G, total, total, 1.0, src.data_ptr() + 4, None, None, out.data_ptr(), 1, 0.0, 0.0, 0.0, 0,
                                          st) == _lib.ERR_ARG


@pytest.mark.parametrize("G", (1, 2, 8))
@pytest.mark.parametrize("momentum,nesterov", [(0.0, False), (0.5, False), (0.5, True)])
def test_gathered_step_on_exact_inputs_is_the_block_scaler_reference(G, momentum, nesterov):
    """The fused step against the restatement of the mean followed by tests/blockscaler_ref.py's SGD (its rule divides by the scale and
    steps; the scale never moves here), two steps: the first starts the buffer, the second uses it.  That reference holds for inputs
    that keep every product exact (it asserts so), so the momentum and the world size are powers of two; the next test takes 0.9 and
    three ranks."""
    total, gs, lr = 1027, 256.0, 2.0 ** -3
    params0, ints = bref.exact_block(total, 2 * G, seed=G)
    r = bref.BlockRef(params0, gs, growth_interval=10 ** 6, momentum=momentum, nesterov=nesterov)
    p = torch.from_numpy(params0.copy()).cuda()
    b = torch.zeros(total).cuda() if momentum else None
    lr_d = torch.tensor([lr]).cuda()
    for k in range(2):
        g = np.stack([bref.scaled(ints[k * G + i], gs) for i in range(G)])
        grad = ops.block_step_gathered(torch.from_numpy(g).cuda(), total, gs, p, b, lr_d, k == 0, momentum, 0.0, 0.0, nesterov)
        assert not r.step(ref.rank_mean(g), lr)
        assert ref.same_bits(grad.cpu().numpy(), r.grad.reshape(-1)) and ref.same_bits(p.cpu().numpy(), r.params), k
        if momentum:
            assert ref.same_bits(b.cpu().numpy(), r.momentum_buffer), k


@pytest.mark.parametrize("G", WORLDS)
@pytest.mark.parametrize("momentum,nesterov,wd", [(0.0, False, 5e-4), (0.9, False, 5e-4), (0.9, True, 0.0)])
def test_gathered_step_is_the_mean_followed_by_the_block_step(G, momentum, nesterov, wd):
    """Inexact inputs, momentum 0.9 and a weight decay: the gradient is the restatement's mean times ``float32(1 / grad_scale)`` bit
    for bit, and parameters and buffer are those of clipmi_vpt_step -- the unsharded static step, held to torch.optim.SGD by its own
    tests -- given the restated mean as its scale * gradient.  ``first_step`` on, then off."""
    total, gs = 1027, 1024.0
    rng = np.random.RandomState(G)
    p0 = rng.standard_normal(total).astype(np.float32)
    pa, pb = torch.from_numpy(p0.copy()).cuda(), torch.from_numpy(p0.copy()).cuda()
    ba, bb = (torch.zeros(total).cuda(), torch.zeros(total).cuda()) if momentum else (None, None)
    lr_d = torch.tensor([0.0035]).cuda()
    for first in (True, False):
        g = (gs * values(G, total + 3, 31 * G + first)).astype(np.float32)
        mean = ref.rank_mean(g, total)
        grad = ops.block_step_gathered(torch.from_numpy(g).cuda(), total, gs, pa, ba, lr_d, first, momentum, 0.0, wd, nesterov)
        assert ref.same_bits(grad.cpu().numpy(), (mean * np.float32(1.0 / gs)).astype(np.float32))
        vptfit.vpt_step(torch.from_numpy(mean).cuda().view(1, 1, total), gs, pb.view(1, 1, total), None if bb is None else bb.view(1, 1, total), lr_d, first,
                        momentum, 0.0, wd, nesterov, want_grad=False)
        assert torch.equal(pa, pb) and (ba is None or torch.equal(ba, bb)), first
    assert not np.array_equal(pa.cpu().numpy(), p0)
