"""Parameterized temperature scaling without a GPU: the hand-written forward and backward of tests/pts_ref.py (the kernels' formulas)
against float64 autograd, the parameter block's helpers, fit_pts' refusals, and the C ABI's surface."""
import ctypes
import re

import numpy as np
import pytest
import torch

import pts_ref as ref
from clip_calibration_amd import _lib, ptsfit


def _case(L, n, K, N, C, seed, edit=None):
    z, y = ref.make_case(N, C, seed)
    block = ref.make_params(L, n, K, seed + 1)
    if edit is not None:
        edit(ref.split(block, L, n, K))
    return block, z, y


def _negative_t(p):
    p["w_out"].mul_(-1.0)
    p["b_out"].fill_(-1.5)


def _dead_unit(p):
    p["W1"][2].fill_(0.0)
    p["b1"][2] = -3.0          # unit 2 of layer 1 is off in every row


CASES = [("default", 2, 5, 10, 9, 37, 3, None), ("t<0", 2, 5, 10, 6, 23, 5, _negative_t), ("no hidden layer", 0, 5, 10, 7, 12, 7, None),
         ("dead unit", 2, 5, 10, 8, 65, 9, _dead_unit), ("deep and wide", 4, 32, 32, 5, 40, 11, None), ("K=1", 1, 3, 1, 4, 2, 13, None)]


@pytest.mark.parametrize("name,L,n,K,N,C,seed,edit", CASES, ids=[c[0] for c in CASES])
def test_hand_written_gradient_is_float64_autograd(name, L, n, K, N, C, seed, edit):
    """The kernels' formulas (label term apart, shift by the row maximum, sign and clamp conventions, relu' (0) = 0), evaluated in float64,
    against torch autograd on the definition: loss and every parameter tensor's gradient to 1e-12 of the tensor's largest magnitude."""
    block, z, y = _case(L, n, K, N, C, seed, edit)
    loss, grad, margin, t = ref.autograd(block, z, y, L, n, K)
    h_loss, h_grad, h_T = ref.hand(block, z, y, L, n, K, torch.float64)
    assert margin > 1e-6
    if name == "t<0":
        assert (t < 0).all()
    if name == "dead unit":
        assert not ref.split(grad, L, n, K)["W1"][2].any() and ref.split(grad, L, n, K)["W1"].any()
    assert abs(h_loss - loss) <= 1e-12 * abs(loss)
    np.testing.assert_allclose(h_T, np.clip(np.abs(t), 1e-12, 1e12), rtol=1e-14)
    want, got = ref.split(grad, L, n, K), ref.split(h_grad, L, n, K)
    for name_, _ in ref.shapes(L, n, K):
        scale = float(np.abs(want[name_]).max())
        assert scale > 0 or name_ in ("W1", "b1")
        assert float(np.abs(got[name_] - want[name_]).max()) <= 1e-12 * scale, name_


def test_gradient_conventions_at_the_kinks():
    """t == 0: T is the lower clamp and no gradient passes abs; |t| beyond the clamp: none passes either."""
    L, n, K = 1, 3, 4
    z, y = ref.make_case(3, 6, 1)
    block = ref.make_params(L, n, K, 2)
    p = ref.split(block, L, n, K)
    p["w_out"].zero_()
    p["b_out"].zero_()
    loss, grad, T = ref.hand(block, z, y, L, n, K, torch.float64)
    assert (T == 1e-12).all() and not grad.any()
    a_loss, a_grad, _, _ = ref.autograd(block, z, y, L, n, K)
    assert not a_grad.any() and abs(a_loss - loss) <= 1e-12
    p["b_out"].fill_(3e12)
    _, grad, T = ref.hand(block, z, y, L, n, K, torch.float64)
    assert (T == 1e12).all() and not grad.any()


def test_block_helpers_agree():
    g = torch.Generator().manual_seed(0)
    for L, n, K in [(2, 5, 10), (0, 7, 3), (4, 32, 32), (1, 1, 1)]:
        P = ptsfit.param_count(L, n, K)
        assert P == ref.count(L, n, K) == _lib.lib.clipmi_pts_param_count(L, n, K)
        block = ptsfit.init_params(L, n, K, generator=g)
        assert block.shape == (P,) and block.dtype == torch.float32 and not block.is_cuda
        views = ptsfit.split_params(block, L, n, K)
        assert [(k, tuple(v.shape)) for k, v in views.items()] == ref.shapes(L, n, K)
        assert sum(v.numel() for v in views.values()) == P
        assert views["b_out"].data_ptr() == block[P - 1:].data_ptr()       # views, in the block's order
        for name, v in views.items():
            fan_in = views["w_out" if name.endswith("out") else "W" + name[1:]].shape[-1]
            assert float(v.abs().max()) <= 1.0 / np.sqrt(fan_in)
        for name, v in ref.split(block, L, n, K).items():
            assert torch.equal(v, views[name])
    assert ptsfit.param_count() == 10 * 5 + 5 + 5 * 5 + 5 + 5 + 1
    a = ptsfit.init_params(generator=torch.Generator().manual_seed(4))
    assert torch.equal(a, ptsfit.init_params(generator=torch.Generator().manual_seed(4)))
    for bad in [(5, 5, 10), (-1, 5, 10), (2, 33, 10), (2, 0, 10), (2, 5, 33), (2, 5, 0)]:
        assert _lib.lib.clipmi_pts_param_count(*bad) == 0
        with pytest.raises(ValueError):
            ptsfit.param_count(*bad)
        with pytest.raises(ValueError):
            ptsfit.init_params(*bad)
    with pytest.raises(ValueError):
        ptsfit.split_params(torch.zeros(5), 2, 5, 10)


def test_fit_pts_refusals_need_no_gpu():
    z, y = ref.make_case(12, 20, 0)
    zt = torch.from_numpy(z)
    with pytest.raises(ValueError, match="top_k"):
        ptsfit.fit_pts(zt[:, :8], y)                                    # C < K
    bad = zt.clone()
    bad[3, 4] = float("nan")
    with pytest.raises(ValueError, match="NaN"):
        ptsfit.fit_pts(bad, y)
    bad[3, 4] = float("inf")
    with pytest.raises(ValueError, match="infinity"):
        ptsfit.fit_pts(bad, y)
    with pytest.raises(ValueError, match="labels"):
        ptsfit.fit_pts(zt, np.where(np.arange(12) == 5, 20, y))
    with pytest.raises(ValueError, match="labels"):
        ptsfit.fit_pts(zt, y[:-1])
    with pytest.raises(TypeError):
        ptsfit.fit_pts(zt, y.astype(np.float32))
    with pytest.raises(ValueError, match="order"):
        ptsfit.fit_pts(zt, y, epochs=2, order=np.zeros((3, 12), np.int64))
    with pytest.raises(ValueError, match="order"):
        ptsfit.fit_pts(zt, y, epochs=1, order=np.full((1, 12), 12, np.int64))
    with pytest.raises(ValueError, match="optimizer"):
        ptsfit.fit_pts(zt, y, optimizer="lbfgs")
    with pytest.raises(ValueError, match="n_layers"):
        ptsfit.fit_pts(zt, y, n_layers=5)
    with pytest.raises(ValueError, match="n_nodes"):
        ptsfit.fit_pts(zt, y, n_nodes=33)
    with pytest.raises(ValueError, match="top_k"):
        ptsfit.fit_pts(zt, y, top_k=0)
    with pytest.raises(ValueError, match="momentum"):
        ptsfit.fit_pts(zt, y, momentum=1.0)
    with pytest.raises(ValueError, match="betas"):
        ptsfit.fit_pts(zt, y, optimizer="adam", betas=(0.9, 1.0))
    with pytest.raises(ValueError, match="params"):
        ptsfit.fit_pts(zt, y, params=torch.zeros(7))
    with pytest.raises(ValueError, match="learning rates"):
        ptsfit.fit_pts(zt, y, epochs=3, lr_per_epoch=[0.1])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ptsfit.fit_pts(zt, y)                                           # everything else is in order: the path itself needs the GPU
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ptsfit.PTSCalibrator(ptsfit.init_params()).apply(zt)


PTS_EXPORTS = ["clipmi_pts_apply", "clipmi_pts_eval", "clipmi_pts_fit", "clipmi_pts_param_count", "clipmi_pts_topk"]


def test_header_and_binding_list_the_entry_points_and_the_abi_stays_16():
    header = re.sub(r"/\*.*?\*/", "", open(_lib.HEADER_PATH).read(), flags=re.S)
    assert sorted(set(re.findall(r"\b(clipmi_pts_[a-z0-9_]+)\s*\(", header))) == PTS_EXPORTS
    assert sorted(n for n in _lib.exported_symbols() if n.startswith("clipmi_pts_")) == PTS_EXPORTS
    for name in PTS_EXPORTS:
        assert hasattr(_lib.lib, name) and f"int {name}(" in header
    assert _lib.ABI_VERSION == 16 and _lib.lib.clipmi_abi_version() == 16 and "#define CLIPMI_ABI_VERSION 16" in header
    make = open(_lib.HEADER_PATH.replace("include/clipmi.h", "clip_calibration_amd/csrc/Makefile")).read()
    assert " pts.hip " in make


def test_c_abi_refusals_need_no_gpu():
    """Limits, shapes and null pointers are refused with the library's own message before anything reaches a device."""
    L = _lib.lib
    p = ctypes.c_void_p(4096)
    assert L.clipmi_pts_topk(p, 20, 4, 20, 33, p, None) == _lib.ERR_SHAPE and "K=33" in _lib.last_error()
    assert L.clipmi_pts_topk(p, 20, 4, 20, 0, p, None) == _lib.ERR_SHAPE
    assert L.clipmi_pts_topk(p, 8, 4, 8, 10, p, None) == _lib.ERR_SHAPE and "C=8 < K=10" in _lib.last_error()
    assert L.clipmi_pts_topk(p, 1, 4, 1, 1, p, None) == _lib.ERR_SHAPE and "C=1" in _lib.last_error()
    assert L.clipmi_pts_topk(p, 19, 4, 20, 10, p, None) == _lib.ERR_SHAPE and "ld=19" in _lib.last_error()
    assert L.clipmi_pts_topk(p, 20, -1, 20, 10, p, None) == _lib.ERR_SHAPE
    assert L.clipmi_pts_topk(None, 20, 4, 20, 10, p, None) == _lib.ERR_ARG and L.clipmi_pts_topk(p, 20, 4, 20, 10, None, None) == _lib.ERR_ARG
    assert L.clipmi_pts_topk(p, 20, 0, 20, 10, p, None) == _lib.OK                                     # no rows: nothing to do

    def apply(logits=p, ld=20, N=4, C=20, params=p, nl=2, nn=5, K=10, out=p, ldo=20):
        return L.clipmi_pts_apply(logits, ld, N, C, params, nl, nn, K, out, ldo, None, None)
    assert apply(nl=5) == _lib.ERR_SHAPE and "n_layers=5" in _lib.last_error()
    assert apply(nl=-1) == _lib.ERR_SHAPE and apply(nn=33) == _lib.ERR_SHAPE and apply(nn=0) == _lib.ERR_SHAPE
    assert apply(C=9, ld=9, ldo=9) == _lib.ERR_SHAPE and apply(ldo=19) == _lib.ERR_SHAPE and apply(ld=19) == _lib.ERR_SHAPE
    assert apply(logits=None) == _lib.ERR_ARG and apply(params=None) == _lib.ERR_ARG and apply(out=None) == _lib.ERR_ARG
    assert apply(N=0) == _lib.OK

    def evaluate(feat=p, logits=p, labels=p, order=None, first=0, rows=4, N=4, C=20, params=p, nl=2, nn=5, K=10, out=p, ws=p, floats=1 << 20):
        return L.clipmi_pts_eval(feat, logits, 20, labels, order, first, rows, N, C, params, nl, nn, K, out, ws, floats, None)
    for k in ("feat", "logits", "labels", "params", "out", "ws"):
        assert evaluate(**{k: None}) == _lib.ERR_ARG, k
    assert evaluate(rows=0) == _lib.ERR_SHAPE and evaluate(first=1) == _lib.ERR_SHAPE and evaluate(first=-1) == _lib.ERR_SHAPE
    assert evaluate(K=33) == _lib.ERR_SHAPE and evaluate(C=5) == _lib.ERR_SHAPE
    assert evaluate(floats=4 * 22 - 1) == _lib.ERR_WORKSPACE and "88 needed" in _lib.last_error()

    def fit(logits=p, labels=p, N=4, C=20, nl=2, nn=5, K=10, batch=3, epochs=1, lr=p, opt=0, mom=0.9, damp=0.0, wd=5e-4, nes=0, b1=0.9, b2=0.999,
            eps=1e-8, state=p, ws=p, floats=1 << 20):
        return L.clipmi_pts_fit(logits, 20, labels, None, N, C, nl, nn, K, batch, epochs, 0, lr, opt, mom, damp, wd, nes, b1, b2, eps, state, None,
                                ws, floats, None)
    for k in ("logits", "labels", "lr", "state", "ws"):
        assert fit(**{k: None}) == _lib.ERR_ARG, k
    assert fit(N=0) == _lib.ERR_SHAPE and fit(batch=0) == _lib.ERR_SHAPE and fit(nl=5) == _lib.ERR_SHAPE and fit(C=9) == _lib.ERR_SHAPE
    assert fit(epochs=-1) == _lib.ERR_ARG and fit(opt=2) == _lib.ERR_ARG and fit(mom=1.0) == _lib.ERR_ARG and fit(nes=1, mom=0.0) == _lib.ERR_ARG
    assert fit(opt=1, b2=1.0) == _lib.ERR_ARG and fit(opt=1, eps=-1.0) == _lib.ERR_ARG and fit(opt=1, wd=-1.0) == _lib.ERR_ARG
    assert fit(floats=4 * 10 + 3 * 22 - 1) == _lib.ERR_WORKSPACE
    assert fit(epochs=0) == _lib.OK                                                                    # nothing is launched
