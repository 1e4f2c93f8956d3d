"""CPU checks of the image preprocessing path (clip_calibration_amd/preprocess.py, csrc/preprocess.hip): the numpy restatement the GPU
tests use as their oracle equals Pillow bit for bit, the committed Pillow fixture equals the restatement, the host geometry follows
torchvision, and the C ABI refuses bad descriptors before anything reaches a device."""
import ctypes
import hashlib
import os

import numpy as np
import pytest
import torch

import preprocess_ref as ref
from clip_calibration_amd import _lib
from clip_calibration_amd.preprocess import (CLIP_MEAN, CLIP_STD, PackedImages, Preprocess, identity_table, normalize_table, pack_images,
                                             resize_geometry)
from conftest import GOLDEN, load_golden

# (height, width, n_px): short side 224 / 225, 1 x N and N x 1, extreme aspect ratios, upscales, ImageNet-typical, odd crops
SWEEP = [(224, 224, 224), (225, 225, 224), (224, 300, 224), (225, 300, 224), (300, 225, 224), (1, 50, 64), (50, 1, 64), (1, 1, 64),
         (1, 700, 64), (224, 2000, 224), (3000, 225, 64), (2000, 224, 64), (32, 32, 224), (100, 224, 224), (32, 32, 64), (17, 23, 64),
         (500, 375, 224), (375, 500, 224), (375, 500, 64), (480, 640, 64), (427, 640, 224), (333, 500, 64), (64, 64, 64), (65, 64, 64),
         (63, 64, 64), (129, 130, 64), (1000, 1000, 64), (768, 1024, 64), (97, 130, 64), (3, 5, 64)]
CHECKER = {(97, 130, 64), (224, 300, 224), (32, 32, 64), (129, 130, 64)}


def _input(h, w, n_px, i):
    return ref.checkerboard(h, w, 2 + i % 2) if (h, w, n_px) in CHECKER else ref.synthetic_image(h, w, i)


@pytest.mark.parametrize("filt", ["bicubic", "bilinear"])
def test_restatement_equals_pillow(filt):
    Image = pytest.importorskip("PIL.Image")
    pf = {"bicubic": Image.BICUBIC, "bilinear": Image.BILINEAR}[filt]
    for i, (h, w, n_px) in enumerate(SWEEP):
        img = _input(h, w, n_px, i)
        nh, nw = ref.resize_size(h, w, n_px)
        top, left = ref.crop_offsets(nh, nw, n_px)
        pil = np.asarray(Image.fromarray(img).resize((nw, nh), pf))[top:top + n_px, left:left + n_px]
        mine = ref.resize_crop(img, n_px, filt)
        assert mine.shape == (n_px, n_px, 3)
        assert np.array_equal(pil, mine), f"{h} x {w} -> {n_px} ({filt}): max |d| {np.abs(pil.astype(int) - mine).max()}"


def test_checkerboard_reaches_both_clamps():
    """The 0 / 255 checkerboards are there to drive bicubic overshoot into the clamp at both ends: make sure they do."""
    for cell in (2, 3):
        img = ref.checkerboard(97, 130, cell).astype(np.int64)
        _, nw = ref.resize_size(97, 130, 64)
        xmin, k, _ = ref.coeffs(130, nw, "bicubic")
        idx = np.minimum(xmin[:, None] + np.arange(k.shape[1])[None, :], 129)
        acc = (img[:, idx, 0] * k[None]).sum(axis=2) + (1 << 21)     # horizontal pass before the clamp
        assert (acc >> 22).max() > 255 and (acc >> 22).min() < 0, cell


def test_fixture_matches_restatement_and_input_hashes():
    g = load_golden("preprocess_cases.npz")
    cases = len([k for k in g if k.startswith("meta")])
    assert cases == 8 and os.path.getsize(os.path.join(GOLDEN, "preprocess_cases.npz")) < 1 << 20
    assert sum(int(g[f"meta{i}"][2] == 224) for i in range(cases)) == 2
    for i in range(cases):
        h, w, n_px, f, checker = (int(v) for v in g[f"meta{i}"])
        img = ref.checkerboard(h, w, 2) if checker else ref.synthetic_image(h, w, i)
        assert hashlib.sha256(img.tobytes()).hexdigest() == str(g[f"sha{i}"]), f"case {i}: input generator changed"
        assert np.array_equal(ref.resize_crop(img, n_px, "bicubic" if f == 3 else "bilinear"), g[f"out{i}"]), f"case {i}"


def test_geometry_follows_torchvision():
    for h, w, n_px in SWEEP + [(375, 500, 336), (1, 3, 224), (10, 17, 4)]:
        short, long = min(h, w), max(h, w)
        nl = int(n_px * long / short)
        nh, nw = (n_px, nl) if h <= w else (nl, n_px)
        top, left = int(round((nh - n_px) / 2.0)), int(round((nw - n_px) / 2.0))
        assert resize_geometry(h, w, n_px) == (nh, nw, top, left)
        assert ref.resize_size(h, w, n_px) == (nh, nw) and ref.crop_offsets(nh, nw, n_px) == (top, left)
    # half to even: (new - n_px) / 2 = 18.5 -> 18, 19.5 -> 20
    assert resize_geometry(224, 224 + 37, 224)[3] == 18
    assert resize_geometry(224, 224 + 39, 224)[3] == 20
    assert resize_geometry(224 + 37, 224, 224)[2] == 18
    assert resize_geometry(375, 500, 224) == (224, 298, 0, 37)
    with pytest.raises(ValueError):
        resize_geometry(0, 5, 224)


def test_normalize_table_is_totensor_then_normalize():
    t = normalize_table()
    assert t.dtype == torch.float32 and t.shape == (3, 256)
    u = torch.arange(256, dtype=torch.uint8).view(1, 16, 16).expand(3, 16, 16).contiguous()
    x = u.to(torch.float32).div(255)                               # torchvision ToTensor
    x = x.sub_(torch.tensor(CLIP_MEAN)[:, None, None]).div_(torch.tensor(CLIP_STD)[:, None, None])   # Normalize
    assert torch.equal(t, x.reshape(3, 256))
    assert torch.equal(identity_table()[1], torch.arange(256, dtype=torch.float32))


def test_pack_images_layout():
    a, b = ref.synthetic_image(5, 7, 0), ref.synthetic_image(3, 2, 1)
    p = pack_images([a, torch.from_numpy(b)])
    assert isinstance(p, PackedImages) and len(p) == 2
    assert p.shapes.tolist() == [[0, 5, 7], [105, 3, 2]]
    assert np.array_equal(p.data.numpy(), np.concatenate([a.reshape(-1), b.reshape(-1)]))
    p2, labels = pack_images([(a, 3), (b, 4)])
    assert labels.tolist() == [3, 4] and torch.equal(p2.data, p.data)
    with pytest.raises(TypeError):
        pack_images([np.zeros((4, 4, 3), np.float32)])


def test_preprocess_arguments():
    with pytest.raises(ValueError):
        Preprocess(224, interpolation="lanczos")
    with pytest.raises(TypeError):
        Preprocess(224, dtype=torch.bfloat16)
    with pytest.raises(ValueError):
        Preprocess(0)


def test_cabi_rejects_bad_arguments_without_a_gpu():
    L = _lib.lib
    p = ctypes.c_void_p(4096)

    def descs(*items):
        return (_lib.ImageDesc * len(items))(*items)

    good = _lib.ImageDesc(0, 10, 20, 60, 3, 1)          # 10 x 20 HWC = 600 bytes
    ws = 1 << 24

    def call(d=None, B=1, n_px=64, filt=_lib.FILTER_BICUBIC, dtype=_lib.F16, nbytes=600, table=p):
        d = descs(good) if d is None else d
        return L.clipmi_preprocess(p, nbytes, d, B, n_px, filt, table, p, dtype, p, ws, None)

    assert call(B=0) == _lib.ERR_SHAPE and "B = 0" in _lib.last_error()
    assert call(n_px=0) == _lib.ERR_SHAPE and "n_px" in _lib.last_error()
    assert call(n_px=4097) == _lib.ERR_SHAPE
    assert call(d=descs(_lib.ImageDesc(0, 10, 0, 60, 3, 1))) == _lib.ERR_SHAPE and "0" in _lib.last_error()     # W = 0
    assert call(d=descs(_lib.ImageDesc(0, 0, 20, 60, 3, 1))) == _lib.ERR_SHAPE                                   # H = 0
    assert call(filt=1) == _lib.ERR_ARG and "filter" in _lib.last_error()
    assert call(filt=4) == _lib.ERR_ARG
    assert call(dtype=7) == _lib.ERR_ARG and "dtype" in _lib.last_error()
    assert call(table=None) == _lib.ERR_ARG
    assert call(nbytes=599) == _lib.ERR_ARG and "outside" in _lib.last_error()                                 # last byte beyond
    assert call(d=descs(_lib.ImageDesc(0, 10, 20, 61, 3, 1))) == _lib.ERR_ARG                                   # row stride too long
    assert call(d=descs(_lib.ImageDesc(1, 10, 20, 60, 3, 1))) == _lib.ERR_ARG                                   # offset pushes it out
    assert call(d=descs(_lib.ImageDesc(-1, 10, 20, 60, 3, 1))) == _lib.ERR_ARG
    assert call(d=descs(_lib.ImageDesc(598, 10, 20, -60, -3, -1))) == _lib.ERR_ARG                              # negative strides: below 0
    assert call(d=descs(good, _lib.ImageDesc(0, 10, 20, 600, 3, 1)), B=2) == _lib.ERR_ARG and "image 1" in _lib.last_error()
    assert L.clipmi_preprocess(p, 600, descs(good), 1, 64, _lib.FILTER_BICUBIC, p, p, _lib.F16, p, 16, None) == _lib.ERR_WORKSPACE
    assert L.clipmi_preprocess_workspace_bytes(descs(good), 0, 64, _lib.FILTER_BICUBIC) == 0
    assert L.clipmi_preprocess_workspace_bytes(descs(good), 1, 64, 0) == 0
    assert L.clipmi_preprocess_workspace_bytes(descs(good), 1, 64, _lib.FILTER_BICUBIC) > 0
    assert L.clipmi_preprocess_workspace_bytes(None, 1, 64, _lib.FILTER_BICUBIC) == 0
