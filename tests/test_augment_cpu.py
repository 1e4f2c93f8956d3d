"""CPU checks of the train transform (clip_calibration_amd/augment.py, csrc/augment.hip): the numpy restatement the GPU tests use as
their oracle equals Pillow's crop -> resize -> flip byte for byte, the sampler restates torchvision's draws and keeps its boxes inside
the images, and the C ABI refuses bad views before anything reaches a device."""
import ctypes
import math

import numpy as np
import pytest
import torch

import augment_ref as ref
import preprocess_ref
from clip_calibration_amd import _lib
from clip_calibration_amd.augment import TrainPreprocess, sample_views

FILTERS = ["bicubic", "bilinear"]


@pytest.mark.parametrize("filt", FILTERS)
def test_restatement_equals_pillow(filt):
    Image = pytest.importorskip("PIL.Image")
    pf = {"bicubic": Image.BICUBIC, "bilinear": Image.BILINEAR}[filt]
    for n_px in ref.N_PX:
        images, views = ref.cases(n_px)
        for b, top, left, h, w, flip in views:
            pil = Image.fromarray(images[b]).crop((left, top, left + w, top + h)).resize((n_px, n_px), pf)
            if flip:
                pil = pil.transpose(Image.FLIP_LEFT_RIGHT)
            mine = ref.view(images[b], (top, left, h, w), n_px, filt, flip)
            assert mine.shape == (n_px, n_px, 3)
            assert np.array_equal(np.asarray(pil), mine), f"image {b} box {(top, left, h, w)} flip {flip} -> {n_px} ({filt})"


def test_cases_reach_both_clamps_and_the_skipped_pass():
    """The checkerboard upscale is there to drive bicubic overshoot into the clamp at both ends, and the boxes with a side of n_px to
    take the skipped pass: make sure they do."""
    images, views = ref.cases(20)
    b, top, left, h, w, _ = views[12]
    assert (b, h, w) == (1, 5, 7)
    box = images[b][top:top + h, left:left + w].astype(np.int64)
    xmin, k, _ = preprocess_ref.coeffs(w, 20, "bicubic")
    idx = np.minimum(xmin[:, None] + np.arange(k.shape[1])[None, :], w - 1)
    acc = (box[:, idx, 0] * k[None]).sum(axis=2) + (1 << 21)          # horizontal pass before the clamp
    assert (acc >> 22).max() > 255 and (acc >> 22).min() < 0
    for n_px in ref.N_PX:
        sides = [(v[3] == n_px, v[4] == n_px) for v in ref.cases(n_px)[1]]
        assert (True, False) in sides and (False, True) in sides and (True, True) in sides


def test_flip_mirrors_the_resized_image():
    img = ref.synthetic_image(30, 41, 5)
    a, b = ref.view(img, (2, 3, 20, 31), 8, "bicubic", False), ref.view(img, (2, 3, 20, 31), 8, "bicubic", True)
    assert np.array_equal(a[:, ::-1], b) and not np.array_equal(a, b)


# ---- sampler -------------------------------------------------------------------------------------------------------------------------

SHAPES = [(375, 500), (500, 375), (224, 224), (64, 80), (333, 400)]      # aspect ratios inside [3/4, 4/3]: see test_boxes_respect_the_bounds


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def test_sampler_is_seeded_and_equals_the_restatement():
    a = sample_views(SHAPES, generator=_gen(3))
    b = sample_views(np.asarray(SHAPES), generator=_gen(3))
    c = sample_views(SHAPES, generator=_gen(4))
    assert len(a) == 6 and all(x.dtype == np.int32 and x.shape == (len(SHAPES),) for x in a)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    assert any(not np.array_equal(x, y) for x, y in zip(a, c))
    assert np.stack(a, axis=1).tolist() == [list(v) for v in ref.sample(SHAPES, generator=_gen(3))]
    kw = dict(scale=(0.3, 0.9), ratio=(0.5, 2.0), flip_p=0.25, views_per_image=2)
    assert np.stack(sample_views(SHAPES, generator=_gen(9), **kw), axis=1).tolist() == [list(v) for v in ref.sample(SHAPES, generator=_gen(9), **kw)]
    torch.manual_seed(11)                                              # no generator: torch's global CPU RNG
    g1 = sample_views(SHAPES)
    torch.manual_seed(11)
    assert np.stack(g1, axis=1).tolist() == [list(v) for v in ref.sample(SHAPES)]


def test_boxes_respect_the_bounds():
    """Every box lies inside its image; w = round(sqrt(area r)) and h = round(sqrt(area / r)) are each within 0.5 of their unrounded
    values, so some (a, b) in [w - 0.5, w + 0.5] x [h - 0.5, h + 0.5] has a b = area in scale * H W and a / b = r in the ratio bounds.
    The shapes' own aspect ratios lie inside the ratio bounds, so a fallback box (the whole image) satisfies the same inequalities."""
    scale, ratio = (0.08, 1.0), (3.0 / 4.0, 4.0 / 3.0)
    eps = 1e-6                                                         # the ratio's logs are fp32
    img, top, left, h, w, flip = sample_views(SHAPES * 40, generator=_gen(0))
    assert set(flip.tolist()) == {0, 1} and img.tolist() == list(range(len(SHAPES) * 40))
    for i, t, l, hh, ww in zip(img, top, left, h, w):
        H, W = SHAPES[i % len(SHAPES)]
        assert hh >= 1 and ww >= 1 and 0 <= t and 0 <= l and t + hh <= H and l + ww <= W
        assert (ww - 0.5) * (hh - 0.5) <= scale[1] * H * W and (ww + 0.5) * (hh + 0.5) >= scale[0] * H * W
        assert (ww - 0.5) / (hh + 0.5) <= ratio[1] * (1 + eps) and (ww + 0.5) / (hh - 0.5) >= ratio[0] * (1 - eps)
    assert len({(int(a), int(b)) for a, b in zip(h, w)}) > 50           # the boxes do vary


def test_fallback_is_the_clamped_centre_crop():
    """H = 10, W = 1000 with the default bounds: a try needs h = round(sqrt(area / r)) <= 10, but area >= 0.08 * 10 000 = 800 and
    r <= 4 / 3 give sqrt(area / r) >= sqrt(600) = 24.5.  No try succeeds, and the box is the centre crop at the largest ratio."""
    assert math.sqrt(0.08 * 10 * 1000 * 3 / 4) > 10.5
    for seed in range(5):
        img, top, left, h, w, _ = sample_views([(10, 1000)], generator=_gen(seed))
        assert (int(img[0]), int(top[0]), int(left[0]), int(h[0]), int(w[0])) == (0, 0, 493, 10, 13)
    _, top, left, h, w, _ = sample_views([(1000, 10)], generator=_gen(0))          # the other way round: ratio clamped from below
    assert (int(top[0]), int(left[0]), int(h[0]), int(w[0])) == ((1000 - 13) // 2, 0, 13, 10)


def test_views_per_image_and_arguments():
    v = sample_views(SHAPES, generator=_gen(1), views_per_image=3)
    assert v[0].tolist() == [b for b in range(len(SHAPES)) for _ in range(3)] and all(x.shape == (15,) for x in v)
    assert sample_views(SHAPES, flip_p=0.0, generator=_gen(1))[5].tolist() == [0] * 5
    assert sample_views(SHAPES, flip_p=1.0, generator=_gen(1))[5].tolist() == [1] * 5
    for bad in (dict(scale=(0.5, 0.1)), dict(ratio=(0.0, 1.0)), dict(flip_p=1.5), dict(views_per_image=0)):
        with pytest.raises(ValueError):
            sample_views(SHAPES, **bad)
    with pytest.raises(ValueError):
        sample_views([(0, 5)])
    with pytest.raises(ValueError):
        TrainPreprocess(224, interpolation="lanczos")
    with pytest.raises(ValueError):
        TrainPreprocess(224, scale=(0.0, 1.0))
    assert TrainPreprocess(64, scale=(0.2, 1.0)).scale == (0.2, 1.0)


# ---- C ABI ---------------------------------------------------------------------------------------------------------------------------

def test_cabi_rejects_bad_views_without_a_gpu():
    L = _lib.lib
    p = ctypes.c_void_p(4096)
    good = _lib.ImageDesc(0, 10, 20, 60, 3, 1)          # 10 x 20 HWC = 600 bytes
    ws = 1 << 24

    def call(views, images=(good,), n_px=8, filt=_lib.FILTER_BICUBIC, dtype=_lib.F16, nbytes=600, V=None, table=p):
        d = (_lib.ImageDesc * len(images))(*images)
        v = (_lib.ViewDesc * max(len(views), 1))(*[_lib.ViewDesc(*x) for x in views])
        return L.clipmi_augment(p, nbytes, d, len(images), v, len(views) if V is None else V, n_px, filt, table, p, dtype, p, ws, None)

    ok = (0, 2, 3, 5, 7, 1)
    assert call([ok, (0, 0, 0, 11, 20, 0)]) == _lib.ERR_ARG and "view 1" in _lib.last_error() and "outside" in _lib.last_error()   # too tall
    assert call([(0, 0, 14, 5, 7, 0)]) == _lib.ERR_ARG and "outside" in _lib.last_error()                    # left + width = 21
    assert call([(0, 6, 0, 5, 7, 0)]) == _lib.ERR_ARG                                                        # top + height = 11
    assert call([(0, -1, 0, 5, 7, 0)]) == _lib.ERR_ARG and call([(0, 0, -1, 5, 7, 0)]) == _lib.ERR_ARG
    assert call([(0, 2 ** 31 - 1, 0, 5, 7, 0)]) == _lib.ERR_ARG and call([(0, 0, 0, 2 ** 31 - 1, 7, 0)]) == _lib.ERR_ARG
    assert call([(0, 0, 0, 0, 7, 0)]) == _lib.ERR_SHAPE and "box" in _lib.last_error()                       # a zero side
    assert call([(0, 0, 0, 5, 0, 0)]) == _lib.ERR_SHAPE and call([(0, 0, 0, -3, 7, 0)]) == _lib.ERR_SHAPE
    assert call([(1, 0, 0, 5, 7, 0)]) == _lib.ERR_ARG and "image 1" in _lib.last_error()                     # image index out of range
    assert call([(-1, 0, 0, 5, 7, 0)]) == _lib.ERR_ARG
    assert call([ok], filt=1) == _lib.ERR_ARG and "filter" in _lib.last_error()                              # an unsupported filter
    assert call([ok], filt=4) == _lib.ERR_ARG
    assert call([], V=0) == _lib.ERR_SHAPE and "V = 0" in _lib.last_error()
    assert call([ok], V=65536) == _lib.ERR_SHAPE
    assert call([ok], n_px=0) == _lib.ERR_SHAPE and call([ok], n_px=4097) == _lib.ERR_SHAPE
    assert call([ok], dtype=7) == _lib.ERR_ARG and call([ok], table=None) == _lib.ERR_ARG
    assert call([ok], nbytes=599) == _lib.ERR_ARG and "pixel buffer" in _lib.last_error()                    # the existing extent check
    assert call([ok], images=(_lib.ImageDesc(0, 10, 0, 60, 3, 1),)) == _lib.ERR_SHAPE
    d, v = (_lib.ImageDesc * 1)(good), (_lib.ViewDesc * 1)(_lib.ViewDesc(*ok))
    assert L.clipmi_augment(p, 600, d, 1, v, 1, 8, _lib.FILTER_BICUBIC, p, p, _lib.F16, p, 16, None) == _lib.ERR_WORKSPACE
    assert L.clipmi_augment(p, 600, d, 1, None, 1, 8, _lib.FILTER_BICUBIC, p, p, _lib.F16, p, ws, None) == _lib.ERR_ARG
    assert L.clipmi_augment_workspace_bytes(d, 1, v, 1, 8, _lib.FILTER_BICUBIC) > 0
    assert L.clipmi_augment_workspace_bytes(d, 1, v, 1, 8, 0) == 0
    assert L.clipmi_augment_workspace_bytes(d, 1, v, 0, 8, _lib.FILTER_BICUBIC) == 0
    assert L.clipmi_augment_workspace_bytes(d, 1, None, 1, 8, _lib.FILTER_BICUBIC) == 0
    bad = (_lib.ViewDesc * 1)(_lib.ViewDesc(0, 0, 0, 11, 20, 0))
    assert L.clipmi_augment_workspace_bytes(d, 1, bad, 1, 8, _lib.FILTER_BICUBIC) == 0
    # the workspace follows the largest kernel: a 300-row box to 8 rows needs more taps than a 5 x 7 one
    tall = (_lib.ImageDesc * 1)(_lib.ImageDesc(0, 310, 30, 90, 3, 1))
    small, big = (_lib.ViewDesc * 1)(_lib.ViewDesc(0, 0, 0, 5, 7, 0)), (_lib.ViewDesc * 1)(_lib.ViewDesc(0, 5, 11, 300, 9, 0))
    assert L.clipmi_augment_workspace_bytes(tall, 1, big, 1, 8, _lib.FILTER_BICUBIC) > L.clipmi_augment_workspace_bytes(tall, 1, small, 1, 8, _lib.FILTER_BICUBIC)
    assert {"clipmi_augment", "clipmi_augment_workspace_bytes"} <= set(_lib.exported_symbols())
