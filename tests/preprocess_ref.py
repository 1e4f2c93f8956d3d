"""numpy restatement of the reference's test transform for uint8 RGB images (clip/clip.py:74-81, Dassl's test transform):
torchvision ``Resize(n_px, BICUBIC)`` on the shorter side -> Pillow ``Image.resize`` (libImaging/Resample.c, 8-bit path) ->
``CenterCrop(n_px)``.  The GPU kernel (clip_calibration_amd/csrc/preprocess.hip) is checked against this, and this against Pillow
(tests/test_preprocess_cpu.py).  Every float step is a float64 numpy op in Pillow's own order, so nothing fuses."""
from __future__ import annotations

import numpy as np

PRECISION_BITS = 22
SUPPORT = {"bilinear": 1.0, "bicubic": 2.0}


def _filter(name: str, x: np.ndarray) -> np.ndarray:
    x = np.abs(x)
    if name == "bicubic":
        a = -0.5
        near = ((a + 2.0) * x - (a + 3.0)) * x * x + 1
        far = (((x - 5) * x + 8) * x - 4) * a
        return np.where(x < 1.0, near, np.where(x < 2.0, far, 0.0))
    if name == "bilinear":
        return np.where(x < 1.0, 1.0 - x, 0.0)
    raise ValueError(f"unknown filter {name!r}")


def coeffs(in_size: int, out_size: int, filt: str, first: int = 0, count: int | None = None):
    """precompute_coeffs + normalize_coeffs_8bpc for outputs first .. first + count - 1: (xmin [n], int32 taps [n, ksize]),
    taps beyond each output's own tap count are 0."""
    count = out_size - first if count is None else count
    scale = float(in_size) / out_size
    filterscale = max(scale, 1.0)
    support = SUPPORT[filt] * filterscale
    ksize = int(np.ceil(support)) * 2 + 1
    xx = np.arange(first, first + count, dtype=np.float64)
    center = (xx + 0.5) * scale
    ss = 1.0 / filterscale
    xmin = np.maximum(np.trunc(center - support + 0.5).astype(np.int64), 0)
    xmax = np.minimum(np.trunc(center + support + 0.5).astype(np.int64), in_size) - xmin
    t = np.arange(ksize)
    valid = t[None, :] < xmax[:, None]
    w = _filter(filt, ((t[None, :] + xmin[:, None]).astype(np.float64) - center[:, None] + 0.5) * ss)
    w = np.where(valid, w, 0.0)
    ww = np.zeros(count)
    for k in range(ksize):                       # Pillow sums the taps left to right
        ww = ww + w[:, k]
    w = np.where(ww[:, None] != 0.0, w / np.where(ww == 0.0, 1.0, ww)[:, None], w)
    scaled = w * float(1 << PRECISION_BITS)
    fixed = np.where(w < 0, np.trunc(-0.5 + scaled), np.trunc(0.5 + scaled)).astype(np.int64)
    return xmin, np.where(valid, fixed, 0), xmax


def _pass(img: np.ndarray, axis: int, out_size: int, filt: str, first: int, count: int) -> np.ndarray:
    """One separable pass of ImagingResample{Horizontal,Vertical}_8bpc along `axis` of an HWC uint8 image."""
    in_size = img.shape[axis]
    xmin, k, _ = coeffs(in_size, out_size, filt, first, count)
    src = np.moveaxis(img.astype(np.int64), axis, 0)              # [in, other, C]
    acc = np.full((count,) + src.shape[1:], 1 << (PRECISION_BITS - 1), dtype=np.int64)
    for j in range(k.shape[1]):
        idx = np.minimum(xmin + j, in_size - 1)
        acc += src[idx] * k[:, j][:, None, None]
    out = np.clip(acc >> PRECISION_BITS, 0, 255).astype(np.uint8)
    return np.moveaxis(out, 0, axis)


def resize_size(h: int, w: int, n_px: int):
    """torchvision Resize(int) on the shorter side: (new_h, new_w)."""
    short, long = min(h, w), max(h, w)
    new_short, new_long = n_px, int(n_px * long / short)
    return (new_short, new_long) if h <= w else (new_long, new_short)


def crop_offsets(new_h: int, new_w: int, n_px: int):
    """torchvision CenterCrop: (top, left), Python's round (half to even)."""
    return int(round((new_h - n_px) / 2.0)), int(round((new_w - n_px) / 2.0))


def pil_resize(img: np.ndarray, out_h: int, out_w: int, filt: str = "bicubic") -> np.ndarray:
    """Image.fromarray(img).resize((out_w, out_h), filt) for an [H, W, 3] uint8 array."""
    h, w = img.shape[:2]
    if w != out_w:
        img = _pass(img, 1, out_w, filt, 0, out_w)
    if h != out_h:
        img = _pass(img, 0, out_h, filt, 0, out_h)
    return img


def resize_crop(img: np.ndarray, n_px: int, filt: str = "bicubic") -> np.ndarray:
    """Resize(n_px) + CenterCrop(n_px) of an [H, W, 3] uint8 image -> [n_px, n_px, 3] uint8, computing only the cropped outputs
    (each output depends on its own taps only, so this equals resize-then-crop)."""
    h, w = img.shape[:2]
    nh, nw = resize_size(h, w, n_px)
    top, left = crop_offsets(nh, nw, n_px)
    if w != nw:
        img = _pass(img, 1, nw, filt, left, n_px)
    else:
        img = img[:, left:left + n_px]
    if h != nh:
        img = _pass(img, 0, nh, filt, top, n_px)
    else:
        img = img[top:top + n_px]
    return np.ascontiguousarray(img)


def synthetic_image(h: int, w: int, case: int) -> np.ndarray:
    """A closed-form integer hash of (y, x, c, case) -> [H, W, 3] uint8 (no RNG stream: the same bits on every machine)."""
    y, x, c = np.meshgrid(np.arange(h, dtype=np.uint64), np.arange(w, dtype=np.uint64), np.arange(3, dtype=np.uint64), indexing="ij")
    v = (y * np.uint64(73856093)) ^ (x * np.uint64(19349663)) ^ (c * np.uint64(83492791)) ^ (np.uint64(case) * np.uint64(2654435761))
    v = (v ^ (v >> np.uint64(13))) * np.uint64(0x5bd1e995) & np.uint64(0xffffffff)
    v = v ^ (v >> np.uint64(15))
    return (v & np.uint64(0xff)).astype(np.uint8)


def checkerboard(h: int, w: int, cell: int = 1) -> np.ndarray:
    """0 / 255 checkerboard: pushes bicubic overshoot into the clamp at both ends."""
    y, x = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    v = (((y // cell) + (x // cell)) % 2 * 255).astype(np.uint8)
    return np.repeat(v[:, :, None], 3, axis=2)
