"""numpy restatement of the reference's train transform for uint8 RGB images, torchvision's PIL path of ``RandomResizedCrop`` +
``RandomHorizontalFlip``: ``img.crop(box).resize((n_px, n_px), filter)`` then ``transpose(FLIP_LEFT_RIGHT)`` -- crop, then stretch
(Pillow's 8-bit resampler on the BOX: tests/preprocess_ref.py ``_pass``), then flip.  The GPU kernel (clip_calibration_amd/csrc/augment.hip)
is checked against this, and this against Pillow (tests/test_augment_cpu.py).  Also a plain-Python restatement of the sampler
(``RandomResizedCrop.get_params`` + the flip draw), written from torchvision's public source one scalar draw at a time."""
from __future__ import annotations

import math

import numpy as np
import torch

from preprocess_ref import _pass, checkerboard, synthetic_image  # noqa: F401  (the image generators are re-exported for the tests)


def view(img: np.ndarray, box, n_px: int, filt: str = "bicubic", flip: bool = False) -> np.ndarray:
    """One view of an [H, W, 3] uint8 image -> [n_px, n_px, 3] uint8.  ``box`` = (top, left, height, width)."""
    top, left, h, w = (int(v) for v in box)
    assert 0 <= top and 0 <= left and h >= 1 and w >= 1 and top + h <= img.shape[0] and left + w <= img.shape[1], box
    out = img[top:top + h, left:left + w]            # Pillow crops first: no tap reaches past the box
    if w != n_px:                                     # Pillow skips a pass whose sizes are equal
        out = _pass(out, 1, n_px, filt, 0, n_px)
    if h != n_px:
        out = _pass(out, 0, n_px, filt, 0, n_px)
    if flip:
        out = out[:, ::-1]
    return np.ascontiguousarray(out)


def get_params(height: int, width: int, scale, ratio, generator):
    """torchvision RandomResizedCrop.get_params: (top, left, h, w)."""
    area = height * width
    log_ratio = torch.log(torch.tensor(ratio))
    for _ in range(10):
        target_area = area * torch.empty(1).uniform_(scale[0], scale[1], generator=generator).item()
        aspect_ratio = torch.exp(torch.empty(1).uniform_(log_ratio[0], log_ratio[1], generator=generator)).item()
        w = int(round(math.sqrt(target_area * aspect_ratio)))
        h = int(round(math.sqrt(target_area / aspect_ratio)))
        if 0 < w <= width and 0 < h <= height:
            i = torch.randint(0, height - h + 1, size=(1,), generator=generator).item()
            j = torch.randint(0, width - w + 1, size=(1,), generator=generator).item()
            return i, j, h, w
    in_ratio = float(width) / float(height)           # fallback: the central crop
    if in_ratio < min(ratio):
        w = width
        h = int(round(w / min(ratio)))
    elif in_ratio > max(ratio):
        h = height
        w = int(round(h * max(ratio)))
    else:
        w, h = width, height
    return (height - h) // 2, (width - w) // 2, h, w


def sample(shapes, scale=(0.08, 1.0), ratio=(3.0 / 4.0, 4.0 / 3.0), flip_p=0.5, generator=None, views_per_image=1):
    """List of (image, top, left, h, w, flip), image by image: get_params, then RandomHorizontalFlip's one ``torch.rand(1) < p``."""
    out = []
    for b, (H, W) in enumerate(shapes):
        for _ in range(views_per_image):
            box = get_params(int(H), int(W), scale, ratio, generator)
            out.append((b,) + tuple(int(v) for v in box) + (int(torch.rand(1, generator=generator).item() < flip_p),))
    return out


N_PX = (8, 20, 72)     # vector store | scalar tail (no multiple of 8) | two column tiles and three row tiles


def cases(n_px: int):
    """(images, views) of the shapes that can still go wrong at this n_px: ``images`` a ragged list of [H, W, 3] uint8 arrays, ``views`` a
    list of (image, top, left, h, w, flip).  Content: a hash image, a 0 / 255 checkerboard (both clamps), a tall image and one a little
    larger than n_px.  Boxes: the whole image, one touching each corner of a larger image, 1 x 1, 1 x W, H x 1, 5 x 7 (an upscale),
    300 x 9 (a tile's input rows exceed one LDS chunk at n_px = 8), and boxes with one side or both equal to n_px (a skipped pass)."""
    images = [synthetic_image(40, 52, 1), checkerboard(40, 52, 2), synthetic_image(310, 30, 2), synthetic_image(n_px + 9, n_px + 13, 3)]
    boxes = [(0, 0, 0, 40, 52), (0, 0, 0, 17, 23), (0, 0, 29, 17, 23), (0, 23, 0, 17, 23), (0, 23, 29, 17, 23),
             (0, 13, 7, 1, 1), (0, 5, 0, 1, 52), (0, 0, 51, 40, 1), (0, 11, 19, 5, 7),
             (1, 0, 0, 40, 52), (1, 7, 9, 21, 30), (1, 23, 29, 17, 23), (1, 11, 19, 5, 7),
             (2, 5, 11, 300, 9), (2, 0, 0, 310, 30),
             (3, 4, 5, n_px, n_px + 6), (3, 3, 2, n_px + 5, n_px), (3, 1, 1, n_px, n_px), (3, 0, 0, n_px + 9, n_px + 13)]
    return images, [b + (i % 2,) for i, b in enumerate(boxes)]
