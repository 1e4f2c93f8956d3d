"""Writes tests/golden/preprocess_cases.npz: Pillow's own Resize(n_px) + CenterCrop(n_px) output (torchvision's sizes and offsets,
Image.resize with BICUBIC / BILINEAR) for eight uint8 RGB inputs, so that a machine without Pillow still has a Pillow ground truth.
Inputs are closed-form (tests/preprocess_ref.py: synthetic_image, checkerboard), never stored: only each input's sha256 and the
outputs are.  Usage: python tools/gen_preprocess_golden.py [out.npz]"""
import hashlib
import os
import sys

import numpy as np
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import preprocess_ref as ref  # noqa: E402

# (height, width, n_px, filter, input): input "hash" = synthetic_image(h, w, case), "checker" = checkerboard(h, w, 2)
CASES = [
    (375, 500, 64, "bicubic", "hash"),     # landscape downscale (ImageNet-typical aspect)
    (500, 375, 64, "bicubic", "hash"),     # portrait downscale
    (64, 64, 64, "bicubic", "hash"),       # identity
    (32, 48, 64, "bicubic", "hash"),       # upscale
    (1, 200, 64, "bicubic", "hash"),       # 1 x N
    (97, 130, 64, "bicubic", "checker"),   # 0 / 255 overshoot into both clamps
    (375, 500, 224, "bicubic", "hash"),
    (427, 640, 224, "bilinear", "hash"),
]
PIL_FILTER = {"bicubic": Image.BICUBIC, "bilinear": Image.BILINEAR}


def case_input(i):
    h, w, _, _, kind = CASES[i]
    return ref.synthetic_image(h, w, i) if kind == "hash" else ref.checkerboard(h, w, 2)


def main(path):
    out = {}
    for i, (h, w, n_px, filt, kind) in enumerate(CASES):
        img = case_input(i)
        nh, nw = ref.resize_size(h, w, n_px)
        top, left = ref.crop_offsets(nh, nw, n_px)
        pil = np.asarray(Image.fromarray(img).resize((nw, nh), PIL_FILTER[filt]))[top:top + n_px, left:left + n_px]
        out[f"out{i}"] = np.ascontiguousarray(pil)
        out[f"meta{i}"] = np.array([h, w, n_px, 3 if filt == "bicubic" else 2, 1 if kind == "checker" else 0], dtype=np.int64)
        out[f"sha{i}"] = np.array(hashlib.sha256(img.tobytes()).hexdigest())
    np.savez_compressed(path, **out)
    print(f"wrote {path} ({os.path.getsize(path)} bytes, {len(CASES)} cases)")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "preprocess_cases.npz"))
