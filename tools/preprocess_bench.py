"""Kernel time of clipmi_preprocess (csrc/preprocess.hip) on batches of 256 uint8 HWC images, against the one-core host path it
replaces (PIL resize + crop, then ToTensor + Normalize with torch CPU ops).  Measurement only; bench.py does not run it.

Per geometry: the C call is timed between two device events (descriptor upload + tap launch + resample launch), median of --iters
launches after --warmup, with the host queueing all of them behind a device sleep so that no host gap lands inside an interval.
Launches rotate over input batches totalling more than 256 MiB, so the Infinity Cache does not serve the reads.  Bytes moved are
computed from the shapes: the input rows and columns the cropped outputs read (uint8) + the fp16 output.

Usage: python tools/preprocess_bench.py [--iters 50] [--warmup 10] [--out profiles/preprocess_bench.json]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import preprocess_ref as ref  # noqa: E402
from clip_calibration_amd import _lib  # noqa: E402
from clip_calibration_amd.preprocess import CLIP_MEAN, CLIP_STD, normalize_table  # noqa: E402

GEOMETRIES = [(375, 500, "500x375 (ImageNet-typical)"), (224, 224, "224x224 (identity)"), (768, 1024, "1024x768"), (32, 32, "32x32 (upscale)")]


def read_bytes(h, w, n_px, filt="bicubic"):
    """uint8 bytes one image's cropped outputs read: (rows read) x (columns read) x 3"""
    nh, nw = ref.resize_size(h, w, n_px)
    top, left = ref.crop_offsets(nh, nw, n_px)
    span = []
    for in_size, out_size, first in ((w, nw, left), (h, nh, top)):
        xmin, _, cnt = ref.coeffs(in_size, out_size, filt, first, n_px)
        span.append(int(xmin[-1] + cnt[-1] - xmin[0]))
    return span[0] * span[1] * 3


def host_rate(h, w, n_px, n=16):
    """images/s of the host path on ONE core: PIL resize + crop + ToTensor + Normalize (torch CPU fp32) + .half()"""
    from PIL import Image
    torch.set_num_threads(1)
    imgs = [Image.fromarray(ref.synthetic_image(h, w, i)) for i in range(n)]
    mean, std = torch.tensor(CLIP_MEAN)[:, None, None], torch.tensor(CLIP_STD)[:, None, None]
    nh, nw = ref.resize_size(h, w, n_px)
    top, left = ref.crop_offsets(nh, nw, n_px)
    t0 = time.perf_counter()
    for im in imgs:
        r = im.resize((nw, nh), Image.BICUBIC).crop((left, top, left + n_px, top + n_px))
        x = torch.from_numpy(np.asarray(r)).permute(2, 0, 1).contiguous().to(torch.float32).div(255)
        x.sub_(mean).div_(std).half()
    return n / (time.perf_counter() - t0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--n-px", type=int, default=224)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    B, n = a.batch, a.n_px
    table = normalize_table().to(dev)
    out = torch.empty((B, 3, n, n), dtype=torch.float16, device=dev)
    rows = []
    for h, w, name in GEOMETRIES:
        per_batch = B * h * w * 3
        nbuf = max(2, -(-(256 << 20) // per_batch) + 1)            # more than 256 MiB of distinct input
        pool = torch.empty(nbuf * per_batch, dtype=torch.uint8, device=dev)
        g = torch.Generator(device=dev).manual_seed(0)
        pool.random_(0, 256, generator=g)
        descs = (_lib.ImageDesc * B)(*[_lib.ImageDesc(i * h * w * 3, h, w, w * 3, 3, 1) for i in range(B)])
        ws_bytes = _lib.lib.clipmi_preprocess_workspace_bytes(descs, B, n, _lib.FILTER_BICUBIC)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        stream = torch.cuda.current_stream(dev)

        def call(k):
            base = pool.data_ptr() + (k % nbuf) * per_batch
            _lib.check(_lib.lib.clipmi_preprocess(base, per_batch, descs, B, n, _lib.FILTER_BICUBIC, table.data_ptr(), out.data_ptr(),
                                                  _lib.F16, ws.data_ptr(), ws_bytes, stream.cuda_stream), "clipmi_preprocess")
        for k in range(a.warmup):
            call(k)
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(a.iters)]
        torch.cuda.synchronize()
        torch.cuda._sleep(200_000_000)                             # the host queues every launch while the device sleeps
        for k, (e0, e1) in enumerate(ev):
            e0.record(stream)
            call(a.warmup + k)
            e1.record(stream)
        torch.cuda.synchronize()
        us = sorted(e0.elapsed_time(e1) * 1e3 for e0, e1 in ev)
        med = statistics.median(us)
        rd = B * read_bytes(h, w, n)
        wr = out.numel() * out.element_size()
        host = host_rate(h, w, n)
        rows.append({"input": name, "H": h, "W": w, "batch": B, "n_px": n, "out_dtype": "fp16", "launches": a.iters,
                     "kernel_us_median": round(med, 2), "kernel_us_min": round(us[0], 2), "kernel_us_max": round(us[-1], 2),
                     "bytes_read": rd, "bytes_written": wr, "gb_per_s": round((rd + wr) / med / 1e3, 1),
                     "images_per_s_device": round(B / med * 1e6), "input_pool_mib": round(nbuf * per_batch / 2**20),
                     "host_one_core_images_per_s": round(host, 1), "host_one_core_us_per_batch": round(B / host * 1e6)})
        print(json.dumps(rows[-1]), flush=True)
        del pool, ws
        torch.cuda.empty_cache()
    res = {"tool": "tools/preprocess_bench.py", "device": torch.cuda.get_device_name(dev), "rows": rows}
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
