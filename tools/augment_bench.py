"""Time of the train transform on the device (clip_calibration_amd.augment.TrainPreprocess, csrc/augment.hip) against the host Pillow
loop it replaces, and of one CLIP-Adapter training step under either.  Measurement only; bench.py does not run it.

1. transform: 256 sampled views (seeded) of 256 images of 500 x 375 to 224, bicubic, fp16.  Device: ``TrainPreprocess(images, views)``
   between two device events, median of --iters calls after --warmup, the host queueing all of them behind a device sleep so that
   no host gap lands inside an interval; the calls rotate over input batches totalling more than 256 MiB, so the Infinity Cache does
   not serve the reads.  Host: ``img.crop(box).resize((224, 224), BICUBIC)`` [+ FLIP_LEFT_RIGHT] + ToTensor + Normalize + .half() on the
   same views in a pool of at most 16 threads (Pillow's resize releases the GIL), wall clock, median of --host-iters passes.
2. step: transform + ViT-B/16 image tower (synthetic weights) + ``AdapterFitState.step`` on a batch of --step-batch images, wall clock
   around --iters steps ending in a device synchronise.  "device": uint8 images already on the GPU, views sampled per step on the
   host.  "host": the Pillow pool per step, the fp16 batch stacked into page-locked memory and copied over, then the same tower and step.

Usage: python tools/augment_bench.py [--iters 30] [--warmup 5] [--out profiles/augment_bench.json]"""
import argparse
import json
import os
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from clip_calibration_amd import synthetic as syn  # noqa: E402
from clip_calibration_amd.adapterfit import AdapterFitState  # noqa: E402
from clip_calibration_amd.augment import TrainPreprocess, sample_views  # noqa: E402
from clip_calibration_amd.model import build_model  # noqa: E402
from clip_calibration_amd.preprocess import CLIP_MEAN, CLIP_STD  # noqa: E402

H, W, N_PX = 375, 500, 224


def host_views(pool, pil_images, views, mean, std):
    """The host path: one view per task on the thread pool -> fp16 [V, 3, 224, 224] on the host."""
    from PIL import Image

    def one(v):
        b, top, left, h, w, flip = (int(x) for x in v)
        r = pil_images[b].crop((left, top, left + w, top + h)).resize((N_PX, N_PX), Image.BICUBIC)
        if flip:
            r = r.transpose(Image.FLIP_LEFT_RIGHT)
        x = torch.from_numpy(np.array(r)).permute(2, 0, 1).contiguous().to(torch.float32).div(255)
        return x.sub_(mean).div_(std).half()
    return torch.stack(list(pool.map(one, np.stack(views, axis=1))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=256)
    ap.add_argument("--step-batch", type=int, default=32)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--host-iters", type=int, default=3)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from PIL import Image
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    torch.set_num_threads(1)                                        # the pool's threads are the host's parallelism
    threads = max(1, min(16, a.threads))
    V = a.views
    gen = torch.Generator().manual_seed(0)
    views = sample_views([(H, W)] * V, generator=gen)
    tp = TrainPreprocess(N_PX)
    stream = torch.cuda.current_stream(dev)

    # ---- 1. the transform alone -------------------------------------------------------------------------------------------------------
    per_batch = V * H * W * 3
    nbuf = max(2, -(-(256 << 20) // per_batch) + 1)
    pool_d = torch.empty((nbuf, V, H, W, 3), dtype=torch.uint8, device=dev)
    pool_d.random_(0, 256, generator=torch.Generator(device=dev).manual_seed(0))
    for k in range(a.warmup):
        tp(pool_d[k % nbuf], views)
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(a.iters)]
    torch.cuda.synchronize()
    torch.cuda._sleep(200_000_000)                                  # the host queues every call while the device sleeps
    for k, (e0, e1) in enumerate(ev):
        e0.record(stream)
        tp(pool_d[(a.warmup + k) % nbuf], views)
        e1.record(stream)
    torch.cuda.synchronize()
    us = sorted(e0.elapsed_time(e1) * 1e3 for e0, e1 in ev)
    host_imgs = pool_d[0].cpu().numpy()
    pil_images = [Image.fromarray(host_imgs[i]) for i in range(V)]
    mean, std = torch.tensor(CLIP_MEAN)[:, None, None], torch.tensor(CLIP_STD)[:, None, None]
    with ThreadPoolExecutor(threads) as pool:
        same = torch.equal(host_views(pool, pil_images, views, mean, std), tp(pool_d[0], views).cpu())
        host_s = []
        for _ in range(a.host_iters):
            t0 = time.perf_counter()
            host_views(pool, pil_images, views, mean, std)
            host_s.append(time.perf_counter() - t0)
    transform = {"views": V, "H": H, "W": W, "n_px": N_PX, "filter": "bicubic", "out_dtype": "fp16", "calls": a.iters,
                 "device_us_median": round(statistics.median(us), 1), "device_us_min": round(us[0], 1), "device_us_max": round(us[-1], 1),
                 "input_pool_mib": round(nbuf * per_batch / 2 ** 20), "host_threads": threads,
                 "host_us_median": round(statistics.median(host_s) * 1e6), "host_us_min": round(min(host_s) * 1e6),
                 "host_passes": a.host_iters, "host_equals_device_bitwise": bool(same)}
    print(json.dumps(transform), flush=True)
    del pool_d
    torch.cuda.empty_cache()

    # ---- 2. one training step ---------------------------------------------------------------------------------------------------------
    Bs = a.step_batch
    model = build_model(dict(syn.synthetic_state_dict("ViT-B/16", seed=0)), {"trainer": "CoOp"}).cuda()
    E, C = int(model.visual.output_dim), 100
    g = torch.Generator().manual_seed(1)
    text = torch.nn.functional.normalize(torch.randn(C, E, generator=g), dim=1).to(dev)
    w1, w2 = (torch.randn(E // 4, E, generator=g) * 0.02).to(dev), (torch.randn(E, E // 4, generator=g) * 0.02).to(dev)
    labels = (torch.arange(Bs) % C).to(dev)
    lr = torch.full((1,), 0.002, dtype=torch.float32, device=dev)
    imgs_d = torch.from_numpy(host_imgs[:Bs]).to(dev)
    shapes = [(H, W)] * Bs

    def device_step(st):
        x = tp(imgs_d, sample_views(shapes, generator=gen))
        st.step(model.image_features_f32(x), labels, lr)

    def host_step(st, pool):
        x = host_views(pool, pil_images[:Bs], sample_views(shapes, generator=gen), mean, std)
        st.step(model.image_features_f32(x.pin_memory().to(dev, non_blocking=True)), labels, lr)

    def timed(step):
        with torch.no_grad():
            for _ in range(a.warmup):
                step()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.iters):
                step()
            torch.cuda.synchronize()
        return (time.perf_counter() - t0) / a.iters * 1e3

    with ThreadPoolExecutor(threads) as pool:
        rounds = []
        for _ in range(3):                                          # the two arms alternate in one process
            st_d, st_h = AdapterFitState(text, w1, w2), AdapterFitState(text, w1, w2)
            rounds.append((timed(lambda: device_step(st_d)), timed(lambda: host_step(st_h, pool))))
    step = {"batch": Bs, "model": "ViT-B/16 (synthetic weights)", "classes": C, "steps_per_round": a.iters, "rounds": len(rounds),
            "device_transform_ms_per_step": [round(r[0], 3) for r in rounds], "host_transform_ms_per_step": [round(r[1], 3) for r in rounds],
            "device_transform_ms_median": round(statistics.median(r[0] for r in rounds), 3),
            "host_transform_ms_median": round(statistics.median(r[1] for r in rounds), 3), "host_threads": threads}
    print(json.dumps(step), flush=True)
    res = {"tool": "tools/augment_bench.py", "device": torch.cuda.get_device_name(dev), "transform": transform, "train_step": step}
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
