"""What batch sharding adds to a VPT and a MaPLe training step (``shard=`` on clip_calibration_amd.vptfit / maplefit, csrc/shard_train.hip,
DESIGN.md "Batch-sharded image-tower fits").  Measurement only; bench.py does not run it.

1. The world-1 sharded step against the unsharded step of the same model, taking turns in one run, on the first shape of
   tools/maplefit_bench.py (ViT-B/16, n_ctx 2, depth 9, batch 4, 100 classes) and of tools/vptfit_bench.py (ViT-B/16, n_ctx 8, depth 12,
   batch 4, 100 classes): the median, minimum and maximum of --iters windows after --warmup untimed steps, one step between two device
   events with a synchronisation behind it.  World 1 over a ``LocalGather`` adds the send block's copy, the rank mean (or the fused
   gathered step) and the losses' mean to the unsharded launches; the overhead is reported beside the run's own spread.
2. clipmi_block_rank_mean alone at G = 2, 4, 8 on MaPLe's block and on VPT's (plus the losses' float), beside a device-to-device copy of
   the G gathered blocks timed in the same run, taking turns.  The kernel reads G blocks and writes one, the copy reads G and writes G:
   both are reported as bytes moved per second, and the kernel as a fraction of the copy's rate.

World sizes above 1 are NOT measured by this tool on any box: it runs in one process on one GPU and claims no speed-up.

Usage: python tools/batchshard_bench.py [--iters 5] [--warmup 2] [--out profiles/batchshard_bench.json]"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from clip_calibration_amd import coopfit, maplefit, ops, synthetic as syn, vptfit  # noqa: E402
from clip_calibration_amd.model import build_model  # noqa: E402

WORLDS = (2, 4, 8)
KERNEL_REPEATS = 20     # launches per timed window of the kernel and of the copy: one launch of the small block is shorter than an event's resolution


def events(n):
    return [torch.cuda.Event(enable_timing=True) for _ in range(n)]


def spread(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v)}


def in_turn(steps, iters, warmup, repeats=1):
    """{name: spread of ms per call} of the callables in ``steps``, which take their windows in turn: a drift of the machine reaches all alike."""
    ms = {name: [] for name in steps}
    for k in range(warmup + iters):
        for name, fn in steps.items():
            a, b = events(2)
            a.record()
            for _ in range(repeats):
                fn()
            b.record()
            torch.cuda.synchronize()
            if k >= warmup:
                ms[name].append(a.elapsed_time(b) / repeats)
    return {name: spread(v) for name, v in ms.items()}


def step_pair(name, make, batch, lr, a):
    base, one = make(None), make(coopfit.Shard(1, 0, coopfit.LocalGather(1)))
    x, y = batch
    t = in_turn({"baseline": lambda: base.step(x, y, lr), "sharded": lambda: one.step(x, y, lr)}, a.iters, a.warmup)
    same = bool(torch.equal(base._master(), one._master()) and torch.equal(base.buf, one.buf))
    over = t["sharded"]["median"] - t["baseline"]["median"]
    noise = max(t["baseline"]["max"] - t["baseline"]["min"], t["sharded"]["max"] - t["sharded"]["min"])
    r = {"fit": name, "world": 1, "block_floats": base._master().numel(), "baseline_step_ms": t["baseline"], "sharded_step_ms": t["sharded"],
         "overhead_ms": over, "overhead_share": over / t["baseline"]["median"], "largest_spread_ms": noise, "overhead_within_the_spread": abs(over) <= noise,
         "same_bits_as_baseline": same}
    print(json.dumps(r), flush=True)
    return r


def kernel_rows(name, total, a):
    rows = []
    for G in WORLDS:
        gathered = torch.randn(G, (total + 3) // 4 * 4, device="cuda")      # the step's receive block: rows of whole 16-byte vectors
        out, copy = torch.empty(total, device="cuda"), torch.empty_like(gathered)
        t = in_turn({"mean": lambda: ops.block_rank_mean(gathered, total, out), "copy": lambda: copy.copy_(gathered)}, a.iters, a.warmup, KERNEL_REPEATS)
        mean_rate = (G + 1) * total * 4 / (t["mean"]["median"] * 1e-3) / 1e9
        copy_rate = 2 * gathered.numel() * 4 / (t["copy"]["median"] * 1e-3) / 1e9
        r = {"block": name, "world": G, "floats": total, "rank_mean_ms": t["mean"], "copy_ms": t["copy"], "rank_mean_GBps": mean_rate, "copy_GBps": copy_rate,
             "rank_mean_share_of_copy_rate": mean_rate / copy_rate}
        print(json.dumps(r), flush=True)
        rows.append(r)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import maplefit_bench as mb
    import vptfit_bench as vb
    torch.cuda.set_device(0)
    g = torch.Generator().manual_seed(1)
    sd = syn.synthetic_state_dict(mb.GEOM, seed=0)
    out = {"geometry": mb.GEOM, "device": torch.cuda.get_device_name(0), "gpus_on_the_box": torch.cuda.device_count(), "iters": a.iters, "warmup": a.warmup,
           "kernel_launches_per_window": KERNEL_REPEATS, "worlds_above_1": "not measured: this tool runs one process on one GPU and claims no speed-up",
           "steps": [], "rank_mean": []}
    images = torch.randn(4, 3, 224, 224, generator=g).half().cuda()
    # MaPLe, the first shape of tools/maplefit_bench.py
    Cn = mb.CLASSES[0]
    model = build_model(dict(sd), {"trainer": "MaPLe", "vision_depth": 0, "language_depth": 0, "vision_ctx": 0, "language_ctx": 0, "maple_length": mb.N_CTX}).cuda()
    pl = maplefit.init_learner_params(model, mb.N_CTX, mb.DEPTH, seed=0)
    ids = syn.synthetic_token_ids(Cn, mb.GEOM, seed=0)
    labels = torch.randint(0, Cn, (4,), generator=g).cuda()
    r = step_pair("maple", lambda sh: maplefit.MaPLeFitState(model, ids, pl, shard=sh), (images, labels), torch.full((1,), mb.LR, device="cuda"), a)
    out["steps"].append(dict(r, n_ctx=mb.N_CTX, depth=mb.DEPTH, batch=4, classes=Cn))
    maple_floats = r["block_floats"]
    del model
    # VPT, the first shape of tools/vptfit_bench.py
    vmodel = build_model(dict(sd), {"trainer": "VPT", "vision_depth": vb.DEPTH, "vision_ctx": vb.N_CTX, "language_depth": 0, "language_ctx": 0}).cuda()
    text = torch.randn(vb.CLASSES, syn.GEOMETRIES[vb.GEOM].embed_dim, generator=g).cuda()
    labels = torch.randint(0, vb.CLASSES, (4,), generator=g).cuda()
    r = step_pair("vpt", lambda sh: vptfit.VPTFitState(vmodel, text, shard=sh), (images, labels), torch.full((1,), 0.0025, device="cuda"), a)
    out["steps"].append(dict(r, n_ctx=vb.N_CTX, depth=vb.DEPTH, batch=4, classes=vb.CLASSES))
    vpt_floats = r["block_floats"]
    out["rank_mean"] += kernel_rows("maple", maple_floats + 1, a) + kernel_rows("vpt", vpt_floats + 1, a)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
