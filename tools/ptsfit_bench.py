"""Time of the PTS fit and of the per-row apply (clip_calibration_amd/ptsfit.py, csrc/pts.hip) at TempScaling's two shapes, (N, C) =
(2 000, 500) and (25 000, 1 000) in batches of 100, next to a torch autograd loop on the GPU over the same cached logits in the same
process: the top-k features once, then per step the MLP, softmax(z / T), the mean squared error, backward and torch.optim's step.
Whole runs are timed between two events on the stream after --warmup untimed runs; median, minimum and maximum of --repeats.  The time
per step does not depend on the number of epochs, so --epochs is short.  Measurement only; bench.py does not run it.
Usage: python tools/ptsfit_bench.py [--out profiles/ptsfit_bench.json]"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from clip_calibration_amd import _lib, fitloop, ops, ptsfit  # noqa: E402

BATCH, MOMENTUM, WEIGHT_DECAY, NET = 100, 0.9, 5e-4, (2, 5, 10)


def split(n, C, seed):
    """Scaled logits around a class prototype, as a CLIP val split gives them: 100 x cosine."""
    rng = np.random.default_rng(seed)
    labels = rng.integers(0, C, n)
    cos = rng.normal(0.2, 0.035, (n, C)) * rng.uniform(0.6, 1.6, n)[:, None]
    cos[np.arange(n), labels] += rng.normal(0.07, 0.05, n)
    return (100.0 * np.clip(cos, -1, 1)).astype(np.float32), labels.astype(np.int64)


def timed(run, warmup, repeats):
    for _ in range(warmup):
        run()
    torch.cuda.synchronize()
    times = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        run()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1) * 1e-3)
    return times


def stats(times, per=1):
    return {"median": statistics.median(times) / per, "min": min(times) / per, "max": max(times) / per}


def torch_loss(block, f, z, y):
    L, n, K = NET
    p = ptsfit.split_params(block, L, n, K)
    h = f
    for l in range(1, L + 1):
        h = torch.relu(h @ p[f"W{l}"].T + p[f"b{l}"])
    T = (h @ p["w_out"] + p["b_out"][0]).abs().clamp(1e-12, 1e12)
    prob = torch.softmax(z / T[:, None], dim=1)
    onehot = torch.nn.functional.one_hot(y, z.shape[1]).to(prob.dtype)
    return ((prob - onehot) ** 2).mean(dim=1).mean()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--epochs", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ptsfit_bench.json"))
    a = ap.parse_args()
    L, n_nodes, K = NET
    P = ptsfit.param_count(L, n_nodes, K)
    props = torch.cuda.get_device_properties(0)
    res = {"device": f"{torch.cuda.get_device_name(0)} ({props.gcnArchName}, {props.multi_processor_count} CUs)", "epochs": a.epochs,
           "batch": BATCH, "net": NET, "momentum": MOMENTUM, "weight_decay": WEIGHT_DECAY, "repeats": a.repeats, "warmup": a.warmup, "runs": []}
    start = ptsfit.init_params(L, n_nodes, K, generator=torch.Generator().manual_seed(0))
    start[-1] += 1.0
    for N, C in ((2000, 500), (25000, 1000)):
        z, labels = split(N, C, 1)
        d_z, d_lab = torch.from_numpy(z).cuda(), torch.from_numpy(labels).cuda()
        rates = fitloop.cosine_warmup_schedule(0.05, a.epochs)
        per_epoch = fitloop.steps_per_epoch(N, BATCH)
        steps = a.epochs * per_epoch
        lr = torch.from_numpy(np.repeat(np.asarray(rates), per_epoch).astype(np.float32)).cuda()
        fresh = torch.zeros(3 * P + 2, dtype=torch.float32).cuda()
        fresh[:P] = start.cuda()
        state = fresh.clone()
        out = torch.empty_like(d_z)
        for name, opt_id in (("sgd", _lib.OPTIM_SGD), ("adam", _lib.OPTIM_ADAM)):
            def hip_fit():
                state.copy_(fresh)
                ops.pts_fit(d_z, d_lab, state, L, n_nodes, K, lr, BATCH, a.epochs, opt_id, MOMENTUM, 0.0, WEIGHT_DECAY, False)

            block = torch.nn.Parameter(start.clone().cuda())

            def torch_fit():
                with torch.no_grad():
                    block.copy_(fresh[:P])
                opt = (torch.optim.SGD([block], lr=1.0, momentum=MOMENTUM, weight_decay=WEIGHT_DECAY) if name == "sgd" else
                       torch.optim.Adam([block], lr=1.0, weight_decay=WEIGHT_DECAY))
                feat = torch.sort(d_z, dim=1, descending=True).values[:, :K].contiguous()
                for e in range(a.epochs):
                    opt.param_groups[0]["lr"] = rates[e]
                    for k in range(per_epoch):
                        lo, hi = k * BATCH, (k + 1) * BATCH
                        loss = torch_loss(block, feat[lo:hi], d_z[lo:hi], d_lab[lo:hi])
                        opt.zero_grad()
                        loss.backward()
                        opt.step()

            hip = timed(hip_fit, a.warmup, a.repeats)
            hip_block = state[:P].clone()
            tor = timed(torch_fit, a.warmup, a.repeats)
            run = {"n": N, "classes": C, "optimizer": name, "steps": steps, "hip_fit_s": stats(hip), "hip_step_us": stats(hip, steps * 1e-6),
                   "torch_loop_s": stats(tor), "torch_step_us": stats(tor, steps * 1e-6),
                   "torch_over_hip": statistics.median(tor) / statistics.median(hip),
                   "max_abs_param_difference": float((hip_block - block.detach()).abs().max())}
            res["runs"].append(run)
            print(json.dumps(run), flush=True)
        topk = timed(lambda: ops.pts_topk(d_z, K), a.warmup, a.repeats)
        apply = timed(lambda: ops.pts_apply(d_z, state[:P], L, n_nodes, K, out=out), a.warmup, a.repeats)
        run = {"n": N, "classes": C, "pts_topk_us": stats(topk, 1e-6), "pts_apply_us": stats(apply, 1e-6),
               "pts_apply_GBps": 2 * d_z.numel() * 4 / statistics.median(apply) * 1e-9}
        res["runs"].append(run)
        print(json.dumps(run), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
