"""Time of TempScaling's fit from cached cosine logits (clip_calibration_amd/tempfit.py, csrc/tempscale.hip): 20 epochs in batches of
100 over (N, C) = (2 000, 500) and (25 000, 1 000), next to the same job done the way it had to be done before -- a torch loop on the GPU
over the same cached logits: scale.exp() * cosine[batch], F.cross_entropy, backward, torch.optim.SGD.step -- in the same process.
Both are timed between two events on the stream, the whole run at a time, after --warmup untimed runs; median of --repeats.
Measurement only; bench.py does not run it.
Usage: python tools/tempscale_bench.py [--out profiles/tempscale_bench.json]"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from clip_calibration_amd import ops, tempfit  # noqa: E402

INIT, EPOCHS, BATCH, MOMENTUM, WEIGHT_DECAY = 4.6052, 20, 100, 0.9, 5e-4


def split(n, C, seed):
    """Cosine logits around a class prototype, as a CLIP val split gives them."""
    rng = np.random.default_rng(seed)
    labels = rng.integers(0, C, n)
    cos = rng.normal(0.2, 0.035, (n, C)) * rng.uniform(0.6, 1.6, n)[:, None]
    cos[np.arange(n), labels] += rng.normal(0.07, 0.05, n)
    return np.clip(cos, -1, 1).astype(np.float32), labels.astype(np.int64)


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tempscale_bench.json"))
    a = ap.parse_args()
    props = torch.cuda.get_device_properties(0)
    res = {"device": f"{torch.cuda.get_device_name(0)} ({props.gcnArchName}, {props.multi_processor_count} CUs)", "epochs": EPOCHS,
           "batch": BATCH, "momentum": MOMENTUM, "weight_decay": WEIGHT_DECAY, "repeats": a.repeats, "warmup": a.warmup, "runs": []}
    for n, C in ((2000, 500), (25000, 1000)):
        cos, labels = split(n, C, 1)
        d_cos, d_lab = torch.from_numpy(cos).cuda(), torch.from_numpy(labels).cuda()
        rates = tempfit.cosine_warmup_schedule(0.05, EPOCHS)
        per_epoch = tempfit.steps_per_epoch(n, BATCH)
        steps = EPOCHS * per_epoch
        lr = torch.from_numpy(np.repeat(np.asarray(rates), per_epoch).astype(np.float32)).cuda()
        fresh = torch.tensor([INIT, 0, 0, 0], dtype=torch.float32).cuda()
        state = fresh.clone()

        def hip_fit():
            state.copy_(fresh)
            ops.tempscale_fit(d_cos, d_lab, state, lr, BATCH, EPOCHS, MOMENTUM, 0.0, WEIGHT_DECAY, False)

        scale = torch.nn.Parameter(torch.tensor(INIT, device="cuda"))

        def torch_fit():
            with torch.no_grad():
                scale.fill_(INIT)
            opt = torch.optim.SGD([scale], lr=1.0, momentum=MOMENTUM, weight_decay=WEIGHT_DECAY)
            for e in range(EPOCHS):
                opt.param_groups[0]["lr"] = rates[e]
                for k in range(per_epoch):
                    loss = F.cross_entropy(scale.exp() * d_cos[k * BATCH:(k + 1) * BATCH], d_lab[k * BATCH:(k + 1) * BATCH])
                    opt.zero_grad()
                    loss.backward()
                    opt.step()

        hip = timed(hip_fit, a.warmup, a.repeats)
        theta_hip = float(state[0])
        tor = timed(torch_fit, a.warmup, a.repeats)
        theta_torch = float(scale.detach())
        run = {"n": n, "classes": C, "steps": steps, "hip_fit_s_median": statistics.median(hip), "hip_fit_s_min": min(hip),
               "hip_step_us_median": statistics.median(hip) / steps * 1e6, "torch_loop_s_median": statistics.median(tor),
               "torch_loop_s_min": min(tor), "torch_step_us_median": statistics.median(tor) / steps * 1e6,
               "torch_over_hip": statistics.median(tor) / statistics.median(hip), "theta_hip": theta_hip, "theta_torch": theta_torch}
        res["runs"].append(run)
        print(json.dumps(run), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
