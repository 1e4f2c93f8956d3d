"""Time of CLIP-Adapter's training on cached image features (clip_calibration_amd/adapterfit.py, csrc/adapter_train.hip): 5 epochs in
batches of 32 with E = 512, H = 128 over (N, C) = (1 600, 100) and (16 000, 1 000), three ways in the same process on the same GPU:
  fit       ops.adapter_fit: every step of the run enqueued by one call
  per_step  AdapterFitState.step batch by batch on gathered rows, the rate in a device tensor (what a caller with a random train
            transform does behind its image tower)
  torch     the plain loop: the restated forward, F.cross_entropy, backward, torch.optim.SGD.step on the two matrices
Each is timed between two events on the stream, the whole run at a time (0.25 to 2.5 thousand steps), after --warmup untimed runs of
the same shape; median and minimum of --repeats, the three ways one after the other in one process.  What the timed region of each
holds besides the steps: fit -- the reset of the two matrices; per_step -- the construction of the state (two weight copies, two zeroed
buffers) and, per step, three slices (features, labels, the step's rate in the device array); torch -- the reset, a new optimiser and the
per-step slices.  The device's current engine clock is read before and after (torch.cuda.clock_rate, 0 where it cannot be read) and
recorded; nothing else runs in the process.  The largest
difference of the final weights between the HIP run and the torch loop is recorded beside the times.  Measurement only; bench.py does
not run it.
Usage: python tools/adapterfit_bench.py [--out profiles/adapterfit_bench.json]"""
import argparse
import json
import math
import os
import statistics
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from clip_calibration_amd import adapterfit, ops, tempfit  # noqa: E402

E, H, EPOCHS, BATCH, RATIO, LOGIT_SCALE, LR, MOMENTUM, WEIGHT_DECAY = 512, 128, 5, 32, 0.2, 4.6052, 0.002, 0.9, 5e-4


def split(n, C, seed):
    """Raw features around a class prototype, L2-normalised text features, labels and a fresh bottleneck."""
    rng = np.random.default_rng(seed)
    T = rng.normal(size=(C, E))
    T /= np.linalg.norm(T, axis=1, keepdims=True)
    labels = rng.integers(0, C, n)
    f = 10.0 * (0.3 * T[labels] + rng.normal(size=(n, E)) / math.sqrt(E))
    w1 = rng.uniform(-1, 1, (H, E)) / math.sqrt(E)
    w2 = rng.uniform(-1, 1, (E, H)) / math.sqrt(H)
    return tuple(torch.from_numpy(a.astype(np.float32)).cuda() for a in (f, T, w1, w2)) + (torch.from_numpy(labels.astype(np.int64)).cuda(),)


def clock_mhz():
    try:
        return int(torch.cuda.clock_rate())
    except Exception:      # no SMI library beside torch: the figure is context, not a result
        return 0


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "adapterfit_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("adapterfit_bench: needs a GPU; nothing is measured without one")
    props = torch.cuda.get_device_properties(0)
    res = {"device": f"{torch.cuda.get_device_name(0)} ({props.gcnArchName}, {props.multi_processor_count} CUs)", "E": E, "H": H,
           "epochs": EPOCHS, "batch": BATCH, "momentum": MOMENTUM, "weight_decay": WEIGHT_DECAY, "repeats": a.repeats, "warmup": a.warmup,
           "runs": []}
    scale = float(np.float32(math.exp(LOGIT_SCALE)))
    res["clock_mhz_before"] = clock_mhz()
    for n, C in ((1600, 100), (16000, 1000)):
        f, T, w1_0, w2_0, y = split(n, C, 1)
        rates = tempfit.cosine_warmup_schedule(LR, EPOCHS)
        per_epoch = tempfit.steps_per_epoch(n, BATCH, True)
        steps = EPOCHS * per_epoch
        lr = torch.from_numpy(np.repeat(np.asarray(rates), per_epoch).astype(np.float32)).cuda()
        w1, w2, m1, m2 = w1_0.clone(), w2_0.clone(), torch.zeros_like(w1_0), torch.zeros_like(w2_0)

        def hip_fit():
            w1.copy_(w1_0)
            w2.copy_(w2_0)
            ops.adapter_fit(f, y, T, w1, w2, m1, m2, lr, RATIO, scale, BATCH, EPOCHS, MOMENTUM, 0.0, WEIGHT_DECAY, False, None, True)

        last = {}

        def hip_steps():
            st = adapterfit.AdapterFitState(T, w1_0, w2_0, RATIO, LOGIT_SCALE, MOMENTUM, 0.0, WEIGHT_DECAY)
            for k in range(steps):
                i = (k % per_epoch) * BATCH
                st.step(f[i:i + BATCH], y[i:i + BATCH], lr[k:k + 1])
            last["state"] = st

        p1, p2 = torch.nn.Parameter(w1_0.clone()), torch.nn.Parameter(w2_0.clone())

        def torch_fit():
            with torch.no_grad():
                p1.copy_(w1_0)
                p2.copy_(w2_0)
            opt = torch.optim.SGD([p1, p2], lr=1.0, momentum=MOMENTUM, weight_decay=WEIGHT_DECAY)
            for e in range(EPOCHS):
                opt.param_groups[0]["lr"] = rates[e]
                for k in range(per_epoch):
                    x = f[k * BATCH:(k + 1) * BATCH]
                    g = RATIO * torch.relu(torch.relu(x @ p1.t()) @ p2.t()) + (1 - RATIO) * x
                    loss = F.cross_entropy(scale * (g / g.norm(dim=-1, keepdim=True)) @ T.t(), y[k * BATCH:(k + 1) * BATCH])
                    opt.zero_grad()
                    loss.backward()
                    opt.step()

        hip = timed(hip_fit, a.warmup, a.repeats)
        per = timed(hip_steps, a.warmup, a.repeats)
        tor = timed(torch_fit, a.warmup, a.repeats)
        st = last["state"]
        run = {"n": n, "classes": C, "steps": steps,
               "fit_s_median": statistics.median(hip), "fit_s_min": min(hip), "fit_step_us_median": statistics.median(hip) / steps * 1e6,
               "per_step_s_median": statistics.median(per), "per_step_s_min": min(per),
               "per_step_step_us_median": statistics.median(per) / steps * 1e6,
               "torch_loop_s_median": statistics.median(tor), "torch_loop_s_min": min(tor),
               "torch_step_us_median": statistics.median(tor) / steps * 1e6,
               "torch_over_fit": statistics.median(tor) / statistics.median(hip), "torch_over_per_step": statistics.median(tor) / statistics.median(per),
               "per_step_equals_fit_bits": bool(torch.equal(st.w1, w1) and torch.equal(st.w2, w2)),
               "max_abs_w1_fit_minus_torch": float((w1 - p1.detach()).abs().max()), "max_abs_w2_fit_minus_torch": float((w2 - p2.detach()).abs().max()),
               "max_abs_w1_moved": float((w1 - w1_0).abs().max())}
        res["runs"].append(run)
        print(json.dumps(run), flush=True)
    res["clock_mhz_after"] = clock_mhz()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
