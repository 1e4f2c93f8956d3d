"""Time of TaskRes' training on cached image features (clip_calibration_amd/taskresfit.py, csrc/taskres_train.hip): 5 epochs of Adam in
batches of 256 with E = 512 over (N, C) = (1 600, 100) and (16 000, 1 000), three ways in the same process on the same GPU:
  fit       ops.taskres_fit: every step of the run enqueued by one call
  per_step  TaskResFitState.step batch by batch on row slices, the rate in a device tensor (what a caller with a random train transform
            does behind its image tower)
  torch     the plain loop: the restated forward, F.cross_entropy, backward, torch.optim.Adam.step on the residuals
Each is timed between two events on the stream, the whole run at a time (30 and 310 steps), after --warmup untimed runs of the same
shape.  The three ways are INTERLEAVED: repeat i runs fit, per_step, torch one after the other, so a clock or neighbour change meets all
three alike; median, minimum and maximum of --repeats are recorded.  What the timed region of each holds besides the steps: fit -- the
reset of the residuals and the two moments; per_step -- the construction of the state and, per step, three slices; torch -- the reset, a
new optimiser and the per-step slices.  The device's current engine clock is read before and after (0 where it cannot be read).  The
three kernels' own times come from one further fit under torch.profiler (mean device time per launch by kernel name; an error string
where the profiler gives no device records).  The largest difference of the final residuals between the HIP run and the torch loop is
recorded beside the times.  Measurement only; bench.py does not run it.
Usage: python tools/taskresfit_bench.py [--out profiles/taskresfit_bench.json]"""
import argparse
import json
import math
import os
import re
import statistics
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from clip_calibration_amd import ops, taskresfit, tempfit  # noqa: E402

E, EPOCHS, BATCH, ALPHA, LOGIT_SCALE, LR, BETAS, EPS, WEIGHT_DECAY = 512, 5, 256, 0.5, 4.6052, 2e-4, (0.9, 0.999), 1e-8, 5e-4


def split(n, C, seed):
    """Raw features around a class prototype, un-normalised base text features and labels."""
    rng = np.random.default_rng(seed)
    T = rng.normal(size=(C, E))
    labels = rng.integers(0, C, n)
    f = 10.0 * (0.3 * T[labels] / np.linalg.norm(T[labels], axis=1, keepdims=True) + rng.normal(size=(n, E)) / math.sqrt(E))
    return tuple(torch.from_numpy(a.astype(np.float32)).cuda() for a in (f, T)) + (torch.from_numpy(labels.astype(np.int64)).cuda(),)


def clock_mhz():
    try:
        return int(torch.cuda.clock_rate())
    except Exception:      # no SMI library beside torch: the figure is context, not a result
        return 0


def once(run):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    run()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e-3


def interleaved(runs, warmup, repeats):
    for _ in range(warmup):
        for run in runs.values():
            run()
    torch.cuda.synchronize()
    times = {k: [] for k in runs}
    for _ in range(repeats):
        for k, run in runs.items():
            times[k].append(once(run))
    return times


def kernel_times(run):
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            run()
            torch.cuda.synchronize()
        out = {}
        for ev in prof.key_averages():
            name = re.search(r"taskres_\w+", ev.key)
            if name:
                total = getattr(ev, "device_time_total", None)
                if total is None:
                    total = getattr(ev, "cuda_time_total", 0.0)
                out[name.group(0)] = {"launches": ev.count, "mean_us": total / max(ev.count, 1)}
        return out or "the profiler recorded no taskres kernel"
    except Exception as e:      # the figure is a breakdown, not a result: say why it is missing
        return f"{type(e).__name__}: {e}"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "taskresfit_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("taskresfit_bench: needs a GPU; nothing is measured without one")
    props = torch.cuda.get_device_properties(0)
    res = {"device": f"{torch.cuda.get_device_name(0)} ({props.gcnArchName}, {props.multi_processor_count} CUs)", "E": E, "epochs": EPOCHS,
           "batch": BATCH, "optimizer": "adam", "betas": BETAS, "eps": EPS, "weight_decay": WEIGHT_DECAY, "alpha": ALPHA, "repeats": a.repeats,
           "warmup": a.warmup, "order": "interleaved: fit, per_step, torch in every repeat", "runs": []}
    scale = float(np.float32(math.exp(LOGIT_SCALE)))
    res["clock_mhz_before"] = clock_mhz()
    for n, C in ((1600, 100), (16000, 1000)):
        f, base, y = split(n, C, 1)
        rates = tempfit.cosine_warmup_schedule(LR, EPOCHS)
        per_epoch = tempfit.steps_per_epoch(n, BATCH, True)
        steps = EPOCHS * per_epoch
        lr = torch.from_numpy(np.repeat(np.asarray(rates), per_epoch).astype(np.float32)).cuda()
        r, m, v = (torch.zeros_like(base) for _ in range(3))

        def hip_fit():
            r.zero_()
            m.zero_()
            v.zero_()
            ops.taskres_fit(f, y, base, r, m, v, lr, ALPHA, scale, BATCH, EPOCHS, "adam", WEIGHT_DECAY, betas=BETAS, eps=EPS, drop_last=True)

        last = {}

        def hip_steps():
            st = taskresfit.TaskResFitState(base, None, ALPHA, LOGIT_SCALE, "adam", BETAS, EPS, WEIGHT_DECAY)
            for k in range(steps):
                i = (k % per_epoch) * BATCH
                st.step(f[i:i + BATCH], y[i:i + BATCH], lr[k:k + 1])
            last["state"] = st

        p = torch.nn.Parameter(torch.zeros_like(base))

        def torch_fit():
            with torch.no_grad():
                p.zero_()
            opt = torch.optim.Adam([p], lr=1.0, betas=BETAS, eps=EPS, weight_decay=WEIGHT_DECAY)
            for e in range(EPOCHS):
                opt.param_groups[0]["lr"] = rates[e]
                for k in range(per_epoch):
                    x = f[k * BATCH:(k + 1) * BATCH]
                    t = base + ALPHA * p
                    z = scale * (x / x.norm(dim=-1, keepdim=True)) @ (t / t.norm(dim=-1, keepdim=True)).t()
                    loss = F.cross_entropy(z, y[k * BATCH:(k + 1) * BATCH])
                    opt.zero_grad()
                    loss.backward()
                    opt.step()

        times = interleaved({"fit": hip_fit, "per_step": hip_steps, "torch": torch_fit}, a.warmup, a.repeats)
        st = last["state"]
        med = {k: statistics.median(t) for k, t in times.items()}
        run = {"n": n, "classes": C, "steps": steps}
        for k, t in times.items():
            run.update({f"{k}_s_median": med[k], f"{k}_s_min": min(t), f"{k}_s_max": max(t), f"{k}_step_us_median": med[k] / steps * 1e6})
        run.update({"torch_over_fit": med["torch"] / med["fit"], "torch_over_per_step": med["torch"] / med["per_step"],
                    "per_step_equals_fit_bits": bool(torch.equal(st.residuals, r)),
                    "max_abs_r_fit_minus_torch": float((r - p.detach()).abs().max()), "max_abs_r_moved": float(r.abs().max()),
                    "kernels": kernel_times(hip_fit)})
        res["runs"].append(run)
        print(json.dumps(run), flush=True)
    res["clock_mhz_after"] = clock_mhz()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
