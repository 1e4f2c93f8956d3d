"""References of the prompt fits' Adam / AdamW step (csrc/optim_step.hip): ``emulate_step``, an fp32 numpy restatement of both rules in
the kernel's order of operations (every product and sum rounded to fp32 where the kernel rounds it: train_rules.h's adam_element and
adamw_element are compiled with contraction off), and ``adam_rule64`` / ``adamw_rule64``, the float64 form of torch.optim.Adam's and
torch.optim.AdamW's rule.  tests/test_optimstep_cpu.py holds both to torch on the CPU; tests/test_gpu_optimstep_ops.py holds the kernels to
``emulate_step`` bit for bit.

The criterion against torch (``within_torch``): the largest distance of an fp32 result from the float64 result is at most TWICE the
largest distance of torch's own fp32 CPU run of the same steps from float64, plus one fp32 ulp of the largest float64 value."""
import math

import numpy as np
import torch

F = np.float32
SEAMS = (1, 255, 256, 257, 1000)          # around the 256-thread workgroups (SCALED_THREADS of csrc/model.h)
BETAS, EPS = (0.9, 0.999), 1e-8
LR = 0.002


def threads():
    """SCALED_THREADS as csrc/model.h sets it."""
    import os
    import re
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "clip_calibration_amd", "csrc", "model.h")
    return int(re.search(r"constexpr int SCALED_THREADS = (\d+);", open(path).read()).group(1))


def bias_table(betas, steps):
    """What fitloop.adam_bias_table must equal: Python's own doubles."""
    b1, b2 = betas
    return np.array([[1 - b1 ** t, math.sqrt(1 - b2 ** t)] for t in range(1, steps + 1)], np.float64)


def make_block(total, seed=0, steps=5):
    """(params [total], grads [steps, total]) fp32: parameters of order 1; gradients of mixed magnitude with, where the block has room,
    exact zeros, a denormal and values of magnitude 1e-8 and 1e4 at fixed places, the block's first and last element among them."""
    rng = np.random.default_rng(seed + 7919 * total)
    w = rng.standard_normal(total).astype(F)
    g = (rng.standard_normal((steps, total)) * 10.0 ** rng.integers(-3, 1, (steps, total))).astype(F)
    special = [F(0.0), F(1e-40), F(1e-8), F(-1e4), F(1e4), F(-1e-8), F(-0.0)]
    for s in range(steps):
        places = [(37 * k + s) % total for k in range(1, len(special) - 1)] + [total - 1, 0]
        for k, i in enumerate(places):                    # a block of one element keeps the last one written, another special every step
            g[s, i] = special[(k + s) % len(special)]
    return w, g


def emulate_step(w, m, v, grad, t, lr, grad_scale=1.0, betas=BETAS, eps=EPS, weight_decay=0.0, decoupled=False):
    """One clipmi_block_step_adam on fp32 arrays, in the kernel's order: returns (w, m, v, unscaled gradient)."""
    b1, b2 = betas
    lr = F(lr)
    omb1, fb2, omb2, feps, wd = F(1.0 - b1), F(b2), F(1.0 - b2), F(eps), F(weight_decay)
    bc1, bc2s = 1 - b1 ** t, math.sqrt(1 - b2 ** t)
    with np.errstate(all="ignore"):
        g = (grad.astype(F) * (F(1.0) / F(grad_scale))).astype(F)
        g_out = g
        p = w.astype(F)
        if wd != 0:
            if decoupled:
                p = (p * F(1.0 - float(lr) * float(wd))).astype(F)
            else:
                g = (g + (wd * p).astype(F)).astype(F)
        m1 = (m + ((g - m).astype(F) * omb1).astype(F)).astype(F)
        v1 = ((fb2 * v).astype(F) + ((omb2 * g).astype(F) * g).astype(F)).astype(F)
        step = F(float(lr) / bc1)
        denom = ((np.sqrt(v1).astype(F) / F(bc2s)).astype(F) + feps).astype(F)
        w1 = (p - ((step * m1).astype(F) / denom).astype(F)).astype(F)
    return w1, m1, v1, g_out


def emulate_run(w, grads, lr=LR, grad_scale=1.0, t0=1, m=None, v=None, **rule):
    """``emulate_step`` over grads [steps, total] at step numbers t0, t0 + 1, ..: the list of (w, m, v) after every step."""
    m = np.zeros_like(w) if m is None else m
    v = np.zeros_like(w) if v is None else v
    out = []
    for k, g in enumerate(grads):
        w, m, v, _ = emulate_step(w, m, v, g, t0 + k, lr, grad_scale, **rule)
        out.append((w, m, v))
    return out


def adam_rule64(w, g, m, v, t, lr, betas=BETAS, eps=EPS, weight_decay=0.0):
    """torch.optim.Adam's rule (no amsgrad) in float64, step number t >= 1: returns (w, m, v)."""
    b1, b2 = betas
    g = g + weight_decay * w
    m = m + (g - m) * (1 - b1)
    v = b2 * v + (1 - b2) * g * g
    w = w - (lr / (1 - b1 ** t)) * m / (np.sqrt(v) / math.sqrt(1 - b2 ** t) + eps)
    return w, m, v


def adamw_rule64(w, g, m, v, t, lr, betas=BETAS, eps=EPS, weight_decay=0.0):
    """torch.optim.AdamW's rule in float64: the decay first, then Adam's rule without weight decay."""
    return adam_rule64(w * (1 - lr * weight_decay), g, m, v, t, lr, betas, eps, 0.0)


def rule64_run(w, grads, lr=LR, betas=BETAS, eps=EPS, weight_decay=0.0, decoupled=False):
    """The float64 form over grads [steps, total]: the parameters after every step, float64 [steps, total]."""
    rule = adamw_rule64 if decoupled else adam_rule64
    w, m, v = w.astype(np.float64), np.zeros(w.shape), np.zeros(w.shape)
    out = []
    for k, g in enumerate(grads):
        w, m, v = rule(w, g.astype(np.float64), m, v, k + 1, lr, betas, eps, weight_decay)
        out.append(w)
    return np.stack(out)


def torch_run(w, grads, dtype, lr=LR, betas=BETAS, eps=EPS, weight_decay=0.0, decoupled=False):
    """torch.optim.Adam / AdamW itself on the CPU in ``dtype`` (single-tensor path): the parameters after every step."""
    p = torch.nn.Parameter(torch.from_numpy(np.array(w)).to(dtype))
    opt = (torch.optim.AdamW if decoupled else torch.optim.Adam)([p], lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, foreach=False)
    out = []
    for g in grads:
        p.grad = torch.from_numpy(np.array(g)).to(dtype)
        opt.step()
        out.append(p.detach().numpy().copy())
    return np.stack(out)


def within_torch(got, t32, t64):
    """(error, bound) of the criterion in the module docstring."""
    err = float(np.abs(np.asarray(got, np.float64) - t64).max())
    yard = float(np.abs(np.asarray(t32, np.float64) - t64).max())
    return err, 2.0 * yard + float(np.spacing(F(np.abs(t64).max())))
