"""Float64 numpy restatement of TempScaling's one-parameter fit (reference trainers/calibration/tempscaling.py:146-169) from cached
cosine logits: the per-batch loss and gradient, torch.optim.SGD's rule on the scalar, the batching and the learning-rate schedule.  It
does not import the package: tests/test_tempscale_cpu.py holds it to torch's own F.cross_entropy + backward + SGD in float64, and
tests/test_gpu_tempscale.py holds the device to it."""
import math

import numpy as np

U = 2.0 ** -24   # unit round-off of fp32


def make_case(n, C, seed, label_is_argmax=0.7):
    """Seeded cosines uniform in [-1, 1] (fp32) and labels; in a share ``label_is_argmax`` of the rows the label's cosine is raised to
    half way between the row's maximum and 1, so that the label is the row's argmax there."""
    rng = np.random.default_rng(seed)
    c = rng.uniform(-1.0, 1.0, (n, C)).astype(np.float32)
    y = rng.integers(0, C, n).astype(np.int64)
    sharp = np.flatnonzero(rng.uniform(size=n) < label_is_argmax)
    c[sharp, y[sharp]] = (0.5 * (c[sharp].max(axis=1).astype(np.float64) + 1.0)).astype(np.float32)
    return c, y


def row_terms(c, y, theta):
    """Per row: (loss_i, d loss_i / d theta) of cross_entropy(exp(theta) * c_i, y_i), float64."""
    c = np.asarray(c, np.float64)
    s = math.exp(float(theta))
    z = s * c
    m = z.max(axis=1, keepdims=True)
    e = np.exp(z - m)
    S = e.sum(axis=1)
    cy = c[np.arange(c.shape[0]), y]
    loss = np.log(S) + m[:, 0] - s * cy
    grad = s * ((e * c).sum(axis=1) / S - cy)
    return loss, grad


def batch_loss_grad(c, y, theta):
    """F.cross_entropy's default reduction: the means over the batch's rows."""
    loss, grad = row_terms(c, y, theta)
    return float(loss.mean()), float(grad.mean())


def sgd_step(theta, buf, step, g, lr, momentum=0.0, dampening=0.0, weight_decay=0.0, nesterov=False):
    """torch.optim.SGD.step on one scalar; returns (theta, buf)."""
    if weight_decay != 0:
        g = g + weight_decay * theta
    if momentum != 0:
        buf = g if step == 0 else momentum * buf + (1 - dampening) * g
        g = g + momentum * buf if nesterov else buf
    return theta - lr * g, buf


def batches(n, batch, epochs, order=None, drop_last=False):
    """Yields (epoch, sample indices): order[e, k * batch : (k + 1) * batch], order None = 0 .. n-1 in every epoch."""
    per_epoch = n // batch if drop_last else -(-n // batch)
    for e in range(epochs):
        idx = np.arange(n) if order is None else np.asarray(order)[e]
        for k in range(per_epoch):
            yield e, idx[k * batch:(k + 1) * batch]


def cosine_warmup_schedule(lr, epochs, warmup_epochs=1, warmup_lr=1e-5):
    """Per-epoch rates: warmup_lr during the warm-up; epoch e >= warmup_epochs at the cosine value of index e - warmup_epochs + 1 (the
    cosine scheduler is first stepped at the end of the last warm-up epoch), index e without a warm-up."""
    out = []
    for e in range(epochs):
        if e < warmup_epochs:
            out.append(warmup_lr)
        else:
            t = e - warmup_epochs + 1 if warmup_epochs > 0 else e
            out.append(lr * (1.0 + math.cos(math.pi * t / epochs)) / 2.0)
    return out


def fit(c, y, init, lr_per_epoch, batch, momentum=0.0, dampening=0.0, weight_decay=0.0, nesterov=False, order=None, drop_last=False):
    """The whole run in float64: (final theta, [every step's batch loss])."""
    c = np.asarray(c, np.float64)
    theta, buf, step, losses = float(init), 0.0, 0, []
    for e, idx in batches(c.shape[0], batch, len(lr_per_epoch), order, drop_last):
        loss, g = batch_loss_grad(c[idx], y[idx], theta)
        theta, buf = sgd_step(theta, buf, step, g, lr_per_epoch[e], momentum, dampening, weight_decay, nesterov)
        losses.append(loss)
        step += 1
    return theta, losses


def batch_error_bound(c, y, theta):
    """First-order bound on |device - float64| for one batch's (mean loss, mean gradient), from the fp32 arithmetic of
    csrc/tempscale.hip, with u = 2^-24 and the exact row quantities s = exp(theta), z_j = s c_j, m = max z, d_j = z_j - m, p = softmax(z),
    cbar = sum p_j c_j:

    * s = expf(theta) is within an ulp (relative 2u) and z_j = fl(s c_j) adds u: |dz_j| <= 3u |z_j|, the same for m;
    * d_j = fl(z_j - m) adds u |d_j|; __expf forms d_j * log2(e) in fp32 (the constant and the product: 2u |d_j| in the exponent) and
      v_exp_f32 is within an ulp (2u): the term exp(d_j) carries a relative error eps_j = u (3 |z_j| + 3 |m| + 3 |d_j| + 2);
      terms that underflow weigh less than 2^-126 of a sum that is at least 1 and do not count;
    * a lane-strided fp32 sum of ceil(C / 64) terms and six tree levels: relative sigma = (ceil(C / 64) + 5) u on sums of one sign;
    * S = sum exp(d_j) is off by E_S = sum p_j eps_j + sigma relatively; logf within an ulp: 2u |log S|; the label's
      d_y carries 3u (|z_y| + |m|) + u |d_y|; the last subtraction u |loss_i|:
        |d loss_i| <= E_S + 2u |log S| + 3u (|z_y| + |m|) + u |d_y| + u |loss_i|
    * T = sum exp(d_j) c_j has one more rounding per term; in T / S the common part of the errors cancels, what is left is
      sum p_j (eps_j + u) |c_j - cbar| + sigma (sum p_j |c_j| + |cbar|) + u |cbar| (the division); then the subtraction of c_y and the
      product with s (2u + u) act on the result:
        |d grad_i| <= s [sum p_j (eps_j + u) |c_j - cbar| + sigma (sum p_j |c_j| + |cbar|) + u |cbar|] + 4u |grad_i|
    * the batch means are formed in float64 and rounded once: u |mean|.
    Returns (bound on the loss, bound on the gradient), absolute."""
    c = np.asarray(c, np.float64)
    n, C = c.shape
    s = math.exp(float(theta))
    z = s * c
    m = z.max(axis=1, keepdims=True)
    d = z - m
    e = np.exp(d)
    S = e.sum(axis=1, keepdims=True)
    p = e / S
    cbar = (p * c).sum(axis=1, keepdims=True)
    rows = np.arange(n)
    loss, grad = row_terms(c, y, theta)
    eps = U * (3 * np.abs(z) + 3 * np.abs(m) + 3 * np.abs(d) + 2)
    sigma = (math.ceil(C / 64) + 5) * U
    E_S = (p * eps).sum(axis=1) + sigma
    zy, dy = z[rows, y], d[rows, y]
    b_loss = E_S + 2 * U * np.abs(np.log(S[:, 0])) + 3 * U * (np.abs(zy) + np.abs(m[:, 0])) + U * np.abs(dy) + U * np.abs(loss)
    b_grad = s * ((p * (eps + U) * np.abs(c - cbar)).sum(axis=1) + sigma * ((p * np.abs(c)).sum(axis=1) + np.abs(cbar[:, 0]))
                  + U * np.abs(cbar[:, 0])) + 4 * U * np.abs(grad)
    return float(b_loss.mean() + U * abs(loss.mean())), float(b_grad.mean() + U * abs(grad.mean()))


def torch_fit(c, y, init, lr_per_epoch, batch, momentum=0.0, dampening=0.0, weight_decay=0.0, nesterov=False, order=None, drop_last=False,
              dtype="float64"):
    """The step the reference performs (tempscaling.py:156-160), by torch itself on the CPU in ``dtype``: F.cross_entropy of
    exp(logit_scale) * cosine, backward, torch.optim.SGD.step, the group's lr set per epoch.  The yardstick of this module (float64) and of
    the device's tolerance (float32).  Returns (final theta, [every step's batch loss])."""
    import torch
    import torch.nn.functional as F
    dt = getattr(torch, dtype)
    ct, yt = torch.from_numpy(np.array(c)).to(dt), torch.from_numpy(np.array(y))
    scale = torch.nn.Parameter(torch.tensor(float(init), dtype=dt))
    opt = torch.optim.SGD([scale], lr=1.0, momentum=momentum, dampening=dampening, weight_decay=weight_decay, nesterov=nesterov)
    losses = []
    for e, idx in batches(ct.shape[0], batch, len(lr_per_epoch), order, drop_last):
        opt.param_groups[0]["lr"] = lr_per_epoch[e]
        idx = torch.from_numpy(np.ascontiguousarray(idx))
        loss = F.cross_entropy(scale.exp() * ct[idx], yt[idx])
        opt.zero_grad()
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    return float(scale.detach()), losses
