"""The plain restatement of clipmi_proda_ctx_step_scaled (csrc/proda_train.hip, DESIGN.md "Dynamic loss scale for ProDA"): the gradient
of ProDA's contexts by tests/prodafit_ref.py's gather (a selected context's class rows in ascending class order, then every context's
no-class row) in fp32, and on it tests/scalerfit_ref.py's rule -- torch._amp_foreach_non_finite_check_and_unscale_, torch.optim.SGD with
the momentum buffer born on the first applied step, torch._amp_update_scale_.  To that rule the P contexts are P prompts of 1 + n_ctx rows
with one context each (``per_class``), whose rows 1 .. n_ctx hold the gathered sums.  Inputs are chosen exact in fp32
(``exact_inputs``), so the fused multiply-adds of the kernels and any other order give the same bits.  tests/test_prodascaler_cpu.py holds
this file to torch on the CPU; tests/test_gpu_prodascaler.py holds the kernels to it."""
import numpy as np
import torch

import prodafit_ref as dref
import scalerfit_ref as ref

POISON = ref.POISON


def gather(d_embed, sel, pos, name_lens, C, P, n_ctx) -> np.ndarray:
    """scale * d ctx, fp32 [P, n_ctx, D], from d_embed fp32 [(C Pb + P) L, D]; ``sel`` as the kernel is given it (already ordered)."""
    d = torch.as_tensor(np.asarray(d_embed, np.float32))
    N = C * len(sel) + P
    return dref.ctx_reduce(d.reshape(N, d.shape[0] // N, -1), [int(p) for p in sel], pos, name_lens, C, P, n_ctx).numpy()


class ProdaScalerRef(ref.ScalerRef):
    """The state of one ProDA fit under the dynamic scale: ``ctx`` [P, n_ctx, D], ``buf``, the scale, the tracker and the counters."""

    def __init__(self, ctx, C, pos, name_lens, init_scale=2.0 ** 16, growth_factor=2.0, backoff_factor=0.5, growth_interval=2000, momentum=0.0,
                 dampening=0.0, weight_decay=0.0, nesterov=False):
        P, n_ctx, _ = np.asarray(ctx).shape
        super().__init__(ctx, P, 1 + n_ctx, n_ctx, True, init_scale, growth_factor, backoff_factor, growth_interval, momentum, dampening,
                         weight_decay, nesterov)
        self.n_cls, self.pos, self.name_lens = C, np.asarray(pos), np.asarray(name_lens)

    def step(self, d_embed, lr, sel) -> bool:
        """One call on d_embed [(C Pb + P) L, D] with the ordered selection ``sel`` [Pb].  Returns found."""
        P, n_ctx, D = self.ctx.shape
        with np.errstate(over="ignore", invalid="ignore"):
            sums = gather(d_embed, sel, self.pos, self.name_lens, self.n_cls, P, n_ctx)
        rows = np.zeros((P, 1 + n_ctx, D), np.float32)
        rows[:, 1:] = sums
        return super().step(rows.reshape(P * (1 + n_ctx), D), lr)


def exact_inputs(C, Pb, P, L, D, n_ctx, steps, seed=0):
    """(ctx [P, n_ctx, D] of multiples of 2^-4 in [-2, 2], `steps` integer matrices [(C Pb + P) L, D] with |v| <= 8): ``scaled(ints,
    scale)`` is the d_embed of a backward that carries `scale` times a gradient of multiples of 2^-8, and a few steps of SGD at a
    power-of-two rate, momentum and weight decay stay exact in fp32."""
    rng = np.random.default_rng(seed)
    ctx = (rng.integers(-32, 33, size=(P, n_ctx, D)) / 16.0).astype(np.float32)
    return ctx, [rng.integers(-8, 9, size=((C * Pb + P) * L, D)).astype(np.float32) for _ in range(steps)]


def scaled(ints, scale):
    return ref.scaled_embed(ints, scale)


def read_rows(sel, pos, name_lens, C, P, L, n_ctx):
    """The (prompt, row) pairs of d_embed [(C Pb + P), L, D] that the gather reads, as a boolean mask [C Pb + P, L]."""
    Pb, h = len(sel), n_ctx // 2
    mask = np.zeros((C * Pb + P, L), bool)
    for q, p in enumerate(sel):
        for c in range(C):
            for j in range(n_ctx):
                mask[c * Pb + q, dref.ctx_row(int(pos[p]), j, int(name_lens[c]), h)] = True
    mask[C * Pb:, 1:1 + n_ctx] = True
    return mask


def workspace_bytes(P, D, n_ctx):
    """The documented layout: the decision record (256) | one int32 flag per workgroup of 256 elements | the gradient, each part rounded up
    to 256 bytes."""
    total = P * n_ctx * D
    up = lambda n: (n + 255) // 256 * 256
    return 256 + up(4 * ((total + 255) // 256)) + up(4 * total)
