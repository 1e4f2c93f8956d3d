"""The plain restatement of clipmi_block_step_scaled (csrc/grad_scaler.hip): tests/scalerfit_ref.py's rule -- torch's GradScaler operators
and torch.optim.SGD, held to torch on the CPU by tests/test_scalerfit_cpu.py -- over a flat block of ``total`` elements.  A block is the
context of ONE prompt with one context row of ``total`` columns, so the row's "sum over the classes" is the gradient itself.  Inputs are
chosen exact in fp32 (scalerfit_ref.exact_inputs), so the fused multiply-adds of sgd_element_fma and any other order give the same bits."""
import numpy as np

import scalerfit_ref as ref

POISON = ref.POISON


class BlockRef(ref.ScalerRef):
    def __init__(self, params, init_scale, growth_factor=2.0, backoff_factor=0.5, growth_interval=2000, momentum=0.0, dampening=0.0,
                 weight_decay=0.0, nesterov=False):
        flat = np.asarray(params, np.float32).reshape(1, -1)
        super().__init__(flat, 1, 2, 1, False, init_scale, growth_factor, backoff_factor, growth_interval, momentum, dampening, weight_decay,
                         nesterov)

    def step(self, grad, lr) -> bool:
        """``grad`` fp32 [total]: scale * gradient.  Returns found."""
        d = np.zeros((2, self.ctx.size), np.float32)
        d[1] = np.asarray(grad, np.float32).reshape(-1)
        return super().step(d, lr)

    @property
    def params(self):
        return self.ctx.reshape(-1)

    @property
    def momentum_buffer(self):
        return None if self.buf is None else self.buf.reshape(-1)


def exact_block(total, steps, seed=0):
    """(params multiples of 2^-4 in [-2, 2], `steps` integer vectors with |v| <= 8): ``scaled(ints, scale)`` is scale times a gradient of
    multiples of 2^-8, and a few steps of SGD at a power-of-two rate and momentum stay exact in fp32."""
    rng = np.random.default_rng(seed)
    params = (rng.integers(-32, 33, size=total) / 16.0).astype(np.float32)
    return params, [rng.integers(-8, 9, size=total).astype(np.float32) for _ in range(steps)]


def scaled(ints, scale):
    return ref.scaled_embed(ints, scale)


def workspace_bytes(total):
    """The documented layout: the decision record (256) | one int32 flag per workgroup of 256 elements | the gradient, each part rounded up
    to 256 bytes."""
    up = lambda n: (n + 255) // 256 * 256
    return 256 + up(4 * ((total + 255) // 256)) + up(4 * total)
