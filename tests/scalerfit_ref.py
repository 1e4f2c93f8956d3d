"""A plain restatement of the dynamic loss scale's rule (csrc/grad_scaler.hip, DESIGN.md "Dynamic loss scale"), for the tests:
``torch.cuda.amp.GradScaler`` around ``torch.optim.SGD`` on one parameter, the context.  tests/test_scalerfit_cpu.py holds it to torch
itself on the CPU; tests/test_gpu_scalerfit.py holds the kernels to it.

The optimiser's arithmetic is done in float64 and every value that is stored must be an fp32 number as it stands (``_store`` asserts it):
on such inputs nothing is rounded anywhere, so torch's CPU kernels (a product and a sum) and the GPU kernels (one fused multiply-add)
agree with it bit for bit, and the reference does not have to know which of the two it is compared with.  ``exact_inputs`` makes inputs
of that kind.
"""
import numpy as np


def _store(x: np.ndarray, what: str) -> np.ndarray:
    y = x.astype(np.float32)
    assert np.array_equal(y.astype(np.float64), x), f"scalerfit_ref: {what} is not exact in fp32 -- choose inputs with fewer bits"
    return y


def context_sum(d_embed: np.ndarray, C: int, L: int, n_ctx: int, per_class: bool) -> np.ndarray:
    """The scaled gradient of the context from d_embed fp32 [C * L, D]: rows 1 .. n_ctx of every prompt, the classes added one after the
    other in fp32 in ascending order (generic context, [n_ctx, D]) or kept apart ([C, n_ctx, D])."""
    rows = np.asarray(d_embed, np.float32).reshape(C, L, -1)[:, 1:1 + n_ctx, :]
    if per_class:
        return rows.copy()
    g = np.zeros(rows.shape[1:], np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        for c in range(C):
            g = (g + rows[c]).astype(np.float32)
    return g


class ScalerRef:
    """The state of one fit: ctx, buf (None until the first applied step), the scale, the tracker and the counters."""

    def __init__(self, ctx, C, L, n_ctx, per_class, init_scale=2.0 ** 16, growth_factor=2.0, backoff_factor=0.5, growth_interval=2000,
                 momentum=0.0, dampening=0.0, weight_decay=0.0, nesterov=False):
        self.ctx = np.array(ctx, np.float32)
        self.buf = None
        self.C, self.L, self.n_ctx, self.per_class = C, L, n_ctx, per_class
        self.scale = np.float32(init_scale)
        self.growth, self.backoff, self.interval = np.float32(growth_factor), np.float32(backoff_factor), int(growth_interval)
        self.momentum, self.dampening, self.weight_decay, self.nesterov = momentum, dampening, weight_decay, nesterov
        self.growth_tracker = self.skipped_steps = self.applied_steps = self.found_inf = 0
        self.grad = None

    def state(self) -> dict:
        return {"scale": float(self.scale), "growth_tracker": self.growth_tracker, "skipped_steps": self.skipped_steps,
                "applied_steps": self.applied_steps, "found_inf": self.found_inf}

    def step(self, d_embed, lr) -> bool:
        """One call: unscale, look at every element, step only when all are finite, update the scale.  Returns found."""
        with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
            inv = np.float32(1.0) / self.scale
            self.grad = (context_sum(d_embed, self.C, self.L, self.n_ctx, self.per_class) * inv).astype(np.float32)
        found = not bool(np.isfinite(self.grad).all())
        self.found_inf = int(found)
        if found:
            self.scale = np.float32(self.scale * self.backoff)
            self.growth_tracker = 0
            self.skipped_steps += 1
            return True
        self._sgd(self.grad.astype(np.float64), float(np.float32(lr)))
        self.applied_steps += 1
        self.growth_tracker += 1
        if self.growth_tracker == self.interval:
            with np.errstate(over="ignore"):
                grown = np.float32(self.scale * self.growth)
            if np.isfinite(grown):
                self.scale = grown
            self.growth_tracker = 0
        return False

    def _sgd(self, g, lr):
        """torch.optim.SGD; the buffer starts as the first applied gradient (torch: ``buf = clone(grad)`` when the state has none)."""
        w = self.ctx.astype(np.float64)
        if self.weight_decay != 0.0:
            g = g + float(np.float32(self.weight_decay)) * w
        if self.momentum != 0.0:
            if self.buf is None:
                b = g
            else:
                b = float(np.float32(self.momentum)) * self.buf.astype(np.float64) + float(np.float32(1.0 - self.dampening)) * g
            self.buf = _store(b, "buf")
            g = g + float(np.float32(self.momentum)) * b if self.nesterov else b
        self.ctx = _store(w - lr * g, "ctx")


def exact_inputs(C, L, D, n_ctx, per_class, steps, seed=0):
    """(ctx multiples of 2^-4 in [-2, 2], a list of `steps` integer matrices [C * L, D] with |v| <= 8): times scale 2^-8 they are the
    d_embed of a gradient of multiples of 2^-8, and a few steps of SGD at a power-of-two rate and momentum stay exact in fp32."""
    rng = np.random.default_rng(seed)
    shape = (C, n_ctx, D) if per_class else (n_ctx, D)
    ctx = (rng.integers(-32, 33, size=shape) / 16.0).astype(np.float32)
    ints = [rng.integers(-8, 9, size=(C * L, D)).astype(np.float32) for _ in range(steps)]
    return ctx, ints


def scaled_embed(ints: np.ndarray, scale: float) -> np.ndarray:
    """ints * scale * 2^-8 in fp32: what a backward that carries `scale` times a gradient of ints * 2^-8 leaves.  Exact."""
    return _store(ints.astype(np.float64) * float(scale) * 2.0 ** -8, "d_embed")


# found-inf patterns of the sequence tests, growth_interval = 2.  A: a skip on the very first step, two skips in a row, a growth two clean
# steps later, a skip, growth right after it.  B: from 2^127 -- the growth of step 1 would pass 2^127 and is not taken (the tracker still
# starts again); a skip brings 2^126, the next growth 2^127 again.
PATTERN_A = (1, 1, 0, 0, 1, 0, 0, 0)
PATTERN_B = (0, 0, 1, 0, 0, 0, 0)
SEQUENCES = {"A": dict(init_scale=2.0 ** 10, pattern=PATTERN_A), "B": dict(init_scale=2.0 ** 127, pattern=PATTERN_B)}
POISON = (np.inf, -np.inf, np.nan)
