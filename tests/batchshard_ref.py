"""numpy restatement of the batch-sharded block fits' reduction (clip_calibration_amd/csrc/shard_train.hip clipmi_block_rank_mean, DESIGN.md
"Batch-sharded image-tower fits"): the G ranks' blocks added one after the other in rank order in fp32 and multiplied by
``float32(1 / G)``, and the same in float64."""
import numpy as np


def rank_mean(gathered, total=None):
    """fp32 [total]: ``(((p_0 + p_1) + p_2) + ..) * float32(1 / G)`` over the rows of ``gathered`` fp32 [G, >= total], every sum and the
    product rounded to fp32; the columns behind ``total`` are not read."""
    g = np.asarray(gathered, np.float32)
    total = g.shape[1] if total is None else int(total)
    with np.errstate(invalid="ignore", over="ignore"):
        s = g[0, :total].copy()
        for r in range(1, g.shape[0]):
            s = (s + g[r, :total]).astype(np.float32)
        return (s * np.float32(1.0 / g.shape[0])).astype(np.float32)


def rank_mean64(gathered, total=None):
    """The float64 form: the same order, nothing rounded to fp32."""
    g = np.asarray(gathered, np.float64)
    total = g.shape[1] if total is None else int(total)
    s = g[0, :total].copy()
    for r in range(1, g.shape[0]):
        s = s + g[r, :total]
    return s / g.shape[0]


ORDER_TRIPLE = (1e8, -1e8, 1.0)     # in ranks 0 .. 2: ((1e8 - 1e8) + 1) / 3 in this order, ((1 - 1e8) + 1e8) / 3 = 0 in the reverse


def same_bits(a, b):
    """Equal bit for bit, but for NaNs, which need only sit in the same places (a NaN's payload is the hardware's to choose)."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(a[~na].view(np.int32), b[~nb].view(np.int32))
