"""numpy restatement of the class-sharded CoOp fit's own arithmetic (clip_calibration_amd/csrc/shard_train.hip, DESIGN.md "Class-sharded
CoOp fit"): the balanced split, the padded gather layout with its compaction map, and the reduced context gradient -- per rank the
ascending fp32 sum of its own classes' rows, then the ranks' partials added in rank order in fp32, then 1 / grad_scale."""
import numpy as np

U32 = 2.0 ** -24      # fp32's unit roundoff


def split(C, G):
    """[(lo, hi)] per rank: contiguous, the first C mod G ranks one class more."""
    if C < G:
        raise ValueError(f"C={C} < G={G}")
    base, rem = divmod(C, G)
    out, lo = [], 0
    for r in range(G):
        hi = lo + base + (1 if r < rem else 0)
        out.append((lo, hi))
        lo = hi
    return out


def padded(blocks, fill=np.nan):
    """The gathered block [G, P, ...] of the ranks' own rows, P = the longest shard (= ceil(C / G)), the padding rows set to ``fill``."""
    P = max(b.shape[0] for b in blocks)
    out = np.full((len(blocks), P) + blocks[0].shape[1:], fill, dtype=blocks[0].dtype)
    for r, b in enumerate(blocks):
        out[r, :b.shape[0]] = b
    return out


def compact_map(C, G):
    """[(rank, row within the rank's block)] for class 0 .. C-1."""
    return [(r, c - lo) for r, (lo, hi) in enumerate(split(C, G)) for c in range(lo, hi)]


def compact(gathered, C):
    return np.stack([gathered[r, i] for r, i in compact_map(C, gathered.shape[0])])


def chain_sum(rows):
    """fp32 sum of rows [n, ...] from 0 in ascending order, every addition rounded: ctx_grad_element's chain."""
    s = np.zeros(rows.shape[1:], np.float32)
    for row in rows.astype(np.float32):
        s = (s + row).astype(np.float32)
    return s


def rank_sum(partials):
    """fp32 sum of partials [G, ...] in rank order, starting from rank 0's."""
    s = partials[0].astype(np.float32)
    for p in partials[1:]:
        s = (s + p.astype(np.float32)).astype(np.float32)
    return s


def partials(rows, G):
    """[G, ...] from the classes' context rows [C, ...] fp32: every rank's ascending chain over its own classes."""
    return np.stack([chain_sum(rows[lo:hi]) for lo, hi in split(rows.shape[0], G)])


def reduced_gradient(rows, G, grad_scale=1.0):
    return (rank_sum(partials(rows, G)) * np.float32(1.0 / grad_scale)).astype(np.float32)


def sum_bound(rows, G):
    """Element-wise bound on |reduced_gradient(rows, G) - the exact sum|: a sum whose every term passes through at most k rounded
    additions is off by at most gamma_k sum |x|, gamma_k = k u / (1 - k u) (Higham, Accuracy and Stability, section 4.2).  A term passes
    through at most ceil(C / G) - 1 additions that round inside its rank's chain (the first, to zero, is exact) and G - 1 across the ranks."""
    C = rows.shape[0]
    k = (-(-C // G) - 1) + (G - 1)
    gamma = k * U32 / (1.0 - k * U32)
    return gamma * np.abs(rows.astype(np.float64)).sum(0)
