"""numpy restatement of the class-sharded CoCoOp step's own arithmetic (clip_calibration_amd/csrc/cocoop_train.hip, DESIGN.md "Class-sharded
CoCoOp fit"): the split of the classes, the padded layouts of the two gathers (NaN in the padding), a rank's partial -- per image the
ascending sum of its own classes' context rows from zero -- and the reduce: the ranks' partials added in rank order from zero, then one
multiplication by 1 / grad_scale.  Every function works in the dtype it is given: float64 for the comparison with tests/cocoopfit_ref.py,
float32 (every addition rounded) for the kernels' bits."""
import numpy as np

from shardfit_ref import split  # noqa: F401  (the balanced split of the classes: the first C mod G ranks one more)


def pad(C, G):
    """Classes per rank of a gathered block: ceil(C / G)."""
    return -(-C // G)


def gathered_text(text, B, C, G, extra=0, fill=np.nan):
    """[G, B ceil(C / G) E + extra] from the unsharded text [B C, E]: block r starts with rank r's [B, C_r, E]; the rest is ``fill``."""
    E = text.shape[1]
    t = text.reshape(B, C, E)
    out = np.full((G, B * pad(C, G) * E + extra), fill, text.dtype)
    for r, (lo, hi) in enumerate(split(C, G)):
        own = t[:, lo:hi].reshape(-1)
        out[r, :own.size] = own
    return out


def compact(gathered, B, C, E):
    """The unsharded [B C, E] back from the gathered blocks; the padding is never read."""
    G = gathered.shape[0]
    out = np.empty((B, C, E), gathered.dtype)
    for r, (lo, hi) in enumerate(split(C, G)):
        out[:, lo:hi] = gathered[r, :B * (hi - lo) * E].reshape(B, hi - lo, E)
    return out.reshape(B * C, E)


def own_rows(d_text, B, C, lo, hi):
    """Rows {b C + c : lo <= c < hi} of d_text [B C, E] as [B (hi - lo), E]."""
    return np.ascontiguousarray(d_text.reshape(B, C, -1)[:, lo:hi]).reshape(B * (hi - lo), -1)


def partial(d_embed, B, n_ctx):
    """A rank's partial [B, n_ctx, D] from ITS d_embed [B C_r, L, D]: the classes ascending from zero, unscaled."""
    dt = d_embed.dtype
    g = d_embed.reshape(B, -1, d_embed.shape[-2], d_embed.shape[-1])
    out = np.zeros((B, n_ctx, d_embed.shape[-1]), dt)
    for c in range(g.shape[1]):
        out = (out + g[:, c, 1:1 + n_ctx]).astype(dt)
    return out


def partials(d_embed, B, C, n_ctx, G, extra=0, fill=np.nan):
    """[G, B n_ctx D + extra] from the UNSHARDED d_embed [B C, L, D]: every rank's partial from its own prompts of it."""
    L, D = d_embed.shape[-2:]
    g = d_embed.reshape(B, C, L, D)
    out = np.full((G, B * n_ctx * D + extra), fill, d_embed.dtype)
    for r, (lo, hi) in enumerate(split(C, G)):
        out[r, :B * n_ctx * D] = partial(np.ascontiguousarray(g[:, lo:hi]).reshape(-1, L, D), B, n_ctx).reshape(-1)
    return out


def reduce_partials(blocks, n, inv_scale=1.0):
    """dcs, flat [n], from the gathered partials [G, >= n]: rank order from zero, then the one multiplication."""
    dt = blocks.dtype
    g = np.zeros(n, dt)
    for r in range(blocks.shape[0]):
        g = (g + blocks[r, :n]).astype(dt)
    return (g * dt.type(inv_scale)).astype(dt)


def sharded_dcs(d_embed, B, C, n_ctx, G, inv_scale=1.0):
    """dcs [B, n_ctx, D] of the sharded step from the unsharded d_embed [B C, L, D]."""
    D = d_embed.shape[-1]
    return reduce_partials(partials(d_embed, B, C, n_ctx, G), B * n_ctx * D, inv_scale).reshape(B, n_ctx, D)


def sharded_gradient(d_embed, x, hid, w2, B, C, n_ctx, G, inv_scale=1.0):
    """The five gradients of the sharded step (numpy in, a dict of numpy out): ``sharded_dcs``, then tests/cocoopfit_ref.py's reduce on a
    one-class stream whose context rows are that dcs -- 0 + dcs is dcs, so its meta-net backward runs on the sharded sum as it is."""
    import torch

    import cocoopfit_ref as cref
    dcs = sharded_dcs(d_embed, B, C, n_ctx, G, inv_scale)
    one = np.zeros((B, 1 + n_ctx, d_embed.shape[-1]), d_embed.dtype)
    one[:, 1:] = dcs
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    return {k: v.numpy() for k, v in cref.reduce(t(one), t(x), t(hid), t(w2), B, 1, n_ctx).items()}
