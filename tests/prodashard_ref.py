"""numpy restatement of the class-sharded ProDA step's own arithmetic (clip_calibration_amd/csrc/proda_train.hip, DESIGN.md "Class-sharded
ProDA fit"): the split of the classes and the dealing of the no-class prompts, the padded layouts of the two gathers, a rank's send
block -- per selected slot the ascending sum of its own classes' rows from zero, then its own no-class rows -- and the reduced gradient:
the ranks' class sums added in rank order from zero, the owner's no-class row last, then 1 / grad_scale.  Every function works in the dtype
it is given: float64 for the comparison with tests/prodafit_ref.py, float32 (every addition rounded) for the kernels' bits."""
import numpy as np

import prodafit_ref as dref
from shardfit_ref import split  # noqa: F401  (the same balanced split for the classes and for the no-class prompts)


def owner(p, n, G):
    """(rank, its first item) of item p under the balanced split of n items."""
    for r, (lo, hi) in enumerate(split(n, G)):
        if lo <= p < hi:
            return r, lo
    raise ValueError(p)


def text_rows(C, Pb, P, G):
    """Rows of one rank's block of the gathered text features."""
    return -(-C // G) * Pb + -(-P // G)


def gathered_text(text, C, Pb, P, G, fill=np.nan):
    """[G, text_rows, E] from the unsharded text [C Pb + P, E]: block r = rank r's class rows, its no-class rows, padding."""
    out = np.full((G, text_rows(C, Pb, P, G), text.shape[1]), fill, text.dtype)
    for r, ((lo, hi), (plo, phi)) in enumerate(zip(split(C, G), split(P, G))):
        own = np.concatenate([text[lo * Pb:hi * Pb], text[C * Pb + plo:C * Pb + phi]])
        out[r, :len(own)] = own
    return out


def rows_of(p, c, pos, name_lens, n_ctx):
    return [dref.ctx_row(int(pos[p]), j, int(name_lens[c]), n_ctx // 2) for j in range(n_ctx)]


def send_block(d_embed, sel, pos, name_lens, n_own, n_ctx, pad_to=None, fill=np.nan):
    """A rank's send block [Pb + pad_to, n_ctx, D] from ITS d_embed [C_r Pb + n_own, L, D] (name_lens: its own classes')."""
    Pb, C = len(sel), len(name_lens)
    out = np.full((Pb + (n_own if pad_to is None else pad_to), n_ctx, d_embed.shape[-1]), fill, d_embed.dtype)
    for q, p in enumerate(sel):
        s = np.zeros((n_ctx, d_embed.shape[-1]), d_embed.dtype)
        for c in range(C):
            s = (s + d_embed[c * Pb + q, rows_of(p, c, pos, name_lens, n_ctx)]).astype(d_embed.dtype)
        out[q] = s
    out[Pb:Pb + n_own] = d_embed[C * Pb:, 1:1 + n_ctx]
    return out


def send_blocks(d_embed, sel, pos, name_lens, C, P, n_ctx, G):
    """[G, Pb + ceil(P / G), n_ctx, D] from the UNSHARDED d_embed [C Pb + P, L, D]: every rank's block from its own rows of it."""
    Pb, out = len(sel), []
    for (lo, hi), (plo, phi) in zip(split(C, G), split(P, G)):
        own = np.concatenate([d_embed[lo * Pb:hi * Pb], d_embed[C * Pb + plo:C * Pb + phi]])
        out.append(send_block(own, sel, pos, name_lens[lo:hi], phi - plo, n_ctx, -(-P // G)))
    return np.stack(out)


def reduce_blocks(blocks, sel, P, inv_scale=1.0):
    """[P, n_ctx, D] from the gathered blocks [G, Pb + ceil(P / G), n_ctx, D]: the padding is never read."""
    G, Pb, dt = blocks.shape[0], len(sel), blocks.dtype
    out = np.zeros((P,) + blocks.shape[2:], dt)
    slots = [int(p) for p in sel]
    for p in range(P):
        g = np.zeros(blocks.shape[2:], dt)
        if p in slots:
            for r in range(G):
                g = (g + blocks[r, slots.index(p)]).astype(dt)
        r, lo = owner(p, P, G)
        g = (g + blocks[r, Pb + p - lo]).astype(dt)
        out[p] = (g * dt.type(inv_scale)).astype(dt)
    return out


def sharded_gradient(d_embed, sel, pos, name_lens, C, P, n_ctx, G, inv_scale=1.0):
    return reduce_blocks(send_blocks(d_embed, sel, pos, name_lens, C, P, n_ctx, G), sel, P, inv_scale)
