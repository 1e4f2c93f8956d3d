"""The one-call training step of the two-tower fits (MaPLe: csrc/maple_train.hip; PromptSRC / IVLP: csrc/promptsrc_train.hip; the symbols
clipmi_maple_train_step, clipmi_promptsrc_train_step and their `_scaled` forms) as far as no GPU is needed: every refusal's code and message, each before anything
is launched, and the workspace size against the documented layout.  A model handle is host memory, and with no device a launch answers
CLIPMI_ERR_HIP, which is none of the codes a refusal returns."""
import ctypes as C
import math

import pytest

from clip_calibration_amd import _lib, synthetic as syn

lib = _lib.lib
REFUSALS = (_lib.OK, _lib.ERR_ARG, _lib.ERR_SHAPE, _lib.ERR_WORKSPACE, _lib.ERR_STATE)
P = C.c_void_p(1 << 20)                    # an aligned pointer nothing reads before a launch
N_PROMPTS, B, ROWS, DEPTH = 3, 2, 2, 2     # tiny: two layers in either tower
COMMON = ("m", "wt", "wv", "prompts", "dtype", "eot", "n_prompts", "seq_rows", "image", "image_dtype", "B", "labels")
SGD = ("momentum", "dampening", "weight_decay", "nesterov")
TAIL = ("grad_out", "workspace", "workspace_bytes", "text_stash", "text_stash_bytes", "vision_stash", "vision_stash_bytes", "stream")
SCALER = ("state", "growth_factor", "backoff_factor", "growth_interval")
SRC_W = ("w_text", "w_image", "w_logit")
ORDER = {
    "maple_train_step": COMMON + ("block", "buf", "n_ctx", "depth", "scale", "grad_scale", "lr", "first_step") + SGD + ("loss",) + TAIL,
    "maple_train_step_scaled": COMMON + ("block", "buf", "n_ctx", "depth", "scale") + SCALER + ("lr",) + SGD + ("loss",) + TAIL,
    "promptsrc_train_step": (COMMON + ("teacher", "block", "buf", "nt", "dt", "nv", "dv", "scale", "grad_scale") + SRC_W + ("lr", "first_step") + SGD
                             + ("losses",) + TAIL),
    "promptsrc_train_step_scaled": (COMMON + ("teacher", "block", "buf", "nt", "dt", "nv", "dv", "scale") + SCALER + SRC_W + ("lr",) + SGD + ("losses",)
                                    + TAIL),
}
SYMBOLS = tuple(ORDER)
MODEL = []


def a(n):
    return (n + 255) // 256 * 256


def handle(g):
    geo = _lib.Geometry(g.embed_dim, g.image_resolution, g.vision_patch_size, g.vision_width, g.vision_layers, g.context_length, g.vocab_size,
                        g.transformer_width, g.transformer_layers, g.transformer_heads)
    h = C.c_void_p()
    assert lib.clipmi_create(C.byref(geo), C.byref(h)) == _lib.OK
    return h


def model():
    """One `tiny` handle with both towers' weights bound to the dummy pointer: binding copies pointers and reads nothing behind them."""
    if not MODEL:
        g = syn.GEOMETRIES["tiny"]
        h = handle(g)
        blocks = (_lib.BlockWeights * 2)(*[_lib.BlockWeights(*[P.value] * len(_lib.BlockWeights._fields_)) for _ in range(2)])
        assert g.vision_layers == g.transformer_layers == 2
        assert lib.clipmi_set_vision_weights(h, C.byref(_lib.VisionWeights(*[P.value] * 8, blocks))) == _lib.OK
        assert lib.clipmi_set_text_weights(h, C.byref(_lib.TextWeights(*[P.value] * 5, blocks))) == _lib.OK
        MODEL.extend((h, g))
    return MODEL


def dgrad(cls, layers):
    blocks = (_lib.BlockDgrad * layers)(*[_lib.BlockDgrad(P.value, P.value, P.value, P.value) for _ in range(layers)])
    return cls(P.value, blocks), blocks


def need(symbol, h, **kw):
    scaled = symbol.endswith("_scaled")
    if symbol.startswith("maple"):
        by = lib.clipmi_maple_train_step_scaled_bytes if scaled else lib.clipmi_maple_train_step_bytes
        return by(h, kw["n_prompts"], kw["seq_rows"], kw["B"], kw["n_ctx"], kw["depth"])
    if scaled:
        return lib.clipmi_promptsrc_train_step_scaled_bytes(h, kw["n_prompts"], kw["seq_rows"], kw["B"], kw["nt"], kw["dt"], kw["nv"], kw["dv"])
    return lib.clipmi_promptsrc_train_step_bytes(h, kw["n_prompts"], kw["seq_rows"], kw["B"], kw["nt"], kw["dt"], kw["nv"])


def call(symbol, **over):
    """The symbol with every argument right but those in ``over``.  ``short``: the workspace is what the sizing function reports for the
    good arguments less that many bytes; without it the workspace is ample, so that a wrong shape meets its own refusal."""
    h, g = model()
    wt, keep_t = dgrad(_lib.TextDgrad, int(g.transformer_layers))
    wv, keep_v = dgrad(_lib.VisionDgrad, int(g.vision_layers))
    kw = dict(m=h, wt=C.byref(wt), wv=C.byref(wv), prompts=P, dtype=_lib.F16, eot=P, n_prompts=N_PROMPTS, seq_rows=0, image=P,
              image_dtype=_lib.F32, B=B, labels=P, teacher=P, block=P, buf=None, n_ctx=ROWS, depth=DEPTH, nt=ROWS, dt=DEPTH, nv=ROWS + 1, dv=DEPTH,
              scale=100.0, grad_scale=1024.0, w_text=25.0, w_image=10.0, w_logit=1.0, lr=P, first_step=1, momentum=0.0, dampening=0.0, weight_decay=0.0,
              nesterov=0, loss=P, losses=P, grad_out=None, workspace=P, text_stash=P, text_stash_bytes=1 << 40, vision_stash=P,
              vision_stash_bytes=1 << 40, stream=None, state=P, growth_factor=2.0, backoff_factor=0.5, growth_interval=2000)
    exact = need(symbol, h, **kw)
    assert exact > 0
    short = over.pop("short", None)
    kw["workspace_bytes"] = 1 << 40 if short is None else exact - short
    kw.update(over)
    return getattr(lib, "clipmi_" + symbol)(*[kw[k] for k in ORDER[symbol]])


def refused(symbol, code, fragment, **over):
    rc = call(symbol, **over)
    err = _lib.last_error()
    assert rc == code and fragment in err and err.startswith(symbol + ":"), (symbol, over, rc, err)


@pytest.mark.parametrize("symbol", SYMBOLS)
def test_a_good_call_gets_as_far_as_the_launch(symbol):
    assert call(symbol, short=0) not in REFUSALS and call(symbol) not in REFUSALS


@pytest.mark.parametrize("symbol", SYMBOLS)
def test_each_wrong_argument_is_refused_before_any_launch(symbol):
    src, scaled = symbol.startswith("promptsrc"), symbol.endswith("_scaled")
    refused(symbol, _lib.ERR_ARG, "null model", m=None)
    for null in ("block", "lr", "labels", "image") + (("teacher", "losses") if src else ()):
        refused(symbol, _lib.ERR_ARG, "null pointer", **{null: None})
    for null in ("prompts", "eot"):
        refused(symbol, _lib.ERR_ARG, "null pointer", **{null: None})
    refused(symbol, _lib.ERR_ARG, "null transposed weights", wt=None)
    refused(symbol, _lib.ERR_ARG, "null transposed weights", wv=None)
    refused(symbol, _lib.ERR_SHAPE, "n_prompts=1 (>= 2)", n_prompts=1)
    refused(symbol, _lib.ERR_SHAPE, "B=0 (>= 1)", B=0)
    if src:
        refused(symbol, _lib.ERR_SHAPE, "nt=0 dt=2", nt=0)
        refused(symbol, _lib.ERR_SHAPE, "nv=0 dv=2", nv=0)
        refused(symbol, _lib.ERR_SHAPE, "dt=0", dt=0)
        refused(symbol, _lib.ERR_SHAPE, "dv=0", dv=0)
        refused(symbol, _lib.ERR_SHAPE, "depth 3 for 2 text layers", dt=3)
        refused(symbol, _lib.ERR_SHAPE, "depth=3 for 2 layers", dv=3)
        refused(symbol, _lib.ERR_SHAPE, "does not fit the 77 token rows", nt=77, dt=1)
        refused(symbol, _lib.ERR_WORKSPACE, "needed", workspace=None)
        for w in SRC_W:
            refused(symbol, _lib.ERR_ARG, "(each finite, >= 0)", **{w: -1.0})
            refused(symbol, _lib.ERR_ARG, "(each finite, >= 0)", **{w: math.nan})
        refused(symbol, _lib.ERR_ARG, "image part must be 16-byte aligned", block=C.c_void_p((1 << 20) + 4))
    else:
        refused(symbol, _lib.ERR_SHAPE, "n_ctx=0 depth=2", n_ctx=0)
        refused(symbol, _lib.ERR_SHAPE, "n_ctx=2 depth=0", depth=0)
        refused(symbol, _lib.ERR_SHAPE, "depth 3 for 2 text layers", depth=3)
        refused(symbol, _lib.ERR_SHAPE, "does not fit the 77 token rows", n_ctx=77, depth=1)
        refused(symbol, _lib.ERR_ARG, "null workspace or stash", workspace=None)
    refused(symbol, _lib.ERR_WORKSPACE, "needed", short=1)
    refused(symbol, _lib.ERR_WORKSPACE, "workspace of 64 bytes", workspace_bytes=64)
    refused(symbol, _lib.ERR_ARG, "256-byte aligned", workspace=C.c_void_p((1 << 20) + 128))
    refused(symbol, _lib.ERR_ARG, "256-byte aligned", text_stash=C.c_void_p((1 << 20) + 128))
    refused(symbol, _lib.ERR_ARG, "256-byte aligned", vision_stash=C.c_void_p((1 << 20) + 128))
    refused(symbol, _lib.ERR_ARG, "null workspace or stash", text_stash=None)
    refused(symbol, _lib.ERR_ARG, "null workspace or stash", vision_stash=None)
    refused(symbol, _lib.ERR_WORKSPACE, "stash too small", text_stash_bytes=1024)
    refused(symbol, _lib.ERR_WORKSPACE, "stash too small", vision_stash_bytes=1024)
    refused(symbol, _lib.ERR_ARG, "image dtype 7", image_dtype=7)
    refused(symbol, _lib.ERR_ARG, "bad dtype 7", dtype=7)
    for bad in (math.inf, -math.inf, math.nan):
        refused(symbol, _lib.ERR_ARG, "both finite" if src else "(finite)", scale=bad)
    refused(symbol, _lib.ERR_ARG, "buffer", momentum=0.9)
    assert call(symbol, momentum=0.9, buf=P) not in REFUSALS
    refused(symbol, _lib.ERR_ARG, "nesterov needs a momentum", nesterov=1)
    refused(symbol, _lib.ERR_ARG, "momentum=1", momentum=1.0, buf=P)
    refused(symbol, _lib.ERR_ARG, "dampening=-0.5", dampening=-0.5)
    refused(symbol, _lib.ERR_ARG, "weight_decay=-1", weight_decay=-1.0)
    if scaled:
        refused(symbol, _lib.ERR_ARG, "scaler's state block", state=None)
        refused(symbol, _lib.ERR_ARG, "growth_factor=0", growth_factor=0.0)
        refused(symbol, _lib.ERR_ARG, "backoff_factor=inf", backoff_factor=math.inf)
        refused(symbol, _lib.ERR_ARG, "growth_interval=0 (>= 1)", growth_interval=0)
        refused(symbol, _lib.ERR_ARG, "4-byte aligned", lr=C.c_void_p((1 << 20) + 2))
    else:
        for bad in (0.0, -2.0, math.inf, math.nan):
            refused(symbol, _lib.ERR_ARG, "(finite, > 0)", grad_scale=bad)


@pytest.mark.parametrize("geom,n_prompts,seq_rows,batch,n_ctx,depth", [("tiny", 3, 0, 2, 2, 2), ("tiny", 2, 8, 1, 1, 1), ("tiny", 100, 8, 33, 4, 2),
                                                                       ("tiny3", 5, 0, 3, 3, 3), ("ViT-B/16", 3, 8, 4, 2, 9)])
def test_maple_workspace_is_the_documented_layout(geom, n_prompts, seq_rows, batch, n_ctx, depth):
    """clipmi_maple_train_step_bytes against the sum of DESIGN.md "MaPLe fit": the text tower's workspace | the image tower's | text and
    d_text [C, E] | feats and d_feats [B, E] | d_embed [C L, Dt] | d_deep [depth, n_ctx, Dt] | vis and d_vis [layers, n_ctx, Dv] | the
    head's | clipmi_maple_step's two [depth, n_ctx, Dt]; every piece rounded up to 256 bytes.  The scaled call adds the gradient block and
    clipmi_block_step_scaled's workspace."""
    g = syn.GEOMETRIES[geom]
    h = handle(g)
    try:
        tws, vws = C.c_size_t(), C.c_size_t()
        assert lib.clipmi_text_train_bytes(h, n_prompts, seq_rows, C.byref(tws), None) == _lib.OK
        assert lib.clipmi_vision_train_bytes(h, batch, n_ctx, C.byref(vws), None) == _lib.OK
        E, Dt, Dv, L = g.embed_dim, g.transformer_width, g.vision_width, seq_rows or g.context_length
        want = (tws.value + vws.value + 2 * a(n_prompts * E * 4) + 2 * a(batch * E * 4) + a(n_prompts * L * Dt * 4) + a(depth * n_ctx * Dt * 4)
                + 2 * a(g.vision_layers * n_ctx * Dv * 4) + lib.clipmi_maple_head_workspace_bytes(batch, E, n_prompts)
                + lib.clipmi_maple_step_workspace_bytes(n_ctx, depth, Dt))
        assert lib.clipmi_maple_step_workspace_bytes(n_ctx, depth, Dt) == 2 * a(depth * n_ctx * Dt * 4)
        assert lib.clipmi_maple_train_step_bytes(h, n_prompts, seq_rows, batch, n_ctx, depth) == want
        total = lib.clipmi_maple_block_floats(n_ctx, depth, Dt, Dv)
        assert lib.clipmi_maple_train_step_scaled_bytes(h, n_prompts, seq_rows, batch, n_ctx, depth) == (
            want + a(4 * total) + lib.clipmi_block_step_scaled_workspace_bytes(total))
        for bad in ((1, seq_rows, batch, n_ctx, depth), (n_prompts, seq_rows, 0, n_ctx, depth), (n_prompts, seq_rows, batch, 0, depth),
                    (n_prompts, seq_rows, batch, n_ctx, 0)):
            assert lib.clipmi_maple_train_step_bytes(h, *bad) == 0 and lib.clipmi_maple_train_step_scaled_bytes(h, *bad) == 0, bad
    finally:
        lib.clipmi_destroy(h)
