"""The image tower's training path for patch sizes the im2col-free loader does not serve (ViT-L/14: patches of 14 pixels), as far as no GPU
is needed: the size query on patch-14 geometries against the documented layout, the unchanged sizes of the patch-8 and patch-16
geometries, and the refusal of a resolution that is no multiple of the patch size.  A model handle is host memory: clipmi_create and
clipmi_vision_train_bytes launch nothing."""
import ctypes as C

import pytest

import vptfit_ref as ref
from clip_calibration_amd import _lib, synthetic as syn

TOY14 = syn.ClipGeometry(128, 42, 2, 128, 14, 77, 256, 128, 2, 2)          # 3 x 3 patches + class = 10 tokens
TOY14_257 = syn.ClipGeometry(128, 224, 2, 128, 14, 77, 256, 128, 2, 2)     # 16 x 16 + 1 = 257: ViT-L/14's resolution and patch


def a(n):
    return (n + 255) // 256 * 256


def handle(g):
    geo = _lib.Geometry(g.embed_dim, g.image_resolution, g.vision_patch_size, g.vision_width, g.vision_layers, g.context_length, g.vocab_size,
                        g.transformer_width, g.transformer_layers, g.transformer_heads)
    h = C.c_void_p()
    rc = _lib.lib.clipmi_create(C.byref(geo), C.byref(h))
    return rc, h


def train_bytes(h, B, n_ctx):
    ws, st = C.c_size_t(7), C.c_size_t(7)
    rc = _lib.lib.clipmi_vision_train_bytes(h, B, n_ctx, C.byref(ws), C.byref(st))
    return rc, ws.value, st.value


def layout(g, B, n_ctx, slot):
    """The documented workspace and stash (DESIGN.md "VPT fit", "Long attention backward"; tests/test_gpu_vision_train_long.py): the tower's
    pieces, the gradient stream, the front end's slot, the fp16 prompts, slot 0's sum, the long kernel's statistics beyond 224 rows."""
    L, D, E, H, layers = g.vision_tokens + n_ctx, g.vision_width, g.embed_dim, g.vision_width // 64, g.vision_layers
    M = B * L
    abl = 12 * B * H * L if L > 224 else 0
    ws = (2 * a(M * D * 2) + a(M * D * 8) + a(M * D * 6) + a(M * D * 4) + a(B * D * 2) + a(B * E * 2) + a(B * D * 4) + a(M * D * 4)
          + a(slot) + a(layers * n_ctx * D * 2) + a(n_ctx * D * 4) + a(abl))
    st = (2 * layers + 1) * a(M * D * 4) + layers * (a(M * D * 6) + a(M * D * 8)) + a(B * 8) + a(layers * n_ctx * D * 4)
    return ws, st


def col_slot(g, B):
    """The im2col matrix: [B G^2, kpad] fp16 with kpad = 3 P^2 rounded up to 64 columns."""
    P = g.vision_patch_size
    kpad = (3 * P * P + 63) // 64 * 64
    return B * g.grid * g.grid * kpad * 2


def image_slot(g, B):
    """The fp16 copy of an fp32 image batch, the loader's slot."""
    return B * 3 * g.image_resolution * g.image_resolution * 2


@pytest.mark.parametrize("g,B,n_ctx,long", [(TOY14, 3, 4, 0), (TOY14_257, 2, 8, 1)])
def test_patch14_sizes_are_the_documented_layout_with_the_im2col_slot(g, B, n_ctx, long):
    assert col_slot(TOY14, 1) == 9 * 640 * 2 and 3 * 14 * 14 == 588
    rc, h = handle(g)
    assert rc == _lib.OK
    try:
        with _lib.option("vision_train_long", long):
            got = train_bytes(h, B, n_ctx)
        want = layout(g, B, n_ctx, col_slot(g, B))
        assert got == (_lib.OK,) + want, (got, want)
        assert a(col_slot(g, B)) != a(image_slot(g, B)), "the case cannot tell the two slots apart"
        assert layout(g, B, n_ctx, image_slot(g, B))[0] != got[1]
    finally:
        _lib.lib.clipmi_destroy(h)


def test_vit_l14_slot_bytes_per_image():
    """The figures the documents quote: 327 680 bytes of im2col matrix per image at ViT-L/14 against 301 056 of the fp16 copy."""
    g = syn.GEOMETRIES["ViT-L/14"]
    assert col_slot(g, 1) == 327680 and image_slot(g, 1) == 301056
    rc, h = handle(g)
    assert rc == _lib.OK
    try:
        with _lib.option("vision_train_long", 1):
            for B, n_ctx in ((1, 2), (4, 2), (4, 4)):
                assert train_bytes(h, B, n_ctx) == (_lib.OK,) + layout(g, B, n_ctx, col_slot(g, B))
        assert train_bytes(h, 1, 2) == (_lib.ERR_SHAPE, 0, 0) and "at most 224" in _lib.last_error()     # by length, not by patch size
    finally:
        _lib.lib.clipmi_destroy(h)


@pytest.mark.parametrize("g,B,n_ctx", [(ref.CUSTOM, 2, 8), (ref.CUSTOM, 1, 1), (syn.GEOMETRIES["tiny"], 3, 8), (syn.GEOMETRIES["ViT-B/16"], 4, 8),
                                       (syn.GEOMETRIES["ViT-B/32"], 2, 4)])
def test_loader_geometries_keep_their_sizes(g, B, n_ctx):
    """Patches of 8, 16 and 32 pixels: byte for byte the layout with the fp16 image copy in the slot, option on or off."""
    rc, h = handle(g)
    assert rc == _lib.OK
    try:
        want = layout(g, B, n_ctx, image_slot(g, B))
        for long in (0, 1):
            with _lib.option("vision_train_long", long):
                assert train_bytes(h, B, n_ctx) == (_lib.OK,) + want
    finally:
        _lib.lib.clipmi_destroy(h)


def test_a_resolution_that_is_no_multiple_of_the_patch_is_refused_before_any_launch():
    """No handle of such a geometry exists (clipmi_create refuses it, so every entry point that takes a handle is covered), and the
    route's first stage refuses it on its own: both before anything is launched -- this test runs without a GPU."""
    for R, P in ((43, 14), (224, 15), (13, 14)):
        rc, h = handle(syn.ClipGeometry(128, R, 2, 128, P, 77, 256, 128, 2, 2))
        assert rc == _lib.ERR_SHAPE and not h.value, (R, P)
        assert _lib.lib.clipmi_patchify(4096, _lib.F16, 8192, 1, R, P, 640, None) == _lib.ERR_SHAPE, (R, P)
        assert "multiple" in _lib.last_error()
    assert _lib.lib.clipmi_patchify(4096, _lib.F16, 8192, 1, 42, 14, 576, None) == _lib.ERR_SHAPE     # kpad below 3 P^2
    assert _lib.lib.clipmi_patchify(4096, _lib.F16, 8192, 0, 42, 14, 640, None) == _lib.OK            # an empty batch launches nothing
