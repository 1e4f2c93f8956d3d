"""clip_calibration_amd: the MI355X (gfx950) CLIP inference-and-calibration path.  Submodules are imported on use; the public
image preprocessing (``Preprocess``, ``PackedImages``, ``pack_images``) is reachable from the package itself."""

_PREPROCESS = ("Preprocess", "PackedImages", "pack_images", "resize_geometry", "normalize_table", "CLIP_MEAN", "CLIP_STD")
__all__ = list(_PREPROCESS)


def __getattr__(name):
    # lazy: importing the package does not load libclipmi.so (bench.py's host-side processes import submodules that never need it)
    if name in _PREPROCESS:
        from . import preprocess
        return getattr(preprocess, name)
    raise AttributeError(f"module 'clip_calibration_amd' has no attribute {name!r}")
