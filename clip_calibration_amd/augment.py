"""The reference's TRAIN transform on the device.  Every training config of the reference has ``INPUT.TRANSFORMS:
["random_resized_crop", "random_flip", "normalize"]`` with ``SIZE: (224, 224)`` and ``INTERPOLATION: "bicubic"``, which Dassl builds as

    RandomResizedCrop(size, scale, interpolation) -> RandomHorizontalFlip() -> ToTensor -> Normalize(mean, std)

``sample_views`` draws the crops and flips on the host with torch's CPU RNG, ``TrainPreprocess`` applies them with ``clipmi_augment``
(csrc/augment.hip): ``img.crop(box).resize((n_px, n_px), filter)``, the flip, and the normalising table, bit for bit as Pillow and
torchvision's PIL path compute them.  ``fit_with_transform`` is the per-batch training loop ``CLIPAdapterCLIP.fit_adapter(loader,
transform=...)`` and ``TaskResCLIP.fit_residuals(loader, transform=...)`` run: transform, image tower, optimiser step, enqueued batch
after batch with no host synchronisation until the end.

torchvision and Dassl are not part of this repository's environment.  What is restated from their public sources and UNVERIFIED here:
* the order of the draws in ``RandomResizedCrop.get_params`` and ``RandomHorizontalFlip`` (``sample_views``);
* the defaults ``scale=(0.08, 1.0)`` (Dassl's ``INPUT.RRCROP_SCALE``), ``ratio=(3/4, 4/3)`` and ``flip_p=0.5``;
* that Dassl composes the flip AFTER the resized crop (the order of ``INPUT.TRANSFORMS``), so the flip mirrors the resized image.
That is why each of them is an argument and why explicit views are accepted wherever views are sampled.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Callable, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib, fitloop
from ._lib import _DT, check, lib
from .preprocess import CLIP_MEAN, CLIP_STD, Preprocess, _FILTERS

Views = Tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray, np.ndarray, np.ndarray]


def sample_views(shapes, scale: Sequence[float] = (0.08, 1.0), ratio: Sequence[float] = (3.0 / 4.0, 4.0 / 3.0), flip_p: float = 0.5,
                 generator: Optional[torch.Generator] = None, views_per_image: int = 1) -> Views:
    """Random crops and flips for images of the given ``shapes`` ([B, 2] of (height, width)): host int32 arrays ``(image, top, left,
    height, width, flip)`` of ``B * views_per_image`` views, the views of image b at ``b * views_per_image ...``.

    Per view, torchvision's ``RandomResizedCrop.get_params`` then ``RandomHorizontalFlip``, drawn from torch's CPU RNG (``generator``, or
    the global one) in this order: up to 10 tries of ``target_area = H * W * torch.empty(1).uniform_(scale[0], scale[1])``,
    ``aspect = exp(torch.empty(1).uniform_(log(ratio[0]), log(ratio[1])))`` (the logs taken in fp32, as ``torch.log(torch.tensor(ratio))``
    gives them), ``w = round(sqrt(target_area * aspect))``, ``h = round(sqrt(target_area / aspect))``, accepted when ``0 < w <= W`` and
    ``0 < h <= H`` and then placed by ``torch.randint(0, H - h + 1)`` and ``torch.randint(0, W - w + 1)``; after 10 failures the centre
    crop of the whole image clamped to the ratio bounds; last, one ``torch.rand(1) < flip_p``.

    The draw order and the defaults are unverified restatements of torchvision's and Dassl's public sources (module docstring)."""
    shapes = np.asarray(shapes.cpu() if isinstance(shapes, torch.Tensor) else shapes)
    if shapes.ndim != 2 or shapes.shape[1] != 2 or shapes.dtype.kind not in "iu" or (shapes.size and shapes.min() < 1):
        raise ValueError("sample_views: shapes must be an integer [B, 2] array of (height, width), each >= 1")
    k = int(views_per_image)
    if k < 1:
        raise ValueError(f"sample_views: views_per_image={views_per_image} (>= 1)")
    if not (len(scale) == 2 and 0.0 < scale[0] <= scale[1] and len(ratio) == 2 and 0.0 < ratio[0] <= ratio[1] and 0.0 <= flip_p <= 1.0):
        raise ValueError(f"sample_views: scale={tuple(scale)}, ratio={tuple(ratio)} (0 < low <= high), flip_p={flip_p} (in [0, 1])")
    log_ratio = torch.log(torch.tensor([float(ratio[0]), float(ratio[1])]))
    lo, hi = float(log_ratio[0]), float(log_ratio[1])
    out = np.zeros((6, shapes.shape[0] * k), dtype=np.int32)
    for v in range(out.shape[1]):
        H, W = int(shapes[v // k, 0]), int(shapes[v // k, 1])
        area = H * W
        for _ in range(10):
            target = area * torch.empty(1).uniform_(float(scale[0]), float(scale[1]), generator=generator).item()
            aspect = torch.exp(torch.empty(1).uniform_(lo, hi, generator=generator)).item()
            w, h = int(round(math.sqrt(target * aspect))), int(round(math.sqrt(target / aspect)))
            if 0 < w <= W and 0 < h <= H:
                top = int(torch.randint(0, H - h + 1, size=(1,), generator=generator).item())
                left = int(torch.randint(0, W - w + 1, size=(1,), generator=generator).item())
                break
        else:
            in_ratio = float(W) / float(H)
            if in_ratio < min(ratio):
                w, h = W, int(round(W / min(ratio)))
            elif in_ratio > max(ratio):
                h, w = H, int(round(H * max(ratio)))
            else:
                w, h = W, H
            top, left = (H - h) // 2, (W - w) // 2
        flip = int(torch.rand(1, generator=generator).item() < flip_p)
        out[:, v] = (v // k, top, left, h, w, flip)
    return tuple(out)


def _view_table(views) -> np.ndarray:
    """``views`` (the six arrays ``sample_views`` returns, or an integer [V, 6] array) -> int32 [V, 6] laid out as clipmi_view_desc."""
    if isinstance(views, tuple) and len(views) == 6:      # a tuple is six columns; a list or an array is [V, 6] rows
        a = np.stack([np.asarray(c) for c in views], axis=1)
    else:
        a = np.asarray(views.cpu() if isinstance(views, torch.Tensor) else views)
    if a.ndim != 2 or a.shape[1] != 6 or a.shape[0] < 1 or a.dtype.kind not in "iu":
        raise ValueError("TrainPreprocess: views must be six integer arrays (image, top, left, height, width, flip) or an integer [V >= 1, 6] array")
    if np.abs(a.astype(np.int64)).max() > np.iinfo(np.int32).max:
        raise ValueError("TrainPreprocess: a view field does not fit 32 bits")
    return np.ascontiguousarray(a, dtype=np.int32)


class TrainPreprocess(Preprocess):
    """``RandomResizedCrop((n_px, n_px), scale, ratio, interpolation) -> RandomHorizontalFlip(flip_p) -> ToTensor -> Normalize(mean,
    std)`` on the GPU for the inputs ``Preprocess`` takes (a uint8 [B,H,W,3] / [B,3,H,W] tensor, a list of uint8 [H_i,W_i,3] images, a
    ``PackedImages``); output [V, 3, n_px, n_px] in ``dtype``, ``normalize=False`` returning the resized bytes.  ``tp(images)`` samples
    one view per image with ``sample_views`` (from ``generator``); ``tp(images, views)`` applies the given views -- the tuple of six
    arrays ``sample_views`` returns, or an integer [V, 6] array or list of rows (image, top, left, height, width, flip); several views may
    name one image.
    Every call runs on the current stream and leaves the host free (no synchronisation), so an instance also serves as
    ``runner.device_batches(..., preprocess=...)``.  What is unverified about the sampling and the flip's place: module docstring."""

    def __init__(self, n_px: int, mean: Sequence[float] = CLIP_MEAN, std: Sequence[float] = CLIP_STD, interpolation: str = "bicubic",
                 dtype: torch.dtype = torch.float16, normalize: bool = True, scale: Sequence[float] = (0.08, 1.0),
                 ratio: Sequence[float] = (3.0 / 4.0, 4.0 / 3.0), flip_p: float = 0.5, generator: Optional[torch.Generator] = None):
        super().__init__(n_px, mean, std, interpolation, dtype, normalize)
        sample_views(np.zeros((0, 2), np.int64), scale, ratio, flip_p)   # argument check only
        self.scale, self.ratio, self.flip_p, self.generator = tuple(scale), tuple(ratio), float(flip_p), generator

    def sample(self, shapes, views_per_image: int = 1) -> Views:
        return sample_views(shapes, self.scale, self.ratio, self.flip_p, self.generator, views_per_image)

    def __call__(self, images, views=None) -> torch.Tensor:
        dev = torch.device("cuda", torch.cuda.current_device())
        buf, descs, B = self._gather(images, dev)
        if views is None:
            views = self.sample(descs.view(np.int32)[:, 2:4])
        return self._run_views(buf, descs, B, _view_table(views), dev)

    def _run_views(self, buf: torch.Tensor, descs: np.ndarray, B: int, views: np.ndarray, dev: torch.device) -> torch.Tensor:
        if buf.device != dev:
            raise RuntimeError(f"TrainPreprocess: images on {buf.device}, current device is {dev}")
        extent = 1 + sum((s - 1) * st for s, st in zip(buf.shape, buf.stride())) if buf.numel() else 0
        while self._inflight and self._inflight[0][1].query():
            self._inflight.popleft()
        V = views.shape[0]
        host = torch.from_numpy(descs).pin_memory()     # page-locked: the uploads on the stream are true async copies
        host_v = torch.from_numpy(views).pin_memory()
        filt = _FILTERS[self.interpolation]
        nbytes = lib.clipmi_augment_workspace_bytes(C.c_void_p(host.data_ptr()), B, C.c_void_p(host_v.data_ptr()), V, self.n_px, filt)
        if nbytes == 0:
            raise _lib.ClipmiError(_lib.ERR_ARG, "clipmi_augment_workspace_bytes", _lib.last_error())
        n = self.n_px
        out = torch.empty((V, 3, n, n), dtype=self.dtype, device=dev)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)   # stream-ordered by the caching allocator
        stream = torch.cuda.current_stream(dev)
        check(lib.clipmi_augment(buf.data_ptr(), extent, host.data_ptr(), B, host_v.data_ptr(), V, n, filt, self._table(dev).data_ptr(),
                                 out.data_ptr(), _DT[self.dtype], ws.data_ptr(), nbytes, stream.cuda_stream), "clipmi_augment")
        ev = torch.cuda.Event()
        ev.record(stream)
        self._inflight.append(((host, host_v), ev))
        return out


def fit_with_transform(state, image_features: Callable[[torch.Tensor], torch.Tensor], n_classes: int, loader, transform: TrainPreprocess,
                       epochs: int, lr: float, lr_per_epoch: Optional[Sequence[float]] = None, views: Optional[Callable] = None,
                       return_history: bool = False, end_epoch: Optional[Callable[[int], None]] = None) -> Optional[np.ndarray]:
    """The reference's training regime for a head trained on frozen towers: ``epochs`` passes over ``loader`` -- a sized iterable of
    (decoded uint8 images in any form ``transform`` takes, labels [B]) iterated once per epoch --, every batch going ``transform`` ->
    ``image_features`` (the frozen tower, fp32 [B, E]) -> ``state.step`` (an ``AdapterFitState`` or ``TaskResFitState``).  The rate of a
    step is read from a device array filled once before the first launch: ``lr_per_epoch`` (None: ``cosine_warmup_schedule(lr, epochs)``)
    repeated ``len(loader)`` times.  ``views(epoch, batch_index, shapes)`` supplies explicit views for a batch; None samples one view per
    image from the transform's generator.  Labels on the host are range-checked there and cross from page-locked memory; labels on the
    GPU are taken as ``state.step`` takes them.  Nothing synchronises between the first launch and the one wait at the end; host images
    cross as ``transform`` moves them (page-locked batches without a wait).  ``end_epoch(e)``, when given, is called behind the last step
    of every epoch e (0-based) and must not synchronise (PromptSRC's prompt aggregation).  Returns the per-step losses with
    ``return_history``."""
    if not isinstance(transform, TrainPreprocess):
        raise TypeError(f"transform must be a TrainPreprocess, got {type(transform)}")
    epochs = int(epochs)
    if epochs < 0:
        raise ValueError(f"epochs={epochs} (>= 0)")
    try:
        per_epoch = len(loader)
    except TypeError as e:
        raise TypeError("with a transform the loader is iterated once per epoch and must have a length (a DataLoader or a list)") from e
    dev = torch.device("cuda", torch.cuda.current_device()) if epochs * per_epoch else None
    _, lr_steps = fitloop.schedule("fit_with_transform", lr, epochs, lr_per_epoch, per_epoch, dev)

    def step(e: int, k: int, batch, lr_d: torch.Tensor, want_loss: bool):
        images, labels = batch
        labels = torch.as_tensor(labels)
        if not labels.is_cuda:
            if labels.dtype.is_floating_point or (labels.numel() and (labels.min() < 0 or labels.max() >= n_classes)):
                raise ValueError(f"labels must be integers in the {n_classes} classes [0, {n_classes})")
            labels = labels.to(torch.int64).pin_memory().to(dev, non_blocking=True)
        else:
            labels = labels.to(torch.int64)
        buf, descs, B = transform._gather(images, dev)
        vw = transform.sample(descs.view(np.int32)[:, 2:4]) if views is None else views(e, k, descs.view(np.int32)[:, 2:4].copy())
        x = transform._run_views(buf, descs, B, _view_table(vw), dev)
        return state.step(image_features(x), labels, lr_d, want_loss=want_loss)

    with torch.no_grad():
        return fitloop.run_batches(step, loader, epochs, lr_steps, return_history, end_epoch)
