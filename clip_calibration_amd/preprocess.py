"""The reference's test transform on the device: decoded uint8 RGB images of any size -> the [B, 3, n_px, n_px] tensor
``model.encode_image`` takes (clip/clip.py:74-81 ``_transform``; Dassl's test transform with ``INPUT.INTERPOLATION`` "bicubic" or
"bilinear" and ``INPUT.PIXEL_MEAN`` / ``PIXEL_STD``, configs/trainers/*/vit_b16.yaml):

    Resize(n_px, BICUBIC) on the shorter side -> CenterCrop(n_px) -> ToTensor -> Normalize(mean, std) [-> .half()]

computed by ``clipmi_preprocess`` (csrc/preprocess.hip) bit for bit as Pillow + torchvision compute it on the host, so the host only
decodes.  ``Preprocess`` takes a uint8 CUDA tensor [B,H,W,3] or [B,3,H,W], a list of uint8 [H_i,W_i,3] tensors / ndarrays (host or
device), or a ``PackedImages`` -- the flat form a DataLoader ``collate_fn=pack_images`` builds in its workers.
"""
from __future__ import annotations

import collections
import ctypes as C
from typing import List, Sequence, Tuple, Union

import numpy as np
import torch

from . import _lib
from ._lib import _DT, check, lib

CLIP_MEAN = (0.48145466, 0.4578275, 0.40821073)     # clip/clip.py:80
CLIP_STD = (0.26862954, 0.26130258, 0.27577711)
_FILTERS = {"bicubic": _lib.FILTER_BICUBIC, "bilinear": _lib.FILTER_BILINEAR}


def resize_geometry(height: int, width: int, n_px: int) -> Tuple[int, int, int, int]:
    """(new_h, new_w, top, left) of torchvision ``Resize(n_px)`` (shorter side -> n_px, longer side ``int(n_px * long / short)``)
    followed by ``CenterCrop(n_px)`` (``int(round((new - n_px) / 2.0))``: Python's round, half to even)."""
    if height < 1 or width < 1 or n_px < 1:
        raise ValueError(f"resize_geometry: bad size {height} x {width} -> {n_px}")
    short, long = min(height, width), max(height, width)
    new_short, new_long = n_px, int(n_px * long / short)
    new_h, new_w = (new_short, new_long) if height <= width else (new_long, new_short)
    return new_h, new_w, int(round((new_h - n_px) / 2.0)), int(round((new_w - n_px) / 2.0))


def normalize_table(mean: Sequence[float] = CLIP_MEAN, std: Sequence[float] = CLIP_STD) -> torch.Tensor:
    """fp32 [3, 256]: ToTensor + Normalize of every byte value, with torchvision's own torch CPU fp32 ops
    (``img.float().div(255)`` then ``sub_(mean).div_(std)``); the kernel looks the resized bytes up in it."""
    u = torch.arange(256, dtype=torch.uint8).expand(3, 256)
    t = u.to(torch.float32).div(255)
    m = torch.as_tensor(mean, dtype=torch.float32)[:, None]
    s = torch.as_tensor(std, dtype=torch.float32)[:, None]
    return t.sub_(m).div_(s).contiguous()


def identity_table() -> torch.Tensor:
    """fp32 [3, 256] with entry u = u: the kernel then returns the resized, cropped bytes themselves (as fp32)."""
    return torch.arange(256, dtype=torch.float32).expand(3, 256).contiguous()


class PackedImages:
    """A batch of HWC uint8 RGB images of different sizes as one flat uint8 buffer (``data``) plus an int64 table ``shapes``
    [B, 3] of (byte offset, height, width).  Built by ``pack_images``; ``pin_memory()`` and ``to()`` move it as one block, so a
    DataLoader with ``collate_fn=pack_images, pin_memory=True`` hands over batches that cross to the GPU in one copy."""

    def __init__(self, data: torch.Tensor, shapes: torch.Tensor):
        if data.dtype != torch.uint8 or data.dim() != 1:
            raise TypeError("PackedImages: data must be a flat uint8 tensor")
        shapes = torch.as_tensor(shapes, dtype=torch.int64).cpu()
        if shapes.dim() != 2 or shapes.shape[1] != 3:
            raise ValueError("PackedImages: shapes must be [B, 3] (offset, height, width)")
        self.data, self.shapes = data, shapes

    def __len__(self) -> int:
        return self.shapes.shape[0]

    @property
    def device(self) -> torch.device:
        return self.data.device

    @property
    def is_cuda(self) -> bool:
        return self.data.is_cuda

    def is_pinned(self) -> bool:
        return self.data.is_pinned()

    def pin_memory(self) -> "PackedImages":
        return PackedImages(self.data.pin_memory(), self.shapes)

    def to(self, device, non_blocking: bool = False) -> "PackedImages":
        return PackedImages(self.data.to(device, non_blocking=non_blocking), self.shapes)

    def cuda(self, non_blocking: bool = False) -> "PackedImages":
        return self.to("cuda", non_blocking=non_blocking)


def _as_hwc(img) -> Union[np.ndarray, torch.Tensor]:
    if isinstance(img, torch.Tensor):
        t = img
    else:
        t = np.asarray(img)
    if t.dtype not in (np.uint8, torch.uint8) or t.ndim != 3 or t.shape[2] != 3:
        raise TypeError(f"images must be uint8 [H, W, 3] RGB, got {getattr(t, 'dtype', type(t))} {tuple(t.shape)}")
    return t


def pack_images(batch: Sequence) -> Union[PackedImages, Tuple[PackedImages, torch.Tensor]]:
    """``collate_fn`` for a DataLoader of decoded images: a list of uint8 [H_i, W_i, 3] host tensors / ndarrays -> ``PackedImages``;
    a list of (image, label) pairs -> (``PackedImages``, int64 labels)."""
    labels = None
    if len(batch) and isinstance(batch[0], (tuple, list)):
        labels = torch.as_tensor([int(lab) for _, lab in batch], dtype=torch.int64)
        batch = [img for img, _ in batch]
    imgs = [_as_hwc(i) for i in batch]
    if any(isinstance(i, torch.Tensor) and i.is_cuda for i in imgs):
        raise TypeError("pack_images packs HOST images (a DataLoader's collate_fn); pass device images to Preprocess directly")
    packed = _pack_host(imgs, pin=False)
    return packed if labels is None else (packed, labels)


def _pack_host(imgs, pin: bool) -> PackedImages:
    sizes = [int(i.shape[0]) * int(i.shape[1]) * 3 for i in imgs]
    offsets = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int64) if imgs else np.zeros(0, np.int64)
    data = torch.empty(int(sum(sizes)), dtype=torch.uint8, pin_memory=pin)
    flat = data.numpy()
    for img, off, n in zip(imgs, offsets, sizes):
        a = img.numpy() if isinstance(img, torch.Tensor) else img
        flat[off:off + n] = np.ascontiguousarray(a).reshape(-1)
    shapes = torch.as_tensor(np.stack([offsets, [i.shape[0] for i in imgs], [i.shape[1] for i in imgs]], axis=1), dtype=torch.int64)
    return PackedImages(data, shapes)


class Preprocess:
    """``Resize(n_px, interpolation) -> CenterCrop(n_px) -> ToTensor -> Normalize(mean, std)`` on the GPU, output ``dtype``
    (fp16 by default: ``encode_image`` casts to the model's fp16 anyway, and takes fp16 without a cast pass).  ``normalize=False``
    replaces ToTensor + Normalize by the identity: the output holds the resized bytes (exactly, in fp32).  Every call runs on the
    current stream and leaves the host free (no synchronisation)."""

    def __init__(self, n_px: int, mean: Sequence[float] = CLIP_MEAN, std: Sequence[float] = CLIP_STD, interpolation: str = "bicubic",
                 dtype: torch.dtype = torch.float16, normalize: bool = True):
        if interpolation not in _FILTERS:
            raise ValueError(f"Preprocess: interpolation {interpolation!r} is not supported (bicubic, bilinear)")
        if dtype not in _DT:
            raise TypeError(f"Preprocess: dtype must be torch.float16 or torch.float32, got {dtype}")
        if not 1 <= int(n_px) <= 4096:
            raise ValueError(f"Preprocess: n_px = {n_px} outside 1 .. 4096")
        self.n_px, self.interpolation, self.dtype = int(n_px), interpolation, dtype
        self.table = normalize_table(mean, std) if normalize else identity_table()
        self._tables = {}                 # device -> fp32 [3, 256] on that device
        self._inflight = collections.deque()   # (page-locked descriptors, event): kept until the stream has passed their upload

    @classmethod
    def for_model(cls, model, **kw) -> "Preprocess":
        """n_px from ``model.visual.input_resolution`` (224 for ViT-B/16, 336 for ViT-L/14@336), output in ``model.dtype``."""
        kw.setdefault("dtype", getattr(model, "dtype", torch.float16))
        return cls(int(model.visual.input_resolution), **kw)

    def _table(self, dev: torch.device) -> torch.Tensor:
        t = self._tables.get(dev)
        if t is None:
            t = self._tables[dev] = self.table.to(dev)
        return t

    def __call__(self, images) -> torch.Tensor:
        dev = torch.device("cuda", torch.cuda.current_device())
        return self._run(*self._gather(images, dev), dev)

    def _gather(self, images, dev: torch.device):
        """Any input form -> (device uint8 buffer, host descriptors int64 [B, 5] laid out as clipmi_image_desc, B)."""
        if isinstance(images, PackedImages):
            if not images.is_cuda:
                images = images.to(dev, non_blocking=images.is_pinned())
            return images.data, self._packed_descs(images), len(images)
        if isinstance(images, torch.Tensor):
            return self._dense(images, dev)
        if isinstance(images, (list, tuple)):
            imgs = [_as_hwc(i) for i in images]
            if not imgs:
                raise ValueError("Preprocess: empty image list")
            if all(isinstance(i, torch.Tensor) and i.is_cuda for i in imgs):
                flat = torch.cat([i.reshape(-1) for i in imgs])       # one device buffer (a device copy)
                sizes = [i.numel() for i in imgs]
                offsets = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int64)
                packed = PackedImages(flat, np.stack([offsets, [i.shape[0] for i in imgs], [i.shape[1] for i in imgs]], axis=1))
            elif any(isinstance(i, torch.Tensor) and i.is_cuda for i in imgs):
                raise TypeError("Preprocess: a list mixes host and device images")
            else:
                packed = _pack_host(imgs, pin=True).to(dev, non_blocking=True)   # one pinned buffer, one copy
            return packed.data, self._packed_descs(packed), len(packed)
        raise TypeError(f"Preprocess: unsupported input {type(images)}")

    @staticmethod
    def _packed_descs(p: PackedImages) -> np.ndarray:
        s = p.shapes.numpy()
        d = np.zeros((len(p), 5), dtype=np.int64)
        d[:, 0] = s[:, 0]
        d32 = d.view(np.int32)
        d32[:, 2], d32[:, 3] = s[:, 1], s[:, 2]
        d[:, 2], d[:, 3], d[:, 4] = 3 * s[:, 2], 3, 1
        return d

    def _dense(self, t: torch.Tensor, dev: torch.device):
        if t.dtype != torch.uint8 or t.dim() != 4 or not (t.shape[3] == 3 or t.shape[1] == 3):
            raise TypeError(f"Preprocess: expected a uint8 [B,H,W,3] or [B,3,H,W] tensor, got {t.dtype} {tuple(t.shape)}")
        if not t.is_cuda:
            t = t.to(dev, non_blocking=t.is_pinned())
        if any(s < 0 for s in t.stride()):
            raise ValueError("Preprocess: negative strides")
        B = t.shape[0]
        if t.shape[3] == 3:     # [B, H, W, 3]
            H, W = t.shape[1], t.shape[2]
            sb, sy, sx, sc = t.stride(0), t.stride(1), t.stride(2), t.stride(3)
        else:                   # [B, 3, H, W]
            H, W = t.shape[2], t.shape[3]
            sb, sc, sy, sx = t.stride(0), t.stride(1), t.stride(2), t.stride(3)
        d = np.zeros((B, 5), dtype=np.int64)
        d[:, 0] = np.arange(B, dtype=np.int64) * sb
        d32 = d.view(np.int32)
        d32[:, 2], d32[:, 3] = H, W
        d[:, 2], d[:, 3], d[:, 4] = sy, sx, sc
        return t, d, B

    def _run(self, buf: torch.Tensor, descs: np.ndarray, B: int, dev: torch.device) -> torch.Tensor:
        if buf.device != dev:
            raise RuntimeError(f"Preprocess: images on {buf.device}, current device is {dev}")
        extent = 1 + sum((s - 1) * st for s, st in zip(buf.shape, buf.stride())) if buf.numel() else 0
        while self._inflight and self._inflight[0][1].query():
            self._inflight.popleft()
        host = torch.from_numpy(descs).pin_memory()   # page-locked: the upload on the stream is a true async copy
        filt = _FILTERS[self.interpolation]
        nbytes = lib.clipmi_preprocess_workspace_bytes(C.c_void_p(host.data_ptr()), B, self.n_px, filt)
        if nbytes == 0:
            raise _lib.ClipmiError(_lib.ERR_ARG, "clipmi_preprocess_workspace_bytes", _lib.last_error())
        n = self.n_px
        out = torch.empty((B, 3, n, n), dtype=self.dtype, device=dev)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)   # stream-ordered by the caching allocator: no reuse across streams in flight
        stream = torch.cuda.current_stream(dev)
        check(lib.clipmi_preprocess(buf.data_ptr(), extent, host.data_ptr(), B, n, filt, self._table(dev).data_ptr(), out.data_ptr(),
                                    _DT[self.dtype], ws.data_ptr(), nbytes, stream.cuda_stream), "clipmi_preprocess")
        ev = torch.cuda.Event()
        ev.record(stream)
        self._inflight.append((host, ev))
        return out
