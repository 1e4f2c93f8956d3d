"""What the trainers' ``fit_*`` wrappers share: the split of ``fit_args``, the shape of the result and the cached-feature pass."""
from __future__ import annotations

import torch


def split_fit_args(fit_args: dict, epochs: int, lr: float):
    """``(run, epochs, lr)`` popped out of ``fit_args``: ``augment.fit_with_transform``'s own arguments, and the run's length and rate with
    the trainer's defaults.  What is left in ``fit_args`` belongs to the ``*FitState``."""
    run = {k: fit_args.pop(k) for k in ("lr_per_epoch", "views", "return_history") if k in fit_args}
    return run, fit_args.pop("epochs", epochs), fit_args.pop("lr", lr)


def pack(fitted, losses):
    """The fitted values as the ``*fit`` functions return them: alone, or followed by the history when there is one."""
    if losses is None:
        return fitted
    return fitted + (losses,) if isinstance(fitted, tuple) else (fitted, losses)


def cached_features(who: str, clip_model, loader):
    """``(features fp32 [N, E], labels int64 [N])`` on the device: one pass of ``loader``, an iterable of (preprocessed images, labels)
    batches, through the frozen image tower."""
    feats, labels = [], []
    with torch.no_grad():
        for image, label in loader:
            f = clip_model.image_features_f32(image)
            feats.append(f)
            labels.append(torch.as_tensor(label).to(device=f.device, dtype=torch.int64))
    if not feats:
        raise ValueError(f"{who}: the loader gave no batch")
    return torch.cat(feats), torch.cat(labels)
