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


MONITOR_ARGS = ("val", "val_bins", "final_model", "val_criterion", "return_monitor")


def validation_set(who: str, clip_model, fit_args: dict):
    """``fit_args``' ``val_loader`` (an iterable of (preprocessed image, label) batches, run through the frozen image tower once) turned into
    ``fit_args["val"]``, as ``trainers/coop.py`` does; ``val_loader`` together with ``val`` is refused."""
    val_loader = fit_args.pop("val_loader", None)
    if val_loader is not None and fit_args.get("val") is not None:
        raise ValueError(f"{who}: val_loader and val are two ways to give one validation set")
    if val_loader is not None:
        fit_args["val"] = cached_features(who, clip_model, val_loader)


def split_monitor_args(who: str, fit_args: dict, n_classes: int, E: int):
    """The ``transform=`` route: the validation arguments popped out of ``fit_args`` and checked as the cached route checks them.  Returns
    ``(val or None, val_bins, select, val_criterion, return_monitor)``."""
    from .. import fitmonitor
    val, val_bins = fit_args.pop("val", None), fit_args.pop("val_bins", 10)
    final_model, criterion = fit_args.pop("final_model", "last_step"), fit_args.pop("val_criterion", "accuracy")
    return_monitor = bool(fit_args.pop("return_monitor", False))
    fitmonitor.check_args(who, val, val_bins, final_model, criterion)
    if val is not None:
        val = fitmonitor.check_val(who, val, E, n_classes)
    return val, val_bins, final_model == "best_val", criterion, return_monitor


def run_with_transform(who: str, state, clip_model, n_classes: int, E: int, loader, transform, epochs, lr, run: dict, fit_args_monitor):
    """``augment.fit_with_transform`` with the state's ``validate`` behind every epoch when a validation set was given (its features
    computed once, by the caller, with the test transform).  Returns ``(losses, monitor dict or None)``."""
    from ..augment import fit_with_transform
    val, val_bins, select, criterion, return_monitor = fit_args_monitor
    end_epoch = None
    if val is not None:
        vf, vl = val
        vl = vl.to(vf.device)
        state.start_monitor(int(epochs), val_bins, select, criterion)
        end_epoch = lambda e: state.validate(vf, vl, e)
    losses = fit_with_transform(state, clip_model.image_features_f32, n_classes, loader, transform, epochs, lr, end_epoch=end_epoch, **run)
    return losses, (state.monitor() if return_monitor else None)


def image_validation_set(who: str, fit_args: dict) -> None:
    """The image-tower fits: ``fit_args``' ``val_loader`` (a sized iterable of (test-transformed images, labels) batches on the GPU,
    iterated once per validated epoch -- the prompts change the image features every epoch, so nothing is cached) turned into
    ``fit_args["val"] = (val_loader, None)``; ``val_loader`` together with ``val`` is refused."""
    val_loader = fit_args.pop("val_loader", None)
    if val_loader is not None and fit_args.get("val") is not None:
        raise ValueError(f"{who}: val_loader and val are two ways to give one validation set")
    if val_loader is not None:
        fit_args["val"] = (val_loader, None)


def split_image_monitor_args(who: str, fit_args: dict) -> dict:
    """The ``transform=`` route of the image-tower fits: the validation arguments popped out of ``fit_args`` and checked as the fit
    functions check them.  The validation images are the caller's test-transformed ones; the train transform never touches them."""
    from .. import fitmonitor
    w = {"val": fit_args.pop("val", None), "val_batch_size": fit_args.pop("val_batch_size", 32), "val_bins": fit_args.pop("val_bins", 10),
         "final_model": fit_args.pop("final_model", "last_step"), "val_criterion": fit_args.pop("val_criterion", "accuracy"),
         "return_monitor": bool(fit_args.pop("return_monitor", False))}
    fitmonitor.check_image_args(who, w["val"], w["val_batch_size"], w["val_bins"], w["final_model"], w["val_criterion"])
    return w


def image_end_epoch(state, watch: dict, epochs: int, steps: int, before=None):
    """``end_epoch`` for ``augment.fit_with_transform``: ``before(e)`` (PromptSRC's GPA work), then the state's ``validate`` when a
    validation set was given and the run has steps; None when there is neither."""
    monitored = watch["val"] is not None and int(epochs) * steps > 0
    if monitored:
        state.start_monitor(int(epochs), watch["val_bins"], watch["val_criterion"], watch["final_model"] == "best_val")
    if not monitored and before is None:
        return None, False

    def end_epoch(e: int) -> None:
        if before is not None:
            before(e)
        if monitored:
            state.validate(watch["val"][0], watch["val"][1], e, watch["val_batch_size"])
    return end_epoch, monitored


def pack_monitored(state, fitted, losses, watch: dict, monitored: bool):
    """``pack`` with the monitor's dict behind the history when ``return_monitor`` was asked for."""
    from .. import fitmonitor
    out = pack(fitted, losses)
    if not watch["return_monitor"]:
        return out
    mon = state.monitor() if monitored else fitmonitor.empty_monitor(watch["val_bins"])
    return out + (mon,) if isinstance(out, tuple) else (out, mon)
