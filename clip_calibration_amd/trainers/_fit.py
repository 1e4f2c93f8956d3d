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


def checked_shard(who: str, fit_args: dict, family=None, **facts):
    """``fit_args``' ``shard`` (or None) after ``shard.check``'s refusals in ``family``'s words, validation by ``val_loader=`` included:
    called in front of ``validation_set``, before either tower runs.  ``facts``: what the trainer knows (``n_cls``, ``n_prompt``, ..)."""
    shard = fit_args.get("shard")
    if shard is not None:
        from ..shard import check
        if family != "coop":    # coopfit's entry points take no ``one_call``
            facts["one_call"] = bool(fit_args.get("one_call", False))
        val = fit_args.get("val_loader") if fit_args.get("val_loader") is not None else fit_args.get("val")
        check(who, shard, family, val=val, final_model=fit_args.get("final_model", "last_step"), **facts)
    return shard


def validation_set(who: str, clip_model, fit_args: dict) -> None:
    """``fit_args``' ``val_loader`` turned into ``fit_args["val"]``; ``val_loader`` together with ``val`` is refused.  With a
    ``clip_model`` the loader is an iterable of (preprocessed image, label) batches, run through the frozen image tower once, and ``val`` is
    the cached ``(features, labels)``.  The image-tower fits pass None: the prompts change the image features every epoch, so nothing is
    cached and ``val`` is ``(val_loader, None)``, a sized iterable of (test-transformed images, labels) batches on the GPU that is iterated
    once per validated epoch."""
    val_loader = fit_args.pop("val_loader", None)
    if val_loader is not None and fit_args.get("val") is not None:
        raise ValueError(f"{who}: val_loader and val are two ways to give one validation set")
    if val_loader is not None:
        fit_args["val"] = (val_loader, None) if clip_model is None else cached_features(who, clip_model, val_loader)


def split_monitor_args(who: str, fit_args: dict, n_classes=None, E=None) -> dict:
    """The ``transform=`` route: the validation arguments popped out of ``fit_args`` and checked as the fit functions check them, as the
    dict ``watch``: ``val`` (or None), ``val_bins``, ``final_model``, ``val_criterion``, ``return_monitor``.  The cached-feature fits give
    ``n_classes`` and ``E``, and ``val`` comes back as ``fitmonitor.check_val`` leaves it; the image-tower fits give neither, and the dict
    has their ``val_batch_size`` too (the validation images are the caller's test-transformed ones; the train transform never touches
    them)."""
    from .. import fitmonitor
    w = {"val": fit_args.pop("val", None), "val_bins": fit_args.pop("val_bins", 10), "final_model": fit_args.pop("final_model", "last_step"),
         "val_criterion": fit_args.pop("val_criterion", "accuracy"), "return_monitor": bool(fit_args.pop("return_monitor", False))}
    if n_classes is None:
        w["val_batch_size"] = fit_args.pop("val_batch_size", 32)
        fitmonitor.check_image_args(who, w["val"], w["val_batch_size"], w["val_bins"], w["final_model"], w["val_criterion"])
    else:
        fitmonitor.check_args(who, w["val"], w["val_bins"], w["final_model"], w["val_criterion"])
        if w["val"] is not None:
            w["val"] = fitmonitor.check_val(who, w["val"], E, n_classes)
    return w


def monitored_end_epoch(state, watch: dict, epochs: int, monitored: bool, before=None):
    """``end_epoch`` for ``augment.fit_with_transform``: ``before(e)`` (PromptSRC's GPA work), then, when the run is ``monitored``, the
    state's ``validate`` on ``watch``'s set, on a monitor started here; None when there is neither."""
    if monitored:
        state.start_monitor(int(epochs), watch["val_bins"], select=watch["final_model"] == "best_val", val_criterion=watch["val_criterion"])
    if not monitored and before is None:
        return None
    chunk = (watch["val_batch_size"],) if "val_batch_size" in watch else ()

    def end_epoch(e: int) -> None:
        if before is not None:
            before(e)
        if monitored:
            state.validate(watch["val"][0], watch["val"][1], e, *chunk)
    return end_epoch


def run_with_transform(who: str, state, clip_model, n_classes: int, E: int, loader, transform, epochs, lr, run: dict, watch: dict):
    """``augment.fit_with_transform`` with the state's ``validate`` behind every epoch when a validation set was given (its features
    computed once, by the caller, with the test transform).  Returns ``(losses, monitor dict or None)``."""
    from ..augment import fit_with_transform
    if watch["val"] is not None:
        vf, vl = watch["val"]
        watch = dict(watch, val=(vf, vl.to(vf.device)))
    end_epoch = monitored_end_epoch(state, watch, epochs, watch["val"] is not None)
    losses = fit_with_transform(state, clip_model.image_features_f32, n_classes, loader, transform, epochs, lr, end_epoch=end_epoch, **run)
    return losses, (state.monitor() if watch["return_monitor"] else None)


def image_end_epoch(state, watch: dict, epochs: int, steps: int, before=None):
    """``(end_epoch, monitored)`` of an image-tower fit: it is monitored when a validation set was given and the run has steps."""
    monitored = watch["val"] is not None and int(epochs) * steps > 0
    return monitored_end_epoch(state, watch, epochs, monitored, before), monitored


def pack_monitored(state, fitted, losses, watch: dict, monitored: bool):
    """``pack`` with the monitor's dict behind the history when ``return_monitor`` was asked for."""
    from .. import fitmonitor
    out = pack(fitted, losses)
    if not watch["return_monitor"]:
        return out
    mon = fitmonitor.returned_monitor(state, monitored, watch["val_bins"], True)
    return out + (mon,) if isinstance(out, tuple) else (out, mon)
