"""What the fits with per-epoch validation share (DESIGN.md "Fit monitor"; reference base_learner.py:41-47, Dassl's ``after_epoch``): the
argument checks of ``val`` / ``val_bins`` / ``final_model`` / ``val_criterion``, the device history -- epoch records, the best block and the
best slot -- and the dict ``monitor()`` returns.  ``coopfit`` reads the dict's code from here; ``adapterfit`` and ``taskresfit`` use all of
it, both for their one-call monitored runs (``ops.adapter_fit`` / ``ops.taskres_fit`` with ``monitor=``) and for ``*FitState.validate``.
Nothing here knows the byte layout of a record: that stays with ``ops``' helpers."""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch

from . import fitloop, ops
from ._lib import lib

FINAL_MODELS = ("last_step", "best_val")


def empty_monitor(val_bins: int = 10) -> dict:
    """What ``monitor()`` returns when nothing has been validated."""
    z = np.zeros(0, np.float64)
    return {"accuracy": z, "nll": z.copy(), "ece": z.copy(), "bins": np.zeros((0, 3, int(val_bins) + 1)), "records": [], "best_epoch": None}


def monitor_dict(records: torch.Tensor, n_bins: int, block: Optional[torch.Tensor]) -> dict:
    """The validated epochs' ``records`` (uint8 [epochs, bytes] on the device) as numbers: per epoch ``accuracy``, ``nll`` (the mean over
    the rows) and ``ece`` (``metrics.ece_from_bins`` of the record's bins), the raw ``bins`` (float64 [epochs, 3, n_bins + 1]: count, sum of
    confidences, correct), the decoded ``records`` and ``best_epoch`` (None without a best ``block``, -1 when no epoch was taken).  It
    reads the history back: one synchronisation."""
    from . import metrics
    recs = ops.decode_val_records(records, n_bins)
    bins = np.stack([ops.val_record_bins(r) for r in recs]) if recs else np.zeros((0, 3, n_bins + 1))
    n = np.array([max(r["n"], 1) for r in recs], np.float64)
    return {"accuracy": np.array([r["correct"] for r in recs], np.float64) / n, "nll": np.array([r["nll_sum"] for r in recs], np.float64) / n,
            "ece": np.array([metrics.ece_from_bins(b, n_bins) for b in bins], np.float64), "bins": bins, "records": recs,
            "best_epoch": None if block is None else ops.decode_best_block(block)["best_epoch"]}


def check_args(who: str, val, val_bins, final_model, val_criterion) -> None:
    """``coopfit.fit_context``'s checks of the validation arguments, with its messages."""
    if final_model not in FINAL_MODELS:
        raise ValueError(f"{who}: final_model={final_model!r} must be one of {FINAL_MODELS}")
    if val_criterion not in ops.VAL_CRITERIA:
        raise ValueError(f"{who}: val_criterion={val_criterion!r} must be one of {sorted(ops.VAL_CRITERIA)}")
    if final_model == "best_val" and val is None:
        raise ValueError(f"{who}: final_model='best_val' needs val=(val_features, val_labels)")
    if val is not None:
        if not isinstance(val, (tuple, list)) or len(val) != 2:
            raise ValueError(f"{who}: val must be (val_features, val_labels)")
        ops._val_bins(who, val_bins)


def check_val(who: str, val, E: int, C: int):
    """``(val_features, val_labels)`` of a checked ``val``: the features [N_val >= 1, E]; labels that are not an int64 tensor on the GPU are
    range-checked on the host, before anything is launched, and come back as an int64 host tensor."""
    vf, vl = val
    if not isinstance(vf, torch.Tensor) or vf.dim() != 2 or vf.shape[0] < 1 or vf.shape[1] != E:
        raise ValueError(f"{who}: val_features must be a [N_val >= 1, E = {E}] tensor")
    if not fitloop._on_gpu_as_is(vl):
        vl = torch.from_numpy(fitloop._labels(who, vl, vf.shape[0], C, "validation rows").astype(np.int64))
    return vf, vl


def pack(fitted, history, monitor, return_history: bool, return_monitor: bool):
    """``fitted`` (a tensor or a tuple of tensors), then the history, then the monitor's dict, each when asked for."""
    res = (fitted if isinstance(fitted, tuple) else (fitted,)) + ((history,) if return_history else ()) + ((monitor,) if return_monitor else ())
    return res if len(res) > 1 else res[0]


class Monitor:
    """The device history of one fit: ``slots`` epoch records of ``val_bins`` confidence bins and, when ``params`` is given, the best block
    and the best slot -- a copy of ``params`` (one contiguous fp32 block on the GPU: what ``clipmi_best_select`` copies) as it is now,
    replaced whenever an epoch is strictly better under ``val_criterion``.  Allocations and one small upload; nothing synchronises."""

    def __init__(self, who: str, slots: int, val_bins: int, val_criterion: str, params: Optional[torch.Tensor], dev):
        if val_criterion not in ops.VAL_CRITERIA:
            raise ValueError(f"{who}: val_criterion={val_criterion!r} must be one of {sorted(ops.VAL_CRITERIA)}")
        self.bins = ops._val_bins(who, val_bins)
        self.records = ops.new_val_records(max(int(slots), 1), self.bins, dev)
        self.criterion, self.seen = val_criterion, 0
        self.block = self.best = None
        if params is not None:
            self.block, self.best = ops.new_best_block(dev), params.clone()
        self.select_ws = torch.empty(256, dtype=torch.uint8, device=dev)
        self.val = self.logits = self.score_ws = self.run_ws = None

    def operands(self, who: str, val_features: torch.Tensor, val_labels, E: int, C: int):
        """The validation set as the kernels take it, made once per set: fp32 features whose rows are read with their stride, the labels
        int64 on the device (an int64 tensor on the GPU is taken as it is; anything else is range-checked on the host), the [N_val, C] fp32
        logits and the scoring workspace."""
        if not isinstance(val_features, torch.Tensor) or val_features.dim() != 2 or val_features.shape[0] < 1 or val_features.shape[1] != E:
            raise ValueError(f"{who}: val_features {tuple(getattr(val_features, 'shape', ()))} must be [N_val >= 1, E = {E}]")
        fitloop._need_gpu(val_features, "val_features")
        key = (val_features.data_ptr(), val_features._version, tuple(val_features.shape), tuple(val_features.stride()), val_features.dtype,
               id(val_labels), getattr(val_labels, "_version", None))
        if self.val is None or self.val[0] != key:
            N = val_features.shape[0]
            labels_d = fitloop.step_labels(who, val_labels, N, C, val_features.device, "validation rows")
            feats = val_features if val_features.dtype == torch.float32 else val_features.float()
            self.val = (key, feats, labels_d, val_labels)
            self.logits = torch.empty(N, C, dtype=torch.float32, device=val_features.device)
            self.score_ws = torch.empty(max(lib.clipmi_val_score_workspace_bytes(N, self.bins), 256), dtype=torch.uint8, device=val_features.device)
        return self.val[1], self.val[2]

    def slot(self, who: str, epoch) -> int:
        """``epoch`` as a checked index into the history, which grows when the index lies behind its end."""
        if isinstance(epoch, bool) or int(epoch) != epoch or int(epoch) < 0:
            raise ValueError(f"{who}: epoch={epoch} must be an integer >= 0")
        epoch = int(epoch)
        if epoch >= self.records.shape[0]:
            grown = ops.new_val_records(epoch + 1, self.bins, self.records.device)
            grown[:self.records.shape[0]].copy_(self.records)
            self.records = grown
        return epoch

    def score(self, epoch: int, labels_d: torch.Tensor, params: Optional[torch.Tensor]) -> None:
        """``self.logits`` into record ``epoch`` and, when the monitor selects, ``params`` into the best slot under the decision; enqueued."""
        record = self.records[epoch]
        ops.val_score(self.logits, labels_d, self.bins, record, self.score_ws)
        if self.block is not None:
            ops.best_select(record, self.block, self.criterion, epoch, params, self.best, self.select_ws)
        self.seen = max(self.seen, epoch + 1)

    def summary(self) -> dict:
        return monitor_dict(self.records[:self.seen], self.bins, self.block)
