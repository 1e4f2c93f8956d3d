"""What the fits with per-epoch validation share (DESIGN.md "Fit monitor"; reference base_learner.py:41-47, Dassl's ``after_epoch``): the
monitor's whole host state.  This module is the only place that knows it.

* The argument checks of ``val`` / ``val_bins`` / ``final_model`` / ``val_criterion`` with their messages (``check_args``,
  ``check_image_args``, ``check_val``) and the shape of a fit function's result (``pack``, ``returned_monitor``, ``empty_monitor``).
* Three history classes.  ``History``: the epoch records, the best block and the best slot on the device, the growth of the records
  (``slot``), the selection (``select``) and the one cache of a cached-feature validation set (``val_set``: shape and device checks, the
  key, the labels; the caller says how the features are prepared).  ``Monitor`` adds the [N_val, C] logits and ``clipmi_val_score``'s
  workspace; ``ImageMonitor`` the 16 N_val bytes of row results of a row-chunked score, and the chunks of a validation set of images.
* One mix-in, ``Monitored``, that every ``*FitState`` inherits: ``start_monitor``, the auto-start, ``monitor``, ``monitor_records``,
  ``val_logits`` / ``val_row_results`` and the best slot.  ``ImageMonitored`` is the same with the image states' argument order.

A state names its history class and its master block and writes its own ``validate`` (DESIGN.md "Fit monitor" has the table of the nine).
TempScaling has no monitor: it trains on the validation loader itself, so a per-epoch validation would be its own training loss.  Nothing
here knows the byte layout of a record: that stays with ``ops``' helpers."""
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


def check_args(who: str, val, val_bins, final_model, val_criterion, first: str = "val_features") -> None:
    """The checks of the validation arguments that every fit function makes first, with one set of messages.  ``first`` names the pair's first element: the
    image-tower fits take ``val_images_or_loader`` there (a tensor of images or a loader of batches; ``ImageMonitor`` checks which)."""
    if final_model not in FINAL_MODELS:
        raise ValueError(f"{who}: final_model={final_model!r} must be one of {FINAL_MODELS}")
    if val_criterion not in ops.VAL_CRITERIA:
        raise ValueError(f"{who}: val_criterion={val_criterion!r} must be one of {sorted(ops.VAL_CRITERIA)}")
    if final_model == "best_val" and val is None:
        raise ValueError(f"{who}: final_model='best_val' needs val=({first}, val_labels)")
    if val is not None:
        if not isinstance(val, (tuple, list)) or len(val) != 2:
            raise ValueError(f"{who}: val must be ({first}, val_labels)")
        ops._val_bins(who, val_bins)


def check_image_args(who: str, val, val_batch_size, val_bins, final_model, val_criterion) -> None:
    """``check_args`` for a ``val=(val_images_or_loader, val_labels)`` and its ``val_batch_size``."""
    check_args(who, val, val_bins, final_model, val_criterion, "val_images_or_loader")
    if val is not None:
        _batch_size(who, val_batch_size)


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


def returned_monitor(source, monitored: bool, val_bins: int, return_monitor: bool) -> Optional[dict]:
    """The monitor's dict as a fit function returns it: None when it was not asked for, ``empty_monitor(val_bins)`` when the run was not
    monitored (no ``val``, or no step), else what ``source`` -- a ``History``, or a state with ``monitor()`` -- has recorded."""
    if not return_monitor:
        return None
    if not monitored:
        return empty_monitor(val_bins)
    return source.summary() if isinstance(source, History) else source.monitor()


def _fp32(features: torch.Tensor) -> torch.Tensor:
    return features if features.dtype == torch.float32 else features.float()


class History:
    """The device history of one fit: ``slots`` epoch records of ``val_bins`` confidence bins and, when ``params`` is given, the best block
    and the best slot -- a copy of ``params`` (one contiguous fp32 block on the GPU: what ``clipmi_best_select`` copies) as it is now,
    replaced whenever an epoch is strictly better under ``val_criterion``.  Allocations and one small upload; nothing synchronises.
    ``Monitor`` feeds it from cached features, ``ImageMonitor`` from images."""

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
        self.val = None     # val_set's cache: (key, prepared features, labels on the device, the labels as given)

    def val_set(self, who: str, val_features: torch.Tensor, val_labels, E: int, C: int, prepare):
        """A cached-feature validation set as the kernels take it, made once per set: ``(prepare(val_features), labels int64 on the
        device, made now)``.  An int64 label tensor on the GPU is taken as it is; anything else is range-checked on the host.  "Once per
        set" goes by the tensors' addresses, versions, shapes, strides and types: labels given as a list or an array and changed in place
        between two validations keep their first upload -- pass a new object, or a tensor."""
        if not isinstance(val_features, torch.Tensor) or val_features.dim() != 2 or val_features.shape[0] < 1 or val_features.shape[1] != E:
            raise ValueError(f"{who}: val_features {tuple(getattr(val_features, 'shape', ()))} must be [N_val >= 1, E = {E}]")
        fitloop._need_gpu(val_features, "val_features")
        key = (val_features.data_ptr(), val_features._version, tuple(val_features.shape), tuple(val_features.stride()), val_features.dtype,
               id(val_labels), getattr(val_labels, "_version", None))
        made = self.val is None or self.val[0] != key
        if made:
            labels_d = fitloop.step_labels(who, val_labels, val_features.shape[0], C, val_features.device, "validation rows")
            self.val = (key, prepare(val_features), labels_d, val_labels)
        return self.val[1], self.val[2], made

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

    def select(self, epoch: int, params: Optional[torch.Tensor]) -> None:
        """Behind the scoring of record ``epoch``: when the history selects, ``params`` into the best slot under the decision; enqueued."""
        if self.block is not None:
            ops.best_select(self.records[epoch], self.block, self.criterion, epoch, params, self.best, self.select_ws)
        self.seen = max(self.seen, epoch + 1)

    def summary(self) -> dict:
        return monitor_dict(self.records[:self.seen], self.bins, self.block)


class Monitor(History):
    """``History`` for the fits that score an [N_val, C] logits matrix (``coopfit``, ``adapterfit``, ``taskresfit``): the validation
    features, their labels, the logits and ``clipmi_val_score``'s workspace."""

    def __init__(self, who: str, slots: int, val_bins: int, val_criterion: str, params: Optional[torch.Tensor], dev):
        super().__init__(who, slots, val_bins, val_criterion, params, dev)
        self.logits = self.score_ws = None

    def operands(self, who: str, val_features: torch.Tensor, val_labels, E: int, C: int, prepare=_fp32):
        """``val_set``'s features and labels -- by default fp32 features whose rows are read with their stride -- and, made with them,
        the [N_val, C] fp32 logits and the scoring workspace."""
        feats, labels_d, made = self.val_set(who, val_features, val_labels, E, C, prepare)
        if made:
            N, dev = val_features.shape[0], val_features.device
            self.logits = torch.empty(N, C, dtype=torch.float32, device=dev)
            self.score_ws = torch.empty(max(lib.clipmi_val_score_workspace_bytes(N, self.bins), 256), dtype=torch.uint8, device=dev)
        return feats, labels_d

    def score(self, epoch: int, labels_d: torch.Tensor, params: Optional[torch.Tensor]) -> None:
        """``self.logits`` into record ``epoch`` and, when the monitor selects, ``params`` into the best slot under the decision; enqueued."""
        ops.val_score(self.logits, labels_d, self.bins, self.records[epoch], self.score_ws)
        self.select(epoch, params)


def _batch_size(who: str, val_batch_size) -> int:
    if isinstance(val_batch_size, bool) or int(val_batch_size) != val_batch_size or int(val_batch_size) < 1:
        raise ValueError(f"{who}: val_batch_size={val_batch_size} must be an integer >= 1")
    return int(val_batch_size)


class ImageMonitor(History):
    """``History`` for the fits that train through the image tower (``vptfit``, ``maplefit``, ``promptsrcfit``), whose validation set is
    images: the features change with the prompts, so every validation runs the tower over the set again, in chunks.  It holds the set -- a
    tensor [N_val, 3, R, R] on the GPU cut into chunks of ``val_batch_size``, or a sized iterable of (images, labels) batches on the GPU
    iterated once per validation --, the labels, the 16 N_val-byte row results (``ops.val_score_rows``) and, for the separate calls, the
    [B, C] logits of one chunk.  Its footprint does not depend on N_val x C: no [N_val, C] logits matrix exists at any time.
    ``ops.val_score_finish`` folds the row results into the record, byte for byte ``ops.val_score``'s on the whole matrix.
    ``cocoopfit``, whose classifier differs per image, keeps its row results here too and fills them from its own fused kernel."""

    def __init__(self, who: str, slots: int, val_bins: int, val_criterion: str, params: Optional[torch.Tensor], dev):
        super().__init__(who, slots, val_bins, val_criterion, params, dev)
        self.rows = self.finish_ws = self.chunk_logits = self.feats_n = None
        self.n_val = 0
        self.set = None

    def chunks(self, who: str, val_images_or_loader, val_labels, C: int, val_batch_size: int, dev):
        """The validation set as (images, labels int64 on the device) chunks.  Tensor form: views of ``val_batch_size`` images, the labels
        int64 on the device (an int64 tensor on the GPU is taken as it is; a host tensor is range-checked and uploaded once per set and
        again when its version moves; a list or an array carries no version, so it is checked and uploaded at every validation).  Loader
        form: the loader's own batches, ``val_labels`` None."""
        if not isinstance(val_images_or_loader, torch.Tensor):
            if val_labels is not None:
                raise ValueError(f"{who}: a loader of (images, labels) batches carries its labels: val_labels must be None")
            if not hasattr(val_images_or_loader, "__len__") or not hasattr(val_images_or_loader, "__iter__") or len(val_images_or_loader) < 1:
                raise ValueError(f"{who}: the validation set must be a tensor of images or a sized iterable of (images, labels) batches")
            return ((im, fitloop.step_labels(who, lab, im.shape[0], C, dev, "validation images")) for im, lab in val_images_or_loader)
        vi, bs = val_images_or_loader, _batch_size(who, val_batch_size)
        if vi.dim() != 4 or vi.shape[0] < 1:
            raise ValueError(f"{who}: val_images {tuple(vi.shape)} must be [N_val >= 1, 3, R, R]")
        fitloop._need_gpu(vi, "val_images")
        N = vi.shape[0]
        key = (vi.data_ptr(), tuple(vi.shape), id(val_labels), val_labels._version) if isinstance(val_labels, torch.Tensor) else None
        if key is None or self.set is None or self.set[0] != key:
            self.set = (key, fitloop.step_labels(who, val_labels, N, C, dev, "validation images"), val_labels)
        lab = self.set[1]
        return ((vi[lo:min(lo + bs, N)], lab[lo:min(lo + bs, N)]) for lo in range(0, N, bs))

    def room(self, rows: int, capacity: int, dev) -> torch.Tensor:
        """The row-result buffer with room for ``rows`` rows; it is made with ``capacity`` rows and grows (a copy on the device) beyond."""
        if self.rows is None or self.rows.shape[0] < rows:
            grown = ops.new_val_row_results(max(rows, capacity), dev)
            if self.rows is not None:
                grown[:self.rows.shape[0]].copy_(self.rows)
            self.rows = grown
        return self.rows

    def logits_for(self, B: int, C: int, E: int, dev):
        """The separate calls' operands of one chunk: normalised features [B, E] and logits [B, C]."""
        if self.chunk_logits is None or self.chunk_logits.shape[0] < B:
            self.chunk_logits = torch.empty(B, C, dtype=torch.float32, device=dev)
            self.feats_n = torch.empty(B, E, dtype=torch.float32, device=dev)
        return self.feats_n[:B], self.chunk_logits[:B]

    def validate(self, who: str, tower, prompts: torch.Tensor, text_n: torch.Tensor, scale: float, val_images_or_loader, val_labels, epoch,
                 val_batch_size: int, params: Optional[torch.Tensor], one_call: bool = True) -> None:
        """Enqueue one validation into slot ``epoch``: every chunk through ``tower.val_chunk`` (a ``vptfit._Tower``) at the fp32
        ``prompts`` against the normalised text features ``text_n`` [C, E], then the finish and, when the monitor selects, the selection of
        ``params``.  Nothing synchronises."""
        epoch = self.slot(who, epoch)
        Cn, dev = int(text_n.shape[0]), text_n.device
        row0 = 0
        loader = not isinstance(val_images_or_loader, torch.Tensor)
        for images, labels_d in self.chunks(who, val_images_or_loader, val_labels, Cn, val_batch_size, dev):
            images = tower.images(who, images)
            B = images.shape[0]
            capacity = B * len(val_images_or_loader) if loader else val_images_or_loader.shape[0]
            rows = self.room(row0 + B, capacity, dev)
            tower.val_chunk(self, images, prompts, text_n, scale, labels_d, self.bins, rows, row0, one_call)
            row0 += B
        if self.n_val and row0 != self.n_val and self.seen:
            raise ValueError(f"{who}: the validation set has {row0} rows, the history's earlier epochs {self.n_val}")
        self.n_val = row0
        need = lib.clipmi_val_score_finish_workspace_bytes(row0, self.bins)
        if self.finish_ws is None or self.finish_ws.numel() < need:
            self.finish_ws = torch.empty(max(need, 256), dtype=torch.uint8, device=dev)
        ops.val_score_finish(self.rows[:row0], self.bins, self.records[epoch], self.finish_ws)
        self.select(epoch, params)

    def row_results(self) -> torch.Tensor:
        """The row results of the last validation, uint8 [N_val, 16] on the device; no read-back."""
        if self.rows is None:
            raise ValueError("nothing has been validated")
        return self.rows[:self.n_val]


class Monitored:
    """The monitor surface of a ``*FitState``.  The state gives ``_who`` (its class name), ``_master()`` (its one contiguous fp32 master
    block on the GPU: what ``clipmi_best_select`` copies), ``_history`` (the history class ``start_monitor`` makes), its own ``validate``,
    which starts with ``self._monitor_for(epoch)``, and a named view of ``_best_block``.

    ``_unseen_summary``: what ``monitor()`` returns between ``start_monitor`` and the first ``validate``.  True (CoOp, CLIP-Adapter,
    TaskRes): the history's own summary -- no epochs, ``bins`` of the monitor's width, ``best_epoch`` -1 when it selects.  False (the
    other six): ``empty_monitor()`` -- 10 bins, ``best_epoch`` None."""

    _mon: Optional[History] = None
    _history = Monitor
    _unseen_summary = False

    def start_monitor(self, slots: int, val_bins: int = 10, select: bool = False, val_criterion: str = "accuracy") -> None:
        """The device history ``validate`` writes: ``slots`` epoch records of ``val_bins`` confidence bins and, with ``select``, the best
        block and the best slot -- a copy of the master block as it is now, replaced whenever a validated epoch is strictly better under
        ``val_criterion``.  The optimiser state, the scaler block and a GPA sum are not selected.  Allocations and one small upload;
        nothing synchronises."""
        master = self._master()
        self._mon = self._history(f"{self._who}.start_monitor", slots, val_bins, val_criterion, master if select else None, master.device)

    def _monitor_for(self, epoch) -> History:
        """The history, started with ``epoch + 1`` slots of 10 bins and no selection when ``start_monitor`` was not called."""
        if self._mon is None:
            self.start_monitor(int(epoch) + 1 if isinstance(epoch, int) and epoch >= 0 else 1)
        return self._mon

    def monitor(self) -> dict:
        """The history as numbers (``monitor_dict``); it reads the history back: one synchronisation."""
        if self._mon is None or not (self._mon.seen or self._unseen_summary):
            return empty_monitor()
        return self._mon.summary()

    def monitor_records(self) -> torch.Tensor:
        """The device history, uint8 [slots, ops.val_record_bytes(val_bins)]; no read-back."""
        if self._mon is None:
            raise ValueError(f"{self._who}.monitor_records: nothing has been validated")
        return self._mon.records

    def val_logits(self) -> torch.Tensor:
        """The fp32 [N_val, C] logits of the last ``validate``, where a ``Monitor`` keeps them (the next ``validate`` overwrites them)."""
        if getattr(self._mon, "logits", None) is None:
            raise ValueError(f"{self._who}.val_logits: nothing has been validated")
        return self._mon.logits

    def val_row_results(self) -> torch.Tensor:
        """The last validation's row results where an ``ImageMonitor`` keeps them, uint8 [N_val, 16] on the device
        (``ops.decode_val_row_results``); no read-back."""
        if getattr(self._mon, "rows", None) is None:
            raise ValueError(f"{self._who}.val_row_results: nothing has been validated")
        return self._mon.row_results()

    def _best_block(self, what: str) -> torch.Tensor:
        """The best slot on the device: the master block of the best epoch so far, or the one ``start_monitor`` saw while no epoch has
        been taken.  No read-back."""
        if self._mon is None or self._mon.best is None:
            raise ValueError(f"{self._who}.{what}: the monitor does not select (start_monitor(..., select=True))")
        return self._mon.best


class ImageMonitored(Monitored):
    """``Monitored`` for the three image-tower fit states, whose public ``start_monitor`` takes the criterion in front of ``select``."""

    _history = ImageMonitor

    def start_monitor(self, slots: int, val_bins: int = 10, val_criterion: str = "accuracy", select: bool = False) -> None:
        """``Monitored.start_monitor`` in the image states' argument order."""
        Monitored.start_monitor(self, slots, val_bins, select=select, val_criterion=val_criterion)
