"""Device-side stand-in for VLClassification.process/evaluate and VLCalibration.predict on the ECE branch
(reference evaluators/vl_evaluator.py:40-51,59-102; trainers/calibration/vl_calibrator.py:83-109) -- SURVEY f-1.

The reference copies logits, labels and both feature matrices to python lists every batch (3 D2H syncs + ``tolist()``);
here (conf, pred) come out of the logits kernel and only 3*(n_bins+1) float64 accumulators live on the device until
``evaluate``.  With ``keep_samples=True`` the per-sample (conf, pred, label) vectors -- 16 B per sample -- are kept on
the device as well and copied to the host ONCE in ``evaluate`` for the metrics that need the samples themselves
(macro-F1, AdaptiveECE's equal-mass bins, PIECE's proximity bins).  With ``sample_metrics="device"`` those three come from kernels too
(csrc/sample_metrics.hip: per-class counts, order statistics by radix select, grouped gap sums) and only the selected order
statistics, the [3, G] group sums and the [3 C + 1] counts are copied -- nothing of O(N)."""
from __future__ import annotations

from collections import OrderedDict
from typing import List, Optional

import numpy as np
import torch

from . import ops
from .metrics import (AdaptiveECE, PIECE, classwise_from_bins, ece_from_bins, gap_from_groups, macro_f1, macro_f1_from_counts, mce_from_bins,
                      quantile_edges_from_order_stats, quantile_ranks)


class DeviceCalibrationEvaluator:
    def __init__(self, n_bins: int = 10, device="cuda", keep_samples: bool = False, piece_bins: int = 10,
                 sample_metrics: str = "host", n_classes: Optional[int] = None, proper_scores: bool = False):
        """``proper_scores``: accept whole rows through ``process_rows`` (csrc/row_scores.hip) and report their mean negative log-likelihood,
        mean Brier score and class-wise ECE behind the other keys; off by default, and then nothing changes.
        ``sample_metrics``: where macro-F1, ACE and PIECE are computed from the kept samples -- "host" (numpy, after one copy of the
        vectors) or "device" (kernels; needs ``keep_samples`` and ``n_classes``, the width of the logits the predictions index)."""
        if sample_metrics not in ("host", "device"):
            raise ValueError(f"sample_metrics={sample_metrics!r} (\"host\" or \"device\")")
        if sample_metrics == "device" and not (keep_samples and n_classes is not None and int(n_classes) >= 1):
            raise ValueError("sample_metrics=\"device\" needs keep_samples=True and n_classes >= 1")
        self.n_bins = n_bins
        self.piece_bins = piece_bins
        self.keep_samples = keep_samples
        self.sample_metrics = sample_metrics
        self.n_classes = None if n_classes is None else int(n_classes)
        self.bins = torch.zeros(3 * (n_bins + 1), dtype=torch.float64, device=device)
        self.proper_scores = bool(proper_scores)
        self._row_out: List[torch.Tensor] = []      # fp32 [rows, 2] = (nll, brier) per processed batch
        self._class_acc: Optional[torch.Tensor] = None   # int64 [3, C, n_bins + 1], ops.new_row_scores_acc
        self._conf: List[torch.Tensor] = []
        self._pred: List[torch.Tensor] = []
        self._gt: List[torch.Tensor] = []

    def reset(self):
        self.bins.zero_()
        self._conf, self._pred, self._gt = [], [], []
        self._row_out, self._class_acc = [], None

    def process_rows(self, rows: torch.Tensor, gt: torch.Tensor, from_probs: bool = False):
        """Score whole rows -- fp32 logits [B, C], or probabilities as given with ``from_probs`` (a calibrator's rows need not sum to 1) --
        against their labels: the rows' (nll, brier) stay on the device, the class-wise bins add up in one integer block."""
        if not self.proper_scores:
            raise RuntimeError("evaluator was built with proper_scores=False")
        gt = gt.to(rows.device, torch.int64)
        row_out, self._class_acc = ops.row_scores(rows, gt, from_probs=from_probs, n_bins=self.n_bins, acc=self._class_acc)
        self._row_out.append(row_out)

    def _append_proper_scores(self, res) -> None:
        """``nll`` and ``brier`` raw, ``cw_ece`` x 100, behind the keys that are there -- only when rows were processed."""
        rows = [r for r in self._row_out if r.shape[0]]
        if not rows or self._class_acc is None:
            return
        row_out = rows[0] if len(rows) == 1 else torch.cat(rows)
        if row_out.is_cuda:
            fin = ops.row_scores_finish(row_out.contiguous(), self._class_acc)
        else:   # blocks merged on the host (a CPU process group): the same arithmetic in numpy
            r = row_out.numpy().astype(np.float64)
            fin = {"nll": float(r[:, 0].mean()), "brier": float(r[:, 1].mean()),
                   "cw_ece": classwise_from_bins(self._class_acc.numpy(), r.shape[0])}
        res["nll"], res["brier"], res["cw_ece"] = fin["nll"], fin["brier"], 100.0 * fin["cw_ece"]

    def process(self, conf: torch.Tensor, pred: torch.Tensor, gt: torch.Tensor):
        gt = gt.to(conf.device, torch.int64)
        ops.ece_accumulate(conf, pred, gt, self.bins, self.n_bins)
        if self.keep_samples:
            self._conf.append(conf)
            self._pred.append(pred)
            self._gt.append(gt)

    def note_processed(self, conf: torch.Tensor, pred: torch.Tensor, gt: torch.Tensor):
        """The fused tail (ops.fused_tail with ``bins=self.bins``) has already added this batch to the bin accumulators;
        only the optional per-sample vectors are kept here."""
        if self.keep_samples:
            self._conf.append(conf)
            self._pred.append(pred)
            self._gt.append(gt.to(conf.device, torch.int64))

    def merge_from(self, other_bins: torch.Tensor):
        self.bins += other_bins.to(self.bins.device)

    def samples(self):
        """(conf f32, pred i64, gt i64) numpy vectors of everything processed so far: one D2H copy each."""
        if not self.keep_samples:
            raise RuntimeError("evaluator was built with keep_samples=False")
        if not self._conf:
            return np.zeros(0, np.float32), np.zeros(0, np.int64), np.zeros(0, np.int64)
        return (torch.cat(self._conf).cpu().numpy(), torch.cat(self._pred).cpu().numpy().astype(np.int64),
                torch.cat(self._gt).cpu().numpy())

    def _device_sample_metrics(self, proximity) -> "OrderedDict[str, float]":
        """macro_f1, ace and (with a proximity) piece as fractions, from the kept device vectors: every launch first, then the copies
        of the selected order statistics, then the two group launches whose edges the host derives from them."""
        if not self._conf:
            raise ValueError("sample_metrics=\"device\": no samples were processed")
        conf = torch.cat(self._conf).to(torch.float32)
        pred = torch.cat(self._pred).to(torch.int32)
        gt = torch.cat(self._gt).to(torch.int64)
        n = conf.shape[0]
        if proximity is not None:
            proximity = torch.as_tensor(proximity).to(device=conf.device, dtype=torch.float32)
            if proximity.dim() != 1 or proximity.shape[0] != n:
                raise ValueError(f"proximity has {tuple(proximity.shape)} entries for {n} samples")
        counts = ops.class_counts(pred, gt, self.n_classes)

        def select(x, n_bins):
            ranks = quantile_ranks(n, n_bins)
            distinct = np.unique(ranks)            # ascending, as the kernel wants them; at most 2 * (n_bins + 1)
            return ranks, distinct, ops.order_stats(x, distinct)

        def edges(selected, n_bins):
            ranks, distinct, (values, nans) = selected
            stats = values.cpu().numpy()[np.searchsorted(distinct, ranks)]
            return quantile_edges_from_order_stats(stats, n, n_bins, nan_count=int(nans.item()))

        sel_conf = select(conf, self.n_bins)
        sel_prox = select(proximity, self.piece_bins) if proximity is not None else None
        ace = ops.group_gap_accumulate(conf, pred, gt, key=conf, key_edges=edges(sel_conf, self.n_bins))
        piece = None
        if sel_prox is not None:
            piece = ops.group_gap_accumulate(conf, pred, gt, key=proximity, key_edges=edges(sel_prox, self.piece_bins),
                                             conf_edges=np.linspace(0, 1, self.n_bins + 1)[1:-1])
        counts = counts.cpu().numpy()
        if counts[-1]:
            raise ValueError(f"{int(counts[-1])} samples have a label or a prediction outside [0, {self.n_classes})")
        res = OrderedDict(macro_f1=macro_f1_from_counts(counts), ace=gap_from_groups(ace.cpu().numpy()))
        if piece is not None:
            res["piece"] = gap_from_groups(piece.cpu().numpy())
        return res

    def evaluate(self, proximity=None) -> "OrderedDict[str, float]":
        """Keys and scaling follow vl_evaluator.py:59-102 (percentages except ``confidence``).  ``macro_f1`` and ``ace``
        need keep_samples; ``piece`` additionally needs the per-sample proximity (base_learner.py:136-137): a numpy vector, or with
        ``sample_metrics="device"`` a device tensor that stays there."""
        if self.keep_samples and self.sample_metrics == "device":
            return self._evaluate_device(proximity)
        b = self.bins.cpu().numpy().reshape(3, self.n_bins + 1)
        total = b[0].sum()
        res = OrderedDict()
        res["accuracy"] = 100.0 * b[2].sum() / total
        res["error_rate"] = 100.0 - res["accuracy"]
        if self.keep_samples:
            conf, pred, gt = self.samples()
            res["macro_f1"] = 100.0 * macro_f1(pred, gt)
        res["confidence"] = b[1].sum() / total
        res["ece"] = 100.0 * ece_from_bins(b, self.n_bins)
        res["mce"] = 100.0 * mce_from_bins(b, self.n_bins)
        if self.keep_samples:
            res["ace"] = 100.0 * AdaptiveECE(conf, pred, gt, self.n_bins)
            if proximity is not None:
                proximity = np.asarray(proximity)
                if proximity.shape[0] != conf.shape[0]:
                    raise ValueError(f"proximity has {proximity.shape[0]} rows for {conf.shape[0]} samples")
                res["piece"] = 100.0 * PIECE(conf, proximity, pred, gt, self.piece_bins, self.n_bins)
        res["total"] = int(total)
        self._append_proper_scores(res)
        return res

    def _evaluate_device(self, proximity) -> "OrderedDict[str, float]":
        """``evaluate`` with the sample-level metrics from the device: the same keys in the same order with the same scaling."""
        sample = self._device_sample_metrics(proximity)
        b = self.bins.cpu().numpy().reshape(3, self.n_bins + 1)
        total = b[0].sum()
        res = OrderedDict()
        res["accuracy"] = 100.0 * b[2].sum() / total
        res["error_rate"] = 100.0 - res["accuracy"]
        res["macro_f1"] = 100.0 * sample["macro_f1"]
        res["confidence"] = b[1].sum() / total
        res["ece"] = 100.0 * ece_from_bins(b, self.n_bins)
        res["mce"] = 100.0 * mce_from_bins(b, self.n_bins)
        res["ace"] = 100.0 * sample["ace"]
        if "piece" in sample:
            res["piece"] = 100.0 * sample["piece"]
        res["total"] = int(total)
        self._append_proper_scores(res)
        return res
