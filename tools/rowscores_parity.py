"""Worst error over its derived bound of the row-score kernels on every seeded case of tests/rowscores_ref.py, next to the same ratio
for an fp32 emulation of the kernel's rounding points in numpy:  python tools/rowscores_parity.py [out.txt]  (a GPU is required).
profiles/rowscores_parity.txt is this tool's output."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import rowscores_ref as ref  # noqa: E402
from clip_calibration_amd import ops  # noqa: E402


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "rowscores_parity.txt")
    assert torch.cuda.is_available(), "rowscores_parity needs a GPU"
    lines = ["row scores: worst |device - float64| / bound (tests/rowscores_ref.py), and the same for numpy's fp32 at the kernel's rounding points",
             "N in %s, C in %s, n_bins in %s; exp and log held to 3 ulp" % (ref.NS, ref.CS, ref.BINS),
             "%-7s %-6s %-6s %10s %10s %10s %10s %10s %9s" % ("rows", "N", "C", "nll", "brier", "conf_sum", "emu nll", "emu brier", "excluded")]
    worst = {}
    for from_probs in (False, True):
        kind = "probs" if from_probs else "logits"
        for N in ref.NS:
            for C in ref.CS:
                rows_h, labels_h = ref.case_inputs(N, C, from_probs)
                rows, labels = torch.from_numpy(rows_h).cuda(), torch.from_numpy(labels_h).cuda()
                got = {"nll_ratio": 0.0, "brier_ratio": 0.0, "conf_ratio": 0.0, "excluded": 0}
                for n_bins in ref.BINS:
                    row_out, acc = ops.row_scores(rows, labels, from_probs=from_probs, n_bins=n_bins)
                    g = ref.compare_case(rows_h, labels_h, n_bins, from_probs, row_out.cpu().numpy(), acc.cpu().numpy())
                    got = {k: max(got[k], g[k]) for k in got}
                r = ref.reference(rows_h, labels_h, 10, from_probs)
                nll, brier, _ = ref.emulate_fp32(rows_h, labels_h, from_probs)
                en = float((np.abs(nll - r["nll"]) / ref.nll_bound(r["nll"], C, r["zmax"], from_probs)).max())
                eb = float((np.abs(brier - r["brier"]) / ref.brier_bound(r["p"], labels_h, C, r["zmax"], from_probs)).max())
                lines.append("%-7s %-6d %-6d %10.4f %10.4f %10.4f %10.4f %10.4f %9d" % (kind, N, C, got["nll_ratio"], got["brier_ratio"],
                                                                                  got["conf_ratio"], en, eb, got["excluded"]))
                for k, v in (("nll", got["nll_ratio"]), ("brier", got["brier_ratio"]), ("conf_sum", got["conf_ratio"]), ("emu nll", en), ("emu brier", eb)):
                    worst[(kind, k)] = max(worst.get((kind, k), 0.0), v)
    for kind in ("logits", "probs"):
        lines.append("worst %-6s " % kind + ", ".join("%s %.4f" % (k, worst[(kind, k)]) for k in ("nll", "brier", "conf_sum", "emu nll", "emu brier")))
    lines.append("counts and hits: equal to the restatement in every case; conf_sum of the probability rows: bit for bit")
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines[-4:]))


if __name__ == "__main__":
    main()
