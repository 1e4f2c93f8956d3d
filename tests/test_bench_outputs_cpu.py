"""bench.py's command-line surface: `--full` (everything beyond the headline) and `--dump-outputs DIR` (what the last timed step returned,
one .npy per array, float32 / float64, at most 64 MB).  The writer is checked here on host tensors shaped like fused_tail's outputs."""
import os
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_help_lists_full_and_dump_outputs():
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       text=True, timeout=120)
    assert p.returncode == 0, p.stdout
    assert "--full" in p.stdout and "--dump-outputs DIR" in p.stdout


def _last_step(B, C, E, seed=0):
    g = torch.Generator().manual_seed(seed)
    logits = torch.randn(B, C, generator=g)
    feats = torch.nn.functional.normalize(torch.randn(B, E, generator=g), dim=1)
    conf, pred = torch.softmax(logits, 1).max(1)
    return logits, feats, conf, pred.to(torch.int32)


def test_dump_outputs_writes_every_array(tmp_path):
    import bench
    last = _last_step(6, 10, 8)
    bins = np.arange(33, dtype=np.float64)
    bench.dump_outputs(str(tmp_path / "out"), last, bins, {"ece": 12.5, "accuracy": 50.0})
    got = {f[:-4]: np.load(tmp_path / "out" / f) for f in os.listdir(tmp_path / "out")}
    assert set(got) == {"logits", "image_features", "conf", "pred", "ece_bins", "ece_percent", "accuracy_percent"}
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    np.testing.assert_array_equal(got["logits"], last[0].numpy())
    np.testing.assert_array_equal(got["image_features"], last[1].numpy())
    np.testing.assert_array_equal(got["conf"], last[2].numpy())
    np.testing.assert_array_equal(got["pred"], last[3].numpy().astype(np.float64))
    np.testing.assert_array_equal(got["ece_bins"], bins)
    assert float(got["ece_percent"]) == 12.5 and float(got["accuracy_percent"]) == 50.0


def test_dump_outputs_samples_rows_above_the_limit(tmp_path, monkeypatch):
    import bench
    last = _last_step(512, 1000, 512)
    limit = 2 ** 20 + 512 * 1024
    monkeypatch.setattr(bench, "DUMP_OUTPUTS_MAX_BYTES", limit)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), last, np.zeros(33), {"ece": 0.0, "accuracy": 0.0})
    total = sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a"))
    assert total <= limit
    rows_a, rows_b = np.load(tmp_path / "a" / "rows.npy"), np.load(tmp_path / "b" / "rows.npy")
    np.testing.assert_array_equal(rows_a, rows_b)                                     # fixed, seeded sample
    rows = rows_a.astype(np.int64)
    assert 0 < rows.size < 512 and np.all(np.diff(rows) > 0)
    np.testing.assert_array_equal(np.load(tmp_path / "a" / "logits.npy"), last[0].numpy()[rows])
    np.testing.assert_array_equal(np.load(tmp_path / "a" / "pred.npy"), last[3].numpy()[rows].astype(np.float64))
