"""Writes tests/golden/isotonic_cases.npz: what the reference's own MultiIsotonicRegression and BinMeanShift classes (float32, as
vl_calibrator.py runs them) give on a few seeded cases, and sklearn's float64 isotonic thresholds on the same float32 x, so that a
machine without the reference, scipy or sklearn still has both ground truths.  Arrays only.

Usage: python tools/gen_isotonic_golden.py <reference checkout> [out.npz]

The two reference modules are loaded from <reference checkout>/trainers/calibration by file path (nothing of them is copied).  Per
case `k` the file holds the inputs (val / test logits rounded to float16 values, labels, proximities, a DAC factor per class), the x
values numpy formed from them (the exact fit depends on every bit of x, and numpy's float32 exp need not be the same on every CPU),
the as-run outputs (`ref32_*`: fit_transform on val, transform on test without and with DAC, plain and Bin-Mean-Shift), `bin_edges`,
the float64 thresholds (`X64`, `y64`; `bms_X64_b`, `bms_y64_b` per bin) and `ref32_vs_ref64` = the (mean, max) absolute difference
between the as-run outputs and the float64 fit's over the test rows, plain and Bin-Mean-Shift.

A case must have the as-run reference and the float64 fit agree on the top-1 of every calibrated row; the generator walks the seeds
upwards from the case's first until one does, and records it."""
import importlib.util
import os
import sys
import types

import numpy as np
from scipy.special import softmax
from sklearn.isotonic import IsotonicRegression

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import isotonic_ref as ref  # noqa: E402

# name: (N_val, N_test, C, first seed, kind)
CASES = {
    "c50": (260, 240, 50, 100, "cosine"),     # the common shape, C below the wave size
    "c2": (200, 160, 2, 200, "cosine"),       # the reference's n_classes == 2 one-hot path
    "ties": (200, 160, 20, 300, "ties"),      # logits on a grid of 8 values: many exactly tied x
    "c131": (150, 120, 131, 400, "cosine"),   # C neither a multiple of 64 nor below it
}
BINS = 5


def load(path, name):
    for missing in ("pandas", "pdb"):   # imported by the module, unused by the two classes
        try:
            __import__(missing)
        except ImportError:
            sys.modules[missing] = types.ModuleType(missing)
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def make_inputs(n_val, n_test, C, seed, kind):
    """Cosine-like logits x 100 around a class prototype, rounded to float16 values; proximity higher where the row is cleaner."""
    rng = np.random.default_rng(seed)

    def split(n):
        labels = rng.integers(0, C, n)
        noise = rng.uniform(0.6, 1.6, n)
        cos = rng.normal(0.2, 0.035, (n, C)) * noise[:, None]
        cos[np.arange(n), labels] += rng.normal(0.07, 0.05, n)
        lg = cos * 100.0
        if kind == "ties":
            lg = np.round(lg / 4.0) * 4.0
            lg = np.clip(lg, 8.0, 36.0)
        prox = np.exp(-(0.5 + 0.25 * noise + rng.normal(0, 0.05, n))).astype(np.float32)
        return lg.astype(np.float16).astype(np.float32), labels.astype(np.int64), prox

    v, t = split(n_val), split(n_test)
    dac = rng.uniform(0.55, 1.0, C).astype(np.float32)
    return v, t, dac


def dac_scale(logits, dac):
    """distanse_aware_calibration.py:49-58 in float32."""
    return logits * dac[logits.argmax(axis=1)][:, None]


def sk64(x, labels):
    ir = IsotonicRegression(out_of_bounds="clip").fit(x.astype(np.float64).ravel(), ref.onehot(labels, x.shape[1]).ravel())
    return ir.X_thresholds_.astype(np.float64), ir.y_thresholds_.astype(np.float64)


def build_case(mir, mpi, n_val, n_test, C, seed, kind):
    (vl, vy, vp), (tl, ty, tp), dac = make_inputs(n_val, n_test, C, seed, kind)
    p_val = softmax(vl, axis=1)                       # vl_calibrator.py:60
    p_test = {"": softmax(tl, axis=-1), "_dac": softmax(dac_scale(tl, dac), axis=-1)}
    out = {"val_logits": vl, "val_labels": vy, "val_prox": vp, "test_logits": tl, "test_labels": ty, "test_prox": tp, "dac": dac,
           "seed": np.int64(seed), "x_val": ref.second_softmax(p_val)}
    for s, p in p_test.items():
        out["x_test" + s] = ref.second_softmax(p)
    assert out["x_val"].dtype == np.float32
    plain = mir.MultiIsotonicRegression()
    out["ref32_plain_val"] = plain.fit_transform(p_val, vy)
    bms = mpi.BinMeanShift("multi_isotonic_regression", mir.MultiIsotonicRegression, bin_strategy="quantile", normalize_conf=False,
                           proximity_bin=BINS)
    out["ref32_bms_val"] = bms.fit_transform(p_val, vp, vy)
    out["bin_edges"] = np.asarray(bms.bin_edges)
    for s, p in p_test.items():
        out["ref32_plain_test" + s] = plain.transform(p)
        out["ref32_bms_test" + s] = bms.transform(p, tp)
    # the float64 fit on the same float32 x
    out["X64"], out["y64"] = sk64(out["x_val"], vy)
    no = ref.bin_index(out["bin_edges"], vp)
    tables = []
    for b in range(BINS):
        X, Y = sk64(out["x_val"][no == b], vy[no == b])
        out[f"bms_X64_{b}"], out[f"bms_y64_{b}"] = X, Y
        tables.append((X, Y))
    ok, diffs = True, {"plain": [], "bms": []}
    for s in ("val", "test", "test_dac"):
        x = out["x_" + s]
        prox = vp if s == "val" else tp
        for name, r64 in (("plain", ref.calibrate(out["X64"], out["y64"], x)),
                          ("bms", ref.calibrate_bins(out["bin_edges"], tables, x, prox))):
            r32 = np.asarray(out[f"ref32_{name}_{s}"])
            ok &= bool(np.array_equal(r32.argmax(axis=1), r64.argmax(axis=1)))
            if s != "val":
                diffs[name].append(np.abs(r32.astype(np.float64) - r64.astype(np.float64)).ravel())
    for k in [k for k in out if k.startswith("ref32_")]:
        out[k] = np.asarray(out[k], np.float32)
    d = {n: np.concatenate(v) for n, v in diffs.items()}
    out["ref32_vs_ref64_mean"] = np.array([d["plain"].mean(), d["bms"].mean()])
    out["ref32_vs_ref64_max"] = np.array([d["plain"].max(), d["bms"].max()])
    return ok, out


def main(reference, path):
    cal = os.path.join(reference, "trainers", "calibration")
    mir = load(os.path.join(cal, "multi_isotonic_regression.py"), "ref_multi_isotonic_regression")
    mpi = load(os.path.join(cal, "multi_proximity_isotonic.py"), "ref_multi_proximity_isotonic")
    out = {"cases": np.array(sorted(CASES))}
    for name, (n_val, n_test, C, seed, kind) in CASES.items():
        for s in range(seed, seed + 50):
            ok, case = build_case(mir, mpi, n_val, n_test, C, s, kind)
            if ok:
                break
        else:
            raise SystemExit(f"{name}: no seed in {seed}..{seed + 49} has the float32 and float64 fits agree on every top-1")
        print(f"{name}: seed {s}, thresholds {case['X64'].size} (float64), ref32 vs ref64 mean {case['ref32_vs_ref64_mean']}, "
              f"max {case['ref32_vs_ref64_max']}")
        out.update({f"{name}_{k}": v for k, v in case.items()})
    np.savez_compressed(path, **out)
    print(f"wrote {path} ({os.path.getsize(path)} bytes, {len(CASES)} cases)")


if __name__ == "__main__":
    if len(sys.argv) < 2:
        raise SystemExit(__doc__)
    main(sys.argv[1], sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "tests", "golden", "isotonic_cases.npz"))
