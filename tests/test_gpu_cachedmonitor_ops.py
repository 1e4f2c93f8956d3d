"""The validation logits of the CLIP-Adapter and TaskRes fits on the GPU (clipmi_adapter_val_logits, clipmi_taskres_val_logits through
ops) at every seam of the kernels and of clipmi_val_score's 64-row workgroups: held element-wise against float64 on the device's own
inputs under the bound tests/cachedmonitor_ref.py derives (tests/cached_fit_ref.py's derivation for these fits' training forward), with a
NaN-prefilled output, canaries around the exact buffer and two runs compared bit for bit; the shared-forward contract against the fits' own
steps; and non-finite rows."""
import math

import numpy as np
import pytest
import torch

import cachedmonitor_ref as ref
import fitmonitor_ref
import head_ref

pytestmark = pytest.mark.gpu

from clip_calibration_amd import ops  # noqa: E402
from clip_calibration_amd.adapterfit import AdapterFitState  # noqa: E402
from clip_calibration_amd.taskresfit import TaskResFitState  # noqa: E402

S = 100.0
CANARY = 12345.0
PAD = 64               # floats: the view between the canaries stays 16-byte aligned
WIDTHS = [(128, 32), (512, 128)]
# C = 1000, past the 256-class seam the loss heads had, once per width with N_val 65
CASES = [(n, c) for c in (3, 257) for n in (1, 64, 65, 130)] + [(65, 1000)]
PARAMS = [(k, e, h, n, c) for k in ("adapter", "taskres") for e, h in WIDTHS for n, c in CASES]


def guarded_out(N, C):
    whole = torch.full((N * C + 2 * PAD,), CANARY, dtype=torch.float32, device="cuda")
    out = whole[PAD:PAD + N * C].view(N, C)
    out.fill_(float("nan"))
    return whole, out


def canaries_intact(whole, n):
    w = whole.cpu().numpy()
    return bool((w[:PAD] == CANARY).all() and (w[PAD + n:] == CANARY).all())


def run(kind, c, feats, out=None):
    """The device's logits of case ``c`` on the features ``feats`` (a GPU tensor)."""
    if kind == "adapter":
        return ops.adapter_val_logits(feats, torch.from_numpy(np.array(c["T"])).cuda(), torch.from_numpy(np.array(c["w1"])).cuda(),
                                      torch.from_numpy(np.array(c["w2"])).cuda(), ref.RATIO, S, out=out)
    return ops.taskres_val_logits(feats, torch.from_numpy(np.array(c["base"])).cuda(), torch.from_numpy(np.array(c["r"])).cuda(), ref.ALPHA, S, out=out)


def case_and_bound(kind, E, H, N, C):
    if kind == "adapter":
        c = ref.adapter_val_case(N, E, H, C)
        return c, ref.adapter_logits_bound(c["f"], c["T"], c["w1"], c["w2"], ref.RATIO, S)
    c = ref.taskres_val_case(N, E, C)
    return c, ref.taskres_logits_bound(c["f"], c["base"], c["r"], ref.ALPHA, S)


@pytest.mark.parametrize("kind,E,H,N,C", PARAMS, ids=["-".join(map(str, p)) for p in PARAMS])
def test_logits_within_the_bound_exact_buffer_same_bits(kind, E, H, N, C):
    c, (z, tz) = case_and_bound(kind, E, H, N, C)
    feats = torch.from_numpy(np.array(c["f"])).cuda()
    whole, out = guarded_out(N, C)
    got = run(kind, c, feats, out)
    torch.cuda.synchronize()
    assert got.data_ptr() == out.data_ptr() and canaries_intact(whole, N * C)
    first = out.cpu()
    assert torch.isfinite(first).all(), "an element of the NaN-prefilled output was not written"
    r = head_ref.ratio(first, z, tz)
    print(f"cachedmonitor-parity: {kind} E={E} H={H} N_val={N} C={C}: max error / bound {r:.3f}")
    assert r <= 1.0
    again = run(kind, c, feats).cpu()
    assert first.numpy().tobytes() == again.numpy().tobytes()


@pytest.mark.parametrize("kind", ["adapter", "taskres"])
def test_features_as_a_column_slice_of_a_wider_matrix(kind):
    E, H, N, C = 128, 32, 65, 257
    c, (z, tz) = case_and_bound(kind, E, H, N, C)
    wide = torch.full((N, E + 24), float("nan"), device="cuda")          # whatever lies outside [N_val, E] is never read into a sum
    wide[:, 8:8 + E] = torch.from_numpy(np.array(c["f"])).cuda()
    sliced = wide[:, 8:8 + E]
    assert sliced.stride(0) == E + 24 and not sliced.is_contiguous()
    got = run(kind, c, sliced).cpu()
    assert head_ref.ratio(got, z, tz) <= 1.0
    assert got.numpy().tobytes() == run(kind, c, sliced.contiguous()).cpu().numpy().tobytes()


@pytest.mark.parametrize("kind", ["adapter", "taskres"])
def test_a_non_finite_row_gives_a_non_finite_row_and_touches_no_other(kind):
    E, H, N, C = 128, 32, 130, 257
    c, _ = case_and_bound(kind, E, H, N, C)
    feats = torch.from_numpy(np.array(c["f"])).cuda()
    clean = run(kind, c, feats).cpu().numpy()
    bad = feats.clone()
    bad[1, 5], bad[64, 0], bad[129, E - 1] = float("nan"), float("inf"), float("-inf")
    got = run(kind, c, bad).cpu().numpy()
    rows = [1, 64, 129]
    assert not np.isfinite(got[rows]).any()
    keep = np.setdiff1d(np.arange(N), rows)
    assert got[keep].tobytes() == clean[keep].tobytes()
    # clipmi_val_score counts those rows as wrong and carries the NaN into nll_sum
    y = torch.from_numpy(np.array(c["y"])).cuda()
    rec = ops.decode_val_records(ops.val_score(torch.from_numpy(got).cuda(), y, 10), 10)[0]
    want = fitmonitor_ref.record(got, np.array(c["y"]), 10)
    assert rec["n"] == N and rec["correct"] == want["correct"] <= N - 3 and math.isnan(rec["nll_sum"])


@pytest.mark.parametrize("kind", ["adapter", "taskres"])
def test_validation_sees_the_logits_a_training_step_sees(kind):
    """The shared-forward contract.  Steps of one row at rate 0 (no weight decay, no momentum) leave the weights as they are and return the
    row's loss as the training kernels form it: xent_row's log(S) - (z_y - max) with S summed thread-strided over the workgroup and its waves'
    trees added in order, exp by __expf.  That is the row rule of tests/fitmonitor_ref.py on the step's own logits in another, documented
    summation order (DESIGN.md "Fit monitor"), so the step's loss is held to the float64 row rule ON THE VALIDATION LOGITS within
    head_ref._softmax_bound with a zero bound on the logits: the roundings of the loss alone.  A validation forward that differed from the
    step's in an operand or a term would be outside it by orders of magnitude."""
    E, H, N, C = 128, 32, 8, 257
    c, _ = case_and_bound(kind, E, H, N, C)
    feats, y = torch.from_numpy(np.array(c["f"])).cuda(), torch.from_numpy(np.array(c["y"])).cuda()
    if kind == "adapter":
        st = AdapterFitState(torch.from_numpy(np.array(c["T"])).cuda(), torch.from_numpy(np.array(c["w1"])), torch.from_numpy(np.array(c["w2"])),
                             ratio=ref.RATIO, logit_scale=math.log(S), momentum=0.0, weight_decay=0.0)
        before = (st.w1.clone(), st.w2.clone())
        nsum = head_ref.ceil_div(C, 1024) + 21
    else:
        st = TaskResFitState(torch.from_numpy(np.array(c["base"])).cuda(), torch.from_numpy(np.array(c["r"])), alpha=ref.ALPHA,
                             logit_scale=math.log(S), optimizer="sgd", momentum=0.0, weight_decay=0.0)
        before = (st.residuals.clone(),)
        nsum = None
    rate = torch.zeros(1, device="cuda")
    losses = torch.cat([st.step(feats[i:i + 1], y[i:i + 1], rate, want_loss=True) for i in range(N)]).cpu().double()
    after = (st.w1, st.w2) if kind == "adapter" else (st.residuals,)
    assert all(torch.equal(a, b) for a, b in zip(before, after))
    st.validate(feats, y, 0)
    z = st.val_logits().cpu().double()
    scale = st.scale
    assert scale == float(np.float32(math.exp(math.log(S))))
    _, _, _, _, rows, trows = head_ref._softmax_bound(z, torch.zeros_like(z), torch.from_numpy(np.array(c["y"])), 1.0, C, nsum=nsum)
    _, nll, _ = fitmonitor_ref.score_rows(st.val_logits().cpu().numpy(), np.array(c["y"]))
    assert np.allclose(rows.numpy(), nll, rtol=1e-12, atol=1e-12)
    r = head_ref.ratio(losses, rows, trows)
    print(f"cachedmonitor-parity: {kind} step loss against the row rule on the validation logits: max error / bound {r:.3f}, "
          f"max bound {float(trows.max()):.3e}")
    assert r <= 1.0
