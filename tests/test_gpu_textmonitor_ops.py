"""The two new validation kernels at operator level.

clipmi_cocoop_val_rows (the per-pair tail fused into the row score) against clipmi_val_score_rows on the logits of
``ops.logits_per_image``, byte for byte: C of 1, 5, 63, 64, 65 and 1000, chunks of 1 and 3 images, E = 128, one row with a label outside
[0, C) and one row whose image feature holds a NaN.

clipmi_proda_val_mean (normalise and average a class's P text features) against float64 for P of 1, 2, 6 and 32 with 3 classes, and byte
for byte against the two calls it fuses (``group_mean(l2_normalize(.))``).

The bound (tests/textmonitor_ref.py ``mean_bound``), with u = 2^-24 (a rounding to nearest errs by at most u relative) and m = max_p
|u_{p,e}| over a class's unit rows: a unit row's element carries (E / 2 + 3) u relative from its norm (E u on the sum of squares, halved
by the root), the root, the reciprocal and the product.  The P elements are added one by one from zero: the k-th partial sum is at most
k m and its rounding errs by at most u k m, so the P roundings of the accumulation err by at most u m P (P + 1) / 2 together, which the
division by P turns into u m (P + 1) / 2; the division itself rounds once more, u m.  Together at most ((P + 1) / 2 + 1) u m <= (P + 1) u m
for every P >= 1 -- the P fp32 roundings of the accumulation -- beside the rows' own (E / 2 + 3) u m."""
import numpy as np
import pytest
import torch

import textmonitor_ref as tref

pytestmark = pytest.mark.gpu

from clip_calibration_amd import ops  # noqa: E402

E = 128


@pytest.mark.parametrize("Bv", [1, 3])
@pytest.mark.parametrize("C", [1, 5, 63, 64, 65, 1000])
def test_cocoop_val_rows_equals_the_score_of_the_per_image_logits(C, Bv):
    g = torch.Generator().manual_seed(1000 * C + Bv)
    img = torch.randn(Bv, E, generator=g)
    img = (img / img.norm(dim=1, keepdim=True)).cuda()
    base = torch.randn(1, C, E, generator=g)
    txt = ((base + 0.5 * torch.randn(Bv, C, E, generator=g)) * 0.3).cuda()
    labels = torch.randint(0, C, (Bv,), generator=g)
    labels[0] = C                                # outside [0, C): never an address, the row counts as wrong with a NaN nll
    if Bv > 1:
        img[1, 7] = float("nan")                 # a NaN feature: every logit of the row is a NaN
    labels = labels.cuda()
    scale = 31.5
    logits = ops.logits_per_image(img, txt, scale, want_conf_pred=False, want_last_text=False)[0]
    want = ops.val_score_rows(logits, labels, 10).cpu().numpy()
    rows = ops.new_val_row_results(Bv + 2, "cuda")
    got = ops.cocoop_val_rows(img, txt, scale, labels, 10, rows, 1).cpu().numpy()
    assert np.array_equal(got[1:1 + Bv], want), "the fused rows differ from val_score_rows on logits_per_image's logits"
    assert not got[0].any() and not got[-1].any(), "a row result outside the chunk was written"
    dec = ops.decode_val_row_results(got[1:1 + Bv])
    assert dec["hit"][0] == 0 and np.isnan(dec["nll"][0]) and (C == 1 or np.isfinite(dec["conf"][0]))
    if Bv > 1:
        assert dec["hit"][1] == 0 and np.isnan(dec["nll"][1]) and np.isnan(dec["conf"][1]) and dec["bin"][1] == 10
    again = ops.cocoop_val_rows(img, txt, scale, labels, 10).cpu().numpy()
    assert np.array_equal(again, want), "two runs differ"


@pytest.mark.parametrize("P", [1, 2, 6, 32])
def test_proda_val_mean_against_float64_and_the_two_calls_it_fuses(P):
    Cn = 3
    g = torch.Generator().manual_seed(50 + P)
    centre = torch.randn(Cn, 1, E, generator=g)
    text = ((centre + 0.4 * torch.randn(Cn, P, E, generator=g)) * (0.1 + 5.0 * torch.rand(Cn, P, 1, generator=g))).reshape(Cn * P, E)
    got = ops.proda_val_mean(text.cuda(), P)
    two = ops.group_mean(ops.l2_normalize(text.cuda()), P)
    assert torch.equal(got.view(torch.int32), two.view(torch.int32)), "not the bits of group_mean(l2_normalize(.))"
    want, bound = tref.proda_mean(text.numpy(), P), tref.mean_bound(text.numpy(), P)
    err = np.abs(got.cpu().numpy().astype(np.float64) - want)
    print(f"textmonitor-parity: proda_val_mean P={P}: max error {err.max():.3e}, worst ratio to the bound {(err / bound).max():.3f}")
    assert (err <= bound).all()
    assert torch.equal(ops.proda_val_mean(text.cuda(), P), got), "two runs differ"
