"""GPU checks of clipmi_augment (csrc/augment.hip) through clip_calibration_amd.augment: the resized bytes of every view equal the numpy
restatement of Pillow's crop -> resize -> flip (tests/augment_ref.py) exactly, the normalised output is the table lookup of those bytes
bit for bit, a flip is a mirrored store, a whole-image view of a square image is Preprocess of it, every input form gives the same bits,
and fit_adapter / fit_residuals with a transform leave the weights of a hand-written loop over the same views."""
import math

import numpy as np
import pytest
import torch

import augment_ref as ref
from clip_calibration_amd import synthetic as syn
from clip_calibration_amd.adapterfit import AdapterFitState
from clip_calibration_amd.augment import TrainPreprocess, sample_views
from clip_calibration_amd.model import build_model
from clip_calibration_amd.preprocess import Preprocess, normalize_table, pack_images
from clip_calibration_amd.runner import device_batches
from clip_calibration_amd.taskresfit import TaskResFitState
from clip_calibration_amd.trainers import CLIPAdapterCLIP, TaskResCLIP

pytestmark = pytest.mark.gpu

_WANT = {}


def want_bytes(n_px, filt):
    """uint8 [V, n_px, n_px, 3] of the case list, computed once per (n_px, filter) and shared."""
    if (n_px, filt) not in _WANT:
        images, views = ref.cases(n_px)
        _WANT[n_px, filt] = np.stack([ref.view(images[b], (t, l, h, w), n_px, filt, f) for b, t, l, h, w, f in views])
    return _WANT[n_px, filt]


def _bytes(out):
    """identity-table output -> uint8 [V, n_px, n_px, 3] (asserting that every value is an exact byte)"""
    o = out.cpu()
    assert torch.equal(o, o.round()) and o.min() >= 0 and o.max() <= 255
    return o.to(torch.uint8).permute(0, 2, 3, 1).numpy()


@pytest.mark.parametrize("filt", ["bicubic", "bilinear"])
@pytest.mark.parametrize("n_px", ref.N_PX)
def test_view_bytes_exact(n_px, filt):
    images, views = ref.cases(n_px)
    tp = TrainPreprocess(n_px, interpolation=filt, dtype=torch.float32, normalize=False)
    got = _bytes(tp(images, np.asarray(views)))
    want = want_bytes(n_px, filt)
    for i, v in enumerate(views):
        assert np.array_equal(got[i], want[i]), f"view {v} -> {n_px} {filt}: max |d| {np.abs(got[i].astype(int) - want[i]).max()}"


@pytest.mark.parametrize("n_px", ref.N_PX)
def test_normalised_output_is_the_table_lookup(n_px):
    images, views = ref.cases(n_px)
    u8 = torch.from_numpy(want_bytes(n_px, "bicubic")).permute(0, 3, 1, 2).long()                 # [V, 3, n, n]
    want = torch.stack([normalize_table()[c][u8[:, c]] for c in range(3)], dim=1)
    got32 = TrainPreprocess(n_px, dtype=torch.float32)(images, np.asarray(views)).cpu()
    assert torch.equal(got32.view(torch.int32), want.view(torch.int32))
    got16 = TrainPreprocess(n_px)(images, np.asarray(views)).cpu()
    assert got16.dtype == torch.float16 and torch.equal(got16.view(torch.int16), want.half().view(torch.int16))


@pytest.mark.parametrize("n_px", ref.N_PX)
def test_flip_is_a_mirrored_store(n_px):
    images, views = ref.cases(n_px)
    v = np.asarray(views)
    plain, flipped = v.copy(), v.copy()
    plain[:, 5], flipped[:, 5] = 0, 1
    for dtype in (torch.float16, torch.float32):
        tp = TrainPreprocess(n_px, dtype=dtype)
        a, b = tp(images, plain), tp(images, flipped)
        assert torch.equal(torch.flip(a, dims=[3]), b) and not torch.equal(a, b)


@pytest.mark.parametrize("filt", ["bicubic", "bilinear"])
def test_whole_square_image_equals_preprocess(filt):
    """Resize on the shorter side + CenterCrop of a square image is a stretch of the whole image."""
    for n_px in ref.N_PX:
        imgs = [ref.synthetic_image(s, s, 10 + s) for s in (1, 7, n_px, 50, 131)] + [ref.checkerboard(33, 33, 2)]
        views = [(i, 0, 0, im.shape[0], im.shape[1], 0) for i, im in enumerate(imgs)]
        for dtype in (torch.float16, torch.float32):
            a = TrainPreprocess(n_px, interpolation=filt, dtype=dtype)(imgs, np.asarray(views))
            assert torch.equal(a, Preprocess(n_px, interpolation=filt, dtype=dtype)(imgs))


def test_input_forms_agree():
    B, H, W = 3, 45, 61
    hwc = np.stack([ref.synthetic_image(H, W, 20 + i) for i in range(B)])
    views = sample_views([(H, W)] * B, generator=torch.Generator().manual_seed(5), views_per_image=2)
    tp = TrainPreprocess(20)
    base = tp(list(hwc), views)                                                # host list
    assert base.shape == (2 * B, 3, 20, 20)
    dense = torch.from_numpy(hwc).cuda()
    same = lambda x: torch.equal(x.view(torch.int16), base.view(torch.int16))
    assert same(tp(dense, views))                                              # [B, H, W, 3] CUDA
    assert same(tp(torch.from_numpy(hwc), np.stack(views, axis=1)))            # host dense, views as one [V, 6] array
    assert same(tp(dense.permute(0, 3, 1, 2).contiguous(), views))             # [B, 3, H, W] CUDA
    assert same(tp([dense[i] for i in range(B)], views))                       # device list
    assert same(tp(pack_images(list(hwc)), views))                             # PackedImages, pageable
    assert same(tp(pack_images(list(hwc)).pin_memory(), views))                # PackedImages, pinned
    big = torch.zeros(B, H + 10, W + 20, 4, dtype=torch.uint8)                 # a strided crop view of a wider RGBA-like buffer
    big[:, 5:5 + H, 7:7 + W, :3] = torch.from_numpy(hwc)
    view = big.cuda()[:, 5:5 + H, 7:7 + W, :3]
    assert not view.is_contiguous() and same(tp(view, views))
    want = np.stack([ref.view(hwc[b], (t, l, h, w), 20, "bicubic", f) for b, t, l, h, w, f in np.stack(views, axis=1)])
    got = _bytes(TrainPreprocess(20, dtype=torch.float32, normalize=False)(dense, views))
    assert np.array_equal(got, want)


def test_repeated_images_each_view_alone_and_two_calls():
    """V > B with images repeated: every view has the bits it has in a call of its own, and a second call gives the same bits."""
    images, views = ref.cases(20)
    v = np.asarray(views + views[::-1])                                         # V = 38 views of B = 4 images
    tp = TrainPreprocess(20)
    first, second = tp(images, v), tp(images, v)
    assert first.shape[0] == 38 and torch.equal(first, second)
    for i in (0, 5, 13, 17, 20, 37):
        alone = tp([images[v[i, 0]]], np.asarray([[0] + v[i, 1:].tolist()]))
        assert torch.equal(alone[0], first[i]), i


def test_sampled_call_uses_the_generator():
    imgs = [ref.synthetic_image(h, w, i) for i, (h, w) in enumerate([(64, 80), (90, 70), (33, 47)])]
    tp = TrainPreprocess(20, generator=torch.Generator().manual_seed(8))
    got = tp(imgs)
    views = sample_views([i.shape[:2] for i in imgs], generator=torch.Generator().manual_seed(8))
    assert got.shape == (3, 3, 20, 20) and torch.equal(got, tp(imgs, views))
    with pytest.raises(Exception, match="outside"):
        tp(imgs, [[0, 0, 0, 65, 80, 0]])
    with pytest.raises(ValueError):
        tp(imgs, np.zeros((0, 6), np.int32))


def test_device_batches_train_preprocess():
    sizes = [[(75, 100), (64, 64), (20, 90)], [(100, 75), (33, 33)], [(28, 40)] * 4]
    mk = lambda s, j: [ref.synthetic_image(h, w, 40 + j + i) for i, (h, w) in enumerate(s)]
    batches = [(pack_images(mk(s, j)).pin_memory(), torch.arange(len(s))) for j, s in enumerate(sizes)]
    dense = (torch.from_numpy(np.stack(mk([(50, 70)] * 2, 9))), torch.tensor([7, 8]))
    loader = batches + [dense]
    got = list(device_batches(loader, preprocess=TrainPreprocess(20, generator=torch.Generator().manual_seed(2))))
    tp = TrainPreprocess(20, generator=torch.Generator().manual_seed(2))         # the same draws, batch by batch
    assert len(got) == len(loader)
    for (img, lab), (src, src_lab) in zip(got, loader):
        assert img.is_cuda and img.dtype == torch.float16 and lab.is_cuda
        assert torch.equal(img, tp(src)) and torch.equal(lab.cpu(), src_lab)


# ---- training under the transform ------------------------------------------------------------------------------------------------------

def _train_loader():
    """Two batches of four ragged decoded images with host labels, for the tiny model (n_px = 64, 5 classes)."""
    sizes = [(80, 100), (64, 64), (70, 51), (120, 90), (66, 97), (100, 100), (45, 80), (90, 64)]
    imgs = [ref.synthetic_image(h, w, 70 + i) for i, (h, w) in enumerate(sizes)]
    labels = torch.arange(8) % 5
    return [(pack_images(imgs[i:i + 4]).pin_memory(), labels[i:i + 4]) for i in (0, 4)]


def _tiny():
    return build_model(dict(syn.synthetic_state_dict("tiny", seed=0)), {"trainer": "CoOp"}).cuda()


def test_fit_adapter_with_a_transform_equals_the_hand_written_loop():
    model, loader = _tiny(), _train_loader()
    ids = syn.synthetic_token_ids(5, "tiny", seed=90, n_ctx_placeholders=4)
    torch.manual_seed(0)
    ad = CLIPAdapterCLIP(model, ids, n_ctx=4, ratio=0.2, seed=6)
    before = [ad.adapter.fc[i].weight.detach().clone() for i in (0, 2)]
    rates = [0.002, 0.001]
    # the oracle: transform -> image_features_f32 -> AdapterFitState.step, over the views the seed gives
    tp = TrainPreprocess.for_model(model, generator=torch.Generator().manual_seed(21))
    assert tp.n_px == 64 and tp.dtype == model.dtype
    with torch.no_grad():
        st = AdapterFitState(ad.text_features(), before[0].float(), before[1].float(), ratio=0.2, logit_scale=math.log(ad.scale))
        want_losses = []
        for e in range(2):
            for images, labels in loader:
                want_losses.append(st.step(model.image_features_f32(tp(images)), labels, rates[e], want_loss=True))
    tp2 = TrainPreprocess.for_model(model, generator=torch.Generator().manual_seed(21))
    w1, w2, losses = ad.fit_adapter(loader, transform=tp2, epochs=2, lr_per_epoch=rates, return_history=True)
    assert torch.equal(w1, st.w1) and torch.equal(w2, st.w2) and np.array_equal(losses, torch.cat(want_losses).cpu().numpy())
    assert losses.shape == (4,) and np.isfinite(losses).all() and not torch.equal(w1, before[0].float())
    for i, fitted in ((0, w1), (2, w2)):
        w = ad.adapter.fc[i].weight
        assert w.dtype == model.dtype and torch.equal(w, fitted.to(w.dtype))
    # explicit views reach the kernels: whole-image, unflipped views give other weights than the sampled ones, the same on every run
    whole = lambda e, k, shapes: np.stack([np.arange(len(shapes)), 0 * shapes[:, 0], 0 * shapes[:, 0], shapes[:, 0], shapes[:, 1], 0 * shapes[:, 0]], axis=1)
    runs = []
    for _ in range(2):
        with torch.no_grad():
            ad.adapter.fc[0].weight.copy_(before[0])
            ad.adapter.fc[2].weight.copy_(before[1])
        runs.append(ad.fit_adapter(loader, transform=tp2, epochs=2, lr_per_epoch=rates, views=whole))
    assert len(runs[0]) == 2 and torch.equal(runs[0][0], runs[1][0]) and not torch.equal(runs[0][0], w1)


def test_fit_residuals_with_a_transform_equals_the_hand_written_loop():
    model, loader = _tiny(), _train_loader()
    ids = torch.stack([syn.synthetic_token_ids(5, "tiny", seed=90 + i) for i in range(3)], dim=1)      # [C, T, 77]
    tr = TaskResCLIP(model, ids, alpha=0.5)
    res = tr.prompt_learner.text_feature_residuals
    rates = [2e-3, 1e-3]
    tp = TrainPreprocess.for_model(model, generator=torch.Generator().manual_seed(22))
    with torch.no_grad():
        st = TaskResFitState(tr.prompt_learner.base_text_features.float(), None, alpha=0.5, logit_scale=math.log(tr.scale))
        want_losses = []
        for e in range(2):
            for images, labels in loader:
                want_losses.append(st.step(model.image_features_f32(tp(images)), labels, rates[e], want_loss=True))
    tp2 = TrainPreprocess.for_model(model, generator=torch.Generator().manual_seed(22))
    fitted, losses = tr.fit_residuals(loader, transform=tp2, epochs=2, lr_per_epoch=rates, return_history=True)
    assert torch.equal(fitted, st.residuals) and np.array_equal(losses, torch.cat(want_losses).cpu().numpy())
    assert fitted.dtype == torch.float32 and fitted.any() and torch.equal(res.detach(), fitted.to(res.dtype))
    with pytest.raises(ValueError, match="classes"):
        tr.fit_residuals([(loader[0][0], torch.tensor([0, 1, 2, 5]))], transform=tp2, epochs=1)
    with pytest.raises(TypeError, match="length"):
        tr.fit_residuals(iter(loader), transform=tp2, epochs=1)
