"""GPU checks of clipmi_preprocess (csrc/preprocess.hip) through clip_calibration_amd.preprocess: the resized bytes equal the numpy
restatement of Pillow (tests/preprocess_ref.py) and the committed Pillow fixture exactly, the normalised output equals torchvision's
ToTensor -> Normalize (-> .half()) bit for bit, every input form gives the same bits, encode_image of the result equals encode_image of
the host-preprocessed batch, and the output does not depend on what runs beside it."""
import numpy as np
import pytest
import torch

import preprocess_ref as ref
from clip_calibration_amd import synthetic as syn
from clip_calibration_amd.model import build_model
from clip_calibration_amd.preprocess import CLIP_MEAN, CLIP_STD, Preprocess, pack_images
from clip_calibration_amd.runner import device_batches
from conftest import load_golden

pytestmark = pytest.mark.gpu

SWEEP = [(224, 224), (225, 300), (300, 225), (1, 50), (50, 1), (224, 2000), (3000, 225), (32, 32), (100, 224), (500, 375), (375, 500),
         (97, 130), (17, 23), (64, 64), (1, 1)]


def _images(sizes, seed=0):
    return [ref.checkerboard(h, w, 2) if i % 5 == 4 else ref.synthetic_image(h, w, seed + i) for i, (h, w) in enumerate(sizes)]


def _host_reference(imgs, n_px, filt="bicubic", mean=CLIP_MEAN, std=CLIP_STD):
    """torchvision's ToTensor -> Normalize on torch CPU fp32, of the restated Pillow output: [B, 3, n_px, n_px] fp32."""
    out = []
    for img in imgs:
        u8 = torch.from_numpy(ref.resize_crop(img, n_px, filt)).permute(2, 0, 1).contiguous()
        x = u8.to(torch.float32).div(255)
        out.append(x.sub_(torch.tensor(mean)[:, None, None]).div_(torch.tensor(std)[:, None, None]))
    return torch.stack(out)


def _bytes(out):
    """identity-table output -> uint8 [B, n_px, n_px, 3] (asserting that every value is an exact byte)"""
    o = out.cpu()
    assert torch.equal(o, o.round()) and o.min() >= 0 and o.max() <= 255
    return o.to(torch.uint8).permute(0, 2, 3, 1).numpy()


@pytest.mark.parametrize("filt", ["bicubic", "bilinear"])
def test_ragged_batch_bytes_exact(filt):
    imgs = _images(SWEEP)
    for n_px in (64, 224):
        pp = Preprocess(n_px, interpolation=filt, dtype=torch.float32, normalize=False)
        got = _bytes(pp(imgs))
        for i, img in enumerate(imgs):
            want = ref.resize_crop(img, n_px, filt)
            assert np.array_equal(got[i], want), f"{img.shape} -> {n_px} {filt}: max |d| {np.abs(got[i].astype(int) - want).max()}"
        if filt == "bicubic" and n_px == 64:          # one image per call gives the same bytes
            for i in (0, 3, 5, 9):
                assert np.array_equal(_bytes(pp([imgs[i]]))[0], got[i])


def test_fixture_bytes_exact():
    g = load_golden("preprocess_cases.npz")
    for i in range(len([k for k in g if k.startswith("meta")])):
        h, w, n_px, f, checker = (int(v) for v in g[f"meta{i}"])
        img = ref.checkerboard(h, w, 2) if checker else ref.synthetic_image(h, w, i)
        pp = Preprocess(n_px, interpolation="bicubic" if f == 3 else "bilinear", dtype=torch.float32, normalize=False)
        assert np.array_equal(_bytes(pp([torch.from_numpy(img).cuda()]))[0], g[f"out{i}"]), f"case {i}"


@pytest.mark.parametrize("n_px", [224, 336])
def test_normalised_output_bitwise(n_px):
    imgs = _images([(375, 500), (500, 375), (n_px, n_px), (300, 1000), (40, 60)], seed=7)
    want = _host_reference(imgs, n_px)
    got32 = Preprocess(n_px, dtype=torch.float32)(imgs).cpu()
    assert torch.equal(got32.view(torch.int32), want.view(torch.int32))
    got16 = Preprocess(n_px)(imgs).cpu()
    assert got16.dtype == torch.float16 and torch.equal(got16.view(torch.int16), want.half().view(torch.int16))


def test_input_forms_agree():
    B, H, W = 3, 150, 211
    hwc = np.stack([ref.synthetic_image(H, W, 20 + i) for i in range(B)])
    pp = Preprocess(64)
    base = pp(list(hwc))                                                   # host list
    dense = torch.from_numpy(hwc).cuda()
    same = lambda x: torch.equal(x.view(torch.int16), base.view(torch.int16))
    assert same(pp(dense))                                                 # [B, H, W, 3] CUDA
    assert same(pp(dense.permute(0, 3, 1, 2).contiguous()))                # [B, 3, H, W] CUDA
    assert same(pp([dense[i] for i in range(B)]))                          # device list
    assert same(pp(pack_images(list(hwc))))                                # PackedImages, pageable
    assert same(pp(pack_images(list(hwc)).pin_memory()))                   # PackedImages, pinned
    assert same(pp(pack_images(list(hwc)).cuda()))                         # PackedImages on the device
    big = torch.zeros(B, H + 10, W + 20, 4, dtype=torch.uint8)             # a strided crop view of a wider RGBA-like buffer
    big[:, 5:5 + H, 7:7 + W, :3] = torch.from_numpy(hwc)
    view = big.cuda()[:, 5:5 + H, 7:7 + W, :3]
    assert not view.is_contiguous() and same(pp(view))
    chw_view = big.cuda().permute(0, 3, 1, 2)[:, :3, 5:5 + H, 7:7 + W]     # [B, 3, H, W] view with a channel stride of 1
    assert same(pp(chw_view))
    np.testing.assert_array_equal(base.cpu().float().numpy(), _host_reference(list(hwc), 64).half().float().numpy())


def test_encode_image_end_to_end_tiny():
    sd = syn.synthetic_state_dict("tiny", seed=0)
    model = build_model(dict(sd), {"trainer": "ZeroshotCLIP"}).cuda()
    pp = Preprocess.for_model(model)
    assert pp.n_px == model.visual.input_resolution == 64
    imgs = _images([(375, 500), (64, 64), (90, 70), (500, 375)], seed=3)
    with torch.no_grad():
        a = model.encode_image(pp(imgs))
        b = model.encode_image(_host_reference(imgs, 64).cuda())
    assert torch.equal(a, b)


def test_encode_image_end_to_end_vitb16():
    sd = syn.synthetic_state_dict("ViT-B/16", seed=0)
    model = build_model(dict(sd), {"trainer": "ZeroshotCLIP"}).cuda()
    pp = Preprocess.for_model(model)
    assert pp.n_px == 224
    imgs = _images([(375, 500), (224, 224), (640, 427)], seed=11)
    with torch.no_grad():
        a = model.encode_image(pp(imgs))
        b = model.encode_image(_host_reference(imgs, 224).cuda())
    assert torch.equal(a, b)


def test_deterministic_beside_the_tower():
    sd = syn.synthetic_state_dict("ViT-B/16", seed=0)
    model = build_model(dict(sd), {"trainer": "ZeroshotCLIP"}).cuda()
    imgs = torch.from_numpy(np.stack([ref.synthetic_image(375, 500, 30 + i) for i in range(64)])).cuda()
    pp = Preprocess(224)
    first, second = pp(imgs), pp(imgs)
    x = torch.randn(64, 3, 224, 224, device="cuda").half()
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.no_grad():
        for _ in range(3):
            side.wait_stream(torch.cuda.current_stream())
            feats = model.encode_image(x)                      # main stream: the tower
            with torch.cuda.stream(side):
                beside = pp(imgs)                               # side stream: co-resident with the tower's kernels
            torch.cuda.current_stream().wait_stream(side)
            torch.cuda.synchronize()
            assert torch.equal(beside.view(torch.int16), first.view(torch.int16))
    assert torch.equal(first.view(torch.int16), second.view(torch.int16)) and feats.isfinite().all()


def test_device_batches_preprocess():
    pp = Preprocess(64)
    sizes = [[(375, 500), (64, 64), (20, 90)], [(500, 375), (33, 33)], [(128, 200)] * 4]
    batches = [(pack_images(_images(s, seed=40 + j)).pin_memory(), torch.arange(len(s))) for j, s in enumerate(sizes)]
    dense = (torch.from_numpy(np.stack(_images([(100, 140)] * 2, seed=60))), torch.tensor([7, 8]))
    loader = batches + [dense]
    got = list(device_batches(loader, preprocess=pp))
    assert len(got) == len(loader)
    for (img, lab), (src, src_lab) in zip(got, loader):
        assert img.is_cuda and img.dtype == torch.float16 and lab.is_cuda
        assert torch.equal(img.view(torch.int16), pp(src).view(torch.int16)) and torch.equal(lab.cpu(), src_lab)
