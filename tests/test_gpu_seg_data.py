"""DeepLab-v1 training data on the GPU (wseg_amd/seg_data.py DeviceSegData, csrc/seg_data.hip): the HSV launch bit for bit against the host chain
on all 2^24 colours, the fused label gather against the plain restatement of tests/seg_data_ref.py, the whole chain against the host chain
from the same draws (the image compared as int32 so that -0.0 cannot pass for +0.0), determinism, the hand-over to seg_cross_entropy, and
the refusals of the entry point."""
import random

import numpy as np
import pytest
import torch

from tests import seg_data_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _forced(h, w, crop, scale, flip, seed, hsv_r=(0, 0, 0)):
    """a sample at a given scale and flip bit (the ranges leave the generator no choice); the crop offsets come from the seed"""
    from wseg_amd import seg_data as D
    img, lab = R.image(h, w, seed), R.label_map(h, w, seed)
    s = D.make_seg_sample(f"s{seed}", img, lab, crop, scale_r=(scale, scale), hsv_r=hsv_r, flip_p=1.0 if flip else 0.0, rng=random.Random(seed))
    assert s["params"]["scale"] == scale and s["params"]["flip"] == int(flip)
    return s


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


# ------------------------------------------------------------------------------------------------ the HSV launch
@pytest.fixture(scope="module")
def dsd():
    from wseg_amd import seg_data as D
    return D.DeviceSegData(DEV, crop=32)


def test_hsv_kernel_on_all_colours_equals_the_host_chain(dsd):
    from wseg_amd import data as wdata, seg_data as D
    rgb = R.all_colours()
    hsv_wg = D.geometry(4096 * 4096, 32)[0]
    assert hsv_wg * 256 * 4 < 4096 * 4096                                        # several passes of the grid-stride loop
    got = dsd.hsv(rgb, (0, 0, 0)).cpu().numpy()
    assert np.array_equal(got, wdata.hsv_jitter(rgb, 0, 0, 0))


@pytest.mark.parametrize("deltas", [(10, 10, 10), (-10, -10, -10), (10, -10, 10), (-10, 10, -10)])
def test_hsv_kernel_with_offsets_equals_the_host_chain(dsd, deltas):
    from wseg_amd import data as wdata
    sub = R.all_colours().reshape(-1, 3)[::7]                                    # every 7th colour: 2396746 = 2 x 1198373, an odd width
    sub = np.ascontiguousarray(sub.reshape(2, -1, 3))
    h, s, v = wdata.rgb2hsv_u8(sub)
    dh, ds, dv = deltas                                                          # the wrap and the clips are reached
    assert ((h + dh >= 180).any() or (h + dh < 0).any()) and ((s + ds > 255).any() or (s + ds < 0).any()) and ((v + dv > 255).any() or (v + dv < 0).any())
    got = dsd.hsv(sub, deltas).cpu().numpy()
    assert np.array_equal(got, wdata.hsv_jitter(sub, *deltas))


@pytest.mark.parametrize("hw", [(37, 53), (1, 1), (3, 1), (2, 6)])
def test_hsv_kernel_flips_into_column_w_minus_1_minus_x(dsd, hw):
    from wseg_amd import data as wdata
    img = R.image(hw[0], hw[1], 3)                                               # 37 x 53: the width is no multiple of any vector width
    want = wdata.hsv_jitter(img, 3, -7, 5)
    assert np.array_equal(dsd.hsv(img, (3, -7, 5), flip=True).cpu().numpy(), want[:, ::-1])
    assert np.array_equal(dsd.hsv(img, (3, -7, 5), flip=False).cpu().numpy(), want)
    assert np.array_equal(want, R.hsv_jitter(img, 3, -7, 5))


# ------------------------------------------------------------------------------------------------ labels
LABEL_CASES = [((23, 31), 0.5, 32),          # padding on both axes
               ((40, 56), 1.5, 32),          # the crop inside on both axes
               ((20, 90), 1.0, 32),          # one axis of each kind
               ((23, 31), 0.77, 32),
               ((131, 150), 0.77, 64)]       # crop 64: four workgroups per image in the finish launch


@pytest.mark.parametrize("flip", [0, 1])
@pytest.mark.parametrize("hw,scale,crop", LABEL_CASES)
def test_labels_equal_the_direct_formula(hw, scale, crop, flip):
    from wseg_amd import seg_data as D
    s = _forced(hw[0], hw[1], crop, scale, flip, seed=17 + flip)
    p = s["params"]
    assert set(np.unique(s["label"])) == set(range(21)) | {255}
    if crop == 64:
        assert D.geometry(1, crop)[2] > 1 and D.geometry(1, crop)[3] == 4        # more than one workgroup per image; no loop to pass twice
    _, label = D.DeviceSegData(DEV, crop)([s])
    want = R.label_chain(s["label"], p, crop)
    assert np.array_equal(label[0].cpu().numpy(), want)
    assert (want == 255).any()


# ------------------------------------------------------------------------------------------------ the whole chain
def _drawn_batch(crop, seed):
    """three images of different sizes with drawn parameters: (samples, host chain outputs from the same generator states)"""
    from wseg_amd import data as wdata, seg_data as D
    sizes = [(37, 53), (3 * crop, 2 * crop + 5), (crop // 2 + 3, 3 * crop + 1)]
    samples, host = [], []
    for i, (h, w) in enumerate(sizes):
        img, lab = R.image(h, w, seed + i), R.label_map(h, w, seed + i)
        samples.append(D.make_seg_sample(f"d{i}", img, lab, crop, rng=random.Random(seed + i)))
        host.append(wdata.seg_apply_transforms(img, lab, wdata.seg_train_transform(crop, rng=random.Random(seed + i))))
    return samples, host


@pytest.mark.parametrize("crop", [32, 64, 30])             # 30: no multiple of 4, the scalar finish kernel
def test_whole_chain_equals_the_host_chain_bit_for_bit(crop):
    from wseg_amd import seg_data as D
    samples, host = _drawn_batch(crop, seed=40)
    flips = [s["params"]["flip"] for s in samples]
    assert 0 < sum(flips) < 3                                                   # one of them flipped, one not
    assert any(s["params"]["rh"] < crop or s["params"]["rw"] < crop for s in samples) and any(s["params"]["rh"] > crop for s in samples)
    assert D.geometry(1, crop)[3] == (1 if crop % 4 else 4)
    img, label = D.DeviceSegData(DEV, crop)(D.seg_collate(samples))
    img, label = img.cpu().numpy(), label.cpu().numpy()
    for i, (himg, hlab) in enumerate(host):
        assert np.array_equal(_bits(img[i]), _bits(himg)), i
        assert np.array_equal(label[i], hlab), i
        pad = hlab == 255
        assert not np.signbit(img[i][:, pad & (himg == 0).all(0)]).any()


def test_an_image_past_one_pass_of_the_resize_loop():
    """530 x 517 at 1.1: 530 x 569 and 583 x 569 pixels per pass against 1024 workgroups of 256 threads"""
    from wseg_amd import data as wdata, seg_data as D
    crop, seed = 64, 9
    h, w = 530, 517
    img, lab = R.image(h, w, seed), R.label_map(h, w, seed)
    kw = dict(scale_r=(1.1, 1.1), hsv_r=(10, 10, 10), flip_p=1.0)
    s = D.make_seg_sample("big", img, lab, crop, rng=random.Random(seed), **kw)
    p = s["params"]
    assert D.geometry(h * p["rw"], crop)[1] * 256 < h * p["rw"] and D.geometry(h * p["rw"], crop)[1] == 1024
    himg, hlab = wdata.seg_apply_transforms(img, lab, wdata.seg_train_transform(crop, rng=random.Random(seed), **kw))
    gimg, glab = D.DeviceSegData(DEV, crop)([s])
    assert np.array_equal(_bits(gimg[0].cpu().numpy()), _bits(himg)) and np.array_equal(glab[0].cpu().numpy(), hlab)
    assert np.array_equal(hlab, R.label_chain(lab, p, crop))


# ------------------------------------------------------------------------------------------------ determinism and the contract
def test_determinism_contract_and_the_hand_over_to_the_loss():
    from tests import seg_loss_f64 as S
    from wseg_amd import seg_data as D
    from wseg_amd.seg_loss import seg_cross_entropy
    crop = 64
    samples, _ = _drawn_batch(crop, seed=40)
    batch = D.seg_collate(samples)
    dev = D.DeviceSegData(DEV, crop)
    img, label = dev(batch)
    img2, label2 = dev(batch)
    assert img.dtype == torch.float32 and tuple(img.shape) == (3, 3, crop, crop) and img.is_contiguous() and img.is_cuda
    assert label.dtype == torch.uint8 and tuple(label.shape) == (3, crop, crop) and label.is_contiguous() and label.is_cuda
    assert torch.equal(img.view(torch.int32), img2.view(torch.int32)) and torch.equal(label, label2)
    keep = img.clone(), label.clone()
    dev.launch_last()                                                           # every launch is out of place: again the same bytes
    assert torch.equal(img.view(torch.int32), keep[0].view(torch.int32)) and torch.equal(label, keep[1])
    # the label goes into the loss as it comes
    g = torch.Generator().manual_seed(3)
    coarse = (4.0 * torch.randn(3, 21, crop // 8, crop // 8, generator=g)).float()
    loss, stats = seg_cross_entropy(coarse.to(DEV), label)
    ref = S.restate(coarse.double(), label.cpu())
    assert int(ref["count"]) > 0 and int(ref["oor"]) == 0 and int((label == 255).sum()) > 0
    assert S.within(loss.detach().cpu(), ref["loss"], S.loss_bar(ref, coarse))
    assert float(stats[1]) == float(ref["count"])


# ------------------------------------------------------------------------------------------------ refusals
def test_bad_descriptors_are_refused_before_any_launch():
    from wseg_amd import _lib as L, seg_data as D
    crop = 32
    samples, _ = _drawn_batch(crop, seed=40)
    dev = D.DeviceSegData(DEV, crop)
    img, label = dev(D.seg_collate(samples))
    good = img.clone(), label.clone()
    aug, seg, d_desc, seg_at, n = dev._last
    lut, div = dev._lut()
    a_dev, s_dev = d_desc.data_ptr(), d_desc.data_ptr() + seg_at

    def call(aug_h=aug, seg_h=seg, a_d=a_dev, s_d=s_dev, n_=n, crop_=crop, lut_=lut, div_=div, stages=7):
        L.seg_data_batch(aug_h, seg_h, a_d, s_d, n_, crop_, lut_, div_, stages)

    def refused(**kw):
        img.fill_(-7.0); label.fill_(99)
        with pytest.raises(RuntimeError, match="seg_data_batch"):
            call(**kw)
        torch.cuda.synchronize()
        assert bool((img == -7.0).all()) and bool((label == 99).all())         # nothing was launched

    refused(n_=0)
    refused(n_=-1)
    refused(crop_=0)
    refused(crop_=-32)
    refused(stages=0)
    refused(aug_h=None)
    refused(seg_h=None)
    refused(a_d=0)
    refused(s_d=0)
    refused(lut_=0)
    refused(div_=0)

    def with_field(arr, i, name, value, **kw):
        old = getattr(arr[i], name)
        setattr(arr[i], name, value)
        try:
            refused(**kw)
        finally:
            setattr(arr[i], name, old)

    for name in ("src", "tmp", "img", "out", "xb", "xk", "yb", "yk"):           # a null pointer
        with_field(aug, 1, name, None)
    for name in ("raw", "lab", "yi", "xi", "lab_out"):
        with_field(seg, 2, name, None)
    a = aug[1]                                                                   # 96 x 69 scaled: larger than the crop in both dimensions
    assert a.rh > crop and a.rw > crop and a.ch == crop and a.cw == crop
    with_field(aug, 1, "ch", crop + 1)                                           # ch / cw beyond the crop
    with_field(aug, 1, "cw", crop + 1)
    with_field(aug, 1, "ch", 0)
    with_field(aug, 1, "cw", -1)
    with_field(aug, 1, "cont_top", 1)                                            # the rectangle leaves the container
    with_field(aug, 1, "cont_left", -1)
    with_field(aug, 1, "img_top", a.rh - crop + 1)                               # the rectangle leaves the rescaled image
    with_field(aug, 1, "img_left", a.rw - crop + 1)
    with_field(aug, 1, "img_top", -1)
    with_field(aug, 1, "img_left", -1)
    with_field(aug, 0, "H", 0)
    with_field(aug, 0, "rw", 0)
    with_field(aug, 0, "flip", 2)
    with_field(aug, 0, "out", aug[0].out + 4)                                    # off the 16-byte alignment of the vector stores
    with_field(seg, 0, "raw", seg[0].raw + 1)
    b = aug[0]                                                                   # 37 x 53: a small image
    if b.rh < crop:
        with_field(aug, 0, "ch", b.rh + 1)                                       # more rows than the rescaled image has
        with_field(aug, 0, "cont_top", crop - b.ch + 1)
    # and the untouched descriptors still give the outputs of the first call
    call()
    torch.cuda.synchronize()
    assert torch.equal(img.view(torch.int32), good[0].view(torch.int32)) and torch.equal(label, good[1])
