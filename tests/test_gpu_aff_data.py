"""AffinityNet training data on the GPU (wseg_amd/aff_data.py DeviceAffData, csrc/aff_data.hip, csrc/augment.hip wseg_aff_augment_batch):
the label map against the float64 dense rule of tests/aff_data_ref.py — exactly on quantised scores, and up to derived near-ties on generic
floats —, the image bit for bit against the host chain from the same draws, determinism and the hand-over to affinity_loss."""
import functools
import random

import numpy as np
import pytest
import torch

from tests import aff_data_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
Q = R.Q


def _sample(name, h, w, la, ha, crop, seed, **override):
    """a sample with drawn jitter and, where given, explicit crop / flip parameters (consistent ones: DeviceAffData checks them)"""
    from wseg_amd import aff_data as D
    s = D.make_aff_sample(name, R.image(h, w, seed), la, ha, crop, rng=random.Random(seed))
    s["params"].update(override)
    return s


def _exact_batch():
    """crop 64 (8 x 8 label maps).  Per sample: (H, W), shipped planes of the low / high alpha stack, explicit placement:
      0  larger than the crop in both dimensions, odd img_left, not flipped; carries the constructed ties and thresholds
      1  smaller in both, cont_top / cont_left no multiples of 8, flipped; the low-alpha stack has no plane 0
      2  mixed (short and wide), flipped; the high-alpha stack has no plane 0 and one plane only
      3  mixed (tall and narrow), not flipped; four planes against two
      4  smaller in both; the low-alpha stack is all zero: nothing of it is shipped"""
    crop = 64
    specs = [((150, 203), (0, 3, 7), (0, 3, 12), dict(img_top=41, img_left=77, cont_top=0, cont_left=0, flip=0)),
             ((37, 50), (5, 9), (0, 5, 20), dict(img_top=0, img_left=0, cont_top=13, cont_left=5, flip=1)),
             ((50, 100), (0, 2), (2,), dict(img_top=0, img_left=33, cont_top=6, cont_left=0, flip=1)),
             ((100, 41), (0, 1, 19, 20), (0, 19), dict(img_top=20, img_left=0, cont_top=0, cont_left=11, flip=0)),
             ((40, 40), (), (0, 4), dict(img_top=0, img_left=0, cont_top=24, cont_left=3, flip=0))]
    samples, dense = [], []
    for i, ((h, w), pl, ph, place) in enumerate(specs):
        la, ha = R.quantised_stack(h, w, pl, 20 + i), R.quantised_stack(h, w, ph, 60 + i)
        if i == 0:
            def window(oy, ox):                                  # source pixels of label cell (oy, ox) of sample 0 (cont 0, no flip)
                return (slice(None), slice(41 + 8 * oy, 49 + 8 * oy), slice(77 + 8 * ox, 85 + 8 * ox))
            la[window(2, 3)] = 0; la[(0,) + window(2, 3)[1:]] = 0.25      # two shipped planes tie on top: 3 and 7 at 0.5 over plane 0 at 0.25
            la[(3,) + window(2, 3)[1:]] = 0.5; la[(7,) + window(2, 3)[1:]] = 0.5
            ha[window(2, 3)] = 0; ha[(12,) + window(2, 3)[1:]] = 0.75
            for ox, v in ((1, 2), (2, 3)):                       # one pixel of v * 2^-12 in the window: pooled maxima of 2 * 2^-18 and 3 * 2^-18
                la[window(4, ox)] = 0; ha[window(4, ox)] = 0
                la[3, 41 + 32 + 5, 77 + 8 * ox + 6] = v * Q
                ha[3, 41 + 32 + 2, 77 + 8 * ox + 1] = v * Q
        if i == 1:
            la[:, 8:24, 10:30] = 0                               # shipped planes 5 and 9 at 0 against the absent plane 0: label cells (3, 4), (3, 5)
        if not pl:
            la[:] = 0
        samples.append(_sample("e%d" % i, h, w, la, ha, crop, 900 + i, **place))
        dense.append((la, ha))
    return crop, samples, dense


@pytest.fixture(scope="module")
def exact():
    from wseg_amd import aff_data as D
    crop, samples, dense = _exact_batch()
    batch = D.aff_collate(samples)
    refs = [R.dense_rule(la, ha, s["params"], crop, np.float64) for s, (la, ha) in zip(samples, dense)]
    return dict(crop=crop, samples=samples, dense=dense, batch=batch, label=np.stack([r[0] for r in refs]), pooled=[r[1] for r in refs])


def _top2(pooled21):
    s = np.sort(pooled21, axis=-1)
    return s[..., -1], s[..., -2]


def test_labels_on_quantised_scores_equal_the_float64_dense_rule_at_every_cell(exact):
    from wseg_amd import aff_data as D
    samples, pooled, ref = exact["samples"], exact["pooled"], exact["label"]
    # the batch holds what it was built to hold
    assert [s["ids"][0].tolist() for s in samples] == [[0, 3, 7], [5, 9], [0, 2], [0, 1, 19, 20], []]
    assert [s["ids"][1].tolist() for s in samples] == [[0, 3, 12], [0, 5, 20], [2], [0, 19], [0, 4]]
    assert samples[0]["params"]["img_left"] % 2 == 1 and {s["params"]["flip"] for s in samples} == {0, 1}
    assert samples[1]["params"]["cont_top"] % 8 and samples[1]["params"]["cont_left"] % 8
    t1, t2 = _top2(pooled[0][2, 3, :21])
    assert t1 == t2 == 0.5 and ref[0, 2, 3] == 3                                      # tie of two shipped planes: the lower one
    assert pooled[0][4, 1].max() == 2 * 2.0 ** -18 and ref[0, 4, 1] == 255             # below float32(1e-5): no score
    assert pooled[0][4, 2].max() == 3 * 2.0 ** -18 and ref[0, 4, 2] == 3               # above it
    for ox in (4, 5):                                                                   # shipped planes at 0 against the absent plane 0, inside the image
        assert pooled[1][3, ox, :21].max() == 0 and pooled[1][3, ox, 21:].max() > 0 and ref[1, 3, ox] in (0, 255)
    present = set(np.unique(ref).tolist())
    assert {0, 255} <= present and len(present - {0, 255}) >= 2, present
    img, label = D.DeviceAffData(DEV, exact["crop"])(exact["batch"])
    torch.cuda.synchronize()
    got = label.cpu().numpy()
    print("cells", got.size, "differing", int((got != ref).sum()), "labels present", sorted(present))
    assert np.array_equal(got, ref), np.argwhere(got != ref)[:10]


GENERIC_SIZES = [(37, 50), (150, 203), (100, 140), (130, 90), (128, 128), (75, 190), (203, 150), (60, 129)]


def _generic_batch():
    crop, samples, dense = 128, [], []
    for i, (h, w) in enumerate(GENERIC_SIZES):
        a, b = 1 + (3 * i) % 20, 1 + (3 * i + 7) % 20
        la, ha = R.float_stack(h, w, (0, a, b), 3000 + i, 1.0), R.float_stack(h, w, (0, a, b) if i % 3 else (a, b), 4000 + i, -1.0)
        samples.append(_sample("g%d" % i, h, w, la, ha, crop, 5000 + i))
        dense.append((la, ha))
    return crop, samples, dense


def generic_reference(crop, samples, dense):
    """(float64 labels, cells where float32 may differ).  All pooled terms are >= 0, so a float32 sum of 64 of them in any order is within
    63 * 2^-24 relative of the true sum: the arg-max of a stack can differ only where its top-1 / top-2 gap is below 2 * 64 * 2^-24 * top-1,
    the no-score test only where the overall maximum lies within that bar of 1e-5."""
    bar = 2 * 64 * 2.0 ** -24
    labels, loose = [], []
    for s, (la, ha) in zip(samples, dense):
        lab, pooled = R.dense_rule(la, ha, s["params"], crop, np.float64)
        ex = np.zeros(lab.shape, bool)
        for half in (pooled[..., :21], pooled[..., 21:]):
            t1, t2 = _top2(half)
            ex |= (t1 - t2) < bar * t1
        mx = pooled.max(axis=-1)
        ex |= np.abs(mx - R.F32_1E5) < bar * mx
        labels.append(lab); loose.append(ex)
    return np.stack(labels), np.stack(loose)


def test_labels_on_generic_floats_match_float64_outside_derived_near_ties():
    from wseg_amd import aff_data as D
    crop, samples, dense = _generic_batch()
    ref, loose = generic_reference(crop, samples, dense)
    present = set(np.unique(ref).tolist())
    assert {0, 255} <= present and len(present - {0, 255}) >= 2, present
    assert loose.sum() <= 0.001 * loose.size, (int(loose.sum()), loose.size)           # (checked on the CPU for these seeds: the cap holds)
    _, label = D.DeviceAffData(DEV, crop)(D.aff_collate(samples))
    torch.cuda.synchronize()
    got = label.cpu().numpy()
    bad = (got != ref) & ~loose
    print("cells", ref.size, "near ties excluded", int(loose.sum()), "differing", int((got != ref).sum()), "differing outside them", int(bad.sum()))
    assert not bad.any(), np.argwhere(bad)[:10]


IMAGE_SIZES = [(37, 50), (150, 203), (50, 100), (140, 41), (64, 64), (129, 203), (120, 160), (90, 131)]


@functools.lru_cache(maxsize=None)
def _drawn_batch(crop):
    """(samples, [(img, label) of the host chain from the same draws]): quantised scores, so the host's float32 means are exact"""
    from wseg_amd import aff_data as D
    samples, refs = [], []
    for i, (h, w) in enumerate(IMAGE_SIZES):
        img = R.image(h, w, 30 + i)
        la, ha = R.quantised_stack(h, w, (0, 6, 11), 200 + i), R.quantised_stack(h, w, (0, 6), 300 + i)
        seed = 1200 + i
        refs.append(R.host_chain(img, la, ha, seed, crop)[:2])
        random.seed(seed)
        samples.append(D.make_aff_sample("i%d" % i, img, la, ha, crop))
    return samples, refs


@pytest.mark.parametrize("crop", [64, 128])
def test_image_equals_the_host_chain_bit_for_bit(crop):
    from wseg_amd import aff_data as D
    lut = D.normalize_lut_f32()
    samples, refs = _drawn_batch(crop)
    assert {s["params"]["flip"] for s in samples} == {0, 1}
    assert any(s["params"]["H"] > crop and s["params"]["W"] > crop for s in samples)
    assert len({tuple(s["params"]["op"]) for s in samples}) > 3                       # several jitter orders
    out, label = D.DeviceAffData(DEV, crop)(D.aff_collate(samples))
    torch.cuda.synchronize()
    assert tuple(out.shape) == (len(samples), 3, crop, crop) and out.dtype == torch.float32
    for i, (s, (ref_img, ref_label)) in enumerate(zip(samples, refs)):
        got = out[i].cpu().numpy()
        assert np.array_equal(got, ref_img), (i, s["params"], float(np.abs(got - ref_img).max()), int((got != ref_img).sum()))
        assert np.array_equal(label[i].cpu().numpy(), ref_label), (i, s["params"])   # (quantised scores: the host's float32 means are exact)
    p = samples[0]["params"]                                                          # 37 x 50: padded on every side it can be
    assert p["ch"] == 37 and p["cw"] == 50 and p["H"] < crop and p["W"] < crop
    left = crop - p["cont_left"] - p["cw"] if p["flip"] else p["cont_left"]           # first container column of the pasted rectangle, as output
    outside = np.ones((crop, crop), bool)
    outside[p["cont_top"]:p["cont_top"] + 37, left:left + 50] = False
    got = out[0].cpu().numpy()
    for c in range(3):
        assert lut[c][0] != 0 and (got[c][outside] == lut[c][0]).all(), c


def test_determinism_and_the_contract_with_affinity_loss():
    from wseg_amd import aff_data as D
    from wseg_amd.aff_loss import affinity_loss
    crop = 64
    samples, refs = _drawn_batch(crop)
    batch, n = D.aff_collate(samples), len(samples)
    dad = D.DeviceAffData(DEV, crop)
    img1, lab1 = dad(batch)
    img2, lab2 = dad(batch)
    torch.cuda.synchronize()
    assert torch.equal(lab1, lab2) and torch.equal(img1, img2) and lab1.data_ptr() != lab2.data_ptr()
    assert lab1.dtype == torch.uint8 and lab1.is_contiguous() and lab1.is_cuda and tuple(lab1.shape) == (n, crop // 8, crop // 8)
    assert img1.dtype == torch.float32 and img1.is_contiguous() and img1.is_cuda
    host_labels = torch.from_numpy(np.stack([r[1] for r in refs]))           # the host chain's label maps, from the same draws
    feat = torch.nn.functional.elu(torch.randn(n, 8, crop // 8, crop // 8, generator=torch.Generator().manual_seed(3))).to(DEV)
    loss_d, stats_d = affinity_loss(feat, lab1)                              # the device tensor as it is
    loss_h, stats_h = affinity_loss(feat, host_labels.to(DEV))
    torch.cuda.synchronize()
    print("stats", stats_d.tolist())
    assert torch.equal(stats_d, stats_h) and torch.equal(loss_d, loss_h)
    assert stats_d.shape == (7,) and float(stats_d[4]) > 1 and float(stats_d[5]) > 1 and float(stats_d[6]) > 1     # all three pair kinds occur
    with pytest.raises(RuntimeError):
        D.DeviceAffData("cpu", crop)(batch)
    with pytest.raises(ValueError):
        D.DeviceAffData(DEV, 60)(batch)
    many = dict(batch, params=[dict(p, np=[22, p["np"][1]]) for p in batch["params"]])
    with pytest.raises(ValueError):
        dad(many)
