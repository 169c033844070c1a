"""DeepLab-v1 training data on the host (wseg_amd/data.py RandomHSV ... SegRandomCrop, wseg_amd/seg_data.py draw_seg_params and the tables):
the draws against the host chain's, the cv2-free transforms against fixtures made by the reference's own transform.py
(scripts/make_seg_data_goldens.py), the label index tables against the direct formula, the forward HSV against exact rational arithmetic on all
2^24 colours, the HSV round trip within a bound derived from the quantisation steps — and planted defects, each of which one of these
checks must catch."""
import os
import random

import numpy as np
import pytest

from tests import seg_data_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "seg_data_chain.npz")


class Recording:
    """writes down every draw the chain makes of a random.Random (a wrapper, not a subclass: overriding random() in a subclass makes
    randrange draw through it, another stream)"""

    def __init__(self, seed):
        self.rng, self.calls = random.Random(seed), []

    def randint(self, a, b):
        v = self.rng.randint(a, b); self.calls.append(("randint", a, b, v)); return v

    def random(self):
        v = self.rng.random(); self.calls.append(("random", v)); return v

    def randrange(self, *a):
        v = self.rng.randrange(*a); self.calls.append(("randrange", a, v)); return v

    def getstate(self):
        return self.rng.getstate()


def _host(img, lab, crop, seed, **kw):
    from wseg_amd import data as wdata
    rng = Recording(seed)
    out = wdata.seg_apply_transforms(img, lab, wdata.seg_train_transform(crop, rng=rng, **kw))
    return out, rng


# (H, W) on both sides of the crop at every scale of [0.5, 1.5], and on one side only
@pytest.mark.parametrize("hw", [(20, 24), (150, 170), (20, 170), (170, 20), (64, 64), (47, 90), (33, 47)])
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_draws_are_the_host_chains_draws_in_its_order(hw, seed):
    from wseg_amd import seg_data as D
    h, w = hw
    crop = 64
    img, lab = R.image(h, w, seed), R.label_map(h, w, seed)
    (himg, hlab), rng_h = _host(img, lab, crop, seed)
    rng_d = Recording(seed)
    p = D.draw_seg_params(w, h, crop, rng=rng_d)
    # the same calls with the same arguments and results, in the same order (randrange's argument carries the rescaled size), and the
    # same generator state afterwards
    assert rng_d.calls == rng_h.calls
    assert [c[0] for c in rng_d.calls] == ["randint"] * 3 + ["random", "random", "randrange", "randrange"]
    assert rng_d.getstate() == rng_h.getstate()
    assert (p["dh"], p["ds"], p["dv"]) == tuple(c[3] for c in rng_d.calls[:3])
    assert p["flip"] == int(rng_d.calls[3][1] < 0.5) and p["scale"] == rng_d.calls[4][1] * (1.5 - 0.5) + 0.5
    assert (p["rh"], p["rw"]) == (round(h * p["scale"]), round(w * p["scale"]))
    # and they mean the same: the plain restatement under these parameters gives the host chain's output
    rimg, rlab = R.chain(img, lab, p, crop)
    assert np.array_equal(himg.view(np.int32), rimg.view(np.int32)) and np.array_equal(hlab, rlab)


def test_make_seg_sample_draws_once_and_builds_the_tables():
    from wseg_amd import augment as A, seg_data as D
    h, w, crop, seed = 37, 53, 32, 5
    s = D.make_seg_sample("a", R.image(h, w, seed), R.label_map(h, w, seed), crop, rng=random.Random(seed))
    p = D.draw_seg_params(w, h, crop, rng=random.Random(seed))
    assert {k: s["params"][k] for k in p} == p
    xb, xk = A.pil_bicubic_coeffs(w, p["rw"])
    assert np.array_equal(s["xb"], xb) and np.array_equal(s["xk"], xk) and s["yi"].shape == (p["rh"],) and s["xi"].shape == (p["rw"],)
    b = D.seg_collate([s, D.make_seg_sample("b", R.image(9, 70, 1), R.label_map(9, 70, 1), crop, rng=random.Random(1))])
    for smp in (s,):
        q = smp["params"]
        assert np.array_equal(b["u8"].numpy()[q["img_off"]:q["img_off"] + h * w * 3].reshape(h, w, 3), smp["img"])
        assert np.array_equal(b["u8"].numpy()[q["lab_off"]:q["lab_off"] + h * w].reshape(h, w), smp["label"])
        assert q["img_off"] % 16 == 0 and q["lab_off"] % 16 == 0
        for k, o in zip(D.TABLES, q["tab_off"]):
            assert np.array_equal(b["tab"].numpy()[o:o + smp[k].size], smp[k].reshape(-1))


# ------------------------------------------------------------------------------------------------ fixtures of the reference's transform.py
def _fixture_case(z, i):
    state = (3, tuple(int(x) for x in z[f"state_{i}"]), None)
    return z[f"in_image_{i}"], z[f"in_seg_{i}"], z[f"out_image_{i}"], z[f"out_seg_{i}"], state, float(z[f"next_{i}"])


def _reproduces_fixtures(crop_cls=None, flip_cls=None):
    """does the host chain's flip -> normalise -> crop give the reference's bytes, offsets and generator state on every fixture case?"""
    from wseg_amd import data as wdata
    z = np.load(GOLDEN)
    crop, ok = int(z["crop"]), True
    assert tuple(z["mean"]) == wdata.SEG_MEAN and tuple(z["std"]) == wdata.SEG_STD
    sizes = set()
    for i, (h, w, seed) in enumerate(z["cases"]):
        image, seg, ref_img, ref_seg, state, nxt = _fixture_case(z, i)
        sizes.add((h > crop, w > crop))
        rng = random.Random(int(seed))
        x, lab = (flip_cls or wdata.RandomFlip)(0.5, rng=rng)(image, seg)
        x, lab = wdata.ImageNorm()(x, lab)
        x, lab = (crop_cls or wdata.SegRandomCrop)(crop, rng=rng)(x, lab)
        assert ref_img.dtype == np.float32 and ref_seg.dtype == np.float32 and x.dtype == np.float32 and lab.dtype == np.uint8
        good = np.array_equal(x.view(np.int32), ref_img.view(np.int32))       # as bits: -0.0 cannot pass for the +0.0 padding
        good = good and np.array_equal(lab.astype(np.float32), ref_seg)
        good = good and rng.getstate() == state and rng.random() == nxt
        # the fixture itself holds what it is there to show: +0.0 and 255 outside the pasted rectangle
        pad = ref_seg == 255
        assert not np.signbit(ref_img[np.all(ref_img == 0, axis=-1)]).any()
        if h < crop or w < crop:
            assert pad.any() and np.all(ref_img[np.all(ref_img == 0, axis=-1)] == 0)
        ok = ok and good
    assert sizes >= {(False, False), (True, True), (False, True), (True, False)}
    assert z["flipped"].any() and not z["flipped"].all()
    return ok


def test_flip_normalise_crop_reproduce_the_reference_fixtures():
    assert _reproduces_fixtures()


def test_padding_is_plus_zero_and_255_at_the_drawn_offsets():
    from wseg_amd import data as wdata
    rng = random.Random(3)
    x = np.full((5, 7, 3), -1.5, np.float32)
    img, lab = wdata.SegRandomCrop(16, rng=rng)(x, np.full((5, 7), 4, np.uint8))
    rng2 = random.Random(3)
    cl, ct = rng2.randrange(16 - 7 + 1), rng2.randrange(16 - 5 + 1)          # width first
    inside = np.zeros((16, 16), bool); inside[ct:ct + 5, cl:cl + 7] = True
    assert np.all(img[inside] == -1.5) and np.all(img[~inside] == 0) and not np.signbit(img[~inside]).any()
    assert np.all(lab[inside] == 4) and np.all(lab[~inside] == 255)


def test_normalise_is_the_float32_table():
    from wseg_amd import aff_data, augment, data as wdata
    v = np.arange(256, dtype=np.uint8)
    x, _ = wdata.ImageNorm()(np.stack([v, v, v], -1)[None], None)
    lut = aff_data.normalize_lut_f32()
    assert np.array_equal(x[0].T.view(np.int32), lut.view(np.int32))
    assert not np.array_equal(lut, augment.normalize_lut())                   # (the float64 table of the contrast chain is another one)


# ------------------------------------------------------------------------------------------------ label index tables
def test_label_index_tables():
    from wseg_amd import data as wdata, seg_data as D
    for n in (1, 7, 64):
        t = wdata.nearest_index_table(n, n, 1.0)
        assert np.array_equal(t, np.arange(n)) and t.dtype == np.int32        # the identity at s = 1
    # monotone, from 0, never past the last source index
    for n_in, s in ((31, 1.5), (13, 0.77), (5, 0.5), (3, 1.4), (9, 1.45)):
        t = wdata.nearest_index_table(n_in, round(n_in * s), s)
        assert t.max() <= n_in - 1 and t.min() == 0 and np.all(np.diff(t) >= 0)
    assert wdata.nearest_index_table(5, 8, 1.5).tolist() == [0, 0, 1, 2, 2, 3, 4, 4]          # round(7.5) = 8, half to even; floor(7 / 1.5) = 4
    # the last entries clamp: round(10 * 0.95) = round(9.5) = 10 positions and floor(9 / 0.95) = 9 is the last index, but a table of 4
    # positions over 2 sources at 1.25 reaches floor(3 / 1.25) = 2 > n - 1 = 1
    assert wdata.nearest_index_table(10, 10, 0.95)[-1] == 9
    assert wdata.nearest_index_table(2, 4, 1.25).tolist() == [0, 0, 1, 1]
    assert wdata.nearest_index_table(1, 2, 1.5).tolist() == [0, 0]
    # the direct formula, and composing with the flip = flipping, then indexing
    for s in (0.5, 0.77, 1.5):
        for flip in (0, 1):
            h, w = 23, 31
            lab = R.label_map(h, w, 7)
            p = dict(scale=s, rh=round(h * s), rw=round(w * s), flip=flip)
            yi, xi = D.label_index_tables(h, w, p)
            direct = R.nearest(np.flip(lab, axis=1) if flip else lab, p["rh"], p["rw"], s)
            assert np.array_equal(lab[yi][:, xi], direct)
            assert yi.dtype == np.int32 and xi.dtype == np.int32 and 0 <= xi.min() and xi.max() < w


# ------------------------------------------------------------------------------------------------ HSV
@pytest.fixture(scope="module")
def colours():
    from wseg_amd import data as wdata
    rgb = R.all_colours()
    return rgb, wdata.rgb2hsv_u8(rgb), R.hsv_forward_exact(rgb)


def test_forward_hsv_against_exact_rational_arithmetic_on_all_colours(colours):
    # Measured share of the 2^24 colours where the 12-bit tables (which round halves up) differ from the exact quotient rounded half to
    # even: H on 368109 colours (2.1941 %), S on 199146 (1.1870 %); never by more than 1.
    rgb, (h, s, v), (he, se, ve) = colours
    assert np.array_equal(v, ve)
    dh = np.abs(h - he)
    dh = np.minimum(dh, 180 - dh)                                               # compared modulo 180
    ds = np.abs(s - se)
    print(f"forward HSV, table against exact: H differs on {np.count_nonzero(dh)} colours ({100 * np.mean(dh > 0):.4f} %), max {dh.max()}; "
          f"S on {np.count_nonzero(ds)} ({100 * np.mean(ds > 0):.4f} %), max {ds.max()}")
    assert dh.max() <= 1 and ds.max() <= 1
    assert h.min() == 0 and h.max() == 179 and s.min() == 0 and s.max() == 255
    # and the plain Python statement of the table formula gives the host chain's integers
    sub = rgb[::97, ::89]
    hs, ss, vs = R.hsv_forward(sub)
    assert np.array_equal(hs, h[::97, ::89]) and np.array_equal(ss, s[::97, ::89]) and np.array_equal(vs, v[::97, ::89])


def roundtrip_bound():
    """max |channel out - channel in| of RGB -> HSV -> RGB at zero offsets, from the quantisation steps (never from a run).
    With C = V S the chroma, every output channel is V - C g(H) with g piecewise linear in the hue, slope 1 per sector (60 degrees = 30
    hue steps) and 0 <= g <= 1: a hue error of dH steps moves a channel by at most C dH / 30, a saturation error of dS (in 1/255) by at
    most V dS g <= v dS / 255, both at most at C = V = 255 / 255.  V itself is exact (v / 255 * 255 rounds back to v).
      dH  half a step of the rounding to 2-degree steps, plus the table: hdiv is off its quotient by <= 1/2, times |hn| <= 5 * 255, / 4096
      dS  half a step, plus the table: sdiv off by <= 1/2, times diff <= 255, / 4096
    plus half a unit for the final rounding to uint8; the float32 roundings of the inverse (some 10 of relative 2^-24 on values <= 255)
    are far below the gap to the next integer.  The differences are integers: the bound is the floor."""
    dH = 0.5 + 0.5 * 5 * 255 / 4096
    dS = 0.5 + 0.5 * 255 / 4096
    return int(np.floor(255 * dH / 30 + dS + 0.5 + 255 * 10 * 2.0 ** -24))


def _roundtrip_within_bound(h, s, v, rgb, inverse):
    out = inverse(h, s, v)
    worst = int(np.abs(out.astype(np.int32) - rgb.astype(np.int32)).max())
    return worst <= roundtrip_bound(), worst


def test_round_trip_at_zero_offsets_stays_within_the_quantisation_bound(colours):
    from wseg_amd import data as wdata
    rgb, (h, s, v), _ = colours
    assert roundtrip_bound() == 6
    ok, worst = _roundtrip_within_bound(h, s, v, rgb, wdata.hsv2rgb_u8)
    print(f"HSV round trip at zero offsets over all 2^24 colours: max |channel difference| {worst}, bound {roundtrip_bound()}")
    assert ok
    assert np.array_equal(wdata.hsv_jitter(rgb[::16, ::16], 0, 0, 0), wdata.hsv2rgb_u8(h, s, v)[::16, ::16])
    grey = rgb[..., 0:1].repeat(3, -1)[:1, :256] * 0 + np.arange(256, dtype=np.uint8)[None, :, None]
    assert np.array_equal(wdata.hsv_jitter(grey, 0, 0, 0), grey)               # s = 0: r = g = b = v exactly


OFFSETS = [(0, 0, 0), (10, 10, 10), (-10, -10, -10), (10, -10, 10), (-10, 10, -10), (3, -7, 5)]


def _jitter_equals_restatement(jitter):
    """does `jitter` give the plain restatement's bytes on an image that holds hues next to both ends and s, v next to both clips?"""
    img = R.all_colours()[::61, ::67].copy()                                    # 68 x 62 colours spread over the cube
    img[0, :6] = [[255, 0, 0], [255, 0, 4], [250, 2, 0], [2, 1, 1], [254, 255, 253], [0, 0, 0]]
    return all(np.array_equal(jitter(img, *d), R.hsv_jitter(img, *d)) for d in OFFSETS)


def test_hsv_jitter_equals_the_plain_restatement():
    from wseg_amd import data as wdata
    assert _jitter_equals_restatement(wdata.hsv_jitter)
    img = R.all_colours()[::61, ::67]
    h, s, v = wdata.rgb2hsv_u8(img)                                              # the offsets reach the wrap and the clips on this image
    assert (h + 10 >= 180).any() and (h - 10 < 0).any() and (s + 10 > 255).any() and (s - 10 < 0).any() and (v + 10 > 255).any() and (v - 10 < 0).any()


# ------------------------------------------------------------------------------------------------ planted defects
def test_planted_defects_are_caught(colours):
    from wseg_amd import data as wdata
    rgb, (h, s, v), _ = colours
    sub = (slice(None, None, 5), slice(None, None, 3))

    # a wrong sector row: rows 2 and 3 of the table swapped -> the round trip leaves the bound
    wrong = list(wdata.HSV_SECTORS); wrong[2], wrong[3] = wrong[3], wrong[2]
    ok, worst = _roundtrip_within_bound(h[sub], s[sub], v[sub], rgb[sub], lambda *a: wdata.hsv2rgb_u8(*a, sectors=tuple(wrong)))
    assert not ok and worst > 100
    assert _roundtrip_within_bound(h[sub], s[sub], v[sub], rgb[sub], wdata.hsv2rgb_u8)[0]

    def variant(wrap=True, clip_s=True, clip_v=True):
        def jitter(img, dh, ds, dv):
            hh, ss, vv = wdata.rgb2hsv_u8(img)
            hh = (hh + dh) % 180 if wrap else (hh + dh).astype(np.uint8).astype(np.int32)      # (the uint8 stack of transform.py:99)
            ss = np.clip(ss + ds, 0, 255) if clip_s else (ss + ds).astype(np.uint8).astype(np.int32)
            vv = np.clip(vv + dv, 0, 255) if clip_v else (vv + dv).astype(np.uint8).astype(np.int32)
            return np.ascontiguousarray(wdata.hsv2rgb_u8(hh, ss, vv))
        return jitter
    assert _jitter_equals_restatement(variant())                                # the scaffold itself is sound
    assert not _jitter_equals_restatement(variant(wrap=False))                  # hue not wrapped at 180
    assert not _jitter_equals_restatement(variant(clip_s=False))                # S not clipped
    assert not _jitter_equals_restatement(variant(clip_v=False))                # V not clipped

    # a flip applied after the rescale: the nearest rescale floors, so it does not commute with the flip
    himg, wimg, crop, seed = 23, 31, 32, 11
    img, lab = R.image(himg, wimg, seed), R.label_map(himg, wimg, seed)
    kw = dict(scale_r=(0.77, 0.77), flip_p=1.0, hsv_r=(0, 0, 0))

    def equals_restatement(transforms, rng):
        from wseg_amd import seg_data as D
        out_img, out_lab = wdata.seg_apply_transforms(img, lab, transforms)
        p = D.draw_seg_params(wimg, himg, crop, rng=random.Random(seed), **kw)
        rimg, rlab = R.chain(img, lab, p, crop)
        return np.array_equal(out_img.view(np.int32), rimg.view(np.int32)) and np.array_equal(out_lab, rlab)
    rng = random.Random(seed)
    t = wdata.seg_train_transform(crop, rng=rng, **kw)
    assert equals_restatement(t, rng)
    rng = random.Random(seed)
    t = wdata.seg_train_transform(crop, rng=rng, **kw)
    flip_late = [t[0], _Swapped(t[1], t[2]), t[3], t[4]]                        # same draws in the same order, the flip applied after the rescale
    assert not equals_restatement(flip_late, rng)

    # padding with normalize(0) instead of +0.0: the reference fixtures refuse it
    class PadNormZero(wdata.SegRandomCrop):
        def __call__(self, image, label):
            out, seg = super().__call__(image, label)
            pad = seg == 255
            lut0 = np.array([(0 / 255 - m) / sd for m, sd in zip(wdata.SEG_MEAN, wdata.SEG_STD)], np.float32)
            out = out.copy(); out[pad & np.all(out == 0, axis=-1)] = lut0
            return out, seg
    assert not _reproduces_fixtures(crop_cls=PadNormZero)


class _Swapped:
    """draws the flip, then the scale (the chain's order of draws), but rescales BEFORE it flips"""

    def __init__(self, flip, scale):
        self.flip, self.scale = flip, scale

    def __call__(self, image, label):
        do_flip = self.flip.rng.random() < self.flip.flip_t
        image, label = self.scale(image, label)
        if do_flip:
            image, label = np.flip(image, axis=1), np.flip(label, axis=1)
        return image, label


# ------------------------------------------------------------------------------------------------ the datasets, from files
def test_datasets_read_the_jpeg_and_the_label_png(tmp_path):
    import PIL.Image
    from wseg_amd import data as wdata, seg_data as D
    name, h, w, crop = "2007_000123", 41, 57, 32
    os.makedirs(tmp_path / "JPEGImages"); os.makedirs(tmp_path / "pseudo")
    PIL.Image.fromarray(R.image(h, w, 2)).save(tmp_path / "JPEGImages" / (name + ".jpg"), quality=95)
    lab = R.label_map(h, w, 2)
    png = PIL.Image.frombytes("P", (w, h), lab.tobytes())                 # a palette PNG, as the pseudo labels are written: the indices are the classes
    png.putpalette([(i * 37) % 256 for i in range(768)])
    png.save(tmp_path / "pseudo" / (name + ".png"))
    (tmp_path / "train.txt").write_text(f"/JPEGImages/{name}.jpg /SegmentationClassAug/{name}.png\n")
    img = np.asarray(PIL.Image.open(tmp_path / "JPEGImages" / (name + ".jpg")).convert("RGB"))
    assert np.array_equal(wdata.load_seg_label(str(tmp_path / "pseudo" / (name + ".png"))), lab)

    random.seed(77)
    raw = D.VOCSegDatasetRaw(str(tmp_path / "train.txt"), str(tmp_path), str(tmp_path / "pseudo"), crop)
    assert len(raw) == 1
    s = raw[0]
    state = random.getstate()
    assert s["name"] == name and np.array_equal(s["img"], img) and np.array_equal(s["label"], lab)
    assert {k: s["params"][k] for k in ("dh", "flip", "scale")} == {k: D.draw_seg_params(w, h, crop, rng=random.Random(77))[k] for k in ("dh", "flip", "scale")}

    random.seed(77)                                           # the host dataset draws the same draws from the module's generator
    host = wdata.VOCSegTrainDataset(str(tmp_path / "train.txt"), str(tmp_path), str(tmp_path / "pseudo"), wdata.seg_train_transform(crop))
    himg, hlab = host[0]
    assert random.getstate() == state
    rimg, rlab = R.chain(img, lab, s["params"], crop)
    assert himg.shape == (3, crop, crop) and himg.dtype == np.float32 and hlab.shape == (crop, crop) and hlab.dtype == np.uint8
    assert np.array_equal(himg.view(np.int32), rimg.view(np.int32)) and np.array_equal(hlab, rlab)
