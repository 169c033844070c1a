"""The kernels of csrc/augment.hip one stage at a time against Pillow itself — PIL.Image.resize, ImageEnhance, convert("HSV") and the
slicing of wseg_amd/data.py —, BIT FOR BIT, on inputs built to reach what a random image does not: all 2^24 colours through the hue and
saturation ops, blend factors at which a fused multiply-add would show, mean luminances exactly on a .5 boundary, contrast in every stage
slot and after another op, an image the grid walks twice, resampler clipping on both sides, the identity resize, every crop placement.

The stages run through the C ABI on hand-built AugDesc arrays: the colour ops through wseg_aff_augment_batch (rw = W, rh = H, the ops not
under test -1; the image buffer is jittered in place and read back), the resize through wseg_augment_batch with all ops -1 (`tmp` and `img`
read back).  Every buffer a kernel writes lies between sentinel guards.  tests/augment_emul.py builds the inputs;
tests/test_augment_emul_host.py shows on the CPU that they would expose each wrong variant it names.  Nothing here is compared with that
restatement: it only states what an input hits (pytest -s prints the counts)."""
import functools

import numpy as np
import pytest
import torch

from tests import augment_emul as E

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 64                                               # elements of sentinel in front of, between and behind the regions of a blob
CROP = 8                                                 # of the calls whose finish kernel is not under test


class Blob:
    """One device buffer of several regions with sentinel guards around each: add() reserves (and optionally fills) a region, upload()
    puts it on the device, check() reads it back, asserts every guard element untouched and returns the regions."""

    def __init__(self, dtype, sentinel):
        self.dtype, self.sentinel, self.regions, self.size = dtype, sentinel, [], GUARD

    def add(self, data=None, size=None):
        size = int(data.size if data is not None else size)
        self.regions.append((self.size, size, None if data is None else np.ascontiguousarray(data, self.dtype).reshape(-1)))
        self.size += (size + 15) // 16 * 16 + GUARD                   # (16-element alignment, as the product's collate gives)
        return len(self.regions) - 1

    def upload(self):
        host = np.full(self.size, self.sentinel, self.dtype)
        for off, size, data in self.regions:
            if data is not None:
                host[off:off + size] = data
        self.dev = torch.from_numpy(host).to(DEV)
        return self

    def ptr(self, i):
        return self.dev.data_ptr() + self.regions[i][0] * self.dev.element_size()

    def check(self):
        back = self.dev.cpu().numpy()
        guard = np.ones(self.size, bool)
        for off, size, _ in self.regions:
            guard[off:off + size] = False
        same = np.isnan(back[guard]) if isinstance(self.sentinel, float) and np.isnan(self.sentinel) else back[guard] == self.sentinel
        assert same.all(), f"{int((~same).sum())} guard elements overwritten"
        return [back[off:off + size] for off, size, _ in self.regions]


def _upload_descs(descs):
    return torch.from_numpy(np.frombuffer(bytes(descs), np.uint8).copy()).to(DEV)


def _placement(d, rh, rw, crop):
    d.flip = d.cont_top = d.cont_left = d.img_top = d.img_left = 0
    d.ch, d.cw = min(crop, rh), min(crop, rw)


def run_colour(cases, lut=None, crop=CROP, garbage=0x5A5A5A5A5A5A5A5A):
    """cases: [dict(img, op, factor, hue_shift, + optional placement)] through wseg_aff_augment_batch in ONE call ->
    ([image as jittered in place], out float32 [n, 3, crop, crop]).  The sums buffer starts as `garbage`."""
    from wseg_amd import _lib as L
    from wseg_amd.augment import AugDesc
    n = len(cases)
    imgs, out = Blob(np.uint8, 0xA5), Blob(np.float32, float("nan"))
    for c in cases:
        imgs.add(c["img"])
        out.add(size=3 * crop * crop)
    imgs.upload(); out.upload()
    sums = torch.full((4 * n + GUARD,), garbage, dtype=torch.int64, device=DEV)
    lut_d = torch.from_numpy(np.ascontiguousarray(E.distinct_lut() if lut is None else lut, np.float32)).to(DEV)
    descs = (AugDesc * n)()
    for i, c in enumerate(cases):
        d, (h, w) = descs[i], c["img"].shape[:2]
        d.H, d.W, d.rh, d.rw = h, w, h, w
        d.img, d.out, d.hue_shift = imgs.ptr(i), out.ptr(i), c.get("hue_shift", 0)
        for j in range(4):
            d.op[j], d.factor[j] = c["op"][j], c["factor"][j]
        _placement(d, h, w, crop)
        for k in ("flip", "cont_top", "cont_left", "img_top", "img_left", "ch", "cw"):
            if k in c:
                setattr(d, k, c[k])
        assert 0 <= d.img_top <= h - d.ch and 0 <= d.img_left <= w - d.cw and 0 <= d.cont_top <= crop - d.ch and 0 <= d.cont_left <= crop - d.cw
    d_desc = _upload_descs(descs)
    L.aff_augment_batch(d_desc, n, max(c["img"].shape[0] * c["img"].shape[1] for c in cases), lut_d, crop, sums)
    torch.cuda.synchronize()
    assert (sums[4 * n:] == garbage).all()
    got = [r.reshape(c["img"].shape) for r, c in zip(imgs.check(), cases)]
    res = out.check()
    assert not any(np.isnan(r).any() for r in res)                    # the finish kernel wrote every element it owns
    return got, np.stack(res).reshape(n, 3, crop, crop)


def run_resize(cases, lut=None, crop=CROP):
    """cases: [dict(img, rh, rw, + optional placement)] through wseg_augment_batch with all ops -1 in ONE call ->
    ([tmp uint8 [H, rw, 3]], [img uint8 [rh, rw, 3]], out float32 [n, 3, crop, crop])"""
    from wseg_amd import _lib as L
    from wseg_amd import augment as A
    n = len(cases)
    src, tab = Blob(np.uint8, 0xA5), Blob(np.int32, 0x7FFFFFFF)       # (a guard coefficient read by mistake would wreck the sum)
    tmp, res, out = Blob(np.uint8, 0xA5), Blob(np.uint8, 0xA5), Blob(np.float32, float("nan"))
    for c in cases:
        h, w = c["img"].shape[:2]
        src.add(c["img"])
        for t in A.pil_bicubic_coeffs(w, c["rw"]) + A.pil_bicubic_coeffs(h, c["rh"]):
            tab.add(t)
        tmp.add(size=h * c["rw"] * 3); res.add(size=c["rh"] * c["rw"] * 3); out.add(size=3 * crop * crop)
    for b in (src, tab, tmp, res, out):
        b.upload()
    sums = torch.full((4 * n + GUARD,), -1, dtype=torch.int64, device=DEV)
    lut_d = torch.from_numpy(np.ascontiguousarray(E.distinct_lut() if lut is None else lut, np.float32)).to(DEV)
    descs = (A.AugDesc * n)()
    max_pixels = 1
    for i, c in enumerate(cases):
        d, (h, w) = descs[i], c["img"].shape[:2]
        d.src, d.H, d.W, d.rh, d.rw = src.ptr(i), h, w, c["rh"], c["rw"]
        d.xb, d.xk, d.yb, d.yk = (tab.ptr(4 * i + j) for j in range(4))
        d.xks, d.yks = (tab.regions[4 * i + j][1] // n_out for j, n_out in ((1, c["rw"]), (3, c["rh"])))
        d.tmp, d.img, d.out, d.hue_shift = tmp.ptr(i), res.ptr(i), out.ptr(i), 0
        for j in range(4):
            d.op[j], d.factor[j] = -1, 0.0
        _placement(d, c["rh"], c["rw"], crop)
        for k in ("flip", "cont_top", "cont_left", "img_top", "img_left", "ch", "cw"):
            if k in c:
                setattr(d, k, c[k])
        assert 0 <= d.img_top <= c["rh"] - d.ch and 0 <= d.img_left <= c["rw"] - d.cw and 0 <= d.cont_top <= crop - d.ch and 0 <= d.cont_left <= crop - d.cw
        max_pixels = max(max_pixels, h * c["rw"], c["rh"] * c["rw"])
    d_desc = _upload_descs(descs)
    L.augment_batch(d_desc, n, max_pixels, lut_d, crop, sums)
    torch.cuda.synchronize()
    assert (sums[4 * n:] == -1).all()
    src.check(); tab.check()
    tmps = [r.reshape(c["img"].shape[0], c["rw"], 3) for r, c in zip(tmp.check(), cases)]
    ress = [r.reshape(c["rh"], c["rw"], 3) for r, c in zip(res.check(), cases)]
    outs = out.check()
    assert not any(np.isnan(r).any() for r in outs)
    return tmps, ress, np.stack(outs).reshape(n, 3, crop, crop)


def _one(img, op, factor=0.0, hue_shift=0):
    return dict(img=img, op=[op, -1, -1, -1], factor=[factor, 0.0, 0.0, 0.0], hue_shift=hue_shift)


@functools.lru_cache(maxsize=None)
def _pil_hsv_of_all_colours():
    hsv = E.pil_rgb2hsv(E.all_colours())
    hsv.setflags(write=False)
    return hsv


# ---------------------------------------------------------------------------------------------- hue
@pytest.mark.parametrize("shift", E.HUE_SHIFTS)
def test_hue_on_all_colours(shift):
    ac, hsv = E.all_colours(), _pil_hsv_of_all_colours()
    shifted = np.array(hsv)
    shifted[..., 0] = (shifted[..., 0].astype(np.int16) + shift) % 256     # (the op as data.ColorJitter spells it)
    ref = E.pil_hsv2rgb(shifted)
    h, s = shifted[..., 0].reshape(-1), shifted[..., 1].reshape(-1)
    sector = np.floor(h.astype(np.float64) * 6.0 / 255.0).astype(int)
    per_sector = np.bincount(sector[s > 0], minlength=7)
    greys = np.unique(hsv.reshape(-1, 3)[(hsv[..., 1] == 0).reshape(-1)][:, 2]).size
    assert (per_sector[:6] > 0).all() and greys == 256
    assert per_sector[6] > 0 or shift == 0                            # h == 255 (i == 6) is reached only through a shift
    (got,), _ = run_colour([_one(ac, 3, hue_shift=shift)])
    bad = (got != ref).any(axis=-1)
    print(f"hue shift {shift}: 16777216 colours compared, differing {int(bad.sum())}; coloured pixels per sector i = 0..6 {per_sector.tolist()}, "
          f"grey values {greys}")
    if bad.any():
        y, x = np.argwhere(bad)[0]
        pytest.fail(f"{int(bad.sum())} colours differ; the first: rgb {ac[y, x].tolist()} Pillow hsv {hsv[y, x].tolist()} shifted {shifted[y, x].tolist()} "
                    f"Pillow rgb {ref[y, x].tolist()} device rgb {got[y, x].tolist()}")


# ---------------------------------------------------------------------------------------------- saturation, brightness
@pytest.mark.parametrize("factor", E.SATURATION_FACTORS, ids=repr)
def test_saturation_on_all_colours(factor):
    ac = E.all_colours()
    ref = E.pil_op(ac, 2, factor, 0)
    (got,), _ = run_colour([_one(ac, 2, factor)])
    bad = (got != ref).any(axis=-1)
    lum = E.pil_lum(ac)
    hit = int(E.fuse_changed(factor)[lum[..., None], ac].any(axis=-1).sum())
    print(f"saturation {factor!r}: 16777216 colours compared, differing {int(bad.sum())}; colours a fused blend would change {hit}")
    assert (hit > 0) == (factor in E.FUSE_BELOW + E.FUSE_ABOVE)
    if bad.any():
        y, x = np.argwhere(bad)[0]
        pytest.fail(f"{int(bad.sum())} colours differ; the first: rgb {ac[y, x].tolist()} luminance {int(lum[y, x])} Pillow {ref[y, x].tolist()} "
                    f"device {got[y, x].tolist()}")


def test_brightness_on_every_value():
    img = E.every_value_image()
    for c in range(3):
        assert np.array_equal(np.unique(img[..., c]), np.arange(256))
    got, _ = run_colour([_one(img, 0, f) for f in E.BRIGHTNESS_FACTORS])
    over_any = 0
    for f, g in zip(E.BRIGHTNESS_FACTORS, got):
        ref = E.pil_op(img, 0, f, 0)
        over = int((E.emul_blend_unclipped(0, img, f) > 255).sum())
        over_any += over
        print(f"brightness {f}: {img.size} values compared, differing {int((g != ref).sum())}; unclipped results above 255: {over}")
        assert np.array_equal(g, ref), (f, np.argwhere(g != ref)[:5])
    assert over_any > 0


# ---------------------------------------------------------------------------------------------- contrast and the luminance sum
def test_contrast_and_the_luminance_sum_in_one_batch():
    cases = E.contrast_cases()
    refs = [E.pil_chain(c["img"], c["op"], c["factor"], c["hue_shift"]) for c in cases]
    pixels = [c["img"].shape[0] * c["img"].shape[1] for c in cases]
    assert len(cases) >= 12 and {c["op"].index(1) for c in cases} == {0, 1, 2, 3}
    assert any(n % 64 for n in pixels) and max(pixels) > 1024 * 256 and len(set(pixels)) >= 8
    for c in cases:                                                   # the means, from Pillow's L image
        if c["op"].index(1) == min(j for j in range(4) if c["op"][j] >= 0):
            s, n = int(E.pil_lum(c["img"]).astype(np.int64).sum()), c["img"].shape[0] * c["img"].shape[1]
            c["mean2"] = (2 * s, n)
    half = [c["name"] for c in cases if "mean2" in c and (c["mean2"][0] % c["mean2"][1] == 0) and (c["mean2"][0] // c["mean2"][1]) % 2]
    below = [c["name"] for c in cases if "mean2" in c and ((c["mean2"][0] + 2) % c["mean2"][1] == 0) and ((c["mean2"][0] + 2) // c["mean2"][1]) % 2]
    exact = [c["name"] for c in cases if "mean2" in c and c["mean2"][0] % (2 * c["mean2"][1]) == 0 and 0 < c["mean2"][0] < 510 * c["mean2"][1]]
    assert len(half) >= 3 and len(below) >= 3 and len(exact) >= 3, (half, below, exact)
    assert any(not c["img"].any() for c in cases) and any((c["img"] == 255).all() for c in cases)
    for c in cases:                                                   # every value in every channel (but for the black and the white image)
        assert c["name"] in ("black", "white") or all(np.unique(c["img"][..., ch]).size == 256 for ch in range(3)), c["name"]
    assert any(0 in c["op"][:c["op"].index(1)] for c in cases) and any(3 in c["op"][:c["op"].index(1)] for c in cases)
    fuse = [c["factor"][c["op"].index(1)] for c in cases if c["factor"][c["op"].index(1)] in E.FUSE_BELOW + E.FUSE_ABOVE]
    assert min(fuse) < 1 < max(fuse)
    got1, _ = run_colour(cases, garbage=0x5A5A5A5A5A5A5A5A)
    got2, _ = run_colour(cases, garbage=-1)                           # fresh upload, other garbage in the sums: the same result
    print(f"contrast batch: {len(cases)} images, {sum(pixels)} pixels; mean exactly k + 0.5: {half}; exactly k: {exact}; just below k + 0.5: {below}")
    wrong = []
    for c, ref, g1, g2 in zip(cases, refs, got1, got2):
        d1, d2 = int((g1 != ref).any(axis=-1).sum()), int((g1 != g2).any(axis=-1).sum())
        print(f"  {c['name']}: {c['img'].shape[0]} x {c['img'].shape[1]}, op {c['op']}, factor {c['factor'][c['op'].index(1)]!r}: differing from Pillow {d1}, "
              f"between the two runs {d2}")
        if d1 or d2:
            wrong.append((c["name"], d1, d2))
    assert not wrong, wrong


# ---------------------------------------------------------------------------------------------- resize
def test_both_resize_passes_in_one_batch():
    from wseg_amd import augment as A
    cases = [dict(name=case[0], img=E.resize_image(case), rh=case[2][0], rw=case[2][1]) for case in E.RESIZE_CASES]
    tmps, ress, _ = run_resize(cases)
    totals, wrong = np.zeros((2, 2), np.int64), []
    for c, tmp, res in zip(cases, tmps, ress):
        h, w = c["img"].shape[:2]
        ref_tmp, ref = E.pil_resize(c["img"], c["rw"], h), E.pil_resize(c["img"], c["rw"], c["rh"])
        (xb, xk), (yb, yk) = A.pil_bicubic_coeffs(w, c["rw"]), A.pil_bicubic_coeffs(h, c["rh"])
        a1, a2 = E.emul_resize_pass(c["img"], xb, xk, 1), E.emul_resize_pass(ref_tmp, yb, yk, 0)
        hit = np.array([[(a1 < 0).sum(), (a1 > 255).sum()], [(a2 < 0).sum(), (a2 > 255).sum()]])
        totals += hit
        d1, d2 = int((tmp != ref_tmp).sum()), int((res != ref).sum())
        print(f"resize {c['name']}: {h} x {w} -> {c['rh']} x {c['rw']}, taps {xk.shape[1]} / {yk.shape[1]}: horizontal pass differing {d1} of {tmp.size}, "
              f"both passes {d2} of {res.size}; accumulator below 0 / above 255: horizontal {hit[0].tolist()}, vertical {hit[1].tolist()}")
        if d1 or d2:
            wrong.append((c["name"], d1, d2))
    assert (totals > 0).all(), totals
    assert not wrong, wrong


# ---------------------------------------------------------------------------------------------- the two finish kernels
def _luts(aff):
    from wseg_amd import aff_data as D
    from wseg_amd import augment as A
    return {"distinct": E.distinct_lut(), "production": D.normalize_lut_f32() if aff else A.normalize_lut()}


@pytest.mark.parametrize("table", ["distinct", "production"])
@pytest.mark.parametrize("crop", E.FINISH_CROPS)
@pytest.mark.parametrize("aff", [False, True], ids=["contrast", "affinity"])
def test_finish_kernels_place_flip_and_pad(aff, crop, table):
    lut = _luts(aff)[table]
    cases = [dict(c, op=[-1] * 4, factor=[0.0] * 4, rh=c["img"].shape[0], rw=c["img"].shape[1]) for c in E.finish_cases(crop)]
    if aff:
        imgs, out = run_colour(cases, lut, crop)
    else:
        _, imgs, out = run_resize(cases, lut, crop)                   # (identity resize: the finish kernel reads `img`)
    wrong, padded = [], 0
    for i, c in enumerate(cases):
        assert np.array_equal(imgs[i], c["img"]), c["name"]           # no colour op ran; the identity resize reproduced the source
        ref = E.ref_finish(c["img"], c, crop, lut, aff)
        if table == "production":                                     # the classes of wseg_amd/data.py themselves
            assert np.array_equal(ref, E.host_finish(c["img"], c, crop, aff)), c["name"]
        pad = np.ones((crop, crop), bool)
        left = crop - c["cont_left"] - c["cw"] if (aff and c["flip"]) else c["cont_left"]
        pad[c["cont_top"]:c["cont_top"] + c["ch"], left:left + c["cw"]] = False
        for ch in range(3):
            assert (ref[ch][pad] == (lut[ch][0] if aff else 0.0)).all()
        padded += int(pad.sum())
        if not np.array_equal(out[i], ref):
            wrong.append((c["name"], int((out[i] != ref).sum())))
    print(f"finish {'affinity' if aff else 'contrast'} crop {crop} table {table}: {len(cases)} placements, {out.size} values compared, "
          f"{3 * padded} of them padding; differing {wrong}")
    assert padded > 0 and not wrong, wrong
