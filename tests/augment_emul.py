"""The arithmetic of csrc/augment.hip restated in numpy, with the named wrong variants a compiler flag or a careless edit could produce, and
the input builders that tests/test_augment_emul_host.py and tests/test_gpu_augment_kernels.py share.  TEST INFRASTRUCTURE, not product code.

The reference of both test files is Pillow itself (the `pil_*` functions at the end: PIL.Image.resize, ImageEnhance, convert("HSV") and the
slicing of wseg_amd/data.py).  The restatement (`emul_*`) is never what the device is compared with: the host file proves it equal to
Pillow on the inputs below and uses its variants to show that those inputs would expose each of them; the GPU file uses it only to state
what an input hits (overshoot of the resampler, unclipped brightness)."""
import functools

import numpy as np
import PIL.Image
import PIL.ImageEnhance

F32, F64 = np.float32, np.float64
VARIANTS = ("fused_blend", "h_float", "fmod_float", "hsv_trunc", "mean_no_half", "lum_no_round")


def _check(variant):
    if variant is not None and variant not in VARIANTS:
        raise ValueError(f"unknown variant {variant!r}")


# ---------------------------------------------------------------------------------------------- the restatement
def emul_resize_pass(src, bounds, coeffs, axis):
    """aug_resize_kernel without its final clip: (2^21 + sum_j src[lo + j] * k[j]) >> 22 along `axis` (1: horizontal, 0: vertical) of a
    uint8 [H, W, 3] image -> int64, so that values below 0 and above 255 are visible.  np.clip(., 0, 255) is what the kernel stores."""
    src = np.asarray(src)
    n_out = bounds.shape[0]
    acc = np.full((src.shape[0], n_out, 3) if axis == 1 else (n_out, src.shape[1], 3), 1 << 21, np.int64)
    for j in range(coeffs.shape[1]):
        idx = np.minimum(bounds[:, 0] + j, src.shape[axis] - 1)
        kj = np.where(j < bounds[:, 1], coeffs[:, j], 0).astype(np.int64)
        acc += (src[:, idx, :].astype(np.int64) * kj[None, :, None]) if axis == 1 else (src[idx, :, :].astype(np.int64) * kj[:, None, None])
    return acc >> 22


def emul_lum(rgb, variant=None):
    """lum_of (Convert.c rgb2l): (19595 r + 38470 g + 7471 b + 0x8000) >> 16.  lum_no_round drops the rounding constant."""
    _check(variant)
    p = np.asarray(rgb).astype(np.int64)
    return (p[..., 0] * 19595 + p[..., 1] * 38470 + p[..., 2] * 7471 + (0 if variant == "lum_no_round" else 0x8000)) >> 16


def emul_blend_unclipped(deg, img, alpha, variant=None):
    """The float32 value blend_u8 forms: deg + alpha * (img - deg), the product rounded to float32 before the sum (Blend.c as a compiler
    without contraction builds it).  fused_blend: the product exact, one rounding (what a fused multiply-add gives)."""
    _check(variant)
    alpha = F32(alpha)
    deg, img = np.asarray(deg).astype(np.int64), np.asarray(img).astype(np.int64)
    if variant == "fused_blend":                         # 24-bit alpha x 9-bit difference + 8-bit integer: exact in float64
        return (F64(alpha) * (img - deg).astype(F64) + deg.astype(F64)).astype(F32)
    return deg.astype(F32) + alpha * (img - deg).astype(F32)


def emul_blend(deg, img, alpha, variant=None):
    """blend_u8: truncation inside [0, 1]; outside, the clip to [0, 255] first"""
    t = emul_blend_unclipped(deg, img, alpha, variant)
    if not 0.0 <= F32(alpha) <= 1.0:
        t = np.clip(t, F32(0), F32(255))
    return t.astype(np.int32).astype(np.uint8)


def emul_rgb2hsv(rgb, variant=None):
    """rgb2hsv_u8 (Convert.c rgb2hsv_row: float variables, double constants).  h_float: the hue in float throughout; fmod_float: the
    `h / 6 + 1` step and its fmod in float."""
    _check(variant)
    p = np.asarray(rgb).astype(np.int32)
    r, g, b = p[..., 0], p[..., 1], p[..., 2]
    maxc, minc = np.maximum(r, np.maximum(g, b)), np.minimum(r, np.minimum(g, b))
    grey = maxc == minc
    with np.errstate(divide="ignore", invalid="ignore"):
        cr = (maxc - minc).astype(F32)
        s = cr / maxc.astype(F32)
        rc, gc, bc = (maxc - r).astype(F32) / cr, (maxc - g).astype(F32) / cr, (maxc - b).astype(F32) / cr
        if variant == "h_float":
            hg, hb = F32(2) + rc - bc, F32(4) + gc - rc
        else:
            hg, hb = (2.0 + rc.astype(F64) - bc.astype(F64)).astype(F32), (4.0 + gc.astype(F64) - rc.astype(F64)).astype(F32)
        h = np.where(r == maxc, bc - gc, np.where(g == maxc, hg, hb)).astype(F32)
        if variant == "fmod_float":
            t = h / F32(6) + F32(1)
            h = t - np.floor(t)
        else:
            t = h.astype(F64) / 6.0 + 1.0
            h = (t - np.floor(t)).astype(F32)
        ih, isat = (h.astype(F64) * 255.0), (s.astype(F64) * 255.0)
        ih, isat = np.where(grey, 0, ih).astype(np.int64), np.where(grey, 0, isat).astype(np.int64)
    out = np.empty(p.shape, np.uint8)
    out[..., 0], out[..., 1], out[..., 2] = np.clip(ih, 0, 255), np.clip(isat, 0, 255), maxc
    return out


def emul_hsv2rgb(hsv, variant=None):
    """hsv2rgb_u8 (Convert.c hsv2rgb).  hsv_trunc: p, q, t truncated, not rounded."""
    _check(variant)
    p = np.asarray(hsv).astype(np.int32)
    h, s, v = p[..., 0], p[..., 1], p[..., 2]
    t6 = h.astype(F32).astype(F64) * 6.0 / 255.0
    i = np.floor(t6).astype(np.int32)
    f = (t6 - i.astype(F32).astype(F64)).astype(F32).astype(F64)
    fs = (s.astype(F32).astype(F64) / 255.0).astype(F32).astype(F64)
    vf = v.astype(F64)
    half = 0.0 if variant == "hsv_trunc" else 0.5
    def fin(a): return np.clip(np.floor(a + half), 0, 255).astype(np.uint8)
    pp, q, t = fin(vf * (1.0 - fs)), fin(vf * (1.0 - fs * f)), fin(vf * (1.0 - fs * (1.0 - f)))
    vv = v.astype(np.uint8)
    sel = i % 6
    out = np.empty(p.shape, np.uint8)
    for c, choice in enumerate(((vv, q, pp, pp, t, vv), (t, vv, vv, q, pp, pp), (pp, pp, t, vv, vv, q))):
        out[..., c] = np.choose(sel, choice)
    grey = s == 0
    out[grey] = vv[grey][:, None]
    return out


def emul_mean(lum_sum, pixels, variant=None):
    """aug_color_kernel's contrast mean: int(sum / pixels + 0.5) in float64.  mean_no_half drops the 0.5."""
    _check(variant)
    return int(F64(lum_sum) / F64(pixels) + (0.0 if variant == "mean_no_half" else 0.5))


def emul_hue(rgb, shift, variant=None):
    hsv = emul_rgb2hsv(rgb, variant if variant in ("h_float", "fmod_float") else None)
    hsv[..., 0] = ((hsv[..., 0].astype(np.int32) + shift) % 256 + 256) % 256
    return emul_hsv2rgb(hsv, variant if variant == "hsv_trunc" else None)


def emul_chain(img, ops, factors, hue_shift, variant=None):
    """aug_lum_sum_kernel + aug_color_kernel over the four stage slots: 0 brightness, 1 contrast, 2 saturation, 3 hue, -1 none.
    -> (image, [mean used by each contrast stage])"""
    _check(variant)
    img, means = np.asarray(img).copy(), []
    bv = variant if variant == "fused_blend" else None
    lv = variant if variant == "lum_no_round" else None
    for op, f in zip(ops, factors):
        if op == 3:
            img = emul_hue(img, hue_shift, variant)
        elif op >= 0:
            if op == 1:
                means.append(emul_mean(int(emul_lum(img, lv).sum()), img.shape[0] * img.shape[1], variant))
            deg = 0 if op == 0 else (means[-1] if op == 1 else emul_lum(img, lv)[..., None])
            img = emul_blend(deg, img, f, bv)
    return img, means


def chunked(fn, arr, chunk=1 << 20):
    """fn over the first axis of `arr` in pieces (the float64 temporaries of 2^24 pixels would not fit comfortably)"""
    flat = arr.reshape(-1, arr.shape[-1])
    out = np.concatenate([fn(flat[i:i + chunk]) for i in range(0, flat.shape[0], chunk)])
    return out.reshape(arr.shape[:-1] + out.shape[1:])


# ---------------------------------------------------------------------------------------------- inputs
@functools.lru_cache(maxsize=None)
def all_colours():
    """uint8 [4096, 4096, 3]: pixel number i (row-major) is the colour (i >> 16, (i >> 8) & 255, i & 255) — read as RGB or as HSV"""
    i = np.arange(1 << 24, dtype=np.uint32)
    img = np.stack([(i >> 16).astype(np.uint8), ((i >> 8) & 255).astype(np.uint8), (i & 255).astype(np.uint8)], axis=-1).reshape(4096, 4096, 3)
    img.setflags(write=False)
    return img


def colour_index(px):
    px = np.asarray(px).astype(np.int64)
    return (px[..., 0] << 16) | (px[..., 1] << 8) | px[..., 2]


def every_value_pixels(n=256):
    """uint8 [n, 3], n >= 256: every value 0..255 in every channel, no pixel grey for n = 256 (three different permutations)"""
    i = np.arange(n)
    return np.stack([i % 256, (i * 7 + 101) % 256, (255 - i * 3) % 256], axis=-1).astype(np.uint8)


def every_value_image(h=24, w=32):
    return every_value_pixels(h * w).reshape(h, w, 3)


def image_with_lum_sum(h, w, lum_sum, seed):
    """uint8 [h, w, 3] whose luminance sum (emul_lum = Convert.c rgb2l) is exactly `lum_sum`: the 256 pixels of every_value_pixels and
    h * w - 256 grey fillers (a grey pixel's luminance is its value: the three weights add up to 2^16), shuffled."""
    base = every_value_pixels()
    n_fill = h * w - 256
    rest = lum_sum - int(emul_lum(base).sum())
    if n_fill <= 0 or not 0 <= rest <= 255 * n_fill:
        raise ValueError(f"a luminance sum of {lum_sum} is out of reach of {h} x {w} pixels")
    q, r = divmod(rest, n_fill)
    fill = np.full(n_fill, q, np.int64)
    fill[:r] += 1
    px = np.concatenate([base, np.repeat(fill.astype(np.uint8)[:, None], 3, axis=1)])
    img = px[np.random.default_rng(seed).permutation(h * w)].reshape(h, w, 3)
    assert int(emul_lum(img).sum()) == lum_sum
    return img


def resample_pattern(h, w, kind, seed=0):
    """uint8 [h, w, 3] of 0 / 255 with edges in both directions, so that the bicubic lobes overshoot on both sides:
    'checker' cells of 3 x 2 pixels (per channel another phase), 'step' a few straight edges at irregular positions, 'noise' random."""
    y, x = np.mgrid[0:h, 0:w]
    if kind == "checker":
        ch = [((y + c) // 3 + (x + 2 * c) // 2) % 2 for c in range(3)]
    elif kind == "step":
        ch = [((y * 5 + c) // 17 + (x * 3 + 2 * c) // 13) % 2 for c in range(3)]
    elif kind == "noise":
        rng = np.random.default_rng(seed)
        return rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    else:
        raise ValueError(kind)
    return (np.stack(ch, axis=-1) * 255).astype(np.uint8)


def fuse_candidates(lo=0.7, hi=1.3, qmax=64, ulps=2):
    """the float32 values within `ulps` of a fraction p / q, q <= qmax, inside [lo, hi] (float32 bounds)"""
    lo, hi = F32(lo), F32(hi)
    out = set()
    for q in range(1, qmax + 1):
        for p in range(int(np.floor(float(lo) * q)), int(np.ceil(float(hi) * q)) + 1):
            c = F32(p / q)
            up = dn = c
            out.add(float(c))
            for _ in range(ulps):
                up, dn = np.nextafter(up, F32(2)), np.nextafter(dn, F32(0))
                out.add(float(up)); out.add(float(dn))
    return np.array(sorted(v for v in out if lo <= F32(v) <= hi), F32)


def fuse_changed(alpha):
    """bool [256 deg, 256 value]: the pairs whose blend_u8 output a fused multiply-add would change at this factor"""
    deg, val = np.mgrid[0:256, 0:256]
    return emul_blend(deg, val, alpha) != emul_blend(deg, val, alpha, "fused_blend")


@functools.lru_cache(maxsize=None)
def fuse_search(lo=0.7, hi=1.3, qmax=64, ulps=2):
    """(factors float32 [n], changed pairs per factor and degenerate value int32 [n, 256]) over fuse_candidates"""
    cand = fuse_candidates(lo, hi, qmax, ulps)
    return cand, np.stack([fuse_changed(a).sum(axis=1).astype(np.int32) for a in cand])


def fuse_ranked(lo=0.7, hi=1.3, qmax=64, ulps=2):
    """[(factor, changed pairs of the 65 536)] in descending order of the count"""
    cand, per_deg = fuse_search(lo, hi, qmax, ulps)
    tot = per_deg.sum(axis=1)
    order = np.argsort(-tot, kind="stable")
    return [(float(cand[i]), int(tot[i])) for i in order]


# ---------------------------------------------------------------------------------------------- the cases both test files run
# Fuse-sensitive factors, from fuse_ranked() (tests/test_augment_emul_host.py asserts that the search still puts them first on their side of 1
# and prints the counts).  A factor drawn uniformly from [0.7, 1.3] is almost never one of them.
FUSE_BELOW = (0.9999998807907104, 0.7499999403953552, 0.9090909361839294)
FUSE_ABOVE = (1.0000001192092896, 1.2000000476837158, 1.0909091234207153, 1.2499998807907104)

HUE_SHIFTS = (0, 1, -1, 25, -25, 128)                    # int(hf * 255) of hf in [-0.1, 0.1] spans -25..25; 128 wraps every hue
SATURATION_FACTORS = (0.7, 1.0, 1.3) + FUSE_BELOW[:2] + FUSE_ABOVE[:2]
BRIGHTNESS_FACTORS = (0.7, 1.3)


def _half(h, w, k):
    assert (h * w) % 2 == 0
    return h * w * k + h * w // 2


def contrast_cases():
    """The batch of the contrast test: [dict(name, img, op, factor, hue_shift)].  Means exactly k + 0.5, exactly k and the largest sum
    below k + 0.5 for k = 1, 127, 254; contrast in each stage slot; contrast after brightness and after hue; a pixel count that is no
    multiple of 64; an image above 1024 x 256 pixels; all black and all white; fuse-sensitive factors on both sides of 1."""
    B, A = FUSE_BELOW, FUSE_ABOVE
    cases = []

    def add(name, img, op, factor, hue_shift=0):
        cases.append(dict(name=name, img=img, op=list(op), factor=[float(F32(f)) for f in factor], hue_shift=hue_shift))
    slot = lambda s, f: ([1 if j == s else -1 for j in range(4)], [f if j == s else 0.0 for j in range(4)])   # noqa: E731
    sizes = {1: (200, 180), 127: (37, 30), 254: (300, 250)}
    plan = {1: ((0, 0.7), (1, A[1]), (2, B[1])), 127: ((3, A[0]), (0, B[0]), (1, 1.3)), 254: ((2, B[2]), (3, 0.7), (0, A[2]))}
    for k, (h, w) in sizes.items():
        for (what, lum_sum), (s, f) in zip((("half", _half(h, w, k)), ("exact", h * w * k), ("below", _half(h, w, k) - 1)), plan[k]):
            add(f"k{k}_{what}", image_with_lum_sum(h, w, lum_sum, 7 * k + s), *slot(s, f))
    add("large_below", image_with_lum_sum(520, 512, _half(520, 512, 127) - 1, 5), *slot(1, B[0]))
    add("large_half", image_with_lum_sum(513, 520, _half(513, 520, 100), 6), *slot(2, A[3]))
    add("black", np.zeros((33, 47, 3), np.uint8), *slot(0, 1.3))
    add("white", np.full((20, 50, 3), 255, np.uint8), *slot(3, 0.7))
    add("after_brightness", image_with_lum_sum(90, 111, 90 * 111 * 140 + 17, 8), [0, 1, -1, -1], [0.7, A[1], 0.0, 0.0])
    add("after_hue", every_value_pixels(61 * 67).reshape(61, 67, 3), [-1, 3, -1, 1], [0.0, 0.0, 0.0, B[1]], 25)
    add("after_two", every_value_pixels(70 * 45).reshape(70, 45, 3), [2, 0, 1, 3], [1.3, 1.3, 0.7, 0.0], -25)
    return cases


# (H, W) -> (rh, rw): both passes of one image cover a size pair of the issue's table (source -> target along one axis)
RESIZE_CASES = (
    ("500to448", (375, 500), (336, 448), "checker"),      # horizontal 500 -> 448: 7 taps; vertical 375 -> 336
    ("upscale", (375, 500), (576, 768), "step"),          # 500 -> 768 and 375 -> 576
    ("strong_upscale", (120, 160), (576, 768), "checker"),   # 160 -> 768
    ("identity", (500, 500), (500, 500), "noise"),        # the coefficients must reproduce the copy Pillow makes
    ("identity_h", (500, 375), (448, 375), "step"),       # identity in one pass only
    ("97to41", (97, 60), (41, 25), "step"),               # vertical 97 -> 41: 11 taps
    ("small", (3, 5), (7, 3), "noise"),                   # vertical 3 -> 7, horizontal 5 -> 3
    ("one_wide", (40, 1), (17, 4), "checker"),            # every tap of the horizontal pass on the one source pixel
    ("one_high", (1, 30), (3, 13), "step"),
    ("tall", (333, 41), (500, 62), "noise"),
)


def resize_image(case):
    name, (h, w), _, kind = case
    return resample_pattern(h, w, kind, seed=sum(map(ord, name)))


FINISH_CROPS = (40, 64)


def finish_cases(crop):
    """[dict(name, img, flip, img_top, img_left, cont_top, cont_left, ch, cw)]: larger than the crop in both dimensions (offsets 0 / maximal),
    smaller in both (container offsets 0 / maximal), the two mixed placements; each with flip 0 and 1."""
    rng = np.random.default_rng(crop)
    shapes = (("larger", (70, 83)), ("smaller", (23, 31)), ("wide", (30, 90)), ("tall", (90, 30)))
    cases = []
    for name, (h, w) in shapes:
        img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        ch, cw = min(crop, h), min(crop, w)
        for at_max in ((0, 0), (1, 1)) if name in ("larger", "smaller") else ((0, 1), (1, 0)):
            it, ct = ((h - ch) * at_max[0], 0) if h > crop else (0, (crop - ch) * at_max[0])
            il, cl = ((w - cw) * at_max[1], 0) if w > crop else (0, (crop - cw) * at_max[1])
            for flip in (0, 1):
                cases.append(dict(name=f"{name}_{at_max[0]}{at_max[1]}_flip{flip}", img=img, flip=flip, img_top=it, img_left=il,
                                  cont_top=ct, cont_left=cl, ch=ch, cw=cw))
    return cases


def distinct_lut():
    """lut[c][v] = 1000 c + v: exact in float32 and different at every (channel, value), so a wrong channel or value shows"""
    return (1000.0 * np.arange(3)[:, None] + np.arange(256)[None, :]).astype(F32)


# ---------------------------------------------------------------------------------------------- the reference: Pillow, as wseg_amd/data.py calls it
def pil_rgb2hsv(img):
    return np.asarray(PIL.Image.fromarray(np.ascontiguousarray(img)).convert("HSV"))


def pil_hsv2rgb(hsv):
    return np.asarray(PIL.Image.fromarray(np.ascontiguousarray(hsv), "HSV").convert("RGB"))


def pil_hue(img, shift, hsv=None):
    """data.ColorJitter's hue op with int(hf * 255) = shift (`hsv`: the HSV image where the caller already has it)"""
    hsv = np.array(pil_rgb2hsv(img) if hsv is None else hsv)
    hsv[..., 0] = (hsv[..., 0].astype(np.int16) + shift) % 256
    return pil_hsv2rgb(hsv)


def pil_op(img, op, factor, hue_shift):
    im = PIL.Image.fromarray(np.ascontiguousarray(img))
    if op == 0:
        return np.asarray(PIL.ImageEnhance.Brightness(im).enhance(factor))
    if op == 1:
        return np.asarray(PIL.ImageEnhance.Contrast(im).enhance(factor))
    if op == 2:
        return np.asarray(PIL.ImageEnhance.Color(im).enhance(factor))
    return pil_hue(img, hue_shift)


def pil_chain(img, ops, factors, hue_shift):
    for op, f in zip(ops, factors):
        if op >= 0:
            img = pil_op(img, op, f, hue_shift)
    return np.asarray(img)


def pil_lum(img):
    return np.asarray(PIL.Image.fromarray(np.ascontiguousarray(img)).convert("L"))


def pil_resize(img, rw, rh):
    return np.asarray(PIL.Image.fromarray(np.ascontiguousarray(img)).resize((rw, rh), resample=PIL.Image.Resampling.BICUBIC))


class _Draws:
    """stands in for the `random` module inside wseg_amd.data: RandomCrop's two randrange draws (width first) come from the case"""

    def __init__(self, values):
        self.values = list(values)

    def randrange(self, n):
        v = self.values.pop(0)
        assert 0 <= v < n, (v, n)
        return v


def host_finish(img, c, crop, aff):
    """The tail of the two host chains run through the classes of wseg_amd/data.py themselves (production normalisation), with the
    crop's draws prescribed by the case -> float32 [3, crop, crop]"""
    from wseg_amd import data as wdata
    from wseg_amd.resnet38_contrast import Normalize
    h, w = img.shape[:2]
    draws = _Draws([c["img_left"] if w > crop else c["cont_left"], c["img_top"] if h > crop else c["cont_top"]])
    keep, wdata.random = wdata.random, draws
    try:
        if aff:
            x = Normalize()(wdata.RandomCrop(crop)(np.asarray(img)))
            x = np.fliplr(x).copy() if c["flip"] else x
        else:
            x = np.asarray(PIL.Image.fromarray(img).transpose(PIL.Image.Transpose.FLIP_LEFT_RIGHT)) if c["flip"] else img
            x = wdata.RandomCrop(crop)(Normalize()(x))
    finally:
        wdata.random = keep
    assert not draws.values
    return np.ascontiguousarray(wdata.HWC_to_CHW(x))


def ref_finish(img, c, crop, lut, aff):
    """The tail of the two host chains as wseg_amd/data.py slices it, on a 256-entry table per channel -> float32 [3, crop, crop].
    Contrast chain (aff=False): flip the image, normalise it, RandomCrop into a ZERO container.  AffinityNet chain (aff=True): RandomCrop
    the raw image into a zero container, normalise the container (padding = lut[c][0]), flip the container."""
    def norm(a): return np.stack([lut[k][a[..., k]] for k in range(3)], axis=-1).astype(F32)
    sl_c = (slice(c["cont_top"], c["cont_top"] + c["ch"]), slice(c["cont_left"], c["cont_left"] + c["cw"]))
    sl_i = (slice(c["img_top"], c["img_top"] + c["ch"]), slice(c["img_left"], c["img_left"] + c["cw"]))
    if aff:
        cont = np.zeros((crop, crop, 3), np.uint8)
        cont[sl_c] = img[sl_i]
        cont = norm(cont)
        if c["flip"]:
            cont = np.fliplr(cont)
    else:
        src = norm(img[:, ::-1] if c["flip"] else img)
        cont = np.zeros((crop, crop, 3), F32)
        cont[sl_c] = src[sl_i]
    return np.ascontiguousarray(np.transpose(cont, (2, 0, 1)))
