"""Shared by tests/test_seg_data_host.py and tests/test_gpu_seg_data.py: a plain per-sample restatement of the DeepLab-v1 training data chain
(segmentation/lib/datasets/BaseDataset.py:88-98 with lib/datasets/transform.py), written from the chain's definition and never from
wseg_amd/data.py or csrc/seg_data.hip, and the inputs the tests feed it.  TEST INFRASTRUCTURE, no tests here.

  chain            RandomHSV -> np.flip(axis=1) -> rescale (image PIL bicubic, label nearest) -> (x / 255 - mean) / std in float32 -> paste into
                   a +0.0 / 255 container -> CHW, with GIVEN draws `p` instead of `random`
  label            the direct float64 index formula min(floor(o * (1 / s)), n - 1) per output position: no tables, a flip of the ARRAY
  hsv_forward      the integer formula with the two division tables, pixel by pixel in plain Python integers (small images)
  hsv_forward_exact  S = 255 diff / v and H = 30 hn / diff as exact rationals, rounded half to even in integer arithmetic (all 2^24 colours)

cv2 is not available: the HSV arithmetic and Pillow's bicubic are this project's statement of the chain, not the reference's bytes."""
import math

import numpy as np
import PIL.Image

MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
SECTORS = ((1, 3, 0), (1, 0, 2), (3, 0, 1), (0, 2, 1), (0, 1, 3), (2, 1, 0))


def image(h, w, seed):
    rng = np.random.default_rng(seed)
    low = rng.integers(0, 256, (h // 6 + 1, w // 6 + 1, 3), dtype=np.uint8)
    img = np.asarray(PIL.Image.fromarray(low).resize((w, h), PIL.Image.Resampling.BICUBIC)).copy()
    img[::7, ::5] = rng.integers(0, 256, img[::7, ::5].shape, dtype=np.uint8)        # some high-frequency content
    return img


def label_map(h, w, seed, block=3):
    """uint8 [h, w] holding every value of 0 .. 20 and 255, constant on small blocks (no multiple of any scale's step)"""
    rng = np.random.default_rng(seed)
    vals = np.array(list(range(21)) + [255], np.uint8)
    low = vals[rng.integers(0, 22, (h // block + 1, w // block + 1))]
    lab = np.kron(low, np.ones((block, block), np.uint8))[:h, :w].copy()
    flat = lab.reshape(-1)
    pos = rng.permutation(flat.size)[:22]
    if flat.size >= 22:
        flat[pos] = vals                                     # every value occurs
    return lab


def all_colours():
    """uint8 [4096, 4096, 3]: every RGB colour once"""
    c = np.arange(1 << 24, dtype=np.uint32)
    return np.stack([(c >> 16) & 255, (c >> 8) & 255, c & 255], -1).astype(np.uint8).reshape(4096, 4096, 3)


def _rdiv_half_even(a, b):
    """round(a / b) half to even for integer arrays, b > 0; 0 where b == 0"""
    a, b = a.astype(np.int64), b.astype(np.int64)
    safe = np.where(b == 0, 1, b)
    q, r = np.divmod(a, safe)                                # floor division: 0 <= r < b
    up = (2 * r > safe) | ((2 * r == safe) & (q % 2 == 1))
    return np.where(b == 0, 0, q + up)


def _hue_numerator(r, g, b, v, diff):
    return np.where(v == r, g - b, np.where(v == g, b - r + 2 * diff, r - g + 4 * diff))


def hsv_forward_exact(rgb):
    """(h, s, v) int64 of uint8 [..., 3]: the defining formulas H = 180 hn / (6 diff) and S = 255 diff / v rounded half to even from the
    exact rationals; a negative h wraps by 180"""
    c = np.asarray(rgb).astype(np.int64)
    r, g, b = c[..., 0], c[..., 1], c[..., 2]
    v = c.max(-1)
    diff = v - c.min(-1)
    s = _rdiv_half_even(255 * diff, v)
    h = _rdiv_half_even(30 * _hue_numerator(r, g, b, v, diff), diff)
    return np.where(h < 0, h + 180, h), s, v


def hsv_forward(rgb):
    """(h, s, v) of a small uint8 [H, W, 3] image: the table formula in Python integers, pixel by pixel"""
    sdiv = [0] + [int(round(255 * 4096 / i)) for i in range(1, 256)]
    hdiv = [0] + [int(round(180 * 4096 / (6 * i))) for i in range(1, 256)]
    rgb = np.asarray(rgb)
    out = np.zeros(rgb.shape, np.int64)
    for idx in np.ndindex(rgb.shape[:-1]):
        r, g, b = (int(x) for x in rgb[idx])
        v = max(r, g, b)
        diff = v - min(r, g, b)
        s = (diff * sdiv[v] + 2048) >> 12
        if v == r:
            hn = g - b
        elif v == g:
            hn = b - r + 2 * diff
        else:
            hn = r - g + 4 * diff
        h = (hn * hdiv[diff] + 2048) >> 12                    # Python's >> is arithmetic
        if h < 0:
            h += 180
        out[idx] = (h, s, v)
    return out[..., 0], out[..., 1], out[..., 2]


def hsv_inverse(h, s, v):
    """uint8 [..., 3] RGB: float32 throughout, one rounding per operation, sector by sector with masks"""
    f32 = np.float32
    h, s, v = (np.asarray(a, np.int64) for a in (h, s, v))
    S = s.astype(f32) / f32(255)
    V = v.astype(f32) / f32(255)
    hh = h.astype(f32) * (f32(6) / f32(180))
    hh = np.where(hh >= f32(6), hh - f32(6), hh)               # (h < 180 never gets here)
    sec = np.floor(hh)
    f = hh - sec
    p0 = V
    p1 = V * (f32(1) - S)
    p2 = V * (f32(1) - S * f)
    p3 = V * (f32(1) - S * (f32(1) - f))
    tab = (p0, p1, p2, p3)
    b, g, r = np.zeros_like(V), np.zeros_like(V), np.zeros_like(V)
    for k, (ib, ig, ir) in enumerate(SECTORS):
        m = sec == k
        b, g, r = np.where(m, tab[ib], b), np.where(m, tab[ig], g), np.where(m, tab[ir], r)
    grey = s == 0
    r, g, b = np.where(grey, V, r), np.where(grey, V, g), np.where(grey, V, b)
    out = np.stack([r, g, b], -1)
    assert out.dtype == np.float32
    return np.clip(np.rint(out * f32(255)), 0, 255).astype(np.uint8)


def hsv_jitter(img, dh, ds, dv):
    h, s, v = hsv_forward(img)
    h = (h + dh) % 180
    s = np.clip(s + ds, 0, 255)
    v = np.clip(v + dv, 0, 255)
    return hsv_inverse(h, s, v)


def nearest(label, rh, rw, scale):
    """the label rescaled to rh x rw by the direct formula, one output position at a time"""
    H, W = label.shape
    inv = 1.0 / scale
    out = np.empty((rh, rw), label.dtype)
    for y in range(rh):
        sy = min(int(math.floor(y * inv)), H - 1)
        for x in range(rw):
            out[y, x] = label[sy, min(int(math.floor(x * inv)), W - 1)]
    return out


def paste(img_f32, label, p, crop):
    ct, cl, it, il, ch, cw = (p[k] for k in ("cont_top", "cont_left", "img_top", "img_left", "ch", "cw"))
    cont = np.zeros((crop, crop, 3), np.float32)
    cont[ct:ct + ch, cl:cl + cw] = img_f32[it:it + ch, il:il + cw]
    seg = np.full((crop, crop), 255, np.uint8)
    seg[ct:ct + ch, cl:cl + cw] = label[it:it + ch, il:il + cw]
    return cont, seg


def label_chain(label, p, crop):
    """uint8 [crop, crop]: flip the array, rescale by the direct formula, paste into 255"""
    lab = np.flip(label, axis=1) if p["flip"] else label
    lab = nearest(lab, p["rh"], p["rw"], p["scale"])
    return paste(np.zeros(lab.shape + (3,), np.float32), lab, p, crop)[1]


def chain(img, label, p, crop):
    """(img float32 [3, crop, crop], label uint8 [crop, crop]) of one sample under the draws `p`"""
    x = hsv_jitter(img, p["dh"], p["ds"], p["dv"])
    if p["flip"]:
        x = np.flip(x, axis=1)
    x = np.asarray(PIL.Image.fromarray(np.ascontiguousarray(x)).resize((p["rw"], p["rh"]), PIL.Image.Resampling.BICUBIC))
    x = x.astype(np.float32)
    for c in range(3):
        x[..., c] = (x[..., c] / np.float32(255) - np.float32(MEAN[c])) / np.float32(STD[c])
    lab = np.flip(label, axis=1) if p["flip"] else label
    lab = nearest(lab, p["rh"], p["rw"], p["scale"])
    cont, seg = paste(x, lab, p, crop)
    return np.ascontiguousarray(cont.transpose(2, 0, 1)), seg
