"""Shared by tests/test_aff_data_host.py and tests/test_gpu_aff_data.py: the literal dense restatement of the AffinityNet label path
(voc12/data.py:233-258 under the transforms of aff_train.py:39-60) and the inputs the tests feed it.

`dense_rule` does what the reference does, with given draws instead of `random`: a 42-channel zero container, the pasted rectangle,
np.fliplr, reshape-mean over 8 x 8 in `dtype`, the label rule.  In float32 it is the yardstick of the host chain; in float64 it is the
reference of the device kernel.

Quantised scores are multiples of 2^-12 in [0, 1]: a sum of 64 of them is a multiple of 2^-12 below 2^7, 19 bits, exact in float32 in any
order — so every order of summation, numpy's pairwise one and the kernel's, gives the same bits as float64."""
import random

import numpy as np
import PIL.Image

Q = 2.0 ** -12
F32_1E5 = float(np.float32(1e-5))       # the threshold the float32 comparison of voc12/data.py:251 applies


def dense_rule(la, ha, p, crop, dtype):
    """(label uint8 [crop/8, crop/8], pooled [crop/8, crop/8, 42] in dtype) of two dense [21, H, W] stacks under the draws `p`."""
    stack = np.transpose(np.array(list(la) + list(ha)), (1, 2, 0)).astype(dtype)
    cont = np.zeros((crop, crop, 42), dtype)
    ct, cl, it, il, ch, cw = (p[k] for k in ("cont_top", "cont_left", "img_top", "img_left", "ch", "cw"))
    cont[ct:ct + ch, cl:cl + cw] = stack[it:it + ch, il:il + cw]
    if p["flip"]:
        cont = np.fliplr(cont)
    pooled = cont.reshape(crop // 8, 8, crop // 8, 8, 42).mean(axis=(1, 3))
    assert pooled.dtype == dtype
    no_score = np.max(pooled, -1) < (np.float32(1e-5) if dtype == np.float32 else F32_1E5)
    l_la = np.argmax(pooled[..., :21], axis=-1).astype(np.uint8)
    l_ha = np.argmax(pooled[..., 21:], axis=-1).astype(np.uint8)
    label = l_la.copy()
    label[l_la == 0] = 255
    label[l_ha == 0] = 0
    label[no_score] = 255
    return label, pooled


def image(h, w, seed):
    rng = np.random.default_rng(seed)
    low = rng.integers(0, 256, (h // 6 + 1, w // 6 + 1, 3), dtype=np.uint8)
    img = np.asarray(PIL.Image.fromarray(low).resize((w, h), PIL.Image.Resampling.BICUBIC)).copy()
    img[::7, ::5] = rng.integers(0, 256, img[::7, ::5].shape, dtype=np.uint8)        # some high-frequency content
    return img


def quantised_stack(h, w, planes, seed, block=5):
    """float32 [21, h, w]: the given planes hold multiples of 2^-12 in [0, 1], constant on block x block squares (no multiple of the 8 x 8
    windows, so the windows mix values), with a fifth of the squares zero; every other plane is zero."""
    rng = np.random.default_rng(seed)
    s = np.zeros((21, h, w), np.float32)
    for c in planes:
        low = rng.integers(0, 4097, (h // block + 1, w // block + 1)) * (rng.random((h // block + 1, w // block + 1)) > 0.2)
        s[c] = (np.kron(low, np.ones((block, block)))[:h, :w] * Q).astype(np.float32)
        if not s[c].any():
            s[c, 0, 0] = Q
    return s


def float_stack(h, w, planes, seed, bg_shift):
    """float32 [21, h, w], softmax-like and NOT quantised: a softmax over the given planes of smooth random logits (plane 0 shifted by
    bg_shift), zero elsewhere — the shape of the CRF score files."""
    rng = np.random.default_rng(seed)
    logits = []
    for c in planes:
        low = rng.normal(0, 2.0, (h // 9 + 2, w // 9 + 2)).astype(np.float32)
        up = np.asarray(PIL.Image.fromarray(low).resize((w, h), PIL.Image.Resampling.BICUBIC))
        logits.append(up + (bg_shift if c == 0 else 0.0) + rng.normal(0, 0.05, (h, w)))
    e = np.exp(np.stack(logits) - np.max(logits, axis=0))
    s = np.zeros((21, h, w), np.float32)
    s[list(planes)] = (e / e.sum(axis=0)).astype(np.float32)
    return s


def host_chain(img_u8, la, ha, seed, crop):
    """(img, label, generator state afterwards) of the host chain (wseg_amd/data.py) from random.seed(seed)"""
    from wseg_amd import data as wdata
    from wseg_amd.resnet38_contrast import Normalize
    model_stub = type("M", (), {"normalize": Normalize()})()
    random.seed(seed)
    img, label = wdata.aff_apply_transforms(PIL.Image.fromarray(img_u8), la, ha, wdata.aff_train_transform(model_stub, crop))
    return img, label, random.getstate()
