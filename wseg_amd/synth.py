"""Deterministic synthetic weights, images and labels for the hot path.

The reference needs the ImageNet ResNet-38 `.params` file (contrast_train.py:98-106) and the
VOC images; neither exists offline, so every test / benchmark regenerates *procedural*
values.  Every tensor is a closed-form integer hash of (name, seed, element index), computed
with exact int64 tensor arithmetic — bit-identical on CPU and on the GPU, any torch version.
"""
import zlib
from collections import OrderedDict

import torch

from .arch import AFF_HEAD_CONVS, state_dict_spec


def hash_uniform(key, n, device="cpu"):
    """float32 [n], uniform in [0,1) with 24 random bits: two rounds of a 32-bit
    xorshift-multiply mix of (index + key)."""
    h = torch.arange(n, dtype=torch.int64, device=device)
    h += int(key) & 0xFFFFFFFF
    h &= 0xFFFFFFFF
    for _ in range(2):
        h ^= (h >> 16)
        h *= 0x45D9F3B
        h &= 0xFFFFFFFF
    h ^= (h >> 16)
    h >>= 8
    return h.to(torch.float32).mul_(2.0 ** -24)


def _mix32(h):
    """hash_uniform's mix of an int64 tensor of 32-bit values, in place: two xorshift-multiply rounds and a final xorshift"""
    for _ in range(2):
        h ^= (h >> 16)
        h *= 0x45D9F3B
        h &= 0xFFFFFFFF
    h ^= (h >> 16)
    return h


def dropout_keep(M, C, key, p=0.5, device="cpu"):
    """bool [M, C]: the keep mask of nn.Dropout(p) as csrc/seg_head.hip's bn_relu_drop computes it from a counter, bit for bit: with i = row * C + col
    (M * C < 2^32), u = mix32((mix32(i) + key) mod 2^32) >> 8, keep iff u * 2^-24 >= p (in float32).  The key enters BETWEEN two mixes: added to
    the counter itself, consecutive keys give one mask shifted by an element."""
    if M * C >= 1 << 32:
        raise ValueError(f"dropout_keep: M * C = {M * C} passes the 32-bit counter")
    h = _mix32(torch.arange(M * C, dtype=torch.int64, device=device))
    h += int(key) & 0xFFFFFFFF
    h &= 0xFFFFFFFF
    h = _mix32(h) >> 8
    return (h.to(torch.float32).mul_(2.0 ** -24) >= torch.tensor(p, dtype=torch.float32, device=device)).view(M, C)


def dropout_key(seed, step):
    """The 32-bit key of training step `step` under `seed` for dropout_keep (the DeepLab head's dropout1)"""
    return (_key("seg.dropout1", seed) + 0x85EBCA6B * (int(step) + 1)) & 0xFFFFFFFF


def _key(name, seed):
    return (zlib.crc32(name.encode()) + 0x9E3779B1 * (seed + 1)) & 0xFFFFFFFF


def _uniform(name, seed, shape, lo, hi, device="cpu"):
    n = 1
    for s in shape:
        n *= s
    u = hash_uniform(_key(name, seed), n, device)
    return u.mul_(float(hi - lo)).add_(float(lo)).reshape(shape)


def procedural_tensor(name, shape, seed=0, device="cpu"):
    """Value of state_dict entry `name` (float32, or int64 for num_batches_tracked)."""
    if name.endswith("num_batches_tracked"):
        return torch.zeros((), dtype=torch.int64, device=device)
    if name.endswith("running_var"):
        return _uniform(name, seed, shape, 0.5, 1.5, device)
    if name.endswith("running_mean"):
        return _uniform(name, seed, shape, -0.2, 0.2, device)
    if ".bn" in name or name.startswith("bn7"):
        if name.endswith(".weight"):
            return _uniform(name, seed, shape, 0.5, 1.5, device)
        return _uniform(name, seed, shape, -0.2, 0.2, device)
    # conv weights: kaiming-like; the closing conv of every residual branch is damped so the
    # activation scale stays O(1..30) through the 17 pre-activation blocks.
    cout, cin, kh, kw = shape
    fan_in = cin * kh * kw
    gain = 1.0
    if name.endswith("conv_branch2b1.weight") and not name.startswith(("b6.", "b7.")):
        gain = 0.5
    if name.endswith("conv_branch2b2.weight"):
        gain = 0.5
    if name.startswith("f9."):
        gain = 2.0
    if name.startswith("fc8."):
        gain = 0.03                           # keeps the GAP logits O(1): BCE not saturated
    a = gain * (6.0 / fan_in) ** 0.5          # uniform(-a,a) has std gain*sqrt(2/fan_in)
    return _uniform(name, seed, shape, -a, a, device)


def procedural_state_dict(seed=0, device="cpu"):
    sd = OrderedDict()
    for k, shape in state_dict_spec().items():
        sd[k] = procedural_tensor(k, shape, seed, device)
    return sd


def synthetic_images(n, size, seed=0, device="cpu"):
    """float32 [n,3,H,W], zero mean / unit variance, bell-shaped (sum of 3 uniforms) — the
    statistics of a normalised VOC crop (contrast_train.py:64-75, resnet38d.py:104-118)."""
    h, w = (size, size) if isinstance(size, int) else size
    u = sum(_uniform(f"img{j}", seed, (n, 3, h, w), -1.0, 1.0, device) for j in range(3))
    return u


def synthetic_labels(n, seed=0, device="cpu"):
    """float32 [n,20] multi-hot with 1-3 positives (VOC histogram: SURVEY.md §8d)."""
    u = _uniform("labels", seed, (n, 4), 0.0, 1.0).tolist()
    lab = torch.zeros(n, 20)
    for i in range(n):
        k = 1 if u[i][0] < 0.62 else (2 if u[i][0] < 0.91 else 3)
        first = int(u[i][1] * 20)
        for j in range(k):
            lab[i, (first + j * (1 + int(u[i][2 + (j > 1)] * 6))) % 20] = 1.0
    return lab.to(device)


DROPOUT_SITES = OrderedDict([("b6.dropout_2b1", (512, 0.3)), ("b6.dropout_2b2", (1024, 0.3)),
                             ("b7.dropout_2b1", (1024, 0.5)), ("b7.dropout_2b2", (2048, 0.5)),
                             ("dropout7", (4096, 0.5))])


def synthetic_dropout_masks(n, seed=0, device="cpu"):
    """Per-(n,channel) Dropout2d scale factors (0 or 1/(1-p)) for the five Dropout2d sites
    (resnet38d.py:64,68 with p=0.3 / 0.5; resnet38_contrast.py:14 with p=0.5)."""
    out = OrderedDict()
    for k, (c, p) in DROPOUT_SITES.items():
        keep = (_uniform("mask." + k, seed, (n, c), 0.0, 1.0, device) >= p).float() / (1.0 - p)
        out[k] = keep
    return out


AFF_HEAD_GAIN = {"f8_3": 1.0, "f8_4": 1.0, "f8_5": 1.0, "f9": 0.05}


def procedural_aff_state_dict(seed=0, device="cpu"):
    """State dict of the AffinityNet (network/resnet38_aff.py): the backbone entries of procedural_state_dict(seed), then the four
    head convs, uniform with std gain*sqrt(2/fan_in) under keys of their own ("aff." + name: distinct from the contrast head's values).
    f9's small gain keeps the mean |f_i - f_j| of its 448 ELU features O(0.1), so exp(-.)^beta spreads over (0, 1) instead of vanishing."""
    sd = OrderedDict()
    for k, shape in state_dict_spec(AFF_HEAD_CONVS).items():
        head = k.split(".")[0]
        if head in AFF_HEAD_CONVS:
            cout, cin, kh, kw = shape
            a = AFF_HEAD_GAIN[head] * (6.0 / (cin * kh * kw)) ** 0.5
            sd[k] = _uniform("aff." + k, seed, shape, -a, a, device)
        else:
            sd[k] = procedural_tensor(k, shape, seed, device)
    return sd


SEG_HEAD_GAIN = {"conv_fov": 1.0, "conv_fov2": 1.0, "cls_conv": 1.0}
# Added to cls_conv's bias (seed 0's values; other seeds take them as they are).  With random weights the part of each logit that does not depend
# on the pixel — a random projection of the features' channel MEANS — is about five times the spread over the pixels, so one class would win
# every synthetic image and a label-map comparison would check nothing.  These constants are minus that part as the reference net computes it
# (scripts/make_seg_goldens.py: the per-class spatial mean of the mean logits, averaged over its three cases, rounded to 0.5); what is left
# of it on one image is as large as the spatial part, and several classes share the map.
SEG_CLS_BIAS_CENTRE = (10.0, 7.0, 4.0, -8.5, 3.0, 0.5, -4.5, -7.0, 2.0, -0.5, 0.0, -8.0, 2.0, 3.0, -1.0, 3.0, 5.5, -6.5, -12.5, -0.5, 6.0)


def procedural_seg_state_dict(seed=0, device="cpu"):
    """State dict of the DeepLab-v1 net (segmentation/lib/net/deeplabv1.py over resnet38d): the backbone entries of procedural_state_dict(seed)
    under `backbone.`, then the head under keys of its own ("seg." + name).  The head's two BatchNorms carry statistics as non-trivial as the
    backbone's (weight, variance in [0.5, 1.5], bias, mean in [-0.2, 0.2]), cls_conv a bias in [-1, 1] plus SEG_CLS_BIAS_CENTRE, so that
    the arg-max map of a synthetic image holds several classes."""
    from .arch import SEG_BACKBONE_PREFIX, seg_state_dict_spec
    sd = OrderedDict()
    for k, shape in seg_state_dict_spec().items():
        if k.startswith(SEG_BACKBONE_PREFIX):
            sd[k] = procedural_tensor(k[len(SEG_BACKBONE_PREFIX):], shape, seed, device)
            continue
        head, leaf = k.split(".")
        if leaf == "num_batches_tracked":
            sd[k] = torch.zeros((), dtype=torch.int64, device=device)
        elif head.startswith("bn_"):
            lo, hi = (0.5, 1.5) if leaf in ("weight", "running_var") else (-0.2, 0.2)
            sd[k] = _uniform("seg." + k, seed, shape, lo, hi, device)
        elif leaf == "bias":
            sd[k] = _uniform("seg." + k, seed, shape, -1.0, 1.0, device) + torch.tensor(SEG_CLS_BIAS_CENTRE, dtype=torch.float32, device=device)
        else:
            cout, cin, kh, kw = shape
            a = SEG_HEAD_GAIN[head] * (6.0 / (cin * kh * kw)) ** 0.5
            sd[k] = _uniform("seg." + k, seed, shape, -a, a, device)
    return sd


def synthetic_cam_dict(H, W, classes, seed=0, device="cpu"):
    """{class: float32 [H, W]} — what contrast_infer.py:82-90 writes per image (per-class normalised CAMs in [0, 1]), in closed form: per
    class one anisotropic Gaussian bump (centre / widths from the hash) plus a small hash texture, scaled to a maximum of 1."""
    out = {}
    ys = torch.arange(H, dtype=torch.float32, device=device).view(H, 1)
    xs = torch.arange(W, dtype=torch.float32, device=device).view(1, W)
    for c in classes:
        u = _uniform(f"cam{c}", seed, (4,), 0.0, 1.0).tolist()
        cy, cx = u[0] * H, u[1] * W
        sy, sx = (0.15 + 0.35 * u[2]) * H, (0.15 + 0.35 * u[3]) * W
        m = torch.exp(-(((ys - cy) / sy) ** 2 + ((xs - cx) / sx) ** 2) * 0.5)
        m = m + 0.05 * _uniform(f"camtex{c}", seed, (H, W), 0.0, 1.0, device)
        out[int(c)] = (m / m.max()).to(torch.float32)
    return out


def synthetic_rgb_image(H, W, seed=0):
    """uint8 [H, W, 3] (CPU): a piecewise-smooth picture — four flat-coloured ellipses (centres / colours from the hash, semi-axes
    0.35 H x 0.35 W, later ones on top) over black, a horizontal ramp of 20 levels and +-12 levels of hash texture.  N(0, 1) noise
    (synthetic_images) makes a bilateral kernel degenerate: no two pixels are alike.  float64 arithmetic, rounded half to even."""
    u = hash_uniform(1234 + seed, H * W * 3).double().reshape(H, W, 3)
    r = hash_uniform(99 + seed, 40).double()
    yy = torch.arange(H, dtype=torch.float64).view(H, 1)
    xx = torch.arange(W, dtype=torch.float64).view(1, W)
    img = torch.zeros(H, W, 3, dtype=torch.float64)
    for k in range(4):
        cy, cx = r[5 * k] * H, r[5 * k + 1] * W
        inside = ((yy - cy) / (0.35 * H)) ** 2 + ((xx - cx) / (0.35 * W)) ** 2 < 1
        img[inside] = r[5 * k + 2:5 * k + 5] * 255
    img += (20 * xx / W).unsqueeze(-1) + 24 * (u - 0.5)
    return img.round().clamp_(0, 255).to(torch.uint8)


def synthetic_aff_label_map(h, w, seed=0, classes=(3, 11), block=3, p_bg=0.35, p_ignore=0.15):
    """uint8 [h, w] AffinityNet label map (0 background, a class number, 255 ignore) in block x block patches, so that pairs of all three
    kinds (background, foreground, negative) and ignored pixels occur at every radius."""
    bh, bw = -(-h // block), -(-w // block)
    u = _uniform("afflab", seed, (bh, bw), 0.0, 1.0)
    p_cls = (1.0 - p_bg - p_ignore) / len(classes)
    coarse = torch.full((bh, bw), 255, dtype=torch.uint8)
    coarse[u < p_bg] = 0
    for i, c in enumerate(classes):
        coarse[(u >= p_bg + i * p_cls) & (u < p_bg + (i + 1) * p_cls)] = c
    return coarse.repeat_interleave(block, 0).repeat_interleave(block, 1)[:h, :w].contiguous()
