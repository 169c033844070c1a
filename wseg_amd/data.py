"""Host-side VOC12 plumbing for the CLIs: file formats of voc12/data.py:40-121 and the transforms of
contrast_train.py:64-75 / tool/imutils.py:6-67, restated on PIL >= 10 + numpy only (the reference
needs torchvision and the removed PIL.Image.CUBIC).  Not part of the accelerated path: it feeds it.

List files: one line per image, `/JPEGImages/<name>.jpg [/SegmentationClassAug/<name>.png]`; the image
name is characters [-15:-4] of the first field (voc12/data.py:49-55).  Labels: a pickled dict
name -> float32[20] (`cls_labels.npy`, voc12/data.py:40-44) — read by a restricted unpickler that admits numeric numpy
containers only (wseg_amd/safe_npy.py: the file is untrusted input); a plain .npz (names, labels) is accepted too.
"""
import os
import random

import numpy as np
import PIL.Image
import PIL.ImageEnhance
import torch
from torch.utils.data import Dataset

from .safe_npy import load_pickled_npy

IMG_FOLDER_NAME = "JPEGImages"
BICUBIC = PIL.Image.Resampling.BICUBIC


def img_name_of(line):
    """Image name of one list line: `voc12/*.txt` lines are `/JPEGImages/<name>.jpg [/SegmentationClassAug/<name>.png]`
    (voc12/data.py:49-55 takes characters [-15:-4] of the first field); the devkit's `ImageSets/Segmentation/*.txt` lists that
    eval.py:112 reads hold the bare name."""
    first = line.strip().split(' ')[0]
    if '/' in first or first.lower().endswith(('.jpg', '.png')):
        return os.path.splitext(os.path.basename(first))[0]
    return first


def load_img_name_list(dataset_path):
    return [img_name_of(line) for line in open(dataset_path).read().splitlines() if line.strip()]


def get_img_path(img_name, voc12_root):
    return os.path.join(voc12_root, IMG_FOLDER_NAME, img_name + '.jpg')


def load_labels(path, names):
    if path.endswith(".npz"):
        z = np.load(path)
        table = dict(zip([str(n) for n in z["names"]], z["labels"].astype(np.float32)))
    else:
        table = load_pickled_npy(path)
    return [np.asarray(table[n], np.float32) for n in names]


class RandomResizeLong:                                    # tool/imutils.py:6-27
    def __init__(self, min_long, max_long):
        self.min_long, self.max_long = min_long, max_long

    def __call__(self, img):
        target_long = random.randint(self.min_long, self.max_long)
        w, h = img.size
        shape = (int(round(w * target_long / h)), target_long) if w < h else (target_long, int(round(h * target_long / w)))
        return img.resize(shape, resample=BICUBIC)


class RandomHorizontalFlip:
    def __call__(self, img):
        return img.transpose(PIL.Image.Transpose.FLIP_LEFT_RIGHT) if random.random() < 0.5 else img


class ColorJitter:
    """brightness/contrast/saturation factors U(1-a,1+a), hue shift U(-h,h), random order
    (the torchvision transform the reference configures at contrast_train.py:68-69)."""

    def __init__(self, brightness=0.3, contrast=0.3, saturation=0.3, hue=0.1):
        self.b, self.c, self.s, self.h = brightness, contrast, saturation, hue

    def __call__(self, img):
        ops = []
        ops.append(lambda im, f=random.uniform(1 - self.b, 1 + self.b): PIL.ImageEnhance.Brightness(im).enhance(f))
        ops.append(lambda im, f=random.uniform(1 - self.c, 1 + self.c): PIL.ImageEnhance.Contrast(im).enhance(f))
        ops.append(lambda im, f=random.uniform(1 - self.s, 1 + self.s): PIL.ImageEnhance.Color(im).enhance(f))
        hf = random.uniform(-self.h, self.h)

        def hue(im):
            hsv = np.array(im.convert("HSV"))
            hsv[..., 0] = (hsv[..., 0].astype(np.int16) + int(hf * 255)) % 256
            return PIL.Image.fromarray(hsv, "HSV").convert("RGB")
        ops.append(hue)
        random.shuffle(ops)
        for op in ops:
            img = op(img)
        return img


class RandomCrop:                                          # tool/imutils.py:30-67
    def __init__(self, cropsize):
        self.cropsize = cropsize

    def __call__(self, imgarr):
        h, w, c = imgarr.shape
        cs = self.cropsize
        ch, cw = min(cs, h), min(cs, w)
        w_space, h_space = w - cs, h - cs
        if w_space > 0:
            cont_left, img_left = 0, random.randrange(w_space + 1)
        else:
            cont_left, img_left = random.randrange(-w_space + 1), 0
        if h_space > 0:
            cont_top, img_top = 0, random.randrange(h_space + 1)
        else:
            cont_top, img_top = random.randrange(-h_space + 1), 0
        container = np.zeros((cs, cs, c), np.float32)
        container[cont_top:cont_top + ch, cont_left:cont_left + cw] = imgarr[img_top:img_top + ch, img_left:img_left + cw]
        return container


def HWC_to_CHW(img):
    return np.transpose(img, (2, 0, 1))


class VOC12ClsDataset(Dataset):                            # voc12/data.py:58-90
    def __init__(self, img_name_list_path, voc12_root, labels_path, transform=None):
        self.img_name_list = load_img_name_list(img_name_list_path)
        self.voc12_root = voc12_root
        self.transform = transform
        self.label_list = load_labels(labels_path, self.img_name_list)

    def __len__(self):
        return len(self.img_name_list)

    def __getitem__(self, idx):
        name = self.img_name_list[idx]
        img = PIL.Image.open(get_img_path(name, self.voc12_root)).convert("RGB")
        if self.transform:
            for t in self.transform:
                img = t(img)
        return name, img, torch.from_numpy(self.label_list[idx])


class VOC12ImageDataset(Dataset):                          # voc12/data.py:58-74: (name, image) without labels (aff_infer.py:58-62)
    def __init__(self, img_name_list_path, voc12_root, transform=None):
        self.img_name_list = load_img_name_list(img_name_list_path)
        self.voc12_root = voc12_root
        self.transform = transform

    def __len__(self):
        return len(self.img_name_list)

    def __getitem__(self, idx):
        name = self.img_name_list[idx]
        img = PIL.Image.open(get_img_path(name, self.voc12_root)).convert("RGB")
        if self.transform:
            for t in self.transform:
                img = t(img)
        return name, img


class VOC12ClsDatasetMSF(VOC12ClsDataset):                 # voc12/data.py:92-121
    def __init__(self, img_name_list_path, voc12_root, labels_path, scales, inter_transform=None, unit=1):
        super().__init__(img_name_list_path, voc12_root, labels_path, transform=None)
        self.scales, self.unit, self.inter_transform = scales, unit, inter_transform

    def __getitem__(self, idx):
        name, img, label = super().__getitem__(idx)
        rounded = (int(round(img.size[0] / self.unit) * self.unit), int(round(img.size[1] / self.unit) * self.unit))
        out = []
        for s in self.scales:
            s_img = img.resize((round(rounded[0] * s), round(rounded[1] * s)), resample=BICUBIC)
            for t in (self.inter_transform or []):
                s_img = t(s_img)
            out.append(s_img)
            out.append(np.flip(s_img, -1).copy())
        return name, out, label


def train_transform(model, crop_size):
    """contrast_train.py:64-75."""
    return [RandomResizeLong(448, 768), RandomHorizontalFlip(), ColorJitter(0.3, 0.3, 0.3, 0.1), np.asarray,
            model.normalize, RandomCrop(crop_size), HWC_to_CHW, torch.from_numpy]


# ---------------------------------------------------------------------------------------------- AffinityNet training data (aff_train.py:39-60)
class RandomHorizontalFlipArray:                           # tool/imutils.py:141-157: one random BIT, np.fliplr on the HWC array
    def __call__(self, arr):
        return np.fliplr(arr).copy() if bool(random.getrandbits(1)) else arr


class AvgPool2d:
    """tool/imutils.py:130-138 (skimage.measure.block_reduce with np.mean) for an [h, w, c] array whose sides are multiples of ksize, which
    is all the AffinityNet chain feeds it: block means in the array's own dtype (float32 in, float32 out)."""

    def __init__(self, ksize):
        self.ksize = ksize

    def __call__(self, arr):
        h, w, c = arr.shape
        k = self.ksize
        if h % k or w % k:
            raise ValueError(f"AvgPool2d({k}): sides {h} x {w} are no multiples of {k}")
        return arr.reshape(h // k, k, w // k, k, c).mean(axis=(1, 3))


def aff_train_transform(model, crop_size):
    """aff_train.py:39-60: the (joint, image, label) transform lists VOC12AffDataset applies in zip order — ColorJitter on the PIL image,
    np.asarray, joint RandomCrop THEN normalize (on the float32 container: numpy float32 arithmetic, padding = normalize(0)), joint flip
    THEN HWC_to_CHW / AvgPool2d(8).  There is no RandomResizeLong in this chain."""
    if crop_size % 8:
        raise ValueError(f"aff_train_transform: crop {crop_size} is no multiple of 8")
    joint = [None, None, RandomCrop(crop_size), RandomHorizontalFlipArray()]
    img = [ColorJitter(0.3, 0.3, 0.3, 0.1), np.asarray, model.normalize, HWC_to_CHW]
    label = [None, None, None, AvgPool2d(8)]
    return joint, img, label


def aff_apply_transforms(img, la_scores, ha_scores, transforms):
    """voc12/data.py:233-258 for one decoded sample: img a PIL RGB image, la_scores / ha_scores float32 [21, H, W] (the files aff_prepare
    writes), transforms = aff_train_transform(...) -> (img float32 [3, crop, crop], label uint8 [crop/8, crop/8]: 0 background, 1..20 a
    class, 255 ignore).  The reference goes on to its three pair-label tensors; here the map is the contract (aff_loss.pair_labels gives
    the three tensors to whoever wants them)."""
    label = np.array(list(la_scores) + list(ha_scores))
    label = np.transpose(label, (1, 2, 0))
    for joint_t, img_t, label_t in zip(*transforms):
        if joint_t:
            img_label = joint_t(np.concatenate((img, label), axis=-1))      # (uint8 with float32: a float32 array)
            img, label = img_label[..., :3], img_label[..., 3:]
        if img_t:
            img = img_t(img)
        if label_t:
            label = label_t(label)
    no_score_region = np.max(label, -1) < np.float32(1e-5)                   # (the comparison is on the float32 means)
    label_la, label_ha = np.array_split(label, 2, axis=-1)
    label_la = np.argmax(label_la, axis=-1).astype(np.uint8)
    label_ha = np.argmax(label_ha, axis=-1).astype(np.uint8)
    label = label_la.copy()
    label[label_la == 0] = 255
    label[label_ha == 0] = 0
    label[no_score_region] = 255
    return np.ascontiguousarray(img), label


class VOC12AffDataset(VOC12ImageDataset):                  # voc12/data.py:201-261
    """(img float32 [3, crop, crop], label uint8 [crop/8, crop/8]) per image, on the host (numpy / PIL): the CPU path of AffinityNet
    training data and the yardstick of the device path (wseg_amd/aff_data.py).  Score files: `<la_crf_dir>/<name>.npy` and
    `<ha_crf_dir>/<name>.npy`, float32 [21, H, W] each."""

    def __init__(self, img_name_list_path, label_la_dir, label_ha_dir, voc12_root, transforms):
        super().__init__(img_name_list_path, voc12_root, transform=None)
        self.label_la_dir, self.label_ha_dir, self.transforms = label_la_dir, label_ha_dir, transforms

    def __getitem__(self, idx):
        name, img = super().__getitem__(idx)
        la = np.load(os.path.join(self.label_la_dir, name + '.npy'))
        ha = np.load(os.path.join(self.label_ha_dir, name + '.npy'))
        return aff_apply_transforms(img, la, ha, self.transforms)


# ---------------------------------------------------------------------------------------------- DeepLab-v1 training data
# The chain of segmentation/lib/datasets/BaseDataset.py:88-98 (__weak_augment__) with the transforms of lib/datasets/transform.py under
# experiment/SEAM_deeplabv1_resnet38/config.py (crop 448, scale [0.5, 1.5], H/S/V 10/10/10, flip 0.5), on (image uint8 [H, W, 3], label
# uint8 [H, W]) pairs.  The reference's RandomHSV and RandomScale call cv2, which is not available here: the 8-bit HSV arithmetic below is
# OpenCV's definition restated, and Pillow's bicubic stands in for cv2.INTER_CUBIC (as in seg_infer) — both UNPINNED against cv2 itself
# (DESIGN.md §8 9(c)).  RandomFlip, ImageNorm and the crop are pinned to the reference (tests/golden/seg_data_*.npz).  This is the host
# path of DeepLab training data and what the device path (wseg_amd/seg_data.py) is held to, bit for bit.
SEG_MEAN, SEG_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
HSV_SECTORS = ((1, 3, 0), (1, 0, 2), (3, 0, 1), (0, 2, 1), (0, 1, 3), (2, 1, 0))      # (b, g, r) in [V, p, q, t] per hue sector


def hsv_div_tables():
    """(sdiv, hdiv) int32 [256]: sdiv[i] = round(255 * 4096 / i), hdiv[i] = round(180 * 4096 / (6 * i)), both 0 at i = 0 (no quotient is
    at a half: 255 * 2^12 and 15 * 2^13 have no factor 2 left for an i <= 255)"""
    sdiv, hdiv = np.zeros(256, np.int32), np.zeros(256, np.int32)
    for i in range(1, 256):
        sdiv[i] = int(round(255 * 4096 / i))
        hdiv[i] = int(round(180 * 4096 / (6 * i)))
    return sdiv, hdiv


def rgb2hsv_u8(rgb):
    """uint8 [..., 3] RGB -> int32 (h in [0, 180), s, v in [0, 255]): the 8-bit conversion in integers, with the 12-bit division tables"""
    sdiv, hdiv = hsv_div_tables()
    c = np.asarray(rgb).astype(np.int32)
    r, g, b = c[..., 0], c[..., 1], c[..., 2]
    v = np.maximum(r, np.maximum(g, b))
    diff = v - np.minimum(r, np.minimum(g, b))
    s = (diff * sdiv[v] + 2048) >> 12
    hn = np.where(v == r, g - b, np.where(v == g, b - r + 2 * diff, r - g + 4 * diff))      # ties: r, then g, then b
    h = (hn * hdiv[diff] + 2048) >> 12                          # arithmetic shift
    h = np.where(h < 0, h + 180, h)
    return h, s, v


def hsv2rgb_u8(h, s, v, sectors=HSV_SECTORS):
    """integer h (degrees / 2), s, v in [0, 255] -> uint8 [..., 3] RGB in float32 arithmetic, every product and difference rounded on
    its own, the result rounded half to even"""
    f32 = np.float32
    h, s, v = np.asarray(h), np.asarray(s), np.asarray(v)
    S, V = s.astype(f32) / f32(255), v.astype(f32) / f32(255)
    hh = h.astype(f32) * (f32(6) / f32(180))
    while (hh < 0).any():
        hh = np.where(hh < 0, hh + f32(6), hh)
    while (hh >= 6).any():
        hh = np.where(hh >= 6, hh - f32(6), hh)
    fl = np.floor(hh)
    sec, f = fl.astype(np.int32), hh - fl
    bad = (sec < 0) | (sec >= 6)
    sec, f = np.where(bad, 0, sec), np.where(bad, f32(0), f)
    one = f32(1)
    tab = np.stack([V, V * (one - S), V * (one - S * f), V * (one - S * (one - f))], axis=-1)
    assert tab.dtype == np.float32
    idx = np.asarray(sectors, np.int64)[sec]                    # [..., 3] = the table slots of (b, g, r)
    bgr = np.take_along_axis(tab, idx, axis=-1)
    bgr = np.where((s == 0)[..., None], V[..., None], bgr)
    out = np.clip(np.rint(bgr * f32(255)), 0, 255).astype(np.uint8)
    return out[..., ::-1]


def hsv_jitter(img_u8, dh, ds, dv):
    """transform.py:83-101 on a decoded uint8 RGB image with given offsets"""
    h, s, v = rgb2hsv_u8(img_u8)
    h = (h + dh) % 180                                          # Python's (numpy's) non-negative modulo
    s = np.clip(s + ds, 0, 255)
    v = np.clip(v + dv, 0, 255)
    return np.ascontiguousarray(hsv2rgb_u8(h, s, v))


def seg_scaled_size(h, w, scale):
    """size after RandomScale: (round(H * s), round(W * s)), half to even as Python's round"""
    rh, rw = int(round(h * scale)), int(round(w * scale))
    if rh < 1 or rw < 1:
        raise ValueError(f"RandomScale: {h} x {w} at scale {scale} leaves no pixel")
    return rh, rw


def nearest_index_table(n_in, n_out, scale):
    """int32 [n_out]: the source index of every output position of a nearest-neighbour rescale by `scale`: min(floor(o * (1 / scale)),
    n_in - 1) in float64, the reciprocal computed once"""
    inv = 1.0 / float(scale)
    return np.minimum(np.floor(np.arange(n_out, dtype=np.float64) * inv).astype(np.int64), n_in - 1).astype(np.int32)


class RandomHSV:                                           # lib/datasets/transform.py:76-102
    def __init__(self, h_r, s_r, v_r, rng=random):
        self.h_r, self.s_r, self.v_r, self.rng = h_r, s_r, v_r, rng

    def __call__(self, image, label):
        dh = self.rng.randint(-self.h_r, self.h_r)
        ds = self.rng.randint(-self.s_r, self.s_r)
        dv = self.rng.randint(-self.v_r, self.v_r)
        return hsv_jitter(image, dh, ds, dv), label


class RandomFlip:                                          # lib/datasets/transform.py:104-124: np.flip(axis=1) of the image and the label
    def __init__(self, threshold, rng=random):
        self.flip_t, self.rng = threshold, rng

    def __call__(self, image, label):
        if self.rng.random() < self.flip_t:
            image, label = np.flip(image, axis=1), np.flip(label, axis=1)
        return image, label


class RandomScale:                                         # lib/datasets/transform.py:126-149: the image cubic, the label nearest
    def __init__(self, scale_r, rng=random):
        self.scale_r, self.rng = scale_r, rng

    def __call__(self, image, label):
        h, w = image.shape[:2]
        scale = self.rng.random() * (self.scale_r[1] - self.scale_r[0]) + self.scale_r[0]
        rh, rw = seg_scaled_size(h, w, scale)
        image = np.asarray(PIL.Image.fromarray(np.ascontiguousarray(image)).resize((rw, rh), BICUBIC))
        label = label[nearest_index_table(h, rh, scale)][:, nearest_index_table(w, rw, scale)]
        return image, label


class ImageNorm:                                           # lib/datasets/transform.py:151-168: float32 arithmetic on the float32 image
    def __init__(self, mean=SEG_MEAN, std=SEG_STD):
        self.mean, self.std = mean, std

    def __call__(self, image, label):
        image = image.astype(np.float32)
        for c in range(3):
            image[..., c] = (image[..., c] / 255 - self.mean[c]) / self.std[c]
        return image, label


class SegRandomCrop:
    """lib/datasets/transform.py:12-74: the width draw before the height draw; the float32 image into a ZERO container (the padding is
    +0.0, not normalize(0)), the label into a container of 255."""

    def __init__(self, output_size, rng=random):
        self.output_size, self.rng = (output_size, output_size) if isinstance(output_size, int) else tuple(output_size), rng

    def __call__(self, image, label):
        h, w = image.shape[:2]
        oh, ow = self.output_size
        ch, cw = min(h, oh), min(w, ow)
        h_space, w_space = h - oh, w - ow
        if w_space > 0:
            cont_left, img_left = 0, self.rng.randrange(w_space + 1)
        else:
            cont_left, img_left = self.rng.randrange(-w_space + 1), 0
        if h_space > 0:
            cont_top, img_top = 0, self.rng.randrange(h_space + 1)
        else:
            cont_top, img_top = self.rng.randrange(-h_space + 1), 0
        img_crop = np.zeros((oh, ow, 3), np.float32)
        img_crop[cont_top:cont_top + ch, cont_left:cont_left + cw] = image[img_top:img_top + ch, img_left:img_left + cw]
        seg_crop = np.full((oh, ow), 255, label.dtype)
        seg_crop[cont_top:cont_top + ch, cont_left:cont_left + cw] = label[img_top:img_top + ch, img_left:img_left + cw]
        return img_crop, seg_crop


def seg_train_transform(crop=448, scale_r=(0.5, 1.5), hsv_r=(10, 10, 10), flip_p=0.5, rng=random):
    """BaseDataset.py:88-98 under config.py: RandomHSV -> RandomFlip -> RandomScale -> ImageNorm -> RandomCrop"""
    return [RandomHSV(*hsv_r, rng=rng), RandomFlip(flip_p, rng=rng), RandomScale(scale_r, rng=rng), ImageNorm(), SegRandomCrop(crop, rng=rng)]


def seg_apply_transforms(image, label, transforms):
    """(img float32 [3, crop, crop], label uint8 [crop, crop]: 0..20 a class, 255 ignore) of one decoded sample (ToTensor's CHW; the
    reference's int64 label is emitted as uint8, the form seg_loss.seg_cross_entropy accepts)"""
    image, label = np.asarray(image, np.uint8), np.asarray(label, np.uint8)
    if image.ndim != 3 or image.shape[2] != 3 or label.shape != image.shape[:2]:
        raise ValueError(f"seg_apply_transforms: image {image.shape} with label {label.shape}")
    for t in transforms:
        image, label = t(image, label)
    return np.ascontiguousarray(HWC_to_CHW(image)), np.ascontiguousarray(label)


def load_seg_label(path):
    """a label PNG (palette or greyscale: the stored indices) as uint8 [H, W] (VOCDataset.py load_pseudo_segmentation / load_segmentation)"""
    return np.asarray(PIL.Image.open(path), dtype=np.uint8)


class VOCSegTrainDataset(VOC12ImageDataset):
    """(img float32 [3, crop, crop], label uint8 [crop, crop]) per image on the host: the CPU path of DeepLab-v1 training data and the
    yardstick of the device path (wseg_amd/seg_data.py).  Labels: `<pseudo_gt_dir>/<name>.png`."""

    def __init__(self, img_name_list_path, voc12_root, pseudo_gt_dir, transforms=None):
        super().__init__(img_name_list_path, voc12_root, transform=None)
        self.pseudo_gt_dir, self.transforms = pseudo_gt_dir, transforms or seg_train_transform()

    def __getitem__(self, idx):
        name, img = super().__getitem__(idx)
        label = load_seg_label(os.path.join(self.pseudo_gt_dir, name + '.png'))
        return seg_apply_transforms(np.asarray(img), label, self.transforms)
