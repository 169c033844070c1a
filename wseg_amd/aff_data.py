"""AffinityNet training data on the device: decoded files -> (img float32 [N, 3, crop, crop], label uint8 [N, crop/8, crop/8]), the two
tensors a training step consumes (`label` is what aff_loss.affinity_loss accepts, with no host round trip).

The transform chain is aff_train.py:39-60 in the zip order of voc12/data.py:237-249 (host restatement: wseg_amd/data.py
aff_train_transform / VOC12AffDataset): ColorJitter on the PIL image -> np.asarray -> joint RandomCrop(crop) of the image and the 42 CRF score
planes into a zero float32 container, THEN normalize (numpy float32 arithmetic; the padding becomes normalize(0)) -> joint flip of the
container (one random bit) -> HWC_to_CHW / AvgPool2d(8) -> the label rule of voc12/data.py:251-258.  The host pipeline moves two dense
float32 [21, H, W] stacks per image through a 45-channel crop; almost all of those planes are zero.  Here a DataLoader worker reads the
files, draws the parameters from Python's `random` in the host chain's order and keeps only the planes that hold a value (`pack_scores`);
`DeviceAffData` does the rest on the GPU (csrc/augment.hip wseg_aff_augment_batch, csrc/aff_data.hip wseg_aff_labels_batch): the image bit
for bit what the host chain gives from the same draws, the label map the dense rule's (tests/test_gpu_aff_data.py).
"""
import os
import random

import numpy as np
import PIL.Image
import torch
from torch.utils.data import Dataset

from . import _lib as L
from . import data as wdata
from .augment import CROP_KEYS, AugDesc, fill_shared
from .stage_io import DescRing

MAX_PLANES = 21


def normalize_lut_f32(mean=(0.485, 0.456, 0.406), std=(0.229, 0.224, 0.225)):
    """(v / 255. - mean) / std for v = 0..255 per channel in FLOAT32 arithmetic — what network/resnet38d.py:104-118 gives on the float32
    container RandomCrop returns (the AffinityNet chain normalises after the crop).  augment.normalize_lut is the float64 evaluation the
    contrast chain needs (it normalises the uint8 image): the two tables differ in the last bit of many entries."""
    v = np.arange(256, dtype=np.float32)
    return np.stack([((v / np.float32(255.) - np.float32(mean[c])) / np.float32(std[c])).astype(np.float32) for c in range(3)])


def draw_aff_params(w, h, crop=448, jitter=(0.3, 0.3, 0.3, 0.1), rng=random):
    """The random draws of the host chain (wseg_amd/data.py aff_train_transform: ColorJitter, RandomCrop, RandomHorizontalFlipArray), in
    its order, from the same generator calls: the jitter draws, the crop's width draw, its height draw, the flip bit."""
    b, c, s, hj = jitter
    fb, fc, fs = rng.uniform(1 - b, 1 + b), rng.uniform(1 - c, 1 + c), rng.uniform(1 - s, 1 + s)
    hf = rng.uniform(-hj, hj)
    order = [0, 1, 2, 3]
    rng.shuffle(order)                                      # (the host shuffles its list of four ops: same permutation)
    w_space, h_space = w - crop, h - crop
    if w_space > 0:
        cont_left, img_left = 0, rng.randrange(w_space + 1)
    else:
        cont_left, img_left = rng.randrange(-w_space + 1), 0
    if h_space > 0:
        cont_top, img_top = 0, rng.randrange(h_space + 1)
    else:
        cont_top, img_top = rng.randrange(-h_space + 1), 0
    flip = rng.getrandbits(1)
    return dict(flip=int(flip), op=order, factor=[(fb, fc, fs, 0.0)[o] for o in order], hue_shift=int(hf * 255),
                cont_top=cont_top, cont_left=cont_left, img_top=img_top, img_left=img_left, ch=min(crop, h), cw=min(crop, w))


def pack_scores(stack):
    """(ids int32 [P], planes float32 [P, H, W]): the planes of a [K <= 21, H, W] CRF score stack that hold any non-zero value, in ascending
    plane id.  An absent plane is a zero plane to the device, which then gives the label of the dense rule — for scores >= 0 (CRF
    probabilities).  Negative scores are NOT supported (a negative mean would lose to an absent plane's zero where the dense arg-max may
    pick it): they raise here."""
    s = np.asarray(stack)
    if s.ndim != 3 or not 1 <= s.shape[0] <= MAX_PLANES or s.shape[1] < 1 or s.shape[2] < 1:
        raise ValueError(f"pack_scores: a [K <= {MAX_PLANES}, H, W] score stack, got {s.shape}")
    s = s.astype(np.float32, copy=False)
    if (s < 0).any():
        raise ValueError("pack_scores: negative scores are not supported (CRF probabilities are >= 0)")
    ids = np.flatnonzero(s.reshape(s.shape[0], -1).any(axis=1)).astype(np.int32)
    return ids, np.ascontiguousarray(s[ids])


def make_aff_sample(name, img_u8, la_scores, ha_scores, crop=448, rng=random):
    """One sample as a DataLoader worker produces it (numpy arrays only; packed per batch by `aff_collate`)."""
    img_u8 = np.ascontiguousarray(img_u8, dtype=np.uint8)
    h, w = img_u8.shape[:2]
    la, ha = np.asarray(la_scores), np.asarray(ha_scores)
    if img_u8.ndim != 3 or img_u8.shape[2] != 3 or la.shape[1:] != (h, w) or ha.shape[1:] != (h, w):
        raise ValueError(f"make_aff_sample: image {img_u8.shape} with score stacks {la.shape} and {ha.shape}")
    p = draw_aff_params(w, h, crop, rng=rng)
    p.update(H=h, W=w)
    la_ids, la_planes = pack_scores(la)
    ha_ids, ha_planes = pack_scores(ha)
    return dict(name=name, img=img_u8, params=p, ids=(la_ids, ha_ids), planes=(la_planes, ha_planes))


class VOC12AffDatasetRaw(Dataset):
    """voc12/data.py:201-261 for the device pipeline: the decoded image, the random draws and the sparse planes of the two score stacks
    (`<la_crf_dir>/<name>.npy`, `<ha_crf_dir>/<name>.npy`, float32 [21, H, W])."""

    def __init__(self, img_name_list_path, label_la_dir, label_ha_dir, voc12_root, crop=448):
        self.img_name_list = wdata.load_img_name_list(img_name_list_path)
        self.label_la_dir, self.label_ha_dir, self.voc12_root, self.crop = label_la_dir, label_ha_dir, voc12_root, crop

    def __len__(self):
        return len(self.img_name_list)

    def __getitem__(self, idx):
        name = self.img_name_list[idx]
        img = np.asarray(PIL.Image.open(wdata.get_img_path(name, self.voc12_root)).convert("RGB"))
        la = np.load(os.path.join(self.label_la_dir, name + '.npy'))
        ha = np.load(os.path.join(self.label_ha_dir, name + '.npy'))
        return make_aff_sample(name, img, la, ha, self.crop)


def aff_collate(samples):
    """Runs in the DataLoader worker.  Images and plane sets differ per sample, so a batch is three blobs — uint8: the decoded images back
    to back; float32: the shipped planes of both stacks of every image, each plane 16-byte aligned; int32: their plane ids — and the
    per-image parameter dicts with the offsets (elements of the blob's dtype): three tensors cross the process boundary."""
    n_img = n_pl = n_id = 0
    for s in samples:
        p = s["params"]
        p["img_off"] = n_img
        n_img += (s["img"].size + 15) // 16 * 16
        p["plane_stride"] = (p["H"] * p["W"] + 3) // 4 * 4
        p["planes_off"], p["ids_off"], p["np"] = [], [], []
        for ids in s["ids"]:
            p["planes_off"].append(n_pl); p["ids_off"].append(n_id); p["np"].append(len(ids))
            n_pl += len(ids) * p["plane_stride"]
            n_id += len(ids)
    img = np.empty(n_img, np.uint8)
    planes = np.zeros(max(n_pl, 4), np.float32)
    idb = np.zeros(max(n_id, 1), np.int32)
    for s in samples:
        p = s["params"]
        img[p["img_off"]:p["img_off"] + s["img"].size] = s["img"].reshape(-1)
        hw = p["H"] * p["W"]
        for ids, pl, po, io in zip(s["ids"], s["planes"], p["planes_off"], p["ids_off"]):
            idb[io:io + len(ids)] = ids
            for k in range(len(ids)):
                planes[po + k * p["plane_stride"]:po + k * p["plane_stride"] + hw] = pl[k].reshape(-1)
    return dict(img=torch.from_numpy(img), planes=torch.from_numpy(planes), ids=torch.from_numpy(idb),
                params=[s["params"] for s in samples], names=[s["name"] for s in samples])


def dense_bytes(batch):
    """(shipped, dense): bytes of the three blobs of a collated batch, and of what the host chain reads for the same images (the image and two
    dense float32 [21, H, W] stacks each)."""
    shipped = sum(batch[k].numel() * batch[k].element_size() for k in ("img", "planes", "ids"))
    return shipped, sum(p["H"] * p["W"] * (3 + 2 * MAX_PLANES * 4) for p in batch["params"])


class DeviceAffData:
    """__call__(batch) -> (img float32 [N, 3, crop, crop], label uint8 [N, crop/8, crop/8]) on `device`, enqueued on the current stream;
    nothing waits for the device (the descriptors go through stage_io.DescRing).
    Limits: crop % 8 == 0; at most 21 planes per stack; any H, W >= 1."""

    def __init__(self, device, crop=448):
        self.device, self.crop = torch.device(device), int(crop)
        if self.device.type != "cuda":
            raise RuntimeError("DeviceAffData runs on the MI355X only (the host pipeline is wseg_amd.data.VOC12AffDataset)")
        if self.crop < 8 or self.crop % 8:
            raise ValueError(f"DeviceAffData: crop {crop} is no positive multiple of 8 (the label map is crop/8 x crop/8)")
        self.lut = torch.from_numpy(normalize_lut_f32()).to(self.device).contiguous()
        self.ring = DescRing(self.device)

    def _check(self, p, n_img, n_planes, n_ids):
        """every offset and extent the kernels will follow, against the blobs (raw pointers beyond __call__)"""
        H, W, crop = p["H"], p["W"], self.crop
        ok = H >= 1 and W >= 1 and p["ch"] == min(crop, H) and p["cw"] == min(crop, W) and p["flip"] in (0, 1)
        ok = ok and 0 <= p["img_top"] <= H - p["ch"] and 0 <= p["img_left"] <= W - p["cw"]
        ok = ok and 0 <= p["cont_top"] <= crop - p["ch"] and 0 <= p["cont_left"] <= crop - p["cw"]
        ok = ok and 0 <= p["img_off"] and p["img_off"] + H * W * 3 <= n_img and p["plane_stride"] >= H * W
        if not ok:
            raise ValueError(f"DeviceAffData: inconsistent sample parameters {p}")
        for s in range(2):
            if not 0 <= p["np"][s] <= MAX_PLANES:
                raise ValueError(f"DeviceAffData: {p['np'][s]} planes in a stack (at most {MAX_PLANES})")
            if p["np"][s] and (p["planes_off"][s] < 0 or p["planes_off"][s] % 4 or p["ids_off"][s] < 0 or p["ids_off"][s] + p["np"][s] > n_ids
                               or p["planes_off"][s] + (p["np"][s] - 1) * p["plane_stride"] + H * W > n_planes):
                raise ValueError(f"DeviceAffData: plane offsets of {p} leave the blobs")

    def __call__(self, batch):
        """batch: what `aff_collate` made of a list of samples (a list of samples is accepted too)."""
        if isinstance(batch, (list, tuple)):
            batch = aff_collate(batch)
        params, crop, dev = batch["params"], self.crop, self.device
        n = len(params)
        if crop % 8:
            raise ValueError(f"DeviceAffData: crop {crop} is no multiple of 8")
        ids_host = batch["ids"]
        if ids_host.numel() and (int(ids_host.min()) < 0 or int(ids_host.max()) >= MAX_PLANES):
            raise ValueError(f"DeviceAffData: plane ids outside [0, {MAX_PLANES})")
        for p in params:
            self._check(p, batch["img"].numel(), batch["planes"].numel(), ids_host.numel())
        d_img, d_planes, d_ids = (self.ring.to_device(batch[k]) for k in ("img", "planes", "ids"))
        img = torch.empty(n, 3, crop, crop, device=dev, dtype=torch.float32)
        label = torch.empty(n, crop // 8, crop // 8, device=dev, dtype=torch.uint8)
        aug, lab = (AugDesc * n)(), (L.AffLabelDesc * n)()
        max_pixels = 1
        for i, p in enumerate(params):
            a, b = aug[i], lab[i]
            a.H, a.W, a.rh, a.rw = p["H"], p["W"], p["H"], p["W"]
            a.img, a.out = d_img.data_ptr() + p["img_off"], img[i].data_ptr()      # jittered in place: the upload is scratch
            fill_shared(a, p)
            for s in range(2):
                b.planes[s], b.ids[s], b.np[s] = d_planes.data_ptr() + 4 * p["planes_off"][s], d_ids.data_ptr() + 4 * p["ids_off"][s], p["np"][s]
            b.H, b.W, b.plane_stride, b.flip = p["H"], p["W"], p["plane_stride"], p["flip"]
            for k in CROP_KEYS:
                setattr(b, k, p[k])
            max_pixels = max(max_pixels, p["H"] * p["W"])
        d_desc, (_, lab_at) = self.ring.upload(aug, lab)        # both descriptor arrays in one staging buffer, one copy
        sums = torch.empty(n * 4, device=dev, dtype=torch.int64)
        self._keep = (d_img, d_planes, d_ids, d_desc, sums)   # (alive until the next call: the kernels are asynchronous)
        self._last = (d_desc.data_ptr(), lab_at, n, max_pixels, sums, img, label)
        self.launch_last()
        return img, label

    def launch_last(self, image=True, labels=True):
        """The launches of the last call again, on its uploaded blobs and into its outputs (scripts/bench_aff_data.py times the kernels
        apart from the copies with it).  The colour ops work in place, so a repeated image pass jitters the upload once more: same work,
        other values; the label pass reads only."""
        desc, lab_at, n, max_pixels, sums, img, label = self._last
        if image:
            L.aff_augment_batch(desc, n, max_pixels, self.lut, self.crop, sums)
        if labels:
            L.aff_labels_batch(desc + lab_at, n, self.crop, label)
