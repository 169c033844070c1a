"""DeepLab-v1 training data on the device: decoded files -> (img float32 [N, 3, crop, crop], label uint8 [N, crop, crop]), the two tensors a
DeepLab training step consumes (`label` is what seg_loss.seg_cross_entropy accepts, with no host round trip).

The transform chain is segmentation/lib/datasets/BaseDataset.py:88-98 (__weak_augment__) with lib/datasets/transform.py under
experiment/SEAM_deeplabv1_resnet38/config.py (host restatement: wseg_amd/data.py seg_train_transform / VOCSegTrainDataset): RandomHSV on
the decoded uint8 image -> RandomFlip of image and label (before the rescale) -> RandomScale (image cubic, label nearest) -> ImageNorm in
float32 arithmetic -> RandomCrop into a container of +0.0 (image) and 255 (label) -> CHW.  A DataLoader worker decodes the JPEG and the
label PNG, draws the parameters from Python's `random` in the host chain's order and builds the small tables: Pillow's bicubic coefficients
(augment.pil_bicubic_coeffs) and the label's two nearest-neighbour index tables (float64 on the host; the column table composed with the
flip).  `DeviceSegData` does the rest on the GPU (csrc/seg_data.hip wseg_seg_data_batch: four launches per batch), both outputs bit for bit
what the host chain gives from the same draws (tests/test_gpu_seg_data.py).

Unpinned against the reference: its RandomHSV and its cubic resize call cv2, which is not available here.  The 8-bit HSV arithmetic is
OpenCV's definition restated (wseg_amd/data.py rgb2hsv_u8 / hsv2rgb_u8) and Pillow's bicubic stands in for cv2.INTER_CUBIC (a = -0.5 and
antialiased when shrinking, against a = -0.75 without antialiasing; as in seg_infer): DESIGN.md §8 9(c).  The flip, the normalisation, the
crop and the order of the draws ARE pinned to the reference's transform.py (tests/golden/seg_data_*.npz).
"""
import ctypes as C
import os
import random

import numpy as np
import PIL.Image
import torch
from torch.utils.data import Dataset

from . import _lib as L
from . import data as wdata
from .aff_data import normalize_lut_f32
from .augment import CROP_KEYS, AugDesc, pil_bicubic_coeffs
from .stage_io import DescRing

TABLES = ("xb", "xk", "yb", "yk", "yi", "xi")
HSV, RESIZE, FINISH = 1, 2, 4                  # the launches of wseg_seg_data_batch (include/wseg_hip.h WSEG_SEG_DATA_*)


def draw_seg_params(w, h, crop=448, scale_r=(0.5, 1.5), hsv_r=(10, 10, 10), flip_p=0.5, rng=random):
    """The random draws of the host chain (wseg_amd/data.py seg_train_transform: RandomHSV, RandomFlip, RandomScale, SegRandomCrop), in its
    order, from the same generator calls: the h, s, v offsets, the flip, the scale, the crop's width draw, its height draw."""
    dh, ds, dv = (rng.randint(-r, r) for r in hsv_r)
    flip = rng.random() < flip_p
    scale = rng.random() * (scale_r[1] - scale_r[0]) + scale_r[0]
    rh, rw = wdata.seg_scaled_size(h, w, scale)
    w_space, h_space = rw - crop, rh - crop
    if w_space > 0:
        cont_left, img_left = 0, rng.randrange(w_space + 1)
    else:
        cont_left, img_left = rng.randrange(-w_space + 1), 0
    if h_space > 0:
        cont_top, img_top = 0, rng.randrange(h_space + 1)
    else:
        cont_top, img_top = rng.randrange(-h_space + 1), 0
    return dict(dh=dh, ds=ds, dv=dv, flip=int(flip), scale=scale, rh=rh, rw=rw, cont_top=cont_top, cont_left=cont_left, img_top=img_top,
                img_left=img_left, ch=min(crop, rh), cw=min(crop, rw))


def label_index_tables(h, w, p):
    """(yi int32 [rh], xi int32 [rw]) of the draws `p`: label_out[y][x] = label[yi[y]][xi[x]] is the nearest rescale of the FLIPPED label
    (flipping, then indexing column xi[x], reads column W-1-xi[x] of the unflipped label)"""
    yi = wdata.nearest_index_table(h, p["rh"], p["scale"])
    xi = wdata.nearest_index_table(w, p["rw"], p["scale"])
    return yi, (w - 1 - xi).astype(np.int32) if p["flip"] else xi


def make_seg_sample(name, img_u8, label_u8, crop=448, scale_r=(0.5, 1.5), hsv_r=(10, 10, 10), flip_p=0.5, rng=random):
    """One sample as a DataLoader worker produces it (numpy arrays only; packed per batch by `seg_collate`)."""
    img_u8, label_u8 = np.ascontiguousarray(img_u8, dtype=np.uint8), np.ascontiguousarray(label_u8, dtype=np.uint8)
    if img_u8.ndim != 3 or img_u8.shape[2] != 3 or label_u8.shape != img_u8.shape[:2]:
        raise ValueError(f"make_seg_sample: image {img_u8.shape} with label {label_u8.shape}")
    h, w = label_u8.shape
    p = draw_seg_params(w, h, crop, scale_r, hsv_r, flip_p, rng)
    xb, xk = pil_bicubic_coeffs(w, p["rw"])
    yb, yk = pil_bicubic_coeffs(h, p["rh"])
    yi, xi = label_index_tables(h, w, p)
    p.update(H=h, W=w, xks=xk.shape[1], yks=yk.shape[1])
    return dict(name=name, img=img_u8, label=label_u8, params=p, xb=xb, xk=xk, yb=yb, yk=yk, yi=yi, xi=xi)


class VOCSegDatasetRaw(Dataset):
    """VOCDataset / BaseDataset.__sample_generate__ for the device pipeline: the decoded image, the label PNG `<pseudo_gt_dir>/<name>.png`
    (a ground-truth SegmentationClass folder goes through the same loader), the random draws and the tables."""

    def __init__(self, name_list_path, voc12_root, pseudo_gt_dir, crop=448):
        self.img_name_list = wdata.load_img_name_list(name_list_path)
        self.voc12_root, self.pseudo_gt_dir, self.crop = voc12_root, pseudo_gt_dir, crop

    def __len__(self):
        return len(self.img_name_list)

    def __getitem__(self, idx):
        name = self.img_name_list[idx]
        img = np.asarray(PIL.Image.open(wdata.get_img_path(name, self.voc12_root)).convert("RGB"))
        label = wdata.load_seg_label(os.path.join(self.pseudo_gt_dir, name + '.png'))
        return make_seg_sample(name, img, label, self.crop)


def seg_collate(samples):
    """Runs in the DataLoader worker.  A batch is ONE uint8 blob (per image the decoded image, then its label map, each 16-byte aligned),
    ONE int32 blob (the six tables of every image) and the per-image parameter dicts with their offsets."""
    n_u8 = n_tab = 0
    for s in samples:
        p = s["params"]
        p["img_off"] = n_u8
        n_u8 += (s["img"].size + 15) // 16 * 16
        p["lab_off"] = n_u8
        n_u8 += (s["label"].size + 15) // 16 * 16
        p["tab_off"] = []
        for k in TABLES:
            p["tab_off"].append(n_tab)
            n_tab += s[k].size
    u8 = np.zeros(n_u8, np.uint8)
    tab = np.empty(n_tab, np.int32)
    for s in samples:
        p = s["params"]
        u8[p["img_off"]:p["img_off"] + s["img"].size] = s["img"].reshape(-1)
        u8[p["lab_off"]:p["lab_off"] + s["label"].size] = s["label"].reshape(-1)
        for k, o in zip(TABLES, p["tab_off"]):
            tab[o:o + s[k].size] = s[k].reshape(-1)
    return dict(u8=torch.from_numpy(u8), tab=torch.from_numpy(tab), params=[s["params"] for s in samples], names=[s["name"] for s in samples])


def geometry(max_pixels, crop):
    """(workgroups per image of the hsv launch at max_pixels = H*W, of a resize pass at max_pixels = its output pixels, of the finish launch,
    container pixels per finish thread) — wseg_seg_data_geometry"""
    out = (C.c_int32 * 4)()
    L.check(L.lib.wseg_seg_data_geometry(int(max_pixels), int(crop), out), "wseg_seg_data_geometry")
    return tuple(out)


class DeviceSegData:
    """__call__(batch) -> (img float32 [N, 3, crop, crop], label uint8 [N, crop, crop]) on `device`, enqueued on the current stream; nothing
    waits for the device (the descriptors go through stage_io.DescRing).  Any crop >= 1 and any H, W >= 1; 16-byte stores at crop % 4 == 0."""

    def __init__(self, device, crop=448):
        self.device, self.crop = torch.device(device), int(crop)
        if self.device.type != "cuda":
            raise RuntimeError("DeviceSegData runs on the MI355X only (the host pipeline is wseg_amd.data.VOCSegTrainDataset)")
        if self.crop < 1:
            raise ValueError(f"DeviceSegData: crop {crop}")
        sdiv, hdiv = wdata.hsv_div_tables()
        tables = np.concatenate([normalize_lut_f32().reshape(-1).view(np.int32), sdiv, hdiv])      # one upload: [3][256] f32, then the two
        self.tables = torch.from_numpy(tables).to(self.device).contiguous()                          # 256-entry division tables
        self.ring = DescRing(self.device)

    def _lut(self):
        return self.tables.data_ptr(), self.tables.data_ptr() + 4 * 768

    def _check(self, p, tab, n_u8):
        """every offset and extent the kernels will follow, against the blobs (raw pointers beyond __call__); the crop rectangle itself is
        the entry point's to refuse"""
        H, W, rh, rw = p["H"], p["W"], p["rh"], p["rw"]
        ok = H >= 1 and W >= 1 and rh >= 1 and rw >= 1 and p["flip"] in (0, 1) and p["xks"] >= 1 and p["yks"] >= 1
        ok = ok and 0 <= p["img_off"] and p["img_off"] + H * W * 3 <= n_u8 and 0 <= p["lab_off"] and p["lab_off"] + H * W <= n_u8
        sizes = (2 * rw, rw * p["xks"], 2 * rh, rh * p["yks"], rh, rw) if ok else ()
        ok = ok and all(0 <= o and o + n <= tab.size for o, n in zip(p["tab_off"], sizes))
        if not ok:
            raise ValueError(f"DeviceSegData: inconsistent sample parameters {p}")
        t = [tab[o:o + n] for o, n in zip(p["tab_off"], sizes)]
        for b, ks, n_in in ((t[0].reshape(-1, 2), p["xks"], W), (t[2].reshape(-1, 2), p["yks"], H)):
            if (b[:, 0] < 0).any() or (b[:, 1] < 0).any() or (b[:, 1] > ks).any() or (b[:, 0] + b[:, 1] > n_in).any():
                raise ValueError(f"DeviceSegData: resampling bounds of {p} leave the image")
        if t[4].min() < 0 or t[4].max() >= H or t[5].min() < 0 or t[5].max() >= W:
            raise ValueError(f"DeviceSegData: label index tables of {p} leave the label map")

    def __call__(self, batch):
        """batch: what `seg_collate` made of a list of samples (a list of samples is accepted too)."""
        if isinstance(batch, (list, tuple)):
            batch = seg_collate(batch)
        params, crop, dev = batch["params"], self.crop, self.device
        n = len(params)
        tab_host = batch["tab"].numpy()
        for p in params:
            self._check(p, tab_host, batch["u8"].numel())
        d_u8, d_tab = self.ring.to_device(batch["u8"]), self.ring.to_device(batch["tab"])
        offs, total = [], 0
        for p in params:                                        # scratch per image: the jittered image, the horizontal pass, the rescaled image
            o = []
            for nbytes in (p["H"] * p["W"] * 3, p["H"] * p["rw"] * 3, p["rh"] * p["rw"] * 3):
                o.append(total); total += (nbytes + 15) // 16 * 16
            offs.append(o)
        scratch = torch.empty(total, device=dev, dtype=torch.uint8)
        img = torch.empty(n, 3, crop, crop, device=dev, dtype=torch.float32)
        label = torch.empty(n, crop, crop, device=dev, dtype=torch.uint8)
        aug, seg = (AugDesc * n)(), (L.SegDataDesc * n)()
        for i, (p, o) in enumerate(zip(params, offs)):
            a, b, to = aug[i], seg[i], [d_tab.data_ptr() + 4 * t for t in p["tab_off"]]
            a.H, a.W, a.rh, a.rw, a.flip = p["H"], p["W"], p["rh"], p["rw"], p["flip"]
            a.src, a.tmp, a.img = (scratch.data_ptr() + x for x in o)
            a.xb, a.xk, a.xks, a.yb, a.yk, a.yks = to[0], to[1], p["xks"], to[2], to[3], p["yks"]
            a.out = img[i].data_ptr()
            for j in range(4):
                a.op[j] = -1                                    # (the colour ops of the contrast chain: not read here)
            for k in CROP_KEYS:
                setattr(a, k, p[k])
            b.raw, b.lab = d_u8.data_ptr() + p["img_off"], d_u8.data_ptr() + p["lab_off"]
            b.yi, b.xi, b.lab_out = to[4], to[5], label[i].data_ptr()
            b.dh, b.ds, b.dv = p["dh"], p["ds"], p["dv"]
        self._keep = (d_u8, d_tab, scratch, aug, seg)             # (alive until the next call: the kernels are asynchronous)
        self._last = None
        self._upload_and_launch(aug, seg, n)
        return img, label

    def _upload_and_launch(self, aug, seg, n, stages=HSV | RESIZE | FINISH):
        """the entry point reads the host copies (it refuses bad descriptors before any launch), the kernels the uploaded ones"""
        d_desc, (_, seg_at) = self.ring.upload(aug, seg)          # both descriptor arrays in one staging buffer, one copy
        self._last = (aug, seg, d_desc, seg_at, n)
        self.launch_last(stages)

    def launch_last(self, stages=HSV | RESIZE | FINISH):
        """The launches of the last call again (any subset: HSV, RESIZE, FINISH), on its uploaded blobs and into its outputs
        (scripts/bench_seg_data.py times the launches apart from the copies with it).  Every launch is out of place: same values."""
        aug, seg, d_desc, seg_at, n = self._last
        lut, div = self._lut()
        L.seg_data_batch(aug, seg, d_desc.data_ptr(), d_desc.data_ptr() + seg_at, n, self.crop, lut, div, stages)

    def hsv(self, img_u8, deltas=(0, 0, 0), flip=False):
        """The HSV launch alone: a decoded uint8 [H, W, 3] image (numpy) -> the jittered, optionally flipped uint8 [H, W, 3] image on the
        device, which is what the resampler reads."""
        img_u8 = np.ascontiguousarray(img_u8, dtype=np.uint8)
        if img_u8.ndim != 3 or img_u8.shape[2] != 3 or img_u8.size == 0:
            raise ValueError(f"DeviceSegData.hsv: a uint8 [H, W, 3] image, got {img_u8.shape}")
        d_raw = self.ring.to_device(torch.from_numpy(img_u8))
        out = torch.empty_like(d_raw)
        aug, seg = (AugDesc * 1)(), (L.SegDataDesc * 1)()
        a, b = aug[0], seg[0]
        a.H, a.W, a.rh, a.rw, a.flip, a.src = img_u8.shape[0], img_u8.shape[1], img_u8.shape[0], img_u8.shape[1], int(bool(flip)), out.data_ptr()
        b.raw, (b.dh, b.ds, b.dv) = d_raw.data_ptr(), (int(d) for d in deltas)
        self._keep = (d_raw, out, aug, seg)
        self._upload_and_launch(aug, seg, 1, HSV)
        return out
