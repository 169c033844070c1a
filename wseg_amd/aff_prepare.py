"""CLI of the reference's aff_prepare.py (same flags) on the MI355X path: the AffinityNet training labels.  Per image, the CAM
dictionary contrast_infer wrote (<cam_dir>/<name>.npy) becomes a label map with the background (1 - max_c cam)^alpha, the dense CRF
(sxy 80 / srgb 13, Gaussian sxy 3, 10 iterations) refines it, and its Q is saved as <out_crf>/<alpha:.2f>/<name>.npy, a plain
float32 [21, H, W] array — what VOC12AffDataset.__getitem__ reads as --la_crf_dir / --ha_crf_dir (voc12/data.py:231-233).

Kept from the reference: --crf_iters is parsed and never used (t = 10).  Not kept: the reference loops over five exponents but passes
--alpha every time, writing the same file five times; here it is computed once.  Added: --alpha takes several values
(`--alpha 4 32`), all computed in one pass per image — the label sets share every kernel evaluation (wseg_amd.crf).
The CRF is the exact mean field; agreement with pydensecrf's permutohedral approximation is unmeasured.
"""
import argparse
import os

import numpy as np
import PIL.Image
import torch

from . import data as wdata
from .crf import crf_inference, labels_from_cams
from .safe_npy import load_pickled_npy
from .stage_io import WriteBehind

CRF_BILATERAL, CRF_GAUSSIAN, CRF_T = (80, 13, 10), (3, 3), 10          # aff_prepare.py:39-47, :34


def build_parser():
    parser = argparse.ArgumentParser()
    parser.add_argument("--infer_list", default="./VOC2012/ImageSets/Segmentation/trainaug.txt", type=str)
    parser.add_argument("--num_workers", default=8, type=int)
    parser.add_argument("--voc12_root", default='VOC2012', type=str)
    parser.add_argument("--cam_dir", default=None, type=str)
    parser.add_argument("--out_crf", default=None, type=str)
    parser.add_argument("--crf_iters", default=10, type=float)
    parser.add_argument("--alpha", default=[4.0], type=float, nargs="+")
    return parser


class _Images(torch.utils.data.Dataset):
    """decoded RGB image + CAM dictionary of every name (the loader's workers overlap the decode with the device)"""

    def __init__(self, names, voc12_root, cam_dir):
        self.names, self.root, self.cam_dir = names, voc12_root, cam_dir

    def __len__(self):
        return len(self.names)

    def __getitem__(self, idx):
        name = self.names[idx]
        with PIL.Image.open(wdata.get_img_path(name, self.root)) as im:
            img = torch.from_numpy(np.array(im.convert("RGB")))
        cams = load_pickled_npy(os.path.join(self.cam_dir, name + '.npy'))
        return name, img, {k: torch.from_numpy(np.asarray(v, np.float32)) for k, v in cams.items()}      # (keys as read: cam_planes judges them)


def main(argv=None):
    args = build_parser().parse_args(argv)
    if args.cam_dir is None or args.out_crf is None:
        raise SystemExit("aff_prepare needs --cam_dir and --out_crf")
    alphas = [float(a) for a in args.alpha]
    folders = [os.path.join(args.out_crf, '%.2f' % a) for a in alphas]
    for d in folders:
        os.makedirs(d, exist_ok=True)
    names = wdata.load_img_name_list(args.infer_list)              # both list formats: voc12/*.txt path lines and the devkit's bare names
    loader = torch.utils.data.DataLoader(_Images(names, args.voc12_root, args.cam_dir), shuffle=False, num_workers=args.num_workers,
                                         pin_memory=True, batch_size=None)
    dev = torch.device("cuda")

    def write(name, host):
        for s, d in enumerate(folders):
            np.save(os.path.join(d, name + '.npy'), host[s].numpy())

    with WriteBehind(write) as out:                 # the files of image i - 1 are written while image i computes
        for name, img, cams in loader:
            img = img.to(dev, non_blocking=True)
            labels = labels_from_cams(cams, alpha=alphas, size=tuple(img.shape[:2]), device=dev)
            out.submit(name, crf_inference(img, labels, t=CRF_T, bilateral=CRF_BILATERAL, gaussian=CRF_GAUSSIAN))


if __name__ == '__main__':
    main()
