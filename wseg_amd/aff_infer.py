"""CLI of the reference's aff_infer.py (same flags) on the MI355X path: AffinityNet random-walk refinement of the CAM dictionaries
contrast_infer writes (<cam_dir>/<name>.npy) into pseudo masks <out_rw>/<name>.png.

The reference builds the dense [area, area] affinity matrix on the host, raises it to beta, normalises its columns, squares it logt
times (dense GEMMs) and multiplies the pooled CAM by it.  Here the same product is 2^logt applications of the sparse stencil
(csrc/affinity.hip), planes in LDS, and nothing crosses to the host but the final uint8 mask.  --alpha and --crf are accepted and
ignored, as in the reference (its bg score is a hard-coded 0.27 and its CRF block is commented out).
"""
import argparse
import os

import numpy as np
import PIL.Image
import torch

from . import _lib as L
from . import data as wdata
from . import synth
from .eval import DeviceEval, load_gt
from .safe_npy import load_pickled_npy
from .stage_io import WriteBehind, cam_planes, load_net

BG_SCORE = 0.27


@torch.no_grad()
def random_walk_image(model, img, cam_dict, orig_size, beta=8, logt=6, return_cam_rw=False):
    """img: the normalised image [1,3,H,W] (or [3,H,W]) at its original size; cam_dict {class (0..19): float [H,W]} (numpy or torch);
    returns the uint8 [H,W] device mask (and the walked stride-8 planes [21, dh, dw] with return_cam_rw).  Nothing synchronises."""
    dev = next(model.parameters()).device
    H, W = orig_size
    img = torch.as_tensor(img)
    if img.dim() == 3:
        img = img.unsqueeze(0)
    assert img.shape[0] == 1 and tuple(img.shape[2:]) == (H, W), (tuple(img.shape), orig_size)
    Hp, Wp = -(-H // 8) * 8, -(-W // 8) * 8
    dh, dw = Hp // 8, Wp // 8
    x = torch.zeros(1, 3, Hp, Wp, device=dev, dtype=torch.float32)               # F.pad to a multiple of 8 (aff_infer.py:72-75)
    x[:, :, :H, :W].copy_(img.to(dev, non_blocking=True))
    aff, (h, w, r) = model.affinities(x)
    assert (h, w) == (dh, dw), ((h, w), (dh, dw))
    P = aff.shape[1]
    area = h * w
    wgt = torch.empty(1, 2 * P, area, device=dev, dtype=torch.float32)
    rsum = torch.empty(1, area, device=dev, dtype=torch.float32)
    L.rw_prepare(aff, wgt, rsum, 1, h, w, r, beta)
    cams, idx, _ = cam_planes(cam_dict, (H, W), dev)
    pooled = torch.empty(21, dh, dw, device=dev, dtype=torch.float32)
    L.rw_pool(cams, [-1] + idx, BG_SCORE, pooled, H, W, dh, dw)
    cam_rw = torch.empty_like(pooled)
    L.random_walk(wgt, rsum, pooled, cam_rw, 1, 21, h, w, r, logt)
    pred = torch.empty(H, W, device=dev, dtype=torch.uint8)
    L.rw_finish(cam_rw, pred, 21, dh, dw, H, W)
    return (pred, cam_rw) if return_cam_rw else pred


def build_parser():
    parser = argparse.ArgumentParser()
    parser.add_argument("--weights", required=True, type=str)
    parser.add_argument("--network", default="wseg_amd.resnet38_aff", type=str)
    parser.add_argument("--infer_list", default="voc12/val.txt", type=str)
    parser.add_argument("--num_workers", default=8, type=int)
    parser.add_argument("--cam_dir", required=True, type=str)
    parser.add_argument("--voc12_root", default='VOC2012', type=str)
    parser.add_argument("--alpha", default=6, type=float)
    parser.add_argument("--out_rw", default='out_rw', type=str)
    parser.add_argument("--beta", default=8, type=int)
    parser.add_argument("--logt", default=6, type=int)
    parser.add_argument("--crf", default=False, type=bool)
    parser.add_argument("--precision", default=None, choices=[None, "bf16", "fp32", "bf16x3"])
    parser.add_argument("--gt_dir", default=None, type=str, help="evaluate while inferring: the mIoU of the masks against <gt_dir>/<name>.png")
    return parser


def main(argv=None):
    args = build_parser().parse_args(argv)
    os.makedirs(args.out_rw, exist_ok=True)
    model = load_net(args.network, args.weights, args.precision, synth.procedural_aff_state_dict)
    model.eval()
    model.cuda()

    ds = wdata.VOC12ImageDataset(args.infer_list, args.voc12_root, transform=[np.asarray, model.normalize, wdata.HWC_to_CHW])
    loader = torch.utils.data.DataLoader(ds, shuffle=False, num_workers=args.num_workers, pin_memory=True)

    def write(name, host):
        PIL.Image.fromarray(host.numpy()).save(os.path.join(args.out_rw, name + '.png'))

    ev = DeviceEval("cuda") if args.gt_dir is not None else None       # --gt_dir: confusion counts of every mask, on the device until the end
    with WriteBehind(write) as out:                 # the png of image i - 1 is written while image i computes
        for name, img in loader:
            name = name[0]
            H, W = img.shape[2], img.shape[3]
            cam = load_pickled_npy(os.path.join(args.cam_dir, name + '.npy'))
            gt = load_gt(args.gt_dir, name, (H, W)) if ev is not None else None
            pred = random_walk_image(model, img, cam, (H, W), args.beta, args.logt)
            if gt is not None:
                ev.add_masks(pred, torch.from_numpy(gt).pin_memory().to(pred.device, non_blocking=True))
            out.submit(name, pred)
    if ev is None:
        return None
    res = ev.mask_result()
    print('mIoU: %.3f' % res['mIoU'])
    return res


if __name__ == '__main__':
    main()
