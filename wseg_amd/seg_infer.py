"""The DeepLab stage's test script (segmentation/experiment/SEAM_deeplabv1_resnet38/test.py) on the MI355X path: multi-scale, flipped
inference of a `deeplabv1` ResNet-38 checkpoint into label PNGs <out_png>/<name>.png, with the mIoU while inferring (--gt_dir).

Per image the reference runs the net on 6 scales x {plain, x-flipped}, resamples each result twice (to the scaled input, then to the
original size), un-flips, averages, and takes softmax and arg-max: 24 resize launches and 12 full-size intermediates.  Here the plain
and the flipped image of one scale are ONE N = 2 backbone + head pass (6 passes per image), and everything after the stride-8 logits is
one launch (csrc/seg.hip, wseg_seg_fuse); nothing crosses to the host but the final uint8 map.

The scaled inputs are made on the host from the normalised float image (the reference normalises first, then cv2.resize(fx, fy,
INTER_CUBIC)): PIL bicubic at size (round(h r), round(w r)) — cv2's sizing rounds half to even as Python's round does.  cv2 itself is
not available offline: parity with the reference is pinned from the list of scaled images onward, the resize is not.

--crf refines the softmax with the fully connected CRF of segmentation/lib/utils/DenseCRF.py:dense_crf (unary_from_softmax, Gaussian
sxy 3 compat 3, bilateral sxy 32 srgb 13 compat 10, one iteration).  Three things to know: the reference's own test.py calls
dense_crf_from_deeplabv2, which does not exist in its utils/DenseCRF.py, so `dense_crf` is taken as the specification; this is the EXACT
mean field over all pixel pairs, not pydensecrf's permutohedral lattice; agreement with pydensecrf is unmeasured (the package is not
available offline).
"""
import argparse
import os

import numpy as np
import PIL.Image
import torch

from . import arch
from . import _lib as L
from . import data as wdata
from . import synth
from .eval import DeviceEval, load_gt
from .stage_io import WriteBehind, load_net

TEST_MULTISCALE = (0.5, 0.75, 1.0, 1.25, 1.5, 1.75)       # config.py:48 of the experiment
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def scaled_size(h, w, rate):
    """cv2.resize(img, None, fx=rate, fy=rate)'s output size: round half to even of the product (375 x 0.5 -> 188, 375 x 1.5 -> 562)."""
    return int(round(h * rate)), int(round(w * rate))


def scaled_inputs(img_hwc, scales=TEST_MULTISCALE):
    """The normalised float32 [H, W, 3] image at every scale, PIL bicubic per channel (mode F): a list of float32 [3, h', w'] arrays."""
    img = np.ascontiguousarray(img_hwc, np.float32)
    H, W = img.shape[:2]
    out = []
    for r in scales:
        h, w = scaled_size(H, W, r)
        if h < 1 or w < 1:
            raise ValueError(f"scale {r} of a {H} x {W} image is empty")
        out.append(np.stack([np.asarray(PIL.Image.fromarray(np.ascontiguousarray(img[..., c])).resize((w, h), wdata.BICUBIC), np.float32) for c in range(3)]))
    return out


def denormalise_u8(img_hwc):
    """utils/imutils.py img_denorm + astype(uint8) of test.py:97: the image the CRF's bilateral term sees"""
    x = np.asarray(img_hwc, np.float32) * np.asarray(STD, np.float32) + np.asarray(MEAN, np.float32)
    return (x * 255).clip(0, 255).astype(np.uint8)


@torch.no_grad()
def coarse_passes(model, scaled, flip=True):
    """The net on every scaled input [3, ih, iw] (numpy or torch), the plain and the x-flipped image of one scale as one N = 2 batch:
    the list of L.SegPass in the reference's order (scale ascending, plain before flipped).  Nothing synchronises."""
    dev = next(model.parameters()).device
    passes = []
    for x in scaled:
        x = torch.as_tensor(x)
        x = (x if x.is_cuda else x.pin_memory()).to(dev, non_blocking=True).float()
        ih, iw = int(x.shape[1]), int(x.shape[2])
        batch = torch.stack([x, x.flip(2)]) if flip else x.unsqueeze(0)
        rows, (fh, fw) = model.coarse_logits(batch)
        passes += [L.SegPass(rows, arch.SEG_CLS_ROWS, n, fh, fw, ih, iw, n == 1) for n in range(batch.shape[0])]
    return passes


@torch.no_grad()
def fuse_image(model, scaled, size, flip=True, want=("amax",)):
    """test.py:71-104 for one image: scaled = the scaled inputs, size = the original (H, W).  Returns a dict with the uint8 [H, W] device
    label map `amax` and whichever of `mean` [21, H, W], `prob` [21, H, W], `margin` [H, W] (float32) `want` names."""
    H, W = size
    passes = coarse_passes(model, scaled, flip)
    dev = passes[0].rows.device
    out = {"amax": torch.empty(H, W, device=dev, dtype=torch.uint8)}
    for k in ("mean", "prob"):
        if k in want:
            out[k] = torch.empty(arch.NUM_CLASSES, H, W, device=dev, dtype=torch.float32)
    if "margin" in want:
        out["margin"] = torch.empty(H, W, device=dev, dtype=torch.float32)
    with torch.cuda.device(dev):
        L.seg_fuse(passes, H, W, arch.NUM_CLASSES, out["amax"], out.get("mean"), out.get("prob"), out.get("margin"))
    return out


@torch.no_grad()
def infer_image(model, img_hwc, scales=TEST_MULTISCALE, flip=True, crf=False, scaled=None):
    """The uint8 [H, W] device label map of one normalised float32 [H, W, 3] image (scaled: its scaled inputs when a loader worker has made them)."""
    H, W = img_hwc.shape[:2]
    scaled = scaled_inputs(img_hwc, scales) if scaled is None else scaled
    if not crf:
        return fuse_image(model, scaled, (H, W), flip)["amax"]
    from .crf import crf_inference_from_probs
    prob = fuse_image(model, scaled, (H, W), flip, want=("prob",))["prob"]
    img_u8 = torch.from_numpy(denormalise_u8(img_hwc)).to(prob.device, non_blocking=True)
    return crf_inference_from_probs(img_u8, prob, t=1, return_argmax=True)[1]


class _Scaled:
    """loader transform: normalised HWC image -> (image, its scaled inputs); the workers decode and resize, the device is the main process's"""

    def __init__(self, scales):
        self.scales = tuple(scales)

    def __call__(self, img):
        return img, scaled_inputs(img, self.scales)


def build_parser():
    parser = argparse.ArgumentParser()
    parser.add_argument("--weights", required=True, type=str, help="a deeplabv1 ResNet-38 state_dict (.pth), or `procedural`")
    parser.add_argument("--network", default="wseg_amd.deeplabv1_resnet38", type=str)
    parser.add_argument("--infer_list", default="voc12/val.txt", type=str)
    parser.add_argument("--voc12_root", default='VOC2012', type=str)
    parser.add_argument("--scales", default=list(TEST_MULTISCALE), type=float, nargs="+", help="TEST_MULTISCALE of the experiment's config")
    parser.add_argument("--no_flip", action="store_true", help="TEST_FLIP off: one pass per scale")
    parser.add_argument("--crf", action="store_true",
                        help="refine the softmax with the dense CRF of utils/DenseCRF.py:dense_crf (one iteration).  The reference's test.py calls "
                             "dense_crf_from_deeplabv2, which its checkout does not define, so dense_crf is the specification; this is the exact "
                             "mean field, not pydensecrf's lattice; agreement with pydensecrf is unmeasured")
    parser.add_argument("--out_png", default=None, type=str, help="label PNGs <out_png>/<name>.png, as the reference's dataset.save_result writes")
    parser.add_argument("--gt_dir", default=None, type=str, help="evaluate while inferring: the mIoU of the label maps against <gt_dir>/<name>.png")
    parser.add_argument("--precision", default=None, choices=[None, "bf16", "fp32", "bf16x3"])
    parser.add_argument("--num_workers", default=8, type=int)
    return parser


def main(argv=None):
    args = build_parser().parse_args(argv)
    if args.out_png is not None:
        os.makedirs(args.out_png, exist_ok=True)
    model = load_net(args.network, args.weights, args.precision, synth.procedural_seg_state_dict)
    model.eval()
    model.cuda()

    ds = wdata.VOC12ImageDataset(args.infer_list, args.voc12_root, transform=[np.asarray, model.normalize, _Scaled(args.scales)])
    loader = torch.utils.data.DataLoader(ds, shuffle=False, num_workers=args.num_workers, batch_size=None)

    def write(name, host):
        if args.out_png is not None:
            PIL.Image.fromarray(host.numpy()).save(os.path.join(args.out_png, name + '.png'))

    ev = DeviceEval("cuda") if args.gt_dir is not None else None       # --gt_dir: confusion counts of every map, on the device until the end
    with WriteBehind(write) as out:                 # the png of image i - 1 is written while image i computes
        for name, (img, scaled) in loader:
            img = np.asarray(img)
            H, W = img.shape[:2]
            gt = load_gt(args.gt_dir, name, (H, W)) if ev is not None else None
            pred = infer_image(model, img, args.scales, not args.no_flip, args.crf, scaled=scaled)
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
