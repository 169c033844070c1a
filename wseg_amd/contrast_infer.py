"""CLI of the reference's contrast_infer.py (same flags, :19-31) on the MI355X path.  Writes the same files:
<out_cam>/<name>.npy (pickled dict class -> float32[H,W] of the present classes, :82-90) and
<out_cam_pred>/<name>.png (uint8 argmax, :97-99), and <out_crf>/<name>.png (:102-134): the uint8 arg-max of the dense CRF on the CAM
labels with a constant background score of 0.26, sxy 50 / srgb 5, 10 iterations.  Two quirks of the reference are kept: the CRF's
background score is the constant 0.26 whatever --out_cam_pred_alpha says, and --crf_iters is parsed and never used (t = 10).  The CRF is wseg_amd.crf: exact mean field on the device; agreement with pydensecrf's permutohedral
approximation is unmeasured."""
import argparse
import os

import numpy as np
import PIL.Image
import torch

from . import data as wdata
from . import synth
from .crf import crf_inference, labels_from_cams
from .eval import DeviceEval, curve_lines, load_gt
from .infer import infer_image
from .stage_io import WriteBehind, load_net

CRF_BG_SCORE, CRF_BILATERAL, CRF_GAUSSIAN, CRF_T = 0.26, (50, 5, 10), (3, 3), 10        # contrast_infer.py:104, 121-122, 113


def crf_prediction(img_u8, cam_dict):
    """contrast_infer.py:104-112 `_crf`: uint8 [H, W] device arg-max of the CRF on the labels of [0.26] ++ cam_dict"""
    labels = labels_from_cams(cam_dict, bg_score=CRF_BG_SCORE, size=tuple(img_u8.shape[:2]), device=img_u8.device)
    _, amax = crf_inference(img_u8, labels, t=CRF_T, bilateral=CRF_BILATERAL, gaussian=CRF_GAUSSIAN, return_argmax=True)
    return amax[0]


def build_parser():
    parser = argparse.ArgumentParser()
    parser.add_argument("--weights", required=True, type=str)
    parser.add_argument("--network", default="wseg_amd.resnet38_contrast", type=str)
    parser.add_argument("--infer_list", default="voc12/train.txt", type=str)
    parser.add_argument("--num_workers", default=8, type=int)
    parser.add_argument("--voc12_root", default='VOC2012', type=str)
    parser.add_argument("--out_cam", default=None, type=str)
    parser.add_argument("--out_crf", default=None, type=str)
    parser.add_argument("--out_cam_pred", default=None, type=str)
    parser.add_argument("--out_cam_pred_alpha", default=0.26, type=float)
    parser.add_argument("--crf_iters", default=10, type=float)
    parser.add_argument("--labels", default="voc12/cls_labels.npy", type=str)
    parser.add_argument("--precision", default=None, choices=[None, "bf16", "fp32", "bf16x3"])
    parser.add_argument("--gt_dir", default=None, type=str,
                        help="evaluate while inferring: <gt_dir>/<name>.png -> the 60-threshold CAM curve, the mIoU of the arg-max masks (and of the CRF masks)")
    return parser


def main(argv=None):
    args = build_parser().parse_args(argv)

    model = load_net(args.network, args.weights, args.precision, synth.procedural_state_dict)
    model.eval()
    model.cuda()

    ds = wdata.VOC12ClsDatasetMSF(args.infer_list, args.voc12_root, args.labels, scales=[0.5, 1.0, 1.5, 2.0],
                                  inter_transform=[np.asarray, model.normalize, wdata.HWC_to_CHW])
    loader = torch.utils.data.DataLoader(ds, shuffle=False, num_workers=args.num_workers, pin_memory=True)
    def write(img_name, host):
        host_pred, host_crf, host_cams = host
        if host_crf is not None:
            PIL.Image.fromarray(host_crf.numpy()).save(os.path.join(args.out_crf, img_name + '.png'))
        if host_cams is not None:
            np.save(os.path.join(args.out_cam, img_name + '.npy'), {k: v.numpy() for k, v in host_cams.items()})
        if args.out_cam_pred is not None:
            PIL.Image.fromarray(host_pred.numpy()).save(os.path.join(args.out_cam_pred, img_name + '.png'))

    for d in (args.out_cam, args.out_cam_pred, args.out_crf):
        if d is not None:
            os.makedirs(d, exist_ok=True)
    # --gt_dir: the evaluator's counters are fed from the device tensors of each image (wseg_amd.eval.DeviceEval: one kernel per add, no
    # synchronisation, read back once after the loop), so the background score can be chosen without writing a single dictionary
    ev_curve = ev_pred = ev_crf = None
    if args.gt_dir is not None:
        ev_curve, ev_pred = DeviceEval("cuda"), DeviceEval("cuda")
        ev_crf = DeviceEval("cuda") if args.out_crf is not None else None
    # One image behind: the device work of image i is enqueued (nothing in infer_image synchronises) and only then are the files of
    # image i - 1 written (the reference's loop, contrast_infer.py:52-99, syncs per image on `.cpu()`).
    with WriteBehind(write) as out:
        for it, (img_name, img_list, label) in enumerate(loader):
            img_name, label = img_name[0], label[0]
            with PIL.Image.open(wdata.get_img_path(img_name, args.voc12_root)) as im:      # (header only: the reference decodes the image again for its shape)
                W, H = im.size
                rgb = np.array(im.convert("RGB")) if args.out_crf is not None else None
            gt = load_gt(args.gt_dir, img_name, (H, W)) if args.gt_dir is not None else None
            norm_cam, pred, cam_dict = infer_image(model, img_list, label, (H, W), args.out_cam_pred_alpha)
            crf_pred = None
            if rgb is not None:
                crf_pred = crf_prediction(torch.from_numpy(rgb).pin_memory().to(pred.device, non_blocking=True), cam_dict)
            if gt is not None:
                gt = torch.from_numpy(gt).pin_memory().to(pred.device, non_blocking=True)
                ev_curve.add_cams(cam_dict, gt)
                ev_pred.add_masks(pred, gt)
                if crf_pred is not None:
                    ev_crf.add_masks(crf_pred, gt)
            out.submit(img_name, (pred, crf_pred, cam_dict if args.out_cam is not None else None))
    if ev_curve is None:
        return None
    mious = [r['mIoU'] for r in ev_curve.curve_results()]
    lines, best = curve_lines(mious)
    print('\n'.join(lines))
    print('best background score: %.3f\tmIoU: %.3f%%' % best)
    out = {'curve': mious, 'best': best, 'pred': ev_pred.mask_result(), 'crf': ev_crf.mask_result() if ev_crf is not None else None}
    print('cam_pred (alpha %.2f) mIoU: %.3f' % (args.out_cam_pred_alpha, out['pred']['mIoU']))
    if out['crf'] is not None:
        print('crf mIoU: %.3f' % out['crf']['mIoU'])
    return out


if __name__ == '__main__':
    main()
