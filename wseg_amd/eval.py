"""CAM mIoU evaluation — counterpart of the reference's eval.py:13-86,109-136 (the second half of the headline
metric, "CAM mIoU vs ref").  Two paths with the same results:

* host (the default, needs no GPU): numpy, like the reference (which forks 8 CPU processes); the per-image TP/P/T counting is
  vectorised with bincount instead.  `--curve` repeats the whole evaluation once per threshold, as the reference does.
* device (`--device`, or `DeviceEval` on tensors that are already there): the pixel counting runs in csrc/eval.hip into integer
  counters that stay on the device until the end, and the 60 thresholds of `--curve` take ONE pass: per pixel the kernel finds the
  largest foreground score m, the lowest class c that attains it and the number k of thresholds strictly below m; the arg-max
  over [t] ++ scores is c + 1 for the first k thresholds and background for the rest, so a histogram over (ground truth, c, k) and
  suffix sums over k (`counts_from_hist`) give every threshold's P / T / TP.  All integers: equal to the host path, not close to it.

Inputs are the files contrast_infer writes:
  type 'png'  : <predict_folder>/<name>.png (uint8 argmax)
  type 'npy'  : <predict_folder>/<name>.npy, a pickled dict class->float32[H,W]; prediction = argmax over
                [bg threshold t] ++ maps (eval.py:31-39), swept over t in --curve mode (eval.py:130-136).
Ground truth: <gt_folder>/<name>.png, label 255 ignored (eval.py:41-43).  IoU_c = TP_c / (T_c + P_c - TP_c).

    python -m wseg_amd.eval --list voc12/val.txt --predict_dir out_cam --gt_dir VOC2012/SegmentationClassAug --type npy --t 0.26
    python -m wseg_amd.eval --list voc12/val.txt --predict_dir out_cam --gt_dir VOC2012/SegmentationClassAug --type npy --curve --device
"""
import argparse
import os
import time

import numpy as np
import PIL.Image

from .data import load_img_name_list
from .safe_npy import load_pickled_npy

CATEGORIES = ['background', 'aeroplane', 'bicycle', 'bird', 'boat', 'bottle', 'bus', 'car', 'cat', 'chair', 'cow',
              'diningtable', 'dog', 'horse', 'motorbike', 'person', 'pottedplant', 'sheep', 'sofa', 'train', 'tvmonitor']
GT_ROWS, FG_CLASSES, MAX_THRESHOLDS = 22, 20, 64      # the counters' axes (include/wseg_hip.h WSEG_EVAL_*): gt row 21 = "21..254"


def load_prediction(folder, name, input_type, threshold, num_cls=21):
    if input_type == 'png':
        return np.array(PIL.Image.open(os.path.join(folder, name + '.png')))
    d = load_pickled_npy(os.path.join(folder, name + '.npy'))       # dict class -> float32[H,W] (restricted unpickler)
    h, w = list(d.values())[0].shape
    tensor = np.zeros((num_cls, h, w), np.float32)
    for key, v in d.items():
        tensor[key + 1] = v
    tensor[0, :, :] = threshold
    return np.argmax(tensor, axis=0).astype(np.uint8)


def do_eval(name_list, predict_folder, gt_folder, input_type='png', threshold=1.0, num_cls=21):
    TP = np.zeros(num_cls, np.int64); P = np.zeros(num_cls, np.int64); T = np.zeros(num_cls, np.int64)
    for name in name_list:
        predict = load_prediction(predict_folder, name, input_type, threshold, num_cls)
        gt = np.array(PIL.Image.open(os.path.join(gt_folder, name + '.png')))
        cal = gt < 255
        mask = (predict == gt) & cal
        P += np.bincount(predict[cal].astype(np.int64), minlength=num_cls)[:num_cls]
        T += np.bincount(gt[cal].astype(np.int64), minlength=num_cls)[:num_cls]
        TP += np.bincount(gt[mask].astype(np.int64), minlength=num_cls)[:num_cls]
    IoU = TP / (T + P - TP + 1e-10)
    T_TP = T / (TP + 1e-10)
    P_TP = P / (TP + 1e-10)
    FP_ALL = (P - TP) / (T + P - TP + 1e-10)
    FN_ALL = (T - TP) / (T + P - TP + 1e-10)
    out = {CATEGORIES[i]: IoU[i] * 100 for i in range(num_cls)}
    out['mIoU'] = float(np.mean(IoU) * 100)
    out['t_tp'] = float(np.mean(T_TP[1:])); out['p_tp'] = float(np.mean(P_TP[1:]))
    out['fp_all'] = float(np.mean(FP_ALL[1:])); out['fn_all'] = float(np.mean(FN_ALL[1:]))
    return out


# ---------------------------------------------------------------------------------------------- from counters to results (pure numpy)
def results_from_counts(P, T, TP, num_cls=21):
    """The dictionary do_eval returns, from integer P / T / TP of at least num_cls classes: the same float64 expressions on the same integers."""
    P, T, TP = (np.asarray(x, np.int64)[:num_cls] for x in (P, T, TP))
    IoU = TP / (T + P - TP + 1e-10)
    T_TP = T / (TP + 1e-10)
    P_TP = P / (TP + 1e-10)
    FP_ALL = (P - TP) / (T + P - TP + 1e-10)
    FN_ALL = (T - TP) / (T + P - TP + 1e-10)
    out = {CATEGORIES[i]: IoU[i] * 100 for i in range(num_cls)}
    out['mIoU'] = float(np.mean(IoU) * 100)
    out['t_tp'] = float(np.mean(T_TP[1:])); out['p_tp'] = float(np.mean(P_TP[1:]))
    out['fp_all'] = float(np.mean(FP_ALL[1:])); out['fn_all'] = float(np.mean(FN_ALL[1:]))
    return out


def counts_from_conf(conf):
    """conf [22, 22] (gt row x prediction column, row / column 21 = "21 and above") -> int64 (P, T, TP) of the 21 classes as do_eval counts
    them: P over all 22 rows (a stray gt value still counts towards its prediction), T over all 22 columns, TP the diagonal."""
    conf = np.asarray(conf).astype(np.int64).reshape(GT_ROWS, GT_ROWS)
    return conf.sum(axis=0)[:21], conf[:21].sum(axis=1), np.diagonal(conf)[:21].copy()


def counts_from_hist(hist):
    """hist [22, 20, T+1] (gt row, winning foreground class c, thresholds strictly below the winning score k) -> int64 (P, T, TP), each
    [T, 21]: at threshold i a pixel is predicted c + 1 when i < k and background otherwise, so the foreground counts are suffix sums over k."""
    hist = np.asarray(hist).astype(np.int64)
    assert hist.ndim == 3 and hist.shape[:2] == (GT_ROWS, FG_CLASSES), hist.shape
    nthr = hist.shape[2] - 1
    fg = np.cumsum(hist[:, :, ::-1], axis=2)[:, :, ::-1][:, :, 1:]        # fg[g, c, i] = sum over k > i
    total = hist.sum(axis=(1, 2))                                          # pixels per gt row
    bg = total[:, None] - fg.sum(axis=1)                                   # bg[g, i]
    P = np.zeros((nthr, 21), np.int64); T = np.zeros((nthr, 21), np.int64); TP = np.zeros((nthr, 21), np.int64)
    P[:, 0] = bg.sum(axis=0)
    P[:, 1:] = fg.sum(axis=0).T
    T[:] = total[:21]
    TP[:, 0] = bg[0]
    TP[:, 1:] = fg[np.arange(1, 21), np.arange(20)].T
    return P, T, TP


def curve_thresholds(thresholds=None):
    """The curve's thresholds as float32, cast exactly as `tensor[0, :, :] = threshold` casts them (default: eval.py:130-132, i / 100)."""
    thr = np.array([np.float32(t) for t in ([i / 100.0 for i in range(60)] if thresholds is None else thresholds)], np.float32)
    if not 1 <= thr.size <= MAX_THRESHOLDS:
        raise ValueError(f"{thr.size} thresholds: the device curve takes 1 to {MAX_THRESHOLDS}")
    if np.isnan(thr).any() or (np.diff(thr) < 0).any():
        raise ValueError("the thresholds must be non-decreasing after the cast to float32")
    return thr


class DeviceEval:
    """Evaluation counters on the device.  add_masks / add_cams enqueue one kernel on the current stream and return; nothing is read
    back before mask_result / curve_results / counts.  One instance holds a confusion matrix (masks) and a curve histogram (CAMs)."""

    def __init__(self, device, thresholds=None, num_cls=21):
        self.thr = curve_thresholds(thresholds)
        if not 1 <= num_cls <= 21:
            raise ValueError(f"num_cls={num_cls} outside 1..21")
        import torch
        from . import _lib as L
        from .stage_io import cam_planes
        self._torch, self._L, self._cam_planes = torch, L, cam_planes
        self.num_cls = num_cls
        self.conf = torch.zeros(GT_ROWS, GT_ROWS, dtype=torch.int64, device=device)
        self.hist = torch.zeros(GT_ROWS, FG_CLASSES, self.thr.size + 1, dtype=torch.int64, device=device)
        self.device = self.hist.device               # with its index ("cuda" -> cuda:0), as tensors report it

    def _u8(self, x, what):
        torch = self._torch
        if not torch.is_tensor(x):
            x = torch.from_numpy(np.ascontiguousarray(x))
        if x.dtype != torch.uint8:
            raise ValueError(f"{what} must be uint8, got {x.dtype}")
        return x.to(self.device, non_blocking=True).contiguous()

    def add_masks(self, pred, gt):
        pred, gt = self._u8(pred, "pred"), self._u8(gt, "gt")
        if pred.shape != gt.shape or gt.numel() == 0:
            raise ValueError(f"prediction {tuple(pred.shape)} against ground truth {tuple(gt.shape)}")
        self._L.eval_confusion(pred, gt, gt.numel(), self.conf)

    def add_cams(self, cams, gt, classes=None):
        """cams: {class 0..19: [H, W]} (torch or numpy: infer_image's cam_dict, or what load_pickled_npy returns; empty = every score 0),
        or a [K, H, W] array holding the planes of `classes` (default 0..K-1), which crosses to the device in one copy.  Views into one
        float32 device tensor are read in place (stage_io.cam_planes)."""
        torch = self._torch
        gt = self._u8(gt, "gt")
        n = gt.numel()
        if not isinstance(cams, dict):
            if not torch.is_tensor(cams):
                cams = torch.from_numpy(np.ascontiguousarray(cams, np.float32))
            cams = cams.to(self.device, non_blocking=True)
            cams = {int(c): cams[i] for i, c in enumerate(range(len(cams)) if classes is None else classes)}
        if n == 0:
            raise ValueError(f"ground truth {tuple(gt.shape)} is empty")
        planes, idx, _ = self._cam_planes(cams, gt.shape, self.device, FG_CLASSES)      # (planes stays referenced until the launch is enqueued)
        if planes is None:
            self._L.eval_curve(None, 0, 0, idx, gt, n, self.thr, self.hist)
        else:
            self._L.eval_curve(planes.data_ptr(), n, planes.shape[0], idx, gt, n, self.thr, self.hist)

    def counts(self, which):
        """int64 (P, T, TP): 'mask' -> [num_cls] each, 'curve' -> [thresholds, num_cls] each.  Reads the counters (synchronises)."""
        if which == 'mask':
            return tuple(x[:self.num_cls] for x in counts_from_conf(self.conf.cpu().numpy()))
        if which == 'curve':
            return tuple(x[:, :self.num_cls] for x in counts_from_hist(self.hist.cpu().numpy()))
        raise ValueError(which)

    def mask_result(self):
        return results_from_counts(*self.counts('mask'), num_cls=self.num_cls)

    def curve_results(self):
        P, T, TP = self.counts('curve')
        return [results_from_counts(P[i], T[i], TP[i], num_cls=self.num_cls) for i in range(self.thr.size)]


def load_gt(gt_dir, name, size=None):
    """<gt_dir>/<name>.png as a uint8 [H, W] array (palette indices); a missing file or a size other than `size` (H, W) is an error."""
    path = os.path.join(gt_dir, name + '.png')
    if not os.path.exists(path):
        raise FileNotFoundError(f"ground truth of image {name} is missing: {path}")
    gt = np.array(PIL.Image.open(path))
    if gt.dtype != np.uint8 or gt.ndim != 2 or (size is not None and gt.shape != tuple(size)):
        raise ValueError(f"{path}: a uint8 label map of size {size} is expected, got {gt.dtype} {gt.shape}")
    return gt


# ---------------------------------------------------------------------------------------------- command line
def curve_lines(mious, thresholds=None):
    """The lines --curve prints for the mIoU values of the thresholds (default i / 100), and the best (threshold, mIoU): the first maximum."""
    ts = [i / 100.0 for i in range(len(mious))] if thresholds is None else list(thresholds)
    lines = ['%d/%d background score: %.3f\tmIoU: %.3f%%' % (i, len(ts), t, m) for i, (t, m) in enumerate(zip(ts, mious))]
    best = None
    for t, m in zip(ts, mious):
        if best is None or m > best[1]:
            best = (t, m)
    return lines, best


def writelog(filepath, metric, comment):
    """eval.py:89-106: append a timestamp, a tab and the comment; the metric as `key:value  ` pairs; a line of '='."""
    with open(filepath, 'a') as f:
        f.write(time.strftime("%Y-%m-%d %H:%M:%S", time.localtime()))
        f.write('\t%s\n' % comment)
        f.write(''.join('%s:%s  ' % (k, v) for k, v in metric.items()) + '\n')
        f.write('=====================================\n')


class _EvalFiles:
    """One image's prediction and ground truth, read in a DataLoader worker: ('png': pred, gt) or ('npy': classes, planes [K, H, W], gt)."""

    def __init__(self, names, predict_dir, gt_dir, input_type):
        self.names, self.predict_dir, self.gt_dir, self.input_type = list(names), predict_dir, gt_dir, input_type

    def __len__(self):
        return len(self.names)

    def __getitem__(self, i):
        name = self.names[i]
        if self.input_type == 'png':
            pred = np.array(PIL.Image.open(os.path.join(self.predict_dir, name + '.png')))
            return pred, load_gt(self.gt_dir, name, pred.shape)
        d = load_pickled_npy(os.path.join(self.predict_dir, name + '.npy'))
        keys = sorted(d)
        gt = load_gt(self.gt_dir, name, np.shape(d[keys[0]]) if keys else None)        # (a missing or ill-sized ground truth is named here)
        planes = np.stack([np.asarray(d[k], np.float32) for k in keys]) if keys else np.zeros((0,) + gt.shape, np.float32)
        return [int(k) for k in keys], planes, gt


def device_eval_files(names, predict_dir, gt_dir, input_type, thresholds=None, num_workers=8, device="cuda"):
    """One pass over the files into a DeviceEval: the masks' confusion counts ('png') or the curve histogram of `thresholds` ('npy')."""
    import torch
    ev = DeviceEval(device, thresholds)
    loader = torch.utils.data.DataLoader(_EvalFiles(names, predict_dir, gt_dir, input_type), batch_size=None, shuffle=False,
                                         num_workers=num_workers, pin_memory=True)
    for item in loader:
        if input_type == 'png':
            ev.add_masks(*item)
        else:
            keys, planes, gt = item
            ev.add_cams(planes, gt, classes=keys)
    return ev


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--list", default='voc12/train.txt', type=str)
    ap.add_argument("--predict_dir", default="./out_rw", type=str)
    ap.add_argument("--gt_dir", default='VOC2012/SegmentationClassAug', type=str)
    ap.add_argument("--type", default='png', choices=['npy', 'png'], type=str)
    ap.add_argument("--t", default=None, type=float)
    ap.add_argument("--curve", action="store_true")
    ap.add_argument("--logfile", default=None, type=str)        # (the reference defaults to ./evallog.txt; here nothing is written unless asked)
    ap.add_argument("--comment", default='', type=str)
    ap.add_argument("--device", action="store_true", help="count on the GPU (csrc/eval.hip); --curve then takes one pass over the files")
    ap.add_argument("--num_workers", default=8, type=int, help="--device: DataLoader workers that read and decode the files")
    a = ap.parse_args(argv)
    names = load_img_name_list(a.list)              # both list formats: voc12/*.txt path lines and the devkit's bare names
    if not a.curve:
        t = a.t if a.t is not None else 1.0
        if not a.device:
            res = do_eval(names, a.predict_dir, a.gt_dir, a.type, t)
        else:
            ev = device_eval_files(names, a.predict_dir, a.gt_dir, a.type, [t], a.num_workers)
            res = ev.mask_result() if a.type == 'png' else ev.curve_results()[0]
        print('mIoU: %.3f' % res['mIoU'])
        if a.logfile is not None:
            writelog(a.logfile, res, a.comment)
        return res
    if not a.device:
        best, mious = None, []
        for i in range(60):                                          # eval.py:130-136: t = 0.00 .. 0.59
            t = i / 100.0
            res = do_eval(names, a.predict_dir, a.gt_dir, a.type, t)
            print('%d/60 background score: %.3f\tmIoU: %.3f%%' % (i, t, res['mIoU']))
            if best is None or res['mIoU'] > best[1]:
                best = (t, res['mIoU'])
            mious.append(res['mIoU'])                               # (kept for --logfile only)
    else:
        ev = device_eval_files(names, a.predict_dir, a.gt_dir, a.type, None, a.num_workers)
        mious = [r['mIoU'] for r in ev.curve_results()] if a.type == 'npy' else [ev.mask_result()['mIoU']] * 60     # (a png does not depend on t)
        lines, best = curve_lines(mious)
        print('\n'.join(lines))
    print('best background score: %.3f\tmIoU: %.3f%%' % best)
    if a.logfile is not None:
        writelog(a.logfile, {'mIoU': mious}, a.comment)
    return best


if __name__ == '__main__':
    main()
