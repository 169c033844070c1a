"""The contracts of csrc/eval.hip in a few lines of numpy, the per-threshold brute force they must agree with, and the adversarial
inputs both test files share (tests/test_eval_counts_host.py, tests/test_gpu_eval.py).  TEST INFRASTRUCTURE, not product code."""
import numpy as np


def emulate_conf(pred, gt):
    """wseg_eval_confusion: conf[min(gt, 21)][min(pred, 21)] += 1 where gt != 255"""
    pred, gt = np.asarray(pred).reshape(-1).astype(np.int64), np.asarray(gt).reshape(-1).astype(np.int64)
    conf = np.zeros((22, 22), np.int64)
    keep = gt != 255
    np.add.at(conf, (np.minimum(gt[keep], 21), np.minimum(pred[keep], 21)), 1)
    return conf


def emulate_hist(planes, src, gt, thr):
    """wseg_eval_curve: planes float32 [K, n] (or None), src 20 ints, thr float32 [T] -> hist[min(gt, 21)][c][k] += 1 where gt != 255, with
    m = the largest of the 20 scores (absent = 0.0), c = the lowest class attaining it, k = thresholds strictly below m (all in float32)"""
    gt = np.asarray(gt).reshape(-1).astype(np.int64)
    thr = np.asarray(thr, np.float32)
    scores = np.zeros((20, gt.size), np.float32)
    for c in range(20):
        if src[c] >= 0:
            scores[c] = np.asarray(planes[src[c]], np.float32).reshape(-1)
    m, c = scores.max(axis=0), scores.argmax(axis=0)               # (argmax: the first maximum)
    k = (thr[:, None] < m[None, :]).sum(axis=0)
    hist = np.zeros((22, 20, thr.size + 1), np.int64)
    keep = gt != 255
    np.add.at(hist, (np.minimum(gt[keep], 21), c[keep], k[keep]), 1)
    return hist


def brute_counts(images, thresholds):
    """The evaluator's loop (eval.py:31-52) once per threshold, as it stands there.  images: [(cam dict {class: [H, W]}, gt uint8 [H, W])];
    -> int64 (P, T, TP), each [len(thresholds), 21].  (An empty dictionary, which eval.py cannot read, scores 0 everywhere.)"""
    nt = len(thresholds)
    P, T, TP = (np.zeros((nt, 21), np.int64) for _ in range(3))
    for i, threshold in enumerate(thresholds):
        for d, gt in images:
            tensor = np.zeros((21,) + gt.shape, np.float32)
            for key in d:
                tensor[key + 1] = d[key]
            tensor[0, :, :] = threshold
            predict = np.argmax(tensor, axis=0).astype(np.uint8)
            cal = gt < 255
            mask = (predict == gt) * cal
            for c in range(21):
                P[i, c] += np.sum((predict == c) * cal)
                T[i, c] += np.sum((gt == c) * cal)
                TP[i, c] += np.sum((gt == c) * mask)
    return P, T, TP


def brute_mask_counts(pairs):
    """eval.py:41-52 on (pred, gt) uint8 pairs -> int64 (P, T, TP) [21]"""
    P, T, TP = (np.zeros(21, np.int64) for _ in range(3))
    for predict, gt in pairs:
        cal = gt < 255
        mask = (predict == gt) * cal
        for c in range(21):
            P[c] += np.sum((predict == c) * cal)
            T[c] += np.sum((gt == c) * cal)
            TP[c] += np.sum((gt == c) * mask)
    return P, T, TP


GRID = np.array([np.float32(i / 100.0) for i in range(-8, 70)], np.float32)       # the float32 threshold grid and a little beyond: ties with t


def gt_map(rng, shape, stray=True):
    gt = rng.integers(0, 21, shape).astype(np.uint8)
    gt[rng.random(shape) < 0.1] = 255
    if stray and gt.size > 1:
        gt.reshape(-1)[rng.integers(0, gt.size)] = 100            # a value in 21..254: counts towards P of its prediction only
        gt.reshape(-1)[0] = 255
    return gt


def adversarial_case(seed, shape=(20, 30)):
    """(cam dict, gt): scores on the float32 threshold grid (ties with t) including negatives; classes 3 and 7 bitwise equal; class 12 holds
    exact zeros where every other plane is negative, and class 0 is ABSENT: there the maximum is 0.0 and the lowest class attaining it is 0."""
    rng = np.random.default_rng(seed)
    a = GRID[rng.integers(0, GRID.size, shape)]
    b = GRID[rng.integers(0, GRID.size, shape)]
    zero = rng.random(shape) < 0.3
    a[zero] = -np.abs(a[zero]) - np.float32(0.01)
    b[zero] = np.where(rng.random(int(zero.sum())) < 0.5, np.float32(0.0), np.float32(-0.0))
    return {3: a, 7: a.copy(), 12: b}, gt_map(rng, shape)


def planes_and_src(d):
    """a cam dict as the kernel's arguments: (planes [K, H, W] float32 or None, src)"""
    keys = sorted(d)
    src = [-1] * 20
    for i, k in enumerate(keys):
        src[k] = i
    return (np.stack([np.asarray(d[k], np.float32) for k in keys]) if keys else None), src
