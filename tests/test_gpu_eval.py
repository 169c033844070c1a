"""GPU: the evaluation counters of csrc/eval.hip (wseg_eval_confusion, wseg_eval_curve) through the C ABI against the numpy emulation of
their contracts (tests/eval_emul.py, itself pinned to the evaluator's per-threshold loop in tests/test_eval_counts_host.py), and
wseg_amd.eval.DeviceEval against the reference evaluator's IoU tables.  Integer counters: every comparison is equality."""
import os

import numpy as np
import pytest
import torch

from tests import eval_emul as E

pytestmark = pytest.mark.gpu

THR = {"T1": [0.26], "T60": [i / 100.0 for i in range(60)], "T64": [i / 100.0 - 0.02 for i in range(64)],
       "ties": [-0.05, 0.0, 0.0, 0.3, 0.3, 0.31, 0.55]}                        # equal neighbours and a negative threshold


def _thr(name):
    from wseg_amd import eval as weval
    return weval.curve_thresholds(THR[name])


def _random_case(seed, shape, K):
    """K present classes with scores on the float32 threshold grid (ties with t and between planes, negatives), gt with 255 and a stray value"""
    rng = np.random.default_rng(seed)
    classes = sorted(rng.choice(20, K, replace=False).tolist())
    return {c: E.GRID[rng.integers(0, E.GRID.size, shape)] for c in classes}, E.gt_map(rng, shape)


def _run_curve(d, gt, thr, hist=None, pad=0, shift=0):
    """wseg_eval_curve on a cam dict -> the int64 histogram.  pad: plane stride = H*W + pad with NaN in the padding; shift: planes and gt
    start `shift` elements into their buffers (off the 16-byte alignment: the scalar path)."""
    from wseg_amd import _lib as L
    planes, src = E.planes_and_src(d)
    n = gt.size
    if hist is None:
        hist = torch.zeros(22, 20, len(thr) + 1, dtype=torch.int64, device="cuda")
    gbuf = torch.full((n + shift,), 7, dtype=torch.uint8, device="cuda")
    gbuf[shift:] = torch.from_numpy(gt.reshape(-1)).cuda()
    K = 0 if planes is None else len(planes)
    pbuf = None
    if K:
        pbuf = torch.full((shift + K * (n + pad),), float("nan"), device="cuda")
        pbuf[shift:].view(K, n + pad)[:, :n] = torch.from_numpy(planes.reshape(K, n)).cuda()
    L.eval_curve(None if pbuf is None else pbuf[shift:], n + pad, K, src, gbuf[shift:], n, thr, hist)
    return hist


CURVE_CASES = [
    ((1, 1), 1, "T60", 0, 0), ((1, 1), 0, "T1", 0, 0), ((7, 13), 0, "T60", 0, 0), ((7, 13), 3, "T1", 0, 0), ((7, 13), 1, "T64", 0, 0),
    ((20, 30), 3, "ties", 0, 0), ((20, 30), 20, "T60", 0, 0),
    ((20, 30), 11, "T60", 0, 0), ((20, 30), 12, "T60", 0, 0),          # either side of the 64 KiB of LDS: workgroup histogram / straight global adds
    ((64, 67), 3, "T64", 0, 0), ((64, 67), 20, "T64", 0, 0), ((64, 67), 1, "T60", 0, 0),
    ((64, 67), 3, "T60", 8, 0), ((64, 67), 3, "T60", 3, 0), ((64, 67), 3, "T60", 0, 1),          # padded strides (vector / scalar), shifted bases
    ((375, 500), 3, "T60", 0, 0),
]


@pytest.mark.parametrize("shape,K,tname,pad,shift", CURVE_CASES, ids=lambda v: str(v).replace(" ", ""))
def test_eval_curve_equals_the_emulation(shape, K, tname, pad, shift):
    thr = _thr(tname)
    d, gt = _random_case(31 * shape[0] + 7 * K + len(tname), shape, K)
    planes, src = E.planes_and_src(d)
    want = E.emulate_hist(None if planes is None else planes.reshape(K, -1), src, gt, thr)
    got = _run_curve(d, gt, thr, pad=pad, shift=shift).cpu().numpy()
    assert got.sum() == int((gt != 255).sum()) and np.array_equal(got, want), np.argwhere(got != want)[:5]


@pytest.mark.parametrize("shift", [0, 1])
def test_eval_curve_without_a_workgroup_histogram_on_shared_cells(shift):
    """20 present planes (the global-add path) with smooth maps: whole waves count into one cell, some lanes ignored, runs of a few cells"""
    rng = np.random.default_rng(6)
    shape = (64, 67)
    d = {c: np.full(shape, np.float32(0.01 * c), np.float32) for c in range(20)}
    d[5] = np.repeat(E.GRID[rng.integers(0, E.GRID.size, (64, 1))], 67, axis=1)           # one value per row: runs of 67 equal pixels
    gt = np.repeat(rng.integers(0, 21, (8, 67)), 8, axis=0).astype(np.uint8)
    gt[rng.random(shape) < 0.2] = 255
    thr = _thr("T60")
    planes, src = E.planes_and_src(d)
    got = _run_curve(d, gt, thr, shift=shift).cpu().numpy()
    assert np.array_equal(got, E.emulate_hist(planes.reshape(20, -1), src, gt, thr))


@pytest.mark.parametrize("seed", [0, 1])
def test_eval_curve_adversarial_inputs(seed):
    """ties with t, two bitwise-equal planes, the absent class 0 against a present plane of exact (+/-) zeros, negative scores -> the counts
    of the evaluator's own loop at all 60 thresholds"""
    from wseg_amd import eval as weval
    images = [E.adversarial_case(seed), E.adversarial_case(50 + seed, (7, 13))]
    thr = _thr("T60")
    hist = None
    for d, gt in images:
        hist = _run_curve(d, gt, thr, hist)
    hist = hist.cpu().numpy()
    assert hist[:, 0, 0].sum() > 0 and hist[:, 12, 0].sum() == 0 and hist[:, 7].sum() == 0
    for g, w in zip(weval.counts_from_hist(hist), E.brute_counts(images, THR["T60"])):
        assert np.array_equal(g, w)


def _run_conf(pred, gt, conf=None, shift=0):
    from wseg_amd import _lib as L
    n = gt.size
    if conf is None:
        conf = torch.zeros(22, 22, dtype=torch.int64, device="cuda")
    bufs = []
    for a in (pred, gt):
        b = torch.full((n + shift,), 3, dtype=torch.uint8, device="cuda")
        b[shift:] = torch.from_numpy(a.reshape(-1)).cuda()
        bufs.append(b[shift:])
    L.eval_confusion(bufs[0], bufs[1], n, conf)
    return conf


def _mask_case(seed, shape):
    rng = np.random.default_rng(seed)
    pred = rng.integers(0, 21, shape).astype(np.uint8)
    pred[rng.random(shape) < 0.05] = 21
    pred[rng.random(shape) < 0.05] = 255                            # predictions >= 21: column 21
    return pred, E.gt_map(rng, shape)


@pytest.mark.parametrize("shape,shift", [((1, 1), 0), ((7, 13), 0), ((20, 30), 0), ((64, 67), 0), ((64, 67), 1), ((375, 500), 0)])
def test_eval_confusion_equals_the_emulation(shape, shift):
    pred, gt = _mask_case(shape[0], shape)
    got = _run_conf(pred, gt, shift=shift).cpu().numpy()
    want = E.emulate_conf(pred, gt)
    assert np.array_equal(got, want) and (shape == (1, 1) or got[:, 21].sum() > 0)


def test_ignored_ground_truth_counts_nothing():
    d, _ = _random_case(3, (20, 30), 3)
    gt = np.full((20, 30), 255, np.uint8)
    assert int(_run_curve(d, gt, _thr("T60")).abs().sum()) == 0
    assert int(_run_conf(_mask_case(3, (20, 30))[0], gt).abs().sum()) == 0


def test_accumulation_and_run_to_run_equality():
    """three images of different sizes into one buffer = the sum of three separate runs; the same sequence twice is bit-equal"""
    thr = _thr("T60")
    cases = [_random_case(20 + i, s, k) for i, (s, k) in enumerate((((7, 13), 1), ((64, 67), 3), ((20, 30), 12)))]
    masks = [_mask_case(30 + i, s) for i, s in enumerate(((7, 13), (64, 67), (20, 30)))]
    runs = []
    for _ in range(2):
        hist = conf = None
        for d, gt in cases:
            hist = _run_curve(d, gt, thr, hist)
        for p, g in masks:
            conf = _run_conf(p, g, conf)
        runs.append((hist.cpu().numpy(), conf.cpu().numpy()))
    assert np.array_equal(runs[0][0], runs[1][0]) and np.array_equal(runs[0][1], runs[1][1])
    assert np.array_equal(runs[0][0], sum(_run_curve(d, gt, thr).cpu().numpy() for d, gt in cases))
    assert np.array_equal(runs[0][1], sum(_run_conf(p, g).cpu().numpy() for p, g in masks))


def test_bad_arguments_are_refused():
    from wseg_amd import _lib as L
    n = 64
    planes = torch.zeros(3, n, device="cuda")
    gt = torch.zeros(n, dtype=torch.uint8, device="cuda")
    hist = torch.zeros(22, 20, 3, dtype=torch.int64, device="cuda")
    conf = torch.zeros(22, 22, dtype=torch.int64, device="cuda")
    src = [-1] * 20
    src[4], src[9] = 0, 2
    ok = dict(planes=planes, stride=n, nplanes=3, src=src, gt=gt, n=n, thr=[0.1, 0.2], hist=hist)
    bad = [dict(thr=[0.2, 0.1]), dict(thr=[0.1, float("nan")]), dict(thr=[]), dict(thr=[0.01 * i for i in range(65)]),
           dict(src=src[:9] + [3] + src[10:]), dict(src=src[:9] + [-2] + src[10:]), dict(hist=None), dict(gt=None), dict(planes=None),
           dict(n=0), dict(stride=n - 1)]
    for kw in bad:
        a = {**ok, **kw}
        h = hist.data_ptr() if "thr" in kw else a["hist"]          # (an address: the binding's own size check would answer first)
        with pytest.raises(RuntimeError, match=r"wseg_eval_curve failed \(-1\)"):
            L.eval_curve(a["planes"], a["stride"], a["nplanes"], a["src"], a["gt"], a["n"], a["thr"], h)
    for a in ((None, gt, n, conf), (gt, None, n, conf), (gt, gt, n, None), (gt, gt, 0, conf)):
        with pytest.raises(RuntimeError, match="eval_confusion"):
            L.eval_confusion(*a)
    L.eval_curve(*[ok[k] for k in ("planes", "stride", "nplanes", "src", "gt", "n", "thr", "hist")])
    torch.cuda.synchronize()
    assert int(hist.sum()) == n and int(conf.sum()) == 0            # the refused calls touched nothing


@pytest.mark.parametrize("shape,classes", [((7, 13), [3, 5, 8]), ((20, 30), [0, 1, 2]), ((7, 13), [11]), ((9, 11), [2, 4, 6])])
def test_views_into_one_tensor_are_read_in_place(monkeypatch, shape, classes):
    """infer_image's dictionary (views into one [20, H, W] tensor; gaps between the classes, H*W odd or no multiple of 4): add_cams hands the
    kernel the address of the lowest view, the stride H*W and the views' plane numbers — no stacked copy — and counts what the copy counts"""
    from wseg_amd import _lib as L, eval as weval
    rng = np.random.default_rng(len(classes) + shape[0])
    n = shape[0] * shape[1]
    full = torch.full((20,) + shape, float("nan"), device="cuda")
    d = {c: E.GRID[rng.integers(0, E.GRID.size, shape)] for c in classes}
    for c, v in d.items():
        full[c] = torch.from_numpy(v).cuda()
    gt = E.gt_map(rng, shape)
    calls = []
    real = L.eval_curve
    monkeypatch.setattr(L, "eval_curve", lambda planes, stride, nplanes, src, *rest: (calls.append((planes, stride, nplanes, list(src))), real(planes, stride, nplanes, src, *rest))[1])
    ev = weval.DeviceEval("cuda")                                  # ("cuda", as every caller passes it: the views report cuda:0)
    ev.add_cams({c: full[c] for c in classes}, torch.from_numpy(gt).cuda())
    planes, stride, nplanes, src = calls[0]
    assert planes == full[classes[0]].data_ptr() and stride == n and nplanes == classes[-1] - classes[0] + 1
    assert src == [c - classes[0] if c in classes else -1 for c in range(20)]
    ev.add_cams(full[classes[0]:classes[-1] + 1][[c - classes[0] for c in classes]].clone(), gt, classes=classes)      # one [K, H, W] array: its planes in place too
    planes, stride, nplanes, src = calls[1]
    assert stride == n and nplanes == len(classes) and sorted(s for s in src if s >= 0) == list(range(len(classes)))
    p_, src_ = E.planes_and_src(d)
    assert np.array_equal(ev.hist.cpu().numpy(), 2 * E.emulate_hist(p_.reshape(len(classes), -1), src_, gt, ev.thr))


def test_device_eval_reproduces_the_reference_tables(golden_dir):
    """DeviceEval on the contents of eval_ref.npz: the IoU tables the reference's own eval.py produced (png, and npy at 0.10 / 0.26 / 0.50),
    to the 1e-9 of test_eval_matches_the_reference_evaluator; dictionaries that are views into one [20, H, W] tensor (what infer_image
    returns) count exactly as separate tensors and as numpy dictionaries do."""
    from wseg_amd import eval as weval
    g = np.load(os.path.join(golden_dir, "eval_ref.npz"))
    names = [str(n) for n in g["names"]]
    cats = weval.CATEGORIES + ["mIoU"]
    evs = {k: weval.DeviceEval("cuda", thresholds=[0.1, 0.26, 0.5]) for k in ("views", "separate", "numpy")}
    for n in names:
        gt, keys, cams = g[f"gt/{n}"], [int(k) for k in g[f"camkeys/{n}"]], g[f"cams/{n}"]
        full = torch.full((20,) + gt.shape, -1.0, device="cuda")
        for k, v in zip(keys, cams):
            full[k] = torch.from_numpy(v).cuda()
        gt_dev = torch.from_numpy(gt).cuda()
        evs["views"].add_cams({k: full[k] for k in keys}, gt_dev)
        evs["separate"].add_cams({k: full[k].clone() for k in keys}, gt_dev)
        evs["numpy"].add_cams({k: v for k, v in zip(keys, cams)}, gt)
        evs["views"].add_masks(torch.from_numpy(g[f"pred/{n}"]).cuda(), gt_dev)
        evs["numpy"].add_masks(g[f"pred/{n}"], gt)
    res = evs["views"].curve_results()
    for i, t in enumerate((0.1, 0.26, 0.5)):
        np.testing.assert_allclose([res[i][c] for c in cats], g["iou/npy_t%.2f" % t], rtol=0, atol=1e-9)
    np.testing.assert_allclose([evs["views"].mask_result()[c] for c in cats], g["iou/png"], rtol=0, atol=1e-9)
    for other in ("separate", "numpy"):
        for a, b in zip(evs["views"].counts("curve"), evs[other].counts("curve")):
            assert np.array_equal(a, b)
    for a, b in zip(evs["views"].counts("mask"), evs["numpy"].counts("mask")):
        assert np.array_equal(a, b)
    assert sorted(res[0]) == sorted(cats + ["t_tp", "p_tp", "fp_all", "fn_all"])
