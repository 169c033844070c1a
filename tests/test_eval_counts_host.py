"""Host: the device evaluator's arithmetic without a device.  A numpy emulation of the two kernels' contracts (tests/eval_emul.py) fed
through wseg_amd.eval.counts_from_hist / counts_from_conf must EQUAL the evaluator's per-threshold loop (eval.py:31-52) on adversarial
inputs: integers, so equality; plus threshold validation and the --logfile / --comment block."""
import re

import numpy as np
import pytest

from tests import eval_emul as E
from wseg_amd import eval as weval

THR60 = weval.curve_thresholds()


def _hist_of(images, thr):
    hist = np.zeros((22, 20, len(thr) + 1), np.int64)
    for d, gt in images:
        planes, src = E.planes_and_src(d)
        hist += E.emulate_hist(None if planes is None else planes.reshape(len(planes), -1), src, gt, thr)
    return hist


def _assert_counts_equal(got, want):
    for name, g, w in zip("P T TP".split(), got, want):
        assert g.dtype == np.int64 and np.array_equal(g, w), (name, np.argwhere(g != w)[:5])


@pytest.mark.parametrize("seed", range(6))
def test_curve_counts_equal_the_per_threshold_loop(seed):
    """ties with t (scores on the float32 threshold grid), two bitwise-equal planes, an absent class 0 below a present plane of exact zeros,
    negative scores, ground truth with 255 and a stray 100 — at all 60 thresholds, two images of different sizes accumulated"""
    images = [E.adversarial_case(seed), E.adversarial_case(100 + seed, (7, 13))]
    assert any((gt == 100).any() for _, gt in images) and any((gt == 255).any() for _, gt in images)
    d, gt = images[0]
    zero_max = (d[12] == 0) & (d[3] < 0)                          # the maximum over the 20 classes is the absent classes' 0.0 and class 12's
    assert zero_max.sum() > 20 and (d[3] == d[7]).all()
    assert np.isin(d[3][d[3] >= 0], THR60).any()
    hist = _hist_of(images, THR60)
    assert hist[:, 0, 0].sum() > 0 and hist[:, 0, 1:].sum() == 0 and hist[:, 12, 0].sum() == 0        # the absent class 0 takes every tie at zero
    got = weval.counts_from_hist(hist)
    _assert_counts_equal(got, E.brute_counts(images, [i / 100.0 for i in range(60)]))
    assert got[0][:, 4].sum() > 0 and got[0][:, 13].sum() > 0 and got[0][:, 8].sum() == 0      # 7 never beats its bitwise copy 3


@pytest.mark.parametrize("thr", [[0.26], [-0.05, 0.0, 0.0, 0.3, 0.3, 0.31], [i / 100.0 for i in range(64)]])
def test_curve_counts_other_threshold_lists(thr):
    """T = 1, equal neighbours with a negative threshold, T = 64"""
    images = [E.adversarial_case(11)]
    got = weval.counts_from_hist(_hist_of(images, weval.curve_thresholds(thr)))
    _assert_counts_equal(got, E.brute_counts(images, thr))


def test_curve_counts_of_an_empty_dictionary():
    """all 20 classes absent: m = 0, c = 0 — class 1 is predicted below threshold 0 and background from 0 on"""
    gt = E.gt_map(np.random.default_rng(2), (5, 9))
    thr = [-0.5, 0.0, 0.5]
    got = weval.counts_from_hist(_hist_of([({}, gt)], weval.curve_thresholds(thr)))
    _assert_counts_equal(got, E.brute_counts([({}, gt)], thr))
    cal = int((gt < 255).sum())
    assert got[0][0].tolist() == [0, cal] + [0] * 19 and got[0][1].tolist() == [cal] + [0] * 20


def test_mask_counts_equal_the_loop():
    """predictions >= 21 and stray ground-truth values: P counts them by prediction, T and TP drop them"""
    rng = np.random.default_rng(5)
    pairs = []
    for shape in ((20, 30), (7, 13)):
        pred = rng.integers(0, 21, shape).astype(np.uint8)
        pred[rng.random(shape) < 0.05] = 37
        pred[rng.random(shape) < 0.05] = 255
        gt = E.gt_map(rng, shape)
        gt[0, 1], pred[0, 1] = 37, 37                               # equal and out of range: no TP
        gt[0, 2], pred[0, 2] = 100, 4
        pairs.append((pred, gt))
    got = weval.counts_from_conf(sum(E.emulate_conf(p, g) for p, g in pairs))
    _assert_counts_equal(got, E.brute_mask_counts(pairs))


def test_results_from_counts_are_do_evals(tmp_path):
    import PIL.Image
    rng = np.random.default_rng(9)
    names = ["a", "b"]
    pairs = []
    for n in names:
        pred, gt = rng.integers(0, 21, (12, 17)).astype(np.uint8), E.gt_map(rng, (12, 17))
        PIL.Image.fromarray(pred).save(tmp_path / (n + ".png"))
        (tmp_path / "gt").mkdir(exist_ok=True)
        PIL.Image.fromarray(gt).save(tmp_path / "gt" / (n + ".png"))
        pairs.append((pred, gt))
    want = weval.do_eval(names, str(tmp_path), str(tmp_path / "gt"), "png")
    got = weval.results_from_counts(*weval.counts_from_conf(sum(E.emulate_conf(p, g) for p, g in pairs)))
    assert list(got) == list(want) and all(got[k] == want[k] for k in want)


@pytest.mark.parametrize("thr", [[0.3, 0.2], [0.0, 0.5, 0.4999], [], [i / 100.0 for i in range(65)], [0.1, float("nan")]])
def test_bad_thresholds_are_refused(thr):
    with pytest.raises(ValueError):
        weval.curve_thresholds(thr)
    with pytest.raises(ValueError):
        weval.DeviceEval("cpu", thresholds=thr)                   # (refused before anything touches a device)


def test_thresholds_are_cast_like_the_evaluator():
    thr = weval.curve_thresholds()
    t = np.zeros((1, 1, 1), np.float32)
    for i in range(60):
        t[0, :, :] = i / 100.0
        assert thr[i] == t[0, 0, 0]
    assert thr.dtype == np.float32 and thr.size == 60
    assert weval.curve_thresholds([0.1, 0.1 + 1e-12]).tolist() == [np.float32(0.1)] * 2       # equal after the cast: accepted


def _tiny_set(tmp_path):
    import PIL.Image
    names = ["2007_000001", "2007_000002"]
    for d in ("gt", "npy"):
        (tmp_path / d).mkdir()
    for i, n in enumerate(names):
        d, gt = E.adversarial_case(40 + i, (9, 11))
        PIL.Image.fromarray(gt).save(tmp_path / "gt" / (n + ".png"))
        np.save(tmp_path / "npy" / (n + ".npy"), d, allow_pickle=True)
    (tmp_path / "list.txt").write_text("\n".join(names) + "\n")
    return names, ["--list", str(tmp_path / "list.txt"), "--predict_dir", str(tmp_path / "npy"), "--gt_dir", str(tmp_path / "gt"), "--type", "npy"]


def test_host_output_is_unchanged_and_logfile_block(tmp_path, capsys):
    names, argv = _tiny_set(tmp_path)
    want = [weval.do_eval(names, str(tmp_path / "npy"), str(tmp_path / "gt"), "npy", i / 100.0) for i in range(60)]
    res = weval.main(argv + ["--t", "0.26"])
    assert capsys.readouterr().out == "mIoU: %.3f\n" % want[26]["mIoU"] and res == want[26]
    best = weval.main(argv + ["--curve"])
    lines = ["%d/60 background score: %.3f\tmIoU: %.3f%%" % (i, i / 100.0, want[i]["mIoU"]) for i in range(60)]
    ibest = int(np.argmax([w["mIoU"] for w in want]))             # (the first maximum, as `>` keeps it)
    lines.append("best background score: %.3f\tmIoU: %.3f%%" % (ibest / 100.0, want[ibest]["mIoU"]))
    assert capsys.readouterr().out == "\n".join(lines) + "\n" and best == (ibest / 100.0, want[ibest]["mIoU"])
    assert sorted(p.name for p in tmp_path.iterdir()) == ["gt", "list.txt", "npy"]           # no log file unless asked for

    log = tmp_path / "evallog.txt"
    weval.main(argv + ["--t", "0.26", "--logfile", str(log), "--comment", "first run"])
    weval.main(argv + ["--curve", "--logfile", str(log), "--comment", "the curve"])
    capsys.readouterr()
    got = log.read_text().split("\n")
    stamp = r"\d{4}-\d\d-\d\d \d\d:\d\d:\d\d"
    assert re.fullmatch(stamp + "\tfirst run", got[0]) and re.fullmatch(stamp + "\tthe curve", got[3])
    assert got[1] == "".join("%s:%s  " % (k, v) for k, v in want[26].items())
    assert got[1].startswith("background:%s  aeroplane:%s  " % (want[26]["background"], want[26]["aeroplane"]))
    assert got[4] == "mIoU:%s  " % [w["mIoU"] for w in want]
    assert got[2] == got[5] == "=====================================" and got[6:] == [""]


def test_the_device_cli_loader_names_a_bad_ground_truth(tmp_path):
    """the files `--device` reads in its workers: a missing or ill-sized ground truth is an error that names the file"""
    import PIL.Image
    names, _ = _tiny_set(tmp_path)
    files = weval._EvalFiles(names, str(tmp_path / "npy"), str(tmp_path / "gt"), "npy")
    keys, planes, gt = files[0]
    assert keys == [3, 7, 12] and planes.shape == (3, 9, 11) and planes.dtype == np.float32 and gt.shape == (9, 11)
    PIL.Image.fromarray(np.zeros((9, 12), np.uint8)).save(tmp_path / "gt" / (names[0] + ".png"))
    with pytest.raises(ValueError, match=names[0]):
        files[0]
    (tmp_path / "gt" / (names[1] + ".png")).unlink()
    with pytest.raises(FileNotFoundError, match=names[1]):
        files[1]
