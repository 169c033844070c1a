"""GPU: evaluation on the device from the command lines.  A tiny VOC tree (procedural weights, three small images, random ground-truth
PNGs with ignore pixels) -> `eval --curve --device` prints what `eval --curve` prints; `contrast_infer --gt_dir` and `aff_infer --gt_dir`
report, from the device tensors, exactly what the host evaluator computes afterwards from the files they wrote."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SIZES = [(96, 128), (75, 101), (40, 57)]
NAMES = [f"2007_00002{i}" for i in range(len(SIZES))]


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    """the VOC tree, and ONE contrast_infer run with every output directory and --gt_dir: (paths, what main returned)"""
    import PIL.Image
    from wseg_amd import contrast_infer, synth
    tmp = tmp_path_factory.mktemp("evalcli")
    root = tmp / "VOC2012"
    (root / "JPEGImages").mkdir(parents=True)
    (tmp / "gt").mkdir()
    rng = np.random.default_rng(4)
    labels = synth.synthetic_labels(len(NAMES), 3)
    for i, (n, hw) in enumerate(zip(NAMES, SIZES)):
        PIL.Image.fromarray(rng.integers(0, 256, hw + (3,), dtype=np.uint8)).save(root / "JPEGImages" / (n + ".jpg"))
        present = [0] + [c + 1 for c in range(20) if float(labels[i][c]) > 0]
        coarse = rng.choice(present + [255], size=(-(-hw[0] // 8), -(-hw[1] // 8)))            # 8 x 8 blocks of the image's classes, bg and ignore
        gt = np.kron(coarse, np.ones((8, 8), np.int64))[:hw[0], :hw[1]].astype(np.uint8)
        PIL.Image.fromarray(gt).save(tmp / "gt" / (n + ".png"))
    lst = tmp / "list.txt"
    lst.write_text("\n".join(f"/JPEGImages/{n}.jpg /SegmentationClassAug/{n}.png" for n in NAMES) + "\n")
    np.save(tmp / "cls_labels.npy", {n: labels[i].numpy() for i, n in enumerate(NAMES)}, allow_pickle=True)
    base = ["--weights", "procedural", "--infer_list", str(lst), "--voc12_root", str(root), "--labels", str(tmp / "cls_labels.npy"),
            "--num_workers", "0", "--precision", "fp32"]
    out = contrast_infer.main(base + ["--out_cam", str(tmp / "cam"), "--out_cam_pred", str(tmp / "pred"), "--out_crf", str(tmp / "crf"),
                                      "--gt_dir", str(tmp / "gt")])
    return tmp, lst, base, out


def test_contrast_infer_reports_what_the_host_evaluator_computes(tree):
    from wseg_amd import eval as weval
    tmp, lst, base, out = tree
    for i in range(60):
        want = weval.do_eval(NAMES, str(tmp / "cam"), str(tmp / "gt"), "npy", i / 100.0)
        assert abs(out["curve"][i] - want["mIoU"]) <= 1e-9, (i, out["curve"][i], want["mIoU"])
    ibest = int(np.argmax(out["curve"]))
    assert out["best"] == (ibest / 100.0, out["curve"][ibest])
    for key, d in (("pred", "pred"), ("crf", "crf")):
        want = weval.do_eval(NAMES, str(tmp / d), str(tmp / "gt"), "png")
        assert sorted(out[key]) == sorted(want) and all(abs(out[key][k] - want[k]) <= 1e-9 for k in want), key
    assert len(set(round(m, 6) for m in out["curve"])) > 1          # the curve moves with the threshold on this data


def test_contrast_infer_evaluates_without_writing_anything(tree, capsys):
    from wseg_amd import contrast_infer
    tmp, lst, base, out = tree
    before = sorted(p.name for p in tmp.iterdir())
    again = contrast_infer.main(base + ["--gt_dir", str(tmp / "gt")])
    assert again["curve"] == out["curve"] and again["pred"] == out["pred"] and again["crf"] is None
    assert sorted(p.name for p in tmp.iterdir()) == before
    lines = capsys.readouterr().out.strip().split("\n")
    assert lines[:60] == ["%d/60 background score: %.3f\tmIoU: %.3f%%" % (i, i / 100.0, m) for i, m in enumerate(out["curve"])]
    assert lines[60] == "best background score: %.3f\tmIoU: %.3f%%" % out["best"] and lines[61].startswith("cam_pred (alpha 0.26) mIoU: ")


def test_eval_cli_on_the_device_prints_the_host_lines(tree, capsys):
    from wseg_amd import eval as weval
    tmp, lst, base, out = tree
    argv = ["--list", str(lst), "--predict_dir", str(tmp / "cam"), "--gt_dir", str(tmp / "gt"), "--type", "npy"]
    host_best = weval.main(argv + ["--curve"])
    host = capsys.readouterr().out
    dev_best = weval.main(argv + ["--curve", "--device", "--num_workers", "2", "--logfile", str(tmp / "log.txt"), "--comment", "dev"])
    dev = capsys.readouterr().out
    assert dev == host and dev_best == host_best and len(host.strip().split("\n")) == 61
    assert (tmp / "log.txt").read_text().split("\n")[1] == "mIoU:%s  " % out["curve"]
    for extra, kind in ((["--type", "npy", "--t", "0.26"], "cam"), (["--type", "png"], "pred")):
        a = ["--list", str(lst), "--predict_dir", str(tmp / kind), "--gt_dir", str(tmp / "gt")] + extra
        h, d = weval.main(a), weval.main(a + ["--device", "--num_workers", "0"])
        assert h == d
    capsys.readouterr()


def test_aff_infer_reports_the_miou_of_its_masks(tree):
    from wseg_amd import aff_infer, eval as weval
    tmp, lst, base, out = tree
    res = aff_infer.main(["--weights", "procedural", "--infer_list", str(lst), "--voc12_root", str(tmp / "VOC2012"), "--cam_dir", str(tmp / "cam"),
                          "--out_rw", str(tmp / "rw"), "--num_workers", "0", "--precision", "fp32", "--gt_dir", str(tmp / "gt")])
    want = weval.do_eval(NAMES, str(tmp / "rw"), str(tmp / "gt"), "png")
    assert sorted(res) == sorted(want) and all(abs(res[k] - want[k]) <= 1e-9 for k in want)


def test_a_missing_ground_truth_is_named(tree, tmp_path):
    from wseg_amd import aff_infer
    tmp, lst, base, out = tree
    with pytest.raises(FileNotFoundError, match=NAMES[0]):
        aff_infer.main(["--weights", "procedural", "--infer_list", str(lst), "--voc12_root", str(tmp / "VOC2012"), "--cam_dir", str(tmp / "cam"),
                        "--out_rw", str(tmp_path / "rw"), "--num_workers", "0", "--precision", "fp32", "--gt_dir", str(tmp_path / "nowhere")])
