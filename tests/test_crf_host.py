"""Dense CRF without a GPU: the float64 oracle (tests/crf_exact.py) against the specification's own constants and identities, the
background rules, the synthetic picture, and the two CLIs' parsers against the reference's flags and defaults."""
import numpy as np
import pytest
import torch

from tests import crf_exact as X


def _case(H=12, W=17, seed=5):
    from wseg_amd import synth
    img = synth.synthetic_rgb_image(H, W, seed).numpy()
    cams = {k: v.numpy() for k, v in synth.synthetic_cam_dict(H, W, [3, 11, 14], seed).items()}
    return img, cams


def test_oracle_unary_values():
    U = X.unary(np.array([[0, 3], [20, 3]], np.uint8))
    assert U.dtype == torch.float32 and tuple(U.shape) == (4, 21)
    assert abs(float(U[0, 0]) - 0.356675) < 5e-7 and abs(float(U[0, 1]) - 4.199705) < 5e-7
    assert int((U < 1).sum()) == 4 and float(U[1, 3]) == float(U[0, 0]) and float(U[2, 20]) == float(U[0, 0])


def test_oracle_q_rows_sum_to_one_and_crf_moves_labels():
    img, cams = _case()
    lab = X.label_tensor(cams, 12, 17, bg_score=0.26)
    r = X.crf(img, np.stack([lab, X.label_tensor(cams, 12, 17, alpha=4)]), t=3, bilateral=(50, 5, 10.0))
    assert tuple(r["Q"].shape) == (2, 21, 12, 17)
    assert float((r["Q"].sum(1) - 1).abs().max()) < 1e-12
    one = X.crf(img, lab, t=3, bilateral=(50, 5, 10.0))          # the label sets do not interact
    assert float((one["Q"][0] - r["Q"][0]).abs().max()) < 1e-12


def test_oracle_bilateral_on_constant_colour_is_the_gaussian():
    img = np.full((9, 14, 3), 77, np.uint8)
    fb, fg = X.features(img, 4.0, 13.0), X.features(img, 4.0)
    Q = torch.rand(9 * 14, 5, dtype=torch.float64, generator=torch.Generator().manual_seed(1))
    nb, ng = X.norm(fb), X.norm(fg)
    assert float((nb - ng).abs().max()) < 1e-14
    assert float((X.filt(fb, nb, Q) - X.filt(fg, ng, Q)).abs().max()) < 1e-13


def test_background_rules():
    from wseg_amd import crf
    assert crf.bg_rule(bg_score=0.26) == (0, 0.26) and crf.bg_rule(alpha=32) == (1, 32.0)
    with pytest.raises(ValueError):
        crf.bg_rule()
    with pytest.raises(ValueError):
        crf.bg_rule(0.26, 4)
    with pytest.raises(RuntimeError):                            # device only: no CPU fallback
        crf.labels_from_cams({0: np.zeros((2, 2), np.float32)}, bg_score=0.26, device="cpu")
    # the oracle's rule: tensor[0] is still zero inside the max, and a higher exponent shrinks the background
    img, cams = _case()
    l4, l32 = X.label_tensor(cams, 12, 17, alpha=4), X.label_tensor(cams, 12, 17, alpha=32)
    assert set(np.unique(l4).tolist()) <= {0, 4, 12, 15}
    assert bool(np.all((l32 == 0) <= (l4 == 0)))
    mx = np.max(np.stack([cams[k] for k in cams]), 0)
    assert np.array_equal(l4 == 0, np.power(1 - mx, np.float32(4)) >= mx)


def test_synthetic_rgb_image_is_piecewise_smooth():
    from wseg_amd import synth
    a, b = synth.synthetic_rgb_image(40, 56, 1), synth.synthetic_rgb_image(40, 56, 1)
    assert a.dtype == torch.uint8 and tuple(a.shape) == (40, 56, 3) and torch.equal(a, b)
    assert not torch.equal(a, synth.synthetic_rgb_image(40, 56, 2))
    d = (a[:, 1:].int() - a[:, :-1].int()).abs().amax(2)
    assert float((d <= 25).float().mean()) > 0.9 and int(d.max()) > 60      # flat regions with +-12 texture, and real edges


def test_parsers_take_the_reference_flags_and_defaults():
    from wseg_amd import aff_prepare, contrast_infer
    a = aff_prepare.build_parser().parse_args([])
    assert (a.infer_list, a.num_workers, a.voc12_root, a.cam_dir, a.out_crf, a.crf_iters, a.alpha) == \
        ("./VOC2012/ImageSets/Segmentation/trainaug.txt", 8, "VOC2012", None, None, 10, [4.0])
    a = aff_prepare.build_parser().parse_args(["--infer_list", "l", "--num_workers", "2", "--voc12_root", "r", "--cam_dir", "c",
                                               "--out_crf", "o", "--crf_iters", "5", "--alpha", "4", "32"])
    assert a.alpha == [4.0, 32.0] and a.crf_iters == 5 and a.cam_dir == "c"
    assert aff_prepare.build_parser().parse_args(["--alpha", "8"]).alpha == [8.0]
    c = contrast_infer.build_parser().parse_args(["--weights", "w", "--out_crf", "d"])
    assert (c.out_crf, c.crf_iters, c.out_cam_pred_alpha, c.infer_list, c.num_workers, c.voc12_root) == \
        ("d", 10, 0.26, "voc12/train.txt", 8, "VOC2012")
    assert (contrast_infer.CRF_BG_SCORE, contrast_infer.CRF_BILATERAL, contrast_infer.CRF_T) == (0.26, (50, 5, 10), 10)
    assert (aff_prepare.CRF_BILATERAL, aff_prepare.CRF_T) == ((80, 13, 10), 10)
