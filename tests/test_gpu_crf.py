"""Dense CRF on the GPU (csrc/crf.hip, wseg_amd/crf.py) against the float64 restatement of the specification (tests/crf_exact.py).

How the bars are set (the convention of tests/test_gpu_loss_kernels.py: derived from the kernel's arithmetic, safety factor 2, never
fitted to a run).  U32 = 2^-24.  One all-pairs sum T_i = sum_j k_ij x_j has only non-negative terms; the kernel errs in three places:
  * the exponent: integer differences and their squared sums are exact; the two constants (3 roundings each), one product and one fma
    make it relatively 5 U32 off, so k is relatively 5 U32 A off (A = |fi - fj|^2 / 2 in nats) — summed: 5 U32 T2_i with
    T2_i = sum_j k_ij A_ij x_j, which the oracle returns (`moment=True`); on the test pictures T2 / T <= 2.0
  * v_exp_f32: 1 ulp = 2 U32, relative
  * the sum: an f32 fma chain (v_mfma_f32_16x16x4_f32) in two levels, 256 sources per first-level sum, N / 256 first-level sums joined
    in a second chain.  Each rounding is at most U32 of the partial sum; with independent roundings the error of an n-term chain of
    like terms has standard deviation U32 sqrt(n) T / 3 (partial sums grow linearly), and the bar takes 4 sigma:
    R_ACC(N) = (4/3) U32 (sqrt(min(N, 256)) + sqrt(N / 256))          [64x88: 1.6e-6; 375x500: 3.4e-6]
    (the worst case N U32 would be 1.1e-2 at 375x500 and is never approached by sums of positive terms)
  n_i = 1/sqrt(T_i + 1e-20) carries half the sum's relative error plus two roundings.  A filter output F = n_i sum_j k_ij n_j Q_j
  carries the sum's error, n_i's, and — taken at full weight although it averages out over j — the largest n_j's, plus the roundings of
  n_j Q_j and of the final product.  The separable Gaussian is two short chains (41 taps each at sxy = 3, same 4-sigma model) with expf
  weights.  Its window is NOT part of the bar: the oracle sums all pairs, and whatever a window drops has to fit under the relative
  bar plus GAUSS_FLOOR, the one absolute term — a third (1 / w_g) of one f32 rounding of the smallest logit magnitude the filter
  can feed, |-U| >= 0.3567: an error below it cannot move a logit by one rounding.
Ten iterations: every iteration adds a fresh, independent logit error e = w_b dF_b + w_g dF_g; the mean-field map carries an earlier
error forward with gain <= 1 on these pictures (the oracle's own float32 run drifts 9.4e-6 from float64 in ten iterations, no more than
its per-iteration rounding predicts), so the bar is sqrt(t) e, times the safety factor.  It must come out <= 5e-4 (asserted): a path
that needs more is not f32-faithful.

CPU check of the cases below with the committed generator (synthetic_rgb_image; float32 torch against float64, ten iterations):
  40x56 seed 1 (50, 5):   max |dlogit| 9.4e-6, 0 arg-max mismatches, min top-2 margin 1.06e-2, 0 px under 1e-3, 6.5 % of labels changed
  64x88 seed 2 (80, 13):  5.9e-6, 0, 8.6e-3, 0, 18.6 %        40x56 seed 1 (80, 13): 4.9e-6, 0, 6.0e-2, 0, 6.1 %
  64x88 seed 2 (50, 5):   7.3e-6, 0, 8.2e-3, 0, 17.8 %
  100x125 seed 3 (50, 5): 7.2e-6, 0, 1.09e-2, 0, 14.0 %       100x125 seed 4 (80, 13): 6.6e-6, 0, 6.5e-3, 0, 15.2 %   (CPU only: 50 s each)
"""
import math
import os
import threading

import numpy as np
import pytest
import torch

from tests import crf_exact as X

pytestmark = pytest.mark.gpu

U32 = 2.0 ** -24
SAFETY = 2.0
LOGIT_BAR_CEILING = 5e-4
PARAMS = [(50, 5), (80, 13)]
SEEDS = {(40, 56): 1, (64, 88): 2, (37, 53): 7, (375, 500): 9}


def r_acc(N):
    return 4.0 / 3.0 * U32 * (math.sqrt(min(N, 256)) + math.sqrt(N / 256.0))


R_GAUSS = 4.0 / 3.0 * U32 * 2 * math.sqrt(41) + 2 * U32                # two 41-tap chains, expf weights
GAUSS_FLOOR = U32 * 0.356675 / 3.0


def rel_n(N, abar):
    """relative bar of n_i (before the safety factor); abar = T2 / T of the normalisation sum"""
    return 0.5 * (r_acc(N) + 2 * U32 + 5 * U32 * abar) + 2 * U32


def filter_bar(N, n, T, T2, abar_n):
    """bar of F = n_i T_i, elementwise [N, C]"""
    rn = float(rel_n(N, abar_n).max())
    return SAFETY * (n[:, None] * ((r_acc(N) + 4 * U32) * T + 5 * U32 * T2) + 2 * rn * n[:, None] * T)


def _picture(H, W):
    from wseg_amd import synth
    seed = SEEDS[(H, W)]
    img = synth.synthetic_rgb_image(H, W, seed)
    cams = synth.synthetic_cam_dict(H, W, [3, 11, 14], seed)
    return img, cams


def _planes(H, W, S, kind, seed):
    """[S * 21, H, W] float32: a soft distribution per pixel, or a one-hot one"""
    g = torch.Generator().manual_seed(seed)
    if kind == "soft":
        return torch.softmax(3 * torch.randn(S, 21, H, W, generator=g), 1).reshape(S * 21, H, W).float()
    idx = torch.randint(0, 21, (S, 1, H, W), generator=g)
    return torch.zeros(S, 21, H, W).scatter_(1, idx, 1.0).reshape(S * 21, H, W)


@pytest.mark.parametrize("size", [(40, 56), (37, 53), (64, 88)])
@pytest.mark.parametrize("sxy,srgb", PARAMS)
def test_norm_and_one_filter_application(size, sxy, srgb):
    from wseg_amd import crf
    H, W = size
    N = H * W
    img, _ = _picture(H, W)
    dimg = img.cuda()
    fb, fg = X.features(img.numpy(), sxy, srgb), X.features(img.numpy(), 3.0)
    one = torch.ones(N, 1, dtype=torch.float64)
    Tn, T2n = X.kernel_apply(fb, one, moment=True)
    nb = 1.0 / torch.sqrt(Tn[:, 0] + 1e-20)
    abar = T2n[:, 0] / Tn[:, 0]
    got_n = crf.bilateral_norm(dimg, sxy, srgb).cpu().double().reshape(-1)
    err = ((got_n - nb).abs() / nb)
    print(f"{H}x{W} ({sxy},{srgb}) n: max rel err {float(err.max()):.3e} (bar {SAFETY * float(rel_n(N, abar).max()):.3e}), T2/T max {float(abar.max()):.2f}")
    assert bool((err <= SAFETY * rel_n(N, abar)).all())
    # the Gaussian's n and filter (sxy = 3): the oracle sums all pairs, the kernel a window
    Tg = X.kernel_apply(fg, one)[:, 0]
    ng = 1.0 / torch.sqrt(Tg + 1e-20)
    got_ng = crf.gaussian_norm(dimg, 3.0)
    rel_ng = 0.5 * R_GAUSS + 2 * U32
    assert float(((got_ng.cpu().double().reshape(-1) - ng).abs() / ng).max()) <= SAFETY * rel_ng
    for S in (1, 2):
        for kind in ("soft", "onehot"):
            P = _planes(H, W, S, kind, 10 * S + len(kind))
            Xc = P.reshape(S * 21, N).t().double()
            T, T2 = X.kernel_apply(fb, nb[:, None] * Xc, moment=True)
            ref = nb[:, None] * T
            got = crf.bilateral_filter(dimg, P.cuda(), sxy, srgb).cpu().double().reshape(S * 21, N).t()
            bar = filter_bar(N, nb, T, T2, abar)
            e = (got - ref).abs()
            print(f"  S={S} {kind}: bilateral max err {float(e.max()):.3e}, max err/bar {float((e / bar.clamp_min(1e-300)).max()):.3f}")
            assert bool((e <= bar).all())
            refg = ng[:, None] * X.kernel_apply(fg, ng[:, None] * Xc)
            gotg = crf.gaussian_filter(P.cuda(), 3.0, got_ng).cpu().double().reshape(S * 21, N).t()
            barg = SAFETY * ((R_GAUSS + 2 * U32 + 2 * rel_ng) * refg + GAUSS_FLOOR)
            eg = (gotg - refg).abs()
            print(f"  S={S} {kind}: Gaussian max err {float(eg.max()):.3e}, max err/bar {float((eg / barg.clamp_min(1e-300)).max()):.3f}")
            assert bool((eg <= barg).all())


def test_full_size_rows_against_float64():
    """375 x 500, (80, 13): n and one bilateral application on 512 hash-chosen rows (border rows included), float64 over all 187 500 j"""
    from wseg_amd import crf, synth
    H, W = 375, 500
    N = H * W
    img, _ = _picture(H, W)
    dimg = img.cuda()
    pick = (synth.hash_uniform(4242, 600).double() * N).long().clamp_(max=N - 1).tolist()
    border = [0, W - 1, (H - 1) * W, N - 1, 7 * W, 9 * W - 1, 201, (H - 1) * W + 333]                          # corners, edges
    rows = torch.tensor(list(dict.fromkeys(border + pick))[:512])
    assert len(rows) == 512
    ys, xs = rows // W, rows % W
    assert int(((ys == 0) | (ys == H - 1) | (xs == 0) | (xs == W - 1)).sum()) >= 8
    fb = X.features(img.numpy(), 80, 13)
    got_n = crf.bilateral_norm(dimg, 80, 13).cpu().double().reshape(-1)
    P = _planes(H, W, 2, "soft", 3)
    got = crf.bilateral_filter(dimg, P.cuda(), 80, 13).cpu().double().reshape(42, N).t()
    Xc = P.reshape(42, N).t().double()
    worst_n = worst_f = 0.0
    # the float64 n_j of ALL pixels would cost N^2; the rows' sums use the kernel's n_j, whose error is the 2 rn term of filter_bar.  That n
    # is checked in float64 on the rows and on a second hash-chosen sample of 256 sources j, where T2 / T <= 4 (assumed below) is checked too
    rowset = set(rows.tolist())
    second = torch.tensor([j for j in dict.fromkeys((synth.hash_uniform(777, 400).double() * N).long().clamp_(max=N - 1).tolist())
                           if j not in rowset][:256])
    assert len(second) == 256
    for s in range(0, 256, 64):
        r = second[s:s + 64]
        K, A = X.kernel_rows(fb, r)
        Tn, T2n = K.sum(1), (K * A).sum(1)
        n = 1.0 / torch.sqrt(Tn + 1e-20)
        assert float((T2n / Tn).max()) <= 4.0
        assert bool(((got_n[r] - n).abs() / n <= SAFETY * rel_n(N, T2n / Tn)).all())
    for s in range(0, len(rows), 64):
        r = rows[s:s + 64]
        K, A = X.kernel_rows(fb, r)
        Tn, T2n = K.sum(1), (K * A).sum(1)
        n = 1.0 / torch.sqrt(Tn + 1e-20)
        abar = T2n / Tn
        en = (got_n[r] - n).abs() / n
        assert bool((en <= SAFETY * rel_n(N, abar)).all()), float(en.max())
        xin = got_n[:, None] * Xc
        T, T2 = K @ xin, (K * A) @ xin
        bar = filter_bar(N, n, T, T2, torch.full_like(abar, 4.0))          # T2 / T of n_j elsewhere: <= 4 assumed, 2.0 seen on the rows
        e = (got[r] - n[:, None] * T).abs()
        worst_n, worst_f = max(worst_n, float(en.max())), max(worst_f, float((e / bar).max()))
        assert float(abar.max()) <= 4.0
        assert bool((e <= bar).all()), float((e / bar).max())
    print(f"375x500: n max rel err {worst_n:.3e} (R_ACC {r_acc(N):.3e}); filter max err/bar {worst_f:.3f} on {len(rows)} rows")


def logit_bar(img, sxy, srgb, ref, t=10):
    """the derived bar of the logits after t iterations (module docstring), from the oracle's own quantities; asserted <= 5e-4"""
    N = img.shape[0] * img.shape[1]
    fb = X.features(img.numpy(), sxy, srgb)
    Tn, T2n = X.kernel_apply(fb, torch.ones(N, 1, dtype=torch.float64), moment=True)
    abar = float((T2n / Tn).max())
    rel_b = (r_acc(N) + 4 * U32 + 5 * U32 * abar) + 2 * float(rel_n(N, torch.tensor(abar)))
    rel_g = (R_GAUSS + 2 * U32) + 2 * (0.5 * R_GAUSS + 2 * U32)
    e_it = 10.0 * float(ref["fb"].max()) * rel_b + 3.0 * float(ref["fg"].max()) * rel_g + 4 * U32 * float(ref["logits"].abs().max())
    bar = SAFETY * math.sqrt(t) * e_it
    assert bar <= LOGIT_BAR_CEILING, bar
    return bar, abar


def _run_case(H, W, sxy, srgb):
    from wseg_amd import crf
    img, cams = _picture(H, W)
    lab = X.label_tensor({k: v.numpy() for k, v in cams.items()}, H, W, bg_score=0.26)
    ref = X.crf(img.numpy(), lab, 10, bilateral=(sxy, srgb, 10.0), gaussian=(3, 3.0))
    dlab = crf.labels_from_cams(cams, bg_score=0.26)
    assert np.array_equal(dlab.cpu().numpy(), lab)
    Q, logits, amax = crf.crf_inference(img.cuda(), dlab, t=10, bilateral=(sxy, srgb, 10), gaussian=(3, 3), return_logits=True,
                                        return_argmax=True)
    return img, lab, ref, Q, logits, amax


@pytest.mark.parametrize("size", [(40, 56), (64, 88)])
@pytest.mark.parametrize("sxy,srgb", PARAMS)
def test_ten_iterations_against_float64(size, sxy, srgb):
    H, W = size
    N = H * W
    img, lab, ref, Q, logits, amax = _run_case(H, W, sxy, srgb)
    bar, abar = logit_bar(img, sxy, srgb, ref)
    err = float((logits.cpu().double() - ref["logits"]).abs().max())
    print(f"{H}x{W} ({sxy},{srgb}): max |dlogit| {err:.3e}, bar {bar:.3e} (T2/T {abar:.2f}, Fb max {float(ref['fb'].max()):.3f})")
    assert err <= bar
    assert float((Q.sum(1) - 1).abs().max()) <= 21 * 2 * U32 * SAFETY            # 21 quotients of one f32 sum
    l64 = ref["logits"][0].reshape(21, N)
    top2 = torch.topk(l64, 2, 0)[0]
    sure = (top2[0] - top2[1]) >= 1e-3
    assert float((~sure).float().mean()) <= 1e-3
    a = amax[0].cpu().reshape(-1).long()
    assert bool((a[sure] == l64.argmax(0)[sure]).all())
    assert bool((Q[0].argmax(0).cpu().reshape(-1)[sure] == a[sure]).all())
    changed = float((l64.argmax(0).numpy() != lab.reshape(-1)).mean())
    assert changed >= 0.03, changed                                               # the CRF does move labels: not a trivial case


def test_two_label_sets_share_one_pass():
    from wseg_amd import crf
    H, W = 64, 88
    img, cams = _picture(H, W)
    dimg = img.cuda()
    labs = crf.labels_from_cams(cams, alpha=(4, 32))
    assert tuple(labs.shape) == (2, H, W) and not torch.equal(labs[0], labs[1])
    for s, a in enumerate((4, 32)):
        assert np.array_equal(labs[s].cpu().numpy(), X.label_tensor({k: v.numpy() for k, v in cams.items()}, H, W, alpha=a))
    both, lg = crf.crf_inference(dimg, labs, bilateral=(80, 13, 10), return_logits=True)
    # A label set's columns see the same k values, the same sources in the same order and the same fma chain whichever columns they are
    # and whatever stands beside them, and every other kernel works per (set, pixel): the bar is zero — bit equality.
    for s in range(2):
        one, lg1 = crf.crf_inference(dimg, labs[s], bilateral=(80, 13, 10), return_logits=True)
        assert torch.equal(lg1[0], lg[s]), float((lg1[0] - lg[s]).abs().max())
        assert torch.equal(one[0], both[s])
    assert float((both[0] - both[1]).abs().max()) > 0.1
    five = crf.crf_inference(dimg, torch.stack([labs[0], labs[1], labs[0], labs[1], labs[0]]), bilateral=(80, 13, 10))     # > one pass
    assert tuple(five.shape) == (5, 21, H, W)
    assert torch.equal(five[4], both[0]) and torch.equal(five[3], both[1]) and torch.equal(five[2], both[0])


def test_horizontal_flip_covariance():
    from wseg_amd import crf
    H, W = 40, 56
    img, cams = _picture(H, W)
    lab = crf.labels_from_cams(cams, bg_score=0.26)
    Q, lg = crf.crf_inference(img.cuda(), lab, bilateral=(50, 5, 10), return_logits=True)
    Qf, lgf = crf.crf_inference(torch.flip(img, dims=[1]).cuda(), torch.flip(lab, dims=[1]), bilateral=(50, 5, 10), return_logits=True)
    # the mirrored picture is the same sums in another order of j: the derived ten-iteration bar, as against float64
    ref = X.crf(img.numpy(), lab.cpu().numpy(), 10, bilateral=(50, 5, 10.0), gaussian=(3, 3.0))
    bar, _ = logit_bar(img, 50, 5, ref)
    dl = float((torch.flip(lgf, dims=[3]) - lg).abs().max())
    dq = float((torch.flip(Qf, dims=[3]) - Q).abs().max())
    print(f"flip: max |dlogit| {dl:.3e} (bar {bar:.3e}), max |dQ| {dq:.3e}")
    assert dl <= bar
    assert dq <= 0.5 * bar                   # soft-max: |dQ_c| <= 2 Q_c (1 - Q_c) max|dlogit| <= max|dlogit| / 2


def test_eight_threads_one_device():
    from wseg_amd import crf
    H, W = 40, 56
    img, cams = _picture(H, W)
    dimg = img.cuda()
    labs = [crf.labels_from_cams(cams, alpha=a) for a in (1, 2, 4, 8, 12, 16, 24, 32)]
    want = [crf.crf_inference(dimg, l, bilateral=(80, 13, 10)) for l in labs]
    torch.cuda.synchronize()
    got, errs = [None] * 8, []

    def work(k):
        try:
            with torch.cuda.stream(torch.cuda.Stream()):
                for _ in range(3):
                    got[k] = crf.crf_inference(dimg, labs[k], bilateral=(80, 13, 10))
                torch.cuda.current_stream().synchronize()
        except Exception as e:                                                     # noqa: BLE001
            errs.append(e)

    th = [threading.Thread(target=work, args=(k,)) for k in range(8)]
    [t.start() for t in th]
    [t.join() for t in th]
    assert not errs, errs
    for k in range(8):
        assert torch.equal(got[k], want[k]), k


def test_cli_end_to_end(tmp_path):
    """--out_crf and aff_prepare on a few synthetic JPEGs with procedural weights"""
    import PIL.Image
    from wseg_amd import aff_prepare, contrast_infer, crf, synth
    from wseg_amd.safe_npy import load_pickled_npy
    H, W = 96, 128
    root = tmp_path / "VOC2012"
    (root / "JPEGImages").mkdir(parents=True)
    names = [f"2007_00000{i}" for i in range(3)]
    for i, n in enumerate(names):
        PIL.Image.fromarray(synth.synthetic_rgb_image(H, W, 20 + i).numpy()).save(root / "JPEGImages" / (n + ".jpg"), quality=95)
    lst = tmp_path / "list.txt"
    lst.write_text("\n".join(f"/JPEGImages/{n}.jpg /SegmentationClassAug/{n}.png" for n in names) + "\n")
    bare = tmp_path / "bare.txt"
    bare.write_text("\n".join(names[:2]) + "\n")
    labels = {n: synth.synthetic_labels(3, 0)[i].numpy() for i, n in enumerate(names)}
    np.save(tmp_path / "cls_labels.npy", labels, allow_pickle=True)
    contrast_infer.main(["--weights", "procedural", "--infer_list", str(lst), "--voc12_root", str(root), "--labels",
                         str(tmp_path / "cls_labels.npy"), "--out_cam", str(tmp_path / "cam"), "--out_crf", str(tmp_path / "crf"),
                         "--num_workers", "0", "--precision", "fp32"])
    for n in names:
        png = np.asarray(PIL.Image.open(tmp_path / "crf" / (n + ".png")))
        assert png.shape == (H, W) and png.dtype == np.uint8
        cams = load_pickled_npy(str(tmp_path / "cam" / (n + ".npy")))
        present = {int(k) + 1 for k in cams}
        assert present == {int(c) + 1 for c in np.nonzero(labels[n])[0]}
        assert set(np.unique(png).tolist()) <= {0} | present
        rgb = torch.from_numpy(np.array(PIL.Image.open(root / "JPEGImages" / (n + ".jpg")).convert("RGB"))).cuda()
        lab = crf.labels_from_cams({k: torch.from_numpy(v) for k, v in cams.items()}, bg_score=0.26)
        direct = crf.crf_inference(rgb, lab, t=10, n_labels=21, gt_prob=0.7, bilateral=(50, 5, 10), gaussian=(3, 3))
        assert np.array_equal(direct[0].argmax(0).cpu().numpy().astype(np.uint8), png)
    aff_prepare.main(["--infer_list", str(bare), "--voc12_root", str(root), "--cam_dir", str(tmp_path / "cam"), "--out_crf",
                      str(tmp_path / "aff"), "--num_workers", "0", "--alpha", "4", "32"])
    for n in names[:2]:
        la = np.load(tmp_path / "aff" / "4.00" / (n + ".npy"), allow_pickle=True)
        ha = np.load(tmp_path / "aff" / "32.00" / (n + ".npy"), allow_pickle=True)
        assert la.shape == ha.shape == (21, H, W) and la.dtype == ha.dtype == np.float32
        label = np.transpose(np.array(list(la) + list(ha)), (1, 2, 0))            # VOC12AffDataset.__getitem__ (voc12/data.py:231-235)
        assert label.shape == (H, W, 42)
        la_arg, ha_arg = np.argmax(label[:, :, :21], 2), np.argmax(label[:, :, 21:], 2)   # voc12/data.py: the two arg-max label maps
        assert la_arg.shape == ha_arg.shape == (H, W) and max(la_arg.max(), ha_arg.max()) <= 20
        np.testing.assert_allclose(la.sum(0), 1.0, atol=1e-5)
        cams = load_pickled_npy(str(tmp_path / "cam" / (n + ".npy")))
        l2 = crf.labels_from_cams(cams, alpha=(4, 32)).cpu().numpy()
        assert bool(np.all((l2[1] == 0) <= (l2[0] == 0)))                         # before the CRF: the alpha-32 background inside the alpha-4 one
        assert (float(np.abs(la - ha).max()) > 1e-3) == bool((l2[0] != l2[1]).any())   # the two files differ exactly when the two label maps do
    assert not (tmp_path / "aff" / "4.00" / (names[2] + ".npy")).exists()
