"""AffinityNet inference on the GPU: affinities, dense matrix and random walk against the reference's own outputs (fixtures made by
scripts/make_aff_goldens.py), the kernels against torch ops on the device, edge cases, the aff_infer CLI end to end, and the drop-in
module contract."""
import os
import threading

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.test_aff_host import AFF_CASES, load_case

pytestmark = pytest.mark.gpu

# fp32 (parity mode): the reference's own winner / runner-up margin at a pixel whose arg-max differs must be inside f32 noise
REF_NEAR_TIE_MARGIN = 1e-4
# bf16x3 / bf16 against the reference's fp32 masks: bar = 2 x measured (mismatching-pixel fraction; mIoU: 100 - 2 x (100 - measured)),
# worst case over the four fixtures.  beta = 8 amplifies the feature error (aff^8), yet the masks hold.  Measured on an MI355X
# (profiles/r04_aff_infer.txt):
#   bf16x3: 0 mismatching pixels on every fixture, mIoU 100.0            -> bars 1e-4 / 99.9 (floors: 2 x 0 would demand bit-equality)
#   bf16:   1.0133e-4 (19 px of 187 500, 375x500), mIoU 99.820 (100x125) -> bars 2.1e-4 / 99.64
BF16X3_MISMATCH_BAR, BF16X3_MIOU_BAR = 1e-4, 99.9
BF16_MISMATCH_BAR, BF16_MIOU_BAR = 2.1e-4, 99.64


def _net(prec):
    from wseg_amd import synth
    from wseg_amd.resnet38_aff import Net
    m = Net(precision=prec)
    m.load_state_dict(synth.procedural_aff_state_dict(0), strict=True)
    m.eval()
    m.cuda()
    return m


@pytest.fixture(scope="module")
def nets():
    return {}


def _get(nets, prec):
    if prec not in nets:
        nets[prec] = _net(prec)
    return nets[prec]


def _padded(g):
    from wseg_amd import synth
    H, W = int(g["H"]), int(g["W"])
    img = synth.synthetic_images(1, (H, W), int(g["img_seed"]))
    Hp, Wp = -(-H // 8) * 8, -(-W // 8) * 8
    return img, F.pad(img, (0, Wp - W, 0, Hp - H)).cuda()


def _cams(g):
    from wseg_amd import synth
    return {k: v.numpy() for k, v in synth.synthetic_cam_dict(int(g["H"]), int(g["W"]), g["classes"].tolist(), int(g["cam_seed"])).items()}


def _near_tie_ok(g, flat_idx):
    """every differing pixel is one where the reference's own margin is inside f32 noise"""
    if "margin" in g:
        m = g["margin"].reshape(-1)[flat_idx]
    else:
        lut = dict(zip(g["near_idx"].tolist(), g["near_margin"].tolist()))
        m = np.array([lut.get(int(i), np.inf) for i in flat_idx])
    return bool(np.all(m <= REF_NEAR_TIE_MARGIN)), m


def _miou(pred, ref, ncls=21):
    ious = []
    for c in np.union1d(np.unique(pred), np.unique(ref)):
        tp = np.sum((pred == c) & (ref == c))
        ious.append(tp / (np.sum(pred == c) + np.sum(ref == c) - tp))
    return 100.0 * float(np.mean(ious))


@pytest.mark.parametrize("name", AFF_CASES)
def test_fp32_affinities_match_reference(golden_dir, nets, name):
    g = load_case(golden_dir, name)
    _, x = _padded(g)
    m = _get(nets, "fp32")
    aff = m(x)
    assert aff.shape == (1,) + g["aff"].shape and aff.dtype == torch.float32
    got = aff[0].cpu().numpy()
    print(name, "max rel err", float(np.max(np.abs(got - g["aff"]) / g["aff"])))
    np.testing.assert_allclose(got, g["aff"], rtol=1e-5, atol=0)
    if "aff_mat" in g:
        dense = m(x, True)
        assert dense.is_cuda and dense.shape == g["aff_mat"].shape
        np.testing.assert_allclose(dense.cpu().numpy(), g["aff_mat"], rtol=1e-5, atol=0)
        assert torch.equal((dense != 0).cpu(), torch.from_numpy(g["aff_mat"] != 0))          # the scatter: exactly the reference's pattern


@pytest.mark.parametrize("name", AFF_CASES)
def test_fp32_random_walk_matches_reference(golden_dir, nets, name):
    from wseg_amd.aff_infer import random_walk_image
    g = load_case(golden_dir, name)
    H, W = int(g["H"]), int(g["W"])
    img, _ = _padded(g)
    pred, cam_rw = random_walk_image(_get(nets, "fp32"), img, _cams(g), (H, W), int(g["beta"]), int(g["logt"]), return_cam_rw=True)
    ref = g["cam_rw"]
    scale = np.abs(ref).reshape(21, -1).max(axis=1).reshape(21, 1, 1) + 1e-12
    err = float((np.abs(cam_rw.cpu().numpy() - ref) / scale).max())
    pred = pred.cpu().numpy()
    diff = np.flatnonzero(pred.reshape(-1) != g["pred"].reshape(-1))
    ok, margins = _near_tie_ok(g, diff)
    print(name, "cam_rw rel err", err, "arg-max mismatches", diff.size, "their reference margins", margins.tolist()[:8])
    assert err < 1e-4, err
    assert pred.shape == (H, W) and pred.dtype == np.uint8
    assert diff.size <= max(2, int(1e-4 * H * W)) and ok, (diff.size, margins)


@pytest.mark.parametrize("prec", ["bf16x3", "bf16"])
def test_reduced_precision_masks(golden_dir, nets, prec):
    from wseg_amd.aff_infer import random_walk_image
    worst_mis, worst_miou = 0.0, 100.0
    for name in AFF_CASES:
        g = load_case(golden_dir, name)
        H, W = int(g["H"]), int(g["W"])
        img, _ = _padded(g)
        pred = random_walk_image(_get(nets, prec), img, _cams(g), (H, W)).cpu().numpy()
        mis = float(np.mean(pred != g["pred"]))
        miou = _miou(pred, g["pred"])
        print(prec, name, "mismatch fraction", mis, "mIoU", miou)
        worst_mis, worst_miou = max(worst_mis, mis), min(worst_miou, miou)
    bars = {"bf16x3": (BF16X3_MISMATCH_BAR, BF16X3_MIOU_BAR), "bf16": (BF16_MISMATCH_BAR, BF16_MIOU_BAR)}[prec]
    assert worst_mis <= bars[0] and worst_miou >= bars[1], (worst_mis, worst_miou)


def _dense_walk(aff, h, w, r, pooled, beta, logt):
    """The reference's formulation on the device: dense A (from the pairs), A^beta, column normalisation, logt squarings, v . T."""
    from wseg_amd import _lib as L
    A = torch.empty(h * w, h * w, device="cuda")
    L.aff_to_dense(aff, A, h, w, r)
    A = torch.pow(A, beta)
    T = A / torch.sum(A, dim=0, keepdim=True)
    for _ in range(logt):
        T = torch.matmul(T, T)
    return torch.matmul(pooled.view(pooled.shape[0], -1), T).view(pooled.shape)


@pytest.mark.parametrize("hw", [(8, 11), (47, 63)])
def test_stencil_walk_kernel_against_dense_power(hw):
    from wseg_amd import _lib as L
    from wseg_amd.resnet38_aff import pair_radius
    h, w = hw
    r = pair_radius(h, w)
    P = L.aff_num_offsets(r)
    n_from = (h - r + 1) * (w - 2 * r + 2)
    gen = torch.Generator().manual_seed(3)
    aff = (0.55 + 0.4 * torch.rand(1, P, n_from, generator=gen)).cuda()
    pooled = torch.rand(21, h, w, generator=gen).cuda()
    wgt = torch.empty(1, 2 * P, h * w, device="cuda")
    rsum = torch.empty(1, h * w, device="cuda")
    L.rw_prepare(aff, wgt, rsum, 1, h, w, r, 8)
    out = torch.empty_like(pooled)
    L.random_walk(wgt, rsum, pooled, out, 1, 21, h, w, r, 6)
    ref = _dense_walk(aff, h, w, r, pooled, 8, 6)
    scale = ref.abs().amax(dim=(1, 2), keepdim=True)
    assert float(((out - ref).abs() / scale).max()) < 1e-4
    # logt = 0: one step, in place (v_in aliases v_out)
    one = pooled.clone()
    L.random_walk(wgt, rsum, one, one, 1, 21, h, w, r, 0)
    ref1 = _dense_walk(aff, h, w, r, pooled, 8, 0)
    torch.testing.assert_close(one, ref1, rtol=1e-5, atol=1e-6)


def test_pool_upsample_argmax_kernels_against_torch():
    from wseg_amd import _lib as L
    gen = torch.Generator().manual_seed(5)
    H, W = 93, 130
    dh, dw = -(-H // 8), -(-W // 8)
    cams = torch.rand(3, H, W, generator=gen).cuda()
    src = [-1] * 21
    src[4], src[9], src[20] = 0, 2, 1
    pooled = torch.empty(21, dh, dw, device="cuda")
    L.rw_pool(cams, src, 0.27, pooled, H, W, dh, dw)
    full = torch.zeros(21, dh * 8, dw * 8, device="cuda")
    full[0, :H, :W] = 0.27
    full[4, :H, :W], full[9, :H, :W], full[20, :H, :W] = cams[0], cams[2], cams[1]
    torch.testing.assert_close(pooled, F.avg_pool2d(full, 8, 8), rtol=1e-6, atol=1e-7)
    cam = torch.rand(21, dh, dw, generator=gen).cuda()
    pred = torch.empty(H, W, device="cuda", dtype=torch.uint8)
    L.rw_finish(cam, pred, 21, dh, dw, H, W)
    up = F.interpolate(cam[None], (dh * 8, dw * 8), mode="bilinear", align_corners=False)[0, :, :H, :W]
    top2 = torch.topk(up, 2, dim=0).values
    ref = torch.max(up, 0)[1].to(torch.uint8)
    diff = pred != ref
    assert int(diff.sum()) <= 3 and bool(((top2[0] - top2[1])[diff] < 1e-6).all())
    ties = torch.zeros(21, dh, dw, device="cuda")                          # all planes equal: the first maximum wins, as torch.max
    L.rw_finish(ties, pred, 21, dh, dw, H, W)
    assert int(pred.max()) == 0


def test_edge_cases_empty_and_single_class(nets):
    from wseg_amd import synth
    from wseg_amd.aff_infer import random_walk_image
    from wseg_amd import _lib as L
    m = _get(nets, "fp32")
    H, W = 61, 83                                            # sides not multiples of 8
    img = synth.synthetic_images(1, (H, W), 90)
    assert int(random_walk_image(m, img, {}, (H, W)).max()) == 0                  # no class: background everywhere
    cams = {k: v.numpy() for k, v in synth.synthetic_cam_dict(H, W, [12], 91).items()}
    pred, cam_rw = random_walk_image(m, img, cams, (H, W), return_cam_rw=True)
    assert set(np.unique(pred.cpu().numpy()).tolist()) <= {0, 13}
    # against the dense formulation on the same features
    Hp, Wp = -(-H // 8) * 8, -(-W // 8) * 8
    x = F.pad(img, (0, Wp - W, 0, Hp - H)).cuda()
    aff, (h, w, r) = m.affinities(x)
    pooled = torch.empty(21, h, w, device="cuda")
    src = [-1] * 21
    src[13] = 0
    L.rw_pool(torch.from_numpy(cams[12])[None].cuda(), src, 0.27, pooled, H, W, h, w)
    ref = _dense_walk(aff, h, w, r, pooled, 8, 6)
    assert float(((cam_rw - ref).abs() / ref.abs().amax(dim=(1, 2), keepdim=True).clamp_min(1e-12)).max()) < 1e-4
    with pytest.raises(ValueError, match="min edge >= 5"):               # feature edge 4: the reference has no pair set there
        m(torch.zeros(1, 3, 32, 64, device="cuda"))
    assert m(torch.zeros(1, 3, 33, 40, device="cuda")).shape == (1, 4, 4 * 3)      # edge 5 (33 px): radius 2, 4 offsets, 4 x 3 from pixels


def test_aff_infer_cli_end_to_end(tmp_path):
    import PIL.Image
    from wseg_amd import aff_infer, contrast_infer, data as wdata, eval as weval, synth
    root = tmp_path / "VOC2012"; (root / "JPEGImages").mkdir(parents=True)
    sizes = [(96, 128), (75, 101), (40, 57)]
    names = [f"2007_00001{i}" for i in range(len(sizes))]
    rng = np.random.default_rng(1)
    for n, hw in zip(names, sizes):
        PIL.Image.fromarray(rng.integers(0, 256, hw + (3,), dtype=np.uint8)).save(root / "JPEGImages" / (n + ".jpg"))
    lst = tmp_path / "list.txt"
    lst.write_text("\n".join(f"/JPEGImages/{n}.jpg /SegmentationClassAug/{n}.png" for n in names) + "\n")
    np.save(tmp_path / "cls_labels.npy", {n: synth.synthetic_labels(len(names), 3)[i].numpy() for i, n in enumerate(names)}, allow_pickle=True)
    contrast_infer.main(["--weights", "procedural", "--infer_list", str(lst), "--voc12_root", str(root), "--labels",
                         str(tmp_path / "cls_labels.npy"), "--out_cam", str(tmp_path / "cam"), "--num_workers", "0", "--precision", "fp32"])
    aff_infer.main(["--weights", "procedural", "--infer_list", str(lst), "--voc12_root", str(root), "--cam_dir", str(tmp_path / "cam"),
                    "--out_rw", str(tmp_path / "rw"), "--num_workers", "0", "--precision", "fp32"])
    m = _net("fp32")
    ds = wdata.VOC12ImageDataset(str(lst), str(root), transform=[np.asarray, m.normalize, wdata.HWC_to_CHW])
    for i, (n, hw) in enumerate(zip(names, sizes)):
        png = np.asarray(PIL.Image.open(tmp_path / "rw" / (n + ".png")))
        assert png.shape == hw and png.dtype == np.uint8 and png.max() <= 20
        _, img = ds[i]
        from wseg_amd.safe_npy import load_pickled_npy
        direct = aff_infer.random_walk_image(m, torch.from_numpy(np.ascontiguousarray(img))[None], load_pickled_npy(str(tmp_path / "cam" / (n + ".npy"))), hw)
        assert np.array_equal(png, direct.cpu().numpy()), n
    res = weval.main(["--list", str(lst), "--predict_dir", str(tmp_path / "rw"), "--gt_dir", str(tmp_path / "rw"), "--type", "png"])
    seen = set(np.unique(np.concatenate([np.asarray(PIL.Image.open(tmp_path / "rw" / (n + ".png"))).ravel() for n in names])).tolist())
    assert all(abs(res[weval.CATEGORIES[c]] - 100.0) < 1e-7 for c in seen)


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_dropin_replicate_and_threads(prec):
    from wseg_amd import synth
    m = _net(prec)
    xs = [synth.synthetic_images(1, s, 70 + i).cuda() for i, s in enumerate([(40, 56), (64, 48), (72, 104), (48, 48)])]
    with torch.no_grad():
        serial = [m(x) for x in xs]
        rep = torch.nn.parallel.replicate(m, [0])[0]
        assert torch.equal(rep(xs[0]), serial[0])
        out = [None] * len(xs)
        fresh = _net(prec)
        ths = [threading.Thread(target=lambda i=i: out.__setitem__(i, fresh(xs[i]))) for i in range(len(xs))]
        for t in ths:
            t.start()
        for t in ths:
            t.join()
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(out, serial))
