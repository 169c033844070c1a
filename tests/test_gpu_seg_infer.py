"""DeepLab-v1 multi-scale inference on the GPU (wseg_amd/deeplabv1_resnet38.py, wseg_amd/seg_infer.py, csrc/seg.hip) against the fixtures the
reference's own deeplabv1 produced on the CPU in float32 (scripts/make_seg_goldens.py, tests/golden/seg_*.npz).

The bars that decide are the reference's own (tests/seg_env.py; scripts/make_seg_envelopes.py, tests/golden/seg_*_env.npz, seg_*_tap64.npz):
the yardstick is the reference's net in float64, and each mode may deviate from it by what the reference's own evaluation in that
arithmetic deviates, computed in the test from the stored per-pass coarse logits.
    fp32    <= SAFETY . max |v - c64| over the reference in float32 in three vectorised orders and as one sequential K chain per conv
            (the mean logits: the same through seg_f64.fuse, + seg_f64.fuse_bar_local for our float32 collect kernel)
    bf16x3  <= SAFETY . max |x3 - c64| + the fp32 bar, x3 = every conv as hi.hi + hi.lo + lo.hi of the bf16 halves summed in float64
    bf16    <= 1.0 . max |reference in bfloat16 - c64| on the mean logits, and no more labels off float64's than that run has
    fp32, bf16x3: labels equal float64's wherever float64's margin is >= twice the mean bar (all but <= 1 %), margin map within twice it
    the backbone's output (conv_fov's input) of two passes per case on 273 channels, per mode by the stored envelopes of the same variants
Measured on the MI355X (profiles/r20_seg_envelopes.txt), ours / bar: fp32 coarse 0.46-0.67, bf16x3 coarse 0.41-0.52, bf16 mean 0.58-0.73
and labels 0.40-0.62; tap fp32 0.55-0.92, bf16x3 0.32-0.43, bf16 0.48-0.57.

The older bars below are fitted to our own output and kept beside them.  max |ours - fixture| per case was MEASURED on the MI355X against
the float32 fixture, and the bar is twice that (the kernels are deterministic and the inputs fixed: the factor covers a rebuild).  The
label map must equal the fixture's outside the pixels whose stored margin is below twice the mean-logit bar; those may be at most 1 % of
the image, and the bar itself must stay below 1e-3 max |logit| or the mode fails.

MEASURED (MI355X; profiles/r16_seg_infer.txt), max |ours - fixture| of the per-pass coarse logits / of the mean logits (max |mean logit|):
    fp32    40x56 7.44e-5 / 1.24e-5 (4.84)   33x47 5.83e-5 / 9.78e-6 (5.52)   100x125 1.19e-4 / 4.51e-5 (13.96)     bar / 1e-3 max: <= 0.006
    bf16x3  40x56 4.63e-4 / 1.01e-4          33x47 4.15e-4 / 9.82e-5          100x125 9.96e-4 / 3.04e-4             bar / 1e-3 max: <= 0.044
  both modes: every label equal to the reference's, the excluded share (stored margin < 2 x bar) at most 0.08 %.
bf16 is judged by the share of pixels that agree with the reference's label map, measured minus one percentage point:
    bf16    40x56 99.06 %   33x47 98.45 %   100x125 98.82 %    (max |mean - fixture| 0.067 / 0.060 / 0.205: 20-30 x the 1e-3 max |logit| line)
"""
import numpy as np
import pytest
import torch

from tests.test_seg_host import CASES, load_case

pytestmark = pytest.mark.gpu

# {mode: {case: (max |coarse - fixture|, max |mean - fixture|)}} as measured; the asserted bar is twice the figure
MEASURED = {
    "fp32": {"seg_40x56": (7.4387e-05, 1.2398e-05), "seg_33x47": (5.8323e-05, 9.7752e-06), "seg_100x125": (1.1921e-04, 4.5061e-05)},
    "bf16x3": {"seg_40x56": (4.6349e-04, 1.0085e-04), "seg_33x47": (4.1509e-04, 9.8228e-05), "seg_100x125": (9.9564e-04, 3.0375e-04)},
}
BF16_AGREEMENT = {"seg_40x56": 0.99062, "seg_33x47": 0.98453, "seg_100x125": 0.98816}      # measured share of pixels equal to the reference's label map
_nets, _runs = {}, {}


def net(mode):
    """one Net per precision mode with the procedural weights of the fixtures, shared by every test"""
    if mode not in _nets:
        from wseg_amd import synth
        from wseg_amd.deeplabv1_resnet38 import Net
        m = Net(precision=mode)
        m.load_state_dict(synth.procedural_seg_state_dict(0), strict=True)
        _nets[mode] = m.eval().cuda()
    return _nets[mode]


def scaled_of(z):
    from wseg_amd import synth
    from wseg_amd.seg_infer import scaled_inputs
    H, W = int(z["H"]), int(z["W"])
    img = synth.synthetic_images(1, (H, W), int(z["img_seed"]))[0].permute(1, 2, 0).numpy()
    return img, scaled_inputs(img, [float(s) for s in z["scales"]])


def run_case(mode, name):
    """our per-pass coarse logits [n_pass][21, fh, fw], mean logits, label map and margin of a fixture case (computed once per mode)"""
    if (mode, name) not in _runs:
        from wseg_amd import seg_infer
        from wseg_amd import _lib as L
        z = load_case(name)
        H, W = int(z["H"]), int(z["W"])
        _img, scaled = scaled_of(z)
        model = net(mode)
        passes = seg_infer.coarse_passes(model, scaled, flip=True)
        coarse = [p.rows.float().view(-1, p.fh, p.fw, p.ld)[p.img, :, :, :21].permute(2, 0, 1).cpu() for p in passes]
        pad = max(float(p.rows.float()[:, 21:].abs().max()) for p in passes)
        out = dict(amax=torch.empty(H, W, device="cuda", dtype=torch.uint8), mean=torch.empty(21, H, W, device="cuda"),
                   margin=torch.empty(H, W, device="cuda"))
        L.seg_fuse(passes, H, W, 21, out["amax"], out["mean"], None, out["margin"])
        _runs[(mode, name)] = dict(z=z, coarse=coarse, pad=pad, flips=[p.flip for p in passes], **{k: v.cpu() for k, v in out.items()})
    return _runs[(mode, name)]


def figures(mode, name):
    """(max |coarse - fixture|, max |mean - fixture|, max |fixture mean logit|, share of pixels whose label equals the fixture's)"""
    r = run_case(mode, name)
    z = r["z"]
    assert len(r["coarse"]) == int(z["n_pass"]) and r["flips"] == [i % 2 == 1 for i in range(len(r["coarse"]))]
    dc = max(float((c - torch.from_numpy(zc)).abs().max()) for c, zc in zip(r["coarse"], z["coarse"]))
    dm = float((r["mean"] - torch.from_numpy(z["mean"])).abs().max())
    agree = float((r["amax"].numpy() == z["label"]).mean())
    return dc, dm, float(np.abs(z["mean"]).max()), agree


@pytest.mark.parametrize("name", CASES)
@pytest.mark.parametrize("mode", ["fp32", "bf16x3"])
def test_logits_and_labels_against_the_reference(mode, name):
    dc, dm, mx, agree = figures(mode, name)
    r = run_case(mode, name)
    z = r["z"]
    print(f"{mode} {name}: max |coarse - ref| {dc:.3e}, max |mean - ref| {dm:.3e}, max |mean logit| {mx:.2f}, label agreement {agree:.4%}")
    assert r["pad"] == 0.0                                       # the three padding columns of the cls_conv rows are zero
    m_coarse, m_mean = MEASURED[mode][name]
    assert dc <= 2 * m_coarse and dm <= 2 * m_mean
    bar = 2 * m_mean
    assert bar < 1e-3 * mx, "the mode's logit bar is not below 1e-3 max |logit|"
    unsure = z["margin"] < 2 * bar
    assert float(unsure.mean()) <= 0.01
    assert bool((r["amax"].numpy()[~unsure] == z["label"][~unsure]).all())
    assert float((r["margin"] - torch.from_numpy(z["margin"])).abs().max()) <= 2 * bar


@pytest.mark.parametrize("name", CASES)
def test_bf16_label_agreement(name):
    dc, dm, mx, agree = figures("bf16", name)
    print(f"bf16 {name}: max |coarse - ref| {dc:.3e}, max |mean - ref| {dm:.3e}, max |mean logit| {mx:.2f}, label agreement {agree:.4%}")
    assert agree >= BF16_AGREEMENT[name] - 0.01


@pytest.mark.parametrize("name", CASES)
@pytest.mark.parametrize("mode", ["fp32", "bf16x3"])
def test_logits_and_labels_within_the_reference_envelopes_of_float64(mode, name):
    """the derived bars (tests/seg_env.py): the same run as above against the reference's float64 run, held to the reference's own float32
    (and split-bf16) deviation from it.  Also max |ours - x3| for bf16x3: the quantity to watch, without an assertion (a residual that flips
    at a rounding boundary has no derived bound)."""
    from tests import seg_env
    e, r = seg_env.load_env(name), run_case(mode, name)
    print(f"{mode} {name}:")
    failed = seg_env.judge(e, mode, r["coarse"], r["mean"], r["amax"], r["margin"])
    if mode == "bf16x3":
        d = seg_env.coarse_dev(r["coarse"], e["coarse"]["x3"])
        print(f"  max |ours - x3| {max(d):.3e} (per pass {' '.join(f'{v:.1e}' for v in d)});  max |x3 - c64| {e['d_coarse']['x3']:.3e}")
    assert failed == []


@pytest.mark.parametrize("name", CASES)
def test_bf16_within_the_reference_bf16_envelope_of_float64(name):
    """our bf16 mode is no further from float64 than the reference's own bfloat16 run, on the mean logits and on the labels, with no margin
    factor (float32 accumulators and epilogues against a run that rounds every op).  The coarse ratio is printed, not asserted."""
    from tests import seg_env
    e, r = seg_env.load_env(name), run_case("bf16", name)
    ref = e["fused"]["c64"]
    d = seg_env.coarse_dev(r["coarse"], e["coarse"]["c64"])
    for i, (di, ei) in enumerate(zip(d, e["d_pass"]["bf16"])):
        print(f"  pass {i:2d}: max |ours - c64| {di:.3e}  reference bf16 {ei:.3e}  ratio {di / ei:.3f}")
    dm = float((r["mean"].double() - ref["mean"]).abs().max())
    dis, env_dis = seg_env.label_disagreement(e, r["amax"]), seg_env.label_disagreement(e, e["fused"]["bf16"]["amax"])
    print(f"bf16 {name}: coarse {max(d):.3e} / {e['d_coarse']['bf16']:.3e} = {max(d) / e['d_coarse']['bf16']:.3f}   mean {dm:.3e} / "
          f"{e['d_mean']['bf16']:.3e} = {dm / e['d_mean']['bf16']:.3f}   label disagreement {dis:.3%} / {env_dis:.3%}")
    assert dm <= 1.0 * e["d_mean"]["bf16"]
    assert dis <= env_dis


@pytest.mark.parametrize("name", CASES)
@pytest.mark.parametrize("mode", ["fp32", "bf16x3", "bf16"])
def test_backbone_tap_within_the_reference_envelopes_of_float64(mode, name):
    """relu(bn7(conv6)), the head's input, of the plain pass of the smallest and of the largest scale on the stored channel subset against
    the reference's float64 tap: separates a backbone deviation from a head deviation when an end-to-end assertion fails"""
    from tests import seg_env
    e = seg_env.load_env(name)
    t = e["tap"]
    _img, scaled = scaled_of(e["z"])
    model = net(mode)
    failed = []
    for i in (int(v) for v in t["tap_passes"]):
        x = torch.from_numpy(scaled[i // 2]).cuda()[None]
        with torch.no_grad():
            st, _ps = model._engine.active(x.device).run_backbone([x])
        tap = torch.from_numpy(t[f"tap_{i}"])
        (fh, fw), = st["dims"]
        assert (fh, fw) == tuple(tap.shape[:2]) and tuple(st["t"].shape) == (fh * fw, 4096)
        ours = st["t"].view(fh, fw, 4096)[:, :, int(t["c0"])::int(t["stride"])].double().cpu()
        d, bar = float((ours - tap).abs().max()), seg_env.tap_bar(e, mode, i)
        print(f"{mode} {name} tap pass {i} {fh}x{fw}: max |ours - tap64| {d:.3e}  bar {bar:.3e}  ratio {d / bar:.3f}  (max |tap64| {float(t[f'tapmax_{i}']):.2f})")
        if not d <= bar:
            failed.append(i)
    assert failed == []


@pytest.mark.parametrize("mode", ["fp32", "bf16", "bf16x3"])
def test_plain_and_flipped_as_one_batch_equal_two_single_passes(mode):
    """the N = 2 pass of one scale gives, row for row and bit for bit, what the two N = 1 passes give; forward() is the single pass resampled"""
    z = load_case("seg_33x47")
    _img, scaled = scaled_of(z)
    model = net(mode)
    for x in (scaled[0], scaled[3]):
        x = torch.from_numpy(x).cuda()
        both, dims = model.coarse_logits(torch.stack([x, x.flip(2)]))
        one, dims1 = model.coarse_logits(x[None])
        other, _ = model.coarse_logits(x.flip(2)[None])
        assert dims == dims1 and tuple(both.shape) == (2 * dims[0] * dims[1], 24)
        assert torch.equal(both[:one.shape[0]], one) and torch.equal(both[one.shape[0]:], other)
        assert not torch.equal(one, other)
    full = model(x[None])
    assert tuple(full.shape) == (1, 21, x.shape[1], x.shape[2]) and full.dtype == torch.float32
    from tests import seg_f64
    ref = seg_f64.resize(one.float().view(dims[0], dims[1], 24)[:, :, :21].permute(2, 0, 1).cpu(), x.shape[1], x.shape[2])
    M = float(one.float().abs().max())
    from tests.f64_bars import _interp_bar
    assert float((full[0].cpu().double() - ref).abs().max()) <= _interp_bar(dims[0], dims[1], M)


def test_cli_writes_the_in_memory_maps_and_their_miou(tmp_path, capsys):
    """python -m wseg_amd.seg_infer on three synthetic JPEGs with --weights procedural --out_png --gt_dir: the PNGs are the in-memory path's
    label maps, and the printed mIoU is wseg_amd.eval's host path on those PNGs"""
    import PIL.Image
    from wseg_amd import eval as weval
    from wseg_amd import seg_infer, synth
    root = tmp_path / "VOC2012"
    (root / "JPEGImages").mkdir(parents=True)
    (tmp_path / "gt").mkdir()
    names, sizes = [f"2007_00000{i}" for i in range(3)], [(40, 56), (33, 47), (48, 40)]
    for i, (n, (H, W)) in enumerate(zip(names, sizes)):
        PIL.Image.fromarray(synth.synthetic_rgb_image(H, W, 30 + i).numpy()).save(root / "JPEGImages" / (n + ".jpg"), quality=95)
        PIL.Image.fromarray(synth.synthetic_aff_label_map(H, W, 40 + i, classes=(0, 1, 3, 13)).numpy()).save(tmp_path / "gt" / (n + ".png"))
    lst = tmp_path / "list.txt"
    lst.write_text("\n".join(f"/JPEGImages/{n}.jpg /SegmentationClassAug/{n}.png" for n in names) + "\n")
    scales = ["0.5", "1.0", "1.5"]
    res = seg_infer.main(["--weights", "procedural", "--infer_list", str(lst), "--voc12_root", str(root), "--out_png", str(tmp_path / "png"),
                          "--gt_dir", str(tmp_path / "gt"), "--num_workers", "0", "--precision", "fp32", "--scales"] + scales)
    printed = capsys.readouterr().out
    model = net("fp32")
    for n, (H, W) in zip(names, sizes):
        png = np.asarray(PIL.Image.open(tmp_path / "png" / (n + ".png")))
        assert png.shape == (H, W) and png.dtype == np.uint8
        img = model.normalize(np.asarray(PIL.Image.open(root / "JPEGImages" / (n + ".jpg")).convert("RGB")))
        direct = seg_infer.infer_image(model, img, [float(s) for s in scales])
        assert np.array_equal(direct.cpu().numpy(), png)
    host = weval.do_eval(names, str(tmp_path / "png"), str(tmp_path / "gt"))
    assert abs(res["mIoU"] - host["mIoU"]) <= 1e-9 and ("mIoU: %.3f" % host["mIoU"]) in printed
