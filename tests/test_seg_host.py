"""Host-side checks of the DeepLab-v1 inference stage (wseg_amd/deeplabv1_resnet38.py, wseg_amd/seg_infer.py) against the fixtures
scripts/make_seg_goldens.py made by running the reference's deeplabv1 (tests/golden/seg_*.npz), and of the envelopes
scripts/make_seg_envelopes.py made by running it in float64, float32, split-bf16 and bfloat16 (seg_*_env.npz, seg_*_tap64.npz).  No GPU."""
import os

import numpy as np
import pytest
import torch

from tests import seg_f64
from tests.conftest import GOLDEN

CASES = ["seg_40x56", "seg_33x47", "seg_100x125"]


def load_case(name):
    """the fixture as a dict; `mean` joined from its two files where it was split (the committed-file limit), `coarse` as a list"""
    z = dict(np.load(os.path.join(GOLDEN, name + ".npz")))
    if "mean" not in z:
        z["mean"] = np.concatenate([np.load(os.path.join(GOLDEN, f"{name}_mean_{p}.npz"))["mean"] for p in "ab"])
    z["coarse"] = [z.pop(f"coarse_{i}") for i in range(int(z["n_pass"]))]
    return z


def ref_passes(z):
    """[(coarse [21, fh, fw], (ih, iw), flip)] in the reference's order: scale ascending, plain before flipped"""
    return [(torch.from_numpy(c), tuple(int(v) for v in z["sizes"][i // 2]), i % 2 == 1) for i, c in enumerate(z["coarse"])]


@pytest.fixture(scope="module")
def keys():
    return np.load(os.path.join(GOLDEN, "seg_state_dict_keys.npz"))


def test_state_dict_keys_and_strict_round_trip(keys):
    from wseg_amd import arch, synth
    from wseg_amd.deeplabv1_resnet38 import Net
    net = Net(precision="fp32")
    sd = net.state_dict()
    want = [str(k) for k in keys["keys"]]
    assert len(want) == 242 and list(sd.keys()) == want == list(arch.seg_state_dict_spec().keys())
    assert [",".join(str(d) for d in sd[k].shape) for k in want] == [str(s) for s in keys["shapes"]]
    head = [k for k in want if not k.startswith("backbone.")]
    assert len(head) == 14 and "cls_conv.bias" in head and "bn_fov.num_batches_tracked" in head and "bn_fov2.num_batches_tracked" in head
    proc = synth.procedural_seg_state_dict(0)
    assert list(proc.keys()) == want
    net.load_state_dict(proc, strict=True)
    other = Net(precision="fp32")
    other.load_state_dict(net.state_dict(), strict=True)
    for k, v in other.state_dict().items():
        assert torch.equal(v, proc[k]), k
    # non-trivial BatchNorm statistics and a bias: an implementation that ignored them would not reproduce the fixtures
    for bn in ("bn_fov", "bn_fov2"):
        assert float(proc[bn + ".running_mean"].abs().min()) > 0 and float((proc[bn + ".running_var"] - 1).abs().mean()) > 0.1
        assert float((proc[bn + ".weight"] - 1).abs().mean()) > 0.1 and float(proc[bn + ".bias"].abs().mean()) > 0.01
    assert float(proc["cls_conv.bias"].abs().mean()) > 0.1
    backbone = synth.procedural_state_dict(0)
    assert torch.equal(proc["backbone.b5.conv_branch2a.weight"], backbone["b5.conv_branch2a.weight"])


def test_parameter_groups_match_the_reference(keys):
    from wseg_amd.deeplabv1_resnet38 import Net
    net = Net(precision="fp32").eval()
    names = {id(p): n for n, p in net.named_parameters()}
    groups = [[names[id(p)] for p in g] for g in net.get_parameter_groups()]
    for i in range(4):
        assert groups[i] == [str(n) for n in keys[f"group{i}"]], i
    assert groups[2] == ["conv_fov.weight", "conv_fov2.weight", "cls_conv.weight"] and groups[3] == ["cls_conv.bias"] and not groups[1]
    assert "backbone.conv1a.weight" not in groups[0] and len(groups[0]) == 42
    assert hasattr(net, "normalize") and net.normalize(np.zeros((2, 2, 3), np.uint8)).dtype == np.float32


def test_forward_refuses_training_mode():
    from wseg_amd.deeplabv1_resnet38 import Net
    net = Net(precision="fp32")
    net.train()
    with pytest.raises(RuntimeError, match="inference-only"):
        net(torch.zeros(1, 3, 40, 56))
    assert all(not m.training for m in net.backbone.modules() if isinstance(m, torch.nn.BatchNorm2d))     # the backbone's BatchNorms stay in eval
    net.eval()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        net(torch.zeros(1, 3, 40, 56))


def test_scaled_sizes_round_half_to_even():
    from wseg_amd.seg_infer import TEST_MULTISCALE, scaled_inputs, scaled_size
    assert scaled_size(375, 500, 0.5) == (188, 250) and scaled_size(375, 500, 1.5) == (562, 750)
    assert scaled_size(375, 500, 0.75) == (281, 375) and scaled_size(375, 500, 1.75) == (656, 875)
    assert TEST_MULTISCALE == (0.5, 0.75, 1.0, 1.25, 1.5, 1.75)
    img = np.random.default_rng(0).standard_normal((33, 47, 3)).astype(np.float32)
    out = scaled_inputs(img)
    assert [o.shape for o in out] == [(3,) + scaled_size(33, 47, r) for r in TEST_MULTISCALE] and all(o.dtype == np.float32 for o in out)
    assert np.array_equal(out[2], img.transpose(2, 0, 1))                       # scale 1.0: PIL returns the image itself


@pytest.mark.parametrize("name", CASES)
def test_fixture_inputs_are_reproducible_and_conditions_hold(name):
    """the scaled-size list the fixture was made from is what our host code makes from its seed; at least 4 classes hold >= 2 % of the
    pixels; at most 1 % of the pixels have a margin below 1e-3 max|mean logit| (the conditions the GPU tests rely on)"""
    from wseg_amd import synth
    from wseg_amd.seg_infer import scaled_inputs
    z = load_case(name)
    H, W = int(z["H"]), int(z["W"])
    img = synth.synthetic_images(1, (H, W), int(z["img_seed"]))[0].permute(1, 2, 0).numpy()
    scaled = scaled_inputs(img, [float(s) for s in z["scales"]])
    assert [list(s.shape[1:]) for s in scaled] == z["sizes"].tolist() and int(z["n_pass"]) == 2 * len(scaled)
    assert z["label"].shape == z["margin"].shape == (H, W) and z["mean"].shape == (21, H, W)
    share = np.bincount(z["label"].reshape(-1), minlength=21) / (H * W)
    assert int((share >= 0.02).sum()) >= 4, share
    assert float((z["margin"] < 1e-3 * np.abs(z["mean"]).max()).mean()) <= 0.01
    for f in os.listdir(GOLDEN):
        if f.startswith(name):
            assert os.path.getsize(os.path.join(GOLDEN, f)) < 1 << 20, f


@pytest.mark.parametrize("name", CASES)
def test_float64_collect_reproduces_the_reference(name):
    """tests/seg_f64.py on the fixture's per-pass coarse logits gives the fixture's mean logits within the float32 bar, and its label map
    outside the margins below that bar"""
    z = load_case(name)
    H, W = int(z["H"]), int(z["W"])
    passes = ref_passes(z)
    out = seg_f64.fuse(passes, H, W)
    M = max(float(np.abs(c).max()) for c in z["coarse"])
    bar = seg_f64.fuse_bar(passes, M)
    err = float((out["mean"] - torch.from_numpy(z["mean"]).double()).abs().max())
    print(f"{name}: max |mean_64 - reference| {err:.3e} (bar {bar:.3e}, max |logit| {M:.2f})")
    assert err <= bar
    assert float((out["margin"] - torch.from_numpy(z["margin"]).double()).abs().max()) <= 2 * bar
    sure = out["margin"] >= 2 * bar                   # (two logits, each off by the bar)
    print(f"{name}: {float((~sure).double().mean()):.2%} of the pixels are inside the bar")
    assert float(sure.double().mean()) >= 0.95
    assert bool((out["amax"][sure] == torch.from_numpy(z["label"]).long()[sure]).all())


def test_conv_plan_accepts_the_head_launches():
    """the three head launches in all three modes, on the smallest and on a VOC-sized map, N = 2; conv_fov is the 3x3 at dilation 12"""
    from wseg_amd import _lib as L
    from wseg_amd import arch
    from wseg_amd.engine import head_conv
    for dims in ([(3, 4)], [(47, 63)], [(83, 110)]):
        for dt in (L.BF16, L.F32, L.F32X3):
            for c, extra in ((head_conv("conv_fov", 4096, 512, dims, k=3, dil=arch.SEG_HEAD_DILATION), {}),
                             (head_conv("conv_fov2", 512, 512, dims), {}),
                             (head_conv("cls_conv", 512, arch.SEG_CLS_ROWS, dims), dict(relu_out2=0))):
                kw = c.fwd_kw(2)
                assert kw["pad"] == kw["dil"] * (kw["KH"] // 2)
                plan = L.conv_plan(L._ANY, L._ANY, None, L._ANY, dtype=dt, shift=L._ANY, **kw, **extra)
                assert plan.family in (L.CONV_64x128, L.CONV_128x128, L.CONV_224x256, L.CONV_256x256) and plan.nwg >= 1, (c.name, dt, plan)
    assert head_conv("conv_fov", 4096, 512, [(5, 7)], k=3, dil=12).fwd_kw(1)["pad"] == 12


# ---- the reference's float64 / float32 / split-bf16 / bfloat16 runs: the envelopes the GPU bars are made of (tests/seg_env.py) ----

def load_env(name):
    """the reference's variants of a case with the envelopes computed from them (tests/seg_env.py:load_env)"""
    from tests import seg_env
    return seg_env.load_env(name)


def test_envelope_table(capsys):
    """prints what profiles/r20_seg_envelopes.txt records: per case the deviation of every variant from float64, coarse / mean / labels"""
    from tests import seg_env
    with capsys.disabled():
        print()
        for name in CASES:
            e = load_env(name)
            print(f"{name}: max |c64 logit| {e['M']:.2f}, max |mean64| {float(e['fused']['c64']['mean'].abs().max()):.2f}, fuse_bar {e['fuse_bar']:.3e} (for any logits that large {e['fuse_bar_worst']:.3e})")
            for v in seg_env.VARIANTS[1:]:
                print(f"  {v:9s} - c64: coarse {e['d_coarse'][v]:.3e}  mean {e['d_mean'][v]:.3e}  label disagreement "
                      f"{seg_env.label_disagreement(e, e['fused'][v]['amax']):.2%}")
            print(f"  ENV32 coarse {e['env32_coarse']:.3e} mean {e['env32_mean']:.3e};  bars fp32 {seg_env.bars(e, 'fp32')[0]:.3e} / {seg_env.bars(e, 'fp32')[1]:.3e}"
                  f"  bf16x3 {seg_env.bars(e, 'bf16x3')[0]:.3e} / {seg_env.bars(e, 'bf16x3')[1]:.3e}")
            t = e["tap"]
            for i in t["tap_passes"]:
                print(f"  tap pass {int(i)} {t[f'tap_{i}'].shape}: max |tap64| {float(t[f'tapmax_{i}']):.2f}  " +
                      "  ".join(f"{v} {float(t[f'dev_{v}_{i}']):.3e}" for v in t["tap_variants"]))


@pytest.mark.parametrize("name", CASES)
def test_envelopes_tie_to_the_fixture_and_the_chain_is_the_longest_order(name):
    from tests import seg_env
    from tests.f64_bars import SAFETY
    e = load_env(name)
    z = e["z"]
    # the sequential K chain deviates at least as much as every vectorised order: otherwise the emulation is not doing what it says
    for v in seg_env.F32_ORDERS:
        assert e["d_coarse"]["f32_chain"] >= e["d_coarse"][v] > 0, v
    assert e["env32_coarse"] == e["d_coarse"]["f32_chain"]
    # the committed float32 fixture is one more float32 order of the same weights and inputs
    d_fix = max(seg_env.coarse_dev(z["coarse"], e["coarse"]["c64"]))
    print(f"{name}: max |fixture coarse - c64| {d_fix:.3e}, ENV32 {e['env32_coarse']:.3e}")
    assert d_fix <= SAFETY * e["env32_coarse"]
    # float64's label map is the fixture's outside the margins below twice the fp32 mean bar; those are at most 1 % of the pixels
    ref = e["fused"]["c64"]
    bar_mean = seg_env.bars(e, "fp32")[1]
    unsure = ref["margin"] < 2 * bar_mean
    print(f"{name}: fp32 mean bar {bar_mean:.3e}, {float(unsure.double().mean()):.3%} of the pixels below twice it")
    assert float(unsure.double().mean()) <= 0.01
    assert bool((ref["amax"] == torch.from_numpy(z["label"]).long())[~unsure].all())
    assert 0 < e["fuse_bar"] <= e["fuse_bar_worst"]           # the collect's bar for these logits never exceeds the one for any logits that large
    # the bars order as the arithmetic does, and stay far below the 1e-3 max |logit| line the fixtures' near-tie condition is stated at
    assert e["d_coarse"]["f32_chain"] < e["d_coarse"]["x3"] < e["d_coarse"]["bf16"]
    assert seg_env.bars(e, "bf16x3")[1] < 1e-3 * float(ref["mean"].abs().max())
    # the tap: at least 256 channels of c64's conv_fov input, float64, the envelopes ordered the same way
    t = e["tap"]
    sizes = [tuple(-(-int(s) // 8) for s in z["sizes"][k]) for k in (0, len(z["sizes"]) - 1)]
    assert [int(i) for i in t["tap_passes"]] == [0, 2 * (len(z["sizes"]) - 1)]
    for i, (fh, fw) in zip(t["tap_passes"], sizes):
        tap = t[f"tap_{i}"]
        assert tap.dtype == np.float64 and tap.shape == (fh, fw, len(range(int(t["c0"]), 4096, int(t["stride"])))) and tap.shape[2] >= 256
        assert set(range(int(t["c0"]), 4096, int(t["stride"]))[j] // 256 for j in range(tap.shape[2])) == set(range(16))
        assert float(tap.min()) == 0.0 and float(tap.max()) <= float(t[f"tapmax_{i}"])          # a ReLU's output
        assert 0 < float(t[f"dev_f32_chain_{i}"]) < float(t[f"dev_x3_{i}"]) < float(t[f"dev_bf16_{i}"])
        for v in t["tap_variants"]:
            assert float(t[f"devsub_{v}_{i}"]) <= float(t[f"dev_{v}_{i}"])
    for f in os.listdir(GOLDEN):
        if f.startswith(name):
            assert os.path.getsize(os.path.join(GOLDEN, f)) < 1 << 20, f


@pytest.mark.parametrize("name", CASES)
def test_the_bars_tell_a_wrong_mode_from_a_right_one(name):
    """stored variants standing in for a GPU run (their collect in float64): the sequential float32 chain passes the fp32 rules and the
    split-bf16 sum the bf16x3 rules; the reference's bfloat16 run fails both, and the split-bf16 sum fails fp32's"""
    from tests import seg_env
    e = load_env(name)

    def run(mode, v):
        f = e["fused"][v]
        print(f"{name}: {v} judged as {mode}")
        return seg_env.judge(e, mode, e["coarse"][v], f["mean"], f["amax"], f["margin"], f32_collect=False)
    assert run("fp32", "f32_chain") == []
    assert run("fp32", "c64") == []
    assert run("bf16x3", "x3") == []
    assert run("bf16x3", "f32_chain") == []
    for mode in ("fp32", "bf16x3"):
        failed = run(mode, "bf16")
        assert "coarse" in failed and "mean" in failed, failed
    assert "coarse" in run("fp32", "x3")
