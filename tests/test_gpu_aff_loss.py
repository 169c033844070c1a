"""The AffinityNet training loss on the GPU (csrc/aff_loss.hip, wseg_amd/aff_loss.py) against the float64 restatement and the bars derived
in tests/aff_loss_f64.py (from the kernels' arithmetic, safety factor 2, never fitted to a run), against the reference's recorded loss and
gradient, and on the label and tie edge cases.  The restatement runs on the device in float64, once per case."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import aff_loss_f64 as A
from tests.f64_bars import _gen
from wseg_amd import _lib as L, synth
from wseg_amd.aff_loss import AffinityLoss, aff_loss_rows, aff_loss_rows_backward, affinity_loss, pair_labels
from wseg_amd.resnet38_aff import pair_radius

pytestmark = pytest.mark.gpu
DEV = "cuda"

# (h, w, radius, N, feature scale): the smallest map the reference accepts, two maps whose sides are no multiple of anything, the training map
# (3 images: 7488 from pixels = 1872 workgroups, more than the 256 threads of the finish kernel take in one pass).  The scale moves
# the affinities: ~0.4 at 1.0, ~0.97 at 0.05 (where log(1.00001 - aff) is badly conditioned and the bars say so).
SHAPES = [(5, 7, 2, 1, 1.0), (8, 11, 3, 2, 0.05), (13, 16, 5, 2, 0.3), (56, 56, 5, 3, 1.0)]
# (C, ld, dtype): the AffinityNet's 448 in both dtypes, one active lane, all 64 lanes, and rows wider than their channels
CHANNELS = [(448, 448, torch.float32), (448, 448, torch.bfloat16), (8, 8, torch.float32), (512, 512, torch.float32), (64, 96, torch.float32)]
F32_1E5 = float(np.float32(1e-5))


def features(N, C, h, w, seed, dtype=torch.float32, scale=1.0):
    """[N, C, h, w] on the device: ELU of a normal sample, as f9's output is"""
    return (F.elu(torch.randn(N, C, h, w, generator=_gen(seed))) * scale).to(dtype).to(DEV)


def label_maps(N, h, w, seed, block=2):
    return torch.stack([synth.synthetic_aff_label_map(h, w, seed + i, block=block) for i in range(N)]).to(DEV)


def to_rows(feat, ld):
    """engine layout [N*h*w][ld]: channels contiguous, the columns >= C hold something that is not a feature"""
    N, C, h, w = feat.shape
    rows = torch.full((N * h * w, ld), 1e3, dtype=feat.dtype, device=feat.device)
    rows[:, :C] = feat.permute(0, 2, 3, 1).reshape(-1, C)
    return rows


def run_rows(feat, label, r, ld=None, ld_d=None, gscale=None):
    N, C, h, w = feat.shape
    ld, ld_d = ld or C, ld_d or C
    out7, ctx = aff_loss_rows(to_rows(feat, ld), ld, C, label, N, h, w, r)
    d = torch.full((N * h * w, ld_d), float("nan"), device=DEV)
    aff_loss_rows_backward(ctx, gscale, out=d, ld_d=ld_d)
    return out7, ctx["aff"], d


def assert_within(name, got, ref, bar):
    err = (got.double() - ref).abs()
    worst = float((err - bar).max())
    print(f"{name}: max |err| {float(err.max()):.3e}, max bar {float(torch.as_tensor(bar).max()):.3e}, max (err - bar) {worst:.3e}")
    assert torch.isfinite(got).all() and worst <= 0.0, name


def assert_matches_restatement(feat, label, r, out7, aff, d_nchw, gscale=1.0):
    ref = A.restate(feat, label, r, gscale=gscale)
    cnt = [A.f32_count(c) for c in ref["counts"]]
    print("pairs bg/fg/neg", ref["counts"], "out7", out7.tolist())
    assert out7[4:].tolist() == cnt                                             # the counts are exact
    assert_within("out7", out7[:4], ref["out7"][:4], ref["bar_out7"][:4])
    if aff is not None:
        assert_within("aff", aff, ref["aff"], ref["bar_aff"])
    assert_within("d_feat", d_nchw, ref["grad"], ref["bar_grad"])
    return ref


@pytest.mark.parametrize("C,ld,dtype", CHANNELS, ids=lambda v: str(v).replace("torch.", ""))
@pytest.mark.parametrize("h,w,r,N,scale", SHAPES)
def test_kernels_against_f64(h, w, r, N, scale, C, ld, dtype):
    feat = features(N, C, h, w, 100 + h, dtype, scale)
    label = label_maps(N, h, w, 7 + h, block=2 if h < 56 else 3)
    out7, aff, d = run_rows(feat, label, r, ld, ld)
    ref = assert_matches_restatement(feat, label, r, out7, aff, d[:, :C].view(N, h, w, C).permute(0, 3, 1, 2))
    assert min(ref["counts"]) > 0                                               # no term is tested on an empty sum
    if ld > C:                                                                  # columns >= C untouched, columns < C all written
        assert torch.isnan(d[:, C:]).all() and torch.isfinite(d[:, :C]).all()


@pytest.mark.parametrize("name", ["aff_loss_7x7", "aff_loss_13x13"])
def test_reference_fixture_through_affinity_loss(golden_dir, name):
    """The reference's own loss and dL/dz (float32, CPU, recorded) from the recorded pre-ELU z: bar = the restatement's recorded distance to
    the reference (2 x measured, tests/aff_loss_f64.py) plus the kernels' derived bar.  ELU and its derivative are applied on the host, as
    the reference's run did, so that the loss layer alone is under test."""
    g = np.load(os.path.join(golden_dir, name + ".npz"))
    z = torch.from_numpy(g["z"])
    r = int(g["radius"])
    assert r == pair_radius(*z.shape[2:])
    feat = F.elu(z).to(DEV).requires_grad_()
    label = torch.from_numpy(g["label"]).to(DEV)
    loss, stats = affinity_loss(feat, label)                                    # radius None: the reference's rule
    loss.backward()
    ref = A.restate(feat, label, r, need_grad=True)
    want = torch.from_numpy(g["out7"]).double().to(DEV)
    assert stats[4:].tolist() == g["out7"][4:].tolist() and float(loss.detach()) == float(stats[0])
    assert_within("scalars", stats[:4], want[:4], A.REF_BAR_OUT7 * want[:4].abs() + ref["bar_out7"][:4])
    sel = torch.from_numpy(g["dz_channels"]).to(DEV)
    de = A.elu_grad(z.double()).to(DEV)
    dz = (feat.grad.double() * de)[:, sel]
    dz_ref = torch.from_numpy(g["dz"]).double().to(DEV)
    assert_within("dL/dz", dz, dz_ref, A.REF_BAR_DZ * dz_ref.abs().max() + (ref["bar_grad"] * de)[:, sel])


def test_label_edge_cases():
    N, C, h, w, r = 2, 64, 8, 11, 3
    feat = features(N, C, h, w, 5)
    empty = [0.0, 0.0, 0.0, 0.0, F32_1E5, F32_1E5, F32_1E5]
    # all ignore: exactly the empty scalars, an exactly zero gradient, nothing NaN / Inf
    out7, aff, d = run_rows(feat, torch.full((N, h, w), 255, dtype=torch.uint8, device=DEV), r)
    assert out7.tolist() == empty and torch.equal(d, torch.zeros_like(d)) and torch.isfinite(aff).all()
    # a single labelled pixel is in no valid pair
    one = torch.full((N, h, w), 255, dtype=torch.uint8, device=DEV)
    one[1, 3, 5] = 3
    out7, _, d = run_rows(feat, one, r)
    assert out7.tolist() == empty and torch.equal(d, torch.zeros_like(d))
    # all background: every pair is a bg pair, the other two terms are exactly 0
    zeros = torch.zeros((N, h, w), dtype=torch.uint8, device=DEV)
    out7, aff, d = run_rows(feat, zeros, r)
    assert out7[2:4].tolist() == [0.0, 0.0] and out7[5:].tolist() == [F32_1E5, F32_1E5]
    assert float(out7[4]) == A.f32_count(aff.numel()) and float(out7[1]) > 0 and float(out7[0]) == float(out7[1]) / 4
    assert_matches_restatement(feat, zeros, r, out7, aff, d.view(N, h, w, C).permute(0, 3, 1, 2))
    # one class everywhere: only fg
    out7, _, _ = run_rows(feat, torch.full((N, h, w), 7, dtype=torch.uint8, device=DEV), r)
    assert out7[1] == 0 and out7[3] == 0 and out7[2] > 0 and float(out7[5]) == A.f32_count(aff.numel())


def test_exact_ties_give_exactly_zero():
    """sign(0) = 0 (torch's abs backward).  Channel groups that are constant over the map (ELU saturates at -1, and does so exactly) tie in
    every pair: their gradient is exactly 0.  Duplicated neighbouring rows tie on every channel of their own pair."""
    N, C, h, w, r = 2, 64, 8, 11, 3
    feat = features(N, C, h, w, 6)
    feat[:, 8:16] = -1.0                                                        # one whole lane's 8 channels
    feat[:, 30:34] = 0.37                                                       # a group across two lanes
    feat[:, :, 2, 4] = feat[:, :, 2, 5]                                         # from (2,4) / to (2,5): offset (0, 1)
    feat[:, :, 4, 6] = feat[:, :, 3, 5]                                         # from (3,5) / to (4,6): offset (1, 1)
    label = label_maps(N, h, w, 21)
    out7, aff, d = run_rows(feat, label, r)
    d = d.view(N, h, w, C).permute(0, 3, 1, 2)
    assert torch.equal(d[:, 8:16], torch.zeros_like(d[:, 8:16])) and torch.equal(d[:, 30:34], torch.zeros_like(d[:, 30:34]))
    assert d.abs().max() > 0
    assert_matches_restatement(feat, label, r, out7, aff, d)
    # with ALL rows equal every pair ties on every channel: aff = 1 exactly and no gradient at all, while the loss is not zero
    same = feat[:, :, :1, :1].expand(N, C, h, w).contiguous()
    out7, aff, d = run_rows(same, label, r)
    assert torch.equal(aff, torch.ones_like(aff)) and torch.equal(d, torch.zeros_like(d)) and float(out7[3]) > 10.0


def test_run_to_run_bit_identical():
    N, C, h, w, r = 3, 448, 56, 56, 5
    feat = features(N, C, h, w, 8, torch.bfloat16)
    label = label_maps(N, h, w, 31, block=3)
    a, b = run_rows(feat, label, r), run_rows(feat, label, r)
    for x, y in zip(a, b):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))


def test_loss_only_call_gives_the_same_bits():
    N, C, h, w, r = 2, 448, 13, 16, 5
    feat = features(N, C, h, w, 9)
    label = label_maps(N, h, w, 41)
    rows = to_rows(feat, C)
    with_aff, ctx = aff_loss_rows(rows, C, C, label, N, h, w, r)
    without, ctx0 = aff_loss_rows(rows, C, C, label, N, h, w, r, with_aff=False)
    assert ctx0["aff"] is None and torch.equal(with_aff.view(torch.int32), without.view(torch.int32))
    with pytest.raises(RuntimeError, match="with_aff=False"):
        aff_loss_rows_backward(ctx0)
    # the affinities are those of the inference kernel, bit for bit
    aff = torch.empty_like(ctx["aff"])
    L.aff_pairs(rows, C, C, aff, N, h, w, r)
    assert torch.equal(aff.view(torch.int32), ctx["aff"].view(torch.int32))


@pytest.mark.parametrize("channels_last", [True, False], ids=["channels_last", "contiguous"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_autograd_against_plain_torch(dtype, channels_last):
    """AffinityLoss against the reference's formulation in plain torch on the device (index_select gathers, float label tensors, f32) on
    the same values, with a non-unit upstream gradient.  Both are f32 evaluations of one function: the plain one's chains are no longer
    than the kernels' (tree reductions over C and over the pairs, the same 2 P accumulations per row in its index_select backward, the
    same expf / logf), so each lies within the derived bar of the float64 value and the two within twice the bar of each other.  A
    gradient returned in bf16 adds one bf16 rounding of its value (2^-8 relative: aff_loss_f64.bf16_store_bar)."""
    N, C, h, w, r = 2, 448, 13, 16, 5
    base = features(N, C, h, w, 10, dtype, 0.3)
    feat = base.clone(memory_format=torch.channels_last if channels_last else torch.contiguous_format).requires_grad_()
    label = label_maps(N, h, w, 51)
    loss, stats = affinity_loss(feat, label, r)
    assert stats.requires_grad is False and loss.shape == () and stats.shape == (7,) and float(loss.detach()) == float(stats[0])
    if channels_last:                                                           # consumed in place: the rows ARE the tensor
        assert loss.grad_fn.saved["rows"].data_ptr() == feat.data_ptr()
    (3 * loss).backward()
    g = feat.grad
    assert g.dtype == dtype and g.shape == feat.shape
    assert g.is_contiguous(memory_format=torch.channels_last) if channels_last else g.is_contiguous()

    plain_in = base.detach().float().clone().requires_grad_()
    labels = [torch.from_numpy(np.stack([pair_labels(m, r)[j] for m in label.cpu().numpy()])).to(DEV) for j in range(3)]
    p_loss, p_stats = A.plain_torch_loss(plain_in, labels, r)
    (3 * p_loss).backward()
    ref = A.restate(base, label, r, gscale=3.0)
    assert stats[4:].tolist() == p_stats[4:].tolist() == [A.f32_count(c) for c in ref["counts"]]
    assert_within("scalars vs plain torch", stats[:4], p_stats[:4].double(), 2 * ref["bar_out7"][:4])
    stored = A.bf16_store_bar if dtype == torch.bfloat16 else (lambda _ref, bar: bar)
    assert_within("gradient vs plain torch", g.float(), plain_in.grad.double(), stored(ref["grad"], 2 * ref["bar_grad"]))
    assert_within("gradient vs float64", g.float(), ref["grad"], stored(ref["grad"], ref["bar_grad"]))
    # a second backward through the same Function with another upstream gradient, and the module-level alias
    feat.grad = None
    loss2, _ = AffinityLoss.apply(feat, label, r)
    loss2.backward()
    assert_within("unit upstream gradient", feat.grad.float() * 3, ref["grad"], stored(ref["grad"], ref["bar_grad"]))
