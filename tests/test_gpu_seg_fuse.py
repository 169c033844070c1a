"""wseg_seg_fuse (csrc/seg.hip) on its own against the float64 restatement of test.py's collect step (tests/seg_f64.py).

Bars (the convention of tests/test_gpu_loss_kernels.py: derived, safety factor 2, never fitted to a run): the mean logits are held to
seg_f64.fuse_bar — the bilinear bar of tests/f64_bars.py applied twice plus the roundings of the running sum and the division; the
softmax adds its own roundings (PROB_BAR); the arg-max is exact wherever the float64 top-2 margin is at least twice the mean's bar, and
the first-maximum rule is checked on constructed exact ties.  bf16 rows are read exactly (the float64 side sees the same bf16 values).
"""
import pytest
import torch

from tests import seg_f64
from tests.f64_bars import SAFETY, U32

pytestmark = pytest.mark.gpu

LD = 24


def _rows(coarse, dtype, ld=LD):
    """[n, C, fh, fw] float -> pixel rows [n * fh * fw, ld] of `dtype` on the device (columns >= C hold a poison the kernel must not use)"""
    n, C, fh, fw = coarse.shape
    rows = torch.full((n * fh * fw, ld), 1e30)
    rows[:, :C] = coarse.permute(0, 2, 3, 1).reshape(-1, C)
    return rows.to(dtype).cuda()


def _case(seed, n_cls, dims, dtype, H, W):
    """dims: [(fh, fw, ih, iw, flip)] one entry per pass, each pass its own one-image batch"""
    from wseg_amd import _lib as L
    g = torch.Generator().manual_seed(seed)
    passes, ref_passes = [], []
    for (fh, fw, ih, iw, flip) in dims:
        c = (4.0 * torch.randn(1, n_cls, fh, fw, generator=g)).to(dtype).float()      # the values both sides see
        passes.append(L.SegPass(_rows(c, dtype), LD, 0, fh, fw, ih, iw, flip))
        ref_passes.append((c[0], (ih, iw), flip))
    return passes, ref_passes


def _run(passes, H, W, n_cls):
    from wseg_amd import _lib as L
    out = dict(mean=torch.empty(n_cls, H, W, device="cuda"), prob=torch.empty(n_cls, H, W, device="cuda"),
               amax=torch.empty(H, W, device="cuda", dtype=torch.uint8), margin=torch.empty(H, W, device="cuda"))
    L.seg_fuse(passes, H, W, n_cls, out["amax"], out["mean"], out["prob"], out["margin"])
    return {k: v.cpu() for k, v in out.items()}


def _check(passes, ref_passes, H, W, n_cls, what):
    got = _run(passes, H, W, n_cls)
    ref = seg_f64.fuse(ref_passes, H, W)
    M = max(float(c.abs().max()) for c, _s, _f in ref_passes)
    bar = seg_f64.fuse_bar(ref_passes, M)
    err = float((got["mean"].double() - ref["mean"]).abs().max())
    print(f"{what}: max |dmean| {err:.3e} (bar {bar:.3e}, max |logit| {M:.2f})")
    assert err <= bar
    # softmax of a mean that is `bar` off: |dp| <= p (1 - p) 2 bar <= bar / 2, plus expf (2 U32), n_cls sum roundings and the quotient
    prob_bar = 0.5 * bar + SAFETY * (n_cls + 4) * U32
    assert float((got["prob"].double() - ref["prob"]).abs().max()) <= prob_bar
    assert float((got["margin"].double() - ref["margin"]).abs().max()) <= 2 * bar + SAFETY * U32 * 2 * M
    sure = ref["margin"] >= 2 * bar
    assert float(sure.double().mean()) >= 0.95
    assert bool((got["amax"].long()[sure] == ref["amax"][sure]).all())
    return got


SHAPES = [
    # (coarse, intermediate, output): every coarse size of the issue; intermediates both smaller and larger than the output; H or W = 1
    ((1, 1), (8, 8), (5, 9)),
    ((2, 3), (16, 24), (11, 13)),
    ((5, 7), (40, 56), (33, 47)),
    ((5, 7), (20, 28), (40, 56)),
    ((13, 16), (100, 125), (57, 301)),          # more than one block, W no multiple of the block
    ((5, 7), (40, 56), (1, 37)),
    ((5, 7), (40, 56), (29, 1)),
    ((2, 3), (1, 24), (7, 9)),                  # an intermediate of one row: stage 1 divides by ih - 1 = 0
    ((1, 4), (9, 1), (6, 5)),
]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "c%dx%d_i%dx%d_o%dx%d" % (s[0] + s[1] + s[2]))
def test_one_and_two_passes_against_float64(shape, dtype):
    (fh, fw), (ih, iw), (H, W) = shape
    for n_cls in (21, 2):
        passes, ref = _case(11 + n_cls, n_cls, [(fh, fw, ih, iw, False)], dtype, H, W)
        _check(passes, ref, H, W, n_cls, f"1 pass n_cls {n_cls}")
        passes, ref = _case(23 + n_cls, n_cls, [(fh, fw, ih, iw, False), (fh, fw, ih, iw, True)], dtype, H, W)
        _check(passes, ref, H, W, n_cls, f"plain + flipped n_cls {n_cls}")


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_twelve_passes_odd_width(dtype):
    """the reference's schedule on a 33 x 47 image: six scales, plain then flipped, intermediates from 16 x 24 to 58 x 82"""
    H, W = 33, 47
    dims = []
    for (ih, iw), (fh, fw) in zip([(16, 24), (25, 35), (33, 47), (41, 59), (50, 70), (58, 82)], [(2, 3), (4, 5), (5, 6), (6, 8), (7, 9), (8, 11)]):
        dims += [(fh, fw, ih, iw, False), (fh, fw, ih, iw, True)]
    passes, ref = _case(5, 21, dims, dtype, H, W)
    _check(passes, ref, H, W, 21, "12 passes")


def test_flip_samples_the_mirrored_column_and_batches_index_by_image():
    """A flipped pass alone equals the plain pass's result mirrored, bit for bit (torch.flip after the resize); image 1 of an N = 2 batch is
    read from its own rows."""
    from wseg_amd import _lib as L
    H, W, fh, fw, ih, iw = 19, 31, 5, 7, 40, 56
    g = torch.Generator().manual_seed(3)
    c = 4.0 * torch.randn(2, 21, fh, fw, generator=g)
    rows = _rows(c, torch.float32)
    plain0 = _run([L.SegPass(rows, LD, 0, fh, fw, ih, iw, False)], H, W, 21)
    plain1 = _run([L.SegPass(rows, LD, 1, fh, fw, ih, iw, False)], H, W, 21)
    flip1 = _run([L.SegPass(rows, LD, 1, fh, fw, ih, iw, True)], H, W, 21)
    alone1 = _run([L.SegPass(_rows(c[1:], torch.float32), LD, 0, fh, fw, ih, iw, False)], H, W, 21)
    assert torch.equal(plain1["mean"], alone1["mean"]) and not torch.equal(plain0["mean"], plain1["mean"])
    assert torch.equal(flip1["mean"], plain1["mean"].flip(-1))
    assert torch.equal(flip1["amax"], plain1["amax"].flip(-1))


def test_first_maximum_wins_on_exact_ties():
    from wseg_amd import _lib as L
    H, W = 6, 10
    c = torch.zeros(1, 21, 2, 2)
    c[0, 4] = c[0, 9] = c[0, 17] = 3.0            # three classes tie exactly everywhere (constant planes resample exactly)
    c[0, 2, 0, 0] = 5.5                           # class 2 wins near one corner (5.5 (5 - y) (9 - x) / 45 is 3 at no pixel)
    got = _run([L.SegPass(_rows(c, torch.float32), LD, 0, 2, 2, 12, 20, False)], H, W, 21)
    ref = seg_f64.fuse([(c[0], (12, 20), False)], H, W)
    tie = ref["mean"][4] >= ref["mean"][2]
    assert bool(tie.any()) and bool((~tie).any())
    assert bool((got["amax"][tie] == 4).all()) and bool((got["amax"][~tie] == 2).all())
    assert bool((got["margin"][tie & (ref["mean"][4] > ref["mean"][2])] == 0).all())
    two = torch.zeros(1, 2, 1, 1)
    got2 = _run([L.SegPass(_rows(two, torch.float32), LD, 0, 1, 1, 3, 3, False)], 4, 4, 2)
    assert bool((got2["amax"] == 0).all()) and bool((got2["prob"] == 0.5).all())


def test_bad_arguments_are_refused():
    from wseg_amd import _lib as L
    rows = torch.zeros(35, LD, device="cuda")
    amax = torch.empty(8, 8, device="cuda", dtype=torch.uint8)
    with pytest.raises(RuntimeError):
        L.seg_fuse([L.SegPass(rows, LD, 1, 5, 7, 40, 56, False)], 8, 8, 21, amax)           # image 1 of a one-image batch
    with pytest.raises(RuntimeError):
        L.seg_fuse([L.SegPass(rows[:, :16].contiguous(), 16, 0, 5, 7, 40, 56, False)], 8, 8, 21, amax)      # ld < 24
    with pytest.raises(RuntimeError):
        L.seg_fuse([L.SegPass(rows, LD, 0, 5, 7, 40, 56, False)] * 17, 8, 8, 21, amax)
    with pytest.raises(RuntimeError):
        L.seg_fuse([L.SegPass(rows, LD, 0, 5, 7, 40, 56, False)], 8, 8, 33, amax)
