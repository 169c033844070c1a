"""wseg_aff_pairs_backward (csrc/aff_loss.hip) against float64 autograd of aff = exp(-mean_c |f_to - f_from|) on the pair set of
resnet38_aff.indices_of_pairs, every element inside a bar derived from the kernel's arithmetic (the convention of tests/f64_bars.py:
u = 2^-24, SAFETY = 2 on the error terms, never fitted to a run).

The bar.  A row of d_feat is  sum over the pairs the pixel belongs to of  k * sign(f_to - f_from),  k = d_aff * (-aff / C).
  the sign          exact: an f32 (or bf16) subtraction never rounds across zero, and sign(0) = 0
  aff, as read      wseg_aff_pairs' f32 value: one rounding per subtraction, 448 per accumulated |difference| in any order, one for the
                    division — at most (C + 2) u relative to the mean m, which the exponential turns into (C + 2) u m relative to aff — and
                    expf's 2 ulp = 4 u (the HIP math API's bound, as tests/conv_f64.py takes expm1f's): rho = ((C + 2) m + 4) u
  k                 two more roundings (the division by C, the product): rho + 2 u
  the gather        at most 2 P terms are added to a partial sum <= sum |k|: 2 P u sum |k|
  bar[q]            SAFETY (sum_pairs |k| (rho + 2 u) + 2 P u sum_pairs |k|), the same for every channel of the row; the f32 store is exact.
A pixel in no pair has bar 0: its row must be exactly zero.  Where two feature rows tie on a channel the reference contributes an exact
zero (torch's abs backward), so a kernel with sign(0) = 1 would miss the bar by |k|, five orders of magnitude above it.
"""
import numpy as np
import pytest
import torch

from tests.f64_bars import SAFETY, U32

pytestmark = pytest.mark.gpu

C = 448
# (N, h, w, radius, duplicated rows)
CASES = [(2, 7, 7, 3, False), (2, 13, 13, 5, False), (2, 9, 12, 4, False), (2, 7, 7, 3, True)]
_refs = {}


def _reference(N, h, w, r, dup, dtype):
    """feature rows (values of `dtype`), d_aff, the float64 gradient and the bar per row: computed once, never written to"""
    key = (N, h, w, r, dup, dtype)
    if key in _refs:
        return _refs[key]
    from wseg_amd.resnet38_aff import indices_of_pairs, pair_offsets
    g = torch.Generator().manual_seed(100 * h + w + (7 if dup else 0))
    feat = (torch.rand(N, h * w, C, generator=g) * 2 - 1).to(dtype)
    if dup:                                     # whole rows and single channels repeated: exact zeros of f_to - f_from
        feat[:, 1::3] = feat[:, 0:-1:3][:, :feat[:, 1::3].shape[1]]
        feat[:, :, ::5] = feat[:, :1, ::5]
    ind_from, ind_to = (torch.from_numpy(i) for i in indices_of_pairs(r, (h, w)))
    P, n_from = len(pair_offsets(r)), ind_from.numel()
    d_aff = torch.rand(N, P, n_from, generator=g) * 2 - 1
    f = feat.double().requires_grad_(True)
    ff = f[:, ind_from].unsqueeze(1)                                  # [N, 1, n_from, C]
    ft = f[:, ind_to].view(N, P, n_from, C)
    m = (ft - ff).abs().mean(-1)
    aff = torch.exp(-m)
    (aff * d_aff.double()).sum().backward()
    k = (d_aff.double().abs() * aff.detach() / C)                     # |k| per pair
    rho = ((C + 2) * m.detach() + 4) * U32
    per_pair = k * (rho + 2 * U32) + 2 * P * U32 * k
    bar = torch.zeros(N, h * w, dtype=torch.float64)
    bar.index_add_(1, ind_from, per_pair.sum(1))
    bar.index_add_(1, ind_to, per_pair.reshape(N, -1))
    in_pair = torch.zeros(h * w, dtype=torch.bool)
    in_pair[ind_from] = True
    in_pair[ind_to] = True
    _refs[key] = (feat, d_aff, f.grad, SAFETY * bar, in_pair, (f.grad == 0).double().mean().item())
    return _refs[key]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("case", CASES, ids=[f"{n}x{h}x{w}_r{r}{'_dup' if d else ''}" for n, h, w, r, d in CASES])
def test_aff_pairs_backward_f64(case, dtype):
    from wseg_amd import _lib as L
    N, h, w, r, dup = case
    feat, d_aff, ref, bar, in_pair, zero_share = _reference(N, h, w, r, dup, dtype)
    assert bool((~in_pair).any()), "the case must hold pixels that belong to no pair"
    if dup:
        assert zero_share > 0.1, "the duplicated rows must produce exact zeros of f_to - f_from"
    rows = feat.reshape(N * h * w, C).contiguous().cuda()
    P, n_from = d_aff.shape[1:]
    aff = torch.empty(N, P, n_from, device="cuda", dtype=torch.float32)
    L.aff_pairs(rows, C, C, aff, N, h, w, r)
    outs = []
    for _ in range(2):
        d_feat = torch.full((N * h * w, C), float("nan"), device="cuda", dtype=torch.float32)
        L.aff_pairs_backward(rows, C, C, aff, d_aff.cuda(), d_feat, C, N, h, w, r)
        outs.append(d_feat)
    assert torch.equal(outs[0], outs[1]), "two runs must be bit-identical"
    got = outs[0].double().cpu().view(N, h * w, C)
    err = (got - ref).abs()
    worst = float((err / bar.unsqueeze(-1).clamp_min(1e-300)).max())
    print(f"aff_pairs_backward {case} {dtype}: max err {float(err.max()):.3e}, max err/bar {worst:.3f}, |ref| max {float(ref.abs().max()):.3e}")
    assert bool((err <= bar.unsqueeze(-1)).all())
    assert bool((got[:, ~in_pair] == 0).all()), "rows of pixels in no pair must be exactly zero"


def test_aff_pairs_backward_keeps_the_columns_behind_C():
    """ld_d > C: the columns >= C of every row are untouched (the write contract of the loss backward, whose row walk this is)"""
    from wseg_amd import _lib as L
    N, h, w, r = 1, 7, 7, 3
    feat, d_aff, _ref, _bar, _p, _z = _reference(N, h, w, r, False, torch.float32)
    rows = feat.reshape(N * h * w, C).contiguous().cuda()
    aff = torch.empty(N, d_aff.shape[1], d_aff.shape[2], device="cuda", dtype=torch.float32)
    L.aff_pairs(rows, C, C, aff, N, h, w, r)
    tight = torch.empty(N * h * w, C, device="cuda", dtype=torch.float32)
    L.aff_pairs_backward(rows, C, C, aff, d_aff[:N].cuda(), tight, C, N, h, w, r)
    wide = torch.full((N * h * w, C + 8), -7.0, device="cuda", dtype=torch.float32)
    L.aff_pairs_backward(rows, C, C, aff, d_aff[:N].cuda(), wide, C + 8, N, h, w, r)
    assert torch.equal(wide[:, :C], tight) and bool((wide[:, C:] == -7.0).all())
