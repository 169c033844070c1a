"""Float64 restatement of the AffinityNet training loss (aff_train.py:111-119 on network/resnet38_aff.py:57-63) with the label rule of
voc12/data.py:170-199 on a label map, and the error bars of the HIP kernels (csrc/aff_loss.hip) derived from their arithmetic.
TEST INFRASTRUCTURE, no tests here.

restate(feat, label, radius) gathers the pairs over resnet38_aff.indices_of_pairs, takes exp(-mean|ft - ff|), applies the three terms and
lets autograd produce the gradient, all in float64 on feat's device.  Two things are taken over from the specification AS F32 VALUES,
because they are part of what is computed, not errors of computing it: the constants 1e-5 and 1.00001 (= f32(1. + 1e-5): the
reference folds the two Python floats and hands one f32 scalar to the tensor op), and cnt = f32(count) + f32(1e-5) rounded to f32.  For
bf16 inputs the restatement takes the same bf16-rounded values; the kernel's conversion to f32 is exact, so the bars do not change.

How the bars are set (the convention of tests/f64_bars.py: from the kernel's arithmetic, safety factor 2, never fitted to a run).
u = U32 = 2^-24; every bound is first order in u.
  s = sum_c |ft_c - ff_c|    one rounding per difference (|.| is exact), 7 additions per lane (8 channels, the first lands on 0), then the
                             6-step butterfly: 14 roundings on any path through non-negative terms -> relatively 14 u; m = s / C: 15 u
  aff = expf(-m)             the argument error 15 u m shows as a relative error of aff, plus expf's documented 1 ulp = 2 u:
                             d_aff = aff (15 u m + 2 u)                                                          [the bar of `aff`]
  T = -logf(arg)             arg = aff + 1e-5 or 1.00001 - aff, one rounding: d_arg = d_aff + u arg; the logarithm turns it into
                             d_arg / arg absolute (this is the conditioning of log(1.00001 - aff) near aff = 1: it is evaluated per pair on
                             the float64 aff, not assumed), plus logf's documented 1 ulp = 2 u of |T|:  d_T = d_arg / arg + 2 u |T|
  sums                       a wave adds its <= P terms of a kind in sequence, the workgroup adds 4 waves (P + 3 roundings of non-negative
                             partial sums), the finish kernel adds the workgroups in f64 (negligible):  d_S = sum d_T + (P + 3) u S
  x_loss = S / cnt           cnt as specified (exact), the quotient rounded once to f32 (taken as 2 u):  d_S / cnt + 2 u x_loss
  loss                       /4 and /2 are exact, two additions: d_bg / 4 + d_fg / 4 + d_neg / 2 + 3 u loss
  counts                     integers throughout: exact, bar 0
  gradient                   per pair k = g w / arg * aff / C with w = 1 / (4 cnt) or 1 / (2 cnt): relatively d_arg / arg + d_aff / aff from
                             its two inputs and 5 roundings (g / (4 cnt): 2, / arg, aff / C, the product): d_k = |k| (d_arg/arg + d_aff/aff + 5 u)
                             sign(ft_c - ff_c) is exact in f32 (a difference of two floats rounds to zero only if they are equal), k * sign is
                             exact; a pixel's row accumulates its <= 2 P pairs in sequence, each addition within u of a partial sum
                             <= sum |k|:  d_row = sum_pairs d_k + 2 P u sum_pairs |k|   (one bar per pixel, for all its channels)
"""
import numpy as np
import torch

from tests.f64_bars import SAFETY, U32
from wseg_amd.resnet38_aff import indices_of_pairs, pair_offsets

EPS = float(np.float32(1e-5))                  # log(aff + 1e-5)
ONE_PLUS_EPS = float(np.float32(1.00001))      # log(1. + 1e-5 - aff)
N_SUM = 14                                     # roundings on a path of the |diff| sum
EXP_ULP = LOG_ULP = 2.0 * U32                  # expf, logf: 1 ulp (HIP math API)
U_BF16 = 2.0 ** -8                             # bf16 unit roundoff: 8 significand bits (7 stored), round to nearest -> half an ulp = 2^-8 relative


def bf16_store_bar(ref, bar):
    """bar of a value computed within `bar` of `ref` and then rounded to bf16: the rounding is within U_BF16 of the computed value"""
    return bar + U_BF16 * (ref.abs() + bar)

# restate() against the REFERENCE's float32 CPU outputs in tests/golden/aff_loss_{7x7,13x13}.npz (scripts/make_aff_loss_goldens.py prints
# and stores the deviations when it makes the fixtures): worst relative deviation, max |a - b| / max |b| per tensor and |a - b| / |b| per
# scalar, over both fixtures.  Measured:
#   aff 8.28e-8 (13x13)     seven scalars 1.68e-7 (13x13)     dL/dz 1.69e-7 (7x7)
# bar = 2 x measured; the margin covers another BLAS / thread count where the restatement is evaluated again.
REF_BAR_AFF, REF_BAR_OUT7, REF_BAR_DZ = 1.66e-7, 3.36e-7, 3.38e-7


def f32_count(c):
    """cnt of the specification: f32(count) + f32(1e-5), rounded to f32"""
    return float(np.float32(c) + np.float32(1e-5))


def pair_kinds(label, radius):
    """(bg, fg, neg) bool [N, P, n_from] of a uint8 [N, h, w] label tensor: the rule of voc12/data.py:182-197 per pair"""
    N, h, w = label.shape
    ind_from, ind_to = (torch.from_numpy(a).to(label.device) for a in indices_of_pairs(radius, (h, w)))
    lab = label.reshape(N, -1).long()
    lf = lab[:, ind_from][:, None, :]
    lt = lab[:, ind_to].view(N, len(pair_offsets(radius)), -1)
    valid = (lf < 255) & (lt < 255)
    pos = lf == lt
    return pos & (lf == 0), pos & (lf != 0) & valid, ~pos & valid


def restate(feat, label, radius, gscale=1.0, need_grad=True):
    """feat [N, C, h, w] (any float dtype: its values are taken as they are), label uint8 [N, h, w] on the same device.
    Returns a dict: out7 [7], aff [N, P, n_from], grad [N, C, h, w] = gscale * d loss / d feat (all float64), counts (3 ints), and the
    bars bar_out7 [7], bar_aff [N, P, n_from], bar_grad [N, 1, h, w] (safety factor included)."""
    N, C, h, w = feat.shape
    dev = feat.device
    P = len(pair_offsets(radius))
    ind_from, ind_to = (torch.from_numpy(a).to(dev) for a in indices_of_pairs(radius, (h, w)))
    x = feat.detach().double().reshape(N, C, h * w).requires_grad_(need_grad)
    ff = torch.index_select(x, 2, ind_from).unsqueeze(2)
    ft = torch.index_select(x, 2, ind_to).view(N, C, P, -1)
    m = torch.mean(torch.abs(ft - ff), dim=1)
    aff = torch.exp(-m)
    kinds = pair_kinds(label, radius)
    counts = [int(k.sum()) for k in kinds]
    cnt = [f32_count(c) for c in counts]
    t_pos, t_neg = -torch.log(aff + EPS), -torch.log(ONE_PLUS_EPS - aff)
    terms = [t_pos, t_pos, t_neg]
    sums = [(t * k).sum() for t, k in zip(terms, kinds)]
    losses = [s / c for s, c in zip(sums, cnt)]
    loss = losses[0] / 4 + losses[1] / 4 + losses[2] / 2
    grad = None
    if need_grad:
        (gscale * loss).backward()
        grad = x.grad.view(N, C, h, w)
    with torch.no_grad():
        aff, m = aff.detach(), m.detach()
        out7 = torch.stack([loss.detach(), *[v.detach() for v in losses], *[torch.tensor(c, dtype=torch.float64, device=dev) for c in cnt]])
        d_aff = aff * ((N_SUM + 1) * U32 * m + EXP_ULP)
        args = [aff + EPS, aff + EPS, ONE_PLUS_EPS - aff]
        bar_loss, d_k_sum, k_sum = [], torch.zeros_like(aff), torch.zeros_like(aff)
        for j in range(3):
            kf = kinds[j].double()
            rel_arg = (d_aff + U32 * args[j]) / args[j]
            d_t = rel_arg + LOG_ULP * terms[j].detach().abs()
            d_s = (d_t * kf).sum() + (P + 3) * U32 * sums[j].detach().abs()
            bar_loss.append(d_s / cnt[j] + 2 * U32 * losses[j].detach().abs())
            k = kf * abs(gscale) / ((4.0 if j < 2 else 2.0) * cnt[j]) / args[j] * aff / C
            k_sum += k
            d_k_sum += k * (rel_arg + d_aff / aff + 5 * U32)
        bar_total = bar_loss[0] / 4 + bar_loss[1] / 4 + bar_loss[2] / 2 + 3 * U32 * loss.detach().abs()
        zero = torch.zeros((), dtype=torch.float64, device=dev)
        bar_out7 = SAFETY * torch.stack([bar_total, *bar_loss, zero, zero, zero])
        per_pair = d_k_sum + 2 * P * U32 * k_sum                               # [N, P, n_from]
        bar_grad = torch.zeros(N, h * w, dtype=torch.float64, device=dev)
        bar_grad.index_add_(1, ind_from, per_pair.sum(dim=1))
        bar_grad.index_add_(1, ind_to, per_pair.reshape(N, -1))
    return dict(out7=out7, aff=aff, grad=grad, counts=counts, bar_out7=bar_out7, bar_aff=SAFETY * d_aff,
                bar_grad=SAFETY * bar_grad.view(N, 1, h, w))


def plain_torch_loss(feat, labels, radius):
    """The reference's formulation (two index_select gathers of [N, C, P * n_from], the three [N, P, n_from] float label tensors `labels`
    = (bg, fg, neg) as multipliers) in feat's dtype on feat's device: (loss, the 7 scalars)."""
    N, C, h, w = feat.shape
    P = len(pair_offsets(radius))
    ind_from, ind_to = (torch.from_numpy(a).to(feat.device) for a in indices_of_pairs(radius, (h, w)))
    x = feat.reshape(N, C, h * w)
    src = torch.index_select(x, 2, ind_from).unsqueeze(2)
    dst = torch.index_select(x, 2, ind_to).view(N, C, P, -1)
    aff = torch.exp(-(dst - src).abs().mean(dim=1))
    return loss_from_aff(aff, labels)


def loss_from_aff(aff, labels):
    """The three loss lines of aff_train.py:111-119 on aff [N, P, n_from] and the label tensors (bg, fg, neg): (loss, the 7 scalars)."""
    cnt = [lab.sum() + 1e-5 for lab in labels]
    nll = [-torch.log(aff + 1e-5)] * 2 + [-torch.log((1. + 1e-5) - aff)]
    part = [(lab * t).sum() / c for lab, t, c in zip(labels, nll, cnt)]
    loss = part[0] / 4 + part[1] / 4 + part[2] / 2
    return loss, torch.stack([loss, *part, *cnt]).detach()


def elu(z):
    return torch.where(z > 0, z, torch.expm1(z))


def elu_grad(z):
    return torch.where(z > 0, torch.ones_like(z), torch.exp(z))
