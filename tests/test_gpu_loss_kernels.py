"""GPU: the loss-phase kernels one entry point at a time (csrc/maps.hip, csrc/loss.hip, csrc/nce.hip, the planar resizes of
csrc/head.hip) against float64 CPU references of the same operation.

How the bars are set: every tolerance is derived from the kernel's arithmetic, never fitted to a run.
  u = 2^-24, the unit roundoff of f32.  A sum of m f32 terms accumulated in a serial chain of length c has error
  <= c * u * sum|terms|; every bar below states its chain and carries a safety factor of 2.
Decisions (arg-max / arg-min, top-k membership, max_onehot, pseudo-label arg-max) are not arithmetic: the arithmetic is
compared under the kernel's own decisions, and every decision that differs from the float64 one is asserted to be a
near-tie of the float64 values within the derived value bar (where the kernel does not return its decision — the rank band
of nce_fused — the pixels whose float64 values are such near-ties are left out, and their share is capped).  Exact ties are built from dyadic values (multiples of
1/64 on grids whose interpolation weights are multiples of 1/16), where f32 and float64 agree bit for bit, and the
stated tie rule is asserted exactly.
"""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from .f64_bars import SAFETY, U32, _bits, _coord_bar, _gen, _interp_bar     # (shared with test_gpu_pcm_head_kernels.py)
# the float64 references and bar helpers live in tests/loss_f64.py, where the stage judge of the loss phase (test_gpu_loss_stages.py) uses them too
from .loss_f64 import (NCE_CI, NCE_MAX_EXCLUDED, S_BAR, _exact_grid, _label_full, _max_norm_inj, _nce_reference, _nce_sum_bar, _proto_bar, _protos64,
                       _resize64, _resize_bwd64, _select_ref, _stats_chain, _up64, sampling_rule)

pytestmark = pytest.mark.gpu

DEV = "cuda"


def _L():
    from wseg_amd import _lib as L
    return L


# ------------------------------------------------------------------------------------------------ planar resize (head.hip)
RESIZE_CASES = [(56, 56, 448, 448), (21, 21, 500, 500), (16, 16, 128, 128), (448, 448, 56, 56), (16, 16, 16, 16),
                (13, 11, 97, 40), (7, 5, 1, 1), (1, 1, 9, 9)]


@pytest.mark.parametrize("align", [True, False])
@pytest.mark.parametrize("ih,iw,oh,ow", RESIZE_CASES)
def test_resize_planar_fwd_and_bwd(ih, iw, oh, ow, align):
    L = _L()
    g = _gen(11 + ih * 7 + ow)
    planes = 3
    x = torch.randn(planes, ih, iw, generator=g)
    dy = torch.randn(planes, oh, ow, generator=g)
    mul = torch.tensor([0.5, -1.25, 3.0])
    add = torch.tensor([0.25, 0.0, -0.75])
    M = float(x.abs().max())
    # forward: one sample (_coord_bar per axis on |p1 - p0| <= 2M, 6 roundings); the plane multiplier and accumulate add one each
    fbar = SAFETY * (2.0 * _coord_bar(max(ih, iw)) * 2.0 * M + 6.0 * U32 * M)
    ref = _resize64(x, oh, ow, align)
    out = torch.empty(planes, oh, ow, device=DEV)
    L.resize_planar_fwd(x.to(DEV), out, planes, ih, iw, oh, ow, align)
    torch.testing.assert_close(out.cpu().double(), ref, rtol=0, atol=fbar)
    flipped = torch.empty_like(out)
    L.resize_planar_fwd(x.to(DEV), flipped, planes, ih, iw, oh, ow, align, flip_x=True)
    assert torch.equal(flipped.cpu(), torch.flip(out.cpu(), dims=[-1]))         # the same samples, mirrored: bit-equal
    base = torch.randn(planes, oh, ow, generator=g)
    acc = base.to(DEV)
    L.resize_planar_fwd(x.to(DEV), acc, planes, ih, iw, oh, ow, align, plane_mul=mul.to(DEV), accumulate=True)
    torch.testing.assert_close(acc.cpu().double(), base.double() + ref * mul.double()[:, None, None], rtol=0,
                               atol=fbar * 3.0 + SAFETY * 2.0 * U32 * float((base.double() + ref * mul.double()[:, None, None]).abs().max()))

    # backward: gather over the outputs that touch an input pixel: at most nx * ny of them (nx = 2 ow / iw + 3); each term's
    # weights carry |delta f| <= _coord_bar per axis plus 4 roundings, the row / column sums are chains of nx + ny + 2
    nx, ny = math.ceil(2 * ow / iw) + 3, math.ceil(2 * oh / ih) + 3
    G = float((dy.abs() + add.abs()[:, None, None]).max())

    def bbar(T2, m=1.0):
        return SAFETY * m * ((2.0 * _coord_bar(max(ih, iw)) + 4.0 * U32) * nx * ny * G + (nx + ny + 4) * U32 * T2)

    ref_b = _resize_bwd64(dy, ih, iw, align)
    T2 = _resize_bwd64(dy.abs() + add.abs()[:, None, None], ih, iw, align)
    d_in = torch.empty(planes, ih, iw, device=DEV)
    L.resize_planar_bwd(dy.to(DEV), d_in, planes, ih, iw, oh, ow, align)
    err = (d_in.cpu().double() - ref_b).abs()
    assert bool((err <= bbar(T2)).all()), f"resize_planar_bwd align={align}: max err {float(err.max()):.3e} (bar {float(bbar(T2).max()):.3e})"
    # <resize(x), g> == <x, resize_bwd(g)> on the kernel outputs, in float64
    lhs, rhs = float((out.cpu().double() * dy.double()).sum()), float((x.double() * d_in.cpu().double()).sum())
    dbar = float((x.double().abs() * bbar(T2)).sum()) + fbar * float(dy.double().abs().sum())
    assert abs(lhs - rhs) <= dbar, (lhs, rhs, dbar)
    # plane_mul, plane_add (a constant added to every d_out of the plane) and accumulate
    ref_c = _resize_bwd64(dy + add[:, None, None], ih, iw, align) * mul.double()[:, None, None]
    base_i = torch.randn(planes, ih, iw, generator=g)
    acc_i = base_i.to(DEV)
    L.resize_planar_bwd(dy.to(DEV), acc_i, planes, ih, iw, oh, ow, align, accumulate=True, plane_mul=mul.to(DEV), plane_add=add.to(DEV))
    err = (acc_i.cpu().double() - base_i.double() - ref_c).abs()
    bar = bbar(T2, 3.0) * 2.0 + SAFETY * U32 * (base_i.double().abs() + ref_c.abs())
    assert bool((err <= bar).all()), f"resize_planar_bwd (mul/add/acc) align={align}: max err {float(err.max()):.3e}"


# ------------------------------------------------------------------------------------------------ radix select (loss.hip)
def _value_set(kind, rows, n, g):
    if kind == "gauss":
        return torch.randn(rows, n, generator=g)
    if kind == "quant":                        # multiples of 1/64: massive exact ties, +0 and -0 both present
        v = (torch.randn(rows, n, generator=g) * 8).round() / 64
        v.view(-1)[0::7] = 0.0
        v.view(-1)[3::7] = -0.0
        return v
    if kind == "equal":
        return torch.full((rows, n), 0.75)
    if kind == "negative":
        return -(torch.rand(rows, n, generator=g) + 0.01)
    if kind == "inf":
        v = torch.randn(rows, n, generator=g)
        v.view(-1)[1::97] = float("inf")
        v.view(-1)[5::89] = float("-inf")
        return v
    raise ValueError(kind)


def _same_nonfinite(a, b):
    return (math.isnan(a) and math.isnan(b)) or a == b


@pytest.mark.parametrize("kind", ["gauss", "quant", "equal", "negative", "inf"])
@pytest.mark.parametrize("n,rows", [(448 * 448, 1), (21 * 128 * 128, 2), (4099, 4), (1, 4)])
def test_select_kth_and_finish(n, rows, kind):
    """n = 4099 runs the n % 4 != 0 scalar loops of select_hist / select_sum."""
    L = _L()
    g = _gen(n % 1000 + len(kind))
    v = _value_set(kind, rows, n, g)
    v64 = v.double()
    vd = v.to(DEV)
    ws = torch.empty(L.select_workspace_bytes(rows), device=DEV, dtype=torch.uint8)
    gs = max(1, min(32, (n + 8191) // 8192))
    per_thread = (math.ceil(n / (4 * gs * 256)) * 4) if n % 4 == 0 else math.ceil(n / (gs * 256))
    chain = per_thread + 6 + 4 + gs                # serial per thread, wave tree, 4 waves, same-address atomics of the workgroups
    for k in sorted({1, n // 4, int(0.2 * n), n} - {0}):
        for largest in (True, False):
            for use_abs in (False, True):
                for relu in (False, True):
                    thr, s, cs, ce, sabs = _select_ref(v64, k, largest, use_abs, relu)
                    res = torch.empty(rows, 4, device=DEV)
                    L.select_kth(vd, rows, n, k, largest, use_abs, relu, res, ws)
                    scale = 0.5 / k
                    loss = torch.zeros(1, device=DEV)
                    L.select_finish(res, rows, k, relu, scale, loss)
                    r = res.cpu().double()
                    what = f"k={k} largest={largest} abs={use_abs} relu={relu}"
                    assert torch.equal(r[:, 0], thr), what                          # thresholds: exact (-0 == +0)
                    assert torch.equal(r[:, 2], cs) and torch.equal(r[:, 3], ce), what   # counts: exact integers
                    fin_ref, fin_abs, fin_bar = 0.0, 0.0, 0.0
                    for i in range(rows):
                        t = max(float(thr[i]), 0.0) if relu else float(thr[i])
                        if math.isfinite(float(s[i])):
                            bar = SAFETY * chain * U32 * float(sabs[i])
                            assert abs(float(r[i, 1]) - float(s[i])) <= bar, (what, i, float(r[i, 1]), float(s[i]))
                        else:
                            assert _same_nonfinite(float(r[i, 1]), float(s[i])), (what, i, float(r[i, 1]), float(s[i]))
                        fin_ref += float(s[i]) + (k - float(cs[i])) * t       # (0 * inf = nan, as in the kernel)
                        fin_abs += float(sabs[i]) + abs(k - float(cs[i])) * abs(t)
                        fin_bar += SAFETY * chain * U32 * float(sabs[i])
                    got = float(loss.cpu()[0])
                    ref = fin_ref * scale
                    if math.isfinite(ref):
                        # + the finish loop: 3 roundings per row and a chain of `rows` adds, then the scale and the atomic
                        bar = scale * (fin_bar + SAFETY * (rows + 5) * U32 * fin_abs)
                        assert abs(got - ref) <= bar, (what, got, ref, bar)
                    else:
                        assert _same_nonfinite(got, ref), (what, got, ref)


# ------------------------------------------------------------------------------------------------ plane statistics
def _special_planes(low):
    low[0] = -(low[0].abs() + 0.25)            # all-negative plane: relu == 0 everywhere -> max / min at index 0
    low[1] = 0.0                               # constant plane -> index 0
    return low


# (h, w, S, planes): 448 / 128 / 160 crops, non-square + odd S, the S > 1024 plain-column loop, planes > 4096 (chunks = 1),
# and a dyadic grid (scales 1/8 and 1/16) on which U is exact: ties and first-index rules are asserted exactly there
UP_STATS_CASES = [(56, 56, 448, 42), (16, 16, 128, 42), (20, 20, 160, 21), (13, 11, 97, 21), (130, 130, 1040, 2),
                  (5, 5, 40, 4200), (17, 9, 129, 21)]


@pytest.mark.parametrize("h,w,S,planes", UP_STATS_CASES)
def test_up_plane_stats(h, w, S, planes):
    L = _L()
    g = _gen(h * 1000 + S + planes)
    exact = _exact_grid(h, w, S)
    low = torch.randn(planes, h, w, generator=g)
    if exact:
        low = (low * 16).round() / 64
        low[2, 1:3, 1:3] = float(low.max()) + 1.0           # a flat maximum: many hi-res pixels tie, the first must win
    low = _special_planes(low)
    chunks = max(1, min(min(16, S // 16), max(1, 4096 // planes)))
    stats = torch.empty(planes, 6, device=DEV)
    L.up_plane_stats(low.to(DEV), stats, planes, h, w, S)
    st = stats.cpu()
    U = _up64(low, S).view(planes, -1)
    R = U.clamp_min(0)
    M = float(low.abs().max())
    ubar = 0.0 if exact else _interp_bar(h, w, M)
    imx, imn = _bits(st[:, 3]), _bits(st[:, 4])
    assert bool(((imx >= 0) & (imx < S * S) & (imn >= 0) & (imn < S * S)).all())
    rows = torch.arange(planes)
    vmx, vmn = R[rows, imx], R[rows, imn]
    # values under the kernel's decisions
    assert bool(((st[:, 0].double() - vmx).abs() <= ubar).all())
    assert bool(((st[:, 1].double() - vmn).abs() <= ubar).all())
    # a decision that differs from the float64 one is a near-tie of the float64 values
    assert bool((vmx >= R.max(1).values - 2 * ubar).all())
    assert bool((vmn <= R.min(1).values + 2 * ubar).all())
    if exact:                                                 # first index, bit-exact
        Rn = R.numpy()
        assert imx.tolist() == [int(np.argmax(r)) for r in Rn]
        assert imn.tolist() == [int(np.argmin(r)) for r in Rn]
    assert imx[:2].tolist() == [0, 0] and imn[:2].tolist() == [0, 0]
    assert st[:2, 0].tolist() == [0.0, 0.0] and st[:2, 1].tolist() == [0.0, 0.0]
    # sum of U: the accumulation chain plus every sample's own error
    sbar = SAFETY * (_stats_chain(S, chunks) + 1) * U32 * U.abs().sum(1) + S * S * ubar
    assert bool(((st[:, 2].double() - U.sum(1)).abs() <= sbar).all())

    # the label20 gate: labelled planes (and bg) equal to the ungated run (max / min / args bit-equal; the sum only up to
    # the order of its float atomics, inside the same chain bar); unlabelled planes are not read downstream
    N = (planes + 20) // 21
    label20 = (torch.rand(N, 20, generator=g) < 0.5).float()
    stats_l = torch.empty(planes, 6, device=DEV)
    L.up_plane_stats(low.to(DEV), stats_l, planes, h, w, S, label20.to(DEV))
    lab = torch.cat([torch.ones(N, 1), label20], 1).view(-1)[:planes] > 0
    sl = stats_l.cpu()
    assert torch.equal(sl[lab][:, [0, 1, 3, 4, 5]], st[lab][:, [0, 1, 3, 4, 5]])
    assert bool(((sl[lab][:, 2].double() - st[lab][:, 2].double()).abs() <= 2 * sbar[lab]).all())

    # plane_stats on materialised f32 planes: same contract, decisions on the same f32 values are exact
    if S * S * planes <= 9_000_000:
        U32t = U.float()
        st2 = torch.empty(planes, 6, device=DEV)
        L.plane_stats(U32t.to(DEV), st2, planes, S * S)
        st2 = st2.cpu()
        R32 = U32t.clamp_min(0).double().numpy()
        assert st2[:, 0].tolist() == [float(r.max()) for r in R32]
        assert st2[:, 1].tolist() == [float(r.min()) for r in R32]
        assert _bits(st2[:, 3]).tolist() == [int(np.argmax(r)) for r in R32]
        assert _bits(st2[:, 4]).tolist() == [int(np.argmin(r)) for r in R32]
        pchunks = max(1, min(min(64, S * S // 8192), max(1, 2048 // planes)))
        pbar = SAFETY * (_stats_chain(S, pchunks) + 1) * U32 * U32t.double().abs().sum(1)
        assert bool(((st2[:, 2].double() - U32t.double().sum(1)).abs() <= pbar).all())


# ------------------------------------------------------------------------------------------------ classification loss
@pytest.mark.parametrize("zmag", [0.1, 30.0, 100.0])
@pytest.mark.parametrize("labels", ["random", "zeros", "ones"])
def test_cls_loss(zmag, labels):
    L = _L()
    g = _gen(int(zmag * 10) + len(labels))
    N, npix, coef = 3, 448 * 448, 0.5
    z = zmag * torch.where(torch.rand(N, 21, generator=g) < 0.5, -1.0, 1.0) * (0.5 + torch.rand(N, 21, generator=g))
    y = {"random": (torch.rand(N, 20, generator=g) < 0.5).float(), "zeros": torch.zeros(N, 20), "ones": torch.ones(N, 20)}[labels]
    stats = torch.zeros(N * 21, 6)
    stats[:, 2] = (z * npix).view(-1)
    loss = torch.zeros(1, device=DEV)
    bias = torch.empty(N * 21, device=DEV)
    L.cls_loss(stats.to(DEV), y.to(DEV), loss, bias, N, npix, coef)
    z64 = stats[:, 2].double().view(N, 21) / npix
    ref = F.multilabel_soft_margin_loss(z64[:, 1:], y.double())
    # per term: z carries one rounding (u |z| through a slope <= 1), exp / log1p / min / sub / mul about 8 roundings of
    # |term| + |log1p|; the block sum is a chain of 1 + 6 + 4; then / (20 N) and the atomic
    zz = z64[:, 1:]
    terms = F.binary_cross_entropy_with_logits(zz, y.double(), reduction="none")
    l1p = torch.log1p(torch.exp(-zz.abs()))
    term_err = (U32 * (zz.abs() + 8 * (terms + l1p))).sum()
    bar = SAFETY * (float(term_err) + 11 * U32 * float(terms.sum())) / (20 * N) + SAFETY * 2 * U32 * float(ref)
    assert abs(float(loss.cpu()[0]) - float(ref)) <= bar, (float(loss.cpu()[0]), float(ref), bar)
    b = bias.cpu().double().view(N, 21)
    assert torch.equal(b[:, 0], torch.zeros(N, dtype=torch.float64))
    sg = torch.sigmoid(zz)
    ref_b = coef * (sg - y.double()) / (20 * N) / npix
    # sigmoid in f32: |delta sg| <= u (|z| sg (1-sg) + 4 sg); then (sg - y), * coef, / (20 N), / npix: 4 roundings
    # (+ 2^-126: at |z| = 100 exp overflows / sg underflows below the normal f32 range)
    bbar = SAFETY * coef / (20 * N * npix) * (U32 * (zz.abs() * sg * (1 - sg) + 4 * sg) + 4 * U32 * (sg - y.double()).abs() + 2.0 ** -126)
    assert bool(((b[:, 1:] - ref_b).abs() <= bbar).all()), float((b[:, 1:] - ref_b).abs().max())


# ------------------------------------------------------------------------------------------------ min-pool values + loss
@pytest.mark.parametrize("h,w,S", [(56, 56, 448), (16, 16, 128), (13, 11, 97), (17, 9, 129)])
def test_up_rvmin_values_and_min_pool_loss(h, w, S):
    from oracle.loss import adaptive_min_pooling_loss
    L = _L()
    g = _gen(S + 5)
    N = 2
    exact = _exact_grid(h, w, S)
    low = torch.rand(N, 21, h, w, generator=g)
    label20 = (torch.rand(N, 20, generator=g) < 0.4).float()
    label20[:, 2] = 1.0; label20[:, 6] = 1.0; label20[:, 9] = 0.0               # an absent class; two labelled classes that tie
    if exact:
        low = (low * 64).round() / 64
    low[:, 7] = low[:, 3]                      # channels 3 and 7 (labels 2 and 6) identical: the first channel (3) must win
    low[:, 3, 0, 0] = low[:, 7, 0, 0] = 2.0    # the tie is also the maximum at pixel 0
    q = torch.empty(N, S * S, device=DEV)
    argc = torch.empty(N, S * S, device=DEV, dtype=torch.uint8)
    L.up_rvmin_values(low.to(DEV).contiguous(), label20.to(DEV), q, argc, N, h, w, S)
    U = _up64(low.view(N * 21, h, w), S).view(N, 21, S * S)
    lab = torch.cat([torch.ones(N, 1), label20], 1).double()
    prod = (U * lab[:, :, None])[:, 1:]
    ubar = 0.0 if exact else _interp_bar(h, w, float(low.abs().max()))
    qk, ak = q.cpu().double(), argc.cpu().long()
    assert bool(((ak >= 1) & (ak <= 20)).all())
    val_at = torch.gather(prod, 1, (ak - 1)[:, None]).squeeze(1)
    assert bool(((qk - val_at).abs() <= ubar).all())                    # q under the kernel's arg channel
    assert bool((val_at >= prod.max(1).values - 2 * ubar).all())        # a different arg channel is a near-tie
    assert bool((ak[:, 0] == 3).all())                                   # exact tie: the first channel wins
    if exact:
        assert torch.equal(qk, prod.max(1).values)
        assert torch.equal(ak - 1, torch.from_numpy(np.argmax(prod.numpy(), axis=1)))
    # the loss: k = S*S // 4 smallest relu(q) per image, through select_kth + select_finish
    k = S * S // 4
    res = torch.empty(N, 4, device=DEV)
    ws = torch.empty(L.select_workspace_bytes(N), device=DEV, dtype=torch.uint8)
    L.select_kth(q, N, S * S, k, False, False, True, res, ws)
    loss = torch.zeros(1, device=DEV)
    L.select_finish(res, N, k, True, 1.0 / (k * N), loss)
    ref = float(adaptive_min_pooling_loss(prod.view(N, 20, S, S)))
    gs = max(1, min(32, (S * S + 8191) // 8192))
    chain = S * S / (gs * 256) + 4 + 10 + gs + N + 3
    # each selected value moves by <= ubar (the k-smallest sum is 1-Lipschitz per element); the sums' chain on max q
    bar = ubar + SAFETY * chain * U32 * float(qk.abs().max())
    assert abs(float(loss.cpu()[0]) - ref) <= bar, (float(loss.cpu()[0]), ref, bar)


# ------------------------------------------------------------------------------------------------ max-norm + resize
@pytest.mark.parametrize("h,w,S", [(56, 56, 448), (20, 20, 160), (16, 16, 128), (13, 11, 97)])
def test_up_norm_resize_forward(h, w, S):
    L = _L()
    g = _gen(S + 17)
    N, OS = 2, 128
    low = torch.rand(N * 21, h, w, generator=g) * 2 - 0.3
    label20 = (torch.rand(N, 20, generator=g) < 0.5).float()
    stats = torch.empty(N * 21, 6, device=DEV)
    L.up_plane_stats(low.to(DEV), stats, N * 21, h, w, S)
    out = torch.empty(N, 21, OS, OS, device=DEV)
    L.up_norm_resize_forward(low.to(DEV), stats, label20.to(DEV), out, N, h, w, S, OS)
    st = stats.cpu()
    imx, imn = _bits(st[:, 3]), _bits(st[:, 4])
    U = _up64(low, S).view(N * 21, -1)
    A = _max_norm_inj(U, imx, imn).view(N * 21, S, S)
    lab = torch.cat([torch.ones(N, 1), label20], 1).double().view(-1)
    ref = (_resize64(A, OS, OS, True) * lab[:, None, None]).view(N, 21, OS, OS)
    R = U.clamp_min(0)
    D = (R.max(1).values - R.min(1).values + 1e-5)
    ubar = _interp_bar(h, w, float(low.abs().max()))
    # max_norm moves by <= 3 ubar / D (the sample, mx and mn each off by ubar) plus 3 roundings of values <= 1; the second
    # resize adds its own coordinate error (values <= 1 differ by <= 1) and 6 roundings
    bar = (SAFETY * (3 * ubar / D + 3 * U32) + _interp_bar(S, S, 1.0)).view(N, 21, 1, 1) * lab.view(N, 21, 1, 1)
    err = (out.cpu().double() - ref).abs()
    assert bool((err <= bar).all()), float(err.max())
    assert bool((out.cpu()[lab.view(N, 21) == 0] == 0).all())                # unlabelled planes: exactly 0


@pytest.mark.parametrize("h,S", [(56, 448), (16, 128), (13, 97), (1, 448)])
def test_resize_adjoint_ones(h, S):
    L = _L()
    wv = torch.empty(h, device=DEV)
    L.resize_adjoint_ones(wv, h, S)
    x = torch.zeros(1, 1, h, dtype=torch.float64, requires_grad=True)
    F.interpolate(x, size=S, mode="linear", align_corners=True).sum().backward()
    ref = x.grad.view(-1)
    # S serial adds of weights <= 1 (chain S on the total ref[y]); every weight off by <= 2 |delta f| over the <= 2S/h + 2 outputs
    bar = SAFETY * (S * U32 * ref + 2 * _coord_bar(h) * (2 * S / h + 2))
    assert bool(((wv.cpu().double() - ref).abs() <= bar).all()), (wv.cpu(), ref)


# ------------------------------------------------------------------------------------------------ up_maps_backward
MAPS_BWD_CASES = ([(56, 56, 448, t) for t in ("cam", "rv")] +
                  [(h, w, S, t) for h, w, S in [(16, 16, 128), (13, 11, 97), (17, 9, 129)] for t in ("norm", "bias", "sel", "cam", "rv")])


@pytest.mark.parametrize("h,w,S,term", MAPS_BWD_CASES)
def test_up_maps_backward(h, w, S, term):
    """Each term alone and the two configurations loss_hip.py launches (cam: norm + GAP bias; rv: norm + min-pool
    selection), against float64 autograd under the kernel's max / min / top-k decisions.  S = 97 and 129 run the
    unvectorised selection loop (odd S*S); (17, 9, 129) is h != w on an exact grid where the selection has exact ties."""
    L = _L()
    g = _gen(S * 3 + len(term))
    N, OS = 2, 128
    exact = _exact_grid(h, w, S)
    low = torch.rand(N * 21, h, w, generator=g) * 1.5 + 0.05       # positive maps: relu and the max_norm gate are not near-ties
    if exact:
        low = (low * 64).round() / 64
    low[5] = -(low[5] + 0.125)                                    # (n 0, class 5): U <= 0 -> max / min routes must be skipped
    label20 = (torch.rand(N, 20, generator=g) < 0.5).float()
    label20[0, 4] = 1.0; label20[0, 2] = 0.0                      # class 5 labelled, class 3 unlabelled
    lab = _label_full(label20)
    do_norm, do_bias, do_sel = term in ("norm", "cam", "rv"), term in ("bias", "cam"), term in ("sel", "rv")
    lowd = low.to(DEV).contiguous()
    stats = torch.empty(N * 21, 6, device=DEV)
    L.up_plane_stats(lowd, stats, N * 21, h, w, S, label20.to(DEV) if term in ("sel", "rv") else None)
    G = torch.randn(N * 21, OS, OS, generator=g) if do_norm else None
    bias = (torch.randn(N * 21, generator=g) * 1e-3) if do_bias else None
    if bias is not None:
        bias.view(N, 21)[:, 0] = 0.0
    wy = wx = q = argc = res = None
    k, coef = 0, 0.0
    if do_bias:
        wy, wx = torch.empty(h, device=DEV), torch.empty(w, device=DEV)
        L.resize_adjoint_ones(wy, h, S); L.resize_adjoint_ones(wx, w, S)
    if do_sel:
        q = torch.empty(N, S * S, device=DEV)
        argc = torch.empty(N, S * S, device=DEV, dtype=torch.uint8)
        L.up_rvmin_values(lowd, label20.to(DEV), q, argc, N, h, w, S)
        k, coef = S * S // 4, 0.5 / (S * S // 4 * N)
        res = torch.empty(N, 4, device=DEV)
        ws = torch.empty(L.select_workspace_bytes(N), device=DEV, dtype=torch.uint8)
        L.select_kth(q, N, S * S, k, False, False, True, res, ws)
    d_low = torch.empty(N * 21, h, w, device=DEV)
    L.up_maps_backward(G.to(DEV) if G is not None else None, lowd, stats, label20.to(DEV),
                       bias.to(DEV) if bias is not None else None, wy, wx, q, argc, res, k, coef, d_low, N, h, w, S, OS)
    got = d_low.cpu().double()

    # float64 reference under the kernel's decisions
    st = stats.cpu()
    imx, imn = _bits(st[:, 3]), _bits(st[:, 4])
    L21 = lab.view(-1)
    x = low.double().clone().requires_grad_(True)
    U = _up64(x, S).view(N * 21, S * S)
    total = torch.zeros((), dtype=torch.float64)
    abs_hi = torch.zeros(N * 21, S * S, dtype=torch.float64)        # sum |terms| reaching every hi-res pixel (for the bars)
    ubar = 0.0 if exact else _interp_bar(h, w, float(low.abs().max()))
    if do_norm:
        labelled = L21 != 0
        ls = torch.nonzero(labelled).view(-1)
        A = _max_norm_inj(U[ls], imx[ls], imn[ls]).view(-1, S, S)
        out = _resize64(A, OS, OS, True)
        total = total + (out * G.double()[ls]).sum()
        Rl = U[ls].detach().clamp_min(0)
        rows = torch.arange(len(ls))
        D = Rl[rows, imx[ls]] - Rl[rows, imn[ls]] + 1e-5
        gabs = _resize_bwd64(G.abs()[ls], S, S, True).view(len(ls), -1)
        abs_hi[ls] += gabs / D[:, None]
        # the max / min routes: |At| + |At - Bt| <= 2 sum |t|, scattered from the arg-max / arg-min pixels
        route = 2 * gabs.sum(1) / D
        abs_hi[ls, imx[ls]] += route
        abs_hi[ls, imn[ls]] += route
    if do_bias:
        total = total + (U * bias.double()[:, None]).sum()
        abs_hi += bias.double().abs()[:, None]
    if do_sel:
        qk, ak, rk = q.cpu().double(), argc.cpu().long(), res.cpu().double()
        thr, cs, ce = rk[:, 0:1], rk[:, 2:3], rk[:, 3:4]
        wsel = torch.where(qk < thr, 1.0, torch.where(qk == thr, (k - cs) / ce.clamp_min(1), 0.0)) * (qk > 0)
        for c in range(1, 21):
            m = (ak == c).double() * wsel * coef * lab[:, c:c + 1]
            Uc = U.view(N, 21, S * S)[:, c]
            total = total + (m * Uc).sum()
            abs_hi.view(N, 21, -1)[:, c] += m.abs()
    if do_sel and exact:
        assert float(rk[:, 3].max()) > 1                          # ties at the threshold are present and share the remainder
    total.backward()
    ref = x.grad
    # bar per low-res cell: every hi-res term reaches a cell through one LDS atomic; a cell takes <= (2S/h + 3)(2S/w + 3)
    # hi-res pixels, each from <= (2 OS/S + 3)^2 outputs, plus 2 * chunks route / flush atomics and the 8-level A / B trees.
    # Weights carry the coordinate error (_coord_bar per axis, both resizes), and max / min / every gated sample the ubar
    # of the U they were read from (relative ubar / D on invD and on av).
    chunks = max(1, min(64, S * S // 2048))
    chain = (2 * S / h + 3) * (2 * S / w + 3) * (2 * OS / S + 3) ** 2 + 2 * chunks + 16 + OS * OS / (256 * chunks)
    cell_abs = _resize_bwd64(abs_hi.view(N * 21, S, S), h, w, True)
    rel = chain * U32 + 2 * (_coord_bar(max(h, w)) + _coord_bar(S))
    if do_norm and not exact:
        Dmin = float(D.min())
        rel += 3 * ubar / Dmin
    bar = SAFETY * rel * cell_abs
    err = (got - ref).abs()
    assert bool((err <= bar).all()), f"max err {float(err.max()):.3e} at {int(err.argmax())}, bar there {float(bar.view(-1)[err.argmax()]):.3e}"
    # unlabelled planes (and the bias-free c = 0 of the selection term) get exactly 0
    zero_planes = (L21 == 0) if not do_bias else ((L21 == 0) & (bias.double() == 0))
    assert bool((got[zero_planes] == 0).all())
    # plane (0, 5) has U <= 0: relu is 0 there, so nothing of the norm term reaches it (no max / min route either)
    if term == "norm":
        assert bool((got[5] == 0).all())


# ------------------------------------------------------------------------------------------------ ER / ECR
@pytest.mark.parametrize("N", [1, 2])
def test_er_ecr_prep_select_and_backward(N):
    from oracle.loss import max_onehot
    L = _L()
    g = _gen(40 + N)
    npix = 128 * 128
    c1 = (torch.rand(N, 21, npix, generator=g) * 64).floor() / 64        # dyadic CAMs: 1 - max is exact, max_onehot ties are exact
    c2 = (torch.rand(N, 21, npix, generator=g) * 64).floor() / 64
    c1[0, 3, 0] = c1[0, 8, 0] = 1.0                                      # two equal fg maxima at pixel 0
    c1[:, :, 1] = 0.0; c2[:, :, 1] = 0.0                                  # all-zero pixels
    r1, r2 = torch.randn(N, 21, npix, generator=g), torch.randn(N, 21, npix, generator=g)
    er_coef = 1.0 / (N * 20 * npix)
    d = [t.to(DEV).contiguous() for t in (c1, c2, r1, r2)]
    Gc1, Gc2 = torch.empty(N, 21, npix, device=DEV), torch.empty(N, 21, npix, device=DEV)
    dlt = torch.empty(2 * N, 21 * npix, device=DEV)
    er = torch.zeros(1, device=DEV)
    L.er_ecr_prep(*d, Gc1, Gc2, dlt[:N], dlt[N:], er, N, npix, er_coef)
    # ER sum: 20 adds per pixel, the block tree (6 + 4), one same-address atomic per block
    terms = (c1.double() - c2.double())[:, 1:].abs()
    chain = 20 + 10 + N * npix // 256
    assert abs(float(er.cpu()[0]) - float(terms.sum())) <= SAFETY * chain * U32 * float(terms.sum())
    sg = torch.sign(c1.double() - c2.double())
    ref_g = (sg * torch.tensor(er_coef, dtype=torch.float32).double())
    ref_g[:, 0] = 0.0
    assert torch.equal(Gc1.cpu().double(), ref_g) and torch.equal(Gc2.cpu().double(), -ref_g + 0.0)
    # dlt = r - onehot(other view): one correctly rounded f32 subtraction of exact operands -> bit-equal
    def onehot(c):
        x = c.double().clone()
        x[:, 0] = 1.0 - x[:, 1:].max(1).values
        return max_onehot(x.view(N, 21, npix, 1)).view(N, 21, npix)
    oh1, oh2 = onehot(c1), onehot(c2)
    assert int((oh1[0, 1:, 0] != 0).sum()) == 2                           # max_onehot keeps every tied maximum
    ref_d = torch.cat([(r1.double() - oh2).float().view(N, -1), (r2.double() - oh1).float().view(N, -1)])
    dl = dlt.cpu()
    assert torch.equal(dl, ref_d)
    # ECR selection (largest |dlt|) and its backward
    K = int(21 * npix * 0.2)
    coef = 1.0 / (N * K)
    res = torch.empty(2 * N, 4, device=DEV)
    ws = torch.empty(L.select_workspace_bytes(2 * N), device=DEV, dtype=torch.uint8)
    L.select_kth(dlt, 2 * N, 21 * npix, K, True, True, False, res, ws)
    loss = torch.zeros(1, device=DEV)
    L.select_finish(res, 2 * N, K, False, coef, loss)
    Gr = torch.empty(2 * N, 21 * npix, device=DEV)
    L.ecr_backward(dlt, res, Gr, 2 * N, 21 * npix, K, coef)
    a = dl.double().abs()
    top = torch.topk(a, K, dim=1).values
    thr = top[:, -1]
    r = res.cpu().double()
    assert torch.equal(r[:, 0], thr)
    cs, ce = (a > thr[:, None]).sum(1).double(), (a == thr[:, None]).sum(1).double()
    assert torch.equal(r[:, 2], cs) and torch.equal(r[:, 3], ce)
    gs = max(1, min(32, (21 * npix + 8191) // 8192))
    schain = math.ceil(21 * npix / (4 * gs * 256)) * 4 + 10 + gs + 2 * N + 3
    ref_loss = float(top.sum()) * coef
    assert abs(float(loss.cpu()[0]) - ref_loss) <= SAFETY * schain * U32 * ref_loss
    gr = Gr.cpu().double()
    sgn = torch.sign(dl.double())
    c32 = float(torch.tensor(coef, dtype=torch.float32))
    strict, tie = a > thr[:, None], a == thr[:, None]
    assert torch.equal(gr[strict], sgn[strict] * c32)                   # strict members: exactly +-coef
    assert bool((gr[~strict & ~tie] == 0).all())                         # outside the selection: exactly 0
    for i in range(2 * N):
        share = gr[i][tie[i]].abs()
        assert bool((share == share[0]).all())
        want = (K - float(cs[i])) * c32
        # each share: (k - cs) / ce and * coef, 2 roundings; their sum here is a float64 sum of ce equal terms
        assert abs(float(share.sum()) - want) <= SAFETY * 2 * U32 * want, (i, float(share.sum()), want)
        assert torch.equal(torch.sign(gr[i][tie[i]]), sgn[i][tie[i]])


# ------------------------------------------------------------------------------------------------ head rows resize + gradient
HEAD_LD = 192


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("ih,iw", [(56, 56), (16, 16), (13, 11)])
def test_rows_resize_forward_and_head_grad_fused(ih, iw, dtype):
    L = _L()
    g = _gen(ih * iw + (dtype == torch.bfloat16))
    N, oh, ow = 2, 16, 16
    head = torch.randn(N * ih * iw, HEAD_LD, generator=g)
    head[::5, :128:3] = 0.0                                               # exact zeros: masked in the gradient
    head = head.to(dtype)
    h64 = head.double()
    F_ = torch.empty(N * oh * ow, 128, device=DEV)
    L.rows_resize_forward(head.to(DEV), HEAD_LD, F_, N, ih, iw, oh, ow)
    x = h64[:, :128].view(N, ih, iw, 128).permute(0, 3, 1, 2)
    ref = F.interpolate(x, size=(oh, ow), mode="bilinear", align_corners=True).permute(0, 2, 3, 1).reshape(-1, 128)
    torch.testing.assert_close(F_.cpu().double(), ref, rtol=0, atol=_interp_bar(ih, iw, float(h64.abs().max())))

    dF = torch.randn(N * oh * ow, 128, generator=g)
    d_cam = torch.randn(N, 21, ih, iw, generator=g)
    d_head = torch.full((N * ih * iw, HEAD_LD), 7.0, dtype=dtype, device=DEV)
    L.head_grad_fused(dF.to(DEV), d_cam.to(DEV), head.to(DEV), d_head, HEAD_LD, N, ih, iw, oh, ow)
    xg = torch.zeros(N, 128, ih, iw, dtype=torch.float64, requires_grad=True)
    dF4 = dF.double().view(N, oh, ow, 128).permute(0, 3, 1, 2)
    (F.interpolate(xg, size=(oh, ow), mode="bilinear", align_corners=True) * dF4).sum().backward()
    adj = xg.grad.permute(0, 2, 3, 1).reshape(-1, 128)
    xa = torch.zeros(N, 128, ih, iw, dtype=torch.float64, requires_grad=True)
    (F.interpolate(xa, size=(oh, ow), mode="bilinear", align_corners=True) * dF4.abs()).sum().backward()
    T2 = xa.grad.permute(0, 2, 3, 1).reshape(-1, 128)
    mask = h64[:, :128] > 0
    ref_g = torch.where(mask, adj, torch.zeros((), dtype=torch.float64))
    # one serial chain over the <= nx * ny touching outputs (2 roundings each), weights off by _coord_bar per axis
    nx, ny = math.ceil(2 * ow / iw) + 3, math.ceil(2 * oh / ih) + 3
    bar = SAFETY * ((2 * _coord_bar(max(ih, iw)) + 4 * U32) * nx * ny * float(dF.abs().max()) + (nx * ny + 2) * U32 * T2)
    got = d_head.cpu().double()
    if dtype == torch.bfloat16:                                           # stored in bf16: one bf16 ulp of the float64 value
        bar = bar + torch.exp2(torch.floor(torch.log2(ref_g.abs().clamp_min(2.0 ** -126))) - 7)
    assert bool(((got[:, :128] - ref_g).abs() <= bar).all()), float((got[:, :128] - ref_g).abs().max())
    assert bool((got[:, :128][~mask] == 0).all())
    assert torch.equal(got[:, 128:149], d_cam.permute(0, 2, 3, 1).reshape(-1, 21).to(dtype).double())
    assert bool((got[:, 149:] == 0).all())


# ------------------------------------------------------------------------------------------------ pseudo labels
@pytest.mark.parametrize("bg", [0.2, 0.9])
@pytest.mark.parametrize("N", [1, 3])
def test_pseudo_label(N, bg):
    from oracle.loss import pseudo_labels_and_prototypes
    L = _L()
    g = _gen(N * 10 + int(bg * 10))
    npix = 256
    R = torch.randn(N, 21, 16, 16, generator=g) * 0.5 + 0.3
    R[:, 5] = 0.3                                                         # a constant class plane (mx == mn)
    label20 = (torch.rand(N, 20, generator=g) < 0.3).float()
    label20[:, 4] = 1.0; label20[:, 10] = 0.0
    y = torch.empty(N * npix, device=DEV, dtype=torch.int32)
    ncam = torch.empty(N, 21, npix, device=DEV)
    L.pseudo_label(R.to(DEV), label20.to(DEV), bg, y, ncam, N, npix)
    nk, yk = ncam.cpu(), y.cpu().long()
    # the kernel's zeroing decision v < mn + 1e-5, reproduced in f32 (one IEEE add and a compare)
    v32 = R.view(N, 21, npix).clamp_min(0)
    mx32, mn32 = v32.max(2, keepdim=True).values, v32.min(2, keepdim=True).values
    zero_k = v32 < (mn32 + torch.tensor(1e-5, dtype=torch.float32))
    v64, mx, mn = v32.double(), mx32.double(), mn32.double()
    zero_64 = v64 < mn + 1e-5
    diff = zero_k != zero_64                                              # a differing decision is a near-tie of the threshold
    assert bool(((v64 - mn - 1e-5).abs()[diff] <= SAFETY * 2 * U32 * (mn + 1e-5).expand_as(v64)[diff]).all())
    D = mx - mn + 1e-5
    ref = (torch.where(zero_k, torch.zeros((), dtype=torch.float64), v64) - mn - 1e-5) / D
    ref[:, 0] = bg
    # numerator 2 roundings of magnitude |v| + mn + 1e-5, denominator 2 of mx + mn + 1e-5, the division 1; f32(bg) 1
    bar = SAFETY * (2 * U32 * (v64 + mn + 1e-5) / D + ref.abs() * (2 * U32 * (mx + mn + 1e-5) / D + 2 * U32))
    assert bool(((nk.double() - ref).abs() <= bar).all()), float((nk.double() - ref).abs().max())
    # the oracle's ncam (float64) agrees wherever the zeroing decisions agree
    _, _, cam_o = pseudo_labels_and_prototypes(R.double(), torch.randn(N, 128, 16, 16, generator=g).double(), torch.cat([torch.ones(N, 1), label20], 1).double().view(N, 21, 1, 1), bg)
    cam_o = cam_o.view(N, 21, npix)
    same = ~diff
    assert bool(((nk.double() - cam_o).abs()[same] <= bar[same]).all())
    # labels: the first arg-max of the kernel's own scores, exactly; a differing float64 label is a near-tie
    lab = torch.cat([torch.ones(N, 1), label20], 1)
    sk = (nk * lab[:, :, None]).numpy()
    assert torch.equal(yk.view(N, npix), torch.from_numpy(np.argmax(sk, axis=1)).long())
    s64 = cam_o * lab.double()[:, :, None]
    at = torch.gather(s64, 1, yk.view(N, 1, npix)).squeeze(1)
    assert bool((at >= s64.max(1).values - 2 * bar.max()).all())


# ------------------------------------------------------------------------------------------------ prototypes
def _proto_inputs(n, npix, seed):
    g = _gen(seed)
    ncam = (torch.rand(n, 21, npix, generator=g) * 64).round() / 64       # many exact ties
    ncam[:, 0] = 0.2; ncam[:, 7] = -1.0                                   # constant rows: the tie table
    feat = torch.randn(n * npix, 128, generator=g)
    feat[:, 0] = torch.arange(n * npix).float()                           # column 0 names the pixel (exact below 2^24)
    return ncam, feat


def _candidates(ncam, feat, K, tie):
    L = _L()
    N, _, npix = ncam.shape
    cv, cf = torch.empty(21, K, device=DEV), torch.empty(21, K, 128, device=DEV)
    cc = torch.empty(21, device=DEV, dtype=torch.int32)
    L.proto_candidates(ncam.contiguous().to(DEV), feat.contiguous().to(DEV), tie.to(DEV), cv, cf, cc, N, npix, K)
    return cv, cf, cc


@pytest.mark.parametrize("n", [1, 16, 128])
def test_proto_candidates_and_merge(n):
    """n = 128: P = 32768, the wrapper's LDS limit (P * 4 = 128 KiB of values in one workgroup); one more image is refused."""
    from wseg_amd.loss_hip import cpu_tie_pattern
    L = _L()
    npix, K = 256, 32
    P = n * npix
    ncam, feat = _proto_inputs(n, npix, 70 + n)
    tie = cpu_tie_pattern(P, K)
    cv, cf, cc = _candidates(ncam, feat, K, tie)
    rows = ncam.transpose(0, 1).reshape(21, -1)
    const = rows.max(1).values == rows.min(1).values
    idx = torch.argsort(rows, dim=1, descending=True, stable=True)[:, :K]  # a top-K with the lowest-index tie rule
    idx[const] = tie.long()
    assert torch.equal(cc.cpu().bool(), const)
    assert torch.equal(cf.cpu()[:, :, 0].long(), idx)                    # the kernel's set, exactly
    assert torch.equal(cv.cpu(), torch.gather(rows, 1, idx))
    assert torch.equal(cf.cpu(), feat[idx])
    protos = torch.empty(21, 128, device=DEV)
    L.proto_merge(cv, cf, cc, protos, 1, K)
    ref = _protos64(cv.cpu(), cf.cpu())
    bar = _proto_bar(cv.cpu(), cf.cpu(), K)
    assert bool(((protos.cpu().double() - ref).abs() <= bar).all())
    # the oracle's prototypes (restated in float64) where its K-th / (K+1)-th margin decides the set
    srt = torch.sort(rows.double(), dim=1, descending=True).values
    clear = (srt[:, K - 1] > srt[:, K]) & ~const
    tv, ti = torch.topk(rows.double(), K, dim=-1)
    oref = F.normalize(torch.stack([(tv[i, :, None] * feat.double()[ti[i]]).sum(0) / tv[i].sum() for i in range(21)]), dim=-1)
    assert bool(((protos.cpu().double() - oref).abs() <= bar)[clear].all())
    if n == 128:
        with pytest.raises(RuntimeError):
            nc2, ft2 = _proto_inputs(n + 1, npix, 1)
            _candidates(nc2, ft2, K, cpu_tie_pattern(P + npix, K))


@pytest.mark.parametrize("n", [1, 16])
def test_proto_non_finite_values(n):
    """A diverged step: an all-NaN class plane (class 3) and one NaN value among finite ones (class 4) in the candidates'
    input, and one NaN candidate value (class 5) in the merge.  NaN ranks as -inf; no index leaves the row.  The classes
    that hold a selected NaN get a NaN prototype, every other prototype is bit-equal to the finite run."""
    from wseg_amd.loss_hip import cpu_tie_pattern
    L = _L()
    npix, K = 256, 32
    P = n * npix
    ncam, feat = _proto_inputs(n, npix, 90 + n)
    tie = cpu_tie_pattern(P, K)
    cv0, cf0, cc0 = _candidates(ncam, feat, K, tie)
    p0 = torch.empty(21, 128, device=DEV)
    L.proto_merge(cv0, cf0, cc0, p0, 1, K)
    bad = ncam.clone()
    bad[:, 3] = float("nan")
    bad[0, 4, 0] = float("nan")
    cv, cf, cc = _candidates(bad, feat, K, tie)
    cv[5, 7] = float("nan")
    protos = torch.empty(21, 128, device=DEV)
    L.proto_merge(cv, cf, cc, protos, 1, K)
    torch.cuda.synchronize()
    pc = protos.cpu()
    # class 3: every value ranks -inf == constant row -> the tie table, NaN values, NaN prototype
    assert bool(cc.cpu()[3]) and torch.equal(cf.cpu()[3, :, 0].long(), tie.long())
    assert bool(torch.isnan(cv.cpu()[3]).all()) and bool(torch.isnan(pc[3]).all())
    # class 4: the NaN pixel ranks last: the set is the top-K of the finite values (lowest index first)
    row4 = bad[:, 4].reshape(-1).clone()
    row4[torch.isnan(row4)] = float("-inf")
    idx4 = torch.argsort(row4, descending=True, stable=True)[:K]
    assert torch.equal(cf.cpu()[4, :, 0].long(), idx4)
    # class 5: a NaN candidate at world 1 is always merged: NaN prototype
    assert bool(torch.isnan(pc[5]).all())
    others = [c for c in range(21) if c not in (3, 4, 5)]
    assert torch.equal(pc[others], p0.cpu()[others])
    assert bool(torch.isfinite(pc[4]).all())


# ------------------------------------------------------------------------------------------------ pixel-to-prototype contrast (nce.hip)
@pytest.fixture(scope="module", params=[77, 1000, 4096, 300007])
def nce_case(request):
    """Inputs of both views (the generators of the retired fused-vs-unfused test) and their float64 reference, built once per P.
    P = 77: one partial 64-pixel group, partial 16-pixel tiles; 1000: tails in both group sizes; 4096: full groups; 300007: every
    record-pass wave walks 4-5 tiles (the two-tiles-in-flight pipeline in steady state, odd and even trip counts)."""
    P = request.param
    g = _gen(P)
    V = []
    for _ in range(2):
        Fv = torch.randn(P, 128, generator=g)
        Fv[5] = 0.0                                          # a dead pixel: zero feature row (the F.normalize eps path)
        V.append(dict(F=Fv, p=F.normalize(torch.randn(21, 128, generator=g), dim=1),
                      y=torch.randint(0, 21, (P,), generator=g, dtype=torch.int32),
                      w=(torch.rand(P, generator=g) < 0.4).float() * torch.rand(P, generator=g) / P,
                      rkey=torch.rand(P, generator=g)))
    cc = 0.1 / (2 * P)
    with_grad = P <= 8192                                    # (P = 300007 compares records and loss sums only)
    dec = _nce_reference(V, cc, NCE_CI, False)
    for v, d in zip(V, dec):
        v["w"] = torch.where(d["undecided"], torch.zeros(()), v["w"])       # the intra term covers the decided pixels only
    ref = _nce_reference(V, cc, NCE_CI, True) if with_grad else dec
    return dict(P=P, V=V, cc=cc, ref=ref, with_grad=with_grad)


def _dev_views(V):
    return [{k: t.to(DEV) for k, t in v.items()} for v in V]


def test_nce_records(nce_case):
    """rec[3][P] = {label bits, similarity to the pixel's own class, random key}: labels and keys exact, the similarity within S_BAR of
    float64; the split-bf16 form (operands x = hi + lo to 16-17 bits) within 3e-6 of the exact record, the bar it has always been held
    to; without keys the same labels and similarities, bit for bit."""
    L = _L()
    P, V, ref = nce_case["P"], nce_case["V"], nce_case["ref"]
    D = _dev_views(V)
    rec = [torch.full((3, P), float("nan"), device=DEV) for _ in D]
    L.nce_records([dict(F=d["F"], p_own=d["p"], y_own=d["y"], rkey=d["rkey"], rec=r) for d, r in zip(D, rec)], P)
    rec3 = [torch.full((3, P), float("nan"), device=DEV) for _ in D]
    L.nce_records([dict(F=d["F"], p_own=d["p"], y_own=d["y"], rkey=d["rkey"], rec=r) for d, r in zip(D, rec3)], P, split_bf16=True)
    rec0 = [torch.full((3, P), float("nan"), device=DEV) for _ in D]
    L.nce_records([dict(F=d["F"], p_own=d["p"], y_own=d["y"], rec=r) for d, r in zip(D, rec0)], P)
    for i, (v, r) in enumerate(zip(V, ref)):
        rc, r3, r0 = rec[i].cpu(), rec3[i].cpu(), rec0[i].cpu()
        assert torch.equal(rc[0].view(torch.int32), v["y"]) and torch.equal(rc[2], v["rkey"])
        s64 = r["So"].gather(1, r["yo"])[:, 0]
        err = (rc[1].double() - s64).abs()
        assert float(err.max()) <= S_BAR, f"view {i}: max |dS| {float(err.max()):.3e} (bar {S_BAR:.3e})"
        assert float(rc[1, 5]) == 0.0                                            # the dead pixel: exactly 0
        assert torch.equal(r3[0].view(torch.int32), v["y"]) and torch.equal(r3[2], v["rkey"])
        assert float((r3[1] - rc[1]).abs().max()) <= 3e-6
        assert torch.equal(r0[:2].view(torch.int32), rc[:2].view(torch.int32)) and bool(torch.isnan(r0[2]).all())
    if P > 8192:
        return                                               # (the single-rank sampler sorts one view in LDS: P <= 8192)
    # the records feed the sort-based sampler through a leading dimension of 1 exactly as a [P,21] table does through 21
    table = torch.zeros(P, 21, device=DEV)
    table[torch.arange(P, device=DEV), D[0]["y"].long()] = rec[0][1]
    w21, w1 = torch.empty(P, device=DEV), torch.empty(P, device=DEV)
    L.intra_weights(D[0]["y"], table, D[0]["rkey"], None, w21, P)
    L.intra_weights(D[0]["y"], rec[0][1], D[0]["rkey"], None, w1, P, ld_s=1)
    assert torch.equal(w21, w1) and float(w1.sum()) > 0


def test_nce_fused(nce_case):
    """The three loss sums and dF of both views against float64.  The rank band 3..12 is a decision: a pixel whose float64 gap at rank
    2/3 or 12/13 is below 2 S_BAR carries no intra weight and is left out of the dF comparison (at most 2 % per view); the cross terms
    do not depend on the band and cover every pixel."""
    L = _L()
    P, V, ref, cc = nce_case["P"], nce_case["V"], nce_case["ref"], nce_case["cc"]
    share = [float(r["undecided"].double().mean()) for r in ref]
    assert max(share) <= NCE_MAX_EXCLUDED, f"P={P}: excluded share per view {share[0]:.4%}, {share[1]:.4%}"
    D = _dev_views(V)
    dF = [torch.full((P, 128), float("nan"), device=DEV) for _ in D]
    sums = torch.zeros(3, device=DEV)
    L.nce_fused([dict(F=d["F"], p_own=d["p"], p_oth=o["p"], y_own=d["y"], y_oth=o["y"], w_intra=d["w"], dF=g)
                 for d, o, g in ((D[0], D[1], dF[0]), (D[1], D[0], dF[1]))], P, cc, NCE_CI, sums)
    got = sums.cpu().double()
    for k in range(3):
        wts = [torch.full((P,), cc, dtype=torch.float64) if k < 2 else NCE_CI * v["w"].double() for v in V]
        want = sum(float((w * r["L"][k]).sum()) for w, r in zip(wts, ref))
        bar = _nce_sum_bar(torch.cat([r["L"][k] for r in ref]), torch.cat(wts), P)
        assert want > 0 and float(got[k]) != 0.0
        assert abs(float(got[k]) - want) <= bar, f"P={P} sum {k}: {float(got[k]):.9g} vs {want:.9g}, bar {bar:.3e} (excluded {share[0]:.4%}, {share[1]:.4%})"
    for i, r in enumerate(ref):
        g = dF[i].cpu()
        assert bool(torch.isfinite(g).all())
        assert bool((g[5] == 0).all())                                           # the dead pixel: inv = 0, the gradient is exactly 0
        if not nce_case["with_grad"]:
            continue
        keep = ~r["undecided"]
        err = (g.double() - r["dF"]).abs()[keep]
        over = err - r["dF_bar"][keep]
        assert float(over.max()) <= 0, (f"P={P} view {i}: max err {float(err.max()):.3e}, worst excess {float(over.max()):.3e} over a bar of "
                                        f"{float(r['dF_bar'][keep].view(-1)[over.argmax()]):.3e} (excluded {share[i]:.4%})")


# ------------------------------------------------------------------------------------------------ hard-pixel sampling
def sampling_inputs(ranks):
    """Labels, a [PG,21] similarity table and random keys of a gathered batch: an absent class, a single-pixel class, tied similarities
    and tied keys (the order falls back to the pixel index).  P = 1024 per rank at 8 ranks: the sort-based kernel holds 8192 pixels."""
    P = 1536 if ranks < 8 else 1024
    g = _gen(11 + ranks)
    PG = P * ranks
    y = torch.randint(0, 21, (PG,), generator=g, dtype=torch.int32)
    y[y == 7] = 3                                   # an absent class
    y[5] = 19; y[y == 19] = 2; y[5] = 19            # a class with a single pixel (skipped, still counted)
    S = (torch.rand(PG, 21, generator=g) * 2 - 1)
    S[10:40, :] = S[9, :]                           # tied similarities: order falls back to the pixel index
    y[10:40] = y[9]
    rk = torch.rand(PG, generator=g)
    rk[100:120] = rk[99]
    return P, y, S, rk


def test_intra_weights_against_the_sampling_rule():
    """contrast_train.py:302-331 restated on integers: per class with len >= 2 the random half (the len // 2 smallest keys) and the
    similarity rank band [int(0.6 len) - len // 2, int(0.6 len)), ties ordered by pixel index; weight = selections / (2 (len // 2) C),
    C = classes present.  An integer rule on f32 keys: exact up to the kernel's one f32 division (rtol 1e-6)."""
    L = _L()
    P, y, S, rk = sampling_inputs(1)
    w = torch.empty(P, device=DEV)
    L.intra_weights(y.to(DEV), S.to(DEV), rk.to(DEV), None, w, P)
    yn, rkn = y.numpy(), rk.numpy()
    sim = S.numpy()[np.arange(P), yn]
    present = np.unique(yn)
    assert 7 not in present and int((yn == 19).sum()) == 1
    ref = sampling_rule(yn, sim, rkn=rkn)
    got = w.cpu().double().numpy()
    assert ref.sum() > 0 and (got[ref == 0] == 0).all()
    np.testing.assert_allclose(got, ref, rtol=1e-6, atol=0)
