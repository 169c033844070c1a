"""GPU: the PCM (csrc/pcm.hip), CAM-head (csrc/head.hip) and SGD (csrc/optim.hip) kernels and a few one-pass utilities
(csrc/api.hip, csrc/loss.hip) one entry point at a time against float64 CPU references of the same operation.

How the bars are set (the rules of test_gpu_loss_kernels.py): every tolerance is derived from the kernel's arithmetic, never
fitted to a run.
  u = 2^-24, the unit roundoff of f32.  A sum accumulated in a serial chain of length c has error <= c * u * sum|terms|;
  every bar states its chain and carries the safety factor of 2 (SAFETY).  The f32 MFMA chain over the 192 channels counts as
  a chain of 192 whatever order the hardware uses, the i-loop over the hw rows as a chain of hw.
bf16 results are compared with float64 computed from the same bf16-rounded inputs, so only the kernel's internal roundings
enter: 2^-9 relative for each value the kernel rounds to bf16 (relu(S), W; with SAFETY this is the half-ulp bound 2^-8),
3 * 2^-17 * sum_c |P_ic| |Q_jc| for the split-precision gate product, and the f32 chains.
Decisions are not arithmetic: the arithmetic is compared under the kernel's own decision where the kernel returns it
(cam_gate's kept entries, infer_finish's zeroing and labels), and a decision that differs from the float64 one must be a
near-tie of the float64 values within the derived bar.  The PCM backward does not return its gate S > 0: every element's bar
gets a flip term, sum over the rows i whose float64 |S_ij| <= sbar_ij of |t_ij| |Fh_ik| (both launches), and the share of
pairs inside that band is capped at 0.1 % so that the term cannot hide a failure.  Exact ties are built from values on which
f32 and float64 agree bit for bit, and the stated tie rule is asserted exactly.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from .f64_bars import SAFETY, U32, _gen, _interp_bar
# the float64 references and bars of the PCM kernels, shared with the stage tests of the head passes (KF = 192 feature channels; BAND_CAP,
# the largest share of (i, j) pairs whose gate may be undecided at sbar; BF16_RND per value the bf16 kernels round, SPLIT_T the
# split-precision gate product: see the module docstring)
from .head_f64 import BAND_CAP, BF16_RND, KF, SPLIT_T, _pcm_bwd_reference, _pcm_fwd64, _pcm_fwd_bars, _ulp_bf16

pytestmark = pytest.mark.gpu

DEV = "cuda"
GUARD = 64                  # sentinel elements behind an output buffer
SENT = 7.0


def _L():
    from wseg_amd import _lib as L
    return L


def _guarded(numel, fill, dtype=torch.float32):
    """a flat device buffer of numel elements filled with `fill`, with GUARD sentinels behind it; returns (whole, view)"""
    whole = torch.full((numel + GUARD,), fill, dtype=dtype)
    whole[numel:] = SENT
    whole = whole.to(DEV)
    return whole, whole[:numel]


def _guard_ok(whole):
    return bool((whole[-GUARD:].cpu().float() == SENT).all())


def _i16(t):
    return t.contiguous().cpu().view(torch.int16)


def _i32(t):
    return t.contiguous().cpu().view(torch.int32)


# ------------------------------------------------------------------------------------------------ l2norm (pcm.hip)
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("ldf,lddf", [(192, 192), (256, 200)])
@pytest.mark.parametrize("rows", [1, 5, 317])
def test_l2norm_forward_and_backward(rows, ldf, lddf, dtype):
    """Fh = F / (|F| + 1e-5) and its backward against float64 autograd; rows scaled by 1e-6, 1 and 1e3 in turn, one all-zero
    row (rows > 1), rows % 4 != 0, padded leading dimensions whose columns >= 192 must stay untouched."""
    L = _L()
    g = _gen(rows * 7 + ldf + (dtype == torch.bfloat16))
    Fm = torch.randn(rows, ldf, generator=g) * torch.tensor([1e-6, 1.0, 1e3])[torch.arange(rows) % 3][:, None]
    zrow = rows // 2 if rows > 1 else None
    if zrow is not None:
        Fm[zrow] = 0.0
    Fm = Fm.to(dtype)
    dFh = torch.randn(rows, KF, generator=g)
    Fh_w, Fh = _guarded(rows * KF, float("nan"))
    nrm_w, nrm = _guarded(rows, float("nan"))
    L.l2norm_forward(Fm.to(DEV), ldf, Fh, nrm, rows)
    dF = torch.full((rows, lddf), SENT, dtype=dtype, device=DEV)
    L.l2norm_backward(Fm.to(DEV), ldf, dFh.to(DEV), nrm, dF, lddf, rows)
    assert _guard_ok(Fh_w) and _guard_ok(nrm_w)

    x = Fm.double()[:, :KF].clone().requires_grad_(True)
    nr = x.norm(dim=1, keepdim=True)
    y = x / (nr + 1e-5)
    (y * dFh.double()).sum().backward()
    ref_g, nr, y = x.grad, nr.detach(), y.detach()
    assert bool(torch.isfinite(ref_g).all())
    # |F|: 3 products (1 u each) and 2 adds per lane, 6 shuffle levels: a chain of 9 + 1 on a sum of squares = 10 u, halved by the
    # square root, + 1 u of the root itself: 6 u
    got_n = nrm.cpu().double()[:, None]
    assert bool(((got_n - nr).abs() <= SAFETY * 6 * U32 * nr).all()), float(((got_n - nr).abs() / nr.clamp_min(1e-30)).max())
    # r = 1 / (|F| + f32(1e-5)): 6 u, the add, the constant and the division 1 u each = 9 u; Fh = F * r: 1 u more
    got = Fh.cpu().double().view(rows, KF)
    assert bool(((got - y).abs() <= SAFETY * 10 * U32 * y.abs()).all()), float((got - y).abs().max())
    # dF = d * r - F * k, k = dot * r * r / |F| (0 on a zero row): d * r carries r's 9 u + 1 u; dot is a chain of 9 + 1 on A = sum|F d|;
    # k adds two r (18 u), |F| (6 u) and 3 roundings, F * k 1 u: 10 u A + 28 u |dot| <= 38 u A; the subtraction 1 u of each side
    v, d = x.detach(), dFh.double()
    r = 1.0 / (nr + 1e-5)
    A = (v * d).abs().sum(1, keepdim=True)
    bar = SAFETY * U32 * (12 * d.abs() * r + 40 * v.abs() * A * r * r / nr.clamp_min(1e-300))
    gd = dF.cpu().double()
    if dtype == torch.bfloat16:                               # stored in bf16: one bf16 ulp of the float64 value
        bar = bar + _ulp_bf16(ref_g)
    err = (gd[:, :KF] - ref_g).abs()
    assert bool((err <= bar).all()), f"max err {float(err.max()):.3e}, worst excess {float((err - bar).max()):.3e}"
    assert bool((gd[:, KF:] == SENT).all())
    if zrow is not None:
        assert bool((got[zrow] == 0).all()) and float(got_n[zrow]) == 0.0
        # dF = dFh / 1e-5: the f32 constant, the division and the product, 1 u each
        zb = SAFETY * 3 * U32 * (d[zrow] / 1e-5).abs() + (_ulp_bf16(d[zrow] / 1e-5) if dtype == torch.bfloat16 else 0.0)
        assert bool(((gd[zrow, :KF] - d[zrow] / 1e-5).abs() <= zb).all())


# ------------------------------------------------------------------------------------------------ PCM (pcm.hip)
PCM_HW = [1, 15, 33, 64, 65, 117, 256]
# hw = 1, 15: one partly filled wave tile (clamped columns); 33: a second row tile with one live row; 65: a second workgroup with
# one live column; 64 / 256: full tiles; 117: the 13 x 9 map of the whole-net tests


def _gate_like(n_rows, g):
    """G built like cam_gate's output: non-negative, one kept foreground class per pixel (the rest exact zeros, sometimes all of
    them), column 0 = 1 - fgmax, column 21 = 1, columns 22..31 = 0."""
    v = torch.rand(n_rows, 20, generator=g)
    v[torch.rand(n_rows, 20, generator=g) < 0.3] = 0.0
    v[::11] = 0.0                                             # pixels without any foreground: bg = 1
    mx = v.max(1, keepdim=True).values
    G = torch.zeros(n_rows, 32)
    G[:, 1:21] = torch.where(v == mx, v, torch.zeros(()))
    G[:, 0] = 1.0 - mx[:, 0]
    G[:, 21] = 1.0
    return G


def _pcm_inputs(N, hw, seed, exact=False):
    g = _gen(seed)
    if exact:                                                 # S is a multiple of 1/256: exact in f32 and in float64
        Fh = torch.randint(-1, 2, (N * hw, KF), generator=g).float() / 16
    else:                                                     # unit rows, S ~ N(0, 1/192): about half of the gates are open
        Fm = torch.randn(N * hw, KF, generator=g).double()
        Fh = (Fm / (Fm.norm(dim=1, keepdim=True) + 1e-5)).float()
    return Fh, _gate_like(N * hw, g), torch.randn(N, 21, hw, generator=g)


def _assert_balanced(S_list, hw):
    if hw == 1:                                               # the single pair is the diagonal, S = |Fh|^2 = 1
        return
    pos = float(torch.cat([(s > 0).double().view(-1) for s in S_list]).mean())
    assert 0.25 <= pos <= 0.75, pos


def _run_pcm_forward(fn, Fd, Gd, N, hw):
    rv_w, rv = _guarded(N * 21 * hw, float("nan"))
    den_w, den = _guarded(N * hw, float("nan"))
    fn(Fd, Gd, rv, den, N, hw)
    assert _guard_ok(rv_w) and _guard_ok(den_w)
    return rv.cpu().view(N, 21, hw), den.cpu().view(N, hw)


def _check_pcm_forward(rv_k, den_k, Fh64, G64, N, hw, relu_rel=0.0):
    S_all = []
    for n in range(N):
        sl = slice(n * hw, (n + 1) * hw)
        rv, den, S, _, bar_rv, bar_den = _pcm_fwd_bars(Fh64[sl], G64[sl], hw, relu_rel)
        S_all.append(S)
        e_rv, e_den = (rv_k[n].double() - rv).abs(), (den_k[n].double() - den).abs()
        assert bool((e_rv <= bar_rv).all()), f"n={n} cam_rv: max err {float(e_rv.max()):.3e}, worst excess {float((e_rv - bar_rv).max()):.3e}"
        assert bool((e_den <= bar_den).all()), f"n={n} den: max err {float(e_den.max()):.3e}, worst excess {float((e_den - bar_den).max()):.3e}"
    return S_all


@pytest.mark.parametrize("hw", PCM_HW)
def test_pcm_forward(hw):
    """cam_rv = relu(S)^T G / (colsum + 1e-5) and den = colsum against float64, NaN-filled outputs with guards behind them, and
    image 1 of the N = 2 launch bit-equal to a launch on that image alone."""
    L = _L()
    N = 2
    Fh, G, _ = _pcm_inputs(N, hw, 100 + hw)
    Fd, Gd = Fh.to(DEV), G.to(DEV)
    rv_k, den_k = _run_pcm_forward(L.pcm_forward, Fd, Gd, N, hw)
    S_all = _check_pcm_forward(rv_k, den_k, Fh.double(), G.double(), N, hw)
    _assert_balanced(S_all, hw)
    rv1, den1 = _run_pcm_forward(L.pcm_forward, Fd[hw:], Gd[hw:], 1, hw)
    assert torch.equal(_i32(rv1[0]), _i32(rv_k[1])) and torch.equal(_i32(den1[0]), _i32(den_k[1]))


@pytest.mark.parametrize("hw", [1, 15])
def test_pcm_forward_small_denominator(hw):
    """Unit rows scaled by 2^-8 (the kernel takes Fh as given): S_jj = 2^-16 = 1.5e-5, so the 1e-5 of the denominator is as large as
    the column sum itself and cam_rv is wrong by a factor without it; the bars are the forward's own."""
    L = _L()
    N = 2
    Fh, G, _ = _pcm_inputs(N, hw, 200 + hw)
    Fh = Fh * 2.0 ** -8
    rv_k, den_k = _run_pcm_forward(L.pcm_forward, Fh.to(DEV), G.to(DEV), N, hw)
    _check_pcm_forward(rv_k, den_k, Fh.double(), G.double(), N, hw)
    assert float(den_k.max()) < 1e-4


def _pcm_bwd_case(hw, seed, exact, with_base):
    L = _L()
    N = 2
    Fh, G, d_rv = _pcm_inputs(N, hw, seed, exact)
    F64, G64 = Fh.double(), G.double()
    fwd = [_pcm_fwd64(F64[n * hw:(n + 1) * hw], G64[n * hw:(n + 1) * hw]) for n in range(N)]
    rv_in = torch.stack([f[0] for f in fwd]).float()
    den_in = torch.stack([f[1] for f in fwd]).float()
    base = torch.randn(N * hw, KF, generator=_gen(seed + 1)) if with_base else torch.zeros(N * hw, KF)
    DN_w, DN = _guarded(N * hw * 32, float("nan"))
    d_w, dFh = _guarded(N * hw * KF, 0.0)
    dFh.copy_(base.view(-1))
    L.pcm_backward(Fh.to(DEV), G.to(DEV), d_rv.to(DEV), rv_in.to(DEV), den_in.to(DEV), DN, dFh, N, hw)
    assert _guard_ok(DN_w) and _guard_ok(d_w)
    got = dFh.cpu().double().view(N * hw, KF) - base.double()
    DN_k = DN.cpu().double().view(N * hw, 32)
    in_band = 0
    for n in range(N):
        sl = slice(n * hw, (n + 1) * hw)
        ref, bar, DN64, bar_dn, nb = _pcm_bwd_reference(F64[sl], G64[sl], d_rv[n].double(), rv_in[n].double(), den_in[n].double(), hw,
                                                        base[sl].double(), t_chain=32, with_band=not exact)
        in_band += nb
        e_dn = (DN_k[sl] - DN64).abs()
        assert bool((e_dn <= bar_dn).all()), f"n={n} DN: max err {float(e_dn.max()):.3e}"
        assert bool((DN_k[sl][:, 22:] == 0).all())
        err = (got[sl] - ref).abs()
        assert bool((err <= bar).all()), (f"n={n} dFh: max err {float(err.max()):.3e} (|ref| max {float(ref.abs().max()):.3e}), worst excess "
                                         f"{float((err - bar).max()):.3e}, pairs in the gate band {nb}")
    return fwd, in_band / (N * hw * hw)


@pytest.mark.parametrize("with_base", [False, True])
@pytest.mark.parametrize("hw", PCM_HW)
def test_pcm_backward(hw, with_base):
    """dFh (+= onto a zeroed and onto a random buffer) and the DN scratch against float64 autograd of the forward.  Share of
    pairs inside the gate band with these inputs, measured on the CPU: none at hw = 1, 15 and 33; 0.024 % at hw = 64 and 65 (one
    pair, counted as (i, j) and (j, i), in each image); 0.007 % at hw = 117 and 0.008 % at hw = 256 (the cap is 0.1 %)."""
    fwd, share = _pcm_bwd_case(hw, 100 + hw, False, with_base)
    _assert_balanced([f[2] for f in fwd], hw)
    assert share <= BAND_CAP, share


def test_pcm_backward_exact_gates():
    """Fh entries from {-1, 0, 1} / 16 at hw = 117: every S is a multiple of 1 / 256, exact in f32 and in float64, so the band is
    empty by construction and the flip term is zero.  About 4 % of the pairs have S == 0 exactly: the reference (autograd of
    relu) closes the gate there, and so must the kernel (`S > 0`, not `>=`)."""
    fwd, _ = _pcm_bwd_case(117, 7, True, False)
    S = torch.stack([f[2] for f in fwd])
    assert torch.equal(S, (S * 256).round() / 256)
    zeros, pos = float((S == 0).double().mean()), float((S > 0).double().mean())
    assert zeros > 0.02 and 0.25 <= pos <= 0.75, (zeros, pos)


# ------------------------------------------------------------------------------------------------ bf16 conversions and the bf16 PCM
def _bf16_values(total, g):
    x = torch.randn(total, generator=g) * torch.tensor([1e-3, 1.0, 300.0])[torch.arange(total) % 3]
    sp = torch.tensor([0.0, -0.0, float("inf"), float("-inf"), 1.00390625, 1.01171875, -1.00390625, 3.0e38, 2.0 ** -126],
                      dtype=torch.float32)                    # 1 + 2^-8 and 1 + 3 * 2^-8: round-to-nearest-even ties (down / up)
    x[:min(total, sp.numel())] = sp[:total]
    if total > 64:                                            # more exact ties: the 17th bit set alone below a random bf16
        t = x[32:64].bfloat16().float().view(torch.int32) | 0x8000
        x[32:64] = t.view(torch.float32)
    return x


@pytest.mark.parametrize("total", [4096, 4097, 4098, 4099, 1, 3])
def test_to_bf16_and_split_bf16(total):
    """total % 4 in {0, 1, 2, 3}: the scalar tail of to_bf16.  hi and lo bit-equal to the torch roundings."""
    L = _L()
    x = _bf16_values(total, _gen(total))
    out_w, out = _guarded(total, 1.0, torch.bfloat16)
    L.to_bf16(x.to(DEV), out)
    assert _guard_ok(out_w)
    assert torch.equal(_i16(out), _i16(x.bfloat16()))
    hi_w, hi = _guarded(total, 1.0, torch.bfloat16)
    lo_w, lo = _guarded(total, 1.0, torch.bfloat16)
    L.split_bf16(x.to(DEV), hi, lo)
    assert _guard_ok(hi_w) and _guard_ok(lo_w)
    hi_ref = x.bfloat16()
    fin = torch.isfinite(hi_ref.float())                      # (x - hi is NaN at +-inf and where 3e38 rounds to inf)
    assert torch.equal(_i16(hi), _i16(hi_ref))
    assert torch.equal(_i16(lo)[fin], _i16((x - hi_ref.float()).bfloat16())[fin])
    # hi is x to 8 bits; x - hi is exact in f32 and has at most 15 bits below 2^-9 |x| (or is 2^-8 2^e itself): lo's half ulp <= 2^-17 |x|
    xs, res = x[fin].double(), (x.double() - hi.cpu().double() - lo.cpu().double())[fin]
    normal = xs.abs() >= 2.0 ** -100                          # (lo of a value near the bottom of the f32 range is subnormal)
    assert bool((res.abs()[normal] <= 2.0 ** -17 * xs.abs()[normal]).all())


@pytest.mark.parametrize("hw", PCM_HW)
def test_pcm_bf16_forward_and_backward(hw):
    """The bf16-MFMA PCM against float64 from the same rounded operands: Fb = bf16(Fh) everywhere, Gb in the forward, Gb + Gl in
    the backward's gate product (DN is split by the entry point itself).  Products of bf16 values are exact in f32, so S keeps its
    chain of 192; relu(S) and W are rounded to bf16; t = Pl.Qh + Ph.Ql + Ph.Qh is three MFMAs (a chain of 96) and drops Pl.Ql.
    Image 1 of the N = 2 forward launch is bit-equal to a launch on that image alone.
    Share of pairs inside the gate band with these inputs (Fb = bf16(Fh), seeds 300 + hw), measured on the CPU: none at hw = 1, 15,
    33, 64 and 65; 0.0073 % at hw = 117 and 0.0168 % at hw = 256 (the cap is 0.1 %).  Open gates: all at hw = 1 (the diagonal),
    0.47-0.51 of the pairs at every other size."""
    L = _L()
    N = 2
    Fh, G, d_rv = _pcm_inputs(N, hw, 300 + hw)
    Fd, Gd = Fh.to(DEV), G.to(DEV)
    Fb = torch.empty(N * hw, KF, device=DEV, dtype=torch.bfloat16)
    Gb, Gl = (torch.empty(N * hw, 32, device=DEV, dtype=torch.bfloat16) for _ in range(2))
    L.to_bf16(Fd, Fb)
    L.split_bf16(Gd, Gb, Gl)
    assert torch.equal(_i16(Fb), _i16(Fh.bfloat16())) and torch.equal(_i16(Gb), _i16(G.bfloat16()))
    F64, Gb64 = Fb.cpu().double(), Gb.cpu().double()
    Gs64 = Gb64 + Gl.cpu().double()
    rv_k, den_k = _run_pcm_forward(L.pcm_forward_bf16, Fb, Gb, N, hw)
    S_all = _check_pcm_forward(rv_k, den_k, F64, Gb64, N, hw, relu_rel=BF16_RND)
    _assert_balanced(S_all, hw)
    rv1, den1 = _run_pcm_forward(L.pcm_forward_bf16, Fb[hw:], Gb[hw:], 1, hw)
    assert torch.equal(_i32(rv1[0]), _i32(rv_k[1])) and torch.equal(_i32(den1[0]), _i32(den_k[1]))

    fwd = [_pcm_fwd64(F64[n * hw:(n + 1) * hw], Gs64[n * hw:(n + 1) * hw]) for n in range(N)]
    rv_in = torch.stack([f[0] for f in fwd]).float()
    den_in = torch.stack([f[1] for f in fwd]).float()
    DN_w, DN = _guarded(N * hw * 32, float("nan"))
    DNb_w, DNb = _guarded(N * hw * 32, 1.0, torch.bfloat16)
    DNl_w, DNl = _guarded(N * hw * 32, 1.0, torch.bfloat16)
    d_w, dFh = _guarded(N * hw * KF, 0.0)
    L.pcm_backward_bf16(Fb, Gb, Gl, d_rv.to(DEV), rv_in.to(DEV), den_in.to(DEV), DN, DNb, DNl, dFh, N, hw)
    assert _guard_ok(DN_w) and _guard_ok(DNb_w) and _guard_ok(DNl_w) and _guard_ok(d_w)
    got = dFh.cpu().double().view(N * hw, KF)
    DN_k = DN.cpu().double().view(N * hw, 32)
    # the split of DN: hi + lo == DN to 2^-17 relative (see test_to_bf16_and_split_bf16), hi the plain rounding
    assert torch.equal(_i16(DNb), _i16(DN.cpu().bfloat16()))
    assert bool(((DN_k - DNb.cpu().double().view(-1, 32) - DNl.cpu().double().view(-1, 32)).abs() <= 2.0 ** -17 * DN_k.abs()).all())
    in_band = 0
    for n in range(N):
        sl = slice(n * hw, (n + 1) * hw)
        ref, bar, DN64, bar_dn, nb = _pcm_bwd_reference(F64[sl], Gs64[sl], d_rv[n].double(), rv_in[n].double(), den_in[n].double(), hw,
                                                        torch.zeros(hw, KF, dtype=torch.float64), t_chain=96, t_rel=SPLIT_T, w_rel=BF16_RND)
        in_band += nb
        assert bool(((DN_k[sl] - DN64).abs() <= bar_dn).all())
        err = (got[sl] - ref).abs()
        assert bool((err <= bar).all()), (f"n={n} dFh: max err {float(err.max()):.3e} (|ref| max {float(ref.abs().max()):.3e}), worst excess "
                                         f"{float((err - bar).max()):.3e}, pairs in the gate band {nb}")
    assert in_band / (N * hw * hw) <= BAND_CAP


# ------------------------------------------------------------------------------------------------ head_split / cam_gate (head.hip)
HEAD_CASES = [(5, 9), (3, 117), (2, 256), (1, 1)]
# (5, 9): every wave spans several images (the per-thread atomics); (3, 117): some waves straddle two images; (2, 256): every wave
# inside one image (the wave maximum and one atomic)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("N,hw", HEAD_CASES)
def test_head_split(N, hw, dtype):
    L = _L()
    ld, c0 = 192, 128
    g = _gen(N * 1000 + hw)
    head = torch.randn(N * hw, ld, generator=g)
    head[:hw, c0 + 3] = -(head[:hw, c0 + 3].abs() + 0.125)   # (image 0, class 3): all negative -> cmax exactly +0
    head[0, c0 + 3] = -0.0
    head[hw // 2, c0 + 7] = -0.0
    head = head.to(dtype)
    cam_w, cam = _guarded(N * 21 * hw, float("nan"))
    cmax_w, cmax = _guarded(N * 21, 1e30)                     # garbage on entry: the entry point clears it itself
    L.head_split(head.to(DEV), ld, c0, cam, cmax, N, hw)
    assert _guard_ok(cam_w) and _guard_ok(cmax_w)
    ref = head.float()[:, c0:c0 + 21].view(N, hw, 21).permute(0, 2, 1).contiguous()
    assert torch.equal(_i32(cam).view(N, 21, hw), _i32(ref))                # the upcast source, bit for bit (-0.0 included)
    ref_max = ref.clamp_min(0).amax(2) + 0.0
    assert torch.equal(_i32(cmax).view(N, 21), _i32(ref_max))
    assert int(_i32(cmax).view(N, 21)[0, 3]) == 0


def _gate_inputs(N, hw, g):
    cam = (torch.randn(N, 21, hw, generator=g) * 16).round() / 16
    cam[:, 3] = -(cam[:, 3].abs() + 0.25)                     # a class with cmax == 0: v = 0 everywhere
    cam[:, 1:, 0] = -cam[:, 1:, 0].abs()                      # pixel 0: every foreground value is 0 -> fgmax = 0, bg = 1
    if hw > 1:
        cam[:, 5, 1] = 6.0                                    # class 5 is the pixel's maximum at pixel 1 ...
    cam[:, 9] = cam[:, 5]                                     # ... and class 9 is the same plane: both are kept
    return cam


@pytest.mark.parametrize("N,hw", HEAD_CASES)
def test_cam_gate(N, hw):
    """resnet38_contrast.py:41-48 in float64, under the kernel's own keep / zero decisions: a kept foreground entry equals v within its
    bar and is a (near-)maximum; a zeroed one lies below another class's value, up to a near-tie."""
    L = _L()
    cam = _gate_inputs(N, hw, _gen(N * 77 + hw))
    cmax = cam.clamp_min(0).amax(2)
    G_w, G = _guarded(N * hw * 32, float("nan"))
    L.cam_gate(cam.to(DEV), cmax.to(DEV), G, N, hw)
    assert _guard_ok(G_w)
    out = G.cpu().view(N, hw, 32).permute(0, 2, 1)            # [N,32,hw]
    d = cam.double().clamp_min(0)
    m = (cmax.double() + 1e-5)[:, :, None]
    v = (d - 1e-5).clamp_min(0) / m
    # v: the subtraction 1 u and its f32 constant u * 1e-5 -> u (d + 2e-5) / m; the denominator's add and constant 2 u, the division 1 u
    bar = SAFETY * U32 * ((d + 2e-5) / m + 3 * v)
    fg, fbar = v[:, 1:], bar[:, 1:]
    pbar = fbar.max(1, keepdim=True).values                   # the pixel's bar: what the f32 maximum may be off by
    fgmax = fg.max(1, keepdim=True).values
    o = out[:, 1:21].double()
    kept = o != 0
    assert bool(((o - fg).abs()[kept] <= fbar[kept]).all())
    assert bool((fg[kept] >= (fgmax - 2 * pbar).expand_as(fg)[kept]).all())           # nothing but a (near-)maximum is kept
    top2 = torch.topk(fg, 2, dim=1).values
    others = torch.where(fg == fgmax, top2[:, 1:2].expand_as(fg), fgmax.expand_as(fg))  # the largest value of the other classes
    zeroed_ok = (fg <= fbar) | (fg < others) | (fg <= others + 2 * pbar)
    assert bool(zeroed_ok[~kept].all())                       # (a unique maximum that was zeroed fails here)
    # bg = 1 - fgmax: the maximum off by <= pbar, the subtraction 1 u
    assert bool(((out[:, 0:1].double() - (1 - fgmax)).abs() <= pbar + SAFETY * U32 * (1 - fgmax).abs()).all())
    assert bool((out[:, 21] == 1).all()) and bool((out[:, 22:] == 0).all())
    # the exact cases
    assert torch.equal(_i32(out[:, 5]), _i32(out[:, 9]))      # identical planes: identical f32 values, neither is below the other
    if hw > 1:
        assert bool((out[:, 5, 1] != 0).all()) and bool((out[:, 9, 1] != 0).all())
    assert bool((out[:, 3] == 0).all())                       # cmax == 0
    assert bool((out[:, 0, 0] == 1).all()) and bool((out[:, 1:21, 0] == 0).all())   # fgmax == 0: bg = 1, nothing to zero


# ------------------------------------------------------------------------------------------------ pcm_xs
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("c_end", [256, 200])
@pytest.mark.parametrize("H,W,h,w", [(104, 72, 13, 9), (64, 64, 8, 8), (9, 9, 9, 9), (40, 40, 1, 1)])
def test_pcm_xs(H, W, h, w, c_end, dtype):
    L = _L()
    N, ld, c_xs = 2, 256, 192
    x = torch.randn(N, 3, H, W, generator=_gen(H + w))
    feat = torch.full((N * h * w, ld), SENT, dtype=dtype, device=DEV)
    L.pcm_xs(x.to(DEV), feat, ld, c_xs, c_end, N, H, W, h, w)
    got = feat.cpu().double()
    ref = F.interpolate(x.double(), size=(h, w), mode="bilinear", align_corners=True).permute(0, 2, 3, 1).reshape(-1, 3)
    bar = torch.full_like(ref, _interp_bar(H, W, float(x.abs().max())))
    if dtype == torch.bfloat16:                               # stored in bf16: one bf16 ulp of the float64 value
        bar = bar + _ulp_bf16(ref)
    assert bool(((got[:, c_xs:c_xs + 3] - ref).abs() <= bar).all()), float((got[:, c_xs:c_xs + 3] - ref).abs().max())
    assert bool((got[:, :c_xs] == SENT).all()) and bool((got[:, c_end:] == SENT).all())
    assert bool((got[:, c_xs + 3:c_end] == 0).all())


# ------------------------------------------------------------------------------------------------ head_grad_rows
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("ld", [192, 152])
@pytest.mark.parametrize("hw", [9, 117])
def test_head_grad_rows(hw, ld, dtype):
    """An exact kernel: columns [0,128) the gradient masked by head > 0 (0.0 and -0.0 are masked), [128,149) a copy, the rest 0."""
    L = _L()
    N = 2
    g = _gen(hw + ld)
    head = torch.randn(N * hw, ld, generator=g)
    head[::3, :128:5] = 0.0
    head[1::3, 1:128:5] = -0.0
    head = head.to(dtype)
    d_fp = torch.randn(N, 128, hw, generator=g)
    d_cam = torch.randn(N, 21, hw, generator=g)
    mask = head.float()[:, :128] > 0
    assert 0.3 < float(mask.float().mean()) < 0.6 and int((head.float()[:, :128] == 0).sum()) > 0
    for use_fp, use_cam in ((True, True), (False, True), (True, False)):
        want = torch.zeros(N * hw, ld)
        if use_fp:
            want[:, :128] = torch.where(mask, d_fp.permute(0, 2, 1).reshape(-1, 128), torch.zeros(()))
        if use_cam:
            want[:, 128:149] = d_cam.permute(0, 2, 1).reshape(-1, 21)
        d_w, d_head = _guarded(N * hw * ld, SENT, dtype)
        L.head_grad_rows(d_fp.to(DEV) if use_fp else None, d_cam.to(DEV) if use_cam else None, head.to(DEV), d_head.view(N * hw, ld), ld, N, hw)
        assert _guard_ok(d_w)
        got = d_head.cpu().view(N * hw, ld)
        assert torch.equal(got.float(), want.to(dtype).float()), (use_fp, use_cam)
        assert bool((got[:, 149:] == 0).all())


# ------------------------------------------------------------------------------------------------ infer_finish
@pytest.mark.parametrize("npix", [1, 257, 94 * 125])
def test_infer_finish(npix):
    """Fed through plane_stats as wseg_amd/infer.py does.  norm_cam under the kernel's zeroing decision v < mn + 1e-5 (reproduced in
    f32: one IEEE add and a compare); pred = the first strict maximum against alpha of the kernel's own norm_cam.  A second run
    takes alpha from the first run's output, so that a class ties with alpha exactly."""
    L = _L()
    g = _gen(npix)
    x = (torch.randn(20, npix, generator=g) * 32).round() / 64
    x[1] = 0.5                                                # a constant plane
    x[2] = -(x[2].abs() + 0.25)                               # an all-negative plane
    x[4] = x[3]                                               # two identical classes: the first wins a tie
    x[6, 0] = 8.0                                             # class 7 owns pixel 0
    xd = x.to(DEV)
    stats = torch.empty(20, 6, device=DEV)
    L.plane_stats(xd, stats, 20, npix)

    def run(alpha):
        nc_w, nc = _guarded(20 * npix, float("nan"))
        pr_w, pr = _guarded(npix, 99, torch.uint8)
        L.infer_finish(xd, stats, alpha, nc, pr, npix)
        assert _guard_ok(nc_w) and _guard_ok(pr_w)
        return nc.cpu().view(20, npix), pr.cpu().long()

    nk, pk = run(0.3)
    st = stats.cpu()
    v32 = x.clamp_min(0)
    mx32, mn32 = st[:, 0:1], st[:, 1:2]
    assert torch.equal(mx32, v32.max(1, keepdim=True).values) and torch.equal(mn32, v32.min(1, keepdim=True).values)
    zero_k = v32 < (mn32 + torch.tensor(1e-5, dtype=torch.float32))
    v64, mx, mn = v32.double(), mx32.double(), mn32.double()
    diff = zero_k != (v64 < mn + 1e-5)                        # a differing decision is a near-tie of the threshold
    assert bool(((v64 - mn - 1e-5).abs()[diff] <= SAFETY * 2 * U32 * (mn + 1e-5).expand_as(v64)[diff]).all())
    D = mx - mn + 1e-5
    ref = (torch.where(zero_k, torch.zeros((), dtype=torch.float64), v64) - mn - 1e-5) / D
    # numerator: two subtractions and the f32 constant, 3 u of |v| + mn + 1e-5; denominator the same on mx + mn + 1e-5; the division 1 u
    bar = SAFETY * U32 * (3 * (v64 + mn + 1e-5) / D + ref.abs() * (3 * (mx + mn + 1e-5) / D + 1))
    assert bool(((nk.double() - ref).abs() <= bar).all()), float((nk.double() - ref).abs().max())

    def check_pred(nc, pred, alpha):
        a32 = torch.tensor(alpha, dtype=torch.float32)
        scores = torch.cat([a32.expand(1, npix), nc]).numpy()                       # np.argmax: the first maximum == strict `>` in order
        assert torch.equal(pred, torch.from_numpy(np.argmax(scores, axis=0)).long())
        s64 = torch.cat([a32.double().expand(1, npix), ref])
        at = torch.gather(s64, 0, pred[None])[0]
        assert bool((at >= s64.max(0).values - 2 * bar.max(0).values).all())        # a differing float64 label is a near-tie

    check_pred(nk, pk, 0.3)
    assert torch.equal(_i32(nk[3]), _i32(nk[4])) and not bool((pk == 5).any())      # identical classes: the later one never wins
    alpha2 = float(nk[6, 0])
    nk2, pk2 = run(alpha2)
    assert torch.equal(_i32(nk2), _i32(nk))
    check_pred(nk2, pk2, alpha2)
    if npix > 1:
        assert alpha2 > 0.9 and int(pk[0]) == 7 and int(pk2[0]) == 0                # a tie with alpha is not a strict maximum


# ------------------------------------------------------------------------------------------------ sgd_step (optim.hip)
SGD_BIG = 8192 * 256 * 4 + 1024       # one more than the grid covers in one pass: the grid-stride loop runs again over the tail


def _sgd_segments(numel):
    if numel == 4:
        return [(0, 4, 0.01, 5e-4)]
    M = 1 << 20
    # five segments; [3M, 3M + 4096) lies in none of them (lr = wd = 0 there); one segment has wd == 0; the last ends with the tail
    return [(0, M, 0.01, 5e-4), (M, 3 * M, 0.02, 0.0), (3 * M + 4096, 6 * M, 0.1, 5e-4), (6 * M, 8 * M, 0.2, 1e-3), (8 * M, numel, 0.05, 5e-4)]


@pytest.mark.parametrize("numel,momentum,gscale", [(SGD_BIG, 5e-4, 1.0), (SGD_BIG, 0.9, 0.125), (4, 0.9, 0.125)])
def test_sgd_step(numel, momentum, gscale):
    """d = g * gscale + wd * p; buf = first ? d : mom * buf + d; p -= lr * buf: three steps against a float64 step from the kernel's
    own previous state, with and without the bf16 mirror."""
    L = _L()
    g = _gen(numel % 1000 + int(momentum * 10))
    segs = _sgd_segments(numel)
    lr = torch.zeros(numel, dtype=torch.float64)
    wd = torch.zeros(numel, dtype=torch.float64)
    covered = torch.zeros(numel, dtype=torch.bool)
    for b, e, l, w in segs:
        lr[b:e], wd[b:e], covered[b:e] = float(np.float32(l)), float(np.float32(w)), True
    mom, gs = float(np.float32(momentum)), float(np.float32(gscale))
    p0 = torch.randn(numel, generator=g)
    pa, pb = p0.clone().to(DEV), p0.clone().to(DEV)
    buf_a = torch.full((numel,), float("nan"), device=DEV)    # garbage on entry: the first step must not read it
    buf_b = torch.full((numel,), float("inf"), device=DEV)
    mir_w, mir = _guarded(numel, 1.0, torch.bfloat16)
    p_prev, buf_prev = p0.double(), None
    for step in range(3):
        grad = torch.randn(numel, generator=g) * (8.0 if gscale != 1.0 else 1.0)
        gd = grad.to(DEV)
        L.sgd_step(pa, gd, buf_a, segs, momentum, gscale, step == 0, bf16_mirror=mir)
        L.sgd_step(pb, gd, buf_b, segs, momentum, gscale, step == 0)
        pk, bk = pa.cpu(), buf_a.cpu()
        assert torch.equal(_i32(pb), _i32(pk)) and torch.equal(_i32(buf_b), _i32(bk))     # the mirror changes nothing
        assert torch.equal(_i16(mir), _i16(pk.bfloat16())) and _guard_ok(mir_w)
        g0 = grad.double() * gs
        dd = g0 + wd * p_prev
        bref = dd if step == 0 else mom * buf_prev + dd
        pref = p_prev - lr * bref
        # g * gscale 1 u; each fma one rounding of its result: d (u |d|), buf (u |buf|, d's error passes through), p (u |p|, buf's times lr)
        e_d = U32 * (g0.abs() + dd.abs())
        e_b = e_d + U32 * bref.abs()
        assert bool(((bk.double() - bref).abs() <= SAFETY * e_b).all()), f"step {step}: buf"
        assert bool(((pk.double() - pref).abs() <= SAFETY * (lr * e_b + U32 * pref.abs())).all()), f"step {step}: p"
        # outside every segment: lr = wd = 0 -> p untouched, bit for bit; the first buf is the rounded product alone
        assert torch.equal(_i32(pk[~covered]), _i32(p0[~covered]))
        if step == 0:
            assert torch.equal(_i32(bk[~covered]), _i32((grad * torch.tensor(gscale))[~covered]))
        p_prev, buf_prev = pk.double(), bk.double()
    if numel > 4:
        assert int((~covered).sum()) == 4096


# ------------------------------------------------------------------------------------------------ exact utilities (api.hip, loss.hip)
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("ic_rot", [0, 3])
@pytest.mark.parametrize("OC,T,IC,OCp,ICp", [(6, 9, 10, 8, 16), (24, 1, 195, 32, 200)])
def test_pack_weights(OC, T, IC, OCp, ICp, ic_rot, dtype):
    """master [OC][T][IC] -> fwd [OCp][T][ICp] and tr [ICp][T][OCp], zero padded, packed column ic = master column (ic + ic_rot) % IC."""
    L = _L()
    master = torch.randn(OC, T, IC, generator=_gen(OC + IC + ic_rot))
    want = torch.zeros(OCp, T, ICp)
    want[:OC, :, :IC] = torch.roll(master, -ic_rot, dims=2)
    want_f, want_t = want.to(dtype), want.permute(2, 1, 0).contiguous().to(dtype)
    code = L.dtype_code(want_f)
    for use_f, use_t in ((True, True), (True, False), (False, True)):
        f_w, wf = _guarded(OCp * T * ICp, SENT, dtype)
        t_w, wt = _guarded(OCp * T * ICp, SENT, dtype)
        L.pack_weights(master.to(DEV), wf if use_f else None, wt if use_t else None, OC, T, IC, OCp, ICp, code, ic_rot=ic_rot)
        assert _guard_ok(f_w) and _guard_ok(t_w)
        for used, got, ref in ((use_f, wf, want_f), (use_t, wt, want_t)):
            if used:
                assert torch.equal(got.cpu().view(ref.shape).float(), ref.float())
            else:
                assert bool((got.cpu().float() == SENT).all())


def test_copy2d_batch():
    """three pieces with different strides (16-byte chunks = 4 floats) into a sentinel-filled destination: only the named chunks change"""
    L = _L()
    src = torch.arange(4 * 400, dtype=torch.float32)
    dst0 = torch.full((4 * 500,), SENT)
    pieces = [(3, 10, 5, 2, 7, 9), (60, 100, 1, 33, 33, 40), (200, 300, 9, 4, 11, 4)]     # src_off, dst_off, rows, cols16, ld_src, ld_dst
    table, want, first = [], dst0.view(-1, 4).clone(), 0
    s4 = src.view(-1, 4)
    for so, do, rows, cols, lds, ldd in pieces:
        table.append([first, so, do, rows, cols, lds, ldd])
        for r in range(rows):
            want[do + r * ldd: do + r * ldd + cols] = s4[so + r * lds: so + r * lds + cols]
        first += rows * cols
    dst = dst0.to(DEV)
    L.copy2d_batch(src.to(DEV), dst, torch.tensor(table, dtype=torch.int64, device=DEV), len(pieces), first)
    assert torch.equal(dst.cpu().view(-1, 4), want)
    assert int((want != SENT).any(1).sum()) == first          # the pieces do not overlap: exactly `first` chunks were named


def test_dropout_scale():
    """out = u >= p ? 1 / (1 - p) : 0 with p = p0 below split_at and p1 from it on; u == p is kept; the scale is the f32 quotient."""
    L = _L()
    n, split = 1000, 333
    p0, p1 = 0.3, 0.5
    u = torch.rand(n, generator=_gen(5))
    p0f, p1f = torch.tensor(p0, dtype=torch.float32), torch.tensor(p1, dtype=torch.float32)
    u[0] = p0f; u[1] = torch.nextafter(p0f, torch.tensor(0.0)); u[2] = 0.0
    u[split - 1] = 0.4                                        # kept under p0, dropped under p1: the last index before split_at ...
    u[split] = 0.4; u[split + 1] = p1f; u[n - 1] = torch.nextafter(p1f, torch.tensor(0.0))      # ... and the first from it on
    out_w, out = _guarded(n, float("nan"))
    L.dropout_scale(u.to(DEV), out, split, p0, p1)
    assert _guard_ok(out_w)
    p = torch.where(torch.arange(n) < split, p0f, p1f)
    want = torch.where(u >= p, torch.tensor(1.0) / (torch.tensor(1.0) - p), torch.zeros(()))
    assert torch.equal(_i32(out), _i32(want))
    o = out.cpu()
    assert float(o[0]) > 1.4 and float(o[1]) == 0 and float(o[split - 1]) > 1.4 and float(o[split]) == 0 and float(o[split + 1]) == 2.0


def test_loss_finish():
    """acc = [cls1 + cls2, (rvmin1 + rvmin2) / 2, er_sum, ecr, cross, cross2, intra, -] -> [loss, cls, er, ecr, nce, intra, cross, cross2]
    with cls = acc0 / 2 + acc1, er = er_sum * er_coef, nce = cross + cross2 + intra, loss = cls + er + ecr + nce (contrast_train.py:174, 389-395)."""
    L = _L()
    acc = torch.randn(8, generator=_gen(8)) * torch.tensor([1.0, 0.1, 5e4, 0.3, 2.0, 2.0, 0.05, 1e9])
    er_coef = 1.0 / (2 * 20 * 128 * 128)
    out_w, out = _guarded(8, float("nan"))
    L.loss_finish(acc.to(DEV), er_coef, out)
    assert _guard_ok(out_w)
    a, k = acc.double(), float(np.float32(er_coef))
    cls, er, ecr, nce = a[0] * 0.5 + a[1], a[2] * k, a[3], a[4] + a[5] + a[6]
    want = torch.stack([cls + er + ecr + nce, cls, er, ecr, nce, a[6], a[4], a[5]])
    mag = a[0].abs() * 0.5 + a[1].abs() + (a[2] * k).abs() + a[3].abs() + a[4].abs() + a[5].abs() + a[6].abs()
    # at most 7 roundings on the way to the total (cls 2, er 1, nce 2, the total 3 adds; fewer for every other entry), each of a partial sum <= mag
    got = out.cpu().double()
    assert bool(((got - want).abs() <= SAFETY * 8 * U32 * mag).all()), (got, want)
    assert torch.equal(_i32(out[5:8]), _i32(acc[[6, 4, 5]]))  # plain copies
