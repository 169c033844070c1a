"""The AffinityNet head's training path on the GPU (csrc/aff_head.hip, wseg_amd/aff_head.py, Engine.run_aff_head): the ELU-backward kernel
alone, the forward with context and the backward stage by stage against the float64 restatement and the bars of tests/aff_head_f64.py
(derived from the kernels' arithmetic, safety factor 2, never fitted to a run), the whole chain through autograd into the training
loss, and inference left bit for bit as it was.  One Net + engine per precision mode, cached at module level."""
import pytest
import torch
import torch.nn.functional as F

from tests import aff_head_f64 as H
from tests import aff_loss_f64 as A
from tests.f64_bars import SAFETY, U32, _gen
from wseg_amd import _lib as L, synth
from wseg_amd.aff_head import aff_head_backward, aff_head_forward, affinity_head, backward_launches
from wseg_amd.aff_loss import affinity_loss
from wseg_amd.resnet38_aff import pair_radius

pytestmark = pytest.mark.gpu
DEV = "cuda"
MODES = ["fp32", "bf16", "bf16x3"]
# (N, h, w): 35 rows = one partial tile; 416 rows = several 64-row tiles with a 32-row tail; 1311 rows = past the 256-row tiles, with a tail
MAPS = [(1, 5, 7), (2, 13, 16), (3, 19, 23)]
TDT = {"fp32": torch.float32, "bf16": torch.bfloat16, "bf16x3": torch.float32}
_NETS = {}


def _net(mode):
    if mode not in _NETS:
        from wseg_amd.resnet38_aff import Net
        m = Net(precision=mode)
        m.load_state_dict(synth.procedural_aff_state_dict(0), strict=True)
        _NETS[mode] = m.cuda()
    return _NETS[mode]


def _i(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def assert_within(name, got, ref, bar):
    err = (got.double() - ref).abs()
    worst = float((err - bar).max())
    ratio = float((err / torch.as_tensor(bar, dtype=torch.float64, device=err.device).clamp_min(1e-300)).max())
    print(f"{name}: max |err| {float(err.max()):.3e}, max bar {float(torch.as_tensor(bar).max()):.3e}, max (err - bar) {worst:.3e}, "
          f"max err / bar {ratio:.4f}")
    assert torch.isfinite(got).all() and worst <= 0.0, name


# ------------------------------------------------------------------------------------------------ 1. the ELU-backward kernel alone
# M, C, ld_g, ld_y, ld_dz, first column.  The last: 9370 x 448 / 8 = 524720 chunks, past the 2048 x 256 threads of one launch — the second
# trip of the grid-stride loop, on a column slice (ld 456), out of place and in place
ELU_SHAPES = [(1, 8, 8, 8, 8, 0), (35, 448, 448, 448, 448, 0), (416, 256, 448, 448, 448, 192), (1311, 64, 96, 448, 72, 0),
              (9370, 448, 456, 448, 456, 8)]
ELU_STRIDES = {9370}                                           # the M whose launch takes the second trip
ELU_GRID = 2048 * 256                                          # threads of the widest launch (csrc/aff_head.hip: at most 2048 workgroups)
ELU_DTYPES = [(torch.float32, torch.float32, torch.float32), (torch.float32, torch.bfloat16, torch.bfloat16),
              (torch.bfloat16, torch.bfloat16, torch.bfloat16)]


def _round_once_bf16(exact):
    """float64 -> bf16 with ONE rounding: to f32 by round-to-odd (truncate, then set the last bit when inexact: 24 bits are more than bf16's 8 + 2),
    then the ordinary f32 -> bf16 rounding"""
    t = exact.float()
    t = torch.where(t.double().abs() > exact.abs(), torch.nextafter(t, torch.zeros_like(t)), t)
    sticky = (t.double() != exact).to(torch.int32)
    return (t.view(torch.int32) | sticky).view(torch.float32).bfloat16()


@pytest.mark.parametrize("gscale", [None, 3.0])
@pytest.mark.parametrize("dts", ELU_DTYPES, ids=lambda d: "-".join(str(x).replace("torch.", "") for x in d))
@pytest.mark.parametrize("M,C,ld_g,ld_y,ld_dz,c0", ELU_SHAPES)
def test_elu_backward_rows(M, C, ld_g, ld_y, ld_dz, c0, dts, gscale):
    gdt, ydt, zdt = dts
    assert (M * C // 8 > ELU_GRID) == (M in ELU_STRIDES)      # which cases stride: a later change of the grid cannot silently empty them
    if M in ELU_STRIDES:
        assert ld_g != C and ld_dz != C and ld_g == ld_dz      # ... on a column slice, and in place below where the dtypes agree
    gen = _gen(M + C)
    g = torch.randn(M, ld_g, generator=gen).to(gdt)
    y = F.elu(torch.randn(M, ld_y, generator=gen))
    cols = torch.arange(ld_y)[None, :] + torch.arange(M)[:, None]
    y[cols % 5 == 0] = -1.0                                   # ELU saturated exactly
    y[cols % 5 == 1] = 0.0                                    # the y + 1 branch with derivative 1
    y[cols % 5 == 2] = y[cols % 5 == 2].abs() + 0.125         # positive
    y = y.to(ydt)
    gd, yd = g.to(DEV), y.to(DEV)
    gs = None if gscale is None else torch.tensor([gscale], device=DEV)
    dz = torch.full((M, ld_dz), float("nan"), dtype=zdt, device=DEV)
    cy = min(c0, ld_y - C)                                    # (y of ld_y = C has no column to skip: the slice of g and dz against whole rows of y)
    gv, yv, zv = gd.view(-1)[c0:], yd.view(-1)[cy:], dz.view(-1)[c0:]          # a column slice: the same rows from column c0 on
    L.elu_backward_rows(gv, ld_g, yv, ld_y, gs, zv, ld_dz, M, C)
    got = dz.cpu()
    g64, y64 = g.double()[:, c0:c0 + C], y.double()[:, cy:cy + C]
    ref, bar = H.elu_backward(g64, y64, gscale, zdt == torch.bfloat16)
    out = got[:, c0:c0 + C]
    assert torch.isfinite(out).all()
    assert_within("dz", out, ref, bar)
    keep = torch.ones(M, ld_dz, dtype=torch.bool)
    keep[:, c0:c0 + C] = False
    assert torch.isnan(got[keep]).all()                       # nothing outside the C columns is written
    # the exact properties
    pos, sat, zero = y64 > 0, y64 == -1, y64 == 0
    assert pos.any() and sat.any() and zero.any()
    exact = g64 * (1.0 if gscale is None else gscale)         # f32 x f32: exact in float64
    once = _round_once_bf16(exact) if zdt == torch.bfloat16 else exact.float()
    assert torch.equal(_i(out[pos]), _i(once[pos]))           # gscale * g rounded once
    assert torch.equal(_i(out[zero]), _i(once[zero]))         # derivative 1
    assert bool((out[sat] == 0).all())
    # in place (dz = g) where dtype and ld agree: the same bits
    if gdt == zdt:
        g2 = torch.full((M, ld_dz), float("nan"), dtype=gdt, device=DEV)
        g2[:, c0:c0 + C] = gd[:, c0:c0 + C]
        v2 = g2.view(-1)[c0:]
        L.elu_backward_rows(v2, ld_dz, yv, ld_y, gs, v2, ld_dz, M, C)
        assert torch.equal(_i(g2.cpu()[:, c0:c0 + C]), _i(out))
        assert torch.isnan(g2.cpu()[keep]).all()


# ------------------------------------------------------------------------------------------------ inputs of the head
def _inputs(mode, N, h, w, seed):
    """(conv4, conv5, t) pixel rows in the mode's dtype: normal samples, t = relu of one (exact zeros)"""
    M = N * h * w
    where = DEV if M > 5000 else "cpu"                        # (the training shape: 100 M samples are drawn on the device)
    gen = torch.Generator(device=where).manual_seed(seed)
    c4, c5 = torch.randn(M, 512, generator=gen, device=where), torch.randn(M, 1024, generator=gen, device=where)
    t = torch.relu(torch.randn(M, 4096, generator=gen, device=where))
    return [x.to(TDT[mode]).to(DEV) for x in (c4, c5, t)]


def _inference_head(net, c4, c5, t, N, h, w):
    """the head as Net.affinities launches it (no context)"""
    eng = net._engine.active(t.device)
    return eng.run_aff_head(c4, c5, t, [(h, w)], N)


# ------------------------------------------------------------------------------------------------ 2. forward with context
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("N,h,w", MAPS)
def test_head_forward_against_f64(N, h, w, mode):
    net = _net(mode)
    c4, c5, t = _inputs(mode, N, h, w, 11 + h)
    f9, ctx = aff_head_forward(net, c4, c5, t, N, h, w)
    W = {k: v.to(DEV) for k, v in H.weights64(net, mode).items()}
    feat = ctx["feat"]
    assert f9.shape == (N * h * w, 448) and f9.dtype == TDT[mode] and ctx["f9"] is f9
    for name, x in (("f8_3", c4), ("f8_4", c5), ("f8_5", t)):
        a, b = H.SLICES[name]
        ref, bar = H.elu_conv(x.double(), W[name], mode)
        assert_within(name, feat[:, a:b], ref, bar)
    ref, bar = H.elu_conv(feat.double(), W["f9"], mode)       # fed with the kernel path's own feat
    assert_within("f9", f9, ref, bar)
    assert float((f9.double() < 0).double().mean()) > 0.05 and float((f9.double() > 0).double().mean()) > 0.05     # both ELU branches
    feat_i, f9_i = _inference_head(net, c4, c5, t, N, h, w)
    assert torch.equal(_i(f9_i), _i(f9)) and torch.equal(_i(feat_i), _i(feat))


# ------------------------------------------------------------------------------------------------ 3. backward stage by stage
def _backward_case(mode, N, h, w, epi1=False, twice=True):
    net = _net(mode)
    M = N * h * w
    c4, c5, t = _inputs(mode, N, h, w, 23 + h)
    eng = net._engine.active(t.device)
    d_f9 = (torch.randn(M, 448, generator=_gen(5 + h)) * 1e-3).to(DEV)
    gs = torch.tensor([3.0], device=DEV)
    f9, ctx = aff_head_forward(net, c4, c5, t, N, h, w)
    W = {k: v.to(DEV) for k, v in H.weights64(net, mode).items()}
    ops = {}
    if epi1:                                                  # the BN-ReLU backward operands; the mask is t itself (exact zeros: no near-tie)
        ops = dict(scale=(torch.rand(4096, generator=_gen(3)) + 0.5).to(DEV), mask=t)
    eng.attach_grads()
    eng.flat_g.zero_()
    cap = {}
    d4, d5, dt_ = aff_head_backward(ctx, d_f9, gs, capture=cap, **ops)
    once = {k: eng.grad_slice(k).clone() for k in W}
    feat64, dz9, dzf = ctx["feat"].double(), cap["dz9"], cap["dzf"]
    bf = mode == "bf16"
    ref, bar = H.elu_backward(d_f9.double(), f9.double(), 3.0, bf)
    assert_within("dz9", dz9, ref, bar)
    ref, bar_w9 = H.wgrad(feat64, dz9.double(), mode)
    assert_within("dW_f9", once["f9"].view(448, 448), ref, bar_w9)
    bars_w = {"f9": bar_w9}
    ref, bar = H.dgrad(dz9.double(), W["f9"], mode)
    assert_within("d_feat", cap["d_feat"], ref, bar)
    ref, bar = H.elu_backward(cap["d_feat"].double(), feat64, None, bf)
    assert_within("dzf", dzf, ref, bar)
    for name, x, dx in (("f8_3", c4, d4), ("f8_4", c5, d5), ("f8_5", t, dt_)):
        a, b = H.SLICES[name]
        dy = dzf.double()[:, a:b]
        ref, bars_w[name] = H.wgrad(x.double(), dy, mode)
        assert_within("dW_" + name, once[name].view(ref.shape), ref, bars_w[name])
        gate = dict(scale=ops["scale"].double(), mask=t.double()) if (epi1 and name == "f8_5") else {}
        ref, bar = H.dgrad(dy, W[name], mode, **gate)
        assert dx.shape == x.shape and dx.dtype == x.dtype
        assert_within("d_" + name, dx, ref, bar)
        if gate:
            assert bool((dx[t == 0] == 0).all()) and float((t == 0).double().mean()) > 0.3
    if twice:                                                 # weight gradients accumulate: a second backward, nothing zeroed in between
        aff_head_backward(ctx, d_f9, gs, **ops)
        for name in W:
            assert_within("2 x dW_" + name, eng.grad_slice(name).view(bars_w[name].shape), 2 * once[name].double().view(bars_w[name].shape),
                          2 * bars_w[name])
    return cap, ctx


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("N,h,w", MAPS)
def test_head_backward_stages(N, h, w, mode):
    cap, _ = _backward_case(mode, N, h, w)
    fam = cap["plans"]["f8_5"].family
    if mode == "bf16" and (N, h, w) == (3, 19, 23):
        assert fam == L.CONV_64x128, cap["plans"]["f8_5"]     # 1311 rows x 4096 channels: 64-row tiles
    if (N, h, w) == (1, 5, 7):
        assert fam == L.CONV_128x128, cap["plans"]["f8_5"]    # 35 rows: one 128-row tile per 128 channels


@pytest.mark.parametrize("mode", MODES)
def test_head_backward_bn_relu_operands(mode):
    """scale / mask on the f8_5 data gradient: the epilogue-1 form d_t * scale[c] * (t > 0)"""
    cap, _ = _backward_case(mode, 2, 13, 16, epi1=True, twice=False)
    assert cap["plans"]["f8_5"].family in (L.CONV_64x128, L.CONV_128x128)


def test_head_backward_training_shape_bf16():
    """N = 8, 56 x 56 in bf16: the size at which the planner moves the branch data gradients to the 256-tile kernel and the f9 / f8_5 weight
    gradients to the 256 x 256 pipe kernel — on column slices of ld 448, which no other launch of the project gives them."""
    N, h, w = 8, 56, 56
    la = backward_launches(N, h, w, L.BF16)
    assert L.conv_plan(**la["dgrad_f8_5"]).family in (L.CONV_224x256, L.CONV_256x256)
    assert L.wgrad_plan(**la["wgrad_f8_5"]).family == L.WGRAD_256x256 and L.wgrad_plan(**la["wgrad_f9"]).family == L.WGRAD_256x256
    cap, _ = _backward_case("bf16", N, h, w, twice=False)
    assert cap["plans"]["f8_5"].family in (L.CONV_224x256, L.CONV_256x256)


# ------------------------------------------------------------------------------------------------ 4. end to end through autograd
def test_autograd_head_and_loss_fp32():
    """loss = affinity_loss(affinity_head(net, c4, c5, c6), label); (3 loss).backward() against float64 autograd of the restated head with
    the restated loss (tests/aff_loss_f64.py) evaluated on the head's own f9.  First-order propagation of the stage bars (raw errors e_*,
    safety factor 2 on the sum; u = 2^-24; Wk = |W| in float64; elu' is 1-Lipschitz in the ELU output):
      e_feat, e_f9      the forward bars of tests/aff_head_f64.py; f9 adds e_feat Wk9^T
      e_dz9  = bar_grad of the loss * elu'(f9) + |g| e_f9 + 3 u |dz9|
      e_dfeat = e_dz9 Wk9 + 448 u (|dz9| Wk9);   e_dzf = e_dfeat elu'(feat) + |d_feat| e_feat + 3 u |dzf|
      e_dx   = e_dzf Wk + K u (|dzf| Wk);   e_dW9 = e_feat^T |dz9| + |feat|^T e_dz9 + M u |feat|^T |dz9|;   e_dW = |x|^T e_dzf + M u |x|^T |dzf|"""
    mode, N, h, w = "fp32", 2, 13, 16
    net = _net(mode)
    M, r = N * h * w, pair_radius(h, w)
    gen = _gen(77)
    c4 = torch.randn(N, 512, h, w, generator=gen).to(DEV).requires_grad_()
    c5 = torch.randn(N, 1024, h, w, generator=gen).to(DEV).requires_grad_()
    c6 = torch.relu(torch.randn(N, 4096, h, w, generator=gen)).to(DEV).requires_grad_()
    label = torch.stack([synth.synthetic_aff_label_map(h, w, 7 + i, block=2) for i in range(N)]).to(DEV)
    eng = net._engine.active(c6.device)
    eng.attach_grads()
    eng.flat_g.zero_()
    out = affinity_head(net, c4, c5, c6)
    assert out.shape == (N, 448, h, w) and out.is_contiguous(memory_format=torch.channels_last)
    loss, stats = affinity_loss(out, label)
    assert loss.grad_fn.saved["rows"].data_ptr() == out.data_ptr()              # the loss consumed the head's output without a copy
    (3 * loss).backward()
    assert net.f9.weight.grad.data_ptr() == eng.grad_slice("f9").data_ptr()     # a view into the flat gradient buffer

    W2 = {k: v.to(DEV) for k, v in H.weights64(net, mode).items()}
    w4 = {k: v.view(*v.shape, 1, 1).clone().requires_grad_() for k, v in W2.items()}
    x4, x5, x6 = (x.detach().double().requires_grad_() for x in (c4, c5, c6))
    feat64, f964 = H.restate_head(x4, x5, x6, w4)
    ref = A.restate(out.detach(), label, r, gscale=3.0)
    assert min(ref["counts"]) > 0                                               # no term is tested on an empty sum
    assert_within("loss", stats[:4], ref["out7"][:4], ref["bar_out7"][:4])
    f964.backward(ref["grad"])

    rows = lambda v: v.detach().permute(0, 2, 3, 1).reshape(M, -1)
    X = {"f8_3": rows(x4), "f8_4": rows(x5), "f8_5": rows(x6)}
    feat, f9, g = rows(feat64), rows(f964), rows(ref["grad"])
    Wk = {k: v.abs() for k, v in W2.items()}
    e_feat = torch.cat([H.gemm_bar(X[k], W2[k], mode) + H.EXPM1_ULP * feat[:, a:b].abs() for k, (a, b) in H.SLICES.items()], dim=1)
    e_f9 = H.gemm_bar(feat, W2["f9"], mode) + H.EXPM1_ULP * f9.abs() + e_feat @ Wk["f9"].T
    assert_within("f9", rows(out), f9, SAFETY * e_f9)
    dz9 = g * H.elu_grad(f9)
    e_dz9 = rows(ref["bar_grad"].expand(N, 448, h, w)) / SAFETY * H.elu_grad(f9) + g.abs() * e_f9 + 3 * U32 * dz9.abs()
    d_feat = dz9 @ W2["f9"]
    e_dfeat = e_dz9 @ Wk["f9"] + 448 * U32 * (dz9.abs() @ Wk["f9"])
    dzf = d_feat * H.elu_grad(feat)
    e_dzf = e_dfeat * H.elu_grad(feat) + d_feat.abs() * e_feat + 3 * U32 * dzf.abs()
    e_w = {"f9": e_feat.T @ dz9.abs() + feat.abs().T @ e_dz9 + M * U32 * (feat.abs().T @ dz9.abs())}
    for (k, (a, b)), xin, x64 in zip(H.SLICES.items(), (c4, c5, c6), (x4, x5, x6)):
        e_dx = e_dzf[:, a:b] @ Wk[k] + (b - a) * U32 * (dzf[:, a:b].abs() @ Wk[k])
        assert_within("d_" + k, rows(xin.grad), rows(x64.grad), SAFETY * e_dx)
        e_w[k] = X[k].abs().T @ e_dzf[:, a:b] + M * U32 * (X[k].abs().T @ dzf[:, a:b].abs())
    for k in W2:                                                                # e_w is [IC, OC]: dW = dY^T X is its transpose
        assert_within("dW_" + k, getattr(net, k).weight.grad.reshape(W2[k].shape), w4[k].grad.view(W2[k].shape), SAFETY * e_w[k].T)


# ------------------------------------------------------------------------------------------------ 5. inference untouched
@pytest.mark.parametrize("mode", MODES)
def test_inference_unchanged_after_a_head_backward(mode):
    from wseg_amd.resnet38_aff import Net
    net = _net(mode)
    _backward_case(mode, 1, 5, 7, twice=False)                # training packs + a context on this net
    x = synth.synthetic_images(1, (72, 56), 3).to(DEV)
    net.eval()
    aff, geo = net.affinities(x)
    fresh = Net(precision=mode)
    fresh.load_state_dict(synth.procedural_aff_state_dict(0), strict=True)
    fresh.eval().cuda()
    aff0, geo0 = fresh.affinities(x)
    assert geo == geo0 and torch.equal(_i(aff), _i(aff0))
    with pytest.raises(RuntimeError, match="inference-only"):
        net.train()(x)
    net.eval()
