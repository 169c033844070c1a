"""The DeepLab-v1 head's training path on the GPU (csrc/seg_head.hip, wseg_amd/seg_head.py, Engine.run_seg_head_train): the four kernels alone
through _lib, the head stage by stage, the whole chain through autograd into the training loss, and inference left as it was — against the
float64 restatement and the bars of tests/seg_head_f64.py (derived from the kernels' arithmetic, safety factor 2, never fitted to a run).
One Net + engine per precision mode, cached at module level."""
import pytest
import torch

from tests import seg_head_f64 as H
from tests.f64_bars import _gen
from tests.test_gpu_aff_head import _i, _round_once_bf16, assert_within
from wseg_amd import _lib as L, arch, synth
from wseg_amd.seg_head import backward_launches, seg_head, seg_head_backward, seg_head_forward
from wseg_amd.seg_loss import seg_cross_entropy

pytestmark = pytest.mark.gpu
DEV = "cuda"
MODES = ["fp32", "bf16", "bf16x3"]
# (N, h, w): no off-centre tap of the dilation-12 conv in range; one row / four columns of taps; both sides, and 868 rows = past the 256-row tiles
MAPS = [(1, 5, 7), (2, 13, 16), (1, 28, 31)]
TDT = {"fp32": torch.float32, "bf16": torch.bfloat16, "bf16x3": torch.float32}
EPS, MOM, P = 1e-5, 0.0003, 0.5
_NETS = {}


def _net(mode):
    if mode not in _NETS:
        from wseg_amd.deeplabv1_resnet38 import Net
        m = Net(precision=mode)
        m.load_state_dict(synth.procedural_seg_state_dict(0), strict=True)
        _NETS[mode] = m.cuda().train()
    return _NETS[mode]


# ------------------------------------------------------------------------------------------------ 1. the four kernels alone
# (M, C, ld, first column).  Row chunks (from the workspace size): 2 and 32 rows are ONE partial per column, 35 two, 416 thirteen, 1311 forty-one
SHAPES = [(2, 8, 8, 0), (32, 16, 16, 0), (35, 512, 512, 0), (416, 512, 512, 0), (1311, 64, 96, 8)]
DTYPES = [(torch.float32, torch.float32), (torch.bfloat16, torch.bfloat16), (torch.bfloat16, torch.float32)]      # (z / y / dz, g)
KEY = 0x9E3779B1


def _wide(block, ld, c0, dt):
    """`block` [M, C] as columns [c0, c0 + C) of NaN rows ld wide: (the matrix, the pointer view from column c0)"""
    wide = torch.full((block.shape[0], ld), float("nan"), dtype=dt, device=DEV)
    wide[:, c0:c0 + block.shape[1]] = block.to(dt).to(DEV)
    return wide, wide.view(-1)[c0:]


def _vec(C, fill=None):
    v = torch.full((C + 8,), float("nan"), device=DEV)
    if fill is not None:
        v[:C] = fill.to(DEV)
    return v


def _kernels_once(M, C, ld, c0, zdt, gdt, z, g, gamma, beta, rm, rv, inplace=False):
    """the four kernels in the head's order on one set of inputs: {name: tensor} of everything they write (buffers start as NaN)"""
    ws = torch.empty(L.bn_stats_workspace_bytes(M, C), device=DEV, dtype=torch.uint8)
    o = {k: _vec(C) for k in ("mean", "invstd", "scale", "shift", "d_gamma", "d_beta", "sums")}
    o["running_mean"], o["running_var"] = _vec(C, rm), _vec(C, rv)
    zw, zv = _wide(z, ld, c0, zdt)
    L.bn_stats(zv, ld, M, C, gamma, beta, EPS, MOM, o["mean"], o["invstd"], o["scale"], o["shift"], o["running_mean"], o["running_var"], ws)
    o["y"], yv = _wide(torch.full((M, C), float("nan")), ld, c0, zdt)
    L.bn_relu_drop(zv, ld, o["scale"], o["shift"], yv, ld, M, C, P, KEY)
    gw, gv = _wide(g, ld, c0, gdt)
    if inplace:
        o["dz"], dzv = gw, gv
    else:
        o["dz"], dzv = _wide(torch.full((M, C), float("nan")), ld, c0, zdt)
    L.bn_relu_backward(gv, ld, yv, ld, zv, ld, o["mean"], o["invstd"], gamma, 1.0 / (1.0 - P), dzv, ld, o["d_gamma"], o["d_beta"], M, C, ws)
    gw2, gv2 = _wide(g, ld, c0, gdt)
    L.col_sums(gv2, ld, M, C - 3, o["sums"], ws)
    return o


@pytest.mark.parametrize("dts", DTYPES, ids=lambda d: "-".join(str(x).replace("torch.", "") for x in d))
@pytest.mark.parametrize("M,C,ld,c0", SHAPES)
def test_head_kernels(M, C, ld, c0, dts):
    zdt, gdt = dts
    bf = zdt == torch.bfloat16
    chunks = H.workspace_chunks(L.bn_stats_workspace_bytes(M, C), C)
    assert chunks == H.row_chunks(M) and (chunks == 1) == (M <= 32)
    gen = _gen(M + C)
    z = torch.randn(M, C, generator=gen)
    z[:, 0] += 64.0                                             # mean = 64 std: the cancellation case
    z[:, 1] = 0.375                                             # constant: var 0
    z = z.to(zdt).float()
    g = torch.randn(M, C, generator=gen).to(gdt).float()
    gamma, beta = (torch.rand(C, generator=gen) + 0.5).to(DEV), (torch.rand(C, generator=gen) - 0.5).to(DEV)
    beta[2] = -100.0                                            # y is zero in every row of column 2
    rm, rv = torch.rand(C, generator=gen) - 0.5, torch.rand(C, generator=gen) + 0.5
    o = _kernels_once(M, C, ld, c0, zdt, gdt, z, g, gamma, beta, rm, rv)
    # nothing outside the C columns / elements is written
    cols = torch.ones(M, ld, dtype=torch.bool)
    cols[:, c0:c0 + C] = False
    for k in ("y", "dz"):
        assert torch.isnan(o[k].cpu()[cols]).all(), k
    for k in ("mean", "invstd", "scale", "shift", "d_gamma", "d_beta", "running_mean", "running_var"):
        assert torch.isnan(o[k][C:]).all() and torch.isfinite(o[k][:C]).all(), k
    assert torch.isnan(o["sums"][C - 3:]).all()
    # the statistics
    z64, g64, ga64, be64 = z.double().to(DEV), g.double().to(DEV), gamma.double(), beta.double()
    ref = H.bn_stats(z64, ga64, be64, EPS, MOM, rm.double().to(DEV), rv.double().to(DEV))
    for k in ("mean", "invstd", "scale", "shift", "running_mean", "running_var"):
        assert_within(k, o[k][:C], *ref[k])
    assert float(o["invstd"][1]) == float(torch.tensor(EPS ** -0.5, dtype=torch.float64).float())      # the constant column: var = 0 exactly
    assert float(o["mean"][1]) == 0.375
    # y: the dropped elements are the host mask's, the kept ones 2 relu(z scale + shift) rounded once
    keep = synth.dropout_keep(M, C, KEY, P, device=DEV)
    y = o["y"][:, c0:c0 + C]
    sc64, sh64 = o["scale"][:C].double(), o["shift"][:C].double()
    assert_within("y", y, *H.bn_relu_drop(z64, sc64, sh64, keep, P, bf))
    exact = 2.0 * torch.relu(z64 * sc64 + sh64)
    once = _round_once_bf16(exact) if bf else exact.float()
    assert bool((y[~keep] == 0).all()) and torch.equal(_i(y[keep]), _i(once[keep]))
    assert bool((y[:, 2] == 0).all()) and (M * C < 4096 or 0.1 < float((y > 0).double().mean()) < 0.45)
    # the backward
    rb = H.bn_relu_backward(g64, y.double(), z64, o["mean"][:C].double(), o["invstd"][:C].double(), ga64, 1.0 / (1.0 - P), bf)
    dz = o["dz"][:, c0:c0 + C]
    assert_within("d_beta", o["d_beta"][:C], *rb["s1"])
    assert_within("d_gamma", o["d_gamma"][:C], *rb["s2"])
    assert_within("dz", dz, *rb["dz"])
    assert bool((dz[:, 2] == 0).all()) and float(o["d_beta"][2]) == 0.0 and float(o["d_gamma"][2]) == 0.0
    assert_within("col_sums", o["sums"][:C - 3], *[t_[:C - 3] for t_ in H.col_sums(g64)])
    # a second run gives the same bits in every output (NaN padding included); in place (dz = g) where the dtypes agree, too
    o2 = _kernels_once(M, C, ld, c0, zdt, gdt, z, g, gamma, beta, rm, rv, inplace=zdt == gdt)
    for k in o:
        a, b = o[k], o2[k]
        if k == "dz" and zdt == gdt:                            # (the in-place buffer holds g's NaN frame: the same frame)
            assert torch.isnan(b.cpu()[cols]).all()
            a, b = a[:, c0:c0 + C], b[:, c0:c0 + C]
        assert torch.equal(_i(a), _i(b)), k


def test_col_sums_of_the_cls_gradient_rows():
    """the d_bias launch: 21 sums of [M][24] rows, the pad columns ignored (NaN there must not reach a sum)"""
    for M, dt in ((868, torch.float32), (416, torch.bfloat16)):
        x = torch.randn(M, 24, generator=_gen(M)).to(dt).to(DEV)
        x[:, 21:] = float("nan")
        out = _vec(24)
        L.col_sums(x, 24, M, 21, out, torch.empty(L.bn_stats_workspace_bytes(M, 24), device=DEV, dtype=torch.uint8))
        ref, bar = H.col_sums(x.double()[:, :21])
        assert_within("d_bias", out[:21], ref, bar)
        assert torch.isnan(out[21:]).all()


def test_refusals_come_before_any_launch():
    x = torch.zeros(64, 16, device=DEV)
    v = torch.ones(16, device=DEV)
    ws = torch.empty(L.bn_stats_workspace_bytes(64, 16), device=DEV, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="more than one value per channel"):
        L.bn_stats(x, 16, 1, 16, v, v, EPS, MOM, v.clone(), v.clone(), None, None, None, None, ws)
    with pytest.raises(RuntimeError, match="multiple of 8"):
        L.bn_stats(x, 16, 64, 12, v, v, EPS, MOM, v.clone(), v.clone(), None, None, None, None, ws)
    with pytest.raises(RuntimeError, match="multiple of 8"):
        L.bn_relu_drop(x, 12, v, v, x.clone(), 16, 64, 8, 0.5, 1)
    with pytest.raises(RuntimeError, match="16-byte aligned"):
        L.bn_relu_drop(x.view(-1)[1:], 16, v, v, x.clone(), 16, 63, 8, 0.5, 1)
    with pytest.raises(RuntimeError, match="may alias g only"):
        L.bn_relu_backward(x, 16, x.clone(), 16, x.clone(), 16, v, v, v, 2.0, x, 8, None, None, 63, 8, ws)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ 2. the head stage by stage
def _t_rows(mode, N, h, w, seed):
    return torch.relu(torch.randn(N * h * w, 4096, generator=_gen(seed))).to(TDT[mode]).to(DEV)


def _reset_grads(net, eng):
    eng.attach_grads()
    eng.flat_g.zero_()
    for p_ in (net.cls_conv.bias, net.bn_fov.weight, net.bn_fov.bias, net.bn_fov2.weight, net.bn_fov2.bias):
        p_.grad = None


@pytest.mark.parametrize("N,h,w", MAPS)
@pytest.mark.parametrize("mode", MODES)
def test_head_stage_by_stage(mode, N, h, w):
    net, bf = _net(mode), mode == "bf16"
    M, key = N * h * w, synth.dropout_key(3, h)
    t = _t_rows(mode, N, h, w, M)
    bns = (net.bn_fov, net.bn_fov2)
    before = [(b.running_mean.double().clone(), b.running_var.double().clone(), int(b.num_batches_tracked)) for b in bns]
    rows, ctx = seg_head_forward(net, t, N, h, w, key)
    eng = ctx["eng"]
    W = {k: v.to(DEV) for k, v in H.weights64(net, mode).items()}
    d = lambda x: x.double()                                                    # noqa: E731
    X0 = H.unfold_rows(d(t), N, h, w)
    x = X0
    keep = synth.dropout_keep(M, 512, key, P, device=DEV)
    for i, (cname, bn) in enumerate(zip(("conv_fov", "conv_fov2"), bns), 1):
        assert_within(f"z{i}", ctx[f"z{i}"], *H.conv(x, W[cname], mode))
        st = H.bn_stats(d(ctx[f"z{i}"]), d(bn.weight.detach()), d(bn.bias.detach()), bn.eps, bn.momentum, before[i - 1][0], before[i - 1][1])
        for j, k in enumerate(("mean", "invstd", "scale", "shift")):
            assert_within(f"{k}{i}", ctx[f"stats{i}"][j], *st[k])
        assert_within(f"running_mean{i}", bn.running_mean, *st["running_mean"])
        assert_within(f"running_var{i}", bn.running_var, *st["running_var"])
        assert int(bn.num_batches_tracked) == before[i - 1][2] + 1
        y = ctx[f"y{i}"]
        assert_within(f"y{i}", y, *H.bn_relu_drop(d(ctx[f"z{i}"]), d(ctx[f"stats{i}"][2]), d(ctx[f"stats{i}"][3]), keep if i == 2 else None, P, bf))
        x = d(y)
    assert bool((ctx["y2"][~keep] == 0).all())
    W3 = torch.zeros(24, 512, dtype=torch.float64, device=DEV)
    W3[:21] = W["cls_conv"]
    bias = torch.zeros(24, dtype=torch.float64, device=DEV)
    bias[:21] = d(net.cls_conv.bias.detach())
    assert_within("rows", rows, *H.conv(d(ctx["y2"]), W3, mode, bias))
    assert bool((rows[:, 21:] == 0).all())

    d_rows = torch.zeros(M, 24, device=DEV)
    d_rows[:, :21] = (torch.randn(M, 21, generator=_gen(M + 1)) / M).to(DEV)
    scale7 = (torch.rand(4096, generator=_gen(7)) + 0.5).to(DEV)
    for epi1 in (False, True):
        _reset_grads(net, eng)
        cap = {}
        d_t = seg_head_backward(ctx, d_rows, **(dict(scale=scale7, mask=t) if epi1 else {}), capture=cap)
        tag = " (epi 1)" if epi1 else ""
        dp = d(cap["d_pad"])[:, :21]
        assert bool((cap["d_pad"][:, 21:] == 0).all())
        assert_within("d_bias" + tag, net.cls_conv.bias.grad, *H.col_sums(d(d_rows)[:, :21]))
        assert_within("dW_cls" + tag, eng.grad_view("cls_conv").reshape(21, 512), *H.wgrad(d(ctx["y2"]), dp, mode))
        assert_within("d_y2" + tag, cap["d_y2"], *H.dgrad(dp, W["cls_conv"], mode))
        b2 = H.bn_relu_backward(d(cap["d_y2"]), d(ctx["y2"]), d(ctx["z2"]), d(ctx["mean2"]), d(ctx["invstd2"]), d(net.bn_fov2.weight.detach()), 2.0, bf)
        assert_within("dz2" + tag, cap["dz2"], *b2["dz"])
        assert_within("d_beta2" + tag, net.bn_fov2.bias.grad, *b2["s1"])
        assert_within("d_gamma2" + tag, net.bn_fov2.weight.grad, *b2["s2"])
        assert_within("dW_fov2" + tag, eng.grad_view("conv_fov2").reshape(512, 512), *H.wgrad(d(ctx["y1"]), d(cap["dz2"]), mode))
        assert_within("d_y1" + tag, cap["d_y1"], *H.dgrad(d(cap["dz2"]), W["conv_fov2"], mode))
        b1 = H.bn_relu_backward(d(cap["d_y1"]), d(ctx["y1"]), d(ctx["z1"]), d(ctx["mean1"]), d(ctx["invstd1"]), d(net.bn_fov.weight.detach()), 1.0, bf)
        assert_within("dz1" + tag, cap["dz1"], *b1["dz"])
        assert_within("d_beta1" + tag, net.bn_fov.bias.grad, *b1["s1"])
        assert_within("d_gamma1" + tag, net.bn_fov.weight.grad, *b1["s2"])
        assert_within("dW_fov" + tag, eng.grad_view("conv_fov").reshape(512, 4096 * 9), *H.wgrad(X0, d(cap["dz1"]), mode))
        assert_within("d_t" + tag, d_t, *H.dgrad3(d(cap["dz1"]), W["conv_fov"], N, h, w, mode, *((d(scale7), d(t)) if epi1 else ())))
        assert set(cap["plans"]) == {"cls_conv", "conv_fov2", "conv_fov"}
    _reset_grads(net, eng)


def test_the_backward_launches_are_the_ones_planned():
    for mode in MODES:
        dt = L.F32X3 if mode == "bf16x3" else (L.BF16 if mode == "bf16" else L.F32)
        launches = backward_launches(2, 13, 16, dt)
        assert launches["wgrad_cls_conv"]["OC_dw"] == 21 and launches["wgrad_cls_conv"]["ld_dy"] == launches["dgrad_cls_conv"]["IC"] == 64
        assert launches["dgrad_conv_fov"]["dil"] == launches["wgrad_conv_fov"]["dil"] == 12 and launches["dgrad_conv_fov"]["mode"] == 1


# ------------------------------------------------------------------------------------------------ 4. end to end through autograd
def _end_to_end(mode, key, seed=5):
    net = _net(mode)
    N, h, w = 2, 13, 16
    eng = net._engine.active(torch.device(DEV, torch.cuda.current_device()))
    _reset_grads(net, eng)
    conv6 = torch.relu(torch.randn(N, 4096, h, w, generator=_gen(seed))).to(DEV).requires_grad_(True)
    label = torch.randint(0, 21, (N, 104, 128), generator=_gen(seed + 1), dtype=torch.uint8)
    label[:, :9] = 255
    out = seg_head(net, conv6, key)
    seen = {}
    out.register_hook(lambda g: seen.update(g=g.detach().clone()))
    loss, stats = seg_cross_entropy(out[:, :21], label)
    loss.backward()
    got = dict(out=out.detach().clone(), loss=loss.detach().clone(), d_conv6=conv6.grad.clone(), d_bias=net.cls_conv.bias.grad.clone(),
               d_gamma1=net.bn_fov.weight.grad.clone(), d_beta1=net.bn_fov.bias.grad.clone(), d_gamma2=net.bn_fov2.weight.grad.clone(),
               d_beta2=net.bn_fov2.bias.grad.clone(), g=seen["g"], **{"dW_" + k: eng.grad_view(k).clone() for k in H.CONVS})
    _reset_grads(net, eng)
    return got, conv6.detach(), label


@pytest.mark.parametrize("mode", MODES)
def test_end_to_end_is_deterministic_and_keyed(mode):
    a, _c, _l = _end_to_end(mode, 11)
    b, _c, _l = _end_to_end(mode, 11)
    for k in a:
        if not k.startswith("dW_"):                             # (some weight-gradient kernels accumulate with float atomics)
            assert torch.equal(_i(a[k]), _i(b[k])), k
    c, _c, _l = _end_to_end(mode, 12)
    assert not torch.equal(a["out"], c["out"]) and not torch.equal(a["d_conv6"], c["d_conv6"])
    assert float(a["loss"]) > 0 and bool(torch.isfinite(a["d_conv6"]).all())


@pytest.mark.parametrize("mode", MODES)
def test_end_to_end_through_autograd(mode):
    """seg_head -> seg_cross_entropy -> backward().  (a) The autograd form IS the engine-layout path: on the same rows and the gradient the loss
    handed back, seg_head_forward / seg_head_backward give the same bits in everything but the conv weight gradients (float atomics: those
    agree within twice the launch's bar) — and that path is held to the float64 bars launch by launch above.  (b) Every result lies within the
    COMPOSED bar of the float64 chain run from the inputs alone (H.chain: worst-case radii through three products and two normalisations).  At
    K = 36864 those bars are vacuous — measured, fp32: d_conv6 8.6e-10 off the float64 chain at max |d_conv6| 4.3e-4 under a bar of 8e10; bf16
    7.4e-5; bf16x3 5.2e-9 — so (b) states the deviation from float64 (printed per result) more than it tests it; (a) is the test."""
    net, bf = _net(mode), mode == "bf16"
    N, h, w, key = 2, 13, 16, 11
    M = N * h * w
    a, conv6, _label = _end_to_end(mode, key)
    eng = net._engine.active(conv6.device)
    t = conv6.permute(0, 2, 3, 1).to(TDT[mode]).contiguous().view(M, 4096)
    g_rows = a["g"].permute(0, 2, 3, 1).contiguous().view(M, 24)
    assert bool((g_rows[:, 21:] == 0).all())
    # (a) the engine-layout path on the same operands
    rows, ctx = seg_head_forward(net, t, N, h, w, key)
    assert torch.equal(_i(rows.view(N, h, w, 24).permute(0, 3, 1, 2)), _i(a["out"]))
    _reset_grads(net, eng)
    cap = {}
    d_t = seg_head_backward(ctx, g_rows, capture=cap)
    assert torch.equal(_i(d_t.view(N, h, w, 4096).permute(0, 3, 1, 2).float()), _i(a["d_conv6"]))
    for k, p_ in (("d_bias", net.cls_conv.bias), ("d_gamma1", net.bn_fov.weight), ("d_beta1", net.bn_fov.bias), ("d_gamma2", net.bn_fov2.weight),
                  ("d_beta2", net.bn_fov2.bias)):
        assert torch.equal(_i(p_.grad), _i(a[k])), k
    d = lambda x: x.double()                                                    # noqa: E731
    X0 = H.unfold_rows(d(t), N, h, w)
    for k, x, dy in (("cls_conv", d(ctx["y2"]), d(cap["d_pad"])[:, :21]), ("conv_fov2", d(ctx["y1"]), d(cap["dz2"])), ("conv_fov", X0, d(cap["dz1"]))):
        _ref, bar = H.wgrad(x, dy, mode)
        diff = (d(eng.grad_view(k)).reshape(bar.shape) - d(a["dW_" + k]).reshape(bar.shape)).abs()
        assert bool((diff <= 2 * bar).all()), k
    _reset_grads(net, eng)
    # (b) the float64 chain from the inputs alone
    W = {k: v.to(DEV) for k, v in H.weights64(net, mode).items()}
    bn = {1: (d(net.bn_fov.weight.detach()), d(net.bn_fov.bias.detach())), 2: (d(net.bn_fov2.weight.detach()), d(net.bn_fov2.bias.detach()))}
    comp = H.chain(d(t), W, d(net.cls_conv.bias.detach()), bn, synth.dropout_keep(M, 512, key, P, device=DEV), d(g_rows)[:, :21], N, h, w, mode,
                   net.bn_fov.eps, P)
    rows_of = lambda x: x.permute(0, 2, 3, 1).reshape(M, -1)                    # noqa: E731
    got = {"rows": rows_of(a["out"])[:, :21], "d_t": rows_of(a["d_conv6"]), "d_bias": a["d_bias"], "dW_cls_conv": a["dW_cls_conv"].reshape(21, 512),
           "dW_conv_fov2": a["dW_conv_fov2"].reshape(512, 512), "dW_conv_fov": a["dW_conv_fov"].reshape(512, 4096 * 9),
           "d_gamma1": a["d_gamma1"], "d_beta1": a["d_beta1"], "d_gamma2": a["d_gamma2"], "d_beta2": a["d_beta2"]}
    assert set(got) == set(comp)
    for k, (ref, bar) in comp.items():
        ok, ratio = H.inside(got[k], ref, bar)
        print(f"{mode} {k}: max |err| {float((d(got[k]) - ref).abs().max()):.3e}, max |ref| {float(ref.abs().max()):.3e}, max composed bar "
              f"{float(bar.max()):.3e}, max err / bar {ratio:.4f}")
        assert ok and bool(torch.isfinite(got[k]).all()), k


# ------------------------------------------------------------------------------------------------ 5. nothing else moved
@pytest.mark.parametrize("mode", MODES)
def test_eval_follows_the_trained_statistics_and_the_backbone_packs_stay(mode):
    from wseg_amd.deeplabv1_resnet38 import Net
    net = Net(precision=mode)
    net.load_state_dict(synth.procedural_seg_state_dict(0), strict=True)
    net.cuda().eval()
    x = synth.synthetic_images(1, (40, 56), 3).to(DEV)
    net.coarse_logits(x)
    eng = net._engine.active(x.device)
    # an untouched net: run_seg_head is the three launches with the folds of the stored statistics, bit for bit
    P_ = eng.ensure_packs(x.device, L.F32X3 if mode == "bf16x3" else (L.BF16 if mode == "bf16" else L.F32))
    for bname in ("bn_fov", "bn_fov2"):
        bn = getattr(net, bname)
        scale = bn.weight.detach().float() / torch.sqrt(bn.running_var.float() + arch.BN_EPS)
        assert torch.equal(P_["bn"][bname][0], scale) and torch.equal(P_["bn"][bname][1], bn.bias.detach().float() - bn.running_mean.float() * scale)
    frozen_before = {k: v for k, v in eng._frozen_packs["w"].items()}
    bn_before = {k: v for k, v in eng._frozen_packs["bn"].items() if not k.startswith(("bn_fov", "cls_conv"))}
    fkey = eng._frozen_key
    stats_before = {b_: (getattr(net, b_).running_mean.clone(), getattr(net, b_).running_var.clone()) for b_ in ("bn_fov", "bn_fov2")}
    # one training step of the head
    net.train()
    N, h, w = 1, 5, 7
    rows, ctx = seg_head_forward(net, _t_rows(mode, N, h, w, 9), N, h, w, 77)
    d_rows = torch.zeros(N * h * w, 24, device=DEV)
    d_rows[:, :21] = 0.01
    seg_head_backward(ctx, d_rows)
    net.eval()
    rows1, _dims = net.coarse_logits(x)
    for bname in ("bn_fov", "bn_fov2"):                         # the running statistics moved, and eval folds the new ones
        bn = getattr(net, bname)
        scale = bn.weight.detach().float() / torch.sqrt(bn.running_var.float() + arch.BN_EPS)
        assert torch.equal(eng._frozen_packs["bn"][bname][0], scale)
        assert torch.equal(eng._frozen_packs["bn"][bname][1], bn.bias.detach().float() - bn.running_mean.float() * scale)
        assert not torch.equal(bn.running_mean, stats_before[bname][0]) and not torch.equal(bn.running_var, stats_before[bname][1])
    assert eng._frozen_key == fkey
    assert all(eng._frozen_packs["w"][k] is v for k, v in frozen_before.items())
    assert all(eng._frozen_packs["bn"][k] is v for k, v in bn_before.items())
    fresh = Net(precision=mode)
    fresh.load_state_dict(net.state_dict(), strict=True)
    fresh.cuda().eval()
    rows2, _dims = fresh.coarse_logits(x)
    assert torch.equal(_i(rows1), _i(rows2))
    assert int(net.bn_fov.num_batches_tracked) == int(net.bn_fov2.num_batches_tracked) == 1
    # training mode is still refused by the net itself
    with pytest.raises(RuntimeError, match="inference-only"):
        net.train().forward(x)
    with pytest.raises(RuntimeError, match="TRAINING path"):
        seg_head_forward(net.eval(), _t_rows(mode, N, h, w, 9), N, h, w, 77)
