"""The convolution kernels (csrc/conv_igemm.hip, conv_wgrad.hip, conv_wgrad_kernels.h, the stem) one family at a time through the C ABI against
the float64 references of tests/conv_f64.py, every element of every stored output inside the bar DERIVED there (storage rounding without a
safety factor + accumulation + epilogue arithmetic; tests/test_conv_bars_host.py shows on the CPU what those bars catch).  The kernel a case
names is asserted through the plan query (_conv / _wgrad of tests/test_gpu_conv.py); outputs start as NaN, or lie inside a sentinel guard
where a row stride or an offset is used.  Each test prints max err / bar per output (table of an MI355X run: profiles/README.md)."""
import pytest
import torch

from tests import conv_f64 as X
from tests.test_gpu_conv import CONV_FAMILY, ROWS_64_128, TILE_256, WGRAD_128, WGRAD_PIPE, _conv, _wgrad

pytestmark = pytest.mark.gpu

GUARD = -7.0
_problems = {}


def _problem(c):
    """operands, references and bars of a case: computed once, shared by the families that run it, never written to"""
    if c.name not in _problems:
        _problems[c.name] = X.conv_problem(c) if hasattr(c, "kind") else X.wgrad_problem(c)
    return _problems[c.name]


def _check(tag, got, ref, bar):
    err = (got.double().cpu() - ref).abs()
    print(f"{tag}: max err {float(err.max()):.3e}, max err/bar {float((err / bar).max()):.3f}")
    assert bool((err <= bar).all()), tag             # (a NaN left in the output fails here)


def _weights(p, dev):
    """the pack the kernel reads: [out_ch][taps][in_ch] (+ the second source's [out_ch][IC2] behind it), rows zero-padded to w_rows"""
    from wseg_amd import _lib as L
    c = p.c
    w1 = (p.w.permute(0, 2, 3, 1) if c.kind == "fwd" else p.w.permute(1, 2, 3, 0)).reshape(c.out_ch, -1)
    if c.IC2:
        w2 = p.w2.reshape(c.out_ch, c.IC2) if c.kind == "fwd" else p.w2.reshape(c.IC2, c.out_ch).t()
        w1 = torch.cat([w1, w2], dim=1)
    wrows = max(c.out_ch, getattr(c, "w_rows", 0))
    wp = torch.zeros(wrows, w1.shape[1], dtype=w1.dtype, device=dev)
    wp[:c.out_ch] = w1.to(dev)
    if c.dt == "x3":
        w32, wp = wp, torch.empty_like(wp)
        L.pack_x3(w32, wp)
    return wp


def _launch_kw(p, bm, dev):
    """the keywords of the launch of case p.c on family bm_hint = bm (operands on `dev`; the plan query takes them on the CPU too)"""
    from wseg_amd import _lib as L
    c, ep = p.c, p.ep
    in_sizes = c.sizes if c.kind == "fwd" else c.osizes
    kw = dict(N=c.N, IH=in_sizes[0][0], IW=in_sizes[0][1], IC=c.in_ch, OH=p.out_sizes[0][0], OW=p.out_sizes[0][1], OC=c.out_ch, KH=c.k, KW=c.k,
              stride=c.s, dil=c.d, pad=c.d * (c.k // 2), mode=int(c.kind == "dgrad"), bm_hint=bm, epi=ep["epi"], relu_out2=ep["relu_out2"],
              relu_lt=ep["relu_lt"], w_rows=getattr(c, "w_rows", 0), dtype=L.F32X3 if c.dt == "x3" else None)
    if c.seg2:
        kw["seg2"] = (*in_sizes[1], *p.out_sizes[1])
    for name in ("r_pre", "r_post", "mask", "scale", "shift", "drop"):
        if name in ep:
            kw[name] = ep[name].to(dev)
    if c.IC2:
        ld2 = c.ld_in2 or c.IC2                                     # (ld_in2 > IC2: the second source has a row stride)
        in2 = torch.zeros(sum(c.N * h * w for h, w in in_sizes), ld2, device=dev, dtype=X.TORCH_DT[c.dt])
        in2[:, :c.IC2] = torch.cat([X.rows(x) for x in p.x2s]).to(dev)
        kw.update(in2=in2, IC2=c.IC2, ld_in2=ld2)
    return kw


def _family(c, bm):
    return CONV_FAMILY[bm] if bm else (TILE_256 if c.IC2 else ROWS_64_128)


def _run_conv(p, bm):
    c, dev = p.c, "cuda"
    tdt = X.TORCH_DT[c.dt]
    kw = _launch_kw(p, bm, dev)
    inp = torch.cat([X.rows(x) for x in p.xs]).contiguous().to(dev)
    wide = c.opset in ("relu_lt_tail", "epi2_relu")                 # the stored block sits at channel offset 64 of rows 128 channels wider
    LD, OFF = (c.out_ch + 128, 64) if wide else (c.out_ch, 0)
    if wide:
        kw["ld_out"] = LD
    bufs = {name: torch.full((p.M, LD), GUARD if wide else float("nan"), device=dev, dtype=tdt) for name in p.refs}
    _conv(_family(c, bm), inp, _weights(p, dev), bufs["out"][:, OFF:] if "out" in bufs else None, bufs.get("out2"), perm=c.perm.get(bm), **kw)
    for name, (ref, bar) in p.refs.items():
        _check(f"{c.name} bm={bm} {name}", bufs[name][:, OFF:OFF + c.out_ch], ref, bar)
        if wide:
            assert bool((bufs[name][:, :OFF] == GUARD).all()) and bool((bufs[name][:, OFF + c.out_ch:] == GUARD).all())


CONV_RUNS = [(c, bm) for c in X.CONV_CASES + X.epi_cases() if not c.name.startswith("pair") for bm in c.fams]   # (pair*: _run_pair)


@pytest.mark.parametrize("c,bm", CONV_RUNS, ids=[f"{c.name}-{bm}" for c, bm in CONV_RUNS])
def test_conv_f64(c, bm):
    """forward and data gradient (bf16, f32, split-bf16), every epilogue operand set, two sources, two row segments"""
    _run_conv(_problem(c), bm)


@pytest.mark.parametrize("c", X.STEM_CASES, ids=lambda c: c.name)
def test_stem_f64(c):
    """the stem (f32 fma chain of 27 products from f32 operands) with its BN-ReLU second output, in both weight layouts"""
    from wseg_amd import _lib as L
    p, dev = _problem(c), "cuda"
    tdt = X.TORCH_DT[c.store]
    x, sc, sh = p.xs[0].contiguous().to(dev), p.ep["scale"].to(dev), p.ep["shift"].to(dev)
    for fn, w in ((L.stem_conv, p.w.permute(0, 2, 3, 1)), (L.stem_conv_kc, p.w.permute(2, 3, 1, 0).reshape(27, 64))):
        raw = torch.full((p.M, 64), float("nan"), device=dev, dtype=tdt)
        act = torch.full_like(raw, float("nan"))
        fn(x, w.contiguous().to(dev), sc, sh, raw, act, c.N, c.H, c.W, L.dtype_code(raw))
        _check(f"{c.name} {fn.__name__} raw", raw, *p.refs["out"])
        _check(f"{c.name} {fn.__name__} act", act, *p.refs["out2"])


def _wgrad_kw(c):
    """the geometry keywords of a weight-gradient case (conv_wgrad, wgrad_plan, and the pair grid's weight-gradient half)"""
    kw = dict(N=c.N, IH=c.H, IW=c.W, IC=c.IC, OH=c.osizes[0][0], OW=c.osizes[0][1], OC=c.OC, KH=c.k, KW=c.k, stride=c.s, dil=c.d,
              pad=c.d * (c.k // 2), ld_x=c.ld_x, ld_dy=c.ld_dy, dw_rot=c.dw_rot)
    if c.seg2:
        kw["seg2"] = (*c.seg2, *c.osizes[1])
    return kw


def _wgrad_launch_kw(c, hint):
    from wseg_amd import _lib as L
    return dict(IC_dw=c.IC_dw, OC_dw=c.OC_dw, tile_hint=hint, dtype={"f32": L.F32, "bf16": L.BF16, "x3": L.F32X3}[c.dt], **_wgrad_kw(c))


def _view(block, ld, off, dev):
    """`block` [rows][channels] as the column block [off, off + channels) of a matrix with rows `ld` wide whose every other element is NaN
    (a correct kernel decides channel validity per 16-byte chunk against IC / OC and never loads them): (pointer view, the matrix)"""
    if ld == block.shape[1] and off == 0:
        t = block.contiguous().to(dev)
        return t, t
    wide = torch.full((block.shape[0], ld), float("nan"), dtype=block.dtype, device=dev)
    wide[:, off:off + block.shape[1]] = block.to(dev)
    return wide.view(-1)[off:], wide


WGRAD_RUNS = [(c, h) for c in X.WGRAD_CASES.values() if c.name not in X.PAIR_CASES for h in c.hints]


@pytest.mark.parametrize("c,hint", WGRAD_RUNS, ids=[f"{c.name}-{h}" for c, h in WGRAD_RUNS])
def test_wgrad_f64(c, hint):
    """the weight gradient on zeros with the planner's split (or the one the case forces), then once more with split_k = 3 on top of that
    content; dw narrower than the operands and rotated where the case says so; operands as column blocks of wider NaN-filled matrices where
    it has row strides; a sentinel guard behind the buffer.  Kernel family and staging variant are asserted through the plan."""
    from wseg_amd import _lib as L
    p, dev = _problem(c), "cuda"
    xr, dyr = X.wgrad_rows(p)
    (xg, _xkeep), (dyg, _dykeep) = _view(xr, c.ld_x, c.x_off, dev), _view(dyr, c.ld_dy, c.dy_off, dev)
    n, NG, SENTINEL = p.ref.numel(), 4096, -12345.0
    buf = torch.zeros(n + NG, device=dev, dtype=torch.float32)
    buf[n:] = SENTINEL
    pipe = X.wgrad_pipe(c, hint)
    kw = _wgrad_launch_kw(c, hint)
    prior = None
    for split_k in (c.split_k, 3):
        plan = L.wgrad_plan(xg, dyg, buf, split_k=split_k, **kw)
        assert plan.unit == (c.unit if pipe else 0), (c.name, hint, plan)
        _wgrad(WGRAD_PIPE if pipe else WGRAD_128, xg, dyg, buf, split_k=split_k, **kw)
        got = buf[:n].reshape(p.ref.shape).double().cpu()
        ref, bar = X.wgrad_bar(p, plan.nsplit, prior)
        _check(f"{c.name} hint={hint} split_k={split_k} ({plan.nsplit} splits) dw", got, ref, bar)
        prior = got
    assert bool((buf[n:] == SENTINEL).all())


def _run_pair(name):
    from wseg_amd import _lib as L
    pd, pw, dev = _problem(next(c for c in X.CONV_CASES if c.name == name + "_dgrad")), _problem(X.WGRAD_CASES[name]), "cuda"
    c = pd.c
    dy = torch.cat([X.rows(x) for x in pd.xs]).contiguous().to(dev)
    xg, dyw = (t.contiguous().to(dev) for t in X.wgrad_rows(pw))
    dkw, wkw = _launch_kw(pd, 0, dev), _wgrad_kw(pw.c)
    wt = _weights(pd, dev)
    dx = torch.full((pd.M, c.Cin), float("nan"), device=dev, dtype=torch.bfloat16)
    n, NG, SENTINEL = pw.ref.numel(), 4096, -12345.0
    buf = torch.zeros(n + NG, device=dev, dtype=torch.float32)
    buf[n:] = SENTINEL
    fused, dg_plan, wg_plan = L.conv_pair_plan(wkw, dy, wt, dx, **dkw)
    assert fused == 1 and dg_plan.family in TILE_256 and wg_plan.family == WGRAD_PIPE and wg_plan.unit == pw.c.unit, (fused, dg_plan, wg_plan)
    L.conv_igemm(dy, wt, dx, pair_wgrad=(xg, dyw, buf, wkw), **dkw)
    _check(f"{name} dx", dx, *pd.refs["out"])
    _check(f"{name} dw ({wg_plan.nsplit} splits)", buf[:n].reshape(pw.ref.shape), *X.wgrad_bar(pw, wg_plan.nsplit))
    assert bool((buf[n:] == SENTINEL).all())


def test_conv_bwd_pair_f64():
    """wseg_conv_bwd_pair: data gradient and weight gradient of a layer in one grid (the smallest geometry the pair plan fuses)"""
    _run_pair("pair")


def test_conv_bwd_pair_seg2_f64():
    """the joint grid on two row segments: 1x1, N = 2, 119x125 + 36x44, 256 -> 256.  M1 = 29750 is no multiple of 64, so the seam falls
    inside a K-tile of a straight walk and the weight-gradient half has to split its range there.  (95x100 + 36x44 = 22168 pixels is not
    fused: the data gradient of a 256 -> 256 layer plans onto 256-row tiles, which the joint grid needs, only above 32768 pixels; this is the
    nearest two-segment geometry of the same shape that conv_pair_plan reports as fused.)"""
    _run_pair("pair_seg2")
