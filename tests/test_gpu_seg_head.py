"""The DeepLab-v1 head's training path on the GPU (csrc/seg_head.hip, wseg_amd/seg_head.py, Engine.run_seg_head_train): the four kernels alone
through _lib, the head stage by stage, the whole chain through autograd into the training loss, and inference left as it was — against the
float64 restatement and the bars of tests/seg_head_f64.py (derived from the kernels' arithmetic, safety factor 2, never fitted to a run).
The kernel cases cross every size at which the kernels change path (row chunks longer than 32 rows, more than one batch of partials in the
finish kernels, the second trip of the streaming launches: _assert_geometry states each), every option of wseg_bn_relu_drop (no dropout, a keep
factor that is no power of two, the mixed dtype pairs) and the false-tie correction of its bf16 store on inputs aimed at it.  One Net + engine per precision mode, cached at module level."""
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
# — all of 32 rows, one batch of the finish kernels.  Past 16384 rows the chunks grow (GEOMETRY): 16420 rows are 457 chunks of 36 rows with
# a tail of 4 — four batches of 128 partials, the last one clamped — on 264 columns (no multiple of 64: idle lanes in the finish and in the
# reduce), and 16420 x 264 / 8 chunks of 8 columns are more than the 2048 x 256 threads of a streaming launch: the second trip of the
# grid-stride loops, out of place and in place.  31360 rows (N = 10 at 56 x 56) are 490 chunks of 64 rows, on the narrowest legal row.
SHAPES = [(2, 8, 8, 0), (32, 16, 16, 0), (35, 512, 512, 0), (416, 512, 512, 0), (1311, 64, 96, 8), (16420, 264, 272, 8), (31360, 8, 8, 0)]
GEOMETRY = {16420: dict(R=36, chunks=457, tail=4, depth=13), 31360: dict(R=64, chunks=490, tail=64, depth=20)}      # what the large M are there for
STREAM_GRID = 2048 * 256                                         # threads of the widest streaming launch (sh_stream_blocks)
FINISH_BATCH = 16 * 8                                            # partials a finish workgroup loads per batch (16 groups x SH_BATCH)
DTYPES = [(torch.float32, torch.float32), (torch.bfloat16, torch.bfloat16), (torch.bfloat16, torch.float32)]      # (z / y / dz, g)
KEY = 0x9E3779B1


def _assert_geometry(M, C):
    """the thresholds a shape crosses, from the restated constants: a later change of the kernels' constants fails here, not silently"""
    R, chunks = H.rows_per_chunk(M), H.row_chunks(M)
    assert (R == 32) == (M <= 16384) and chunks <= 512
    if M in GEOMETRY:
        geo = GEOMETRY[M]
        assert (R, chunks, M - (chunks - 1) * R, H.depth(M)) == (geo["R"], geo["chunks"], geo["tail"], geo["depth"])
        assert chunks > 3 * FINISH_BATCH and chunks % FINISH_BATCH != 0               # four batches, the last one partly past the end
    else:
        assert chunks <= FINISH_BATCH
    return M * C // 8 > STREAM_GRID                              # the streaming launches take a second trip


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
    assert _assert_geometry(M, C) == (M == 16420) and (M != 16420 or (C % 64 != 0 and ld != C))
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


# wseg_bn_relu_drop alone: every (z, y) dtype pair at p = 0 (the launch after bn_fov: no dropout), 0.25 (a keep factor that is no power of two)
# and 0.5, on a small column slice of several workgroups and on the shape whose launch strides
DROP_SHAPES = [(1311, 64, 96, 8), (16420, 264, 272, 8)]
DROP_DTYPES = [(torch.float32, torch.float32), (torch.bfloat16, torch.bfloat16), (torch.float32, torch.bfloat16), (torch.bfloat16, torch.float32)]   # (z, y)


def _drop_once(z, zdt, ydt, scale, shift, M, C, ld, c0, p, key):
    _zw, zv = _wide(z, ld, c0, zdt)
    yw, yv = _wide(torch.full((M, C), float("nan")), ld, c0, ydt)
    L.bn_relu_drop(zv, ld, scale, shift, yv, ld, M, C, p, key)
    return yw


@pytest.mark.parametrize("p", [0.0, 0.25, 0.5])
@pytest.mark.parametrize("dts", DROP_DTYPES, ids=lambda d: "-".join(str(x).replace("torch.", "") for x in d))
@pytest.mark.parametrize("M,C,ld,c0", DROP_SHAPES)
def test_bn_relu_drop_options(M, C, ld, c0, dts, p):
    zdt, ydt = dts
    bf = ydt == torch.bfloat16
    large = _assert_geometry(M, C)
    assert large == (M == 16420)
    gen = _gen(M + C + 1)
    z = torch.randn(M, C, generator=gen).to(zdt).float()
    scale, shift = _vec(C, torch.rand(C, generator=gen) + 0.5), _vec(C, torch.rand(C, generator=gen) - 0.5)
    shift[2] = -100.0                                           # y is zero in every row of column 2
    yw = _drop_once(z, zdt, ydt, scale, shift, M, C, ld, c0, p, KEY)
    cols = torch.ones(M, ld, dtype=torch.bool)
    cols[:, c0:c0 + C] = False
    assert torch.isnan(yw.cpu()[cols]).all()                    # nothing outside the C columns is written
    y = yw[:, c0:c0 + C]
    z64, sc64, sh64 = z.double().to(DEV), scale[:C].double(), shift[:C].double()
    keep = synth.dropout_keep(M, C, KEY, p, device=DEV) if p > 0 else None
    assert_within(f"y (p = {p})", y, *H.bn_relu_drop(z64, sc64, sh64, keep, p, bf))
    pre = torch.relu(z64 * sc64 + sh64)
    assert bool((y[:, 2] == 0).all()) and 0.3 < float((pre > 0).double().mean()) < 0.7
    other = _drop_once(z, zdt, ydt, scale, shift, M, C, ld, c0, p, KEY + 1)[:, c0:c0 + C]
    if p == 0.0:                                                # relu(fma(z, scale, shift)) rounded once; no element dropped, the key unused
        once = _round_once_bf16(pre) if bf else pre.float()
        assert torch.equal(_i(y), _i(once)) and torch.equal(_i(other), _i(y))
        return
    assert bool((y[~keep] == 0).all()) and bool((y[keep & (pre.float() > 0)] > 0).all())     # the dropped elements: exactly the mask's zeros
    assert not torch.equal(_i(other), _i(y))
    share = float(keep.double().mean())
    if large:
        assert abs(share - (1.0 - p)) <= 0.01, share            # (4.3 M elements: 0.01 is 48 standard deviations)
    if p == 0.5:                                                # the factor 2 is exact: the kept elements are 2 relu(.) rounded once
        once = _round_once_bf16(2.0 * pre) if bf else (2.0 * pre).float()
        assert torch.equal(_i(y[keep]), _i(once[keep]))
    # (p = 0.25: the f32 factor 4/3 and its product round again, "rounded once" does not hold and is not asserted: the bar above is the test)


# ---- the false-tie correction (sh_off_the_false_tie), aimed at.  fmaf(z, a, b) is ONE rounding to f32; the bf16 store rounds again.  Where the
# f32 value ends in 0x8000 — exactly between two bf16 values — while the exact z a + b does not, the second rounding alone would go to the even
# neighbour whatever side the exact value is on.  a0 / a1 = 1 + 2^-8 / 1 + 2^-7 + 2^-8 are such patterns with an even / odd bf16 below;
# b = +-2^-30 is below half an f32 ulp of the product: it decides the side and leaves the f32 pattern.  2^-60 does the same and vanishes in
# float64 too (the kernel's residual branch): the oracle is exact rational arithmetic, and equals the float64 expression wherever that is exact.
_A0, _A1, _T, _E = 1.0 + 2.0 ** -8, 1.0 + 2.0 ** -7 + 2.0 ** -8, 2.0 ** -30, 2.0 ** -60
# (z, scale, shift, expected bf16 bits or None, lands on the tie pattern)
TIES = [
    (1.0, _A0, _T, 0x3F81, True), (1.0, _A0, -_T, 0x3F80, True), (1.0, _A0, 0.0, 0x3F80, True),           # false ties, and the true tie: even
    (1.0, _A1, _T, 0x3F82, True), (1.0, _A1, -_T, 0x3F81, True), (1.0, _A1, 0.0, 0x3F82, True),           # the odd neighbour below
    (1.0, _A0, _E, 0x3F81, True), (1.0, _A0, -_E, 0x3F80, True), (1.0, _A1, -_E, 0x3F81, True), (1.0, _A1, _E, 0x3F82, True),
    (-1.0, -_A0, _T, 0x3F81, True), (-1.0, -_A0, -_T, 0x3F80, True), (-1.0, -_A1, -_T, 0x3F81, True),     # a positive result of negative operands
    (1.0, -_A0, _T, 0x0000, True), (1.0, -_A0, -_T, 0x0000, True), (-1.0, _A1, 0.0, 0x0000, True),        # a negative pre-activation: +0
    (2.0, _A0, _T, 0x4001, True), (0.5, _A1, -_T, 0x3F01, True), (4.0, _A1, 0.0, 0x4082, True),           # other binades
    (1.0, 1.0, _T, 0x3F80, False), (1.0, _A0 + 2.0 ** -20, 0.0, 0x3F81, False),                           # no tie pattern: the correction stays out
    (_A0, 1.0, _T, 0x3F81, True), (_A0, 1.0, -_T, 0x3F80, True), (_A1, 1.0, 0.0, 0x3F82, True), (_A0, 2.0, -_T, 0x4000, True),   # f32 z carries it
    (_A1, 1.0, -_T, 0x3F81, True), (_A0, -1.0, _T, 0x0000, True),
]
TIES_BF16_Z = [t_ for t_ in TIES if t_[0] in (1.0, -1.0, 2.0, 0.5, 4.0)]


def _bf16_bits(x):
    """the bf16 bit pattern of the non-negative rational x (a normal number or 0), rounded ONCE, to nearest, ties to even"""
    from fractions import Fraction
    if x == 0:
        return 0
    e = 0
    while Fraction(2) ** (e + 1) <= x:
        e += 1
    while Fraction(2) ** e > x:
        e -= 1
    m = x / Fraction(2) ** (e - 7)                               # in [128, 256): 8 significant bits before the point
    q, rem = int(m), m - int(m)
    q += 1 if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and q % 2 == 1) else 0
    return ((e + 127) << 7) + (q - 128)                          # (q = 256 carries into the exponent by itself)


@pytest.mark.parametrize("zdt", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_bn_relu_drop_false_ties(zdt):
    from fractions import Fraction
    ties = TIES if zdt == torch.float32 else TIES_BF16_Z
    n, M = len(ties), 32                                         # one row block; every row holds every case (z is constant down a column)
    C = (n + 7) // 8 * 8
    assert M * C // 8 <= 256
    zc, sc, sh = torch.ones(C), torch.ones(C), torch.zeros(C)
    zc[:n], sc[:n], sh[:n] = (torch.tensor([t_[j] for t_ in ties], dtype=torch.float64).float() for j in range(3))
    assert torch.equal(zc.to(zdt).float(), zc) and [float(v) for v in sc[:n]] == [t_[1] for t_ in ties]       # the operands are exact
    assert _i(sc[:1])[0] == 0x3F808000 and 0x3F818000 in _i(sc[:n]).tolist()
    exact = [Fraction(t_[0]) * Fraction(t_[1]) + Fraction(t_[2]) for t_ in ties]
    r32 = torch.tensor([float(v) for v in exact], dtype=torch.float64).float()          # fmaf's result (these double roundings are exact or far off a tie)
    on_tie = [(b & 0xFFFF) == 0x8000 for b in _i(r32).tolist()]
    assert on_tie == [t_[4] for t_ in ties] and sum(e_ != Fraction(float(r)) for e_, r, t_ in zip(exact, r32, ties) if t_[4]) >= 12
    z = zc[None, :].expand(M, C).contiguous()
    scale, shift = _vec(C, sc), _vec(C, sh)
    z64 = z.double().to(DEV)
    for p, factor in ((0.0, 1), (0.5, 2)):
        want = torch.tensor([_bf16_bits(max(v, Fraction(0)) * factor) for v in exact], dtype=torch.int32)
        if p == 0.0:
            assert want.tolist() == [t_[3] for t_ in ties]
        yw = _drop_once(z, zdt, torch.bfloat16, scale, shift, M, C, C, 0, p, KEY)
        got = _i(yw).cpu().to(torch.int32) & 0xFFFF
        keep = synth.dropout_keep(M, C, KEY, p) if p > 0 else torch.ones(M, C, dtype=torch.bool)
        assert bool(keep[:, :n].any(0).all()) and bool((got[~keep] == 0).all())         # every case is kept in some row
        rows_want = want[None, :].expand(M, n)
        bad = (got[:, :n] != rows_want) & keep[:, :n]
        assert not bool(bad.any()), (p, [(ties[c], hex(int(got[r, c]))) for r, c in bad.nonzero().tolist()[:8]])
        # the float64 expression rounded once is the same oracle wherever float64 holds the sum exactly (all but the 2^-60 shifts)
        f64 = factor * torch.relu(z64 * scale[:C].double() + shift[:C].double())
        once = (_i(_round_once_bf16(f64)).cpu().to(torch.int32) & 0xFFFF)[:, :n]
        exact64 = torch.tensor([abs(t_[2]) != _E for t_ in ties])
        assert torch.equal(once[:, exact64], rows_want[:, exact64])
        assert torch.equal(got[:, :n][:, exact64][keep[:, :n][:, exact64]], once[:, exact64][keep[:, :n][:, exact64]])


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


def test_head_stages_past_16384_rows_bf16():
    """N = 1, 129 x 128 = 16512 rows in bf16: the smallest map whose column reductions run 36-row chunks (459 of them, a tail of 24) — through the
    engine path's own workspace, d_pad and in-place backward, which the kernel tests above do not touch.  Every launch but the two of K = 36864
    is held to its bar from the path's own upstream tensors, as in test_head_stage_by_stage.  The dilation-12 conv_fov launches (forward, data
    and weight gradient) are only required to be finite here: their unfolded float64 operand would be 5 GB, and tests/test_gpu_seg_head_conv.py
    and tests/test_gpu_seg_head_bwd_conv.py hold those launches on every tile family.  The families the planner chose are printed."""
    from wseg_amd.seg_head import _conv
    mode, N, h, w = "bf16", 1, 129, 128
    net, bf, M = _net(mode), True, N * h * w
    assert M > 16384 >= 128 * 128                                                                          # the first map past the threshold
    assert (H.rows_per_chunk(M), H.row_chunks(M), M - 458 * 36, H.depth(M)) == (36, 459, 24, 13)
    assert M * 512 // 8 > STREAM_GRID                                                                      # the streaming launches stride
    key = synth.dropout_key(3, h)
    t = torch.relu(torch.randn(M, 4096, generator=torch.Generator(device=DEV).manual_seed(M), device=DEV)).to(TDT[mode])
    bns = (net.bn_fov, net.bn_fov2)
    before = [(b.running_mean.double().clone(), b.running_var.double().clone(), int(b.num_batches_tracked)) for b in bns]
    rows, ctx = seg_head_forward(net, t, N, h, w, key)
    eng = ctx["eng"]
    W = {k: v.to(DEV) for k, v in H.weights64(net, mode).items()}
    d = lambda x: x.double()                                                    # noqa: E731
    keep = synth.dropout_keep(M, 512, key, P, device=DEV)
    assert bool(torch.isfinite(ctx["z1"]).all())                                # conv_fov forward: finite only (see above)
    assert_within("z2", ctx["z2"], *H.conv(d(ctx["y1"]), W["conv_fov2"], mode))
    for i, bn in enumerate(bns, 1):
        st = H.bn_stats(d(ctx[f"z{i}"]), d(bn.weight.detach()), d(bn.bias.detach()), bn.eps, bn.momentum, before[i - 1][0], before[i - 1][1])
        for j, k in enumerate(("mean", "invstd", "scale", "shift")):
            assert_within(f"{k}{i}", ctx[f"stats{i}"][j], *st[k])
        assert_within(f"running_mean{i}", bn.running_mean, *st["running_mean"])
        assert_within(f"running_var{i}", bn.running_var, *st["running_var"])
        assert int(bn.num_batches_tracked) == before[i - 1][2] + 1
        assert_within(f"y{i}", ctx[f"y{i}"], *H.bn_relu_drop(d(ctx[f"z{i}"]), d(ctx[f"stats{i}"][2]), d(ctx[f"stats{i}"][3]), keep if i == 2 else None, P, bf))
    assert bool((ctx["y2"][~keep] == 0).all())
    W3 = torch.zeros(24, 512, dtype=torch.float64, device=DEV)
    W3[:21] = W["cls_conv"]
    bias = torch.zeros(24, dtype=torch.float64, device=DEV)
    bias[:21] = d(net.cls_conv.bias.detach())
    assert_within("rows", rows, *H.conv(d(ctx["y2"]), W3, mode, bias))
    assert bool((rows[:, 21:] == 0).all())

    d_rows = torch.zeros(M, 24, device=DEV)
    d_rows[:, :21] = torch.randn(M, 21, generator=torch.Generator(device=DEV).manual_seed(M + 1), device=DEV) / M
    _reset_grads(net, eng)
    cap = {}
    d_t = seg_head_backward(ctx, d_rows, capture=cap)
    dp = d(cap["d_pad"])[:, :21]
    assert bool((cap["d_pad"][:, 21:] == 0).all())
    assert_within("d_bias", net.cls_conv.bias.grad, *H.col_sums(d(d_rows)[:, :21]))
    assert_within("dW_cls", eng.grad_view("cls_conv").reshape(21, 512), *H.wgrad(d(ctx["y2"]), dp, mode))
    assert_within("d_y2", cap["d_y2"], *H.dgrad(dp, W["cls_conv"], mode))
    b2 = H.bn_relu_backward(d(cap["d_y2"]), d(ctx["y2"]), d(ctx["z2"]), d(ctx["mean2"]), d(ctx["invstd2"]), d(net.bn_fov2.weight.detach()), 2.0, bf)
    assert_within("dz2", cap["dz2"], *b2["dz"])
    assert_within("d_beta2", net.bn_fov2.bias.grad, *b2["s1"])
    assert_within("d_gamma2", net.bn_fov2.weight.grad, *b2["s2"])
    assert_within("dW_fov2", eng.grad_view("conv_fov2").reshape(512, 512), *H.wgrad(d(ctx["y1"]), d(cap["dz2"]), mode))
    assert_within("d_y1", cap["d_y1"], *H.dgrad(d(cap["dz2"]), W["conv_fov2"], mode))
    b1 = H.bn_relu_backward(d(cap["d_y1"]), d(ctx["y1"]), d(ctx["z1"]), d(ctx["mean1"]), d(ctx["invstd1"]), d(net.bn_fov.weight.detach()), 1.0, bf)
    assert_within("dz1", cap["dz1"], *b1["dz"])
    assert_within("d_beta1", net.bn_fov.bias.grad, *b1["s1"])
    assert_within("d_gamma1", net.bn_fov.weight.grad, *b1["s2"])
    dW_fov = eng.grad_view("conv_fov")
    assert bool(torch.isfinite(dW_fov).all()) and bool(torch.isfinite(d_t).all()) and float(dW_fov.abs().max()) > 0 and float(d_t.abs().max()) > 0
    assert set(cap["plans"]) == {"cls_conv", "conv_fov2", "conv_fov"}
    launches = backward_launches(N, h, w, L.BF16)
    for name in H.CONVS:
        fwd = L.conv_plan(dtype=L.BF16, **_conv(name, [(h, w)], arch.SEG_CLS_ROWS if name == "cls_conv" else None).fwd_kw(N))
        print(f"{name}: forward geometry {fwd}; data gradient {cap['plans'][name]}; weight gradient {L.wgrad_plan(**launches['wgrad_' + name])}")
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
