"""tests/seg_head_f64.py on the CPU: the stage restatements chained equal torch's float64 autograd of the reference's lines (output, d_t, every
parameter gradient, the running statistics of nn.BatchNorm2d(512, momentum=0.0003) after one step); a float32 evaluation of the same chain
passes every bar and planted defects fail one — also at 16420 and 31360 rows, where the row chunks are longer than 32 rows and the finish
kernels load more than one batch of partials (a miscounted tail chunk, a dropped batch and a reduce that disagrees with the finish about the
chunk length are planted there), and with the keep factor 4/3 of p = 0.25; the counter-hash dropout mask of synth.dropout_keep is balanced and its keys are independent;
the refusals of wseg_amd.seg_head."""
import math

import pytest
import torch
import torch.nn as nn

from tests import seg_head_f64 as H
from wseg_amd import synth

N, h, w, IC, C, NC = 2, 13, 16, 8, 512, 21
M = N * h * w
EPS, MOM, P = 1e-5, 0.0003, 0.5


def _rand(shape, seed, scale=1.0):
    return (torch.rand(shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64) * 2 - 1) * scale


def _problem():
    p = dict(t=_rand((M, IC), 1).relu(), W1=_rand((C, IC * 9), 2, (6.0 / (IC * 9)) ** 0.5), W2=_rand((C, C), 3, (6.0 / C) ** 0.5),
             W3=_rand((NC, C), 4, (6.0 / C) ** 0.5), bias=_rand((NC,), 5), d_rows=_rand((M, NC), 6, 1.0 / M),
             g1=_rand((C,), 7, 0.5) + 1, b1=_rand((C,), 8, 0.2), g2=_rand((C,), 9, 0.5) + 1, b2=_rand((C,), 10, 0.2),
             rm1=_rand((C,), 11, 0.2), rv1=_rand((C,), 12, 0.5) + 1, rm2=_rand((C,), 13, 0.2), rv2=_rand((C,), 14, 0.5) + 1,
             keep=synth.dropout_keep(M, C, synth.dropout_key(0, 0), P))
    return p


def _stats32(x, gamma, beta, rm, rv, defect=None):
    """wseg_bn_stats's arithmetic on f32 rows: per chunk the f32 sums about the chunk's first row, the finish in float64, outputs rounded to f32.
    defect: a planted fault of the large geometries (test_planted_size_defects_fail) — "tail_is_full": the finish counts the short last chunk as
    R rows; "first_batch_only": the finish adds the first 128 chunks and stops; "reduce_in_32_rows": the reduce sums 32 rows from each chunk's
    first row while the finish (and the chunks' first rows) follow R"""
    R = H.rows_per_chunk(x.shape[0])
    g = x[0].double()
    S1, S2 = torch.zeros_like(g), torch.zeros_like(g)
    for k, r0 in enumerate(range(0, x.shape[0], R)):
        if defect == "first_batch_only" and k >= 128:
            break
        blk = x[r0:r0 + R]
        n = R if defect == "tail_is_full" else blk.shape[0]
        d = (blk[:32] if defect == "reduce_in_32_rows" else blk) - blk[0]
        s1, s2, dk = d.sum(0).double(), (d * d).sum(0).double(), blk[0].double() - g
        S1 += s1 + n * dk
        S2 += s2 + 2 * dk * s1 + n * dk * dk
    m = x.shape[0]
    mean = g + S1 / m
    var = ((S2 - S1 * S1 / m) / m).clamp_min(0)
    invstd = (var + EPS) ** -0.5
    scale = gamma.double() * invstd
    out = dict(mean=mean, var=var, invstd=invstd, scale=scale, shift=beta.double() - mean * scale,
               running_mean=(1 - MOM) * rm.double() + MOM * mean, running_var=(1 - MOM) * rv.double() + MOM * var * m / (m - 1))
    return {k: v.float() for k, v in out.items()}


def _chain(p, dt):
    """the head forward and backward stage by stage in dtype `dt`: {stage: (value, float64 restatement of that stage from the chain's own upstream
    tensors, bar)}.  In float64 value and restatement coincide: that chain IS the restatement."""
    f = lambda k: p[k].to(dt)                                                   # noqa: E731
    r = lambda k: p[k].to(dt).double()                                          # noqa: E731  (the operand as the chain holds it)
    out = {}

    def fma(z, a, b):                                                           # one rounding, as the kernel's fmaf (f32 products are exact in float64)
        return (z.double() * a.double() + b.double()).to(dt)

    def put(name, got, ref_bar):
        out[name] = (got, ref_bar[0], ref_bar[1])
        return got

    def stats(i, z, gk, bk, rmk, rvk):
        ref = H.bn_stats(z.double(), r(gk), r(bk), EPS, MOM, r(rmk), r(rvk))
        got = {k: v[0] for k, v in ref.items()} if dt == torch.float64 else _stats32(z, f(gk), f(bk), f(rmk), f(rvk))
        for k in ref:
            put(f"{k}{i}", got[k], ref[k])
        return got

    def bwd(i, g, y, z, st, gk, s):
        ref = H.bn_relu_backward(g.double(), y.double(), z.double(), st["mean"].double(), st["invstd"].double(), r(gk), s, False)
        dy = s * g * (y > 0)
        xhat = (z - st["mean"]) * st["invstd"]
        s1, s2 = dy.sum(0), (dy * xhat).sum(0)
        put(f"s1_{i}", s1, ref["s1"])
        put(f"s2_{i}", s2, ref["s2"])
        return put(f"dz{i}", f(gk) * st["invstd"] * ((dy - s1 / M) - xhat * (s2 / M)), ref["dz"])

    X0 = H.unfold_rows(f("t"), N, h, w)
    z1 = put("z1", X0 @ f("W1").T, H.conv(X0.double(), r("W1"), "fp32"))
    st1 = stats(1, z1, "g1", "b1", "rm1", "rv1")
    y1 = put("y1", torch.relu(fma(z1, st1["scale"], st1["shift"])), H.bn_relu_drop(z1.double(), st1["scale"].double(), st1["shift"].double(), None, 0, False))
    z2 = put("z2", y1 @ f("W2").T, H.conv(y1.double(), r("W2"), "fp32"))
    st2 = stats(2, z2, "g2", "b2", "rm2", "rv2")
    y2 = put("y2", torch.relu(fma(z2, st2["scale"], st2["shift"])) * p["keep"].to(dt) * 2,
             H.bn_relu_drop(z2.double(), st2["scale"].double(), st2["shift"].double(), p["keep"], P, False))
    put("rows", y2 @ f("W3").T + f("bias"), H.conv(y2.double(), r("W3"), "fp32", r("bias")))
    d = f("d_rows")
    put("d_bias", d.sum(0), H.col_sums(d.double()))
    put("dW_cls", d.T @ y2, H.wgrad(y2.double(), d.double(), "fp32"))
    d_y2 = put("d_y2", d @ f("W3"), H.dgrad(d.double(), r("W3"), "fp32"))
    dz2 = bwd(2, d_y2, y2, z2, st2, "g2", 2.0)
    put("dW_fov2", dz2.T @ y1, H.wgrad(y1.double(), dz2.double(), "fp32"))
    d_y1 = put("d_y1", dz2 @ f("W2"), H.dgrad(dz2.double(), r("W2"), "fp32"))
    dz1 = bwd(1, d_y1, y1, z1, st1, "g1", 1.0)
    put("dW_fov", dz1.T @ X0, H.wgrad(X0.double(), dz1.double(), "fp32"))
    put("d_t", H.fold_rows(dz1 @ f("W1"), N, h, w), H.dgrad3(dz1.double(), r("W1"), N, h, w, "fp32"))
    return out


@pytest.fixture(scope="module")
def problem():
    return _problem()


def _close(a, b, what):
    assert float((a - b).abs().max()) <= 1e-10 * max(1.0, float(b.abs().max())), what


def test_restatement_equals_float64_autograd(problem):
    p = problem
    nchw = lambda r: r.view(N, h, w, -1).permute(0, 3, 1, 2)                    # noqa: E731
    t = nchw(p["t"]).clone().requires_grad_(True)
    W = {"conv_fov": p["W1"].view(C, IC, 3, 3).clone(), "conv_fov2": p["W2"].view(C, C, 1, 1).clone(), "cls_conv": p["W3"].view(NC, C, 1, 1).clone(),
         "cls_bias": p["bias"].clone()}
    bn = {"bn_fov": (p["g1"].clone(), p["b1"].clone()), "bn_fov2": (p["g2"].clone(), p["b2"].clone())}
    leaves = list(W.values()) + [x for pair in bn.values() for x in pair]
    for x in leaves:
        x.requires_grad_(True)
    out = H.restate_head(t, W, bn, nchw(p["keep"]), P, EPS)
    out.backward(nchw(p["d_rows"]))
    c = {k: v[0] for k, v in _chain(p, torch.float64).items()}
    _close(c["rows"], out.detach().permute(0, 2, 3, 1).reshape(M, NC), "rows")
    _close(c["d_t"], t.grad.permute(0, 2, 3, 1).reshape(M, IC), "d_t")
    for name, got in (("conv_fov", c["dW_fov"]), ("conv_fov2", c["dW_fov2"]), ("cls_conv", c["dW_cls"]), ("cls_bias", c["d_bias"])):
        _close(got, W[name].grad.reshape(got.shape), name)
    for i, name in ((1, "bn_fov"), (2, "bn_fov2")):
        _close(c[f"s2_{i}"], bn[name][0].grad, name + ".weight")
        _close(c[f"s1_{i}"], bn[name][1].grad, name + ".bias")
    # the running statistics after one step of the module the reference builds
    for i, z in ((1, c["z1"]), (2, c["z2"])):
        m = nn.BatchNorm2d(C, eps=EPS, momentum=MOM).double().train()
        m.running_mean.copy_(p[f"rm{i}"])
        m.running_var.copy_(p[f"rv{i}"])
        m(nchw(z))
        _close(c[f"running_mean{i}"], m.running_mean, "running_mean")
        _close(c[f"running_var{i}"], m.running_var, "running_var")
        assert int(m.num_batches_tracked) == 1


def test_float32_chain_passes_every_bar(problem):
    worst = {}
    for name, (got, ref, bar) in _chain(problem, torch.float32).items():
        ok, ratio = H.inside(got, ref, bar)
        worst[name] = round(ratio, 3)
        assert ok, (name, ratio)
    print("max err / bar per stage:", worst)
    assert len(worst) == 32


def test_composed_bars_hold_the_float32_chain_end_to_end(problem):
    """H.chain from the INPUTS only: its references are the float64 chain, and its composed bars hold every end result of the float32 chain.
    They are worst-case radii carried through three products and two normalisations and come out WIDE (printed: up to several times the value
    for d_t on this problem): they bound, they do not discriminate — a dropped s1 term stays inside them.  The stage bars above are the sharp ones."""
    p = problem
    r = lambda k: p[k].float().double()                                         # noqa: E731
    comp = H.chain(r("t"), {"conv_fov": r("W1"), "conv_fov2": r("W2"), "cls_conv": r("W3")}, r("bias"), {1: (r("g1"), r("b1")), 2: (r("g2"), r("b2"))},
                   p["keep"], r("d_rows"), N, h, w, "fp32", EPS, P)
    c32 = {k: v[0] for k, v in _chain(p, torch.float32).items()}
    names = {"rows": "rows", "d_bias": "d_bias", "dW_cls_conv": "dW_cls", "dW_conv_fov2": "dW_fov2", "dW_conv_fov": "dW_fov", "d_t": "d_t",
             "d_beta1": "s1_1", "d_gamma1": "s2_1", "d_beta2": "s1_2", "d_gamma2": "s2_2"}
    assert set(comp) == set(names)
    worst = {}
    for k, k32 in names.items():
        ref, bar = comp[k]
        ok, worst[k] = H.inside(c32[k32], ref, bar)
        assert ok, (k, worst[k])
        print(f"{k}: max composed bar {float(bar.max()):.2e} at max |ref| {float(ref.abs().max()):.2e}")
    print("end to end, max err / composed bar:", {k: round(v, 4) for k, v in worst.items()})


# ------------------------------------------------------------------------------------------------------------------ planted defects
def _stat_rows(dt=torch.float32):
    """[416, 16] rows of unit spread: column 0 has mean 64 std (the cancellation case), column 1 is constant"""
    x = _rand((416, 16), 21, 3 ** 0.5)
    x[:, 0] += 64.0
    x[:, 1] = 0.375
    return x.to(dt)


def _stat_args():
    return _rand((16,), 22, 0.5).float() + 1, _rand((16,), 23, 0.2).float(), _rand((16,), 24, 0.2).float(), _rand((16,), 25, 0.5).float() + 1


def test_stats_pass_and_defects_fail():
    x = _stat_rows()
    gamma, beta, rm, rv = _stat_args()
    ref = H.bn_stats(x.double(), gamma.double(), beta.double(), EPS, MOM, rm.double(), rv.double())
    got = _stats32(x, gamma, beta, rm, rv)
    for k, (r, bar) in ref.items():
        assert H.inside(got[k], r, bar)[0], k
    assert float(got["var"][1]) == 0.0 and float(got["invstd"][1]) == float(torch.tensor(EPS ** -0.5).float())
    # the variance as E[x^2] - mean^2 in f32: the offset column leaves its bar (u mean^2 = 4096 u var), the centred ones need not
    naive = (x * x).mean(0) - x.mean(0) ** 2
    r, bar = ref["var"]
    assert float((naive.double() - r).abs()[0]) > float(bar[0])
    naive_invstd = (naive.clamp_min(0) + EPS) ** -0.5
    assert not H.inside(naive_invstd[:1], ref["invstd"][0][:1], ref["invstd"][1][:1])[0]
    # the biased variance in the running update
    biased = ((1 - MOM) * rv.double() + MOM * got["var"].double()).float()
    assert not H.inside(biased, *ref["running_var"])[0]
    # eps outside the square root
    outside = (1.0 / (got["var"].double().sqrt() + EPS)).float()
    assert not H.inside(outside[2:], ref["invstd"][0][2:], ref["invstd"][1][2:])[0]


def test_backward_defects_fail():
    z = _rand((416, 16), 31, 3 ** 0.5).float()
    g = _rand((416, 16), 32).float()
    gamma, beta, _rm, _rv = _stat_args()
    st = _stats32(z, gamma, beta, _rm, _rv)
    keep = synth.dropout_keep(416, 16, 5, P)
    pre = torch.relu(z * st["scale"] + st["shift"])
    y = pre * keep * 2
    ref = H.bn_relu_backward(g.double(), y.double(), z.double(), st["mean"].double(), st["invstd"].double(), gamma.double(), 2.0, False)

    def dz(s=2.0, gate=y, use_s1=True, use_s2=True):
        dy = s * g * (gate > 0)
        xhat = (z - st["mean"]) * st["invstd"]
        s1, s2 = dy.sum(0), (dy * xhat).sum(0)
        return gamma * st["invstd"] * ((dy - (s1 / 416 if use_s1 else 0)) - xhat * (s2 / 416 if use_s2 else 0)), s1, s2

    good, s1, s2 = dz()
    assert H.inside(good, *ref["dz"])[0] and H.inside(s1, *ref["s1"])[0] and H.inside(s2, *ref["s2"])[0]
    for kw in (dict(use_s1=False), dict(use_s2=False), dict(s=1.0), dict(gate=pre)):
        assert not H.inside(dz(**kw)[0], *ref["dz"])[0], kw
    assert not H.inside(dz(s=1.0)[1], *ref["s1"])[0] and not H.inside(dz(gate=pre)[2], *ref["s2"])[0]


# ------------------------------------------------------------------------------------------------------------------ past 16384 rows
# 16420 rows: 457 chunks of 36 rows, the last of 4 — four batches of 128 partials in the finish, depth 13.  31360 rows (N = 10 at 56 x 56):
# 490 chunks of 64 rows, depth 20.  The GPU cases of tests/test_gpu_seg_head.py run these geometries; here the bars are judged at them.
BIG = {16420: (36, 457, 4, 13), 31360: (64, 490, 64, 20)}


def _big_rows(m_, seed):
    """[m_, 16] f32 rows of unit spread: column 0 has mean 64 std, column 1 is constant"""
    x = _rand((m_, 16), seed, 3 ** 0.5)
    x[:, 0] += 64.0
    x[:, 1] = 0.375
    return x.float()


def _bwd32(g, y, z, st, gamma, s, chunks=None):
    """wseg_bn_relu_backward's arithmetic in f32: per chunk the f32 sums of dy and dy * xhat, added in float64, m1 / m2 / k rounded to f32, dz in
    f32.  chunks: add only the first so many partials (a planted fault)"""
    m_, R = z.shape[0], H.rows_per_chunk(z.shape[0])
    dy = s * g * (y > 0)
    xhat = (z - st["mean"]) * st["invstd"]
    t2 = dy * xhat
    S1, S2 = torch.zeros(z.shape[1], dtype=torch.float64), torch.zeros(z.shape[1], dtype=torch.float64)
    for k, r0 in enumerate(range(0, m_, R)):
        if chunks is not None and k >= chunks:
            break
        S1 += dy[r0:r0 + R].sum(0).double()
        S2 += t2[r0:r0 + R].sum(0).double()
    m1, m2, kk = (S1 / m_).float(), (S2 / m_).float(), gamma * st["invstd"]
    return dict(s1=S1.float(), s2=S2.float(), dz=kk * ((dy - m1) - xhat * m2))


def _worst(got, ref):
    out = {}
    for k, (r, bar) in ref.items():
        ok, out[k] = H.inside(got[k], r, bar)
        assert ok, (k, out[k])
    return {k: round(v, 3) for k, v in out.items()}


@pytest.mark.parametrize("m_", list(BIG))
def test_f32_evaluations_pass_the_bars_past_16384_rows(m_):
    assert (H.rows_per_chunk(m_), H.row_chunks(m_), m_ - (H.row_chunks(m_) - 1) * H.rows_per_chunk(m_), H.depth(m_)) == BIG[m_]
    x = _big_rows(m_, 41)
    gamma, beta, rm, rv = _stat_args()
    ref = H.bn_stats(x.double(), gamma.double(), beta.double(), EPS, MOM, rm.double(), rv.double())
    st = _stats32(x, gamma, beta, rm, rv)
    print(f"M = {m_}: bn_stats, max err / bar", _worst(st, ref))
    assert float(st["var"][1]) == 0.0 and float(st["mean"][1]) == 0.375
    # the backward on the same rows: y = relu(fma) under the p = 0.5 mask
    g = _rand((m_, 16), 42).float()
    keep = synth.dropout_keep(m_, 16, 5, P)
    y = torch.relu((x.double() * st["scale"].double() + st["shift"].double()).float()) * keep * 2
    rb = H.bn_relu_backward(g.double(), y.double(), x.double(), st["mean"].double(), st["invstd"].double(), gamma.double(), 2.0, False)
    print(f"M = {m_}: bn_relu_backward, max err / bar", _worst(_bwd32(g, y, x, st, gamma, 2.0), rb))


@pytest.mark.parametrize("defect", ["tail_is_full", "first_batch_only", "reduce_in_32_rows"])
def test_planted_size_defects_fail(defect):
    m_ = 16420
    x = _big_rows(m_, 41)
    gamma, beta, rm, rv = _stat_args()
    ref = H.bn_stats(x.double(), gamma.double(), beta.double(), EPS, MOM, rm.double(), rv.double())
    got = _stats32(x, gamma, beta, rm, rv, defect=defect)
    fails = {k: not H.inside(got[k], r, bar)[0] for k, (r, bar) in ref.items()}
    ratio = {k: round(H.inside(got[k], r, bar)[1], 1) for k, (r, bar) in ref.items()}
    print(defect, "max err / bar", ratio)
    assert fails["mean"] and fails["var"] and fails["invstd"] and fails["shift"], (defect, ratio)      # a wrong count or a lost partial moves both moments
    # ... on every column that has a spread; the constant column stays exact under a wrong count (every difference is 0)
    r, bar = ref["mean"]
    off = (got["mean"].double() - r).abs() > bar
    assert bool(off[2:].all()) and bool(off[0]), (defect, off)


def test_backward_sums_that_stop_after_the_first_batch_fail():
    m_ = 16420
    x = _big_rows(m_, 41)
    gamma, beta, rm, rv = _stat_args()
    st = _stats32(x, gamma, beta, rm, rv)
    g = _rand((m_, 16), 42).float()
    y = torch.relu((x.double() * st["scale"].double() + st["shift"].double()).float())
    rb = H.bn_relu_backward(g.double(), y.double(), x.double(), st["mean"].double(), st["invstd"].double(), gamma.double(), 1.0, False)
    got = _bwd32(g, y, x, st, gamma, 1.0, chunks=128)
    assert not H.inside(got["s1"], *rb["s1"])[0] and not H.inside(got["s2"], *rb["s2"])[0] and not H.inside(got["dz"], *rb["dz"])[0]


def test_keep_factor_that_is_no_power_of_two():
    """p = 0.25: y = relu(fma(z, scale, shift)) * f32(4/3) in f32 — the fma's rounding, the factor's own and the product's: 3 u |y|, under the
    2 x 2 u of H.bn_relu_drop.  A factor of 2 (p = 0.5's) or 1 (the mask without the scale) leaves it."""
    m_, p = 1311, 0.25
    z = _big_rows(m_, 43)
    gamma, beta, rm, rv = _stat_args()
    st = _stats32(z, gamma, beta, rm, rv)
    keep = synth.dropout_keep(m_, 16, 7, p)
    assert abs(float(keep.double().mean()) - 0.75) <= 4 * math.sqrt(0.1875 / keep.numel())
    pre = torch.relu((z.double() * st["scale"].double() + st["shift"].double()).float())
    factor = torch.tensor(1.0) / (torch.tensor(1.0) - torch.tensor(p))              # f32, as the launch function computes it
    assert factor.dtype == torch.float32 and float(factor) != 4.0 / 3.0
    ref, bar = H.bn_relu_drop(z.double(), st["scale"].double(), st["shift"].double(), keep, p, False)
    ok, ratio = H.inside(pre * keep * factor, ref, bar)
    print(f"p = 0.25 in f32: max err / bar {ratio:.3f}")
    assert ok and bool((pre * keep * factor)[~keep].eq(0).all())
    for wrong in (2.0, 1.0):
        assert not H.inside(pre * keep * wrong, ref, bar)[0], wrong
    assert not H.inside(pre * factor, ref, bar)[0]                                   # nothing dropped


# ------------------------------------------------------------------------------------------------------------------ the dropout mask
KEYS = (0, 1, 0x9E3779B1)
SHAPES = ((35, 512), (416, 512), (1311, 512))


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_dropout_mask_is_balanced(shape):
    m_, c_ = shape
    n = m_ * c_
    for key in KEYS:
        keep = synth.dropout_keep(m_, c_, key, P)
        assert keep.dtype == torch.bool and tuple(keep.shape) == shape
        assert torch.equal(keep, synth.dropout_keep(m_, c_, key, P))              # deterministic
        k = keep.double()
        overall = abs(float(k.mean()) - 0.5) / math.sqrt(0.25 / n)
        cols = float((k.mean(0) - 0.5).abs().max()) / math.sqrt(0.25 / m_)
        rows = float((k.mean(1) - 0.5).abs().max()) / math.sqrt(0.25 / c_)
        print(f"{shape} key {key:#x}: overall {overall:.2f} sigma, columns {cols:.2f}, rows {rows:.2f}")
        assert overall <= 4 and cols <= 5 and rows <= 5


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_consecutive_keys_are_independent(shape):
    m_, c_ = shape
    for key in KEYS:
        a = synth.dropout_keep(m_, c_, key, P).view(-1)
        b = synth.dropout_keep(m_, c_, (key + 1) & 0xFFFFFFFF, P).view(-1)
        for shift in range(-2, 3):
            x, y = (a[shift:], b[:b.numel() - shift]) if shift >= 0 else (a[:shift], b[-shift:])
            agree = float((x == y).double().mean())
            assert abs(agree - 0.5) <= 4 * math.sqrt(0.25 / x.numel()), (key, shift, agree)


def test_dropout_mask_restates_the_formula():
    """element by element in Python integers, as the kernel's comment states it"""
    def mix(v):
        for _ in range(2):
            v ^= v >> 16
            v = (v * 0x45D9F3B) & 0xFFFFFFFF
        return v ^ (v >> 16)

    keep = synth.dropout_keep(5, 8, 0x9E3779B1, 0.5)
    for i in range(40):
        u = mix((mix(i) + 0x9E3779B1) & 0xFFFFFFFF) >> 8
        assert bool(keep.view(-1)[i]) == (u * 2.0 ** -24 >= 0.5)
    assert float(synth.dropout_keep(64, 512, 3, 0.3).double().mean()) == pytest.approx(0.7, abs=4 * math.sqrt(0.21 / (64 * 512)))


# ------------------------------------------------------------------------------------------------------------------ refusals, geometry
def test_cpu_tensors_are_refused():
    from wseg_amd import seg_head
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        seg_head.seg_head(None, torch.zeros(1, 4096, 2, 2), 0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        seg_head.seg_head_forward(None, torch.zeros(4, 4096), 1, 2, 2, 0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        seg_head.seg_head_backward(dict(eng=None, dt=0, N=1, h=2, w=2), torch.zeros(4, 24))


def test_net_forward_still_refuses_training_mode():
    from wseg_amd.deeplabv1_resnet38 import Net
    net = Net(precision="fp32").train()
    assert net.bn_fov.momentum == net.bn_fov2.momentum == MOM and net.bn_fov.training and not net.backbone.bn7.training
    for call in (net.forward, net.coarse_logits):
        with pytest.raises(RuntimeError, match="inference-only"):
            call(torch.zeros(1, 3, 16, 16))


def test_every_backward_launch_is_planned_in_every_mode():
    from wseg_amd import _lib as L, seg_head
    for dt in (L.F32, L.BF16, L.F32X3):
        for (n_, h_, w_) in ((1, 5, 7), (2, 13, 16), (1, 28, 31), (10, 56, 56)):
            for epi1 in (False, True):
                launches = seg_head.backward_launches(n_, h_, w_, dt, epi1)
                assert list(launches) == ["wgrad_cls_conv", "dgrad_cls_conv", "wgrad_conv_fov2", "dgrad_conv_fov2", "wgrad_conv_fov", "dgrad_conv_fov"]
                for name, kw in launches.items():
                    kw = dict(kw)
                    if kw.get("epi") == 1:
                        kw.update(scale=64, mask=64)
                    plan = (L.wgrad_plan if name.startswith("wgrad") else L.conv_plan)(**kw)
                    assert plan.family > 0 and plan.nwg > 0, (name, plan)


def test_chunk_geometry_matches_the_workspace():
    from wseg_amd import _lib as L
    for m_ in (2, 32, 33, 35, 416, 1311, 16384, 16385, 31360):
        assert H.workspace_chunks(L.bn_stats_workspace_bytes(m_, 512), 512) == H.row_chunks(m_), m_
    assert H.row_chunks(32) == 1 and H.row_chunks(35) == 2 and H.row_chunks(31360) == 490 and H.depth(31360) == 20
    assert L.bn_stats_workspace_bytes(0, 512) == -1 and L.bn_stats_workspace_bytes(8, 12) == -1
