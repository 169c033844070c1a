"""Float64 references, derived error bars, float32 CPU emulations, planted defects and the case tables of the AffinityNet inference kernels
(csrc/affinity.hip: wseg_aff_pairs, wseg_aff_to_dense, wseg_rw_prepare, wseg_random_walk, wseg_rw_pool, wseg_rw_finish).  TEST INFRASTRUCTURE,
no tests here: tests/test_aff_infer_bars_host.py judges the bars on the CPU, tests/test_gpu_aff_infer_kernels.py judges the kernels with them.

Geometry: wseg_amd.resnet38_aff.pair_offsets / indices_of_pairs (pinned to the reference's index arrays by tests/test_aff_host.py).  The
references address pixels through those index arrays; the emulations compute coordinates the way the kernels do, so the two are written
independently.  Everything is numpy; a reference takes its inputs AS STORED (f32 values, bf16 inputs as their bf16 values: the kernel's
widening of bf16 is exact).

How the bars are set (the convention of tests/f64_bars.py: from the kernel's arithmetic, SAFETY = 2 on every error term, never fitted to a
run).  u = U32 = 2^-24, first order in u.
  pairs     aff = expf(-(s / C)), s the |diff| sum of one wave.  The arithmetic is that of aff_loss.hip's forward, so the bar is the one derived
            in tests/aff_loss_f64.py (N_SUM = 14 roundings on a path of the sum, one more for s / C, expf within EXP_ULP):
            bar = aff ((N_SUM + 1) u m + EXP_ULP), m = mean_c |ft - ff|.  Identical rows: every difference is 0, s = 0, expf(-0) = 1 exactly.
  dense     a scatter of stored values: bit equality, bar 0.
  prepare   wgt = powf(aff, beta).  HIP's math-accuracy table is not at hand here; the ROCm device library is written to the OpenCL accuracy
            table, which gives pow 16 ulp, so POW_ULP = 16 ulp = 32 u relative (THE ONE ASSUMED CONSTANT of this file), plus one quantum of
            the subnormal range (2^-149) where the power underflows.  Exact, bar 0: no edge -> 0; aff == 1 -> 1; beta == 0 -> 1 on every
            edge, powf(0, 0) included.
            rsum = 1 / S, S = 1 + the 2P slots added in sequence: the slots' own errors add up, each of the 2P additions rounds a partial sum
            <= S (non-negative terms), the division is taken as 1 ulp = 2 u:  d_S = sum d_wgt + 2P u S,  bar = rsum (d_S / S + 2 u).
  walk      per plane in the max norm, M = max |v_in|.  One step is v'_j = rsum_j (v_j + sum_k w_k v_k): a combination with non-negative
            weights that sum to 1 up to rounding, so an error already in v is carried with gain <= 1.  The step's own roundings: 2P fmas, each
            rounding a partial sum <= M / rsum_j, then the product with rsum_j: (2P + 1) u M.  After `steps` = 2^logt steps
            n = steps (2P + 1) roundings.  WORST CASE  n u M  where n u <= WALK_WORST_MAX = 1e-4 (every case up to logt = 3, and logt = 6 at
            radius 2 and 3); above it (logt = 6 at radius 4, 5, 6: n = 2880, 4416, 6976, a worst case of 1.7e-4 .. 4.2e-4 M that would hide a
            wrong low-weight slot) the 4-sigma CHAIN MODEL of tests/conv_f64.py:  (4/3) u sqrt(n) M.  ITS ASSUMPTION: the n roundings are
            independent and unbiased, each uniform within u of a quantity <= M (standard deviation u sqrt(n) M / 3, taken at 4 sigma).
            A biased fma would break it; the worst case would not.  WALK_CASES names the model of every case (`model`).
            The reference takes the same f32 wgt and rsum the kernel is given, so only the walk's own roundings are judged.
  pool      64 values added in sequence from 0 (the first addition is exact: 63 roundings of a partial sum <= sum |v|), / 64 exact:
            bar = 63 u sum |v| / 64.
  finish    scale = 1/8 and the coordinates 0.125 (o + 0.5) - 0.5 are exact in f32, so are the weights l and 1 - l (multiples of 1/16).
            fma(ly, fma(lx, p11, hx p10), hy fma(lx, p01, hx p00)), every fma written out so that all planes round alike: three products
            and three fmas, 6 roundings of quantities <= M4 = max |corner|: value bar 6 u M4.  The kernel returns only the arg-max, so a pixel is
            JUDGED when the float64 top-2 margin exceeds twice the value bar (the largest over the planes at that pixel): no rounding inside
            the bar can change the winner there, and the arg-max must agree.  The unjudged pixels are capped at FINISH_UNJUDGED_MAX = 0.5 % of
            a case, for the float64 reference alone (a condition on the inputs, checked in the host test, not a measurement of the kernel).
            Two planes that are bitwise copies go through the same arithmetic and come out bitwise equal: `v > best` keeps the lower index,
            bar 0; the margin of such a case is taken with the upper copy left out.
  composed  pool -> prepare -> walk -> finish against the float64 chain, the bars summed: the pool bar is carried through the walk with gain
            <= 1; a step's coefficients c_k = w_k rsum_j (sum 1) are off by at most rel_w + rel_r relatively (the prepare bars), which adds
            (rel_w + rel_r) M per step; then the walk's own bar.  The arg-max is judged where the margin exceeds twice (value bar + that sum).

Planted defects (variants of the emulations; `judges` of a case lists what it must see, the host test holds it to that):
  pairs    mean_ld (divisor ld, visible with ld > C), drop_group (the last 8 channels missing)
  prepare  no_diag (column sum without the 1), beta_plus1, to_plus (slots P..2P-1 from pixel j + offset), batch0 (image n reads image 0)
  walk     logt_steps (logt steps, not 2^logt), slot_minus (slot 0 reads j - o), batch0 (image n walks on image 0's weights)
  pool     count_div (divides by the number of in-image pixels; visible with a side that is no multiple of 8)
  finish   align_true (align_corners=True coordinates), last_max (the last maximum wins; visible on bitwise-equal planes)
"""
import math
from types import SimpleNamespace

import numpy as np

from tests.aff_loss_f64 import EXP_ULP, N_SUM
from tests.f64_bars import SAFETY, U32
from wseg_amd.resnet38_aff import indices_of_pairs, pair_offsets

POW_ULP = 16 * 2.0 * U32            # powf: 16 ulp (OpenCL accuracy table, to which the ROCm device library is written), 1 ulp = 2 u
F32_TINY = 2.0 ** -149              # one quantum of the f32 subnormal range
WALK_WORST_MAX = 1e-4               # n u above which the chain model replaces the walk's worst case (see the docstring)
FINISH_ROUNDINGS = 6
FINISH_UNJUDGED_MAX = 0.005
f32, f64 = np.float32, np.float64


def geo(r, h, w):
    offs = pair_offsets(r)
    ind_from, ind_to = indices_of_pairs(r, (h, w))
    return SimpleNamespace(r=r, h=h, w=w, P=len(offs), offs=offs, area=h * w, n_from=len(ind_from), ind_from=ind_from,
                           ind_to=ind_to.reshape(len(offs), -1), cw=w - 2 * (r - 1), ch=h - r + 1)


def to_bf16(x):
    """round-to-nearest-even to bf16, returned as the f32 array of those values"""
    b = np.ascontiguousarray(x, dtype=f32).view(np.uint32)
    return ((b + (((b >> 16) & 1) + 0x7FFF)) & np.uint32(0xFFFF0000)).view(f32)


def _rng(seed):
    return np.random.default_rng(seed)


def rand_aff(seed, N, g, lo=0.05):
    """affinities in [lo, 1) with exact zeros and exact ones among them"""
    rng = _rng(seed)
    a = (lo + (1 - lo) * rng.random((N, g.P, g.n_from))).astype(f32)
    k = rng.random(a.shape)
    a[k < 0.04] = 0.0
    a[k > 0.96] = 1.0
    return a


# ------------------------------------------------------------------------------------------------------------------ cases
MAPS = {2: (5, 7), 3: (8, 11), 4: (10, 13), 5: (11, 12), 6: (12, 13)}       # one map per radius
MINIMAL = {r: (r, 2 * r - 1) for r in range(2, 7)}                           # one from pixel


def _pc(name, r, hw, C, pad, dt, N, dup=False):
    c = SimpleNamespace(name=name, r=r, h=hw[0], w=hw[1], C=C, ld=C + pad, dt=dt, N=N, dup=dup, judges={"drop_group"})
    if pad:
        c.judges.add("mean_ld")
    return c


PAIR_CASES = [
    _pc("min_r2_C8_f32", 2, MINIMAL[2], 8, 0, "f32", 1),                    # one item: three idle waves in the only workgroup
    _pc("min_r3_C24_ld32_bf16_N3", 3, MINIMAL[3], 24, 8, "bf16", 3),        # 3 items
    _pc("min_r4_C448_ld456_f32_N3", 4, MINIMAL[4], 448, 8, "f32", 3),
    _pc("min_r5_C512_bf16", 5, MINIMAL[5], 512, 0, "bf16", 1),
    _pc("min_r6_C512_ld520_f32_N3", 6, MINIMAL[6], 512, 8, "f32", 3),
    _pc("5x7_r2_C448_f32", 2, MAPS[2], 448, 0, "f32", 1),
    _pc("5x7_r2_C24_ld32_bf16_N3", 2, MAPS[2], 24, 8, "bf16", 3),
    _pc("8x11_r3_C8_ld16_f32", 3, MAPS[3], 8, 8, "f32", 1),                 # 42 items: partial last workgroup
    _pc("8x11_r3_C448_ld456_bf16_N3", 3, MAPS[3], 448, 8, "bf16", 3),       # 126 items
    _pc("10x13_r4_C24_f32_N3", 4, MAPS[4], 24, 0, "f32", 3),                # 147 items
    _pc("10x13_r4_C512_ld520_bf16", 4, MAPS[4], 512, 8, "bf16", 1),         # 49 items
    _pc("11x12_r5_C448_ld456_f32_N3", 5, MAPS[5], 448, 8, "f32", 3),
    _pc("12x13_r6_C448_bf16", 6, MAPS[6], 448, 0, "bf16", 1),               # 21 items
    _pc("12x13_r6_C8_f32_N3", 6, MAPS[6], 8, 0, "f32", 3),                  # 63 items
    _pc("47x63_r5_C448_ld456_f32", 5, (47, 63), 448, 8, "f32", 1),          # the geometry of a 375x500 image
    _pc("8x11_r3_C448_dup_rows", 3, MAPS[3], 448, 0, "f32", 1, dup=True),   # pixels repeat with period 3: a third of the pairs is exactly 1
]


def _prc(name, r, hw, N, beta):
    c = SimpleNamespace(name=name, r=r, h=hw[0], w=hw[1], N=N, beta=beta, judges={"no_diag", "beta_plus1", "to_plus"})
    if N > 1 and beta > 0:                     # (beta == 0: every edge weighs 1 in every image)
        c.judges.add("batch0")
    return c


PREPARE_CASES = [_prc(f"{'min_' if m is MINIMAL else ''}{hw[0]}x{hw[1]}_r{r}_N{N}_b{beta}", r, hw, N, beta)
                 for m, r, N, beta in [(MINIMAL, 2, 1, 8), (MINIMAL, 3, 3, 1), (MINIMAL, 4, 1, 0), (MINIMAL, 5, 3, 8), (MINIMAL, 6, 1, 1),
                                       (MAPS, 2, 3, 8), (MAPS, 2, 1, 0), (MAPS, 3, 1, 8), (MAPS, 3, 3, 0), (MAPS, 4, 3, 1), (MAPS, 4, 1, 8),
                                       (MAPS, 5, 3, 8), (MAPS, 5, 1, 1), (MAPS, 6, 1, 8), (MAPS, 6, 3, 0)]
                 for hw in [m[r]]] + [_prc("47x63_r5_N1_b8", 5, (47, 63), 1, 8)]


def walk_model(P, logt):
    n = (1 << logt) * (2 * P + 1)
    return "worst" if n * U32 <= WALK_WORST_MAX else "chain"


def walk_rel(P, logt):
    """the walk's bar relative to M = max |v_in| of the plane, before SAFETY"""
    n = (1 << logt) * (2 * P + 1)
    return n * U32 if n * U32 <= WALK_WORST_MAX else 4.0 / 3.0 * U32 * math.sqrt(n)


def _wc(name, r, hw, N, planes, logt, beta=8):
    c = SimpleNamespace(name=name, r=r, h=hw[0], w=hw[1], N=N, planes=planes, logt=logt, beta=beta, judges={"logt_steps", "slot_minus"},
                        model=walk_model(len(pair_offsets(r)), logt))
    if N > 1:
        c.judges.add("batch0")
    return c


WALK_CASES = [
    _wc("5x7_r2_p21_l0", 2, MAPS[2], 1, 21, 0),                 # area 35                                   worst case
    _wc("5x7_r2_N3_p5_l6", 2, MAPS[2], 3, 5, 6),                #                                           worst case (n = 576)
    _wc("8x11_r3_N3_p1_l1", 3, MAPS[3], 3, 1, 1),               # area 88                                   worst case
    _wc("8x11_r3_p5_l6_b1", 3, MAPS[3], 1, 5, 6, beta=1),       #                                           worst case (n = 1600)
    _wc("10x13_r4_N3_p21_l3", 4, MAPS[4], 3, 21, 3),            # area 130                                  worst case
    _wc("10x13_r4_p5_l6", 4, MAPS[4], 1, 5, 6),                 #                                           chain (n = 2880)
    _wc("47x63_r5_p21_l6", 5, (47, 63), 1, 21, 6),              # area 2961, the production call            chain (n = 4416)
    _wc("47x63_r5_N3_p5_l1", 5, (47, 63), 3, 5, 1),             #                                           worst case
    _wc("64x128_r6_p5_l3", 6, (64, 128), 1, 5, 3),              # area 8192 = WSEG_RW_MAX_PLANE, 64 KiB LDS worst case
    _wc("64x128_r6_N3_p1_l6", 6, (64, 128), 3, 1, 6),           #                                           chain (n = 6976)
]


def _plc(name, H, W, src, bg=0.27, ncam=3):
    c = SimpleNamespace(name=name, H=H, W=W, dh=-(-H // 8), dw=-(-W // 8), src=src, bg=bg, ncam=ncam, judges=set())
    if H % 8 or W % 8:
        c.judges.add("count_div")
    return c


def _src(**kw):
    s = [-1] * 21
    for k, v in kw.items():
        s[int(k[1:])] = v
    return s


POOL_CASES = [
    _plc("8x8", 8, 8, _src(c1=0, c20=2)),
    _plc("5x7", 5, 7, _src(c0=1, c3=1, c7=1, c8=0)),                                    # a repeated source; src[0] is ignored (bg plane)
    _plc("93x130", 93, 130, _src(c4=0, c9=2, c20=1, c12=0)),
    _plc("64x72", 64, 72, _src(c1=2, c2=1, c3=0)),
    _plc("61x83_nocams", 61, 83, _src(), bg=0.4, ncam=0),                                # null cams, every src < 0
]


def _fc(name, planes, H, W, kind="rand"):
    c = SimpleNamespace(name=name, planes=planes, H=H, W=W, dh=-(-H // 8), dw=-(-W // 8), kind=kind, dup=None, judges=set())
    if kind == "rand" and planes > 1:
        c.judges.add("align_true")
    if kind == "dup":
        c.dup = (min(4, planes - 2), planes - 1)          # the upper plane is a bitwise copy of the lower; both hold the maximum everywhere
        c.judges.add("last_max")
    return c


FINISH_CASES = [
    _fc("p1_8x8", 1, 8, 8),
    _fc("p2_5x23_dh1", 2, 5, 23),
    _fc("p21_93x130", 21, 93, 130),
    _fc("p32_64x72", 32, 64, 72),
    _fc("p20_61x83", 20, 61, 83),
    _fc("p21_61x83_dup", 21, 61, 83, "dup"),
    _fc("p2_16x24_dup", 2, 16, 24, "dup"),
    _fc("p5_16x24_equal", 5, 16, 24, "equal"),
]

COMPOSED_CASES = [SimpleNamespace(name="75x101_r4_b8_l6", H=75, W=101, r=4, beta=8, logt=6, src=_src(c2=0, c7=1, c15=2)),
                  SimpleNamespace(name="93x130_r5_b8_l6", H=93, W=130, r=5, beta=8, logt=6, src=_src(c1=2, c12=0, c20=1))]


# ------------------------------------------------------------------------------------------------------------------ pairs
def pair_problem(c):
    """p.rows [N * area][ld] f32 (bf16 cases: bf16 values), the padding columns NaN; p.ref / p.bar [N][P][n_from] float64"""
    g = geo(c.r, c.h, c.w)
    rng = _rng(11)
    feat = (rng.random((c.N, g.area, c.C)) * 2 - 1).astype(f32)
    if c.dup:
        feat = feat[:, np.arange(g.area) % 3]
    if c.dt == "bf16":
        feat = to_bf16(feat)
    rows = np.full((c.N * g.area, c.ld), np.nan, f32)
    rows[:, :c.C] = feat.reshape(-1, c.C)
    x = feat.astype(f64)
    m = np.stack([np.abs(x[:, g.ind_to[q]] - x[:, g.ind_from]).mean(axis=2) for q in range(g.P)], axis=1)
    ref = np.exp(-m)
    return SimpleNamespace(c=c, g=g, feat=feat, rows=rows, m=m, ref=ref, bar=SAFETY * ref * ((N_SUM + 1) * U32 * m + EXP_ULP))


def emulate_pairs(p, defect=None):
    """aff_pairs_kernel in f32: 8 channels per lane added in sequence from 0, the 6-step xor butterfly over 64 lanes, expf(-(s / C))"""
    c, g = p.c, p.g
    G = c.C // 8 - (1 if defect == "drop_group" else 0)
    fc = f32(c.ld if defect == "mean_ld" else c.C)
    lane = np.arange(64)
    out = np.empty((c.N, g.P, g.n_from), f32)
    fy, fx = np.divmod(np.arange(g.n_from), g.cw)
    fx = fx + g.r - 1
    a = p.feat[:, fy * g.w + fx]
    for q, (dy, dx) in enumerate(g.offs):
        b = p.feat[:, (fy + dy) * g.w + fx + dx]
        d = np.abs(b - a).reshape(c.N, g.n_from, c.C // 8, 8)
        s = np.zeros(d.shape[:3], f32)
        for e in range(8):
            s = s + d[..., e]
        lanes = np.zeros((c.N, g.n_from, 64), f32)
        lanes[..., :G] = s[..., :G]
        for o in (32, 16, 8, 4, 2, 1):
            lanes = lanes + lanes[..., lane ^ o]
        out[:, q] = np.exp(-(lanes[..., 0] / fc))
    return out


def dense_ref(aff, g):
    """the dense matrix of one image's affinities [P][n_from]: both orientations and the unit diagonal"""
    d = np.zeros((g.area, g.area), aff.dtype)
    for q in range(g.P):
        d[g.ind_from, g.ind_to[q]] = aff[q]
        d[g.ind_to[q], g.ind_from] = aff[q]
    d[np.arange(g.area), np.arange(g.area)] = 1
    return d


# ------------------------------------------------------------------------------------------------------------------ prepare
def prepare_ref(aff, g, beta):
    """float64 wgt [N][2P][area] and rsum [N][area] of f32 affinities [N][P][n_from], their bars, and `exact` [N][2P][area]: where wgt must
    hold bit for bit"""
    N = aff.shape[0]
    a64 = aff.astype(f64)
    wgt = np.zeros((N, 2 * g.P, g.area))
    edge = np.zeros((2 * g.P, g.area), bool)
    one = np.zeros((N, 2 * g.P, g.area), bool)
    for q in range(g.P):
        for slot, at in ((q, g.ind_from), (g.P + q, g.ind_to[q])):
            wgt[:, slot, at] = a64[:, q] ** beta
            edge[slot, at] = True
            one[:, slot, at] = aff[:, q] == 1
    S = 1.0 + wgt.sum(axis=1)
    rsum = 1.0 / S
    d_w = np.where(edge, POW_ULP * wgt + F32_TINY, 0.0)
    exact = ~edge[None] | one | (beta == 0)
    d_S = d_w.sum(axis=1) + 2 * g.P * U32 * S
    return SimpleNamespace(wgt=wgt, rsum=rsum, edge=edge, exact=exact, bar_w=np.where(exact, 0.0, SAFETY * d_w),
                           bar_r=SAFETY * rsum * (d_S / S + 2 * U32))


def emulate_prepare(aff, g, beta, defect=None):
    """rw_prepare_kernel in f32, by coordinates as the kernel walks them: (wgt [N][2P][area], rsum [N][area])"""
    N = aff.shape[0]
    if defect == "batch0":
        aff = np.broadcast_to(aff[:1], aff.shape)
    fb = f32(beta + (1 if defect == "beta_plus1" else 0))
    y, x = np.divmod(np.arange(g.area), g.w)
    x_lo, x_hi = g.r - 1, g.w - g.r + 1
    wgt = np.zeros((N, 2 * g.P, g.area), f32)
    s = np.full((N, g.area), 0.0 if defect == "no_diag" else 1.0, f32)
    sgn = 1 if defect == "to_plus" else -1
    slots = [(q, y, x) for q in range(g.P)] + [(g.P + q, y + sgn * dy, x + sgn * dx) for q, (dy, dx) in enumerate(g.offs)]
    for slot, iy, ix in slots:
        ok = (iy >= 0) & (iy < g.ch) & (ix >= x_lo) & (ix < x_hi)
        src = np.where(ok, iy * g.cw + ix - x_lo, 0)
        v = np.where(ok, np.power(aff[:, slot % g.P][:, src], fb), f32(0)).astype(f32)
        wgt[:, slot] = v
        s = s + v
    with np.errstate(divide="ignore"):
        return wgt, (f32(1) / s).astype(f32)


# ------------------------------------------------------------------------------------------------------------------ walk
def walk_ref(wgt, rsum, v, g, steps):
    """`steps` stencil applications in float64, through the pair index arrays: v [N][planes][area]; wgt / rsum as the kernel is given them"""
    w, r, cur = wgt.astype(f64), rsum.astype(f64), v.astype(f64)
    for _ in range(steps):
        acc = cur.copy()
        for q in range(g.P):
            acc[:, :, g.ind_from] += cur[:, :, g.ind_to[q]] * w[:, None, q, g.ind_from]
            acc[:, :, g.ind_to[q]] += cur[:, :, g.ind_from] * w[:, None, g.P + q, g.ind_to[q]]
        cur = acc * r[:, None]
    return cur


def _fma32(a, b, c):
    """fmaf on f32 arrays: the product is exact in float64, the sum is rounded to float64 and then to f32"""
    return (a.astype(f64) * b.astype(f64) + c.astype(f64)).astype(f32)


def emulate_walk(wgt, rsum, v, g, logt, defect=None):
    """random_walk_kernel in f32: clamped neighbour addresses, weight 0 outside the stencil, the fma chain in slot order, times rsum"""
    steps = logt if defect == "logt_steps" else 1 << logt
    if defect == "batch0":
        wgt, rsum = np.broadcast_to(wgt[:1], wgt.shape), np.broadcast_to(rsum[:1], rsum.shape)
    j = np.arange(g.area)
    cur = v.astype(f32)
    for _ in range(steps):
        acc = cur
        for q, (dy, dx) in enumerate(g.offs):
            o = dy * g.w + dx
            i1, i2 = np.minimum(j + o, g.area - 1), np.maximum(j - o, 0)
            if defect == "slot_minus" and q == 0:
                i1 = i2
            acc = _fma32(cur[:, :, i1], wgt[:, None, q], acc)
            acc = _fma32(cur[:, :, i2], wgt[:, None, g.P + q], acc)
        cur = acc * rsum[:, None]
    return cur


def walk_problem(c):
    g = geo(c.r, c.h, c.w)
    aff = rand_aff(21, c.N, g, lo=0.3)
    wgt, rsum = emulate_prepare(aff, g, c.beta)
    rng = _rng(22)
    v = rng.random((c.N, c.planes, g.area)).astype(f32)
    v[:, 1::2] = v[:, 1::2] * 2 - 1                             # odd planes are signed
    v[0, 0] = f32(0.7)                                          # a plane of constants
    ref = walk_ref(wgt, rsum, v, g, 1 << c.logt)
    M = np.abs(v).max(axis=2, keepdims=True).astype(f64)
    return SimpleNamespace(c=c, g=g, aff=aff, wgt=wgt, rsum=rsum, v=v, ref=ref, bar=SAFETY * walk_rel(g.P, c.logt) * M * np.ones_like(ref))


def dense_walk64(aff, g, beta, logt, v):
    """The reference's dense formulation in float64: A^beta, column normalisation, logt squarings, v . T  (one image: aff [P][n_from],
    v [planes][area])"""
    A = dense_ref(aff.astype(f64), g) ** beta
    T = A / A.sum(axis=0, keepdims=True)
    for _ in range(logt):
        T = T @ T
    return v.astype(f64) @ T


def stencil_walk64(aff, g, beta, logt, v):
    """the same in float64 through the stencil: float64 weights and reciprocal column sums, 2^logt applications"""
    pr = prepare_ref(aff[None], g, beta)
    return walk_ref(pr.wgt, pr.rsum, v[None], g, 1 << logt)[0]


# ------------------------------------------------------------------------------------------------------------------ pool
def _full_planes(cams, src, bg, H, W, dh, dw, dtype):
    full = np.zeros((21, dh * 8, dw * 8), dtype)
    full[0, :H, :W] = f32(bg)
    for c in range(1, 21):
        if src[c] >= 0:
            full[c, :H, :W] = cams[src[c]]
    return full.reshape(21, dh, 8, dw, 8).transpose(0, 1, 3, 2, 4).reshape(21, dh, dw, 64)


def pool_ref(cams, src, bg, H, W):
    """(ref, bar) [21][dh][dw] float64: the mean of the zero-padded 8x8 blocks; plane 0 is the bg score over the image"""
    dh, dw = -(-H // 8), -(-W // 8)
    b = _full_planes(cams, src, bg, H, W, dh, dw, f64)
    return b.mean(axis=3), SAFETY * 63 * U32 * np.abs(b).sum(axis=3) / 64


def emulate_pool(cams, src, bg, H, W, defect=None):
    dh, dw = -(-H // 8), -(-W // 8)
    b = _full_planes(cams, src, bg, H, W, dh, dw, f32)
    acc = np.zeros(b.shape[:3], f32)
    for i in range(64):
        acc = acc + b[..., i]
    div = f32(64)
    if defect == "count_div":
        inside = np.zeros((dh * 8, dw * 8), f32)
        inside[:H, :W] = 1
        div = inside.reshape(dh, 8, dw, 8).sum(axis=(1, 3))[None]
    return (acc / div).astype(f32)


def pool_problem(c):
    cams = (_rng(31).random((max(c.ncam, 1), c.H, c.W)) * 2 - 0.5).astype(f32)
    ref, bar = pool_ref(cams, c.src, c.bg, c.H, c.W)
    return SimpleNamespace(c=c, cams=cams, ref=ref, bar=bar)


# ------------------------------------------------------------------------------------------------------------------ finish
def _coords(n_out, n_in, dtype, align_true=False):
    o = np.arange(n_out).astype(dtype)
    if align_true:
        s = o * dtype((n_in - 1) / (8 * n_in - 1))
    else:
        s = np.maximum(dtype(0.125) * (o + dtype(0.5)) - dtype(0.5), dtype(0))
    i0 = s.astype(np.int64)
    return i0, i0 + (i0 < n_in - 1), (s - i0).astype(dtype)


def _upsample(cam, H, W, dtype, align_true=False):
    """the interpolation expression of rw_finish_kernel in `dtype`: (values [planes][H][W], the largest |corner| per value)"""
    _planes, dh, dw = cam.shape
    y0, y1, ly = _coords(H, dh, dtype, align_true)
    x0, x1, lx = _coords(W, dw, dtype, align_true)
    ly, lx = ly[None, :, None], lx[None, None, :]
    hy, hx = dtype(1) - ly, dtype(1) - lx
    p = cam.astype(dtype)
    p00, p01, p10, p11 = (p[:, ya][:, :, xa] for ya, xa in ((y0, x0), (y0, x1), (y1, x0), (y1, x1)))
    fma = _fma32 if dtype is f32 else (lambda a, b, c: a * b + c)
    up = fma(ly, fma(lx, p11, hx * p10), hy * fma(lx, p01, hx * p00))
    return up, np.max(np.abs(np.stack([p00, p01, p10, p11])), axis=0)


def finish_ref(cam, H, W, dup=None, extra_bar=0.0):
    """float64 bilinear (align_corners=False) on the [8dh][8dw] grid cropped to [H][W]: r.arg (first maximum), r.judged [H][W] (margin >
    twice the value bar), r.up, r.bar.  dup = (a, b): plane b is a bitwise copy of plane a and is left out of the margin.  extra_bar: an
    error already in cam (per plane or scalar)."""
    up, m4 = _upsample(cam, H, W, f64)
    bar = (SAFETY * FINISH_ROUNDINGS * U32 * m4 + np.reshape(extra_bar, (-1, 1, 1))).max(axis=0)
    others = np.delete(up, dup[1], axis=0) if dup else up
    if others.shape[0] > 1:
        top = np.sort(others, axis=0)[-2:]
        judged = (top[1] - top[0]) > 2 * bar
    else:
        judged = np.ones((H, W), bool)
    return SimpleNamespace(up=up, arg=up.argmax(axis=0), judged=judged, bar=bar, unjudged=1.0 - judged.mean())


def emulate_finish(cam, H, W, defect=None):
    up, _ = _upsample(cam.astype(f32), H, W, f32, align_true=defect == "align_true")
    if defect == "last_max":
        return (up.shape[0] - 1 - up[::-1].argmax(axis=0)).astype(np.uint8)
    return up.argmax(axis=0).astype(np.uint8)


def finish_problem(c):
    rng = _rng(41)
    cam = rng.random((c.planes, c.dh, c.dw)).astype(f32)
    if c.kind == "equal":
        cam[:] = cam[0]
    if c.kind == "dup":
        a, b = c.dup
        cam[a] += f32(1.5)
        cam[b] = cam[a]
    return SimpleNamespace(c=c, cam=cam, ref=finish_ref(cam, c.H, c.W, c.dup))


# ------------------------------------------------------------------------------------------------------------------ composed
def composed_problem(c):
    """pool -> prepare -> walk -> finish in float64 with the summed bars (see the docstring): p.cam / p.bar_cam [21][area], p.fin"""
    dh, dw = -(-c.H // 8), -(-c.W // 8)
    g = geo(c.r, dh, dw)
    # three regions (left, right, bottom), each with a class of its own in the CAMs; affinities high inside a region and low across, as a
    # trained network gives them: the walk sharpens the regions, and the arg-max is close only along their borders
    rng = _rng(51)
    reg = np.where(np.arange(dh)[:, None] >= (2 * dh) // 3, 2, (np.arange(dw)[None, :] >= dw // 2).astype(np.int64))
    reg_px = np.kron(reg, np.ones((8, 8), np.int64))[:c.H, :c.W]
    cams = np.stack([0.15 * rng.random((c.H, c.W)) + 0.8 * (reg_px == k) for k in range(3)]).astype(f32)
    flat = reg.reshape(-1)
    same = flat[g.ind_to] == flat[g.ind_from][None]
    aff = np.where(same, 0.85 + 0.15 * rng.random(same.shape), 0.05 + 0.1 * rng.random(same.shape)).astype(f32)[None]
    pooled, bar_pool = pool_ref(cams, c.src, 0.27, c.H, c.W)
    pooled, bar_pool = pooled.reshape(21, -1), bar_pool.reshape(21, -1)
    pr = prepare_ref(aff, g, c.beta)
    steps = 1 << c.logt
    cam = walk_ref(pr.wgt, pr.rsum, pooled[None], g, steps)[0]
    e_pool = bar_pool.max(axis=1, keepdims=True)
    M = np.abs(pooled).max(axis=1, keepdims=True) + e_pool
    rel_c = SAFETY * POW_ULP + float((pr.bar_r / pr.rsum).max())
    bar_cam = e_pool + steps * (rel_c + 2 * g.P * F32_TINY) * M + SAFETY * walk_rel(g.P, c.logt) * M
    fin = finish_ref(cam.reshape(21, dh, dw), c.H, c.W, extra_bar=bar_cam[:, 0])
    return SimpleNamespace(c=c, g=g, dh=dh, dw=dw, cams=cams, aff=aff, pooled=pooled, bar_pool=bar_pool, cam=cam,
                           bar_cam=bar_cam * np.ones_like(cam), fin=fin)


def emulate_composed(p):
    c, g = p.c, p.g
    pooled = emulate_pool(p.cams, c.src, 0.27, c.H, c.W).reshape(1, 21, -1)
    wgt, rsum = emulate_prepare(p.aff, g, c.beta)
    cam = emulate_walk(wgt, rsum, pooled, g, c.logt)[0]
    return cam, emulate_finish(cam.reshape(21, p.dh, p.dw), c.H, c.W)
