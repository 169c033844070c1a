"""Float64 references, derived error bars, CPU emulations and the case tables of the convolution kernels (csrc/conv_igemm.hip, conv_wgrad.hip,
conv_wgrad_kernels.h, the stem of api.hip).  TEST INFRASTRUCTURE, no tests here: tests/test_conv_bars_host.py judges the bars on the CPU,
tests/test_gpu_conv_f64.py judges the kernels with them.

References.  Everything is computed by torch on the CPU in float64 from operands ALREADY ROUNDED to the storage dtype (bf16 operands are bf16
values, f32 and split-bf16 operands are f32 values), in the kernels' row layout: an activation is [rows = pixels of segment 1 then segment 2]
[channels].  conv_problem() covers forward and data gradient (stride, dilation, padding, two row segments, a second 1x1 source) with every
fused epilogue the network launches, and the stem; wgrad_problem() the weight gradient with IC_dw / OC_dw extents and accumulation onto
existing content.  Next to each reference stands its ABSOLUTE-VALUE COMPANION S = conv(|x|, |w|) (weight gradient: A = sum |x| |dy|): the
sum of the magnitudes of the products of one output, which is what accumulation error scales with.

How the bars are set (the convention of tests/f64_bars.py: from the kernel's arithmetic, SAFETY = 2 on the error terms, never fitted to a
run).  U32 = 2^-24.  A bar is  bar = ROUND(|ref| + e) + e,  e = the error of the f32 value the kernel holds before it stores.
  ROUND, storage rounding   [half_ulp]
      half a unit in the last place of the stored format at the reference's binade: bf16 2^(floor(log2 |ref|) - 8), f32
      2^(floor(log2 |ref|) - 24); the binade is taken at |ref| + e, so a value that e can push over a power of two is judged at the upper
      binade.  NO safety factor: round-to-nearest-even of a held value is exact arithmetic, and a doubled term is exactly what a truncating
      store needs to pass.  (f32 storage: the accumulator is stored as it is; the term stands for the last rounding and is negligible.)
  e, accumulation           [acc_rel]
      products of bf16 operands are exact in f32; every accumulated product costs at most one f32 rounding of a partial sum <= S:
      e_acc = n U32 S with n = K = IC KH KW (+ IC2 with two sources) roundings; f32 operands (v_mfma_f32_16x16x4_f32, the stem's fma
      chain): the same count.  Split-bf16 accumulates three products per element: n = 3 K.
      This is the worst case and holds for any summation order inside or between MFMAs.  Above n = N_CHAIN = 1500 roundings it exceeds half
      a bf16 ulp of a typical output and would hide the storage rounding, so there the 4-sigma chain model of tests/test_gpu_crf.py stands in:
      e_acc = (4/3) U32 sqrt(n) S.  ITS ASSUMPTION: the n roundings are independent and unbiased, each uniform within U32 of a partial sum
      that grows linearly to at most S (standard deviation U32 sqrt(n) S / 3, taken at 4 sigma).  A biased accumulator (truncation inside the
      matrix unit) would break it; the worst case would not.  The cases with n <= 1500 carry no such assumption and are the ones that judge
      rounding and scale (`judges` of every case).
  e, split-bf16 (WSEG_F32X3) [X3_MISSING]
      x = hi + lo + r with hi = RNE_bf16(x), lo = RNE_bf16(x - hi) (split_bf16x8 of common.h for the activations, wseg_pack_x3 of api.hip
      for the weights: the same two statements), so |lo| <= 2^-9 |x| and |r| <= 2^-9 |lo| <= 2^-18 |x|.  The kernels add hi.hi + lo.hi + hi.lo;
      x y minus that is lo.lo + r y + (hi + lo) r_y, at most 3 2^-18 |x y| to first order: e_x3 = 3 2^-18 S.
  e, weight gradient        [wgrad_bar]
      the accumulation runs over the pixels: one rounding per accumulated product and one per split-K / pair-grid atomic,
      n = n_pix + splits (split-bf16: 3 n_pix + splits, plus 3 2^-18 A), e = acc_rel(n) A: the worst case n U32 A up to N_CHAIN roundings,
      the chain model above it (the worst case of the joint grid's 33792 pixels, 4e-3 A, is half of max |dw| and judges nothing).
      Content already in dw takes part in the `splits` atomics only: + splits U32 |prior|.  Stored as f32.
  e, epilogues              [epilogue]
      e is carried through the epilogue's f32 operations in the order the kernels apply them (epilogue_image / wave_local_epilogue_batch):
      an addition of a residual adds one rounding U32 |result|; v scale + shift is an fma or a product and a sum: two roundings,
      U32 (|v scale| + |result|), and e is multiplied by |scale|; the dropout factor multiplies value and e and is counted as one rounding;
      ReLU, relu_lt and the mask are exact and do not amplify (gain <= 1).  `out2` is computed from the UNROUNDED sum: its e starts from
      the e of the held value, never from the bar of `out`, and it gets the storage rounding of its own magnitude.
      ELU (x > 0 ? x : expm1f(x)): gain <= 1 on x <= 0, plus expm1f's documented 1 ulp = 2 U32 |result| (HIP math API).
  Every error term carries SAFETY; the storage rounding does not.
No exclusions: every element of every output is compared, there is no near-tie rule and no share of elements left out.

CPU emulations (emulate_conv / emulate_wgrad): the honest kernel is torch's float32 convolution of the same operands (split-bf16: the three
float32 convolutions of the split parts), the epilogue in float32, and the kernel's store (RNE to bf16).  The planted defects are the ones
tests/test_gpu_conv.py's fitted bars let through: `trunc` a truncating bf16 store, `scale` every result times 1 + 2^-8, `drop_product` one
(tap, channel) product missing from every output, `drop_lohi` the lo.hi term of split-bf16 missing, `drop_pixel` one output pixel's
contribution missing from the weight gradient.  What a case can see is its `judges`: trunc needs a bf16 store and n <= N_CHAIN (beside
e_acc = 2 n U32 S of a long chain a missing half ulp is no longer visible; f32 storage has no storage rounding to get wrong); scale and
drop_product are seen by every case, drop_lohi by every split-bf16 forward / data-gradient case; what a weight-gradient case sees follows
from its pixel count (_wcase).
"""
import math
from types import SimpleNamespace

import torch
import torch.nn.functional as F

from tests.f64_bars import SAFETY, U32

N_CHAIN = 1500                      # roundings above which the chain model replaces the worst case (see the docstring)
X3_MISSING = 3.0 * 2.0 ** -18       # what hi.hi + lo.hi + hi.lo leaves out, relative to S
EXPM1_ULP = 2.0 * U32               # expm1f: 1 ulp
SIG_BITS = {"bf16": 8, "f32": 24}   # significand bits of a storage format
TORCH_DT = {"bf16": torch.bfloat16, "f32": torch.float32, "x3": torch.float32}
DEFECT_SCALE = 1.0 + 2.0 ** -8


def rand(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(shape, generator=g) * 2 - 1) * scale


def rows(t):       # [N, C, H, W] -> [N*H*W, C]
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1])


def half_ulp(mag, store):
    """half a unit in the last place of `store` at the binade of mag (>= 0, float64)"""
    _m, ex = torch.frexp(mag.clamp_min(2.0 ** -126))              # mag = m 2^ex, m in [0.5, 1): floor(log2 mag) = ex - 1
    return torch.ldexp(torch.ones_like(mag), ex - 1 - SIG_BITS[store])


def acc_rel(n):
    """accumulation error of n f32 roundings, relative to the sum of magnitudes (before SAFETY)"""
    return n * U32 if n <= N_CHAIN else 4.0 / 3.0 * U32 * math.sqrt(n)


def stored_bar(ref, e, store):
    return half_ulp(ref.abs() + e, store) + e


def _osz(h, k, s, d, pad):
    return (h + 2 * pad - d * (k - 1) - 1) // s + 1


# ------------------------------------------------------------------------------------------------------------------ cases
def _case(name, kind, dt, N, H, W, Cin, Cout, k, s, d, fams, opset="plain", seg2=None, IC2=0, ld_in2=0, store=None, perm=None):
    """kind fwd / dgrad of the convolution Cin -> Cout on an H x W input.  fams: bm_hint values to run (0 = the planner's choice)."""
    c = SimpleNamespace(name=name, kind=kind, dt=dt, N=N, H=H, W=W, Cin=Cin, Cout=Cout, k=k, s=s, d=d, fams=fams, opset=opset, seg2=seg2,
                        IC2=IC2, ld_in2=ld_in2, store=store or ("bf16" if dt == "bf16" else "f32"), perm=perm or {})
    c.in_ch, c.out_ch = (Cin, Cout) if kind == "fwd" else (Cout, Cin)
    c.K = c.in_ch * k * k + IC2
    c.n_round = 3 * c.K if dt == "x3" else c.K
    c.judges = {"scale", "drop_product"}
    if c.store == "bf16" and c.n_round <= N_CHAIN:
        c.judges.add("trunc")
    if dt == "x3":
        c.judges.add("drop_lohi")
    return c


BF16_ALL = (64, 128, 224, 256, 259)
CONV_CASES = [
    # forward, bf16
    _case("fwd300", "fwd", "bf16", 2, 15, 10, 64, 256, 3, 1, 1, BF16_ALL),                   # 300 rows: one full + one partial tile at 128 / 224 / 256; K = 576
    _case("fwd_k64_s2", "fwd", "bf16", 1, 21, 19, 64, 192, 1, 2, 1, (64, 128)),             # K = 64, stride-2 1x1
    _case("fwd_3col", "fwd", "bf16", 3, 9, 9, 128, 768, 3, 1, 1, BF16_ALL),                 # 243 rows < one tile, three column tiles; K = 1152
    _case("fwd_dil4", "fwd", "bf16", 1, 12, 12, 64, 256, 3, 1, 4, BF16_ALL),                # most taps are padding
    # data gradient, bf16
    _case("dgrad_1x1_300", "dgrad", "bf16", 2, 15, 10, 256, 256, 1, 1, 1, (128, 224, 256, 259)),        # K = 256
    _case("dgrad_s2_perm", "dgrad", "bf16", 2, 12, 12, 256, 256, 3, 2, 1, (224, 256), perm={224: 1, 256: 1}),   # rows in parity-class order
    _case("dgrad_s2_odd", "dgrad", "bf16", 1, 13, 11, 256, 256, 3, 2, 1, (128, 224, 256), perm={224: 0, 256: 0}),
    # f32 and split-bf16
    _case("fwd300_f32", "fwd", "f32", 2, 15, 10, 64, 256, 3, 1, 1, (64, 128)),
    _case("fwd300_x3", "fwd", "x3", 2, 15, 10, 64, 256, 3, 1, 1, (64, 128, 224, 256)),
    _case("dgrad_1x1_f32", "dgrad", "f32", 2, 15, 10, 256, 256, 1, 1, 1, (64, 128)),
    _case("dgrad_1x1_x3", "dgrad", "x3", 2, 15, 10, 256, 256, 1, 1, 1, (64, 128, 224, 256)),
    # two sources (the 256-tile kernels), two row segments
    _case("two_src_1x1", "fwd", "bf16", 2, 21, 17, 192, 512, 1, 1, 1, (0, 224), opset="post_out_out2", seg2=(8, 9), IC2=192, ld_in2=256),
    _case("two_src_3x3_fwd", "fwd", "bf16", 2, 19, 16, 128, 256, 3, 1, 1, (0,), seg2=(7, 10), IC2=128),
    _case("two_src_3x3_dgrad", "dgrad", "bf16", 2, 19, 16, 256, 128, 3, 1, 1, (0,), seg2=(7, 10), IC2=128),
    # the joint grid's data gradient (with WGRAD_CASES["pair"])
    _case("pair_dgrad", "dgrad", "bf16", 2, 132, 128, 256, 256, 3, 1, 1, (0,)),
]


def epi_cases():
    """the operand sets of tests/test_gpu_conv.py (EPI_CASES: families x EPI_SETS, elu, perm_mask_post) as cases of this module, plus epi 2"""
    from tests.test_gpu_conv import EPI_CASES
    out = []
    for dt, bm, opset in EPI_CASES + [("bf16", 0, "epi2_relu"), ("bf16", 256, "epi2_relu")]:
        if opset == "perm_mask_post":
            c = _case(f"epi_{opset}_{dt}_{bm}", "dgrad", dt, 2, 12, 12, 256, 256, 3, 2, 1, (bm,), opset="epi1_mask_post_noscale", perm={bm: 1})
        else:
            big = bm in (224, 256)
            OC = (256 if bm == 259 else 152) if opset == "relu_lt_tail" else (256 if big else 128)
            c = _case(f"epi_{opset}_{dt}_{bm}", "fwd", dt, 2, 15, 10, 64, OC, 3, 1, 1, (bm,), opset=opset)
            c.w_rows = 256 if (big and OC % 256) else 0
        out.append(c)
    return out


STEM_CASES = [_case(f"stem_{st}", "fwd", "f32", 2, 37, 70, 3, 64, 3, 1, 1, (0,), opset="stem", store=st) for st in ("f32", "bf16")]


def _wcase(name, dt, N, H, W, IC, OC, k, s, d, hints, IC_dw=0, OC_dw=0):
    c = SimpleNamespace(name=name, dt=dt, N=N, H=H, W=W, IC=IC, OC=OC, k=k, s=s, d=d, hints=hints, IC_dw=IC_dw or IC, OC_dw=OC_dw or OC)
    # what the case can see, with n = the roundings of wgrad_bar and r = SAFETY acc_rel(n), the bar relative to A.  An element three sigma
    # out has |ref| = sqrt(n_pix) sigma_x sigma_dy 3 = sqrt(n_pix) and A = n_pix / 4 (uniform operands): |ref| / A = 4 / sqrt(n_pix), so a
    # scale defect shows where 2^-8 4 / sqrt(n_pix) > r.  A dropped pixel removes up to |x dy| = 1 = 4 A / n_pix: it shows where
    # 4 / n_pix > r.  A dropped lo.hi term is a random sum of n_pix terms of about 2^-10 |x dy|, some 2^-10 A / sqrt(n_pix) relative.
    pad = d * (k // 2)
    c.n_pix = N * _osz(H, k, s, d, pad) * _osz(W, k, s, d, pad)
    r = SAFETY * (acc_rel((3 if dt == "x3" else 1) * c.n_pix + 1) + (X3_MISSING if dt == "x3" else 0.0))
    c.judges = set()
    if 2.0 ** -8 * 4 / math.sqrt(c.n_pix) > r:
        c.judges.add("scale")
    if 4.0 / c.n_pix > r:
        c.judges.add("drop_pixel")
    if dt == "x3" and 2.0 ** -10 * 4 / math.sqrt(c.n_pix) > r:
        c.judges.add("drop_lohi")
    return c


WGRAD_CASES = {c.name: c for c in [
    _wcase("wg_tail320", "bf16", 2, 10, 10, 320, 320, 3, 1, 1, (128, 256)),        # 64-wide tail in both tile dimensions, partial K-tile
    _wcase("wg_dil2", "bf16", 1, 13, 11, 256, 512, 3, 1, 2, (128, 256)),
    _wcase("wg_extents", "bf16", 2, 12, 10, 256, 256, 3, 1, 1, (128, 256), IC_dw=248, OC_dw=200),
    _wcase("wg_f32", "f32", 2, 20, 20, 64, 128, 3, 1, 1, (128,)),
    _wcase("wg_x3", "x3", 2, 20, 20, 64, 128, 3, 1, 1, (128,)),
    _wcase("pair", "bf16", 2, 132, 128, 256, 256, 3, 1, 1, (0,)),
]}


# ------------------------------------------------------------------------------------------------------------------ forward / data gradient
def _linear(c, xs, x2s, w, w2, dtype):
    """rows of the linear part of case c in `dtype`: per segment conv (fwd) or its data gradient, plus the 1x1 second source"""
    pad, outs = c.d * (c.k // 2), []
    for i, x in enumerate(xs):
        if c.kind == "fwd":
            y = F.conv2d(x.to(dtype), w.to(dtype), None, c.s, pad, c.d)
        else:
            H, W = c.sizes[i]
            op = [n - ((o - 1) * c.s - 2 * pad + c.d * (c.k - 1) + 1) for n, o in ((H, x.shape[2]), (W, x.shape[3]))]
            y = F.conv_transpose2d(x.to(dtype), w.to(dtype), None, c.s, pad, op, 1, c.d)
        if x2s:
            y = y + (F.conv2d if c.kind == "fwd" else F.conv_transpose2d)(x2s[i].to(dtype), w2.to(dtype))
        outs.append(rows(y))
    return torch.cat(outs)


def conv_problem(c):
    """operands (rounded to the storage dtype), float64 reference and bar of every stored output of case c:
    p.refs = {"out": (ref, bar), "out2": (ref, bar)} in row layout, p.e0 the error of the held sum"""
    tdt = TORCH_DT[c.dt]
    c.sizes = [(c.H, c.W)] + ([c.seg2] if c.seg2 else [])
    pad = c.d * (c.k // 2)
    c.osizes = [(_osz(h, c.k, c.s, c.d, pad), _osz(w_, c.k, c.s, c.d, pad)) for h, w_ in c.sizes]
    p = SimpleNamespace(c=c)
    in_sizes = c.sizes if c.kind == "fwd" else c.osizes                  # spatial sizes of the kernel's input / output rows
    p.out_sizes = c.osizes if c.kind == "fwd" else c.sizes
    wscale = 0.3 if c.opset == "stem" else (2.0 / (c.Cin * c.k * c.k)) ** 0.5
    p.xs = [rand((c.N, c.in_ch, h, w_), 1 + i).to(tdt) for i, (h, w_) in enumerate(in_sizes)]
    p.w = rand((c.Cout, c.Cin, c.k, c.k), 30, wscale).to(tdt)
    p.x2s, p.w2 = [], None
    if c.IC2:
        p.x2s = [rand((c.N, c.IC2, h, w_), 11 + i).to(tdt) for i, (h, w_) in enumerate(in_sizes)]
        w2 = rand((c.out_ch, c.IC2, 1, 1), 31, (1.0 / c.IC2) ** 0.5).to(tdt)
        p.w2 = w2 if c.kind == "fwd" else w2.permute(1, 0, 2, 3).contiguous()      # (data gradient: the 1x1 conv out_ch -> IC2 whose gradient this is)
    p.M = sum(c.N * h * w_ for h, w_ in p.out_sizes)
    p.img = torch.cat([i * c.N + torch.arange(c.N).repeat_interleave(h * w_) for i, (h, w_) in enumerate(p.out_sizes)])   # n_glob of a row
    p.y = _linear(c, p.xs, p.x2s, p.w, p.w2, torch.float64)
    p.S = _linear(c, [x.abs() for x in p.xs], [x.abs() for x in p.x2s], p.w.abs(), None if p.w2 is None else p.w2.abs(), torch.float64)
    p.e0 = SAFETY * (acc_rel(c.n_round) + (X3_MISSING if c.dt == "x3" else 0.0)) * p.S
    p.ep = _epilogue_operands(c, p.M, tdt)
    p.refs = epilogue(p, p.y, p.e0, torch.float64)
    return p


def _epilogue_operands(c, M, tdt):
    OC, o = c.out_ch, c.opset
    ep = dict(epi=0, relu_out2=1, relu_lt=0, want_out=True, want_out2=False)
    full = lambda seed: rand((M, OC), seed).to(tdt)
    n_img = c.N * (2 if c.seg2 else 1)
    scale, shift = rand((OC,), 6) + 1.5, rand((OC,), 7)
    drop = (torch.rand(n_img, OC, generator=torch.Generator().manual_seed(8)) > 0.5).float() * 2
    if o == "post_out_out2":
        ep.update(r_post=full(4), scale=scale, shift=shift, drop=drop, want_out2=True)
    elif o == "pre_out2_only":
        ep.update(r_pre=full(5), scale=scale, shift=shift, relu_out2=0, want_out=False, want_out2=True)
    elif o == "relu_lt_tail":
        ep.update(relu_lt=128)
    elif o == "epi1_mask_post":
        ep.update(epi=1, scale=scale, mask=full(9), r_post=full(4))
    elif o == "epi1_mask_post_noscale":
        ep.update(epi=1, mask=full(9), r_post=full(4))
    elif o == "epi1_mask_drop":
        ep.update(epi=1, scale=scale, mask=full(9), drop=drop)
    elif o == "epi2_relu":
        ep.update(epi=2)
    elif o == "elu":
        ep.update(epi=3)
    elif o == "stem":
        ep.update(scale=scale, shift=shift, want_out2=True)
    else:
        assert o == "plain", o
    return ep


def epilogue(p, v, e, dtype, store_fn=None):
    """The fused epilogue of the held sums v (rows) in `dtype`, in the kernels' order of operations.  float64 with an error e: returns
    {name: (ref, bar)}; float32 with a store function: the emulation, {name: stored tensor}."""
    ep, c = p.ep, p.c
    emu = store_fn is not None
    t = lambda a: a.to(dtype)
    u = 0.0 if emu else SAFETY * U32
    e = 0.0 if emu else e
    res = {}
    if "r_pre" in ep:
        v = v + t(ep["r_pre"]); e = e + u * v.abs()
    if ep["epi"] == 0:
        if "r_post" in ep:
            v = v + t(ep["r_post"]); e = e + u * v.abs()
        if ep["relu_lt"]:
            v = torch.cat([F.relu(v[:, :ep["relu_lt"]]), v[:, ep["relu_lt"]:]], dim=1)
        if ep["want_out"]:
            res["out"] = (v, e)
        if ep["want_out2"]:
            vs = v * t(ep["scale"])
            x = vs + t(ep["shift"])
            e2 = e * t(ep["scale"]).abs() + u * (vs.abs() + x.abs())
            if ep["relu_out2"]:
                x = F.relu(x)
            if "drop" in ep:
                dr = t(ep["drop"])[p.img]
                x = x * dr; e2 = e2 * dr + u * x.abs()
            res["out2"] = (x, e2)
    elif ep["epi"] == 1:
        x = v
        if "scale" in ep:
            x = x * t(ep["scale"]); e = e * t(ep["scale"]).abs() + u * x.abs()
        if "drop" in ep:
            dr = t(ep["drop"])[p.img]
            x = x * dr; e = e * dr + u * x.abs()
        if "mask" in ep:
            keep = (ep["mask"].float() > 0).to(dtype)
            x = x * keep; e = e * keep
        if "r_post" in ep:
            x = x + t(ep["r_post"]); e = e + u * x.abs()
        res["out"] = (x, e)
    elif ep["epi"] == 2:
        res["out"] = (F.relu(v), e)
    else:
        x = torch.where(v > 0, v, torch.expm1(v))
        res["out"] = (x, e + (0.0 if emu else SAFETY * EXPM1_ULP) * x.abs())
    if emu:
        return {k: store_fn(x) for k, (x, _e) in res.items()}
    return {k: (x, stored_bar(x, e_, c.store)) for k, (x, e_) in res.items()}


def split_bf16(x):
    """(hi, lo) of split_bf16x8 / wseg_pack_x3: hi = RNE_bf16(x), lo = RNE_bf16(x - hi), as float32"""
    hi = x.float().to(torch.bfloat16).float()
    return hi, (x.float() - hi).to(torch.bfloat16).float()


def store(x32, fmt, trunc=False):
    """the kernel's store of a held f32 value as a float64 tensor: RNE to bf16 (or, the planted defect, truncation), f32 as it is"""
    if fmt == "f32":
        return x32.double()
    if trunc:
        return (x32.contiguous().view(torch.int32) & -65536).view(torch.float32).double()
    return x32.to(torch.bfloat16).double()


def emulate_conv(p, defect=None):
    """{name: stored output} of the honest kernel (defect None) or of one with a planted defect, on the CPU in float32"""
    c = p.c
    f = torch.float32
    if c.dt == "x3":
        parts = [split_bf16(x) for x in p.xs]
        (xh, xl), (wh, wl) = ([a for a, _b in parts], [b for _a, b in parts]), split_bf16(p.w)
        v = _linear(c, xh, [], wh, None, f) + _linear(c, xh, [], wl, None, f)
        if defect != "drop_lohi":
            v = v + _linear(c, xl, [], wh, None, f)
    else:
        v = _linear(c, p.xs, p.x2s, p.w, p.w2, f)
    if defect == "drop_product":                    # the centre tap's product of input channel 0 is missing from every output it reaches
        w1 = torch.zeros_like(p.w)
        ci = 0 if c.kind == "fwd" else slice(None)
        co = slice(None) if c.kind == "fwd" else 0
        w1[co, ci, c.k // 2, c.k // 2] = p.w[co, ci, c.k // 2, c.k // 2]
        v = v - _linear(c, p.xs, [], w1, None, f)
    if defect == "scale":
        v = v * DEFECT_SCALE
    return epilogue(p, v, None, f, store_fn=lambda x: store(x, c.store, trunc=defect == "trunc"))


# ------------------------------------------------------------------------------------------------------------------ weight gradient
def wgrad_problem(c):
    """x, dy (storage dtype, NCHW), the float64 weight gradient [OC][taps][IC] and its companion A = sum |x| |dy|"""
    tdt = TORCH_DT[c.dt]
    pad = c.d * (c.k // 2)
    p = SimpleNamespace(c=c, pad=pad, OH=_osz(c.H, c.k, c.s, c.d, pad), OW=_osz(c.W, c.k, c.s, c.d, pad))
    p.x = rand((c.N, c.IC, c.H, c.W), 1).to(tdt)
    p.dy = rand((c.N, c.OC, p.OH, p.OW), 3).to(tdt)
    p.n_pix = c.N * p.OH * p.OW
    p.ref = _wgrad(c, p.x, p.dy, torch.float64)
    p.A = _wgrad(c, p.x.abs(), p.dy.abs(), torch.float64)
    return p


def _wgrad(c, x, dy, dtype):
    g = torch.nn.grad.conv2d_weight(x.to(dtype), (c.OC, c.IC, c.k, c.k), dy.to(dtype), c.s, c.d * (c.k // 2), c.d)
    return g.permute(0, 2, 3, 1).reshape(c.OC, c.k * c.k, c.IC)[:c.OC_dw, :, :c.IC_dw]


def wgrad_bar(p, splits, prior=None):
    """bar of dw = prior + weight gradient after a launch of `splits` atomics per element (the plan's nsplit)"""
    x3 = p.c.dt == "x3"
    e = acc_rel((3 if x3 else 1) * p.n_pix + splits) * p.A + (X3_MISSING * p.A if x3 else 0.0)
    ref = p.ref
    if prior is not None:
        e = e + splits * U32 * prior.abs()
        ref = ref + prior
    return ref, stored_bar(ref, SAFETY * e, "f32")


def emulate_wgrad(p, defect=None, prior=None):
    c, f = p.c, torch.float32
    dy = p.dy.float()
    if defect == "drop_pixel":                      # one output pixel (image 0, centre) adds nothing
        dy = dy.clone()
        dy[0, :, p.OH // 2, p.OW // 2] = 0
    if c.dt == "x3":
        (xh, xl), (dh, dl) = split_bf16(p.x), split_bf16(dy)
        g = _wgrad(c, xh, dh, f) + _wgrad(c, xh, dl, f)
        if defect != "drop_lohi":
            g = g + _wgrad(c, xl, dh, f)
    else:
        g = _wgrad(c, p.x, dy, f)
    if defect == "scale":
        g = g * DEFECT_SCALE
    return (g if prior is None else g + prior.float()).double()
