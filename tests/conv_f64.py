"""Float64 references, derived error bars, CPU emulations and the case tables of the convolution kernels (csrc/conv_igemm.hip, conv_wgrad.hip,
conv_wgrad_kernels.h, the stem of api.hip).  TEST INFRASTRUCTURE, no tests here: tests/test_conv_bars_host.py judges the bars on the CPU,
tests/test_gpu_conv_f64.py judges the kernels with them.

References.  Everything is computed by torch on the CPU in float64 from operands ALREADY ROUNDED to the storage dtype (bf16 operands are bf16
values, f32 and split-bf16 operands are f32 values), in the kernels' row layout: an activation is [rows = pixels of segment 1 then segment 2]
[channels].  conv_problem() covers forward and data gradient (stride, dilation, padding, two row segments, a second 1x1 source) with every
fused epilogue the network launches, and the stem; wgrad_problem() the weight gradient with IC_dw / OC_dw extents, two row segments, row
strides and column offsets of the operands, the column rotation dw_rot, a forced split and accumulation onto existing content.  Next to
each reference stands its ABSOLUTE-VALUE COMPANION S = conv(|x|, |w|) (weight gradient: A = sum |x| |dy|): the sum of the magnitudes of the
products of one output, which is what accumulation error scales with.

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
contribution missing from the weight gradient.  The weight gradient's address paths (conv_wgrad_kernels.h stages its operands in three ways,
chosen by geometry) have defects of their own: `seam_pixel` the first output pixel of the second row segment takes its x window with the
first segment's width (a missed re-decode, a wrong pointer correction at the seam), `wrap_pixel` the first output pixel of image 1 takes the
window of the pixel before it (a wrong image wrap of the incremental advance), `pad_wrap` a tap past the right border reads the next row's
first pixels instead of zero (a validity test gone wrong), `drop_tail` the partial last K-tile adds nothing, `rot_off` dw's columns rotated
by dw_rot - 1.
What a case can see is its `judges`: trunc needs a bf16 store and n <= N_CHAIN (beside
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
    _case("pair_seg2_dgrad", "dgrad", "bf16", 2, 119, 125, 256, 256, 1, 1, 1, (0,), seg2=(36, 44)),   # (with WGRAD_CASES["pair_seg2"])
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


WGRAD_PK = {"bf16": 64, "f32": 32, "x3": 32}      # pixels per K-step of the weight-gradient kernels (conv_wgrad_kernels.h)
WGRAD_FEATURES = ("1x1", "stride2", "dilated", "tiny", "seam", "split8", "ctail", "extents", "rot", "views")


def _wcase(name, dt, N, H, W, IC, OC, k, s, d, hints, IC_dw=0, OC_dw=0, seg2=None, ld_x=0, ld_dy=0, x_off=0, dy_off=0, dw_rot=0, split_k=0,
           unit=None, nsplit=None, nwg=None, tiny_seg=None):
    """A weight-gradient case.  seg2 = (H2, W2): a second row segment (same N); ld_x / ld_dy / x_off / dy_off: the operand is the column
    block [off, off + channels) of rows ld wide; dw_rot: column rotation of dw; split_k: the first launch's split (0 = the planner's).
    unit / nsplit / nwg: what the plan of the first launch must report (None: not stated); tiny_seg: the segment (0 / 1) whose map is so
    small that one K-step of 64 pixels wraps more than one image (the header's rule, 64 // OW + 1 > OH)."""
    c = SimpleNamespace(name=name, dt=dt, N=N, H=H, W=W, IC=IC, OC=OC, k=k, s=s, d=d, hints=hints, IC_dw=IC_dw or IC, OC_dw=OC_dw or OC,
                        seg2=seg2, ld_x=ld_x or IC, ld_dy=ld_dy or OC, x_off=x_off, dy_off=dy_off, dw_rot=dw_rot, split_k=split_k,
                        unit=unit, nsplit=nsplit, nwg=nwg, tiny_seg=tiny_seg)
    # what the case can see, with n = the roundings of wgrad_bar and r = SAFETY acc_rel(n), the bar relative to A.  An element three sigma
    # out has |ref| = sqrt(n_pix) sigma_x sigma_dy 3 = sqrt(n_pix) and A = n_pix / 4 (uniform operands): |ref| / A = 4 / sqrt(n_pix), so a
    # scale defect shows where 2^-8 4 / sqrt(n_pix) > r.  A dropped pixel removes up to |x dy| = 1 = 4 A / n_pix: it shows where
    # 4 / n_pix > r.  A dropped lo.hi term is a random sum of n_pix terms of about 2^-10 |x dy|, some 2^-10 A / sqrt(n_pix) relative.
    # The address defects (seam_pixel, wrap_pixel, pad_wrap, drop_tail) each replace or remove the x window of at least one output pixel, and
    # rot_off moves every column: whoever sees a dropped pixel sees them, where the geometry has the feature at all.
    pad = d * (k // 2)
    c.sizes = [(H, W)] + ([seg2] if seg2 else [])
    c.osizes = [(_osz(h, k, s, d, pad), _osz(w_, k, s, d, pad)) for h, w_ in c.sizes]
    c.n_pix = sum(N * oh * ow for oh, ow in c.osizes)
    r = SAFETY * (acc_rel((3 if dt == "x3" else 1) * c.n_pix + 1) + (X3_MISSING if dt == "x3" else 0.0))
    c.judges = set()
    if 2.0 ** -8 * 4 / math.sqrt(c.n_pix) > r:
        c.judges.add("scale")
    if 4.0 / c.n_pix > r:
        c.judges.add("drop_pixel")
        if seg2 and k > 1 and seg2[1] != W:                         # (the top row of a 1x1 window is the same at any width)
            c.judges.add("seam_pixel")
        if N > 1:
            c.judges.add("wrap_pixel")
        if any((ow - 1) * s + (k - 1) * d - pad >= w_ for (_h, w_), (_oh, ow) in zip(c.sizes, c.osizes)):
            c.judges.add("pad_wrap")
        if c.n_pix % WGRAD_PK[dt]:
            c.judges.add("drop_tail")
        if dw_rot:
            c.judges.add("rot_off")
    if dt == "x3" and 2.0 ** -10 * 4 / math.sqrt(c.n_pix) > r:
        c.judges.add("drop_lohi")
    return c


def wgrad_pipe(c, hint):
    """does the run (case, tile_hint) name the 256x256 kernel"""
    return hint == 256 and c.dt == "bf16" and c.IC >= 256 and c.OC >= 256


def wgrad_features(c, hint):
    """the features of WGRAD_FEATURES a run has, from the case's attributes"""
    tile = 256 if wgrad_pipe(c, hint) else 128
    has = {"1x1": c.k == 1, "stride2": c.s == 2, "dilated": c.d > 1 and c.k > 1, "tiny": c.tiny_seg is not None, "seam": c.seg2 is not None,
           "split8": c.split_k == 8, "ctail": c.IC % tile != 0 or c.OC % tile != 0, "extents": c.IC_dw < c.IC or c.OC_dw < c.OC,
           "rot": c.dw_rot != 0, "views": c.ld_x > c.IC or c.ld_dy > c.OC}
    return {f for f, on in has.items() if on}


def _wcases(name, dts, *args, **kw):
    """one case per dtype, named name_<dtype> where there are several"""
    return [_wcase(name if len(dts) == 1 else f"{name}_{dt}", dt, *args, **kw) for dt in dts]


_OLD_WGRAD = [
    _wcase("wg_tail320", "bf16", 2, 10, 10, 320, 320, 3, 1, 1, (128, 256)),        # 64-wide tail in both tile dimensions, partial K-tile
    _wcase("wg_dil2", "bf16", 1, 13, 11, 256, 512, 3, 1, 2, (128, 256)),
    _wcase("wg_extents", "bf16", 2, 12, 10, 256, 256, 3, 1, 1, (128, 256), IC_dw=248, OC_dw=200),
    _wcase("wg_f32", "f32", 2, 20, 20, 64, 128, 3, 1, 1, (128,)),
    _wcase("wg_x3", "x3", 2, 20, 20, 64, 128, 3, 1, 1, (128,)),
    _wcase("pair", "bf16", 2, 132, 128, 256, 256, 3, 1, 1, (0,)),
]
for _c in _OLD_WGRAD:                 # (every one of them that reaches the 256x256 kernel stages with StageUnit)
    _c.unit = 1
B, BF, BFX = ("bf16",), ("bf16", "f32"), ("bf16", "f32", "x3")
# The smallest shapes at which each address path of conv_wgrad_kernels.h is still taken.  128x128 kernel (conv_wgrad_kernel, any dtype):
_NEW_128 = (
    _wcases("wg_1x1_head", B, 2, 9, 9, 256, 152, 1, 1, 1, (128,), OC_dw=149, nsplit=1)      # taps = 1, 24-wide OC tail tile with the extent inside it, 162 px = 2 K-tiles + 34
    + _wcases("wg_s2", BFX, 2, 21, 19, 64, 128, 3, 2, 1, (128,), nsplit=1)                  # 11x10 out: strided taps on odd sizes, both K-step widths
    + _wcases("wg_1x1_s2", BF, 1, 21, 19, 64, 192, 1, 2, 1, (128,), nsplit=1)
    + _wcases("wg_dil4", B, 2, 14, 14, 64, 128, 3, 1, 4, (128,), nsplit=1)                  # most taps are padding
    + _wcases("wg_tiny", BF, 6, 5, 5, 64, 128, 3, 1, 1, (128,), nsplit=1, tiny_seg=0)       # one K-step spans 2.56 / 1.28 images: both `while` loops iterate
    + _wcases("wg_seg2", BFX, 2, 12, 10, 64, 128, 3, 1, 1, (128,), seg2=(5, 4), nsplit=1, tiny_seg=1)   # seam at row 240 = 3 64 + 48 = 7 32 + 16: mid-tile
    + _wcases("wg_seg2_s2", B, 2, 21, 19, 64, 128, 3, 2, 1, (128,), seg2=(9, 9), nsplit=1, tiny_seg=1)  # seam at 220, strided, second map 5x5
    + _wcases("wg_rot", BF, 2, 9, 9, 256, 192, 1, 1, 1, (128,), IC_dw=195, dw_rot=3, nsplit=1)          # the f9 form: x columns 195..255 must not reach dw
    + _wcases("wg_views", BF, 2, 9, 9, 72, 128, 1, 1, 1, (128,), ld_x=80, ld_dy=256, dy_off=64, nsplit=1)  # the f8_4 form, NaN outside the blocks
    + _wcases("wg_split8", B, 2, 16, 15, 64, 128, 3, 1, 1, (128,), split_k=8, nsplit=8, nwg=72)         # nsplit % 8 == 0 block map, last split 32 rows
)
# 256x256 kernel (conv_wgrad_pipe_kernel, bf16, tile_hint 256): unit 1 = StageUnit, 0 = StageGeneral
_NEW_256 = (
    _wcases("wgp_s2", B, 2, 21, 19, 320, 256, 3, 2, 1, (256,), unit=0, nsplit=1)            # branch-free advance; IC tail with an absent channel half
    + _wcases("wgp_1x1_s2", B, 2, 21, 19, 256, 320, 1, 2, 1, (256,), IC_dw=250, OC_dw=300, unit=0, nsplit=1)    # OC tail, extents in the general epilogue
    + _wcases("wgp_dil2_s2", B, 2, 21, 19, 256, 256, 3, 2, 2, (256,), unit=0, nsplit=1)     # dilated strided taps (no dilated StageGeneral layer otherwise)
    + _wcases("wgp_tiny", B, 6, 5, 5, 256, 256, 3, 1, 1, (256,), unit=0, nsplit=1, tiny_seg=0)          # simple_adv off: unit 0 although same-size stride 1
    + _wcases("wgp_seg2_unit", B, 2, 12, 10, 256, 256, 3, 1, 2, (256,), seg2=(9, 8), ld_x=320, ld_dy=264, unit=1, nsplit=1)   # nA = 4 then nB = 3; xcross != 0
    + _wcases("wgp_seg2_s2", B, 2, 21, 19, 256, 256, 3, 2, 1, (256,), seg2=(17, 15), unit=0, nsplit=1)  # simple_adv on, seam re-decode at 220
    + _wcases("wgp_seg2_tiny", B, 2, 12, 10, 256, 256, 3, 1, 1, (256,), seg2=(5, 4), unit=0, nsplit=1, tiny_seg=1)    # simple_adv off, seam
    + _wcases("wgp_split8", B, 2, 16, 15, 256, 256, 3, 1, 1, (256,), split_k=8, unit=1, nsplit=8, nwg=72)             # the other block map on the pipe kernel
    + _wcases("wgp_split8_s2", B, 2, 31, 29, 256, 256, 3, 2, 1, (256,), split_k=8, unit=0, nsplit=8, nwg=72)          # the same on StageGeneral (16x15 out)
)
# the joint grid on two row segments: 1x1 (its float64 reference costs a ninth of a 3x3 one), M1 = 29750 = 464 64 + 54 is no multiple of 64.
# (The pair plan fuses only where the data gradient plans onto 256-row tiles, at 256 -> 256 above 32768 pixels: 95x100 + 36x44 = 22168 pixels
# is not fused, 119x125 + 36x44 = 32918 is the nearest geometry of that shape that is.)
_PAIR_SEG2 = _wcases("pair_seg2", B, 2, 119, 125, 256, 256, 1, 1, 1, (0,), seg2=(36, 44), unit=1)
WGRAD_CASES = {c.name: c for c in _OLD_WGRAD + _NEW_128 + _NEW_256 + _PAIR_SEG2}
PAIR_CASES = ("pair", "pair_seg2")                 # run through wseg_conv_bwd_pair, not stand-alone


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
GATHER_DEFECTS = ("seam_pixel", "wrap_pixel", "pad_wrap")


def wgrad_problem(c):
    """xs, dys (storage dtype, NCHW, one per row segment; x, dy = the first segment's), the float64 weight gradient [OC_dw][taps][IC_dw]
    (summed over the segments, columns rotated by dw_rot) and its companion A = sum |x| |dy|"""
    tdt = TORCH_DT[c.dt]
    pad = c.d * (c.k // 2)
    p = SimpleNamespace(c=c, pad=pad, OH=c.osizes[0][0], OW=c.osizes[0][1])
    p.xs = [rand((c.N, c.IC, h, w_), 1 + i).to(tdt) for i, (h, w_) in enumerate(c.sizes)]
    p.dys = [rand((c.N, c.OC, oh, ow), 3 + i).to(tdt) for i, (oh, ow) in enumerate(c.osizes)]
    p.x, p.dy = p.xs[0], p.dys[0]
    p.n_pix = c.n_pix
    p.ref = _wgrad(c, p.xs, p.dys, torch.float64)
    p.A = _wgrad(c, [x.abs() for x in p.xs], [dy.abs() for dy in p.dys], torch.float64)
    return p


def wgrad_rows(p):
    """the operands in the kernels' row layout: x [input pixels of segment 1 then 2][IC], dy [output pixels likewise][OC]"""
    return torch.cat([rows(x) for x in p.xs]), torch.cat([rows(dy) for dy in p.dys])


def _wgrad(c, xs, dys, dtype, defect=None):
    """dw [OC_dw][taps][IC_dw] of the operand lists (one entry per row segment) in `dtype`: reference column (ic + dw_rot) % IC_dw holds
    input channel ic.  The address defects go through the explicit gather (_wgrad_gather), everything else through conv2d_weight."""
    if defect in GATHER_DEFECTS:
        g = sum(_wgrad_gather(c, i, x.to(dtype), dy.to(dtype), defect) for i, (x, dy) in enumerate(zip(xs, dys)))
    else:
        g = sum(torch.nn.grad.conv2d_weight(x.to(dtype), (c.OC, c.IC, c.k, c.k), dy.to(dtype), c.s, c.d * (c.k // 2), c.d)
                .permute(0, 2, 3, 1).reshape(c.OC, c.k * c.k, c.IC) for x, dy in zip(xs, dys))
    rot = c.dw_rot - 1 if defect == "rot_off" else c.dw_rot
    return torch.roll(g[:c.OC_dw, :, :c.IC_dw], rot, dims=2)


def _wgrad_gather(c, seg, x, dy, defect=None):
    """The weight gradient of row segment `seg` as the kernels compute it: per tap, dy^T times the x rows gathered at
    base(n) + iy W + ix, zero where the tap falls outside the image.  defect None is conv2d_weight (asserted on the CPU);
      seam_pixel  the first output pixel of segment 2 takes its window with segment 1's width (row iy W1 + ix of its image);
      wrap_pixel  the first output pixel of image 1 (segment 1) takes the window of the pixel before it, the last of image 0;
      pad_wrap    a tap past the right border reads on in the row layout (the next row's first pixels), not zero."""
    (H, W), (OH, OW), N, pad = c.sizes[seg], c.osizes[seg], c.N, c.d * (c.k // 2)
    xr, dyr = rows(x), rows(dy)
    n = torch.arange(N).repeat_interleave(OH * OW)
    oy = torch.arange(OH).repeat_interleave(OW).repeat(N)
    ox = torch.arange(OW).repeat(N * OH)
    g = torch.zeros(c.OC, c.k * c.k, c.IC, dtype=x.dtype)
    for tap in range(c.k * c.k):
        iy, ix = oy * c.s + (tap // c.k) * c.d - pad, ox * c.s + (tap % c.k) * c.d - pad
        ok = (iy >= 0) & (iy < H) & (ix >= 0) & (ix < W)
        src = n * H * W + iy * W + ix
        if defect == "pad_wrap":
            ok = ok | ((iy >= 0) & (iy < H) & (ix >= W) & (src < N * H * W))
        if defect == "seam_pixel" and seg == 1:
            src[0] = iy[0] * c.W + ix[0]
            ok[0] = ok[0] & (src[0] < N * H * W)
        if defect == "wrap_pixel" and seg == 0 and N > 1:
            src[OH * OW], ok[OH * OW] = src[OH * OW - 1], ok[OH * OW - 1]
        g[:, tap, :] = dyr.t() @ (xr[src.clamp(0, N * H * W - 1)] * ok[:, None].to(x.dtype))
    return g


def wgrad_bar(p, splits, prior=None):
    """bar of dw = prior + weight gradient after a launch of `splits` atomics per element (the plan's nsplit)"""
    x3 = p.c.dt == "x3"
    e = acc_rel((3 if x3 else 1) * p.n_pix + splits) * p.A + (X3_MISSING * p.A if x3 else 0.0)
    ref = p.ref
    if prior is not None:
        e = e + splits * U32 * prior.abs()
        ref = ref + prior
    return ref, stored_bar(ref, SAFETY * e, "f32")


def _drop_rows(c, dys, first, count):
    """dys with the output pixels [first, first + count) of the row layout set to zero"""
    out, at = [], 0
    for dy in dys:
        r = rows(dy).clone()
        lo, hi = max(first - at, 0), min(first + count - at, r.shape[0])
        if lo < hi:
            r[lo:hi] = 0
        at += r.shape[0]
        N, C, H, W = dy.shape
        out.append(r.reshape(N, H, W, C).permute(0, 3, 1, 2))
    return out


def emulate_wgrad(p, defect=None, prior=None):
    c, f = p.c, torch.float32
    dys = [dy.float() for dy in p.dys]
    if defect == "drop_pixel":                      # one output pixel (image 0, centre) adds nothing
        dys[0] = dys[0].clone()
        dys[0][0, :, p.OH // 2, p.OW // 2] = 0
    if defect == "drop_tail":                       # the partial last K-tile adds nothing
        tail = c.n_pix % WGRAD_PK[c.dt]
        dys = _drop_rows(c, dys, c.n_pix - tail, tail)
    if c.dt == "x3":
        xh, xl = zip(*[split_bf16(x) for x in p.xs])
        dh, dl = zip(*[split_bf16(dy) for dy in dys])
        g = _wgrad(c, xh, dh, f, defect) + _wgrad(c, xh, dl, f, defect)
        if defect != "drop_lohi":
            g = g + _wgrad(c, xl, dh, f, defect)
    else:
        g = _wgrad(c, p.xs, dys, f, defect)
    if defect == "scale":
        g = g * DEFECT_SCALE
    return (g if prior is None else g + prior.float()).double()
