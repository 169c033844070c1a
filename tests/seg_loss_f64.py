"""float64 restatement of the DeepLab-v1 training loss (segmentation/lib/net/deeplabv1.py:50 + experiment/SEAM_deeplabv1_resnet38/train.py:85,97):
the coarse logits resampled bilinearly (align_corners=True) to the label size, cross-entropy with ignore_index 255, mean over the valid pixels
of the batch — and its gradient on the coarse logits as the explicit TRANSPOSED resample of (softmax - onehot) / count.  Written from that
math and never from the kernels (csrc/seg_loss.hip); the yardstick of tests/test_seg_loss_host.py and tests/test_gpu_seg_loss.py, with the
bars an f32 evaluation of the same math may differ by.  TEST INFRASTRUCTURE, no tests here.

Bars (the convention of tests/f64_bars.py: derived, one SAFETY = 2 on the sum of the terms, never fitted to a run).  u = U32, n = n_cls,
M = max |logit|, every line a bound on an absolute error:

  e_z    one resampled logit                      _interp_bar(fh, fw, M) / SAFETY          (coordinate error times the slope, six roundings)
  r_lse  the roundings of lse = mx + log(sum_c exp(z_c - mx)) on GIVEN z:
           z_c - mx            one rounding of a value <= 2M, a relative error of exp's argument        2M u
           expf                1 ulp                                                                     EXP_ULP
           the n-term sum      n - 1 roundings, all terms positive                                       (n - 1) u
           -> relative error of the sum, the absolute error of its log;  logf: 1 ulp of |log sum| <= log n   LOG_ULP log n
           mx + log            one rounding of |lse| <= M + log n                                        (M + log n) u
  e_lse  = e_z + r_lse                            lse is 1-Lipschitz in the logits (sup norm): the softmax weights sum to one
  e_nll  = e_lse + e_z + (2M + log n) u           z[label]'s own error, and the rounding of lse - z[label] (|nll| <= 2M + log n)
  loss   = sum nll / count:  mean of e_nll, plus a summation tree of D levels over non-negative terms (D u times the mean; the kernels' tree
           has 8 f32 levels, the rest is f64; a balanced tree over count terms has ceil(log2 count): D is the deeper of the two), plus the
           quotient's rounding u |loss|
  grad   of one coarse cell and class, g = sum_pix w_y w_x (p_c - [c = label]) / count over the valid pixels whose taps include the cell:
           e_p  p_c = exp(z_c - lse):  the softmax of logits e_z off is within min(p, 1 - p) expm1(2 e_z) (p'/p lies in exp(+-2 e_z), and the
                same holds for 1 - p_c, the sum of the others); the saved lse carries r_lse, the subtraction one rounding of a value
                <= 2M + log n, expf 1 ulp: p (r_lse + (2M + log n) u + EXP_ULP)
           (a) sum_pix w_y w_x e_p / count                                   the cell's tap weights times the softmax error
           (b) (coord_y + coord_x) sum_pix |p - onehot| / count              the weight error: each axis weight is a hat function of the source
                coordinate, slope 1, so |dw| <= |ds| = _coord_bar per axis (and the other axis' weight <= 1); summed over the pixels within
                1 + _coord_bar of the cell — a pixel the f64 coordinates leave just outside may be inside in f32, with a weight <= _coord_bar
           (c) (S + 6) u sum_pix w_y w_x |p - onehot| / count                S - 1 additions in any order (S = the cell's valid pixels), and
                per term the roundings of 1 - f (two axes), w_y w_x, p - onehot, their product; the scale gscale / count and its product: 2 more
  bf16 rows are read exactly: the float64 side gets the same bf16 values.  A bf16 d_rows adds one bf16 rounding of the value (bf16_store_bar).
"""
import math

import torch

from tests import seg_f64
from tests.f64_bars import SAFETY, U32, _coord_bar, _interp_bar

EXP_ULP = LOG_ULP = 2.0 * U32                  # expf, logf: 1 ulp (HIP math API)
U_BF16 = 2.0 ** -8                             # bf16 unit roundoff (round to nearest: half an ulp = 2^-8 relative)
IGNORE = 255

# coarse -> label size, N; every coarse and label size at which the kernels take another path
SHAPES = [
    ((1, 1), (5, 9), 1),                       # coarse size 1: one cell's support is the whole image
    ((2, 3), (11, 13), 1),
    ((5, 7), (33, 47), 1),
    ((5, 7), (40, 56), 1),
    ((7, 7), (49, 49), 1),                     # scale 6/48, exact
    ((4, 6), (10, 16), 1),                     # scale 3/9 is inexact in f32: f32(1/3) * 3 sits at an integer boundary
    ((13, 16), (57, 301), 1),                  # several workgroups, W no multiple of the block
    ((5, 7), (1, 37), 1),
    ((5, 7), (29, 1), 1),
    ((13, 16), (7, 9), 1),                     # a downsample: cells with no pixel get exact zeros
    ((5, 7), (33, 47), 3),                     # image 1 entirely ignored
    ((17, 33), (131, 253), 2),                 # 66286 pixels = 259 forward workgroups: the finish adds partials t and t + 256; 33143 pixels an
]                                              # image: one workgroup straddles the two; scales 16/130 and 32/252, both inexact in f32
PAST_256_PARTIALS = SHAPES[-1]                 # run at 21 classes only (CLASS_CASES)
# every (shape, n_cls) of the sweeps of tests/test_gpu_seg_loss.py and tests/test_seg_loss_host.py
CLASS_CASES = [(s, n) for s in SHAPES for n in (21, 2) if n == 21 or s != PAST_256_PARTIALS]
# the class counts of the other two 8-column chunk counts (NC8 = 2: 9 .. 16 classes; NC8 = 4: 25 .. 32, the maximum): the first and the last
# of each, the last without a pad column; on an upsample and on the downsample
NC8_COUNTS = (9, 16, 25, 32)
NC8_SHAPES = (((5, 7), (33, 47), 1), ((13, 16), (7, 9), 1))


def forward_workgroups(shape):
    """workgroups of the forward launch (256 label pixels each) = partials the finish adds"""
    (_fh, _fw), (H, W), N = shape
    return (N * H * W + 255) // 256


def shape_id(s):
    (fh, fw), (H, W), N = s
    return f"{fh}x{fw}-{H}x{W}-N{N}"


def make_label(N, H, W, n_cls, seed):
    """uint8 [N, H, W]: random classes, about 15 % of 255 in blocks, one fully ignored row per image (H > 1)"""
    g = torch.Generator().manual_seed(seed)
    lab = torch.randint(0, n_cls, (N, H, W), generator=g, dtype=torch.int64)
    for n in range(N):
        for _ in range(4):                                       # four blocks of about 0.2 x 0.2 of the map: 15 % with the overlaps
            bh, bw = max(1, round(0.2 * H)), max(1, round(0.2 * W))
            y0 = int(torch.randint(0, H - bh + 1, (1,), generator=g))
            x0 = int(torch.randint(0, W - bw + 1, (1,), generator=g))
            lab[n, y0:y0 + bh, x0:x0 + bw] = IGNORE
        if H > 1:
            lab[n, int(torch.randint(0, H, (1,), generator=g))] = IGNORE
    return lab.to(torch.uint8)


def make_case(shape, n_cls, dtype, seed):
    """(coarse [N, n_cls, fh, fw] float32 holding values `dtype` represents exactly, label uint8 [N, H, W]) of one SHAPES entry"""
    (fh, fw), (H, W), N = shape
    g = torch.Generator().manual_seed(seed)
    coarse = (4.0 * torch.randn(N, n_cls, fh, fw, generator=g)).to(dtype).float()
    label = make_label(N, H, W, n_cls, seed + 1)
    if N == 3:
        label[1] = IGNORE
    return coarse, label


def axis_matrix(n_in, n_out):
    """[n_out, n_in] float64: row o holds the align_corners=True weights of output position o (1 - f at i0, f at i1)"""
    i0, i1, f = seg_f64._axis(n_in, n_out)
    Wm = torch.zeros(n_out, n_in, dtype=torch.float64)
    o = torch.arange(n_out)
    Wm.index_put_((o, i0), 1 - f, accumulate=True)
    Wm.index_put_((o, i1), f, accumulate=True)
    return Wm


def restate(coarse, label, gscale=1.0):
    """coarse [N, C, fh, fw], label integer [N, H, W] -> dict of float64: loss, count, nll_sum, oor (the four scalars), lse [N, H, W],
    grad [N, C, fh, fw] = gscale * d loss / d coarse, and what the bars need (p, absg = |p - onehot| on the valid pixels, valid)"""
    N, C, fh, fw = coarse.shape
    H, W = label.shape[1:]
    label = label.long()
    z = seg_f64.resize(coarse, H, W)                                              # [N, C, H, W]
    valid = label < C                                                             # 255 and anything in [C, 255) are ignored
    oor = ((label >= C) & (label != IGNORE)).sum()
    lse = torch.logsumexp(z, 1)
    safe = label.clamp(max=C - 1)                                                 # (an ignored pixel's class is never used below)
    nll = lse - z.gather(1, safe[:, None])[:, 0]
    count = valid.sum()
    nll_sum = torch.where(valid, nll, torch.zeros_like(nll)).sum()
    loss = nll_sum / count                                                        # no valid pixel: 0 / 0, the mean of an empty set
    p = torch.exp(z - lse[:, None])
    onehot = torch.zeros_like(p).scatter_(1, safe[:, None], 1.0)
    diff = torch.where(valid[:, None], p - onehot, torch.zeros_like(p))           # an ignored pixel contributes nothing
    G = torch.where(valid[:, None], diff / count, torch.zeros_like(p))
    Wy, Wx = axis_matrix(fh, H), axis_matrix(fw, W)
    grad = gscale * torch.einsum("yi,ncyx,xj->ncij", Wy, G, Wx)                   # the transposed resample
    return dict(loss=loss, count=count.double(), nll_sum=nll_sum, oor=oor.double(), lse=lse, grad=grad, p=p, absg=diff.abs(), valid=valid,
                Wy=Wy, Wx=Wx)


def out4_ref(ref):
    return torch.stack([ref["loss"], ref["count"], ref["nll_sum"], ref["oor"]])


def _r_lse(n, M):
    return (2.0 * M + (n - 1)) * U32 + EXP_ULP + LOG_ULP * math.log(n) + (M + math.log(n)) * U32


def lse_bar(fh, fw, n, M):
    """|lse_f32 - lse_64| of one pixel: e_lse of the module docstring, times SAFETY"""
    return SAFETY * (_interp_bar(fh, fw, M) / SAFETY + _r_lse(n, M))


def nll_bar(fh, fw, n, M):
    e_z = _interp_bar(fh, fw, M) / SAFETY
    return SAFETY * (2.0 * e_z + _r_lse(n, M) + (2.0 * M + math.log(n)) * U32)


def loss_bar(ref, coarse):
    """|loss_f32 - loss_64| (module docstring, `loss`)"""
    N, n, fh, fw = coarse.shape
    M = float(coarse.abs().max())
    count = int(ref["count"])
    if count == 0:
        return 0.0                                                                # NaN on both sides, compared as such
    depth = max(8, math.ceil(math.log2(max(count, 2))))
    loss = abs(float(ref["loss"]))
    return nll_bar(fh, fw, n, M) + SAFETY * (depth + 1) * U32 * loss


def nll_sum_bar(ref, coarse):
    return loss_bar(ref, coarse) * float(ref["count"])


def grad_bar(ref, coarse, gscale=1.0):
    """[N, C, fh, fw]: the bar of every element of the gradient (module docstring, `grad` (a) + (b) + (c)), times SAFETY and |gscale|"""
    N, n, fh, fw = coarse.shape
    H, W = ref["valid"].shape[1:]
    count = float(ref["count"])
    if count == 0:
        return torch.zeros(N, n, fh, fw, dtype=torch.float64)                     # nothing contributes: exact zeros
    M = float(coarse.abs().max())
    e_z = _interp_bar(fh, fw, M) / SAFETY
    p, absg, valid = ref["p"], ref["absg"], ref["valid"]
    Wy, Wx = ref["Wy"], ref["Wx"]
    t = lambda A, X, B: torch.einsum("yi,ncyx,xj->ncij", A, X, B)
    e_p = torch.minimum(p, 1 - p) * math.expm1(2.0 * e_z) + p * (_r_lse(n, M) + (2.0 * M + math.log(n)) * U32 + EXP_ULP)
    term_a = t(Wy, torch.where(valid[:, None], e_p, torch.zeros_like(p)), Wx)
    cy, cx = _coord_bar(fh), _coord_bar(fw)
    sy = torch.arange(H, dtype=torch.float64) * ((fh - 1) / (H - 1) if H > 1 else 0.0)
    sx = torch.arange(W, dtype=torch.float64) * ((fw - 1) / (W - 1) if W > 1 else 0.0)
    Ey = ((sy[:, None] - torch.arange(fh)[None, :]).abs() < 1 + cy).double()      # [H, fh]: the pixels within 1 + coord of the cell
    Ex = ((sx[:, None] - torch.arange(fw)[None, :]).abs() < 1 + cx).double()
    term_b = ((cy if fh > 1 else 0.0) + (cx if fw > 1 else 0.0)) * t(Ey, absg, Ex)   # (an axis of one input position has the weight 1 exactly)
    S = torch.einsum("yi,nyx,xj->nij", (Wy > 0).double(), valid.double(), (Wx > 0).double())[:, None]
    term_c = (S + 6.0) * U32 * t(Wy, absg, Wx)
    return SAFETY * abs(gscale) * (term_a + term_b + term_c) / count


def bf16_store_bar(ref, bar):
    """bar of a value computed within `bar` of `ref` and then rounded to bf16: the rounding is within U_BF16 of the computed value"""
    return bar + U_BF16 * (ref.abs() + bar)


def nan_equal(a, b):
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    return bool((torch.isnan(a) == torch.isnan(b)).all())


def within(got, ref, bar):
    """every element of `got` within `bar` of `ref`, NaN exactly where `ref` has NaN"""
    got, ref = torch.as_tensor(got).double(), torch.as_tensor(ref).double()
    bar = torch.as_tensor(bar, dtype=torch.float64).expand_as(ref)
    nan = torch.isnan(ref)
    return nan_equal(got, ref) and bool(((got - ref).abs()[~nan] <= bar[~nan]).all())


def judge(got, ref, coarse, gscale=1.0, grad_store_bf16=False):
    """dict name -> (ok, worst error / bar) of an evaluation `got` (loss, lse or None, grad) against the restatement `ref`"""
    N, n, fh, fw = coarse.shape
    M = float(coarse.abs().max())
    gb = grad_bar(ref, coarse, gscale)
    if grad_store_bf16:
        gb = bf16_store_bar(ref["grad"], gb)
    checks = dict(loss=(got["loss"], ref["loss"], loss_bar(ref, coarse)), grad=(got["grad"], ref["grad"], gb))
    if got.get("lse") is not None:
        checks["lse"] = (got["lse"], ref["lse"], lse_bar(fh, fw, n, M))
    out = {}
    for k, (g, r, b) in checks.items():
        g, r = torch.as_tensor(g).double(), torch.as_tensor(r).double()
        b = torch.as_tensor(b, dtype=torch.float64).expand_as(r)
        fin = ~torch.isnan(r) & ~torch.isnan(g)
        ratio = ((g - r).abs()[fin] / b[fin].clamp_min(1e-300)).max().item() if bool(fin.any()) else 0.0
        out[k] = (within(g, r, b), ratio)
    return out
