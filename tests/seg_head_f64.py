"""Float64 restatement of the DeepLab-v1 head in training mode (segmentation/lib/net/deeplabv1.py:42-49 under plain nn.BatchNorm2d) and the error
bars of its HIP launches, derived from the kernels' arithmetic (the convention of tests/f64_bars.py: safety factor 2, every bar states its
chain, none is fitted to a run).  TEST INFRASTRUCTURE, no tests here.

restate_head is the reference's own lines under torch autograd in float64 (F.batch_norm(training=True), the dropout mask supplied).  The stage
functions restate ONE launch each on pixel rows and are fed with the kernel path's own upstream tensors cast to float64, so every bar is the
chain of one launch.  u = U32 = 2^-24.  The GEMM bars (gemm_bar, wgrad, dgrad, stored) are tests/aff_head_f64.py's; the 3x3 conv at dilation 12
is the same product on the unfolded rows [M, 9 IC] (a tap outside the map is a zero column: the K u bound only gets looser).

The column reductions of csrc/seg_head.hip (bn_stats, bn_relu_backward, col_sums).  A workgroup owns R = rows_per_chunk(M) rows; each of its
256 threads adds the n_t = ceil(R / 4) rows of its wave in an f32 chain, the four waves are added in two more f32 levels, everything behind
that is float64 (2^-53: not counted).  With the roundings that form a term this is D = depth(M) = n_t + 4 roundings per term at most (n_t - 1
chain adds + 2 wave levels <= n_t + 1; up to 3 to form the term: d = x - shift and its square; s g and the fma with xhat are counted apart).
  mean     sum of d = x - shift_k about the chunk's first row shift_k:  D u mean|x - shift_k|, + u |mean| (stored f32)
  var      = S2/M - (S1/M)^2 about ANY centre is exact in float64 given the partials; the partials' errors e1_k (of sum d), e2_k (of sum d^2)
           enter as (1/M) sum_k e2_k + (2/M) sum_k (shift_k - mean) e1_k:  D u (mean (x - shift_k)^2 + 2 mean |shift_k - mean| |x - shift_k|).
           There is no term in u mean^2: a column of mean 64 std costs what its spread about the chunks' first rows costs, var-sized.
           (E[x^2] - mean^2 in f32 has the term u mean^2 = 4096 u var there: test_seg_head_host plants it.)
  invstd   = (var + eps)^-1/2:  invstd / (2 (var + eps)) var_bar, + u invstd
  scale    = gamma invstd: |gamma| invstd_bar + u |scale|;   shift = beta - mean scale: |scale| mean_bar + |mean| scale_bar + u |shift|
  running  (1 - m) r + m stat in float64, stored f32:  m stat_bar + u |result|   (running_var: stat = var M / (M - 1))
  y        relu(fma(z, scale, shift)) [* 1 / (1 - p)] from the kernel's own scale / shift: one rounding, one more for the factor: 2 u |y|,
           stored; the dropped elements are exactly 0.  (p = 0.5, the head's: the factor 2 is exact and the product rounds nothing: u |y|.
           A factor that is no power of two — p = 0.25: f32(4/3) — carries its own rounding as well: 3 u |y|, which the safety factor still
           covers (2 x 2 u); the bar is left as it is, test_seg_head_host.py judges an f32 evaluation against it.)
  s1       = sum dy, dy = s g [y > 0] (one rounding):  D u sum |dy| + u |s1|
  s2       = sum dy xhat, xhat = (z - mean) invstd (two roundings, the fma one more):  (D + 2) u sum |dy xhat| + u |s2|
  dz       = k ((dy - m1) - xhat m2), k = gamma invstd, m1 = s1 / M, m2 = s2 / M (each stored f32):
           |k| (u |dy| + s1_bar / M + |xhat| s2_bar / M + 2 u |xhat m2|) + 4 u |k| (|dy| + |m1| + |xhat m2|), stored
  col_sums D u sum |x| + u |sum|
"""
import torch
import torch.nn.functional as F

from tests.aff_head_f64 import SPLIT_X3, dgrad, gemm_bar, stored, wgrad  # noqa: F401  (re-exported: the 1x1 stages use them as they are)
from tests.f64_bars import SAFETY, U32

DIL = 12
CONVS = ("conv_fov", "conv_fov2", "cls_conv")


def rows_per_chunk(M):
    """sh_rows_per_chunk of csrc/seg_head.hip"""
    return max(32, ((M + 511) // 512 + 3) // 4 * 4)


def row_chunks(M):
    return -(-M // rows_per_chunk(M))


def depth(M):
    return -(-rows_per_chunk(M) // 4) + 4


def workspace_chunks(nbytes, C):
    """row chunks of a wseg_bn_stats_workspace_bytes(M, C) answer: (3 chunks + 3) C floats"""
    return (nbytes // (4 * C) - 3) // 3


# ------------------------------------------------------------------------------------------------------------------ the reference's lines
def restate_head(t, w, bn, keep, p=0.5, eps=1e-5):
    """deeplabv1.py:42-49 in training mode on NCHW float64: w {conv: [OC, IC, k, k]} and "cls_bias"; bn {"bn_fov" / "bn_fov2": (gamma, beta)};
    keep: the dropout mask [N, 512, h, w] (bool).  Returns the [N, 21, h, w] logits."""
    x = F.conv2d(t, w["conv_fov"], None, 1, DIL, DIL)
    x = F.relu(F.batch_norm(x, None, None, bn["bn_fov"][0], bn["bn_fov"][1], True, 0.0, eps))
    x = F.conv2d(x, w["conv_fov2"])
    x = F.relu(F.batch_norm(x, None, None, bn["bn_fov2"][0], bn["bn_fov2"][1], True, 0.0, eps))
    x = x * keep.to(x.dtype) / (1.0 - p)
    return F.conv2d(x, w["cls_conv"], w["cls_bias"])


def weights64(net, mode):
    """{conv: [OC, IC k k] float64} of the three head convs as the packs of `mode` hold them (bf16: rounded to bf16), columns in F.unfold's
    order ic * k * k + tap"""
    out = {}
    for name in CONVS:
        wt = getattr(net, name).weight.detach()
        wt = wt.reshape(wt.shape[0], -1)
        out[name] = (wt.bfloat16() if mode == "bf16" else wt).double()
    return out


def unfold_rows(x, N, h, w):
    """pixel rows [M, C] -> the rows of the 3x3 dilation-12 conv [M, C 9] (column c * 9 + tap)"""
    C = x.shape[1]
    u = F.unfold(x.view(N, h, w, C).permute(0, 3, 1, 2), 3, DIL, DIL)             # [N, C 9, h w]
    return u.permute(0, 2, 1).reshape(N * h * w, C * 9)


def fold_rows(u, N, h, w):
    """the adjoint of unfold_rows: [M, C 9] -> [M, C]"""
    C = u.shape[1] // 9
    x = F.fold(u.view(N, h * w, C * 9).permute(0, 2, 1), (h, w), 3, DIL, DIL)      # [N, C, h, w]
    return x.permute(0, 2, 3, 1).reshape(N * h * w, C)


def conv(X, W, mode, bias=None):
    """(ref, bar) of rows X W^T (+ bias) as a forward launch stores its raw sum (epilogue 0; the bias: one more rounding)"""
    ref = X @ W.T
    bar = gemm_bar(X, W, mode)
    if bias is not None:
        ref = ref + bias
        bar = bar + U32 * ref.abs()
    return ref, stored(ref, SAFETY * bar, mode)


def dgrad3(dY, W, N, h, w, mode, scale=None, mask=None):
    """(ref, bar) of the 3x3 dilation-12 data gradient (W [OC, IC 9]): K = 9 OC products per element; optionally the epi-1 form"""
    ref = fold_rows(dY @ W, N, h, w)
    S = fold_rows(dY.abs() @ W.abs(), N, h, w)
    bar = (9 * dY.shape[1] * U32 + (SPLIT_X3 if mode == "bf16x3" else 0.0)) * S
    if scale is not None:
        gate = scale[None, :] * (mask > 0)
        ref, bar = ref * gate, bar * gate.abs() + 2 * U32 * (ref * gate).abs()
    return ref, stored(ref, SAFETY * bar, mode)


# ------------------------------------------------------------------------------------------------------------------ csrc/seg_head.hip
def _chunk_shift(x):
    """[M, C]: for every row the first row of its chunk (the partial's shift)"""
    M, R = x.shape[0], rows_per_chunk(x.shape[0])
    first = torch.arange(M, device=x.device) // R * R
    return x[first]


def bn_stats(x, gamma, beta, eps, momentum, running_mean, running_var):
    """{name: (ref, bar)} of wseg_bn_stats on float64 rows x [M, C]: mean, var (not an output: for the planted defects), invstd, scale, shift,
    running_mean, running_var"""
    M, D = x.shape[0], depth(x.shape[0])
    mean = x.mean(0)
    var = ((x - mean) ** 2).mean(0)
    sh = _chunk_shift(x)
    dev = (x - sh).abs()
    mean_core = D * U32 * dev.mean(0)
    var_core = D * U32 * ((dev ** 2).mean(0) + 2 * ((sh - mean).abs() * dev).mean(0))
    invstd = (var + eps) ** -0.5
    invstd_core = invstd / (2 * (var + eps)) * var_core
    scale = gamma * invstd
    scale_core = gamma.abs() * invstd_core
    shift = beta - mean * scale
    shift_core = scale.abs() * mean_core + mean.abs() * scale_core
    out = {"mean": (mean, SAFETY * (mean_core + U32 * mean.abs())), "var": (var, SAFETY * var_core),
           "invstd": (invstd, SAFETY * (invstd_core + U32 * invstd)), "scale": (scale, SAFETY * (scale_core + U32 * scale.abs())),
           "shift": (shift, SAFETY * (shift_core + U32 * shift.abs()))}
    if running_mean is not None:
        rm = (1 - momentum) * running_mean + momentum * mean
        rv = (1 - momentum) * running_var + momentum * var * M / (M - 1)
        out["running_mean"] = (rm, SAFETY * (momentum * mean_core + U32 * rm.abs()))
        out["running_var"] = (rv, SAFETY * (momentum * var_core * M / (M - 1) + U32 * rv.abs()))
    return out


def bn_relu_drop(z, scale, shift, keep, p, out_bf16):
    """(ref, bar) of y from the kernel's own scale / shift; keep: bool [M, C] or None"""
    ref = F.relu(z * scale + shift)
    if keep is not None:
        ref = ref * keep.to(ref.dtype) / (1.0 - p)
    return ref, stored(ref, SAFETY * 2 * U32 * ref.abs(), "bf16" if out_bf16 else "fp32")


def bn_relu_backward(g, y, z, mean, invstd, gamma, s, out_bf16):
    """{s1, s2, dz: (ref, bar)} of wseg_bn_relu_backward from the float64 casts of the kernel's inputs"""
    M, D = z.shape[0], depth(z.shape[0])
    dy = s * g * (y > 0)
    xhat = (z - mean) * invstd
    s1, s2 = dy.sum(0), (dy * xhat).sum(0)
    s1_bar = SAFETY * (D * U32 * dy.abs().sum(0) + U32 * s1.abs())
    s2_bar = SAFETY * ((D + 2) * U32 * (dy * xhat).abs().sum(0) + U32 * s2.abs())
    k, m1, m2 = gamma * invstd, s1 / M, s2 / M
    dz = k * (dy - m1 - xhat * m2)
    core = k.abs() * (U32 * dy.abs() + 2 * U32 * (xhat * m2).abs()) + 4 * U32 * k.abs() * (dy.abs() + m1.abs() + (xhat * m2).abs())
    dz_bar = SAFETY * core + k.abs() * (s1_bar / M + xhat.abs() * s2_bar / M)
    return {"s1": (s1, s1_bar), "s2": (s2, s2_bar), "dz": (dz, stored(dz, dz_bar, "bf16" if out_bf16 else "fp32"))}


def col_sums(x):
    ref = x.sum(0)
    return ref, SAFETY * (depth(x.shape[0]) * U32 * x.abs().sum(0) + U32 * ref.abs())


# ------------------------------------------------------------------------------------------------------------------ the composed chain
def _prod(a, ra, b, rb):
    """radius of a b for |da| <= ra, |db| <= rb (the second-order term kept)"""
    return a.abs() * rb + b.abs() * ra + ra * rb


def _stats_r(z, r_z, gamma, beta, eps):
    """batch statistics of rows known to r_z: {name: (ref, radius)}.  mean: mean r_z; var = mean (z - mean)^2 moves by at most
    mean (2 |z - mean| r_z + r_z^2) (the perturbation's own mean drops out of the cross term); invstd exactly, at the smaller variance; each plus
    the launch's own bar"""
    own = bn_stats(z, gamma, beta, eps, 0.0, None, None)
    mean, var, invstd, scale, shift = (own[k][0] for k in ("mean", "var", "invstd", "scale", "shift"))
    r_mean = r_z.mean(0) + own["mean"][1]
    r_var = (2 * (z - mean).abs() * r_z + r_z ** 2).mean(0) + own["var"][1]
    r_invstd = ((var - r_var).clamp_min(0) + eps) ** -0.5 - invstd + own["invstd"][1]
    r_scale = gamma.abs() * r_invstd + own["scale"][1]
    r_shift = _prod(mean, r_mean, scale, r_scale) + own["shift"][1]
    return {"mean": (mean, r_mean), "invstd": (invstd, r_invstd), "scale": (scale, r_scale), "shift": (shift, r_shift)}


def _bwd_r(g, r_g, y, unc, z, r_z, st, gamma, s, bf):
    """the BN-ReLU(-dropout) backward of operands known to their radii; unc: elements whose gate y > 0 the radius of the pre-activation cannot
    decide (there dy is anything between 0 and s g).  {s1, s2, dz: (ref, radius)}"""
    M = z.shape[0]
    (mean, r_mean), (invstd, r_invstd) = st["mean"], st["invstd"]
    own = bn_relu_backward(g, y, z, mean, invstd, gamma, s, bf)
    gate = y > 0
    dy = s * g * gate
    r_dy = torch.where(unc, s * (g.abs() + r_g), s * r_g * gate)
    zc = z - mean
    xhat = zc * invstd
    r_xhat = _prod(zc, r_z + r_mean, invstd, r_invstd)
    s1, s2 = own["s1"][0], own["s2"][0]
    r_s1 = r_dy.sum(0) + own["s1"][1]
    r_s2 = _prod(dy, r_dy, xhat, r_xhat).sum(0) + own["s2"][1]
    k, r_k = gamma * invstd, gamma.abs() * r_invstd
    inner = dy - s1 / M - xhat * (s2 / M)
    r_inner = r_dy + r_s1 / M + _prod(xhat, r_xhat, s2 / M, r_s2 / M)
    return {"s1": (s1, r_s1), "s2": (s2, r_s2), "dz": (own["dz"][0], _prod(k, r_k, inner, r_inner) + own["dz"][1])}


def chain(t, W, bias, bn, keep, d_rows, N, h, w, mode, eps=1e-5, p=0.5):
    """The head forward and backward in float64 from the kernel path's INPUTS only — t [M, 4096] as the engine holds it, the weights as the packs
    hold them (weights64), bias [21], bn {1: (gamma, beta), 2: ...}, the dropout mask, and the gradient d_rows [M, 21] the loss handed back — with
    the COMPOSED bar of every result: each launch's own bar (above) plus the radius its operands arrive with, carried through the launch's
    arithmetic (a product a b of operands known to ra, rb is known to |a| rb + |b| ra + ra rb; a matrix product carries a radius through the
    absolute values of the other operand; an element whose ReLU gate the radius of its pre-activation cannot decide carries its whole gradient
    as radius).  Nothing is fitted.  Returns {name: (ref, bar)}.
    These are WORST-CASE radii through three products and two normalisations, and they are wide: about the size of the values on the small host
    problem (K = 72), and meaningless at the real K = 36864, where the first conv's K u bound alone exceeds a column's spread and the radius of
    the second variance passes the variance (measured on an MI355X, fp32, 2 x 13 x 16: d_t off the float64 chain by 8.6e-10 at max |d_t| 4.3e-4,
    composed bar 8e10).  They bound; they do not discriminate.  The sharp end-to-end statement is the bitwise one of
    tests/test_gpu_seg_head.py::test_end_to_end_through_autograd, on top of the per-launch bars."""
    bf = mode == "bf16"
    W1, W2, W3 = W["conv_fov"], W["conv_fov2"], W["cls_conv"]
    X0 = unfold_rows(t, N, h, w)
    z1, r_z1 = conv(X0, W1, mode)
    st1 = _stats_r(z1, r_z1, bn[1][0], bn[1][1], eps)
    v1 = z1 * st1["scale"][0] + st1["shift"][0]
    r_v1 = _prod(z1, r_z1, *st1["scale"]) + st1["shift"][1]
    y1, own = bn_relu_drop(z1, st1["scale"][0], st1["shift"][0], None, p, bf)
    r_y1 = r_v1 + own
    z2, own = conv(y1, W2, mode)
    r_z2 = r_y1 @ W2.abs().T + own
    st2 = _stats_r(z2, r_z2, bn[2][0], bn[2][1], eps)
    v2 = z2 * st2["scale"][0] + st2["shift"][0]
    r_v2 = _prod(z2, r_z2, *st2["scale"]) + st2["shift"][1]
    y2, own = bn_relu_drop(z2, st2["scale"][0], st2["shift"][0], keep, p, bf)
    s = 1.0 / (1.0 - p)
    r_y2 = s * keep * r_v2 + own
    rows, own = conv(y2, W3, mode, bias)
    out = {"rows": (rows, r_y2 @ W3.abs().T + own)}
    d = d_rows
    out["d_bias"] = col_sums(d)
    ref, own = wgrad(y2, d, mode)
    out["dW_cls_conv"] = (ref, d.abs().T @ r_y2 + own)
    d_y2, r_dy2 = dgrad(d, W3, mode)
    b2 = _bwd_r(d_y2, r_dy2, y2, keep & (v2.abs() <= r_v2), z2, r_z2, st2, bn[2][0], s, bf)
    dz2, r_dz2 = b2["dz"]
    ref, own = wgrad(y1, dz2, mode)
    out["dW_conv_fov2"] = (ref, r_dz2.T @ (y1.abs() + r_y1) + dz2.abs().T @ r_y1 + own)
    d_y1, own = dgrad(dz2, W2, mode)
    b1 = _bwd_r(d_y1, r_dz2 @ W2.abs() + own, y1, v1.abs() <= r_v1, z1, r_z1, st1, bn[1][0], 1.0, bf)
    dz1, r_dz1 = b1["dz"]
    ref, own = wgrad(X0, dz1, mode)
    out["dW_conv_fov"] = (ref, r_dz1.T @ X0.abs() + own)
    ref, own = dgrad3(dz1, W1, N, h, w, mode)
    out["d_t"] = (ref, fold_rows(r_dz1 @ W1.abs(), N, h, w) + own)
    out.update(d_beta1=b1["s1"], d_gamma1=b1["s2"], d_beta2=b2["s1"], d_gamma2=b2["s2"])
    return out


def inside(got, ref, bar):
    """every element of `got` within `bar` of `ref` (a NaN fails); returns max err / bar for the tests' prints"""
    err = (got.double() - ref).abs()
    ok = bool((err <= bar).all())
    ratio = float((err / bar.clamp_min(1e-300)).max()) if err.numel() else 0.0
    return ok, ratio
