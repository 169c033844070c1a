"""Float64 restatement of the AffinityNet head (network/resnet38_aff.py:39-42) and the error bars of its HIP launches, derived from the
kernels' arithmetic (the convention of tests/f64_bars.py: safety factor 2, every bar states its chain, none is fitted to a run).
TEST INFRASTRUCTURE, no tests here.

restate_head is the reference's own lines under torch autograd in float64.  The stage functions below restate ONE launch each on pixel
rows (a 1x1 convolution is the product rows . W^T) and are fed with the kernel path's own upstream tensor cast to float64, so every bar
is the chain of one launch.  u = U32 = 2^-24.

  GEMM, K terms of f32 accumulation (MFMA, any order):  K u (|X| |W|^T), evaluated in float64                                  [gemm_bar]
    fp32    nothing more (v_mfma_f32_16x16x4_f32 is an f32 fma chain)
    bf16x3  every f32 operand is x = hi + lo, hi = RNE bf16(x), lo = RNE bf16(x - hi), and the product is hi.hi + lo.hi + hi.lo
            (include/wseg_hip.h "dtype", csrc/common.h split_bf16x8; scripts/emulate_split_bf16.py is the same three-product form):
            |x - hi - lo| <= 2^-17 |x| for either operand (pinned by test_to_bf16_and_split_bf16) and the dropped lo.lo <= 2^-8 2^-8
            |x||w| (|lo| is within bf16's half ulp, 2^-8 relative): SPLIT_X3 = 2^-17 + 2^-17 + 2^-16 = 2^-15 of |X| |W|^T
    bf16    the operands ARE bf16 values (activations as the kernels stored them; the weights are rounded to bf16 on the test side, as
            the packs are): their products are exact in f32, the chain is the same K u
  stored in bf16: one bf16 ulp of the float64 result more                                                                      [_ulp_bf16]
  ELU epilogue (elu1: v > 0 ? v : expm1f(v)): elu is 1-Lipschitz, so the sum's error passes at most unchanged; expm1f is 1 ulp (HIP math
            API) = 2 u |elu|
  BN-ReLU backward epilogue (epi 1): two more products (scale, drop) = 2 u |result|
  weight gradient dW = X^T dY over M pixels (float atomics over pixel ranges in some kernels: the bound does not depend on the order):
            M u (|X|^T |dY|), + SPLIT_X3 (|X|^T |dY|) in bf16x3; dW is f32 in every mode
  ELU backward (csrc/aff_head.hip): gscale * g, y + 1, their product: 3 u |result| (+ one bf16 ulp when stored in bf16)
"""
import torch
import torch.nn.functional as F

from tests.f64_bars import SAFETY, U32

SPLIT_X3 = 2.0 ** -15
EXPM1_ULP = 2.0 * U32
SLICES = {"f8_3": (0, 64), "f8_4": (64, 192), "f8_5": (192, 448)}


def _ulp_bf16(x):
    """one bf16 ulp of a float64 value (a result stored in bf16)"""
    return torch.exp2(torch.floor(torch.log2(x.abs().clamp_min(2.0 ** -126))) - 7)


def restate_head(conv4, conv5, conv6, w):
    """network/resnet38_aff.py:39-42 on NCHW float64 tensors; w: {name: [OC, IC, 1, 1] float64}.  Returns (feat, f9) NCHW."""
    f8_3 = F.elu(F.conv2d(conv4, w["f8_3"]))
    f8_4 = F.elu(F.conv2d(conv5, w["f8_4"]))
    f8_5 = F.elu(F.conv2d(conv6, w["f8_5"]))
    feat = torch.cat([f8_3, f8_4, f8_5], dim=1)
    return feat, F.elu(F.conv2d(feat, w["f9"]))


def weights64(net, mode):
    """{name: [OC, IC] float64} of the four head convs as the packs of `mode` hold them (bf16: rounded to bf16)"""
    out = {}
    for name in ("f8_3", "f8_4", "f8_5", "f9"):
        wt = getattr(net, name).weight.detach()
        wt = wt.reshape(wt.shape[0], wt.shape[1])
        out[name] = (wt.bfloat16() if mode == "bf16" else wt).double()
    return out


def stored(ref, bar, mode):
    """the bar of a result the kernel stores in the mode's activation dtype"""
    return bar + _ulp_bf16(ref) if mode == "bf16" else bar


def gemm_bar(X, W, mode):
    """raw (no safety factor) error of rows X [M, K] times W^T (W [OC, K]) accumulated in f32"""
    K = X.shape[1]
    return (K * U32 + (SPLIT_X3 if mode == "bf16x3" else 0.0)) * (X.abs() @ W.abs().T)


def elu_conv(X, W, mode):
    """(ref, bar) of elu(X W^T) as the forward launch (epilogue 3) stores it"""
    ref = F.elu(X @ W.T)
    return ref, stored(ref, SAFETY * (gemm_bar(X, W, mode) + EXPM1_ULP * ref.abs()), mode)


def dgrad(dY, W, mode, scale=None, mask=None):
    """(ref, bar) of the data gradient dY W (W [OC, IC]: the forward weight), optionally the epi-1 form * scale[c] * (mask > 0)"""
    ref = dY @ W
    bar = gemm_bar(dY, W.T, mode)
    if scale is not None:
        gate = scale[None, :] * (mask > 0)
        ref, bar = ref * gate, bar * gate.abs() + 2 * U32 * (ref * gate).abs()
    return ref, stored(ref, SAFETY * bar, mode)


def wgrad(X, dY, mode):
    """(ref, bar) of dW [OC, IC] = dY^T X over the M rows (f32 result)"""
    M = X.shape[0]
    return dY.T @ X, SAFETY * (M * U32 + (SPLIT_X3 if mode == "bf16x3" else 0.0)) * (dY.abs().T @ X.abs())


def elu_grad(y):
    """ELU's derivative from its output"""
    return torch.where(y > 0, torch.ones_like(y), y + 1)


def elu_backward(g, y, gscale, out_bf16):
    """(ref, bar) of gscale * g * elu'(y) from the float64 casts of the kernel's inputs"""
    ref = (1.0 if gscale is None else gscale) * g * elu_grad(y)
    bar = SAFETY * U32 * 3 * ref.abs()
    return ref, bar + _ulp_bf16(ref) if out_bf16 else bar
