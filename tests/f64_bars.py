"""Shared pieces of the kernel-by-kernel GPU tests (test_gpu_loss_kernels.py, test_gpu_pcm_head_kernels.py): the f32 unit
roundoff, the safety factor every derived bar carries, and the bars of one bilinear sample.  TEST INFRASTRUCTURE, no tests here."""
import torch

U32 = 2.0 ** -24          # f32 unit roundoff
SAFETY = 2.0              # the safety factor on every derived bar


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _bits(col):
    """an index the kernels store as the bits of an int in a float slot"""
    return col.contiguous().view(torch.int32).long()


def _coord_bar(n_in):
    # |delta f| of an f32 source coordinate s = f32(scale) * o (two roundings, s < n_in): 2 u n_in.  align=False adds the
    # -0.5 subtraction and (o + 0.5) stays exact: 3 u (n_in + 1) covers both modes.
    return 3.0 * U32 * (n_in + 1)


def _interp_bar(h, w, M):
    """|U_f32 - U_64| of one bilinear sample of values bounded by M: per axis |delta f| * |p1 - p0| <= coord * 2M, plus
    six roundings (two (1-f), two products, two fma / adds) of magnitude <= M."""
    return SAFETY * (2.0 * _coord_bar(max(h, w)) * 2.0 * M + 6.0 * U32 * M)
