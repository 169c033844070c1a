"""float64 restatement of the DeepLab stage's multi-scale collect step (segmentation/experiment/SEAM_deeplabv1_resnet38/test.py:84-103 with
deeplabv1.py:50), written from that math and never from the kernel: per pass the coarse logits are resampled bilinearly
(align_corners=True) to the scaled input size, resampled again to the original size, an odd (flipped) entry is flipped back, then mean
over the passes, softmax over the classes, arg-max.  The yardstick of tests/test_seg_host.py and tests/test_gpu_seg_fuse.py, with the
bar an f32 evaluation of the same math may differ by.  TEST INFRASTRUCTURE, no tests here."""
import torch

from tests.f64_bars import SAFETY, U32, _coord_bar, _interp_bar


def _axis(n_in, n_out):
    """align_corners=True source coordinates: (i0, i1, f) of the n_out output positions, exact in float64"""
    s = torch.arange(n_out, dtype=torch.float64) * ((n_in - 1) / (n_out - 1) if n_out > 1 else 0.0)
    i0 = s.floor().clamp_(max=n_in - 1).long()
    i1 = (i0 + 1).clamp_(max=n_in - 1)
    return i0, i1, s - i0


def resize(x, oh, ow):
    """[..., h, w] -> [..., oh, ow] float64, bilinear with align_corners=True"""
    x = x.double()
    y0, y1, fy = _axis(x.shape[-2], oh)
    x0, x1, fx = _axis(x.shape[-1], ow)
    rows = x[..., y0, :] * (1 - fy)[:, None] + x[..., y1, :] * fy[:, None]
    return rows[..., x0] * (1 - fx) + rows[..., x1] * fx


def fuse(passes, H, W):
    """passes: [(coarse [C, fh, fw], (ih, iw), flip)] in the reference's order -> dict(mean [C, H, W], prob, amax [H, W] int64 (the first
    maximum), margin [H, W] = top-1 minus top-2 of the mean), float64"""
    maps = []
    for coarse, (ih, iw), flip in passes:
        m = resize(resize(coarse, ih, iw), H, W)
        maps.append(m.flip(-1) if flip else m)
    mean = torch.stack(maps).mean(0)
    top2 = torch.topk(mean, 2, dim=0).values
    return dict(mean=mean, prob=torch.softmax(mean, 0), amax=torch.argmax(mean, 0), margin=top2[0] - top2[1])


def fuse_bar(passes, M):
    """|mean_f32 - mean_64| of `fuse` evaluated in float32 on logits bounded by M: per pass the bilinear bar of tests/f64_bars.py applied
    twice (stage 1 on the coarse grid; stage 2 on the intermediate grid, whose inputs carry stage 1's error with weights that sum to 1),
    the largest over the passes; then the n - 1 roundings of the running sum (partial sums bounded by n M) and the division's, over n."""
    n = len(passes)
    per_pass = max(_interp_bar(c.shape[-2], c.shape[-1], M) + _interp_bar(ih, iw, M) for c, (ih, iw), _f in passes)
    return per_pass + SAFETY * n * U32 * M


def _step(x):
    """the largest |difference| of two neighbours of [..., h, w], along either axis"""
    x = x.double()
    dy = float((x[..., 1:, :] - x[..., :-1, :]).abs().max()) if x.shape[-2] > 1 else 0.0
    dx = float((x[..., :, 1:] - x[..., :, :-1]).abs().max()) if x.shape[-1] > 1 else 0.0
    return max(dy, dx)


def fuse_bar_local(passes):
    """`fuse_bar` for THESE logits instead of any logits bounded by M: the same terms, with what the worst case puts at 2M — |p1 - p0| of
    the two samples an interpolation blends, which the source coordinate's rounding error multiplies — replaced by the largest neighbour
    difference the pass's grid really has (stage 1: of the coarse logits; stage 2: of their float64 resample to the scaled input size),
    and M by the pass's own max |logit|.  Never above fuse_bar(passes, max |logit|); on the fixtures of
    tests/test_seg_host.py (a net's stride-8 logits resampled 8x) 6-12x below it."""
    def sample(n_in, D, M):                  # f64_bars._interp_bar with D for 2M
        return SAFETY * (2.0 * _coord_bar(n_in) * D + 6.0 * U32 * M)
    per_pass, Mx = 0.0, 0.0
    for c, (ih, iw), _f in passes:
        M = float(c.abs().max())
        Mx = max(Mx, M)
        per_pass = max(per_pass, sample(max(c.shape[-2:]), _step(c), M) + sample(max(ih, iw), _step(resize(c, ih, iw)), M))
    return per_pass + SAFETY * len(passes) * U32 * Mx
