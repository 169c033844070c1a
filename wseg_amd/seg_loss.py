"""The DeepLab-v1 training loss (segmentation/lib/net/deeplabv1.py:50 + experiment/SEAM_deeplabv1_resnet38/train.py:85,97) on the HIP kernels
of csrc/seg_loss.hip.

The reference resamples the stride-8 logits to the label size (F.interpolate, bilinear, align_corners=True) and takes
nn.CrossEntropyLoss(ignore_index=255) of the full-size [N, 21, H, W] tensor.  Here every label pixel samples its image's coarse cls_conv rows
itself; between forward and backward one f32 plane per image is kept (the log-sum-exp), and the gradient is gathered per coarse cell:

  seg_ce_rows / seg_ce_rows_backward     the engine-layout entry points (pixel rows [N*fh*fw][ld], f32 or bf16, as Engine.run_seg_head leaves them)
  SegCrossEntropy / seg_cross_entropy    torch.autograd on a [N, n_cls, fh, fw] logit map

The four scalars `loss, count, nll_sum, out_of_range` and the gradient are bit-identical from run to run: no kernel accumulates in an order
that depends on scheduling (the device's own bilinear backward scatters with atomics).  Nothing synchronises with the host.  A label value in
[n_cls, 255) is ignored like 255 and counted in `out_of_range`; a batch without a valid pixel gives torch's answer (a NaN loss, a zero gradient).
"""
import torch

from . import _lib as L

STATS = ("loss", "count", "nll_sum", "out_of_range")


def _device_only(t, what):
    if not t.is_cuda:
        raise RuntimeError(f"wseg_amd.seg_loss runs only on an MI355X (HIP) device; there is no CPU fallback ({what} is on {t.device})")


def _label_on(label, device, N, H, W):
    label = torch.as_tensor(label)
    if label.dtype not in (torch.uint8, torch.int64):
        raise TypeError(f"seg_loss: the label map must be uint8 or int64 (0 .. n_cls-1 a class, 255 ignore), got {label.dtype}")
    if tuple(label.shape) != (N, H, W):
        raise ValueError(f"seg_loss: label map {tuple(label.shape)} for a batch of {N} and a label size of {H} x {W}")
    label = label.to(device, non_blocking=True)
    if label.dtype != torch.uint8:
        label = label.to(torch.uint8)                 # on the device, no sync, no value check: a bad value shows in stats' out_of_range
    return label.contiguous()


def seg_ce_rows(rows, ld, label, N, fh, fw, H, W, n_cls=21, with_lse=True):
    """(out4, ctx): the four scalars STATS (f32, on the device) of the cls_conv pixel rows [N*fh*fw][ld] (f32 or bf16, the classes in columns
    [0, n_cls) of every row, ld % 8 == 0, 16-byte aligned) against the label map [N, H, W] (uint8, or int64 cast on the device).  ctx goes to
    seg_ce_rows_backward and keeps `rows` alive (not copied: do not overwrite them in between); with_lse=False skips the [N, H, W] log-sum-exp
    plane (loss only, no backward)."""
    _device_only(rows, "rows")
    if rows.data_ptr() % 16:
        raise ValueError(f"seg_ce_rows: rows at {rows.data_ptr():#x} are not 16-byte aligned")
    label = _label_on(label, rows.device, N, H, W)
    nbytes = L.seg_ce_workspace_bytes(N, H, W)
    if nbytes < 0:
        raise RuntimeError("seg_ce_rows: " + L.lib.wseg_last_error().decode())
    ws = torch.empty(nbytes, device=rows.device, dtype=torch.uint8)
    out4 = torch.empty(4, device=rows.device, dtype=torch.float32)
    lse = torch.empty(N, H, W, device=rows.device, dtype=torch.float32) if with_lse else None
    L.seg_ce_forward(rows, ld, label, lse, ws, out4, N, fh, fw, H, W, n_cls)
    return out4, dict(rows=rows, ld=ld, label=label, lse=lse, out4=out4, N=N, fh=fh, fw=fw, H=H, W=W, n_cls=n_cls)


def seg_ce_rows_backward(ctx, gscale=None, out=None, ld_d=None, dtype=torch.float32):
    """d_rows [N*fh*fw][ld_d] = gscale * d loss / d rows, f32 or bf16 (`dtype`, or `out`'s; bf16 is the f32 sum rounded once).  gscale: a
    one-element f32 device tensor, None = 1.  Columns [0, n_cls rounded up to 8) of every row are written, zeros in the columns >= n_cls;
    `out` (ld_d beyond that) keeps its other columns."""
    if ctx["lse"] is None:
        raise RuntimeError("seg_ce_rows_backward: the forward ran with with_lse=False")
    nc8 = (ctx["n_cls"] + 7) // 8 * 8
    M = ctx["N"] * ctx["fh"] * ctx["fw"]
    ld_d = ld_d or (nc8 if out is None else out.shape[-1])
    if out is None:
        out = torch.empty(M, ld_d, device=ctx["rows"].device, dtype=dtype)
    if out.dtype not in (torch.float32, torch.bfloat16) or not out.is_cuda or not out.is_contiguous() or out.numel() < (M - 1) * ld_d + nc8 \
            or out.data_ptr() % 16:
        raise ValueError("seg_ce_rows_backward: `out` must be a contiguous, 16-byte aligned f32 or bf16 device buffer of N*fh*fw rows of ld_d")
    if gscale is not None:
        _device_only(gscale, "gscale")
        gscale = gscale.reshape(-1)[:1].float().contiguous()
    L.seg_ce_backward(ctx["rows"], ctx["ld"], ctx["label"], ctx["lse"], ctx["out4"], gscale, out, ld_d,
                      ctx["N"], ctx["fh"], ctx["fw"], ctx["H"], ctx["W"], ctx["n_cls"])
    return out


class SegCrossEntropy(torch.autograd.Function):
    """(loss, stats) = SegCrossEntropy.apply(coarse, label): coarse [N, n_cls, fh, fw] f32 / bf16 on the device, label [N, H, W] uint8 / int64."""

    @staticmethod
    def forward(ctx, coarse, label):
        _device_only(coarse, "coarse")
        if coarse.dim() != 4 or coarse.dtype not in (torch.float32, torch.bfloat16):
            raise TypeError(f"seg_cross_entropy: coarse must be [N, n_cls, fh, fw] in float32 or bfloat16, got {tuple(coarse.shape)} {coarse.dtype}")
        N, n_cls, fh, fw = coarse.shape
        label = torch.as_tensor(label)
        if label.dim() != 3:
            raise ValueError(f"seg_cross_entropy: label map {tuple(label.shape)} is not [N, H, W]")
        H, W = label.shape[1:]
        nc8 = (n_cls + 7) // 8 * 8
        ctx.channels_last = coarse.is_contiguous(memory_format=torch.channels_last) and not coarse.is_contiguous()
        rows = coarse.detach().permute(0, 2, 3, 1)                   # channels_last with n_cls % 8 == 0: already the pixel rows, no copy
        if n_cls != nc8:                                             # the kernels read whole 8-column chunks: pack into rows of ld = nc8
            packed = torch.zeros(N, fh, fw, nc8, device=coarse.device, dtype=coarse.dtype)
            packed[..., :n_cls] = rows
            rows = packed
        elif not rows.is_contiguous() or rows.data_ptr() % 16:
            rows = rows.contiguous() if not rows.is_contiguous() else rows.clone()
        out4, ctx.saved = seg_ce_rows(rows, nc8, label, N, fh, fw, H, W, n_cls)
        stats = out4.detach()
        ctx.mark_non_differentiable(stats)
        return out4[0].clone(), stats

    @staticmethod
    def backward(ctx, g_loss, _g_stats):
        s = ctx.saved
        d = seg_ce_rows_backward(s, g_loss, dtype=s["rows"].dtype)                                          # in coarse's dtype, rounded once
        d = d.view(s["N"], s["fh"], s["fw"], -1)[..., :s["n_cls"]].permute(0, 3, 1, 2)                       # NCHW over pixel rows
        return d.contiguous(memory_format=torch.channels_last if ctx.channels_last else torch.contiguous_format), None


def seg_cross_entropy(coarse, label):
    """(loss, stats): F.cross_entropy(F.interpolate(coarse, (H, W), mode='bilinear', align_corners=True), label.long(), ignore_index=255) of
    the logit map `coarse` [N, n_cls, fh, fw] (f32 or bf16; a channels_last tensor whose n_cls is a multiple of 8 is consumed without a copy,
    any other is packed once into 8-column-padded pixel rows — a coarse-size copy) against the label map [N, H, W] (uint8, or int64 cast on
    the device without a sync or a value check).  `loss` is differentiable w.r.t. coarse (the gradient comes back in coarse's dtype and memory
    format); `stats` is the detached 4-vector STATS on the device, whose out_of_range entry is where a bad label shows."""
    return SegCrossEntropy.apply(coarse, label)
