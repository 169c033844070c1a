"""The AffinityNet training loss (aff_train.py:111-119 applied to network/resnet38_aff.py:57-63) on the HIP kernels of csrc/aff_loss.hip.

The reference gathers two [N, C, P, n_from] tensors, reduces them to aff = exp(-mean|ft - ff|) and multiplies by three [N, P, n_from] float
label tensors its dataset builds on the host.  Here the labels are one uint8 map [N, h, w] (0 background, 1..20 a class, 255 ignore); the
three indicators of a pair follow from its two label bytes inside the kernels, and loss and gradient are one pass over the feature rows each:

  aff_loss_rows / aff_loss_rows_backward   the engine-layout entry points (pixel rows [N*h*w][ld], f32 or bf16)
  AffinityLoss / affinity_loss             torch.autograd on an [N, C, h, w] feature map (C % 8 == 0, C <= 512)
  pair_labels                              the reference's three label tensors of one map, on the host (numpy)
  aff_label_map                            the label map of two CRF score stacks, on the host (numpy)

The seven scalars `loss, bg_loss, fg_loss, neg_loss, bg_cnt, fg_cnt, neg_cnt` (the keys of aff_train.py's AverageMeter, in its order) and
the gradient are bit-identical from run to run: no kernel accumulates in an order that depends on scheduling.  Nothing synchronises with
the host.  The ELU head under the loss is wseg_amd/aff_head.py (its output is consumed here without a copy); the trainer and CLI are
wseg_amd/aff_train.py; the label map comes from wseg_amd/aff_data.py on the device.
"""
import numpy as np
import torch

from . import _lib as L
from .resnet38_aff import indices_of_pairs, pair_offsets, pair_radius

STATS = ("loss", "bg_loss", "fg_loss", "neg_loss", "bg_cnt", "fg_cnt", "neg_cnt")


def _device_only(t, what):
    if not t.is_cuda:
        raise RuntimeError(f"wseg_amd.aff_loss runs only on an MI355X (HIP) device; there is no CPU fallback ({what} is on {t.device})")


def _label_on(label, device, N, h, w):
    label = torch.as_tensor(label)
    if label.dtype != torch.uint8:
        raise TypeError(f"aff_loss: the label map must be uint8 (0 background, 1..20 a class, 255 ignore), got {label.dtype}")
    if tuple(label.shape) != (N, h, w):
        raise ValueError(f"aff_loss: label map {tuple(label.shape)} for features of {N} x {h} x {w}")
    return label.to(device, non_blocking=True).contiguous()


def aff_loss_rows(rows, ld, C, label, N, h, w, radius=None, with_aff=True):
    """(out7, ctx): the seven scalars (f32, on the device) of pixel rows [N*h*w][ld] (f32 or bf16, channels [0, C) of every row) against the
    label map uint8 [N, h, w].  radius None: the rule of resnet38_aff.pair_radius.  ctx goes to aff_loss_rows_backward and keeps `rows`
    alive (not copied: do not overwrite them in between); with_aff=False skips the [N, P, n_from] affinities (loss only, no backward)."""
    _device_only(rows, "rows")
    r = pair_radius(h, w) if radius is None else int(radius)
    if rows.numel() < (N * h * w - 1) * ld + C or rows.data_ptr() % 16:
        raise ValueError(f"aff_loss_rows: {rows.numel()} elements / address {rows.data_ptr():#x} for {N * h * w} 16-byte aligned rows of ld {ld}")
    nbytes = L.aff_loss_workspace_bytes(N, h, w, r)
    if nbytes < 0:
        raise RuntimeError("aff_loss_rows: " + L.lib.wseg_last_error().decode())
    label = _label_on(label, rows.device, N, h, w)
    ws = torch.empty(nbytes, device=rows.device, dtype=torch.uint8)
    out7 = torch.empty(7, device=rows.device, dtype=torch.float32)
    aff = None
    if with_aff:
        aff = torch.empty(N, L.aff_num_offsets(r), (h - r + 1) * (w - 2 * r + 2), device=rows.device, dtype=torch.float32)
    L.aff_loss_forward(rows, ld, C, label, aff, ws, out7, N, h, w, r)
    return out7, dict(rows=rows, ld=ld, C=C, label=label, aff=aff, out7=out7, N=N, h=h, w=w, radius=r)


def aff_loss_rows_backward(ctx, gscale=None, out=None, ld_d=None):
    """d_rows f32 [N*h*w][ld_d] = gscale * d loss / d rows (gscale: a one-element f32 device tensor, None = 1).  Every row's columns
    [0, C) are written; `out` (ld_d >= C) keeps its columns >= C."""
    if ctx["aff"] is None:
        raise RuntimeError("aff_loss_rows_backward: the forward ran with with_aff=False")
    C, M = ctx["C"], ctx["N"] * ctx["h"] * ctx["w"]
    ld_d = ld_d or (C if out is None else out.shape[-1])
    if out is None:
        out = torch.empty(M, ld_d, device=ctx["rows"].device, dtype=torch.float32)
    if out.dtype != torch.float32 or not out.is_contiguous() or out.numel() < (M - 1) * ld_d + C or out.data_ptr() % 16:
        raise ValueError("aff_loss_rows_backward: `out` must be a contiguous, 16-byte aligned f32 buffer of N*h*w rows of ld_d")
    if gscale is not None:
        _device_only(gscale, "gscale")
        gscale = gscale.reshape(-1)[:1].float().contiguous()
    L.aff_loss_backward(ctx["rows"], ctx["ld"], C, ctx["label"], ctx["aff"], ctx["out7"], gscale, out, ld_d,
                        ctx["N"], ctx["h"], ctx["w"], ctx["radius"])
    return out


class AffinityLoss(torch.autograd.Function):
    """(loss, stats) = AffinityLoss.apply(feat, label, radius): feat [N, C, h, w] f32 / bf16 on the device, label uint8 [N, h, w]."""

    @staticmethod
    def forward(ctx, feat, label, radius=None):
        _device_only(feat, "feat")
        if feat.dim() != 4 or feat.dtype not in (torch.float32, torch.bfloat16):
            raise TypeError(f"affinity_loss: feat must be [N, C, h, w] in float32 or bfloat16, got {tuple(feat.shape)} {feat.dtype}")
        N, C, h, w = feat.shape
        ctx.channels_last = feat.is_contiguous(memory_format=torch.channels_last) and not feat.is_contiguous()
        rows = feat.detach().permute(0, 2, 3, 1)                     # channels_last: already the pixel rows, no copy
        if not rows.is_contiguous() or rows.data_ptr() % 16:
            rows = rows.contiguous() if not rows.is_contiguous() else rows.clone()
        out7, ctx.saved = aff_loss_rows(rows, C, C, label, N, h, w, radius)
        ctx.in_dtype = feat.dtype
        stats = out7.detach()
        ctx.mark_non_differentiable(stats)
        return out7[0].clone(), stats

    @staticmethod
    def backward(ctx, g_loss, _g_stats):
        s = ctx.saved
        d = aff_loss_rows_backward(s, g_loss).view(s["N"], s["h"], s["w"], s["C"]).permute(0, 3, 1, 2)     # NCHW in channels_last strides
        d = d.to(ctx.in_dtype)                                                                             # (keeps the strides)
        return (d if ctx.channels_last else d.contiguous()), None, None


def affinity_loss(feat, label, radius=None):
    """(loss, stats): the reference's AffinityNet loss of the feature map `feat` [N, C, h, w] (the ELU output of f9; f32 or bf16, a
    channels_last tensor is consumed without a copy) against the label map uint8 [N, h, w].  `loss` is differentiable w.r.t. feat (the
    gradient comes back in feat's dtype and memory format); `stats` is the detached 7-vector STATS on the device."""
    return AffinityLoss.apply(feat, label, radius)


# ---------------------------------------------------------------------------------------------- host helpers (numpy)
def pair_labels(label_map, radius):
    """(bg, fg, neg) float32 [P, n_from]: the three outputs of voc12/data.py ExtractAffinityLabelInRadius.__call__ (lines 170-199) for
    an h x w uint8 label map, over the pair set of resnet38_aff.indices_of_pairs (the extractor itself is square-only).  For users of the
    reference's three-tensor contract; the kernels evaluate the same rule per pair from the map."""
    lab = np.asarray(label_map)
    if lab.ndim != 2 or lab.dtype != np.uint8:
        raise TypeError("pair_labels: an [h, w] uint8 label map")
    ind_from, ind_to = indices_of_pairs(radius, lab.shape)
    flat = lab.reshape(-1)
    lf = flat[ind_from][None, :]
    lt = flat[ind_to].reshape(len(pair_offsets(radius)), -1)
    valid = (lf < 255) & (lt < 255)
    pos = lf == lt
    bg = pos & (lf == 0)
    fg = pos & (lf != 0) & valid
    neg = ~pos & valid
    return bg.astype(np.float32), fg.astype(np.float32), neg.astype(np.float32)


def aff_label_map(la_scores, ha_scores):
    """uint8 [h, w] label map from the low-alpha and high-alpha CRF score stacks, [K, h, w] each with plane 0 = background (the layout of
    the .npy files aff_prepare writes): arg-max of each stack; 255 where the low-alpha stack says background; 0 where the high-alpha
    stack says background (its lower threshold leaves fewer, surer background pixels); 255 where no score of either stack reaches 1e-5
    (outside the crop).  Restates voc12/data.py:251-258 — parity with the reference is by reading those lines, not pinned by a fixture:
    there the rule is inline in a dataset's __getitem__ and cannot be called apart from VOC files."""
    la, ha = np.asarray(la_scores), np.asarray(ha_scores)
    if la.ndim != 3 or la.shape != ha.shape:
        raise ValueError(f"aff_label_map: two [K, h, w] score stacks of one shape, got {la.shape} and {ha.shape}")
    no_score = np.maximum(la.max(axis=0), ha.max(axis=0)) < 1e-5
    l_la = np.argmax(la, axis=0).astype(np.uint8)
    l_ha = np.argmax(ha, axis=0).astype(np.uint8)
    label = l_la.copy()
    label[l_la == 0] = 255
    label[l_ha == 0] = 0
    label[no_score] = 255
    return label
