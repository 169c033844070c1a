"""Fully connected CRF on the device (csrc/crf.hip): the refinement the reference asks of pydensecrf in contrast_infer.py:102-134
(--out_crf) and aff_prepare.py:34-50.

This is the EXACT mean field of the model those calls define: unary_from_labels(gt_prob, zero_unsure=False), a Potts Gaussian term
(x/sxy, y/sxy) and a Potts bilateral term (x/sxy, y/sxy, r/srgb, g/srgb, b/srgb), both DIAG_KERNEL + NORMALIZE_SYMMETRIC, every pair
of pixels evaluated.  pydensecrf approximates the same filters with a permutohedral lattice; agreement with pydensecrf's permutohedral
approximation is unmeasured (the package is not available offline).  DESIGN.md §3 states the update.

There is no CPU fallback: tensors live on the device, a missing kernel is an error.  Nothing here synchronises.
"""
import numpy as np
import torch

from . import _lib as L
from .stage_io import cam_planes

MAX_SETS_PER_PASS = L.CRF_MAX_COLUMNS // 21      # label sets of 21 labels that share one pass over the pairs


def bg_rule(bg_score=None, alpha=None):
    """(rule code, parameter) of the background plane: a constant score (contrast_infer.py:108), or (1 - max_c cam)^alpha
    (aff_prepare.py:61).  Exactly one of the two must be given."""
    if (bg_score is None) == (alpha is None):
        raise ValueError("labels_from_cams: give exactly one of bg_score= / alpha=")
    if bg_score is not None:
        return L.CRF_BG_CONST, float(bg_score)
    return L.CRF_BG_POWER, float(alpha)


@torch.no_grad()
def labels_from_cams(cam_dict, bg_score=None, alpha=None, size=None, n_labels=21, device="cuda"):
    """cam_dict {class 0..19: float [H, W]} (numpy or torch, what contrast_infer writes) -> uint8 device labels: the arg-max over
    [background] ++ classes, absent classes at 0.  bg_score=x: constant background, [H, W].  alpha=a: background (1 - max)^a, [H, W];
    alpha=(a0, a1, ...): one label set per exponent, [S, H, W]."""
    many = alpha is not None and not np.isscalar(alpha)
    rules = [bg_rule(None, a) for a in alpha] if many else [bg_rule(bg_score, alpha)]
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError("labels_from_cams runs on the device only (wseg_amd has no CPU fallback)")
    cams, idx, (H, W) = cam_planes(cam_dict, size, device, n_labels - 1)
    src = [-1] + idx
    out = torch.empty(len(rules), H, W, device=device, dtype=torch.uint8)
    with torch.cuda.device(device):
        for s, (rule, param) in enumerate(rules):
            L.crf_labels(cams, src, n_labels, rule, param, out[s], H * W)
    return out if many else out[0]


class _Image:
    """the per-image state every label set shares: features, both normalisations"""

    def __init__(self, img_u8, gauss_sxy, sxy, srgb):
        if img_u8.dtype != torch.uint8 or img_u8.dim() != 3 or img_u8.shape[2] != 3 or not img_u8.is_cuda:
            raise ValueError(f"img_u8 must be a uint8 [H, W, 3] device tensor, got {img_u8.dtype} {tuple(img_u8.shape)} on {img_u8.device}")
        self.img = img_u8.contiguous()
        self.H, self.W = int(img_u8.shape[0]), int(img_u8.shape[1])
        self.N = self.H * self.W
        self.npad = L.crf_padded_pixels(self.N)
        self.sxy, self.srgb, self.gauss_sxy = float(sxy), float(srgb), float(gauss_sxy)
        dev = img_u8.device
        f32 = dict(device=dev, dtype=torch.float32)
        self.feat = torch.empty(self.npad // 4, 8, 4, **f32)
        ones = torch.empty(self.npad // 4, 16, 4, **f32)
        self.ng = torch.empty(self.N, **f32)
        L.crf_prepare(self.img, self.H, self.W, self.gauss_sxy, self.feat, ones, self.ng)
        sums = torch.empty(self.npad, 16, **f32)
        L.crf_bilateral(self.feat, ones, sums, self.N, 16, self.sxy, self.srgb)
        self.nb = torch.empty(self.N, **f32)
        L.crf_rsqrt(sums, 16, self.nb, self.N)


def _mean_field(im, labels, t, n_labels, gt_prob, wb, wg, want_logits, prob=None):
    """t mean-field iterations of S label sets (labels [S, H, W]) or, with prob [n_labels, H, W], of the one set whose unary is
    unary_from_softmax(prob) (labels, gt_prob unused) — the same filters and the same update kernel body either way."""
    S, N = (1 if prob is not None else labels.shape[0]), im.N
    NC = L.crf_columns(S, n_labels)
    f32 = dict(device=im.img.device, dtype=torch.float32)
    Qn = torch.empty(im.npad // 4, NC, 4, **f32)
    Qg = torch.empty(S * n_labels, N, **f32)
    outb = torch.empty(im.npad, NC, **f32)
    outg, tmp = torch.empty_like(Qg), torch.empty_like(Qg)
    Q = torch.empty(S, n_labels, im.H, im.W, **f32)
    logits = torch.empty_like(Q) if want_logits else None
    amax = torch.empty(S, im.H, im.W, device=im.img.device, dtype=torch.uint8)

    def update(ob, og, last):
        outs = (Q if last else None, logits if last else None, amax if last else None)
        if prob is not None:
            L.crf_update_prob(prob, ob, og, im.nb, im.ng, Qn, Qg, *outs, n_labels, N, wb, wg)
        else:
            L.crf_update(labels, ob, og, im.nb, im.ng, Qn, Qg, *outs, S, n_labels, N, gt_prob, wb, wg)

    update(None, None, t == 0)
    for it in range(t):
        L.crf_bilateral(im.feat, Qn, outb, N, NC, im.sxy, im.srgb)
        L.crf_gaussian(Qg, tmp, outg, S * n_labels, im.H, im.W, im.gauss_sxy)
        update(outb, outg, it == t - 1)
    return Q, logits, amax


@torch.no_grad()
def crf_inference(img_u8, labels, t=10, n_labels=21, gt_prob=0.7, bilateral=(80, 13, 10), gaussian=(3, 3), return_logits=False,
                  return_argmax=False):
    """Mean-field inference of the reference's _crf_inference(img, labels, t, n_labels, gt_prob) with exact kernels.
    img_u8 [H, W, 3] uint8 and labels [S, H, W] or [H, W] uint8, both on the device; bilateral = (sxy, srgb, compat), gaussian =
    (sxy, compat) — contrast_infer uses (50, 5, 10), aff_prepare (80, 13, 10), both (3, 3).  Returns Q [S, n_labels, H, W] float32 on
    the device (S = 1 for [H, W] labels); with return_logits / return_argmax also the last iteration's logits (same shape) and the
    uint8 [S, H, W] arg-max.  The S label sets share every kernel evaluation, MAX_SETS_PER_PASS of them per pass over the pairs."""
    if not 2 <= n_labels <= L.CRF_MAX_LABELS:
        raise ValueError(f"n_labels={n_labels} outside [2, {L.CRF_MAX_LABELS}]")
    if int(t) != t or t < 0:
        raise ValueError(f"t={t} is not a non-negative integer")
    if labels.dim() == 2:
        labels = labels.unsqueeze(0)
    if labels.dtype != torch.uint8 or labels.dim() != 3 or labels.device != img_u8.device:
        raise ValueError(f"labels must be uint8 [S, H, W] or [H, W] on the image's device, got {labels.dtype} {tuple(labels.shape)}")
    if tuple(labels.shape[1:]) != tuple(img_u8.shape[:2]):
        raise ValueError(f"labels {tuple(labels.shape[1:])} and image {tuple(img_u8.shape[:2])} differ in size")
    labels = labels.contiguous()
    (sxy, srgb, wb), (gsxy, wg) = bilateral, gaussian
    with torch.cuda.device(img_u8.device):
        im = _Image(img_u8, gsxy, sxy, srgb)
        per = max(1, L.CRF_MAX_COLUMNS // n_labels)
        parts = [_mean_field(im, labels[s:s + per], int(t), n_labels, float(gt_prob), float(wb), float(wg), return_logits)
                 for s in range(0, labels.shape[0], per)]
    Q, logits, amax = parts[0] if len(parts) == 1 else tuple(torch.cat(x) if x[0] is not None else None for x in zip(*parts))
    out = (Q,) + ((logits,) if return_logits else ()) + ((amax,) if return_argmax else ())
    return out[0] if len(out) == 1 else out


@torch.no_grad()
def crf_inference_from_probs(img_u8, prob, t=1, bilateral=(32, 13, 10), gaussian=(3, 3), return_logits=False, return_argmax=False):
    """Mean-field inference of the DeepLab stage's dense_crf(probs, img, n_iters=1) (segmentation/lib/utils/DenseCRF.py:5-39) with exact
    kernels: unary_from_softmax, U = -ln(clip(p, 1e-5, 1)), a Gaussian term (sxy 3, compat 3) and a bilateral term (sxy 32, srgb 13,
    compat 10).  img_u8 [H, W, 3] uint8 and prob [M, H, W] float32 (2 <= M <= 32), both on the device.  Returns Q [M, H, W] float32 on
    the device; with return_logits / return_argmax also the last iteration's logits and the uint8 [H, W] arg-max."""
    if prob.dim() != 3 or prob.dtype != torch.float32 or prob.device != img_u8.device:
        raise ValueError(f"prob must be float32 [M, H, W] on the image's device, got {prob.dtype} {tuple(prob.shape)}")
    M = int(prob.shape[0])
    if not 2 <= M <= L.CRF_MAX_LABELS:
        raise ValueError(f"prob has {M} planes, outside [2, {L.CRF_MAX_LABELS}]")
    if int(t) != t or t < 0:
        raise ValueError(f"t={t} is not a non-negative integer")
    if tuple(prob.shape[1:]) != tuple(img_u8.shape[:2]):
        raise ValueError(f"prob {tuple(prob.shape[1:])} and image {tuple(img_u8.shape[:2])} differ in size")
    (sxy, srgb, wb), (gsxy, wg) = bilateral, gaussian
    with torch.cuda.device(img_u8.device):
        im = _Image(img_u8, gsxy, sxy, srgb)
        Q, logits, amax = _mean_field(im, None, int(t), M, None, float(wb), float(wg), return_logits, prob=prob.contiguous())
    out = (Q[0],) + ((logits[0],) if return_logits else ()) + ((amax[0],) if return_argmax else ())
    return out[0] if len(out) == 1 else out


# ---- the two filters on their own (tests, scripts/bench_crf.py): planes [C, H, W] in, the symmetric-normalised filter out
@torch.no_grad()
def bilateral_norm(img_u8, sxy, srgb):
    """n [H, W] = 1 / sqrt(sum_j k(f_i, f_j) + 1e-20) of the bilateral kernel"""
    with torch.cuda.device(img_u8.device):
        im = _Image(img_u8, 3.0, sxy, srgb)
    return im.nb.view(im.H, im.W)


@torch.no_grad()
def bilateral_filter(img_u8, planes, sxy, srgb, image_state=None):
    """planes [C, H, W] float32 (C <= 64) -> n_i * sum_j k(f_i, f_j) * n_j * planes[c][j], all pairs"""
    with torch.cuda.device(img_u8.device):
        return _bilateral_filter(img_u8, planes, sxy, srgb, image_state)


def _bilateral_filter(img_u8, planes, sxy, srgb, image_state):
    im = image_state or _Image(img_u8, 3.0, sxy, srgb)
    C = int(planes.shape[0])
    NC = L.crf_columns(C, 1)
    if NC > L.CRF_MAX_COLUMNS or tuple(planes.shape[1:]) != (im.H, im.W):
        raise ValueError(f"planes {tuple(planes.shape)}: at most {L.CRF_MAX_COLUMNS} planes of {(im.H, im.W)}")
    x = torch.zeros(NC, im.npad, device=planes.device, dtype=torch.float32)
    x[:C, :im.N] = planes.reshape(C, im.N).float() * im.nb
    Qn = x.view(NC, im.npad // 4, 4).permute(1, 0, 2).contiguous()
    out = torch.empty(im.npad, NC, device=planes.device, dtype=torch.float32)
    L.crf_bilateral(im.feat, Qn, out, im.N, NC, im.sxy, im.srgb)
    return (out[:im.N, :C].t() * im.nb).reshape(C, im.H, im.W)


@torch.no_grad()
def gaussian_norm(img_u8, sxy):
    with torch.cuda.device(img_u8.device):
        im = _Image(img_u8, sxy, 80.0, 13.0)
    return im.ng.view(im.H, im.W)


@torch.no_grad()
def gaussian_filter(planes, sxy, ng):
    """planes [C, H, W] float32, ng [H, W] from gaussian_norm -> the symmetric-normalised spatial filter"""
    C, H, W = planes.shape
    x = (planes.float() * ng).contiguous()
    tmp, out = torch.empty_like(x), torch.empty_like(x)
    with torch.cuda.device(planes.device):
        L.crf_gaussian(x, tmp, out, C, H, W, float(sxy))
    return out * ng
