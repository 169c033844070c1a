"""float64 restatement of the dense-CRF specification (DESIGN.md §3 "crf"): the mean-field update the reference's pydensecrf calls
define (contrast_infer.py:102-134, aff_prepare.py:34-50), with EXACT all-pairs Gaussian kernels.  The yardstick of tests/test_crf_host.py
and tests/test_gpu_crf.py; torch on the CPU only, written from the specification and never from the kernels.

  U[c, i]   = -ln(gt_prob) where c == labels[i], -ln((1 - gt_prob) / (M - 1)) elsewhere, rounded to float32 (unary_from_labels)
  k(fi, fj) = exp(-|fi - fj|^2 / 2), summed over ALL j (j = i included)
  n_i       = 1 / sqrt(sum_j k(fi, fj) + 1e-20);  filter(Q)[i, c] = n_i * sum_j k(fi, fj) * n_j * Q[j, c]      (NORMALIZE_SYMMETRIC)
  Q_0 = softmax(-U);  logit = -U + w_g * filter_g(Q) + w_b * filter_b(Q);  Q = softmax(logit), t times
"""
import math

import numpy as np
import torch


def features(img_u8, sxy, srgb=None):
    """[N, 2] (Gaussian) or [N, 5] (bilateral) float64 features of an [H, W, 3] uint8 image, pixel i = y * W + x"""
    img = np.asarray(img_u8)
    H, W = img.shape[:2]
    yy, xx = np.mgrid[0:H, 0:W]
    f = [xx.reshape(-1) / float(sxy), yy.reshape(-1) / float(sxy)]
    if srgb is not None:
        f += [img[..., c].reshape(-1).astype(np.float64) / float(srgb) for c in range(3)]
    return torch.as_tensor(np.stack(f, 1), dtype=torch.float64)


def kernel_rows(f, rows):
    """K[rows, :] float64 and the exponent's magnitude A = |fi - fj|^2 / 2 (for error bars)"""
    A = torch.zeros(len(rows), f.shape[0], dtype=f.dtype)
    for d in range(f.shape[1]):
        A += (f[rows, d][:, None] - f[None, :, d]) ** 2
    A *= 0.5
    return torch.exp(-A), A


def kernel_apply(f, X, chunk=1024, moment=False, dtype=torch.float64):
    """K @ X over all pairs, chunked over rows; moment=True also returns (K * A) @ X, A the exponent's magnitude"""
    f = f.to(dtype)
    X = X.to(dtype)
    out = torch.empty_like(X)
    mom = torch.empty_like(X) if moment else None
    for s in range(0, f.shape[0], chunk):
        K, A = kernel_rows(f, torch.arange(s, min(s + chunk, f.shape[0])))
        out[s:s + chunk] = K @ X
        if moment:
            mom[s:s + chunk] = (K * A) @ X
    return (out, mom) if moment else out


def norm(f, dtype=torch.float64):
    """n [N]"""
    return 1.0 / torch.sqrt(kernel_apply(f, torch.ones(f.shape[0], 1), dtype=dtype)[:, 0] + 1e-20)


def filt(f, n, X, dtype=torch.float64):
    """the symmetric-normalised filter of X [N, C]"""
    n = n.to(dtype)
    return n[:, None] * kernel_apply(f, n[:, None] * X.to(dtype), dtype=dtype)


def unary(labels, M=21, gt_prob=0.7):
    """[N, M] float32 energies of a label map"""
    lab = torch.as_tensor(np.asarray(labels).reshape(-1).astype(np.int64))
    U = torch.full((lab.numel(), M), float(-math.log((1.0 - gt_prob) / (M - 1))), dtype=torch.float32)
    U[torch.arange(lab.numel()), lab] = float(-math.log(gt_prob))
    return U


def crf(img_u8, labels, t=10, M=21, gt_prob=0.7, bilateral=(80, 13, 10.0), gaussian=(3, 3.0), dtype=torch.float64):
    """labels [S, H, W] or [H, W] -> dict(Q [S, M, H, W], logits (last iteration), fb / fg (last filter outputs)), all `dtype`"""
    labels = np.asarray(labels)
    if labels.ndim == 2:
        labels = labels[None]
    S, H, W = labels.shape
    N = H * W
    fg, fb = features(img_u8, gaussian[0]), features(img_u8, bilateral[0], bilateral[1])
    ng, nb = norm(fg, dtype), norm(fb, dtype)
    U = torch.cat([unary(labels[s], M, gt_prob) for s in range(S)], 1).to(dtype)          # [N, S*M]
    sm = lambda z: torch.softmax(z.view(N, S, M), 2).view(N, S * M)
    Q = sm(-U)
    lg = -U
    Fg = Fb = torch.zeros_like(Q)
    for _ in range(t):
        Fg, Fb = filt(fg, ng, Q, dtype), filt(fb, nb, Q, dtype)
        lg = -U + gaussian[1] * Fg + bilateral[2] * Fb
        Q = sm(lg)
    shape = lambda z: z.t().reshape(S, M, H, W)
    return dict(Q=shape(Q), logits=shape(lg), fb=shape(Fb), fg=shape(Fg))


def label_tensor(cam_dict, H, W, bg_score=None, alpha=None, M=21):
    """the reference's label map (contrast_infer.py:104-109 / aff_prepare.py:57-63): uint8 [H, W]"""
    tensor = np.zeros((M, H, W), np.float32)
    for key in cam_dict:
        tensor[key + 1] = np.asarray(cam_dict[key], np.float32)
    if alpha is None:
        tensor[0, :, :] = bg_score
    else:
        tensor[0, :, :] = np.power(1 - np.max(tensor, axis=0, keepdims=True), np.float32(alpha))
    return np.argmax(tensor, axis=0).astype(np.uint8)
