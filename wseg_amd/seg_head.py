"""The DeepLab-v1 head in training mode: segmentation/lib/net/deeplabv1.py:42-49 — conv_fov (3x3, dilation 12) -> bn_fov -> ReLU -> conv_fov2 ->
bn_fov2 -> ReLU -> Dropout(0.5) -> cls_conv — with both BatchNorms on BATCH statistics (train.py:52 builds the net with plain nn.BatchNorm2d
on one GPU), forward with a saved context and backward down to t = relu(bn7(conv6)), where Engine.run_trunk_backward takes over.

  seg_head_forward / seg_head_backward   the engine-layout entry points (pixel rows in the dtype of the net's precision mode)
  SegHead / seg_head                     torch.autograd on an NCHW device tensor; the output is a channels_last view of the cls_conv rows
  backward_launches                      the GEMM launches of the backward as descriptors (what L.conv_plan / L.wgrad_plan take)

The forward is Engine.run_seg_head_train: the conv launches of inference writing raw sums, csrc/seg_head.hip in between (batch statistics with
the running update, the fold, ReLU, the counter-hash dropout mask of `drop_key`: synth.dropout_keep is its host restatement).  The backward:
  d_bias += column sums of d_rows                                  csrc/seg_head.hip col_sums (21 of the 24 columns)
  dW_cls += y2^T d_rows;  d_y2 = d_rows W_cls                      L.conv_wgrad (OC_dw 21) / L.conv_igemm mode 1
  dz2 = BN-ReLU-dropout backward of d_y2                           csrc/seg_head.hip bn_relu_backward, in place (s = 1 / (1 - p))
  dW_fov2 += y1^T dz2;  d_y1 = dz2 W_fov2
  dz1 = BN-ReLU backward of d_y1                                   in place (s = 1)
  dW_fov += t^T dz1 (3x3, dilation 12);  d_t = the 3x3 data gradient at dilation 12
The conv launch walks K in 128-byte rows, so cls_conv's data gradient cannot read 24-column rows: d_rows is copied (and cast to the mode's
dtype) into a buffer zero-padded to Engine.SEG_CLS_DGRAD_K columns, which the weight gradient reads too (ld_dy).  Conv weight gradients
ACCUMULATE into the engine's flat gradient buffer (Engine.grad_slice; attach_grads makes them the parameters' .grad); cls_conv.bias.grad and
the BatchNorms' weight.grad / bias.grad (by-products of the reduction: the reference's optimizer never sees them) accumulate as ordinary
tensors.  d_t takes the optional bn7-ReLU operands (scale / mask / drop: epilogue 1), as aff_head_backward's f8_5 gradient does.  Everything
outside the conv weight gradients (some of whose kernels add with float atomics) is bit-identical from run to run.  Nothing synchronises with
the host.  The rest of the stage — the backbone's backward from d_t, the data path, the trainer — does not exist yet.
"""
import functools

import torch

from . import arch
from . import _lib as L
from .engine import DT_OF, Engine, device_only, grad_to_rows, head_backward_launchers, head_conv, nchw_to_rows, rows_to_nchw

CONVS = tuple(arch.SEG_HEAD_CONVS)                                  # conv_fov, conv_fov2, cls_conv
_device_only = functools.partial(device_only, "seg_head")


def _conv(name, dims, cout=None):
    co, ci, k = arch.SEG_HEAD_CONVS[name]
    return head_conv(name, ci, cout or co, dims, k=k, dil=arch.SEG_HEAD_DILATION if k > 1 else 1)


def backward_launches(N, h, w, dt, epi1=False):
    """{launch: keywords} of the six GEMM launches of seg_head_backward on an N x h x w map in precision code `dt` (L.F32 / L.BF16 / L.F32X3), in
    launch order: "wgrad_<conv>" are keywords of L.conv_wgrad / L.wgrad_plan, "dgrad_<conv>" of L.conv_igemm / L.conv_plan (tensors and the
    epilogue operands aside).  epi1: the conv_fov data gradient with scale / mask / drop (epilogue 1)."""
    dims, K = [(h, w)], Engine.SEG_CLS_DGRAD_K
    out = {}
    out["wgrad_cls_conv"] = dict(_conv("cls_conv", dims, arch.SEG_CLS_ROWS).wgrad_kw(N), ld_dy=K, OC_dw=arch.NUM_CLASSES, dtype=dt)
    out["dgrad_cls_conv"] = dict(_conv("cls_conv", dims, K).dgrad_kw(N), dtype=dt)
    for name in ("conv_fov2", "conv_fov"):
        c = _conv(name, dims)
        out["wgrad_" + name] = dict(c.wgrad_kw(N), dtype=dt)
        out["dgrad_" + name] = dict(c.dgrad_kw(N), epi=1 if (epi1 and name == "conv_fov") else 0, dtype=dt)
    return out


def seg_head_forward(net, t, N, h, w, drop_key):
    """(rows [M, 24], ctx) of the pixel rows t = relu(bn7(conv6)) [M, 4096] (M = N * h * w, contiguous, the dtype of net.precision); rows: the 21
    logits and three zero columns, as in inference.  Updates bn_fov's / bn_fov2's running statistics and num_batches_tracked.  drop_key: the
    32-bit key of this step's dropout mask (synth.dropout_key).  ctx goes to seg_head_backward and keeps t alive (not copied)."""
    _device_only(t, "t")
    if not (net.training and net.bn_fov.training and net.bn_fov2.training):
        raise RuntimeError("seg_head_forward is the TRAINING path (batch statistics, dropout): call net.train() first; "
                           "inference is Net.coarse_logits / Engine.run_seg_head")
    tdt = L.TORCH_DTYPE[DT_OF[net.precision]]
    if t.dtype != tdt or tuple(t.shape) != (N * h * w, 4096) or not t.is_contiguous():
        raise ValueError(f"seg_head_forward: t must be contiguous {tdt} rows [{N * h * w}, 4096], got {tuple(t.shape)} {t.dtype}")
    eng = net._engine.active(t.device)
    rows, saved = eng.run_seg_head_train(t, [(h, w)], N, drop_key)
    p = float(net.dropout1.p)
    ctx = dict(saved, eng=eng, dt=DT_OF[net.precision], N=N, h=h, w=w, t=t, rows=rows, drop_s=1.0 / (1.0 - p), drop_key=drop_key)
    ctx.update(mean1=saved["stats1"][0], invstd1=saved["stats1"][1], mean2=saved["stats2"][0], invstd2=saved["stats2"][1])
    return rows, ctx


def _accumulate(param, g):
    if param.requires_grad:
        if param.grad is None:
            param.grad = g.clone()
        else:
            param.grad += g


def seg_head_backward(ctx, d_rows, scale=None, mask=None, drop=None, capture=None):
    """d_t [M, 4096] in the engine's dtype from d_rows [M, ld >= 24] (f32 as seg_ce_rows_backward writes it, or the engine's dtype; the columns
    >= 21 are not read as classes); adds the three conv weight gradients to the flat gradient buffer, cls_conv's bias gradient and the BatchNorm
    gradients to their .grad.  scale [4096] / mask [M, 4096] / drop [N, 4096]: the BN-ReLU backward operands of the conv_fov data gradient
    (d_t * scale[c] * drop[n, c] * (mask > 0)).  capture: a dict that receives d_pad, d_y2, dz2, d_y1, dz1 (copies where a later launch
    overwrites them), d_bias, the BatchNorm gradients and the plans of the data-gradient launches (tests)."""
    eng, dt, N, h, w = ctx["eng"], ctx["dt"], ctx["N"], ctx["h"], ctx["w"]
    M, K, NC = N * h * w, Engine.SEG_CLS_DGRAD_K, arch.NUM_CLASSES
    tdt = L.TORCH_DTYPE[dt]
    _device_only(d_rows, "d_rows")
    if d_rows.dim() != 2 or d_rows.shape[0] != M or d_rows.shape[1] < arch.SEG_CLS_ROWS or d_rows.stride(1) != 1 \
            or d_rows.dtype not in (torch.float32, tdt):
        raise ValueError(f"seg_head_backward: d_rows must be [{M}, >= {arch.SEG_CLS_ROWS}] rows in float32 or {tdt}, "
                         f"got {tuple(d_rows.shape)} {d_rows.dtype}")
    dev, net = d_rows.device, eng.net
    P = eng.head_wt(dev)
    eng.attach_grads()
    launches = backward_launches(N, h, w, dt, epi1=any(o is not None for o in (scale, mask, drop)))
    wgrad, dgrad = head_backward_launchers(eng, P, launches, capture)
    ws = torch.empty(L.bn_stats_workspace_bytes(M, 512), device=dev, dtype=torch.uint8)

    def bn_backward(i, g, s):
        bn = eng.bn_module(arch.SEG_HEAD_BNS[CONVS[i - 1]][0])
        dgb = torch.empty(2, 512, device=dev, dtype=torch.float32)
        L.bn_relu_backward(g, 512, ctx[f"y{i}"], 512, ctx[f"z{i}"], 512, ctx[f"mean{i}"], ctx[f"invstd{i}"], bn.weight.detach(), s, g, 512,
                           dgb[0], dgb[1], M, 512, ws)
        _accumulate(bn.weight, dgb[0])
        _accumulate(bn.bias, dgb[1])
        if capture is not None:
            capture[f"d_gamma{i}"], capture[f"d_beta{i}"] = dgb[0], dgb[1]

    d_bias = torch.empty(NC, device=dev, dtype=torch.float32)
    L.col_sums(d_rows, d_rows.stride(0), M, NC, d_bias, ws)
    _accumulate(net.cls_conv.bias, d_bias)
    d_pad = torch.zeros(M, K, device=dev, dtype=tdt)
    d_pad[:, :NC].copy_(d_rows[:, :NC])
    wgrad("cls_conv", ctx["y2"], d_pad)
    d_y2 = torch.empty(M, 512, device=dev, dtype=tdt)
    dgrad("cls_conv", d_pad, d_y2)
    if capture is not None:
        capture.update(d_bias=d_bias, d_pad=d_pad, d_y2=d_y2.clone())
    bn_backward(2, d_y2, ctx["drop_s"])
    dz2 = d_y2
    wgrad("conv_fov2", ctx["y1"], dz2)
    d_y1 = torch.empty(M, 512, device=dev, dtype=tdt)
    dgrad("conv_fov2", dz2, d_y1)
    if capture is not None:
        capture.update(dz2=dz2, d_y1=d_y1.clone())
    bn_backward(1, d_y1, 1.0)
    dz1 = d_y1
    wgrad("conv_fov", ctx["t"], dz1)
    d_t = torch.empty(M, 4096, device=dev, dtype=tdt)
    dgrad("conv_fov", dz1, d_t, **(dict(scale=scale, mask=mask, drop=drop) if launches["dgrad_conv_fov"]["epi"] else {}))
    if capture is not None:
        capture.update(dz1=dz1)
    return d_t


class SegHead(torch.autograd.Function):
    """logits = SegHead.apply(conv6, anchor, net, drop_key): see seg_head."""

    @staticmethod
    def forward(ctx, conv6, anchor, net, drop_key):
        N, _, h, w = conv6.shape
        rows, ctx.saved = seg_head_forward(net, nchw_to_rows(conv6, L.TORCH_DTYPE[DT_OF[net.precision]]), N, h, w, drop_key)
        ctx.in_dtype = conv6.dtype
        ctx.set_materialize_grads(False)
        return rows_to_nchw(rows, N, h, w, rows.dtype)

    @staticmethod
    def backward(ctx, g):
        if g is None:
            return None, None, None, None
        s = ctx.saved
        N, h, w = s["N"], s["h"], s["w"]
        d_t = seg_head_backward(s, grad_to_rows(g, L.TORCH_DTYPE[s["dt"]]))
        return (rows_to_nchw(d_t, N, h, w, ctx.in_dtype) if ctx.needs_input_grad[0] else None), None, None, None


def seg_head(net, conv6, drop_key):
    """The training-mode logit map [N, 24, h, w] (a channels_last view of the engine's cls_conv rows, in the dtype of net.precision: channels
    0..20 are the classes, 21..23 zero padding) of the NCHW device tensor conv6 [N, 4096, h, w] (= relu(bn7(.)), what the backbone hands the head).
    Differentiable: gradients flow to conv6 and, through the engine's flat gradient buffer, to the three head weights; cls_conv.bias and the two
    BatchNorms get ordinary .grad tensors.  seg_loss.seg_ce_rows reads the rows behind the view as they are (ld 24, n_cls 21);
    seg_loss.seg_cross_entropy takes the slice [:, :21] (which it packs: a coarse-size copy)."""
    _device_only(conv6, "conv6")
    if conv6.dim() != 4 or conv6.shape[1] != 4096:
        raise ValueError(f"seg_head: conv6 must be [N, 4096, h, w], got {tuple(conv6.shape)}")
    eng = net._engine.active(conv6.device)
    anchor = eng.flat_w.new_zeros((), requires_grad=torch.is_grad_enabled())       # the weights live in the flat buffer: keeps the node in the graph
    return SegHead.apply(conv6, anchor, net, drop_key)
