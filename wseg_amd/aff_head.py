"""The AffinityNet head in training mode: the four 1x1 ELU convs f8_3, f8_4, f8_5, f9 of network/resnet38_aff.py:39-42, forward with a
saved context and backward down to the three tensors the backbone hands the head.

  aff_head_forward / aff_head_backward   the engine-layout entry points (pixel rows in the dtype of the net's precision mode)
  AffinityHead / affinity_head           torch.autograd on NCHW device tensors; the output is a channels_last view of the f9 rows, which
                                         wseg_amd.aff_loss.affinity_loss consumes without a copy
  backward_launches                      the GEMM launches of the backward as descriptors (what L.conv_plan / L.wgrad_plan take)

The forward is Engine.run_aff_head — the launches of inference, so f9 is bit for bit what Net.affinities computes — and keeps feat (the
three ELU outputs side by side, [M, 448]) and f9: ELU's derivative follows from its OUTPUT (1 above zero, y + 1 below), no pre-activation
is stored.  The backward:
  dz9    = elu'(f9) . gscale . d_f9          csrc/aff_head.hip (also the f32 -> bf16 cast of the loss gradient in bf16 mode)
  dW_f9 += feat^T dz9;   d_feat = dz9 W_f9   L.conv_wgrad / L.conv_igemm mode 1
  dzf    = elu'(feat) . d_feat               csrc/aff_head.hip, in place
  per branch f8_3 / f8_4 / f8_5 on the column slice [0,64) / [64,192) / [192,448) of dzf (ld 448, as the forward writes them):
  dW += x^T dzf_slice;  d_x = dzf_slice W    -> d_conv4 [M,512], d_conv5 [M,1024], d_t [M,4096]
Weight gradients ACCUMULATE into the engine's flat gradient buffer (Engine.grad_slice; attach_grads makes them the parameters' .grad).
The f8_5 data gradient takes the optional BN-ReLU backward operands of the contrast head's data gradient (scale / mask / drop: epilogue
1), so that the backbone's backward can later fold bn7's ReLU in; with none it is the plain gradient w.r.t. t = relu(bn7(conv6)).
Every data gradient and its weight gradient are two launches (the joint grid of wseg_conv_bwd_pair is not used here).  Nothing
synchronises with the host.  The rest of the step — the backbone's backward with gradient taps, trainer, CLI — is wseg_amd/aff_train.py.
"""
import functools

import torch

from . import arch
from . import _lib as L
from .engine import AFF_FEAT_C, AFF_FEAT_SLICES, DT_OF, device_only, grad_to_rows, head_backward_launchers, head_conv, nchw_to_rows, rows_to_nchw

BRANCHES = (("f8_3", "conv4"), ("f8_4", "conv5"), ("f8_5", "t"))     # (conv, the name of its input in the context)
_device_only = functools.partial(device_only, "aff_head")

def _conv(name, dims):
    cout, cin = arch.AFF_HEAD_CONVS[name]
    return head_conv(name, cin, cout, dims)


def backward_launches(N, h, w, dt, epi1=False):
    """{launch: keywords} of the eight GEMM launches of aff_head_backward on an N x h x w map in precision code `dt` (L.F32 / L.BF16 / L.F32X3),
    in launch order: "wgrad_<conv>" are keywords of L.conv_wgrad / L.wgrad_plan, "dgrad_<conv>" of L.conv_igemm / L.conv_plan (tensors and
    the epilogue operands aside).  epi1: the f8_5 data gradient with scale / mask / drop (epilogue 1)."""
    dims = [(h, w)]
    out = {}
    c9 = _conv("f9", dims)
    out["wgrad_f9"] = dict(c9.wgrad_kw(N), dtype=dt)
    out["dgrad_f9"] = dict(c9.dgrad_kw(N), dtype=dt)
    for name, _ in BRANCHES:
        c = _conv(name, dims)
        out["wgrad_" + name] = dict(c.wgrad_kw(N), ld_dy=AFF_FEAT_C, dtype=dt)
        out["dgrad_" + name] = dict(c.dgrad_kw(N), ld_in=AFF_FEAT_C, epi=1 if (epi1 and name == "f8_5") else 0, dtype=dt)
    return out


def aff_head_forward(net, conv4, conv5, t, N, h, w):
    """(f9_rows [M, 448], ctx) of the pixel rows conv4 [M, 512], conv5 [M, 1024], t = relu(bn7(conv6)) [M, 4096] (M = N * h * w, contiguous,
    the dtype of net.precision).  ctx goes to aff_head_backward and keeps the inputs alive (not copied)."""
    for name, x, c in (("conv4", conv4, 512), ("conv5", conv5, 1024), ("t", t, 4096)):
        _device_only(x, name)
        tdt = L.TORCH_DTYPE[DT_OF[net.precision]]
        if x.dtype != tdt or tuple(x.shape) != (N * h * w, c) or not x.is_contiguous():
            raise ValueError(f"aff_head_forward: {name} must be contiguous {tdt} rows [{N * h * w}, {c}], got {tuple(x.shape)} {x.dtype}")
    eng = net._engine.active(t.device)
    dims = [(h, w)]
    feat, f9 = eng.run_aff_head(conv4, conv5, t, dims, N)
    return f9, dict(eng=eng, dt=DT_OF[net.precision], N=N, h=h, w=w, conv4=conv4, conv5=conv5, t=t, feat=feat, f9=f9)


def aff_head_backward(ctx, d_f9, gscale=None, scale=None, mask=None, drop=None, capture=None):
    """(d_conv4 [M, 512], d_conv5 [M, 1024], d_t [M, 4096]) in the engine's dtype from d_f9 [M, ld >= 448] (f32 as aff_loss_rows_backward
    writes it, or the engine's dtype), times gscale (a one-element f32 device tensor; None = 1); adds the four weight gradients to the flat
    gradient buffer.  scale [4096] / mask [M, 4096] / drop [N, 4096]: the BN-ReLU backward operands of the f8_5 data gradient
    (d_t * scale[c] * drop[n, c] * (mask > 0)).  capture: a dict that receives dz9, d_feat (a copy: the ELU backward overwrites it), dzf and
    the plans of the data-gradient launches (tests)."""
    eng, dt, N, h, w = ctx["eng"], ctx["dt"], ctx["N"], ctx["h"], ctx["w"]
    M, C = N * h * w, AFF_FEAT_C
    tdt = L.TORCH_DTYPE[dt]
    _device_only(d_f9, "d_f9")
    if d_f9.dim() != 2 or d_f9.shape[0] != M or d_f9.shape[1] < C or d_f9.stride(1) != 1 or d_f9.dtype not in (torch.float32, tdt):
        raise ValueError(f"aff_head_backward: d_f9 must be [{M}, >= {C}] rows in float32 or {tdt}, got {tuple(d_f9.shape)} {d_f9.dtype}")
    if gscale is not None:
        _device_only(gscale, "gscale")
        gscale = gscale.reshape(-1)[:1].float().contiguous()
    dev = d_f9.device
    P = eng.head_wt(dev)
    eng.attach_grads()
    launches = backward_launches(N, h, w, dt, epi1=any(o is not None for o in (scale, mask, drop)))
    wgrad, dgrad = head_backward_launchers(eng, P, launches, capture)

    def E(c):
        return torch.empty(M, c, device=dev, dtype=tdt)

    dz9 = E(C)
    L.elu_backward_rows(d_f9, d_f9.stride(0), ctx["f9"], C, gscale, dz9, C, M, C)
    wgrad("f9", ctx["feat"], dz9)
    d_feat = E(C)
    dgrad("f9", dz9, d_feat)
    if capture is not None:
        capture.update(dz9=dz9, d_feat=d_feat.clone())
    L.elu_backward_rows(d_feat, C, ctx["feat"], C, None, d_feat, C, M, C)      # dzf, in place
    dzf = d_feat
    outs = []
    for name, src in BRANCHES:
        c0 = AFF_FEAT_SLICES[name][0]
        dy = dzf.view(-1)[c0:] if c0 else dzf
        wgrad(name, ctx[src], dy)
        dx = E(arch.AFF_HEAD_CONVS[name][1])
        dgrad(name, dy, dx, **(dict(scale=scale, mask=mask, drop=drop) if name == "f8_5" else {}))
        outs.append(dx)
    if capture is not None:
        capture.update(dzf=dzf)
    return tuple(outs)


class AffinityHead(torch.autograd.Function):
    """f9 = AffinityHead.apply(conv4, conv5, conv6, anchor, net): see affinity_head."""

    @staticmethod
    def forward(ctx, conv4, conv5, conv6, anchor, net):
        N, _, h, w = conv6.shape
        tdt = L.TORCH_DTYPE[DT_OF[net.precision]]
        f9, ctx.saved = aff_head_forward(net, nchw_to_rows(conv4, tdt), nchw_to_rows(conv5, tdt), nchw_to_rows(conv6, tdt), N, h, w)
        ctx.in_dtypes = (conv4.dtype, conv5.dtype, conv6.dtype)
        ctx.set_materialize_grads(False)
        return rows_to_nchw(f9, N, h, w, f9.dtype)

    @staticmethod
    def backward(ctx, g):
        if g is None:
            return None, None, None, None, None
        s = ctx.saved
        N, h, w = s["N"], s["h"], s["w"]
        ds = aff_head_backward(s, grad_to_rows(g, L.TORCH_DTYPE[s["dt"]]))
        return tuple(rows_to_nchw(d, N, h, w, dt_) if need else None for d, dt_, need in zip(ds, ctx.in_dtypes, ctx.needs_input_grad)) + (None, None)


def affinity_head(net, conv4, conv5, conv6):
    """The f9 feature map [N, 448, h, w] (a channels_last view of the engine's rows, in the dtype of net.precision) of the NCHW device
    tensors conv4 [N, 512, h, w], conv5 [N, 1024, h, w], conv6 [N, 4096, h, w] (= relu(bn7(.)), as resnet38d's forward_as_dict hands it
    over).  Differentiable: gradients flow to the three inputs and, through the engine's flat gradient buffer, to the four head weights
    (their .grad are views of it after the backward)."""
    for name, x, c in (("conv4", conv4, 512), ("conv5", conv5, 1024), ("conv6", conv6, 4096)):
        _device_only(x, name)
        if x.dim() != 4 or x.shape[1] != c or x.shape[0] != conv6.shape[0] or x.shape[2:] != conv6.shape[2:]:
            raise ValueError(f"affinity_head: {name} must be [N, {c}, h, w] on conv6's map, got {tuple(x.shape)}")
    eng = net._engine.active(conv6.device)
    anchor = eng.flat_w.new_zeros((), requires_grad=torch.is_grad_enabled())       # the weights live in the flat buffer: keeps the node in the graph
    return AffinityHead.apply(conv4, conv5, conv6, anchor, net)
