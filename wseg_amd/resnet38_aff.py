"""Drop-in replacement of the reference's AffinityNet module: `--network wseg_amd.resnet38_aff`.

Mirrors the public contract of network/resnet38_aff.py (+ network/resnet38d.py:104-214): `Net()`, `forward(x, to_dense=False)`
returning the pair affinities [N, P, n_from] (or, with to_dense, the dense [area, area] matrix of one image as a device tensor),
`.normalize`, `.get_parameter_groups()`, and the reference's state_dict keys (the backbone, then f8_3, f8_4, f8_5, f9).  The
sub-modules are parameter containers: the backbone runs through wseg_amd.engine (the contrast net's kernels and packs), the
ELU head on the implicit-GEMM conv (epilogue 3; Engine.run_aff_head), the pairs / dense scatter in csrc/affinity.hip.  `forward` is
inference: in training mode it raises.  Training (aff_train.py) enters through names of its own: `train_forward` / `train_backward` (the
saved backbone pass and the ELU head of wseg_amd/aff_head.py; the head's backward, then Engine.run_trunk_backward with the conv4 / conv5
gradients as taps), which wseg_amd.aff_train.AffTrainer drives without autograd, and `affinities_train`, their differentiable wrapper.
"""
import os

import numpy as np
import torch
import torch.nn as nn

from . import arch
from . import engine
from . import _lib as L
from .resnet38_contrast import Net as _ContrastNet, Normalize, _Block, train_frozen

FEAT_C = engine.AFF_FEAT_C                      # [f8_3 64 | f8_4 128 | f8_5 256]: the concat of resnet38_aff.py:47 is three column slices
DEFAULT_RADIUS = 5
PREDEFINED_FEATURESIZE = 448 // 8               # resnet38_aff.py:27-29 (the same pair set as the general rule at 56 x 56)


def pair_radius(h, w, radius=DEFAULT_RADIUS):
    """The radius rule of resnet38_aff.py:51-56: (min_edge - 1) // 2 below 2 * radius + 1, else `radius`.  The reference's pair set is empty
    at radius 1 (min feature edge 3 or 4: its index construction fails), so a map whose min edge is below 5 is refused here."""
    min_edge = min(h, w)
    r = (min_edge - 1) // 2 if min_edge < radius * 2 + 1 else radius
    if r < 2:
        raise ValueError(f"AffinityNet needs a feature map with min edge >= 5 (an input side >= 33 px); got {h}x{w} (radius {r})")
    return r


def pair_offsets(radius):
    """[(dy, dx)] in the reference's order (tool/pyutils.py get_indices_of_pairs)."""
    out = [(0, x) for x in range(1, radius)]
    for y in range(1, radius):
        for x in range(-radius + 1, radius):
            if x * x + y * y < radius * radius:
                out.append((y, x))
    return out


def indices_of_pairs(radius, size):
    """(ind_from [n_from], ind_to [P * n_from]) int64 — the pair set the kernels use, as flat pixel indices of an h x w map.
    "from" pixels: rows [0, h-r+1) x columns [r-1, w-r+1)."""
    h, w = size
    rf = radius - 1
    full = np.arange(h * w, dtype=np.int64).reshape(h, w)
    ch, cw = h - rf, w - 2 * rf
    ind_from = full[:ch, rf:rf + cw].reshape(-1)
    ind_to = np.concatenate([full[dy:dy + ch, rf + dx:rf + dx + cw].reshape(-1) for dy, dx in pair_offsets(radius)])
    return ind_from, ind_to


def _pair_affinities(f9, N, h, w, r):
    aff = torch.empty(N, L.aff_num_offsets(r), (h - r + 1) * (w - 2 * r + 2), device=f9.device, dtype=torch.float32)
    L.aff_pairs(f9, FEAT_C, FEAT_C, aff, N, h, w, r)
    return aff


class _AffinitiesTrain(torch.autograd.Function):
    """aff = exp(-mean_c |f9[to] - f9[from]|) of the f9 rows of Net.train_forward, with the whole net's backward behind it."""

    @staticmethod
    def forward(ctx, anchor, f9, saved, N, h, w, r):
        aff = _pair_affinities(f9, N, h, w, r)
        ctx.save_for_backward(aff, f9)
        ctx.saved, ctx.geo = saved, (N, h, w, r)
        return aff

    @staticmethod
    def backward(ctx, g):
        aff, f9 = ctx.saved_tensors
        N, h, w, r = ctx.geo
        d_f9 = torch.empty(N * h * w, FEAT_C, device=f9.device, dtype=torch.float32)
        L.aff_pairs_backward(f9, FEAT_C, FEAT_C, aff, g.contiguous().float(), d_f9, FEAT_C, N, h, w, r)
        Net.train_backward(ctx.saved, d_f9)
        ctx.saved = ctx.geo = None
        return (None,) * 7


class Net(nn.Module):
    HEAD_KIND = "aff"
    HEAD_CONVS = arch.AFF_HEAD_CONVS
    FLAT_HEAD_ORDER = tuple(arch.AFF_HEAD_CONVS)
    FROZEN_BLOCKS = arch.FROZEN_BLOCKS         # network/resnet38d.py:154 not_training, as the contrast net

    def __init__(self, precision=None):
        super().__init__()
        self.conv1a = nn.Conv2d(3, 64, 3, padding=1, bias=False)
        for spec in arch.BLOCKS:
            setattr(self, spec[0], _Block(spec))
        self.bn7 = nn.BatchNorm2d(4096)
        self.f8_3 = nn.Conv2d(512, 64, 1, bias=False)
        self.f8_4 = nn.Conv2d(1024, 128, 1, bias=False)
        self.f8_5 = nn.Conv2d(4096, 256, 1, bias=False)
        self.f9 = nn.Conv2d(448, 448, 1, bias=False)
        # inits of network/resnet38_aff.py:19-22
        nn.init.kaiming_normal_(self.f8_3.weight)
        nn.init.kaiming_normal_(self.f8_4.weight)
        nn.init.kaiming_normal_(self.f8_5.weight)
        nn.init.xavier_uniform_(self.f9.weight, gain=4)
        self.not_training = [self.conv1a] + [getattr(self, b) for b in self.FROZEN_BLOCKS]
        self.from_scratch_layers = [self.f8_3, self.f8_4, self.f8_5, self.f9]
        self.predefined_featuresize = PREDEFINED_FEATURESIZE
        self.radius = DEFAULT_RADIUS
        self.normalize = Normalize()
        self.precision = precision or os.environ.get("WSEG_PRECISION", "bf16")
        assert self.precision in ("bf16", "fp32", "bf16x3")

    _engine = _ContrastNet._engine             # one engine per module instance (replicas get their own)

    # ---- reference API -------------------------------------------------------------------
    def forward(self, x, to_dense=False):
        """network/resnet38_aff.py:40-97."""
        if self.training:
            raise RuntimeError("wseg_amd.resnet38_aff.Net is inference-only (aff_train is out of scope): call .eval() first")
        aff, (h, w, r) = self.affinities(x)
        if not to_dense:
            return aff
        if aff.shape[0] != 1:
            raise ValueError("forward(x, to_dense=True) builds the matrix of ONE image (as the reference): batch size must be 1")
        dense = torch.empty(h * w, h * w, device=aff.device, dtype=torch.float32)
        L.aff_to_dense(aff, dense, h, w, r)
        return dense

    @torch.no_grad()
    def affinities(self, x):
        """(aff [N, P, n_from] f32, (h, w, radius)) on the HIP kernels; nothing synchronises."""
        if not x.is_cuda:
            raise RuntimeError("wseg_amd.resnet38_aff runs only on an MI355X (HIP) device; there is no CPU fallback")
        x = x.contiguous().float()
        eng = self._engine.active(x.device)
        st, ps = eng.run_backbone([x])                                 # conv4 / conv5 / conv6 (resnet38d.py:160-189)
        N = x.shape[0]
        dims = st["dims"]
        (h, w), = dims
        r = pair_radius(h, w, self.radius)
        _, f9 = eng.run_aff_head(st["conv4"], st["conv5"], st["t"], dims, N, ps=ps)
        return _pair_affinities(f9, N, h, w, r), (h, w, r)

    # ---- training (aff_train.py): enters here and through wseg_amd.aff_train, never through forward ----------
    def set_dropout_masks(self, mask_sets):
        """Inject Dropout2d scale factors: a list of dicts over the FOUR sites of the backbone (b6 / b7 dropout_2b1, dropout_2b2: this net
        has no dropout7), one consumed per training pass — the parity tests."""
        self._engine.injected_masks = list(mask_sets) if mask_sets is not None else None

    def train_forward(self, x):
        """The training-mode pass down to the f9 rows: backbone with saved activations, then the ELU head.  Returns (f9 rows [M, 448] in
        the mode's dtype, (h, w, radius), saved) — `saved` goes to train_backward.  No autograd graph, nothing synchronises."""
        if not self.training:
            raise RuntimeError("wseg_amd.resnet38_aff: the training pass needs training mode (call .train() first); .eval() has forward / affinities")
        if not x.is_cuda:
            raise RuntimeError("wseg_amd.resnet38_aff runs only on an MI355X (HIP) device; there is no CPU fallback")
        from . import aff_head
        x = x.contiguous().float()
        eng = self._engine.active(x.device)
        st, _ps, S = eng.run_backbone([x], save=True)
        (h, w), = st["dims"]
        r = pair_radius(h, w, self.radius)
        f9, hctx = aff_head.aff_head_forward(self, st["conv4"], st["conv5"], st["t"], x.shape[0], h, w)
        return f9, (h, w, r), dict(eng=eng, S=S, head=hctx)

    @staticmethod
    def train_backward(saved, d_f9, gscale=None, between=None):
        """From d_f9 [M, >= 448] (f32 or the mode's dtype; times the one-element device tensor gscale) to every trainable weight's gradient
        in the flat buffer: the head's backward, whose f8_5 data gradient folds bn7's scale and ReLU in, then the trunk's with the conv4 /
        conv5 gradients as taps of b5 / b6.  Gradients ACCUMULATE (the flat buffer is zeroed when it is first attached as the parameters'
        .grad, and by the optimizer's zero_grad).  between: called between the two phases (scripts/bench_aff_train.py records an event)."""
        from . import aff_head
        eng, S = saved["eng"], saved["S"]
        s7, _ = eng.packs["bn"]["bn7"]
        d_conv4, d_conv5, d_conv6 = aff_head.aff_head_backward(saved["head"], d_f9, gscale, scale=s7, mask=S["fea"])
        if between is not None:
            between()
        eng.run_trunk_backward(S, d_conv6, {"b5": d_conv4, "b6": d_conv5})

    def affinities_train(self, x):
        """aff [N, P, n_from] f32 as `affinities` computes it, in training mode and differentiable: its backward (one autograd node) runs
        aff_pairs_backward, the head's backward and the trunk's, and leaves the gradients in the parameters' .grad (views of the flat
        buffer).  The reference's loss lines (aff_train.py:111-119) as torch ops on it train the net.  As any autograd gradient these
        ACCUMULATE over backward calls: clear them with the optimizer's zero_grad (one memset of the flat buffer) or with
        zero_grad(set_to_none=True) (the next backward re-attaches the views and zeroes the buffer).  With gradients disabled the pass still
        runs in training mode (dropout masks drawn) but keeps nothing: the saved activations are dropped before it returns."""
        f9, (h, w, r), saved = self.train_forward(x)
        if not torch.is_grad_enabled():
            del saved
            return _pair_affinities(f9, x.shape[0], h, w, r)
        anchor = saved["eng"].flat_w.new_zeros((), requires_grad=True)     # the weights live in the flat buffer: keeps the node in the graph
        return _AffinitiesTrain.apply(anchor, f9, saved, x.shape[0], h, w, r)

    def get_parameter_groups(self):
        """network/resnet38_aff.py:100-119."""
        groups = ([], [], [], [])
        for m in self.modules():
            if isinstance(m, (nn.Conv2d, nn.modules.normalization.GroupNorm)):
                if m.weight.requires_grad:
                    (groups[2] if m in self.from_scratch_layers else groups[0]).append(m.weight)
                if m.bias is not None and m.bias.requires_grad:
                    (groups[3] if m in self.from_scratch_layers else groups[1]).append(m.bias)
        return groups

    train = train_frozen                       # (forward still refuses training mode: see affinities_train)
