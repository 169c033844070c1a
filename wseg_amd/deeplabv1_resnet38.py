"""Drop-in replacement of the reference's DeepLab-v1 segmentation net over ResNet-38d: `--network wseg_amd.deeplabv1_resnet38`.

Mirrors the public contract of segmentation/lib/net/deeplabv1.py:deeplabv1 with net/backbone/resnet38d.py (the SEAM experiment
segmentation/experiment/SEAM_deeplabv1_resnet38): `Net()`, `forward(x)` returning the [N, 21, h, w] logits at the input size,
`.normalize`, `.get_parameter_groups()`, and the reference's 242 state_dict keys (`backbone.*`, then conv_fov, bn_fov, conv_fov2,
bn_fov2, cls_conv with its bias), so a published checkpoint loads with strict=True.  The sub-modules are parameter containers: the
backbone runs through wseg_amd.engine (the contrast net's kernels and packs), the head's three convs on the implicit-GEMM conv
(Engine.run_seg_head: conv_fov is its 3x3 launch at dilation 12, both head BatchNorms folded into the epilogue, cls_conv's bias the
epilogue's shift), the resample to the input size in csrc/seg.hip.  Inference only: in training mode `forward` raises.  Of the training
stage the loss layer exists — wseg_amd.seg_loss.seg_cross_entropy, the cross-entropy of the resampled coarse logits and its gradient on the
cls_conv rows (csrc/seg_loss.hip) — and the head layer: wseg_amd.seg_head, the head's training forward (BatchNorm on batch statistics, dropout)
and its backward down to t = relu(bn7(conv6)) (csrc/seg_head.hip) — and the data path: wseg_amd.seg_data.DeviceSegData turns decoded images
and label PNGs into the (img float32 [N, 3, crop, crop], label uint8 [N, crop, crop]) pair of a training step on the device (csrc/seg_data.hip;
host chain: wseg_amd.data.VOCSegTrainDataset).  The backbone's backward from t and the trainer do not exist yet, so `forward` keeps refusing
training mode.
"""
import os

import torch
import torch.nn as nn

from . import arch
from . import _lib as L
from .resnet38_contrast import Net as _ContrastNet, Normalize, _Block

_NO_TRAINING = ("wseg_amd.deeplabv1_resnet38.Net is inference-only: the training loss exists (wseg_amd.seg_loss.seg_cross_entropy on the coarse "
                "logits), the training forward does not yet: call .eval() first")


class _Backbone(nn.Module):
    """Parameter container with the attribute names of net/backbone/resnet38d.py:Net.  Never called."""

    def __init__(self):
        super().__init__()
        self.conv1a = nn.Conv2d(3, 64, 3, padding=1, bias=False)
        for spec in arch.BLOCKS:
            setattr(self, spec[0], _Block(spec))
        self.bn7 = nn.BatchNorm2d(4096)
        self.not_training = [self.conv1a]
        self.OUTPUT_DIM = 4096

    def forward(self, *a, **k):
        raise RuntimeError("wseg_amd backbones are parameter containers; call Net.forward")

    def train(self, mode=True):
        """net/backbone/resnet38d.py:192-214: conv1a frozen, every BatchNorm in eval and frozen, in either mode."""
        super().train(mode)
        self.conv1a.weight.requires_grad = False
        for layer in self.modules():
            if isinstance(layer, nn.BatchNorm2d):
                layer.eval()
                layer.bias.requires_grad = False
                layer.weight.requires_grad = False
        return self


class Net(nn.Module):
    HEAD_KIND = "seg"
    HEAD_CONVS = arch.SEG_HEAD_CONVS
    FLAT_HEAD_ORDER = tuple(arch.SEG_HEAD_CONVS)
    # the prefix the engine serves this net with today (inference does not depend on it); the reference trains from b2 on: the training change is this line
    FROZEN_BLOCKS = arch.FROZEN_BLOCKS

    def __init__(self, precision=None):
        super().__init__()
        self.backbone = _Backbone()
        self.conv_fov = nn.Conv2d(4096, 512, 3, 1, padding=arch.SEG_HEAD_DILATION, dilation=arch.SEG_HEAD_DILATION, bias=False)
        self.bn_fov = nn.BatchNorm2d(512, momentum=arch.SEG_TRAIN_BN_MOM)
        self.conv_fov2 = nn.Conv2d(512, 512, 1, 1, padding=0, bias=False)
        self.bn_fov2 = nn.BatchNorm2d(512, momentum=arch.SEG_TRAIN_BN_MOM)
        self.dropout1 = nn.Dropout(0.5)
        self.cls_conv = nn.Conv2d(512, arch.NUM_CLASSES, 1, 1, padding=0)
        # inits of deeplabv1.py:29-36
        for m in (self.conv_fov, self.conv_fov2, self.cls_conv):
            nn.init.kaiming_normal_(m.weight, mode='fan_out', nonlinearity='relu')
        self.not_training = []
        self.from_scratch_layers = [self.conv_fov, self.conv_fov2, self.cls_conv]
        self.normalize = Normalize()
        self.precision = precision or os.environ.get("WSEG_PRECISION", "bf16")
        assert self.precision in ("bf16", "fp32", "bf16x3")

    _engine = _ContrastNet._engine             # one engine per module instance (replicas get their own)

    def __getattr__(self, name):
        """The engine addresses the backbone's layers by the names of the contrast net (conv1a, b2 ... b7, bn7): they resolve into `backbone`."""
        try:
            return super().__getattr__(name)
        except AttributeError:
            backbone = self.__dict__.get("_modules", {}).get("backbone")
            if backbone is not None and name in backbone._modules:
                return backbone._modules[name]
            raise

    # ---- reference API -------------------------------------------------------------------
    def forward(self, x):
        """deeplabv1.py:39-51 in eval mode: the logits resampled (bilinear, align_corners=True) to the input size, [N, 21, h, w] float32."""
        if self.training:
            raise RuntimeError(_NO_TRAINING)
        rows, (fh, fw) = self.coarse_logits(x)
        N, h, w = x.shape[0], x.shape[2], x.shape[3]
        out = torch.empty(N, arch.NUM_CLASSES, h, w, device=rows.device, dtype=torch.float32)
        amax = torch.empty(h, w, device=rows.device, dtype=torch.uint8)
        for n in range(N):                       # one pass of the fusion kernel per image: its second stage (h, w) -> (h, w) is the identity
            L.seg_fuse([L.SegPass(rows, arch.SEG_CLS_ROWS, n, fh, fw, h, w, False)], h, w, arch.NUM_CLASSES, amax, mean_logits=out[n])
        return out

    @torch.no_grad()
    def coarse_logits(self, x):
        """(cls_conv pixel rows [N * fh * fw, 24] in the mode's dtype — 21 logits and three zero columns — and the stride-8 dims (fh, fw)); nothing
        synchronises.  seg_infer.fuse_image resamples and fuses them without the intermediate full-size maps."""
        if self.training:
            raise RuntimeError(_NO_TRAINING)
        if not x.is_cuda:
            raise RuntimeError("wseg_amd.deeplabv1_resnet38 runs only on an MI355X (HIP) device; there is no CPU fallback")
        x = x.contiguous().float()
        eng = self._engine.active(x.device)
        st, ps = eng.run_backbone([x])
        return eng.run_seg_head(st["t"], st["dims"], x.shape[0], ps=ps), st["dims"][0]

    def get_parameter_groups(self):
        """deeplabv1.py:53-69."""
        groups = ([], [], [], [])
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                if m.weight.requires_grad:
                    (groups[2] if m in self.from_scratch_layers else groups[0]).append(m.weight)
                if m.bias is not None and m.bias.requires_grad:
                    (groups[3] if m in self.from_scratch_layers else groups[1]).append(m.bias)
        return groups
