"""ResNet-38d + contrast head layer table.

Single source of truth for parameter names / shapes of the hot path.  Mirrors the
constructor of the reference model (network/resnet38d.py:121-155 and
network/resnet38_contrast.py:12-29) as *data*, so the host code, the weight packer and
the synthetic-weight generator all agree on the 233 state_dict keys.
"""
from collections import OrderedDict
from typing import NamedTuple

# (name, kind, cin, mid, cout, stride, first_dilation, dilation, dropout)
#   kind 'res' = ResBlock (two 3x3 convs), 'bot' = ResBlock_bot (1x1, 3x3, 1x1)
BLOCKS = [
    ("b2",   "res", 64,   128,  128,  2, 1, 1, 0.0),
    ("b2_1", "res", 128,  128,  128,  1, 1, 1, 0.0),
    ("b2_2", "res", 128,  128,  128,  1, 1, 1, 0.0),
    ("b3",   "res", 128,  256,  256,  2, 1, 1, 0.0),
    ("b3_1", "res", 256,  256,  256,  1, 1, 1, 0.0),
    ("b3_2", "res", 256,  256,  256,  1, 1, 1, 0.0),
    ("b4",   "res", 256,  512,  512,  2, 1, 1, 0.0),
    ("b4_1", "res", 512,  512,  512,  1, 1, 1, 0.0),
    ("b4_2", "res", 512,  512,  512,  1, 1, 1, 0.0),
    ("b4_3", "res", 512,  512,  512,  1, 1, 1, 0.0),
    ("b4_4", "res", 512,  512,  512,  1, 1, 1, 0.0),
    ("b4_5", "res", 512,  512,  512,  1, 1, 1, 0.0),
    ("b5",   "res", 512,  512,  1024, 1, 1, 2, 0.0),
    ("b5_1", "res", 1024, 512,  1024, 1, 2, 2, 0.0),
    ("b5_2", "res", 1024, 512,  1024, 1, 2, 2, 0.0),
    ("b6",   "bot", 1024, 512,  2048, 1, 4, 4, 0.3),
    ("b7",   "bot", 2048, 1024, 4096, 1, 4, 4, 0.5),
]

# resnet38_contrast.py:29 (+ conv1a): the reference's value for the contrast and affinity nets.  Each Net class states its own FROZEN_BLOCKS; the
# engine derives everything else from it (prefix_of): they are leading blocks, so the forward pass up to there depends on no trainable weight
FROZEN_BLOCKS = ("b2", "b2_1", "b2_2")
HEAD_CONVS = OrderedDict([                       # resnet38_contrast.py:15-20
    ("fc8",     (21,  4096)),
    ("fc_proj", (128, 4096)),
    ("f8_3",    (64,  512)),
    ("f8_4",    (128, 1024)),
    ("f9",      (192, 195)),
])
AFF_HEAD_CONVS = OrderedDict([                   # resnet38_aff.py:13-17 (AffinityNet: ELU branches on conv4 / conv5 / conv6, then f9)
    ("f8_3", (64,  512)),
    ("f8_4", (128, 1024)),
    ("f8_5", (256, 4096)),
    ("f9",   (448, 448)),
])
# DeepLab-v1 head (segmentation/lib/net/deeplabv1.py:18-23) on t = relu(bn7(conv6)): (cout, cin, k) — conv_fov is 3x3 at dilation 12, each of
# the first two convs is followed by a BatchNorm + ReLU, cls_conv alone has a bias
SEG_HEAD_CONVS = OrderedDict([
    ("conv_fov",  (512, 4096, 3)),
    ("conv_fov2", (512, 512, 1)),
    ("cls_conv",  (21,  512, 1)),
])
SEG_HEAD_BNS = {"conv_fov": ("bn_fov", 512), "conv_fov2": ("bn_fov2", 512)}      # the BatchNorm registered behind a head conv
SEG_HEAD_BIAS = ("cls_conv",)
SEG_HEAD_DILATION = 12
SEG_TRAIN_BN_MOM = 0.0003                         # config.py TRAIN_BN_MOM: the momentum of the head's two BatchNorms (train.py:52)
SEG_BACKBONE_PREFIX = "backbone."
SEG_CLS_ROWS = 24                                # cls_conv's pack and pixel rows, zero-padded: the conv launches need OC % 8 == 0
NUM_CLASSES = 21
PROJ_DIM = 128
BN_EPS = 1e-5


def block_same_shape(b):
    name, kind, cin, mid, cout, stride, fd, d, p = b
    return kind == "res" and cin == cout and stride == 1


def block_convs(b):
    """[(param_prefix, cin, cout, k, stride, dilation)] in module-registration order."""
    name, kind, cin, mid, cout, stride, fd, d, p = b
    out = []
    if kind == "res":
        out.append((f"{name}.conv_branch2a", cin, mid, 3, stride, fd))
        out.append((f"{name}.conv_branch2b1", mid, cout, 3, 1, d))
        if not block_same_shape(b):
            out.append((f"{name}.conv_branch1", cin, cout, 1, stride, 1))
    else:
        out.append((f"{name}.conv_branch2a", cin, cout // 4, 1, stride, 1))
        out.append((f"{name}.conv_branch2b1", cout // 4, cout // 2, 3, 1, d))
        out.append((f"{name}.conv_branch2b2", cout // 2, cout, 1, 1, 1))
        out.append((f"{name}.conv_branch1", cin, cout, 1, stride, 1))
    return out


class Prefix(NamedTuple):
    """The frozen prefix of a net as the engine reads it (prefix_of; one per Engine)"""
    n: int                  # number of frozen blocks: BLOCKS[:n]
    channels: int           # of the prefix's output: the last frozen block's, the stem's 64 for an empty prefix
    trainable: tuple        # the rows of BLOCKS behind it
    convs: tuple            # their block_convs rows, in flat-buffer order
    first: str              # the first trainable block: its input comes from the prefix, so it gets weight gradients only
    frozen_convs: tuple     # conv names of the frozen blocks (conv1a aside)
    no_dgrad: frozenset     # the convs of the first trainable block that read its input: no data gradient, no transposed pack


def prefix_of(net):
    """Prefix of net.FROZEN_BLOCKS; refuses what the engine cannot serve: the frozen blocks are a leading run of BLOCKS, and the first trainable
    block exists and is a ResBlock (Engine._trunk_backward handles a first block only in its ResBlock branch)."""
    frozen, who = tuple(net.FROZEN_BLOCKS), f"{type(net).__module__}.{type(net).__qualname__}"
    n = len(frozen)
    if tuple(b[0] for b in BLOCKS[:n]) != frozen:
        raise ValueError(f"{who}.FROZEN_BLOCKS = {frozen}: the engine serves a leading run of arch.BLOCKS (b2, b2_1, ...)")
    if n == len(BLOCKS) or BLOCKS[n][1] != "res":
        raise ValueError(f"{who}.FROZEN_BLOCKS = {frozen}: the first trainable block must exist and be a ResBlock")
    return Prefix(n, BLOCKS[n - 1][4] if n else 64, tuple(BLOCKS[n:]), tuple(c for b in BLOCKS[n:] for c in block_convs(b)), BLOCKS[n][0],
                  tuple(c[0] for b in BLOCKS[:n] for c in block_convs(b)),
                  frozenset(c[0] for c in block_convs(BLOCKS[n]) if c[0].endswith(("branch2a", "branch1"))))


def block_bns(b):
    """[(param_prefix, channels)] in module-registration order."""
    name, kind, cin, mid, cout, stride, fd, d, p = b
    if kind == "res":
        return [(f"{name}.bn_branch2a", cin), (f"{name}.bn_branch2b1", mid)]
    return [(f"{name}.bn_branch2a", cin), (f"{name}.bn_branch2b1", cout // 4),
            (f"{name}.bn_branch2b2", cout // 2)]


def state_dict_spec(head_convs=None, head_bns=None, head_bias=(), backbone_prefix=""):
    """OrderedDict key -> shape, in the reference's state_dict() order (233 keys with the contrast head).
    head_convs: the net's head table (default HEAD_CONVS; AFF_HEAD_CONVS for the AffinityNet): name -> (cout, cin) of a 1x1 conv or
    (cout, cin, k).  head_bns {conv name: (bn name, channels)}: a BatchNorm registered behind that conv; head_bias: the head convs with
    a bias; backbone_prefix: the backbone is a sub-module of that name (seg_state_dict_spec: the DeepLab head, 242 keys)."""
    spec = OrderedDict()
    spec["conv1a.weight"] = (64, 3, 3, 3)

    def add_bn(prefix, c):
        spec[prefix + ".weight"] = (c,)
        spec[prefix + ".bias"] = (c,)
        spec[prefix + ".running_mean"] = (c,)
        spec[prefix + ".running_var"] = (c,)
        spec[prefix + ".num_batches_tracked"] = ()

    for b in BLOCKS:
        name, kind = b[0], b[1]
        convs = dict((p, (co, ci, k, k)) for (p, ci, co, k, s, d) in block_convs(b))
        bns = dict(block_bns(b))
        # registration order inside the reference blocks (resnet38d.py:15-25, 60-72)
        if kind == "res":
            order = ["bn_branch2a", "conv_branch2a", "bn_branch2b1", "conv_branch2b1", "conv_branch1"]
        else:
            order = ["bn_branch2a", "conv_branch2a", "bn_branch2b1", "conv_branch2b1",
                     "bn_branch2b2", "conv_branch2b2", "conv_branch1"]
        for o in order:
            p = f"{name}.{o}"
            if p in bns:
                add_bn(p, bns[p])
            elif p in convs:
                spec[p + ".weight"] = convs[p]
    add_bn("bn7", 4096)
    if backbone_prefix:
        spec = OrderedDict((backbone_prefix + k, v) for k, v in spec.items())
    for hname, shape in (HEAD_CONVS if head_convs is None else head_convs).items():
        co, ci, k = shape if len(shape) == 3 else (*shape, 1)
        spec[hname + ".weight"] = (co, ci, k, k)
        if hname in head_bias:
            spec[hname + ".bias"] = (co,)
        if head_bns and hname in head_bns:
            add_bn(*head_bns[hname])
    return spec


def seg_state_dict_spec():
    """The 242 keys of the reference's deeplabv1 over resnet38d: `backbone.*`, then conv_fov, bn_fov, conv_fov2, bn_fov2, cls_conv (+ bias)."""
    return state_dict_spec(SEG_HEAD_CONVS, SEG_HEAD_BNS, SEG_HEAD_BIAS, SEG_BACKBONE_PREFIX)


def block_out_dims(b, dims):
    """Output (h, w) of block `b` for each input (h, w) of `dims`.  Every conv of a block produces this size: the strided conv is the
    block's first one (3x3 at first_dilation in a ResBlock, 1x1 in a ResBlock_bot), padded by dilation * (k // 2)."""
    name, kind, cin, mid, cout, stride, fd, d, p = b
    k, dil = (3, fd) if kind == "res" else (1, 1)
    span = 2 * (dil * (k // 2)) - dil * (k - 1) - 1
    return [((h + span) // stride + 1, (w + span) // stride + 1) for (h, w) in dims]


def forward_macs(H, W, head_convs=None):
    """Algorithmic multiply-accumulates of ONE Net.forward on an H x W image (conv MACs = Cin * Cout * k^2 * h_out * w_out
    for every conv of resnet38d.py:160-189 and resnet38_contrast.py:34-54, PCM = hw^2 * (192 + 21), resnet38_contrast.py:70-73).
    448 x 448 -> 403.697e9, 128 x 128 -> 32.798e9.
    head_convs: another head table (AFF_HEAD_CONVS): its 1x1 convs replace the contrast head and the PCM term."""
    macs = 3 * 64 * 9 * H * W                                   # conv1a, stride 1, same size
    h, w = H, W
    for b in BLOCKS:
        (oh, ow), = block_out_dims(b, [(h, w)])
        for (_n, ci, co, k, s, dd) in block_convs(b):
            macs += ci * co * k * k * oh * ow                   # every conv of a block produces the block's output size
        h, w = oh, ow
    hw = h * w
    if head_convs is not None:
        return macs + hw * sum(s[0] * s[1] * (s[2] ** 2 if len(s) == 3 else 1) for s in head_convs.values())
    macs += hw * sum(co * ci for (co, ci) in HEAD_CONVS.values())
    macs += hw * hw * (192 + 21)
    return macs
