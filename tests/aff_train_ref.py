"""CPU restatement of the reference's AffinityNet training step (aff_train.py:105-123 on network/resnet38_aff.py:35-63).  TEST
INFRASTRUCTURE, no tests here: tests/test_aff_train_host.py pins it on the fixtures the reference itself produced
(scripts/make_aff_train_goldens.py -> tests/golden/aff_train_*.npz); tests/test_gpu_aff_train.py then holds the HIP path to the same fixtures.

Functional, as oracle/net.py: the backbone is oracle.net.backbone (imported, training mode = explicit Dropout2d masks over the FOUR sites of
b6 / b7: this net has no dropout7), then the four ELU convs, the pair gather, the three loss lines, and oracle.optim.PolySGD built as
aff_train.py:72-78 builds the reference's optimizer.
"""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import net as onet
from oracle import optim as ooptim
from wseg_amd import synth
from wseg_amd.aff_loss import STATS, pair_labels
from wseg_amd.resnet38_aff import indices_of_pairs, pair_radius

FIXTURES = ("aff_train_64_N2", "aff_train_104_N1")
SCRATCH = ("f8_3.", "f8_4.", "f8_5.", "f9.")
# the four head weights, one conv each of b7 ... b3, and the two skip convs whose data gradient takes a tap
GRAD_KEYS = ["f8_3.weight", "f8_4.weight", "f8_5.weight", "f9.weight", "b7.conv_branch2b1.weight", "b6.conv_branch2a.weight",
             "b5.conv_branch2a.weight", "b4.conv_branch2a.weight", "b3.conv_branch2a.weight", "b5.conv_branch1.weight", "b6.conv_branch1.weight"]
MASK_SITES = ("b6.dropout_2b1", "b6.dropout_2b2", "b7.dropout_2b1", "b7.dropout_2b2")


def aff_masks(n, seed):
    """the Dropout2d scale factors of the AffinityNet's four sites (synth.synthetic_dropout_masks without dropout7)"""
    m = synth.synthetic_dropout_masks(n, seed)
    return {k: m[k] for k in MASK_SITES}


SLICE = 1536          # samples per stored slice: two steps of gradient and weight slices of eleven keys stay within the size of the step fixtures


def slice_of(t):
    """the fixtures' strided SLICE-sample slice of a tensor (an odd stride: a stride that shares factors with the 9 taps and the channel counts
    visits a few taps and channels over and over — for b7.conv_branch2b1 under one image's dropout masks, only zeros)"""
    flat = t.detach().reshape(-1)
    return flat[::max(1, flat.numel() // SLICE) | 1][:SLICE]


def pair_signs(f9_nchw, r):
    """sign(f_to - f_from) [N, C, P, n_from] of a feature map: the decisions of |.| in the pair distance"""
    N, C, h, w = f9_nchw.shape
    ind_from, ind_to = (torch.from_numpy(i) for i in indices_of_pairs(r, (h, w)))
    x = f9_nchw.reshape(N, C, -1)
    ff = torch.index_select(x, 2, ind_from).unsqueeze(2)
    return torch.sign(torch.index_select(x, 2, ind_to).view(N, C, -1, ff.size(3)) - ff)


def forward(img, sd, masks, radius=5, gates=None, signs=None):
    """(aff [N, P, n_from], (h, w, r)): network/resnet38_aff.py:35-63 in training mode (masks None: eval).  gates / signs: another
    implementation's decisions in place of this one's — its ReLU masks (oracle.net._relu) and its sign(f_to - f_from) (pair_signs): |d|
    becomes d * sign, which differs from |d| only where the two implementations' d straddle zero, by less than their difference."""
    d = onet.backbone(img, sd, masks, gates)
    f8_3 = F.elu(F.conv2d(d["conv4"], sd["f8_3.weight"]))
    f8_4 = F.elu(F.conv2d(d["conv5"], sd["f8_4.weight"]))
    f8_5 = F.elu(F.conv2d(d["conv6"], sd["f8_5.weight"]))
    x = F.elu(F.conv2d(torch.cat([f8_3, f8_4, f8_5], dim=1), sd["f9.weight"]))
    N, C, h, w = x.shape
    r = pair_radius(h, w, radius)
    ind_from, ind_to = (torch.from_numpy(i) for i in indices_of_pairs(r, (h, w)))
    x = x.view(N, C, -1)
    ff = torch.index_select(x, 2, ind_from).unsqueeze(2)
    ft = torch.index_select(x, 2, ind_to).view(N, C, -1, ff.size(3))
    dist = torch.abs(ft - ff) if signs is None else (ft - ff) * signs
    return torch.exp(-torch.mean(dist, dim=1)), (h, w, r)


def labels_of(maps, r):
    """the reference's three label tensors [N, P, n_from] of uint8 maps [N, h, w]"""
    per = [pair_labels(np.asarray(m), r) for m in maps]
    return tuple(torch.from_numpy(np.stack([p[j] for p in per])) for j in range(3))


def loss_lines(aff, labels):
    """aff_train.py:111-119: (loss, the seven scalars in STATS order)"""
    bg_label, fg_label, neg_label = labels
    bg_count = torch.sum(bg_label) + 1e-5
    fg_count = torch.sum(fg_label) + 1e-5
    neg_count = torch.sum(neg_label) + 1e-5
    bg_loss = torch.sum(- bg_label * torch.log(aff + 1e-5)) / bg_count
    fg_loss = torch.sum(- fg_label * torch.log(aff + 1e-5)) / fg_count
    neg_loss = torch.sum(- neg_label * torch.log(1. + 1e-5 - aff)) / neg_count
    loss = bg_loss / 4 + fg_loss / 4 + neg_loss / 2
    return loss, torch.stack([loss, bg_loss, fg_loss, neg_loss, bg_count, fg_count, neg_count]).detach()


def label_maps(g, step):
    return np.stack([synth.synthetic_aff_label_map(int(g["h"]), int(g["w"]), int(s)).numpy() for s in g["label_seeds"][step]])


def optimizer(sd, lr, wt_dec, max_step):
    """aff_train.py:72-78 (groups taken before .train(): group 0 holds every conv weight outside the from-scratch layers)"""
    conv_keys = [k for k, v in sd.items() if v.dim() == 4]
    g0 = [sd[k] for k in conv_keys if not k.startswith(SCRATCH)]
    g2 = [sd[k] for k in conv_keys if k.startswith(SCRATCH)]
    return ooptim.PolySGD([{"params": g0, "lr": lr, "weight_decay": wt_dec}, {"params": [], "lr": 2 * lr, "weight_decay": 0},
                           {"params": g2, "lr": 10 * lr, "weight_decay": wt_dec}, {"params": [], "lr": 20 * lr, "weight_decay": 0}],
                          lr=lr, weight_decay=wt_dec, max_step=max_step)


def run_steps(g, sd0):
    """The fixture's consecutive steps on the CPU: [(scalars [7], {key: gradient}, {key: weight after the step})] per step, and the
    optimizer (its groups' final lr)."""
    n, size, seed, steps = int(g["n"]), int(g["size"]), int(g["seed"]), int(g["steps"])
    sd = {k: v.clone() for k, v in sd0.items()}
    keys = onet.trainable_keys(sd)
    opt = optimizer(sd, float(g["lr"]), float(g["wt_dec"]), int(g["max_step"]))
    out = []
    for s_ in range(steps):
        for k in keys:
            sd[k].requires_grad_(True)
            sd[k].grad = None
        aff, (h, w, r) = forward(synth.synthetic_images(n, size, seed + s_), sd, aff_masks(n, int(g["mask_seeds"][s_])))
        assert (h, w, r) == (int(g["h"]), int(g["w"]), int(g["radius"]))
        loss, out7 = loss_lines(aff, labels_of(label_maps(g, s_), r))
        loss.backward()
        grads = {k: sd[k].grad for k in keys}
        for k in keys:
            sd[k].requires_grad_(False)
        opt.step({id(sd[k]): grads[k] for k in keys})
        out.append((out7, grads, {k: sd[k].clone() for k in GRAD_KEYS}))
    return out, opt


__all__ = ["STATS", "FIXTURES", "GRAD_KEYS", "aff_masks", "forward", "labels_of", "loss_lines", "optimizer", "run_steps", "slice_of", "label_maps", "pair_signs"]
