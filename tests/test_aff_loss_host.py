"""AffinityNet training loss, host side (no GPU): the label rule against the reference extractor's recorded outputs, the float64
restatement (tests/aff_loss_f64.py) against the reference's recorded loss and gradient, the label-map rule on hand-built cases, and the
argument checks of the three C entry points (they run before any device call)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from tests import aff_loss_f64 as A
from wseg_amd import _lib as L, synth
from wseg_amd.aff_loss import aff_label_map, pair_labels
from wseg_amd.resnet38_aff import indices_of_pairs, pair_offsets

from tests.aff_loss_f64 import REF_BAR_AFF, REF_BAR_DZ, REF_BAR_OUT7        # 2 x the measured deviation: stated there

LOSS_FIXTURES = ["aff_loss_7x7", "aff_loss_13x13"]


def test_pair_labels_equal_reference_extractor(golden_dir):
    g = np.load(os.path.join(golden_dir, "aff_loss_labels.npz"))
    assert g["cases"].tolist() == [[7, 3, 1], [13, 5, 1], [56, 5, 2]]
    for s, r, seed in g["cases"].tolist():
        key = f"{s}x{s}"
        lab = g[key + "_map"]
        np.testing.assert_array_equal(lab, synth.synthetic_aff_label_map(s, s, seed).numpy())      # the generator is part of the fixture
        out = pair_labels(lab, r)
        P, n_from = len(pair_offsets(r)), (s - r + 1) * (s - 2 * r + 2)
        assert all(o.shape == (P, n_from) and o.dtype == np.float32 for o in out)
        bits = np.packbits(np.stack(out).astype(bool).reshape(3, -1), axis=1)
        np.testing.assert_array_equal(bits, g[key + "_bits"], err_msg=key)
        assert [int(o.sum()) for o in out] == g[key + "_counts"].tolist()
        assert set(np.unique(np.stack(out)).tolist()) <= {0.0, 1.0}
        assert g[key + "_counts"].min() >= 10


@pytest.mark.parametrize("h,w,r", [(5, 7, 2), (8, 11, 3), (13, 16, 5)])
def test_pair_labels_pair_order_on_non_square_maps(h, w, r):
    """The extractor is square-only: on other maps the pair order is the one of indices_of_pairs (itself pinned to the reference's index
    arrays by test_aff_host.py): the rule applied to the labels at those indices gives the three tensors, and ignoring one pixel
    changes exactly the entries of the pairs that hold it."""
    ind_from, ind_to = indices_of_pairs(r, (h, w))
    P = len(pair_offsets(r))
    lab = synth.synthetic_aff_label_map(h, w, 4, block=2).numpy()
    flat = lab.reshape(-1).astype(np.int64)
    lf, lt = np.tile(flat[ind_from], P), flat[ind_to]
    valid = (lf < 255) & (lt < 255)
    bg, fg, neg = pair_labels(lab, r)
    np.testing.assert_array_equal(bg.reshape(-1), ((lf == lt) & (lf == 0)).astype(np.float32))
    np.testing.assert_array_equal(fg.reshape(-1), ((lf == lt) & (lf != 0) & valid).astype(np.float32))
    np.testing.assert_array_equal(neg.reshape(-1), ((lf != lt) & valid).astype(np.float32))
    assert bg.shape == (P, len(ind_from)) and bg.sum() > 0 and fg.sum() > 0 and neg.sum() > 0
    # every pair once: moving one label changes exactly the pairs that hold that pixel, at the positions indices_of_pairs gives them
    q = int(ind_from[len(ind_from) // 2])
    lab2 = lab.copy()
    lab2.reshape(-1)[q] = 255
    changed = np.flatnonzero(np.stack(pair_labels(lab2, r)).reshape(3, -1).sum(0) != np.stack([bg, fg, neg]).reshape(3, -1).sum(0))
    holds_q = np.flatnonzero(((np.tile(ind_from, P) == q) | (ind_to == q)) & valid)
    np.testing.assert_array_equal(changed, holds_q)


@pytest.mark.parametrize("name", LOSS_FIXTURES)
def test_f64_restatement_reproduces_reference_loss_and_gradient(golden_dir, name):
    g = np.load(os.path.join(golden_dir, name + ".npz"))
    z = torch.from_numpy(g["z"])
    r = int(g["radius"])
    got = A.restate(torch.nn.functional.elu(z), torch.from_numpy(g["label"]), r)
    dev_aff = float(np.abs(got["aff"].numpy() - g["aff"]).max() / np.abs(g["aff"]).max())
    dev_out7 = max(abs(float(got["out7"][i]) - float(g["out7"][i])) / abs(float(g["out7"][i])) for i in range(7))
    dz = (got["grad"] * A.elu_grad(z.double())).numpy()[:, g["dz_channels"]]
    dev_dz = float(np.abs(dz - g["dz"]).max() / np.abs(g["dz"]).max())
    print(name, "relative deviations: aff", dev_aff, "out7", dev_out7, "dz", dev_dz, "| recorded:", float(g["dev_aff"]), float(g["dev_out7"]),
          float(g["dev_dz"]))
    assert got["counts"] == [int(round(float(c))) for c in g["out7"][4:]] and min(got["counts"]) >= 10
    assert dev_aff <= REF_BAR_AFF and dev_out7 <= REF_BAR_OUT7 and dev_dz <= REF_BAR_DZ, (dev_aff, dev_out7, dev_dz)
    # the label-map rule and the three-tensor contract agree on the loss: the plain formulation from pair_labels gives the same scalars
    labels = [torch.from_numpy(np.stack([pair_labels(m, r)[j] for m in g["label"]])).double() for j in range(3)]
    _, plain = A.plain_torch_loss(torch.nn.functional.elu(z).double(), labels, r)
    assert float((plain[:4] - got["out7"][:4]).abs().max()) < 1e-6


def test_aff_label_map_rule():
    K, h, w = 4, 3, 4
    la, ha = np.zeros((K, h, w), np.float32), np.zeros((K, h, w), np.float32)
    # (0,0): class 2 in both                                  -> 2
    la[2, 0, 0], ha[2, 0, 0] = 0.9, 0.8
    # (0,1): la says background, ha says class 3              -> 255 (la-background wins over the class)
    la[0, 0, 1], ha[3, 0, 1] = 0.7, 0.6
    # (0,2): la says background AND ha says background        -> 0   (ha-background overrides)
    la[0, 0, 2], ha[0, 0, 2] = 0.7, 0.6
    # (0,3): la says class 1, ha says background              -> 0
    la[1, 0, 3], ha[0, 0, 3] = 0.7, 0.6
    # (1,0): no score reaches 1e-5 (arg-max 0 in both: "background" by arg-max) -> 255 all the same
    la[1, 1, 0], ha[2, 1, 0] = 5e-6, 9e-6
    # (1,1): la class 3, ha class 1: the label is la's         -> 3
    la[3, 1, 1], ha[1, 1, 1] = 0.5, 0.4
    want = np.full((h, w), 255, np.uint8)                     # everything else: all-zero scores = no-score region
    want[0, 0], want[0, 2], want[0, 3], want[1, 1] = 2, 0, 0, 3
    got = aff_label_map(la, ha)
    assert got.dtype == np.uint8 and got.shape == (h, w)
    np.testing.assert_array_equal(got, want)
    # just at the threshold: 1e-5 is a score
    la[:, 2, 2], ha[:, 2, 2] = 0, 0
    la[2, 2, 2] = ha[2, 2, 2] = 1e-5
    assert aff_label_map(la, ha)[2, 2] == 2
    with pytest.raises(ValueError):
        aff_label_map(la, ha[:3])


def test_device_entry_points_refuse_the_cpu():
    from wseg_amd.aff_loss import affinity_loss, aff_loss_rows
    with pytest.raises(RuntimeError, match="runs only on an MI355X"):
        affinity_loss(torch.zeros(1, 8, 5, 7), torch.zeros(1, 5, 7, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="runs only on an MI355X"):
        aff_loss_rows(torch.zeros(35, 8), 8, 8, torch.zeros(1, 5, 7, dtype=torch.uint8), 1, 5, 7)


GOOD = dict(ld=64, C=64, N=2, h=13, w=16, radius=5, ld_d=64)
REJECTS = [
    (dict(radius=1), "radius 1 outside [2, 6]"),
    (dict(radius=7), "radius 7 outside [2, 6]"),
    (dict(h=4, w=4, radius=3), "a 4x4 map has no 'from' pixel at radius 3"),     # (the radius rule gives a 4x4 map radius 1: refused as well)
    (dict(h=4, w=4), "a 4x4 map has no 'from' pixel at radius 5"),
    (dict(C=12, ld=16, ld_d=16), "C=12"),
    (dict(C=520, ld=520, ld_d=520), "C=520"),
    (dict(ld=56), "C=64 ld=56"),
]


def _forward(kw, stream=None):
    ptr = C.c_void_p(L._ANY)                                   # stand-in addresses nobody dereferences: every call below is refused first
    return L.lib.wseg_aff_loss_forward(ptr, kw["ld"], kw["C"], ptr, ptr, ptr, ptr, kw["N"], kw["h"], kw["w"], kw["radius"], L.F32, stream)


def _backward(kw, stream=None):
    ptr = C.c_void_p(L._ANY)
    return L.lib.wseg_aff_loss_backward(ptr, kw["ld"], kw["C"], ptr, ptr, ptr, None, ptr, kw["ld_d"], kw["N"], kw["h"], kw["w"], kw["radius"],
                                        L.F32, stream)


def test_entry_points_exist_and_reject_bad_arguments():
    for fn in ("wseg_aff_loss_workspace_bytes", "wseg_aff_loss_forward", "wseg_aff_loss_backward"):
        assert hasattr(L.lib, fn), fn
    assert L.aff_loss_workspace_bytes(2, 13, 16, 5) == -(-2 * 9 * 8 // 4) * 24        # [blocks][6] f32, one wave of 4 per from pixel
    assert L.aff_loss_workspace_bytes(8, 56, 56, 5) == (8 * 52 * 48 // 4) * 24
    for change, text in REJECTS:
        kw = {**GOOD, **change}
        for call in (_forward, _backward):
            assert call(kw) == -1, (change, call.__name__)
            assert text in L.lib.wseg_last_error().decode(), (change, L.lib.wseg_last_error().decode())
    assert _backward({**GOOD, "ld_d": 56}) == -1 and "ld_d=56" in L.lib.wseg_last_error().decode()
    assert L.aff_loss_workspace_bytes(2, 4, 4, 3) == -1 and L.aff_loss_workspace_bytes(2, 13, 16, 7) == -1
    null = C.c_void_p(None)
    assert L.lib.wseg_aff_loss_forward(null, 64, 64, null, null, null, null, 2, 13, 16, 5, L.F32, None) == -1
    assert "null pointer" in L.lib.wseg_last_error().decode()
