"""AffinityNet inference, host side (no GPU): the pair set and radius rule against the reference's own index arrays, the stencil
reformulation of the random walk against the reference's dense squarings, the state_dict layout, and the aff_infer CLI flags."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from wseg_amd import arch, synth
from wseg_amd.resnet38_aff import indices_of_pairs, pair_offsets, pair_radius

AFF_CASES = ["aff_40x56", "aff_64x88", "aff_100x125", "aff_375x500"]


def load_case(golden_dir, name):
    if name == "aff_375x500":
        g = dict(np.load(os.path.join(golden_dir, name + "_rw.npz")))
        g["aff"] = np.load(os.path.join(golden_dir, name + "_pairs.npz"))["aff"]
        return g
    return dict(np.load(os.path.join(golden_dir, name + ".npz")))


def test_pair_indices_and_radius_match_reference(golden_dir):
    g = np.load(os.path.join(golden_dir, "aff_pair_indices.npz"))
    checked = refused = 0
    for h, w in g["sizes"].tolist():
        key = f"{h}x{w}"
        if key + "_fails" in g:                                       # the reference cannot build a pair set there: we refuse clearly
            with pytest.raises(ValueError, match="min edge >= 5"):
                pair_radius(h, w)
            refused += 1
            continue
        r = pair_radius(h, w)
        assert r == int(g[key + "_radius"]), key
        ind_from, ind_to = indices_of_pairs(r, (h, w))
        np.testing.assert_array_equal(ind_from, g[key + "_from"], err_msg=key)
        np.testing.assert_array_equal(ind_to, g[key + "_to"], err_msg=key)
        checked += 1
    assert refused == 2 and checked == len(g["sizes"]) - 2
    assert [pair_radius(5, 7), pair_radius(8, 11), pair_radius(56, 56)] == [2, 3, 5]
    assert len(pair_offsets(5)) == 34 and len(pair_offsets(2)) == 4


def test_crop_asymmetry():
    """'from' pixels are rows [0, h-r+1) x columns [r-1, w-r+1): the first r-1 columns have no edge to their right-hand neighbour."""
    h, w, r = 8, 11, 3
    ind_from, ind_to = indices_of_pairs(r, (h, w))
    P = len(pair_offsets(r))
    pairs = set(zip(np.tile(ind_from, P).tolist(), ind_to.tolist()))
    assert (0 * w + 0, 0 * w + 1) not in pairs and (1 * w + 1, 1 * w + 2) not in pairs      # columns 0, 1 (= r-1 of them): none
    assert (0 * w + 2, 0 * w + 3) in pairs
    assert (0 * w + w - 2, 0 * w + w - 1) not in pairs                                      # the right-hand r-1 columns: not from pixels
    assert ((h - 1) * w + 5, (h - 1) * w + 6) not in pairs                                  # the last r-1 rows: not from pixels
    assert ((h - r) * w + 5, (h - r) * w + 6) in pairs


def _dense(aff, h, w, r):
    ind_from, ind_to = indices_of_pairs(r, (h, w))
    area = h * w
    A = torch.zeros(area, area, dtype=torch.float64)
    fr = torch.from_numpy(np.tile(ind_from, aff.shape[0]))
    to = torch.from_numpy(ind_to)
    v = torch.from_numpy(aff.reshape(-1)).double()
    A[fr, to] = v
    A[to, fr] = v
    A[torch.arange(area), torch.arange(area)] = 1.0
    return A


@pytest.mark.parametrize("name", ["aff_40x56", "aff_64x88"])
def test_dense_matrix_from_pairs_matches_reference(golden_dir, name):
    g = load_case(golden_dir, name)
    H, W = int(g["H"]), int(g["W"])
    h, w = -(-H // 8), -(-W // 8)
    A = _dense(g["aff"], h, w, pair_radius(h, w))
    np.testing.assert_array_equal(A.float().numpy(), g["aff_mat"])


def pooled_cam(g):
    """The walk's input as aff_infer.py builds it (bg 0.27, class planes at k+1, zero padding, 8x8 average pooling)."""
    H, W = int(g["H"]), int(g["W"])
    Hp, Wp = -(-H // 8) * 8, -(-W // 8) * 8
    cams = synth.synthetic_cam_dict(H, W, g["classes"].tolist(), int(g["cam_seed"]))
    full = torch.zeros(21, Hp, Wp)
    for k, v in cams.items():
        full[k + 1, :H, :W] = v
    full[0, :H, :W] = 0.27
    return F.avg_pool2d(full, 8, 8)


def stencil_walk(aff, pooled, h, w, r, beta, logt):
    """v <- v . T, T = A^beta / colsum, 2^logt times, T never formed densely: the sparse stencil the HIP walk applies (f64 here)."""
    ind_from, ind_to = indices_of_pairs(r, (h, w))
    area = h * w
    fr = np.tile(ind_from, aff.shape[0])
    rows = np.concatenate([fr, ind_to, np.arange(area)])
    cols = np.concatenate([ind_to, fr, np.arange(area)])
    vals = np.concatenate([aff.reshape(-1), aff.reshape(-1), np.ones(area, np.float32)]).astype(np.float64) ** beta
    colsum = np.bincount(cols, weights=vals, minlength=area)
    T = torch.sparse_coo_tensor(np.stack([cols, rows]), vals / colsum[cols], (area, area))     # T^t: v_new^t = T^t v^t
    v = pooled.reshape(21, -1).double().t()
    for _ in range(2 ** logt):
        v = torch.sparse.mm(T, v)
    return v.t().reshape(21, h, w)


@pytest.mark.parametrize("name", AFF_CASES)
def test_stencil_walk_equals_dense_squaring(golden_dir, name):
    g = load_case(golden_dir, name)
    H, W = int(g["H"]), int(g["W"])
    h, w = -(-H // 8), -(-W // 8)
    rw = stencil_walk(g["aff"], pooled_cam(g), h, w, pair_radius(h, w), int(g["beta"]), int(g["logt"])).numpy()
    ref = g["cam_rw"]
    scale = np.abs(ref).reshape(21, -1).max(axis=1).reshape(21, 1, 1) + 1e-12
    err = float((np.abs(rw - ref) / scale).max())
    assert err < 1e-4, err


def test_aff_state_dict_spec_matches_reference_keys(golden_dir):
    g = np.load(os.path.join(golden_dir, "aff_state_dict_keys.npz"))
    spec = arch.state_dict_spec(arch.AFF_HEAD_CONVS)
    assert list(spec.keys()) == [str(k) for k in g["keys"]]
    assert [",".join(str(d) for d in s) for s in spec.values()] == [str(s) for s in g["shapes"]]
    sd = synth.procedural_aff_state_dict(0)
    assert list(sd.keys()) == list(spec.keys()) and all(tuple(sd[k].shape) == spec[k] for k in spec)
    assert len(arch.state_dict_spec()) == 233 and list(arch.state_dict_spec())[-1] == "f9.weight"     # the contrast table is unchanged
    base = synth.procedural_state_dict(0)
    for k in base:
        if k.split(".")[0] not in arch.AFF_HEAD_CONVS and k.split(".")[0] not in arch.HEAD_CONVS:
            assert torch.equal(sd[k], base[k]), k                                                  # the backbone is shared


def test_aff_net_module_contract():
    from wseg_amd.resnet38_aff import Net
    m = Net(precision="fp32")
    assert list(m.state_dict().keys()) == list(arch.state_dict_spec(arch.AFF_HEAD_CONVS).keys())
    m.load_state_dict(synth.procedural_aff_state_dict(0), strict=True)
    groups = m.get_parameter_groups()
    assert [len(g) for g in groups] == [len([k for k in m.state_dict() if k.endswith("weight") and "bn" not in k]) - 4, 0, 4, 0]
    assert groups[2][3] is m.f9.weight
    with pytest.raises(RuntimeError, match="inference-only"):
        m.train()(torch.zeros(1, 3, 64, 64))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.eval()(torch.zeros(1, 3, 64, 64))


def test_aff_infer_cli_flags():
    from wseg_amd.aff_infer import build_parser
    a = build_parser().parse_args(["--weights", "w.pth", "--cam_dir", "cams"])
    assert (a.network, a.infer_list, a.num_workers, a.voc12_root, a.out_rw) == \
        ("wseg_amd.resnet38_aff", "voc12/val.txt", 8, "VOC2012", "out_rw")
    assert (a.alpha, a.beta, a.logt, a.crf, a.precision) == (6, 8, 6, False, None)
    a = build_parser().parse_args(["--weights", "procedural", "--cam_dir", "c", "--beta", "4", "--logt", "3", "--precision", "fp32",
                                   "--alpha", "12"])
    assert (a.weights, a.beta, a.logt, a.precision, a.alpha) == ("procedural", 4, 3, "fp32", 12.0)
    with pytest.raises(SystemExit):
        build_parser().parse_args(["--weights", "w.pth"])                 # --cam_dir is required
