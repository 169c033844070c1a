"""wseg_amd.stage_io on the host: cam_planes (the in-place view, the stacked copy, the refusals, and parity with the stacking every
consumer did before it was shared), load_net and the optimizer's four groups.  CPU tensors only; WriteBehind and DescRing need a stream
(tests/test_gpu_stage_io.py)."""
import numpy as np
import pytest
import torch

from wseg_amd import synth
from wseg_amd.stage_io import cam_planes, load_net

H, W = 7, 13                      # H * W = 91 is odd: a float4 shortcut over the planes would show


def _views(classes, seed=0):
    """what infer_image returns: views into one [20, H, W] tensor — NaN wherever no chosen class lives"""
    full = torch.full((20, H, W), float("nan"))
    g = torch.Generator().manual_seed(seed)
    for c in classes:
        full[c] = torch.rand(H, W, generator=g)
    return full, {c: full[c] for c in classes}


def _parent_stack(cam_dict):
    """the stacking path as every consumer wrote it before: float32 maps over the sorted keys, plane i at position i"""
    keys = sorted(cam_dict)
    return keys, torch.stack([cam_dict[k].float() if torch.is_tensor(cam_dict[k]) else torch.as_tensor(np.asarray(cam_dict[k], np.float32))
                              for k in keys])


def _check_parity(cam_dict, planes, idx):
    keys, ref = _parent_stack(cam_dict)
    assert len(idx) == 20 and [c for c in range(20) if idx[c] >= 0] == [int(k) for k in keys]
    for i, k in enumerate(keys):
        assert planes[idx[int(k)]].dtype == torch.float32 and torch.equal(planes[idx[int(k)]], ref[i]), k


@pytest.mark.parametrize("classes", [[3, 5, 8], [11], [0, 1, 2]])
def test_cam_planes_reads_views_of_one_tensor_in_place(classes):
    full, d = _views(classes)
    planes, idx, size = cam_planes(d, (H, W), "cpu")
    assert size == (H, W)
    assert planes.data_ptr() == full[classes[0]].data_ptr() and planes.shape == (classes[-1] - classes[0] + 1, H, W)
    assert planes.stride() == (H * W, W, 1)
    assert idx == [c - classes[0] if c in classes else -1 for c in range(20)]
    assert not any(torch.isnan(planes[i]).any() for i in idx if i >= 0)
    _check_parity(d, planes, idx)
    planes2, idx2, size2 = cam_planes(d, None, "cpu")                           # without size=: the maps' own
    assert planes2.data_ptr() == planes.data_ptr() and idx2 == idx and size2 == (H, W)


def _copy_cases():
    rng = np.random.default_rng(5)
    full, views = _views([2, 9])
    wide, flat = torch.rand(3, W, H), torch.rand(3 * H * W)
    return {
        "numpy float64": {4: rng.random((H, W)), 17: rng.random((H, W))},
        "numpy and torch": {1: rng.random((H, W)).astype(np.float32), 6: torch.rand(H, W)},
        "two storages": {0: torch.rand(H, W), 19: torch.rand(H, W)},
        "transposed view": {5: wide[0].t(), 7: wide[2].t()},
        "keys out of order": {12: views[9], 3: torch.rand(H, W), 8: views[2]},
        "float64 views": dict(zip((2, 3), torch.rand(2, H, W, dtype=torch.float64))),
        "views no whole plane apart": {0: flat[:H * W].view(H, W), 1: flat[H * W + 5:2 * H * W + 5].view(H, W)},
    }


@pytest.mark.parametrize("case", list(_copy_cases()))
def test_cam_planes_copies_anything_else_once(case):
    d = _copy_cases()[case]
    planes, idx, size = cam_planes(d, (H, W), "cpu")
    assert size == (H, W) and planes.shape == (len(d), H, W) and planes.is_contiguous() and planes.dtype == torch.float32
    assert all(planes.data_ptr() != v.data_ptr() for v in d.values() if torch.is_tensor(v))
    assert [idx[k] for k in sorted(d)] == list(range(len(d)))
    _check_parity(d, planes, idx)


def test_cam_planes_empty_dictionary():
    planes, idx, size = cam_planes({}, (H, W), "cpu")
    assert planes is None and idx == [-1] * 20 and size == (H, W)
    assert cam_planes({}, (H, W), "cpu", n_classes=5)[1] == [-1] * 5
    with pytest.raises(ValueError, match="size"):
        cam_planes({}, None, "cpu")


@pytest.mark.parametrize("bad", [20, -1, 3.5])
def test_cam_planes_refuses_a_key_that_is_no_class(bad):
    with pytest.raises(ValueError, match="CAM classes"):
        cam_planes({2: np.zeros((H, W), np.float32), bad: np.zeros((H, W), np.float32)}, (H, W), "cpu")
    full, d = _views([2, 4])
    with pytest.raises(ValueError, match="CAM classes"):                         # (views of one tensor: the same rule before the in-place path)
        cam_planes({2: d[2], bad: d[4]}, (H, W), "cpu")


def test_cam_planes_refuses_differing_and_unexpected_shapes():
    with pytest.raises(ValueError, match="shapes"):
        cam_planes({1: torch.zeros(H, W), 2: torch.zeros(H, W + 1)}, None, "cpu")
    with pytest.raises(ValueError, match="shapes"):
        cam_planes({1: np.zeros((H, W)), 2: torch.zeros(W, H)}, None, "cpu")
    with pytest.raises(ValueError, match="shapes"):
        cam_planes({1: torch.zeros(H, W)}, (H, W + 1), "cpu")
    with pytest.raises(ValueError, match="shapes"):
        cam_planes(_views([3, 5])[1], (W, H), "cpu")


@pytest.fixture(scope="module")
def aff_sd():
    return synth.procedural_aff_state_dict(0)


def _assert_holds(model, ref):
    got = model.state_dict()
    assert set(ref) <= set(got)
    for k, v in ref.items():
        assert torch.equal(got[k], v), k


def test_load_net_procedural_contrast(proc_sd):
    _assert_holds(load_net("wseg_amd.resnet38_contrast", "procedural", "fp32", synth.procedural_state_dict), proc_sd)


def test_load_net_procedural_aff(aff_sd):
    _assert_holds(load_net("wseg_amd.resnet38_aff", "procedural", None, synth.procedural_aff_state_dict), aff_sd)


def test_load_net_from_a_file_and_the_params_refusal(tmp_path, aff_sd):
    torch.save(aff_sd, tmp_path / "w.pth")                       # (a fresh Net holds random weights: equality comes from the file alone)
    _assert_holds(load_net("wseg_amd.resnet38_aff", str(tmp_path / "w.pth"), "fp32", synth.procedural_aff_state_dict), aff_sd)
    with pytest.raises(SystemExit, match=r"mxnet \.params conversion needs mxnet \(absent offline\): convert to a \.pth state_dict first"):
        load_net("wseg_amd.resnet38_aff", "x.params", None, synth.procedural_aff_state_dict)


def test_build_optimizer_groups():
    from wseg_amd import aff_train, optim
    assert aff_train.build_optimizer is optim.build_optimizer

    class Model:                                                 # (the four lists every Net.get_parameter_groups returns)
        groups = [[torch.nn.Parameter(torch.zeros(i + 1))] for i in range(4)]

        def get_parameter_groups(self):
            return self.groups
    lr, wd = 0.01, 5e-4
    opt = optim.build_optimizer(Model(), lr, wd, 100)
    assert all(len(g['params']) == 1 and g['params'][0] is m[0] for g, m in zip(opt.param_groups, Model.groups))
    assert [g['lr'] for g in opt.param_groups] == [lr, 2 * lr, 10 * lr, 20 * lr]
    assert [g['weight_decay'] for g in opt.param_groups] == [wd, 0, wd, 0]
    assert opt.max_step == 100 and opt.global_step == 0
