"""wseg_amd.stage_io on the device: WriteBehind's order, depth, pinned copies and drain; DescRing's uploads beyond its slots and capacity.
(cam_planes, load_net and the optimizer groups need no stream: tests/test_stage_io_host.py.)"""
import ctypes as C

import numpy as np
import pytest
import torch

from wseg_amd.stage_io import DescRing, WriteBehind

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _ramp(shape, dtype):
    return (torch.arange(int(np.prod(shape)), device=DEV) % 50).to(dtype).view(shape)


def _tree(i):
    """the device tree of item i: four kinds, cycled"""
    kind = i % 4
    if kind == 0:
        return _ramp((3, 5), torch.uint8)
    if kind == 1:
        return {3: _ramp((7, 13), torch.float32), 11: _ramp((7, 13), torch.float32) * 0.5, "none": None}
    if kind == 2:
        return (_ramp((4,), torch.int64), None, [_ramp((2, 3), torch.float32)])
    return _ramp((1,), torch.float32)


def _leaves(tree):
    if tree is None:
        return []
    if isinstance(tree, dict):
        return [x for v in tree.values() for x in _leaves(v)]
    if isinstance(tree, (tuple, list)):
        return [x for v in tree for x in _leaves(v)]
    return [tree]


def _same_structure(a, b):
    if isinstance(a, dict):
        return isinstance(b, dict) and list(a) == list(b) and all(_same_structure(a[k], b[k]) for k in a)
    if isinstance(a, (tuple, list)):
        return type(a) is type(b) and len(a) == len(b) and all(_same_structure(x, y) for x, y in zip(a, b))
    return (a is None) == (b is None)


@pytest.mark.parametrize("depth", [1, 2])
def test_write_behind_order_depth_and_pinned_copies(depth):
    written, expect = [], {}
    wb = WriteBehind(lambda key, host: written.append((key, host)), depth=depth)
    for i in range(7):
        tree = _tree(i)
        expect[i] = [(t + (i + 1)).cpu() for t in _leaves(tree)]
        for t in _leaves(tree):
            t.add_(i + 1)                                        # a device kernel right in front of the submit: the copy must come after it
        wb.submit(i, tree)
        assert [k for k, _ in written] == list(range(max(0, i + 1 - depth)))         # exactly the items older than `depth`, in order
    wb.close()
    assert [k for k, _ in written] == list(range(7))
    wb.close()
    assert len(written) == 7
    for i, (key, host) in enumerate(written):
        assert _same_structure(_tree(i), host)
        leaves = _leaves(host)
        assert len(leaves) == len(expect[i])
        for h, e in zip(leaves, expect[i]):
            assert h.device.type == "cpu" and h.is_pinned() and h.dtype == e.dtype and torch.equal(h, e), (i, h, e)


def test_write_behind_context_manager_and_a_failing_write():
    written = []
    with WriteBehind(lambda key, host: written.append(key)) as wb:
        for i in range(3):
            wb.submit(i, _tree(i))
        assert written == [0, 1]
    assert written == [0, 1, 2]                                  # leaving the block drains

    def write(key, host):
        if key == 1:
            raise OSError("disk full")
        written.append(key)
    del written[:]
    wb = WriteBehind(write)
    wb.submit(0, _tree(0))
    wb.submit(1, _tree(1))
    with pytest.raises(OSError, match="disk full"):
        wb.submit(2, _tree(2))                                   # writes item 1: its exception reaches the caller
    wb.close()
    assert written == [0, 2]                                     # the failed item is not written twice
    with pytest.raises(OSError, match="disk full"):
        with WriteBehind(write) as wb:
            wb.submit(0, _tree(0))
            wb.submit(1, _tree(1))                               # item 1 is written on the way out


class _Desc(C.Structure):
    _fields_ = [("p", C.c_void_p), ("a", C.c_int32), ("b", C.c_float)]


def test_desc_ring_uploads_beyond_its_slots_and_capacity():
    ring = DescRing(DEV)
    rng = np.random.default_rng(3)
    sizes = [(1, 1), (4, 37), (64, 5), (3, 1000), (17, 17), (2, DescRing.MIN_BYTES + 100), (5, 9), (1, 15), (40, 16), (8, 33), (2, 2), (9, 4000)]
    assert len(sizes) == 12 and any(C.sizeof(_Desc) * n + m > DescRing.MIN_BYTES for n, m in sizes)
    kept = []
    for n, m in sizes:
        descs, raw = (_Desc * n)(), (C.c_uint8 * m)(*rng.integers(0, 256, m).tolist())
        for j in range(n):
            descs[j].p, descs[j].a, descs[j].b = int(rng.integers(1, 2 ** 48)), int(rng.integers(-2 ** 31, 2 ** 31)), float(rng.random())
        d, offs = ring.upload(descs, raw)
        assert d.dtype == torch.uint8 and d.device.type == "cuda" and len(offs) == 2 and all(o % 16 == 0 for o in offs)
        assert offs[0] == 0 and offs[1] >= C.sizeof(descs) and d.numel() == offs[1] + m
        kept.append((d, offs, bytes(descs), bytes(raw)))
    torch.cuda.synchronize()
    for d, offs, b0, b1 in kept:
        host = d.cpu().numpy().tobytes()
        assert host[offs[0]:offs[0] + len(b0)] == b0 and host[offs[1]:offs[1] + len(b1)] == b1


def test_desc_ring_to_device():
    ring = DescRing(DEV)
    t = torch.arange(1000, dtype=torch.int32)
    for src in (t, t.pin_memory()):
        d = ring.to_device(src)
        assert d.device.type == "cuda" and torch.equal(d.cpu(), t)
