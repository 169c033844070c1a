"""Host plumbing the stage CLIs and the two device data paths share, each piece once: the write-behind of results (`WriteBehind`), a CAM
dictionary as planes + class index (`cam_planes`), the page-locked descriptor ring (`DescRing`) and model construction (`load_net`).
Imports without a GPU and without the library; nothing here launches a kernel."""
import collections
import ctypes as C
import importlib

import numpy as np
import torch


def _to_pinned(tree):
    if tree is None:
        return None
    if isinstance(tree, dict):
        return {k: _to_pinned(v) for k, v in tree.items()}
    if isinstance(tree, (tuple, list)):
        return type(tree)(_to_pinned(v) for v in tree)
    host = torch.empty(tree.shape, dtype=tree.dtype, pin_memory=True)
    return host.copy_(tree, non_blocking=True)


class WriteBehind:
    """`depth` items behind: submit(key, tree) starts the device tensors of `tree` (a tensor, or a dict / tuple / list of them; None entries
    pass through) on their way to pinned host buffers, records an event on the current stream, and only then calls write(key, host_tree)
    for the items older than `depth` — the png / npy writes and the loader hand-over overlap the GPU instead of alternating with it (the
    reference's loops sync per image on `.cpu()`).  close() writes the rest; leaving the `with` block on an exception writes nothing more."""

    def __init__(self, write, depth=1):
        self.write, self.depth, self._queue = write, depth, collections.deque()

    def submit(self, key, tree):
        host, ev = _to_pinned(tree), torch.cuda.Event()
        ev.record()
        self._queue.append((key, host, ev))
        self._drain(self.depth)

    def _drain(self, keep):
        while len(self._queue) > keep:
            key, host, ev = self._queue.popleft()
            ev.synchronize()
            self.write(key, host)

    def close(self):
        self._drain(0)

    def __enter__(self):
        return self

    def __exit__(self, exc_type, exc, tb):
        if exc_type is None:
            self.close()
        self._queue.clear()


def cam_planes(cam_dict, size=None, device="cuda", n_classes=20):
    """{class 0..n_classes-1: [H, W]} (numpy or torch) -> (planes float32 [P, H, W] on `device` or None, idx, (H, W)): idx[c] is the plane
    of class c, -1 if absent.  Contiguous float32 views of one tensor on `device`, whole planes apart (infer_image's dictionary), are
    read in place: `planes` is a view from the lowest to the highest of them.  Anything else is stacked over the sorted keys and copied
    once.  An empty dictionary gives None and needs `size`.  Bad keys, differing shapes and a shape other than `size` are ValueErrors."""
    idx = [-1] * n_classes
    if not cam_dict:
        if size is None:
            raise ValueError("an empty CAM dictionary needs size=(H, W)")
        return None, idx, tuple(size)
    keys = sorted(cam_dict)
    if any(int(k) != k or not 0 <= k < n_classes for k in keys):
        raise ValueError(f"CAM classes {keys} outside the integers 0..{n_classes - 1}")
    maps = [cam_dict[k] for k in keys]
    shapes = {m.shape for m in maps}                              # (torch.Size and numpy's tuple compare and hash alike)
    if len(shapes) != 1 or len(min(shapes)) != 2 or (size is not None and shapes != {tuple(size)}):
        raise ValueError(f"CAM maps of shapes {sorted(shapes)}, expected one [H, W]" + (f" = {tuple(size)}" if size is not None else ""))
    (H, W), dev = min(shapes), torch.device(device)
    if dev.type == "cuda" and dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())      # with its index, as tensors report it
    n = H * W
    if n and all(isinstance(m, torch.Tensor) and m.dtype == torch.float32 and m.device == dev and m.is_contiguous() for m in maps) \
            and len({m.untyped_storage().data_ptr() for m in maps}) == 1:
        offs = [m.storage_offset() for m in maps]
        lo = min(offs)
        if all((o - lo) % n == 0 for o in offs) and len(set(offs)) == len(offs):
            planes = maps[offs.index(lo)].as_strided(((max(offs) - lo) // n + 1, H, W), (n, W, 1))
            for k, o in zip(keys, offs):
                idx[int(k)] = (o - lo) // n
            return planes, idx, (H, W)
    maps = [m.detach().float() if torch.is_tensor(m) else torch.as_tensor(np.asarray(m, np.float32)) for m in maps]
    if len({m.device for m in maps}) > 1:
        maps = [m.to(dev) for m in maps]
    for i, k in enumerate(keys):
        idx[int(k)] = i
    return torch.stack(maps).to(dev, non_blocking=True).contiguous(), idx, (H, W)


class DescRing:
    """Page-locked staging for the small descriptor arrays a batched launch reads: a pageable copy would make the host wait for the
    stream (= the whole previous training step) on every call.  `slots` buffers take turns; one is reused only after the upload that
    last left it has completed, and replaced when it is too small."""
    MIN_BYTES = 16384

    def __init__(self, device, slots=4):
        self.device, self._ring, self._slot = torch.device(device), [None] * slots, 0

    def to_device(self, t):
        """(a DataLoader with pin_memory=True hands over page-locked blobs: its pinning thread did the copy in the background)"""
        return (t if t.is_pinned() else t.pin_memory()).to(self.device, non_blocking=True)

    def upload(self, *arrays):
        """ctypes arrays -> (uint8 device tensor holding them back to back, the 16-byte aligned byte offset of each), one copy"""
        offs, nbytes = [], 0
        for a in arrays:
            offs.append((nbytes + 15) // 16 * 16)
            nbytes = offs[-1] + C.sizeof(a)
        entry = self._ring[self._slot]
        if entry is None or entry[0].numel() < nbytes:
            entry = self._ring[self._slot] = (torch.empty(max(nbytes, self.MIN_BYTES), dtype=torch.uint8).pin_memory(), torch.cuda.Event())
        else:
            entry[1].synchronize()                            # the copy that last used this slot has been consumed
        stage, ev = entry
        for a, o in zip(arrays, offs):
            C.memmove(stage.data_ptr() + o, C.addressof(a), C.sizeof(a))
        d_desc = stage[:nbytes].to(self.device, non_blocking=True)
        ev.record()
        self._slot = (self._slot + 1) % len(self._ring)
        return d_desc, offs


def load_net(network, weights, precision, procedural, strict=True, device=None, warn_mismatch=False):
    """`Net` of the module `network` (with precision= if given) holding `weights`: "procedural" -> procedural(0) (made on `device` if
    given), else a .pth state_dict.  warn_mismatch: a tensor of another size is printed, not raised (aff_train.py:88-92)."""
    Net = getattr(importlib.import_module(network), 'Net')
    model = Net(precision=precision) if precision else Net()
    if weights == "procedural":
        weights_dict = procedural(0, device=device or "cpu")
    elif weights[-7:] == '.params':
        raise SystemExit("mxnet .params conversion needs mxnet (absent offline): convert to a .pth state_dict first")
    else:
        weights_dict = torch.load(weights, map_location="cpu", weights_only=True)
    try:
        model.load_state_dict(weights_dict, strict=strict)
    except RuntimeError as e:
        if not warn_mismatch:
            raise
        print(e)
    return model
