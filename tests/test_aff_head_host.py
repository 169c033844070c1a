"""AffinityNet head training path, host side (no GPU): the ELU-backward entry point's argument checks (they run before any device call),
the device-only error of the autograd entry, the transposed-pack table of the four head convs, and the planners' answer to every GEMM
launch the backward issues."""
import ctypes as C

import pytest
import torch

from wseg_amd import _lib as L
from wseg_amd.aff_head import BRANCHES, affinity_head, backward_launches

GOOD = dict(ld_g=448, g_dtype=L.F32, ld_y=448, y_dtype=L.BF16, ld_dz=448, dz_dtype=L.BF16, M=35, C=448, g=L._ANY, y=L._ANY, dz=L._ANY)
REJECTS = [
    (dict(C=12), "C=12"),
    (dict(C=0), "C=0"),
    (dict(ld_g=452), "ld_g=452"),
    (dict(ld_y=100, C=96), "ld_y=100"),
    (dict(ld_dz=440), "ld_dz=440"),
    (dict(g=L._ANY + 8), "16-byte aligned"),
    (dict(dz=L._ANY + 4), "16-byte aligned"),
    (dict(g_dtype=7), "bad dtype (g 7"),
    (dict(dz_dtype=L.F32X3), "bad dtype"),
    (dict(M=0), "M=0"),
    (dict(g=None), "null pointer"),
    (dict(g=L._ANY, dz=L._ANY, g_dtype=L.F32, dz_dtype=L.BF16, alias=True), "alias"),
]


def _call(kw):
    """stand-in addresses nobody dereferences: every call made here is refused first"""
    return L.lib.wseg_elu_backward_rows(C.c_void_p(kw["g"]), kw["ld_g"], kw["g_dtype"], C.c_void_p(kw["y"]), kw["ld_y"], kw["y_dtype"], None,
                                        C.c_void_p(kw["dz"]), kw["ld_dz"], kw["dz_dtype"], C.c_long(kw["M"]), kw["C"], None)


def test_elu_backward_entry_point_exists_and_rejects_bad_arguments():
    assert hasattr(L.lib, "wseg_elu_backward_rows") and callable(L.elu_backward_rows)
    for change, text in REJECTS:
        kw = {**GOOD, **change}
        if kw.pop("alias", False):                            # dz == g with another dtype
            kw["y"] = L._ANY + 16
        else:
            kw["y"], kw["dz"] = kw["y"] + 1024, (kw["dz"] + 2048 if kw["dz"] else kw["dz"])       # three distinct buffers
        assert _call(kw) == -1, change
        assert text in L.lib.wseg_last_error().decode(), (change, L.lib.wseg_last_error().decode())
    # the binding refuses a tensor too short for its rows before any pointer leaves Python
    with pytest.raises(RuntimeError, match="dz has 64 elements"):
        L.elu_backward_rows(torch.zeros(35, 8), 8, torch.zeros(35, 8), 8, None, torch.zeros(8, 8), 8, 35, 8)


def test_affinity_head_refuses_the_cpu():
    from wseg_amd.resnet38_aff import Net
    net = Net(precision="fp32")
    with pytest.raises(RuntimeError, match="runs only on an MI355X"):
        affinity_head(net, torch.zeros(1, 512, 5, 7), torch.zeros(1, 1024, 5, 7), torch.zeros(1, 4096, 5, 7))
    # the transposed-pack table: the four masters close the flat buffers in the order f8_3, f8_4, f8_5, f9; packs are [IC][1][OC]
    eng = net._engine
    eng._ensure_flat(torch.device("cpu"))
    specs = eng.head_wt_specs()
    assert [s[0] for s in specs] == ["f8_3", "f8_4", "f8_5", "f9"]
    assert [s[3] for s in specs] == [(512, 1, 64), (1024, 1, 128), (4096, 1, 256), (448, 1, 448)]
    end = eng.flat_w.numel()
    for name, off, n, (ci, t, co) in reversed(specs):
        assert n == ci * t * co and off + n == end and off % 32 == 0, name       # (whole 32-element groups: the split-bf16 pack)
        assert getattr(net, name).weight.data_ptr() == eng.flat_w[off:].data_ptr()
        end = off
    assert eng.grad_slice("f9").numel() == 448 * 448 and eng.grad_slice("f9").data_ptr() == eng.flat_g[specs[3][1]:].data_ptr()


MAPS = [(1, 5, 7), (2, 13, 16), (3, 19, 23), (8, 56, 56)]


@pytest.mark.parametrize("dt", [L.F32, L.BF16, L.F32X3], ids=["fp32", "bf16", "bf16x3"])
@pytest.mark.parametrize("N,h,w", MAPS)
def test_planners_accept_every_backward_launch(N, h, w, dt):
    M = N * h * w
    for epi1 in (False, True):
        la = backward_launches(N, h, w, dt, epi1=epi1)
        assert list(la) == ["wgrad_f9", "dgrad_f9"] + [k + n for n, _ in BRANCHES for k in ("wgrad_", "dgrad_")]
        for key, kw in la.items():
            name = key.split("_", 1)[1]
            co, ci = {"f8_3": (64, 512), "f8_4": (128, 1024), "f8_5": (256, 4096), "f9": (448, 448)}[name]
            if key.startswith("dgrad"):
                ops = dict(scale=L._ANY, mask=L._ANY, drop=L._ANY) if kw.get("epi") == 1 else {}
                assert (kw.get("epi") == 1) == (epi1 and name == "f8_5")
                p = L.conv_plan(**kw, **ops)
                assert p.family in (L.CONV_64x128, L.CONV_128x128, L.CONV_224x256, L.CONV_256x256), (key, p)
                assert p.tile_cols in (128, 256) and p.nwg == -(-M // p.tile_rows) * -(-ci // p.tile_cols), (key, p)
                assert kw["mode"] == 1 and kw["IC"] == co and kw["OC"] == ci and kw.get("ld_in", co) == (448 if name != "f9" else co)
                if p.family in (L.CONV_224x256, L.CONV_256x256):
                    assert dt != L.F32 and ci % 256 == 0 and p.tapf == 1 and p.perm == 0, (key, p)
            else:
                p = L.wgrad_plan(**kw)
                assert p.family in (L.WGRAD_128x128, L.WGRAD_256x256) and p.nsplit >= 1 and p.nwg > 0, (key, p)
                assert kw["IC"] == ci and kw["OC"] == co and kw.get("ld_dy", co) == 448
                if p.family == L.WGRAD_256x256:
                    assert dt == L.BF16 and min(ci, co) >= 256 and M >= 16384, (key, p)
    # the 256-tile families appear at the training shape only
    if M < 16384:
        assert all(L.conv_plan(**kw).family in (L.CONV_64x128, L.CONV_128x128) for k, kw in backward_launches(N, h, w, dt).items() if k[0] == "d")
