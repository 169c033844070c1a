"""The conv / wgrad launch planner through its query entry points (wseg_conv_plan, wseg_wgrad_plan, wseg_conv_bwd_pair_plan): pure host
arithmetic — the function the launches themselves ask — so these tests need no GPU.  Pointers are stand-in addresses nobody dereferences."""
import pytest

from wseg_amd import _lib as L

CONV = dict(N=2, IH=20, IW=20, IC=64, OH=20, OW=20, OC=128, KH=3, KW=3, pad=1)
WGRAD = dict(N=2, IH=20, IW=20, IC=64, OH=20, OW=20, OC=128, KH=3, KW=3, pad=1)
TWO = dict(N=2, IH=20, IW=20, IC=128, OH=20, OW=20, OC=256, KH=1, KW=1, in2=L._ANY, IC2=128)      # a valid two-source launch


# every rejection of the planner before it became one function (conv_validate, conv_fill_args, wseg_conv_igemm, conv_plan_256), each with a
# descriptor that trips it: (changes to CONV or TWO, text of wseg_last_error)
CONV_REJECTS = [
    (CONV, dict(inp=None), "conv_igemm: null pointer"),
    (CONV, dict(w=None), "conv_igemm: null pointer"),
    (CONV, dict(out=None), "conv_igemm: null pointer"),
    (CONV, dict(dtype=3), "conv_igemm: bad dtype 3"),
    (CONV, dict(IC=32), "conv_igemm: IC=32 must be a multiple of 64"),
    (CONV, dict(IC=16, ld_in=64, dtype=L.F32), "conv_igemm: IC=16 must be a multiple of 32"),
    (CONV, dict(OC=12), "conv_igemm: OC=12 / ld_in=64 must be multiples of 8"),
    (CONV, dict(ld_in=68), "conv_igemm: OC=128 / ld_in=68 must be multiples of 8"),
    (CONV, dict(OH=0), "conv_igemm: empty shape"),
    (CONV, dict(stride=0), "conv_igemm: bad geometry"),
    (CONV, dict(mode=2), "conv_igemm: bad mode"),
    (CONV, dict(epi=4), "conv_igemm: bad epilogue"),
    (CONV, dict(IC=128, ld_in=64), "conv_igemm: ld_in < IC"),
    (CONV, dict(ld_out=120), "conv_igemm: bad ld_out"),
    (CONV, dict(out2=L._ANY, epi=1), "conv_igemm: bad out2"),
    (CONV, dict(out2=L._ANY, ld_out2=132), "conv_igemm: bad out2"),
    (CONV, dict(r_pre=L._ANY, ld_rpre=132), "conv_igemm: bad ld_rpre"),
    (CONV, dict(r_post=L._ANY, ld_rpost=132), "conv_igemm: bad ld_rpost"),
    (CONV, dict(mask=L._ANY, ld_mask=132), "conv_igemm: bad ld_mask"),
    (CONV, dict(seg2=(8, 8, 8, 0)), "conv_igemm: bad second segment"),
    (CONV, dict(seg2=(8, 8, -1, 8)), "conv_igemm: bad second segment"),
    (CONV, dict(w_rows=64), "conv_igemm: w_rows=64 < OC=128"),
    (CONV, dict(N=40000, OH=300, OW=300, IH=300, IW=300), "conv_igemm: tensor too large"),
    (TWO, dict(stride=2), "conv_igemm: the two-source form is a same-size stride-1 bf16 convolution with OC % 256 == 0 on the 256-tile kernel"),
    (TWO, dict(OC=128), "conv_igemm: the two-source form is"),
    (TWO, dict(KH=3, KW=3, pad=0), "conv_igemm: the two-source form is"),
    (TWO, dict(dtype=L.F32X3), "conv_igemm: the two-source form is"),
    (TWO, dict(bm_hint=128), "conv_igemm: the two-source form is"),
    (TWO, dict(epi=3), "conv_igemm: the two-source form is"),      # (new: ELU exists on the 64 / 128-row tiles only, which do not read in2)
    (TWO, dict(IC2=96), "conv_igemm: IC2=96 must be a multiple of 64 and <= ld_in2"),
    (TWO, dict(ld_in2=64), "conv_igemm: IC2=128 must be a multiple of 64 and <= ld_in2"),
    (CONV, dict(out=None, out2=L._ANY, epi=0, bm_hint=257), "conv_igemm: bm_hint 257 was a development hook and no longer exists"),
    (CONV, dict(bm_hint=258), "conv_igemm: bm_hint 258 was a development hook"),
    (CONV, dict(bm_hint=-1), "conv_igemm: bm_hint -1 was a development hook"),
    (CONV, dict(IC=256, OC=256, IH=20000, OH=20000, IW=4, OW=4, N=1, bm_hint=256), "conv_igemm: shape too large for the 256-tile kernel"),
    (CONV, dict(IH=9000, OH=9000, IW=4, OW=4, N=1, bm_hint=259), "conv_igemm: shape too large for the 512x128-tile kernel"),
]
WGRAD_REJECTS = [
    (dict(x=None), "conv_wgrad: null pointer"),
    (dict(dtype=3), "conv_wgrad: bad dtype"),
    (dict(IC=60), "conv_wgrad: IC/OC/ld must be multiples of 8 (IC=60 OC=128 ld_x=60 ld_dy=128)"),
    (dict(ld_x=32), "conv_wgrad: leading dims too small"),
    (dict(IC_dw=72), "conv_wgrad: bad dw extents"),
    (dict(dw_rot=64), "conv_wgrad: dw_rot=64 must lie in [0, IC_dw)"),
    (dict(dil=0), "conv_wgrad: bad shape"),
    (dict(seg2=(8, 8, 8, 0)), "conv_wgrad: bad second segment"),
    (dict(N=40000, OH=300, OW=300, IH=300, IW=300), "conv_wgrad: too many pixels"),
    (dict(IC=256, OC=256, tile_hint=256, dw_rot=3), "conv_wgrad: dw_rot is supported by the 128-tile kernel only"),
]


def _split(kw):
    """(positional stand-ins, keywords) of a plan call: inp / w / out / out2 (x / dy / dw) given as keywords replace the stand-in address"""
    kw = dict(kw)
    pos = {k: kw.pop(k) for k in ("inp", "w", "out", "out2", "x", "dy", "dw") if k in kw}
    return pos, kw


@pytest.mark.parametrize("base,change,message", CONV_REJECTS, ids=[f"{i}-{m[12:40]}" for i, (_b, _c, m) in enumerate(CONV_REJECTS)])
def test_conv_plan_rejections(base, change, message):
    assert L.conv_plan(**base).nwg > 0                       # the descriptor is good before the change
    pos, kw = _split({**base, **change})
    with pytest.raises(RuntimeError) as e:
        L.conv_plan(**pos, **kw)
    assert message in str(e.value)


@pytest.mark.parametrize("change,message", WGRAD_REJECTS, ids=[m[12:40] for _c, m in WGRAD_REJECTS])
def test_wgrad_plan_rejections(change, message):
    assert L.wgrad_plan(**WGRAD).nwg > 0
    pos, kw = _split({**WGRAD, **change})
    with pytest.raises(RuntimeError) as e:
        L.wgrad_plan(**pos, **kw)
    assert message in str(e.value)


def test_hints_force_what_they_say():
    """bm_hint / tile_hint name a kernel: the plan is that kernel wherever it takes the shape; where it does not, the launch runs on the 64 / 128-row
    tiles (as before the plan could be asked — now the fallback is visible), and the retired development hooks fail loudly."""
    big = dict(N=2, IH=40, IW=40, IC=256, OH=40, OW=40, OC=256, KH=3, KW=3, pad=1)
    for bm, family, rows, cols in ((64, L.CONV_64x128, 64, 128), (128, L.CONV_128x128, 128, 128), (224, L.CONV_224x256, 224, 256),
                                   (256, L.CONV_256x256, 256, 256), (259, L.CONV_512x128, 512, 128)):
        p = L.conv_plan(bm_hint=bm, **big)
        assert (p.family, p.tile_rows, p.tile_cols) == (family, rows, cols)
        assert p.nwg == -(-3200 // rows) * (256 // cols)
    rows_64_128 = (L.CONV_64x128, L.CONV_128x128)
    assert L.conv_plan(bm_hint=256, **{**big, "OC": 128}).family in rows_64_128              # OC % 256 != 0 and no padded pack
    assert L.conv_plan(bm_hint=256, **{**big, "OC": 192, "w_rows": 256}).family == L.CONV_256x256   # ... with one: whole 256-row weight tiles
    assert L.conv_plan(bm_hint=224, epi=3, **big).family in rows_64_128                      # ELU exists on the 64 / 128-row tiles only
    assert L.conv_plan(bm_hint=259, epi=3, **big).family in rows_64_128
    assert L.conv_plan(bm_hint=259, mode=1, stride=2, **{**big, "OH": 80, "OW": 80}).family in rows_64_128     # no strided data gradient on 512 x 128
    assert L.conv_plan(bm_hint=256, dtype=L.F32, **{**big, "IC": 32 * 8}).family in rows_64_128                # exact f32: 64 / 128-row tiles only
    for bm in (257, 258, -1, -2):
        with pytest.raises(RuntimeError, match="development hook"):
            L.conv_plan(bm_hint=bm, **big)
    # tapf: the 32-bit tap arithmetic, not for strided data gradients; perm: those walk their rows in parity-class order instead
    assert L.conv_plan(bm_hint=256, **big).tapf == 1
    s2 = L.conv_plan(bm_hint=256, mode=1, stride=2, **{**big, "OH": 80, "OW": 80})
    assert (s2.family, s2.tapf, s2.perm) == (L.CONV_256x256, 0, 1)
    w = dict(N=2, IH=40, IW=40, IC=256, OH=40, OW=40, OC=256, KH=3, KW=3, pad=1)
    assert L.wgrad_plan(**w).family == L.WGRAD_128x128                                       # 3200 pixels: too few for the 256 x 256 tiles by choice
    p = L.wgrad_plan(tile_hint=256, split_k=2, **w)
    assert (p.family, p.tile_rows, p.nsplit, p.unit, p.nwg) == (L.WGRAD_256x256, 256, 2, 1, 9 * 2)
    assert L.wgrad_plan(tile_hint=128, **{**w, "N": 16}).family == L.WGRAD_128x128
    assert L.wgrad_plan(tile_hint=256, dtype=L.F32, **w).family == L.WGRAD_128x128           # the 256 x 256 kernel is bf16 only
    assert L.wgrad_plan(tile_hint=256, stride=2, **{**w, "IH": 80, "IW": 80}).unit == 0       # UNIT: same-size stride-1 layers


PAIRS = [
    dict(N=16, H=56, W=56, IC=512, OC=512, k=3, extra={}),                                   # 1: the issue's example
    dict(N=1, H=40, W=40, IC=512, OC=512, k=3, extra={}),                                    # 0: too few pixels for either big tile
    dict(N=2, H=96, W=100, IC=256, OC=512, k=1, extra=dict(in2=L._ANY, IC2=128, epi=1, scale=L._ANY, mask=L._ANY)),   # two-source data gradient
    dict(N=2, H=96, W=96, IC=256, OC=512, k=1, extra=dict(bm_hint=256)),                     # a forced tile height is never paired
    dict(N=2, H=96, W=96, IC=256, OC=512, k=1, extra=dict(dtype=L.F32X3)),                   # bf16 only
    dict(N=2, H=96, W=96, IC=256, OC=512, k=1, extra=dict(out2=L._ANY)),                     # `out` only
]


@pytest.mark.parametrize("case", PAIRS, ids=lambda c: f"N{c['N']}-{c['H']}x{c['W']}-k{c['k']}-{'-'.join(c['extra']) or 'plain'}")
def test_pair_plan_agrees_with_single_plans(case):
    N, H, W, IC, OC, k, extra = (case[key] for key in ("N", "H", "W", "IC", "OC", "k", "extra"))
    geo = dict(N=N, KH=k, KW=k, pad=k // 2)
    dkw = dict(IH=H, IW=W, IC=OC, OH=H, OW=W, OC=IC, mode=1, **geo, **extra)        # data gradient: in = dY [.., OC], out = dX [.., IC]
    wkw = dict(IH=H, IW=W, IC=IC, OH=H, OW=W, OC=OC, **geo)
    fused, dg, wg = L.conv_pair_plan(wkw, **dkw)
    one_dg, one_wg = L.conv_plan(**dkw), L.wgrad_plan(dtype=extra.get("dtype"), **wkw)
    fields = [f for f, _t in L.LaunchPlan._fields_]
    assert [getattr(dg, f) for f in fields] == [getattr(one_dg, f) for f in fields]
    assert [getattr(wg, f) for f in fields] == [getattr(one_wg, f) for f in fields]
    qualifies = (one_dg.family in (L.CONV_224x256, L.CONV_256x256) and one_dg.tapf == 1 and one_dg.perm == 0 and one_wg.family == L.WGRAD_256x256
                 and not extra.get("bm_hint") and extra.get("dtype") is None and "out2" not in extra)
    assert fused == int(qualifies)
    assert fused == {0: 1, 1: 0, 2: 1}.get(PAIRS.index(case), 0)


def test_pair_plan_reports_a_bad_descriptor():
    good = dict(N=16, IH=56, IW=56, IC=512, OH=56, OW=56, OC=512, KH=3, KW=3, pad=1)
    with pytest.raises(RuntimeError, match="conv_igemm: bad mode"):
        L.conv_pair_plan(good, mode=3, **good)
    with pytest.raises(RuntimeError, match="conv_wgrad: bad dw extents"):
        L.conv_pair_plan({**good, "IC_dw": 1024}, mode=1, **good)



def _conv_kernel(plan, kw):
    """the kernel instantiation and workgroup count a conv plan stands for, written as a kernel trace names it"""
    dt, epi = L.BF16 if kw.get("dtype") is None else kw["dtype"], kw.get("epi", 0)
    if plan.family in (L.CONV_64x128, L.CONV_128x128):
        return [f"conv_igemm_kernel<{dt}, {epi}, {plan.tile_rows}>", plan.nwg]
    if plan.family in (L.CONV_224x256, L.CONV_256x256):
        return [f"conv_igemm256_kernel<{epi}, {plan.tile_rows // 32}, {dt}, {plan.tapf}>", plan.nwg]
    assert plan.family == L.CONV_512x128
    return [f"conv_igemm512x128_kernel<{epi}>", plan.nwg]


def _wgrad_kernel(plan, kw):
    if plan.family == L.WGRAD_256x256:
        return [f"conv_wgrad_pipe_kernel<{plan.unit}>", plan.nwg]
    return [f"conv_wgrad_kernel<{L.BF16 if kw.get('dtype') is None else kw['dtype']}, 128, 128, 2, 2>", plan.nwg]


def test_plan_table_of_the_training_step_and_the_inference_geometry():
    """The plan of EVERY conv / wgrad launch of one B = 16, 448^2 + 128^2 bf16 training step and of one 375 x 500 inference image (scales 0.5 / 1 /
    1.5 / 2 x flip) against what those launches ran before the planner became one function.

    tests/golden/conv_plan_table.json was NOT made with this planner.  Each entry's keywords are what the engine passed to L.conv_igemm /
    L.conv_wgrad (Conv.fwd_kw / dgrad_kw / wgrad_kw plus the epilogue operands; a tensor is recorded as "T"), written down in launch order while
    `rocprofv3 --kernel-trace` traced the same process at the parent commit; `expect` is transcribed from that trace: the kernel name encodes
    EPI / NI / DT / TAPF / UNIT (or DT / EPI / BM), the grid size divided by the workgroup size gives nwg, and a pair shows as one
    conv_bwd_pair_kernel dispatch or as two (profiles/r05_planner_dispatch_comparison.txt).  Identical launches are listed once with their count."""
    import json
    import os
    table = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "conv_plan_table.json")))
    assert {e["phase"] for e in table} == {"train", "infer"}
    tensor = lambda kw: {k: (L._ANY if v == "T" else tuple(v) if isinstance(v, list) else v) for k, v in kw.items()}
    for e in table:
        kw = tensor(e["kw"])
        if e["fn"] == "wgrad":
            got = [_wgrad_kernel(L.wgrad_plan(**kw), kw)]
        else:
            pos = dict(out=L._ANY if e["out"] else None, out2=L._ANY if e["out2"] else None)
            if "pair" not in e:
                got = [_conv_kernel(L.conv_plan(**pos, **kw), kw)]
            else:
                wkw = tensor(e["pair"])
                fused, dg, wg = L.conv_pair_plan(wkw, **pos, **kw)
                if fused:
                    got = [[f"conv_bwd_pair_kernel<{kw.get('epi', 0)}, {dg.tile_rows // 32}, {wg.unit}>", ((dg.nwg + 7) & ~7) + wg.nwg]]
                else:
                    got = [_conv_kernel(dg, kw), _wgrad_kernel(wg, wkw)]
        assert got == e["expect"], (e, got)
