"""ctypes binding of libwseg_hip.so (the C ABI of include/wseg_hip.h).

There is deliberately NO fallback: if the library is missing the import raises, and every
wrapper raises RuntimeError(wseg_last_error()) on a non-zero status.
"""
import contextlib
import ctypes as C
import os
import typing

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("WSEG_LIB") or os.path.join(_HERE, "libwseg_hip.so")   # (WSEG_LIB: a probe build kept beside the product, development only)

F32, BF16, F32X3 = 0, 1, 2      # F32X3: f32 tensors, conv / wgrad products as split-bf16 (hi.hi + lo.hi + hi.lo)
PROFILE_WGRAD = None
PROFILE = None        # set to a list by bench.py to collect (start_event, end_event, flops) per conv launch
PROFILE_STRIDE = 1    # event-bracket launch i of step s only when (i + s) % stride == 0: an event pair costs ~10 us of
_profile_idx = 0      # stream time, 81 pairs per step would slow the timed region by ~2 %
_profile_phase = 0


def profile_begin_step(step):
    """bench.py calls this at the start of every timed step: launch indices restart, the sampling phase rotates."""
    global _profile_idx, _profile_phase
    _profile_idx, _profile_phase = 0, step % max(1, PROFILE_STRIDE)


def _profile_sample():
    global _profile_idx
    i = _profile_idx
    _profile_idx += 1
    return (i + _profile_phase) % max(1, PROFILE_STRIDE) == 0, i
TORCH_DTYPE = {F32: torch.float32, BF16: torch.bfloat16, F32X3: torch.float32}


class ConvDesc(C.Structure):
    _fields_ = [("inp", C.c_void_p), ("w", C.c_void_p), ("out", C.c_void_p), ("out2", C.c_void_p),
                ("r_pre", C.c_void_p), ("r_post", C.c_void_p), ("mask", C.c_void_p),
                ("scale", C.c_void_p), ("shift", C.c_void_p), ("drop", C.c_void_p),
                ("N", C.c_int32), ("IH", C.c_int32), ("IW", C.c_int32), ("IC", C.c_int32), ("ld_in", C.c_int32),
                ("OH", C.c_int32), ("OW", C.c_int32), ("OC", C.c_int32), ("ld_out", C.c_int32), ("ld_out2", C.c_int32),
                ("ld_rpre", C.c_int32), ("ld_rpost", C.c_int32), ("ld_mask", C.c_int32),
                ("KH", C.c_int32), ("KW", C.c_int32), ("stride", C.c_int32), ("dil", C.c_int32), ("pad", C.c_int32),
                ("mode", C.c_int32), ("epi", C.c_int32), ("dtype", C.c_int32), ("relu_out2", C.c_int32),
                ("relu_lt", C.c_int32), ("bm_hint", C.c_int32),
                ("IH2", C.c_int32), ("IW2", C.c_int32), ("OH2", C.c_int32), ("OW2", C.c_int32),
                ("in2", C.c_void_p), ("ld_in2", C.c_int32), ("IC2", C.c_int32), ("w_rows", C.c_int32)]


class WgradDesc(C.Structure):
    _fields_ = [("x", C.c_void_p), ("dy", C.c_void_p), ("dw", C.c_void_p),
                ("N", C.c_int32), ("IH", C.c_int32), ("IW", C.c_int32), ("IC", C.c_int32), ("ld_x", C.c_int32),
                ("OH", C.c_int32), ("OW", C.c_int32), ("OC", C.c_int32), ("ld_dy", C.c_int32),
                ("KH", C.c_int32), ("KW", C.c_int32), ("stride", C.c_int32), ("dil", C.c_int32), ("pad", C.c_int32),
                ("dtype", C.c_int32), ("split_k", C.c_int32), ("IC_dw", C.c_int32), ("OC_dw", C.c_int32),
                ("tile_hint", C.c_int32),
                ("IH2", C.c_int32), ("IW2", C.c_int32), ("OH2", C.c_int32), ("OW2", C.c_int32), ("dw_rot", C.c_int32)]


def _load():
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(wseg_amd has no CPU/eager fallback)")
    lib = C.CDLL(LIB_PATH)
    lib.wseg_last_error.restype = C.c_char_p
    lib.wseg_version.restype = C.c_int
    for fn in ("wseg_sizeof_conv_desc", "wseg_sizeof_wgrad_desc", "wseg_select_workspace_bytes", "wseg_plane_stats_workspace_bytes"):
        getattr(lib, fn).restype = C.c_size_t
    if lib.wseg_sizeof_conv_desc() != C.sizeof(ConvDesc) or lib.wseg_sizeof_wgrad_desc() != C.sizeof(WgradDesc):
        raise ImportError(f"{LIB_PATH} was built from another include/wseg_hip.h (descriptor sizes "
                          f"{lib.wseg_sizeof_conv_desc()}/{lib.wseg_sizeof_wgrad_desc()} vs {C.sizeof(ConvDesc)}/{C.sizeof(WgradDesc)}): rebuild it")
    return lib


lib = _load()


def _ptr(t):
    return t.data_ptr() if torch.is_tensor(t) else t       # (None; or an int: the plan queries take stand-in addresses)


def stream_ptr():
    return torch.cuda.current_stream().cuda_stream


def check(status, what):
    if status != 0:
        raise RuntimeError(f"{what} failed ({status}): {lib.wseg_last_error().decode()}")


def _v(x):
    return C.c_void_p(_ptr(x))


def _s():
    return C.c_void_p(stream_ptr())


def _f(x):
    return C.c_float(x)


def _call(name, *args):
    """lib.<name>(*args, current stream), raising on a non-zero status"""
    check(getattr(lib, name)(*args, _s()), name)


def dtype_code(t):
    if t.dtype == torch.float32:
        return F32
    if t.dtype == torch.bfloat16:
        return BF16
    raise TypeError(f"unsupported dtype {t.dtype}")


def _flops_label(kind, *, N, IH, IW, IC, OH, OW, OC, KH, KW, stride=1, dil=1, seg2=None, mode=0, IC2=None, **_):
    """(algorithmic FLOPs, label) of a conv / wgrad launch for the profiler.  Pixels counted: the CONV's output pixels — the launch's
    input side for a data gradient (mode 1); IC2: channels of a second source."""
    oh, ow = (OH, OW) if mode == 0 else (IH, IW)
    pix = N * oh * ow
    if seg2 is not None:
        pix += N * (seg2[2] * seg2[3] if mode == 0 else seg2[0] * seg2[1])
    kin = IC * KH * KW + (IC2 or 0)
    return 2.0 * pix * kin * OC, f"{kind} {IC}{('+%d' % IC2) if IC2 else ''}->{OC} k{KH} s{stride} d{dil} {OH}x{OW}"


@contextlib.contextmanager
def _timed(sink, entry):
    """Bracket a launch with HIP events on its stream and append (ev0, ev1, *entry()) to `sink`; sink None: just run it."""
    if sink is None:
        yield
        return
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ev0.record()
    yield
    ev1.record()
    sink.append((ev0, ev1) + tuple(entry()))


def conv_igemm(inp, w, out=None, out2=None, *, pair_wgrad=None, **kw):
    """One conv launch; `kw`: the keywords of _conv_desc.  w_rows: rows of the weight pack when it is zero-padded beyond OC (wseg_conv_desc.w_rows).
    pair_wgrad: (x, dy, dw, kwargs of conv_wgrad) — a weight gradient launched in the SAME grid as this data gradient (wseg_conv_bwd_pair; the
    library falls back to two launches when the pair does not qualify: conv_pair_plan tells)."""
    d = _conv_desc(inp, w, out, out2, **kw)
    ic2 = (d.IC2 or d.IC) if d.in2 else 0        # two sources: w = [OC][KH*KW*IC + IC2]
    krow, wrows = d.KH * d.KW * d.IC + ic2, max(d.OC, d.w_rows)
    if w.numel() < wrows * krow:                 # (raw pointers beyond this line: a short weight buffer would be read out of bounds)
        raise RuntimeError(f"conv_igemm: weight buffer has {w.numel()} elements, the launch reads {wrows} x {krow}")
    sampled, launch_idx = _profile_sample() if PROFILE is not None else (False, 0)

    def entry():
        kind = "fwd" if d.mode == 0 else ("dgrad+wgrad" if pair_wgrad is not None else "dgrad")
        flops, label = _flops_label(kind, **{**kw, "IC2": ic2})
        wflops = _flops_label("wgrad", **pair_wgrad[3])[0] if pair_wgrad is not None else 0.0
        return flops + wflops, label, launch_idx

    with _timed(PROFILE if sampled else None, entry):        # bench.py: HIP events on the launch stream around this launch
        if pair_wgrad is not None:
            wx, wdy, wdw, wkw = pair_wgrad
            _call("wseg_conv_bwd_pair", C.byref(d), C.byref(_wgrad_desc(wx, wdy, wdw, **wkw)))
        else:
            _call("wseg_conv_igemm", C.byref(d))


def _conv_desc(inp, w, out, out2, *, N, IH, IW, IC, OH, OW, OC, KH, KW, stride=1, dil=1, pad=0,
               mode=0, epi=0, r_pre=None, r_post=None, mask=None, scale=None, shift=None, drop=None,
               ld_in=None, ld_out=None, ld_out2=None, ld_rpre=None, ld_rpost=None, ld_mask=None, relu_out2=1,
               relu_lt=0, bm_hint=0, seg2=None, in2=None, ld_in2=None, IC2=0, dtype=None, w_rows=0):
    d = ConvDesc()
    d.inp, d.w, d.out, d.out2 = _ptr(inp), _ptr(w), _ptr(out), _ptr(out2)
    d.r_pre, d.r_post, d.mask = _ptr(r_pre), _ptr(r_post), _ptr(mask)
    d.scale, d.shift, d.drop = _ptr(scale), _ptr(shift), _ptr(drop)
    d.N, d.IH, d.IW, d.IC, d.ld_in = N, IH, IW, IC, ld_in or IC
    d.OH, d.OW, d.OC, d.ld_out, d.ld_out2 = OH, OW, OC, ld_out or OC, ld_out2 or OC
    d.ld_rpre, d.ld_rpost, d.ld_mask = ld_rpre or OC, ld_rpost or OC, ld_mask or OC
    d.KH, d.KW, d.stride, d.dil, d.pad = KH, KW, stride, dil, pad
    d.mode, d.epi, d.dtype, d.relu_out2, d.relu_lt, d.bm_hint = mode, epi, (dtype_code(inp) if dtype is None else dtype), relu_out2, relu_lt, bm_hint
    if seg2 is not None:                         # (IH2, IW2, OH2, OW2): second row segment, same N
        d.IH2, d.IW2, d.OH2, d.OW2 = seg2
    ic2 = (IC2 or IC) if in2 is not None else 0  # two sources: w = [OC][KH*KW*IC + IC2]
    if in2 is not None:
        d.in2, d.IC2, d.ld_in2 = _ptr(in2), IC2, ld_in2 or ic2
    d.w_rows = w_rows
    return d


def _wgrad_desc(x, dy, dw, *, N, IH, IW, IC, OH, OW, OC, KH, KW, stride=1, dil=1, pad=0,
                ld_x=None, ld_dy=None, split_k=0, IC_dw=None, OC_dw=None, tile_hint=0, seg2=None, dtype=None, dw_rot=0):
    d = WgradDesc()
    d.x, d.dy, d.dw = _ptr(x), _ptr(dy), _ptr(dw)
    d.N, d.IH, d.IW, d.IC, d.ld_x = N, IH, IW, IC, ld_x or IC
    d.OH, d.OW, d.OC, d.ld_dy = OH, OW, OC, ld_dy or OC
    d.KH, d.KW, d.stride, d.dil, d.pad = KH, KW, stride, dil, pad
    d.dtype, d.split_k = (dtype_code(x) if dtype is None else dtype), split_k
    d.IC_dw, d.OC_dw, d.tile_hint = IC_dw or IC, OC_dw or OC, tile_hint
    d.dw_rot = dw_rot
    if seg2 is not None:
        d.IH2, d.IW2, d.OH2, d.OW2 = seg2
    assert not torch.is_tensor(dw) or dw.dtype == torch.float32
    return d


def conv_wgrad(x, dy, dw, **kw):
    """dw += the weight gradient of the conv described by `kw` (the keywords of _wgrad_desc)"""
    d = _wgrad_desc(x, dy, dw, **kw)
    with _timed(PROFILE_WGRAD, lambda: _flops_label("wgrad", **kw)):
        _call("wseg_conv_wgrad", C.byref(d))


# ---- what a launch would run (wseg_conv_plan / wseg_wgrad_plan / wseg_conv_bwd_pair_plan): pure host arithmetic, works without a GPU
CONV_64x128, CONV_128x128, CONV_224x256, CONV_256x256, CONV_512x128, WGRAD_128x128, WGRAD_256x256 = range(1, 8)     # WSEG_CONV_* / WSEG_WGRAD_*
_ANY = 64             # stand-in address of a tensor the caller does not have: the planners only test pointers against NULL


class LaunchPlan(C.Structure):
    _fields_ = [(k, C.c_int32) for k in ("family", "tile_rows", "tile_cols", "nwg", "perm", "tapf", "nsplit", "unit")]

    def __repr__(self):
        return "LaunchPlan(" + ", ".join(f"{k}={getattr(self, k)}" for k, _t in self._fields_) + ")"


def _plan_dtype(t, dtype):
    return dtype if dtype is not None else (dtype_code(t) if torch.is_tensor(t) else BF16)


def conv_plan(inp=_ANY, w=_ANY, out=_ANY, out2=None, *, dtype=None, **kw):
    """The plan of conv_igemm(inp, w, out, out2, **kw) — the same keywords; the tensors may be left out (bf16 unless `dtype` says otherwise)."""
    plan = LaunchPlan()
    check(lib.wseg_conv_plan(C.byref(_conv_desc(inp, w, out, out2, dtype=_plan_dtype(inp, dtype), **kw)), C.byref(plan)), "wseg_conv_plan")
    return plan


def wgrad_plan(x=_ANY, dy=_ANY, dw=_ANY, *, dtype=None, **kw):
    """The plan of conv_wgrad(x, dy, dw, **kw)."""
    plan = LaunchPlan()
    check(lib.wseg_wgrad_plan(C.byref(_wgrad_desc(x, dy, dw, dtype=_plan_dtype(x, dtype), **kw)), C.byref(plan)), "wseg_wgrad_plan")
    return plan


def conv_pair_plan(wgrad_kw, inp=_ANY, w=_ANY, out=_ANY, out2=None, *, dtype=None, **kw):
    """The plan of conv_igemm(inp, w, out, out2, pair_wgrad=(x, dy, dw, wgrad_kw), **kw): (fused, data-gradient plan, weight-gradient plan);
    fused 1 = one grid, 0 = the two ordinary launches.  The weight gradient is planned in the data gradient's dtype unless wgrad_kw carries a
    `dtype` of its own (conv_igemm takes it from the tensor x; the engine's pairs are of one dtype)."""
    dg, wg = LaunchPlan(), LaunchPlan()
    dtype = _plan_dtype(inp, dtype)
    wdtype = dtype if wgrad_kw.get("dtype") is None else wgrad_kw["dtype"]
    fused = lib.wseg_conv_bwd_pair_plan(C.byref(_conv_desc(inp, w, out, out2, dtype=dtype, **kw)),
                                        C.byref(_wgrad_desc(_ANY, _ANY, _ANY, **{**wgrad_kw, "dtype": wdtype})), C.byref(dg), C.byref(wg))
    if fused < 0:                                # (0 and 1 are both answers here)
        check(fused, "wseg_conv_bwd_pair_plan")
    return fused, dg, wg


def pack_weights(master, fwd, tr, OC, T, IC, OCp, ICp, dtype, ic_rot=0):
    _call("wseg_pack_weights", _v(master), _v(fwd), _v(tr), OC, T, IC, OCp, ICp, ic_rot, dtype)


def copy2d_batch(src, dst, table, npieces, total_chunks):
    _call("wseg_copy2d_batch", _v(src), _v(dst), _v(table), npieces, C.c_long(total_chunks))


def pack_transposed_batch(master, out, table, nlayers, total_tiles, dtype):
    _call("wseg_pack_transposed_batch", _v(master), _v(out), _v(table), nlayers, C.c_long(total_tiles), dtype)


def pack_transposed_batch_bf16(mirror, out, table, nlayers, total_tiles):
    _call("wseg_pack_transposed_batch_bf16", _v(mirror), _v(out), _v(table), nlayers, C.c_long(total_tiles))


def dropout_scale(u, out, split_at, p0, p1):
    _call("wseg_dropout_scale", _v(u), _v(out), C.c_long(u.numel()), C.c_long(split_at), _f(p0), _f(p1))


def stem_conv_kc(x, w_kc, scale, shift, raw, act, N, H, W, dtype):
    if w_kc.numel() != 27 * 64 or w_kc.dtype != torch.float32:
        raise RuntimeError("stem_conv_kc: weights must be f32 [27][64]")
    _call("wseg_stem_conv_kc", _v(x), _v(w_kc), _v(scale), _v(shift), _v(raw), _v(act), N, H, W, dtype)


def stem_conv(x, w, scale, shift, raw, act, N, H, W, dtype):
    _call("wseg_stem_conv", _v(x), _v(w), _v(scale), _v(shift), _v(raw), _v(act), N, H, W, dtype)


def head_split(head, ld, c0, cam_low, cmax, N, hw):
    check(lib.wseg_head_split(_v(head), ld, c0, _v(cam_low), _v(cmax), N, hw, dtype_code(head), _s()), "wseg_head_split")


def cam_gate(cam_low, cmax, G, N, hw):
    check(lib.wseg_cam_gate(_v(cam_low), _v(cmax), _v(G), N, hw, _s()), "wseg_cam_gate")


def pcm_xs(x, feat, ld, c_xs, c_end, N, H, W, h, w):
    check(lib.wseg_pcm_xs(_v(x), _v(feat), ld, c_xs, c_end, N, H, W, h, w, dtype_code(feat), _s()), "wseg_pcm_xs")


def head_grad_rows(d_fproj, d_cam_low, head, d_head, ld, N, hw):
    check(lib.wseg_head_grad_rows(_v(d_fproj), _v(d_cam_low), _v(head), _v(d_head), ld, N, hw, dtype_code(head), _s()), "wseg_head_grad_rows")


def resize_planar_fwd(inp, out, planes, ih, iw, oh, ow, align, plane_mul=None, flip_x=False, accumulate=False):
    check(lib.wseg_resize_planar_fwd(_v(inp), _v(out), _v(plane_mul), C.c_long(planes), ih, iw, oh, ow, int(align), int(flip_x), int(accumulate), _s()), "wseg_resize_planar_fwd")


def infer_finish(sum_cam, stats, alpha, norm_cam, pred, npix):
    check(lib.wseg_infer_finish(_v(sum_cam), _v(stats), C.c_float(alpha), _v(norm_cam), _v(pred), npix, _s()), "wseg_infer_finish")


def resize_planar_bwd(d_out, d_in, planes, ih, iw, oh, ow, align, accumulate=False, plane_mul=None, plane_add=None):
    check(lib.wseg_resize_planar_bwd(_v(d_out), _v(d_in), _v(plane_mul), _v(plane_add), C.c_long(planes), ih, iw, oh, ow, int(align), int(accumulate), _s()), "wseg_resize_planar_bwd")


def l2norm_forward(F, ldf, Fh, nrm, rows):
    check(lib.wseg_l2norm_forward(_v(F), ldf, _v(Fh), _v(nrm), C.c_long(rows), dtype_code(F), _s()), "wseg_l2norm_forward")


def l2norm_backward(F, ldf, dFh, nrm, dF, lddf, rows):
    check(lib.wseg_l2norm_backward(_v(F), ldf, _v(dFh), _v(nrm), _v(dF), lddf, C.c_long(rows), dtype_code(F), _s()), "wseg_l2norm_backward")


def pcm_forward(Fh, G, cam_rv, den, N, hw):
    check(lib.wseg_pcm_forward(_v(Fh), _v(G), _v(cam_rv), _v(den), N, hw, _s()), "wseg_pcm_forward")


def pcm_backward(Fh, G, d_cam_rv, cam_rv, den, DN, dFh, N, hw):
    check(lib.wseg_pcm_backward(_v(Fh), _v(G), _v(d_cam_rv), _v(cam_rv), _v(den), _v(DN), _v(dFh), N, hw, _s()), "wseg_pcm_backward")


def sgd_step(params, grads, buf, segs, momentum, grad_scale, first_step, bf16_mirror=None):
    """segs: list of (begin, end, lr, weight_decay) over the flat buffers."""
    n = len(segs)
    LongArr, FloatArr = C.c_long * n, C.c_float * n
    b = LongArr(*[s[0] for s in segs]); e = LongArr(*[s[1] for s in segs])
    lr = FloatArr(*[s[2] for s in segs]); wd = FloatArr(*[s[3] for s in segs])
    check(lib.wseg_sgd_step(_v(params), _v(grads), _v(buf), C.c_long(params.numel()), b, e, lr, wd, n,
                            C.c_float(momentum), C.c_float(grad_scale), int(first_step), _v(bf16_mirror), _s()), "wseg_sgd_step")


# ---------------------------------------------------------------------------------------------- loss kernels
def plane_stats(U, stats, planes, npix):
    ws = torch.empty(int(lib.wseg_plane_stats_workspace_bytes(C.c_long(planes))), device=U.device, dtype=torch.uint8)
    _call("wseg_plane_stats", _v(U), _v(stats), C.c_long(planes), npix, _v(ws))
def cls_loss(stats, label20, loss_out, plane_bias, N, npix, coef): _call("wseg_cls_loss", _v(stats), _v(label20), _v(loss_out), _v(plane_bias), N, npix, _f(coef))
def select_workspace_bytes(rows): return int(lib.wseg_select_workspace_bytes(rows))
def select_kth(vals, rows, n, k, largest, use_abs, relu_vals, res, ws): _call("wseg_select_kth", _v(vals), rows, n, k, int(largest), int(use_abs), int(relu_vals), _v(res), _v(ws))
def loss_finish(acc, er_coef, out8): _call("wseg_loss_finish", _v(acc), _f(er_coef), _v(out8))
def select_finish(res, rows, k, relu_vals, scale, loss_out): _call("wseg_select_finish", _v(res), rows, k, int(relu_vals), _f(scale), _v(loss_out))
def er_ecr_prep(c1, c2, r1, r2, Gc1, Gc2, dlt1, dlt2, er_sum, N, npix, er_coef): _call("wseg_er_ecr_prep", _v(c1), _v(c2), _v(r1), _v(r2), _v(Gc1), _v(Gc2), _v(dlt1), _v(dlt2), _v(er_sum), N, npix, _f(er_coef))
def ecr_backward(dlt, res, Gr, N, per_row, k, coef): _call("wseg_ecr_backward", _v(dlt), _v(res), _v(Gr), N, per_row, k, _f(coef))
def rows_resize_forward(head, ld, F, N, ih, iw, oh, ow): _call("wseg_rows_resize_forward", _v(head), ld, _v(F), N, ih, iw, oh, ow, dtype_code(head))
def head_grad_fused(dF, d_cam_low, head, d_head, ld, N, ih, iw, oh, ow): _call("wseg_head_grad_fused", _v(dF), _v(d_cam_low), _v(head), _v(d_head), ld, N, ih, iw, oh, ow, dtype_code(head))
def pseudo_label(R, label20, bg_thr, y, ncam, N, npix): _call("wseg_pseudo_label", _v(R), _v(label20), _f(bg_thr), _v(y), _v(ncam), N, npix)
def proto_candidates(ncam, F, tie_idx, cand_val, cand_feat, cand_const, N, npix, K): _call("wseg_proto_candidates", _v(ncam), _v(F), _v(tie_idx), _v(cand_val), _v(cand_feat), _v(cand_const), N, npix, K)
def proto_merge(cand_val, cand_feat, cand_const, protos, world, K, rank_stride=0): _call("wseg_proto_merge", _v(cand_val), _v(cand_feat), _v(cand_const), _v(protos), world, K, C.c_long(rank_stride))
def intra_weights(y, S_own, rkey, rand_flag, w, P, ld_s=21): _call("wseg_intra_weights", _v(y), _v(S_own), ld_s, _v(rkey), _v(rand_flag), _v(w), P)
def intra_weights_global(rec, w, P, ranks, own_rank, scale, rank_stride): _call("wseg_intra_weights_global", _v(rec), _v(w), P, ranks, own_rank, _f(scale), C.c_long(rank_stride))


class NceView(C.Structure):
    _fields_ = [("F", C.c_void_p), ("p_own", C.c_void_p), ("p_oth", C.c_void_p), ("y_own", C.c_void_p), ("y_oth", C.c_void_p),
                ("w_intra", C.c_void_p), ("rkey", C.c_void_p), ("rec", C.c_void_p), ("dF", C.c_void_p)]


def _nce_views(views):
    arr = (NceView * len(views))()
    for i, v in enumerate(views):
        for k, _t in NceView._fields_:
            setattr(arr[i], k, _ptr(v.get(k)))
    return arr


def nce_records(views, P, split_bf16=False):
    """views: list of dicts (F, p_own, y_own, rec[, rkey]) — one launch for all of them."""
    _call("wseg_nce_records", _nce_views(views), len(views), P, int(split_bf16))


def nce_fused(views, P, coef_cross, coef_intra, sums):
    """views: list of dicts (F, p_own, p_oth, y_own, y_oth, w_intra, dF) — one launch for all of them."""
    _call("wseg_nce_fused", _nce_views(views), len(views), P, _f(coef_cross), _f(coef_intra), _v(sums))


# ---- SEAM map losses evaluated on the fly from the stride-8 maps (csrc/maps.hip): no [N,21,S,S] tensors
def up_plane_stats(low, stats, planes, h, w, S, label20=None):
    ws = torch.empty(int(lib.wseg_plane_stats_workspace_bytes(C.c_long(planes))), device=low.device, dtype=torch.uint8)
    _call("wseg_up_plane_stats", _v(low), _v(stats), C.c_long(planes), h, w, S, _v(label20), _v(ws))
def up_rvmin_values(low, label20, q, argc, N, h, w, S): _call("wseg_up_rvmin_values", _v(low), _v(label20), _v(q), _v(argc), N, h, w, S)
def up_norm_resize_forward(low, stats, label20, out, N, h, w, S, OS): _call("wseg_up_norm_resize_forward", _v(low), _v(stats), _v(label20), _v(out), N, h, w, S, OS)
def resize_adjoint_ones(wvec, h, S): _call("wseg_resize_adjoint_ones", _v(wvec), h, S)
def up_maps_backward(G, low, stats, label20, plane_bias, wvec_y, wvec_x, q, argc, res, k, coef, d_low, N, h, w, S, OS):
    _call("wseg_up_maps_backward", _v(G), _v(low), _v(stats), _v(label20), _v(plane_bias), _v(wvec_y), _v(wvec_x), _v(q), _v(argc), _v(res),
          k, _f(coef), _v(d_low), N, h, w, S, OS)


def gemm256_probe(A, B, Cout, M, N, K, variant=0):
    if not hasattr(lib, "wseg_gemm256_probe"):
        raise RuntimeError("wseg_gemm256_probe is a development probe: rebuild with `WSEG_PROBES=1 bash wseg_amd/csrc/build.sh`")
    check(lib.wseg_gemm256_probe(_v(A), _v(B), _v(Cout), M, N, K, variant, _s()), "wseg_gemm256_probe")


def debug_stamps(n_wg):
    """probe builds: the in-kernel stamps of the last 256-tile conv launch, [n_wg, 24] uint64: 8 wall-clock stamps (100 MHz) + 2 x 8 slot cycle sums in WSEG_PROBES=2 builds (csrc/conv_igemm.hip)"""
    if not hasattr(lib, "wseg_debug_stamps"):
        raise RuntimeError("wseg_debug_stamps exists in probe builds only: rebuild with `WSEG_PROBES=1 bash wseg_amd/csrc/build.sh`")
    import numpy as np
    torch.cuda.synchronize()
    buf = np.zeros((min(n_wg, 4096), 24), dtype=np.uint64)
    lib.wseg_debug_stamps.argtypes = [C.c_void_p, C.c_size_t]
    check(lib.wseg_debug_stamps(buf.ctypes.data_as(C.c_void_p), C.c_size_t(buf.nbytes)), "wseg_debug_stamps")
    return buf


def debug_set_diag(v):
    """probe builds: timing switches of the 256-tile conv main loop (results wrong by design; csrc/conv_igemm.hip g_wseg_diag)"""
    if not hasattr(lib, "wseg_debug_set_diag"):
        raise RuntimeError("wseg_debug_set_diag exists in probe builds only")
    check(lib.wseg_debug_set_diag(int(v)), "wseg_debug_set_diag")


def to_bf16(inp, out): _call("wseg_to_bf16", _v(inp), _v(out), C.c_long(inp.numel()))
def split_bf16(inp, hi, lo): _call("wseg_split_bf16", _v(inp), _v(hi), _v(lo), C.c_long(inp.numel()))
def pack_x3(src, dst): _call("wseg_pack_x3", _v(src), _v(dst), C.c_long(src.numel()))
def pcm_forward_bf16(Fb, Gb, cam_rv, den, N, hw): _call("wseg_pcm_forward_bf16", _v(Fb), _v(Gb), _v(cam_rv), _v(den), N, hw)
def pcm_backward_bf16(Fb, Gb, Gl, d_cam_rv, cam_rv, den, DN, DNb, DNl, dFh, N, hw): _call("wseg_pcm_backward_bf16", _v(Fb), _v(Gb), _v(Gl), _v(d_cam_rv), _v(cam_rv), _v(den), _v(DN), _v(DNb), _v(DNl), _v(dFh), N, hw)


# ---------------------------------------------------------------------------------------------- AffinityNet inference (csrc/affinity.hip)
RW_MAX_PLANE = 8192          # WSEG_RW_MAX_PLANE


def aff_num_offsets(radius): return int(lib.wseg_aff_num_offsets(radius))
def aff_pairs(feat, ld, C_, aff, N, h, w, radius): _call("wseg_aff_pairs", _v(feat), ld, C_, _v(aff), N, h, w, radius, dtype_code(feat))
def aff_to_dense(aff, dense, h, w, radius): _call("wseg_aff_to_dense", _v(aff), _v(dense), h, w, radius)
def rw_prepare(aff, wgt, rsum, N, h, w, radius, beta): _call("wseg_rw_prepare", _v(aff), _v(wgt), _v(rsum), N, h, w, radius, int(beta))
def random_walk(wgt, rsum, v_in, v_out, N, planes, h, w, radius, logt):
    _call("wseg_random_walk", _v(wgt), _v(rsum), _v(v_in), _v(v_out), N, planes, h, w, radius, int(logt))
def rw_pool(cams, src, bg, pooled, H, W, dh, dw):
    """src: 21 ints, plane c <- cams[src[c]] (-1: zero plane; plane 0 is the bg score)."""
    _call("wseg_rw_pool", _v(cams), (C.c_int * 21)(*[int(s) for s in src]), _f(bg), _v(pooled), H, W, dh, dw)
def rw_finish(cam_rw, pred, planes, dh, dw, H, W): _call("wseg_rw_finish", _v(cam_rw), _v(pred), planes, dh, dw, H, W)


# ---------------------------------------------------------------------------------------------- evaluation counters (csrc/eval.hip)
EVAL_ROWS, EVAL_CLASSES, EVAL_MAX_THR = 22, 20, 64        # WSEG_EVAL_*


def _eval_check(what, counters, cells, n, *u8):
    """(raw pointers beyond the wrappers below) the counter buffer must be int64 of exactly `cells`, the uint8 buffers hold n pixels"""
    if torch.is_tensor(counters) and (counters.dtype != torch.int64 or counters.numel() != cells or not counters.is_contiguous()):
        raise RuntimeError(f"{what}: the counters must be a contiguous int64 tensor of {cells} cells")
    for t_ in u8:
        if torch.is_tensor(t_) and (t_.dtype != torch.uint8 or t_.numel() < n or not t_.is_contiguous()):
            raise RuntimeError(f"{what}: a contiguous uint8 buffer of {n} pixels is expected")


def eval_confusion(pred, gt, n, conf):
    """conf (int64 [22, 22] device, read as u64) += the confusion counts of the uint8 buffers pred / gt [n]."""
    _eval_check("eval_confusion", conf, EVAL_ROWS * EVAL_ROWS, n, pred, gt)
    _call("wseg_eval_confusion", _v(pred), _v(gt), C.c_long(n), _v(conf))
def eval_curve(planes, plane_stride, nplanes, src, gt, n, thr, hist):
    """src: 20 ints, class c <- planes[src[c] * plane_stride:] (-1: absent, score 0); thr: HOST float32 values, non-decreasing;
    hist (int64 [22, 20, len(thr) + 1] device, read as u64) += the (gt row, winner, thresholds below the maximum) counts.
    planes: a float32 tensor, or the device address of plane 0 (views into a larger tensor: the caller vouches for the extent)."""
    _eval_check("eval_curve", hist, EVAL_ROWS * EVAL_CLASSES * (len(thr) + 1), n, gt)
    if torch.is_tensor(planes) and (planes.dtype != torch.float32 or planes.numel() < (nplanes - 1) * plane_stride + n):
        raise RuntimeError(f"eval_curve: planes must be float32 with {nplanes} planes of {n} pixels, {plane_stride} apart")
    _call("wseg_eval_curve", _v(planes), C.c_long(plane_stride), nplanes, (C.c_int * 20)(*[int(s) for s in src]), _v(gt), C.c_long(n),
          (C.c_float * len(thr))(*[float(t) for t in thr]), len(thr), _v(hist))


# ---------------------------------------------------------------------------------------------- AffinityNet training loss (csrc/aff_loss.hip)
lib.wseg_aff_loss_workspace_bytes.restype = C.c_long


def aff_loss_workspace_bytes(N, h, w, radius): return int(lib.wseg_aff_loss_workspace_bytes(N, h, w, radius))
def aff_loss_forward(feat, ld, C_, label, aff, ws, out7, N, h, w, radius, dtype=None):
    _call("wseg_aff_loss_forward", _v(feat), ld, C_, _v(label), _v(aff), _v(ws), _v(out7), N, h, w, radius, dtype_code(feat) if dtype is None else dtype)
def aff_loss_backward(feat, ld, C_, label, aff, out7, gscale, d_feat, ld_d, N, h, w, radius, dtype=None):
    _call("wseg_aff_loss_backward", _v(feat), ld, C_, _v(label), _v(aff), _v(out7), _v(gscale), _v(d_feat), ld_d, N, h, w, radius,
          dtype_code(feat) if dtype is None else dtype)
def aff_pairs_backward(feat, ld, C_, aff, d_aff, d_feat, ld_d, N, h, w, radius, dtype=None):
    """d_feat f32 [N*h*w][ld_d] from d_aff [N, P, n_from] f32 and the aff / feat of aff_pairs (the loss backward's row walk: every row written once)."""
    M, npairs = N * h * w, N * aff_num_offsets(radius) * (h - radius + 1) * (w - 2 * radius + 2)
    for name, t_, need in (("feat", feat, (M - 1) * ld + C_), ("aff", aff, npairs), ("d_aff", d_aff, npairs), ("d_feat", d_feat, (M - 1) * ld_d + C_)):
        if t_.numel() < need:                    # (raw pointers beyond this line)
            raise RuntimeError(f"aff_pairs_backward: {name} has {t_.numel()} elements, the launch touches {need}")
    if aff.dtype != torch.float32 or d_aff.dtype != torch.float32 or d_feat.dtype != torch.float32 or not (aff.is_contiguous() and d_aff.is_contiguous()):
        raise RuntimeError("aff_pairs_backward: aff, d_aff and d_feat must be float32, aff and d_aff contiguous")
    _call("wseg_aff_pairs_backward", _v(feat), ld, C_, _v(aff), _v(d_aff), _v(d_feat), ld_d, N, h, w, radius, dtype_code(feat) if dtype is None else dtype)


# ---------------------------------------------------------------------------------------------- AffinityNet training data (csrc/aff_data.hip, csrc/augment.hip)
class AffLabelDesc(C.Structure):                 # wseg_aff_label_desc
    _fields_ = [("planes", C.c_void_p * 2), ("ids", C.c_void_p * 2), ("np", C.c_int32 * 2), ("H", C.c_int32), ("W", C.c_int32),
                ("plane_stride", C.c_int64), ("flip", C.c_int32), ("cont_top", C.c_int32), ("cont_left", C.c_int32), ("img_top", C.c_int32),
                ("img_left", C.c_int32), ("ch", C.c_int32), ("cw", C.c_int32)]


lib.wseg_sizeof_aff_label_desc.restype = C.c_size_t
if lib.wseg_sizeof_aff_label_desc() != C.sizeof(AffLabelDesc):
    raise ImportError(f"wseg_aff_label_desc: library {lib.wseg_sizeof_aff_label_desc()} bytes, binding {C.sizeof(AffLabelDesc)}: rebuild libwseg_hip.so")


def augment_batch(descs_dev, n, max_pixels, lut, crop, lum_sums):
    """descs_dev: address of n wseg_aug_desc on the device (augment.AugDesc: resize src -> tmp -> img, colour ops on img, finish into out);
    max_pixels: the largest H * rw or rh * rw of the batch; lum_sums: scratch of 4 * n 64-bit words."""
    _call("wseg_augment_batch", _v(descs_dev), n, max_pixels, _v(lut), crop, _v(lum_sums))


def aff_augment_batch(descs_dev, n, max_pixels, lut, crop, lum_sums):
    """descs_dev: address of n wseg_aug_desc on the device (rw = W, rh = H, img = the uploaded image, jittered in place)."""
    _call("wseg_aff_augment_batch", _v(descs_dev), n, max_pixels, _v(lut), crop, _v(lum_sums))


def aff_labels_batch(descs_dev, n, crop, out_u8):
    """descs_dev: address of n wseg_aff_label_desc on the device; out_u8: uint8 [n, crop/8, crop/8]."""
    if out_u8.dtype != torch.uint8 or not out_u8.is_contiguous() or out_u8.numel() != n * (crop // 8) ** 2:       # (raw pointers beyond this line)
        raise RuntimeError(f"aff_labels_batch: out_u8 must be a contiguous uint8 tensor of {n} x {crop // 8} x {crop // 8}")
    _call("wseg_aff_labels_batch", _v(descs_dev), n, crop, _v(out_u8))


# ---------------------------------------------------------------------------------------------- DeepLab-v1 training data (csrc/seg_data.hip)
class SegDataDesc(C.Structure):                  # wseg_seg_data_desc
    _fields_ = [("raw", C.c_void_p), ("lab", C.c_void_p), ("yi", C.c_void_p), ("xi", C.c_void_p), ("lab_out", C.c_void_p),
                ("dh", C.c_int32), ("ds", C.c_int32), ("dv", C.c_int32), ("reserved", C.c_int32)]


lib.wseg_sizeof_seg_data_desc.restype = C.c_size_t
if lib.wseg_sizeof_seg_data_desc() != C.sizeof(SegDataDesc):
    raise ImportError(f"wseg_seg_data_desc: library {lib.wseg_sizeof_seg_data_desc()} bytes, binding {C.sizeof(SegDataDesc)}: rebuild libwseg_hip.so")


def seg_data_batch(aug_host, seg_host, aug_dev, seg_dev, n, crop, lut, hsv_div, stages=7):
    """aug_host / seg_host: ctypes arrays of n wseg_aug_desc / wseg_seg_data_desc (the entry point checks them before any launch and raises
    on a bad one); aug_dev / seg_dev: the addresses of their copies on the device; lut: f32 [3][256]; hsv_div: int32 sdiv[256], hdiv[256];
    stages: 1 hsv | 2 resize | 4 finish."""
    host = [C.c_void_p(C.addressof(a)) if a is not None else C.c_void_p(None) for a in (aug_host, seg_host)]
    _call("wseg_seg_data_batch", *host, _v(aug_dev), _v(seg_dev), n, crop, _v(lut), _v(hsv_div), stages)


# ---------------------------------------------------------------------------------------------- AffinityNet head, training (csrc/aff_head.hip)
def elu_backward_rows(g, ld_g, y, ld_y, gscale, dz, ld_dz, M, C_):
    """dz[m, c] = gscale * g[m, c] * (y[m, c] > 0 ? 1 : y[m, c] + 1) for c < C_ on M pixel rows; y: the saved ELU output; gscale: a one-element
    f32 device tensor or None; g / y / dz: f32 or bf16 tensors, each of its own ld (dz may be g itself)."""
    for name, t_, ld in (("g", g, ld_g), ("y", y, ld_y), ("dz", dz, ld_dz)):
        if t_.numel() < (M - 1) * ld + C_:       # (raw pointers beyond this line)
            raise RuntimeError(f"elu_backward_rows: {name} has {t_.numel()} elements, {M} rows of ld {ld} with {C_} columns need {(M - 1) * ld + C_}")
    _call("wseg_elu_backward_rows", _v(g), ld_g, dtype_code(g), _v(y), ld_y, dtype_code(y), _v(gscale), _v(dz), ld_dz, dtype_code(dz), C.c_long(M), C_)


# ---------------------------------------------------------------------------------------------- dense CRF, exact mean field (csrc/crf.hip)
CRF_PIX_ALIGN, CRF_MAX_LABELS, CRF_MAX_COLUMNS = 128, 32, 64     # WSEG_CRF_*
CRF_BG_CONST, CRF_BG_POWER = 0, 1


def crf_padded_pixels(npix): return int(lib.wseg_crf_padded_pixels(int(npix)))
def crf_columns(S, n_labels): return int(lib.wseg_crf_columns(int(S), int(n_labels)))
def crf_labels(cams, src, n_labels, rule, param, labels, npix):
    """src: n_labels ints, plane c <- cams[src[c]] (-1: zero plane; plane 0 follows the background rule)."""
    _call("wseg_crf_labels", _v(cams), (C.c_int * n_labels)(*[int(s) for s in src]), n_labels, int(rule), _f(param), _v(labels), npix)
def crf_prepare(img, H, W, gauss_sxy, feat, ones, ng): _call("wseg_crf_prepare", _v(img), H, W, _f(gauss_sxy), _v(feat), _v(ones), _v(ng))
def crf_bilateral(feat, Qn, out, npix, ncols, sxy, srgb): _call("wseg_crf_bilateral", _v(feat), _v(Qn), _v(out), npix, ncols, _f(sxy), _f(srgb))
def crf_rsqrt(sums, stride, n, npix): _call("wseg_crf_rsqrt", _v(sums), stride, _v(n), npix)
def crf_gaussian(inp, tmp, out, planes, H, W, sxy): _call("wseg_crf_gaussian", _v(inp), _v(tmp), _v(out), planes, H, W, _f(sxy))
def crf_update(labels, outb, outg, nb, ng, Qn, Qg, Qout, logits, amax, S, n_labels, npix, gt_prob, w_bilateral, w_gaussian):
    _call("wseg_crf_update", _v(labels), _v(outb), _v(outg), _v(nb), _v(ng), _v(Qn), _v(Qg), _v(Qout), _v(logits), _v(amax), S, n_labels, npix,
          _f(gt_prob), _f(w_bilateral), _f(w_gaussian))
def crf_update_prob(prob, outb, outg, nb, ng, Qn, Qg, Qout, logits, amax, n_labels, npix, w_bilateral, w_gaussian):
    """wseg_crf_update for one label set whose unary is -ln(clip(prob, 1e-5, 1)), prob f32 [n_labels][npix]."""
    if prob.dtype != torch.float32 or not prob.is_contiguous() or prob.numel() != n_labels * npix:      # (raw pointers beyond this line)
        raise RuntimeError(f"crf_update_prob: prob must be a contiguous float32 tensor of {n_labels} x {npix}")
    _call("wseg_crf_update_prob", _v(prob), _v(outb), _v(outg), _v(nb), _v(ng), _v(Qn), _v(Qg), _v(Qout), _v(logits), _v(amax), n_labels, npix,
          _f(w_bilateral), _f(w_gaussian))


# ---------------------------------------------------------------------------------------------- DeepLab multi-scale fusion (csrc/seg.hip)
SEG_MAX_PASSES, SEG_MAX_CLASSES = 16, 32         # WSEG_SEG_*


class SegPassDesc(C.Structure):                  # wseg_seg_pass
    _fields_ = [("rows", C.c_void_p), ("ld", C.c_int32), ("dtype", C.c_int32), ("img", C.c_int32), ("fh", C.c_int32), ("fw", C.c_int32),
                ("ih", C.c_int32), ("iw", C.c_int32), ("flip", C.c_int32)]


lib.wseg_sizeof_seg_pass.restype = C.c_size_t
if lib.wseg_sizeof_seg_pass() != C.sizeof(SegPassDesc):
    raise ImportError(f"wseg_seg_pass: library {lib.wseg_sizeof_seg_pass()} bytes, binding {C.sizeof(SegPassDesc)}: rebuild libwseg_hip.so")


class SegPass(typing.NamedTuple):
    """One pass of seg_fuse: the cls_conv pixel rows [images * fh * fw, ld] (f32 or bf16), the image inside that batch, the coarse dims, the
    intermediate dims (the scaled input's size) and whether the pass saw the x-flipped image."""
    rows: torch.Tensor
    ld: int
    img: int
    fh: int
    fw: int
    ih: int
    iw: int
    flip: bool


def seg_fuse(passes, H, W, n_cls, amax, mean_logits=None, prob=None, margin=None):
    """wseg_seg_fuse: the two-stage align_corners resample of every pass, un-flip, mean, softmax and arg-max in one launch; the
    descriptors travel as launch arguments.  amax uint8 [H * W]; mean_logits / prob f32 [n_cls, H * W]; margin f32 [H * W]."""
    if not 1 <= len(passes) <= SEG_MAX_PASSES:
        raise RuntimeError(f"seg_fuse: {len(passes)} passes outside [1, {SEG_MAX_PASSES}]")
    arr = (SegPassDesc * len(passes))()
    nc8 = (n_cls + 7) // 8 * 8
    for i, p in enumerate(passes):               # (raw pointers beyond this loop)
        if p.rows.numel() < (p.img + 1) * p.fh * p.fw * p.ld or p.ld < nc8 or p.img < 0 or not p.rows.is_contiguous() or not p.rows.is_cuda:
            raise RuntimeError(f"seg_fuse: pass {i}: rows of {p.rows.numel()} elements do not hold image {p.img} of {p.fh} x {p.fw} x ld {p.ld} (>= {nc8})")
        arr[i] = SegPassDesc(p.rows.data_ptr(), p.ld, dtype_code(p.rows), p.img, p.fh, p.fw, p.ih, p.iw, int(p.flip))
    for name, t_, n, dt in (("amax", amax, H * W, torch.uint8), ("mean_logits", mean_logits, n_cls * H * W, torch.float32),
                            ("prob", prob, n_cls * H * W, torch.float32), ("margin", margin, H * W, torch.float32)):
        if t_ is not None and (t_.dtype != dt or t_.numel() != n or not t_.is_contiguous() or not t_.is_cuda):
            raise RuntimeError(f"seg_fuse: {name} must be a contiguous {dt} device tensor of {n} elements")
    if amax is None:
        raise RuntimeError("seg_fuse: the arg-max output is required")
    _call("wseg_seg_fuse", arr, len(passes), H, W, n_cls, _v(mean_logits), _v(prob), _v(amax), _v(margin))


# ---------------------------------------------------------------------------------------------- DeepLab training loss (csrc/seg_loss.hip)
lib.wseg_seg_ce_workspace_bytes.restype = C.c_long


def seg_ce_workspace_bytes(N, H, W): return int(lib.wseg_seg_ce_workspace_bytes(N, H, W))
def _seg_ce_extents(what, rows, ld, label, lse, N, fh, fw, H, W, n_cls):
    """the extents the raw pointers of a seg_ce launch must cover (the library checks ld, alignment, n_cls and the sizes themselves)"""
    nc8 = (n_cls + 7) // 8 * 8
    if not rows.is_cuda or not rows.is_contiguous() or rows.numel() < (N * fh * fw - 1) * ld + nc8:
        raise RuntimeError(f"{what}: rows of {rows.numel()} elements do not hold {N} x {fh} x {fw} contiguous device rows of ld {ld} (>= {nc8})")
    if label.dtype != torch.uint8 or not label.is_cuda or not label.is_contiguous() or label.numel() != N * H * W:
        raise RuntimeError(f"{what}: label must be a contiguous uint8 device tensor of {N} x {H} x {W}")
    if lse is not None and (lse.dtype != torch.float32 or not lse.is_cuda or not lse.is_contiguous() or lse.numel() != N * H * W):
        raise RuntimeError(f"{what}: lse must be a contiguous float32 device tensor of {N} x {H} x {W}")
def seg_ce_forward(rows, ld, label, lse, ws, out4, N, fh, fw, H, W, n_cls):
    """wseg_seg_ce_forward: out4 = loss, count, sum of nll, out-of-range labels; lse f32 [N, H, W] or None (a loss-only call)."""
    _seg_ce_extents("seg_ce_forward", rows, ld, label, lse, N, fh, fw, H, W, n_cls)
    need = seg_ce_workspace_bytes(N, H, W)
    if need < 0 or ws.numel() * ws.element_size() < need or not ws.is_cuda or out4.dtype != torch.float32 or out4.numel() < 4 or not out4.is_cuda:
        raise RuntimeError(f"seg_ce_forward: workspace of {need} bytes and a float32 out4 of 4 elements, both on the device ({lib.wseg_last_error().decode()})")
    _call("wseg_seg_ce_forward", _v(rows), ld, dtype_code(rows), _v(label), _v(lse), _v(ws), _v(out4), N, fh, fw, H, W, n_cls)
def seg_ce_backward(rows, ld, label, lse, out4, gscale, d_rows, ld_d, N, fh, fw, H, W, n_cls):
    """wseg_seg_ce_backward: d_rows (f32 or bf16) [N*fh*fw][ld_d] = gscale * d loss / d rows, columns [0, n_cls rounded up to 8) of every row."""
    _seg_ce_extents("seg_ce_backward", rows, ld, label, lse, N, fh, fw, H, W, n_cls)
    nc8 = (n_cls + 7) // 8 * 8
    if lse is None or not d_rows.is_cuda or not d_rows.is_contiguous() or d_rows.numel() < (N * fh * fw - 1) * ld_d + nc8:
        raise RuntimeError(f"seg_ce_backward: lse, and contiguous device d_rows holding {N * fh * fw} rows of ld_d {ld_d} (>= {nc8})")
    _call("wseg_seg_ce_backward", _v(rows), ld, dtype_code(rows), _v(label), _v(lse), _v(out4), _v(gscale), _v(d_rows), ld_d, dtype_code(d_rows),
          N, fh, fw, H, W, n_cls)


# ---------------------------------------------------------------------------------------------- DeepLab head, training (csrc/seg_head.hip)
lib.wseg_bn_stats_workspace_bytes.restype = C.c_long


def bn_stats_workspace_bytes(M, C_): return int(lib.wseg_bn_stats_workspace_bytes(C.c_long(M), C_))
def _seg_head_extents(what, M, C_, rows=(), vecs=(), ws=None):
    """the extents the raw pointers of a seg-head launch must cover: rows (name, tensor, ld) of M rows with C_ columns, f32 vectors (name,
    tensor or None) of C_ elements, the workspace (the library checks dtype codes, ld, alignment and the sizes themselves)"""
    for name, t_, ld in rows:
        if not t_.is_cuda or t_.numel() < (M - 1) * ld + C_:
            raise RuntimeError(f"{what}: {name} ({t_.numel()} elements on {t_.device}) does not hold {M} device rows of ld {ld} with {C_} columns")
    for name, t_ in vecs:
        if t_ is not None and (not t_.is_cuda or t_.dtype != torch.float32 or not t_.is_contiguous() or t_.numel() < C_):
            raise RuntimeError(f"{what}: {name} must be a contiguous float32 device tensor of {C_} elements")
    if ws is not None:
        need = bn_stats_workspace_bytes(M, (C_ + 7) // 8 * 8)
        if need < 0 or not ws.is_cuda or ws.numel() * ws.element_size() < need:
            raise RuntimeError(f"{what}: the workspace must be a device buffer of {need} bytes ({lib.wseg_last_error().decode()})")
def bn_stats(x, ld, M, C_, gamma, beta, eps, momentum, mean, invstd, scale, shift, running_mean, running_var, ws):
    """wseg_bn_stats: batch mean / invstd (and the fold scale / shift, the running update: each may be None) of the C_ columns of M rows."""
    _seg_head_extents("bn_stats", M, C_, [("x", x, ld)], [("gamma", gamma), ("beta", beta), ("mean", mean), ("invstd", invstd), ("scale", scale),
                      ("shift", shift), ("running_mean", running_mean), ("running_var", running_var)], ws)
    _call("wseg_bn_stats", _v(x), ld, dtype_code(x), C.c_long(M), C_, _v(gamma), _v(beta), C.c_double(eps), C.c_double(momentum), _v(mean),
          _v(invstd), _v(scale), _v(shift), _v(running_mean), _v(running_var), _v(ws))
def bn_relu_drop(z, ld_z, scale, shift, y, ld_y, M, C_, p=0.0, key=0):
    """wseg_bn_relu_drop: y = relu(z * scale + shift), times keep / (1 - p) of the counter-hash mask synth.dropout_keep(M, C_, key, p) when p > 0."""
    _seg_head_extents("bn_relu_drop", M, C_, [("z", z, ld_z), ("y", y, ld_y)], [("scale", scale), ("shift", shift)])
    _call("wseg_bn_relu_drop", _v(z), ld_z, dtype_code(z), _v(scale), _v(shift), _v(y), ld_y, dtype_code(y), C.c_long(M), C_, _f(p),
          C.c_uint(int(key) & 0xFFFFFFFF))
def bn_relu_backward(g, ld_g, y, ld_y, z, ld_z, mean, invstd, gamma, s, dz, ld_dz, d_gamma, d_beta, M, C_, ws):
    """wseg_bn_relu_backward: dz = gamma * invstd * (dy - s1/M - xhat * s2/M) with dy = s * g * [y > 0]; d_beta = s1, d_gamma = s2 (or None)."""
    if y.dtype != z.dtype or dz.dtype != z.dtype:
        raise TypeError(f"bn_relu_backward: y ({y.dtype}), z ({z.dtype}) and dz ({dz.dtype}) share one dtype")
    _seg_head_extents("bn_relu_backward", M, C_, [("g", g, ld_g), ("y", y, ld_y), ("z", z, ld_z), ("dz", dz, ld_dz)],
                      [("mean", mean), ("invstd", invstd), ("gamma", gamma), ("d_gamma", d_gamma), ("d_beta", d_beta)], ws)
    _call("wseg_bn_relu_backward", _v(g), ld_g, dtype_code(g), _v(y), ld_y, _v(z), ld_z, dtype_code(z), _v(mean), _v(invstd), _v(gamma), _f(s),
          _v(dz), ld_dz, _v(d_gamma), _v(d_beta), C.c_long(M), C_, _v(ws))
def col_sums(rows, ld, M, C_, out, ws):
    """wseg_col_sums: out[c] = the sum over the M rows of column c < C_ (f32); whole 8-column chunks are read."""
    _seg_head_extents("col_sums", M, (C_ + 7) // 8 * 8, [("rows", rows, ld)], [], ws)
    if not out.is_cuda or out.dtype != torch.float32 or not out.is_contiguous() or out.numel() < C_:
        raise RuntimeError(f"col_sums: out must be a contiguous float32 device tensor of {C_} elements")
    _call("wseg_col_sums", _v(rows), ld, dtype_code(rows), C.c_long(M), C_, _v(out), _v(ws))
