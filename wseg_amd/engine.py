"""Forward/backward orchestration of the ResNet-38d + CAM/PCM head on the HIP kernels.

Host-side plumbing only: allocates torch tensors (device memory), folds the frozen BatchNorms,
keeps the trainable weights in ONE flat f32 buffer (and their gradients in another — a single
RCCL all-reduce / fused SGD target), and issues the C-ABI kernels of libwseg_hip.so in the order
of network/resnet38d.py:160-189 and network/resnet38_contrast.py:31-75.  Activations are NHWC
("pixel rows") in the precision mode's dtype; 21-class maps are planar f32.

The whole network is one torch.autograd.Function: its backward runs the hand-written dgrad /
wgrad / PCM-backward kernels and accumulates straight into the flat gradient buffer.
"""
import threading
import weakref
from typing import NamedTuple

import torch

from . import arch
from . import _lib as L

HEAD_LD = 192          # fused head rows: [f_proj 128 | cam 21 | zero pad 43]  (a 256-wide row for the 256-tile kernels measured slower: profiles/HISTORY.md)
FEAT_LD = 256          # PCM feature rows: [f8_3 64 | f8_4 128 | x_s 3 | zero pad 61]
AFF_FEAT_C = 448       # AffinityNet feature rows [f8_3 64 | f8_4 128 | f8_5 256]: the concat of network/resnet38_aff.py:47 is three column slices
AFF_FEAT_SLICES = {"f8_3": (0, 64), "f8_4": (64, 192), "f8_5": (192, 448)}


DT_OF = {"bf16": L.BF16, "fp32": L.F32, "bf16x3": L.F32X3}   # bf16x3: f32 storage, conv / wgrad products as split-bf16 (3 bf16 MFMAs)


def _cdt(dt):
    """dtype override for the conv / wgrad launches: the split-bf16 mode runs on f32 tensors."""
    return L.F32X3 if dt == L.F32X3 else None


class Conv(NamedTuple):
    """One conv layer over the batched views, described once.  name: the key of its pack in P["w"] / P["wt"] (for a weight gradient: the parameter's
    name); din / dout: [(h, w)] per view of its input / output.  The three methods are the geometry keywords of L.conv_igemm / L.conv_wgrad."""
    name: str
    cin: int
    cout: int
    k: int
    stride: int
    dil: int
    din: list
    dout: list

    def _kw(self, N, ic, oc, di, do):
        seg2 = (di[1][0], di[1][1], do[1][0], do[1][1]) if len(di) == 2 else None        # the second view's row segment
        return dict(N=N, IH=di[0][0], IW=di[0][1], IC=ic, OH=do[0][0], OW=do[0][1], OC=oc, KH=self.k, KW=self.k,
                    stride=self.stride, dil=self.dil, pad=self.dil * (self.k // 2), seg2=seg2)

    def fwd_kw(self, N):
        return self._kw(N, self.cin, self.cout, self.din, self.dout)

    def dgrad_kw(self, N):
        """in = dY over the conv's OUTPUT dims, out = dX over its INPUT dims"""
        return dict(self._kw(N, self.cout, self.cin, self.dout, self.din), mode=1)

    wgrad_kw = fwd_kw                                       # (x over din, dY over dout: the forward geometry)


def block_launch_convs(b, din, dout):
    """The convs of block `b` (an arch.BLOCKS row) as launch descriptors, keyed by short name: branch2a, branch2b1, branch2b2 (bottleneck),
    branch1 (absent in a same-shape ResBlock).  Name, channels, kernel, stride and dilation are arch.block_convs(b)'s; the two convs that
    read the block's input (branch2a, the strided one, and the skip conv branch1) map din -> dout, the others dout -> dout."""
    return {name.split(".conv_")[1]: Conv(name, cin, cout, k, stride, dil, din if name.endswith(("branch2a", "branch1")) else dout, dout)
            for (name, cin, cout, k, stride, dil) in arch.block_convs(b)}


def head_conv(name, cin, cout, dims, k=1, dil=1):            # a head layer: a same-size conv on the stride-8 maps (1x1 but for DeepLab's conv_fov)
    return Conv(name, cin, cout, k, 1, dil, dims, dims)


# ---- what the training-mode head modules (aff_head.py, seg_head.py) share
def device_only(module, t, what):
    if not t.is_cuda:
        raise RuntimeError(f"wseg_amd.{module} runs only on an MI355X (HIP) device; there is no CPU fallback ({what} is on {t.device})")


def head_backward_launchers(eng, P, launches, capture):
    """(wgrad(name, x, dy), dgrad(name, dy, out, **operands)) of a head's backward over its `backward_launches` dict: the weight gradient of a
    trainable conv into its slice of flat_g, the data gradient on the transposed pack P["wt"][name] with the epilogue operands; capture (a dict
    or None) receives the plan of every data-gradient launch under "plans".  The keywords carry an explicit dtype: not _Pass.wgrad / dgrad."""
    def wgrad(name, x, dy):
        if eng.conv_param(name).requires_grad:
            L.conv_wgrad(x, dy, eng.grad_slice(name), **launches["wgrad_" + name])

    def dgrad(name, dy, out, **operands):
        kw = dict(launches["dgrad_" + name], **operands)
        if capture is not None:
            capture.setdefault("plans", {})[name] = L.conv_plan(dy, P["wt"][name], out, None, **kw)
        L.conv_igemm(dy, P["wt"][name], out, None, **kw)
    return wgrad, dgrad


def nchw_to_rows(x, tdt):
    """NCHW -> contiguous pixel rows [N*h*w, C] in tdt (a channels_last tensor of that dtype is taken as it is)"""
    N, C, h, w = x.shape
    r = x.detach().permute(0, 2, 3, 1)
    if r.dtype != tdt:
        r = r.to(tdt)
    return r.contiguous().view(N * h * w, C)


def rows_to_nchw(rows, N, h, w, dtype):
    """pixel rows -> the NCHW view in channels_last strides, in `dtype`"""
    v = rows.view(N, h, w, rows.shape[1]).permute(0, 3, 1, 2)
    return v if v.dtype == dtype else v.to(dtype)


def grad_to_rows(g, tdt):
    """an NCHW gradient -> contiguous, 16-byte aligned pixel rows [N*h*w, C] in float32 or tdt, what a head's backward takes"""
    rows = g.permute(0, 2, 3, 1)
    if rows.dtype not in (torch.float32, tdt):
        rows = rows.float()
    rows = rows.contiguous().view(-1, g.shape[1])
    return rows.clone() if rows.data_ptr() % 16 else rows


class _Pass:
    """What the launches of one pass share: batch size, device, precision mode, packs, and the launch helpers — `conv` of a forward pass; `wgrad`,
    `dgrad`, `block_done` of a backward pass (Engine._begin_backward), with its streams: `main`, and `side`, the PCM branch's until main has waited for it."""

    def __init__(self, eng, N, dev, dt, P):
        self.eng, self.N, self.dev, self.dt, self.P = eng, N, dev, dt, P
        self.main = self.side = None
        self.planes = {}                                     # split-bf16 mode: (hi, lo) bf16 planes of an f32 operand, made once per tensor

    def rows_of(self, dims):
        return sum(self.N * h * w for (h, w) in dims)

    def offs_of(self, dims):
        o, out = 0, []
        for (h, w) in dims:
            out.append(o)
            o += self.N * h * w
        return out

    def E(self, m, c):
        return torch.empty((m, c), device=self.dev, dtype=L.TORCH_DTYPE[self.dt])

    def conv(self, c, inp, out, out2=None, **kw):
        L.conv_igemm(inp, self.P["w"][c.name], out, out2, dtype=_cdt(self.dt), **c.fwd_kw(self.N), **kw)

    def trainable(self, nm):
        return self.eng.conv_param(nm).requires_grad

    def split(self, t_):
        key = (t_.data_ptr(), t_.numel())
        if key not in self.planes:
            hi, lo = torch.empty(t_.shape, device=self.dev, dtype=torch.bfloat16), torch.empty(t_.shape, device=self.dev, dtype=torch.bfloat16)
            L.split_bf16(t_, hi, lo)
            self.planes[key] = (hi, lo, t_)                  # (keeps the source alive: the key is its address)
        return self.planes[key][:2]

    def wgrad(self, c, x, dy, **kw):
        """dW of conv `c` accumulated into its slice of flat_g (nothing when the parameter is frozen)"""
        if not self.trainable(c.name):
            return
        dw = self.eng.grad_slice(c.name)
        args = dict(c.wgrad_kw(self.N), dtype=_cdt(self.dt), **kw)
        if self.dt == L.F32X3 and c.cin >= 256 and c.cout >= 256 and not kw and x.is_contiguous() and dy.is_contiguous() \
                and x.shape[1] == c.cin and dy.shape[1] == c.cout:
            # split-bf16 products on the bf16 pixel-reduction kernel: dW += X_lo^T dY_hi + X_hi^T dY_lo + X_hi^T dY_hi (it accumulates
            # with float atomics anyway) — 3 launches at the bf16 kernel's rate beat one launch of the f32-tile kernel that splits inside
            (xh, xl), (dh, dl) = self.split(x), self.split(dy)
            args["dtype"] = None
            L.conv_wgrad(xl, dh, dw, **args)
            L.conv_wgrad(xh, dl, dw, **args)
            L.conv_wgrad(xh, dh, dw, **args)
        else:
            L.conv_wgrad(x, dy, dw, **args)

    def block_done(self, nm):
        """All weight gradients of block `nm` are enqueued: the data-parallel trainer may start reducing its bucket."""
        if self.eng.block_done_hook is not None:
            if self.side is not None:                        # the last bucket (b7 + heads) holds the PCM branch's f9 / f8_3 / f8_4 gradients
                self.main.wait_stream(self.side)
                self.side = None
            self.eng.block_done_hook(nm)

    def dgrad(self, c, dy, out, pair=None, **kw):
        """dX of conv `c`.  pair = (conv, x, dy): a weight gradient of the same dY, launched in the same grid in bf16 mode
        (wseg_conv_bwd_pair) and on its own behind this launch otherwise."""
        pw = None
        if pair is not None and self.dt == L.BF16 and self.trainable(pair[0].name):
            pc, px, pdy = pair
            pw = (px, pdy, self.eng.grad_slice(pc.name), dict(pc.wgrad_kw(self.N), dtype=_cdt(self.dt)))
        L.conv_igemm(dy, self.P["wt"][c.name], out, None, dtype=_cdt(self.dt), pair_wgrad=pw, **c.dgrad_kw(self.N), **kw)
        if pair is not None and pw is None:
            self.wgrad(*pair)

    def end_backward(self):
        self.planes.clear()
        if self.side is not None:
            self.main.wait_stream(self.side)


class Engine:
    """One per Net INSTANCE (a replica made by nn.parallel.replicate gets its own, see Net._replicate_for_data_parallel).
    Re-entrancy (contrast_infer.py:69-73 calls one module from 8 threads): everything that mutates engine state — the flat
    buffers, the packs, the parameters' `.data` — happens under `self.lock`; a forward pass itself only reads them and
    allocates its own activations."""

    def __init__(self, net, parent=None):
        self._net_ref = weakref.ref(net)    # (no reference cycle; the Net owns the Engine)
        self.prefix = arch.prefix_of(net)   # the frozen blocks, stated by the net's class, and what follows from them; refuses what cannot be served
        self.parent = parent                # replica: the engine of the module it was replicated from
        self.lock = threading.RLock()
        self.delegate = None                # set by ensure_flat on a replica that aliases its parent's flat buffer
        self.flat_w = None
        self.flat_g = None
        self.packs = None
        self.pack_key = None
        self.injected_masks = None
        self._order = None
        self.flat_w_version = 0             # bumped by the fused SGD step (raw kernel writes)
        self.flat_wb = None
        self.flat_wb_version = None
        self.block_done_hook = None         # called with the block name when all of its weight gradients are enqueued
        self.capture_ctx = False            # tests: keep the saved forward context of the last training pass in `last_ctx`
        self.last_ctx = None
        self.last_loss_views = None         # tests: loss_hip.step's per-view intermediates of the last step (capture_ctx)
        self.offsets = None                 # {parameter name: (offset, numel)} in the flat buffers (ensure_flat)
        self.flat_w3 = None                 # bf16x3: split-bf16 pack of flat_w
        self.flat_wt = self.flat_wt3 = None     # transposed (dgrad) packs, flat; their batch tables below
        self._wt_table = self._wt_table64 = None
        self._wt_tiles = self._wt_tiles64 = 0
        self._wt_pending = None             # (dt, mirror) until finish_packs has made the transposed packs
        self._frozen_packs = self._frozen_key = None
        self._seg_fold_key = None           # seg_fold_key of the DeepLab head's eval folds inside _frozen_packs["bn"]
        self.seg_stats_version = 0          # bumped by run_seg_head_train (raw kernel writes of the head BatchNorms' running statistics)
        self._seg_train_bias = None         # run_seg_head_train: cls_conv's bias zero-padded to 24, persistent
        self._head_bufs = None
        self._fused = None                  # _fused_plan
        self._late_ev = None                # event of the late packs until the forward pass has waited for it
        self._mirror_pversions = None
        self._streams = {}                  # role -> side stream (stream())

    @property
    def net(self):
        net = self._net_ref()
        if net is None:
            raise RuntimeError("wseg_amd.Engine outlived its Net")
        return net

    # ------------------------------------------------------------------ parameters
    def conv_param(self, name):
        mod = self.net
        for part in name.split("."):
            mod = getattr(mod, part)
        return mod.weight

    def bn_module(self, name):
        mod = self.net
        for part in name.split("."):
            mod = getattr(mod, part)
        return mod

    def trainable_order(self):
        """Flat-buffer order: the convs of the trainable blocks (b3..b7 behind the reference's prefix), then the net's FLAT_HEAD_ORDER — for
        the contrast net fc_proj, fc8 (adjacent: the fused head GEMM's weight gradient is one [149,4096] block), f8_3, f8_4, f9."""
        if self._order is None:
            self._order = [c[0] for c in self.prefix.convs] + list(self.net.FLAT_HEAD_ORDER)
        return self._order

    def __deepcopy__(self, memo):
        return None                         # a copied Net builds its own engine on first use (Net._engine)

    def __reduce__(self):
        return (type(None), ())             # pickling a whole Net: the engine is derived state

    def ensure_flat(self, device):
        """(Re)build the flat weight / gradient buffers when the parameters moved, and return the engine whose buffers serve this
        module on `device`: itself, or the original's for an aliasing replica.  Serialised: eight inference threads may enter a fresh
        module at once (contrast_infer.py:69-73); callers use the RETURNED engine — `self.delegate` is written exactly once per call,
        under the lock, and never passes through None while another thread may be reading it."""
        with self.lock:
            return self._ensure_flat(device)

    def active(self, device):
        """The engine whose buffers serve this module on `device`: itself, or the original's for an aliasing replica."""
        return self.ensure_flat(device)

    def _ensure_flat(self, device):
        names = self.trainable_order()
        first = self.conv_param(names[0])
        par = self.parent
        if par is not None:
            # a replica on the original's device holds ALIASES of the original's parameters (nn.parallel.replicate hands device 0
            # the source tensors): when those already live in the original engine's flat buffer, its buffers and packs serve
            # this replica as they are; anything else (other device, original not flattened yet) gets buffers of its own below
            with par.lock:
                if (par.flat_w is not None and first.device == par.flat_w.device == device
                        and first.data_ptr() == par.flat_w.data_ptr()):
                    self.delegate = par
                    return par
        if (self.flat_w is not None and self.flat_w.device == first.device
                and first.data_ptr() == self.flat_w.data_ptr() and first.device == device):
            self.delegate = None
            return self
        total = sum(self.conv_param(n).numel() for n in names)
        flat_w = torch.empty(total, device=device, dtype=torch.float32)
        flat_g = torch.zeros(total, device=device, dtype=torch.float32)
        off = 0
        self.offsets = {}
        for n in names:
            p = self.conv_param(n)
            oc, ic, kh, kw = p.shape
            view = flat_w[off:off + p.numel()].view(oc, kh, kw, ic).permute(0, 3, 1, 2)
            view.copy_(p.data.to(device))
            p.data = view                                        # logical [OC,IC,KH,KW], physical [OC][KH][KW][IC]
            p._wseg_flat = (self, off, p.numel())                # lets PolyOptimizer find the flat buffers
            self.offsets[n] = (off, p.numel())
            off += p.numel()
        for n in ("conv1a",) + self.prefix.frozen_convs:
            p = self.conv_param(n)
            p.data = p.data.to(device).contiguous(memory_format=torch.channels_last)
        self.flat_w, self.flat_g = flat_w, flat_g
        self.packs = None
        self.flat_wb_version = None                          # the bf16 mirror (if any) is stale
        self.delegate = None
        return self

    def _mirror_fresh(self, names):
        """False when a parameter was modified through torch (load_state_dict, manual edits) since the mirror was written."""
        return self._mirror_pversions == tuple(self.conv_param(n_)._version for n_ in names)

    def grad_buckets(self, after=None):
        """Contiguous slices of flat_g in the order backward completes them: {block name: (begin, end)} — the slice is
        final once that block's weight gradients are enqueued (flat order = forward order; the heads sit behind b7).
        after: the trigger blocks, last first; default b7, b5, b4 as far as they lie behind the first trainable block, then that block."""
        firsts = {b[0]: min(self.offsets[c[0]][0] for c in arch.block_convs(b)) for b in self.prefix.trainable}
        if after is None:
            after = tuple(nm for nm in ("b7", "b5", "b4") if nm in firsts and nm != self.prefix.first) + (self.prefix.first,)
        out, end = {}, self.flat_g.numel()
        for name in after:
            out[name] = (firsts[name], end)
            end = firsts[name]
        assert end == 0, "the last bucket must reach the start of the flat buffer"
        return out

    def grad_slice(self, name, numel=None):
        """The flat-gradient elements of parameter `name` (numel: a longer run that starts there)"""
        off, n = self.offsets[name]
        return self.flat_g[off:off + (numel or n)]

    def grad_view(self, name):
        oc, ic, kh, kw = self.conv_param(name).shape
        return self.grad_slice(name).view(oc, kh, kw, ic).permute(0, 3, 1, 2)

    def stream(self, role, device):
        """The side stream of `role` on `device`, created on first use: HIP maps streams onto four hardware queues in creation order, and
        that layout moves the step time, so nothing creates one ahead of its first use."""
        st = self._streams.get(role)
        if st is None or st.device != device:
            st = self._streams[role] = torch.cuda.Stream(device)
        return st

    def _flat_like(self, buf, dtype, device):
        """`buf` when it is a flat_w-sized buffer of this dtype on this device, else a new (uninitialised) one"""
        if buf is not None and buf.dtype == dtype and buf.device == device and buf.numel() == self.flat_w.numel():
            return buf
        return torch.empty(self.flat_w.numel(), device=device, dtype=dtype)

    def attach_grads(self):
        """Make every trainable p.grad a view of flat_g (zeroing it if the caller dropped the grads,
        e.g. optimizer.zero_grad(set_to_none=True))."""
        names = self.trainable_order()
        p0 = self.conv_param(names[0])
        if p0.grad is not None and p0.grad.data_ptr() == self.flat_g.data_ptr():
            return
        self.flat_g.zero_()
        for n in names:
            p = self.conv_param(n)
            if p.requires_grad:
                p.grad = self.grad_view(n)

    # ------------------------------------------------------------------ packs
    def _bn_fold(self, name, device):
        bn = self.bn_module(name)
        scale = (bn.weight.detach().float() / torch.sqrt(bn.running_var.float() + arch.BN_EPS)).to(device)
        shift = (bn.bias.detach().float() - bn.running_mean.float() * scale).to(device)
        return scale.contiguous(), shift.contiguous()

    @staticmethod
    def _x3(w32):
        """Split-bf16 pack of an f32 weight pack [rows][K] (K % 32 == 0): per 32 K-elements [32 hi | 32 lo] bf16 in the same bytes
        (kept in a float32-typed tensor of the same shape: only the conv kernels of dtype F32X3 read it)."""
        out = torch.empty_like(w32)
        L.pack_x3(w32.contiguous(), out)
        return out

    def frozen_key(self, device, dt):
        """Identity of everything the frozen prefix (conv1a, b2*, every folded BatchNorm) is computed from: precision, device, the versions of
        all buffers / BN parameters / frozen conv weights.  The frozen packs are rebuilt when it changes, and a lookahead prefix computed under
        another key is dropped (Trainer.step)."""
        net = self.net
        # (the DeepLab head's folds — bn_fov, bn_fov2, cls_conv's bias — have a key of their own, seg_fold_key: a training step moves them)
        return (dt, str(device)) + tuple(b._version for n_, b in net.named_buffers() if not n_.startswith("bn_fov")) + \
            tuple(p._version for n_, p in net.named_parameters() if ".bn" in n_ or n_.startswith("bn7")) + \
            tuple((self.conv_param(n_)._version, self.conv_param(n_).data_ptr()) for n_ in self.prefix.frozen_convs) + \
            (net.conv1a.weight._version, net.conv1a.weight.data_ptr())

    def seg_fold_key(self, device):
        """Identity of what the DeepLab head's eval folds are computed from: the two head BatchNorms' parameters and statistics, cls_conv's bias, and
        seg_stats_version — run_seg_head_train's kernels write the running statistics through raw pointers, which advances no tensor version.
        Apart from frozen_key: a training step moves these three small folds, not the backbone's BN folds and b2 packs."""
        net = self.net
        mods = [self.bn_module(bname) for bname, _c in arch.SEG_HEAD_BNS.values()]
        return (str(device), self.seg_stats_version, net.cls_conv.bias._version, net.cls_conv.bias.data_ptr()) + \
            tuple(t_._version for m in mods for t_ in (m.weight, m.bias, m.running_mean, m.running_var))

    def ensure_packs(self, device, dt, defer_wt=False, late_stream=None):
        with self.lock:
            return self._ensure_packs(device, dt, defer_wt, late_stream)

    def _ensure_packs(self, device, dt, defer_wt=False, late_stream=None):
        """Packed (cast / transposed) weights + folded BatchNorms.  Frozen pieces (every BN, conv1a, b2*) are
        cached on their own key so a training step only re-packs the 40 trainable tensors.
        defer_wt: the transposed (dgrad) packs are only needed by the backward pass — the fused training step lets
        `finish_packs()` make them on a side stream during the loss phase, when the chip is mostly idle.
        late_stream: the packs the forward pass needs only from b5 on (the K-concatenated skip packs, the head, f9: ~10 small launches that would
        otherwise sit in front of every step) are made on that stream; the forward pass waits for them where it first uses one (`_join_late_packs`)."""
        net = self.net
        tdt = L.TORCH_DTYPE[dt]
        fkey = self.frozen_key(device, dt)
        if self._frozen_packs is None or self._frozen_key != fkey:
            F_ = {"w": {}, "bn": {}}
            for i, b in enumerate(arch.BLOCKS):
                for (bname, c) in arch.block_bns(b):
                    F_["bn"][bname] = self._bn_fold(bname, device)
                if i < self.prefix.n:
                    for (cname, ci, co, k, s, d) in arch.block_convs(b):
                        wf = torch.empty(co, k * k, ci, device=device, dtype=tdt)
                        L.pack_weights(self.conv_param(cname).detach(), wf, None, co, k * k, ci, co, ci, L.F32 if dt == L.F32X3 else dt)
                        F_["w"][cname] = self._x3(wf) if dt == L.F32X3 else wf
            F_["bn"]["bn7"] = self._bn_fold("bn7", device)
            F_["w"]["conv1a_kc"] = net.conv1a.weight.detach().to(device).float().permute(2, 3, 1, 0).reshape(27, 64).contiguous()   # [k = (ky*3+kx)*3+ic][oc] for the packed-FMA stem
            self._frozen_packs, self._frozen_key = F_, fkey
            self._seg_fold_key = None
            self.packs = None
        if net.HEAD_KIND == "seg":
            # DeepLab head (deeplabv1.py:42-49), eval mode: the two head BatchNorms folded like the backbone's; cls_conv's bias as the `shift` of its
            # launch, zero-padded to the pack's rows.  Keyed apart from the frozen packs (seg_fold_key), entered into their "bn" dict in place.
            skey = self.seg_fold_key(device)
            if self._seg_fold_key != skey:
                bnf = self._frozen_packs["bn"]
                for bname, _c in arch.SEG_HEAD_BNS.values():
                    bnf[bname] = self._bn_fold(bname, device)
                bias = torch.zeros(arch.SEG_CLS_ROWS, device=device, dtype=torch.float32)
                bias[:arch.NUM_CLASSES] = net.cls_conv.bias.detach().float().to(device)
                bnf["cls_conv"] = (None, bias)
                self._seg_fold_key = skey
        names = self.trainable_order()
        key = (dt, str(device), self.flat_w_version) + tuple(self.conv_param(n_)._version for n_ in names)
        if self.packs is not None and key == self.pack_key:
            return self.packs
        P = {"w": dict(self._frozen_packs["w"]), "wt": {}, "bn": self._frozen_packs["bn"]}
        trunk_convs, no_dgrad = self.prefix.convs, self.prefix.no_dgrad
        # forward packs [OC][T][IC] have exactly the layout of the flat master buffer: in f32 mode they ARE views of
        # it, in bf16 mode they are views of ONE cast copy (a single launch instead of one per layer)
        if dt == L.BF16:
            wb = self._flat_like(self.flat_wb, torch.bfloat16, device)
            if wb is not self.flat_wb:
                self.flat_wb, self.flat_wb_version = wb, None
            if self.flat_wb_version != self.flat_w_version or not self._mirror_fresh(names):
                L.to_bf16(self.flat_w, self.flat_wb)             # (normally the fused SGD step has already written it)
                self.flat_wb_version = self.flat_w_version
            self._mirror_pversions = tuple(self.conv_param(n_)._version for n_ in names)
            mirror = self.flat_wb
        elif dt == L.F32X3:
            self.flat_w3 = self._flat_like(self.flat_w3, torch.float32, device)
            L.pack_x3(self.flat_w, self.flat_w3)             # (every trainable tensor's rows are whole 32-element groups, f9 aside: it has its own pack)
            mirror = self.flat_w3
        else:
            mirror = self.flat_w
        # transposed (dgrad) packs [IC][T][OC]: ONE flat buffer, ONE launch over all layers (same offsets as flat_w)
        wt = self._flat_like(self.flat_wt, tdt, device)
        if wt is not self.flat_wt:
            self.flat_wt = wt
            rows, tiles = [], 0
            for (cname, ci, co, k, s, d) in trunk_convs:
                if cname in no_dgrad:
                    continue
                off, n = self.offsets[cname]
                rows.append([tiles, off, off, co, k * k, ci])
                tiles += ((co + 31) // 32) * ((ci + 31) // 32) * k * k
            self._wt_table = torch.tensor(rows, dtype=torch.int64, device=device)
            self._wt_tiles = tiles
            rows64, t64 = [], 0                              # the bf16 -> bf16 variant works on 64x64 tiles
            for (_t, off_i, off_o, co, T_, ci) in rows:
                rows64.append([t64, off_i, off_o, co, T_, ci])
                t64 += ((co + 63) // 64) * ((ci + 63) // 64) * T_
            self._wt_table64 = torch.tensor(rows64, dtype=torch.int64, device=device)
            self._wt_tiles64 = t64
        self._wt_pending = (dt, mirror)
        if dt == L.F32X3:
            self.flat_wt3 = self._flat_like(self.flat_wt3, torch.float32, device)
        for (cname, ci, co, k, s, d) in trunk_convs:
            T = k * k
            off, n = self.offsets[cname]
            P["w"][cname] = mirror[off:off + n].view(co, T, ci)
            if cname not in no_dgrad:
                P["wt"][cname] = (self.flat_wt3 if dt == L.F32X3 else self.flat_wt)[off:off + n].view(ci, T, co)

        def late():
            # bf16 mode: a block's skip conv and its last conv as ONE two-source product (K-concatenation): rows [W_a[oc] | W_b[oc]] — the skip output is
            # then neither written nor re-read (444 MB each way for b7).  b6 / b7: [W_branch1 | W_branch2b2]; b5 (the residual-block form, 3x3 last conv +
            # 1x1 skip conv at stride 1): [W_branch2b1 (9 taps) | W_branch1].  All pieces are copied from the bf16 mirror in ONE launch into buffers
            # that persist across steps (`_fused_plan`).
            if dt == L.BF16:
                plan = self._fused_plan(device)
                for nm, buf in plan["fwd_bufs"].items():
                    P["w"][nm + ".skip_fused"] = buf
                L.copy2d_batch(mirror, plan["fwd_flat"], plan["fwd_table"], plan["fwd_table"].shape[0], plan["fwd_chunks"])
            if net.HEAD_KIND == "aff":
                # AffinityNet head (resnet38_aff.py:13-17): four plain 1x1 packs, views of the mirror like the backbone's (every row is whole
                # 32-element groups, so the split-bf16 mirror holds them too)
                for nm, (co, ci) in net.HEAD_CONVS.items():
                    off, n = self.offsets[nm]
                    P["w"][nm] = mirror[off:off + n].view(co, 1, ci)
                return
            if net.HEAD_KIND == "seg":
                # DeepLab head: conv_fov [512][9][4096] and conv_fov2 as views of the mirror; cls_conv's 21 rows copied into a pack zero-padded to
                # 24 (every row is whole 32-element groups: the split-bf16 mirror's rows are copied as they are, and a zero row splits into zeros)
                for nm, (co, ci, k) in net.HEAD_CONVS.items():
                    off, n = self.offsets[nm]
                    if co % 8 == 0:
                        P["w"][nm] = mirror[off:off + n].view(co, k * k, ci)
                        continue
                    hb = self._head_bufs
                    if hb is None or hb[0] != (dt, str(device)):
                        hb = self._head_bufs = ((dt, str(device)), torch.zeros(arch.SEG_CLS_ROWS, k * k, ci, device=device, dtype=mirror.dtype))
                    hb[1].view(-1)[:n].copy_(mirror[off:off + n])
                    P["w"][nm] = hb[1]
                return
            # fused head: rows [fc_proj | fc8 | 0]; its transposed pack is made from the two f32 masters directly
            hb = self._head_bufs                                 # persistent: the zero padding (rows / columns 149..191) is written once
            if hb is None or hb[0] != (dt, str(device)):
                # (the forward pack holds 256 rows — 107 of them zero: the head GEMM then runs on the 256-tile kernel, which reads whole 256-row weight
                #  tiles and masks the columns >= HEAD_LD; conv_igemm w_rows)
                hb = self._head_bufs = ((dt, str(device)), torch.zeros(256, 1, 4096, device=device, dtype=tdt),
                                        torch.zeros(4096, 1, HEAD_LD, device=device, dtype=tdt),
                                        torch.empty(192, 1, FEAT_LD, device=device, dtype=tdt), torch.empty(FEAT_LD, 1, 192, device=device, dtype=tdt))
            wh, wht = hb[1], hb[2]
            pdt = L.F32 if dt == L.F32X3 else dt                  # (split-bf16: f32 packs first, split below)
            L.pack_weights(net.fc_proj.weight.detach(), wh, None, 128, 1, 4096, 128, 4096, pdt)
            L.pack_weights(net.fc8.weight.detach(), wh[128:], None, 21, 1, 4096, 21, 4096, pdt)
            off, _ = self.offsets["fc_proj"]                     # fc_proj and fc8 are adjacent in flat_w: one [149,4096] master
            L.pack_weights(self.flat_w[off:off + 149 * 4096], None, wht, 149, 1, 4096, HEAD_LD, 4096, pdt)
            if dt == L.F32X3:
                wh, wht = self._x3(wh), self._x3(wht)
            P["w"]["head"], P["wt"]["head"] = wh, wht
            for nm, (co, ci) in (("f8_3", (64, 512)), ("f8_4", (128, 1024))):
                off, n = self.offsets[nm]
                P["w"][nm] = mirror[off:off + n].view(co, 1, ci)
            # f9: input columns re-ordered to the internal feature layout [f8_3 | f8_4 | x_s | pad] = the master's columns rotated by 3
            off9, n9 = self.offsets["f9"]
            wf, wt = hb[3], hb[4]
            L.pack_weights(self.flat_w[off9:off9 + n9], wf, wt, 192, 1, 195, 192, FEAT_LD, pdt, ic_rot=3)
            if dt == L.F32X3:
                wf, wt = self._x3(wf), self._x3(wt)
            P["w"]["f9"], P["wt"]["f9"] = wf, wt

        # (the names exist at once — the forward pass tests `in P["w"]` — their contents when `_late_ev` has been waited for)
        self._late_ev = None
        if late_stream is not None:
            cur = torch.cuda.current_stream(device)
            late_stream.wait_stream(cur)
            with torch.cuda.stream(late_stream):
                late()
            self._late_ev = late_stream.record_event()
        else:
            late()
        self.packs, self.pack_key = P, key
        if not defer_wt:
            self.finish_packs()
        return P

    def _join_late_packs(self, device):
        if self._late_ev is not None:
            torch.cuda.current_stream(device).wait_event(self._late_ev)
            self._late_ev = None

    def finish_packs(self):
        """The transposed (dgrad) packs [IC][T][OC] of the current weights: ONE launch over all layers into the flat buffer the
        `P["wt"]` views point into, plus the K-concatenated backward packs of the two-source launches.  Runs on the CURRENT
        stream (the fused step calls it on a side stream and joins before the backward pass); no-op when already done."""
        if self._wt_pending is None:
            return
        (dt, mirror), self._wt_pending = self._wt_pending, None
        P = self.packs
        if dt == L.BF16:                                     # from the bf16 mirror (written by the fused SGD): a third of the traffic
            L.pack_transposed_batch_bf16(mirror, self.flat_wt, self._wt_table64, self._wt_table64.shape[0], self._wt_tiles64)
        else:
            L.pack_transposed_batch(self.flat_w, self.flat_wt, self._wt_table, self._wt_table.shape[0], self._wt_tiles, L.F32 if dt == L.F32X3 else dt)
            if dt == L.F32X3:
                L.pack_x3(self.flat_wt, self.flat_wt3)
        if dt == L.BF16 and any(k.endswith(".skip_fused") for k in P["w"]):
            # the K-concatenated backward packs of the two-source launches, one launch from the transposed packs just made.  b5 (res):
            # d_t = dgrad_3x3(du; W_2a) + D . W_branch1 — nine taps of du, then one K segment of D; b6 / b7 (bot): d_t = D . W_branch1 + du1 . W_branch2a
            plan = self._fused_plan(self.flat_wt.device)
            for nm, buf in plan["bwd_bufs"].items():
                P["wt"][nm + ".skip_fused"] = buf
            L.copy2d_batch(self.flat_wt, plan["bwd_flat"], plan["bwd_table"], plan["bwd_table"].shape[0], plan["bwd_chunks"])

    def _fused_blocks(self):
        """[(name, kind, cin, mid, cout)] of the blocks whose skip conv and last conv run as one two-source launch (bf16 mode)"""
        out = []
        for b in self.prefix.trainable:
            nm, kind, cin_, mid_, cout_, stride = b[0], b[1], b[2], b[3], b[4], b[5]
            if stride != 1 or cout_ % 256:
                continue
            if kind == "res" and not arch.block_same_shape(b) and cin_ % 256 == 0:
                out.append((nm, kind, cin_, mid_, cout_))
            elif kind != "res" and cin_ == cout_ // 2:
                out.append((nm, kind, cin_, mid_, cout_))
        return out

    def _fused_plan(self, device):
        """Persistent K-concatenated pack buffers + the piece tables of wseg_copy2d_batch (16-byte = 8-element units), built once per device."""
        plan = self._fused
        if plan is not None and plan["device"] == device:
            return plan

        def build(pieces_of):
            rows_tab, bufs, sizes, chunk0, base = [], {}, [], 0, 0
            for (nm, kind, cin_, mid_, cout_) in self._fused_blocks():
                nrows, width, pieces = pieces_of(nm, kind, cin_, mid_, cout_)       # pieces: (param name, cols, column offset)
                for (pname, cols, coff) in pieces:
                    off, n = self.offsets[pname]
                    assert n == nrows * cols and off % 8 == 0 and cols % 8 == 0 and coff % 8 == 0 and width % 8 == 0 and base % 8 == 0
                    rows_tab.append([chunk0, off // 8, (base + coff) // 8, nrows, cols // 8, cols // 8, width // 8])
                    chunk0 += nrows * (cols // 8)
                sizes.append((nm, base, nrows, width))
                base += nrows * width
            flat = torch.empty(base, device=device, dtype=torch.bfloat16)
            for nm, b0, nrows, width in sizes:
                bufs[nm] = flat[b0:b0 + nrows * width].view(nrows, width)
            return flat, bufs, torch.tensor(rows_tab, dtype=torch.int64, device=device), chunk0

        def fwd_pieces(nm, kind, cin_, mid_, cout_):
            if kind == "res":
                return cout_, 9 * mid_ + cin_, [(nm + ".conv_branch2b1", 9 * mid_, 0), (nm + ".conv_branch1", cin_, 9 * mid_)]
            return cout_, cin_ + cout_ // 2, [(nm + ".conv_branch1", cin_, 0), (nm + ".conv_branch2b2", cout_ // 2, cin_)]

        def bwd_pieces(nm, kind, cin_, mid_, cout_):          # transposed packs [cin][T][cout']: rows = cin
            if kind == "res":
                return cin_, 9 * mid_ + cout_, [(nm + ".conv_branch2a", 9 * mid_, 0), (nm + ".conv_branch1", cout_, 9 * mid_)]
            return cin_, cout_ + cout_ // 4, [(nm + ".conv_branch1", cout_, 0), (nm + ".conv_branch2a", cout_ // 4, cout_)]

        ff, fb, ft, fc = build(fwd_pieces)
        bf, bb, bt, bc = build(bwd_pieces)
        self._fused = dict(device=device, fwd_flat=ff, fwd_bufs=fb, fwd_table=ft, fwd_chunks=fc, bwd_flat=bf, bwd_bufs=bb, bwd_table=bt, bwd_chunks=bc)
        return self._fused

    # ------------------------------------------------------------------ dropout
    MASK_SPECS = (("b6.dropout_2b1", 512, 0.3), ("b6.dropout_2b2", 1024, 0.3),
                  ("b7.dropout_2b1", 1024, 0.5), ("b7.dropout_2b2", 2048, 0.5), ("dropout7", 4096, 0.5))

    def _masks(self, n, views, device, specs=None):
        """Dropout2d scales [views*n, C] per dropout site (rows of view 1, then view 2): injected (parity tests) or drawn
        on the device — one uniform draw + one kernel for all five sites (specs: a prefix of MASK_SPECS; the AffinityNet has no dropout7)."""
        specs = specs or self.MASK_SPECS
        net = self.net
        if not net.training:
            return None
        if self.injected_masks:
            per_view = []
            for _ in range(views):
                m = self.injected_masks.pop(0)
                per_view.append({k: v.to(device=device, dtype=torch.float32) for k, v in m.items()})
            return {k: torch.cat([m[k] for m in per_view], dim=0).contiguous() for k in per_view[0]}
        rows = views * n
        total = sum(c for _, c, _ in specs)
        u = torch.rand(rows * total, device=device)
        flat = torch.empty_like(u)
        L.dropout_scale(u, flat, rows * (512 + 1024), 0.3, 0.5)          # the two b6 sites (p = 0.3) come first
        out, off = {}, 0
        for key, c, _p in specs:
            out[key] = flat[off:off + rows * c].view(rows, c)
            off += rows * c
        return out

    # ------------------------------------------------------------------ forward
    def forward(self, x, lowres=False):
        if not x.is_cuda:
            raise RuntimeError("wseg_amd.Net runs only on an MI355X (HIP) device; there is no CPU fallback")
        x = x.contiguous().float()
        act = self.ensure_flat(x.device)
        if act is not self:                                   # replica whose parameters alias the original's flat buffer
            return act.forward(x, lowres)
        need_grad = torch.is_grad_enabled() and any(p.requires_grad for p in self.net.parameters())
        if need_grad:
            anchor = self.flat_w.new_zeros((), requires_grad=True)
            return _NetFunction.apply(x, anchor, self, lowres)
        outs, _ = self.run_forward([x], save=False, lowres=lowres)
        return outs[0]

    def _run_blocks(self, xs, state, first, last, save, S, final_t=None):
        """Blocks arch.BLOCKS[first:last] over the batched views.  state: the dict an earlier call returned; None: conv1a first."""
        V, dev, N = len(xs), xs[0].device, xs[0].shape[0]
        dt = DT_OF[self.net.precision]
        P = self.ensure_packs(dev, dt)
        masks = S["masks"] if S is not None else None
        ps = _Pass(self, N, dev, dt, P)
        E, conv, rows_of = ps.E, ps.conv, ps.rows_of

        def next_bn(i):
            if i + 1 < len(arch.BLOCKS):
                return P["bn"][arch.BLOCKS[i + 1][0] + ".bn_branch2a"], None
            return P["bn"]["bn7"], (masks["dropout7"] if masks else None)

        sdims = {}
        conv4 = conv5 = None
        if state is None:
            dims = [(x.shape[2], x.shape[3]) for x in xs]
            sc, sh = P["bn"]["b2.bn_branch2a"]
            t = E(rows_of(dims), 64)
            for x, off, (H, W) in zip(xs, ps.offs_of(dims), dims):
                L.stem_conv_kc(x, P["w"]["conv1a_kc"], sc, sh, None, t[off:], N, H, W, L.F32 if dt == L.F32X3 else dt)
            xraw = None
        else:
            t, xraw, dims = state["t"], state["xraw"], state["dims"]
        for i in range(first, last):
            b = arch.BLOCKS[i]
            name, kind, cin, mid, cout, stride, fd, d, p = b
            same = arch.block_same_shape(b)
            if (name + ".skip_fused") in P["w"]:
                self._join_late_packs(dev)
            (nsc, nsh), ndrop = next_bn(i)
            nxt_same = i + 1 < len(arch.BLOCKS) and arch.block_same_shape(arch.BLOCKS[i + 1])
            odims = arch.block_out_dims(b, dims)
            Mo = rows_of(odims)
            cv = block_launch_convs(b, dims, odims)
            if kind == "res":
                s1, sh1 = P["bn"][name + ".bn_branch2b1"]
                v = E(Mo, mid)
                conv(cv["branch2a"], t, None, v, scale=s1, shift=sh1)
                xn = E(Mo, cout) if nxt_same else None
                tn = final_t if (final_t is not None and i == last - 1) else E(Mo, cout)
                assert tn.shape == (Mo, cout) and tn.dtype == L.TORCH_DTYPE[dt]
                if (name + ".skip_fused") in P["w"]:            # branch2b1 + the 1x1 skip conv branch1 as one two-source launch: nine taps of v, then one K segment of t
                    conv(cv["branch2b1"]._replace(name=name + ".skip_fused"), v, xn, tn, in2=t, IC2=cin, scale=nsc, shift=nsh, drop=ndrop)
                else:
                    if same:
                        rpost = xraw
                    else:
                        rpost = E(Mo, cout)
                        conv(cv["branch1"], t, rpost)
                    conv(cv["branch2b1"], v, xn, tn, r_post=rpost, scale=nsc, shift=nsh, drop=ndrop)
                if save:
                    S[name] = dict(t=t, v=v)
            else:
                c4, c2 = cout // 4, cout // 2
                s1, sh1 = P["bn"][name + ".bn_branch2b1"]
                s2, sh2 = P["bn"][name + ".bn_branch2b2"]
                d1 = masks[name + ".dropout_2b1"] if masks else None
                d2 = masks[name + ".dropout_2b2"] if masks else None
                v1 = E(Mo, c4)
                conv(cv["branch2a"], t, None, v1, scale=s1, shift=sh1, drop=d1)
                v2 = E(Mo, c2)
                conv(cv["branch2b1"], v1, None, v2, scale=s2, shift=sh2, drop=d2)
                xn = None
                tn = E(Mo, cout)
                if (name + ".skip_fused") in P["w"]:            # branch1 + branch2b2 in one launch: out = [t | v2] . [W_branch1 | W_branch2b2]^T (stride 1: din == dout)
                    conv(cv["branch1"]._replace(name=name + ".skip_fused"), t, xn, tn, in2=v2, scale=nsc, shift=nsh, drop=ndrop)
                else:
                    b1 = E(Mo, cout)
                    conv(cv["branch1"], t, b1)
                    conv(cv["branch2b2"], v2, xn, tn, r_post=b1, scale=nsc, shift=nsh, drop=ndrop)
                if save:
                    S[name] = dict(t=t, v1=v1, v2=v2)
            sdims[name] = (dims, odims)
            if name == "b5":
                conv4 = t
            if name == "b6":
                conv5 = t
            t, xraw, dims = tn, xn, odims
        return dict(t=t, xraw=xraw, dims=dims, conv4=conv4, conv5=conv5, sdims=sdims, N=N, V=V, dt=dt,
                    in_dims=state["in_dims"] if state is not None else [tuple(x.shape[2:]) for x in xs])

    def prefix_out_shape(self, xs):
        """(rows, channels) of run_prefix's result for these views"""
        N = xs[0].shape[0]
        dims = [tuple(x.shape[2:]) for x in xs]
        for b in arch.BLOCKS[:self.prefix.n]:
            dims = arch.block_out_dims(b, dims)
        return sum(N * h * w for (h, w) in dims), self.prefix.channels

    def run_prefix(self, xs, out=None):
        """The part of the forward pass that depends on no trainable weight: conv1a and the blocks Net.train() freezes (the net's frozen blocks, self.prefix;
        resnet38_contrast.py:86-95 `not_training`), for one or two batched views.  Returns what run_forward continues from.  Because it depends only on the
        IMAGES, the fused step runs it for the NEXT batch on a side stream inside the loss phase of the current step (loss_hip.step `lookahead`).
        out: a [prefix_out_shape] tensor for the result — the fused step allocates it on the CALLER's stream, so that the one tensor that crosses from the
        prefix stream to the next step belongs to the caller's allocator pool (no record_stream bookkeeping: with it the reserved memory grew by 6 GB)."""
        return self._run_blocks(xs, None, 0, self.prefix.n, False, None, final_t=out)

    def run_backbone(self, xs, save=False):
        """conv1a and every block, no head (the AffinityNet puts its own on top).  Returns (state, pass): state["t"] = relu(bn7(conv6)),
        state["conv4"] / ["conv5"] the inputs of b5 / b6, state["dims"] the stride-8 dims; `pass.conv` launches on the current packs.
        save: returns (state, pass, S) — S is the context run_trunk_backward takes (_run_trunk), with the four block masks."""
        if not save:
            return self._run_trunk(xs, False, None)[:2]
        assert len(xs) == 1, "the saved backbone pass takes one view"
        return self._run_trunk(xs, True, self.MASK_SPECS[:4])

    def _run_trunk(self, xs, save, mask_specs, prefix=None, keep_frozen=False):
        """The trunk's forward pass, the one entry of run_forward and run_backbone: conv1a and the frozen blocks (or the caller's `prefix`), the
        trainable blocks, the late packs joined.  mask_specs: the Dropout2d sites that get a mask in training mode — MASK_SPECS, its first four
        (the AffinityNet backbone has no dropout7: that site is present as None), or None: no dropout in any mode.  keep_frozen: the frozen
        blocks' activations are saved too (the tests' gate capture).  Returns (state of _run_blocks, pass, S), S the context, created here only:
          always: masks {site: [V*N, C] scales} or None, dims {block: (input dims, output dims)}, N, V, dt, xs
          save, read by the trunk's backward (with masks, dims, N, dt): per trainable block S[name] = {t, v} (ResBlock) or {t, v1, v2} (bottleneck),
            its input relu(bn_branch2a(x)) and the inputs of its later convs; fea = relu(bn7(conv6)) (. dropout7), bn7's ReLU mask; hdims, M
          save, read by the contrast backward only: conv4, conv5 (the inputs of b5 / b6), and what run_forward adds: lowres, head, feat, G, Fm,
            Fh, Fb, Gb, Gl, nrm, views"""
        V, dev, N = len(xs), xs[0].device, xs[0].shape[0]
        dt = DT_OF[self.net.precision]
        P = self.ensure_packs(dev, dt)
        masks = self._masks(N, V, dev, mask_specs) if mask_specs else None
        if masks is not None and len(mask_specs) == 4:
            assert "dropout7" not in masks, "the AffinityNet backbone has four Dropout2d sites: injected masks carry no dropout7"
            masks["dropout7"] = None
        S = {"masks": masks, "dims": {}, "N": N, "V": V, "dt": dt, "xs": xs}
        if prefix is None:
            prefix = self._run_blocks(xs, None, 0, self.prefix.n, keep_frozen, S if keep_frozen else None)
        assert prefix["N"] == N and prefix["V"] == V and prefix["dt"] == dt and prefix["in_dims"] == [tuple(x.shape[2:]) for x in xs], \
            "the prefix was computed for another batch shape / precision"
        st = self._run_blocks(xs, prefix, self.prefix.n, len(arch.BLOCKS), save, S)
        S["dims"].update(prefix["sdims"], **st["sdims"])
        self._join_late_packs(dev)
        ps = _Pass(self, N, dev, dt, P)
        if save:
            S.update(fea=st["t"], hdims=st["dims"], M=ps.rows_of(st["dims"]), conv4=st["conv4"], conv5=st["conv5"])
        return st, ps, S

    def run_trunk_backward(self, S, D, taps=None):
        """The backbone's backward on its own: _trunk_backward, checked, from D [M, 4096], the gradient at conv6 BEFORE bn7 (aff_head_backward's
        d_t with scale = bn7's scale and mask = t), on the context S of run_backbone(save=True).  taps {"b5": d_conv4, "b6": d_conv5}: gradients
        w.r.t. those blocks' input t = relu(bn_branch2a(x)) (pixel rows in the mode's dtype), added before the block's mask . scale.  Weight
        gradients accumulate into flat_g, block_done fires as in run_backward; the PCM and contrast-head sections do not run."""
        tdt = L.TORCH_DTYPE[S["dt"]]
        taps = dict(taps or {})
        blocks = {b[0]: b for b in self.prefix.trainable[1:]}
        for nm, tap in list(taps.items()) + [("conv6", D)]:
            if nm == "conv6":
                rows, c = S["M"], 4096
            else:
                b = blocks.get(nm)
                if b is None or arch.block_same_shape(b):
                    raise ValueError(f"run_trunk_backward: block {nm!r} takes no gradient tap (a trainable block with a skip conv, behind {self.prefix.first})")
                rows, c = sum(S["N"] * h * w for (h, w) in S["dims"][nm][0]), b[2]
            if tuple(tap.shape) != (rows, c) or tap.dtype != tdt or tap.device != S["fea"].device:
                raise ValueError(f"run_trunk_backward: the gradient at {nm} must be {tdt} rows [{rows}, {c}] on {S['fea'].device}, "
                                 f"got {tuple(tap.shape)} {tap.dtype} on {tap.device}")
            if not tap.is_contiguous():
                raise ValueError(f"run_trunk_backward: the gradient at {nm} must be contiguous (strides {tuple(tap.stride())})")
        ps = self._begin_backward(S)
        self._trunk_backward(ps, S, dict(taps, conv6=D))
        ps.end_backward()

    def _head_pass(self, t, N, ps):
        """The pass a head launches on: `ps`, the one run_backbone returned, or (None) one on the current packs with the late packs joined"""
        if ps is not None:
            return ps
        dev, dt = t.device, DT_OF[self.net.precision]
        P = self.ensure_packs(dev, dt)
        self._join_late_packs(dev)
        return _Pass(self, N, dev, dt, P)

    def run_aff_head(self, conv4, conv5, t, dims, N, ps=None):
        """The AffinityNet head as a unit (network/resnet38_aff.py:39-42): the three 1x1 ELU convs of conv4 / conv5 / t = relu(bn7(conv6)) into the
        column slices [0,64) / [64,192) / [192,448) of `feat`, then f9 + ELU.  Inputs are pixel rows in the mode's dtype; returns (feat [M,448],
        f9 [M,448]).  ps: the pass run_backbone returned (inference); None: a pass on the current packs."""
        ps = self._head_pass(t, N, ps)
        M = ps.rows_of(dims)
        C = AFF_FEAT_C

        def conv(inp, name, out, cin, cout):                  # 1x1 conv + ELU into a column slice of `out`
            ps.conv(head_conv(name, cin, cout, dims), inp, out, epi=3, ld_out=C)

        feat = ps.E(M, C)
        for name, inp in (("f8_3", conv4), ("f8_4", conv5), ("f8_5", t)):
            (cout, cin), c0 = arch.AFF_HEAD_CONVS[name], AFF_FEAT_SLICES[name][0]
            conv(inp, name, feat.view(-1)[c0:] if c0 else feat, cin, cout)
        f9 = ps.E(M, C)
        conv(feat, "f9", f9, C, C)
        return feat, f9

    def run_seg_head(self, t, dims, N, ps=None):
        """The DeepLab-v1 head as a unit (segmentation/lib/net/deeplabv1.py:42-49, eval mode): conv_fov (3x3, dilation 12) + bn_fov + ReLU,
        conv_fov2 (1x1) + bn_fov2 + ReLU, cls_conv (1x1 + bias) on t = relu(bn7(conv6)), pixel rows in the mode's dtype.  Each launch writes
        only what the next one reads (`out2`, the affine form of the epilogue).  Returns the cls_conv pixel rows [M, 24] in the mode's dtype:
        21 logits and three zero columns.  ps: the pass run_backbone returned; None: a pass on the current packs."""
        ps = self._head_pass(t, N, ps)
        M, bn = ps.rows_of(dims), ps.P["bn"]
        (c1, ci1, k1), (c2, ci2, _k2), (_c3, ci3, _k3) = arch.SEG_HEAD_CONVS.values()
        f1 = ps.E(M, c1)
        ps.conv(head_conv("conv_fov", ci1, c1, dims, k=k1, dil=arch.SEG_HEAD_DILATION), t, None, f1, scale=bn["bn_fov"][0], shift=bn["bn_fov"][1])
        f2 = ps.E(M, c2)
        ps.conv(head_conv("conv_fov2", ci2, c2, dims), f1, None, f2, scale=bn["bn_fov2"][0], shift=bn["bn_fov2"][1])
        rows = ps.E(M, arch.SEG_CLS_ROWS)
        ps.conv(head_conv("cls_conv", ci3, arch.SEG_CLS_ROWS, dims), f2, None, rows, shift=bn["cls_conv"][1], relu_out2=0)
        return rows

    def run_seg_head_train(self, t, dims, N, drop_key, ps=None):
        """The DeepLab-v1 head in TRAINING mode (deeplabv1.py:42-49 under train.py:52's plain nn.BatchNorm2d): the three conv launches of
        run_seg_head, conv_fov and conv_fov2 writing their raw output z (`out`, no fold), each followed by the batch statistics (L.bn_stats, which
        also updates the module's running statistics in place) and y = relu(z * scale + shift) (L.bn_relu_drop), the second with nn.Dropout's
        mask of `drop_key` (synth.dropout_keep); cls_conv as in inference, its bias read from the parameter into a persistent 24-element buffer.
        Returns (rows [M, 24], saved): saved holds z1, y1, z2, y2 and per BatchNorm stats [4, 512] f32 = mean, invstd, scale, shift."""
        ps = self._head_pass(t, N, ps)
        net, dev, M = self.net, t.device, ps.rows_of(dims)
        if M * 512 >= 1 << 32:
            raise ValueError(f"run_seg_head_train: {M} rows of 512 channels pass the dropout mask's 32-bit counter")
        ws = torch.empty(L.bn_stats_workspace_bytes(M, 512), device=dev, dtype=torch.uint8)
        saved, x = {}, t
        for i, (cname, (co, ci, k)) in enumerate(list(arch.SEG_HEAD_CONVS.items())[:2], 1):
            bn = self.bn_module(arch.SEG_HEAD_BNS[cname][0])
            if bn.momentum is None or not bn.track_running_stats:
                raise RuntimeError("run_seg_head_train: the head BatchNorms track running statistics with a fixed momentum")
            z = ps.E(M, co)
            ps.conv(head_conv(cname, ci, co, dims, k=k, dil=arch.SEG_HEAD_DILATION if k > 1 else 1), x, z)
            stats = torch.empty(4, co, device=dev, dtype=torch.float32)
            L.bn_stats(z, co, M, co, bn.weight.detach(), bn.bias.detach(), bn.eps, bn.momentum, stats[0], stats[1], stats[2], stats[3],
                       bn.running_mean, bn.running_var, ws)
            bn.num_batches_tracked += 1
            y = ps.E(M, co)
            L.bn_relu_drop(z, co, stats[2], stats[3], y, co, M, co, net.dropout1.p if i == 2 else 0.0, drop_key)
            saved.update({f"z{i}": z, f"y{i}": y, f"stats{i}": stats})
            x = y
        self.seg_stats_version += 1
        bias = self._seg_train_bias
        if bias is None or bias.device != dev:
            bias = self._seg_train_bias = torch.zeros(arch.SEG_CLS_ROWS, device=dev, dtype=torch.float32)
        bias[:arch.NUM_CLASSES].copy_(net.cls_conv.bias.detach())
        rows = ps.E(M, arch.SEG_CLS_ROWS)
        ps.conv(head_conv("cls_conv", arch.SEG_HEAD_CONVS["cls_conv"][1], arch.SEG_CLS_ROWS, dims), x, None, rows, shift=bias, relu_out2=0)
        return rows, saved

    SEG_CLS_DGRAD_K = 64       # channels of the cls_conv data gradient's input: the conv launch walks K in 128-byte rows (64 bf16 / 32 f32)

    def head_wt(self, device):
        """P["wt"] of the net's HEAD_CONVS (the AffinityNet's four, DeepLab's three; the contrast head's are made with its forward packs), the
        data-gradient packs [IC][T][OC] in the mode's dtype (split-bf16: pre-split), made from the f32 masters on first use per set of packs:
        inference never pays for them.  A conv whose OC is no multiple of 8 (cls_conv) gets SEG_CLS_DGRAD_K columns, its classes and zeros
        behind them: its data gradient reads a gradient buffer zero-padded to that width.  Returns the current packs."""
        dt = DT_OF[self.net.precision]
        with self.lock:
            P = self._ensure_packs(device, dt)
            specs = self.head_wt_specs()
            if specs[-1][0] not in P["wt"]:
                pdt = L.F32 if dt == L.F32X3 else dt
                for nm, off, n, (ci, T, cop) in specs:
                    co = n // (ci * T)
                    wt = (torch.empty if cop == co else torch.zeros)(ci, T, cop, device=device, dtype=L.TORCH_DTYPE[dt])
                    L.pack_weights(self.flat_w[off:off + n], None, wt, co, T, ci, cop, ci, pdt)
                    P["wt"][nm] = self._x3(wt) if dt == L.F32X3 else wt
        self._join_late_packs(device)
        return P

    def head_wt_specs(self):
        """[(name, offset of its f32 master [OC][T][IC] in the flat buffers, numel, shape [IC][T][OC'] of its transposed pack)] of the net's
        HEAD_CONVS, each (cout, cin) or (cout, cin, k); OC' = OC, or SEG_CLS_DGRAD_K where OC % 8 != 0"""
        out = []
        for nm, (co, ci, *k) in self.net.HEAD_CONVS.items():
            T = k[0] ** 2 if k else 1
            out.append((nm, *self.offsets[nm], (ci, T, co if co % 8 == 0 else self.SEG_CLS_DGRAD_K)))
        return out

    def run_forward(self, xs, save, lowres=False, prefix=None):
        """xs: list of one or two image batches (same N).  Two views are BATCHED: every activation is one row
        matrix [rows(view 1) ++ rows(view 2)][C] and every conv / wgrad is ONE launch over both row segments
        (the 128x128 view alone cannot fill the chip).  Returns ([per-view output tuple], saved context).
        prefix: the result of run_prefix(xs) when the caller has already computed it."""
        assert len(xs) in (1, 2) and all(x.shape[0] == xs[0].shape[0] for x in xs)
        st, ps, S = self._run_trunk(xs, save, self.MASK_SPECS, prefix, keep_frozen=save and self.capture_ctx)
        S["lowres"] = lowres
        N, dev, dt = ps.N, ps.dev, ps.dt
        fea, dims, conv4, conv5 = st["t"], st["dims"], st["conv4"], st["conv5"]       # fea: relu(bn7(x)) * dropout7   [M,4096]
        E, conv = ps.E, ps.conv
        M, offs = ps.rows_of(dims), ps.offs_of(dims)
        head = E(M, HEAD_LD)
        conv(head_conv("head", 4096, HEAD_LD, dims), fea, head, relu_lt=128, w_rows=256)
        feat = E(M, FEAT_LD)
        conv(head_conv("f8_3", 512, 64, dims), conv4, feat, epi=2, ld_out=FEAT_LD)
        conv(head_conv("f8_4", 1024, 128, dims), conv5, feat.view(-1)[64:], epi=2, ld_out=FEAT_LD)
        G = torch.empty(M, 32, device=dev, dtype=torch.float32)
        views = []
        for x, off, (h, w) in zip(xs, offs, dims):
            hw = h * w
            cam_low = torch.empty(N, 21, h, w, device=dev, dtype=torch.float32)
            cmax = torch.empty(N, 21, device=dev, dtype=torch.float32)
            L.head_split(head[off:], HEAD_LD, 128, cam_low, cmax, N, hw)
            L.cam_gate(cam_low, cmax, G[off:], N, hw)
            L.pcm_xs(x, feat[off:], FEAT_LD, 192, FEAT_LD, N, x.shape[2], x.shape[3], h, w)
            views.append(dict(h=h, w=w, H=x.shape[2], W=x.shape[3], off=off, rows=N * hw, cam_low=cam_low))
        Fm = E(M, 192)
        conv(head_conv("f9", FEAT_LD, 192, dims), feat, Fm)
        Fh = torch.empty(M, 192, device=dev, dtype=torch.float32)
        nrm = torch.empty(M, device=dev, dtype=torch.float32)
        L.l2norm_forward(Fm, 192, Fh, nrm, M)
        Fb = Gb = Gl = None
        if dt == L.BF16:                                      # bf16-MFMA PCM (throughput mode); fp32 mode keeps the exact-f32 kernel
            Fb = torch.empty(M, 192, device=dev, dtype=torch.bfloat16)
            Gb = torch.empty(M, 32, device=dev, dtype=torch.bfloat16)
            L.to_bf16(Fh, Fb)
            if save:                                          # the backward pass takes the gate map as hi + lo (split precision, csrc/pcm.hip)
                Gl = torch.empty(M, 32, device=dev, dtype=torch.bfloat16)
                L.split_bf16(G, Gb, Gl)
            else:
                L.to_bf16(G, Gb)
        outs = []
        for vw, x in zip(views, xs):
            h, w, off, hw = vw["h"], vw["w"], vw["off"], vw["h"] * vw["w"]
            rvd = torch.empty(N, 21, h, w, device=dev, dtype=torch.float32)
            den = torch.empty(N, hw, device=dev, dtype=torch.float32)
            if dt == L.BF16:
                L.pcm_forward_bf16(Fb[off:], Gb[off:], rvd, den, N, hw)
            else:
                L.pcm_forward(Fh[off:], G[off:], rvd, den, N, hw)
            head_v = head[off:off + N * hw].view(N, h, w, HEAD_LD)
            f_proj = head_v[..., :128].permute(0, 3, 1, 2)
            if lowres:
                outs.append((vw["cam_low"], rvd, f_proj, head_v))
            else:
                H, W = vw["H"], vw["W"]
                cam = torch.empty(N, 21, H, W, device=dev, dtype=torch.float32)
                cam_rv = torch.empty(N, 21, H, W, device=dev, dtype=torch.float32)
                L.resize_planar_fwd(vw["cam_low"], cam, N * 21, h, w, H, W, True)
                L.resize_planar_fwd(rvd, cam_rv, N * 21, h, w, H, W, True)
                outs.append((cam, cam_rv, f_proj.float() if dt == L.BF16 else f_proj, rvd))
            # (the saved copy protects the PCM backward from a caller that edits its output in place; the fused step — lowres — only reads it)
            vw.update(rvd=(rvd if lowres else rvd.clone()) if save else None, den=den)
        if save and self.capture_ctx:
            self.last_ctx = S
        if save:
            S.update(head=head, G=G, feat=feat, Fm=Fm, Fh=Fh, Fb=Fb, Gb=Gb, Gl=Gl, nrm=nrm, views=views)
        return outs, S

    # ------------------------------------------------------------------ backward
    def _begin_backward(self, S):
        """What every backward pass starts with: the transposed packs (no-op when the caller made them), the gradient views, the pass that launches"""
        self.finish_packs()
        self.attach_grads()
        ps = _Pass(self, S["N"], S["fea"].device, S["dt"], self.packs)
        ps.main = torch.cuda.current_stream(ps.dev)
        return ps

    def run_backward(self, S, grads, d_head_rows=None):
        """grads: per view (g_cam, g_cam_rv, g_fproj, g_rvd) — gradients of the view's four outputs (any may be
        None); in the fused (lowres) path g_cam / g_cam_rv are gradients of the stride-8 maps and `d_head_rows`
        (joint rows [f_proj | cam | pad]) may be supplied directly.  Accumulates into flat_g."""
        ps = self._begin_backward(S)
        P, dt, dev, N, M, hdims, masks = ps.P, ps.dt, ps.dev, ps.N, S["M"], S["hdims"], S["masks"]
        E, main, trainable, wgrad, dgrad = ps.E, ps.main, ps.trainable, ps.wgrad, ps.dgrad
        # ---- per-view adjoints of the x8 upsamples / gather of the stride-8 gradients
        d_cam_low, d_rvd = [], []
        for vw, (g_cam, g_cam_rv, g_fproj, g_rvd) in zip(S["views"], grads):
            h, w, H, W = vw["h"], vw["w"], vw["H"], vw["W"]
            if S["lowres"]:
                d_cam_low.append(g_cam)
                d_rvd.append(g_cam_rv)
                continue
            dc = None
            if g_cam is not None:
                dc = torch.empty(N, 21, h, w, device=dev, dtype=torch.float32)
                L.resize_planar_bwd(g_cam.contiguous().float(), dc, N * 21, h, w, H, W, True)
            dr = None
            if g_cam_rv is not None:
                dr = torch.empty(N, 21, h, w, device=dev, dtype=torch.float32)
                L.resize_planar_bwd(g_cam_rv.contiguous().float(), dr, N * 21, h, w, H, W, True)
            if g_rvd is not None:
                dr = g_rvd.contiguous().float() if dr is None else dr + g_rvd
            d_cam_low.append(dc)
            d_rvd.append(dr)
        # ---- PCM branch -> f9, f8_3, f8_4.  It ends in WEIGHT gradients only (f8_3 / f8_4 read conv4 / conv5 detached, resnet38_contrast.py:63-64),
        # so nothing of the backbone's backward pass waits for it: it runs on its own stream beside the first blocks (0.5 ms of small kernels + two PCM
        # launches that otherwise sit in front of the head's data gradient), joined before the gradients are consumed
        # (same-box A/B against running it in line: 35.25 / 35.16 -> 34.94 / 34.94 ms per step; the b7 launches it overlaps slow down by ~1 %).
        pcm_stream = None
        if any(d is not None for d in d_rvd):
            pcm_stream = self.stream("pcm", dev)
            pcm_stream.wait_stream(main)
            with torch.cuda.stream(pcm_stream):
                DN = torch.empty(M, 32, device=dev, dtype=torch.float32)
                dFh = torch.zeros(M, 192, device=dev, dtype=torch.float32)
                DNb = torch.empty(M, 32, device=dev, dtype=torch.bfloat16) if S["Fb"] is not None else None
                DNl = torch.empty(M, 32, device=dev, dtype=torch.bfloat16) if S["Fb"] is not None else None
                for vw, dr in zip(S["views"], d_rvd):
                    if dr is None:
                        continue
                    off, hw = vw["off"], vw["h"] * vw["w"]
                    if S["Fb"] is not None:
                        L.pcm_backward_bf16(S["Fb"][off:], S["Gb"][off:], S["Gl"][off:], dr.contiguous(), vw["rvd"], vw["den"], DN[off:], DNb[off:],
                                            DNl[off:], dFh[off:], N, hw)
                    else:
                        L.pcm_backward(S["Fh"][off:], S["G"][off:], dr.contiguous(), vw["rvd"], vw["den"], DN[off:], dFh[off:], N, hw)
                dF = E(M, 192)
                L.l2norm_backward(S["Fm"], 192, dFh, S["nrm"], dF, 192, M)
                # feature rows are [f8_3 64 | f8_4 128 | x_s 3 | pad], f9.weight's columns [x_s | f8_3 | f8_4]: the weight-gradient kernel rotates
                # its dW columns by 3 and accumulates straight into the flat gradient buffer (no staging tensor, no slice adds)
                wgrad(head_conv("f9", FEAT_LD, 192, hdims), S["feat"], dF, IC_dw=195, dw_rot=3)
                if trainable("f8_3") or trainable("f8_4"):
                    d_feat = E(M, FEAT_LD)
                    dgrad(head_conv("f9", FEAT_LD, 192, hdims), dF, d_feat, epi=1, mask=S["feat"])
                    wgrad(head_conv("f8_3", 512, 64, hdims), S["conv4"], d_feat, ld_dy=FEAT_LD)
                    wgrad(head_conv("f8_4", 1024, 128, hdims), S["conv5"], d_feat.view(-1)[64:], ld_dy=FEAT_LD)
        ps.side = pcm_stream
        # ---- head
        if d_head_rows is None:
            if all(dc is None for dc in d_cam_low) and all(g[2] is None for g in grads):
                return ps.end_backward()
            d_head_rows = E(M, HEAD_LD)
            for vw, dc, g in zip(S["views"], d_cam_low, grads):
                off, hw = vw["off"], vw["h"] * vw["w"]
                gf = g[2].contiguous().float() if g[2] is not None else None
                L.head_grad_rows(gf, dc.contiguous() if dc is not None else None, S["head"][off:], d_head_rows[off:], HEAD_LD, N, hw)
        chead = head_conv("head", 4096, HEAD_LD, hdims)
        if trainable("fc_proj") or trainable("fc8"):          # fc_proj and fc8 are adjacent in flat_g: one [149,4096] block
            L.conv_wgrad(S["fea"], d_head_rows, self.grad_slice("fc_proj", 149 * 4096), OC_dw=149, dtype=_cdt(dt), **chead.wgrad_kw(N))
        s7, _ = P["bn"]["bn7"]
        taps = {"conv6": E(M, 4096)}
        dgrad(chead, d_head_rows, taps["conv6"], epi=1, scale=s7, drop=masks["dropout7"] if masks else None, mask=S["fea"])
        self._trunk_backward(ps, S, taps)                    # (from THIS frame: the PCM branch's operands above live until its stream is joined)
        ps.end_backward()

    def _trunk_backward(self, ps, S, taps):
        """The trunk's backward pass, the block loop from the last block to the first trainable one.  taps {"conv6": D [M, 4096], the gradient at
        conv6 before bn7; block: a gradient w.r.t. that block's input t (run_trunk_backward)}.  D is taken OUT of the dict, so that a caller
        who keeps no other reference (run_backward: 0.44 GB at the training shape) has it freed when b7 has consumed it, as every later Din is."""
        P, masks, D = ps.P, S["masks"], taps.pop("conv6")
        E, rows_of, wgrad, dgrad, block_done = ps.E, ps.rows_of, ps.wgrad, ps.dgrad, ps.block_done
        for b in reversed(self.prefix.trainable):
            name, kind, cin, mid, cout, stride, fd, d, p = b
            same = arch.block_same_shape(b)
            din, dout = S["dims"][name]
            Mi, Mo = rows_of(din), rows_of(dout)
            sv = S[name]
            sa, _ = P["bn"][name + ".bn_branch2a"]
            first_trainable = name == self.prefix.first  # its input comes from the frozen prefix
            cv = block_launch_convs(b, din, dout)
            c2a, c2b1, c1 = cv["branch2a"], cv["branch2b1"], cv.get("branch1")
            tap = taps.get(name)                         # a gradient w.r.t. this block's input t from outside the trunk: r_pre of the launch that writes Din (or tmp)
            if kind == "res":
                s1, _ = P["bn"][name + ".bn_branch2b1"]
                du = E(Mo, mid)
                # (each data gradient takes the weight gradient of the same dY into its launch: wseg_conv_bwd_pair)
                dgrad(c2b1, D, du, epi=1, scale=s1, mask=sv["v"], pair=(c2b1, sv["v"], D))
                fused_skip = (name + ".skip_fused") in P["wt"] and not first_trainable
                if not (same and not first_trainable):
                    wgrad(c2a, sv["t"], du)
                if not same and not fused_skip:
                    wgrad(c1, sv["t"], D)
                if first_trainable:
                    block_done(name)
                    break
                Din = E(Mi, cin)
                if same:
                    dgrad(c2a, du, Din, epi=1, scale=sa, mask=sv["t"], r_post=D, pair=(c2a, sv["t"], du))
                elif fused_skip:                               # branch2a's and branch1's data gradients into t in one launch: 9 taps of du + one K segment of D (+ the skip conv's weight gradient: same D)
                    dgrad(c2a._replace(name=name + ".skip_fused"), du, Din, in2=D, IC2=cout, epi=1, scale=sa, mask=sv["t"], pair=(c1, sv["t"], D),
                          r_pre=tap)
                else:
                    tmp = E(Mi, cin)
                    dgrad(c1, D, tmp, r_pre=tap)
                    dgrad(c2a, du, Din, epi=1, scale=sa, mask=sv["t"], r_pre=tmp)
                D = Din
                block_done(name)
            else:
                c4, c2 = cout // 4, cout // 2
                s1, _ = P["bn"][name + ".bn_branch2b1"]
                s2, _ = P["bn"][name + ".bn_branch2b2"]
                d1 = masks[name + ".dropout_2b1"] if masks else None
                d2 = masks[name + ".dropout_2b2"] if masks else None
                c2b2 = cv["branch2b2"]
                du2 = E(Mo, c2)
                dgrad(c2b2, D, du2, epi=1, scale=s2, drop=d2, mask=sv["v2"], pair=(c2b2, sv["v2"], D))
                du1 = E(Mo, c4)
                dgrad(c2b1, du2, du1, epi=1, scale=s1, drop=d1, mask=sv["v1"], pair=(c2b1, sv["v1"], du2))
                wgrad(c2a, sv["t"], du1)
                Din = E(Mi, cin)
                if (name + ".skip_fused") in P["wt"]:          # branch1's and branch2a's 1x1 data gradients into t as ONE two-source product (+ the skip conv's weight gradient)
                    dgrad(c1._replace(name=name + ".skip_fused"), D, Din, epi=1, scale=sa, mask=sv["t"], in2=du1, IC2=c4,
                          pair=(c1, sv["t"], D), r_pre=tap)
                else:
                    tmp = E(Mi, cin)
                    dgrad(c1, D, tmp, pair=(c1, sv["t"], D), r_pre=tap)
                    dgrad(c2a, du1, Din, epi=1, scale=sa, mask=sv["t"], r_pre=tmp)
                D = Din
                block_done(name)


class _NetFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, anchor, eng, lowres):
        outs, S = eng.run_forward([x], save=True, lowres=lowres)
        ctx.eng, ctx.S = eng, S
        ctx.set_materialize_grads(False)
        if lowres:
            ctx.mark_non_differentiable(outs[0][3])
        return outs[0]

    @staticmethod
    def backward(ctx, g0, g1, g2, g3):
        S = ctx.S
        ctx.eng.run_backward(S, [(g0, g1, g2, None if S["lowres"] else g3)])
        ctx.S = None
        return None, None, None, None
