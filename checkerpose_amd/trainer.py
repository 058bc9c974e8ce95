"""Training-side launch program: the forward in train mode (batch-statistics BatchNorm, live
weights re-packed inside the program) followed by its own backward, as ONE static launch list over the C ABI.

Design.  TrainProgram extends engine.Program with a *tape*: every forward emitter that has a gradient pushes a closure
which, when the tape is unwound in reverse, appends the backward launches (BN / bias backward, data-gradient convs --
the forward conv kernels over transformed weights --, MFMA weight-gradients, graph-op marginals).  Activation
gradients live in the storage dtype in per-tensor buffers that are zero-filled once and accumulated into (conv
epilogues accumulate through their `residual` operand), parameter gradients are fp32 slices of ONE flat buffer
(a single bucket for the data-parallel all-reduce, parallel.allreduce_gradients_).  The liveness planner of the base
class keeps every saved activation alive until its last backward reader automatically.  Nothing here computes;
torch supplies memory and the autograd hook (model/_runtime.py: _TrainFn) only.
"""
import ctypes as C
import os
import weakref
from typing import NamedTuple, Optional

import torch

from . import _abi
from ._abi import (CpWgradReduceItem, CpWgradItem, CpFuseBwdItem, CP_WGRAD_ITEM_3X3_S2_SMALL, CP_WGRAD_ITEM_3X3, CP_WGRAD_ITEM_3X3_SMALL, CP_WGRAD_ITEM_GENERIC_BF16,
                   CP_WGRAD_ITEM_GENERIC_F32, ACT_LEAKY, ACT_NONE, ACT_RELU, CP_BF16, CP_F32, CpPackItem, CpWgradDesc, CpBnItem, BN_GROUP_MAX,
                   CP_BN_ITEM_STATS, CP_BN_ITEM_APPLY, CP_BN_ITEM_BWD_SUMS, CP_BN_ITEM_BWD_APPLY)
from .engine import Act, Program, WeightStore, _ptr, _rup


ALL_TAPS_KINDS = (CP_WGRAD_ITEM_3X3, CP_WGRAD_ITEM_3X3_SMALL, CP_WGRAD_ITEM_3X3_S2_SMALL)      # one block = all nine taps
MARKERS = ("__fork__", "__sync__", "__join__", "__mark__", "__wait__")                          # ops that are no launches


# ---- train-mode BatchNorm: the records of a layer and the argument tuples of its four passes.  A pass over ONE layer is a launch of its
# own (cp_bn_*), a pass over several independent layers is a grouped launch (cp_bn_group) whose items cp_bn_item_* fill from the SAME
# tuple: the C signatures differ only in the leading stream and the trailing CpBnItem*
class BnState(NamedTuple):
    """what a train-mode BatchNorm layer's forward keeps: the batch statistics the apply pass writes (the backward reads them), the
    live parameters and running statistics, the layer's fp64 accumulator slot"""
    mean: torch.Tensor
    rstd: torch.Tensor
    gamma: torch.Tensor
    beta: torch.Tensor
    rmean: torch.Tensor
    rvar: torch.Tensor
    acc: int
    momentum: float = 0.1
    eps: float = 1e-5


class BnLayer(NamedTuple):
    """forward: out = act(BatchNorm(x) + residual) over the batch statistics of the raw conv output x"""
    x: Act
    gamma: torch.Tensor
    beta: torch.Tensor
    rmean: torch.Tensor
    rvar: torch.Tensor
    residual: Optional[Act]
    out: Act
    act: int
    slope: float = 0.0
    st: Optional[BnState] = None       # filled in by TrainProgram.bn_forward


class BnGrad(NamedTuple):
    """backward, in place on gy: gy <- d loss / d raw ; gres += dz ; dgamma / dbeta written.  raw None (and bn None) = bias-only layer;
    y is read only behind an activation"""
    gy: Act
    y: Optional[Act]
    raw: Optional[Act]
    bn: Optional[BnState]
    act: int
    slope: float
    gres: Optional[Act]
    dgamma: Optional[int]
    dbeta: Optional[int]
    acc: int = 0                       # filled in by TrainProgram.bn_backward


def _opt(P, a):
    """the (pointer, channel stride, channel offset) triple of an optional operand"""
    return (P(a.tbuf), a.cstride, a.coff) if a is not None else (None, 0, 0)


def _tbufs(*acts):
    return [a.tbuf for a in acts if a is not None]


def _bn_stats_args(tp, P, m):
    x = m.x
    return (tp.dtype, P(x.tbuf), x.B * x.H * x.W, x.C, x.cstride, x.coff, tp._acc_ptr(m.st.acc))


def _bn_apply_args(tp, P, m):
    x, st, out = m.x, m.st, m.out
    return ((tp.dtype, P(x.tbuf), x.cstride, x.coff, tp._acc_ptr(st.acc), st.gamma.data_ptr(), st.beta.data_ptr(), st.rmean.data_ptr(),
             st.rvar.data_ptr(), st.momentum, st.eps) + _opt(P, m.residual) +
            (P(out.tbuf), out.cstride, out.coff, x.B * x.H * x.W, x.C, m.act, m.slope, st.mean.data_ptr(), st.rstd.data_ptr()))


def _bn_bwd_head(tp, P, m):
    gy = m.gy
    return (tp.dtype, P(gy.tbuf), gy.cstride, gy.coff) + _opt(P, m.y) + _opt(P, m.raw) + (_ptr(m.bn and m.bn.mean), _ptr(m.bn and m.bn.rstd))


def _bn_bwd_sums_args(tp, P, m):
    gy = m.gy
    return _bn_bwd_head(tp, P, m) + (gy.B * gy.H * gy.W, gy.C, m.act, m.slope, tp._acc_ptr(m.acc))


def _bn_bwd_apply_args(tp, P, m):
    gy = m.gy
    return (_bn_bwd_head(tp, P, m) + (_ptr(m.bn and m.bn.gamma), tp._acc_ptr(m.acc), gy.B * gy.H * gy.W, gy.C, m.act, m.slope) +
            _opt(P, gy) + _opt(P, m.gres) + (1, m.dgamma, m.dbeta))


class BnPass(NamedTuple):
    name: str          # recorder name of the single launch; the grouped one is <name>_group:<members>
    single: str        # C entry point of the pass over one layer
    fill: str          # C entry point that fills a CpBnItem from the same arguments
    kind: int          # CP_BN_ITEM_*
    args: object       # (program, P, record) -> the argument tuple behind the stream
    reads: object      # record -> TBufs read
    writes: object     # record -> TBufs written


BN_STATS = BnPass("bn_stats", "cp_bn_stats_accumulate", "cp_bn_item_stats", CP_BN_ITEM_STATS, _bn_stats_args,
                  lambda m: _tbufs(m.x), lambda m: [])
BN_APPLY = BnPass("bn_apply", "cp_bn_apply", "cp_bn_item_apply", CP_BN_ITEM_APPLY, _bn_apply_args,
                  lambda m: _tbufs(m.x, m.residual), lambda m: _tbufs(m.out))
BN_BWD_SUMS = BnPass("bn_bwd_acc", "cp_bn_bwd_accumulate", "cp_bn_item_bwd_sums", CP_BN_ITEM_BWD_SUMS, _bn_bwd_sums_args,
                     lambda m: _tbufs(m.gy, m.y, m.raw), lambda m: [])
BN_BWD_APPLY = BnPass("bn_bwd", "cp_bn_bwd_apply", "cp_bn_item_bwd_apply", CP_BN_ITEM_BWD_APPLY, _bn_bwd_apply_args,
                      lambda m: _tbufs(m.gy, m.y, m.raw, m.gres), lambda m: _tbufs(m.gy, m.gres))


class TrainWeightStore(WeightStore):
    """Weights change every step: packing launches are appended to the program (right before their consumer) instead
    of being run once at build time; per-channel vectors may be live device tensors passed through unchanged."""

    def __init__(self, lib, sd, dtype, device):
        super().__init__(lib, sd, dtype, device)
        self.prog = None
        self.passthrough = set()
        self.repacks_every_step = True

    def _image(self, ck, nbytes, keep, fill, what):
        """a packed weight image of `nbytes`, made once per cache key `ck`: one "packs" item of the program, filled by
        fill(image pointer, byref(item)) -> status; `keep`: the tensors the item reads"""
        def make():
            out = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
            self.prog.keep += keep + [out]
            self.prog.prep_item("packs", lambda ref: fill(out.data_ptr(), ref), what)
            return out
        return self.cached(ck, make)

    def pack(self, name, w, Cout, Cin, R, S, cin_phys, cout_rows, transposed=0, phase=0, row_map=None):
        def fill(op, ref):
            rm = None
            if row_map is not None:
                rm = torch.tensor(row_map, dtype=torch.int32, device=self.device)
                self.prog.keep.append(rm)
            return self.lib.cp_pack_item_conv(self.dtype, w.data_ptr(), Cout, Cin, R, S, cin_phys, transposed, phase, _ptr(rm), cout_rows, op, ref)
        return self._image((name, cin_phys, cout_rows, transposed, phase), self.lib.cp_packed_weight_bytes(self.dtype, cout_rows, cin_phys, R, S),
                           [w], fill, "pack:" + name)

    def pack_halo(self, name, w, Cout, Cin, cin_phys):
        return self._image(("halo", name, cin_phys), self.lib.cp_packed_halo_weight_bytes(self.dtype, Cout, cin_phys), [w],
                           lambda op, ref: self.lib.cp_pack_item_halo(self.dtype, w.data_ptr(), Cout, Cin, cin_phys, op, ref), "pack_halo:" + name)

    def pack_gemm(self, name, w, Cout, Cin, cin_phys):
        return self._image(("gemm", name, cin_phys), self.lib.cp_packed_gemm_weight_bytes(self.dtype, Cout, cin_phys), [w],
                           lambda op, ref: self.lib.cp_pack_item_gemm(self.dtype, w.data_ptr(), Cout, Cin, cin_phys, op, ref), "pack_gemm:" + name)

    def affine(self, name, scale, shift, rows):
        if id(scale) in self.passthrough and id(shift) in self.passthrough:
            return scale, shift
        return super().affine(name, scale, shift, rows)


_WG_ARENAS = weakref.WeakValueDictionary()      # the TrainPrograms hold the arenas: the last program gone, its 4 GiB go back to torch


def _shared_wgrad_arena(device):
    """The weight-gradient partial-sum arena of `device` + the current stream (CHECKERPOSE_AMD_WGRAD_ARENA_MB, default 4096), and that
    stream's handle: partial sums of two programs that share an arena are ordered only by running on ONE stream, so a program
    remembers the stream it was built for and `_TrainFn` refuses to replay it on another (model/_runtime.py)."""
    dev = torch.device(device)
    idx = dev.index if dev.index is not None else torch.cuda.current_device()
    nbytes = int(os.environ.get("CHECKERPOSE_AMD_WGRAD_ARENA_MB", "4096")) << 20
    stream = torch.cuda.current_stream(dev).cuda_stream
    key = (idx, stream, nbytes)
    arena = _WG_ARENAS.get(key)
    if arena is None:
        arena = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        _WG_ARENAS[key] = arena
    return arena, stream


class PendingWgrad:
    """a layer's weight gradient waiting for its grouped launch (flush_wgrad_compute fills kind .. wsn in three phases)"""
    __slots__ = ("lib", "d", "dt", "xt", "dw", "flops", "k3s1", "pix", "cc", "taps", "kind", "work", "target", "need", "blocks", "wsp", "wsn")

    def __init__(self, lib, d, dt, xt, dw, flops):
        self.lib, self.d, self.dt, self.xt, self.dw, self.flops = lib, d, dt, xt, dw, flops
        self.k3s1 = d.R == 3 and d.stride == 1
        self.pix, self.cc, self.taps = d.B * d.Ho * d.Wo, ((d.Cout + 63) // 64) * ((d.Cin + 63) // 64), d.R * d.S

    def item(self, dy, x, ws, ws_bytes, target):
        """this layer's share of a grouped launch over the operands dy / x, its partial tiles in ws[:ws_bytes], cut into about `target`
        workgroups -> (CpWgradItem, the CpWgradReduceItem it owes: ws null if it adds with atomics instead)"""
        ci, ri = CpWgradItem(), CpWgradReduceItem()
        _abi.check(self.lib.cp_conv2d_wgrad_item(C.byref(self.d), dy, x, self.dw, ws, ws_bytes, target, C.byref(ci), C.byref(ri)),
                   "cp_conv2d_wgrad_item")
        return ci, ri


class TrainProgram(Program):
    training = True

    def __init__(self, lib, ws, dtype, B, device, pgrad, pslots):
        super().__init__(lib, ws, dtype, B, device)
        ws.prog = self
        self.tape = []
        self.grads = {}            # forward TBuf -> gradient TBuf
        self.pgrad = pgrad         # flat fp32 parameter-gradient buffer
        self.pslots = pslots       # state-dict key -> element offset into pgrad
        self.nograd = set()        # id(TBuf) of tensors that need no gradient (the input image)
        self._bn_ws = {}           # lane -> BatchNorm partial-sum workspace
        # weight-gradient pixel-slice partials: every layer gets its OWN region of this arena and its reduction is DEFERRED; when the
        # arena is full (and at the end of the backward) one cp_wgrad_reduce_batch launch settles every pending layer
        # (ONE arena per device and stream, shared by every TrainProgram -- the stage schedule, a ragged last batch and a second module
        # each build their own program, but the partials never outlive the backward that wrote them and backwards on one stream are
        # ordered)
        self.wg_ws, self.wg_stream = _shared_wgrad_arena(device)
        self._wg_off, self._wg_items, self._wg_keys = 0, [], set()
        # grouped weight gradients: the partial-sum launches of up to wg_group_n layers wait for each other and go out as ONE launch
        # per kernel kind (cp_wgrad_group), every layer cut into its share of wg_group_blocks workgroups instead of a GPU's worth
        self.wg_group_n = int(os.environ.get("CHECKERPOSE_AMD_WGRAD_GROUP_N", "64"))
        self.wg_group_flops = float(os.environ.get("CHECKERPOSE_AMD_WGRAD_GROUP_GFLOP", "40")) * 1e9     # bigger layers launch alone
        gb = [int(v) for v in os.environ.get("CHECKERPOSE_AMD_WGRAD_GROUP_BLOCKS", "512,1024,1024").split(",")]
        self.wg_group_blocks = {CP_WGRAD_ITEM_3X3: gb[0], CP_WGRAD_ITEM_3X3_SMALL: gb[1], CP_WGRAD_ITEM_GENERIC_BF16: gb[2],
                                CP_WGRAD_ITEM_GENERIC_F32: gb[2], CP_WGRAD_ITEM_3X3_S2_SMALL: gb[1]}
        self.wg_reduce_n = int(os.environ.get("CHECKERPOSE_AMD_WGRAD_REDUCE_N", "96"))
        self._wgc_pending = []
        self.wgrad_flops = {}      # op index -> algorithmic FLOPs of that weight-gradient launch (bench_train roofline)
        self.n_fwd_ops = None
        self._touched, self.pslot_done, self.pslot_done_call = [], {}, {}
        self._ones, self._zeros = {}, {}
        self.acc_total = 0         # fp64 BatchNorm accumulators (elements), one arena zero-filled at the start of a step
        self.acc_arena = None
        self._add(lib.cp_memset_zero, lambda P: (self.acc_arena.data_ptr(), self.acc_arena.numel() * 8), "acc_zero", [], [])
        # weight preparation (packing, data-gradient / EdgeConv views, bias refreshes) reads only parameters: all items of a
        # half are processed by TWO launches at its start (views, then the packs that may consume them) -- cp_pack_batch
        self.items = {("views", 0): [], ("packs", 0): [], ("views", 1): [], ("packs", 1): []}
        self.prep_tabs = {}        # (kind, half) -> that launch's table (finalize)
        self.half = 0
        for kind in ("views", "packs"):
            self._add(lib.cp_pack_batch, (lambda k: lambda P: self._batch_args(k, 0))(kind), "prep_%s_fwd" % kind, [], [])
        self.arena = []            # gradient TBufs (not recycled: 288 GB of HBM; one zero fill instead of ~370)
        self.grad_arena = None
        self.kinks = {}            # activation key -> Act whose sign is the (Leaky)ReLU branch taken (tests: oracle FORCE_MASK)
        self.debug = {}            # name -> Acts of interest (tools/train_debug.py with CHECKERPOSE_AMD_NO_RECYCLE=1)

    # ---- lanes: the FORWARD half keeps the eval program's fork/join markers (the liveness planner keeps a region's tensors alive
    # over the whole region); the backward half is emitted after the last join.  Both halves replay on one ordered stream.
    # Scratch that is shared between launches is per lane (bn_ws).
    def prep_item(self, kind, fill, what):
        """one item of the current half's `kind` ("views" / "packs") launch, filled by fill(byref(item)) -> status"""
        it = CpPackItem()
        _abi.check(fill(C.byref(it)), what)
        self.items[(kind, self.half)].append(it)

    def _batch_args(self, kind, half):
        return (self.dtype,) + self.prep_tabs.get((kind, half), (None, None, 0, 0))

    def _table(self, items, blocks):
        """the device tables of a grouped launch over `items` (workgroups per item: `blocks`), kept alive with the program ->
        (item table pointer, prefix table pointer, number of items, total workgroups)"""
        raw, prefix, total = _abi.device_table(items, blocks, self.device)
        self.keep += [raw, prefix]
        return (raw.data_ptr(), prefix.data_ptr(), len(items), total)

    # ---- small helpers
    @property
    def bn_ws(self):
        if self.lane not in self._bn_ws:
            self._bn_ws[self.lane] = torch.empty(self.lib.cp_bn_bwd_workspace_bytes(4096), dtype=torch.uint8, device=self.device)
        return self._bn_ws[self.lane]

    def const_vec(self, n, one):
        d = self._ones if one else self._zeros
        n = _rup(n, 16)
        if n not in d:
            d[n] = (torch.ones if one else torch.zeros)(n, dtype=torch.float32, device=self.device)
            self.ws.passthrough.add(id(d[n]))
        return d[n]

    def vec(self, n):
        t = torch.zeros(_rup(n, 16), dtype=torch.float32, device=self.device)
        self.keep.append(t)
        self.ws.passthrough.add(id(t))
        return t

    def pg_ptr(self, key):
        self._touched.append(key)          # the tape closure being unwound writes this parameter's gradient
        return self.pgrad.data_ptr() + 4 * self.pslots[key]

    def memset_t(self, tbuf, name="memset"):
        fn = self.lib.cp_memset_zero
        nb = tbuf.nbytes
        self._add(fn, lambda P: (P(tbuf), nb), name, [], [tbuf])

    def memcpy(self, dst_ptr, src_ptr, nbytes, name="memcpy", prep=False):
        if prep:
            self.prep_item("views", lambda ref: self.lib.cp_pack_item_copy_f32(src_ptr, dst_ptr, nbytes // 4, ref), name)
        else:
            self._add(self.lib.cp_memcpy_d2d, lambda P: (dst_ptr, src_ptr, nbytes), name, [], [])

    def live_vec(self, n, segments):
        """padded fp32 vector refreshed inside the program from live parameter storage: segments = [(dst_off, tensor,
        src_off, count)]"""
        t = self.vec(n)
        for doff, src, soff, cnt in segments:
            self.keep.append(src)
            self.memcpy(t.data_ptr() + 4 * doff, src.data_ptr() + 4 * soff, 4 * cnt, "refresh_vec", prep=True)
        return t

    def scratch_f32(self, numel):
        t = torch.empty(numel, dtype=torch.float32, device=self.device)
        self.keep.append(t)
        return t

    def grad_of(self, a: Act):
        """gradient view matching `a` (same geometry) -- buffer created and zero-filled on first request"""
        g = self.grads.get(a.tbuf)
        if g is None:
            g = self.tensor(a.tbuf.nbytes, es=1)
            g.nbytes = a.tbuf.nbytes
            self.grads[a.tbuf] = g
            self.arena.append(g)       # gradient buffers live in one arena zero-filled by ONE launch (finalize())
        return Act(g, a.B, a.H, a.W, a.C, a.Cphys, a.cstride, a.coff)

    def needs_grad(self, a: Act):
        return id(a.tbuf) not in self.nograd

    # ---- train-mode BatchNorm: two launches per pass (column sums by fp64 atomics into a per-layer accumulator pair, then the
    # consumer kernel derives the coefficients itself) -- the accumulators of the whole step are zero-filled by ONE launch
    def _acc_slot(self, C_):
        off = self.acc_total
        self.acc_total += int(self.lib.cp_bn_acc_doubles(C_))
        return off

    def _acc_ptr(self, off):
        return self.acc_arena.data_ptr() + 8 * off

    def _bn_pass(self, p: BnPass, members):
        """one BatchNorm pass over INDEPENDENT layers (the branches of an HRNet module at equal depth, the fuse convs of a module): one
        layer is a launch of its own; several go out as ONE launch per BN_GROUP_MAX of them (cp_bn_group: at B = 32 a single pass is a
        5-13 us launch over 0.3-5 MB, latency not bandwidth), their items built when the workspace is planned (pointers are final then)"""
        reads, writes = [t for m in members for t in p.reads(m)], [t for m in members for t in p.writes(m)]
        if len(members) == 1:
            m = members[0]
            self._add(getattr(self.lib, p.single), lambda P: p.args(self, P, m), p.name, reads, writes)
            return
        fill = getattr(self.lib, p.fill)
        for lo in range(0, len(members), BN_GROUP_MAX):
            chunk = members[lo:lo + BN_GROUP_MAX]

            def argb(P, chunk=chunk):
                items = [CpBnItem() for _ in chunk]
                for m, it in zip(chunk, items):
                    _abi.check(fill(*p.args(self, P, m), C.byref(it)), p.fill)
                return (self.dtype, p.kind) + self._table(items, [it.blocks for it in items]) + (max(int(it.lds_bytes) for it in items),)
            self._add(self.lib.cp_bn_group, argb, "%s_group:%d" % (p.name, len(chunk)), reads, writes)

    def bn_forward(self, layers):
        """[BnLayer] of independent layers -> [BnState]: the statistics of all of them, then apply (+residual, +activation)"""
        members = []
        for m in layers:
            C_ = m.x.C
            st = BnState(self.vec(C_), self.vec(C_), m.gamma, m.beta, m.rmean, m.rvar, self._acc_slot(C_))
            self.keep += [m.gamma, m.beta, m.rmean, m.rvar]
            members.append(m._replace(st=st))
        self._bn_pass(BN_STATS, members)
        self._bn_pass(BN_APPLY, members)
        return [m.st for m in members]

    def affine_act(self, x: Act, scale, shift, residual, out: Act, act, slope=0.0):
        xt, ot = x.tbuf, out.tbuf
        rt = residual.tbuf if residual is not None else None
        M = x.B * x.H * x.W
        sp, tp = scale.data_ptr(), shift.data_ptr()
        rcs, rco = (residual.cstride, residual.coff) if residual is not None else (0, 0)
        self._add(self.lib.cp_affine_act,
                  lambda P: (self.dtype, P(xt), x.cstride, x.coff, sp, tp, P(rt) if rt is not None else None, rcs, rco, P(ot),
                             out.cstride, out.coff, M, x.C, act, slope), "affine_act", [xt, rt], [ot])
        return out

    def bn_backward(self, grads):
        """[BnGrad] of independent layers: the column sums of all of them, then apply"""
        members = [m._replace(y=m.y if m.act != ACT_NONE else None, acc=self._acc_slot(m.gy.C)) for m in grads]
        self._bn_pass(BN_BWD_SUMS, members)
        self._bn_pass(BN_BWD_APPLY, members)

    def bn_bwd(self, *m):
        """bn_backward of one layer: the fields of a BnGrad"""
        self.bn_backward([BnGrad(*m)])

    # ---- dense layer backward
    def wgrad(self, dy: Act, x: Act, dw_ptr, Cout, Cin, R, S, stride, pad, Ho=None, Wo=None, base=0, sco=None, sci=None):
        d = CpWgradDesc()
        d.dtype, d.B, d.H, d.W = self.dtype, x.B, x.H, x.W
        d.Ho, d.Wo = (dy.H, dy.W) if Ho is None else (Ho, Wo)
        d.Cout, d.dy_cstride, d.dy_coff = Cout, dy.cstride, dy.coff
        d.Cin, d.x_cstride, d.x_coff = Cin, x.cstride, x.coff
        d.R, d.S, d.stride, d.pad = R, S, stride, pad
        d.dw_base, d.dw_sco, d.dw_sci, d.dw_sr, d.dw_ss = base, (Cin * R * S if sco is None else sco), (R * S if sci is None else sci), S, 1
        self.keep.append(d)
        dref = C.byref(d)
        dt, xt = dy.tbuf, x.tbuf
        name = "wgrad:%d->%d k%d s%d %dx%d" % (Cin, Cout, R, stride, x.H, x.W)
        flops = 2 * dy.B * d.Ho * d.Wo * R * S * Cin * Cout                # algorithmic, unpadded
        if flops < self.wg_group_flops:
            self._wgc_pending.append(PendingWgrad(self.lib, d, dt, xt, dw_ptr, flops))
            if len(self._wgc_pending) >= self.wg_group_n:
                self.flush_wgrad_compute()
            return
        need = (int(self.lib.cp_conv2d_wgrad_scratch_bytes(dref)) + 255) // 256 * 256
        if self._wg_off + need > self.wg_ws.numel():
            self.flush_wgrad_compute()
            self._flush_wgrad_reduce()
        need = min(need, self.wg_ws.numel())
        wsp = self.wg_ws.data_ptr() + self._wg_off
        item, spare = CpWgradReduceItem(), CpWgradReduceItem()
        base = self.wg_ws.data_ptr()      # any aligned non-null pointer: the plan only validates dy / x, it launches nothing
        _abi.check(self.lib.cp_conv2d_wgrad_plan(dref, base, base, dw_ptr, wsp, need, C.byref(item)), "cp_conv2d_wgrad_plan")
        self.keep.append(spare)
        sref = C.byref(spare)
        self._add(self.lib.cp_conv2d_wgrad_deferred, lambda P: (dref, P(dt), P(xt), dw_ptr, wsp, need, sref), name, [dt, xt], [])
        if item.ws:                       # this layer owes a reduction (tiny layers add with atomics instead)
            self._wg_items.append(item)
            self._wg_off += need
        self.wgrad_flops[len(self.ops) - 1] = flops

    def flush_wgrad_compute(self):
        """the partial-sum launches of the waiting layers: ONE launch per kernel kind.  A layer's share of the launch's workgroups is
        proportional to its work (pixels x channel blocks), so all blocks of a launch run about equally long."""
        pend, self._wgc_pending = self._wgc_pending, []
        if not pend:
            return
        arena, asz = self.wg_ws.data_ptr(), self.wg_ws.numel()
        for m in pend:                        # kernel kind of every layer (depends on the descriptor only)
            m.kind = int(m.item(arena, arena, arena, asz, 0)[0].kind)
            m.work = m.pix * m.cc * (1 if m.kind in ALL_TAPS_KINDS else m.taps)
        kinds = sorted({m.kind for m in pend})
        for kind in kinds:                    # every layer's share of its launch, and the partial tiles that share needs
            mem = [m for m in pend if m.kind == kind]
            total = float(sum(m.work for m in mem))
            for m in mem:
                m.target = max(1, int(round(self.wg_group_blocks[kind] * m.work / total)))
                ci, ri = m.item(arena, arena, arena, asz, m.target)
                m.need = (int(ri.S) * int(ri.GY) * int(ri.taps_in_block) * 4096 * 4 + 255) // 256 * 256 if ri.ws else 0
                m.blocks = int(ci.blocks)
        need_all = sum(m.need for m in pend)
        if need_all > asz:
            raise RuntimeError("checkerpose_amd: the weight-gradient arena (%d MB, CHECKERPOSE_AMD_WGRAD_ARENA_MB) is smaller than the partial "
                               "tiles of one group of layers (%d MB)" % (asz >> 20, (need_all >> 20) + 1))
        if self._wg_off + need_all > asz:     # the reductions owed so far (their producers are all emitted) free the arena
            self._flush_wgrad_reduce()
        for kind in kinds:                    # every layer's place in the arena, and the launch of its kind
            mem = [m for m in pend if m.kind == kind]
            for m in mem:
                if m.need:
                    m.wsp, m.wsn = arena + self._wg_off, m.need
                    ci, ri = m.item(arena, arena, m.wsp, m.wsn, m.target)
                    assert ri.ws == m.wsp and int(ci.blocks) == m.blocks
                    self._wg_items.append(ri)
                    self._wg_off += m.need
                else:
                    m.wsp, m.wsn = arena, asz

            def argb(P, mem=mem, kind=kind):
                items = [m.item(P(m.dt), P(m.xt), m.wsp, m.wsn, m.target)[0] for m in mem]
                assert all(int(it.blocks) == m.blocks and int(it.kind) == m.kind for it, m in zip(items, mem))
                return (kind,) + self._table(items, [it.blocks for it in items])
            k3 = all(m.k3s1 for m in mem)
            self._add(self.lib.cp_wgrad_group, argb, "wgrad_group:%s x%d" % (" k3 s1 " if k3 else "mixed", len(mem)),
                      [t for m in mem for t in (m.dt, m.xt)], [])
            self.wgrad_flops[len(self.ops) - 1] = sum(m.flops for m in mem)
        if len(self._wg_items) >= self.wg_reduce_n:        # settle in a few instalments: the data-parallel step's gradient buckets
            self.flush_wgrad()                              # complete (and start their all-reduce) while the backward goes on

    def _flush_wgrad_reduce(self):
        if self._wg_items:
            tab = self._table(self._wg_items, [self.lib.cp_wgrad_reduce_item_blocks(C.byref(it)) for it in self._wg_items])
            self._add(self.lib.cp_wgrad_reduce_batch, lambda P: tab, "wgrad_reduce_batch:%d" % tab[2], [], [])
        self._wg_off, self._wg_items = 0, []

    def flush_wgrad(self):
        """every weight-gradient launch still waiting, then one launch for every reduction owed so far; the parameters touched since
        the last flush are final only behind it (gradient buckets of the data-parallel step, plan_gradient_buckets)"""
        self.flush_wgrad_compute()
        self._flush_wgrad_reduce()
        for k in self._wg_keys:
            self.pslot_done[k] = len(self.ops)
        self._wg_keys = set()

    def weight_dgrad(self, w, Cout, Cin, R, S):
        wt = self.scratch_f32(Cout * Cin * R * S).view(Cin, Cout, R, S)
        self.keep.append(w)
        self.prep_item("views", lambda ref: self.lib.cp_pack_item_dgrad_view(w.data_ptr(), Cout, Cin, R, S, wt.data_ptr(), ref), "weight_dgrad")
        return wt

    def conv_backward(self, key, w, x: Act, g: Act, R, S, stride, pad):
        """g = d loss / d (raw conv output) in channels-last; accumulates into grad(x), writes the weight gradient."""
        self.conv_backward_group([(key, w, x, g, R, S, stride, pad)])

    def conv_backward_group(self, members):
        """conv_backward of INDEPENDENT layers [(key, w, x, g, R, S, stride, pad)]: every weight gradient first, the 3x3 / stride 1
        data-gradient convs behind them"""
        dg = []
        for key, w, x, g, R, S, stride, pad in members:
            Cout, Cin = w.shape[0], w.shape[1]
            self.wgrad(g, x, self.pg_ptr(key + ".weight"), Cout, Cin, R, S, stride, pad)
            if not self.needs_grad(x):
                continue
            if stride == 1 and R == 3 and S == 3 and pad == 1:
                gx = self.grad_of(x)
                wt = self.weight_dgrad(w, Cout, Cin, 3, 3)
                dg.append((g, key + "#dgrad", wt, self.const_vec(Cin, True), self.const_vec(Cin, False), gx))
            else:
                self._dgrad(key, w, x, g, R, S, stride, pad)
        for g, key, wt, one, zero, gx in dg:
            self.conv(g, key, wt, one, zero, 3, 3, 1, 1, wt.shape[0], residual=gx, out=gx)

    def _dgrad(self, key, w, x: Act, g: Act, R, S, stride, pad):
        Cout, Cin = w.shape[0], w.shape[1]
        gx = self.grad_of(x)
        one, zero = self.const_vec(Cin, True), self.const_vec(Cin, False)
        if stride == 1:
            wt = self.weight_dgrad(w, Cout, Cin, R, S)
            self.conv(g, key + "#dgrad", wt, one, zero, R, S, 1, R - 1 - pad, Cin, residual=gx, out=gx)
        elif stride == 2 and R == 3 and S == 3 and pad == 1 and x.H == 2 * g.H and x.W == 2 * g.W:
            for ph in range(4):       # ConvTranspose2d(k3,s2,p1,op1) phases over w read as (Cin_t = Cout, Cout_t = Cin, 3, 3)
                a, b = ph >> 1, ph & 1
                self.conv(g, key + "#dgrad", w, one, zero, 1 + a, 1 + b, 1, 0, gx.Cphys, transposed=1, phase=ph, residual=gx,
                          ostr=(gx.coff + (a * gx.W + b) * gx.cstride, gx.H * gx.W * gx.cstride, 2 * gx.W * gx.cstride,
                                2 * gx.cstride, 1), out_tbuf=gx.tbuf, out_hw=(g.H, g.W))
        elif stride == 2 and R == 1 and S == 1 and pad == 0:
            wt = self.weight_dgrad(w, Cout, Cin, 1, 1)
            self.conv(g, key + "#dgrad", wt, one, zero, 1, 1, 1, 0, gx.Cphys, residual=gx,
                      ostr=(gx.coff, gx.H * gx.W * gx.cstride, 2 * gx.W * gx.cstride, 2 * gx.cstride, 1), out_tbuf=gx.tbuf,
                      out_hw=(g.H, g.W))
        else:
            raise RuntimeError("no data-gradient path for conv %s (k=%d, stride=%d, pad=%d)" % (key, R, stride, pad))

    def upsample2x_bwd(self, gout: Act, gin: Act):
        gt, it = gout.tbuf, gin.tbuf
        tail = (gin.B, gin.H, gin.W, gin.Cphys, gout.cstride, gout.coff, gin.cstride, gin.coff, 1)
        self._add(self.lib.cp_upsample2x_bilinear_ac_bwd, lambda P: (self.dtype, P(gt), P(it)) + tail, "upsample2x_bwd", [gt, it], [it])

    def fuse_sum_bwd(self, gout: Act, out: Act, gsrc: Act, shift, relu):
        gt, ot, st_ = gout.tbuf, out.tbuf, gsrc.tbuf
        tail = (gsrc.B, gsrc.H, gsrc.W, gsrc.Cphys, int(shift), 1 if relu else 0, 1)
        self._add(self.lib.cp_fuse_sum_act_bwd, lambda P: (self.dtype, P(gt), P(ot), P(st_)) + tail, "fuse_sum_bwd", [gt, ot, st_], [st_])

    def fuse_sum_bwd_group(self, members):
        """members: [(gout, out, gsrc, shift, relu)] writing DISTINCT gradient tensors (a module's whole fuse layer): one launch"""
        if len(members) == 1:
            for m in members:
                self.fuse_sum_bwd(*m)
            return
        lib, dt = self.lib, self.dtype
        for lo in range(0, len(members), 64):
            mem = members[lo:lo + 64]

            def argb(P, mem=mem):
                items, nbs = [], []
                for gout, out, gsrc, shift, relu in mem:
                    it, nb = CpFuseBwdItem(), C.c_uint32()
                    _abi.check(lib.cp_fuse_sum_act_bwd_item(dt, P(gout.tbuf), P(out.tbuf), P(gsrc.tbuf), gsrc.B, gsrc.H, gsrc.W, gsrc.Cphys,
                                                            int(shift), 1 if relu else 0, 1, C.byref(it), C.byref(nb)), "cp_fuse_sum_act_bwd_item")
                    items.append(it)
                    nbs.append(nb.value)
                return (dt,) + self._table(items, nbs)
            tbs = [t for gout, out, gsrc, _, _ in mem for t in (gout.tbuf, out.tbuf, gsrc.tbuf)]
            self._add(lib.cp_fuse_sum_act_bwd_group, argb, "fuse_sum_bwd_group:%d" % len(mem), tbs, [m[2].tbuf for m in mem])

    def maxpool_bwd(self, x: Act, gout: Act, gin: Act):
        xt, gt, it = x.tbuf, gout.tbuf, gin.tbuf
        assert x.coff == 0 and x.cstride == x.Cphys
        self._add(self.lib.cp_maxpool3x3s2_bwd, lambda P: (self.dtype, P(xt), P(gt), P(it), x.B, x.H, x.W, x.Cphys, 1),
                  "maxpool_bwd", [xt, gt, it], [it])

    def strided_to_act(self, src_ptr_fn, src_dtype, base, sb, sp, sc, out: Act, C_, reads=()):
        """strided tensor -> dense channels-last Act (out must be dense: coff 0, cstride == Cphys)"""
        assert out.coff == 0 and out.cstride == out.Cphys
        ot = out.tbuf
        HW = out.H * out.W
        self._add(self.lib.cp_strided_to_nhwc,
                  lambda P: (self.dtype, src_ptr_fn(P), src_dtype, base, sb, sp, sc, P(ot), out.B, HW, C_, out.Cphys),
                  "strided_to_nhwc", list(reads), [ot])

    # ---- train-mode EdgeConv
    def edge_weight_view(self, w, Co, Ci, mode):
        out = self.scratch_f32(2 * Co * Ci)
        self.keep.append(w)
        self.prep_item("views", lambda ref: self.lib.cp_pack_item_edge_view(w.data_ptr(), Co, Ci, mode, out.data_ptr(), ref), "edge_weight_view")
        return out.view(2 * Co, Ci, 1, 1) if mode == 0 else out.view(Ci, 2 * Co, 1, 1)

    def edge_train_fwd(self, pq: Act, graph, gamma, beta, rmean, rvar, out: Act, Co, slope, momentum=0.1, eps=1e-5):
        N = pq.W
        st_ = dict(scale=self.vec(Co), shift=self.vec(Co), mean=self.vec(Co), rstd=self.vec(Co), gamma=gamma,
                   kstar=torch.empty(pq.B * N * Co, dtype=torch.uint8, device=self.device),
                   ws=torch.empty(self.lib.cp_edge_train_workspace_bytes(pq.B, Co), dtype=torch.uint8, device=self.device))
        self.keep += [st_, gamma, beta, rmean, rvar]
        pt, ot = pq.tbuf, out.tbuf
        gp = graph["gids"].data_ptr() if graph["gids"] is not None else None
        a1 = (graph["idx"].data_ptr(), gp, gamma.data_ptr(), beta.data_ptr(), rmean.data_ptr(), rvar.data_ptr(), momentum, eps)
        a2 = (st_["kstar"].data_ptr(), st_["scale"].data_ptr(), st_["shift"].data_ptr(), st_["mean"].data_ptr(),
              st_["rstd"].data_ptr(), st_["ws"].data_ptr(), pq.B, N, graph["K"], Co, graph["G"], slope)
        self._add(self.lib.cp_edgeconv_train_fwd, lambda P: (self.dtype, P(pt)) + a1 + (P(ot), out.cstride, out.coff) + a2,
                  "edge_train_fwd", [pt], [ot])
        return st_

    def edge_train_bwd(self, pq: Act, graph, st_, out: Act, gout: Act, D: Act, dgamma_ptr, dbeta_ptr, Co, slope):
        N = pq.W
        pt, ot, gt, dt = pq.tbuf, out.tbuf, gout.tbuf, D.tbuf
        gp = graph["gids"].data_ptr() if graph["gids"] is not None else None
        a1 = (graph["idx"].data_ptr(), graph["rev_ptr"].data_ptr(), graph["rev_edge"].data_ptr(), gp)
        a3 = (st_["gamma"].data_ptr(), st_["mean"].data_ptr(), st_["rstd"].data_ptr())
        a4 = (dgamma_ptr, dbeta_ptr, st_["ws"].data_ptr(), pq.B, N, graph["K"], Co, graph["G"], slope)
        kp = st_["kstar"].data_ptr()
        self._add(self.lib.cp_edgeconv_train_bwd,
                  lambda P: (self.dtype, P(pt)) + a1 + (P(ot), out.cstride, out.coff, kp, P(gt), gout.cstride, gout.coff) + a3 +
                            (P(dt),) + a4, "edge_train_bwd", [pt, ot, gt], [dt])

    def index2feat_bwd(self, gout: Act, xid_t, yid_t, mask_t, dpatch_f32, N, Hp, Wp, E_ch, k):
        gt = gout.tbuf
        args = (xid_t.data_ptr(), yid_t.data_ptr(), mask_t.data_ptr(), dpatch_f32.data_ptr(), gout.B, N, Hp, Wp, E_ch, k,
                gout.cstride, gout.coff)
        self._add(self.lib.cp_index2feat_gather_bwd_t, lambda P: (self.dtype, P(gt)) + args, "index2feat_bwd", [gt], [])

    def finalize(self):
        for key, items in self.items.items():
            if not items:
                continue
            self.prep_tabs[key] = self._table(items, [(int(it.total) + 255) // 256 for it in items])
        self.acc_arena = torch.zeros(max(self.acc_total, 2), dtype=torch.float64, device=self.device)
        total = sum(t.nbytes for t in self.arena)
        self.grad_arena = torch.empty(max(total, 256), dtype=torch.uint8, device=self.device)
        off = 0
        for t in self.arena:
            t.fixed = self.grad_arena[off:off + t.nbytes]
            off += t.nbytes
        super().finalize()
        # op indices (launches + fork / sync / join markers) -> launch (call) indices, like everything bench_train reads
        call_of, n = [], 0                      # call_of[i] = launches among ops[:i]
        for op in self.ops:
            call_of.append(n)
            n += 0 if op[0] in MARKERS else 1
        call_of.append(n)
        self.pslot_done_call = {k: call_of[i] for k, i in self.pslot_done.items()}
        self.n_fwd_ops = call_of[self.n_fwd_ops]
        self.wgrad_flops = {call_of[i]: f for i, f in self.wgrad_flops.items()}
        return self

    def zero_grad_arena(self):
        """ONE zero fill of every activation-gradient buffer, at the start of the backward half"""
        self._add(self.lib.cp_memset_zero, lambda P: (self.grad_arena.data_ptr(), self.grad_arena.numel()), "grad_zero", [], [])

    # ---- tape
    def mark_forward_end(self):
        self.n_fwd_ops = len(self.ops)
        self.half = 1
        for kind in ("views", "packs"):
            self._add(self.lib.cp_pack_batch, (lambda k: lambda P: self._batch_args(k, 1))(kind), "prep_%s_bwd" % kind, [], [])

    def unwind(self):
        """append the backward launches; remember, per parameter, the op index after which its gradient is final"""
        for fn in reversed(self.tape):
            self._touched = []
            fn()
            for key in self._touched:
                self.pslot_done[key] = len(self.ops)
            self._wg_keys.update(self._touched)
        self.flush_wgrad()
        self.tape = []

    def gradient_buckets(self, nbuckets=4):
        """Cut the flat gradient buffer into ~equal contiguous buckets and the backward launches into as many segments, such
        that bucket k is final once segment k has run: [(call_lo, call_hi, elem_lo, elem_hi)], segments in launch order.  The
        backward runs head first, so the buffer's tail (decoder / refinement parameters) completes long before the
        backbone's -- its all-reduce can travel over xGMI under the remaining backward."""
        from .parallel import plan_gradient_buckets
        return plan_gradient_buckets(self.pslots, self.pgrad.numel(), self.pslot_done_call, self.n_fwd_ops, len(self.calls), nbuckets)

    def read_act(self, a: Act):
        """debug: the current contents of an activation / gradient view as a (B, H, W, C) fp32 CPU tensor"""
        dt = torch.bfloat16 if self.dtype == CP_BF16 else torch.float32
        es = 2 if self.dtype == CP_BF16 else 4
        n = a.B * a.H * a.W * a.cstride
        raw = a.tbuf.fixed if a.tbuf.fixed is not None else self.workspace[a.tbuf.offset:a.tbuf.offset + a.tbuf.nbytes]
        flat = raw[:n * es].view(dt).view(a.B, a.H, a.W, a.cstride)
        return flat[..., a.coff:a.coff + a.C].float().cpu()

    def run_range(self, stream_ptr, lo, hi):
        for fn, args, name in self.calls[lo:hi]:
            rc = fn(stream_ptr, *args[1:])
            if rc != 0:
                _abi.check(rc, name)
