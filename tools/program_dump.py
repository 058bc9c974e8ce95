"""Canonical text of the launch programs the emitters build, for A/B-ing a host-side refactor of netbuilder.py / engine.py: two trees
emit the same programs exactly when this tool's output is byte-equal (`python tools/program_dump.py > a.txt` in each, then diff).

Per matrix row (PoseNet / woProg / InitNet x backbone x dtype x batch x kernel selection, eval and one training step) and per batch slice:
the sched list, workspace_bytes, flops, conv_log, then every call as `<C symbol> <recorder's name> lane=<k>` with its arguments --
pointers (told from integers by fn.argtypes) as `ws+<offset>` inside the program's workspace and `p<k>` (numbered by first
appearance) elsewhere, by-reference structs and arrays field by field under the same rules -- and the sha256 of every output
tensor of one run on det_image(B, seed=100) (training: deterministic mode, outputs + the parameter-gradient arena + every module
buffer after the step, i.e. the BatchNorm running statistics and counters).  A grouped launch (TABLES) is followed by its item table and
prefix table, read back from the device: every item field by field, each 64-bit word of an opaque parameter block as `ws+<offset>`,
`p<k>+<offset>` inside an allocation the program or the module holds, or the integer it is.  Last, the sorted set of C symbols launched
over the whole matrix: a recorder none of whose entry points is listed was not compared.

  --json FILE            also write {row: sha256 of the row's text}
  --rows TEXT            only the rows whose name contains TEXT
  --time-build N         instead of the dump: wall time of N program builds at B = 256 (bf16 PoseNet, first forward after invalidate())
  --time-build-train N   likewise for the training program: bf16 PoseNet, B = 32, first training step after invalidate()
"""
import argparse
import ctypes as C
import hashlib
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from checkerpose_amd import _abi, set_deterministic                          # noqa: E402
from checkerpose_amd.synthetic import build_net, build_woprog, det_image     # noqa: E402


class Canon:
    """pointer naming of one program"""

    def __init__(self, prog, held=()):
        ws = prog.workspace
        self.lo, self.hi, self.names = ws.data_ptr(), ws.data_ptr() + ws.numel(), {}
        self.allocs = sorted({(t.data_ptr(), t.data_ptr() + t.numel() * t.element_size()) for t in held if t.numel()})

    def ptr(self, v):
        v = getattr(v, "value", v)
        if not v:
            return "null"
        if self.lo <= v < self.hi:
            return "ws+%d" % (v - self.lo)
        return self.names.setdefault(v, "p%d" % len(self.names))

    def word(self, v):
        """one 64-bit word of an opaque parameter block: a pointer into the workspace or into a held allocation (the outermost one that
        contains it), else the integer"""
        v = int(v)
        if self.lo <= v < self.hi:
            return "ws+%d" % (v - self.lo)
        if v in self.names:
            return self.names[v] + "+0"
        for lo, hi in self.allocs:
            if lo <= v < hi:
                return "%s+%d" % (self.ptr(lo), v - lo)
        return str(v)

    def value(self, v, ctype=None):
        if hasattr(v, "_obj"):                                   # C.byref(x)
            return self.value(v._obj)
        if isinstance(v, C.Structure):
            return "{%s}" % ", ".join("%s=%s" % (n, self.value(getattr(v, n), t)) for n, t in v._fields_)
        if isinstance(v, C.Array) and v._type_ is C.c_uint64:    # an opaque block (CpBnItem.params, CpWgradItem.params)
            return "[%s]" % ", ".join(self.word(e) for e in v)
        if isinstance(v, C.Array):
            return "[%s]" % ", ".join(self.value(e, v._type_) for e in v)
        if ctype is C.c_void_p or isinstance(v, C.c_void_p):
            return self.ptr(v)
        if v is None:
            return "null"
        return repr(float(v)) if ctype is C.c_float or isinstance(v, float) else str(int(v))


SYMBOLS = set()          # every C entry point some dumped program launches


# grouped launches: C symbol -> (item type, position of the item-table pointer among the arguments behind the stream; the prefix-table
# pointer and the item count follow it)
TABLES = {"cp_bn_group": (_abi.CpBnItem, 2), "cp_wgrad_group": (_abi.CpWgradItem, 1), "cp_wgrad_reduce_batch": (_abi.CpWgradReduceItem, 0),
          "cp_fuse_sum_act_bwd_group": (_abi.CpFuseBwdItem, 1), "cp_pack_batch": (_abi.CpPackItem, 1)}


class _DeviceBytes:
    def __init__(self, ptr, n):
        self.__cuda_array_interface__ = {"shape": (n,), "typestr": "|u1", "data": (int(ptr), False), "version": 2}


def read_device(ptr, n, device):
    return torch.as_tensor(_DeviceBytes(ptr, n), device=device).cpu().numpy().tobytes()


def tensors_in(x, depth=0):
    """every tensor reachable from x through lists, tuples and dicts"""
    if torch.is_tensor(x):
        return [x]
    if isinstance(x, dict):
        x = list(x.values())
    if isinstance(x, (list, tuple)) and depth < 4:
        return [t for e in x for t in tensors_in(e, depth + 1)]
    return []


def held_tensors(prog, net):
    """the allocations opaque words may point into: what the program keeps alive, its arenas, the module's parameters and buffers"""
    held = tensors_in(list(prog.keep))
    for name in ("pgrad", "acc_arena", "grad_arena", "wg_ws"):
        held += tensors_in(getattr(prog, name, None))
    if net is not None:
        held += [t for t in net.state_dict(keep_vars=True).values() if t.is_cuda]
    return held


def dump_table(cn, fn, args, out, device):
    itype, at = TABLES[fn.__name__]
    raw, prefix, n = (getattr(a, "value", a) for a in args[at:at + 3])
    if not n:
        return
    size = C.sizeof(itype)
    blob = read_device(raw, n * size, device)
    for k in range(n):
        out.append("  item %d %s" % (k, cn.value(itype.from_buffer_copy(blob, k * size))))
    pre = (C.c_uint32 * (n + 1)).from_buffer_copy(read_device(prefix, 4 * (n + 1), device))
    out.append("  prefix %s" % (list(pre),))


def dump_program(prog, out, net=None):
    SYMBOLS.update(fn.__name__ for fn, _, _ in prog.calls)
    lane_of = {item[1]: item[2] for item in prog.sched if item[0] == "op"}
    out.append("sched %r" % (prog.sched,))
    out.append("workspace_bytes %d flops %d" % (prog.workspace_bytes, prog.flops))
    out.append("conv_log %r" % (list(prog.conv_log),))
    cn = Canon(prog, held_tensors(prog, net))
    for i, (fn, args, name) in enumerate(prog.calls):
        types = list(fn.argtypes)[1:]                            # [0]: the stream
        assert len(types) == len(args) - 1, (fn.__name__, len(types), len(args))
        out.append("%s %s lane=%d (%s)" % (fn.__name__, name, lane_of[i], ", ".join(cn.value(a, t) for a, t in zip(args[1:], types))))
        if fn.__name__ in TABLES:
            dump_table(cn, fn, args[1:], out, prog.workspace.device)


def sha(t):
    return hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()


def tensors_of(res):
    if torch.is_tensor(res):
        return [res]
    return [t for r in res for t in tensors_of(r)] if isinstance(res, (tuple, list)) else []


def obj_ids(B, dev):
    return torch.tensor([(3 * i) % 13 + 1 for i in range(B)], device=dev)


def call(net, img, lm, stage=None):
    if not hasattr(net, "init_net"):                             # InitNet alone
        return net(img, obj_ids(img.shape[0], img.device)) if lm else net(img)
    if lm:
        return net(img, None, obj_ids(img.shape[0], img.device), stage=stage)
    return net(img, None, stage=stage)


def eval_row(make, dtype, B, lm=False, stage=None, selection="auto"):
    dev = torch.device("cuda:0")
    out = []
    with torch.no_grad():
        net = make().to(dev)
        net.set_compute_dtype(dtype)
        net.set_kernel_selection(selection)
        res = call(net, det_image(B, seed=100).to(dev), lm, stage)       # builds the program, runs it once (eagerly)
        torch.cuda.synchronize()
        for k, sub in enumerate(net.program_for(B, stage).progs):
            out.append("slice %d" % k)
            dump_program(sub, out)
    out += ["out%d %s" % (k, sha(t)) for k, t in enumerate(tensors_of(res))]
    return out


# the smallest power of two (MB) of CHECKERPOSE_AMD_WGRAD_ARENA_MB at which the fp32 PoseNet training program builds at B = 2 (found on the
# commit before the trainer refactor: 32 raises "arena is smaller than ..."): the backward runs out of arena and settles in instalments
SMALL_ARENA_MB = 64


def train_row(make, lm, dtype=None, env=None):
    dev = torch.device("cuda:0")
    B, out = 2, []
    saved = {k: os.environ.get(k) for k in (env or {})}
    os.environ.update(env or {})
    set_deterministic(True)
    try:
        net = make().to(dev).train()
        if dtype is not None:
            net.set_compute_dtype(dtype)
        with torch.enable_grad():
            res = call(net, det_image(B, seed=100).to(dev), lm)
            ts = [t for t in tensors_of(res) if t.requires_grad]
            torch.autograd.backward(ts, [torch.ones_like(t) for t in ts])
        torch.cuda.synchronize()
        pr = list(net._train_programs.values())[-1]              # (no public accessor: program_for lists the eval programs)
        out.append("n_fwd_ops %d" % pr["prog"].n_fwd_ops)
        dump_program(pr["prog"], out, net)
        out += ["out%d %s" % (k, sha(t)) for k, t in enumerate(tensors_of(res))]
        out.append("pgrad %s" % sha(pr["pgrad"]))
        out += ["buffer %s %s" % (k, sha(t)) for k, t in net.named_buffers()]
    finally:
        set_deterministic(False)
        for k, v in saved.items():
            os.environ.pop(k) if v is None else os.environ.__setitem__(k, v)
    return out


def matrix():
    pose, wop = (lambda: build_net(512)), build_woprog
    rows = []
    for B in (2, 64):
        rows.append(("posenet bf16 B=%d" % B, lambda B=B: eval_row(pose, "bf16", B)))
    rows.append(("posenet fp32 B=2", lambda: eval_row(pose, "fp32", 2)))
    rows.append(("posenet bf16 B=2 stage=1", lambda: eval_row(pose, "bf16", 2, stage=1)))
    for sel in ("per_crop", "tiled"):
        rows.append(("posenet bf16 B=2 %s" % sel, lambda sel=sel: eval_row(pose, "bf16", 2, selection=sel)))
    for B in (2, 64):
        rows.append(("woprog bf16 B=%d" % B, lambda B=B: eval_row(wop, "bf16", B, lm=True)))
    rows.append(("woprog fp32 B=2", lambda: eval_row(wop, "fp32", 2, lm=True)))
    rows.append(("posenet graph=0 bf16 B=2", lambda: eval_row(lambda: build_net(512, graph=0), "bf16", 2)))
    # N = 4096: the patch-ordered rows and the permutes; the tiled EdgeConv itself needs B * N / 512 workgroups to fill the chip, which
    # at B = 2 only the pinned per-crop selection grants
    lm4096 = []                                                  # one net for both rows: its patch schedule is host work of seconds

    def lm_net():
        if not lm4096:
            lm4096.append(build_net(4096, lm=True))
        return lm4096[0]
    for sel in ("auto", "per_crop"):
        rows.append(("posenet lm N=4096 bf16 B=2 %s" % sel, lambda sel=sel: eval_row(lm_net, "bf16", 2, lm=True, selection=sel)))
    rows.append(("initnet bf16 B=2", lambda: eval_row(lambda: build_net(512, full=False), "bf16", 2)))
    # the other backbones: maxpool, the unfused basic_block and the fp32 small-Cout halo rule (resnet34), the small HRNet's branches
    for dt in ("bf16", "fp32"):
        rows.append(("posenet resnet34 %s B=2" % dt, lambda dt=dt: eval_row(lambda: build_net(512, backbone="resnet34"), dt, 2)))
    rows.append(("posenet hrnet_w18_small bf16 B=2 per_crop",
                 lambda: eval_row(lambda: build_net(512, backbone="hrnet_w18_small"), "bf16", 2, selection="per_crop")))
    rows.append(("posenet bf16 B=96", lambda: eval_row(pose, "bf16", 96)))      # the smallest batch at which auto takes hr_stem and edge_fused
    rows.append(("posenet train fp32 B=2", lambda: train_row(pose, False)))
    rows.append(("woprog train fp32 B=2", lambda: train_row(wop, True)))
    # the training recorders' other paths: the bf16 weight-gradient kind and BatchNorm items; max-pool backward and the ungrouped basic
    # blocks; the small HRNet; every weight gradient launched alone (cp_conv2d_wgrad_deferred); a weight-gradient arena that fills up
    # in mid-backward (cp_wgrad_reduce_batch in instalments)
    rows.append(("posenet train bf16 B=2", lambda: train_row(pose, False, "bf16")))
    rows.append(("posenet resnet34 train fp32 B=2", lambda: train_row(lambda: build_net(512, backbone="resnet34"), False)))
    rows.append(("posenet hrnet_w18_small train fp32 B=2", lambda: train_row(lambda: build_net(512, backbone="hrnet_w18_small"), False)))
    rows.append(("posenet train fp32 B=2 wgrad alone", lambda: train_row(pose, False, env={"CHECKERPOSE_AMD_WGRAD_GROUP_GFLOP": "0"})))
    rows.append(("posenet train fp32 B=2 arena %d MB" % SMALL_ARENA_MB,
                 lambda: train_row(pose, False, env={"CHECKERPOSE_AMD_WGRAD_ARENA_MB": str(SMALL_ARENA_MB)})))
    return rows


def time_build(n):
    dev = torch.device("cuda:0")
    with torch.no_grad():
        net = build_net(512).to(dev).set_compute_dtype("bf16")
        img = det_image(256, seed=100).to(dev)
        net(img, None)                                           # library load, allocator warm-up
        secs = []
        for _ in range(n):
            net.invalidate()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            net(img, None)
            torch.cuda.synchronize()
            secs.append(time.perf_counter() - t0)
            assert net.program_for(256) is not None
    print(json.dumps({"program_build_b256_seconds": secs}))


def time_build_train(n):
    dev = torch.device("cuda:0")
    net = build_net(512).to(dev).train().set_compute_dtype("bf16")
    img = det_image(32, seed=100).to(dev)

    def step():
        with torch.enable_grad():
            ts = [t for t in tensors_of(net(img, None)) if t.requires_grad]
            torch.autograd.backward(ts, [torch.ones_like(t) for t in ts])
        torch.cuda.synchronize()
    step()                                                       # library load, allocator warm-up
    secs = []
    for _ in range(n):
        net.invalidate()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        step()
        secs.append(time.perf_counter() - t0)
        assert len(net._train_programs) == 1
    print(json.dumps({"train_program_build_b32_seconds": secs}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json")
    ap.add_argument("--time-build", type=int, default=0)
    ap.add_argument("--time-build-train", type=int, default=0)
    ap.add_argument("--rows", help="only the rows whose name contains this text")
    a = ap.parse_args()
    if a.time_build:
        return time_build(a.time_build)
    if a.time_build_train:
        return time_build_train(a.time_build_train)
    digests = {}
    for name, row in matrix():
        if a.rows and a.rows not in name:
            continue
        text = "\n".join(["==== " + name] + row()) + "\n"
        sys.stdout.write(text)
        sys.stdout.flush()
        digests[name] = hashlib.sha256(text.encode()).hexdigest()
    print("==== C symbols launched\n" + "\n".join(sorted(SYMBOLS)))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(digests, f, indent=1)


if __name__ == "__main__":
    main()
