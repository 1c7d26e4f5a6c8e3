"""Record of the C-ABI calls the conv autograd host path makes: tests/golden/conv_calls.json.

    python tests/golden/make_conv_calls.py

Pure Python, no GPU and no library: every scenario below drives the public entry points of
tpgan_ops (conv2d, conv2d_group, linear, conv2d_folded, ModificationLayer.ResidualBlock) on CPU
tensors with a recording stub in place of libtpgan_hip.so, and the file keeps the ledger of calls
the stub saw, in order.  It pins WHAT the Python side asks of the library -- descriptors, tensor
strides, aliasing, the number and order of planner queries -- so the host path can be restructured
against it.  Regenerate it only with a change that MEANS to move a call, and read the diff.
tests/test_conv_calls.py regenerates every scenario in memory and compares.

tpgan_ops is touched only through: load, tt, stream_ptr, _time_launches (a deterministic fake that
issues the launch once and reads its time from the scenario's table) and, of torch.cuda,
synchronize / is_current_stream_capturing / Event (tpgan_lib's loaded-library slot holds the stub
too, for check()'s error text); besides its public switches (AUTOTUNE, PACK,
FUSED_BWD, GROUP, ACT_LINK, PROBE, DATA_TUNE, GRAD_READY_HOOK) and the per-scenario start state
(_WS_BYTES and the tuning cache emptied, PACK["fallbacks"] zero).

Layout of the file:
  descs      the distinct masked descriptors; a call names one as "D<index>"
  scenarios  name -> list of calls [function, argument, ...] (+ "rc=<status>" when not 0)
Arguments by their C type:
  ConvDesc*  "D<k>": the fields THAT ENTRY POINT reads (READS below), the rest masked out
  TpgTensor  "<pointer name>:<dtype code>:<4 strides>", or "-" for a null tensor
  void* / other pointers   "P" (set) or "-" (null)
  scalars    their value (floats rounded to 6 digits)
Pointer names do not depend on the allocator: the replacement tt keeps every tensor it sees alive
for the scenario; a pointer inside a registered input / parameter / gradient buffer is named after
it, "+<byte offset>" where it is not the start; any other is t<k> in order of first appearance (the
whole storage of a tensor tt saw, so views of it read t<k>+<offset>).
Lines that start with "#" are host events in call order: "#ready <name>" (GRAD_READY_HOOK),
"#pack_run" (the jobs of the tpg_pack_run just recorded), "#state" (counters after the scenario).
"""
import contextlib
import ctypes
import json
import os
import struct
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "conv_calls.json")
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(HERE)), "tp-gan_amd"))

import torch  # noqa: E402

import tpgan_lib as L  # noqa: E402

GEOM = ("n", "in_c", "in_h", "in_w", "out_c", "out_h", "out_w", "kh", "kw", "stride_h", "stride_w", "pad_t", "pad_b",
        "pad_l", "pad_r", "pad_mode", "transposed")
BASE = GEOM + ("dtype", "act", "slope", "res_scale", "flags")
ALL = tuple(n for n, _ in L.ConvDesc._fields_)
_DATA = BASE + ("data_ksplit", "data_algo")
# the descriptor fields each entry point reads (include/tpgan.h)
READS = {"tpg_conv2d_fwd": _DATA, "tpg_conv2d_bwd_data": _DATA, "tpg_conv2d_workspace": _DATA,
         "tpg_conv2d_packed_bytes": _DATA, "tpg_conv2d_pack_jobs": _DATA,
         "tpg_conv2d_bwd_filter": BASE + ("algo", "ksplit"), "tpg_conv2d_bwd": ALL}
JB = 32  # the stub's pack job: <Q source, Q image, i op, i index, 8 bytes of padding>
WS_OVER_CAP = 300 << 20  # the stub's workspace answer for data_ksplit >= 16: past _DATA_SPLIT_WS_CAP
BF16, F32 = torch.bfloat16, torch.float32


def _num(v):
    return round(v, 6) if isinstance(v, float) else v


class Recorder:
    """The stub library of one scenario and its ledger."""

    def __init__(self, descs):
        self.calls, self.raw = [], []  # raw: (function, every descriptor field) per call with a descriptor
        self.descs = descs
        self.keep, self.ranges, self.anon = [], [], 0
        self.det = 0
        self.fail = None    # fn(name, desc fields or None) -> status to answer instead of 0
        self.times = None   # fn(name, desc fields, how often this launch was timed before) -> ms
        self.timed = {}

    # ---- pointer names
    def register(self, name, t):
        st = t.untyped_storage()
        self.ranges.append([st.data_ptr(), max(st.nbytes(), 1), name])
        self.keep.append(t)
        return t

    def _range(self, p):
        for r in self.ranges:
            if r[0] <= p < r[0] + r[1]:
                return r
        return None

    def seen(self, t):
        """(tt) keep t alive; its storage becomes a nameable range."""
        self.keep.append(t)
        st = t.untyped_storage()
        if self._range(t.data_ptr()) is None:
            self.ranges.append([st.data_ptr(), max(st.nbytes(), 1), None])

    def name(self, p):
        r = self._range(p)
        if r is None:
            r = [p, 1, None]
            self.ranges.append(r)
        if r[2] is None:
            r[2] = "t%d" % self.anon
            self.anon += 1
        return r[2] if p == r[0] else "%s+%d" % (r[2], p - r[0])

    # ---- the ledger
    def event(self, *what):
        self.calls.append(["#" + what[0]] + list(what[1:]))

    def _desc(self, fn, d):
        full = {f: _num(getattr(d, f)) for f in ALL}
        self.raw.append((fn, full))
        masked = {f: full[f] for f in READS.get(fn, BASE)}
        if masked not in self.descs:
            self.descs.append(masked)
        return "D%d" % self.descs.index(masked), full

    def _tensor(self, t):
        if not t.data:
            return "-"
        return "%s:%d:%s" % (self.name(t.data), t.dtype, ",".join(str(s) for s in t.stride))

    def record(self, fn, args):
        res, argtypes = L.EXPORTS[fn]
        row, full = [fn], None
        for a, ty in zip(args, argtypes):
            if ty is ctypes.POINTER(L.ConvDesc):
                s, full = self._desc(fn, a._obj)
                row.append(s)
            elif ty is L.TpgTensor:
                row.append(self._tensor(a))
            elif ty is ctypes.c_void_p or hasattr(ty, "contents"):
                null = a is None or a == 0 or (isinstance(a, ctypes.c_void_p) and not a.value)
                row.append("-" if null else "P")
            else:
                row.append(_num(a))
        self.calls.append(row)
        return row, full

    def __getattr__(self, fn):
        if fn not in L.EXPORTS:
            raise AttributeError(fn)

        def call(*args):
            if fn == "tpg_get_deterministic":  # (a host getter, asked before every workspace lookup: not a call
                return self.det                # worth pinning)
            if fn == "tpg_last_error":
                return b"stub"
            row, full = self.record(fn, args)
            if fn == "tpg_set_deterministic":
                self.det = args[0]
                return None
            if fn == "tpg_conv2d_workspace":
                return WS_OVER_CAP if full["data_ksplit"] >= 16 else 1024 + 64 * full["data_ksplit"]
            if fn == "tpg_conv2d_packed_bytes":
                return 64
            if fn == "tpg_pack_job_bytes":
                return JB
            if fn == "tpg_pack_prepare":
                return 3 * args[1]
            if fn == "tpg_conv2d_pack_jobs":
                n = 2 if args[1] == L.OP_BWD_DATA else 1
                for i in range(n):
                    args[4][i * JB:(i + 1) * JB] = struct.pack("<QQii8x", args[2].data, args[3], args[1], i)
                return n
            if fn == "tpg_pack_run":
                rawj = ctypes.string_at(args[0], args[1] * JB)
                jobs = [struct.unpack("<QQii8x", rawj[i * JB:(i + 1) * JB]) for i in range(args[1])]
                self.event("pack_run", [[self.name(s), self.name(im), op, i] for s, im, op, i in jobs])
                return 0
            rc = self.fail(fn, full) if self.fail is not None else 0
            if rc:
                row.append("rc=%d" % rc)
            return rc if L.EXPORTS[fn][0] is not None else None
        return call


class _Event:
    def __init__(self, enable_timing=False):
        pass

    def record(self):
        pass


@contextlib.contextmanager
def patched(ops, rec):
    """tpgan_ops on CPU tensors over rec's stub; every switch and counter put back on exit."""
    def cpu_tt(t):
        if t is None:
            return L.TpgTensor()
        rec.seen(t)
        d = L.TpgTensor()
        d.data, d.dtype = t.data_ptr(), L.dtype_code(t.dtype)
        for i, s in enumerate(t.stride()):
            d.stride[i] = s
        return d

    def timed(fn, reps=0):
        fn()  # (one real issue of the launch: the ledger shows the descriptor the trial ran with)
        name, full = rec.raw[-1]
        key = (name, full["algo"], full["ksplit"], full["data_ksplit"], full["data_algo"])
        k = rec.timed[key] = rec.timed.get(key, 0) + 1
        return rec.times(name, full, k - 1) if rec.times is not None else 1.0

    saved = [(ops, k, getattr(ops, k)) for k in ("load", "tt", "stream_ptr", "_time_launches")]
    saved += [(torch.cuda, k, getattr(torch.cuda, k)) for k in ("synchronize", "is_current_stream_capturing", "Event")]
    saved.append((L, "_lib", L._lib))
    L._lib = rec  # (tpgan_lib.check reads the failed call's message from the loaded library)
    dicts = [(dd, dict(dd)) for dd in (ops.AUTOTUNE, ops.PACK, ops.FUSED_BWD, ops.GROUP, ops.ACT_LINK, ops.PROBE,
                                       ops.DATA_TUNE, ops.RES_LINK)]
    hook, ws = ops.GRAD_READY_HOOK[0], dict(ops._WS_BYTES)
    ops.load, ops.tt, ops.stream_ptr, ops._time_launches = (lambda: rec), cpu_tt, (lambda: ctypes.c_void_p(7)), timed
    torch.cuda.synchronize = lambda *a: None
    torch.cuda.is_current_stream_capturing = lambda: False
    torch.cuda.Event = _Event
    # the scenario's start state
    ops._WS_BYTES.clear()
    ops.AUTOTUNE.update(enabled=False, cache={}, trials=0, frozen=False)
    ops.PACK.update(enabled=True, audit=None, fallbacks=0)
    ops.PROBE.update(match=None, events=[])
    ops.GRAD_READY_HOOK[0] = lambda p: rec.event("ready", rec.name(p.grad.data_ptr()))
    try:
        yield
    finally:
        for obj, k, v in saved:
            setattr(obj, k, v)
        for dd, old in dicts:
            dd.clear()
            dd.update(old)
        ops.GRAD_READY_HOOK[0] = hook
        ops._WS_BYTES.clear()
        ops._WS_BYTES.update(ws)


# ---- scenario helpers ---------------------------------------------------------------------
class Env:
    def __init__(self, ops, rec):
        self.ops, self.rec = ops, rec

    def act(self, name, n, c, h, w, dtype=F32, grad=True):
        """A registered channels-last activation (what the product allocates), zero-filled."""
        t = self.ops.new_act(n, c, h, w, dtype, "cpu")
        t.zero_()
        self.rec.register(name, t)
        return t.requires_grad_(grad)

    def weight(self, name, co, ci, k, grad=True, bias=True, transposed=False):
        w = torch.zeros(*((ci, co) if transposed else (co, ci)), k, k).contiguous(memory_format=torch.channels_last)
        self.rec.register(name, w)
        b = self.rec.register(name + ".b", torch.zeros(co)) if bias else None
        return w.requires_grad_(grad), (b.requires_grad_(grad) if b is not None else None)

    def flat(self, net):
        """FlatParams over net: its parameters and their gradients named flat.data / flat.grad."""
        import tpgan_train
        fl = tpgan_train.FlatParams(net, "cpu")
        self.rec.register("flat.data", fl.data)
        self.rec.register("flat.grad", fl.grad)
        return fl

    def state(self):
        ops = self.ops
        cache = sorted([list(map(str, k[:2] if k[0] == "dsplit" else k[:1])), list(v)] for k, v in
                       ops.AUTOTUNE["cache"].items())
        self.rec.event("state", {"fallbacks": ops.PACK["fallbacks"], "trials": ops.AUTOTUNE["trials"], "cache": cache,
                                 "ws_keys": len(ops._WS_BYTES), "probe_events": [e[3] for e in ops.PROBE["events"]]})


LEAKY = torch.nn.LeakyReLU(0.2)
P1 = (1, 1, 1, 1)


def _plain(E, dtype=F32, bias=True, residual=False, need=(True, True, True, True), act=LEAKY, stride=1, pad=P1,
           cin=8, cout=16, k=3, hw=6, transposed=False, output_padding=(0, 0), pad_mode=L.PAD_ZERO, nchw=False,
           concurrent=False, res_scale=1.0):
    """One conv2d forward + backward on unmanaged tensors."""
    ops = E.ops
    if nchw:
        x = E.rec.register("x", torch.zeros(2, cin, hw, hw)).requires_grad_(need[0])
    else:
        x = E.act("x", 2, cin, hw, hw, dtype, grad=need[0])
    w, b = E.weight("w", cout, cin, k, bias=bias, transposed=transposed)
    w.requires_grad_(need[1])
    if b is not None:
        b.requires_grad_(need[2])
    with ops.compute_dtype(dtype), ops.concurrent(concurrent):
        geom = ops.ConvGeom(k, k, (stride, stride), pad, pad_mode, transposed, output_padding)
        oh, ow = geom.out_hw(hw, hw)
        r = E.act("res", 2, cout, oh, ow, dtype, grad=need[3]) if residual else None
        y = ops.conv2d(x, w, b, stride=(stride, stride), pad=pad, pad_mode=pad_mode, act=act, residual=r,
                       res_scale=res_scale, transposed=transposed, output_padding=output_padding)
        if y.requires_grad:
            y.backward(E.act("gy", 2, cout, oh, ow, dtype, grad=False))
    E.state()


def _net(cin=8, cout=16, k=3, n=1, bias=True):
    torch.manual_seed(0)
    return torch.nn.Sequential(*[torch.nn.Conv2d(cin, cout, k, padding=k // 2, bias=bias) for _ in range(n)])


def _managed(E, passes=1, dtype=BF16, cin=8, cout=16, k=3, hw=6, x_grad=True, concurrent=False):
    """conv2d on a FlatParams-managed layer (fused dW / dbias targets, packed images), `passes` times."""
    ops = E.ops
    net = _net(cin, cout, k)
    E.flat(net)
    for i in range(passes):
        x = E.act("x%d" % i, 2, cin, hw, hw, dtype, grad=x_grad)
        with ops.compute_dtype(dtype), ops.concurrent(concurrent):
            y = ops.conv2d(x, net[0].weight, net[0].bias, pad=(k // 2,) * 4, act=LEAKY)
            y.backward(E.act("gy%d" % i, 2, cout, hw, hw, dtype, grad=False))
    E.state()


def _chain(E, link):
    """Producer conv + its only consumer (ActToken), fp32."""
    ops = E.ops
    ops.ACT_LINK["enabled"] = link
    x = E.act("x", 2, 8, 6, 6)
    w1, b1 = E.weight("w1", 16, 8, 3)
    w2, b2 = E.weight("w2", 8, 16, 3)
    h = ops.conv2d(x, w1, b1, pad=P1, act=LEAKY)
    y = ops.conv2d(h, w2, b2, pad=P1, act=torch.nn.ReLU(), act_in_ok=True)
    y.backward(E.act("gy", 2, 8, 6, 6, grad=False))
    E.state()


def _resblock(E, dtype):
    """ModificationLayer.ResidualBlock with an identity shortcut: the parked gradient is accepted."""
    import ModificationLayer as ML
    ops = E.ops
    torch.manual_seed(0)
    blk = ML.ResidualBlock(8, 8, kernel_size=3, activation=torch.nn.LeakyReLU(0.01))
    for i, p in enumerate(blk.parameters()):
        E.rec.register("p%d" % i, p.data)
    x = E.act("x", 2, 8, 6, 6, dtype)
    with ops.compute_dtype(dtype):
        y = blk(x)
        y.backward(E.act("gy", 2, 8, 6, 6, dtype, grad=False))
    E.state()


def _gradlink_mismatch(E):
    """A link whose parked gradient the first conv cannot accumulate into: the last conv ran in
    fp32, the first in bf16 (the dx + acc path)."""
    ops = E.ops
    link = ops.GradLink()
    x = E.act("x", 2, 8, 6, 6, BF16)
    w1, b1 = E.weight("w1", 8, 8, 3)
    w2, b2 = E.weight("w2", 8, 8, 3)
    with ops.compute_dtype(BF16):
        h = ops.conv2d(x, w1, b1, pad=P1, act=LEAKY, link_dx=link)
    y = ops.conv2d(h, w2, b2, pad=P1, act=LEAKY, residual=x, link_res=link)
    y.backward(E.act("gy", 2, 8, 6, 6, F32, grad=False))
    E.state()


def _second_order(E, managed):
    """create_graph=True, then a backward through the gradient (_ActMask / _ConvFwdPlain /
    _ConvDgrad / _ConvWgrad), with the weight's packed images (managed) or without."""
    ops = E.ops
    if managed:
        net = _net()
        E.flat(net)
        w, b = net[0].weight, net[0].bias
    else:
        w, b = E.weight("w", 16, 8, 3)
    x = E.act("x", 2, 8, 6, 6, BF16)
    with ops.compute_dtype(BF16), ops.act_links(False):
        y = ops.conv2d(x, w, b, pad=P1, act=LEAKY)
        (gx,) = torch.autograd.grad(y, x, E.act("gy", 2, 16, 6, 6, BF16, grad=False), create_graph=True)
        E.rec.event("second")
        gx.float().pow(2).sum().backward()
    E.state()


def _group(E, members, mode="fused"):
    ops = E.ops
    net = _net(n=members)
    E.flat(net)
    ops.GROUP["enabled"] = mode != "off"
    with ops.compute_dtype(BF16), ops.concurrent():
        xs = [E.act("x%d" % m, 2, 8, 6 + m, 6, BF16) for m in range(members)]
        outs = ops.conv2d_group([dict(x=x, weight=c.weight, bias=c.bias, pad=P1, act=LEAKY) for x, c in zip(xs, net)])
        gys = [E.act("gy%d" % m, 2, 16, 6 + m, 6, BF16, grad=False) for m in range(members)]
        if mode == "graph":
            with ops.act_links(False):
                gx = torch.autograd.grad(outs, xs, gys, create_graph=True)
                E.rec.event("second")
                sum(g.float().pow(2).sum() for g in gx).backward()
        else:
            torch.autograd.backward(outs, gys)
    E.state()


def _autotune(E, managed, frozen=False, margin=False):
    """Both tuners with the fake timer.  Forward: (4, 1) is fastest and wins (the plan and it are
    timed twice); with margin=True the plan's second trial comes within the margin and keeps its
    place.  Input gradient: (2, 2) wins.  data_ksplit 16 is past the workspace cap; the stub
    refuses (8, 2).  Weight gradient: algo 3 / split 2 wins, algos >= 6 answer -30.  A second pass
    hits the cache."""
    ops = E.ops
    ops.AUTOTUNE["enabled"], ops.AUTOTUNE["frozen"] = True, frozen

    def times(fn, d, again):
        cand = (d["data_ksplit"], d["data_algo"])
        if fn == "tpg_conv2d_fwd":
            if cand == (0, 0) and again and margin:
                return 0.92
            return 0.9 if cand == (4, 1) else 1.0 + 0.01 * cand[0]
        if fn == "tpg_conv2d_bwd":
            return 0.5 if cand == (2, 2) else 1.0
        return 0.7 if (d["algo"], d["ksplit"]) == (3, 2) else 1.0 + 0.1 * d["algo"]

    def fail(fn, d):
        if fn == "tpg_conv2d_bwd_filter" and d["algo"] >= 6:
            return -30
        if fn in ("tpg_conv2d_fwd", "tpg_conv2d_bwd") and (d["data_ksplit"], d["data_algo"]) == (8, 2):
            return -22
        return 0
    E.rec.times, E.rec.fail = times, fail
    if managed:
        _managed(E, passes=2)
    else:
        x = E.act("x", 2, 8, 6, 6, BF16)
        w, b = E.weight("w", 16, 8, 3)
        with ops.compute_dtype(BF16):
            for i in range(2):
                y = ops.conv2d(x, w, b, pad=P1, act=LEAKY)
                y.backward(E.act("gy%d" % i, 2, 16, 6, 6, BF16, grad=False))
        E.state()


def _autotune_three_calls(E):
    E.ops.FUSED_BWD["enabled"] = False
    _autotune(E, managed=True)


def _refused(E):
    """Every call that is handed a packed image answers -21: re-run with the fp32 weight."""
    E.rec.fail = lambda fn, d: -21 if d is not None and d["flags"] & L.FLAG_WPACKED else 0
    _managed(E)


def _probe(E):
    E.ops.PROBE["match"] = lambda d, which: which == "wgrad"
    _managed(E)


def _three_calls(E, **kw):
    E.ops.FUSED_BWD["enabled"] = False
    _plain(E, **kw)


def _three_calls_managed(E):
    E.ops.FUSED_BWD["enabled"] = False
    _managed(E)


def _linear(E):
    ops = E.ops
    w = E.rec.register("w", torch.zeros(10, 8 * 3 * 3)).requires_grad_(True)
    b = E.rec.register("w.b", torch.zeros(10)).requires_grad_(True)
    x4 = E.act("x4", 2, 8, 3, 3)
    ops.linear(x4, w, b, act=LEAKY).backward(E.rec.register("gy4", torch.zeros(2, 10)))
    x2 = E.rec.register("x2", torch.zeros(2, 72)).requires_grad_(True)
    ops.linear(x2, w, b).backward(E.rec.register("gy2", torch.zeros(2, 10)))
    ops.LINEAR_FLAT["enabled"] = False
    try:
        ops.linear(x4, w, b, act=LEAKY).backward(E.rec.register("gy4b", torch.zeros(2, 10)))
    finally:
        ops.LINEAR_FLAT["enabled"] = True
    E.state()


def _folded(E):
    """conv2d_folded on a 3-channel image: all taps folded (3x3) and the horizontal taps (7x7)."""
    ops = E.ops
    for k in (3, 7):
        x = E.rec.register("x%d" % k, torch.zeros(2, 3, 6, 6)).requires_grad_(True)
        w, b = E.weight("w%d" % k, 16, 3, k)
        y = ops.conv2d_folded(_as_device(x), w, b, (1, 1), (k // 2,) * 4, LEAKY)
        y.backward(E.act("gy%d" % k, 2, 16, 6, 6, grad=False))
    E.state()


class _OnDevice(torch.Tensor):
    """A CPU tensor that answers is_cuda: folded_args / linear ask it of their input before any call."""
    is_cuda = property(lambda self: True)

    @classmethod
    def __torch_function__(cls, func, types, args=(), kwargs=None):
        with torch._C.DisableTorchFunctionSubclass():
            return func(*args, **(kwargs or {}))


def _as_device(x):
    return x.as_subclass(_OnDevice)


def _linear_flat(E):
    ops = E.ops
    w = E.rec.register("w", torch.zeros(10, 8 * 3 * 3)).requires_grad_(True)
    b = E.rec.register("w.b", torch.zeros(10)).requires_grad_(True)
    x4 = E.act("x4", 2, 8, 3, 3)
    ops.linear(_as_device(x4), w, b, act=LEAKY).backward(E.rec.register("gy", torch.zeros(2, 10)))
    E.state()


SCENARIOS = [
    ("plain_f32", lambda E: _plain(E)),
    ("plain_bf16", lambda E: _plain(E, BF16)),
    ("no_bias_residual", lambda E: _plain(E, bias=False, residual=True, res_scale=0.5)),
    ("bias_residual_bf16", lambda E: _plain(E, BF16, residual=True)),
    ("no_act", lambda E: _plain(E, act=None)),
    ("no_dx", lambda E: _plain(E, need=(False, True, True, True))),
    ("no_dw", lambda E: _plain(E, need=(True, False, True, True), residual=True)),
    ("no_dbias", lambda E: _plain(E, BF16, need=(True, True, False, True))),
    ("transposed", lambda E: _plain(E, BF16, transposed=True, stride=2, output_padding=(1, 1), act=torch.nn.ReLU())),
    ("stride2", lambda E: _plain(E, stride=2)),
    ("reflect", lambda E: _plain(E, BF16, k=2, pad=(1, 0, 1, 0), pad_mode=L.PAD_REFLECT)),
    ("c1_input", lambda E: _plain(E, cin=1)),
    ("nchw_f32_input", lambda E: _plain(E, BF16, nchw=True)),
    ("concurrent", lambda E: _plain(E, BF16, concurrent=True)),
    ("act_link", lambda E: _chain(E, True)),
    ("act_link_off", lambda E: _chain(E, False)),
    ("gradlink_f32", lambda E: _resblock(E, F32)),
    ("gradlink_bf16", lambda E: _resblock(E, BF16)),
    ("gradlink_mismatch", _gradlink_mismatch),
    ("three_calls", lambda E: _three_calls(E, residual=True)),
    ("three_calls_bf16", lambda E: _three_calls(E, dtype=BF16, need=(True, True, True, True))),
    ("three_calls_managed", _three_calls_managed),
    ("second_order_packed", lambda E: _second_order(E, True)),
    ("second_order_unpacked", lambda E: _second_order(E, False)),
    ("managed", lambda E: _managed(E, passes=2)),
    ("managed_no_dx_concurrent", lambda E: _managed(E, x_grad=False, concurrent=True)),
    ("packed_refused", _refused),
    ("group2", lambda E: _group(E, 2)),
    ("group4", lambda E: _group(E, 4)),
    ("group2_off", lambda E: _group(E, 2, "off")),
    ("group2_graph", lambda E: _group(E, 2, "graph")),
    ("autotune_managed", lambda E: _autotune(E, True)),
    ("autotune_unmanaged_margin", lambda E: _autotune(E, False, margin=True)),
    ("autotune_three_calls", _autotune_three_calls),
    ("autotune_frozen", lambda E: _autotune(E, True, frozen=True)),
    ("probe_wgrad_split", _probe),
    ("linear", _linear),
    ("linear_flat", _linear_flat),
    ("folded", _folded),
]


def run_scenario(fn, descs=None):
    """-> (ledger, raw descriptors of its calls)."""
    import tpgan_ops
    rec = Recorder([] if descs is None else descs)
    with patched(tpgan_ops, rec):
        fn(Env(tpgan_ops, rec))
    return rec.calls, rec.raw


def generate():
    """-> ({"descs": [...], "scenarios": {name: ledger}}, {name: raw descriptors})."""
    descs, out, raws = [], {}, {}
    for name, fn in SCENARIOS:
        out[name], raws[name] = run_scenario(fn, descs)
    return {"descs": descs, "scenarios": out}, raws


def expand(doc, name):
    """A scenario's ledger with every "D<k>" replaced by the descriptor it names."""
    return [[doc["descs"][int(a[1:])] if isinstance(a, str) and a[:1] == "D" and a[1:].isdigit() else a for a in row]
            for row in doc["scenarios"][name]]


def dump(doc, path):
    with open(path, "w") as f:
        f.write('{"descs": [\n')
        f.write(",\n".join("  " + json.dumps(d, separators=(",", ":")) for d in doc["descs"]))
        f.write('\n ],\n "scenarios": {\n')
        f.write(",\n".join('  %s: [\n%s\n  ]' % (json.dumps(k), ",\n".join(
            "   " + json.dumps(r, separators=(",", ":")) for r in v)) for k, v in doc["scenarios"].items()))
        f.write("\n }\n}\n")


if __name__ == "__main__":
    doc, _ = generate()
    dump(doc, OUT)
    print(len(doc["scenarios"]), "scenarios,", sum(len(v) for v in doc["scenarios"].values()), "calls,",
          len(doc["descs"]), "descriptors,", os.path.getsize(OUT), "bytes")
