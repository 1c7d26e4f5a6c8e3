"""CPU: the host bookkeeping of the pre-packed weight images (tpgan_ops._pack_entry /
_packed_weight / repack / repack_range, FlatParams.adam_* / relayout / weights_loaded).

The bookkeeping is driven on a real FlatParams over CPU tensors with a stub in place of the
library: the stub's pack jobs are fixed bytes that name the job's source pointer, image pointer
and op, and its tpg_pack_run reads the job table it is handed, so every test sees exactly which
images a launch would have re-packed and from which fp32 source.

The last tests use the real library's host-side planner (no device work): the pack jobs of a
shape do not depend on TPG_FLAG_CONCURRENT, data_algo or data_ksplit, which is why the entry key
leaves them out (tests/test_gpu_pack.py holds the same on the device: images bit for bit, and
results with every plan forced at use time)."""
import ctypes
import struct

import pytest
import torch

import tpgan_lib as L

JB = 32  # the stub's job size: <Q source, Q image, i op, i index within the entry, 8 bytes of padding>


class StubLib:
    def __init__(self):
        self.runs = []  # one list of (source, image, op, index) per tpg_pack_run
        self.adam = 0

    def tpg_get_deterministic(self):
        return 0

    def tpg_conv2d_packed_bytes(self, dref, op):
        return 0 if dref._obj.in_c == 1 else 64  # (a 1-channel input stands for "no packed form")

    def tpg_pack_job_bytes(self):
        return JB

    def tpg_conv2d_pack_jobs(self, dref, op, w, image, host, max_jobs):
        n = 2 if op == L.OP_BWD_DATA else 1
        for i in range(n):
            host[i * JB:(i + 1) * JB] = struct.pack("<QQii8x", w.data, image, op, i)
        return n

    def tpg_pack_prepare(self, host, n):
        return 3 * n

    def tpg_pack_run(self, table, n, nblocks, stream):
        assert nblocks == 3 * n
        raw = ctypes.string_at(table, n * JB)
        self.runs.append([struct.unpack("<QQii8x", raw[i * JB:(i + 1) * JB]) for i in range(n)])
        return 0

    def tpg_adam(self, *args):
        self.adam += 1
        return 0


def _cpu_tt(t):
    d = L.TpgTensor()
    d.data = t.data_ptr()
    d.dtype = L.dtype_code(t.dtype)
    for i, s in enumerate(t.stride()):
        d.stride[i] = s
    return d


@pytest.fixture
def env(monkeypatch):
    """(tpgan_ops, tpgan_train, stub library, [current stream id]) with the library, tt and
    stream_ptr of tpgan_ops replaced; the audit ledger is on."""
    import tpgan_ops
    import tpgan_train
    stub = StubLib()
    stream = [7]
    monkeypatch.setattr(tpgan_ops, "load", lambda: stub)
    monkeypatch.setattr(tpgan_ops, "tt", _cpu_tt)
    monkeypatch.setattr(tpgan_ops, "stream_ptr", lambda: ctypes.c_void_p(stream[0]))
    monkeypatch.setitem(tpgan_ops.PACK, "audit", [])
    monkeypatch.setitem(tpgan_ops.PACK, "enabled", True)
    return tpgan_ops, tpgan_train, stub, stream


def _net():
    torch.manual_seed(0)
    return torch.nn.Sequential(torch.nn.Conv2d(8, 16, 3, padding=1), torch.nn.Conv2d(16, 8, 3, padding=1),
                               torch.nn.Conv2d(8, 8, 1), torch.nn.Conv2d(8, 8, 1))


def _desc(p, n=2, hw=6, flags=0, data_algo=0, data_ksplit=0):
    cout, cin, k, _ = p.shape
    d = L.ConvDesc()
    d.n, d.in_c, d.in_h, d.in_w, d.out_c, d.out_h, d.out_w = n, cin, hw, hw, cout, hw, hw
    d.kh = d.kw = k
    d.stride_h = d.stride_w = 1
    d.pad_t = d.pad_b = d.pad_l = d.pad_r = k // 2
    d.dtype = L.TPG_BF16
    d.flags, d.data_algo, d.data_ksplit = flags, data_algo, data_ksplit
    return d


def _weights(net):
    return [m.weight for m in net]


def _use(ops, p, op=L.OP_FWD, **kw):
    return ops._packed_weight(p, _desc(p, **kw), op, p.data)


def _entries(flat):
    return {k: e for k, e in flat.pack_entries.items() if e is not None}


def _sources(run):
    return sorted((src, op, i) for src, _, op, i in run)


def _jobs_of(entries):
    return sorted((e.src, e.op, i) for e in entries for i in range(e.njobs))


def test_lazy_pack_once_and_ledger(env):
    ops, train, stub, stream = env
    net = _net()
    flat = train.FlatParams(net, "cpu")
    w0 = _weights(net)[0]
    buf = _use(ops, w0)
    assert buf is not None and buf.numel() == 64
    assert stub.runs == [[(w0.data_ptr(), buf.data_ptr(), L.OP_FWD, 0)]]
    stream[0] = 9
    assert _use(ops, w0) is buf and len(stub.runs) == 1  # current: read, not packed again
    (key, e), = _entries(flat).items()
    assert (e.op, e.src, e.strides, e.shape) == (L.OP_FWD, w0.data_ptr(), tuple(w0.stride()), tuple(w0.shape))
    assert ops.PACK["audit"] == [("lazy", key, 7, 0, 0), ("read", key, 7, 0, 0), ("read", key, 9, 0, 0)]
    # fp32 compute, an unmanaged weight and PACK off take no image (and leave no ledger line)
    d32 = _desc(w0)
    d32.dtype = L.TPG_F32
    assert ops._packed_weight(w0, d32, L.OP_FWD, w0.data) is None
    assert ops._packed_weight(torch.nn.Parameter(w0.detach().clone()), _desc(w0), L.OP_FWD, w0.data) is None
    ops.PACK["enabled"] = False
    assert _use(ops, w0) is None
    assert len(ops.PACK["audit"]) == 3 and len(stub.runs) == 1


def test_entry_keeps_the_descriptor_it_was_planned_with(env):
    ops, train, stub, _ = env
    net = _net()
    flat = train.FlatParams(net, "cpu")
    w0 = _weights(net)[0]
    d = _desc(w0, flags=L.FLAG_CONCURRENT, data_algo=2, data_ksplit=5)
    ops._packed_weight(w0, d, L.OP_BWD_DATA, w0.data)
    d.flags, d.data_algo, d.data_ksplit, d.n = 0, 0, 0, 99  # the caller goes on changing its own descriptor
    (e,) = _entries(flat).values()
    assert (e.desc.flags, e.desc.data_algo, e.desc.data_ksplit, e.desc.n) == (L.FLAG_CONCURRENT, 2, 5, 2)
    assert e.op == L.OP_BWD_DATA and e.njobs == 2


def test_plan_fields_share_one_entry(env):
    """Descriptors that differ only in CONCURRENT / data_algo / data_ksplit share an entry: the C
    side's pack plan (PackArgs, halo nks / BN / ntiles / half, region sizes) follows shape and
    dtype alone -- test_pack_jobs_ignore_plan_fields below on the real planner,
    tests/test_gpu_pack.py::test_prepacked_plan_cross on the device."""
    ops, train, stub, _ = env
    net = _net()
    flat = train.FlatParams(net, "cpu")
    w0 = _weights(net)[0]
    a = _use(ops, w0)
    assert _use(ops, w0, flags=L.FLAG_CONCURRENT) is a
    assert _use(ops, w0, data_algo=2) is a
    assert _use(ops, w0, data_ksplit=4) is a
    assert len(_entries(flat)) == 1 and len(stub.runs) == 1
    assert _use(ops, w0, n=4) is not a  # (the shape is in the key)
    assert len(_entries(flat)) == 2


def test_entry_created_after_table_joins_next_batched_launch(env):
    ops, train, stub, _ = env
    net = _net()
    flat = train.FlatParams(net, "cpu")
    w = _weights(net)
    _use(ops, w[0])
    _use(ops, w[0], L.OP_BWD_DATA)
    flat.epoch += 1
    ops.repack(flat)
    assert _sources(stub.runs[-1]) == _jobs_of(_entries(flat).values()) and len(stub.runs[-1]) == 3
    table = flat.pack_table
    flat.epoch += 1
    ops.repack(flat)
    assert flat.pack_table is table and len(stub.runs[-1]) == 3  # (unchanged entries: the table is reused)
    # a new entry after the table was built: packed lazily now, in the batched launch from then on
    _use(ops, w[1])
    late = [e for e in _entries(flat).values() if e.src == w[1].data_ptr()]
    assert len(late) == 1 and flat.pack_table is None and _sources(stub.runs[-1]) == _jobs_of(late)
    flat.epoch += 1
    assert all(e.epoch != flat.epoch for e in _entries(flat).values())
    ops.repack(flat)
    assert len(stub.runs[-1]) == 4 and _sources(stub.runs[-1]) == _jobs_of(_entries(flat).values())
    assert all(e.epoch == flat.epoch for e in _entries(flat).values())
    n = len(stub.runs)
    for p, op in ((w[0], L.OP_FWD), (w[0], L.OP_BWD_DATA), (w[1], L.OP_FWD)):
        _use(ops, p, op)
    assert len(stub.runs) == n  # all current: no lazy pack
    # a shape without a packed form leaves a None entry that no launch counts
    one = torch.nn.Conv2d(1, 8, 3, padding=1)
    f1 = train.FlatParams(one, "cpu")
    assert _use(ops, one.weight) is None and list(f1.pack_entries.values()) == [None]
    ops.repack(f1)
    assert len(stub.runs) == n


def test_entry_created_after_range_table_joins_next_range_launch(env):
    ops, train, stub, _ = env
    net = _net()
    flat = train.FlatParams(net, "cpu")
    w = _weights(net)
    total = flat.data.numel()
    _use(ops, w[0])
    ops.repack_range(flat, 0, total, 1)
    assert _sources(stub.runs[-1]) == [(w[0].data_ptr(), L.OP_FWD, 0)]
    _use(ops, w[2], L.OP_BWD_DATA)  # after the range table was built
    ops.repack_range(flat, 0, total, 2)
    assert _sources(stub.runs[-1]) == _jobs_of(_entries(flat).values()) and len(stub.runs[-1]) == 3
    assert all(e.epoch == 2 for e in _entries(flat).values())


def test_repack_range_partition_marks_every_entry_once(env):
    ops, train, stub, _ = env
    net = _net()
    flat = train.FlatParams(net, "cpu")
    w = _weights(net)
    for p in w:
        _use(ops, p)
        _use(ops, p, L.OP_BWD_DATA)
    entries = _entries(flat)
    assert len(entries) == 8
    offs = {p.data_ptr(): (p.data_ptr() - flat.data.data_ptr()) // 4 for p in w}
    total = flat.data.numel()
    o1, o2 = offs[w[1].data_ptr()], offs[w[2].data_ptr()]
    # cuts: on w[1]'s first element (w[1] goes right), one element into w[2] (w[2] stays left: a
    # weight belongs to the range that holds its first element), and inside w[3]
    cuts = [0, o1, o2 + 1, offs[w[3].data_ptr()] + 5, total]
    want = [[w[0]], [w[1], w[2]], [w[3]], []]
    ops.PACK["audit"].clear()
    n0 = len(stub.runs)
    for (a, b), ps in zip(zip(cuts, cuts[1:]), want):
        before = len(stub.runs)
        ops.repack_range(flat, a, b - a, 5)
        es = [e for e in entries.values() if e.src in [p.data_ptr() for p in ps]]
        if es:
            assert _sources(stub.runs[-1]) == _jobs_of(es), (a, b)
        else:
            assert len(stub.runs) == before  # (no entry starts here: no launch)
    assert len(stub.runs) == n0 + 3
    marks = [ev[1] for ev in ops.PACK["audit"] if ev[0] == "range"]
    assert sorted(marks, key=repr) == sorted(entries, key=repr)  # every entry exactly once
    assert all(e.epoch == 5 for e in entries.values())
    assert all(ev == ("range", ev[1], 7, flat.epoch, 5) for ev in ops.PACK["audit"])
    # the boundary rule itself: one element to either side moves w[1]
    ops.repack_range(flat, 0, o1 + 1, 6)
    assert sorted(e.src for e in entries.values() if e.epoch == 6) == sorted([w[0].data_ptr(), w[1].data_ptr()] * 2)
    ops.repack_range(flat, 0, o1, 7)
    assert sorted(e.src for e in entries.values() if e.epoch == 7) == [w[0].data_ptr()] * 2


def test_bucketed_adam_withheld_range_is_packed_lazily_once(env):
    ops, train, stub, _ = env
    net = _net()
    flat = train.FlatParams(net, "cpu")
    w = _weights(net)
    for p in w:
        _use(ops, p)
    base = flat.data.data_ptr()
    starts = [(p.data_ptr() - base) // 4 for p in w] + [flat.data.numel()]
    spans = [(starts[i], starts[i + 1] - starts[i]) for i in range(4)]  # (a weight and its bias each)
    flat.adam_begin()
    for i in (0, 1, 3):  # the third range is withheld
        flat.adam_bucket(spans[i][0], spans[i][1], 1e-4)
    flat.adam_end()
    assert stub.adam == 4  # (the step counter's launch and three slices)
    by_src = {e.src: e for e in _entries(flat).values()}
    assert [by_src[p.data_ptr()].epoch == flat.epoch for p in w] == [True, True, False, True]
    n = len(stub.runs)
    ops.PACK["audit"].clear()
    for p in w:
        _use(ops, p)
    assert len(stub.runs) == n + 1 and _sources(stub.runs[-1]) == [(w[2].data_ptr(), L.OP_FWD, 0)]
    for p in w:
        _use(ops, p)
    assert len(stub.runs) == n + 1
    assert [ev[0] for ev in ops.PACK["audit"]].count("lazy") == 1
    assert all(e.epoch == flat.epoch for e in by_src.values())


def test_whole_adam_and_weights_loaded_repack_everything(env):
    ops, train, stub, _ = env
    net = _net()
    flat = train.FlatParams(net, "cpu")
    w = _weights(net)
    for p in w:
        _use(ops, p)
        _use(ops, p, L.OP_BWD_DATA)
    for update in (lambda: flat.adam(1e-4), flat.weights_loaded):
        ep = flat.epoch
        n = len(stub.runs)
        update()
        assert flat.epoch == ep + 1 and len(stub.runs) == n + 1
        assert _sources(stub.runs[-1]) == _jobs_of(_entries(flat).values()) and len(stub.runs[-1]) == 12
        assert all(e.epoch == flat.epoch for e in _entries(flat).values())


def test_relayout_and_moved_weight_never_hit_an_old_entry(env):
    ops, train, stub, _ = env
    net = _net()
    flat = train.FlatParams(net, "cpu")
    w = _weights(net)
    for p in w:
        _use(ops, p)
    old = dict(_entries(flat))
    old_data = flat.data
    flat.adam(1e-4)
    version = flat.pack_version
    flat.relayout(list(reversed(range(len(flat.params)))))
    assert flat.pack_entries == {} and flat.pack_table is None and flat.pack_version > version
    n = len(stub.runs)
    ops.repack(flat)  # nothing to re-pack: in particular not the dropped entries' jobs
    assert len(stub.runs) == n
    for p in w:
        buf = _use(ops, p)
        assert all(buf is not e.buf for e in old.values())
        src, image, op, _ = stub.runs[-1][0]
        assert (src, image) == (p.data_ptr(), buf.data_ptr())
        assert flat.data.data_ptr() <= src < flat.data.data_ptr() + 4 * flat.data.numel()
    assert len(stub.runs) == n + 4
    assert not set(old) & set(flat.pack_entries)
    lo, hi = old_data.data_ptr(), old_data.data_ptr() + 4 * old_data.numel()
    assert not any(lo <= e.src < hi for e in _entries(flat).values())
    # one parameter re-bound to another place of the same buffer (same shape, same strides): the
    # data pointer is in the key, so the image of the old place is not handed out for the new one
    a, b = w[2], w[3]
    buf_a = _use(ops, a)
    a.data = b.data
    buf_moved = _use(ops, a)
    assert buf_moved is not buf_a and buf_moved is _use(ops, b)


def test_source_outside_flat_buffer_is_refused(env):
    ops, train, stub, _ = env
    net = _net()
    flat = train.FlatParams(net, "cpu")
    w = _weights(net)
    _use(ops, w[1])
    # a managed parameter whose storage is not the flat buffer (a clone, an .to() copy)
    w[0].data = w[0].data.clone()
    with pytest.raises(RuntimeError, match=r"op 0, weight \(16, 8, 3, 3\).*outside the flat"):
        _use(ops, w[0])
    assert len(_entries(flat)) == 1 and len(stub.runs) == 1
    # the last element counts: a weight that ends exactly at the buffer's end passes, the same
    # weight against a buffer one element shorter does not
    last = torch.nn.Conv2d(8, 8, 1, bias=False)
    f2 = train.FlatParams(last, "cpu")
    assert _use(ops, last.weight) is not None
    f2.data = f2.data[:-1]
    with pytest.raises(RuntimeError, match=r"op 1, weight \(8, 8, 1, 1\).*outside the flat"):
        _use(ops, last.weight, L.OP_BWD_DATA)
    # the buffers replaced under live entries (what relayout() would be without dropping them)
    flat.data = torch.zeros_like(flat.data)
    flat.epoch += 1
    with pytest.raises(RuntimeError, match=r"op 0, weight \(8, 16, 3, 3\).*outside the flat"):
        ops.repack(flat)
    with pytest.raises(RuntimeError, match="outside the flat"):
        ops.repack_range(flat, -(1 << 60), 1 << 61, flat.epoch)
    assert len(stub.runs) == 2  # (the two lazy packs that were in order; no refused entry launched anything)


def test_frozen_holder_has_no_buffer_to_check(env):
    ops, _, stub, _ = env
    w = torch.randn(8, 8, 3, 3)
    w._tpg_flat = ops._FrozenPack()
    buf = ops._packed_weight(w, _desc(w), L.OP_FWD, w)
    assert buf is not None and ops._packed_weight(w, _desc(w), L.OP_FWD, w) is buf and len(stub.runs) == 1


# ---- the real host-side planner -----------------------------------------------------------------
# (n, cin, h, w, cout, k, stride, pad (t, b, l, r), reflect, transposed, output_padding): the
# geometries of tests/test_gpu_pack.py
PLAN_GEOMS = [
    (2, 75, 24, 40, 75, 7, 1, (3,) * 4, False, False, 0),
    (2, 206, 16, 24, 206, 5, 1, (2,) * 4, False, False, 0),
    (1, 206, 20, 36, 64, 5, 1, (2,) * 4, False, False, 0),
    (2, 208, 16, 16, 208, 3, 1, (1,) * 4, False, False, 0),
    (2, 80, 20, 24, 80, 5, 1, (2,) * 4, False, False, 0),
    (2, 40, 12, 12, 48, 3, 1, (1,) * 4, False, False, 0),
    (2, 16, 8, 8, 8, 3, 1, (1,) * 4, False, False, 0),
    (4, 64, 10, 10, 64, 3, 1, (1,) * 4, False, False, 0),
    (2, 128, 20, 20, 128, 3, 1, (1,) * 4, False, False, 0),
    (8, 256, 8, 8, 256, 3, 1, (1,) * 4, False, False, 0),
    (4, 512, 8, 8, 512, 3, 1, (1,) * 4, False, False, 0),
    (2, 64, 8, 8, 160, 3, 1, (1,) * 4, False, False, 0),
    (2, 128, 16, 16, 64, 1, 1, (0,) * 4, False, False, 0),
    (4, 128, 16, 16, 64, 3, 2, (1,) * 4, False, False, 0),
    (4, 64, 5, 5, 32, 3, 2, (1,) * 4, False, True, 1),
    (4, 96, 8, 8, 96, 2, 1, (1, 0, 1, 0), True, False, 0),
]


def _real_desc(g, dtype=L.TPG_BF16):
    n, cin, h, w, cout, k, s, pad, reflect, transposed, op = g
    d = L.ConvDesc()
    d.n, d.in_c, d.in_h, d.in_w, d.out_c = n, cin, h, w, cout
    d.kh = d.kw = k
    d.stride_h = d.stride_w = s
    d.pad_t, d.pad_b, d.pad_l, d.pad_r = pad
    if transposed:
        d.out_h = (h - 1) * s - pad[0] - pad[1] + k + op
        d.out_w = (w - 1) * s - pad[2] - pad[3] + k + op
    else:
        d.out_h = (h + pad[0] + pad[1] - k) // s + 1
        d.out_w = (w + pad[2] + pad[3] - k) // s + 1
    d.pad_mode = L.PAD_REFLECT if reflect else L.PAD_ZERO
    d.transposed = 1 if transposed else 0
    d.dtype = dtype
    d.act, d.slope, d.res_scale = L.ACT_LEAKY, 0.01, 1.0
    return d


def _real_jobs(lib, d, op):
    """(image bytes, raw pack jobs) the planner gives for (d, op): host work only, the two
    pointers are just written into the jobs."""
    n, cin, cout, k = d.n, d.in_c, d.out_c, d.kh
    wshape = (cin, cout, k, k) if d.transposed else (cout, cin, k, k)
    w = L.TpgTensor()
    w.data, w.dtype = 0x10000, L.TPG_F32
    # a channels-last weight: dim 1 innermost
    w.stride[0], w.stride[1], w.stride[2], w.stride[3] = wshape[1] * k * k, 1, k * wshape[1], wshape[1]
    nb = lib.tpg_conv2d_packed_bytes(ctypes.byref(d), op)
    jb = lib.tpg_pack_job_bytes()
    host = ctypes.create_string_buffer(jb * 64)
    nj = lib.tpg_conv2d_pack_jobs(ctypes.byref(d), op, w, 0x20000, host, 64)
    assert nj >= 0, lib.tpg_last_error()
    return nb, host.raw[:jb * nj]


@pytest.mark.parametrize("dtype", [L.TPG_BF16, L.TPG_F16], ids=["bf16", "f16"])
@pytest.mark.parametrize("g", PLAN_GEOMS, ids=["%dx%d-%d" % (g[1], g[5], i) for i, g in enumerate(PLAN_GEOMS)])
def test_pack_jobs_ignore_plan_fields(g, dtype):
    """The invariant the entry key rests on: tpg_conv2d_packed_bytes and every byte of the pack
    jobs are the same whatever flags & CONCURRENT, data_algo and data_ksplit say (in both
    reduction modes), for the forward and the input-gradient image."""
    lib = L.load(require_gpu=False)
    prev = lib.tpg_get_deterministic()
    try:
        for op in (L.OP_FWD, L.OP_BWD_DATA):
            ref = None
            for det in (0, 1):
                lib.tpg_set_deterministic(det)
                for flags in (0, L.FLAG_CONCURRENT):
                    for ks, algo in ((0, 0), (1, 0), (2, 0), (5, 0), (0, 1), (0, 2), (4, 2)):
                        d = _real_desc(g, dtype)
                        d.flags, d.data_ksplit, d.data_algo = flags, ks, algo
                        got = _real_jobs(lib, d, op)
                        assert got[0] > 0 and got[1], (op, "no packed form")
                        if ref is None:
                            ref = got
                        assert got[0] == ref[0], (op, det, flags, ks, algo, got[0], ref[0])
                        assert got[1] == ref[1], (op, det, flags, ks, algo)
    finally:
        lib.tpg_set_deterministic(prev)


def test_pack_jobs_follow_the_shape():
    """(the comparison above can fail: another batch size or dtype does change the jobs)"""
    lib = L.load(require_gpu=False)
    g = PLAN_GEOMS[8]
    a = _real_jobs(lib, _real_desc(g), L.OP_FWD)
    assert _real_jobs(lib, _real_desc(g[:4] + (64,) + g[5:]), L.OP_FWD) != a
    assert _real_jobs(lib, _real_desc(g), L.OP_BWD_DATA)[1] != a[1]
