"""Shared by the GPU pack tests: rebuild a pre-packed weight image from scratch.

An entry's image is checked against the LIVE fp32 parameter, not against the entry's own stored
jobs: the source pointer is looked up among the network's current parameters, fresh jobs are
planned with tpg_conv2d_pack_jobs from the entry's stored descriptor into new buffers, and every
byte the pack kernel writes must equal the entry's image.  (Which bytes it writes is measured,
not assumed: two fresh packs into buffers pre-filled with 0x00 and 0xff agree exactly on the
written bytes; the rest is row / region padding that no pack ever touches.)"""
import ctypes

import torch


def live_view(params, e):
    """The view (entry's shape and strides) of the live parameter that starts at the entry's
    source pointer, or None.  The view must cover that parameter's elements exactly once."""
    nel = 1
    for s in e.shape:
        nel *= s
    for p in params:
        if p.data_ptr() == e.src and p.numel() == nel:
            dims = sorted((st, sz) for sz, st in zip(e.shape, e.strides) if sz > 1)
            run = 1
            for st, sz in dims:
                assert st == run, ("entry view is not a dense re-indexing of its parameter", e.shape, e.strides)
                run *= sz
            return p.data.as_strided(e.shape, e.strides, p.storage_offset())
    return None


def _fresh(ops, e, w, fill):
    import tpgan_lib as L
    lib = ops.load()
    d = L.ConvDesc.from_buffer_copy(e.desc)
    nb = lib.tpg_conv2d_packed_bytes(ctypes.byref(d), e.op)
    assert nb == e.buf.numel(), (nb, e.buf.numel())
    buf = torch.full((nb,), fill, dtype=torch.uint8, device=w.device)
    jb = lib.tpg_pack_job_bytes()
    host = ctypes.create_string_buffer(jb * 64)
    n = lib.tpg_conv2d_pack_jobs(ctypes.byref(d), e.op, ops.tt(w), buf.data_ptr(), host, 64)
    assert n == e.njobs, (n, e.njobs)
    nblocks = lib.tpg_pack_prepare(host, n)
    assert nblocks == e.nblocks
    dev = torch.frombuffer(bytearray(host.raw[:jb * n]), dtype=torch.uint8).to(w.device)
    ops.check(lib.tpg_pack_run(dev.data_ptr(), n, nblocks, ops.stream_ptr()))
    torch.cuda.synchronize()
    return buf


def image_is_fresh(ops, e, w):
    """(ok, written bytes): e.buf against a from-scratch pack of the live fp32 view w."""
    a = _fresh(ops, e, w, 0x00)
    b = _fresh(ops, e, w, 0xFF)
    written = a == b
    nw = int(written.sum())
    # (every weight element is in the image at least once, as a 16-bit value)
    assert nw >= 2 * w.numel(), ("the fresh pack wrote too little", nw, w.numel())
    return bool(torch.equal(e.buf[written], a[written])), nw


def check_entries(ops, flat, params, tag):
    """Every image of `flat` is current and equals a fresh pack of its live parameter; returns
    how many were checked."""
    torch.cuda.synchronize()
    n = 0
    for key, e in flat.pack_entries.items():
        if e is None or not e.njobs:
            continue
        what = (tag, key[0], key[1][:9])
        assert e.epoch == flat.epoch, what + (e.epoch, flat.epoch)
        assert e.key == key and (e.src, e.strides) == (key[2], key[3]), what
        w = live_view(params, e)
        assert w is not None, what + ("no live parameter at the entry's source pointer", hex(e.src))
        ok, _ = image_is_fresh(ops, e, w)
        assert ok, what + ("image differs from a fresh pack of the live weight",)
        n += 1
    return n
