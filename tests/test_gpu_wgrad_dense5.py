"""GPU: the dense five-tap weight-gradient tile (desc.algo 14: one block per kernel row of a
5-wide kernel and per channel tile of at most 112 x 112, the 5 x (b / 16) column blocks dealt to
the 8 waves) against the fp64 torch weight and bias gradient of the 16-bit-rounded inputs.

Shapes are the smallest that reach every path: maps of 3 x 64 (every row within reach of the
vertical padding), 7 x 64 and 3 x 128 (two 64-pixel segments: the horizontal halo crosses a
segment boundary); channel pairs 206 x 206 (two a-tiles and two b-tiles, the second of each with
a dead block row / column), 80 x 80, 64 x 64, 64 x 206 (a swapped operand shows), 17 x 113 and
113 x 17 (dead 16-blocks, a 16-byte chunk straddling the channel count, a second tile of one
channel); one and three pixel splits (2 x 3 x 64: 6 k-tiles split 2 / 2 / 2, 2 x 7 x 64: 14 split
5 / 5 / 4); with the bias gradient (tpg_conv2d_bwd) and without (tpg_conv2d_bwd_filter); zero and
reflect padding; bf16 and fp16; dW and dbias pre-filled, since the kernel accumulates.  The
current tile (algo 7, or 9 where 7 refuses) runs on the same inputs under the same bound."""
import ctypes
import zlib

import pytest
import torch
import torch.nn.functional as F

from _cases import rel

pytestmark = pytest.mark.gpu

# tests/test_gpu_ops.py test_wgrad_rowhalo: 16-bit weight gradients of 16-bit-representable
# inputs differ from fp64 only by the fp32 accumulation order
RH_TOL = 1e-5
DENSE5, CURRENT = 14, (7, 9)

MAPS = [(3, 64), (7, 64), (3, 128)]
CHANNELS = [(206, 206), (80, 80), (64, 64), (64, 206), (17, 113), (113, 17)]  # (dY, X)
N, K, PAD = 2, 5, 2


def _inputs(gpu, cout, cin, h, w, dtype, refl):
    """x, g on the device, and the fp64 dW / dbias of their rounded values."""
    import tpgan_ops as T
    gen = torch.Generator().manual_seed(zlib.crc32(repr((cout, cin, h, w, str(dtype), refl)).encode()))
    x64 = (torch.rand(N, cin, h, w, generator=gen, dtype=torch.float64) * 2 - 1).to(dtype).double()
    g64 = (torch.rand(N, cout, h, w, generator=gen, dtype=torch.float64) * 2 - 1).to(dtype).double()
    w64 = torch.zeros((cout, cin, K, K), dtype=torch.float64, requires_grad=True)
    xin = F.pad(x64, (PAD, PAD, PAD, PAD), mode="reflect") if refl else x64
    F.conv2d(xin, w64, None, 1, 0 if refl else PAD).backward(g64)
    x = T.new_act(N, cin, h, w, dtype, gpu)
    x.copy_(x64.to(gpu))
    g = T.new_act(N, cout, h, w, dtype, gpu)
    g.copy_(g64.to(gpu))
    return x, g, w64.grad, g64.sum(dim=(0, 2, 3)), gen


def _launch(lib, d, x, g, dw, db):
    from tpgan_lib import stream_ptr, tt
    if db is None:
        return lib.tpg_conv2d_bwd_filter(ctypes.byref(d), tt(x), tt(g), tt(dw), None, 0, stream_ptr())
    # no activation: g is gy itself; no dx
    return lib.tpg_conv2d_bwd(ctypes.byref(d), tt(x), tt(None), tt(None), tt(g), tt(None), tt(None), tt(dw),
                              db.data_ptr(), None, 0, stream_ptr())


def _run(lib, d, x, g, dw, db):
    from tpgan_lib import check
    check(_launch(lib, d, x, g, dw, db))
    torch.cuda.synchronize()


def _run_current(lib, d, x, g, dw, db, ks):
    """The tile the tuner had before: algo 7, or 9 where 7 refuses the shape (-30, before any launch)."""
    from tpgan_lib import check
    d.algo, d.ksplit = CURRENT[0], ks
    rc = _launch(lib, d, x, g, dw, db)
    if rc == -30:
        d.algo = CURRENT[1]
        rc = _launch(lib, d, x, g, dw, db)
    check(rc)
    torch.cuda.synchronize()
    return d.algo


@pytest.mark.parametrize("chan", CHANNELS, ids=["%dx%d" % c for c in CHANNELS])
@pytest.mark.parametrize("hw", MAPS, ids=["%dx%d" % m for m in MAPS])
def test_wgrad_dense5_vs_fp64(gpu, hw, chan):
    import tpgan_ops as T
    from tpgan_lib import PAD_REFLECT, PAD_ZERO, load
    lib = load()
    (h, w), (cout, cin) = hw, chan
    for dtype in (torch.bfloat16, torch.float16):
        for refl in (False, True):
            x, g, ref_w, ref_b, gen = _inputs(gpu, cout, cin, h, w, dtype, refl)
            geo = T.ConvGeom(K, K, (1, 1), (PAD, PAD, PAD, PAD), PAD_REFLECT if refl else PAD_ZERO)
            d = geo.desc(N, cin, h, w, cout, h, w, dtype, 0, 0.0, 1.0)
            for ks in (1, 3):
                for bias in (False, True):
                    for new in (True, False):
                        init = torch.randn((cout, cin, K, K), generator=gen).float()
                        binit = torch.randn(cout, generator=gen).float()
                        dw = init.to(gpu).contiguous(memory_format=torch.channels_last)
                        db = binit.to(gpu) if bias else None
                        if new:
                            d.algo, d.ksplit = DENSE5, ks
                            _run(lib, d, x, g, dw, db)
                        else:
                            _run_current(lib, d, x, g, dw, db, ks)
                        what = (d.algo, str(dtype), "reflect" if refl else "zero", ks, bias)
                        e = rel(dw.cpu() - init, ref_w)
                        assert e < RH_TOL, what + (e,)
                        if bias:
                            e = rel(db.cpu() - binit, ref_b)
                            assert e < RH_TOL, what + ("dbias", e)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
def test_wgrad_dense5_deterministic(gpu, dtype):
    """tpg_set_deterministic(1): one block adds each dW element and one wave each dbias element
    once, whatever split was asked for, so two runs are bit-identical (and still right)."""
    import tpgan_ops as T
    from tpgan_lib import PAD_ZERO, load
    lib = load()
    h, w, cout, cin = 3, 128, 206, 206
    x, g, ref_w, ref_b, gen = _inputs(gpu, cout, cin, h, w, dtype, False)
    geo = T.ConvGeom(K, K, (1, 1), (PAD, PAD, PAD, PAD), PAD_ZERO)
    d = geo.desc(N, cin, h, w, cout, h, w, dtype, 0, 0.0, 1.0)
    d.algo, d.ksplit = DENSE5, 3
    init = torch.randn((cout, cin, K, K), generator=gen).float()
    binit = torch.randn(cout, generator=gen).float()
    lib.tpg_set_deterministic(1)
    try:
        got = []
        for _ in range(2):
            dw = init.to(gpu).contiguous(memory_format=torch.channels_last)
            db = binit.to(gpu)
            _run(lib, d, x, g, dw, db)
            got.append((dw.cpu(), db.cpu()))
    finally:
        lib.tpg_set_deterministic(0)
    assert torch.equal(got[0][0], got[1][0]) and torch.equal(got[0][1], got[1][1])
    assert rel(got[0][0] - init, ref_w) < RH_TOL and rel(got[0][1] - binit, ref_b) < RH_TOL
