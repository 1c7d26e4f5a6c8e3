"""Op-level float64 parity of the identity-extractor kernels (csrc/tpg_features.hip): depthwise
conv forward / input gradient / weight gradient, training-mode BatchNorm forward / backward,
max and global average pooling, and the eval-mode BatchNorm fold.

Every kernel is compared alone with a float64 restatement of the same operation on inputs that
were first rounded to the dtype under test, so the reference sees exactly what the kernel loads.
Where a backward applies act' from the saved output, the reference takes its mask from the y
the device forward stored (the kernel's documented contract); y itself is checked separately.

Bounds (none of them is fitted to what the kernels produce):
  * a tensor stored in 16 bits differs from fp32 accumulation by one round-to-nearest of the
    output, relative error <= 2^-9 (bf16) / 2^-12 (fp16): relative L2 < 2^-8 / 2^-11;
  * fp32 outputs of representable inputs differ from fp64 by fp32 summation order only: 1e-5 for
    sums over pixels (test_wgrad_rowhalo, test_dwconv_vs_aten), 1e-6 for pooling;
  * BatchNorm subtracts a batch mean, so its fp32 error depends on conditioning: max(1e-5,
    4 x floor), floor = distance of aten's CPU float32 batch norm from the fp64 reference (the
    factor 4: per-thread partials, an LDS tree and one atomic per block in arrival order are
    another summation order than aten's, and one that varies from run to run);
  * selections and copies (max pooling y, gradient routing) are bit-exact.
"""
import ctypes
import functools
import zlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from _cases import rel

pytestmark = pytest.mark.gpu

DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
ROUND16 = {"bf16": 2.0 ** -8, "f16": 2.0 ** -11}  # twice the round-to-nearest bound
ACTS = {"none": (0, 0.0), "relu": (1, 0.0), "leaky": (2, 0.1), "relu6": (3, 0.0)}
ACT_MODULES = {"none": lambda: None, "relu": torch.nn.ReLU, "leaky": lambda: torch.nn.LeakyReLU(0.1),
               "relu6": torch.nn.ReLU6}


def _seed(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def _act64(v, act):
    code, slope = ACTS[act]
    if code == 1:
        return v.clamp(min=0)
    if code == 2:
        return torch.where(v > 0, v, v * slope)
    if code == 3:
        return v.clamp(0, 6)
    return v


def _act_grad64(g, y, act):
    """g * act'(pre-activation), the linear piece identified from the stored output y."""
    code, slope = ACTS[act]
    if code == 1:
        return torch.where(y > 0, g, torch.zeros_like(g))
    if code == 2:
        return torch.where(y > 0, g, g * slope)
    if code == 3:
        return torch.where((y > 0) & (y < 6), g, torch.zeros_like(g))
    return g


def _bound(dt, f32_bound):
    return ROUND16[dt] if dt != "f32" else f32_bound


def _dev_act(t64, dtype, gpu):
    """A channels-last activation (tpgan_ops.new_act) holding the (already rounded) fp64 values."""
    import tpgan_ops as T
    v = T.new_act(*t64.shape, dtype=dtype, device=gpu)
    v.copy_(t64.to(gpu))
    return v


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


# ------------------------------------------------------------------------ depthwise conv --
DW_GEOMS = [
    # (N, C, H, W, kh, kw, stride, pad)
    (2, 96, 20, 18, 3, 3, 1, 1),    # 9 forward blocks, 3 weight-gradient blocks
    (2, 960, 8, 8, 3, 3, 1, 1),     # widest real layer: 4 wgrad blocks, nch 120 / 240 (idle lanes)
    (1, 1030, 5, 5, 3, 3, 2, 1),    # fp32: second channel group with a tail; 16-bit: surplus group
    (3, 19, 12, 10, 3, 3, 2, 1),    # even map: the last row / column meets only some taps
    (2, 24, 9, 11, 2, 2, 2, 0),     # a kernel other than 3x3
    (2, 40, 7, 7, 1, 1, 1, 0),      # 1x1
]
DW_IDS = ["c96", "c960", "c1030s2", "c19s2", "k2s2", "k1"]


@functools.lru_cache(maxsize=None)
def _dw_ref(geom, dt):
    """fp64 inputs (rounded to the dtype; w, b, residual too) and F.conv2d(groups=C) results."""
    N, C, H, W, kh, kw, s, p = geom
    dtype = DTYPES[dt]
    gen = _seed("dw", geom, dt)

    def u(*shape):
        return torch.rand(*shape, generator=gen, dtype=torch.float64) * 2 - 1

    x = u(N, C, H, W).to(dtype).double()
    w = (u(C, 1, kh, kw) * 2).float().double()
    b = (u(C) * 2 + 1).float().double()
    xr, wr = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    pre = F.conv2d(xr, wr, None, s, p, groups=C)
    g = u(*pre.shape).to(dtype).double()
    res = (u(*pre.shape) * 2).to(dtype).double()
    pre.backward(g)
    return dict(x=x, w=w, b=b, g=g, res=res, pre=pre.detach(), dx=xr.grad, dw=wr.grad)


def _dw_desc(geom, dtype, oh, ow, act="none", res_scale=1.0):
    import tpgan_ops as T
    N, C, H, W, kh, kw, s, p = geom
    code, slope = ACTS[act]
    return T._dw_desc(N, C, H, W, oh, ow, kh, kw, (s, s), (p, p), dtype, code, slope, res_scale)


def _dw_forward(gpu, geom, dt, act, bias, residual, res_scale):
    from tpgan_lib import check, load, stream_ptr, tt
    import tpgan_ops as T
    lib = load()
    r = _dw_ref(geom, dt)
    dtype = DTYPES[dt]
    N, C = geom[0], geom[1]
    oh, ow = r["pre"].shape[2:]
    x = _dev_act(r["x"], dtype, gpu)
    w = r["w"].float().to(gpu)
    b = r["b"].float().to(gpu) if bias else None
    res = _dev_act(r["res"], dtype, gpu) if residual else None
    y = T.new_act(N, C, oh, ow, dtype, gpu)
    d = _dw_desc(geom, dtype, oh, ow, act, res_scale)
    check(lib.tpg_dwconv2d_fwd(ctypes.byref(d), tt(x), tt(w), _ptr(b), tt(res), tt(y), stream_ptr()))
    torch.cuda.synchronize()
    ref = r["pre"]
    if bias:
        ref = ref + r["b"].view(1, -1, 1, 1)
    if residual:
        ref = ref + res_scale * r["res"]
    return y.double().cpu(), _act64(ref, act)


@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("geom", DW_GEOMS, ids=DW_IDS)
def test_dwconv_fwd(gpu, geom, dt):
    y, ref = _dw_forward(gpu, geom, dt, "relu6", True, False, 1.0)
    e = rel(y, ref)
    print("dw fwd", geom, dt, "%.3e" % e)
    if geom[4] * geom[5] == 9:  # both clamps of ReLU6 are live
        assert bool((ref == 6).any()) and bool((ref == 0).any())
    assert e < _bound(dt, 1e-5)


@pytest.mark.parametrize("variant", ["nobias", "residual", "none", "relu", "leaky", "relu6"])
@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("geom", DW_GEOMS[:2], ids=DW_IDS[:2])
def test_dwconv_fwd_variants(gpu, geom, dt, variant):
    """bias = NULL, a residual scaled by 0.5 inside the activation, and each fused activation."""
    if variant == "nobias":
        y, ref = _dw_forward(gpu, geom, dt, "none", False, False, 1.0)
    elif variant == "residual":
        y, ref = _dw_forward(gpu, geom, dt, "relu6", True, True, 0.5)
    else:
        y, ref = _dw_forward(gpu, geom, dt, variant, True, False, 1.0)
    e = rel(y, ref)
    print("dw fwd", geom, dt, variant, "%.3e" % e)
    assert e < _bound(dt, 1e-5)


@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("geom", DW_GEOMS, ids=DW_IDS)
def test_dwconv_bwd_data(gpu, geom, dt):
    from tpgan_lib import check, load, stream_ptr, tt
    import tpgan_ops as T
    lib = load()
    r = _dw_ref(geom, dt)
    dtype = DTYPES[dt]
    N, C, H, W = geom[:4]
    oh, ow = r["pre"].shape[2:]
    g = _dev_act(r["g"], dtype, gpu)
    w = r["w"].float().to(gpu)
    dx = T.new_act(N, C, H, W, dtype, gpu)
    dx.fill_(float("nan"))  # every input pixel is written, also those no tap reaches (stride 2)
    d = _dw_desc(geom, dtype, oh, ow)
    check(lib.tpg_dwconv2d_bwd_data(ctypes.byref(d), tt(g), tt(w), tt(dx), stream_ptr()))
    torch.cuda.synchronize()
    e = rel(dx.double().cpu(), r["dx"])
    print("dw dgrad", geom, dt, "%.3e" % e)
    assert e < _bound(dt, 1e-5)


@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("geom", DW_GEOMS, ids=DW_IDS)
def test_dwconv_bwd_filter(gpu, geom, dt):
    """dw is fp32 for every compute dtype and the entry point accumulates into it."""
    from tpgan_lib import check, load, stream_ptr, tt
    lib = load()
    r = _dw_ref(geom, dt)
    dtype = DTYPES[dt]
    oh, ow = r["pre"].shape[2:]
    x = _dev_act(r["x"], dtype, gpu)
    g = _dev_act(r["g"], dtype, gpu)
    init = torch.randn(r["w"].shape, generator=_seed("dwinit", geom, dt)).float()
    dw = init.to(gpu)
    d = _dw_desc(geom, dtype, oh, ow)
    check(lib.tpg_dwconv2d_bwd_filter(ctypes.byref(d), tt(x), tt(g), tt(dw), stream_ptr()))
    torch.cuda.synchronize()
    e = rel(dw.double().cpu() - init.double(), r["dw"])
    print("dw wgrad", geom, dt, "%.3e" % e)
    assert e < 1e-5


@pytest.mark.parametrize("dt", list(DTYPES))
def test_dwconv_rejects_unaligned_rows(gpu, dt):
    """A pixel stride that is no multiple of 16 bytes is refused (-12) by the host-side check,
    before any launch: the sentinel-filled outputs stay as they were."""
    from tpgan_lib import load, stream_ptr, tt
    import tpgan_ops as T
    lib = load()
    dtype = DTYPES[dt]
    geom = (2, 19, 6, 5, 3, 3, 1, 1)
    N, C, H, W = geom[:4]
    ps = 22 if dt == "f32" else 20  # 88 / 40 bytes
    bad = torch.full((N, H, W, ps), 3.0, dtype=dtype, device=gpu).permute(0, 3, 1, 2)[:, :C]
    good = T.new_act(N, C, H, W, dtype, gpu)
    good.fill_(3.0)
    w = torch.full((C, 1, 3, 3), 0.25, dtype=torch.float32, device=gpu)
    d = _dw_desc(geom, dtype, H, W)
    keep_bad, keep_good, keep_w = bad.clone(), good.clone(), w.clone()
    s = stream_ptr()
    rcs = [lib.tpg_dwconv2d_fwd(ctypes.byref(d), tt(bad), tt(w), None, tt(None), tt(good), s),
           lib.tpg_dwconv2d_fwd(ctypes.byref(d), tt(good), tt(w), None, tt(None), tt(bad), s),
           lib.tpg_dwconv2d_fwd(ctypes.byref(d), tt(good), tt(w), None, tt(bad), tt(good), s),
           lib.tpg_dwconv2d_bwd_data(ctypes.byref(d), tt(bad), tt(w), tt(good), s),
           lib.tpg_dwconv2d_bwd_data(ctypes.byref(d), tt(good), tt(w), tt(bad), s),
           lib.tpg_dwconv2d_bwd_filter(ctypes.byref(d), tt(bad), tt(good), tt(w), s),
           lib.tpg_dwconv2d_bwd_filter(ctypes.byref(d), tt(good), tt(bad), tt(w), s)]
    torch.cuda.synchronize()
    assert rcs == [-12] * 7
    assert torch.equal(bad, keep_bad) and torch.equal(good, keep_good) and torch.equal(w, keep_w)


# ------------------------------------------------------------------ training BatchNorm --
# Beside each case: the measured floor (aten CPU float32 from fp64) -> the kernel's measured
# distance from fp64 on an MI355X, fp32 run with ReLU6 and momentum 0.1, for y, dx, dgamma and
# dbeta (every fp32 bound is therefore the 1e-5 term of max(1e-5, 4 x floor)); then the 16-bit
# y / dx distances, which sit under the rounding bounds 3.91e-3 (bf16) and 4.88e-4 (fp16).
# The running statistics and save_mean / save_invstd measured 3e-8..6e-8 in every case and dtype,
# dgamma / dbeta of the 16-bit runs 2e-8..2e-7.
BN_CASES = [
    # (N, C, H, W)
    # 3 blocks, channel tail
    #   y 3.85e-8 -> 6.50e-8, dx 5.72e-8 -> 7.07e-8, dgamma 6.81e-8 -> 1.09e-7, dbeta 1.29e-7 -> 1.33e-7
    #   bf16 y 1.61e-3, dx 1.69e-3; fp16 y 1.96e-4, dx 2.08e-4
    (4, 37, 16, 15),
    # 3 blocks at 6 pixel lanes
    #   y 4.29e-8 -> 5.24e-8, dx 5.87e-8 -> 7.01e-8, dgamma 5.49e-8 -> 1.01e-7, dbeta 7.90e-8 -> 8.15e-8
    #   bf16 y 1.57e-3, dx 1.66e-3; fp16 y 1.98e-4, dx 2.07e-4
    (2, 320, 7, 7),
    # MobileNetV2's last BN; fp32: two channel groups
    #   y 4.40e-8 -> 5.46e-8, dx 6.74e-8 -> 7.49e-8, dgamma 5.50e-8 -> 7.80e-8, dbeta 6.41e-8 -> 6.30e-8
    #   bf16 y 1.59e-3, dx 1.67e-3; fp16 y 2.00e-4, dx 2.05e-4
    (2, 1280, 3, 3),
    # ResNet-50; 16-bit: exactly one full group with ppi = 1; fp32: two full groups
    #   y 4.64e-8 -> 5.71e-8, dx 7.08e-8 -> 8.64e-8, dgamma 5.49e-8 -> 8.51e-8, dbeta 4.63e-8 -> 5.83e-8
    #   bf16 y 1.62e-3, dx 1.64e-3; fp16 y 2.03e-4, dx 2.07e-4
    (2, 2048, 2, 2),
    # 16-bit: second channel group with a tail
    #   y 5.06e-8 -> 5.97e-8, dx 8.35e-8 -> 9.85e-8, dgamma 5.50e-8 -> 8.33e-8, dbeta 4.03e-8 -> 5.51e-8
    #   bf16 y 1.62e-3, dx 1.67e-3; fp16 y 2.02e-4, dx 2.05e-4
    (1, 2056, 2, 3),
]
BN_IDS = ["c37", "c320", "c1280", "c2048", "c2056"]
# fp32 only: per-channel mean ~30, standard deviation ~0.1.  Here the floor term decides:
#   y 8.01e-6 -> 1.55e-5 (bound 3.21e-5), dgamma 8.20e-6 -> 2.06e-5 (bound 3.28e-5),
#   dx 2.54e-7 -> 7.14e-7, dbeta 1.04e-7 -> 1.44e-7, save_mean 2.02e-8 -> 6.07e-8 (bound 1e-5)
BN_HIGH_MEAN = (4, 37, 16, 15)
EPS = 1e-5


@functools.lru_cache(maxsize=None)
def _bn_inputs(case, dt, high_mean=False):
    N, C, H, W = case
    dtype = DTYPES[dt]
    gen = _seed("bn", case, dt, high_mean)

    def u(*shape):
        return torch.rand(*shape, generator=gen, dtype=torch.float64)

    z = torch.randn(N, C, H, W, generator=gen, dtype=torch.float64)
    if high_mean:
        x = z * 0.1 + (30 + u(1, C, 1, 1) * 2 - 1)
    else:
        x = z * (1 + u(1, C, 1, 1)) + (u(1, C, 1, 1) * 2 - 1)
    x = x.to(dtype).double()
    gamma = (1 + 2 * u(C)).float().double()
    beta = (3 * u(C) - 1).float().double()
    dy = (u(N, C, H, W) * 2 - 1).to(dtype).double()
    # every channel's batch variance is well above eps (checked here, on the CPU)
    assert float(x.var((0, 2, 3), unbiased=False).min()) > 100 * EPS
    return x, gamma, beta, dy


def _bn_check(name, got, ref, floor_val, dt, out16, log):
    """fp32 outputs: the floor rule; 16-bit stored tensors: the output-rounding bound."""
    e = rel(got, ref)
    f = rel(floor_val, ref)
    bound = ROUND16[dt] if (out16 and dt != "f32") else max(1e-5, 4 * f)
    log.append("%s floor %.2e kernel %.2e bound %.2e" % (name, f, e, bound))
    return e < bound


def _bn_run(gpu, case, dt, act="relu6", track=True, momentum=0.1, high_mean=False):
    import tpgan_ops as T
    from tpgan_lib import TpgTensor, check, load, stream_ptr, tt
    lib = load()
    N, C, H, W = case
    M = N * H * W
    dtype = DTYPES[dt]
    x64, gamma64, beta64, dy64 = _bn_inputs(case, dt, high_mean)

    # ---- forward through the product wrapper
    bn = torch.nn.BatchNorm2d(C, eps=EPS, momentum=momentum, track_running_stats=track)
    with torch.no_grad():
        bn.weight.copy_(gamma64)
        bn.bias.copy_(beta64)
    bn = bn.to(gpu).train()
    x = _dev_act(x64, dtype, gpu)
    with T.compute_dtype(dtype):
        y = T.batchnorm_train(x, bn, act=ACT_MODULES[act]())
    torch.cuda.synchronize()
    xs, ys, _, mean, invstd = y.grad_fn.saved_tensors
    assert xs.data_ptr() == x.data_ptr() and ys.data_ptr() == y.data_ptr() and y.dtype == dtype

    # fp64 reference, and the same formulas by aten in float32 on the CPU (the floor)
    mean64 = x64.mean((0, 2, 3))
    var64 = x64.var((0, 2, 3), unbiased=False)
    invstd64 = 1 / torch.sqrt(var64 + EPS)
    xhat64 = (x64 - mean64.view(1, -1, 1, 1)) * invstd64.view(1, -1, 1, 1)
    y64 = _act64(xhat64 * gamma64.view(1, -1, 1, 1) + beta64.view(1, -1, 1, 1), act)
    rm32, rv32 = torch.zeros(C), torch.ones(C)
    x32 = x64.float().requires_grad_(True)
    w32, b32 = gamma64.float().requires_grad_(True), beta64.float().requires_grad_(True)
    pre32, smean32, sinv32 = torch.native_batch_norm(x32, w32, b32, rm32, rv32, True, momentum, EPS)
    y32 = _act64(pre32.detach(), act)

    log, ok = [], []
    yd = y.detach().double().cpu()
    ok.append(_bn_check("y", yd, y64, y32, dt, True, log))
    ok.append(_bn_check("save_mean", mean.cpu(), mean64, smean32.detach(), dt, False, log))
    ok.append(_bn_check("save_invstd", invstd.cpu(), invstd64, sinv32.detach(), dt, False, log))
    if track:
        ok.append(_bn_check("running_mean", bn.running_mean.cpu(), momentum * mean64, rm32, dt, False, log))
        rv64 = (1 - momentum) + momentum * var64 * M / (M - 1)
        ok.append(_bn_check("running_var", bn.running_var.cpu(), rv64, rv32, dt, False, log))
        assert int(bn.num_batches_tracked) == 1
    else:
        assert bn.running_mean is None and bn.running_var is None and bn.num_batches_tracked is None

    # ---- backward through the C ABI; act' from the y the device stored
    g64 = _act_grad64(dy64, yd, act)
    sg, sgx = g64.sum((0, 2, 3)), (g64 * xhat64).sum((0, 2, 3))
    dx64 = (gamma64 * invstd64).view(1, -1, 1, 1) * (g64 - (sg / M).view(1, -1, 1, 1)
                                                    - xhat64 * (sgx / M).view(1, -1, 1, 1))
    dx32, dg32, db32 = torch.autograd.grad(pre32, (x32, w32, b32), g64.float())
    dy = _dev_act(dy64, dtype, gpu)
    gam = gamma64.float().to(gpu)
    ws = torch.empty(2 * C, dtype=torch.float32, device=gpu)

    def bwd(dx, dgamma, dbeta):
        check(lib.tpg_bn_train_bwd(N, C, H, W, ACTS[act][0], ACTS[act][1], tt(dy), tt(y), tt(x), _ptr(gam),
                                   _ptr(mean), _ptr(invstd), tt(dx) if dx is not None else TpgTensor(),
                                   _ptr(dgamma), _ptr(dbeta), _ptr(ws), stream_ptr()))
        torch.cuda.synchronize()

    gen = _seed("bninit", case, dt)
    ig, ib = torch.randn(C, generator=gen), torch.randn(C, generator=gen)
    # (a) everything, dgamma / dbeta pre-filled: the entry point adds to them
    dx, dgam, dbet = T.new_act(N, C, H, W, dtype, gpu), ig.to(gpu), ib.to(gpu)
    bwd(dx, dgam, dbet)
    ok.append(_bn_check("dx", dx.double().cpu(), dx64, dx32, dt, True, log))
    ok.append(_bn_check("dgamma", dgam.double().cpu() - ig.double(), sgx, dg32, dt, False, log))
    ok.append(_bn_check("dbeta", dbet.double().cpu() - ib.double(), sg, db32, dt, False, log))
    # (b) dx.data == NULL: the parameter gradients alone
    dgam, dbet = ig.to(gpu), ib.to(gpu)
    bwd(None, dgam, dbet)
    ok.append(_bn_check("dgamma (no dx)", dgam.double().cpu() - ig.double(), sgx, dg32, dt, False, log))
    ok.append(_bn_check("dbeta (no dx)", dbet.double().cpu() - ib.double(), sg, db32, dt, False, log))
    # (c) NULL dgamma / dbeta: the input gradient alone
    dx = T.new_act(N, C, H, W, dtype, gpu)
    bwd(dx, None, None)
    ok.append(_bn_check("dx (no dgamma)", dx.double().cpu(), dx64, dx32, dt, True, log))
    print("bn", case, dt, act, "track" if track else "notrack", momentum, "high-mean" if high_mean else "",
          "\n   " + "\n   ".join(log))
    assert all(ok), log


@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("case", BN_CASES, ids=BN_IDS)
def test_bn_train(gpu, case, dt):
    _bn_run(gpu, case, dt)


@pytest.mark.parametrize("variant", ["none", "relu", "leaky", "notrack", "momentum0.3"])
@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("case", BN_CASES[:2], ids=BN_IDS[:2])
def test_bn_train_variants(gpu, case, dt, variant):
    """The other activations, track_running_stats = False (the NULL pair) and another momentum."""
    if variant == "notrack":
        _bn_run(gpu, case, dt, track=False)
    elif variant == "momentum0.3":
        _bn_run(gpu, case, dt, momentum=0.3)
    else:
        _bn_run(gpu, case, dt, act=variant)


def test_bn_train_high_mean(gpu):
    """Per-channel mean ~30 at standard deviation ~0.1: E[x^2] - E[x]^2 in fp32 would lose the
    variance (30^2 * 2^-24 is 5e-5 against 1e-2) and miss the floor rule; two passes do not."""
    _bn_run(gpu, BN_HIGH_MEAN, "f32", high_mean=True)


# --------------------------------------------------------------------------- pooling --
POOL_CASES = [
    # (k, s, p), (N, C, H, W)
    ((3, 2, 1), (2, 20, 12, 10)),
    ((3, 2, 1), (2, 20, 13, 11)),
    ((2, 2, 0), (2, 33, 8, 8)),
    ((3, 1, 1), (1, 7, 6, 5)),
    ((2, 2, 1), (1, 16, 7, 9)),
]
POOL_IDS = ["k3s2p1-12x10", "k3s2p1-13x11", "k2s2p0", "k3s1p1", "k2s2p1"]
POOL_BIG = (2, 64, 130, 130)  # 2,163,200 elements > 8192 blocks x 256 threads: a second grid-stride pass


def _bits(t):
    """The raw bit patterns of a CPU tensor as a numpy integer array."""
    t = t.contiguous()
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16).numpy()


def _maxpool_run(gpu, geo, x64, dt, g_seed):
    """(y, dx) of the device op and (y, dx, g) of F.max_pool2d on the same rounded fp64 values."""
    import tpgan_ops as T
    k, s, p = geo
    dtype = DTYPES[dt]
    xr = x64.clone().requires_grad_(True)
    yr = F.max_pool2d(xr, k, s, p)
    g64 = (torch.rand(yr.shape, generator=g_seed, dtype=torch.float64) * 2 - 1).to(dtype).double()
    yr.backward(g64)
    xg = x64.float().to(gpu).requires_grad_(True)
    with T.compute_dtype(dtype):
        y = T.maxpool2d(xg, k, s, p)
    y.backward(g64.to(dtype).to(gpu))
    torch.cuda.synchronize()
    assert y.dtype == dtype
    return y.detach().cpu(), xg.grad.double().cpu(), yr.detach(), xr.grad


@functools.lru_cache(maxsize=None)
def _pool_x(shape, dt):
    # randn rounded to the dtype: bf16 leaves ties inside windows (first tap in scan order wins)
    return torch.randn(*shape, generator=_seed("pool", shape), dtype=torch.float64).to(DTYPES[dt]).double()


@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("geo,shape", POOL_CASES, ids=POOL_IDS)
def test_maxpool(gpu, geo, shape, dt):
    y, dx, yr, dxr = _maxpool_run(gpu, geo, _pool_x(shape, dt), dt, _seed("poolg", geo, shape))
    np.testing.assert_array_equal(_bits(y), _bits(yr.to(DTYPES[dt])))
    e = rel(dx, dxr)
    print("maxpool dx", geo, shape, dt, "%.3e" % e)
    assert e < _bound(dt, 1e-6)


@pytest.mark.parametrize("dt", list(DTYPES))
def test_maxpool_nan(gpu, dt):
    """Isolated NaNs, at most one per 3x3 window (every fourth row and column): y is NaN exactly
    where torch's is and bit-equal elsewhere."""
    import tpgan_ops as T
    dtype = DTYPES[dt]
    x64 = _pool_x((2, 20, 13, 11), dt).clone()
    x64[:, ::3, ::4, ::4] = float("nan")
    yr = F.max_pool2d(x64, 3, 2, 1).to(dtype)
    with T.compute_dtype(dtype):
        y = T.maxpool2d(x64.float().to(gpu), 3, 2, 1)
    torch.cuda.synchronize()
    y = y.cpu()
    nan = torch.isnan(yr)
    assert 0 < int(nan.sum()) < nan.numel()
    np.testing.assert_array_equal(torch.isnan(y).numpy(), nan.numpy())
    np.testing.assert_array_equal(_bits(torch.where(nan, torch.zeros_like(y), y)),
                                  _bits(torch.where(nan, torch.zeros_like(yr), yr)))


def _avgpool_run(gpu, x64, dt, gen):
    import tpgan_ops as T
    dtype = DTYPES[dt]
    N, C, H, W = x64.shape
    g64 = (torch.rand(N, C, 1, 1, generator=gen, dtype=torch.float64) * 2 - 1).to(dtype).double()
    xg = x64.float().to(gpu).requires_grad_(True)
    with T.compute_dtype(dtype):
        a = T.global_avgpool(xg)
    a.backward(g64.to(dtype).to(gpu))
    torch.cuda.synchronize()
    assert a.dtype == dtype and tuple(a.shape) == (N, C, 1, 1)
    ref = x64.mean((2, 3), keepdim=True)
    dref = (g64 / (H * W)).expand(N, C, H, W)
    return rel(a.detach().double().cpu(), ref), rel(xg.grad.double().cpu(), dref)


@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("shape", [c[1] for c in POOL_CASES] + [(2, 33, 1, 1)],
                         ids=["%dx%dx%dx%d" % c[1] for c in POOL_CASES] + ["1x1"])
def test_avgpool(gpu, shape, dt):
    # (+0.5: a mean that is not a cancellation, so the relative bound is about the kernel)
    x64 = (_pool_x(shape, dt) + 0.5).to(DTYPES[dt]).double()
    e, de = _avgpool_run(gpu, x64, dt, _seed("avgg", shape))
    print("avgpool", shape, dt, "%.3e %.3e" % (e, de))
    assert e < _bound(dt, 1e-6) and de < _bound(dt, 1e-6)


def test_pool_grid_stride(gpu):
    """bf16, one tensor of 2,163,200 elements: the grid-stride loops of maxpool_fwd / _bwd (k3 s1
    p1 keeps the map size) and avgpool_bwd take a second pass."""
    dt = "bf16"
    x64 = (_pool_x(POOL_BIG, dt) + 0.5).to(DTYPES[dt]).double()
    assert x64.numel() > 8192 * 256
    y, dx, yr, dxr = _maxpool_run(gpu, (3, 1, 1), x64, dt, _seed("poolg-big"))
    np.testing.assert_array_equal(_bits(y), _bits(yr.to(DTYPES[dt])))
    assert rel(dx, dxr) < ROUND16[dt]
    e, de = _avgpool_run(gpu, x64, dt, _seed("avgg-big"))
    print("pool grid-stride avg", "%.3e %.3e" % (e, de))
    assert e < ROUND16[dt] and de < ROUND16[dt]


# --------------------------------------------------------------------------- bn_fold --
FOLD_SHAPES = [(37, 5, 3, 3), (960, 1, 3, 3), (8, 300, 1, 1)]


def _fold_case(shape, with_bias):
    O, I, kh, kw = shape
    gen = _seed("fold", shape)
    w = torch.randn(O, I, kh, kw, generator=gen).double()
    b = torch.randn(O, generator=gen).double() if with_bias else None
    bn = torch.nn.BatchNorm2d(O).double().eval()
    with torch.no_grad():
        bn.weight.copy_(1 + 0.3 * torch.randn(O, generator=gen))
        bn.bias.copy_(torch.randn(O, generator=gen))
        bn.running_mean.copy_(torch.randn(O, generator=gen))
        bn.running_var.copy_(0.2 + torch.rand(O, generator=gen))
    groups = O if I == 1 else 1
    x = torch.randn(2, I * groups, 6, 5, generator=gen, dtype=torch.float64)
    with torch.no_grad():
        yref = bn(F.conv2d(x, w, b, 1, kh // 2, groups=groups))
    return w, b, bn, x, yref, groups


def _fold_assert(shape, wf, bf, w, b, bn, x, yref, groups):
    with torch.no_grad():
        sc = bn.weight / torch.sqrt(bn.running_var + bn.eps)
        assert rel(wf, w * sc.view(-1, 1, 1, 1)) < 1e-6
        assert rel(bf, ((b if b is not None else 0) - bn.running_mean) * sc + bn.bias) < 1e-6
        assert rel(F.conv2d(x, wf, bf, 1, shape[2] // 2, groups=groups), yref) < 1e-6


@pytest.mark.parametrize("variant", ["wrapper", "wrapper-nobias", "wrapper-cl", "abi-alias", "abi-cl-nobias"])
@pytest.mark.parametrize("shape", FOLD_SHAPES, ids=["37x5x3x3", "960x1x3x3", "8x300x1x1"])
def test_bn_fold(gpu, shape, variant):
    """Reference: an eval-mode nn.BatchNorm2d in fp64 applied after the conv (all parameters are
    drawn in float32, so the fp64 reference sees what the kernel loads).  tpgan_ops.bn_fold
    never aliases its output with the weight, so in-place folding (w_out = w) goes through the
    C ABI here; 'cl' is a channels-last (strided) weight."""
    import copy
    import tpgan_ops as T
    from tpgan_lib import check, load, stream_ptr, tt
    lib = load()
    O, I, kh, kw = shape
    with_bias = "nobias" not in variant
    w, b, bn, x, yref, groups = _fold_case(shape, with_bias)
    wg = w.float().to(gpu)
    if "cl" in variant:
        wg = wg.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)  # logical OIHW, memory OHWI
        assert wg.stride(1) == 1 or I == 1
    bg = b.float().to(gpu) if with_bias else None
    bng = copy.deepcopy(bn).float().to(gpu)
    if variant.startswith("wrapper"):
        with torch.no_grad():
            wf, bf = T.bn_fold(wg, bg, bng)
        torch.cuda.synchronize()
        assert wf.stride() == wg.stride() and wf.data_ptr() != wg.data_ptr()
        assert torch.equal(wg.cpu(), w.float().permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
                           if "cl" in variant else w.float())
    else:
        wf = wg if "alias" in variant else torch.full_like(wg, float("nan"))
        bf = torch.full((O,), float("nan"), dtype=torch.float32, device=gpu)
        check(lib.tpg_bn_fold(O, I, kh, kw, tt(wg), _ptr(bg), _ptr(bng.weight.detach()), _ptr(bng.bias.detach()),
                              _ptr(bng.running_mean), _ptr(bng.running_var), float(bng.eps), tt(wf), _ptr(bf),
                              stream_ptr()))
        torch.cuda.synchronize()
    _fold_assert(shape, wf.double().cpu(), bf.double().cpu(), w, b, bn, x, yref, groups)
