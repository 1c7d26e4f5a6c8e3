"""Op-level parity of the LocalFuser (fuse_fwd_kernel / fuse_bwd_kernel) and fc2's maxout
(maxout_fwd_kernel / maxout_bwd_kernel) of csrc/tpg_elementwise.hip, each alone through tpgan_ops.

Both are selections: the output is one of the (dtype-rounded) inputs or the zero canvas, a gradient
element is the incoming gradient or 0.  So everything is compared bit for bit, in every dtype, NaN
positions as masks -- there is no bound to derive and none to fit.

The LocalFuser reference is numpy in float64 on the rounded parts: four zero canvases, each part
pasted at (top, left) and clipped to the canvas, np.argmax over the stack (the first maximum wins,
so the lower part index wins a tie, and the first NaN wins: LocalFuser's docstring, torch.max);
gy at a pixel goes to the winning part only where that part covers the pixel, so a pixel whose
covering values are all negative gives 0 (the canvas of a part that does not cover it wins) and
routes its gradient nowhere.  maxout2 is max(x[:, 0::2], x[:, 1::2]), the first on ties.
"""
import numpy as np
import pytest
import torch

from test_gpu_elementwise import DTYPES, _assert_same_bits, _seed

pytestmark = pytest.mark.gpu

PROD = dict(hw=(128, 128), sizes=((40, 40), (40, 40), (32, 40), (32, 48)), tops=(19, 18, 47, 72), lefts=(18, 65, 43, 40))
# a 20 x 24 canvas: part 0 starts above / left of it (negative top and left) and overlaps part 1,
# part 3 overlaps part 1, part 2 runs past the bottom / right edge, rows 12.. of columns 0..7 and
# the top right corner are covered by no part
SMALL = dict(hw=(20, 24), sizes=((8, 10), (9, 9), (7, 8), (6, 6)), tops=(-3, 2, 15, 6), lefts=(-2, 4, 18, 8))
# the product placements on a canvas one column wider: 2 * 64 * 128 * 129 = 2,113,536 elements
BIG = dict(PROD, hw=(128, 129))


def _fuse_ref(parts, gy, hw, tops, lefts):
    """(y, [dpart]) in float64 numpy, by the module docstring."""
    OH, OW = hw
    N, C = parts[0].shape[:2]
    canv = np.zeros((4, N, C, OH, OW))
    cover = np.zeros((4, OH, OW), bool)
    for k, p in enumerate(parts):
        ph, pw = p.shape[2:]
        y0, y1, x0, x1 = max(tops[k], 0), min(tops[k] + ph, OH), max(lefts[k], 0), min(lefts[k] + pw, OW)
        canv[k, :, :, y0:y1, x0:x1] = p[:, :, y0 - tops[k]:y1 - tops[k], x0 - lefts[k]:x1 - lefts[k]]
        cover[k, y0:y1, x0:x1] = True
    arg = np.argmax(canv, axis=0)
    y = np.take_along_axis(canv, arg[None], 0)[0]
    grads = []
    for k, p in enumerate(parts):
        ph, pw = p.shape[2:]
        y0, y1, x0, x1 = max(tops[k], 0), min(tops[k] + ph, OH), max(lefts[k], 0), min(lefts[k] + pw, OW)
        g = np.zeros(p.shape)
        win = (arg[:, :, y0:y1, x0:x1] == k) & cover[k, y0:y1, x0:x1]
        g[:, :, y0 - tops[k]:y1 - tops[k], x0 - lefts[k]:x1 - lefts[k]] = np.where(win, gy[:, :, y0:y1, x0:x1], 0.0)
        grads.append(g)
    return y, grads, arg, cover


def _to_dev(v, dtype, gpu, cl):
    import tpgan_ops as T
    t = v.to(dtype).to(gpu)
    if not cl:
        return t.contiguous()
    b = T.new_act(*t.shape, dtype=dtype, device=gpu)
    b.copy_(t)
    return b


def _run_fuse(gpu, geo, n, c, dt, gy_cl, nograd=(), plant=None, key=""):
    import tpgan_ops as T
    dtype = DTYPES[dt]
    gen = _seed("fuse", geo["hw"], n, c, dt, key)
    parts = [(torch.rand(n, c, h, w, generator=gen, dtype=torch.float64) * 2 - 1).to(dtype) for h, w in geo["sizes"]]
    if plant:
        plant(parts)
    gy = (torch.rand(n, c, *geo["hw"], generator=gen, dtype=torch.float64) * 2 - 1).to(dtype)
    # parts 0 / 2 channels-last activations (the local pathways' outputs), 1 / 3 plain NCHW
    dev = [_to_dev(p, dtype, gpu, k % 2 == 0).requires_grad_(k not in nograd) for k, p in enumerate(parts)]
    with T.compute_dtype(dtype):
        y = T.local_fuse(dev, geo["hw"], geo["tops"], geo["lefts"])
    y.backward(_to_dev(gy, dtype, gpu, gy_cl))
    torch.cuda.synchronize()
    want_y, want_g, arg, cover = _fuse_ref([p.double().numpy() for p in parts], gy.double().numpy(), geo["hw"],
                                           geo["tops"], geo["lefts"])
    assert y.dtype == dtype
    _assert_same_bits(y.detach().cpu().contiguous(), torch.from_numpy(want_y).to(dtype), "fuse y")
    for k, (d, g) in enumerate(zip(dev, want_g)):
        if k in nograd:
            assert d.grad is None
            continue
        assert d.grad.dtype == dtype
        _assert_same_bits(d.grad.cpu().contiguous(), torch.from_numpy(g).to(dtype), "fuse grad %d" % k)
    return parts, want_y, want_g, arg, cover


def _plant_small(parts):
    """Exact ties between overlapping parts (1 and 3: canvas rows 6..7, columns 8..12; 0 and 1:
    canvas row 2, columns 4..7), of both signs, and one NaN in part 1 under part 0."""
    parts[3][:, :, 0:2, 0:5] = parts[1][:, :, 4:6, 4:9]
    parts[1][:, :, 0, 0:4] = parts[0][:, :, 5, 6:10]
    parts[1][0, 0, 1, 1] = float("nan")


@pytest.mark.parametrize("gy_cl", [False, True], ids=["gy-nchw", "gy-cl"])
@pytest.mark.parametrize("dt", ["f32", "bf16", "f16"])
@pytest.mark.parametrize("c", [3, 1, 13])  # 13: a channel tail on the padded 16-channel pixel row
def test_local_fuse_small_canvas(gpu, c, dt, gy_cl):
    """Clipping on all four sides, overlaps, an uncovered region, ties, NaN, negative-only pixels."""
    n = 2
    parts, y, grads, arg, cover = _run_fuse(gpu, SMALL, n, c, dt, gy_cl, plant=_plant_small)
    p = [t.double().numpy() for t in parts]
    # what the case is meant to contain (checked on the reference, which the kernel matched bit for bit)
    assert not cover.any(0).all() and cover.sum(0).max() >= 2
    assert np.isnan(y[0, 0, 3, 5]) and grads[1][0, 0, 1, 1] != 0 and grads[0][0, 0, 6, 7] == 0  # the NaN and its gradient
    tie = p[3][:, :, 0:2, 0:5] == p[1][:, :, 4:6, 4:9]
    assert tie.all()
    pos = p[1][:, :, 4:6, 4:9] > 0  # a positive tie: part 1 (the lower index) takes the gradient, part 3 none
    assert pos.any() and (grads[3][:, :, 0:2, 0:5][pos] == 0).all() and (grads[1][:, :, 4:6, 4:9][pos] != 0).all()
    # a pixel covered only by part 2, negative there: output 0, no gradient to any part
    only2 = cover[2] & ~cover[0] & ~cover[1] & ~cover[3]
    neg = (p[2][:, :, :5, :6] < 0) & only2[15:20, 18:24]
    assert neg.any() and (y[:, :, 15:20, 18:24][neg] == 0).all() and (grads[2][:, :, :5, :6][neg] == 0).all()
    assert (y[:, :, ~cover.any(0)] == 0).all()


@pytest.mark.parametrize("dt", ["f32", "bf16", "f16"])
def test_local_fuse_product_geometry(gpu, dt):
    """The 128 x 128 placements at N = 1, C = 8; the mouth (part 3) takes no gradient."""
    _run_fuse(gpu, PROD, 1, 8, dt, True, nograd=(3,))


def test_local_fuse_second_pass(gpu):
    """2,113,536 canvas elements > grid_for's 8192 x 256 = 2,097,152: the forward's grid-stride loop
    runs a second, ragged pass.  (The largest part has 196,608 elements: the backward never does.)"""
    assert 2 * 64 * 128 * 129 > 8192 * 256 > 2 * 64 * 32 * 48
    _run_fuse(gpu, BIG, 2, 64, "bf16", True)


# ------------------------------------------------------------------------------- maxout --
def _maxout_ref(x, gy):
    m = x.shape[1] // 2
    x0, x1 = x[:, 0:2 * m:2], x[:, 1:2 * m:2]
    second = (x1 > x0) | (np.isnan(x1) & ~np.isnan(x0))
    dx = np.zeros(x.shape)
    dx[:, 0:2 * m:2] = np.where(second, 0.0, gy)
    dx[:, 1:2 * m:2] = np.where(second, gy, 0.0)
    return np.where(second, x1, x0), dx


def _run_maxout(gpu, b, k, dt, sliced=False, key=""):
    import tpgan_ops as T
    dtype = DTYPES[dt]
    gen = _seed("maxout", b, k, dt, key)
    x = (torch.randn(b, k, generator=gen, dtype=torch.float64)).to(dtype)
    m = k // 2
    x[:, 1:2 * m:6] = x[:, 0:2 * m:6]  # ties in every third pair: the first takes the gradient
    if m > 2:  # a NaN second of a pair, and a NaN first of one in the last row
        x[0, 3] = float("nan")
        x[b - 1, 4] = float("nan")
    gy = (torch.rand(b, m, generator=gen, dtype=torch.float64) + 0.5).to(dtype)
    if sliced:  # columns [3, 3 + k) of a wider row: a row stride that is not k, a shifted pointer
        wide = torch.full((b, k + 8), 9.0, dtype=dtype, device=gpu)
        xd = wide[:, 3:3 + k]
        xd.copy_(x.to(gpu))
    else:
        xd = x.to(gpu)
    xd.requires_grad_(True)
    y = T.maxout2(xd)
    gyd = gy.to(gpu)
    # the gradient buffer comes from the caching allocator: hand it a block of NaN, so that a
    # column the backward leaves unwritten shows
    junk = torch.full((b, k), float("nan"), dtype=dtype, device=gpu)
    del junk
    y.backward(gyd)
    torch.cuda.synchronize()
    want_y, want_dx = _maxout_ref(x.double().numpy(), gy.double().numpy())
    assert tuple(y.shape) == (b, m) and y.dtype == dtype
    _assert_same_bits(y.detach().cpu(), torch.from_numpy(want_y).to(dtype), "maxout y")
    _assert_same_bits(xd.grad.cpu().contiguous(), torch.from_numpy(want_dx).to(dtype), "maxout dx")
    assert (want_dx != 0).sum() == b * m  # every pair routes its (non-zero) gradient to exactly one side
    return want_dx


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("b,k", [(3, 512), (1, 2)], ids=["3x512", "1x2"])
def test_maxout2(gpu, b, k, dt):
    _run_maxout(gpu, b, k, dt)


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_maxout2_column_slice(gpu, dt):
    _run_maxout(gpu, 3, 12, dt, sliced=True)


def test_maxout2_second_pass(gpu):
    """5 x 419,431 pairs = 2,097,155 > 8192 x 256: three elements of the forward and half of the
    backward's 4,194,310 run in a second grid-stride pass."""
    assert 5 * 419_431 > 8192 * 256
    _run_maxout(gpu, 5, 2 * 419_431, "f32")


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_maxout2_odd_width(gpu, dt):
    """k = 7: MaxPool1d(2, 2) drops the last feature, so its gradient is exactly 0 (it was
    uninitialised memory: _Maxout2.backward now zeroes the column the kernel does not write)."""
    dx = _run_maxout(gpu, 3, 7, dt)
    assert (dx[:, 6] == 0).all()
