"""GPU: the fused G-step losses (tpg_losses.hip via tpgan_ops.image_losses / l1_means) against
their torch fp64 restatement on the CPU -- the same formulas tpgan_train._g_losses computed with
aten before (build-defined; weights config.py:59-82): values, gradients,
16-bit channels-last inputs with padded pixel rows, odd widths and one-row maps, and
bit-identical reruns (fixed-order reductions).

The reference is float64 autograd of the formula on the values the kernel reads (the inputs
rounded to their dtype, read back), so it differs from the kernel only by the kernel's own fp32
arithmetic and the one rounding of each gradient element to the input's dtype:
  value     1e-5 relative (the project's bound for fp32 sums; every term is a positive weight
            times a sum of absolute values, so nothing cancels)
  gradient  fp32 1e-6 relative L2; bf16 2^-8, fp16 2^-11: the unit roundoff of the one rounding of
            each element to its dtype (ACTB_G_BOUND of test_gpu_ops.py).  A gradient takes few
            distinct values (weight / count times a small integer), so the error is not averaged
            over many roundings: a value just above a power of two sits at nearly the whole bound.
            The signs are exact: the fp32 difference of two representable values has the sign of
            the exact difference, and sign(0) = 0 as torch's abs backward.
fp16 keeps that relative rounding only for normal numbers (>= 2^-14): the weights of a case grow
with its element count (_weights) so that a gradient element, weight / count, stays there.
"""
import pytest
import torch

from _cases import rel

pytestmark = pytest.mark.gpu

DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
G_BOUND = {torch.float32: 1e-6, torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
BIG = (2, 3, 150, 147)  # 132,300 elements > the 512 x 256 = 131,072 threads of the partial-sum grid


def _img_ref(x, r, wp, ws, wt):
    tv = (x[:, :, 1:, :] - x[:, :, :-1, :]).abs().mean() if x.shape[2] > 1 else x.new_zeros(())
    tv = tv + ((x[:, :, :, 1:] - x[:, :, :, :-1]).abs().mean() if x.shape[3] > 1 else x.new_zeros(()))
    return wp * (x - r).abs().mean() + ws * (x - x.flip(3)).abs().mean() + wt * tv


def _dev_input(x64, dtype, gpu, cl):
    t = x64.to(dtype).to(gpu)
    if cl:  # the conv output layout: channels last, pixel rows padded to 8 channels
        import tpgan_ops
        n, c, h, w = t.shape
        b = tpgan_ops.new_act(n, c, h, w, dtype, gpu)
        b.copy_(t)
        t = b
    return t


def _layout(x64, dtype, gpu, layout):
    """x64 rounded to `dtype` on the device as: "nchw" contiguous; "cl" a new_act buffer (channels
    last, pixel rows padded to 8 channels); "slice" channels [1, 1 + C) of a new_act buffer three
    channels wider (the data pointer is not the buffer's, the pixel row holds other channels)."""
    import tpgan_ops
    t = x64.to(dtype).to(gpu)
    if layout == "nchw":
        return t.contiguous()
    n, c, h, w = t.shape
    if layout == "cl":
        b = tpgan_ops.new_act(n, c, h, w, dtype, gpu)
    else:
        wide = tpgan_ops.new_act(n, c + 3, h, w, dtype, gpu)
        wide.fill_(7.0)  # (the neighbours of the slice: never read, never written)
        b = wide[:, 1:1 + c]
        b.wide = wide
    b.copy_(t)
    return b


def _weights(shape):
    """(w_pix, w_sym, w_tv), all positive, in the ratio 1.7 : 0.3 : 0.25 and grown with the element
    count beyond 4096, so that a gradient element (about weight / count) is a normal fp16 number."""
    n, c, h, w = shape
    s = max(1.0, n * c * h * w / 4096.0)
    return 1.7 * s, 0.3 * s, 0.25 * s


def _rand(shape, gen):
    return torch.rand(shape, generator=gen, dtype=torch.float64) * 2 - 1


def _check_image_losses(x, r, shape, gscale, what):
    """image_losses(x, r) and its gradient under an incoming scale against float64 autograd of
    _img_ref on the same values; a rerun gives the same bits.  Returns the measured errors."""
    import tpgan_ops
    wp, ws, wt = _weights(shape)
    x.requires_grad_(True)
    y = tpgan_ops.image_losses(x, r, wp, ws, wt)
    (y * gscale).backward()
    xr = x.detach().double().cpu().requires_grad_(True)  # the same (rounded) input values
    yr = _img_ref(xr, r.double().cpu(), wp, ws, wt)
    (yr * gscale).backward()
    ev = abs(y.item() - yr.item()) / abs(yr.item())
    eg = rel(x.grad.double().cpu(), xr.grad)
    print("image_losses %s: value %.2e grad %.2e" % (what, ev, eg))
    assert x.grad.dtype == x.dtype and tuple(x.grad.shape) == tuple(x.shape)
    assert ev <= 1e-5, what
    assert eg < G_BOUND[x.dtype], what
    y2 = tpgan_ops.image_losses(x.detach(), r, wp, ws, wt)
    assert torch.equal(y.detach(), y2)  # fixed-order reduction
    return xr


# measured on the MI355X, largest over the six shapes (value, gradient) -- f32: 1.1e-7, 9.2e-8;
# bf16: 8.4e-8, 1.8e-3 (bound 3.9e-3); f16: 4.8e-8, 2.7e-4 (bound 4.9e-4)
@pytest.mark.parametrize("shape", [
    (4, 3, 32, 32),  # 48 blocks, even width
    (2, 3, 17, 13),  # odd width: the middle column is its own mirror (sign(0) of the symmetry term)
    (3, 2, 1, 9),    # one row: no vertical TV (ky = 0, the term's mean is over no element)
    BIG,             # a second grid-stride pass with a ragged tail (1,228 elements), odd width
    (1, 1, 3, 5),    # one block, 15 live threads, C = 1
    (2, 2, 9, 1),    # w == 1: the symmetry term is identically 0, no horizontal TV (kx = 0)
], ids=["32", "odd", "1row", "2pass", "1block", "w1"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16], ids=["f32", "bf16", "f16"])
def test_image_losses(gpu, shape, dtype):
    g = torch.Generator().manual_seed(11)
    x64, r64 = _rand(shape, g), _rand(shape, g)
    x = _dev_input(x64, dtype, gpu, dtype != torch.float32)
    _check_image_losses(x, r64.float().to(gpu), shape, 2.5, "%s %s" % (shape, dtype))


# measured: value <= 5.8e-8; gradient f32 4.8e-8, bf16 1.9e-3, f16 3.0e-4 (the layouts change addresses only)
@pytest.mark.parametrize("shape,dt,layout,rkind,gscale", [
    ((2, 3, 17, 13), "bf16", "nchw", "f32", 1.0),      # 16-bit x with W-contiguous rows; dx contiguous
    ((2, 3, 17, 13), "f16", "nchw", "bf16cl", -2.5),   # the same in fp16, r read as bf16 channels-last
    ((2, 3, 17, 13), "bf16", "slice", "bf16cl", -2.5),  # x a channel slice [:, 1:4] of a 6-channel buffer
    ((2, 3, 17, 13), "f16", "slice", "f32", 1.0),
    ((2, 3, 17, 13), "f32", "slice", "bf16cl", 1.0),   # fp32 channels-last x, 16-bit r
    ((2, 3, 17, 13), "f32", "cl", "f32", -2.5),
    (BIG, "bf16", "slice", "bf16cl", -2.5),            # the second pass through non-trivial strides
    (BIG, "f16", "nchw", "f32", 1.0),
    ((1, 1, 3, 5), "bf16", "cl", "bf16cl", 1.0),       # C = 1 in an 8-channel pixel row
    ((2, 2, 9, 1), "f16", "slice", "bf16cl", -2.5),    # w == 1 on a slice
    ((3, 2, 1, 9), "bf16", "nchw", "f32", -2.5),       # one row, NCHW 16-bit
], ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_image_losses_layouts(gpu, shape, dt, layout, rkind, gscale):
    g = torch.Generator().manual_seed(13)
    x64, r64 = _rand(shape, g), _rand(shape, g)
    x = _layout(x64, DTYPES[dt], gpu, layout)
    r = r64.float().to(gpu) if rkind == "f32" else _layout(r64, torch.bfloat16, gpu, "cl")
    _check_image_losses(x, r, shape, gscale, "%s %s %s r=%s g=%s" % (shape, dt, layout, rkind, gscale))
    if layout == "slice":  # the channels around the slice keep their fill
        c = shape[1]
        assert bool((x.wide[:, 0] == 7.0).all()) and bool((x.wide[:, 1 + c:] == 7.0).all())


@pytest.mark.parametrize("dt", ["f32", "bf16", "f16"])
def test_image_losses_planted_zeros(gpu, dt):
    """(measured: value <= 6.9e-8; gradient f32 4.6e-8, bf16 1.7e-3, f16 2.0e-4.)
    Exact zeros of every difference the loss takes, planted after rounding to the dtype (copies
    of representable values): x == r, mirror-equal pairs, vertically and horizontally equal
    neighbours.  torch's abs backward gives 0 there (the reference is autograd of _img_ref); a
    kernel with sign(0) = +-1 is off by a whole weight / count on each such element."""
    dtype = DTYPES[dt]
    shape = (2, 3, 17, 13)
    g = torch.Generator().manual_seed(17)
    x0 = _rand(shape, g).to(dtype).double()
    r0 = _rand(shape, g).float().double()
    # mirror-equal pairs: rows 2..4 are palindromes
    half = x0[:, :, 2:5, :6].clone()
    x0[:, :, 2:5, 7:] = half.flip(3)
    # vertically equal neighbours: row 9 repeats row 8; horizontally equal: column 4 repeats column 3
    x0[:, :, 9, :] = x0[:, :, 8, :]
    x0[:, :, 11:, 4] = x0[:, :, 11:, 3]
    # x == r on a block (r is fp32: it holds every 16-bit value exactly)
    r0[:, 1, 12:16, 5:11] = x0[:, 1, 12:16, 5:11]
    assert torch.equal(x0.to(dtype).double(), x0)
    x = _dev_input(x0, dtype, gpu, dtype != torch.float32)
    xr = _check_image_losses(x, r0.float().to(gpu), shape, -2.5, "planted zeros " + dt)
    xv = xr.detach()
    assert int((xv == r0).sum()) >= 2 * 4 * 6
    assert int((xv == xv.flip(3)).sum()) >= 2 * 3 * 3 * 13
    assert int((xv[:, :, 1:] == xv[:, :, :-1]).sum()) >= 2 * 3 * 13
    assert int((xv[:, :, :, 1:] == xv[:, :, :, :-1]).sum()) >= 2 * 3 * 6


# ------------------------------------------------------------------------------ l1_means --
def _l1_run(gpu, segs, weights, gscale, what):
    """segs: (shape, a dtype, a layout, b dtype, a requires grad, planted a == b).  Returns the
    measured errors after asserting the bounds of the module docstring."""
    import tpgan_ops
    g = torch.Generator().manual_seed(5)
    pairs, refs = [], []
    for shape, adt, alay, bdt, needs, plant in segs:
        a64 = _rand(shape, g).to(DTYPES[adt]).double()
        b64 = _rand(shape, g).to(DTYPES[bdt]).double()
        if plant:  # every third element: a == b exactly (both dtypes hold the fp32-rounded bf16 value)
            eq = a64.to(torch.bfloat16).double()
            m = (torch.arange(a64.numel()) % 3 == 0).reshape(shape)
            a64 = torch.where(m, eq, a64)
            b64 = torch.where(m, eq, b64)
        a = _layout(a64, DTYPES[adt], gpu, alay).requires_grad_(needs)
        b = _layout(b64, DTYPES[bdt], gpu, "nchw")
        pairs.append((a, b))
        refs.append((a64.clone().requires_grad_(needs), b64))
        assert torch.equal(a.detach().double().cpu(), a64) and torch.equal(b.double().cpu(), b64)
    y = tpgan_ops.l1_means(pairs, weights)
    (y * gscale).backward()
    means = [(a - b).abs().mean() for a, b in refs]
    yr = sum(w * m for w, m in zip(weights, means))
    (yr * gscale).backward()
    scale = sum(abs(w) * float(m) for w, m in zip(weights, means))
    ev = abs(y.item() - float(yr)) / scale
    assert ev <= 1e-5, what
    errs = []
    for k, ((a, _), (ar, _)) in enumerate(zip(pairs, refs)):
        if not a.requires_grad:
            assert a.grad is None
            continue
        assert a.grad.dtype == a.dtype
        e = rel(a.grad.double().cpu(), ar.grad)
        errs.append(e)
        assert e < G_BOUND[a.dtype], (what, k, e)
    print("l1_means %s: value %.2e grads %s" % (what, ev, ["%.1e" % e for e in errs]))
    y2 = tpgan_ops.l1_means([(a.detach(), b) for a, b in pairs], weights)
    assert torch.equal(y.detach(), y2)  # fixed-order reduction
    return refs


def test_l1_means(gpu):
    """The product call: four bf16 channels-last local patches against fp32 crops."""
    shapes = [(4, 3, 40, 40), (4, 3, 40, 40), (4, 3, 32, 40), (4, 3, 32, 48)]
    _l1_run(gpu, [(s, "bf16", "cl", "f32", True, False) for s in shapes], [0.25, 0.5, 0.75, 1.0], 1.0, "product")


# measured -- value <= 9.0e-8 of sum |w_i| mean_i; gradients f32 <= 4.8e-8, f16 2.4e-5, bf16 <= 3.1e-3
# (the 132,300-element segment: every element is +-40 / 132,300, whose bf16 rounding alone is 3.1e-3)
L1_CASES = {
    # one segment: l1_seg's loop body never runs
    "1seg": ([((2, 3, 5, 7), "f32", "nchw", "f32", True, True)], [0.7], 1.0),
    # eight segments of different shapes, layouts and dtypes: a zero and a negative weight, planted
    # a == b (sign 0), a f32 against b bf16, and segment 3 without a gradient (NULL da) between
    # two that have one
    "8seg": ([((1, 2, 3, 5), "bf16", "cl", "f32", True, True),
              ((2, 3, 4, 4), "f32", "nchw", "bf16", True, True),
              ((1, 1, 7, 3), "f16", "cl", "f32", True, False),
              ((2, 2, 5, 5), "bf16", "slice", "f32", False, True),
              ((1, 3, 2, 9), "f16", "nchw", "f16", True, True),
              ((3, 1, 1, 1), "f32", "cl", "f32", True, False),
              ((1, 4, 6, 2), "bf16", "nchw", "bf16", True, False),
              ((2, 3, 3, 3), "f32", "slice", "f32", True, True)],
             [0.25, -1.5, 0.0, 2.0, 1.0, 0.5, -0.125, 3.0], -2.5),
    # a one-element segment first (the first block straddles two segments after its first thread),
    # then 132,300 elements: the boundary to the last segment lies in the second grid-stride pass
    # (element 132,301 > 131,072), inside a block; the weight of the big segment grows with its
    # count (_weights' reason), the last one has no gradient
    "ragged": ([((1, 1, 1, 1), "f32", "nchw", "f32", True, False),
                (BIG, "bf16", "cl", "f32", True, True),
                ((2, 3, 9, 11), "f32", "nchw", "bf16", True, True),
                ((1, 2, 3, 3), "bf16", "cl", "f32", False, False)],
               [1.0, 40.0, -0.5, 1.0], 1.0),
}


@pytest.mark.parametrize("name", list(L1_CASES))
def test_l1_means_cases(gpu, name):
    segs, weights, gscale = L1_CASES[name]
    refs = _l1_run(gpu, segs, weights, gscale, name)
    if any(s[5] for s in segs):
        assert any(bool((a.detach() == b).any()) for a, b in refs)


def test_l1_means_rejects_nine(gpu):
    import tpgan_ops
    pairs = [(torch.zeros(1, 1, 2, 2, device=gpu), torch.zeros(1, 1, 2, 2, device=gpu)) for _ in range(9)]
    with pytest.raises(ValueError):
        tpgan_ops.l1_means(pairs, [1.0] * 9)
    with pytest.raises(ValueError):
        tpgan_ops.l1_means(pairs[:8], [1.0] * 7)
