"""CPU: the plan of the dense five-tap weight-gradient tile (desc.algo 14, tile index 8 of
tp-gan_amd/csrc/tpg_wgrad_rh.hip) through tpg_conv2d_wgrad_plan: the channel tiles and pixel
splits on the four 5x5 layers of the step, every refusal (-30, message set, caller's struct
untouched), deterministic mode, and the untuned plans it must not have moved."""
import ctypes
import importlib.util
import json
import os

import pytest

import tpgan_lib as L

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DENSE5_ALGO, DENSE5_TILE = 14, 8
ROW_HALO = L.WGRAD_KERNELS.index("row_halo")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(L.LIB_PATH):
        pytest.skip("libtpgan_hip.so not built")
    lib = ctypes.CDLL(L.LIB_PATH)
    for name in ("tpg_conv2d_wgrad_plan", "tpg_set_deterministic", "tpg_last_error"):
        getattr(lib, name).restype, getattr(lib, name).argtypes = L.EXPORTS[name]
    return lib


@pytest.fixture(scope="module")
def gen():
    spec = importlib.util.spec_from_file_location("make_wgrad_plans",
                                                  os.path.join(REPO, "tests", "golden", "make_wgrad_plans.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    return gen


def _plan(gen, lib, shape, dtype, layout=0, det=0, algo=DENSE5_ALGO, ks=1):
    got = gen.query(L, lib, shape, dtype, layout, 0, det, algo, ks)
    return got[0] if len(got) == 1 else dict(zip(gen.PLAN_FIELDS, got))


# name: (n, in_c, h, w, out_c), a-tile (dY channels), b-tile (X channels), a-tiles x b-tiles
# channel tiles: n = ceil(C / 112) tiles of ceil(C / n) channels rounded up to 16
LAYERS = {
    "enhance_128": ((32, 206, 128, 128, 206), 112, 112, 2 * 2),
    "add_64": ((32, 80, 64, 64, 80), 80, 80, 1),
    "conv5_0": ((32, 206, 128, 128, 64), 64, 112, 1 * 2),
    "conv64_64": ((32, 64, 64, 64, 64), 64, 64, 1),
}


@pytest.mark.parametrize("dtype", [L.TPG_BF16, L.TPG_F16], ids=["bf16", "f16"])
@pytest.mark.parametrize("layer", sorted(LAYERS))
def test_dense5_plan_on_layer(lib, gen, layer, dtype):
    (n, ci, h, w, co), tm, tn, ntiles = LAYERS[layer]
    shape = gen.conv(n, ci, h, w, co, 5, 1, 2)
    nkt = n * h * (w // 64)  # 64-pixel row segments
    for ks in (1, 4, 12, nkt, nkt + 1, 1 << 20):
        per = -(-nkt // min(ks, nkt))  # the split rounds to whole k-tile groups
        splits = -(-nkt // per)
        assert splits == (ks if ks <= nkt else nkt)
        p = _plan(gen, lib, shape, dtype, ks=ks)
        assert p["kernel"] == ROW_HALO and p["cfg"] == DENSE5_TILE, (ks, p)
        assert (p["tile_m"], p["tile_n"]) == (tm, tn) and p["taps_per_block"] == 5, (ks, p)
        assert p["tiles"] == ntiles * 5, (ks, p)                           # per kernel row and (a, b) tile
        assert p["splits"] == splits and p["per_split"] == per, (ks, p)
        assert p["flags"] & 1 and not p["flags"] & 16, (ks, p)             # sums the bias; no dead-block skip
        nshare = p["tiles"] // -(-co // tm)                                # (b, row) tiles of one a-tile
        assert 1 <= p["bias_share"] <= nshare and p["bias_share"] * p["splits"] <= max(16, p["splits"]), (ks, p)


def test_dense5_plan_split_model_and_small_shapes(lib, gen):
    # no split asked for: whole rounds of 256 resident blocks, 20 tiles x 12 (or 13) on enhance_128
    p = _plan(gen, lib, gen.conv(32, 206, 128, 128, 206, 5, 1, 2), L.TPG_BF16, ks=0)
    assert p["cfg"] == DENSE5_TILE and p["tiles"] == 20 and p["splits"] in (12, 13), p
    # 6 k-tiles asked for 3 splits are 2 / 2 / 2, 14 are 5 / 5 / 4
    p = _plan(gen, lib, gen.conv(2, 206, 3, 64, 206, 5, 1, 2), L.TPG_BF16, ks=3)
    assert (p["splits"], p["per_split"], p["tiles"]) == (3, 2, 20), p
    p = _plan(gen, lib, gen.conv(2, 80, 7, 64, 80, 5, 1, 2), L.TPG_BF16, ks=3)
    assert (p["splits"], p["per_split"], p["tiles"]) == (3, 5, 5), p
    # odd channel counts: 17 -> one tile of 32, 113 -> two of 64
    p = _plan(gen, lib, gen.conv(2, 113, 3, 64, 17, 5, 1, 2), L.TPG_BF16)
    assert (p["tile_m"], p["tile_n"], p["tiles"]) == (32, 64, 2 * 5), p
    p = _plan(gen, lib, gen.conv(2, 17, 3, 64, 113, 5, 1, 2), L.TPG_BF16)
    assert (p["tile_m"], p["tile_n"], p["tiles"]) == (64, 32, 2 * 5), p
    # a non-square 5-wide kernel: still one block per kernel row
    s = list(gen.conv(2, 80, 8, 64, 64, 5, 1, 2))
    s[gen.SHAPE_FIELDS.index("kh")] = 3
    s[gen.SHAPE_FIELDS.index("pad_t")] = s[gen.SHAPE_FIELDS.index("pad_b")] = 1
    p = _plan(gen, lib, tuple(s), L.TPG_BF16, ks=2)
    assert p["cfg"] == DENSE5_TILE and p["tiles"] == 3 and p["splits"] == 2, p


def test_dense5_plan_deterministic(lib, gen):
    shape = gen.conv(32, 206, 128, 128, 206, 5, 1, 2)
    for ks in (0, 1, 12, 1 << 20):
        p = _plan(gen, lib, shape, L.TPG_BF16, det=1, ks=ks)
        assert p["cfg"] == DENSE5_TILE and p["splits"] == 1 and p["bias_share"] == 1 and p["tiles"] == 20, (ks, p)
        assert p["per_split"] == 32 * 128 * 2, (ks, p)


REFUSED = {
    "kw_7": (lambda g: g.conv(2, 75, 8, 64, 75, 7, 1, 3), L.TPG_BF16, 0),
    "kw_3": (lambda g: g.conv(2, 64, 64, 64, 64, 3, 1, 1), L.TPG_BF16, 0),
    "stride_2": (lambda g: g.conv(2, 64, 128, 128, 64, 5, 2, 2), L.TPG_BF16, 0),
    "transposed": (lambda g: g.conv(2, 80, 64, 64, 80, 5, 1, 2, True), L.TPG_BF16, 0),
    "composite_5x5_valid": (lambda g: g.conv(2, 64, 5, 5, 64, 5, 1, 0), L.TPG_BF16, 0),
    "fp32": (lambda g: g.conv(2, 80, 8, 64, 80, 5, 1, 2), L.TPG_F32, 0),
    "width_96": (lambda g: g.conv(2, 80, 8, 96, 80, 5, 1, 2), L.TPG_BF16, 0),
    "width_40": (lambda g: g.conv(2, 80, 8, 40, 80, 5, 1, 2), L.TPG_BF16, 0),
    "unaligned_rows": (lambda g: g.conv(2, 206, 8, 64, 206, 5, 1, 2), L.TPG_BF16, 1),
    "row_stride_view": (lambda g: g.conv(2, 206, 8, 64, 206, 5, 1, 2), L.TPG_BF16, 2),
    "extent_2_31": (lambda g: g.conv(2, 206, 8, 64, 206, 5, 1, 2), L.TPG_BF16, 3),
}


@pytest.mark.parametrize("case", sorted(REFUSED))
def test_dense5_plan_refusals(lib, gen, case):
    mk, dtype, layout = REFUSED[case]
    shape = mk(gen)
    d = L.ConvDesc()
    for k, v in zip(gen.SHAPE_FIELDS, shape):
        setattr(d, k, v)
    d.dtype, d.algo, d.ksplit, d.slope, d.res_scale = dtype, DENSE5_ALGO, 2, 0.2, 1.0
    x = gen._act(L, d.in_c, d.in_h, d.in_w, dtype, layout)
    g = gen._act(L, d.out_c, d.out_h, d.out_w, dtype, layout)
    a, b = (d.in_c, d.out_c) if d.transposed else (d.out_c, d.in_c)
    dw = L.TpgTensor()
    dw.data, dw.dtype = gen.FAKE, L.TPG_F32
    dw.stride[0], dw.stride[1], dw.stride[2], dw.stride[3] = b * d.kh * d.kw, 1, d.kw * b, b
    plan = L.WgradPlan(kernel=-7, cfg=-8, splits=-9)
    lib.tpg_conv2d_wgrad_plan(ctypes.byref(L.ConvDesc()), x, g, dw, ctypes.byref(plan))  # (leaves another message)
    assert lib.tpg_conv2d_wgrad_plan(ctypes.byref(d), x, g, dw, ctypes.byref(plan)) == -30
    assert (plan.kernel, plan.cfg, plan.splits) == (-7, -8, -9)
    assert b"row-halo kernel does not apply" in lib.tpg_last_error()
    # (the same tensors are plannable without the forced tile, so the refusal is the tile's)
    d.algo, d.ksplit = 0, 0
    assert lib.tpg_conv2d_wgrad_plan(ctypes.byref(d), x, g, dw, ctypes.byref(plan)) == 0


def test_dense7_refusals_and_untuned_plans_unmoved(lib, gen):
    """The 7-wide dense tile (algo 13) still refuses 5-wide kernels, and algo == 0 on the four
    layers returns what the parent returned where the recorded rows hold the shape."""
    assert _plan(gen, lib, gen.conv(2, 80, 64, 64, 80, 5, 1, 2), L.TPG_BF16, algo=13) == -30
    fx = json.load(open(os.path.join(REPO, "tests", "golden", "wgrad_plans.json")))
    want = [gen.conv(32, 206, 128, 128, 206, 5, 1, 2), gen.conv(2, 206, 5, 64, 206, 5, 1, 2),
            gen.conv(1, 130, 3, 192, 20, 5, 1, 2), gen.conv(32, 64, 128, 128, 64, 5, 2, 2)]
    idx = {fx["shapes"].index(list(s)) for s in want}
    rows = [r for r in fx["rows"] if r[0] in idx and r[5] == 0 and r[6] == 0]
    assert len({r[0] for r in rows}) == len(want)
    for r in rows:
        assert gen.query(L, lib, fx["shapes"][r[0]], *r[1:7]) == r[7:], r
