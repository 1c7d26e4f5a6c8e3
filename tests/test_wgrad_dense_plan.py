"""CPU: the plan of the dense tap-per-wave weight-gradient tile (desc.algo 13, tile index 7 of
tp-gan_amd/csrc/tpg_wgrad_rh.hip) through tpg_conv2d_wgrad_plan: where it applies, the pixel
split it is given, every refusal (-30, message set, caller's struct untouched), deterministic
mode, and the untuned plans it must not have moved."""
import ctypes
import importlib.util
import json
import os

import pytest

import tpgan_lib as L

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DENSE_ALGO, DENSE_TILE = 13, 7
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


def _plan(gen, lib, shape, dtype, layout=0, det=0, algo=DENSE_ALGO, ks=1):
    got = gen.query(L, lib, shape, dtype, layout, 0, det, algo, ks)
    return got[0] if len(got) == 1 else dict(zip(gen.PLAN_FIELDS, got))


@pytest.mark.parametrize("dtype", [L.TPG_BF16, L.TPG_F16], ids=["bf16", "f16"])
def test_dense_plan_on_add_128(lib, gen, dtype):
    shape = gen.conv(32, 75, 128, 128, 75, 7, 1, 3)  # add_128 at bs32
    nkt = 32 * 128 * (128 // 64)                     # 64-pixel row segments
    for ks, splits in ((1, 1), (4, 4), (36, 36), (nkt, nkt), (nkt + 1, nkt), (1 << 20, nkt)):
        p = _plan(gen, lib, shape, dtype, ks=ks)
        assert p["kernel"] == ROW_HALO and p["cfg"] == DENSE_TILE, (ks, p)
        assert (p["tile_m"], p["tile_n"]) == (80, 80) and p["taps_per_block"] == 7, (ks, p)
        assert p["tiles"] == 7, (ks, p)                                    # one block per kernel row
        assert p["splits"] == splits and p["per_split"] == -(-nkt // splits), (ks, p)
        assert p["flags"] & 1 and not p["flags"] & 16, (ks, p)             # sums the bias; no dead-block skip
        assert 1 <= p["bias_share"] <= 7 and p["bias_share"] * p["splits"] <= max(16, p["splits"]), (ks, p)
    # the split rounds to whole k-tile groups: 10 k-tiles asked for 3 splits are 4 / 4 / 2
    p = _plan(gen, lib, gen.conv(2, 75, 5, 64, 75, 7, 1, 3), dtype, ks=3)
    assert (p["splits"], p["per_split"], p["tiles"]) == (3, 4, 7), p
    # a non-square 7-wide kernel: still one block per kernel row
    s = list(gen.conv(2, 80, 8, 64, 65, 7, 1, 3))
    s[gen.SHAPE_FIELDS.index("kh")] = 3
    s[gen.SHAPE_FIELDS.index("pad_t")] = s[gen.SHAPE_FIELDS.index("pad_b")] = 1
    p = _plan(gen, lib, tuple(s), dtype, ks=2)
    assert p["cfg"] == DENSE_TILE and p["tiles"] == 3 and p["splits"] == 2, p


def test_dense_plan_deterministic(lib, gen):
    shape = gen.conv(32, 75, 128, 128, 75, 7, 1, 3)
    for ks in (0, 1, 36, 1 << 20):
        p = _plan(gen, lib, shape, L.TPG_BF16, det=1, ks=ks)
        assert p["cfg"] == DENSE_TILE and p["splits"] == 1 and p["bias_share"] == 1 and p["tiles"] == 7, (ks, p)
        assert p["per_split"] == 32 * 128 * 2, (ks, p)


REFUSED = {
    "stride_2": (lambda g: g.conv(2, 75, 128, 128, 75, 7, 2, 3), L.TPG_BF16, 0),
    "transposed": (lambda g: g.conv(2, 75, 64, 64, 75, 7, 1, 3, True), L.TPG_BF16, 0),
    "composite_7x7_valid": (lambda g: g.conv(2, 64, 7, 7, 64, 7, 1, 0), L.TPG_BF16, 0),
    "kw_5": (lambda g: g.conv(2, 80, 64, 64, 80, 5, 1, 2), L.TPG_BF16, 0),
    "kw_3": (lambda g: g.conv(2, 64, 64, 64, 64, 3, 1, 1), L.TPG_BF16, 0),
    "in_c_81": (lambda g: g.conv(2, 81, 8, 64, 75, 7, 1, 3), L.TPG_BF16, 0),
    "out_c_81": (lambda g: g.conv(2, 75, 8, 64, 81, 7, 1, 3), L.TPG_BF16, 0),
    "width_96": (lambda g: g.conv(2, 75, 8, 96, 75, 7, 1, 3), L.TPG_BF16, 0),
    "width_40": (lambda g: g.conv(2, 75, 8, 40, 75, 7, 1, 3), L.TPG_BF16, 0),
    "fp32": (lambda g: g.conv(2, 75, 8, 64, 75, 7, 1, 3), L.TPG_F32, 0),
    "unaligned_rows": (lambda g: g.conv(2, 75, 8, 64, 75, 7, 1, 3), L.TPG_BF16, 1),
    "row_stride_view": (lambda g: g.conv(2, 75, 8, 64, 75, 7, 1, 3), L.TPG_BF16, 2),
    "extent_2_31": (lambda g: g.conv(2, 75, 8, 64, 75, 7, 1, 3), L.TPG_BF16, 3),
}


@pytest.mark.parametrize("case", sorted(REFUSED))
def test_dense_plan_refusals(lib, gen, case):
    mk, dtype, layout = REFUSED[case]
    shape = mk(gen)
    d = L.ConvDesc()
    for k, v in zip(gen.SHAPE_FIELDS, shape):
        setattr(d, k, v)
    d.dtype, d.algo, d.ksplit, d.slope, d.res_scale = dtype, DENSE_ALGO, 2, 0.2, 1.0
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


def test_untuned_plans_unmoved(lib, gen):
    """algo == 0 on a handful of shapes, the tile's own among them: what the parent returned, read
    from the recorded rows."""
    fx = json.load(open(os.path.join(REPO, "tests", "golden", "wgrad_plans.json")))
    want = [gen.conv(32, 75, 128, 128, 75, 7, 1, 3), gen.conv(32, 206, 128, 128, 206, 5, 1, 2),
            gen.conv(32, 3, 128, 128, 64, 7, 1, 3), gen.conv(1, 75, 4, 128, 75, 7, 1, 3),
            gen.conv(1, 64, 5, 64, 48, 7, 1, 3, reflect=True), gen.conv(32, 64, 128, 128, 64, 5, 2, 2)]
    idx = {fx["shapes"].index(list(s)) for s in want}
    rows = [r for r in fx["rows"] if r[0] in idx and r[5] == 0 and r[6] == 0]
    assert len({r[0] for r in rows}) == len(want) and len(rows) >= 4 * len(want)
    for r in rows:
        assert gen.query(L, lib, fx["shapes"][r[0]], *r[1:7]) == r[7:], r
