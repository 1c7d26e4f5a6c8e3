"""Record of the weight-gradient planner's picks: tests/golden/wgrad_plans.json.

    python tests/golden/make_wgrad_plans.py [walk.txt]

Every case is run through tpg_conv2d_wgrad_plan (host arithmetic only: no GPU, the tensors are
a never-dereferenced pointer plus real strides) and written as one row.  The file pins the
kernel, tile and pixel split of every shape below; regenerate it only with a change that MEANS
to move a plan, and read the diff.  tests/test_wgrad_plans.py replays the rows.

Layout of the file:
  shapes  [n, in_c, in_h, in_w, out_c, out_h, out_w, kh, kw, stride_h, stride_w, pad_t, pad_b,
           pad_l, pad_r, pad_mode, transposed]
  rows    [shape index, dtype, layout, flags, deterministic, algo, ksplit, then either the
           status (< 0) or the ten tpg_wgrad_plan fields in header order]
  layouts of x and g (channels-last, logical NCHW strides):
    0  dense, channels padded to 8 (what the product allocates)
    1  dense, channels as they are (odd counts fail the 16-byte row test: generic kernel)
    2  a view two pixels narrower than its buffer (row stride > W * pixel stride)
    3  layout 0 with a batch stride of 2^30 elements (byte extent past 2^31)

walk.txt (optional; kept when absent): the valid descriptors of tools/planner_asan.cpp's seeded
random walk, one per line as the 17 shape fields, dtype, ksplit, algo, flags.
"""
import ctypes
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "wgrad_plans.json")
SHAPE_FIELDS = ("n", "in_c", "in_h", "in_w", "out_c", "out_h", "out_w", "kh", "kw", "stride_h", "stride_w",
                "pad_t", "pad_b", "pad_l", "pad_r", "pad_mode", "transposed")
PLAN_FIELDS = ("kernel", "cfg", "tile_m", "tile_n", "splits", "per_split", "tiles", "taps_per_block", "bias_share",
               "flags")
F32, BF16, F16 = 0, 1, 2
CONCURRENT = 2
FAKE = 0x10000  # 16-byte aligned, never dereferenced


def _act(L, c, h, w, dtype, layout):
    cp = c if layout == 1 else (c + 7) // 8 * 8
    row = (w + (2 if layout == 2 else 0)) * cp
    t = L.TpgTensor()
    t.data, t.dtype = FAKE, dtype
    t.stride[0], t.stride[1], t.stride[2], t.stride[3] = h * row, 1, row, cp
    if layout == 3:
        t.stride[0] = max(t.stride[0], 1 << 30)
    return t


def query(L, lib, shape, dtype, layout, flags, det, algo, ksplit):
    """One call of tpg_conv2d_wgrad_plan: [status] when it fails, else the plan fields."""
    d = L.ConvDesc()
    for k, v in zip(SHAPE_FIELDS, shape):
        setattr(d, k, v)
    d.dtype, d.flags, d.algo, d.ksplit = dtype, flags, algo, ksplit
    d.slope, d.res_scale = 0.2, 1.0
    x = _act(L, d.in_c, d.in_h, d.in_w, dtype, layout)
    g = _act(L, d.out_c, d.out_h, d.out_w, dtype, layout)
    a, b = (d.in_c, d.out_c) if d.transposed else (d.out_c, d.in_c)
    dw = L.TpgTensor()  # fp32 [a][b][kh][kw], channels-last
    dw.data, dw.dtype = FAKE, F32
    dw.stride[0], dw.stride[1], dw.stride[2], dw.stride[3] = b * d.kh * d.kw, 1, d.kw * b, b
    plan = L.WgradPlan()
    lib.tpg_set_deterministic(det)
    try:
        rc = lib.tpg_conv2d_wgrad_plan(ctypes.byref(d), x, g, dw, ctypes.byref(plan))
    finally:
        lib.tpg_set_deterministic(0)
    return [rc] if rc else [getattr(plan, f) for f in PLAN_FIELDS]


def conv(n, ci, h, w, co, k, s, p, tr=False, op=0, reflect=False, pads=None):
    pt, pb, pl, pr = pads or (p, p, p, p)
    if tr:
        oh, ow = (h - 1) * s - 2 * p + k + op, (w - 1) * s - 2 * p + k + op
    else:
        oh, ow = (h + pt + pb - k) // s + 1, (w + pl + pr - k) // s + 1
    return (n, ci, h, w, co, oh, ow, k, k, s, s, pt, pb, pl, pr, 1 if reflect else 0, 1 if tr else 0)


# tests/test_capi.py SHAPES (G, D and the local pathways at bs32), then the layer list of
# tools/planner_asan.cpp
LAYERS = [
    conv(32, 206, 128, 128, 206, 5, 1, 2), conv(32, 75, 128, 128, 75, 7, 1, 3), conv(32, 3, 128, 128, 64, 7, 1, 3),
    conv(32, 64, 128, 128, 64, 5, 2, 2), conv(32, 576, 8, 8, 576, 2, 1, 0, reflect=True, pads=(1, 0, 1, 0)),
    conv(32, 576, 8, 8, 512, 3, 2, 1, True, 1), conv(32, 64, 8, 8, 32, 3, 4, 0, True, 1),
    conv(32, 320, 1, 1, 64, 8, 1, 0, True), conv(32, 512, 8, 8, 512, 8, 1, 0), conv(32, 512, 4, 4, 1, 3, 1, 1),
    conv(32, 3, 40, 40, 64, 3, 1, 1),
    conv(32, 64, 64, 64, 128, 3, 2, 1), conv(32, 128, 32, 32, 256, 3, 2, 1), conv(32, 256, 16, 16, 512, 3, 2, 1),
    conv(32, 512, 8, 8, 512, 3, 1, 1), conv(32, 64, 128, 128, 64, 3, 1, 1, reflect=True),
    conv(32, 64, 1, 1, 64, 8, 1, 0, True), conv(32, 512, 8, 8, 256, 3, 2, 1, True, 1),
    conv(32, 256, 16, 16, 128, 3, 2, 1, True, 1), conv(32, 128, 32, 32, 64, 3, 2, 1, True, 1),
    conv(32, 96, 128, 128, 64, 5, 1, 2), conv(32, 64, 128, 128, 3, 3, 1, 1), conv(32, 3, 40, 48, 64, 3, 1, 1),
    conv(32, 64, 20, 24, 128, 3, 2, 1), conv(32, 128, 10, 12, 64, 3, 2, 1, True, 1),
    conv(32, 256, 16, 16, 1, 16, 1, 0),
]
# tests/test_gpu_ops.py: WG_GEOMS, RH_GEOMS, IH_GEOMS with the picks each test makes
WG_GEOMS = [conv(2, 75, 12, 10, 75, 7, 1, 3), conv(2, 206, 9, 9, 206, 5, 1, 2), conv(4, 64, 5, 5, 64, 3, 1, 1),
            conv(2, 64, 9, 9, 128, 3, 2, 1), conv(2, 32, 5, 5, 24, 3, 2, 1, True, 1)]
RH_GEOMS = [conv(2, 206, 5, 64, 206, 5, 1, 2), conv(1, 75, 4, 128, 75, 7, 1, 3), conv(2, 64, 6, 64, 32, 3, 1, 1),
            conv(2, 40, 5, 64, 72, 3, 1, 1, reflect=True), conv(1, 3, 7, 64, 64, 7, 1, 3),
            conv(1, 130, 3, 192, 20, 5, 1, 2), conv(1, 64, 5, 64, 48, 7, 1, 3, reflect=True)]
IH_GEOMS = [conv(2, 40, 8, 8, 72, 3, 1, 1), conv(3, 64, 16, 16, 48, 3, 1, 1, reflect=True),
            conv(2, 96, 4, 32, 40, 3, 1, 1), conv(1, 32, 2, 64, 33, 3, 1, 1),
            conv(4, 48, 8, 8, 56, 2, 1, 0, reflect=True, pads=(1, 0, 1, 0)), conv(2, 130, 8, 8, 200, 3, 1, 1),
            conv(2, 64, 40, 40, 64, 3, 1, 1), conv(3, 128, 20, 20, 72, 3, 1, 1, reflect=True),
            conv(4, 96, 10, 10, 256, 3, 1, 1), conv(5, 32, 5, 5, 40, 3, 1, 1), conv(2, 64, 32, 48, 64, 3, 1, 1),
            conv(2, 40, 8, 12, 24, 3, 1, 1)]
WG_PICKS = [(a, k) for a in range(1, 6) for k in (1, 3, 8)] + [(0, 0)]
RH_PICKS = [(6, 1), (6, 3), (7, 7), (8, 2), (9, 5), (0, 0)]
IH_PICKS = [(10, 1), (10, 3), (11, 1), (11, 2), (0, 0)]
WALK = 300  # descriptors of the random walk kept


def cases(walk):
    """(shape, dtype, layout, flags, det, algo, ksplit) of every row, in file order."""
    out = []
    for s in LAYERS:  # the untuned plan in every mode
        out += [(s, dt, lay, fl, det, 0, 0) for dt in (F32, BF16, F16) for lay in range(4)
                for fl in (0, CONCURRENT) for det in (0, 1)]
    for s in LAYERS:  # every tuner pick, covered or not (fp32: the halo algos all answer -30)
        out += [(s, BF16, 0, 0, 0, a, k) for a in range(1, 13) for k in (1, 3, 36, 64)]
        out += [(s, F32, 0, 0, 0, a, k) for a in range(1, 6) for k in (1, 3, 36, 64)]
        out += [(s, F32, 0, 0, 0, a, 1) for a in range(6, 13)]
    for geoms, dts, picks in ((WG_GEOMS, (F32, BF16, F16), WG_PICKS), (RH_GEOMS, (BF16, F16), RH_PICKS),
                              (IH_GEOMS, (BF16, F16), IH_PICKS)):
        out += [(s, dt, 0, 0, 0, a, k) for s in geoms for dt in dts for a, k in picks]
    for w in walk[:WALK]:  # the walk's own dtype / ksplit / algo / flags
        out += [(tuple(w[:17]), w[17], lay, w[20], 0, w[19], w[18]) for lay in (0, 1)]
    return out


def main():
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(HERE)), "tp-gan_amd"))
    import tpgan_lib as L
    lib = ctypes.CDLL(L.LIB_PATH)
    for name in ("tpg_conv2d_wgrad_plan", "tpg_set_deterministic"):
        getattr(lib, name).restype, getattr(lib, name).argtypes = L.EXPORTS[name]
    if len(sys.argv) > 1:
        walk = [[int(v) for v in ln.split()[-21:]] for ln in open(sys.argv[1]) if ln.strip()]
    else:
        old = json.load(open(OUT))
        walk = [old["shapes"][r[0]] + [r[1], r[6], r[5], r[3]] for r in old["rows"][-2 * WALK::2]]
    shapes, rows = [], []
    for (s, dt, lay, fl, det, a, k) in cases(walk):
        if list(s) not in shapes:
            shapes.append(list(s))
        rows.append([shapes.index(list(s)), dt, lay, fl, det, a, k] + query(L, lib, s, dt, lay, fl, det, a, k))
    with open(OUT, "w") as f:
        f.write('{"shape_fields": %s,\n "plan_fields": %s,\n "shapes": [\n' % (json.dumps(SHAPE_FIELDS),
                                                                              json.dumps(PLAN_FIELDS)))
        f.write(",\n".join("  " + json.dumps(s, separators=(",", ":")) for s in shapes))
        f.write('\n ],\n "rows": [\n')
        f.write(",\n".join("  " + json.dumps(r, separators=(",", ":")) for r in rows))
        f.write("\n ]\n}\n")
    kinds = {}
    for r in rows:
        key = r[7] if len(r) == 8 else L.WGRAD_KERNELS[r[7]]
        kinds[key] = kinds.get(key, 0) + 1
    print(len(rows), "rows,", os.path.getsize(OUT), "bytes:", kinds)


if __name__ == "__main__":
    main()
