"""Record of the forward / input-gradient planner's picks: tests/golden/data_plans.json.

    python tests/golden/make_data_plans.py

Every case is run through tpg_conv2d_data_plan (host arithmetic only: no GPU, the tensors are a
never-dereferenced pointer plus real strides) and written as one row.  The file pins, for every
shape below, the form, the kernel each problem finally runs on, its tile, k split, weight region
and split-K bytes, and the status of the calls that are refused; regenerate it only with a change
that MEANS to move a plan, and read the diff.  tests/test_capi.py replays the rows.

Layout of the file:
  shapes  as tests/golden/wgrad_plans.json
  rows    [shape index, op, dtype, layout, flags, deterministic, data_ksplit, data_algo, in_act,
           short workspace, then the status (< 0) or an index into plans]
  plans   the distinct answers: the five plan_fields, then the prob_fields of every problem
  op      0 forward, 1 input gradient, 3 masked input gradient (tpg_conv2d_bwd's first attempt)
  layouts of the activations: make_wgrad_plans.py's four; the workspace offered is
          tpg_conv2d_workspace(d, op), or 256 bytes in the short-workspace rows
The shapes: make_wgrad_plans.LAYERS, the forward / input-gradient geometries of
tests/test_gpu_ops.py and tests/test_gpu_pack.py, the shapes of the plan-branch tests, and the
random walk of tools/planner_asan.cpp as wgrad_plans.json recorded it.
"""
import ctypes
import importlib.util
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "data_plans.json")
_spec = importlib.util.spec_from_file_location("make_wgrad_plans", os.path.join(HERE, "make_wgrad_plans.py"))
W = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(W)
SHAPE_FIELDS, conv, F32, BF16, F16, CONCURRENT = W.SHAPE_FIELDS, W.conv, W.F32, W.BF16, W.F16, W.CONCURRENT
PLAN_FIELDS = ("flags", "ws_bytes", "packed_bytes", "tmp_bytes", "sk_off")
PROB_FIELDS = ("kernel", "cfg", "th", "tw", "img", "bn", "rows", "halo_px", "taps", "ksteps", "ksplit", "kps", "paired",
               "pw_tile", "wp_off", "wp_bytes", "sk_bytes")
FWD, BWD, MASKED = 0, 1, 3
WPACKED, DX_ACCUM = 1, 4
LEAKY = 2


def tensors(L, shape, op, dtype, layout):
    """(a, y, m, g, x) of tpg_conv2d_data_plan for a shape in one layout."""
    d = dict(zip(SHAPE_FIELDS, shape))
    x = W._act(L, d["in_c"], d["in_h"], d["in_w"], dtype, layout)
    y = W._act(L, d["out_c"], d["out_h"], d["out_w"], dtype, layout)
    return (x, y, y, y, x) if op == FWD else (y, x, y, y, x)


def query(L, lib, shape, op, dtype, layout, flags, det, ks, algo, in_act, short):
    """One call of tpg_conv2d_data_plan: [status] when it fails, else the plan and problem fields."""
    d = L.ConvDesc()
    for k, v in zip(SHAPE_FIELDS, shape):
        setattr(d, k, v)
    d.dtype, d.flags, d.data_ksplit, d.data_algo, d.in_act = dtype, flags, ks, algo, in_act
    d.act, d.slope, d.in_slope, d.res_scale = LEAKY, 0.2, 0.2, 1.0
    ws = 256 if short else lib.tpg_conv2d_workspace(ctypes.byref(d), FWD if op == FWD else BWD)
    plan = L.DataPlan()
    lib.tpg_set_deterministic(det)
    try:
        rc = lib.tpg_conv2d_data_plan(ctypes.byref(d), op, *tensors(L, shape, op, dtype, layout), ws, ctypes.byref(plan))
    finally:
        lib.tpg_set_deterministic(0)
    if rc:
        return [rc]
    return [getattr(plan, f) for f in PLAN_FIELDS] + [getattr(plan.prob[i], f) for i in range(plan.nprobs)
                                                      for f in PROB_FIELDS]


def _t(n, ci, h, w, co, k, s, p, tr=False, op=0, refl=False):  # a tests/test_gpu_ops.py geometry
    return conv(n, ci, h, w, co, k, s, p, tr, op, reflect=refl, pads=(1, 0, 1, 0) if refl else None)


# tests/test_gpu_ops.py: GEOMS, GEOMS512, SPLITK_GEOMS, test_forced_data_split
OPS_GEOMS = [
    _t(2, 206, 12, 10, 206, 5, 1, 2), _t(2, 75, 9, 9, 75, 7, 1, 3), _t(2, 576, 8, 8, 576, 2, 1, 0, refl=True),
    _t(3, 512, 4, 4, 512, 3, 1, 1), _t(2, 64, 17, 15, 128, 3, 2, 1), _t(2, 416, 6, 5, 128, 3, 2, 1, True, 1),
    _t(2, 576, 4, 4, 512, 3, 2, 1, True, 1), _t(2, 64, 3, 3, 32, 3, 4, 0, True, 1), _t(2, 320, 1, 1, 64, 8, 1, 0, True),
    _t(2, 512, 8, 8, 40, 8, 1, 0), _t(2, 32, 20, 18, 3, 3, 1, 1), _t(1, 3, 33, 31, 64, 7, 1, 3),
    _t(2, 64, 9, 9, 64, 5, 2, 2), _t(1, 206, 40, 36, 206, 5, 1, 2), _t(1, 75, 33, 34, 75, 7, 1, 3),
    _t(1, 64, 64, 64, 32, 3, 1, 1), _t(1, 64, 48, 48, 128, 3, 1, 1), _t(1, 64, 32, 32, 416, 3, 1, 1),
    _t(1, 208, 32, 32, 64, 3, 2, 1, True, 1), _t(1, 64, 64, 64, 64, 3, 2, 1), _t(1, 24, 40, 40, 24, 2, 1, 0, refl=True),
    _t(1, 8, 40, 40, 3, 3, 1, 1), _t(8, 512, 8, 8, 512, 3, 1, 1), _t(12, 256, 5, 5, 256, 3, 1, 1),
    _t(6, 128, 10, 10, 128, 3, 1, 1), _t(4, 64, 20, 20, 64, 3, 1, 1), _t(3, 256, 8, 12, 256, 3, 1, 1),
    _t(5, 256, 16, 16, 512, 3, 2, 1), _t(4, 512, 5, 5, 256, 3, 2, 1, True, 1), _t(4, 576, 8, 8, 576, 2, 1, 0, refl=True),
    _t(3, 200, 10, 10, 197, 3, 1, 1), _t(1, 208, 24, 32, 208, 3, 1, 1), _t(4, 96, 16, 16, 384, 3, 1, 1),
    _t(2, 64, 8, 8, 160, 3, 1, 1), _t(1, 80, 32, 40, 80, 5, 1, 2), _t(3, 40, 10, 10, 72, 3, 1, 1),
    _t(3, 64, 10, 12, 3, 1, 1, 0), _t(2, 20, 9, 11, 2, 3, 1, 1), _t(2, 32, 66, 70, 3, 3, 1, 1),
    _t(3, 64, 9, 7, 128, 1, 1, 0), _t(2, 256, 8, 8, 1024, 1, 1, 0), _t(2, 2048, 4, 4, 512, 1, 1, 0),
    _t(3, 256, 10, 9, 512, 1, 2, 0), _t(2, 128, 16, 16, 64, 1, 1, 0),
    _t(16, 75, 128, 128, 75, 7, 1, 3), _t(16, 64, 128, 128, 64, 3, 1, 1), _t(16, 128, 128, 128, 64, 5, 1, 2),
    _t(22, 24, 128, 96, 40, 3, 1, 1),
    _t(32, 512, 8, 8, 512, 3, 1, 1), _t(32, 256, 5, 5, 256, 3, 1, 1), _t(32, 64, 10, 10, 72, 3, 1, 1),
    _t(32, 256, 8, 8, 256, 3, 1, 1), _t(16, 128, 16, 16, 64, 3, 2, 1), _t(8, 64, 20, 20, 72, 5, 1, 2),
]
# tests/test_gpu_pack.py: GEOMS and the rest of XGEOMS
PACK_GEOMS = [_t(2, 75, 24, 40, 75, 7, 1, 3), _t(2, 206, 16, 24, 206, 5, 1, 2), _t(1, 206, 20, 36, 64, 5, 1, 2),
              _t(2, 208, 16, 16, 208, 3, 1, 1), _t(2, 80, 20, 24, 80, 5, 1, 2), _t(2, 40, 12, 12, 48, 3, 1, 1),
              _t(2, 16, 8, 8, 8, 3, 1, 1), _t(4, 64, 10, 10, 64, 3, 1, 1), _t(2, 128, 20, 20, 128, 3, 1, 1),
              _t(8, 256, 8, 8, 256, 3, 1, 1), _t(4, 512, 8, 8, 512, 3, 1, 1), _t(4, 128, 16, 16, 64, 3, 2, 1),
              _t(4, 64, 5, 5, 32, 3, 2, 1, True, 1), _t(4, 96, 8, 8, 96, 2, 1, 0, refl=True)]
# the plan-branch tests of tests/test_gpu_ops.py: unaligned rows (generic kernel; -21 when
# pre-packed), a 1x1 conv whose batch stride the pointwise kernel refuses (layout 3)
BRANCH_GEOMS = [_t(2, 3, 6, 6, 8, 3, 1, 1), _t(2, 32, 8, 8, 64, 1, 1, 0)]
PICKS = [(ks, algo) for ks in (0, 1, 3, 8) for algo in (0, 1, 2)]
WALK = 300  # descriptors of the random walk kept


def cases(walk):
    """(shape, op, dtype, layout, flags, det, data_ksplit, data_algo, in_act, short) of every row."""
    out = []
    ops = (FWD, BWD, MASKED)
    for s in W.LAYERS:  # the untuned plan over dtypes, layouts, CONCURRENT and deterministic mode
        out += [(s, FWD, dt, lay, fl, det, 0, 0, 0, 0) for dt, lay, fl, det in (
            (BF16, 0, 0, 0), (BF16, 0, CONCURRENT, 0), (BF16, 0, 0, 1), (BF16, 1, 0, 0), (BF16, 2, CONCURRENT, 1),
            (BF16, 3, 0, 0), (F32, 0, 0, 0), (F32, 1, CONCURRENT, 0), (F32, 3, 0, 1), (F16, 0, CONCURRENT, 1),
            (F16, 2, 0, 0))]
        out += [(s, BWD, dt, lay, fl, det, 0, 0, 0, 0) for dt, lay, fl, det in (
            (BF16, 0, 0, 0), (BF16, 0, CONCURRENT, 1), (BF16, 1, 0, 0), (BF16, 3, 0, 0), (F32, 2, 0, 0), (F16, 0, 0, 1))]
        out += [(s, MASKED, dt, lay, fl, det, 0, 0, 0, 0) for dt, lay, fl, det in (
            (BF16, 0, 0, 0), (BF16, 0, CONCURRENT, 1), (BF16, 1, 0, 0), (BF16, 3, 0, 0), (F32, 0, 0, 0), (F16, 2, 0, 0))]
        # pre-packed weights, dx accumulation, in_act, a short workspace, every tuner pick
        out += [(s, op, BF16, lay, WPACKED | fl, 0, 0, 0, 0, 0) for op, lay, fl in (
            (FWD, 0, 0), (FWD, 1, 0), (FWD, 3, CONCURRENT), (BWD, 0, CONCURRENT), (BWD, 2, 0), (BWD, 3, 0))]
        out += [(s, MASKED, BF16, 0, WPACKED, 0, 0, 0, 0, 0), (s, BWD, F32, 0, DX_ACCUM, 0, 0, 0, 0, 0),
                (s, BWD, BF16, 0, DX_ACCUM, 0, 0, 0, 0, 0), (s, MASKED, BF16, 0, DX_ACCUM, 0, 0, 0, 0, 0)]
        out += [(s, op, BF16, lay, fl, 0, 0, 0, LEAKY, 0) for op, lay, fl in (
            (BWD, 0, 0), (BWD, 1, 0), (BWD, 0, DX_ACCUM), (MASKED, 0, 0))]
        out += [(s, op, BF16, 0, 0, 0, 0, 0, 0, 1) for op in (FWD, BWD)]
        out += [(s, (FWD, BWD)[k % 2], BF16, 0, 0, 0, ks, a, 0, 0) for k, (ks, a) in enumerate(PICKS[1:])]
    for i, s in enumerate(OPS_GEOMS + PACK_GEOMS + BRANCH_GEOMS):
        out += [(s, op, BF16, 0, 0, 0, 0, 0, 0, 0) for op in ops] + [(s, op, F32, 0, 0, 0, 0, 0, 0, 0) for op in (FWD, BWD)]
        out += [(s, (FWD, BWD)[(i + k) % 2], F16, lay, fl, det, 0, 0, ia, 0)
                for k, (lay, fl, det, ia) in enumerate(((1, 0, 0, 0), (3, WPACKED, 0, 0), (i % 4, CONCURRENT, 1, LEAKY)))]
        ks, a = PICKS[1 + i % 11]
        out += [(s, op, BF16, 0, (CONCURRENT, WPACKED, DX_ACCUM, 0)[i % 4], 0, ks, a, 0, 0) for op in (FWD, BWD)]
    for s in BRANCH_GEOMS:
        out += [(s, op, BF16, lay, fl, 0, 0, 0, 0, 0) for op in ops for lay in (1, 3) for fl in (0, WPACKED)]
    for i, w in enumerate(walk[:WALK]):  # the walk's own dtype and flags, the picks in turn
        ks, a = PICKS[i % 12]
        out += [(tuple(w[:17]), op, w[17], lay, w[20], (i // 3) % 2, ks, a, LEAKY if i % 5 == 0 else 0, 0)
                for op, lay in (((FWD, BWD)[i % 2], (i // 2) % 4), (MASKED, 0))[:2 if i % 8 == 0 else 1]]
    return out


def main():
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(HERE)), "tp-gan_amd"))
    import tpgan_lib as L
    lib = ctypes.CDLL(L.LIB_PATH)
    for name in ("tpg_conv2d_data_plan", "tpg_conv2d_workspace", "tpg_set_deterministic"):
        getattr(lib, name).restype, getattr(lib, name).argtypes = L.EXPORTS[name]
    old = json.load(open(os.path.join(HERE, "wgrad_plans.json")))
    walk = [old["shapes"][r[0]] + [r[1], r[6], r[5], r[3]] for r in old["rows"][-2 * W.WALK::2]]
    shapes, rows, plans, index = [], [], [], {}
    for c in cases(walk):
        if list(c[0]) not in shapes:
            shapes.append(list(c[0]))
        got = query(L, lib, *c)
        if len(got) > 1:  # a plan: kept once
            if tuple(got) not in index:
                index[tuple(got)] = len(plans)
                plans.append(got)
            got = [index[tuple(got)]]
        rows.append([shapes.index(list(c[0]))] + list(c[1:]) + got)
    dump = lambda v: ",\n".join("  " + json.dumps(r, separators=(",", ":")) for r in v)
    with open(OUT, "w") as f:
        f.write('{"shape_fields": %s,\n "plan_fields": %s,\n "prob_fields": %s,\n "shapes": [\n' % (
            json.dumps(SHAPE_FIELDS), json.dumps(PLAN_FIELDS), json.dumps(PROB_FIELDS)))
        f.write(dump(shapes) + '\n ],\n "rows": [\n' + dump(rows) + '\n ],\n "plans": [\n' + dump(plans) + "\n ]\n}\n")
    print(len(rows), "rows,", len(plans), "plans,", os.path.getsize(OUT), "bytes:", summary(L, rows, plans))


def summary(L, rows, plans):
    """Rows per status and per kernel kind (a row counts once for every kind among its problems)."""
    n, k0, np_ = {}, PROB_FIELDS.index("kernel"), len(PLAN_FIELDS)
    for r in rows:
        keys = [r[-1]] if r[-1] < 0 else sorted({L.DATA_KERNELS[v] for v in plans[r[-1]][np_ + k0::len(PROB_FIELDS)]})
        for key in keys:
            n[key] = n.get(key, 0) + 1
    return n


if __name__ == "__main__":
    main()
