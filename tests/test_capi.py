"""CPU: the C-ABI library (tp-gan_amd/libtpgan_hip.so) loads without a GPU, exports every
function include/tpgan.h declares, and its host-side planner (workspace sizing and
descriptor validation, no device work) behaves."""
import ctypes
import os
import re

import pytest

import tpgan_lib as L

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_functions():
    src = open(os.path.join(REPO, "include", "tpgan.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(tpg_[a-z0-9_]+)\s*\(", src)))


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(L.LIB_PATH):
        pytest.skip("libtpgan_hip.so not built")
    lib = ctypes.CDLL(L.LIB_PATH)
    for name, (res, args) in L.EXPORTS.items():
        f = getattr(lib, name)
        f.restype = res
        f.argtypes = args
    return lib


def test_header_matches_binding():
    assert header_functions() == sorted(L.EXPORTS), "tpgan_lib.EXPORTS must bind exactly the header's functions"


def test_exports(lib):
    """The library's defined `T tpg_*` dynamic symbols are exactly the header's functions: nothing
    missing, and no internal launcher exported with C linkage beside them."""
    import shutil
    import subprocess
    for name in header_functions():
        assert hasattr(lib, name), name
    assert lib.tpg_version().decode().startswith("tpgan_hip")
    nm = shutil.which("nm") or shutil.which("llvm-nm", path="/opt/rocm/lib/llvm/bin")  # (the Makefile's LLVM_BIN)
    if nm is None:
        pytest.skip("nm not installed")
    out = subprocess.run([nm, "-D", "--defined-only", L.LIB_PATH], check=True, capture_output=True, text=True).stdout
    exported = sorted(m.group(1) for m in re.finditer(r"^\S+ T (tpg_\w+)$", out, flags=re.M))
    assert exported == header_functions()


def _desc(n, cin, h, w, cout, k, s, p, transposed=False, op=0, reflect=False, dtype=L.TPG_BF16):
    d = L.ConvDesc()
    d.n, d.in_c, d.in_h, d.in_w, d.out_c = n, cin, h, w, cout
    if transposed:
        d.out_h = (h - 1) * s - 2 * p + k + op
        d.out_w = (w - 1) * s - 2 * p + k + op
    elif reflect:
        d.out_h, d.out_w = h, w
    else:
        d.out_h = (h + 2 * p - k) // s + 1
        d.out_w = (w + 2 * p - k) // s + 1
    d.kh = d.kw = k
    d.stride_h = d.stride_w = s
    if reflect:
        d.pad_t, d.pad_b, d.pad_l, d.pad_r = 1, 0, 1, 0
        d.pad_mode = L.PAD_REFLECT
    else:
        d.pad_t = d.pad_b = d.pad_l = d.pad_r = p
    d.transposed = 1 if transposed else 0
    d.dtype = dtype
    d.act = L.ACT_LEAKY
    d.slope = 0.01
    d.res_scale = 1.0
    return d


# every conv shape class of G + D at bs32
SHAPES = [
    (32, 206, 128, 128, 206, 5, 1, 2, False, 0, False),
    (32, 75, 128, 128, 75, 7, 1, 3, False, 0, False),
    (32, 3, 128, 128, 64, 7, 1, 3, False, 0, False),
    (32, 64, 128, 128, 64, 5, 2, 2, False, 0, False),
    (32, 576, 8, 8, 576, 2, 1, 0, False, 0, True),
    (32, 576, 8, 8, 512, 3, 2, 1, True, 1, False),
    (32, 64, 8, 8, 32, 3, 4, 0, True, 1, False),
    (32, 320, 1, 1, 64, 8, 1, 0, True, 0, False),
    (32, 512, 8, 8, 512, 8, 1, 0, False, 0, False),
    (32, 512, 4, 4, 1, 3, 1, 1, False, 0, False),
    (32, 3, 40, 40, 64, 3, 1, 1, False, 0, False),
]


@pytest.mark.parametrize("shape", SHAPES, ids=[str(i) for i in range(len(SHAPES))])
@pytest.mark.parametrize("dtype", [L.TPG_F32, L.TPG_BF16])
def test_workspace_sizes(lib, shape, dtype):
    n, cin, h, w, cout, k, s, p, tr, op, refl = shape
    d = _desc(n, cin, h, w, cout, k, s, p, tr, op, refl, dtype)
    for op_ in (L.OP_FWD, L.OP_BWD_DATA, L.OP_BWD_FILTER):
        ws = lib.tpg_conv2d_workspace(ctypes.byref(d), op_)
        assert ws > 0, (shape, op_, lib.tpg_last_error())
    # the packed weights alone need at least the weight tensor in the compute dtype
    esize = 2 if dtype == L.TPG_BF16 else 4
    assert lib.tpg_conv2d_workspace(ctypes.byref(d), L.OP_FWD) >= cin * cout * k * k * esize


def test_bad_descriptors(lib):
    d = _desc(2, 16, 8, 8, 16, 3, 1, 1)
    d.out_h = 9  # inconsistent with the geometry
    assert lib.tpg_conv2d_workspace(ctypes.byref(d), L.OP_FWD) == 0
    assert b"Conv2d output" in lib.tpg_last_error()
    d = _desc(2, 16, 8, 8, 16, 3, 1, 1)
    d.dtype = 7
    assert lib.tpg_conv2d_workspace(ctypes.byref(d), L.OP_FWD) == 0
    assert b"dtype" in lib.tpg_last_error()
    d = _desc(2, 16, 8, 8, 16, 9, 1, 4)  # 81 taps > 64
    assert lib.tpg_conv2d_workspace(ctypes.byref(d), L.OP_FWD) == 0
    d = _desc(2, 16, 4, 4, 16, 3, 2, 1, transposed=True, op=1)
    d.pad_mode = L.PAD_REFLECT
    assert lib.tpg_conv2d_workspace(ctypes.byref(d), L.OP_FWD) == 0
    assert b"reflect" in lib.tpg_last_error()
    # a kernel larger than the padded input: C's truncating division gives a "consistent"
    # 0- or 1-pixel output that torch rejects (the 0-pixel case divided by zero in the planner)
    for k, s in ((3, 2), (3, 3)):
        d = _desc(2, 16, 1, 1, 16, k, s, 0)
        assert lib.tpg_conv2d_workspace(ctypes.byref(d), L.OP_FWD) == 0
        assert b"larger than the padded input" in lib.tpg_last_error() or b"empty" in lib.tpg_last_error()


def test_null_tensor_rejected_without_device_work(lib):
    d = _desc(2, 16, 8, 8, 16, 3, 1, 1)
    z = L.TpgTensor()
    rc = lib.tpg_conv2d_fwd(ctypes.byref(d), z, z, None, z, z, None, 0, None)
    assert rc < 0 and b"NULL" in lib.tpg_last_error()
    # one entry point per kernel file (features, image, identity): the same status as ever, and
    # the message names the call -- they share the conv entry points' error plumbing
    for call, name in ((lambda: lib.tpg_avgpool_fwd(1, 16, 8, 8, z, z, None), b"avgpool"),
                       (lambda: lib.tpg_denorm_u8(1, 3, 8, 8, z, None, None), b"denorm_u8"),
                       (lambda: lib.tpg_l2_normalize(1, 4, z, None, 4, None, None, None), b"l2_normalize")):
        lib.tpg_conv2d_fwd(ctypes.byref(d), z, z, None, z, z, None, 0, None)  # (an unrelated earlier failure)
        assert call() == -10
        assert name in lib.tpg_last_error() and b"NULL" in lib.tpg_last_error()


def test_wgrad_plans_match_recorded(lib):
    """tpg_conv2d_wgrad_plan returns, for every row of tests/golden/wgrad_plans.json, exactly the
    recorded status or plan (kernel, tile, pixel split, tiles, taps per block, bias share, flags).
    The fixture is a record of the planner's picks -- TP-GAN's layer shapes, the GPU tests'
    weight-gradient geometries and a random walk, over dtypes, layouts, CONCURRENT,
    deterministic mode and every tuner pick -- first taken from the code before planning and
    launching were split.  It is regenerated (tests/golden/make_wgrad_plans.py) only by a
    change that means to move a plan."""
    import importlib.util
    import json
    spec = importlib.util.spec_from_file_location("make_wgrad_plans",
                                                  os.path.join(REPO, "tests", "golden", "make_wgrad_plans.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    fx = json.load(open(os.path.join(REPO, "tests", "golden", "wgrad_plans.json")))
    assert tuple(fx["shape_fields"]) == gen.SHAPE_FIELDS and tuple(fx["plan_fields"]) == gen.PLAN_FIELDS
    assert len(fx["rows"]) > 4000
    bad = []
    for r in fx["rows"]:
        got = gen.query(L, lib, fx["shapes"][r[0]], *r[1:7])
        if got != r[7:]:
            bad.append((fx["shapes"][r[0]], r[1:7], "recorded", r[7:], "got", got))
    assert not bad, "%d of %d plans moved, first: %s" % (len(bad), len(fx["rows"]), bad[:3])
    # a failing status leaves the caller's struct alone and sets the message
    d = _desc(32, 64, 128, 128, 64, 5, 2, 2)
    d.algo, d.ksplit = 6, 1
    x, g = gen._act(L, 64, 128, 128, L.TPG_BF16, 0), gen._act(L, 64, 64, 64, L.TPG_BF16, 0)
    dw = gen._act(L, 64, 5, 5, L.TPG_F32, 1)
    plan = L.WgradPlan(kernel=-7)
    assert lib.tpg_conv2d_wgrad_plan(ctypes.byref(d), x, g, dw, ctypes.byref(plan)) == -30
    assert plan.kernel == -7 and b"row-halo kernel does not apply" in lib.tpg_last_error()


def _data_gen():
    import importlib.util
    import json
    spec = importlib.util.spec_from_file_location("make_data_plans",
                                                  os.path.join(REPO, "tests", "golden", "make_data_plans.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    return gen, json.load(open(os.path.join(REPO, "tests", "golden", "data_plans.json")))


def test_data_plans_match_recorded(lib):
    """tpg_conv2d_data_plan returns, for every row of tests/golden/data_plans.json, exactly the
    recorded status or plan: form flags, workspace layout and per problem the kernel it finally
    runs on, config, tile, k split, weight region and split-K bytes.  The fixture was first taken
    from the code before planning and launching were split (its launch sites dumped these fields
    and returned), over TP-GAN's layer shapes, the GPU tests' geometries and a random walk,
    crossed with op, dtype, tensor layout, CONCURRENT, deterministic mode, pre-packed weights,
    dx accumulation, in_act and every forced k split / kernel.  It is regenerated
    (tests/golden/make_data_plans.py) only by a change that means to move a plan."""
    gen, fx = _data_gen()
    assert tuple(fx["shape_fields"]) == gen.SHAPE_FIELDS and tuple(fx["plan_fields"]) == gen.PLAN_FIELDS
    assert tuple(fx["prob_fields"]) == gen.PROB_FIELDS and len(fx["rows"]) > 2000
    bad, statuses, kinds, flags = [], set(), set(), 0
    k0, npf, nf = gen.PROB_FIELDS.index("kernel"), len(gen.PLAN_FIELDS), len(gen.PROB_FIELDS)
    for r in fx["rows"]:
        want = [r[-1]] if r[-1] < 0 else fx["plans"][r[-1]]
        got = gen.query(L, lib, fx["shapes"][r[0]], *r[1:-1])
        if got != want:
            bad.append((fx["shapes"][r[0]], r[1:-1], "recorded", want, "got", got))
        if r[-1] < 0:
            statuses.add(r[-1])
        else:
            flags |= want[0]
            kinds |= set(want[npf + k0::nf])
    assert not bad, "%d of %d plans moved, first: %s" % (len(bad), len(fx["rows"]), bad[:3])
    # the record covers every kernel kind, every form flag and every refusal
    assert kinds == {0, 1, 2} and flags == 31 and statuses >= {-4, -20, -21, -31, -32}, (kinds, flags, statuses)
    # a failing status leaves the caller's struct alone and sets the message
    s = gen._t(2, 3, 6, 6, 8, 3, 1, 1)
    d = _desc(2, 3, 6, 6, 8, 3, 1, 1)
    d.flags = L.FLAG_WPACKED
    plan = L.DataPlan(nprobs=-7)
    rc = lib.tpg_conv2d_data_plan(ctypes.byref(d), L.OP_FWD, *gen.tensors(L, s, L.OP_FWD, L.TPG_BF16, 1), 1 << 20,
                                  ctypes.byref(plan))
    assert rc == -21 and plan.nprobs == -7 and b"need the generic one" in lib.tpg_last_error()


def test_data_plan_branches(lib):
    """The run-time decisions the plan took over, on the shapes the GPU tests run them with
    (tests/test_gpu_ops.py test_unaligned_input_runs_generic_kernel, test_halo_512_rows_vs_torch):
    unaligned rows fall back to the generic kernel, or -21 with pre-packed weights; the 512-row
    tile has no masked mode (-31: tpg_conv2d_bwd takes the activation pass); a batch stride past
    the pointwise kernel's 2^31-byte extent gives the halo kernel the same plan, one past the halo
    kernel's 2^31 elements the generic kernel.  (The last two need a buffer of that extent to
    run, so they are held here alone.)"""
    gen, _ = _data_gen()

    def kinds(shape, op, layout, flags=0):
        got = gen.query(L, lib, shape, op, L.TPG_BF16, layout, flags, 0, 0, 0, 0, 0)
        return got[0] if len(got) == 1 else [L.DATA_KERNELS[k] for k in got[len(gen.PLAN_FIELDS)::len(gen.PROB_FIELDS)]]

    thin = gen._t(2, 3, 6, 6, 8, 3, 1, 1)
    assert kinds(thin, L.OP_FWD, 0) == ["halo"] and kinds(thin, L.OP_FWD, 1) == ["generic"]
    assert kinds(thin, L.OP_FWD, 1, L.FLAG_WPACKED) == -21
    big = gen._t(16, 64, 128, 128, 64, 3, 1, 1)
    got = gen.query(L, lib, big, L.OP_BWD_DATA, L.TPG_BF16, 0, 0, 0, 0, 0, 0, 0)
    assert got[len(gen.PLAN_FIELDS) + gen.PROB_FIELDS.index("rows")] == 512
    assert kinds(big, L.OP_BWD_DATA_MASKED, 0) == -31
    assert kinds(gen._t(4, 64, 20, 20, 64, 3, 1, 1), L.OP_BWD_DATA_MASKED, 0) == ["halo"]
    pw = gen._t(2, 32, 8, 8, 64, 1, 1, 0)
    assert kinds(pw, L.OP_FWD, 0) == ["pointwise"] and kinds(pw, L.OP_FWD, 3) == ["halo"]
    assert kinds(gen._t(3, 32, 8, 8, 64, 1, 1, 0), L.OP_FWD, 3) == ["generic"]


def test_data_plans_agree_with_sizing(lib):
    """What used to agree only because three entry points planned under the same scope: for every
    recorded plan tpg_conv2d_workspace is the plan's workspace, and where the same call takes
    pre-packed weights, tpg_conv2d_packed_bytes is the plan's packed bytes and
    tpg_conv2d_pack_jobs gives one job per problem with taps, its region at the plan's offset."""
    gen, fx = _data_gen()
    npf, nf = len(gen.PLAN_FIELDS), len(gen.PROB_FIELDS)
    jb = lib.tpg_pack_job_bytes()
    host = ctypes.create_string_buffer(jb * 64)
    w = L.TpgTensor()
    w.data, w.dtype = 0x10000, L.TPG_F32
    checked = 0
    for r in fx["rows"]:
        if r[-1] < 0:
            continue
        shape, (op, dtype, layout, flags, det, ks, algo, in_act, short) = fx["shapes"][r[0]], r[1:-1]
        d = L.ConvDesc()
        for k, v in zip(gen.SHAPE_FIELDS, shape):
            setattr(d, k, v)
        d.dtype, d.flags, d.data_ksplit, d.data_algo = dtype, flags, ks, algo
        lib.tpg_set_deterministic(det)
        try:
            pop = L.OP_FWD if op == L.OP_FWD else L.OP_BWD_DATA
            assert lib.tpg_conv2d_workspace(ctypes.byref(d), pop) == fx["plans"][r[-1]][1], r
            got = gen.query(L, lib, shape, op, dtype, layout, flags | L.FLAG_WPACKED, det, ks, algo, in_act, short)
            if len(got) == 1:
                assert got[0] == -21, (r, got)
                continue
            assert lib.tpg_conv2d_packed_bytes(ctypes.byref(d), pop) == got[2], r
            nj = lib.tpg_conv2d_pack_jobs(ctypes.byref(d), pop, w, 0x20000, host, 64)
            probs = [got[i:i + nf] for i in range(npf, len(got), nf)]
            offs = [p[gen.PROB_FIELDS.index("wp_off")] for p in probs if p[gen.PROB_FIELDS.index("taps")] > 0]
            # (PackJob begins with PackArgs: W, four strides, then Wp)
            regions = [int.from_bytes(host.raw[j * jb + 40:j * jb + 48], "little") - 0x20000 for j in range(nj)]
            assert regions == offs, (r, regions, offs)
            checked += 1
        finally:
            lib.tpg_set_deterministic(0)
    assert checked > 1000


def test_planner_sanitizer_sweep():
    """The planner (descriptor validation, plans, workspace and pre-pack sizing) rebuilt with
    host AddressSanitizer + UBSan and driven over TP-GAN's layer shapes, a seeded random walk of
    geometries and malformed descriptors (tools/planner_asan.cpp).  The sweep first found a
    divide-by-zero on a 0-pixel Conv2d output, now rejected by check_desc."""
    import shutil
    import subprocess
    src = os.path.join(REPO, "tp-gan_amd")
    objs = [os.path.join(src, "build", f) for f in os.listdir(os.path.join(src, "build"))
            if f.endswith(".o")] if os.path.isdir(os.path.join(src, "build")) else []
    if not shutil.which("/opt/rocm/bin/hipcc") or len(objs) < 8:
        pytest.skip("needs hipcc and the built kernel objects (make -C tp-gan_amd)")
    r = subprocess.run(["make", "-s", "-C", src, "asan"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([os.path.join(src, "build", "asan", "planner_asan"), "20000"], capture_output=True,
                       text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "ok" in r.stdout and "ERROR" not in r.stderr, r.stdout + r.stderr[-4000:]
