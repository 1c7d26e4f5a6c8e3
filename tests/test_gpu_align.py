"""GPU: face alignment -- tpgan_ops.affine_warp_u8 bit for bit against the integer restatement
(tests/_align_ref.py), tpgan_ops.similarity_fit exactly where float32 is exact and against the
float64 closed form within a measured bound elsewhere, its status bits, and FaceAligner between
LandmarkDetector and Frontalizer."""
import ctypes

import numpy as np
import pytest
import torch

import _align_ref as A
from _cases import load_det

pytestmark = pytest.mark.gpu

Q = 65536


@pytest.fixture(autouse=True)
def _no_autotune():
    import tpgan_ops
    old = tpgan_ops.AUTOTUNE["enabled"]
    tpgan_ops.AUTOTUNE["enabled"] = False
    yield
    tpgan_ops.AUTOTUNE["enabled"] = old


# ---------------------------------------------------------------- 1. the warp, bit for bit

def _q(*v):
    return tuple(int(round(x * Q)) for x in v)


_C30, _S30 = 0.5 * np.cos(np.pi / 6), 0.5 * np.sin(np.pi / 6)
# name -> (matrix for a photo of width W, n, status)
MATRICES = {
    "identity": (lambda W: (Q, 0, 0, 0, Q, 0), 1, 0),
    "scale2": (lambda W: (2 * Q, 0, 0, 0, 2 * Q, 0), 2, 0),
    "quarter_turn": (lambda W: (0, -Q, W * Q, Q, 0, 0), 1, 0),
    "rot30_half": (lambda W: _q(_C30, -_S30, 10.3, _S30, _C30, 4.7), 1, 0),  # upsampling
    "scale3.3_off_every_edge": (lambda W: _q(3.3, 0, -20.6, 0, 3.3, -15.2), 4, 0),
    "scale40": (lambda W: _q(40, 0, 1.5, 0, 40, 2.25), 16, 8),
    "affine": (lambda W: _q(1.7, 0.4, -3.2, -0.3, 0.8, 5.5), 2, 0),  # no similarity: shear, unequal axes
}
OUT_SIZES = [(16, 24), (128, 128)]


@pytest.fixture(scope="module")
def photos(gpu):
    """1 x 1, 37 x 53 and 200 x 150 (H x W), the last a view into a wider image: its rows are 160
    pixels apart.  (numpy copies for the restatement, device tensors for the kernel.)"""
    rng = np.random.default_rng(5)
    host = [rng.integers(0, 256, (1, 1, 3), dtype=np.uint8), rng.integers(0, 256, (37, 53, 3), dtype=np.uint8)]
    wide = rng.integers(0, 256, (200, 160, 3), dtype=np.uint8)
    host.append(wide[:, 4:154])
    dev = [torch.from_numpy(host[0]).to(gpu), torch.from_numpy(host[1]).to(gpu), torch.from_numpy(wide).to(gpu)[:, 4:154]]
    assert dev[2].stride(0) == 160 * 3 and not dev[2].is_contiguous()
    return host, dev


def _raw_launch(dev, mats, out_hw, rec_hw):
    """tpg_affine_warp_u8 on sentinel-filled outputs; rec_hw[i] is the size job i's record is built for."""
    import tpgan_lib as L
    lib = L.load()
    gpu = dev[0].device
    B = len(dev)
    jb = lib.tpg_warp_job_bytes()
    jobs = (ctypes.c_uint8 * (B * jb))()
    for i, t in enumerate(dev):
        L.check(lib.tpg_warp_pack_job(jobs, i, t.data_ptr(), t.shape[0], t.shape[1], 3, t.stride(0) if t.shape[0] > 1
                                      else t.shape[1] * 3, rec_hw[i][0], rec_hw[i][1]))
    jobs_dev = torch.frombuffer(jobs, dtype=torch.uint8).to(gpu)
    m = torch.tensor(mats, dtype=torch.int32, device=gpu)
    out = torch.full((B, out_hw[0], out_hw[1], 3), 0xA5, dtype=torch.uint8, device=gpu)
    status = torch.full((B,), -7, dtype=torch.int32, device=gpu)
    L.check(lib.tpg_affine_warp_u8(B, jobs_dev.data_ptr(), m.data_ptr(), out_hw[0], out_hw[1], out.data_ptr(),
                                   status.data_ptr(), L.stream_ptr()))
    torch.cuda.synchronize()
    return out, status


@pytest.mark.parametrize("name", list(MATRICES))
def test_warp_equals_the_integer_restatement(gpu, photos, name):
    import tpgan_ops
    host, dev = photos
    make, n, st = MATRICES[name]
    mats = [make(h.shape[1]) for h in host]
    for m in mats:
        assert A.supersample(m) == (n, st == 8)
    for out_hw in OUT_SIZES:
        want = [A.warp_int(h, m, *out_hw) for h, m in zip(host, mats)]
        assert [w[1] for w in want] == [st] * 3
        # a fourth job whose record was built for another output size: its slots stay as they were
        other = (out_hw[0] + 1, out_hw[1])
        out, status = _raw_launch(dev + [dev[1]], mats + [mats[1]], out_hw, [out_hw] * 3 + [other])
        for b in range(3):
            np.testing.assert_array_equal(out[b].cpu().numpy(), want[b][0], err_msg="%s %s photo %d" % (name, out_hw, b))
        assert status.tolist() == [st] * 3 + [-7]
        assert bool((out[3] == 0xA5).all())
        # the wrapper: the same bytes from the list of views, row stride honoured
        u8, ws = tpgan_ops.affine_warp_u8(dev, torch.tensor(mats, dtype=torch.int32, device=gpu).reshape(3, 2, 3), out_hw)
        assert torch.equal(u8, out[:3]) and ws.tolist() == [st] * 3
    if name == "identity":
        np.testing.assert_array_equal(want[2][0][:128, :128], host[2][:128, :128])  # (the last out_hw is 128 x 128)
    if name == "quarter_turn":
        np.testing.assert_array_equal(want[1][0][:53, :37], np.transpose(host[1][:, ::-1], (1, 0, 2)))


def test_warp_batched_tensor_and_argument_errors(gpu, photos):
    import tpgan_ops
    host, dev = photos
    batch = torch.from_numpy(np.stack([host[1], host[1][::-1].copy()])).to(gpu)
    m = torch.tensor([_q(0.5, 0, 3, 0, 0.5, 2), _q(1.5, 0.2, 0, -0.2, 1.5, 1)], dtype=torch.int32, device=gpu)
    u8, st = tpgan_ops.affine_warp_u8(batch, m, (20, 31))
    assert tuple(u8.shape) == (2, 20, 31, 3) and st.tolist() == [0, 0]
    for b in range(2):
        np.testing.assert_array_equal(u8[b].cpu().numpy(), A.warp_int(batch[b].cpu().numpy(), m[b].tolist(), 20, 31)[0])
    # a crop of the batch: a view with batch and row strides of the parent
    crop = batch[:, 5:30, 7:40]
    u8c, _ = tpgan_ops.affine_warp_u8(crop, m, (20, 31))
    for b in range(2):
        np.testing.assert_array_equal(u8c[b].cpu().numpy(),
                                      A.warp_int(crop[b].cpu().numpy(), m[b].tolist(), 20, 31)[0])
    with pytest.raises(ValueError, match="matrix_q16"):
        tpgan_ops.affine_warp_u8(batch, m.float(), (20, 31))
    with pytest.raises(ValueError, match="matrix_q16"):
        tpgan_ops.affine_warp_u8(batch, m[:1], (20, 31))
    with pytest.raises(ValueError, match="1..4096"):
        tpgan_ops.affine_warp_u8(batch, m, (0, 31))
    with pytest.raises(ValueError, match="packed RGB"):
        tpgan_ops.affine_warp_u8(batch[:, :, ::2], m, (20, 31))
    with pytest.raises(ValueError, match="uint8"):
        tpgan_ops.affine_warp_u8([batch[0].float()], m[:1], (20, 31))
    with pytest.raises(ValueError, match="must be on"):
        tpgan_ops.affine_warp_u8([batch[0].cpu()], m[:1], (20, 31))


# ---------------------------------------------------------------- 2. the fit

TEMPLATES = {2: [[1, 2], [5, 4]],
             4: [[1, 2], [5, 2], [3, 4], [3, 7]],
             8: [[1, 2], [5, 2], [3, 4], [3, 7], [0, 0], [6, 1], [2, 5], [4, 6]]}
TURNS = [((1, 0), (0, 1)), ((0, -1), (1, 0)), ((-1, 0), (0, -1)), ((0, 1), (-1, 0))]  # rotation by k quarter turns


def _similar(q, scale, turn, t):
    r = np.array(TURNS[turn], np.float64)
    return (scale * (np.asarray(q, np.float64) @ r.T) + np.asarray(t, np.float64)).astype(np.float32)


@pytest.mark.parametrize("K", [2, 4, 8])
def test_fit_exact_cases(gpu, K):
    """Power-of-two scales and quarter turns of a small-integer template: every product, sum and
    quotient of the closed form is exact in float32, so the float and 16.16 matrices are exact."""
    import tpgan_ops
    q = TEMPLATES[K]
    cases = [(s, k, t) for s in (0.5, 1.0, 2.0, 4.0, 32.0) for k in range(4) for t in ((100.0, 50.0), (-7.5, 1000.25))]
    pts = np.stack([_similar(q, s, k, t) for s, k, t in cases])
    want = np.array([[s * TURNS[k][0][0], s * TURNS[k][0][1], t[0], s * TURNS[k][1][0], s * TURNS[k][1][1], t[1]]
                     for s, k, t in cases], np.float32)
    m, mq, st = tpgan_ops.similarity_fit(torch.from_numpy(pts).to(gpu), q)
    assert tuple(m.shape) == (len(cases), 2, 3) and m.dtype == torch.float32 and mq.dtype == torch.int32
    assert st.tolist() == [0] * len(cases)
    np.testing.assert_array_equal(m.cpu().numpy().reshape(-1, 6), want)
    np.testing.assert_array_equal(mq.cpu().numpy().reshape(-1, 6), (want.astype(np.float64) * Q).astype(np.int32))
    np.testing.assert_array_equal(A.fit32(pts, q), want)  # the restatement agrees with itself


def fit_tolerance_inputs():
    """Two groups of 32 faces, each with its own four-point template in 128 x 128: the template under
    a random similarity plus a few percent of jitter, landing in 4096 x 4096 and in 64 x 64."""
    rng = np.random.default_rng(2024)
    groups = []
    for side in (4096.0, 64.0):
        q = rng.uniform(8, 120, (4, 2)).astype(np.float32)
        s = rng.uniform(0.1, 0.3, 32) * side / 128.0 * 2
        th = rng.uniform(-np.pi, np.pi, 32)
        c = q.astype(np.float64) - q.astype(np.float64).mean(0)
        rot = np.stack([np.stack([np.cos(th), -np.sin(th)], -1), np.stack([np.sin(th), np.cos(th)], -1)], 1)
        p = s[:, None, None] * np.einsum("bij,kj->bki", rot, c) + side / 2 + rng.uniform(-0.1, 0.1, (32, 1, 2)) * side
        p = p + rng.normal(0, 0.02, p.shape) * (s[:, None, None] * 40)
        assert p.min() >= 0 and p.max() <= side
        groups.append((side, q, p.astype(np.float32)))
    return groups


def test_fit_within_the_measured_float32_bound(gpu):
    """The device's float matrix against fit64.  Per group and matrix entry the bound is 4 x the
    largest |fit32 - fit64| over the same 32 faces, plus one float32 ulp of the entry (the factor 4
    allows the device another summation order and a reciprocal; this kernel uses neither).

    Measured on these inputs (fit32 against fit64, largest over the faces; a and b are entries 0, 1,
    3, 4, t entries 2, 5):
        points in 4096 x 4096   a, b: 2.2e-6   t: 2.7e-4   -> bounds 8.6e-6 and 1.1e-3 (+ 1 ulp)
        points in 64 x 64       a, b: 4.0e-8   t: 6.7e-6   -> bounds 1.6e-7 and 2.7e-5 (+ 1 ulp)
    (|a|, |b| up to 18.6 and |t| up to 3394 in the first group, 0.28 and 64 in the second.)"""
    import tpgan_ops
    for side, q, p in fit_tolerance_inputs():
        ref = A.fit64(p, q)
        err32 = np.abs(A.fit32(p, q).astype(np.float64) - ref).max(0)
        m, mq, st = tpgan_ops.similarity_fit(torch.from_numpy(p).to(gpu), q)
        got = m.cpu().numpy().reshape(32, 6)
        assert st.tolist() == [0] * 32
        bound = 4 * err32[None, :] + np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64)
        err = np.abs(got.astype(np.float64) - ref)
        print("side %g: fit32 err %s, device err %s, bound (max) %s" % (side, err32, err.max(0), bound.max(0)))
        assert (err <= bound).all(), (side, err.max(0), bound.max(0))
        assert got[:, 0].tolist() == got[:, 4].tolist() and got[:, 1].tolist() == (-got[:, 3]).tolist()
        np.testing.assert_array_equal(mq.cpu().numpy().reshape(32, 6), A.q16(got))
        np.testing.assert_array_equal(mq.cpu().numpy().reshape(32, 6), np.rint(got.astype(np.float64) * Q).astype(np.int32))


@pytest.mark.parametrize("K", [2, 4, 8])
def test_fit_status_bits(gpu, K):
    import tpgan_lib as L
    import tpgan_ops
    lib = L.load()
    q = TEMPLATES[K]
    good = _similar(q, 2.0, 1, (40.0, 30.0))
    faces = {"good": good, "nan": good.copy(), "inf": good.copy(), "far": good.copy(),
             "coincident": np.tile(good[:1], (K, 1)), "scale33": _similar(q, 33.0, 0, (5.0, 6.0)),
             "scale32": _similar(q, 32.0, 2, (5.0, 6.0)), "shift": _similar(q, 1.0, 0, (20000.0, 3.0)),
             "shift_ok": _similar(q, 1.0, 0, (3.0, -16000.0)), "not_found": good.copy()}
    faces["nan"][K - 1, 1] = np.nan
    faces["inf"][0, 0] = -np.inf
    faces["far"][1, 0] = 2.0e9
    names = list(faces)
    want_st = {"good": 0, "nan": 1, "inf": 1, "far": 1, "coincident": 2, "scale33": 2, "scale32": 0, "shift": 2,
               "shift_ok": 0, "not_found": 4}
    pts = torch.from_numpy(np.stack([faces[n] for n in names])).to(gpu)
    in_st = torch.tensor([0] * (len(names) - 1) + [9], dtype=torch.int32, device=gpu)
    m, mq, st = tpgan_ops.similarity_fit(pts, q, in_st)
    assert st.tolist() == [want_st[n] for n in names]
    m, mq = m.cpu().numpy().reshape(-1, 6), mq.cpu().numpy().reshape(-1, 6)
    for i, n in enumerate(names):
        if want_st[n] & 3:
            assert m[i].tolist() == list(A.IDENTITY), n
            assert mq[i].tolist() == [Q, 0, 0, 0, Q, 0], n
    # "not found" travels on, the matrix is fitted all the same; without in_status bit 2 stays clear
    assert m[names.index("not_found")].tolist() == m[0].tolist() == [0.0, -2.0, 40.0, 2.0, 0.0, 30.0]
    assert m[names.index("scale32")].tolist() == [-32.0, 0.0, 5.0, 0.0, -32.0, 6.0]
    assert m[names.index("shift_ok")].tolist() == [1.0, 0.0, 3.0, 0.0, 1.0, -16000.0]
    assert tpgan_ops.similarity_fit(pts, q)[2].tolist() == [want_st[n] & 3 for n in names]
    # every slot is written: the raw call on sentinel-filled outputs gives the same arrays
    B = len(names)
    outs = [torch.full((B, 6), 7.5, device=gpu), torch.full((B, 6), 7, dtype=torch.int32, device=gpu),
            torch.full((B,), 7, dtype=torch.int32, device=gpu)]
    tmpl = (ctypes.c_float * (2 * K))(*[float(v) for r in q for v in r])
    L.check(lib.tpg_similarity_fit(B, K, pts.data_ptr(), tmpl, in_st.data_ptr(), *[t.data_ptr() for t in outs],
                                   L.stream_ptr()))
    np.testing.assert_array_equal(outs[0].cpu().numpy(), m)
    np.testing.assert_array_equal(outs[1].cpu().numpy(), mq)
    assert outs[2].tolist() == st.tolist()


def test_fit_argument_errors(gpu):
    import tpgan_ops
    pts = torch.zeros(2, 4, 2, device=gpu)
    with pytest.raises(ValueError, match="device tensor"):
        tpgan_ops.similarity_fit(pts.cpu(), TEMPLATES[4])
    with pytest.raises(ValueError, match="float32"):
        tpgan_ops.similarity_fit(pts.double(), TEMPLATES[4])
    with pytest.raises(ValueError, match="template"):
        tpgan_ops.similarity_fit(pts, TEMPLATES[2])
    with pytest.raises(ValueError, match="2..8"):
        tpgan_ops.similarity_fit(torch.zeros(2, 9, 2, device=gpu), [[0, 0]] * 9)
    with pytest.raises(ValueError, match="in_status"):
        tpgan_ops.similarity_fit(pts, TEMPLATES[4], torch.zeros(2, device=gpu))
    with pytest.raises(RuntimeError, match="coincide"):
        tpgan_ops.similarity_fit(pts, [[3, 3]] * 4)
    with pytest.raises(RuntimeError, match="not finite"):
        tpgan_ops.similarity_fit(pts, [[3, 3], [4, float("nan")], [5, 5], [6, 6]])


# ---------------------------------------------------------------- 3. composition

TEMPLATE = [[44.0, 52.0], [84.0, 52.0], [64.0, 76.0], [64.0, 98.0]]


def _raw_photos(gpu):
    from _resize_ref import load_golden
    g = load_golden()
    imgs = [g["%d:raw" % k] for k in (1, 2, 3)]  # 150x170, 96x110, 200x140
    assert len({im.shape for im in imgs}) == 3
    return [torch.from_numpy(im).to(gpu) for im in imgs]


def _detector_model():
    """The deterministic MobileNetV2 weights of the feature golden with the six location convs times
    256 (tests/test_gpu_landmarks.py: the plain weights put every location below 0.5 px)."""
    import MobileNetV2 as MN
    from oracle.det_init import det_module_state
    m = MN.MobileNetV2()
    sd = m.state_dict()
    new = {k: torch.from_numpy(np.asarray(v)).to(sd[k].dtype) for k, v in det_module_state(m, "mnv2/").items()}
    for k in new:
        if k.startswith("ssd_head.location_layer."):
            new[k] = new[k] * 256.0
    m.load_state_dict(new)
    return m


@pytest.fixture(scope="module")
def composed(gpu):
    import D_and_G_model as DG
    import tpgan_infer
    import tpgan_ops
    old = tpgan_ops.AUTOTUNE["enabled"]
    tpgan_ops.AUTOTUNE["enabled"] = False
    try:
        imgs = _raw_photos(gpu)
        det = tpgan_infer.LandmarkDetector(_detector_model(), device=gpu, compute_dtype=torch.bfloat16,
                                           confidence_threshold=0.2, on_missing="best")
        G = DG.Generator(64, 347, use_batchnorm=False)
        load_det(G, "G/", torch.float32)
        al = tpgan_infer.FaceAligner(TEMPLATE, device=gpu)
        fz = tpgan_infer.Frontalizer(G, device=gpu, compute_dtype=torch.bfloat16, detector=det)
        fza = tpgan_infer.Frontalizer(G, device=gpu, compute_dtype=torch.bfloat16, detector=det, aligner=al)
        with tpgan_ops.deterministic():
            d = det.detect(imgs)
            da = det.detect(imgs, aligner=al)
            out = fz(imgs)
            outa = fza(imgs)
        torch.cuda.synchronize()
    finally:
        tpgan_ops.AUTOTUNE["enabled"] = old
    return {"imgs": imgs, "det": det, "al": al, "fz": fz, "fza": fza, "d": d, "da": da, "out": out, "outa": outa}


def test_detect_with_aligner_is_fit_warp_detect(gpu, composed):
    import tpgan_ops
    imgs, det, al, d, da = (composed[k] for k in ("imgs", "det", "al", "d", "da"))
    print("first pass points_photo", d["points_photo"].tolist(), "matrix", da["matrix"].tolist())
    m, mq, fst = tpgan_ops.similarity_fit(d["points_photo"], TEMPLATE, d["status"])
    u8, wst = tpgan_ops.affine_warp_u8(imgs, mq)
    assert torch.equal(da["u8_128"], u8) and da["u8_128"].dtype == torch.uint8
    assert torch.equal(da["matrix"], m) and torch.equal(da["align_status"], fst | wst)
    assert not bool((da["align_status"] & 3).any())
    assert not torch.equal(da["u8_128"], d["u8_128"])  # the aligned faces are not the squashed photos
    a = al.align(imgs, d["points_photo"], d["status"])
    assert sorted(a) == ["matrix", "matrix_q16", "status", "u8"]
    assert torch.equal(a["u8"], u8) and torch.equal(a["matrix_q16"], mq) and torch.equal(a["status"], fst | wst)
    # the second pass is a plain detection on the aligned faces
    with tpgan_ops.deterministic():
        d2 = det.detect(da["u8_128"])
    for k in ("points", "score", "anchor", "boxes", "status", "u8_128"):
        assert torch.equal(da[k], d2[k]), k
    # points_photo: the aligned points through the matrix, back in the photo's own pixels
    pts, mat = da["points"].cpu().numpy(), da["matrix"].cpu().numpy()
    want = pts[..., 0:1] * mat[:, None, :, 0] + pts[..., 1:2] * mat[:, None, :, 1] + mat[:, None, :, 2]
    np.testing.assert_allclose(da["points_photo"].cpu().numpy(), want, rtol=1e-6, atol=1e-4)
    assert sorted(da) == sorted(list(d) + ["matrix", "align_status"])


def test_frontalizer_with_aligner(gpu, composed):
    import tpgan_infer
    import tpgan_ops
    imgs, det, al, fz, fza, da, out, outa = (composed[k] for k in ("imgs", "det", "al", "fz", "fza", "da", "out", "outa"))
    with tpgan_ops.deterministic():
        assert torch.equal(outa, fz(da["u8_128"]))
        assert not torch.equal(outa, out)
        r = fza.evaluate(imgs, None, frontal=imgs)
        assert torch.equal(r["fake_u8"], outa)
        assert torch.equal(r["sse"], tpgan_ops.image_metrics(outa, da["u8_128"])[0])  # frontal aligned the same way
    with pytest.raises(ValueError, match="needs a detector"):
        tpgan_infer.Frontalizer(fz.G, device=gpu, aligner=al)
    with pytest.raises(ValueError, match="FaceAligner"):
        tpgan_infer.Frontalizer(fz.G, device=gpu, detector=det, aligner=object())
    with pytest.raises(ValueError, match="128 x 128"):
        tpgan_infer.Frontalizer(fz.G, device=gpu, detector=det, aligner=tpgan_infer.FaceAligner(TEMPLATE, gpu, (64, 64)))
    with pytest.raises(ValueError, match="128 x 128"):
        det.detect(imgs, aligner=tpgan_infer.FaceAligner(TEMPLATE, gpu, (64, 64)))


def test_without_aligner_nothing_changes(gpu, composed):
    """detect(imgs) and Frontalizer(G, detector=det)(imgs) against the same steps made one by one
    through the calls that were there before the aligner."""
    import tpgan_ops
    from DataAndDataset import FaceBatcher
    imgs, det, fz, d, out = (composed[k] for k in ("imgs", "det", "fz", "d", "out"))
    fb = FaceBatcher(gpu)
    with tpgan_ops.deterministic(), torch.no_grad():
        u8 = fb.resize(imgs, (128, 128))
        loc, cls = det._head(u8)
        points, score, anchor, boxes, status = tpgan_ops.ssd_landmarks(loc, cls, 0.2)
        wh = np.array([[t.shape[1], t.shape[0]] for t in imgs], np.float64)
        photo = points * torch.from_numpy((wh / 128.0).astype(np.float32)).to(gpu)[:, None, :]
        want = {"points": points, "points_photo": photo, "score": score, "anchor": anchor, "boxes": boxes,
                "status": status, "u8_128": u8}
        assert sorted(d) == sorted(want)
        for k in want:
            assert torch.equal(d[k], want[k]), k
        assert torch.equal(out, fz.frontalize_batch(fb.from_points(u8, boxes), None))
        assert torch.equal(det.detect(imgs, aligner=None)["points"], points)


def test_a_failed_fit_raises(gpu, composed):
    """Four landmarks on one point: no scale or rotation can be fitted; detect names the faces."""
    imgs, det, al = composed["imgs"], composed["det"], composed["al"]
    loc = torch.full((3, 12, 2), 60.5, device=gpu)
    cls = torch.zeros(3, 12, 5, device=gpu)
    head = det._head
    det._head = lambda u8: (loc[:u8.shape[0]], cls[:u8.shape[0]])
    try:
        with pytest.raises(ValueError, match=r"cannot align face\(s\) \[0, 1, 2\].*degenerate"):
            det.detect(imgs, aligner=al)
        a = al.align(imgs, torch.full((3, 4, 2), float("nan"), device=gpu))
        assert a["status"].tolist() == [1, 1, 1]
        with pytest.raises(ValueError, match=r"cannot align face\(s\) \[0, 1, 2\].*NaN"):
            al.check_status(a["status"].tolist())
        h, w = min(imgs[1].shape[0], 128), min(imgs[1].shape[1], 128)
        assert torch.equal(a["u8"][1, :h, :w], imgs[1][:h, :w])  # the identity: a copy of the top-left
    finally:
        det._head = head
