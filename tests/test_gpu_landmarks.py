"""GPU: the landmark front end -- tpgan_ops.ssd_landmarks against the existing decoder bit for bit
and against the float64 restatement (tests/_landmark_ref.py), its boxes against the existing box
kernel, u8_to_unit, landmark_accuracy against the reference's recorded values
(landmark_golden.npz), and tpgan_infer.LandmarkDetector alone and in front of the Frontalizer."""
import ctypes
import os

import numpy as np
import pytest
import torch

import _landmark_ref as R
from _cases import golden, load_det

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 5), (3, 394, 5), (2, 257, 6), (2, 4096, 5)]
IDX4 = [[0, 0], [1, 1], [2, 2], [3, 3], [3, 3]]  # [le, re, nose, mouth, mouth] of four points


@pytest.fixture(autouse=True)
def _no_autotune():
    import tpgan_ops
    old = tpgan_ops.AUTOTUNE["enabled"]
    tpgan_ops.AUTOTUNE["enabled"] = False
    yield
    tpgan_ops.AUTOTUNE["enabled"] = old


def _random_head(shape, gpu):
    B, n, C = shape
    rng = np.random.RandomState(B * 10007 + n * 13 + C)
    loc = (rng.rand(B, n, 2) * 150 - 11).astype(np.float32)
    cls = (rng.randn(B, n, C) * 1.5).astype(np.float32)
    return torch.from_numpy(loc).to(gpu), torch.from_numpy(cls).to(gpu)


def _lattice_head(gpu):
    rng = np.random.RandomState(100)
    cls = (rng.randint(-32, 33, (3, 394, 5)) / 8.0).astype(np.float32)
    loc = (rng.rand(3, 394, 2) * 150 - 11).astype(np.float32)
    return torch.from_numpy(loc).to(gpu), torch.from_numpy(cls).to(gpu)


def _scale(B, gpu):
    s = np.tile((128.0 / np.array([[150, 170], [96, 110], [200, 140]], np.float64)).astype(np.float32), (B, 1))[:B]
    return torch.from_numpy(np.ascontiguousarray(s)).to(gpu)


# ---------------------------------------------------------------- 1. decode against ssd_decode

@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_decode_equals_ssd_decode_top1(gpu, shape):
    import tpgan_ops
    loc, cls = _random_head(shape, gpu)
    realised = float(tpgan_ops.ssd_landmarks(loc, cls, 0.0)[1][0, 0])  # conf == a score: strict > fails
    for conf in (0.0, 0.5, realised):
        points, score, anchor, boxes, status = tpgan_ops.ssd_landmarks(loc, cls, conf)
        keep, sc = tpgan_ops.ssd_decode(loc, cls, conf, 20.0, 1)
        keep, sc = keep[:, :4, 0], sc[:, :4, 0]
        found = keep >= 0
        assert torch.equal(anchor[found], keep[found])
        assert torch.equal(score[found], sc[found])  # bit for bit
        bits = (status[:, None] >> torch.arange(4, device=gpu)[None, :]) & 1
        assert torch.equal(bits != 0, ~found)
        assert int((status & 16).max()) == 0
        # the best anchor is reported whether found or not: its point is loc[anchor]
        want = torch.gather(loc, 1, anchor.long()[:, :, None].expand(-1, -1, 2))
        assert torch.equal(points, want)
        if conf == 0.0:
            assert bool(found.all())
    assert not bool(found[0, 0])  # the strict case really occurred


# ---------------------------------------------------------------- 2. ties, NaN, coverage

def test_ties_take_the_lowest_index(gpu):
    import tpgan_ops
    n = 600
    cls = torch.zeros(2, n, 5, device=gpu)
    loc = torch.arange(2 * n * 2, dtype=torch.float32, device=gpu).reshape(2, n, 2)
    # image 0: every logit equal -> anchor 0 for every class
    # image 1: two equal maxima per class, in different waves' strides, planted in either order
    pairs = {0: (70, 454), 1: (300, 130), 2: (511, 512), 3: (599, 3)}
    for l, (i, j) in pairs.items():
        cls[1, i, l] = cls[1, j, l] = 3.0
    points, score, anchor, boxes, status = tpgan_ops.ssd_landmarks(loc, cls, 0.1)
    assert anchor[0].tolist() == [0, 0, 0, 0]
    assert anchor[1].tolist() == [70, 130, 511, 3]
    assert status.tolist() == [0, 0]
    assert float((score[0] - 0.2).abs().max()) <= 1e-6 and torch.equal(points[0], loc[0, :1].expand(4, 2))


def test_nan_rows_are_never_chosen(gpu):
    import tpgan_ops
    loc, cls = _random_head((3, 257, 6), gpu)
    cls = cls.clone()
    clean = tpgan_ops.ssd_landmarks(loc, cls, 0.0)
    # image 0: the winning rows get a NaN logit (and would otherwise win by far)
    for l in range(4):
        a = int(clean[2][0, l])
        cls[0, a, l] = 50.0
        cls[0, a, 5] = float("nan")
    # image 1: class 2's logit is NaN at every anchor: logsumexp spreads it, no score of that
    # image is a number
    cls[1, :, 2] = float("nan")
    points, score, anchor, boxes, status = tpgan_ops.ssd_landmarks(loc, cls, 0.0)
    ref = R.decode_top1(loc.cpu().numpy(), cls.cpu().numpy(), 0.0)
    assert np.array_equal(anchor.cpu().numpy(), ref[2])
    for l in range(4):
        assert int(anchor[0, l]) != int(clean[2][0, l]) and int(anchor[0, l]) >= 0
    assert anchor[1].tolist() == [-1, -1, -1, -1] and score[1].tolist() == [0.0] * 4
    assert bool(torch.isnan(points[1]).all())
    st = status.tolist()
    assert st[0] == 0 and st[2] == 0
    assert st[1] & (1 << 2 | 16) == (1 << 2 | 16) and st[1] == 31
    assert np.array_equal(status.cpu().numpy(), ref[3])
    assert boxes[1].tolist() == R.boxes(np.full((1, 4, 2), np.nan, np.float32))[0].tolist()
    assert torch.equal(anchor[2], clean[2][2]) and torch.equal(score[2], clean[1][2])


def test_every_output_slot_is_written(gpu):
    import tpgan_lib as L
    lib = L.load()
    B, n, C = 3, 394, 5
    loc, cls = _random_head((B, n, C), gpu)
    wh = (ctypes.c_int32 * 8)(40, 40, 40, 40, 40, 32, 48, 32)
    outs = [torch.full((B, 4, 2), 7.0, device=gpu), torch.full((B, 4), 7.0, device=gpu),
            torch.full((B, 4), 7, dtype=torch.int32, device=gpu), torch.full((B, 4, 4), 7, dtype=torch.int32, device=gpu),
            torch.full((B,), 7, dtype=torch.int32, device=gpu)]
    # (the values are chosen so that no true result is 7: locations are not integers, scores
    # are below 1, and the anchors / boxes / status are checked against a second call)
    L.check(lib.tpg_ssd_landmarks(B, n, C, loc.data_ptr(), cls.data_ptr(), 0.0, None, wh,
                                  *[t.data_ptr() for t in outs], L.stream_ptr()))
    import tpgan_ops
    want = tpgan_ops.ssd_landmarks(loc, cls, 0.0)
    for got, w in zip(outs, want):
        assert torch.equal(got, w)
    assert not bool((outs[0] == 7).any()) and not bool((outs[1] == 7).any())


# ---------------------------------------------------------------- 3. decode against float64

def test_decode_equals_float64_restatement_on_lattice_logits(gpu):
    import tpgan_ops
    loc, cls = _lattice_head(gpu)
    x = cls.cpu().numpy().astype(np.float64)
    p = np.exp(x - x.max(2, keepdims=True))
    p = p / p.sum(2, keepdims=True)
    top2 = np.sort(p[:, :, :4], axis=1)[:, -2:, :]
    assert ((top2[:, 1] - top2[:, 0]) / top2[:, 1]).min() > 1e-5  # the inputs: far above fp32 rounding (6e-8)
    for conf in (0.0, 0.5):
        points, score, anchor, boxes, status = tpgan_ops.ssd_landmarks(loc, cls, conf)
        rp, rs, ra, rst = R.decode_top1(loc.cpu().numpy(), cls.cpu().numpy(), conf)
        assert np.array_equal(anchor.cpu().numpy(), ra)
        assert np.array_equal(points.cpu().numpy(), rp)
        assert np.abs(score.cpu().numpy() - rs).max() <= 1e-6
        assert np.array_equal(status.cpu().numpy(), rst)


# ---------------------------------------------------------------- 4. boxes

def _check_boxes(gpu, loc, cls, conf, scale, expect_bad=False):
    from DataAndDataset import FaceBatcher
    import tpgan_ops
    fb4 = FaceBatcher(gpu, pts_idx=IDX4, check=False)
    unscaled = tpgan_ops.ssd_landmarks(loc, cls, conf)[0]
    points, score, anchor, boxes, status = tpgan_ops.ssd_landmarks(loc, cls, conf, scale)
    lm5, want, wst = fb4.landmark_boxes(unscaled, scale)
    assert torch.equal(boxes, want)
    assert torch.equal(points, lm5[:, :4])
    assert torch.equal((status & 16) != 0, wst != 0)
    assert boxes.cpu().numpy().tolist() == R.boxes(points.cpu().numpy()).tolist()
    assert bool((status & 16).any()) == expect_bad
    return points, boxes, status


@pytest.mark.parametrize("scaled", [False, True], ids=["plain", "scaled"])
def test_boxes_equal_the_box_kernel_and_process(gpu, scaled):
    for shape in SHAPES[1:]:
        loc, cls = _random_head(shape, gpu)
        _check_boxes(gpu, loc, cls, 0.5, _scale(shape[0], gpu) if scaled else None)
    loc, cls = _lattice_head(gpu)
    _check_boxes(gpu, loc, cls, 0.0, _scale(3, gpu) if scaled else None)


@pytest.mark.parametrize("scaled", [False, True], ids=["plain", "scaled"])
def test_boxes_edge_coordinates(gpu, scaled):
    """A negative coordinate, coordinates exactly on an integer (floor keeps them), and a
    location of inf: status bit 4 and the zeros the existing kernel writes."""
    n = 12
    cls = torch.zeros(2, n, 5, device=gpu)
    loc = torch.full((2, n, 2), 60.5, device=gpu)
    for l in range(4):
        cls[:, l + 2, l] = 4.0
    loc[0, 2] = torch.tensor([-3.5, 17.0])
    loc[0, 3] = torch.tensor([-8.0, -0.25])
    loc[0, 4] = torch.tensor([127.0, 0.0])
    loc[0, 5] = torch.tensor([64.0, 1e9])
    loc[1, 2] = torch.tensor([float("inf"), 5.0])
    loc[1, 4] = torch.tensor([2.5, float("-inf")])
    loc[1, 5] = torch.tensor([3e9, -3e9])
    scale = torch.tensor([[1.0, 0.5], [0.75, 1.0]], device=gpu) if scaled else None
    points, boxes, status = _check_boxes(gpu, loc, cls, 0.5, scale, expect_bad=True)
    assert status.tolist() == [0, 16]
    if not scaled:
        assert boxes[0, 0].tolist() == [-4 - 20 + 1, 17 - 20 + 1, -4 + 20 + 1, 17 + 20 + 1]
        assert boxes[0, 1].tolist() == [-8 - 19, -1 - 19, -8 + 21, -1 + 21]
        assert boxes[1, 0].tolist() == [0 - 19, 5 - 19, 0 + 21, 5 + 21]
        assert boxes[1, 2].tolist() == [2 - 19, 0 - 15, 2 + 21, 0 + 17]
        assert boxes[1, 3].tolist() == [0 - 23, 0 - 15, 0 + 25, 0 + 17]


# ---------------------------------------------------------------- 5. u8_to_unit

@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16], ids=["f32", "bf16", "f16"])
@pytest.mark.parametrize("first", [0, 46], ids=["0-209", "46-255"])  # 210 bytes per image pair: all 256 in two
def test_u8_to_unit_exact(gpu, dtype, first):
    import tpgan_ops
    u = (np.arange(2 * 5 * 7 * 3) + first).astype(np.uint8).reshape(2, 5, 7, 3)
    assert first + u.size - 1 <= 255
    img = torch.from_numpy(u).to(gpu)
    want = torch.from_numpy((u.astype(np.float32) / np.float32(255)).transpose(0, 3, 1, 2).copy()).to(dtype)
    cl = tpgan_ops.u8_to_unit(img, dtype)  # channels-last, the conv kernels' layout
    assert cl.dtype == dtype and tuple(cl.shape) == (2, 3, 5, 7) and cl.stride(1) == 1
    assert torch.equal(cl.cpu(), want)
    plain = torch.full((2, 3, 5, 7), 9.0, dtype=dtype, device=gpu)
    assert tpgan_ops.u8_to_unit(img, out=plain) is plain and plain.is_contiguous()
    assert torch.equal(plain.cpu(), want)
    big = torch.full((2, 4, 8, 11), 9.0, dtype=dtype, device=gpu)
    view = big[:, 1:, 2:7, 3:10]
    tpgan_ops.u8_to_unit(img, out=view)
    assert torch.equal(view.cpu(), want)
    mask = torch.ones_like(big, dtype=torch.bool)
    mask[:, 1:, 2:7, 3:10] = False
    assert bool((big[mask] == 9.0).all())  # nothing outside the view was touched
    # a strided u8 source: every other column of a wider image
    wide = torch.zeros(2, 5, 14, 3, dtype=torch.uint8, device=gpu)
    wide[:, :, ::2] = img
    assert torch.equal(tpgan_ops.u8_to_unit(wide[:, :, ::2], dtype).cpu(), want)


def test_landmark_ops_argument_errors(gpu):
    import tpgan_ops
    loc, cls = _random_head((2, 20, 5), gpu)
    with pytest.raises(ValueError, match="device tensor"):
        tpgan_ops.ssd_landmarks(loc.cpu(), cls, 0.5)
    with pytest.raises(ValueError, match="float32"):
        tpgan_ops.ssd_landmarks(loc, cls.half(), 0.5)
    with pytest.raises(ValueError, match="float32"):
        tpgan_ops.ssd_landmarks(loc[0], cls, 0.5)
    with pytest.raises(ValueError, match="C >= 5"):
        tpgan_ops.ssd_landmarks(loc, cls[:, :, :4], 0.5)
    with pytest.raises(ValueError, match="4096"):
        tpgan_ops.ssd_landmarks(torch.zeros(1, 4097, 2, device=gpu), torch.zeros(1, 4097, 5, device=gpu), 0.5)
    with pytest.raises(ValueError, match="scale"):
        tpgan_ops.ssd_landmarks(loc, cls, 0.5, scale=torch.ones(3, 2, device=gpu))
    with pytest.raises(ValueError, match="device tensor"):
        tpgan_ops.u8_to_unit(torch.zeros(1, 4, 4, 3, dtype=torch.uint8), torch.float32)
    with pytest.raises(ValueError, match="dtype"):
        tpgan_ops.u8_to_unit(torch.zeros(1, 4, 4, 3, dtype=torch.uint8, device=gpu), torch.float64)
    pts = torch.zeros(2, 4, 2, device=gpu)
    with pytest.raises(ValueError, match="bands"):
        tpgan_ops.landmark_accuracy(pts, pts, thresholds=range(1, 10), weights=[1.0] * 9)
    with pytest.raises(ValueError, match="bands"):
        tpgan_ops.landmark_accuracy(pts, pts, thresholds=(), weights=())
    with pytest.raises(ValueError, match="ascend"):
        tpgan_ops.landmark_accuracy(pts, pts, thresholds=(5, 4), weights=(1, 1))
    with pytest.raises(ValueError, match="status"):
        tpgan_ops.landmark_accuracy(pts, pts, status=torch.zeros(2, device=gpu))
    with pytest.raises(ValueError, match="device tensor"):
        tpgan_ops.landmark_accuracy(pts.cpu(), pts)


# ---------------------------------------------------------------- 6. accuracy

def test_accuracy_equals_the_reference(gpu):
    import tpgan_ops
    G = golden("landmark_golden.npz")
    K = int(G["ncases"])
    pred = torch.from_numpy(np.stack([G["%d:dec_point" % k][:4] for k in range(K)])).to(gpu)
    truth = torch.from_numpy(np.concatenate([G["%d:truth" % k] for k in range(K)])).to(gpu)
    want = np.array([G["%d:acc" % k] for k in range(K)], np.float32)
    acc = tpgan_ops.landmark_accuracy(pred, truth)
    assert acc.dtype == torch.float32 and np.array_equal(acc.cpu().numpy(), want)  # exactly
    singles = torch.cat([tpgan_ops.landmark_accuracy(pred[k:k + 1], truth[k:k + 1].reshape(1, 4, 2)) for k in range(K)])
    assert torch.equal(singles, acc)
    # the whole chain on the device: the fixture's head outputs decoded, then scored
    for k in range(K):
        loc, cls = torch.from_numpy(G["%d:loc" % k]).to(gpu), torch.from_numpy(G["%d:cls" % k]).to(gpu)
        points, score, anchor, boxes, status = tpgan_ops.ssd_landmarks(loc, cls, 0.5)
        assert anchor[0].tolist() == G["%d:planted" % k][:4].tolist() and status.tolist() == [0]
        assert np.array_equal(points.cpu().numpy()[0], G["%d:dec_point" % k][:4])
        assert np.abs(score.cpu().numpy()[0] - G["%d:dec_score" % k][:4]).max() <= 1e-6
        assert float(tpgan_ops.landmark_accuracy(points, truth[k:k + 1], status)) == float(want[k])


def test_accuracy_missing_nan_and_custom_bands(gpu):
    import tpgan_ops
    truth = torch.zeros(3, 4, 2, device=gpu)
    pred = torch.tensor([[[3, 0], [0, 7], [12, 0], [0, 40]],
                         [[3, 0], [0, 7], [float("nan"), 0], [0, 40]],
                         [[3, 4], [0, 5.5], [0.5, 0], [0, 0]]], dtype=torch.float32, device=gpu)
    f = np.float32
    assert tpgan_ops.landmark_accuracy(pred, truth).tolist() == [
        float((f(1.0) + f(0.9) + f(0.65) + f(0.1)) / f(4)), float((f(1.0) + f(0.9) + f(0.0) + f(0.1)) / f(4)),
        float((f(1.0) + f(0.9) + f(1.0) + f(0.0)) / f(4))]
    status = torch.tensor([1 | 8, 2, 16], dtype=torch.int32, device=gpu)  # bit 4 is no missing bit
    got = tpgan_ops.landmark_accuracy(pred, truth, status)
    assert got.tolist() == [float((f(0.0) + f(0.9) + f(0.65) + f(0.0)) / f(4)),
                            float((f(1.0) + f(0.0) + f(0.0) + f(0.1)) / f(4)),
                            float((f(1.0) + f(0.9) + f(1.0) + f(0.0)) / f(4))]
    assert np.array_equal(got.cpu().numpy(), R.accuracy(pred.cpu().numpy(), truth.cpu().numpy(), status.cpu().numpy()))
    custom = tpgan_ops.landmark_accuracy(pred, truth, thresholds=(0.5, 5, 100), weights=(4.0, 2.0, 1.0))
    want = R.accuracy(pred.cpu().numpy(), truth.cpu().numpy(), None, (0.5, 5, 100), (4.0, 2.0, 1.0))
    assert np.array_equal(custom.cpu().numpy(), want)
    assert custom.tolist() == [(2 + 1 + 1 + 1) / 4, (2 + 1 + 0 + 1) / 4, (2 + 1 + 4 + 0) / 4]
    one = tpgan_ops.landmark_accuracy(pred, truth, thresholds=(8,), weights=(0.5,))
    assert one.tolist() == [0.25, 0.25, 0.375]
    eight = tpgan_ops.landmark_accuracy(pred, truth, thresholds=range(1, 9), weights=[1.0] * 8)
    assert eight.tolist() == [0.5, 0.5, 0.75]


# ---------------------------------------------------------------- 7. the detector on the reference's run

@pytest.fixture(scope="module")
def det_sd():
    """The feature golden's deterministic MobileNetV2 weights as a CPU state_dict."""
    import MobileNetV2 as MN
    from oracle.det_init import det_module_state
    m = MN.MobileNetV2()
    sd = m.state_dict()
    return {k: torch.from_numpy(np.asarray(v)).to(sd[k].dtype) for k, v in det_module_state(m, "mnv2/").items()}


def _mnv2(sd):
    import MobileNetV2 as MN
    m = MN.MobileNetV2()
    m.load_state_dict(sd)
    return m


def test_detector_on_the_reference_run(gpu, det_sd):
    import tpgan_infer
    import tpgan_ops
    G = golden("features_golden.npz")
    det = tpgan_infer.LandmarkDetector(_mnv2(det_sd), device=gpu, compute_dtype=torch.float32)
    assert not det.model.training and not any(p.requires_grad for p in det.model.parameters())
    assert all(isinstance(p._tpg_flat, tpgan_ops._FrozenPack) for p in det.model.parameters())
    x = torch.from_numpy(G["in:x128"]).float().to(gpu)
    with torch.no_grad(), tpgan_ops.compute_dtype(torch.float32):
        loc, cls = det.model(x)
    loc, cls = loc.float(), cls.float()
    points, score, anchor, boxes, status = tpgan_ops.ssd_landmarks(loc, cls, 0.5)
    # (from the fixture's eval:cls on the CPU: best scores 0.241 .. 0.286, margins to the runner-up
    # >= 1.9e-3; the product's fp32 parity on these logits is ~1e-6)
    assert anchor.tolist() == [[334, 36, 373, 253]] * 2
    ref = R.decode_top1(G["eval:loc"].astype(np.float32), G["eval:cls"].astype(np.float32), 0.5)
    assert ref[2].tolist() == anchor.tolist()
    got, want = points.cpu().numpy().astype(np.float64), np.stack([G["eval:loc"][b, [334, 36, 373, 253]] for b in (0, 1)])
    assert np.linalg.norm(got - want) <= 1e-3 * np.linalg.norm(want)
    assert np.abs(score.cpu().numpy() - ref[1]).max() <= 1e-4 and 0.24 < float(score.min()) and float(score.max()) < 0.29
    assert status.tolist() == [15, 15]
    assert tpgan_ops.ssd_landmarks(loc, cls, 0.2)[4].tolist() == [0, 0]
    # the same head outputs through detect(): nothing is returned for a batch with a missing landmark
    det._head = lambda u8: (loc, cls)
    photos = torch.zeros(2, 128, 128, 3, dtype=torch.uint8, device=gpu)
    with pytest.raises(ValueError, match=r"face\(s\) \[0, 1\].*left_eye.*mouth"):
        det.detect(photos)
    det.on_missing = "best"
    d = det.detect(photos)
    assert d["status"].tolist() == [15, 15] and d["anchor"].tolist() == anchor.tolist()
    assert torch.equal(d["boxes"], boxes) and torch.equal(d["points"], points)
    det.on_missing, det.confidence_threshold = "raise", 0.2
    assert det.detect(photos)["status"].tolist() == [0, 0]
    bad = loc.clone()
    bad[1, 36, 0] = float("inf")
    det._head = lambda u8: (bad, cls)
    with pytest.raises(ValueError, match=r"cannot convert float NaN to integer.*\[1\]"):
        det.detect(photos)
    truth = torch.from_numpy(want.astype(np.float32)).to(gpu) + 3.0
    assert det.accuracy(points, truth).tolist() == [1.0, 1.0]
    assert det.accuracy(points, truth, status).tolist() == [0.0, 0.0]


# ---------------------------------------------------------------- 8. composition

def _raw_photos(gpu):
    from _resize_ref import load_golden
    g = load_golden()
    imgs = [g["%d:raw" % k] for k in (1, 2, 3)]  # 150x170, 96x110, 200x140
    assert len({im.shape for im in imgs}) == 3
    t = np.linspace(0.0, 1.0, 68)
    base = np.stack([0.5 + 0.22 * np.cos(2 * np.pi * t * 3), 0.5 + 0.22 * np.sin(2 * np.pi * t * 5)], -1)
    lm = np.stack([base * [im.shape[1], im.shape[0]] for im in imgs]).astype(np.float32)
    return [torch.from_numpy(im).to(gpu) for im in imgs], torch.from_numpy(lm).to(gpu)


@pytest.fixture(scope="module")
def wide_sd(det_sd):
    """det_sd with the six location convs times 256: with the deterministic weights every predicted
    location is below 0.5 px (all four boxes equal); a power of two scales the fp32 head exactly."""
    sd = {k: v.clone() for k, v in det_sd.items()}
    scaled = [k for k in sd if k.startswith("ssd_head.location_layer.")]
    assert len(scaled) == 12
    for k in scaled:
        sd[k] = sd[k] * 256.0
    return sd


def _generator():
    import D_and_G_model as DG
    G = DG.Generator(64, 347, use_batchnorm=False)
    load_det(G, "G/", torch.float32)
    return G


@pytest.fixture(scope="module")
def composed(gpu, wide_sd):
    """One detector + Frontalizer and their results on the three photos, shared by the tests below."""
    import tpgan_infer
    import tpgan_ops
    old = tpgan_ops.AUTOTUNE["enabled"]
    tpgan_ops.AUTOTUNE["enabled"] = False
    try:
        imgs, lm = _raw_photos(gpu)
        det = tpgan_infer.LandmarkDetector(_mnv2(wide_sd), device=gpu, compute_dtype=torch.bfloat16,
                                           confidence_threshold=0.2)
        fz = tpgan_infer.Frontalizer(_generator(), device=gpu, compute_dtype=torch.bfloat16, detector=det)
        with tpgan_ops.deterministic():
            d = det.detect(imgs)
            out = fz(imgs)
        torch.cuda.synchronize()
    finally:
        tpgan_ops.AUTOTUNE["enabled"] = old
    return {"imgs": imgs, "lm": lm, "det": det, "fz": fz, "d": d, "out": out}


def test_detect_outputs(gpu, composed):
    d, imgs = composed["d"], composed["imgs"]
    print("points", d["points"].tolist(), "score", d["score"].tolist())
    assert tuple(d["points"].shape) == (3, 4, 2) and d["points"].dtype == torch.float32
    assert d["status"].tolist() == [0, 0, 0] and float(d["score"].min()) > 0.2
    pts = d["points"].cpu().numpy()
    assert any(len({tuple(p) for p in pts[b]}) > 1 for b in range(3))  # not degenerate: the points of a face differ
    assert len({tuple(b) for b in d["boxes"][0, :, :2].tolist()}) > 1
    wh = np.array([[im.shape[1], im.shape[0]] for im in imgs], np.float64)
    want = pts * (wh / 128.0).astype(np.float32)[:, None, :]
    assert np.array_equal(d["points_photo"].cpu().numpy(), want)
    assert d["u8_128"].dtype == torch.uint8 and tuple(d["u8_128"].shape) == (3, 128, 128, 3)
    assert d["anchor"].dtype == torch.int32 and d["boxes"].dtype == torch.int32


def test_from_points_equals_from_raw_and_the_box_route(gpu, composed):
    from DataAndDataset import PATCH_NAMES, PATCH_SIZE, FaceBatcher
    d, imgs, lm = composed["d"], composed["imgs"], composed["lm"]
    fb = FaceBatcher(gpu)
    p = fb.from_points(d["u8_128"], d["boxes"])
    r = fb.from_raw(imgs, lm)
    for k in ("I128", "I64", "I32", "u8_128"):
        assert torch.equal(p[k], r[k]), k
    assert sorted(p) == sorted(r)
    boxes = FaceBatcher(gpu, pts_idx=IDX4, check=False).landmark_boxes(d["points"])[1]
    assert torch.equal(boxes, d["boxes"])
    jobs = [(n, PATCH_SIZE[n][1], PATCH_SIZE[n][0], i) for i, n in enumerate(PATCH_NAMES)]
    want = fb._crop(d["u8_128"], jobs, boxes)
    for n in PATCH_NAMES:
        assert torch.equal(p[n], want[n]), n
        assert tuple(p[n].shape) == (3, 3, PATCH_SIZE[n][1], PATCH_SIZE[n][0])
    with pytest.raises(ValueError, match="boxes"):
        fb.from_points(d["u8_128"], d["boxes"].float())
    with pytest.raises(ValueError, match="boxes"):
        fb.from_points(d["u8_128"], d["boxes"][:2])


def test_frontalizer_with_detector(gpu, composed):
    import tpgan_infer
    import tpgan_ops
    from DataAndDataset import FaceBatcher
    d, imgs, fz, det, out = composed["d"], composed["imgs"], composed["fz"], composed["det"], composed["out"]
    fb = FaceBatcher(gpu)
    assert out.dtype == torch.uint8 and tuple(out.shape) == (3, 128, 128, 3)
    with tpgan_ops.deterministic():
        assert torch.equal(out, fz.frontalize_batch(fb.from_points(d["u8_128"], d["boxes"]), None))
        fz.max_batch = det.max_batch = 2  # the same frozen models, two faces then one
        try:
            d2 = det.detect(imgs)
            for k in d:
                assert torch.equal(d2[k], d[k]), k
            assert torch.equal(fz(imgs), out)
        finally:
            fz.max_batch = det.max_batch = 32
        r = fz.evaluate(imgs, None, frontal=imgs)
        assert sorted(r) == ["fake_u8", "psnr", "sse", "ssim"] and torch.equal(r["fake_u8"], out)
        assert torch.equal(fz(imgs, composed["lm"]), tpgan_infer.Frontalizer(fz.G, device=gpu)(imgs, composed["lm"]))
    bare = tpgan_infer.Frontalizer(fz.G, device=gpu, compute_dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="detector"):
        bare(imgs)
    with pytest.raises(ValueError, match="detector"):
        bare.evaluate(imgs, None, frontal=imgs)
    with pytest.raises(ValueError, match="LandmarkDetector"):
        tpgan_infer.Frontalizer(fz.G, device=gpu, detector=object())
    det.device = torch.device("cpu")  # (one GPU here: a detector that says it lives elsewhere)
    try:
        with pytest.raises(ValueError, match="detector is on"):
            tpgan_infer.Frontalizer(fz.G, device=gpu, detector=det)
    finally:
        det.device = fz.device


def test_detect_at_256(gpu, composed, wide_sd):
    import tpgan_infer
    import tpgan_ops
    imgs, d = composed["imgs"], composed["d"]
    det = tpgan_infer.LandmarkDetector(_mnv2(wide_sd), device=gpu, compute_dtype=torch.bfloat16,
                                       confidence_threshold=0.2, detect_hw=(256, 256), on_missing="best")
    with tpgan_ops.deterministic():
        d2 = det.detect(imgs)
        assert torch.equal(d2["u8_128"], d["u8_128"])
        u8 = det._batcher().resize(d["u8_128"], (256, 256))
        with torch.no_grad():
            loc, cls = det._head(u8)
        assert tuple(loc.shape) == (3, 1540, 2)
        want = tpgan_ops.ssd_landmarks(loc, cls, 0.2, torch.full((3, 2), 0.5, device=gpu))
    for got, w in zip((d2["points"], d2["score"], d2["anchor"], d2["boxes"], d2["status"]), want):
        assert torch.equal(got, w)
    unscaled = tpgan_ops.ssd_landmarks(loc, cls, 0.2)[0]
    assert torch.equal(d2["points"], unscaled * 0.5)


def test_detector_checkpoints_and_reloads(gpu, composed, wide_sd, tmp_path):
    import tpgan_infer
    import tpgan_ops
    imgs, d = composed["imgs"], composed["d"]
    bare = str(tmp_path / "detector.pth")
    torch.save(wide_sd, bare)
    os.makedirs(str(tmp_path / "pretrain"))
    other = {k: (v * 0.5 if v.is_floating_point() else v) for k, v in wide_sd.items()}
    torch.save(other, str(tmp_path / "pretrain" / "model_epoch_2.pth"))
    torch.save(wide_sd, str(tmp_path / "pretrain" / "model_epoch_10.pth"))
    keys = ("points", "score", "anchor", "boxes", "status")
    with tpgan_ops.deterministic():
        for path, epoch in ((bare, None), (str(tmp_path / "pretrain"), None), (str(tmp_path / "pretrain"), 10)):
            det = tpgan_infer.LandmarkDetector.from_checkpoint(path, epoch=epoch, device=gpu, compute_dtype=torch.bfloat16,
                                                               confidence_threshold=0.2)
            got = det.detect(imgs)
            for k in keys:
                assert torch.equal(got[k], d[k]), (path, epoch, k)
        # new weights: the folded BatchNorm and the packed images follow
        sd2 = {}
        for i, (k, v) in enumerate(wide_sd.items()):
            ramp = torch.cos(torch.arange(v.numel(), dtype=torch.float32) * 0.37 + i).reshape(v.shape)
            sd2[k] = v * (1.0 + 0.05 * ramp) if v.is_floating_point() else v.clone()
        det.on_missing = "best"
        det.load_state_dict(sd2)
        second = det.detect(imgs)
        fresh = tpgan_infer.LandmarkDetector(_mnv2(sd2), device=gpu, compute_dtype=torch.bfloat16,
                                             confidence_threshold=0.2, on_missing="best").detect(imgs)
    assert not torch.equal(second["score"], d["score"])
    for k in keys:
        assert torch.equal(second[k], fresh[k]), k
    with pytest.raises(ValueError, match="missing"):
        det.load_state_dict({k: v for k, v in sd2.items() if k != next(iter(sd2))})
