"""CPU: the landmark front end's host side.  The numpy restatements the GPU tests compare against
(tests/_landmark_ref.py) reproduce the reference's own decoder and accuracy measure
(tests/golden/landmark_golden.npz, made by tests/golden/make_golden_landmarks.py); the three entry
points are declared, bound and refuse malformed calls before any device work; a checkpoint with
a missing key is refused before a detector is built."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import _landmark_ref as R
import tpgan_lib as L
from _cases import golden

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("tpg_ssd_landmarks", "tpg_landmark_accuracy", "tpg_u8_to_unit")


@pytest.fixture(scope="module")
def G():
    return golden("landmark_golden.npz")


def _cases(G):
    return range(int(G["ncases"]))


def test_golden_covers_the_band_edges(G):
    """What the fixture was built for: every edge of the bands, one float32 step past an edge, an
    exact hit and a miss beyond the last band; 12 to 40 anchors; five decoded classes per case."""
    dist = np.concatenate([G["%d:dist" % k] for k in _cases(G)])
    for edge in (0, 5, 10, 18, 30, 45):
        assert (dist == edge).any(), edge
    for edge in (5, 10, 18, 30, 45):
        assert (dist == float(np.nextafter(np.float32(edge), np.float32(np.inf)))).any(), edge
    assert (dist > 46).any()
    ns = [G["%d:cls" % k].shape[1] for k in _cases(G)]
    assert min(ns) >= 12 and max(ns) <= 40 and len(ns) >= 12
    for k in _cases(G):
        assert G["%d:dec_class" % k].tolist() == [0, 1, 2, 3, 4]
    assert float(G["0:acc"]) == 0.4375  # distances (0, 3, 12, 40): the exact hit scores 0


def test_decode_restatement_reproduces_the_reference(G):
    for k in _cases(G):
        loc, cls = G["%d:loc" % k], G["%d:cls" % k]
        points, score, anchor, status = R.decode_top1(loc, cls, 0.5)
        assert anchor[0].tolist() == G["%d:planted" % k][:4].tolist(), k
        assert np.array_equal(points[0], G["%d:dec_point" % k][:4]), k
        assert np.abs(score[0] - G["%d:dec_score" % k][:4]).max() <= 1e-6, k
        assert status.tolist() == [0], k


def test_accuracy_restatement_reproduces_the_reference(G):
    for k in _cases(G):
        got = R.accuracy(G["%d:dec_point" % k][None, :4], G["%d:truth" % k])
        assert got.dtype == np.float32 and got[0] == G["%d:acc" % k], (k, got, G["%d:acc" % k])
    # the decode feeds it: points of the restated decode, the same values
    for k in _cases(G):
        pts = R.decode_top1(G["%d:loc" % k], G["%d:cls" % k], 0.5)[0]
        assert R.accuracy(pts, G["%d:truth" % k])[0] == G["%d:acc" % k], k


def test_accuracy_restatement_status_and_nan():
    truth = np.zeros((1, 8), np.float32)
    pred = np.array([[3, 0, 7, 0, 12, 0, np.nan, 0]], np.float32)
    assert R.accuracy(pred, truth)[0] == np.float32((np.float32(1.0) + np.float32(0.9) + np.float32(0.65)) / 4)
    assert R.accuracy(pred, truth, status=np.array([1 | 4]))[0] == np.float32(0.9) / np.float32(4)


def test_boxes_restatement_is_process():
    """The restated boxes against the product's host process() (the reference's arithmetic, pinned
    by data_golden.npz) on [le, re, nose, mouth, mouth]."""
    import DataAndDataset as DD

    class Rec:
        def crop(self, box):
            return box

    rng = np.random.RandomState(5)
    pts = ((rng.rand(6, 4, 2) - 0.2) * 150).astype(np.float32)
    pts[0, 0] = [17.0, -3.0]  # exactly on an integer, and negative
    got = R.boxes(pts)
    for b in range(pts.shape[0]):
        lm5 = np.concatenate([pts[b], pts[b, 3:4]]).astype(np.float32)
        want = DD.process(Rec(), lm5)
        assert [list(want[n]) for n in DD.PATCH_NAMES] == got[b].tolist()
    bad = np.array([[[np.inf, 2.5], [np.nan, -np.inf], [1, 1], [2, 2]]], np.float32)
    assert R.boxes(bad)[0, 0].tolist() == [-19, -17, 21, 23] and R.boxes(bad)[0, 1].tolist() == [-19, -19, 21, 21]


def _header_decl(name):
    src = open(os.path.join(REPO, "include", "tpgan.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    m = re.search(r"int32_t\s+%s\s*\(([^;]*)\)\s*;" % name, src)
    return None if m is None else [a.strip() for a in m.group(1).split(",")]


def test_header_declares_and_binding_binds():
    for name in ENTRIES:
        args = _header_decl(name)
        assert args is not None, "%s is not declared in include/tpgan.h" % name
        assert name in L.EXPORTS, "%s is not bound in tpgan_lib.EXPORTS" % name
        res, argtypes = L.EXPORTS[name]
        assert res is ctypes.c_int32 and len(argtypes) == len(args), (name, args)
        assert args[-1].startswith("tpg_stream_t")
    assert L.LM_MAX_BANDS == 8


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(L.LIB_PATH):
        pytest.skip("libtpgan_hip.so not built")
    lib = ctypes.CDLL(L.LIB_PATH)
    for name in ENTRIES + ("tpg_last_error",):
        f = getattr(lib, name)
        f.restype, f.argtypes = L.EXPORTS[name]
    return lib


def _ssd(lib, B=2, n=394, C=5, loc=0x10000, cls=0x10000, wh=True, outs=(0x20000,) * 5, scale=None):
    whv = (ctypes.c_int32 * 8)(40, 40, 40, 40, 40, 32, 48, 32) if wh else None
    return lib.tpg_ssd_landmarks(B, n, C, loc, cls, 0.5, scale, whv, *outs, None)


def _acc(lib, B=4, nb=5, ptr=(0x10000, 0x10000, 0x10000), thr=True, wgt=True, thresholds=(5, 10, 18, 30, 45)):
    t = (ctypes.c_float * 8)(*thresholds) if thr else None
    w = (ctypes.c_float * 8)(1.0, 0.9, 0.65, 0.35, 0.1) if wgt else None
    return lib.tpg_landmark_accuracy(B, ptr[0], ptr[1], None, nb, t, w, ptr[2], None)


def _unit(lib, n=2, c=3, h=128, w=128, img=0x10000, strides=True, data=0x20000, dtype=L.TPG_BF16):
    out = L.TpgTensor()
    out.data, out.dtype = data, dtype
    for i, s in enumerate((128 * 128 * 8, 1, 128 * 8, 8)):
        out.stride[i] = s
    st = (ctypes.c_int64 * 4)(128 * 128 * 3, 1, 128 * 3, 3) if strides else None
    return lib.tpg_u8_to_unit(n, c, h, w, img, st, out, None)


def test_entry_points_refuse_null_pointers(lib):
    """-10 with the call's own name, and no device work: this runs without a GPU."""
    calls = [("ssd_landmarks", lambda: _ssd(lib, loc=None)), ("ssd_landmarks", lambda: _ssd(lib, cls=None)),
             ("ssd_landmarks", lambda: _ssd(lib, wh=False))]
    for i in range(5):
        outs = tuple(None if j == i else 0x20000 for j in range(5))
        calls.append(("ssd_landmarks", lambda outs=outs: _ssd(lib, outs=outs)))
    for i in range(3):
        ptr = tuple(None if j == i else 0x10000 for j in range(3))
        calls.append(("landmark_accuracy", lambda ptr=ptr: _acc(lib, ptr=ptr)))
    calls += [("landmark_accuracy", lambda: _acc(lib, thr=False)), ("landmark_accuracy", lambda: _acc(lib, wgt=False)),
              ("u8_to_unit", lambda: _unit(lib, img=None)), ("u8_to_unit", lambda: _unit(lib, strides=False)),
              ("u8_to_unit", lambda: _unit(lib, data=None))]
    for name, call in calls:
        assert call() == -10, name
        assert name in lib.tpg_last_error().decode(), (name, lib.tpg_last_error())


def test_entry_points_refuse_bad_sizes(lib):
    calls = [("ssd_landmarks", lambda: _ssd(lib, n=0)), ("ssd_landmarks", lambda: _ssd(lib, n=4097)),
             ("ssd_landmarks", lambda: _ssd(lib, C=4)), ("ssd_landmarks", lambda: _ssd(lib, B=0)),
             ("landmark_accuracy", lambda: _acc(lib, nb=0)), ("landmark_accuracy", lambda: _acc(lib, nb=9)),
             ("landmark_accuracy", lambda: _acc(lib, B=0)),
             ("landmark_accuracy", lambda: _acc(lib, thresholds=(5, 10, 9, 30, 45))),
             ("u8_to_unit", lambda: _unit(lib, n=0)), ("u8_to_unit", lambda: _unit(lib, c=0)),
             ("u8_to_unit", lambda: _unit(lib, h=-1)), ("u8_to_unit", lambda: _unit(lib, n=32768, h=256, w=256))]
    for name, call in calls:
        assert call() == -2, name
        assert name in lib.tpg_last_error().decode(), (name, lib.tpg_last_error())
    assert _unit(lib, dtype=7) == -11


def test_ops_refuse_host_tensors_without_a_device():
    """tpgan_ops validates before it loads the library: ValueError, not a device error."""
    import tpgan_ops
    loc, cls = torch.zeros(1, 12, 2), torch.zeros(1, 12, 5)
    with pytest.raises(ValueError, match="device tensor"):
        tpgan_ops.ssd_landmarks(loc, cls, 0.5)
    with pytest.raises(ValueError, match="float32"):
        tpgan_ops.ssd_landmarks(loc.double(), cls, 0.5)
    with pytest.raises(ValueError, match="device tensor"):
        tpgan_ops.u8_to_unit(torch.zeros(1, 4, 4, 3, dtype=torch.uint8))
    with pytest.raises(ValueError, match="uint8"):
        tpgan_ops.u8_to_unit(torch.zeros(1, 4, 4, 3))
    with pytest.raises(ValueError, match="device tensor"):
        tpgan_ops.landmark_accuracy(torch.zeros(2, 4, 2), torch.zeros(2, 4, 2))
    with pytest.raises(ValueError, match=r"\[B, 4, 2\]"):
        tpgan_ops.landmark_accuracy(torch.zeros(2, 5, 2), torch.zeros(2, 4, 2))


def test_from_checkpoint_rejects_a_missing_key_before_building(tmp_path, monkeypatch):
    import MobileNetV2 as MN
    import tpgan_infer
    built = []
    monkeypatch.setattr(tpgan_infer.LandmarkDetector, "__init__", lambda self, *a, **k: built.append(1))
    sd = MN.MobileNetV2().state_dict()
    first = next(iter(sd))
    path = str(tmp_path / "model_epoch_2.pth")
    torch.save({k: v for k, v in sd.items() if k != first}, path)
    with pytest.raises(ValueError, match="missing"):
        tpgan_infer.LandmarkDetector.from_checkpoint(path)
    with pytest.raises(ValueError, match="missing"):
        tpgan_infer.LandmarkDetector.from_checkpoint(str(tmp_path))  # the directory: its largest epoch
    wrong = dict(sd)
    wrong[first] = torch.zeros(3)
    torch.save(wrong, str(tmp_path / "model_epoch_10.pth"))
    with pytest.raises(ValueError, match="shape"):
        tpgan_infer.LandmarkDetector.from_checkpoint(str(tmp_path))  # epoch 10 > 2
    os.makedirs(str(tmp_path / "empty"))
    with pytest.raises(ValueError, match="no model_epoch"):
        tpgan_infer.LandmarkDetector.from_checkpoint(str(tmp_path / "empty"))
    assert not built
    torch.save(sd, str(tmp_path / "model_epoch_11.pth"))
    tpgan_infer.LandmarkDetector.from_checkpoint(str(tmp_path))  # a whole state_dict reaches the constructor
    assert built == [1]
