"""CPU: the host side of the face alignment -- the integer restatement of the warp against its three
known answers, tpg_warp_pack_job's record layout, the entry points' argument checks (no device
work), FaceAligner's template checks and template_from_landmarks.  Every comparison is exact."""
import ctypes
import os
import struct

import numpy as np
import pytest

import _align_ref as A
import tpgan_lib as L

Q = 65536


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


def _photo(h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


SIZES = [(5, 7), (7, 5), (12, 9), (20, 20)]


@pytest.mark.parametrize("hw", SIZES, ids=["%dx%d" % s for s in SIZES])
def test_identity_copies_top_left(hw):
    h, w = hw
    a = _photo(h, w, 1)
    out, st = A.warp_int(a, (Q, 0, 0, 0, Q, 0), h, w)
    np.testing.assert_array_equal(out, a)
    assert st == 0 and A.supersample((Q, 0, 0, 0, Q, 0)) == (1, False)
    out, _ = A.warp_int(a, (Q, 0, 0, 0, Q, 0), h - 2, w - 3)
    np.testing.assert_array_equal(out, a[:h - 2, :w - 3])
    # past the photo: the last row and column, replicated
    out, _ = A.warp_int(a, (Q, 0, 0, 0, Q, 0), h + 2, w + 1)
    np.testing.assert_array_equal(out, np.pad(a, ((0, 2), (0, 1), (0, 0)), mode="edge"))


@pytest.mark.parametrize("hw", [(6, 8), (10, 14), (20, 20)], ids=lambda s: "%dx%d" % s)
def test_scale_two_is_the_box_average(hw):
    h, w = hw
    a = _photo(h, w, 2)
    out, st = A.warp_int(a, (2 * Q, 0, 0, 0, 2 * Q, 0), h // 2, w // 2)
    box = a.astype(np.int64).reshape(h // 2, 2, w // 2, 2, 3).sum((1, 3))
    np.testing.assert_array_equal(out, (box + 2) // 4)  # round half up
    assert st == 0 and A.supersample((2 * Q, 0, 0, 0, 2 * Q, 0)) == (2, False)


@pytest.mark.parametrize("hw", SIZES, ids=["%dx%d" % s for s in SIZES])
def test_quarter_turn(hw):
    h, w = hw
    a = _photo(h, w, 3)
    out, st = A.warp_int(a, (0, -Q, w * Q, Q, 0, 0), w, h)
    # out[oy, ox] = a[ox, w - 1 - oy]
    np.testing.assert_array_equal(out, np.transpose(a[:, ::-1], (1, 0, 2)))
    assert st == 0


def test_supersample_thresholds():
    assert A.supersample((Q, 0, 0, 0, Q, 0)) == (1, False)
    assert A.supersample((Q + 1, 0, 0, 0, Q, 0)) == (2, False)
    assert A.supersample((0, 16 * Q, 0, 16 * Q, 0, 0)) == (16, False)
    assert A.supersample((0, 16 * Q, 0, 16 * Q + 1, 0, 0)) == (16, True)
    assert A.supersample((-2 ** 31, 0, 0, -2 ** 31, 0, 0)) == (16, True)  # d = 2^63
    # a rotation's columns have the same length: n follows the scale, not the angle
    c, s = int(round(3 * Q * np.cos(0.5))), int(round(3 * Q * np.sin(0.5)))
    assert A.supersample((c, -s, 0, s, c, 0))[0] in (3, 4)
    a = _photo(9, 9, 4)
    assert A.warp_int(a, (40 * Q, 0, 0, 0, 40 * Q, 0), 4, 4)[1] == 8


def test_warp_job_record(lib):
    jb = lib.tpg_warp_job_bytes()
    assert jb == 32
    jobs = (ctypes.c_uint8 * (3 * jb))()
    src = 0x7000000000
    assert lib.tpg_warp_pack_job(jobs, 1, src, 53, 37, 3, 120, 128, 96) == 0
    # the header's layout: 0 src, 8 row stride, 16 H, 20 W, 24 out_h, 28 out_w
    assert struct.unpack_from("<Qq4i", bytes(jobs), jb) == (src, 120, 53, 37, 128, 96)
    assert not any(bytes(jobs)[:jb]) and not any(bytes(jobs)[2 * jb:])
    before = bytes(jobs)
    assert lib.tpg_warp_pack_job(jobs, 1, src, 53, 37, 3, 110, 128, 128) < 0
    assert b"row stride" in lib.tpg_last_error()
    assert lib.tpg_warp_pack_job(jobs, 1, src, 53, 37, 4, 148, 128, 128) < 0
    assert b"3 interleaved bands" in lib.tpg_last_error()
    for h, w, oh, ow in ((0, 37, 128, 128), (53, 4097, 128, 128), (53, 37, 0, 128), (53, 37, 128, 4097)):
        assert lib.tpg_warp_pack_job(jobs, 1, src, h, w, 3, 4097 * 3, oh, ow) < 0
        assert b"1..4096" in lib.tpg_last_error()
    assert lib.tpg_warp_pack_job(jobs, -1, src, 53, 37, 3, 111, 128, 128) < 0
    assert lib.tpg_warp_pack_job(jobs, 1, None, 53, 37, 3, 111, 128, 128) < 0 and b"NULL" in lib.tpg_last_error()
    assert lib.tpg_warp_pack_job(None, 1, src, 53, 37, 3, 111, 128, 128) < 0
    assert bytes(jobs) == before
    assert lib.tpg_warp_pack_job(jobs, 0, src, 4096, 4096, 3, 4096 * 3, 1, 1) == 0


def test_entry_points_refuse_before_device_work(lib):
    """No GPU is needed: every refusal happens before a launch.  The pointers handed in are host
    memory or fake addresses and are never dereferenced on the device."""
    buf = (ctypes.c_uint8 * 256)()
    p = ctypes.addressof(buf)
    tmpl = (ctypes.c_float * 16)(*[float(v) for v in (30, 40, 90, 40, 60, 70, 60, 100, 0, 0, 1, 1, 2, 2, 3, 3)])
    fit = lib.tpg_similarity_fit
    assert fit(1, 4, None, tmpl, None, p, p, p, None) < 0 and b"NULL" in lib.tpg_last_error()
    assert fit(1, 4, p, None, None, p, p, p, None) < 0 and b"NULL" in lib.tpg_last_error()
    assert fit(1, 4, p, tmpl, None, None, p, p, None) < 0
    assert fit(1, 4, p, tmpl, None, p, None, p, None) < 0
    assert fit(1, 4, p, tmpl, None, p, p, None, None) < 0
    for k in (-1, 0, 1, 9):
        assert fit(1, k, p, tmpl, None, p, p, p, None) < 0 and b"2..8" in lib.tpg_last_error()
    assert fit(-1, 4, p, tmpl, None, p, p, p, None) < 0
    assert fit(0, 4, None, None, None, None, None, None, None) == 0
    for bad in (float("nan"), float("inf"), float("-inf")):
        t = (ctypes.c_float * 8)(30, 40, 90, bad, 60, 70, 60, 100)
        assert fit(1, 4, p, t, None, p, p, p, None) < 0 and b"not finite" in lib.tpg_last_error()
    same = (ctypes.c_float * 8)(5, 6, 5, 6, 5, 6, 5, 6)
    assert fit(1, 4, p, same, None, p, p, p, None) < 0 and b"coincide" in lib.tpg_last_error()
    huge = (ctypes.c_float * 4)(-3e38, 0, 3e38, 0)  # S overflows float32
    assert fit(1, 2, p, huge, None, p, p, p, None) < 0 and b"coincide" in lib.tpg_last_error()
    assert not any(bytes(buf))
    warp = lib.tpg_affine_warp_u8
    assert warp(1, None, p, 128, 128, p, p, None) < 0 and b"NULL" in lib.tpg_last_error()
    assert warp(1, p, None, 128, 128, p, p, None) < 0
    assert warp(1, p, p, 128, 128, None, p, None) < 0
    assert warp(1, p, p, 128, 128, p, None, None) < 0
    for oh, ow in ((0, 128), (128, 0), (4097, 128), (128, 4097)):
        assert warp(1, p, p, oh, ow, p, p, None) < 0 and b"1..4096" in lib.tpg_last_error()
    assert warp(-1, p, p, 128, 128, p, p, None) < 0
    assert warp(65536, p, p, 128, 128, p, p, None) < 0 and b"65535" in lib.tpg_last_error()
    assert warp(0, None, None, 128, 128, None, None, None) == 0
    assert not any(bytes(buf))


def test_face_aligner_rejects_bad_templates():
    import tpgan_infer as I
    good = [[40.0, 50.0], [88.0, 50.0], [64.0, 75.0], [64.0, 98.0]]
    for bad in (float("nan"), float("inf")):
        t = [list(r) for r in good]
        t[2][1] = bad
        with pytest.raises(ValueError, match="NaN or infinite"):
            I.FaceAligner(t)
    with pytest.raises(ValueError, match="coincide"):
        I.FaceAligner([[64.0, 64.0]] * 4)
    with pytest.raises(ValueError, match=r"\[4, 2\]"):
        I.FaceAligner(good[:3])
    with pytest.raises(ValueError, match=r"\[4, 2\]"):
        I.FaceAligner(np.zeros((4, 3), np.float32))
    with pytest.raises(ValueError, match="out_hw"):
        I.FaceAligner(good, out_hw=(0, 128))
    al = I.FaceAligner(good, device="cpu")  # (construction alone touches no device)
    assert al.template.dtype == np.float32 and al.template.tolist() == good and al.out_hw == (128, 128)


def test_template_from_landmarks():
    import tpgan_infer as I
    from DataAndDataset import FIVE_PTS_IDX_REPAIRED
    rng = np.random.default_rng(11)
    lm = rng.uniform(5, 250, (3, 68, 2)).astype(np.float32)
    lm[0] = np.arange(136, dtype=np.float32).reshape(68, 2)  # a face whose means are exact
    scale = np.array([[0.5, 0.25], [1.0, 2.0], [0.75, 0.5]], np.float32)
    for sc in (None, scale):
        centres = np.empty((3, 4, 2), np.float32)
        for f in range(3):
            five = []
            for lo, hi in FIVE_PTS_IDX_REPAIRED:
                acc = np.zeros(2, np.float32)
                for i in range(lo, hi + 1):
                    acc = acc + lm[f, i]
                pt = acc / np.float32(hi - lo + 1)
                five.append(pt * sc[f] if sc is not None else pt)
            centres[f, :3] = five[:3]
            centres[f, 3] = (five[3] + five[4]) / np.float32(2)
        want = centres.astype(np.float64).mean(0).astype(np.float32)
        got = I.FaceAligner.template_from_landmarks(lm, sc)
        assert isinstance(got, np.ndarray) and got.dtype == np.float32 and got.shape == (4, 2)
        np.testing.assert_array_equal(got, want)
    # face 0 by hand: landmark i is (2i, 2i + 1)
    one = I.FaceAligner.template_from_landmarks(lm[:1])
    np.testing.assert_array_equal(one, np.array([[77, 78], [89, 90], [62, 63], [102, 103]], np.float32))
    import torch
    np.testing.assert_array_equal(I.FaceAligner.template_from_landmarks(torch.from_numpy(lm), torch.from_numpy(scale)),
                                  got)
    lm[1, 30, 0] = np.nan
    with pytest.raises(ValueError, match=r"face\(s\) \[1\]"):
        I.FaceAligner.template_from_landmarks(lm)
    with pytest.raises(ValueError, match="lm68"):
        I.FaceAligner.template_from_landmarks(lm[0])
