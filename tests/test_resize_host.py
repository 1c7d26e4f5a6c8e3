"""CPU: the host side of the LANCZOS resize (tpg_resize_ksize / _coeffs / _workspace / _pack_job,
no device work) against tests/_resize_ref.py, the reference's recorded bytes
(tests/golden/resize_golden.npz) and, where it imports, live Pillow.  Every comparison is exact."""
import ctypes
import math
import os
import struct

import numpy as np
import pytest

import _resize_ref as R
import tpgan_lib as L

PAIRS = [(1, 128), (3, 128), (96, 128), (127, 128), (129, 128), (150, 128), (1024, 128), (4096, 32), (128, 64),
         (64, 32)]


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


@pytest.fixture(scope="module")
def gold():
    return R.load_golden()


def lib_table(lib):
    """(in, out) -> (bounds, k) from tpg_resize_coeffs, in exactly-sized arrays, cached."""
    cache = {}

    def table(in_size, out_size):
        if (in_size, out_size) not in cache:
            ks = lib.tpg_resize_ksize(in_size, out_size)
            assert ks > 0, lib.tpg_last_error()
            bounds = np.full((out_size, 2), -7, np.int32)
            k = np.full((out_size, ks), -7, np.int32)
            assert lib.tpg_resize_coeffs(in_size, out_size, bounds.ctypes.data, k.ctypes.data) == 0, \
                lib.tpg_last_error()
            cache[(in_size, out_size)] = (bounds, k)
        return cache[(in_size, out_size)]

    return table


@pytest.mark.parametrize("pair", PAIRS, ids=["%dto%d" % p for p in PAIRS])
def test_coeffs_match_restatement(lib, pair):
    in_size, out_size = pair
    assert lib.tpg_resize_ksize(in_size, out_size) == 2 * math.ceil(3 * max(in_size / out_size, 1)) + 1
    assert lib.tpg_resize_ksize(in_size, out_size) == R.ksize(in_size, out_size)
    bounds, k = lib_table(lib)(in_size, out_size)
    rb, rk = R.coeffs(in_size, out_size)
    np.testing.assert_array_equal(bounds, rb)
    np.testing.assert_array_equal(k, rk)
    assert lib.tpg_resize_table_ints(in_size, out_size) == bounds.size + k.size
    assert np.abs(k).max() < 2 ** 23  # the kernels' 24-bit multiply-add


def test_fixture_chain_from_library_tables(lib, gold):
    """The numpy integer passes driven by the LIBRARY's tables give every 128 / 64 / 32 image the
    reference's Pillow produced."""
    table = lib_table(lib)
    assert int(gold["n"]) == 8
    for k in range(int(gold["n"])):
        u128 = R.resize(gold["%d:raw" % k], 128, 128, table)
        np.testing.assert_array_equal(u128, gold["%d:u8_128" % k], err_msg="%d 128" % k)
        u64 = R.resize(u128, 64, 64, table)
        np.testing.assert_array_equal(u64, gold["%d:u8_64" % k], err_msg="%d 64" % k)
        np.testing.assert_array_equal(R.resize(u64, 32, 32, table), gold["%d:u8_32" % k], err_msg="%d 32" % k)
    assert (gold["5:u8_128"] == 0).any() and (gold["5:u8_128"] == 255).any()  # the checker clips at both ends


def test_passes_match_live_pillow(lib):
    Image = pytest.importorskip("PIL.Image")
    table = lib_table(lib)
    rng = np.random.default_rng(7)
    for _ in range(20):
        w, h, ow, oh = (int(v) for v in rng.integers(1, 401, 4))
        a = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        ref = np.asarray(Image.fromarray(a).resize((ow, oh), Image.LANCZOS))
        np.testing.assert_array_equal(R.resize(a, oh, ow, table), ref, err_msg=str((w, h, ow, oh)))


def test_bad_sizes_refused(lib):
    buf = np.zeros(1 << 16, np.int32)
    for bad in (0, -1, 4097):
        for a, b in ((bad, 128), (128, bad)):
            assert lib.tpg_resize_ksize(a, b) == 0
            assert b"1..4096" in lib.tpg_last_error()
            assert lib.tpg_resize_coeffs(a, b, buf.ctypes.data, buf.ctypes.data) < 0
            assert b"1..4096" in lib.tpg_last_error()
            assert lib.tpg_resize_table_ints(a, b) == 0
        assert lib.tpg_resize_workspace(bad, 64, 128, 128) < 0
        assert lib.tpg_resize_workspace(64, 64, 128, bad) < 0
        assert b"1..4096" in lib.tpg_last_error()
    assert not buf.any()
    assert lib.tpg_resize_coeffs(64, 32, None, buf.ctypes.data) < 0 and b"NULL" in lib.tpg_last_error()


def test_workspace_and_job_records(lib):
    assert lib.tpg_resize_workspace(480, 640, 128, 128) == 480 * 128 * 3
    assert lib.tpg_resize_workspace(53, 37, 128, 128) == (53 * 128 * 3 + 15) // 16 * 16
    assert lib.tpg_resize_workspace(300, 128, 128, 128) == 0  # pass along W skipped
    assert lib.tpg_resize_workspace(128, 300, 128, 128) == 0  # pass along H skipped
    jb = lib.tpg_resize_job_bytes()
    assert jb == 64
    jobs = (ctypes.c_uint8 * (3 * jb))()
    src = 0x7000000000
    assert lib.tpg_resize_pack_job(jobs, 1, src, 53, 37, 3, 111, 128, 128, 1000, 2000, 4096) == 0
    rec = struct.unpack_from("<Qqqqq6i", bytes(jobs), jb)
    assert rec == (src, 111, 1000, 2000, 4096, 53, 37, 128, 128, R.ksize(37, 128), R.ksize(53, 128))
    assert not any(bytes(jobs)[:jb]) and not any(bytes(jobs)[2 * jb:])
    # a row stride smaller than W*3 bytes, and every other malformed argument, leaves the record alone
    before = bytes(jobs)
    assert lib.tpg_resize_pack_job(jobs, 1, src, 53, 37, 3, 110, 128, 128, 0, 0, 0) < 0
    assert b"row stride" in lib.tpg_last_error()
    assert lib.tpg_resize_pack_job(jobs, 1, src, 53, 37, 4, 148, 128, 128, 0, 0, 0) < 0
    assert b"3 interleaved bands" in lib.tpg_last_error()
    assert lib.tpg_resize_pack_job(jobs, 1, src, 53, 37, 1, 37, 128, 128, 0, 0, 0) < 0
    assert lib.tpg_resize_pack_job(jobs, 1, src, 0, 37, 3, 111, 128, 128, 0, 0, 0) < 0
    assert lib.tpg_resize_pack_job(jobs, 1, src, 53, 4097, 3, 4097 * 3, 128, 128, 0, 0, 0) < 0
    assert lib.tpg_resize_pack_job(jobs, 1, src, 53, 37, 3, 111, 128, 128, -1, 0, 0) < 0
    assert lib.tpg_resize_pack_job(jobs, 1, src, 53, 37, 3, 111, 128, 128, 0, 0, 8) < 0
    assert b"multiple of 16" in lib.tpg_last_error()
    assert lib.tpg_resize_pack_job(jobs, -1, src, 53, 37, 3, 111, 128, 128, 0, 0, 0) < 0
    assert lib.tpg_resize_pack_job(jobs, 1, None, 53, 37, 3, 111, 128, 128, 0, 0, 0) < 0
    assert lib.tpg_resize_pack_job(None, 1, src, 53, 37, 3, 111, 128, 128, 0, 0, 0) < 0
    assert bytes(jobs) == before
    # the launcher refuses before any device work
    assert lib.tpg_resize_u8(1, None, None, 128, 128, None, None, None) < 0 and b"NULL" in lib.tpg_last_error()
    assert lib.tpg_resize_u8(-1, jobs, jobs, 128, 128, jobs, None, None) < 0
    assert lib.tpg_resize_u8(1, jobs, jobs, 0, 128, jobs, None, None) < 0
    assert lib.tpg_resize_u8(0, None, None, 128, 128, None, None, None) == 0
