"""CPU: the numpy restatement of the identity scoring kernels (tests/_identity_ref.py) on a case
worked by hand, the C-ABI's argument validation (negative code, message, no device work) and the
top-k workspace query."""
import ctypes
import os

import numpy as np
import pytest
import torch

import _identity_ref as R
import tpgan_lib as L


def test_reference_on_a_hand_written_case():
    """3 probes x 4 gallery rows, D = 2, k = 5 > G.  Gallery rows 0 and 2 point the same way (an
    exact tie, the lower index first), probe 1 is orthogonal to three of them (a three-way tie at 0,
    one of them -0.0); probe 2 is probe 0 with gallery row 0 skipped."""
    gallery = np.array([[3.0, 0.0], [0.0, 2.0], [0.5, 0.0], [-4.0, 0.0]])
    probes = np.array([[2.0, 0.0], [0.0, 7.0], [2.0, 0.0]])
    gu, gn = R.normalize(gallery)
    pu, pn = R.normalize(probes)
    np.testing.assert_array_equal(gn, [3.0, 2.0, 0.5, 4.0])
    np.testing.assert_array_equal(gu, [[1, 0], [0, 1], [1, 0], [-1, 0]])
    sim = R.similarity(pu, gu)
    np.testing.assert_array_equal(sim, [[1, 0, 1, -1], [0, 1, 0, 0], [1, 0, 1, -1]])
    idx, score = R.topk(sim, 5, skip=[-1, -1, 0])
    ninf = -np.inf
    np.testing.assert_array_equal(idx, [[0, 2, 1, 3, -1], [1, 0, 2, 3, -1], [2, 1, 3, -1, -1]])
    np.testing.assert_array_equal(score, [[1, 1, 0, -1, ninf], [1, 0, 0, 0, ninf], [1, 0, -1, ninf, ninf]])
    idx1, score1 = R.topk(sim, 1)
    np.testing.assert_array_equal(idx1, [[0], [1], [0]])
    assert idx.dtype == np.int32
    # the bound: (3 D + 16) u sum |p g| = 22 u where the rows are parallel, 0 where orthogonal
    b = R.bound(pu, gu)
    np.testing.assert_allclose(b, 22 * 2.0 ** -24 * np.abs(sim), rtol=1e-15)
    np.testing.assert_array_equal(R.cosine_pairs(probes, gallery[:3]), [1, 1, 1])
    zu, zn = R.normalize(np.zeros((1, 3)))
    assert zn[0] == 0 and not zu.any()


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


def _rows(dtype=L.TPG_F32, data=0x1000):
    t = L.TpgTensor()
    t.data = data  # never dereferenced: every call below fails validation first
    t.dtype = dtype
    t.stride[0], t.stride[1] = 512, 1
    return t


P16 = ctypes.c_void_p(0x1000)  # 16-byte aligned, never dereferenced


def _rejected(lib, rc, word):
    msg = lib.tpg_last_error()
    assert rc < 0 and word in msg, (rc, msg)


def test_capi_l2_normalize_validation(lib):
    call = lambda **k: lib.tpg_l2_normalize(k.get("n", 4), k.get("d", 515), k.get("x", _rows()), k.get("out", P16),
                                            k.get("dpad", 516), k.get("norm", P16), k.get("status", P16), None)
    _rejected(lib, call(x=_rows(data=None)), b"NULL")
    _rejected(lib, call(out=None), b"NULL")
    _rejected(lib, call(status=None), b"NULL")
    for d in (0, -1, 4097):
        _rejected(lib, call(d=d, dpad=max(d, 0)), b"1..4096")
    for dpad in (515, 512, 520):
        _rejected(lib, call(dpad=dpad), b"dpad")
    _rejected(lib, call(x=_rows(dtype=9)), b"dtype")
    _rejected(lib, call(n=-1), b"n must")


def test_capi_cosine_pairs_validation(lib):
    call = lambda **k: lib.tpg_cosine_pairs(k.get("n", 4), k.get("d", 512), k.get("a", _rows()), k.get("b", _rows()),
                                            k.get("cos", P16), k.get("status", P16), None)
    _rejected(lib, call(a=_rows(data=None)), b"NULL")
    _rejected(lib, call(b=_rows(data=None)), b"NULL")
    _rejected(lib, call(cos=None), b"NULL")
    _rejected(lib, call(status=None), b"NULL")
    for d in (0, 4097):
        _rejected(lib, call(d=d), b"1..4096")
    _rejected(lib, call(b=_rows(dtype=3)), b"dtype")


def test_capi_cosine_topk_validation(lib):
    def call(**k):
        return lib.tpg_cosine_topk(k.get("P", 4), k.get("G", 100), k.get("d", 515), k.get("dpad", 516),
                                   k.get("probes", P16), k.get("gallery", P16), k.get("k", 5), k.get("skip", None),
                                   k.get("gchunk", 0), k.get("idx", P16), k.get("score", P16), k.get("ws", P16),
                                   k.get("ws_bytes", 1 << 20), None)
    for name in ("probes", "gallery", "idx", "score", "ws"):
        _rejected(lib, call(**{name: None}), b"NULL")
    for k in (0, 9, -3):
        _rejected(lib, call(k=k), b"1..8")
        assert lib.tpg_cosine_topk_workspace(4, 100, k, 0) < 0 and b"1..8" in lib.tpg_last_error()
    for d in (0, 4097):
        _rejected(lib, call(d=d), b"1..4096")
    for dpad in (515, 520):
        _rejected(lib, call(dpad=dpad), b"dpad")
    for gchunk in (1, 8, 15, -1):
        _rejected(lib, call(gchunk=gchunk), b"gchunk")
        assert lib.tpg_cosine_topk_workspace(4, 100, 5, gchunk) < 0 and b"gchunk" in lib.tpg_last_error()
    need = lib.tpg_cosine_topk_workspace(4, 100, 5, 16)
    _rejected(lib, call(gchunk=16, ws_bytes=need - 1), b"workspace")
    _rejected(lib, call(ws_bytes=0), b"workspace")
    _rejected(lib, call(P=(1 << 24) + 1), b"2^24")
    _rejected(lib, call(G=-1), b"2^24")
    _rejected(lib, call(probes=ctypes.c_void_p(0x1004)), b"aligned")


def test_cosine_topk_workspace_grows(lib):
    ws = lib.tpg_cosine_topk_workspace
    assert ws(1, 1, 1, 0) > 0 and ws(0, 0, 1, 0) > 0
    assert ws(4096, 16384, 5, 0) > 0 and ws(1 << 24, 1 << 24, 8, 0) > 0
    # one k-entry list of (score, index) per probe and chunk
    assert ws(4, 100, 8, 16) == 4 * 7 * 8 * 8
    assert ws(5, 100, 8, 16) > ws(4, 100, 8, 16)            # with P
    assert ws(4, 100, 8, 16) > ws(4, 100, 8, 48) > ws(4, 100, 8, 128)  # with the number of chunks: 7, 3, 1
    assert ws(4, 113, 8, 16) > ws(4, 112, 8, 16)            # a ragged last chunk is a chunk
    assert ws(4, 100, 8, 16) > ws(4, 100, 5, 16)
    assert ws(1 << 24, 1 << 24, 1, 16) < 0 and b"blocks" in lib.tpg_last_error()


def test_ops_reject_cpu_and_wrong_dtype():
    import tpgan_ops
    x = torch.zeros(3, 8)
    with pytest.raises(ValueError, match="device tensor"):
        tpgan_ops.l2_normalize(x)
    with pytest.raises(ValueError, match="2-D"):
        tpgan_ops.l2_normalize(torch.zeros(8))
    with pytest.raises(ValueError, match="float32, bfloat16 or float16"):
        tpgan_ops.l2_normalize(x.double())
    with pytest.raises(ValueError, match="1..4096"):
        tpgan_ops.l2_normalize(torch.zeros(2, 4097))
    with pytest.raises(ValueError, match="device tensor"):
        tpgan_ops.cosine_pairs(x, x)
    with pytest.raises(ValueError, match="float32, bfloat16 or float16"):
        tpgan_ops.cosine_pairs(x.long(), x.long())
    with pytest.raises(ValueError, match="device tensor"):
        tpgan_ops.cosine_topk(x, x)
    with pytest.raises(ValueError, match="float32"):
        tpgan_ops.cosine_topk(x.half(), x.half())


def test_identity_scorer_rejects_bad_arguments():
    import tpgan_infer
    with pytest.raises(ValueError, match="compute_dtype"):
        tpgan_infer.IdentityScorer(torch.nn.Identity(), device="cpu", compute_dtype=torch.float64)
    with pytest.raises(ValueError, match="FeatureExtractModel"):
        tpgan_infer.IdentityScorer(torch.nn.Identity(), device="cpu")
    res = {"idx": torch.tensor([[0, 1], [2, -1], [1, 0]], dtype=torch.int32),
           "label": torch.tensor([[7, 8], [9, -1], [5, 7]])}
    np.testing.assert_array_equal(tpgan_infer.IdentityScorer.cmc([7, 7, 7], res).numpy(), [1 / 3, 2 / 3])
    np.testing.assert_array_equal(tpgan_infer.IdentityScorer.cmc([-1, -1, -1], res).numpy(), [0.0, 0.0])
