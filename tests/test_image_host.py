"""CPU: the numpy restatement of the inference image path (tests/_image_ref.py) and what it
records about the kernel's arithmetic, the C-ABI's argument validation (no device work), and
Frontalizer.from_checkpoint's state_dict check."""
import ctypes
import os

import numpy as np
import pytest
import torch

import _image_ref as R
import tpgan_lib as L


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16], ids=["f32", "bf16", "f16"])
def test_denorm_inverts_normalize_for_every_byte(dtype):
    u = np.arange(256, dtype=np.uint8)
    x = torch.from_numpy(R.normalize(u)).to(dtype).float().numpy()  # x as a tensor of `dtype` holds it
    np.testing.assert_array_equal(R.denorm_u8(x), u)


def test_denorm_rule_edges():
    x = np.array([np.nan, np.inf, -np.inf, 3.0, -3.0, -1.0, 1.0, 0.0], np.float32)
    np.testing.assert_array_equal(R.denorm_u8(x), [0, 255, 0, 255, 0, 0, 255, 128])


@pytest.fixture(scope="module")
def ssim_table():
    """case -> float64 reference and the error of each candidate form against it."""
    out = {}
    for name, (a, b) in R.metric_cases().items():
        ref = R.ssim(a, b, np.float64, "centred")
        out[name] = {"ref": ref,
                     "raw_f32": abs(R.ssim(a, b, np.float32, "raw") - ref),
                     "centred_f32": abs(R.ssim(a, b, np.float32, "centred") - ref),
                     "kernel": abs(float(np.float32(R.ssim(a, b, np.float64, "raw"))) - ref)}
    return out


def test_ssim_form_chosen_for_the_kernel(ssim_table):
    """Why tpg_image_metrics_u8 accumulates its five raw moments in float64: in float32 the
    raw-moment variance cancels on a flat bright region and misses the tests' 1e-5 bound, while
    the float64 raw-moment form rounded to a float (the kernel's) holds it on every case."""
    for name, r in ssim_table.items():
        print("%-18s ref %.9f  raw f32 %.2e  centred f32 %.2e  raw f64 -> f32 (kernel) %.2e"
              % (name, r["ref"], r["raw_f32"], r["centred_f32"], r["kernel"]))
    assert ssim_table["flat_bright"]["raw_f32"] > 1e-5
    for name, r in ssim_table.items():
        assert r["kernel"] <= 1e-5, (name, r)


def test_ssim_reference_sanity(ssim_table):
    assert ssim_table["identical_23x17"]["ref"] == 1.0
    assert ssim_table["noise"]["ref"] < 0.05
    assert 0.3 < ssim_table["smooth"]["ref"] < 1.0
    a, b = R.metric_cases()["one_window_11x11"]
    # one window: the map is a single value per channel, computed here from scratch
    w2 = np.outer(R.gauss(), R.gauss())
    vals = []
    for c in range(3):
        x, y = a[..., c].astype(np.float64), b[..., c].astype(np.float64)
        mx, my = (w2 * x).sum(), (w2 * y).sum()
        vx, vy, cxy = (w2 * (x - mx) ** 2).sum(), (w2 * (y - my) ** 2).sum(), (w2 * (x - mx) * (y - my)).sum()
        vals.append((2 * mx * my + R.C1) * (2 * cxy + R.C2) / ((mx * mx + my * my + R.C1) * (vx + vy + R.C2)))
    assert abs(np.mean(vals) - ssim_table["one_window_11x11"]["ref"]) < 1e-12


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


def _fake_tensor(dtype=L.TPG_F32):
    t = L.TpgTensor()
    t.data = 0x1000  # never dereferenced: every call below fails validation first
    t.dtype = dtype
    for i, s in enumerate((3 * 8 * 8, 8 * 8, 8, 1)):
        t.stride[i] = s
    return t


def test_capi_denorm_validation(lib):
    p = ctypes.c_void_p(0x1000)
    rc = lib.tpg_denorm_u8(2, 3, 8, 8, L.TpgTensor(), p, None)
    assert rc < 0 and b"NULL" in lib.tpg_last_error()
    rc = lib.tpg_denorm_u8(2, 3, 8, 8, _fake_tensor(), None, None)
    assert rc < 0 and b"NULL" in lib.tpg_last_error()
    for c in (0, 5):
        rc = lib.tpg_denorm_u8(2, c, 8, 8, _fake_tensor(), p, None)
        assert rc < 0 and b"1..4" in lib.tpg_last_error(), c
    rc = lib.tpg_denorm_u8(2, 3, 8, 8, _fake_tensor(dtype=9), p, None)
    assert rc < 0 and b"dtype" in lib.tpg_last_error()
    assert lib.tpg_denorm_u8(2, 3, 0, 8, _fake_tensor(), p, None) < 0


def test_capi_metrics_validation(lib):
    p = ctypes.c_void_p(0x1000)
    args = lambda **k: [k.get("n", 2), k.get("h", 16), k.get("w", 16), k.get("c", 3), k.get("a", p), k.get("b", p),
                        k.get("sse", p), k.get("ssim", p), k.get("ws", p), k.get("ws_bytes", 1 << 20), None]
    for name in ("a", "b", "sse", "ws"):
        rc = lib.tpg_image_metrics_u8(*args(**{name: None}))
        assert rc < 0 and b"NULL" in lib.tpg_last_error(), name
    for c in (0, 5):
        rc = lib.tpg_image_metrics_u8(*args(c=c))
        assert rc < 0 and b"1..4" in lib.tpg_last_error(), c
        assert lib.tpg_image_metrics_workspace(2, 16, 16, c) < 0
    rc = lib.tpg_image_metrics_u8(*args(h=10))
    assert rc < 0 and b"11" in lib.tpg_last_error()
    rc = lib.tpg_image_metrics_u8(*args(w=10))
    assert rc < 0 and b"11" in lib.tpg_last_error()
    rc = lib.tpg_image_metrics_u8(*args(ws_bytes=8))
    assert rc < 0 and b"workspace" in lib.tpg_last_error()
    assert lib.tpg_image_metrics_workspace(2, 11, 11, 3) > 0
    assert lib.tpg_image_metrics_workspace(3, 128, 128, 3) > 0
    assert lib.tpg_image_metrics_workspace(3, 128, 128, 3) > lib.tpg_image_metrics_workspace(2, 11, 11, 3)


def test_ops_reject_cpu_and_wrong_dtype():
    import tpgan_ops
    with pytest.raises(ValueError, match="device tensor"):
        tpgan_ops.denorm_u8(torch.zeros(1, 3, 8, 8))
    with pytest.raises(ValueError, match="4-D"):
        tpgan_ops.denorm_u8(torch.zeros(3, 8, 8))
    u = torch.zeros(1, 16, 16, 3, dtype=torch.uint8)
    with pytest.raises(ValueError, match="device tensor"):
        tpgan_ops.image_metrics(u, u)
    with pytest.raises(ValueError, match="uint8"):
        tpgan_ops.image_metrics(u.float(), u.float())


def test_from_checkpoint_names_missing_key(tmp_path):
    import D_and_G_model as DG
    import tpgan_infer
    G = DG.Generator(64, 347, use_batchnorm=False)
    sd = G.state_dict()
    gone = "global_pathway.conv6.0.bias" if "global_pathway.conv6.0.bias" in sd else sorted(sd)[7]
    short = {k: v for k, v in sd.items() if k != gone}
    path = str(tmp_path / "model_epoch_1.pth")
    torch.save(short, path)
    with pytest.raises(ValueError) as e:
        tpgan_infer.Frontalizer.from_checkpoint(path)
    assert gone in str(e.value) and "missing" in str(e.value)
    extra = dict(sd, not_a_layer=torch.zeros(1))
    torch.save(extra, path)
    with pytest.raises(ValueError, match="not_a_layer"):
        tpgan_infer.Frontalizer.from_checkpoint(path)
    wrong = dict(sd)
    wrong[gone] = torch.zeros(tuple(sd[gone].shape) + (2,))
    torch.save(wrong, path)
    with pytest.raises(ValueError, match="shape"):
        tpgan_infer.Frontalizer.from_checkpoint(path)
