"""numpy restatement of the inference image path (tp-gan_amd/csrc/tpg_image.hip): the u8
rounding rule of tpg_denorm_u8, the integer squared error and Wang et al.'s SSIM of
tpg_image_metrics_u8.  ssim() takes the arithmetic dtype and the accumulation form, so the
float32 forms can be compared with float64 on the CPU (tests/test_image_host.py)."""
import numpy as np


def denorm_u8(x):
    """x: float array holding the element values (a bf16 / f16 tensor converted to float32 is
    exact) -> uint8, step by step in float32 (numpy rounds after every operation: no FMA)."""
    x = np.asarray(x, np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        t = (x + np.float32(1.0)) * np.float32(127.5)
        t = t + np.float32(0.5)
        t = np.where(np.isnan(t), np.float32(0.0), t)
        return np.clip(np.floor(t), 0.0, 255.0).astype(np.uint8)


def normalize(u8):
    """FaceBatcher.normalize's u / 255 * 2 - 1 in float32 (tpg_crop_normalize)."""
    u = np.asarray(u8).astype(np.float32)
    return (u / np.float32(255.0)) * np.float32(2.0) - np.float32(1.0)


def sse(a, b):
    d = np.asarray(a).astype(np.int64) - np.asarray(b).astype(np.int64)
    return int((d * d).sum())


def gauss(dtype=np.float64):
    k = np.arange(11, dtype=np.float64)
    g = np.exp(-(k - 5.0) ** 2 / (2.0 * 1.5 ** 2))
    return (g / g.sum()).astype(dtype)


C1, C2 = 6.5025, 58.5225


def _sep(x, g):
    """Valid 11-tap correlation along W then H of [H, W, C], accumulated tap by tap in x's dtype."""
    H, W, _ = x.shape
    t = np.zeros((H, W - 10, x.shape[2]), x.dtype)
    for k in range(11):
        t = t + g[k] * x[:, k:k + W - 10]
    o = np.zeros((H - 10, W - 10, x.shape[2]), x.dtype)
    for k in range(11):
        o = o + g[k] * t[k:k + H - 10]
    return o


def ssim(a, b, dtype=np.float64, form="centred"):
    """a, b: uint8 [H, W, C] (H, W >= 11) -> python float, everything in `dtype`.
    form "raw":     separable passes over x, y, x^2, y^2, xy; sigma = E[xy] - mu_x mu_y
                    (the kernel's form, which runs it in float64);
    form "centred": each 11 x 11 window directly, sigma = sum w (x - mu_x)(y - mu_y)
                    (no cancellation; in float64 the reference the tests compare against)."""
    a = np.asarray(a).astype(dtype)
    b = np.asarray(b).astype(dtype)
    g = gauss(dtype)
    c1, c2 = dtype(C1), dtype(C2)
    if form == "raw":
        mu_a, mu_b = _sep(a, g), _sep(b, g)
        va = _sep(a * a, g) - mu_a * mu_a
        vb = _sep(b * b, g) - mu_b * mu_b
        cov = _sep(a * b, g) - mu_a * mu_b
    else:
        w2 = np.outer(g, g).astype(dtype)
        wa = np.lib.stride_tricks.sliding_window_view(a, (11, 11), axis=(0, 1))  # [H-10, W-10, C, 11, 11]
        wb = np.lib.stride_tricks.sliding_window_view(b, (11, 11), axis=(0, 1))
        mu_a = (wa * w2).sum(axis=(-2, -1), dtype=dtype)
        mu_b = (wb * w2).sum(axis=(-2, -1), dtype=dtype)
        da = wa - mu_a[..., None, None]
        db = wb - mu_b[..., None, None]
        va = (w2 * da * da).sum(axis=(-2, -1), dtype=dtype)
        vb = (w2 * db * db).sum(axis=(-2, -1), dtype=dtype)
        cov = (w2 * da * db).sum(axis=(-2, -1), dtype=dtype)
    m = ((dtype(2) * mu_a * mu_b + c1) * (dtype(2) * cov + c2)) / ((mu_a * mu_a + mu_b * mu_b + c1) * (va + vb + c2))
    assert m.dtype == dtype
    return float(m.mean(dtype=dtype))


def psnr(sse_, hwc):
    return float("inf") if sse_ == 0 else 10.0 * np.log10(255.0 ** 2 * hwc[0] * hwc[1] * hwc[2] / sse_)


def metric_cases():
    """name -> (a, b) uint8 [H, W, 3]: the pairs the SSIM bound is checked on, host and device."""
    rng = np.random.RandomState(7)
    out = {}
    out["noise"] = (rng.randint(0, 256, (128, 128, 3)).astype(np.uint8),
                    rng.randint(0, 256, (128, 128, 3)).astype(np.uint8))
    y, x = np.mgrid[0:128, 0:128].astype(np.float64)
    smooth = np.stack([127.5 + 100.0 * np.sin(x / 9.0 + c) * np.cos(y / 13.0 - c) for c in range(3)], -1)
    out["smooth"] = (np.clip(np.rint(smooth), 0, 255).astype(np.uint8),
                     np.clip(np.rint(smooth + rng.normal(0.0, 8.0, smooth.shape)), 0, 255).astype(np.uint8))
    flat = np.full((128, 128, 3), 254, np.uint8)
    rows = flat.copy()
    rows[1::2] = 253
    out["flat_bright"] = (flat, rows)
    same = rng.randint(0, 256, (23, 17, 3)).astype(np.uint8)
    out["identical_23x17"] = (same, same.copy())
    out["one_window_11x11"] = (rng.randint(0, 256, (11, 11, 3)).astype(np.uint8),
                               rng.randint(0, 256, (11, 11, 3)).astype(np.uint8))
    return out
