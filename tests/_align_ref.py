"""numpy restatements of the face-alignment kernels (include/tpgan.h, tpg_similarity_fit and
tpg_affine_warp_u8), for the CPU and GPU alignment tests.

  fit64     the closed-form similarity fit in float64: the yardstick of the tolerance test
  fit32     the same formula in numpy float32 in the header's operation order (sums over the points
            in index order, IEEE divisions): its distance from fit64 is what float32 costs
  warp_int  the warp's integer rules in exact Python / int64 arithmetic, one floor division per
            sub-sample as the header states them (the kernel factors that division out)
"""
import numpy as np

IDENTITY = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0)


def fit64(points, template):
    """points [B, K, 2], template [K, 2] -> float64 [B, 6] = (a, -b, tx, b, a, ty)."""
    p = np.asarray(points, np.float64)
    q = np.asarray(template, np.float64)
    qm, pm = q.mean(0), p.mean(1)
    qc, pc = q - qm, p - pm[:, None, :]
    S = (qc * qc).sum()
    a = (qc[None, :, 0] * pc[:, :, 0] + qc[None, :, 1] * pc[:, :, 1]).sum(1) / S
    b = (qc[None, :, 0] * pc[:, :, 1] - qc[None, :, 1] * pc[:, :, 0]).sum(1) / S
    tx = pm[:, 0] - (a * qm[0] - b * qm[1])
    ty = pm[:, 1] - (b * qm[0] + a * qm[1])
    return np.stack([a, -b, tx, b, a, ty], 1)


def fit32(points, template):
    """The header's float32 sequence -> float32 [B, 6].  Every intermediate is a float32 array, so
    numpy rounds after each operation and nothing is contracted."""
    f = np.float32
    p = np.asarray(points, f)
    q = np.asarray(template, f)
    B, K = p.shape[0], p.shape[1]
    qs = np.zeros(2, f)
    for k in range(K):
        qs = qs + q[k]
    qm = qs / f(K)
    qc = q - qm
    S = f(0)
    for k in range(K):
        S = S + (qc[k, 0] * qc[k, 0] + qc[k, 1] * qc[k, 1])
    ps = np.zeros((B, 2), f)
    for k in range(K):
        ps = ps + p[:, k]
    pm = ps / f(K)
    sa, sb = np.zeros(B, f), np.zeros(B, f)
    for k in range(K):
        cx, cy = p[:, k, 0] - pm[:, 0], p[:, k, 1] - pm[:, 1]
        sa = sa + (qc[k, 0] * cx + qc[k, 1] * cy)
        sb = sb + (qc[k, 0] * cy - qc[k, 1] * cx)
    a, b = sa / S, sb / S
    tx = pm[:, 0] - (a * qm[0] - b * qm[1])
    ty = pm[:, 1] - (b * qm[0] + a * qm[1])
    out = np.stack([a, -b, tx, b, a, ty], 1)
    assert out.dtype == f
    return out


def q16(matrix):
    """rint(float32(v) * 65536) as int32, the fit's fixed-point output (float32 product: exact, a
    multiplication by a power of two)."""
    m = np.asarray(matrix, np.float32) * np.float32(65536.0)
    return np.rint(m).astype(np.int64).astype(np.int32)


def supersample(m):
    """(n, undersampled) of a 16.16 matrix (m00, m01, tx, m10, m11, ty), in exact integers."""
    m00, m01, _, m10, m11, _ = (int(v) for v in m)
    d = max(m00 * m00 + m10 * m10, m01 * m01 + m11 * m11)
    for n in range(1, 17):
        if (n * 65536) ** 2 >= d:
            return n, False
    return 16, True


def warp_int(src, m, out_h, out_w):
    """src uint8 [H, W, 3] (any strides), m six ints -> (uint8 [out_h, out_w, 3], status)."""
    src = np.asarray(src)
    H, W = src.shape[0], src.shape[1]
    m00, m01, tx, m10, m11, ty = (int(v) for v in m)
    n, under = supersample(m)
    pix = src.astype(np.int64)
    ox = np.arange(out_w, dtype=np.int64)[None, :]
    oy = np.arange(out_h, dtype=np.int64)[:, None]
    acc = np.zeros((out_h, out_w, 3), np.int64)
    for j in range(n):
        for i in range(n):
            U = 2 * n * ox + 2 * i + 1
            V = 2 * n * oy + 2 * j + 1
            X = tx + np.floor_divide(m00 * U + m01 * V, 2 * n) - 32768  # |.| < 2^50: exact in int64
            Y = ty + np.floor_divide(m10 * U + m11 * V, 2 * n) - 32768
            ix, fx = X >> 16, (X >> 8) & 255
            iy, fy = Y >> 16, (Y >> 8) & 255
            x0, x1 = np.clip(ix, 0, W - 1), np.clip(ix + 1, 0, W - 1)
            y0, y1 = np.clip(iy, 0, H - 1), np.clip(iy + 1, 0, H - 1)
            acc += ((256 - fx) * (256 - fy))[..., None] * pix[y0, x0] + (fx * (256 - fy))[..., None] * pix[y0, x1] \
                + ((256 - fx) * fy)[..., None] * pix[y1, x0] + (fx * fy)[..., None] * pix[y1, x1]
    assert acc.max() < 2 ** 32
    out = (acc + 32768 * n * n) // (65536 * n * n)
    assert out.min() >= 0 and out.max() <= 255
    return out.astype(np.uint8), 8 if under else 0
