"""Python restatement of Pillow's 8-bit LANCZOS resize (Image.resize(size, Image.LANCZOS) on RGB
images), the specification tpg_resize_coeffs and tpg_resize_u8 are held to byte for byte.

Per axis, in -> out samples, 22 fractional bits:
    scale = in / out;  fs = max(scale, 1);  support = 3 * fs;  ksize = int(ceil(support)) * 2 + 1
    per output xx: center = (xx + 0.5) * scale, window [xmin, xmin + n) clipped to the axis,
    weights lanczos((x + xmin - center + 0.5) / fs) normalised by their sum (added in index
    order), rounded half away from zero to integers.
    (Pillow multiplies by 1 / fs, as the library does; the rounded tables of every pair the
    tests use are the same either way.)
One pass: out = clip(((1 << 21) + sum_x src[xmin + x] * k[x]) >> 22, 0, 255).  The pass along
W runs first and leaves a uint8 image; the pass along H runs on that.  A pass whose in == out is
skipped.
"""
import math

import numpy as np

PB = 22


def sinc(x):
    if x == 0.0:
        return 1.0
    x = x * math.pi
    return math.sin(x) / x


def lanczos(x):
    if -3.0 <= x < 3.0:
        return sinc(x) * sinc(x / 3.0)
    return 0.0


def ksize(in_size, out_size):
    return int(math.ceil(3.0 * max(in_size / out_size, 1.0))) * 2 + 1


def coeffs(in_size, out_size):
    """-> (bounds int32 [out, 2] = (xmin, n), k int32 [out, ksize])."""
    scale = in_size / out_size
    fs = max(scale, 1.0)
    support = 3.0 * fs
    ks = int(math.ceil(support)) * 2 + 1
    bounds = np.zeros((out_size, 2), np.int32)
    k = np.zeros((out_size, ks), np.int32)
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size)
        n = xmax - xmin
        w = [lanczos((x + xmin - center + 0.5) / fs) for x in range(n)]
        tot = 0.0
        for v in w:
            tot += v
        for x in range(n):
            v = w[x] / tot if tot != 0.0 else w[x]
            k[xx, x] = int(v * (1 << PB) + 0.5) if v >= 0 else int(v * (1 << PB) - 0.5)
        bounds[xx] = (xmin, n)
    return bounds, k


def pass_w(a, out_size, table=coeffs):
    """One pass along axis 1 of a uint8 [H, W, C] array; `table(in, out)` supplies (bounds, k)."""
    h, w, c = a.shape
    if out_size == w:
        return a
    bounds, k = table(w, out_size)
    ai = a.astype(np.int64)
    out = np.zeros((h, out_size, c), np.uint8)
    for xx in range(out_size):
        xmin, n = int(bounds[xx, 0]), int(bounds[xx, 1])
        ss = (1 << (PB - 1)) + np.tensordot(ai[:, xmin:xmin + n, :], k[xx, :n].astype(np.int64), axes=([1], [0]))
        assert np.abs(ss).max() < 2 ** 31  # the device sums in int32
        out[:, xx, :] = np.clip(ss >> PB, 0, 255)
    return out


def resize(a, out_h, out_w, table=coeffs):
    """uint8 [H, W, 3] -> uint8 [out_h, out_w, 3], W first, then H on the rounded image."""
    t = pass_w(np.ascontiguousarray(a), out_w, table)
    return np.ascontiguousarray(pass_w(t.transpose(1, 0, 2), out_h, table).transpose(1, 0, 2))


def load_golden():
    """tests/golden/resize_golden.npz (make_golden_resize.py) as a dict, completed with the arrays
    it shares with data_golden.npz: the first four faces' k:u8_128 and 0:img."""
    import os
    here = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    with np.load(os.path.join(here, "resize_golden.npz"), allow_pickle=False) as z:
        g = {k: z[k] for k in z.files}
    with np.load(os.path.join(here, "data_golden.npz"), allow_pickle=False) as z:
        for k in range(int(g["n"])):
            if "%d:u8_128" % k not in g:
                g["%d:u8_128" % k] = z["test:%d:u8_128" % k]
        g["0:img"] = z["test:0:img"]
    return g
