"""numpy float32 restatements of the landmark front end, independent of the kernels:

  decode_top1   per landmark class the anchor of the largest softmax score.  The choice is made
                on a float64 softmax (lowest index among equal scores, NaN never); the reported
                score is the kernels' float32 expression exp(x[l] - logsumexp(x)).
  boxes         process()'s crop boxes (DataAndDataset.py:42-54) on [le, re, nose, mouth, mouth]:
                the midpoint of the mouth with itself is the mouth, then floor and the +-half sizes.
  accuracy      Pretrain.py's banded accuracy (:17-64), the bands summed in the reference's order.

tests/test_landmark_host.py pins all three to the reference's own run (landmark_golden.npz).
"""
import math

import numpy as np

PATCH_WH = ((40, 40), (40, 40), (40, 32), (48, 32))  # (w, h): left_eye, right_eye, nose, mouth
THRESHOLDS = (5, 10, 18, 30, 45)
WEIGHTS = (1.0, 0.9, 0.65, 0.35, 0.1)


def lse32(x):
    """float32 logsumexp of one logit row, in the kernels' order: max, sequential sum of exp, log."""
    x = np.asarray(x, np.float32)
    m = x[0]
    for v in x[1:]:
        m = np.maximum(m, v)
    s = np.float32(0)
    for v in x:
        s = np.float32(s + np.exp(np.float32(v - m), dtype=np.float32))
    return np.float32(m + np.log(s, dtype=np.float32))


def decode_top1(loc, cls, conf, scale=None):
    """loc (B, n, 2), cls (B, n, C) float32 -> (points (B, 4, 2), score (B, 4), anchor (B, 4), status (B))."""
    loc, cls = np.asarray(loc, np.float32), np.asarray(cls, np.float32)
    B, n, C = cls.shape
    points = np.full((B, 4, 2), np.nan, np.float32)
    score = np.zeros((B, 4), np.float32)
    anchor = np.full((B, 4), -1, np.int32)
    status = np.zeros(B, np.int32)
    with np.errstate(all="ignore"):
        x = cls.astype(np.float64)
        e = np.exp(x - x.max(axis=2, keepdims=True))
        p = e / e.sum(axis=2, keepdims=True)
        for b in range(B):
            for l in range(4):
                col = p[b, :, l]
                ok = ~np.isnan(col)
                if ok.any():
                    a = int(np.argmax(np.where(ok, col, -np.inf)))  # (argmax: the first of equal maxima)
                    anchor[b, l] = a
                    score[b, l] = np.exp(np.float32(cls[b, a, l] - lse32(cls[b, a])), dtype=np.float32)
                    pt = loc[b, a].copy()
                    if scale is not None:
                        pt = (pt * np.asarray(scale, np.float32)[b]).astype(np.float32)
                    points[b, l] = pt
                if not (anchor[b, l] >= 0 and score[b, l] > np.float32(conf)):
                    status[b] |= 1 << l
                if not np.all(np.isfinite(points[b, l])) or np.any(np.abs(points[b, l]) > 1e9):
                    status[b] |= 16
    return points, score, anchor, status


def boxes(points):
    """points (B, 4, 2) float32 -> int32 (B, 4, 4) (left, upper, right, lower).  A coordinate the
    reference's math.floor raises on (NaN, infinite; the kernels also |v| > 1e9) counts as 0."""
    points = np.asarray(points, np.float32)
    out = np.zeros((points.shape[0], 4, 4), np.int32)
    for b in range(points.shape[0]):
        lm = np.concatenate([points[b], points[b, 3:4]]).astype(np.float32)  # [le, re, nose, mouth, mouth]
        with np.errstate(all="ignore"):
            lm[3, 0] = (lm[3, 0] + lm[4, 0]) / np.float32(2.0)
            lm[3, 1] = (lm[3, 1] + lm[4, 1]) / np.float32(2.0)
        for i, (w, h) in enumerate(PATCH_WH):
            xy = [math.floor(v) if np.isfinite(v) and abs(v) <= 1e9 else 0 for v in lm[i]]
            out[b, i] = (xy[0] - w // 2 + 1, xy[1] - h // 2 + 1, xy[0] + w // 2 + 1, xy[1] + h // 2 + 1)
    return out


def accuracy(pred, truth, status=None, thresholds=THRESHOLDS, weights=WEIGHTS):
    """pred, truth (B, 4, 2) or (B, 8) float32 -> float32 (B)."""
    pred = np.asarray(pred, np.float32).reshape(-1, 4, 2)
    truth = np.asarray(truth, np.float32).reshape(-1, 4, 2)
    out = np.zeros(pred.shape[0], np.float32)
    with np.errstate(all="ignore"):
        d2 = (pred - truth) ** 2                             # float32 squares
        d = np.sqrt((d2[..., 0] + d2[..., 1]).astype(np.float32))
    for b in range(pred.shape[0]):
        total = np.float32(0)
        for l in range(4):
            sc, prev = np.float32(0), np.float32(0)
            for t, w in zip(thresholds, weights):
                if d[b, l] > prev and d[b, l] <= np.float32(t):
                    sc = np.float32(sc + np.float32(w))
                prev = np.float32(t)
            if status is not None and (int(status[b]) >> l) & 1:
                sc = np.float32(0)
            total = np.float32(total + sc)                   # sequential float32 sum, then / 4
        out[b] = total / np.float32(4)
    return out
