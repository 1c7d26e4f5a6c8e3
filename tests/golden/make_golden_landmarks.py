"""Golden fixture for the landmark front end, made by running the REFERENCE's own decoder and
accuracy measure here on the CPU (never on the GPU box):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_landmarks.py

torchvision (imported by Pretrain.py:6, DataAndDataset.py:3, UtilityMethods.py:9) and
torch.utils.tensorboard (Pretrain.py:8) are not installed: both are stubbed, neither is used by
what runs here.  Recorded per case k (hand-built head outputs of 12 to 40 anchors, batch 1):
  k:loc, k:cls, k:truth   the inputs: locations (1, n, 2), logits (1, n, 5), truth (1, 8)
  k:planted               the one anchor per class (five of them, the background included) whose
                          softmax score is above 0.5 -- so the reference's positional predicts[:-1]
                          coincides with "drop the background class"
  k:dec_class, k:dec_score, k:dec_point   MultiTaskDecoder()(loc, cls)[0], (class, score, point)
  k:acc                   Pretrain._calculate_accuracy(decoded, truth)
  k:dist                  the distances the case was built for (documentation; 0, the band edges
                          5 / 10 / 18 / 30 / 45, one float32 step past an edge, and beyond 45)
"""
import os
import sys
import types

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"

import numpy as np  # noqa: E402
import torch  # noqa: E402


def _stub_modules():
    tv = types.ModuleType("torchvision")
    tvt = types.ModuleType("torchvision.transforms")
    tv.transforms = tvt
    sys.modules.setdefault("torchvision", tv)
    sys.modules.setdefault("torchvision.transforms", tvt)
    tb = types.ModuleType("torch.utils.tensorboard")
    tb.SummaryWriter = object
    sys.modules.setdefault("torch.utils.tensorboard", tb)
    sys.path.insert(0, REF)


def up(v):
    """The next float32 above v."""
    return float(np.nextafter(np.float32(v), np.float32(np.inf)))


# per case: anchors, truth (4 points), and per landmark the offset of the predicted point from
# the truth.  Truth coordinates are small integers or zero so the offsets survive the float32
# subtraction exactly; (3, 4), (6, 8), (18, 24), (27, 36) are exact 5 / 10 / 30 / 45 diagonals.
T0 = [(0, 0), (0, 0), (0, 0), (0, 0)]
T1 = [(40, 52), (88, 50), (64, 76), (66, 100)]
CASES = [
    (12, T1, [(0, 0), (3, 0), (0, 12), (40, 0)]),                    # 0.4375: the exact hit scores 0
    (17, T0, [(5, 0), (up(5), 0), (10, 0), (18, 0)]),
    (23, T0, [(30, 0), (0, 45), (0, up(45)), (60, 0)]),
    (40, T0, [(up(18), 0), (0, up(30)), (up(10), 0), (1e-3, 0)]),
    (31, T1, [(3, 4), (6, 8), (18, 24), (27, 36)]),
    (13, T1, [(-3, -4), (-6, 8), (18, -24), (-27, -36)]),           # towards negative coordinates
    (29, [(2, 3), (1, 1), (0, 2), (3, 0)], [(-5, 0), (0, -10), (-18, 0), (0, -30)]),  # negative points
    (36, T1, [(40, 0), (20, 0), (12, 0), (7, 0)]),                   # scores 0.1 0.35 0.65 0.9
    (24, T1, [(7, 0), (12, 0), (20, 0), (40, 0)]),                   # the same, the other way round
    (19, T1, [(20, 0), (7, 0), (40, 0), (12, 0)]),
    (27, T1, [(1, 0), (7, 0), (12, 0), (20, 0)]),                    # 1.0 0.9 0.65 0.35
    (33, T1, [(2.5, 1.25), (0, 44.75), (100, 100), (0.5, 0)]),
    (15, T0, [(0, 0), (0, 0), (0, 0), (0, 0)]),                      # four exact hits: 0
]


def build(k, n, truth, offs, rng):
    loc = (rng.random((n, 2)) * 120).astype(np.float32) + np.float32(0.37)
    cls = ((rng.random((n, 5)) - 0.5)).astype(np.float32)            # no class near 0.5 anywhere ...
    planted = rng.permutation(n)[:5]
    for c, a in enumerate(planted):                                  # ... but at one anchor per class
        cls[a, c] = np.float32(2.5 + 0.5 * ((k + c) % 7))
    truth = np.array(truth, np.float32)
    for l in range(4):
        loc[planted[l]] = truth[l] + np.array(offs[l], np.float32)
    return loc[None], cls[None], truth.reshape(1, 8), planted.astype(np.int32)


def main():
    _stub_modules()
    import MobileNetV2 as RM
    import Pretrain as RP

    rng = np.random.default_rng(20261021)
    dec = RM.MultiTaskDecoder()
    rec = {"ncases": np.array(len(CASES))}
    for k, (n, truth, offs) in enumerate(CASES):
        loc, cls, tr, planted = build(k, n, truth, offs, rng)
        out = dec(torch.from_numpy(loc), torch.from_numpy(cls))
        assert len(out) == 1 and [c for c, _, _ in out[0]] == [0, 1, 2, 3, 4], out
        acc = RP._calculate_accuracy(out[0], torch.from_numpy(tr))
        rec["%d:loc" % k], rec["%d:cls" % k], rec["%d:truth" % k], rec["%d:planted" % k] = loc, cls, tr, planted
        rec["%d:dec_class" % k] = np.array([c for c, _, _ in out[0]], np.int32)
        rec["%d:dec_score" % k] = np.array([float(s) for _, s, _ in out[0]], np.float32)
        rec["%d:dec_point" % k] = np.stack([p.numpy() for _, _, p in out[0]]).astype(np.float32)
        rec["%d:acc" % k] = np.array(acc, np.float32)
        assert np.float32(acc) == acc  # (.item() of a float32 mean)
        rec["%d:dist" % k] = np.array([np.hypot(*o) for o in offs], np.float64)
        print(k, n, rec["%d:dist" % k].round(4).tolist(), acc)
    assert abs(float(rec["0:acc"]) - 0.4375) == 0.0
    np.savez_compressed(os.path.join(HERE, "landmark_golden.npz"), **rec)
    print("wrote %d arrays" % len(rec))


if __name__ == "__main__":
    main()
