"""Golden fixture for the LANCZOS resize and FaceBatcher.from_raw, made by running the REFERENCE's
own TestDataset (and Pillow) here, never on the GPU box:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_resize.py

torchvision is stubbed as in make_golden_data.py (ToTensor: HWC u8 -> CHW float32 / 255) and the
five-point table is R5 (index 54).  The first four faces repeat make_golden_data.py's seeded
recipe (128x128, 150x170, 96x110, 200x140); the generator asserts that their 128x128 bytes are
data_golden.npz's test:k:u8_128, which ties the two fixtures together.  Four more raw sizes
follow: 37x53 (rows of 111 bytes), 129x127 (a 0/255 checker of 5-pixel squares: the ringing at
its edges is clipped at both ends), 128x300 (pass along W skipped) and 300x128 (pass along H
skipped).  Sizes are (width, height).

Recorded per sample k (resize_golden.npz):
  k:raw      the uint8 [H, W, 3] image TestDataset opened       k:lm68  float32 [68, 2]
  k:u8_128 / k:u8_64 / k:u8_32   Image.resize(..., LANCZOS) chain 128 -> 64 -> 32, uint8 HWC
  k:left_eye, k:right_eye, k:nose, k:mouth   the reference's patches, float32 CHW in [-1, 1]
  0:img64, 0:img32               the reference's whole images, float32 CHW in [-1, 1]
Everything the issue lists would take 1.9 MB, mostly incompressible random bytes, so what another
array already holds is asserted here instead of stored again:
  - k:u8_128 of the first four faces and 0:img ARE data_golden.npz's test:k:u8_128 and test:0:img
    (asserted below); tests/_resize_ref.py's load_golden() reads them from there;
  - for k > 0 the whole-image tensors img / img64 / img32 are not stored: the generator asserts,
    for EVERY sample, that they equal u8 / 255 * 2 - 1 of the recorded bytes computed in float32,
    the map sample 0's tensors pin (make_golden_data.py does the same for its img).
  pil_version  PIL.__version__
"""
import os
import sys
import tempfile

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import numpy as np  # noqa: E402
import PIL  # noqa: E402
from PIL import Image  # noqa: E402

from make_golden_data import _stub_torchvision  # noqa: E402

EXTRA = [(37, 53), (129, 127), (128, 300), (300, 128)]
CHECKER = 5  # sample index of the 0/255 checker


def to_unit(u8):
    return (np.transpose(u8, (2, 0, 1)).astype(np.float32) / np.float32(255) * np.float32(2) - np.float32(1))


def main():
    _stub_torchvision()
    import UtilityMethods as UM
    import DataAndDataset as DD

    # make_golden_data.py's stream: the two landmark draws of its part 1 come first
    rng = np.random.default_rng(20260117)
    rng.random((6, 68, 2))
    rng.random((6, 68, 2))
    UM.five_pts_idx[4] = [54, 54]
    sizes = [(128, 128), (150, 170), (96, 110), (200, 140)]
    imgs, lms = [], []
    for k, (w, h) in enumerate(sizes):
        imgs.append((rng.random((h, w, 3)) * 256).astype(np.uint8))
        base = rng.random((68, 2)) * np.array([w, h])
        if k == 1:
            base[36:48] = [[2.0, 3.0]] * 12
        if k == 3:
            base[27:36] = [[w - 1.5, h - 0.5]] * 9
        lms.append(" ".join("%.3f" % v for v in base.astype(np.float32).reshape(-1)))
    rng2 = np.random.default_rng(20261020)
    for w, h in EXTRA:
        k = len(imgs)
        if k == CHECKER:
            yy, xx = np.mgrid[0:h, 0:w]
            img = np.repeat((((yy // 5 + xx // 5) & 1) * 255).astype(np.uint8)[:, :, None], 3, axis=2)
            img[:, :, 1] = 255 - img[:, :, 1]  # bands out of phase
        else:
            img = (rng2.random((h, w, 3)) * 256).astype(np.uint8)
        imgs.append(np.ascontiguousarray(img))
        base = rng2.random((68, 2)) * np.array([w, h])
        lms.append(" ".join("%.3f" % v for v in base.astype(np.float32).reshape(-1)))

    rec = {"pil_version": np.array(PIL.__version__)}
    with np.load(os.path.join(HERE, "data_golden.npz"), allow_pickle=False) as z:
        data_gold = {k: z[k] for k in z.files}
    with tempfile.TemporaryDirectory() as td:
        paths = []
        for k, img in enumerate(imgs):
            p = os.path.join(td, "face%d.png" % k)
            Image.fromarray(img).save(p)
            paths.append(p)
        ds = DD.TestDataset(paths, lms)
        for k in range(len(paths)):
            b = ds[k]
            raw = np.asarray(Image.open(paths[k]))
            np.testing.assert_array_equal(raw, imgs[k])
            u128 = np.asarray(Image.fromarray(raw).resize((128, 128), Image.LANCZOS))
            u64 = np.asarray(Image.fromarray(u128).resize((64, 64), Image.LANCZOS))
            u32 = np.asarray(Image.fromarray(u64).resize((32, 32), Image.LANCZOS))
            if k < len(sizes):
                np.testing.assert_array_equal(u128, data_gold["test:%d:u8_128" % k])
                np.testing.assert_array_equal(np.array(lms[k].split(" "), np.float32).reshape(-1, 2),
                                              data_gold["test:%d:lm68" % k])
            for key, u in (("img", u128), ("img64", u64), ("img32", u32)):
                np.testing.assert_array_equal(b[key].numpy(), to_unit(u))
                if k == 0 and key != "img":
                    rec["0:%s" % key] = b[key].numpy()
            if k == 0:
                np.testing.assert_array_equal(b["img"].numpy(), data_gold["test:0:img"])
            for key in ("left_eye", "right_eye", "nose", "mouth"):
                rec["%d:%s" % (k, key)] = b[key].numpy()
            rec["%d:raw" % k] = raw
            rec["%d:lm68" % k] = np.array(lms[k].split(" "), np.float32).reshape(-1, 2)
            rec["%d:u8_64" % k], rec["%d:u8_32" % k] = u64, u32
            if k >= len(sizes):
                rec["%d:u8_128" % k] = u128
    out = rec["%d:u8_128" % CHECKER]
    assert (out == 0).any() and (out == 255).any()
    rec["n"] = np.array(len(imgs))
    dst = os.path.join(HERE, "resize_golden.npz")
    np.savez_compressed(dst, **rec)
    print("wrote %d arrays, %d bytes" % (len(rec), os.path.getsize(dst)))
    assert os.path.getsize(dst) < 1000000


if __name__ == "__main__":
    main()
