"""GPU: FaceBatcher.resize / from_raw (tpg_resize_u8) against the reference's recorded Pillow
bytes (tests/golden/resize_golden.npz) and the restatement in tests/_resize_ref.py.  Integer
work: every comparison is exact."""
import numpy as np
import pytest
import torch

import _resize_ref as R
from oracle import data_oracle as DO

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gold():
    return R.load_golden()


@pytest.fixture(scope="module")
def fb(gpu):
    import DataAndDataset as DD
    return DD.FaceBatcher(gpu)


def _dev(arrs, gpu):
    return [torch.from_numpy(np.ascontiguousarray(a)).to(gpu) for a in arrs]


def _chain(fb, imgs, one_by_one):
    res, cur = [], imgs
    for s in (128, 64, 32):
        if one_by_one:
            cur = torch.cat([fb.resize([t], (s, s)) for t in cur])
        else:
            cur = fb.resize(cur, (s, s))
        res.append(cur)
        cur = list(cur.unbind(0)) if one_by_one else cur
    return [r.cpu().numpy() for r in res]


def test_fixture_heterogeneous_batch(gpu, fb, gold):
    """All eight raw sizes in ONE call per target (128, then 64 and 32 from the results): every
    byte is Pillow's.  The same images one per call give the same bytes (the job table)."""
    n = int(gold["n"])
    imgs = _dev([gold["%d:raw" % k] for k in range(n)], gpu)
    batch = _chain(fb, imgs, False)
    single = _chain(fb, imgs, True)
    for got, tag in zip(batch, ("u8_128", "u8_64", "u8_32")):
        assert got.dtype == np.uint8 and got.shape[0] == n
        for k in range(n):
            np.testing.assert_array_equal(got[k], gold["%d:%s" % (k, tag)], err_msg="%d %s" % (k, tag))
    for a, b in zip(batch, single):
        np.testing.assert_array_equal(a, b)


# (W, H, out_w, out_h): fewer source samples than taps with both bounds clipped; rows of 111
# bytes; 49 taps along W and an upscale along H; both passes skipped (a copy); an output row of
# 111 bytes (byte stores, a last group of 3); each single pass alone at an odd width
SHAPES = [(3, 5, 128, 128), (37, 53, 128, 128), (1024, 40, 128, 128), (128, 128, 128, 128), (200, 140, 37, 53),
          (61, 128, 128, 128), (128, 47, 128, 128), (1, 1, 128, 128), (257, 131, 1, 1)]


@pytest.mark.parametrize("shape", SHAPES, ids=["%dx%dto%dx%d" % s for s in SHAPES])
def test_shapes_against_restatement(gpu, fb, shape):
    w, h, ow, oh = shape
    rng = np.random.default_rng(w * 4099 + h)
    a = rng.integers(0, 256, (2, h, w, 3), dtype=np.uint8)
    ref = np.stack([R.resize(a[i], oh, ow) for i in range(2)])
    got_list = fb.resize(_dev([a[0], a[1]], gpu), (oh, ow)).cpu().numpy()
    got_tensor = fb.resize(torch.from_numpy(a).to(gpu), (oh, ow)).cpu().numpy()  # the [B, H, W, 3] form
    np.testing.assert_array_equal(got_list, ref)
    np.testing.assert_array_equal(got_tensor, ref)


def test_image_at_the_end_of_its_buffer(gpu, fb):
    """A 130x130 image (390-byte rows: every other row starts 2 bytes off a dword) that is the
    last thing in its allocation, and the same image followed by sentinel bytes: the output does
    not depend on anything outside the image."""
    rng = np.random.default_rng(130)
    a = rng.integers(0, 256, (130, 130, 3), dtype=np.uint8)
    ref = R.resize(a, 128, 128)
    n = a.size
    for lead in (0, 1, 2, 3):  # every address phase of the first row
        buf = torch.empty(lead + n, dtype=torch.uint8, device=gpu)
        buf[lead:].copy_(torch.from_numpy(a).reshape(-1))
        img = buf[lead:].view(130, 130, 3)  # ends exactly where the buffer ends
        np.testing.assert_array_equal(fb.resize([img])[0].cpu().numpy(), ref, err_msg="lead %d" % lead)
    outs = []
    for fill in (0xFF, 0x00):
        buf = torch.full((5 + n + 64,), fill, dtype=torch.uint8, device=gpu)
        buf[5:5 + n].copy_(torch.from_numpy(a).reshape(-1))
        outs.append(fb.resize([buf[5:5 + n].view(130, 130, 3)])[0].cpu().numpy())
        assert bool((buf[5 + n:] == fill).all()) and bool((buf[:5] == fill).all())
    np.testing.assert_array_equal(outs[0], ref)
    np.testing.assert_array_equal(outs[1], ref)


def test_checker_clips_at_both_ends(gpu, fb):
    yy, xx = np.mgrid[0:140, 0:200]
    a = np.repeat((((yy // 5 + xx // 5) & 1) * 255).astype(np.uint8)[:, :, None], 3, axis=2)
    a[:, :, 1] = 255 - a[:, :, 1]
    got = fb.resize(_dev([a], gpu))[0].cpu().numpy()
    assert (got == 0).any() and (got == 255).any() and ((got > 0) & (got < 255)).any()
    np.testing.assert_array_equal(got, R.resize(a, 128, 128))


def test_from_raw_matches_test_dataset(gpu, fb, gold):
    """from_raw on the raw photos gives the reference's TestDataset outputs bit for bit: patches,
    the 128 / 64 / 32 images in [-1, 1]; boxes are those __call__ computes from the fixture's own
    128x128 bytes."""
    import DataAndDataset as DD
    n = int(gold["n"])
    imgs = _dev([gold["%d:raw" % k] for k in range(n)], gpu)
    lm = torch.from_numpy(np.stack([gold["%d:lm68" % k] for k in range(n)])).to(gpu)
    out = fb.from_raw(imgs, lm)
    wh = np.array([[gold["%d:raw" % k].shape[1], gold["%d:raw" % k].shape[0]] for k in range(n)], np.float64)
    scale = torch.from_numpy((128.0 / wh).astype(np.float32)).to(gpu)
    u8_128 = torch.from_numpy(np.stack([gold["%d:u8_128" % k] for k in range(n)])).to(gpu)
    direct = fb(u8_128, lm, scale)
    assert torch.equal(out["boxes"], direct["boxes"])
    assert torch.equal(out["u8_128"], u8_128)
    for k in range(n):
        for name in DD.PATCH_NAMES:
            np.testing.assert_array_equal(out[name][k].cpu().numpy(), gold["%d:%s" % (k, name)],
                                          err_msg="%d %s" % (k, name))
        # the generator asserted, for every sample, that the reference's whole-image tensors are
        # this float32 map of the recorded bytes; sample 0's tensors are recorded and pin the map
        for key, tag in (("I128", "u8_128"), ("I64", "u8_64"), ("I32", "u8_32")):
            np.testing.assert_array_equal(out[key][k].cpu().numpy(), DO.to_unit(gold["%d:%s" % (k, tag)]),
                                          err_msg="%d %s" % (k, key))
    for key, ref in (("I128", "0:img"), ("I64", "0:img64"), ("I32", "0:img32")):
        np.testing.assert_array_equal(out[key][0].cpu().numpy(), gold[ref])
    # the [B, H, W, 3] form on the one 128x128 face
    one = fb.from_raw(imgs[0][None], lm[:1])
    for key in ("I128", "I64", "I32", "left_eye", "mouth", "boxes"):
        assert torch.equal(one[key][0], out[key][0])


def test_rejects_what_the_kernels_cannot_take(gpu, fb):
    good = torch.zeros(40, 50, 3, dtype=torch.uint8, device=gpu)
    with pytest.raises(ValueError, match="must be on"):
        fb.resize([good, torch.zeros(40, 50, 3, dtype=torch.uint8)])
    with pytest.raises(ValueError, match="uint8"):
        fb.resize([good.float()])
    with pytest.raises(ValueError, match="contiguous"):
        fb.resize([torch.zeros(40, 100, 3, dtype=torch.uint8, device=gpu)[:, ::2]])
    with pytest.raises(ValueError, match="contiguous"):
        fb.resize(torch.zeros(2, 40, 50, 6, dtype=torch.uint8, device=gpu)[..., ::2])
    with pytest.raises(ValueError, match="3 interleaved bands"):
        fb.resize([torch.zeros(40, 50, 4, dtype=torch.uint8, device=gpu)])
    with pytest.raises(ValueError, match="3 interleaved bands"):
        fb.resize(torch.zeros(2, 40, 50, 4, dtype=torch.uint8, device=gpu))
    with pytest.raises(ValueError, match="uint8"):
        fb.resize([good[0]])  # [W, 3]: not an image
    with pytest.raises(ValueError, match="1..4096"):
        fb.resize([good], (0, 128))
    out = fb.resize([])
    assert out.shape == (0, 128, 128, 3) and out.dtype == torch.uint8 and out.device == gpu
    assert fb.resize(torch.zeros(0, 40, 50, 3, dtype=torch.uint8, device=gpu), (64, 32)).shape == (0, 64, 32, 3)


def test_two_streams_and_a_growing_table_cache(gpu):
    """Two calls on two streams with different batches, the second adding size pairs to the
    cached table buffer while the first may still run: both exact, and the tables the first call
    was given are the same bytes at the same address afterwards."""
    import DataAndDataset as DD
    fb = DD.FaceBatcher(gpu)
    rng = np.random.default_rng(99)
    a = rng.integers(0, 256, (24, 200, 260, 3), dtype=np.uint8)
    b = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for w, h in ((61, 45), (300, 128), (260, 90))]
    ta, tb = torch.from_numpy(a).to(gpu), _dev(b, gpu)
    ref_a = np.stack([R.resize(a[0], 128, 128), R.resize(a[23], 128, 128)])
    ref_b = np.stack([R.resize(x, 128, 128) for x in b])
    fb.resize(ta[:1])  # the first batch's tables are in the cache before the streams start
    used = fb._tab_used
    ptr, before = fb._tab.data_ptr(), fb._tab[:used].clone()
    s1, s2 = torch.cuda.Stream(gpu), torch.cuda.Stream(gpu)
    torch.cuda.synchronize()
    with torch.cuda.stream(s1):
        ra = fb.resize(ta)
    with torch.cuda.stream(s2):
        rb = fb.resize(tb)
    with torch.cuda.stream(s1):
        rb1 = fb.resize(tb)  # on the other stream, from the tables the second call added
    torch.cuda.synchronize()
    assert fb._tab_used > used and fb._tab.data_ptr() == ptr and torch.equal(fb._tab[:used], before)
    np.testing.assert_array_equal(ra[[0, 23]].cpu().numpy(), ref_a)
    np.testing.assert_array_equal(rb.cpu().numpy(), ref_b)
    np.testing.assert_array_equal(rb1.cpu().numpy(), ref_b)
    assert torch.equal(ra[1:], fb.resize(ta[1:]))


def test_copy_only_batch_on_a_fresh_batcher(gpu):
    """Both passes skipped for every image, before any table exists: the launch copies."""
    import DataAndDataset as DD
    fresh = DD.FaceBatcher(gpu)
    a = torch.from_numpy(np.random.default_rng(3).integers(0, 256, (3, 128, 128, 3), dtype=np.uint8)).to(gpu)
    got = fresh.resize(a)
    assert torch.equal(got, a) and got.data_ptr() != a.data_ptr() and fresh._tab_used == 0
