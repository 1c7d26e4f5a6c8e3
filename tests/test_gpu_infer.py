"""GPU: the inference path -- tpgan_ops.denorm_u8 / image_metrics (tpg_image.hip) against the
numpy restatement (tests/_image_ref.py), and tpgan_infer.Frontalizer against the existing
Generator forward, the reference's golden output, its own weight reloads and checkpoints."""
import numpy as np
import pytest
import torch

import _image_ref as R
from _cases import golden, load_det

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.bfloat16, torch.float16]
IDS = ["f32", "bf16", "f16"]
INS = ["I128", "left_eye", "right_eye", "nose", "mouth"]


# ---------------------------------------------------------------- denorm_u8

def _denorm_values(numel, rng):
    """uniform [-1.2, 1.2], then every half-way point (k + 0.5) / 127.5 - 1 with its two float32
    neighbours, +-3, +-inf and NaN (cycled to fill)."""
    k = np.arange(-2, 258, dtype=np.float64)
    half = ((k + 0.5) / 127.5 - 1.0).astype(np.float32)
    trio = np.stack([half, np.nextafter(half, np.float32(-4)), np.nextafter(half, np.float32(4))], -1).reshape(-1)
    special = np.concatenate([np.array([3, -3, np.inf, -np.inf, np.nan, 1, -1, 0], np.float32), trio])
    v = rng.uniform(-1.2, 1.2, numel).astype(np.float32)
    m = min(numel // 2, special.size)  # (the small shapes hold the first of them; 2x3x128x128 holds all)
    v[numel - m:] = special[:m]
    return v


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("layout", ["nchw", "nhwc", "nhwc_pad8"])
@pytest.mark.parametrize("shape", [(2, 3, 5, 7), (1, 1, 11, 13), (3, 4, 8, 8), (2, 3, 128, 128)],
                         ids=lambda s: "x".join(map(str, s)))
def test_denorm_u8_exact(gpu, shape, layout, dtype):
    import tpgan_ops
    n, c, h, w = shape
    rng = np.random.RandomState(sum(shape))
    vals = torch.from_numpy(_denorm_values(n * c * h * w, rng).reshape(shape)).to(dtype)
    if layout == "nchw":
        x = vals.to(gpu).contiguous()
    elif layout == "nhwc":  # a channels-last view, pixel stride c
        x = vals.to(gpu).permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
    else:  # the model's activations: a channel slice of an [N, H, W, 8] buffer
        buf = torch.full((n, h, w, 8), float("nan"), dtype=dtype, device=gpu)
        buf[..., :c] = vals.to(gpu).permute(0, 2, 3, 1)
        x = buf[..., :c].permute(0, 3, 1, 2)
    assert tuple(x.shape) == shape
    got = tpgan_ops.denorm_u8(x)
    want = R.denorm_u8(vals.float().numpy()).transpose(0, 2, 3, 1)
    assert got.dtype == torch.uint8 and tuple(got.shape) == (n, h, w, c) and got.is_contiguous()
    np.testing.assert_array_equal(got.cpu().numpy(), want)


def test_denorm_u8_unaligned_views(gpu):
    """Offsets that break the vector paths' alignment (odd storage offsets, a cropped window of a
    wider image) and a float16 NCHW tensor whose rows start 2-element aligned only."""
    import tpgan_ops
    rng = np.random.RandomState(3)
    big = torch.from_numpy(rng.uniform(-1.2, 1.2, (2, 3, 19, 23)).astype(np.float32)).to(gpu)
    for dt in DTYPES:
        b = big.to(dt)
        cl = b.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
        for x in (b[:, :, 1:, 3:], b[:, 1:, 2:9, 1:6], cl[:, :, :, 1:], cl[:, 1:], b[:, :, ::2, ::3]):
            want = R.denorm_u8(x.float().cpu().numpy()).transpose(0, 2, 3, 1)
            np.testing.assert_array_equal(tpgan_ops.denorm_u8(x).cpu().numpy(), want)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_denorm_u8_round_trip(gpu, dtype):
    from DataAndDataset import FaceBatcher
    import tpgan_ops
    fb = FaceBatcher(gpu, dtype=dtype)
    u8 = torch.arange(256, dtype=torch.uint8).repeat(3).reshape(1, 16, 16, 3).to(gpu)
    x = fb.normalize(u8)
    assert x.dtype == dtype
    assert torch.equal(tpgan_ops.denorm_u8(x), u8)


def test_ops_argument_errors(gpu):
    import tpgan_ops
    with pytest.raises(ValueError):
        tpgan_ops.denorm_u8(torch.zeros(1, 5, 8, 8, device=gpu))
    with pytest.raises(ValueError):
        tpgan_ops.denorm_u8(torch.zeros(1, 3, 8, 8, device=gpu, dtype=torch.float64))
    u = torch.zeros(1, 10, 16, 3, dtype=torch.uint8, device=gpu)
    with pytest.raises(ValueError, match="11"):
        tpgan_ops.image_metrics(u, u)
    sse, ssim = tpgan_ops.image_metrics(u, u, ssim=False)  # squared error alone has no size floor
    assert ssim is None and sse.tolist() == [0]
    with pytest.raises(ValueError, match="match"):
        tpgan_ops.image_metrics(u, u[:, :, :12])


# ---------------------------------------------------------------- image_metrics

@pytest.fixture(scope="module")
def metric_refs():
    """case -> (a, b, integer sse, float64 SSIM), computed once."""
    return {k: (a, b, R.sse(a, b), R.ssim(a, b, np.float64, "centred")) for k, (a, b) in R.metric_cases().items()}


def _dev(gpu, *arrs):
    return [torch.from_numpy(np.ascontiguousarray(a)).to(gpu) for a in arrs]


@pytest.mark.parametrize("case", ["noise", "smooth", "flat_bright", "identical_23x17", "one_window_11x11"])
def test_image_metrics_cases(gpu, metric_refs, case):
    import tpgan_infer
    import tpgan_ops
    a, b, sse_ref, ssim_ref = metric_refs[case]
    ta, tb = _dev(gpu, a[None], b[None])
    sse, ssim = tpgan_ops.image_metrics(ta, tb)
    assert sse.dtype == torch.int64 and ssim.dtype == torch.float32
    print("%s: sse %d (ref %d), ssim %.9f (ref %.9f, diff %.2e)" % (case, int(sse[0]), sse_ref, float(ssim[0]),
                                                                     ssim_ref, abs(float(ssim[0]) - ssim_ref)))
    assert int(sse[0]) == sse_ref
    assert abs(float(ssim[0]) - ssim_ref) <= 1e-5
    psnr = tpgan_infer.psnr_from_sse(sse, a.shape)
    assert psnr.dtype == torch.float64
    if case == "identical_23x17":
        assert sse_ref == 0 and float(psnr[0]) == float("inf") and float(ssim[0]) >= 1 - 1e-5
    else:
        assert abs(float(psnr[0]) - R.psnr(sse_ref, a.shape)) <= 1e-9
    # a second call is bit-identical
    sse2, ssim2 = tpgan_ops.image_metrics(ta, tb)
    assert torch.equal(sse, sse2) and torch.equal(ssim, ssim2)


def test_image_metrics_batch_equals_singles(gpu, metric_refs):
    import tpgan_ops
    names = ["noise", "smooth", "flat_bright"]  # three different 128 x 128 x 3 pairs
    ta, tb = _dev(gpu, np.stack([metric_refs[k][0] for k in names]), np.stack([metric_refs[k][1] for k in names]))
    sse, ssim = tpgan_ops.image_metrics(ta, tb)
    for i, k in enumerate(names):
        s1, m1 = tpgan_ops.image_metrics(ta[i:i + 1], tb[i:i + 1])
        assert torch.equal(sse[i:i + 1], s1) and torch.equal(ssim[i:i + 1], m1), k
        assert int(sse[i]) == metric_refs[k][2] and abs(float(ssim[i]) - metric_refs[k][3]) <= 1e-5, k
    assert len({float(v) for v in ssim}) == 3


@pytest.mark.parametrize("c", [1, 2, 4])
def test_image_metrics_channel_counts(gpu, c):
    """c = 1, 2 and 4 on a size that is no multiple of the 16-pixel tile."""
    import tpgan_ops
    rng = np.random.RandomState(40 + c)
    a = rng.randint(0, 256, (2, 37, 21, c)).astype(np.uint8)
    b = np.clip(a.astype(np.int32) + rng.randint(-20, 21, a.shape), 0, 255).astype(np.uint8)
    sse, ssim = tpgan_ops.image_metrics(*_dev(gpu, a, b))
    for i in range(2):
        assert int(sse[i]) == R.sse(a[i], b[i])
        assert abs(float(ssim[i]) - R.ssim(a[i], b[i], np.float64, "centred")) <= 1e-5


# ---------------------------------------------------------------- Frontalizer

@pytest.fixture(autouse=True)
def _no_autotune():
    import tpgan_ops
    old = tpgan_ops.AUTOTUNE["enabled"]
    tpgan_ops.AUTOTUNE["enabled"] = False
    yield
    tpgan_ops.AUTOTUNE["enabled"] = old


@pytest.fixture(scope="module")
def det_sd():
    """The e2e golden's deterministic Generator weights as a CPU state_dict."""
    import D_and_G_model as DG
    G = DG.Generator(64, 347, use_batchnorm=False)
    load_det(G, "G/", torch.float32)
    return {k: v.detach().clone() for k, v in G.state_dict().items()}


def _generator(sd):
    import D_and_G_model as DG
    G = DG.Generator(64, 347, use_batchnorm=False)
    G.load_state_dict(sd)
    return G


@pytest.fixture(scope="module")
def e2e_inputs(gpu):
    E = golden("e2e_golden.npz")
    batch = {k: torch.from_numpy(E["in:" + k]).float().to(gpu) for k in INS}
    return E, batch, torch.from_numpy(E["in:z"]).float().to(gpu)


@pytest.fixture(scope="module")
def existing_forward(gpu, det_sd, e2e_inputs):
    """dtype -> denorm_u8(G(...)[0]) of an independently loaded Generator run the existing way
    (no Frontalizer, weights packed inside each call), deterministic mode; computed once."""
    import tpgan_ops
    cache = {}

    def run(dtype):
        if dtype not in cache:
            _, b, z = e2e_inputs
            G = _generator(det_sd).to(gpu)
            with tpgan_ops.deterministic(), tpgan_ops.compute_dtype(dtype):
                out = G(b["I128"], b["left_eye"], b["right_eye"], b["nose"], b["mouth"], z, False)[0]
                cache[dtype] = tpgan_ops.denorm_u8(out)
            torch.cuda.synchronize()
        return cache[dtype]
    return run


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_frontalizer_equals_existing_forward(gpu, det_sd, e2e_inputs, existing_forward, dtype):
    import tpgan_infer
    import tpgan_ops
    _, batch, z = e2e_inputs
    fz = tpgan_infer.Frontalizer(_generator(det_sd), device=gpu, compute_dtype=dtype)
    assert not fz.G.training and not any(p.requires_grad for p in fz.G.parameters())
    assert all(isinstance(p._tpg_flat, tpgan_ops._FrozenPack) for p in fz.G.parameters())
    with tpgan_ops.deterministic():
        got = fz.frontalize_batch(batch, z)
        again = fz.frontalize_batch(batch, z)  # from the images packed by the first call
    want = existing_forward(dtype)
    assert got.dtype == torch.uint8 and tuple(got.shape) == (2, 128, 128, 3)
    assert torch.equal(got, want) and torch.equal(again, want)
    if dtype != torch.float32:  # packed once: the second call packed nothing new
        packed = [e for p in fz.G.parameters() for e in p._tpg_flat.pack_entries.values() if e is not None]
        assert packed and all(e.epoch == 0 for e in packed)


def test_frontalizer_keeps_a_trainers_flat_params(gpu, det_sd, e2e_inputs, existing_forward):
    """A Generator bound to FlatParams is used as it is: the holder that follows the optimizer stays,
    the module's mode and requires_grad flags are as they were after the call."""
    import tpgan_infer
    import tpgan_ops
    import tpgan_train
    _, batch, z = e2e_inputs
    G = _generator(det_sd).to(gpu)
    flat = tpgan_train.FlatParams(G, gpu)
    fz = tpgan_infer.Frontalizer(G, device=gpu, compute_dtype=torch.bfloat16)
    assert G.training and all(p._tpg_flat is flat and p.requires_grad for p in G.parameters())
    with tpgan_ops.deterministic():
        assert torch.equal(fz.frontalize_batch(batch, z), existing_forward(torch.bfloat16))
    assert G.training and all(p._tpg_flat is flat for p in G.parameters())


def test_frontalizer_against_reference_golden(gpu, det_sd, e2e_inputs):
    """fp32 output against the restatement's quantisation of the reference's float64 run: no byte
    off by more than 1, at most 1 % of bytes differ (the fp32 path is ~1e-6 relative from the
    golden, i.e. ~1e-4 LSB: about 1e-4 of the bytes sit that close to a rounding boundary)."""
    import tpgan_infer
    E, batch, z = e2e_inputs
    fz = tpgan_infer.Frontalizer(_generator(det_sd), device=gpu, compute_dtype=torch.float32)
    got = fz.frontalize_batch(batch, z).cpu().numpy().astype(np.int32)
    want = R.denorm_u8(E["out:I128_fake"].astype(np.float32)).transpose(0, 2, 3, 1).astype(np.int32)
    diff = np.abs(got - want)
    print("bytes differing from the golden's quantisation: %d of %d (max |diff| %d)"
          % (int((diff != 0).sum()), diff.size, int(diff.max())))
    assert diff.max() <= 1
    assert (diff != 0).mean() <= 0.01
    assert want.std() > 5  # (the golden image is not flat: the comparison means something)


def _perturbed(sd):
    out = {}
    for i, (k, v) in enumerate(sd.items()):
        if v.is_floating_point():
            ramp = torch.cos(torch.arange(v.numel(), dtype=torch.float32) * 0.37 + i).reshape(v.shape)
            out[k] = v * (1.0 + 0.05 * ramp)
        else:
            out[k] = v.clone()
    return out


def test_frontalizer_weights_follow_load_state_dict(gpu, det_sd, e2e_inputs):
    import tpgan_infer
    import tpgan_ops
    _, batch, z = e2e_inputs
    sd2 = _perturbed(det_sd)
    fz = tpgan_infer.Frontalizer(_generator(det_sd), device=gpu, compute_dtype=torch.bfloat16)
    with tpgan_ops.deterministic():
        first = fz.frontalize_batch(batch, z)
        fz.load_state_dict(sd2)
        second = fz.frontalize_batch(batch, z)
        fresh = tpgan_infer.Frontalizer(_generator(sd2), device=gpu, compute_dtype=torch.bfloat16)
        want = fresh.frontalize_batch(batch, z)
    assert not torch.equal(first, second)
    assert torch.equal(second, want)
    with pytest.raises(ValueError, match="missing"):
        fz.load_state_dict({k: v for k, v in sd2.items() if k != next(iter(sd2))})


def _raw_photos(gpu):
    from _resize_ref import load_golden
    g = load_golden()
    imgs = [g["%d:raw" % k] for k in (1, 2, 3)]  # 150x170, 96x110, 200x140
    assert len({im.shape for im in imgs}) == 3
    t = np.linspace(0.0, 1.0, 68)
    base = np.stack([0.5 + 0.22 * np.cos(2 * np.pi * t * 3), 0.5 + 0.22 * np.sin(2 * np.pi * t * 5)], -1)
    lm = np.stack([base * [im.shape[1], im.shape[0]] for im in imgs]).astype(np.float32)
    return [torch.from_numpy(im).to(gpu) for im in imgs], torch.from_numpy(lm).to(gpu)


def test_frontalizer_raw_photos(gpu, det_sd):
    from DataAndDataset import FaceBatcher
    import tpgan_infer
    import tpgan_ops
    imgs, lm = _raw_photos(gpu)
    fz = tpgan_infer.Frontalizer(_generator(det_sd), device=gpu, compute_dtype=torch.bfloat16, max_batch=32)
    fb = FaceBatcher(gpu)
    with tpgan_ops.deterministic():
        whole = fz(imgs, lm)
        assert whole.dtype == torch.uint8 and tuple(whole.shape) == (3, 128, 128, 3)
        assert torch.equal(whole, fz.frontalize_batch(fb.from_raw(imgs, lm)))
        fz.max_batch = 2  # the same frozen model, two faces then one
        assert torch.equal(fz(imgs, lm), whole)
        gen = torch.Generator().manual_seed(5)
        zr = fz(imgs, lm, z=gen)
        gen.manual_seed(5)
        assert torch.equal(zr, fz(imgs, lm, z=torch.randn(3, 64, generator=gen)))
        assert not torch.equal(zr, whole)
    bad = lm.clone()
    bad[1, 40, 0] = float("nan")
    with pytest.raises(ValueError, match=r"\[1\]"):
        fz(imgs, bad)


def test_frontalizer_evaluate(gpu, det_sd):
    import tpgan_infer
    import tpgan_ops
    imgs, lm = _raw_photos(gpu)
    fz = tpgan_infer.Frontalizer(_generator(det_sd), device=gpu, compute_dtype=torch.bfloat16)
    with tpgan_ops.deterministic():
        r = fz.evaluate(imgs, lm, frontal=imgs)  # raw photos as the ground truth: resized on the device
        fake = r["fake_u8"]
        real = fz._batcher().resize(imgs, (128, 128))
        sse, ssim = tpgan_ops.image_metrics(fake, real)
        assert torch.equal(r["sse"], sse) and torch.equal(r["ssim"], ssim)
        want = 10.0 * np.log10(255.0 ** 2 * 128 * 128 * 3 / sse.cpu().numpy().astype(np.float64))
        assert r["psnr"].dtype == torch.float64 and r["psnr"].is_cuda
        np.testing.assert_allclose(r["psnr"].cpu().numpy(), want, rtol=1e-12)
        assert int(sse.min()) > 0
        same = fz.evaluate(imgs, lm, frontal=fake)
    assert torch.equal(same["fake_u8"], fake)
    assert same["sse"].tolist() == [0, 0, 0]
    assert torch.isinf(same["psnr"]).all() and (same["psnr"] > 0).all()
    assert float(same["ssim"].min()) >= 1 - 1e-5


def test_frontalizer_from_checkpoint(gpu, det_sd, e2e_inputs, existing_forward, tmp_path):
    import os
    import tpgan_infer
    import tpgan_ops
    _, batch, z = e2e_inputs
    bare = str(tmp_path / "generator.pth")
    torch.save(det_sd, bare)
    os.makedirs(str(tmp_path / "ckpt" / "G"))
    torch.save(det_sd, str(tmp_path / "ckpt" / "G" / "model_epoch_3.pth"))
    want = existing_forward(torch.bfloat16)
    for path, epoch in ((bare, None), (str(tmp_path / "ckpt"), 3), (str(tmp_path / "ckpt"), None)):
        fz = tpgan_infer.Frontalizer.from_checkpoint(path, epoch=epoch, device=gpu, compute_dtype=torch.bfloat16)
        with tpgan_ops.deterministic():
            assert torch.equal(fz.frontalize_batch(batch, z), want), (path, epoch)
