"""GPU: identity scoring -- tpgan_ops.l2_normalize / cosine_topk / cosine_pairs (tpg_identity.hip)
against the float64 restatement and its float32 error bound (tests/_identity_ref.py), and
tpgan_infer.IdentityScorer / Frontalizer.evaluate(identity=...) on top of them."""
import numpy as np
import pytest
import torch

import _identity_ref as R
from _cases import load_det

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
DTYPES = [torch.float32, torch.bfloat16, torch.float16]
DT_IDS = ["f32", "bf16", "f16"]
LAYOUTS = ["contiguous", "column_slice", "transposed"]


def _laid_out(vals, layout, gpu):
    """vals (a CPU [n, d] tensor of the final dtype) as a device tensor of the given layout."""
    n, d = vals.shape
    if layout == "contiguous":
        return vals.to(gpu).contiguous()
    if layout == "column_slice":
        buf = torch.full((n, d + 7), 3.0, dtype=vals.dtype, device=gpu)
        x = buf[:, 3:3 + d]
    else:
        x = torch.zeros(d, n, dtype=vals.dtype, device=gpu).t()
    x.copy_(vals)
    assert layout != "transposed" or x.stride() == (1, n)
    return x


def _gauss(seed, n, d, dtype=torch.float32):
    v = np.random.RandomState(seed).standard_normal((n, d)).astype(np.float32)
    return torch.from_numpy(v).to(dtype)


# ---------------------------------------------------------------- l2_normalize

NORM_SHAPES = [(1, 1), (5, 3), (17, 4), (33, 515), (8, 1280)]


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("shape", NORM_SHAPES, ids=lambda s: "%dx%d" % s)
def test_l2_normalize(gpu, shape, dtype, layout):
    import tpgan_ops
    n, d = shape
    vals = _gauss(11 + n + d, n, d, dtype)
    x = _laid_out(vals, layout, gpu)
    unit, norm = tpgan_ops.l2_normalize(x)
    again, _ = tpgan_ops.l2_normalize(x)
    ref, rn = R.normalize(vals.double().numpy())  # float64 of the input as `dtype` holds it
    got = unit.cpu().numpy().astype(np.float64)
    assert unit.dtype == torch.float32 and tuple(unit.shape) == (n, d) and tuple(norm.shape) == (n,)
    err = np.abs(got - ref)
    lim = (d + 8) * U * np.abs(ref)
    print("l2_normalize %s %s %s: max err / bound %.3f" % (shape, dtype, layout, float((err / np.maximum(lim, 1e-300)).max())))
    assert (err <= lim).all()
    np.testing.assert_allclose(norm.cpu().numpy(), rn, rtol=(d + 8) * U)
    dpad = (d + 3) // 4 * 4
    padded = unit._base
    assert tuple(padded.shape) == (n, dpad) and padded.is_contiguous()
    assert not padded[:, d:].any()  # pad columns exactly 0
    assert torch.equal(unit, again)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("shape", [(5, 3), (33, 515)], ids=lambda s: "%dx%d" % s)
def test_l2_normalize_bad_rows(gpu, shape, dtype):
    import tpgan_ops
    n, d = shape
    vals = _gauss(5, n, d, dtype)
    vals[1] = 0
    vals[2, d - 1] = float("nan")
    vals[4, 0] = float("-inf")
    x = vals.to(gpu)
    unit, norm, status = tpgan_ops.l2_normalize(x, check=False)
    want = [0] * n
    want[1] = want[2] = want[4] = 1
    assert status.dtype == torch.int32 and status.tolist() == want
    assert not unit[[1, 2, 4]].any() and not unit._base[[1, 2, 4]].any()
    good = [i for i in range(n) if not want[i]]
    ref, _ = R.normalize(vals[good].double().numpy())
    assert (np.abs(unit[good].cpu().numpy() - ref) <= (d + 8) * U * np.abs(ref)).all()
    with pytest.raises(ValueError, match=r"\[1, 2, 4\]"):
        tpgan_ops.l2_normalize(x)


# ---------------------------------------------------------------- cosine_topk

_TOPK_CACHE = {}


def _topk_case(gpu, P, G, D, seed=None):
    """Gaussian probes and gallery, their device unit rows (tpg_l2_normalize) and the float64
    similarity and bound of the same float32 inputs; computed once per shape."""
    key = (P, G, D, seed)
    if key not in _TOPK_CACHE:
        import tpgan_ops
        rs = np.random.RandomState(1000 + P + G + D if seed is None else seed)
        g = rs.standard_normal((G, D)).astype(np.float32)  # (gallery first, then probes)
        p = rs.standard_normal((P, D)).astype(np.float32)
        pu, _ = R.normalize(p)
        gu, _ = R.normalize(g)
        dp, _ = tpgan_ops.l2_normalize(torch.from_numpy(p).to(gpu))
        dg, _ = tpgan_ops.l2_normalize(torch.from_numpy(g).to(gpu))
        _TOPK_CACHE[key] = {"p": dp, "g": dg, "s64": R.similarity(pu, gu), "bound": R.bound(pu, gu)}
    return _TOPK_CACHE[key]


TOPK_SHAPES = [(1, 1, 1, 1), (1, 5, 3, 5), (17, 129, 4, 8), (33, 1031, 515, 8), (64, 128, 512, 8)]


@pytest.mark.parametrize("gchunk", [0, 16])
@pytest.mark.parametrize("shape", TOPK_SHAPES, ids=lambda s: "P%d_G%d_D%d_k%d" % s)
def test_cosine_topk_within_bound(gpu, shape, gchunk):
    import tpgan_ops
    P, G, D, k = shape
    c = _topk_case(gpu, P, G, D)
    idx, score = tpgan_ops.cosine_topk(c["p"], c["g"], k=k, gchunk=gchunk)
    assert idx.dtype == torch.int32 and score.dtype == torch.float32 and tuple(idx.shape) == tuple(score.shape) == (P, k)
    idx, score = idx.cpu().numpy(), score.cpu().numpy().astype(np.float64)
    s64, bound = c["s64"], c["bound"]
    best = -np.sort(-s64, axis=1)[:, :k]          # the r-th best float64 score
    slack = 2 * bound.max(axis=1)
    worst = 0.0
    for p in range(P):
        assert ((idx[p] >= 0) & (idx[p] < G)).all() and len(set(idx[p].tolist())) == k, (p, idx[p])
        assert (np.diff(score[p]) <= 0).all(), (p, score[p])
        err = np.abs(score[p] - s64[p, idx[p]])
        worst = max(worst, float((err / bound[p, idx[p]]).max()))
        assert (err <= bound[p, idx[p]]).all(), (p, err, bound[p, idx[p]])
        assert (s64[p, idx[p]] >= best[p] - slack[p]).all(), (p, s64[p, idx[p]], best[p])
    print("cosine_topk %s gchunk %d: max |score - s64| / bound %.3f" % (shape, gchunk, worst))


@pytest.mark.parametrize("gchunk", [0, 16, 48])
def test_cosine_topk_exact_indices(gpu, gchunk):
    """(65, 300, 64, 5) from RandomState(434): the smallest gap between neighbouring top-6 float64
    scores is 2.2x the sum of their two bounds (largest bound 1.0e-5), so an exact-f32 search must
    return the reference's indices; 16-bit operands (error ~1e-4) would not."""
    import tpgan_ops
    c = _topk_case(gpu, 65, 300, 64, seed=434)
    want, wscore = R.topk(c["s64"], 5)
    top6 = -np.sort(-c["s64"], axis=1)[:, :6]
    order = np.argsort(-c["s64"], axis=1)[:, :6]
    b6 = np.take_along_axis(c["bound"], order, axis=1)
    gap = ((top6[:, :-1] - top6[:, 1:]) / (b6[:, :-1] + b6[:, 1:])).min()
    print("smallest top-6 gap / sum of bounds %.2f, largest bound %.2e" % (gap, c["bound"].max()))
    assert gap > 1.0  # (the case decides every rank)
    idx, score = tpgan_ops.cosine_topk(c["p"], c["g"], k=5, gchunk=gchunk)
    np.testing.assert_array_equal(idx.cpu().numpy(), want)
    assert np.abs(score.cpu().numpy() - wscore).max() <= c["bound"].max()


def test_cosine_topk_planted(gpu):
    import tpgan_ops
    rs = np.random.RandomState(77)
    G, D, P = 257, 1280, 16
    g = rs.standard_normal((G, D)).astype(np.float32)
    planted = rs.permutation(G)[:P]
    planted[0], planted[1] = 256, 0  # the last row (alone in its tile) and the first
    p = (g[planted] + 0.3 * rs.standard_normal((P, D))).astype(np.float32)
    dg, _ = tpgan_ops.l2_normalize(torch.from_numpy(g).to(gpu))
    dp, _ = tpgan_ops.l2_normalize(torch.from_numpy(p).to(gpu))
    for gchunk in (0, 64):
        idx, score = tpgan_ops.cosine_topk(dp, dg, k=1, gchunk=gchunk)
        assert idx[:, 0].tolist() == planted.tolist()
        assert float(score.min()) > 0.9


def test_cosine_topk_semantics(gpu):
    import tpgan_ops
    rs = np.random.RandomState(9)
    G, D, P = 300, 24, 6
    g = rs.standard_normal((G, D)).astype(np.float32)
    g[200] = g[5]      # duplicates in different tiles and lane halves
    g[37] = g[33]      # and inside one tile
    p = rs.standard_normal((P, D)).astype(np.float32)
    p[0], p[1] = g[5], g[33]
    dg, _ = tpgan_ops.l2_normalize(torch.from_numpy(g).to(gpu))
    dp, _ = tpgan_ops.l2_normalize(torch.from_numpy(p).to(gpu))
    pu, _ = R.normalize(p)
    gu, _ = R.normalize(g)
    s64 = R.similarity(pu, gu)
    # (identical rows must tie in the reference too, whatever its summation order gave)
    s64[:, 200], s64[:, 37] = s64[:, 5], s64[:, 33]
    for gchunk in (0, 16, 100):
        idx, score = tpgan_ops.cosine_topk(dp, dg, k=4, gchunk=gchunk)
        assert idx[0, :2].tolist() == [5, 200] and idx[1, :2].tolist() == [33, 37]
        assert score[0, 0].item() == score[0, 1].item() and score[1, 0].item() == score[1, 1].item()
        np.testing.assert_array_equal(idx.cpu().numpy(), R.topk(s64, 4)[0])
        # skip removes exactly that index: the duplicate moves up, nothing else changes
        skip = torch.tensor([5, 37, -1, 0, 299, 1000], dtype=torch.int32, device=gpu)
        sidx, sscore = tpgan_ops.cosine_topk(dp, dg, k=4, skip=skip, gchunk=gchunk)
        np.testing.assert_array_equal(sidx.cpu().numpy(), R.topk(s64, 4, skip=skip.tolist())[0])
        assert sidx[0, 0].item() == 200 and sidx[1, :2].tolist()[0] == 33 and 37 not in sidx[1].tolist()
        assert torch.equal(sidx[2], idx[2]) and torch.equal(sscore[2], score[2])
        # two runs are bit-identical, and the scores do not depend on the chunking
        idx2, score2 = tpgan_ops.cosine_topk(dp, dg, k=4, gchunk=gchunk)
        assert torch.equal(idx, idx2) and torch.equal(score, score2)
        ref_idx, ref_score = tpgan_ops.cosine_topk(dp, dg, k=4, gchunk=0)
        assert torch.equal(idx, ref_idx) and torch.equal(score, ref_score)
    # k > G, and k > eligible rows: -1 / -inf tails
    small = dg[:3]
    ninf = float("-inf")
    for gchunk in (0, 16):
        idx, score = tpgan_ops.cosine_topk(dp, small, k=8, gchunk=gchunk)
        want = R.topk(s64[:, :3], 8)[0]
        np.testing.assert_array_equal(idx.cpu().numpy(), want)
        assert (idx[:, 3:] == -1).all() and (score[:, 3:] == ninf).all() and torch.isfinite(score[:, :3]).all()
        skip = torch.tensor([0, 1, 2, -1, 0, 1], dtype=torch.int32, device=gpu)
        idx, score = tpgan_ops.cosine_topk(dp, small, k=3, skip=skip, gchunk=gchunk)
        np.testing.assert_array_equal(idx.cpu().numpy(), R.topk(s64[:, :3], 3, skip=skip.tolist())[0])
        assert idx[0, 2].item() == -1 and score[0, 2].item() == ninf and idx[3, 2].item() >= 0
    # a [n, d] tensor that is not l2_normalize's own view is padded by a copy: same answer
    a, b = tpgan_ops.cosine_topk(dp.clone(), dg.clone(), k=4)
    assert torch.equal(a, ref_idx) and torch.equal(b, ref_score)
    with pytest.raises(ValueError, match="1..8"):
        tpgan_ops.cosine_topk(dp, dg, k=9)
    with pytest.raises(ValueError, match="gchunk"):
        tpgan_ops.cosine_topk(dp, dg, gchunk=8)
    with pytest.raises(ValueError, match="skip"):
        tpgan_ops.cosine_topk(dp, dg, skip=torch.zeros(P, dtype=torch.int64, device=gpu))


def test_cosine_topk_graph_replay(gpu):
    """One stream, no parallel branches: the search and the merge captured and replayed once."""
    import tpgan_ops
    c = _topk_case(gpu, 33, 1031, 515)
    skip = torch.arange(33, dtype=torch.int32, device=gpu)
    eager = tpgan_ops.cosine_topk(c["p"], c["g"], k=8, skip=skip, gchunk=16)  # (sizes the workspace)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = tpgan_ops.cosine_topk(c["p"], c["g"], k=8, skip=skip, gchunk=16)
    out[0].fill_(-7)
    out[1].zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out[0], eager[0]) and torch.equal(out[1], eager[1])


# ---------------------------------------------------------------- cosine_pairs

@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("shape", NORM_SHAPES, ids=lambda s: "%dx%d" % s)
def test_cosine_pairs(gpu, shape, dtype, layout):
    import tpgan_ops
    n, d = shape
    va, vb = _gauss(21 + n + d, n, d, dtype), _gauss(22 + n + d, n, d, dtype)
    a, b = _laid_out(va, layout, gpu), _laid_out(vb, "contiguous", gpu)
    cos = tpgan_ops.cosine_pairs(a, b)
    au, _ = R.normalize(va.double().numpy())
    bu, _ = R.normalize(vb.double().numpy())
    ref, lim = (au * bu).sum(1), R.pair_bound(au, bu)
    err = np.abs(cos.cpu().numpy().astype(np.float64) - ref)
    print("cosine_pairs %s %s %s: max err / bound %.3f" % (shape, dtype, layout, float((err / lim).max())))
    assert cos.dtype == torch.float32 and tuple(cos.shape) == (n,)
    assert (err <= lim).all()
    assert torch.equal(cos, tpgan_ops.cosine_pairs(a, b))
    # mixed dtypes: b as float32 of the same values
    mixed = tpgan_ops.cosine_pairs(a, b.float())
    assert (np.abs(mixed.cpu().numpy().astype(np.float64) - ref) <= lim).all()


def test_cosine_pairs_bad_rows(gpu):
    import tpgan_ops
    a, b = _gauss(1, 6, 37), _gauss(2, 6, 37)
    a[1] = 0
    b[3, 36] = float("nan")
    a[4, 0] = float("inf")
    cos, status = tpgan_ops.cosine_pairs(a.to(gpu), b.to(gpu), check=False)
    assert status.tolist() == [0, 1, 0, 1, 1, 0]
    assert cos[[1, 3, 4]].tolist() == [0.0, 0.0, 0.0] and torch.isfinite(cos).all() and cos[0].item() != 0
    with pytest.raises(ValueError, match=r"\[1, 3, 4\]"):
        tpgan_ops.cosine_pairs(a.to(gpu), b.to(gpu))
    with pytest.raises(ValueError, match="must match"):
        tpgan_ops.cosine_pairs(a.to(gpu), b[:5].to(gpu))


# ---------------------------------------------------------------- IdentityScorer

@pytest.fixture(autouse=True)
def _no_autotune():
    import tpgan_ops
    old = tpgan_ops.AUTOTUNE["enabled"]
    tpgan_ops.AUTOTUNE["enabled"] = False
    yield
    tpgan_ops.AUTOTUNE["enabled"] = old


def _extractor():
    """ResNet-18 back-end with deterministic weights: the values _cases.load_det gives every weight
    and bias (oracle.det_init.det_param by state_dict name), and det_init's well-conditioned
    BatchNorm states, where load_det's 0.1 u would make a running variance negative and cannot fill
    the 0-dim num_batches_tracked."""
    import FeatureExtract as FE
    from oracle.det_init import det_module_state
    ext = FE.FeatureExtractModel("resnet", 10)
    sd = ext.state_dict()
    ext.load_state_dict({k: torch.from_numpy(np.asarray(v)).to(sd[k].dtype)
                         for k, v in det_module_state(ext, "ids/").items()})
    return ext


def _faces(gpu, seed, B=3):
    rs = np.random.RandomState(seed)
    # smooth blobs rather than white noise, so that the faces differ in more than texture
    yy, xx = np.mgrid[0:128, 0:128] / 127.0
    out = np.empty((B, 128, 128, 3), np.uint8)
    for b in range(B):
        f = rs.uniform(1, 5, (3, 2))
        ph = rs.uniform(0, 6.28, (3, 2))
        for ch in range(3):
            v = np.sin(f[ch, 0] * 3 * xx + ph[ch, 0]) * np.cos(f[ch, 1] * 3 * yy + ph[ch, 1])
            out[b, :, :, ch] = np.clip(127.5 + 100 * v + rs.standard_normal((128, 128)) * 8, 0, 255).astype(np.uint8)
    return torch.from_numpy(out).to(gpu)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_identity_scorer(gpu, dtype):
    from DataAndDataset import FaceBatcher
    import tpgan_infer
    import tpgan_ops
    scorer = tpgan_infer.IdentityScorer(_extractor(), device=gpu, compute_dtype=dtype)
    assert not scorer.extractor.training and not any(p.requires_grad for p in scorer.extractor.parameters())
    fa, fb = _faces(gpu, 1), _faces(gpu, 2)
    with tpgan_ops.deterministic():
        emb = scorer.embed(fa)
        # the extractor's own last feature, run the existing way
        with torch.no_grad(), tpgan_ops.compute_dtype(dtype):
            feat = scorer.extractor.extract_features(FaceBatcher(gpu).normalize(fa))[-1]
        feat = feat.reshape(3, -1)
        D = feat.shape[1]
        assert emb.dtype == torch.float32 and tuple(emb.shape) == (3, D) and D == 512
        ref = torch.nn.functional.normalize(feat.double(), dim=1).cpu().numpy()
        err = np.abs(emb.cpu().numpy().astype(np.float64) - ref)
        assert (err <= (D + 8) * U * np.abs(ref)).all(), float(err.max())
        assert (np.abs(np.linalg.norm(emb.cpu().numpy().astype(np.float64), axis=1) - 1.0) <= 1e-6).all()
        scorer.max_batch = 2  # two faces, then one: the same embeddings
        assert torch.equal(scorer.embed(fa), emb)
        scorer.max_batch = 32

        first = scorer.enroll(fa, [10, 11, 12])
        second = scorer.enroll(fb, torch.tensor([20, 21, 22]))
        assert first.tolist() == [0, 1, 2] and second.tolist() == [3, 4, 5] and scorer.size == 6
        assert tuple(scorer.gallery.shape) == (6, D) and scorer.labels.tolist() == [10, 11, 12, 20, 21, 22]
        probes = torch.cat([fb, fa])
        res = scorer.identify(probes, k=3)
    assert res["label"][:, 0].tolist() == [20, 21, 22, 10, 11, 12]
    assert res["idx"][:, 0].tolist() == [3, 4, 5, 0, 1, 2]
    assert float(res["score"][:, 0].min()) >= 1 - 1e-5
    assert res["label"].dtype == torch.int64 and tuple(res["label"].shape) == (6, 3)
    assert torch.equal(res["label"], scorer.labels[res["idx"].long()])
    cmc = scorer.cmc([20, 21, 22, 10, 11, 12], res)
    assert cmc.dtype == torch.float64 and cmc.tolist() == [1.0, 1.0, 1.0]
    # embeddings in, the probe's own enrolment skipped: the best match is somebody else
    skip = torch.tensor([3, 4, 5, 0, 1, 2], dtype=torch.int32, device=gpu)
    with tpgan_ops.deterministic():
        other = scorer.identify(scorer.embed(probes), k=6, skip=skip)
    assert (other["idx"][:, 0] != skip).all() and (other["idx"][:, 5] == -1).all() and (other["label"][:, 5] == -1).all()
    assert torch.equal(other["idx"][:, :2], torch.stack([res["idx"][:, 1], res["idx"][:, 2]], 1))
    assert scorer.cmc([20, 21, 22, 10, 11, 12], other).tolist() == [0.0] * 6
    scorer.clear()
    assert scorer.size == 0
    with pytest.raises(ValueError, match="empty"):
        scorer.identify(fa)


def _raw_photos(gpu):
    from _resize_ref import load_golden
    g = load_golden()
    imgs = [g["%d:raw" % k] for k in (1, 2, 3)]
    t = np.linspace(0.0, 1.0, 68)
    base = np.stack([0.5 + 0.22 * np.cos(2 * np.pi * t * 3), 0.5 + 0.22 * np.sin(2 * np.pi * t * 5)], -1)
    lm = np.stack([base * [im.shape[1], im.shape[0]] for im in imgs]).astype(np.float32)
    return [torch.from_numpy(im).to(gpu) for im in imgs], torch.from_numpy(lm).to(gpu)


def test_frontalizer_evaluate_identity(gpu):
    import D_and_G_model as DG
    import tpgan_infer
    import tpgan_ops
    G = DG.Generator(64, 347, use_batchnorm=False)
    load_det(G, "G/", torch.float32)
    fz = tpgan_infer.Frontalizer(G, device=gpu, compute_dtype=torch.bfloat16)
    scorer = tpgan_infer.IdentityScorer(_extractor(), device=gpu, compute_dtype=torch.bfloat16)
    imgs, lm = _raw_photos(gpu)
    with tpgan_ops.deterministic():
        plain = fz.evaluate(imgs, lm, frontal=imgs)
        r = fz.evaluate(imgs, lm, frontal=imgs, identity=scorer)
        real = fz._batcher().resize(imgs, (128, 128))
        want = tpgan_ops.cosine_pairs(scorer.embed(r["fake_u8"]), scorer.embed(real))
    assert set(plain) == {"fake_u8", "sse", "psnr", "ssim"}
    assert set(r) == set(plain) | {"id_cos"}
    for k in plain:
        assert torch.equal(plain[k], r[k]), k
    assert r["id_cos"].dtype == torch.float32 and tuple(r["id_cos"].shape) == (3,)
    assert torch.equal(r["id_cos"], want)
    assert torch.isfinite(r["id_cos"]).all() and float(r["id_cos"].abs().max()) <= 1 + 1e-6
    with pytest.raises(ValueError, match="IdentityScorer"):
        fz.evaluate(imgs, lm, frontal=imgs, identity=object())
