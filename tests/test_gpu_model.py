"""End-to-end GPU parity: the product's Generator + Discriminator (fp32 MFMA path) on
the reference's own B=2 golden run (tests/golden/e2e_golden.npz: outputs of
D_and_G_model.Generator/Discriminator with R1-R3 and deterministic weights, float64),
including per-parameter gradient summaries for all 348 parameter tensors."""
import numpy as np
import pytest
import torch

from _cases import golden, load_det, rel

pytestmark = pytest.mark.gpu

G_OUT = ["I128_fake", "encoder_predict", "fused_local_fake", "le_fake", "re_fake", "nose_fake", "mouth_fake",
         "fused_local_real"]
INS = ["I128", "left_eye", "right_eye", "nose", "mouth", "z"]


def _e2e(gpu, flat):
    import D_and_G_model as DG
    E = golden("e2e_golden.npz")
    G = DG.Generator(64, 347, use_batchnorm=False)
    D = DG.Discriminator()
    load_det(G, "G/", torch.float32)
    load_det(D, "D/", torch.float32)
    G, D = G.to(gpu), D.to(gpu)
    if flat:  # the train step's layout: params/grads are views of flat buffers, fused dW/db accumulation
        import tpgan_train
        G._flat = tpgan_train.FlatParams(G, gpu)
        D._flat = tpgan_train.FlatParams(D, gpu)
    ins = {k: torch.from_numpy(E["in:" + k]).float().to(gpu).requires_grad_(True) for k in INS}
    outs = G(ins["I128"], ins["left_eye"], ins["right_eye"], ins["nose"], ins["mouth"], ins["z"], False)
    loss = 0
    from oracle.det_init import det_uniform
    for name, o in zip(G_OUT, outs):
        if name == "fused_local_real":
            continue
        pr = torch.from_numpy(det_uniform("proj/e2e/" + name, o.numel())).reshape(o.shape).float().to(gpu)
        loss = loss + (o * pr).sum()
    d_fake = D(outs[0])
    pr = torch.from_numpy(det_uniform("proj/e2e/d_fake", d_fake.numel())).reshape(d_fake.shape).float().to(gpu)
    loss = loss + (d_fake * pr).sum()
    loss.backward()
    torch.cuda.synchronize()
    return E, G, D, ins, outs, d_fake


@pytest.fixture(scope="module")
def e2e(gpu):
    return _e2e(gpu, False)


@pytest.fixture(scope="module")
def e2e_flat(gpu):
    return _e2e(gpu, True)


def test_generator_outputs(e2e):
    E, G, D, ins, outs, d_fake = e2e
    for name, o in zip(G_OUT, outs):
        ref = E["out:" + name]
        assert tuple(o.shape) == ref.shape, name
        assert rel(o.detach().cpu(), ref) < 1e-3, name
    assert rel(d_fake.detach().cpu(), E["out:d_fake"]) < 1e-3


def test_input_grads(e2e):
    # per-tensor bound 1e-2: the aten CPU fp32 path itself lands at
    # 1.1e-3 (I128) / 1.2e-3 (z) from the float64 reference here, from LeakyReLU kinks
    # and LocalFuser / maxout near-ties that flip with summation order.
    E, G, D, ins, outs, d_fake = e2e
    for k in INS:
        if "din:" + k in E.files:
            assert rel(ins[k].grad.cpu(), E["din:" + k]) < 1e-2, k


def _check_gsum(E, prefix, model):
    from oracle.det_init import det_uniform
    allg, allr = [], []
    worst = 0.0
    for k, p in model.named_parameters():
        ref = E["gsum:%s/%s" % (prefix, k)]
        g = p.grad.detach().double().reshape(-1).cpu().numpy()
        u = det_uniform("sample/%s/%s" % (prefix, k), 16)
        idx = np.floor((u + 1.0) * 0.5 * g.size).astype(np.int64).clip(0, g.size - 1)
        norm = np.sqrt((g * g).sum())
        worst = max(worst, abs(norm - ref[0]) / max(ref[0], 1e-30))
        allg.append(g[idx])
        allr.append(ref[2:])
    # per-tensor norm within 1e-2, concatenated samples within 1e-3
    assert worst < 1e-2, worst
    assert rel(np.concatenate(allg), np.concatenate(allr)) < 1e-3


def test_generator_param_grads(e2e):
    E, G, D, ins, outs, d_fake = e2e
    _check_gsum(E, "G", G)


def test_discriminator_param_grads(e2e):
    E, G, D, ins, outs, d_fake = e2e
    _check_gsum(E, "D", D)


def test_discriminator_real(e2e, gpu):
    E, G, D, ins, outs, d_fake = e2e
    with torch.no_grad():
        d = D(ins["I128"].detach())
    assert rel(d.cpu(), E["out:d_real"]) < 1e-3


def test_fused_grad_accumulation(e2e_flat):
    """Flat-buffer models (FlatParams: HIP dW / db added in place into the flat gradient)
    reproduce the reference gradients, and a second backward accumulates (+=)."""
    E, G, D, ins, outs, d_fake = e2e_flat
    _check_gsum(E, "G", G)
    _check_gsum(E, "D", D)
    assert all(p.grad.data_ptr() >= G._flat.grad.data_ptr() for p in G.parameters())
    g1 = D._flat.grad.clone()
    D._flat.grad.zero_()
    D(ins["I128"].detach()).sum().backward()
    first = D._flat.grad.clone()
    D(ins["I128"].detach()).sum().backward()
    torch.cuda.synchronize()
    assert rel(D._flat.grad.cpu(), 2 * first.cpu()) < 1e-6
    assert g1.abs().sum() > 0


# ---- bf16: the dtype the benchmark runs (round-1 verdict: no bf16 end-to-end parity test) ----
def _grad_metrics(E, prefix, named_grads):
    """(worst per-tensor norm error, concatenated 16-sample error) of a list of
    (name, gradient) against the golden summaries, as _check_gsum measures them."""
    from oracle.det_init import det_uniform
    allg, allr = [], []
    worst = 0.0
    for k, gr in named_grads:
        ref = E["gsum:%s/%s" % (prefix, k)]
        g = np.asarray(gr, np.float64).reshape(-1)
        u = det_uniform("sample/%s/%s" % (prefix, k), 16)
        idx = np.floor((u + 1.0) * 0.5 * g.size).astype(np.int64).clip(0, g.size - 1)
        if ref[0] > 1e-20:
            worst = max(worst, abs(np.sqrt((g * g).sum()) - ref[0]) / ref[0])
        allg.append(g[idx])
        allr.append(ref[2:])
    return worst, rel(np.concatenate(allg), np.concatenate(allr))


def _oracle_bf16_floor(E):
    """The same projected loss through the CPU oracle in bfloat16 (aten CPU bf16 convs:
    fp32 accumulation, bf16 activations, as the HIP path): its distance to the float64
    golden is what bf16 storage alone costs, the floor the bf16 bounds are set from."""
    from oracle import tpgan_oracle as O
    from oracle.det_init import det_uniform
    PG, PD = O.make_params(torch.bfloat16)
    for p in list(PG.values()) + list(PD.values()):
        p.requires_grad_(True)
    ins = {k: torch.from_numpy(E["in:" + k]).to(torch.bfloat16) for k in INS}
    outs = O.generator(PG, ins["I128"], ins["left_eye"], ins["right_eye"], ins["nose"], ins["mouth"], ins["z"])
    d_fake = O.discriminator(PD, outs[0])
    loss = 0
    for name, o in zip(G_OUT, outs):
        if name == "fused_local_real":
            continue
        pr = torch.from_numpy(det_uniform("proj/e2e/" + name, o.numel())).reshape(o.shape).float()
        loss = loss + (o.float() * pr).sum()
    pr = torch.from_numpy(det_uniform("proj/e2e/d_fake", d_fake.numel())).reshape(d_fake.shape).float()
    loss = loss + (d_fake.float() * pr).sum()
    loss.backward()
    fwd = {name: rel(o.detach().float(), E["out:" + name]) for name, o in zip(G_OUT, outs)}
    gG = _grad_metrics(E, "G", [(k, p.grad.float().numpy()) for k, p in PG.items()])
    gD = _grad_metrics(E, "D", [(k, p.grad.float().numpy()) for k, p in PD.items()])
    return fwd, gG, gD


@pytest.fixture(scope="module")
def e2e_bf16(gpu):
    import tpgan_ops
    with tpgan_ops.compute_dtype(torch.bfloat16):
        return _e2e(gpu, True)


def test_bf16_generator_discriminator_vs_golden(e2e_bf16):
    """bf16 MFMA path (the benchmark's dtype, flat-buffer train-step layout) on the
    reference-run golden: every G output and D(fake) within SURVEY.md §8c's documented bf16
    bound 2e-2; G and D gradients within 3x of the bf16 CPU oracle's own distance to the
    float64 golden (per-tensor norms and the concatenated samples; never tighter than 2e-2)."""
    E, G, D, ins, outs, d_fake = e2e_bf16
    fwd_floor, gG_floor, gD_floor = _oracle_bf16_floor(E)
    for name, o in zip(G_OUT, outs):
        assert o.dtype == torch.bfloat16
        err = rel(o.detach().float().cpu(), E["out:" + name])
        assert err < 2e-2, (name, err, fwd_floor[name])
    assert rel(d_fake.detach().float().cpu(), E["out:d_fake"]) < 2e-2
    for prefix, model, (fw, fs) in (("G", G, gG_floor), ("D", D, gD_floor)):
        worst, samp = _grad_metrics(E, prefix, [(k, p.grad.detach().double().cpu().numpy())
                                                for k, p in model.named_parameters()])
        assert worst < max(3 * fw, 2e-2), (prefix, worst, fw)
        assert samp < max(3 * fs, 2e-2), (prefix, samp, fs)


# ---- BASELINE configs[0]: global pathway only + D, B=4 ----------
def test_config1_global_pathway_and_d_vs_oracle(gpu):
    """GlobalPathway with zero local inputs (local_fake_image = 0, local_feature = 0) + D on
    its output, B=4, fp32 MFMA path; loss = mean D(fake) + L1(fake, frontal).  Outputs, the
    loss and every G/D parameter gradient against the float64 CPU oracle
    (D_and_G_model.py:161-329, 409-435): forward 1e-3, concatenated gradients 1e-3 (or 3x the
    fp32 CPU floor), per tensor 1e-2."""
    import D_and_G_model as DG
    import tpgan_ops
    from oracle import tpgan_oracle as O
    from oracle.det_init import det_input
    B = 4
    G = DG.Generator(64, 347, use_batchnorm=False)
    D = DG.Discriminator()
    load_det(G, "G/", torch.float32)
    load_det(D, "D/", torch.float32)
    gp, D = G.global_pathway.to(gpu), D.to(gpu)
    I128 = torch.from_numpy(det_input("cfg1/I128", (B, 3, 128, 128)))
    z = torch.from_numpy(det_input("cfg1/z", (B, 64)))
    front = torch.from_numpy(det_input("cfg1/frontal", (B, 3, 128, 128)))
    with tpgan_ops.deterministic():
        fake, fc2 = gp(I128.float().to(gpu), torch.zeros(B, 3, 128, 128, device=gpu),
                       torch.zeros(B, 64, 128, 128, device=gpu), z.float().to(gpu))
        d = D(fake)
        loss = d.float().mean() + (fake.float() - front.float().to(gpu)).abs().mean()
        loss.backward()
        torch.cuda.synchronize()

    def ref(dtype):
        PG, PD = O.make_params(dtype)
        PG = {k: v for k, v in PG.items() if k.startswith("global_pathway.")}
        for p in list(PG.values()) + list(PD.values()):
            p.requires_grad_(True)
        f, c2 = O.global_only(PG, I128.to(dtype), z.to(dtype))
        dd = O.discriminator(PD, f)
        lo = dd.mean() + (f - front.to(dtype)).abs().mean()
        lo.backward()
        return f, c2, dd, lo, PG, PD

    f64, c264, d64, l64, PG, PD = ref(torch.float64)
    _, _, _, _, PG32, PD32 = ref(torch.float32)
    assert rel(fake.detach().cpu(), f64.detach()) < 1e-3
    assert rel(fc2.detach().cpu(), c264.detach()) < 1e-3
    assert rel(d.detach().cpu(), d64.detach()) < 1e-3
    assert abs(float(loss) - float(l64)) <= 1e-3 * abs(float(l64))
    for model, P, P32, pre in ((gp, PG, PG32, "global_pathway."), (D, PD, PD32, "")):
        names = [k for k, _ in model.named_parameters()]
        mine = torch.cat([p.grad.detach().double().cpu().reshape(-1) for p in model.parameters()])
        want = torch.cat([P[pre + k].grad.reshape(-1) for k in names])
        floor = rel(torch.cat([P32[pre + k].grad.double().reshape(-1) for k in names]), want)
        assert rel(mine, want) < max(1e-3, 3 * floor), (pre, rel(mine, want), floor)
        for k, p in model.named_parameters():
            gr = P[pre + k].grad
            if float(gr.norm()) > 0:
                assert rel(p.grad.detach().cpu(), gr) < 1e-2, k


# ---- BASELINE configs[4]: G generalised to 256x256 (build extension; the reference is
# 128-only, so parity here is against the oracle's restatement with the same extension,
# oracle.tpgan_oracle.fuser_pads / make_params(img_size=256)), and the fp16 MFMA path ----
def _g256(gpu, dtype, B=1):
    import D_and_G_model as DG
    import tpgan_ops
    from oracle.det_init import det_input, det_uniform
    G = DG.Generator(64, 347, use_batchnorm=False, img_size=256)
    D = DG.Discriminator()
    load_det(G, "G/", torch.float32)
    load_det(D, "D/", torch.float32)
    G, D = G.to(gpu), D.to(gpu)
    shapes = {"I128": (3, 256, 256), "left_eye": (3, 80, 80), "right_eye": (3, 80, 80), "nose": (3, 64, 80),
              "mouth": (3, 64, 96), "z": (64,)}
    ins = {k: torch.from_numpy(det_input("g256/" + k, (B,) + s)) for k, s in shapes.items()}
    gi = {k: v.float().to(gpu).requires_grad_(k == "I128") for k, v in ins.items()}
    with tpgan_ops.compute_dtype(dtype):
        outs = G(gi["I128"], gi["left_eye"], gi["right_eye"], gi["nose"], gi["mouth"], gi["z"], False)
        d = D(outs[0])
    loss = 0
    for name, o in zip(G_OUT, outs):
        if name == "fused_local_real":
            continue
        pr = torch.from_numpy(det_uniform("proj/g256/" + name, o.numel())).reshape(o.shape).float().to(gpu)
        loss = loss + (o.float() * pr).sum()
    pr = torch.from_numpy(det_uniform("proj/g256/d", d.numel())).reshape(d.shape).float().to(gpu)
    loss = loss + (d.float() * pr).sum()
    loss.backward()
    torch.cuda.synchronize()
    return ins, G, D, outs, d, gi


def test_generator_256_vs_oracle(gpu):
    """G at 256x256 (LocalFuser canvas 256, fc1 on 16x16x512, deconv_8 16x16) + D, fp32 MFMA
    path, against the float64 oracle: outputs 1e-3, I128 and concatenated parameter gradients
    1e-3 (or 3x the oracle's own fp32 floor)."""
    from oracle import tpgan_oracle as O
    from oracle.det_init import det_uniform
    ins, G, D, outs, d, gi = _g256(gpu, torch.float32)
    assert tuple(outs[0].shape) == (1, 3, 256, 256) and tuple(d.shape) == (1, 1, 8, 8)

    def ref(dt):
        PG, PD = O.make_params(dt, img_size=256)
        for p in list(PG.values()) + list(PD.values()):
            p.requires_grad_(True)
        xi = {k: v.detach().clone().to(dt).requires_grad_(k == "I128") for k, v in ins.items()}
        ro = O.generator(PG, xi["I128"], xi["left_eye"], xi["right_eye"], xi["nose"], xi["mouth"], xi["z"])
        rd = O.discriminator(PD, ro[0])
        lo = 0
        for name, o in zip(G_OUT, ro):
            if name == "fused_local_real":
                continue
            lo = lo + (o * torch.from_numpy(det_uniform("proj/g256/" + name, o.numel())).reshape(o.shape).to(dt)).sum()
        lo = lo + (rd * torch.from_numpy(det_uniform("proj/g256/d", rd.numel())).reshape(rd.shape).to(dt)).sum()
        lo.backward()
        return ro, rd, xi, PG, PD

    ro, rd, xi, PG, PD = ref(torch.float64)
    _, _, xi32, PG32, PD32 = ref(torch.float32)
    for name, o, r in zip(G_OUT, outs, ro):
        assert rel(o.detach().cpu(), r.detach()) < 1e-3, name
    assert rel(d.detach().cpu(), rd.detach()) < 1e-3
    assert rel(gi["I128"].grad.cpu(), xi["I128"].grad) < max(1e-3, 3 * rel(xi32["I128"].grad.double(),
                                                                           xi["I128"].grad))
    for model, P, P32 in ((G, PG, PG32), (D, PD, PD32)):
        names = [k for k, _ in model.named_parameters()]
        mine = torch.cat([p.grad.detach().double().cpu().reshape(-1) for p in model.parameters()])
        want = torch.cat([P[k].grad.reshape(-1) for k in names])
        floor = rel(torch.cat([P32[k].grad.double().reshape(-1) for k in names]), want)
        assert rel(mine, want) < max(1e-3, 3 * floor), (rel(mine, want), floor)


def test_generator_256_fp16_vs_fp32(gpu):
    """The fp16 MFMA path at 256x256 against the fp32 path on the same weights and inputs:
    outputs within the documented 16-bit bound 2e-2, I128 gradient direction (cosine > 0.99)."""
    _, _, _, o32, d32, g32 = _g256(gpu, torch.float32)
    _, _, _, o16, d16, g16 = _g256(gpu, torch.float16)
    for name, a, b in zip(G_OUT, o16, o32):
        assert a.dtype == torch.float16
        assert rel(a.detach().float().cpu(), b.detach().cpu()) < 2e-2, name
    assert rel(d16.detach().float().cpu(), d32.detach().cpu()) < 2e-2
    x, y = g16["I128"].grad.double().reshape(-1), g32["I128"].grad.double().reshape(-1)
    assert bool(torch.isfinite(x).all())
    assert float(torch.dot(x, y) / (x.norm() * y.norm())) > 0.99


# ---- launch groups (tpg_group_begin / tpg_group_end): the four LocalPathways in lockstep ----
@pytest.mark.parametrize("dtype,flat", [(torch.bfloat16, True), (torch.float16, False), (torch.bfloat16, False)])
def test_local_pathways_grouped_equal_per_patch(gpu, dtype, flat):
    """LocalPathway.forward_group (one grouped node per layer: one grid per kernel position over
    the four patches of different sizes) against the per-patch modules on the same weights and
    inputs.  Deterministic mode (no split-K / pixel-split atomics): each member runs the same
    kernel code with the same tiles and splits either way, so outputs, the patch gradients
    and every parameter gradient are bit-identical.  flat: FlatParams-managed (pre-packed
    weights, dW / db accumulated into the flat gradient buffer, GradLink shortcut hand-off)."""
    import D_and_G_model as DG
    import tpgan_ops
    import tpgan_train
    torch.manual_seed(11)
    paths = torch.nn.ModuleList([DG.LocalPathway(use_batchnorm=False) for _ in range(4)]).to(gpu)
    fl = tpgan_train.FlatParams(paths, gpu) if flat else None
    B = 6
    xs = [torch.randn(B, 3, h, w, device=gpu) for h, w in ((40, 40), (40, 40), (32, 40), (32, 48))]
    proj = [(torch.randn(B, 3, h, w, device=gpu), torch.randn(B, 64, h, w, device=gpu))
            for h, w in ((40, 40), (40, 40), (32, 40), (32, 48))]

    def run(group):
        if fl is not None:
            fl.zero_grad()
        else:
            paths.zero_grad(set_to_none=True)
        xin = [x.clone().requires_grad_(True) for x in xs]
        old, tune = tpgan_ops.GROUP["enabled"], tpgan_ops.AUTOTUNE["enabled"]
        tpgan_ops.GROUP["enabled"] = group
        tpgan_ops.AUTOTUNE["enabled"] = False  # (both runs on the default weight-gradient tiles)
        try:
            with tpgan_ops.compute_dtype(dtype), tpgan_ops.deterministic():
                outs = (DG.LocalPathway.forward_group(list(paths), xin) if group else
                        [p(x) for p, x in zip(paths, xin)])
                loss = 0
                for (img, feat), (pi, pf) in zip(outs, proj):
                    loss = loss + (img.float() * pi).sum() + (feat.float() * pf).sum()
                loss.backward()
        finally:
            tpgan_ops.GROUP["enabled"] = old
            tpgan_ops.AUTOTUNE["enabled"] = tune
        torch.cuda.synchronize()
        return ([o.detach().clone() for pair in outs for o in pair], [x.grad.clone() for x in xin],
                [p.grad.detach().clone() for p in paths.parameters()])

    a, b = run(True), run(False)
    for u, v in zip(a[0], b[0]):
        assert u.dtype == dtype and torch.equal(u, v)
    for u, v in zip(a[1], b[1]):
        assert torch.equal(u, v)
    for (name, _), u, v in zip(paths.named_parameters(), a[2], b[2]):
        assert torch.equal(u, v), name
        assert bool(torch.isfinite(u).all()) and float(u.abs().max()) > 0, name


def test_group_flushes_before_ungrouped_entry_point(gpu):
    """include/tpgan.h: inside a launch group "a call that needs another kernel flushes the record
    first, so the semantics are always those of the calls run in order" -- also for the entry
    points of the kernel files.  The C ABI directly: a recorded halo conv (the plan says so; 16
    channels keep it off the pointwise kernel) into a zero-filled y, then tpg_avgpool_fwd(y -> m)
    before the group ends.  m is bit-equal to the same two calls outside a group, and not the
    average of the zero fill."""
    import ctypes
    import tpgan_lib as L
    lib = L.load()
    N, C, H, W, k = 1, 16, 8, 8, 3
    gen = torch.Generator().manual_seed(13)
    x = (torch.rand(N, H, W, C, generator=gen) + 0.5).to(gpu).bfloat16().permute(0, 3, 1, 2)
    w = (torch.rand(C, C, k, k, generator=gen) + 0.5).to(gpu).contiguous(memory_format=torch.channels_last)
    d = L.ConvDesc(n=N, in_c=C, in_h=H, in_w=W, out_c=C, out_h=H, out_w=W, kh=k, kw=k, stride_h=1, stride_w=1,
                   pad_t=1, pad_b=1, pad_l=1, pad_r=1, dtype=L.TPG_BF16, res_scale=1.0)
    ws = lib.tpg_conv2d_workspace(ctypes.byref(d), L.OP_FWD)
    buf = torch.zeros(ws, device=gpu, dtype=torch.uint8)
    none, plan = L.TpgTensor(), L.DataPlan()

    def run(group):
        y = torch.zeros(N, H, W, C, device=gpu, dtype=torch.bfloat16).permute(0, 3, 1, 2)
        m = torch.full((N, C), -1.0, device=gpu, dtype=torch.bfloat16)
        L.check(lib.tpg_conv2d_data_plan(ctypes.byref(d), L.OP_FWD, L.tt(x), L.tt(y), none, none, none, ws,
                                         ctypes.byref(plan)))
        assert plan.nprobs == 1 and L.DATA_KERNELS[plan.prob[0].kernel] == "halo"
        torch.cuda.synchronize()
        if group:
            lib.tpg_group_begin()
            lib.tpg_group_member()
        try:
            L.check(lib.tpg_conv2d_fwd(ctypes.byref(d), L.tt(x), L.tt(w), None, none, L.tt(y), buf.data_ptr(), ws,
                                       L.stream_ptr()))
            L.check(lib.tpg_avgpool_fwd(N, C, H, W, L.tt(y), L.tt(m), L.stream_ptr()))
        finally:
            if group:
                L.check(lib.tpg_group_end())
        torch.cuda.synchronize()
        return m

    plain, grouped = run(False), run(True)
    assert float(plain.float().min()) > 0  # (positive inputs and weights: every mean is positive)
    assert torch.equal(grouped, plain) and bool((grouped != 0).any())


def test_local_pathways_grouped_nondeterministic(gpu):
    """Default (split) mode: grouped and per-patch runs agree to summation-order rounding."""
    import D_and_G_model as DG
    import tpgan_ops
    torch.manual_seed(12)
    paths = torch.nn.ModuleList([DG.LocalPathway(use_batchnorm=False) for _ in range(4)]).to(gpu)
    xs = [torch.randn(16, 3, h, w, device=gpu) for h, w in ((40, 40), (40, 40), (32, 40), (32, 48))]

    def run(group):
        paths.zero_grad(set_to_none=True)
        old = tpgan_ops.GROUP["enabled"]
        tpgan_ops.GROUP["enabled"] = group
        try:
            with tpgan_ops.compute_dtype(torch.bfloat16):
                outs = (DG.LocalPathway.forward_group(list(paths), xs) if group else
                        [p(x) for p, x in zip(paths, xs)])
                loss = sum(img.float().square().mean() + feat.float().mean() for img, feat in outs)
                loss.backward()
        finally:
            tpgan_ops.GROUP["enabled"] = old
        torch.cuda.synchronize()
        return [o.detach().float() for pair in outs for o in pair], [p.grad.detach().clone() for p in paths.parameters()]

    a, b = run(True), run(False)
    for u, v in zip(a[0], b[0]):
        assert rel(u.cpu(), v.cpu()) < 1e-2
    ga = torch.cat([g.reshape(-1) for g in a[1]]).double()
    gb = torch.cat([g.reshape(-1) for g in b[1]]).double()
    assert rel(ga.cpu(), gb.cpu()) < 2e-2
