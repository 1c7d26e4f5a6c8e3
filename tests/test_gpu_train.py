"""GPU tests of the train step (tp-gan_amd/tpgan_train.py): the HIP Adam against
torch.optim.Adam, one full fp32 G+D step against the oracle's restatement of the same
step (oracle functions + torch.optim.Adam on CPU, float64), and hipGraph replay against
eager execution."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from _cases import load_det, rel

pytestmark = pytest.mark.gpu

BETAS = (0.5, 0.999)
LR = 1e-3


def test_adam_vs_torch(gpu):
    import tpgan_ops
    g = torch.Generator().manual_seed(3)
    n = 10_003  # not a multiple of 4: vector body + scalar tail
    p0 = torch.randn(n, generator=g, dtype=torch.float64)
    grads = [torch.randn(n, generator=g, dtype=torch.float64) for _ in range(3)]
    ref = p0.clone().requires_grad_(True)
    opt = torch.optim.Adam([ref], lr=LR, betas=BETAS, eps=1e-8, weight_decay=0.01)
    p = p0.float().to(gpu)
    m = torch.zeros_like(p)
    v = torch.zeros_like(p)
    st = torch.zeros(4, dtype=torch.float32, device=gpu)
    for gr in grads:
        ref.grad = gr.clone()
        opt.step()
        tpgan_ops.adam_step(p, (gr * 2).float().to(gpu), m, v, LR, BETAS[0], BETAS[1], 1e-8, 0.01, st, 0, 0.5)
    torch.cuda.synchronize()
    assert float(st[0]) == 3.0
    assert rel(p.cpu(), ref.detach()) < 1e-6


def test_adam_skips_nonfinite_gradients(gpu):
    """ADVICE r2 (fp16 loss scale): tpg_grad_check + tpg_adam leave parameters, moments and the
    step counter untouched when any gradient element is inf / NaN, and update normally after."""
    import tpgan_train
    torch.manual_seed(0)
    m = torch.nn.Sequential(torch.nn.Linear(7, 5), torch.nn.Linear(5, 3)).to(gpu)
    f = tpgan_train.FlatParams(m, gpu)
    f.grad.copy_(torch.randn(f.grad.shape))
    f.adam(LR, BETAS, check_finite=True)
    assert not f.last_step_skipped() and float(f.adam_state[0]) == 1.0
    snap = [t.clone() for t in (f.data, f.exp_avg, f.exp_avg_sq, f.adam_state)]
    for bad in (float("nan"), float("inf")):
        f.grad[3] = bad
        f.adam(LR, BETAS, check_finite=True)
        assert f.last_step_skipped()
        for a, b in zip(snap[:3], (f.data, f.exp_avg, f.exp_avg_sq)):
            assert torch.equal(a, b)
        assert torch.equal(snap[3][:3], f.adam_state[:3])
    f.grad[3] = 0.5
    f.adam(LR, BETAS, check_finite=True)
    assert not f.last_step_skipped() and float(f.adam_state[0]) == 2.0
    assert not torch.equal(snap[0], f.data)


def _batch(B, seed=5):
    g = torch.Generator().manual_seed(seed)

    def u(*s):
        return torch.rand(*s, generator=g, dtype=torch.float64) * 2 - 1

    return {"I128": u(B, 3, 128, 128), "left_eye": u(B, 3, 40, 40), "right_eye": u(B, 3, 40, 40),
            "nose": u(B, 3, 32, 40), "mouth": u(B, 3, 32, 48), "z": u(B, 64), "frontal": u(B, 3, 128, 128),
            "frontal_left_eye": u(B, 3, 40, 40), "frontal_right_eye": u(B, 3, 40, 40),
            "frontal_nose": u(B, 3, 32, 40), "frontal_mouth": u(B, 3, 32, 48),
            "label": torch.randint(0, 347, (B,), generator=g)}


def _oracle_step(PG, PD, b, W):
    """The trainer's step restated on the oracle (float64 CPU): D-step, Adam on D, G-step
    through the updated D, Adam on G (tpgan_train.TPGANTrainer._phase_a/b/c)."""
    from oracle import tpgan_oracle as O
    for p in list(PG.values()) + list(PD.values()):
        p.requires_grad_(True)
    optD = torch.optim.Adam(list(PD.values()), lr=LR, betas=BETAS)
    optG = torch.optim.Adam(list(PG.values()), lr=LR, betas=BETAS)
    fake, pred, _, le, re, no, mo, _ = O.generator(PG, b["I128"], b["left_eye"], b["right_eye"], b["nose"],
                                                   b["mouth"], b["z"])
    B = fake.shape[0]
    d = O.discriminator(PD, torch.cat([b["frontal"], fake.detach()], 0))
    loss_D = d[B:].mean() - d[:B].mean()
    gD = torch.autograd.grad(loss_D, list(PD.values()))
    for p, gr in zip(PD.values(), gD):
        p.grad = gr
    optD.step()
    d_gen = O.discriminator(PD, fake)
    l_tv = (fake[:, :, 1:] - fake[:, :, :-1]).abs().mean() + (fake[:, :, :, 1:] - fake[:, :, :, :-1]).abs().mean()
    loss_G = (W["weight_pixelwise"] * W["weight_128"] * (fake - b["frontal"]).abs().mean() +
              W["weight_pixelwise_local"] * ((le - b["frontal_left_eye"]).abs().mean() +
                                             (re - b["frontal_right_eye"]).abs().mean() +
                                             (no - b["frontal_nose"]).abs().mean() +
                                             (mo - b["frontal_mouth"]).abs().mean()) / 4 +
              W["weight_symmetry"] * (fake - fake.flip(3)).abs().mean() - W["weight_adv_G"] * d_gen.mean() +
              W["weight_total_varation"] * l_tv + W["weight_cross_entropy"] * F.cross_entropy(pred, b["label"]))
    gG = torch.autograd.grad(loss_G, list(PG.values()))
    for p, gr in zip(PG.values(), gG):
        p.grad = gr
    optG.step()
    return float(loss_D.detach()), float(loss_G.detach()), gD, gG


def _models(gpu):
    import D_and_G_model as DG
    G = DG.Generator(64, 347, use_batchnorm=False)
    D = DG.Discriminator()
    load_det(G, "G/", torch.float32)
    load_det(D, "D/", torch.float32)
    return G.to(gpu), D.to(gpu)


def test_train_step_vs_oracle(gpu):
    """One fp32 trainer step (G forward, D-step + HIP Adam, G-step through the updated D
    + HIP Adam) against the oracle: losses, flat gradients (global-norm 1e-3) and the
    updated parameters."""
    import tpgan_ops
    import tpgan_train
    from oracle import tpgan_oracle as O
    G, D = _models(gpu)
    tr = tpgan_train.TPGANTrainer(G, D, lr=LR, betas=BETAS, compute_dtype=torch.float32, use_dropout=False)
    b = _batch(2)
    with tpgan_ops.deterministic():  # fixed-order reductions: no run-to-run kink flips
        out = tr.step({k: (v.float() if v.is_floating_point() else v).to(gpu) for k, v in b.items()})
        torch.cuda.synchronize()
    PG, PD = O.make_params(torch.float64)
    P0 = {("G", k): v.clone() for k, v in PG.items()}
    P0.update({("D", k): v.clone() for k, v in PD.items()})
    lD, lG, gD, gG = _oracle_step(PG, PD, b, tr.w)
    # the same step in float32 on the CPU: its distance to float64 is the floor any fp32
    # implementation sits at (LeakyReLU kinks / fuser ties flip with summation order)
    PG32, PD32 = O.make_params(torch.float32)
    b32 = {k: (v.float() if v.is_floating_point() else v) for k, v in b.items()}
    _, _, gD32, gG32 = _oracle_step(PG32, PD32, b32, tr.w)
    assert abs(float(out["loss_D"]) - lD) <= 1e-3 * max(abs(lD), 1e-3)
    assert abs(float(out["loss_G"]) - lG) <= 1e-3 * abs(lG)
    for tag, model, grads, grads32, P in (("G", G, gG, gG32, PG), ("D", D, gD, gD32, PD)):
        names = [k for k, _ in model.named_parameters()]
        mine = torch.cat([p.grad.detach().double().cpu().reshape(-1) for p in model.parameters()])
        ref = torch.cat([gr.detach().reshape(-1) for gr in grads])
        floor = rel(torch.cat([gr.detach().double().reshape(-1) for gr in grads32]), ref)
        # global 1e-3, <= 1e-2 per tensor.  Deterministic mode: with split-K
        # fp32 atomics a D.model.3 LeakyReLU pre-activation within 1e-7 of zero used to land on
        # either side from run to run (round 1 had to widen this bound to 2e-3).
        assert rel(mine, ref) < max(1e-3, 3 * floor), (tag, rel(mine, ref), floor)
        for (k, p), gr in zip(model.named_parameters(), grads):
            if float(gr.norm()) > 0:
                assert rel(p.grad.detach().cpu(), gr) < 1e-2, (tag, k)
        # Adam moves each weight by ~lr: compare the update itself, not just the weights
        # (loose: elements whose gradient is ~0 may take either sign on the first step)
        p0 = torch.cat([P0[(tag, k)].reshape(-1) for k in names])
        pm = torch.cat([p.detach().double().cpu().reshape(-1) for p in model.parameters()])
        pr = torch.cat([P[k].detach().reshape(-1) for k in names])
        assert rel(pm - p0, pr - p0) < 5e-2, tag


def _snapshot(tr):
    return [t.clone() for f in (tr.fG, tr.fD) for t in (f.data, f.exp_avg, f.exp_avg_sq, f.adam_state)]


def _restore(tr, snap):
    ts = [t for f in (tr.fG, tr.fD) for t in (f.data, f.exp_avg, f.exp_avg_sq, f.adam_state)]
    for t, s in zip(ts, snap):
        t.copy_(s)
    for f in (tr.fG, tr.fD):  # the pre-packed bf16 weight images follow the restored values
        f.weights_loaded()


@pytest.mark.parametrize("segmented", [False, True])
def test_graph_replay_matches_eager(gpu, segmented):
    """Two hipGraph replays of the bf16 step land on the same weights as two eager steps
    from the same state — bit for bit, in the deterministic mode (no split-K atomics, so the
    eager steps themselves are reproducible; the default mode's order-dependent sums made the
    old yardstick, 3x the eager-vs-eager spread, a flaky one)."""
    import tpgan_ops
    with tpgan_ops.deterministic():
        _graph_case(gpu, segmented)


class _Cycle:
    """A reference cycle that owns device memory (what a dropped trainer <-> gradient-sync
    pair was in round 4): freed only by the cyclic garbage collector."""

    def __init__(self, gpu):
        self.t = torch.empty(1 << 20, device=gpu)
        self.me = self


def test_graph_capture_gc_safe(gpu):
    """a cyclic collection inside the capture window freed device memory
    mid-capture and aborted the process.  Here a device-memory cycle becomes garbage at the
    start of phase B -- inside the capture -- with the collector's threshold at 1, so any
    allocation of Python objects would collect it there; capture() keeps the collector off
    for the window, the capture completes, and the replays still match eager steps bit for bit
    (deterministic mode).  The cycle is collected once the capture has ended."""
    import gc
    import weakref
    import tpgan_ops
    holder = {"c": _Cycle(gpu)}
    probe = weakref.ref(holder["c"])
    seen = {}

    def arm(tr):
        orig = tr._phase_b

        def phase_b(b):
            if tr._capturing and "c" in holder:
                del holder["c"]              # unreachable now, but for the cycle
                seen["gc_enabled"] = gc.isenabled()
                seen["alive_in_capture"] = probe() is not None
            return orig(b)
        tr._phase_b = phase_b

    thr = gc.get_threshold()
    gc.set_threshold(1, 1, 1)
    try:
        with tpgan_ops.deterministic():
            _graph_case(gpu, False, arm=arm)
    finally:
        gc.set_threshold(*thr)
    assert seen == {"gc_enabled": False, "alive_in_capture": True}, seen
    gc.collect()
    assert probe() is None


def _graph_case(gpu, segmented, arm=None):
    import tpgan_train
    G, D = _models(gpu)
    tr = tpgan_train.TPGANTrainer(G, D, lr=LR, betas=BETAS, compute_dtype=torch.bfloat16, use_dropout=False)
    b = tpgan_train.synthetic_batch(4, gpu, seed=11)
    tr.step(b)  # autotune outside capture
    torch.cuda.synchronize()
    snap = _snapshot(tr)
    if arm is not None:
        arm(tr)

    def two_eager():
        _restore(tr, snap)
        outs = [tr.step(b) for _ in range(2)]
        torch.cuda.synchronize()
        return tr.fG.data.clone(), tr.fD.data.clone(), tr.fG.adam_state.clone(), outs

    e1 = two_eager()
    e2 = two_eager()
    _restore(tr, snap)
    tr.capture(b, warmup=0, segmented=segmented)
    _restore(tr, snap)
    # both replays' outputs are held until the end: a loss that aliased the graph pool would
    # read step 2's value for step 1 (round 2's dropped graphed-loss path)
    outs = [tr.step_graphed() for _ in range(2)]
    torch.cuda.synchronize()
    assert float(tr.fG.adam_state[0]) == float(e1[2][0])
    for got, a, c in ((tr.fG.data, e1[0], e2[0]), (tr.fD.data, e1[1], e2[1])):
        assert torch.equal(a, c)      # eager reruns reproduce
        assert torch.equal(got, a)    # and the graph replays match them
    for k in ("loss_D", "loss_G"):
        for s in range(2):
            assert torch.equal(e1[3][s][k], e2[3][s][k]), (k, s)
            assert torch.equal(outs[s][k], e1[3][s][k]), (k, s, float(outs[s][k]), float(e1[3][s][k]))
        assert not torch.equal(outs[0][k], outs[1][k]), k  # the two steps' losses do differ
    # parameters moved after capture (the data-parallel bucket relayout): replay refuses
    tr.fD.relayout(list(range(len(tr.fD.params))))
    with pytest.raises(RuntimeError, match="re-laid out"):
        tr.step_graphed()


def test_graph_replay_segmented_with_identity(gpu):
    """segmented capture (one graph per phase, the data-parallel form) of a step with
    the identity loss.  Eager phase A forks the real-image features onto a side stream that
    phase B joins; a per-phase capture must not leave that fork open, so the capture computes
    them in phase B.  Two replays against two eager steps (bf16, deterministic)."""
    import FeatureExtract as FE
    import tpgan_ops
    import tpgan_train
    with tpgan_ops.deterministic():
        G, D = _models(gpu)
        torch.manual_seed(0)
        ext = FE.FeatureExtractModel("mobilenetv2", 347).to(gpu)
        tr = tpgan_train.TPGANTrainer(G, D, lr=LR, betas=BETAS, compute_dtype=torch.bfloat16, use_dropout=False,
                                      identity_fn=FE.IdentityPreservingLoss(ext, torch.bfloat16))
        b = tpgan_train.synthetic_batch(2, gpu, seed=13)
        tr.step(b)
        torch.cuda.synchronize()
        snap = _snapshot(tr)
        eager = [tr.step(b) for _ in range(2)]
        torch.cuda.synchronize()
        ref = (tr.fG.data.clone(), tr.fD.data.clone())
        _restore(tr, snap)
        tr.capture(b, warmup=0, segmented=True)
        _restore(tr, snap)
        outs = [tr.step_graphed() for _ in range(2)]
        torch.cuda.synchronize()
    for got, want in ((tr.fG.data, ref[0]), (tr.fD.data, ref[1])):
        assert rel(got.cpu(), want.cpu()) < 1e-6
    for s in range(2):
        for k in ("loss_D", "loss_G"):
            a, c = float(outs[s][k]), float(eager[s][k])
            assert np.isfinite(a) and abs(a - c) <= 1e-6 * max(abs(c), 1e-3), (s, k, a, c)


def test_identity_side_stream_bit_identical(gpu):
    """tpgan_train.IDENTITY_STREAM: the identity loss (and, through autograd's stream rule, its
    input-gradient backward) on a side stream beside D(fake) gives the same step as one stream
    (bf16, deterministic: the same kernels in the same order per stream -> bit-identical)."""
    import FeatureExtract as FE
    import tpgan_ops
    import tpgan_train
    prev = tpgan_train.IDENTITY_STREAM["enabled"]
    res = {}
    try:
        with tpgan_ops.deterministic():
            for on in (False, True):
                tpgan_train.IDENTITY_STREAM["enabled"] = on
                G, D = _models(gpu)
                torch.manual_seed(0)
                ext = FE.FeatureExtractModel("resnet50", 347).to(gpu)
                tr = tpgan_train.TPGANTrainer(G, D, lr=LR, betas=BETAS, compute_dtype=torch.bfloat16,
                                              use_dropout=False,
                                              identity_fn=FE.IdentityPreservingLoss(ext, torch.bfloat16))
                b = tpgan_train.synthetic_batch(2, gpu, seed=17)
                outs = [tr.step(b) for _ in range(2)]
                torch.cuda.synchronize()
                res[on] = (tr.fG.data.clone(), tr.fD.data.clone(), [float(o["loss_G"]) for o in outs])
    finally:
        tpgan_train.IDENTITY_STREAM["enabled"] = prev
    assert torch.equal(res[True][0], res[False][0]) and torch.equal(res[True][1], res[False][1])
    assert res[True][2] == res[False][2]


def test_gradient_penalty_double_backward_vs_oracle(gpu):
    """WGAN-GP through the HIP double backward: the penalty and D's parameter gradients
    of it against torch's double backward of the oracle D (float64 CPU), global 1e-3."""
    import D_and_G_model as DG
    import tpgan_train
    from oracle import tpgan_oracle as O
    from oracle.det_init import det_input
    G, D = _models(gpu)
    tr = tpgan_train.TPGANTrainer(G, D, compute_dtype=torch.float32, use_dropout=False)
    real = torch.from_numpy(det_input("gp/real", (2, 3, 128, 128)))
    fake = torch.from_numpy(det_input("gp/fake", (2, 3, 128, 128)))
    alpha = torch.tensor([0.3, 0.8], dtype=torch.float64).view(2, 1, 1, 1)
    for p in D.parameters():
        p.grad = None
    gp = tr.gradient_penalty(real.float().to(gpu), fake.float().to(gpu), alpha.float().to(gpu))
    gp.backward()
    torch.cuda.synchronize()
    _, PD = O.make_params(torch.float64)
    for p in PD.values():
        p.requires_grad_(True)
    xh = (alpha * real + (1 - alpha) * fake).requires_grad_(True)
    (gx,) = torch.autograd.grad(O.discriminator(PD, xh).sum(), xh, create_graph=True)
    gp_ref = ((gx.reshape(2, -1).norm(dim=1) - 1.0) ** 2).mean()
    gD = torch.autograd.grad(gp_ref, list(PD.values()), allow_unused=True)  # the head bias drops out of grad_x
    gD = [torch.zeros_like(p) if g is None else g for p, g in zip(PD.values(), gD)]
    assert abs(float(gp) - float(gp_ref)) <= 1e-3 * abs(float(gp_ref))
    mine = torch.cat([(p.grad if p.grad is not None else torch.zeros_like(p)).detach().double().cpu().reshape(-1)
                      for p in D.parameters()])
    ref = torch.cat([g.reshape(-1) for g in gD])
    assert rel(mine, ref) < 1e-3


def test_train_step_with_gp_flat(gpu):
    """The full bf16 step with WGAN-GP on flat parameters: D's double-backward gradients
    land in the flat buffer (views stay bound) and the step stays finite."""
    import tpgan_train
    G, D = _models(gpu)
    tr = tpgan_train.TPGANTrainer(G, D, compute_dtype=torch.bfloat16, gradient_penalty=True)
    b = tpgan_train.synthetic_batch(2, gpu, seed=5)
    out = tr.step(b)
    torch.cuda.synchronize()
    assert np.isfinite(float(out["loss_D"])) and np.isfinite(float(out["loss_G"]))
    base = tr.fD.grad.data_ptr()
    end = base + tr.fD.grad.numel() * 4
    assert all(base <= p.grad.data_ptr() < end for p in D.parameters())
    assert float(tr.fD.grad.abs().sum()) > 0


def test_prepacked_weights_match_inline_packing(gpu):
    """After a train step the FlatParams-managed convs use pre-packed weight images
    (tpg_pack_run after Adam).  Default mode: G / D outputs and input gradients match the per-call
    packing path to within the run-to-run floor.  Deterministic mode: three whole train steps from
    one snapshot with the images and three with per-call packing land on the same weights and Adam
    moments bit for bit, eager and as graph replays -- an image one update stale in any step moves
    the next step's weights, so nothing but equality passes."""
    import tpgan_ops
    import tpgan_train
    G, D = _models(gpu)
    tr = tpgan_train.TPGANTrainer(G, D, compute_dtype=torch.bfloat16, use_dropout=False)
    b = tpgan_train.synthetic_batch(2, gpu, seed=21)
    tr.step(b)  # (the first step also re-lays the flat buffers out in gradient-completion order)
    tr.step(b)
    torch.cuda.synchronize()
    # images re-packed after the update: one batched table for the whole network, or per bucket
    # when G's Adam ran bucket by bucket under the backward (TPGANTrainer.overlap_optimizer)
    assert len(tr.fG.pack_entries) > 50
    assert tr.fG.pack_table is not None or (tr.overlap_optimizer and tr.fG.range_packs[1])

    # every module output of G's forward, per run (on a mismatch the message names the first
    # modules whose outputs differ; this test failed once in a full-suite run, gpurun r06u, and
    # did not reproduce in isolation: tools/pack_mismatch.py, r06w)
    names = {m: n for n, m in G.named_modules()}
    calls = []

    def hook(m, inp, out):
        t = out[0] if isinstance(out, (tuple, list)) else out
        if torch.is_tensor(t):
            calls.append((names[m], t.detach().float().clone()))

    hooks = [m.register_forward_hook(hook) for m in G.modules()]

    def run():
        calls.clear()
        x = b["I128"].clone().requires_grad_(True)
        with tpgan_ops.compute_dtype(torch.bfloat16):
            outs = G(x, b["left_eye"], b["right_eye"], b["nose"], b["mouth"], b["z"], False)
            d = D(outs[0])
        (outs[0].float().sum() + d.float().sum()).backward()
        torch.cuda.synchronize()
        return outs[0].detach().float().clone(), d.detach().float().clone(), x.grad.clone(), list(calls)

    try:
        a = run()
        a2 = run()  # run-to-run floor: split-K fp32 atomics (stride-2 convs, fc1) are order-dependent
        tpgan_ops.PACK["enabled"] = False
        try:
            c = run()
        finally:
            tpgan_ops.PACK["enabled"] = True
    finally:
        for h in hooks:
            h.remove()
    diff = [(n, rel(t2.cpu(), t0.cpu())) for (n, t0), (_, t2) in zip(a[3], c[3]) if rel(t2.cpu(), t0.cpu()) > 1e-6][:6]
    failures = []  # (both halves always run: the default-mode verdict is given at the end)
    for i in range(3):
        floor = rel(a2[i].cpu(), a[i].cpu())
        if not rel(c[i].cpu(), a[i].cpu()) <= max(3 * floor, 1e-6):
            failures.append(("default mode", i, rel(c[i].cpu(), a[i].cpu()), floor, diff))
    del a, a2, c, calls

    # ---- deterministic mode: whole trajectories.  Both paths take the same plans there (no data
    # split tuner, no split-K; the weight-gradient picks come from the one shared cache), so the
    # only difference left is who wrote the 16-bit weight image
    def state():
        torch.cuda.synchronize()
        return [t.clone() for f in (tr.fG, tr.fD) for t in (f.data, f.exp_avg, f.exp_avg_sq)]

    with tpgan_ops.deterministic():
        tr.step(b)
        torch.cuda.synchronize()
        snap = _snapshot(tr)
        got = {}
        for graphed in (False, True):
            for pack in (True, False):
                tpgan_ops.PACK["enabled"] = pack
                try:
                    _restore(tr, snap)
                    if graphed:
                        tr.reset_capture()
                        tr.capture(b, warmup=0)
                        _restore(tr, snap)
                    for _ in range(3):
                        tr.step_graphed() if graphed else tr.step(b)
                    got[(graphed, pack)] = state()
                finally:
                    tpgan_ops.PACK["enabled"] = True
        tr.reset_capture()
    assert not torch.equal(got[(False, True)][0], snap[0])  # (the steps did move the weights)
    tnames = ("fG.data", "fG.exp_avg", "fG.exp_avg_sq", "fD.data", "fD.exp_avg", "fD.exp_avg_sq")
    for graphed in (False, True):
        for n, x, y in zip(tnames, got[(graphed, True)], got[(graphed, False)]):
            if not torch.equal(x, y):
                failures.append(("deterministic, %s: pre-packed vs inline" % ("graph replays" if graphed else "eager"), n,
                                 rel(x.cpu(), y.cpu())))
    assert not failures, failures


def _images_current(tr, tag):
    """Every pre-packed image of G and D is at its network's epoch and equals a from-scratch pack
    (fresh jobs, new buffer) of the LIVE parameter found at the entry's source pointer; an entry
    whose pointer matches no live parameter fails by name.  Returns the number checked."""
    import tpgan_ops
    from _packcheck import check_entries
    return sum(check_entries(tpgan_ops, f, f.params, tag + "/" + n) for n, f in (("G", tr.fG), ("D", tr.fD)))


def test_prepacked_images_current_after_steps(gpu):
    """Every pre-packed weight image of G and D equals a fresh pack of the current fp32 weights
    after eager steps, after a restore (weights_loaded) and after graph replays: no entry left
    out of the batched re-pack, none packed from a stale or foreign weight pointer.  The fresh
    pack is planned from the live parameter view, not from the entry's stored jobs (re-running
    those proves nothing about where they read from)."""
    import tpgan_train
    G, D = _models(gpu)
    tr = tpgan_train.TPGANTrainer(G, D, compute_dtype=torch.bfloat16, use_dropout=False)
    b = tpgan_train.synthetic_batch(2, gpu, seed=29)
    for _ in range(3):
        tr.step(b)
    assert _images_current(tr, "eager") > 50
    snap = _snapshot(tr)
    tr.step(b)
    _restore(tr, snap)
    assert _images_current(tr, "restored") > 50
    tr.capture(b, warmup=1)
    for _ in range(2):
        tr.step_graphed()
    assert _images_current(tr, "graph") > 50


def test_prepacked_images_current_bucketed_optimizer(gpu):
    """The same with overlap_optimizer=True: G's images re-packed bucket by bucket on the
    communication stream (repack_range), through the step that re-lays the flat buffers out
    (every image dropped and rebuilt at the parameters' new addresses), a restore, and a
    capture."""
    import tpgan_train
    G, D = _models(gpu)
    tr = tpgan_train.TPGANTrainer(G, D, compute_dtype=torch.bfloat16, use_dropout=False, overlap_optimizer=True)
    assert tr.gsync is not None and tr.gsync.optimizer is not None
    b = tpgan_train.synthetic_batch(2, gpu, seed=29)
    tr.step(b)  # learns the bucket order and re-lays G's buffers out
    assert tr.fG.layout_version == 1 and not any(e is not None for e in tr.fG.pack_entries.values())
    tr.step(b)  # the first step on the new layout: every G image is new
    assert _images_current(tr, "relaid") > 50
    tr.step(b)
    assert tr.fG.range_packs[1] and _images_current(tr, "bucketed") > 50
    snap = _snapshot(tr)
    tr.step(b)
    _restore(tr, snap)
    assert _images_current(tr, "restored") > 50
    tr.capture(b, warmup=1)
    for _ in range(2):
        tr.step_graphed()
    assert _images_current(tr, "graph") > 50


def _ledger_check(events, first_clean, tag):
    """events: one list of ledger lines per step.  No lazy pack from step `first_clean` on; and a
    lazily packed image is read, for as long as it stays at that epoch, on the stream that packed
    it (a read on another stream has no ordering against the pack unless somebody put one there)."""
    for s, evs in enumerate(events[first_clean:], first_clean):
        lazy = [(e[1][0], e[1][1][:9]) for e in evs if e[0] == "lazy"]
        assert not lazy, (tag, "step %d packs on use" % s, len(lazy), lazy[:4])
    flat = [e for evs in events for e in evs]
    packed_on = {}
    for kind, key, stream, fepoch, eepoch in flat:
        if kind == "lazy":
            packed_on[(key, eepoch)] = stream
        elif kind in ("batched", "range"):
            packed_on.pop((key, eepoch), None)  # (re-packed by the optimizer: no longer the lazy image)
        elif kind == "read" and (key, eepoch) in packed_on:
            assert stream == packed_on[(key, eepoch)], (
                tag, "image packed on use on stream %#x is read on stream %#x" % (packed_on[(key, eepoch)], stream),
                key[0], key[1][:9], eepoch)
    return sum(1 for e in flat if e[0] == "lazy"), sum(1 for e in flat if e[0] == "read")


def test_pack_ledger_stream_order(gpu, monkeypatch):
    """tpgan_ops.PACK["audit"] over four eager steps (side-stream local pathways, the identity
    fork) and over capture()'s warm-up on its side stream: which stream packed each image and
    which streams read it."""
    import FeatureExtract as FE
    import tpgan_ops
    import tpgan_train
    assert tpgan_ops.MULTISTREAM and tpgan_train.IDENTITY_STREAM["enabled"]
    G, D = _models(gpu)
    torch.manual_seed(0)
    ext = FE.FeatureExtractModel("mobilenetv2", 347).to(gpu)
    tr = tpgan_train.TPGANTrainer(G, D, lr=LR, betas=BETAS, compute_dtype=torch.bfloat16, use_dropout=False,
                                  identity_fn=FE.IdentityPreservingLoss(ext, torch.bfloat16))
    b = tpgan_train.synthetic_batch(2, gpu, seed=31)
    audit = []
    monkeypatch.setitem(tpgan_ops.PACK, "audit", audit)
    events, relaid = [], -1
    for s in range(4):
        n0, lv = len(audit), (tr.fG.layout_version, tr.fD.layout_version)
        tr.step(b)
        torch.cuda.synchronize()
        events.append(audit[n0:])
        if (tr.fG.layout_version, tr.fD.layout_version) != lv:
            relaid = s
    first_clean = relaid + 2  # the second step after the last relayout (none: after construction)
    assert first_clean <= 2, relaid
    nlazy, nread = _ledger_check(events, first_clean, "eager")
    print("ledger, eager: %d lazy packs, %d reads, %d streams" % (nlazy, nread, len({e[2] for e in audit})))
    assert nlazy > 50 and nread > 4 * 50  # (the first step did pack on use, every step reads)
    assert len({e[2] for e in audit if e[0] == "read"}) > 1  # (the side streams are in the ledger)
    assert any(e[0] == "batched" for e in audit)
    # capture()'s warm-up steps run on a side stream of its own; every image is current by now
    n0 = len(audit)
    tr.capture(b, warmup=2, segmented=True)
    torch.cuda.synchronize()
    _ledger_check(events + [audit[n0:]], len(events), "capture warm-up")
def test_deterministic_mode_bit_identical(gpu):
    """tpg_set_deterministic: two bf16 train steps from the same state give bit-identical
    parameters, gradients and Adam moments (SURVEY.md §5 race detection / run-to-run)."""
    import tpgan_ops
    import tpgan_train
    G, D = _models(gpu)
    tr = tpgan_train.TPGANTrainer(G, D, lr=LR, betas=BETAS, compute_dtype=torch.bfloat16, use_dropout=False)
    b = tpgan_train.synthetic_batch(4, gpu, seed=17)
    with tpgan_ops.deterministic():
        tr.step(b)
        torch.cuda.synchronize()
        snap = _snapshot(tr)
        res = []
        for _ in range(2):
            _restore(tr, snap)
            tr.step(b)
            torch.cuda.synchronize()
            res.append([t.clone() for t in (tr.fG.data, tr.fD.data, tr.fG.grad, tr.fD.grad, tr.fG.exp_avg_sq)])
    for a, c in zip(*res):
        assert torch.equal(a, c)


def test_real_ahead_reuse_and_invalidation(gpu, tmp_path):
    """The next step's precomputed D(real) pass (real_ahead) is used only for the
    batch it was computed on, unchanged, under the same D weights:
      - announced and unchanged: reused;
      - the same batch object refilled in place (copy_) before the step: NOT reused, and the step
        lands bit for bit where a trainer without real_ahead lands (deterministic mode);
      - D's weights replaced by load_checkpoint after the pass: NOT reused."""
    import tpgan_ops
    import tpgan_train
    b = tpgan_train.synthetic_batch(4, gpu, seed=23)
    new_frontal = tpgan_train.synthetic_batch(4, gpu, seed=24)["frontal"]
    with tpgan_ops.deterministic():
        G, D = _models(gpu)
        # (both trainers keep the module-order flat layout -- no bucketed optimizer, hence no step-1
        # relayout at world 1 -- so that one's snapshot restores into the other)
        ref = tpgan_train.TPGANTrainer(G, D, lr=LR, betas=BETAS, compute_dtype=torch.bfloat16, use_dropout=False,
                                       real_ahead=False, overlap_optimizer=False)
        ref.step(b)
        snap = _snapshot(ref)
        b2 = {k: (v.clone() if k != "frontal" else new_frontal.clone()) for k, v in b.items()}
        ref.step(b2)
        torch.cuda.synchronize()
        want = [t.clone() for t in (ref.fG.data, ref.fD.data)]

        ra = tpgan_train.TPGANTrainer(ref.G, ref.D, lr=LR, betas=BETAS, compute_dtype=torch.bfloat16,
                                      use_dropout=False, real_ahead=True, overlap_optimizer=False)
        _restore(ra, snap)
        bb = {k: v.clone() for k, v in b.items()}
        ra._real_ahead(bb)  # (as the previous step would have, announcing bb)
        assert ra._d_real_next is not None
        bb["frontal"].copy_(new_frontal)  # the caller refills its persistent batch in place
        ra.step(bb)
        torch.cuda.synchronize()
        assert ra.real_ahead_used == 0
        for a, c in zip(want, (ra.fG.data, ra.fD.data)):
            assert torch.equal(a, c)

        # unchanged announced batch: reused
        ra.step(bb, next_b=bb)
        ra.step(bb)
        assert ra.real_ahead_used == 1
        # weights loaded after the pass: the stale pass is dropped
        ra.save_checkpoint(str(tmp_path), 1)
        ra.step(bb, next_b=bb)
        ra.load_checkpoint(str(tmp_path), 1)
        ra.step(bb)
        torch.cuda.synchronize()
        assert ra.real_ahead_used == 1


def test_bucketed_optimizer_bit_identical(gpu):
    """TPGANTrainer(overlap_optimizer=True): G's Adam and weight repack issued bucket by bucket
    on the communication stream under the G backward (world 1) land bit for bit where the
    whole-network update after the backward lands (deterministic mode, bf16, same state; the
    Adam kernel's update of an element must not depend on where its bucket slice starts)."""
    import tpgan_ops
    import tpgan_train
    G, D = _models(gpu)
    tr = tpgan_train.TPGANTrainer(G, D, lr=LR, betas=BETAS, compute_dtype=torch.bfloat16, use_dropout=False,
                                  overlap_optimizer=True)
    assert tr.gsync is not None and tr.gsync.optimizer is not None
    b = tpgan_train.synthetic_batch(4, gpu, seed=29)
    with tpgan_ops.deterministic():
        tr.step(b)  # (learns the bucket layout and relays the flat buffers out)
        torch.cuda.synchronize()
        snap = _snapshot(tr)
        res = {}
        for mode in ("bucketed", "whole", "bucketed"):
            _restore(tr, snap)
            opt = tr.gsync.optimizer
            if mode == "whole":
                tr.gsync.optimizer = None
            try:
                tr.step(b)
                tr.step(b)
            finally:
                tr.gsync.optimizer = opt
            torch.cuda.synchronize()
            res.setdefault(mode, []).append([t.clone() for t in (tr.fG.data, tr.fG.exp_avg, tr.fG.exp_avg_sq,
                                                                 tr.fG.adam_state, tr.fD.data)])
    for a, c, a2 in zip(res["bucketed"][0], res["whole"][0], res["bucketed"][1]):
        assert torch.equal(a, a2)
        assert torch.equal(a, c)


def test_bs32_step_properties(gpu):
    """The benchmark's configuration (bf16, bs32, flat params, autotuned kernels) against the
    same step in fp32 (deterministic) from the same weights and batch: losses finite and within
    2e-2, parameters finite, G / D gradients within a bound scaled from B=2.  Why scaled: the
    batch-mean gradient shrinks as per-sample contributions cancel (G: |g| at bs32 is ~1/4 of
    B=2), while the error of bf16 weights and activations is largely systematic (the same
    rounded weights for every sample) and does not; so bs32 may sit at
    err(B=2) * |g(B=2)| / |g(bs32)|, and the test allows 3x that (never below 5e-2)."""
    _step_property_case(gpu, 32, torch.bfloat16)


def _step_property_case(gpu, B, lowp, img=128, identity=None):
    """test_bs32_step_properties for one workload: the 16-bit step at batch B against the fp32
    deterministic step from the same weights, extractor and batch (see its docstring for the
    bound; fp16 gradients are compared with the static loss scale divided out)."""
    import D_and_G_model as DG
    import FeatureExtract as FE
    import tpgan_ops
    import tpgan_train
    res = {}
    for bb in (2, B):
        for dt in (torch.float32, lowp):
            G = DG.Generator(64, 347, use_batchnorm=False, img_size=img)
            D = DG.Discriminator()
            load_det(G, "G/", torch.float32)
            load_det(D, "D/", torch.float32)
            G, D = G.to(gpu), D.to(gpu)
            idf = None
            if identity is not None:
                torch.manual_seed(0)
                idf = FE.IdentityPreservingLoss(FE.FeatureExtractModel(identity, 347).to(gpu), dt)
            tr = tpgan_train.TPGANTrainer(G, D, lr=LR, betas=BETAS, compute_dtype=dt, use_dropout=False,
                                          identity_fn=idf)
            b = tpgan_train.synthetic_batch(bb, gpu, seed=23, img_size=img)
            with tpgan_ops.deterministic(dt == torch.float32):
                out = tr.step(b)
                torch.cuda.synchronize()
            assert np.isfinite(float(out["loss_D"])) and np.isfinite(float(out["loss_G"])), (bb, dt)
            for f in (tr.fG, tr.fD):
                assert bool(torch.isfinite(f.grad).all()) and bool(torch.isfinite(f.data).all()), (bb, dt)
            res[(bb, dt)] = (float(out["loss_D"]), float(out["loss_G"]), (tr.fG.grad / tr.loss_scale).cpu(),
                             (tr.fD.grad / tr.loss_scale).cpu())
            del tr, G, D, idf
            torch.cuda.empty_cache()
    a, c = res[(B, torch.float32)], res[(B, lowp)]
    assert abs(c[0] - a[0]) <= 2e-2 * max(abs(a[0]), 1e-2) and abs(c[1] - a[1]) <= 2e-2 * abs(a[1]), (a[:2], c[:2])
    a2, c2 = res[(2, torch.float32)], res[(2, lowp)]
    for i, tag in ((2, "G"), (3, "D")):
        err2, errB = rel(c2[i], a2[i]), rel(c[i], a[i])
        shrink = float(a2[i].norm()) / float(a[i].norm())
        assert errB < max(5e-2, 3 * err2 * shrink), (tag, errB, err2, shrink)


@pytest.mark.timeout(400)
def test_config3_bs32_resnet50_step_properties(gpu):
    """BASELINE configs[2] at its size: bs32, bf16, ResNet-50 identity-preserving loss in the G
    step (reference D_and_G_model.py:350-407 + FeatureExtract.py:5-41; ResNet-50 is
    build-defined, parity unpinned) against the fp32 deterministic step."""
    _step_property_case(gpu, 32, torch.bfloat16, identity="resnet50")


@pytest.mark.timeout(400)
def test_config5_bs16_256_fp16_step_properties(gpu):
    """BASELINE configs[4] at its per-GPU size: bs16, 256x256, fp16 MFMA (static loss scale),
    MobileNetV2 identity loss, against the fp32 deterministic step (G at 256 is the build's
    generalisation of the 128-only reference: parity unpinned)."""
    _step_property_case(gpu, 16, torch.float16, img=256, identity="mobilenetv2")


def test_config5_fp16_256_step(gpu):
    """BASELINE configs[4] in small: the 256x256 G + D train step in fp16 (static loss scale,
    unscaled in the Adam launch) with the MobileNetV2 identity loss, B=2: finite losses,
    parameters and gradients; the fp16 step's gradients against the fp32 step's from the same
    weights and batch, within the bf16-style bound of test_bs32_step_properties."""
    import D_and_G_model as DG
    import FeatureExtract as FE
    import tpgan_ops
    import tpgan_train
    from _cases import load_det
    res = {}
    for dt in (torch.float32, torch.float16):
        G = DG.Generator(64, 347, use_batchnorm=False, img_size=256)
        D = DG.Discriminator()
        load_det(G, "G/", torch.float32)
        load_det(D, "D/", torch.float32)
        G, D = G.to(gpu), D.to(gpu)
        torch.manual_seed(0)
        ext = FE.FeatureExtractModel("mobilenetv2", 347).to(gpu)
        tr = tpgan_train.TPGANTrainer(G, D, lr=LR, betas=BETAS, compute_dtype=dt, use_dropout=False,
                                      identity_fn=FE.IdentityPreservingLoss(ext, dt))
        assert tr.loss_scale == (1024.0 if dt == torch.float16 else 1.0)
        b = tpgan_train.synthetic_batch(2, gpu, seed=31, img_size=256)
        with tpgan_ops.deterministic(dt == torch.float32):
            out = tr.step(b)
            torch.cuda.synchronize()
        assert np.isfinite(float(out["loss_D"])) and np.isfinite(float(out["loss_G"])), dt
        for f in (tr.fG, tr.fD):
            assert bool(torch.isfinite(f.grad).all()) and bool(torch.isfinite(f.data).all()), dt
        res[dt] = (float(out["loss_G"]), (tr.fG.grad / tr.loss_scale).cpu(), (tr.fD.grad / tr.loss_scale).cpu())
        del tr, G, D, ext
        torch.cuda.empty_cache()
    a, c = res[torch.float32], res[torch.float16]
    assert abs(c[0] - a[0]) <= 2e-2 * abs(a[0])
    assert rel(c[1], a[1]) < 1e-1 and rel(c[2], a[2]) < 1e-1, (rel(c[1], a[1]), rel(c[2], a[2]))