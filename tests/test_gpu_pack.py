"""GPU: pre-packed weight images (FlatParams-managed parameters, tpg_conv2d_pack_jobs +
tpg_pack_run) against the pack-inside-the-call path, bit for bit.

Both paths run the same kernel with the same plan, so they differ only in who wrote the bf16
weight image: the batched pack kernel (its item path for forward images, its LDS-transpose path
for input-gradient images) or the per-call pack.  The geometries include the channel counts
whose last 32-channel k-step holds <= 16 live channels (75, 206, 208, 80: the halo kernel's
paired steps, two taps per MFMA, tpg_halo.hip) -- the layers of D_and_G_model.py:257-279
(add_conv_and_deconv_128, enhance_features_128, conv5, enhance_features_64, add_conv_and_deconv_64).
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

GEOMS = [  # (n, cin, h, w, cout, k)
    (2, 75, 24, 40, 75, 7),
    (2, 206, 16, 24, 206, 5),
    (1, 206, 20, 36, 64, 5),
    (2, 208, 16, 16, 208, 3),
    (2, 80, 20, 24, 80, 5),
    (2, 40, 12, 12, 48, 3),
    (2, 16, 8, 8, 8, 3),
]


@pytest.mark.parametrize("geom", GEOMS, ids=[str(g[1]) + "x" + str(g[5]) + "-" + str(i) for i, g in enumerate(GEOMS)])
def test_prepacked_equals_call_packed(gpu, geom):
    import tpgan_ops
    import tpgan_train
    n, cin, h, w, cout, k = geom
    gen = torch.Generator().manual_seed(cin * 31 + k)
    x0 = (torch.rand(n, cin, h, w, generator=gen) * 2 - 1)
    w0 = (torch.rand(cout, cin, k, k, generator=gen) * 2 - 1) * (1.0 / (cin * k * k) ** 0.5)
    b0 = torch.rand(cout, generator=gen) * 0.1
    gy0 = torch.rand(n, cout, h, w, generator=gen) * 2 - 1
    res = []
    for managed in (False, True):
        conv = torch.nn.Conv2d(cin, cout, k, padding=k // 2).to(gpu)
        with torch.no_grad():
            conv.weight.copy_(w0)
            conv.bias.copy_(b0)
        conv = conv.to(memory_format=torch.channels_last)
        if managed:  # (the parameters become views of one flat buffer: pre-packed images)
            flat = tpgan_train.FlatParams(conv, gpu)
        x = x0.to(gpu).contiguous(memory_format=torch.channels_last).requires_grad_(True)
        with tpgan_ops.compute_dtype(torch.bfloat16), tpgan_ops.deterministic():
            y = tpgan_ops.conv2d(x, conv.weight, conv.bias, pad=(k // 2,) * 4, act=torch.nn.LeakyReLU(0.01))
            y.backward(gy0.to(gpu).to(y.dtype))
        torch.cuda.synchronize()
        if managed:
            assert len(flat.pack_entries) >= 2, flat.pack_entries  # (forward and input-gradient images)
        res.append((y.detach().float().cpu(), x.grad.float().cpu()))
    (y0, dx0), (y1, dx1) = res
    assert torch.equal(y0, y1), float((y0 - y1).abs().max())
    assert torch.equal(dx0, dx1), float((dx0 - dx1).abs().max())


# ---- pre-packed images x launch plans -------------------------------------------------------------
# An image is packed once per weight update under whatever descriptor its first user had
# (tpgan_ops._pack_entry: before the data-split tuner put its pick into the descriptor, inside or
# outside tpgan_ops.concurrent()) and then consumed under every plan the same shape is launched
# with.  That is sound only if the image's layout follows shape and dtype alone
# (tests/test_pack_host.py::test_pack_jobs_ignore_plan_fields holds it on the planner); here the
# device side: for every planner branch and every forced (data_ksplit, data_algo), with the image
# packed under one concurrency flag and used under the other, the managed path gives what the
# pack-inside-the-call path gives, and the image equals a from-scratch pack of the live weight.
# (n, cin, h, w, cout, k, stride, pad (t, b, l, r), reflect, transposed, output_padding)
def _g(n, cin, h, w, cout, k, s=1, pad=None, reflect=False, transposed=False, op=0):
    return (n, cin, h, w, cout, k, s, (k // 2,) * 4 if pad is None else pad, reflect, transposed, op)


XGEOMS = [_g(*g) for g in GEOMS] + [
    # small maps on both sides of the small_map / pointwise-kernel rule (C % 32 == 0, C <= 256 or
    # above, BN % 64 == 0 or not)
    _g(4, 64, 10, 10, 64, 3), _g(2, 128, 20, 20, 128, 3), _g(8, 256, 8, 8, 256, 3), _g(4, 512, 8, 8, 512, 3),
    _g(2, 64, 8, 8, 160, 3),
    _g(2, 128, 16, 16, 64, 1),                                # 1x1: the pointwise kernel
    _g(4, 128, 16, 16, 64, 3, s=2),                           # stride 2
    _g(4, 64, 5, 5, 32, 3, s=2, transposed=True, op=1),       # transposed stride 2
    _g(4, 96, 8, 8, 96, 2, pad=(1, 0, 1, 0), reflect=True),   # reflect 2x2
]
XPLANS = [(0, 0), (1, 0), (2, 0), (5, 0), (0, 1), (0, 2), (4, 2)]  # (0, 0): the planner's own rule
# geometries whose packed call may be refused (-21) and re-run packing inline, with the reason:
# none -- every tensor here is a 16-byte aligned channels-last activation and none is a
# full-kernel GEMM form
XFALLBACK_OK = {}


def _xid(g):
    return "%s%dx%d_%dx%d_k%ds%d%s" % ("T" if g[9] else "", g[1], g[4], g[2], g[3], g[5], g[6], "r" if g[8] else "")


@pytest.mark.parametrize("plan", XPLANS, ids=["ks%d_algo%d" % p for p in XPLANS])
@pytest.mark.parametrize("geom", XGEOMS, ids=[_xid(g) + "-" + str(i) for i, g in enumerate(XGEOMS)])
def test_prepacked_plan_cross(gpu, geom, plan, monkeypatch):
    import contextlib
    import tpgan_ops
    import tpgan_train
    from _cases import rel
    from _packcheck import image_is_fresh, live_view
    n, cin, h, w, cout, k, s, pad, reflect, transposed, op = geom
    gen = torch.Generator().manual_seed(cin * 131 + cout * 7 + k)
    x0 = (torch.rand(n, cin, h, w, generator=gen) * 2 - 1)
    wshape = (cin, cout, k, k) if transposed else (cout, cin, k, k)
    w0 = (torch.rand(*wshape, generator=gen) * 2 - 1) * (1.0 / (cin * k * k) ** 0.5)
    b0 = torch.rand(cout, generator=gen) * 0.1
    args = dict(stride=(s, s), pad=pad, pad_mode=tpgan_ops.PAD_REFLECT if reflect else tpgan_ops.PAD_ZERO,
                transposed=transposed, output_padding=(op, op))
    oh, ow = tpgan_ops.ConvGeom(k, k, **args).out_hw(h, w)
    gy0 = (torch.rand(n, cout, oh, ow, generator=gen) * 2 - 1).to(gpu).to(torch.bfloat16)
    calls = []

    def forced(lib, d, op_, device, launch):  # (the hook test_forced_data_split uses)
        d.data_ksplit, d.data_algo = plan
        calls.append(op_)
        return plan
    monkeypatch.setattr(tpgan_ops, "_tuned_data_split", forced)
    # (the weight-gradient tuner's timing sweeps have nothing to do with the images; its default plan)
    monkeypatch.setitem(tpgan_ops.AUTOTUNE, "enabled", False)
    assert tpgan_ops.CONCURRENT_HINT["enabled"] and not tpgan_ops.load().tpg_get_deterministic()

    def make(managed):
        conv = (torch.nn.ConvTranspose2d(cin, cout, k) if transposed else torch.nn.Conv2d(cin, cout, k)).to(gpu)
        with torch.no_grad():
            conv.weight.copy_(w0)
            conv.bias.copy_(b0)
        conv = conv.to(memory_format=torch.channels_last)
        return conv, (tpgan_train.FlatParams(conv, gpu) if managed else None)

    def run(conv, conc):
        x = x0.to(gpu).contiguous(memory_format=torch.channels_last).requires_grad_(True)
        with tpgan_ops.compute_dtype(torch.bfloat16), (tpgan_ops.concurrent() if conc else contextlib.nullcontext()):
            y = tpgan_ops.conv2d(x, conv.weight, conv.bias, act=torch.nn.LeakyReLU(0.01), **args)
            y.backward(gy0)
        torch.cuda.synchronize()
        return y.detach().float().cpu(), x.grad.float().cpu()

    plain, _ = make(False)
    inline = {conc: (run(plain, conc), run(plain, conc)) for conc in (False, True)}
    assert sorted(set(calls)) == [0, 1], calls  # forward and input gradient both took the plan
    exact = {conc: all(torch.equal(a, b) for a, b in zip(*inline[conc])) for conc in (False, True)}
    if s == 1 and not transposed:
        assert exact[False] and exact[True], "a stride-1 in-call path must reproduce bit for bit"

    # (pack-time flag, use-time flag): the same, packed inside concurrent() and used outside, the reverse
    for pack_conc, use_conc in ((False, False), (True, True), (True, False), (False, True)):
        tag = (_xid(geom), plan, "packed conc=%d, used conc=%d" % (pack_conc, use_conc))
        conv, flat = make(True)
        f0 = tpgan_ops.PACK["fallbacks"]
        got = run(conv, pack_conc)   # creates both entries and packs the images
        entries = [e for e in flat.pack_entries.values() if e is not None]
        assert sorted(e.op for e in entries) == [0, 1] and all(e.njobs and e.epoch == flat.epoch for e in entries), tag
        for e in entries:
            assert bool(e.desc.flags & tpgan_ops.FLAG_CONCURRENT) == pack_conc, tag
            assert (e.desc.data_ksplit, e.desc.data_algo) == (0, 0), tag  # (packed before the tuner's pick)
        bufs = [e.buf.data_ptr() for e in entries]
        if use_conc != pack_conc:
            got = run(conv, use_conc)  # the same images, consumed under the other flag
            assert [e.buf.data_ptr() for e in flat.pack_entries.values() if e is not None] == bufs, tag
        nfb = tpgan_ops.PACK["fallbacks"] - f0
        assert nfb == 0 or _xid(geom) in XFALLBACK_OK, tag + ("%d packed calls fell back to inline packing" % nfb,)
        want, again = inline[use_conc]
        for name, a, r, r2 in zip(("y", "dx"), got, want, again):
            if exact[use_conc]:
                assert torch.equal(a, r), tag + (name, float((a - r).abs().max()))
            else:
                dist, spread = rel(a, r), rel(r2, r)
                print("%s %s: packed-vs-inline %.3e, inline-vs-inline %.3e" % (tag, name, dist, spread))
                assert dist <= 4 * spread, tag + (name, dist, spread)
        for e in entries:
            wv = live_view(flat.params, e)
            assert wv is not None, tag + ("no live parameter at the entry's source",)
            ok, nw = image_is_fresh(tpgan_ops, e, wv)
            assert ok, tag + ("op %d image differs from a fresh pack under its stored descriptor" % e.op,)
            # ... and from one planned under the use-time descriptor: the layouts do not differ
            d_use = e.desc
            keep = (d_use.flags, d_use.data_ksplit, d_use.data_algo)
            d_use.flags = tpgan_ops.FLAG_CONCURRENT if use_conc else 0
            d_use.data_ksplit, d_use.data_algo = plan
            try:
                ok2, nw2 = image_is_fresh(tpgan_ops, e, wv)
            finally:
                d_use.flags, d_use.data_ksplit, d_use.data_algo = keep
            assert ok2 and nw2 == nw, tag + ("op %d image depends on the plan fields" % e.op,)
