"""Measure the inference path (tp-gan_amd/tpgan_infer.py) on the GPU.

    python tools/bench_infer.py [--batch 32] [--iters 20] [--raw 640x480] [--out profiles/r08/infer.txt]

Frontalizer in bf16 on a resident batch of synthetic raw WxH photos with synthetic landmarks:

  - the whole fz(imgs, lm68) call (LANCZOS resize, crops, Generator forward, denorm_u8): faces/s
    from HIP events around `iters` calls after 3 warm-up calls (which also pack the frozen
    weights and autotune the shapes), and from the host clock around the same calls and a
    synchronise;
  - the Generator forward alone on the batch FaceBatcher.from_raw made (events), beside the wall
    time of one bs32 training step recorded in profiles/r06/kernel_trace_final.txt (34.31 ms; the
    trace does not tell forward kernels from backward ones, the same kernels serve both, so the
    forward's share is this measurement over that step);
  - tpg_denorm_u8 on the forward's own output and tpg_image_metrics_u8 on the result against a
    second batch, each alone: events around `kiters` back-to-back launches, against the bytes
    the kernel has to move (HBM peak 8 TB/s, MI355X_MICROARCH.md).  Both are launch-latency
    sized at this batch; the --big line times them on 1024 faces, where the bytes dominate.

--identity runs the identity-scoring leg instead (profiles/r10/identity.txt), in one process:

  - tpgan_ops.cosine_topk at P = 4096 probes, D = 512, k = 5 against G = 16384 and G = 131072
    unit rows, and torch.matmul + torch.topk on the same rows (hipBLAS plus a P x G float32 matrix
    in memory) as the baseline: `rounds` rounds, each timing one then the other with HIP events
    around back-to-back calls, after both are warmed up; the median round is reported with the
    spread, the share of the 157 TF f32 matrix peak (2 P G D over the time) and the bytes of the
    similarity matrix the fused search never writes;
  - IdentityScorer.embed at B = 32 with the ResNet-18 back-end in bf16.

--detect runs the landmark-detector leg instead (profiles/r11/landmarks.txt), in one process, bf16,
B = 32 synthetic raw photos, after warm-up, HIP events and the host clock around each:

  - LandmarkDetector.detect (resize, u8_to_unit, MobileNetV2 + SSD head, ssd_landmarks, status read);
  - Frontalizer(imgs) with the detector attached and no landmarks given;
  - the decode-to-boxes step alone, tpgan_ops.ssd_landmarks as back-to-back launches, and as its
    baseline the route there was before it on the same tensors: MultiTaskDecoder()(loc, cls), the
    lists assembled into a host array, uploaded, FaceBatcher.landmark_boxes.

Prints one JSON line per measurement; --out also writes them to a file.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tp-gan_amd"))

TRAIN_STEP_MS_R06 = 34.31  # profiles/r06/kernel_trace_final.txt: wall span per bs32 G+D step


def events(fn, iters):
    s = torch.cuda.current_stream()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    e0.record(s)
    for _ in range(iters):
        fn()
    e1.record(s)
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters, (time.perf_counter() - t0) * 1e3 / iters


F32_MATRIX_PEAK = 157e12  # MI355X f32-input MFMA peak, FLOP/s (MI355X_MICROARCH.md)


def identity_leg(a, emit):
    import FeatureExtract as FE
    import tpgan_infer
    import tpgan_ops
    dev = torch.device("cuda", 0)
    P, D, k = 4096, 512, 5
    gen = torch.Generator(device=dev).manual_seed(0)
    probes, _ = tpgan_ops.l2_normalize(torch.randn(P, D, generator=gen, device=dev))
    for G, iters in ((16384, 200), (131072, 40)):
        gallery, _ = tpgan_ops.l2_normalize(torch.randn(G, D, generator=gen, device=dev))

        def fused():
            return tpgan_ops.cosine_topk(probes, gallery, k=k)

        def aten():
            return torch.topk(torch.matmul(probes, gallery.t()), k, dim=1)
        for _ in range(3):
            idx, score = fused()
            ref = aten()
        torch.cuda.synchronize()
        same = float((idx.long() == ref.indices).float().mean())
        dmax = float((score - ref.values).abs().max())
        t_f, t_a = [], []
        for _ in range(a.rounds):  # interleaved: the two forms alternate on the same box
            t_f.append(events(fused, iters)[0])
            t_a.append(events(aten, iters)[0])
        mf, ma = float(np.median(t_f)), float(np.median(t_a))
        flop = 2.0 * P * G * D
        emit({"op": "cosine_topk vs torch.matmul + torch.topk, f32 unit rows", "P": P, "G": G, "D": D, "k": k,
              "rounds": a.rounds, "calls_per_round": iters,
              "fused_ms": round(mf, 4), "fused_ms_min_max": [round(min(t_f), 4), round(max(t_f), 4)],
              "aten_ms": round(ma, 4), "aten_ms_min_max": [round(min(t_a), 4), round(max(t_a), 4)],
              "fused_over_aten": round(mf / ma, 4),
              "fused_TFLOPs": round(flop / (mf * 1e-3) / 1e12, 2),
              "fused_share_of_157TF_f32_matrix_peak": round(flop / (mf * 1e-3) / F32_MATRIX_PEAK, 4),
              "similarity_matrix_bytes_not_written": P * G * 4,
              "indices_equal_to_aten": round(same, 6), "max_abs_score_diff": dmax,
              "note": "fused time is both launches (search + merge) of the whole call; aten time is the GEMM "
                      "and the top-k over the stored P x G matrix"})
        del gallery, ref
    torch.manual_seed(0)
    scorer = tpgan_infer.IdentityScorer(FE.FeatureExtractModel("resnet"), device=dev, compute_dtype=torch.bfloat16)
    B = 32
    faces = torch.randint(0, 256, (B, 128, 128, 3), dtype=torch.uint8, device=dev)
    for _ in range(3):
        scorer.embed(faces)
    torch.cuda.synchronize()
    ms, wall = events(lambda: scorer.embed(faces), a.iters)
    emit({"op": "IdentityScorer.embed (u8 128x128x3 -> unit f32 [B, 512]), ResNet-18 back-end, bf16", "batch": B,
          "ms_per_batch": round(ms, 3), "ms_per_batch_host_clock": round(wall, 3),
          "faces_per_s": round(B / (ms * 1e-3), 1)})


def detect_leg(a, emit):
    import D_and_G_model as DG
    import MobileNetV2 as MN
    import tpgan_infer
    import tpgan_ops
    from DataAndDataset import FaceBatcher
    dev = torch.device("cuda", 0)
    w, h = (int(v) for v in a.raw.lower().split("x"))
    B = a.batch
    rng = np.random.default_rng(0)
    imgs = [torch.from_numpy(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)).to(dev) for _ in range(B)]
    torch.manual_seed(0)
    # untrained weights: no score reaches a confidence threshold, so every landmark takes its best
    # anchor (on_missing="best"); the work per call is that of a trained detector
    det = tpgan_infer.LandmarkDetector(MN.MobileNetV2(), device=dev, compute_dtype=torch.bfloat16, max_batch=B,
                                       on_missing="best")
    fz = tpgan_infer.Frontalizer(DG.Generator(64, 347, use_batchnorm=False), device=dev, compute_dtype=torch.bfloat16,
                                 max_batch=B, detector=det)
    for _ in range(3):
        d = det.detect(imgs)
        fz(imgs)
    torch.cuda.synchronize()
    iters, kiters = max(a.iters, 100), max(a.kiters, 2000)  # windows of a few hundred ms and of ~30 ms

    def rounds(fn, n):
        t = [events(fn, n) for _ in range(a.rounds)]
        ev, wl = [x[0] for x in t], [x[1] for x in t]
        return float(np.median(ev)), float(np.median(wl)), [round(min(ev), 4), round(max(ev), 4)]
    ms, wall, mm = rounds(lambda: det.detect(imgs), iters)
    emit({"op": "LandmarkDetector.detect (raw %dx%d photos -> points, boxes, status), bf16" % (w, h), "batch": B,
          "rounds": a.rounds, "calls_per_round": iters, "ms_per_batch": round(ms, 3), "ms_per_batch_min_max": mm,
          "ms_per_batch_host_clock": round(wall, 3), "faces_per_s": round(B / (ms * 1e-3), 1),
          "note": "ends with the one status read of the batch"})
    ms, wall, mm = rounds(lambda: fz(imgs), iters)
    emit({"op": "Frontalizer.__call__ with the detector, no landmarks given (raw %dx%d -> u8 128x128x3), bf16" % (w, h),
          "batch": B, "rounds": a.rounds, "calls_per_round": iters, "ms_per_batch": round(ms, 3),
          "ms_per_batch_min_max": mm, "ms_per_batch_host_clock": round(wall, 3),
          "faces_per_s": round(B / (ms * 1e-3), 1)})

    # the decode-to-boxes step alone, on the head outputs of the same photos
    with torch.no_grad():
        loc, cls = det._head(d["u8_128"])
    n = loc.shape[1]
    conf = 0.0  # both routes then decode a point for every class of every face
    for _ in range(5):
        fused = tpgan_ops.ssd_landmarks(loc, cls, conf)
    torch.cuda.synchronize()

    dec = MN.MultiTaskDecoder(confidence_threshold=conf, top_k=1)
    fb4 = FaceBatcher(dev, pts_idx=[[0, 0], [1, 1], [2, 2], [3, 3], [3, 3]], check=False)

    def today():
        out = dec(loc, cls)  # tpg_ssd_decode, keep / score to the host, lists of tuples per image
        pts = torch.stack([torch.stack([p for c, _, p in res if c < 4]) for res in out])
        host = pts.cpu().numpy().astype(np.float32)  # the landmark array reassembled on the host ...
        return fb4.landmark_boxes(torch.from_numpy(host).to(dev))  # ... uploaded again, then the box kernel
    for _ in range(3):
        base = today()
    torch.cuda.synchronize()
    same = bool(torch.equal(base[1], fused[3]))
    t_f, t_b = [], []
    for _ in range(a.rounds):  # interleaved: the two routes alternate on the same box
        t_f.append(events(lambda: tpgan_ops.ssd_landmarks(loc, cls, conf), kiters))
        t_b.append(events(today, iters))
    ms, wall = (float(np.median([x[i] for x in t_f])) for i in (0, 1))
    bms, bwall = (float(np.median([x[i] for x in t_b])) for i in (0, 1))
    line = {"op": "decode to crop boxes: tpg_ssd_landmarks, back-to-back launches", "batch": B, "anchors": n,
            "rounds": a.rounds, "calls_per_round": kiters, "us_per_call": round(ms * 1e3, 2),
            "us_per_call_min_max": [round(min(x[0] for x in t_f) * 1e3, 2), round(max(x[0] for x in t_f) * 1e3, 2)],
            "us_per_call_host_clock": round(wall * 1e3, 2), "device_to_host_copies": 0}
    line.update({"baseline_calls_per_round": iters,
                 "baseline_us_per_call_min_max": [round(min(x[0] for x in t_b) * 1e3, 2),
                                                  round(max(x[0] for x in t_b) * 1e3, 2)],
                 "baseline": "MultiTaskDecoder()(loc, cls) -> lists -> host array -> upload -> FaceBatcher.landmark_boxes",
                 "baseline_us_per_call": round(bms * 1e3, 2), "baseline_us_per_call_host_clock": round(bwall * 1e3, 2),
                 "baseline_over_fused_host_clock": round(bwall / wall, 2), "boxes_equal": same})
    emit(line)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--kiters", type=int, default=200)
    ap.add_argument("--raw", default="640x480", metavar="WxH")
    ap.add_argument("--big", type=int, default=1024, help="faces of the kernels-alone line")
    ap.add_argument("--identity", action="store_true", help="the identity-scoring leg instead of the image path")
    ap.add_argument("--rounds", type=int, default=5, help="interleaved rounds of the identity leg")
    ap.add_argument("--detect", action="store_true", help="the landmark-detector leg instead of the image path")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_infer.py needs a ROCm GPU (there is no CPU path)")
    if a.identity or a.detect:
        lines = []

        def emit_id(d):
            lines.append(json.dumps(d))
            print(lines[-1], flush=True)
        (identity_leg if a.identity else detect_leg)(a, emit_id)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                f.write("\n".join(lines) + "\n")
        return
    import D_and_G_model as DG
    import tpgan_infer
    import tpgan_ops

    dev = torch.device("cuda", 0)
    w, h = (int(v) for v in a.raw.lower().split("x"))
    B = a.batch
    rng = np.random.default_rng(0)
    imgs = [torch.from_numpy(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)).to(dev) for _ in range(B)]
    lm = torch.from_numpy((rng.random((B, 68, 2)) * 0.5 + 0.25).astype(np.float32) * np.float32([w, h])).to(dev)
    torch.manual_seed(0)
    fz = tpgan_infer.Frontalizer(DG.Generator(64, 347, use_batchnorm=False), device=dev, compute_dtype=torch.bfloat16,
                                 max_batch=B)
    lines = []

    def emit(d):
        lines.append(json.dumps(d))
        print(lines[-1], flush=True)

    for _ in range(3):
        out = fz(imgs, lm)
    torch.cuda.synchronize()
    ms, wall = events(lambda: fz(imgs, lm), a.iters)
    emit({"op": "Frontalizer.__call__ (raw %dx%d photos -> u8 128x128x3), bf16" % (w, h), "batch": B,
          "ms_per_batch": round(ms, 3), "ms_per_batch_host_clock": round(wall, 3),
          "faces_per_s": round(B / (ms * 1e-3), 1)})

    batch = fz._batcher().from_raw(imgs, lm)
    z = torch.zeros(B, 64, device=dev)
    G = fz.G

    def fwd():
        with torch.no_grad(), tpgan_ops.compute_dtype(torch.bfloat16):
            return G(batch["I128"], batch["left_eye"], batch["right_eye"], batch["nose"], batch["mouth"], z, False)[0]
    for _ in range(3):
        x = fwd()
    torch.cuda.synchronize()
    ms, _ = events(fwd, a.iters)
    emit({"op": "Generator.forward alone (frozen, packed-once weights), bf16", "batch": B, "ms_per_batch": round(ms, 3),
          "faces_per_s": round(B / (ms * 1e-3), 1), "train_step_ms_bs32_r06": TRAIN_STEP_MS_R06,
          "forward_over_train_step": round(ms * (32.0 / B) / TRAIN_STEP_MS_R06, 4),
          "note": "profiles/r06/kernel_trace_final.txt does not separate forward from backward kernels; "
                  "the share is this forward over that step's wall time"})

    other = torch.from_numpy(rng.integers(0, 256, (B, 128, 128, 3), dtype=np.uint8)).to(dev)
    for tag, n in (("batch", B), ("big", a.big)):
        xs = x  # the forward's output: a channels-last view, pixel stride 8
        if n != B:  # the same layout, more faces
            xs = tpgan_ops.new_act(n, 3, 128, 128, x.dtype, dev)
            xs.copy_(torch.rand(n, 3, 128, 128, device=dev) * 2 - 1)
        u = tpgan_ops.denorm_u8(xs)
        v = other if n == B else torch.randint(0, 256, (n, 128, 128, 3), dtype=torch.uint8, device=dev)
        for _ in range(5):
            tpgan_ops.denorm_u8(xs)
            tpgan_ops.image_metrics(u, v)
        torch.cuda.synchronize()
        ms, _ = events(lambda: tpgan_ops.denorm_u8(xs), a.kiters)
        nbytes = n * 128 * 128 * 3 * (xs.element_size() + 1)
        emit({"op": "tpg_denorm_u8 (%s [N,3,128,128] channels-last view -> u8)" % str(xs.dtype).split(".")[-1],
              "faces": n, "us_per_call": round(ms * 1e3, 2), "bytes": nbytes,
              "GB_per_s": round(nbytes / (ms * 1e-3) / 1e9, 1), "frac_of_8TBps": round(nbytes / (ms * 1e-3) / 8e12, 4),
              "note": "algorithmic bytes (3 channels in, 3 bytes out); the view's pixel stride is %d elements, so "
                      "the loads touch every cache line of the buffer" % xs.stride(3)})
        ms, _ = events(lambda: tpgan_ops.image_metrics(u, v), a.kiters)
        nbytes = 2 * n * 128 * 128 * 3
        emit({"op": "tpg_image_metrics_u8 (SSE + SSIM, two launches, u8 [N,128,128,3] x 2)", "faces": n,
              "us_per_call": round(ms * 1e3, 2), "bytes": nbytes, "GB_per_s": round(nbytes / (ms * 1e-3) / 1e9, 1),
              "faces_per_s": round(n / (ms * 1e-3), 1)})
    # the validation call end to end: the same photos scored against the first run's result (split-K
    # atomics reorder sums outside deterministic mode, so the two runs may differ in a few bytes)
    for _ in range(2):
        r = fz.evaluate(imgs, lm, out)
    torch.cuda.synchronize()
    ms, wall = events(lambda: fz.evaluate(imgs, lm, out), a.iters)
    emit({"op": "Frontalizer.evaluate (the call above + SSE / PSNR / SSIM against u8 frontals)", "batch": B,
          "ms_per_batch": round(ms, 3), "ms_per_batch_host_clock": round(wall, 3),
          "faces_per_s": round(B / (ms * 1e-3), 1), "rerun_vs_first_run_min_psnr_db": float(r["psnr"].min()),
          "rerun_vs_first_run_min_ssim": float(r["ssim"].min())})
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
