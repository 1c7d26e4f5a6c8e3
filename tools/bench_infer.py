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

--align runs the face-alignment leg instead (profiles/r12/align.txt), in one process, bf16, B = 32
synthetic raw photos of four different sizes, after warm-up, HIP events and the host clock, the
median of `rounds` interleaved rounds with the spread:

  - LandmarkDetector.detect(imgs) and LandmarkDetector.detect(imgs, aligner=...): the front end with
    one pass and with fit + warp + a second pass (an untrained detector: the points are wherever
    its best anchors are, the work per call is that of a trained one);
  - FaceAligner.align alone on planted points (the template under a tilt of up to 20 degrees, the
    face 45 % of the photo's width), then tpgan_ops.similarity_fit and tpgan_ops.affine_warp_u8
    alone as back-to-back calls, with the sub-sampling factors the matrices gave.
  --commit names the tree the numbers are from; the first line records it and the device.

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


ALIGN_TEMPLATE = [[44.0, 52.0], [84.0, 52.0], [64.0, 76.0], [64.0, 98.0]]  # a plausible frame, not a measured one


def align_leg(a, emit):
    import MobileNetV2 as MN
    import tpgan_infer
    import tpgan_ops
    dev = torch.device("cuda", 0)
    B = a.batch
    sizes = [(480, 640), (640, 480), (768, 1024), (300, 250)]  # (H, W), cycled over the batch
    rng = np.random.default_rng(0)
    hw = [sizes[i % len(sizes)] for i in range(B)]
    imgs = [torch.from_numpy(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)).to(dev) for h, w in hw]
    emit({"device": torch.cuda.get_device_name(0), "hip": torch.version.hip, "commit": a.commit, "batch": B,
          "photo_sizes_hw": sizes, "compute_dtype": "bf16"})
    torch.manual_seed(0)
    det = tpgan_infer.LandmarkDetector(MN.MobileNetV2(), device=dev, compute_dtype=torch.bfloat16, max_batch=B,
                                       on_missing="best")
    al = tpgan_infer.FaceAligner(ALIGN_TEMPLATE, device=dev)
    iters, kiters = max(a.iters, 100), max(a.kiters, 2000)

    def rounds(fns, n):
        """Interleaved rounds of the given calls -> per call (median events ms, median host ms, [min, max])."""
        t = [[] for _ in fns]
        for _ in range(a.rounds):
            for k, fn in enumerate(fns):
                t[k].append(events(fn, n))
        return [(float(np.median([x[0] for x in r])), float(np.median([x[1] for x in r])),
                 [round(min(x[0] for x in r), 4), round(max(x[0] for x in r), 4)]) for r in t]

    # planted points: the template's 128 x 128 frame scaled to 45 % of the photo's width, tilted
    q = np.asarray(ALIGN_TEMPLATE, np.float64)
    pts = []
    for h, w in hw:
        s, th = 0.45 * w / 128.0, np.deg2rad(rng.uniform(-20, 20))
        r = np.array([[np.cos(th), -np.sin(th)], [np.sin(th), np.cos(th)]])
        pts.append(s * (q - q.mean(0)) @ r.T + [0.5 * w, 0.45 * h])
    pts = torch.from_numpy(np.stack(pts).astype(np.float32)).to(dev)
    for _ in range(5):
        res = al.align(imgs, pts)
    torch.cuda.synchronize()
    assert res["status"].tolist() == [0] * B
    mq = res["matrix_q16"]
    n_of = []
    for m in mq.reshape(B, 6).tolist():
        d = max(m[0] * m[0] + m[3] * m[3], m[1] * m[1] + m[4] * m[4])
        n_of.append(next(n for n in range(1, 17) if (n * 65536) ** 2 >= d))
    (ms_a, wall_a, mm_a), (ms_f, wall_f, mm_f), (ms_w, wall_w, mm_w) = rounds(
        [lambda: al.align(imgs, pts), lambda: tpgan_ops.similarity_fit(pts, al.template),
         lambda: tpgan_ops.affine_warp_u8(imgs, mq)], kiters)
    out_bytes = B * 128 * 128 * 3
    taps = sum(n * n for n in n_of) * 128 * 128 * 4
    emit({"op": "FaceAligner.align (fit + warp, mixed-size photos -> u8 128x128x3), planted points", "batch": B,
          "rounds": a.rounds, "calls_per_round": kiters, "us_per_call": round(ms_a * 1e3, 2),
          "us_per_call_min_max": [round(v * 1e3, 2) for v in mm_a], "us_per_call_host_clock": round(wall_a * 1e3, 2),
          "faces_per_s": round(B / (ms_a * 1e-3), 1), "subsampling_n_per_photo": sorted(set(n_of)),
          "device_to_host_copies": 0})
    emit({"op": "tpg_similarity_fit alone, back-to-back calls", "batch": B, "calls_per_round": kiters,
          "us_per_call": round(ms_f * 1e3, 2), "us_per_call_min_max": [round(v * 1e3, 2) for v in mm_f],
          "us_per_call_host_clock": round(wall_f * 1e3, 2)})
    emit({"op": "tpg_affine_warp_u8 alone (job table upload + one launch), back-to-back calls", "batch": B,
          "calls_per_round": kiters, "us_per_call": round(ms_w * 1e3, 2),
          "us_per_call_min_max": [round(v * 1e3, 2) for v in mm_w], "us_per_call_host_clock": round(wall_w * 1e3, 2),
          "out_bytes": out_bytes, "bilinear_taps": taps, "Gtaps_per_s": round(taps / (ms_w * 1e-3) / 1e9, 1),
          "note": "events span the host's record packing and upload too: at this size the call is bound by them "
                  "when the host clock equals the event time"})

    # the warp kernel alone: the job table resident, the output reused, the C entry point called directly
    import ctypes
    import tpgan_lib as L
    lib = L.load()
    jb = lib.tpg_warp_job_bytes()
    jobs = (ctypes.c_uint8 * (B * jb))()
    for i, t in enumerate(imgs):
        L.check(lib.tpg_warp_pack_job(jobs, i, t.data_ptr(), t.shape[0], t.shape[1], 3, t.stride(0), 128, 128))
    jobs_dev = torch.frombuffer(jobs, dtype=torch.uint8).to(dev)
    out = torch.empty(B, 128, 128, 3, dtype=torch.uint8, device=dev)
    wst = torch.empty(B, dtype=torch.int32, device=dev)
    args = (B, jobs_dev.data_ptr(), mq.data_ptr(), 128, 128, out.data_ptr(), wst.data_ptr(), L.stream_ptr())

    def kernel():
        lib.tpg_affine_warp_u8(*args)
    for _ in range(5):
        kernel()
    torch.cuda.synchronize()
    assert torch.equal(out, res["u8"])
    (ms_k, wall_k, mm_k), = rounds([kernel], kiters)
    emit({"op": "affine_warp_kernel alone (resident job table, C entry point, back-to-back launches)", "batch": B,
          "calls_per_round": kiters, "us_per_launch": round(ms_k * 1e3, 2),
          "us_per_launch_min_max": [round(v * 1e3, 2) for v in mm_k], "us_per_launch_host_clock": round(wall_k * 1e3, 2),
          "blocks": 64 * B, "bilinear_taps": taps, "Gtaps_per_s": round(taps / (ms_k * 1e-3) / 1e9, 1),
          "note": "an upper bound of the kernel time: launches queue back to back, so when the host clock equals "
                  "the event time this too is the host's launch rate"})

    # the front end with one pass and with two
    for _ in range(3):
        det.detect(imgs)
    try:
        for _ in range(3):
            d = det.detect(imgs, aligner=al)
    except ValueError as e:  # the untrained detector put a face's four points on one spot: no timing to report
        emit({"op": "LandmarkDetector.detect with the aligner", "error": str(e)})
        (ms, wall, mm), = rounds([lambda: det.detect(imgs)], iters)
        emit({"op": "LandmarkDetector.detect (mixed-size photos -> points, boxes, status), bf16", "batch": B,
              "rounds": a.rounds, "calls_per_round": iters, "ms_per_batch": round(ms, 3), "ms_per_batch_min_max": mm,
              "ms_per_batch_host_clock": round(wall, 3)})
        return
    torch.cuda.synchronize()
    (ms, wall, mm), (ms2, wall2, mm2) = rounds([lambda: det.detect(imgs), lambda: det.detect(imgs, aligner=al)], iters)
    emit({"op": "LandmarkDetector.detect (mixed-size photos -> points, boxes, status), bf16", "batch": B,
          "rounds": a.rounds, "calls_per_round": iters, "ms_per_batch": round(ms, 3), "ms_per_batch_min_max": mm,
          "ms_per_batch_host_clock": round(wall, 3), "faces_per_s": round(B / (ms * 1e-3), 1)})
    emit({"op": "LandmarkDetector.detect(imgs, aligner) (detect, fit, warp, detect again), bf16", "batch": B,
          "rounds": a.rounds, "calls_per_round": iters, "ms_per_batch": round(ms2, 3), "ms_per_batch_min_max": mm2,
          "ms_per_batch_host_clock": round(wall2, 3), "faces_per_s": round(B / (ms2 * 1e-3), 1),
          "over_one_pass": round(ms2 / ms, 3), "align_status_or": int(d["align_status"].max()),
          "note": "ends with the one read of the three status arrays"})


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
    ap.add_argument("--align", action="store_true", help="the face-alignment leg instead of the image path")
    ap.add_argument("--commit", default="unknown", help="the tree the numbers are from (recorded by --align)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_infer.py needs a ROCm GPU (there is no CPU path)")
    if a.identity or a.detect or a.align:
        lines = []

        def emit_id(d):
            lines.append(json.dumps(d))
            print(lines[-1], flush=True)
        (identity_leg if a.identity else detect_leg if a.detect else align_leg)(a, emit_id)
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
