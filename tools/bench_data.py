"""Measure the device data path against the HBM roofline.

    python tools/bench_data.py [--batch 256] [--iters 50]

FaceBatcher on a resident batch: tpg_landmark_boxes + tpg_crop_normalize (image + 4 patches,
float32 NCHW outputs).  Algorithmic bytes per face: the 128x128x3 u8 image read once (49,152 B)
+ the float32 image written (196,608 B) + the four float32 patches written ((40*40*2 + 40*32 +
48*32) * 3 * 4 = 72,192 B) = 317,952 B; landmarks (544 B in, 224 B out) are counted too.
Timed with HIP events on the launch stream; peak 8 TB/s (MI355X_MICROARCH.md).

    python tools/bench_data.py --raw [WxH] [--batch 256] [--iters 50]      (default 640x480)

FaceBatcher.resize (tpg_resize_u8) of a resident batch of raw WxH photos to 128x128 against the
only other way to get those bytes, PIL's Image.resize(..., Image.LANCZOS) on the host with a pool
of 16 threads (the CPUs one command is given, not os.cpu_count()).  Algorithmic bytes per face:
the raw image read once (W*H*3) + the 128x128x3 output written (49,152 B), and, stated
separately, the intermediate image H*128*3 written by the pass along W and read by the pass
along H.  The device time is a whole resize() call (job records built and uploaded, two
launches), from HIP events around `iters` calls after 3 warm-up calls and from the host clock
around the same calls and a synchronise.  The host figure is the best of 5 passes over the batch.
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tp-gan_amd"))


HOST_THREADS = 16


def bench_raw(a, DD, dev):
    import time
    import numpy as np
    w, h = (int(v) for v in a.raw.lower().split("x"))
    B = a.batch
    rng = np.random.default_rng(0)
    host = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for _ in range(B)]
    imgs = [torch.from_numpy(x).to(dev) for x in host]
    fb = DD.FaceBatcher(dev, check=False)
    for _ in range(3):
        out = fb.resize(imgs)
    torch.cuda.synchronize()
    s = torch.cuda.current_stream()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    e0.record(s)
    for _ in range(a.iters):
        out = fb.resize(imgs)
    e1.record(s)
    torch.cuda.synchronize()
    wall_ms = (time.perf_counter() - t0) * 1e3 / a.iters
    ms = e0.elapsed_time(e1) / a.iters
    io, mid = w * h * 3 + 128 * 128 * 3, 2 * h * 128 * 3 if (w != 128 and h != 128) else 0
    gbs = (io + mid) * B / (ms * 1e-3) / 1e9
    res = {"op": "FaceBatcher.resize (tpg_resize_u8, LANCZOS, %dx%d -> 128x128)" % (w, h), "batch": B,
           "ms_per_batch": round(ms, 4), "ms_per_batch_host_clock": round(wall_ms, 4),
           "faces_per_s": round(B / (ms * 1e-3), 1),
           "roofline": {"bound": "hbm", "achieved": round(gbs, 1), "peak": 8000.0, "unit": "GB/s",
                        "frac": round(gbs / 8000.0, 4), "bytes_per_face": io + mid,
                        "bytes_per_face_raw_read_plus_output": io, "bytes_per_face_intermediate_write_plus_read": mid}}
    try:
        from PIL import Image
    except ImportError:
        res["host_pil"] = "skipped: PIL is not installed here"
    else:
        from concurrent.futures import ThreadPoolExecutor
        pil = [Image.fromarray(x) for x in host]
        ref = np.asarray(pil[0].resize((128, 128), Image.LANCZOS))
        res["device_equals_pil"] = bool((out[0].cpu().numpy() == ref).all())
        best = float("inf")
        with ThreadPoolExecutor(HOST_THREADS) as pool:
            for _ in range(6):  # the first pass warms the pool up
                t0 = time.perf_counter()
                list(pool.map(lambda im: im.resize((128, 128), Image.LANCZOS), pil))
                dt = time.perf_counter() - t0
                best = min(best, dt) if _ else best
        res["host_pil"] = {"threads": HOST_THREADS, "ms_per_batch": round(best * 1e3, 3),
                           "faces_per_s": round(B / best, 1), "pil_version": Image.__version__}
        res["device_over_host"] = round((B / (ms * 1e-3)) / (B / best), 2)
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--raw", nargs="?", const="640x480", default=None, metavar="WxH",
                    help="measure FaceBatcher.resize of raw WxH photos against 16-thread PIL (default 640x480)")
    a = ap.parse_args()
    import DataAndDataset as DD
    dev = torch.device("cuda", 0)
    if a.raw:
        return bench_raw(a, DD, dev)
    g = torch.Generator(device="cpu").manual_seed(0)
    B = a.batch
    img = torch.randint(0, 256, (B, 128, 128, 3), generator=g, dtype=torch.uint8).to(dev)
    lm = (torch.rand(B, 68, 2, generator=g) * 100 + 14).to(dev)
    fb = DD.FaceBatcher(dev, check=False)
    for _ in range(3):
        fb(img, lm)
    torch.cuda.synchronize()
    s = torch.cuda.current_stream()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(s)
    for _ in range(a.iters):
        fb(img, lm)
    e1.record(s)
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / a.iters
    per_face = 49152 + 196608 + 72192 + 544 + 224
    gbs = per_face * B / (ms * 1e-3) / 1e9
    print(json.dumps({"op": "FaceBatcher (tpg_landmark_boxes + tpg_crop_normalize)", "batch": B,
                      "ms_per_batch": round(ms, 4), "faces_per_s": round(B / (ms * 1e-3), 1),
                      "roofline": {"bound": "hbm", "achieved": round(gbs, 1), "peak": 8000.0, "unit": "GB/s",
                                   "frac": round(gbs / 8000.0, 4), "bytes_per_face": per_face}}))


if __name__ == "__main__":
    main()
