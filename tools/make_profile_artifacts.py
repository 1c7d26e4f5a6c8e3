"""Turn one tools/gpu_r2pmc.sh run (gpurun_out/<tag>) into the committed evidence under
profiles/<round>/: the bench line, PMC calibration, HBM traffic of the dominant kernels,
SQ MFMA utilisation, and the kernel-trace summary with the dominant kernel's forward-only
average (to compare with the bench's HIP-event average).

    python tools/make_profile_artifacts.py gpurun_out/r02 profiles/r02
"""
import csv
import glob
import json
import os
import shutil
import statistics
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import prof_summary as PS  # noqa: E402

E128_FLOPS = 2 * 32 * 128 * 128 * 206 * 206 * 25
E128_FWD_BYTES = 650141768  # x + residual in, y out (206 ch, bf16), weights
E128_WGRAD_BYTES = 2 * (32 * 128 * 128 * 206 * 2) + 206 * 206 * 25 * 4  # dY + X in, dW (fp32) out


def counters(d, kernel_sub, grid=None):
    out = {}
    for fn in glob.glob(os.path.join(d, "**", "*counter_collection.csv"), recursive=True):
        with open(fn) as f:
            for r in csv.DictReader(f):
                if kernel_sub not in r["Kernel_Name"]:
                    continue
                if grid and int(r.get("Grid_Size", 0) or 0) != grid:
                    continue
                out.setdefault(r["Counter_Name"], []).append(float(r["Counter_Value"]))
    return {k: statistics.median(v) for k, v in out.items()}, {k: len(v) for k, v in out.items()}


def main():
    src, dst = sys.argv[1], sys.argv[2]
    os.makedirs(dst, exist_ok=True)
    # bench line (of a `bench.py --full` run: its roofline object is used below)
    with open(os.path.join(src, "bench.log")) as f:
        line = [ln for ln in f if ln.startswith("{")][-1]
    bench = json.loads(line)
    with open(os.path.join(dst, "bench.json"), "w") as f:
        json.dump(bench, f, indent=1)
    # calibration: known byte counts of tools/pmc_calib.hip
    known = {"wr16": 512 << 20, "wr2": 512 << 20, "wr16_row": (512 << 20) // 416 * 412, "rd16": 512 << 20,
             "rd16_lds": 512 << 20}
    cal = {}
    for k, b in known.items():
        w, _ = counters(os.path.join(src, "cal_write"), k + "(")
        r, _ = counters(os.path.join(src, "cal_fetch"), k + "(")
        cal[k] = {"known_bytes": b, "WRITE_SIZE_bytes": w.get("WRITE_SIZE", 0) * 1024,
                  "FETCH_SIZE_bytes": r.get("FETCH_SIZE", 0) * 1024}
        cal[k]["write_ratio"] = cal[k]["WRITE_SIZE_bytes"] / b
        cal[k]["fetch_ratio"] = cal[k]["FETCH_SIZE_bytes"] / b
    cal["_note"] = ("tools/pmc_calib.hip: each kernel touches a known byte count of a 512 MiB buffer (2x the "
                    "Infinity Cache). WRITE_SIZE reads 16-B and 2-B stores exactly; FETCH_SIZE reads 16-B loads "
                    "(plain and LDS-DMA) at 1/2 -> the x2 correction (MI355X_MICROARCH.md, HBM section).")
    with open(os.path.join(dst, "pmc_calibration.json"), "w") as f:
        json.dump(cal, f, indent=1)
    # dominant kernel forward: only forward dispatches (grid filter; bench_layers --passes fwd)
    fe, nf = counters(os.path.join(src, "e128_fetch"), "halo_kernel", 1048576)
    wr, nw = counters(os.path.join(src, "e128_write"), "halo_kernel", 1048576)
    fetch_b, write_b = fe["FETCH_SIZE"] * 1024 * 2, wr["WRITE_SIZE"] * 1024
    dom = {"kernel": "halo_kernel<bf16,4,208,8,1> forward, enhance_features_128 (206->206 5x5, 128x128, bs32, "
                     "+residual)",
           "source": "rocprofv3 --kernel-trace --pmc FETCH_SIZE / WRITE_SIZE (separate runs) of "
                     "tools/bench_layers.py --only enhance_128 --passes fwd --iters 3; grid 1048576 only",
           "dispatches": [nf.get("FETCH_SIZE", 0), nw.get("WRITE_SIZE", 0)],
           "raw_fetch_kb_median": fe["FETCH_SIZE"], "raw_write_kb_median": wr["WRITE_SIZE"],
           "fetch_bytes": fetch_b, "write_bytes": write_b, "traffic_bytes": fetch_b + write_b,
           "correction": "FETCH_SIZE x2, WRITE_SIZE x1 (profiles/<round>/pmc_calibration.json); KB = 1024 B",
           "algorithmic_bytes": E128_FWD_BYTES,
           "algorithmic_write_bytes": 32 * 128 * 128 * 206 * 2,
           "write_over_output": write_b / (32 * 128 * 128 * 206 * 2),
           "traffic_over_algorithmic": (fetch_b + write_b) / E128_FWD_BYTES,
           "note": "WRITE_SIZE = the 208-channel-stride output exactly (whole 64-B lines of 206 live channels); "
                   "FETCH_SIZE above the 434 MB of x + residual: halo re-reads of neighbouring tiles (5x5, "
                   "4-row tiles) that miss the per-XCD L2"}
    with open(os.path.join(dst, "pmc_enhance128_fwd.json"), "w") as f:
        json.dump(dom, f, indent=1)
    shutil.copy(os.path.join(dst, "pmc_enhance128_fwd.json"), os.path.join(os.path.dirname(dst.rstrip("/")),
                                                                          "pmc_dominant.json"))
    # weight gradient of the same layer
    wf, _ = counters(os.path.join(src, "wg_fetch"), "wgrad_rh_kernel")
    ww, _ = counters(os.path.join(src, "wg_write"), "wgrad_rh_kernel")
    l2, _ = counters(os.path.join(src, "l2"), "wgrad_rh_kernel") if os.path.isdir(os.path.join(src, "l2")) else ({}, {})
    wg = {"kernel": "wgrad_rh_kernel (tile chosen by bench_layers' default planner), enhance_128 weight gradient",
          "fetch_bytes": wf.get("FETCH_SIZE", 0) * 2048, "write_bytes": ww.get("WRITE_SIZE", 0) * 1024,
          "algorithmic_bytes": E128_WGRAD_BYTES,
          "note": "write = fp32 atomics of the pixel splits into dW (exact for one-dword atomics)"}
    wg["traffic_over_algorithmic"] = (wg["fetch_bytes"] + wg["write_bytes"]) / E128_WGRAD_BYTES
    with open(os.path.join(dst, "pmc_enhance128_wgrad.json"), "w") as f:
        json.dump(wg, f, indent=1)
    # SQ passes
    sq = subprocess.run([sys.executable, os.path.join(HERE, "sq_summary.py"),
                         "--pass", "fwd", os.path.join(src, "sq_fwd"), os.path.join(src, "sq2_fwd"),
                         "--pass", "dgrad", os.path.join(src, "sq_dgrad"), os.path.join(src, "sq2_dgrad"),
                         "--pass", "wgrad", os.path.join(src, "sq_wgrad"), os.path.join(src, "sq2_wgrad"),
                         "--out", os.path.join(dst, "sq_mfma.json")], capture_output=True, text=True)
    with open(os.path.join(dst, "sq_mfma.txt"), "w") as f:
        f.write(sq.stdout)
    # kernel trace of the bench step
    trace = os.path.join(src, "prof", "run_kernel_trace.csv")
    steps = 10
    summ = subprocess.run([sys.executable, os.path.join(HERE, "prof_summary.py"), trace, "--steps", str(steps),
                           "--top", "60", "--csv", os.path.join(dst, "kernel_stats_window.csv")],
                          capture_output=True, text=True).stdout
    rows, _ = PS.window(PS.load(trace), steps)
    adam = [i for i, r in enumerate(rows) if "adam_kernel" in r[2]]
    fwd = []
    start = 0
    for a in adam[1::2] + [len(rows)]:  # per step (each ends with the G Adam)
        seq = [r for r in rows[start:a] if "halo_kernel<1, 4, 208, 8, 1" in r[2]]
        fwd += [(r[1] - r[0]) / 1e6 for r in seq[:2]]  # the step's first two: enhance_128 forwards
        start = a
    with open(os.path.join(dst, "kernel_trace_summary.txt"), "w") as f:
        f.write("rocprofv3 --kernel-trace --stats -- python3 bench.py --steps 10 --warmup 5 --no-cpu-baseline\n")
        f.write("window: the last %d steps (tools/prof_summary.py)\n\n" % steps)
        f.write(summ)
        f.write("\ndominant kernel, forward launches only (first two halo_kernel<1,4,208,8,1> per step): "
                "%d launches, average %.4f ms -> %.1f TF/s; bench.py's HIP-event average over its timed "
                "steps: %.4f ms\n" % (len(fwd), statistics.mean(fwd), E128_FLOPS / statistics.mean(fwd) / 1e9,
                                      bench["roofline"]["avg_launch_ms"]))
    for fn in ("run_kernel_stats.csv", "run_domain_stats.csv"):
        p = os.path.join(src, "prof", fn)
        if os.path.exists(p):
            shutil.copy(p, os.path.join(dst, "rocprof_" + fn.replace("run_", "")))
    print(open(os.path.join(dst, "kernel_trace_summary.txt")).read()[-400:])


if __name__ == "__main__":
    main()
