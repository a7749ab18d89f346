#!/usr/bin/env python3
"""Time-series throughput: gnm.connectome.connectivity_from_timeseries and mean_bold_features (csrc/timeseries.hip:
column means, fp64 matrix-core Gram of the upper blocks, normalisation) next to the host route they replace,
np.corrcoef(ts[s], rowvar=False) per subject.  One JSON line per (S, T, dtype); times are wall-clock medians.
    python tools/bench_timeseries.py [--S 256,1024] [--T 1200,4800] [--n 400] [--reps 5] [--out FILE]
    python tools/bench_timeseries.py --stats KERNEL_STATS.csv --S 1024 --T 1200 [--out FILE]
Per case: the device kernels on a resident [S, T, n] stack (means alone, means + Gram + normalise), the achieved fp64
rate of the Gram (S n (n + 1) / 2 T multiply-adds, 2 flop each, over the means + Gram + normalise time, so a floor of
the kernel's own rate), the end-to-end time from a pinned host array with its upload timed separately (stacks up to
--upload-max-gb), and host np.corrcoef timed on --host-sample subjects and scaled to S.  The second form reads the
kernel-stats CSV of `rocprofv3 --kernel-trace --stats --output-format csv -- python tools/bench_timeseries.py ...` (at
ONE S and T) and prints per-kernel times; the Gram's line carries its fp64 TFLOP/s against the 78.6 TFLOP/s fp64
matrix figure of the MI355X."""
import argparse
import csv
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "graph-neural-mapping_amd"))
import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--S", default="256,1024")
ap.add_argument("--T", default="1200,4800")
ap.add_argument("--n", type=int, default=400)
ap.add_argument("--dtypes", default="float64,float32")
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--host-sample", type=int, default=8, help="subjects np.corrcoef is timed on (0: skip)")
ap.add_argument("--upload-max-gb", type=float, default=4.0)
ap.add_argument("--stats", default=None, help="summarise this rocprofv3 kernel-stats CSV instead of timing")
ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
args = ap.parse_args()
PEAK_F64 = 78.6e12
lines = []


def emit(rec):
    lines.append(rec)
    print(json.dumps(rec), flush=True)


def med(ts):
    return 1e3 * float(np.median(ts))


if args.stats:
    S, T, n = int(args.S.split(",")[0]), int(args.T.split(",")[0]), args.n
    flop = 2.0 * S * (n * (n + 1) / 2) * T     # upper triangle, diagonal included: one multiply-add = 2 flop
    with open(args.stats) as f:
        for row in csv.DictReader(f):
            name = row["Name"]
            if "gnm_ts_" not in name:
                continue
            big = float(row["MaxNs"]) * 1e-9                   # the S-subject launches (warm-ups are 2 subjects)
            rec = {"bench": "timeseries_kernel", "kernel": name, "calls": int(row["Calls"]),
                   "avg_us": float(row["AverageNs"]) / 1e3, "min_us": float(row["MinNs"]) / 1e3, "max_us": big * 1e6,
                   "S": S, "T": T, "n": n}
            if "gram" in name:
                rec.update(tflops=flop / big / 1e12, frac_of_f64_matrix_peak=flop / big / PEAK_F64)
            emit(rec)
else:
    import torch
    from gnm import connectome as C

    dev = torch.device("cuda:0")
    n = args.n
    for S in [int(x) for x in args.S.split(",")]:
        for T in [int(x) for x in args.T.split(",")]:
            for dname in args.dtypes.split(","):
                dt = getattr(torch, dname)
                g = torch.Generator(device=dev).manual_seed(S + T)
                ts = torch.randn((S, T, n), generator=g, device=dev, dtype=dt) * 50 + 1e4
                C.connectivity_from_timeseries(ts[:2])                      # warm-up (launch configuration)
                C.mean_bold_features(ts[:2])
                x, t_off, _, _ = C._as_timeseries(ts, dev)
                mean_t, fc_t, feat_t = [], [], []
                for _ in range(args.reps):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    mean = C._ts_means(x, t_off, S, n)
                    torch.cuda.synchronize()
                    t1 = time.perf_counter()
                    fc = C._ts_fc(x, t_off, mean, S, n)
                    torch.cuda.synchronize()
                    t2 = time.perf_counter()
                    C._ts_zscores(mean, S, n, torch.float32)
                    torch.cuda.synchronize()
                    t3 = time.perf_counter()
                    mean_t.append(t1 - t0); fc_t.append(t2 - t0); feat_t.append(t3 - t2)
                    del fc
                flop = 2.0 * S * (n * (n + 1) / 2) * T
                rec = {"bench": "timeseries", "route": "device, resident", "S": S, "T": T, "n": n, "dtype": dname,
                       "reps": args.reps, "means_ms": med(mean_t), "fc_ms": med(fc_t), "zscores_ms": med(feat_t),
                       "gram_tflops_floor": flop / float(np.median(fc_t)) / 1e12}
                nbytes = ts.element_size() * ts.numel()
                if nbytes <= args.upload_max_gb * 1e9:
                    host = torch.empty(ts.shape, dtype=dt, pin_memory=True)
                    host.copy_(ts)
                    up_t, e2e_t = [], []
                    for _ in range(max(1, args.reps // 2)):
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        d = host.to(dev, non_blocking=True)
                        torch.cuda.synchronize()
                        up_t.append(time.perf_counter() - t0)
                        del d
                        t0 = time.perf_counter()
                        C.connectivity_from_timeseries(host, device=dev)
                        torch.cuda.synchronize()
                        e2e_t.append(time.perf_counter() - t0)
                    rec.update(upload_gb=nbytes / 1e9, upload_ms=med(up_t), host_to_fc_ms=med(e2e_t))
                    del host
                if args.host_sample > 0 and dname == "float64":
                    k = min(S, args.host_sample)
                    sample = ts[:k].cpu().numpy()
                    t0 = time.perf_counter()
                    for s in range(k):
                        np.corrcoef(sample[s], rowvar=False)
                    per = (time.perf_counter() - t0) / k
                    rec.update(host_corrcoef_ms_per_subject=1e3 * per, host_corrcoef_ms_x_S=1e3 * per * S,
                               speedup_fc=per * S / float(np.median(fc_t)))
                emit(rec)
                del ts, x, t_off, mean
                torch.cuda.empty_cache()
if args.out:
    with open(args.out, "a") as f:
        for rec in lines:
            f.write(json.dumps(rec) + "\n")
