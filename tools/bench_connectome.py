#!/usr/bin/env python3
"""Connectome-builder throughput: gnm.connectome.graphs_from_connectivity -- thresholds, edges, node order and arena
CSR built on the device (csrc/connectome.hip) -- next to the host route it replaces: dense_fc-style numpy thresholding
(np.percentile, np.triu, np.nonzero per subject, gnm/synth.py) followed by GraphArena.add_many, on the same [S, n, n]
fp64 correlation matrices.  One JSON line per (S, route); times are wall-clock medians from matrices resident where
the route wants them (device for the device build, host for numpy) to graphs registered in a fresh arena.
    python tools/bench_connectome.py [--S 256,1024] [--n 400] [--sparsity 30] [--reps 5] [--out FILE]
    python tools/bench_connectome.py --stats KERNEL_STATS.csv [--S 1024] [--out FILE]
The second form reads a `rocprofv3 --kernel-trace --stats` table of a run of the first (at ONE S) and prints, per
gnm_connectome kernel, calls and times (max: the S-subject launches), with the bytes each launch reads at least (thresholds: 9 passes over the
n^2 fp64 values; structure: the upper triangle once) against 8 TB/s."""
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
ap.add_argument("--n", type=int, default=400)
ap.add_argument("--sparsity", type=float, default=30)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--host-reps", type=int, default=1)
ap.add_argument("--stats", default=None, help="summarise this rocprofv3 kernel-stats CSV instead of timing")
ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
args = ap.parse_args()
HBM = 8e12
lines = []


def emit(rec):
    lines.append(rec)
    print(json.dumps(rec), flush=True)


if args.stats:
    S, n = int(args.S.split(",")[0]), args.n
    floor_bytes = {"thr": 8.0 * n * n * S * 9, "structure": 8.0 * n * (n - 1) / 2 * S, "emit": None}
    with open(args.stats) as f:
        for row in csv.DictReader(f):
            name = row["Name"]
            if "gnm_connectome" not in name:
                continue
            big = float(row["MaxNs"]) * 1e-9            # the S-subject launches (the warm-up ones are 2 subjects)
            rec = {"bench": "connectome_kernel", "kernel": name, "calls": int(row["Calls"]),
                   "avg_us": float(row["AverageNs"]) / 1e3, "min_us": float(row["MinNs"]) / 1e3, "max_us": big * 1e6,
                   "S": S, "n": n}
            for key, nb in floor_bytes.items():
                if key + "_kernel" in name and nb:
                    rec.update(bytes_read_min=nb, max_us_frac_of_8TBps=nb / big / HBM)
            emit(rec)
else:
    import torch
    from gnm.arena import GraphArena
    from gnm.connectome import connectivity_thresholds, graphs_from_connectivity
    from gnm.synth import SynthGraph

    dev = torch.device("cuda:0")
    n, sp = args.n, args.sparsity
    sp = int(sp) if float(sp).is_integer() else sp
    for S in [int(x) for x in args.S.split(",")]:
        g = torch.Generator(device=dev).manual_seed(S)
        ts = torch.randn((S, 256, n), generator=g, device=dev, dtype=torch.float64)
        ts = ts - ts.mean(1, keepdim=True)
        ts = ts / ts.norm(dim=1, keepdim=True)
        fc = torch.bmm(ts.transpose(1, 2), ts).contiguous()              # [S, n, n] correlation matrices
        del ts
        feats = torch.randn((n, 7), generator=g, device=dev)
        labels = [s % 2 for s in range(S)]
        graphs_from_connectivity(GraphArena(dev), fc[:2], sp, feats, labels[:2])  # warm-up (launch configuration)
        thr_t, dev_t = [], []
        for _ in range(args.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            connectivity_thresholds(fc, sp)
            torch.cuda.synchronize()
            thr_t.append(time.perf_counter() - t0)
            ar = GraphArena(dev)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            gs = graphs_from_connectivity(ar, fc, sp, feats, labels)
            torch.cuda.synchronize()
            dev_t.append(time.perf_counter() - t0)
        nnz = int(np.sum(ar.nnz))
        emit({"bench": "connectome", "route": "device", "S": S, "n": n, "sparsity": sp, "reps": args.reps,
              "ms": 1e3 * float(np.median(dev_t)), "thresholds_ms": 1e3 * float(np.median(thr_t)),
              "us_per_subject": 1e6 * float(np.median(dev_t)) / S, "directed_edges": nnz})
        if args.host_reps > 0:                                         # 0: the device route alone (kernel traces)
            fch, fh = fc.cpu().numpy(), feats.cpu().numpy()
            host_t, prep_t = [], []
            for _ in range(args.host_reps):
                t0 = time.perf_counter()
                hs = []
                for s in range(S):
                    m = fch[s]
                    iu, ju = np.nonzero(np.triu(m > np.percentile(m, 100 - sp), 1))
                    hs.append(SynthGraph(n, np.stack([iu, ju], 1), fh, labels[s]))
                t1 = time.perf_counter()
                har = GraphArena(dev)
                har.add_many(hs)
                torch.cuda.synchronize()
                host_t.append(time.perf_counter() - t0)
                prep_t.append(t1 - t0)
            assert int(np.sum(har.nnz)) == nnz
            emit({"bench": "connectome", "route": "host numpy + add_many", "S": S, "n": n, "sparsity": sp,
                  "reps": args.host_reps, "ms": 1e3 * float(np.median(host_t)),
                  "threshold_ms": 1e3 * float(np.median(prep_t)), "us_per_subject": 1e6 * float(np.median(host_t)) / S,
                  "speedup_device": float(np.median(host_t)) / float(np.median(dev_t))})
        del fc, gs, ar
        torch.cuda.empty_cache()
if args.out:
    with open(args.out, "a") as f:
        for rec in lines:
            f.write(json.dumps(rec) + "\n")
