#!/usr/bin/env python3
"""Class-activation-map throughput: graphs per second of GIN_InfoMaxReg.class_activation(graphs, (0, 1), kind) -- the
batched per-node maps of csrc/cam.hip (kind="activation") and csrc/saliency.hip's gnm_saliency_maps (kind="gradient")
-- next to the per-graph loops a user of the reference would run, on 400-node dense connectivity graphs at L = 5, m = 2,
H = 64, for F0 = 7 and one-hot F0 = 400.  One JSON line per (F0, kind, route); a "graph" is both classes of one graph.
The per-graph baselines are lower bounds of what a per-graph map costs: the eval forward([g]) for the activation kind
(the map needs the hidden layers on top of it) and compute_saliency([g], c) for both classes for the gradient kind (the
map needs every layer's h.grad on top of it).
    python tools/bench_class_activation.py [--B 256] [--reps 5] [--loop-graphs 32] [--f0 7,400] [--out FILE]
    python tools/bench_class_activation.py --stats KERNEL_STATS.csv [--B 256] [--out FILE]
The second form reads a `rocprofv3 --kernel-trace --stats` table of a run of the first and prints, per kernel of the
feature, calls and mean time, and for gnm_class_activation_kernel its algorithmic bytes (4 N H L of z) as a fraction of
8 TB/s."""
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
ap.add_argument("--B", type=int, default=256)
ap.add_argument("--n", type=int, default=400)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--loop-graphs", type=int, default=32)
ap.add_argument("--f0", default="7,400")
ap.add_argument("--stats", default=None, help="summarise this rocprofv3 kernel-stats CSV instead of timing")
ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
args = ap.parse_args()
H, L, M = 64, 5, 2
lines = []


def emit(rec):
    lines.append(rec)
    print(json.dumps(rec), flush=True)


if args.stats:
    with open(args.stats) as f:
        for row in csv.DictReader(f):
            name = row["Name"]
            if "gnm_class_activation_kernel" in name or "gnm_saliency_layer_kernel<true>" in name:
                avg = float(row["AverageNs"])
                rec = {"bench": "class_activation_kernel", "kernel": name, "calls": int(row["Calls"]),
                       "avg_us": avg / 1e3, "min_us": float(row["MinNs"]) / 1e3, "max_us": float(row["MaxNs"]) / 1e3}
                if "gnm_class_activation_kernel" in name:
                    nbytes = 4.0 * args.B * args.n * H * L
                    rec.update(B=args.B, n=args.n, H=H, L=L, algorithmic_bytes=nbytes,
                               frac_of_8TBps=nbytes / (avg * 1e-9) / 8e12)
                emit(rec)
else:
    import torch
    from gnm import synth
    from models.graphcnn import GIN_InfoMaxReg

    dev = torch.device("cuda:0")
    base = synth.make_pool("dense_fc", args.B, n=args.n, f0=7)
    for f0 in [int(x) for x in args.f0.split(",")]:
        graphs = base
        if f0 != 7:
            assert f0 == args.n, "one_hot features: F0 = n"
            graphs = [synth.SynthGraph(args.n, np.zeros((0, 2), np.int64), np.eye(args.n, dtype=np.float32), g.label)
                      for g in base]
            for g, src in zip(graphs, base):
                g.edge_mat = src.edge_mat
        torch.manual_seed(0)
        model = GIN_InfoMaxReg(L, M, f0, H, 2, 0.5, True, "sum", "sum", dev).to(dev).eval()
        for kind in ("activation", "gradient"):
            model.class_activation(graphs, (0, 1), kind=kind)           # warm-up: arena, allocator, code objects
            torch.cuda.synchronize()
            ts = []
            for _ in range(args.reps):
                t0 = time.perf_counter()
                model.class_activation(graphs, (0, 1), kind=kind)
                torch.cuda.synchronize()
                ts.append(time.perf_counter() - t0)
            t = float(np.median(ts))
            emit({"bench": "class_activation", "kind": kind, "route": "batched", "B": args.B, "n": args.n, "F0": f0,
                  "H": H, "L": L, "m": M, "classes": 2, "median_s": t, "graphs_per_s": args.B / t,
                  "us_per_graph": 1e6 * t / args.B, "reps": args.reps})
        G = min(args.loop_graphs, len(graphs))
        with torch.no_grad():
            for g in graphs[:2]:
                model([g])
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for g in graphs[:G]:
                model([g])
            torch.cuda.synchronize()
            t = time.perf_counter() - t0
        emit({"bench": "class_activation", "kind": "activation", "route": "per_graph_forward", "B": G, "n": args.n,
              "F0": f0, "H": H, "L": L, "m": M, "total_s": t, "us_per_graph": 1e6 * t / G})
        for g in graphs[:2]:
            model.compute_saliency([g], 0)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for g in graphs[:G]:
            for c in (0, 1):
                model.compute_saliency([g], c)
        torch.cuda.synchronize()
        t = time.perf_counter() - t0
        emit({"bench": "class_activation", "kind": "gradient", "route": "per_graph_compute_saliency", "B": G,
              "n": args.n, "F0": f0, "H": H, "L": L, "m": M, "classes": 2, "total_s": t, "us_per_graph": 1e6 * t / G})
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        for r in lines:
            f.write(json.dumps(r) + "\n")
