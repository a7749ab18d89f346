#!/usr/bin/env python3
"""Per-ROI occlusion throughput: GIN_InfoMaxReg.occlusion(graphs, (0, 1)) -- every node-deleted copy of a graph as a
virtual graph over the source graph's bit adjacency (csrc/occlusion.hip) -- next to the route without it, timed in its
two parts: (a) building the n node-deleted copies of a subject on the host and registering them in the arena, (b)
model.predict() on the registered copies.  400-node dense connectivity graphs at L = 5, m = 2, H = 64, for F0 = 7 and
one-hot F0 = 400.  One JSON line per (F0, route); times are medians after a warm-up, per VIRTUAL graph (one deleted
copy, both classes).
    python tools/bench_occlusion.py [--subjects 8] [--reps 5] [--f0 7,400] [--no-parent] [--out FILE]
    python tools/bench_occlusion.py --stats KERNEL_STATS.csv [--subjects 8] [--out FILE]
The second form reads a `rocprofv3 --kernel-trace --stats` table of a run of the first and prints, for the layer
kernels, calls and mean time against their two floors per launch of `subjects` graphs: HBM bytes (each virtual graph's
[n, H] activations read once and written once: 8 n^2 H per subject and layer; layer 0 only writes) at 8 TB/s, and the
split-bf16 products (per virtual graph: aggregation 3 x 2 x 32 W x 16 ceil(n / 16) x H, Linears 6 x 2 x 32 W x H^2
each, W = ceil(n / 32)) at 2.5 PFLOP/s."""
import argparse
import csv
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "graph-neural-mapping_amd"))
import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--subjects", type=int, default=8)
ap.add_argument("--n", type=int, default=400)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--f0", default="7,400")
ap.add_argument("--no-parent", action="store_true", help="time the device route only")
ap.add_argument("--stats", default=None, help="summarise this rocprofv3 kernel-stats CSV instead of timing")
ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
args = ap.parse_args()
H, L, M = 64, 5, 2
HBM, BF16 = 8e12, 2.5e15
lines = []


def emit(rec):
    lines.append(rec)
    print(json.dumps(rec), flush=True)


def finish():
    if args.out:
        with open(args.out, "a") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if args.stats:
    n, S = args.n, args.subjects
    W, ks = (n + 31) // 32, (n + 15) // 16
    agg = 3 * 2 * 32 * W * 16 * ks * H
    lin = 6 * 2 * 32 * W * H * H
    floors = {"<true>": (4 * n * n * H * S, (M - 1) * lin * n * S),           # layer 0: writes only, no aggregation
              "<false>": (8 * n * n * H * S, (agg + M * lin) * n * S)}
    for row in csv.DictReader(open(args.stats)):
        name = row.get("Name") or row.get("KernelName") or ""
        for key, (nbytes, flops) in floors.items():
            if "gnm_occlusion_layer_kernel" in name and key in name:
                mean_us = float(row.get("AverageNs") or row.get("Average") or 0) / 1e3
                emit(dict(kernel=name.split("(")[0], calls=int(float(row.get("Calls") or 0)), mean_us=round(mean_us, 2),
                          hbm_floor_us=round(nbytes / HBM * 1e6, 2), mfma_floor_us=round(flops / BF16 * 1e6, 2),
                          frac_hbm=round(nbytes / HBM * 1e6 / mean_us, 3) if mean_us else None,
                          frac_mfma=round(flops / BF16 * 1e6 / mean_us, 3) if mean_us else None, subjects=S, n=n))
    finish()
    sys.exit(0)

import torch
from gnm import synth
from models.graphcnn import GIN_InfoMaxReg

dev = torch.device("cuda:0")


class Copy:
    pass


def deleted_copy(g, v):
    """g without node v: edges at v dropped, the later nodes renumbered, the other feature rows kept"""
    em = g.edge_mat.numpy()
    em = em[:, (em != v).all(0)]
    c = Copy()
    c.g = list(range(len(g.g) - 1))
    c.label = g.label
    c.edge_mat = torch.from_numpy(np.ascontiguousarray(em - (em > v)))
    c.node_features = torch.cat([g.node_features[:v], g.node_features[v + 1:]], 0)
    return c


def timed(fn, reps):
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t)
    return statistics.median(ts)


for f0 in [int(x) for x in args.f0.split(",")]:
    graphs = [synth.dense_fc_graph(g, n=args.n) for g in range(args.subjects)]
    if f0 == args.n:
        for g in graphs:
            g.node_features = torch.eye(args.n)
    torch.manual_seed(0)
    model = GIN_InfoMaxReg(L, M, f0, H, 2, 0.5, True, "sum", "sum", dev).to(dev)
    V = args.subjects * args.n
    model.occlusion(graphs, (0, 1))                                      # warm-up (registers the graphs, loads the code)
    t = timed(lambda: model.occlusion(graphs, (0, 1)), args.reps)
    emit(dict(route="occlusion", f0=f0, n=args.n, subjects=args.subjects, H=H, L=L, ms=round(t * 1e3, 3),
              us_per_virtual_graph=round(t / V * 1e6, 3), ms_per_subject=round(t / args.subjects * 1e3, 3)))
    if args.no_parent:
        continue
    # the route without the method, one subject (n copies): (a) host copies + arena registration, (b) predict on them
    g = graphs[0]
    t0 = time.perf_counter()
    copies = [deleted_copy(g, v) for v in range(args.n)]
    t1 = time.perf_counter()
    model.arena().add_many(copies)
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    model.predict(copies)                                                # warm-up
    tp = timed(lambda: model.predict(copies), args.reps)
    emit(dict(route="copies", f0=f0, n=args.n, subjects=1, H=H, L=L, host_copy_us_per_virtual_graph=round((t1 - t0) / args.n * 1e6, 1),
              register_us_per_virtual_graph=round((t2 - t1) / args.n * 1e6, 1),
              predict_us_per_virtual_graph=round(tp / args.n * 1e6, 3), predict_ms_per_subject=round(tp * 1e3, 3),
              occlusion_speedup_over_predict=round(tp / args.n / (t / V), 2)))
finish()
