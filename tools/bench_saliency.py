#!/usr/bin/env python3
"""Saliency throughput (main.py:60-68's workload): graphs per second of GIN_InfoMaxReg.saliency(graphs, (0, 1)) -- the
batched eval-mode input gradient, csrc/saliency.hip -- next to the per-graph compute_saliency loop main.py runs, on 400-node
dense connectivity graphs at L = 5, m = 2, H = 64, for F0 = 7 and one_hot F0 = 400.  One JSON line per (F0, route).
A "graph" is both classes of one graph in both routes.
    python tools/bench_saliency.py [--B 256] [--reps 5] [--loop-graphs 32] [--f0 7,400] [--out FILE]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "graph-neural-mapping_amd"))
import numpy as np
import torch

ap = argparse.ArgumentParser()
ap.add_argument("--B", type=int, default=256)
ap.add_argument("--n", type=int, default=400)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--loop-graphs", type=int, default=32)
ap.add_argument("--f0", default="7,400")
ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
args = ap.parse_args()

from gnm import synth
from models.graphcnn import GIN_InfoMaxReg

dev = torch.device("cuda:0")
base = synth.make_pool("dense_fc", args.B, n=args.n, f0=7)
lines = []
for f0 in [int(x) for x in args.f0.split(",")]:
    graphs = base
    if f0 != 7:
        assert f0 == args.n, "one_hot features: F0 = n"
        graphs = [synth.SynthGraph(args.n, np.zeros((0, 2), np.int64), np.eye(args.n, dtype=np.float32), g.label)
                  for g in base]
        for g, src in zip(graphs, base):
            g.edge_mat = src.edge_mat
    torch.manual_seed(0)
    model = GIN_InfoMaxReg(5, 2, f0, 64, 2, 0.5, True, "sum", "sum", dev).to(dev).eval()
    model.saliency(graphs, (0, 1))                                   # warm-up: arena, allocator, code objects
    torch.cuda.synchronize()
    ts = []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        model.saliency(graphs, (0, 1))
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    t = float(np.median(ts))
    rec = {"bench": "saliency", "route": "batched", "kernel_route": model.saliency_routes[0], "B": args.B, "n": args.n,
           "F0": f0, "H": 64, "L": 5, "m": 2, "classes": 2, "median_s": t, "graphs_per_s": args.B / t,
           "us_per_graph": 1e6 * t / args.B, "reps": args.reps}
    lines.append(rec)
    print(json.dumps(rec), flush=True)
    G = min(args.loop_graphs, len(graphs))
    for g in graphs[:2]:
        model.compute_saliency([g], 0)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for g in graphs[:G]:
        for c in (0, 1):
            model.compute_saliency([g], c)
    torch.cuda.synchronize()
    t = time.perf_counter() - t0
    rec = {"bench": "saliency", "route": "per_graph_compute_saliency", "B": G, "n": args.n, "F0": f0, "H": 64, "L": 5,
           "m": 2, "classes": 2, "total_s": t, "graphs_per_s": G / t, "us_per_graph": 1e6 * t / G,
           "ms_per_call": 1e3 * t / (2 * G)}
    lines.append(rec)
    print(json.dumps(rec), flush=True)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        for r in lines:
            f.write(json.dumps(r) + "\n")
