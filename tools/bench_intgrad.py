#!/usr/bin/env python3
"""Integrated-gradients throughput: GIN_InfoMaxReg.integrated_gradients(graphs, (0, 1), steps=K) -- every (graph, step)
pair as a virtual graph over the source graph's adjacency (csrc/intgrad.hip) -- next to the route without it, timed in
its two parts: (a) building the K rescaled copies of every subject on the host and registering them in the arena, (b)
model.saliency() on the registered copies at the same K, then the weighted sum and the (X - x') product in torch.
400-node dense connectivity graphs at L = 5, m = 2, H = 64, for F0 = 7 and one-hot F0 = 400, zero baseline, midpoint
rule.  One JSON line per (F0, route); times are medians of --reps runs after a warm-up.
    python tools/bench_intgrad.py [--subjects 8] [--steps 32] [--reps 5] [--f0 7,400] [--no-parent] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "graph-neural-mapping_amd"))

ap = argparse.ArgumentParser()
ap.add_argument("--subjects", type=int, default=8)
ap.add_argument("--n", type=int, default=400)
ap.add_argument("--steps", type=int, default=32)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--f0", default="7,400")
ap.add_argument("--no-parent", action="store_true", help="time the device route only")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "intgrad_bench.jsonl"),
                help="append the JSON lines to this file")
args = ap.parse_args()
H, L, M = 64, 5, 2
lines = []

import torch
from gnm import synth
from gnm.intgrad import quadrature
from models.graphcnn import GIN_InfoMaxReg

dev = torch.device("cuda:0")


def emit(rec):
    lines.append(rec)
    print(json.dumps(rec), flush=True)


class Copy:
    pass


def rescaled_copy(g, a):
    c = Copy()
    c.g, c.label, c.edge_mat = g.g, g.label, g.edge_mat
    c.node_features = float(a) * g.node_features
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


K, S = args.steps, args.subjects
alphas, weights = quadrature("midpoint", K)
for f0 in [int(x) for x in args.f0.split(",")]:
    graphs = [synth.dense_fc_graph(g, n=args.n) for g in range(S)]
    if f0 == args.n:
        for g in graphs:
            g.node_features = torch.eye(args.n)
    torch.manual_seed(0)
    model = GIN_InfoMaxReg(L, M, f0, H, 2, 0.5, True, "sum", "sum", dev).to(dev)
    got = model.integrated_gradients(graphs, (0, 1), steps=K)            # warm-up (registers the graphs, loads the code)
    t = timed(lambda: model.integrated_gradients(graphs, (0, 1), steps=K), args.reps)
    emit(dict(route="integrated_gradients", f0=f0, n=args.n, subjects=S, steps=K, H=H, L=L, ms=round(t * 1e3, 3),
              ms_per_subject=round(t / S * 1e3, 3), us_per_virtual_graph=round(t / (S * K) * 1e6, 3)))
    if args.no_parent:
        continue
    # the route without the method: (a) K host copies per subject + arena registration, (b) saliency() on them
    t0 = time.perf_counter()
    copies = [rescaled_copy(g, a) for g in graphs for a in alphas]
    t1 = time.perf_counter()
    model.arena().add_many(copies)
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    w = torch.as_tensor(weights, dtype=torch.float32, device=dev).view(1, 1, K, 1, 1)
    X = torch.stack([g.node_features for g in graphs]).to(dev)

    def parent():
        sal = model.saliency(copies, (0, 1), batch_size=S * K)           # [2, S K, n, F0]
        return (sal.view(2, S, K, args.n, f0) * w).sum(2) * X

    ref = parent()                                                       # warm-up
    tp = timed(parent, args.reps)
    scale = float(ref.abs().max())
    emit(dict(route="saliency_on_copies", f0=f0, n=args.n, subjects=S, steps=K, H=H, L=L,
              host_copy_ms_per_subject=round((t1 - t0) / S * 1e3, 3), register_ms_per_subject=round((t2 - t1) / S * 1e3, 3),
              saliency_ms=round(tp * 1e3, 3), saliency_ms_per_subject=round(tp / S * 1e3, 3),
              speedup_over_saliency=round(tp / t, 2), max_diff_rel=float((got - ref).abs().max()) / scale))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        for rec in lines:
            f.write(json.dumps(rec) + "\n")
