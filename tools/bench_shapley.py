#!/usr/bin/env python3
"""Shapley throughput: GIN_InfoMaxReg.shapley() -- every coalition of a labelling's groups as a virtual lesion described
by 4 bytes (csrc/shapley.hip gnm_coalition_pack in front of csrc/lesion.hip's forward, gnm_shapley_exact /
gnm_shapley_permutation behind it) -- next to its yardstick IN THE SAME RUN: lesion() on the same coalitions given as
explicit bool masks (the coalition that keeps no node left out: lesion() does not take it).  400-node dense connectivity
graphs at L = 5, m = 2, H = 64, for F0 = 7 and one-hot F0 = 400; 8 subjects, both classes; exact K = 7 and K = 12 (50
unlabelled nodes) and permutation K = 400 (one player per node), M = 8.  One JSON line per (F0, case); times are medians
after a warm-up, in microseconds per COALITION scored.  `call`: the whole method (base forward, host arrays, uploads,
the forward, for shapley() the reduction too); `device`: gnm/attribution.py shapley_hip / lesion_hip alone on the registered
batch; `reduce`: the reduction kernel alone on the scores.
    python tools/bench_shapley.py [--subjects 8] [--reps 5] [--f0 7,400] [--cases exact7,exact12,perm400] [--out FILE]"""
import argparse
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
ap.add_argument("--cases", default="exact7,exact12,perm400")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "shapley_bench.jsonl"),
                help="the JSON lines are written here (the file is replaced)")
args = ap.parse_args()
H, L, M_MLP, PERMS = 64, 5, 2, 8
lines = []


def emit(rec):
    lines.append(rec)
    print(json.dumps(rec), flush=True)


import torch
from gnm import attribution, synth
from gnm import shapley as sh
from models.graphcnn import GIN_InfoMaxReg

dev = torch.device("cuda:0")


def timed(fn, reps):
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t)
    return statistics.median(ts)


def labelling(K, n):
    """one player per node at K = n; otherwise random groups with 50 unlabelled (background) nodes"""
    if K == n:
        return np.arange(n)
    rng = np.random.default_rng(K)
    lab = rng.integers(0, K, n)
    lab[rng.permutation(n)[:50]] = -1
    return lab


for f0 in [int(x) for x in args.f0.split(",")]:
    graphs = [synth.dense_fc_graph(g, n=args.n) for g in range(args.subjects)]
    if f0 == args.n:
        for g in graphs:
            g.node_features = torch.eye(args.n)
    torch.manual_seed(0)
    model = GIN_InfoMaxReg(L, M_MLP, f0, H, 2, 0.5, True, "sum", "sum", dev).to(dev)
    model.eval()
    names, tensors, buffers = model._param_lists()
    P = dict(zip(names, tensors))
    P.update(buffers)
    batch = model._batch_of(graphs)
    X = batch.arena.features(batch).detach()
    G = args.subjects
    for case in args.cases.split(","):
        exact = case.startswith("exact")
        K = int(case[5:]) if exact else int(case[4:])
        lab = labelling(K, args.n)
        if exact:
            kw, ranks = dict(method="exact"), None
            ids = np.arange(1 << K, dtype=np.int64)
            removed = sh.coalition_removed(lab, ids)
        else:
            perms = sh.draw_permutations(PERMS, K, seed=0)
            kw, ranks = dict(method="permutation", permutations=perms), sh.ranks_of(perms)
            mj = [(0, j) for j in range(K + 1)] + [(m, j) for m in range(1, PERMS) for j in range(1, K)]
            ids = np.array([m * (K + 1) + j for m, j in mj], dtype=np.int64)
            pr = sh.prefix_removed(lab, perms)
            removed = np.stack([pr[m, j] for m, j in mj])
        masks = removed[~removed.all(1)]                                  # lesion() takes no set that removes every node
        V, Vl = G * ids.shape[0], G * masks.shape[0]
        model.shapley(graphs, (0, 1), lab, **kw)                          # warm-up
        t_call = timed(lambda: model.shapley(graphs, (0, 1), lab, **kw), args.reps)
        model.lesion(graphs, (0, 1), masks)
        t_les = timed(lambda: model.lesion(graphs, (0, 1), masks), args.reps)
        # the device parts alone, on the registered batch
        rows = np.tile(lab[None, :], (G, 1))
        vgraph = np.repeat(np.arange(G, dtype=np.int32), ids.shape[0])
        all_ids = np.tile(ids, G)
        t_dev = timed(lambda: attribution.shapley_hip(model._spec, batch, X, P, [0, 1], rows, vgraph, all_ids, K, ranks),
                      args.reps)
        rem = np.tile(masks, (G, 1)).astype(np.uint8)
        vg_l = np.repeat(np.arange(G, dtype=np.int32), masks.shape[0])
        t_ldev = timed(lambda: attribution.lesion_hip(model._spec, batch, X, P, [0, 1], rem, vg_l), args.reps)
        if exact:
            vals = torch.randn((2, G, 1 << K), device=dev)
            t_red = timed(lambda: attribution.shapley_exact_hip(vals, K, interactions=True), args.reps)
        else:
            vals = torch.randn((2, G, PERMS, K + 1), device=dev)
            t_red = timed(lambda: attribution.shapley_permutation_hip(vals, ranks), args.reps)
        us = lambda t, v: round(t / v * 1e6, 3)                           # noqa: E731
        emit(dict(case=case, f0=f0, n=args.n, subjects=G, K=K, H=H, L=L, coalitions=V, lesion_sets=Vl,
                  shapley_call_ms=round(t_call * 1e3, 3), shapley_call_us=us(t_call, V),
                  lesion_call_ms=round(t_les * 1e3, 3), lesion_call_us=us(t_les, Vl),
                  call_ratio=round((t_call / V) / (t_les / Vl), 3),
                  shapley_hip_us=us(t_dev, V), lesion_hip_us=us(t_ldev, Vl),
                  device_ratio=round((t_dev / V) / (t_ldev / Vl), 3), reduce_ms=round(t_red * 1e3, 3)))
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    for rec in lines:
        f.write(json.dumps(rec) + "\n")
