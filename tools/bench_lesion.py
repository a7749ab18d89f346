#!/usr/bin/env python3
"""Set-lesion throughput: GIN_InfoMaxReg.lesion(graphs, (0, 1), sets) -- every (graph, removed set) pair as a virtual
graph over the source graph's bit adjacency under a keep mask (csrc/lesion.hip) -- next to the route without it, timed
in its parts: (a) building the set-deleted copies on the host, (b) registering them in the arena, (c) model.predict() on
the registered copies (one call per set size: a batch holds graphs of one node count).  400-node dense connectivity
graphs at L = 5, m = 2, H = 64, for F0 = 7 and one-hot F0 = 400; 8 subjects x the 20 sets of a deletion curve (fractions
0, 0.05, ..., 0.95 of a random ranking).  One JSON line per (F0, route); times are medians after a warm-up, per
VIRTUAL graph (one lesioned copy, both classes).  `lesion` is the whole method call (the base forward, the host mask
arrays, the uploads, the one read-back of the kept counts); `lesion_hip` is gnm/attribution.py lesion_hip alone on the
registered batch (XW, the mask packing, the read-back, L + 1 launches).
    python tools/bench_lesion.py [--subjects 8] [--sets 20] [--reps 5] [--f0 7,400] [--no-parent] [--out FILE]"""
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
ap.add_argument("--sets", type=int, default=20)
ap.add_argument("--n", type=int, default=400)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--f0", default="7,400")
ap.add_argument("--no-parent", action="store_true", help="time the device route only")
ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
args = ap.parse_args()
H, L, M = 64, 5, 2
lines = []


def emit(rec):
    lines.append(rec)
    print(json.dumps(rec), flush=True)


import torch
from gnm import attribution, synth
from gnm.lesion import masks_from_ranking
from models.graphcnn import GIN_InfoMaxReg

dev = torch.device("cuda:0")


class Copy:
    pass


def deleted_copy(g, rm):
    """g without the nodes of the bool mask rm: their edges dropped, the survivors renumbered, the other rows kept"""
    em = g.edge_mat.numpy()
    em = em[:, ~rm[em].any(0)]
    new = np.cumsum(~rm) - 1
    c = Copy()
    c.g = list(range(int((~rm).sum())))
    c.label = g.label
    c.edge_mat = torch.from_numpy(np.ascontiguousarray(new[em]))
    c.node_features = g.node_features[torch.from_numpy(~rm)]
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
    ranking = np.random.default_rng(0).random((args.subjects, args.n))
    masks, counts = masks_from_ranking(ranking, np.arange(args.sets) / float(args.sets))
    V = args.subjects * args.sets
    common = dict(f0=f0, n=args.n, subjects=args.subjects, sets=args.sets, H=H, L=L)
    model.lesion(graphs, (0, 1), masks)                                  # warm-up (registers the graphs, loads the code)
    t = timed(lambda: model.lesion(graphs, (0, 1), masks), args.reps)
    # lesion_hip alone, on the registered batch
    model.eval()
    names, tensors, buffers = model._param_lists()
    P = dict(zip(names, tensors))
    P.update(buffers)
    batch = model._batch_of(graphs)
    X = batch.arena.features(batch).detach()
    removed = np.concatenate(masks).astype(np.uint8)
    vgraph = np.repeat(np.arange(args.subjects, dtype=np.int32), args.sets)
    th = timed(lambda: attribution.lesion_hip(model._spec, batch, X, P, [0, 1], removed, vgraph), args.reps)
    emit(dict(route="lesion", ms=round(t * 1e3, 3), us_per_virtual_graph=round(t / V * 1e6, 3),
              lesion_hip_ms=round(th * 1e3, 3), lesion_hip_us_per_virtual_graph=round(th / V * 1e6, 3), **common))
    if args.no_parent:
        continue
    # the route without the method: (a) host copies, (b) arena registration, (c) predict per set size
    t0 = time.perf_counter()
    copies = [[deleted_copy(g, masks[j][k]) for j, g in enumerate(graphs)] for k in range(args.sets)]
    t1 = time.perf_counter()
    for grp in copies:
        model.arena().add_many(grp)
    torch.cuda.synchronize()
    t2 = time.perf_counter()

    def predict_all():
        for grp in copies:
            model.predict(grp)
    predict_all()                                                        # warm-up
    tp = timed(predict_all, args.reps)
    emit(dict(route="copies", host_copy_us_per_virtual_graph=round((t1 - t0) / V * 1e6, 1),
              register_us_per_virtual_graph=round((t2 - t1) / V * 1e6, 1),
              predict_us_per_virtual_graph=round(tp / V * 1e6, 3), predict_ms=round(tp * 1e3, 3),
              lesion_speedup_over_predict=round(tp / t, 2), lesion_hip_speedup_over_predict=round(tp / th, 2),
              lesion_speedup_over_copies_with_host=round((tp + t2 - t0) / t, 2), **common))
if args.out:
    with open(args.out, "a") as f:
        for rec in lines:
            f.write(json.dumps(rec) + "\n")
