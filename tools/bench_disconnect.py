#!/usr/bin/env python3
"""Disconnection throughput: GIN_InfoMaxReg.disconnect(graphs, (0, 1), a, b) -- every (graph, set pair) as a virtual
graph over the source graph's bit adjacency under a keep mask chosen per row (csrc/disconnect.hip) -- next to lesion() on
the same number of sets in the same run (the same kernel less one select per staged word: the figure to read it against)
and to the route without the method, timed in its parts: (a) building the edge-cut copies on the host, (b) registering
them in the arena, (c) model.predict() on the registered copies.  400-node dense connectivity graphs at L = 5, m = 2,
H = 64, for F0 = 7 and one-hot F0 = 400; 8 subjects x the 105 pairs of a 14-group labelling (7 networks x 2
hemispheres).  One JSON line per (F0, route); times are medians after a warm-up, per VIRTUAL graph (one cut copy, both
classes).  `disconnect` is the whole method call (the base forward, the host mask arrays, the uploads); `disconnect_hip`
is gnm/attribution.py disconnect_hip alone on the registered batch (XW, the mask packing, L + 1 launches); `lesion` /
`lesion_hip` are the same two figures of lesion() with each pair's set A as the removed set.
    python tools/bench_disconnect.py [--subjects 8] [--groups 14] [--reps 5] [--f0 7,400] [--no-parent] [--out FILE]"""
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
ap.add_argument("--groups", type=int, default=14, help="parcel groups K: K (K + 1) / 2 pairs per subject")
ap.add_argument("--n", type=int, default=400)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--f0", default="7,400")
ap.add_argument("--no-parent", action="store_true", help="time the device routes only")
ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
args = ap.parse_args()
H, L, M = 64, 5, 2
lines = []


def emit(rec):
    lines.append(rec)
    print(json.dumps(rec), flush=True)


import torch
from gnm import attribution, synth
from gnm.lesion import cut_edge_counts, pair_sets
from models.graphcnn import GIN_InfoMaxReg

dev = torch.device("cuda:0")


class Copy:
    pass


def cut_copy(g, a, b):
    """g without the edges between the bool masks a and b: the same nodes and rows, the edge_mat columns filtered"""
    em = g.edge_mat.numpy()
    c = Copy()
    c.g = g.g
    c.label = g.label
    c.edge_mat = torch.from_numpy(np.ascontiguousarray(em[:, ~((a[em[0]] & b[em[1]]) | (b[em[0]] & a[em[1]]))]))
    c.node_features = g.node_features
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
    labels = np.random.default_rng(0).integers(0, args.groups, args.n)
    a, b, pairs = pair_sets(labels, args.groups)
    S = len(pairs)
    V = args.subjects * S
    common = dict(f0=f0, n=args.n, subjects=args.subjects, pairs=S, H=H, L=L,
                  mean_cut_edges=round(float(np.mean([cut_edge_counts(g.edge_mat, a, b).mean() for g in graphs])), 1))
    model.disconnect(graphs, (0, 1), a, b)                               # warm-up (registers the graphs, loads the code)
    t = timed(lambda: model.disconnect(graphs, (0, 1), a, b), args.reps)
    # disconnect_hip alone, on the registered batch
    model.eval()
    names, tensors, buffers = model._param_lists()
    P = dict(zip(names, tensors))
    P.update(buffers)
    batch = model._batch_of(graphs)
    X = batch.arena.features(batch).detach()
    in_a = np.tile(a, (args.subjects, 1)).astype(np.uint8)
    in_b = np.tile(b, (args.subjects, 1)).astype(np.uint8)
    vgraph = np.repeat(np.arange(args.subjects, dtype=np.int32), S)
    th = timed(lambda: attribution.disconnect_hip(model._spec, batch, X, P, [0, 1], in_a, in_b, vgraph), args.reps)
    emit(dict(route="disconnect", ms=round(t * 1e3, 3), us_per_virtual_graph=round(t / V * 1e6, 3),
              disconnect_hip_ms=round(th * 1e3, 3), disconnect_hip_us_per_virtual_graph=round(th / V * 1e6, 3), **common))
    # lesion() on the same number of sets, in the same run
    model.lesion(graphs, (0, 1), a)
    tl = timed(lambda: model.lesion(graphs, (0, 1), a), args.reps)
    model.eval()
    tlh = timed(lambda: attribution.lesion_hip(model._spec, batch, X, P, [0, 1], in_a, vgraph), args.reps)
    emit(dict(route="lesion", ms=round(tl * 1e3, 3), us_per_virtual_graph=round(tl / V * 1e6, 3),
              lesion_hip_ms=round(tlh * 1e3, 3), lesion_hip_us_per_virtual_graph=round(tlh / V * 1e6, 3),
              disconnect_over_lesion=round(t / tl, 3), disconnect_hip_over_lesion_hip=round(th / tlh, 3), **common))
    if args.no_parent:
        continue
    # the route without the method: (a) host copies, (b) arena registration, (c) predict on the copies
    t0 = time.perf_counter()
    copies = [[cut_copy(g, a[s], b[s]) for g in graphs] for s in range(S)]
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
              disconnect_speedup_over_predict=round(tp / t, 2), disconnect_hip_speedup_over_predict=round(tp / th, 2),
              disconnect_speedup_over_copies_with_host=round((tp + t2 - t0) / t, 2), **common))
if args.out:
    with open(args.out, "a") as f:
        for rec in lines:
            f.write(json.dumps(rec) + "\n")
