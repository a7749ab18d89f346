#!/usr/bin/env python3
"""Hub measures on the device (gnm.hubs.hub_measures, csrc/hubs.hip): the two launches timed by device events after a
warm-up, next to the numpy oracle and, where it imports, networkx's betweenness_centrality on ONE graph of each case in
the same run.  One JSON line per case.
    python tools/bench_hubs.py [--cases 1024x400,64x1000k] [--windows 64] [--reps 7] [--modules 7] [--no-networkx]
                               [--out FILE]
Cases SxN: S graphs of N nodes from correlations of random series, the percentile rule at sparsity 30; a trailing k
(64x1000k): the kNN rule at knn=20.  --windows S: the graphs of one sliding-window study (S subjects, T = 1200, window 50,
stride 10, n = 400, sparsity 30: 116 windows each; 0 skips it).  Labels: arange(n) % --modules.
Reported per case: betweenness_ms (gnm_topology_betweenness), modules_ms (gnm_topology_modules), call_ms (wall clock of
hub_measures around a device synchronise, batch assembly, label upload and allocations included), all medians over
--reps; the LDS words the betweenness searches read per second -- a node not yet reached reads its W row words and the W
mask words once a forward level, a node at levels 1 .. deepest - 1 once more on the way back, counted exactly on the first
graph from the oracle's distances and scaled by S -- against the ds_read_b32 rate of the chip (128 B/clk/CU: about
75 TB/s with every CU streaming); host_s and networkx_s for one graph."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "graph-neural-mapping_amd"))
import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--cases", default="1024x400,64x1000k")
ap.add_argument("--windows", type=int, default=64, help="subjects of the sliding-window study (0: skip)")
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--modules", type=int, default=7)
ap.add_argument("--no-networkx", action="store_true")
ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
args = ap.parse_args()
lines = []
LDS_READ_B32_TB_S = 75.0            # ds_read_b32, every CU streaming


def emit(rec):
    lines.append(rec)
    print(json.dumps(rec), flush=True)


import torch
from gnm import connectome as C
from gnm import hubs as H
from gnm import topology as T
from gnm._cabi import check, lib
from gnm.arena import GraphArena

dev = torch.device("cuda:0")


def sync():
    torch.cuda.synchronize()
    return time.perf_counter()


def med(ts):
    return float(np.median(ts))


def edges_of(g):
    em = g.edge_mat.numpy()
    return np.ascontiguousarray(em[:, :em.shape[1] // 2].T)


def words_read_betweenness(edges, n):
    """row and mask words the betweenness kernel reads for one graph (see the module docstring)"""
    D = T._distances(T._adjacency(edges, n)).astype(np.int64)
    depth = D.max(1)                                            # per source
    fwd = np.where(D > 0, D, 0).sum() + ((D < 0) * (depth[:, None] + 1)).sum()
    back = ((D >= 1) & (D <= depth[:, None] - 1)).sum()
    return int(fwd + back) * 2 * ((n + 31) // 32)


def one_graph_references(edges, n, lab):
    rec = {}
    t0 = time.perf_counter()
    h = H.hub_measures_host(edges, n, labels=lab)
    rec["host_s"] = time.perf_counter() - t0
    if not args.no_networkx:
        try:
            import networkx as nx
        except ImportError:
            return rec, h
        G = nx.Graph()
        G.add_nodes_from(range(n))
        G.add_edges_from(edges.tolist())
        t0 = time.perf_counter()
        bc = nx.betweenness_centrality(G, normalized=False)
        rec["networkx_betweenness_s"] = time.perf_counter() - t0
        bc = np.array([bc[v] for v in range(n)])
        rec["networkx_betweenness_rel_diff"] = float(np.abs(bc - h.betweenness).max() / max(bc.max(), 1e-300))
    return rec, h


def run(name, arena, graphs, extra):
    n = len(graphs[0].g)
    lab = np.arange(n, dtype=np.int64) % args.modules
    batch = arena.batch(graphs)
    B, N, n_max = batch.B, batch.N, batch.n_max
    m = H.hub_measures(arena, graphs, labels=lab)               # warm-up of both launches
    K = int(m.module_degree.shape[1])
    st = torch.cuda.current_stream(dev).cuda_stream
    csr = batch.csr_ptrs()
    lab_dev = torch.from_numpy(np.tile(lab, B).astype(np.int32)).to(dev)

    def betweenness():
        check(lib.gnm_topology_betweenness(*csr, batch.node_off.data_ptr(), B, n_max, None, m.betweenness.data_ptr(),
                                           m.betweenness_normalized.data_ptr(), st), "gnm_topology_betweenness")

    def modules():
        check(lib.gnm_topology_modules(*csr, batch.node_off.data_ptr(), lab_dev.data_ptr(), B, n_max, K,
                                       m.module_degree.data_ptr(), m.participation.data_ptr(),
                                       m.within_module_z.data_ptr(), m.module_edges.data_ptr(),
                                       m.modularity.data_ptr(), st), "gnm_topology_modules")

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    bet_t, mod_t, call_t = [], [], []
    for _ in range(args.reps):
        bet_t.append(timed(betweenness))
        mod_t.append(timed(modules))
        t0 = sync()
        H.hub_measures(arena, graphs, labels=lab)
        call_t.append(1e3 * (sync() - t0))
    e0 = edges_of(graphs[0])
    refs, h = one_graph_references(e0, n, lab)
    g0 = m.graph(0).numpy()
    same = all(np.asarray(getattr(g0, k)).tobytes() == np.asarray(getattr(h, k)).tobytes()
               for k in H.NODE_FIELDS + H.GRAPH_FIELDS)
    words = words_read_betweenness(e0, n)
    rec = {"bench": "hubs", "case": name, "graphs": B, "n": n, "nodes_total": N, "modules": K, "reps": args.reps,
           "edges_graph0": int(e0.shape[0]), "graph0_bitwise_oracle": bool(same),
           "workgroup_threads": 512 if n_max <= 512 else 1024,
           "betweenness_ms": med(bet_t), "modules_ms": med(mod_t), "betweenness_ms_all": [round(t, 3) for t in bet_t],
           "modules_ms_all": [round(t, 3) for t in mod_t], "call_ms": med(call_t),
           "betweenness_us_per_graph": 1e3 * med(bet_t) / B, "modules_us_per_graph": 1e3 * med(mod_t) / B,
           "betweenness_lds_words_graph0": words,
           "betweenness_lds_tb_per_s": words * B * 4 / (med(bet_t) * 1e-3) / 1e12,
           "lds_read_b32_peak_tb_per_s": LDS_READ_B32_TB_S}
    rec["betweenness_lds_share_of_peak"] = rec["betweenness_lds_tb_per_s"] / LDS_READ_B32_TB_S
    rec.update(refs)
    rec.update(extra)
    emit(rec)


for case in args.cases.split(","):
    knn = case.endswith("k")
    S, n = (int(v) for v in case.rstrip("k").split("x"))
    g = torch.Generator(device=dev).manual_seed(S + n)
    fc = torch.empty((S, n, n), dtype=torch.float64, device=dev)
    for lo in range(0, S, 64):                                  # correlations of n + 100 rows, 64 subjects at a time
        k = min(S, lo + 64) - lo
        fc[lo:lo + k] = C.connectivity_from_timeseries(torch.randn((k, n + 100, n), generator=g, device=dev,
                                                                   dtype=torch.float64))
    ar = GraphArena(dev)
    feats = torch.ones((n, 1), dtype=torch.float32, device=dev)
    if knn:
        graphs = C.graphs_from_connectivity(ar, fc, None, feats, [0] * S, knn=20)
    else:
        graphs = C.graphs_from_connectivity(ar, fc, 30, feats, [0] * S)
    del fc
    run(case, ar, graphs, {"rule": "knn=20" if knn else "sparsity=30"})
    del ar, graphs
    torch.cuda.empty_cache()

if args.windows > 0:
    S, Tn, n, window, stride = args.windows, 1200, 400, 50, 10
    g = torch.Generator(device=dev).manual_seed(S + Tn)
    ts = torch.randn((S, Tn, n), generator=g, device=dev, dtype=torch.float64) * 50 + 1e4
    ar = GraphArena(dev)
    graphs, _ = C.dynamic_graphs_from_timeseries(ar, ts, 30, [s % 2 for s in range(S)], window, stride)
    del ts
    run("windows", ar, graphs, {"rule": "sparsity=30", "subjects": S, "T": Tn, "window": window, "stride": stride})

if args.out:
    with open(args.out, "a") as fh:
        for rec in lines:
            fh.write(json.dumps(rec) + "\n")
