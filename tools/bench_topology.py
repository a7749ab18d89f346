#!/usr/bin/env python3
"""Graph measures on the device (gnm.topology.graph_measures, csrc/topology.hip): the two launches timed by device
events after a warm-up, with and without local efficiency, next to the numpy oracle and, where it imports, networkx on
ONE graph of each kind in the same run.  One JSON line per case.
    python tools/bench_topology.py [--cases 1024x400,64x1000k] [--windows 64] [--reps 7] [--no-networkx] [--out FILE]
Cases SxN: S graphs of N nodes from correlations of random series, the percentile rule at sparsity 30; a trailing k
(64x1000k): the kNN rule at knn=20.  --windows S: the graphs of one sliding-window study (S subjects, T = 1200, window 50,
stride 10, n = 400, sparsity 30: 116 windows each; 0 skips it).
Reported per case: nodes_ms (gnm_topology_nodes), local_ms (gnm_topology_local), call_ms / call_nolocal_ms (wall clock of
graph_measures around a device synchronise, batch assembly and allocations included), all medians over --reps; the LDS
bytes the local-efficiency searches read per second -- rows read, counted exactly on the first graph with the oracle's
search and scaled by S, times the words a lane group fetches per row -- against the ds_read_b32 rate of the chip
(128 B/clk/CU: about 75 TB/s with every CU streaming); host_s and networkx_s for one graph."""
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


def rows_read_local(edges, n):
    """rows the local-efficiency searches of one graph read: a search expands every node it reaches, itself included"""
    A = T._adjacency(edges, n)
    total = 0
    for v in range(n):
        S = np.flatnonzero(A[v])
        if S.shape[0] >= 2:
            total += int((T._distances(A[np.ix_(S, S)]) >= 0).sum())
    return total


def one_graph_references(edges, n):
    rec = {}
    t0 = time.perf_counter()
    T.graph_measures_host(edges, n, local_efficiency=False)
    t1 = time.perf_counter()
    h = T.graph_measures_host(edges, n)
    t2 = time.perf_counter()
    rec.update(host_nolocal_s=t1 - t0, host_s=t2 - t1)
    if not args.no_networkx:
        try:
            import networkx as nx
        except ImportError:
            return rec, h
        G = nx.Graph()
        G.add_nodes_from(range(n))
        G.add_edges_from(edges.tolist())
        t0 = time.perf_counter()
        ge = nx.global_efficiency(G)
        t1 = time.perf_counter()
        le = nx.local_efficiency(G)
        t2 = time.perf_counter()
        rec.update(networkx_global_efficiency_s=t1 - t0, networkx_local_efficiency_s=t2 - t1,
                   networkx_global_efficiency_diff=abs(ge - float(h.global_efficiency[0])),
                   networkx_local_efficiency_diff=abs(le - float(h.mean_local_efficiency[0])))
    return rec, h


def run(name, arena, graphs, extra):
    n = len(graphs[0].g)
    batch = arena.batch(graphs)
    B, N, n_max = batch.B, batch.N, batch.n_max
    m = T.graph_measures(arena, graphs)                                     # warm-up of both launches
    T.graph_measures(arena, graphs, local_efficiency=False)
    f = {k: getattr(m, k) for k in T.NODE_FIELDS + T.GRAPH_FIELDS}
    st = torch.cuda.current_stream(dev).cuda_stream
    csr = batch.csr_ptrs()

    def nodes():
        check(lib.gnm_topology_nodes(*csr, batch.node_off.data_ptr(), B, n_max,
                                     *[f[k].data_ptr() for k in ("degree", "triangles", "clustering", "eccentricity",
                                                                 "reachable", "distance_sum", "component",
                                                                 "nodal_efficiency", "edges", "components",
                                                                 "distance_histogram", "diameter", "global_efficiency",
                                                                 "characteristic_path_length", "transitivity",
                                                                 "mean_clustering")], st), "gnm_topology_nodes")

    def local():
        check(lib.gnm_topology_local(*csr, batch.node_off.data_ptr(), B, n_max, None, f["local_efficiency"].data_ptr(),
                                     f["mean_local_efficiency"].data_ptr(), st), "gnm_topology_local")

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    nodes_t, local_t, call_t, bare_t = [], [], [], []
    for _ in range(args.reps):
        nodes_t.append(timed(nodes))
        local_t.append(timed(local))
        t0 = sync()
        T.graph_measures(arena, graphs)
        t1 = sync()
        T.graph_measures(arena, graphs, local_efficiency=False)
        t2 = sync()
        call_t.append(1e3 * (t1 - t0)); bare_t.append(1e3 * (t2 - t1))
    e0 = edges_of(graphs[0])
    refs, h = one_graph_references(e0, n)
    g0 = m.graph(0).numpy()
    same = all(np.array_equal(getattr(g0, k), getattr(h, k), equal_nan=True) for k in T.NODE_FIELDS + T.GRAPH_FIELDS)
    rows = rows_read_local(e0, n)
    words, group = (n_max + 31) // 32, (16 if n_max <= 512 else 32)
    rec = {"bench": "topology", "case": name, "graphs": B, "n": n, "nodes_total": N, "reps": args.reps,
           "edges_graph0": int(e0.shape[0]), "graph0_bitwise_oracle": bool(same),
           "nodes_ms": med(nodes_t), "local_ms": med(local_t), "nodes_ms_all": [round(t, 3) for t in nodes_t],
           "local_ms_all": [round(t, 3) for t in local_t], "call_ms": med(call_t), "call_nolocal_ms": med(bare_t),
           "us_per_graph": 1e3 * med(call_t) / B, "us_per_graph_nolocal": 1e3 * med(bare_t) / B,
           "local_rows_read_graph0": rows, "row_words": words, "group_lanes": group,
           "local_lds_row_tb_per_s": rows * B * words * 4 / (med(local_t) * 1e-3) / 1e12,
           "local_lds_fetched_tb_per_s": rows * B * group * 4 / (med(local_t) * 1e-3) / 1e12,
           "lds_read_b32_peak_tb_per_s": LDS_READ_B32_TB_S}
    rec["local_lds_fetched_share_of_peak"] = rec["local_lds_fetched_tb_per_s"] / LDS_READ_B32_TB_S
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
