#!/usr/bin/env python3
"""k-nearest-neighbour connectome graphs on the device (gnm.connectome.graphs_from_connectivity(..., knn=k), csrc/
connectome.hip gnm_connectome_knn_structure) next to the percentile route at the sparsity that gives the same edge
count, in one process.  One JSON line per case; times are wall-clock medians around a device synchronise, the two routes
alternating.
    python tools/bench_knn.py [--cases 1024x400,64x1000] [--k 20] [--reps 7] [--dynamic 64] [--host 64] [--out FILE]
Per case SxN (FC resident on the device, fp64, correlations of random series): FC to registered graphs through either
route (fresh arena each run), and the structure stage alone (gnm_connectome_knn_structure against
gnm_connectome_thresholds + gnm_connectome_structure) with the bytes of FC it has to read per second.  --dynamic S:
dynamic_graphs_from_timeseries at T = 1200, window 50, stride 10, n = 400 through either rule.  --host H: the host route
once on the first H matrices of the first case: numpy knn_edges + SynthGraph + GraphArena.add_many."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "graph-neural-mapping_amd"))
import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--cases", default="1024x400,64x1000")
ap.add_argument("--k", type=int, default=20)
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--dynamic", type=int, default=64, help="S of the sliding-window run (0: skip)")
ap.add_argument("--host", type=int, default=64, help="matrices of the host route (0: skip)")
ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
args = ap.parse_args()
lines = []


def emit(rec):
    lines.append(rec)
    print(json.dumps(rec), flush=True)


def med(ts):
    return 1e3 * float(np.median(ts))


import torch
from gnm import connectome as C
from gnm._cabi import check, lib
from gnm.arena import GraphArena
from gnm.synth import SynthGraph

dev = torch.device("cuda:0")
k = args.k


def sync():
    torch.cuda.synchronize()
    return time.perf_counter()


def edges_of(arena, gids):
    return sum(arena.nnz[g] for g in gids) // 2


first_fc = None
for case in args.cases.split(","):
    S, n = (int(v) for v in case.split("x"))
    g = torch.Generator(device=dev).manual_seed(S + n)
    fc = torch.empty((S, n, n), dtype=torch.float64, device=dev)
    for lo in range(0, S, 64):                                  # correlations of n + 100 rows, 64 subjects at a time
        m = min(S, lo + 64) - lo
        fc[lo:lo + m] = C.connectivity_from_timeseries(torch.randn((m, n + 100, n), generator=g, device=dev,
                                                                   dtype=torch.float64))
    if first_fc is None:
        first_fc = fc
    feats = torch.ones((n, 1), dtype=torch.float32, device=dev)
    labels = [0] * S
    ar = GraphArena(dev)
    E = edges_of(ar, ar.add_connectivity(fc, None, feats, knn=k))
    sparsity = 100.0 * (2 * E / S + n) / (n * n)                # entries above the threshold: both triangles, diagonal
    Ep = edges_of(ar, ar.add_connectivity(fc, sparsity, feats))
    del ar
    # the structure stage alone
    per = int(lib.gnm_connectome_workspace_words(1, n))
    work = torch.empty(S * per, dtype=torch.int32, device=dev)
    sel = torch.empty(int(lib.gnm_connectome_knn_scratch_words(S, n)), dtype=torch.int32, device=dev)
    nnz = torch.empty(S, dtype=torch.int32, device=dev)
    iso = torch.empty(S, dtype=torch.int32, device=dev)
    thr = torch.empty(S, dtype=torch.float64, device=dev)
    k_lo, k_hi, gamma = C.percentile_indexes(n * n, sparsity)
    st = torch.cuda.current_stream(dev).cuda_stream

    def knn_stage():
        check(lib.gnm_connectome_knn_structure(fc.data_ptr(), S, n, k, 0, sel.data_ptr(), work.data_ptr(),
                                               nnz.data_ptr(), iso.data_ptr(), st), "gnm_connectome_knn_structure")

    def thr_stage():
        check(lib.gnm_connectome_thresholds(fc.data_ptr(), S, n, k_lo, k_hi, gamma, thr.data_ptr(), st),
              "gnm_connectome_thresholds")

    def pct_stage():
        check(lib.gnm_connectome_structure(fc.data_ptr(), S, n, thr.data_ptr(), work.data_ptr(), nnz.data_ptr(),
                                           iso.data_ptr(), st), "gnm_connectome_structure")

    knn_t, pct_t, ks_t, ts_t, ps_t = [], [], [], [], []
    for _ in range(args.reps):
        t0 = sync()
        GraphArena(dev).add_connectivity(fc, None, feats, knn=k)
        t1 = sync()
        GraphArena(dev).add_connectivity(fc, sparsity, feats)
        t2 = sync()
        knn_stage()
        t3 = sync()
        thr_stage()
        t4 = sync()
        pct_stage()
        t5 = sync()
        knn_t.append(t1 - t0); pct_t.append(t2 - t1); ks_t.append(t3 - t2); ts_t.append(t4 - t3); ps_t.append(t5 - t4)
    fc_bytes = S * n * n * 8.0
    emit({"bench": "knn", "S": S, "n": n, "k": k, "reps": args.reps, "fc_gb": fc_bytes / 1e9,
          "knn_edges_per_graph": E / S, "percentile_sparsity": sparsity, "percentile_edges_per_graph": Ep / S,
          "knn_graphs_ms": med(knn_t), "percentile_graphs_ms": med(pct_t),
          "knn_graphs_ms_all": [round(1e3 * t, 3) for t in knn_t],
          "percentile_graphs_ms_all": [round(1e3 * t, 3) for t in pct_t],
          "knn_us_per_graph": 1e3 * med(knn_t) / S, "percentile_us_per_graph": 1e3 * med(pct_t) / S,
          "knn_structure_ms": med(ks_t), "thresholds_ms": med(ts_t), "percentile_structure_ms": med(ps_t),
          "knn_structure_fc_tb_per_s": fc_bytes / float(np.median(ks_t)) / 1e12,
          "percentile_structure_fc_tb_per_s": fc_bytes / float(np.median(ps_t)) / 1e12})
    del work, sel, nnz, iso, thr
    if fc is not first_fc:
        del fc
    torch.cuda.empty_cache()

if args.host > 0 and first_fc is not None:
    H = min(args.host, int(first_fc.shape[0]))
    n = int(first_fc.shape[1])
    t0 = sync()
    host = first_fc[:H].cpu().numpy()
    t1 = time.perf_counter()
    feat = np.ones((n, 1), np.float32)
    graphs = [SynthGraph(n, np.stack(C.knn_edges(m, k), 1), feat, 0) for m in host]
    t2 = time.perf_counter()
    GraphArena(dev).add_many(graphs)
    t3 = sync()
    emit({"bench": "knn_host", "graphs": H, "n": n, "k": k, "download_ms": 1e3 * (t1 - t0),
          "knn_edges_and_graph_ms": 1e3 * (t2 - t1), "add_many_ms": 1e3 * (t3 - t2),
          "host_ms_per_graph": 1e3 * (t3 - t1) / H})
    del graphs, host
del first_fc
torch.cuda.empty_cache()

if args.dynamic > 0:
    S, T, n, window, stride = args.dynamic, 1200, 400, 50, 10
    g = torch.Generator(device=dev).manual_seed(S + T)
    ts = torch.randn((S, T, n), generator=g, device=dev, dtype=torch.float64) * 50 + 1e4
    labels = [s % 2 for s in range(S)]
    ar = GraphArena(dev)
    gs, _ = C.dynamic_graphs_from_timeseries(ar, ts[:1], None, labels[:1], window, stride, knn=k)          # warm-up
    E = edges_of(ar, [x._gnm_cache[1] for x in gs]) / len(gs)
    sparsity = 100.0 * (2 * E + n) / (n * n)
    C.dynamic_graphs_from_timeseries(ar, ts[:1], sparsity, labels[:1], window, stride)
    del ar, gs
    torch.cuda.empty_cache()
    knn_t, pct_t, iso_k, iso_p = [], [], 0, 0
    for _ in range(args.reps):
        a = GraphArena(dev)
        t0 = sync()
        gs, _ = C.dynamic_graphs_from_timeseries(a, ts, None, labels, window, stride, knn=k)
        t1 = sync()
        ng, iso_k = len(gs), sum(a.iso)
        del gs, a
        b = GraphArena(dev)
        t2 = sync()
        gp, _ = C.dynamic_graphs_from_timeseries(b, ts, sparsity, labels, window, stride)
        t3 = sync()
        iso_p = sum(b.iso)
        del gp, b
        torch.cuda.empty_cache()
        knn_t.append(t1 - t0); pct_t.append(t3 - t2)
    emit({"bench": "knn_dynamic", "S": S, "T": T, "n": n, "window": window, "stride": stride, "k": k, "graphs": ng,
          "reps": args.reps, "percentile_sparsity": sparsity, "knn_series_to_graphs_ms": med(knn_t),
          "percentile_series_to_graphs_ms": med(pct_t), "knn_us_per_graph": 1e3 * med(knn_t) / ng,
          "percentile_us_per_graph": 1e3 * med(pct_t) / ng, "knn_graphs_with_isolated_node": int(iso_k),
          "percentile_graphs_with_isolated_node": int(iso_p)})
if args.out:
    with open(args.out, "a") as f:
        for rec in lines:
            f.write(json.dumps(rec) + "\n")
