#!/usr/bin/env python3
"""Connectivity-saliency throughput: GIN_InfoMaxReg.edge_saliency(graphs, (0, 1)) -- the batched d score / d A of
csrc/edgesal.hip over gnm_saliency's layer launches -- next to a per-graph torch autograd loop with a dense adjacency
leaf (what a user has to write today: the eval forward restated in torch, one backward per graph and class), on
400-node dense connectivity graphs at L = 5, m = 2, H = 64, for F0 = 7 and one-hot F0 = 400.  One JSON line per
(B, F0, route); a "graph" is both classes of one graph.
    python tools/bench_edge_saliency.py [--B 64,256] [--reps 5] [--loop-graphs 16] [--f0 7,400] [--out FILE]
    python tools/bench_edge_saliency.py --stats KERNEL_STATS.csv [--B 256] [--out FILE]
The second form reads a `rocprofv3 --kernel-trace --stats` table of a run of the first at ONE B and prints, for
gnm_edge_saliency_kernel, calls and mean time against its two floors per launch (one class of B graphs): HBM bytes
(S_l and h_{l-1} of every layer, Y, the [n, n] output: 4 (2 L n H + n^2) per graph) at 8 TB/s, and the six-term
split-bf16 products (6 x 2 x (32 W)^2 x L H per graph, W = ceil(n / 32)) at 2.5 PFLOP/s."""
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
ap.add_argument("--B", default="64,256")
ap.add_argument("--n", type=int, default=400)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--loop-graphs", type=int, default=16)
ap.add_argument("--f0", default="7,400")
ap.add_argument("--stats", default=None, help="summarise this rocprofv3 kernel-stats CSV instead of timing")
ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
args = ap.parse_args()
H, L, M = 64, 5, 2
HBM, BF16 = 8e12, 2.5e15
lines = []


def emit(rec):
    lines.append(rec)
    print(json.dumps(rec), flush=True)


def restated_edge_grad(model, g, cls, dev):
    """d logit[cls] / d A for one graph: the eval forward restated in torch with a dense leaf adjacency"""
    import torch
    n = len(g.g)
    A = torch.zeros((n, n), device=dev)
    em = g.edge_mat.to(dev)
    A[em[0], em[1]] = 1.0
    if not model.learn_eps:
        A = A + torch.eye(n, device=dev)
    A.requires_grad_()
    h = g.node_features.to(dev)
    logit = 0
    for l in range(model.num_layers):
        pooled = A @ h
        if model.neighbor_pooling_type == "average":
            pooled = pooled / A.sum(1, keepdim=True)
        if model.learn_eps:
            pooled = pooled + (1 + model.eps[l]) * h
        mlp = model.mlps[l]
        if model.num_mlp_layers == 1:
            x = mlp.linear(pooled)
        else:
            x = pooled
            for k in range(model.num_mlp_layers - 1):
                x = torch.relu(mlp.batch_norms[k](mlp.linears[k](x)))
            x = mlp.linears[-1](x)
        h = torch.relu(model.batch_norms[l](x))
        pg = h.mean(0) if model.graph_pooling_type == "average" else h.sum(0)
        logit = logit + model.linears_prediction[l](pg)
    (ga,) = torch.autograd.grad(logit[cls], A)
    return ga


if args.stats:
    B = int(args.B.split(",")[0])
    W = (args.n + 31) // 32
    nbytes = 4.0 * B * (2 * L * args.n * H + args.n * args.n)
    flops = 6 * 2.0 * B * (32 * W) ** 2 * L * H
    with open(args.stats) as f:
        for row in csv.DictReader(f):
            name = row["Name"]
            if "gnm_edge_saliency_kernel" in name or "gnm_saliency_layer_kernel<false>" in name:
                avg = float(row["AverageNs"]) * 1e-9
                rec = {"bench": "edge_saliency_kernel", "kernel": name, "calls": int(row["Calls"]),
                       "avg_us": avg * 1e6, "min_us": float(row["MinNs"]) / 1e3, "max_us": float(row["MaxNs"]) / 1e3}
                if "gnm_edge_saliency_kernel" in name:
                    rec.update(B=B, n=args.n, H=H, L=L, algorithmic_bytes=nbytes, hbm_floor_us=1e6 * nbytes / HBM,
                               frac_of_8TBps=nbytes / avg / HBM, mfma_flops=flops,
                               mfma_floor_us=1e6 * flops / BF16, frac_of_bf16_peak=flops / avg / BF16)
                emit(rec)
else:
    import torch
    from gnm import synth
    from models.graphcnn import GIN_InfoMaxReg

    dev = torch.device("cuda:0")
    Bs = [int(x) for x in args.B.split(",")]
    base = synth.make_pool("dense_fc", max(Bs), n=args.n, f0=7)
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
        for B in Bs:
            gs = graphs[:B]
            model.edge_saliency(gs, (0, 1), batch_size=B)           # warm-up: arena, allocator, code objects
            torch.cuda.synchronize()
            ts = []
            for _ in range(args.reps):
                t0 = time.perf_counter()
                model.edge_saliency(gs, (0, 1), batch_size=B)
                torch.cuda.synchronize()
                ts.append(time.perf_counter() - t0)
            t = float(np.median(ts))
            emit({"bench": "edge_saliency", "route": "batched", "B": B, "n": args.n, "F0": f0, "H": H, "L": L, "m": M,
                  "classes": 2, "median_s": t, "graphs_per_s": B / t, "us_per_graph": 1e6 * t / B, "reps": args.reps})
            model.class_activation(gs, (0, 1), kind="gradient")
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            model.class_activation(gs, (0, 1), kind="gradient")
            torch.cuda.synchronize()
            t = time.perf_counter() - t0
            emit({"bench": "edge_saliency", "route": "gradient_cam_batched_reference_point", "B": B, "n": args.n,
                  "F0": f0, "classes": 2, "us_per_graph": 1e6 * t / B})
        G = min(args.loop_graphs, len(graphs))
        for g in graphs[:2]:
            restated_edge_grad(model, g, 0, dev)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for g in graphs[:G]:
            for c in (0, 1):
                restated_edge_grad(model, g, c, dev)
        torch.cuda.synchronize()
        t = time.perf_counter() - t0
        emit({"bench": "edge_saliency", "route": "per_graph_torch_dense_leaf", "B": G, "n": args.n, "F0": f0, "H": H,
              "L": L, "m": M, "classes": 2, "total_s": t, "us_per_graph": 1e6 * t / G})
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        for r in lines:
            f.write(json.dumps(r) + "\n")
