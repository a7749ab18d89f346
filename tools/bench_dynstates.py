#!/usr/bin/env python3
"""Connectivity-state clustering throughput: one Lloyd iteration of gnm.connectome.connectivity_states (csrc/dynstates.hip:
gnm_states_assign, gnm_states_accumulate, gnm_states_finish) on a resident FC stack, next to a plain torch restatement
on the same device data, and of connectivity_states_from_timeseries, which recomputes the FC chunk by chunk, next to the
recomputation alone.  One JSON line per case; times are wall-clock medians around a device synchronise, the routes
alternating inside one process.
    python tools/bench_dynstates.py [--S 64] [--series-S 932] [--T 1200] [--n 400] [--window 50] [--stride 10] [--k 5]
                                    [--reps 7] [--out FILE]
FC route (S subjects, FC resident): an iteration = assignment + accumulation over the chunks + the division + the one
integer read back; its parts timed apart as well; the bytes it must read (the real entries of the 64 x 64 upper block
pairs, once for the assignment and once for the update) against the 8 TB/s HBM figure.  The torch restatement: features
gathered from the upper triangle, the direct squared-distance form in fp64 over chunks of --torch-chunk windows,
index_add_ for the sums.  Series route (--series-S subjects, 0 to skip): an iteration next to `corr alone`, the window
means and fused correlation over the same chunks into the same buffer."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "graph-neural-mapping_amd"))
import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--S", type=int, default=64)
ap.add_argument("--series-S", type=int, default=932)
ap.add_argument("--T", type=int, default=1200)
ap.add_argument("--n", type=int, default=400)
ap.add_argument("--window", type=int, default=50)
ap.add_argument("--stride", type=int, default=10)
ap.add_argument("--k", type=int, default=5)
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--torch-chunk", type=int, default=256)
ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
args = ap.parse_args()
HBM = 8.0e12
lines = []


def emit(rec):
    lines.append(rec)
    print(json.dumps(rec), flush=True)


def med(ts):
    return 1e3 * float(np.median(ts))


import torch
from gnm import connectome as C
from gnm import states as ST

dev = torch.device("cuda:0")
T, n, window, stride, k = args.T, args.n, args.window, args.stride, args.k


def sync():
    torch.cuda.synchronize()
    return time.perf_counter()


def series(S):
    """S subjects whose 200-row stretches follow one of k mixing matrices: windows that cluster"""
    g = torch.Generator(device=dev).manual_seed(S + T)
    r = max(2, n // 3)
    mix = torch.randn((k, n, r), generator=g, device=dev, dtype=torch.float64)
    seg = 200
    which = torch.randint(0, k, (S, (T + seg - 1) // seg), generator=g, device=dev)
    z = torch.randn((S, T, r), generator=g, device=dev, dtype=torch.float64)
    out = 0.5 * torch.randn((S, T, n), generator=g, device=dev, dtype=torch.float64)
    for s0 in range(0, T, seg):
        m = mix[which[:, s0 // seg]]                                    # [S, n, r]
        out[:, s0:s0 + seg] += torch.einsum("str,snr->stn", z[:, s0:s0 + seg], m)
    return out


def upper_block_bytes():
    nb = (n + 63) // 64
    size = [min(64, n - 64 * b) for b in range(nb)]
    return 8 * sum(size[i] * size[j] for i in range(nb) for j in range(i, nb))


def iteration(eng, cen, prev):
    eng.sweep(cen, True)
    changed = int((eng.labels != prev).sum().item())
    eng.finish(cen)
    return changed


def plans(S):
    ts = series(S)
    x = ts.reshape(S * T, n)
    w_beg_h, _, _ = C._plan_windows(np.arange(S + 1, dtype=np.int64) * T, window, stride)
    return ts, x, torch.from_numpy(w_beg_h).to(dev)


# ---------------------------------------------------------------------------------------------------- FC resident
S = args.S
ts, x, w_beg = plans(S)
W = int(w_beg.shape[0])
fc = C.dynamic_connectivity_from_timeseries(ts, window, stride).reshape(W, n, n)
start = np.linspace(0, W - 1, k).astype(np.int64)
eng = ST._fc_engine(fc, k)
iu, ju = torch.triu_indices(n, n, 1, device=dev)


def torch_iteration(cen, prev):
    Mf = cen[:, iu, ju]
    sums = torch.zeros((k, n, n), dtype=torch.float64, device=dev)
    labels = torch.empty(W, dtype=torch.int64, device=dev)
    for lo in range(0, W, args.torch_chunk):
        part = fc[lo:lo + args.torch_chunk]
        X = part[:, iu, ju]
        d = ((X[:, None, :] - Mf[None]) ** 2).sum(-1)
        labels[lo:lo + args.torch_chunk] = d.argmin(1)
        sums.index_add_(0, labels[lo:lo + args.torch_chunk], part)
    changed = int((labels != prev).sum().item())
    counts = torch.bincount(labels, minlength=k).clamp_(min=1)
    return sums / counts[:, None, None].double(), labels, changed


cen0 = fc[torch.from_numpy(start).to(dev)].clone()
cen = cen0.clone()
prev = torch.zeros(W, dtype=torch.int32, device=dev)
iteration(eng, cen, prev)                                               # warm-up of both routes, and their agreement
tc, tl, _ = torch_iteration(cen0, prev.long())
agree = float((tl.int() == eng.labels).double().mean())
cen_diff = float((torch.triu(tc) - torch.triu(cen)).abs().max())
it_t, as_t, ac_t, to_t = [], [], [], []
for _ in range(args.reps):
    cen = cen0.clone()
    t0 = sync()
    iteration(eng, cen, prev)
    t1 = sync()
    torch_iteration(cen0, prev.long())
    t2 = sync()
    eng.sweep(cen0, False)
    t3 = sync()
    with torch.cuda.device(dev):
        st = torch.cuda.current_stream(dev).cuda_stream
        eng.sum.zero_()
        eng.count.zero_()
        for lo, hi, part in eng.chunks():
            C.check(C.lib.gnm_states_accumulate(part.data_ptr(), eng.labels[lo:].data_ptr(), hi - lo, n, k,
                                                eng.sum.data_ptr(), eng.count.data_ptr(), st), "gnm_states_accumulate")
    t4 = sync()
    it_t.append(t1 - t0); to_t.append(t2 - t1); as_t.append(t3 - t2); ac_t.append(t4 - t3)
must = 2.0 * W * upper_block_bytes()
full = C.connectivity_states(fc, k, init=start)
emit({"bench": "dynstates_fc", "S": S, "T": T, "n": n, "window": window, "stride": stride, "k": k, "windows": W,
      "fc_gb": W * n * n * 8 / 1e9, "reps": args.reps, "iteration_ms": med(it_t),
      "iteration_ms_all": [round(1e3 * t, 3) for t in it_t], "us_per_window": 1e3 * med(it_t) / W,
      "assign_ms": med(as_t), "accumulate_ms": med(ac_t), "must_read_gb": must / 1e9,
      "must_read_tb_per_s": must / float(np.median(it_t)) / 1e12, "frac_of_hbm": must / float(np.median(it_t)) / HBM,
      "assign_frac_of_hbm": 0.5 * must / float(np.median(as_t)) / HBM,
      "accumulate_frac_of_hbm": 0.5 * must / float(np.median(ac_t)) / HBM,
      "torch_iteration_ms": med(to_t), "torch_iteration_ms_all": [round(1e3 * t, 3) for t in to_t],
      "torch_over_kernels": med(to_t) / med(it_t), "labels_agreeing_with_torch": agree,
      "max_abs_centroid_minus_torch": cen_diff, "full_run_iterations": full.n_iter, "full_run_converged": full.converged,
      "full_run_counts": full.counts.tolist()})
del fc, eng, ts, x, w_beg, cen, cen0, full
torch.cuda.empty_cache()

# ---------------------------------------------------------------------------------------------------- series resident
if args.series_S > 0:
    S = args.series_S
    ts, x, w_beg = plans(S)
    W = int(w_beg.shape[0])
    eng = ST._series_engine(x, w_beg, window, None, n, k)
    start = np.linspace(0, W - 1, k).astype(np.int64)
    cen0 = eng.pick(start).clone()
    prev = torch.zeros(W, dtype=torch.int32, device=dev)
    iteration(eng, cen0.clone(), prev)
    it_t, corr_t = [], []
    for _ in range(args.reps):
        cen = cen0.clone()
        t0 = sync()
        iteration(eng, cen, prev)
        t1 = sync()
        for _lo, _hi, _part in eng.chunks():
            pass
        t2 = sync()
        it_t.append(t1 - t0); corr_t.append(t2 - t1)
    emit({"bench": "dynstates_series", "S": S, "T": T, "n": n, "window": window, "stride": stride, "k": k, "windows": W,
          "fc_if_materialised_gb": W * n * n * 8 / 1e9, "chunk_budget_gb": C.DYNFC_WORK_BYTES / 1e9, "reps": args.reps,
          "iteration_ms": med(it_t), "iteration_ms_all": [round(1e3 * t, 3) for t in it_t],
          "us_per_window": 1e3 * med(it_t) / W, "corr_alone_ms": med(corr_t),
          "corr_alone_ms_all": [round(1e3 * t, 3) for t in corr_t],
          "clustering_over_corr": (med(it_t) - med(corr_t)) / med(corr_t)})
if args.out:
    with open(args.out, "a") as f:
        for rec in lines:
            f.write(json.dumps(rec) + "\n")
