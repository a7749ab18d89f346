#!/usr/bin/env python3
"""Headline benchmark: graphs/sec, forward + backward, of the GIN hot path on MI355X.

    python bench.py --gpus N --steps K --warmup W [--full]      (N > 1: launched by torch.distributed.run)

Workload at N = 1 (BASELINE.json configs[1]): batches of 1024 synthetic 400-node dense-FC
connectivity graphs (47,600 directed edges each), 7 input features, hidden 64, 5 GIN
layers, 2-layer MLPs, sum/sum pooling, learn_eps, train mode, final_dropout 0.5.  One step
= one full GIN_InfoMaxReg.forward (encoder + readout + classifier + Infomax
discriminator) + the reference loss CE + 0.05*BCE (main.py:34-37) + backward; the graph
pool (CSR + features) and labels are resident in HBM before the timed region.  For N > 1
every rank owns `--batch` graphs per step (weak scaling, configs[2] at --batch 512) and the
step ends with ONE RCCL all-reduce of the flat gradient buffer.

Prints one JSON line (rank 0).  A plain run does only what the headline needs: set-up, warm-up, the timed steps,
--dump-outputs, the line.  --full adds the figures that cost time or launches of their own: `cpu_baseline`, the CSR
gather timing next to the matrix-core kernel (`roofline.csr_gather`) and, when no timed step carried HIP events
(--graph on, N > 1), a few eager steps after the timed region for `kernel_ms` and the rooflines.  Extra objects:
  roofline      the sum-aggregation kernel at F = 64 (forward launches, as the step runs them: with the
                previous layer's BatchNorm+ReLU+readout on the tile load): bytes per launch / mean launch duration
                from HIP events on the launch stream, against 8 TB/s.  Bytes: for the matrix-core kernel the bytes
                its algorithm MOVES (features in + out + bit adjacency; the PMC-measured traffic when on record), with
                SURVEY.md 8(d)'s CSR-canonical count (396,804 B per graph-layer) as `frac_csr_equivalent`; for the CSR
                gather kernels the canonical count itself.
  roofline_mlp  the Linear(64,64) forward launches: bytes in + out against 8 TB/s (the split-precision bf16 kernel
                is HBM-bound; with GNM_LIN_NO_SPLIT=1 the fp32-MFMA kernel against 157.3 TFLOP/s).
  cpu_baseline  (--full) oracle/gin_torch_cpu.py (torch-CPU restatement with the reference's own ATen operators,
                all host cores; pinned to the reference's golden vectors) timed on this host on config C1 (B = 32 of the
                same graphs), rank 0, N = 1 only; the numpy oracle's time next to it.

--dump-outputs DIR writes what the last timed step computed (loss, parameter gradients, BatchNorm running
statistics) as DIR/<name>.npy; the inputs are seeded, so two builds run with the same arguments compare file by file.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.join(ROOT, "graph-neural-mapping_amd")
for p in (ROOT, PKG):
    if p not in sys.path:
        sys.path.insert(0, p)
# multi-process GPU work on this pool needs dmabuf IPC (already exported on the boxes; kept if the launcher's
# environment was rebuilt) -- must be set before the HIP runtime initialises
os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")

import numpy as np
import torch
import torch.distributed as dist
import torch.nn.functional as F

import hashlib
import socket
import subprocess

AGG_BYTES_PER_GRAPH_LAYER = lambda n, E, Fw: 4 * n * Fw * 2 + 4 * E + 4 * (n + 1)
HBM_PEAK_GBS = 8000.0        # MI355X_MICROARCH.md: 8.0 TB/s spec (6.29 TB/s measured copy ceiling)
HBM_MEASURED_GBS = 6290.0
MFMA_F32_PEAK_TF = 157.3


def self_launch(args):
    """`python bench.py --gpus N` with no launcher around it: start the N ranks ourselves (one process per GPU
    through torch.distributed.run, rendezvous on 127.0.0.1), relay their output and exit code.  Runs BEFORE this
    process touches the GPU, and the ranks are children, never an exec over this process."""
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(args.gpus),
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    env.setdefault("OMP_NUM_THREADS", str(max(1, (os.cpu_count() or 8) // max(1, args.gpus))))
    return subprocess.call(cmd, env=env)


def file_sha256(path):
    h = hashlib.sha256()
    with open(path, "rb") as f:
        h.update(f.read())
    return h.hexdigest()


def measured_traffic(profile_json, csrc_dir, variant):
    """HBM bytes per 1024-graph launch of the aggregation kernel from the committed PMC summary -- but only while
    that entry was taken on THIS kernel source (each entry records the csrc file its kernel lives in and that file's
    sha256, tools/pmc_agg_summary.py); a stale entry yields (None, reason): a number that silently stops describing
    the kernel is worse than none."""
    if not os.path.exists(profile_json):
        return None, "no PMC summary (%s)" % os.path.basename(profile_json)
    ent = json.load(open(profile_json)).get(variant)
    if not isinstance(ent, dict):
        return None, "no '%s' entry in %s" % (variant, os.path.basename(profile_json))
    src = ent.get("kernel_source")
    if not src or "sha256" not in ent:
        return None, "stale: the '%s' entry of %s predates per-entry source hashes" % (variant, os.path.basename(profile_json))
    have = file_sha256(os.path.join(csrc_dir, src))
    if ent["sha256"] != have:
        return None, "stale: '%s' was measured on %s %s, this is %s" % (variant, src, ent["sha256"][:12], have[:12])
    return float(ent["hbm_bytes_per_launch"]), ent["source"]


def step_roofline(B, ms_per_step):
    """The whole training step against HBM: the sum over ALL kernels of a step of their PMC traffic (2 x FETCH_SIZE +
    WRITE_SIZE, separate rocprofv3 --pmc passes over this same command: tools/pmc_step.sh -> profiles/step_traffic.json)
    divided by the step time of THIS run.  Dropped (null traffic) once any kernel source changed since the passes."""
    path = os.path.join(ROOT, "profiles", "step_traffic.json")
    if not os.path.exists(path):
        return {"bound": "hbm", "traffic": None, "traffic_source": "no profiles/step_traffic.json"}
    ent = json.load(open(path))
    have = csrc_sha256(os.path.join(PKG, "csrc"))
    if ent.get("csrc_sha256") != have:
        return {"bound": "hbm", "traffic": None, "traffic_source": "stale: profiles/step_traffic.json was measured on "
                "csrc %s, this is %s" % (str(ent.get("csrc_sha256"))[:12], have[:12])}
    bytes_step = float(ent["hbm_bytes_per_step"]) * B / float(ent["graphs_per_step"])
    ach = bytes_step / (ms_per_step * 1e-3) / 1e9
    return {"bound": "hbm", "achieved": ach, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": ach / HBM_PEAK_GBS,
            "frac_of_measured_copy_peak": ach / HBM_MEASURED_GBS, "traffic": bytes_step,
            "traffic_source": ent.get("source"), "kernels": ent.get("kernels"), "ms_per_step": ms_per_step}


def csrc_sha256(csrc_dir):
    h = hashlib.sha256()
    for f in sorted(os.listdir(csrc_dir)):
        if f.endswith((".hip", ".h", ".cpp")):
            h.update(f.encode())
            h.update(open(os.path.join(csrc_dir, f), "rb").read())
    return h.hexdigest()


DUMP_BUDGET_BYTES = 64 * 1000 * 1000


def step_outputs(model, loss):
    """What one training step hands its caller, as host float32 arrays: the loss, the gradient of every parameter
    (views of the flat gradient buffer) and the BatchNorm running statistics the step updated."""
    out = {"loss": np.asarray(loss.detach().float().cpu().numpy(), dtype=np.float32)}
    for name, p in model.named_parameters():
        if p.grad is not None:
            out["grad." + name] = p.grad.detach().float().cpu().numpy()
    for name, b in model.named_buffers():
        if b.is_floating_point():
            out["buffer." + name] = b.detach().float().cpu().numpy()
    return out


def write_outputs(outdir, arrays, budget=DUMP_BUDGET_BYTES):
    """DIR/<name>.npy for every array.  Over the budget, every array is cut to the same fraction of its elements: a
    fixed (seeded, sorted) sample of its flattened entries, so two runs keep the same positions.  (256 bytes per
    file are held back for the .npy header and the one element every array keeps.)"""
    os.makedirs(outdir, exist_ok=True)
    total = sum(a.nbytes for a in arrays.values())
    frac = min(1.0, (budget - 256 * len(arrays)) / float(total)) if total else 1.0
    sampled = []
    for name, a in sorted(arrays.items()):
        if frac < 1.0 and a.size > 1:
            k = max(1, int(a.size * frac))
            idx = np.sort(np.random.default_rng(0).choice(a.size, k, replace=False))
            a = a.reshape(-1)[idx]
            sampled.append(name)
        np.save(os.path.join(outdir, name + ".npy"), np.asarray(a, dtype=np.float32))
    print("bench: wrote %d arrays to %s%s" % (len(arrays), outdir,
                                              " (sampled: %s)" % ", ".join(sampled) if sampled else ""), file=sys.stderr)


def usable_cpus():
    """cores this process may actually run on: the affinity mask, cut by the cgroup CPU quota when there is one
    (os.cpu_count() is the machine's, and a thread per machine core inside a 16-core share only adds switching)"""
    n = os.cpu_count() or 1
    try:
        n = min(n, len(os.sched_getaffinity(0)))
    except Exception:
        pass
    for path in ("/sys/fs/cgroup/cpu.max", "/sys/fs/cgroup/cpu/cpu.cfs_quota_us"):
        try:
            txt = open(path).read().split()
            if path.endswith("cpu.max"):
                if txt[0] != "max":
                    n = min(n, max(1, int(float(txt[0]) / float(txt[1]) + 0.5)))
            else:
                q = int(txt[0])
                if q > 0:
                    per = int(open("/sys/fs/cgroup/cpu/cpu.cfs_period_us").read())
                    n = min(n, max(1, int(q / per + 0.5)))
            break
        except Exception:
            continue
    return max(1, n)


def cpu_baseline(graphs, state, budget_s=30.0, with_numpy_oracle=False):
    """CPU baseline on config C1 (32 graphs, fwd + loss + bwd, fp32) on this host's cores, both variants SURVEY.md 8(d)
    asks for -- (ii) the full step with the Infomax tail and (i) encoder + classifier only -- from two restatements:
      * `value`: oracle/gin_torch_cpu.py, the torch-CPU restatement 8(d) specifies (the reference's own ATen operators
        and cost structure: COO spmm, nn.Bilinear's trilinear autograd), torch.set_num_threads(os.cpu_count());
      * `numpy_oracle`: oracle/gin_oracle.py, the parity checker (restructured discriminator: faster than the reference)."""
    from oracle import gin_oracle as O
    from oracle.gin_torch_cpu import TorchCpuGIN
    ncpu = usable_cpus()
    try:
        from threadpoolctl import threadpool_info
        blas_threads = max([p.get("num_threads", 1) for p in threadpool_info()] + [1])
    except Exception:
        blas_threads = ncpu
    ob = [O.OGraph(len(g.g), g.edge_mat.numpy(), g.node_features.numpy(), g.label) for g in graphs]
    rng = np.random.default_rng(0)
    perm = rng.permutation(len(ob))

    def timed(fn, budget, warm=3, n=10):
        """`warm` warm-up steps, then `n` timed ones, median reported -- cut short only when the host
        cannot afford it: a first step that alone exceeds the budget IS the sample, and the timed loop stops at the
        budget (the baseline must stay bounded on any host: an unbounded loop once ran into the driver's limit on a box
        whose cgroup gave the job a fraction of the cores torch had threads for).  Returns (times, warm-ups done)."""
        t_start = time.perf_counter()
        t0 = time.perf_counter()
        fn()
        first = time.perf_counter() - t0
        if first > budget:
            return [first], 0
        done = 1
        while done < warm and time.perf_counter() - t_start + first < 0.3 * budget:
            fn()
            done += 1
        ts = []
        while len(ts) < n and (not ts or time.perf_counter() - t_start + float(np.median(ts)) < budget):
            t0 = time.perf_counter()
            fn()
            ts.append(time.perf_counter() - t0)
        return ts, done

    old_threads = torch.get_num_threads()
    torch.set_num_threads(ncpu)
    try:
        tmodel = TorchCpuGIN(state, 5, 2, True, "sum", "sum")
        t_ii, w_ii = timed(lambda: tmodel.train_step(ob, perm, 0.05, True), budget_s * 0.8)
        t_i, w_i = timed(lambda: tmodel.train_step(ob, perm, 0.05, False), budget_s * 0.2)
        torch_threads = torch.get_num_threads()
    finally:
        torch.set_num_threads(old_threads)
    numpy_leg = None
    if with_numpy_oracle:       # (--numpy-oracle: the parity checker's own time; off by default since round 4 -- the
        #                          protocol above needs the budget)
        model = O.OracleGIN(state, 5, 2, True, "sum", "sum", dtype=np.float32)
        n_ii, _ = timed(lambda: model.train_step_grads(ob, perm, update_running=False, want_disc=True), 8.0, 1, 5)
        n_i, _ = timed(lambda: model.train_step_grads(ob, perm, update_running=False, want_disc=False), 5.0, 1, 5)
        numpy_leg = {"value": len(ob) / float(np.median(n_ii)), "unit": "graphs/s", "cores": int(blas_threads),
                     "encoder_classifier_only": len(ob) / float(np.median(n_i)),
                     "sample": "oracle/gin_oracle.py (the parity checker): numpy dense algebra on BLAS threads + "
                               "scipy CSR spmm on ONE thread, discriminator restructured as two GEMMs + row dots "
                               "(no [N,LH,LH]-sized trilinear intermediates, so faster than the reference's "
                               "path); median of %d / %d steps" % (len(n_ii), len(n_i))}
    med = lambda ts: float(np.median(ts))
    cpu = "unknown"
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                cpu = line.split(":", 1)[1].strip()
                break
    except Exception:
        pass
    return {"value": len(ob) / med(t_ii), "unit": "graphs/s", "cores": int(torch_threads), "kind": "port",
            "sample": "config C1: %d dense-FC 400-node graphs, fwd+loss+bwd WITH the Infomax tail (variant ii), fp32, "
                      "torch-CPU restatement (oracle/gin_torch_cpu.py), %d warm-up + median of %d timed steps (%.2f s each; "
                      "SURVEY.md 8(d) asks for 3 + 10, a slow host gets fewer inside the %.0f s budget)"
                      % (len(ob), w_ii, len(t_ii), med(t_ii), budget_s),
            "encoder_classifier_only": {"value": len(ob) / med(t_i), "unit": "graphs/s",
                                        "sample": "variant (i): same graphs, CE(c_logit) only, no discriminator; "
                                                  "%d warm-up + median of %d steps (%.2f s each)"
                                                  % (w_i, len(t_i), med(t_i))},
            "what_it_is": "oracle/gin_torch_cpu.py: the reference's own ATen operators on the host cores "
                          "(torch.spmm on the uncoalesced COO block adjacency, F.linear, F.batch_norm, F.bilinear with "
                          "its trilinear autograd) with torch.set_num_threads(cores the job may use: affinity mask and "
                          "cgroup quota, os.cpu_count() otherwise); pinned to the "
                          "reference's golden vectors (tests/test_torch_cpu_baseline.py).  Survey container, real "
                          "reference, 8 cores: 7.3 graphs/s.  Restated with the reference's cost structure since "
                          "round 3 (rounds 1-2 timed the numpy oracle here, whose restructured discriminator made it "
                          "about twice as fast: 36-46 graphs/s).  A reported baseline, not the optimisation target",
            "numpy_oracle": numpy_leg,
            "host_cpu": cpu, "host_logical_cpus": os.cpu_count(), "usable_cpus": ncpu}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=None, help="graphs per GPU per step (default 1024; 512 when --gpus > 1)")
    ap.add_argument("--pool", type=int, default=None,
                    help="distinct graphs resident per GPU (default 4096 = SURVEY.md 8(d), 390 MB of column ids: more "
                         "than the 256 MiB Infinity Cache; 512 for the sparse config)")
    ap.add_argument("--selftest-launch", action="store_true",
                    help="CPU check of the N > 1 launch path: the ranks only rendezvous (gloo), all-reduce one number "
                         "and rank 0 prints a stub JSON line; no GPU is touched")
    ap.add_argument("--hidden", type=int, default=64)
    ap.add_argument("--layers", type=int, default=5)
    ap.add_argument("--config", default="c2", choices=["c2", "c4"],
                    help="c2: 400-node dense-FC graphs, hidden 64 (headline); c4: 1000-node kNN k=20, hidden 128")
    ap.add_argument("--graph", choices=["auto", "on", "off"], default="auto",
                    help="replay the step from a captured hipGraph.  auto: N > 1 replays every timed step (whichever of "
                         "replay / eager is faster with the job's collective); N = 1 replays too, except every 10th timed "
                         "step, which is launched eagerly so that HIP events can bracket the roofline kernels INSIDE the "
                         "timed region.  An all-eager step costs ~2 ms of host time against ~3 ms of GPU time: on a box "
                         "whose host is busy it is host-bound (4.1 ms measured once), replay is not.  off: all eager")
    ap.add_argument("--neighbor-pooling", default="sum", choices=["sum", "average", "max"],
                    help="max: outside the north_star (csrc/maxpool.hip), eager launches only, no roofline object")
    ap.add_argument("--graph-pooling", default="sum", choices=["sum", "average"])
    ap.add_argument("--keep-pct", type=float, default=30.0,
                    help="dense-FC graphs: percent of the correlation matrix kept as edges (30 = the reference's "
                         "default --sparsity 30 -> 47,600 directed edges; 100 = complete graph, 159,600)")
    ap.add_argument("--no-learn-eps", action="store_true")
    ap.add_argument("--no-direct-grads", action="store_true",
                    help="let autograd accumulate parameter gradients instead of writing them into the flat buffer")
    ap.add_argument("--agg0-cache", action="store_true",
                    help="take layer 0's parameter-independent A.X from the arena's per-graph cache instead of "
                         "aggregating the input features inside every step (off: the step does all the work)")
    ap.add_argument("--sync-bn", action="store_true",
                    help="N > 1: BatchNorm over the union batch (20 tiny all-reduces per step, eager launches)")
    ap.add_argument("--torch-loss", action="store_true",
                    help="compute CE + 0.05*BCE with torch ops (as main.py does) instead of the fused loss kernel")
    ap.add_argument("--full", action="store_true",
                    help="also measure what the headline does not need: the CPU baseline (up to ~30 s), the CSR gather "
                         "kernel next to the matrix-core one, and kernel times on extra eager steps when no timed step "
                         "carried HIP events")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="--full without the CPU baseline")
    ap.add_argument("--numpy-oracle", action="store_true",
                    help="--full: also time oracle/gin_oracle.py (the numpy parity checker) next to the torch-CPU port")
    ap.add_argument("--no-kernel-timer", action="store_true")
    ap.add_argument("--time-all-kernels", action="store_true",
                    help="HIP events around every launch (default: only the two kernels the rooflines are quoted on)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last timed step handed its caller (the loss, every "
                         "parameter gradient, the BatchNorm running statistics) as DIR/<name>.npy, float32, at most "
                         "64 MB in all (rank 0)")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")

    if args.gpus > 1 and "RANK" not in os.environ:
        sys.exit(self_launch(args))                 # no launcher around us: be the launcher (nothing touched the GPU yet)
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        raise SystemExit("--gpus %d but WORLD_SIZE=%d" % (args.gpus, world))
    if args.selftest_launch:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if world > 1:
            dist.init_process_group("gloo", rank=rank, world_size=world)
        t = torch.tensor([float(rank + 1)], dtype=torch.float64)
        if world > 1:
            dist.all_reduce(t)
            dist.destroy_process_group()
        if rank == 0:
            print(json.dumps({"selftest_launch": True, "n_gpus": world, "rank_sum": float(t.item())}))
        return
    # test hook (1-GPU box): GNM_BENCH_SHARE_GPU=1 puts every rank on cuda:0 and uses gloo, which exercises the
    # whole N > 1 code path except RCCL itself
    share = os.environ.get("GNM_BENCH_SHARE_GPU") == "1"
    if share:
        local_rank = 0
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    # test hook (1-GPU box): GNM_BENCH_FORCE_DIST=1 initialises RCCL ("nccl") at world size 1 and runs the N > 1 step
    # path on it -- communicator init, the AVG all-reduce of the flat gradients, its capture into the step's hipGraph,
    # the launch-mode trial.  Two ranks cannot share a GPU under RCCL, so this is as much of the multi-GPU path as one
    # GPU can execute; the reported line is labelled.
    forced = world == 1 and os.environ.get("GNM_BENCH_FORCE_DIST") == "1"
    if forced:
        os.environ["GNM_DP_FORCE_COLLECTIVE"] = "1"
    multi = world > 1 or forced
    if multi:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if forced and "MASTER_PORT" not in os.environ:
            with socket.socket() as sk:
                sk.bind(("127.0.0.1", 0))
                os.environ["MASTER_PORT"] = str(sk.getsockname()[1])
        if share:
            dist.init_process_group("gloo", rank=rank, world_size=world)
        else:
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)

    from gnm import core, synth
    from gnm.parallel import DataParallelGIN, seed_rank_rng
    from models.graphcnn import GIN_InfoMaxReg

    sparse = args.config == "c4"
    B = args.batch or ((1024 if world == 1 else 512) if not sparse else 256)
    pool_n = args.pool or (4096 if not sparse else 512)
    if args.neighbor_pooling == "max":      # Python neighbour lists per graph (as the reference holds them): keep it small
        B = args.batch or 256
        pool_n = args.pool or B
    n, f0, H, L, C = (1000 if sparse else 400), 7, (128 if sparse else args.hidden), args.layers, 2

    t_gen = time.perf_counter()
    if sparse:
        pool = synth.make_pool("knn", pool_n, first=rank * pool_n, n=n, f0=f0)
    else:
        pool = synth.make_pool("dense_fc", pool_n, first=rank * pool_n, n=n, f0=f0, keep_pct=args.keep_pct)
    torch.manual_seed(0)
    model = GIN_InfoMaxReg(L, 2, f0, H, C, 0.5, not args.no_learn_eps, args.graph_pooling, args.neighbor_pooling,
                           dev).to(dev)
    state_cpu = {k: v.detach().cpu().numpy().copy() for k, v in model.state_dict().items()}
    model.train()
    dp = DataParallelGIN(model, direct_grads=not args.no_direct_grads, sync_bn=args.sync_bn and world > 1)
    dp.broadcast_parameters()
    arena = model.arena()
    gids_all = np.array(arena.add_many(pool), dtype=np.int64)
    labels_all = torch.tensor([g.label for g in pool], dtype=torch.int64, device=dev)
    E = int(pool[0].edge_mat.shape[1])
    t_gen = time.perf_counter() - t_gen

    rng = np.random.default_rng(1234 + rank)
    seed_rank_rng(99, rank)
    nsteps = args.warmup + args.steps
    # main.py:26: a random B-subset of the pool without replacement (with replacement only if the pool is smaller) -- the
    # data loader's draw.  Everything the reference's forward does with the chosen graphs (graphcnn.py:84-134, 195: the
    # block adjacency, the readout segments, X_concat) has its counterpart in assemble(), which runs INSIDE the timed
    # step since round 4: O(B) host index arithmetic, two pinned uploads, six small device gathers.
    sels = [rng.permutation(pool_n)[:B] if pool_n >= B else rng.integers(0, pool_n, B) for _ in range(nsteps)]
    labels_by_gid = torch.zeros(int(gids_all.max()) + 1, dtype=torch.int64, device=dev)
    labels_by_gid[torch.as_tensor(gids_all, device=dev)] = labels_all

    def assemble(i):
        bt = arena.batch_from_gids(gids_all[sels[i]])
        return bt, labels_by_gid[bt.gids]

    prebuilt = None
    if args.neighbor_pooling == "max":
        # the neighbour lists the reference's max pooling reads (graphcnn.py:55-81), built from the SAME selection
        # as the batch's CSR and features; Python lists per graph -> device arrays per batch, untimed (outside the
        # north_star; `batch_assembly` says so in the line)
        from gnm.maxnb import MaxNeighbours
        prebuilt = []
        for i in range(nsteps):
            bt, lab = assemble(i)
            for j in sels[i]:
                if getattr(pool[j], "neighbors", None) is None:
                    pool[j].build_neighbors()
            bt.maxnb = MaxNeighbours([pool[j] for j in sels[i]], args.no_learn_eps, dev)
            prebuilt.append((bt, lab))
    template = assemble(0)[0] if prebuilt is None else prebuilt[0][0]
    # replayed steps take the ids, labels and permutation through ONE pinned upload (CapturedTrainStep.run_gids)
    labels_host = np.array([g.label for g in pool], dtype=np.int64)
    packed_gids = gids_all[sels[0]] if (prebuilt is None and template.equal_n) else None
    N = template.N
    d_labels = torch.cat([torch.ones(N, 1), torch.zeros(N, 1)], 0).to(dev)   # main.py:32, sized by node count

    if args.torch_loss:
        def loss_fn(c_logit, d_logit, lab):
            return F.cross_entropy(c_logit, lab) + 0.05 * F.binary_cross_entropy_with_logits(d_logit, d_labels)
    else:
        from gnm.train import infomax_loss

        def loss_fn(c_logit, d_logit, lab):        # the same two losses, one fused pass (gnm_loss_ce_bce)
            return infomax_loss(c_logit, d_logit, lab, 0.05)[0]

    use_graph = args.graph in ("on", "auto") and not args.sync_bn and args.neighbor_pooling != "max"
    # N = 1, auto: replayed steps with an eager step (HIP events on the roofline kernels) every `timer_every`
    hybrid = args.graph == "auto" and not multi and not args.no_kernel_timer
    captured = captured_cc = None
    capture_notes = {}
    if use_graph:
        from gnm.graphs import CapturedTrainStep
        try:
            captured = CapturedTrainStep(model, template, loss_fn, zero_grad=dp.zero_grad,
                                         agg0_cache=args.agg0_cache, gids_host=packed_gids)
        except Exception as e:                      # capture is an optimisation: fall back to eager launches
            print("hipGraph capture failed (%s: %s); running eagerly" % (type(e).__name__, e), file=sys.stderr)
            capture_notes["step"] = "%s: %s" % (type(e).__name__, e)
            captured = None
            dp.fp.zero_grad()
        # (opt-in, GNM_BENCH_CC_CAPTURE=1: at world size 1 the replay with the collective inside measured 1.560 ms against
        #  1.497 ms with the collective launched behind the graph -- nothing to gain -- and a capture that went wrong on
        #  ONE rank of a real multi-GPU job would leave the others waiting in a collective.  The forced single-rank test
        #  hook turns it on, so the path stays exercised on RCCL.)
        if captured is not None and multi and not share and (forced or os.environ.get("GNM_BENCH_CC_CAPTURE") == "1"):
            # N > 1 on RCCL: a second graph with the gradient all-reduce recorded INSIDE it, behind the backward
            # (one replay per step, no launch between the last kernel and the collective).  Whether RCCL's
            # all-reduce captures is a property of the installed build: on any failure the step keeps the
            # collective outside.  Which variant runs is decided by the timed trial below.
            try:
                captured_cc = CapturedTrainStep(model, template, loss_fn, zero_grad=dp.zero_grad,
                                                agg0_cache=args.agg0_cache, post_backward=dp.allreduce_gradients,
                                                gids_host=packed_gids)
            except Exception as e:
                print("capturing the all-reduce inside the step's hipGraph failed (%s: %s); it stays outside"
                      % (type(e).__name__, e), file=sys.stderr)
                capture_notes["step+allreduce"] = "%s: %s" % (type(e).__name__, e)
                captured_cc = None
    if multi and world > 1:
        # every rank must run the same launch mode (the trial below and the steps call collectives): a capture that
        # failed on ONE rank demotes all of them
        ok = torch.tensor([int(captured is not None), int(captured_cc is not None)], dtype=torch.int32,
                          device=dev if dist.get_backend() == "nccl" else "cpu")
        dist.all_reduce(ok, op=dist.ReduceOp.MIN)
        ok = ok.cpu().tolist()
        if not ok[0] and captured is not None:
            captured = None
            dp.fp.zero_grad()
        if not ok[1]:
            captured_cc = None
    perms = [np.random.permutation(B) for _ in range(nsteps)]     # graphcnn.py:199, one draw per forward

    # launch mode of a step: "graph+cc" (replay incl. the collective), "graph" (replay, collective launched behind
    # it), "eager"
    mode = "graph" if captured is not None else "eager"

    def feats(bt):          # explicit X = aggregate it in the step; None = arena cache (--agg0-cache)
        return None if args.agg0_cache else arena.features(bt)

    def step(i, eager=False):
        replay = (mode in ("graph", "graph+cc")) and not eager
        if replay and packed_gids is not None:
            # batch assembly of a replayed step: host index arithmetic + one upload, inside the timed region
            cap = captured_cc if mode == "graph+cc" else captured
            loss = cap.run_gids(gids_all[sels[i]], labels_host[sels[i]], perms[i])
            if mode == "graph+cc":
                return loss                                      # the all-reduce is part of the replayed graph
            dp.allreduce_gradients()
            return loss
        bt, lab = assemble(i) if prebuilt is None else prebuilt[i]
        if mode == "graph+cc" and not eager:
            return captured_cc.run(bt, lab, perms[i])           # the all-reduce is part of the replayed graph
        if mode == "graph" and not eager:
            loss = captured.run(bt, lab, perms[i])
        else:
            dp.zero_grad()
            c_logit, d_logit = model.forward_batch(bt, X=feats(bt), perm=perms[i])
            loss = loss_fn(c_logit, d_logit, lab)
            loss.backward()
        dp.allreduce_gradients()
        return loss

    for i in range(args.warmup):
        step(i)
    trial_ms = None
    if captured is not None and args.graph == "auto" and multi:
        # the launch modes are bitwise equivalent; keep whichever is fastest together with this job's collective
        # (decided once, on untimed steps, identically on every rank: the times are MAX-reduced)
        from gnm.parallel import choose_launch_mode

        def measure(name, n=3):
            nonlocal mode
            mode = name
            step(0)
            torch.cuda.synchronize()
            dist.barrier()
            t0 = time.perf_counter()
            for i in range(n):
                step(i % nsteps)
            torch.cuda.synchronize()
            tt = torch.tensor([time.perf_counter() - t0], dtype=torch.float64, device=dev)
            dist.all_reduce(tt, op=dist.ReduceOp.MAX)
            return float(tt.item()) / n
        cands = (["graph+cc"] if captured_cc is not None else []) + ["graph", "eager"]
        def agree(ok):       # every rank drops the same candidates (a rank that failed has left its collectives)
            f = torch.tensor([int(ok)], dtype=torch.int32, device=dev if dist.get_backend() == "nccl" else "cpu")
            dist.all_reduce(f, op=dist.ReduceOp.MIN)
            return bool(int(f.item()))
        trial_errors = {}
        mode, trial_s = choose_launch_mode(cands, measure, agree=agree, errors=trial_errors)
        trial_ms = {k: 1e3 * v for k, v in trial_s.items()}
        if trial_errors:
            capture_notes["launch_mode_trial_errors"] = trial_errors
    elif captured_cc is not None and args.graph == "on":
        mode = "graph+cc"
    if mode == "eager":
        captured = None
    elif mode == "graph+cc":
        captured = captured_cc
    kernel_timer = None
    if not args.no_kernel_timer and (captured is None or hybrid):
        kernel_timer = core.KernelTimer(None if args.time_all_kernels else
                                        ("agg_fwd_F%d" % H, "agg_bwd_F%d" % H, "lin_fwd_K%d_H%d" % (H, H)))
    # the HIP events of the roofline kernels cost ~2 % of a step when recorded on every launch: they are recorded on
    # every 4th timed step.  In the hybrid mode the steps that carry them are EAGER steps, which a busy host stretches
    # (measured: 1.5-2.7 % on the run's average at every 4th): every 10th there (still inside the timed region: 2 steps
    # x 4 / 4 / 9 launches of the three roofline kernels at the default --steps 20)
    timer_every = 1 if args.time_all_kernels or args.steps < 8 else (10 if hybrid and args.steps >= 20 else 4)
    if multi:
        dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(args.warmup, nsteps):
        # (the eager steps sit in the MIDDLE of their stride: the host needs longer to launch one than the GPU to run it, which
        #  shows only when the GPU queue is empty -- as it is at the first timed step, right behind the synchronisation)
        core.TIMER = kernel_timer if (i - args.warmup) % timer_every == timer_every // 2 else None
        loss = step(i, eager=core.TIMER is not None)
    core.TIMER = kernel_timer
    t_enqueued = time.perf_counter() - t0        # host time to enqueue all steps (no sync inside)
    torch.cuda.synchronize()
    if multi:
        dist.barrier()
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    timer, core.TIMER = core.TIMER, None
    if multi:
        t = torch.tensor([elapsed], dtype=torch.float64, device=dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
    if args.dump_outputs and rank == 0:
        # before anything below launches more work on the model (the eager roofline steps overwrite the gradients)
        write_outputs(args.dump_outputs, step_outputs(model, loss))
    loss_val = float(loss.item())
    rank_check = None
    if multi:
        # What the ranks must agree on after a step: the parameters (broadcast once, then only read here) and the
        # all-reduced flat gradient (bitwise: every rank ends with the same ring result).  Their local losses differ --
        # each rank owns its own graphs -- and are listed.  Gathered on the host through the job's own backend.
        mine = torch.tensor([float(dp.fp.flat.double().sum().item()), float(dp.fp.flat_grad.double().sum().item()),
                             float(dp.fp.flat_grad.double().abs().sum().item()), loss_val], dtype=torch.float64)
        gath = [torch.zeros_like(mine) for _ in range(world)]
        if dist.get_backend() == "nccl":
            gd = [g.to(dev) for g in gath]
            dist.all_gather(gd, mine.to(dev))
            gath = [g.cpu() for g in gd]
        else:
            dist.all_gather(gath, mine)
        allv = torch.stack(gath).numpy()
        rank_check = {"params_agree_after_broadcast": bool((allv[:, 0] == allv[0, 0]).all()),
                      "grads_agree_after_allreduce": bool((allv[:, 1] == allv[0, 1]).all() and (allv[:, 2] == allv[0, 2]).all()),
                      "grad_abs_sum": float(allv[0, 2]), "final_loss_per_rank": [float(v) for v in allv[:, 3]]}

    if args.full and timer is None and not args.no_kernel_timer and rank == 0:
        # replayed steps carry no HIP events: time the two roofline kernels on a few eager steps of the same
        # batches, after (and outside) the timed region
        core.TIMER = core.KernelTimer(("agg_fwd_F%d" % H, "agg_bwd_F%d" % H, "lin_fwd_K%d_H%d" % (H, H)))
        for i in range(min(3, nsteps)):
            bt, lab = assemble(i) if prebuilt is None else prebuilt[i]
            c_logit, d_logit = model.forward_batch(bt, X=feats(bt), perm=perms[i])
            loss_fn(c_logit, d_logit, lab).backward()
        torch.cuda.synchronize()
        timer, core.TIMER = core.TIMER, None
    if not np.isfinite(loss_val):
        raise SystemExit("non-finite loss %r" % loss_val)
    if rank == 0:
        total_graphs = B * world * args.steps
        out = {
            "metric": "graphs/sec fwd+bwd, 400-node dense FC graphs, hidden_dim 64, 5 layers" if not sparse else
                      "graphs/sec fwd+bwd, 1000-node kNN(k=20) graphs, hidden_dim 128, 5 layers (BASELINE configs[3])",
            "value": total_graphs / elapsed, "unit": "graphs/s", "n_gpus": world, "steps": args.steps,
            "warmup": args.warmup, "ms_per_step": 1e3 * elapsed / args.steps, "higher_is_better": True,
            "scaling": "weak", "vs_baseline": None, "dtype": "f32", "data": "synthetic",
            "config": {"workload": "configs[%d]: %d x %d %s graphs/step (%d directed edges each), "
                                   "F0=7, hidden %d, %d GIN layers, 2-layer MLP, %s, "
                                   "full forward (classifier + Infomax discriminator) + CE+0.05*BCE + backward%s"
                                   % (3 if sparse else (1 if world == 1 else 2), world, B,
                                      "1000-node kNN(k=20)" if sparse else "dense-FC 400-node", E, H, L,
                                      "neighbor=%s/graph=%s%s" % (args.neighbor_pooling, args.graph_pooling,
                                                                  "" if args.no_learn_eps else ", learn_eps"),
                                      ", flat-gradient RCCL all-reduce" if world > 1 else ""),
                       "graphs_per_gpu": B, "global_batch": B * world, "nodes_per_graph": n, "edges_per_graph": E,
                       "pool_graphs_per_gpu": pool_n, "parallelism": "dp%d" % world},
            "final_loss": loss_val, "setup_seconds": round(t_gen, 1),
            "batch_assembly": ("inside the timed step (graphcnn.py:84-134, 195 in the reference's forward): replayed steps "
                               "-- arena ids, labels and permutation packed on the host, one pinned upload, feature "
                               "gather on the device; eager steps -- arena.batch_from_gids + label gather"
                               if prebuilt is None else
                               "outside the timed region (max pooling: Python neighbour lists per graph)"),
            "eager_fallbacks": int(getattr(captured, "eager_fallbacks", 0)) if captured is not None else None,
            "host_enqueue_ms_per_step": 1e3 * t_enqueued / args.steps,
            "launch_mode": ("eager" if captured is None else
                            "hipGraph replay, every %d%s timed step eager with HIP events on the roofline kernels"
                            % (timer_every, "th" if timer_every > 3 else "") if hybrid else
                            ("hipGraph replay with the RCCL all-reduce captured inside the graph" if mode == "graph+cc"
                             else "hipGraph replay")),
        }
        if multi:
            out["collective"] = {"backend": dist.get_backend(), "world": world,
                                 "op": "AVG (1/W inside the collective)" if dp._avg_ok else
                                       ("SUM + scale launch" if dp._avg_ok is False else "gloo staging (test hook)"),
                                 "avg_fallback_reason": dp.avg_fallback_reason, "launch_mode_trial_ms": trial_ms,
                                 "capture_notes": capture_notes or None, "launch_mode": mode,
                                 "rank_check": rank_check,
                                 "forced_single_rank_test_hook": bool(forced)}
        roof, roof_mlp = None, None
        default_cfg = (args.neighbor_pooling, args.graph_pooling, args.keep_pct, args.no_learn_eps) == \
            ("sum", "sum", 30.0, False)
        if timer is not None:
            summ = timer.summary()
            out["kernel_ms"] = {k: [c, round(ms, 4)] for k, (c, ms, _) in sorted(summ.items())}
            key = "agg_fwd_F%d" % H
            # one tag can hold two kernels (KernelTimer.summary keeps them apart as "tag|meta"): quote the roofline on
            # the variant the step launches most
            cands = [k for k in summ if k == key or k.startswith(key + "|")]
            if cands:
                c, ms, meta = summ[max(cands, key=lambda k: summ[k][0])]
                fused = bool(meta.get("fused_bnrelu"))
                bytes_launch = AGG_BYTES_PER_GRAPH_LAYER(n, E, H) * meta["B"]
                ach = bytes_launch / (ms * 1e-3) / 1e9
                # which kernel these launches were: the matrix-core kernel over the bit adjacency (csrc/aggm.hip, dense
                # batches), else csrc/agg.hip: the 64-wide tile kernel or feature slices
                fs = int(core.lib.gnm_agg_slice_width(H, n))
                if meta.get("mfma"):
                    kname = "gnm_aggm_kernel (MFMA over the bit adjacency, forward, F=%d%s)" % (
                        H, ", with fused BatchNorm+ReLU+readout prologue" if fused else "")
                    variant = "mfma_fused_bnrelu" if fused else "mfma_plain"
                elif fs == 64 and H == 64:
                    kname = "gnm_agg16_kernel (forward, F=64%s)" % (
                        ", with fused BatchNorm+ReLU+readout prologue" if fused else "")
                    variant = "fused_bnrelu" if fused else "plain"
                else:
                    kname = "gnm_agg_kernel<%d, %d> (forward%s, F=%d as %d slices of %d floats per graph)" % (
                        fs // 4, 1 if fused else 0, " with fused BatchNorm+ReLU+readout prologue" if fused else "", H,
                        (H + fs - 1) // fs, fs)
                    variant = "sliced_%sn%d_F%d" % ("fused_" if fused else "", n, H)
                traffic, traffic_src = None, "not measured for this configuration"
                if default_cfg:
                    # rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes (tools/pmc_agg.sh), counted on a 1024-graph
                    # launch; one workgroup per graph and slice, so it is linear in the graph count
                    per1024, traffic_src = measured_traffic(os.path.join(ROOT, "profiles", "agg_traffic.json"),
                                                            os.path.join(PKG, "csrc"), variant)
                    if per1024 is not None:
                        traffic = per1024 * meta["B"] / 1024.0
                csr_bytes_launch = bytes_launch
                if meta.get("mfma"):
                    # The matrix-core kernel never reads column ids: its algorithm moves features in + result out + the
                    # graph's bit adjacency (gnm_adj_bits_words: 26,624 B at n = 400) + the node offsets.  `achieved` /
                    # `frac` are quoted on THOSE bytes (the measured PMC traffic when the committed entry matches this
                    # kernel source, it agrees with the count to 0.3 %); SURVEY 8(d)'s CSR-canonical count, which this
                    # kernel does not move, is kept apart as `frac_csr_equivalent`.
                    bits_b = 4 * int(core.lib.gnm_adj_bits_words(n))
                    bytes_launch = (4 * n * H * 2 + bits_b + 4 * (n + 1)) * meta["B"]
                    ach = (traffic if traffic is not None else bytes_launch) / (ms * 1e-3) / 1e9
                roof = {"bound": "hbm", "kernel": kname, "achieved": ach,
                        "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": ach / HBM_PEAK_GBS,
                        "frac_of_measured_copy_peak": ach / HBM_MEASURED_GBS, "traffic": traffic,
                        "traffic_source": traffic_src,
                        "algorithmic_bytes_per_launch": bytes_launch, "mean_launch_ms": ms, "launches_timed": c,
                        "graph_layers_per_s": meta["B"] / (ms * 1e-3)}
                if meta.get("mfma"):
                    roof["achieved_is"] = ("measured HBM traffic (PMC) / launch time" if traffic is not None else
                                           "bytes the bit-adjacency algorithm moves (features in + out + bits) / launch time")
                    roof["csr_canonical_bytes_per_launch"] = csr_bytes_launch
                    roof["frac_csr_equivalent"] = csr_bytes_launch / (ms * 1e-3) / 1e9 / HBM_PEAK_GBS
                if traffic is not None:
                    # where the kernel moves fewer bytes than the canonical count (16-bit ids, or the bit
                    # adjacency of the matrix-core kernel), also quote the fraction of peak the MOVED bytes amount to
                    roof["frac_of_peak_from_traffic"] = traffic / (ms * 1e-3) / 1e9 / HBM_PEAK_GBS
                if fused and getattr(model._spec, "keep_hidden", False):
                    # the timed launches also apply the previous layer's BatchNorm+ReLU, write that activation
                    # (4nF bytes per graph, not part of SURVEY 8(d)'s canonical aggregation bytes) and its readout
                    # (only when the arrays are kept: by default the activation is not written at all)
                    extra = 4.0 * n * H * meta["B"]
                    roof["frac_incl_fused_activation_write"] = (bytes_launch + extra) / (ms * 1e-3) / 1e9 / HBM_PEAK_GBS
                if args.full and meta.get("mfma") and rank == 0:
                    # BASELINE.json's north_star describes the aggregation as a CSR neighbour-sum; dense batches run the
                    # matrix-core kernel instead.  The CSR gather kernel stays the general path:
                    # time it on the same batch here (outside the timed region, plain forward form) so that both
                    # fractions are on record.  GNM_DENSE_FILL=2 runs the whole step on it.
                    bt0 = template
                    xg = torch.randn(bt0.N, H, device=dev)
                    yg = torch.empty_like(xg)
                    was = bt0.dense
                    bt0.dense = False
                    try:
                        spec0 = model._spec
                        epsp = model.eps.data_ptr() + 4 if spec0.learn_eps else None
                        for _ in range(3):
                            core._agg(bt0, xg, yg, H, epsp, spec0, backward=False)
                        evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(20)]
                        for a_, b_ in evs:
                            a_.record(); core._agg(bt0, xg, yg, H, epsp, spec0, backward=False); b_.record()
                        torch.cuda.synchronize()
                        ms_g = float(np.median([a_.elapsed_time(b_) for a_, b_ in evs]))
                    finally:
                        bt0.dense = was
                    roof["csr_gather"] = {
                        "kernel": "gnm_agg16_kernel (CSR gather from the LDS tile, plain forward, F=%d), same batch, "
                                  "timed after the run" % H,
                        "median_launch_ms": ms_g, "launches_timed": 20,
                        "frac": csr_bytes_launch / (ms_g * 1e-3) / 1e9 / HBM_PEAK_GBS}
                bkey = "agg_bwd_F%d" % H
                bc = [k for k in summ if k == bkey or k.startswith(bkey + "|")]
                if bc:          # the backward launches (same canonical bytes: g in, dh out, same ids)
                    cb, msb, _ = summ[max(bc, key=lambda k: summ[k][0])]
                    roof["backward"] = {"mean_launch_ms": msb, "launches_timed": cb,
                                        "frac_csr_equivalent": csr_bytes_launch / (msb * 1e-3) / 1e9 / HBM_PEAK_GBS}
                    if meta.get("mfma"):
                        # the fused backward (gnm_aggm_bwd_stats) also reads Z of the layer below for the ReLU mask /
                        # BatchNorm sums: g in + Z in + dh out + bits (PMC: 357.2 MB per 1024-graph launch)
                        bwd_b, bsrc = None, None
                        if default_cfg:
                            bwd_b, bsrc = measured_traffic(os.path.join(ROOT, "profiles", "agg_traffic.json"),
                                                           os.path.join(PKG, "csrc"), "mfma_backward_stats")
                        bwd_bytes = bwd_b * meta["B"] / 1024.0 if bwd_b is not None else \
                            (4 * n * H * 3 + bits_b + 4 * (n + 1)) * meta["B"]
                        roof["backward"]["frac"] = bwd_bytes / (msb * 1e-3) / 1e9 / HBM_PEAK_GBS
                        roof["backward"]["bytes_per_launch"] = bwd_bytes
                        roof["backward"]["bytes_are"] = "PMC traffic" if bwd_b is not None else "g in + Z in + dh out + bits"
                    else:
                        roof["backward"]["frac"] = roof["backward"]["frac_csr_equivalent"]
            key = "lin_fwd_K%d_H%d" % (H, H)
            if key in summ:
                c, ms, meta = summ[key]
                fl = 2.0 * meta["N"] * H * H
                tf = fl / (ms * 1e-3) / 1e12
                gbs = (meta["N"] * H * 4 * 2) / (ms * 1e-3) / 1e9
                split = (H == 64 and os.environ.get("GNM_LIN_GENERIC") is None and
                         not any(os.environ.get(k, "0") not in ("", "0") for k in ("GNM_LIN_NO_SPLIT", "GNM_LIN_NO_STREAM")))
                if split:
                    # csrc/linear.hip gnm_lin_split_kernel: both operands as three exact bf16 planes, six bf16 MFMA
                    # terms per product -- the matrix pipe is no longer what the waves queue for; HBM is
                    roof_mlp = {"bound": "hbm", "kernel": "gnm_lin_split_kernel<2> (Linear %dx%d fwd, 3 x 3 bf16 planes, "
                                                          "6 MFMA terms)" % (H, H),
                                "achieved": gbs, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": gbs / HBM_PEAK_GBS,
                                "mean_launch_ms": ms, "launches_timed": c, "hbm_GBs": gbs,
                                "fp32_equivalent_TFLOPs": tf, "bf16_mfma_TFLOPs": 6 * tf,
                                "bf16_mfma_frac_of_2500": 6 * tf / 2500.0}
                elif H == 128 and os.environ.get("GNM_LIN_GENERIC") is None and \
                        not any(os.environ.get(k, "0") not in ("", "0") for k in ("GNM_LIN_NO_SPLIT",)):
                    # csrc/linear.hip gnm_lin_split128_kernel (configs[3]): K = H = 128 on the bf16 pipe, weight planes
                    # in LDS, A fragments straight from global memory: 20 us of matrix pipe against >= 52 us of
                    # traffic per 256,000-row launch -- HBM-bound
                    roof_mlp = {"bound": "hbm", "kernel": "gnm_lin_split128_kernel<false> (Linear %dx%d fwd, 3 x 3 bf16 "
                                                          "planes, 6 MFMA terms)" % (H, H),
                                "achieved": gbs, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": gbs / HBM_PEAK_GBS,
                                "mean_launch_ms": ms, "launches_timed": c, "hbm_GBs": gbs,
                                "fp32_equivalent_TFLOPs": tf, "bf16_mfma_TFLOPs": 6 * tf,
                                "bf16_mfma_frac_of_2500": 6 * tf / 2500.0}
                else:
                    roof_mlp = {"bound": "mfma", "kernel": "fp32-MFMA Linear kernels of csrc/linear.hip "
                                                          "(v_mfma_f32_32x32x2_f32; Linear %dx%d fwd)" % (H, H),
                                "achieved": tf, "peak": MFMA_F32_PEAK_TF, "unit": "TFLOP/s", "frac": tf / MFMA_F32_PEAK_TF,
                                "mean_launch_ms": ms, "launches_timed": c, "hbm_GBs": gbs}
        out["roofline"] = roof
        out["roofline_mlp"] = roof_mlp
        out["roofline_step"] = step_roofline(B, 1e3 * elapsed / args.steps) if (default_cfg and not sparse and world == 1
                                                                            and H == 64 and L == 5) else None
        if args.full and world == 1 and not args.no_cpu_baseline and not sparse and default_cfg:
            out["cpu_baseline"] = cpu_baseline(pool[:32], state_cpu, with_numpy_oracle=args.numpy_oracle)
        else:
            out["cpu_baseline"] = None
        print(json.dumps(out))
    if multi:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
