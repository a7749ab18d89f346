#!/usr/bin/env python3
"""Generate the disconnection goldens (disconnect/dc_*.npz) by running the REAL reference on CPU.

Run where the reference checkout is (it never travels to the GPU machine), like make_lesion_goldens.py:

    python tests/golden/make_disconnect_goldens.py

For every graph g of a case and each of its 5 set pairs (A, B) the reference's eval forward runs on an explicit edge-cut
copy (tests/test_disconnect_host.py cut_edges: every edge_mat column (u, v) with (u in A and v in B) or (u in B and v in
A) dropped, the column order kept, all n nodes and feature rows kept) and the class logits are stored, DATA ONLY:
  * em_{g}, feat_{g}     edge_mat [2, E] and node features [n, F0] of the SOURCE graph
  * a_{g}, b_{g}         the set pairs, uint8 [5, n] each (1 = in the set): the empty cut, one node against all nodes
                         (it is isolated), two disjoint random thirds, a random half within itself, all against all
  * base_{g}             the reference's eval forward([G_g]) c_logit, [C]
  * disconnected_{g}     c_logit of forward([G_g (/) (A, B)]) per pair, [5, C]   (NaN where the reference gives NaN)
  * state_<name>         the seeded state_dict (the discriminator's left out: it plays no part)
The 11 cases, shapes and graph kinds are the lesion goldens': graph pooling {sum, average} x neighbour pooling {sum,
average} x learn_eps {on, off}, one asymmetric edge_mat, one star-like graph and one one-hot input.  In the star-like
graph pair 1 is the hub against ONE LEAF, which leaves that leaf without neighbours.  Under average + learned eps an
isolated node is the 0/0 row: NaN, asserted here against expect_nan_cut.
"""
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import make_goldens as MG  # noqa: E402  (the reference import, SynthGraph, corr_graph, build_model)
from make_occlusion_goldens import B, C, F0, H, L, M, N_NODES, T, directed, hub_graph  # noqa: E402
from test_disconnect_host import cut_edges, expect_nan_cut  # noqa: E402

OUT_DIR = os.path.join(HERE, "disconnect")


def pairs_of(kind, seed, n):
    """the 5 set pairs of a graph: (A's, B's), bool [5, n] each"""
    rng = np.random.default_rng(seed)
    SA, SB = np.zeros((5, n), dtype=bool), np.zeros((5, n), dtype=bool)
    if kind == "hub":
        SA[1, 0] = True                         # the hub against one of its leaves: the leaf loses its only neighbour
        SB[1, n - 2] = True
    else:
        SA[1, rng.integers(0, n)] = True        # one node against all nodes: it is isolated
        SB[1] = True
    # (the star-like graph: from its ring nodes, which keep the hub, so that only pairs 1 and 4 isolate a node)
    pool = np.arange(1, n - 2) if kind == "hub" else np.arange(n)
    perm = rng.permutation(pool)
    SA[2, perm[:n // 3]] = True                 # two disjoint random thirds
    SB[2, perm[n // 3:2 * (n // 3)]] = True
    SA[3, rng.choice(pool, n // 2, replace=False)] = True
    SB[3] = SA[3]                               # a random half within itself
    SA[4] = SB[4] = True                        # all against all: the edgeless graph
    return SA, SB


def run_case(tag, model_seed, graph_seed, learn_eps, gpool, npool, kind="corr"):
    f0 = N_NODES if kind == "onehot" else F0
    graphs = []
    for g in range(B):
        if kind == "hub":
            graphs.append(hub_graph(graph_seed + g, N_NODES, f0))
            continue
        gs = graph_seed + g
        while True:         # every node with two neighbours, as the occlusion goldens
            und, feats, label = MG.corr_graph(gs, N_NODES, T, f0, keep_pct=45.0)
            if np.bincount(und.ravel(), minlength=N_NODES).min() >= 2:
                break
            gs += 100
        if kind == "onehot":
            feats = np.eye(N_NODES, dtype=np.float32)
        gr = MG.SynthGraph(N_NODES, und, feats, label)
        graphs.append(directed(gr, graph_seed + g) if kind == "asym" else gr)
    model = MG.build_model(model_seed, L, M, f0, H, C, 0.0, learn_eps, gpool, npool)
    gen = torch.Generator().manual_seed(model_seed + 5)
    with torch.no_grad():   # running statistics away from their defaults, so eval-mode BatchNorm matters
        for name, b in model.named_buffers():
            if name.endswith("running_mean"):
                b.copy_(0.1 * torch.randn(b.shape, generator=gen))
            elif name.endswith("running_var"):
                b.copy_(0.5 + torch.rand(b.shape, generator=gen))
    out = {"cfg": np.array([L, M, f0, H, C, int(learn_eps), B, N_NODES], dtype=np.int64),
           "gpool": np.array(gpool), "npool": np.array(npool)}
    for k, v in model.state_dict().items():
        if not k.startswith("disc."):
            out["state_" + k] = v.detach().numpy().copy()
    model.eval()
    for gi, gr in enumerate(graphs):
        SA, SB = pairs_of(kind, graph_seed + 31 * gi + 7, N_NODES)
        out[f"em_{gi}"] = gr.edge_mat.numpy().astype(np.int16)
        out[f"feat_{gi}"] = gr.node_features.numpy().copy()
        out[f"a_{gi}"] = SA.astype(np.uint8)
        out[f"b_{gi}"] = SB.astype(np.uint8)
        with torch.no_grad():
            np.random.seed(0)
            out[f"base_{gi}"] = model([gr])[0].numpy()[0].copy()
            dis = []
            for A, Bs in zip(SA, SB):
                np.random.seed(0)
                dis.append(model([cut_edges(gr, A, Bs)])[0].numpy()[0].copy())
        out[f"disconnected_{gi}"] = np.stack(dis)
        nan = np.isnan(out[f"disconnected_{gi}"])
        want = np.array([expect_nan_cut(gr, A, Bs, npool, learn_eps) for A, Bs in zip(SA, SB)])
        assert (nan.all(1) == want).all() and (nan.any(1) == want).all(), (tag, nan, want)
        if kind == "hub":
            assert want.tolist() == [False, True, False, False, True], (tag, want)
        assert np.isfinite(out[f"base_{gi}"]).all()
    out["labels"] = np.array([g.label for g in graphs], dtype=np.int64)
    os.makedirs(OUT_DIR, exist_ok=True)
    path = os.path.join(OUT_DIR, f"dc_{tag}.npz")
    np.savez_compressed(path, **out)
    print(f"dc_{tag}: {os.path.getsize(path) / 1024:.0f} KB")


def main():
    seed = 0
    for gpool in ("sum", "average"):
        for npool in ("sum", "average"):
            for le in (True, False):
                run_case(f"g{gpool}_n{npool}_eps{int(le)}", 70 + seed, 6000 + 10 * seed, le, gpool, npool)
                seed += 1
    run_case("asym_gaverage_naverage_eps0", 90, 6200, False, "average", "average", kind="asym")
    run_case("hub_gsum_naverage_eps1", 91, 6210, True, "sum", "average", kind="hub")
    run_case("onehot_gsum_nsum_eps1", 92, 6220, True, "sum", "sum", kind="onehot")


if __name__ == "__main__":
    main()
