#!/usr/bin/env python3
"""Generate the connectivity-saliency goldens (edge/edge_*.npz) by running the REAL reference on CPU.

Run where the reference checkout is (it never travels to the GPU machine), like make_goldens.py:

    python tests/golden/make_edge_saliency_goldens.py

The reference builds its block adjacency as a sparse tensor (models/graphcnn.py:84-106) and multiplies every layer's
input by it (:154-161, :178-182; under neighbour "average" also dividing by its row sums).  This script wraps the
instance's adjacency builder so the returned Adj_block is a coalesced sparse LEAF that requires grad, runs
compute_saliency([g], c) (:254-266, eval mode) and stores, per graph g and class c, DATA ONLY:
  * edge_{g}_{c}     Adj_block.grad.to_dense(), [n, n]: d score_c / d A[u, v], absent entries included
  * und_{g}, feat_{g}, labels, and the seeded state_dict (the discriminator's left out: it plays no part)
for small graphs across graph pooling {sum, average} x neighbour pooling {sum, average} x learn_eps {on, off}.  Graph 1
has an isolated node wherever the reference defines the result (not average pooling with learned eps: 0/0 there).
"""
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import make_goldens as MG  # noqa: E402  (the reference import, SynthGraph, make_batch, build_model)

# a directory of their own: helpers.golden_cases() parametrizes other tests over every tests/golden/*.npz
OUT_DIR = os.path.join(HERE, "edge")
B, N_NODES, T, L, M, F0, H, C = 2, 16, 40, 3, 2, 5, 32, 2


def leaf_adjacency(model):
    """wrap the instance's sum/average adjacency builder: the Adj_block it returns becomes a grad-requiring leaf"""
    name = "_GIN_InfoMaxReg__preprocess_neighbors_sumavepool"
    orig = getattr(model, name)
    box = []

    def wrapped(*a, **k):
        adj = orig(*a, **k).coalesce().detach().requires_grad_()
        box.append(adj)
        return adj
    setattr(model, name, wrapped)
    return box


def run_case(tag, model_seed, graph_seed, learn_eps, gpool, npool):
    iso_ok = not (npool == "average" and learn_eps)
    while True:             # average + learned eps divides by the degree (graphcnn.py:157-158): the first seed on
        graphs, raw = MG.make_batch(graph_seed, B, N_NODES, T, F0, isolate=(1, 3) if iso_ok else None, keep_pct=30.0)
        if iso_ok or all(min(len(x) for x in gr.neighbors) > 0 for gr in graphs):
            break           # from graph_seed whose graphs have no isolated node
        graph_seed += 1
    if iso_ok:
        assert len(graphs[1].neighbors[3]) == 0
    model = MG.build_model(model_seed, L, M, F0, H, C, 0.0, learn_eps, gpool, npool)
    g = torch.Generator().manual_seed(model_seed + 5)
    with torch.no_grad():   # running statistics away from their defaults, so eval-mode BatchNorm matters
        for name, b in model.named_buffers():
            if name.endswith("running_mean"):
                b.copy_(0.1 * torch.randn(b.shape, generator=g))
            elif name.endswith("running_var"):
                b.copy_(0.5 + torch.rand(b.shape, generator=g))
    out = {"cfg": np.array([L, M, F0, H, C, int(learn_eps), B, N_NODES], dtype=np.int64),
           "gpool": np.array(gpool), "npool": np.array(npool)}
    for k, v in model.state_dict().items():
        if not k.startswith("disc."):
            out["state_" + k] = v.detach().numpy().copy()
    for gi, (und, feats, label) in enumerate(raw):
        out[f"und_{gi}"] = und.astype(np.int16)
        out[f"feat_{gi}"] = feats
    out["labels"] = np.array([r[2] for r in raw], dtype=np.int64)
    box = leaf_adjacency(model)
    for gi, gr in enumerate(graphs):
        for c in range(C):
            box.clear()
            model.compute_saliency([gr], c)
            assert len(box) == 1 and box[0].grad is not None
            e = box[0].grad.to_dense().numpy().copy()
            assert e.shape == (N_NODES, N_NODES) and np.isfinite(e).all()
            out[f"edge_{gi}_{c}"] = e
        model.zero_grad()
    os.makedirs(OUT_DIR, exist_ok=True)
    path = os.path.join(OUT_DIR, f"edge_{tag}.npz")
    np.savez_compressed(path, **out)
    print(f"edge_{tag}: {os.path.getsize(path) / 1024:.0f} KB")


def main():
    seed = 0
    for gpool in ("sum", "average"):
        for npool in ("sum", "average"):
            for le in (True, False):
                run_case(f"g{gpool}_n{npool}_eps{int(le)}", 40 + seed, 5000 + 10 * seed, le, gpool, npool)
                seed += 1


if __name__ == "__main__":
    main()
