#!/usr/bin/env python3
"""Generate the set-lesion goldens (lesion/les_*.npz) by running the REAL reference on CPU.

Run where the reference checkout is (it never travels to the GPU machine), like make_occlusion_goldens.py:

    python tests/golden/make_lesion_goldens.py

For every graph g of a case and each of its 5 removed sets D the reference's eval forward runs on an explicit
set-deleted copy (tests/test_lesion_host.py delete_nodes: the nodes of D, their feature rows and every edge into or out of
one of them removed, the survivors renumbered, edge_mat order kept) and the class logits are stored, DATA ONLY:
  * em_{g}, feat_{g}     edge_mat [2, E] and node features [n, F0] of the SOURCE graph
  * sets_{g}             the removed sets, uint8 [5, n] (1 = removed): the empty set, one node, a few nodes, a random
                         half, all but one
  * base_{g}             the reference's eval forward([G_g]) c_logit, [C]
  * lesioned_{g}         c_logit of forward([G_g \\ D]) per set, [5, C]   (NaN where the reference gives NaN)
  * state_<name>         the seeded state_dict (the discriminator's left out: it plays no part)
Cases: graph pooling {sum, average} x neighbour pooling {sum, average} x learn_eps {on, off}, one asymmetric edge_mat,
one star-like graph whose hub, removed together with one leaf, isolates another leaf under average + learned eps (the
0/0 row), and one one-hot input.  Under average + learned eps the all-but-one set leaves a lone node: NaN as well.
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
from test_lesion_host import delete_nodes, expect_nan  # noqa: E402

OUT_DIR = os.path.join(HERE, "lesion")


def sets_of(kind, seed, n):
    """the 5 removed sets of a graph, bool [5, n]"""
    rng = np.random.default_rng(seed)
    S = np.zeros((5, n), dtype=bool)
    if kind == "hub":
        S[1, [0, n - 2]] = True                 # the hub and one of its leaves: the other leaf loses its only neighbour
        S[2, [n - 2]] = True                    # the leaf alone: nothing is isolated
        S[3, [1, 2, 3, n - 1]] = True           # ring nodes and the other leaf; the hub keeps everyone connected
    else:
        S[1, rng.integers(0, n)] = True
        S[2, rng.choice(n, 3, replace=False)] = True
        S[3, rng.choice(n, n // 2, replace=False)] = True
    S[4] = True
    S[4, rng.integers(0, n)] = False            # all but one
    return S


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
        S = sets_of(kind, graph_seed + 31 * gi + 7, N_NODES)
        out[f"em_{gi}"] = gr.edge_mat.numpy().astype(np.int16)
        out[f"feat_{gi}"] = gr.node_features.numpy().copy()
        out[f"sets_{gi}"] = S.astype(np.uint8)
        with torch.no_grad():
            np.random.seed(0)
            out[f"base_{gi}"] = model([gr])[0].numpy()[0].copy()
            les = []
            for D in S:
                np.random.seed(0)
                les.append(model([delete_nodes(gr, D)])[0].numpy()[0].copy())
        out[f"lesioned_{gi}"] = np.stack(les)
        nan = np.isnan(out[f"lesioned_{gi}"])
        want = np.array([expect_nan(gr, D, npool, learn_eps) for D in S])
        assert (nan.all(1) == want).all() and (nan.any(1) == want).all(), (tag, nan, want)
        if kind == "hub":
            assert want.tolist() == [False, True, False, False, True], (tag, want)
        assert np.isfinite(out[f"base_{gi}"]).all()
    out["labels"] = np.array([g.label for g in graphs], dtype=np.int64)
    os.makedirs(OUT_DIR, exist_ok=True)
    path = os.path.join(OUT_DIR, f"les_{tag}.npz")
    np.savez_compressed(path, **out)
    print(f"les_{tag}: {os.path.getsize(path) / 1024:.0f} KB")


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
