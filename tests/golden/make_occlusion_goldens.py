#!/usr/bin/env python3
"""Generate the node-occlusion goldens (occlusion/occ_*.npz) by running the REAL reference on CPU.

Run where the reference checkout is (it never travels to the GPU machine), like make_cam_goldens.py:

    python tests/golden/make_occlusion_goldens.py

For every graph g of a case and every node v the reference's eval forward runs on an explicit node-deleted copy
(tests/test_occlusion_host.py delete_node: node v, its feature row and every edge into or out of it removed, the
surviving nodes renumbered, edge_mat order kept) and the class logits are stored, DATA ONLY:
  * em_{g}, feat_{g}     edge_mat [2, E] and node features [n, F0] of the SOURCE graph
  * base_{g}             the reference's eval forward([G_g]) c_logit, [C]
  * occluded_{g}         c_logit of forward([G_g \\ v]) for v = 0 .. n-1, [n, C]   (NaN where the reference gives NaN)
  * state_<name>         the seeded state_dict (the discriminator's left out: it plays no part)
Cases: graph pooling {sum, average} x neighbour pooling {sum, average} x learn_eps {on, off}, one asymmetric edge_mat,
one star-like graph whose hub isolates a leaf under average + learned eps (the 0/0 row), and one one-hot input.
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
from test_occlusion_host import delete_node  # noqa: E402

OUT_DIR = os.path.join(HERE, "occlusion")
B, N_NODES, T, L, M, F0, H, C = 2, 10, 40, 2, 2, 3, 32, 2


def directed(graph, seed):
    """drop one direction of about a third of the undirected edges: an asymmetric edge_mat"""
    em = graph.edge_mat.numpy()
    E = em.shape[1] // 2                        # util.py:99-100: (i, j) pairs, then (j, i) pairs
    rng = np.random.default_rng(seed)
    drop = np.zeros(2 * E, dtype=bool)
    drop[E:][rng.random(E) < 0.35] = True
    em = np.ascontiguousarray(em[:, ~drop])
    assert set(map(tuple, em.T)) != set(map(tuple, em[::-1].T)), "still symmetric; pick another seed"
    graph.edge_mat = torch.from_numpy(em)
    return graph


def hub_graph(seed, n, f0):
    """node 0 is a hub joined to everyone, nodes 1..n-3 form a ring, nodes n-2 and n-1 hang on the hub alone"""
    rng = np.random.default_rng(seed)
    und = [(0, j) for j in range(1, n)] + [(j, j + 1) for j in range(1, n - 3)] + [(1, n - 3)]
    return MG.SynthGraph(n, np.asarray(und), rng.standard_normal((n, f0)).astype(np.float32), int(rng.integers(0, 2)))


def run_case(tag, model_seed, graph_seed, learn_eps, gpool, npool, kind="corr"):
    f0 = N_NODES if kind == "onehot" else F0
    graphs = []
    for g in range(B):
        if kind == "hub":
            graphs.append(hub_graph(graph_seed + g, N_NODES, f0))
            continue
        gs = graph_seed + g
        while True:         # every node with two neighbours: no deleted copy has a 0/0 row (average + learned eps)
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
        out[f"em_{gi}"] = gr.edge_mat.numpy().astype(np.int16)
        out[f"feat_{gi}"] = gr.node_features.numpy().copy()
        with torch.no_grad():
            np.random.seed(0)
            out[f"base_{gi}"] = model([gr])[0].numpy()[0].copy()
            occ = []
            for v in range(N_NODES):
                np.random.seed(0)
                occ.append(model([delete_node(gr, v)])[0].numpy()[0].copy())
        out[f"occluded_{gi}"] = np.stack(occ)
        nan = np.isnan(out[f"occluded_{gi}"]).any(1)
        if kind == "hub":
            assert nan[0] and not nan[1:].any(), (tag, nan)     # deleting the hub, and only that, isolates the leaves
        else:
            assert not nan.any(), "%s: a deleted copy with a NaN score; pick another seed" % tag
        assert np.isfinite(out[f"base_{gi}"]).all()
    out["labels"] = np.array([g.label for g in graphs], dtype=np.int64)
    os.makedirs(OUT_DIR, exist_ok=True)
    path = os.path.join(OUT_DIR, f"occ_{tag}.npz")
    np.savez_compressed(path, **out)
    print(f"occ_{tag}: {os.path.getsize(path) / 1024:.0f} KB")


def main():
    seed = 0
    for gpool in ("sum", "average"):
        for npool in ("sum", "average"):
            for le in (True, False):
                run_case(f"g{gpool}_n{npool}_eps{int(le)}", 40 + seed, 5000 + 10 * seed, le, gpool, npool)
                seed += 1
    run_case("asym_gaverage_naverage_eps0", 60, 5200, False, "average", "average", kind="asym")
    run_case("hub_gsum_naverage_eps1", 61, 5210, True, "sum", "average", kind="hub")
    run_case("onehot_gsum_nsum_eps1", 62, 5220, True, "sum", "sum", kind="onehot")


if __name__ == "__main__":
    main()
