"""CPU checks of GIN_InfoMaxReg.disconnect() / disconnection_matrix() (virtual disconnection of ROI-set pairs): the
edge-cut graph builder the GPU tests share, gnm/lesion.py pair_sets / cut_edge_counts, the formulation
csrc/disconnect.hip computes (a keep mask chosen per row, the masked degree, the readout over all n nodes) restated in
fp64 numpy against the fp64 oracle on explicit copies, the goldens of the real reference (tests/golden/disconnect/), the
new C-ABI entries, argument validation and the conditioning of the GPU small-shape matrix's seeds -- everything that does
not need a GPU."""
import glob
import os
import re

import numpy as np
import pytest
import torch

from helpers import GOLDEN_DIR, RTOL, rel_err
from test_occlusion_host import DeletedGraph, _G, _cpu_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("gnm_disconnect", "gnm_disconnect_scratch_floats")
DC_CASES = sorted(os.path.basename(f)[:-4] for f in glob.glob(os.path.join(GOLDEN_DIR, "disconnect", "dc_*.npz")))
POOLS = [(np_, gp, le) for np_ in ("sum", "average") for gp in ("sum", "average") for le in (True, False)]


def _mask(S, n, what):
    S = np.asarray(S)
    m = S.astype(bool) if S.dtype == np.bool_ else np.isin(np.arange(n), S.astype(np.int64))
    if m.shape != (n,) or (S.dtype != np.bool_ and S.size and (S.min() < 0 or S.max() >= n)):
        raise ValueError("cut_edges: set %s outside a %d-node graph" % (what, n))
    return m


def _edge_mat(graph):
    em = graph.edge_mat
    em = em.detach().cpu().numpy() if torch.is_tensor(em) else np.asarray(em)
    return em.astype(np.int64).reshape(2, -1)


def cut_edges(graph, A, B):
    """`graph` without the edges between the node sets A and B (indices or bool masks), as a new S2VGraph-shaped
    object: every column (u, v) of edge_mat with (u in A and v in B) or (u in B and v in A) dropped, the column order
    preserved; the same n nodes and feature rows; neighbors / max_neighbor rebuilt under the same rule."""
    n = len(graph.g)
    a, b = _mask(A, n, "A"), _mask(B, n, "B")
    em = _edge_mat(graph)
    cut = (a[em[0]] & b[em[1]]) | (b[em[0]] & a[em[1]])
    feats = graph.node_features
    feats = feats.detach().cpu() if torch.is_tensor(feats) else torch.as_tensor(np.asarray(feats))
    d = DeletedGraph()
    d.g = list(range(n))
    d.label = getattr(graph, "label", 0)
    d.node_tags = None
    d.edge_mat = torch.from_numpy(np.ascontiguousarray(em[:, ~cut]))
    d.node_features = feats.clone()
    nb = getattr(graph, "neighbors", None)
    if nb is not None:
        d.neighbors = [[int(u) for u in row if not ((a[j] and b[u]) or (b[j] and a[u]))] for j, row in enumerate(nb)]
        d.max_neighbor = max((len(x) for x in d.neighbors), default=0)
    return d


def expect_nan_cut(graph, A, B, npool, learn_eps):
    """whether the reference's score of graph (/) (A, B) is NaN: neighbour "average" with learned eps and a node left
    without a neighbour (edge_mat row 0 = the row of Adj_block) -- the 0/0 row"""
    if not (npool == "average" and learn_eps):
        return False
    n = len(graph.g)
    deg = np.bincount(_edge_mat(cut_edges(graph, A, B))[0], minlength=n)
    return bool((deg == 0).any())


def load_dc_case(name):
    d = dict(np.load(os.path.join(GOLDEN_DIR, "disconnect", name + ".npz")))
    L, m, f0, H, C, le, B, n = [int(x) for x in d["cfg"]]
    cfg = dict(L=L, m=m, f0=f0, H=H, C=C, learn_eps=bool(le), B=B, n=n, gpool=str(d["gpool"]), npool=str(d["npool"]))
    state = {k[len("state_"):]: v for k, v in d.items() if k.startswith("state_")}
    return cfg, state, d


def dc_graphs(cfg, d):
    """(the source graphs of a golden case, S2VGraph-shaped; their set pairs: bool [S, n] A's and B's per graph)"""
    out = []
    for g in range(cfg["B"]):
        o = _G()
        o.g = list(range(cfg["n"]))
        o.edge_mat = torch.from_numpy(d[f"em_{g}"].astype(np.int64))
        o.node_features = torch.from_numpy(d[f"feat_{g}"])
        o.label = int(d["labels"][g])
        out.append(o)
    return (out, [d[f"a_{g}"].astype(bool) for g in range(cfg["B"])],
            [d[f"b_{g}"].astype(bool) for g in range(cfg["B"])])


def _args_of(a):
    return (a["L"], a["m"], a["learn_eps"], a["gpool"], a["npool"]) if isinstance(a, dict) else a


def oracle_disconnect(state, cfg_or_args, graphs, pa, pb, dtype=np.float64, group=16):
    """(base [G, C], disconnected: per graph [S_g, C]) of the contract through oracle.gin_oracle.OracleGIN's eval forward
    on explicit edge-cut copies (graphs are independent in eval mode: `group` to a forward); cfg_or_args: a case's cfg or
    (L, m, learn_eps, gpool, npool)"""
    from oracle import gin_oracle as O
    orc = O.OracleGIN(state, *_args_of(cfg_or_args), dtype=dtype)

    def scores(gs):
        out = []
        for i in range(0, len(gs), group):
            og = [O.OGraph(len(g.g), np.asarray(g.edge_mat), np.asarray(g.node_features), getattr(g, "label", 0))
                  for g in gs[i:i + group]]
            with np.errstate(all="ignore"):
                out.append(np.asarray(orc.forward(og, np.arange(len(og)), training=False, want_disc=False)[0]))
        return np.concatenate(out, 0)
    base = scores(list(graphs))
    copies = [cut_edges(g, A, B) for g, SA, SB in zip(graphs, pa, pb) for A, B in zip(SA, SB)]
    flat = scores(copies) if copies else np.zeros((0, base.shape[1]))
    starts = np.concatenate([[0], np.cumsum([len(SA) for SA in pa])])
    return base, [flat[starts[g]:starts[g + 1]] for g in range(len(graphs))]


def cut_forward64(state, args, graph, A, B):
    """What csrc/disconnect.hip computes, in fp64 numpy on the SOURCE graph: row r of the adjacency ANDed with the
    complement of B if r is in A and with the complement of A if r is in B, the degree of the masked rows, every row
    kept, the readout over all n nodes.  [C] logits."""
    L, m, learn_eps, gpool, npool = args
    p = {k: np.asarray(v, dtype=np.float64) for k, v in state.items() if np.asarray(v).dtype.kind == "f"}
    n = len(graph.g)
    a, b = np.asarray(A, dtype=bool), np.asarray(B, dtype=bool)
    KA, KB = ~a, ~b
    em = _edge_mat(graph)
    adj = np.zeros((n, n))
    np.add.at(adj, (em[0], em[1]), 1.0)
    keep = np.where(a[:, None], KB[None, :], True) & np.where(b[:, None], KA[None, :], True)     # chosen per ROW
    Am = adj * keep
    deg = Am.sum(1) + (0 if learn_eps else 1)

    def bn(x, name):
        return (x - p[name + ".running_mean"]) / np.sqrt(p[name + ".running_var"] + 1e-5) * p[name + ".weight"] \
            + p[name + ".bias"]

    h = np.asarray(graph.node_features, dtype=np.float64)
    score = 0.0
    scale = float(np.float32(1.0 / n)) if gpool == "average" else 1.0
    with np.errstate(all="ignore"):
        for l in range(L):
            pooled = Am @ h
            if not learn_eps:
                pooled = pooled + h
            if npool == "average":
                pooled = pooled / deg[:, None]
            if learn_eps:
                pooled = pooled + (1 + p["eps"][l]) * h
            x = pooled
            for k in range(m):
                wn = f"mlps.{l}.linear" if m == 1 else f"mlps.{l}.linears.{k}"
                x = x @ p[wn + ".weight"].T + p[wn + ".bias"]
                x = np.maximum(bn(x, f"batch_norms.{l}" if k == m - 1 else f"mlps.{l}.batch_norms.{k}"), 0)
            h = x
            score = score + (h.sum(0) * scale) @ p[f"linears_prediction.{l}.weight"].T + p[f"linears_prediction.{l}.bias"]
    return score


# ------------------------------------------------------------------------------ the GPU small-shape matrix's inputs
MATRIX_SHAPES = [(H, m, L) for H in (32, 64, 128) for m in (1, 2, 3) for L in (1, 3)]


def matrix_seed(H, m):
    """the model seed of the small-shape matrix (tests/test_gpu_disconnect.py), chosen for conditioning: see
    test_matrix_seeds_are_well_conditioned"""
    return 200 + H + m


def matrix_graphs():
    """tests/test_gpu_lesion.py's five graphs: n = 6, 33, 40, 40 directed, 70"""
    from test_gpu_saliency import random_graph
    return [random_graph(10, 6, 0.6, 7), random_graph(11, 33, 0.2, 7), random_graph(12, 40, 0.2, 7),
            random_graph(13, 40, 0.2, 7, directed=True), random_graph(14, 70, 0.15, 7)]


def matrix_pairs(n, seed):
    """the set pairs of the small-shape matrix for an n-node graph: (A's, B's), bool [S, n] each"""
    rng = np.random.default_rng(seed)
    idx = np.arange(n)
    none, every = np.zeros(n, dtype=bool), np.ones(n, dtype=bool)
    P = [(none, none), (idx == n // 2, every), (every, every)]                   # empty; one node isolated; edgeless
    if n > 32:
        P.append((idx < 32, (idx >= 32) & (idx < 64)))                           # row block 0 x row block 1
    for e in (7, 15, 63):                                                        # byte, half-row and word edges,
        if n > e + 2:                                                            # overlapping sets
            P.append((np.isin(idx, (e, e + 1)), np.isin(idx, (e + 1, e + 2))))
    perm = rng.permutation(n)
    t = n // 3
    P.append((np.isin(idx, perm[:t]), np.isin(idx, perm[t:2 * t])))              # two disjoint random thirds
    half = np.isin(idx, rng.choice(n, n // 2, replace=False))
    P.append((half, half))                                                       # a random half within itself
    return np.stack([a for a, _ in P]), np.stack([b for _, b in P])


def matrix_inputs():
    gs = matrix_graphs()
    prs = [matrix_pairs(len(g.g), 20 + i) for i, g in enumerate(gs)]
    return gs, [a for a, _ in prs], [b for _, b in prs]


# ---------------------------------------------------------------------------------------------- the builder
def test_cut_edges_builder():
    g = _G()
    g.g = list(range(6))
    g.label = 1
    #                        0->1  1->0  1->2  3->1  2->4  4->2  4->3  2->2  5->0  3->5
    g.edge_mat = torch.tensor([[0, 1, 1, 3, 2, 4, 4, 2, 5, 3], [1, 0, 2, 1, 4, 2, 3, 2, 0, 5]])
    g.node_features = torch.arange(18, dtype=torch.float32).reshape(6, 3)
    g.neighbors = [[1], [0, 2], [4, 2], [1, 5], [2, 3], [0]]
    d = cut_edges(g, [0, 1], [1, 2])                          # A x B and B x A: 0-1 both ways, 1->2; not 3->1
    assert d.edge_mat.tolist() == [[3, 2, 4, 4, 2, 5, 3], [1, 4, 2, 3, 2, 0, 5]]
    assert len(d.g) == 6 and torch.equal(d.node_features, g.node_features)
    assert d.neighbors == [[], [], [4, 2], [1, 5], [2, 3], [0]] and d.max_neighbor == 2
    s = cut_edges(g, [1, 2], [0, 1])                          # symmetric in (A, B)
    assert s.edge_mat.tolist() == d.edge_mat.tolist() and s.neighbors == d.neighbors
    # the explicit (2, 2) edge goes exactly when 2 is in A and in B
    assert [2, 2] in cut_edges(g, [2], [4]).edge_mat.t().tolist()
    assert [2, 2] not in cut_edges(g, [2], [2]).edge_mat.t().tolist()
    w = cut_edges(g, [2, 4], [2, 4])                          # within a set
    assert w.edge_mat.tolist() == [[0, 1, 1, 3, 4, 5, 3], [1, 0, 2, 1, 3, 0, 5]]
    one_way = cut_edges(g, [3], [1])                          # a directed edge is cut from either side
    assert [3, 1] not in one_way.edge_mat.t().tolist() and one_way.edge_mat.shape[1] == 9
    m = cut_edges(g, np.array([1, 1, 0, 0, 0, 0], dtype=bool), np.array([0, 1, 1, 0, 0, 0], dtype=bool))
    assert m.edge_mat.tolist() == d.edge_mat.tolist()
    for A, B in (([], [0, 1, 2]), ([0, 1], []), ([], [])):    # an empty set: nothing is cut
        e = cut_edges(g, A, B)
        assert e.edge_mat.tolist() == g.edge_mat.tolist() and e.neighbors == g.neighbors
    full = cut_edges(g, np.ones(6, dtype=bool), np.ones(6, dtype=bool))
    assert full.edge_mat.shape == (2, 0) and len(full.g) == 6 and full.max_neighbor == 0
    assert g.edge_mat.shape[1] == 10 and len(g.neighbors[1]) == 2        # the source graph is left alone
    for bad in ([6], [-1], np.ones(5, dtype=bool)):
        with pytest.raises(ValueError):
            cut_edges(g, bad, [0])
        with pytest.raises(ValueError):
            cut_edges(g, [0], bad)
    assert expect_nan_cut(g, [0, 1], [1, 2], "average", True)            # rows 0 and 1 are left without a neighbour
    assert not expect_nan_cut(g, [0, 1], [1, 2], "average", False) and not expect_nan_cut(g, [0, 1], [1, 2], "sum", True)
    assert not expect_nan_cut(g, [2], [2], "average", True)


# ---------------------------------------------------------------------------------------------- gnm/lesion.py
def test_pair_sets_order_and_unlabelled_nodes():
    from gnm.lesion import pair_sets
    lab = np.array([0, 2, -1, 1, 2, 0, -1])
    a, b, pairs = pair_sets(lab)
    assert pairs.tolist() == [[0, 0], [0, 1], [0, 2], [1, 1], [1, 2], [2, 2]] and pairs.dtype == np.int64
    assert a.shape == b.shape == (6, 7) and a.dtype == b.dtype == np.bool_
    for s, (p, q) in enumerate(pairs):
        assert a[s].tolist() == (lab == p).tolist() and b[s].tolist() == (lab == q).tolist()
    assert not a[:, [2, 6]].any() and not b[:, [2, 6]].any()             # label -1: in no set
    a4, b4, pairs4 = pair_sets(lab, K=4)                                  # a network without nodes here: empty sets
    assert pairs4.shape == (10, 2) and pairs4[3].tolist() == [0, 3] and not b4[3].any() and not a4[9].any()
    assert pair_sets(torch.tensor([1, 0]).numpy())[2].tolist() == [[0, 0], [0, 1], [1, 1]]
    e = pair_sets(np.full(5, -1))
    assert e[0].shape == (0, 5) and e[2].shape == (0, 2)
    for bad in (dict(labels=np.array([0, -2])), dict(labels=np.array([0, 3]), K=3), dict(labels=np.zeros((2, 2), int)),
                dict(labels=np.array([0.0, 1.0]))):
        with pytest.raises(ValueError):
            pair_sets(**bad)


def test_cut_edge_counts_against_a_loop():
    from gnm.lesion import cut_edge_counts, pair_sets
    from test_gpu_saliency import random_graph
    rng = np.random.default_rng(4)
    for gi, directed in enumerate((False, True)):
        g = random_graph(60 + gi, 23, 0.3, 3, directed=directed)
        em = _edge_mat(g)
        em = np.concatenate([em, [[5, 9], [5, 9]]], 1)                    # explicit (v, v) edges
        a, b = rng.random((7, 23)) < 0.4, rng.random((7, 23)) < 0.4
        a[0] = False                                                      # an empty set
        b[1] = True
        a[2] = b[2]                                                       # within a set
        got = cut_edge_counts(em, a, b)
        assert got.dtype == np.int64 and got.shape == (7,)
        want = [sum(1 for u, v in em.T if (a[s, u] and b[s, v]) or (b[s, u] and a[s, v])) for s in range(7)]
        assert got.tolist() == want and got[0] == 0 and got[1:].min() > 0
        assert cut_edge_counts(em, b, a).tolist() == want                 # symmetric in (a, b)
        assert cut_edge_counts(torch.as_tensor(em), a.astype(np.uint8), b.astype(np.int64)).tolist() == want
        within = cut_edge_counts(em, a, a)
        assert within.tolist() == [int((a[s, em[0]] & a[s, em[1]]).sum()) for s in range(7)]
        gx = _G()
        gx.g, gx.edge_mat, gx.node_features = list(range(23)), torch.as_tensor(em), g.node_features
        for s in range(7):                                                # what cut_edges drops
            assert em.shape[1] - cut_edges(gx, a[s], b[s]).edge_mat.shape[1] == want[s]
        lab = rng.integers(-1, 3, 23)
        pa, pb, pairs = pair_sets(lab)
        cnt = cut_edge_counts(em, pa, pb)
        every = lab >= 0                                                  # the pairs partition the labelled edges
        assert cnt.sum() == int((every[em[0]] & every[em[1]]).sum())
    with pytest.raises(ValueError):
        cut_edge_counts(em, a, b[:, :-1])
    with pytest.raises(ValueError):
        cut_edge_counts(np.array([[0], [23]]), a, b)


# ---------------------------------------------------------------------------------------------- the goldens
def test_disconnect_goldens_present():
    assert len(DC_CASES) == 11
    pools = {(load_dc_case(c)[0]["gpool"], load_dc_case(c)[0]["npool"], load_dc_case(c)[0]["learn_eps"])
             for c in DC_CASES if re.match(r"dc_g(sum|average)_n", c)}
    assert pools == {(g, n_, e) for g in ("sum", "average") for n_ in ("sum", "average") for e in (True, False)}
    for extra in ("dc_asym_", "dc_hub_", "dc_onehot_"):
        assert any(c.startswith(extra) for c in DC_CASES), extra
    for f in glob.glob(os.path.join(GOLDEN_DIR, "disconnect", "*.npz")):
        assert os.path.getsize(f) < 64 * 1024, f


@pytest.mark.parametrize("case", DC_CASES)
def test_golden_pairs_and_nan_pattern(case):
    """5 pairs per graph, the empty cut and all x all among them; NaN exactly where a node loses every neighbour under
    average + learned eps"""
    cfg, _, d = load_dc_case(case)
    graphs, pa, pb = dc_graphs(cfg, d)
    n = cfg["n"]
    for g, (gr, SA, SB) in enumerate(zip(graphs, pa, pb)):
        assert SA.shape == SB.shape == (5, n)
        assert not SA[0].any() and not SB[0].any() and SA[4].all() and SB[4].all()
        assert SA[1].sum() == 1 and not (SA[2] & SB[2]).any() and SA[2].any() and SB[2].any()
        assert np.array_equal(SA[3], SB[3]) and SA[3].sum() == n // 2
        assert np.isfinite(d[f"base_{g}"]).all()
        nan = np.isnan(d[f"disconnected_{g}"])
        want = [expect_nan_cut(gr, A, B, cfg["npool"], cfg["learn_eps"]) for A, B in zip(SA, SB)]
        assert (nan.all(1) == want).all() and (nan.any(1) == want).all(), (g, nan, want)
        assert not want[0] and want[4] == (cfg["npool"] == "average" and cfg["learn_eps"])
    if case.startswith("dc_asym_"):
        em = d["em_0"].astype(np.int64)
        assert set(map(tuple, em.T)) != set(map(tuple, em[::-1].T))
    if case.startswith("dc_onehot_"):
        assert cfg["f0"] == n and np.array_equal(d["feat_0"], np.eye(n, dtype=np.float32))
    if case.startswith("dc_hub_"):
        assert cfg["learn_eps"] and cfg["npool"] == "average"
        assert pa[0][1][0] and pb[0][1].sum() == 1 and pb[0][1][n - 2]      # the hub against one leaf: the leaf isolated
        assert np.isnan(d["disconnected_0"][1]).all()
        assert np.isfinite(d["disconnected_0"][2]).all() and np.isfinite(d["disconnected_0"][3]).all()


@pytest.mark.parametrize("case", DC_CASES)
def test_oracle_on_cut_copies_reproduces_reference_goldens(case):
    """the contract (cut_edges + the eval forward) through the fp64 oracle against the real reference's fp32 scores"""
    cfg, state, d = load_dc_case(case)
    graphs, pa, pb = dc_graphs(cfg, d)
    base, dis = oracle_disconnect(state, cfg, graphs, pa, pb)
    for g in range(cfg["B"]):
        scale = float(np.abs(d[f"base_{g}"]).max())
        assert rel_err(base[g], d[f"base_{g}"]) <= RTOL, (g, "base")
        assert rel_err(dis[g], d[f"disconnected_{g}"], floor=scale) <= RTOL, (g, "disconnected")   # (NaN patterns equal)


# ---------------------------------------------------------------------------------------------- the formulation
@pytest.mark.parametrize("case", DC_CASES)
def test_row_mask_identity(case):
    """the per-row keep mask + the masked degree + the readout over n nodes on the SOURCE graph (what the kernel
    computes) is the forward of the explicit copy, in fp64, NaN pattern included: every pooling form, the asymmetric,
    hub and one-hot cases, the goldens' pairs and further random ones with overlapping sets"""
    cfg, state, d = load_dc_case(case)
    graphs, pa, pb = dc_graphs(cfg, d)
    args = _args_of(cfg)
    rng = np.random.default_rng(5)
    n = cfg["n"]
    pa = [np.concatenate([a, rng.random((4, n)) < 0.4]) for a in pa]
    pb = [np.concatenate([b, rng.random((4, n)) < 0.4]) for b in pb]
    _, dis = oracle_disconnect(state, args, graphs, pa, pb)
    seen_nan = False
    for g, (gr, SA, SB) in enumerate(zip(graphs, pa, pb)):
        got = np.stack([cut_forward64(state, args, gr, A, B) for A, B in zip(SA, SB)])
        scale = float(np.abs(dis[g][~np.isnan(dis[g])]).max())
        assert rel_err(got, dis[g], floor=scale) <= 1e-12, (g, case)
        seen_nan |= bool(np.isnan(dis[g]).any())
    assert seen_nan == (cfg["npool"] == "average" and cfg["learn_eps"])   # (all x all: every node isolated)


def test_row_mask_identity_with_an_explicit_self_edge():
    """an explicit (v, v) edge next to the self loop of learn_eps False: cut when v is in A and in B, and only then"""
    cfg, state, d = load_dc_case([c for c in DC_CASES if c.startswith("dc_gaverage_naverage_eps0")][0])
    graphs, _, _ = dc_graphs(cfg, d)
    gr = graphs[0]
    gr.edge_mat = torch.cat([gr.edge_mat, torch.tensor([[3, 7], [3, 7]])], 1)
    n = cfg["n"]
    idx = np.arange(n)
    pa = [np.stack([idx == 3, np.isin(idx, (3, 7)), idx == 3])]
    pb = [np.stack([idx == 3, np.isin(idx, (3, 5)), idx == 7])]
    args = _args_of(cfg)
    base, dis = oracle_disconnect(state, args, [gr], pa, pb)
    got = np.stack([cut_forward64(state, args, gr, A, B) for A, B in zip(pa[0], pb[0])])
    assert rel_err(got, dis[0], floor=float(np.abs(base).max())) <= 1e-12
    assert np.abs(dis[0][0] - base[0]).max() > 1e-6                      # cutting (3, 3) alone moves the score


# ---------------------------------------------------------------------------------------------- the C ABI
def test_disconnect_entries_declared_bound_and_exported():
    from gnm import _build, _cabi, attribution
    header = open(os.path.join(ROOT, "include", "gnm_hip.h")).read()
    declared = set(re.findall(r"\b(gnm_[a-z0-9_]+)\s*\(", header))
    for name in NEW:
        assert name in declared and name in _cabi.SIGNATURES
        assert getattr(_cabi.lib, name) is not None
    assert "disconnect.hip" in _build.SOURCES
    f = _cabi.lib.gnm_disconnect_scratch_floats
    # lesion's formula: two [rows, H] activation arrays + L x V x ceil(n_max / 32) x H readout shares
    assert f(840 * 400, 840, 400, 64, 5) == 2 * 840 * 400 * 64 + 5 * 840 * 13 * 64
    for args in ((33, 1, 33, 32, 1), (160 * 400, 160, 400, 64, 5), (-1, 1, 1, 1, 1), (1, 1, 1, 1, -1)):
        assert f(*args) == _cabi.lib.gnm_lesion_scratch_floats(*args)
    assert attribution.disconnect_decline is attribution.lesion_decline


def test_disconnect_kernels_in_the_code_object(tmp_path):
    from test_isa_hazards import disassemble
    asm = disassemble(tmp_path)
    assert re.search(r"_Z27gnm_disconnect_layer_kernelILb1EEv6DcArgs", asm)        # layer 0
    assert re.search(r"_Z27gnm_disconnect_layer_kernelILb0EEv6DcArgs", asm)        # layers >= 1
    assert re.search(r"gnm_disconnect_finish_kernel", asm)
    assert re.search(r"gnm_lesion_finish_kernel", asm) and re.search(r"gnm_occlusion_finish_kernel", asm)


def disconnect_call(B=1, n_max=400, V=20, rows=8000, H=64, L=5, m=2, Cn=2, cls=(0, 1), ldo=20, ldxw=64, mstride=16,
                    vn=None, null=True, ptr=1 << 20, no_b=False):
    """gnm_disconnect's status for a call whose checks must fail before a pointer is touched (`ptr`: a non-NULL
    placeholder the call never dereferences; null: pass NULL arrays instead; no_b: only the second mask NULL)"""
    import ctypes as C
    from gnm._cabi import lib
    arr = (C.c_int * max(len(cls), 1))(*cls) if cls is not None else None
    vn = np.ascontiguousarray(np.full(max(V, 1), min(n_max, 400)) if vn is None else vn, dtype=np.int32)
    a = None if null else ptr
    return lib.gnm_disconnect(a, a, a, a, a, a, None if no_b else a, mstride, a, None if null else vn.ctypes.data, B,
                              n_max, V, rows, a, ldxw, H, L, m, Cn, arr, len(cls or ()), 0, 0, 0, 1e-5, a, None, a, a,
                              ldo, None)


def test_disconnect_bad_arguments_launch_nothing():
    """every check runs before a pointer is touched: gnm_lesion's return codes, and the node counts"""
    call = disconnect_call
    assert call(B=0) == 0 and call(V=0) == 0                  # nothing to do
    assert call(H=36) == -2 and call(H=256) == -2
    assert call(m=4) == -2 and call(m=0) == -2 and call(L=17) == -2 and call(L=0) == -2
    assert call(n_max=417) == -2 and call(n_max=1) == -2
    assert call(cls=(2,)) == -1 and call(cls=(-1,)) == -1 and call(cls=()) == -1 and call(cls=None) == -1
    assert call(ldo=19) == -1 and call(B=-1) == -1 and call(rows=19) == -1
    assert call() == -1                                       # a covered shape with NULL arrays
    # with every array given: a leading dimension, the mask stride, one mask missing, a node count outside 1 .. n_max
    assert call(null=False, ldxw=63) == -1
    assert call(null=False, mstride=8) == -1 and call(null=False, mstride=24) == -1
    assert call(null=False, no_b=True) == -1
    v = np.full(20, 400)
    for q, bad in ((0, 0), (19, 401), (5, -3)):
        vv = v.copy()
        vv[q] = bad
        assert call(null=False, vn=vv) == -1


# ---------------------------------------------------------------------------------------------- the methods
def test_disconnect_argument_validation():
    m, gs = _cpu_model()
    n = len(gs[0].g)
    ok = np.zeros((2, n), dtype=bool)
    ok[1, :3] = True
    one = _G()
    one.g, one.edge_mat, one.node_features = [0], torch.zeros((2, 0), dtype=torch.int64), gs[0].node_features[:1]
    small = _G()
    small.g, small.edge_mat = [0, 1, 2], torch.tensor([[0, 1, 1, 2], [1, 0, 2, 1]])
    small.node_features = gs[0].node_features[:3]
    two = ok.astype(np.int64) * 2
    bad = [dict(graphs=[], cls=0), dict(cls=2), dict(cls=-1), dict(cls=(0, 5)), dict(cls=()),
           dict(cls=0, batch_size=0),
           dict(cls=0, a=np.zeros((2, n + 1), dtype=bool)),               # the wrong width
           dict(cls=0, b=np.zeros((2, n + 1), dtype=bool)),
           dict(cls=0, a=two), dict(cls=0, b=two),                        # neither bool nor 0 / 1
           dict(cls=0, a=np.zeros(n, dtype=bool)),                        # not [S, n]
           dict(cls=0, b=ok[:1]),                                         # a and b of different shapes
           dict(cls=0, a=[ok] * len(gs), b=[ok] * (len(gs) - 1) + [ok[:1]]),
           dict(cls=0, a=[ok] * len(gs), b=ok),                           # a and b of different forms
           dict(cls=0, a=[ok] * (len(gs) - 1)),                           # one mask per graph
           dict(graphs=gs + [small], cls=0),                              # a shared mask over different node counts
           dict(graphs=gs + [one], cls=0, a=[ok] * len(gs) + [np.zeros((1, 1), dtype=bool)])]
    for kw in bad:
        kw = dict(kw)
        graphs = kw.pop("graphs", gs)
        a = kw.pop("a", ok)
        with pytest.raises(ValueError):
            m.disconnect(graphs, a=a, **kw)
    lab = np.zeros(n, dtype=np.int64)
    for kw in (dict(labels=lab[:-1]), dict(labels=np.full(n, -1)), dict(labels=np.full(n, -2)),
               dict(labels=lab.astype(np.float64)), dict(labels=[lab] * (len(gs) - 1)),
               dict(labels=lab, graphs=gs + [small])):
        kw = dict(kw)
        with pytest.raises(ValueError):
            m.disconnection_matrix(kw.pop("graphs", gs), 0, **kw)
    assert m.training                                       # validation fails before the mode changes


def test_disconnect_has_no_cpu_fallback_and_restores_the_mode():
    from gnm._cabi import GnmError
    m, gs = _cpu_model()
    n = len(gs[0].g)
    every = np.ones((1, n), dtype=bool)                     # (a set holding every node is taken: no ValueError first)
    for training in (True, False):
        m.train(training)
        with pytest.raises(GnmError):
            m.disconnect(gs, (0, 1), every)
        with pytest.raises(GnmError):
            m.disconnect(gs, 0, np.zeros((1, n), dtype=bool), every)
        with pytest.raises(GnmError):
            m.disconnection_matrix(gs, 0, np.arange(n) % 3)
        assert m.training == training


# ---------------------------------------------------------------------------------------------- conditioning
@pytest.mark.parametrize("H,m,L", MATRIX_SHAPES)
def test_matrix_seeds_are_well_conditioned(H, m, L):
    """The GPU small-shape matrix compares at RTOL = 1e-5 relative to a graph's max |base|; a base that is a
    cancellation of much larger terms makes ANY fp32 forward miss that (tests/test_gpu_lesion.py
    test_small_shape_matrix).  So the seeds are judged by the fp32 numpy oracle alone, never by a HIP output: for every
    model, graph and pair of the matrix it must sit within RTOL / 4 = 2.5e-6 of fp64."""
    from rowblock_midrange_cases import cpu_model
    gs, pa, pb = matrix_inputs()
    assert [a.shape[0] for a in pa] == [5, 8, 8, 8, 9]
    worst = 0.0
    for npool, gpool, le in POOLS:
        model = cpu_model(L, m, 7, H, le, gpool, npool, seed=matrix_seed(H, m))
        st = {k: v.detach().numpy().astype(np.float64) if v.dtype.is_floating_point else v.numpy()
              for k, v in model.state_dict().items()}
        st32 = {k: v.astype(np.float32) if v.dtype.kind == "f" else v for k, v in st.items()}
        args = (L, m, le, gpool, npool)
        b64, d64 = oracle_disconnect(st, args, gs, pa, pb, group=64)
        b32, d32 = oracle_disconnect(st32, args, gs, pa, pb, dtype=np.float32, group=64)
        for g in range(len(gs)):
            scale = float(np.abs(b64[g]).max())
            worst = max(worst, rel_err(b32[g], b64[g]), rel_err(d32[g], d64[g], floor=scale))
    print("fp32 oracle against fp64, H=%d m=%d L=%d: %.2e" % (H, m, L, worst))
    assert worst <= RTOL / 4
