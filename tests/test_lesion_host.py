"""CPU checks of GIN_InfoMaxReg.lesion() / deletion_curve() (virtual lesions of ROI sets): the set-deleted graph builder
the GPU tests share, gnm/lesion.py (the removed sets of a deletion curve and the curve's area), the formulation
csrc/lesion.hip computes (zeroed rows, masked degree, readout over n - |D| nodes) restated in fp64 numpy against the
fp64 oracle on explicit copies, the goldens of the real reference (tests/golden/lesion/), the new C-ABI entries and
argument validation -- everything that does not need a GPU."""
import glob
import os
import re

import numpy as np
import pytest
import torch

from helpers import GOLDEN_DIR, RTOL, rel_err
from test_occlusion_host import DeletedGraph, _G, _cpu_model, delete_node

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("gnm_lesion", "gnm_lesion_pack", "gnm_lesion_scratch_floats", "gnm_lesion_mask_words")
LES_CASES = sorted(os.path.basename(f)[:-4] for f in glob.glob(os.path.join(GOLDEN_DIR, "lesion", "les_*.npz")))


def delete_nodes(graph, D):
    """`graph` without the nodes of D (indices or a bool mask), as a new S2VGraph-shaped object: test_occlusion_host's
    delete_node for a set -- the nodes, their feature rows and every edge into or out of one of them removed; the
    survivors renumbered in order; edge_mat order preserved; the other feature rows unchanged."""
    n = len(graph.g)
    D = np.asarray(D)
    rm = D.astype(bool) if D.dtype == np.bool_ else np.isin(np.arange(n), D.astype(np.int64))
    if rm.shape != (n,) or (D.dtype != np.bool_ and D.size and (D.min() < 0 or D.max() >= n)):
        raise ValueError("delete_nodes: a set outside a %d-node graph" % n)
    if rm.all():
        raise ValueError("delete_nodes: the set removes every node")
    em = graph.edge_mat
    em = em.detach().cpu().numpy() if torch.is_tensor(em) else np.asarray(em)
    em = em.astype(np.int64).reshape(2, -1)
    em = em[:, ~rm[em].any(0)]
    new = np.cumsum(~rm) - 1                                   # the new index of a kept node
    em = new[em]
    feats = graph.node_features
    feats = feats.detach().cpu() if torch.is_tensor(feats) else torch.as_tensor(np.asarray(feats))
    d = DeletedGraph()
    d.g = list(range(int((~rm).sum())))
    d.label = getattr(graph, "label", 0)
    d.node_tags = None
    d.edge_mat = torch.from_numpy(np.ascontiguousarray(em.reshape(2, -1)))
    d.node_features = feats[torch.from_numpy(~rm)].clone()
    nb = getattr(graph, "neighbors", None)
    if nb is not None:
        d.neighbors = [[int(new[u]) for u in row if not rm[u]] for j, row in enumerate(nb) if not rm[j]]
        d.max_neighbor = max((len(x) for x in d.neighbors), default=0)
    return d


def expect_nan(graph, removed, npool, learn_eps):
    """whether the reference's score of graph \\ removed is NaN: neighbour "average" with learned eps and a kept node
    none of whose neighbours (edge_mat row 0 = the row of Adj_block) is kept -- the 0/0 row"""
    if not (npool == "average" and learn_eps):
        return False
    rm = np.asarray(removed, dtype=bool)
    em = np.asarray(graph.edge_mat).astype(np.int64).reshape(2, -1)
    em = em[:, ~rm[em].any(0)]
    deg = np.bincount(em[0], minlength=rm.shape[0])
    return bool((deg[~rm] == 0).any())


def load_les_case(name):
    d = dict(np.load(os.path.join(GOLDEN_DIR, "lesion", name + ".npz")))
    L, m, f0, H, C, le, B, n = [int(x) for x in d["cfg"]]
    cfg = dict(L=L, m=m, f0=f0, H=H, C=C, learn_eps=bool(le), B=B, n=n, gpool=str(d["gpool"]), npool=str(d["npool"]))
    state = {k[len("state_"):]: v for k, v in d.items() if k.startswith("state_")}
    return cfg, state, d


def les_graphs(cfg, d):
    """(the source graphs of a golden case, S2VGraph-shaped; their removed sets, bool [S, n] each)"""
    out = []
    for g in range(cfg["B"]):
        o = _G()
        o.g = list(range(cfg["n"]))
        o.edge_mat = torch.from_numpy(d[f"em_{g}"].astype(np.int64))
        o.node_features = torch.from_numpy(d[f"feat_{g}"])
        o.label = int(d["labels"][g])
        out.append(o)
    return out, [d[f"sets_{g}"].astype(bool) for g in range(cfg["B"])]


def oracle_lesion(state, cfg_or_args, graphs, sets, dtype=np.float64):
    """(base [G, C], lesioned: per graph [S_g, C]) of the contract through oracle.gin_oracle.OracleGIN's eval forward
    on explicit set-deleted copies; cfg_or_args: a case's cfg or (L, m, learn_eps, gpool, npool)"""
    from oracle import gin_oracle as O
    a = cfg_or_args
    if isinstance(a, dict):
        a = (a["L"], a["m"], a["learn_eps"], a["gpool"], a["npool"])
    orc = O.OracleGIN(state, *a, dtype=dtype)

    def score(g):
        og = O.OGraph(len(g.g), np.asarray(g.edge_mat), np.asarray(g.node_features), getattr(g, "label", 0))
        with np.errstate(all="ignore"):
            return orc.forward([og], np.arange(1), training=False, want_disc=False)[0]
    base = np.concatenate([score(g) for g in graphs], 0)
    C = base.shape[1]
    les = [np.concatenate([score(delete_nodes(g, D)) for D in S], 0) if len(S) else np.zeros((0, C))
           for g, S in zip(graphs, sets)]
    return base, les


def masked_forward64(state, args, graph, removed):
    """What csrc/lesion.hip computes, in fp64 numpy on the SOURCE graph: the adjacency's columns of D masked, the degree
    of the masked rows, rows of D zeroed in every layer's output, the readout over n - |D| nodes.  [C] logits."""
    L, m, learn_eps, gpool, npool = args
    p = {k: np.asarray(v, dtype=np.float64) for k, v in state.items() if np.asarray(v).dtype.kind == "f"}
    n = len(graph.g)
    rm = np.asarray(removed, dtype=bool)
    keep = ~rm
    em = np.asarray(graph.edge_mat).astype(np.int64).reshape(2, -1)
    A = np.zeros((n, n))
    np.add.at(A, (em[0], em[1]), 1.0)
    Am = A * keep[None, :]
    deg = Am.sum(1) + (0 if learn_eps else 1)

    def bn(x, name):
        return (x - p[name + ".running_mean"]) / np.sqrt(p[name + ".running_var"] + 1e-5) * p[name + ".weight"] \
            + p[name + ".bias"]

    h = np.asarray(graph.node_features, dtype=np.float64)
    score = 0.0
    kept = int(keep.sum())
    scale = float(np.float32(1.0 / kept)) if gpool == "average" else 1.0
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
            h = np.where(keep[:, None], x, 0.0)                  # zeros by assignment: a removed row's NaN is dropped
            score = score + (h.sum(0) * scale) @ p[f"linears_prediction.{l}.weight"].T + p[f"linears_prediction.{l}.bias"]
    return score


# ---------------------------------------------------------------------------------------------- the builder
def test_delete_nodes_builder():
    g = _G()
    g.g = list(range(5))
    g.label = 1
    g.edge_mat = torch.tensor([[0, 1, 1, 3, 2, 4, 4], [1, 0, 2, 1, 4, 2, 3]])
    g.node_features = torch.arange(15, dtype=torch.float32).reshape(5, 3)
    g.neighbors = [[1], [0, 2], [4], [1], [2, 3]]
    for v in range(5):                                           # one node: test_occlusion_host.delete_node
        a, b = delete_nodes(g, [v]), delete_node(g, v)
        assert a.edge_mat.tolist() == b.edge_mat.tolist() and torch.equal(a.node_features, b.node_features)
        assert a.neighbors == b.neighbors and a.max_neighbor == b.max_neighbor and len(a.g) == 4
    d = delete_nodes(g, [1, 3])
    assert len(d.g) == 3 and d.edge_mat.tolist() == [[1, 2], [2, 1]]          # 2->4, 4->2 renumbered, in order
    assert torch.equal(d.node_features, g.node_features[[0, 2, 4]])
    assert d.neighbors == [[], [2], [1]] and d.max_neighbor == 1
    m = delete_nodes(g, np.array([False, True, False, True, False]))
    assert m.edge_mat.tolist() == d.edge_mat.tolist()
    e = delete_nodes(g, [])
    assert e.edge_mat.tolist() == g.edge_mat.tolist() and torch.equal(e.node_features, g.node_features)
    one = delete_nodes(g, [0, 1, 2, 3])
    assert len(one.g) == 1 and one.edge_mat.shape == (2, 0) and one.node_features.tolist() == [[12.0, 13.0, 14.0]]
    assert g.edge_mat.shape[1] == 7 and len(g.g) == 5                   # the source graph is left alone
    for bad in ([0, 1, 2, 3, 4], [5], [-1], np.ones(4, dtype=bool)):
        with pytest.raises(ValueError):
            delete_nodes(g, bad)


# ---------------------------------------------------------------------------------------------- gnm/lesion.py
def test_masks_from_ranking_orders_ties_and_cap():
    from gnm.lesion import masks_from_ranking
    r = np.array([[0.5, 2.0, 2.0, -1.0, 0.5, 3.0, 0.0, 2.0, 1.0, 0.5]])
    fr = [0.0, 0.1, 0.35, 0.5, 0.95, 1.0]
    masks, counts = masks_from_ranking(r, fr, "descending")
    assert len(masks) == 1 and masks[0].shape == (6, 10) and masks[0].dtype == np.bool_
    assert counts[0].tolist() == [0, 1, 3, 5, 9, 9]                      # floor(f n), capped at n - 1
    desc = [5, 1, 2, 7, 8, 0, 4, 9, 6, 3]                                # ties to the lower index
    for k, c in enumerate(counts[0]):
        assert sorted(np.nonzero(masks[0][k])[0].tolist()) == sorted(desc[:c])
    masks_a, counts_a = masks_from_ranking(r, fr, "ascending")
    asc = [3, 6, 0, 4, 9, 8, 1, 2, 7, 5]                                 # ties to the lower index here too
    assert counts_a[0].tolist() == counts[0].tolist()
    for k, c in enumerate(counts_a[0]):
        assert sorted(np.nonzero(masks_a[0][k])[0].tolist()) == sorted(asc[:c])
    assert not masks[0][0].any() and masks[0][-1].sum() == 9 and not masks[0][-1][3]   # all but the lowest-ranked


def test_masks_from_ranking_ragged_and_tensors():
    from gnm.lesion import masks_from_ranking
    rk = [np.arange(4.0), torch.tensor([3.0, 1.0, 2.0]), np.array([1.0, 1.0])]
    masks, counts = masks_from_ranking(rk, [0.0, 0.5, 1.0])
    assert [m.shape for m in masks] == [(3, 4), (3, 3), (3, 2)]
    assert [c.tolist() for c in counts] == [[0, 2, 3], [0, 1, 2], [0, 1, 1]]
    assert masks[0][1].tolist() == [False, False, True, True]
    assert masks[1][2].tolist() == [True, False, True]
    assert masks[2][2].tolist() == [True, False]                         # a tie: the lower index goes first
    empty, cnt = masks_from_ranking(rk, [])                              # the empty fraction list: no sets
    assert [m.shape for m in empty] == [(0, 4), (0, 3), (0, 2)] and all(c.shape == (0,) for c in cnt)


def test_masks_from_ranking_rejects():
    from gnm.lesion import masks_from_ranking
    ok = np.arange(6.0).reshape(2, 3)
    for bad in ([-0.1], [1.01], [float("nan")]):
        with pytest.raises(ValueError):
            masks_from_ranking(ok, bad)
    for val in (float("nan"), float("inf"), -float("inf")):
        r = ok.copy()
        r[1, 2] = val
        with pytest.raises(ValueError):
            masks_from_ranking(r, [0.5])
    with pytest.raises(ValueError):
        masks_from_ranking(ok, [0.5], order="random")
    with pytest.raises(ValueError):
        masks_from_ranking(np.zeros((2, 3, 4)), [0.5])
    with pytest.raises(ValueError):
        masks_from_ranking([np.zeros(0)], [0.5])


def test_curve_area_trapezoid():
    from gnm.lesion import curve_area
    s = np.array([[4.0, 2.0, 1.0, 0.5], [1.0, 1.0, 3.0, -1.0]], dtype=np.float32)
    x = np.array([0.0, 0.1, 0.5, 0.9])
    hand = [((4 + 2) / 2 * 0.1 + (2 + 1) / 2 * 0.4 + (1 + 0.5) / 2 * 0.4) / 0.9,
            ((1 + 1) / 2 * 0.1 + (1 + 3) / 2 * 0.4 + (3 - 1) / 2 * 0.4) / 0.9]
    a = curve_area(s, x)
    assert a.dtype == np.float64 and a.shape == (2,) and np.allclose(a, hand, rtol=1e-15, atol=0)
    xs = np.stack([x, np.array([0.0, 0.25, 0.25, 0.5])])                 # per-graph fractions; a repeated point adds 0
    b = curve_area(s, xs)
    assert np.isclose(b[0], hand[0], rtol=1e-15)
    assert np.isclose(b[1], ((1 + 1) / 2 * 0.25 + 0.0 + (3 - 1) / 2 * 0.25) / 0.5, rtol=1e-15)
    assert curve_area(np.array([7.0]), np.array([0.3])) == 7.0           # zero span: the single score
    assert curve_area(np.array([7.0, 9.0]), np.array([0.5, 0.5])) == 7.0
    assert curve_area(np.ones((3, 2, 4)), x).shape == (3, 2)
    assert np.isnan(curve_area(np.array([1.0, np.nan, 2.0]), np.array([0.0, 0.5, 1.0])))
    with pytest.raises(ValueError):
        curve_area(np.zeros((2, 0)), np.zeros(0))


# ---------------------------------------------------------------------------------------------- the goldens
def test_lesion_goldens_present():
    assert len(LES_CASES) == 11
    pools = {(load_les_case(c)[0]["gpool"], load_les_case(c)[0]["npool"], load_les_case(c)[0]["learn_eps"])
             for c in LES_CASES if re.match(r"les_g(sum|average)_n", c)}
    assert pools == {(g, n_, e) for g in ("sum", "average") for n_ in ("sum", "average") for e in (True, False)}
    for extra in ("les_asym_", "les_hub_", "les_onehot_"):
        assert any(c.startswith(extra) for c in LES_CASES), extra
    for f in glob.glob(os.path.join(GOLDEN_DIR, "lesion", "*.npz")):
        assert os.path.getsize(f) < 64 * 1024, f


@pytest.mark.parametrize("case", LES_CASES)
def test_golden_sets_and_nan_pattern(case):
    """5 sets per graph, the empty set and an all-but-one set among them; NaN exactly where a kept node loses every
    neighbour under average + learned eps"""
    cfg, _, d = load_les_case(case)
    graphs, sets = les_graphs(cfg, d)
    for g, (gr, S) in enumerate(zip(graphs, sets)):
        assert S.shape == (5, cfg["n"])
        sizes = S.sum(1).tolist()
        assert 0 in sizes and cfg["n"] - 1 in sizes and any(1 < k < cfg["n"] - 1 for k in sizes)
        assert np.isfinite(d[f"base_{g}"]).all()
        nan = np.isnan(d[f"lesioned_{g}"])
        want = [expect_nan(gr, D, cfg["npool"], cfg["learn_eps"]) for D in S]
        assert (nan.all(1) == want).all() and (nan.any(1) == want).all(), (g, nan, want)
    if case.startswith("les_asym_"):
        em = d["em_0"].astype(np.int64)
        assert set(map(tuple, em.T)) != set(map(tuple, em[::-1].T))
    if case.startswith("les_onehot_"):
        assert cfg["f0"] == cfg["n"] and np.array_equal(d["feat_0"], np.eye(cfg["n"], dtype=np.float32))
    if case.startswith("les_hub_"):
        assert cfg["learn_eps"] and cfg["npool"] == "average"
        S = sets[0]
        k = [i for i in range(5) if S[i].sum() == 2][0]                    # the hub and one leaf: the other leaf isolated
        assert S[k][0] and np.isnan(d["lesioned_0"][k]).all()
        assert any(np.isfinite(d["lesioned_0"][i]).all() and S[i].any() for i in range(5))


@pytest.mark.parametrize("case", LES_CASES)
def test_oracle_on_deleted_copies_reproduces_reference_goldens(case):
    """the contract (delete_nodes + the eval forward) through the fp64 oracle against the real reference's fp32 scores"""
    cfg, state, d = load_les_case(case)
    graphs, sets = les_graphs(cfg, d)
    base, les = oracle_lesion(state, cfg, graphs, sets)
    for g in range(cfg["B"]):
        scale = float(np.abs(d[f"base_{g}"]).max())
        assert rel_err(base[g], d[f"base_{g}"]) <= RTOL, (g, "base")
        assert rel_err(les[g], d[f"lesioned_{g}"], floor=scale) <= RTOL, (g, "lesioned")   # (NaN patterns equal)


# ---------------------------------------------------------------------------------------------- the formulation
@pytest.mark.parametrize("case", LES_CASES)
def test_zeroed_rows_identity(case):
    """zeroed rows + masked degree + the readout over n - |D| nodes on the SOURCE graph (what the kernel computes) is the
    forward of the explicit copy, in fp64, NaN pattern included: every pooling form, the asymmetric, hub and one-hot
    cases, the goldens' sets and further random ones"""
    cfg, state, d = load_les_case(case)
    graphs, sets = les_graphs(cfg, d)
    args = (cfg["L"], cfg["m"], cfg["learn_eps"], cfg["gpool"], cfg["npool"])
    rng = np.random.default_rng(5)
    more = [np.stack([rng.random(cfg["n"]) < f for f in (0.2, 0.5, 0.8)]) for _ in graphs]
    for S in more:
        S[:, 0] &= ~S.all(1)                                     # (never the whole graph)
    sets = [np.concatenate([a, b]) for a, b in zip(sets, more)]
    _, les = oracle_lesion(state, args, graphs, sets)
    seen_nan = False
    for g, (gr, S) in enumerate(zip(graphs, sets)):
        got = np.stack([masked_forward64(state, args, gr, D) for D in S])
        scale = float(np.abs(les[g][~np.isnan(les[g])]).max())
        assert rel_err(got, les[g], floor=scale) <= 1e-12, (g, case)
        seen_nan |= bool(np.isnan(les[g]).any())
    assert seen_nan == (cfg["npool"] == "average" and cfg["learn_eps"])   # (the all-but-one set: a lone node)


# ---------------------------------------------------------------------------------------------- the C ABI
def test_lesion_entries_declared_bound_and_exported():
    from gnm import _cabi
    header = open(os.path.join(ROOT, "include", "gnm_hip.h")).read()
    declared = set(re.findall(r"\b(gnm_[a-z0-9_]+)\s*\(", header))
    for name in NEW:
        assert name in declared and name in _cabi.SIGNATURES
        assert getattr(_cabi.lib, name) is not None
    f = _cabi.lib.gnm_lesion_scratch_floats
    # two [rows, H] activation arrays + L x V x ceil(n_max / 32) x H readout shares
    assert f(160 * 400, 160, 400, 64, 5) == 2 * 160 * 400 * 64 + 5 * 160 * 13 * 64
    assert f(33, 1, 33, 32, 1) == 2 * 33 * 32 + 2 * 32
    for bad in ((-1, 1, 1, 1, 1), (1, -1, 1, 1, 1), (1, 1, -1, 1, 1), (1, 1, 1, -1, 1), (1, 1, 1, 1, -1)):
        assert f(*bad) == 0
    from gnm import attribution
    assert attribution.LESION_SCRATCH_BYTES == 2 << 30


def test_lesion_kernels_in_the_code_object(tmp_path):
    from test_isa_hazards import disassemble
    asm = disassemble(tmp_path)
    assert re.search(r"_Z23gnm_lesion_layer_kernelILb1EEv6LsArgs", asm)            # layer 0
    assert re.search(r"_Z23gnm_lesion_layer_kernelILb0EEv6LsArgs", asm)            # layers >= 1
    assert re.search(r"gnm_lesion_finish_kernel", asm) and re.search(r"gnm_lesion_pack_kernel", asm)


def lesion_call(B=1, n_max=400, V=20, rows=8000, H=64, L=5, m=2, Cn=2, cls=(0, 1), ldo=20, ldxw=64, mstride=16,
                kept=None, vn=None, null=True, ptr=1 << 20):
    """gnm_lesion's status for a call whose checks must fail before a pointer is touched (`ptr`: a non-NULL placeholder
    the call never dereferences; null: pass NULL arrays instead)"""
    import ctypes as C
    from gnm._cabi import lib
    arr = (C.c_int * max(len(cls), 1))(*cls) if cls is not None else None
    kept = np.ascontiguousarray(np.full(max(V, 1), 7) if kept is None else kept, dtype=np.int32)
    vn = np.ascontiguousarray(np.full(max(V, 1), min(n_max, 400)) if vn is None else vn, dtype=np.int32)
    a = None if null else ptr
    return lib.gnm_lesion(a, a, a, a, a, a, mstride, a, None if null else kept.ctypes.data,
                          None if null else vn.ctypes.data, B, n_max, V, rows, a, ldxw, H, L, m, Cn, arr,
                          len(cls or ()), 0, 0, 0, 1e-5, a, None, a, a, ldo, None)


def test_lesion_bad_arguments_launch_nothing():
    """every check runs before a pointer is touched: gnm_occlusion's return codes, and the kept counts"""
    call = lesion_call
    assert call(B=0) == 0 and call(V=0) == 0                  # nothing to do
    assert call(H=36) == -2 and call(H=256) == -2
    assert call(m=4) == -2 and call(m=0) == -2 and call(L=17) == -2 and call(L=0) == -2
    assert call(n_max=417) == -2 and call(n_max=1) == -2
    assert call(cls=(2,)) == -1 and call(cls=(-1,)) == -1 and call(cls=()) == -1 and call(cls=None) == -1
    assert call(ldo=19) == -1 and call(B=-1) == -1 and call(rows=19) == -1
    assert call() == -1                                       # a covered shape with NULL arrays
    # with every array given: a leading dimension, the mask stride, and a kept count outside 1 .. n
    assert call(null=False, ldxw=63) == -1
    assert call(null=False, mstride=8) == -1 and call(null=False, mstride=24) == -1
    k = np.full(20, 7)
    for q, bad in ((0, 0), (19, 401), (5, -3)):
        kk = k.copy()
        kk[q] = bad
        assert call(null=False, kept=kk) == -1
    vn = np.full(20, 400)
    vn[3] = 6                                                 # kept 7 of a 6-node graph
    assert call(null=False, vn=vn) == -1
    import ctypes as C
    from gnm._cabi import lib
    assert lib.gnm_lesion_pack(None, 400, None, None, 1, 400, 20, 16, None, None, None) == -1
    assert lib.gnm_lesion_pack(1 << 20, 399, 1 << 20, 1 << 20, 1, 400, 20, 16, 1 << 20, 1 << 20, None) == -1
    assert lib.gnm_lesion_pack(1 << 20, 400, 1 << 20, 1 << 20, 1, 400, 20, 8, 1 << 20, 1 << 20, None) == -1
    assert lib.gnm_lesion_pack(1 << 20, 417, 1 << 20, 1 << 20, 1, 417, 20, 16, 1 << 20, 1 << 20, None) == -2
    assert lib.gnm_lesion_pack(None, 0, None, None, 0, 0, 0, 0, None, None, None) == 0


# ---------------------------------------------------------------------------------------------- the methods
def test_lesion_argument_validation():
    m, gs = _cpu_model()
    n = len(gs[0].g)
    ok = np.zeros((2, n), dtype=bool)
    ok[1, :3] = True
    one = _G()
    one.g, one.edge_mat, one.node_features = [0], torch.zeros((2, 0), dtype=torch.int64), gs[0].node_features[:1]
    small = _G()
    small.g, small.edge_mat = [0, 1, 2], torch.tensor([[0, 1, 1, 2], [1, 0, 2, 1]])
    small.node_features = gs[0].node_features[:3]
    full = ok.copy()
    full[0, :] = True
    two = ok.astype(np.int64) * 2
    bad = [dict(graphs=[], cls=0), dict(cls=2), dict(cls=-1), dict(cls=(0, 5)), dict(cls=()),
           dict(cls=0, batch_size=0),
           dict(cls=0, rois=np.zeros((2, n + 1), dtype=bool)),            # the wrong width
           dict(cls=0, rois=full),                                        # a set that removes every node
           dict(cls=0, rois=two),                                         # neither bool nor 0 / 1
           dict(cls=0, rois=np.zeros(n, dtype=bool)),                     # not [S, n]
           dict(cls=0, rois=[ok] * (len(gs) - 1)),                        # one mask per graph
           dict(cls=0, rois=[ok] * (len(gs) - 1) + [ok[:, :-1]]),
           dict(graphs=gs + [small], cls=0),                              # a shared mask over different node counts
           dict(graphs=gs + [one], cls=0, rois=[ok] * len(gs) + [np.zeros((1, 1), dtype=bool)])]
    for kw in bad:
        kw = dict(kw)
        graphs = kw.pop("graphs", gs)
        rois = kw.pop("rois", ok)
        with pytest.raises(ValueError):
            m.lesion(graphs, rois=rois, **kw)
    rk = np.zeros((len(gs), n))
    for kw in (dict(fractions=[1.5]), dict(fractions=[]), dict(order="sideways"), dict(ranking=rk[:, :-1]),
               dict(ranking=rk[:-1]), dict(ranking=np.full((len(gs), n), np.nan))):
        kw = dict(kw)
        with pytest.raises(ValueError):
            m.deletion_curve(gs, 0, kw.pop("ranking", rk), **kw)
    assert m.training                                       # validation fails before the mode changes


def test_lesion_has_no_cpu_fallback_and_restores_the_mode():
    from gnm._cabi import GnmError
    m, gs = _cpu_model()
    n = len(gs[0].g)
    for training in (True, False):
        m.train(training)
        with pytest.raises(GnmError):
            m.lesion(gs, (0, 1), np.zeros((1, n), dtype=bool))
        with pytest.raises(GnmError):
            m.deletion_curve(gs, 0, np.zeros((len(gs), n)))
        assert m.training == training
