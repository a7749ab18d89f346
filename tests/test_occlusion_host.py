"""CPU checks of GIN_InfoMaxReg.occlusion() (per-ROI occlusion maps): the node-deleted graph builder the GPU tests
share, the contract restated through the fp64 oracle against goldens of the real reference (tests/golden/occlusion/),
the layer-0 identity csrc/occlusion.hip relies on, the new C-ABI entries, their kernels in the gfx950 code object, and
argument validation -- everything that does not need a GPU."""
import glob
import os
import re

import numpy as np
import pytest
import torch

from helpers import GOLDEN_DIR, RTOL, load_case, rel_err
from test_cabi_host import graphs_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("gnm_occlusion", "gnm_occlusion_scratch_floats")
OCC_CASES = sorted(os.path.basename(f)[:-4] for f in glob.glob(os.path.join(GOLDEN_DIR, "occlusion", "occ_*.npz")))


class DeletedGraph:
    """S2VGraph-shaped (util.py:9-17): what the reference's forward and the arena read"""


def delete_node(graph, v):
    """`graph` without node v, as a new S2VGraph-shaped object: the node, its feature row and every edge into or out of
    it (either direction of an asymmetric edge_mat) removed; the surviving nodes renumbered 0 .. n-2 in order (u -> u - 1
    for u > v); edge_mat order preserved; the other feature rows unchanged (a one-hot row keeps its width)."""
    n = len(graph.g)
    if not 0 <= v < n or n < 2:
        raise ValueError("delete_node: node %d of a %d-node graph" % (v, n))
    em = graph.edge_mat
    em = em.detach().cpu().numpy() if torch.is_tensor(em) else np.asarray(em)
    em = em.astype(np.int64).reshape(2, -1)
    em = em[:, (em != v).all(0)]
    em = em - (em > v)
    feats = graph.node_features
    feats = feats.detach().cpu() if torch.is_tensor(feats) else torch.as_tensor(np.asarray(feats))
    d = DeletedGraph()
    d.g = list(range(n - 1))
    d.label = getattr(graph, "label", 0)
    d.node_tags = None
    d.edge_mat = torch.from_numpy(np.ascontiguousarray(em))
    d.node_features = torch.cat([feats[:v], feats[v + 1:]], 0).clone()
    nb = getattr(graph, "neighbors", None)
    if nb is not None:
        d.neighbors = [[u - (u > v) for u in row if u != v] for j, row in enumerate(nb) if j != v]
        d.max_neighbor = max((len(x) for x in d.neighbors), default=0)
    return d


def load_occ_case(name):
    d = dict(np.load(os.path.join(GOLDEN_DIR, "occlusion", name + ".npz")))
    L, m, f0, H, C, le, B, n = [int(x) for x in d["cfg"]]
    cfg = dict(L=L, m=m, f0=f0, H=H, C=C, learn_eps=bool(le), B=B, n=n, gpool=str(d["gpool"]), npool=str(d["npool"]))
    state = {k[len("state_"):]: v for k, v in d.items() if k.startswith("state_")}
    return cfg, state, d


class _G:
    pass


def occ_graphs(cfg, d):
    """the source graphs of a golden case, S2VGraph-shaped"""
    out = []
    for g in range(cfg["B"]):
        o = _G()
        o.g = list(range(cfg["n"]))
        o.edge_mat = torch.from_numpy(d[f"em_{g}"].astype(np.int64))
        o.node_features = torch.from_numpy(d[f"feat_{g}"])
        o.label = int(d["labels"][g])
        out.append(o)
    return out


def oracle_scores(state, cfg_or_args, graphs, dtype=np.float64):
    """(base [G, C], occluded: per graph [n_g, C]) of the contract through oracle.gin_oracle.OracleGIN's eval forward on
    explicit node-deleted copies; cfg_or_args: a case's cfg or (L, m, learn_eps, gpool, npool)"""
    from oracle import gin_oracle as O
    a = cfg_or_args
    if isinstance(a, dict):
        a = (a["L"], a["m"], a["learn_eps"], a["gpool"], a["npool"])
    orc = O.OracleGIN(state, *a, dtype=dtype)

    def og(g):
        return O.OGraph(len(g.g), np.asarray(g.edge_mat), np.asarray(g.node_features), getattr(g, "label", 0))

    def score(gs):
        with np.errstate(all="ignore"):
            return orc.forward([og(g) for g in gs], np.arange(len(gs)), training=False, want_disc=False)[0]
    base = np.concatenate([score([g]) for g in graphs], 0)
    occluded = [np.concatenate([score([delete_node(g, v)]) for v in range(len(g.g))], 0) for g in graphs]
    return base, occluded


# ---------------------------------------------------------------------------------------------- the builder
def test_delete_node_builder():
    g = _G()
    g.g = list(range(5))
    g.label = 1
    #                         0->1  1->0  1->2  3->1  2->4  4->2  4->3      (1 -> 2 and 3 -> 1 are one-directional)
    g.edge_mat = torch.tensor([[0, 1, 1, 3, 2, 4, 4], [1, 0, 2, 1, 4, 2, 3]])
    g.node_features = torch.arange(15, dtype=torch.float32).reshape(5, 3)
    g.neighbors = [[1], [0, 2], [4], [1], [2, 3]]
    d = delete_node(g, 1)
    assert len(d.g) == 4 and d.label == 1
    assert d.edge_mat.tolist() == [[1, 3, 3], [3, 1, 2]]                 # 2->4, 4->2, 4->3 renumbered, in order
    assert torch.equal(d.node_features, g.node_features[[0, 2, 3, 4]])
    assert d.neighbors == [[], [3], [], [1, 2]] and d.max_neighbor == 2
    assert g.edge_mat.shape[1] == 7 and len(g.g) == 5                   # the source graph is left alone
    d0, d4 = delete_node(g, 0), delete_node(g, 4)
    assert d0.edge_mat.tolist() == [[0, 2, 1, 3, 3], [1, 0, 3, 1, 2]]
    assert d4.edge_mat.tolist() == [[0, 1, 1, 3], [1, 0, 2, 1]]
    eye = _G()
    eye.g, eye.edge_mat, eye.node_features = list(range(3)), torch.tensor([[0, 1], [1, 0]]), torch.eye(3)
    assert delete_node(eye, 0).node_features.tolist() == [[0, 1, 0], [0, 0, 1]]   # one-hot rows keep their width
    for bad in (-1, 5):
        with pytest.raises(ValueError):
            delete_node(g, bad)
    one = _G()
    one.g, one.edge_mat, one.node_features = [0], torch.zeros((2, 0), dtype=torch.int64), torch.ones(1, 3)
    with pytest.raises(ValueError):
        delete_node(one, 0)


# ---------------------------------------------------------------------------------------------- the goldens
def test_occlusion_goldens_present():
    assert len(OCC_CASES) == 11
    pools = {(load_occ_case(c)[0]["gpool"], load_occ_case(c)[0]["npool"], load_occ_case(c)[0]["learn_eps"])
             for c in OCC_CASES if re.match(r"occ_g(sum|average)_n", c)}
    assert pools == {(g, n_, e) for g in ("sum", "average") for n_ in ("sum", "average") for e in (True, False)}
    for extra in ("occ_asym_", "occ_hub_", "occ_onehot_"):
        assert any(c.startswith(extra) for c in OCC_CASES), extra
    for f in glob.glob(os.path.join(GOLDEN_DIR, "occlusion", "*.npz")):
        assert os.path.getsize(f) < 64 * 1024, f


@pytest.mark.parametrize("case", OCC_CASES)
def test_oracle_on_deleted_copies_reproduces_reference_goldens(case):
    """the contract (delete_node + the eval forward) through the fp64 oracle against the real reference's fp32 scores"""
    cfg, state, d = load_occ_case(case)
    graphs = occ_graphs(cfg, d)
    base, occluded = oracle_scores(state, cfg, graphs)
    for g in range(cfg["B"]):
        scale = float(np.abs(d[f"base_{g}"]).max())
        assert rel_err(base[g], d[f"base_{g}"]) <= RTOL, (g, "base")
        assert rel_err(occluded[g], d[f"occluded_{g}"], floor=scale) <= RTOL, (g, "occluded")   # (NaN patterns equal)


def test_golden_special_cases_are_what_they_claim():
    cfg, _, d = load_occ_case([c for c in OCC_CASES if c.startswith("occ_asym_")][0])
    em = d["em_0"].astype(np.int64)
    assert set(map(tuple, em.T)) != set(map(tuple, em[::-1].T))                           # asymmetric
    cfg, _, d = load_occ_case([c for c in OCC_CASES if c.startswith("occ_hub_")][0])
    assert cfg["learn_eps"] and cfg["npool"] == "average"
    for g in range(cfg["B"]):
        nan = np.isnan(d[f"occluded_{g}"])
        assert nan[0].all() and not nan[1:].any() and np.isfinite(d[f"base_{g}"]).all()   # the hub isolates a leaf
    cfg, _, d = load_occ_case([c for c in OCC_CASES if c.startswith("occ_onehot_")][0])
    assert cfg["f0"] == cfg["n"] and np.array_equal(d["feat_0"], np.eye(cfg["n"], dtype=np.float32))
    for c in OCC_CASES:
        if not c.startswith("occ_hub_"):
            cfg, _, d = load_occ_case(c)
            assert all(np.isfinite(d[f"occluded_{g}"]).all() for g in range(cfg["B"])), c


# ---------------------------------------------------------------------------------------------- layer 0
@pytest.mark.parametrize("npool", ["sum", "average"])
@pytest.mark.parametrize("learn_eps", [True, False])
def test_layer0_identity(npool, learn_eps):
    """csrc/occlusion.hip's layer 0 in numpy fp64: with XW = X W^T and S = (A + I) XW of the SOURCE graph, row r != v of
    the deleted graph's first pre-activation is (S[r] - a_rv XW[v]) [/ (deg_r + 1 - a_rv)] + b under self loops and
    (S[r] - XW[r] - a_rv XW[v]) [/ (deg_r - a_rv)] + (1 + eps) XW[r] + b under learned eps -- against the direct form
    pooled(G \\ v) W^T + b on an asymmetric graph."""
    rng = np.random.default_rng(3)
    n, F0, H, eps = 9, 5, 4, 0.3
    A = (rng.random((n, n)) < 0.5).astype(np.float64)
    A[:, :3] = 1                                              # (every row keeps a neighbour when one node goes)
    np.fill_diagonal(A, 0)
    X, W, b = rng.standard_normal((n, F0)), rng.standard_normal((H, F0)), rng.standard_normal(H)
    XW = X @ W.T
    S = (A + np.eye(n)) @ XW
    deg = A.sum(1)
    for v in range(n):
        keep = [r for r in range(n) if r != v]
        Ad, Xd = A[np.ix_(keep, keep)], X[keep]
        if learn_eps:
            pooled = Ad @ Xd
            if npool == "average":
                pooled = pooled / Ad.sum(1, keepdims=True)
            pooled = pooled + (1 + eps) * Xd
        else:
            Ad = Ad + np.eye(n - 1)
            pooled = Ad @ Xd
            if npool == "average":
                pooled = pooled / Ad.sum(1, keepdims=True)
        direct = pooled @ W.T + b
        for k, r in enumerate(keep):
            a = A[r, v]
            if learn_eps:
                t = S[r] - XW[r] - a * XW[v]
                if npool == "average":
                    t = t / (deg[r] - a)
                t = t + (1 + eps) * XW[r]
            else:
                t = S[r] - a * XW[v]
                if npool == "average":
                    t = t / (deg[r] + 1 - a)
            assert np.abs(t + b - direct[k]).max() <= 1e-12 * max(1.0, np.abs(direct).max()), (v, r)


# ---------------------------------------------------------------------------------------------- the C ABI
def test_occlusion_entries_declared_bound_and_exported():
    from gnm import _cabi
    header = open(os.path.join(ROOT, "include", "gnm_hip.h")).read()
    declared = set(re.findall(r"\b(gnm_[a-z0-9_]+)\s*\(", header))
    for name in NEW:
        assert name in declared and name in _cabi.SIGNATURES
        assert getattr(_cabi.lib, name) is not None
    # two [rows, H] activation arrays + L x V x ceil(n_max / 32) x H readout shares
    assert _cabi.lib.gnm_occlusion_scratch_floats(160000, 400, 400, 64, 5) == 2 * 160000 * 64 + 5 * 400 * 13 * 64
    # the documented default: 8 graphs of 400 nodes at hidden_dim 128 (5 layers) stay under 2 GiB
    assert 4 * _cabi.lib.gnm_occlusion_scratch_floats(8 * 160000, 8 * 400, 400, 128, 5) < 2 << 30


def test_occlusion_kernels_in_the_code_object(tmp_path):
    from test_isa_hazards import disassemble
    asm = disassemble(tmp_path)
    assert re.search(r"_Z26gnm_occlusion_layer_kernelILb1EEv6OcArgs", asm)         # layer 0
    assert re.search(r"_Z26gnm_occlusion_layer_kernelILb0EEv6OcArgs", asm)         # layers >= 1
    assert re.search(r"gnm_occlusion_finish_kernel", asm)


def test_occlusion_bad_arguments_launch_nothing():
    """every check runs before a pointer is touched: the status with NULL arrays"""
    import ctypes as C
    from gnm._cabi import lib

    def call(B=1, n_max=400, V=400, rows=160000, H=64, L=5, m=2, Cn=2, cls=(0, 1), ldo=400, ldxw=64):
        arr = (C.c_int * max(len(cls), 1))(*cls) if cls is not None else None
        return lib.gnm_occlusion(None, None, None, None, None, None, None, B, n_max, V, rows, None, ldxw, None, 64, H, L,
                                 m, Cn, arr, len(cls or ()), 0, 0, 0, 1e-5, None, None, None, None, ldo, None)
    assert call(B=0) == 0 and call(V=0) == 0                  # nothing to do
    assert call(H=36) == -2 and call(H=256) == -2
    assert call(m=4) == -2 and call(m=0) == -2 and call(L=17) == -2 and call(L=0) == -2
    assert call(n_max=417) == -2 and call(n_max=1) == -2
    assert call(cls=(2,)) == -1 and call(cls=(-1,)) == -1 and call(cls=()) == -1 and call(cls=None) == -1
    assert call(ldo=399) == -1 and call(B=-1) == -1
    assert call() == -1                                       # a covered shape with NULL arrays


# ---------------------------------------------------------------------------------------------- the method
def _cpu_model(case="tiny_s1_eps1_gsum_nsum"):
    from models.graphcnn import GIN_InfoMaxReg
    cfg, state, d = load_case(case)
    m = GIN_InfoMaxReg(cfg["L"], cfg["m"], cfg["f0"], cfg["H"], cfg["C"], 0.0, True, "sum", "sum", torch.device("cpu"))
    return m, graphs_of(cfg, d)


def test_occlusion_argument_validation():
    m, gs = _cpu_model()
    one = _G()
    one.g, one.edge_mat, one.node_features = [0], torch.zeros((2, 0), dtype=torch.int64), gs[0].node_features[:1]
    bad = [dict(graphs=[], cls=0), dict(cls=2), dict(cls=-1), dict(cls=(0, 5)), dict(cls=()),
           dict(cls=0, batch_size=0), dict(graphs=gs + [one], cls=0)]
    for kw in bad:
        kw = dict(kw)
        graphs = kw.pop("graphs", gs)
        with pytest.raises(ValueError):
            m.occlusion(graphs, **kw)
    assert m.training                                       # validation fails before the mode changes


def test_occlusion_has_no_cpu_fallback_and_restores_the_mode():
    from gnm._cabi import GnmError
    m, gs = _cpu_model()
    for training in (True, False):
        m.train(training)
        with pytest.raises(GnmError):
            m.occlusion(gs, (0, 1))
        assert m.training == training
