"""Shared by the kNN tests (tests/test_knn_host.py, tests/test_gpu_knn.py): the input kinds, an independent restatement of
the rule with Python's sorted, the hand-made rows and the comparison helpers.  No tests here."""
import numpy as np


def bits_eq(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def fc_stack(S, n, seed, kind="corr"):
    """the input kinds of tests/test_gpu_connectome.py: correlation matrices (asymmetric to the ulp) and the tie-heavy
    kind, seven values and no symmetry"""
    rng = np.random.default_rng(seed)
    if kind == "corr":
        return np.stack([np.corrcoef(rng.standard_normal((max(n, 2) + 3, n)).T).reshape(n, n) for _ in range(S)])
    if kind == "ties":
        return rng.integers(-3, 4, (S, n, n)).astype(np.float64) / 4
    raise ValueError(kind)


def ks_for(n):
    """k in {1, 2, 5, 20, n - 2, n - 1, n + 3}, clipped to valid values (k >= 1)"""
    return sorted({k for k in (1, 2, 5, 20, n - 2, n - 1, n + 3) if k >= 1})


def brute_selection(fc, k, absolute=False):
    """[n, n] bool, row i's selection: its candidates sorted with Python's sorted on (-key, column), the first k taken"""
    n = fc.shape[0]
    sel = np.zeros((n, n), dtype=bool)
    for i in range(n):
        cands = []
        for v in range(n):
            x = float(fc[i, v])
            if v == i or x != x:
                continue
            key = abs(x) if absolute else x
            cands.append((-key, v))                 # -0.0 == 0.0 in a tuple comparison: the column decides
        for _, v in sorted(cands)[:k]:
            sel[i, v] = True
    return sel


def brute_adjacency(fc, k, mutual=False, absolute=False):
    sel = brute_selection(fc, k, absolute)
    return (sel & sel.T) if mutual else (sel | sel.T)


def brute_edges(fc, k, mutual=False, absolute=False):
    return np.nonzero(np.triu(brute_adjacency(fc, k, mutual, absolute), 1))


def oracle_adjacency(fc, k, mutual=False, absolute=False):
    """the symmetric adjacency of gnm.connectome.knn_edges"""
    from gnm.connectome import knn_edges
    n = fc.shape[0]
    iu, ju = knn_edges(fc, k, mutual, absolute)
    A = np.zeros((n, n), dtype=bool)
    A[iu, ju] = True
    return A | A.T


def hand_made(n, k):
    """{name: [n, n] matrix}: rows built around the k-th place of the order.  Every matrix starts from the tie-heavy kind,
    so the rows that are not hand-made are ordinary."""
    base = fc_stack(1, n, 7000 + n, "ties")[0]
    out = {}
    m = base.copy(); m[3, :] = 0.25; m[n - 1, :] = -1.5
    out["all_equal_rows"] = m
    m = base.copy()                                 # row 2: k - 2 entries above zero, then a run of mixed zeros
    m[2, :] = -1.0
    m[2, 5:5 + k - 2] = 0.5
    m[2, 10 + k:10 + k + 12] = np.tile([0.0, -0.0, -0.0, 0.0], 3)
    out["signed_zeros"] = m
    m = base.copy(); m[4, 9] = np.inf; m[4, 11] = -np.inf; m[6, :] = -np.inf; m[6, n - 2] = np.inf; m[8, :] = np.inf
    out["infinities"] = m
    m = base.copy(); m[5, 17] = np.nan; m[5, 0] = np.nan; m[7, n - 1] = np.nan
    out["nan_inside"] = m
    m = base.copy(); m[12, :] = np.nan; m[:, 12] = np.nan
    out["nan_row_and_column"] = m
    m = base.copy(); m[20, :] = np.nan; m[20, [1, 40, n - 1]] = [0.5, -0.25, 0.5]      # three candidates, k > 3
    out["few_candidates"] = m
    rng = np.random.default_rng(n)
    m = rng.standard_normal((n, n)); m[0, 1] = 9.0; m[1, 0] = -9.0; m[2, 3] = -9.0; m[3, 2] = 9.0
    out["asymmetric"] = m
    m = 0.1 * rng.standard_normal((n, n)); m[:, :k] -= 5.0                              # strongest entries negative
    out["negative_strongest"] = m
    return out


def host_twin(g):
    """the same graph built the host way: a SynthGraph of the device graph's edge_mat and neighbours (as in
    tests/test_gpu_connectome.py)"""
    from gnm.synth import SynthGraph
    em = g.edge_mat.numpy()
    h = SynthGraph(len(g.g), em[:, :em.shape[1] // 2].T, g.node_features.numpy(), g.label)
    assert np.array_equal(h.edge_mat.numpy(), em)
    h.neighbors = [list(x) for x in g.neighbors]
    h.max_neighbor = g.max_neighbor
    return h


def arena_rows(ar, gid):
    from gnm._cabi import lib
    n, E = ar.n[gid], ar.nnz[gid]
    rp = ar.rowptr.buf[ar.rp_off[gid]:ar.rp_off[gid] + n + 1].cpu().numpy()
    col = ar.col.buf[ar.col_off[gid]:ar.col_off[gid] + E].cpu().numpy()
    w = int(lib.gnm_adj_bits_words(n))
    bits = ar.bits.buf[ar.bits_off[gid]:ar.bits_off[gid] + w].cpu().numpy() if ar.bits_ok[gid] else None
    return rp, col, bits, E, ar.iso[gid], ar.sym[gid], ar.bits_ok[gid]


def same_rows(a, b, what=None):
    for x, y in zip(a, b):
        assert (x is None and y is None) or bits_eq(np.asarray(x), np.asarray(y)), what


def same_graphs(a, b):
    assert len(a) == len(b)
    for g, h in zip(a, b):
        assert np.array_equal(g.edge_mat.numpy(), h.edge_mat.numpy())
        assert g.neighbors == h.neighbors and g.max_neighbor == h.max_neighbor and g.label == h.label
        assert bits_eq(g.node_features.numpy(), h.node_features.numpy())
