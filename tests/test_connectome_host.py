"""CPU checks of the connectome builder (gnm/connectome.py, csrc/connectome.hip): the host's percentile indexes against
numpy, the C entries' argument checks (nothing is launched), the order rule against the reference loader's goldens
(tests/golden/connectome, made by make_connectome_goldens.py), and the arena row order the emission kernel writes,
restated on the host, against GraphArena.add's host CSR."""
import os

import numpy as np
import pytest
import torch

import connectome_goldens

GOLDEN = connectome_goldens.PATHS
SPARSITIES = [0, 0.5, 1, 5, 30, 33.3, 50, 66.6, 70, 99, 99.99, 100, 12.345678]


def lerp(a, b, g):
    """numpy's _lerp, scalar float64"""
    d = np.float64(b) - np.float64(a)
    r = np.float64(a) + d * np.float64(g)
    if g >= 0.5:
        r = np.float64(b) - d * (np.float64(1.0) - np.float64(g))
    return r


@pytest.mark.parametrize("N", [1, 2, 4, 49, 100, 10000, 160000, 1000000])
def test_percentile_indexes_match_numpy(N):
    from gnm.connectome import percentile_indexes
    rng = np.random.default_rng(N)
    a = rng.standard_normal(min(N, 200000))
    if a.shape[0] != N:                    # the index arithmetic alone for the large N
        for sp in SPARSITIES:
            k_lo, k_hi, g = percentile_indexes(N, sp)
            vi = (N - 1) * np.true_divide(100 - sp, 100)
            assert k_lo == min(int(np.floor(vi)), N - 1) and k_hi in (k_lo, k_lo + 1)
        return
    srt = np.sort(a)
    for sp in SPARSITIES + [int(x) for x in range(0, 101, 7)]:
        k_lo, k_hi, g = percentile_indexes(N, sp)
        want = np.percentile(a, 100 - sp)
        got = lerp(srt[k_lo], srt[k_hi], g)
        assert got.tobytes() == np.float64(want).tobytes(), (N, sp, got, want)


def test_sparsity_is_validated():
    from gnm.connectome import connectivity_thresholds, percentile_indexes
    for bad in (-1, 100.5, float("nan"), "30", True, None, [30]):
        with pytest.raises(ValueError):
            percentile_indexes(16, bad)
        with pytest.raises(ValueError):
            connectivity_thresholds(np.zeros((1, 4, 4)), bad)
    assert percentile_indexes(16, np.int64(30)) == percentile_indexes(16, 30)


def test_c_entries_check_arguments_before_launching():
    from gnm._cabi import lib
    nmax = lib.gnm_connectome_max_nodes()
    assert nmax == 4096
    assert lib.gnm_connectome_workspace_words(3, 0) < 0 and lib.gnm_connectome_workspace_words(1, nmax + 1) < 0
    w = lib.gnm_connectome_workspace_words(1, 400)
    assert w % 4 == 0 and w >= 400 * 13 + 800 and lib.gnm_connectome_workspace_words(5, 400) == 5 * w
    fake = 1 << 20                                   # never dereferenced: every call below returns before a launch
    # thresholds: sizes, order-statistic indexes, gamma, pointers
    assert lib.gnm_connectome_thresholds(fake, 1, 0, 0, 0, 0.0, fake, None) == -1
    assert lib.gnm_connectome_thresholds(fake, -1, 4, 0, 0, 0.0, fake, None) == -1
    assert lib.gnm_connectome_thresholds(fake, 1, nmax + 1, 0, 0, 0.0, fake, None) == -2
    assert lib.gnm_connectome_thresholds(fake, 1, 4, 3, 2, 0.0, fake, None) == -1
    assert lib.gnm_connectome_thresholds(fake, 1, 4, 3, 5, 0.0, fake, None) == -1
    assert lib.gnm_connectome_thresholds(fake, 1, 4, 15, 16, 0.0, fake, None) == -1
    assert lib.gnm_connectome_thresholds(fake, 1, 4, -1, 0, 0.0, fake, None) == -1
    assert lib.gnm_connectome_thresholds(fake, 1, 4, 2, 3, float("nan"), fake, None) == -1
    assert lib.gnm_connectome_thresholds(fake, 1, 4, 2, 3, -0.5, fake, None) == -1
    assert lib.gnm_connectome_thresholds(None, 1, 4, 2, 3, 0.5, fake, None) == -1
    assert lib.gnm_connectome_thresholds(fake, 1, 4, 2, 3, 0.5, None, None) == -1
    assert lib.gnm_connectome_thresholds(None, 0, 4, 2, 3, 0.5, None, None) == 0          # nothing to do
    # structure / emission
    assert lib.gnm_connectome_structure(fake, 1, 0, fake, fake, fake, fake, None) == -1
    assert lib.gnm_connectome_structure(fake, 1, nmax + 1, fake, fake, fake, fake, None) == -2
    assert lib.gnm_connectome_structure(fake, 1, 8, None, fake, fake, fake, None) == -1
    assert lib.gnm_connectome_structure(fake, 1, 8, fake, fake + 4, fake, fake, None) == -1   # workspace alignment
    assert lib.gnm_connectome_structure(fake, 1, 8, fake, fake, fake, None, None) == -1
    assert lib.gnm_connectome_structure(None, 0, 8, None, None, None, None, None) == 0
    assert lib.gnm_connectome_emit(fake, 1, 0, fake, fake, fake, fake, None) == -1
    assert lib.gnm_connectome_emit(fake, 1, nmax + 1, fake, fake, fake, fake, None) == -2
    assert lib.gnm_connectome_emit(fake, 1, 8, fake, None, fake, fake, None) == -1
    assert lib.gnm_connectome_emit(fake, 1, 8, fake, fake, fake, None, None) == -1
    assert lib.gnm_connectome_emit(None, 0, 8, None, None, None, None, None) == 0


def test_no_cpu_fallback():
    from gnm._cabi import GnmError
    from gnm.arena import GraphArena
    from gnm.connectome import graphs_from_connectivity
    fc = np.eye(6)[None].repeat(2, 0)
    with pytest.raises(GnmError):
        graphs_from_connectivity(GraphArena("cpu"), fc, 30, np.zeros((6, 3), np.float32), [0, 1])
    with pytest.raises(ValueError):
        graphs_from_connectivity(GraphArena("cpu"), np.zeros((2, 6, 5)), 30, np.zeros((6, 3), np.float32), [0, 1])
    with pytest.raises(ValueError):
        graphs_from_connectivity(GraphArena("cpu"), np.zeros((1, 4097, 4097), np.float32), 30,
                                 np.zeros((4097, 1), np.float32), [0])


def golden_graphs():
    """(case, sparsity, subject, fc, edge_mat, neighbors, max_neighbor) of every golden graph"""
    for path in GOLDEN:
        d = connectome_goldens.load(path)
        for sp, s, em, nb, mx in d["graphs"]:
            yield os.path.basename(path), sp, s, d["fc"][s], em, nb, mx


def test_goldens_present():
    assert len(GOLDEN) >= 3
    assert sum(1 for _ in golden_graphs()) >= 15


def test_order_rule_reproduces_the_reference_loader():
    """the numpy restatement of load_data's graph (gnm.connectome.order_graph) on the reference's own threshold"""
    from gnm.connectome import order_graph
    for case, sp, s, fc, em, nb, mx in golden_graphs():
        n = fc.shape[0]
        thr = np.percentile(fc, 100 - sp)
        iu, ju = np.nonzero(np.triu(fc > thr, 1))
        em2, nb2, mx2 = order_graph(n, iu, ju)
        assert np.array_equal(em2, em), (case, sp, s)
        assert nb2 == nb, (case, sp, s)
        assert mx2 == mx, (case, sp, s)


def _place(m, odd, cut):
    """the emission kernel's closed form of gnm_csr_parity_order (csrc/connectome.hip ct_place)"""
    p = 4 * (m >> 1) + (2 if odd else 0) + (m & 1)
    if p < cut:
        return p
    before = 2 * (cut >> 2) + (max((cut & 3) - 2, 0) if odd else min(cut & 3, 2))
    return cut + m - before


def device_rows(n, iu, ju):
    """the CSR the emission kernel writes, restated: row x = its later-in-pi neighbours by ascending id, then its
    earlier-in-pi neighbours in pi order, each id at its ct_place position"""
    t = np.arange(n)
    np.minimum.at(t, ju, iu)
    pi = np.lexsort((np.arange(n), t))
    rank = np.empty(n, np.int64)
    rank[pi] = np.arange(n)
    adj = [set() for _ in range(n)]
    for a, b in zip(iu.tolist(), ju.tolist()):
        adj[a].add(b)
        adj[b].add(a)
    rowptr = np.zeros(n + 1, np.int32)
    cols = []
    for x in range(n):
        pre = sorted(v for v in adj[x] if rank[v] > rank[x]) + sorted((v for v in adj[x] if rank[v] < rank[x]),
                                                                       key=lambda v: rank[v])
        ne = sum(1 for v in pre if v % 2 == 0)
        cut = min(4 * (ne >> 1) + (ne & 1), 4 * ((len(pre) - ne) >> 1) + 2 + ((len(pre) - ne) & 1))
        row = [0] * len(pre)
        me = mo = 0
        for v in pre:
            if v & 1:
                row[_place(mo, True, cut)] = v
                mo += 1
            else:
                row[_place(me, False, cut)] = v
                me += 1
        cols += row
        rowptr[x + 1] = len(cols)
    return rowptr, np.asarray(cols, np.uint16)


def test_emission_order_equals_the_host_csr_of_add():
    """what GraphArena.add builds from the reference's edge_mat (gnm_csr_from_edge_mat + gnm_csr_parity_order), row
    for row, on the golden graphs and on rows of every small degree"""
    from gnm.arena import GraphArena
    cases = [(fc.shape[0], np.nonzero(np.triu(fc > np.percentile(fc, 100 - sp), 1))) for _, sp, _, fc, _, _, _ in
             golden_graphs() if fc.shape[0] <= 100]
    rng = np.random.default_rng(5)
    for n, p in ((9, 0.5), (40, 0.1), (40, 0.3), (64, 0.9), (130, 0.05)):
        A = np.triu(rng.random((n, n)) < p, 1)
        cases.append((n, np.nonzero(A)))
    from gnm.connectome import order_graph
    for n, (iu, ju) in cases:
        em, _, _ = order_graph(n, iu, ju)
        rp, col, tr = GraphArena._host_csr(n, np.ascontiguousarray(em))
        assert tr is None
        rp2, col2 = device_rows(n, iu, ju)
        assert np.array_equal(rp, rp2) and np.array_equal(col, col2), n


def test_lazy_graph_is_s2vgraph_shaped():
    from gnm.connectome import ConnectomeGraph

    class FakeArena:
        _token = object()

    g = ConnectomeGraph(FakeArena(), 3, 5, 1)
    assert len(g.g) == 5 and g.label == 1 and g.node_tags is None and g._gnm_cache[1] == 3
    g.neighbors = [[1], [0], [], [], []]
    g.max_neighbor = 1
    g.edge_mat = torch.zeros((2, 0), dtype=torch.long)
    g.node_features = torch.zeros((5, 2))
    assert g.max_neighbor == 1 and g.neighbors[0] == [1] and g.edge_mat.shape == (2, 0)
