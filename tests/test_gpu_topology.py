"""Graph measures on the GPU (csrc/topology.hip, gnm/topology.py graph_measures).  The feature has no tolerance: every
integer field and every fp64 field is bitwise the numpy oracle's (graph_measures_host), for a graph alone, inside a
ragged batch at any position, and whichever route registered it in the arena."""
import functools

import numpy as np
import pytest
import torch

from topology_cases import (GRAPH_FIELDS, KINDS, NODE_FIELDS, check_closed_form, edges_of, same_measures, synth)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NOT_LOCAL = [f for f in NODE_FIELDS + GRAPH_FIELDS if "local" not in f]


@functools.lru_cache(maxsize=None)
def oracle(kind, n):
    """computed once per (kind, n), shared by the tests, never written to"""
    from gnm.topology import graph_measures_host
    return graph_measures_host(edges_of(kind, n), n)


def measure(graphs, **kw):
    from gnm.arena import GraphArena
    from gnm.topology import graph_measures
    m = graph_measures(GraphArena(DEV), graphs, **kw)
    assert m.degree.is_cuda and m.degree.dtype == torch.int32 and m.distance_histogram.dtype == torch.int64
    assert m.edges.dtype == torch.int64 and m.global_efficiency.dtype == torch.float64
    return m.numpy()


# n around the word (32) and wave (64) boundaries, every kind in one ragged-free batch of eleven graphs
@pytest.mark.parametrize("n", [1, 2, 31, 32, 33, 63, 64, 65, 97])
def test_every_kind_is_bitwise_the_oracle(n):
    m = measure([synth(n, edges_of(kind, n)) for kind in KINDS])
    assert len(m) == len(KINDS) and m.node_off.tolist() == [n * i for i in range(len(KINDS) + 1)]
    for i, kind in enumerate(KINDS):
        same_measures(m.graph(i), oracle(kind, n), (kind, n))
    for i, kind in enumerate(KINDS[:7]):                           # the structured kinds: closed forms as well
        check_closed_form(m.graph(i), kind, n)


# 416 / 417: the bit-matrix limit of the aggregation kernels, which these kernels do not have; 512 / 513: the last graph
# of a 16-lane group and the first of a 32-lane group; the limit itself
@pytest.mark.parametrize("kind,n", [("sparsity30", 400), ("knn5", 400), ("sparsity30", 416), ("knn5", 416),
                                    ("sparsity30", 417), ("knn5", 417), ("knn5", 512), ("knn5", 513), ("knn20", 1000),
                                    ("knn5", None)])
def test_large_graphs_are_bitwise_the_oracle(kind, n):
    from gnm._cabi import lib
    n = int(lib.gnm_topology_max_nodes()) if n is None else n
    same_measures(measure([synth(n, edges_of(kind, n))]).graph(0), oracle(kind, n), (kind, n))


def test_longest_path_against_its_closed_form():
    """the deepest search and the last histogram column: the path graph of gnm_topology_max_nodes() nodes"""
    from gnm._cabi import lib
    n = int(lib.gnm_topology_max_nodes())
    m = measure([synth(n, edges_of("path", n))]).graph(0)
    assert check_closed_form(m, "path", n) >= 10
    assert int(m.diameter[0]) == n - 1 and int(m.distance_histogram[0, n - 1]) == 2


def test_ragged_batch_is_bitwise_each_graph_alone_at_any_position():
    cases = [("sparsity30", 1), ("er03", 33), ("sparsity30", 400), ("knn5", 97)]
    make = lambda order: [synth(n, edges_of(kind, n)) for kind, n in (cases[i] for i in order)]
    alone = [measure([g]).graph(0) for g in make(range(4))]
    for (kind, n), a in zip(cases, alone):
        same_measures(a, oracle(kind, n), (kind, n))
    for order in ([0, 1, 2, 3], [2, 3, 0, 1], [3, 2, 1, 0]):
        m = measure(make(order))
        assert m.distance_histogram.shape == (4, 400)
        for pos, i in enumerate(order):
            same_measures(m.graph(pos), alone[i], (order, pos))
    # beside a graph of more than 512 nodes the small graphs run in 32-lane groups: the same bytes
    m = measure(make([1, 3]) + [synth(513, edges_of("knn5", 513))] + make([0]))
    for pos, i in enumerate([1, 3, None, 0]):
        same_measures(m.graph(pos), oracle("knn5", 513) if i is None else alone[i], ("wide", pos))


def test_arena_routes_give_the_same_bytes():
    from gnm.arena import GraphArena
    from gnm.connectome import (dynamic_connectivity_from_timeseries, dynamic_graphs_from_timeseries, graph_measures,
                                graph_measures_host, graphs_from_connectivity)
    from knn_cases import host_twin
    n, T, window, stride = 65, 90, 80, 10
    ts = np.random.default_rng(5).standard_normal((1, T, n))
    ar = GraphArena(DEV)
    dyn, windows = dynamic_graphs_from_timeseries(ar, ts, 30, [1], window, stride)
    fc = dynamic_connectivity_from_timeseries(ts, window, stride, device=DEV)[0]
    static = graphs_from_connectivity(ar, fc, 30, np.ones((n, 1), np.float32), [0] * len(dyn))
    knn = graphs_from_connectivity(ar, fc, None, np.ones((n, 1), np.float32), [0] * len(dyn), knn=5, mutual=True)
    assert len(dyn) == len(static) == 2
    twins = [host_twin(g) for g in dyn + knn]
    m = graph_measures(ar, dyn + static + twins[:2] + knn + twins[2:]).numpy()
    for w in range(2):
        em = dyn[w].edge_mat.numpy()
        want = graph_measures_host(em[:, :em.shape[1] // 2].T, n)
        for pos in (w, 2 + w, 4 + w):
            same_measures(m.graph(pos), want, ("route", pos))
        em = knn[w].edge_mat.numpy()
        want = graph_measures_host(em[:, :em.shape[1] // 2].T, n)
        for pos in (6 + w, 8 + w):
            same_measures(m.graph(pos), want, ("knn route", pos))


@pytest.mark.parametrize("kind,n", [("er03", 33), ("two_cliques", 65), ("knn5", 97)])
def test_self_loops_and_repeated_edges_in_the_csr_change_nothing(kind, n):
    from gnm.arena import GraphArena
    from gnm.topology import graph_measures
    e = edges_of(kind, n)
    loops = np.stack([np.arange(n), np.arange(n)], 1)
    noisy = synth(n, np.concatenate([e, e[::2], loops[::3], e[:5]]))
    ar = GraphArena(DEV)
    m = graph_measures(ar, [noisy, synth(n, e)]).numpy()
    gid = noisy._gnm_cache[1]
    assert ar.nnz[gid] > 2 * e.shape[0] and not ar.bits_ok[gid]     # the CSR holds the repeats; no bit matrix exists
    same_measures(m.graph(0), oracle(kind, n), (kind, n))
    same_measures(m.graph(1), oracle(kind, n), (kind, n))


def test_over_the_limit_raises_and_launches_nothing(monkeypatch):
    from gnm import _cabi
    from gnm.arena import GraphArena
    from gnm.topology import graph_measures
    limit = int(_cabi.lib.gnm_topology_max_nodes())
    launched = []
    for name in ("gnm_topology_nodes", "gnm_topology_local"):
        monkeypatch.setattr(_cabi.lib, name, lambda *a, _n=name: launched.append(_n) or 0)
    ar = GraphArena(DEV)
    with pytest.raises(_cabi.GnmError, match=str(limit)):
        graph_measures(ar, [synth(33, edges_of("ring", 33)), synth(limit + 1, edges_of("path", limit + 1))])
    assert launched == []


def test_without_local_efficiency():
    graphs = lambda: [synth(n, edges_of(kind, n)) for kind, n in (("er03", 65), ("knn5", 97), ("empty", 2))]
    full, bare = measure(graphs()), measure(graphs(), local_efficiency=False)
    assert bare.local_efficiency is None and bare.mean_local_efficiency is None
    assert full.local_efficiency is not None and full.mean_local_efficiency.shape == (3,)
    same_measures(full, bare, "flag", NOT_LOCAL)
