"""Hub measures on the GPU (csrc/hubs.hip, gnm/hubs.py hub_measures).  No tolerance anywhere: every field is bitwise the
numpy oracle's (hub_measures_host), for a graph alone, inside a ragged batch at any position, and whichever route
registered it in the arena."""
import functools

import numpy as np
import pytest
import torch

from hubs_cases import (HUB_FIELDS, KINDS, MODULE_FIELDS, betweenness_closed_form, case_edges, edges_of, labels_of,
                        normalized, same_hubs, synth)
from knn_cases import bits_eq

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@functools.lru_cache(maxsize=None)
def oracle(kind, n, scheme="mod5"):
    """computed once per case, shared by the tests, never written to"""
    from gnm.hubs import hub_measures_host
    return hub_measures_host(case_edges(kind, n), n, labels=labels_of(scheme, n))


def measure(graphs, **kw):
    from gnm.arena import GraphArena
    from gnm.hubs import hub_measures
    return hub_measures(GraphArena(DEV), graphs, **kw).numpy()


def check_closed_form(h, kind, n):
    want = betweenness_closed_form(kind, n)
    if want is not None:
        assert bits_eq(h.betweenness, want), (kind, n, h.betweenness, want)
        assert bits_eq(h.betweenness_normalized, normalized(want, n)), (kind, n)
    return want is not None


# n around the word (32) and wave (64) boundaries, every kind in one batch of eleven graphs under one [n] labelling
@pytest.mark.parametrize("n", [1, 2, 3, 31, 32, 33, 63, 64, 65, 97])
def test_every_kind_is_bitwise_the_oracle(n):
    h = measure([synth(n, edges_of(kind, n)) for kind in KINDS], labels=labels_of("mod5", n))
    assert len(h) == len(KINDS) and h.node_off.tolist() == [n * i for i in range(len(KINDS) + 1)]
    closed = 0
    for i, kind in enumerate(KINDS):
        same_hubs(h.graph(i), oracle(kind, n), (kind, n))
        closed += check_closed_form(h.graph(i), kind, n)
    assert closed == 6                              # empty, complete, path, ring, star, two cliques


def test_inexact_path_counts_are_bitwise_the_oracle():
    """40 layers of three nodes: 3^39 shortest paths between the ends, above 2^53; both sides add in the same order"""
    n = 120
    same_hubs(measure([synth(n, case_edges("layered3", n))], labels=labels_of("mod5", n)).graph(0),
              oracle("layered3", n), "layered3")


# 512 / 513: the last graph of the 512-thread launch and the first of the 1024-thread one; 416 / 417 as the graph-measure
# tests have them; the project's kNN configuration at 1000 nodes
@pytest.mark.parametrize("kind,n", [("sparsity30", 400), ("knn5", 416), ("knn5", 417), ("knn5", 512), ("knn5", 513),
                                    ("knn20", 1000)])
def test_large_graphs_are_bitwise_the_oracle(kind, n):
    same_hubs(measure([synth(n, edges_of(kind, n))], labels=labels_of("mod5", n)).graph(0), oracle(kind, n), (kind, n))


def test_every_module_at_the_node_limit():
    """K = 64 label masks beside the rows of a graph of gnm_topology_max_nodes() nodes: the most LDS the kernel asks for"""
    from gnm._cabi import lib
    n = int(lib.gnm_topology_max_nodes())
    h = measure([synth(n, edges_of("knn5", n))], labels=labels_of("mod64", n), betweenness=False)
    same_hubs(h.graph(0), oracle("knn5", n, "mod64"), ("knn5", n), MODULE_FIELDS)


@pytest.mark.parametrize("n", [513, None])
def test_longest_path_against_its_closed_form(n):
    """the deepest searches: n - 1 levels from either end of the path graph, at gnm_topology_max_nodes() nodes for None"""
    from gnm._cabi import lib
    n = int(lib.gnm_topology_max_nodes()) if n is None else n
    h = measure([synth(n, edges_of("path", n))]).graph(0)
    assert check_closed_form(h, "path", n)
    assert h.betweenness[n // 2] == float((n // 2) * (n - 1 - n // 2)) and h.betweenness[0] == 0.0


def test_ragged_batch_is_bitwise_each_graph_alone_at_any_position():
    cases = [("sparsity30", 1), ("er03", 33), ("sparsity30", 400), ("knn5", 97)]
    make = lambda order: [synth(n, edges_of(kind, n)) for kind, n in (cases[i] for i in order)]
    labels = lambda order: np.concatenate([labels_of("mod5", cases[i][1]) if i is not None else labels_of("mod5", 513)
                                           for i in order])
    alone = [measure([g], labels=labels([i])).graph(0) for i, g in enumerate(make(range(4)))]
    for (kind, n), a in zip(cases, alone):
        same_hubs(a, oracle(kind, n), (kind, n))
    for order in ([0, 1, 2, 3], [2, 3, 0, 1], [3, 2, 1, 0]):
        h = measure(make(order), labels=labels(order))
        assert h.module_degree.shape == (531, 5) and h.module_edges.shape == (4, 5, 5)
        for pos, i in enumerate(order):                         # the one-node graph alone has K = 1
            same_hubs(h.graph(pos), alone[i], (order, pos), pad=True)
    # beside a graph of more than 512 nodes the small graphs run in the 1024-thread launch: the same bytes
    order = [1, 3, None, 0]
    h = measure(make([1, 3]) + [synth(513, edges_of("knn5", 513))] + make([0]), labels=labels(order))
    for pos, i in enumerate(order):
        same_hubs(h.graph(pos), oracle("knn5", 513) if i is None else alone[i], ("wide", pos), pad=True)


def test_arena_routes_give_the_same_bytes():
    from gnm.arena import GraphArena
    from gnm.connectome import graphs_from_connectivity, hub_measures, hub_measures_host
    from knn_cases import fc_stack, host_twin
    n = 65
    fc = torch.from_numpy(fc_stack(2, n, 11)).to(DEV)
    ar = GraphArena(DEV)
    built = graphs_from_connectivity(ar, fc, 30, np.ones((n, 1), np.float32), [0, 1])
    twins = [host_twin(g) for g in built]                       # the same graphs through add_many
    lab = labels_of("mod5", n)
    h = hub_measures(ar, built + twins, labels=lab).numpy()
    for w in range(2):
        em = built[w].edge_mat.numpy()
        want = hub_measures_host(em[:, :em.shape[1] // 2].T, n, labels=lab)
        for pos in (w, 2 + w):
            same_hubs(h.graph(pos), want, ("route", pos))


@pytest.mark.parametrize("kind,n", [("er03", 33), ("two_cliques", 65), ("knn5", 97)])
def test_self_loops_and_repeated_edges_in_the_csr_change_nothing(kind, n):
    from gnm.arena import GraphArena
    from gnm.hubs import hub_measures
    e = edges_of(kind, n)
    loops = np.stack([np.arange(n), np.arange(n)], 1)
    noisy = synth(n, np.concatenate([e, e[::2], loops[::3], e[:5]]))
    ar = GraphArena(DEV)
    h = hub_measures(ar, [noisy, synth(n, e)], labels=labels_of("mod5", n)).numpy()
    assert ar.nnz[noisy._gnm_cache[1]] > 2 * e.shape[0]         # the CSR holds the repeats
    same_hubs(h.graph(0), oracle(kind, n), (kind, n))
    same_hubs(h.graph(1), oracle(kind, n), (kind, n))


def test_each_half_launches_alone(monkeypatch):
    from gnm import _cabi
    calls = []
    for name in ("gnm_topology_betweenness", "gnm_topology_modules"):
        real = getattr(_cabi.lib, name)
        monkeypatch.setattr(_cabi.lib, name, lambda *a, _n=name, _f=real: calls.append(_n) or _f(*a))
    graphs = lambda: [synth(n, edges_of(kind, n)) for kind, n in (("er03", 65), ("knn5", 97))]
    lab = np.concatenate([labels_of("mod5", 65), labels_of("mod5", 97)])
    full = measure(graphs(), labels=lab)
    assert calls == ["gnm_topology_betweenness", "gnm_topology_modules"]
    del calls[:]
    bare = measure(graphs(), labels=lab, betweenness=False)
    assert calls == ["gnm_topology_modules"]
    assert bare.betweenness is None and bare.betweenness_normalized is None
    same_hubs(bare, full, "modules alone", MODULE_FIELDS)
    del calls[:]
    plain = measure(graphs())
    assert calls == ["gnm_topology_betweenness"]
    assert all(getattr(plain, name) is None for name in MODULE_FIELDS)
    same_hubs(plain, full, "betweenness alone", HUB_FIELDS[:2])


def test_dtypes_and_device_of_every_field():
    from gnm.arena import GraphArena
    from gnm.hubs import hub_measures
    n = 33
    h = hub_measures(GraphArena(DEV), [synth(n, edges_of("er03", n)) for _ in range(2)], labels=labels_of("mod5", n))
    want = {"betweenness": (torch.float64, (2 * n,)), "betweenness_normalized": (torch.float64, (2 * n,)),
            "module_degree": (torch.int32, (2 * n, 5)), "participation": (torch.float64, (2 * n,)),
            "within_module_z": (torch.float64, (2 * n,)), "module_edges": (torch.int64, (2, 5, 5)),
            "modularity": (torch.float64, (2,))}
    for name in HUB_FIELDS:
        t = getattr(h, name)
        assert t.is_cuda and t.dtype == want[name][0] and tuple(t.shape) == want[name][1], name
    assert len(h) == 2 and h.node_off.tolist() == [0, n, 2 * n]


def test_over_the_limit_raises_and_launches_nothing(monkeypatch):
    from gnm import _cabi
    from gnm.arena import GraphArena
    from gnm.hubs import hub_measures
    limit = int(_cabi.lib.gnm_topology_max_nodes())
    launched = []
    for name in ("gnm_topology_betweenness", "gnm_topology_modules"):
        monkeypatch.setattr(_cabi.lib, name, lambda *a, _n=name: launched.append(_n) or 0)
    with pytest.raises(_cabi.GnmError, match=str(limit)):
        hub_measures(GraphArena(DEV), [synth(33, edges_of("ring", 33)), synth(limit + 1, edges_of("path", limit + 1))])
    assert launched == []
