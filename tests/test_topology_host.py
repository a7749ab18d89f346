"""The numpy oracle of the graph measures (gnm/topology.py graph_measures_host) and the host side of graph_measures,
without a GPU: the oracle against closed forms on the structured kinds and against networkx on all kinds, its
indifference to self loops and repeated edges, argument validation, and the header's declarations of what _cabi binds."""
import os
import re

import numpy as np
import pytest

from topology_cases import (GRAPH_FIELDS, INT_FIELDS, KINDS, NODE_FIELDS, STRUCTURED, check_closed_form, edges_of,
                            same_measures, synth)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("n", [1, 2, 3, 33, 65])
@pytest.mark.parametrize("kind", STRUCTURED)
def test_oracle_equals_closed_forms(kind, n):
    from gnm.topology import graph_measures_host
    m = graph_measures_host(edges_of(kind, n), n)
    for name in NODE_FIELDS:
        assert getattr(m, name).shape == (n,), name
    for name in GRAPH_FIELDS:
        assert getattr(m, name).shape == ((1, max(n, 1)) if name == "distance_histogram" else (1,)), name
    checked = check_closed_form(m, kind, n)
    assert checked >= 10 or (kind == "two_cliques" and n <= 3)
    bare = graph_measures_host(edges_of(kind, n), n, local_efficiency=False)
    assert bare.local_efficiency is None and bare.mean_local_efficiency is None
    same_measures(bare, m, (kind, n), [f for f in NODE_FIELDS + GRAPH_FIELDS if "local" not in f])


@pytest.mark.parametrize("kind,n", [(k, n) for k in KINDS for n in (33, 65)] + [("er03", 97), ("knn5", 97),
                                                                                 ("sparsity30", 97), ("path", 3)])
def test_oracle_agrees_with_networkx(kind, n):
    nx = pytest.importorskip("networkx")
    from gnm.topology import graph_measures_host
    e = edges_of(kind, n)
    m = graph_measures_host(e, n)
    G = nx.Graph()
    G.add_nodes_from(range(n))
    G.add_edges_from(e.tolist())
    tri, clu = nx.triangles(G), nx.clustering(G)
    assert m.degree.tolist() == [G.degree(v) for v in range(n)]
    assert m.triangles.tolist() == [tri[v] for v in range(n)]
    assert int(m.edges[0]) == G.number_of_edges()
    assert int(m.components[0]) == nx.number_connected_components(G)
    hist = np.zeros(n, dtype=np.int64)
    for v in range(n):
        dist = nx.single_source_shortest_path_length(G, v)
        far = [d for d in dist.values() if d > 0]
        assert int(m.eccentricity[v]) == max(far, default=0)
        assert int(m.reachable[v]) == len(far) and int(m.distance_sum[v]) == sum(far)
        assert int(m.component[v]) == min(dist)
        np.add.at(hist, far, 1)
        assert abs(m.nodal_efficiency[v] - sum(1.0 / d for d in far) / (n - 1)) <= 1e-12
        assert abs(m.clustering[v] - clu[v]) <= 1e-12
    assert m.distance_histogram[0].tolist() == hist.tolist()
    assert int(m.diameter[0]) == (int(np.flatnonzero(hist).max()) if hist.any() else 0)
    assert abs(m.transitivity[0] - nx.transitivity(G)) <= 1e-12
    assert abs(m.mean_clustering[0] - nx.average_clustering(G)) <= 1e-12
    assert abs(m.global_efficiency[0] - nx.global_efficiency(G)) <= 1e-12
    assert abs(m.mean_local_efficiency[0] - nx.local_efficiency(G)) <= 1e-12
    for v in range(n):
        assert abs(m.local_efficiency[v] - nx.global_efficiency(G.subgraph(G[v]))) <= 1e-12
    if hist.any():
        want = float((hist * np.arange(n)).sum()) / float(hist.sum())
        assert abs(m.characteristic_path_length[0] - want) <= 1e-12
        if nx.is_connected(G):
            assert abs(m.characteristic_path_length[0] - nx.average_shortest_path_length(G)) <= 1e-12
    else:
        assert np.isnan(m.characteristic_path_length[0])


@pytest.mark.parametrize("kind,n", [("er03", 33), ("two_cliques", 33), ("knn5", 65), ("empty", 3)])
def test_self_loops_and_repeated_edges_change_nothing(kind, n):
    from gnm.topology import graph_measures_host
    e = edges_of(kind, n)
    m = graph_measures_host(e, n)
    loops = np.stack([np.arange(n), np.arange(n)], 1)
    noisy = np.concatenate([e, e[::2, ::-1], loops[::3], e[:5], loops[:1]])
    same_measures(graph_measures_host(noisy, n), m, (kind, n))
    A = np.zeros((n, n), dtype=bool)
    A[e[:, 0], e[:, 1]] = True                      # one triangle only, and a diagonal
    A[np.arange(n), np.arange(n)] = True
    same_measures(graph_measures_host(A), m, (kind, n))
    same_measures(graph_measures_host(A | A.T, n), m, (kind, n))
    for name in INT_FIELDS:
        assert getattr(m, name).dtype == (np.int64 if name in ("edges", "distance_histogram") else np.int32), name


def test_oracle_arguments():
    from gnm.topology import graph_measures_host
    with pytest.raises(ValueError):
        graph_measures_host(np.array([[0, 1]]))                             # an edge list without n
    with pytest.raises(ValueError):
        graph_measures_host(np.array([[0, 5]]), 3)                          # a node outside the graph
    with pytest.raises(ValueError):
        graph_measures_host(np.zeros((3, 4), dtype=bool))
    with pytest.raises(ValueError):
        graph_measures_host(np.zeros((3, 3), dtype=np.float64), 3)


def test_graph_measures_validates_before_any_launch(monkeypatch):
    import torch
    from gnm import _cabi
    from gnm.arena import GraphArena
    from gnm.connectome import GraphMeasures, graph_measures, graph_measures_host
    from gnm.synth import SynthGraph
    from gnm import topology
    assert graph_measures is topology.graph_measures and graph_measures_host is topology.graph_measures_host
    assert GraphMeasures is topology.GraphMeasures
    launched = []
    for name in ("gnm_topology_nodes", "gnm_topology_local"):
        monkeypatch.setattr(_cabi.lib, name, lambda *a, _n=name: launched.append(_n) or 0)
    limit = int(_cabi.lib.gnm_topology_max_nodes())
    assert limit >= 1000
    ar = GraphArena("cpu")
    ok = synth(5, edges_of("ring", 5))
    # an arena that is not on a GPU: no CPU fallback
    with pytest.raises(_cabi.GnmError, match="GPU only"):
        graph_measures(ar, [ok])
    # a directed graph: edge_mat with one direction only
    directed = SynthGraph(4, np.zeros((0, 2), np.int64), np.ones((4, 1), np.float32), 0)
    directed.edge_mat = torch.tensor([[0, 1, 2], [1, 2, 3]], dtype=torch.int64)
    with pytest.raises(ValueError, match="not symmetric"):
        graph_measures(ar, [ok, directed])
    # above the limit: GnmError naming it
    big = synth(limit + 1, edges_of("path", limit + 1))
    with pytest.raises(_cabi.GnmError, match=str(limit)):
        graph_measures(ar, [ok, big])
    assert synth(limit, edges_of("path", limit)) is not None
    # an empty list gives empty arrays, whatever the arena
    for local in (True, False):
        m = graph_measures(ar, [], local_efficiency=local)
        assert len(m) == 0 and m.node_off.tolist() == [0]
        assert tuple(m.degree.shape) == (0,) and m.degree.dtype == torch.int32
        assert tuple(m.distance_histogram.shape) == (0, 0) and m.distance_histogram.dtype == torch.int64
        assert tuple(m.global_efficiency.shape) == (0,) and m.global_efficiency.dtype == torch.float64
        assert (m.local_efficiency is None) == (not local) and (m.mean_local_efficiency is None) == (not local)
    assert launched == []


def test_launchers_refuse_bad_sizes_without_a_device():
    from gnm._cabi import lib
    limit = int(lib.gnm_topology_max_nodes())
    args_nodes = [None] * 5 + [1, limit + 1] + [None] * 17
    args_local = [None] * 5 + [1, limit + 1] + [None] * 4
    assert lib.gnm_topology_nodes(*args_nodes) == -2                        # GNM_ERR_UNSUPPORTED, nothing launched
    assert lib.gnm_topology_local(*args_local) == -2
    args_nodes[6] = args_local[6] = 0
    assert lib.gnm_topology_nodes(*args_nodes) == -1 and lib.gnm_topology_local(*args_local) == -1
    args_nodes[5:7] = args_local[5:7] = [0, limit]
    assert lib.gnm_topology_nodes(*args_nodes) == 0 and lib.gnm_topology_local(*args_local) == 0      # B = 0
    assert lib.gnm_topology_workspace_bytes(4, limit, 1) >= 0 and lib.gnm_topology_workspace_bytes(4, limit + 1, 1) == -1


def test_graph_accessor_slices_by_node_off():
    from gnm.topology import GraphMeasures, graph_measures_host
    parts = [graph_measures_host(edges_of(k, n), n) for k, n in (("ring", 5), ("empty", 1), ("star", 4))]
    n_max = 5
    fields = {}
    for name in NODE_FIELDS + GRAPH_FIELDS:
        if name == "distance_histogram":
            fields[name] = np.stack([np.pad(p.distance_histogram[0], (0, n_max - p.distance_histogram.shape[1]))
                                     for p in parts])
        else:
            fields[name] = np.concatenate([getattr(p, name) for p in parts])
    m = GraphMeasures([0, 5, 6, 10], **fields)
    assert len(m) == 3
    for i, p in enumerate(parts):
        same_measures(m.graph(i), p, i)
        same_measures(m.numpy().graph(i - 3), p, i)
        assert m.graph(i).node_off.tolist() == p.node_off.tolist()
    with pytest.raises(IndexError):
        m.graph(3)


def test_header_declares_what_cabi_binds():
    from gnm import _cabi
    header = open(os.path.join(ROOT, "include", "gnm_hip.h")).read()
    body = re.sub(r"/\*.*?\*/", "", header, flags=re.S)                     # declarations only, not the comments
    declared = set(re.findall(r"\b(gnm_[a-z0-9_]+)\s*\(", body))
    new = {"gnm_topology_max_nodes", "gnm_topology_workspace_bytes", "gnm_topology_nodes", "gnm_topology_local"}
    assert new <= set(_cabi.SIGNATURES)
    for name in _cabi.SIGNATURES:
        assert name in declared, name
    # the argument counts of the new entry points, as the header writes them
    for name in new:
        m = re.search(r"\b%s\s*\(([^)]*)\)" % name, body)
        params = [p for p in m.group(1).split(",") if p.strip() and p.strip() != "void"]
        assert len(params) == len(_cabi.SIGNATURES[name][1]), name
