"""The numpy oracle of the hub measures (gnm/hubs.py hub_measures_host) and the host side of hub_measures, without a
GPU: betweenness against closed forms (bitwise) and networkx (1e-12 of the largest entry), the module measures against
networkx's modularity and a numpy restatement of the BCT formulas, label handling, argument validation, and the header's
declarations of the new entry points."""
import os
import re

import numpy as np
import pytest

from hubs_cases import (DTYPES, HUB_FIELDS, KINDS, MODULE_FIELDS, bct_module_z, bct_participation,
                        betweenness_closed_form, case_edges, edges_of, labels_of, normalized, same_hubs, synth)
from knn_cases import bits_eq

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def nx_graph(nx, e, n):
    G = nx.Graph()
    G.add_nodes_from(range(n))
    G.add_edges_from(e.tolist())
    return G


def adjacency(e, n):
    A = np.zeros((n, n), dtype=np.int64)
    A[e[:, 0], e[:, 1]] = 1
    A[e[:, 1], e[:, 0]] = 1
    return A


@pytest.mark.parametrize("n", [1, 2, 3, 33, 64, 65])
@pytest.mark.parametrize("kind", ["path", "star", "ring", "complete", "two_cliques", "empty"])
def test_betweenness_equals_closed_forms_bitwise(kind, n):
    from gnm.hubs import hub_measures_host
    h = hub_measures_host(edges_of(kind, n), n)
    want = betweenness_closed_form(kind, n)
    assert bits_eq(h.betweenness, want), (kind, n, h.betweenness, want)
    assert bits_eq(h.betweenness_normalized, normalized(want, n)), (kind, n)
    for name in MODULE_FIELDS:
        assert getattr(h, name) is None, name
    assert len(h) == 1 and h.node_off.tolist() == [0, n]


def test_two_cliques_joined_by_an_edge():
    """the bridge ends carry every path between the rest of their clique and the other side: (c - 1) c for cliques of c
    nodes; nobody else is between anything"""
    from gnm.hubs import hub_measures_host
    for c in (2, 5, 16):
        bc = hub_measures_host(edges_of("two_cliques", 2 * c), 2 * c).betweenness
        want = np.zeros(2 * c)
        want[[c - 1, c]] = (c - 1) * c
        assert bits_eq(bc, want), (c, bc)


@pytest.mark.parametrize("kind,n", [(k, 97) for k in KINDS] + [("layered3", 120)])
def test_betweenness_agrees_with_networkx(kind, n):
    nx = pytest.importorskip("networkx")
    from gnm.hubs import hub_measures_host
    e = case_edges(kind, n)
    h = hub_measures_host(e, n)
    G = nx_graph(nx, e, n)
    for norm, got in ((False, h.betweenness), (True, h.betweenness_normalized)):
        ref = nx.betweenness_centrality(G, normalized=norm)
        ref = np.array([ref[v] for v in range(n)])
        print(kind, n, norm, "largest difference", float(np.abs(got - ref).max()), "largest entry", float(ref.max()))
        assert np.abs(got - ref).max() <= 1e-12 * ref.max(), (kind, n, norm)


@pytest.mark.parametrize("scheme", ["mod7", "blocks7"])
@pytest.mark.parametrize("kind", KINDS)
def test_module_measures_agree_with_networkx_and_the_bct_formulas(kind, scheme):
    nx = pytest.importorskip("networkx")
    from gnm.hubs import hub_measures_host
    n, K = 97, 7
    e, lab = edges_of(kind, n), labels_of(scheme, n)
    h = hub_measures_host(e, n, labels=lab)
    A = adjacency(e, n)
    assert h.module_degree.shape == (n, K) and h.module_edges.shape == (1, K, K)
    # the integer fields: no node is background, so a node's module degrees add up to its degree
    assert h.module_degree.sum(1).tolist() == A.sum(1).tolist()
    me = h.module_edges[0]
    assert (me == me.T).all() and int(np.trace(me) + np.triu(me, 1).sum()) == e.shape[0]
    for a in range(K):
        for b in range(K):
            between = int(A[np.ix_(lab == a, lab == b)].sum())
            assert int(me[a, b]) == (between // 2 if a == b else between)
    assert np.abs(h.participation - bct_participation(A, lab, K)).max() <= 1e-12
    assert np.abs(h.within_module_z - bct_module_z(A, lab, K)).max() <= 1e-12
    if e.shape[0]:
        q = nx.community.modularity(nx_graph(nx, e, n), [set(np.flatnonzero(lab == m).tolist()) for m in range(K)])
        assert abs(h.modularity[0] - q) <= 1e-12
    else:
        assert h.modularity[0] == 0.0 and not h.participation.any() and not h.within_module_z.any()


def test_labels_background_small_modules_and_module_counts():
    from gnm.hubs import hub_measures_host
    n = 33
    e = edges_of("er03", n)
    A = adjacency(e, n)
    full = hub_measures_host(e, n, labels=np.arange(n) % 5)
    lab = labels_of("mod5", n)                                  # node 0 in no module
    h = hub_measures_host(e, n, labels=lab)
    assert h.within_module_z[0] == 0.0
    assert (h.module_degree[:, 1:] == full.module_degree[:, 1:]).all()
    assert (h.module_degree[:, 0] == full.module_degree[:, 0] - A[:, 0]).all()
    assert (h.module_degree.sum(1) == A.sum(1) - A[:, 0]).all()
    assert int(np.trace(h.module_edges[0]) + np.triu(h.module_edges[0], 1).sum()) == e.shape[0] - int(A[0].sum())
    # a module of one node: z = 0.0; a module without nodes (label 2 is never used): an empty row and column
    lab = np.zeros(n, dtype=np.int64)
    lab[5] = 1
    lab[6] = 3
    h = hub_measures_host(e, n, labels=lab)
    assert h.module_degree.shape == (n, 4) and not h.module_degree[:, 2].any()
    assert h.within_module_z[5] == 0.0 and h.within_module_z[6] == 0.0
    assert not h.module_edges[0, 2].any() and not h.module_edges[0, :, 2].any()
    # K = 1: every edge is inside the one module, Q = 1 - 1 = 0, participation 0
    h = hub_measures_host(e, n, labels=np.zeros(n, dtype=np.int64))
    assert h.module_edges.tolist() == [[[e.shape[0]]]] and h.modularity[0] == 0.0 and not h.participation.any()
    assert np.abs(h.within_module_z - bct_module_z(A, np.zeros(n, dtype=np.int64), 1)).max() <= 1e-12
    # K = 64 is the most; 65 is refused
    n = 70
    e = edges_of("er03", n)
    h = hub_measures_host(e, n, labels=labels_of("mod64", n))
    assert h.module_degree.shape == (n, 64) and h.module_degree.sum(1).tolist() == adjacency(e, n).sum(1).tolist()
    with pytest.raises(ValueError, match="64"):
        hub_measures_host(e, n, labels=np.arange(n) % 65)
    for bad in (np.full(n, -2), np.zeros(n - 1, dtype=np.int64), np.zeros(n), np.zeros((n, 1), dtype=np.int64)):
        with pytest.raises(ValueError):
            hub_measures_host(e, n, labels=bad)
    for name in HUB_FIELDS:
        assert getattr(h, name).dtype == DTYPES[name], name


@pytest.mark.parametrize("kind,n", [("er03", 33), ("two_cliques", 33), ("knn5", 65), ("empty", 3)])
def test_self_loops_and_repeated_edges_change_nothing(kind, n):
    from gnm.hubs import hub_measures_host
    e, lab = edges_of(kind, n), labels_of("mod5", n)
    h = hub_measures_host(e, n, labels=lab)
    loops = np.stack([np.arange(n), np.arange(n)], 1)
    noisy = np.concatenate([e, e[::2, ::-1], loops[::3], e[:5], loops[:1]])
    same_hubs(hub_measures_host(noisy, n, labels=lab), h, (kind, n))
    A = np.zeros((n, n), dtype=bool)
    A[e[:, 0], e[:, 1]] = True
    A[np.arange(n), np.arange(n)] = True
    same_hubs(hub_measures_host(A, labels=lab), h, (kind, n))


def test_hub_measures_validates_before_any_launch(monkeypatch):
    import torch
    from gnm import _cabi, hubs
    from gnm.arena import GraphArena
    from gnm.connectome import HubMeasures, hub_measures, hub_measures_host
    from gnm.synth import SynthGraph
    assert hub_measures is hubs.hub_measures and hub_measures_host is hubs.hub_measures_host
    assert HubMeasures is hubs.HubMeasures
    launched = []
    for name in ("gnm_topology_betweenness", "gnm_topology_modules"):
        monkeypatch.setattr(_cabi.lib, name, lambda *a, _n=name: launched.append(_n) or 0)
    limit = int(_cabi.lib.gnm_topology_max_nodes())
    assert limit >= 1000 and int(_cabi.lib.gnm_topology_max_modules()) == 64
    ar = GraphArena("cpu")
    ok = lambda: synth(5, edges_of("ring", 5))
    with pytest.raises(_cabi.GnmError, match="GPU only"):                  # no CPU fallback
        hub_measures(ar, [ok()])
    with pytest.raises(_cabi.GnmError, match="GPU only"):
        hub_measures(ar, [ok(), ok()], labels=np.arange(5) % 2)
    directed = SynthGraph(4, np.zeros((0, 2), np.int64), np.ones((4, 1), np.float32), 0)
    directed.edge_mat = torch.tensor([[0, 1, 2], [1, 2, 3]], dtype=torch.int64)
    with pytest.raises(ValueError, match="not symmetric"):
        hub_measures(ar, [ok(), directed])
    with pytest.raises(_cabi.GnmError, match=str(limit)):
        hub_measures(ar, [ok(), synth(limit + 1, edges_of("path", limit + 1))])
    # an [n] label vector beside a ragged batch, a wrong length, too many modules, a label below -1
    ragged = lambda: [ok(), synth(7, edges_of("ring", 7))]
    with pytest.raises(ValueError, match="labels"):
        hub_measures(ar, ragged(), labels=np.arange(5) % 2)
    with pytest.raises(ValueError, match="labels"):
        hub_measures(ar, [ok(), ok()], labels=np.arange(7) % 2)
    with pytest.raises(ValueError, match="64"):
        hub_measures(ar, [synth(70, edges_of("ring", 70))], labels=np.arange(70) % 65)
    with pytest.raises(ValueError):
        hub_measures(ar, [ok()], labels=np.full(5, -2))
    with pytest.raises(_cabi.GnmError, match="GPU only"):                  # [N] labels in batch order are taken
        hub_measures(ar, ragged(), labels=np.arange(12) % 3)
    # an empty list gives empty arrays, whatever the arena
    h = hub_measures(ar, [], labels=np.arange(5) % 3)
    assert len(h) == 0 and h.node_off.tolist() == [0]
    assert tuple(h.betweenness.shape) == (0,) and h.betweenness.dtype == torch.float64
    assert tuple(h.module_degree.shape) == (0, 3) and h.module_degree.dtype == torch.int32
    assert tuple(h.module_edges.shape) == (0, 3, 3) and h.module_edges.dtype == torch.int64
    h = hub_measures(ar, [], betweenness=False)
    assert all(getattr(h, name) is None for name in HUB_FIELDS)
    assert launched == []


def test_launchers_refuse_bad_sizes_without_a_device():
    from gnm._cabi import lib
    limit = int(lib.gnm_topology_max_nodes())
    bet = [None] * 5 + [1, limit + 1] + [None] * 4
    mod = [None] * 6 + [1, limit + 1, 5] + [None] * 6
    assert lib.gnm_topology_betweenness(*bet) == -2 and lib.gnm_topology_modules(*mod) == -2    # GNM_ERR_UNSUPPORTED
    bet[6] = mod[7] = 0
    assert lib.gnm_topology_betweenness(*bet) == -1 and lib.gnm_topology_modules(*mod) == -1
    mod[7:9] = [limit, 65]
    assert lib.gnm_topology_modules(*mod) == -2
    mod[8] = 0
    assert lib.gnm_topology_modules(*mod) == -1
    bet[5:7] = [0, limit]
    mod[6:9] = [0, limit, 64]
    assert lib.gnm_topology_betweenness(*bet) == 0 and lib.gnm_topology_modules(*mod) == 0      # B = 0
    assert lib.gnm_topology_betweenness_workspace_bytes(4, limit) == 0
    assert lib.gnm_topology_betweenness_workspace_bytes(4, limit + 1) == -1


def test_graph_accessor_slices_by_node_off():
    from gnm.hubs import HubMeasures, hub_measures_host
    cases = (("ring", 5), ("path", 3), ("star", 4))
    parts = [hub_measures_host(edges_of(k, n), n, labels=np.arange(n) % 3) for k, n in cases]
    fields = {name: np.concatenate([getattr(p, name) for p in parts]) for name in HUB_FIELDS}
    h = HubMeasures([0, 5, 8, 12], **fields)
    assert len(h) == 3
    for i, p in enumerate(parts):
        same_hubs(h.graph(i), p, i)
        same_hubs(h.numpy().graph(i - 3), p, i)
        assert h.graph(i).node_off.tolist() == p.node_off.tolist()
    with pytest.raises(IndexError):
        h.graph(3)


def test_header_declares_the_hub_entry_points():
    from gnm import _cabi
    header = open(os.path.join(ROOT, "include", "gnm_hip.h")).read()
    body = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    new = ("gnm_topology_max_modules", "gnm_topology_betweenness_workspace_bytes", "gnm_topology_betweenness",
           "gnm_topology_modules")
    for name in new:
        m = re.search(r"\b%s\s*\(([^)]*)\)" % name, body)
        assert m, name
        params = [p for p in m.group(1).split(",") if p.strip() and p.strip() != "void"]
        assert len(params) == len(_cabi.SIGNATURES[name][1]), name
