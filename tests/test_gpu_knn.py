"""The kNN edge rule on the GPU (csrc/connectome.hip gnm_connectome_knn_structure; gnm/connectome.py knn_adjacency and the
knn= keyword of the builders).  Everything is bitwise, the feature has no tolerance: the selected adjacency equals the
host oracle knn_edges, the graphs equal order_graph of those edges, arena rows equal GraphArena.add_many of the host
twin, and model outputs equal those of host-built graphs, alone and mixed in one batch."""
import numpy as np
import pytest
import torch

from knn_cases import (arena_rows, bits_eq, fc_stack, hand_made, host_twin, ks_for, oracle_adjacency, same_graphs,
                       same_rows)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def oracle_stack(fc, k, mutual, absolute):
    return np.stack([oracle_adjacency(m, k, mutual, absolute) for m in fc])


# ---------------------------------------------------------------------------------------------------- selection
@pytest.mark.parametrize("absolute", [False, True])
@pytest.mark.parametrize("kind", ["corr", "ties"])
@pytest.mark.parametrize("n", [1, 2, 7, 63, 64, 65, 129, 400, 513, 1000])
def test_selection_equals_knn_edges(n, kind, absolute):
    from gnm.connectome import knn_adjacency
    S = 3 if n < 513 else 2
    fc = fc_stack(S, n, 17 * n + (kind == "ties"), kind)
    dev = torch.from_numpy(fc).to(DEV)
    for k in ks_for(n):
        for mutual in (False, True):
            got = knn_adjacency(dev, k, mutual, absolute)
            assert got.dtype == torch.bool and tuple(got.shape) == (S, n, n) and got.is_cuda
            assert np.array_equal(got.cpu().numpy(), oracle_stack(fc, k, mutual, absolute)), (k, mutual)


@pytest.mark.parametrize("n,k", [(65, 5), (129, 20)])
def test_hand_made_rows(n, k):
    from gnm.arena import GraphArena
    from gnm.connectome import graphs_from_connectivity, knn_adjacency
    cases = hand_made(n, k)
    names = list(cases)
    fc = np.stack([cases[x] for x in names])
    for mutual in (False, True):
        for absolute in (False, True):
            got = knn_adjacency(fc, k, mutual, absolute).cpu().numpy()                 # host input
            want = oracle_stack(fc, k, mutual, absolute)
            for j, name in enumerate(names):
                assert np.array_equal(got[j], want[j]), (name, mutual, absolute)
            assert np.array_equal(knn_adjacency(torch.from_numpy(fc).to(DEV), k, mutual, absolute).cpu().numpy(), got)
    # the node of the all-NaN row and column is isolated and reported, its neighbours in the stack are not
    ar = GraphArena(DEV)
    gs = graphs_from_connectivity(ar, fc, None, np.ones((n, 1), np.float32), [0] * len(names), knn=k)
    j = names.index("nan_row_and_column")
    assert ar.iso[gs[j]._gnm_cache[1]] and gs[j].neighbors[12] == []
    assert not ar.iso[gs[names.index("asymmetric")]._gnm_cache[1]]
    # fp32 input and its fp64 widening
    f32 = fc.astype(np.float32)
    for absolute in (False, True):
        a = knn_adjacency(f32, k, absolute=absolute).cpu().numpy()
        assert np.array_equal(a, knn_adjacency(f32.astype(np.float64), k, absolute=absolute).cpu().numpy())
        assert np.array_equal(a, knn_adjacency(torch.from_numpy(f32).to(DEV), k, absolute=absolute).cpu().numpy())
        assert np.array_equal(a, oracle_stack(f32.astype(np.float64), k, False, absolute))


# ---------------------------------------------------------------------------------------------------- graphs
GRAPH_CASES = [(1, 1, "corr", False), (2, 1, "corr", False), (7, 2, "ties", True), (63, 5, "corr", True),
               (64, 5, "ties", False), (65, 5, "ties", True), (65, 68, "corr", False), (129, 20, "ties", False),
               (129, 2, "corr", True), (400, 20, "corr", False), (513, 5, "ties", False), (1000, 20, "corr", False)]


@pytest.mark.parametrize("n,k,kind,mutual", GRAPH_CASES)
def test_graphs_and_arena_rows(n, k, kind, mutual):
    from gnm.arena import GraphArena
    from gnm.connectome import graphs_from_connectivity, knn_edges, order_graph
    S = 3 if n < 513 else 2
    fc = fc_stack(S, n, 200 + n + k, kind)
    absolute = (n % 2 == 0)
    feats = np.random.default_rng(0).standard_normal((S, n, 3)).astype(np.float32)
    ar = GraphArena(DEV)
    gs = graphs_from_connectivity(ar, fc, None, feats, list(range(S)), knn=k, mutual=mutual, absolute=absolute)
    for s, g in enumerate(gs):
        em, nb, mx = order_graph(n, *knn_edges(fc[s], k, mutual, absolute))
        assert len(g.g) == n and g.label == s
        assert np.array_equal(g.edge_mat.numpy(), em) and g.neighbors == nb and g.max_neighbor == mx
        assert bits_eq(g.node_features.numpy(), feats[s])
    ids = ar.add_many([host_twin(g) for g in gs])
    for g, gid in zip(gs, ids):
        same_rows(arena_rows(ar, g._gnm_cache[1]), arena_rows(ar, gid), (n, k, kind, mutual))
    iso = [bool(ar.iso[g._gnm_cache[1]]) for g in gs]
    deg_min = min(min(len(x) for x in g.neighbors) for g in gs)
    assert iso == [min(len(x) for x in g.neighbors) == 0 for g in gs]
    if (n, k, kind, mutual) == (65, 5, "ties", True):
        assert any(iso)                                   # a mutual graph on tie-heavy rows leaves nodes alone
    if (n, k, kind, mutual) == (400, 20, "corr", False):
        assert not any(iso) and deg_min >= 20             # the union graph: minimum degree k
    if not mutual and n > 1:
        assert deg_min >= min(k, n - 1)


def test_subject_chunks(monkeypatch):
    from gnm._cabi import lib
    from gnm.arena import GraphArena
    from gnm.connectome import graphs_from_connectivity
    n, S, k = 65, 5, 5
    fc = fc_stack(S, n, 77, "ties")
    feats = np.ones((n, 2), np.float32)
    ar = GraphArena(DEV)
    whole = graphs_from_connectivity(ar, fc, None, feats, [0] * S, knn=k)
    per = 4 * (int(lib.gnm_connectome_workspace_words(1, n)) + int(lib.gnm_connectome_knn_scratch_words(1, n)))
    for fit in (1, 2):
        # the selection bits count: one byte less than `fit` subjects' workspace and scratch fits fit - 1 of them
        monkeypatch.setattr(GraphArena, "CONNECTOME_WORK_BYTES", fit * per)
        ar2 = GraphArena(DEV)
        calls = []
        real = lib.gnm_connectome_knn_structure
        monkeypatch.setattr(lib, "gnm_connectome_knn_structure", lambda *a: (calls.append(a[1]), real(*a))[1])
        part = graphs_from_connectivity(ar2, fc, None, feats, [0] * S, knn=k)
        monkeypatch.setattr(lib, "gnm_connectome_knn_structure", real)
        assert calls == [fit] * (S // fit) + ([S % fit] if S % fit else [])
        same_graphs(part, whole)
        for g, h in zip(part, whole):
            same_rows(arena_rows(ar2, g._gnm_cache[1]), arena_rows(ar, h._gnm_cache[1]), fit)
    monkeypatch.setattr(GraphArena, "CONNECTOME_WORK_BYTES", 2 * per - 1)
    calls = []
    monkeypatch.setattr(lib, "gnm_connectome_knn_structure", lambda *a: (calls.append(a[1]), real(*a))[1])
    graphs_from_connectivity(GraphArena(DEV), fc, None, feats, [0] * S, knn=k)
    assert calls == [1] * S


def test_no_threshold_launch_on_the_knn_route(monkeypatch):
    from gnm._cabi import lib
    from gnm.arena import GraphArena
    from gnm.connectome import graphs_from_connectivity

    def refuse(*a):
        raise AssertionError("gnm_connectome_thresholds / _structure launched on the kNN route")
    monkeypatch.setattr(lib, "gnm_connectome_thresholds", refuse)
    monkeypatch.setattr(lib, "gnm_connectome_structure", refuse)
    gs = graphs_from_connectivity(GraphArena(DEV), fc_stack(2, 30, 1), None, np.ones((30, 1), np.float32), [0, 1], knn=3)
    assert len(gs) == 2 and gs[0].max_neighbor >= 3


def test_a_graph_does_not_depend_on_its_call():
    from gnm.arena import GraphArena
    from gnm.connectome import graphs_from_connectivity, knn_adjacency
    n, k = 129, 20
    fc = np.concatenate([fc_stack(2, n, 5, "ties"), fc_stack(2, n, 6, "corr")])
    feats = np.ones((n, 1), np.float32)
    ar = GraphArena(DEV)
    stack = graphs_from_connectivity(ar, fc, None, feats, [0] * 4, knn=k)
    again = graphs_from_connectivity(ar, fc, None, feats, [0] * 4, knn=k)
    adj = knn_adjacency(fc, k).cpu().numpy()
    assert np.array_equal(adj, knn_adjacency(fc, k).cpu().numpy())
    for s in range(4):
        alone = graphs_from_connectivity(ar, fc[s:s + 1], None, feats, [0], knn=k)[0]
        rows = arena_rows(ar, stack[s]._gnm_cache[1])
        same_rows(rows, arena_rows(ar, alone._gnm_cache[1]), s)
        same_rows(rows, arena_rows(ar, again[s]._gnm_cache[1]), s)
        assert np.array_equal(knn_adjacency(fc[s:s + 1], k).cpu().numpy()[0], adj[s])


# ---------------------------------------------------------------------------------------------------- builders
def factor_series(rng, T, n, quiet=None):
    """ROIs that share one strong factor; `quiet`: that ROI is nearly constant and runs against the factor, so that it
    correlates negatively with every other ROI in every window"""
    shared = rng.standard_normal((T, 1))
    x = rng.standard_normal((T, n)) + 1.5 * shared
    if quiet is not None:
        x[:, quiet] = 100.0 - 1e-3 * (shared[:, 0] + 0.1 * rng.standard_normal(T))
    return x


def test_timeseries_builder_equals_the_connectivity_builder():
    from gnm import connectome as C
    from gnm.arena import GraphArena
    rng = np.random.default_rng(21)
    ts = np.stack([factor_series(rng, 40, 65) for _ in range(3)])
    for kw in (dict(knn=5), dict(knn=7, mutual=True, absolute=True)):
        got = C.graphs_from_timeseries(GraphArena(DEV), ts, None, [0, 1, 0], **kw)
        ref = C.graphs_from_connectivity(GraphArena(DEV), C.connectivity_from_timeseries(ts), None,
                                         C.mean_bold_features(ts), [0, 1, 0], **kw)
        same_graphs(got, ref)
        assert got[0].edge_mat.shape[1] > 0


@pytest.mark.parametrize("tapered", [False, True])
def test_dynamic_builder_equals_the_materialised_fc(tapered, monkeypatch):
    from gnm import connectome as C
    from gnm.arena import GraphArena
    rng = np.random.default_rng(22)
    n, window, stride, k = 65, 17, 6, 5
    ts = [factor_series(rng, T, n) for T in (41, 17, 30)]
    labels = [0, 1, 1]
    w = np.hamming(window + 2)[1:-1] if tapered else None
    where = [(s, j, int(t0)) for s, x in enumerate(ts) for j, t0 in enumerate(C.window_starts(len(x), window, stride))]
    assert len(where) == 9
    fc = torch.cat(C.dynamic_connectivity_from_timeseries(ts, window, stride, taper=w))
    feats = C.mean_bold_features([ts[s][t0:t0 + window] for s, _, t0 in where])
    for kw in (dict(knn=k), dict(knn=k, mutual=True)):
        ref = C.graphs_from_connectivity(GraphArena(DEV), fc, None, feats, [labels[s] for s, _, _ in where], **kw)
        graphs, windows = C.dynamic_graphs_from_timeseries(GraphArena(DEV), ts, None, labels, window, stride, taper=w, **kw)
        assert windows.tolist() == [list(v) for v in where]
        same_graphs(graphs, ref)
        for per_chunk in (1, 2, 3):
            monkeypatch.setattr(C, "DYNFC_WORK_BYTES", per_chunk * 8 * n * n)
            assert max(hi - lo for lo, hi in C._plan_chunks(len(where), n, C.DYNFC_WORK_BYTES)) == per_chunk
            g2, w2 = C.dynamic_graphs_from_timeseries(GraphArena(DEV), ts, None, labels, window, stride, taper=w, **kw)
            assert np.array_equal(w2, windows)
            same_graphs(g2, ref)
        monkeypatch.undo()


def test_every_window_is_attributable_where_the_percentile_graph_is_not():
    """The point of the rule.  One ROI runs against the factor the others share: above a percentile of the whole window
    matrix it keeps no edge, and neighbour average + learn_eps then has a 0/0 row: edge_saliency declines the graph with
    ValueError, saliency leaves its kernel for autograd and returns NaN.  The kNN graph of the same window gives that ROI
    its k strongest connections, and both methods run on every window."""
    from gnm import connectome as C
    from models.graphcnn import GIN_InfoMaxReg
    rng = np.random.default_rng(23)
    n, window, stride, k = 65, 17, 8, 5
    ts = np.stack([factor_series(rng, 49, n, quiet=9) for _ in range(2)])
    torch.manual_seed(0)
    model = GIN_InfoMaxReg(3, 2, 1, 32, 2, 0.0, True, "sum", "average", torch.device(DEV)).to(DEV)
    model.eval()
    ar = model.arena()
    knn, windows = C.dynamic_graphs_from_timeseries(model, ts, None, [0, 1], window, stride, knn=k)
    edges = np.mean([g.edge_mat.shape[1] // 2 for g in knn])
    sparsity = 100.0 * (2 * edges + n) / (n * n)              # the same count of entries above the threshold
    pct, _ = C.dynamic_graphs_from_timeseries(model, ts, sparsity, [0, 1], window, stride)
    assert len(knn) == len(pct) == 10
    pe = np.mean([g.edge_mat.shape[1] // 2 for g in pct])
    assert 0.8 * edges <= pe <= 1.25 * edges, (edges, pe)     # a comparable edge count
    iso_pct = [bool(ar.iso[g._gnm_cache[1]]) for g in pct]
    iso_knn = [bool(ar.iso[g._gnm_cache[1]]) for g in knn]
    assert any(iso_pct) and not any(iso_knn)
    assert all(min(len(x) for x in g.neighbors) >= k for g in knn)
    sal = model.saliency(knn, (0, 1))
    assert model.saliency_routes == ["hip"] and tuple(sal.shape) == (2, 10, n, 1) and torch.isfinite(sal).all()
    es = model.edge_saliency(knn, 1)
    assert torch.isfinite(es).all()
    lone = [pct[iso_pct.index(True)]]
    assert len(lone[0].neighbors[9]) == 0
    with pytest.raises(ValueError, match="isolated"):
        model.edge_saliency(lone, 1)
    nan = model.saliency(lone, 1)
    assert model.saliency_routes == ["autograd"] and torch.isnan(nan).any()


# ---------------------------------------------------------------------------------------------------- model
def make_model(npool, learn_eps, f0, gpool="sum", seed=0, H=32):
    from models.graphcnn import GIN_InfoMaxReg
    torch.manual_seed(seed)
    return GIN_InfoMaxReg(3, 2, f0, H, 2, 0.0, learn_eps, gpool, npool, torch.device(DEV)).to(DEV)


def train_step(model, graphs):
    model.train()
    model.zero_grad(set_to_none=True)
    np.random.seed(3)
    c, d = model(graphs)
    loss = c.float().square().sum() + d.float().square().mean()
    loss.backward()
    torch.cuda.synchronize()
    return c.detach().cpu().numpy(), d.detach().cpu().numpy(), {k: p.grad.detach().cpu().numpy().copy()
                                                                  for k, p in model.named_parameters() if p.grad is not None}


@pytest.mark.parametrize("npool", ["sum", "average", "max"])
@pytest.mark.parametrize("learn_eps", [True, False])
def test_model_outputs_bitwise_equal_host_built(npool, learn_eps):
    from gnm.connectome import graphs_from_connectivity
    n, S, k = 60, 6, 6
    fc = fc_stack(S, n, 7)
    feat = np.eye(n, dtype=np.float32)                # one-hot: tied maxima under max pooling
    model = make_model(npool, learn_eps, n, gpool="average" if npool == "average" else "sum")
    gs = graphs_from_connectivity(model, fc, None, feat, [s % 2 for s in range(S)], knn=k)
    hs = [host_twin(g) for g in gs]
    p1, p2 = model.predict(gs).cpu().numpy(), model.predict(hs).cpu().numpy()
    assert bits_eq(p1, p2) and np.isfinite(p1).all()
    a, b = train_step(model, gs), train_step(model, hs)
    assert bits_eq(a[0], b[0]) and bits_eq(a[1], b[1])
    assert a[2].keys() == b[2].keys() and all(bits_eq(a[2][k], b[2][k]) for k in a[2])
    model.eval()
    s1, s2 = model.saliency(gs, (0, 1)), model.saliency(hs, (0, 1))
    assert bits_eq(s1.cpu().numpy(), s2.cpu().numpy())


def test_mixed_batch_of_knn_percentile_and_host_graphs():
    from gnm.connectome import graphs_from_connectivity
    n = 80
    model = make_model("sum", True, 5)
    rng = np.random.default_rng(1)
    feats = rng.standard_normal((3, n, 5)).astype(np.float32)
    kn = graphs_from_connectivity(model, fc_stack(3, n, 11), None, feats, [0, 1, 1], knn=6)
    pc = graphs_from_connectivity(model, fc_stack(3, n, 12), 25, feats, [1, 0, 1])
    hs = [host_twin(g) for g in graphs_from_connectivity(model, fc_stack(3, n, 13), None, feats, [0, 0, 1], knn=4,
                                                        mutual=True)]
    apart = np.concatenate([model.predict(x).cpu().numpy() for x in (kn, pc, hs)])
    order = [0, 3, 6, 1, 4, 7, 2, 5, 8]
    mixed = model.predict([(kn + pc + hs)[j] for j in order]).cpu().numpy()
    assert bits_eq(mixed, apart[order])
    assert bits_eq(model.predict(kn + pc + hs).cpu().numpy(), apart)


def test_sparse_regime_predicts_as_the_host_twins():
    """the CSR gather route: 1000 nodes, k = 20, H = 128, B = 2"""
    from gnm.connectome import graphs_from_connectivity
    n = 1000
    model = make_model("sum", True, 4, H=128)
    feats = np.random.default_rng(2).standard_normal((n, 4)).astype(np.float32)
    gs = graphs_from_connectivity(model, fc_stack(2, n, 31), None, feats, [0, 1], knn=20)
    p = model.predict(gs).cpu().numpy()
    assert bits_eq(p, model.predict([host_twin(g) for g in gs]).cpu().numpy()) and np.isfinite(p).all()


# ---------------------------------------------------------------------------------------------------- C-ABI
def test_c_entries_check_arguments_before_launching():
    from gnm._cabi import lib
    nmax = lib.gnm_connectome_max_nodes()
    n, S, k = 40, 2, 3
    fc = torch.from_numpy(fc_stack(S, n, 1)).to(DEV)
    work = torch.zeros(int(lib.gnm_connectome_workspace_words(S, n)) + 4, dtype=torch.int32, device=DEV)
    sel = torch.zeros(int(lib.gnm_connectome_knn_scratch_words(S, n)), dtype=torch.int32, device=DEV)
    nnz = torch.full((S,), -7, dtype=torch.int32, device=DEV)
    iso = torch.full((S,), -7, dtype=torch.int32, device=DEV)
    knn, words = lib.gnm_connectome_knn_structure, lib.gnm_connectome_knn_scratch_words
    p = [fc.data_ptr(), sel.data_ptr(), work.data_ptr(), nnz.data_ptr(), iso.data_ptr()]
    assert work.data_ptr() % 16 == 0
    assert knn(p[0], S, n, 0, 0, p[1], p[2], p[3], p[4], None) == -1                     # k = 0
    assert knn(p[0], S, n, -1, 0, p[1], p[2], p[3], p[4], None) == -1
    assert knn(p[0], S, n, k, 4, p[1], p[2], p[3], p[4], None) == -1                     # an unknown flag
    assert knn(p[0], S, 0, k, 0, p[1], p[2], p[3], p[4], None) == -1
    assert knn(p[0], -1, n, k, 0, p[1], p[2], p[3], p[4], None) == -1
    assert knn(p[0], S, nmax + 1, k, 0, p[1], p[2], p[3], p[4], None) == -2              # n above the limit
    for hole in range(5):                                                                # null pointers, each in turn
        q = list(p)
        q[hole] = None
        assert knn(q[0], S, n, k, 0, q[1], q[2], q[3], q[4], None) == -1
    assert knn(p[0], S, n, k, 0, p[1], p[2] + 4, p[3], p[4], None) == -1                 # a misaligned work
    assert knn(None, 0, n, k, 0, None, None, None, None, None) == 0                      # S = 0: GNM_OK, no launch
    assert knn(None, 0, n, 0, 0, None, None, None, None, None) == -1                     # a bad k even then
    torch.cuda.synchronize()
    assert (nnz.cpu() == -7).all() and (iso.cpu() == -7).all() and not work.cpu().any()  # nothing above launched
    assert words(3, 65) == 3 * 65 * 3 and words(0, 400) == 0 and words(2, nmax) == 2 * nmax * (nmax // 32)
    assert words(-1, 8) == -1 and words(1, 0) == -1 and words(1, nmax + 1) == -1
    # and a good call does launch
    assert knn(p[0], S, n, k, 0, p[1], p[2], p[3], p[4], None) == 0
    torch.cuda.synchronize()
    assert (nnz.cpu() >= 2 * k).all() and (iso.cpu() == 0).all()
