"""The device connectome builder (gnm/connectome.py, csrc/connectome.hip) on the GPU: thresholds bitwise equal to
np.percentile, graphs equal to the reference loader's goldens, arena rows bitwise equal to GraphArena.add of the same
graph, and model outputs bitwise equal between device-built and host-built graphs, alone and mixed in one batch."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
import connectome_goldens

GOLDEN = connectome_goldens.PATHS
SPARSITIES = [0, 0.5, 1, 30, 33.3, 70, 99.99, 100]


def same_bits(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a.shape == b.shape and (np.array_equal(a.view(np.uint64), b.view(np.uint64))
                                   or (np.isnan(a) == np.isnan(b)).all() and np.array_equal(a[~np.isnan(a)].view(np.uint64),
                                                                                             b[~np.isnan(b)].view(np.uint64)))


def bits_eq(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def fc_stack(S, n, seed, kind="corr"):
    rng = np.random.default_rng(seed)
    if kind == "corr":
        return np.stack([np.corrcoef(rng.standard_normal((max(n, 2) + 3, n)).T).reshape(n, n) for _ in range(S)])
    if kind == "ties":
        return rng.integers(-3, 4, (S, n, n)).astype(np.float64) / 4
    raise ValueError(kind)


@pytest.mark.parametrize("n", [1, 2, 7, 400, 1000])
def test_thresholds_bitwise_equal_numpy(n):
    from gnm.connectome import connectivity_thresholds
    S = 3 if n < 1000 else 2
    mats = [fc_stack(S, n, n), fc_stack(S, n, n + 1, "ties")]
    if n >= 2:
        inf = fc_stack(S, n, n + 2).copy()
        inf[0, 0, 1] = np.inf
        inf[1, :, : n // 2] = -np.inf
        inf[2 % S, 1, 0] = np.inf
        inf[2 % S, 0, 0] = -np.inf
        mats.append(inf)
    for fc in mats:
        for sp in SPARSITIES:
            got = connectivity_thresholds(fc, sp).cpu().numpy()
            want = np.array([np.percentile(fc[s], 100 - sp) for s in range(S)])
            assert same_bits(got, want), (n, sp, got, want)


def test_thresholds_nan_float32_and_device_input():
    from gnm.arena import GraphArena
    from gnm.connectome import connectivity_thresholds, graphs_from_connectivity
    fc = fc_stack(3, 50, 9)
    fc[1, 7, 3] = np.nan
    thr = connectivity_thresholds(fc, 30).cpu().numpy()
    assert np.isnan(thr[1]) and not np.isnan(thr[0]) and not np.isnan(thr[2])
    f32 = fc_stack(2, 64, 3).astype(np.float32)
    wide = f32.astype(np.float64)
    for sp in (30, 12.5):
        got = connectivity_thresholds(torch.from_numpy(f32).to(DEV), sp).cpu().numpy()
        assert same_bits(got, [np.percentile(wide[s], 100 - sp) for s in range(2)])
    ar = GraphArena(DEV)
    gs = graphs_from_connectivity(ar, fc, 30, np.ones((50, 2), np.float32), [0, 1, 0])
    assert gs[1].edge_mat.shape == (2, 0) and gs[1].max_neighbor == 0 and ar.nnz[gs[1]._gnm_cache[1]] == 0
    assert all(len(x) == 0 for x in gs[1].neighbors) and ar.iso[gs[1]._gnm_cache[1]]


@pytest.mark.parametrize("path", GOLDEN, ids=[os.path.basename(p) for p in GOLDEN])
def test_graphs_equal_the_reference_loader(path):
    from gnm.arena import GraphArena
    from gnm.connectome import graphs_from_connectivity
    d = connectome_goldens.load(path)
    fc, feat, labels = d["fc"], d["feat"], d["labels"]
    ar = GraphArena(DEV)
    built = {}
    for sp, s, em, nb, mx in d["graphs"]:
        if sp not in built:
            src = torch.from_numpy(fc).to(DEV) if sp == 50 else fc          # host and device input
            built[sp] = graphs_from_connectivity(ar, src, sp, feat, labels)
        g = built[sp][s]
        assert len(g.g) == fc.shape[1] and g.label == labels[s] and g.node_tags is None
        assert np.array_equal(g.edge_mat.numpy(), em), (sp, s)
        assert g.neighbors == nb, (sp, s)
        assert g.max_neighbor == mx
        assert np.array_equal(g.node_features.numpy(), feat)


def host_twin(g):
    """the same graph built the host way: a SynthGraph of the device graph's edge_mat and neighbours"""
    from gnm.synth import SynthGraph
    em = g.edge_mat.numpy()
    h = SynthGraph(len(g.g), em[:, :em.shape[1] // 2].T, g.node_features.numpy(), g.label)
    assert np.array_equal(h.edge_mat.numpy(), em)
    h.neighbors = [list(x) for x in g.neighbors]
    h.max_neighbor = g.max_neighbor
    return h


def arena_rows(ar, gid):
    n, E = ar.n[gid], ar.nnz[gid]
    rp = ar.rowptr.buf[ar.rp_off[gid]:ar.rp_off[gid] + n + 1].cpu().numpy()
    col = ar.col.buf[ar.col_off[gid]:ar.col_off[gid] + E].cpu().numpy()
    from gnm._cabi import lib
    w = int(lib.gnm_adj_bits_words(n))
    bits = ar.bits.buf[ar.bits_off[gid]:ar.bits_off[gid] + w].cpu().numpy() if ar.bits_ok[gid] else None
    return rp, col, bits, E, ar.iso[gid], ar.sym[gid], ar.bits_ok[gid]


@pytest.mark.parametrize("n,sp,kind", [(400, 30, "corr"), (100, 5, "ties"), (37, 50, "corr"), (1000, 10, "corr"),
                                       (7, 100, "corr")])
def test_arena_rows_bitwise_equal_add(n, sp, kind):
    from gnm.arena import GraphArena
    from gnm.connectome import graphs_from_connectivity
    S = 4 if n < 1000 else 2
    fc = fc_stack(S, n, 100 + n, kind)
    ar = GraphArena(DEV)
    gs = graphs_from_connectivity(ar, fc, sp, np.random.default_rng(0).standard_normal((S, n, 3)).astype(np.float32),
                                  list(range(S)))
    twins = [host_twin(g) for g in gs]
    ids = ar.add_many(twins)
    for g, gid in zip(gs, ids):
        a, b = arena_rows(ar, g._gnm_cache[1]), arena_rows(ar, gid)
        for x, y in zip(a, b):
            assert (x is None and y is None) or np.array_equal(np.asarray(x), np.asarray(y)), (n, sp)
        assert np.array_equal(ar.feat.buf[ar.feat_off[gid]:ar.feat_off[gid] + n].cpu().numpy(),
                              ar.feat.buf[ar.feat_off[g._gnm_cache[1]]:ar.feat_off[g._gnm_cache[1]] + n].cpu().numpy())


def make_model(npool, learn_eps, f0, gpool="sum", seed=0):
    from models.graphcnn import GIN_InfoMaxReg
    torch.manual_seed(seed)
    return GIN_InfoMaxReg(3, 2, f0, 32, 2, 0.0, learn_eps, gpool, npool, torch.device(DEV)).to(DEV)


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
    n, S = 60, 6
    fc = fc_stack(S, n, 7)
    feat = np.eye(n, dtype=np.float32)                # one-hot: tied maxima under max pooling
    model = make_model(npool, learn_eps, n, gpool="average" if npool == "average" else "sum")
    gs = graphs_from_connectivity(model, fc, 30, feat, [s % 2 for s in range(S)])
    hs = [host_twin(g) for g in gs]
    p1, p2 = model.predict(gs).cpu().numpy(), model.predict(hs).cpu().numpy()
    assert bits_eq(p1, p2)
    a, b = train_step(model, gs), train_step(model, hs)
    assert bits_eq(a[0], b[0]) and bits_eq(a[1], b[1])
    assert a[2].keys() == b[2].keys() and all(bits_eq(a[2][k], b[2][k]) for k in a[2])
    model.eval()
    s1, s2 = model.saliency(gs, (0, 1)), model.saliency(hs, (0, 1))
    assert bits_eq(s1.cpu().numpy(), s2.cpu().numpy())


def test_mixed_batch():
    from gnm.connectome import graphs_from_connectivity
    n = 80
    model = make_model("sum", True, 5)
    rng = np.random.default_rng(1)
    gs = graphs_from_connectivity(model, fc_stack(4, n, 11), 25, rng.standard_normal((4, n, 5)).astype(np.float32),
                                  [0, 1, 1, 0])
    hs = [host_twin(g) for g in gs]
    mixed = [gs[0], hs[1], gs[2], hs[3]]
    p_dev, p_host, p_mix = (model.predict(x).cpu().numpy() for x in (gs, hs, mixed))
    assert bits_eq(p_dev, p_host) and bits_eq(p_mix, p_dev)
    a, b = train_step(model, mixed), train_step(model, hs)
    assert bits_eq(a[0], b[0]) and all(bits_eq(a[2][k], b[2][k]) for k in a[2])
    # graphs of the second kind added after the first keep working with the earlier ones
    more = graphs_from_connectivity(model.arena(), fc_stack(2, n, 12), 25, rng.standard_normal((n, 5)).astype(np.float32),
                                    [1, 0])
    assert model.predict(gs + more + hs).shape == (10, 2)
