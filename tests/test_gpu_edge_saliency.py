"""GIN_InfoMaxReg.edge_saliency(): the connectivity saliency d score / d A (csrc/edgesal.hip over gnm_saliency's layer
launches) against the reference's goldens (tests/golden/edge/) and the fp64 dense-adjacency restatement of
tests/test_edge_saliency_host.py; declined shapes, batch invariance, determinism, return shapes, side effects (none) and
NaN confinement."""
import numpy as np
import pytest
import torch

from test_edge_saliency_host import EDGE_CASES, load_edge_case, restate_edge
from test_gpu_class_activation import multigraph, state64
from test_gpu_saliency import Graph, model_of, random_graph

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EDGE_RTOL = 1e-5        # max|map - reference| / max|reference|, per graph and class


def reference_edges(model, graphs, classes):
    st = state64(model)
    out = {}
    for i, g in enumerate(graphs):
        em = g.edge_mat.numpy()
        for c in classes:
            out[i, c] = restate_edge(st, model.num_layers, model.num_mlp_layers, model.learn_eps,
                                     model.graph_pooling_type, model.neighbor_pooling_type, em[0], em[1],
                                     g.node_features.numpy(), c).numpy()
    return out


def check_edges(model, graphs, classes=(0, 1), batch_size=64, what=""):
    got = model.edge_saliency(graphs, tuple(classes), batch_size=batch_size)
    ref = reference_edges(model, graphs, classes)
    worst = 0.0
    for ci, c in enumerate(classes):
        for i, g in enumerate(graphs):
            r = ref[i, c]
            x = got[ci][i].cpu().numpy()
            assert x.shape == r.shape
            scale = np.abs(r).max()
            err = np.abs(x - r).max()
            assert err <= EDGE_RTOL * scale, "%s graph %d class %d: %.3e of %.3e" % (what, i, c, err, scale)
            worst = max(worst, err / scale)
            # absent entries (and the diagonal) are part of the contract: non-trivial, and they match too
            n = r.shape[0]
            em = g.edge_mat.numpy()
            A = np.zeros((n, n), bool)
            A[em[0], em[1]] = True
            if not model.learn_eps:
                A[np.arange(n), np.arange(n)] = True
            off = ~A
            if off.any():
                assert np.abs(r[off]).max() > 1e-3 * scale, (what, i, c)
                assert np.abs(x[off] - r[off]).max() <= EDGE_RTOL * scale
            diag = np.diagonal(r)
            assert np.abs(diag).max() > 1e-3 * scale, (what, i, c)
            assert np.abs(np.diagonal(x) - diag).max() <= EDGE_RTOL * scale
    print("worst rel err %s: %.2e" % (what, worst))
    return got, worst


def golden_model_and_graphs(case):
    from models.graphcnn import GIN_InfoMaxReg
    cfg, state, d = load_edge_case(case)
    model = GIN_InfoMaxReg(cfg["L"], cfg["m"], cfg["f0"], cfg["H"], cfg["C"], 0.0, cfg["learn_eps"], cfg["gpool"],
                           cfg["npool"], torch.device(DEV)).to(DEV)
    missing, unexpected = model.load_state_dict({k: torch.as_tensor(v) for k, v in state.items()}, strict=False)
    assert not unexpected and all(k.startswith("disc.") for k in missing)
    graphs = []
    for g in range(cfg["B"]):
        und = d[f"und_{g}"].astype(np.int64)
        both = np.concatenate([und, und[:, ::-1]], 0)                      # util.py:99-103
        graphs.append(Graph(cfg["n"], both[:, 0], both[:, 1], d[f"feat_{g}"], int(d["labels"][g])))
    return cfg, d, model, graphs


@pytest.mark.parametrize("case", EDGE_CASES)
def test_against_reference_goldens(case):
    cfg, d, model, graphs = golden_model_and_graphs(case)
    got = model.edge_saliency(graphs, (0, 1))
    assert got.shape == (2, cfg["B"], cfg["n"], cfg["n"])
    for g in range(cfg["B"]):
        for c in (0, 1):
            ref = d[f"edge_{g}_{c}"]
            err = np.abs(got[c, g].cpu().numpy() - ref).max()
            assert err <= EDGE_RTOL * np.abs(ref).max(), (g, c, err)


def test_max_pooling_declines():
    from models.graphcnn import GIN_InfoMaxReg
    cfg, d, _, graphs = golden_model_and_graphs(EDGE_CASES[0])
    model = GIN_InfoMaxReg(cfg["L"], cfg["m"], cfg["f0"], cfg["H"], cfg["C"], 0.0, True, "sum", "max",
                           torch.device(DEV)).to(DEV)
    with pytest.raises(ValueError, match="max neighbour pooling"):
        model.edge_saliency(graphs, (0, 1))


POOLS = [(np_, gp, le) for np_ in ("sum", "average") for gp in ("sum", "average") for le in (True, False)]


@pytest.mark.parametrize("m", [1, 2, 3])
@pytest.mark.parametrize("H", [32, 64, 128])
def test_small_graphs(H, m):
    """40-node graphs (one asymmetric, one with an isolated node where defined) in batches of 3, and tiny 6-node
    graphs, F0 = 7, every sum / average pooling and eps form"""
    for npool, gpool, le in POOLS:
        model = model_of(3, m, 7, H, le, gpool, npool, seed=H + m)
        iso = 0 if (npool == "average" and le) else 2
        gs = [random_graph(10 + i, 40, 0.2, 7, directed=(i == 2), iso=iso if i == 3 else 0) for i in range(5)]
        tiny = [random_graph(50 + i, 6, 0.4, 7) for i in range(4)]
        check_edges(model, gs, batch_size=3, what="H%d m%d %s/%s eps%d" % (H, m, npool, gpool, le))
        check_edges(model, tiny, what="tiny H%d m%d %s/%s eps%d" % (H, m, npool, gpool, le))


@pytest.mark.parametrize("npool,learn_eps", [(np_, le) for np_ in ("sum", "average") for le in (True, False)])
@pytest.mark.parametrize("one_hot", [False, True])
def test_400_node_dense(npool, learn_eps, one_hot):
    """the reference's shape: 400-node dense connectivity graphs (30 % fill), H = 64, L = 5, F0 = 7 or one-hot 400"""
    from gnm import synth
    gs = [synth.dense_fc_graph(g, n=400) for g in range(2)]
    if one_hot:
        for g in gs:
            g.node_features = torch.eye(400)
    f0 = 400 if one_hot else 7
    gpool = "average" if npool == "sum" else "sum"
    model = model_of(5, 2, f0, 64, learn_eps, gpool, npool, seed=7)
    got, worst = check_edges(model, gs, what="400-node %s/%s eps%d one_hot%d" % (npool, gpool, learn_eps, one_hot))
    assert got.shape == (2, 2, 400, 400)


@pytest.mark.parametrize("shape,why", [("knn1000", "more than 416 nodes"), ("multigraph", "bit adjacency"),
                                       ("H36", "hidden_dim 36"), ("iso", "isolated node")])
def test_declines(shape, why):
    from gnm import synth
    if shape == "knn1000":
        model, gs = model_of(2, 2, 7, 128, False, "average", "sum", seed=6), [synth.knn_graph(0, n=1000)]
    elif shape == "multigraph":
        model, gs = model_of(3, 2, 7, 64, True, "sum", "average", seed=13), [multigraph(160, 30, 7)]
    elif shape == "H36":
        model, gs = model_of(3, 2, 7, 36, True, "sum", "average", seed=8), [random_graph(120, 30, 0.2, 7)]
    else:
        model, gs = model_of(2, 2, 7, 64, True, "sum", "average", seed=3), [random_graph(70, 30, 0.2, 7, iso=3)]
    for training in (True, False):
        model.train(training)
        with pytest.raises(ValueError, match=why):
            model.edge_saliency(gs, 0)
        assert model.training == training


def test_batch_invariant_and_deterministic():
    model = model_of(3, 2, 7, 64, False, "sum", "average", seed=15)
    gs = [random_graph(180 + i, 40, 0.2, 7) for i in range(7)]
    a = model.edge_saliency(gs, (0, 1))
    b = model.edge_saliency(gs, (0, 1))
    assert torch.equal(a, b)                                  # bitwise, run to run
    for bs in (1, 3):
        other = model.edge_saliency(gs, (0, 1), batch_size=bs)
        for i in range(len(gs)):
            for c in (0, 1):
                assert (a[c, i] - other[c, i]).abs().max() <= EDGE_RTOL * other[c, i].abs().max()


def test_return_shapes():
    model = model_of(3, 2, 7, 64, True, "average", "sum", seed=4)
    gs = [random_graph(90 + i, n, 0.2, 7) for i, n in enumerate((20, 33, 64, 7, 1))]
    got, _ = check_edges(model, gs, batch_size=3, what="ragged")
    assert isinstance(got, list) and [x.shape for x in got[0]] == [(n, n) for n in (20, 33, 64, 7, 1)]
    one = model.edge_saliency(gs, 1, batch_size=3)
    assert isinstance(one, list) and all(torch.equal(a, b) for a, b in zip(one, got[1]))
    same = [random_graph(100 + i, 24, 0.3, 7) for i in range(3)]
    seq = model.edge_saliency(same, (1, 0, 1))
    assert seq.shape == (3, 3, 24, 24)
    single = model.edge_saliency(same, 0)
    assert single.shape == (3, 24, 24) and torch.equal(single, seq[1]) and torch.equal(seq[0], seq[2])


@pytest.mark.parametrize("start_training", [True, False])
def test_no_side_effects(start_training):
    model = model_of(3, 2, 7, 64, True, "average", "sum", seed=11)
    gs = [random_graph(140 + i, 40, 0.2, 7) for i in range(4)]
    for i, p in enumerate(model.parameters()):
        if i % 3:
            p.grad = torch.randn_like(p)
    grads = {n: (p.grad.clone() if p.grad is not None else None) for n, p in model.named_parameters()}
    bufs = {n: b.clone() for n, b in model.named_buffers()}
    model.train(start_training)
    np.random.seed(123)
    rng = np.random.get_state()
    model.edge_saliency(gs, (0, 1))
    assert model.training == start_training
    st = np.random.get_state()
    assert st[0] == rng[0] and np.array_equal(st[1], rng[1]) and st[2:] == rng[2:]
    for n, p in model.named_parameters():
        if grads[n] is None:
            assert p.grad is None, n
        else:
            assert torch.equal(p.grad, grads[n]), n
    for n, b_ in model.named_buffers():
        assert torch.equal(b_, bufs[n]), n


def test_nan_stays_in_its_graph():
    model = model_of(3, 2, 7, 64, True, "sum", "sum", seed=12)
    gs = [random_graph(150 + i, 40, 0.2, 7) for i in range(3)]
    clean = model.edge_saliency(gs, (0, 1))
    gs[1].node_features = gs[1].node_features.clone()
    gs[1].node_features[5, 2] = float("nan")
    model._arena = None                                   # the arena caches a graph's features once per arena
    got = model.edge_saliency(gs, (0, 1))
    for c in (0, 1):
        assert torch.equal(got[c, 0], clean[c, 0]) and torch.equal(got[c, 2], clean[c, 2])
        assert torch.isnan(got[c, 1]).all()
