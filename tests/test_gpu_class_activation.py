"""GIN_InfoMaxReg.class_activation(): the per-node class activation maps (csrc/cam.hip for kind="activation",
csrc/saliency.hip's gnm_saliency_maps for kind="gradient") against the reference's goldens (tests/golden/cam/), the fp64
restatement of tests/test_cam_host.py, the eval logits; batch invariance, determinism, side effects (none), the gradient
kind's declined shapes and NaN confinement."""
import numpy as np
import pytest
import torch

from helpers import neighbors_of
from test_cam_host import CAM_CASES, load_cam_case, restate
from test_gpu_saliency import Graph, model_of, random_graph

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CAM_RTOL = 1e-5         # max|map - reference| / max|reference|, per graph


def state64(model):
    return {k: v.detach().cpu().numpy().astype(np.float64) if v.dtype.is_floating_point else v.cpu().numpy()
            for k, v in model.state_dict().items()}


def reference_maps(model, graphs, classes, kind, state=None):
    """the fp64 restatement, one graph at a time: {(i, c): map}"""
    st = state if state is not None else state64(model)
    out = {}
    for i, g in enumerate(graphs):
        em = g.edge_mat.numpy()
        for c in classes:
            _, _, cam, gcam, _ = restate(st, model.num_layers, model.num_mlp_layers, model.learn_eps,
                                         model.graph_pooling_type, model.neighbor_pooling_type, em[0], em[1],
                                         g.neighbors, g.node_features.numpy(), c)
            out[i, c] = (cam if kind == "activation" else gcam).numpy()
    return out


def check_maps(model, graphs, kind, classes=(0, 1), batch_size=256):
    got = model.class_activation(graphs, tuple(classes), kind=kind, batch_size=batch_size)
    ref = reference_maps(model, graphs, classes, kind)
    worst = 0.0
    for ci, c in enumerate(classes):
        for i in range(len(graphs)):
            r = ref[i, c]
            g = got[ci][i].cpu().numpy()
            assert g.shape == r.shape
            scale = np.abs(r).max()
            err = np.abs(g - r).max()
            assert err <= CAM_RTOL * scale, "%s graph %d class %d: %.3e of %.3e" % (kind, i, c, err, scale)
            worst = max(worst, err / scale if scale > 0 else 0.0)
    return got, worst


def golden_model_and_graphs(case):
    from models.graphcnn import GIN_InfoMaxReg
    cfg, state, d = load_cam_case(case)
    model = GIN_InfoMaxReg(cfg["L"], cfg["m"], cfg["f0"], cfg["H"], cfg["C"], 0.0, cfg["learn_eps"], cfg["gpool"],
                           cfg["npool"], torch.device(DEV)).to(DEV)
    missing, unexpected = model.load_state_dict({k: torch.as_tensor(v) for k, v in state.items()}, strict=False)
    assert not unexpected and all(k.startswith("disc.") for k in missing)
    graphs = []
    for g in range(cfg["B"]):
        und = d[f"und_{g}"].astype(np.int64)
        both = np.concatenate([und, und[:, ::-1]], 0)                      # util.py:99-103
        gr = Graph(cfg["n"], both[:, 0], both[:, 1], d[f"feat_{g}"], int(d["labels"][g]))
        gr.neighbors = neighbors_of(und, cfg["n"])                          # the reference's order (max pooling ties)
        gr.max_neighbor = max(len(x) for x in gr.neighbors)
        graphs.append(gr)
    return cfg, d, model, graphs


@pytest.mark.parametrize("kind", ["activation", "gradient"])
@pytest.mark.parametrize("case", CAM_CASES)
def test_against_reference_goldens(case, kind):
    cfg, d, model, graphs = golden_model_and_graphs(case)
    if kind == "gradient" and cfg["npool"] == "max":
        with pytest.raises(ValueError, match="max neighbour pooling"):
            model.class_activation(graphs, (0, 1), kind=kind)
        return
    got = model.class_activation(graphs, (0, 1), kind=kind)
    key = "cam" if kind == "activation" else "gcam"
    for g in range(cfg["B"]):
        for c in (0, 1):
            ref = d[f"{key}_{g}_{c}"]
            err = np.abs(got[c, g].cpu().numpy() - ref).max()
            assert err <= CAM_RTOL * np.abs(ref).max(), (g, c, err)


POOLS = [(np_, gp, le) for np_ in ("sum", "average") for gp in ("sum", "average") for le in (True, False)]


@pytest.mark.parametrize("m", [1, 2, 3])
@pytest.mark.parametrize("H", [32, 64, 128])
def test_small_graphs_both_kinds(H, m):
    """40-node graphs (one asymmetric) in batches of 3, and tiny 6-node graphs, F0 = 7, every pooling form"""
    worst = 0.0
    for npool, gpool, le in POOLS:
        model = model_of(3, m, 7, H, le, gpool, npool, seed=H + m)
        gs = [random_graph(10 + i, 40, 0.2, 7, directed=(i == 2)) for i in range(5)]
        tiny = [random_graph(50 + i, 6, 0.4, 7) for i in range(4)]
        for kind in ("activation", "gradient"):
            worst = max(worst, check_maps(model, gs, kind, batch_size=3)[1], check_maps(model, tiny, kind)[1])
    print("worst rel err H=%d m=%d: %.2e" % (H, m, worst))


@pytest.mark.parametrize("npool,gpool,learn_eps", [("sum", "sum", True), ("average", "average", False)])
@pytest.mark.parametrize("one_hot", [False, True])
def test_400_node_dense_both_kinds(npool, gpool, learn_eps, one_hot):
    """the reference's shape: 400-node dense connectivity graphs, H = 64, F0 = 7 or one-hot 400"""
    from gnm import synth
    gs = [synth.dense_fc_graph(g, n=400) for g in range(3)]
    if one_hot:
        for g in gs:
            g.node_features = torch.eye(400)
    f0 = 400 if one_hot else 7
    model = model_of(3, 2, f0, 64, learn_eps, gpool, npool, seed=7)
    for kind in ("activation", "gradient"):
        got, worst = check_maps(model, gs, kind, batch_size=2)
        assert got.shape == (2, 3, 400)
        print("worst rel err 400-node", kind, npool, gpool, learn_eps, one_hot, worst)


def test_ragged_batches_return_lists():
    model = model_of(3, 2, 7, 64, True, "average", "sum", seed=4)
    gs = [random_graph(90 + i, n, 0.2, 7) for i, n in enumerate((20, 33, 64, 7, 1))]
    for kind in ("activation", "gradient"):
        got, _ = check_maps(model, gs, kind, batch_size=3)
        assert isinstance(got, list) and [x.shape[0] for x in got[0]] == [20, 33, 64, 7, 1]
        one = model.class_activation(gs, 1, kind=kind, batch_size=3)
        assert isinstance(one, list) and all(torch.equal(a, b) for a, b in zip(one, got[1]))


def multigraph(seed, n, f0):
    """a graph whose edge list repeats some edges (the reference's spmm sums duplicates)"""
    g = random_graph(seed, n, 0.2, f0)
    src, dst = g.edge_mat.numpy()
    k = len(src) // 4
    return Graph(n, np.concatenate([src, src[:k]]), np.concatenate([dst, dst[:k]]), g.node_features.numpy(), g.label)


@pytest.mark.parametrize("shape", ["max_sum_eps", "max_avg_self", "knn1000", "multigraph", "H36", "ragged_max"])
def test_activation_kind_wider_shapes(shape):
    """what only the activation kind covers: max pooling, the CSR-gather path (n = 1000), multigraphs, H = 36"""
    from gnm import synth
    if shape == "max_sum_eps":
        model, gs = model_of(3, 2, 7, 64, True, "sum", "max", seed=5), [random_graph(110 + i, 30, 0.2, 7)
                                                                           for i in range(3)]
    elif shape == "max_avg_self":
        model, gs = model_of(3, 2, 7, 32, False, "average", "max", seed=5), [random_graph(115 + i, 30, 0.2, 7, iso=2)
                                                                               for i in range(3)]
    elif shape == "knn1000":
        model, gs = model_of(2, 2, 7, 128, False, "average", "sum", seed=6), [synth.knn_graph(g, n=1000)
                                                                                for g in range(2)]
    elif shape == "multigraph":
        model, gs = model_of(3, 2, 7, 64, True, "sum", "average", seed=13), [multigraph(160 + i, 30, 7)
                                                                               for i in range(3)]
    elif shape == "H36":
        model, gs = model_of(3, 2, 7, 36, True, "sum", "average", seed=8), [random_graph(120 + i, 30, 0.2, 7)
                                                                              for i in range(3)]
    else:
        model, gs = model_of(2, 2, 7, 32, False, "average", "max", seed=9), [random_graph(130 + i, n, 0.3, 7)
                                                                               for i, n in enumerate((12, 25, 9))]
    got, worst = check_maps(model, gs, "activation", batch_size=2)
    print("worst rel err", shape, worst)


@pytest.mark.parametrize("shape,why", [("max", "max neighbour pooling"), ("knn1000", "more than 416 nodes"),
                                       ("H36", "hidden_dim 36"), ("iso", "isolated node")])
def test_gradient_kind_declines(shape, why):
    from gnm import synth
    if shape == "max":
        model, gs = model_of(3, 2, 7, 64, True, "sum", "max", seed=5), [random_graph(110, 30, 0.2, 7)]
    elif shape == "knn1000":
        model, gs = model_of(2, 2, 7, 128, False, "average", "sum", seed=6), [synth.knn_graph(0, n=1000)]
    elif shape == "H36":
        model, gs = model_of(3, 2, 7, 36, True, "sum", "average", seed=8), [random_graph(120, 30, 0.2, 7)]
    else:
        model, gs = model_of(2, 2, 7, 64, True, "sum", "average", seed=3), [random_graph(70, 30, 0.2, 7, iso=3)]
    model.train()
    with pytest.raises(ValueError, match=why):
        model.class_activation(gs, 0, kind="gradient")
    assert model.training


@pytest.mark.parametrize("npool,gpool,learn_eps", [("sum", "sum", True), ("average", "average", False),
                                                   ("max", "average", True), ("max", "sum", False)])
def test_activation_sums_to_the_eval_logit(npool, gpool, learn_eps):
    model = model_of(3, 2, 7, 64, learn_eps, gpool, npool, seed=14)
    gs = [random_graph(170 + i, 40, 0.2, 7) for i in range(6)]
    cam = model.class_activation(gs, (0, 1))
    logits = model.predict(gs)
    for c in (0, 1):
        bias = sum(model.linears_prediction[l].bias[c] for l in range(3))
        total = cam[c].sum(1) + bias
        bound = CAM_RTOL * (cam[c].abs().sum(1) + sum(abs(model.linears_prediction[l].bias[c]) for l in range(3)))
        assert torch.all((total - logits[:, c]).abs() <= bound), (total, logits[:, c])


@pytest.mark.parametrize("kind", ["activation", "gradient"])
def test_batch_invariant_and_deterministic(kind):
    model = model_of(3, 2, 7, 64, True, "sum", "average", seed=15)
    gs = [random_graph(180 + i, 40, 0.2, 7) for i in range(7)]
    a = model.class_activation(gs, (0, 1), kind=kind)
    b = model.class_activation(gs, (0, 1), kind=kind)
    one = model.class_activation(gs, (0, 1), kind=kind, batch_size=1)
    assert torch.equal(a, b)
    for i in range(len(gs)):
        for c in (0, 1):
            assert (a[c, i] - one[c, i]).abs().max() <= CAM_RTOL * one[c, i].abs().max()


@pytest.mark.parametrize("kind", ["activation", "gradient"])
@pytest.mark.parametrize("start_training", [True, False])
def test_no_side_effects(kind, start_training):
    model = model_of(3, 2, 7, 64, True, "average", "sum", seed=11)
    gs = [random_graph(140 + i, 40, 0.2, 7) for i in range(4)]
    for i, p in enumerate(model.parameters()):
        if i % 3:
            p.grad = torch.randn_like(p)
    grads = {n: (p.grad.clone() if p.grad is not None else None) for n, p in model.named_parameters()}
    bufs = {n: b.clone() for n, b in model.named_buffers()}
    sal_before = model.saliency(gs, (0, 1))
    model.train(start_training)
    np.random.seed(123)
    rng = np.random.get_state()
    model.class_activation(gs, (0, 1), kind=kind)
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
    assert torch.equal(model.saliency(gs, (0, 1)), sal_before)


@pytest.mark.parametrize("kind", ["activation", "gradient"])
def test_nan_stays_in_its_graph(kind):
    model = model_of(3, 2, 7, 64, True, "sum", "sum", seed=12)
    gs = [random_graph(150 + i, 40, 0.2, 7) for i in range(3)]
    clean = model.class_activation(gs, (0, 1), kind=kind)
    gs[1].node_features = gs[1].node_features.clone()
    gs[1].node_features[5, 2] = float("nan")
    model._arena = None                                   # the arena caches a graph's features once per arena
    got = model.class_activation(gs, (0, 1), kind=kind)
    for c in (0, 1):
        assert torch.equal(got[c, 0], clean[c, 0]) and torch.equal(got[c, 2], clean[c, 2])
        if kind == "gradient":
            assert torch.isnan(got[c, 1]).all()
