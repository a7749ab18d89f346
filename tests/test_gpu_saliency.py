"""GIN_InfoMaxReg.saliency(): the batched eval-mode input gradient (csrc/saliency.hip, or the whole-batch autograd route
for shapes the kernel declines) against the per-graph compute_saliency loop of main.py:60-68, the reference's goldens and
the fp64 oracle; and its side effects (none)."""
import numpy as np
import pytest
import torch

from helpers import RTOL, TRUE_SHAPE_GRAD_RTOL, assert_close, load_case, golden_cases
from test_gpu_model_parity import make_graphs, make_model

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
# max|batched - per graph| / max|per graph| per graph.  Bound 1e-5.  Worst measured over this file's HIP-route cases on
# an MI355X: 1.07e-6 (400-node dense graphs, F0 = 7, neighbour sum / graph average, learn_eps False); the small-graph
# matrix stays below 6.1e-7.  The two sides differ in summation order only.
SAL_RTOL = 1e-5


class Graph:
    """S2VGraph-shaped (util.py:9-17) graph from DIRECTED edges as they are (edge_mat is used as given)."""

    def __init__(self, n, src, dst, feats, label=0):
        self.g = list(range(n))
        self.label = label
        self.edge_mat = torch.as_tensor(np.stack([np.asarray(src, np.int64), np.asarray(dst, np.int64)]))
        self.node_features = torch.as_tensor(np.asarray(feats, np.float32))
        nb = [[] for _ in range(n)]
        for a, b in zip(src, dst):
            nb[a].append(int(b))
        self.neighbors = nb
        self.max_neighbor = max(len(x) for x in nb)


def random_graph(seed, n, p, f0, iso=0, directed=False, one_hot=False):
    """random graph with a ring i -> i + 1 (so no node lacks neighbours), then `iso` nodes cut loose"""
    rng = np.random.default_rng(seed)
    A = rng.random((n, n)) < p
    A[np.arange(n), (np.arange(n) + 1) % n] = True
    np.fill_diagonal(A, False)
    if not directed:
        A = np.triu(A, 1)
        A = A | A.T
    if iso:
        A[:iso, :] = False
        A[:, :iso] = False
    src, dst = np.nonzero(A)
    feats = np.eye(n, dtype=np.float32) if one_hot else rng.standard_normal((n, f0)).astype(np.float32)
    return Graph(n, src, dst, feats, int(rng.integers(0, 2)))


def model_of(L, m, f0, H, learn_eps, gpool, npool, seed=0, C=2):
    from models.graphcnn import GIN_InfoMaxReg
    torch.manual_seed(seed)
    model = GIN_InfoMaxReg(L, m, f0, H, C, 0.5, learn_eps, gpool, npool, torch.device(DEV)).to(DEV)
    with torch.no_grad():                       # running statistics and affines away from their defaults
        g = torch.Generator().manual_seed(seed + 1)
        for name, b in model.named_buffers():
            if name.endswith("running_mean"):
                b.copy_(0.1 * torch.randn(b.shape, generator=g).to(DEV))
            elif name.endswith("running_var"):
                b.copy_(0.5 + torch.rand(b.shape, generator=g).to(DEV))
        for name, p in model.named_parameters():
            if "batch_norms" in name:
                p.add_(0.1 * torch.randn(p.shape, generator=g).to(DEV))
        if learn_eps:
            model.eps.copy_(0.2 * torch.randn(L, generator=g).to(DEV))
    return model


def per_graph(model, graphs, cls):
    return [model.compute_saliency([g], cls).detach().clone() for g in graphs]


def check_against_loop(model, graphs, classes=(0, 1), batch_size=256):
    sal = model.saliency(graphs, tuple(classes), batch_size=batch_size)
    worst = 0.0
    for ci, c in enumerate(classes):
        ref = per_graph(model, graphs, c)
        for i, r in enumerate(ref):
            got = sal[ci][i]
            assert got.shape == r.shape
            scale = float(r.abs().max())
            err = float((got - r).abs().max())
            assert err <= SAL_RTOL * scale, "graph %d class %d: max|d| %.3e vs max|ref| %.3e" % (i, c, err, scale)
            worst = max(worst, err / scale if scale > 0 else 0.0)
    return sal, worst


POOLS = [(np_, gp, le) for np_ in ("sum", "average") for gp in ("sum", "average") for le in (True, False)]


@pytest.mark.parametrize("npool,gpool,learn_eps", POOLS)
@pytest.mark.parametrize("m", [1, 2, 3])
@pytest.mark.parametrize("H", [32, 64, 128])
def test_batched_equals_per_graph_small(npool, gpool, learn_eps, m, H):
    """40-node graphs (one of them asymmetric) and tiny 6-node graphs (B > n), F0 = 7, batches of 3 over 5 graphs."""
    model = model_of(3, m, 7, H, learn_eps, gpool, npool, seed=H + m)
    gs = [random_graph(10 + i, 40, 0.2, 7, directed=(i == 2)) for i in range(5)]
    _, w1 = check_against_loop(model, gs, batch_size=3)
    assert model.saliency_routes == ["hip", "hip"]
    tiny = [random_graph(50 + i, 6, 0.4, 7) for i in range(10)]
    _, w2 = check_against_loop(model, tiny)
    assert model.saliency_routes == ["hip"]
    print("worst rel err", npool, gpool, learn_eps, m, H, max(w1, w2))


@pytest.mark.parametrize("npool,gpool,learn_eps", POOLS)
def test_isolated_nodes(npool, gpool, learn_eps):
    """graphs with nodes that have no neighbours: the HIP route, except neighbour "average" + learn_eps, whose 0/0 rows
    (graphcnn.py:157-158) take the autograd route with its NaN semantics."""
    model = model_of(2, 2, 7, 64, learn_eps, gpool, npool, seed=3)
    gs = [random_graph(70 + i, 30, 0.2, 7, iso=3) for i in range(4)]
    sal = model.saliency(gs, (0, 1))
    expect = "autograd" if (npool == "average" and learn_eps) else "hip"
    assert model.saliency_routes == [expect]
    for ci in (0, 1):
        ref = per_graph(model, gs, ci)
        for i, r in enumerate(ref):
            r, got = r.cpu().numpy(), sal[ci][i].cpu().numpy()
            assert np.array_equal(np.isnan(r), np.isnan(got))
            fin = np.isfinite(r)
            scale = np.abs(r[fin]).max() if fin.any() else 0.0
            assert np.abs(got[fin] - r[fin]).max(initial=0.0) <= SAL_RTOL * scale


@pytest.mark.parametrize("npool,gpool,learn_eps", [("sum", "sum", True), ("average", "average", False),
                                                   ("average", "sum", True), ("sum", "average", False)])
@pytest.mark.parametrize("one_hot", [False, True])
def test_batched_equals_per_graph_400_dense(npool, gpool, learn_eps, one_hot):
    """the reference's shape: 400-node dense connectivity graphs, L = 5, H = 64, F0 = 7 or one_hot 400."""
    from gnm import synth
    gs = [synth.dense_fc_graph(g, n=400) for g in range(3)]
    if one_hot:
        for g in gs:
            g.node_features = torch.eye(400)
    f0 = 400 if one_hot else 7
    model = model_of(5, 2, f0, 64, learn_eps, gpool, npool, seed=7)
    sal, worst = check_against_loop(model, gs, batch_size=2)
    assert model.saliency_routes == ["hip", "hip"]
    assert sal.shape == (2, 3, 400, f0)
    print("worst rel err 400-node", npool, gpool, learn_eps, one_hot, worst)


def test_ragged_node_counts_hip_route_returns_lists():
    model = model_of(3, 2, 7, 64, True, "average", "sum", seed=4)
    gs = [random_graph(90 + i, n, 0.2, 7) for i, n in enumerate((20, 33, 64, 7))]
    sal, _ = check_against_loop(model, gs, batch_size=3)
    assert model.saliency_routes == ["hip", "hip"]
    assert isinstance(sal, list) and len(sal) == 2 and [s.shape[0] for s in sal[0]] == [20, 33, 64, 7]
    one = model.saliency(gs, 1)
    assert isinstance(one, list) and all(torch.equal(a, b) for a, b in zip(one, sal[1]))


@pytest.mark.parametrize("kind", ["max", "knn1000", "H36", "ragged_max"])
def test_fallback_route(kind):
    from gnm import synth
    if kind == "max":
        model = model_of(3, 2, 7, 64, True, "sum", "max", seed=5)
        gs = [random_graph(110 + i, 30, 0.2, 7) for i in range(3)]
    elif kind == "knn1000":
        model = model_of(2, 2, 7, 128, False, "average", "sum", seed=6)
        gs = [synth.knn_graph(g, n=1000) for g in range(2)]
    elif kind == "H36":
        model = model_of(3, 2, 7, 36, True, "sum", "average", seed=8)
        gs = [random_graph(120 + i, 30, 0.2, 7) for i in range(3)]
    else:
        model = model_of(2, 2, 7, 32, False, "average", "max", seed=9)
        gs = [random_graph(130 + i, n, 0.3, 7) for i, n in enumerate((12, 25, 9))]
    sal, worst = check_against_loop(model, gs, batch_size=2)
    assert set(model.saliency_routes) == {"autograd"}
    if kind == "ragged_max":
        assert isinstance(sal, list) and [s.shape[0] for s in sal[0]] == [12, 25, 9]
    else:
        assert sal.shape[:2] == (2, len(gs))


@pytest.mark.parametrize("case", [c for c in golden_cases() if c.startswith("tiny_")])
def test_saliency_vs_reference_golden(case):
    cfg, state, d = load_case(case)
    model = make_model(cfg, state)
    graphs = make_graphs(cfg, d)
    sal = model.saliency(graphs[:1], (0, 1))
    for cls in (0, 1):
        assert_close(sal[cls][0].cpu().numpy(), d[f"saliency_cls{cls}"], rtol=5 * RTOL, what=f"saliency {cls}")


def test_saliency_one_hot_true_shape_vs_fp64_oracle():
    """one_hot F0 = 400 at n = 400 (main.py's default input features): the HIP route against the fp64 oracle at the
    bound test_gpu_model_parity.py uses for compute_saliency."""
    from gnm import synth
    from oracle import gin_oracle as O
    n, L, m, H = 400, 2, 2, 64
    graphs = []
    for g in range(2):
        gr = synth.dense_fc_graph(g, n=n, f0=1)
        gr.node_features = torch.eye(n)
        graphs.append(gr)
    model = model_of(L, m, n, H, True, "sum", "sum", seed=9)
    state = {k: v.detach().cpu().numpy().astype(np.float64) if v.dtype.is_floating_point else v.cpu().numpy()
             for k, v in model.state_dict().items()}
    sal = model.saliency(graphs, 1)
    assert model.saliency_routes == ["hip"]
    for i, gr in enumerate(graphs):
        om = O.OracleGIN(state, L, m, True, "sum", "sum", dtype=np.float64)
        ref = om.compute_saliency(O.OGraph(n, gr.edge_mat.numpy(), gr.node_features.numpy(), gr.label), 1)
        assert_close(sal[i].cpu().numpy(), ref, rtol=TRUE_SHAPE_GRAD_RTOL, what="saliency",
                     floor=1e-2 * np.abs(ref).max())


@pytest.mark.parametrize("start_training", [True, False])
def test_no_side_effects_and_deterministic(start_training):
    model = model_of(3, 2, 7, 64, True, "average", "sum", seed=11)
    gs = [random_graph(140 + i, 40, 0.2, 7) for i in range(4)]
    # some .grad present (and one parameter without), as after a training step
    for i, p in enumerate(model.parameters()):
        if i % 3:
            p.grad = torch.randn_like(p)
    grads = {n: (p.grad.clone() if p.grad is not None else None) for n, p in model.named_parameters()}
    bufs = {n: b.clone() for n, b in model.named_buffers()}
    model.train(start_training)
    np.random.seed(123)
    rng = np.random.get_state()
    a = model.saliency(gs, (0, 1))
    b = model.saliency(gs, (0, 1))
    assert model.saliency_routes == ["hip"]
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
    assert torch.equal(a, b)


def test_nan_stays_in_its_graph():
    model = model_of(3, 2, 7, 64, True, "sum", "sum", seed=12)
    gs = [random_graph(150 + i, 40, 0.2, 7) for i in range(3)]
    clean = model.saliency(gs, (0, 1))
    gs[1].node_features = gs[1].node_features.clone()
    gs[1].node_features[5, 2] = float("nan")
    model._arena = None                                   # the arena caches a graph's features once per arena
    sal = model.saliency(gs, (0, 1))
    assert model.saliency_routes == ["hip", "autograd"]        # the NaN graph on its own, the others on the kernel
    for ci in (0, 1):
        assert torch.equal(sal[ci][0], clean[ci][0]) and torch.equal(sal[ci][2], clean[ci][2])
        ref = model.compute_saliency([gs[1]], ci).cpu().numpy()
        got = sal[ci][1].cpu().numpy()
        assert np.array_equal(np.isnan(ref), np.isnan(got))
        fin = np.isfinite(ref)
        scale = np.abs(ref[fin]).max() if fin.any() else 0.0
        assert np.abs(got[fin] - ref[fin]).max(initial=0.0) <= SAL_RTOL * max(scale, 1e-30)
