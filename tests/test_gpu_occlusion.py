"""GIN_InfoMaxReg.occlusion() (csrc/occlusion.hip): the class scores of every node-deleted copy of a graph, computed on
virtual graphs, against three anchors -- the real reference's goldens (tests/golden/occlusion/), the route without the
method (model.predict() on explicit copies made by tests/test_occlusion_host.py delete_node) and the fp64 oracle on the
same copies; delta's definition, batch-size invariance, determinism, side effects (none), NaN confinement and the
declined shapes.

Accuracy is asserted on `occluded` and `base` (delta is a difference of two nearly equal numbers), as helpers.rel_err:
max-norm relative to the graph's max |score|, NaN patterns equal.  Small cases (L <= 5, n <= 64): the flat RTOL = 1e-5.
n = 400, L = 5: helpers.Calibrated, max(RTOL, TRUE_SHAPE_FACTOR x err) with err the error of the independent fp32 CPU
forward oracle.gin_torch_cpu.TorchCpuGIN against the fp64 oracle ON THE SAME DELETED GRAPHS -- never a HIP output.
Worst values measured on an MI355X (also in DESIGN.md section 3.12): goldens 6.9e-7; the small-graph matrix 6.5e-6
(H = 32, m = 2); n = 400 at F0 = 7: base 2.3e-6, occluded 3.5e-6 under a bound of 3.3e-5 (the fp32 CPU forward itself:
8.3e-6); n = 400 one-hot: base 1.9e-7, occluded 6.6e-7 under 1e-5."""
import numpy as np
import pytest
import torch

from helpers import RTOL, Calibrated, rel_err
from test_gpu_saliency import model_of, random_graph
from test_occlusion_host import OCC_CASES, delete_node, load_occ_case, occ_graphs, oracle_scores

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
POOLS = [(np_, gp, le) for np_ in ("sum", "average") for gp in ("sum", "average") for le in (True, False)]


def state64(model):
    return {k: v.detach().cpu().numpy().astype(np.float64) if v.dtype.is_floating_point else v.cpu().numpy()
            for k, v in model.state_dict().items()}


def spec_of(model):
    return (model.num_layers, model.num_mlp_layers, model.learn_eps, model.graph_pooling_type,
            model.neighbor_pooling_type)


def run(model, graphs, classes=(0, 1), **kw):
    """(delta, base [C, G] numpy, occluded: per graph [n_g, C] numpy) with delta = base - occluded checked bitwise"""
    delta, base, occ = model.occlusion(graphs, tuple(classes), return_scores=True, **kw)
    assert base.shape == (len(classes), len(graphs)) and base.dtype == torch.float32
    if torch.is_tensor(occ):
        assert occ.shape == (len(classes), len(graphs), len(graphs[0].g)) and occ.dtype == torch.float32
        assert torch.equal(torch.nan_to_num(delta, nan=7.0), torch.nan_to_num(base.unsqueeze(-1) - occ, nan=7.0))
        per = [occ[:, g].t().cpu().numpy() for g in range(len(graphs))]
    else:
        for ci in range(len(classes)):
            for g in range(len(graphs)):
                assert occ[ci][g].shape == (len(graphs[g].g),)
                assert torch.equal(torch.nan_to_num(delta[ci][g], nan=7.0),
                                   torch.nan_to_num(base[ci, g] - occ[ci][g], nan=7.0))
        per = [torch.stack([occ[ci][g] for ci in range(len(classes))], 1).cpu().numpy() for g in range(len(graphs))]
    return delta, base.cpu().numpy(), per


def check(got, ref, classes=(0, 1), rtol=RTOL):
    """base and occluded of run() against (base [G, C], occluded per graph [n_g, C]); returns the worst error"""
    _, base, per = got
    rbase, rocc = ref
    worst = 0.0
    for g in range(len(per)):
        scale = float(np.abs(rbase[g]).max())
        e1 = rel_err(base[:, g], np.asarray(rbase[g])[list(classes)])
        r = np.asarray(rocc[g])[:, list(classes)]
        if np.isnan(r).all():                                    # (rel_err has no entry to take a maximum over)
            assert np.isnan(per[g]).all() and per[g].shape == r.shape
            e2 = 0.0
        else:
            e2 = rel_err(per[g], r, floor=scale)
        assert e1 <= rtol and e2 <= rtol, "graph %d: base %.3e occluded %.3e > %.1e" % (g, e1, e2, rtol)
        worst = max(worst, e1, e2)
    return worst


def predict_scores(model, graphs):
    """the route without the method: predict() on the graphs and on explicit node-deleted copies (graphs of one size)"""
    base = model.predict(graphs).cpu().numpy()
    copies = [delete_node(g, v) for g in graphs for v in range(len(g.g))]
    pred = model.predict(copies).cpu().numpy()
    n = len(graphs[0].g)
    return base, [pred[g * n:(g + 1) * n] for g in range(len(graphs))]


# ---------------------------------------------------------------------------------------------- parity
@pytest.mark.parametrize("case", OCC_CASES)
def test_against_reference_goldens(case):
    from models.graphcnn import GIN_InfoMaxReg
    cfg, state, d = load_occ_case(case)
    model = GIN_InfoMaxReg(cfg["L"], cfg["m"], cfg["f0"], cfg["H"], cfg["C"], 0.0, cfg["learn_eps"], cfg["gpool"],
                           cfg["npool"], torch.device(DEV)).to(DEV)
    missing, unexpected = model.load_state_dict({k: torch.as_tensor(v) for k, v in state.items()}, strict=False)
    assert not unexpected and all(k.startswith("disc.") for k in missing)
    graphs = occ_graphs(cfg, d)
    got = run(model, graphs)
    golden = (np.stack([d[f"base_{g}"] for g in range(cfg["B"])]), [d[f"occluded_{g}"] for g in range(cfg["B"])])
    worst = check(got, golden)                                   # (the hub case: NaN exactly where the reference has it)
    worst = max(worst, check(got, oracle_scores(state64(model), spec_of(model), graphs)))
    if "hub" in case:
        assert all(np.isnan(p[0]).all() and np.isfinite(p[1:]).all() for p in got[2])
    print("worst rel err %s: %.2e" % (case, worst))


@pytest.mark.parametrize("m", [1, 2, 3])
@pytest.mark.parametrize("H", [32, 64, 128])
def test_small_graphs_three_anchors(H, m):
    """40-node graphs (two row blocks; one asymmetric) in batches of 2 and tiny 6-node graphs, F0 = 7, every pooling
    form: against the fp64 oracle and against predict() on explicit copies"""
    worst = 0.0
    for npool, gpool, le in POOLS:
        model = model_of(3, m, 7, H, le, gpool, npool, seed=H + m)
        for gs, bs in (([random_graph(10 + i, 40, 0.2, 7, directed=(i == 1)) for i in range(3)], 2),
                       ([random_graph(50 + i, 6, 0.6, 7) for i in range(2)], 8)):
            ref = oracle_scores(state64(model), spec_of(model), gs)
            assert all(np.isfinite(o).all() for o in ref[1])          # nothing is silently excluded
            got = run(model, gs, batch_size=bs)
            worst = max(worst, check(got, ref), check(got, predict_scores(model, gs)))
    print("worst rel err H=%d m=%d: %.2e" % (H, m, worst))


def test_ragged_batches_return_lists():
    model = model_of(3, 2, 7, 64, True, "average", "average", seed=4)
    gs = [random_graph(90 + i, n, 0.3, 7) for i, n in enumerate((20, 33, 64, 7, 2))]
    ref = oracle_scores(state64(model), spec_of(model), gs)
    got = run(model, gs, batch_size=3)
    delta = got[0]
    assert isinstance(delta, list) and [x.shape[0] for x in delta[0]] == [20, 33, 64, 7, 2]
    check(got, ref)                                              # (NaN where a deleted copy has a 0/0 row, as the oracle)
    one = model.occlusion(gs, 1, batch_size=3)
    assert isinstance(one, list) and all(torch.equal(torch.nan_to_num(a), torch.nan_to_num(b))
                                         for a, b in zip(one, delta[1]))
    d1, b1, o1 = model.occlusion(gs[:1], 0, return_scores=True)
    assert d1.shape == (1, 20) and b1.shape == (1,) and o1.shape == (1, 20)


@pytest.mark.parametrize("tag,one_hot,npool,gpool,learn_eps", [("f7_gaverage_naverage_eps1", False, "average", "average", True),
                                                               ("onehot_gsum_nsum_eps1", True, "sum", "sum", True)])
def test_400_node_dense(tag, one_hot, npool, gpool, learn_eps):
    """the reference's shape: a 400-node dense connectivity graph, L = 5, H = 64, F0 = 7 and one-hot 400 (main.py's
    default input feature), all 400 deleted copies, under the calibrated bound of the file header.  The two CPU
    references of the 400 copies (two minutes of CPU time) are stored by tests/golden/make_occlusion_true_shape.py;
    the fingerprint ties them to this test's model."""
    import os
    from gnm import synth
    from helpers import GOLDEN_DIR
    ref = dict(np.load(os.path.join(GOLDEN_DIR, "occlusion", "true_n400_%s.npz" % tag)))
    g = synth.dense_fc_graph(0, n=400)
    if one_hot:
        g.node_features = torch.eye(400)
    deg = np.bincount(g.edge_mat.numpy()[0], minlength=400)
    assert deg.min() >= 2                                        # no deleted copy has a 0/0 row: no NaN in the reference
    assert np.isfinite(ref["occluded64"]).all() and np.isfinite(ref["occluded32"]).all()
    model = model_of(5, 2, 400 if one_hot else 7, 64, learn_eps, gpool, npool, seed=7)
    st = state64(model)
    fp = np.array([[st[k].astype(np.float64).sum(), np.abs(st[k].astype(np.float64)).sum()] for k in sorted(st)])
    assert np.array_equal(fp, ref["fingerprint"]), "the stored references belong to another model"
    got = run(model, [g])
    cal = Calibrated()
    scale = float(np.abs(ref["base64"]).max())
    cal.check(got[1][:, 0], ref["base32"], ref["base64"], "base")
    cal.check(got[2][0], ref["occluded32"], ref["occluded64"], "occluded", floor=scale)
    print("400-node %s: %s" % (tag, [(w, "%.2e" % e, "%.2e" % r, "%.2e" % b_) for w, e, r, b_ in cal.log]))


# ---------------------------------------------------------------------------------------------- behaviour
def test_batch_size_invariance_and_determinism(monkeypatch):
    from gnm import attribution
    model = model_of(3, 2, 7, 64, True, "average", "average", seed=2)
    gs = [random_graph(20 + i, 40, 0.2, 7) for i in range(5)]
    d0, b0, o0 = model.occlusion(gs, (0, 1), return_scores=True)
    assert torch.isfinite(o0).all()
    for bs in (1, 2, 5, 256):
        d, b, o = model.occlusion(gs, (0, 1), batch_size=bs, return_scores=True)
        assert torch.equal(d, d0) and torch.equal(b, b0) and torch.equal(o, o0), bs      # (256 again: run to run)
    from gnm._cabi import lib
    monkeypatch.setattr(attribution, "OCCLUSION_SCRATCH_BYTES", 4 * int(lib.gnm_occlusion_scratch_floats(2 * 1600, 80, 40, 64, 3)))
    #                                                             (the scratch of two graphs: chunks of 2, 2 and 1)
    d, b, o = model.occlusion(gs, (0, 1), batch_size=256, return_scores=True)
    assert torch.equal(d, d0) and torch.equal(b, b0) and torch.equal(o, o0)
    assert torch.equal(model.occlusion(gs, 1), d0[1]) and torch.equal(model.occlusion(gs, (1, 0)), d0.flip(0))


@pytest.mark.parametrize("training", [True, False])
def test_no_side_effects(training):
    model = model_of(3, 2, 7, 64, True, "sum", "average", seed=3)
    model.train(training)
    gs = [random_graph(30 + i, 40, 0.2, 7) for i in range(2)]
    before = {k: v.clone() for k, v in model.state_dict().items()}
    np.random.seed(11)
    rng = np.random.get_state()
    out = model.occlusion(gs, 0)
    assert out.shape == (2, 40) and out.device.type == "cuda" and not out.requires_grad
    assert model.training == training
    assert all(p.grad is None for p in model.parameters())
    after = model.state_dict()
    assert all(torch.equal(before[k], after[k]) for k in before)
    now = np.random.get_state()
    assert rng[0] == now[0] and np.array_equal(rng[1], now[1]) and rng[2:] == now[2:]


def test_nan_feature_stays_in_its_graph():
    model = model_of(3, 2, 7, 64, False, "average", "sum", seed=5)
    gs = [random_graph(40 + i, 40, 0.2, 7) for i in range(3)]
    clean = model.occlusion([gs[0], gs[2]], (0, 1))
    gs[1].node_features[3, 2] = float("nan")
    got = model.occlusion(gs, (0, 1))
    assert torch.isnan(got[:, 1]).all()
    assert torch.equal(got[:, 0], clean[:, 0]) and torch.equal(got[:, 2], clean[:, 1])


def test_declined_shapes_raise_with_their_reason():
    gs = [random_graph(60 + i, 40, 0.2, 7) for i in range(2)]
    nb = model_of(2, 2, 7, 64, True, "sum", "max", seed=1)
    with pytest.raises(ValueError, match="max neighbour pooling"):
        nb.occlusion(gs, 0)
    model = model_of(2, 2, 7, 64, True, "sum", "sum", seed=1)
    with pytest.raises(ValueError, match="416"):
        model.occlusion([random_graph(70, 420, 0.05, 7)], 0)
    with pytest.raises(ValueError, match="hidden_dim 16"):
        model_of(2, 2, 7, 16, True, "sum", "sum", seed=1).occlusion(gs, 0)
    with pytest.raises(ValueError, match="num_mlp_layers"):
        model_of(2, 4, 7, 64, True, "sum", "sum", seed=1).occlusion(gs, 0)
    model._spec.sync_bn = object()
    with pytest.raises(ValueError, match="synchronised BatchNorm"):
        model.occlusion(gs, 0)
    model._spec.sync_bn = None
    with pytest.raises(ValueError, match="fewer than 2 nodes"):
        model.occlusion(gs + [random_graph(71, 1, 0.5, 7)], 0)
    assert model.occlusion(gs, 0).shape == (2, 40)               # and the model still works
