"""GIN_InfoMaxReg.integrated_gradients() (csrc/intgrad.hip over csrc/saliency.hip's layer launches): the attribution
computed on virtual (graph, step) copies against the fp64 oracle on explicit rescaled copies (tests/test_intgrad_host.py
oracle_ig) -- on the sources of the real reference's goldens (tests/golden/intgrad/), across the small-shape matrix and
at the reference's 400-node shape; the tie to gnm_saliency, completeness, and the method's behaviour (layouts,
determinism, NaN confinement, no side effects, declined shapes).

Every comparison is in max-norm relative to the case's max |attr| (helpers.rel_err).  Small cases: the flat bound 1e-5,
the project's bound for saliency() under the same measure.  n = 400, L = 5: max(1e-5, 4 x the distance of the
independent fp32 CPU restatement from the fp64 oracle), stored by tests/golden/make_intgrad_goldens.py --true-shape --
never a HIP output."""
import os

import numpy as np
import pytest
import torch

from helpers import GOLDEN_DIR, RTOL, TRUE_SHAPE_FACTOR, rel_err
from test_gpu_occlusion import spec_of, state64
from test_gpu_saliency import POOLS, model_of, random_graph
from test_intgrad_host import IG_CASES, METHODS, load_ig_case, oracle_ig, quadrature

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def oracle_of(model, graphs, classes, alphas, weights, baseline=None):
    """per graph (attr [C, n, F0], base [C], base0 [C]) through the fp64 oracle"""
    st, sp = state64(model), spec_of(model)
    return [oracle_ig(st, sp, g, classes, alphas, weights, baseline) for g in graphs]


def worst_err(got, ref):
    """got: the method's result for a sequence `cls` ([C, G, n, F0] or per-class lists of per-graph tensors); ref:
    oracle_of's.  The worst rel_err over the graphs, each relative to its own max |attr| over the classes."""
    worst = 0.0
    for g, (attr, _, _) in enumerate(ref):
        mine = np.stack([(got[ci][g]).cpu().numpy() for ci in range(len(attr))])
        assert mine.shape == attr.shape and mine.dtype == np.float32
        assert np.abs(attr).max() > 0
        worst = max(worst, rel_err(mine, attr))
    return worst


def baseline_of(n, f0, seed=5):
    return (0.5 * np.random.default_rng(seed).standard_normal((n, f0))).astype(np.float32)


# ---------------------------------------------------------------------------------------------- parity
@pytest.mark.parametrize("case", IG_CASES)
def test_against_golden_sources(case):
    from models.graphcnn import GIN_InfoMaxReg
    cfg, state, graphs, d = load_ig_case(case)
    model = GIN_InfoMaxReg(cfg["L"], cfg["m"], cfg["f0"], cfg["H"], cfg["C"], 0.0, cfg["learn_eps"], cfg["gpool"],
                           cfg["npool"], torch.device(DEV)).to(DEV)
    missing, unexpected = model.load_state_dict({k: torch.as_tensor(v) for k, v in state.items()}, strict=False)
    assert not unexpected and all(k.startswith("disc.") for k in missing)
    worst = 0.0
    for K in (1, 5):
        got = model.integrated_gradients(graphs, (0, 1), steps=K, baseline=d.get("baseline"))
        assert got.shape == (2, cfg["B"], cfg["n"], cfg["f0"]) and got.dtype == torch.float32
        for g in range(cfg["B"]):
            e = rel_err(got[:, g].cpu().numpy(), d[f"oracle_{K}_{g}"])
            print("%s K=%d graph %d: %.2e" % (case, K, g, e))
            worst = max(worst, e)
    assert worst <= RTOL, worst


@pytest.mark.parametrize("m", [1, 2, 3])
@pytest.mark.parametrize("H", [32, 64, 128])
def test_small_shape_matrix(H, m):
    """every pooling form at this (H, m), the other axes cycled so that each value meets each (H, m): L in {1, 3},
    n in {7, 33, 70} (a sub-block graph, a partial second 32-row block, a third block), B in {1, 3}, K in {1, 2, 5},
    the three rules, zero and non-zero baselines, F0 = 3 and one-hot"""
    worst = 0.0
    hi = (32, 64, 128).index(H)
    for i, (npool, gpool, le) in enumerate(POOLS):
        L = (1, 3)[i % 2]
        n = (7, 33, 70)[(i + hi + m) % 3]
        B = (1, 3)[(i // 2 + m) % 2]
        method = METHODS[(i + hi) % 3]
        K = max((1, 2, 5)[(i + m) % 3], 2 if method == "trapezoid" else 1)
        one_hot = (i + hi + m) % 4 == 0
        f0 = n if one_hot else 3
        base = baseline_of(n, f0, seed=i) if (i // 4 + hi + m) % 2 else None
        model = model_of(L, m, f0, H, le, gpool, npool, seed=H + m + i)
        gs = [random_graph(100 * i + j, n, 0.3, f0, one_hot=one_hot) for j in range(B)]
        alphas, weights = quadrature(method, K)
        got = model.integrated_gradients(gs, (0, 1), steps=K, baseline=base, method=method)
        assert got.shape == (2, B, n, f0)
        e = worst_err(got, oracle_of(model, gs, (0, 1), alphas, weights, base))
        print("H=%d m=%d %s/%s/eps%d L=%d n=%d B=%d K=%d %s onehot=%d base=%d: %.2e"
              % (H, m, npool, gpool, le, L, n, B, K, method, one_hot, base is not None, e))
        worst = max(worst, e)
    assert worst <= RTOL, worst


def test_32_steps_asymmetric_and_ragged():
    """K = 32 (the default), one asymmetric graph (the transposed bits), and a ragged batch (list output)"""
    model = model_of(3, 2, 3, 64, True, "average", "average", seed=11)
    gs = [random_graph(200, 33, 0.3, 3), random_graph(201, 33, 0.3, 3, directed=True)]
    em = gs[1].edge_mat.numpy()
    assert set(map(tuple, em.T)) != set(map(tuple, em[::-1].T))
    got = model.integrated_gradients(gs, (0, 1))
    e = worst_err(got, oracle_of(model, gs, (0, 1), *quadrature("midpoint", 32)))
    print("K=32 with an asymmetric graph: %.2e" % e)
    assert e <= RTOL
    rg = [random_graph(210, 7, 0.5, 3), random_graph(211, 33, 0.3, 3)]
    got = model.integrated_gradients(rg, (0, 1), steps=5, method="gausslegendre")
    assert isinstance(got, list) and [x.shape for x in got[0]] == [(7, 3), (33, 3)]
    e = worst_err(got, oracle_of(model, rg, (0, 1), *quadrature("gausslegendre", 5)))
    print("ragged: %.2e" % e)
    assert e <= RTOL
    one = model.integrated_gradients(rg, 1, steps=5, method="gausslegendre")
    assert isinstance(one, list) and all(torch.equal(a, b) for a, b in zip(one, got[1]))
    with pytest.raises(ValueError, match="one node count"):
        model.integrated_gradients(rg, 0, baseline=np.zeros((7, 3), dtype=np.float32))


@pytest.mark.parametrize("npool,gpool,le", [POOLS[0], POOLS[7]])
def test_one_step_at_the_input_is_saliency_times_x(npool, gpool, le):
    """the driver with alphas = [1], weights = [1] and a zero baseline against gnm_saliency: saliency_hip(X) * X.  Not
    bitwise: layer 0 takes another route (alpha P + b instead of the Linear of the aggregate)."""
    from gnm.attribution import integrated_gradients_hip, saliency_hip
    model = model_of(3, 2, 7, 64, le, gpool, npool, seed=3).eval()
    gs = [random_graph(220 + j, 40, 0.2, 7) for j in range(2)]
    batch = model._batch_of(gs)
    X = batch.arena.features(batch).detach()
    names, tensors, buffers = model._param_lists()
    P = dict(zip(names, tensors))
    P.update(buffers)
    sal = torch.stack(saliency_hip(model._spec, batch, X, P, (0, 1))) * X
    got = integrated_gradients_hip(model._spec, batch, X, P, (0, 1), [1.0], [1.0])
    e = rel_err(got.cpu().numpy(), sal.cpu().numpy())
    print("against saliency_hip * X: %.2e" % e)
    assert e <= RTOL


class _Copy:
    pass


def with_features(graph, feats):
    c = _Copy()
    c.g, c.edge_mat, c.label, c.node_features = graph.g, graph.edge_mat, getattr(graph, "label", 0), feats
    return c


@pytest.mark.parametrize("npool,gpool,le", POOLS)
def test_completeness_on_the_device(npool, gpool, le):
    """delta against the fp64 oracle's residual at the same K, relative to max |score|; base and base0 are predict()'s
    logits, bitwise (F0 = 3: every eval forward of these graphs takes the evaluation encoder)"""
    model = model_of(3, 2, 3, 64, le, gpool, npool, seed=21)
    gs = [random_graph(230 + j, 33, 0.3, 3) for j in range(3)]
    base_x = baseline_of(33, 3)
    for bl in (None, base_x):
        attr, base, base0, delta = model.integrated_gradients(gs, (0, 1), steps=5, baseline=bl, return_scores=True)
        assert base.shape == base0.shape == delta.shape == (2, 3) and delta.dtype == torch.float32
        assert torch.equal(delta, attr.sum((-2, -1)) - (base - base0))
        ref = oracle_of(model, gs, (0, 1), *quadrature("midpoint", 5), bl)
        for g, (a64, b64, b064) in enumerate(ref):
            scale = max(np.abs(b64).max(), np.abs(b064).max())
            want = a64.sum((-2, -1)) - (b64 - b064)
            err = np.abs(delta[:, g].cpu().numpy() - want).max() / scale
            print("%s/%s/eps%d baseline=%d graph %d: delta %s (oracle %s), off by %.2e" %
                  (npool, gpool, le, bl is not None, g, delta[:, g].tolist(), want.tolist(), err))
            assert err <= RTOL
        zero = torch.zeros(33, 3) if bl is None else torch.from_numpy(bl)
        assert torch.equal(base, model.predict(gs)[:, [0, 1]].t())
        assert torch.equal(base0, model.predict([with_features(g, zero) for g in gs])[:, [0, 1]].t())
    a1, b1, b01, d1 = model.integrated_gradients(gs, 1, steps=5, baseline=base_x, return_scores=True)
    assert torch.equal(a1, attr[1]) and torch.equal(b1, base[1]) and torch.equal(b01, base0[1]) and torch.equal(d1, delta[1])


# ---------------------------------------------------------------------------------------------- the reference's shape
@pytest.mark.parametrize("tag,one_hot,npool,gpool,learn_eps", [("f7_gaverage_naverage_eps1", False, "average", "average", True),
                                                               ("onehot_gsum_nsum_eps1", True, "sum", "sum", True)])
def test_400_node_dense(tag, one_hot, npool, gpool, learn_eps):
    """a 400-node dense connectivity graph, L = 5, H = 64, K = 8, F0 = 7 and one-hot 400: against the stored fp64 oracle
    attribution under max(1e-5, 4 x the fp32 CPU restatement's own distance).  Measured on an MI355X: see DESIGN.md
    section 3.13."""
    from gnm import synth
    ref = dict(np.load(os.path.join(GOLDEN_DIR, "intgrad", "true_n400_%s.npz" % tag)))
    g = synth.dense_fc_graph(0, n=400)
    if one_hot:
        g.node_features = torch.eye(400)
    model = model_of(5, 2, 400 if one_hot else 7, 64, learn_eps, gpool, npool, seed=7)
    st = state64(model)
    fp = np.array([[st[k].astype(np.float64).sum(), np.abs(st[k].astype(np.float64)).sum()] for k in sorted(st)])
    assert np.array_equal(fp, ref["fingerprint"]), "the stored references belong to another model"
    got = model.integrated_gradients([g], (0, 1), steps=8)[:, 0].cpu().numpy()
    a64 = ref["attr64"]
    if one_hot:                                                  # stored as its diagonal: the rest is exactly zero
        full = np.zeros((2, 400, 400))
        full[:, np.arange(400), np.arange(400)] = a64
        a64 = full
    bound = max(RTOL, TRUE_SHAPE_FACTOR * float(ref["dist32"]))
    e = rel_err(got, a64)
    print("400-node %s: device %.2e, fp32 CPU restatement %.2e, bound %.2e" % (tag, e, float(ref["dist32"]), bound))
    assert e <= bound


# ---------------------------------------------------------------------------------------------- behaviour
def test_classes_determinism_and_batch_size(monkeypatch):
    from gnm import attribution
    model = model_of(3, 2, 7, 64, True, "average", "average", seed=2)
    gs = [random_graph(240 + j, 40, 0.2, 7) for j in range(3)]
    base = baseline_of(40, 7)
    a0 = model.integrated_gradients(gs, (0, 1), steps=5, baseline=base)
    assert torch.isfinite(a0).all()
    assert torch.equal(model.integrated_gradients(gs, (0, 1), steps=5, baseline=base), a0)          # run to run
    assert torch.equal(model.integrated_gradients(gs, 0, steps=5, baseline=base), a0[0])            # multi-class
    assert torch.equal(model.integrated_gradients(gs, 1, steps=5, baseline=base), a0[1])
    assert torch.equal(model.integrated_gradients(gs, (1, 0), steps=5, baseline=base), a0.flip(0))
    a1 = model.integrated_gradients(gs, (0, 1), steps=5, baseline=base, batch_size=1)
    a3 = model.integrated_gradients(gs, (0, 1), steps=5, baseline=base, batch_size=3)
    scale = float(a0.abs().max())
    assert float((a1 - a3).abs().max()) <= RTOL * scale
    # the driver's chunks: room for two graphs' arrays -> chunks of 2 and 1 graphs, never a part of one graph's steps
    monkeypatch.setattr(attribution, "INTGRAD_SCRATCH_BYTES", 4 * attribution._intgrad_floats(80, 64, 3, 2, 5))
    ac = model.integrated_gradients(gs, (0, 1), steps=5, baseline=base)
    assert float((ac - a0).abs().max()) <= RTOL * scale
    monkeypatch.setattr(attribution, "INTGRAD_SCRATCH_BYTES", 1)
    ac = model.integrated_gradients(gs, (0, 1), steps=5, baseline=base)                             # one graph a chunk
    assert float((ac - a0).abs().max()) <= RTOL * scale


@pytest.mark.parametrize("training", [True, False])
def test_no_side_effects(training):
    model = model_of(3, 2, 7, 64, True, "sum", "average", seed=3)
    model.train(training)
    gs = [random_graph(250 + j, 40, 0.2, 7) for j in range(2)]
    before = {k: v.clone() for k, v in model.state_dict().items()}
    np.random.seed(11)
    rng = np.random.get_state()
    out = model.integrated_gradients(gs, 0, steps=3, return_scores=True)
    assert out[0].shape == (2, 40, 7) and out[0].device.type == "cuda" and not out[0].requires_grad
    assert model.training == training
    assert all(p.grad is None for p in model.parameters())
    after = model.state_dict()
    assert all(torch.equal(before[k], after[k]) for k in before)
    now = np.random.get_state()
    assert rng[0] == now[0] and np.array_equal(rng[1], now[1]) and rng[2:] == now[2:]


def test_nan_feature_stays_in_its_graph():
    model = model_of(3, 2, 7, 64, False, "average", "sum", seed=5)
    gs = [random_graph(260 + j, 40, 0.2, 7) for j in range(3)]
    clean = model.integrated_gradients([gs[0], gs[2]], (0, 1), steps=3)
    gs[1].node_features[3, 2] = float("nan")
    got = model.integrated_gradients(gs, (0, 1), steps=3)
    assert torch.isnan(got[:, 1]).all()
    assert torch.equal(got[:, 0], clean[:, 0]) and torch.equal(got[:, 2], clean[:, 1])


def test_declined_shapes_raise_with_their_reason():
    gs = [random_graph(270 + j, 40, 0.2, 7) for j in range(2)]
    with pytest.raises(ValueError, match="max neighbour pooling"):
        model_of(2, 2, 7, 64, True, "sum", "max", seed=1).integrated_gradients(gs, 0)
    model = model_of(2, 2, 7, 64, True, "sum", "sum", seed=1)
    with pytest.raises(ValueError, match="without a bit adjacency"):
        model.integrated_gradients([random_graph(280, 420, 0.05, 7)], 0)
    with pytest.raises(ValueError, match="hidden_dim 48"):
        model_of(2, 2, 7, 48, True, "sum", "sum", seed=1).integrated_gradients(gs, 0)
    with pytest.raises(ValueError, match="isolated node"):
        model_of(2, 2, 7, 64, True, "sum", "average", seed=1).integrated_gradients(
            [random_graph(281, 40, 0.2, 7, iso=1)], 0)
    assert model.integrated_gradients(gs, 0, steps=2).shape == (2, 40, 7)      # and the model still works
