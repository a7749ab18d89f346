"""GIN_InfoMaxReg.lesion() / deletion_curve() (csrc/lesion.hip): the class scores of set-deleted copies of a graph,
computed on virtual graphs under a keep mask, against three anchors -- the real reference's goldens
(tests/golden/lesion/), the route without the method (model.predict() on explicit copies made by
tests/test_lesion_host.py delete_nodes) and the fp64 oracle on the same copies; occlusion() on one-node sets; delta's
definition, invariance to the batch size, the chunking and the other sets of the call, side effects (none), NaN
confinement, the declined shapes and the bad masks.

Accuracy is asserted on `lesioned` and `base` (delta is a difference of two nearly equal numbers), as helpers.rel_err:
max-norm relative to the graph's max |score|, NaN patterns equal.  Small cases (L <= 3, n <= 70): the flat RTOL = 1e-5.
n = 400, L = 5: helpers.Calibrated, max(RTOL, TRUE_SHAPE_FACTOR x err) with err the error of the independent fp32 CPU
forward oracle.gin_torch_cpu.TorchCpuGIN against the fp64 oracle ON THE SAME DELETED GRAPHS -- never a HIP output.
Worst values measured on an MI355X (also in DESIGN.md section 3.14): see MEASURED below."""
import numpy as np
import pytest
import torch

from helpers import RTOL, Calibrated, rel_err
from test_gpu_occlusion import spec_of, state64
from test_gpu_saliency import model_of, random_graph
from test_lesion_host import (LES_CASES, delete_nodes, expect_nan, lesion_call, les_graphs, load_les_case,
                              oracle_lesion)

# MEASURED on an MI355X (every test prints its worst error, pytest -s; also in DESIGN.md section 3.14): goldens 2.8e-7;
# the small-shape matrix 2.1e-6 (H = 32, m = 3, L = 1; H = 64 at most 7.1e-7, H = 128 at most 1.2e-6); the empty set
# against predict() 5.5e-7 and one-node sets against occlusion() 8.5e-7; deletion_curve's fraction 0 against base 1.0e-7;
# n = 400 at F0 = 7: base 2.3e-6, lesioned 4.8e-7 under a bound of 1.33e-5 (the fp32 CPU forward itself: 3.3e-6 and
# 8.5e-7); n = 400 one-hot: base 1.9e-7, lesioned 4.6e-7 under 1e-5.  71 to 416 nodes: tests/test_gpu_rowblock_midrange.py.

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
POOLS = [(np_, gp, le) for np_ in ("sum", "average") for gp in ("sum", "average") for le in (True, False)]


def run(model, graphs, sets, classes=(0, 1), **kw):
    """(delta, base [C, G] numpy, lesioned: per graph [S_g, C] numpy) with delta = base - lesioned checked bitwise"""
    delta, base, les = model.lesion(graphs, tuple(classes), sets, return_scores=True, **kw)
    assert base.shape == (len(classes), len(graphs)) and base.dtype == torch.float32
    nn7 = lambda t: torch.nan_to_num(t, nan=7.0)                                   # noqa: E731
    if torch.is_tensor(les):
        assert les.dtype == torch.float32 and les.shape[:2] == (len(classes), len(graphs))
        assert torch.equal(nn7(delta), nn7(base.unsqueeze(-1) - les))
        per = [les[:, g].t().cpu().numpy() for g in range(len(graphs))]
    else:
        for ci in range(len(classes)):
            for g in range(len(graphs)):
                assert torch.equal(nn7(delta[ci][g]), nn7(base[ci, g] - les[ci][g]))
        per = [torch.stack([les[ci][g] for ci in range(len(classes))], 1).cpu().numpy() for g in range(len(graphs))]
    return delta, base.cpu().numpy(), per


def check(got, ref, classes=(0, 1), rtol=RTOL):
    """base and lesioned of run() against (base [G, C], lesioned per graph [S_g, C]); returns the worst error"""
    _, base, per = got
    rbase, rles = ref
    worst = 0.0
    for g in range(len(per)):
        scale = float(np.abs(rbase[g]).max())
        e1 = rel_err(base[:, g], np.asarray(rbase[g])[list(classes)])
        e2 = rel_err(per[g], np.asarray(rles[g])[:, list(classes)], floor=scale)
        assert e1 <= rtol and e2 <= rtol, "graph %d: base %.3e lesioned %.3e > %.1e" % (g, e1, e2, rtol)
        worst = max(worst, e1, e2)
    return worst


def predict_scores(model, graphs, sets):
    """the route without the method: predict() on the graphs and on explicit set-deleted copies (in batches of one
    node count, as predict() asks)"""
    base = np.concatenate([model.predict([g]).cpu().numpy() for g in graphs], 0)
    copies = [(gi, si, delete_nodes(g, D)) for gi, (g, S) in enumerate(zip(graphs, sets)) for si, D in enumerate(S)]
    out = [np.zeros((len(S), base.shape[1])) for S in sets]
    for n in sorted({len(c.g) for _, _, c in copies}):
        grp = [(gi, si, c) for gi, si, c in copies if len(c.g) == n]
        pred = model.predict([c for _, _, c in grp]).cpu().numpy()
        for (gi, si, _), p in zip(grp, pred):
            out[gi][si] = p
    return base, out


def matrix_sets(n, seed):
    """the sets of the small-shape matrix for an n-node graph, bool [S, n]"""
    rng = np.random.default_rng(seed)
    S = [np.zeros(n, dtype=bool)]                                                 # empty
    S.append(np.arange(n) == n // 2)                                              # one node
    S.append(np.arange(n) != 1)                                                   # all but one
    if n > 32:
        S.append(np.arange(n) < 32)                                               # a whole row block
    if n > 64:
        S.append((np.arange(n) >= 32) & (np.arange(n) < 64))
    for a in (7, 15, 63):                                                         # byte, half-row and word edges
        if n > a + 2:
            S.append(np.isin(np.arange(n), (a, a + 1)))
    half = np.zeros(n, dtype=bool)
    half[rng.choice(n, n // 2, replace=False)] = True
    S.append(half)
    return np.stack(S)


# ---------------------------------------------------------------------------------------------- parity
@pytest.mark.parametrize("case", LES_CASES)
def test_against_reference_goldens(case):
    from models.graphcnn import GIN_InfoMaxReg
    cfg, state, d = load_les_case(case)
    model = GIN_InfoMaxReg(cfg["L"], cfg["m"], cfg["f0"], cfg["H"], cfg["C"], 0.0, cfg["learn_eps"], cfg["gpool"],
                           cfg["npool"], torch.device(DEV)).to(DEV)
    missing, unexpected = model.load_state_dict({k: torch.as_tensor(v) for k, v in state.items()}, strict=False)
    assert not unexpected and all(k.startswith("disc.") for k in missing)
    graphs, sets = les_graphs(cfg, d)
    got = run(model, graphs, sets)
    golden = (np.stack([d[f"base_{g}"] for g in range(cfg["B"])]), [d[f"lesioned_{g}"] for g in range(cfg["B"])])
    worst = check(got, golden)                                   # (NaN exactly where the reference has it)
    ref = oracle_lesion(state64(model), spec_of(model), graphs, sets)
    worst = max(worst, check(got, ref))
    for g, (gr, S) in enumerate(zip(graphs, sets)):              # NaN confinement: exactly the sets the oracle marks
        want = np.array([expect_nan(gr, D, cfg["npool"], cfg["learn_eps"]) for D in S])
        assert (np.isnan(ref[1][g]).all(1) == want).all() and (np.isnan(got[2][g]).all(1) == want).all()
        assert (np.isnan(got[2][g]).any(1) == want).all()
    if "hub" in case:
        assert any(np.isnan(p).any() for p in got[2]) and all(np.isfinite(p[0]).all() for p in got[2])
    print("worst rel err %s: %.2e" % (case, worst))


@pytest.mark.parametrize("L", [1, 3])
@pytest.mark.parametrize("m", [1, 2, 3])
@pytest.mark.parametrize("H", [32, 64, 128])
def test_small_shape_matrix(H, m, L):
    """n = 6, 33, 40 (one asymmetric) and 70 -- one, two and three row blocks, 33 across a block edge, 70 across the
    64-column word of the bit layout -- F0 = 7, every pooling form, the sets of matrix_sets: against the fp64 oracle and
    against predict() on explicit copies.

    The model seeds (200 + H + m) are chosen for conditioning, judged by the fp32 numpy oracle alone: rel_err divides
    by a graph's max |base|, and a base that is a cancellation of much larger terms makes ANY fp32 forward miss 1e-5.
    With seed H + m the case H = 32, m = 1, L = 1 has such a graph (average / sum, no learned eps, the asymmetric one:
    base 0.09 out of terms near 2), where the fp32 oracle is itself 6.0e-6 from fp64; with these seeds it is within
    1.9e-6 of fp64 on all 18 x 8 models, every graph and set."""
    gs = [random_graph(10, 6, 0.6, 7), random_graph(11, 33, 0.2, 7), random_graph(12, 40, 0.2, 7),
          random_graph(13, 40, 0.2, 7, directed=True), random_graph(14, 70, 0.15, 7)]
    sets = [matrix_sets(len(g.g), 20 + i) for i, g in enumerate(gs)]
    assert [s.shape[0] for s in sets] == [4, 7, 7, 7, 9]
    worst = 0.0
    for npool, gpool, le in POOLS:
        model = model_of(L, m, 7, H, le, gpool, npool, seed=200 + H + m)
        ref = oracle_lesion(state64(model), spec_of(model), gs, sets)
        for g, S, r in zip(gs, sets, ref[1]):                    # finite wherever finiteness is expected: nothing is
            want = np.array([expect_nan(g, D, npool, le) for D in S])        # silently excluded
            assert (np.isnan(r).any(1) == want).all() and np.isfinite(r[~want]).all()
        assert np.isfinite(ref[0]).all()
        got = run(model, gs, sets, batch_size=3)
        worst = max(worst, check(got, ref), check(got, predict_scores(model, gs, sets)))
    print("worst rel err H=%d m=%d L=%d: %.2e" % (H, m, L, worst))


def test_empty_set_is_predict_and_one_node_sets_are_occlusion():
    worst_p = worst_o = 0.0
    for npool, gpool, le in POOLS:
        model = model_of(3, 2, 7, 64, le, gpool, npool, seed=9)
        gs = [random_graph(30 + i, 40, 0.2, 7, directed=(i == 1)) for i in range(2)]
        sets = np.concatenate([np.zeros((1, 40), dtype=bool), np.eye(40, dtype=bool)])
        _, base, les = model.lesion(gs, (0, 1), sets, return_scores=True)
        assert les.shape == (2, 2, 41)
        pred = model.predict(gs).cpu().numpy()                   # [G, C]
        _, _, occ = model.occlusion(gs, (0, 1), return_scores=True)        # [C, G, n]
        for g in range(2):
            scale = float(np.abs(pred[g]).max())
            worst_p = max(worst_p, rel_err(les[:, g, 0].cpu().numpy(), pred[g]),
                          rel_err(base[:, g].cpu().numpy(), pred[g]))
            worst_o = max(worst_o, rel_err(les[:, g, 1:].cpu().numpy(), occ[:, g].cpu().numpy(), floor=scale))
    print("worst rel err: empty set vs predict %.2e, one-node sets vs occlusion %.2e" % (worst_p, worst_o))
    assert worst_p <= RTOL and worst_o <= RTOL


def test_ragged_batches_and_result_shapes():
    model = model_of(3, 2, 7, 64, True, "average", "average", seed=4)
    gs = [random_graph(90 + i, n, 0.3, 7) for i, n in enumerate((20, 33, 64, 7, 2))]
    rng = np.random.default_rng(1)
    sets = []
    for i, g in enumerate(gs):                                   # 1 .. 5 sets per graph, the empty set first
        n = len(g.g)
        S = rng.random((i + 1, n)) < 0.4
        S[0] = False
        S[:, 0] &= ~S.all(1)
        sets.append(S)
    ref = oracle_lesion(state64(model), spec_of(model), gs, sets)
    got = run(model, gs, sets, batch_size=3)
    delta = got[0]
    assert isinstance(delta, list) and len(delta) == 2 and [tuple(x.shape) for x in delta[0]] == [(k,) for k in range(1, 6)]
    check(got, ref)                                              # (NaN where a copy has a 0/0 row, as the oracle)
    one = model.lesion(gs, 1, sets, batch_size=3)
    assert isinstance(one, list) and all(torch.equal(torch.nan_to_num(a), torch.nan_to_num(b))
                                         for a, b in zip(one, delta[1]))
    same = [s[:1] for s in sets]                                 # equal set counts over ragged graphs: a tensor
    d1, b1, l1 = model.lesion(gs, 0, same, return_scores=True)
    assert d1.shape == (5, 1) and b1.shape == (5,) and l1.shape == (5, 1)
    eq = [random_graph(80 + i, 20, 0.3, 7) for i in range(3)]
    shared = torch.as_tensor(rng.random((4, 20)) < 0.3)
    d2 = model.lesion(eq, (0, 1), shared)                        # one [S, n] mask over equal graphs: a tensor
    assert torch.is_tensor(d2) and d2.shape == (2, 3, 4) and d2.device.type == "cuda"
    d3 = model.lesion(eq, (0, 1), [shared.numpy().astype(np.int64)] * 3)
    assert torch.equal(torch.nan_to_num(d2), torch.nan_to_num(d3))


# ---------------------------------------------------------------------------------------------- behaviour
def test_determinism_batch_size_chunks_and_other_sets(monkeypatch):
    from gnm import attribution, core
    from gnm._cabi import lib
    model = model_of(3, 2, 7, 64, True, "average", "average", seed=2)
    gs = [random_graph(20 + i, 40, 0.2, 7) for i in range(5)]
    rng = np.random.default_rng(3)
    sets = rng.random((6, 40)) < 0.3
    sets[0] = False
    d0, b0, l0 = model.lesion(gs, (0, 1), sets, return_scores=True)
    assert torch.isfinite(l0).all()
    for bs in (1, 3, 8, 8):                                      # (8 again: run to run)
        d, b, o = model.lesion(gs, (0, 1), sets, batch_size=bs, return_scores=True)
        assert torch.equal(d, d0) and torch.equal(b, b0) and torch.equal(o, l0), bs
    order = [4, 2, 2, 0, 5, 1, 3, 2]                             # sets duplicated and reordered within the call
    _, _, o = model.lesion(gs, (0, 1), sets[order], return_scores=True)
    assert torch.equal(o, l0[:, :, order])
    _, _, o = model.lesion(gs, (0, 1), sets[3:4], return_scores=True)      # a set alone
    assert torch.equal(o, l0[:, :, 3:4])
    calls = []
    real = lib.gnm_lesion
    monkeypatch.setattr(core.lib, "gnm_lesion", lambda *a: calls.append(1) or real(*a), raising=False)
    monkeypatch.setattr(attribution, "LESION_SCRATCH_BYTES", 4 * int(lib.gnm_lesion_scratch_floats(7 * 40, 7, 40, 64, 3)))
    d, b, o = model.lesion(gs, (0, 1), sets, batch_size=8, return_scores=True)       # 30 virtual graphs, 7 to a chunk
    assert len(calls) == 5
    assert torch.equal(d, d0) and torch.equal(b, b0) and torch.equal(o, l0)
    assert torch.equal(model.lesion(gs, 1, sets), d0[1]) and torch.equal(model.lesion(gs, (1, 0), sets), d0.flip(0))


@pytest.mark.parametrize("training", [True, False])
def test_no_side_effects(training):
    model = model_of(3, 2, 7, 64, True, "sum", "average", seed=3)
    model.train(training)
    gs = [random_graph(30 + i, 40, 0.2, 7) for i in range(2)]
    sets = np.random.default_rng(0).random((3, 40)) < 0.3
    before = {k: v.clone() for k, v in model.state_dict().items()}
    np.random.seed(11)
    rng = np.random.get_state()
    out = model.lesion(gs, 0, sets)
    scores, area = model.deletion_curve(gs, 0, np.random.default_rng(1).random((2, 40)), fractions=[0, 0.5])
    assert out.shape == (2, 3) and out.device.type == "cuda" and not out.requires_grad
    assert scores.shape == (2, 2) and area.shape == (2,) and area.dtype == np.float64
    assert model.training == training
    assert all(p.grad is None for p in model.parameters())
    after = model.state_dict()
    assert all(torch.equal(before[k], after[k]) for k in before)
    now = np.random.get_state()
    assert rng[0] == now[0] and np.array_equal(rng[1], now[1]) and rng[2:] == now[2:]


def test_nan_feature_stays_in_its_graph():
    model = model_of(3, 2, 7, 64, False, "average", "sum", seed=5)
    gs = [random_graph(40 + i, 40, 0.2, 7) for i in range(3)]
    sets = np.random.default_rng(2).random((4, 40)) < 0.3
    sets[1, 3] = True                                            # (the bad row inside a set: still all-NaN, as stated)
    clean = model.lesion([gs[0], gs[2]], (0, 1), sets)
    assert torch.isfinite(clean).all()
    gs[1].node_features[3, 2] = float("nan")
    got = model.lesion(gs, (0, 1), sets)
    assert torch.isnan(got[:, 1]).all()
    assert torch.equal(got[:, 0], clean[:, 0]) and torch.equal(got[:, 2], clean[:, 1])


def test_declined_shapes_and_bad_masks_raise_with_their_reason():
    gs = [random_graph(60 + i, 40, 0.2, 7) for i in range(2)]
    ok = np.zeros((2, 40), dtype=bool)
    ok[1, :5] = True
    nb = model_of(2, 2, 7, 64, True, "sum", "max", seed=1)
    with pytest.raises(ValueError, match="max neighbour pooling"):
        nb.lesion(gs, 0, ok)
    model = model_of(2, 2, 7, 64, True, "sum", "sum", seed=1)
    with pytest.raises(ValueError, match="416"):
        model.lesion([random_graph(70, 420, 0.05, 7)], 0, np.zeros((1, 420), dtype=bool))
    with pytest.raises(ValueError, match="hidden_dim 16"):
        model_of(2, 2, 7, 16, True, "sum", "sum", seed=1).lesion(gs, 0, ok)
    with pytest.raises(ValueError, match="num_mlp_layers"):
        model_of(2, 4, 7, 64, True, "sum", "sum", seed=1).lesion(gs, 0, ok)
    model._spec.sync_bn = object()
    with pytest.raises(ValueError, match="synchronised BatchNorm"):
        model.lesion(gs, 0, ok)
    model._spec.sync_bn = None
    with pytest.raises(ValueError, match="fewer than 2 nodes"):
        model.lesion(gs + [random_graph(71, 1, 0.5, 7)], 0, [ok, ok, np.zeros((1, 1), dtype=bool)])
    with pytest.raises(ValueError, match="removes every node"):
        model.lesion(gs, 0, np.ones((1, 40), dtype=bool))
    with pytest.raises(ValueError, match="41 wide for a 40-node graph"):
        model.lesion(gs, 0, np.zeros((1, 41), dtype=bool))
    with pytest.raises(ValueError, match="0 and 1"):
        model.lesion(gs, 0, np.full((1, 40), 2))
    with pytest.raises(ValueError, match="one node count"):
        model.lesion(gs + [random_graph(72, 20, 0.3, 7)], 0, ok)
    # the C entry: a bad argument returns its code and launches nothing
    assert lesion_call(H=36) == -2 and lesion_call(cls=(2,)) == -1 and lesion_call() == -1
    assert lesion_call(null=False, kept=np.zeros(20)) == -1
    assert model.lesion(gs, 0, ok).shape == (2, 2)               # and the model still works


# ---------------------------------------------------------------------------------------------- deletion curves
def test_deletion_curve_small():
    from gnm.lesion import curve_area, masks_from_ranking
    model = model_of(3, 2, 7, 64, False, "average", "average", seed=6)
    gs = [random_graph(50 + i, 40, 0.2, 7) for i in range(3)]
    rank, base, _ = model.occlusion(gs, (0, 1), return_scores=True)
    rank = rank[0]                                               # class 0's occlusion delta, [G, n]
    fr = [0, 0.05, 0.1, 0.3, 0.5, 0.9, 0.95, 1.0]
    scores, area = model.deletion_curve(gs, (0, 1), rank, fractions=fr)
    assert scores.shape == (2, 3, 8) and scores.dtype == torch.float32 and scores.device.type == "cuda"
    assert area.shape == (2, 3) and area.dtype == np.float64
    masks, counts = masks_from_ranking(rank.cpu().numpy(), fr)
    assert counts[0].tolist() == [0, 2, 4, 12, 20, 36, 38, 39]
    _, lbase, les = model.lesion(gs, (0, 1), masks, return_scores=True)
    assert torch.equal(scores, les)                              # bitwise lesion() on the same masks
    want = curve_area(les.cpu().numpy(), np.stack(counts) / 40.0)
    assert np.array_equal(area, want) and np.isfinite(area).all()
    one, a1 = model.deletion_curve(gs, 1, list(rank), fractions=fr)       # a list of per-graph rankings, an int class
    assert torch.equal(one, scores[1]) and np.array_equal(a1, area[1])
    asc, _ = model.deletion_curve(gs, (0, 1), rank, fractions=fr, order="ascending")
    assert torch.equal(asc[:, :, 0], scores[:, :, 0])            # fraction 0: the empty set, whatever the order
    assert not torch.equal(asc[:, :, 1:], scores[:, :, 1:])
    e = max(rel_err(asc[:, g, 0].cpu().numpy(), base[:, g].cpu().numpy()) for g in range(3))
    print("fraction 0 against base: %.2e" % e)
    assert e <= RTOL and torch.equal(lbase, base)
    dflt, _ = model.deletion_curve(gs, 0, rank)
    assert dflt.shape == (3, 20) and torch.equal(dflt[:, 0], scores[0, :, 0])


@pytest.mark.parametrize("tag,one_hot,npool,gpool,learn_eps", [("f7_gaverage_naverage_eps1", False, "average", "average", True),
                                                               ("onehot_gsum_nsum_eps1", True, "sum", "sum", True)])
def test_deletion_curve_400_nodes(tag, one_hot, npool, gpool, learn_eps):
    """the reference's shape: a 400-node dense connectivity graph, L = 5, H = 64, F0 = 7 and one-hot 400: 8 sets, a
    deletion curve at fractions 0, 0.05, 0.25, 0.5, 0.75, 0.9, 0.95 plus all-but-one, under the calibrated bound of the
    file header; the 16 CPU references (fp32 torch and fp64 numpy on the same deleted graphs) are computed here"""
    from gnm import synth
    from gnm.lesion import masks_from_ranking
    from oracle import gin_oracle as O
    from oracle.gin_torch_cpu import TorchCpuGIN
    g = synth.dense_fc_graph(0, n=400)
    if one_hot:
        g.node_features = torch.eye(400)
    model = model_of(5, 2, 400 if one_hot else 7, 64, learn_eps, gpool, npool, seed=7)
    rank = torch.nan_to_num(model.occlusion([g], 0)).cpu().numpy()
    fr = [0, 0.05, 0.25, 0.5, 0.75, 0.9, 0.95, 1.0]              # (1.0: capped at n - 1, all but one)
    masks, counts = masks_from_ranking(rank, fr)
    assert counts[0].tolist() == [0, 20, 100, 200, 300, 360, 380, 399]
    scores, area = model.deletion_curve([g], (0, 1), rank, fractions=fr)
    base = model.predict([g]).cpu().numpy()[0]
    st = state64(model)
    spec = spec_of(model)
    cpu = TorchCpuGIN({k: np.asarray(v, dtype=np.float32) if np.asarray(v).dtype.kind == "f" else v
                       for k, v in st.items()}, *spec)
    orc = O.OracleGIN(st, *spec, dtype=np.float64)
    r32, r64 = [], []
    for D in masks[0]:
        c = delete_nodes(g, D)
        og = O.OGraph(len(c.g), c.edge_mat.numpy(), c.node_features.numpy())
        with torch.no_grad(), np.errstate(all="ignore"):
            r32.append(cpu.forward([og], [0], training=False, want_disc=False)[0].numpy()[0])
            r64.append(orc.forward([og], np.arange(1), training=False, want_disc=False)[0][0])
    r32, r64 = np.stack(r32), np.stack(r64)
    want = np.array([expect_nan(g, D, npool, learn_eps) for D in masks[0]])
    assert (np.isnan(r64).any(1) == want).all() and np.isfinite(r64[~want]).all() and not want[0]
    cal = Calibrated()
    scale = float(np.abs(r64[0]).max())
    cal.check(base, r32[0], r64[0], "base")
    cal.check(scores[:, 0].t().cpu().numpy(), r32, r64, "lesioned", floor=scale)
    assert np.isfinite(area).all() == (not want.any())
    print("400-node %s: %s" % (tag, [(w, "%.2e" % e, "%.2e" % r, "%.2e" % b_) for w, e, r, b_ in cal.log]))
