"""GIN_InfoMaxReg.disconnect() / disconnection_matrix() (csrc/disconnect.hip): the class scores of edge-cut copies of a
graph, computed on virtual graphs under a keep mask chosen per row, against three anchors -- the real reference's goldens
(tests/golden/disconnect/), the route without the method (model.predict() on explicit copies made by
tests/test_disconnect_host.py cut_edges) and the fp64 oracle on the same copies; the identities of the rule (symmetry, a
pair without an edge between its sets, b = a, the matrix layer), invariance to the batch size, the chunking and the other
pairs of the call, side effects (none), NaN confinement, the declined shapes and the bad masks.

Accuracy is asserted on `disconnected` and `base` (delta is a difference of two nearly equal numbers) by
test_gpu_lesion.check: max-norm relative to the graph's max |base|, NaN patterns equal.  Small cases (L <= 3, n <= 70):
the flat RTOL = 1e-5, on seeds whose conditioning tests/test_disconnect_host.py asserts.  n = 257 and 416: RTOL, or
helpers.Calibrated (4 x the fp32 numpy oracle's own error) for a case whose fp32 oracle is further than RTOL / 4 from
fp64 -- such a case is printed, not dropped.  n = 400, L = 5: helpers.Calibrated against the independent fp32 CPU forward
oracle.gin_torch_cpu.TorchCpuGIN and the fp64 oracle ON THE SAME CUT GRAPHS -- never a HIP output.  Every test prints its
worst error (pytest -s); the values measured on an MI355X are in DESIGN.md section 3.15."""
import numpy as np
import pytest
import torch

from helpers import RTOL, Calibrated, rel_err
from test_disconnect_host import (DC_CASES, MATRIX_SHAPES, cut_edges, dc_graphs, disconnect_call, expect_nan_cut,
                                  load_dc_case, matrix_inputs, matrix_seed, oracle_disconnect)
from test_gpu_lesion import check
from test_gpu_occlusion import spec_of, state64
from test_gpu_saliency import model_of, random_graph

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
POOLS = [(np_, gp, le) for np_ in ("sum", "average") for gp in ("sum", "average") for le in (True, False)]
nn7 = lambda t: torch.nan_to_num(t, nan=7.0)                                       # noqa: E731


def run(model, graphs, a, b=None, classes=(0, 1), **kw):
    """(delta, base [C, G] numpy, disconnected: per graph [S_g, C] numpy) with delta = base - disconnected bitwise"""
    delta, base, dis = model.disconnect(graphs, tuple(classes), a, b, return_scores=True, **kw)
    assert base.shape == (len(classes), len(graphs)) and base.dtype == torch.float32
    if torch.is_tensor(dis):
        assert dis.dtype == torch.float32 and dis.shape[:2] == (len(classes), len(graphs)) and dis.device.type == "cuda"
        assert torch.equal(nn7(delta), nn7(base.unsqueeze(-1) - dis))
        per = [dis[:, g].t().cpu().numpy() for g in range(len(graphs))]
    else:
        for ci in range(len(classes)):
            for g in range(len(graphs)):
                assert torch.equal(nn7(delta[ci][g]), nn7(base[ci, g] - dis[ci][g]))
        per = [torch.stack([dis[ci][g] for ci in range(len(classes))], 1).cpu().numpy() for g in range(len(graphs))]
    return delta, base.cpu().numpy(), per


def predict_scores(model, graphs, pa, pb):
    """the route without the method: predict() on the graphs and on explicit edge-cut copies (in batches of one node
    count, as predict() asks)"""
    base = np.concatenate([model.predict([g]).cpu().numpy() for g in graphs], 0)
    copies = [(gi, si, cut_edges(g, A, B)) for gi, (g, SA, SB) in enumerate(zip(graphs, pa, pb))
              for si, (A, B) in enumerate(zip(SA, SB))]
    out = [np.zeros((len(SA), base.shape[1])) for SA in pa]
    for n in sorted({len(c.g) for _, _, c in copies}):
        grp = [(gi, si, c) for gi, si, c in copies if len(c.g) == n]
        pred = model.predict([c for _, _, c in grp]).cpu().numpy()
        for (gi, si, _), p in zip(grp, pred):
            out[gi][si] = p
    return base, out


def nan_where_expected(graphs, pa, pb, npool, le, *results):
    """NaN in exactly the pairs expect_nan_cut marks, in every score of such a pair, for each per-graph result list"""
    for g, (gr, SA, SB) in enumerate(zip(graphs, pa, pb)):
        want = np.array([expect_nan_cut(gr, A, B, npool, le) for A, B in zip(SA, SB)], dtype=bool)
        for per in results:
            nan = np.isnan(per[g])
            assert (nan.any(1) == want).all() and (nan.all(1) == want).all(), (g, want)


# ---------------------------------------------------------------------------------------------- parity
@pytest.mark.parametrize("case", DC_CASES)
def test_against_reference_goldens(case):
    from models.graphcnn import GIN_InfoMaxReg
    cfg, state, d = load_dc_case(case)
    model = GIN_InfoMaxReg(cfg["L"], cfg["m"], cfg["f0"], cfg["H"], cfg["C"], 0.0, cfg["learn_eps"], cfg["gpool"],
                           cfg["npool"], torch.device(DEV)).to(DEV)
    missing, unexpected = model.load_state_dict({k: torch.as_tensor(v) for k, v in state.items()}, strict=False)
    assert not unexpected and all(k.startswith("disc.") for k in missing)
    graphs, pa, pb = dc_graphs(cfg, d)
    got = run(model, graphs, pa, pb)
    golden = (np.stack([d[f"base_{g}"] for g in range(cfg["B"])]), [d[f"disconnected_{g}"] for g in range(cfg["B"])])
    worst = check(got, golden)                                   # (NaN exactly where the reference has it)
    ref = oracle_disconnect(state64(model), spec_of(model), graphs, pa, pb)
    worst = max(worst, check(got, ref))
    nan_where_expected(graphs, pa, pb, cfg["npool"], cfg["learn_eps"], ref[1], got[2])
    if "hub" in case:
        assert all(np.isnan(p[1]).all() and np.isfinite(p[0]).all() and np.isfinite(p[2]).all() for p in got[2])
    print("worst rel err %s: %.2e" % (case, worst))


@pytest.mark.parametrize("H,m,L", MATRIX_SHAPES)
def test_small_shape_matrix(H, m, L):
    """n = 6, 33, 40 (one asymmetric) and 70 -- one, two and three row blocks, 33 across a block edge, 70 across the
    64-column word of the bit layout -- F0 = 7, every pooling form, the pairs of test_disconnect_host.matrix_pairs (the
    empty pair, one node against all, all against all, row block 0 against row block 1, overlapping sets at the byte,
    half-row and word edges, two disjoint thirds, a half within itself): against the fp64 oracle and against predict()
    on explicit copies.  The seeds: test_disconnect_host.test_matrix_seeds_are_well_conditioned."""
    gs, pa, pb = matrix_inputs()
    worst = 0.0
    for npool, gpool, le in POOLS:
        model = model_of(L, m, 7, H, le, gpool, npool, seed=matrix_seed(H, m))
        ref = oracle_disconnect(state64(model), spec_of(model), gs, pa, pb, group=64)
        nan_where_expected(gs, pa, pb, npool, le, ref[1])        # finite wherever finiteness is expected: nothing is
        assert np.isfinite(ref[0]).all()                         # silently excluded
        got = run(model, gs, pa, pb, batch_size=3)
        worst = max(worst, check(got, ref), check(got, predict_scores(model, gs, pa, pb)))
    print("worst rel err H=%d m=%d L=%d: %.2e" % (H, m, L, worst))


@pytest.mark.parametrize("npool,gpool,le", POOLS)
def test_identities_are_bitwise(npool, gpool, le):
    """disconnect(a, b) = disconnect(b, a); a pair with no edge between its sets = the empty pair; disconnect(a) =
    disconnect(a, a); the matrix layer = the matching disconnect() pairs, symmetric; the empty pair against predict()"""
    from gnm.lesion import cut_edge_counts, pair_sets
    model = model_of(3, 2, 7, 64, le, gpool, npool, seed=9)
    gs = [random_graph(30 + i, 40, 0.2, 7, directed=(i == 1)) for i in range(2)]
    rng = np.random.default_rng(8)
    a, b = rng.random((6, 40)) < 0.35, rng.random((6, 40)) < 0.35
    a[0] = b[0] = False                                          # the empty pair
    idx = np.arange(40)
    for j, g in enumerate(gs):                                   # per graph a pair with NO edge between its sets:
        em = g.edge_mat.numpy()                                  # node 5 against the nodes it has no edge with
        nbr = np.zeros(40, dtype=bool)
        nbr[em[1][em[0] == 5]] = True
        nbr[em[0][em[1] == 5]] = True
        far = ~nbr & (idx != 5)
        assert far.any() and cut_edge_counts(em, (idx == 5)[None], far[None])[0] == 0
        if j == 0:
            a1, b1 = (idx == 5), far
        else:
            a2, b2 = (idx == 5), far
    la = [np.concatenate([a, a1[None]]), np.concatenate([a, a2[None]])]
    lb = [np.concatenate([b, b1[None]]), np.concatenate([b, b2[None]])]
    _, base, ab = model.disconnect(gs, (0, 1), la, lb, return_scores=True)
    _, _, ba = model.disconnect(gs, (0, 1), lb, la, return_scores=True)
    assert ab.shape == (2, 2, 7) and torch.equal(nn7(ab), nn7(ba))
    assert torch.equal(nn7(ab[:, :, 6]), nn7(ab[:, :, 0]))       # nothing to cut: the empty pair's bits
    _, _, aa = model.disconnect(gs, (0, 1), a, a, return_scores=True)
    _, _, a_ = model.disconnect(gs, (0, 1), a, return_scores=True)
    assert torch.equal(nn7(aa), nn7(a_))
    pred = model.predict(gs).cpu().numpy()                       # [G, C]
    e = max(max(rel_err(ab[:, g, 0].cpu().numpy(), pred[g]), rel_err(base[:, g].cpu().numpy(), pred[g])) for g in range(2))
    assert e <= RTOL
    lab = rng.integers(-1, 4, 40)
    pa, pb, pairs = pair_sets(lab)
    assert len(pairs) == 10
    dm, mbase, ms = model.disconnection_matrix(gs, (0, 1), lab, return_scores=True)
    dd, dbase, ds = model.disconnect(gs, (0, 1), pa, pb, return_scores=True)
    assert dm.shape == ms.shape == (2, 2, 4, 4) and dm.dtype == torch.float32 and dm.device.type == "cuda"
    assert torch.equal(mbase, dbase) and torch.equal(mbase, base)
    for s, (p, q) in enumerate(pairs):
        for mat, flat in ((dm, dd), (ms, ds)):
            assert torch.equal(nn7(mat[:, :, p, q]), nn7(flat[:, :, s]))
            assert torch.equal(nn7(mat[:, :, q, p]), nn7(flat[:, :, s]))
    assert torch.equal(nn7(dm), nn7(dm.transpose(-1, -2)))
    one = model.disconnection_matrix(gs, 1, [lab, lab])          # an int class, per-graph labels
    assert one.shape == (2, 4, 4) and torch.equal(nn7(one), nn7(dm[1]))
    print("empty pair against predict(): %.2e" % e)


# ---------------------------------------------------------------------------------------------- above 256 nodes
def big_pairs(n, seed):
    """the pairs of the n > 256 cases (rb_half_words = 8: the second 128-bit load of a half row is live)"""
    idx = np.arange(n)
    rng = np.random.default_rng(seed)
    blk = lambda rb: (idx >= 32 * rb) & (idx < 32 * rb + 32)                       # noqa: E731
    half = np.isin(idx, rng.choice(n, n // 2, replace=False))
    every = np.ones(n, dtype=bool)
    P = [(np.isin(idx, (255, 256)), blk(0)), (blk(8), blk((n - 1) // 32)), (blk(0), every), (half, ~half),
         (every, every)]
    return np.stack([a for a, _ in P]), np.stack([b for _, b in P])


@pytest.mark.parametrize("npool,gpool,le", POOLS)
@pytest.mark.parametrize("n", [257, 416])
def test_above_256_nodes(n, npool, gpool, le):
    """H = 64, m = 2, L = 3; an undirected graph at edge probability 12 / n and a directed one at 0.5; against the fp64
    oracle under RTOL -- or, if this case's own fp32 numpy oracle is further than RTOL / 4 from fp64, under
    helpers.Calibrated's 4 x that distance, and the case is reported"""
    model = model_of(3, 2, 7, 64, le, gpool, npool, seed=300 + n)
    gs = [random_graph(5000 + n, n, 12.0 / n, 7), random_graph(5001 + n, n, 0.5, 7, directed=True)]
    prs = [big_pairs(n, 40 + i) for i in range(2)]
    pa, pb = [p[0] for p in prs], [p[1] for p in prs]
    st = state64(model)
    st32 = {k: v.astype(np.float32) if v.dtype.kind == "f" else v for k, v in st.items()}
    ref = oracle_disconnect(st, spec_of(model), gs, pa, pb)
    r32 = oracle_disconnect(st32, spec_of(model), gs, pa, pb, dtype=np.float32)
    nan_where_expected(gs, pa, pb, npool, le, ref[1])
    cal = Calibrated()
    for g in range(2):
        fin = ~np.isnan(ref[1][g]).any(1)
        cal.noise = max(cal.noise, rel_err(r32[0][g], ref[0][g]),
                        rel_err(r32[1][g][fin], ref[1][g][fin], floor=float(np.abs(ref[0][g]).max())))
    bound = max(cal.base, cal.factor * cal.noise)                # RTOL unless the fp32 oracle is past RTOL / 4
    got = run(model, gs, pa, pb)
    worst = check(got, ref, rtol=bound)
    nan_where_expected(gs, pa, pb, npool, le, got[2])
    print("n=%d %s/%s/eps%d: worst %.2e under %.2e (fp32 oracle %.2e)%s"
          % (n, npool, gpool, le, worst, bound, cal.noise, "  CALIBRATED" if bound > RTOL else ""))


# ---------------------------------------------------------------------------------------------- the true shape
@pytest.mark.parametrize("tag,one_hot,npool,gpool,learn_eps", [("f7_gaverage_naverage_eps1", False, "average", "average", True),
                                                               ("onehot_gsum_nsum_eps1", True, "sum", "sum", True)])
def test_disconnection_matrix_400_nodes(tag, one_hot, npool, gpool, learn_eps):
    """the reference's shape: a 400-node dense connectivity graph, L = 5, H = 64, F0 = 7 and one-hot 400; a 7-network
    labelling, 28 pairs through disconnection_matrix(), under the calibrated bound of the file header; the CPU
    references (fp32 torch and fp64 numpy on the same cut graphs) are computed here, as test_deletion_curve_400_nodes"""
    from gnm import synth
    from gnm.lesion import cut_edge_counts, pair_sets
    from rowblock_midrange_cases import oracle_scores64, torch_scores32
    g = synth.dense_fc_graph(0, n=400)
    if one_hot:
        g.node_features = torch.eye(400)
    model = model_of(5, 2, 400 if one_hot else 7, 64, learn_eps, gpool, npool, seed=7)
    lab = np.random.default_rng(3).integers(0, 7, 400)
    lab[::57] = -1                                               # a few ROIs of no network
    pa, pb, pairs = pair_sets(lab)
    assert len(pairs) == 28 and cut_edge_counts(g.edge_mat, pa, pb).min() > 0
    delta, base, scores = model.disconnection_matrix([g], (0, 1), lab, return_scores=True)
    assert delta.shape == scores.shape == (2, 1, 7, 7) and base.shape == (2, 1)
    assert torch.equal(nn7(delta), nn7(base[:, :, None, None] - scores))
    flat = scores[:, 0, pairs[:, 0], pairs[:, 1]].t().cpu().numpy()                # [28, C]
    st, spec = state64(model), spec_of(model)
    copies = [g] + [cut_edges(g, A, B) for A, B in zip(pa, pb)]
    r64, r32 = oracle_scores64(st, spec, copies, group=8), torch_scores32(st, spec, copies, group=8)
    want = np.array([expect_nan_cut(g, A, B, npool, learn_eps) for A, B in zip(pa, pb)])
    assert (np.isnan(r64[1:]).any(1) == want).all() and np.isfinite(r64[1:][~want]).all() and np.isfinite(r64[0]).all()
    cal = Calibrated()
    scale = float(np.abs(r64[0]).max())
    cal.check(base[:, 0].cpu().numpy(), r32[0], r64[0], "base")
    cal.check(flat, r32[1:], r64[1:], "disconnected", floor=scale)
    print("400-node %s: %s" % (tag, [(w, "%.2e" % e, "%.2e" % r, "%.2e" % b_) for w, e, r, b_ in cal.log]))


# ---------------------------------------------------------------------------------------------- behaviour
def test_ragged_batch_is_bitwise_each_graph_alone():
    from rowblock_midrange_cases import ragged_graphs
    model = model_of(3, 2, 7, 64, True, "average", "average", seed=4)
    gs = ragged_graphs()
    assert [len(g.g) for g in gs] == [33, 256, 257, 416, 2]
    rng = np.random.default_rng(1)
    la = [rng.random((i + 1, len(g.g))) < 0.4 for i, g in enumerate(gs)]
    lb = [rng.random((i + 1, len(g.g))) < 0.4 for i, g in enumerate(gs)]
    for x in la + lb:
        x[0] = False                                             # the empty pair first
    delta, base, dis = model.disconnect(gs, (0, 1), la, lb, batch_size=8, return_scores=True)
    assert isinstance(delta, list) and len(delta) == 2 and [tuple(x.shape) for x in delta[0]] == [(k,) for k in range(1, 6)]
    for j, g in enumerate(gs):
        d1, b1, s1 = model.disconnect([g], (0, 1), [la[j]], [lb[j]], return_scores=True)
        assert s1.shape == (2, 1, j + 1) and torch.equal(b1[:, 0], base[:, j])
        for ci in range(2):
            assert torch.equal(nn7(s1[ci, 0]), nn7(dis[ci][j])) and torch.equal(nn7(d1[ci, 0]), nn7(delta[ci][j]))
    same = model.disconnect(gs, 0, [x[:1] for x in la])          # equal pair counts over ragged graphs: a tensor
    assert torch.is_tensor(same) and same.shape == (5, 1)


def test_determinism_batch_size_chunks_and_other_pairs(monkeypatch):
    from gnm import attribution, core
    from gnm._cabi import lib
    from rowblock_midrange_cases import chunk_graphs
    model = model_of(3, 2, 7, 64, True, "average", "average", seed=2)
    gs = chunk_graphs()                                          # 5 graphs of 257 nodes
    rng = np.random.default_rng(3)
    a, b = rng.random((6, 257)) < 0.3, rng.random((6, 257)) < 0.3
    a[0] = b[0] = False
    a[1] = np.arange(257) >= 255                                 # columns 255 and 256: either side of the word groups
    d0, b0, s0 = model.disconnect(gs, (0, 1), a, b, return_scores=True)
    assert s0.shape == (2, 5, 6)
    for bs in (1, 3, 8, 8):                                      # (8 again: run to run)
        d, bb, s = model.disconnect(gs, (0, 1), a, b, batch_size=bs, return_scores=True)
        assert torch.equal(nn7(d), nn7(d0)) and torch.equal(bb, b0) and torch.equal(nn7(s), nn7(s0)), bs
    order = [4, 2, 2, 0, 5, 1, 3, 2]                             # pairs duplicated and reordered within the call
    _, _, s = model.disconnect(gs, (0, 1), a[order], b[order], return_scores=True)
    assert torch.equal(nn7(s), nn7(s0[:, :, order]))
    _, _, s = model.disconnect(gs, (0, 1), a[3:4], b[3:4], return_scores=True)     # a pair alone
    assert torch.equal(nn7(s), nn7(s0[:, :, 3:4]))
    calls = []
    real = lib.gnm_disconnect
    monkeypatch.setattr(core.lib, "gnm_disconnect", lambda *x: calls.append(1) or real(*x), raising=False)
    monkeypatch.setattr(attribution, "LESION_SCRATCH_BYTES", 4 * int(lib.gnm_disconnect_scratch_floats(7 * 257, 7, 257, 64, 3)))
    d, bb, s = model.disconnect(gs, (0, 1), a, b, batch_size=8, return_scores=True)        # 30 virtual graphs, 7 to a chunk
    assert len(calls) == 5
    assert torch.equal(nn7(d), nn7(d0)) and torch.equal(bb, b0) and torch.equal(nn7(s), nn7(s0))


def test_eleven_classes_against_one_at_a_time():
    model = model_of(3, 2, 7, 64, False, "average", "sum", seed=6, C=11)
    gs = [random_graph(50 + i, 40, 0.2, 7) for i in range(2)]
    rng = np.random.default_rng(5)
    a, b = rng.random((3, 40)) < 0.4, rng.random((3, 40)) < 0.4
    d, base, s = model.disconnect(gs, tuple(range(11)), a, b, return_scores=True)
    assert d.shape == (11, 2, 3) and base.shape == (11, 2) and torch.isfinite(s).all()
    for c in (0, 7, 8, 10):                                      # both finish launches (8 classes each)
        d1, b1, s1 = model.disconnect(gs, c, a, b, return_scores=True)
        assert d1.shape == (2, 3) and b1.shape == (2,)
        assert torch.equal(d1, d[c]) and torch.equal(b1, base[c]) and torch.equal(s1, s[c])
    rev = model.disconnect(gs, tuple(range(10, -1, -1)), a, b)
    assert torch.equal(rev, d.flip(0))


@pytest.mark.parametrize("training", [True, False])
def test_no_side_effects(training):
    model = model_of(3, 2, 7, 64, True, "sum", "average", seed=3)
    model.train(training)
    gs = [random_graph(30 + i, 40, 0.2, 7) for i in range(2)]
    a = np.random.default_rng(0).random((3, 40)) < 0.3
    before = {k: v.clone() for k, v in model.state_dict().items()}
    np.random.seed(11)
    rng = np.random.get_state()
    out = model.disconnect(gs, 0, a, ~a)
    mat = model.disconnection_matrix(gs, 0, np.arange(40) % 3)
    assert out.shape == (2, 3) and out.device.type == "cuda" and not out.requires_grad
    assert mat.shape == (2, 3, 3) and not mat.requires_grad
    assert model.training == training
    assert all(p.grad is None for p in model.parameters())
    after = model.state_dict()
    assert all(torch.equal(before[k], after[k]) for k in before)
    now = np.random.get_state()
    assert rng[0] == now[0] and np.array_equal(rng[1], now[1]) and rng[2:] == now[2:]


def test_nan_feature_stays_in_its_graph():
    model = model_of(3, 2, 7, 64, False, "average", "sum", seed=5)
    gs = [random_graph(40 + i, 40, 0.2, 7) for i in range(3)]
    rng = np.random.default_rng(2)
    a, b = rng.random((4, 40)) < 0.3, rng.random((4, 40)) < 0.3
    clean = model.disconnect([gs[0], gs[2]], (0, 1), a, b)
    assert torch.isfinite(clean).all()
    gs[1].node_features[3, 2] = float("nan")
    got = model.disconnect(gs, (0, 1), a, b)
    assert torch.isnan(got[:, 1]).all()
    assert torch.equal(got[:, 0], clean[:, 0]) and torch.equal(got[:, 2], clean[:, 1])


def test_declined_shapes_and_bad_masks_raise_with_their_reason():
    gs = [random_graph(60 + i, 40, 0.2, 7) for i in range(2)]
    ok = np.zeros((2, 40), dtype=bool)
    ok[1, :5] = True
    nb = model_of(2, 2, 7, 64, True, "sum", "max", seed=1)
    with pytest.raises(ValueError, match="max neighbour pooling"):
        nb.disconnect(gs, 0, ok)
    model = model_of(2, 2, 7, 64, True, "sum", "sum", seed=1)
    with pytest.raises(ValueError, match="416"):
        model.disconnect([random_graph(70, 420, 0.05, 7)], 0, np.zeros((1, 420), dtype=bool))
    with pytest.raises(ValueError, match="hidden_dim 16"):
        model_of(2, 2, 7, 16, True, "sum", "sum", seed=1).disconnect(gs, 0, ok)
    with pytest.raises(ValueError, match="num_mlp_layers"):
        model_of(2, 4, 7, 64, True, "sum", "sum", seed=1).disconnect(gs, 0, ok)
    model._spec.sync_bn = object()
    with pytest.raises(ValueError, match="synchronised BatchNorm"):
        model.disconnect(gs, 0, ok)
    model._spec.sync_bn = None
    with pytest.raises(ValueError, match="fewer than 2 nodes"):
        model.disconnect(gs + [random_graph(71, 1, 0.5, 7)], 0, [ok, ok, np.zeros((1, 1), dtype=bool)])
    with pytest.raises(ValueError, match="41 wide for a 40-node graph"):
        model.disconnect(gs, 0, np.zeros((1, 41), dtype=bool))
    with pytest.raises(ValueError, match="0 and 1"):
        model.disconnect(gs, 0, ok, np.full((2, 40), 2))
    with pytest.raises(ValueError, match="shapes"):
        model.disconnect(gs, 0, ok, ok[:1])
    with pytest.raises(ValueError, match="one node count"):
        model.disconnect(gs + [random_graph(72, 20, 0.3, 7)], 0, ok)
    # the C entry: a bad argument returns its code and launches nothing
    assert disconnect_call(H=36) == -2 and disconnect_call(cls=(2,)) == -1 and disconnect_call() == -1
    assert disconnect_call(null=False, vn=np.zeros(20)) == -1
    every = np.ones((1, 40), dtype=bool)                         # sets holding every node are taken: the edgeless graph
    assert model.disconnect(gs, 0, ok).shape == (2, 2) and torch.isfinite(model.disconnect(gs, 0, every)).all()
