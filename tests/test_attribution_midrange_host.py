"""The CPU half of the mid-range gradient-map tests -- saliency(), class_activation() of both kinds and edge_saliency()
between 97 and 416 nodes, and the input-width forms of the final dX launch (tests/rowblock_midrange_cases.py; the GPU half
is tests/test_gpu_attribution_midrange.py).  Without a GPU, by the CPU references alone and never by a HIP output:

  * ReLU margin at the graph's own features: in one plain fp64 eval forward of every graph no pre-activation under a ReLU
    sits within one fp32 ulp of zero at its layer's scale (rowblock_midrange_cases.IG_RELU_MARGIN; the existing check
    covers integrated_gradients()' quadrature points only);
  * fp32 floor: the fp32 references (OracleGIN.compute_saliency, test_cam_host.restate,
    test_edge_saliency_host.restate_edge in float32) stay within 1e-5 (saliency, gradient class activation, edge
    saliency) and 4e-5 (class activation: a sum of L positive and negative layer terms that cancel) of the fp64 ones,
    per graph over the classes, max-norm relative to each map's max |fp64|; so the GPU bound max(1e-5, 4 x that
    distance) never exceeds 4e-5, or 1.6e-4 for class activation;
  * every reference is finite and non-zero, and an edge map's absent entries and diagonal are non-trivial;
  * the shapes reach what the GPU file claims: plain arithmetic from the kernels' constants.
A case that breaks a condition is used as a reseeded variant (rowblock_midrange_cases.GRAD_SEEDS); a cap never moves."""
import numpy as np
import pytest

import rowblock_midrange_cases as T
from helpers import RTOL, rel_err

CAPS = dict(sal=1e-5, cam=4e-5, gcam=1e-5, edge=1e-5)
WIDTH_CAP = 2.5e-6              # the width cases: 4 x the floor stays under the flat 1e-5
PIN = 1e-12


def _all_grad_cases():
    return [c for n in T.NODES for c in T.grad_cases(n)]


def test_grad_seeds_name_cases_of_the_table_and_leave_it_alone():
    known = {c.id for n in T.NODES for c in T.cases(n)} | {c.id for c in T.CLASS_CASES + T.WIDTH_CASES}
    known |= {T.RAGGED_CASE.id, T.CHUNK_CASE.id}
    assert set(T.GRAD_SEEDS) <= known
    for need in ("n190-H128-m1-sum-sum-eps1", "n256-H32-m2-average-sum-eps1", "n257-H64-m2-sum-sum-eps1"):
        assert need in T.GRAD_SEEDS
    for n in T.NODES:
        for c, g in zip(T.cases(n), T.grad_cases(n)):
            if c.id in T.GRAD_SEEDS:
                assert g.id == c.id + "-g" and g.seed == T.GRAD_SEEDS[c.id] != c.seed
                assert g._replace(id=c.id, seed=c.seed) == c
                a, b = T.graphs_of(c), T.graphs_of(g)                           # the same graphs, another model
                assert all(np.array_equal(x.edge_mat, y.edge_mat) for x, y in zip(a, b))
            else:
                assert g is c
    assert len({c.id for c in _all_grad_cases()}) == len(_all_grad_cases())


def test_the_shapes_reach_what_the_gpu_tests_claim():
    # the average correction's byte walk brow[(j & 1) * HPW + (j >> 3)]: words 1 .. 3 of the HPW = 4 layout, 4 and up at 8
    hpw4 = {w for n in T.NODES if T.half_words(n) == 4 for w in T.correction_words(n)}
    hpw8 = {w for n in T.NODES if T.half_words(n) == 8 for w in T.correction_words(n)}
    assert {1, 2, 3} <= hpw4 and max(hpw4) == 3 and max(hpw8) >= 4 and max(hpw8) < 8
    assert T.correction_words(64) == [0] and T.correction_words(257) == [0, 1, 2, 3, 4]
    assert T.correction_words(416) == [0, 1, 2, 3, 4, 5, 6]
    # every n meets average pooling, and the tile loop wave + 4 t >= W runs at W = 4 .. 13
    for n in T.NODES:
        assert {c.npool for c in T.grad_cases(n)} == {"sum", "average"}
    assert {T.row_blocks(n) for n in T.NODES} == {4, 5, 6, 8, 9, 13}
    # the LDS strip stride lde = 32 W + 4 by n_max with a smaller graph in the launch: the ragged batch
    assert max(T.RAGGED_NODES) == T.MAX_N and len({T.row_blocks(n) for n in T.RAGGED_NODES}) == 5
    assert T.RAGGED_CASE.npool == "average"
    # gnm_class_activation_kernel: 64-row blocks; the last block's second half empty, partly live and full
    blocks = [T.cam_blocks(n) for n in T.NODES]
    assert blocks == [(2, 1), (3, 0), (3, 30), (4, 32), (5, 0), (7, 0), (7, 0)]
    assert T.cam_blocks(32) == (1, 0) and T.cam_blocks(64) == (1, 32) and T.cam_blocks(65) == (2, 0) and T.cam_blocks(96) == (2, 0)
    assert {live == 0 for _, live in blocks} == {True, False}
    # more than kCamMaxC = 8 classes: a second launch at out[8:], the class numbers in the caller's order
    from gnm._cabi import lib
    step = int(lib.gnm_class_activation_max_classes())
    assert step == 8 and all(len(cl) > step for cl in T.CLASS_LISTS)
    assert T.CLASS_LISTS[0][step:] != tuple(range(step, len(T.CLASS_LISTS[0])))
    # the input-width forms of the final dX launch
    table = {33: (2, 2), 64: (2, 2), 65: (3, 1), 96: (3, 1), 97: (4, 0), 128: (4, 0), 129: (5, 0)}
    assert {f0 for _, f0 in T.WIDTHS} == set(table)
    for f0, (nco, ks) in table.items():
        assert T.dx_form(f0)[:2] == (nco, ks), f0
    assert T.dx_form(33)[2] == "KS = 2" and T.dx_form(96)[2] == "KS = 1, 1 idle"
    assert T.dx_form(128)[2] == "wave per tile" and T.dx_form(129)[2] == "wave 0 takes 2 tiles"
    assert T.dx_form(7)[:2] == (1, 4) and T.dx_form(257)[0] == 9 and T.dx_form(400)[0] == 13   # what ran before
    assert {f0 % 32 for _, f0 in T.WIDTHS} == {0, 1}
    assert {(n, f0) for n, f0 in T.WIDTHS if n == 97} == {(97, 65), (97, 129)}
    assert T.row_blocks(40) == 2 and 40 - 32 == 8
    for nco in (2, 3, 4, 5):                                    # each NCO meets more than one H
        assert len({c.H for c in T.WIDTH_CASES if T.dx_form(c.F0)[0] == nco}) >= 2, nco
    for c in T.WIDTH_CASES:
        assert (c.H, c.m) in T.WIDTH_HM and c.F0 <= int(lib.gnm_linear_max_k(c.H)) and c.F0 <= 192
        assert c.K == T.WIDTH_STEPS == 2 and c.method == "midpoint" and not c.baseline and not c.one_hot
    assert int(lib.gnm_linear_max_k(128)) == 192
    assert len({(c.npool, c.gpool, c.eps) for c in T.WIDTH_CASES}) >= 6
    assert T.BATCH_CASE.n == 257 and len(T.batch_graphs()) == 3


def _check_graph(what, a64, a32, maps, caps, graph, learn_eps):
    """the conditions on one graph's references; returns {map: the fp32 reference's distance from fp64}"""
    out = {}
    for k in maps:
        x64, x32 = getattr(a64, k), getattr(a32, k)
        assert x64.dtype == np.float64 and x32.dtype == np.float32 and x64.shape == x32.shape, (what, k)
        assert np.isfinite(x64).all() and np.isfinite(x32).all(), (what, k)
        assert all(np.abs(x).max() > 0 for x in x64), (what, k)
        e = T.attr_noise(x32, x64)
        assert e <= caps[k], "%s: the fp32 %s reference is %.2e from fp64 (cap %.1e)" % (what, k, e, caps[k])
        assert T.attr_bound(x32, x64) <= 4 * caps[k]
        out[k] = e
    if "edge" in maps:                       # absent entries and the diagonal are part of the contract: non-trivial
        n = len(graph.g)
        em = np.asarray(graph.edge_mat)
        A = np.zeros((n, n), bool)
        A[em[0], em[1]] = True
        if not learn_eps:
            A[np.arange(n), np.arange(n)] = True
        for r in a64.edge:
            scale = np.abs(r).max()
            assert (~A).any() and np.abs(r[~A]).max() > 1e-3 * scale, what
            assert np.abs(np.diagonal(r)).max() > 1e-3 * scale, what
    return out


def _check_case(case, graphs, r64, r32, maps=T.MAPS, caps=CAPS):
    margin = T.relu_margin_of(T.state_of(case), T.spec_of(case), graphs)
    assert margin >= T.IG_RELU_MARGIN, "%s: a pre-activation at %.1e of its layer's largest" % (case.id, margin)
    worst = dict.fromkeys(maps, 0.0)
    for d, g in enumerate(graphs):
        e = _check_graph("%s graph %d" % (case.id, d), r64[d], r32[d], maps, caps, g, case.eps)
        worst = {k: max(worst[k], e[k]) for k in maps}
    return worst


@pytest.mark.parametrize("n", T.NODES)
def test_gradient_map_references_stay_within_the_conditions(n):
    worst = dict.fromkeys(T.MAPS, 0.0)
    for case in T.grad_cases(n):
        assert T.relu_margin(case) == T.relu_margin_of(T.state_of(case), T.spec_of(case), T.graphs_of(case))
        e = _check_case(case, T.graphs_of(case), T.attribution_reference(case),
                        T.attribution_reference(case, "float32"))
        worst = {k: max(worst[k], e[k]) for k in T.MAPS}
    print("n=%d: the fp32 references are at most %s from the fp64 ones (caps %s)" %
          (n, "  ".join("%s %.2e" % (k, worst[k]) for k in T.MAPS), "  ".join("%.0e" % CAPS[k] for k in T.MAPS)))


def test_the_three_named_cases_miss_the_margin_with_the_table_seed():
    """what GRAD_SEEDS is for: at the seed of the lesion / occlusion / integrated-gradients table these cases have a
    pre-activation under IG_RELU_MARGIN at their own features"""
    for cid in ("n190-H128-m1-sum-sum-eps1", "n256-H32-m2-average-sum-eps1", "n257-H64-m2-sum-sum-eps1"):
        case = next(c for n in T.NODES for c in T.cases(n) if c.id == cid)
        assert T.relu_margin(case) < T.IG_RELU_MARGIN <= T.relu_margin(T.grad_case(case)), cid


def test_the_restatement_and_the_oracle_share_the_forward():
    """the references come from two fp64 routes (OracleGIN for saliency, the torch restatements for the maps): pinned
    to each other where they meet -- the restatement's class activation map sums to the oracle's eval logit"""
    case = T.grad_cases(129)[0]
    st, sp = T.state_of(case), T.spec_of(case)
    logits = T.oracle_scores64(st, sp, T.graphs_of(case))
    for d, r in enumerate(T.attribution_reference(case)):
        for c in (0, 1):
            bias = sum(float(st["linears_prediction.%d.bias" % l][c]) for l in range(T.LAYERS))
            assert abs(r.cam[c].sum() + bias - logits[d, c]) <= PIN * (np.abs(r.cam[c]).sum() + abs(bias))


def test_the_further_cases_stay_within_the_conditions():
    """the ragged batch (33, 256, 257, 416 and 2 nodes), the third graph of the batch-size case and the 11-class cases
    under the same conditions"""
    c = T.grad_case(T.RAGGED_CASE)
    gs = T.ragged_graphs()
    assert [len(g.g) for g in gs] == list(T.RAGGED_NODES)
    assert not any(T.ig_declined(c, g) for g in gs)
    w = _check_case(c, gs, T.ragged_attribution_reference(), T.ragged_attribution_reference("float32"))
    print("ragged: %s" % w)
    c = T.grad_case(T.BATCH_CASE)
    gs = T.batch_graphs()
    assert not any(T.ig_declined(c, g) for g in gs)
    w = _check_case(c, gs, T.batch_attribution_reference(), T.batch_attribution_reference("float32"))
    print("batch sizes: %s" % w)
    for case in T.CLASS_CASES:
        c = T.grad_case(case)
        r64, r32 = T.class_attribution_reference(c), T.class_attribution_reference(c, "float32")
        assert r64[0].cam.shape == (11, c.n) and (r64[0].sal is not None) == (c.n == 129)
        w = _check_case(c, T.graphs_of(c), r64, r32, maps=T.class_maps(c))
        print("%s: %s" % (c.id, w))


@pytest.mark.parametrize("case", T.WIDTH_CASES, ids=[c.id for c in T.WIDTH_CASES])
def test_input_width_references_stay_within_the_conditions(case):
    c = T.grad_case(case)
    gs = T.graphs_of(c)
    assert [tuple(g.node_features.shape) for g in gs] == [(c.n, c.F0)] * 2
    em = [np.asarray(g.edge_mat) for g in gs]
    assert set(map(tuple, em[0].T)) == set(map(tuple, em[0][::-1].T))               # undirected
    assert set(map(tuple, em[1].T)) != set(map(tuple, em[1][::-1].T))               # directed
    assert not any(T.ig_declined(c, g) for g in gs)
    caps = dict.fromkeys(T.MAPS, WIDTH_CAP)
    w = _check_case(c, gs, T.attribution_reference(c, "float64", (0, 1), ("sal",)),
                    T.attribution_reference(c, "float32", (0, 1), ("sal",)), maps=("sal",), caps=caps)
    margin = T.ig_relu_margin(c)                                # ... and at integrated_gradients()' quadrature points
    assert margin >= T.IG_RELU_MARGIN, "%s: a pre-activation at %.1e of its layer's largest" % (c.id, margin)
    r64, r32 = T.ig_reference(c), T.ig_reference(c, "float32")
    for d in range(2):
        assert r64[d][0].shape == (2, c.n, c.F0) and np.isfinite(r64[d][0]).all() and np.abs(r64[d][0]).max() > 0
        e = rel_err(r32[d][0], r64[d][0])
        assert e <= WIDTH_CAP, "%s graph %d: the fp32 integrated gradients are %.2e from fp64" % (c.id, d, e)
        w["ig"] = max(w.get("ig", 0.0), e)
    assert 4 * max(w.values()) <= RTOL
    print("%s (%s): fp32 floors %s" % (c.id, T.dx_form(c.F0)[2], w))
