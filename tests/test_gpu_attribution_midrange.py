"""saliency(), class_activation() of both kinds and edge_saliency() between 97 and 416 nodes (csrc/saliency.hip,
csrc/cam.hip, csrc/edgesal.hip over csrc/gnm_rowblock.h) against fp64 references, on the case table of
tests/rowblock_midrange_cases.py: n in {97, 129, 190, 256, 257, 401, 416} x H in {32, 64, 128} x m in {1, 2, 3}, L = 3,
every pooling form, an undirected and a directed graph per case, classes (0, 1); and the input-width forms of the final dX
launch (F0 = 33 .. 129: NCO = 2 .. 5 column tiles) for saliency() and integrated_gradients().  What the shapes reach (words
1 .. 6 of the average correction's byte walk at both half-row layouts, the tile loop at W = 4 .. 13, the strip stride of a
larger batch-mate, the gradient map's read-modify-write and the kept per-layer S_l at those W, partly live 64-row blocks
and a second launch of the class activation kernel for more than 8 classes, each form of the dX launch) is stated and
checked in tests/test_attribution_midrange_host.py, with the conditions on the references the bounds here rest on.

References: OracleGIN.compute_saliency (saliency), test_cam_host.restate (both class activation kinds),
test_edge_saliency_host.restate_edge (edge saliency), oracle_ig (integrated gradients), all in fp64.  Bound:
helpers.Calibrated's rule, max(RTOL, 4 x err) with err the distance of the SAME reference computed in fp32 on the CPU from
the fp64 one on that graph -- at most 4e-5 (1.6e-4 for the activation kind) by the host test's caps, never a HIP output;
max-norm relative to the graph-and-class map's max |fp64|; no NaN anywhere.  Success means the kernel ran: edge_saliency()
and the gradient kind raise when they decline, the activation kind always runs csrc/cam.hip, and saliency()'s route is
asserted.

MEASURED on an MI355X (pytest -s prints them; also in DESIGN.md sections 3.7 - 3.9 and 3.13), per n = 97, 129, 190, 256,
257, 401, 416 the error that comes closest to its bound (bound 1e-5 unless stated):
  saliency()                        1.2e-6  6.8e-7  1.1e-6  8.5e-7  5.9e-7  7.4e-7  6.3e-7
  class_activation(), activation    3.9e-6 (bound 2.5e-5)  5.6e-6 (1.7e-5)  1.6e-5 (5.7e-5)  2.0e-5 (5.6e-5)  6.1e-6 (1.9e-5)
                                    8.2e-6 (2.2e-5)  3.3e-6; the fp32 CPU restatement is itself up to 1.4e-5 from fp64 there
                                    (the L layer terms of a node cancel), and the sum over nodes meets predict()'s logit
  class_activation(), gradient      1.3e-6  1.5e-6  1.2e-6  3.2e-6 (1.5e-5)  1.9e-6  1.3e-6  2.6e-6 (1.05e-5)
  edge_saliency()                   1.8e-6  1.3e-6  1.4e-6  1.4e-6  1.1e-6  1.2e-6  1.6e-6, absent entries and diagonal included
  the ragged batch (33, 256, 257, 416, 2 nodes), in the batch and alone: saliency 3.4e-7, activation 3.8e-7, gradient
  6.7e-7, edge 5.8e-7, bitwise run to run; batch sizes 1 and 3 at n = 257: 4.7e-7, 1.3e-6, 4.5e-7, 9.3e-7
  11 classes: n = 129 saliency 5.9e-7, activation 3.7e-6 (bound 1.8e-5), gradient 8.5e-7, edge 1.1e-6; n = 257 activation
  8.3e-6 (bound 2.8e-5), gradient 8.6e-7; every class bitwise the class asked for alone
  the dX launch at F0 = 33, 64, 65, 96, 97, 128, 129 (n = 40) and 65, 129 (n = 97):
    saliency()              2.1e-7  3.7e-7  5.8e-7  1.9e-7  2.6e-7  5.3e-7  2.3e-7;  5.4e-7  6.2e-7
    integrated_gradients()  2.7e-7  4.2e-7  5.7e-7  1.8e-7  2.2e-7  5.4e-7  4.1e-7;  6.2e-7  5.7e-7
At F0 = 129 integrated_gradients()' base was not predict()'s logit to the bit (dense features wider than the evaluation
encoder's 128 columns: the training kernels, where predict() takes layer 0's aggregate from the arena's cache and base
formed it per batch); _intgrad_batch now takes the cached aggregate as forward_batch does.
"""
import numpy as np
import pytest
import torch

import rowblock_midrange_cases as T
from helpers import RTOL, rel_err
from test_gpu_intgrad import worst_err
from test_gpu_rowblock_midrange import model_for

pytestmark = pytest.mark.gpu


class Worst:
    """the worst error seen, as a fraction of its bound, and what it was"""

    def __init__(self):
        self.e, self.b = 0.0, RTOL

    def see(self, e, b):
        if e / b > self.e / self.b:
            self.e, self.b = e, b

    def __str__(self):
        return "worst %.2e under %.2e" % (self.e, self.b)


def check_map(got, ref64, ref32, what, worst):
    """got [C, ...] (a tensor, or per-class tensors) of one graph against its references [C, ...]: every class within
    the graph's bound, relative to that class's max |ref64|; rel_err refuses a NaN"""
    got = np.stack([x.cpu().numpy() for x in got])
    assert got.shape == ref64.shape and got.dtype == np.float32, (what, got.shape, ref64.shape)
    bound = T.attr_bound(ref32, ref64)
    for ci in range(len(ref64)):
        e = rel_err(got[ci], ref64[ci])
        print("  %s class index %d: %.2e (bound %.2e)" % (what, ci, e, bound))
        assert e <= bound, "%s class index %d: %.3e > %.2e" % (what, ci, e, bound)
        worst.see(e, bound)
    return got


def check_edge_parts(got, ref64, ref32, graph, learn_eps, what):
    """as test_gpu_edge_saliency.check_edges: the absent entries and the diagonal of the reference are non-trivial, and
    they match under the same bound"""
    n = len(graph.g)
    em = np.asarray(graph.edge_mat)
    A = np.zeros((n, n), bool)
    A[em[0], em[1]] = True
    if not learn_eps:
        A[np.arange(n), np.arange(n)] = True
    off = ~A
    bound = T.attr_bound(ref32, ref64)
    for x, r in zip(got, ref64):
        scale = np.abs(r).max()
        assert off.any() and np.abs(r[off]).max() > 1e-3 * scale, what
        assert np.abs(x[off] - r[off]).max() <= bound * scale, what
        assert np.abs(np.diagonal(r)).max() > 1e-3 * scale, what
        assert np.abs(np.diagonal(x) - np.diagonal(r)).max() <= bound * scale, what


def check_logit(model, cam, logits, classes, what):
    """sum_v cam[v] + sum_l bias_l[c] is the eval logit (test_gpu_class_activation.test_activation_sums_to_the_eval_logit)"""
    L = len(model.linears_prediction)
    for ci, c in enumerate(classes):
        bias = [float(model.linears_prediction[l].bias[c].detach()) for l in range(L)]
        total = float(cam[ci].double().sum()) + sum(bias)
        bound = RTOL * (float(cam[ci].double().abs().sum()) + sum(abs(b) for b in bias))
        assert abs(total - float(logits[c])) <= bound, (what, c, total, float(logits[c]), bound)


def per_graph(res, d):
    """graph d's [C, ...] of a method's result for a sequence of classes, dense or lists"""
    return [res[ci][d] for ci in range(len(res))]


# ---------------------------------------------------------------------------------------------- the matrix
@pytest.mark.parametrize("n", T.NODES)
def test_saliency(n):
    worst = Worst()
    for case in T.grad_cases(n):
        model, gs = model_for(case), T.graphs_of(case)
        r64, r32 = T.attribution_reference(case), T.attribution_reference(case, "float32")
        got = model.saliency(gs, (0, 1))
        assert model.saliency_routes == ["hip"]
        assert got.shape == (2, 2, n, case.F0) and got.dtype == torch.float32
        for d in range(2):
            check_map(got[:, d], r64[d].sal, r32[d].sal, "%s graph %d" % (case.id, d), worst)
    print("saliency n=%d: %s" % (n, worst))


@pytest.mark.parametrize("n", T.NODES)
def test_class_activation(n):
    wa, wg = Worst(), Worst()
    for case in T.grad_cases(n):
        model, gs = model_for(case), T.graphs_of(case)
        r64, r32 = T.attribution_reference(case), T.attribution_reference(case, "float32")
        cam = model.class_activation(gs, (0, 1))
        gcam = model.class_activation(gs, (0, 1), kind="gradient")
        assert cam.shape == gcam.shape == (2, 2, n)
        logits = model.predict(gs)
        for d in range(2):
            check_map(cam[:, d], r64[d].cam, r32[d].cam, "%s activation graph %d" % (case.id, d), wa)
            check_map(gcam[:, d], r64[d].gcam, r32[d].gcam, "%s gradient graph %d" % (case.id, d), wg)
            check_logit(model, cam[:, d], logits[d], (0, 1), "%s graph %d" % (case.id, d))
    print("class_activation n=%d: activation %s, gradient %s" % (n, wa, wg))


@pytest.mark.parametrize("n", T.NODES)
def test_edge_saliency(n):
    worst = Worst()
    for case in T.grad_cases(n):
        model, gs = model_for(case), T.graphs_of(case)
        r64, r32 = T.attribution_reference(case), T.attribution_reference(case, "float32")
        got = model.edge_saliency(gs, (0, 1))
        assert got.shape == (2, 2, n, n) and got.dtype == torch.float32
        for d in range(2):
            what = "%s graph %d" % (case.id, d)
            x = check_map(got[:, d], r64[d].edge, r32[d].edge, what, worst)
            check_edge_parts(x, r64[d].edge, r32[d].edge, gs[d], case.eps, what)
    print("edge_saliency n=%d: %s" % (n, worst))


# ---------------------------------------------------------------------------------------------- further cases
def _four_methods(model, gs, classes, **kw):
    """{map: result} of the four methods on one list of graphs"""
    return dict(sal=model.saliency(gs, classes, **kw), cam=model.class_activation(gs, classes, **kw),
                gcam=model.class_activation(gs, classes, kind="gradient", **kw),
                edge=model.edge_saliency(gs, classes, **kw))


def _same_bits(a, b):
    if torch.is_tensor(a):
        return torch.equal(a, b)
    return len(a) == len(b) and all(_same_bits(x, y) for x, y in zip(a, b))


def test_ragged_batch_across_the_word_group_boundary():
    """graphs of 33, 256, 257, 416 and 2 nodes in one call of each method: both half-row word-group sizes, the edge
    kernel's LDS strip stride and tile count sized by the 416-node batch-mate.  Every graph within its bound, in the
    batch and alone; the call repeated gives the same bits"""
    case = T.grad_case(T.RAGGED_CASE)
    model, gs = model_for(case), T.ragged_graphs()
    r64, r32 = T.ragged_attribution_reference(), T.ragged_attribution_reference("float32")
    got = _four_methods(model, gs, (0, 1))
    assert model.saliency_routes == ["hip"]
    again = _four_methods(model, gs, (0, 1))
    worst = {k: Worst() for k in T.MAPS}
    for k in T.MAPS:
        assert isinstance(got[k], list) and len(got[k]) == 2 and _same_bits(got[k], again[k]), k
    for d, g in enumerate(gs):
        n = len(g.g)
        alone = _four_methods(model, [g], (0, 1))
        assert tuple(got["edge"][0][d].shape) == (n, n) and tuple(got["sal"][0][d].shape) == (n, T.F0)
        for k in T.MAPS:
            what = "ragged %s, %d nodes" % (k, n)
            x = check_map(per_graph(got[k], d), getattr(r64[d], k), getattr(r32[d], k), what, worst[k])
            y = check_map(alone[k][:, 0], getattr(r64[d], k), getattr(r32[d], k), what + " alone", worst[k])
            if k == "edge":
                check_edge_parts(x, r64[d].edge, r32[d].edge, g, case.eps, what)
                check_edge_parts(y, r64[d].edge, r32[d].edge, g, case.eps, what + " alone")
    print("ragged batch: " + "; ".join("%s %s" % (k, worst[k]) for k in T.MAPS))


@pytest.mark.parametrize("case", T.CLASS_CASES, ids=[c.id for c in T.CLASS_CASES])
def test_more_than_eight_classes(case):
    """11 classes, asked for as a shuffled 10-tuple and as all 11: class_activation_hip runs a second launch of
    gnm_class_activation that writes at out[8:] with the class numbers in the caller's order; the gradient kind,
    saliency() and edge_saliency() (n = 129, the shuffled tuple) run their launches per class.  Per class against fp64,
    and bitwise the class asked for alone"""
    case = T.grad_case(case)
    model, gs = model_for(case), T.graphs_of(case)
    r64, r32 = T.class_attribution_reference(case), T.class_attribution_reference(case, "float32")
    worst = {k: Worst() for k in T.class_maps(case)}

    def run(k, classes):
        if k == "sal":
            res = model.saliency(gs, classes)
            assert model.saliency_routes == ["hip"]
            return res
        if k == "edge":
            return model.edge_saliency(gs, classes)
        return model.class_activation(gs, classes, kind="activation" if k == "cam" else "gradient")

    for k in T.class_maps(case):
        single = {c: run(k, c) for c in range(case.C)}
        for cl in (T.CLASS_LISTS if k in ("cam", "gcam") else T.CLASS_LISTS[:1]):
            got = run(k, cl)
            assert got.shape[:2] == (len(cl), 2)
            for ci, c in enumerate(cl):
                assert torch.equal(got[ci], single[c]), (k, cl, c)
            for d in range(2):
                pick = list(cl)
                check_map(got[:, d], getattr(r64[d], k)[pick], getattr(r32[d], k)[pick],
                          "%s %s graph %d" % (case.id, k, d), worst[k])
    logits = model.predict(gs)
    cam = model.class_activation(gs, T.CLASS_LISTS[1])
    for d in range(2):
        check_logit(model, cam[:, d], logits[d], T.CLASS_LISTS[1], "%s graph %d" % (case.id, d))
    print("%s: %s" % (case.id, "; ".join("%s %s" % (k, worst[k]) for k in worst)))


def test_batch_sizes_at_eight_half_row_words():
    """3 graphs of 257 nodes at batch_size 1 and 3 (and the default, one batch): every result within its bound"""
    case = T.grad_case(T.BATCH_CASE)
    model, gs = model_for(case), T.batch_graphs()
    r64, r32 = T.batch_attribution_reference(), T.batch_attribution_reference("float32")
    worst = {k: Worst() for k in T.MAPS}
    for bs in (1, 3):
        got = _four_methods(model, gs, (0, 1), batch_size=bs)
        assert model.saliency_routes == ["hip"] * (3 if bs == 1 else 1)
        for d, g in enumerate(gs):
            for k in T.MAPS:
                what = "batch_size %d %s graph %d" % (bs, k, d)
                x = check_map(got[k][:, d], getattr(r64[d], k), getattr(r32[d], k), what, worst[k])
                if k == "edge":
                    check_edge_parts(x, r64[d].edge, r32[d].edge, g, case.eps, what)
    print("batch sizes 1 and 3: " + "; ".join("%s %s" % (k, worst[k]) for k in T.MAPS))


# ---------------------------------------------------------------------------------------------- the final dX launch
@pytest.mark.parametrize("case", T.WIDTH_CASES, ids=[c.id for c in T.WIDTH_CASES])
def test_input_width_forms_of_the_dx_launch(case):
    """saliency() and integrated_gradients(steps=2) at F0 = 33 .. 129: the final launch of gnm_saliency and of
    gnm_integrated_gradients with 2 .. 5 column tiles (two waves per tile, three waves and an idle one, a wave per
    tile, wave 0 on two tiles) and a column tail of 1 or none"""
    case = T.grad_case(case)
    model, gs = model_for(case), T.graphs_of(case)
    r64 = T.attribution_reference(case, "float64", (0, 1), ("sal",))
    r32 = T.attribution_reference(case, "float32", (0, 1), ("sal",))
    ws, wi = Worst(), Worst()
    got = model.saliency(gs, (0, 1))
    assert model.saliency_routes == ["hip"] and got.shape == (2, 2, case.n, case.F0)
    for d in range(2):
        check_map(got[:, d], r64[d].sal, r32[d].sal, "%s saliency graph %d" % (case.id, d), ws)
    attr, base, _, _ = model.integrated_gradients(gs, (0, 1), steps=T.WIDTH_STEPS, return_scores=True)
    assert attr.shape == (2, 2, case.n, case.F0) and attr.dtype == torch.float32
    i64, i32 = T.ig_reference(case), T.ig_reference(case, "float32")
    for d in range(2):
        check_map(attr[:, d], i64[d][0], i32[d][0], "%s integrated gradients graph %d" % (case.id, d), wi)
    assert worst_err(attr, i64) <= max(T.attr_bound(i32[d][0], i64[d][0]) for d in range(2))
    assert torch.equal(base, model.predict(gs)[:, [0, 1]].t())
    print("%s (%s): saliency %s, integrated gradients %s" % (case.id, T.dx_form(case.F0)[2], ws, wi))
