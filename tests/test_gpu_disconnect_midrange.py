"""disconnect() and disconnection_matrix() between 97 and 416 nodes (csrc/disconnect.hip, rb_stage_bits_cut of
csrc/gnm_rowblock.h) against the fp64 oracle on explicit edge-cut copies, on the case table of
tests/rowblock_midrange_cases.py: n in {97, 129, 190, 256, 257, 401, 416} x H in {32, 64, 128} x m in {1, 2, 3}, L = 3,
every pooling form, an undirected and a directed graph per case, sparse and dense, and the one-hot case of n = 257; one
test per case.  The pairs (rowblock_midrange_cases.disconnect_pairs) name rows by the fields of the per-row membership
lookup rb_row_bit -- word, half, byte -- which a lesion never makes: words 2 and 3 of a half row at HPW = 4 (n = 129 ..
256), words 4 .. 6 at HPW = 8, dead rows behind full blocks, up to 26 steps of rb_bits_product per wave at every H, the
layer-0 short cut of m = 1.  What the pairs reach, the conditions on the references and the wrong formulations they tell
apart (each at least 1e-4 of max |base| from the right one on every case: 5 x the largest bound here) are stated and
checked in tests/test_disconnect_midrange_host.py.

Bound: helpers.Calibrated, max(RTOL, 4 x err) with err the distance of the independent fp32 CPU forward (TorchCpuGIN)
from the fp64 oracle ON THE SAME CUT COPIES -- at most 2e-5 by the host test's cap, never a HIP output; on base and
disconnected, max-norm relative to the graph's max |base|; NaN exactly in the pairs expect_nan_cut marks.

MEASURED on an MI355X (pytest -s prints them; also in DESIGN.md section 3.15), the error that comes closest to its bound
per n = 97, 129, 190, 256, 257, 401, 416 (bound 1e-5 unless stated):
  disconnect()              5.8e-7  7.0e-7  4.7e-7  8.0e-7  2.3e-6 (bound 1.46e-5: H = 32, m = 2, average / sum, no learned
                            eps, where the fp32 CPU forward is 3.6e-6 from fp64)  6.4e-7  5.6e-7
  disconnection_matrix()    1.8e-7  2.7e-7  3.1e-7  1.5e-7  5.1e-7  3.8e-7  4.2e-7
  11 classes                5.2e-7 (n = 129) and 3.7e-7 (n = 257), every class bitwise the class asked for alone
With rb_row_bit's word index, or the in_b select of rb_stage_bits_cut, made wrong for words 2 and 3 at HPW = 4 in a
scratch build, all 31 tests here at n = 129, 190 and 256 failed (errors 4.0e-4 .. 1.5e-1, or the NaN pattern) while every
test of tests/test_gpu_disconnect.py still passed.
disconnect(b, a) is disconnect(a, b) to the bit on every case.
"""
import numpy as np
import pytest
import torch

import rowblock_midrange_cases as T
import test_gpu_disconnect as DC
from helpers import Calibrated
from test_gpu_rowblock_midrange import model_for

pytestmark = pytest.mark.gpu
CASES = T.all_dc_cases()
MATRIX_CASES = tuple(T.dc_matrix_case(n) for n in T.NODES)
CLASS_CASES = tuple(T.dc_case(c) for c in T.CLASS_CASES)
WORST = {}                                        # (what, n) -> (error, bound): the one closest to its bound so far


def check_disconnect(got, d, r, classes=None):
    """graph d of test_gpu_disconnect.run()'s result against its DisconnectRef; returns (worst error, bound)"""
    cl = list(range(r.base64.shape[0])) if classes is None else list(classes)
    cal = Calibrated()
    scale = float(np.abs(r.base64).max())
    cal.check(got[1][:, d], r.base32[cl], r.base64[cl], "base", floor=scale)
    cal.check(got[2][d], r.dis32[:, cl], r.dis64[:, cl], "disconnected", floor=scale)
    nan = np.isnan(got[2][d])
    assert (nan.any(1) == r.want_nan).all() and (nan.all(1) == r.want_nan).all()
    return max(e for _, e, _, _ in cal.log), cal.log[-1][3]


def report(what, case, d, e, b):
    print("  %s %s graph %d: %.2e (bound %.2e)" % (what, case.id, d, e, b))
    w = WORST.get((what, case.n))
    if w is None or e / b > w[0] / w[1]:
        WORST[what, case.n] = (e, b)
    print("  %s n=%d: worst so far %.2e under %.2e" % ((what, case.n) + WORST[what, case.n]))


def test_the_cases_are_the_table():
    assert len(CASES) == 64 and [c.n for c in MATRIX_CASES] == list(T.NODES)
    assert sum(c.one_hot for c in CASES) == 1 and {(c.H, c.m) for c in MATRIX_CASES} == {(64, 2)}


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_disconnect(case):
    model, gs, refs = model_for(case), T.graphs_of(case), T.disconnect_reference(case)
    pa, pb = [r.a for r in refs], [r.b for r in refs]
    got = DC.run(model, gs, pa, pb, batch_size=3)                                  # (delta = base - disconnected bitwise)
    for d, r in enumerate(refs):
        e, b = check_disconnect(got, d, r)
        report("disconnect", case, d, e, b)
    rev = DC.run(model, gs, pb, pa, batch_size=3)
    assert np.array_equal(rev[1], got[1])
    for d in range(2):
        assert np.array_equal(rev[2][d], got[2][d], equal_nan=True), "disconnect(b, a) is not disconnect(a, b)"


@pytest.mark.parametrize("case", MATRIX_CASES, ids=[c.id for c in MATRIX_CASES])
def test_disconnection_matrix(case):
    """a 5-network labelling per graph with some nodes of no network: [C, G, 5, 5], symmetric, bitwise the matching
    disconnect() pairs of gnm.lesion.pair_sets, within the bound of the fp64 oracle on the 15 cut copies"""
    from gnm.lesion import pair_sets
    model, gs, refs = model_for(case), T.graphs_of(case), T.matrix_reference(case)
    K = T.MATRIX_NETWORKS
    labs = [T.matrix_labels(case, d) for d in range(2)]
    delta, base, scores = model.disconnection_matrix(gs, (0, 1), labs, batch_size=3, return_scores=True)
    assert delta.shape == scores.shape == (2, 2, K, K) and base.shape == (2, 2) and scores.dtype == torch.float32
    assert torch.equal(DC.nn7(delta), DC.nn7(base[:, :, None, None] - scores))
    assert torch.equal(DC.nn7(scores), DC.nn7(scores.transpose(-1, -2)))
    assert torch.equal(DC.nn7(delta), DC.nn7(delta.transpose(-1, -2)))
    pairs = pair_sets(labs[0], K)[2]
    assert len(pairs) == 15 and all(np.array_equal(pair_sets(lab, K)[0], r.a) for lab, r in zip(labs, refs))
    flat = DC.run(model, gs, [r.a for r in refs], [r.b for r in refs], batch_size=3)
    assert np.array_equal(flat[1], base.cpu().numpy())
    for d, r in enumerate(refs):
        mat = scores[:, d, pairs[:, 0], pairs[:, 1]].t().cpu().numpy()             # [15, C]
        assert np.array_equal(mat, flat[2][d], equal_nan=True)
        e, b = check_disconnect(flat, d, r)
        report("disconnection_matrix", case, d, e, b)


@pytest.mark.parametrize("case", CLASS_CASES, ids=[c.id for c in CLASS_CASES])
def test_more_than_eight_classes(case):
    """11 classes, asked for as a shuffled 10-tuple and as all 11: the finish kernel runs a second launch that writes at
    out + 8 ldo.  Per class against the fp64 oracle, and bitwise the classes asked for one at a time."""
    model, gs, refs = model_for(case), T.graphs_of(case), T.disconnect_reference(case)
    pa, pb = [r.a for r in refs], [r.b for r in refs]
    single = {c: DC.run(model, gs, pa, pb, classes=(c,)) for c in range(11)}
    for cl in T.CLASS_LISTS:
        got = DC.run(model, gs, pa, pb, classes=cl)
        for d, r in enumerate(refs):
            e, b = check_disconnect(got, d, r, classes=cl)
            report("11 classes", case, d, e, b)
            for ci, c in enumerate(cl):
                assert got[1][ci, d] == single[c][1][0, d]
                assert np.array_equal(got[2][d][:, ci], single[c][2][d][:, 0], equal_nan=True), (cl, c, d)
