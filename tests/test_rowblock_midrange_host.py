"""The CPU half of the mid-range row-block tests (tests/rowblock_midrange_cases.py; the GPU half is
tests/test_gpu_rowblock_midrange.py).  Without a GPU:

  * the table reaches what it claims -- plain arithmetic from the kernels' constants (both half-row word-group sizes,
    the row-block counts, every residue mod 4 of rb_bits_product's per-wave step count at each H and a count of 5 or
    more, every pooling form with every n and every H);
  * the references alone stay within the conditions the GPU bounds rest on: on every finite lesion case the independent
    fp32 CPU forward (TorchCpuGIN) on the explicit deleted copy is within 5e-6 of the fp64 oracle, so the calibrated GPU
    bound max(1e-5, 4 x that distance) never exceeds 2e-5; the fp32 OracleGIN integrated gradients are within 2.5e-6 of
    the fp64 ones, so the flat 1e-5 is at least 4 x the fp32 floor, and no pre-activation under a ReLU sits within one
    fp32 ulp of zero at its layer's scale (rowblock_midrange_cases.IG_RELU_MARGIN: the gradient is not continuous
    there); NaN exactly where expect_nan says, in at most 3
    sets per graph, never in the empty set.  A seed that breaks a condition is changed
    (rowblock_midrange_cases.SEEDS); the condition is not;
  * the fast fp64 reference is pinned to the oracle: test_lesion_host.masked_forward64 (the kernel's formulation on the
    source graph) and its batched form masked_forward64_sets against the fp64 oracle on explicit copies, within 1e-12
    of max |base|, on every set of the table and on the named one-node sets -- which is what lets the GPU test check
    all n columns of occlusion() against the batched form."""
import numpy as np
import pytest

import rowblock_midrange_cases as T
from helpers import RTOL, rel_err
from test_lesion_host import masked_forward64

FP32_LESION_CAP = 5e-6
FP32_IG_CAP = 2.5e-6
PIN = 1e-12


def _all_cases():
    return [c for n in T.NODES for c in T.cases(n)]


def test_the_table_covers_what_it_claims():
    assert {T.half_words(n) for n in T.NODES} == {4, 8}
    assert T.half_words(256) == 4 and T.half_words(257) == 8 and max(T.NODES) == T.MAX_N
    assert {T.row_blocks(n) for n in T.NODES} == {4, 5, 6, 8, 9, 13}
    assert [(n + 15) // 16 for n in T.NODES] == [7, 9, 12, 16, 17, 26, 26]
    assert 401 - 32 * 12 == 17 and 32 * 13 - 401 == 15 and 416 == 32 * 13          # 15 dead rows / none
    for H in T.HS:
        counts = [k for n in T.NODES for k in T.wave_steps(n, H)]
        assert {k % 4 for k in counts} == {0, 1, 2, 3}, (H, counts)
        assert max(counts) >= 5, (H, counts)
    assert 6 in T.wave_steps(190, 64)
    assert T.wave_steps(416, 128) == [26] and T.wave_steps(416, 32) == [7, 7, 6, 6]
    for n in T.NODES:
        cs = T.cases(n)
        assert {(c.H, c.m) for c in cs} == {(H, m) for H in T.HS for m in T.MS}
        assert {(c.npool, c.gpool, c.eps) for c in cs} == set(T.POOLS), n
        assert all(c.n == n and c.F0 in (7, n) for c in cs)
        assert sum(c.npool == "average" and c.eps for c in cs if T.all_but_one_case(n) == c) == 1
    for H in T.HS:
        assert {(c.npool, c.gpool, c.eps) for c in _all_cases() if c.H == H} == set(T.POOLS), H
    onehot = [c for c in _all_cases() if c.one_hot]
    assert len(onehot) == 1 and onehot[0].n == 257 and onehot[0].F0 == 257 and 257 % 16 != 0
    assert {c.K for c in _all_cases()} == {1, 2, 5} and {c.method for c in _all_cases()} == set(T.METHODS)
    assert {c.baseline for c in _all_cases()} == {True, False}
    assert all(c.K >= 2 for c in _all_cases() if c.method == "trapezoid")
    assert len({c.id for c in _all_cases()}) == len(_all_cases())
    assert all(c.C == 11 for c in T.CLASS_CASES) and {c.n for c in T.CLASS_CASES} == {129, 257}
    assert all(len(cl) > 8 and max(cl) < 11 and len(set(cl)) == len(cl) for cl in T.CLASS_LISTS)
    assert T.CLASS_LISTS[0] != tuple(sorted(T.CLASS_LISTS[0]))
    assert {T.half_words(n) for n in T.RAGGED_NODES if n > 2} == {4, 8}


@pytest.mark.parametrize("n", T.NODES)
def test_graphs_and_sets_are_what_the_table_says(n):
    W = T.row_blocks(n)
    for case in T.cases(n):
        gs = T.graphs_of(case)
        em = [np.asarray(g.edge_mat) for g in gs]
        adj = [np.zeros((n, n), dtype=bool) for _ in gs]
        for A, e in zip(adj, em):
            A[e[0], e[1]] = True
            assert int(A.sum()) == e.shape[1] and not A.diagonal().any()            # no repeated edge, no self loop
        assert np.array_equal(adj[0], adj[0].T)                                     # undirected
        assert not np.array_equal(adj[1], adj[1].T)                                 # directed: the transposed bits differ
        fill = [e.shape[1] / float(n * n) for e in em]
        assert (min(fill) < 0.3 and max(fill) > 0.4) and (fill[0] < fill[1]) == (case.dens[0] < case.dens[1])
        declined = [T.ig_declined(case, g) for g in gs]
        assert not any(declined)                     # (a ring: no node without neighbours)
        for d in range(2):
            sets, names = T.lesion_sets(case, d)
            assert names[:5] == ["empty", "last-node", "block-0", "last-block", "block-2"]
            assert not sets[0].any() and sets[1].sum() == 1 and sets[1][n - 1]
            assert sets[2][:32].all() and sets[2].sum() == 32
            assert sets[3][32 * (W - 1):].all() and sets[3].sum() == n - 32 * (W - 1)
            assert sets[4][64:96].all() and sets[4].sum() == 32
            if n > 256:
                assert names[5:7] == ["255-256", "block-of-256"]
                assert np.nonzero(sets[5])[0].tolist() == [255, 256]
                assert sets[6][256:min(n, 288)].all() and sets[6].sum() == min(n, 288) - 256
            k = names.index("half")
            assert sets[k].sum() == n // 2 and sets[k + 1].sum() == int(0.8 * n)
            assert ("all-but-one" in names) == (d == 0 and case == T.all_but_one_case(n))
            if "all-but-one" in names:
                assert sets[-1].sum() == n - 1
            assert not sets.all(1).any()
    # the pooling forms integrated_gradients() declines on this n's graphs: at most 1 of the 8
    assert len({(c.npool, c.gpool, c.eps) for c in T.cases(n) if any(T.ig_declined(c, g) for g in T.graphs_of(c))}) <= 1


def test_the_library_and_the_table_agree_on_the_mask_width():
    """gnm_lesion_mask_words (the one place the library and gnm/core.py take a keep mask's width from) against this
    suite's independent copy of the half-row layout, at every node count the row-block kernels take"""
    from gnm._cabi import lib
    for n in range(1, 417):
        assert lib.gnm_lesion_mask_words(n) == 2 * T.half_words(n), n
    assert lib.gnm_lesion_mask_words(256) == 8 and lib.gnm_lesion_mask_words(257) == 16


def _check_lesion_conditions(what, want_nan, base64, base32, les64, les32, names=None):
    assert np.isfinite(base64).all() and np.isfinite(base32).all(), what
    nan64 = np.isnan(les64)
    assert (nan64.any(1) == want_nan).all() and (nan64.all(1) == want_nan).all(), (what, names, want_nan)
    assert np.array_equal(np.isnan(les32), nan64), what
    assert want_nan.sum() <= 3 and not want_nan[0], (what, names, want_nan)
    e = T.fp32_noise(base32, base64, les32, les64)
    assert e <= FP32_LESION_CAP, "%s: the fp32 CPU forward is %.2e from fp64" % (what, e)
    assert max(RTOL, 4 * e) <= 2e-5
    return e


@pytest.mark.parametrize("n", T.NODES)
def test_lesion_references_stay_within_the_conditions(n):
    worst = 0.0
    for case in T.cases(n):
        for d, r in enumerate(T.lesion_reference(case)):
            worst = max(worst, _check_lesion_conditions("%s graph %d" % (case.id, d), r.want_nan, r.base64, r.base32,
                                                        r.les64, r.les32, r.names))
        if case == T.all_but_one_case(n):
            assert T.lesion_reference(case)[0].want_nan[-1]                     # the guaranteed NaN row
    print("n=%d: the fp32 CPU forward is at most %.2e from the fp64 oracle (cap %.1e)" % (n, worst, FP32_LESION_CAP))


@pytest.mark.parametrize("n", T.NODES)
def test_integrated_gradients_references_stay_within_the_conditions(n):
    worst = 0.0
    for case in T.cases(n):
        r64, r32 = T.ig_reference(case), T.ig_reference(case, "float32")
        for d in range(2):
            assert np.isfinite(r64[d][0]).all() and np.abs(r64[d][0]).max() > 0
            e = rel_err(r32[d][0], r64[d][0])
            assert e <= FP32_IG_CAP, "%s graph %d: the fp32 oracle is %.2e from fp64" % (case.id, d, e)
            worst = max(worst, e)
        margin = T.ig_relu_margin(case)
        assert margin >= T.IG_RELU_MARGIN, "%s: a pre-activation at %.1e of its layer's largest" % (case.id, margin)
    assert 4 * worst <= RTOL
    print("n=%d: the fp32 integrated gradients are at most %.2e from the fp64 ones (cap %.1e)" % (n, worst, FP32_IG_CAP))


def _pin(state, spec, graph, sets, les64, named, scale):
    """masked_forward64 and masked_forward64_sets against the oracle on explicit copies: the sets with their scores
    les64, and the named one-node sets with theirs"""
    worst = 0.0
    n = len(graph.g)
    one = np.eye(n, dtype=bool)[named[0]]
    for S, ref in ((sets, les64), (one, named[1])):
        slow = np.stack([masked_forward64(state, spec, graph, D) for D in S])
        fast = T.masked_forward64_sets(state, spec, graph, S)
        worst = max(worst, T.err(slow, ref, scale), T.err(fast, ref, scale))
    return worst


@pytest.mark.parametrize("n", T.NODES)
def test_the_fast_reference_is_pinned_to_the_oracle(n):
    worst = 0.0
    for case in T.cases(n):
        st, sp = T.state_of(case), T.spec_of(case)
        for g, r, named in zip(T.graphs_of(case), T.lesion_reference(case), T.named_reference(case)):
            assert named[0] == [v for v in (0, 15, 16, 31, 32, 63, 64, 255, 256) if v < n - 1] + [n - 1]
            e = _pin(st, sp, g, r.sets, r.les64, named, float(np.abs(r.base64).max()))
            assert e <= PIN, "%s: masked_forward64 is %.2e from the oracle on explicit copies" % (case.id, e)
            worst = max(worst, e)
    print("n=%d: masked_forward64 and its batched form are at most %.2e from the oracle (pin %.0e)" % (n, worst, PIN))


def test_the_further_cases_stay_within_the_conditions():
    """the cases outside the per-n matrix -- 11 classes at n = 129 and 257, the ragged batch of 33, 256, 257, 416 and 2
    nodes -- under the same conditions and the same pin"""
    worst = pin = 0.0
    for case in T.CLASS_CASES:
        st, sp = T.state_of(case), T.spec_of(case)
        assert st["linears_prediction.0.weight"].shape[0] == 11
        for d, (g, r, named) in enumerate(zip(T.graphs_of(case), T.lesion_reference(case), T.named_reference(case))):
            assert r.les64.shape[1] == 11
            worst = max(worst, _check_lesion_conditions("%s graph %d" % (case.id, d), r.want_nan, r.base64, r.base32,
                                                        r.les64, r.les32, r.names))
            pin = max(pin, _pin(st, sp, g, r.sets, r.les64, named, float(np.abs(r.base64).max())))
    gs, sets, les, occs = T.ragged_reference()
    assert [len(g.g) for g in gs] == list(T.RAGGED_NODES) and [s.shape[0] for s in sets] == [1, 2, 3, 4, 5]
    st, sp = T.state_of(T.RAGGED_CASE), T.spec_of(T.RAGGED_CASE)
    for d, (g, S, (b64, b32, l64, l32, want), occ) in enumerate(zip(gs, sets, les, occs)):
        worst = max(worst, _check_lesion_conditions("ragged graph %d" % d, want, b64, b32, l64, l32))
        pin = max(pin, _pin(st, sp, g, S, l64, (occ.named, occ.named64), float(np.abs(b64).max())))
    assert np.isnan(occs[-1].named64).all()          # the 2-node graph under average + learned eps: a lone node left
    assert pin <= PIN, pin
    print("further cases: fp32 CPU forward at most %.2e from fp64; masked_forward64 at most %.2e" % (worst, pin))
