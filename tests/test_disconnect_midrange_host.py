"""The CPU half of the mid-range disconnect() tests (the disconnect section of tests/rowblock_midrange_cases.py; the GPU
half is tests/test_gpu_disconnect_midrange.py).  Every check here is judged by CPU references alone.

What a cut has that a lesion has not is a lookup per ROW: rb_stage_bits_cut (csrc/gnm_rowblock.h) decides whether row r is
in A or in B with rb_row_bit on the two keep masks, word ((r >> 3) & 1) * HPW + (r >> 6), bit (((r >> 4) & 3) << 3) +
(r & 7).  The words that lookup reads for rows of some proper set A or B of the table, and the dead rows r >= n of the last
row block (they reach the r < n guards, rc = min(r, n - 1), the unmasked staging and vr / vrow):

  n    HPW  words read for rows of the sets               dead rows
  97    4   0 1 | 4 5                                      31
  129   4   0 1 2 | 4 5          (word 2: row 128 alone)   31
  190   4   0 1 2 | 4 5 6                                   2
  256   4   0 1 2 3 | 4 5 6 7                               0
  257   8   0 1 2 3 4 | 8 9 10 11  (word 4: row 256 alone) 31
  401   8   0 .. 6 | 8 .. 14                               15
  416   8   0 .. 6 | 8 .. 14                                0

so n = 129 .. 256 reaches words 2 and 3 of a half row at HPW = 4 -- which no test of tests/test_gpu_disconnect.py does --
and n > 256 words 4 .. 6 at HPW = 8.

  * Structure: the table above, the pairs of disconnect_pairs(), and every non-empty pair cuts an edge of its graph.
  * The formulation: test_disconnect_host.cut_forward64 (what the kernel computes, on the source graph) and its form
    for any keep matrix, keep_forward64, are within 1e-12 of the fp64 oracle on explicit cut copies on every finite pair
    of every case, NaN exactly where expect_nan_cut says.
  * The NaN share: NaN only under neighbour average with learned eps, only where expect_nan_cut says, always for
    "last-node x all" and "all x all", possibly for "half x complement", for no other pair: at most 3 pairs per graph
    (67 of the table's 1648 pairs).
  * Conditioning: the independent fp32 CPU forward is within FP32_LESION_CAP = 5e-6 of the fp64 oracle on every graph
    and its finite cut copies, so the calibrated GPU bound max(RTOL, 4 x that) never exceeds 2e-5.  Worst per n = 97 ..
    416: 5.4e-7, 5.9e-7, 4.9e-7, 3.1e-6, 4.3e-6, 1.9e-6, 1.3e-6.  A case over the cap would get another model seed
    (rowblock_midrange_cases.DC_SEEDS); none needed one.
  * Discriminating power: six wrong formulations of the cut (rowblock_midrange_cases.disconnect_mutants: the masks
    swapped, a one-sided cut, the row membership bits or the column mask bits of the high words lost, the membership
    read from the other half row, the degree of the uncut row) each differ from the right one by at least MUTANT_FLOOR =
    1e-4 of max |base| on some finite pair of EVERY case they apply to -- 5 x the largest GPU bound, so a kernel that
    computes one of them cannot pass.  Smallest separations over the table: row bits lost 1.9e-4 (n = 257: row 256
    alone), column bits lost 6.1e-4, the other half 4.1e-3, one-sided 6.4e-3, swapped 7.3e-3, degree 1.6e-2."""
import numpy as np
import pytest

import rowblock_midrange_cases as T
from helpers import RTOL, rel_err
from test_disconnect_host import cut_forward64
from test_rowblock_midrange_host import FP32_LESION_CAP, PIN

MUTANT_FLOOR = 1e-4
MAY_BE_NAN = ("last-node x all", "half x complement", "all x all")
# n: (HPW, the words rb_row_bit reads for rows of the table's proper sets, dead rows of the last block)
STRUCTURE = {
    97: (4, {0, 1, 4, 5}, 31),
    129: (4, {0, 1, 2, 4, 5}, 31),
    190: (4, {0, 1, 2, 4, 5, 6}, 2),
    256: (4, {0, 1, 2, 3, 4, 5, 6, 7}, 0),
    257: (8, {0, 1, 2, 3, 4, 8, 9, 10, 11}, 31),
    401: (8, set(range(7)) | set(range(8, 15)), 15),
    416: (8, set(range(7)) | set(range(8, 15)), 0),
}


def test_the_table_reaches_the_row_lookup_it_claims():
    assert set(STRUCTURE) == set(T.NODES)
    assert len(T.all_dc_cases()) == 64 and len({c.id for c in T.all_dc_cases()}) == 64
    assert set(T.DC_SEEDS) <= {c.id for n in T.NODES for c in T.cases(n)} | {c.id for c in T.CLASS_CASES}
    for n in T.NODES:
        hpw, words, dead = STRUCTURE[n]
        assert T.half_words(n) == hpw and 32 * T.row_blocks(n) - n == dead
        case = T.dc_cases(n)[0]
        seen = set()
        for d in range(2):
            names, a, b = T.disconnect_pairs(case, d)
            for S in np.concatenate([a, b]):
                if not S.all():
                    seen |= {T.row_bit_word(n, int(r)) for r in np.nonzero(S)[0]}
        assert seen == words, (n, sorted(seen))
        assert words == {T.row_bit_word(n, r) for r in range(n)}            # (the lookup of all x all reads no other)
        in_half = {w % hpw for w in words}
        if 129 <= n <= 256:
            assert hpw == 4 and 2 in in_half
        if n > 256:
            assert hpw == 8 and 4 in in_half
    assert 3 in {w % 4 for w in STRUCTURE[256][1]} and 6 in {w % 8 for w in STRUCTURE[401][1]}
    assert [n for n in T.NODES if STRUCTURE[n][2]] == [97, 129, 190, 257, 401]
    for n in T.NODES:                            # disconnection_matrix(): one case per n; 11 classes above 70 nodes
        c = T.dc_matrix_case(n)
        assert (c.n, c.H, c.m, c.one_hot) == (n, 64, 2, False)
    assert [(c.n, c.H, c.C) for c in T.CLASS_CASES] == [(129, 64, 11), (257, 128, 11)]


@pytest.mark.parametrize("n", T.NODES)
def test_pairs_are_what_the_table_says(n):
    from gnm.lesion import cut_edge_counts
    W = T.row_blocks(n)
    idx = np.arange(n)
    edges = [e for e in T.WORD_EDGES if n > e + 1]
    for case in T.dc_cases(n):
        for d, g in enumerate(T.graphs_of(case)):
            names, a, b = T.disconnect_pairs(case, d)
            assert a.shape == b.shape == (len(names), n) and a.dtype == b.dtype == np.bool_
            assert names[:7] == ["empty", "last-node x all", "block-0 x block-1", "block-%d x block-%d" % (W - 2, W - 1),
                                 "block-2 within itself", "half rows", "bytes"]
            assert names[7:] == ["word edge %d" % e for e in edges] + ["half x complement", "overlapping random sets",
                                                                       "all x all"]
            assert not a[0].any() and not b[0].any()
            assert np.nonzero(a[1])[0].tolist() == [n - 1] and b[1].all()
            assert np.array_equal(a[2], idx < 32) and np.array_equal(b[2], (idx >= 32) & (idx < 64))
            assert np.array_equal(a[3], idx >> 5 == W - 2) and np.array_equal(b[3], idx >> 5 == W - 1) and b[3].any()
            assert np.array_equal(a[4], idx >> 5 == 2) and np.array_equal(b[4], a[4])
            assert np.array_equal(a[5], ~b[5]) and a[5][:8].all() and b[5][8:16].all() and a[5][16]
            assert a[6][16:32].all() and b[6][48:64].all() and not (a[6] | b[6])[:16].any() and not (a[6] & b[6]).any()
            for k, e in enumerate(edges):
                assert np.nonzero(a[7 + k])[0].tolist() == [e, e + 1]
                assert np.nonzero(b[7 + k])[0].tolist() == list(range(32)) + sorted({e + 1, min(e + 2, n - 1)})
            k = 7 + len(edges)
            assert a[k].sum() == n // 2 and np.array_equal(b[k], ~a[k])
            assert (a[k + 1] & b[k + 1]).any() and (a[k + 1] & ~b[k + 1]).any() and (b[k + 1] & ~a[k + 1]).any()
            assert a[k + 2].all() and b[k + 2].all() and k + 3 == len(names)
            cnt = cut_edge_counts(g.edge_mat, a, b)
            assert cnt[0] == 0 and cnt[1:].min() > 0, (case.id, d, cnt)           # every non-empty pair cuts an edge
            assert cnt[-1] == np.asarray(g.edge_mat).shape[1]
    if n == 257:                                 # row 256 alone -- word 4, the second 128-bit load -- is named by the
        named = [s for s in range(len(names)) if a[s][256] and not a[s].all() and a[s].sum() <= 2]      # word edge only
        assert [names[s] for s in named] == ["last-node x all", "word edge 255"]


def _check_conditions(what, r):
    assert np.isfinite(r.base64).all() and np.isfinite(r.base32).all(), what
    nan64 = np.isnan(r.dis64)
    assert (nan64.any(1) == r.want_nan).all() and (nan64.all(1) == r.want_nan).all(), (what, r.names, r.want_nan)
    assert np.array_equal(np.isnan(r.dis32), nan64), what
    e = T.fp32_noise(r.base32, r.base64, r.dis32, r.dis64)
    assert e <= FP32_LESION_CAP, "%s: the fp32 CPU forward is %.2e from fp64" % (what, e)
    assert max(RTOL, 4 * e) <= 2e-5
    return e


def _check_nan_share(case, r):
    nan = [k for k, w in zip(r.names, r.want_nan) if w]
    if not (case.npool == "average" and case.eps):
        assert not nan, (case.id, nan)
        return 0
    assert set(nan) <= set(MAY_BE_NAN) and len(nan) <= 3, (case.id, nan)
    assert "last-node x all" in nan and "all x all" in nan, (case.id, nan)
    return len(nan)


@pytest.mark.parametrize("n", T.NODES)
def test_disconnect_references_stay_within_the_conditions(n):
    worst, nans, pairs = 0.0, 0, 0
    for case in T.dc_cases(n):
        for d, r in enumerate(T.disconnect_reference(case)):
            worst = max(worst, _check_conditions("%s graph %d" % (case.id, d), r))
            nans += _check_nan_share(case, r)
            pairs += len(r.names)
    assert pairs == 2 * len(T.dc_cases(n)) * (10 + sum(n > e + 1 for e in T.WORD_EDGES))
    print("n=%d: the fp32 CPU forward is at most %.2e from the fp64 oracle on the cut copies (cap %.1e); %d of %d pairs NaN"
          % (n, worst, FP32_LESION_CAP, nans, pairs))


def test_the_nan_share_of_the_whole_table():
    refs = [r for c in T.all_dc_cases() for r in T.disconnect_reference(c)]
    assert (sum(int(r.want_nan.sum()) for r in refs), sum(len(r.names) for r in refs)) == (67, 1648)
    assert max(int(r.want_nan.sum()) for r in refs) == 3


def _finite_pairs(case):
    """(graph, its DisconnectRef, the indices of its finite pairs, max |base|) per graph of a case"""
    for g, r in zip(T.graphs_of(case), T.disconnect_reference(case)):
        yield g, r, np.nonzero(~r.want_nan)[0], float(np.abs(r.base64).max())


@pytest.mark.parametrize("n", T.NODES)
def test_the_formulation_is_pinned_to_the_oracle(n):
    """cut_forward64, and keep_forward64 on cut_keep(A, B), against the fp64 oracle on explicit cut copies"""
    worst = 0.0
    for case in T.dc_cases(n):
        st, sp = T.state_of(case), T.spec_of(case)
        for g, r, fin, scale in _finite_pairs(case):
            slow = np.stack([cut_forward64(st, sp, g, A, B) for A, B in zip(r.a, r.b)])
            fast = T.keep_forward64(st, sp, g, np.stack([T.cut_keep(A, B) for A, B in zip(r.a, r.b)]))
            for got in (slow, fast):
                assert np.isnan(got[r.want_nan]).all() and np.isfinite(got[fin]).all(), case.id
                e = rel_err(got[fin], r.dis64[fin], floor=scale)
                assert e <= PIN, "%s: the row-mask formulation is %.2e from the oracle on explicit copies" % (case.id, e)
                worst = max(worst, e)
    print("n=%d: cut_forward64 and keep_forward64 are at most %.2e from the oracle (pin %.0e)" % (n, worst, PIN))


def mutant_separations(case):
    """per mutant that applies to the case: the largest distance from the right formulation over the finite pairs of its
    two graphs, relative to the graph's max |base| (a NaN where the right score is finite: inf)"""
    st, sp = T.state_of(case), T.spec_of(case)
    sep = {}
    for g, r, fin, scale in _finite_pairs(case):
        right = T.keep_forward64(st, sp, g, np.stack([T.cut_keep(r.a[s], r.b[s]) for s in fin]))
        muts = [T.disconnect_mutants(r.a[s], r.b[s], case.n) for s in fin]
        for k in T.MUTANTS:
            if k == "degree of the uncut row" and case.npool != "average":
                continue                         # (no degree without the neighbour average)
            if k.endswith("high words lost") and case.n <= 128:
                continue                         # (no row from 128 on: a half row has words 0 and 1 alone)
            got = T.keep_forward64(st, sp, g, np.stack([m[k][0] for m in muts]), muts[0][k][1])
            d = np.abs(got - right).max(1) / scale
            sep[k] = max(sep.get(k, 0.0), float(np.where(np.isnan(d), np.inf, d).max()))
    return sep


@pytest.mark.parametrize("n", T.NODES)
def test_the_pairs_tell_wrong_formulations_apart(n):
    low = {}
    for case in T.dc_cases(n):
        sep = mutant_separations(case)
        assert set(sep) == {k for k in T.MUTANTS if (case.npool == "average" or not k.startswith("degree"))
                            and (n > 128 or not k.endswith("high words lost"))}
        for k, v in sep.items():
            assert v >= MUTANT_FLOOR, "%s: \"%s\" is only %.2e from the right formulation" % (case.id, k, v)
            low[k] = min(low.get(k, np.inf), v)
    print("n=%d: smallest separation per wrong formulation: %s" % (n, {k: "%.1e" % v for k, v in low.items()}))


def test_the_further_cases_stay_within_the_conditions():
    """the 11-class cases (n = 129 and 257) and the 15 network pairs of disconnection_matrix() at one case per n, under
    the same conditions and the same pin"""
    from gnm.lesion import cut_edge_counts, pair_sets
    worst = pin = 0.0
    for case in (T.dc_case(c) for c in T.CLASS_CASES):
        assert T.state_of(case)["linears_prediction.0.weight"].shape[0] == 11
        for d, r in enumerate(T.disconnect_reference(case)):
            assert r.dis64.shape[1] == 11
            worst = max(worst, _check_conditions("%s graph %d" % (case.id, d), r))
            _check_nan_share(case, r)
    for n in T.NODES:
        case = T.dc_matrix_case(n)
        st, sp = T.state_of(case), T.spec_of(case)
        for d, (g, r) in enumerate(zip(T.graphs_of(case), T.matrix_reference(case))):
            lab = T.matrix_labels(case, d)
            assert (lab == -1).sum() >= 4 and set(lab.tolist()) == set(range(-1, T.MATRIX_NETWORKS))
            a, b, pairs = pair_sets(lab, T.MATRIX_NETWORKS)
            assert len(pairs) == 15 and np.array_equal(a, r.a) and np.array_equal(b, r.b)
            assert cut_edge_counts(g.edge_mat, a, b).min() > 0
            worst = max(worst, _check_conditions("%s matrix graph %d" % (case.id, d), r))
            fin = ~r.want_nan
            got = T.keep_forward64(st, sp, g, np.stack([T.cut_keep(A, B) for A, B in zip(a, b)]))
            assert np.isnan(got[r.want_nan]).all()
            pin = max(pin, rel_err(got[fin], r.dis64[fin], floor=float(np.abs(r.base64).max())))
    assert pin <= PIN, pin
    print("further cases: fp32 CPU forward at most %.2e from fp64; keep_forward64 at most %.2e" % (worst, pin))
