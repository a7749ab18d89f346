"""The CPU half of the long-window sliding-window tests (tests/dynfc_cases.py; the GPU half is
tests/test_gpu_dynfc_long_windows.py).  It checks the case table and the reference, never the kernel:

  * the constants the table is built on (kKt, the two kDepth) are still what csrc/timeseries.hip says;
  * the table reaches every state of gnm_dynfc_corr's fetch ring that tests/test_gpu_dynfc.py does not: by the ring's
    model (dynfc_cases.ring_plan) the short table never refills a slot of the rectangular kernel, and the long one holds
    a slot refilled twice, three outer trips and last stages of 16, 1 and 15 real rows for both kernels, and the
    rectangular kernel's first refill (the tapered kernel's comes at 33 to 48 rows: the short table's window 33);
  * numpy, the GPU test's reference, is itself well inside the GPU test's 1e-12 on these inputs: within 1e-13 of an
    np.longdouble restatement (measured: 8.4e-15 at worst, at 1200 rows of fp32 input), a tenth of that bound;
  * no series of the table has a constant column inside a window, so a NaN the GPU test sees is not the inputs'."""
import os

import numpy as np
import pytest

import dynfc_cases as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ring():
    with open(os.path.join(ROOT, "graph-neural-mapping_amd", "csrc", "timeseries.hip")) as f:
        return D.ring_constants(f.read())


def test_ring_constants_are_the_kernels(ring):
    kKt, rect, taper = ring
    assert (kKt, rect, taper) == (16, 4, 2), "the fetch ring of gnm_dynfc_corr changed: revisit dynfc_cases.LONG_WINDOWS"


def test_ring_constants_fail_clearly_when_the_source_moves():
    with pytest.raises(AssertionError, match="kKt"):
        D.ring_constants("constexpr int kDepth = kTaper ? 2 : 4;")
    with pytest.raises(AssertionError, match="kDepth"):
        D.ring_constants("constexpr int kKt = 16;   // rows\nconstexpr int kDepth = 4;")
    assert D.ring_constants("constexpr int kKt = 8;\n  constexpr int kDepth = kTaper ? 3 : 5;  // x") == (8, 5, 3)


def test_ring_plan_against_a_hand_walk():
    # (window, kDepth) -> nk, refills, most refills of one slot, outer trips, at 16 rows a stage
    for (window, depth), want in {(50, 4): (4, 0, 0, 1), (64, 4): (4, 0, 0, 1), (65, 4): (5, 1, 1, 2),
                                  (128, 4): (8, 4, 1, 2), (129, 4): (9, 5, 2, 3), (1200, 4): (75, 71, 18, 19),
                                  (2, 2): (1, 0, 0, 1), (32, 2): (2, 0, 0, 1), (33, 2): (3, 1, 1, 2),
                                  (50, 2): (4, 2, 1, 2), (65, 2): (5, 3, 2, 3), (1200, 2): (75, 73, 37, 38)}.items():
        assert D.ring_plan(window, depth == 2, 16, depth) == want, (window, depth)
        assert D.ring_plan(window, depth == 2, 16, (4, 2)) == want, (window, depth)


def test_the_short_table_never_refills_the_rectangular_ring(ring):
    """the gap: every window of tests/test_gpu_dynfc.py runs the rectangular kernel's prologue only, and refills a slot
    of the tapered kernel once at most"""
    kKt, rect, taper = ring
    for window in D.WINDOWS:
        nk, refills, most, trips = D.ring_plan(window, False, kKt, rect)
        assert refills == 0 and trips == 1, window
        assert D.ring_plan(window, True, kKt, taper)[2] <= 1, window


def test_the_long_table_reaches_the_rings_steady_state(ring):
    kKt, rect, taper = ring
    assert D.LONG_WINDOWS == [64, 65, 80, 81, 128, 129, 143, 257, 1200] and D.LONG_NS == [1, 7, 64, 65, 129]
    assert D.LONG_BIG_N == [(400, 65), (400, 129)]
    assert len(D.LONG_CASES) == 47 and len(set(D.LONG_CASES)) == 47
    for tapered, depth in ((False, rect), (True, taper)):
        plans = {w: D.ring_plan(w, tapered, kKt, depth) for w in D.LONG_WINDOWS}
        assert any(p[2] >= 2 for p in plans.values()), tapered                  # a slot refilled twice
        assert any(p[3] >= 3 for p in plans.values()), tapered                  # three outer trips
        for rem in (0, 1, kKt - 1):                                             # real rows of the last stage: 16, 1, 15
            assert any(w % kKt == rem and plans[w][1] >= 1 for w in D.LONG_WINDOWS), (tapered, rem)
    # the first refill: exactly one.  The rectangular ring's is in the long table (65 rows: five stages for four slots).
    # The tapered ring's is at three stages, 33 .. 48 rows, which no window past the rectangular ring can be: it is the
    # short table's window 33, so the two tables together hold it.
    assert any(D.ring_plan(w, False, kKt, rect)[1] == 1 for w in D.LONG_WINDOWS)
    assert not any(D.ring_plan(w, True, kKt, taper)[1] == 1 for w in D.LONG_WINDOWS)
    assert any(D.ring_plan(w, True, kKt, taper)[1] == 1 for w in D.WINDOWS)
    # the big-n cases sit on the rectangular ring's first refill and on its first slot refilled twice
    assert [D.ring_plan(w, False, kKt, rect)[1:3] for _, w in D.LONG_BIG_N] == [(1, 1), (5, 2)]
    # window means past one 128-value leaf of the pairwise sum, and past two levels of it
    assert any(128 < w <= 256 for w in D.LONG_WINDOWS) and any(w > 256 for w in D.LONG_WINDOWS)


@pytest.mark.parametrize("window", D.LONG_WINDOWS)
def test_numpy_is_within_1e13_of_longdouble_on_the_tables_inputs(window):
    assert np.finfo(np.longdouble).eps < 1e-18, "np.longdouble is no wider than float64 here: no reference to check against"
    n = 65
    worst = 0.0
    for dtype in (np.float64, np.float32):
        for stride, ts in D.long_case_series(n, window, dtype):
            assert ts[0].dtype == dtype and abs(float(ts[0].mean()) - 1e5) < 1.0        # the 1e5 offset is part of it
            for w in D.tapers(window):
                for s, k, t0 in D.host_windows(ts, window, stride):
                    xw = ts[s][t0:t0 + window].astype(np.float64)
                    got, want = D.ref_fc(xw, w), D.ref_fc_longdouble(xw, w)
                    assert not np.isnan(got).any() and got.shape == (n, n)
                    err = float(np.abs(got - want).max())
                    assert err <= 1e-13, (window, dtype, stride, w is not None, s, k, err)
                    worst = max(worst, err)
    print("window %d: worst |numpy - longdouble| %.3e" % (window, worst))


@pytest.mark.parametrize("n,window", D.LONG_CASES)
def test_no_column_is_constant_inside_a_window(n, window):
    for stride, ts in D.long_case_series(n, window, np.float32):
        assert [len(x) for x in ts] == D.ragged_lengths(window, stride)
        where = D.host_windows(ts, window, stride)
        assert [sum(1 for v in where if v[0] == s) for s in range(3)] == [3, 1, 2]
        for s, k, t0 in where:
            xw = ts[s][t0:t0 + window]
            assert np.isfinite(xw).all() and (xw.max(0) > xw.min(0)).all(), (n, window, stride, s, k)
    # the float64 series round to these: a column that varies after rounding varied before it
    a, b = D.long_case_series(n, window, np.float64)[0][1], D.long_case_series(n, window, np.float32)[0][1]
    assert all(np.array_equal(x.astype(np.float32), y) for x, y in zip(a, b))
