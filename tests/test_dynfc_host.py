"""CPU checks of the sliding-window path (gnm/connectome.py window_starts, dynamic_connectivity_from_timeseries,
dynamic_graphs_from_timeseries; csrc/timeseries.hip gnm_dynfc_*): the window enumeration, every argument check before
anything touches a device, the C-ABI declared, bound and exported, and the chunk planner."""
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["gnm_dynfc_max_windows", "gnm_dynfc_means", "gnm_dynfc_corr"]


def test_window_starts_against_a_hand_enumeration():
    from gnm.connectome import window_starts
    cases = [((10, 4, 1), [0, 1, 2, 3, 4, 5, 6]),
             ((10, 4, 3), [0, 3, 6]),
             ((11, 4, 3), [0, 3, 6]),             # the trailing row fills no window
             ((12, 4, 3), [0, 3, 6]),
             ((13, 4, 3), [0, 3, 6, 9]),
             ((7, 7, 1), [0]),                    # T == window
             ((7, 7, 5), [0]),
             ((11, 7, 5), [0]),                   # T == window + stride - 1
             ((12, 7, 5), [0, 5]),
             ((20, 3, 8), [0, 8, 16]),            # stride > window: rows between windows are skipped
             ((18, 3, 8), [0, 8]),
             ((2, 2, 1), [0]),
             ((1200, 50, 10), list(range(0, 1151, 10)))]
    for (T, window, stride), want in cases:
        got = window_starts(T, window, stride)
        assert got.dtype == np.int64 and got.tolist() == want, (T, window, stride)
        assert np.array_equal(got, np.arange(0, T - window + 1, stride))
    assert len(window_starts(1200, 50, 10)) == 116
    assert window_starts(np.int64(10), np.int32(4), np.int64(3)).tolist() == [0, 3, 6]


def test_window_starts_rejects_bad_arguments():
    from gnm.connectome import window_starts
    for T, window, stride in ((10, 4.0, 1), (10, "4", 1), (10, True, 1), (10, 1, 1), (10, 0, 1), (10, -3, 1),
                              (10, 4, 0), (10, 4, -1), (10, 4, 1.5), (3, 4, 1), (0, 2, 1)):
        with pytest.raises(ValueError):
            window_starts(T, window, stride)


def test_value_errors_come_before_any_device():
    """every call below names the CPU as its device, where the time-series path raises GnmError: a ValueError shows the
    argument was checked first"""
    from gnm.arena import GraphArena
    from gnm.connectome import dynamic_connectivity_from_timeseries as dfc
    from gnm.connectome import dynamic_graphs_from_timeseries as dgr
    from gnm._cabi import GnmError
    rng = np.random.default_rng(0)
    ok = rng.standard_normal((2, 12, 5))
    ragged = [rng.standard_normal((12, 5)), rng.standard_normal((5, 5)), rng.standard_normal((9, 5))]
    good = np.hamming(8)[1:-1]
    bad_tapers = [np.ones(5), np.ones((6, 1)), np.ones((1, 6)), [1, 1, 1, 1, 1, np.nan], [1, 1, 1, 1, 1, np.inf],
                  [1, 1, 1, -1e-3, 1, 1], [0, 0, 0, 3, 0, 0], np.zeros(6), np.ones(6, dtype=complex)]
    for kw in (dict(window=6.0), dict(window=1), dict(window=6, stride=0), dict(window=6, stride=2.0),
               dict(window=13), dict(window=None)):
        with pytest.raises(ValueError):
            dfc(ok, device="cpu", **kw)
        with pytest.raises(ValueError):
            dgr(GraphArena("cpu"), ok, 30, [0, 1], **kw)
    for t in bad_tapers:
        with pytest.raises(ValueError):
            dfc(ok, 6, taper=t, device="cpu")
        with pytest.raises(ValueError):
            dgr(GraphArena("cpu"), ok, 30, [0, 1], 6, taper=t)
    with pytest.raises(ValueError, match=r"ts\[1\]"):                    # the short subject is named
        dfc(ragged, 6, device="cpu")
    with pytest.raises(ValueError, match=r"ts\[1\]"):
        dgr(GraphArena("cpu"), ragged, 30, [0, 1, 0], 6)
    with pytest.raises(ValueError):
        dfc(ok[0], 6, device="cpu")                                      # [T, n] is not a stack
    with pytest.raises(ValueError):
        dfc(ok.astype(np.float16), 6, device="cpu")
    with pytest.raises(ValueError):
        dgr(GraphArena("cpu"), ok, 30, [0, 1, 0], 6)                     # labels
    with pytest.raises(ValueError):
        dgr(GraphArena("cpu"), ok, 101, [0, 1], 6)                       # sparsity
    with pytest.raises(ValueError):
        dgr(GraphArena("cpu"), ok, 30, [0, 1], 6, node_features="one_hot")
    with pytest.raises(ValueError):
        dgr(GraphArena("cpu"), ok, 30, [0, 1], 6, node_features=np.ones((3, 5, 2), np.float32))   # 3 subjects for 2
    # with every argument right, the CPU is refused as a device, not computed on
    with pytest.raises(GnmError):
        dfc(ok, 6, taper=good, device="cpu")
    with pytest.raises(GnmError):
        dgr(GraphArena("cpu"), ok, 30, [0, 1], 6, stride=2)


def test_symbols_declared_bound_and_exported():
    from gnm import _cabi
    header = open(os.path.join(ROOT, "include", "gnm_hip.h")).read()
    for name in SYMBOLS:
        assert re.search(r"\b%s\(" % name, header), name
        assert name in _cabi.SIGNATURES, name
        assert getattr(_cabi.lib, name) is not None


def test_launch_limit_is_the_grams():
    from gnm._cabi import lib
    nmax = lib.gnm_timeseries_max_nodes()
    for n in (1, 64, 65, 400, nmax):
        nb = (n + 63) // 64
        assert lib.gnm_dynfc_max_windows(n) == (0x7fffffff // 256) // (nb * (nb + 1) // 2)
    assert lib.gnm_dynfc_max_windows(0) == 0 and lib.gnm_dynfc_max_windows(nmax + 1) == 0


def test_c_entries_check_arguments_before_launching():
    from gnm._cabi import lib
    nmax = lib.gnm_timeseries_max_nodes()
    fake = 1 << 20                                   # never dereferenced: every call below returns before a launch
    means, corr = lib.gnm_dynfc_means, lib.gnm_dynfc_corr
    assert means(fake, 1, fake, 8, 1, 0, fake, None) == -1
    assert means(fake, 1, fake, 8, -1, 4, fake, None) == -1
    assert means(fake, 1, fake, 1, 1, 4, fake, None) == -1
    assert means(fake, 1, fake, 0, 1, 4, fake, None) == -1
    assert means(fake, 1, fake, 1, 0, 4, fake, None) == -1             # a bad window even with nothing to do
    assert means(fake, 1, fake, 8, 1, nmax + 1, fake, None) == -2
    assert means(None, 1, fake, 8, 1, 4, fake, None) == -1
    assert means(fake, 0, None, 8, 1, 4, fake, None) == -1
    assert means(fake, 1, fake, 8, 1, 4, None, None) == -1
    assert means(None, 1, None, 8, 0, 4, None, None) == 0              # nothing to do
    assert corr(fake, 1, fake, 8, fake, None, 1, 0, fake, None) == -1
    assert corr(fake, 1, fake, 8, fake, None, -1, 4, fake, None) == -1
    assert corr(fake, 1, fake, 1, fake, None, 1, 4, fake, None) == -1
    assert corr(fake, 1, fake, -5, fake, fake, 1, 4, fake, None) == -1
    assert corr(fake, 1, fake, 8, fake, None, 1, nmax + 1, fake, None) == -2
    assert corr(None, 1, fake, 8, fake, None, 1, 4, fake, None) == -1
    assert corr(fake, 0, None, 8, fake, fake, 1, 4, fake, None) == -1
    assert corr(fake, 1, fake, 8, fake, fake, 1, 4, None, None) == -1
    assert corr(fake, 1, fake, 8, None, None, 1, 4, fake, None) == -1  # neither means nor a taper
    assert corr(None, 1, None, 8, None, None, 0, 4, None, None) == 0
    # one window past the launch limit: refused, the driver splits there
    for n in (4, 400, nmax):
        assert corr(fake, 1, fake, 8, fake, None, lib.gnm_dynfc_max_windows(n) + 1, n, fake, None) == -2


def test_chunk_planner_stays_within_budget_and_covers_every_window_once():
    from gnm import connectome as C
    assert C.DYNFC_WORK_BYTES == 1 << 30
    for total in (1, 2, 7, 116, 1000):
        for n in (1, 7, 400):
            per = 8 * n * n
            for budget in (1, per - 1, per, per + 1, 2 * per, 3 * per, 3 * per + 5, 10 ** 4 * per, 1 << 30):
                chunks = C._plan_chunks(total, n, budget)
                flat = [k for lo, hi in chunks for k in range(lo, hi)]
                assert flat == list(range(total)), (total, n, budget)
                assert all(hi > lo for lo, hi in chunks)
                for lo, hi in chunks:
                    # a single matrix larger than the budget still goes through, alone
                    assert (hi - lo) * per <= budget or hi - lo == 1, (total, n, budget)
                assert len(chunks) == -(-total // max(1, budget // per))       # and no smaller than it has to be
    assert C._plan_chunks(116 * 64, 400, 1 << 30)[0] == (0, 838)


def test_window_plan_is_subject_major():
    from gnm.connectome import _plan_windows, window_starts
    t_off = np.array([0, 12, 19, 40], dtype=np.int64)
    w_beg, windows, counts = _plan_windows(t_off, 5, 3)
    want = [(s, k, int(t0)) for s in range(3) for k, t0 in enumerate(window_starts(int(t_off[s + 1] - t_off[s]), 5, 3))]
    assert windows.dtype == np.int64 and windows.tolist() == [list(r) for r in want]
    assert w_beg.dtype == np.int64 and w_beg.tolist() == [int(t_off[s]) + t0 for s, _, t0 in want]
    assert counts.tolist() == [3, 1, 6]
    assert (w_beg + 5 <= t_off[windows[:, 0] + 1]).all()               # every window ends inside its subject


def test_taper_argument():
    from gnm.connectome import _taper_arg
    assert _taper_arg(None, 6) is None
    w = _taper_arg(torch.tensor([0, 1, 2, 2, 1, 0]), 6)                 # zeros are fine beside two positive weights
    assert w.dtype == np.float64 and w.tolist() == [0, 1, 2, 2, 1, 0]
    h = np.hamming(8)[1:-1].astype(np.float32)
    assert np.array_equal(_taper_arg(h, 6), h.astype(np.float64))


def test_numpy_weighted_constant_is_not_nan():
    """why the GPU tests keep constant ROIs out of tapered windows: numpy's weighted mean of a constant is not exact,
    so np.cov(aweights=) gives a tiny non-zero variance and no NaN where np.corrcoef gives a NaN row and column"""
    rng = np.random.default_rng(0)
    x = rng.standard_normal((50, 4))
    x[:, 2] = 7.0
    w = np.hamming(52)[1:-1]
    with np.errstate(all="ignore"):
        c = np.cov(x, rowvar=False, aweights=w)
        assert np.isnan(np.corrcoef(x, rowvar=False)[2]).all()
    assert c[2, 2] != 0.0 and c[2, 2] < 1e-28
