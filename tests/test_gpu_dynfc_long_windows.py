"""The sliding-window path (csrc/timeseries.hip gnm_dynfc_means, gnm_dynfc_corr; gnm/connectome.py) past the shapes
tests/test_gpu_dynfc.py stops at: windows of 64 to 1200 rows, where gnm_dynfc_corr's fetch ring is refilled inside the K
loop (the rectangular kernel's never is at 50 rows and below), the outer loop takes up to 19 (38 under a taper) trips,
the window means enter numpy's pairwise recursion, and the driver splits a call above gnm_dynfc_max_windows(n).  The
table, the ring's model and the checks of the reference are in tests/dynfc_cases.py and
tests/test_dynfc_long_windows_host.py.

Bounds: the project's 1e-12 against numpy with numpy's NaN pattern and |R| <= 1; 2e-12 between
the sliding and the static route, each within 1e-12 of numpy; everything else is bitwise.  numpy itself is within
8.4e-15 of an np.longdouble restatement on these inputs (the host file).  Worst |R - numpy| measured over the table:
in DESIGN.md 3.17."""
import time

import numpy as np
import pytest
import torch

import dynfc_cases as D
from dynfc_cases import bits_eq, check_against_numpy, host_windows, nan_windows, same_graphs, series, tapers

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


# ------------------------------------------------------------------------------------------------ a. against numpy
@pytest.mark.parametrize("taper", range(3), ids=D.TAPER_NAMES)
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("n,window", D.LONG_CASES)
def test_every_long_window_matches_numpy(n, window, dtype, taper):
    from gnm.connectome import dynamic_connectivity_from_timeseries
    w = tapers(window)[taper]
    worst = 0.0
    for stride, ts in D.long_case_series(n, window, dtype):
        where = host_windows(ts, window, stride)
        assert [sum(1 for v in where if v[0] == s) for s in range(3)] == [3, 1, 2]
        got = dynamic_connectivity_from_timeseries(ts, window, stride, taper=w)
        assert isinstance(got, list) and [int(g.shape[0]) for g in got] == [3, 1, 2]
        got = [g.cpu().numpy() for g in got]
        for s, k, t0 in where:
            err = check_against_numpy(got[s][k], ts[s][t0:t0 + window].astype(np.float64), w,
                                      (n, window, stride, D.TAPER_NAMES[taper], s, k))
            worst = max(worst, err)
    print("n %d window %d %s %s: worst |R - numpy| %.3e" % (n, window, np.dtype(dtype).name, D.TAPER_NAMES[taper], worst))


# ------------------------------------------------------------------------------------------------ b. the static route
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("T,n", [(1200, 129), (257, 65)])
def test_whole_series_window_is_the_static_route_within_its_bound(T, n, dtype):
    """one window of all T rows against connectivity_from_timeseries of the same rows: each is within 1e-12 of numpy"""
    from gnm.connectome import connectivity_from_timeseries, dynamic_connectivity_from_timeseries
    rng = np.random.default_rng(100 * T + n)
    ts = [series(rng, T, n, offset=1e4 * s).astype(dtype) for s in range(2)]
    got = dynamic_connectivity_from_timeseries(ts, T, 1)
    assert [tuple(g.shape) for g in got] == [(1, n, n)] * 2
    static = connectivity_from_timeseries(ts).cpu().numpy()
    for s in range(2):
        g = got[s][0].cpu().numpy()
        diff = np.abs(g - static[s]).max()
        print("T %d n %d %s series %d: |sliding - static| %.3e" % (T, n, np.dtype(dtype).name, s, diff))
        assert diff <= 2e-12, (T, n, s, diff)
        check_against_numpy(g, ts[s].astype(np.float64), None, (T, n, s))


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("window", [129, 257, 1200])
def test_long_window_means_are_bitwise_the_static_means(window, dtype):
    """129, 257 and 1200 rows: one, two and four levels of numpy's pairwise recursion, entered from a window descriptor"""
    from gnm import connectome as C
    rng = np.random.default_rng(window)
    n, stride = 70, 37
    ts = [series(rng, T, n, offset=1e4 * (s + 1), scale=50.0).astype(dtype)
          for s, T in enumerate((window + 80, window, window + 40))]
    where = host_windows(ts, window, stride)
    assert len(where) == 3 + 1 + 2
    slices = [ts[s][t0:t0 + window] for s, _, t0 in where]
    x, t_off, _, _ = C._as_timeseries(ts, torch.device(DEV))
    w_beg, _, _ = C._plan_windows(t_off.cpu().numpy(), window, stride)
    mean = C._dyn_means(x, torch.from_numpy(w_beg).to(DEV), window, n)
    sx, st, sS, _ = C._as_timeseries(slices, torch.device(DEV))
    assert bits_eq(mean.cpu().numpy(), C._ts_means(sx, st, sS, n).cpu().numpy())
    # both sides above are one kernel: numpy's means of the same rows, to the static test's 1e-13 relative
    want = np.stack([np.asfortranarray(a.astype(np.float64)).mean(0) for a in slices])
    assert np.abs(mean.cpu().numpy() - want).max() / np.abs(want).max() <= 1e-13
    assert bits_eq(C._ts_zscores(mean, len(where), n, torch.float64).cpu().numpy(),
                   C.mean_bold_features(slices, dtype=torch.float64).cpu().numpy())


# ------------------------------------------------------------------------------------------------ c. independence
@pytest.mark.parametrize("window", [81, 129])
def test_a_long_windows_fc_is_bitwise_independent_of_the_call(window):
    from gnm.connectome import dynamic_connectivity_from_timeseries as dfc
    rng = np.random.default_rng(7 + window)
    n = 70
    stack = np.stack([series(rng, window + 41, n, offset=3e3 * s) for s in range(3)])
    ragged = [series(rng, window + 13, n), stack[1], series(rng, window + 5, n, offset=10.0)]
    for w in tapers(window):
        alone = dfc(stack[1:2], window, 1, taper=w).cpu().numpy()[0]                      # [42, n, n]
        assert alone.shape == (42, n, n)
        assert bits_eq(alone, dfc(stack, window, 1, taper=w).cpu().numpy()[1])
        assert bits_eq(alone, dfc(ragged, window, 1, taper=w)[1].cpu().numpy())
        on_dev = [torch.from_numpy(a).to(DEV) for a in ragged]
        assert bits_eq(alone, dfc(on_dev, window, 1, taper=w)[1].cpu().numpy())
        assert bits_eq(alone, dfc(torch.from_numpy(stack).to(DEV), window, 1, taper=w).cpu().numpy()[1])
        fifth = dfc(ragged, window, 5, taper=w)[1].cpu().numpy()                            # starts 0, 5, .., 40
        assert fifth.shape[0] == 9 and bits_eq(fifth, alone[::5])
        one = dfc([stack[1][15:15 + window]], window, 1, taper=w)[0].cpu().numpy()          # the window's rows alone
        assert bits_eq(one[0], alone[15])
        f32 = stack.astype(np.float32)
        wide = f32.astype(np.float64)
        assert bits_eq(dfc(f32, window, 6, taper=w).cpu().numpy(), dfc(wide, window, 6, taper=w).cpu().numpy())
        assert bits_eq(dfc(torch.from_numpy(f32).to(DEV), window, 6, taper=w).cpu().numpy(),
                       dfc(wide, window, 6, taper=w).cpu().numpy())


# ------------------------------------------------------------------------------------------------ d. descriptor order
@pytest.mark.parametrize("tapered", [False, True])
def test_descriptors_in_any_order_and_repeated(tapered):
    """w_beg permuted and with entries repeated gives bitwise the same permutation of the ascending-order result"""
    from gnm import connectome as C
    rng = np.random.default_rng(21)
    n, window = 65, 81
    ts = [series(rng, T, n, offset=1e3 * s) for s, T in enumerate((window + 9, window, window + 4))]
    x, t_off, _, _ = C._as_timeseries(ts, torch.device(DEV))
    asc, _, _ = C._plan_windows(t_off.cpu().numpy(), window, 1)
    W = len(asc)
    assert W == 10 + 1 + 5 and (np.diff(asc) > 0).all()
    order = np.concatenate([rng.permutation(W), rng.permutation(W)[:5], [W - 1, W - 1, 0]])
    assert sorted(set(order.tolist())) == list(range(W)) and not (np.diff(order) > 0).all()
    wd = torch.from_numpy(np.hamming(window + 2)[1:-1]).to(DEV) if tapered else None

    def run(w_beg):
        w_beg = torch.from_numpy(np.ascontiguousarray(w_beg)).to(DEV)
        mean = C._dyn_means(x, w_beg, window, n)
        out = torch.full((int(w_beg.shape[0]), n, n), 7.0, dtype=torch.float64, device=DEV)
        C._dyn_corr(x, w_beg, window, None if tapered else mean, wd, n, out)
        return mean.cpu().numpy(), out.cpu().numpy()

    mean_a, fc_a = run(asc)
    mean_p, fc_p = run(asc[order])
    assert bits_eq(mean_p, mean_a[order]) and bits_eq(fc_p, fc_a[order])
    where = host_windows(ts, window, 1)
    for k in (0, 9, 10, 15):                                            # and the ascending result is numpy's
        s, _, t0 = where[k]
        check_against_numpy(fc_a[k], ts[s][t0:t0 + window], None if wd is None else wd.cpu().numpy(), k)


# ------------------------------------------------------------------------------------------------ e. NaN, inf, constants
def test_nan_and_inf_reach_exactly_the_long_windows_that_cover_their_row():
    """window 81: the last stage holds 1 real row and 15 padded ones.  Stride 1, so the window that ends on the row
    before a bad row and the one that starts on the row after it are both there, and both are clean."""
    from gnm.connectome import dynamic_connectivity_from_timeseries, window_starts
    rng = np.random.default_rng(4)
    n, window, T = 9, 81, 260
    x = series(rng, T, n)
    x[85, 2] = np.nan                                   # windows 5 .. 85
    x[170, 6] = np.inf                                  # windows 90 .. 170
    starts = window_starts(T, window, 1)
    assert starts.tolist() == list(range(180))
    cover_nan, cover_inf = list(range(5, 86)), list(range(90, 171))
    for w in tapers(window):
        got = dynamic_connectivity_from_timeseries([x], window, 1, taper=w)[0].cpu().numpy()
        assert nan_windows(got) == cover_nan + cover_inf
        for k in (4, 86, 89, 171):                      # ends on the row before, starts on the row after
            assert np.isfinite(got[k]).all()
        for k, t0 in enumerate(starts):
            check_against_numpy(got[k], x[t0:t0 + window], w, (k, w is not None))
        for cover, col in ((cover_nan, 2), (cover_inf, 6)):
            want = np.zeros((n, n), bool)
            want[col, :] = want[:, col] = True
            assert all(np.array_equal(np.isnan(got[k]), want) for k in cover)


@pytest.mark.parametrize("window", [81, 129])
def test_constant_roi_inside_exactly_one_long_rectangular_window(window):
    from gnm.connectome import dynamic_connectivity_from_timeseries
    rng = np.random.default_rng(3 + window)
    n = 9
    x = series(rng, window + 20, n)
    x[10:10 + window, 4] = 7.0                          # window 10 of the stride-1 tiling, and no other
    got = dynamic_connectivity_from_timeseries([x], window, 1)[0].cpu().numpy()
    assert got.shape[0] == 21 and nan_windows(got) == [10]
    want = np.zeros((n, n), bool)
    want[4, :] = want[:, 4] = True
    assert np.array_equal(np.isnan(got[10]), want)
    for k in range(21):
        check_against_numpy(got[k], x[k:k + window], None, k)


# ------------------------------------------------------------------------------------------------ f. the split, by proxy
class SmallLaunchLimit:
    """gnm._cabi.lib with gnm_dynfc_max_windows answering `limit`: every other attribute is the real library's"""

    def __init__(self, real, limit):
        self._real, self._limit, self.asked, self.launches = real, limit, 0, []

    def __getattr__(self, name):
        return getattr(self._real, name)

    def gnm_dynfc_max_windows(self, n):
        self.asked += 1
        return self._limit

    def gnm_dynfc_corr(self, x, f64, w_beg, window, mean, taper, W, n, fc, stream):
        self.launches.append(int(W))
        return self._real.gnm_dynfc_corr(x, f64, w_beg, window, mean, taper, W, n, fc, stream)


@pytest.mark.parametrize("tapered", [False, True])
def test_launch_split_by_proxy(tapered, monkeypatch):
    from gnm import connectome as C
    from gnm.arena import GraphArena
    rng = np.random.default_rng(31)
    n, window, sp = 65, 81, 30
    ts = [series(rng, window + 6, n, offset=1e3), series(rng, window + 3, n)]          # 7 + 4 = 11 windows
    labels = [1, 0]
    w = np.hamming(window + 2)[1:-1] if tapered else None
    whole = torch.cat(C.dynamic_connectivity_from_timeseries(ts, window, 1, taper=w)).cpu().numpy()
    assert whole.shape == (11, n, n)
    ref, windows = C.dynamic_graphs_from_timeseries(GraphArena(DEV), ts, sp, labels, window, 1, taper=w)
    assert len(ref) == 11 and any(g.edge_mat.shape[1] > 0 for g in ref)

    proxy = SmallLaunchLimit(C.lib, 3)
    monkeypatch.setattr(C, "lib", proxy)
    got = torch.cat(C.dynamic_connectivity_from_timeseries(ts, window, 1, taper=w)).cpu().numpy()
    assert proxy.asked == 1 and proxy.launches == [3, 3, 3, 2]
    assert bits_eq(got, whole)
    # chunks of 4 windows crossed with launches of 3: (3, 1), (3, 1), 3
    monkeypatch.setattr(C, "DYNFC_WORK_BYTES", 4 * 8 * n * n)
    assert C._plan_chunks(11, n, C.DYNFC_WORK_BYTES) == [(0, 4), (4, 8), (8, 11)]
    proxy.launches.clear()
    graphs, w2 = C.dynamic_graphs_from_timeseries(GraphArena(DEV), ts, sp, labels, window, 1, taper=w)
    assert proxy.asked == 4 and proxy.launches == [3, 1, 3, 1, 3]
    assert np.array_equal(w2, windows)
    same_graphs(graphs, ref)


# ------------------------------------------------------------------------------------------------ g. the split, for real
def test_launch_split_for_real():
    """n = 1, window 2, stride 1: gnm_dynfc_max_windows(1) + 5 windows of two rows each, the only shape at which the real
    limit is reachable (34 MB of fp32 input, 67 MB of output).  np.corrcoef of one ROI is c / c: 1.0, or NaN where the
    window's variance is zero or a row is not finite."""
    from gnm import connectome as C
    t_start = time.perf_counter()
    limit = int(C.lib.gnm_dynfc_max_windows(1))
    T = limit + 6
    rng = np.random.default_rng(41)
    x = rng.standard_normal((T, 1), dtype=np.float32)
    for r in (5, limit - 1, limit, limit + 3):
        x[r, 0] = np.nan
    x[limit + 5, 0] = x[limit + 4, 0]                   # one equal pair beyond the limit: the last window
    v = x[:, 0]
    bad = ~np.isfinite(v)
    want = np.where(bad[:-1] | bad[1:] | (v[:-1] == v[1:]), np.nan, 1.0)
    assert want.shape == (limit + 5,) and want.dtype == np.float64
    # windows limit - 2 .. limit + 4, the second launch from `limit` on: only (limit + 1, limit + 2) is a clean pair
    assert np.isnan(want[limit - 2:]).tolist() == [True, True, True, False, True, True, True]
    assert np.isnan(want[:8]).tolist() == [False] * 4 + [True, True, False, False]
    xd = torch.from_numpy(x).to(DEV).unsqueeze(0)
    for taper in (None, [1.0, 2.0]):
        got = C.dynamic_connectivity_from_timeseries(xd, 2, 1, taper=taper)
        assert tuple(got.shape) == (1, limit + 5, 1, 1) and got.dtype == torch.float64
        got = got.reshape(-1).cpu().numpy()
        assert np.array_equal(got, want, equal_nan=True), np.flatnonzero(~((got == want) | (np.isnan(got) & np.isnan(want))))[:10]
        del got
    print("launch split for real: %d windows, %.2f s" % (limit + 5, time.perf_counter() - t_start))


# ------------------------------------------------------------------------------------------------ h. a time course
def test_class_score_time_course_at_a_long_window():
    from gnm import connectome as C
    from gnm.arena import GraphArena
    from models.graphcnn import GIN_InfoMaxReg
    rng = np.random.default_rng(13)
    n, S, window, stride = 64, 2, 81, 40
    ts = np.stack([series(rng, 170, n, offset=1e4, scale=80.0) for _ in range(S)])      # starts 0, 40, 80: 3 windows
    torch.manual_seed(0)
    model = GIN_InfoMaxReg(3, 2, 1, 32, 2, 0.0, True, "sum", "sum", torch.device(DEV)).to(DEV)
    model.eval()
    graphs, windows = C.dynamic_graphs_from_timeseries(model, ts, 30, [0, 1], window, stride)
    W = len(graphs) // S
    assert W == 3 and windows[:, 1].tolist() == list(range(3)) * 2 and windows[:, 2].tolist() == [0, 40, 80] * 2
    fc = C.dynamic_connectivity_from_timeseries(ts, window, stride)
    feats = C.mean_bold_features([ts[s][t0:t0 + window] for s, _, t0 in windows.tolist()])
    ref = C.graphs_from_connectivity(GraphArena(DEV), fc.reshape(S * W, n, n), 30, feats,
                                     [g.label for g in graphs])
    same_graphs(graphs, ref)
    scores = model.predict(graphs)
    assert bits_eq(scores.cpu().numpy(), model.predict(ref).cpu().numpy())
    course = scores.reshape(S, W, -1)
    assert tuple(course.shape) == (S, W, 2) and torch.isfinite(course).all()
