"""Connectivity states on the device (gnm/states.py, csrc/dynstates.hip) against the numpy oracle of
tests/dynstates_cases.py, which runs on the FC the device itself computed and read back.

Labels, n_iter, converged, counts and centroids are compared exactly (centroids bitwise: sequential sums in ascending
window order and one division); the label comparison rests on the oracle margin being above 1e-9 in every case, asserted
here on the device's FC and in tests/test_dynstates_host.py on numpy's.  Distances: |dist - oracle| <= 1e-11 max(oracle,
1), a priori (P + 3) 2^-53 for a sum of P non-negative terms in any order.  Everything about one result in two calls
(stack, chunk size, route, launch shape, host or device input, fp32 widening) is bitwise.  The worst measured distance
error is printed per case; DESIGN.md 3.19 records it."""
import functools

import numpy as np
import pytest
import torch

import dynstates_cases as D
from dynstates_cases import WINDOW, STRIDE, bits_eq, check_distances, init_windows

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@functools.lru_cache(maxsize=None)
def device_fc(n, taper=False):
    """(fc [W, n, n] on the device, the same array on the host) of the case's series"""
    from gnm.connectome import dynamic_connectivity_from_timeseries
    w = np.hamming(WINDOW + 2)[1:-1] if taper else None
    fc = dynamic_connectivity_from_timeseries(D.case_series(n), WINDOW, STRIDE, taper=w)
    fc = fc.reshape(-1, n, n)
    h = fc.cpu().numpy()
    h.setflags(write=False)
    return fc, h


@functools.lru_cache(maxsize=None)
def oracle(n, k, max_iter=100):
    h = device_fc(n)[1]
    return D.oracle_run(h, h[init_windows(k)], max_iter)


def traced(fn, *args, **kw):
    """(result, records of gnm.states.TRACE during the call)"""
    from gnm import states
    states.TRACE = []
    try:
        out = fn(*args, **kw)
        return out, states.TRACE
    finally:
        states.TRACE = None


def sequential_sum(values):
    s = 0.0
    for v in values:
        s = s + float(v)
    return s


def same_result(a, b):
    assert bits_eq(a.centroids.cpu().numpy(), b.centroids.cpu().numpy())
    assert bits_eq(a.labels.cpu().numpy(), b.labels.cpu().numpy())
    assert bits_eq(a.distances.cpu().numpy(), b.distances.cpu().numpy())
    assert bits_eq(a.counts.cpu().numpy(), b.counts.cpu().numpy())
    assert a.inertia == b.inertia and a.n_iter == b.n_iter and a.converged == b.converged


def against_oracle(st, trace, want, what):
    """everything a run returns against an oracle run on the same FC; the worst distance ratio"""
    history = [r[2] for r in trace if r[0] == "labels"]
    assert len(history) == len(want["history"]), what
    for it, (a, b) in enumerate(zip(history, want["history"])):
        assert a.dtype == np.int32 and np.array_equal(a, b), (what, it, np.flatnonzero(a != b)[:8])
    assert st.n_iter == want["n_iter"] and st.converged == want["converged"], what
    labels = st.labels.cpu().numpy()
    assert labels.dtype == np.int32 and np.array_equal(labels, want["labels"]), what
    cen = st.centroids.cpu().numpy()
    assert bits_eq(cen, want["centroids"]), (what, np.abs(cen - want["centroids"]).max())
    assert np.array_equal(cen, cen.transpose(0, 2, 1))
    assert st.counts.dtype == torch.int64 and np.array_equal(st.counts.cpu().numpy(), want["counts"]), what
    dist = st.distances.cpu().numpy()
    worst = check_distances(dist, want["dist"], what)
    ok = labels >= 0
    assert st.inertia == sequential_sum(dist[ok, labels[ok]]), what           # ascending window order, on the device
    assert abs(st.inertia - want["inertia"]) <= D.DIST_RTOL * max(want["inertia"], 1.0), what
    return worst


# ------------------------------------------------------------------------------------------------ a. labels, centroids
@pytest.mark.parametrize("n,k", D.CASES + [D.BIG])
def test_label_sequence_centroids_and_distances_match_the_oracle(n, k):
    from gnm.connectome import ConnectivityStates, connectivity_states
    fc, h = device_fc(n)
    assert h.shape == ((40 if (n, k) == D.BIG else 171), n, n) and np.isfinite(h).all()
    want = oracle(n, k)
    assert want["converged"] and want["margin"] > D.MARGIN, (n, k, want["margin"])
    st, trace = traced(connectivity_states, fc, k, init=init_windows(k))
    assert isinstance(st, ConnectivityStates) and st.windows is None
    assert st.centroids.is_cuda and st.centroids.dtype == torch.float64 and tuple(st.centroids.shape) == (k, n, n)
    assert tuple(st.distances.shape) == (h.shape[0], k) and tuple(st.labels.shape) == (h.shape[0],)
    worst = against_oracle(st, trace, want, (n, k))
    print("n %d k %d: %d iterations, margin %.2e, worst |dist - oracle| / max(oracle, 1) %.3e"
          % (n, k, st.n_iter, want["margin"], worst))
    if n == 1:                                                  # no feature: exact zeros, state 0, the mean diagonal
        assert not st.distances.cpu().numpy().any() and not st.labels.cpu().numpy().any()
        assert st.centroids.cpu().numpy()[0, 0, 0] == sequential_sum(h[:, 0, 0]) / h.shape[0] and st.inertia == 0.0
    elif k > 1:
        assert st.n_iter >= 2 and len(set(st.labels.cpu().numpy().tolist())) > 1


# ------------------------------------------------------------------------------------------------ b. independence
def test_a_windows_distances_are_bitwise_independent_of_the_call():
    from gnm.connectome import assign_states
    n, k = 65, 5
    fc, h = device_fc(n)
    cen = h[init_windows(k)] * 0.5 + 0.25 * h[init_windows(k) + 3]              # not windows themselves
    labels, dist = (t.cpu().numpy() for t in assign_states(fc, cen))
    want_l, want_d = D.oracle_assign(h, cen)
    assert np.array_equal(labels, want_l)
    check_distances(dist, want_d, "stack")
    for w in (0, 1, 2, 3, 85, 170):                                             # alone: every slot of a pass of four
        l1, d1 = assign_states(fc[w:w + 1], cen)
        assert bits_eq(d1.cpu().numpy()[0], dist[w]) and int(l1[0]) == labels[w]
    rng = np.random.default_rng(3)
    order = np.concatenate([rng.permutation(171), [170, 170, 0], rng.permutation(171)[:40]])
    lp, dp = assign_states(fc[torch.from_numpy(order).to(DEV)], cen)
    assert bits_eq(dp.cpu().numpy(), dist[order]) and bits_eq(lp.cpu().numpy(), labels[order])
    lh, dh = assign_states(h, torch.from_numpy(cen))                            # host input, torch centroids
    assert lh.is_cuda and bits_eq(dh.cpu().numpy(), dist) and bits_eq(lh.cpu().numpy(), labels)
    f32 = h.astype(np.float32)
    c32 = cen.astype(np.float32)
    a = assign_states(f32, c32)
    b = assign_states(torch.from_numpy(f32.astype(np.float64)).to(DEV), c32.astype(np.float64))
    assert bits_eq(a[1].cpu().numpy(), b[1].cpu().numpy()) and bits_eq(a[0].cpu().numpy(), b[0].cpu().numpy())
    check_distances(a[1].cpu().numpy(), D.oracle_assign(f32.astype(np.float64), c32.astype(np.float64))[1], "f32")


@pytest.mark.parametrize("n", [2, 64, 65, 129])
def test_diagonal_and_lower_triangle_never_enter_a_distance(n):
    """the features are i < j: another diagonal and a NaN lower triangle, in the windows and in the centroids, leave
    every distance bitwise as it is (a correlation matrix's own diagonal is 1.0 everywhere and would hide a slip)"""
    from gnm.connectome import assign_states
    k = 5
    fc, h = device_fc(n)
    cen = np.array(h[init_windows(k) + 2])
    labels, dist = (t.cpu().numpy() for t in assign_states(fc, cen))
    check_distances(dist, D.oracle_assign(h, cen)[1], n)
    low = np.tril(np.ones((n, n), bool), -1)
    h2, cen2 = np.array(h), cen.copy()
    h2[:, low] = np.nan
    cen2[:, low] = np.nan
    np.einsum("wii->wi", h2)[:] = 3.0 + np.arange(n)
    np.einsum("cii->ci", cen2)[:] = -7.0
    l2, d2 = (t.cpu().numpy() for t in assign_states(h2, cen2))
    assert bits_eq(d2, dist) and bits_eq(l2, labels)


class FewGroups:
    """gnm._cabi.lib with gnm_states_assign launched with `groups` workgroups per block pair, each striding over the
    windows: the stand-in for a launch that has more windows than its grid; every other attribute is the real library's"""

    def __init__(self, real, groups):
        self._real, self._groups, self.calls = real, groups, 0

    def __getattr__(self, name):
        return getattr(self._real, name)

    def gnm_states_assign(self, fc, cen, W, n, k, groups, work, dist, label, stream):
        self.calls += 1
        assert groups == 0
        return self._real.gnm_states_assign(fc, cen, W, n, k, self._groups, work, dist, label, stream)


@pytest.mark.parametrize("groups", [1, 3, 40])
def test_window_stride_by_proxy(groups, monkeypatch):
    """171 windows through 1, 3 and 40 groups of four windows (k = 5): 43, 15 and 2 rounds, the last one window short"""
    from gnm import connectome as C
    n, k = 129, 5
    fc, h = device_fc(n)
    whole = C.connectivity_states(fc, k, init=init_windows(k))
    proxy = FewGroups(C.lib, groups)
    monkeypatch.setattr(C, "lib", proxy)
    got = C.connectivity_states(fc, k, init=init_windows(k))
    assert proxy.calls == whole.n_iter
    same_result(got, whole)
    l1, d1 = C.assign_states(fc[:5], whole.centroids)
    assert bits_eq(d1.cpu().numpy(), whole.distances.cpu().numpy()[:5])


@pytest.mark.parametrize("taper", [False, True], ids=["rectangular", "hamming"])
@pytest.mark.parametrize("n,k", [(65, 5), (7, 16)])
def test_series_route_is_bitwise_the_fc_route_at_any_chunk_size(n, k, taper, monkeypatch):
    from gnm import connectome as C
    ts = D.case_series(n)
    w = np.hamming(WINDOW + 2)[1:-1] if taper else None
    fc, h = device_fc(n, taper)
    whole = C.connectivity_states(fc, k, init=init_windows(k))
    assert whole.converged and whole.n_iter >= 3
    if not taper:
        against_oracle(*traced(C.connectivity_states_from_timeseries, ts, k, WINDOW, STRIDE, init=init_windows(k)),
                       oracle(n, k), (n, k, "series"))
    seeded = C.connectivity_states(fc, k, seed=4)
    for windows_per_chunk in (1, 2, 3, 1 << 20):
        monkeypatch.setattr(C, "DYNFC_WORK_BYTES", windows_per_chunk * 8 * n * n)
        assert len(C._plan_chunks(171, n, C.DYNFC_WORK_BYTES)) == -(-171 // windows_per_chunk)
        got = C.connectivity_states_from_timeseries(ts, k, WINDOW, STRIDE, w, init=init_windows(k))
        same_result(got, whole)
        assert got.windows.shape == (171, 3) and got.windows[:, 0].tolist() == [s for s in range(3) for _ in range(57)]
        same_result(C.connectivity_states(fc, k, init=init_windows(k)), whole)      # the FC route in chunks too
        if windows_per_chunk in (2, 1 << 20):
            same_result(C.connectivity_states_from_timeseries(ts, k, WINDOW, STRIDE, w, seed=4), seeded)
    # a list of ragged series on the device, and centroids as the start
    monkeypatch.setattr(C, "DYNFC_WORK_BYTES", 50 * 8 * n * n)
    ragged = [torch.from_numpy(ts[0]).to(DEV), torch.from_numpy(ts[1][:203]).to(DEV), torch.from_numpy(ts[2][:47]).to(DEV)]
    keep = np.concatenate([np.arange(57), 57 + np.arange(37), 114 + np.arange(6)])
    start = h[init_windows(k)]
    a = C.connectivity_states_from_timeseries(ragged, k, WINDOW, STRIDE, w, init=start)
    same_result(a, C.connectivity_states(h[keep], k, init=start))
    assert a.windows[:, 0].tolist() == [0] * 57 + [1] * 37 + [2] * 6


# ------------------------------------------------------------------------------------------------ c. invalid windows
def test_invalid_windows_are_labelled_minus_one_and_enter_nothing():
    from gnm import connectome as C
    n, k = 7, 3
    ts = np.array(D.planted_series(n, seed=99))
    ts[0, 50, 2] = np.nan
    ts[1, 100, 3] = np.inf
    ts[2, 120:160, 4] = 7.0                                     # constant over whole windows: starts 120 .. 140
    poisoned = ~np.isfinite(D.numpy_fc(ts)[:, np.triu_indices(n)[0], np.triu_indices(n)[1]]).all(1)
    assert poisoned.sum() == 4 + 4 + 5 and not poisoned[[0, 1, 2]].any()
    fc = C.dynamic_connectivity_from_timeseries(ts, WINDOW, STRIDE).reshape(-1, n, n)
    h = fc.cpu().numpy()
    valid = np.flatnonzero(~poisoned)
    start = h[valid[[0, 60, 120]]]
    want = D.oracle_run(h[valid], start)
    assert want["margin"] > D.MARGIN and want["n_iter"] >= 3
    st, trace = traced(C.connectivity_states, fc, k, init=start)
    labels = st.labels.cpu().numpy()
    assert np.array_equal(labels == -1, poisoned)
    assert all(np.array_equal(r[2] == -1, poisoned) for r in trace if r[0] == "labels")
    assert not np.isfinite(st.distances.cpu().numpy()[poisoned]).all(1).any()
    # the valid windows alone, on the device and in the oracle
    only, trace_only = traced(C.connectivity_states, fc[torch.from_numpy(valid).to(DEV)], k, init=start)
    against_oracle(only, trace_only, want, "valid only")
    assert [np.array_equal(a[2][valid], b[2]) for a, b in zip(trace, trace_only)] == [True] * len(trace_only)
    assert len(trace) == len(trace_only)
    assert bits_eq(st.centroids.cpu().numpy(), only.centroids.cpu().numpy())
    assert bits_eq(st.counts.cpu().numpy(), only.counts.cpu().numpy()) and st.inertia == only.inertia
    assert int(st.counts.sum()) == valid.shape[0]
    assert bits_eq(st.distances.cpu().numpy()[valid], only.distances.cpu().numpy())      # neighbours are untouched
    # the series route sees the same windows
    same_result(C.connectivity_states_from_timeseries(ts, k, WINDOW, STRIDE, init=start), st)
    stats = C.state_statistics(st.labels, st.windows if st.windows is not None else [57, 57, 57], k)
    assert np.allclose(stats.occupancy.sum(1), 1.0) and stats.transitions.sum() < 171 - 3
    with pytest.raises(ValueError):                             # window 10 covers the NaN row
        C.connectivity_states(fc, k, init=[0, 10, 20])
    with pytest.raises(ValueError):
        C.connectivity_states_from_timeseries(ts, k, WINDOW, STRIDE, init=[0, 10, 20])
    with pytest.raises(ValueError):                             # no valid window at all
        C.connectivity_states(fc[torch.from_numpy(np.flatnonzero(poisoned)).to(DEV)], k, init=start)
    with pytest.raises(ValueError):
        C.connectivity_states(fc[torch.from_numpy(np.flatnonzero(poisoned)).to(DEV)], k)


# ------------------------------------------------------------------------------------------------ d. empty cluster
def test_an_empty_cluster_keeps_its_centroid():
    from gnm.connectome import connectivity_states
    n, k = 63, 5
    fc, h = device_fc(n)
    start = np.array(h[init_windows(k)])
    start[2] = -1.0                                             # farther from every window than any window is
    np.einsum("ii->i", start[2])[:] = 1.0
    want = D.oracle_run(h, start)
    assert want["counts"][2] == 0 and want["margin"] > D.MARGIN and want["n_iter"] >= 3
    st, trace = traced(connectivity_states, fc, k, init=start)
    against_oracle(st, trace, want, "empty cluster")
    assert int(st.counts[2]) == 0 and bits_eq(st.centroids[2].cpu().numpy(), start[2])


# ------------------------------------------------------------------------------------------------ e. max_iter
@pytest.mark.parametrize("max_iter", [1, 2])
def test_max_iter_exhausted_returns_labels_of_the_returned_centroids(max_iter):
    from gnm.connectome import assign_states, connectivity_states
    n, k = 64, 5
    fc, h = device_fc(n)
    assert oracle(n, k)["n_iter"] >= 5
    want = oracle(n, k, max_iter)
    assert not want["converged"] and len(want["history"]) == max_iter + 1
    st, trace = traced(connectivity_states, fc, k, init=init_windows(k), max_iter=max_iter)
    against_oracle(st, trace, want, max_iter)
    assert not st.converged and st.n_iter == max_iter
    labels, dist = assign_states(fc, st.centroids)
    assert bits_eq(labels.cpu().numpy(), st.labels.cpu().numpy())
    assert bits_eq(dist.cpu().numpy(), st.distances.cpu().numpy())
    assert not np.array_equal(trace[-1][2], trace[-2][2])       # the update moved labels: the last assignment matters


# ------------------------------------------------------------------------------------------------ f. k-means++
def test_kmeanspp_seeding():
    from gnm import connectome as C
    n, k = 65, 5
    fc, h = device_fc(n)
    h = np.array(h)
    h[[4, 90]] = np.nan                                          # two invalid windows are never drawn
    fc = torch.from_numpy(h).to(DEV)
    a, trace = traced(C.connectivity_states, fc, k, seed=12, max_iter=1)
    b = C.connectivity_states(fc, k, seed=12, max_iter=1)
    same_result(a, b)
    seeds = [r for r in trace if r[0] == "seed"]
    chosen = [r[2] for r in seeds]
    assert len(seeds) == k and len(set(chosen)) == k and not set(chosen) & {4, 90}
    rng = np.random.default_rng(12)
    for c, (_, d2, w) in enumerate(seeds):
        assert d2.shape == (171,) and np.array_equal(np.isfinite(d2), np.isfinite(h[:, 0, 1]))
        assert C.kmeanspp_draw(d2, rng, first=(c == 0)) == w                    # the device's own vector, numpy's draw
        cen = h[chosen[:c]] if c else np.zeros((1, n, n))
        check_distances(d2, D.oracle_assign(h, cen)[1].min(1), ("seed", c))
        assert c == 0 or not d2[chosen[:c]].any()                               # a chosen window is at distance 0.0
    # the first assignment of the run is against exactly those windows
    first = [r for r in trace if r[0] == "labels"][0][2]
    assert np.array_equal(first, D.oracle_assign(h, h[chosen])[0])
    other = C.connectivity_states(fc, k, seed=13, max_iter=1)
    assert not bits_eq(other.centroids.cpu().numpy(), a.centroids.cpu().numpy())
    full = C.connectivity_states(fc, k, seed=12)
    assert full.converged and np.array_equal(full.labels.cpu().numpy() == -1, np.isnan(h[:, 0, 1]))


# ------------------------------------------------------------------------------------------------ g. states as graphs
def test_centroids_become_graphs_and_states_summarise_subjects():
    from gnm import connectome as C
    from models.graphcnn import GIN_InfoMaxReg
    n, k = 64, 5
    st = C.connectivity_states_from_timeseries(D.case_series(n), k, WINDOW, STRIDE, init=init_windows(k))
    torch.manual_seed(0)
    model = GIN_InfoMaxReg(3, 2, 1, 32, 2, 0.0, True, "sum", "sum", torch.device(DEV)).to(DEV)
    model.eval()
    feats = torch.linspace(-1, 1, n).reshape(n, 1)
    graphs = C.graphs_from_connectivity(model, st.centroids, 30, feats, [0] * k)
    assert len(graphs) == k and all(len(g.g) == n and g.edge_mat.shape[1] > 0 for g in graphs)
    scores = model.predict(graphs)
    assert tuple(scores.shape) == (k, 2) and torch.isfinite(scores).all()
    stats = C.state_statistics(st.labels, st.windows, k)
    assert stats.occupancy.shape == (3, k) and np.allclose(stats.occupancy.sum(1), 1.0)
    assert stats.transitions.sum() == 3 * 56 and (stats.n_transitions > 0).all()
    assert np.array_equal(np.bincount(st.labels.cpu().numpy(), minlength=k), st.counts.cpu().numpy())


# ------------------------------------------------------------------------------------------------ h. arguments
def test_argument_errors_on_the_device():
    from gnm import connectome as C
    n = 7
    fc, h = device_fc(n)
    for k in (0, 17, 172):
        with pytest.raises(ValueError):
            C.connectivity_states(fc, k)
    with pytest.raises(ValueError):
        C.connectivity_states(fc[:4], 5)
    for init in ([0, 3, 3], [0, 1, 171], [0, -1, 2], [0, 1], h[:2], h[:3, :, :5]):
        with pytest.raises(ValueError):
            C.connectivity_states(fc, 3, init=init)
    bad = np.array(h[:3])
    bad[1, 2, 5] = np.nan
    with pytest.raises(ValueError):
        C.connectivity_states(fc, 3, init=bad)
    bad[1, 2, 5] = np.inf
    with pytest.raises(ValueError):
        C.assign_states(fc, bad)
    ok = np.array(h[:3])
    ok[1, 5, 2] = np.nan                                        # below the diagonal: never read
    same_result(C.connectivity_states(fc, 3, init=ok), C.connectivity_states(fc, 3, init=h[:3]))
