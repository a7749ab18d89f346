"""CPU half of the connectivity-state tests (gnm/states.py, csrc/dynstates.hip): the numpy oracle of
tests/dynstates_cases.py against an independent restatement, the margin condition the GPU label comparison rests on,
state_statistics against plain loops, the k-means++ draw on fixed vectors, and the argument checks that need no device.
The header, gnm/_cabi.py SIGNATURES and the library agreeing on the new symbols is tests/test_cabi_host.py's."""
import numpy as np
import pytest
import torch

import dynstates_cases as D
from dynstates_cases import bits_eq


# ------------------------------------------------------------------------------------------------ the oracle
def restated_run(fc, init, max_iter=100):
    """the same iteration written differently: distances from masked full matrices one window at a time, centroids
    from np.cumsum along the member axis (sequential by definition)"""
    n = fc.shape[1]
    upper = np.triu(np.ones((n, n), bool), 1)
    M, prev, history = np.array(init, dtype=np.float64), None, []
    for _ in range(max_iter):
        d = np.empty((fc.shape[0], M.shape[0]))
        for w in range(fc.shape[0]):
            for c in range(M.shape[0]):
                diff = np.where(upper, fc[w] - M[c], 0.0)
                d[w, c] = np.sum(diff * diff)
        label = np.array([int(np.argmin(r)) if np.isfinite(r).all() else -1 for r in d], dtype=np.int32)
        history.append(label)
        if prev is not None and np.array_equal(label, prev):
            break
        for c in range(M.shape[0]):
            members = fc[label == c]
            if len(members):
                m = np.cumsum(members, axis=0)[-1] / float(len(members))
                for i in range(n):
                    for j in range(i, n):
                        M[c, i, j] = M[c, j, i] = m[i, j]
        prev = label
    return history, M, d


@pytest.mark.parametrize("n,k", [(7, 5), (5, 3)])
def test_oracle_against_an_independent_restatement(n, k):
    ts = D.planted_series(n, seed=11 + n)
    fc = D.numpy_fc(ts)
    fc[13] = np.nan                                             # one invalid window: label -1, enters nothing
    init = fc[D.init_windows(k)]
    got = D.oracle_run(fc, init)
    history, M, d = restated_run(fc, init)
    assert got["converged"] and got["n_iter"] == len(history) >= 3
    assert all(np.array_equal(a, b) for a, b in zip(got["history"], history))
    assert got["labels"][13] == -1 and (got["labels"] >= 0).sum() == fc.shape[0] - 1
    assert bits_eq(got["centroids"], M)
    assert np.array_equal(got["centroids"], got["centroids"].transpose(0, 2, 1))
    ok = got["labels"] >= 0
    assert np.abs(got["dist"][ok] - d[ok]).max() <= 1e-12 * max(1.0, d[ok].max())
    assert got["counts"].sum() == ok.sum()
    assert got["inertia"] == pytest.approx(d[ok, got["labels"][ok]].sum(), rel=1e-12)


def test_oracle_keeps_an_empty_clusters_centroid_and_reports_max_iter():
    fc = D.numpy_fc(D.planted_series(7))
    init = fc[D.init_windows(3)].copy()
    init[1] = -1.0
    got = D.oracle_run(fc, init)
    assert got["counts"][1] == 0 and bits_eq(got["centroids"][1], init[1]) and got["converged"]
    short = D.oracle_run(fc, fc[D.init_windows(2)], max_iter=2)
    assert not short["converged"] and short["n_iter"] == 2 and len(short["history"]) == 3
    assert np.array_equal(short["labels"], D.oracle_assign(fc, short["centroids"])[0])


# ------------------------------------------------------------------------------------------------ the margin condition
@pytest.mark.parametrize("n,k", D.CASES + [D.BIG])
def test_every_gpu_case_has_an_oracle_margin_above_the_bound(n, k):
    """a condition of the GPU label comparison, not a tolerance: with np.corrcoef's FC (within 1e-12 of the device's)
    the two smallest distances of every window differ by more than 1e-9 relative at every assignment"""
    fc = D.numpy_fc(D.case_series(n))
    assert fc.shape[0] == (40 if (n, k) == D.BIG else 171)
    got = D.oracle_run(fc, fc[D.init_windows(k)])
    assert got["converged"] and got["margin"] > D.MARGIN, (n, k, got["margin"])
    if n >= 2 and k >= 2:
        assert np.isfinite(got["margin"])
        if (n, k) != D.BIG:
            assert 3 <= got["n_iter"] <= 30 and all(m > 0 for m in got["moved"][:-1]) and got["moved"][0] >= 5
    else:
        assert got["n_iter"] == 2 and (got["labels"] == 0).all()          # no feature, or one state


# ------------------------------------------------------------------------------------------------ state_statistics
STAT_CASES = {
    "run_ends_at_a_subject_boundary": ([0, 0, 1, 1, 1, 1, 1, 0, 2], [5, 4], 3),
    "invalid_inside_a_run": ([1, 1, -1, 1, 1, 1, 0, -1, -1, 0], [10], 2),
    "state_never_visited": ([0, 0, 2, 2, 0, 3, 3, 3], [4, 4], 5),
    "subject_with_one_window": ([1, 0, 0, 1, 2], [1, 3, 1], 3),
    "ragged_counts": ([0, 1, 0, 1, 1, 1, -1, 2, 2, 0, 0, 0, 0, 1, 2, 2, -1], [2, 7, 0, 5, 3], 3),
    "all_invalid_subject": ([-1, -1, 0, 0], [2, 2], 1),
}


@pytest.mark.parametrize("name", sorted(STAT_CASES))
def test_state_statistics_against_plain_loops(name):
    from gnm.connectome import state_statistics
    labels, counts, k = STAT_CASES[name]
    want = D.loop_statistics(labels, counts, k)
    windows = np.array([(s, i, 5 * i) for s, c in enumerate(counts) for i in range(c)], dtype=np.int64).reshape(-1, 3)
    forms = [(np.array(labels, dtype=np.int32), np.array(counts)),
             (torch.tensor(labels, dtype=torch.int32), torch.tensor(counts))]
    if all(c > 0 for c in counts):                              # the table cannot name a subject without windows
        forms.append((np.array(labels), windows))
    for lab, wc in forms:
        got = state_statistics(lab, wc, k)
        assert bits_eq(got.occupancy, want[0]) and bits_eq(got.dwell, want[1])
        assert bits_eq(got.transitions, want[2]) and bits_eq(got.n_transitions, want[3])


def test_state_statistics_by_hand():
    from gnm.connectome import state_statistics
    got = state_statistics([0, 0, 1, -1, 1, 1, 2], [6, 1], 3)
    assert got.occupancy.tolist() == [[0.4, 0.6, 0.0], [0.0, 0.0, 1.0]]
    assert got.dwell.tolist() == [[2.0, 1.5, 0.0], [0.0, 0.0, 1.0]]              # the -1 splits state 1's run: 1 and 2
    assert got.transitions[0].tolist() == [[1, 1, 0], [0, 1, 0], [0, 0, 0]] and not got.transitions[1].any()
    assert got.n_transitions.tolist() == [1, 0]
    for bad in (([0, 1], [3], 2), ([0, 2], [2], 2), ([0, -2], [2], 2), ([0.5, 1.0], [2], 2), ([0, 1], [2], 0)):
        with pytest.raises(ValueError):
            state_statistics(*bad)


# ------------------------------------------------------------------------------------------------ the k-means++ draw
class FixedRng:
    """a generator whose next random() and integers() are given"""

    def __init__(self, u=None, i=None):
        self.u, self.i = u, i

    def random(self):
        return self.u

    def integers(self, n):
        assert 0 <= self.i < n
        return self.i


def test_kmeanspp_draw_on_fixed_vectors():
    from gnm.connectome import kmeanspp_draw
    d2 = np.array([0.0, 1.0, 0.0, 3.0, np.nan, 4.0, np.inf, 0.0])             # cumulative 0 1 1 4 4 8 8 8
    for u, want in ((0.0, 1), (0.1249, 1), (0.125, 3), (0.4999, 3), (0.5, 5), (0.999, 5), (1.0, 5)):
        assert kmeanspp_draw(d2, FixedRng(u=u)) == want, u
    single = np.array([0.0, 0.0, 2.5, 0.0])
    assert all(kmeanspp_draw(single, FixedRng(u=u)) == 2 for u in (0.0, 0.3, 1.0 - 2.0 ** -53))
    with pytest.raises(ValueError):
        kmeanspp_draw(np.zeros(5), FixedRng(u=0.5))                            # only centres already chosen are left
    with pytest.raises(ValueError):
        kmeanspp_draw(np.array([np.nan, 0.0]), FixedRng(u=0.5))
    # the first centre: uniform over the finite entries, whatever their values
    assert [kmeanspp_draw(d2, FixedRng(i=i), first=True) for i in range(6)] == [0, 1, 2, 3, 5, 7]
    with pytest.raises(ValueError):
        kmeanspp_draw(np.array([np.nan, np.inf]), FixedRng(i=0), first=True)
    # a real generator: the same seed draws the same window, and the frequencies follow the weights
    a = [kmeanspp_draw(d2, np.random.default_rng(5)) for _ in range(2)]
    assert a[0] == a[1]
    rng = np.random.default_rng(0)
    hits = np.bincount([kmeanspp_draw(d2, rng) for _ in range(4000)], minlength=8)
    assert hits[[0, 2, 4, 6, 7]].sum() == 0 and np.abs(hits[[1, 3, 5]] / 4000 - np.array([1, 3, 4]) / 8).max() < 0.03


# ------------------------------------------------------------------------------------------------ arguments
def test_argument_errors_that_need_no_device():
    from gnm import connectome as C
    assert int(C.lib.gnm_states_max_k()) == 16
    assert int(C.lib.gnm_states_workspace_doubles(10, 65, 3)) == 10 * 3 * 3
    assert int(C.lib.gnm_states_workspace_doubles(10, 5000, 3)) == 0 == int(C.lib.gnm_states_workspace_doubles(1, 7, 17))
    fc = np.zeros((20, 5, 5))
    ts = np.zeros((2, 40, 5))                                                   # window 20, stride 5: 10 windows
    for k in (0, 17, 21, 2.0, True):
        with pytest.raises(ValueError):
            C.connectivity_states(fc, k)
    for k in (0, 17, 11):
        with pytest.raises(ValueError):
            C.connectivity_states_from_timeseries(ts, k, 20, 5)
    for init in ([0, 3, 3], [0, 1, 20], [0, -1, 2], [0, 1], np.zeros((3, 5, 4)), np.zeros((2, 5, 5)),
                 np.zeros((3, 5, 5), np.int64), [0.0, 1.0, 2.0], np.zeros((3, 3))):
        with pytest.raises(ValueError):
            C.connectivity_states(fc, 3, init=init)
    with pytest.raises(ValueError):
        C.connectivity_states_from_timeseries(ts, 3, 20, 5, init=[0, 1, 10])
    for max_iter in (0, -1, 1.5):
        with pytest.raises(ValueError):
            C.connectivity_states(fc, 3, max_iter=max_iter)
    with pytest.raises(ValueError):
        C.connectivity_states(np.zeros((4, 5, 6)), 2)
    with pytest.raises(ValueError):
        C.connectivity_states_from_timeseries(ts, 2, 41, 5)                    # the window plan's own checks
    # the null-pointer and range checks of the C entry points run before any launch
    lib = C.lib
    assert lib.gnm_states_assign(None, None, 4, 5, 2, 0, None, None, None, None) == -1
    assert lib.gnm_states_assign(None, None, 0, 5, 2, 0, None, None, None, None) == 0
    assert lib.gnm_states_assign(None, None, 4, 5, 17, 0, None, None, None, None) == -2
    assert lib.gnm_states_assign(None, None, 4, 5, 2, -1, None, None, None, None) == -1
    assert lib.gnm_states_accumulate(None, None, 4, 5000, 2, None, None, None) == -2
    assert lib.gnm_states_accumulate(None, None, 4, 5, 2, None, None, None) == -1
    assert lib.gnm_states_finish(None, None, 5, 2, None, None) == -1
    assert lib.gnm_states_inertia(None, None, 0, 2, None, None) == -1


def test_states_have_no_cpu_fallback():
    from gnm import connectome as C
    from gnm._cabi import GnmError
    with pytest.raises(GnmError):
        C.connectivity_states(np.zeros((20, 5, 5)), 3, device="cpu")
    with pytest.raises(GnmError):
        C.connectivity_states_from_timeseries(np.zeros((2, 40, 5)), 3, 20, 5, device="cpu")
