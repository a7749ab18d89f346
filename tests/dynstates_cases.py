"""Shared by the connectivity-state tests (tests/test_dynstates_host.py, tests/test_gpu_dynstates.py): the planted-state
series, the case table and the numpy oracle of gnm/states.py and csrc/dynstates.hip.  No tests here.

The oracle is the contract restated: features X = fc[:, iu, ju] over np.triu_indices(n, 1); distances
((X - M)**2).sum(-1), argmin, -1 where a row is not finite; a centroid is the Python loop s = s + fc[w] over its members
in ascending order, then s / count on i <= j, mirrored; the iteration of the module's docstring.

margin: the least relative gap (second - best) / second between a valid window's two smallest distances over every
assignment of a run.  A device distance is within (P + 3) 2^-53 <= 1e-11 relative of the oracle's, so above a margin
of 1e-9 the device's argmin cannot differ from the oracle's.  Where both distances are exactly 0.0 (n = 1: no feature,
every sum is empty) the tie is exact on both sides and the smallest index wins on both: counted as no constraint."""
import functools

import numpy as np

NS = [1, 2, 7, 63, 64, 65, 129]         # 63, 64, 65, 129: the last block pair holds 63, 64, 1 and 1 real columns
KS = [1, 2, 5, 16]                      # 16: the register limit of the assignment kernel
CASES = [(n, k) for n in NS for k in KS]
BIG = (400, 5)                          # ten block pairs, about 40 windows
WINDOW, STRIDE, ROWS, SUBJECTS, SEGMENT = 20, 5, 300, 3, 60
MARGIN = 1e-9
DIST_RTOL = 1e-11                       # (P + 3) 2^-53 = 8.9e-12 at n = 400, a sum of P non-negative terms in any order


def bits_eq(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def planted_series(n, subjects=SUBJECTS, rows=ROWS, seed=None):
    """[subjects, rows, n]: every SEGMENT-row stretch is z @ mix[c].T + 0.5 noise with c drawn among 4 mixing matrices
    [n, max(2, n // 3)]"""
    rng = np.random.default_rng(7000 + n if seed is None else seed)
    r = max(2, n // 3)
    mix = rng.standard_normal((4, n, r))
    out = np.empty((subjects, rows, n))
    for s in range(subjects):
        for t0 in range(0, rows, SEGMENT):
            c = int(rng.integers(4))
            m = min(SEGMENT, rows - t0)
            out[s, t0:t0 + m] = rng.standard_normal((m, r)) @ mix[c].T + 0.5 * rng.standard_normal((m, n))
    return out


def big_series():
    """n = 400: 2 subjects of 115 rows, 20 windows each"""
    return planted_series(BIG[0], subjects=2, rows=115)


def init_windows(k):
    return np.arange(k, dtype=np.int64) * 7


def numpy_fc(ts):
    """[W, n, n]: np.corrcoef of every window, subject-major and window-minor"""
    n = ts.shape[2]
    with np.errstate(all="ignore"):
        return np.stack([np.asarray(np.corrcoef(x[t0:t0 + WINDOW], rowvar=False)).reshape(n, n)
                         for x in ts for t0 in range(0, x.shape[0] - WINDOW + 1, STRIDE)])


def oracle_assign(fc, M):
    n = fc.shape[1]
    iu, ju = np.triu_indices(n, 1)
    X = fc[:, iu, ju]
    with np.errstate(all="ignore"):
        d = np.stack([((X - M[c][iu, ju][None]) ** 2).sum(-1) for c in range(M.shape[0])], 1)
    label = np.argmin(np.where(np.isnan(d), np.inf, d), 1).astype(np.int32)
    label[~np.isfinite(d).all(1)] = -1
    return label, d


def oracle_update(fc, M, label):
    M = M.copy()
    n = fc.shape[1]
    for c in range(M.shape[0]):
        members = np.flatnonzero(label == c)
        if members.shape[0] == 0:
            continue
        s = np.zeros((n, n))
        for w in members:
            s = s + fc[w]
        m = np.triu(s / float(members.shape[0]))
        M[c] = m + np.triu(m, 1).T
    return M


def margin_of(d, label):
    ok = label >= 0
    if d.shape[1] < 2 or not ok.any():
        return np.inf
    two = np.sort(d[ok], 1)[:, :2]
    with np.errstate(all="ignore"):
        gap = np.where(two[:, 1] > 0, (two[:, 1] - two[:, 0]) / two[:, 1], np.inf)
    return float(gap.min())


def oracle_run(fc, init, max_iter=100):
    """dict(history: the label vector of every assignment, centroids, labels, dist, counts, inertia, n_iter, converged,
    margin, moved: labels changed by each assignment after the first)"""
    M, prev, history, margin, moved = np.array(init, dtype=np.float64), None, [], np.inf, []
    converged, n_iter = False, 0
    for it in range(1, max_iter + 1):
        n_iter = it
        label, d = oracle_assign(fc, M)
        history.append(label)
        margin = min(margin, margin_of(d, label))
        if prev is not None:
            moved.append(int((label != prev).sum()))
            if moved[-1] == 0:
                converged = True
                break
        M = oracle_update(fc, M, label)
        prev = label
    else:
        label, d = oracle_assign(fc, M)
        history.append(label)
        margin = min(margin, margin_of(d, label))
    inertia = 0.0
    for w in np.flatnonzero(label >= 0):
        inertia = inertia + d[w, label[w]]
    counts = np.bincount(label[label >= 0], minlength=M.shape[0])
    return dict(history=history, centroids=M, labels=label, dist=d, counts=counts, inertia=inertia, n_iter=n_iter,
                converged=converged, margin=margin, moved=moved)


@functools.lru_cache(maxsize=None)
def case_series(n):
    ts = big_series() if n == BIG[0] else planted_series(n)
    ts.setflags(write=False)
    return ts


def check_distances(got, want, what):
    """|got - want| <= DIST_RTOL max(want, 1) where want is finite, the same non-finite pattern elsewhere; the worst
    ratio |got - want| / max(want, 1)"""
    fin = np.isfinite(want)
    assert np.array_equal(np.isfinite(got), fin), what
    err = np.abs(got[fin] - want[fin]) / np.maximum(want[fin], 1.0)
    worst = float(err.max(initial=0.0))
    assert worst <= DIST_RTOL, (what, worst)
    return worst


def loop_statistics(labels, counts, k):
    """state_statistics restated as plain Python loops over one subject at a time"""
    occ, dwell, trans, ntr = [], [], [], []
    o = 0
    for cnt in counts:
        seg = [int(v) for v in labels[o:o + cnt]]
        o += cnt
        valid = [v for v in seg if v >= 0]
        occ.append([valid.count(c) / len(valid) if valid else 0.0 for c in range(k)])
        runs = [[] for _ in range(k)]
        t = 0
        while t < len(seg):
            u = t
            while u + 1 < len(seg) and seg[u + 1] == seg[t]:
                u += 1
            if seg[t] >= 0:
                runs[seg[t]].append(u - t + 1)
            t = u + 1
        dwell.append([sum(r) / len(r) if r else 0.0 for r in runs])
        tr = [[0] * k for _ in range(k)]
        for a, b in zip(seg[:-1], seg[1:]):
            if a >= 0 and b >= 0:
                tr[a][b] += 1
        trans.append(tr)
        ntr.append(sum(tr[a][b] for a in range(k) for b in range(k) if a != b))
    return np.array(occ).reshape(len(counts), k), np.array(dwell).reshape(len(counts), k), \
        np.array(trans, dtype=np.int64).reshape(len(counts), k, k), np.array(ntr, dtype=np.int64)
