"""Shared by the sliding-window tests (tests/test_gpu_dynfc.py, tests/test_gpu_dynfc_long_windows.py and the CPU half
tests/test_dynfc_long_windows_host.py): the numpy reference, the series and tapers, the comparison helpers, the case
tables and a model of the fetch ring of gnm_dynfc_corr (csrc/timeseries.hip).  No tests here.

The short table (NS x WINDOWS) is the feature's design envelope: windows of at most 50 rows, nk = ceil(window / kKt)
<= 4 stages, which the rectangular kernel's prologue fetches whole.  The long table walks past it: the in-loop refill,
a slot refilled twice and more, three and more trips of the outer loop, window % kKt in {0, 1, 15} on the last stage,
and window means longer than one 128-value leaf of numpy's pairwise sum (129, 257 and 1200 rows: one, two and four
levels of the recursion)."""
import re

import numpy as np

NS = [1, 2, 7, 63, 64, 65, 129, 400]              # both sides of the 64-column block, the skipped lower quadrant
WINDOWS = [2, 3, 15, 16, 17, 32, 33, 50]          # both sides of the 16-row stage

LONG_WINDOWS = [64, 65, 80, 81, 128, 129, 143, 257, 1200]
LONG_NS = [1, 7, 64, 65, 129]
LONG_BIG_N = [(400, 65), (400, 129)]              # ten block pairs a window, at the first refill and the second
LONG_CASES = [(n, window) for window in LONG_WINDOWS for n in LONG_NS] + LONG_BIG_N


def long_strides(window):
    return (1, window + 3)                        # overlapping by all but one row, and with rows skipped


def ref_fc(xw, w=None):
    n = xw.shape[1]
    if w is None:
        return np.asarray(np.corrcoef(xw, rowvar=False)).reshape(n, n)
    c = np.atleast_2d(np.cov(xw, rowvar=False, aweights=w))
    s = np.sqrt(np.diag(c)); r = c / s[:, None]; r = r / s[None, :]
    return np.clip(r, -1, 1)


def ref_fc_longdouble(xw, w=None):
    """the same matrix restated in np.longdouble: weighted mean, centred, Xc^T (w * Xc), divided by the two roots"""
    x = np.asarray(xw, dtype=np.longdouble)
    wt = np.ones(x.shape[0], np.longdouble) if w is None else np.asarray(w, dtype=np.longdouble)
    xc = x - (wt[:, None] * x).sum(0) / wt.sum()
    c = xc.T @ (wt[:, None] * xc)
    s = np.sqrt(np.diag(c))
    return c / s[:, None] / s[None, :]


def bits_eq(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def series(rng, T, n, offset=0.0, scale=1.0):
    shared = rng.standard_normal((T, 1))
    return offset + scale * (rng.standard_normal((T, n)) + 0.5 * shared * rng.standard_normal((1, n)))


def tapers(window):
    t = np.arange(window, dtype=np.float64)
    gauss = np.exp(-0.5 * ((t - (window - 1) / 2.0) / (window / 4.0)) ** 2)
    return [None, np.hamming(window + 2)[1:-1], gauss]


TAPER_NAMES = ["none", "hamming", "gaussian"]


def host_windows(ts, window, stride):
    from gnm.connectome import window_starts
    return [(s, k, int(t0)) for s, x in enumerate(ts) for k, t0 in enumerate(window_starts(len(x), window, stride))]


def check_against_numpy(got, xw, w, what):
    with np.errstate(all="ignore"):
        want = ref_fc(xw, w)
    assert got.shape == want.shape and got.dtype == np.float64, what
    assert np.array_equal(np.isnan(got), np.isnan(want)), what
    ok = ~np.isnan(want)
    err = np.abs(got[ok] - want[ok]).max(initial=0.0)
    assert err <= 1e-12, (what, err)
    assert np.all(np.abs(got[ok]) <= 1.0), what
    return err


def nan_windows(got):
    return [k for k in range(got.shape[0]) if np.isnan(got[k]).any()]


def same_graphs(a, b):
    assert len(a) == len(b)
    for g, h in zip(a, b):
        assert np.array_equal(g.edge_mat.numpy(), h.edge_mat.numpy())
        assert g.neighbors == h.neighbors and g.max_neighbor == h.max_neighbor and g.label == h.label
        assert bits_eq(g.node_features.numpy(), h.node_features.numpy())


def ragged_lengths(window, stride):
    """3, 1 and 2 windows, with trailing rows that fill no window where the stride leaves room; the second series is one
    window exactly"""
    return [window + 2 * stride + min(stride - 1, 2), window, window + stride + min(stride - 1, 1)]


def long_case_series(n, window, dtype):
    """[(stride, [three ragged series of `dtype`])] of one long-window case, the same arrays on the CPU and GPU halves:
    the first series of each list carries a 1e5 offset with unit std"""
    rng = np.random.default_rng(1000 * n + window)
    return [(stride, [series(rng, T, n, offset=1e5 if s == 0 else 0.0).astype(dtype)
                      for s, T in enumerate(ragged_lengths(window, stride))]) for stride in long_strides(window)]


def ring_constants(source):
    """(kKt, kDepth rectangular, kDepth tapered) read out of the text of csrc/timeseries.hip"""
    kt = re.search(r"constexpr\s+int\s+kKt\s*=\s*(\d+)\s*;", source)
    depth = re.search(r"constexpr\s+int\s+kDepth\s*=\s*kTaper\s*\?\s*(\d+)\s*:\s*(\d+)\s*;", source)
    assert kt, "csrc/timeseries.hip: `constexpr int kKt = <rows per stage>;` not found: the long-window table " \
               "(tests/dynfc_cases.py) is built on it and has to be revisited"
    assert depth, "csrc/timeseries.hip: `constexpr int kDepth = kTaper ? <tapered> : <rectangular>;` not found: the " \
                  "fetch ring of gnm_dynfc_corr changed and the long-window table (tests/dynfc_cases.py) has to be revisited"
    return int(kt.group(1)), int(depth.group(2)), int(depth.group(1))


def ring_plan(window, tapered, kKt, kDepth):
    """(nk, refills, most refills of one slot, outer trips) of gnm_dynfc_corr's fetch ring at one window length, by
    walking its loops: the prologue fetches stages 0 .. kDepth - 1, iteration kc refills slot kc % kDepth with stage
    kc + kDepth when that stage exists.  kDepth: the depth, or the pair (rectangular, tapered) `tapered` chooses from."""
    depth = int(kDepth[1 if tapered else 0]) if isinstance(kDepth, (tuple, list)) else int(kDepth)
    nk = -(-int(window) // kKt)
    per_slot = [0] * depth
    trips = 0
    for kc0 in range(0, nk, depth):
        trips += 1
        for j in range(depth):
            kc = kc0 + j
            if kc >= nk:
                break
            if kc + depth < nk:
                per_slot[j] += 1
    refills = sum(per_slot)
    assert refills == max(0, nk - depth)
    return nk, refills, max(per_slot), trips
