"""Decoder of the time-series goldens (tests/golden/timeseries/*.npz, made by golden/make_timeseries_goldens.py with the
reference loader): each subject's parsed time series, the loader's fp64 mean_bold z-scores and fp32 node features."""
import glob
import os

import numpy as np

DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "timeseries")
PATHS = sorted(glob.glob(os.path.join(DIR, "*.npz")))


def load(path):
    d = np.load(path)
    S = d["z64"].shape[0]
    ts = [d["ts_k_%d" % s].astype(np.float64) / np.float64(d["ts_scale"]) for s in range(S)]
    return {"ts": ts, "z64": d["z64"], "feat32": d["feat32"], "labels": d["labels"]}


def pairwise_sum(a):
    """numpy's pairwise summation of a 1-D float64 sequence (what np.add.reduce runs on a contiguous axis), restated:
    the order the device's means and z-scores use (csrc/timeseries.hip np_pairwise_sum)"""
    n = len(a)
    if n > 128:
        h = n // 2
        h -= h % 8
        return pairwise_sum(a[:h]) + pairwise_sum(a[h:])
    if n < 8:
        r = np.float64(0.0)
        for v in a:
            r = r + v
        return r
    r = [np.float64(a[j]) for j in range(8)]
    i = 8
    while i < n - n % 8:
        for j in range(8):
            r[j] = r[j] + a[i + j]
        i += 8
    res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]))
    for v in a[i:]:
        res = res + v
    return res


def mean_bold_restated(x):
    """the device's z-scores of one [T, n] float64 series: pairwise column sums over time / T, then dataset.py:73-74
    with pairwise sums over the ROIs"""
    T, n = x.shape
    m = np.array([np.float64(0.0) + pairwise_sum(x[:, c]) for c in range(n)]) / np.float64(T)
    mu = (np.float64(0.0) + pairwise_sum(m)) / np.float64(n)
    d = m - mu
    sd = np.sqrt((np.float64(0.0) + pairwise_sum(d * d)) / np.float64(n))
    return (m - mu) / (sd + 1e-8)
