"""The device time-series path (gnm/connectome.py, csrc/timeseries.hip) on the GPU: FC within 1e-12 of np.corrcoef
with numpy's NaN pattern, results bitwise independent of the launch a subject is in, mean_bold features against the
reference loader's goldens, and graphs and model outputs equal to those built from the host's np.corrcoef."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
import timeseries_goldens

GOLDEN = timeseries_goldens.PATHS


def corrcoef(x):
    """np.corrcoef(x, rowvar=False) as an [n, n] array (numpy returns a scalar for n = 1)"""
    n = x.shape[1]
    return np.asarray(np.corrcoef(x, rowvar=False)).reshape(n, n)


def bits_eq(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def series(rng, T, n, offset=0.0, scale=1.0):
    shared = rng.standard_normal((T, 1))
    return offset + scale * (rng.standard_normal((T, n)) + 0.5 * shared * rng.standard_normal((1, n)))


@pytest.mark.parametrize("T", [2, 3, 50, 1200])
@pytest.mark.parametrize("n", [1, 2, 7, 16, 17, 63, 400, 1000])
def test_fc_matches_corrcoef(n, T):
    from gnm.connectome import connectivity_from_timeseries
    rng = np.random.default_rng(1000 * n + T)
    ts = np.stack([series(rng, T, n), series(rng, T, n, offset=1e5)])      # the second: a large offset, unit std
    got = connectivity_from_timeseries(ts).cpu().numpy()
    assert got.shape == (2, n, n) and got.dtype == np.float64
    for s in range(2):
        want = corrcoef(ts[s])
        assert np.array_equal(np.isnan(got[s]), np.isnan(want)), (n, T, s)
        ok = ~np.isnan(want)
        err = np.abs(got[s][ok] - want[ok]).max(initial=0.0)
        assert err <= 1e-12, (n, T, s, err)
        assert np.all(np.abs(got[s][ok]) <= 1.0)
    if n >= 2 and T >= 50:
        # the offset case tells a one-pass covariance apart: X^T X - T m m^T is far outside the bound
        x = ts[1]
        m = x.mean(0)
        c = (x.T @ x - T * np.outer(m, m)) / (T - 1)
        sd = np.sqrt(np.diag(c))
        assert np.nanmax(np.abs(np.clip(c / sd[:, None] / sd[None, :], -1, 1) - corrcoef(x))) > 1e-9


def test_bitwise_independent_of_the_launch():
    from gnm.connectome import connectivity_from_timeseries, mean_bold_features
    rng = np.random.default_rng(7)
    n = 70
    stack = np.stack([series(rng, 120, n, offset=3e3 * s) for s in range(3)])
    ragged = [series(rng, 33, n), stack[1], series(rng, 250, n, offset=10.0), stack[2][:1]]
    fc_alone = connectivity_from_timeseries(stack[1:2]).cpu().numpy()[0]
    fc_stack = connectivity_from_timeseries(stack).cpu().numpy()[1]
    fc_ragged = connectivity_from_timeseries(ragged).cpu().numpy()[1]
    fc_dev = connectivity_from_timeseries([torch.from_numpy(a).to(DEV) for a in ragged]).cpu().numpy()[1]
    assert bits_eq(fc_alone, fc_stack) and bits_eq(fc_alone, fc_ragged) and bits_eq(fc_alone, fc_dev)
    for dt in (torch.float32, torch.float64):
        z = [mean_bold_features(stack[1:2], dtype=dt), mean_bold_features(stack, dtype=dt)[1:2],
             mean_bold_features(ragged, dtype=dt)[1:2]]
        assert all(bits_eq(z[0].cpu().numpy(), w.cpu().numpy()) for w in z[1:])
    # float32 input: bitwise the widened float64 input
    f32 = stack.astype(np.float32)
    wide = f32.astype(np.float64)
    assert bits_eq(connectivity_from_timeseries(f32).cpu().numpy(), connectivity_from_timeseries(wide).cpu().numpy())
    assert bits_eq(connectivity_from_timeseries(torch.from_numpy(f32).to(DEV)).cpu().numpy(),
                   connectivity_from_timeseries(wide).cpu().numpy())
    assert bits_eq(mean_bold_features(f32).cpu().numpy(), mean_bold_features(wide).cpu().numpy())
    r32 = [a.astype(np.float32) for a in ragged]
    assert bits_eq(connectivity_from_timeseries(r32).cpu().numpy(),
                   connectivity_from_timeseries([a.astype(np.float64) for a in r32]).cpu().numpy())


def test_nan_pattern_is_numpys():
    from gnm.connectome import connectivity_from_timeseries
    rng = np.random.default_rng(3)
    cases = []
    x = series(rng, 40, 9)
    x[:, 4] = 7.0                                       # a constant ROI (its mean is exact)
    cases.append(x)
    cases.append(series(rng, 1, 9))                     # T = 1: all NaN
    x = series(rng, 40, 9)
    x[5, 2] = np.nan
    cases.append(x)
    x = series(rng, 40, 9)
    x[11, 6] = np.inf
    cases.append(x)
    x = series(rng, 40, 9)
    x[0, 1] = -np.inf
    x[:, 8] = 0.0
    cases.append(x)
    cases.append(np.full((5, 1), 2.0))                  # n = 1, constant: c / c = NaN
    cases.append(series(rng, 5, 1))                     # n = 1: exactly 1.0
    for k, x in enumerate(cases):
        with np.errstate(all="ignore"):
            want = corrcoef(x)
        got = connectivity_from_timeseries([x]).cpu().numpy()[0]
        assert np.array_equal(np.isnan(got), np.isnan(want)), k
        assert np.isnan(want).any() or x.shape[1] == 1, k
        ok = ~np.isnan(got)
        assert np.all(np.abs(got[ok]) <= 1.0), k
        assert np.abs(got[ok] - want[ok]).max(initial=0.0) <= 1e-12, k
    assert connectivity_from_timeseries([cases[-1]]).cpu().numpy()[0, 0, 0] == 1.0


def ulp_diff32(a, b):
    a = np.asarray(a, np.float32).view(np.int32).astype(np.int64)
    b = np.asarray(b, np.float32).view(np.int32).astype(np.int64)
    a = np.where(a < 0, -(a & 0x7fffffff), a)
    b = np.where(b < 0, -(b & 0x7fffffff), b)
    return np.abs(a - b)


@pytest.mark.parametrize("path", GOLDEN, ids=[os.path.basename(p) for p in GOLDEN])
def test_mean_bold_equals_the_reference_loader(path):
    from gnm.connectome import mean_bold_features
    d = timeseries_goldens.load(path)
    z64 = mean_bold_features(d["ts"], dtype=torch.float64).cpu().numpy()[..., 0]
    z32 = mean_bold_features(d["ts"]).cpu().numpy()[..., 0]
    want64, want32 = d["z64"], d["feat32"]
    assert z64.shape == want64.shape and z32.dtype == np.float32
    rel = np.abs(z64 - want64) / np.abs(want64).max(axis=1, keepdims=True)
    assert rel.max() <= 1e-13, rel.max()
    assert ulp_diff32(z32, want32).max() <= 1
    print("%s: %d of %d fp64 z-scores and %d fp32 features differ from the loader's"
          % (os.path.basename(path), int((z64 != want64).sum()), z64.size, int((z32 != want32).sum())))


def test_mean_bold_equals_numpy_on_random_stacks():
    from gnm.connectome import mean_bold_features
    rng = np.random.default_rng(11)
    for S, T, n in ((3, 300, 50), (2, 1200, 400), (4, 7, 3), (1, 1, 5)):
        ts = np.stack([series(rng, T, n, offset=1e4 * (s + 1), scale=50.0) for s in range(S)])
        z64 = mean_bold_features(ts, dtype=torch.float64).cpu().numpy()[..., 0]
        z32 = mean_bold_features(ts).cpu().numpy()[..., 0]
        for s in range(S):
            with np.errstate(all="ignore"):
                m = np.asfortranarray(ts[s]).mean(0)                # numpy on the loader's (column-major) layout
                loader = (m - m.mean()) / (m.std() + 1e-8)
                m = ts[s].mean(0)                                   # numpy on the row-major array
                plain = (m - m.mean()) / (m.std() + 1e-8)
            scale = max(np.abs(loader).max(), 1e-300)
            assert np.abs(z64[s] - timeseries_goldens.mean_bold_restated(ts[s])).max() / scale <= 1e-13
            assert np.abs(z64[s] - loader).max() / scale <= 1e-13
            assert ulp_diff32(z32[s], loader.astype(np.float32)).max() <= 1
            # numpy's two layouts sum the column means in different orders; with means near 1e4 and a spread of
            # about 1.5 their z-scores differ by up to ~1e-11 relative, so the row-major bound is numpy's own spread
            assert np.abs(z64[s] - plain).max() / scale <= 1e-10
            assert ulp_diff32(z32[s], plain.astype(np.float32)).max() <= 1


def host_graph(fc, sp, feat, label):
    """the graph load_data builds from one FC matrix, on the host (np.percentile, np.triu, networkx's order)"""
    from gnm.connectome import order_graph
    from gnm.synth import SynthGraph
    n = fc.shape[0]
    iu, ju = np.nonzero(np.triu(fc > np.percentile(fc, 100 - sp), 1))
    em, nb, mx = order_graph(n, iu, ju)
    h = SynthGraph(n, em[:, :em.shape[1] // 2].T, feat, label)
    assert np.array_equal(h.edge_mat.numpy(), em)
    h.neighbors, h.max_neighbor = nb, mx
    return h


def well_separated(fc, sp):
    """no entry within 1e-10 of numpy's threshold.  Each value of R sits next to its mirror (equal, or one ulp apart),
    so the two order statistics the percentile reads are often one entry and its mirror: then the edge depends on
    which of the two is larger, which a 1e-13 difference can flip.  Such data cannot be compared edge for edge."""
    return not (np.abs(fc - np.percentile(fc, 100 - sp)) < 1e-10).any()


def separated_series(sp, n, Ts):
    """the first of a fixed sequence of draws whose host FC passes well_separated for every subject"""
    for seed in range(100 * sp, 100 * sp + 50):
        rng = np.random.default_rng(seed)
        ts = [series(rng, T, n, offset=500.0 * s) for s, T in enumerate(Ts)]
        fc = np.stack([corrcoef(x) for x in ts])
        if all(well_separated(fc[s], sp) for s in range(len(ts))):
            return ts, fc
    raise AssertionError("no well-separated draw")


# n with the two order statistics of percentile(100 - sp) in different value pairs: the sorted off-diagonal values come
# in (entry, mirror) pairs at positions 2m, 2m + 1, so an even k_lo would always read an entry and its own mirror
@pytest.mark.parametrize("sp,n", [(5, 93), (30, 90), (50, 90)])
def test_graphs_equal_those_of_the_host_corrcoef(sp, n):
    from gnm.arena import GraphArena
    from gnm.connectome import graphs_from_connectivity, graphs_from_timeseries
    ts, fc = separated_series(sp, n, (60, 200, 45, 120))
    labels = [0, 1, 1, 0]
    feat = np.ones((n, 2), np.float32)
    ar = GraphArena(DEV)
    dev = graphs_from_timeseries(ar, ts, sp, labels, node_features=feat)
    host = graphs_from_connectivity(ar, fc, sp, feat, labels)
    for g, h in zip(dev, host):
        assert np.array_equal(g.edge_mat.numpy(), h.edge_mat.numpy()), sp
        assert g.neighbors == h.neighbors and g.max_neighbor == h.max_neighbor and g.label == h.label
        assert np.array_equal(g.node_features.numpy(), feat)
    mb = graphs_from_timeseries(GraphArena(DEV), ts, sp, labels)       # mean_bold features
    for s, g in enumerate(mb):
        assert g.node_features.shape == (n, 1) and g.node_features.dtype == torch.float32
        assert np.array_equal(g.edge_mat.numpy(), dev[s].edge_mat.numpy())


@pytest.mark.parametrize("npool", ["sum", "average", "max"])
def test_mean_bold_model_outputs_equal_host_built(npool):
    from gnm.connectome import connectivity_from_timeseries, graphs_from_timeseries, mean_bold_features
    from models.graphcnn import GIN_InfoMaxReg
    rng = np.random.default_rng(5)
    n, S = 64, 5
    ts = [series(rng, T, n, offset=1e4, scale=80.0) for T in (100, 150, 90, 100, 300)]
    torch.manual_seed(0)
    model = GIN_InfoMaxReg(3, 2, 1, 32, 2, 0.0, True, "average" if npool == "average" else "sum", npool,
                           torch.device(DEV)).to(DEV)
    labels = [s % 2 for s in range(S)]
    gs = graphs_from_timeseries(model, ts, 30, labels)
    fc = connectivity_from_timeseries(ts).cpu().numpy()
    feat = mean_bold_features(ts).cpu().numpy()
    hs = [host_graph(fc[s], 30, feat[s], labels[s]) for s in range(S)]
    for g, h in zip(gs, hs):
        assert np.array_equal(g.edge_mat.numpy(), h.edge_mat.numpy())
        assert bits_eq(g.node_features.numpy(), h.node_features.numpy())
    model.eval()
    assert bits_eq(model.predict(gs).cpu().numpy(), model.predict(hs).cpu().numpy())
    assert bits_eq(model.saliency(gs, (0, 1)).cpu().numpy(), model.saliency(hs, (0, 1)).cpu().numpy())
