"""The sliding-window path (gnm/connectome.py dynamic_connectivity_from_timeseries, dynamic_graphs_from_timeseries;
csrc/timeseries.hip gnm_dynfc_means, gnm_dynfc_corr) on the GPU: every window's FC within 1e-12 of numpy with numpy's NaN
pattern, rectangular and tapered; bitwise independent of the call a window is part of; per-window mean_bold features
bitwise the static path's; graphs and model outputs bitwise those built from the materialised FC, whatever the chunking.

The bound 1e-12 is the static path's.  Worst |R - numpy| measured over the accuracy cases below: 1.0e-15
(DESIGN.md 3.17)."""
import numpy as np
import pytest
import torch

from dynfc_cases import (NS, WINDOWS, bits_eq, check_against_numpy, host_windows, nan_windows, same_graphs, series,
                         tapers)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.mark.parametrize("window", WINDOWS)
@pytest.mark.parametrize("n", NS)
def test_every_window_matches_numpy(n, window):
    from gnm.connectome import dynamic_connectivity_from_timeseries
    rng = np.random.default_rng(1000 * n + window)
    worst = 0.0
    for stride in (1, 7, window, window + 3):
        # ragged, with trailing rows that fill no window where the stride leaves room; the first series carries a 1e5
        # offset with unit std; the second is one window exactly
        Ts = [window + 2 * stride + min(stride - 1, 2), window, window + stride + min(stride - 1, 1)]
        ts = [series(rng, T, n, offset=1e5 if s == 0 else 0.0) for s, T in enumerate(Ts)]
        where = host_windows(ts, window, stride)
        assert [sum(1 for v in where if v[0] == s) for s in range(3)] == [3, 1, 2]
        for w in tapers(window):
            got = dynamic_connectivity_from_timeseries(ts, window, stride, taper=w)
            assert isinstance(got, list) and [int(g.shape[0]) for g in got] == [3, 1, 2]
            for s, k, t0 in where:
                err = check_against_numpy(got[s][k].cpu().numpy(), ts[s][t0:t0 + window], w,
                                          (n, window, stride, w is not None, s, k))
                worst = max(worst, err)
    print("n %d window %d: worst |R - numpy| %.3e" % (n, window, worst))


def test_stack_shape_and_windows():
    from gnm.connectome import dynamic_connectivity_from_timeseries
    rng = np.random.default_rng(2)
    ts = np.stack([series(rng, 41, 7) for _ in range(3)])
    got = dynamic_connectivity_from_timeseries(ts, 10, 4)
    assert tuple(got.shape) == (3, 8, 7, 7) and got.dtype == torch.float64 and got.is_cuda
    got = got.cpu().numpy()
    for s in range(3):
        for k in range(8):
            check_against_numpy(got[s, k], ts[s, 4 * k:4 * k + 10], None, (s, k))


def test_constant_roi_inside_exactly_one_rectangular_window():
    from gnm.connectome import dynamic_connectivity_from_timeseries
    rng = np.random.default_rng(3)
    x = series(rng, 40, 9)
    x[16:24, 4] = 7.0                                   # window 2 of the stride-8 tiling, and no other
    got = dynamic_connectivity_from_timeseries([x], 8, 8)[0].cpu().numpy()
    assert got.shape[0] == 5 and nan_windows(got) == [2]
    want = np.zeros((9, 9), bool)
    want[4, :] = want[:, 4] = True
    assert np.array_equal(np.isnan(got[2]), want)
    for k in range(5):
        check_against_numpy(got[k], x[8 * k:8 * k + 8], None, k)
    # the same rows at stride 1: only the window that starts at row 16 lies inside the constant stretch
    got = dynamic_connectivity_from_timeseries([x], 8, 1)[0].cpu().numpy()
    assert nan_windows(got) == [16]


def test_nan_and_inf_reach_exactly_the_windows_that_cover_their_row():
    from gnm.connectome import dynamic_connectivity_from_timeseries, window_starts
    rng = np.random.default_rng(4)
    x = series(rng, 40, 9)
    x[13, 2] = np.nan
    x[13, 6] = np.inf
    starts = window_starts(40, 8, 3)
    cover = [k for k, t0 in enumerate(starts) if t0 <= 13 < t0 + 8]
    assert cover == [2, 3, 4]
    for w in tapers(8):
        got = dynamic_connectivity_from_timeseries([x], 8, 3, taper=w)[0].cpu().numpy()
        assert nan_windows(got) == cover
        for k, t0 in enumerate(starts):
            check_against_numpy(got[k], x[t0:t0 + 8], w, (k, w is not None))
        want = np.zeros((9, 9), bool)
        want[[2, 6], :] = want[:, [2, 6]] = True
        assert all(np.array_equal(np.isnan(got[k]), want) for k in cover)


def test_non_finite_value_under_a_zero_weight_still_poisons_its_window():
    from gnm.connectome import dynamic_connectivity_from_timeseries
    rng = np.random.default_rng(5)
    w = np.array([0.0, 1.0, 2.0, 3.0, 3.0, 2.0, 1.0, 0.0])
    for bad in (np.inf, -np.inf, np.nan):
        x = series(rng, 40, 9)
        x[16, 3] = bad                                  # first row of window 2: weight 0, and x * w is NaN in numpy
        got = dynamic_connectivity_from_timeseries([x], 8, 8, taper=w)[0].cpu().numpy()
        assert nan_windows(got) == [2]
        for k in range(5):
            check_against_numpy(got[k], x[8 * k:8 * k + 8], w, (bad, k))
        assert np.isnan(got[2][3]).all() and np.isnan(got[2][:, 3]).all()


def test_a_windows_fc_is_bitwise_independent_of_the_call():
    from gnm.connectome import dynamic_connectivity_from_timeseries as dfc
    rng = np.random.default_rng(7)
    n, window = 70, 20
    stack = np.stack([series(rng, 61, n, offset=3e3 * s) for s in range(3)])
    ragged = [series(rng, 33, n), stack[1], series(rng, 25, n, offset=10.0)]
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
        one = dfc([stack[1][15:35]], window, 1, taper=w)[0].cpu().numpy()                   # the window's rows alone
        assert bits_eq(one[0], alone[15])
        f32 = stack.astype(np.float32)
        wide = f32.astype(np.float64)
        assert bits_eq(dfc(f32, window, 6, taper=w).cpu().numpy(), dfc(wide, window, 6, taper=w).cpu().numpy())
        assert bits_eq(dfc(torch.from_numpy(f32).to(DEV), window, 6, taper=w).cpu().numpy(),
                       dfc(wide, window, 6, taper=w).cpu().numpy())


def test_rectangular_window_is_the_static_path_within_its_bound():
    """the static route on the explicit slices is the only other way to these matrices: both are within 1e-12 of numpy"""
    from gnm.connectome import connectivity_from_timeseries, dynamic_connectivity_from_timeseries
    rng = np.random.default_rng(8)
    x = series(rng, 80, 129, offset=1e4)
    got = dynamic_connectivity_from_timeseries([x], 50, 10)[0].cpu().numpy()
    static = connectivity_from_timeseries([x[t0:t0 + 50] for t0 in range(0, 31, 10)]).cpu().numpy()
    assert got.shape == static.shape and np.abs(got - static).max() <= 2e-12


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_window_mean_bold_is_bitwise_the_static_paths(dtype):
    from gnm import connectome as C
    from gnm.arena import GraphArena
    rng = np.random.default_rng(11)
    n, window, stride = 50, 33, 7
    ts = [series(rng, T, n, offset=1e4 * (s + 1), scale=50.0).astype(dtype) for s, T in enumerate((60, 33, 150))]
    where = host_windows(ts, window, stride)
    slices = [ts[s][t0:t0 + window] for s, _, t0 in where]
    want32 = C.mean_bold_features(slices).cpu().numpy()
    want64 = C.mean_bold_features(slices, dtype=torch.float64).cpu().numpy()
    for w in (None, np.hamming(window + 2)[1:-1]):                      # the plain means, whatever the taper
        graphs, _ = C.dynamic_graphs_from_timeseries(GraphArena(DEV), ts, 30, [0, 1, 0], window, stride, taper=w)
        assert len(graphs) == len(where)
        for k, g in enumerate(graphs):
            assert g.node_features.dtype == torch.float32 and bits_eq(g.node_features.numpy(), want32[k])
    # the float64 z-scores of the same window means
    x, t_off, S, _ = C._as_timeseries(ts, torch.device(DEV))
    w_beg, _, _ = C._plan_windows(t_off.cpu().numpy(), window, stride)
    mean = C._dyn_means(x, torch.from_numpy(w_beg).to(DEV), window, n)
    assert bits_eq(C._ts_zscores(mean, len(where), n, torch.float64).cpu().numpy(), want64)
    sx, st, sS, _ = C._as_timeseries(slices, torch.device(DEV))
    assert bits_eq(mean.cpu().numpy(), C._ts_means(sx, st, sS, n).cpu().numpy())


@pytest.mark.parametrize("tapered", [False, True])
def test_graphs_equal_those_of_the_materialised_fc(tapered, monkeypatch):
    from gnm import connectome as C
    from gnm.arena import GraphArena
    rng = np.random.default_rng(12)
    n, window, stride, sp = 90, 20, 7, 30
    ts = [series(rng, T, n, offset=500.0 * s) for s, T in enumerate((50, 20, 64))]
    labels = [0, 1, 1]
    w = np.hamming(window + 2)[1:-1] if tapered else None
    where = host_windows(ts, window, stride)
    fc = torch.cat(C.dynamic_connectivity_from_timeseries(ts, window, stride, taper=w))
    feats = C.mean_bold_features([ts[s][t0:t0 + window] for s, _, t0 in where])
    flat_labels = [labels[s] for s, _, _ in where]
    ref = C.graphs_from_connectivity(GraphArena(DEV), fc, sp, feats, flat_labels)
    graphs, windows = C.dynamic_graphs_from_timeseries(GraphArena(DEV), ts, sp, labels, window, stride, taper=w)
    assert windows.dtype == np.int64 and windows.tolist() == [list(v) for v in where]
    same_graphs(graphs, ref)
    assert any(g.edge_mat.shape[1] > 0 for g in graphs)
    for per_chunk in (1, 2, 3):
        monkeypatch.setattr(C, "DYNFC_WORK_BYTES", per_chunk * 8 * n * n)
        assert max(hi - lo for lo, hi in C._plan_chunks(len(where), n, C.DYNFC_WORK_BYTES)) == per_chunk
        g2, w2 = C.dynamic_graphs_from_timeseries(GraphArena(DEV), ts, sp, labels, window, stride, taper=w)
        assert np.array_equal(w2, windows)
        same_graphs(g2, ref)
    # array features: one [n, F] for every window, or [S, n, F] per subject
    shared = rng.standard_normal((n, 2)).astype(np.float32)
    per_subject = rng.standard_normal((3, n, 2)).astype(np.float32)
    g3, _ = C.dynamic_graphs_from_timeseries(GraphArena(DEV), ts, sp, labels, window, stride, taper=w,
                                             node_features=shared)
    g4, _ = C.dynamic_graphs_from_timeseries(GraphArena(DEV), ts, sp, labels, window, stride, taper=w,
                                             node_features=per_subject)
    for k, (s, _, _) in enumerate(where):
        assert bits_eq(g3[k].node_features.numpy(), shared) and bits_eq(g4[k].node_features.numpy(), per_subject[s])
        assert np.array_equal(g3[k].edge_mat.numpy(), ref[k].edge_mat.numpy())
        assert np.array_equal(g4[k].edge_mat.numpy(), ref[k].edge_mat.numpy())


def test_class_score_time_course():
    from gnm import connectome as C
    from gnm.arena import GraphArena
    from models.graphcnn import GIN_InfoMaxReg
    rng = np.random.default_rng(13)
    n, S, window, stride = 64, 2, 20, 7
    ts = np.stack([series(rng, 50, n, offset=1e4, scale=80.0) for _ in range(S)])       # starts 0 .. 28: 5 windows
    torch.manual_seed(0)
    model = GIN_InfoMaxReg(3, 2, 1, 32, 2, 0.0, True, "sum", "sum", torch.device(DEV)).to(DEV)
    model.eval()
    graphs, windows = C.dynamic_graphs_from_timeseries(model, ts, 30, [0, 1], window, stride)
    W = len(graphs) // S
    assert W == 5 and windows[:, 1].tolist() == list(range(5)) * 2
    fc = C.dynamic_connectivity_from_timeseries(ts, window, stride)
    feats = C.mean_bold_features([ts[s][t0:t0 + window] for s, _, t0 in windows.tolist()])
    ref = C.graphs_from_connectivity(GraphArena(DEV), fc.reshape(S * W, n, n), 30, feats,
                                     [g.label for g in graphs])
    same_graphs(graphs, ref)
    scores = model.predict(graphs)
    assert bits_eq(scores.cpu().numpy(), model.predict(ref).cpu().numpy())
    course = scores.reshape(S, W, -1)
    assert tuple(course.shape) == (S, W, 2) and torch.isfinite(course).all()
