"""CPU checks of the time-series path (gnm/connectome.py connectivity_from_timeseries, mean_bold_features,
graphs_from_timeseries; csrc/timeseries.hip): argument checks before anything is launched, the ragged packing, the
C-ABI declared and exported, and the summation order the device uses, restated on the host, against the reference
loader's mean_bold goldens (tests/golden/timeseries, made by make_timeseries_goldens.py)."""
import os
import re

import numpy as np
import pytest
import torch

import timeseries_goldens

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["gnm_timeseries_max_nodes", "gnm_timeseries_means", "gnm_timeseries_zscores", "gnm_timeseries_gram",
           "gnm_timeseries_normalize"]


def test_symbols_declared_bound_and_exported():
    from gnm import _cabi
    header = open(os.path.join(ROOT, "include", "gnm_hip.h")).read()
    for name in SYMBOLS:
        assert re.search(r"\b%s\(" % name, header), name
        assert name in _cabi.SIGNATURES, name
        assert getattr(_cabi.lib, name) is not None
    assert _cabi.lib.gnm_timeseries_max_nodes() == _cabi.lib.gnm_connectome_max_nodes() == 4096


def test_c_entries_check_arguments_before_launching():
    from gnm._cabi import lib
    nmax = lib.gnm_timeseries_max_nodes()
    fake = 1 << 20                                   # never dereferenced: every call below returns before a launch
    assert lib.gnm_timeseries_means(fake, 1, fake, 1, 0, fake, None) == -1
    assert lib.gnm_timeseries_means(fake, 1, fake, -1, 4, fake, None) == -1
    assert lib.gnm_timeseries_means(fake, 1, fake, 1, nmax + 1, fake, None) == -2
    assert lib.gnm_timeseries_means(None, 1, fake, 1, 4, fake, None) == -1
    assert lib.gnm_timeseries_means(fake, 0, None, 1, 4, fake, None) == -1
    assert lib.gnm_timeseries_means(fake, 1, fake, 1, 4, None, None) == -1
    assert lib.gnm_timeseries_means(None, 1, None, 0, 4, None, None) == 0               # nothing to do
    assert lib.gnm_timeseries_zscores(fake, 1, 0, fake, fake, None) == -1
    assert lib.gnm_timeseries_zscores(fake, 1, nmax + 1, fake, fake, None) == -2
    assert lib.gnm_timeseries_zscores(fake, 1, 4, None, None, None) == -1
    assert lib.gnm_timeseries_zscores(None, 1, 4, fake, None, None) == -1
    assert lib.gnm_timeseries_zscores(None, 0, 4, None, None, None) == 0
    assert lib.gnm_timeseries_gram(fake, 1, fake, fake, 1, 0, fake, fake, None) == -1
    assert lib.gnm_timeseries_gram(fake, 1, fake, fake, 1, nmax + 1, fake, fake, None) == -2
    assert lib.gnm_timeseries_gram(fake, 1, fake, None, 1, 8, fake, fake, None) == -1
    assert lib.gnm_timeseries_gram(fake, 1, fake, fake, 1, 8, fake, None, None) == -1
    assert lib.gnm_timeseries_gram(None, 1, None, None, 0, 8, None, None, None) == 0
    assert lib.gnm_timeseries_normalize(fake, 1, 0, fake, None) == -1
    assert lib.gnm_timeseries_normalize(fake, 1, nmax + 1, fake, None) == -2
    assert lib.gnm_timeseries_normalize(None, 1, 8, fake, None) == -1
    assert lib.gnm_timeseries_normalize(None, 0, 8, None, None) == 0


def test_pack_timeseries():
    from gnm.connectome import pack_timeseries
    rng = np.random.default_rng(0)
    parts = [rng.standard_normal((T, 5)) for T in (3, 1, 7)]
    x, t_off = pack_timeseries(parts)
    assert t_off.dtype == np.int64 and t_off.tolist() == [0, 3, 4, 11]
    assert x.dtype == torch.float64 and tuple(x.shape) == (11, 5) and not x.is_cuda
    for s, p in enumerate(parts):
        assert np.array_equal(x[t_off[s]:t_off[s + 1]].numpy(), p)
    # float32 stays float32; a float64 among them widens all (exactly)
    f32 = [p.astype(np.float32) for p in parts]
    x32, _ = pack_timeseries(f32)
    assert x32.dtype == torch.float32 and np.array_equal(x32.numpy(), np.concatenate(f32))
    mixed, _ = pack_timeseries([f32[0], torch.from_numpy(parts[1]), f32[2]])
    assert mixed.dtype == torch.float64
    assert np.array_equal(mixed.numpy(), np.concatenate([f32[0].astype(np.float64), parts[1],
                                                         f32[2].astype(np.float64)]))


def test_arguments_are_checked():
    from gnm._cabi import GnmError
    from gnm.arena import GraphArena
    from gnm.connectome import connectivity_from_timeseries, graphs_from_timeseries, mean_bold_features
    ok = np.zeros((2, 5, 4))
    bad = [np.zeros((5, 4)), np.zeros((1, 2, 5, 4)), np.zeros((2, 5, 4), np.int64), np.zeros((2, 5, 4), np.float16),
           np.zeros((2, 0, 4)), np.zeros((2, 5, 0)), np.zeros((1, 2, 4097), np.float32), [],
           [np.zeros((5, 4)), np.zeros((5, 3))], [np.zeros((5, 4)), np.zeros((0, 4))], [np.zeros((2, 5, 4))],
           [np.zeros((5, 4), np.int32)]]
    for ts in bad:
        for dev in ("cpu", "cuda:0"):            # the shape is checked before the device
            with pytest.raises(ValueError):
                connectivity_from_timeseries(ts, device=dev)
            with pytest.raises(ValueError):
                mean_bold_features(ts, device=dev)
        with pytest.raises(ValueError):
            graphs_from_timeseries(GraphArena("cpu"), ts, 30, [0] * 2)
    with pytest.raises(GnmError):
        connectivity_from_timeseries(ok, device="cpu")
    with pytest.raises(GnmError):
        mean_bold_features([ok[0], ok[1][:3]], device="cpu")
    with pytest.raises(GnmError):
        graphs_from_timeseries(GraphArena("cpu"), ok, 30, [0, 1])
    with pytest.raises(ValueError):                # label count
        graphs_from_timeseries(GraphArena("cpu"), ok, 30, [0, 1, 0])
    with pytest.raises(ValueError):
        graphs_from_timeseries(GraphArena("cpu"), [ok[0]], 30, [0, 1])
    with pytest.raises(ValueError):                # sparsity, node_features, dtype
        graphs_from_timeseries(GraphArena("cpu"), ok, 101, [0, 1])
    with pytest.raises(ValueError):
        graphs_from_timeseries(GraphArena("cpu"), ok, 30, [0, 1], node_features="one_hot")
    with pytest.raises(ValueError):
        mean_bold_features(ok, device="cpu", dtype=torch.float16)


def test_goldens_present():
    assert len(timeseries_goldens.PATHS) >= 3
    sizes = [timeseries_goldens.load(p)["z64"].shape for p in timeseries_goldens.PATHS]
    assert any(n == 400 for _, n in sizes) and sum(S for S, _ in sizes) >= 5


def test_device_order_reproduces_the_reference_loader():
    """the summation order of the device's means and z-scores, restated on the host, gives the loader's mean_bold
    features bitwise (its pandas array is column-major, so np.mean sums each column pairwise)"""
    for path in timeseries_goldens.PATHS:
        d = timeseries_goldens.load(path)
        for s, x in enumerate(d["ts"]):
            z = timeseries_goldens.mean_bold_restated(x)
            assert z.tobytes() == d["z64"][s].tobytes(), (path, s)
            assert z.astype(np.float32).tobytes() == d["feat32"][s].tobytes(), (path, s)
            f = np.asfortranarray(x).mean(0)
            assert np.array_equal(f, np.array([timeseries_goldens.pairwise_sum(x[:, c]) for c in
                                               range(x.shape[1])]) / x.shape[0])
