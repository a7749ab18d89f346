"""CPU checks of the kNN edge rule (gnm/connectome.py knn_edges, knn_adjacency and the knn= keyword of the builders;
csrc/connectome.hip gnm_connectome_knn_structure): the host oracle against an independent brute-force restatement, the
properties the rule promises, every argument check before anything touches a device, and the C-ABI declared, bound and
exported."""
import os
import re

import numpy as np
import pytest

from knn_cases import brute_adjacency, brute_edges, fc_stack, hand_made, oracle_adjacency

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["gnm_connectome_knn_scratch_words", "gnm_connectome_knn_structure"]
NS = [1, 2, 7, 65]


def ks(n):
    return sorted({k for k in (1, 2, 5, n - 1, n + 3) if k >= 1})


def test_symbols_declared_bound_and_exported():
    from gnm import _cabi
    header = open(os.path.join(ROOT, "include", "gnm_hip.h")).read()
    for name in SYMBOLS:
        assert re.search(r"\b%s\(" % name, header), name
        assert name in _cabi.SIGNATURES, name
        assert getattr(_cabi.lib, name) is not None


@pytest.mark.parametrize("kind", ["corr", "ties"])
@pytest.mark.parametrize("n", NS)
def test_knn_edges_equals_the_brute_force_restatement(n, kind):
    from gnm.connectome import knn_edges
    fc = fc_stack(2, n, 31 * n + (kind == "ties"), kind)
    for m in fc:
        for k in ks(n):
            for mutual in (False, True):
                for absolute in (False, True):
                    iu, ju = knn_edges(m, k, mutual, absolute)
                    bu, bj = brute_edges(m, k, mutual, absolute)
                    assert np.array_equal(iu, bu) and np.array_equal(ju, bj), (n, kind, k, mutual, absolute)
                    assert (iu < ju).all()


@pytest.mark.parametrize("n,k", [(65, 5), (129, 20)])
def test_knn_edges_on_the_hand_made_rows(n, k):
    for name, m in hand_made(n, k).items():
        for mutual in (False, True):
            for absolute in (False, True):
                assert np.array_equal(oracle_adjacency(m, k, mutual, absolute),
                                      brute_adjacency(m, k, mutual, absolute)), (name, mutual, absolute)
    # what the hand-made rows are there to show, stated by hand
    hm = hand_made(n, k)
    A = oracle_adjacency(hm["nan_row_and_column"], k)
    assert not A[12].any() and not A[:, 12].any()                      # isolated, not an error
    from gnm.connectome import knn_edges
    m = hm["signed_zeros"]
    sel = np.zeros(n, bool)
    iu, ju = knn_edges(np.where(np.arange(n)[:, None] == 2, m, np.nan), k)     # only row 2 selects
    sel[ju[iu == 2]] = True; sel[iu[ju == 2]] = True
    want = list(range(5, 5 + k - 2)) + [10 + k, 10 + k + 1]            # the first two zeros, whatever their sign
    assert np.flatnonzero(sel).tolist() == want
    m = hm["negative_strongest"]
    iu, ju = knn_edges(np.where(np.arange(n)[:, None] == n - 1, m, np.nan), k, absolute=True)
    assert sorted(iu[ju == n - 1].tolist()) == list(range(k))           # the k columns of -5


@pytest.mark.parametrize("kind", ["corr", "ties"])
@pytest.mark.parametrize("n", NS)
def test_properties(n, kind):
    from gnm.connectome import knn_edges
    m = fc_stack(1, n, 5 * n + 1, kind)[0]
    for k in ks(n):
        iu, ju = knn_edges(m, k)
        deg = np.bincount(np.concatenate([iu, ju]), minlength=n)
        assert (deg >= min(k, n - 1)).all()                          # NaN-free: every node has n - 1 candidates
        mu, mj = knn_edges(m, k, mutual=True)
        mdeg = np.bincount(np.concatenate([mu, mj]), minlength=n)
        assert (mdeg <= k).all()
        assert set(zip(mu.tolist(), mj.tolist())) <= set(zip(iu.tolist(), ju.tolist()))
        if k >= n - 1:
            for e in ((iu, ju), (mu, mj)):
                assert len(e[0]) == n * (n - 1) // 2                   # the complete graph
    # with NaNs: a node with >= k candidates still has degree >= k
    if n >= 7:
        h = m.copy()
        h[1, 2:] = np.nan
        h[3, :] = np.nan
        for k in (1, 2, 5):
            iu, ju = knn_edges(h, k)
            deg = np.bincount(np.concatenate([iu, ju]), minlength=n)
            cands = (~np.isnan(h)).sum(1) - (~np.isnan(np.diag(h)))
            assert (deg[cands >= k] >= k).all() and (deg >= np.minimum(cands, k)).all()


def test_arguments_are_checked_before_any_device():
    from gnm import connectome as C
    from gnm._cabi import GnmError
    from gnm.arena import GraphArena
    rng = np.random.default_rng(0)
    n = 6
    fc = fc_stack(2, n, 3)
    ts = rng.standard_normal((2, 12, n))
    feats = np.ones((n, 2), np.float32)
    calls = {
        "add_connectivity": lambda sp, **kw: GraphArena("cpu").add_connectivity(fc, sp, feats, **kw),
        "graphs_from_connectivity": lambda sp, **kw: C.graphs_from_connectivity(GraphArena("cpu"), fc, sp, feats, [0, 1],
                                                                                **kw),
        "graphs_from_timeseries": lambda sp, **kw: C.graphs_from_timeseries(GraphArena("cpu"), ts, sp, [0, 1], **kw),
        "dynamic_graphs_from_timeseries": lambda sp, **kw: C.dynamic_graphs_from_timeseries(GraphArena("cpu"), ts, sp,
                                                                                            [0, 1], 6, **kw),
    }
    for name, call in calls.items():
        with pytest.raises(ValueError, match="both"):
            call(30, knn=3)
        with pytest.raises(ValueError, match="neither"):
            call(None)
        for bad in (0, -1, 2.5, True, "3", np.float64(2.0)):
            with pytest.raises(ValueError, match="knn must be"):
                call(None, knn=bad)
        # with every argument right, the CPU is refused as a device, as it is for sparsity
        for kw in (dict(knn=3), dict(knn=np.int64(2), mutual=True, absolute=True)):
            with pytest.raises(GnmError):
                call(None, **kw)
        with pytest.raises(GnmError):
            call(30)
    for bad in (0, -1, 2.5, True):
        with pytest.raises(ValueError, match="knn must be"):
            C.knn_adjacency(fc, bad, device="cpu")
        with pytest.raises(ValueError, match="knn must be"):
            C.knn_edges(fc[0], bad)
    with pytest.raises(GnmError):
        C.knn_adjacency(fc, 2, device="cpu")
    with pytest.raises(ValueError):
        C.knn_adjacency(fc[0], 2, device="cpu")                         # [n, n] is not a stack
    with pytest.raises(ValueError):
        C.knn_edges(fc, 2)                                              # and a stack is not a matrix


def test_c_entries_check_arguments_before_launching():
    from gnm._cabi import lib
    nmax = lib.gnm_connectome_max_nodes()
    fake = 1 << 20                                   # never dereferenced: every call below returns before a launch
    knn, words = lib.gnm_connectome_knn_structure, lib.gnm_connectome_knn_scratch_words
    assert knn(fake, 1, 8, 0, 0, fake, fake, fake, fake, None) == -1             # k = 0
    assert knn(fake, 1, 8, -3, 0, fake, fake, fake, fake, None) == -1
    assert knn(fake, 1, 0, 2, 0, fake, fake, fake, fake, None) == -1
    assert knn(fake, -1, 8, 2, 0, fake, fake, fake, fake, None) == -1
    assert knn(fake, 1, 8, 2, 4, fake, fake, fake, fake, None) == -1             # an unknown flag
    assert knn(fake, 1, 8, 0, 0, fake, fake, fake, fake, None) == -1
    assert knn(fake, 0, 8, 0, 0, fake, fake, fake, fake, None) == -1             # a bad k even with nothing to do
    assert knn(fake, 1, nmax + 1, 2, 0, fake, fake, fake, fake, None) == -2
    for hole in range(5):                                                        # each pointer in turn
        p = [fake] * 5
        p[hole] = None
        assert knn(p[0], 1, 8, 2, 0, p[1], p[2], p[3], p[4], None) == -1
    assert knn(fake, 1, 8, 2, 0, fake, fake + 4, fake, fake, None) == -1         # work is 16-byte aligned
    assert knn(fake, 1, 8, 2, 0, fake + 2, fake, fake, fake, None) == -1         # sel holds 32-bit words
    assert knn(None, 0, 8, 2, 3, None, None, None, None, None) == 0              # S = 0: nothing to do
    assert words(3, 65) == 3 * 65 * 3 and words(1, 1) == 1 and words(0, 400) == 0
    assert words(2, nmax) == 2 * nmax * (nmax // 32)
    assert words(-1, 8) == -1 and words(1, 0) == -1 and words(1, nmax + 1) == -1
