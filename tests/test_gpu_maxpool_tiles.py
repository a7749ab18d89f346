"""The tiled max-pool kernels of csrc/maxpool.hip (gnm_maxpool_tile_fwd_kernel / gnm_maxpool_tile_bwd_kernel, one workgroup
per graph with its rows in LDS) and the two-stage column minimum, past the states tests/test_gpu_maxpool.py reaches: id
lists longer than the kMaxTileAhead * LPR prefetched ids, several passes with a partly empty last wave, waves that mix
rows without candidates with long rows, the unrolled staging loop, both sides of the two LDS limits per F, and the
column minimum past one block, past the final kernel's unrolled walk and past 64 columns.  The tables and what they
reach are tests/maxpool_cases.py; the CPU half (tests/test_maxpool_tiles_host.py) holds them to the source.

Everything is compared bit for bit (selection is index work): the untiled kernels against the oracle's numpy
restatement (oracle/gin_oracle.py maxpool_fwd / maxpool_bwd), the tiled kernels against the untiled ones.  A NaN equals
a NaN, whatever its payload; every other value must have the same bits, the sign of a zero included."""
import functools

import numpy as np
import pytest
import torch

import maxpool_cases as M

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
IDS = [M.case_id(c) for c in M.TILE_CASES]
AMAX_NULL = {64: M.TileCase(64, (65, 1, 2, 129, 64, 400, 3), "out", "coarse"),
             32: M.TileCase(32, (129, 1, 2, 257, 128, 400, 9), "out", "coarse")}        # run once more without amax


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _ptr(t):
    return t.data_ptr() if t is not None else None


def _strided(a, ld, fill=float("nan")):
    """`a` on the device in rows of `ld` elements, the padding columns holding `fill`"""
    a = torch.as_tensor(a)
    t = torch.full((a.shape[0], ld), fill, dtype=a.dtype, device=DEV)
    t[:, :a.shape[1]] = a.to(DEV)
    return t


def _same(a, b):
    """bitwise equal, a NaN equal to any NaN"""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype.kind != "f":
        return bool(np.array_equal(a, b))
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a[~na].view(np.uint32), b[~nb].view(np.uint32)))


def _np(t):
    return t.detach().cpu().numpy()


@functools.lru_cache(maxsize=2)
def _expected(case, learn_eps):
    """(graphs, h, pooled [+ (1 + eps) h], the oracle's cache) of one case, built once"""
    from oracle import gin_oracle as O
    graphs = M.case_graphs(case)
    h = M.case_features(case, graphs)
    want, cache = O.maxpool_fwd(h, O.build_padded_neighbors(graphs, learn_eps))
    if learn_eps:
        with np.errstate(invalid="ignore"):
            want = want + (np.float32(1) + np.float32(M.EPS)) * h          # fp32, op by op (graphcnn.py:161)
    return graphs, h, want, cache


class _Run:
    """the device arrays of one (case, eps form): neighbour lists, features, the column minimum where rows are padded"""

    def __init__(self, graphs, h, learn_eps):
        from gnm._cabi import check, lib
        from gnm.maxnb import MaxNeighbours
        self.mb = MaxNeighbours(graphs, not learn_eps, DEV)
        self.N, self.F = h.shape
        self.sizes = [g.num_nodes for g in graphs]
        self.B, self.n_max = len(self.sizes), max(self.sizes)
        self.node_off = torch.tensor(M.node_offsets(graphs), dtype=torch.int32, device=DEV)
        self.ldh, self.ldo = self.F + 8, self.F + 4
        self.hd = _strided(h, self.ldh)
        self.eps = torch.tensor([M.EPS], dtype=torch.float32, device=DEV) if learn_eps else None
        self.dummy = self.amin = None
        if self.mb.need_dummy:
            nblk = lib.gnm_maxpool_colmin_blocks(self.N)
            wv = torch.empty(nblk, self.F, device=DEV)
            wi = torch.empty(nblk, self.F, dtype=torch.int32, device=DEV)
            self.dummy = torch.empty(self.F, device=DEV)
            self.amin = torch.empty(self.F, dtype=torch.int32, device=DEV)
            check(lib.gnm_maxpool_colmin(self.hd.data_ptr(), self.ldh, self.N, self.F, wv.data_ptr(), wi.data_ptr(),
                                         self.dummy.data_ptr(), self.amin.data_ptr(), _stream()), "colmin")

    def new_out(self, ld=None):
        return (torch.full((self.N, ld or self.ldo), float("inf"), device=DEV),
                torch.full((self.N, self.F), -7, dtype=torch.int32, device=DEV))

    def fwd(self, out, amax):
        from gnm._cabi import lib
        mb = self.mb
        return lib.gnm_maxpool_fwd(self.hd.data_ptr(), self.ldh, mb.nb_off.data_ptr(), mb.nb_col.data_ptr(), self.N, self.F,
                                   mb.max_deg, int(mb.self_last), _ptr(self.eps), _ptr(self.dummy), out.data_ptr(),
                                   out.stride(0), _ptr(amax), _stream())

    def fwd_tiled(self, out, amax, h_ptr=None, ldh=None, F=None, n_max=None, ldo=None):
        from gnm._cabi import lib
        mb = self.mb
        return lib.gnm_maxpool_fwd_tiled(h_ptr or self.hd.data_ptr(), ldh or self.ldh, mb.nb_off.data_ptr(),
                                         mb.nb_col.data_ptr(), self.node_off.data_ptr(), self.B, n_max or self.n_max,
                                         F or self.F, mb.max_deg, int(mb.self_last), _ptr(self.eps), _ptr(self.dummy),
                                         out.data_ptr(), ldo or out.stride(0), _ptr(amax), _stream())

    def bwd(self, gd, amax, eps, dh):
        from gnm._cabi import lib
        mb = self.mb
        return lib.gnm_maxpool_bwd(gd.data_ptr(), gd.stride(0), amax.data_ptr(), mb.t_off.data_ptr(), mb.t_col.data_ptr(),
                                   self.N, self.F, _ptr(eps), _ptr(mb.iso_rows) if mb.n_iso else None, mb.n_iso,
                                   _ptr(self.amin), dh.data_ptr(), dh.stride(0), _stream())

    def bwd_tiled(self, gd, amax, eps, dh, g_ptr=None, ldg=None, F=None, n_max=None, amax_ptr=None):
        from gnm._cabi import lib
        mb = self.mb
        return lib.gnm_maxpool_bwd_tiled(g_ptr or gd.data_ptr(), ldg or gd.stride(0), amax_ptr or amax.data_ptr(),
                                         mb.t_off.data_ptr(), mb.t_col.data_ptr(), self.node_off.data_ptr(), self.B,
                                         n_max or self.n_max, F or self.F, _ptr(eps),
                                         _ptr(mb.iso_rows) if mb.n_iso else None, mb.n_iso, _ptr(self.amin), dh.data_ptr(),
                                         dh.stride(0), _stream())


def _untouched(out, amax=None):
    return bool(torch.isinf(out).all()) and (amax is None or bool((amax == -7).all()))


def _check_forward(case, learn_eps, run, h, want, cache):
    """a. the column minimum and the untiled forward against the oracle; the tiled forward runs exactly when its tile
    fits the LDS and then gives the untiled kernel's bits.  Returns the amax the backward is to use: the tiled
    forward's where it ran."""
    F = run.F
    assert run.mb.need_dummy == (case.kind != "regular")                    # "regular": nothing padded, dummy is NULL
    out_u, amax_u = run.new_out()
    assert run.fwd(out_u, amax_u) == 0
    assert _same(_np(out_u[:, :F]), want) and bool(torch.isinf(out_u[:, F:]).all())
    assert np.array_equal(_np(amax_u), cache["src"])                        # which candidate won, ties and NaN included
    if run.mb.need_dummy:
        assert np.array_equal(_np(run.amin), cache["amin"])
        assert _same(_np(run.dummy), h[cache["amin"], np.arange(F)])
    out_t, amax_t = run.new_out()
    rc = run.fwd_tiled(out_t, amax_t)
    fits = M.lds_fits(F, run.n_max, "fwd")
    assert rc == (0 if fits else -2), (rc, fits)
    if not fits:
        assert _untouched(out_t, amax_t)                                    # declined: nothing written
        return amax_u
    assert _same(_np(out_t[:, :F]), _np(out_u[:, :F])) and bool(torch.isinf(out_t[:, F:]).all())
    assert torch.equal(amax_t, amax_u)
    if case == AMAX_NULL[F]:
        out_n, _ = run.new_out()
        assert run.fwd_tiled(out_n, None) == 0
        assert _same(_np(out_n), _np(out_t))
    return amax_t


def _check_backward(case, learn_eps, run, h, cache, amax):
    """b. the untiled backward against the oracle on an integer gradient (exact in any order), the tiled backward
    bitwise against the untiled one on that and on a randn gradient (summation order and the fmaf must agree).

    The oracle comparison leaves out the columns of h that hold a NaN ("nan" cases only, at most F / 4 columns:
    tests/test_maxpool_tiles_host.py).  There the dummy (the column minimum, torch.min's first NaN) is a NaN, so in the
    reference a padded row WITH neighbours, none of them NaN, selects the dummy and its gradient continues to
    torch.min's row; the kernels route the dummy's gradient for rows without neighbours only (gnm_maxpool_bwd_dummy_kernel
    walks iso_rows).  The forward's values and selected rows are compared in those columns too, and so is the tiled
    backward against the untiled one."""
    from oracle import gin_oracle as O
    N, F = run.N, run.F
    rng = np.random.default_rng(5)
    g = rng.integers(-3, 4, (N, F)).astype(np.float32)
    want = O.maxpool_bwd(g.copy(), cache)
    eps1 = None
    if learn_eps:
        eps1 = torch.tensor([1.0], dtype=torch.float32, device=DEV)         # (1 + eps) = 2: still exact
        want = want + np.float32(2) * g
    gd = _strided(g, F + 4)
    ldd = F + 8

    def new_dh():
        return torch.full((N, ldd), float("nan"), device=DEV)

    dh_u = new_dh()
    assert run.bwd(gd, amax, eps1, dh_u) == 0
    got = _np(dh_u[:, :F])
    assert not np.isnan(got).any() and bool(torch.isnan(dh_u[:, F:]).all())   # every element written, no padding touched
    cols = ~np.isnan(h).any(0)
    assert cols.all() or case.feat == "nan"
    assert _same(got[:, cols], want[:, cols])
    fits = M.lds_fits(F, run.n_max, "bwd")
    dh_t = new_dh()
    rc = run.bwd_tiled(gd, amax, eps1, dh_t)
    assert rc == (0 if fits else -2), (rc, fits)
    if not fits:
        assert bool(torch.isnan(dh_t).all())                                # declined: nothing written
        return
    assert _same(_np(dh_t[:, :F]), got) and bool(torch.isnan(dh_t[:, F:]).all())
    gen = torch.Generator().manual_seed(11)
    gr = _strided(torch.randn(N, F, generator=gen), F + 4)
    eps2 = torch.tensor([0.25], dtype=torch.float32, device=DEV) if learn_eps else None
    d1, d2 = new_dh(), new_dh()
    assert run.bwd(gr, amax, eps2, d1) == 0 and run.bwd_tiled(gr, amax, eps2, d2) == 0
    assert not bool(torch.isnan(d1[:, :F]).any()) and torch.equal(d1[:, :F].view(torch.int32), d2[:, :F].view(torch.int32))
    assert bool(torch.isnan(d2[:, F:]).all())


@pytest.mark.parametrize("learn_eps", [True, False], ids=["eps", "self"])
@pytest.mark.parametrize("case", M.TILE_CASES, ids=IDS)
def test_tiled_forward_and_backward_bit_exact(case, learn_eps):
    graphs, h, want, cache = _expected(case, learn_eps)
    run = _Run(graphs, h, learn_eps)
    amax = _check_forward(case, learn_eps, run, h, want, cache)
    _check_backward(case, learn_eps, run, h, cache, amax)


@pytest.mark.parametrize("F,n", [(64, 65), (32, 129)])
def test_tiled_declines(F, n):
    """c. what the tiled entries do not take returns -2 and writes nothing: rows that are not 16-byte aligned (a stride
    of F + 3, a base 4 bytes on), F = 48, and an n_max one past the LDS limit -- n_max at the limit runs"""
    case = M.TileCase(F, (n,), "out", "coarse")
    graphs, h, want, cache = _expected(case, True)
    run = _Run(graphs, h, True)
    N, wide = run.N, F + 20                                                 # rows of out / dh wide enough for F = 48
    out, amax = run.new_out(wide)
    assert run.fwd_tiled(out, amax) == 0
    spare = torch.zeros((N + 1) * (F + 8), device=DEV)                      # room for the shifted and the 48-wide views
    g = _strided(np.random.default_rng(2).integers(-3, 4, (N, F)).astype(np.float32), F + 4)
    dh = torch.full((N, wide), float("nan"), device=DEV)
    assert run.bwd_tiled(g, amax, None, dh) == 0
    for kw in (dict(ldh=F + 3), dict(h_ptr=spare.data_ptr() + 4), dict(F=48, ldh=48, h_ptr=spare.data_ptr()),
               dict(ldo=F + 3)):
        o2, a2 = run.new_out(wide)
        assert run.fwd_tiled(o2, a2, **kw) == -2 and _untouched(o2, a2), kw
    for kw in (dict(ldg=F + 3), dict(g_ptr=spare.data_ptr() + 4), dict(F=48, ldg=48, g_ptr=spare.data_ptr()),
               dict(amax_ptr=amax.data_ptr() + 4)):
        d2 = torch.full((N, wide), float("nan"), device=DEV)
        assert run.bwd_tiled(g, amax, None, d2, **kw) == -2 and bool(torch.isnan(d2).all()), kw
    lim_f, lim_b = M.lds_limit(F, "fwd"), M.lds_limit(F, "bwd")
    assert M.lds_fits(F, lim_f, "fwd") and not M.lds_fits(F, lim_f + 1, "fwd") and lim_b < lim_f
    o2, a2 = run.new_out(wide)
    assert run.fwd_tiled(o2, a2, n_max=lim_f + 1) == -2 and _untouched(o2, a2)
    assert run.fwd_tiled(o2, a2, n_max=lim_f) == 0
    assert torch.equal(o2.view(torch.int32), out.view(torch.int32)) and torch.equal(a2, amax)
    d2 = torch.full((N, wide), float("nan"), device=DEV)
    assert run.bwd_tiled(g, amax, None, d2, n_max=lim_b + 1) == -2 and bool(torch.isnan(d2).all())
    assert run.bwd_tiled(g, amax, None, d2, n_max=lim_b) == 0
    assert torch.equal(d2[:, :F].view(torch.int32), dh[:, :F].view(torch.int32))


@pytest.mark.parametrize("case", M.COLMIN_CASES, ids=["N%d-F%d-%s" % c for c in M.COLMIN_CASES])
def test_column_minimum_bit_exact(case):
    """d. gnm_maxpool_colmin (256 rows a block, then one workgroup per 64 columns over the partials) against np.argmin:
    the first NaN, else the smallest value, ties to the smaller row"""
    from gnm._cabi import lib
    h = M.colmin_input(case)
    N, F = h.shape
    amin = np.argmin(h, axis=0)
    hd = _strided(h, F + 3)
    nblk = lib.gnm_maxpool_colmin_blocks(N)
    assert nblk == M.colmin_blocks(N)
    wv, wi = torch.empty(nblk, F, device=DEV), torch.empty(nblk, F, dtype=torch.int32, device=DEV)
    vmin = torch.full((F + 2,), 7.0, device=DEV)
    got = torch.full((F + 2,), -7, dtype=torch.int32, device=DEV)
    assert lib.gnm_maxpool_colmin(hd.data_ptr(), F + 3, N, F, wv.data_ptr(), wi.data_ptr(), vmin.data_ptr(), got.data_ptr(),
                                  _stream()) == 0
    assert np.array_equal(_np(got[:F]), amin) and bool((got[F:] == -7).all())
    assert _same(_np(vmin[:F]), h[amin, np.arange(F)]) and bool((vmin[F:] == 7.0).all())


def _model_graph(H, n):
    from gnm.synth import SynthGraph
    rng = np.random.default_rng(1000 * H + n)
    i = np.arange(n)
    g = SynthGraph(n, np.stack([i, (i + 1) % n], 1), rng.standard_normal((n, 7)).astype(np.float32), 1)
    g.neighbors = M.out_lists(rng, H // 4, n)                               # what "max" pooling reads: the ladder
    g.max_neighbor = max(len(x) for x in g.neighbors)
    return g


def _train_step(model, graphs):
    model.train()
    model.zero_grad(set_to_none=True)
    np.random.seed(3)
    c, d = model(graphs)
    loss = c.float().square().sum() + d.float().square().mean()
    loss.backward()
    torch.cuda.synchronize()
    grads = {k: _np(p.grad).copy() for k, p in model.named_parameters() if p.grad is not None}
    return _np(c), _np(d), _np(loss), grads


@pytest.mark.parametrize("learn_eps", [True, False], ids=["eps", "self"])
@pytest.mark.parametrize("H,n", [(64, 417), (64, 500), (32, 900)])
def test_model_step_bitwise_equal_with_the_tiled_kernels_declined(H, n, learn_eps, monkeypatch):
    """e. one eager train step on a ladder graph: the logits, the loss and every gradient have the bits of the same step
    with both tiled entries declining, and the first step did take them where the tile fits the LDS ((64, 417): both
    directions; (64, 500) and (32, 900): the forward only)"""
    from gnm import core
    from models.graphcnn import GIN_InfoMaxReg
    torch.manual_seed(0)
    model = GIN_InfoMaxReg(3, 2, 7, H, 2, 0.0, learn_eps, "sum", "max", torch.device(DEV)).to(DEV)
    graphs = [_model_graph(H, n)]
    calls = {"fwd": [], "bwd": []}
    real_f, real_b = core.lib.gnm_maxpool_fwd_tiled, core.lib.gnm_maxpool_bwd_tiled

    def spy_f(*a):
        rc = real_f(*a)
        calls["fwd"].append((a[7], a[6], rc))                               # (F, n_max, rc)
        return rc

    def spy_b(*a):
        rc = real_b(*a)
        calls["bwd"].append((a[8], a[7], rc))
        return rc
    monkeypatch.setattr(core.lib, "gnm_maxpool_fwd_tiled", spy_f, raising=False)
    monkeypatch.setattr(core.lib, "gnm_maxpool_bwd_tiled", spy_b, raising=False)
    a = _train_step(model, graphs)
    for which in ("fwd", "bwd"):
        assert any(F == H for F, _, _ in calls[which]), calls
        for F, n_max, rc in calls[which]:
            assert n_max == n and rc == (0 if F in (32, 64) and M.lds_fits(F, n, which) else -2), (which, calls)
    assert all(rc == 0 for F, _, rc in calls["fwd"] if F == H)
    assert all(rc == (0 if n == 417 else -2) for F, _, rc in calls["bwd"] if F == H)
    declined = []
    monkeypatch.setattr(core.lib, "gnm_maxpool_fwd_tiled", lambda *x: declined.append("fwd") or -2, raising=False)
    monkeypatch.setattr(core.lib, "gnm_maxpool_bwd_tiled", lambda *x: declined.append("bwd") or -2, raising=False)
    b = _train_step(model, graphs)
    assert declined.count("fwd") == len(calls["fwd"]) and declined.count("bwd") == len(calls["bwd"])
    assert np.isfinite(a[0]).all() and np.isfinite(a[2]).all()
    for x, y in zip(a[:3], b[:3]):
        assert x.dtype == y.dtype and x.tobytes() == y.tobytes()
    assert a[3].keys() == b[3].keys() and len(a[3]) > 0
    for k in a[3]:
        assert a[3][k].tobytes() == b[3][k].tobytes(), k
