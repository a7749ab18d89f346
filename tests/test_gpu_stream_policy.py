"""What a change of the streaming kernels' cache policy or store mapping can break and the parity tests do not look at
(csrc/gnm_common.h: kLoadOnce on the loads of arrays a launch reads once, kStoreStream on the 16-byte stores of the big
[N, 64] outputs; profiles/store_policy_ab.md has what each measured).  Every entry point is held to its fp64 reference
by test_gpu_kernels.py; here

  1. a producer -> consumer chain re-run in the SAME buffers on other inputs must never see bytes of an earlier pass;
  2. the dW / db partial rows of the fused Linear backwards: every element of every row that exists is written, nothing
     past the last row, the same bits on every run, and the sums are right (the narrow input layer's form included);
  3. no store site touches the padding of an output whose leading dimension is wider than its rows.

Tolerance: 1e-5 relative (max-norm), the one test_gpu_kernels.py holds every fp32 kernel to."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 1e-5


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _t(a, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a).astype(dtype))).to(DEV)


def _bits(a):
    """the tensor's bytes (NaN-safe, sign-of-zero-exact comparison)"""
    a = a.contiguous()
    return a.view(torch.int64 if a.element_size() == 8 else torch.int32)


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


def _close(got, ref, what):
    got = got.double().cpu().numpy() if torch.is_tensor(got) else got
    err = np.abs(got - ref).max() / (np.abs(ref).max() + 1e-30)
    assert err < TOL, (what, err)


# ------------------------------------------------------------------------------------------------------------------
# 1. fresh bytes through a producer -> consumer chain
# ------------------------------------------------------------------------------------------------------------------
class _Chain:
    """One MLP of the model, forward and backward, through the C ABI, on one stream, in buffers it keeps:
    Z1 = X W1^T + b1 (+ BatchNorm statistics) -> bn_finalize -> Z2 = relu(bn(Z1)) W2^T + b2 -> backward of the second
    Linear (the stored-Z pass with the lower BatchNorm's sums) -> backward of the first (the pass that recomputes Z1) ->
    the deferred dW / db reduction of both."""
    K = H = 64

    def __init__(self, N, rng):
        from gnm._cabi import lib
        self.N, H = N, self.H
        f = lambda *s: torch.full(s, float("nan"), device=DEV)
        self.W1, self.W2 = _t(rng.standard_normal((H, H)) / 8), _t(rng.standard_normal((H, H)) / 8)
        self.b1, self.b2 = _t(rng.standard_normal(H)), _t(rng.standard_normal(H))
        self.gamma, self.beta = _t(rng.uniform(0.5, 1.5, H)), _t(rng.standard_normal(H) * 0.3)
        self.rm, self.rv = torch.zeros(H, device=DEV), torch.ones(H, device=DEV)
        self.nbt = torch.zeros(1, dtype=torch.int64, device=DEV)
        self.vec2 = [_t(rng.uniform(0.5, 1.5, H)) for _ in range(5)]      # mean, rstd, cA, m1, m2 of the upper BatchNorm
        self.lgrid, self.bgrid = lib.gnm_linear_grid(N), lib.gnm_linear_bwd_grid(N)
        self.stats = torch.full((self.lgrid, 2, H), float("nan"), dtype=torch.float64, device=DEV)
        self.scale, self.shift, self.mean, self.rstd = f(H), f(H), f(H), f(H)
        self.Z1, self.Z2, self.dA2, self.dA1 = f(N, H), f(N, H), f(N, H), f(N, H)
        self.part = torch.full((self.bgrid, 2, H), float("nan"), dtype=torch.float64, device=DEV)
        nws = int(lib.gnm_linear_bwd_workspace_floats(N, H, H))
        self.ws1, self.ws2 = f(nws), f(nws)
        self.dW1, self.dW2, self.db1, self.db2 = f(H, H), f(H, H), f(H), f(H)
        self.zeros = torch.zeros(H, device=DEV)

    def run(self, X, G):
        from gnm._cabi import check, lib
        N, H, s = self.N, self.H, _stream()
        p = lambda a: a.data_ptr()
        check(lib.gnm_linear_fwd(p(X), H, p(self.W1), H, 0, p(self.b1), p(self.Z1), H, N, H, H, None, None, 0,
                                 p(self.stats), s), "linear_fwd + statistics")
        check(lib.gnm_bn_finalize(p(self.stats), self.lgrid, H, N, p(self.gamma), p(self.beta), p(self.rm), p(self.rv),
                                  p(self.nbt), 0.1, 1e-5, 1, 0, p(self.scale), p(self.shift), p(self.mean), p(self.rstd), s),
              "bn_finalize")
        check(lib.gnm_linear_fwd(p(self.Z1), H, p(self.W2), H, 0, p(self.b2), p(self.Z2), H, N, H, H, p(self.scale),
                                 p(self.shift), 1, None, s), "linear_fwd + prologue")
        check(lib.gnm_linear_bwd_fused(p(G), H, p(self.Z2), H, *[p(v) for v in self.vec2], p(self.Z1), H, p(self.scale),
                                       p(self.shift), 1, p(self.W2), H, p(self.dA2), H, None, H, p(self.db2), p(self.ws2),
                                       N, H, H, p(self.Z1), H, p(self.scale), p(self.shift), p(self.mean), p(self.rstd),
                                       p(self.part), s), "linear_bwd_fused (stored Z, statistics)")
        # (the lower BatchNorm's coefficient vectors stand in as they are: any fixed values serve this test)
        check(lib.gnm_linear_bwd_fused_rz(p(self.dA2), H, p(self.b1), p(self.mean), p(self.rstd), p(self.scale), p(self.zeros),
                                          p(self.zeros), p(X), H, None, None, 0, p(self.W1), H, p(self.dA1), H, None, H,
                                          p(self.db1), p(self.ws1), N, H, H, None, 0, None, None, None, None, None, s),
              "linear_bwd_fused_rz")
        check(lib.gnm_reduce_partials_multi(
            (C.c_void_p * 2)(p(self.ws2), p(self.ws1)), (C.c_void_p * 2)(p(self.dW2), p(self.dW1)), (C.c_int * 2)(H, H),
            (C.c_void_p * 2)(p(self.db2), p(self.db1)), (C.c_int * 2)(H, H), (C.c_int * 2)(H, H), 2, N, s), "reduce_multi")
        return {k: getattr(self, k).clone() for k in ("Z1", "stats", "scale", "shift", "mean", "rstd", "Z2", "dA2", "part",
                                                       "dA1", "ws1", "ws2", "dW1", "db1", "dW2", "db2")}


def test_chain_rerun_in_the_same_buffers_sees_fresh_bytes():
    N, H = 33 * 32 + 1, 64
    rng = np.random.default_rng(11)
    XA, XB = _t(rng.standard_normal((N, H)) * 1.5 + 0.3), _t(rng.standard_normal((N, H)) * 0.7 - 0.2)
    GA, GB = _t(rng.standard_normal((N, H))), _t(rng.standard_normal((N, H)) * 2)
    params = np.random.default_rng(12)
    chain = _Chain(N, params)
    a1 = chain.run(XA, GA)
    b = chain.run(XB, GB)
    a3 = chain.run(XA, GA)
    fresh = _Chain(N, np.random.default_rng(12)).run(XB, GB)
    torch.cuda.synchronize()
    for k in a1:
        assert torch.isfinite(a1[k]).all() and torch.isfinite(b[k]).all(), k
        assert _same_bits(a1[k], a3[k]), "third pass (input A) differs from the first in " + k
        assert _same_bits(b[k], fresh[k]), "input B in reused buffers differs from fresh buffers in " + k
    for k in ("Z1", "Z2", "dA2", "dA1", "dW1", "dW2"):      # (and the two inputs do give different results)
        assert not _same_bits(a1[k], b[k]), k


# ------------------------------------------------------------------------------------------------------------------
# 2. the partial rows of the fused Linear backwards
# ------------------------------------------------------------------------------------------------------------------
def _bwd_case(kind, N, K, H, seed):
    """One fused Linear backward with its reduction deferred, twice, in a NaN-filled workspace one partial row longer
    than needed; returns nothing, asserts everything.  kind: 'pipe' (stored Z, no lower BatchNorm), 'sz' (stored Z, the
    lower BatchNorm is the prologue), 'rz' (Z recomputed), and for K = 7 'narrow' (stored Z) / 'rz' (recomputed)."""
    from gnm._cabi import check, lib
    rng = np.random.default_rng(seed)
    X = (rng.standard_normal((N, K)) * 1.5 + 0.3).astype(np.float32)
    W = (rng.standard_normal((H, K)) / np.sqrt(K)).astype(np.float32)
    b = rng.standard_normal(H).astype(np.float32)
    G = rng.standard_normal((N, H)).astype(np.float32)
    sc, sh = rng.uniform(0.5, 1.5, K).astype(np.float32), rng.standard_normal(K).astype(np.float32)
    lmu, lrs = rng.standard_normal(K).astype(np.float32), rng.uniform(0.5, 1.5, K).astype(np.float32)
    mean, rstd, cA, m1, m2 = (rng.uniform(0.5, 1.5, H).astype(np.float32) for _ in range(5))
    pro = kind == "sz"
    X64 = X.astype(np.float64)
    F64 = np.maximum(X64 * sc + sh, 0) if pro else X64
    if kind == "rz":
        Z64 = F64 @ W.astype(np.float64).T + b
        Z = None
    else:
        Z = rng.standard_normal((N, H)).astype(np.float32)
        Z64 = Z.astype(np.float64)
    dZ = cA * (G - m1 - (Z64 - mean) * rstd * m2)
    Xd, Wd, bd, Gd, scd, shd, lmud, lrsd = map(_t, (X, W, b, G, sc, sh, lmu, lrs))
    vec = [_t(v) for v in (mean, rstd, cA, m1, m2)]
    Zd = _t(Z) if Z is not None else None
    grid = lib.gnm_linear_bwd_grid(N)
    pstride = H * K + H
    assert int(lib.gnm_linear_bwd_workspace_floats(N, H, K)) == grid * pstride
    p = lambda a: a.data_ptr()
    runs = []
    for _ in range(2):
        ws = torch.full(((grid + 1) * pstride,), float("nan"), device=DEV)
        dA = torch.empty(N, K, device=DEV)
        part = torch.empty(grid, 2, K, dtype=torch.float64, device=DEV)
        lo = (p(Xd), K, p(scd), p(shd), p(lmud), p(lrsd), p(part)) if pro else (None, 0, None, None, None, None, None)
        tail = (p(Xd), K) + ((p(scd), p(shd), 1) if pro else (None, None, 0)) + \
            (p(Wd), K, p(dA), K, None, K, None, p(ws), N, K, H) + lo + (_stream(),)
        if kind == "rz":
            check(lib.gnm_linear_bwd_fused_rz(p(Gd), H, p(bd), *[p(v) for v in vec], *tail), "rz")
        else:
            check(lib.gnm_linear_bwd_fused(p(Gd), H, p(Zd), H, *[p(v) for v in vec], *tail), kind)
        assert torch.isnan(ws[grid * pstride:]).all(), (kind, N, K, "the row past the last partial row was written")
        assert torch.isfinite(ws[:grid * pstride]).all(), (kind, N, K, "an element of a partial row was not written")
        dW = torch.full((H, K), float("nan"), device=DEV)
        db = torch.full((H,), float("nan"), device=DEV)
        check(lib.gnm_reduce_partials_multi((C.c_void_p * 1)(p(ws)), (C.c_void_p * 1)(p(dW)), (C.c_int * 1)(K),
                                            (C.c_void_p * 1)(p(db)), (C.c_int * 1)(H), (C.c_int * 1)(K), 1, N, _stream()),
              "reduce_multi")
        runs.append((ws, dW, db))
    _close(runs[0][1], dZ.T @ F64, (kind, N, K, "dW"))
    _close(runs[0][2], dZ.sum(0), (kind, N, K, "db"))
    for x, y in zip(runs[0], runs[1]):
        assert _same_bits(x, y), (kind, N, K, "two runs differ")


def _full_grid_rows():
    from gnm._cabi import lib
    g = lib.gnm_linear_bwd_grid(1 << 30)          # the grid's cap: N = 4 * 32 * grid(N) + 1 has grid(N) = the cap
    n = 4 * 32 * g + 1
    assert lib.gnm_linear_bwd_grid(n) == g
    return n


@pytest.mark.parametrize("N", [1, 31, 33, 33 * 32 + 1, "full grid + 1"])
def test_partial_rows_are_complete_bounded_and_repeatable(N):
    """(33 * 32 + 1 rows: an odd number of partial rows above one, so the two-row workgroups of the recomputing pass end
    on a row that does not exist)"""
    if isinstance(N, str):
        N = _full_grid_rows()
    for kind, K, H in [("pipe", 64, 64), ("sz", 64, 64), ("rz", 64, 64), ("pipe", 32, 64), ("pipe", 64, 32), ("pipe", 32, 32),
                       ("narrow", 7, 64), ("rz", 7, 64)]:
        _bwd_case(kind, N, K, H, seed=N % 1000 + K + H)


# ------------------------------------------------------------------------------------------------------------------
# 3. outputs with a padded leading dimension
# ------------------------------------------------------------------------------------------------------------------
SENT = -12345.5


def _padded(N, W):
    return torch.full((N, W + 4), SENT, device=DEV)


def _check_padded(out, W, ref, what):
    assert (out[:, W:] == SENT).all(), what + ": padding written"
    assert (out[:, :W] != SENT).all() and torch.isfinite(out[:, :W]).all(), what + ": an element was not written"
    if ref is not None:
        _close(out[:, :W], ref, what)


def test_padded_leading_dimension_is_left_alone():
    from gnm._cabi import check, lib
    N, H = 33, 64
    rng = np.random.default_rng(3)
    p = lambda a: a.data_ptr()
    s = _stream()
    W = (rng.standard_normal((H, H)) / 8).astype(np.float32)
    b = rng.standard_normal(H).astype(np.float32)
    X = rng.standard_normal((N, H)).astype(np.float32)
    sc, sh = rng.uniform(0.5, 1.5, H).astype(np.float32), rng.standard_normal(H).astype(np.float32)
    Wd, bd, Xd, scd, shd = map(_t, (W, b, X, sc, sh))
    # Linear forward, K = H = 64 (the split-precision kernel) and K = 7 (the input layer's)
    Z = _padded(N, H)
    check(lib.gnm_linear_fwd(p(Xd), H, p(Wd), H, 0, p(bd), p(Z), H + 4, N, H, H, None, None, 0, None, s), "linear_fwd")
    _check_padded(Z, H, X.astype(np.float64) @ W.astype(np.float64).T + b, "linear_fwd K = 64")
    X7 = rng.standard_normal((N, 7)).astype(np.float32)
    W7 = rng.standard_normal((H, 7)).astype(np.float32)
    X7d, W7d = _t(X7), _t(W7)
    Z7 = _padded(N, H)
    check(lib.gnm_linear_fwd(p(X7d), 7, p(W7d), 7, 0, p(bd), p(Z7), H + 4, N, 7, H, None, None, 0, None, s), "linear_fwd K = 7")
    _check_padded(Z7, H, X7.astype(np.float64) @ W7.astype(np.float64).T + b, "linear_fwd K = 7")
    # the three backwards' dX
    G = rng.standard_normal((N, H)).astype(np.float32)
    Zs = rng.standard_normal((N, H)).astype(np.float32)
    mean, rstd, cA, m1, m2 = (rng.uniform(0.5, 1.5, H).astype(np.float32) for _ in range(5))
    lmu, lrs = rng.standard_normal(H).astype(np.float32), rng.uniform(0.5, 1.5, H).astype(np.float32)
    Gd, Zsd, lmud, lrsd = map(_t, (G, Zs, lmu, lrs))
    vec = [_t(v) for v in (mean, rstd, cA, m1, m2)]
    ws = torch.empty(int(lib.gnm_linear_bwd_workspace_floats(N, H, H)), device=DEV)
    part = torch.empty(lib.gnm_linear_bwd_grid(N), 2, H, dtype=torch.float64, device=DEV)
    W64 = W.astype(np.float64)
    dz = lambda Z64: cA * (G - m1 - (Z64 - mean) * rstd * m2)
    none_lo = (None, 0, None, None, None, None, None)
    dA = _padded(N, H)
    check(lib.gnm_linear_bwd_fused(p(Gd), H, p(Zsd), H, *[p(v) for v in vec], p(Xd), H, None, None, 0, p(Wd), H, p(dA), H + 4,
                                   None, H, None, p(ws), N, H, H, *none_lo, s), "pipe")
    _check_padded(dA, H, dz(Zs.astype(np.float64)) @ W64, "dX, stored Z")
    dA = _padded(N, H)
    check(lib.gnm_linear_bwd_fused(p(Gd), H, p(Zsd), H, *[p(v) for v in vec], p(Xd), H, p(scd), p(shd), 1, p(Wd), H, p(dA),
                                   H + 4, None, H, None, p(ws), N, H, H, p(Xd), H, p(scd), p(shd), p(lmud), p(lrsd), p(part), s),
          "pipe_sz")
    # (masked entries are exact zeros, which differ from the sentinel)
    _check_padded(dA, H, (dz(Zs.astype(np.float64)) @ W64) * ((X * sc + sh) > 0), "dX, stored Z + statistics")
    dA = _padded(N, H)
    check(lib.gnm_linear_bwd_fused_rz(p(Gd), H, p(bd), *[p(v) for v in vec], p(Xd), H, None, None, 0, p(Wd), H, p(dA), H + 4,
                                      None, H, None, p(ws), N, H, H, *none_lo, s), "rz")
    _check_padded(dA, H, dz(X.astype(np.float64) @ W64.T + b) @ W64, "dX, recomputed Z")
    # G of gnm_bn_relu_bwd_stats (three graphs)
    node_off = _t([0, 10, 11, N], np.int32)
    B = 3
    dH = rng.standard_normal((N, H)).astype(np.float32)
    dHd = _t(dH)
    Gout = _padded(N, H)
    bpart = torch.empty(B, 2, H, dtype=torch.float64, device=DEV)
    check(lib.gnm_bn_relu_bwd_stats(p(dHd), H, None, 0, 0, None, None, 0, None, None, p(Zsd), H, p(scd), p(shd), p(lmud),
                                    p(lrsd), 1, p(Gout), H + 4, p(node_off), B, H, p(bpart), s), "bwd_stats")
    _check_padded(Gout, H, dH.astype(np.float64) * ((Zs * sc + sh) > 0), "G of bn_relu_bwd_stats")
    # gnm_gather_graph_rows: hidden-width rows (64) and the input layer's (7), with the second pair
    for width in (64, 7):
        src = rng.standard_normal((50, width)).astype(np.float32)
        src2 = rng.standard_normal((50, width)).astype(np.float32)
        base = np.array([30, 5, 12], np.int64)                     # where each graph's rows start in src
        srcd, src2d, based = _t(src), _t(src2), _t(base, np.int64)
        dst, dst2 = _padded(N, width), _padded(N, width)
        check(lib.gnm_gather_graph_rows(p(srcd), p(src2d), width, width, p(based), p(node_off), B, p(dst), p(dst2), width + 4, s),
              "gather_graph_rows")
        rows = np.concatenate([np.arange(30, 40), [5], np.arange(12, 12 + N - 11)])
        for o, sarr in ((dst, src), (dst2, src2)):
            assert (o[:, width:] == SENT).all(), "gather_graph_rows: padding written"
            assert torch.equal(o[:, :width].cpu(), torch.from_numpy(sarr[rows])), "gather_graph_rows width %d" % width
