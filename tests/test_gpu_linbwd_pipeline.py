"""The second Linear's fused backward (gnm_linear_bwd_fused with sZ == X: the lower BatchNorm's input is this Linear's
input, K = H = 64) through the C ABI, at the sizes where its cross-tile pipeline changes shape.  The launch is capped at
512 workgroups of 4 waves, so a wave owns a second 32-row tile only past 65,536 rows:

    N = 1, 31, 32, 33      one wave has one tile (partial or full), every other wave none: the peeled first tile sees an
                           empty descriptor and the combine still writes zeros
    N = 65,536             exactly one full tile per wave
    N = 65,536 + 33        two waves take a second tile, the last one partial (1 of 32 rows)
    N = 3 * 65,536 - 5     three tiles for most waves, a partial last tile: the loop's back edge in steady state

Inputs and the bound (1e-5, max-norm relative, against an fp64 numpy restatement) are those of
test_gpu_kernels.py::test_linear_backward_recomputing_its_output for this entry.  G, Z, X and dA are allocated one tile
longer than N, NaN past row N (and, with padded row strides, NaN in the padding columns): nothing past N may be read
into a sum or written."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 1e-5
K = H = 64
PAD = 32                    # rows past N: one tile

CASES = [
    # N, (ldg, ldz, ldx, lda)
    (1, (64, 64, 64, 64)),
    (31, (64, 64, 64, 64)),
    (32, (64, 64, 64, 64)),
    (33, (68, 72, 72, 68)),
    (65536, (64, 64, 64, 64)),
    (65536 + 33, (68, 72, 68, 72)),
    (3 * 65536 - 5, (64, 64, 64, 64)),
]


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _padded(a, ld):
    """a [N, C] -> device array [N + PAD, ld], NaN outside a; the test passes its base pointer and ld"""
    n, c = a.shape
    full = np.full((n + PAD, ld), np.nan, dtype=np.float32)
    full[:n, :c] = a
    return torch.from_numpy(full).to(DEV)


def _close(got, ref, what, N):
    assert np.isfinite(got).all(), (N, what, "not finite")
    err = np.abs(got - ref).max() / (np.abs(ref).max() + 1e-30)
    print("N=%d %s: max-norm relative error %.3g" % (N, what, err))
    assert err < TOL, (N, what, err)


@pytest.mark.parametrize("N,lds", CASES, ids=["N%d-ld%d.%d.%d.%d" % ((n,) + l) for n, l in CASES])
def test_second_linear_backward_pipeline(N, lds):
    from gnm._cabi import check, lib
    ldg, ldz, ldx, lda = lds
    rng = np.random.default_rng(N + 1)
    X = (rng.standard_normal((N, K)) * 1.5 + 0.3).astype(np.float32)
    W = (rng.standard_normal((H, K)) / 8).astype(np.float32)
    b = rng.standard_normal(H).astype(np.float32)
    G = rng.standard_normal((N, H)).astype(np.float32)
    sc, sh = rng.uniform(0.5, 1.5, K).astype(np.float32), rng.standard_normal(K).astype(np.float32)
    lmu, lrs = rng.standard_normal(K).astype(np.float32), rng.uniform(0.5, 1.5, K).astype(np.float32)
    mean, rstd, cA, m1, m2 = (rng.uniform(0.5, 1.5, H).astype(np.float32) for _ in range(5))
    # this Linear's stored output, as the forward leaves it: fp32 of relu(bn_lo(X)) W^T + b
    X64 = X.astype(np.float64)
    F64 = np.maximum(X64 * sc + sh, 0)
    Z = (F64 @ W.astype(np.float64).T + b).astype(np.float32)

    # fp64 reference
    dZ = cA.astype(np.float64) * (G - m1 - (Z.astype(np.float64) - mean) * rstd * m2)
    dA_ref = (dZ @ W.astype(np.float64)) * ((X * sc + sh) > 0)
    dW_ref, db_ref = dZ.T @ F64, dZ.sum(0)
    s1_ref, s2_ref = dA_ref.sum(0), (dA_ref * ((X64 - lmu) * lrs)).sum(0)

    Gd, Zd, Xd = _padded(G, ldg), _padded(Z, ldz), _padded(X, ldx)
    Wd, scd, shd, lmud, lrsd = (torch.from_numpy(v).to(DEV) for v in (W, sc, sh, lmu, lrs))
    vec = [torch.from_numpy(v).to(DEV) for v in (mean, rstd, cA, m1, m2)]
    grid = lib.gnm_linear_bwd_grid(N)

    def launch():
        dA = torch.full((N + PAD, lda), float("nan"), device=DEV)
        dW = torch.full((H, K), float("nan"), device=DEV)
        db = torch.full((H,), float("nan"), device=DEV)
        ws = torch.full((int(lib.gnm_linear_bwd_workspace_floats(N, H, K)),), float("nan"), device=DEV)
        part = torch.full((grid, 2, K), float("nan"), dtype=torch.float64, device=DEV)
        check(lib.gnm_linear_bwd_fused(
            Gd.data_ptr(), ldg, Zd.data_ptr(), ldz, *[v.data_ptr() for v in vec],
            Xd.data_ptr(), ldx, scd.data_ptr(), shd.data_ptr(), 1, Wd.data_ptr(), K,
            dA.data_ptr(), lda, dW.data_ptr(), K, db.data_ptr(), ws.data_ptr(), N, K, H,
            Xd.data_ptr(), ldx, scd.data_ptr(), shd.data_ptr(), lmud.data_ptr(), lrsd.data_ptr(), part.data_ptr(),
            _stream()), "fused")
        torch.cuda.synchronize()
        return [a.cpu().numpy() for a in (dA, dW, db, part, ws)]

    dA, dW, db, part, ws = first = launch()

    # rows past N and the padding columns of dA are untouched
    assert np.isnan(dA[N:]).all(), (N, "dA written past row N")
    assert np.isnan(dA[:N, K:]).all(), (N, "dA written past column K")
    # every workgroup wrote its partial rows (zeros where its waves had no tile), and no sum saw a NaN
    assert np.isfinite(part).all() and np.isfinite(ws).all(), (N, "a partial row is missing or not finite")
    _close(dA[:N, :K], dA_ref, "dA", N)
    _close(dW, dW_ref, "dW", N)
    _close(db, db_ref, "db", N)
    ps = part.sum(0)
    _close(ps[0], s1_ref, "sum g", N)
    _close(ps[1], s2_ref, "sum g xhat", N)

    # two launches on the same inputs: the same bits everywhere (NaN padding included)
    for name, a, c in zip(("dA", "dW", "db", "s_partial", "workspace"), first, launch()):
        assert a.tobytes() == c.tobytes(), (N, name, "differs between two launches")
