"""CPU checks of GIN_InfoMaxReg.integrated_gradients(): the quadrature rules (gnm/intgrad.py), the contract restated
through the fp64 oracle (which the GPU tests and the golden generators share), the two identities csrc/intgrad.hip
relies on -- layer 0 is affine in alpha, and the sum over steps commutes with the final dX launch -- completeness of the
contract on the occlusion goldens' sources, the goldens of the real reference (tests/golden/intgrad/), the new C-ABI
entries, their kernels in the gfx950 code object, and argument validation -- everything that does not need a GPU."""
import glob
import os
import re

import numpy as np
import pytest
import torch

from helpers import GOLDEN_DIR, RTOL, rel_err
from test_occlusion_host import _cpu_model, load_occ_case, occ_graphs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("gnm_integrated_gradients", "gnm_integrated_gradients_scratch_floats", "gnm_intgrad_z0")
METHODS = ("midpoint", "trapezoid", "gausslegendre")
IG_CASES = sorted(os.path.basename(f)[:-4] for f in glob.glob(os.path.join(GOLDEN_DIR, "intgrad", "ig_*.npz")))
SOURCES = ("occ_gsum_nsum_eps0", "occ_gaverage_naverage_eps1", "occ_onehot_gsum_nsum_eps1",
           "occ_asym_gaverage_naverage_eps0")


def quadrature(method, steps):
    from gnm.intgrad import quadrature as q
    return q(method, steps)


# ---------------------------------------------------------------------------------------------- the contract, restated
def _oracle(state, args, dtype):
    from oracle import gin_oracle as O
    if isinstance(args, dict):
        args = (args["L"], args["m"], args["learn_eps"], args["gpool"], args["npool"])
    return O, O.OracleGIN(state, *args, dtype=dtype)


def _ograph(O, graph, feats):
    """`graph` with the features `feats` in their own precision (OGraph's constructor rounds them to fp32, which would
    move a quadrature point by an fp32 ulp)"""
    og = O.OGraph(len(graph.g), np.asarray(graph.edge_mat), feats)
    og.node_features = feats
    return og


def _arrays(graph, baseline, dtype):
    X = np.asarray(graph.node_features, dtype=np.float32).astype(dtype)
    x0 = np.zeros_like(X) if baseline is None else np.asarray(baseline, dtype=np.float32).astype(dtype)
    return X, x0


def oracle_ig(state, cfg_or_args, graph, classes, alphas, weights, baseline=None, dtype=np.float64):
    """(attr [len(classes), n, F0], base [len(classes)], base0 [len(classes)]) of the contract through
    oracle.gin_oracle.OracleGIN: the eval forward and its input gradient on an explicit copy of `graph` with the
    features x' + alpha_k (X - x') for every step (one forward per step serves all classes), the gradients summed with
    the weights in `dtype` and multiplied by X - x'; base / base0: the eval logits at X and at x'."""
    O, orc = _oracle(state, cfg_or_args, dtype)
    X, x0 = _arrays(graph, baseline, dtype)
    acc = np.zeros((len(classes),) + X.shape, dtype=dtype)

    def run(feats, want):
        with np.errstate(all="ignore"):
            score, _, cache = orc.forward([_ograph(O, graph, feats)], np.arange(1), training=False, want_disc=False)
        grads = []
        for c in (classes if want else ()):
            dC = np.zeros_like(score)
            dC[0, c] = 1
            grads.append(orc.backward(cache, dC, np.zeros((1, 1), dtype), want_dx=True)["__dX"])
        return score[0], grads

    for a, w in zip(np.asarray(alphas, dtype=dtype), np.asarray(weights, dtype=dtype)):
        _, grads = run(x0 + a * (X - x0), True)
        for ci, g in enumerate(grads):
            acc[ci] += w * g
    base, base0 = run(X, False)[0], run(x0, False)[0]
    return acc * (X - x0), base[list(classes)], base0[list(classes)]


def load_ig_case(name):
    """(cfg, state, source graphs, the golden's own arrays) of a tests/golden/intgrad case: the model and graphs are
    those of the occlusion golden it names"""
    d = dict(np.load(os.path.join(GOLDEN_DIR, "intgrad", name + ".npz")))
    cfg, state, src = load_occ_case(str(d["source"]))
    return cfg, state, occ_graphs(cfg, src), d


# ---------------------------------------------------------------------------------------------- quadrature
@pytest.mark.parametrize("method", METHODS)
def test_quadrature_weights_sum_to_one(method):
    import math
    for K in (1, 2, 3, 5, 8, 32, 64):
        if method == "trapezoid" and K < 2:
            continue
        a, w = quadrature(method, K)
        assert a.dtype == np.float64 and w.dtype == np.float64 and a.shape == (K,) and w.shape == (K,)
        assert abs(math.fsum(w) - 1.0) <= 1e-15, (method, K)
        assert (a >= 0).all() and (a <= 1).all() and (np.diff(a) > 0).all() and (w > 0).all()


def test_quadrature_closed_forms():
    for K in (1, 4, 7):
        a, w = quadrature("midpoint", K)
        assert np.array_equal(a, (np.arange(K) + 0.5) / K) and np.array_equal(w, np.full(K, 1.0 / K))
    a, w = quadrature("trapezoid", 5)
    assert np.array_equal(a, [0.0, 0.25, 0.5, 0.75, 1.0]) and np.array_equal(w, [0.125, 0.25, 0.25, 0.25, 0.125])
    a, w = quadrature("trapezoid", 2)
    assert np.array_equal(a, [0.0, 1.0]) and np.array_equal(w, [0.5, 0.5])
    a, w = quadrature("gausslegendre", 1)
    assert np.allclose(a, [0.5], atol=1e-16) and np.allclose(w, [1.0], atol=1e-16)
    a, w = quadrature("gausslegendre", 2)
    assert np.allclose(a, 0.5 + np.array([-0.5, 0.5]) / np.sqrt(3.0), atol=1e-15) and np.allclose(w, [0.5, 0.5], atol=1e-15)


def test_gauss_legendre_is_exact_to_degree_2k_minus_1():
    for K in range(1, 9):
        a, w = quadrature("gausslegendre", K)
        d = 2 * K - 1
        assert abs(float(np.sum(w * a ** d)) - 1.0 / (d + 1)) <= 1e-13, K
    a, w = quadrature("gausslegendre", 3)                       # and no further: degree 2K is missed
    assert abs(float(np.sum(w * a ** 6)) - 1.0 / 7) > 1e-6


def test_quadrature_bad_arguments():
    for method, steps in (("midpoint", 0), ("midpoint", -3), ("trapezoid", 1), ("gausslegendre", 0), ("simpson", 4),
                          (None, 4), ("midpoint", 2.5), ("midpoint", True), ("midpoint", None)):
        with pytest.raises(ValueError):
            quadrature(method, steps)


# ---------------------------------------------------------------------------------------------- the two identities
def _source(name, g=0):
    cfg, state, d = load_occ_case(name)
    return cfg, {k: v.astype(np.float64) if v.dtype.kind == "f" else v for k, v in state.items()}, occ_graphs(cfg, d)[g]


def _baseline_of(cfg, seed=3):
    return (0.5 * np.random.default_rng(seed).standard_normal((cfg["n"], cfg["f0"]))).astype(np.float32)


def _step(orc, O, graph, feats, cls):
    """(cache, dX) of the eval forward and the class's input gradient on a copy of `graph` with features `feats`"""
    score, _, cache = orc.forward([_ograph(O, graph, feats)], np.arange(1), training=False, want_disc=False)
    dC = np.zeros_like(score)
    dC[0, cls] = 1
    return cache, orc.backward(cache, dC, np.zeros((1, 1)), want_dx=True)["__dX"]


@pytest.mark.parametrize("with_baseline", [False, True])
@pytest.mark.parametrize("source", SOURCES)
def test_layer0_is_affine_in_alpha(source, with_baseline):
    """the first Linear's output of layer 0 on the rescaled graph equals alpha P + (1 - alpha) Q + b, with
    P = pool(X) W0^T and Q = pool(x') W0^T of the source graph"""
    cfg, state, graph = _source(source)
    O, orc = _oracle(state, cfg, np.float64)
    X, x0 = _arrays(graph, _baseline_of(cfg) if with_baseline else None, np.float64)
    W0, b0 = orc._lin(0, 0)
    P = _step(orc, O, graph, X, 0)[0]["layers"][0]["pooled"] @ W0.T
    Q = _step(orc, O, graph, x0, 0)[0]["layers"][0]["pooled"] @ W0.T
    for a in quadrature("gausslegendre", 5)[0]:
        cache, _ = _step(orc, O, graph, x0 + a * (X - x0), 0)
        z0 = cache["layers"][0]["pooled"] @ W0.T + b0
        assert np.abs(z0 - (a * P + (1 - a) * Q + b0)).max() <= 1e-12 * max(1.0, np.abs(z0).max())


class _Recording(np.ndarray):
    """a weight that records what is multiplied onto it from the left: in OracleGIN.backward `dx @ W` is the only such
    product, and its left operand is the gradient at the Linear's output"""
    seen = None

    def __rmatmul__(self, left):
        type(self).seen = np.asarray(left)
        return np.asarray(left) @ np.asarray(self)


@pytest.mark.parametrize("source", SOURCES)
def test_sum_over_steps_commutes_with_the_dx_launch(source):
    """sum_k w_k dX_k equals the dX of sum_k w_k dZ0_k, ((A^T + (1 + eps0) I) (sum_k w_k dZ0_k) [/deg]) W0, with dZ0_k
    the gradient at the output of layer 0's first Linear on the k-th rescaled copy"""
    cfg, state, graph = _source(source)
    O, orc = _oracle(state, cfg, np.float64)
    X, x0 = _arrays(graph, _baseline_of(cfg), np.float64)
    name = "mlps.0.linear.weight" if cfg["m"] == 1 else "mlps.0.linears.0.weight"
    W0 = orc.p[name].copy()
    orc.p[name] = W0.view(_Recording)
    alphas, weights = quadrature("midpoint", 5)
    total, dbar = 0.0, 0.0
    for a, w in zip(alphas, weights):
        cache, dX = _step(orc, O, graph, x0 + a * (X - x0), 1)
        dz0 = _Recording.seen                                    # (layers run top down: layer 0's product is the last)
        assert dz0.shape == (cfg["n"], cfg["H"]) and np.abs(dz0).max() > 0
        total = total + w * dX
        dbar = dbar + w * dz0
    A, deg = cache["A"], cache["deg"]                            # (A holds the self loops when learn_eps is off)
    y = A.T @ (dbar / deg if orc.npool == "average" else dbar)
    if orc.learn_eps:
        y = y + (1 + orc.p["eps"][0]) * dbar
    assert np.abs(total - y @ W0).max() <= 1e-12 * max(1.0, np.abs(total).max())


# ---------------------------------------------------------------------------------------------- completeness
@pytest.mark.parametrize("source", SOURCES)
def test_completeness_residual_shrinks_with_the_steps(source):
    """sum attr -> score(X) - score(0) as the quadrature refines: the fp64 residual of the midpoint rule shrinks
    monotonically from K = 4 over 32 to 256.  (Measured on occ_gsum_nsum_eps0, graph 0, class 0: sums -2.0889, -2.0365,
    -2.0394 against F(X) - F(0) = -2.0388.)"""
    cfg, state, graph = _source(source)
    res = []
    for K in (4, 32, 256):
        attr, base, base0 = oracle_ig(state, cfg, graph, (0,), *quadrature("midpoint", K))
        res.append(abs(float(attr[0].sum() - (base[0] - base0[0]))))
    print("%s: |residual| at K = 4, 32, 256: %.3e %.3e %.3e" % (source, *res))
    assert res[0] > res[1] > res[2] and res[2] < res[0]


# ---------------------------------------------------------------------------------------------- the goldens
def test_intgrad_goldens_present():
    assert len(IG_CASES) == 11
    pools = set()
    for c in IG_CASES:
        cfg, _, _, d = load_ig_case(c)
        if re.match(r"ig_g(sum|average)_n", c):
            pools.add((cfg["gpool"], cfg["npool"], cfg["learn_eps"]))
            assert "baseline" not in d
    assert pools == {(g, n_, e) for g in ("sum", "average") for n_ in ("sum", "average") for e in (True, False)}
    for extra in ("ig_asym_", "ig_onehot_", "ig_baseline_"):
        assert any(c.startswith(extra) for c in IG_CASES), extra
    d = load_ig_case([c for c in IG_CASES if c.startswith("ig_baseline_")][0])[3]
    assert np.abs(d["baseline"]).max() > 0.1
    for f in glob.glob(os.path.join(GOLDEN_DIR, "intgrad", "ig_*.npz")):
        assert os.path.getsize(f) < 64 * 1024, f


@pytest.mark.parametrize("case", IG_CASES)
def test_oracle_reproduces_reference_goldens(case):
    """the contract through the fp64 oracle against the real reference's loop of compute_saliency on rescaled copies
    (fp32), and against the oracle attribution stored next to it"""
    cfg, state, graphs, d = load_ig_case(case)
    for K in (1, 5):
        alphas, weights = quadrature("midpoint", K)
        assert np.array_equal(alphas, d[f"alphas_{K}"]) and np.array_equal(weights, d[f"weights_{K}"])
        for g, graph in enumerate(graphs):
            attr = oracle_ig(state, cfg, graph, (0, 1), alphas, weights, d.get("baseline"))[0]
            assert rel_err(attr, d[f"ref_{K}_{g}"]) <= RTOL, (K, g)
            assert rel_err(attr, d[f"oracle_{K}_{g}"]) <= 1e-12, (K, g)


# ---------------------------------------------------------------------------------------------- the C ABI
def test_intgrad_entries_declared_bound_and_exported():
    from gnm import _cabi
    header = open(os.path.join(ROOT, "include", "gnm_hip.h")).read()
    declared = set(re.findall(r"\b(gnm_[a-z0-9_]+)\s*\(", header))
    for name in NEW:
        assert name in declared and name in _cabi.SIGNATURES
        assert getattr(_cabi.lib, name) is not None
    # gnm_saliency's scratch over the K N virtual rows and the reduced (S, R) pair
    assert _cabi.lib.gnm_integrated_gradients_scratch_floats(3200, 64, 32) == (4 * 32 + 2) * 3200 * 64
    assert (_cabi.lib.gnm_integrated_gradients_scratch_floats(3200, 64, 32)
            == _cabi.lib.gnm_saliency_scratch_floats(32 * 3200, 64) + 2 * 3200 * 64)
    # the documented default (8 graphs of 400 nodes, K = 32, H = 64, m = 2, L = 5) is one chunk of the driver
    from gnm import attribution
    assert 4 * attribution._intgrad_floats(3200, 64, 5, 2, 32) < attribution.INTGRAD_SCRATCH_BYTES
    assert attribution._intgrad_floats(3200, 64, 5, 2, 32) >= 2 * 5 * 32 * 3200 * 64        # the forward's z arrays count


def test_intgrad_kernels_in_the_code_object(tmp_path):
    from test_isa_hazards import disassemble
    asm = disassemble(tmp_path)
    for kernel in ("gnm_intgrad_z0_kernel", "gnm_intgrad_reduce_kernel", "gnm_intgrad_scale_kernel"):
        assert re.search(kernel, asm), kernel


def test_intgrad_bad_arguments_launch_nothing():
    """every check runs before a pointer is touched: the status with NULL arrays, gnm_saliency's codes in its order"""
    from gnm._cabi import lib

    def call(B=1, n_max=400, N=400, F0=7, H=64, L=5, m=2, Cn=2, cls=0, K=8, lda=7, ldx=7):
        return lib.gnm_integrated_gradients(None, None, None, None, None, B, n_max, N, F0, H, L, m, Cn, cls, 0, 0, 0, None,
                                            None, None, None, None, None, K, None, None, ldx, None, 0, 0, None, lda, None)

    def saliency(B=1, n_max=400, N=400, F0=7, H=64, L=5, m=2, Cn=2, cls=0, ldx=7):
        return lib.gnm_saliency(None, None, None, None, None, B, n_max, N, F0, H, L, m, Cn, cls, 0, 0, 0, None, None, None,
                                None, ldx, None)
    assert call(B=0) == 0                                      # nothing to do
    for kw in (dict(H=48), dict(H=256), dict(m=4), dict(m=0), dict(L=17), dict(L=0), dict(n_max=417), dict(n_max=0),
               dict(F0=0), dict(F0=100000), dict(cls=2), dict(cls=-1), dict(N=0), dict()):
        assert call(**kw) == saliency(**kw), kw
    assert call(H=48) == -2 and call(cls=2) == -1 and call() == -1
    assert call(K=0) == -1 and call(K=-1) == -1 and call(lda=6) == -1 and call(ldx=6) == -1
    assert call(H=48, K=0) == -2                               # the shape is judged first, as gnm_saliency does

    def z0(B=1, n_max=400, K=8, H=64, ldp=64, ldz=64):
        return lib.gnm_intgrad_z0(None, ldp, None, 0, None, None, B, n_max, None, K, H, None, ldz, None)
    assert z0(B=0) == 0
    assert z0(H=48) == -2 and z0(n_max=417) == -2 and z0(n_max=0) == -2
    assert z0(K=0) == -1 and z0(ldp=32) == -1 and z0(ldz=60) == -1
    assert z0() == -1                                          # a covered shape with NULL arrays (alphas among them)


# ---------------------------------------------------------------------------------------------- the method
def test_integrated_gradients_argument_validation():
    m, gs = _cpu_model()
    n, F0 = len(gs[0].g), gs[0].node_features.shape[1]
    small = type(gs[0]).__new__(type(gs[0]))
    small.g, small.edge_mat, small.node_features = [0, 1], torch.tensor([[0, 1], [1, 0]]), gs[0].node_features[:2]
    ok = np.zeros((n, F0), dtype=np.float32)
    bad = [dict(graphs=[], cls=0), dict(cls=2), dict(cls=-1), dict(cls=(0, 5)), dict(cls=()), dict(cls=0, batch_size=0),
           dict(cls=0, steps=0), dict(cls=0, steps=1, method="trapezoid"), dict(cls=0, method="simpson"),
           dict(cls=0, steps=2.5), dict(cls=0, baseline=np.zeros((n + 1, F0), dtype=np.float32)),
           dict(cls=0, baseline=np.zeros((n, F0 + 1), dtype=np.float32)), dict(cls=0, baseline=np.zeros(F0, np.float32)),
           dict(cls=0, baseline=np.full((n, F0), np.nan, dtype=np.float32)),
           dict(cls=0, baseline=np.zeros((n, F0), dtype=np.int64)),
           dict(graphs=gs + [small], cls=0, baseline=ok)]
    for kw in bad:
        kw = dict(kw)
        graphs = kw.pop("graphs", gs)
        with pytest.raises(ValueError):
            m.integrated_gradients(graphs, **kw)
    assert m.training                                       # validation fails before the mode changes


def test_integrated_gradients_has_no_cpu_fallback_and_restores_the_mode():
    from gnm._cabi import GnmError
    m, gs = _cpu_model()
    base = np.zeros((len(gs[0].g), gs[0].node_features.shape[1]), dtype=np.float32)
    for training in (True, False):
        m.train(training)
        for kw in (dict(), dict(baseline=base, method="gausslegendre", steps=3, return_scores=True)):
            with pytest.raises(GnmError):
                m.integrated_gradients(gs, (0, 1), **kw)
            assert m.training == training
