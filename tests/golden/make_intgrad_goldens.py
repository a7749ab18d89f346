#!/usr/bin/env python3
"""Generate the integrated-gradients goldens (intgrad/ig_*.npz, intgrad/true_n400_*.npz), DATA ONLY.

Run where the reference checkout is (it never travels to the GPU machine), like make_occlusion_goldens.py:

    python tests/golden/make_intgrad_goldens.py
    python tests/golden/make_intgrad_goldens.py --true-shape

ig_*.npz: the REAL reference on CPU.  The models and graphs are those of the occlusion goldens (occlusion/occ_*.npz,
named by `source`; nothing of them is stored twice).  For every graph g, class c and K in {1, 5} (midpoint rule) the
reference's compute_saliency([g_k], c) runs on explicit copies with the features x' + alpha_k (X - x'), and
  * alphas_{K}, weights_{K}   the quadrature (gnm/intgrad.py, fp64)
  * ref_{K}_{g}               (X - x') * sum_k w_k compute_saliency([g_k], c), c = 0, 1: [2, n, F0] accumulated in fp32
  * oracle_{K}_{g}            the same contract through the fp64 oracle (tests/test_intgrad_host.py oracle_ig)
  * baseline                  x' [n, F0] where it is not zero
Cases: graph pooling {sum, average} x neighbour pooling {sum, average} x learn_eps {on, off}, the asymmetric edge_mat,
the one-hot input, and one non-zero baseline.

true_n400_*.npz (--true-shape): needs nothing but this repository.  tests/test_gpu_intgrad.py's
400-node cases (synth.dense_fc_graph(0), test_gpu_saliency.model_of built on the CPU: the same bits; L = 5, H = 64,
K = 8, midpoint, classes 0 and 1, zero baseline):
  * attr64 [2, 400, F0]       the fp64 oracle attribution (one-hot: its [2, 400] diagonal -- X is the identity, so
                              every other entry is exactly zero)
  * dist32                    max |fp32 OracleGIN attribution - attr64| / max |attr64|: the independent fp32 CPU
                              restatement's own distance, which calibrates the device bound
  * fingerprint               per-tensor (sum, sum of |.|) of the model's state in fp64
"""
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (os.path.join(ROOT, "graph-neural-mapping_amd"), ROOT, os.path.dirname(HERE), HERE):
    sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

OUT_DIR = os.path.join(HERE, "intgrad")
TRUE_CASES = [("f7_gaverage_naverage_eps1", False, "average", "average", True),
              ("onehot_gsum_nsum_eps1", True, "sum", "sum", True)]
TRUE_K = 8


def quadrature(method, steps):
    """gnm/intgrad.py, loaded by path: importing the gnm package would build and load the HIP library"""
    import importlib.util
    spec = importlib.util.spec_from_file_location(
        "_intgrad_rules", os.path.join(ROOT, "graph-neural-mapping_amd", "gnm", "intgrad.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.quadrature(method, steps)


def reference_case(tag, source, baseline_seed=None):
    import make_goldens as MG  # the reference import, build_model
    from test_intgrad_host import oracle_ig
    from test_occlusion_host import load_occ_case, occ_graphs
    cfg, state, d = load_occ_case(source)
    graphs = occ_graphs(cfg, d)
    model = MG.build_model(0, cfg["L"], cfg["m"], cfg["f0"], cfg["H"], cfg["C"], 0.0, cfg["learn_eps"], cfg["gpool"],
                           cfg["npool"])
    missing, unexpected = model.load_state_dict({k: torch.as_tensor(v) for k, v in state.items()}, strict=False)
    assert not unexpected and all(k.startswith("disc.") for k in missing)
    out = {"source": np.array(source)}
    baseline = None
    if baseline_seed is not None:
        baseline = (0.5 * np.random.default_rng(baseline_seed).standard_normal((cfg["n"], cfg["f0"]))).astype(np.float32)
        out["baseline"] = baseline
    for K in (1, 5):
        alphas, weights = quadrature("midpoint", K)
        out[f"alphas_{K}"], out[f"weights_{K}"] = alphas, weights
        for gi, gr in enumerate(graphs):
            X = gr.node_features.clone()
            x0 = torch.zeros_like(X) if baseline is None else torch.from_numpy(baseline)
            acc = torch.zeros((2,) + tuple(X.shape))
            for a, w in zip(alphas.astype(np.float32), weights.astype(np.float32)):
                gr.node_features = x0 + float(a) * (X - x0)
                for c in (0, 1):
                    acc[c] += float(w) * model.compute_saliency([gr], c).detach()
            gr.node_features = X
            out[f"ref_{K}_{gi}"] = (acc * (X - x0)).numpy().copy()
            out[f"oracle_{K}_{gi}"] = oracle_ig(state, cfg, gr, (0, 1), alphas, weights, baseline)[0]
            scale = np.abs(out[f"oracle_{K}_{gi}"]).max()
            err = np.abs(out[f"ref_{K}_{gi}"] - out[f"oracle_{K}_{gi}"]).max() / scale
            assert np.isfinite(out[f"ref_{K}_{gi}"]).all() and scale > 0 and err < 1e-5, (tag, K, gi, err)
    os.makedirs(OUT_DIR, exist_ok=True)
    path = os.path.join(OUT_DIR, f"ig_{tag}.npz")
    np.savez_compressed(path, **out)
    print(f"ig_{tag}: {os.path.getsize(path) / 1024:.0f} KB")


def fingerprint(state):
    return np.array([[np.asarray(state[k], np.float64).sum(), np.abs(np.asarray(state[k], np.float64)).sum()]
                     for k in sorted(state)])


def true_shape():
    import test_gpu_saliency as T
    from gnm import synth
    from test_intgrad_host import oracle_ig
    T.DEV = "cpu"
    alphas, weights = quadrature("midpoint", TRUE_K)
    for tag, one_hot, npool, gpool, le in TRUE_CASES:
        g = synth.dense_fc_graph(0, n=400)
        if one_hot:
            g.node_features = torch.eye(400)
        model = T.model_of(5, 2, 400 if one_hot else 7, 64, le, gpool, npool, seed=7)
        st = {k: v.detach().numpy().astype(np.float64) if v.dtype.is_floating_point else v.numpy()
              for k, v in model.state_dict().items()}
        spec = (5, 2, le, gpool, npool)
        a64 = oracle_ig(st, spec, g, (0, 1), alphas, weights)[0]
        a32 = oracle_ig(st, spec, g, (0, 1), alphas.astype(np.float32), weights.astype(np.float32), dtype=np.float32)[0]
        assert np.isfinite(a64).all() and np.isfinite(a32).all()
        dist = float(np.abs(a32 - a64).max() / np.abs(a64).max())
        if one_hot:
            off = a64.copy()
            off[:, np.arange(400), np.arange(400)] = 0
            assert not off.any()
            a64 = a64[:, np.arange(400), np.arange(400)]
        path = os.path.join(OUT_DIR, "true_n400_%s.npz" % tag)
        os.makedirs(OUT_DIR, exist_ok=True)
        np.savez_compressed(path, attr64=a64, dist32=np.float64(dist), fingerprint=fingerprint(st))
        print("true_n400_%s: fp32 restatement %.2e from fp64, %.0f KB" % (tag, dist, os.path.getsize(path) / 1024))


def main():
    if "--true-shape" in sys.argv:       # a process of its own: the reference's `models` package shadows the project's
        return true_shape()
    for gpool in ("sum", "average"):
        for npool in ("sum", "average"):
            for le in (True, False):
                tag = f"g{gpool}_n{npool}_eps{int(le)}"
                reference_case(tag, "occ_" + tag)
    reference_case("asym_gaverage_naverage_eps0", "occ_asym_gaverage_naverage_eps0")
    reference_case("onehot_gsum_nsum_eps1", "occ_onehot_gsum_nsum_eps1")
    reference_case("baseline_gaverage_nsum_eps1", "occ_gaverage_nsum_eps1", baseline_seed=9)


if __name__ == "__main__":
    main()
