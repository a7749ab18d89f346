#!/usr/bin/env python3
"""Generate occlusion/true_n400_*.npz: the CPU references of tests/test_gpu_occlusion.py's 400-node cases.

    python tests/golden/make_occlusion_true_shape.py

Needs nothing but this repository.  For the 400-node synth.dense_fc_graph(0) and the seeded model of the test
(test_gpu_saliency.model_of, built on the CPU: the same bits), all 400 node-deleted copies run through the fp64 oracle
(oracle/gin_oracle.py) and through the independent fp32 CPU forward (oracle/gin_torch_cpu.py) -- about two minutes of
CPU time, which is why the results are stored instead of recomputed by every test run:
  * base64 [C], occluded64 [400, C]     the fp64 oracle
  * base32 [C], occluded32 [400, C]     the fp32 CPU forward (its distance from the fp64 oracle calibrates the bound)
  * fingerprint                          per-tensor (sum, sum of |.|) of the model's state in fp64: the test asserts its
                                         own model is the one these numbers belong to
"""
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (os.path.dirname(HERE), ROOT, os.path.join(ROOT, "graph-neural-mapping_amd")):
    sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import test_gpu_saliency as T  # noqa: E402
from test_occlusion_host import delete_node, oracle_scores  # noqa: E402

# (tag, one_hot, neighbour pooling, graph pooling, learn_eps): L = 5, m = 2, H = 64, model seed 7
CASES = [("f7_gaverage_naverage_eps1", False, "average", "average", True),
         ("onehot_gsum_nsum_eps1", True, "sum", "sum", True)]


def fingerprint(state):
    return np.array([[np.asarray(state[k], np.float64).sum(), np.abs(np.asarray(state[k], np.float64)).sum()]
                     for k in sorted(state)])


def main():
    from gnm import synth
    from oracle import gin_oracle as O
    from oracle.gin_torch_cpu import TorchCpuGIN
    T.DEV = "cpu"
    for tag, one_hot, npool, gpool, le in CASES:
        g = synth.dense_fc_graph(0, n=400)
        if one_hot:
            g.node_features = torch.eye(400)
        model = T.model_of(5, 2, 400 if one_hot else 7, 64, le, gpool, npool, seed=7)
        st = {k: v.detach().numpy().astype(np.float64) if v.dtype.is_floating_point else v.numpy()
              for k, v in model.state_dict().items()}
        spec = (5, 2, le, gpool, npool)
        base64, occ64 = oracle_scores(st, spec, [g])
        cpu = TorchCpuGIN({k: np.asarray(v, dtype=np.float32) if np.asarray(v).dtype.kind == "f" else v
                           for k, v in st.items()}, *spec)

        def fp32(gr):
            with torch.no_grad():
                og = O.OGraph(len(gr.g), gr.edge_mat.numpy(), gr.node_features.numpy())
                return cpu.forward([og], [0], training=False, want_disc=False)[0].numpy()
        out = dict(base64=base64[0], occluded64=occ64[0], base32=fp32(g)[0],
                   occluded32=np.concatenate([fp32(delete_node(g, v)) for v in range(400)], 0),
                   fingerprint=fingerprint(st))
        assert np.isfinite(out["occluded64"]).all() and np.isfinite(out["occluded32"]).all()
        path = os.path.join(HERE, "occlusion", "true_n400_%s.npz" % tag)
        np.savez_compressed(path, **out)
        print(tag, "%.0f KB" % (os.path.getsize(path) / 1024))


if __name__ == "__main__":
    main()
