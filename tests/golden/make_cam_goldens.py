#!/usr/bin/env python3
"""Generate the class-activation-map goldens (cam/cam_*.npz) by running the REAL reference on CPU.

Run where the reference checkout is (it never travels to the GPU machine), like make_goldens.py:

    python tests/golden/make_cam_goldens.py

The reference's compute_saliency (models/graphcnn.py:254-299) retains the gradient of every layer output
(h.retain_grad(), :284) and allocates the two per-node maps class_activation / grad_class_activation (:288-289) that
nothing fills.  This script runs compute_saliency([g], c) with each layer's returned h captured (next_layer /
next_layer_eps wrapped on the instance) and stores, per graph g and class c, DATA ONLY:
  * h_{g}_{l}            hidden_rep[l] (eval mode), [n, H]
  * hgrad_{g}_{c}_{l}    h.grad left by compute_saliency's backward, [n, H]
  * cam_{g}_{c}          p_g sum_l <h_l[v], linears_prediction[l].weight[c]>           (fp64 from the fp32 tensors)
  * gcam_{g}_{c}         sum_l <h.grad[v], h_l[v]>                                      (fp64 from the fp32 tensors)
  * c_logit_{g}          the reference's eval forward([g]) c_logit, [1, C]
  * state_<name>         the seeded state_dict (the discriminator's left out: it plays no part)
for small graphs across graph pooling {sum, average} x neighbour pooling {sum, average, max} x learn_eps {on, off}.
"""
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import make_goldens as MG  # noqa: E402  (the reference import, SynthGraph, make_batch, build_model)

# a directory of their own: helpers.golden_cases() parametrizes other tests over every tests/golden/*.npz
OUT_DIR = os.path.join(HERE, "cam")
B, N_NODES, T, L, M, F0, H, C = 2, 20, 40, 3, 2, 5, 32, 2


def capture_layers(model):
    """wrap the instance's layer functions so every returned h (the tensor compute_saliency retains) is recorded"""
    hs = []
    for name in ("next_layer", "next_layer_eps"):
        orig = getattr(model, name)

        def wrapped(*a, _orig=orig, **k):
            h = _orig(*a, **k)
            hs.append(h)
            return h
        setattr(model, name, wrapped)
    return hs


def run_case(tag, model_seed, graph_seed, learn_eps, gpool, npool):
    graphs, raw = MG.make_batch(graph_seed, B, N_NODES, T, F0, keep_pct=30.0)
    for gr in graphs:       # neighbour "average" + learn_eps divides by the degree (graphcnn.py:157-158): no 0/0 rows
        if npool == "average" and learn_eps:
            assert min(len(x) for x in gr.neighbors) > 0, "%s: a node without neighbours; pick another seed" % tag
    model = MG.build_model(model_seed, L, M, F0, H, C, 0.0, learn_eps, gpool, npool)
    g = torch.Generator().manual_seed(model_seed + 5)
    with torch.no_grad():   # running statistics away from their defaults, so eval-mode BatchNorm matters
        for name, b in model.named_buffers():
            if name.endswith("running_mean"):
                b.copy_(0.1 * torch.randn(b.shape, generator=g))
            elif name.endswith("running_var"):
                b.copy_(0.5 + torch.rand(b.shape, generator=g))
    out = {"cfg": np.array([L, M, F0, H, C, int(learn_eps), B, N_NODES], dtype=np.int64),
           "gpool": np.array(gpool), "npool": np.array(npool)}
    for k, v in model.state_dict().items():
        if not k.startswith("disc."):               # the discriminator plays no part in the maps
            out["state_" + k] = v.detach().numpy().copy()
    for gi, (und, feats, label) in enumerate(raw):
        out[f"und_{gi}"] = und.astype(np.int16)
        out[f"feat_{gi}"] = feats
    out["labels"] = np.array([r[2] for r in raw], dtype=np.int64)
    Wp = [model.linears_prediction[l].weight.detach().numpy().astype(np.float64) for l in range(L)]
    hs = capture_layers(model)
    for gi, gr in enumerate(graphs):
        model.eval()
        np.random.seed(0)
        with torch.no_grad():
            c_logit, _ = model([gr])
        out[f"c_logit_{gi}"] = c_logit.numpy().copy()
        pg = 1.0 / N_NODES if gpool == "average" else 1.0
        pg = float(np.float32(pg))                    # the reference stores 1./len(graph.g) as fp32
        for c in range(C):
            hs.clear()
            model.compute_saliency([gr], c)
            assert len(hs) == L
            cam = np.zeros(N_NODES)
            gcam = np.zeros(N_NODES)
            for l, h in enumerate(hs):
                hv = h.detach().numpy()
                gv = h.grad.detach().numpy()
                if c == 0:
                    out[f"h_{gi}_{l}"] = hv.copy()
                out[f"hgrad_{gi}_{c}_{l}"] = gv.copy()
                cam += pg * (hv.astype(np.float64) @ Wp[l][c])
                gcam += (gv.astype(np.float64) * hv.astype(np.float64)).sum(1)
            out[f"cam_{gi}_{c}"] = cam
            out[f"gcam_{gi}_{c}"] = gcam
        model.zero_grad()
    os.makedirs(OUT_DIR, exist_ok=True)
    path = os.path.join(OUT_DIR, f"cam_{tag}.npz")
    np.savez_compressed(path, **out)
    print(f"cam_{tag}: {os.path.getsize(path) / 1024:.0f} KB")


def main():
    seed = 0
    for gpool in ("sum", "average"):
        for npool in ("sum", "average", "max"):
            for le in (True, False):
                run_case(f"g{gpool}_n{npool}_eps{int(le)}", 20 + seed, 3000 + 10 * seed, le, gpool, npool)
                seed += 1


if __name__ == "__main__":
    main()
