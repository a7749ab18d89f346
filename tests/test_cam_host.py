"""CPU checks of GIN_InfoMaxReg.class_activation() (the per-node class activation maps): a test-local fp64 autograd
restatement of the two maps against the reference's goldens (tests/golden/cam/), the new C-ABI entries, their kernels in
the gfx950 code object, and argument validation -- everything that does not need a GPU."""
import glob
import os
import re

import numpy as np
import pytest
import torch

from helpers import GOLDEN_DIR, load_case, neighbors_of
from test_cabi_host import graphs_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("gnm_class_activation", "gnm_class_activation_table_words", "gnm_class_activation_max_classes",
       "gnm_saliency_maps")
CAM_CASES = sorted(os.path.basename(f)[:-4] for f in glob.glob(os.path.join(GOLDEN_DIR, "cam", "cam_*.npz")))
CAM_RTOL = 1e-5         # of the largest entry; the goldens are fp32 tensors (the maps summed in fp64 from them)


def load_cam_case(name):
    d = dict(np.load(os.path.join(GOLDEN_DIR, "cam", name + ".npz")))
    L, m, f0, H, C, le, B, n = [int(x) for x in d["cfg"]]
    cfg = dict(L=L, m=m, f0=f0, H=H, C=C, learn_eps=bool(le), B=B, n=n, gpool=str(d["gpool"]), npool=str(d["npool"]))
    state = {k[len("state_"):]: v for k, v in d.items() if k.startswith("state_")}
    return cfg, state, d


def restate(state, L, m, learn_eps, gpool, npool, src, dst, neighbors, feats, cls, dtype=torch.float64):
    """One graph's eval forward as graphcnn.py:151-231 computes it, in `dtype` autograd, with every layer output
    retained (graphcnn.py:284).  Edges (src[k] -> dst[k]) as edge_mat; `neighbors` is graph.neighbors (its order is
    the max pooling's tie order).  Returns (h list, h.grad list, cam, gcam, c_logit row)."""
    S = {k: torch.as_tensor(np.asarray(v), dtype=dtype) for k, v in state.items() if np.asarray(v).dtype.kind == "f"}
    n = feats.shape[0]
    X = torch.as_tensor(np.asarray(feats), dtype=dtype).requires_grad_()         # graphcnn.py:260
    A = torch.zeros((n, n), dtype=dtype)
    src, dst = np.asarray(src, np.int64), np.asarray(dst, np.int64)
    A.index_put_((torch.as_tensor(src), torch.as_tensor(dst)), torch.ones(len(src), dtype=dtype), accumulate=True)
    if not learn_eps:
        A = A + torch.eye(n, dtype=dtype)                                        # graphcnn.py:97-103
    if npool == "max":                                                           # graphcnn.py:54-81
        max_deg = max(len(x) for x in neighbors)
        pad = torch.as_tensor([list(x) + [-1] * (max_deg - len(x)) + ([] if learn_eps else [j])
                               for j, x in enumerate(neighbors)], dtype=torch.int64).reshape(n, -1)

    def bn(z, name):                                                             # eval BatchNorm (running statistics)
        return (z - S[name + ".running_mean"]) / torch.sqrt(S[name + ".running_var"] + 1e-5) * S[name + ".weight"] \
            + S[name + ".bias"]

    hs = []
    h = X
    for l in range(L):
        if npool == "max":                                                       # graphcnn.py:137-143
            hd = torch.cat([h, torch.min(h, dim=0)[0].reshape(1, -1)])
            pooled = torch.max(hd[pad], dim=1)[0]
        else:
            pooled = A @ h
            if npool == "average":
                pooled = pooled / (A @ torch.ones((n, 1), dtype=dtype))
        if learn_eps:
            pooled = pooled + (1 + S["eps"][l]) * h
        x = pooled
        for k in range(m):                                                       # mlp.py:40-49
            wn = f"mlps.{l}.linear" if m == 1 else f"mlps.{l}.linears.{k}"
            x = x @ S[wn + ".weight"].T + S[wn + ".bias"]
            if k < m - 1:
                x = torch.relu(bn(x, f"mlps.{l}.batch_norms.{k}"))
        h = torch.relu(bn(x, f"batch_norms.{l}"))
        h.retain_grad()
        hs.append(h)
    pg = float(np.float32(1.0 / n)) if gpool == "average" else 1.0
    logit = 0
    for l, h in enumerate(hs):
        logit = logit + (pg * h.sum(0)) @ S[f"linears_prediction.{l}.weight"].T + S[f"linears_prediction.{l}.bias"]
    logit[cls].backward()
    with torch.no_grad():
        cam = sum(pg * (h @ S[f"linears_prediction.{l}.weight"][cls]) for l, h in enumerate(hs))
        gcam = sum((h.grad * h).sum(1) for h in hs)
    return [h.detach() for h in hs], [h.grad for h in hs], cam, gcam, logit.detach()


def _rel(a, ref):
    a, ref = np.asarray(a, np.float64), np.asarray(ref, np.float64)
    return np.abs(a - ref).max() / max(np.abs(ref).max(), 1e-30)


def test_cam_goldens_present():
    assert len(CAM_CASES) == 12
    pools = {(load_cam_case(c)[0]["gpool"], load_cam_case(c)[0]["npool"], load_cam_case(c)[0]["learn_eps"])
             for c in CAM_CASES}
    assert pools == {(g, n_, e) for g in ("sum", "average") for n_ in ("sum", "average", "max") for e in (True, False)}


@pytest.mark.parametrize("case", CAM_CASES)
def test_restatement_reproduces_reference_goldens(case):
    """h.grad on every retained layer output, both maps and the logit of the reference's compute_saliency([g], c)"""
    cfg, state, d = load_cam_case(case)
    for g in range(cfg["B"]):
        und = d[f"und_{g}"].astype(np.int64)
        both = np.concatenate([und, und[:, ::-1]], 0)                            # util.py:99-103
        for c in range(cfg["C"]):
            hs, grads, cam, gcam, logit = restate(state, cfg["L"], cfg["m"], cfg["learn_eps"], cfg["gpool"],
                                                  cfg["npool"], both[:, 0], both[:, 1], neighbors_of(und, cfg["n"]),
                                                  d[f"feat_{g}"], c)
            for l in range(cfg["L"]):
                assert _rel(hs[l], d[f"h_{g}_{l}"]) <= CAM_RTOL, (g, c, l, "h")
                assert _rel(grads[l], d[f"hgrad_{g}_{c}_{l}"]) <= CAM_RTOL, (g, c, l, "h.grad")
            assert _rel(cam, d[f"cam_{g}_{c}"]) <= CAM_RTOL, (g, c, "cam")
            assert _rel(gcam, d[f"gcam_{g}_{c}"]) <= CAM_RTOL, (g, c, "gcam")
            assert _rel(logit, d[f"c_logit_{g}"][0]) <= CAM_RTOL, (g, c, "logit")
            # the activation map is an exact decomposition of the logit
            bias = sum(float(state[f"linears_prediction.{l}.bias"][c]) for l in range(cfg["L"]))
            assert abs(float(cam.sum()) + bias - float(logit[c])) <= 1e-12 * (float(cam.abs().sum()) + abs(bias))


def test_cam_entries_declared_bound_and_exported():
    from gnm import _cabi
    header = open(os.path.join(ROOT, "include", "gnm_hip.h")).read()
    declared = set(re.findall(r"\b(gnm_[a-z0-9_]+)\s*\(", header))
    for name in NEW:
        assert name in declared and name in _cabi.SIGNATURES
        assert getattr(_cabi.lib, name) is not None
    assert _cabi.lib.gnm_class_activation_table_words(5) == 5 * 6
    assert _cabi.lib.gnm_class_activation_max_classes() == 8


def test_cam_kernels_in_the_code_object(tmp_path):
    from test_isa_hazards import disassemble
    asm = disassemble(tmp_path)
    assert re.search(r"gnm_class_activation_kernel", asm)
    assert re.search(r"_Z25gnm_saliency_layer_kernelILb1EEv6SlArgs", asm)      # the gradient-map form
    assert re.search(r"_Z25gnm_saliency_layer_kernelILb0EEv6SlArgs", asm)      # gnm_saliency's form


def test_class_activation_bad_arguments_launch_nothing():
    """every check runs before a pointer is touched: GNM_ERR_BAD_ARG with NULL arrays"""
    import ctypes as C
    from gnm._cabi import lib

    def call(B=2, n_max=40, N=80, H=64, L=5, Cn=2, cls=(0, 1), ldo=80):
        arr = (C.c_int * max(len(cls), 1))(*cls) if cls is not None else None
        return lib.gnm_class_activation(None, B, n_max, N, H, L, Cn, arr, len(cls or ()), 0, None, None, ldo, None)
    assert call() == -1                                     # a covered shape with NULL arrays
    assert call(H=36) == -1                                 # ... also at a width that is a multiple of 4
    assert call(H=6) == -1 and call(H=132) == -1 and call(H=0) == -1
    assert call(L=0) == -1 and call(L=17) == -1
    assert call(cls=(2,)) == -1 and call(cls=(-1,)) == -1 and call(cls=(0, 1, 2)) == -1
    assert call(cls=()) == -1 and call(cls=tuple([0] * 9)) == -1
    assert call(cls=None) == -1
    assert call(ldo=79) == -1 and call(B=-1) == -1
    assert call(B=0) == 0 and call(N=0, ldo=0) == 0         # nothing to do


def test_saliency_maps_bad_arguments_launch_nothing():
    from gnm._cabi import lib

    def call(B=1, n_max=400, H=64, L=5, m=2, Cn=2, cls=0):
        return lib.gnm_saliency_maps(None, None, None, None, None, B, n_max, B * n_max, H, L, m, Cn, cls, 0, 0, 0,
                                     None, None, None, None, None)
    assert call(B=0) == 0                                   # nothing to do
    assert call(H=36) == -2 and call(H=256) == -2
    assert call(m=4) == -2 and call(m=0) == -2 and call(L=17) == -2
    assert call(n_max=417) == -2
    assert call(cls=2) == -1 and call(cls=-1) == -1
    assert call() == -1                                     # a covered shape with NULL arrays


def _cpu_model(case="tiny_s1_eps1_gsum_nsum"):
    from models.graphcnn import GIN_InfoMaxReg
    cfg, state, d = load_case(case)
    m = GIN_InfoMaxReg(cfg["L"], cfg["m"], cfg["f0"], cfg["H"], cfg["C"], 0.0, True, "sum", "sum", torch.device("cpu"))
    return m, graphs_of(cfg, d)


def test_class_activation_argument_validation():
    m, gs = _cpu_model()
    bad = [dict(graphs=[], cls=0), dict(cls=2), dict(cls=-1), dict(cls=(0, 5)), dict(cls=()),
           dict(cls=0, batch_size=0), dict(cls=0, kind="cam"), dict(cls=0, kind="grad")]
    for kw in bad:
        kw = dict(kw)
        graphs = kw.pop("graphs", gs)
        with pytest.raises(ValueError):
            m.class_activation(graphs, **kw)
    assert m.training                                       # validation fails before the mode changes


@pytest.mark.parametrize("kind", ["activation", "gradient"])
def test_class_activation_has_no_cpu_fallback_and_restores_the_mode(kind):
    from gnm._cabi import GnmError
    m, gs = _cpu_model()
    for training in (True, False):
        m.train(training)
        with pytest.raises(GnmError):
            m.class_activation(gs, (0, 1), kind=kind)
        assert m.training == training
