"""CPU checks of GIN_InfoMaxReg.edge_saliency() (connectivity saliency d score / d A): a test-local fp64 dense-adjacency
autograd restatement against the reference's goldens (tests/golden/edge/), the new C-ABI entries, the kernel in the
gfx950 code object, and argument validation -- everything that does not need a GPU."""
import glob
import os
import re

import numpy as np
import pytest
import torch

from helpers import GOLDEN_DIR, load_case
from test_cabi_host import graphs_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("gnm_edge_saliency", "gnm_edge_saliency_scratch_floats")
EDGE_CASES = sorted(os.path.basename(f)[:-4] for f in glob.glob(os.path.join(GOLDEN_DIR, "edge", "edge_*.npz")))
EDGE_RTOL = 1e-5        # of each graph's largest entry


def load_edge_case(name):
    d = dict(np.load(os.path.join(GOLDEN_DIR, "edge", name + ".npz")))
    L, m, f0, H, C, le, B, n = [int(x) for x in d["cfg"]]
    cfg = dict(L=L, m=m, f0=f0, H=H, C=C, learn_eps=bool(le), B=B, n=n, gpool=str(d["gpool"]), npool=str(d["npool"]))
    state = {k[len("state_"):]: v for k, v in d.items() if k.startswith("state_")}
    return cfg, state, d


def restate_edge(state, L, m, learn_eps, gpool, npool, src, dst, feats, cls, dtype=torch.float64):
    """d logit[cls] / d A of one graph's eval forward (graphcnn.py:151-231) with A a DENSE autograd leaf: 1 at every
    (src[k], dst[k]) of edge_mat (row = destination of the aggregation), plus the diagonal when learn_eps is False.
    Returns the [n, n] gradient, absent entries included."""
    assert npool in ("sum", "average")
    S = {k: torch.as_tensor(np.asarray(v), dtype=dtype) for k, v in state.items() if np.asarray(v).dtype.kind == "f"}
    n = feats.shape[0]
    A = torch.zeros((n, n), dtype=dtype)
    A.index_put_((torch.as_tensor(np.asarray(src, np.int64)), torch.as_tensor(np.asarray(dst, np.int64))),
                 torch.ones(len(src), dtype=dtype), accumulate=True)
    if not learn_eps:
        A = A + torch.eye(n, dtype=dtype)                                        # graphcnn.py:97-102
    A.requires_grad_()

    def bn(z, name):
        return (z - S[name + ".running_mean"]) / torch.sqrt(S[name + ".running_var"] + 1e-5) * S[name + ".weight"] \
            + S[name + ".bias"]

    h = torch.as_tensor(np.asarray(feats), dtype=dtype)
    logit = 0
    pg = float(np.float32(1.0 / n)) if gpool == "average" else 1.0
    for l in range(L):
        pooled = A @ h
        if npool == "average":
            pooled = pooled / (A @ torch.ones((n, 1), dtype=dtype))             # graphcnn.py:157-158
        if learn_eps:
            pooled = pooled + (1 + S["eps"][l]) * h
        x = pooled
        for k in range(m):                                                       # mlp.py:40-49
            wn = f"mlps.{l}.linear" if m == 1 else f"mlps.{l}.linears.{k}"
            x = x @ S[wn + ".weight"].T + S[wn + ".bias"]
            if k < m - 1:
                x = torch.relu(bn(x, f"mlps.{l}.batch_norms.{k}"))
        h = torch.relu(bn(x, f"batch_norms.{l}"))
        logit = logit + (pg * h.sum(0)) @ S[f"linears_prediction.{l}.weight"].T + S[f"linears_prediction.{l}.bias"]
    (g,) = torch.autograd.grad(logit[cls], A)
    return g


def _rel(a, ref):
    a, ref = np.asarray(a, np.float64), np.asarray(ref, np.float64)
    return np.abs(a - ref).max() / max(np.abs(ref).max(), 1e-30)


def test_edge_goldens_present():
    assert len(EDGE_CASES) == 8
    combos = {(load_edge_case(c)[0]["gpool"], load_edge_case(c)[0]["npool"], load_edge_case(c)[0]["learn_eps"])
              for c in EDGE_CASES}
    assert combos == {(g, n_, e) for g in ("sum", "average") for n_ in ("sum", "average") for e in (True, False)}
    isolated = 0
    for c in EDGE_CASES:
        cfg, _, d = load_edge_case(c)
        for g in range(cfg["B"]):
            assert d[f"edge_{g}_0"].shape == (cfg["n"], cfg["n"])
            und = d[f"und_{g}"].astype(np.int64)
            isolated += len(set(range(cfg["n"])) - set(und.ravel().tolist())) > 0
    assert isolated >= 6                  # every case but average + learned eps has a graph with an isolated node


@pytest.mark.parametrize("case", EDGE_CASES)
def test_restatement_reproduces_reference_goldens(case):
    cfg, state, d = load_edge_case(case)
    for g in range(cfg["B"]):
        und = d[f"und_{g}"].astype(np.int64)
        both = np.concatenate([und, und[:, ::-1]], 0)                            # util.py:99-103
        A = np.zeros((cfg["n"], cfg["n"]), bool)
        A[both[:, 0], both[:, 1]] = True
        for c in range(cfg["C"]):
            got = restate_edge(state, cfg["L"], cfg["m"], cfg["learn_eps"], cfg["gpool"], cfg["npool"], both[:, 0],
                               both[:, 1], d[f"feat_{g}"], c).numpy()
            ref = d[f"edge_{g}_{c}"]
            assert _rel(got, ref) <= EDGE_RTOL, (g, c, _rel(got, ref))
            # the reference's sparse-leaf gradient is dense: absent entries carry the sensitivity to adding an edge
            assert np.abs(ref[~A]).max() > 1e-3 * np.abs(ref).max()


def test_edge_entries_declared_bound_and_exported():
    from gnm import _cabi
    header = open(os.path.join(ROOT, "include", "gnm_hip.h")).read()
    declared = set(re.findall(r"\b(gnm_[a-z0-9_]+)\s*\(", header))
    for name in NEW:
        assert name in declared and name in _cabi.SIGNATURES
        assert getattr(_cabi.lib, name) is not None
    assert _cabi.lib.gnm_edge_saliency_scratch_floats(1000, 64, 5) == 7 * 1000 * 64


def test_edge_kernel_in_the_code_object(tmp_path):
    from test_isa_hazards import disassemble
    asm = disassemble(tmp_path)
    assert re.search(r"gnm_edge_saliency_kernel", asm)


def test_edge_saliency_bad_arguments_launch_nothing():
    """every check runs before a pointer is touched: UNSUPPORTED for declined shapes, BAD_ARG with NULL arrays"""
    from gnm._cabi import lib

    def call(B=1, n_max=400, H=64, L=5, m=2, Cn=2, cls=0, ldy=None, ldo=None):
        return lib.gnm_edge_saliency(None, None, None, None, None, None, B, n_max, B * n_max, H, L, m, Cn, cls, 0, 0,
                                     0, None, None, None, None, H if ldy is None else ldy, None,
                                     n_max if ldo is None else ldo, None)
    assert call(B=0) == 0                                   # nothing to do
    assert call(H=36) == -2 and call(H=256) == -2 and call(H=16) == -2
    assert call(m=4) == -2 and call(m=0) == -2 and call(L=17) == -2 and call(L=0) == -2
    assert call(n_max=417) == -2 and call(n_max=1000) == -2
    assert call(cls=2) == -1 and call(cls=-1) == -1
    assert call(ldo=399) == -1 and call(ldy=32) == -1
    assert call() == -1                                     # a covered shape with NULL arrays


def _cpu_model(case="tiny_s1_eps1_gsum_nsum"):
    from models.graphcnn import GIN_InfoMaxReg
    cfg, state, d = load_case(case)
    m = GIN_InfoMaxReg(cfg["L"], cfg["m"], cfg["f0"], cfg["H"], cfg["C"], 0.0, True, "sum", "sum", torch.device("cpu"))
    return m, graphs_of(cfg, d)


def test_edge_saliency_argument_validation():
    m, gs = _cpu_model()
    bad = [dict(graphs=[], cls=0), dict(cls=2), dict(cls=-1), dict(cls=(0, 5)), dict(cls=()),
           dict(cls=0, batch_size=0), dict(cls=0, batch_size=-3)]
    for kw in bad:
        kw = dict(kw)
        graphs = kw.pop("graphs", gs)
        with pytest.raises(ValueError):
            m.edge_saliency(graphs, **kw)
    assert m.training                                       # validation fails before the mode changes


def test_edge_saliency_has_no_cpu_fallback_and_restores_the_mode():
    from gnm._cabi import GnmError
    m, gs = _cpu_model()
    for training in (True, False):
        m.train(training)
        with pytest.raises(GnmError):
            m.edge_saliency(gs, (0, 1))
        assert m.training == training
