"""CPU checks of GIN_InfoMaxReg.saliency() (the batched eval-mode input gradient): its C-ABI entries, its kernel in the
gfx950 code object, and argument validation -- everything that does not need a GPU."""
import os
import re

import numpy as np
import pytest
import torch

from helpers import load_case
from test_cabi_host import graphs_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("gnm_saliency", "gnm_saliency_table_words", "gnm_saliency_scratch_floats")


def test_saliency_entries_declared_bound_and_exported():
    from gnm import _cabi
    header = open(os.path.join(ROOT, "include", "gnm_hip.h")).read()
    declared = set(re.findall(r"\b(gnm_[a-z0-9_]+)\s*\(", header))
    for name in NEW:
        assert name in declared and name in _cabi.SIGNATURES
        assert getattr(_cabi.lib, name) is not None
    assert _cabi.lib.gnm_saliency_table_words(5, 2) == 5 * 2 * 6 + 2 * 5
    assert _cabi.lib.gnm_saliency_scratch_floats(1000, 64) == 4 * 1000 * 64


def test_saliency_declines_what_it_does_not_cover():
    """shape checks run before anything touches a pointer: GNM_ERR_UNSUPPORTED / GNM_ERR_BAD_ARG with NULL arrays"""
    from gnm._cabi import lib

    def call(B=1, n_max=400, F0=7, H=64, L=5, m=2, C=2, cls=0, ldx=7):
        return lib.gnm_saliency(None, None, None, None, None, B, n_max, B * n_max, F0, H, L, m, C, cls, 0, 0, 0, None,
                                None, None, None, ldx, None)
    assert call(B=0) == 0                                   # nothing to do
    assert call(H=36) == -2 and call(H=256) == -2
    assert call(m=4) == -2 and call(m=0) == -2
    assert call(n_max=417) == -2
    assert call(F0=int(lib.gnm_linear_max_k(64)) + 1, ldx=1000) == -2
    assert call(cls=2) == -1 and call(cls=-1) == -1
    assert call() == -1                                     # a covered shape with NULL arrays


def test_saliency_kernel_in_the_code_object(tmp_path):
    from test_isa_hazards import disassemble
    asm = disassemble(tmp_path)
    assert re.search(r"gnm_saliency_layer_kernel", asm)


def _cpu_model(case="tiny_s1_eps1_gsum_nsum"):
    from models.graphcnn import GIN_InfoMaxReg
    cfg, state, d = load_case(case)
    m = GIN_InfoMaxReg(cfg["L"], cfg["m"], cfg["f0"], cfg["H"], cfg["C"], 0.0, True, "sum", "sum", torch.device("cpu"))
    return m, graphs_of(cfg, d)


def test_saliency_argument_validation():
    m, gs = _cpu_model()
    with pytest.raises(ValueError):
        m.saliency([], 0)
    with pytest.raises(ValueError):
        m.saliency(gs, 2)                                   # a 2-class model
    with pytest.raises(ValueError):
        m.saliency(gs, -1)
    with pytest.raises(ValueError):
        m.saliency(gs, (0, 5))
    with pytest.raises(ValueError):
        m.saliency(gs, ())
    with pytest.raises(ValueError):
        m.saliency(gs, 0, batch_size=0)
    assert m.training                                       # validation fails before the mode changes


def test_saliency_has_no_cpu_fallback_and_restores_the_mode():
    from gnm._cabi import GnmError
    m, gs = _cpu_model()
    m.train()
    for cls in (0, (0, 1), [1], np.int64(1)):
        with pytest.raises(GnmError):
            m.saliency(gs, cls)
        assert m.training
    m.eval()
    with pytest.raises(GnmError):
        m.saliency(gs, (0, 1))
    assert not m.training


def test_compute_saliency_keeps_the_one_graph_contract():
    m, gs = _cpu_model()
    assert len(gs) > 1
    with pytest.raises(AssertionError):
        m.compute_saliency(gs, 0)                           # graphcnn.py:257, untouched
