"""The CPU half of the training-step envelope (tests/train_envelope_cases.py; the GPU half is
tests/test_gpu_train_envelope.py).  For every case, without a GPU:

  * the fp64 oracle runs, and where the fp32 CPU restatement applies (sum / average pooling, no dropout masks) its own
    error against fp64 stays under the reference ceilings: 1e-4 for values, TRUE_SHAPE_GRAD_RTOL for gradients -- a case
    that needs more is badly conditioned and is redrawn, not loosened;
  * in a small case (L <= 5, n <= 64) the smallest |pre-activation| under each ReLU is at least 1e-5 x that ReLU's
    largest: no small case sits on a mask boundary;
  * the declared route is what the routing code does with it: core.agg_launch / core._agg and core.linear_bwd_launch
    run on spies programmed with the declared statuses must call exactly the declared entries, core._dense on the
    case's own fill and width must agree with the declared aggregation kernel, and each declared accept / decline must
    agree with the entry's documented width rule (gnm_agg_slice_width for the CSR forms)."""
import numpy as np
import pytest
import torch

import train_envelope_cases as T
from helpers import TRUE_SHAPE_GRAD_RTOL, rel_err
from test_host_logic import _fake_agg_batch, _fake_lin_save

IDS = [c.id for c in T.CASES]
VALUE_CEILING = 1e-4
_STREAM = 4242


def _gmax(grads):
    m = [float(np.nanmax(np.abs(v))) for k, v in grads.items() if not k.startswith("__") and np.isfinite(v).any()]
    return max(m) if m else 0.0


@pytest.mark.parametrize("case", T.CASES, ids=IDS)
def test_oracle_runs_and_case_is_well_conditioned(case):
    ref, r32 = T.reference(case)
    nan_case = case.kind == "iso" and case.npool == "average" and case.eps
    assert np.isnan(ref["c_logit"]).all() if nan_case else np.isfinite(ref["c_logit"]).all()
    assert ref["d_logit"].shape == (2 * case.B * case.n, 1)
    names = {k for k in T.case_data(case).state if not k.endswith(("running_mean", "running_var", "num_batches_tracked"))}
    assert set(ref["grads"]) == names - (set() if case.eps else {"eps"})
    if r32 is None:
        assert case.npool == "max" or case.drop > 0
        return
    for what in ("c_logit", "d_logit"):
        e = rel_err(r32[what], ref[what])
        assert e <= VALUE_CEILING, "%s: the fp32 CPU step is %.2e from fp64" % (what, e)
    if not nan_case:
        assert abs(r32["loss"] - ref["loss"]) <= VALUE_CEILING * abs(ref["loss"])
    for k, v in ref["buffers"].items():
        e = rel_err(r32["buffers"][k], v)
        assert e <= VALUE_CEILING, "%s: the fp32 CPU step is %.2e from fp64" % (k, e)
    floor = 2e-2 * _gmax(ref["grads"])
    for k, v in ref["grads"].items():
        e = rel_err(r32["grads"][k].reshape(np.shape(v)), v, floor)
        assert e <= TRUE_SHAPE_GRAD_RTOL, "%s: the fp32 CPU gradient is %.2e from fp64" % (k, e)


@pytest.mark.parametrize("case", [c for c in T.CASES if c.L <= 5 and c.n <= 64],
                         ids=[c.id for c in T.CASES if c.L <= 5 and c.n <= 64])
def test_no_small_case_sits_on_a_relu_boundary(case):
    ref, _ = T.reference(case)
    state = T.case_data(case).state
    for l, lc in enumerate(ref["cache"]["layers"]):
        acts = [(lc["bn_out"][0], "batch_norms.%d" % l)]
        acts += [(ent[2], "mlps.%d.batch_norms.%d" % (l, k)) for k, ent in enumerate(lc["mlp"]) if ent[0] == "lin_bn_relu"]
        for (xhat, _, gamma, _), bn in acts:
            y = xhat * gamma + state[bn + ".bias"].astype(np.float64)
            if np.isnan(y).all():
                continue
            ratio = float(np.abs(y).min() / np.abs(y).max())
            assert ratio >= T.RELU_MARGIN, "%s: |pre-activation| down to %.1e x the largest" % (bn, ratio)


# --------------------------------------------------------------------------- the declared route vs the routing code
def _program(monkeypatch, core, names, events):
    """spies on core.lib for `names` that return the status `events` ("entry[label]:status", in order) declare for
    them; returns the log of "entry[label]:status" they were called with"""
    want = {}
    for e in events:
        name, rc = e.rsplit(":", 1)
        want.setdefault(name, []).append(int(rc))
    log = []

    def spy(name):
        def call(*a):
            label = name
            if name == "gnm_linear_bwd_fused" and a[25] is not None:
                label += "[sums]"
            if name == "gnm_linear_fwd":
                assert a[4] == 1
                label += "[dgrad]"
            q = want.get(label)
            assert q, "%s was called, which the declared route %s does not have (so far: %s)" % (label, events, log)
            rc = q.pop(0)
            log.append("%s:%d" % (label, rc))
            return rc
        return call
    for name in names:
        monkeypatch.setattr(core.lib, name, spy(name), raising=False)
    return log


_AGG_NAMES = ("gnm_agg", "gnm_aggm", "gnm_agg_fwd_bnrelu", "gnm_aggm_fwd_bnrelu", "gnm_agg_bwd_stats", "gnm_aggm_bwd_stats")
_LIN_NAMES = ("gnm_linear_bwd_fused_rz", "gnm_linear_bwd_fused", "gnm_bn_bwd_apply", "gnm_linear_wgrad",
              "gnm_linear_dgrad_masked", "gnm_linear_fwd")


def _csr_fused_takes(lib, F, n):
    fs = int(lib.gnm_agg_slice_width(F, n))
    return (F == 64 and fs == 64) or (fs == 32 and F % 32 == 0)


def _check_agg(monkeypatch, core, case, fb, spec, code, F, backward, layer0):
    lib = core.lib
    events = [e for e in T.agg_events(code, backward, layer0) if e != T.READOUT]
    if code.startswith("max"):
        for form in ("fwd_bnrelu", "bwd_stats"):
            log = _program(monkeypatch, core, _AGG_NAMES, [])
            assert core.agg_launch(fb, form, F, (0,) * 8, spec, backward=form == "bwd_stats") == (-2, 0) and log == []
        assert (code == "max-t") <= (F in (32, 64)), "the tiled neighbour-max kernels take F = 32 or 64 only"
        return
    # core._dense on the case's own fill, width and isolated nodes against the kernel the case declares
    assert core._dense(fb, F, spec) == (code[0] in "Mm"), (code, F, fb.dense, fb.iso)
    fused = [e for e in events if "fwd_bnrelu" in e or "bwd_stats" in e]
    plain = [e for e in events if e not in fused]
    if fused:
        log = _program(monkeypatch, core, _AGG_NAMES, fused)
        rc, _ = core.agg_launch(fb, "bwd_stats" if backward else "fwd_bnrelu", F, (0,) * 8, spec, backward=backward)
        assert log == fused and rc == (-2 if plain else 0), (log, fused, rc)
        # the entries' own width rules (csrc/aggm.hip: F == 64 only; csrc/agg.hip: one 64-wide slice or 32-float slices)
        for e in fused:
            name, rc = e.rsplit(":", 1)
            takes = F == 64 if name.startswith("gnm_aggm") else _csr_fused_takes(lib, F, case.n)
            assert takes == (rc == "0"), "%s at F = %d, n = %d" % (e, F, case.n)
    if plain:
        x, y = torch.zeros(fb.N, F), torch.zeros(fb.N, F)
        deps = torch.zeros(64, dtype=torch.float64) if backward and case.eps else None
        log = _program(monkeypatch, core, _AGG_NAMES, plain)
        core._agg(fb, x, y, F, 1000 if case.eps else None, spec, backward, x if deps is not None else None, deps)
        assert log == plain, (log, plain)
        if "gnm_aggm:-2" in plain:        # the partial block takes the plain form without d-eps partials only
            assert F < 32 and deps is not None


@pytest.mark.parametrize("case", T.CASES, ids=IDS)
def test_declared_route_is_what_the_routing_code_does(case, monkeypatch):
    from gnm import core
    lib = core.lib
    monkeypatch.setattr(core, "_STREAM", _STREAM)
    monkeypatch.setattr(core, "TIMER", None)
    graphs = T.case_data(case).graphs
    dense, iso = T.expected_dense(case, graphs), T.has_isolated(graphs)
    assert iso or case.kind != "iso"
    fb = _fake_agg_batch(dense, iso)
    spec = core.GinSpec(case.L, case.m, case.eps, case.gpool, case.npool)
    route = T.expected_route(case)
    # ---- aggregation
    assert (case.agg0 is not None) == (not case.p0 or case.npool == "max")
    if case.agg0:
        _check_agg(monkeypatch, core, case, fb, spec, case.agg0, case.F0, False, True)
    if case.L > 1:
        _check_agg(monkeypatch, core, case, fb, spec, case.fwd, case.H, False, False)
        _check_agg(monkeypatch, core, case, fb, spec, case.bwd, case.H, True, False)
    # ---- Linear backward
    N = 100
    for (l, k), events in route["lin"].items():
        K, H, pro, below, need_dA = T.lin_shape(case, l, k)
        code = T.lin_code(case, l, k)
        sv = _fake_lin_save(core, N, K, H, pro)
        lo = _fake_lin_save(core, N, 5, K, False) if below else None
        G, W, bias, dW, db = torch.zeros(N, H), torch.zeros(H, K), torch.zeros(H), torch.zeros(H, K), torch.zeros(H)
        coef = tuple(torch.zeros(H) for _ in range(3))
        log = _program(monkeypatch, core, _LIN_NAMES, events + ["gnm_bn_bwd_apply:0"])
        r = core.linear_bwd_launch(sv, lo, G, coef, W, bias, dW, db, need_dA, N, _STREAM)
        assert [e for e in log if not e.startswith("gnm_bn_bwd_apply")] == events, ((l, k), log, events)
        assert (r.job is not None) == (code in ("rz", "fused", "fused+sums"))
        assert (r.lo_sums is not None) == (code in ("fused+sums", "generic+masked"))
        # the entries' own shape rules (csrc/linear_bwd.hip)
        sums = below and need_dA
        rz_takes = H == 64 and not sums and ((K == 64 and need_dA) or (K <= 16 and not pro))
        fused_takes = H in (32, 64) and (K in (32, 64) or (1 <= K < 32 and not sums))
        assert (code == "rz") == rz_takes, ((l, k), code)
        assert (code in ("fused", "fused+sums")) == (fused_takes and not rz_takes), ((l, k), code)
        assert (code == "fused+sums") == (fused_takes and bool(sums)), ((l, k), code)
        assert (code == "generic+masked") == (not fused_takes and not rz_takes and K == 128 and H == 128 and bool(sums))
    # ---- head and discriminator (csrc/head.hip head_shape_ok, csrc/disc.hip's vector forms)
    assert (case.head == 0) == (case.C <= 256 and case.L * case.C <= 4096)
    assert (case.disc == "unit") == (case.H // 4 in (8, 16, 32) and case.H % 4 == 0 and case.L <= 5)
    assert case.F0 <= int(lib.gnm_linear_max_k(case.H))
    if case.pair:
        other = T.BY_ID[case.pair]
        assert (other.data or other.id) == (case.data or case.id)


def test_every_route_of_the_envelope_has_a_case():
    """each route the envelope names is declared by at least one case (the ids are listed in
    profiles/train_envelope_parity.md)"""
    seen = set()
    for c in T.CASES:
        r = T.expected_route(c)
        for seq in r["fwd"] + list(r["bwd"].values()) + list(r["lin"].values()) + [r["head"], r["disc"]]:
            seen.update(seq)
    for entry in ("gnm_aggm:0", "gnm_agg:0", "gnm_aggm:-2", "gnm_aggm_fwd_bnrelu:0", "gnm_aggm_fwd_bnrelu:-2",
                  "gnm_agg_fwd_bnrelu:0", "gnm_agg_fwd_bnrelu:-2", "gnm_aggm_bwd_stats:0", "gnm_aggm_bwd_stats:-2",
                  "gnm_agg_bwd_stats:0", "gnm_agg_bwd_stats:-2", "gnm_linear_bwd_fused_rz:0", "gnm_linear_bwd_fused:0",
                  "gnm_linear_bwd_fused[sums]:0", "gnm_linear_bwd_fused:-2", "gnm_linear_bwd_fused[sums]:-2",
                  "gnm_linear_wgrad:0", "gnm_linear_dgrad_masked:0", "gnm_linear_fwd[dgrad]:0",
                  "gnm_maxpool_fwd_tiled:0", "gnm_maxpool_fwd_tiled:-2", "gnm_maxpool_fwd:0", "gnm_maxpool_bwd_tiled:0",
                  "gnm_maxpool_bwd_tiled:-2", "gnm_maxpool_bwd:0", "gnm_bn_relu_readout:0", "gnm_head_fwd:0",
                  "gnm_head_fwd:-2", "gnm_disc_score_fwd_unit:0", "gnm_disc_score_fwd_unit:-2", "gnm_disc_score_fwd:0",
                  "gnm_disc_unit_scale:0", "gnm_disc_score_bwd:0"):
        assert entry in seen, entry
