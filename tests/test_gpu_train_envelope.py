"""One training step (forward, loss, hand-written backward) across its dispatch envelope, against the fp64 oracle
(oracle/gin_oracle.py OracleGIN.train_step_grads): the case table of tests/train_envelope_cases.py, whose ids name the
route each case is there to reach.

Every case first asserts its ROUTE.  The C entries the step chooses among (core.agg_launch, core.linear_bwd_launch, the
neighbour-max kernels, the head, the discriminator) are wrapped on gnm.core.lib by spies that record the entry, its
status and its shape arguments; after the step the log is cut into layers and Linears and compared with the sequences
the case declares (train_envelope_cases.expected_route): a case whose route moved fails with both sequences in the
message.  Then the values: c_logit, d_logit, the loss, every parameter gradient (eps.grad is None without learn_eps),
every BatchNorm's running statistics with num_batches_tracked == 1, and with keep_hidden each hidden layer per node.

Bounds never come from a HIP output.  Small cases (L <= 5, n <= 64), and every case with dropout masks or neighbour
max, which the fp32 CPU restatement does not have: the fuzz test's bounds -- RTOL for logits, loss, buffers and hidden
layers, 5 RTOL for gradients with the 2e-2 gmax floor.  Every other case: max(that, TRUE_SHAPE_FACTOR x the error of
oracle/gin_torch_cpu.py TorchCpuGIN.train_step against fp64 on the same case: the largest over its values / over its
gradients), that error itself at most 1e-4 for values and TRUE_SHAPE_GRAD_RTOL for gradients, and a gradient passes
within its bound of the fp64 oracle or of the fp32 CPU result (a ReLU mask bit may fall either way:
helpers.assert_grad_true_shape).  The measured worst errors, the reference's own and the bounds are printed, and
collected in the JSON file GNM_TRAIN_ENVELOPE_REPORT names when it is set (profiles/train_envelope_parity.md).

The all-NaN case (agg-iso-avg-eps1-gather-nan: neighbour average + learn_eps with isolated nodes makes every train-mode
BatchNorm statistic, output and gradient of the reference NaN) pins the backward's ReLU mask to torch's threshold
backward, y <= 0 ? 0 : g: a NaN pre-activation lets the gradient through."""
import contextlib
import json
import os

import numpy as np
import pytest
import torch

import train_envelope_cases as T
from helpers import RTOL, TRUE_SHAPE_FACTOR, TRUE_SHAPE_GRAD_RTOL, fixed_dropout, rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
VALUE_CEILING = 1e-4
REPORT = os.environ.get("GNM_TRAIN_ENVELOPE_REPORT")

# entry -> the positions of its shape arguments (include/gnm_hip.h)
SPIED = {
    "gnm_agg": dict(B=7, n_max=8, F=14, backward=18), "gnm_aggm": dict(B=9, n_max=10, F=15, backward=19),
    "gnm_agg_fwd_bnrelu": dict(B=5, n_max=6, F=19), "gnm_aggm_fwd_bnrelu": dict(B=7, n_max=8, F=20),
    "gnm_agg_bwd_stats": dict(B=7, n_max=8, F=14), "gnm_aggm_bwd_stats": dict(B=9, n_max=10, F=15),
    "gnm_linear_bwd_fused_rz": dict(N=21, K=22, H=23), "gnm_linear_bwd_fused": dict(N=22, K=23, H=24),
    "gnm_linear_wgrad": dict(N=4, H=5, K=6), "gnm_linear_dgrad_masked": dict(N=6, K=7, H=8),
    "gnm_linear_fwd": dict(N=8, K=9, H=10),
    "gnm_maxpool_fwd": dict(N=4, F=5), "gnm_maxpool_fwd_tiled": dict(B=5, n_max=6, F=7),
    "gnm_maxpool_bwd": dict(N=5, F=6), "gnm_maxpool_bwd_tiled": dict(B=6, n_max=7, F=8),
    "gnm_bn_relu_readout": dict(B=7, H=8),
    "gnm_disc_score_fwd": dict(L=4, H=5, N=11, B=12), "gnm_disc_score_fwd_unit": dict(L=4, H=5, N=11, B=12),
    "gnm_disc_unit_scale": dict(LH=2, B=5), "gnm_disc_score_bwd": dict(L=4, H=5),
    "gnm_head_fwd": dict(B=2, L=3, H=4, C=5),
    "gnm_small_gemm": dict(M=8, N=9, K=10),
}
_AGG = {"gnm_agg", "gnm_aggm", "gnm_agg_fwd_bnrelu", "gnm_aggm_fwd_bnrelu", "gnm_agg_bwd_stats", "gnm_aggm_bwd_stats",
        "gnm_maxpool_fwd", "gnm_maxpool_fwd_tiled", "gnm_maxpool_bwd", "gnm_maxpool_bwd_tiled", "gnm_bn_relu_readout"}
_LIN = {"gnm_linear_bwd_fused_rz", "gnm_linear_bwd_fused", "gnm_linear_bwd_fused[sums]", "gnm_linear_wgrad",
        "gnm_linear_dgrad_masked", "gnm_linear_fwd[dgrad]"}
_DISC = {"gnm_disc_score_fwd", "gnm_disc_score_fwd_unit", "gnm_disc_unit_scale", "gnm_disc_score_bwd"}


def install_spies(mp, core, phase):
    """wrap every entry of SPIED on core.lib; returns the log of (phase, label, status, shape arguments)"""
    log = []

    def spy(name, real, where):
        def call(*a):
            rc = real(*a)
            label = name
            if name == "gnm_linear_bwd_fused" and a[25] is not None:
                label += "[sums]"              # with the lower BatchNorm's sums (sZ)
            elif name == "gnm_linear_fwd" and a[4]:
                label += "[dgrad]"             # the weight k-major: dX = dZ W
            log.append((phase[0], label, int(rc), {k: a[i] for k, i in where.items()}))
            return rc
        return call
    for name, where in SPIED.items():
        mp.setattr(core.lib, name, spy(name, getattr(core.lib, name), where), raising=False)
    return log


def cut_route(case, log):
    """the log of one step cut like train_envelope_cases.expected_route: the forward's aggregation events per layer
    (the Linears' forward launches separate the layers), the backward's Linear groups and aggregation events"""
    L, m = case.L, case.m
    ev = lambda e: "%s:%d" % (e[1], e[2])     # noqa: E731
    fwd, nlin = [[] for _ in range(L + 1)], 0
    for e in log:
        if e[0] != "fwd":
            continue
        if e[1] == "gnm_linear_fwd":
            nlin += 1
        elif e[1] in _AGG:
            assert e[3].get("F", e[3].get("H")) == (case.F0 if nlin == 0 else case.H), e
            fwd[min(nlin // m, L)].append(ev(e))
    assert nlin == L * m, "%d Linear forward launches for %d Linears" % (nlin, L * m)
    groups, shapes, bwd = [], [], {}
    for e in log:
        if e[0] != "bwd":
            continue
        if e[1] in _LIN:
            first = e[1] == "gnm_linear_bwd_fused_rz" or (e[1].startswith("gnm_linear_bwd_fused") and not (
                groups and groups[-1][-1] == "gnm_linear_bwd_fused_rz:-2"))
            if first:
                groups.append([])
                shapes.append((e[3]["K"], e[3]["H"]))
            groups[-1].append(ev(e))
        elif e[1] in _AGG:
            assert e[3]["F"] == case.H, e
            bwd.setdefault(L - len(groups) // m, []).append(ev(e))
    assert len(groups) == L * m, "%d Linear backward groups for %d Linears: %s" % (len(groups), L * m, groups)
    lin = {}
    for g, (seq, shape) in enumerate(zip(groups, shapes)):
        l, k = L - 1 - g // m, m - 1 - g % m
        assert shape == T.lin_shape(case, l, k)[:2], ((l, k), shape)
        lin[(l, k)] = seq
    return dict(fwd=fwd, lin=lin, bwd=bwd, head=[ev(e) for e in log if e[1] == "gnm_head_fwd"],
                disc=[ev(e) for e in log if e[1] in _DISC],
                gemm=[ev(e) for e in log if e[1] == "gnm_small_gemm" and e[0] != "cache"])


def assert_route(case, got):
    want = T.expected_route(case)
    for part in ("fwd", "lin", "bwd", "head", "disc"):
        assert got[part] == want[part], "%s: the %s route moved\n  expected %s\n  actual   %s" % (
            case.id, part, want[part], got[part])
    # the three [B, L H]-sized products of the Infomax tail: the hand-written kernel takes each of them
    assert got["gemm"] == ["gnm_small_gemm:0"] * 3, got["gemm"]


_RESULTS = {}


def step(case):
    """one training step of `case` on the GPU with the spies installed (once per case: the results are shared by the
    tests that compare two cases)"""
    if case.id in _RESULTS:
        return _RESULTS[case.id]
    from gnm import core
    from gnm.train import infomax_loss
    from models.graphcnn import GIN_InfoMaxReg
    d = T.case_data(case)
    dev = torch.device(DEV)
    model = GIN_InfoMaxReg(case.L, case.m, case.F0, case.H, case.C, case.drop, case.eps, case.gpool, case.npool, dev)
    model.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in d.state.items()})
    model = model.to(dev).train()
    sp = model._spec
    sp.keep_hidden = case.keep
    sink = None
    if case.sink:
        sink = sp.grad_sink = {n: torch.full_like(p, float("nan")) for n, p in model.named_parameters()}
    phase, seen = ["cache"], {}
    with pytest.MonkeyPatch.context() as mp:
        log = install_spies(mp, core, phase)
        real_encoder = core.encoder_forward

        def encoder(*a, **k):
            out = real_encoder(*a, **k)
            seen["hidden"] = out[0]
            return out
        mp.setattr(core, "encoder_forward", encoder)
        bt = model._batch_of(d.graphs) if sp.n_max else model.arena().batch(d.graphs)
        X = None
        if not case.p0 and not sp.n_max:
            X = bt.arena.features(bt)              # the layer-0 cache off: the aggregation of X runs in the step
        elif not sp.n_max:
            bt.arena.features_and_agg0(bt, sp.n_avg, not sp.learn_eps)     # the cache filled before the step
        labels = torch.tensor([g.label for g in d.graphs], device=dev)
        phase[0] = "fwd"
        with fixed_dropout(d.masks) if d.masks is not None else contextlib.nullcontext():
            c_logit, d_logit = model.forward_batch(bt, X=X, perm=d.perm)
        N = bt.N
        if case.loss == "infomax":
            loss = infomax_loss(c_logit, d_logit, labels, beta=T.BETA)[0]
        else:
            y = torch.cat([torch.ones(N, 1), torch.zeros(N, 1)]).to(dev)
            loss = torch.nn.functional.cross_entropy(c_logit, labels) + \
                T.BETA * torch.nn.functional.binary_cross_entropy_with_logits(d_logit, y)
        phase[0] = "bwd"
        loss.backward()
        torch.cuda.synchronize()
    grads, none = {}, []
    for name, p in model.named_parameters():
        if sink is not None:
            assert p.grad is None, "%s: .grad set although a gradient sink is installed" % name
            if name == "eps" and not case.eps:
                assert bool(torch.isnan(sink[name]).all())          # no gradient: the sink is left alone
                none.append(name)
            else:
                grads[name] = sink[name].cpu().numpy()
        elif p.grad is None:
            none.append(name)
        else:
            grads[name] = p.grad.detach().cpu().numpy()
    res = dict(c_logit=c_logit.detach().cpu().numpy(), d_logit=d_logit.detach().cpu().numpy(), loss=float(loss.item()),
               grads=grads, none=none, buffers={k: b.cpu().numpy() for k, b in model.named_buffers()},
               hidden=[core.hidden_tensor(h).detach().cpu().numpy() for h in seen["hidden"]] if case.keep else None,
               kept=[not isinstance(h, core.ZAct) for h in seen["hidden"]], route=cut_route(case, log),
               dense=bool(bt.dense), has_bits=bool(bt.has_bits), iso=bool(bt.iso),
               need_dummy=bool(bt.maxnb.need_dummy) if sp.n_max else None)
    _RESULTS[case.id] = res
    return res


def _gmax(grads):
    m = [float(np.nanmax(np.abs(v))) for k, v in grads.items() if not k.startswith("__") and np.isfinite(v).any()]
    return max(m) if m else 0.0


def _err(what, a, ref, floor=0.0):
    """rel_err, its NaN-pattern failure naming the tensor"""
    try:
        return rel_err(a, ref, floor)
    except AssertionError as e:
        raise AssertionError("%s: %s (%d NaN of %d, the oracle %d)" % (what, e, int(np.isnan(a).sum()), np.size(a),
                                                                      int(np.isnan(ref).sum()))) from None


def record(case, rep):
    print("%-40s values %.2e (ref %.2e, bound %.1e)  grads %.2e (ref %.2e, bound %.1e)  worst: %s / %s" % (
        case.id, rep["value_err"], rep["value_ref"], rep["value_bound"], rep["grad_err"], rep["grad_ref"],
        rep["grad_bound"], rep["value_what"], rep["grad_what"]))
    if not REPORT:
        return
    try:
        os.makedirs(os.path.dirname(os.path.abspath(REPORT)), exist_ok=True)
        data = json.load(open(REPORT)) if os.path.exists(REPORT) else {}
        data[case.id] = rep
        json.dump(data, open(REPORT, "w"), indent=1)
    except OSError:
        pass


def check_values(case, res):
    ref, r32 = T.reference(case)
    flat = T.small(case)
    floor = 2e-2 * _gmax(ref["grads"])
    vals = [("c_logit", res["c_logit"], ref["c_logit"], None if r32 is None else r32["c_logit"]),
            ("d_logit", res["d_logit"], ref["d_logit"], None if r32 is None else r32["d_logit"]),
            ("loss", np.array([res["loss"]]), np.array([ref["loss"]]), None if r32 is None else np.array([r32["loss"]]))]
    for k, v in ref["buffers"].items():
        vals.append((k, res["buffers"][k], v, None if r32 is None else r32["buffers"][k]))
    v_ref = g_ref = 0.0
    if not flat:
        # the fp32 CPU restatement's own error on this case: the largest over its values, and over its gradients
        v_ref = max(rel_err(t, r) for _, _, r, t in vals)
        g_ref = max(rel_err(r32["grads"][k].reshape(np.shape(v)), v, floor) for k, v in ref["grads"].items())
        assert v_ref <= VALUE_CEILING and g_ref <= TRUE_SHAPE_GRAD_RTOL, \
            "%s: the fp32 CPU step is %.2e / %.2e from fp64: a badly conditioned case" % (case.id, v_ref, g_ref)
    v_bound, g_bound = max(RTOL, TRUE_SHAPE_FACTOR * v_ref), max(5 * RTOL, TRUE_SHAPE_FACTOR * g_ref)
    if res["hidden"] is not None:
        assert all(res["kept"])
        vals += [("hidden %d" % l, h, ref["cache"]["hidden"][l], None) for l, h in enumerate(res["hidden"])]
    errs = [(_err(what, a, r), what) for what, a, r, _ in vals]
    gerrs = []
    for name, tg in ref["grads"].items():
        assert name in res["grads"], "%s: no gradient" % name
        a = res["grads"][name]
        e = _err(name, a, np.asarray(tg).reshape(a.shape), floor)
        if not flat:
            e = min(e, rel_err(a, r32["grads"][name].reshape(a.shape), floor))
        gerrs.append((e, name))
    rep = dict(value_err=max(errs)[0], value_what=max(errs)[1], value_ref=v_ref, value_bound=v_bound,
               grad_err=max(gerrs)[0], grad_what=max(gerrs)[1], grad_ref=g_ref, grad_bound=g_bound, flat=flat,
               draw=T.case_data(case).draw, dense=res["dense"],
               route={k: (v if isinstance(v, list) else {str(kk): vv for kk, vv in v.items()})
                      for k, v in res["route"].items()})
    record(case, rep)
    for e, what in errs:
        assert e <= v_bound, "%s: %s is %.3e from the fp64 oracle > %.1e" % (case.id, what, e, v_bound)
    for e, what in gerrs:
        assert e <= g_bound, "%s: gradient %s is %.3e from the fp64 oracle > %.1e" % (case.id, what, e, g_bound)
    assert set(res["none"]) == (set() if case.eps else {"eps"}), res["none"]
    for k, b in res["buffers"].items():
        if k.endswith("num_batches_tracked"):
            assert int(b) == 1, k


def assert_same_step(a, b):
    """two routes of the same step agree with each other at the fuzz test's bounds"""
    for what in ("c_logit", "d_logit"):
        assert rel_err(a[what], b[what]) <= RTOL, what
    assert abs(a["loss"] - b["loss"]) <= RTOL * abs(b["loss"])
    floor = 2e-2 * _gmax(b["grads"])
    assert set(a["grads"]) == set(b["grads"])
    for k, v in b["grads"].items():
        e = rel_err(a["grads"][k], v, floor)
        assert e <= 5 * RTOL, "%s: %.3e between the two routes" % (k, e)
    for k, v in b["buffers"].items():
        assert rel_err(a["buffers"][k], v) <= RTOL, k


@pytest.mark.parametrize("case", T.CASES, ids=[c.id for c in T.CASES])
def test_train_step_route_and_values_vs_fp64(case):
    res = step(case)
    # what the arena decided for the batch is what the table assumed for it
    if case.npool != "max":
        assert res["dense"] == T.expected_dense(case, T.case_data(case).graphs)
        assert res["iso"] == T.has_isolated(T.case_data(case).graphs)
    if case.kind == "regular":
        assert res["need_dummy"] is False
    elif case.npool == "max":
        assert res["need_dummy"] is True
    assert_route(case, res["route"])
    check_values(case, res)
    if case.pair:
        assert_same_step(res, step(T.BY_ID[case.pair]))
