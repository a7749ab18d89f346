"""Every captured replay against the eager step, byte for byte, across the training envelope
(tests/train_envelope_cases.py: the case table, the pools and the selection sequences; the CPU half is
tests/test_replay_envelope_host.py).

Nothing here is a tolerance except the two places that say so.  A replay is compared with an eager run of the same
model, the same parameters and the same sequence of batches through tobytes(): NaN patterns and payloads count (the
all-NaN case), and so does the sign of a zero.  The sequence is the pool's: the case's own batch, a disjoint one, one
with a graph twice, the own batch again, one in descending order -- each with its own labels and permutation, and with
edge counts (nnz_max, a launch-sizing argument frozen at capture) that differ from the template's.

  a  gnm.graphs.CapturedTrainStep: on a StaticBatch, on the packed buffer through run_gids, on the packed buffer
     through run(batch): loss, logits, every gradient (or sink tensor) per step, the BatchNorm buffers at the end,
     eager_fallbacks == 0, construction without side effect
  b  gnm.train.FusedTrainStep(capture=True) against capture=False: parts, parameters and Adam state per step, through
     run() and run_gids(), set_lr half-way, weight decay
  c  the edge-count boundary: a heavier graph falls back (once, with one warning) on the StaticBatch capture and
     replays on the packed one; the next batch replays on both
  d  the reference's loop in train mode (CapturedTrain): outputs, .grad, state_dict, the numpy RNG
  e  the reference's loop in eval mode (CapturedEval) for the three eval_fused settings
  f  real dropout under replay: the masks a replay drew, and the backward reading its own forward's mask (fp64 formula,
     RTOL)
  g  the replayed step of (a) on a batch that is not the template against the fp64 oracle (RTOL / 5 RTOL)

The eager twin of (a) and (c) is CapturedTrainStep._fallback's step -- model.zero_grad(set_to_none=False), forward,
loss, backward -- after one step that leaves every .grad allocated (state put back), as the capture's warm-up does: a
backward then ADDS to a zeroed .grad on both sides (0 + -0.0 is +0.0; a fresh .grad would keep the sign).

GNM_REPLAY_ENVELOPE_REPORT names a JSON file that collects, per case and replay kind, the steps replayed, the steps
that fell back and the wall time (profiles/replay_envelope_parity.md)."""
import contextlib
import json
import os
import time
import warnings

import numpy as np
import pytest
import torch

import train_envelope_cases as T
from helpers import RTOL, fixed_dropout, rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
REPORT = os.environ.get("GNM_REPLAY_ENVELOPE_REPORT")


def _cases(kind, excluded=False):
    return [c for c in T.CASES if (T.replay_exclusion(c, kind) is not None) == excluded]


def _ids(cases):
    return [c.id for c in cases]


def bts(t):
    return None if t is None else t.detach().contiguous().cpu().numpy().tobytes()


def record(case, kind, replayed, fell_back, seconds, extra=None):
    print("%-40s %-6s replayed %2d  fell back %d  %.2f s" % (case.id, kind, replayed, fell_back, seconds))
    if not REPORT:
        return
    try:
        os.makedirs(os.path.dirname(os.path.abspath(REPORT)), exist_ok=True)
        data = json.load(open(REPORT)) if os.path.exists(REPORT) else {}
        data.setdefault(case.id, {})[kind] = dict(replayed=replayed, fell_back=fell_back, seconds=round(seconds, 3),
                                                  **(extra or {}))
        json.dump(data, open(REPORT, "w"), indent=1)
    except OSError:
        pass


def assert_same(want, got, what):
    """two lists of {name: bytes or None}, one per step"""
    assert len(want) == len(got), what
    for s, (a, b) in enumerate(zip(want, got)):
        assert set(a) == set(b), (what, s)
        for k in a:
            if a[k] != b[k]:
                if a[k] is None or b[k] is None or len(a[k]) != len(b[k]):
                    raise AssertionError("%s, step %d: %s is %s in the eager run and %s replayed" % (
                        what, s, k, "None" if a[k] is None else "%d bytes" % len(a[k]),
                        "None" if b[k] is None else "%d bytes" % len(b[k])))
                x, y = np.frombuffer(a[k], np.uint8), np.frombuffer(b[k], np.uint8)
                raise AssertionError("%s, step %d: %s differs from the eager run in %d of %d bytes" % (
                    what, s, k, int((x != y).sum()), x.size))


def make_model(case, sink=True):
    """the case's model in train mode on the GPU with the whole pool (and the heavier graph) in its arena: arena id =
    pool index.  Returns (model, the gradient sink or None)"""
    from models.graphcnn import GIN_InfoMaxReg
    d, pool = T.case_data(case), T.case_pool(case)
    dev = torch.device(DEV)
    model = GIN_InfoMaxReg(case.L, case.m, case.F0, case.H, case.C, case.drop, case.eps, case.gpool, case.npool, dev)
    model.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in d.state.items()})
    model = model.to(dev).train()
    model._spec.keep_hidden = case.keep
    s = None
    if sink and case.sink:
        s = model._spec.grad_sink = {n: torch.full_like(p, float("nan")) for n, p in model.named_parameters()}
    adopt_pool(model, pool)
    return model, s


def adopt_pool(model, pool):
    graphs = list(pool.graphs) + ([pool.heavy] if pool.heavy is not None else [])
    ids = model.arena().add_many(graphs)        # (a graph remembers the arena it was added to last)
    assert ids == list(range(len(graphs))), ids


def dropout_ctx(case):
    d = T.case_data(case)
    return fixed_dropout(d.masks, device=DEV) if d.masks is not None else contextlib.nullcontext()


def sequence(case):
    pool = T.case_pool(case)
    return [(np.asarray(pool.selections[s], dtype=np.int64), pool.labels[s], pool.perms[s]) for s in range(5)]


def template_ids(case):
    pool = T.case_pool(case)
    return np.asarray(pool.selections[pool.template], dtype=np.int64)


def state_bytes(model):
    return {k: bts(v) for k, v in model.state_dict().items()}


def make_loss(case, seen, loss=None):
    from gnm.train import infomax_loss
    F = torch.nn.functional
    N = case.B * case.n
    y = torch.cat([torch.ones(N, 1), torch.zeros(N, 1)]).to(DEV)
    kind = loss or case.loss

    def loss_fn(c_logit, d_logit, labels):
        seen["c"], seen["d"] = c_logit, d_logit             # (in a capture: the static tensors every replay rewrites)
        if kind == "infomax":
            return infomax_loss(c_logit, d_logit, labels, beta=T.BETA)[0]
        return F.cross_entropy(c_logit, labels) + T.BETA * F.binary_cross_entropy_with_logits(d_logit, y)
    return loss_fn


def snap(model, sink, loss, seen):
    torch.cuda.synchronize()
    out = {"loss": bts(loss), "c_logit": bts(seen["c"]), "d_logit": bts(seen["d"])}
    for name, p in model.named_parameters():
        out["grad " + name] = bts(sink[name] if sink is not None else p.grad)
    return out


# ------------------------------------------------------------------------------------------------- a, c, g: the step
def eager_steps(case, seq, loss=None):
    """CapturedTrainStep._fallback's step over `seq`: (per-step snapshots, buffers at the end)"""
    model, sink = make_model(case)
    arena, seen = model.arena(), {}
    loss_fn = make_loss(case, seen, loss)

    def one(ids, labels, perm):
        batch = arena.batch_from_gids(ids)
        model.zero_grad(set_to_none=False)
        X = None if case.p0 else arena.features(batch)
        c_logit, d_logit = model.forward_batch(batch, X=X, perm=perm)
        ls = loss_fn(c_logit, d_logit, torch.as_tensor(labels).to(DEV))
        ls.backward()
        return ls
    snaps = []
    with dropout_ctx(case):
        keep = [t for t in model.state_dict().values()]
        saved = [t.clone() for t in keep]
        one(*seq[0])                                # leaves every .grad allocated, like the capture's warm-up steps
        with torch.no_grad():
            for t, s0 in zip(keep, saved):
                t.copy_(s0)
        for ids, labels, perm in seq:
            snaps.append(snap(model, sink, one(ids, labels, perm), seen))
    return snaps, {k: bts(b) for k, b in model.named_buffers()}


FORMS = ("static", "gids", "packed-run")


def captured_steps(case, form, seq, loss=None, expect_fallbacks=0):
    """the same steps from a CapturedTrainStep: (snapshots, buffers at the end, the capture)"""
    from gnm.graphs import CapturedTrainStep
    model, sink = make_model(case)
    arena, seen = model.arena(), {}
    loss_fn = make_loss(case, seen, loss)
    tids = template_ids(case)
    before = state_bytes(model)
    snaps = []
    with dropout_ctx(case):
        cap = CapturedTrainStep(model, arena.batch_from_gids(tids), loss_fn, agg0_cache=case.p0,
                                gids_host=None if form == "static" else tids)
        assert (cap.packed is None) == (form == "static")
        # the layer-0 cache switched off: the step aggregates the input features itself and no cache is ever built
        assert case.p0 or not arena._agg0, "%s: agg0_cache=False and the capture built the layer-0 cache" % case.id
        assert state_bytes(model) == before, "%s: constructing the %s capture changed the model's state" % (case.id, form)
        static = dict(seen)                 # the captured logits; a step that falls back leaves eager ones in `seen`
        for ids, labels, perm in seq:
            n_eager = cap.eager_fallbacks
            if form == "gids":
                ls = cap.run_gids(ids, labels, perm)
            else:
                ls = cap.run(arena.batch_from_gids(ids), torch.as_tensor(labels).to(DEV), perm)
            snaps.append(snap(model, sink, ls, seen if cap.eager_fallbacks > n_eager else static))
    assert cap.eager_fallbacks == expect_fallbacks, (case.id, form, cap.eager_fallbacks)
    return snaps, {k: bts(b) for k, b in model.named_buffers()}, cap


_STATIC = {}          # ANCHOR_CASES id -> the StaticBatch form's snapshots over the pool's sequence: (g) reads them


@pytest.mark.parametrize("case", _cases("step"), ids=_ids(_cases("step")))
def test_captured_train_step_equals_eager_bitwise(case):
    seq = sequence(case)
    want, want_buf = eager_steps(case, seq)
    for form in FORMS:
        t0 = time.perf_counter()
        got, got_buf, cap = captured_steps(case, form, seq)
        dt = time.perf_counter() - t0
        if form == "static" and case.id in T.ANCHOR_CASES:
            _STATIC[case.id] = got
        assert_same(want, got, "%s, CapturedTrainStep (%s)" % (case.id, form))
        assert_same([want_buf], [got_buf], "%s, CapturedTrainStep (%s), buffers" % (case.id, form))
        record(case, "step/" + form, len(seq) - cap.eager_fallbacks, cap.eager_fallbacks, dt)
    nbt = [k for k in want_buf if k.endswith("num_batches_tracked")]
    assert nbt and all(np.frombuffer(got_buf[k], np.int64)[0] == len(seq) for k in nbt)


@pytest.mark.parametrize("id_", ["agg-csr-H64", "lin-rz-wide-H64-m2"])
def test_edge_count_boundary_falls_back_once_and_leaves_no_stale_state(id_):
    case, pool = T.BY_ID[id_], T.case_pool(T.BY_ID[id_])
    base = sequence(case)
    heavy = np.asarray((len(pool.graphs),) + pool.selections[1][1:], dtype=np.int64)
    seq = [base[0], (heavy, base[1][1], base[1][2]), base[1], base[4]]
    want, want_buf = eager_steps(case, seq)
    with pytest.warns(RuntimeWarning, match="runs eagerly") as rec:
        got, got_buf, cap = captured_steps(case, "static", seq, expect_fallbacks=1)
    assert len([w for w in rec if "runs eagerly" in str(w.message)]) == 1
    assert_same(want, got, "%s, StaticBatch capture across the edge-count boundary" % id_)
    assert_same([want_buf], [got_buf], "%s, buffers" % id_)
    for form in ("gids", "packed-run"):
        with warnings.catch_warnings():
            warnings.simplefilter("error", RuntimeWarning)
            got, got_buf, cap = captured_steps(case, form, seq, expect_fallbacks=0)
        assert_same(want, got, "%s, packed capture (%s) across the edge-count boundary" % (id_, form))
        assert_same([want_buf], [got_buf], "%s, buffers" % id_)


@pytest.mark.parametrize("id_", T.ANCHOR_CASES)
def test_replayed_step_on_another_batch_vs_fp64(id_):
    """the replay of (a) on the anchor selection (train_envelope_cases.anchor: selection 1, or the first later one
    that keeps the ReLU margin) against OracleGIN.train_step_grads on that selection: the fuzz bounds of the train
    envelope's small cases, RTOL for values and 5 RTOL for gradients with the 2e-2 gmax floor"""
    case = T.BY_ID[id_]
    s, ref = T.anchor(id_)
    if id_ not in _STATIC:
        _STATIC[id_] = captured_steps(case, "static", sequence(case))[0]
    got = _STATIC[id_][s]
    f32 = lambda k, like: np.frombuffer(got[k], np.float32).reshape(np.shape(like))         # noqa: E731
    errs = {"c_logit": rel_err(f32("c_logit", ref["c_logit"]), ref["c_logit"]),
            "d_logit": rel_err(f32("d_logit", ref["d_logit"]), ref["d_logit"]),
            "loss": abs(float(np.frombuffer(got["loss"], np.float32)[0]) - ref["loss"]) / abs(ref["loss"])}
    gmax = max(float(np.max(np.abs(v))) for v in ref["grads"].values())
    gerrs = {}
    for name, tg in ref["grads"].items():
        assert got["grad " + name] is not None, name
        gerrs[name] = rel_err(f32("grad " + name, tg), np.asarray(tg), 2e-2 * gmax)
    worst_v, worst_g = max(errs, key=errs.get), max(gerrs, key=gerrs.get)
    print("%s: selection %d  values %.2e (%s, bound %.0e)  gradients %.2e (%s, bound %.0e)" % (
        id_, s, errs[worst_v], worst_v, RTOL, gerrs[worst_g], worst_g, 5 * RTOL))
    record(case, "fp64", 1, 0, 0.0, dict(selection=s, value_err=errs[worst_v], value_what=worst_v, value_bound=RTOL,
                                         grad_err=gerrs[worst_g], grad_what=worst_g, grad_bound=5 * RTOL))
    for k, e in errs.items():
        assert e <= RTOL, "%s: %s of the replayed step is %.3e from the fp64 oracle" % (id_, k, e)
    for k, e in gerrs.items():
        assert e <= 5 * RTOL, "%s: gradient %s of the replayed step is %.3e from the fp64 oracle" % (id_, k, e)


# ------------------------------------------------------------------------------------------------- b: FusedTrainStep
LR = (0.01, 0.003, 0.0005)


def fused_walk(case, capture, wd):
    """the sequence through run(), then again through run_gids() (the eager twin: run() both times), set_lr after the
    second step of each walk: (snapshots, buffers, the step object)"""
    from gnm.train import FusedTrainStep
    model, _ = make_model(case, sink=False)
    arena = model.arena()
    tids = template_ids(case)
    before = state_bytes(model)
    snaps = []
    with dropout_ctx(case):
        step = FusedTrainStep(model, lr=LR[0], beta=T.BETA, weight_decay=wd, capture=capture,
                              template_batch=arena.batch_from_gids(tids) if capture else None,
                              template_gids=tids if capture else None)
        opt = step.optimizer
        torch.cuda.synchronize()
        assert state_bytes(model) == before, "%s: constructing FusedTrainStep changed the model's state" % case.id
        assert not bool(opt.exp_avg.any()) and not bool(opt.exp_avg_sq.any()) and int(opt.step_count.item()) == 0
        assert opt.hyper.cpu().tolist() == [LR[0], 0.9, 0.999, 1e-8, wd, 1.0]
        for walk in range(2):
            for k, (ids, labels, perm) in enumerate(sequence(case)):
                if capture and walk == 1:
                    parts = step.run_gids(ids, labels, perm)
                else:
                    parts = step.run(arena.batch_from_gids(ids), torch.as_tensor(labels).to(DEV), perm)
                torch.cuda.synchronize()
                snaps.append({"parts": bts(parts), "flat": bts(step.dp.fp.flat), "exp_avg": bts(opt.exp_avg),
                              "exp_avg_sq": bts(opt.exp_avg_sq), "step_count": bts(opt.step_count)})
                if k == 1:
                    opt.set_lr(LR[1 + walk])            # (the StepLR path) ... and the kernel's copy follows
                    assert opt.hyper.cpu().tolist()[0] == LR[1 + walk] == opt.lr
    return snaps, {k: bts(b) for k, b in model.named_buffers()}, step


@pytest.mark.parametrize("case", _cases("fused"), ids=_ids(_cases("fused")))
def test_fused_train_step_captured_equals_eager_bitwise(case):
    wd = 0.01 if T.CASES.index(case) % 3 == 1 else 0.0
    want, want_buf, _ = fused_walk(case, False, wd)
    t0 = time.perf_counter()
    got, got_buf, step = fused_walk(case, True, wd)
    dt = time.perf_counter() - t0
    assert step.captured.packed is not None
    assert_same(want, got, "%s, FusedTrainStep(capture=True), weight_decay %g" % (case.id, wd))
    assert_same([want_buf], [got_buf], "%s, FusedTrainStep, buffers" % case.id)
    assert step.captured.eager_fallbacks == 0
    assert int(step.optimizer.step_count.item()) == 10
    record(case, "fused", 10, step.captured.eager_fallbacks, dt, dict(weight_decay=wd))


def test_fused_train_step_refuses_neighbour_max():
    from gnm.train import FusedTrainStep
    case = T.BY_ID["max-H64-eps0-gavg-padded"]
    assert T.replay_exclusion(case, "fused")
    model, _ = make_model(case, sink=False)
    tids = template_ids(case)
    with pytest.raises(RuntimeError, match="neighbour lists"):
        FusedTrainStep(model, lr=0.01, beta=T.BETA, capture=True, template_batch=model.arena().batch_from_gids(tids),
                       template_gids=tids)


# ------------------------------------------------------------------------------------------------- d: CapturedTrain
ACCUMULATE = ("lin-rz-wide-H64-m2", "agg-dir-csr-H64")


def reference_loop(case, replay, zero_every):
    """the reference's train() body over the selection sequence, torch's own losses and Adam"""
    pool = T.case_pool(case)
    model, _ = make_model(case)
    model.train_replay = replay
    dev = torch.device(DEV)
    opt = torch.optim.Adam(model.parameters(), lr=0.01)
    ce, bce = torch.nn.CrossEntropyLoss(), torch.nn.BCEWithLogitsLoss()
    N = case.B * case.n
    d_lab = torch.cat([torch.ones(N, 1), torch.zeros(N, 1)], 0).to(dev)
    np.random.seed(11)
    snaps = []
    with dropout_ctx(case):
        for s, ids in enumerate(pool.selections):
            batch = [pool.graphs[j] for j in ids]
            c_logit, d_logit = model(batch)
            loss = ce(c_logit, torch.as_tensor(pool.labels[s]).to(dev)) + T.BETA * bce(d_logit, d_lab)
            if s % zero_every == 0:
                opt.zero_grad()
            loss.backward()
            torch.cuda.synchronize()
            out = {"c_logit": bts(c_logit), "d_logit": bts(d_logit), "loss": bts(loss)}
            for name, p in model.named_parameters():
                out["grad " + name] = bts(p.grad)
            snaps.append(out)
            if s % zero_every == zero_every - 1:
                opt.step()
    rng = np.random.get_state()
    return snaps, state_bytes(model), (rng[0], rng[1].tobytes(), rng[2:]), model


@pytest.mark.parametrize("case", _cases("train"), ids=_ids(_cases("train")))
def test_reference_loop_train_replay_equals_eager_bitwise(case):
    zero_every = 2 if case.id in ACCUMULATE else 1
    want, want_state, want_rng, _ = reference_loop(case, False, zero_every)
    t0 = time.perf_counter()
    got, got_state, got_rng, model = reference_loop(case, True, zero_every)
    dt = time.perf_counter() - t0
    assert model.train_replay is True, "the capture failed and the model switched train replay off"
    assert len(model._train_cache) == 1
    cap = next(iter(model._train_cache.values()))
    assert cap.gen == 5, "%d of 5 forwards replayed" % cap.gen
    assert_same(want, got, "%s, model(batch) in train mode" % case.id)
    assert_same([want_state], [got_state], "%s, state_dict after the loop" % case.id)
    assert want_rng == got_rng
    record(case, "train", cap.gen, 5 - cap.gen, dt, dict(zero_every=zero_every))


@pytest.mark.parametrize("case", [c for c in _cases("train", excluded=True) if c.npool != "max"],
                         ids=_ids([c for c in _cases("train", excluded=True) if c.npool != "max"]))
def test_reference_loop_declines_what_the_table_excludes(case):
    """keep_hidden and an installed gradient sink: no capture is made, and the loop gives the eager results"""
    want, want_state, want_rng, _ = reference_loop(case, False, 1)
    got, got_state, got_rng, model = reference_loop(case, True, 1)
    assert not model._train_cache, T.replay_exclusion(case, "train")
    assert_same(want, got, case.id)
    assert_same([want_state], [got_state], case.id)
    assert want_rng == got_rng


@pytest.mark.parametrize("case", [c for c in T.CASES if c.npool == "max"], ids=_ids([c for c in T.CASES if c.npool == "max"]))
def test_reference_loop_never_captures_neighbour_max(case):
    want, want_state, want_rng, _ = reference_loop(case, False, 1)
    got, got_state, got_rng, model = reference_loop(case, True, 1)
    assert not model._train_cache and not model._eval_cache, T.replay_exclusion(case, "train")
    assert_same(want, got, case.id)
    assert_same([want_state], [got_state], case.id)
    assert want_rng == got_rng


# ------------------------------------------------------------------------------------------------- e: CapturedEval
def eval_walk(case, replay):
    pool = T.case_pool(case)
    model, _ = make_model(case, sink=False)
    model._spec.keep_hidden = False
    model.eval()
    model.eval_replay = replay
    out = []
    np.random.seed(5)
    forwards = 0
    with torch.no_grad():
        for fused in ("layers", True, False):
            model.eval_fused = fused
            for s, ids in enumerate(pool.selections):
                for batch in ([pool.graphs[j] for j in ids], [pool.graphs[ids[-1]]]):
                    c_logit, d_logit = model(batch)
                    lat = model(batch, latent=True)
                    forwards += 2
                    torch.cuda.synchronize()
                    out.append({"c_logit": bts(c_logit), "d_logit": bts(d_logit),
                                "latent": np.ascontiguousarray(lat).tobytes()})
                if s == 1:
                    for p in model.parameters():
                        p.mul_(1.01)
    rng = np.random.get_state()
    return out, (rng[0], rng[1].tobytes(), rng[2:]), forwards, model


@pytest.mark.parametrize("case", _cases("eval"), ids=_ids(_cases("eval")))
def test_reference_loop_eval_replay_equals_eager_bitwise(case, monkeypatch):
    from gnm import graphs as G
    calls = []
    real = G.CapturedEval.run
    monkeypatch.setattr(G.CapturedEval, "run", lambda self, gh, perm: (calls.append(1), real(self, gh, perm))[1])
    want, want_rng, _, _ = eval_walk(case, False)
    assert not calls
    t0 = time.perf_counter()
    got, got_rng, forwards, model = eval_walk(case, True)
    dt = time.perf_counter() - t0
    assert model.eval_replay is True, "the capture failed and the model switched eval replay off"
    assert len(calls) == forwards == 60, "%d of %d eval forwards replayed" % (len(calls), forwards)
    assert_same(want, got, "%s, model(batch) in eval mode" % case.id)
    assert want_rng == got_rng
    record(case, "eval", len(calls), forwards - len(calls), dt)


# ------------------------------------------------------------------------------------------------- f: real dropout
DROPOUT_CASES = ("head-C256-drop", "pool-H64-nsum-gsum-eps1")
REPLAYS = 8


def _check_masks(case, masks):
    """masks: the [L, B, C] mask of each of the 8 replays"""
    p = case.drop
    scale = np.float32(1.0 / (1.0 - p))
    allm = np.stack(masks)
    assert ((allm == 0) | (allm == scale)).all(), "a mask entry is neither 0 nor 1 / (1 - p)"
    assert sum(not np.array_equal(m, masks[0]) for m in masks[1:]) >= 7, "replays repeat the first mask"
    # the keep rate over all replays: a binomial of allm.size draws
    sd = float(np.sqrt(p * (1 - p) / allm.size))
    rate = float((allm != 0).mean())
    assert abs(rate - (1 - p)) <= 5 * sd, "keep rate %.4f, expected %.2f +- %.4f" % (rate, 1 - p, 5 * sd)


def _check_bias_grads(case, mask, dC, grads, what):
    """grad linears_prediction.l.bias == sum_b mask[l, b, :] dC[b, :], in fp64 from this replay's mask"""
    for l in range(case.L):
        ref = (mask[l].astype(np.float64) * dC.astype(np.float64)).sum(0)
        got = grads["linears_prediction.%d.bias" % l]
        # relative to the largest entry; a layer whose mask dropped every logit (0.4^4 at B = C = 2) has none: the
        # largest single product then
        scale = float(np.max(np.abs(ref))) or float(np.max(np.abs(dC))) / (1.0 - case.drop)
        e = float(np.max(np.abs(got - ref)) / scale)
        assert e <= RTOL, "%s: the gradient of linears_prediction.%d.bias is %.2e from its own forward's mask" % (
            what, l, e)


@contextlib.contextmanager
def dropout_spy(holder):
    F = torch.nn.functional
    orig = F.dropout

    def spy(x, p=0.5, training=True, inplace=False):
        holder["mask"] = orig(x, p, training, inplace)       # (captured: the tensor every replay's draw lands in)
        return holder["mask"]
    F.dropout = spy
    try:
        yield
    finally:
        F.dropout = orig


@pytest.mark.parametrize("id_", DROPOUT_CASES)
def test_real_dropout_under_captured_train(id_):
    case, pool = T.BY_ID[id_], T.case_pool(T.BY_ID[id_])
    model, _ = make_model(case)
    torch.manual_seed(1234)
    np.random.seed(3)
    holder, masks = {}, []
    batch = [pool.graphs[j] for j in pool.selections[0]]
    labels = torch.as_tensor(pool.labels[0]).to(DEV)
    d_lab = torch.cat([torch.ones(case.B * case.n, 1), torch.zeros(case.B * case.n, 1)], 0).to(DEV)
    with dropout_spy(holder):
        for r in range(REPLAYS):
            model.zero_grad()
            c_logit, d_logit = model(batch)
            c_logit.retain_grad()
            loss = torch.nn.functional.cross_entropy(c_logit, labels) + \
                T.BETA * torch.nn.functional.binary_cross_entropy_with_logits(d_logit, d_lab)
            loss.backward()
            torch.cuda.synchronize()
            mask = holder["mask"].detach().cpu().numpy().copy()
            masks.append(mask)
            grads = {k: p.grad.detach().cpu().numpy() for k, p in model.named_parameters() if "prediction" in k}
            _check_bias_grads(case, mask, c_logit.grad.cpu().numpy(), grads, "%s, CapturedTrain, replay %d" % (id_, r))
    cap = next(iter(model._train_cache.values()))
    assert len(model._train_cache) == 1 and cap.gen == REPLAYS
    _check_masks(case, masks)


@pytest.mark.parametrize("id_", DROPOUT_CASES)
def test_real_dropout_under_captured_train_step(id_):
    from gnm.graphs import CapturedTrainStep
    case, pool = T.BY_ID[id_], T.case_pool(T.BY_ID[id_])
    model, _ = make_model(case)
    arena = model.arena()
    torch.manual_seed(4321)
    holder, seen, masks = {}, {}, []
    tids = template_ids(case)
    ids, labels, perm = sequence(case)[0]
    with dropout_spy(holder):
        cap = CapturedTrainStep(model, arena.batch_from_gids(tids), make_loss(case, seen, "infomax"), gids_host=tids)
        for r in range(REPLAYS):
            cap.run_gids(ids, labels, perm)
            torch.cuda.synchronize()
            mask = holder["mask"].detach().cpu().numpy().copy()
            masks.append(mask)
            # the fused loss: dC = (softmax(c_logit) - onehot(labels)) / B
            z = seen["c"].detach().cpu().numpy().astype(np.float64)
            e = np.exp(z - z.max(1, keepdims=True))
            dC = e / e.sum(1, keepdims=True)
            dC[np.arange(case.B), labels] -= 1.0
            dC /= case.B
            grads = {k: p.grad.detach().cpu().numpy() for k, p in model.named_parameters() if "prediction" in k}
            _check_bias_grads(case, mask, dC, grads, "%s, CapturedTrainStep, replay %d" % (id_, r))
    assert cap.eager_fallbacks == 0
    _check_masks(case, masks)
