"""CPU-only checks of host logic added in round 2 (no device compute): the per-device launch-configuration
guard, KernelTimer bookkeeping when a fused entry point declines a shape, device selection for launches,
gradient-view re-attachment of the data-parallel wrapper under a stock torch optimizer, constructor shape limits."""
import numpy as np
import pytest
import torch

from helpers import load_case


def test_per_device_configure_once_guard():
    """hipFuncSetAttribute(MaxDynamicSharedMemorySize) is per (kernel, device): the guard every launcher keeps must
    fire once PER DEVICE, not once per process (a second GPU driven from the same process would otherwise launch
    its > 64 KB-LDS kernels unconfigured)."""
    from gnm._cabi import lib
    assert lib.gnm_debug_device_once(0, 1) == 1        # device 0, first use
    assert lib.gnm_debug_device_once(0, 0) == 0
    assert lib.gnm_debug_device_once(1, 0) == 1        # device 1 in the same process: configured on its own
    assert lib.gnm_debug_device_once(1, 0) == 0
    assert lib.gnm_debug_device_once(0, 0) == 0
    assert lib.gnm_debug_device_once(63, 0) == 1
    assert lib.gnm_debug_device_once(64, 0) == 1       # outside the table: never cached, always (re)configured
    assert lib.gnm_debug_device_once(64, 0) == 1
    assert lib.gnm_debug_device_once(-1, 0) == 1
    assert lib.gnm_debug_device_once(0, 1) == 1        # reset forgets


class _FakeEvent:
    clock = 0.0

    def record(self):
        self.t = _FakeEvent.clock

    def elapsed_time(self, other):
        return other.t - self.t


def test_kernel_timer_ignores_declined_fused_call(monkeypatch):
    """The unsupported-then-fallback sequence of encoder_forward: gnm_agg_fwd_bnrelu returns -2 without
    launching, then gnm_agg runs.  Only the launch that happened may be timed, with its own meta (round 1
    averaged an empty interval in and kept the fused label: a 2x inflated roofline for F != 64)."""
    from gnm import core
    monkeypatch.setattr(core, "_new_event", _FakeEvent)
    timer = core.KernelTimer(("agg_fwd_F128",))
    monkeypatch.setattr(core, "TIMER", timer)
    for _ in range(3):
        with core._timed("agg_fwd_F128", F=128, B=256, N=256000, fused_bnrelu=1) as tm:
            rc = -2                                       # declined: nothing launched
            if rc != 0:
                tm.cancel()
        with core._timed("agg_fwd_F128", F=128, B=256, N=256000):
            _FakeEvent.clock += 0.177                     # the real launch
        with core._timed("lin_fwd_K128_H128", N=1):       # not selected by the prefixes
            _FakeEvent.clock += 1.0
    summ = timer.summary()
    assert list(summ) == ["agg_fwd_F128"]
    c, ms, meta = summ["agg_fwd_F128"]
    assert c == 3 and abs(ms - 0.177) < 1e-9
    assert "fused_bnrelu" not in meta

    # a block that raises records nothing either
    with pytest.raises(RuntimeError):
        with core._timed("agg_fwd_F128", F=128, B=1, N=1):
            raise RuntimeError("launch failed")
    assert timer.summary()["agg_fwd_F128"][0] == 3

    # launches of the same tag but different kernels (meta) are reported apart, never averaged together
    with core._timed("agg_fwd_F128", F=128, B=256, N=256000, fused_bnrelu=1):
        _FakeEvent.clock += 0.5
    summ = timer.summary()
    assert set(summ) == {"agg_fwd_F128|", "agg_fwd_F128|fused_bnrelu=1"}
    assert summ["agg_fwd_F128|"][0] == 3 and abs(summ["agg_fwd_F128|fused_bnrelu=1"][1] - 0.5) < 1e-9


class _FakeTensor:
    def __init__(self, device):
        self.device = torch.device(device)
        self.is_cuda = self.device.type == "cuda"


def test_launch_device_selection():
    """Kernels are launched on the stream of the device the TENSORS live on (not torch's current device);
    CPU tensors and replicas spread over two devices are refused before any pointer reaches the library."""
    from gnm import core
    from gnm._cabi import GnmError
    assert core.launch_device(_FakeTensor("cuda:1"), None, _FakeTensor("cuda:1")) == torch.device("cuda:1")
    with pytest.raises(GnmError, match="GPU only"):
        core.launch_device(torch.zeros(1))
    with pytest.raises(GnmError, match="different devices"):
        core.launch_device(_FakeTensor("cuda:0"), _FakeTensor("cuda:1"))
    with pytest.raises(GnmError):
        core.launch_device(None)


def test_direct_grad_sink_survives_stock_optimizer_zero_grad():
    """DataParallelGIN in direct mode + torch.optim.Adam, the multi-GPU recipe of INTEGRATION.md:
    optimizer.zero_grad() (set_to_none=True by default) detaches the flat-buffer views; the sink backward hands
    autograd None, so without re-attachment Adam silently skips every parameter."""
    from gnm.parallel import DataParallelGIN
    from models.graphcnn import GIN_InfoMaxReg
    cfg, state, d = load_case("tiny_s1_eps1_gsum_nsum")
    torch.manual_seed(0)
    model = GIN_InfoMaxReg(cfg["L"], cfg["m"], cfg["f0"], cfg["H"], cfg["C"], 0.0, True, "sum", "sum",
                           torch.device("cpu"))
    dp = DataParallelGIN(model)
    assert dp.direct
    opt = torch.optim.Adam(model.parameters(), lr=1e-2)
    for how in ("dp.zero_grad", "allreduce_only", "module.zero_grad"):
        opt.zero_grad()                                   # grads -> None
        assert all(p.grad is None for p in model.parameters())
        if how == "module.zero_grad":
            model.zero_grad()                             # what compute_saliency does (graphcnn.py:256)
        if how != "allreduce_only":
            dp.zero_grad()
            off = 0
            for p in model.parameters():
                assert p.grad is not None and p.grad.data_ptr() == dp.fp.flat_grad.data_ptr() + 4 * off
                off += p.numel()
        # the HIP backward writes every gradient straight into the sink (= views of the flat buffer)
        for name, t in model._spec.grad_sink.items():
            t.fill_(0.25)
        dp.allreduce_gradients()                          # world 1: only re-attaches
        before = dp.fp.flat.clone()
        opt.step()
        moved = (dp.fp.flat - before).abs()
        assert float(moved.min()) > 0, how                # EVERY parameter took a step
    # non-direct mode: zero_grad zeroes and re-attaches
    model2 = GIN_InfoMaxReg(cfg["L"], cfg["m"], cfg["f0"], cfg["H"], cfg["C"], 0.0, True, "sum", "sum",
                            torch.device("cpu"))
    dp2 = DataParallelGIN(model2, direct_grads=False)
    for p in model2.parameters():
        p.grad = None
    dp2.fp.flat_grad.fill_(3.0)
    dp2.zero_grad()
    assert float(dp2.fp.flat_grad.abs().max()) == 0.0 and all(p.grad is not None for p in model2.parameters())


def test_constructor_rejects_shapes_outside_the_kernels():
    from gnm._cabi import lib
    from models.graphcnn import GIN_InfoMaxReg
    cpu = torch.device("cpu")
    assert lib.gnm_linear_max_k(64) == 448 and lib.gnm_linear_max_k(128) == 192 and lib.gnm_linear_max_k(129) == 0
    GIN_InfoMaxReg(5, 2, 400, 64, 2, 0.5, True, "sum", "sum", cpu)          # the reference's one_hot default fits
    for bad in (dict(hidden_dim=130), dict(hidden_dim=256), dict(hidden_dim=0), dict(num_layers=17),
                dict(input_dim=449), dict(input_dim=400, hidden_dim=128)):
        kw = dict(num_layers=5, input_dim=7, hidden_dim=64)
        kw.update(bad)
        with pytest.raises(ValueError):
            GIN_InfoMaxReg(kw["num_layers"], 2, kw["input_dim"], kw["hidden_dim"], 2, 0.5, True, "sum", "sum", cpu)
    # "max" neighbour pooling runs through the same Linear / BatchNorm kernels: same limits
    with pytest.raises(ValueError):
        GIN_InfoMaxReg(2, 2, 7, 130, 2, 0.5, True, "sum", "max", cpu)
    GIN_InfoMaxReg(2, 2, 7, 64, 2, 0.5, True, "sum", "max", cpu)


def test_bench_self_launches_its_ranks():
    """`python bench.py --gpus 2` with no launcher around it must start its own ranks (round 1 exited with a usage
    message, so the driver's N > 1 form could never run).  --selftest-launch stops after the rendezvous: gloo,
    one all-reduce, rank 0's JSON line relayed through the parent -- no GPU involved."""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--selftest-launch"],
                       capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    out = json.loads(lines[0])
    assert out["n_gpus"] == 2 and out["rank_sum"] == 3.0
    # a world size that contradicts --gpus is an error, not a silent single-rank run
    env2 = dict(env, RANK="0", WORLD_SIZE="1", LOCAL_RANK="0")
    r2 = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--selftest-launch"],
                        capture_output=True, text=True, timeout=120, env=env2)
    assert r2.returncode != 0 and "WORLD_SIZE" in (r2.stderr + r2.stdout)


def test_add_many_equals_add_and_symmetry_check():
    """One-upload bulk insertion gives the same arena as per-graph add(); the O(E) double-transpose symmetry
    test agrees with the definition (edge multiset of A == of A^T), duplicates included."""
    from gnm._cabi import lib
    from gnm.arena import GraphArena
    from gnm import synth
    gs = [synth.dense_fc_graph(i, n=40, t=32, f0=3) for i in range(40)]
    # two asymmetric graphs: a one-way edge, and a duplicated edge whose reverse is single
    e = gs[5].edge_mat.numpy().copy(); gs[5].edge_mat = torch.from_numpy(np.concatenate([e, [[0], [7]]], 1))
    e = gs[9].edge_mat.numpy().copy(); gs[9].edge_mat = torch.from_numpy(np.concatenate([e, e[:, :1]], 1))
    a1, a2 = GraphArena("cpu"), GraphArena("cpu")
    ids1 = [a1.add(g) for g in gs]
    for g in gs:
        g._gnm_cache = None
    ids2 = a2.add_many(gs, threads=4)
    assert ids1 == ids2 == list(range(40))
    assert a2.add_many(gs) == ids2                                   # cached: nothing is added twice
    assert len(a2) == 40
    for f in ("n", "nnz", "sym", "rp_off", "col_off", "t_rp_off", "t_col_off", "feat_off"):
        assert getattr(a1, f) == getattr(a2, f), f
    assert a1.sym.count(False) == 2 and not a1.sym[5] and not a1.sym[9]
    assert torch.equal(a1.rowptr.buf[:a1.rowptr.size], a2.rowptr.buf[:a2.rowptr.size])
    assert torch.equal(a1.col.buf[:a1.col.size], a2.col.buf[:a2.col.size])
    assert torch.equal(a1.feat.buf[:a1.feat.size], a2.feat.buf[:a2.feat.size])
    # brute-force definition on small random multigraphs
    rng = np.random.default_rng(3)
    for trial in range(200):
        n = int(rng.integers(1, 7))
        A = rng.integers(0, 3, (n, n))
        if trial % 2:
            A = A + A.T
        src, dst = np.nonzero(A)
        em = np.stack([np.repeat(src, A[src, dst]), np.repeat(dst, A[src, dst])]).astype(np.int64)
        E = em.shape[1]
        rp = np.empty(n + 1, np.int32); col = np.empty(max(E, 1), np.uint16)
        assert lib.gnm_csr_from_edge_mat(np.ascontiguousarray(em).ctypes.data, E, n, rp.ctypes.data, col.ctypes.data) == 0
        assert bool(lib.gnm_csr_is_symmetric(rp.ctypes.data, col.ctypes.data, n)) == bool((A == A.T).all()), A



def test_choose_launch_mode_trial_logic():
    """bench.py's N > 1 launch-mode trial (gnm.parallel.choose_launch_mode): fastest wins, ties go to the earlier
    candidate, a candidate that raises (a captured collective failing at replay) or returns garbage is dropped,
    nothing measurable raises."""
    from gnm.parallel import choose_launch_mode
    t = {"graph+cc": 2.0e-3, "graph": 2.2e-3, "eager": 4.0e-3}
    calls = []

    def measure(name):
        calls.append(name)
        return t[name]
    assert choose_launch_mode(["graph+cc", "graph", "eager"], measure) == ("graph+cc", t)
    assert calls == ["graph+cc", "graph", "eager"]            # every candidate measured once, in order
    t2 = dict(t, eager=1.0e-3)
    assert choose_launch_mode(["graph+cc", "graph", "eager"], lambda n: t2[n])[0] == "eager"
    assert choose_launch_mode(["graph", "eager"], lambda n: 1.0)[0] == "graph"                     # tie -> preference order

    def flaky(name):
        if name == "graph+cc":
            raise RuntimeError("captured collective failed at replay")
        return float("nan") if name == "graph" else 3.0e-3
    mode, times = choose_launch_mode(["graph+cc", "graph", "eager"], flaky)
    assert mode == "eager" and list(times) == ["eager"]
    with pytest.raises(RuntimeError):
        choose_launch_mode(["graph"], lambda n: (_ for _ in ()).throw(ValueError("x")))
    # a candidate that failed on ANOTHER rank is dropped here as well (agree = MIN over the ranks of the success flag),
    # the exception text is kept, and a GPU fault is not swallowed
    errs = {}
    mode, times = choose_launch_mode(["graph+cc", "graph", "eager"], flaky, agree=lambda ok: ok, errors=errs)
    assert mode == "eager" and "captured collective failed" in errs["graph+cc"]
    veto = iter([False, True, True])
    mode, times = choose_launch_mode(["graph+cc", "graph", "eager"], lambda n: 1e-3, agree=lambda ok: ok and next(veto))
    assert mode == "graph" and "graph+cc" not in times
    with pytest.raises(RuntimeError, match="Memory access fault"):
        choose_launch_mode(["graph", "eager"], lambda n: (_ for _ in ()).throw(RuntimeError("Memory access fault by GPU")))


def test_allreduce_gradients_is_a_mean_and_a_noop_for_one_rank():
    """world size 1: no collective, the flat buffer is untouched (and .grad views are re-attached)."""
    import torch
    from gnm.parallel import DataParallelGIN
    lin = torch.nn.Linear(3, 2)
    dp = DataParallelGIN(lin, direct_grads=False)
    dp.zero_grad()
    lin.weight.grad.fill_(2.0)
    lin.weight.grad = None
    assert dp.allreduce_gradients() is None and dp.world == 1
    assert lin.weight.grad is not None and float(lin.weight.grad.sum()) == 12.0


def test_tile_to_wave_map_of_the_linear_kernels_is_a_bijection():
    """csrc/linear.hip lin_first_tile (balanced numbering of the waves that walk the 32-row tiles with a stride of all
    active waves): for every launch shape each index below 4 x rows belongs to exactly one (workgroup, wave) -- a tile
    nobody takes would be a block of rows left unwritten, a tile taken twice a data race -- and on full launches the first
    `nwg` indices fall on `nwg` different workgroups (what the numbering is for)."""
    from gnm._cabi import lib
    f = lib.gnm_debug_lin_first_tile
    for groups in (1, 2, 3):
        for rows in list(range(1, 14)) + [255, 256, 512, 767, 768]:
            nwg = (rows + groups - 1) // groups
            seen = {}
            for b in range(nwg):
                for wave in range(4 * groups):
                    t = f(wave, groups, rows, nwg, b)
                    active = (b * groups + wave // 4) < rows
                    if not active:
                        assert t >= 4 * rows, (groups, rows, b, wave, t)      # takes no tile
                        continue
                    assert 0 <= t < 4 * rows and t not in seen, (groups, rows, b, wave, t, seen.get(t))
                    seen[t] = (b, wave)
            assert len(seen) == 4 * rows
            if rows == groups * nwg and nwg > 1:
                assert len({seen[t][0] for t in range(nwg)}) == nwg



# the aggregation entries by form: (matrix-core, CSR)
_AGG_ENTRIES = {"plain": ("gnm_aggm", "gnm_agg"), "fwd_bnrelu": ("gnm_aggm_fwd_bnrelu", "gnm_agg_fwd_bnrelu"),
                "bwd_stats": ("gnm_aggm_bwd_stats", "gnm_agg_bwd_stats")}
_STREAM = 4242


def _fake_agg_batch(dense, iso):
    """an arena batch on CPU tensors, every pointer the kernels take distinct"""
    from types import SimpleNamespace
    from gnm.arena import Batch, BatchClass
    buf = lambda: SimpleNamespace(buf=torch.zeros(64, dtype=torch.int32))   # noqa: E731
    b = Batch(SimpleNamespace(rowptr=buf(), col=buf(), bits=buf()),
              BatchClass(B=3, N=30, n_max=12, n_min=8, symmetric=False, dense=dense, iso=iso, has_bits=True, nnz_max=40))
    for name in ("node_off", "rp_off", "col_off", "t_rp_off", "t_col_off", "bits_off", "t_bits_off"):
        setattr(b, name, torch.zeros(4, dtype=torch.int64))
    return b


def _agg_calls(core, b, F, spec, npool, learn_eps):
    """(form, backward, the form's own arguments, call -> d-eps count, timer tag, fused meta, spec or None) of every
    route into the aggregation: core._agg forward, backward and d-eps only; the layer-0 cache's untimed call without a
    spec; the two fused forms"""
    x, y, hf = torch.zeros(b.N, F), torch.zeros(b.N, F), torch.zeros(b.N, F)
    part = torch.zeros(64, dtype=torch.float64)
    eps = 1000 if learn_eps else None
    out = []
    for bwd, dot in ((False, False), (True, False), (True, True)):
        yy = None if dot else y
        h, p = (hf, part) if bwd and learn_eps else (None, None)
        rest = (x.data_ptr(), F, None if dot else y.data_ptr(), 0 if dot else F, F, eps, int(npool == "average"),
                int(not learn_eps), int(bwd), None if h is None else h.data_ptr(), 0 if h is None else F,
                None if p is None else p.data_ptr())
        out.append(("plain", bwd, rest, lambda bwd=bwd, yy=yy, h=h, p=p: core._agg(b, x, yy, F, eps, spec, bwd, h, p),
                    "agg_%s_F%d%s" % ("bwd" if bwd else "fwd", F, "_dot" if dot else ""), {}, spec))
    rest0 = (x.data_ptr(), F, y.data_ptr(), F, F, eps, int(npool == "average"), int(not learn_eps), 0, None, 0, None)
    out.append(("plain", False, rest0,
                lambda: core.agg_launch(b, "plain", F, rest0, timed=False, stream=_STREAM)[1], None, {}, None))
    for form, bwd, meta, graph_args in (("fwd_bnrelu", False, {"fused_bnrelu": 1}, 8),
                                        ("bwd_stats", True, {"fused_stats": 1}, 10)):
        from gnm._cabi import SIGNATURES
        rest = tuple(range(7000, 7000 + len(SIGNATURES[_AGG_ENTRIES[form][1]][1]) - graph_args - 1))
        out.append((form, bwd, rest, lambda form=form, bwd=bwd, rest=rest: core.agg_launch(b, form, F, rest, spec,
                                                                                            backward=bwd),
                    "agg_%s_F%d" % ("bwd" if bwd else "fwd", F), meta, spec))
    return out


@pytest.mark.parametrize("dense", (False, True))
@pytest.mark.parametrize("iso", (False, True))
@pytest.mark.parametrize("F", (7, 64, 128))
def test_aggregation_routing_table(monkeypatch, dense, iso, F):
    """core.agg_launch, the one choice between the matrix-core aggregation (csrc/aggm.hip) and the CSR gather
    (csrc/agg.hip), against the routing the training step made by hand before it (core._agg, encoder_forward's fused
    prologue, _backward's fused epilogue, the layer-0 cache): the entry tried first, the one after a decline (-2), the
    arguments each gets, the d-eps partial count, the timer tag and meta, the failure names, and -2 from a fused form
    that both entries decline.  The six entries are spies returning programmed statuses."""
    from gnm import core
    from gnm._cabi import SIGNATURES, GnmError
    monkeypatch.setattr(core, "_new_event", _FakeEvent)
    monkeypatch.setattr(core, "_STREAM", _STREAM)
    status, calls = {}, []

    def spy(name):
        def call(*argv):
            calls.append((name, argv))
            return status[name]
        return call
    for pair in _AGG_ENTRIES.values():
        for name in pair:
            monkeypatch.setattr(core.lib, name, spy(name), raising=False)

    b = _fake_agg_batch(dense, iso)
    rowptr, col, bits = (t.buf.data_ptr() for t in (b.arena.rowptr, b.arena.col, b.arena.bits))
    for npool in ("sum", "average", "max"):
        for learn_eps in (False, True):
            spec = core.GinSpec(3, 2, learn_eps, "sum", npool)
            for form, bwd, rest, run, tag, meta, sp in _agg_calls(core, b, F, spec, npool, learn_eps):
                # the routing before agg_launch (core._dense): a dense batch of whole 32-column blocks or F < 32 takes
                # the matrix-core kernel, except neighbour "average" + learn_eps with an isolated node -- a rule the
                # layer-0 cache (no spec) does not apply
                mfma = dense and (F % 32 == 0 or F < 32) and not (
                    sp is not None and npool == "average" and learn_eps and iso)
                m_name, c_name = _AGG_ENTRIES[form]
                rp, co = (b.t_rp_off, b.t_col_off) if bwd else (b.rp_off, b.col_off)
                graph = (rowptr, col, rp.data_ptr(), co.data_ptr())
                deg = () if form == "fwd_bnrelu" else (rowptr, b.rp_off.data_ptr())
                node = (b.node_off.data_ptr(), b.B, b.n_max)
                m_argv = graph + (bits, (b.t_bits_off if bwd else b.bits_off).data_ptr()) + deg + node + rest + (_STREAM,)
                c_argv = graph + deg + node + (b.nnz_max,) + rest + (_STREAM,)
                assert len(m_argv) == len(SIGNATURES[m_name][1]) and len(c_argv) == len(SIGNATURES[c_name][1])
                m_count, c_count = 0, 0         # the fused forward writes no d-eps partials
                if form != "fwd_bnrelu":
                    m_count = int(core.lib.gnm_aggm_num_partials(F, b.B))
                    c_count = int(core.lib.gnm_agg_num_partials(F, b.n_max, b.B))
                base = dict(F=F, B=b.B, N=b.N, **meta)
                for rc_m in (0, -2, -1):
                    for rc_c in (0, -2, -1):
                        what = (form, bwd, tag, npool, learn_eps, rc_m, rc_c)
                        status.update({m_name: rc_m, c_name: rc_c})
                        calls.clear()
                        timer = core.KernelTimer()
                        monkeypatch.setattr(core, "TIMER", timer)
                        if form != "plain" and npool == "max":          # the fused forms: never under max pooling
                            assert run() == (-2, 0) and calls == [] and timer.records == [], what
                            continue
                        # expected: entries called, result, recorded meta, failure name
                        want_calls, want, rec, raises = [], None, None, None
                        if mfma:
                            want_calls.append((m_name, m_argv))
                            if rc_m == 0:
                                want, rec = (0, m_count), dict(base, mfma=1)
                            elif rc_m == -1:
                                raises = m_name if form == "plain" else c_name
                        if not want and not raises:
                            want_calls.append((c_name, c_argv))
                            if rc_c == 0:
                                want, rec = (0, c_count), base
                            elif rc_c == -2 and form != "plain":
                                want = (-2, 0)
                            else:                                       # the plain form must end on a launch
                                raises = c_name
                        if raises:
                            with pytest.raises(GnmError, match="^%s failed" % raises):
                                run()
                        else:
                            got = run()
                            assert got == (want[1] if form == "plain" else want), what
                        assert calls == want_calls, what
                        assert [(r[0], r[1]) for r in timer.records] == \
                            ([(tag, rec)] if rec is not None and tag is not None else []), what


_LINBWD_SPIES = ("gnm_linear_bwd_fused_rz", "gnm_linear_bwd_fused", "gnm_bn_bwd_apply", "gnm_linear_wgrad",
                 "gnm_linear_dgrad_masked", "gnm_linear_fwd")


def _fake_lin_save(core, N, K, H, pro):
    """a Linear [K -> H] as encoder_forward saves it, on CPU tensors"""
    sv = core._LinSave()
    sv.x_in, sv.z, sv.K, sv.H, sv.Ng = torch.zeros(N, K), torch.zeros(N, H), K, H, N
    sv.pro = (torch.zeros(K), torch.zeros(K)) if pro else None
    sv.scale, sv.shift, sv.mean, sv.rstd = (torch.zeros(H) for _ in range(4))
    return sv


@pytest.mark.parametrize("K,H", ((7, 64), (16, 64), (64, 64), (32, 64), (64, 32), (128, 128), (400, 64)))
@pytest.mark.parametrize("pro", (False, True))
@pytest.mark.parametrize("below", (False, True))
@pytest.mark.parametrize("need_dA", (False, True))
def test_linear_backward_routing_table(monkeypatch, K, H, pro, below, need_dA):
    """core.linear_bwd_launch, the one place that routes a Linear's backward, against the rules the training step
    applied inline before it:
      * gnm_linear_bwd_fused_rz is asked only when H = 64, no lower-BatchNorm sums are wanted, and K = 64 with dA or
        K <= 16 without a prologue; after its decline, or straight away, gnm_linear_bwd_fused with the stored Z; both
        with dW = NULL and a workspace of gnm_linear_bwd_workspace_floats, their dW / db reduction deferred;
      * the lower BatchNorm's sums ride on those entries when there is a Linear below and dA is wanted, in
        gnm_linear_bwd_grid(N) rows;
      * after -2 from the last of them: gnm_bn_bwd_apply in place, gnm_linear_wgrad with its own workspace, and for dA
        gnm_linear_dgrad_masked (K = H = 128 over a Linear below; gnm_linear_grid(N) rows) or, after its decline, the
        k-major gnm_linear_fwd in column windows of 128;
      * one linbwd_K<K>_H<H> record only when a fused entry ran, wgrad_K<K>_H<H> and lin_dgrad_K<H>_H<window> records
        for the kernels of the generic path; any other status raises under gnm_linear_bwd_fused /
        gnm_linear_dgrad_masked.
    The entries are spies returning programmed statuses; every tensor the function allocates is caught in order."""
    from gnm import core
    from gnm._cabi import SIGNATURES, GnmError
    monkeypatch.setattr(core, "_new_event", _FakeEvent)
    monkeypatch.setattr(core, "_STREAM", _STREAM)
    status, calls, allocs = dict.fromkeys(_LINBWD_SPIES, 0), [], []

    def spy(name):
        def call(*argv):
            calls.append((name, argv))
            return status[name]
        return call
    for name in _LINBWD_SPIES:
        monkeypatch.setattr(core.lib, name, spy(name), raising=False)
    real_empty = torch.empty

    def empty(*a, **k):
        allocs.append(real_empty(*a, **k))
        return allocs[-1]

    N = 100
    lib = core.lib
    sv = _fake_lin_save(core, N, K, H, pro)
    lo = _fake_lin_save(core, N, 5, K, False) if below else None
    G, W, bias, dW, db = torch.zeros(N, H), torch.zeros(H, K), torch.zeros(H), torch.zeros(H, K), torch.zeros(H)
    cA, m1, m2 = (torch.zeros(H) for _ in range(3))
    p = lambda t: t.data_ptr()      # noqa: E731
    pro_args = (p(sv.pro[0]), p(sv.pro[1]), 1) if pro else (None, None, 0)
    lo_args = (p(lo.z), K, p(lo.scale), p(lo.shift), p(lo.mean), p(lo.rstd)) if below else None
    shape = {"N": N, "K": K, "H": H}
    monkeypatch.setattr(torch, "empty", empty)
    for rc_rz in (0, -2, -1):
        for rc_f in (0, -2, -1):
            for rc_m in (0, -2, -1):
                what = (rc_rz, rc_f, rc_m)
                status.update(gnm_linear_bwd_fused_rz=rc_rz, gnm_linear_bwd_fused=rc_f, gnm_linear_dgrad_masked=rc_m)
                calls.clear()
                allocs.clear()
                timer = core.KernelTimer()
                monkeypatch.setattr(core, "TIMER", timer)
                raises, got = None, None
                try:
                    got = core.linear_bwd_launch(sv, lo, G, (cA, m1, m2), W, bias, dW, db, need_dA, N, _STREAM)
                except GnmError as e:
                    raises = str(e).split(" failed")[0]
                for name, argv in calls:
                    assert len(argv) == len(SIGNATURES[name][1]), (name, what)
                # ---- what the rules above give ----
                a = iter(allocs)
                dA = next(a) if need_dA else None
                ws = next(a)
                assert ws.shape == (lib.gnm_linear_bwd_workspace_floats(N, H, K),) and ws.dtype == torch.float32
                sums = next(a) if below and need_dA else None
                if sums is not None:
                    assert sums.shape == (lib.gnm_linear_bwd_grid(N), 2, K) and sums.dtype == torch.float64
                if need_dA:
                    assert dA.shape == (N, K) and dA.dtype == torch.float32
                rest = (p(sv.mean), p(sv.rstd), p(cA), p(m1), p(m2), p(sv.x_in), K) + pro_args + (
                    p(W), K, p(dA) if need_dA else None, K if need_dA else 0, None, K, p(db), p(ws), N, K, H) + (
                    lo_args if sums is not None else (None, 0, None, None, None, None)) + (
                    p(sums) if sums is not None else None, _STREAM)
                want_calls, want_rec, want_raise, want = [], [], None, None
                rc = -2
                if H == 64 and sums is None and ((K == 64 and need_dA) or (K <= 16 and not pro)):
                    want_calls.append(("gnm_linear_bwd_fused_rz", (p(G), H, p(bias)) + rest))
                    rc = rc_rz
                if rc == -2:
                    want_calls.append(("gnm_linear_bwd_fused", (p(G), H, p(sv.z), H) + rest))
                    rc = rc_f
                if rc == 0:
                    want_rec.append(("linbwd_K%d_H%d" % (K, H), shape))
                    want = (dA, sums, lib.gnm_linear_bwd_grid(N), (ws, dW, db, H, K))
                elif rc == -1:
                    want_raise = "gnm_linear_bwd_fused"
                else:
                    want_calls.append(("gnm_bn_bwd_apply", (p(G), H, p(sv.z), H, p(sv.mean), p(sv.rstd), p(cA), p(m1),
                                                            p(m2), p(G), H, N, H, _STREAM)))
                    ws2 = next(a)
                    assert ws2.shape == (lib.gnm_wgrad_workspace_floats(N, H, K),) and ws2.dtype == torch.float32
                    want_calls.append(("gnm_linear_wgrad", (p(G), H, p(sv.x_in), K, N, H, K) + pro_args + (
                        p(dW), K, p(db), p(ws2), _STREAM)))
                    want_rec.append(("wgrad_K%d_H%d" % (K, H), shape))
                    sums2, rc2 = None, -2
                    if need_dA and below and K == 128 and H == 128:
                        sums2 = next(a)
                        assert sums2.shape == (lib.gnm_linear_grid(N), 2, K) and sums2.dtype == torch.float64
                        want_calls.append(("gnm_linear_dgrad_masked", (p(G), H, p(W), K, p(dA), K, N, K, H) + lo_args + (
                            p(sums2), _STREAM)))
                        rc2 = rc_m
                    if rc2 == -1:
                        want_raise = "gnm_linear_dgrad_masked"
                    elif need_dA and rc2 == -2:
                        for k0 in range(0, K, 128):           # dX = dZ W: the weight k-major, 128 columns at a time
                            kw = min(128, K - k0)
                            want_calls.append(("gnm_linear_fwd", (p(G), H, p(W) + 4 * k0, K, 1, None, p(dA) + 4 * k0, K,
                                                                  N, H, kw, None, None, 0, None, _STREAM)))
                            want_rec.append(("lin_dgrad_K%d_H%d" % (H, kw), {"N": N, "K": H, "H": kw}))
                    if want_raise is None:
                        want = (dA, sums2 if rc2 == 0 else None, lib.gnm_linear_grid(N), None)
                assert next(a, None) is None, what           # nothing else was allocated
                assert calls == want_calls, what
                assert [(r[0], r[1]) for r in timer.records] == want_rec, what
                assert raises == want_raise, what
                if want is not None:
                    w_dA, w_sums, w_rows, w_job = want
                    assert got.dA is w_dA, what
                    if w_sums is None:
                        assert got.lo_sums is None, what
                    else:
                        assert got.lo_sums.G is w_dA and got.lo_sums.part is w_sums and got.lo_sums.rows == w_rows, what
                    if w_job is None:
                        assert got.job is None, what
                    else:
                        assert all(x is y for x, y in zip(got.job[:3], w_job[:3])) and tuple(got.job[3:]) == w_job[3:], what
                        assert (got.job.ws, got.job.dW, got.job.db, got.job.H, got.job.K) == tuple(got.job), what


@pytest.mark.parametrize("sizes, budget", [
    ([3, 3, 3, 3], 4 * 6),              # exact fits: two items each
    ([3, 3, 3, 3], 4 * 6 - 1),          # one byte short of two
    ([2, 9, 2, 2, 1], 4 * 5),           # a single item over the budget, alone in its run
    ([5, 1, 7, 1, 1, 1], 1),            # a budget of 1: every item alone
    ([1, 2, 3, 4, 5, 6, 7], 4 * 10),
    ([4], 0), ([], 100),
])
def test_runs_within_against_brute_force(sizes, budget):
    """attribution._runs_within (the chunking of occlusion_hip, lesion_hip and integrated_gradients_hip): in order, no run
    empty, each run the longest that fits -- against the definition, tried run by run"""
    from gnm import attribution
    asked = []

    def floats_of(i0, i1):
        assert 0 <= i0 < i1 <= len(sizes)                       # never an empty or an out-of-range run
        asked.append((i0, i1))
        return sum(sizes[i0:i1]) + (i1 - i0) * max(sizes[i0:i1])      # not additive, as the scratch sizes are not

    want, i0 = [], 0
    while i0 < len(sizes):
        fits = [i1 for i1 in range(i0 + 1, len(sizes) + 1) if 4 * floats_of(i0, i1) <= budget]
        i1 = i0 + 1
        while i1 + 1 in fits:           # stops BEFORE the first item that goes over, whatever fits behind it
            i1 += 1
        want.append((i0, i1))
        i0 = i1
    assert list(attribution._runs_within(len(sizes), floats_of, budget)) == want
    assert [i for a, b in want for i in range(a, b)] == list(range(len(sizes)))     # every item once, in order


@pytest.mark.parametrize("seed", range(6))
def test_runs_under_is_runs_within_on_a_prefix_array(seed):
    """attribution._runs_under (shapley_hip's chunking) against its docstring: _runs_within for the cost
    f[i1] - f[i0] of a non-decreasing prefix array f.  _runs_under's budget is in floats, _runs_within's in bytes.
    Budgets from below the smallest item (every item alone, most of them over the budget) to the whole array in one run,
    the exact boundaries f[j] - f[i] and their neighbours among them; zero-cost items and an empty array too."""
    from gnm import attribution
    rng = np.random.default_rng(seed)
    count = int(rng.integers(0, 40))
    steps = rng.integers(0 if seed % 2 else 1, 50, count)   # (odd seeds: items of cost 0, f not strictly increasing)
    if count:
        steps[int(rng.integers(0, count))] = 400            # one item far above most budgets below
    f = np.concatenate([[0], np.cumsum(steps)]).astype(np.int64)
    edges = {int(f[j] - f[i]) for i in range(count + 1) for j in range(i, count + 1)}
    budgets = {0, 1, 49, 399, 400, 401, int(f[-1]), int(f[-1]) + 1} | {e + d for e in list(edges)[:60] for d in (-1, 0, 1)}
    for budget in sorted(b for b in budgets if b >= 0):
        want = list(attribution._runs_within(len(f) - 1, lambda a, b: int(f[b] - f[a]), 4 * budget))
        assert list(attribution._runs_under(f, budget)) == want, (seed, budget)
        assert [i for a, b in want for i in range(a, b)] == list(range(count))


def test_gradient_collector():
    """core._Grads, where the backward's kernels and torch ops leave the parameter gradients: with a sink
    (GinSpec.grad_sink) they go into its tensors and autograd gets None for every parameter; without one they are
    fresh tensors; needs_input_grad masks both."""
    from gnm import core
    like = {"a": torch.zeros(3, 2), "b": torch.zeros(4), "c": torch.zeros(1, 2, 2)}
    names, needs = ("a", "b", "c", "d"), (True, False, True, True)

    def fill(g):
        """as a backward does: a kernel writes into out(), a torch result is put(), `c` is written as [0] of a 3-D one"""
        a = g.out("a", like["a"])
        a.copy_(torch.arange(6.).view(3, 2))
        g.put("b", torch.arange(4.) + 10)
        g.out("c", like["c"])[0].copy_(torch.eye(2))
        return a

    sink = {k: torch.full_like(v, -1.0) for k, v in like.items()}
    g = core._Grads(sink)
    assert fill(g) is sink["a"]
    assert g.result(names, needs) == (None, None, None, None)
    assert torch.equal(sink["a"], torch.arange(6.).view(3, 2)) and torch.equal(sink["b"], torch.arange(4.) + 10)
    assert torch.equal(sink["c"], torch.eye(2).unsqueeze(0))
    g.put("a", torch.ones(6))                       # a torch result of another shape is reshaped into the sink's tensor
    assert torch.equal(sink["a"], torch.ones(3, 2))

    g = core._Grads(None)
    t = fill(g)
    assert t is not like["a"] and t.shape == like["a"].shape and t.dtype == like["a"].dtype
    res = g.result(names, needs)
    assert res[0] is t and torch.equal(res[0], torch.arange(6.).view(3, 2))
    assert res[1] is None                           # computed, but not asked for
    assert res[2].shape == (1, 2, 2) and torch.equal(res[2][0], torch.eye(2))
    assert res[3] is None                           # asked for, never produced
    assert g.result(names, (True,) * 4)[1] is not None
