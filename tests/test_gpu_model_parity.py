"""GPU parity of the whole hot path (GIN_InfoMaxReg over libgnm_hip.so) against
(a) the golden vectors captured from the real reference and (b) the fp64 oracle.

Tolerances: integer structures bit-exact; activations / logits <= 1e-5 relative
(max-norm) -- the north_star bar; gradients 5e-5 (tiny cases).  The true-shape case uses
the calibrated bounds documented in helpers.py."""
import numpy as np
import pytest
import torch

import json
import os

from helpers import (RTOL, TRUE_SHAPE_GRAD_RTOL, Calibrated, assert_close, assert_grad_true_shape, edge_mat_of,
                     golden_cases, grad_floor, load_case, neighbors_of, rel_err)

REPORT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gpurun_out",
                      "parity_true_shape.json")


def report(case, mode, cal, extra=None):
    """Record what the true-shape checks MEASURED (HIP path vs fp64 oracle, next to the reference's own error
    and the bound applied) in gpurun_out/parity_true_shape.json; DESIGN.md section 5 quotes it."""
    try:
        os.makedirs(os.path.dirname(REPORT), exist_ok=True)
        data = json.load(open(REPORT)) if os.path.exists(REPORT) else {}
        data["%s/%s" % (case, mode)] = {
            "checks": [{"what": w, "hip_vs_fp64": e, "reference_vs_fp64": r, "bound": b, "hip_vs_golden": eg}
                       for (w, e, r, b), eg in zip(cal.log, cal.log_golden)],
            **(extra or {})}
        json.dump(data, open(REPORT, "w"), indent=1)
    except OSError:
        pass
    for (w, e, r, b), eg in zip(cal.log, cal.log_golden):
        print("%-36s %-5s %-12s HIP vs fp64 %.2e   HIP vs golden %.2e   reference vs fp64 %.2e   bound %.1e%s"
              % (case, mode, w, e, eg, r, b, "" if e <= RTOL else "   (> 1e-5)"))

pytestmark = pytest.mark.gpu
CASES = golden_cases()
DEV = "cuda:0"


class G:
    pass


def make_graphs(cfg, d):
    out = []
    for g in range(cfg["B"]):
        o = G()
        o.g = list(range(cfg["n"]))
        o.edge_mat = torch.from_numpy(edge_mat_of(d[f"und_{g}"]))
        o.node_features = torch.from_numpy(d[f"feat_{g}"])
        o.label = int(d["labels"][g])
        o.neighbors = neighbors_of(d[f"und_{g}"], cfg["n"])                 # util.py:86-95
        o.max_neighbor = max(len(x) for x in o.neighbors)
        out.append(o)
    return out


def make_model(cfg, state, dropout=0.0):
    from models.graphcnn import GIN_InfoMaxReg
    dev = torch.device(DEV)
    m = GIN_InfoMaxReg(cfg["L"], cfg["m"], cfg["f0"], cfg["H"], cfg["C"], dropout, cfg["learn_eps"], cfg["gpool"],
                       cfg["npool"], dev)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in state.items()})
    return m.to(dev)


def oracle_model(cfg, state):
    from oracle import gin_oracle as O
    return O, O.OracleGIN(state, cfg["L"], cfg["m"], cfg["learn_eps"], cfg["gpool"], cfg["npool"], dtype=np.float64)


def oracle_batch(O, cfg, d):
    return [O.OGraph(cfg["n"], edge_mat_of(d[f"und_{g}"]), d[f"feat_{g}"], int(d["labels"][g]),
                     neighbors=neighbors_of(d[f"und_{g}"], cfg["n"])) for g in range(cfg["B"])]


def capture_layers(model):
    """pooled (input of the MLP) and hidden (layer output) of every layer, from the
    tensors the autograd Function saved."""
    from gnm import core
    model.eval_replay = False       # the hook below copies to the host inside the forward: not capturable
    model.eval_fused = False        # ... and it hooks the layer-by-layer encoder (the one-launch one: test_gpu_eval_fused.py)
    model.train_replay = False
    store = {}
    orig = core.encoder_forward

    def wrapped(*a, **k):
        hidden, g_f, saved = orig(*a, **k)
        # (layers that exist only as (z, scale, shift) -- core.ZAct -- are materialised the way their consumers re-form them)
        store["hidden"] = [core.hidden_tensor(h).detach().cpu().numpy() for h in hidden]
        store["pooled"] = [s[1].detach().cpu().numpy() for s in saved]
        return hidden, g_f, saved

    return store, orig, wrapped


@pytest.mark.parametrize("case", CASES)
def test_index_structures_bit_exact(case):
    """The device CSR arena encodes exactly the reference's Adj_block edge multiset and
    offsets (graphcnn.py:84-106) and the readout segments (graphcnn.py:109-134)."""
    cfg, state, d = load_case(case)
    model = make_model(cfg, state)
    graphs = make_graphs(cfg, d)
    batch = model._batch_of(graphs)
    if cfg["npool"] == "max":
        # the device arrays the max-pooling kernels walk, expanded the way they walk them, are the reference's padded
        # neighbour list (graphcnn.py:55-81); tests/test_cabi_host.py checks the transposed structure too
        mb, ref = batch.maxnb, d["padded_neighbors"]
        off, col = mb.nb_off.cpu().numpy(), mb.nb_col.cpu().numpy()
        rows = [list(col[off[i]:off[i + 1]]) + [-1] * (mb.max_deg - (off[i + 1] - off[i])) + ([i] if mb.self_last else [])
                for i in range(mb.N)]
        assert np.array_equal(np.asarray(rows, dtype=np.int64).reshape(ref.shape), ref)
    else:
        coo = model.arena().export_adj_coo(batch, self_loops=not cfg["learn_eps"])
        ref = d["adj_indices"]
        assert coo.dtype == np.int64 and coo.shape == ref.shape
        canon = lambda a: a[:, np.lexsort((a[1], a[0]))]
        assert np.array_equal(canon(coo), canon(ref))
    # readout segments: graph_pool row i covers columns node_off[i]..node_off[i+1]
    gp = d["gp_indices"]
    node_off = batch.node_off.cpu().numpy()
    seg = np.repeat(np.arange(cfg["B"]), np.diff(node_off))
    assert np.array_equal(gp[0], seg) and np.array_equal(gp[1], np.arange(batch.N))
    if cfg["gpool"] == "average":
        w = (np.float32(1.0) / np.diff(node_off).astype(np.float32))[seg]
        assert np.array_equal(w, d["gp_values"])


@pytest.mark.parametrize("case", CASES)
def test_eval_forward_vs_golden(case):
    from gnm import core
    cfg, state, d = load_case(case)
    model = make_model(cfg, state).eval()
    graphs = make_graphs(cfg, d)
    store, orig, wrapped = capture_layers(model)
    core.encoder_forward = wrapped
    try:
        np.random.seed(cfg["np_seed"])
        with torch.no_grad():
            c_logit, d_logit = model(graphs)
    finally:
        core.encoder_forward = orig
    rs = slice(None, None, cfg["row_stride"])
    np.random.seed(cfg["np_seed"])
    lat = model(graphs, latent=True)
    assert isinstance(lat, np.ndarray)
    if not case.startswith("true_"):
        for l in range(cfg["L"]):
            assert_close(store["pooled"][l][rs], d[f"eval_pooled_{l}"], what=f"pooled {l}")
            assert_close(store["hidden"][l][rs], d[f"eval_hidden_{l}"], what=f"hidden {l}")
        assert_close(c_logit.cpu().numpy(), d["eval_c_logit"], what="c_logit")
        assert_close(d_logit.cpu().numpy(), d["eval_d_logit"], what="d_logit")
        assert_close(lat, d["eval_latent"], what="latent")
        return
    # true shape: against the fp64 oracle, <= 1e-5 wherever the reference's own fp32 noise leaves room for it
    # (bound = max(1e-5, 4 x the reference's error so far): helpers.Calibrated); the measured values are recorded
    O, om = oracle_model(cfg, state)
    tc_logit, td_logit, tcache = om.forward(oracle_batch(O, cfg, d), d["perm"], training=False)
    cal = Calibrated()
    for l in range(cfg["L"]):
        cal.check(store["pooled"][l][rs], d[f"eval_pooled_{l}"], tcache["layers"][l]["pooled"][rs], what=f"pooled {l}")
        cal.check(store["hidden"][l][rs], d[f"eval_hidden_{l}"], tcache["hidden"][l][rs], what=f"hidden {l}")
    cal.check(c_logit.cpu().numpy(), d["eval_c_logit"], tc_logit, what="c_logit")
    cal.check(d_logit.cpu().numpy(), d["eval_d_logit"], td_logit, what="d_logit")
    cal.check(lat, d["eval_latent"], tcache["g_f"], what="latent")
    report(case, "eval", cal)


@pytest.mark.parametrize("case", CASES)
def test_train_step_vs_golden_and_oracle(case):
    from gnm import core
    cfg, state, d = load_case(case)
    model = make_model(cfg, state).train()
    graphs = make_graphs(cfg, d)
    store, orig, wrapped = capture_layers(model)
    core.encoder_forward = wrapped
    try:
        np.random.seed(cfg["np_seed"])
        c_logit, d_logit = model(graphs)
    finally:
        core.encoder_forward = orig
    N = cfg["B"] * cfg["n"]
    dev = c_logit.device
    c_labels = torch.from_numpy(d["labels"]).to(dev)
    d_labels = torch.cat([torch.ones(N, 1), torch.zeros(N, 1)], 0).to(dev)      # main.py:32 sized by node count
    c_loss = torch.nn.CrossEntropyLoss()(c_logit, c_labels)
    d_loss = torch.nn.BCEWithLogitsLoss()(d_logit, d_labels)
    loss = c_loss + 0.05 * d_loss
    model.zero_grad()
    loss.backward()
    torch.cuda.synchronize()

    O, om = oracle_model(cfg, state)
    truth = om.train_step_grads(oracle_batch(O, cfg, d), d["perm"], beta=0.05)
    tc = truth["cache"]
    rs = slice(None, None, cfg["row_stride"])
    true_shape = case.startswith("true_")
    cal = Calibrated()
    losses = np.array([loss.item(), c_loss.item(), d_loss.item()])
    tl = np.array([truth["loss"], truth["c_loss"], truth["d_loss"]])
    if true_shape:
        for l in range(cfg["L"]):
            cal.check(store["pooled"][l][rs], d[f"train_pooled_{l}"], tc["layers"][l]["pooled"][rs], what=f"pooled {l}")
            cal.check(store["hidden"][l][rs], d[f"train_hidden_{l}"], tc["hidden"][l][rs], what=f"hidden {l}")
        cal.check(c_logit.detach().cpu().numpy(), d["train_c_logit"], truth["c_logit"], what="c_logit")
        cal.check(d_logit.detach().cpu().numpy(), d["train_d_logit"], truth["d_logit"], what="d_logit")
        cal.check(losses, d["train_loss"], tl, what="loss")
    else:
        for l in range(cfg["L"]):
            assert_close(store["pooled"][l][rs], d[f"train_pooled_{l}"], what=f"pooled {l} vs golden")
            assert_close(store["hidden"][l][rs], d[f"train_hidden_{l}"], what=f"hidden {l} vs golden")
            assert_close(store["hidden"][l], tc["hidden"][l], what=f"hidden {l} vs fp64 oracle")
        assert_close(c_logit.detach().cpu().numpy(), d["train_c_logit"], what="c_logit")
        assert_close(d_logit.detach().cpu().numpy(), d["train_d_logit"], what="d_logit")
        assert_close(losses, d["train_loss"], what="loss")

    gtol = TRUE_SHAPE_GRAD_RTOL if true_shape else 5 * RTOL
    floor = grad_floor(d)
    checked = 0
    worst = (0.0, "")
    for name, p in model.named_parameters():
        key = "grad_" + name
        if f"gradnone_{name}" in d:
            assert p.grad is None, name
            continue
        g = p.grad.detach().cpu().numpy()
        tg = truth["grads"][name].reshape(g.shape)
        if true_shape:
            # within 5e-3 of the reference's golden or of the fp64 oracle (helpers.assert_grad_true_shape)
            e_g, e_t = assert_grad_true_shape(g, d[key] if key in d else None, tg, what=name, floor=floor)
            worst = max(worst, (e_t if e_g is None else min(e_g, e_t), name))
        else:
            assert_close(g, tg, rtol=gtol, what=name + " vs fp64 oracle", floor=floor)
            if key in d:
                assert_close(g, d[key], rtol=gtol, what=name + " vs golden", floor=floor)
        checked += 1
    assert checked >= 10
    if true_shape:
        report(case, "train", cal, {"worst_gradient": {"name": worst[1], "err_vs_nearest_anchor": worst[0]}})
    for key in d:
        if key.startswith("bufafter_"):
            name = key[len("bufafter_"):]
            got = dict(model.named_buffers())[name].cpu().numpy()
            if name.endswith("num_batches_tracked"):
                assert int(got) == int(d[key])
            elif true_shape:
                cal.check(got, d[key], om.p[name], what=key)
            else:
                assert_close(got, d[key], what=key)


@pytest.mark.parametrize("case", [c for c in CASES if c.startswith("tiny_")])
def test_saliency_vs_golden(case):
    cfg, state, d = load_case(case)
    model = make_model(cfg, state)
    graphs = make_graphs(cfg, d)
    for cls in (0, 1):
        sal = model.compute_saliency([graphs[0]], cls)
        assert sal.shape == (cfg["n"], cfg["f0"])
        assert_close(sal.cpu().numpy(), d[f"saliency_cls{cls}"], rtol=5 * RTOL, what=f"saliency {cls}")
    assert not model.training            # compute_saliency leaves the model in eval mode (graphcnn.py:255)


def test_dropout_train_mode_runs_and_scales():
    """final_dropout > 0 in train mode: logits are a masked/scaled sum (graphcnn.py:230)."""
    cfg, state, d = load_case("tiny_s0_eps1_gsum_nsum")
    model = make_model(cfg, state, dropout=0.5).train()
    graphs = make_graphs(cfg, d)
    torch.manual_seed(0)
    np.random.seed(1)
    c1, _ = model(graphs)
    model2 = make_model(cfg, state, dropout=0.0).train()
    np.random.seed(1)
    c0, _ = model2(graphs)
    assert c1.shape == c0.shape and torch.isfinite(c1).all()
    assert not torch.allclose(c1, c0)


def test_isolated_node_average_nan_matches_reference():
    """graphcnn.py:157-158: 0/0 for an isolated node under average pooling + learn_eps."""
    from gnm import core
    cfg, state, d = load_case("tiny_s1_eps1_gsum_naverage")
    model = make_model(cfg, state).eval()
    graphs = make_graphs(cfg, d)[:1]
    em = graphs[0].edge_mat.numpy()
    keep = (em[0] != 3) & (em[1] != 3)
    graphs[0].edge_mat = torch.from_numpy(np.ascontiguousarray(em[:, keep]))
    store, orig, wrapped = capture_layers(model)
    core.encoder_forward = wrapped
    try:
        with torch.no_grad():
            c_logit, d_logit = model(graphs)
    finally:
        core.encoder_forward = orig
    # the reference's ReLU keeps a NaN (torch.relu), so the poisoned row reaches the graph's readout and BOTH outputs of
    # that graph are NaN -- fmaxf(x, 0) would quietly return 0 there (csrc/gnm_common.h gnm_relu)
    assert torch.isnan(c_logit).all() and torch.isnan(d_logit).all()
    assert np.isnan(store["pooled"][0][3]).all()
    assert not np.isnan(store["pooled"][0][0]).any()
    # every layer, not only the first: the reference keeps the NaN to the isolated node's own row (nobody gathers
    # it), so hidden[l] / pooled[l] of the OTHER rows stay finite in every layer.  A dense batch in this mode is
    # routed to the CSR gather for exactly that reason (gnm/core.py _dense: the matrix-core product would spread
    # 0 x NaN over the whole graph from layer 1 on).
    O, omodel = oracle_model(cfg, state)
    og = O.OGraph(cfg["n"], graphs[0].edge_mat.numpy(), graphs[0].node_features.numpy())
    with np.errstate(all="ignore"):
        _, _, cache = omodel.forward([og], np.array([0]), training=False)
    for l in range(cfg["L"]):
        ref_p, ref_h = cache["layers"][l]["pooled"], cache["hidden"][l]
        assert np.array_equal(np.isnan(store["pooled"][l]), np.isnan(ref_p)), "pooled %d NaN pattern" % l
        assert np.array_equal(np.isnan(store["hidden"][l]), np.isnan(ref_h)), "hidden %d NaN pattern" % l
        assert np.isnan(ref_p[3]).all() and not np.isnan(np.delete(ref_p, 3, 0)).any()
        assert_close(store["pooled"][l], ref_p, what="pooled %d" % l)


def test_non_symmetric_graph_backward_uses_transposed_csr():
    """Reference graphs are symmetric (util.py:99-100) but edge_mat may be anything:
    gradients must follow A^T.  Checked against the fp64 oracle."""
    cfg, state, d = load_case("tiny_s1_eps1_gsum_nsum")
    rng = np.random.default_rng(5)
    graphs = make_graphs(cfg, d)
    O, om = oracle_model(cfg, state)
    ob = []
    for g in graphs:
        em = g.edge_mat.numpy()
        em = em[:, rng.random(em.shape[1]) < 0.6]          # drop edges at random -> asymmetric
        g.edge_mat = torch.from_numpy(np.ascontiguousarray(em))
        ob.append(O.OGraph(cfg["n"], em, g.node_features.numpy(), g.label))
    model = make_model(cfg, state).train()
    np.random.seed(3)
    perm = np.random.permutation(cfg["B"])
    np.random.seed(3)
    c_logit, d_logit = model(graphs)
    assert not model.arena().batch(graphs).symmetric
    truth = om.train_step_grads(ob, perm)
    N = cfg["B"] * cfg["n"]
    dev = c_logit.device
    loss = torch.nn.CrossEntropyLoss()(c_logit, torch.from_numpy(d["labels"]).to(dev)) + 0.05 * \
        torch.nn.BCEWithLogitsLoss()(d_logit, torch.cat([torch.ones(N, 1), torch.zeros(N, 1)], 0).to(dev))
    loss.backward()
    assert_close(c_logit.detach().cpu().numpy(), truth["c_logit"], what="c_logit")
    floor = 2e-2 * max(float(np.abs(v).max()) for v in truth["grads"].values())
    for name, p in model.named_parameters():
        assert_close(p.grad.cpu().numpy(), truth["grads"][name].reshape(p.shape), rtol=5 * RTOL, what=name,
                     floor=floor)


def test_run_to_run_determinism():
    """All reductions are fixed-order: two identical steps give bitwise identical grads."""
    cfg, state, d = load_case("true_s0_eps1_gsum_nsum")
    graphs = make_graphs(cfg, d)
    outs = []
    for _ in range(2):
        model = make_model(cfg, state).train()
        np.random.seed(11)
        c_logit, d_logit = model(graphs)
        (c_logit.sum() + d_logit.sum()).backward()
        outs.append([p.grad.clone() for p in model.parameters() if p.grad is not None] + [c_logit.detach(), d_logit.detach()])
    for a, b in zip(*outs):
        assert torch.equal(a, b)


@pytest.mark.parametrize("npool,gpool,learn_eps", [("sum", "sum", True), ("average", "average", True),
                                                   ("sum", "average", False)])
def test_sparse_regime_config4_vs_fp64_oracle(npool, gpool, learn_eps):
    """BASELINE configs[3]: 1000-node k-NN (k = 20, symmetrised) graphs, hidden 128 -- the
    [n, 128] tile does not fit LDS, so the aggregation runs as 4 feature slices of 32.
    Whole training step against the fp64 oracle at the full depth (five layers) and the north_star's 1e-5 on the
    logits; the same shape against the REFERENCE's own outputs: the true_c4_* goldens (round 4), which the
    golden-driven tests above pick up by name."""
    from gnm import synth
    from models.graphcnn import GIN_InfoMaxReg
    from oracle import gin_oracle as O
    L, m, f0, H, C, B = 5, 2, 7, 128, 2, 2
    graphs = [synth.knn_graph(g, n=1000, k=20, f0=f0) for g in range(B)]
    assert 25000 < graphs[0].edge_mat.shape[1] < 33000          # ~29.1k directed edges
    dev = torch.device(DEV)
    torch.manual_seed(5)
    model = GIN_InfoMaxReg(L, m, f0, H, C, 0.0, learn_eps, gpool, npool, dev).to(dev).train()
    state = {k: v.detach().cpu().numpy().copy() for k, v in model.state_dict().items()}
    np.random.seed(4)
    perm = np.random.permutation(B)
    np.random.seed(4)
    c_logit, d_logit = model(graphs)
    N = B * 1000
    labels = torch.tensor([g.label for g in graphs], device=dev)
    d_labels = torch.cat([torch.ones(N, 1), torch.zeros(N, 1)], 0).to(dev)
    loss = torch.nn.CrossEntropyLoss()(c_logit, labels) + 0.05 * torch.nn.BCEWithLogitsLoss()(d_logit, d_labels)
    loss.backward()
    ob = [O.OGraph(1000, g.edge_mat.numpy(), g.node_features.numpy(), g.label) for g in graphs]
    truth = O.OracleGIN(state, L, m, learn_eps, gpool, npool, dtype=np.float64).train_step_grads(ob, perm)
    assert_close(c_logit.detach().cpu().numpy(), truth["c_logit"], rtol=RTOL, what="c_logit")
    assert_close(d_logit.detach().cpu().numpy(), truth["d_logit"], rtol=RTOL, what="d_logit")
    floor = 2e-2 * max(float(np.abs(v).max()) for v in truth["grads"].values())
    for name, p in model.named_parameters():
        if p.grad is None:
            assert name == "eps" and not learn_eps
            continue
        # (no reference golden behind THIS batch, so a ReLU-mask bit that fp32 and fp64 arithmetic decide differently
        #  cannot be told from an error: 5e-3 here -- 1.2e-3 measured on one weight of the average / average case -- while
        #  the golden-backed true_c4_* cases above are held to 1e-3 against "the reference's golden or fp64")
        assert_close(p.grad.cpu().numpy(), truth["grads"][name].reshape(p.shape), rtol=5e-3, what=name, floor=floor)


def test_hipgraph_replay_matches_eager_bitwise():
    """gnm.graphs.CapturedTrainStep: the captured training step replayed on NEW batches
    (descriptors, labels and the Infomax permutation copied into static buffers) gives
    bitwise the same loss and gradients as eager launches."""
    from gnm import synth
    from gnm.graphs import CapturedTrainStep
    from models.graphcnn import GIN_InfoMaxReg
    dev = torch.device(DEV)
    pool = synth.make_pool("dense_fc", 12, n=60, t=64, f0=7)
    labels_all = torch.tensor([g.label for g in pool], device=dev)
    N = 4 * 60
    d_labels = torch.cat([torch.ones(N, 1), torch.zeros(N, 1)], 0).to(dev)

    def loss_fn(c, d, lab):
        return torch.nn.functional.cross_entropy(c, lab) + \
            0.05 * torch.nn.functional.binary_cross_entropy_with_logits(d, d_labels)

    def fresh():
        torch.manual_seed(0)
        m = GIN_InfoMaxReg(5, 2, 7, 64, 2, 0.0, True, "sum", "average", dev).to(dev).train()
        ar = m.arena()
        gids = np.array([ar.add(g) for g in pool], dtype=np.int64)
        return m, ar, gids

    sels = [np.array([0, 1, 2, 3]), np.array([7, 4, 11, 9]), np.array([5, 5, 2, 10])]
    perms = [np.array([2, 0, 3, 1]), np.array([0, 1, 2, 3]), np.array([3, 2, 1, 0])]
    # eager reference (fresh model per step so BatchNorm running stats do not matter: compare grads of step i
    # computed from identical parameters; running stats only feed eval mode)
    eager = []
    m, ar, gids = fresh()
    for sel, perm in zip(sels, perms):
        m.zero_grad(set_to_none=False)
        bt = ar.batch_from_gids(gids[sel])
        c, d = m.forward_batch(bt, perm=perm)
        loss = loss_fn(c, d, labels_all[torch.as_tensor(sel, device=dev)])
        loss.backward()
        eager.append([loss.detach().clone()] + [p.grad.clone() for p in m.parameters()])
    m2, ar2, gids2 = fresh()
    for p in m2.parameters():
        p.grad = torch.zeros_like(p)
    cap = CapturedTrainStep(m2, ar2.batch_from_gids(gids2[sels[0]]), loss_fn)
    for sel, perm, ref in zip(sels, perms, eager):
        loss = cap.run(ar2.batch_from_gids(gids2[sel]), labels_all[torch.as_tensor(sel, device=dev)], perm)
        torch.cuda.synchronize()
        got = [loss.detach().clone()] + [p.grad.clone() for p in m2.parameters()]
        for a, b in zip(got, ref):
            assert torch.equal(a, b)
    # round 4: the packed form -- arena ids, labels and permutation through ONE pinned upload (run_gids), and a ready
    # Batch through the same capture (run); a permutation that is not one is refused on the host
    from gnm._cabi import GnmError
    m3, ar3, gids3 = fresh()
    for p in m3.parameters():
        p.grad = torch.zeros_like(p)
    labels_host = np.array([g.label for g in pool], dtype=np.int64)
    cap3 = CapturedTrainStep(m3, ar3.batch_from_gids(gids3[sels[0]]), loss_fn, gids_host=gids3[sels[0]])
    assert cap3.packed is not None
    for k, (sel, perm, ref) in enumerate(zip(sels, perms, eager)):
        if k == 1:
            loss = cap3.run(ar3.batch_from_gids(gids3[sel]), labels_all[torch.as_tensor(sel, device=dev)], perm)
        else:
            loss = cap3.run_gids(gids3[sel], labels_host[sel], perm)
        torch.cuda.synchronize()
        got = [loss.detach().clone()] + [p.grad.clone() for p in m3.parameters()]
        for a, b in zip(got, ref):
            assert torch.equal(a, b)
    assert cap3.eager_fallbacks == 0
    with pytest.raises(GnmError, match="permutation"):
        cap3.run_gids(gids3[sels[0]], labels_host[sels[0]], np.array([0, 0, 1, 2]))


def test_captured_step_runs_a_batch_without_bit_rows_eagerly():
    """A batch that differs from the captured one only in has_bits -- one multigraph among its graphs (a repeated edge:
    no bit rows), in a batch sparse enough to stay on the gather route either way -- is not replayed: run() on the
    packed capture runs the step eagerly, counts it and warns once, with the eager step's bits."""
    import warnings
    from gnm import synth
    from gnm.graphs import CapturedTrainStep
    from models.graphcnn import GIN_InfoMaxReg
    dev = torch.device(DEV)
    n = 120
    pool = synth.make_pool("knn", 6, n=n, k=2, f0=7)                 # ~2.5 % of n^2: below DENSE_MIN_FILL
    e = pool[5].edge_mat
    pool[5].edge_mat = torch.cat([e, e[:, [0, e.shape[1] // 2]]], 1)   # edge 0 once more, both ways
    d_labels = torch.cat([torch.ones(4 * n, 1), torch.zeros(4 * n, 1)], 0).to(dev)

    def loss_fn(c, d, lab):
        return torch.nn.functional.cross_entropy(c, lab) + \
            0.05 * torch.nn.functional.binary_cross_entropy_with_logits(d, d_labels)

    def fresh():
        torch.manual_seed(0)
        m = GIN_InfoMaxReg(3, 2, 7, 32, 2, 0.0, True, "sum", "sum", dev).to(dev).train()
        ar = m.arena()
        return m, ar, np.array(ar.add_many(pool), dtype=np.int64)

    sel, perm = np.array([4, 5, 1, 2]), np.array([2, 0, 3, 1])
    labels = torch.tensor([pool[i].label for i in sel], device=dev)
    m, ar, gids = fresh()
    template, bt = ar.batch_from_gids(gids[:4]), ar.batch_from_gids(gids[sel])
    assert template.has_bits and not bt.has_bits and not template.dense and not bt.dense
    assert template.batch_class._replace(has_bits=False, nnz_max=0) == bt.batch_class._replace(nnz_max=0)
    loss = loss_fn(*m.forward_batch(bt, perm=perm), labels)
    loss.backward()
    want = [loss.detach().clone()] + [p.grad.clone() for p in m.parameters()]

    m2, ar2, gids2 = fresh()
    for p in m2.parameters():
        p.grad = torch.zeros_like(p)
    cap = CapturedTrainStep(m2, ar2.batch_from_gids(gids2[:4]), loss_fn, gids_host=gids2[:4])
    assert cap.packed is not None and cap.packed.batch_class.nnz_max >= bt.nnz_max
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        loss = cap.run(ar2.batch_from_gids(gids2[sel]), labels, perm)
    torch.cuda.synchronize()
    assert cap.eager_fallbacks == 1
    assert [str(w.message) for w in caught if issubclass(w.category, RuntimeWarning)] == \
        ["CapturedTrainStep: a batch of another class than the captured one runs eagerly (counted in .eager_fallbacks)"]
    got = [loss.detach().clone()] + [p.grad.clone() for p in m2.parameters()]
    assert len(got) == len(want)
    for a, b in zip(got, want):
        assert torch.equal(a, b)


@pytest.mark.parametrize("case", ["tiny_s0_eps1_gsum_nsum", "tiny_s1_eps0_gaverage_nsum", "tiny_s2_mlp1",
                                  "tiny_s1_eps1_gaverage_nmax_iso"])
def test_gradient_sink_matches_autograd_accumulation(case):
    """DataParallelGIN's direct mode: kernels write gradients straight into the flat buffer
    (GinSpec.grad_sink) -- bitwise the same values autograd would have accumulated."""
    from gnm.parallel import DataParallelGIN
    cfg, state, d = load_case(case)
    graphs = make_graphs(cfg, d)
    res = []
    for direct in (False, True):
        model = make_model(cfg, state).train()
        dp = DataParallelGIN(model, direct_grads=direct)
        assert dp.direct == direct
        for _ in range(2):                                   # second step: stale values must be overwritten
            dp.zero_grad()
            np.random.seed(5)
            c, dl = model(graphs)
            (c.square().sum() + dl.square().mean()).backward()
        res.append(dp.fp.flat_grad.clone())
        for p in model.parameters():
            assert p.grad is not None
    assert torch.equal(res[0], res[1])


def test_one_hot_input_features_default_of_the_reference():
    """main.py's default --input_feature one_hot gives node_features = identity (F0 = n, util.py:115):
    layer 0 aggregates 400-wide rows (7 feature slices of 64) and its first Linear has K = 400.
    Whole training step against the fp64 oracle; saliency too (dX through the K = 400 Linear)."""
    from gnm import synth
    from models.graphcnn import GIN_InfoMaxReg
    from oracle import gin_oracle as O
    n, L, m, H, C, B = 400, 2, 2, 64, 2, 2
    graphs = []
    for g in range(B):
        gr = synth.dense_fc_graph(g, n=n, f0=1)
        gr.node_features = torch.eye(n)                     # one-hot ROI identity
        graphs.append(gr)
    dev = torch.device(DEV)
    torch.manual_seed(9)
    model = GIN_InfoMaxReg(L, m, n, H, C, 0.0, True, "sum", "sum", dev).to(dev).train()
    state = {k: v.detach().cpu().numpy().copy() for k, v in model.state_dict().items()}
    np.random.seed(2)
    perm = np.random.permutation(B)
    np.random.seed(2)
    c_logit, d_logit = model(graphs)
    N = B * n
    labels = torch.tensor([g.label for g in graphs], device=dev)
    d_labels = torch.cat([torch.ones(N, 1), torch.zeros(N, 1)], 0).to(dev)
    loss = torch.nn.CrossEntropyLoss()(c_logit, labels) + 0.05 * torch.nn.BCEWithLogitsLoss()(d_logit, d_labels)
    loss.backward()
    ob = [O.OGraph(n, g.edge_mat.numpy(), g.node_features.numpy(), g.label) for g in graphs]
    om = O.OracleGIN(state, L, m, True, "sum", "sum", dtype=np.float64)
    truth = om.train_step_grads(ob, perm)
    assert_close(c_logit.detach().cpu().numpy(), truth["c_logit"], rtol=2 * RTOL, what="c_logit")
    assert_close(d_logit.detach().cpu().numpy(), truth["d_logit"], rtol=2 * RTOL, what="d_logit")
    floor = 2e-2 * max(float(np.abs(v).max()) for v in truth["grads"].values())
    for name, p in model.named_parameters():
        assert_close(p.grad.cpu().numpy(), truth["grads"][name].reshape(p.shape), rtol=TRUE_SHAPE_GRAD_RTOL,
                     what=name, floor=floor)
    sal = model.compute_saliency([graphs[0]], 1)
    om2 = O.OracleGIN(state, L, m, True, "sum", "sum", dtype=np.float64)
    for k, v in model.state_dict().items():                  # running stats moved during the train step
        om2.p[k] = v.detach().cpu().numpy().astype(np.float64) if v.dtype.is_floating_point else v.cpu().numpy()
    ref = om2.compute_saliency(ob[0], 1)
    assert sal.shape == (n, n)
    assert_close(sal.cpu().numpy(), ref, rtol=TRUE_SHAPE_GRAD_RTOL, what="saliency", floor=1e-2 * np.abs(ref).max())


def test_ragged_batch_is_rejected_like_the_reference():
    """discriminator.py:24 expands each graph summary N//B times: graphs of different sizes
    cannot go through forward() (the reference fails with a shape error in nn.Bilinear)."""
    from gnm import synth
    from models.graphcnn import GIN_InfoMaxReg
    dev = torch.device(DEV)
    graphs = [synth.dense_fc_graph(0, n=40, t=64), synth.dense_fc_graph(1, n=48, t=64)]
    model = GIN_InfoMaxReg(2, 2, 7, 32, 2, 0.0, True, "sum", "sum", dev).to(dev)
    with pytest.raises(RuntimeError):
        model(graphs)


@pytest.mark.parametrize("learn_eps,npool", [(True, "sum"), (True, "average"), (False, "sum"), (False, "average")])
def test_layer0_aggregate_cache_equals_direct_aggregation(learn_eps, npool):
    """GraphArena.features_and_agg0: layer 0's parameter-independent A X [/deg] comes from a per-graph cache
    (built by the same gnm_agg kernel); passing X explicitly runs the aggregation in the step.  Same results, also
    after the arena has grown past the cached prefix, and eps_0 still gets its gradient."""
    from gnm import synth
    from models.graphcnn import GIN_InfoMaxReg
    dev = torch.device(DEV)
    pool = synth.make_pool("dense_fc", 10, n=50, t=64, f0=7)
    torch.manual_seed(1)
    m = GIN_InfoMaxReg(3, 2, 7, 32, 2, 0.0, learn_eps, "sum", npool, dev).to(dev).train()
    with torch.no_grad():
        m.eps.copy_(torch.tensor([0.3, -0.2, 0.1]))
    ar = m.arena()
    gids = [ar.add(g) for g in pool[:6]]
    for round_ in range(2):
        if round_ == 1:                                   # grow the arena: the cache must extend, not restart
            gids = gids[2:] + [ar.add(g) for g in pool[6:]]
        bt = ar.batch_from_gids(np.array(gids, dtype=np.int64))
        perm = np.arange(len(gids))[::-1].copy()
        outs = []
        for explicit in (False, True):
            m.zero_grad()
            X = ar.features(bt) if explicit else None
            c, d = m.forward_batch(bt, X=X, perm=perm)
            (c.square().sum() + d.square().mean()).backward()
            outs.append((c.detach().cpu().numpy(), d.detach().cpu().numpy(),
                         {k: p.grad.detach().cpu().numpy().copy() for k, p in m.named_parameters() if p.grad is not None}))
        assert_close(outs[0][0], outs[1][0], rtol=RTOL, what="c_logit")
        assert_close(outs[0][1], outs[1][1], rtol=RTOL, what="d_logit")
        gmax = max(np.abs(v).max() for v in outs[1][2].values())
        for k, v in outs[1][2].items():
            assert_close(outs[0][2][k], v, rtol=5e-5, what=k, floor=2e-2 * gmax)
        if learn_eps:
            assert abs(outs[0][2]["eps"][0]) > 0
    X, P0 = ar.features_and_agg0(bt, npool == "average", not learn_eps)
    assert P0 is not None and P0.shape == X.shape


def test_captured_step_refuses_a_reallocated_arena():
    """A captured step holds raw addresses of the arena's buffers: growing the arena afterwards must be reported,
    not silently read through stale pointers."""
    from gnm import synth
    from gnm.graphs import CapturedTrainStep
    from gnm.train import infomax_loss
    from models.graphcnn import GIN_InfoMaxReg
    dev = torch.device(DEV)
    pool = synth.make_pool("dense_fc", 4, n=40, t=64, f0=7)
    torch.manual_seed(0)
    m = GIN_InfoMaxReg(2, 2, 7, 32, 2, 0.0, True, "sum", "sum", dev).to(dev).train()
    for p in m.parameters():
        p.grad = torch.zeros_like(p)
    ar = m.arena()
    gids = np.array([ar.add(g) for g in pool], dtype=np.int64)
    bt = ar.batch_from_gids(gids)
    lab = torch.zeros(4, dtype=torch.int64, device=dev)
    cap = CapturedTrainStep(m, bt, lambda c, d, l: infomax_loss(c, d, l)[0])
    cap.run(bt, lab, np.arange(4))
    for g in synth.make_pool("dense_fc", 300, first=100, n=40, t=64, f0=7):      # enough to outgrow the buffers
        ar.add(g)
    with pytest.raises(RuntimeError, match="re-allocated"):
        cap.run(ar.batch_from_gids(gids), lab, np.arange(4))


@pytest.mark.parametrize("case", [c for c in CASES if c in ("true_s0_eps1_gsum_nsum", "true_s0_eps0_gsum_naverage",
                                                            "tiny_s0_eps1_gsum_nsum", "tiny_s1_eps0_gaverage_nsum",
                                                            "tiny_s0_bgn_eps1_gsum_nsum",
                                                            "tiny_s0_bgn_eps1_gaverage_naverage")])
def test_both_aggregation_paths_at_model_level(case, monkeypatch):
    """The same train step with every batch forced onto the CSR gather (what GNM_DENSE_FILL=2 does) and on the default
    dispatch (these dense golden graphs take the matrix-core kernel): logits and every gradient agree to fp32 rounding,
    and the gather run is held to the fp64 oracle like the default run is elsewhere -- the CSR kernels stay covered end
    to end now that dense batches no longer reach them."""
    from gnm import arena as arena_mod
    cfg, state, d = load_case(case)
    true_shape = case.startswith("true_")
    runs = {}
    for path, fill in (("auto", arena_mod.DENSE_MIN_FILL), ("gather", 2.0)):
        monkeypatch.setattr(arena_mod, "DENSE_MIN_FILL", fill)
        model = make_model(cfg, state).train()
        graphs = make_graphs(cfg, d)
        batch = model.arena().batch(graphs)
        assert batch.dense == (path == "auto"), (path, batch.dense)
        np.random.seed(cfg["np_seed"])
        c_logit, d_logit = model(graphs)
        loss = c_logit.square().mean() + 0.05 * d_logit.square().mean()
        loss.backward()
        runs[path] = dict(c=c_logit.detach().cpu().numpy(), d=d_logit.detach().cpu().numpy(),
                          g={k: p.grad.detach().cpu().numpy() for k, p in model.named_parameters() if p.grad is not None})
    tol = 20 * RTOL if true_shape else RTOL          # two fp32 implementations of a 5-layer net on 400-node graphs
    assert_close(runs["gather"]["c"], runs["auto"]["c"], rtol=tol, what="c_logit, gather vs matrix-core")
    assert_close(runs["gather"]["d"], runs["auto"]["d"], rtol=tol, what="d_logit, gather vs matrix-core")
    gmax = max(float(np.abs(g).max()) for g in runs["auto"]["g"].values())
    for k, g in runs["auto"]["g"].items():
        assert_close(runs["gather"]["g"][k], g, rtol=5e-3 if true_shape else 5e-5, what="grad " + k, floor=2e-2 * gmax)
