"""GIN_InfoMaxReg.shapley() (csrc/shapley.hip in front of and behind csrc/lesion.hip's unchanged forward): the keep
masks gnm_coalition_pack writes against gnm_lesion_pack on the explicit "removed" rows (bitwise); the coalition scores
against lesion() on the same sets (bitwise); phi and the interaction index against the fp64 oracle's game on explicit
set-deleted copies; the device reductions against gnm/shapley.py's restatement and a 2-additive game with known values;
the axioms (efficiency, null player, the empty coalition); the permutation mode; invariance to the batch size, the
chunking and the set of classes; NaN confinement; the declined shapes and the bad arguments.

Bounds.  b = the bound tests/test_gpu_lesion.py applies to ONE score: helpers.RTOL x the graph's max |score| for the
small shapes, helpers.Calibrated's max(RTOL, TRUE_SHAPE_FACTOR x err of the independent fp32 CPU forward against fp64 on
the same deleted graphs) x that scale for n = 400.  phi is a weighted sum, weights adding to 1, of differences of two
scores: |phi - phi64| <= 2 b; the interaction index of differences of four: |inter - inter64| <= 4 b.  The reductions
themselves are fp64 on both sides: 1e-11 x max |v| (the worst-case fp64 bound for 2^15 terms is 3.6e-12); efficiency
1e-9 x max |v| (worst case at K = 16: 2.3e-10).

MEASURED on an MI355X (every test prints its worst figure, pytest -s; also in DESIGN.md section 3.16): the small-shape
matrix scores 0.102 b, phi 0.043 b (bound 2 b), inter 0.069 b (bound 4 b); n = 400 one-hot 0.032 b, 0.007 b, 0.006 b with
b = 1e-5 x max |score| (the fp32 CPU forward is 4.0e-7 from fp64); the reductions against the restatement at most 2.8e-14
of max |v| (K = 16); efficiency 0 on the cases run; all 6 permutations of K = 3 against exact 1.1e-16."""
import itertools

import numpy as np
import pytest
import torch

from helpers import RTOL, TRUE_SHAPE_FACTOR, rel_err
from test_gpu_lesion import POOLS
from test_gpu_occlusion import spec_of, state64
from test_gpu_saliency import model_of, random_graph
from test_lesion_host import delete_nodes, expect_nan
from test_shapley_host import bg_graph, bg_labels, oracle_game, two_additive

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def nn7(t):
    return torch.nan_to_num(t, nan=7.0)


def bias_sum(model, classes):
    """sum_l linears_prediction[l].bias[c], added in fp32 in layer order from 0 (numpy)"""
    out = np.zeros(len(classes), dtype=np.float32)
    for lin in model.linears_prediction:
        out = (out + lin.bias.detach().cpu().numpy()[list(classes)]).astype(np.float32)
    return out


# ---------------------------------------------------------------------------------------------- 1. the pack kernel
def _pack_both(ns, labels, vgraph, ids, removed, K, ranks=None):
    """(masks, kept) of gnm_coalition_pack and of gnm_lesion_pack on `removed`, as numpy arrays"""
    from gnm._cabi import check, lib
    B, V, nm = len(ns), len(vgraph), max(ns)
    node_off = torch.as_tensor(np.concatenate([[0], np.cumsum(ns)]).astype(np.int32)).to(DEV)
    lab = np.full((B, nm), -1, dtype=np.int16)
    for b, l in enumerate(labels):
        lab[b, :ns[b]] = l
    rem = np.ones((V, nm), dtype=np.uint8)                        # entries past a graph's n: ignored by both
    for q, r in enumerate(removed):
        rem[q, :len(r)] = r
    lab_d, rem_d = torch.as_tensor(lab).to(DEV), torch.as_tensor(rem).to(DEV)
    vg_d = torch.as_tensor(np.asarray(vgraph, dtype=np.int32)).to(DEV)
    ids_d = torch.as_tensor(np.asarray(ids, dtype=np.int32)).to(DEV)
    ranks_d = torch.as_tensor(np.asarray(ranks, dtype=np.int16)).to(DEV) if ranks is not None else None
    mstride = int(lib.gnm_lesion_mask_words(nm))
    out = []
    for which in (0, 1):
        masks = torch.full((V, mstride), 0x5A5A5A5A, dtype=torch.int32, device=DEV)
        kept = torch.full((V,), -5, dtype=torch.int32, device=DEV)
        if which == 0:
            check(lib.gnm_coalition_pack(lab_d.data_ptr(), lab_d.stride(0), vg_d.data_ptr(), ids_d.data_ptr(),
                                         ranks_d.data_ptr() if ranks is not None else None,
                                         len(ranks) if ranks is not None else 0, K, node_off.data_ptr(), B, nm, V,
                                         mstride, masks.data_ptr(), kept.data_ptr(), None), "gnm_coalition_pack")
        else:
            check(lib.gnm_lesion_pack(rem_d.data_ptr(), rem_d.stride(0), vg_d.data_ptr(), node_off.data_ptr(), B, nm, V,
                                      mstride, masks.data_ptr(), kept.data_ptr(), None), "gnm_lesion_pack")
        torch.cuda.synchronize()
        out.append((masks.cpu().numpy(), kept.cpu().numpy()))
    return out


NS = (2, 33, 256, 257, 416)                                       # ragged in one batch; 256 | 257: the mask's 8 | 16 words


@pytest.mark.parametrize("K", [1, 4, 16])
def test_pack_identity_bitset(K):
    from gnm.shapley import coalition_removed, kept_counts
    rng = np.random.default_rng(K)
    labels, vgraph, ids, removed = [], [], [], []
    for b, n in enumerate(NS):
        lab = rng.integers(-1, K, n)                              # background among them
        if K > 1:
            lab[lab == 1] = 0 if b % 2 else -1                    # group 1 is empty in every graph
        labels.append(lab)
        pick = np.arange(1 << K) if K <= 4 else np.concatenate([[0, (1 << K) - 1], rng.integers(0, 1 << K, 30)])
        vgraph += [b] * len(pick)
        ids += pick.tolist()
        removed += list(coalition_removed(lab, pick))
    (m0, k0), (m1, k1) = _pack_both(NS, labels, vgraph, ids, removed, K)
    assert np.array_equal(m0, m1) and np.array_equal(k0, k1)      # every word up to mstride, and the kept counts
    want = np.concatenate([kept_counts(labels[b], K, ids=np.asarray(ids)[np.asarray(vgraph) == b]) for b in range(len(NS))])
    assert np.array_equal(k0, want)                               # the counts shapley_hip computes on the host


def test_pack_identity_prefix():
    from gnm.shapley import draw_permutations, kept_counts, prefix_removed, ranks_of
    rng = np.random.default_rng(9)
    for K, labels in ((416, [np.arange(n) for n in NS]),          # one player per node: K = n of the largest graph
                      (4, [np.where(rng.random(n) < 0.2, -1, rng.choice([0, 2, 3], n)) for n in NS])):
        perms = draw_permutations(3, K, seed=K)
        ranks = ranks_of(perms)
        vgraph, ids, removed, want = [], [], [], []
        for b, n in enumerate(NS):
            pr = prefix_removed(labels[b], perms)                 # [M, K + 1, n]
            kc = kept_counts(labels[b], K, perms=perms)
            js = sorted({0, 1, K // 2, K - 1, K} | set(rng.integers(0, K + 1, 6).tolist()))
            for m in range(3):
                for j in js:
                    vgraph.append(b)
                    ids.append(m * (K + 1) + j)
                    removed.append(pr[m, j])
                    want.append(kc[m, j])
        (m0, k0), (m1, k1) = _pack_both(NS, labels, vgraph, ids, removed, K, ranks=ranks)
        assert np.array_equal(m0, m1) and np.array_equal(k0, k1) and np.array_equal(k0, np.asarray(want))


# ---------------------------------------------------------------------------------------------- 2. values are lesions
def test_values_are_bitwise_lesion_scores():
    """n = 40 (a random graph with three background nodes that are NOT joined to every node: NaN coalitions under
    average + learned eps) and n = 257 in one ragged call, K = 4, every pooling form"""
    from gnm.shapley import coalition_removed
    K = 4
    gs = [random_graph(61, 40, 0.08, 7), bg_graph(62, 257, 0.03, 7)]
    labs = [bg_labels(63, 40, K, nbg=3), bg_labels(64, 257, K)]
    sets = [coalition_removed(l, np.arange(1 << K)) for l in labs]
    seen_nan = False
    for npool, gpool, le in POOLS:
        model = model_of(3, 2, 7, 64, le, gpool, npool, seed=21)
        phi, values = model.shapley(gs, (0, 1), labs, return_scores=True)
        _, _, les = model.lesion(gs, (0, 1), sets, return_scores=True)
        assert values.shape == (2, 2, 16) and values.dtype == torch.float32 and values.device.type == "cuda"
        assert phi.shape == (2, 2, K) and phi.dtype == torch.float64 and phi.device.type == "cuda"
        assert torch.equal(torch.isnan(values), torch.isnan(les)) and torch.equal(nn7(values), nn7(les))
        seen_nan |= bool(torch.isnan(values).any())
        assert torch.isfinite(values[:, 1]).all()
    assert seen_nan


# ---------------------------------------------------------------------------------------------- 3. the fp64 oracle
def _check_against_oracle(model, gs, labs, K, bound_rel=RTOL, v64=None):
    """phi, inter and the values of one call against the oracle's game; returns the worst errors relative to b"""
    from gnm.shapley import interactions_from_values, shapley_from_values
    phi, inter, values = model.shapley(gs, (0, 1), labs, interactions=True, return_scores=True)
    st, spec = state64(model), spec_of(model)
    worst = [0.0, 0.0, 0.0]
    for g, (gr, lab) in enumerate(zip(gs, labs)):
        r64 = v64[g] if v64 is not None else oracle_game(st, spec, gr, lab, K)      # [2^K, C]
        assert np.isfinite(r64).all()                             # nothing is silently dropped
        b = bound_rel * np.abs(r64).max()                         # one score's bound: the graph's max |score| (base among them)
        v = values[:, g].cpu().numpy()
        e0 = np.abs(v - r64.T).max()
        e1 = np.abs(phi[:, g].cpu().numpy() - shapley_from_values(r64.T, K)).max()
        e2 = np.abs(inter[:, g].cpu().numpy() - interactions_from_values(r64.T, K)).max()
        assert e0 <= b and e1 <= 2 * b and e2 <= 4 * b, (g, e0 / b, e1 / b, e2 / b)
        worst = [max(w, e / b) for w, e in zip(worst, (e0, e1, e2))]
    return worst


@pytest.mark.parametrize("L", [1, 3])
@pytest.mark.parametrize("m", [1, 2])
@pytest.mark.parametrize("H", [32, 64, 128])
def test_against_the_fp64_oracle(H, m, L):
    """the background-joined graphs of the host test (n = 40 and 33, F0 = 7, K = 4), every pooling form; the model
    seeds are test_gpu_lesion's, chosen there for conditioning"""
    K = 4
    gs = [bg_graph(5, 40, 0.2, 7), bg_graph(8, 33, 0.2, 7)]
    labs = [bg_labels(6, 40, K), bg_labels(9, 33, K)]
    worst = [0.0, 0.0, 0.0]
    for npool, gpool, le in POOLS:
        model = model_of(L, m, 7, H, le, gpool, npool, seed=200 + H + m)
        worst = [max(a, b) for a, b in zip(worst, _check_against_oracle(model, gs, labs, K))]
    print("H=%d m=%d L=%d: worst error / b: values %.3f, phi %.3f (<= 2), inter %.3f (<= 4)" % (H, m, L, *worst))


def test_against_the_fp64_oracle_400_nodes():
    """the reference's shape: a 400-node dense connectivity graph, one-hot features, sum / sum, H = 64, L = 5, a 7-group
    labelling with unlabelled nodes: 128 coalitions, each scored by the fp64 oracle on the explicit copy.  The
    calibration of helpers.Calibrated, as test_gpu_lesion.py's 400-node case: the independent fp32 CPU forward against
    fp64 on the same deleted graphs -- here on every 8th coalition and the full graph (that forward is the slow part;
    a maximum over fewer graphs can only make the bound tighter)"""
    from gnm import synth
    from gnm.shapley import coalition_removed
    from oracle import gin_oracle as O
    from oracle.gin_torch_cpu import TorchCpuGIN
    K = 7
    g = synth.dense_fc_graph(0, n=400)
    g.node_features = torch.eye(400)
    lab = bg_labels(3, 400, K, nbg=0, unlabelled=50)
    assert (lab == -1).sum() == 50 and set(lab.tolist()) == set(range(-1, K))
    model = model_of(5, 2, 400, 64, True, "sum", "sum", seed=7)
    st, spec = state64(model), spec_of(model)
    cpu = TorchCpuGIN({k: np.asarray(v, dtype=np.float32) if np.asarray(v).dtype.kind == "f" else v
                       for k, v in st.items()}, *spec)
    orc = O.OracleGIN(st, *spec, dtype=np.float64)
    r32, r64 = [], []
    cal = [i for i in range(1 << K) if i % 8 == 0 or i == (1 << K) - 1]
    for i, D in enumerate(coalition_removed(lab, np.arange(1 << K))):
        c = delete_nodes(g, D)
        og = O.OGraph(len(c.g), c.edge_mat.numpy(), c.node_features.numpy())
        with torch.no_grad(), np.errstate(all="ignore"):
            if i in cal:
                r32.append(cpu.forward([og], [0], training=False, want_disc=False)[0].numpy()[0])
            r64.append(orc.forward([og], np.arange(1), training=False, want_disc=False)[0][0])
    r32, r64 = np.stack(r32), np.stack(r64)
    noise = rel_err(r32, r64[cal], floor=float(np.abs(r64).max()))
    assert noise <= 1e-3
    bound_rel = max(RTOL, TRUE_SHAPE_FACTOR * noise)
    worst = _check_against_oracle(model, [g], [lab], K, bound_rel=bound_rel, v64=[r64])
    print("n=400: fp32 CPU forward %.2e from fp64, bound %.2e; worst error / b: values %.3f, phi %.3f, inter %.3f"
          % (noise, bound_rel, *worst))


# ---------------------------------------------------------------------------------------------- 4. the reductions
@pytest.mark.parametrize("K", [1, 2, 16])
def test_device_reduction_on_the_two_additive_game(K):
    """the kernels alone, no forward: [2 classes, 3 graphs] of 2-additive games with known phi and inter; K = 16
    exercises the bit-insert indexing at the cap"""
    from gnm.attribution import shapley_exact_hip
    from gnm.shapley import interactions_from_values, shapley_from_values
    games = [two_additive(K, 100 + s) for s in range(6)]
    v = np.stack([gm[0] for gm in games]).reshape(2, 3, 1 << K)
    want_phi = np.stack([gm[1] for gm in games]).reshape(2, 3, K)
    want_inter = np.stack([gm[2] for gm in games]).reshape(2, 3, K, K)
    vd = torch.as_tensor(v.astype(np.float32)).to(DEV)
    phi, inter = shapley_exact_hip(vd, K, interactions=True)
    phi2, none = shapley_exact_hip(vd, K)
    assert none is None and torch.equal(phi, phi2)
    scale = max(np.abs(v).max(), 1.0)
    e1 = np.abs(phi.cpu().numpy() - want_phi).max()
    e2 = np.abs(inter.cpu().numpy() - want_inter).max()
    e3 = np.abs(phi.cpu().numpy() - shapley_from_values(v.astype(np.float32), K)).max()
    e4 = np.abs(inter.cpu().numpy() - interactions_from_values(v.astype(np.float32), K)).max()
    print("K=%d: phi %.2e inter %.2e of max|v|; against the restatement %.2e %.2e"
          % (K, e1 / scale, e2 / scale, e3 / scale, e4 / scale))
    assert max(e1, e2, e3, e4) <= 1e-11 * scale
    it = inter.cpu().numpy()
    assert np.array_equal(it, it.transpose(0, 1, 3, 2)) and not it[..., np.arange(K), np.arange(K)].any()


# ---------------------------------------------------------------------------------------------- 5. the axioms
def test_axioms_efficiency_null_player_and_the_empty_coalition():
    from gnm.shapley import coalition_removed, interactions_from_values, shapley_from_values
    K = 5
    model = model_of(3, 2, 7, 64, False, "average", "sum", seed=31)
    gs = [bg_graph(71, 40, 0.2, 7), random_graph(72, 33, 0.2, 7), bg_graph(73, 70, 0.1, 7)]
    labs = [bg_labels(74, 40, K), np.arange(33) % K, bg_labels(75, 70, K)]
    labs[0][labs[0] == 3] = 2                                     # group 3 has no node in graph 0
    labs[1] = np.where(labs[1] == 1, 0, labs[1])                  # graph 1: no background, and group 1 empty
    phi, inter, values = model.shapley(gs, (0, 1), labs, interactions=True, return_scores=True, batch_size=3)
    assert torch.isfinite(values).all()
    v = values.cpu().numpy()
    scale = np.abs(v).max()
    eff = np.abs(phi.sum(-1).cpu().numpy() - (v[..., -1].astype(np.float64) - v[..., 0].astype(np.float64))).max()
    red = max(np.abs(phi.cpu().numpy() - shapley_from_values(v, K)).max(),
              np.abs(inter.cpu().numpy() - interactions_from_values(v, K)).max())
    print("efficiency %.2e, reduction against the restatement %.2e (of max |v|)" % (eff / scale, red / scale))
    assert eff <= 1e-9 * scale and red <= 1e-11 * scale
    # the null players: exactly 0.0, and an exactly zero interaction row and column
    for g, p in ((0, 3), (1, 1)):
        assert (phi[:, g, p] == 0.0).all() and (inter[:, g, p, :] == 0.0).all() and (inter[:, g, :, p] == 0.0).all()
    assert (phi[:, 2] != 0.0).all() and (phi[:, 0, :3] != 0.0).all()
    # v(empty): without background the bias sum, bitwise (also coalition {1} of graph 1: an empty group alone)
    want = bias_sum(model, (0, 1))
    assert np.array_equal(v[:, 1, 0], want) and np.array_equal(v[:, 1, 0b00010], want)
    # with background: lesion() of all labelled nodes, bitwise
    _, _, les = model.lesion([gs[0], gs[2]], (0, 1), [coalition_removed(labs[0], [0]), coalition_removed(labs[2], [0])],
                             return_scores=True)
    assert torch.equal(values[:, [0, 2], 0], les[:, :, 0])


def test_a_call_of_empty_coalitions_launches_nothing_and_a_mixed_call_scores_the_rest_alike(monkeypatch):
    """shapley_hip on coalitions that keep no node (every node labelled, no background).  Only such coalitions in the
    call: every score is the bias sum, bitwise, and neither the pack nor gnm_lesion runs.  Some of them among others:
    they get the bias sum, and the others the bits of a call that holds those others alone."""
    from gnm import attribution, core
    from gnm._cabi import lib
    K = 3
    model = model_of(1, 1, 7, 32, True, "sum", "sum", seed=61)
    gs = [random_graph(91 + i, 6, 0.4, 7) for i in range(2)]
    batch = model._batch_of(gs)
    X = batch.arena.features(batch).detach()
    P = model._named_tensors()
    labels = np.stack([np.arange(6) % K] * 2)
    calls = []
    for entry in ("gnm_lesion", "gnm_coalition_pack"):
        real = getattr(lib, entry)
        monkeypatch.setattr(core.lib, entry, lambda *a, real=real, entry=entry: calls.append(entry) or real(*a),
                            raising=False)
    want = torch.as_tensor(bias_sum(model, (0, 1)), device=DEV)

    def score(vgraph, ids):
        return attribution.shapley_hip(model._spec, batch, X, P, (0, 1), labels, np.asarray(vgraph), np.asarray(ids), K)
    out = score([0, 0, 1, 1], [0, 0, 0, 0])
    assert out.shape == (2, 4) and torch.equal(out, want[:, None].expand(2, 4))
    assert calls == []
    vgraph, ids = np.array([0, 0, 0, 1, 1, 1]), np.array([0, 0b011, 0b111, 0, 0b100, 0])
    mixed = score(vgraph, ids)
    assert calls == ["gnm_coalition_pack", "gnm_lesion"]
    run = ids != 0
    alone = score(vgraph[run], ids[run])
    assert torch.isfinite(alone).all() and torch.equal(mixed[:, torch.as_tensor(run, device=DEV)], alone)
    assert torch.equal(mixed[:, torch.as_tensor(~run, device=DEV)], want[:, None].expand(2, 3))
    assert calls == ["gnm_coalition_pack", "gnm_lesion"] * 2


# ---------------------------------------------------------------------------------------------- 6. permutation mode
def test_all_permutations_reproduce_the_exact_values():
    from gnm.shapley import permutation_from_values
    K = 3
    model = model_of(3, 2, 7, 64, True, "sum", "sum", seed=41)
    gs = [bg_graph(81 + i, 40, 0.2, 7) for i in range(2)]
    lab = bg_labels(83, 40, K)
    perms = np.array(list(itertools.permutations(range(K))))
    exact, ev = model.shapley(gs, (0, 1), lab, return_scores=True)
    mean, err, values = model.shapley(gs, (0, 1), lab, method="permutation", permutations=perms, return_scores=True)
    assert mean.shape == err.shape == (2, 2, K) and mean.dtype == err.dtype == torch.float64
    assert values.shape == (2, 2, 6, K + 1) and values.dtype == torch.float32
    scale = float(ev.abs().max())
    e = float((mean - exact).abs().max())
    print("all 6 permutations against exact: %.2e of max |v|" % (e / scale))
    assert e <= 1e-9 * scale
    for m, row in enumerate(perms):                               # entry (m, j): the coalition of the first j players, bitwise
        ids = np.concatenate([[0], np.cumsum(1 << row)])
        assert torch.equal(values[:, :, m], ev[:, :, ids])
    rm, re_ = permutation_from_values(values.cpu().numpy(), perms)
    assert np.abs(mean.cpu().numpy() - rm).max() <= 1e-11 * scale and np.abs(err.cpu().numpy() - re_).max() <= 1e-11 * scale
    one = model.shapley(gs, 1, torch.as_tensor(lab), method="permutation", permutations=torch.as_tensor(perms))
    assert torch.equal(one[0], mean[1]) and torch.equal(one[1], err[1])


def test_per_roi_players_sampled():
    from gnm.shapley import draw_permutations, permutation_from_values
    n, M = 33, 4
    model = model_of(3, 2, 7, 64, True, "sum", "sum", seed=42)
    gs = [random_graph(91 + i, n, 0.2, 7) for i in range(2)]
    lab = np.arange(n)
    np.random.seed(5)
    before = np.random.get_state()
    mean, err, values = model.shapley(gs, (0, 1), lab, method="permutation", permutations=M, seed=3, return_scores=True)
    now = np.random.get_state()
    assert before[0] == now[0] and np.array_equal(before[1], now[1]) and before[2:] == now[2:]
    assert mean.shape == err.shape == (2, 2, n) and values.shape == (2, 2, M, n + 1)
    v = values.cpu().numpy()
    scale = np.abs(v).max()
    assert np.isfinite(v).all()
    assert (v[:, :, :, 0] == v[:, :, :1, 0]).all() and (v[:, :, :, n] == v[:, :, :1, n]).all()   # v(empty), v(N): once
    assert np.array_equal(v[:, 0, 0, 0], bias_sum(model, (0, 1)))
    eff = np.abs(mean.sum(-1).cpu().numpy() - (v[:, :, 0, n].astype(np.float64) - v[:, :, 0, 0].astype(np.float64))).max()
    rm, re_ = permutation_from_values(v, draw_permutations(M, n, seed=3))
    e1, e2 = np.abs(mean.cpu().numpy() - rm).max(), np.abs(err.cpu().numpy() - re_).max()
    print("per-ROI: efficiency %.2e, mean %.2e, stderr %.2e (of max |v|)" % (eff / scale, e1 / scale, e2 / scale))
    assert eff <= 1e-9 * scale and e1 <= 1e-11 * scale and e2 <= 1e-11 * scale and (re_ > 0).all()
    again = model.shapley(gs, (0, 1), lab, method="permutation", permutations=M, seed=3, batch_size=1)
    assert torch.equal(again[0], mean) and torch.equal(again[1], err)
    other = model.shapley(gs, (0, 1), lab, method="permutation", permutations=M, seed=4)
    assert not torch.equal(other[0], mean)
    m1, e1_ = model.shapley(gs, 0, lab, method="permutation", permutations=1)
    assert m1.shape == (2, n) and torch.isnan(e1_).all() and torch.isfinite(m1).all()


# ---------------------------------------------------------------------------------------------- 7. determinism
def test_determinism_batch_size_chunks_and_classes(monkeypatch):
    from gnm import attribution, core
    from gnm._cabi import lib
    K = 6
    model = model_of(3, 2, 7, 64, True, "average", "average", seed=2, C=11)
    gs = [bg_graph(20 + i, n, 8.0 / n, 7) for i, n in enumerate((257, 40, 40, 70, 33))]
    labs = [bg_labels(30 + i, len(g.g), K) for i, g in enumerate(gs)]
    cls = tuple(range(11))
    p0, i0, v0 = model.shapley(gs, cls, labs, interactions=True, return_scores=True)
    assert torch.isfinite(v0).all() and v0.shape == (11, 5, 64) and i0.shape == (11, 5, K, K)
    for bs in (1, 3, 8, 8):                                       # (8 again: run to run)
        p, i, v = model.shapley(gs, cls, labs, interactions=True, return_scores=True, batch_size=bs)
        assert torch.equal(p, p0) and torch.equal(i, i0) and torch.equal(v, v0), bs
    for c in (0, 4, 10):                                          # one class at a time
        p, i, v = model.shapley(gs, c, labs, interactions=True, return_scores=True)
        assert torch.equal(p, p0[c]) and torch.equal(i, i0[c]) and torch.equal(v, v0[c])
    calls = []
    real = lib.gnm_lesion
    monkeypatch.setattr(core.lib, "gnm_lesion", lambda *a: calls.append(1) or real(*a), raising=False)
    monkeypatch.setattr(attribution, "LESION_SCRATCH_BYTES", 4 * int(lib.gnm_lesion_scratch_floats(7 * 257, 7, 257, 64, 3)))
    p, i, v = model.shapley(gs[:1], cls, labs[:1], interactions=True, return_scores=True)      # 64 coalitions, 7 to a chunk
    assert len(calls) == 10
    assert torch.equal(p, p0[:, :1]) and torch.equal(i, i0[:, :1]) and torch.equal(v, v0[:, :1])


# ---------------------------------------------------------------------------------------------- 8. NaN
def test_nan_coalitions_and_nan_features_stay_in_their_graph():
    from gnm.shapley import coalition_removed
    K = 4
    model = model_of(3, 2, 7, 64, True, "sum", "average", seed=5)  # neighbour average + learned eps
    gs = [bg_graph(51, 40, 0.2, 7), random_graph(52, 40, 0.08, 7), bg_graph(53, 33, 0.2, 7)]
    labs = [bg_labels(54, 40, K), bg_labels(55, 40, K, nbg=2), bg_labels(56, 33, K)]
    want = [any(expect_nan(g, D, "average", True) for D in coalition_removed(l, np.arange(1 << K)))
            for g, l in zip(gs, labs)]
    assert want == [False, True, False]
    phi, inter, values = model.shapley(gs, (0, 1), labs, interactions=True, return_scores=True)
    for g in range(3):
        assert bool(torch.isnan(phi[:, g]).all()) == want[g] and bool(torch.isnan(phi[:, g]).any()) == want[g]
        off = ~torch.eye(K, dtype=torch.bool, device=inter.device)
        assert bool(torch.isnan(inter[:, g][:, off]).all()) == want[g]
    assert not torch.isnan(values[:, 1]).all()                    # (only some coalitions of graph 1 are NaN)
    clean = model.shapley([gs[0], gs[2]], (0, 1), [labs[0], labs[2]])
    assert torch.equal(phi[:, [0, 2]], clean) and torch.isfinite(clean).all()
    bad = bg_graph(53, 33, 0.2, 7)                                # graph 2 again, as a new object
    bad.node_features[3, 2] = float("nan")                        # a non-finite feature: that graph only
    got = model.shapley([gs[0], gs[1], bad], (0, 1), labs)
    assert torch.isnan(got[:, 2]).all() and torch.equal(got[:, 0], phi[:, 0])


# ---------------------------------------------------------------------------------------------- 9. raises
def test_declined_shapes_and_bad_arguments_raise_with_their_reason():
    gs = [bg_graph(60 + i, 40, 0.2, 7) for i in range(2)]
    ok = bg_labels(62, 40, 3)
    model = model_of(2, 2, 7, 64, True, "sum", "sum", seed=1)
    with pytest.raises(ValueError, match="at most 16 groups, got 17; use method='permutation'"):
        model.shapley(gs, 0, np.arange(40) % 17)
    with pytest.raises(ValueError, match="interactions need method='exact'"):
        model.shapley(gs, 0, ok, method="permutation", permutations=2, interactions=True)
    with pytest.raises(ValueError, match="permutation of 0 .. 2"):
        model.shapley(gs, 0, ok, method="permutation", permutations=[[0, 1, 2], [0, 2, 2]])
    with pytest.raises(ValueError, match="39 labels for a 40-node graph"):
        model.shapley(gs, 0, ok[:-1])
    with pytest.raises(ValueError, match="int"):
        model.shapley(gs, 0, ok.astype(np.float32))
    with pytest.raises(ValueError, match="-1 for background"):
        model.shapley(gs, 0, np.where(ok == 0, -2, ok))
    with pytest.raises(ValueError, match="name no group"):
        model.shapley(gs, 0, np.full(40, -1))
    with pytest.raises(ValueError, match="one node count"):
        model.shapley(gs + [bg_graph(63, 20, 0.3, 7)], 0, ok)
    with pytest.raises(ValueError, match="max neighbour pooling"):
        model_of(2, 2, 7, 64, True, "sum", "max", seed=1).shapley(gs, 0, ok)
    with pytest.raises(ValueError, match="416"):
        model.shapley([random_graph(70, 420, 0.05, 7)], 0, np.arange(420) % 3)
    with pytest.raises(ValueError, match="hidden_dim 16"):
        model_of(2, 2, 7, 16, True, "sum", "sum", seed=1).shapley(gs, 0, ok)
    with pytest.raises(ValueError, match="num_mlp_layers"):
        model_of(2, 4, 7, 64, True, "sum", "sum", seed=1).shapley(gs, 0, ok)
    model._spec.sync_bn = object()
    with pytest.raises(ValueError, match="synchronised BatchNorm"):
        model.shapley(gs, 0, ok)
    model._spec.sync_bn = None
    with pytest.raises(ValueError, match="fewer than 2 nodes"):
        model.shapley(gs + [random_graph(71, 1, 0.5, 7)], 0, [ok, ok, np.zeros(1, dtype=np.int64)])
    assert model.shapley(gs, 0, ok).shape == (2, 3)               # and the model still works


@pytest.mark.parametrize("training", [True, False])
def test_no_side_effects(training):
    model = model_of(3, 2, 7, 64, True, "sum", "average", seed=3)
    model.train(training)
    gs = [bg_graph(30 + i, 40, 0.2, 7) for i in range(2)]
    lab = bg_labels(32, 40, 3)
    before = {k: v.clone() for k, v in model.state_dict().items()}
    np.random.seed(11)
    rng = np.random.get_state()
    phi, inter = model.shapley(gs, 0, lab, interactions=True)
    mean, err = model.shapley(gs, 0, lab, method="permutation", permutations=3)
    assert phi.shape == (2, 3) and inter.shape == (2, 3, 3) and mean.shape == err.shape == (2, 3)
    assert phi.device.type == "cuda" and not phi.requires_grad and not mean.requires_grad
    assert model.training == training
    assert all(p.grad is None for p in model.parameters())
    after = model.state_dict()
    assert all(torch.equal(before[k], after[k]) for k in before)
    now = np.random.get_state()
    assert rng[0] == now[0] and np.array_equal(rng[1], now[1]) and rng[2:] == now[2:]
