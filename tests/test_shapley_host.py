"""CPU checks of GIN_InfoMaxReg.shapley() (Shapley values of ROI networks): gnm/shapley.py -- the weights, the fp64
restatements of the device reductions against independent formulations (all K! orders; a 2-additive game with known
values), the explicit "removed" masks of coalitions and their kept counts -- the game itself on the fp64 oracle over
explicit set-deleted copies (finite on every pooling form, efficient), the empty-graph convention, the new C-ABI entries
and argument validation: everything that does not need a GPU.  The graph builders and the oracle game are shared with
tests/test_gpu_shapley.py."""
import itertools
import os
import re

import numpy as np
import pytest
import torch

from test_lesion_host import _G, _cpu_model, masked_forward64, oracle_lesion

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("gnm_coalition_pack", "gnm_shapley_exact", "gnm_shapley_permutation")
POOLS = [(np_, gp, le) for np_ in ("sum", "average") for gp in ("sum", "average") for le in (True, False)]
BG = 4                                                            # background nodes of the oracle game's graphs


def bg_graph(seed, n, p, f0, nbg=BG, one_hot=False):
    """A random undirected n-node graph with a ring whose LAST nbg nodes are joined to every node: labelled -1
    (background, never removed) they leave every kept node a kept neighbour, so no coalition scores 0/0 NaN."""
    rng = np.random.default_rng(seed)
    A = rng.random((n, n)) < p
    A[np.arange(n), (np.arange(n) + 1) % n] = True
    A[n - nbg:, :] = True
    A = np.triu(A | A.T, 1)
    A = A | A.T
    src, dst = np.nonzero(A)
    g = _G()
    g.g = list(range(n))
    g.label = int(rng.integers(0, 2))
    g.edge_mat = torch.as_tensor(np.stack([src, dst]).astype(np.int64))
    g.node_features = torch.as_tensor(np.eye(n, dtype=np.float32) if one_hot
                                      else rng.standard_normal((n, f0)).astype(np.float32))
    nb = [[] for _ in range(n)]
    for a, b in zip(src, dst):
        nb[a].append(int(b))
    g.neighbors, g.max_neighbor = nb, max(len(x) for x in nb)
    return g


def bg_labels(seed, n, K, nbg=BG, unlabelled=0):
    """labels of bg_graph's nodes: random groups 0 .. K - 1 (each at least once), `unlabelled` further -1 entries, and
    -1 on the last nbg nodes"""
    rng = np.random.default_rng(seed)
    lab = rng.integers(0, K, n).astype(np.int64)
    lab[rng.permutation(n - nbg)[:K]] = np.arange(K)
    if unlabelled:
        lab[rng.permutation(n - nbg)[K:K + unlabelled]] = -1
    lab[n - nbg:] = -1
    return lab


def cpu_state(L, m, f0, H, learn_eps, gpool, npool, seed, C=2):
    """a seeded model's fp64 state dict with running statistics, affines and eps away from their defaults"""
    from models.graphcnn import GIN_InfoMaxReg
    torch.manual_seed(seed)
    model = GIN_InfoMaxReg(L, m, f0, H, C, 0.5, learn_eps, gpool, npool, torch.device("cpu"))
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for name, b in model.named_buffers():
            if name.endswith("running_mean"):
                b.copy_(0.1 * torch.randn(b.shape, generator=g))
            elif name.endswith("running_var"):
                b.copy_(0.5 + torch.rand(b.shape, generator=g))
        for name, p in model.named_parameters():
            if "batch_norms" in name:
                p.add_(0.1 * torch.randn(p.shape, generator=g))
        if learn_eps:
            model.eps.copy_(0.2 * torch.randn(L, generator=g))
    return {k: v.numpy().astype(np.float64) if v.dtype.is_floating_point else v.numpy()
            for k, v in model.state_dict().items()}


def oracle_game(state, args, graph, labels, K):
    """values64 [2^K, C]: the fp64 oracle's score of every coalition of `labels` on explicit set-deleted copies"""
    from gnm.shapley import coalition_removed
    sets = coalition_removed(labels, np.arange(1 << K))
    assert not sets.all(1).any()                                  # (background: never the whole graph)
    return oracle_lesion(state, args, [graph], [sets])[1][0]


def two_additive(K, seed):
    """(values [2^K] of v(S) = sum_{i in S} a_i + sum_{i<j in S} b_ij with small integer a, b; phi; inter)"""
    rng = np.random.default_rng(seed)
    a = rng.integers(-3, 4, K).astype(np.float64)
    b = np.triu(rng.integers(-2, 3, (K, K)), 1).astype(np.float64)
    b = b + b.T
    ids = np.arange(1 << K, dtype=np.int64)
    bits = ((ids[:, None] >> np.arange(K)[None, :]) & 1).astype(np.float64)       # [2^K, K]
    v = bits @ a + 0.5 * np.einsum("si,ij,sj->s", bits, b, bits)
    return v, a + 0.5 * b.sum(1), b


# ---------------------------------------------------------------------------------------------- gnm/shapley.py
def test_weights_sum_to_one_over_the_subsets():
    import math
    from gnm.shapley import interaction_weights, shapley_weights
    for K in (1, 2, 5, 16):
        w = shapley_weights(K)
        assert w.dtype == np.float64 and w.shape == (K,)
        assert abs(sum(math.comb(K - 1, s) * w[s] for s in range(K)) - 1.0) < 1e-15
        u = interaction_weights(K)
        assert u.shape == (K - 1,)
        if K > 1:
            assert abs(sum(math.comb(K - 2, s) * u[s] for s in range(K - 1)) - 1.0) < 1e-15
    assert shapley_weights(3).tolist() == [1 / 3, 1 / 6, 1 / 3]
    with pytest.raises(ValueError):
        shapley_weights(0)


@pytest.mark.parametrize("K", [1, 2, 3, 4, 5])
def test_shapley_from_values_is_the_mean_over_all_orders(K):
    from gnm.shapley import shapley_from_values
    v = np.random.default_rng(K).standard_normal((3, 1 << K)).astype(np.float32)
    want = np.zeros((3, K))
    orders = list(itertools.permutations(range(K)))
    for order in orders:
        S = 0
        for i in order:
            want[:, i] += v[:, S | (1 << i)].astype(np.float64) - v[:, S].astype(np.float64)
            S |= 1 << i
    want /= len(orders)
    got = shapley_from_values(v, K)
    assert got.dtype == np.float64 and got.shape == (3, K)
    assert np.abs(got - want).max() <= 1e-13 * np.abs(v).max()


@pytest.mark.parametrize("K", [2, 6, 16])
def test_two_additive_game_has_known_values_and_interactions(K):
    from gnm.shapley import interactions_from_values, shapley_from_values
    v, phi, inter = two_additive(K, 40 + K)
    v32 = v.astype(np.float32)
    assert np.array_equal(v32.astype(np.float64), v)              # small integers and halves: exact in fp32
    scale = np.abs(v).max()
    assert np.abs(shapley_from_values(v32, K) - phi).max() <= 1e-11 * scale
    got = interactions_from_values(v32, K)
    assert np.abs(got - inter).max() <= 1e-11 * scale
    assert np.array_equal(got, got.T) and not got.diagonal().any()
    assert interactions_from_values(np.zeros(2, dtype=np.float32), 1).tolist() == [[0.0]]


def test_permutation_restatement():
    from gnm.shapley import permutation_from_values, shapley_from_values
    K = 3
    v = np.random.default_rng(3).standard_normal(1 << K).astype(np.float32)
    perms = np.array(list(itertools.permutations(range(K))))
    vals = np.zeros((len(perms), K + 1), dtype=np.float32)
    for m, row in enumerate(perms):
        S = 0
        vals[m, 0] = v[0]
        for j, i in enumerate(row):
            S |= 1 << i
            vals[m, j + 1] = v[S]
    mean, err = permutation_from_values(vals, perms)
    assert np.abs(mean - shapley_from_values(v, K)).max() <= 1e-13 * np.abs(v).max()
    d = np.stack([[float(vals[m, list(row).index(i) + 1]) - float(vals[m, list(row).index(i)]) for i in range(K)]
                  for m, row in enumerate(perms)])
    assert np.allclose(err, d.std(0, ddof=1) / np.sqrt(len(perms)), rtol=1e-12, atol=0)
    _, e1 = permutation_from_values(vals[:1], perms[:1])
    assert np.isnan(e1).all()


def test_removed_masks_and_kept_counts():
    from gnm.shapley import (check_labels, check_permutations, coalition_removed, draw_permutations, kept_counts,
                             prefix_removed, ranks_of)
    lab = np.array([0, 2, -1, 0, 2, 2, -1])                       # background, and group 1 empty
    K = 3
    ids = np.arange(1 << K)
    rm = coalition_removed(lab, ids)
    assert rm.shape == (8, 7) and rm.dtype == np.bool_
    assert not rm[:, [2, 6]].any()                                # background stays
    assert rm[0].tolist() == [True, True, False, True, True, True, False] and not rm[7].any()
    assert rm[0b001].tolist() == [False, True, False, False, True, True, False]
    assert np.array_equal(rm[0b010], rm[0]) and np.array_equal(rm[0b101], rm[0b111])      # the empty group: a null player
    assert np.array_equal(kept_counts(lab, K, ids=ids), (~rm).sum(1))
    perms = np.array([[1, 2, 0], [0, 1, 2]])
    pr = prefix_removed(lab, perms)
    assert pr.shape == (2, 4, 7)
    assert np.array_equal(pr[0, 0], rm[0]) and np.array_equal(pr[0, 1], rm[0b010]) and np.array_equal(pr[0, 2], rm[0b110])
    assert not pr[:, 3].any() and np.array_equal(pr[1, 1], rm[0b001])
    assert np.array_equal(kept_counts(lab, K, perms=perms), (~pr).sum(2))
    assert ranks_of(perms).tolist() == [[2, 0, 1], [0, 1, 2]]
    n = 9                                                         # one player per node
    lab = np.arange(n)
    perms = draw_permutations(3, n, seed=5)
    assert np.array_equal(perms, draw_permutations(3, n, seed=5)) and not np.array_equal(perms, draw_permutations(3, n, 6))
    pr = prefix_removed(lab, perms)
    for m in range(3):
        for j in range(n + 1):
            assert sorted(np.nonzero(~pr[m, j])[0].tolist()) == sorted(perms[m, :j].tolist())
    assert np.array_equal(kept_counts(lab, n, perms=perms), np.broadcast_to(np.arange(n + 1), (3, n + 1)))
    rm = coalition_removed(lab, [0, 0b101, (1 << n) - 1])
    assert rm.sum(1).tolist() == [n, n - 2, 0] and kept_counts(lab, n, ids=[0, 0b101, (1 << n) - 1]).tolist() == [0, 2, n]
    for bad in (np.array([0.0, 1.0]), np.array([[0, 1]]), np.array([0, -2])):
        with pytest.raises(ValueError):
            check_labels(bad)
    with pytest.raises(ValueError):
        check_labels(np.array([0, 1]), 3)
    for bad in ([[0, 0, 1]], [[0, 1, 3]], [[0, 1]], [0, 1, 2], np.zeros((0, 3), dtype=np.int64), [[0.0, 1.0, 2.0]]):
        with pytest.raises(ValueError):
            check_permutations(np.asarray(bad), 3)
    with pytest.raises(ValueError):
        prefix_removed(np.array([0, 3]), np.array([[0, 1, 2]]))


def test_drawing_permutations_leaves_the_global_rng_alone():
    from gnm.shapley import draw_permutations
    np.random.seed(3)
    before = np.random.get_state()
    draw_permutations(4, 7, seed=1)
    now = np.random.get_state()
    assert before[0] == now[0] and np.array_equal(before[1], now[1]) and before[2:] == now[2:]


# ---------------------------------------------------------------------------------------------- the game on the oracle
@pytest.mark.parametrize("npool,gpool,le", POOLS)
def test_game_on_the_oracle_is_finite_and_efficient(npool, gpool, le):
    """K = 4 groups of a 40-node graph with four background nodes joined to every node: every one of the 16 coalition
    scores is finite on every pooling form (so the GPU comparison drops nothing), and the fp64 Shapley values are
    efficient"""
    from gnm.shapley import interactions_from_values, shapley_from_values
    K, n = 4, 40
    args = (3, 2, le, gpool, npool)
    state = cpu_state(3, 2, 7, 64, le, gpool, npool, seed=11)
    g, lab = bg_graph(5, n, 0.2, 7), bg_labels(6, n, K)
    v = oracle_game(state, args, g, lab, K)                       # [16, C]
    assert v.shape == (16, 2) and np.isfinite(v).all()
    phi = shapley_from_values(v.T, K)                             # [C, K]
    scale = np.abs(v).max()
    assert np.abs(phi.sum(1) - (v[-1] - v[0])).max() <= 1e-12 * scale
    inter = interactions_from_values(v.T, K)
    assert np.array_equal(inter, inter.transpose(0, 2, 1)) and np.abs(inter).max() > 0


def test_empty_graph_convention_is_the_bias_sum():
    """a coalition that keeps no node: the head's score of a zero pooled vector at every layer, sum_l bias_l[c] -- what
    the zeroed-rows formulation gives under graph "sum" pooling, whatever the neighbour pooling"""
    from gnm.shapley import coalition_removed, kept_counts
    n, K = 12, 3
    g = bg_graph(7, n, 0.3, 7, nbg=0)
    lab = np.arange(n) % 2                                        # no background; group 2 is empty
    assert kept_counts(lab, K, ids=[0, 0b100, 0b001]).tolist() == [0, 0, 6]
    assert coalition_removed(lab, [0b100]).all()
    for npool, le in (("sum", True), ("average", True), ("average", False)):
        state = cpu_state(3, 2, 7, 32, le, "sum", npool, seed=2)
        want = sum(state["linears_prediction.%d.bias" % l] for l in range(3))
        got = masked_forward64(state, (3, 2, le, "sum", npool), g, np.ones(n, dtype=bool))
        assert np.abs(got - want).max() <= 1e-15 * np.abs(want).max()


# ---------------------------------------------------------------------------------------------- the C ABI
def test_shapley_entries_declared_bound_and_exported():
    from gnm import _build, _cabi
    header = open(os.path.join(ROOT, "include", "gnm_hip.h")).read()
    declared = set(re.findall(r"\b(gnm_[a-z0-9_]+)\s*\(", header))
    for name in NEW:
        assert name in declared and name in _cabi.SIGNATURES
        assert getattr(_cabi.lib, name) is not None
    assert "shapley.hip" in _build.SOURCES


def test_shapley_kernels_in_the_code_object(tmp_path):
    from test_isa_hazards import disassemble
    asm = disassemble(tmp_path)
    assert re.search(r"gnm_coalition_pack_kernelILb0EE", asm) and re.search(r"gnm_coalition_pack_kernelILb1EE", asm)
    for k in ("gnm_shapley_phi_kernel", "gnm_shapley_inter_kernel", "gnm_shapley_permutation_kernel"):
        assert re.search(k, asm), k


def test_shapley_bad_arguments_launch_nothing():
    """every check runs before a pointer is touched (a non-NULL placeholder is never dereferenced)"""
    from gnm._cabi import lib
    p = 1 << 20

    def pack(labels=p, ldl=400, ranks=None, M=0, K=7, B=1, n_max=400, V=20, mstride=16, masks=p):
        return lib.gnm_coalition_pack(labels, ldl, p, p, ranks, M, K, p, B, n_max, V, mstride, masks, p, None)
    assert pack(B=0) == 0 and pack(V=0) == 0                      # nothing to do
    assert pack(n_max=417) == -2 and pack(n_max=0) == -2
    assert pack(ldl=399) == -1 and pack(mstride=8) == -1 and pack(mstride=24) == -1
    assert pack(labels=None) == -1 and pack(masks=None) == -1 and pack(B=-1) == -1
    assert pack(K=0) == -1 and pack(K=33) == -1                   # the bitset form: 1 .. 32
    assert pack(ranks=p, M=2, K=0) == -1 and pack(ranks=p, M=2, K=417) == -1 and pack(ranks=p, M=0, K=5) == -1
    w = np.ones(16)

    def exact(scores=p, lds=8 * 128, C=2, G=8, K=7, w_=w.ctypes.data, u=w.ctypes.data, phi=p, inter=p):
        return lib.gnm_shapley_exact(scores, lds, C, G, K, w_, u, phi, inter, None)
    assert exact(C=0) == 0 and exact(G=0) == 0
    assert exact(K=0) == -2 and exact(K=17) == -2
    assert exact(lds=8 * 128 - 1) == -1 and exact(scores=None) == -1 and exact(w_=None) == -1 and exact(phi=None) == -1
    assert exact(u=None) == -1 and exact(C=-1) == -1

    def perm(scores=p, lds=8 * 4 * 8, C=2, G=8, M=4, K=7, ranks=p, mean=p, err=p):
        return lib.gnm_shapley_permutation(scores, lds, C, G, M, K, ranks, mean, err, None)
    assert perm(C=0) == 0 and perm(G=0) == 0
    assert perm(K=0) == -2 and perm(K=417) == -2
    assert perm(M=0) == -1 and perm(lds=8 * 4 * 8 - 1) == -1
    assert perm(scores=None) == -1 and perm(ranks=None) == -1 and perm(mean=None) == -1 and perm(err=None) == -1


# ---------------------------------------------------------------------------------------------- the method
def test_shapley_argument_validation():
    m, gs = _cpu_model()
    n = len(gs[0].g)
    ok = np.arange(n) % 3
    small = _G()
    small.g, small.edge_mat = [0, 1, 2], torch.tensor([[0, 1, 1, 2], [1, 0, 2, 1]])
    small.node_features = gs[0].node_features[:3]
    wide = np.arange(n) % 17 if n >= 17 else None
    bad = [(dict(graphs=[], cls=0), "empty list"), (dict(cls=2), "class"), (dict(cls=()), "classes"),
           (dict(cls=0, batch_size=0), "batch_size"),
           (dict(cls=0, method="kernel"), "method"),
           (dict(cls=0, labels=ok[:-1]), "labels for a"),                         # the wrong length
           (dict(cls=0, labels=ok.astype(np.float64)), "int"),                    # the wrong dtype
           (dict(cls=0, labels=np.where(ok == 0, -2, ok)), "-1"),                 # below -1
           (dict(cls=0, labels=np.full(n, -1)), "name no group"),
           (dict(cls=0, labels=[ok] * (len(gs) - 1)), "per graph"),
           (dict(graphs=gs + [small], cls=0), "one node count"),                  # a shared labelling over ragged graphs
           (dict(cls=0, interactions=True, method="permutation", permutations=2), "interactions"),
           (dict(cls=0, method="permutation"), "needs permutations"),
           (dict(cls=0, method="permutation", permutations=0), "positive"),
           (dict(cls=0, method="permutation", permutations=[[0, 1, 1]]), "permutation of 0"),
           (dict(cls=0, method="permutation", permutations=[[0, 1]]), r"\[M, 3\]"),
           (dict(cls=0, permutations=3), "belong to")]
    if wide is not None:
        bad.append((dict(cls=0, labels=wide), "at most 16 groups, got 17; use method='permutation'"))
    for kw, why in bad:
        kw = dict(kw)
        graphs = kw.pop("graphs", gs)
        labels = kw.pop("labels", ok)
        with pytest.raises(ValueError, match=why):
            m.shapley(graphs, labels=labels, **kw)
    assert m.training                                       # validation fails before the mode changes


def test_exact_cap_names_the_cap_and_the_way_out():
    from models.graphcnn import GIN_InfoMaxReg
    m = GIN_InfoMaxReg(2, 2, 7, 32, 2, 0.0, True, "sum", "sum", torch.device("cpu"))
    g = bg_graph(1, 20, 0.3, 7)
    with pytest.raises(ValueError, match="at most 16 groups, got 17; use method='permutation'"):
        m.shapley([g], 0, np.arange(20) % 17)


def test_shapley_has_no_cpu_fallback_and_restores_the_mode():
    from gnm._cabi import GnmError
    m, gs = _cpu_model()
    n = len(gs[0].g)
    for training in (True, False):
        m.train(training)
        with pytest.raises(GnmError):
            m.shapley(gs, (0, 1), np.arange(n) % 2)
        with pytest.raises(GnmError):
            m.shapley(gs, 0, np.arange(n) % 2, method="permutation", permutations=2)
        assert m.training == training
