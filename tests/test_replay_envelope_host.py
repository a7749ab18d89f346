"""The CPU half of the replay envelope (tests/test_gpu_replay_envelope.py replays every case of
tests/train_envelope_cases.py from captured hipGraphs on a sequence of batches).  For every case, without a GPU:

  * the pool starts with the case's own graphs, unchanged, and every selection of the sequence is of the template's
    BatchClass -- B, N, n_max, n_min, symmetric, iso through GraphArena.class_of on a host arena, dense through
    train_envelope_cases.expected_dense (a host arena builds no bit rows), iso also through has_isolated -- so a
    capture admits every one of them and none runs eagerly by accident;
  * the StaticBatch template has the most edges in one graph, and at least two selections differ from the case's own
    batch in total edge count and in nnz_max: the launch-sizing argument frozen at capture is not the one an eager
    step on the same batch passes;
  * the heavier extra graph is refused by the StaticBatch template's class and admitted by the class
    PackedStaticBatch rounds it to;
  * which case is left out of which replay kind, and by which condition of the product (replay_exclusion, the one
    table both halves read), against the conditions in models/graphcnn.py and gnm/train.py;
  * the anchor selection of the five fp64-anchored cases keeps RELU_MARGIN."""
import numpy as np
import pytest
import torch

import train_envelope_cases as T

IDS = [c.id for c in T.CASES]


def _host_arena(pool):
    """a host arena over COPIES of the pool's graphs (the graphs are shared with every other test, and a graph
    remembers the arena it was added to)"""
    from gnm.arena import GraphArena
    from test_gpu_eval_envelope import EG
    arena = GraphArena("cpu")
    graphs = list(pool.graphs) + ([pool.heavy] if pool.heavy is not None else [])
    em = [g.edge_mat.numpy() for g in graphs]
    ids = arena.add_many([EG(g.num_nodes, e[0], e[1], g.node_features.numpy()) for g, e in zip(graphs, em)])
    assert ids == list(range(len(graphs)))
    return arena


def _bytes(g):
    return g.edge_mat.numpy().tobytes(), g.node_features.numpy().tobytes(), g.label


@pytest.mark.parametrize("case", T.CASES, ids=IDS)
def test_pool_and_selections_are_of_the_template_class(case):
    pool = T.case_pool(case)
    B = case.B
    assert len(pool.graphs) == T.pool_size(case) == (6 if case.n >= 400 else max(6, 3 * B))
    own = T.case_data(case).graphs
    assert all(a is b for a, b in zip(pool.graphs[:B], own))
    fresh, _ = T.case_graphs(case)       # the builder's results are what they were
    assert [_bytes(g) for g in fresh] == [_bytes(g) for g in own]
    assert len({_bytes(g)[:2] for g in pool.graphs}) >= (1 if case.kind == "regular" else len(pool.graphs))
    arena = _host_arena(pool)
    sel = pool.selections
    assert len(sel) == 5 and sel[0] == tuple(range(B)) == sel[3]
    assert not set(sel[1]) & set(sel[0])
    if B >= 2:
        assert set(sel[2]) & set(sel[0]) and max(sel[2].count(j) for j in sel[2]) == 2
        assert list(sel[4]) == sorted(sel[4], reverse=True) and len(set(sel[4])) == B
    tcls = arena.class_of(np.asarray(sel[pool.template], dtype=np.int64))
    tgraphs = [pool.graphs[j] for j in sel[pool.template]]
    dense, iso = T.expected_dense(case, tgraphs), T.has_isolated(tgraphs)
    # (the tiny graphs of the discriminator cases, n = 6 and 8, have a node without neighbours by chance as well)
    assert iso == tcls.iso and (iso or case.kind != "iso")
    positions = set()
    for s, ids in enumerate(sel):
        assert len(ids) == B
        cls = arena.class_of(np.asarray(ids, dtype=np.int64))
        for f in ("B", "N", "n_max", "n_min", "symmetric", "iso"):
            assert getattr(cls, f) == getattr(tcls, f), (s, f)
        graphs = [pool.graphs[j] for j in ids]
        assert T.expected_dense(case, graphs) == dense, s
        assert T.has_isolated(graphs) == iso, s
        assert cls.nnz_max <= tcls.nnz_max, s
        assert cls.nnz_max == max(g.edge_mat.shape[1] for g in graphs)
        positions |= {k for k, j in enumerate(ids) if T.has_isolated([pool.graphs[j]])}
        assert len(pool.labels[s]) == B and ((0 <= pool.labels[s]) & (pool.labels[s] < case.C)).all()
        assert sorted(pool.perms[s].tolist()) == list(range(B))
        assert B == 1 or not np.array_equal(pool.perms[s], np.arange(B))
    if case.kind == "iso":
        assert positions == {0, 1}       # the isolated graph sits at more than one batch position
    # the frozen launch-sizing argument differs from the eager one.  (A circulant graph -- kind "regular", there for
    # neighbour max alone, which never replays -- has one edge count by construction.)
    if case.kind != "regular":
        own_cls = arena.class_of(np.asarray(sel[0], dtype=np.int64))
        total = lambda ids: sum(pool.graphs[j].edge_mat.shape[1] for j in ids)          # noqa: E731
        differ = [s for s in (1, 2, 4) if total(sel[s]) != total(sel[0])
                  and arena.class_of(np.asarray(sel[s], dtype=np.int64)).nnz_max != own_cls.nnz_max]
        assert len(differ) >= 2, differ
    else:
        assert case.npool == "max"


@pytest.mark.parametrize("case", [c for c in T.CASES if c.kind not in ("iso", "multi")],
                         ids=[c.id for c in T.CASES if c.kind not in ("iso", "multi")])
def test_heavier_graph_is_refused_by_the_static_class_and_admitted_by_the_packed_one(case):
    from gnm.arena import PackedStaticBatch
    pool = T.case_pool(case)
    arena = _host_arena(pool)
    heavy_id = len(pool.graphs)
    assert pool.heavy.edge_mat.shape[1] > max(g.edge_mat.shape[1] for g in pool.graphs)
    tids = np.asarray(pool.selections[pool.template], dtype=np.int64)
    tcls = arena.class_of(tids)
    ids = np.asarray((heavy_id,) + pool.selections[1][1:], dtype=np.int64)
    cls = arena.class_of(ids)
    graphs = [pool.heavy] + [pool.graphs[j] for j in pool.selections[1][1:]]
    assert cls[:-1] == tcls[:-1]                     # the same class but for the edge count ...
    assert T.expected_dense(case, graphs) == T.expected_dense(case, [pool.graphs[j] for j in tids])
    assert T.has_isolated(graphs) == tcls.iso
    assert not tcls.admits(cls)
    packed = PackedStaticBatch(arena, tcls)
    assert packed.batch_class.nnz_max == max(4096, 1 << (tcls.nnz_max - 1).bit_length())
    assert packed.batch_class.admits(cls) and packed.fits(ids)


def test_none_of_the_case_table_is_absent_from_the_pools():
    for case in T.CASES:
        assert (T.case_pool(case).heavy is None) == (case.kind in ("iso", "multi"))


@pytest.mark.parametrize("case", T.CASES, ids=IDS)
def test_exclusions_match_the_product_conditions(case):
    """replay_exclusion against the conditions themselves: forward()'s guards and _forward_train_replay's first line
    (models/graphcnn.py), FusedTrainStep's constructor (gnm/train.py)"""
    from gnm.core import GinSpec
    from models.graphcnn import GIN_InfoMaxReg
    spec = GinSpec(case.L, case.m, case.eps, case.gpool, case.npool)
    spec.keep_hidden = case.keep
    spec.grad_sink = {} if case.sink else None
    n_max = bool(spec.n_max)
    assert n_max == (case.npool == "max")
    want = {
        "step": n_max, "fused": n_max,
        "train": n_max or spec.grad_sink is not None or spec.sync_bn is not None or bool(spec.keep_hidden)
        or not 0 < case.B <= GIN_InfoMaxReg.TRAIN_REPLAY_MAX_B,
        "eval": n_max or not 0 < case.B <= GIN_InfoMaxReg.EVAL_REPLAY_MAX_B,
    }
    for kind in T.REPLAY_KINDS:
        why = T.replay_exclusion(case, kind)
        assert (why is not None) == want[kind], (kind, why)
        assert why is None or isinstance(why, str) and why


def test_exclusion_table_names_every_case_left_out():
    out = {k: [c.id for c in T.CASES if T.replay_exclusion(c, k)] for k in T.REPLAY_KINDS}
    maxp = [c.id for c in T.CASES if c.npool == "max"]
    assert out["step"] == out["fused"] == out["eval"] == maxp and len(maxp) == 10
    assert sorted(set(out["train"]) - set(maxp)) == sorted(
        c.id for c in T.CASES if (c.keep or c.sink) and c.npool != "max")
    assert {"keep-hidden-on", "keep-hidden-on-H128-unfused", "grad-sink-H64", "grad-sink-H128-eps0"} <= set(out["train"])
    # every route of the train envelope that is not neighbour max is replayed by a case of each kind
    for kind in T.REPLAY_KINDS:
        seen = set()
        for c in T.CASES:
            if T.replay_exclusion(c, kind) is None:
                r = T.expected_route(c)
                for seq in r["fwd"] + list(r["bwd"].values()) + list(r["lin"].values()) + [r["head"], r["disc"]]:
                    seen.update(seq)
        for entry in ("gnm_aggm:0", "gnm_agg:0", "gnm_aggm:-2", "gnm_aggm_fwd_bnrelu:0", "gnm_agg_fwd_bnrelu:0",
                      "gnm_agg_fwd_bnrelu:-2", "gnm_aggm_bwd_stats:0", "gnm_agg_bwd_stats:0", "gnm_agg_bwd_stats:-2",
                      "gnm_linear_bwd_fused_rz:0", "gnm_linear_bwd_fused:0", "gnm_linear_bwd_fused[sums]:0",
                      "gnm_linear_wgrad:0", "gnm_linear_dgrad_masked:0", "gnm_linear_fwd[dgrad]:0", "gnm_head_fwd:0",
                      "gnm_head_fwd:-2", "gnm_disc_score_fwd_unit:0", "gnm_disc_score_fwd:0", "gnm_disc_unit_scale:0",
                      "gnm_disc_score_bwd:0"):
            assert entry in seen, (kind, entry)


@pytest.mark.parametrize("id_", T.ANCHOR_CASES)
def test_anchor_selection_keeps_the_relu_margin(id_):
    case = T.BY_ID[id_]
    assert case.drop == 0 and case.L <= 5 and case.n <= 70 and T.replay_exclusion(case, "step") is None
    s, ref = T.anchor(id_)
    _, margin = T.selection_oracle(case, s)
    assert margin >= T.RELU_MARGIN
    assert s != 0 and T.case_pool(case).selections[s] != T.case_pool(case).selections[0]
    print("%s: anchored on selection %d (margin %.2e, pool draw %d)" % (id_, s, margin, T.case_pool(case).redraw))
    assert np.isfinite(ref["c_logit"]).all()


def test_fixed_dropout_resident_form_applies_the_same_masks():
    import torch.nn.functional as F
    from helpers import fixed_dropout
    masks = (np.arange(24).reshape(2, 3, 4) % 3 == 0).astype(np.float32) / np.float32(0.6)
    x = torch.arange(24, dtype=torch.float32).reshape(2, 3, 4) - 7
    orig = F.dropout
    with fixed_dropout(masks):
        a = F.dropout(x, 0.4, True)
    with fixed_dropout(masks, device="cpu"):
        b = F.dropout(x, 0.4, True)
    with fixed_dropout(torch.from_numpy(masks)):
        c = F.dropout(x, 0.4, True)
    assert F.dropout is orig
    assert a.numpy().tobytes() == b.numpy().tobytes() == c.numpy().tobytes()
