"""The batch class a captured replay is specialised to (gnm/arena.py BatchClass): one definition, one predicate, and
every user of it -- StaticBatch.load, PackedStaticBatch.fits, CapturedTrainStep -- refusing the same batches.  Host
arenas only: the class is worked out from host tables."""
import numpy as np
import pytest
import torch

N = 400


def _band(n=N, w=1, one_way=False, isolated=False):
    """node i linked to i+1 .. i+w (mod the cycle length), both ways unless one_way; isolated: the last node left out"""
    k = n - 1 if isolated else n
    src = np.repeat(np.arange(k), w)
    dst = (src + np.tile(np.arange(1, w + 1), k)) % k
    em = np.stack([src, dst]) if one_way else np.stack([np.concatenate([src, dst]), np.concatenate([dst, src])])
    return em.astype(np.int64)


@pytest.fixture()
def pool():
    """a host arena: base graphs (cycles of N nodes, all with bit rows) and one graph per way to leave their class"""
    from gnm.arena import GraphArena
    arena = GraphArena("cpu")
    add = lambda n, em: arena.add_raw(n, em, torch.zeros(n, 3))
    # (the base batch is sparse, 0.5 % of n^2: each variant stays on the gather route, so `dense` never differs)
    ids = {"base": [add(N, _band()) for _ in range(6)], "nobits": add(N, _band()), "n": add(N - 4, _band(N - 4)),
           "asym": add(N, _band(one_way=True)), "iso": add(N, _band(isolated=True)), "nnz": add(N, _band(w=6))}
    # a host arena builds no bit matrices (gnm_adj_bits_build runs on the GPU): give every graph but one bit rows
    arena.bits_ok = [g != ids["nobits"] for g in range(len(arena))]
    arena._dev_tables = None
    return arena, ids


def _variants(ids):
    base = ids["base"]
    same = {"base": base[:4], "same class": base[2:6]}
    other = {"B": base[:3], "n": base[:3] + [ids["n"]], "symmetry": base[:3] + [ids["asym"]],
             "iso": base[:3] + [ids["iso"]], "nnz above the cap": base[:3] + [ids["nnz"]],
             "has_bits": base[:3] + [ids["nobits"]]}
    arr = lambda v: {k: np.array(g, dtype=np.int64) for k, g in v.items()}
    return arr(same), arr(other)


def test_class_of_is_the_class_of_the_batch(pool):
    arena, ids = pool
    same, other = _variants(ids)
    for name, gh in list(same.items()) + list(other.items()):
        b = arena.batch_from_gids(gh)
        assert arena.class_of(gh) == b.batch_class, name
    cls = arena.class_of(same["base"])
    assert (cls.B, cls.N, cls.n_max, cls.n_min, cls.nnz_max) == (4, 4 * N, N, N, 2 * N)
    assert cls.symmetric and cls.has_bits and not cls.iso and not cls.dense
    for name, field in (("has_bits", "has_bits"), ("iso", "iso"), ("symmetry", "symmetric")):
        assert getattr(arena.class_of(other[name]), field) != getattr(cls, field), name


def test_every_user_refuses_a_batch_of_another_class(pool):
    from gnm.arena import BatchClassMismatch, PackedStaticBatch, StaticBatch
    arena, ids = pool
    same, other = _variants(ids)
    template = arena.batch_from_gids(same["base"])
    static = StaticBatch(template)
    packed = PackedStaticBatch(arena, arena.class_of(same["base"]))
    assert packed.batch_class.nnz_max == 4096                 # the launch parameters' edge bound, rounded up
    for name, gh in same.items():
        b = arena.batch_from_gids(gh)
        assert template.batch_class.admits(b.batch_class), name
        assert packed.fits(gh), name
        static.load(b)
        assert torch.equal(static.batch.gids, b.gids)
    for name, gh in other.items():
        b = arena.batch_from_gids(gh)
        assert not template.batch_class.admits(b.batch_class), name
        assert not packed.fits(gh), name
        with pytest.raises(BatchClassMismatch):
            static.load(b)


def test_load_gids_checks_extra(pool):
    from gnm.arena import PackedStaticBatch
    arena, ids = pool
    gh = np.array(ids["base"][:4], dtype=np.int64)
    cls = arena.class_of(gh)
    with_extra = PackedStaticBatch(arena, cls, extra_words=3)
    with pytest.raises(ValueError, match="extra"):
        with_extra.load_gids(gh)                              # would upload whatever the staging slot held before
    with pytest.raises(ValueError, match="3 values"):
        with_extra.load_gids(gh, np.arange(2, dtype=np.int64))
    with_extra.load_gids(gh, np.array([7, 8, 9], dtype=np.int64))
    assert with_extra.extra.tolist() == [7, 8, 9]
    assert torch.equal(with_extra.batch.gids, torch.as_tensor(gh))
    with pytest.raises(ValueError, match="extra"):
        PackedStaticBatch(arena, cls).load_gids(gh, np.arange(3, dtype=np.int64))


def test_captured_step_refuses_a_template_of_another_class_than_its_ids(pool):
    from gnm.graphs import CapturedTrainStep
    arena, ids = pool
    same, other = _variants(ids)
    template = arena.batch_from_gids(same["base"])
    for name in ("has_bits", "nnz above the cap", "iso"):
        # (checked before the model, the loss or the GPU are touched)
        with pytest.raises(ValueError, match="class"):
            CapturedTrainStep(None, template, None, gids_host=other[name])
