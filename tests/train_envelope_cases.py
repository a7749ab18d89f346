"""The case table of the training-step envelope (tests/test_gpu_train_envelope.py on the GPU, tests/test_train_envelope_host.py
without one), with the graph and parameter builders and the references both halves share.

A case is one training step: GIN_InfoMaxReg(...).train(), forward_batch(batch, perm), CE + 0.05 BCE, backward().  Its id
names the route it is there to reach and its fields DECLARE that route:

  agg0        layer 0's aggregation when it runs in the step (the layer-0 cache off, or max pooling), else None
  fwd / bwd   the aggregation of every layer >= 1, forward (the BatchNorm + ReLU + readout prologue form) and backward
              (the BatchNorm-backward epilogue form); codes below
  lin         the Linear backward of (layer 0, k = 0), (layer >= 1, k = 0) and (k >= 1); codes below
  head        the status gnm_head_fwd returns
  disc        "unit" (gnm_disc_score_fwd_unit returned 0) or "declined" (-2, then gnm_disc_score_fwd)

Aggregation codes (M: the matrix-core entry of the form, C: its CSR entry, lower case: the plain form):
  "M"       matrix-core fused form returned 0          "C"      CSR fused form returned 0 (the batch is not dense)
  "M>C"     matrix-core fused -2, CSR fused 0          "C>c"    CSR fused -2, then the unfused pair on gnm_agg
  "M>C>m"   both fused forms -2, unfused on gnm_aggm   "M>C>m>c" ... and gnm_aggm -2 as well (F < 32 with d-eps partials)
  "m" / "c" the plain form alone                       "max-t" / "max-u": the tiled / untiled neighbour-max kernel
Linear backward codes:
  "rz"             gnm_linear_bwd_fused_rz returned 0
  "fused"          gnm_linear_bwd_fused (stored Z) returned 0, no lower BatchNorm
  "fused+sums"     gnm_linear_bwd_fused returned 0 with the lower BatchNorm's sums
  "generic"        gnm_linear_bwd_fused -2, gnm_linear_wgrad, dX (when wanted) by k-major gnm_linear_fwd windows
  "generic+masked" ... dX by gnm_linear_dgrad_masked

expected_route() expands the codes into the per-layer and per-Linear sequences of "entry:status" the GPU test compares
the spies' log with; the host test runs core.agg_launch / core.linear_bwd_launch on spies programmed with the declared
statuses and checks the host-side predicates (core._dense on the case's fill, gnm_agg_slice_width, the fused entries'
width rules), so the table cannot drift from the routing code unnoticed.

Parameters are never trivial (drawn BatchNorm affines and running statistics, drawn eps, labels, a perm that is not the
identity) and every Linear is rescaled on the case's own data in fp64 so that activations stay O(1).  A small case
(L <= 5, n <= 64) whose smallest |pre-activation| under a ReLU is below RELU_MARGIN x the layer's largest is redrawn
with the next parameter seed (case_data, `draw`): no small case sits on a mask boundary.

The last section builds, per case, a pool of graphs of the case's class and a sequence of five batches drawn from it
(case_pool), the table of what keeps a case out of a replay kind (replay_exclusion), and the fp64 anchor of a replayed
step (anchor): what tests/test_gpu_replay_envelope.py and tests/test_replay_envelope_host.py share."""
import collections
import functools
import itertools
import zlib

import numpy as np
import torch

from test_gpu_eval_envelope import EG, _lin_names, make_graph

RELU_MARGIN = 1e-5
BETA = 0.05

_FIELDS = dict(L=2, m=2, F0=7, H=64, C=2, B=2, n=33, kind="sym", dens=None, feats="mixed", gpool="sum", npool="sum",
               eps=True, p0=True, keep=False, sink=False, loss="torch", drop=0.0, data=None,
               agg0=None, fwd="M", bwd="M", lin=("rz", "rz", "fused+sums"), head=0, disc="unit", pair=None)
Case = collections.namedtuple("Case", ["id"] + list(_FIELDS))


def _c(id, **kw):
    bad = set(kw) - set(_FIELDS)
    assert not bad, bad
    return Case(id=id, **{**_FIELDS, **kw})


G3 = ("generic", "generic", "generic")
SPARSE = dict(kind="sparse", dens=0.03, n=70)            # fill 0.03 < DENSE_MIN_FILL: the CSR gather
DROP = dict(drop=0.4)

CASES = [
    # ---- Linear backward: Z recomputed (rz) and stored-Z fused
    _c("lin-rz-wide-H64-m2", L=3),
    _c("lin-rz-narrow-F1", F0=1, **DROP),
    _c("lin-rz-narrow-F7-eps0", eps=False),              # no dX wanted from the input layer's Linear
    _c("lin-rz-narrow-F16", F0=16, npool="average"),
    _c("lin-fused-narrow-F17", F0=17, lin=("fused", "rz", "fused+sums")),
    _c("lin-fused-narrow-F31", F0=31, lin=("fused", "rz", "fused+sums"), gpool="average", **DROP),
    _c("lin-fused-F32-H64", F0=32, lin=("fused", "rz", "fused+sums")),
    _c("lin-fused-F32-H32", F0=32, H=32, fwd="M>C", bwd="M>C", lin=("fused", "fused", "fused+sums")),
    _c("lin-rz-F64-H64", F0=64, lin=("rz", "rz", "fused+sums")),          # the input as wide as the hidden layers
    _c("lin-fused-F64-H64-eps0", F0=64, eps=False, lin=("fused", "rz", "fused+sums")),   # ... without dX: rz declines
    _c("lin-sums-m2-H32", H=32, fwd="M>C", bwd="M>C", lin=("fused", "fused", "fused+sums"), npool="average"),
    _c("lin-sums-m3-H32", H=32, m=3, fwd="M>C", bwd="M>C", lin=("fused", "fused", "fused+sums"), **DROP),
    _c("lin-sums-m2-H64", gpool="average", npool="average"),
    _c("lin-sums-m3-H64", m=3, L=3, eps=False),
    _c("lin-m1-H64", m=1, L=3, lin=("rz", "rz", None)),
    # ---- Linear backward: the generic three-kernel route
    _c("lin-generic-masked-H128-m2", H=128, fwd="M>C>m", bwd="M>C>m", lin=("generic", "generic", "generic+masked")),
    _c("lin-generic-masked-H128-m3", H=128, m=3, fwd="M>C>m", bwd="M>C>m",
       lin=("generic", "generic", "generic+masked"), npool="average", **DROP),
    _c("lin-generic-wide-H48", H=48, fwd="C>c", bwd="C>c", lin=G3, disc="declined"),
    _c("lin-generic-wide-H96", H=96, fwd="M>C>m", bwd="M>C>m", lin=G3, disc="declined", gpool="average"),
    _c("lin-generic-wide-H20", H=20, fwd="M>C>m", bwd="M>C>m>c", lin=G3, disc="declined"),
    _c("lin-generic-wide-H128-F40", H=128, F0=40, fwd="M>C>m", bwd="M>C>m", lin=("generic", "generic", "generic+masked")),
    _c("lin-onehot-F400-n400-H32", F0=400, n=400, B=2, H=32, feats="onehot", fwd="M>C", bwd="M>C",
       lin=("generic", "fused", "fused+sums")),
    # (hidden_dim 128 bounds input_dim to gnm_linear_max_k(128) = 192, which the constructor enforces: the widest
    # one-hot first layer there is 192 columns, two dX windows)
    _c("lin-onehot-F192-n400-H128", F0=192, n=400, B=2, H=128, feats="onehot", fwd="M>C>m", bwd="M>C>m",
       lin=("generic", "generic", "generic+masked"), npool="average", gpool="average"),
    _c("lin-onehot-F200-n200-H64", F0=200, n=200, B=2, feats="onehot", lin=("generic", "rz", "fused+sums")),
    # ---- aggregation on the matrix cores (density 0.3): plain (layer 0, the cache off), prologue, epilogue
    _c("agg-mfma-H64", p0=False, agg0="m", L=3, npool="average"),
    _c("agg-mfma-H32", p0=False, agg0="m", H=32, L=3, fwd="M>C", bwd="M>C", lin=("fused", "fused", "fused+sums")),
    _c("agg-mfma-H128", p0=False, agg0="m", H=128, fwd="M>C>m", bwd="M>C>m", lin=("generic", "generic", "generic+masked")),
    _c("agg-mfma-H48-unfused", p0=False, agg0="m", H=48, fwd="C>c", bwd="C>c", lin=G3, disc="declined"),
    _c("agg-mfma-F20-partial-block", p0=False, agg0="m", F0=20, lin=("fused", "rz", "fused+sums"), eps=False,
       npool="average"),
    _c("agg-mfma-F40-layer0-gather", p0=False, agg0="c", F0=40, lin=("generic", "rz", "fused+sums")),
    # ---- aggregation on the CSR gather (fill 0.03)
    _c("agg-csr-H64", p0=False, agg0="c", L=3, fwd="C", bwd="C", **SPARSE),
    _c("agg-csr-H32", p0=False, agg0="c", H=32, L=3, fwd="C", bwd="C", lin=("fused", "fused", "fused+sums"),
       gpool="average", **SPARSE),
    _c("agg-csr-H128", p0=False, agg0="c", H=128, fwd="C>c", bwd="C>c", lin=("generic", "generic", "generic+masked"),
       **SPARSE),
    _c("agg-csr-H48-unfused", p0=False, agg0="c", H=48, fwd="C>c", bwd="C>c", lin=G3, disc="declined", eps=False,
       **SPARSE),
    _c("agg-csr-H64-avg-eps0", fwd="C", bwd="C", npool="average", eps=False, **SPARSE),
    # ---- isolated nodes in a dense batch
    _c("agg-iso-avg-eps1-gather-nan", kind="iso", npool="average", p0=False, agg0="c", fwd="C", bwd="C"),
    _c("agg-iso-avg-eps0-mfma", kind="iso", npool="average", eps=False, p0=False, agg0="m"),
    _c("agg-iso-sum-eps1-mfma", kind="iso", p0=False, agg0="m"),
    _c("agg-iso-sum-eps0-mfma", kind="iso", eps=False, gpool="average"),
    # ---- directed graphs (the transposed CSR / bits in the backward), a repeated edge
    _c("agg-dir-mfma-H64", kind="dir", L=3, npool="average"),
    _c("agg-dir-mfma-H128-unfused", kind="dir", H=128, fwd="M>C>m", bwd="M>C>m",
       lin=("generic", "generic", "generic+masked")),
    _c("agg-dir-csr-H64", kind="sparse-dir", dens=0.03, n=70, L=3, fwd="C", bwd="C"),
    _c("agg-dir-csr-H32-avg", kind="sparse-dir", dens=0.03, n=70, H=32, fwd="C", bwd="C", npool="average", eps=False,
       lin=("fused", "fused", "fused+sums")),
    _c("agg-multi-edge-gather", kind="multi", p0=False, agg0="c", fwd="C", bwd="C"),
    # ---- row blocks of 32, the second bit-row vector, beyond the bit adjacency
    _c("agg-mfma-n31", n=31), _c("agg-mfma-n32", n=32, npool="average"), _c("agg-mfma-n33-eps0", n=33, eps=False),
    _c("agg-mfma-n63", n=63, gpool="average"), _c("agg-mfma-n65", n=65, npool="average", eps=False),
    _c("agg-mfma-n257-B2", n=257, B=2, p0=False, agg0="m"),
    _c("agg-csr-n417-B2-deg12", n=417, B=2, kind="deg", dens=12, p0=False, agg0="c", fwd="C", bwd="C"),
    _c("agg-csr-n417-B2-deg12-H128", n=417, B=2, kind="deg", dens=12, H=128, fwd="C>c", bwd="C>c",
       lin=("generic", "generic", "generic+masked"), npool="average", eps=False),
] + [
    # ---- pooling and eps: all eight at H = 64
    _c("pool-H64-n%s-g%s-eps%d" % (np_, gp, e), npool=np_, gpool=gp, eps=bool(e), L=3, **DROP)
    for np_ in ("sum", "average") for gp in ("sum", "average") for e in (1, 0)
] + [
    # ... and the four corners at H = 32
    _c("pool-H32-n%s-g%s-eps%d" % (np_, gp, e), H=32, npool=np_, gpool=gp, eps=bool(e), L=3, fwd="M>C", bwd="M>C",
       lin=("fused", "fused", "fused+sums"))
    for np_, gp, e in (("sum", "sum", 1), ("sum", "average", 0), ("average", "sum", 0), ("average", "average", 1))
] + [
    # ---- neighbour max: no fused aggregation form is tried
    _c("max-H64-eps1-gsum-padded", npool="max", agg0="max-u", fwd="max-t", bwd="max-t", L=3, **DROP),
    _c("max-H64-eps0-gavg-padded", npool="max", eps=False, gpool="average", agg0="max-u", fwd="max-t", bwd="max-t"),
    _c("max-H32-eps1-gavg-padded", npool="max", H=32, gpool="average", agg0="max-u", fwd="max-t", bwd="max-t",
       lin=("fused", "fused", "fused+sums")),
    _c("max-H32-eps0-gsum-padded", npool="max", H=32, eps=False, agg0="max-u", fwd="max-t", bwd="max-t",
       lin=("fused", "fused", "fused+sums"), **DROP),
    _c("max-H64-eps1-regular-no-dummy", npool="max", kind="regular", agg0="max-u", fwd="max-t", bwd="max-t"),
    _c("max-H64-eps0-regular-no-dummy", npool="max", kind="regular", eps=False, agg0="max-u", fwd="max-t", bwd="max-t"),
    _c("max-F32-layer0-tiled", npool="max", F0=32, agg0="max-t", fwd="max-t", bwd="max-t",
       lin=("fused", "rz", "fused+sums")),
    # n = 417 still fits the tiled kernels' LDS tile at H = 64 (6 F (n + 1) + 4 (n + 1) bytes in the backward: up to
    # n = 421); n = 640 is beyond both the forward's and the backward's
    _c("max-H64-n417-tiled", npool="max", n=417, B=2, kind="deg", dens=12, agg0="max-u", fwd="max-t", bwd="max-t"),
    _c("max-H64-n640-untiled", npool="max", n=640, B=1, kind="deg", dens=12, agg0="max-u", fwd="max-u", bwd="max-u"),
    # ---- the layer-0 cache, keep_hidden, the gradient sink
    _c("p0-on-eps1", data="p0-eps1", npool="average", pair="p0-off-eps1"),
    _c("p0-off-eps1", data="p0-eps1", npool="average", p0=False, agg0="m"),
    _c("p0-on-eps0", data="p0-eps0", eps=False, pair="p0-off-eps0", **DROP),
    _c("p0-off-eps0", data="p0-eps0", eps=False, p0=False, agg0="m", **DROP),
    _c("keep-hidden-on", data="keep", L=3, keep=True, pair="keep-hidden-off"),
    _c("keep-hidden-off", data="keep", L=3),
    _c("keep-hidden-on-H128-unfused", H=128, keep=True, fwd="M>C>m", bwd="M>C>m",
       lin=("generic", "generic", "generic+masked")),
    _c("keep-hidden-on-max", npool="max", keep=True, agg0="max-u", fwd="max-t", bwd="max-t"),
    _c("grad-sink-H64", sink=True, L=3, **DROP),
    _c("grad-sink-H128-eps0", sink=True, H=128, eps=False, fwd="M>C>m", bwd="M>C>m",
       lin=("generic", "generic", "generic+masked")),
    # ---- the classifier head
    _c("head-C2-drop", **DROP), _c("head-C3-p0", C=3, L=3), _c("head-C3-drop", C=3, L=3, **DROP),
    _c("head-C256", C=256, B=4), _c("head-C256-drop", C=256, B=4, **DROP),
    _c("head-C257-fallback", C=257, B=4, head=-2), _c("head-C257-fallback-drop", C=257, B=4, head=-2, **DROP),
    # ---- the discriminator
    _c("disc-unit-handover-infomax-loss", data="disc", B=5, loss="infomax", **DROP),
    _c("disc-unit-torch-loss-no-handover", data="disc", B=5, pair="disc-unit-handover-infomax-loss", **DROP),
    _c("disc-unit-declines-H20-L3", H=20, L=3, B=2, n=8, loss="infomax", fwd="M>C>m", bwd="M>C>m>c", lin=G3,
       disc="declined"),
    _c("disc-B1", B=1, loss="infomax"),
    _c("disc-B40-n6", B=40, n=6, H=32, m=1, loss="infomax", fwd="M>C", bwd="M>C", lin=("fused", "fused", None), **DROP),
    # ---- depth
    _c("depth-L1-no-deferred-readout", L=1, C=4, lin=("rz", None, "fused+sums")),
    _c("depth-L8-H64-m2", L=8, disc="declined"),
]
BY_ID = {c.id: c for c in CASES}
assert len(BY_ID) == len(CASES)


def small(case):
    """the fuzz test's flat bounds apply: L <= 5 and n <= 64; and, whatever its size, a case with dropout masks or max
    pooling, which the fp32 CPU restatement does not have -- such a case is never calibrated"""
    return (case.L <= 5 and case.n <= 64) or case.drop > 0 or case.npool == "max"


# --------------------------------------------------------------------------- graphs
def _own_graph(rng, n, kind, dens, f0, feats):
    A = np.zeros((n, n), dtype=bool)
    i = np.arange(n)
    if kind == "sparse":                # a ring (no node without neighbours) + random pairs up to the fill `dens`
        A = np.triu(rng.random((n, n)) < max(0.0, dens - 2.0 / n), 1)
        A[i, (i + 1) % n] = True
        A = A | A.T
    elif kind == "sparse-dir":          # a directed ring + random arcs
        A = rng.random((n, n)) < max(0.0, dens - 1.0 / n)
        A[i, (i + 1) % n] = True
    elif kind == "deg":                 # undirected, about `dens` neighbours per node
        A = np.triu(rng.random((n, n)) < dens / n, 1)
        A = A | A.T
    elif kind == "regular":             # circulant: every node has exactly six neighbours
        for d in (1, 2, 5):
            A[i, (i + d) % n] = True
        A = A | A.T
    else:
        raise ValueError(kind)
    np.fill_diagonal(A, False)
    src, dst = np.nonzero(A)
    if feats == "onehot":
        X = np.eye(f0, dtype=np.float32)[rng.integers(0, f0, n)]
    else:
        X = rng.standard_normal((n, f0)) * 10.0 ** rng.uniform(-1.5, 1.5, f0)
    return EG(n, src, dst, X)


def _case_graph(case, rng, kind):
    """one graph of the case's class from `rng`: the per-kind generator, then the label and graph.neighbors"""
    if case.dens is None and case.kind in ("sym", "dir", "iso", "multi"):
        g = make_graph(rng, case.n, kind, case.F0, case.feats)
    else:
        g = _own_graph(rng, case.n, case.kind, case.dens, case.F0, case.feats)
    g.label = int(rng.integers(0, case.C))
    _set_neighbors(g)
    return g


def _set_neighbors(g):
    em = g.edge_mat.numpy()
    # graph.neighbors as util.py:86-90 leaves them, read by neighbour "max" only
    nb = [[] for _ in range(g.num_nodes)]
    for a, b in zip(em[0].tolist(), em[1].tolist()):
        nb[a].append(b)
    g.neighbors = nb
    g.max_neighbor = max((len(x) for x in nb), default=0)


def case_graphs(case):
    rng = np.random.default_rng(zlib.crc32((case.data or case.id).encode()))
    # (isolated nodes in the first graph only, as the eval envelope has them)
    gs = [_case_graph(case, rng, case.kind if case.kind != "iso" or j == 0 else "sym") for j in range(case.B)]
    return gs, rng


def oracle_batch(graphs):
    from oracle import gin_oracle as O
    return [O.OGraph(g.num_nodes, g.edge_mat.numpy(), g.node_features.numpy(), g.label, neighbors=g.neighbors,
                     max_neighbor=g.max_neighbor) for g in graphs]


def expected_dense(case, graphs):
    """what GraphArena.class_of decides for this batch on a GPU arena: every graph has a bit adjacency (at most
    gnm_aggm_max_nodes nodes, no repeated edge) and the batch's fill reaches DENSE_MIN_FILL"""
    from gnm._cabi import lib
    from gnm.arena import DENSE_MIN_FILL
    nnz = 0
    for g in graphs:
        em = g.edge_mat.numpy()
        if g.num_nodes > int(lib.gnm_aggm_max_nodes()) or len(set(zip(em[0].tolist(), em[1].tolist()))) != em.shape[1]:
            return False
        nnz += em.shape[1]
    return nnz >= DENSE_MIN_FILL * sum(float(g.num_nodes) ** 2 for g in graphs)


def has_isolated(graphs):
    """GraphArena's `iso`: a node with an empty CSR row (no edge_mat column starts at it)"""
    return any(len(set(g.edge_mat.numpy()[0].tolist())) < g.num_nodes for g in graphs)


# --------------------------------------------------------------------------- parameters
def _draw_state(case, graphs, seed):
    """(state dict of float32 arrays, smallest relative ReLU margin of the fp64 train-mode forward)"""
    from models.graphcnn import GIN_InfoMaxReg
    from oracle import gin_oracle as O
    L, m = case.L, case.m
    torch.manual_seed(seed)
    model = GIN_InfoMaxReg(L, m, case.F0, case.H, case.C, case.drop, case.eps, case.gpool, case.npool,
                           torch.device("cpu"))
    g = np.random.default_rng(seed + 1000)
    sd = model.state_dict()
    with torch.no_grad():
        for k, t in sd.items():
            if k.endswith("running_mean"):
                t.copy_(torch.from_numpy(g.normal(0, 0.3, t.shape)))
            elif k.endswith("running_var"):
                t.copy_(torch.from_numpy(g.uniform(0.2, 3.0, t.shape)))
            elif "batch_norms" in k and k.endswith("weight"):
                t.copy_(torch.from_numpy(g.uniform(0.5, 1.5, t.shape)))
            elif "batch_norms" in k and k.endswith("bias"):
                t.copy_(torch.from_numpy(g.normal(0, 0.2, t.shape)))
        sd["eps"].copy_(torch.from_numpy(g.uniform(-0.4, 0.4, L)))
        p = {k: t.numpy().astype(np.float64) for k, t in sd.items()}
        ob = oracle_batch(graphs)
        h = np.concatenate([gr.node_features.numpy() for gr in graphs]).astype(np.float64)
        if case.npool == "max":
            padded = O.build_padded_neighbors(ob, case.eps)
        else:
            idx, val, shape = O.build_adj_block(ob, case.eps)
            A = O.coo_to_csr(idx, val, shape, np.float64)
            deg = np.asarray(A.sum(1)).reshape(-1, 1)
        margin, hidden = np.inf, []
        with np.errstate(all="ignore"):
            for l in range(L):
                if case.npool == "max":
                    x = O.maxpool_fwd(h, padded)[0]
                else:
                    x = A @ h
                    if case.npool == "average":
                        x = x / deg
                if case.eps:
                    x = x + (1 + p["eps"][l]) * h
                for k in range(m):
                    wn, bn = _lin_names(l, k, m)
                    z = x @ p[wn + ".weight"].T + p[wn + ".bias"]
                    s = float(np.sqrt(np.mean(z * z)))
                    s = s if np.isfinite(s) and s > 0 else 1.0        # (the 0/0 rows of isolated nodes: all NaN)
                    sd[wn + ".weight"].div_(s)
                    sd[wn + ".bias"].div_(s)
                    p[wn + ".weight"] = sd[wn + ".weight"].numpy().astype(np.float64)
                    p[wn + ".bias"] = sd[wn + ".bias"].numpy().astype(np.float64)
                    z = x @ p[wn + ".weight"].T + p[wn + ".bias"]
                    y = (z - z.mean(0)) / np.sqrt(z.var(0) + 1e-5) * p[bn + ".weight"] + p[bn + ".bias"]
                    if np.isfinite(y).all():
                        margin = min(margin, float(np.abs(y).min() / np.abs(y).max()))
                    x = np.maximum(y, 0)
                h = x
                hidden.append(h)
            # the classifier and the discriminator likewise: logits of O(1).  (A saturated softmax or sigmoid makes
            # the loss gradient p - y a difference of nearly equal fp32 numbers: with logits of 20 the reference's own
            # fp32 gradients sit 2e-4 from fp64.)
            gi, gv, gs = O.build_graph_pool(ob, case.gpool)
            Pm = O.coo_to_csr(gi, gv, gs, np.float64)
            lat = [Pm @ hl for hl in hidden]
            wp = ["linears_prediction.%d" % l for l in range(L)]
            c_logit = sum(lat[l] @ p[wp[l] + ".weight"].T + p[wp[l] + ".bias"] for l in range(L))
            s = float(np.sqrt(np.mean(c_logit * c_logit)))
            if np.isfinite(s) and s > 0:
                for l in range(L):
                    sd[wp[l] + ".weight"].div_(s)
                    sd[wp[l] + ".bias"].div_(s)
            c_x = np.repeat(O.sigmoid(np.concatenate(lat, 1)), case.n, axis=0)
            sc = ((np.concatenate(hidden, 1) @ p["disc.f_k.weight"][0]) * c_x).sum(1) + p["disc.f_k.bias"][0]
            s = float(np.sqrt(np.mean(sc * sc)))
            if np.isfinite(s) and s > 0:
                sd["disc.f_k.weight"].div_(s)
                sd["disc.f_k.bias"].div_(s)
    return {k: v.detach().numpy().copy() for k, v in model.state_dict().items()}, margin


Data = collections.namedtuple("Data", "graphs state perm masks draw")


@functools.lru_cache(maxsize=None)
def _data(key):
    case = next(c for c in CASES if (c.data or c.id) == key)
    graphs, rng = case_graphs(case)
    perm = rng.permutation(case.B)
    while case.B > 1 and np.array_equal(perm, np.arange(case.B)):
        perm = rng.permutation(case.B)
    masks = None
    if case.drop > 0:
        masks = ((rng.random((case.L, case.B, case.C)) >= case.drop) / (1 - case.drop)).astype(np.float32)
    base = zlib.crc32(key.encode()) % 100000
    for draw in range(3000):
        state, margin = _draw_state(case, graphs, base + 7919 * draw)
        # (a small case: redrawn until no pre-activation sits on a ReLU mask boundary, with room for the rounding of
        # the parameters to fp32 between this forward and the oracle's)
        if not (case.L <= 5 and case.n <= 64) or margin >= 1.5 * RELU_MARGIN:
            return Data(graphs, state, perm, masks, draw)
    raise AssertionError("%s: no parameter draw keeps the ReLU margin" % key)


def case_data(case):
    return _data(case.data or case.id)


@functools.lru_cache(maxsize=None)
def _reference(key):
    """(fp64 oracle's train_step_grads, the fp32 CPU restatement's train_step or None, its BatchNorm buffers or None)
    of the case's step: computed once, shared, and never modified"""
    from oracle import gin_oracle as O
    from oracle.gin_torch_cpu import TorchCpuGIN
    case = next(c for c in CASES if (c.data or c.id) == key)
    d = _data(key)
    ob = oracle_batch(d.graphs)
    om = O.OracleGIN(d.state, case.L, case.m, case.eps, case.gpool, case.npool, dtype=np.float64)
    with np.errstate(all="ignore"):
        ref = om.train_step_grads(ob, d.perm, beta=BETA,
                                  dropout_masks=None if d.masks is None else [d.masks[l].astype(np.float64)
                                                                              for l in range(case.L)])
    ref["buffers"] = {k: v for k, v in om.p.items() if k.endswith(("running_mean", "running_var"))}
    r32 = None
    if case.npool != "max" and case.drop == 0:
        t32 = TorchCpuGIN(d.state, case.L, case.m, case.eps, case.gpool, case.npool)
        r32 = t32.train_step(ob, d.perm, beta=BETA)
        r32["buffers"] = {k: v.numpy() for k, v in t32.buf.items() if not k.endswith("num_batches_tracked")}
    return ref, r32


def reference(case):
    return _reference(case.data or case.id)


# --------------------------------------------------------------------------- the declared route, expanded
_AGG_CODES = {
    "M": ["{M}:0"], "C": ["{C}:0"], "M>C": ["{M}:-2", "{C}:0"],
    "C>c": ["{C}:-2", "{R}", "gnm_agg:0"],
    "M>C>m": ["{M}:-2", "{C}:-2", "{R}", "gnm_aggm:0"],
    "M>C>m>c": ["{M}:-2", "{C}:-2", "{R}", "gnm_aggm:-2", "gnm_agg:0"],
    "m": ["gnm_aggm:0"], "c": ["gnm_agg:0"],
    "max-t": ["{R}", "gnm_maxpool_{D}_tiled:0"], "max-u": ["{R}", "gnm_maxpool_{D}_tiled:-2", "gnm_maxpool_{D}:0"],
}
READOUT = "gnm_bn_relu_readout:0"


def agg_events(code, backward, layer0=False):
    """the "entry:status" sequence of one layer's aggregation; {R}: the unfused BatchNorm + ReLU + readout of the layer
    below, a kernel of its own in the forward of a layer >= 1 only"""
    form = "bwd_stats" if backward else "fwd_bnrelu"
    out = []
    for e in _AGG_CODES[code]:
        if e == "{R}":
            if not backward and not layer0:
                out.append(READOUT)
            continue
        out.append(e.format(M="gnm_aggm_" + form, C="gnm_agg_" + form, D="bwd" if backward else "fwd"))
    return out


def lin_shape(case, l, k):
    """(K, H, has a prologue, a Linear below it in the MLP, dX wanted) of Linear (l, k) as linear_bwd_launch sees it"""
    K = case.F0 if (l == 0 and k == 0) else case.H
    return K, case.H, k > 0, k > 0, (k > 0 or l > 0 or case.eps)


def lin_code(case, l, k):
    return case.lin[2] if k > 0 else case.lin[0 if l == 0 else 1]


def lin_events(code, K, H, below, need_dA):
    rz_asked = H == 64 and not (below and need_dA) and ((K == 64 and need_dA) or (K <= 16 and not below))
    if code == "rz":
        return ["gnm_linear_bwd_fused_rz:0"]
    pre = ["gnm_linear_bwd_fused_rz:-2"] if rz_asked else []
    if code == "fused":
        return pre + ["gnm_linear_bwd_fused:0"]
    if code == "fused+sums":
        return pre + ["gnm_linear_bwd_fused[sums]:0"]
    out = pre + ["gnm_linear_bwd_fused%s:-2" % ("[sums]" if below and need_dA else ""), "gnm_linear_wgrad:0"]
    if code == "generic+masked":
        return out + ["gnm_linear_dgrad_masked:0"]
    assert code == "generic", code
    if need_dA:
        out += ["gnm_linear_fwd[dgrad]:0"] * ((K + 127) // 128)
    return out


def expected_route(case):
    """{"fwd": one sequence per layer + the top layer's readout, "lin": {(l, k): sequence}, "bwd": {l: sequence},
    "head": [...], "disc": [...]}"""
    L, m = case.L, case.m
    fwd = [agg_events(case.agg0, False, layer0=True) if case.agg0 else []]
    fwd += [agg_events(case.fwd, False) for _ in range(1, L)]
    fwd.append([READOUT])
    lin = {(l, k): lin_events(lin_code(case, l, k), *[lin_shape(case, l, k)[i] for i in (0, 1, 3, 4)])
           for l in range(L) for k in range(m)}
    bwd = {l: agg_events(case.bwd, True) for l in range(1, L)}
    disc = ["gnm_disc_score_fwd_unit:0"] if case.disc == "unit" else ["gnm_disc_score_fwd_unit:-2",
                                                                       "gnm_disc_score_fwd:0"]
    # the hand-over is used by the loss that recognises it; any other loss, and a declined unit, re-reads the layers
    disc.append("gnm_disc_unit_scale:0" if case.disc == "unit" and case.loss == "infomax" else "gnm_disc_score_bwd:0")
    return dict(fwd=fwd, lin=lin, bwd=bwd, head=["gnm_head_fwd:%d" % case.head], disc=disc)


# --------------------------------------------------------------------------- pools and selection sequences (replays)
# tests/test_gpu_replay_envelope.py replays every case's step from captured hipGraphs on a SEQUENCE of batches and
# compares each replay with the eager step byte for byte; tests/test_replay_envelope_host.py checks the pools.
REPLAY_KINDS = ("step", "fused", "train", "eval")
# the product condition that keeps a case out of a replay kind; None: the case replays.  The one table both halves read.
#   step   gnm.graphs.CapturedTrainStep, both buffer forms       fused  gnm.train.FusedTrainStep(capture=True)
#   train  model(batch) in train mode (gnm.graphs.CapturedTrain)  eval   model(batch) in eval mode (CapturedEval)


def replay_exclusion(case, kind):
    assert kind in REPLAY_KINDS, kind
    if case.npool == "max":
        # models/graphcnn.py forward(): `not self._spec.n_max` guards both replays; a StaticBatch carries no neighbour
        # lists (Batch.maxnb); gnm/train.py FusedTrainStep: "needs the sum/average neighbour-pooling model"
        return "max neighbour pooling never replays (graphcnn.py forward: not _spec.n_max; FusedTrainStep raises)"
    if kind == "train" and case.keep:
        return "keep_hidden: _forward_train_replay declines (graphcnn.py: sp.keep_hidden)"
    if kind == "train" and case.sink:
        return "a gradient sink is installed: _forward_train_replay declines (graphcnn.py: sp.grad_sink is not None)"
    if kind == "train" and case.B > 128:
        return "B > TRAIN_REPLAY_MAX_B"
    if kind == "eval" and case.B > 64:
        return "B > EVAL_REPLAY_MAX_B"
    return None


def pool_size(case):
    """max(6, 3 B); six graphs where they are large (n >= 400)"""
    return 6 if case.n >= 400 else max(6, 3 * case.B)


Pool = collections.namedtuple("Pool", "graphs heavy selections labels perms template redraw")


def _nnz(g):
    return int(g.edge_mat.shape[1])


def _heavier(case, rng, floor):
    """a graph of the case's class with more than `floor` edges: one more of the case's generator, then single edges
    (both directions of a pair for the undirected kinds) added where there is none"""
    g = _case_graph(case, rng, case.kind)
    n = case.n
    A = np.zeros((n, n), dtype=bool)
    em = g.edge_mat.numpy()
    A[em[0], em[1]] = True
    directed = case.kind in ("dir", "sparse-dir")
    while int(A.sum()) <= floor:
        a, b = (int(x) for x in rng.integers(0, n, 2))
        if a == b or A[a, b]:
            continue
        A[a, b] = True
        if not directed:
            A[b, a] = True
    src, dst = np.nonzero(A)
    g.edge_mat = torch.from_numpy(np.ascontiguousarray(np.stack([src, dst]).astype(np.int64)))
    _set_neighbors(g)
    return g


def _build_pool(key, id_, redraw):
    case = BY_ID[id_]
    B, count = case.B, pool_size(case)
    graphs = list(_data(key).graphs)                 # the first B ARE the case's own graphs
    _, rng = case_graphs(case)                       # ... and the rest continue the stream that drew them
    for _ in range(redraw * (count - B)):            # (an anchor case's earlier draws, see _pool)
        _case_graph(case, rng, case.kind)
    for j in range(B, count):
        # (kind "iso": every third pool graph has isolated nodes, so that selections of the template's class can carry
        # one at different batch positions)
        graphs.append(_case_graph(case, rng, case.kind if case.kind != "iso" or j % 3 == 0 else "sym"))
    heavy = None
    if case.kind not in ("iso", "multi"):
        heavy = _heavier(case, rng, max(_nnz(g) for g in graphs))
    if B == 1:
        sel = [[0], [1], [2], [0], [5]]
    elif case.kind == "iso":                         # (B = 2; the graphs with isolated nodes: 0 and 3)
        sel = [[0, 1], [2, 3], [0, 0], [0, 1], [3, 1]]
    else:
        r = min(range(B), key=lambda j: _nnz(graphs[j]))      # (the lighter one twice: nnz_max moves as well)
        sel = [list(range(B)), list(range(B, 2 * B)), [r, r] + list(range(2 * B, 3 * B - 2)), list(range(B)),
               list(range(3 * B - 1, 2 * B - 1, -1))]
    if case.kind != "regular" and B > 1:
        # at least two of the selections 1, 2, 4 differ from the case's own batch in total edge count AND in nnz_max
        # (the launch-sizing argument a capture freezes).  Two graphs drawn with the same edge count can spoil that: the
        # first other choice of graphs outside the own batch takes the selection's place, 4 (descending) before 1
        own = ([_nnz(graphs[j]) for j in sel[0]])
        moved = lambda ids: (sum(_nnz(graphs[j]) for j in ids) != sum(own)            # noqa: E731
                             and max(_nnz(graphs[j]) for j in ids) != max(own)
                             and (case.kind != "iso" or 3 in ids))
        for s, order in ((4, range(count - 1, B - 1, -1)), (1, range(B, count))):
            if sum(moved(sel[k]) for k in (1, 2, 4)) >= 2:
                break
            if not moved(sel[s]):
                sel[s] = next((list(c) for c in itertools.combinations(order, B) if moved(c)), sel[s])
    srng = np.random.default_rng(zlib.crc32((id_ + "/selections").encode()))
    labels, perms = [], []
    for _ in sel:
        labels.append(srng.integers(0, case.C, B).astype(np.int64))
        perm = srng.permutation(B)
        while B > 1 and np.array_equal(perm, np.arange(B)):
            perm = srng.permutation(B)
        perms.append(perm.astype(np.int64))
    # the StaticBatch form is captured on the selection with the most edges in one graph: it admits every other one
    template = max(range(len(sel)), key=lambda s: (max(_nnz(graphs[j]) for j in sel[s]), -s))
    return Pool(tuple(graphs), heavy, tuple(tuple(s) for s in sel), tuple(labels), tuple(perms), template, redraw)


@functools.lru_cache(maxsize=None)
def _pool(key, id_):
    """the pool as drawn; for an ANCHOR_CASES case the graphs beyond the case's own are redrawn further down the same
    stream until one of the selections 1, 2, 4 keeps RELU_MARGIN under the case's parameters (which were drawn for the
    case's own batch): the replayed step on it is compared with the fp64 oracle"""
    if id_ not in ANCHOR_CASES:
        return _build_pool(key, id_, 0)
    for redraw in range(200):
        pool = _build_pool(key, id_, redraw)
        if any(selection_oracle(BY_ID[id_], s, pool)[1] >= RELU_MARGIN for s in (1, 2, 4)):
            return pool
    raise AssertionError("%s: no pool draw has a selection that keeps the ReLU margin" % id_)


def case_pool(case):
    """Pool(graphs, heavy, selections, labels, perms, template): pool_size(case) graphs whose first B are
    case_data(case).graphs; `heavy`, one more graph with more edges than any of them (None for kinds "iso" and
    "multi"), arena id len(graphs) once `graphs + [heavy]` were added in order; the selection sequence as tuples of
    pool indices -- 0 the case's own batch, 1 disjoint from it, 2 overlapping it with one graph twice, 3 the case's own
    batch again, 4 in descending order -- each with its own labels and non-identity permutation; and the index of the
    selection a StaticBatch capture takes as its template.  Built once per case and never modified."""
    return _pool(case.data or case.id, case.id)


def selection_oracle(case, s, pool=None):
    """(the fp64 oracle's train_step_grads on selection s with that selection's labels and permutation, the smallest
    relative |pre-activation| under a ReLU)"""
    from oracle import gin_oracle as O
    d, pool = case_data(case), pool or case_pool(case)
    ob = oracle_batch([pool.graphs[j] for j in pool.selections[s]])
    for g, lab in zip(ob, pool.labels[s]):
        g.label = int(lab)
    om = O.OracleGIN(d.state, case.L, case.m, case.eps, case.gpool, case.npool, dtype=np.float64)
    with np.errstate(all="ignore"):
        ref = om.train_step_grads(ob, pool.perms[s], beta=BETA,
                                  dropout_masks=None if d.masks is None else [d.masks[l].astype(np.float64)
                                                                              for l in range(case.L)])
    margin = np.inf
    for l, lc in enumerate(ref["cache"]["layers"]):
        acts = [(lc["bn_out"][0], "batch_norms.%d" % l)]
        acts += [(ent[2], "mlps.%d.batch_norms.%d" % (l, k)) for k, ent in enumerate(lc["mlp"]) if ent[0] == "lin_bn_relu"]
        for (xhat, _, gamma, _), bn in acts:
            y = xhat * gamma + d.state[bn + ".bias"].astype(np.float64)
            margin = min(margin, float(np.abs(y).min() / np.abs(y).max()))
    return ref, margin


ANCHOR_CASES = ("lin-rz-wide-H64-m2", "agg-csr-H64", "agg-dir-csr-H64", "lin-generic-masked-H128-m2", "lin-sums-m2-H32")


@functools.lru_cache(maxsize=None)
def anchor(id_):
    """(s, the fp64 oracle's step on selection s) of an ANCHOR_CASES case: s = 1, the first batch of the sequence that
    is not the template -- or the first later one that keeps RELU_MARGIN, where selection 1 does not"""
    case = BY_ID[id_]
    for s in (1, 2, 4):
        ref, margin = selection_oracle(case, s)
        if margin >= RELU_MARGIN:
            return s, ref
    raise AssertionError("%s: no selection keeps the ReLU margin" % id_)
