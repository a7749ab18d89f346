"""The case table of the row-block attribution kernels between 71 and 416 nodes (csrc/occlusion.hip, csrc/lesion.hip,
csrc/saliency.hip + csrc/intgrad.hip over csrc/gnm_rowblock.h): tests/test_gpu_rowblock_midrange.py on the GPU,
tests/test_rowblock_midrange_host.py without one.  Data and CPU helpers only; nothing here touches the device library
when the module is imported.

Node counts (W = ceil(n / 32) row blocks, ceil(n / 16) steps of rb_bits_product, HPW = words per half row of the bits):

  n     W   steps  what it reaches
  97    4    7     mid-range, one row in its last block
  129   5    9     mid-range, one row in its last block
  190   6   12     H = 64: 6 steps per wave, residue 2 mod 4
  256   8   16     the last HPW = 4 shape, all blocks full
  257   9   17     the first HPW = 8 shape, one row in its last block
  401  13   26     15 dead rows in the last block
  416  13   26     kRbMaxN, no dead row

Per n: H in {32, 64, 128} x m in {1, 2, 3} at L = 3, F0 = 7, the 8 pooling forms cycled so that each meets every n and
every H; one more case at n = 257 with one-hot features (F0 = 257: layer 0's X W0^T with K not a multiple of 16).  Each
case has an undirected and a directed graph (test_gpu_saliency.random_graph), one at edge probability 12 / n and one at
0.5, alternating.  Models are test_gpu_saliency.model_of's: state_of() draws the same parameters on the CPU, and the GPU
test asserts that the two are the same arrays.

The model seeds are chosen for conditioning by the CPU references alone (tests/test_rowblock_midrange_host.py holds the
conditions, IG_RELU_MARGIN below among them): never by a HIP output.  The references of a case are computed once per process, shared, and never modified.
"""
import collections
import functools

import numpy as np
import torch

from test_intgrad_host import METHODS, oracle_ig, quadrature
from test_lesion_host import delete_nodes, expect_nan

NODES = (97, 129, 190, 256, 257, 401, 416)
HS = (32, 64, 128)
MS = (1, 2, 3)
LAYERS = 3
F0 = 7
MAX_N = 416                                         # kRbMaxN
POOLS = [(np_, gp, le) for np_ in ("sum", "average") for gp in ("sum", "average") for le in (True, False)]
ONE_NODE = (0, 15, 16, 31, 32, 63, 64, 255, 256)    # ... and n - 1: the one-node sets checked on explicit copies
# a case's seed is SEED0 + H + m unless the CPU conditions of the host test asked for another one
SEED0 = 300
SEEDS = {
    # the fp32 oracle's integrated gradients sit 6.9e-4 from the fp64 ones on the undirected graph with seed 367
    "n401-H64-m3-sum-average-eps1": 1367,
    # a pre-activation under a ReLU below IG_RELU_MARGIN (see there) with the default seed: margin before -> after
    "n97-H64-m2-average-sum-eps1": 1366,        # 9.7e-08 -> 8.7e-07
    "n190-H64-m2-average-average-eps1": 1366,   # 6.3e-08 -> 1.0e-06
    "n190-H128-m1-sum-sum-eps1": 1429,          # 8.9e-08 -> 1.8e-06
    "n256-H32-m2-average-sum-eps1": 3334,       # 3.7e-08 -> 5.8e-07
    "n256-H128-m3-sum-average-eps0": 1431,      # 1.5e-08 -> 1.4e-06
    "n257-H128-m2-sum-average-eps0": 7430,      # 1.7e-08 -> 5.1e-07
    "n401-H128-m1-sum-average-eps0": 5429,      # 8.7e-08 -> 6.4e-07
    "n401-H128-m3-average-sum-eps0": 7431,      # 2.0e-08 -> 2.6e-07
    "n416-H64-m3-sum-average-eps0": 26367,      # 5.6e-09 -> 1.5e-06
    "n416-H128-m1-average-sum-eps1": 1429,      # 7.1e-08 -> 1.0e-06
}

Case = collections.namedtuple("Case", "id n H m npool gpool eps F0 one_hot C seed dens K method baseline")


def row_blocks(n):
    return (n + 31) // 32


def half_words(n):
    """rb_half_words(W): words per half row of the bit adjacency and of a keep mask"""
    return (((row_blocks(n) + 1) >> 1) + 3) & ~3


def wave_steps(n, H):
    """the step counts of rb_bits_product's waves: steps s = kh + KS u < ceil(n / 16), KS = 4, 2, 1 k ranges"""
    KS = 4 // (H // 32)
    steps = (n + 15) // 16
    return [-(-(steps - kh) // KS) for kh in range(KS) if kh < steps]


def _case(n, H, m, j, ni, one_hot=False, C=2, tag=""):
    npool, gpool, le = POOLS[(j + ni) % 8]
    method = METHODS[(H // 32 // 2 + m) % 3]
    K = max((1, 2, 5)[(m + ni) % 3], 2 if method == "trapezoid" else 1)
    dens = (12.0 / n, 0.5) if j % 2 == 0 else (0.5, 12.0 / n)     # (undirected graph, directed graph)
    cid = "n%d-H%d-m%d-%s-%s-eps%d%s" % (n, H, m, npool, gpool, le, tag)
    return Case(cid, n, H, m, npool, gpool, le, n if one_hot else F0, one_hot, C, SEEDS.get(cid, SEED0 + H + m), dens, K,
                method, (j + ni) % 2 == 1)


@functools.lru_cache(maxsize=None)
def cases(n):
    """the (H, m, pooling form) cases of node count n; the one-hot case of n = 257 last"""
    ni = NODES.index(n)
    out = [_case(n, H, m, 3 * hi + mi, ni) for hi, H in enumerate(HS) for mi, m in enumerate(MS)]
    if n == 257:
        out.append(_case(257, 64, 2, 0, 0, one_hot=True, tag="-onehot"))
    return tuple(out)


# ---- further cases outside the per-n matrix: more than 8 classes, the ragged batch, the chunked call
CLASS_CASES = (_case(129, 64, 2, 3, 0, C=11, tag="-C11"), _case(257, 128, 1, 2, 0, C=11, tag="-C11"))
CLASS_LISTS = ((7, 2, 9, 0, 4, 10, 1, 8, 3, 5), tuple(range(11)))
RAGGED_CASE = _case(416, 64, 2, 6, 0, tag="-ragged")               # average / average / learned eps
RAGGED_NODES = (33, 256, 257, 416, 2)
CHUNK_CASE = _case(257, 64, 2, 6, 0, tag="-chunks")


def spec_of(case):
    return (LAYERS, case.m, case.eps, case.gpool, case.npool)


def graphs_of(case):
    """(the undirected graph, the directed graph) of a case"""
    from test_gpu_saliency import random_graph
    base = 1000 + case.n + 1000 * (case.H // 32) + 10000 * case.m
    return [random_graph(base + 100000 * d, case.n, case.dens[d], case.F0, directed=bool(d), one_hot=case.one_hot)
            for d in range(2)]


def ragged_graphs():
    from test_gpu_saliency import random_graph
    return [random_graph(7000 + i, n, 0.3 if n < 100 else 24.0 / n, F0, directed=(i == 2))
            for i, n in enumerate(RAGGED_NODES)]


def ragged_sets(graphs):
    """1 .. 5 sets per graph, the empty set first; never the whole graph"""
    rng = np.random.default_rng(71)
    sets = []
    for i, g in enumerate(graphs):
        n = len(g.g)
        S = rng.random((i + 1, n)) < 0.4
        S[0] = False
        S[:, 0] &= ~S.all(1)
        sets.append(S)
    return sets


def chunk_graphs():
    from test_gpu_saliency import random_graph
    return [random_graph(7100 + i, 257, (12.0 / 257, 0.5)[i % 2], F0, directed=(i == 3)) for i in range(5)]


def chunk_sets():
    rng = np.random.default_rng(72)
    S = rng.random((6, 257)) < 0.3
    S[0] = False
    S[1] = np.arange(257) >= 255                                    # columns 255 and 256: either side of the word groups
    return S


def cpu_model(L, m, f0, H, learn_eps, gpool, npool, seed=0, C=2):
    """test_gpu_saliency.model_of on the CPU: the same draws in the same order (the model's parameters are created on
    the CPU before they move to the device, and model_of's generator is a CPU generator)"""
    from models.graphcnn import GIN_InfoMaxReg
    torch.manual_seed(seed)
    model = GIN_InfoMaxReg(L, m, f0, H, C, 0.5, learn_eps, gpool, npool, torch.device("cpu"))
    with torch.no_grad():
        g = torch.Generator().manual_seed(seed + 1)
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
    return model


def model_args(case):
    """model_of's arguments for a case"""
    return (LAYERS, case.m, case.F0, case.H, case.eps, case.gpool, case.npool), dict(seed=case.seed, C=case.C)


@functools.lru_cache(maxsize=None)
def _state(case):
    a, kw = model_args(case)
    return {k: v.detach().numpy().astype(np.float64) if v.dtype.is_floating_point else v.numpy()
            for k, v in cpu_model(*a, **kw).state_dict().items()}


def state_of(case):
    """the case's parameters as test_gpu_occlusion.state64 returns them for model_of(*model_args(case))"""
    return _state(case)


# --------------------------------------------------------------------------- the removed sets
def block_of(n, rb):
    return (np.arange(n) >> 5) == rb


def lesion_sets(case, d):
    """the removed sets of graph d of a case, bool [S, n], and their names"""
    n = case.n
    rng = np.random.default_rng(case.seed * 7 + d + n)
    W = row_blocks(n)
    S = [("empty", np.zeros(n, dtype=bool)), ("last-node", np.arange(n) == n - 1), ("block-0", block_of(n, 0)),
         ("last-block", block_of(n, W - 1)), ("block-2", block_of(n, 2))]
    if n > 256:
        S.append(("255-256", np.isin(np.arange(n), (255, 256))))
        S.append(("block-of-256", block_of(n, 8)))                  # its mask bits: words 4 .. 7 of either half
    for name, frac in (("half", 0.5), ("80%", 0.8)):
        D = np.zeros(n, dtype=bool)
        D[rng.choice(n, int(frac * n), replace=False)] = True
        S.append((name, D))
    if d == 0 and case == all_but_one_case(n):
        S.append(("all-but-one", np.arange(n) != int(rng.integers(0, n))))
    return np.stack([s for _, s in S]), [k for k, _ in S]


def all_but_one_case(n):
    """the case of n that carries the all-but-one set: the first with neighbour average and learned eps (the lone node's
    0 / 0 row: a guaranteed NaN)"""
    return next(c for c in cases(n) if c.npool == "average" and c.eps and not c.one_hot)


def one_node_sets(n):
    return [v for v in ONE_NODE if v < n - 1] + [n - 1]


def ig_declined(case, graph):
    """the condition integrated_gradients() declines on these graphs (attribution.saliency_decline): neighbour average with
    learned eps and a node without neighbours -- an empty row of edge_mat[0]"""
    if not (case.npool == "average" and case.eps):
        return False
    return bool((np.bincount(np.asarray(graph.edge_mat)[0], minlength=len(graph.g)) == 0).any())


def baseline_of(case):
    if not case.baseline:
        return None
    return (0.5 * np.random.default_rng(case.seed + 5).standard_normal((case.n, case.F0))).astype(np.float32)


# --------------------------------------------------------------------------- references
def _ographs(copies):
    from oracle import gin_oracle as O
    return [O.OGraph(len(c.g), np.asarray(c.edge_mat), np.asarray(c.node_features), getattr(c, "label", 0))
            for c in copies]


def oracle_scores64(state, spec, copies, group=16):
    """[len(copies), C] eval logits of explicit graphs through the fp64 oracle (graphs are independent in eval mode:
    several to a forward)"""
    from oracle import gin_oracle as O
    orc = O.OracleGIN(state, *spec, dtype=np.float64)
    out = []
    for i in range(0, len(copies), group):
        og = _ographs(copies[i:i + group])
        with np.errstate(all="ignore"):
            out.append(orc.forward(og, np.arange(len(og)), training=False, want_disc=False)[0])
    return np.concatenate(out, 0)


def torch_scores32(state, spec, copies, group=16):
    """the same through the independent fp32 CPU forward oracle.gin_torch_cpu.TorchCpuGIN"""
    from oracle.gin_torch_cpu import TorchCpuGIN
    cpu = TorchCpuGIN({k: np.asarray(v, dtype=np.float32) if np.asarray(v).dtype.kind == "f" else v
                       for k, v in state.items()}, *spec)
    out = []
    for i in range(0, len(copies), group):
        og = _ographs(copies[i:i + group])
        with torch.no_grad(), np.errstate(all="ignore"):
            out.append(cpu.forward(og, list(range(len(og))), training=False, want_disc=False)[0].numpy())
    return np.concatenate(out, 0)


def masked_forward64_sets(state, args, graph, sets, chunk=32):
    """test_lesion_host.masked_forward64 for many sets at once, [S, C]: the same formulation on the SOURCE graph (the
    adjacency's columns of D masked, the degree of the masked rows, rows of D zeroed in every layer's output, the readout
    over n - |D| nodes) with the sets as a batch dimension.  A row of D that is zero multiplies its column of A by zero,
    so A (h with rows of D zeroed) is (A with columns of D masked) h exactly; each BatchNorm is folded into the Linear
    before it.  Pinned to masked_forward64 and to the fp64 oracle on explicit copies by
    tests/test_rowblock_midrange_host.py."""
    L, m, learn_eps, gpool, npool = args
    p = {k: np.asarray(v, dtype=np.float64) for k, v in state.items() if np.asarray(v).dtype.kind == "f"}
    n = len(graph.g)
    sets = np.asarray(sets, dtype=bool).reshape(-1, n)
    em = np.asarray(graph.edge_mat).astype(np.int64).reshape(2, -1)
    A = np.zeros((n, n))
    np.add.at(A, (em[0], em[1]), 1.0)
    X = np.asarray(graph.node_features, dtype=np.float64)
    H = p["batch_norms.0.weight"].shape[0]
    lin = {}                                                      # the Linear with the BatchNorm behind it folded in
    for l in range(L):
        for k in range(m):
            wn = f"mlps.{l}.linear" if m == 1 else f"mlps.{l}.linears.{k}"
            bn = f"batch_norms.{l}" if k == m - 1 else f"mlps.{l}.batch_norms.{k}"
            sc = p[bn + ".weight"] / np.sqrt(p[bn + ".running_var"] + 1e-5)
            lin[l, k] = (np.ascontiguousarray(p[wn + ".weight"].T * sc),
                         (p[wn + ".bias"] - p[bn + ".running_mean"]) * sc + p[bn + ".bias"])
    chunk = min(chunk, sets.shape[0])
    # activations are [n, s, F]: node-major, so that A multiplies them as one [n, s F] matrix; four buffers, reused
    # (fresh 50 MB arrays cost more in page faults than the products cost in arithmetic)
    bufs = [np.empty(n * chunk * max(H, X.shape[1])) for _ in range(4)]

    def view(j, s, F):
        return bufs[j][:n * s * F].reshape(n, s, F)

    out = []
    for s0 in range(0, sets.shape[0], chunk):
        keep = np.ascontiguousarray(~sets[s0:s0 + chunk].T)       # [n, s]
        s = keep.shape[1]
        deg = A @ keep.astype(np.float64) + (0 if learn_eps else 1)
        scale = (1.0 / keep.sum(0)).astype(np.float32).astype(np.float64) if gpool == "average" else np.ones(s)
        cur = 3
        hself = view(cur, s, X.shape[1])
        hself[:] = X[:, None, :]
        hz = np.where(keep[:, :, None], hself, 0.0)               # (layer 0 alone: the self term keeps the row)
        score = 0.0
        with np.errstate(all="ignore"):
            for l in range(L):
                F = hz.shape[2]
                a, b = [j for j in range(4) if j != cur][:2]
                pooled = view(a, s, F)
                np.matmul(A, hz.reshape(n, s * F), out=pooled.reshape(n, s * F))
                if not learn_eps:
                    pooled += hself
                if npool == "average":
                    pooled /= deg[:, :, None]
                if learn_eps:
                    t = view(b, s, F)
                    np.multiply(hself, 1 + p["eps"][l], out=t)
                    pooled += t
                x, src = pooled.reshape(n * s, F), a
                for k in range(m):
                    W, bias = lin[l, k]
                    dst = b if src == a else a
                    y = view(dst, s, H).reshape(n * s, H)
                    np.matmul(x, W, out=y)
                    y += bias
                    np.maximum(y, 0, out=y)
                    x, src = y, dst
                cur = src
                hz = hself = x.reshape(n, s, H)
                hz[~keep] = 0.0                                   # zeros by assignment: a removed row's NaN is dropped
                score = score + (hz.sum(0) * scale[:, None]) @ p[f"linears_prediction.{l}.weight"].T \
                    + p[f"linears_prediction.{l}.bias"]
        out.append(score)
    return np.concatenate(out, 0)


LesionRef = collections.namedtuple("LesionRef", "sets names want_nan base64 base32 les64 les32")
OccRef = collections.namedtuple("OccRef", "named named64 masked64")


def lesion_reference_of(state, spec, graph, sets, npool, eps):
    copies = [graph] + [delete_nodes(graph, D) for D in sets]
    r64 = oracle_scores64(state, spec, copies)
    r32 = torch_scores32(state, spec, copies)
    want = np.array([expect_nan(graph, D, npool, eps) for D in sets], dtype=bool)
    return r64[0], r32[0], r64[1:], r32[1:], want


@functools.lru_cache(maxsize=None)
def lesion_reference(case):
    """per graph of the case: LesionRef(the sets [S, n], their names, expect_nan per set, base [C] and lesioned [S, C]
    through the fp64 oracle and through the fp32 CPU forward, both on explicit copies)"""
    out = []
    for d, g in enumerate(graphs_of(case)):
        sets, names = lesion_sets(case, d)
        b64, b32, l64, l32, want = lesion_reference_of(state_of(case), spec_of(case), g, sets, case.npool, case.eps)
        out.append(LesionRef(sets, names, want, b64, b32, l64, l32))
    return tuple(out)


def named_reference_of(state, spec, graph):
    """(the named nodes of a graph, the scores of their explicit one-node-deleted copies through the fp64 oracle)"""
    named = one_node_sets(len(graph.g))
    return named, oracle_scores64(state, spec, [delete_nodes(graph, [v]) for v in named])


@functools.lru_cache(maxsize=None)
def named_reference(case):
    return tuple(named_reference_of(state_of(case), spec_of(case), g) for g in graphs_of(case))


def occlusion_reference_of(state, spec, graph, named=None):
    n = len(graph.g)
    named, named64 = named or named_reference_of(state, spec, graph)
    return OccRef(named, named64, masked_forward64_sets(state, spec, graph, np.eye(n, dtype=bool)))


@functools.lru_cache(maxsize=None)
def occlusion_reference(case):
    """per graph of the case: OccRef(the named nodes, their explicit copies' scores through the fp64 oracle [k, C],
    every one-node set through masked_forward64_sets [n, C])"""
    return tuple(occlusion_reference_of(state_of(case), spec_of(case), g, nr)
                 for g, nr in zip(graphs_of(case), named_reference(case)))


@functools.lru_cache(maxsize=None)
def ig_reference(case, dtype="float64"):
    """per graph of the case: oracle_ig's (attr [2, n, F0], base [2], base0 [2]) at the case's rule, K and baseline"""
    alphas, weights = quadrature(case.method, case.K)
    return tuple(oracle_ig(state_of(case), spec_of(case), g, (0, 1), alphas, weights, baseline_of(case),
                           dtype=np.dtype(dtype).type) for g in graphs_of(case))


@functools.lru_cache(maxsize=None)
def ragged_reference():
    """(graphs, sets, per graph (base64, base32, les64, les32, want_nan), per graph OccRef) of the ragged batch"""
    gs = ragged_graphs()
    sets = ragged_sets(gs)
    c = RAGGED_CASE
    les = tuple(lesion_reference_of(state_of(c), spec_of(c), g, S, c.npool, c.eps) for g, S in zip(gs, sets))
    occ = tuple(occlusion_reference_of(state_of(c), spec_of(c), g) for g in gs)
    return gs, sets, les, occ


def fp32_noise(base32, base64, les32, les64):
    """the distance of the fp32 CPU forward from the fp64 oracle on a graph and its finite deleted copies, as the GPU
    tests measure theirs: max-norm relative to the graph's max |base|"""
    from helpers import rel_err
    fin = ~np.isnan(les64).any(1)
    e = rel_err(base32, base64)
    if fin.any():
        e = max(e, rel_err(les32[fin], les64[fin], floor=float(np.abs(base64).max())))
    return e


def err(a, ref, floor):
    """helpers.rel_err (NaN patterns equal), also where every entry is NaN"""
    from helpers import rel_err
    a, ref = np.asarray(a, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    if ref.size and np.isnan(ref).all():
        assert a.shape == ref.shape and np.isnan(a).all(), "NaN pattern differs"
        return 0.0
    return rel_err(a, ref, floor=floor)


# integrated_gradients() differentiates through the ReLUs, so unlike the scores its result is not continuous in the
# rounding: a pre-activation whose sign fp32 arithmetic does not determine makes two correct fp32 backwards differ by a
# whole path weight (seen: 5e-3 of max |attr| from one unit at 1.5e-8 of its layer's largest).  A pre-activation is a sum
# whose partial sums reach the layer's scale and are each rounded to 2^-24 relative, so below one fp32 ulp at that scale
# -- 2^-23 x the layer's largest |pre-activation| -- its sign is noise.  No case may have one there, at any quadrature
# point, judged by the fp64 oracle alone; a case that has is given another seed (SEEDS).
IG_RELU_MARGIN = 2.0 ** -23


@functools.lru_cache(maxsize=None)
def ig_relu_margin(case):
    """the smallest |pre-activation under a ReLU| / the largest of the same BatchNorm output, over the layers, the
    quadrature points and the two graphs of a case, in the fp64 oracle's eval forward"""
    from oracle import gin_oracle as O
    from test_intgrad_host import _arrays, _ograph
    orc = O.OracleGIN(state_of(case), *spec_of(case), dtype=np.float64)
    seen = []
    inner = orc._bn_apply

    def spy(x, prefix, training, update):
        y, c = inner(x, prefix, training, update)
        seen.append(float(np.abs(y).min() / np.abs(y).max()))
        return y, c
    orc._bn_apply = spy
    for g in graphs_of(case):
        X, x0 = _arrays(g, baseline_of(case), np.float64)
        for a in quadrature(case.method, case.K)[0]:
            with np.errstate(all="ignore"):
                orc.forward([_ograph(O, g, x0 + a * (X - x0))], np.arange(1), training=False, want_disc=False)
    return min(seen)


# =========================================================================== saliency, class activation, edge saliency
# The gradient maps -- saliency(), class_activation() of both kinds, edge_saliency() -- on the same table
# (tests/test_gpu_attribution_midrange.py on the GPU, tests/test_attribution_midrange_host.py without one).  Like
# integrated_gradients() they differentiate through the ReLUs, here at the graph's OWN features, which IG_RELU_MARGIN's
# check above reaches only where alpha = 1 is a quadrature point.  A case that breaks a condition of the host test at its
# own features -- the margin, or the fp32 references' distance from the fp64 ones -- is used by these tests as a variant
# with another model seed (grad_case: the id gains "-g"); SEEDS and the cases above stay as they are.
GRAD_SEEDS = {
    # a pre-activation under a ReLU below IG_RELU_MARGIN in the plain eval forward of one of the case's graphs
    # with the table's seed: margin before -> after
    "n190-H128-m1-sum-sum-eps1": 2429,                  # 1.1e-07 -> 1.3e-06
    "n256-H32-m2-average-sum-eps1": 4334,               # 3.6e-08 -> 1.1e-05
    "n257-H64-m2-sum-sum-eps1": 1366,                   # 6.4e-09 -> 2.3e-06 (8.1e-07 with batch_graphs()' third graph)
    "n416-H64-m2-average-average-eps1-ragged": 3366,    # 9.4e-08 -> 5.9e-07 (over ragged_graphs())
}

AttrRef = collections.namedtuple("AttrRef", "sal cam gcam edge")    # per map [len(classes), ...], None where not asked
MAPS = AttrRef._fields


def grad_case(case):
    """the case as the gradient-map tests use it: itself, or its reseeded "-g" variant (same graphs, other model)"""
    if case.id not in GRAD_SEEDS:
        return case
    return case._replace(seed=GRAD_SEEDS[case.id], id=case.id + "-g")


def grad_cases(n):
    return tuple(grad_case(c) for c in cases(n))


def cam_blocks(n):
    """(64-row blocks of gnm_class_activation_kernel, live second-half rows r0 + 32 < n of the last one)"""
    nb = (n + 63) // 64
    return nb, min(max(n - 64 * (nb - 1) - 32, 0), 32)


def correction_words(n):
    """the word indices j >> 3 the average correction of gnm_edge_saliency_kernel reads in a half row: bytes
    j < ceil(n / 8), byte j in word j >> 3 of half j & 1"""
    return sorted({j >> 3 for j in range((n + 7) // 8)})


def dx_form(f0):
    """(NCO, KS, form) of the final dX launch of gnm_saliency_layer_kernel at input width f0: NCO = ceil(f0 / 32)
    column tiles; under 4 the 4 waves split the contraction KS = 4 / NCO ways, from 4 on each wave takes whole tiles"""
    nco = (f0 + 31) // 32
    if nco >= 4:
        return nco, 0, "wave per tile" if nco == 4 else "wave 0 takes %d tiles" % len(range(0, nco, 4))
    ks = 4 // nco
    return nco, ks, "KS = %d%s" % (ks, ", %d idle" % (4 - nco * ks) if nco * ks < 4 else "")


# ---- the input-width forms of the final dX launch: F0 over the NCO = 2 .. 5 forms at two row blocks (n = 40, 8 live
# rows in the second) and two of them at n = 97; (H, m) and the pooling forms cycled; dense Gaussian features
WIDTHS = ((40, 33), (40, 64), (40, 65), (40, 96), (40, 97), (40, 128), (40, 129), (97, 65), (97, 129))
WIDTH_HM = ((32, 1), (64, 2), (128, 3))
WIDTH_STEPS = 2


def _width_case(i, n, f0):
    H, m = WIDTH_HM[i % 3]
    c = _case(n, H, m, i, i // 3, tag="-F%d" % f0)
    return c._replace(F0=f0, K=WIDTH_STEPS, method="midpoint", baseline=False)


WIDTH_CASES = tuple(_width_case(i, n, f0) for i, (n, f0) in enumerate(WIDTHS))

# ---- the batch sizes: one case of n = 257 with a third graph
BATCH_CASE = cases(257)[4]                                           # H = 64, m = 2


def batch_graphs():
    from test_gpu_saliency import random_graph
    return graphs_of(grad_case(BATCH_CASE)) + [random_graph(7200, 257, 24.0 / 257, F0, directed=True)]


def relu_margin_of(state, spec, graphs):
    """ig_relu_margin's measure for ONE plain eval forward of each graph at its own features (no baseline, no
    quadrature): the smallest |pre-activation under a ReLU| / the largest of the same BatchNorm output, fp64 oracle"""
    from oracle import gin_oracle as O
    orc = O.OracleGIN(state, *spec, dtype=np.float64)
    seen = []
    inner = orc._bn_apply

    def spy(x, prefix, training, update):
        y, c = inner(x, prefix, training, update)
        seen.append(float(np.abs(y).min() / np.abs(y).max()))
        return y, c
    orc._bn_apply = spy
    for og in _ographs(graphs):
        with np.errstate(all="ignore"):
            orc.forward([og], np.arange(1), training=False, want_disc=False)
    assert len(seen) == len(graphs) * spec[0] * spec[1]
    return min(seen)


@functools.lru_cache(maxsize=None)
def relu_margin(case):
    return relu_margin_of(state_of(case), spec_of(case), graphs_of(case))


def attribution_reference_of(state, spec, graph, classes, dtype, maps=MAPS):
    """AttrRef of one graph in `dtype` ("float64" / "float32"): sal [C, n, F0] through OracleGIN.compute_saliency, cam and
    gcam [C, n] through test_cam_host.restate, edge [C, n, n] through test_edge_saliency_host.restate_edge"""
    from oracle import gin_oracle as O
    from test_cam_host import restate
    from test_edge_saliency_host import restate_edge
    npdt, tdt = np.dtype(dtype).type, getattr(torch, dtype)
    em = np.asarray(graph.edge_mat)
    feats = np.asarray(graph.node_features)
    out = dict.fromkeys(MAPS)
    with np.errstate(all="ignore"):
        if "sal" in maps:
            orc = O.OracleGIN(state, *spec, dtype=npdt)
            og = _ographs([graph])[0]
            out["sal"] = np.stack([orc.compute_saliency(og, c) for c in classes])
        if "cam" in maps or "gcam" in maps:
            r = [restate(state, *spec, em[0], em[1], graph.neighbors, feats, c, dtype=tdt) for c in classes]
            out["cam"] = np.stack([x[2].numpy() for x in r])
            out["gcam"] = np.stack([x[3].numpy() for x in r])
        if "edge" in maps:
            out["edge"] = np.stack([restate_edge(state, *spec, em[0], em[1], feats, c, dtype=tdt).numpy()
                                    for c in classes])
    return AttrRef(**out)


@functools.lru_cache(maxsize=None)
def attribution_reference(case, dtype="float64", classes=(0, 1), maps=MAPS):
    """per graph of the case: its AttrRef for `classes`"""
    return tuple(attribution_reference_of(state_of(case), spec_of(case), g, classes, dtype, maps)
                 for g in graphs_of(case))


@functools.lru_cache(maxsize=None)
def ragged_attribution_reference(dtype="float64"):
    c = grad_case(RAGGED_CASE)
    return tuple(attribution_reference_of(state_of(c), spec_of(c), g, (0, 1), dtype) for g in ragged_graphs())


@functools.lru_cache(maxsize=None)
def batch_attribution_reference(dtype="float64"):
    c = grad_case(BATCH_CASE)
    return tuple(attribution_reference_of(state_of(c), spec_of(c), g, (0, 1), dtype) for g in batch_graphs())


def class_maps(case):
    """the maps the 11-class tests ask of a CLASS_CASES entry: both class activation kinds, and at n = 129 all four"""
    return MAPS if case.n == 129 else ("cam", "gcam")


def class_attribution_reference(case, dtype="float64"):
    """attribution_reference of an 11-class case for all 11 classes"""
    return attribution_reference(case, dtype, tuple(range(case.C)), class_maps(case))


def attr_noise(ref32, ref64):
    """the fp32 reference's distance from the fp64 one on a graph: the worst, over the classes, of the max-norm distance
    relative to that class's max |ref64|"""
    from helpers import rel_err
    return max(rel_err(a, b) for a, b in zip(ref32, ref64))


def attr_bound(ref32, ref64):
    """helpers.Calibrated's rule on attr_noise: max(RTOL, 4 x the fp32 reference's distance from fp64)"""
    from helpers import RTOL, TRUE_SHAPE_FACTOR
    return max(RTOL, TRUE_SHAPE_FACTOR * attr_noise(ref32, ref64))


# =========================================================================== disconnect
# disconnect() / disconnection_matrix() (csrc/disconnect.hip, rb_stage_bits_cut of csrc/gnm_rowblock.h) on the same table
# (tests/test_gpu_disconnect_midrange.py on the GPU, tests/test_disconnect_midrange_host.py without one).  What a cut has
# that a lesion has not is a lookup per ROW -- whether row r is in A, in B, in both or in neither (rb_row_bit on the two
# keep masks) -- so the pairs below name rows by the fields of that lookup: the word r >> 6, the half (r >> 3) & 1, the
# byte (r >> 4) & 3.  A case that breaks a condition of the host test is used as a variant with another model seed
# (dc_case: the id gains "-d"); SEEDS, GRAD_SEEDS and the cases above stay as they are.
DC_SEEDS = {
    # case id: seed, with the condition's value before -> after.  No case needs one: with the table's seeds the fp32 CPU
    # forward is at most 4.3e-6 from fp64 on the cut copies (cap 5e-6) and every wrong formulation at least 1.9e-4 away
}
WORD_EDGES = (63, 127, 191, 255)                    # rows e, e + 1: either side of a 64-row word of the keep masks
MATRIX_NETWORKS = 5

DisconnectRef = collections.namedtuple("DisconnectRef", "a b names want_nan base64 base32 dis64 dis32")


def dc_case(case):
    """the case as the disconnect tests use it: itself, or its reseeded "-d" variant (same graphs, other model)"""
    if case.id not in DC_SEEDS:
        return case
    return case._replace(seed=DC_SEEDS[case.id], id=case.id + "-d")


def dc_cases(n):
    return tuple(dc_case(c) for c in cases(n))


def all_dc_cases():
    """the 63 cases of the matrix and the one-hot case of n = 257"""
    return tuple(c for n in NODES for c in dc_cases(n))


def dc_matrix_case(n):
    """the case of n that carries the disconnection_matrix() test: H = 64, m = 2, dense features"""
    return next(c for c in dc_cases(n) if c.H == 64 and c.m == 2 and not c.one_hot)


def disconnect_pairs(case, d):
    """the set pairs of graph d of a case: (names, A [S, n] bool, B [S, n] bool)"""
    n = case.n
    rng = np.random.default_rng(case.seed * 11 + d + n)
    idx = np.arange(n)
    W = row_blocks(n)
    none, every = np.zeros(n, dtype=bool), np.ones(n, dtype=bool)
    P = [("empty", none, none),
         ("last-node x all", idx == n - 1, every),                                # a node isolated, dead rows behind it
         ("block-0 x block-1", block_of(n, 0), block_of(n, 1)),                   # the ring edge 31 -> 32 is cut
         ("block-%d x block-%d" % (W - 2, W - 1), block_of(n, W - 2), block_of(n, W - 1)),
         ("block-2 within itself", block_of(n, 2), block_of(n, 2)),               # rows in A and in B: both masks
         ("half rows", ((idx >> 3) & 1) == 0, ((idx >> 3) & 1) == 1),             # the h * HPW half select
         ("bytes", ((idx >> 4) & 3) == 1, ((idx >> 4) & 3) == 3)]                 # the byte shift
    for e in WORD_EDGES:
        if n > e + 1:
            P.append(("word edge %d" % e, np.isin(idx, (e, e + 1)),
                      np.isin(idx, (e + 1, min(e + 2, n - 1))) | block_of(n, 0)))
    half = np.isin(idx, rng.choice(n, n // 2, replace=False))
    P.append(("half x complement", half, ~half))
    P.append(("overlapping random sets", rng.random(n) < 0.35, rng.random(n) < 0.35))
    P.append(("all x all", every, every))                                         # the edgeless graph
    return [k for k, _, _ in P], np.stack([a for _, a, _ in P]), np.stack([b for _, _, b in P])


def disconnect_reference_of(state, spec, graph, a, b, npool, eps):
    """(base64 [C], base32, disconnected64 [S, C], disconnected32, want_nan [S]) of a graph's pairs: the fp64 oracle and
    the independent fp32 CPU forward on explicit edge-cut copies (test_disconnect_host.cut_edges)"""
    from test_disconnect_host import cut_edges, expect_nan_cut
    copies = [graph] + [cut_edges(graph, A, B) for A, B in zip(a, b)]
    r64 = oracle_scores64(state, spec, copies)
    r32 = torch_scores32(state, spec, copies)
    want = np.array([expect_nan_cut(graph, A, B, npool, eps) for A, B in zip(a, b)], dtype=bool)
    return r64[0], r32[0], r64[1:], r32[1:], want


@functools.lru_cache(maxsize=None)
def disconnect_reference(case):
    """per graph of the case: DisconnectRef(A [S, n], B [S, n], the pairs' names, expect_nan_cut per pair, base [C] and
    disconnected [S, C] through the fp64 oracle and through the fp32 CPU forward, both on explicit copies)"""
    out = []
    for d, g in enumerate(graphs_of(case)):
        names, a, b = disconnect_pairs(case, d)
        b64, b32, d64, d32, want = disconnect_reference_of(state_of(case), spec_of(case), g, a, b, case.npool, case.eps)
        out.append(DisconnectRef(a, b, names, want, b64, b32, d64, d32))
    return tuple(out)


def matrix_labels(case, d):
    """the network labelling of graph d for disconnection_matrix(): MATRIX_NETWORKS networks, every 23rd node of none"""
    lab = np.random.default_rng(case.seed * 13 + d + case.n).integers(0, MATRIX_NETWORKS, case.n)
    lab[d::23] = -1
    return lab


@functools.lru_cache(maxsize=None)
def matrix_reference(case):
    """per graph of the case: DisconnectRef of the 15 pairs of gnm.lesion.pair_sets(matrix_labels) (names: the pairs)"""
    from gnm.lesion import pair_sets
    out = []
    for d, g in enumerate(graphs_of(case)):
        a, b, pairs = pair_sets(matrix_labels(case, d), MATRIX_NETWORKS)
        b64, b32, d64, d32, want = disconnect_reference_of(state_of(case), spec_of(case), g, a, b, case.npool, case.eps)
        out.append(DisconnectRef(a, b, [tuple(p) for p in pairs.tolist()], want, b64, b32, d64, d32))
    return tuple(out)


def row_bit_word(n, r):
    """the word of a keep mask rb_row_bit reads for row r: ((r >> 3) & 1) * HPW + (r >> 6)"""
    return ((r >> 3) & 1) * half_words(n) + (r >> 6)


def cut_keep(a, b):
    """the keep matrix of the cut: entry (r, c) is False where row r is in A and column c in B, or r in B and c in A"""
    return (~a[:, None] | ~b[None, :]) & (~b[:, None] | ~a[None, :])


def keep_forward64(state, args, graph, keep, uncut_degree=False):
    """test_disconnect_host.cut_forward64 for any per-row keep matrix [n, n] (entry (r, c): row r keeps column c), or a
    batch [K, n, n] of them, in fp64 numpy on the SOURCE graph: the masked adjacency, its degree -- or, uncut_degree, the
    degree of the unmasked row -- every row kept, the readout over all n nodes.  [C] or [K, C] logits.  With
    cut_keep(A, B) it is cut_forward64 (pinned by the host test); with another matrix it is a wrong formulation for the
    host test to tell apart."""
    L, m, learn_eps, gpool, npool = args
    p = {k: np.asarray(v, dtype=np.float64) for k, v in state.items() if np.asarray(v).dtype.kind == "f"}
    n = len(graph.g)
    keep = np.asarray(keep, dtype=bool)
    single = keep.ndim == 2
    keep = keep.reshape(-1, n, n)
    em = np.asarray(graph.edge_mat).astype(np.int64).reshape(2, -1)
    adj = np.bincount(em[0] * n + em[1], minlength=n * n).reshape(n, n).astype(np.float64)
    Am = adj[None] * keep
    deg = (np.broadcast_to(adj, Am.shape) if uncut_degree else Am).sum(2) + (0 if learn_eps else 1)      # [K, n]

    def bn(x, name):
        return (x - p[name + ".running_mean"]) / np.sqrt(p[name + ".running_var"] + 1e-5) * p[name + ".weight"] \
            + p[name + ".bias"]

    h = np.broadcast_to(np.asarray(graph.node_features, dtype=np.float64), (keep.shape[0], n, graph.node_features.shape[1]))
    score = 0.0
    scale = float(np.float32(1.0 / n)) if gpool == "average" else 1.0
    with np.errstate(all="ignore"):
        for l in range(L):
            pooled = Am @ h
            if not learn_eps:
                pooled = pooled + h
            if npool == "average":
                pooled = pooled / deg[:, :, None]
            if learn_eps:
                pooled = pooled + (1 + p["eps"][l]) * h
            x = pooled
            for k in range(m):
                wn = f"mlps.{l}.linear" if m == 1 else f"mlps.{l}.linears.{k}"
                x = x @ p[wn + ".weight"].T + p[wn + ".bias"]
                x = np.maximum(bn(x, f"batch_norms.{l}" if k == m - 1 else f"mlps.{l}.batch_norms.{k}"), 0)
            h = x
            score = score + (h.sum(1) * scale) @ p[f"linears_prediction.{l}.weight"].T + p[f"linears_prediction.{l}.bias"]
    return score[0] if single else score


MUTANTS = ("masks swapped", "one-sided cut", "row bits of the high words lost", "column bits of the high words lost",
           "row membership from the other half", "degree of the uncut row")


def _rows_lost(a, b, high):
    """rows of the high words are taken to be in neither set; the column masks are whole"""
    ar, br = a & ~high, b & ~high
    return (~ar[:, None] | ~b[None, :]) & (~br[:, None] | ~a[None, :])


def disconnect_mutants(a, b, n):
    """wrong formulations of the cut of (A, B) on an n-node graph, for the host test only: name -> (keep matrix [n, n],
    uncut_degree) for keep_forward64.  "High words": word index r >> 6 of a half row from 2 on (n <= 256, HPW = 4: the
    second half of the one 128-bit load) or from 4 on (n > 256, HPW = 8: the second load)."""
    a, b = np.asarray(a, dtype=bool), np.asarray(b, dtype=bool)
    idx = np.arange(n)
    high = (idx >> 6) >= (2 if n <= 256 else 4)
    right = cut_keep(a, b)
    other = idx ^ 8                                   # a keep mask is zero at columns >= n: such a row reads "in the set"
    ao = np.where(other < n, a[np.minimum(other, n - 1)], True)
    bo = np.where(other < n, b[np.minimum(other, n - 1)], True)
    return {
        "masks swapped": ((~a[:, None] | ~a[None, :]) & (~b[:, None] | ~b[None, :]), False),   # rows of A lose A
        "one-sided cut": (~a[:, None] | ~b[None, :], False),                                    # rows of B keep A
        "row bits of the high words lost": (_rows_lost(a, b, high), False),
        "column bits of the high words lost": (right | high[None, :], False),
        "row membership from the other half": ((~ao[:, None] | ~b[None, :]) & (~bo[:, None] | ~a[None, :]), False),
        "degree of the uncut row": (right, True),
    }
