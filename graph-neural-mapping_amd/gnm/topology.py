"""Graph-theoretic measures of connectome graphs, on the device (csrc/topology.hip).  Re-exported by gnm.connectome.

    m = graph_measures(model_or_arena, graphs, local_efficiency=True)     # GraphMeasures of device tensors
    h = graph_measures_host(adjacency_or_edge_list, n)                    # the same fields of one graph, in numpy

The graphs are read as simple undirected graphs: a repeated edge counts once and a self loop is dropped.  With c_k the
number of nodes at distance k from node v, d its degree and t the pairs of adjacent neighbours it has:

  per node    degree, triangles, clustering = (2.0 * t) / (d * (d - 1)) (0.0 for d < 2), eccentricity (the last k with
              c_k > 0; 0 for an isolated node), reachable = sum c_k, distance_sum = sum k c_k, component (the smallest
              node id reached, v included), nodal_efficiency = eff(c, n - 1) (0.0 for n = 1), local_efficiency =
              eff(H_v, d (d - 1)) with H_v[k] the ordered pairs of neighbours of v at distance k inside the subgraph the
              neighbours induce (0.0 for d < 2: networkx's global_efficiency(G.subgraph(G[v])))
  per graph   edges, components, distance_histogram (column k: the ordered pairs at distance k), diameter (the largest
              finite distance), global_efficiency = eff(histogram, n (n - 1)) (0.0 for n < 2),
              characteristic_path_length = sum k C[k] / sum C[k] (NaN when no pair is connected), transitivity =
              sum_v t_v / sum_v d_v (d_v - 1) / 2 (three times the triangles over the connected triples; 0.0 without
              triples), mean_clustering and mean_local_efficiency (the nodes' values added in ascending order, then one
              division by n)

where eff(H, m) is   acc = 0.0;  for k = 1, 2, ..: if H[k]: acc = acc + float(H[k]) / float(k);   acc / float(m).
Everything before those fp64 formulas is integer work, and both sides apply them to the same integers in the same
order, so the device's fields are bitwise graph_measures_host's, whatever batch a graph is part of.
"""
import numpy as np
import torch

from ._cabi import GnmError, check, lib

NODE_FIELDS = ("degree", "triangles", "clustering", "eccentricity", "reachable", "distance_sum", "component",
               "nodal_efficiency", "local_efficiency")
GRAPH_FIELDS = ("edges", "components", "distance_histogram", "diameter", "global_efficiency",
                "characteristic_path_length", "transitivity", "mean_clustering", "mean_local_efficiency")
_DTYPES = {"degree": "int32", "triangles": "int32", "clustering": "float64", "eccentricity": "int32",
           "reachable": "int32", "distance_sum": "int32", "component": "int32", "nodal_efficiency": "float64",
           "local_efficiency": "float64", "edges": "int64", "components": "int32", "distance_histogram": "int64",
           "diameter": "int32", "global_efficiency": "float64", "characteristic_path_length": "float64",
           "transitivity": "float64", "mean_clustering": "float64", "mean_local_efficiency": "float64"}


class GraphMeasures:
    """The measures of B graphs.  NODE_FIELDS are [N] arrays in batch order (graph i owns rows node_off[i] ..
    node_off[i + 1]), GRAPH_FIELDS [B] arrays, distance_histogram [B, n_max]; int32, int64 and float64 as the module's
    docstring lists them; device tensors from graph_measures, numpy arrays from graph_measures_host.  node_off is a host
    int64 array [B + 1].  local_efficiency and mean_local_efficiency are None when they were not asked for."""

    __slots__ = NODE_FIELDS + GRAPH_FIELDS + ("node_off",)

    def __init__(self, node_off, **fields):
        self.node_off = np.asarray(node_off, dtype=np.int64)
        for name in NODE_FIELDS + GRAPH_FIELDS:
            setattr(self, name, fields[name])

    def __len__(self):
        return int(self.node_off.shape[0]) - 1

    def __repr__(self):
        return "GraphMeasures(graphs=%d, nodes=%d, local_efficiency=%s)" % (
            len(self), int(self.node_off[-1]), self.local_efficiency is not None)

    def graph(self, i):
        """the measures of graph i alone: views of its node rows, its entry of every per-graph array, and its histogram
        row cut to its own node count"""
        B = len(self)
        if not -B <= i < B:
            raise IndexError("graph %d of %d" % (i, B))
        i %= B
        lo, hi = int(self.node_off[i]), int(self.node_off[i + 1])
        out = {}
        for name in NODE_FIELDS:
            a = getattr(self, name)
            out[name] = None if a is None else a[lo:hi]
        for name in GRAPH_FIELDS:
            a = getattr(self, name)
            out[name] = None if a is None else a[i:i + 1]
        out["distance_histogram"] = out["distance_histogram"][:, :max(hi - lo, 1)]
        return GraphMeasures([0, hi - lo], **out)

    def numpy(self):
        """the same record with every field a host numpy array"""
        conv = lambda a: None if a is None else (a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a))
        return GraphMeasures(self.node_off, **{name: conv(getattr(self, name)) for name in NODE_FIELDS + GRAPH_FIELDS})


def graph_measures(model_or_arena, graphs, local_efficiency=True):
    """GraphMeasures of `graphs` (anything GraphArena.batch takes: S2VGraph-shaped objects or ConnectomeGraphs, ragged
    node counts allowed), registered in the arena (a model means model.arena()) if they are not yet.  Two launches, one
    workgroup per graph; local_efficiency=False skips the second and leaves the two local fields None.
    ValueError for a graph that is not symmetric; GnmError for a graph above gnm_topology_max_nodes() nodes and for an
    arena that is not on a GPU: all before anything is launched.  An empty list gives empty arrays."""
    arena = model_or_arena.arena() if hasattr(model_or_arena, "arena") and callable(model_or_arena.arena) \
        else model_or_arena
    graphs = list(graphs)
    dev = arena.device
    limit = int(lib.gnm_topology_max_nodes())

    def alloc(name, *shape):
        return torch.empty(shape, dtype=getattr(torch, _DTYPES[name]), device=dev)

    if not graphs:
        f = {name: alloc(name, 0) for name in NODE_FIELDS + GRAPH_FIELDS}
        f["distance_histogram"] = alloc("distance_histogram", 0, 0)
        if not local_efficiency:
            f["local_efficiency"] = f["mean_local_efficiency"] = None
        return GraphMeasures([0], **f)
    batch = arena.batch(graphs)
    if not batch.symmetric:
        bad = [i for i, g in enumerate(arena.add_many(graphs)) if not arena.sym[g]]
        raise ValueError("graph_measures: graphs %s are not symmetric; the measures are those of undirected graphs"
                         % bad[:8])
    if batch.n_max > limit:
        raise GnmError("graph_measures: a graph of %d nodes; at most %d are supported (gnm_topology_max_nodes: the bit "
                       "rows of a graph stay in one CU's LDS)" % (batch.n_max, limit))
    if dev.type != "cuda":
        raise GnmError("graph measures are computed on the GPU only (libgnm_hip.so); the arena is on %s" % dev)
    B, N, n_max = batch.B, batch.N, max(batch.n_max, 1)
    f = {name: alloc(name, N) for name in NODE_FIELDS}
    f.update({name: alloc(name, B) for name in GRAPH_FIELDS})
    f["distance_histogram"] = alloc("distance_histogram", B, n_max)
    if not local_efficiency:
        f["local_efficiency"] = f["mean_local_efficiency"] = None
    csr = batch.csr_ptrs()
    with torch.cuda.device(dev):
        st = torch.cuda.current_stream(dev).cuda_stream
        check(lib.gnm_topology_nodes(*csr, batch.node_off.data_ptr(), B, n_max, f["degree"].data_ptr(),
                                     f["triangles"].data_ptr(), f["clustering"].data_ptr(),
                                     f["eccentricity"].data_ptr(), f["reachable"].data_ptr(),
                                     f["distance_sum"].data_ptr(), f["component"].data_ptr(),
                                     f["nodal_efficiency"].data_ptr(), f["edges"].data_ptr(),
                                     f["components"].data_ptr(), f["distance_histogram"].data_ptr(),
                                     f["diameter"].data_ptr(), f["global_efficiency"].data_ptr(),
                                     f["characteristic_path_length"].data_ptr(), f["transitivity"].data_ptr(),
                                     f["mean_clustering"].data_ptr(), st), "gnm_topology_nodes")
        if local_efficiency:
            nbytes = int(lib.gnm_topology_workspace_bytes(B, n_max, 1))
            work = torch.empty(nbytes, dtype=torch.uint8, device=dev) if nbytes > 0 else None
            check(lib.gnm_topology_local(*csr, batch.node_off.data_ptr(), B, n_max,
                                         None if work is None else work.data_ptr(), f["local_efficiency"].data_ptr(),
                                         f["mean_local_efficiency"].data_ptr(), st), "gnm_topology_local")
    return GraphMeasures(batch.node_off_host, **f)


# ---------------------------------------------------------------------------------------------------- the numpy oracle
def _adjacency(graph, n):
    """[n, n] bool, symmetric, empty diagonal: from a bool [n, n] adjacency (either triangle may hold an edge) or an
    integer [E, 2] edge list (each pair in any order, repeated pairs and self loops allowed)"""
    a = graph.detach().cpu().numpy() if torch.is_tensor(graph) else np.asarray(graph)
    if a.dtype == np.bool_:
        if n is None:
            n = a.shape[0]
        if a.shape != (n, n):
            raise ValueError("a bool adjacency must be [n, n] = [%d, %d], got %s" % (n, n, a.shape))
        A = a.copy()
    elif a.dtype.kind in "iu" or a.size == 0:
        if n is None:
            raise ValueError("an edge list needs the node count n")
        e = a.astype(np.int64).reshape(-1, 2)
        if e.size and (e.min() < 0 or e.max() >= n):
            raise ValueError("edge list: node ids must lie in 0 .. %d" % (n - 1))
        A = np.zeros((n, n), dtype=bool)
        A[e[:, 0], e[:, 1]] = True
    else:
        raise ValueError("give a bool [n, n] adjacency or an integer [E, 2] edge list, got %s %s" % (a.dtype, a.shape))
    A = A | A.T
    A[np.arange(n), np.arange(n)] = False
    return A


def _distances(A):
    """[n, n] int32 shortest-path lengths of the bool adjacency A, -1 where there is no path: level-synchronous BFS from
    every node at once, (F @ A > 0) & ~visited in float32 (sums of at most n ones: exact below 2^24)"""
    n = A.shape[0]
    Af = A.astype(np.float32)
    D = np.full((n, n), -1, dtype=np.int32)
    D[np.arange(n), np.arange(n)] = 0
    visited = np.eye(n, dtype=bool)
    F = visited.copy()
    k = 0
    while F.any():
        k += 1
        F = ((F.astype(np.float32) @ Af) > 0) & ~visited
        D[F] = k
        visited |= F
    return D


def _level_counts(D):
    """[n, K + 1] int64: column k = the nodes at distance k of each row's node (column 0 zeroed), K the largest distance"""
    n = D.shape[0]
    K = int(D.max()) if n else 0
    C = np.zeros((n, K + 1), dtype=np.int64)
    rows, cols = np.nonzero(D > 0)
    np.add.at(C, (rows, D[rows, cols]), 1)
    return C


def _eff(H, m):
    """eff(H, m) of the module's docstring with Python floats (IEEE fp64)"""
    acc = 0.0
    for k in range(1, len(H)):
        if H[k]:
            acc = acc + float(int(H[k])) / float(k)
    return acc / float(m)


def _seq_mean(x):
    acc = 0.0
    for v in x:
        acc = acc + float(v)
    return acc / float(len(x)) if len(x) else 0.0


def graph_measures_host(graph, n=None, local_efficiency=True):
    """The measures of ONE graph in plain numpy, a GraphMeasures of numpy arrays (B = 1): the oracle the kernels are
    tested against, formulas and their order as the module's docstring states them.  graph: a bool [n, n] adjacency or
    an integer [E, 2] edge list with the node count n; made symmetric, repeated edges and self loops ignored."""
    A = _adjacency(graph, n)
    n = A.shape[0]
    Af = A.astype(np.float32)
    deg = A.sum(1).astype(np.int64)
    tri = ((Af @ Af) * Af).sum(1, dtype=np.float64).astype(np.int64) // 2        # entries <= n: exact
    clu = np.zeros(n, dtype=np.float64)
    ok = deg >= 2
    clu[ok] = (2.0 * tri[ok].astype(np.float64)) / (deg[ok] * (deg[ok] - 1)).astype(np.float64)
    D = _distances(A)
    C = _level_counts(D)
    K = C.shape[1] - 1
    ks = np.arange(K + 1, dtype=np.int64)
    ecc = np.where(C > 0, ks[None, :], 0).max(1) if n else np.zeros(0, np.int64)
    reach = C.sum(1)
    dsum = (C * ks[None, :]).sum(1)
    comp = np.where(D >= 0, np.arange(n)[None, :], n).min(1) if n else np.zeros(0, np.int64)
    acc = np.zeros(n, dtype=np.float64)
    for k in range(1, K + 1):                       # ascending k, every node at once: the scalar formula elementwise
        m = C[:, k] > 0
        acc[m] = acc[m] + C[m, k].astype(np.float64) / float(k)
    nodal = acc / float(n - 1) if n > 1 else np.zeros(n, dtype=np.float64)
    hist = np.zeros(max(n, 1), dtype=np.int64)
    hist[:K + 1] = C.sum(0)
    pairs, dist = int(hist.sum()), int((hist * np.arange(hist.shape[0])).sum())
    triples = int((deg * (deg - 1) // 2).sum())
    out = dict(degree=deg, triangles=tri, clustering=clu, eccentricity=ecc, reachable=reach, distance_sum=dsum,
               component=comp, nodal_efficiency=nodal, local_efficiency=None,
               edges=[int(deg.sum()) // 2], components=[int((comp == np.arange(n)).sum())],
               distance_histogram=hist[None, :], diameter=[K],
               global_efficiency=[_eff(hist, n * (n - 1)) if n > 1 else 0.0],
               characteristic_path_length=[float(dist) / float(pairs) if pairs else float("nan")],
               transitivity=[float(int(tri.sum())) / float(triples) if triples else 0.0],
               mean_clustering=[_seq_mean(clu)], mean_local_efficiency=None)
    if local_efficiency:
        loc = np.zeros(n, dtype=np.float64)
        for v in range(n):
            d = int(deg[v])
            if d < 2:
                continue
            S = np.flatnonzero(A[v])
            Cs = _level_counts(_distances(A[np.ix_(S, S)]))
            loc[v] = _eff(Cs.sum(0), d * (d - 1))
        out["local_efficiency"] = loc
        out["mean_local_efficiency"] = [_seq_mean(loc)]
    return GraphMeasures([0, n], **{name: None if out[name] is None else np.asarray(out[name], dtype=_DTYPES[name])
                                    for name in NODE_FIELDS + GRAPH_FIELDS})
