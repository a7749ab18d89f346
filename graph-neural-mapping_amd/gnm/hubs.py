"""Hub measures of connectome graphs, on the device (csrc/hubs.hip).  Re-exported by gnm.connectome.

    h = hub_measures(model_or_arena, graphs, labels=None, betweenness=True)     # HubMeasures of device tensors
    o = hub_measures_host(adjacency_or_edge_list, n=None, labels=None)          # one graph, numpy: the oracle

The graphs are read as gnm.topology.graph_measures reads them: simple and undirected, a repeated edge counts once and
a self loop is dropped.

Betweenness is Brandes' algorithm with every order fixed.  For the sources s = 0, 1, .. in order, with breadth-first
levels from s:  sigma[s] = 1.0;  for w at level k, sigma[w] = ((0.0 + sigma[v1]) + sigma[v2]) + .. over the neighbours v
of w at level k - 1 in ascending v;  delta = 0 and, for k from the deepest level - 1 down to 1 and v at level k,
delta[v] = ((0.0 + t(w1)) + t(w2)) + .. over the neighbours w of v at level k + 1 in ascending w, where
t(w) = (sigma[v] / sigma[w]) * (1.0 + delta[w]);  total[v] = total[v] + delta[v] for v != s.

  betweenness              total * 0.5: the sum over unordered pairs {s, t}, s != v != t, of sigma_st(v) / sigma_st
                           (networkx's betweenness_centrality(normalized=False))
  betweenness_normalized   betweenness / float((n - 1) * (n - 2) // 2), 0.0 for n < 3

With labels (an int vector, -1 for a node of no module, K = the largest label + 1 modules, at most 64; K = 1 when every
entry is -1), k_v,m the neighbours of v that carry label m:

  module_degree [N, K]     k_v,m
  participation            with d = sum_m k_v,m:  acc = 0.0;  for m ascending: r = float(k_v,m) / float(d);
                           acc = acc + r * r;  then 1.0 - acc  (0.0 for d = 0)
  within_module_z          for v with label m >= 0, over the s nodes u of module m, S1 = sum k_u,m, S2 = sum k_u,m ** 2:
                           float(k_v,m * s - S1) / sqrt(float(s * S2 - S1 ** 2)); 0.0 when the radicand is 0 or v has no
                           module (the population-std z-score of BCT's module_degree_zscore, integer up to the sqrt)
  module_edges [B, K, K]   edges between modules, symmetric, the edges inside a module on the diagonal
  modularity               Newman's Q of the labelling, with E the graph's edges, L_m = module_edges[m, m] and D_m the sum
                           of the full degrees of module m's nodes:  acc = 0.0;  for m ascending:
                           a = float(D_m) / float(2 * E);  acc = acc + (float(L_m) / float(E) - a * a);  0.0 for E = 0

sigma goes inexact above 2^53; both sides add in the same order, so the device's fields are bitwise
hub_measures_host's, whatever batch a graph is part of.
"""
import numpy as np
import torch

from ._cabi import GnmError, check, lib
from .shapley import check_labels
from .topology import _adjacency, _distances

BETWEENNESS_FIELDS = ("betweenness", "betweenness_normalized")
NODE_FIELDS = BETWEENNESS_FIELDS + ("module_degree", "participation", "within_module_z")
GRAPH_FIELDS = ("module_edges", "modularity")
MODULE_FIELDS = NODE_FIELDS[2:] + GRAPH_FIELDS
_DTYPES = {"betweenness": "float64", "betweenness_normalized": "float64", "module_degree": "int32",
           "participation": "float64", "within_module_z": "float64", "module_edges": "int64", "modularity": "float64"}


class HubMeasures:
    """The hub measures of B graphs.  NODE_FIELDS are [N] arrays in batch order (module_degree [N, K]; graph i owns rows
    node_off[i] .. node_off[i + 1]), modularity [B], module_edges [B, K, K]; device tensors from hub_measures, numpy
    arrays from hub_measures_host.  node_off is a host int64 array [B + 1].  The two betweenness fields are None when
    they were not asked for, the MODULE_FIELDS when no labels were given."""

    __slots__ = NODE_FIELDS + GRAPH_FIELDS + ("node_off",)

    def __init__(self, node_off, **fields):
        self.node_off = np.asarray(node_off, dtype=np.int64)
        for name in NODE_FIELDS + GRAPH_FIELDS:
            setattr(self, name, fields[name])

    def __len__(self):
        return int(self.node_off.shape[0]) - 1

    def __repr__(self):
        return "HubMeasures(graphs=%d, nodes=%d, betweenness=%s, modules=%s)" % (
            len(self), int(self.node_off[-1]), self.betweenness is not None,
            None if self.module_degree is None else int(self.module_degree.shape[1]))

    def graph(self, i):
        """the measures of graph i alone: views of its node rows and its entry of every per-graph array"""
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
        return HubMeasures([0, hi - lo], **out)

    def numpy(self):
        """the same record with every field a host numpy array"""
        conv = lambda a: None if a is None else (a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a))
        return HubMeasures(self.node_off, **{name: conv(getattr(self, name)) for name in NODE_FIELDS + GRAPH_FIELDS})


def _module_count(lab):
    """K = the largest label + 1 of a checked label vector, at most gnm_topology_max_modules() (ValueError above); a
    vector that names no module at all (empty, or -1 throughout) counts as one module without nodes, K = 1"""
    limit = int(lib.gnm_topology_max_modules())
    K = max(int(lab.max()) + 1, 1) if lab.size else 1
    if K > limit:
        raise ValueError("labels name %d modules; at most %d (gnm_topology_max_modules) are supported" % (K, limit))
    return K


def hub_measures(model_or_arena, graphs, labels=None, betweenness=True):
    """HubMeasures of `graphs` (anything GraphArena.batch takes, ragged node counts allowed), registered in the arena (a
    model means model.arena()) if they are not yet.  One launch for betweenness and one for the module measures, one
    workgroup per graph; betweenness=False skips the first and leaves its two fields None, labels=None the second and
    leaves MODULE_FIELDS None.  labels: an int [n] vector shared by all graphs (every graph then has n nodes) or one [N]
    vector in batch order; entries >= -1, -1 for a node of no module.
    ValueError for a graph that is not symmetric and for labels that do not fit; GnmError for a graph above
    gnm_topology_max_nodes() nodes and for an arena that is not on a GPU: all before anything is launched.  An empty
    list gives empty arrays."""
    arena = model_or_arena.arena() if hasattr(model_or_arena, "arena") and callable(model_or_arena.arena) \
        else model_or_arena
    graphs = list(graphs)
    dev = arena.device
    limit = int(lib.gnm_topology_max_nodes())
    lab = None if labels is None else check_labels(labels.detach().cpu().numpy() if torch.is_tensor(labels) else labels)

    def alloc(name, *shape):
        return torch.empty(shape, dtype=getattr(torch, _DTYPES[name]), device=dev)

    def fields(N, B, K):
        f = dict.fromkeys(NODE_FIELDS + GRAPH_FIELDS)
        if betweenness:
            f.update({name: alloc(name, N) for name in BETWEENNESS_FIELDS})
        if K is not None:
            f.update(module_degree=alloc("module_degree", N, K), participation=alloc("participation", N),
                     within_module_z=alloc("within_module_z", N), module_edges=alloc("module_edges", B, K, K),
                     modularity=alloc("modularity", B))
        return f

    if not graphs:
        return HubMeasures([0], **fields(0, 0, None if lab is None else _module_count(lab)))
    batch = arena.batch(graphs)
    if not batch.symmetric:
        bad = [i for i, g in enumerate(arena.add_many(graphs)) if not arena.sym[g]]
        raise ValueError("hub_measures: graphs %s are not symmetric; the measures are those of undirected graphs"
                         % bad[:8])
    B, N, n_max = batch.B, batch.N, max(batch.n_max, 1)
    K = None
    if lab is not None:
        sizes = np.diff(np.asarray(batch.node_off_host, dtype=np.int64))
        if (sizes == lab.shape[0]).all():
            lab = np.tile(lab, B)
        elif lab.shape[0] != N:
            raise ValueError("labels must be an [n] vector shared by graphs of n nodes each or an [N] = [%d] vector in "
                             "batch order; got %d labels for graphs of %s nodes" % (N, lab.shape[0], sizes[:8].tolist()))
        K = _module_count(lab)
    if batch.n_max > limit:
        raise GnmError("hub_measures: a graph of %d nodes; at most %d are supported (gnm_topology_max_nodes: the bit "
                       "rows of a graph stay in one CU's LDS)" % (batch.n_max, limit))
    if dev.type != "cuda":
        raise GnmError("hub measures are computed on the GPU only (libgnm_hip.so); the arena is on %s" % dev)
    f = fields(N, B, K)
    csr = batch.csr_ptrs()
    with torch.cuda.device(dev):
        st = torch.cuda.current_stream(dev).cuda_stream
        if betweenness:
            nbytes = int(lib.gnm_topology_betweenness_workspace_bytes(B, n_max))
            work = torch.empty(nbytes, dtype=torch.uint8, device=dev) if nbytes > 0 else None
            check(lib.gnm_topology_betweenness(*csr, batch.node_off.data_ptr(), B, n_max,
                                               None if work is None else work.data_ptr(), f["betweenness"].data_ptr(),
                                               f["betweenness_normalized"].data_ptr(), st), "gnm_topology_betweenness")
        if K is not None:
            lab_dev = torch.from_numpy(lab.astype(np.int32)).to(dev)
            check(lib.gnm_topology_modules(*csr, batch.node_off.data_ptr(), lab_dev.data_ptr(), B, n_max, K,
                                           f["module_degree"].data_ptr(), f["participation"].data_ptr(),
                                           f["within_module_z"].data_ptr(), f["module_edges"].data_ptr(),
                                           f["modularity"].data_ptr(), st), "gnm_topology_modules")
    return HubMeasures(batch.node_off_host, **f)


# ---------------------------------------------------------------------------------------------------- the numpy oracle
def _brandes_total(A):
    """[n] float64: sum over the sources s in ascending order of delta_s, the module docstring's recurrences.  All
    sources advance together level by level; inside a level the Python loop runs over the ascending predecessor (or
    successor) and numpy over every (source, node) pair it feeds, each pair at most once per step: elementwise the
    scalar recurrences, in their order."""
    n = A.shape[0]
    D = _distances(A)
    nbr = [np.flatnonzero(A[v]) for v in range(n)]
    sigma = np.zeros((n, n), dtype=np.float64)          # [source, node]
    sigma[np.arange(n), np.arange(n)] = 1.0
    delta = np.zeros((n, n), dtype=np.float64)
    depth = int(D.max()) if n else 0
    at = [D == k for k in range(depth + 1)]
    for k in range(1, depth + 1):
        for v in range(n):                              # the predecessor, ascending
            S = np.flatnonzero(at[k - 1][:, v])
            if S.size == 0 or nbr[v].size == 0:
                continue
            rows, cols = np.nonzero(at[k][np.ix_(S, nbr[v])])
            s, w = S[rows], nbr[v][cols]
            sigma[s, w] = sigma[s, w] + sigma[s, v]
    for k in range(depth - 1, 0, -1):
        for w in range(n):                              # the successor, ascending
            S = np.flatnonzero(at[k + 1][:, w])
            if S.size == 0 or nbr[w].size == 0:
                continue
            rows, cols = np.nonzero(at[k][np.ix_(S, nbr[w])])
            s, v = S[rows], nbr[w][cols]
            delta[s, v] = delta[s, v] + (sigma[s, v] / sigma[s, w]) * (1.0 + delta[s, w])
    total = np.zeros(n, dtype=np.float64)
    for s in range(n):                                  # delta[s, s] is 0.0
        total = total + delta[s]
    return total


def hub_measures_host(graph, n=None, labels=None):
    """The hub measures of ONE graph in plain numpy, a HubMeasures of numpy arrays (B = 1): the oracle the kernels are
    tested against, formulas and their order as the module's docstring states them.  graph: a bool [n, n] adjacency or
    an integer [E, 2] edge list with the node count n; made symmetric, repeated edges and self loops ignored.  labels:
    None (the MODULE_FIELDS are then None) or an int [n] vector, -1 for a node of no module."""
    A = _adjacency(graph, n)
    n = A.shape[0]
    bc = _brandes_total(A) * 0.5
    out = dict.fromkeys(NODE_FIELDS + GRAPH_FIELDS)
    out["betweenness"] = bc
    out["betweenness_normalized"] = bc / float((n - 1) * (n - 2) // 2) if n >= 3 else np.zeros(n, dtype=np.float64)
    if labels is not None:
        lab = check_labels(labels.detach().cpu().numpy() if torch.is_tensor(labels) else labels, n)
        K = _module_count(lab)
        Ai = A.astype(np.int64)
        member = lab[:, None] == np.arange(K, dtype=np.int64)[None, :]          # [n, K]
        kvm = Ai @ member.astype(np.int64)
        deg = Ai.sum(1)
        part = np.zeros(n, dtype=np.float64)
        z = np.zeros(n, dtype=np.float64)
        size = member.sum(0)
        S1 = [int(kvm[member[:, m], m].sum()) for m in range(K)]
        S2 = [int((kvm[member[:, m], m] ** 2).sum()) for m in range(K)]
        for v in range(n):
            d = int(kvm[v].sum())
            if d:
                acc = 0.0
                for m in range(K):
                    r = float(int(kvm[v, m])) / float(d)
                    acc = acc + r * r
                part[v] = 1.0 - acc
            m = int(lab[v])
            if m >= 0:
                s = int(size[m])
                rad = s * S2[m] - S1[m] * S1[m]
                if rad > 0:
                    z[v] = float(int(kvm[v, m]) * s - S1[m]) / float(np.sqrt(np.float64(rad)))
        pairs = member.astype(np.int64).T @ kvm                                # ordered pairs: the diagonal counts twice
        edges = pairs.copy()
        edges[np.arange(K), np.arange(K)] //= 2
        E = int(deg.sum()) // 2
        q = 0.0
        if E:
            for m in range(K):
                a = float(int(deg[member[:, m]].sum())) / float(2 * E)
                q = q + (float(int(edges[m, m])) / float(E) - a * a)
        out.update(module_degree=kvm, participation=part, within_module_z=z, module_edges=edges[None], modularity=[q])
    return HubMeasures([0, n], **{name: None if out[name] is None else np.asarray(out[name], dtype=_DTYPES[name])
                                  for name in NODE_FIELDS + GRAPH_FIELDS})
