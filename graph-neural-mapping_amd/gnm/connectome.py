"""Connectome graphs from functional-connectivity matrices, built on the device.

Replaces the graph loop of the reference's loader (util.py:20-122 load_data, dataset.py:93-101
DataEdges.get_adjacency) for a whole [S, n, n] stack of FC matrices:

    graphs = graphs_from_connectivity(model_or_arena, fc, sparsity, node_features, labels)

Per subject s, exactly what load_data produces:
  * threshold  thr_s = np.percentile(fc[s], 100 - sparsity) over the whole matrix, diagonal included (dataset.py:94),
               bitwise as numpy 2.x's "linear" method computes it (csrc/connectome.hip, gnm_connectome_thresholds);
  * edges      {u, v}, u < v, with fc[s, u, v] > thr_s: the upper triangle only (dataset.py:95-100);
  * order      networkx's, for the graph load_data builds node by node (util.py:43-103): see order_graph().
The graphs are registered in the arena as they come out of the device (GraphArena.add_connectivity); their edge_mat,
neighbors and node_features are materialized on the host on first access only.

From ROI time series instead of FC matrices (csrc/timeseries.hip; the contract is written out above
connectivity_from_timeseries):

    graphs = graphs_from_timeseries(model_or_arena, ts, sparsity, labels, node_features="mean_bold")

One graph per sliding window of the series (dynamic connectivity; the contract is written out above window_starts):

    graphs, windows = dynamic_graphs_from_timeseries(model_or_arena, ts, sparsity, labels, window, stride=1)

k-nearest-neighbour graphs instead of a percentile threshold (every node keeps at least k neighbours; the contract is
written out above knn_edges): the three builders and GraphArena.add_connectivity take sparsity=None with the keyword
arguments knn=k, mutual=False, absolute=False.  knn_edges is the rule in numpy on the host, knn_adjacency the adjacency
the device selects:

    graphs = graphs_from_connectivity(model_or_arena, fc, None, node_features, labels, knn=20)
    adj = knn_adjacency(fc, 20)                      # [S, n, n] bool, on the device

Connectivity states, k-means over the window FC matrices (gnm/states.py, re-exported here; csrc/dynstates.hip):

    st = connectivity_states_from_timeseries(ts, k, window, stride)      # centroids, labels, distances, counts, inertia
    stats = state_statistics(st.labels, st.windows, k)                   # occupancy, dwell, transitions per subject

Graph-theoretic measures of registered graphs (gnm/topology.py, re-exported here; csrc/topology.hip):

    m = graph_measures(model_or_arena, graphs)       # degree, clustering, path lengths, efficiencies, components

Hub measures of registered graphs (gnm/hubs.py, re-exported here; csrc/hubs.hip):

    h = hub_measures(model_or_arena, graphs, labels)     # betweenness; participation, within-module z, modularity
"""
import numbers

import numpy as np
import torch

from ._cabi import GnmError, check, lib


def _sparsity(sparsity):
    if isinstance(sparsity, (bool, np.bool_)) or not isinstance(sparsity, numbers.Real):
        raise ValueError("sparsity must be an int or float in [0, 100], got %r" % (sparsity,))
    s = int(sparsity) if isinstance(sparsity, numbers.Integral) else float(sparsity)
    if not 0 <= s <= 100:                     # NaN fails too
        raise ValueError("sparsity must be in [0, 100], got %r" % (sparsity,))
    return s


def _knn(knn):
    if isinstance(knn, (bool, np.bool_)) or not isinstance(knn, numbers.Integral):
        raise ValueError("knn must be an int >= 1, got %r" % (knn,))
    if int(knn) < 1:
        raise ValueError("knn must be >= 1, got %r" % (knn,))
    return int(knn)


def _edge_rule(sparsity, knn, mutual=False, absolute=False):
    """(sparsity, None, 0) for the percentile rule or (None, k, flags) for the kNN rule (flags: bit 0 mutual, bit 1
    absolute, as gnm_connectome_knn_structure takes them): exactly one of sparsity and knn is given"""
    if knn is None:
        if sparsity is None:
            raise ValueError("give sparsity (a percentile threshold) or knn (k nearest neighbours): got neither")
        if mutual or absolute:
            raise ValueError("mutual and absolute belong to the kNN rule: give knn, not sparsity")
        return _sparsity(sparsity), None, 0
    if sparsity is not None:
        raise ValueError("give sparsity or knn, not both: with knn=%r sparsity must be None, got %r" % (knn, sparsity))
    return None, _knn(knn), (1 if mutual else 0) | (2 if absolute else 0)


def percentile_indexes(N, sparsity):
    """(k_lo, k_hi, gamma) numpy's percentile(a, 100 - sparsity) of N values reads: order statistics k_lo and k_hi of
    the sorted values and the _lerp weight between them (numpy/lib/_function_base_impl.py _quantile, _get_indexes,
    _get_gamma; method "linear": virtual index (N - 1) q).  Past the last index both statistics are the maximum and
    gamma is numpy's virtual index - (-1)."""
    s = _sparsity(sparsity)
    N = int(N)
    if N < 1:
        raise ValueError("N must be positive")
    q = (100 - s) / 100                        # np.true_divide(100 - threshold, 100), float64
    vi = (N - 1) * q
    if vi >= N - 1:
        return N - 1, N - 1, vi - (-1.0)
    k = int(np.floor(vi))
    return k, k + 1, vi - float(k)


def _as_fc(fc, device):
    """[S, n, n] float64 contiguous tensor on the device (float32 is widened first)"""
    t = fc if torch.is_tensor(fc) else torch.from_numpy(np.asarray(fc))
    if t.dim() != 3 or t.shape[1] != t.shape[2]:
        raise ValueError("fc must be [S, n, n], got %s" % (tuple(t.shape),))
    if t.dtype not in (torch.float64, torch.float32):
        raise ValueError("fc must be float64 or float32, got %s" % t.dtype)
    n = int(t.shape[1])
    if n < 1 or n > int(lib.gnm_connectome_max_nodes()):
        raise ValueError("fc matrices of %d nodes: 1 <= n <= %d is supported (uint16 column ids)"
                         % (n, int(lib.gnm_connectome_max_nodes())))
    if device.type != "cuda":
        raise GnmError("connectome graphs are built on the GPU only (libgnm_hip.so); the device is %s" % device)
    return t.to(device=device, dtype=torch.float64).contiguous()


def _default_device(fc):
    if torch.is_tensor(fc) and fc.is_cuda:
        return fc.device
    return torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else torch.device("cpu")


def _thresholds_dev(fcd, sparsity):
    S, n = int(fcd.shape[0]), int(fcd.shape[1])
    k_lo, k_hi, gamma = percentile_indexes(n * n, sparsity)
    thr = torch.empty(S, dtype=torch.float64, device=fcd.device)
    with torch.cuda.device(fcd.device):
        st = torch.cuda.current_stream(fcd.device).cuda_stream
        check(lib.gnm_connectome_thresholds(fcd.data_ptr(), S, n, k_lo, k_hi, gamma, thr.data_ptr(), st),
              "gnm_connectome_thresholds")
    return thr


def connectivity_thresholds(fc, sparsity, device=None):
    """[S] float64 device tensor: np.percentile(fc[s], 100 - sparsity) per matrix, bitwise (NaN for a matrix holding a
    NaN).  fc: [S, n, n] float64 or float32 (widened first), numpy or torch, host or device."""
    _sparsity(sparsity)
    dev = torch.device(device) if device is not None else _default_device(fc)
    return _thresholds_dev(_as_fc(fc, dev), sparsity)


def order_graph(n, iu, ju):
    """The order load_data's networkx graph gives the undirected edges {iu[e], ju[e]} (iu < ju) of an n-node graph
    (util.py:43-103): nodes are inserted row by row, each row first adding itself, then its new upper neighbours in
    ascending id.  So with t(y) the first row i < y holding an edge {i, y} (y if none), the node order pi sorts by
    (t(y), y).  Returns (edge_mat [2, 2E] int64, neighbors: list of lists, max_neighbor):
      * edge_mat: for each u in pi order, (u, v) for every v later in pi, v ascending; then the same pairs reversed;
      * neighbors[x]: the neighbours earlier in pi, in pi order, then the later ones in ascending id."""
    iu = np.asarray(iu, dtype=np.int64).reshape(-1)
    ju = np.asarray(ju, dtype=np.int64).reshape(-1)
    t = np.arange(n, dtype=np.int64)
    np.minimum.at(t, ju, iu)
    pi = np.lexsort((np.arange(n), t))
    rank = np.empty(n, dtype=np.int64)
    rank[pi] = np.arange(n)
    first_is_u = rank[iu] < rank[ju]
    a = np.where(first_is_u, iu, ju)
    b = np.where(first_is_u, ju, iu)
    o = np.lexsort((b, rank[a]))
    a, b = a[o], b[o]
    edge_mat = np.stack([np.concatenate([a, b]), np.concatenate([b, a])])
    # neighbours: the earlier ends (key rank) before the later ends (key id), per node
    x = np.concatenate([b, a])
    y = np.concatenate([a, b])
    group = np.concatenate([np.zeros(a.shape[0], np.int64), np.ones(a.shape[0], np.int64)])
    key = np.where(group == 0, rank[y], y)
    o = np.lexsort((key, group, x))
    deg = np.bincount(x, minlength=n)
    neighbors = [r.tolist() for r in np.split(y[o], np.cumsum(deg)[:-1])] if n else []
    return edge_mat, neighbors, int(deg.max()) if n else 0


# ---------------------------------------------------------------------------------------------------- kNN rule
# The other edge rule of the builders (knn=k in place of sparsity): a k-nearest-neighbour graph, minimum degree >= k
# where a percentile of the whole matrix bounds no node's degree from below.  Of one matrix fc ([n, n], float64, or
# float32 widened first):
#   candidates  of row i: the columns v != i with fc[i, v] not NaN.  The row is read as stored: the matrix need not be
#               symmetric (np.corrcoef's is not, to the ulp);
#   key         fc[i, v], or |fc[i, v]| with absolute=True;
#   order       descending key, ascending column among equal keys; +0.0 and -0.0 are equal, +-inf ordinary values;
#   selection   row i selects its first min(k, number of candidates) candidates in that order;
#   edge        {u, v}, u < v: u selects v or v selects u (mutual=False), both select each other (mutual=True);
#   graph       node order, edge_mat, neighbors, max_neighbor and arena rows exactly what the percentile path gives for
#               the same upper-triangle edge set: order_graph(n, iu, ju) and the rows GraphArena.add builds from it;
#               iso and nnz as there.  An all-NaN row gives an isolated node, not an error.
# The device (csrc/connectome.hip, gnm_connectome_knn_structure) selects exactly, with no float arithmetic and no float
# atomics: a graph's bits do not depend on the matrices it shares a call with, and two runs give the same bits.

def knn_edges(fc, k, mutual=False, absolute=False):
    """(iu, ju), iu < ju: the upper-triangle edges of the kNN graph of one [n, n] matrix, by the contract above, in
    numpy on the host: the oracle gnm_connectome_knn_structure is tested against."""
    k = _knn(k)
    fc = np.asarray(fc, dtype=np.float64)
    if fc.ndim != 2 or fc.shape[0] != fc.shape[1]:
        raise ValueError("fc must be [n, n], got %s" % (fc.shape,))
    n = fc.shape[0]
    key = (np.abs(fc) if absolute else fc) + 0.0             # -0.0 + 0.0 = +0.0: one key for both zeros
    key[np.arange(n), np.arange(n)] = np.nan                 # not a candidate, like a NaN
    # per row: the candidates by descending key, equal keys by ascending column (stable); NaN sorts last
    order = np.argsort(-key, axis=1, kind="stable")[:, :k]
    taken = np.arange(order.shape[1])[None, :] < (~np.isnan(key)).sum(1)[:, None]
    sel = np.zeros((n, n), dtype=bool)
    sel[np.repeat(np.arange(n), taken.sum(1)), order[taken]] = True
    A = (sel & sel.T) if mutual else (sel | sel.T)
    return np.nonzero(np.triu(A, 1))


def knn_adjacency(fc, k, mutual=False, absolute=False, device=None):
    """[S, n, n] bool device tensor: the symmetric adjacency the builders use for knn=k, unpacked from the bit rows
    gnm_connectome_knn_structure leaves in its workspace.  For inspection, and for testing the select apart from the
    emission.  fc: [S, n, n] float64 or float32 (widened first), numpy or torch, host or device."""
    _, k, flags = _edge_rule(None, k, mutual, absolute)
    dev = torch.device(device) if device is not None else _default_device(fc)
    fcd = _as_fc(fc, dev)
    S, n = int(fcd.shape[0]), int(fcd.shape[1])
    if S == 0:
        return torch.zeros((0, n, n), dtype=torch.bool, device=dev)
    per, W = int(lib.gnm_connectome_workspace_words(1, n)), (n + 31) // 32
    work = torch.empty(S * per, dtype=torch.int32, device=dev)
    sel = torch.empty(int(lib.gnm_connectome_knn_scratch_words(S, n)), dtype=torch.int32, device=dev)
    nnz = torch.empty(S, dtype=torch.int32, device=dev)
    iso = torch.empty(S, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        st = torch.cuda.current_stream(dev).cuda_stream
        check(lib.gnm_connectome_knn_structure(fcd.data_ptr(), S, n, k, flags, sel.data_ptr(), work.data_ptr(),
                                               nnz.data_ptr(), iso.data_ptr(), st), "gnm_connectome_knn_structure")
    rows = work.view(S, per)[:, :n * W].reshape(S, n, W, 1)
    shifts = torch.arange(32, dtype=torch.int32, device=dev)
    up = ((rows >> shifts) & 1).reshape(S, n, W * 32)[:, :, :n].bool()       # bit v of row u: the edge {u < v}
    return up | up.transpose(1, 2)


class ConnectomeGraph:
    """S2VGraph-shaped (util.py:9-17) graph registered in a GraphArena by add_connectivity.  g, label and node_tags are
    plain; edge_mat, neighbors, max_neighbor and node_features are read back from the device on first access (and
    may be assigned, as on an S2VGraph)."""

    __slots__ = ("g", "label", "node_tags", "_gnm_cache", "_gnm_maxnb", "_arena", "_gid", "_edge_mat", "_neighbors",
                 "_max_neighbor", "_node_features")

    def __init__(self, arena, gid, n, label):
        self.g = range(n)                       # only len(graph.g) is read
        self.label = int(label)
        self.node_tags = None
        self._arena, self._gid = arena, gid
        self._gnm_cache = (arena._token, gid)
        self._gnm_maxnb = None
        self._edge_mat = self._neighbors = self._max_neighbor = self._node_features = None

    def _structure(self):
        ar, gid, n = self._arena, self._gid, len(self.g)
        rp0, c0, E = ar.rp_off[gid], ar.col_off[gid], ar.nnz[gid]
        rowptr = ar.rowptr.buf[rp0:rp0 + n + 1].cpu().numpy().astype(np.int64)
        col = ar.col.buf[c0:c0 + E].cpu().numpy().view(np.uint16).astype(np.int64)
        src = np.repeat(np.arange(n, dtype=np.int64), np.diff(rowptr))
        up = src < col
        em, nb, mx = order_graph(n, src[up], col[up])
        if self._edge_mat is None:
            self._edge_mat = torch.from_numpy(em)
        if self._neighbors is None:
            self._neighbors = nb
        if self._max_neighbor is None:
            self._max_neighbor = mx

    @property
    def edge_mat(self):
        if self._edge_mat is None:
            self._structure()
        return self._edge_mat

    @edge_mat.setter
    def edge_mat(self, v):
        self._edge_mat = v

    @property
    def neighbors(self):
        if self._neighbors is None:
            self._structure()
        return self._neighbors

    @neighbors.setter
    def neighbors(self, v):
        self._neighbors = v

    @property
    def max_neighbor(self):
        if self._max_neighbor is None:
            self._structure()
        return self._max_neighbor

    @max_neighbor.setter
    def max_neighbor(self, v):
        self._max_neighbor = v

    @property
    def node_features(self):
        if self._node_features is None:
            ar, r0 = self._arena, self._arena.feat_off[self._gid]
            self._node_features = ar.feat.buf[r0:r0 + len(self.g)].cpu().clone()
        return self._node_features

    @node_features.setter
    def node_features(self, v):
        self._node_features = v


def graphs_from_connectivity(model_or_arena, fc, sparsity, node_features, labels, *, knn=None, mutual=False,
                             absolute=False):
    """S graphs of load_data's shape from an [S, n, n] FC stack (util.py:20-122 for one --sparsity value), registered
    in the arena (a model means model.arena()).  node_features: [n, F] shared by every subject, or [S, n, F];
    labels: S ints.  Returns a list of ConnectomeGraph, usable wherever S2VGraph objects are.
    knn=k with sparsity None: k-nearest-neighbour graphs (the contract above knn_edges; mutual, absolute) instead of
    the percentile threshold."""
    arena = model_or_arena.arena() if hasattr(model_or_arena, "arena") and callable(model_or_arena.arena) \
        else model_or_arena
    _edge_rule(sparsity, knn, mutual, absolute)
    S = int(fc.shape[0]) if hasattr(fc, "shape") else len(fc)
    labels = [int(x) for x in (labels.tolist() if hasattr(labels, "tolist") else labels)]
    if len(labels) != S:
        raise ValueError("labels: %d values for %d matrices" % (len(labels), S))
    gids = arena.add_connectivity(fc, sparsity, node_features, knn=knn, mutual=mutual, absolute=absolute)
    n = int(fc.shape[1])
    return [ConnectomeGraph(arena, gid, n, lab) for gid, lab in zip(gids, labels)]


# ---------------------------------------------------------------------------------------------------- time series
# The FC matrices load_data thresholds (dataset.py:90-91) are Pearson correlations of the ROI time series the loader
# reads for mean_bold (dataset.py:45-46).  csrc/timeseries.hip computes, per subject, what numpy 2.x's
# np.corrcoef(ts[s], rowvar=False) does, in numpy's order:
#   1. Xc = X - mean(X, 0)                      (two passes: the data are centred as they are staged, never
#                                                X^T X - T m m^T, which loses the digits of a large offset)
#   2. C = (Xc^T Xc) * (1 / (T - 1))           (a multiply by the reciprocal; T = 1 gives 1 / 0 = inf, C all NaN)
#   3. s_i = sqrt(C_ii)
#   4. R_ij = (C_ij / s_i) / s_j              for every (i, j), from the one C_ij of the pair (C is symmetric; R is
#                                                not, to the ulp)
#   5. np.clip(R, -1, 1), NaN kept             (n = 1: numpy returns c / c unclipped)
# The Gram runs on fp64 matrix cores with a fixed summation order, so it is not numpy's BLAS order: |R - numpy| is
# within 1e-12, not bitwise.  The column means are numpy's pairwise sums over time divided by T: bitwise what np.mean
# gives for the loader's column-major (pandas) array; a row-major array's np.mean sums sequentially and differs from
# it by rounding.  mean_bold (dataset.py:73-74, util.py:118-121) is z = (m - m.mean()) / (m.std() + 1e-8) of those
# means with numpy's pairwise sums over the ROIs, in fp64, then rounded to fp32.
# Every kernel runs a subject inside one workgroup (no atomics, no split of T), so a subject's FC and features are
# bitwise the same alone, inside a stack or inside a ragged list.

def _as_tensor(a):
    return a if torch.is_tensor(a) else torch.from_numpy(np.asarray(a))


def _check_nodes(n):
    nmax = int(lib.gnm_timeseries_max_nodes())
    if n < 1 or n > nmax:
        raise ValueError("time series of %d ROIs: 1 <= n <= %d is supported" % (n, nmax))


def pack_timeseries(ts):
    """A list of [T_s, n] arrays (numpy or torch) packed into one [sum T, n] tensor, row after row, plus the int64 row
    offsets t_off [S + 1] (numpy) of each subject.  The packed dtype is float64 if any array is float64, else float32
    (widening is exact).  Arrays on the host are packed on the host; if any is on a GPU, all are packed there."""
    parts = [_as_tensor(a) for a in ts]
    if not parts:
        raise ValueError("ts: an empty list of time series")
    n = None
    for k, p in enumerate(parts):
        if p.dim() != 2:
            raise ValueError("ts[%d] must be [T, n], got %s" % (k, tuple(p.shape)))
        if p.dtype not in (torch.float64, torch.float32):
            raise ValueError("ts[%d] must be float64 or float32, got %s" % (k, p.dtype))
        if int(p.shape[0]) < 1:
            raise ValueError("ts[%d] has no time points" % k)
        if n is None:
            n = int(p.shape[1])
        elif int(p.shape[1]) != n:
            raise ValueError("ts[%d] has %d ROIs, ts[0] has %d" % (k, int(p.shape[1]), n))
    _check_nodes(n)
    dtype = torch.float64 if any(p.dtype == torch.float64 for p in parts) else torch.float32
    t_off = np.concatenate([[0], np.cumsum([int(p.shape[0]) for p in parts])]).astype(np.int64)
    on_gpu = [p.device for p in parts if p.is_cuda]
    if on_gpu:
        packed = torch.cat([p.to(device=on_gpu[0], dtype=dtype) for p in parts])
    else:
        npd = np.float64 if dtype == torch.float64 else np.float32
        packed = torch.from_numpy(np.concatenate([p.numpy().astype(npd, copy=False) for p in parts]))
    return packed, t_off


def _ts_device(ts):
    if torch.is_tensor(ts) and ts.is_cuda:
        return ts.device
    if isinstance(ts, (list, tuple)):
        for a in ts:
            if torch.is_tensor(a) and a.is_cuda:
                return a.device
    return torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else torch.device("cpu")


def _timeseries(ts):
    """(x [sum T, n] float32 / float64 tensor, t_off [S + 1] int64 numpy, S, n) from an [S, T, n] array or a list of
    [T_s, n] arrays, every shape and dtype checked; nothing is copied to a device yet."""
    if isinstance(ts, (list, tuple)):
        x, t_off = pack_timeseries(ts)
        S, n = len(t_off) - 1, int(x.shape[1])
    else:
        t = _as_tensor(ts)
        if t.dim() != 3:
            raise ValueError("ts must be [S, T, n] or a list of [T, n] arrays, got shape %s" % (tuple(t.shape),))
        if t.dtype not in (torch.float64, torch.float32):
            raise ValueError("ts must be float64 or float32, got %s" % t.dtype)
        S, T, n = (int(d) for d in t.shape)
        if T < 1:
            raise ValueError("ts has no time points (T = 0)")
        _check_nodes(n)
        x, t_off = t.reshape(S * T, n), np.arange(S + 1, dtype=np.int64) * T
    return x, t_off, S, n


def _to_device(x, t_off, device):
    if device.type != "cuda":
        raise GnmError("time series are reduced on the GPU only (libgnm_hip.so); the device is %s" % device)
    return x.to(device).contiguous(), torch.from_numpy(t_off).to(device)


def _as_timeseries(ts, device):
    """(x [sum T, n] contiguous on the device, t_off [S + 1] int64 on the device, S, n): _timeseries, then the copy"""
    x, t_off, S, n = _timeseries(ts)
    x, t_off = _to_device(x, t_off, device)
    return x, t_off, S, n


def _ts_means(x, t_off, S, n):
    mean = torch.empty((S, n), dtype=torch.float64, device=x.device)
    with torch.cuda.device(x.device):
        st = torch.cuda.current_stream(x.device).cuda_stream
        check(lib.gnm_timeseries_means(x.data_ptr(), int(x.dtype == torch.float64), t_off.data_ptr(), S, n,
                                       mean.data_ptr(), st), "gnm_timeseries_means")
    return mean


def _ts_fc(x, t_off, mean, S, n):
    fc = torch.empty((S, n, n), dtype=torch.float64, device=x.device)
    diag = torch.empty((S, n), dtype=torch.float64, device=x.device)
    with torch.cuda.device(x.device):
        st = torch.cuda.current_stream(x.device).cuda_stream
        check(lib.gnm_timeseries_gram(x.data_ptr(), int(x.dtype == torch.float64), t_off.data_ptr(), mean.data_ptr(),
                                      S, n, fc.data_ptr(), diag.data_ptr(), st), "gnm_timeseries_gram")
        check(lib.gnm_timeseries_normalize(diag.data_ptr(), S, n, fc.data_ptr(), st), "gnm_timeseries_normalize")
    return fc


def _ts_zscores(mean, S, n, dtype):
    z = torch.empty((S, n), dtype=dtype, device=mean.device)
    f64 = dtype == torch.float64
    with torch.cuda.device(mean.device):
        st = torch.cuda.current_stream(mean.device).cuda_stream
        check(lib.gnm_timeseries_zscores(mean.data_ptr(), S, n, z.data_ptr() if f64 else None,
                                         None if f64 else z.data_ptr(), st), "gnm_timeseries_zscores")
    return z.unsqueeze(-1)


def connectivity_from_timeseries(ts, device=None):
    """[S, n, n] float64 device tensor: np.corrcoef(ts[s], rowvar=False) per subject, within 1e-12 elementwise, with
    numpy's NaN pattern (a constant or non-finite ROI gives a NaN row and column, T = 1 an all-NaN matrix) and values
    in [-1, 1] otherwise.  ts: [S, T, n] or a list of [T_s, n] arrays (time in rows, ROIs in columns), float64 or
    float32 (widened on the device, as np.cov computes in float64), numpy or torch, host or device."""
    dev = torch.device(device) if device is not None else _ts_device(ts)
    x, t_off, S, n = _as_timeseries(ts, dev)
    return _ts_fc(x, t_off, _ts_means(x, t_off, S, n), S, n)


def mean_bold_features(ts, device=None, dtype=torch.float32):
    """[S, n, 1] device tensor: the reference loader's mean_bold node features (dataset.py:73-74, util.py:118-121),
    m = ts[s].mean(0), z = (m - m.mean()) / (m.std() + 1e-8) in float64, then rounded to float32.  dtype=torch.float64
    returns the float64 z-scores.  ts as in connectivity_from_timeseries."""
    if dtype not in (torch.float32, torch.float64):
        raise ValueError("dtype must be torch.float32 or torch.float64, got %s" % (dtype,))
    dev = torch.device(device) if device is not None else _ts_device(ts)
    x, t_off, S, n = _as_timeseries(ts, dev)
    return _ts_zscores(_ts_means(x, t_off, S, n), S, n, dtype)


def graphs_from_timeseries(model_or_arena, ts, sparsity, labels, node_features="mean_bold", *, knn=None, mutual=False,
                           absolute=False):
    """S graphs of load_data's shape from ROI time series: the FC of connectivity_from_timeseries, kept on the device
    and passed straight to graphs_from_connectivity's builder (GraphArena.add_connectivity).  node_features:
    "mean_bold" (the loader's [n, 1] features of each subject, mean_bold_features) or an array as
    graphs_from_connectivity takes it ([n, F] or [S, n, F]); labels: S ints.  knn, mutual, absolute: the kNN rule in
    place of sparsity, as graphs_from_connectivity takes them."""
    arena = model_or_arena.arena() if hasattr(model_or_arena, "arena") and callable(model_or_arena.arena) \
        else model_or_arena
    _edge_rule(sparsity, knn, mutual, absolute)
    if isinstance(node_features, str) and node_features != "mean_bold":
        raise ValueError("node_features must be \"mean_bold\" or an array, got %r" % (node_features,))
    labels = [int(x) for x in (labels.tolist() if hasattr(labels, "tolist") else labels)]
    x, t_off, S, n = _timeseries(ts)
    if len(labels) != S:
        raise ValueError("labels: %d values for %d subjects" % (len(labels), S))
    x, t_off = _to_device(x, t_off, arena.device)
    mean = _ts_means(x, t_off, S, n)
    fc = _ts_fc(x, t_off, mean, S, n)
    feats = _ts_zscores(mean, S, n, torch.float32) if isinstance(node_features, str) else node_features
    gids = arena.add_connectivity(fc, sparsity, feats, knn=knn, mutual=mutual, absolute=absolute)
    return [ConnectomeGraph(arena, gid, n, lab) for gid, lab in zip(gids, labels)]


# ---------------------------------------------------------------------------------------------------- sliding windows
# Dynamic functional connectivity: one correlation matrix per sliding window of the same series, rectangular
# (np.corrcoef of the window's rows) or tapered (np.cov(rows, aweights=taper), normalised as np.corrcoef does).  The
# windows are described to the device (first row and one common length), never sliced out or copied, and
# gnm_dynfc_corr (csrc/timeseries.hip) writes each finished R once.  A window's FC and features are bitwise the same
# whichever call, stride, stack or list it is part of.

# most bytes of window FC dynamic_graphs_from_timeseries holds at a time (one chunk; the buffer is reused)
DYNFC_WORK_BYTES = 1 << 30


def _window_args(window, stride):
    if isinstance(window, (bool, np.bool_)) or not isinstance(window, numbers.Integral):
        raise ValueError("window must be an int >= 2, got %r" % (window,))
    if isinstance(stride, (bool, np.bool_)) or not isinstance(stride, numbers.Integral):
        raise ValueError("stride must be an int >= 1, got %r" % (stride,))
    window, stride = int(window), int(stride)
    if window < 2:
        raise ValueError("window must be >= 2 (a correlation needs two rows), got %d" % window)
    if stride < 1:
        raise ValueError("stride must be >= 1, got %d" % stride)
    return window, stride


def window_starts(T, window, stride):
    """First rows of the sliding windows of a T-row series: np.arange(0, T - window + 1, stride) as int64.  Trailing
    rows that do not fill a window are dropped."""
    window, stride = _window_args(window, stride)
    T = int(T)
    if T < window:
        raise ValueError("a series of %d time points is shorter than the window (%d)" % (T, window))
    return np.arange(0, T - window + 1, stride, dtype=np.int64)


def _taper_arg(taper, window):
    """None, or the taper as a float64 numpy array [window]: finite, non-negative, at least two positive weights (with
    one, np.cov's normalisation sum w - sum w^2 / sum w is zero)"""
    if taper is None:
        return None
    w = taper.detach().cpu().numpy() if torch.is_tensor(taper) else np.asarray(taper)
    if w.ndim != 1 or w.shape[0] != window:
        raise ValueError("taper must be 1-D with window = %d weights, got shape %s" % (window, tuple(w.shape)))
    if w.dtype.kind not in "fiu":
        raise ValueError("taper must be real numbers, got dtype %s" % w.dtype)
    w = np.ascontiguousarray(w, dtype=np.float64)
    if not np.isfinite(w).all() or (w < 0).any():
        raise ValueError("taper weights must be finite and non-negative")
    if int((w > 0).sum()) < 2:
        raise ValueError("taper needs at least two positive weights")
    return w


def _plan_windows(t_off, window, stride):
    """(w_beg [sum W] int64: first row of each window in the packed series, windows [sum W, 3] int64: (subject, window
    index, first row within the subject), counts [S]): subject-major, window-minor"""
    begs, rows = [], []
    for s in range(len(t_off) - 1):
        T = int(t_off[s + 1] - t_off[s])
        if T < window:
            raise ValueError("ts[%d] has %d time points, fewer than the window (%d)" % (s, T, window))
        st = window_starts(T, window, stride)
        begs.append(t_off[s] + st)
        rows.append(np.stack([np.full(st.shape[0], s, np.int64), np.arange(st.shape[0], dtype=np.int64), st], 1))
    counts = np.array([b.shape[0] for b in begs], dtype=np.int64)
    return np.concatenate(begs).astype(np.int64), np.concatenate(rows), counts


def _plan_chunks(total, n, budget):
    """[(lo, hi)] covering windows 0 .. total once and in order, each chunk's [hi - lo, n, n] float64 FC within
    `budget` bytes (one window per chunk where a single matrix is larger)"""
    per = max(1, int(budget) // (8 * n * n))
    return [(lo, min(total, lo + per)) for lo in range(0, total, per)]


def _dyn_means(x, w_beg, window, n):
    W = int(w_beg.shape[0])
    mean = torch.empty((W, n), dtype=torch.float64, device=x.device)
    with torch.cuda.device(x.device):
        st = torch.cuda.current_stream(x.device).cuda_stream
        check(lib.gnm_dynfc_means(x.data_ptr(), int(x.dtype == torch.float64), w_beg.data_ptr(), window, W, n,
                                  mean.data_ptr(), st), "gnm_dynfc_means")
    return mean


def _dyn_corr(x, w_beg, window, mean, taper, n, out):
    """out[w] = R of window w for every window of w_beg; one launch, split where the grid would pass the launch limit"""
    W = int(w_beg.shape[0])
    step = int(lib.gnm_dynfc_max_windows(n))
    with torch.cuda.device(x.device):
        st = torch.cuda.current_stream(x.device).cuda_stream
        for lo in range(0, W, step):
            m = min(W, lo + step) - lo
            check(lib.gnm_dynfc_corr(x.data_ptr(), int(x.dtype == torch.float64), w_beg[lo:].data_ptr(), window,
                                     None if mean is None else mean[lo:].data_ptr(),
                                     None if taper is None else taper.data_ptr(), m, n, out[lo:].data_ptr(), st),
                  "gnm_dynfc_corr")
    return out


def dynamic_connectivity_from_timeseries(ts, window, stride=1, taper=None, device=None):
    """One FC matrix per sliding window (first rows window_starts(T_s, window, stride)), float64 on the device:
    [S, W, n, n] for an [S, T, n] stack, a list of [W_s, n, n] views of one buffer for a list of [T_s, n] arrays.
    taper None: np.corrcoef(rows, rowvar=False) of each window; taper [window] (finite, non-negative, two positive
    weights at least): np.cov(rows, rowvar=False, aweights=taper) normalised by its diagonal and clipped, as np.corrcoef
    does.  Within 1e-12 elementwise of numpy with its NaN pattern.  ts as in connectivity_from_timeseries."""
    window, stride = _window_args(window, stride)
    w = _taper_arg(taper, window)
    x, t_off, S, n = _timeseries(ts)
    w_beg, _, counts = _plan_windows(t_off, window, stride)
    dev = torch.device(device) if device is not None else _ts_device(ts)
    x, _ = _to_device(x, t_off, dev)
    w_beg = torch.from_numpy(w_beg).to(dev)
    W = int(w_beg.shape[0])
    fc = torch.empty((W, n, n), dtype=torch.float64, device=dev)
    mean = _dyn_means(x, w_beg, window, n) if w is None else None
    _dyn_corr(x, w_beg, window, mean, None if w is None else torch.from_numpy(w).to(dev), n, fc)
    if isinstance(ts, (list, tuple)):
        return list(torch.split(fc, counts.tolist()))
    return fc.view(S, W // S, n, n)


def dynamic_graphs_from_timeseries(model_or_arena, ts, sparsity, labels, window, stride=1, taper=None,
                                   node_features="mean_bold", *, knn=None, mutual=False, absolute=False):
    """(graphs, windows): one graph of load_data's shape per sliding window, registered in the arena.  graphs is a flat
    list of ConnectomeGraph, subject-major and window-minor, each with its subject's label; windows [sum W, 3] int64 holds
    (subject, window index, first row within the subject) of each.  node_features: "mean_bold" (the z-scores of the
    plain window means, whatever the taper) or an array: [n, F] for every window, or [S, n, F] per subject.  The FC never
    exists whole: windows go through means, z-scores, the fused correlation and GraphArena.add_connectivity in chunks of
    at most DYNFC_WORK_BYTES of FC, in one buffer that is reused.  knn, mutual, absolute: the kNN rule in place of
    sparsity, as graphs_from_connectivity takes them: every window's graph then has minimum degree >= k."""
    arena = model_or_arena.arena() if hasattr(model_or_arena, "arena") and callable(model_or_arena.arena) \
        else model_or_arena
    _edge_rule(sparsity, knn, mutual, absolute)
    window, stride = _window_args(window, stride)
    w = _taper_arg(taper, window)
    mean_bold = isinstance(node_features, str)
    if mean_bold and node_features != "mean_bold":
        raise ValueError("node_features must be \"mean_bold\" or an array, got %r" % (node_features,))
    labels = [int(v) for v in (labels.tolist() if hasattr(labels, "tolist") else labels)]
    x, t_off, S, n = _timeseries(ts)
    if len(labels) != S:
        raise ValueError("labels: %d values for %d subjects" % (len(labels), S))
    w_beg_h, windows, _ = _plan_windows(t_off, window, stride)
    per_subject = None
    if not mean_bold:
        ft = node_features if torch.is_tensor(node_features) else torch.as_tensor(np.asarray(node_features))
        if ft.dim() == 3:
            if int(ft.shape[0]) != S:
                raise ValueError("node_features [S, n, F]: %d subjects for %d series" % (int(ft.shape[0]), S))
            per_subject = ft
    dev = arena.device
    x, _ = _to_device(x, t_off, dev)
    w_beg = torch.from_numpy(w_beg_h).to(dev)
    subj = torch.from_numpy(windows[:, 0].copy()).to(dev)
    if per_subject is not None:
        per_subject = per_subject.to(device=dev, dtype=torch.float32)
    wd = None if w is None else torch.from_numpy(w).to(dev)
    total = int(w_beg.shape[0])
    chunks = _plan_chunks(total, n, DYNFC_WORK_BYTES)
    fc = torch.empty((max(hi - lo for lo, hi in chunks), n, n), dtype=torch.float64, device=dev)
    gids = []
    for lo, hi in chunks:
        m = hi - lo
        mean = _dyn_means(x, w_beg[lo:hi], window, n) if (w is None or mean_bold) else None
        if mean_bold:
            feats = _ts_zscores(mean, m, n, torch.float32)
        else:
            feats = node_features if per_subject is None else per_subject[subj[lo:hi]]
        _dyn_corr(x, w_beg[lo:hi], window, mean if w is None else None, wd, n, fc[:m])
        gids += arena.add_connectivity(fc[:m], sparsity, feats, knn=knn, mutual=mutual, absolute=absolute)
    graphs = [ConnectomeGraph(arena, gid, n, labels[s]) for gid, s in zip(gids, windows[:, 0].tolist())]
    return graphs, windows


# ---------------------------------------------------------------------------------------------------- states
# k-means over the window FC matrices (gnm/states.py, csrc/dynstates.hip), re-exported here; states.py imports this
# module for the window plan and the sliding-window kernels, so the names are looked up on first use
_STATES = ("ConnectivityStates", "StateStatistics", "connectivity_states", "connectivity_states_from_timeseries",
           "assign_states", "state_statistics", "kmeanspp_draw")


# graph-theoretic measures of the registered graphs (gnm/topology.py, csrc/topology.hip), re-exported the same way
_TOPOLOGY = ("GraphMeasures", "graph_measures", "graph_measures_host")
# betweenness and the module-aware hub measures (gnm/hubs.py, csrc/hubs.hip)
_HUBS = ("HubMeasures", "hub_measures", "hub_measures_host")


def __getattr__(name):
    if name in _STATES:
        from . import states
        return getattr(states, name)
    if name in _TOPOLOGY:
        from . import topology
        return getattr(topology, name)
    if name in _HUBS:
        from . import hubs
        return getattr(hubs, name)
    raise AttributeError("module %r has no attribute %r" % (__name__, name))
