"""Host side of GIN_InfoMaxReg.lesion() / deletion_curve(): the removed-node sets of a deletion curve from a per-ROI
ranking, and the curve's area; and of disconnect() / disconnection_matrix(): the set pairs of a network labelling and
the number of edges a cut removes.  numpy only; nothing here touches the device."""
import numpy as np

ORDERS = ("descending", "ascending")


def default_fractions():
    """0, 0.05, ..., 0.95: the default deletion fractions"""
    return np.arange(20, dtype=np.float64) / 20.0


def _per_graph(ranking):
    """ranking ([G, n] array or a list of per-graph [n_g]) as a list of 1-D float64 arrays"""
    if isinstance(ranking, np.ndarray) and ranking.ndim == 2:
        rows = list(ranking)
    elif isinstance(ranking, np.ndarray):
        raise ValueError("ranking must be [G, n] or a list of per-graph [n_g] arrays, got shape %s" % list(ranking.shape))
    else:
        rows = list(ranking)
    out = []
    for g, r in enumerate(rows):
        if hasattr(r, "detach"):
            r = r.detach().cpu().numpy()
        r = np.asarray(r, dtype=np.float64)
        if r.ndim != 1 or r.shape[0] < 1:
            raise ValueError("ranking of graph %d must be a non-empty vector, got shape %s" % (g, list(r.shape)))
        if not np.isfinite(r).all():
            raise ValueError("ranking of graph %d has a non-finite entry" % g)
        out.append(r)
    return out


def masks_from_ranking(ranking, fractions, order="descending"):
    """The removed sets of a deletion curve.  ranking: a [G, n] array or a list of per-graph [n_g] scores (any per-ROI
    map); fractions: K numbers in [0, 1].  Per graph the nodes are sorted by score with a STABLE sort, ties to the lower
    index -- order "descending" removes the highest-ranked first, "ascending" the lowest first (read backwards: the
    insertion curve) -- and set k removes the first min(n - 1, floor(fractions[k] n)) nodes of that order.
    Returns (masks, counts): per graph a bool [K, n_g] array (True = removed) and an int64 [K] array of set sizes."""
    if order not in ORDERS:
        raise ValueError("order must be one of %s, not %r" % (ORDERS, order))
    fr = np.asarray(fractions, dtype=np.float64).reshape(-1)
    if not np.isfinite(fr).all() or (fr < 0).any() or (fr > 1).any():
        raise ValueError("fractions must lie in [0, 1]")
    masks, counts = [], []
    for r in _per_graph(ranking):
        n = r.shape[0]
        perm = np.argsort(-r if order == "descending" else r, kind="stable")
        cnt = np.minimum(n - 1, np.floor(fr * n).astype(np.int64))        # (the fp64 product, as written)
        pos = np.empty(n, dtype=np.int64)
        pos[perm] = np.arange(n)
        masks.append(pos[None, :] < cnt[:, None])
        counts.append(cnt)
    return masks, counts


def pair_sets(labels, K=None):
    """The set pairs of a network-by-network disconnection matrix.  labels: an int [n] vector, entry r the network id
    of node r in 0 .. K - 1, or -1 for a node of no network (it is in no set); K: the number of networks, default
    max(labels) + 1.  Returns (a, b, pairs): bool [S, n] arrays and an int64 [S, 2] array, S = K (K + 1) / 2, the
    unordered pairs (p, q), p <= q, in the order (0, 0), (0, 1), ..., (0, K - 1), (1, 1), ...; a[s] = network p,
    b[s] = network q.  Pair (p, p) is the cut inside network p."""
    lab = np.asarray(labels)
    if lab.ndim != 1 or lab.dtype.kind not in "iu":
        raise ValueError("labels must be an int [n] vector, got dtype %s shape %s" % (lab.dtype, list(lab.shape)))
    lab = lab.astype(np.int64)
    if lab.size and lab.min() < -1:
        raise ValueError("labels must be network ids >= 0, or -1 for no network")
    top = int(lab.max()) + 1 if lab.size else 0
    if K is None:
        K = top
    K = int(K)
    if K < top:
        raise ValueError("labels hold network %d but K = %d" % (top - 1, K))
    pairs = np.array([(p, q) for p in range(K) for q in range(p, K)], dtype=np.int64).reshape(-1, 2)
    member = lab[None, :] == np.arange(K, dtype=np.int64)[:, None]        # [K, n]; -1 matches none
    return member[pairs[:, 0]], member[pairs[:, 1]], pairs


def cut_edge_counts(edge_mat, a, b):
    """How many columns (u, v) of edge_mat [2, E] each cut removes: those with (a[s, u] and b[s, v]) or (b[s, u] and
    a[s, v]).  a, b: bool or 0/1 [S, n].  Returns an int64 [S] array -- the size a delta is to be read against (an
    undirected graph stored as both (u, v) and (v, u) counts both)."""
    a = np.asarray(a) != 0
    b = np.asarray(b) != 0
    if a.ndim != 2 or a.shape != b.shape:
        raise ValueError("a and b must be [S, n] arrays of one shape, got %s and %s" % (list(a.shape), list(b.shape)))
    em = edge_mat.detach().cpu().numpy() if hasattr(edge_mat, "detach") else np.asarray(edge_mat)
    em = em.astype(np.int64).reshape(2, -1)
    if em.size and (em.min() < 0 or em.max() >= a.shape[1]):
        raise ValueError("edge_mat names a node outside the %d-node masks" % a.shape[1])
    u, v = em
    return ((a[:, u] & b[:, v]) | (b[:, u] & a[:, v])).sum(1).astype(np.int64)


def curve_area(scores, realised_fractions):
    """The area under a deletion curve by the trapezoid rule in fp64 over the REALISED fractions count / n, divided by
    their span: the mean score along the curve.  scores: [..., K]; realised_fractions: [K] or broadcastable to scores.
    A curve of zero span (one point, or every point at one fraction) returns its first score.  K = 0 raises."""
    s = np.asarray(scores, dtype=np.float64)
    x = np.broadcast_to(np.asarray(realised_fractions, dtype=np.float64), s.shape)
    if s.shape[-1] == 0:
        raise ValueError("curve_area: an empty curve")
    span = x[..., -1] - x[..., 0]
    area = (0.5 * (s[..., 1:] + s[..., :-1]) * np.diff(x, axis=-1)).sum(-1)
    with np.errstate(all="ignore"):
        return np.where(span != 0, area / np.where(span != 0, span, 1.0), s[..., 0])
