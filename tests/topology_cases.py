"""Shared by the graph-measure tests (tests/test_topology_host.py, tests/test_gpu_topology.py): the graph kinds as [E, 2]
edge lists, closed-form answers of the structured kinds (written from the graphs' definitions, never through
gnm.topology), and the comparison helpers.  No tests here."""
import numpy as np

from knn_cases import bits_eq, fc_stack

STRUCTURED = ("empty", "complete", "path", "ring", "star", "two_cliques", "two_components_isolated")
RANDOM = ("er003", "er03", "sparsity30", "knn5")
KINDS = STRUCTURED + RANDOM

NODE_FIELDS = ("degree", "triangles", "clustering", "eccentricity", "reachable", "distance_sum", "component",
               "nodal_efficiency", "local_efficiency")
GRAPH_FIELDS = ("edges", "components", "distance_histogram", "diameter", "global_efficiency",
                "characteristic_path_length", "transitivity", "mean_clustering", "mean_local_efficiency")
LOCAL_FIELDS = ("local_efficiency", "mean_local_efficiency")
INT_FIELDS = ("degree", "triangles", "eccentricity", "reachable", "distance_sum", "component", "edges", "components",
              "distance_histogram", "diameter")


def _pairs(nodes):
    nodes = list(nodes)
    return [(a, b) for i, a in enumerate(nodes) for b in nodes[i + 1:]]


def _split(n):
    """two_components_isolated: a path on the first p nodes, a clique on the next q, the last node alone"""
    p = max((n - 1) // 2, 0)
    return p, n - 1 - p


def edges_of(kind, n, seed=0):
    """[E, 2] int64 undirected edges (u < v, each once) of an n-node graph of the kind"""
    if kind == "empty":
        e = []
    elif kind == "complete":
        e = _pairs(range(n))
    elif kind == "path":
        e = [(i, i + 1) for i in range(n - 1)]
    elif kind == "ring":                            # below four nodes the path (a 3-ring is the complete graph)
        e = [(i, i + 1) for i in range(n - 1)] + ([(0, n - 1)] if n >= 4 else [])
    elif kind == "star":
        e = [(0, i) for i in range(1, n)]
    elif kind == "two_cliques":                     # nodes 0 .. a - 1 and a .. n - 1, joined by {a - 1, a}
        a = n // 2
        e = _pairs(range(a)) + _pairs(range(a, n)) + ([(a - 1, a)] if a >= 1 else [])
    elif kind == "two_components_isolated":
        p, q = _split(n)
        e = [(i, i + 1) for i in range(p - 1)] + _pairs(range(p, p + q))
    elif kind in ("er003", "er03"):
        rng = np.random.default_rng(1000 * n + seed + (kind == "er03"))
        iu, ju = np.nonzero(np.triu(rng.random((n, n)) < (0.03 if kind == "er003" else 0.3), 1))
        e = np.stack([iu, ju], 1)
    elif kind == "sparsity30":                      # the percentile rule of the builders, dataset.py:93-101
        fc = fc_stack(1, n, 31 * n + seed)[0]
        iu, ju = np.nonzero(np.triu(fc > np.percentile(fc, 70), 1))
        e = np.stack([iu, ju], 1)
    elif kind in ("knn5", "knn20"):                 # mutual kNN at k = 5: often disconnected; the union rule at k = 20
        from gnm.connectome import knn_edges
        fc = fc_stack(1, n, 57 * n + seed)[0]
        iu, ju = knn_edges(fc, 5, mutual=True) if kind == "knn5" else knn_edges(fc, 20)
        e = np.stack([iu, ju], 1)
    else:
        raise ValueError(kind)
    e = np.asarray(e, dtype=np.int64).reshape(-1, 2)
    return np.stack([e.min(1), e.max(1)], 1) if e.size else e


def eff(H, m):
    """the efficiency accumulation of gnm/topology.py's docstring, restated: ascending k, acc = acc + float(H[k]) / float(k), one division by m at the end"""
    acc = 0.0
    for k in range(1, len(H)):
        if H[k]:
            acc = acc + float(H[k]) / float(k)
    return acc / float(m)


def seq_mean(x):
    acc = 0.0
    for v in x:
        acc = acc + float(v)
    return acc / float(len(x))


def closed_form(kind, n):
    """{field: expected array} of a structured kind, from the definition of the graph.  Node fields [n], graph fields
    [1] ([1, n] for the histogram).  Only fields with a closed form that is simple to state are given."""
    z = np.zeros(n, dtype=np.int64)
    ar = np.arange(n, dtype=np.int64)
    hist = np.zeros(max(n, 1), dtype=np.int64)
    out = {}
    if kind == "ring" and n < 4:
        kind = "path"
    if kind == "empty":
        out.update(degree=z, triangles=z, clustering=z * 0.0, eccentricity=z, reachable=z, distance_sum=z, component=ar,
                   nodal_efficiency=z * 0.0, local_efficiency=z * 0.0, edges=[0], components=[n], diameter=[0],
                   transitivity=[0.0])
    elif kind == "complete":
        d = n - 1
        one = 1.0 if n >= 3 else 0.0
        hist[1:2] = n * d if n >= 2 else 0
        out.update(degree=z + d, triangles=z + d * (d - 1) // 2, clustering=z + one, eccentricity=z + min(d, 1),
                   reachable=z + d, distance_sum=z + d, component=z, nodal_efficiency=z + (1.0 if n >= 2 else 0.0),
                   local_efficiency=z + one, edges=[n * d // 2], components=[1], diameter=[min(d, 1)],
                   transitivity=[one])
    elif kind == "path":
        deg = np.minimum(z + 2, n - 1)
        if n >= 2:
            deg[[0, n - 1]] = 1
        for k in range(1, n):
            hist[k] = 2 * (n - k)
        out.update(degree=deg, triangles=z, clustering=z * 0.0, eccentricity=np.maximum(ar, n - 1 - ar),
                   reachable=z + n - 1, distance_sum=ar * (ar + 1) // 2 + (n - 1 - ar) * (n - ar) // 2, component=z,
                   local_efficiency=z * 0.0, edges=[n - 1], components=[1], diameter=[n - 1], transitivity=[0.0])
        c = [[0] + [int(v - k >= 0) + int(v + k < n) for k in range(1, n)] for v in range(n)]
        out["nodal_efficiency"] = np.array([eff(cv, n - 1) if n > 1 else 0.0 for cv in c])
    elif kind == "ring":
        h = n // 2
        for k in range(1, h + 1):
            hist[k] = n if (n % 2 == 0 and k == h) else 2 * n
        c = [0] + [int(hist[k]) // n for k in range(1, h + 1)]
        out.update(degree=z + 2, triangles=z, clustering=z * 0.0, eccentricity=z + h, reachable=z + n - 1,
                   distance_sum=z + sum(k * c[k] for k in range(len(c))), component=z,
                   nodal_efficiency=z + eff(c, n - 1), local_efficiency=z * 0.0, edges=[n], components=[1], diameter=[h],
                   transitivity=[0.0])
    elif kind == "star":
        leaf = (ar > 0).astype(np.int64)
        deg = leaf.copy()
        deg[:1] = n - 1
        if n >= 2:
            hist[1] = 2 * (n - 1)
        if n >= 3:
            hist[2] = (n - 1) * (n - 2)
        far = 2 if n >= 3 else 1
        out.update(degree=deg, triangles=z, clustering=z * 0.0, eccentricity=np.where(leaf == 1, far, min(n - 1, 1)),
                   reachable=z + n - 1, distance_sum=np.where(leaf == 1, 1 + 2 * (n - 2), n - 1), component=z,
                   local_efficiency=z * 0.0, edges=[n - 1], components=[1], diameter=[far if n >= 2 else 0],
                   transitivity=[0.0])
    elif kind == "two_cliques":
        a = n // 2
        b = n - a
        if a < 2:                                   # n <= 3: too small to have the shape; the oracle tests cover it
            return {}
        side = np.where(ar < a, a, b)
        bridge = (ar == a - 1) | (ar == a)
        deg = side - 1 + bridge
        tri = (side - 1) * (side - 2) // 2
        E = a * (a - 1) // 2 + b * (b - 1) // 2 + 1
        hist[1], hist[2], hist[3] = 2 * E, 2 * ((a - 1) + (b - 1)), 2 * (a - 1) * (b - 1)
        other = n - side
        clu = np.array([0.0 if d < 2 else (2.0 * t) / float(d * (d - 1)) for d, t in zip(deg, tri)])
        # a bridge end's neighbours: its clique's other side - 1 nodes, all adjacent, and the far end, adjacent to none
        loc = np.array([0.0 if d < 2 else eff([0, (s - 1) * (s - 2)], d * (d - 1)) for d, s in zip(deg, side)])
        # own side at 1; the far end at 1 from a bridge end and 2 from the rest; the far side one step further
        out.update(degree=deg, triangles=tri, clustering=clu, eccentricity=np.where(bridge, 2, 3), reachable=z + n - 1,
                   distance_sum=np.where(bridge, (side - 1) + 1 + 2 * (other - 1), (side - 1) + 2 + 3 * (other - 1)),
                   component=z, local_efficiency=loc, edges=[E], components=[1], diameter=[3])
        out["transitivity"] = [float(int(tri.sum())) / float(int((deg * (deg - 1) // 2).sum()))]
    elif kind == "two_components_isolated":
        p, q = _split(n)
        part = np.where(ar < p, 0, np.where(ar < p + q, 1, 2))
        i = ar                                      # position inside the path
        deg = np.where(part == 0, np.where((i == 0) | (i == p - 1), min(p - 1, 1), 2), np.where(part == 1, q - 1, 0))
        tri = np.where(part == 1, (q - 1) * (q - 2) // 2, 0)
        for k in range(1, p):
            hist[k] += 2 * (p - k)
        if q >= 2:
            hist[1] += q * (q - 1)
        out.update(degree=deg, triangles=tri, component=np.where(part == 0, 0, np.where(part == 1, p, n - 1)),
                   reachable=np.where(part == 0, p - 1, np.where(part == 1, q - 1, 0)),
                   eccentricity=np.where(part == 0, np.maximum(i, p - 1 - i), np.where(part == 1, min(q - 1, 1), 0)),
                   local_efficiency=np.where((part == 1) & (q >= 3), 1.0, 0.0),
                   edges=[max(p - 1, 0) + q * (q - 1) // 2], components=[(p >= 1) + (q >= 1) + 1],
                   diameter=[max(p - 1, min(q - 1, 1), 0)])
    else:
        raise ValueError(kind)
    if "clustering" in out:
        out["mean_clustering"] = [seq_mean(out["clustering"])] if n else [0.0]
    if "local_efficiency" in out:
        out["mean_local_efficiency"] = [seq_mean(out["local_efficiency"])] if n else [0.0]
    out["distance_histogram"] = hist[None, :]
    pairs = int(hist.sum())
    out["global_efficiency"] = [eff(hist, n * (n - 1)) if n > 1 else 0.0]
    out["characteristic_path_length"] = [float(int((hist * np.arange(hist.shape[0])).sum())) / float(pairs)
                                         if pairs else float("nan")]
    return out


def check_closed_form(m, kind, n):
    """m: a GraphMeasures of numpy arrays of one graph.  Integer fields equal, fp64 fields bitwise (the closed forms
    apply the same formulas to the same integers)."""
    want = closed_form(kind, n)
    for name, w in want.items():
        got = getattr(m, name)
        if got is None:
            assert name in LOCAL_FIELDS, name
            continue
        w = np.asarray(w).astype(got.dtype)
        assert bits_eq(got, w), (kind, n, name, got, w)
    return len(want)


def same_measures(a, b, what=None, fields=NODE_FIELDS + GRAPH_FIELDS):
    """two GraphMeasures of numpy arrays, bitwise in every field (None matches None)"""
    for name in fields:
        x, y = getattr(a, name), getattr(b, name)
        assert (x is None and y is None) or (x is not None and y is not None and bits_eq(x, y)), (what, name, x, y)


def synth(n, edges, label=0):
    from gnm.synth import SynthGraph
    return SynthGraph(n, edges, np.ones((n, 1), np.float32), label)
