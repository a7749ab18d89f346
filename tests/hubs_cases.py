"""Shared by the hub-measure tests (tests/test_hubs_host.py, tests/test_gpu_hubs.py): the layered graph whose path
counts pass 2^53, the labellings, closed-form betweenness of the structured kinds (written from the graphs' definitions,
never through gnm.hubs), restatements of the module formulas, and the comparison helper.  No tests here."""
import numpy as np

from knn_cases import bits_eq
from topology_cases import KINDS, edges_of, synth        # noqa: F401  (re-exported to the two test modules)

HUB_FIELDS = ("betweenness", "betweenness_normalized", "module_degree", "participation", "within_module_z",
              "module_edges", "modularity")
MODULE_FIELDS = HUB_FIELDS[2:]
DTYPES = {"betweenness": np.float64, "betweenness_normalized": np.float64, "module_degree": np.int32,
          "participation": np.float64, "within_module_z": np.float64, "module_edges": np.int64,
          "modularity": np.float64}


def layered3(n):
    """[E, 2] edges of n // 3 layers of three nodes, consecutive layers joined completely: 3^(layers - 1) shortest paths
    between the end layers (3^39 > 2^53 at n = 120), so sigma is inexact there"""
    assert n % 3 == 0
    e = [(3 * l + i, 3 * (l + 1) + j) for l in range(n // 3 - 1) for i in range(3) for j in range(3)]
    return np.asarray(e, dtype=np.int64).reshape(-1, 2)


def case_edges(kind, n):
    return layered3(n) if kind == "layered3" else edges_of(kind, n)


def labels_of(scheme, n):
    """int64 [n] labels: "mod5" = arange(n) % 5 with node 0 in no module (the GPU tests' labelling), "mod7", "blocks7"
    (seven contiguous blocks), "mod64" (every module the kernel can hold)"""
    ar = np.arange(n, dtype=np.int64)
    if scheme == "mod5":
        lab = ar % 5
        lab[:1] = -1
        return lab
    if scheme == "mod7":
        return ar % 7
    if scheme == "blocks7":
        return ar * 7 // max(n, 1)
    if scheme == "mod64":
        return ar % 64
    raise ValueError(scheme)


def betweenness_closed_form(kind, n):
    """[n] float64 unnormalised betweenness of a structured kind from the graph's definition, or None"""
    ar = np.arange(n, dtype=np.int64)
    z = np.zeros(n, dtype=np.float64)
    if kind == "ring" and n < 4:
        kind = "path"
    if kind in ("empty", "complete"):
        return z
    if kind == "path":                              # v separates the v nodes before it from the n - 1 - v after it
        return (ar * (n - 1 - ar)).astype(np.float64)
    if kind == "star":                              # the centre lies between every pair of leaves
        z[:1] = float((n - 1) * (n - 2) // 2)
        return z
    if kind == "ring":
        # odd n: each of the (n - 1) / 2 distances d has n pairs with one path of d - 1 inner nodes; shared by n nodes.
        # even n: the same below n / 2, and the n / 2 antipodal pairs have two paths, each inner node on one of them.
        return z + (float((n - 1) * (n - 3)) / 8.0 if n % 2 else float((n - 2) * (n - 2)) / 8.0)
    if kind == "two_cliques":                       # nodes 0 .. a - 1 and a .. n - 1 joined by {a - 1, a}
        a = n // 2
        b = n - a
        if a < 1:
            return z
        z[a - 1] = float((a - 1) * b)               # between the rest of its clique and the whole other side
        z[a] = float((b - 1) * a)
        return z
    return None


def normalized(bc, n):
    return bc / float((n - 1) * (n - 2) // 2) if n >= 3 else np.zeros(n, dtype=np.float64)


def bct_participation(A, lab, K):
    """1 - sum_m (k_vm / k_v)^2 with k_v the neighbours of v inside any module; 0 where there are none"""
    kvm = np.stack([A[:, lab == m].sum(1) for m in range(K)], 1).astype(np.float64)
    kv = kvm.sum(1)
    with np.errstate(invalid="ignore", divide="ignore"):
        p = 1.0 - ((kvm / kv[:, None]) ** 2).sum(1)
    return np.where(kv > 0, p, 0.0)


def bct_module_z(A, lab, K):
    """BCT's module_degree_zscore: (k - mean) / np.std over the nodes of v's own module, 0 where the std is 0"""
    z = np.zeros(A.shape[0], dtype=np.float64)
    for m in range(K):
        idx = np.flatnonzero(lab == m)
        if idx.size == 0:
            continue
        k = A[np.ix_(idx, idx)].sum(1).astype(np.float64)
        sd = np.std(k)
        z[idx] = (k - k.mean()) / sd if sd > 0 else 0.0
    return z


def same_hubs(a, b, what=None, fields=HUB_FIELDS, pad=False):
    """two HubMeasures of numpy arrays, bitwise in every field (None matches None).  pad: `a` was measured in a batch
    whose labels name more modules than b's own; its further columns of module_degree and module_edges must be zero"""
    for name in fields:
        x, y = getattr(a, name), getattr(b, name)
        if pad and x is not None and y is not None and name in ("module_degree", "module_edges"):
            K = y.shape[-1]
            rest = x.copy()
            if name == "module_edges":
                rest[..., :K, :K] = 0
                x = np.ascontiguousarray(x[..., :K, :K])
            else:
                rest[..., :K] = 0
                x = np.ascontiguousarray(x[..., :K])
            assert not rest.any(), (what, name, rest)
        assert (x is None and y is None) or (x is not None and y is not None and bits_eq(x, y)), (what, name, x, y)
