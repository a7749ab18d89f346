"""Host side of GIN_InfoMaxReg.shapley(): the players are the K groups of a node labelling (-1: background, a node of no
group, never removed), a coalition is the set of groups that are present, and its value is lesion()'s score of the graph
without the labelled nodes of every other group.  Here: the Shapley and interaction weights, the explicit "removed"
masks of coalitions given as bitset ids or as prefixes of permutations (what csrc/shapley.hip gnm_coalition_pack packs
from 4 bytes each), their kept-node counts, and the fp64 restatements of the reductions gnm_shapley_exact /
gnm_shapley_permutation run on the device.  numpy only; nothing here touches the device."""
import math

import numpy as np

EXACT_MAX_PLAYERS = 16         # method="exact": 2^K coalitions per graph
PREFIX_MAX_PLAYERS = 416       # method="permutation": up to one player per node of the largest graph the kernels take


def shapley_weights(K):
    """w_K(s) = 1 / (K C(K - 1, s)), s = 0 .. K - 1: the weight of a coalition of s other players (fp64 [K])"""
    if K < 1:
        raise ValueError("shapley_weights: K must be positive, got %d" % K)
    return np.array([1.0 / (K * math.comb(K - 1, s)) for s in range(K)], dtype=np.float64)


def interaction_weights(K):
    """u_K(s) = 1 / ((K - 1) C(K - 2, s)), s = 0 .. K - 2: the Shapley interaction index's weights (fp64 [K - 1];
    empty at K = 1)"""
    if K < 1:
        raise ValueError("interaction_weights: K must be positive, got %d" % K)
    return np.array([1.0 / ((K - 1) * math.comb(K - 2, s)) for s in range(K - 1)], dtype=np.float64)


def check_labels(labels, n=None):
    """labels as an int64 [n] vector: an int dtype, one dimension, entries >= -1 (ValueError otherwise)"""
    lab = np.asarray(labels)
    if lab.ndim != 1 or lab.dtype.kind not in "iu":
        raise ValueError("labels must be an int [n] vector, got dtype %s shape %s" % (lab.dtype, list(lab.shape)))
    lab = lab.astype(np.int64)
    if lab.size and lab.min() < -1:
        raise ValueError("labels must be group ids >= 0, or -1 for background")
    if n is not None and lab.shape[0] != n:
        raise ValueError("%d labels for a %d-node graph" % (lab.shape[0], n))
    return lab


def check_permutations(perms, K):
    """perms as an int64 [M, K] array whose rows are permutations of 0 .. K - 1 (ValueError otherwise)"""
    p = np.asarray(perms)
    if p.ndim != 2 or p.shape[0] < 1 or p.shape[1] != K or p.dtype.kind not in "iu":
        raise ValueError("permutations must be an int [M, %d] array, M >= 1, got dtype %s shape %s"
                         % (K, p.dtype, list(p.shape)))
    p = p.astype(np.int64)
    if not (np.sort(p, axis=1) == np.arange(K, dtype=np.int64)[None, :]).all():
        raise ValueError("every row of permutations must be a permutation of 0 .. %d" % (K - 1))
    return p


def ranks_of(perms):
    """ranks[m, p] = the position of player p in permutation m (the inverse permutations), int64 [M, K]"""
    p = np.asarray(perms, dtype=np.int64)
    r = np.empty_like(p)
    np.put_along_axis(r, p, np.broadcast_to(np.arange(p.shape[1], dtype=np.int64), p.shape), axis=1)
    return r


def draw_permutations(M, K, seed=0):
    """M rows np.random.default_rng(seed).permutation(K), int64 [M, K]; the numpy global RNG is not touched"""
    if M < 1:
        raise ValueError("permutations must be positive, got %d" % M)
    rng = np.random.default_rng(seed)
    return np.stack([rng.permutation(K) for _ in range(M)]).astype(np.int64)


def coalition_removed(labels, ids):
    """The removed sets of coalitions given as bitset ids: labels int [n], ids int [V]; bit p of an id says group p is
    present.  Returns bool [V, n], True = removed: a labelled node whose group's bit is clear.  Background stays."""
    lab = check_labels(labels)
    ids = np.asarray(ids, dtype=np.int64).reshape(-1)
    present = (ids[:, None] >> np.clip(lab, 0, 62)[None, :]) & 1                  # (ids are below 2^32: bit 62 is clear)
    return (lab >= 0)[None, :] & (present == 0)


def prefix_removed(labels, perms):
    """The removed sets of the prefixes of permutations: labels int [n], perms int [M, K] (rows: permutations of
    0 .. K - 1, K > max(labels)).  Returns bool [M, K + 1, n], True = removed: entry (m, j) keeps the background and the
    groups of the first j players of permutation m, so j = 0 removes every labelled node and j = K none."""
    lab = check_labels(labels)
    p = np.asarray(perms, dtype=np.int64)
    M, K = p.shape
    if lab.size and lab.max() >= K:
        raise ValueError("labels hold group %d but the permutations have %d players" % (int(lab.max()), K))
    rank = ranks_of(p)
    node_rank = rank[:, np.maximum(lab, 0)]                                       # [M, n]
    j = np.arange(K + 1, dtype=np.int64)
    return (lab >= 0)[None, None, :] & (node_rank[:, None, :] >= j[None, :, None])


def group_sizes(labels, K):
    """(sizes int64 [K]: the nodes of each group, background: the number of -1 entries)"""
    lab = check_labels(labels)
    if lab.size and lab.max() >= K:
        raise ValueError("labels hold group %d but K = %d" % (int(lab.max()), K))
    return np.bincount(lab[lab >= 0], minlength=K).astype(np.int64), int((lab < 0).sum())


def kept_counts(labels, K, ids=None, perms=None):
    """The number of nodes each coalition keeps, from the group sizes alone (no mask is formed): with `ids` int64 [V]
    for bitset ids; with `perms` int64 [M, K + 1] for the prefixes of permutations.  The row sums of ~coalition_removed
    / ~prefix_removed."""
    if (ids is None) == (perms is None):
        raise ValueError("kept_counts: give ids or perms")
    sizes, bg = group_sizes(labels, K)
    if ids is not None:
        ids = np.asarray(ids, dtype=np.int64).reshape(-1)
        out = np.full(ids.shape[0], bg, dtype=np.int64)
        for p in np.nonzero(sizes)[0]:
            out += ((ids >> p) & 1) * sizes[p]
        return out
    p = check_permutations(perms, K)
    csum = np.concatenate([np.zeros((p.shape[0], 1), dtype=np.int64), np.cumsum(sizes[p], axis=1)], axis=1)
    return bg + csum


def _insert_zero(c, i):
    """c with a zero bit inserted at position i"""
    return ((c >> i) << (i + 1)) | (c & ((1 << i) - 1))


def _popcount(c):
    out = np.zeros(c.shape, dtype=np.int64)
    c = c.copy()
    while c.any():
        out += c & 1
        c >>= 1
    return out


def shapley_from_values(values, K):
    """phi[..., i] = sum over S in N \\ {i} of w_K(|S|) (v(S + i) - v(S)) in fp64 from values [..., 2^K] (entry id: the
    coalition whose bit p says group p is present).  Differences first, then the weight, then the sum."""
    v = np.asarray(values).astype(np.float64)
    if K < 1 or v.shape[-1] != 1 << K:
        raise ValueError("values must be [..., 2^K] with K >= 1, got K = %d and shape %s" % (K, list(v.shape)))
    w = shapley_weights(K)
    c = np.arange(1 << (K - 1), dtype=np.int64)
    ws = w[_popcount(c)]
    phi = np.empty(v.shape[:-1] + (K,), dtype=np.float64)
    with np.errstate(invalid="ignore"):
        for i in range(K):
            id0 = _insert_zero(c, i)
            phi[..., i] = (ws * (v[..., id0 | (1 << i)] - v[..., id0])).sum(-1)
    return phi


def interactions_from_values(values, K):
    """inter[..., i, j] = sum over S in N \\ {i, j} of u_K(|S|) ((v(S + ij) - v(S + i)) - (v(S + j) - v(S))) in fp64 from
    values [..., 2^K]: the Shapley interaction index, symmetric with a zero diagonal (all zero at K = 1)"""
    v = np.asarray(values).astype(np.float64)
    if K < 1 or v.shape[-1] != 1 << K:
        raise ValueError("values must be [..., 2^K] with K >= 1, got K = %d and shape %s" % (K, list(v.shape)))
    inter = np.zeros(v.shape[:-1] + (K, K), dtype=np.float64)
    if K < 2:
        return inter
    u = interaction_weights(K)
    c = np.arange(1 << (K - 2), dtype=np.int64)
    us = u[_popcount(c)]
    with np.errstate(invalid="ignore"):
        for i in range(K):
            for j in range(i + 1, K):
                id0 = _insert_zero(_insert_zero(c, i), j)
                bi, bj = 1 << i, 1 << j
                d = (v[..., id0 | bi | bj] - v[..., id0 | bi]) - (v[..., id0 | bj] - v[..., id0])
                inter[..., i, j] = inter[..., j, i] = (us * d).sum(-1)
    return inter


def permutation_from_values(values, perms):
    """(mean, stderr) fp64 [..., K] of sampled Shapley values from values [..., M, K + 1] (entry (m, j): the first j
    players of permutation m present) and perms int [M, K]: player i's marginal contribution in permutation m is
    v[m, rank + 1] - v[m, rank], rank its position there; the mean over m and std(ddof=1) / sqrt(M), NaN at M = 1."""
    v = np.asarray(values).astype(np.float64)
    p = np.asarray(perms, dtype=np.int64)
    M, K = p.shape
    if v.shape[-2:] != (M, K + 1):
        raise ValueError("values must be [..., %d, %d], got shape %s" % (M, K + 1, list(v.shape)))
    rank = ranks_of(p)                                                            # [M, K]
    rows = np.arange(M)[:, None]
    with np.errstate(invalid="ignore", divide="ignore"):
        d = v[..., rows, rank + 1] - v[..., rows, rank]                           # [..., M, K]
        mean = d.sum(-2) / M
        if M > 1:
            err = np.sqrt(((d - mean[..., None, :]) ** 2).sum(-2) / (M - 1)) / math.sqrt(M)
        else:
            err = np.full(mean.shape, np.nan)
    return mean, err
