"""Decoder of the connectome goldens (tests/golden/connectome/*.npz, written by
tests/golden/make_connectome_goldens.py, which checks that this decoding reproduces the reference loader's arrays)."""
import glob
import os

import numpy as np

PATHS = sorted(glob.glob(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "connectome", "*.npz")))


def _undelta(d):
    return np.cumsum(np.asarray(d, dtype=np.int64), axis=-1)


def load(path):
    """{"fc": [S, n, n] float64, "feat": [n, F] float32, "labels": [S] int64,
        "graphs": [(sparsity, subject, edge_mat [2, 2E] int64, neighbors (list of lists), max_neighbor)]}"""
    d = np.load(path)
    up = d["fc_upper"].astype(np.float64) / float(d["fc_scale"])
    S, m = up.shape
    n = int(round((np.sqrt(8 * m + 1) - 1) / 2))
    iu = np.triu_indices(n)
    fc = np.empty((S, n, n), dtype=np.float64)
    fc[:, iu[0], iu[1]] = up
    fc[:, iu[1], iu[0]] = up
    fc.reshape(-1)[d["fc_negzero"]] = -0.0
    graphs = []
    for key in sorted(k for k in d.files if k.endswith("_max_neighbor")):
        sp = int(key[2:].split("_")[0])
        for s in range(S):
            half = _undelta(d["sp%d_edge_%d" % (sp, s)]).reshape(2, -1)
            em = np.concatenate([half, half[::-1]], axis=1)
            flat = _undelta(d["sp%d_nb_%d" % (sp, s)])
            off = np.concatenate([[0], np.cumsum(d["sp%d_deg_%d" % (sp, s)].astype(np.int64))])
            nb = [flat[off[i]:off[i + 1]].tolist() for i in range(n)]
            graphs.append((sp, s, em, nb, int(d[key][s])))
    return {"fc": fc, "feat": d["feat"], "labels": d["labels"], "graphs": graphs}
