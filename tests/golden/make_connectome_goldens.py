#!/usr/bin/env python3
"""Generate the connectome-builder goldens (connectome/*.npz) by running the REAL reference loader on CPU.

Run where the reference checkout is (it never travels to the GPU machine), like make_goldens.py:

    python tests/golden/make_connectome_goldens.py

For each case it writes a small synthetic dataset directory in a temporary directory -- ROI names with five "_" fields
(roi/7_400.txt, roi/7_400_coord.csv), a behavioural CSV (behavioral/hcp.csv: Subject, Gender) and one tab-separated
connectivity matrix per subject (connectivity/r<subject>.txt) -- and runs the reference's util.load_data on it with
one-hot node features for sparsity 30, 5 and 50.  Stored per case, DATA ONLY, in a compact lossless form that
tests/connectome_goldens.py decodes (the script checks the decoding reproduces the reference's arrays exactly):
  * fc_upper, fc_scale   the matrices as the reference's DataEdges parsed them (pandas), float64: they are written
                         with a fixed number of decimals, are symmetric, and parse to exactly k / fc_scale, so the
                         integers k of the upper triangle (diagonal included, np.triu_indices order) are stored,
                         with the flat indices of the entries that parsed to -0.0 (fc_negzero)
  * feat                 [n, F] float32, the one-hot node features (the same for every subject), labels [S]
  * sp{P}_edge_{s}       the first half of subject s's edge_mat at sparsity P, [2, E], delta-coded along the edges
                         (the second half is the first with its rows swapped: util.py:100-101, checked here)
  * sp{P}_nb_{s}, sp{P}_deg_{s}   neighbors flattened and delta-coded, and the list lengths [n]
  * sp{P}_max_neighbor   [S]
Cases: n = 400 (one subject, a correlation matrix written to 4 decimals), n = 100 with matrices quantized to k / 2^16
and k / 8 (heavy ties), n = 7 (sparsity 30 and 50 only).
"""
import os
import sys
import tempfile

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
sys.path.insert(0, REF)

import numpy as np  # noqa: E402

sys.path.insert(0, os.path.dirname(HERE))
import connectome_goldens  # noqa: E402  (the decoder the tests use)

import util as ref_util  # noqa: E402  (the reference loader)
from dataset import DataEdges  # noqa: E402

OUT_DIR = os.path.join(HERE, "connectome")
SPARSITIES = (30, 5, 50)


def write_dataset(root, fcs, genders, decimals):
    n = fcs[0].shape[0]
    for d in ("connectivity", "behavioral", "roi"):
        os.makedirs(os.path.join(root, d), exist_ok=True)
    nets = ["Vis", "SomMot", "DorsAttn", "SalVentAttn", "Limbic", "Cont", "Default"]
    with open(os.path.join(root, "roi", "7_400.txt"), "w") as f:
        for i in range(n):
            hemi = "LH" if i < (n + 1) // 2 else "RH"
            f.write("%d\t7Networks_%s_%s_R%d_%d\n" % (i + 1, hemi, nets[i % 7], i // 7, i + 1))
    with open(os.path.join(root, "roi", "7_400_coord.csv"), "w") as f:
        f.write("ROI,R,A,S\n")
        for i in range(n + 1):
            f.write("%d,%d,%d,%d\n" % (i, i % 13, i % 17, i % 19))
    subjects = [100000 + 7 * s for s in range(len(fcs))]
    with open(os.path.join(root, "behavioral", "hcp.csv"), "w") as f:
        f.write("Subject,Gender\n")
        for sub, g in zip(subjects, genders):
            f.write("%d,%s\n" % (sub, g))
    for sub, m in zip(subjects, fcs):
        np.savetxt(os.path.join(root, "connectivity", "r%d.txt" % sub), m, delimiter="\t", fmt="%%.%df" % decimals)
    return subjects


def correlation(rng, n, t):
    return np.corrcoef(rng.standard_normal((t, n)).T)


def delta(a):
    a = np.asarray(a, dtype=np.int64)
    d = np.diff(a, axis=-1, prepend=0) if a.size else a
    assert np.abs(d).max(initial=0) < 32768
    return d.astype(np.int16)


def make_case(name, fcs, genders, sparsities=SPARSITIES, decimals=6):
    ref = {}
    with tempfile.TemporaryDirectory() as root:
        subjects = write_dataset(root, fcs, genders, decimals)
        de = DataEdges(root)
        parsed = []
        for sub in sorted(str(s) for s in subjects):
            de(sub)
            parsed.append(np.asarray(de.df, dtype=np.float64))
        fc = np.stack(parsed)
        n = fc.shape[1]
        scale = 10 ** decimals
        k = np.round(fc * scale)
        assert np.abs(k).max() < 2 ** 31
        iu = np.triu_indices(n)
        negzero = np.flatnonzero((fc == 0) & np.signbit(fc))           # "-0.0000" parses to -0.0
        out = {"fc_upper": k[:, iu[0], iu[1]].astype(np.int32), "fc_scale": np.int64(scale),
               "fc_negzero": negzero.astype(np.int64)}
        ref["fc"] = fc
        for sp in sparsities:
            graphs, _ = ref_util.load_data(root, sp, "one_hot")
            feats = [g.node_features.numpy() for g in graphs]
            assert all(np.array_equal(feats[0], x) for x in feats)
            out["feat"] = ref["feat"] = feats[0].astype(np.float32)
            out["labels"] = ref["labels"] = np.array([g.label for g in graphs], dtype=np.int64)
            out["sp%d_max_neighbor" % sp] = np.array([g.max_neighbor for g in graphs], dtype=np.int64)
            for s, g in enumerate(graphs):
                assert len(g.g) == n
                em = g.edge_mat.numpy().reshape(2, -1)
                E = em.shape[1] // 2
                assert np.array_equal(em[:, E:], em[::-1, :E])
                out["sp%d_edge_%d" % (sp, s)] = delta(em[:, :E])
                nb = [int(v) for row in g.neighbors for v in row]
                out["sp%d_nb_%d" % (sp, s)] = delta(nb)
                out["sp%d_deg_%d" % (sp, s)] = np.array([len(r) for r in g.neighbors], dtype=np.uint16)
                ref[(sp, s)] = (em, [list(map(int, r)) for r in g.neighbors], g.max_neighbor)
    path = os.path.join(OUT_DIR, name + ".npz")
    np.savez_compressed(path, **out)
    # the stored form decodes to exactly what the reference produced
    dec = connectome_goldens.load(path)
    assert dec["fc"].view(np.uint64).tobytes() == ref["fc"].view(np.uint64).tobytes()
    assert np.array_equal(dec["feat"], ref["feat"]) and np.array_equal(dec["labels"], ref["labels"])
    for sp, s, em, nb, mx in dec["graphs"]:
        r = ref[(sp, s)]
        assert np.array_equal(em, r[0]) and nb == r[1] and mx == r[2]
    assert len(dec["graphs"]) == len(sparsities) * fc.shape[0]
    print(path, os.path.getsize(path), "bytes")


def main():
    os.makedirs(OUT_DIR, exist_ok=True)
    rng = np.random.default_rng(20261015)
    # one 400-node subject: the fixture stays small (its matrix alone is 160,000 values)
    make_case("n400", [correlation(rng, 400, 120)], ["M"], decimals=4)
    q = np.round(correlation(rng, 100, 30) * 8) / 8                 # a handful of values: heavy ties
    q16 = np.round(correlation(rng, 100, 30) * 65536) / 65536       # k / 2^16
    make_case("n100_ties", [q16, q, correlation(rng, 100, 40)], ["F", "F", "M"])
    # sparsity 5 keeps no edge of a 7-node matrix (its seven 1.0 diagonal entries exceed 5 % of 49), and the reference
    # loader cannot build an edgeless graph (util.py:103)
    make_case("n7", [correlation(rng, 7, 5) for _ in range(4)], ["M", "F", "F", "M"], sparsities=(30, 50))


if __name__ == "__main__":
    main()
