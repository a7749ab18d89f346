#!/usr/bin/env python3
"""Generate the time-series goldens (timeseries/*.npz) by running the REAL reference loader on CPU.

Run where the reference checkout is (it never travels to the GPU machine), like make_connectome_goldens.py:

    python tests/golden/make_timeseries_goldens.py

For each case it writes a small synthetic dataset directory in a temporary directory -- the ROI, behavioural and
connectivity files of make_connectome_goldens.write_dataset, plus one tab-separated ROI time series per subject
(timeseries/<subject>.txt: time in rows, ROIs in columns, BOLD-like values around 1e4 written to 2 decimals) -- and
runs the reference's DataNodes(...).get_feature('mean_bold') and util.load_data(..., 'mean_bold') on it, with the
module global dataset.sourcedir their DataNodes.__call__ reads (dataset.py:46) set to that directory.  Stored per
case, DATA ONLY:
  * ts_k_{s}, ts_scale   subject s's time series as DataNodes parsed it (pandas), float64: every value parses to
                         exactly ts_k / ts_scale (checked here), so the integers [T_s, n] are stored
  * z64                  [S, n] float64, get_feature('mean_bold')'s z-scores (dataset.py:73-74)
  * feat32               [S, n] float32, load_data's node_features of each subject (util.py:118-121)
  * labels               [S] int64
Cases: n = 7 (two subjects, T = 20 and 9), n = 70 (three subjects, T = 50, 64 and 37), n = 400 (one subject,
T = 100).
"""
import os
import sys
import tempfile

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
sys.path.insert(0, REF)
sys.path.insert(0, HERE)

import numpy as np  # noqa: E402

import dataset as ref_dataset  # noqa: E402  (the reference's loader classes)
import util as ref_util  # noqa: E402
from make_connectome_goldens import write_dataset  # noqa: E402

OUT_DIR = os.path.join(HERE, "timeseries")
SCALE = 100


def bold(rng, T, n):
    """k / SCALE with k integer: a per-ROI offset near 1e4, a shared slow signal and noise"""
    base = 1e4 + 300 * rng.standard_normal(n)
    slow = np.sin(np.linspace(0, 6, T))[:, None] * rng.standard_normal(n)[None, :] * 40
    return np.round((base[None, :] + slow + 60 * rng.standard_normal((T, n))) * SCALE).astype(np.int64)


def make_case(name, ks, genders):
    n = ks[0].shape[1]
    ts = [k.astype(np.float64) / SCALE for k in ks]
    fcs = [np.corrcoef(x, rowvar=False) for x in ts]
    out = {"ts_scale": np.int64(SCALE)}
    with tempfile.TemporaryDirectory() as root:
        subjects = write_dataset(root, fcs, genders, 6)
        os.makedirs(os.path.join(root, "timeseries"))
        for sub, k in zip(subjects, ks):
            with open(os.path.join(root, "timeseries", "%d.txt" % sub), "w") as f:
                for row in k:
                    f.write("\t".join("%d.%02d" % (v // SCALE, v % SCALE) for v in row) + "\n")
        ref_dataset.sourcedir = root                 # the global DataNodes.__call__ reads (dataset.py:46)
        nodes = ref_dataset.DataNodes(root)
        order = sorted(str(s) for s in subjects)     # load_data's subject order
        z64 = []
        for s, sub in enumerate(order):
            nodes(sub)
            parsed = np.asarray(nodes.df_timeseries, dtype=np.float64)
            k = ks[subjects.index(int(sub))]
            assert parsed.shape == k.shape
            assert parsed.tobytes() == (k.astype(np.float64) / SCALE).tobytes(), "parse is not k / scale"
            out["ts_k_%d" % s] = k.astype(np.int32)
            z, _ = nodes.get_feature("mean_bold")
            z64.append(np.asarray(z, dtype=np.float64))
        graphs, _ = ref_util.load_data(root, 30, "mean_bold")
    out["z64"] = np.stack(z64)
    out["feat32"] = np.stack([g.node_features.numpy().reshape(n) for g in graphs]).astype(np.float32)
    out["labels"] = np.array([g.label for g in graphs], dtype=np.int64)
    assert out["feat32"].shape == out["z64"].shape and out["feat32"].dtype == np.float32
    path = os.path.join(OUT_DIR, name + ".npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


def main():
    os.makedirs(OUT_DIR, exist_ok=True)
    rng = np.random.default_rng(20261016)
    make_case("n7", [bold(rng, 20, 7), bold(rng, 9, 7)], ["M", "F"])
    make_case("n70", [bold(rng, 50, 70), bold(rng, 64, 70), bold(rng, 37, 70)], ["F", "M", "F"])
    make_case("n400", [bold(rng, 100, 400)], ["M"])


if __name__ == "__main__":
    main()
