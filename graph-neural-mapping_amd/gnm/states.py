"""Connectivity states: k-means over the window FC matrices of a dynamic-connectivity study, on the device
(csrc/dynstates.hip).  Re-exported by gnm.connectome.

    st = connectivity_states(fc, k)                                        # fc [W, n, n]
    st = connectivity_states_from_timeseries(ts, k, window, stride)        # the FC never exists whole
    labels, dist = assign_states(other_fc, st.centroids)                   # the assignment step alone
    stats = state_statistics(st.labels, st.windows, k)                     # occupancy, dwell, transitions per subject

The features of a window are its entries fc[w, i, j], i < j; only i <= j is ever read.  Both entry points run

    M = init; prev = None
    for it in 1 .. max_iter:
        label, dist = assign(M)                       # label -1: a window with a NaN or inf above its diagonal
        if prev is not None and label == prev: converged; stop
        M = update(M, label); prev = label            # an empty cluster keeps its centroid
    else: label, dist = assign(M)                     # max_iter ran out: the labels belong to the returned centroids

over chunks of at most DYNFC_WORK_BYTES of FC (gnm.connectome), assigning and accumulating while a chunk is there; the
series route recomputes each chunk with the sliding-window kernels into one reused buffer.  A window's distances do not
depend on the call, the sums are sequential in ascending window order and carried from chunk to chunk, the mean is one
division: the two routes agree bitwise at any chunk size, and a numpy loop reproduces a centroid to the last bit.
"""
import numbers

import numpy as np
import torch

from . import connectome as _C
from ._cabi import check

# debugging and tests: a list here receives ("labels", iteration, labels [W] numpy) after every assignment and
# ("seed", distances [W] numpy, chosen window) for every k-means++ draw; each record costs a readback
TRACE = None


class ConnectivityStates:
    """centroids [k, n, n] float64 (device, symmetric, the mean diagonal on the diagonal), labels [W] int32 (device, -1
    for an invalid window), distances [W, k] float64 (device), counts [k] int64 (device: members of each state under
    labels), inertia (float: the assigned distances of the valid windows, added in ascending window order on the
    device), n_iter, converged, windows ([W, 3] int64 numpy (subject, window index, first row) on the series route,
    else None)"""

    __slots__ = ("centroids", "labels", "distances", "counts", "inertia", "n_iter", "converged", "windows")

    def __init__(self, centroids, labels, distances, counts, inertia, n_iter, converged, windows):
        self.centroids, self.labels, self.distances, self.counts = centroids, labels, distances, counts
        self.inertia, self.n_iter, self.converged, self.windows = inertia, n_iter, converged, windows

    def __repr__(self):
        return "ConnectivityStates(k=%d, windows=%d, n_iter=%d, converged=%s, inertia=%r)" % (
            int(self.centroids.shape[0]), int(self.labels.shape[0]), self.n_iter, self.converged, self.inertia)


def _k_arg(k, W):
    if isinstance(k, (bool, np.bool_)) or not isinstance(k, numbers.Integral):
        raise ValueError("k must be an int >= 1, got %r" % (k,))
    k, kmax = int(k), int(_C.lib.gnm_states_max_k())
    if k < 1 or k > kmax:
        raise ValueError("k = %d states: 1 <= k <= %d is supported" % (k, kmax))
    if k > W:
        raise ValueError("k = %d states from %d windows" % (k, W))
    return k


def _iter_arg(max_iter):
    if isinstance(max_iter, (bool, np.bool_)) or not isinstance(max_iter, numbers.Integral) or int(max_iter) < 1:
        raise ValueError("max_iter must be an int >= 1, got %r" % (max_iter,))
    return int(max_iter)


def _init_arg(init, k, n, W):
    """(None, None) for k-means++, ("centroids", [k, n, n] float64 CPU or device tensor) or ("windows", [k] int64 numpy):
    shapes and index ranges checked here, before anything touches the device"""
    if init is None:
        return None, None
    t = init if torch.is_tensor(init) else torch.as_tensor(np.asarray(init))
    if t.dim() == 3:
        if tuple(t.shape) != (k, n, n):
            raise ValueError("init centroids must be [k, n, n] = [%d, %d, %d], got %s" % (k, n, n, tuple(t.shape)))
        if t.dtype not in (torch.float64, torch.float32):
            raise ValueError("init centroids must be float64 or float32, got %s" % t.dtype)
        return "centroids", t
    if t.dim() == 1 and t.dtype in (torch.int64, torch.int32, torch.int16, torch.int8, torch.uint8):
        idx = t.detach().cpu().numpy().astype(np.int64)
        if idx.shape[0] != k:
            raise ValueError("init: %d window indices for k = %d" % (idx.shape[0], k))
        if ((idx < 0) | (idx >= W)).any():
            raise ValueError("init window indices must lie in 0 .. %d, got %s" % (W - 1, idx.tolist()))
        if np.unique(idx).shape[0] != k:
            raise ValueError("init window indices must be distinct, got %s" % (idx.tolist(),))
        return "windows", idx
    raise ValueError("init must be None, [k, n, n] centroids or k window indices, got shape %s %s"
                     % (tuple(t.shape), t.dtype))


def kmeanspp_draw(d2, rng, first=False):
    """The window a k-means++ step draws, in numpy alone.  d2 [W]: each window's squared distance to its nearest centre
    so far, not finite for an invalid window.  first=True: uniformly among the windows whose d2 is finite (the first
    centre; the values are not used).  Otherwise with probability d2 / sum(d2) over the finite entries, by one
    rng.random() against their cumulative sum, so a window at distance 0 (a centre already chosen) is never drawn.
    ValueError when nothing can be drawn."""
    d2 = np.asarray(d2, dtype=np.float64).reshape(-1)
    ok = np.isfinite(d2)
    if first:
        cand = np.flatnonzero(ok)
        if cand.shape[0] == 0:
            raise ValueError("no valid window: every window holds a NaN or inf above its diagonal")
        return int(cand[rng.integers(cand.shape[0])])
    w = np.where(ok, d2, 0.0)
    cum = np.cumsum(w)
    if not (w >= 0).all() or cum.shape[0] == 0 or not cum[-1] > 0:
        raise ValueError("k-means++: every valid window coincides with a centre already chosen (fewer distinct "
                         "windows than k)")
    i = int(np.searchsorted(cum, rng.random() * cum[-1], side="right"))
    return min(i, int(np.flatnonzero(w > 0)[-1]))       # the product may round up to cum[-1] itself


class _Engine:
    """The chunk loop both routes share.  chunks() yields (lo, hi, fc [hi - lo, n, n]) over windows 0 .. W in order;
    pick(idx) gives the FC of the chosen windows [len(idx), n, n]."""

    def __init__(self, chunks, pick, W, n, k, dev, per_chunk):
        self.chunks, self.pick, self.W, self.n, self.k, self.dev = chunks, pick, W, n, k, dev
        self.labels = torch.empty(W, dtype=torch.int32, device=dev)
        self.dist = torch.empty((W, k), dtype=torch.float64, device=dev)
        self.sum = torch.empty((k, n, n), dtype=torch.float64, device=dev)
        self.count = torch.empty(k, dtype=torch.int64, device=dev)
        self.work = torch.empty(int(_C.lib.gnm_states_workspace_doubles(per_chunk, n, k)), dtype=torch.float64,
                                device=dev)

    def sweep(self, cen, accumulate, dist=None):
        """one pass over the windows: labels and distances against cen [kc, n, n] (kc <= k), and with accumulate the
        sums and counts of the update"""
        lib, kc = _C.lib, int(cen.shape[0])
        dist = self.dist if dist is None else dist
        if accumulate:
            self.sum.zero_()
            self.count.zero_()
        with torch.cuda.device(self.dev):
            st = torch.cuda.current_stream(self.dev).cuda_stream
            for lo, hi, fc in self.chunks():
                check(lib.gnm_states_assign(fc.data_ptr(), cen.data_ptr(), hi - lo, self.n, kc, 0, self.work.data_ptr(),
                                            dist[lo:].data_ptr(), self.labels[lo:].data_ptr(), st), "gnm_states_assign")
                if accumulate:
                    check(lib.gnm_states_accumulate(fc.data_ptr(), self.labels[lo:].data_ptr(), hi - lo, self.n, kc,
                                                    self.sum.data_ptr(), self.count.data_ptr(), st),
                          "gnm_states_accumulate")

    def finish(self, cen):
        with torch.cuda.device(self.dev):
            st = torch.cuda.current_stream(self.dev).cuda_stream
            check(_C.lib.gnm_states_finish(self.sum.data_ptr(), self.count.data_ptr(), self.n, self.k, cen.data_ptr(),
                                           st), "gnm_states_finish")

    def inertia(self):
        out = torch.empty(1, dtype=torch.float64, device=self.dev)
        with torch.cuda.device(self.dev):
            st = torch.cuda.current_stream(self.dev).cuda_stream
            check(_C.lib.gnm_states_inertia(self.dist.data_ptr(), self.labels.data_ptr(), self.W, self.k,
                                            out.data_ptr(), st), "gnm_states_inertia")
        return float(out.item())

    def seed(self, rng):
        """k-means++: one sweep per centre, [W] doubles read back for each draw"""
        k, n = self.k, self.n
        cen = torch.zeros((k, n, n), dtype=torch.float64, device=self.dev)
        chosen = []
        for c in range(k):
            kc = max(c, 1)                  # the first sweep runs against one all-zero centroid: finite = valid
            dist = torch.empty((self.W, kc), dtype=torch.float64, device=self.dev)
            self.sweep(cen[:kc], False, dist)
            d2 = dist.min(dim=1).values.cpu().numpy()
            w = kmeanspp_draw(d2, rng, first=(c == 0))
            if TRACE is not None:
                TRACE.append(("seed", d2, w))
            chosen.append(w)
            cen[c] = self.pick(np.array([w], dtype=np.int64))[0]
        return cen, chosen

    def run(self, kind, init, max_iter, seed, windows):
        k, n, dev = self.k, self.n, self.dev
        if kind is None:
            cen, _ = self.seed(np.random.default_rng(seed))
        elif kind == "windows":
            cen = self.pick(init).clone()
            if not bool(torch.isfinite(torch.triu(cen)).all()):
                bad = [int(w) for w, m in zip(init, cen) if not bool(torch.isfinite(torch.triu(m)).all())]
                raise ValueError("init windows %s are invalid: a NaN or inf on or above the diagonal" % bad)
        else:
            cen = init.to(device=dev, dtype=torch.float64).contiguous().clone()
            if not bool(torch.isfinite(torch.triu(cen)).all()):
                raise ValueError("init centroids must be finite on and above the diagonal")
        prev, converged, n_iter = None, False, 0
        for it in range(1, max_iter + 1):
            n_iter = it
            self.sweep(cen, True)
            if TRACE is not None:
                TRACE.append(("labels", it, self.labels.cpu().numpy()))
            if prev is None:
                if int((self.labels >= 0).sum().item()) == 0:       # the iteration's one readback
                    raise ValueError("no valid window: every window holds a NaN or inf above its diagonal")
            elif int((self.labels != prev).sum().item()) == 0:
                converged = True
                break
            self.finish(cen)
            prev = self.labels.clone()
        else:
            self.sweep(cen, False)
            if TRACE is not None:
                TRACE.append(("labels", max_iter + 1, self.labels.cpu().numpy()))
        counts = torch.bincount(self.labels[self.labels >= 0].long(), minlength=k)
        return ConnectivityStates(cen, self.labels, self.dist, counts, self.inertia(), n_iter, converged, windows)


def _fc_engine(fcd, k):
    """the engine over a materialised FC stack on the device, in _plan_chunks' chunks (the workspace is per chunk)"""
    W, n, dev = int(fcd.shape[0]), int(fcd.shape[1]), fcd.device
    plan = _C._plan_chunks(W, n, _C.DYNFC_WORK_BYTES)

    def chunks():
        for lo, hi in plan:
            yield lo, hi, fcd[lo:hi]

    def pick(idx):
        return fcd[torch.from_numpy(np.asarray(idx, dtype=np.int64)).to(dev)]

    return _Engine(chunks, pick, W, n, k, dev, max([hi - lo for lo, hi in plan], default=0))


def _series_engine(x, w_beg, window, wd, n, k):
    """the engine over the windows w_beg of the packed series x (both on the device): every pass recomputes the FC chunk
    by chunk into one buffer (window means and gnm_dynfc_corr, or the tapered form with wd [window])"""
    W, dev = int(w_beg.shape[0]), x.device
    plan = _C._plan_chunks(W, n, _C.DYNFC_WORK_BYTES)
    buf = torch.empty((max(hi - lo for lo, hi in plan), n, n), dtype=torch.float64, device=dev)

    def corr(wb, out):
        mean = _C._dyn_means(x, wb, window, n) if wd is None else None
        return _C._dyn_corr(x, wb, window, mean, wd, n, out)

    def chunks():
        for lo, hi in plan:
            yield lo, hi, corr(w_beg[lo:hi], buf[:hi - lo])

    def pick(idx):
        idx = torch.from_numpy(np.asarray(idx, dtype=np.int64)).to(dev)
        return corr(w_beg[idx].contiguous(), torch.empty((int(idx.shape[0]), n, n), dtype=torch.float64, device=dev))

    return _Engine(chunks, pick, W, n, k, dev, max(hi - lo for lo, hi in plan))


def _fc_shape(fc):
    shape = tuple(fc.shape) if hasattr(fc, "shape") else np.asarray(fc).shape
    if len(shape) != 3 or shape[1] != shape[2]:
        raise ValueError("fc must be [W, n, n], got %s" % (shape,))
    return int(shape[0]), int(shape[1])


def assign_states(fc, centroids, device=None):
    """(labels [W] int32, distances [W, k] float64), both on the device: the assignment step alone, fc [W, n, n] against
    centroids [k, n, n] (finite on i <= j), as connectivity_states takes them.  For windows the states were not fitted
    on; a window's distances are bitwise what any other call gives for it."""
    W, n = _fc_shape(fc)
    cshape = tuple(centroids.shape) if hasattr(centroids, "shape") else np.asarray(centroids).shape
    k = _k_arg(cshape[0] if len(cshape) == 3 else 0, max(W, int(_C.lib.gnm_states_max_k())))     # k > W is fine here
    _, cen = _init_arg(centroids, k, n, W)
    dev = torch.device(device) if device is not None else _C._default_device(fc)
    fcd = _C._as_fc(fc, dev)
    cen = cen.to(device=dev, dtype=torch.float64).contiguous()
    if not bool(torch.isfinite(torch.triu(cen)).all()):
        raise ValueError("centroids must be finite on and above the diagonal")
    eng = _fc_engine(fcd, k)
    eng.sweep(cen, False)
    return eng.labels, eng.dist


def connectivity_states(fc, k, *, init=None, max_iter=100, seed=0, device=None):
    """k connectivity states of the window FC matrices fc [W, n, n] (float64, or float32 widened first; numpy or torch,
    host or device): a ConnectivityStates.  init: None (k-means++ from np.random.default_rng(seed)), [k, n, n] centroids
    (finite on i <= j) or k distinct window indices.  ValueError for a bad k or init and when no window is valid."""
    W, n = _fc_shape(fc)
    k = _k_arg(k, W)
    max_iter = _iter_arg(max_iter)
    kind, init = _init_arg(init, k, n, W)
    dev = torch.device(device) if device is not None else _C._default_device(fc)
    return _fc_engine(_C._as_fc(fc, dev), k).run(kind, init, max_iter, seed, None)


def connectivity_states_from_timeseries(ts, k, window, stride=1, taper=None, *, init=None, max_iter=100, seed=0,
                                        device=None):
    """connectivity_states of the sliding-window FC of ts (dynamic_connectivity_from_timeseries' windows, subject-major
    and window-minor; ts, window, stride and taper as there) without the FC ever existing whole: every pass recomputes
    it chunk by chunk, at most DYNFC_WORK_BYTES at a time in one buffer.  Bitwise the result of connectivity_states on
    the materialised FC, at any chunk size; init window indices count the windows in that order and only those windows
    are computed for them.  The result's windows is the [W, 3] table (subject, window index, first row)."""
    window, stride = _C._window_args(window, stride)
    w = _C._taper_arg(taper, window)
    x, t_off, S, n = _C._timeseries(ts)
    w_beg_h, windows, _ = _C._plan_windows(t_off, window, stride)
    k = _k_arg(k, int(w_beg_h.shape[0]))
    max_iter = _iter_arg(max_iter)
    kind, init = _init_arg(init, k, n, int(w_beg_h.shape[0]))
    dev = torch.device(device) if device is not None else _C._ts_device(ts)
    x, _ = _C._to_device(x, t_off, dev)
    eng = _series_engine(x, torch.from_numpy(w_beg_h).to(dev), window, None if w is None else torch.from_numpy(w).to(dev),
                         n, k)
    return eng.run(kind, init, max_iter, seed, windows)


class StateStatistics:
    """occupancy [S, k], dwell [S, k], transitions [S, k, k] (int64), n_transitions [S] (int64): numpy arrays"""

    __slots__ = ("occupancy", "dwell", "transitions", "n_transitions")

    def __init__(self, occupancy, dwell, transitions, n_transitions):
        self.occupancy, self.dwell, self.transitions, self.n_transitions = occupancy, dwell, transitions, n_transitions


def state_statistics(labels, windows_or_counts, k):
    """Per-subject summaries of a label sequence (labels [W] ints, -1 for an invalid window; subject-major and
    window-minor, as the builders lay windows out).  windows_or_counts: the [W, 3] windows table (its first column is
    the subject) or the [S] number of windows of each subject.  Plain numpy on the host; torch tensors are accepted.
      occupancy[s, c]      the share of subject s's valid windows in state c (0 where it has none)
      dwell[s, c]          the mean length, in windows, of the maximal runs of consecutive windows in state c; 0 where c
                           is never visited; a -1 window ends a run
      transitions[s, a, b] adjacent window pairs (t, t + 1) of subject s with labels a then b, both valid
      n_transitions[s]     its off-diagonal total"""
    lab = labels.detach().cpu().numpy() if torch.is_tensor(labels) else np.asarray(labels)
    wc = windows_or_counts.detach().cpu().numpy() if torch.is_tensor(windows_or_counts) \
        else np.asarray(windows_or_counts)
    if isinstance(k, (bool, np.bool_)) or not isinstance(k, numbers.Integral) or int(k) < 1:
        raise ValueError("k must be an int >= 1, got %r" % (k,))
    k = int(k)
    if lab.ndim != 1 or lab.dtype.kind not in "iu":
        raise ValueError("labels must be a 1-D integer array, got shape %s %s" % (lab.shape, lab.dtype))
    lab = lab.astype(np.int64)
    if wc.ndim == 2:
        subj = wc[:, 0].astype(np.int64)
        if subj.shape[0] != lab.shape[0] or (np.diff(subj) < 0).any() or (subj.shape[0] and subj[0] < 0):
            raise ValueError("windows must be the [W, 3] table of the labelled windows, subject-major")
        counts = np.bincount(subj) if subj.shape[0] else np.zeros(0, np.int64)
    elif wc.ndim == 1 and wc.dtype.kind in "iu":
        counts = wc.astype(np.int64)
    else:
        raise ValueError("windows_or_counts must be a [W, 3] windows table or [S] integer counts")
    if (counts < 0).any() or int(counts.sum()) != lab.shape[0]:
        raise ValueError("the subjects' window counts sum to %d, labels has %d" % (int(counts.sum()), lab.shape[0]))
    if ((lab < -1) | (lab >= k)).any():
        raise ValueError("labels must lie in -1 .. %d" % (k - 1))
    S = counts.shape[0]
    occupancy = np.zeros((S, k))
    dwell = np.zeros((S, k))
    transitions = np.zeros((S, k, k), dtype=np.int64)
    o = 0
    for s in range(S):
        seg = lab[o:o + counts[s]]
        o += int(counts[s])
        valid = seg >= 0
        if valid.any():
            occupancy[s] = np.bincount(seg[valid], minlength=k) / valid.sum()
        a, b = seg[:-1], seg[1:]
        both = (a >= 0) & (b >= 0)
        np.add.at(transitions[s], (a[both], b[both]), 1)
        if seg.shape[0]:
            start = np.flatnonzero(np.concatenate([[True], a != b]))           # first window of every maximal run
            length = np.diff(np.concatenate([start, [seg.shape[0]]]))
            state = seg[start]
            runs = np.bincount(state[state >= 0], minlength=k)
            total = np.bincount(state[state >= 0], weights=length[state >= 0], minlength=k)
            dwell[s] = np.divide(total, runs, out=np.zeros(k), where=runs > 0)
    n_transitions = transitions.sum((1, 2)) - np.trace(transitions, axis1=1, axis2=2)
    return StateStatistics(occupancy, dwell, transitions, n_transitions)
