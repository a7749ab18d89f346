"""The eval-mode attribution drivers over the C-ABI kernels (saliency and class activation maps, occlusion, virtual
lesions, disconnections and Shapley coalitions, integrated gradients), with the predicates that say which batches each
takes, their scratch budgets and chunk planners.  They call the engine, gnm/core.py; the engine never calls them.  As
there, every N-sized array op runs in libgnm_hip.so: no CPU or eager-PyTorch fallback, a non-GPU tensor raises."""
import contextlib
import ctypes as C
import types

import numpy as np

import torch

from ._cabi import GnmError, check, lib, ptr
from .core import BN_EPS, _agg, _eval_table, _linear, _stream, _stream_scope, _timed, encoder_forward, launch_device


def _rowblock_graph_decline(spec, batch, H):
    """The graphs and width the 32-row-block kernels (csrc/gnm_rowblock.h) take: None, or the condition declined"""
    if spec.n_max:
        return "max neighbour pooling"
    if not getattr(batch, "has_bits", False) or batch.n_max > 416:
        return "a graph of more than 416 nodes or without a bit adjacency"
    if H not in (32, 64, 128):
        return "hidden_dim %d not in {32, 64, 128}" % H
    return None


def _rowblock_model_decline(spec, batch, X):
    """The model and batch the 32-row-block kernels take: None, or the condition declined"""
    if not 1 <= spec.m <= 3 or spec.L > 16:
        return "num_mlp_layers outside 1..3 or more than 16 layers"
    if spec.sync_bn is not None:
        return "synchronised BatchNorm"
    if not X.is_cuda or batch.B < 1:
        return "an empty batch or one off the GPU"
    return None


def _width_decline(X, H):
    """None if the split-precision Linear takes X's width as its contraction, else the condition declined"""
    if not 1 <= X.shape[1] <= int(lib.gnm_linear_max_k(H)):
        return "input width %d outside 1..%d" % (X.shape[1], int(lib.gnm_linear_max_k(H)))
    return None


def saliency_decline(spec, batch, X, P, dx):
    """None if csrc/saliency.hip takes this batch, else the condition it declines.  dx: the input width must fit
    gnm_saliency's dX launch (GIN_InfoMaxReg.saliency(); the gradient class activation and edge maps never form dX)."""
    H = P["batch_norms.0.weight"].shape[0]
    why = _rowblock_graph_decline(spec, batch, H)
    if why is None and spec.n_avg and spec.learn_eps and getattr(batch, "iso", False):
        # the 0/0 row of an isolated node: the autograd path's NaN semantics, not re-derived here
        why = "average neighbour pooling with learned eps and an isolated node"
    if why is None:
        why = _rowblock_model_decline(spec, batch, X)
    if why is None and dx:
        why = _width_decline(X, H)
    return why


def _saliency_table_words(spec, P, saved):
    """gnm_saliency's / gnm_saliency_maps' parameter table (include/gnm_hip.h) over an eval forward's `saved`"""
    L, m = spec.L, spec.m
    words = []
    for l in range(L):
        for k in range(m):
            wn = f"mlps.{l}.linear" if m == 1 else f"mlps.{l}.linears.{k}"
            W = P[wn + ".weight"]
            sv = saved[l].lins[k]
            if W.stride(1) != 1 or sv.z.stride(1) != 1:
                raise GnmError("Linear weights and outputs must be row-contiguous")
            words += [W.data_ptr(), W.stride(0), sv.z.data_ptr(), sv.z.stride(0), sv.scale.data_ptr(),
                      sv.shift.data_ptr()]
    for l in range(L):
        wp = P[f"linears_prediction.{l}.weight"]
        if wp.stride(1) != 1:
            raise GnmError("classifier weights must be row-contiguous")
        words += [wp.data_ptr(), wp.stride(0)]
    assert len(words) == int(lib.gnm_saliency_table_words(L, m))
    return words


def _out_array(out, shape, dev):
    """`out`, a float32 destination of `shape` on `dev` whose rows are contiguous, or a new array of that shape"""
    if out is None:
        return torch.empty(shape, dtype=torch.float32, device=dev)
    if tuple(out.shape) != tuple(shape) or out.stride(-1) != 1 or out.dtype != torch.float32 or out.device != dev:
        raise GnmError("output must be a float32 %s array on %s with contiguous rows" % (list(shape), dev))
    return out


def _launch_dims(spec, batch, X, P):
    """What every eval-mode attribution driver reads off its arguments: the launch device, the dimensions, the
    row-contiguous features and the device pointer of eps (None unless learned)"""
    return types.SimpleNamespace(dev=launch_device(X, P["eps"]), L=spec.L, m=spec.m, N=batch.N, B=batch.B,
                                 F0=X.shape[1], H=P["batch_norms.0.weight"].shape[0],
                                 Cn=P["linears_prediction.0.weight"].shape[0], X=X.contiguous(),
                                 eps=P["eps"].data_ptr() if spec.learn_eps else None)


@contextlib.contextmanager
def _saliency_launch(spec, batch, X, P, scratch_floats):
    """What saliency_hip, saliency_maps_hip and edge_saliency_hip share, as the scope of their launches (no autograd,
    the tensors' device and its stream): the dimensions, ONE eval forward through the training kernels (encoder_forward,
    BatchNorm on its running statistics; it leaves every Linear's pre-BatchNorm output z, which give the ReLU masks),
    gnm_saliency's parameter table over it on the device, and scratch_floats(N, H) floats of scratch."""
    k = _launch_dims(spec, batch, X, P)
    dev = k.dev
    with torch.no_grad(), _stream_scope(dev):
        _, _, saved = encoder_forward(spec, batch, k.X, P, training=False, update_running=False)
        k.table = torch.tensor(_saliency_table_words(spec, P, saved), dtype=torch.int64).pin_memory().to(
            dev, non_blocking=True)
        k.scratch = torch.empty(int(scratch_floats(k.N, k.H)), dtype=torch.float32, device=dev)
        yield k
    # (the forward's arrays and the table are freed here with launches still queued: the caching allocator hands
    # their memory only to later work on the same stream)


def saliency_hip(spec, batch, X, P, classes, outs=None):
    """d score[:, c] / d X (graphcnn.py:254-266 for a whole batch in eval mode) for every c in `classes`: one eval
    forward (_saliency_launch), then L + 1 launches of gnm_saliency per class.  Parameters, buffers and the numpy RNG
    are not touched.  Returns a list of [N, F0] tensors, one per class (written into `outs` when given: row-contiguous
    [N, F0] destinations)."""
    res = []
    with _saliency_launch(spec, batch, X, P, lib.gnm_saliency_scratch_floats) as k:
        N, F0 = k.N, k.F0
        for ci, c in enumerate(classes):
            dX = outs[ci] if outs is not None else torch.empty((N, F0), dtype=torch.float32, device=k.dev)
            if dX.shape != (N, F0) or dX.stride(1) != 1:
                raise GnmError("saliency output must be a row-contiguous [%d, %d] array" % (N, F0))
            with _timed("saliency_hip", B=k.B, N=N, F0=F0, H=k.H):
                check(lib.gnm_saliency(*batch.bits_ptrs(transposed=True), batch.node_off.data_ptr(), *batch.deg_ptrs(),
                                       k.B, batch.n_max, N, F0, k.H, spec.L, spec.m, k.Cn, int(c), int(spec.n_avg),
                                       int(not spec.learn_eps), int(spec.g_avg), k.table.data_ptr(), k.eps,
                                       k.scratch.data_ptr(), dX.data_ptr(), dX.stride(0), _stream()), "gnm_saliency")
            res.append(dX)
    return res


def class_activation_hip(spec, batch, X, P, classes, out=None):
    """The per-node class activation maps cam[v] = p_g sum_l <h_l[v], linears_prediction[l].weight[c]> of a whole batch
    (graphcnn.py:288 class_activation) for every c in `classes`: ONE eval forward through the training kernels
    (encoder_forward, BatchNorm on its running statistics), then gnm_class_activation, which re-forms each h_l from the
    layer's z, scale and shift.  Any neighbour pooling or adjacency form.  Parameters, buffers and the numpy RNG are not
    touched.  Returns a float32 [len(classes), N] tensor (`out` when given)."""
    d = _launch_dims(spec, batch, X, P)
    dev, L, m, N, B, H, Cn = d.dev, d.L, d.m, d.N, d.B, d.H, d.Cn
    out = _out_array(out, (len(classes), N), dev)
    with torch.no_grad(), _stream_scope(dev):
        _, _, saved = encoder_forward(spec, batch, d.X, P, training=False, update_running=False)
        words = []
        for l in range(L):
            sv = saved[l].lins[m - 1]
            wp = P[f"linears_prediction.{l}.weight"]
            if sv.z.stride(1) != 1 or wp.stride(1) != 1:
                raise GnmError("layer outputs and classifier weights must be row-contiguous")
            words += [sv.z.data_ptr(), sv.z.stride(0), sv.scale.data_ptr(), sv.shift.data_ptr(), wp.data_ptr(),
                      wp.stride(0)]
        assert len(words) == int(lib.gnm_class_activation_table_words(L))
        table = torch.tensor(words, dtype=torch.int64).pin_memory().to(dev, non_blocking=True)
        step = int(lib.gnm_class_activation_max_classes())
        for j0 in range(0, len(classes), step):
            cls = [int(c) for c in classes[j0:j0 + step]]
            dst = out[j0:j0 + len(cls)]
            with _timed("class_activation_hip", B=B, N=N, H=H, C=len(cls)):
                check(lib.gnm_class_activation(batch.node_off.data_ptr(), B, batch.n_max, N, H, L, Cn,
                                               (C.c_int * len(cls))(*cls), len(cls), int(spec.g_avg),
                                               table.data_ptr(), dst.data_ptr(), dst.stride(0), _stream()),
                      "gnm_class_activation")
    return out


def saliency_maps_hip(spec, batch, X, P, classes, out=None):
    """The gradient class activation maps gcam[v] = sum_l <d score[:, c] / d h_l[v], h_l[v]> of a whole batch
    (graphcnn.py:284,289 grad_class_activation: h.grad on the retained hidden_rep[l] of compute_saliency) for every c
    in `classes`: one eval forward (_saliency_launch), then L launches of gnm_saliency_maps per class.  Parameters,
    buffers and the numpy RNG are not touched.  Returns a float32 [len(classes), N] tensor (`out` when given)."""
    with _saliency_launch(spec, batch, X, P, lib.gnm_saliency_scratch_floats) as k:
        out = _out_array(out, (len(classes), k.N), k.dev)
        for ci, c in enumerate(classes):
            with _timed("saliency_maps_hip", B=k.B, N=k.N, H=k.H):
                check(lib.gnm_saliency_maps(*batch.bits_ptrs(transposed=True), batch.node_off.data_ptr(),
                                            *batch.deg_ptrs(), k.B, batch.n_max, k.N, k.H, spec.L, spec.m, k.Cn, int(c),
                                            int(spec.n_avg), int(not spec.learn_eps), int(spec.g_avg),
                                            k.table.data_ptr(), k.eps, k.scratch.data_ptr(), out[ci].data_ptr(),
                                            _stream()), "gnm_saliency_maps")
    return out


def _first_linear_product(X, P, m, rows, F0, H):
    """XW = X W0^T [rows, H] on the split-precision Linear: layer 0's first Linear without its bias, any input width"""
    W0 = P["mlps.0.linear.weight" if m == 1 else "mlps.0.linears.0.weight"]
    XW = torch.empty((rows, H), dtype=torch.float32, device=X.device)
    _linear(X, W0, 0, None, XW, rows, F0, H, None, None)
    return XW


def _runs_within(count, floats_of, budget_bytes):
    """Items 0 .. count - 1 in order as runs (i0, i1): each the longest run from i0, of at least one item, that stops
    before the first item that would take 4 * floats_of(i0, i1) bytes (items i0 .. i1 - 1) over budget_bytes"""
    i0 = 0
    while i0 < count:
        i1 = i0 + 1
        while i1 < count and 4 * floats_of(i0, i1 + 1) <= budget_bytes:
            i1 += 1
        yield i0, i1
        i0 = i1


def edge_saliency_hip(spec, batch, X, P, classes, out=None):
    """The connectivity saliency d score[:, c] / d A[u, v] of a whole batch for every c in `classes` and every node
    pair (u, v) of each graph, A the dense Adj_block of graphcnn.py:84-106 (see include/gnm_hip.h gnm_edge_saliency):
    one eval forward (_saliency_launch) and Y = X W0^T on the split-precision Linear per batch, then per class L layer
    launches and one contraction launch of gnm_edge_saliency.  The shapes saliency_decline takes.  Parameters,
    buffers and the numpy RNG are not touched.  Returns a float32 [len(classes), N, n_max] tensor (`out` when given):
    graph b's map is rows node_off[b] .. node_off[b + 1], columns 0 .. n_b."""
    L = spec.L
    with _saliency_launch(spec, batch, X, P, lambda N, H: lib.gnm_edge_saliency_scratch_floats(N, H, L)) as k:
        nm = int(batch.n_max)
        out = _out_array(out, (len(classes), k.N, nm), k.dev)
        Y = _first_linear_product(k.X, P, spec.m, k.N, k.F0, k.H)         # layer 0's term at width H: <dZ0, X W0^T>
        for ci, c in enumerate(classes):
            with _timed("edge_saliency_hip", B=k.B, N=k.N, H=k.H):
                check(lib.gnm_edge_saliency(*batch.bits_ptrs(), batch.t_bits_off.data_ptr(), batch.node_off.data_ptr(),
                                            *batch.deg_ptrs(), k.B, nm, k.N, k.H, L, spec.m, k.Cn, int(c),
                                            int(spec.n_avg), int(not spec.learn_eps), int(spec.g_avg),
                                            k.table.data_ptr(), k.eps, k.scratch.data_ptr(), Y.data_ptr(), Y.stride(0),
                                            out[ci].data_ptr(), out.stride(1), _stream()),
                      "gnm_edge_saliency")
    return out


def occlusion_decline(spec, batch, X, P):
    """None if csrc/occlusion.hip takes this batch, else the condition it declines.  Unlike saliency_decline an isolated
    node under average pooling with learned eps is taken: a deleted graph's NaN stays in its own score."""
    H = P["batch_norms.0.weight"].shape[0]
    why = _rowblock_graph_decline(spec, batch, H) or _rowblock_model_decline(spec, batch, X)
    if why is None and batch.n_min < 2:
        why = "a graph of fewer than 2 nodes"
    return why or _width_decline(X, H)


@contextlib.contextmanager
def _virtual_launch(d, spec, P, classes):
    """What the drivers of virtual graphs share, as the scope of their launches (no autograd, the tensors' device and
    its stream).  Adds to d = _launch_dims(...): cls, the classes as a C array; table, eval_forward_fused's device
    parameter table; and XW = X W0^T [N, H] (the split-precision Linear, any input width)."""
    d.cls = (C.c_int * len(classes))(*[int(c) for c in classes])
    with torch.no_grad(), _stream_scope(d.dev):
        d.table = _eval_table(spec, P, d.dev)
        d.XW = _first_linear_product(d.X, P, d.m, d.N, d.F0, d.H)
        yield d


def _score_tail(d, spec, scratch, dst):
    """The arguments gnm_occlusion, gnm_lesion and gnm_disconnect end with, H to the stream (d: _virtual_launch's)"""
    return (d.H, d.L, d.m, d.Cn, d.cls, len(d.cls), int(spec.n_avg), int(not spec.learn_eps), int(spec.g_avg), BN_EPS,
            d.table.data_ptr(), d.eps, scratch.data_ptr(), dst.data_ptr(), dst.stride(0), _stream())


# occlusion_hip's scratch (two [sum n^2, H] activation arrays and the readout shares) stays under this many bytes: the
# source graphs of a batch are run in chunks.  One 416-node graph at H = 128, L = 16 needs 0.22 GB.
OCCLUSION_SCRATCH_BYTES = 2 << 30


def occlusion_hip(spec, batch, X, P, classes, out=None):
    """The eval-mode class scores of every node-deleted copy of every graph of a batch (csrc/occlusion.hip,
    include/gnm_hip.h gnm_occlusion): out[ci, node_off[g] + v] = c_logit[classes[ci]] of graph g without node v.  Per
    batch _virtual_launch's XW and S = (A + I) XW (the CSR gather: one kernel whatever the batch's density, so a graph's
    result does not depend on its batch-mates); then, per chunk of source graphs whose scratch fits
    OCCLUSION_SCRATCH_BYTES, L layer launches and the finish launch.  The shapes occlusion_decline takes.  Parameters,
    buffers and the numpy RNG are not touched.  Returns a float32 [len(classes), N] tensor (`out` when given)."""
    d = _launch_dims(spec, batch, X, P)
    dev, L, N, B, H = d.dev, d.L, d.N, d.B, d.H
    out = _out_array(out, (len(classes), N), dev)
    offs = np.asarray(batch.node_off_host, dtype=np.int64)
    ns = np.diff(offs)
    sq = np.concatenate([[0], np.cumsum(ns * ns)])          # activation rows before graph g: sum of n^2
    with _virtual_launch(d, spec, P, classes):
        f32 = dict(dtype=torch.float32, device=dev)
        XW, S = d.XW, torch.empty((N, H), **f32)
        check(lib.gnm_agg(*batch.csr_ptrs(), *batch.deg_ptrs(), batch.node_off.data_ptr(), B, batch.n_max,
                          batch.nnz_max, XW.data_ptr(), XW.stride(0), S.data_ptr(), S.stride(0), H, None, 0, 1, 0,
                          None, 0, None, _stream()), "gnm_agg")

        def floats(g0, g1):
            return int(lib.gnm_occlusion_scratch_floats(int(sq[g1] - sq[g0]), int(offs[g1] - offs[g0]),
                                                        int(ns[g0:g1].max()), H, L))
        for g0, g1 in _runs_within(B, floats, OCCLUSION_SCRATCH_BYTES):
            nc = ns[g0:g1]
            V, r0, rows = int(nc.sum()), int(offs[g0]), int(sq[g1] - sq[g0])
            up = batch.arena._upload
            node_off = up(torch.as_tensor((offs[g0:g1 + 1] - offs[g0]).astype(np.int32)))
            vrow_off = up(torch.as_tensor(sq[g0:g1] - sq[g0]))
            vgraph = up(torch.as_tensor(np.repeat(np.arange(g1 - g0, dtype=np.int32), nc)))
            bits_off, rp_off = batch.bits_off[g0:g1], batch.rp_off[g0:g1]
            scratch = torch.empty(floats(g0, g1), **f32)
            dst = out[:, r0:r0 + V]
            with _timed("occlusion_hip", B=g1 - g0, N=V, H=H, L=L):
                check(lib.gnm_occlusion(batch.arena.bits.buf.data_ptr(), bits_off.data_ptr(), node_off.data_ptr(),
                                        batch.arena.rowptr.buf.data_ptr(), rp_off.data_ptr(), vgraph.data_ptr(),
                                        vrow_off.data_ptr(), g1 - g0, int(nc.max()), V, rows, XW[r0:].data_ptr(),
                                        XW.stride(0), S[r0:].data_ptr(), S.stride(0),
                                        *_score_tail(d, spec, scratch, dst)), "gnm_occlusion")
    return out


# csrc/lesion.hip takes what csrc/occlusion.hip takes (a virtual graph whose NaN stays in its own score is taken; a set
# leaves at least one node, so a graph needs two), and so does csrc/disconnect.hip (no node is removed, but the virtual
# graphs run through the same row-block forward): one predicate, one set of strings
lesion_decline = disconnect_decline = occlusion_decline

# lesion_hip's scratch (two [sum of n over the virtual graphs, H] activation arrays and the readout shares) stays under
# this many bytes: the virtual graphs of a batch are run in chunks.  8 graphs x 20 sets at n = 400, H = 128: 0.07 GB.
LESION_SCRATCH_BYTES = 2 << 30


def _virtual_ids(d, batch, vgraph, **masks):
    """`vgraph`, the source graph of each virtual graph, as V contiguous int32 in [0, B); GnmError otherwise, or when one
    of `masks` (name=array: a per-virtual-graph node mask) is not [V, >= n_max]"""
    vgraph = np.ascontiguousarray(vgraph, dtype=np.int32)
    Vt, nm = int(vgraph.shape[0]), int(batch.n_max)
    for name, a in masks.items():
        if a.ndim != 2 or a.shape[0] != Vt or a.shape[1] < nm:
            raise GnmError("%s must be [%d, >= %d], got %s" % (name, Vt, nm, list(a.shape)))
    if Vt and (vgraph.min() < 0 or vgraph.max() >= d.B):
        raise GnmError("vgraph entries must be graphs of the batch, 0 .. %d" % (d.B - 1))
    return vgraph


def _plan_within(floats, cum):
    """_virtual_graphs' planner for a driver whose chunks are cut by their own scratch, floats(q0, q1)"""
    return _runs_within(len(cum) - 1, floats, LESION_SCRATCH_BYTES)


def _pack_masks(d, batch, c, removed):
    """gnm_lesion_pack over a chunk of _virtual_graphs: a keep mask and kept count per row of the host uint8 `removed`"""
    rem = c.up(torch.as_tensor(removed))
    check(lib.gnm_lesion_pack(rem.data_ptr(), rem.stride(0), c.vg.data_ptr(), batch.node_off.data_ptr(), d.B, c.n_max,
                              c.masks.shape[0], c.mstride, c.masks.data_ptr(), c.counts.data_ptr(), _stream()),
          "gnm_lesion_pack")


def _lesion_score(c, kept):
    """gnm_lesion over a chunk of _virtual_graphs; kept: the kept counts on the device and the same on the host"""
    check(lib.gnm_lesion(*c.head, c.mstride, kept[0].data_ptr(), kept[1].ctypes.data, *c.tail), "gnm_lesion")


def _virtual_graphs(label, d, spec, batch, P, classes, vgraph, out, plan, scratch_floats, pack, score, copies=1):
    """The chunk loop of lesion_hip, disconnect_hip and shapley_hip: out[ci, q] = the class score of virtual graph q, a
    copy under keep masks of graph vgraph[q] (as _virtual_ids leaves it).  Per batch _virtual_launch's table and XW;
    then per chunk (q0, q1) of whole virtual graphs, as plan(floats, cum) cuts them (floats(q0, q1): the entry's
    scratch_floats of a chunk; cum: the activation rows before each virtual graph), a namespace c: q0, q1, V; nc, the
    node counts (host int32); n_max, rows, mstride; up, the arena's upload; vg (the chunk's vgraph, `copies` times in a
    row) and vrow_off on the device; masks [copies V, mstride] and counts [copies V] for the pack to fill; head and tail,
    the arguments gnm_lesion and gnm_disconnect share up to the first mask and from the node counts on.  kept = pack(c)
    writes the masks and gives the kept counts; score(c, kept) launches the entry, timed under `label`.  Returns a
    float32 [len(classes), V] tensor (`out` when given)."""
    dev, B, H, L = d.dev, d.B, d.H, d.L
    out = _out_array(out, (len(classes), int(vgraph.shape[0])), dev)
    vn = np.diff(np.asarray(batch.node_off_host, dtype=np.int64))[vgraph].astype(np.int32)    # nodes per virtual graph
    cum = np.concatenate([[0], np.cumsum(vn, dtype=np.int64)])

    def floats(q0, q1):
        return int(scratch_floats(int(cum[q1] - cum[q0]), q1 - q0, int(vn[q0:q1].max()), H, L))
    with _virtual_launch(d, spec, P, classes):
        up = batch.arena._upload
        for q0, q1 in plan(floats, cum):
            c = types.SimpleNamespace(q0=q0, q1=q1, V=q1 - q0, nc=np.ascontiguousarray(vn[q0:q1]), up=up,
                                      rows=int(cum[q1] - cum[q0]))
            c.n_max = int(c.nc.max())
            c.mstride = int(lib.gnm_lesion_mask_words(c.n_max))
            c.vg = up(torch.as_tensor(np.tile(vgraph[q0:q1], copies)))
            c.vrow_off = up(torch.as_tensor(cum[q0:q1] - cum[q0]))
            c.masks = torch.empty((copies * c.V, c.mstride), dtype=torch.int32, device=dev)
            c.counts = torch.empty(copies * c.V, dtype=torch.int32, device=dev)
            kept = pack(c)
            scratch = torch.empty(floats(q0, q1), dtype=torch.float32, device=dev)
            c.head = (batch.arena.bits.buf.data_ptr(), batch.bits_off.data_ptr(), batch.node_off.data_ptr(),
                      c.vg.data_ptr(), c.vrow_off.data_ptr(), c.masks.data_ptr())
            c.tail = (c.nc.ctypes.data, B, c.n_max, c.V, c.rows, d.XW.data_ptr(), d.XW.stride(0),
                      *_score_tail(d, spec, scratch, out[:, q0:q1]))
            with _timed(label, B=B, N=c.V, H=H, L=L):
                score(c, kept)
    return out


def lesion_hip(spec, batch, X, P, classes, removed, vgraph, out=None):
    """The eval-mode class scores of set-deleted copies of the graphs of a batch (csrc/lesion.hip, include/gnm_hip.h
    gnm_lesion): out[ci, q] = c_logit[classes[ci]] of graph vgraph[q] of the batch without the nodes r with
    removed[q, r] != 0.  removed: a host uint8 / bool array [V, >= n_max] (entries past a graph's n are ignored);
    vgraph: V host ints in [0, B).  _virtual_graphs' loop: per chunk of whole virtual graphs whose scratch fits
    LESION_SCRATCH_BYTES, the mask-packing launch, ONE read-back of the kept counts, L layer launches and the finish
    launch.  The shapes lesion_decline takes.  Parameters, buffers and the numpy RNG are not touched.  Returns a
    float32 [len(classes), V] tensor (`out` when given)."""
    d = _launch_dims(spec, batch, X, P)
    removed = np.ascontiguousarray(np.asarray(removed) != 0, dtype=np.uint8)
    vgraph = _virtual_ids(d, batch, vgraph, removed=removed)

    def pack(c):
        _pack_masks(d, batch, c, removed[c.q0:c.q1])
        return c.counts, c.counts.cpu().numpy()             # the one read-back of the chunk

    return _virtual_graphs("lesion_hip", d, spec, batch, P, classes, vgraph, out, _plan_within,
                           lib.gnm_lesion_scratch_floats, pack, _lesion_score)


def disconnect_hip(spec, batch, X, P, classes, in_a, in_b, vgraph, out=None):
    """The eval-mode class scores of edge-cut copies of the graphs of a batch (csrc/disconnect.hip, include/gnm_hip.h
    gnm_disconnect): out[ci, q] = c_logit[classes[ci]] of graph vgraph[q] of the batch without the edges (u, v) with
    (in_a[q, u] and in_b[q, v]) or (in_b[q, u] and in_a[q, v]); every node and feature row stays.  in_a, in_b: host
    uint8 / bool arrays [V, >= n_max] (entries past a graph's n are ignored); vgraph: V host ints in [0, B).
    _virtual_graphs' loop: per chunk of whole virtual graphs whose scratch fits LESION_SCRATCH_BYTES, ONE
    gnm_lesion_pack launch over the chunk's A rows followed by its B rows (the two keep masks; the chunk's vg lists its
    virtual graphs twice, gnm_disconnect reads the first V), L layer launches and the finish launch.  Nothing is read
    back: the readout runs over n, which the host knows.  The shapes disconnect_decline takes.  Parameters, buffers
    and the numpy RNG are not touched.  Returns a float32 [len(classes), V] tensor (`out` when given)."""
    d = _launch_dims(spec, batch, X, P)
    in_a = np.ascontiguousarray(np.asarray(in_a) != 0, dtype=np.uint8)
    in_b = np.ascontiguousarray(np.asarray(in_b) != 0, dtype=np.uint8)
    vgraph = _virtual_ids(d, batch, vgraph, in_a=in_a, in_b=in_b)
    if in_a.shape != in_b.shape:
        raise GnmError("in_a and in_b must have one shape, got %s and %s" % (list(in_a.shape), list(in_b.shape)))

    def pack(c):
        _pack_masks(d, batch, c, np.concatenate([in_a[c.q0:c.q1], in_b[c.q0:c.q1]]))    # (its kept counts: not used)
        return c.up(torch.as_tensor(c.nc))                  # the readout's divisor: every node stays

    def score(c, kept):
        check(lib.gnm_disconnect(*c.head, c.masks[c.V:].data_ptr(), c.mstride, kept.data_ptr(), *c.tail),
              "gnm_disconnect")

    return _virtual_graphs("disconnect_hip", d, spec, batch, P, classes, vgraph, out, _plan_within,
                           lib.gnm_disconnect_scratch_floats, pack, score, copies=2)


def _runs_under(f, budget):
    """_runs_within for a cost that is a difference of a non-decreasing prefix array: items 0 .. len(f) - 2 as runs
    (i0, i1), each the longest of at least one item with f[i1] - f[i0] <= budget -- one bisection per run"""
    i0, count = 0, len(f) - 1
    while i0 < count:
        i1 = max(i0 + 1, int(np.searchsorted(f, f[i0] + budget, side="right")) - 1)
        yield i0, i1
        i0 = i1


def shapley_hip(spec, batch, X, P, classes, labels, vgraph, ids, K, ranks=None, out=None):
    """The eval-mode class scores of the coalitions of a node labelling (csrc/shapley.hip gnm_coalition_pack in front
    of the unchanged gnm_lesion): out[ci, q] = c_logit[classes[ci]] of graph vgraph[q] of the batch without its labelled
    nodes whose group is absent from coalition ids[q].  labels: a host int array [B, >= n_max], row b the labels of
    graph b in -1 .. K - 1 (-1: background, never removed; entries past a graph's n are ignored); vgraph: V host ints
    in [0, B); ids: V host ints.  ranks None, the bitset form (K <= 32): bit p of an id says group p is present.
    ranks a host int [M, K] array of inverse permutations, the prefix form (K <= 416): id = m (K + 1) + j keeps the
    groups p with ranks[m, p] < j.

    lesion_hip's chunk loop (_virtual_graphs; here the chunk's scratch is bounded through the batch's largest graph)
    with three differences: a virtual graph costs 4 bytes of description (its id; the labels go up once per batch)
    instead of a removed row; the kept counts gnm_lesion checks are computed here from the group sizes, so nothing is
    read back; and a coalition that keeps no node at all is left out of the launch and scored
    sum_l linears_prediction[l].bias[c], added in fp32 in layer order -- the head's score of a zero pooled vector (if
    none runs, nothing is launched).  The shapes lesion_decline takes.  Returns float32 [len(classes), V] (or `out`)."""
    d = _launch_dims(spec, batch, X, P)
    dev, L, B, H = d.dev, d.L, d.B, d.H
    nm, K = int(batch.n_max), int(K)
    ids = np.ascontiguousarray(ids, dtype=np.int64)
    labels = np.asarray(labels)
    Vt = len(vgraph)
    if labels.ndim != 2 or labels.shape[0] != B or labels.shape[1] < nm or labels.dtype.kind not in "iu":
        raise GnmError("labels must be an int [%d, >= %d] array, got %s %s" % (B, nm, labels.dtype, list(labels.shape)))
    if ids.shape != (Vt,):
        raise GnmError("ids must be [%d], got %s" % (Vt, list(ids.shape)))
    vgraph = _virtual_ids(d, batch, vgraph)
    ns = np.diff(np.asarray(batch.node_off_host, dtype=np.int64))
    lab = labels[:, :nm].astype(np.int64)
    inside = np.arange(nm)[None, :] < ns[:, None]
    if (lab[inside] < -1).any() or (lab[inside] >= K).any():
        raise GnmError("labels must lie in -1 .. %d" % (K - 1))
    if ranks is None:
        if not 1 <= K <= 32:
            raise GnmError("the bitset form takes 1 .. 32 groups, got %d" % K)
        top = 1 << K
    else:
        ranks = np.ascontiguousarray(ranks, dtype=np.int64)
        if not 1 <= K <= 416 or ranks.ndim != 2 or ranks.shape[1] != K or ranks.shape[0] < 1:
            raise GnmError("the prefix form takes ranks [M >= 1, K] with 1 <= K <= 416, got K = %d and %s"
                           % (K, list(ranks.shape)))
        if not (np.sort(ranks, axis=1) == np.arange(K)[None, :]).all():
            raise GnmError("every row of ranks must be a permutation of 0 .. %d" % (K - 1))
        top = ranks.shape[0] * (K + 1)
    if Vt and (ids.min() < 0 or ids.max() >= top):
        raise GnmError("coalition ids must lie in 0 .. %d" % (top - 1))
    # the kept counts from the group sizes: background + the sizes of the groups present
    sizes = np.stack([np.bincount(lab[b][inside[b] & (lab[b] >= 0)], minlength=K) for b in range(B)]).astype(np.int64)
    kept_all = ((lab < 0) & inside).sum(1)[vgraph]
    if ranks is None:
        for p in np.nonzero(sizes.any(0))[0]:
            kept_all = kept_all + ((ids >> int(p)) & 1) * sizes[vgraph, p]
    else:
        order = np.argsort(ranks, axis=1)                                 # order[m, j]: the player at position j
        csum = np.concatenate([np.zeros((B, ranks.shape[0], 1), dtype=np.int64),
                               np.cumsum(sizes[:, order], axis=2)], axis=2)       # [B, M, K + 1]
        kept_all = kept_all + csum[vgraph, ids // (K + 1), ids % (K + 1)]
    out = _out_array(out, (len(classes), Vt), dev)
    run = np.nonzero(kept_all > 0)[0]
    Vr = int(run.shape[0])
    up = batch.arena._upload
    if Vr:
        ids_r = ids[run].astype(np.int32)
        kept_r = np.ascontiguousarray(kept_all[run], dtype=np.int32)
        lab16 = np.full((B, nm), -1, dtype=np.int16)
        lab16[inside] = lab[inside]
        lab_d = up(torch.as_tensor(lab16))                  # once per batch
        ranks_d = up(torch.as_tensor(ranks.astype(np.int16))) if ranks is not None else None

        def plan(floats, cum):
            # gnm_lesion_scratch_floats with the chunk's largest graph bounded by the batch's: a prefix array
            cost = 2 * cum * H + L * np.arange(Vr + 1, dtype=np.int64) * ((nm + 31) // 32) * H
            return _runs_under(cost, LESION_SCRATCH_BYTES // 4)

        def pack(c):
            idd = c.up(torch.as_tensor(ids_r[c.q0:c.q1]))
            check(lib.gnm_coalition_pack(lab_d.data_ptr(), lab_d.stride(0), c.vg.data_ptr(), idd.data_ptr(), ptr(ranks_d),
                                         ranks.shape[0] if ranks is not None else 0, K, batch.node_off.data_ptr(), B,
                                         c.n_max, c.V, c.mstride, c.masks.data_ptr(), c.counts.data_ptr(), _stream()),
                  "gnm_coalition_pack")
            return c.counts, np.ascontiguousarray(kept_r[c.q0:c.q1])

        res = _virtual_graphs("shapley_hip", d, spec, batch, P, classes, vgraph[run], out if Vr == Vt else None, plan,
                              lib.gnm_lesion_scratch_floats, pack, _lesion_score)
    if Vr != Vt:
        # the coalitions that keep no node: the head's score of a zero pooled vector at every layer
        with torch.no_grad(), _stream_scope(dev):
            ci = torch.as_tensor([int(c) for c in classes], device=dev)
            empty = torch.zeros(len(classes), dtype=torch.float32, device=dev)
            for l in range(L):
                empty = empty + P["linears_prediction.%d.bias" % l].detach()[ci]
            out[:] = empty[:, None]
            if Vr:
                out[:, up(torch.as_tensor(run))] = res
    return out


def shapley_exact_hip(values, K, interactions=False):
    """Exact Shapley values from all 2^K coalition scores (csrc/shapley.hip gnm_shapley_exact): values float32
    [n_classes, G, 2^K] on the device -> phi fp64 [n_classes, G, K] and, with interactions, inter fp64
    [n_classes, G, K, K] (else None).  The weights come from gnm/shapley.py (math.comb, fp64)."""
    from .shapley import interaction_weights, shapley_weights
    dev = launch_device(values)
    if values.dim() != 3 or values.dtype != torch.float32 or values.shape[2] != 1 << K:
        raise GnmError("values must be float32 [n_classes, G, 2^%d], got %s %s" % (K, values.dtype, list(values.shape)))
    values = values.contiguous()
    Cc, G = int(values.shape[0]), int(values.shape[1])
    w = np.ascontiguousarray(shapley_weights(K))
    u = np.ascontiguousarray(interaction_weights(K)) if interactions and K > 1 else None
    with torch.no_grad(), _stream_scope(dev):
        phi = torch.empty((Cc, G, K), dtype=torch.float64, device=dev)
        inter = torch.empty((Cc, G, K, K), dtype=torch.float64, device=dev) if interactions else None
        check(lib.gnm_shapley_exact(values.data_ptr(), G << K, Cc, G, K, w.ctypes.data,
                                    u.ctypes.data if u is not None else None, phi.data_ptr(),
                                    inter.data_ptr() if interactions else None, _stream()), "gnm_shapley_exact")
    return phi, inter


def shapley_permutation_hip(values, ranks):
    """Sampled Shapley values from the prefix scores of M permutations (csrc/shapley.hip gnm_shapley_permutation):
    values float32 [n_classes, G, M, K + 1] on the device, ranks a host int [M, K] array of inverse permutations ->
    (mean, stderr) fp64 [n_classes, G, K]."""
    dev = launch_device(values)
    ranks = np.ascontiguousarray(ranks, dtype=np.int64)
    if ranks.ndim != 2 or ranks.shape[0] < 1 or not (np.sort(ranks, axis=1) == np.arange(ranks.shape[1])[None, :]).all():
        raise GnmError("every row of ranks must be a permutation of 0 .. K - 1")
    M, K = ranks.shape
    if values.dim() != 4 or values.dtype != torch.float32 or tuple(values.shape[2:]) != (M, K + 1):
        raise GnmError("values must be float32 [n_classes, G, %d, %d], got %s %s"
                       % (M, K + 1, values.dtype, list(values.shape)))
    values = values.contiguous()
    Cc, G = int(values.shape[0]), int(values.shape[1])
    with torch.no_grad(), _stream_scope(dev):
        ranks_d = torch.as_tensor(ranks.astype(np.int16)).to(dev)
        mean = torch.empty((Cc, G, K), dtype=torch.float64, device=dev)
        err = torch.empty((Cc, G, K), dtype=torch.float64, device=dev)
        check(lib.gnm_shapley_permutation(values.data_ptr(), G * M * (K + 1), Cc, G, M, K, ranks_d.data_ptr(),
                                          mean.data_ptr(), err.data_ptr(), _stream()), "gnm_shapley_permutation")
    return mean, err


# integrated_gradients_hip's device arrays per chunk of source graphs stay under this many bytes: the virtual batch's
# forward keeps every Linear's z and every layer's aggregation, (m L + L - 1) K N H floats, next to 4 K N H of scratch.
# K = 32, 8 graphs of 400 nodes, H = 64, m = 2, L = 5: 0.26 GB of z, 0.47 GB in all.
INTGRAD_SCRATCH_BYTES = 2 << 30


def _intgrad_floats(rows, H, L, m, K):
    """floats integrated_gradients_hip holds for a chunk of `rows` source rows: z0 and the forward's saved arrays over
    the K rows virtual rows, and gnm_integrated_gradients' scratch"""
    return (m * L + L - 1) * K * rows * H + int(lib.gnm_integrated_gradients_scratch_floats(rows, H, K))


def integrated_gradients_hip(spec, batch, X, P, classes, alphas, weights, baseline=None, out=None):
    """Integrated gradients of a whole batch for every c in `classes` (include/gnm_hip.h gnm_integrated_gradients):
    out[ci, row] = (X - x')[row] * sum_k weights[k] d score[:, c] / d X at x' + alphas[k] (X - x'), x' = `baseline`
    ([n, F0], shared by the graphs, which then all have n nodes) or zeros.  Per batch P = pool(X W0^T) (and Q of the
    baseline): the split-precision Linear, then the layer-0 aggregation at width H (agg_launch) -- pool and W0 commute.
    Then per chunk of source graphs whose arrays fit INTGRAD_SCRATCH_BYTES (never a part of one graph's steps):
    gnm_intgrad_z0, the rest of the eval forward over the K B virtual graphs (encoder_forward from z0; the virtual
    batch lists every arena graph K times, so it shares the source graphs' adjacency), and per class
    gnm_integrated_gradients.  The shapes saliency_decline(dx=True) takes.  Parameters, buffers and the numpy RNG are
    not touched.  Returns a float32 [len(classes), N, F0] tensor (`out` when given)."""
    d = _launch_dims(spec, batch, X, P)
    dev, L, m, N, B, H, Cn, F0, X = d.dev, d.L, d.m, d.N, d.B, d.H, d.Cn, d.F0, d.X
    a32 = np.ascontiguousarray(alphas, dtype=np.float64).astype(np.float32)
    w32 = np.ascontiguousarray(weights, dtype=np.float64).astype(np.float32)
    K = int(a32.shape[0])
    if K < 1 or a32.ndim != 1 or w32.shape != a32.shape:
        raise GnmError("integrated gradients need K >= 1 nodes and as many weights")
    out = _out_array(out, (len(classes), N, F0), dev)
    offs = np.asarray(batch.node_off_host, dtype=np.int64)
    ns = np.diff(offs)
    arena = batch.arena
    with torch.no_grad(), _stream_scope(dev):
        f32 = dict(dtype=torch.float32, device=dev)
        b0 = P["mlps.0.linear.bias" if m == 1 else "mlps.0.linears.0.bias"].contiguous()
        al, wt = arena._upload(torch.as_tensor(a32)), arena._upload(torch.as_tensor(w32))

        def pooled_product(src, rows):
            """pool(src) W0^T as pool(src W0^T): src is [rows, F0] (the batch's features, or ONE graph's baseline)"""
            XW = _first_linear_product(src, P, m, rows, F0, H)
            if rows != N:
                XW = XW.repeat(B, 1)
            Pz = torch.empty((N, H), **f32)
            _agg(batch, XW, Pz, H, d.eps, spec, backward=False)
            return Pz

        Pz = pooled_product(X, N)
        Qz = None
        if baseline is not None:
            baseline = baseline.to(device=dev, dtype=torch.float32).contiguous()
            if baseline.dim() != 2 or baseline.shape[1] != F0 or (ns != baseline.shape[0]).any():
                raise GnmError("the baseline must be [n, %d] with n the node count of every graph" % F0)
            Qz = pooled_product(baseline, int(baseline.shape[0]))
        gh = batch.gids.cpu().numpy()
        for g0, g1 in _runs_within(B, lambda g0, g1: _intgrad_floats(int(offs[g1] - offs[g0]), H, L, m, K),
                                   INTGRAD_SCRATCH_BYTES):
            r0, rows = int(offs[g0]), int(offs[g1] - offs[g0])
            sub = batch if (g0, g1) == (0, B) else arena.batch_from_gids(gh[g0:g1])
            vb = arena.batch_from_gids(np.repeat(gh[g0:g1], K))
            z0 = torch.empty((K * rows, H), **f32)
            check(lib.gnm_intgrad_z0(Pz[r0:].data_ptr(), Pz.stride(0), Qz[r0:].data_ptr() if Qz is not None else None,
                                     Qz.stride(0) if Qz is not None else 0, b0.data_ptr(), sub.node_off.data_ptr(),
                                     sub.B, sub.n_max, al.data_ptr(), K, H, z0.data_ptr(), z0.stride(0), _stream()),
                  "gnm_intgrad_z0")
            _, _, saved = encoder_forward(spec, vb, None, P, training=False, update_running=False, z0=z0)
            table = torch.tensor(_saliency_table_words(spec, P, saved), dtype=torch.int64).pin_memory().to(
                dev, non_blocking=True)
            scratch = torch.empty(int(lib.gnm_integrated_gradients_scratch_floats(rows, H, K)), **f32)
            for ci, c in enumerate(classes):
                dst = out[ci, r0:r0 + rows]
                with _timed("integrated_gradients_hip", B=sub.B, N=rows, F0=F0, H=H, K=K):
                    check(lib.gnm_integrated_gradients(
                        *sub.bits_ptrs(transposed=True), sub.node_off.data_ptr(), *sub.deg_ptrs(), sub.B, sub.n_max,
                        rows, F0, H, L, m, Cn, int(c), int(spec.n_avg), int(not spec.learn_eps), int(spec.g_avg),
                        table.data_ptr(), d.eps, scratch.data_ptr(), vb.t_bits_off.data_ptr(),
                        vb.node_off.data_ptr(), vb.rp_off.data_ptr(), K, wt.data_ptr(), X[r0:].data_ptr(), X.stride(0),
                        ptr(baseline), baseline.stride(0) if baseline is not None else 0,
                        int(baseline.shape[0]) if baseline is not None else 0, dst.data_ptr(), out.stride(1),
                        _stream()), "gnm_integrated_gradients")
            del saved, table, scratch, z0
    return out


