"""Forward/backward orchestration of the GIN hot path over the C-ABI kernels.

One torch.autograd.Function (GinInfoMaxFn) covers everything GIN_InfoMaxReg.forward
computes after batch assembly (/root/reference models/graphcnn.py:208-251): the L GIN
layers (neighbour aggregation -> MLP -> BatchNorm -> ReLU), the per-layer graph readout and
classifier, and the Infomax discriminator scores.  Its backward is hand-derived (the same
derivation as oracle/gin_oracle.py, which the tests check it against) and launches the
HIP kernels of csrc/ directly; torch only provides device memory, the stream, and a few
tiny [B, .] dense ops (classifier Linear(H, C), U = sigmoid(g_f) W^T).

Every N-sized array op runs in libgnm_hip.so.  There is no CPU or eager-PyTorch fallback
for the sum/average path: on a non-GPU tensor the calls raise.
"""
import collections
import contextlib
import ctypes as C
import types

import numpy as np

import torch
import torch.nn.functional as F

from ._cabi import GnmError, check, lib, ptr

BN_EPS = 1e-5       # nn.BatchNorm1d defaults (mlp.py:38, graphcnn.py:51)
BN_MOMENTUM = 0.1


_STREAM = None      # raw hipStream_t of torch's current stream, fetched once per forward / backward


def _stream():
    return _STREAM if _STREAM is not None else torch.cuda.current_stream().cuda_stream


def launch_device(*tensors):
    """The one CUDA device all of `tensors` (None entries skipped) live on; GnmError otherwise.  The kernels
    take raw pointers, so nothing below this check would notice a CPU tensor or a second device."""
    dev = None
    for t in tensors:
        if t is None:
            continue
        if not t.is_cuda:
            raise GnmError("the GIN hot path runs on the GPU only (libgnm_hip.so); got a %s tensor" % t.device)
        if dev is None:
            dev = t.device
        elif t.device != dev:
            raise GnmError("tensors on different devices (%s and %s): one model replica lives on one GPU"
                           % (dev, t.device))
    if dev is None:
        raise GnmError("no device tensor to launch on")
    return dev


class _stream_scope:
    """Makes `device` (the device of the tensors being worked on, NOT whatever torch.cuda.current_device() happens
    to be) current for the duration of a forward or backward, and resolves its current stream once:
    torch.cuda.current_stream() costs ~10 us of Python per call and there are ~110 launches per step.  Without
    the device switch a model built on cuda:1 in a process whose current device is 0 would launch on device 0's
    stream with device-1 pointers (autograd's backward thread sets the device, a custom Function.forward does not)."""

    def __init__(self, device):
        self.device = device

    def __enter__(self):
        global _STREAM
        self.prev = _STREAM
        self.guard = torch.cuda.device(self.device)
        self.guard.__enter__()
        _STREAM = torch.cuda.current_stream(self.device).cuda_stream

    def __exit__(self, *exc):
        global _STREAM
        _STREAM = self.prev
        self.guard.__exit__(*exc)
        return False


class KernelTimer:
    """Optional per-launch timing with HIP events recorded on the stream the kernels are
    launched on (torch's current stream).  bench.py turns it on for the timed region to
    compute the roofline figures; it is off (None) otherwise."""

    def __init__(self, prefixes=None):
        self.records = []          # (name, meta, start_event, end_event)
        self.prefixes = tuple(prefixes) if prefixes else None   # only time launches whose tag starts with one

    def summary(self):
        """name -> (count, mean ms, meta); call after a synchronize.  Launches recorded under one name with
        DIFFERENT meta (e.g. the fused-prologue aggregation and the plain one) are different kernels: they are
        kept apart under "name|key=value,..." of the differing keys, never averaged together."""
        groups = {}
        for name, meta, a, b in self.records:
            key = (name, tuple(sorted(meta.items())))
            c, t, m = groups.get(key, (0, 0.0, meta))
            groups[key] = (c + 1, t + a.elapsed_time(b), m)
        by_name = {}
        for (name, _), v in groups.items():
            by_name.setdefault(name, []).append(v)
        out = {}
        for name, vs in by_name.items():
            if len(vs) == 1:
                c, t, m = vs[0]
                out[name] = (c, t / c, m)
                continue
            common = set.intersection(*[set(m.items()) for _, _, m in vs])
            for c, t, m in vs:
                diff = ",".join("%s=%s" % kv for kv in sorted(set(m.items()) - common))
                out["%s|%s" % (name, diff)] = (c, t / c, m)
        return out


TIMER = None


def _new_event():
    """HIP event on the launch stream (a seam the CPU tests replace with a fake clock)."""
    return torch.cuda.Event(enable_timing=True)


class _timed:
    """times the launches of its block under `name` (None: never timed)"""

    def __init__(self, name, **meta):
        self.name, self.meta = name, meta

    def __enter__(self):
        self.on = TIMER is not None and self.name is not None and (TIMER.prefixes is None or
                                                                   self.name.startswith(TIMER.prefixes))
        if self.on:
            self.a = _new_event()
            self.b = _new_event()
            self.a.record()

        return self

    def cancel(self):
        """Nothing was launched inside the block (the entry point declined the shape): record no interval."""
        self.on = False

    def __exit__(self, *exc):
        if self.on and TIMER is not None and exc[0] is None:
            self.b.record()
            TIMER.records.append((self.name, self.meta, self.a, self.b))
        return False


class GinSpec:
    """Static description of the model: which parameter tensor is which."""

    def __init__(self, num_layers, num_mlp_layers, learn_eps, graph_pooling_type, neighbor_pooling_type):
        self.L, self.m = num_layers, num_mlp_layers
        self.learn_eps = bool(learn_eps)
        self.g_avg = graph_pooling_type == "average"
        self.n_avg = neighbor_pooling_type == "average"
        # "max" (graphcnn.py:137-143): csrc/maxpool.hip over batch.maxnb (gnm/maxnb.py) in place of the aggregation
        # kernels; the BatchNorm + ReLU of the layer below then runs as its own kernel
        self.n_max = neighbor_pooling_type == "max"
        # Optional gradient sink {parameter name: tensor}: when set (gnm.parallel.DataParallelGIN
        # points it at views of its flat gradient buffer) the backward kernels write every parameter
        # gradient straight into these tensors (OVERWRITING them) and autograd gets None, instead of
        # fresh tensors that AccumulateGrad then adds into .grad with ~50 tiny kernels per step.
        self.grad_sink = None
        # Optional cross-rank BatchNorm (SURVEY.md 8(e) "sync_bn"): an object with all_reduce(tensor) (SUM over
        # the data-parallel group) and global_count(n).  When set, train-mode BatchNorm normalises with the
        # statistics of the UNION batch, so W ranks reproduce one process on the whole batch.  Eager launches only.
        self.sync_bn = None
        # True: every layer's activation h_l = relu(bn(z_l)) is written to memory as an array (test hooks that read
        # them).  Default: layers whose BatchNorm + ReLU ride on the next aggregation's tile load exist only as ZAct
        # (z, scale, shift) -- the discriminator re-forms them in its kernels; 105 MB per layer less HBM traffic.
        self.keep_hidden = False


def _dense(batch, F_, spec=None):
    """does this batch take the matrix-core aggregation (csrc/aggm.hip)?  The arena decides per batch (dense graphs
    with a bit adjacency, GraphArena.batch_from_gids); the kernel wants whole 32-column blocks, or one partial block
    (the input layer's F0 < 32, plain form only: the fused / d-eps forms decline and the gather runs).
    One mode keeps a dense batch on the CSR gather: neighbour "average" + learn_eps with a node that has no
    neighbours.  That node's row is 0/0 = NaN in the reference (graphcnn.py:157-158) and stays confined to the rows
    that gather it; a product multiplies it by the zero bits of every other row of its graph (0 x NaN = NaN)."""
    if spec is not None and spec.n_avg and spec.learn_eps and getattr(batch, "iso", False):
        return False
    return bool(getattr(batch, "dense", False)) and (F_ % 32 == 0 or F_ < 32)


def agg_partials_capacity(batch, F_):
    """doubles a d-eps partial buffer must hold for this batch, whichever aggregation kernel runs"""
    k = int(lib.gnm_agg_num_partials(F_, batch.n_max, batch.B))
    if _dense(batch, F_):           # (an upper bound: whichever kernel the mode selects)
        k = max(k, int(lib.gnm_aggm_num_partials(F_, batch.B)))
    return k


# The neighbour aggregation's three launch forms.  Each has an entry on the matrix cores over the bit adjacency
# (csrc/aggm.hip) and one that gathers over the CSR (csrc/agg.hip); the two take the same arguments after the graph's.
# form -> (matrix-core entry, CSR entry, timer meta of the form)
_AGG_FORMS = {
    "plain": ("gnm_aggm", "gnm_agg", {}),
    # + the BatchNorm + ReLU + readout of the layer below on the tile load
    "fwd_bnrelu": ("gnm_aggm_fwd_bnrelu", "gnm_agg_fwd_bnrelu", {"fused_bnrelu": 1}),
    # + the BatchNorm-backward sums of the layer below in the epilogue
    "bwd_stats": ("gnm_aggm_bwd_stats", "gnm_agg_bwd_stats", {"fused_stats": 1}),
}


def agg_launch(batch, form, F_, args, spec=None, backward=False, dot=False, timed=True, stream=None):
    """The one place that chooses between the two aggregation kernels.  args: the form's own arguments, everything
    between the graph and the stream.  The matrix-core entry runs when _dense(batch, F_, spec) holds and it does not
    decline (-2), else the CSR gather.  The plain form always ends on a launch; a fused form is not tried under max
    pooling and returns -2 when both entries decline (the caller then runs the unfused kernels).  Timed as
    agg_{fwd,bwd}_F<F_>[_dot] unless `timed` is False.  Returns (status, d-eps partials the kernel that ran wrote)."""
    mfma_entry, csr_entry, meta = _AGG_FORMS[form]
    plain = form == "plain"
    if not plain and spec.n_max:
        return -2, 0
    B, n_max = batch.B, batch.n_max
    pro = form == "fwd_bnrelu"          # the prologue form takes no degree CSR and writes no d-eps partials
    graph = batch.csr_ptrs(backward)
    deg = () if pro else batch.deg_ptrs()
    tail = args + (_stream() if stream is None else stream,)
    tag = ("agg_%s_F%d%s" % ("bwd" if backward else "fwd", F_, "_dot" if dot else "")) if timed else None
    if _dense(batch, F_, spec):
        rc = _agg_try(mfma_entry, mfma_entry if plain else csr_entry, False,
                      graph + batch.bits_ptrs(backward) + deg + (batch.node_off.data_ptr(), B, n_max) + tail,
                      _timed(tag, F=F_, B=B, N=batch.N, **meta, mfma=1))
        if rc == 0:
            return 0, 0 if pro else int(lib.gnm_aggm_num_partials(F_, B))
    rc = _agg_try(csr_entry, csr_entry, plain,
                  graph + deg + (batch.node_off.data_ptr(), B, n_max, batch.nnz_max) + tail,
                  _timed(tag, F=F_, B=B, N=batch.N, **meta))
    return rc, 0 if pro or rc != 0 else int(lib.gnm_agg_num_partials(F_, n_max, B))


def _agg_try(entry, name, final, argv, timed):
    """one entry of agg_launch, in its `timed` block: returns its status, a decline (-2, nothing launched) only when it
    is not the `final` one; any other failure raises under `name`"""
    with timed as tm:
        rc = getattr(lib, entry)(*argv)
        if rc != 0:
            if final or rc != -2:
                check(rc, name)
            tm.cancel()
    return rc


def _agg(batch, x, y, F_, eps_ptr, spec, backward, hfwd=None, deps_partial=None):
    """The plain aggregation (agg_launch).  y = None: only the d-eps partials are produced (no gather).  Returns the
    number of d-eps partials written."""
    return agg_launch(batch, "plain", F_, (x.data_ptr(), x.stride(0), ptr(y), y.stride(0) if y is not None else 0, F_,
                                           eps_ptr, int(spec.n_avg), int(not spec.learn_eps), int(backward), ptr(hfwd),
                                           hfwd.stride(0) if hfwd is not None else 0, ptr(deps_partial)),
                      spec, backward, dot=y is None)[1]


def _max_fwd(batch, h, pooled, F_, eps_ptr):
    """pooled = max over the neighbour rows of h [+ (1 + eps) h] (graphcnn.py:137-143, 149-151/161, 173-175).
    Returns (amax, amin): the selected row of every element and torch.min's row per column -- where the backward
    sends the gradient."""
    mb = getattr(batch, "maxnb", None)
    if mb is None or mb.N != batch.N:
        raise GnmError("neighbor_pooling_type='max' needs the graphs' neighbour lists: call forward(batch_graph)")
    N = batch.N
    dev = h.device
    dummy = amin = None
    if mb.need_dummy:                                   # some row is padded: dummy = torch.min(h, dim=0)[0]  (:140)
        nblk = int(lib.gnm_maxpool_colmin_blocks(N))
        wv = torch.empty((nblk, F_), dtype=torch.float32, device=dev)
        wi = torch.empty((nblk, F_), dtype=torch.int32, device=dev)
        dummy = torch.empty(F_, dtype=torch.float32, device=dev)
        amin = torch.empty(F_, dtype=torch.int32, device=dev)
        check(lib.gnm_maxpool_colmin(h.data_ptr(), h.stride(0), N, F_, wv.data_ptr(), wi.data_ptr(), dummy.data_ptr(),
                                     amin.data_ptr(), _stream()), "gnm_maxpool_colmin")
    if mb.max_deg == 0 and not mb.self_last and N > 0:
        raise IndexError("max(): Expected reduction dim 1 to have non-zero size.")     # what torch.max raises (:142)
    amax = torch.empty((N, F_), dtype=torch.int32, device=dev)
    with _timed("maxpool_fwd_F%d" % F_, F=F_, B=batch.B, N=N):
        # one workgroup per graph with its rows in LDS when the shape allows, else rows gathered from L2: same bits
        rc = lib.gnm_maxpool_fwd_tiled(h.data_ptr(), h.stride(0), mb.nb_off.data_ptr(), mb.nb_col.data_ptr(),
                                       batch.node_off.data_ptr(), batch.B, batch.n_max, F_, mb.max_deg,
                                       int(mb.self_last), eps_ptr, ptr(dummy), pooled.data_ptr(), pooled.stride(0),
                                       amax.data_ptr(), _stream())
        if rc == -2:
            rc = lib.gnm_maxpool_fwd(h.data_ptr(), h.stride(0), mb.nb_off.data_ptr(), mb.nb_col.data_ptr(), N, F_,
                                     mb.max_deg, int(mb.self_last), eps_ptr, ptr(dummy), pooled.data_ptr(),
                                     pooled.stride(0), amax.data_ptr(), _stream())
        check(rc, "gnm_maxpool_fwd")
    return amax, amin


def _max_bwd(batch, dpooled, dh, F_, eps_ptr, aux, hfwd, deps_partial):
    """d h from d pooled through the selection recorded by _max_fwd; d eps partials as a flat dot product.
    Returns the number of d-eps partials written."""
    mb = batch.maxnb
    amax, amin = aux
    with _timed("maxpool_bwd_F%d" % F_, F=F_, B=batch.B, N=batch.N):
        rc = lib.gnm_maxpool_bwd_tiled(dpooled.data_ptr(), dpooled.stride(0), amax.data_ptr(), mb.t_off.data_ptr(),
                                       mb.t_col.data_ptr(), batch.node_off.data_ptr(), batch.B, batch.n_max, F_,
                                       eps_ptr, ptr(mb.iso_rows), mb.n_iso, ptr(amin), dh.data_ptr(), dh.stride(0),
                                       _stream())
        if rc == -2:
            rc = lib.gnm_maxpool_bwd(dpooled.data_ptr(), dpooled.stride(0), amax.data_ptr(), mb.t_off.data_ptr(),
                                     mb.t_col.data_ptr(), batch.N, F_, eps_ptr, ptr(mb.iso_rows), mb.n_iso, ptr(amin),
                                     dh.data_ptr(), dh.stride(0), _stream())
        check(rc, "gnm_maxpool_bwd")
    if deps_partial is None:
        return 0
    check(lib.gnm_rowdot_partials(dpooled.data_ptr(), dpooled.stride(0), hfwd.data_ptr(), hfwd.stride(0), batch.N, F_,
                                  deps_partial.data_ptr(), _stream()), "gnm_rowdot_partials")
    return int(lib.gnm_rowdot_num_partials())


def _linear(x, W, w_kmajor, bias, z, N, K, H, pro, stats):
    with _timed("lin_%s_K%d_H%d" % ("dgrad" if w_kmajor else "fwd", K, H), N=N, K=K, H=H):
        check(lib.gnm_linear_fwd(x.data_ptr(), x.stride(0), W.data_ptr(), W.stride(0), int(w_kmajor), ptr(bias),
                                 z.data_ptr(), z.stride(0), N, K, H, ptr(pro[0]) if pro else None,
                                 ptr(pro[1]) if pro else None, 1 if pro else 0, ptr(stats), _stream()),
              "gnm_linear_fwd")


def _linear_wide(x, W, w_kmajor, bias, z, N, K, H, pro, stats):
    """H > 128 (only dX of a wide first layer): column windows of 128."""
    if H <= 128:
        return _linear(x, W, w_kmajor, bias, z, N, K, H, pro, stats)
    assert stats is None
    for h0 in range(0, H, 128):
        hw = min(128, H - h0)
        Wv = W[:, h0:h0 + hw] if w_kmajor else W[h0:h0 + hw]
        _linear(x, Wv, w_kmajor, bias[h0:h0 + hw] if bias is not None else None, z[:, h0:h0 + hw], N, K, hw, pro, None)


# What a kernel leaves in place of gnm_bn_relu_bwd_stats: G, the gradient under the ReLU mask of the BatchNorm + ReLU it
# arrives at, and that BatchNorm's backward sums in `rows` partial rows [2, width] (fp64)
_BnSums = collections.namedtuple("_BnSums", "G part rows")
# a fused Linear backward's dW / db partials in its workspace: reduced by gnm_reduce_partials_multi after the loop
_ReduceJob = collections.namedtuple("_ReduceJob", "ws dW db H K")
# linear_bwd_launch's result: dX or None, the _BnSums of the BatchNorm below or None, the deferred _ReduceJob or None
_LinBwd = collections.namedtuple("_LinBwd", "dA lo_sums job")


def linear_bwd_launch(sv, lo, G, coef, W, bias, dW, db, need_dA, N, stream):
    """The one place that routes a Linear's backward (mlp.py:43,48-49 under autograd).  sv: the Linear's _LinSave, lo:
    the one below it in the MLP or None; G: the masked gradient at the BatchNorm after the Linear, coef = (cA, m1, m2)
    that BatchNorm's backward coefficients (gnm_bn_bwd_finalize); dW / db: where the parameter gradients go.  In order:
    gnm_linear_bwd_fused_rz (Z recomputed), gnm_linear_bwd_fused (stored Z; with `lo` and need_dA it also masks dA and
    takes lo's BatchNorm-backward sums), each one pass whose dW / db partials are reduced later (job); after two
    declines (-2) gnm_bn_bwd_apply in place, gnm_linear_wgrad, and for dA gnm_linear_dgrad_masked (K = H = 128 over a
    BatchNorm) or the plain product _linear_wide.  Returns a _LinBwd."""
    K, Hk, (cA, m1, m2) = sv.K, sv.H, coef
    f32 = dict(dtype=torch.float32, device=G.device)
    pro = (sv.pro[0].data_ptr(), sv.pro[1].data_ptr(), 1) if sv.pro else (None, None, 0)
    dA = torch.empty((N, K), **f32) if need_dA else None
    ws = torch.empty(int(lib.gnm_linear_bwd_workspace_floats(N, Hk, K)), **f32)
    lo_part, los = None, (None, 0, None, None, None, None)
    if lo is not None and need_dA:
        lo_part = torch.empty((lib.gnm_linear_bwd_grid(N), 2, K), dtype=torch.float64, device=G.device)
        los = (lo.z.data_ptr(), lo.z.stride(0), lo.scale.data_ptr(), lo.shift.data_ptr(), lo.mean.data_ptr(),
               lo.rstd.data_ptr())
    with _timed("linbwd_K%d_H%d" % (K, Hk), N=N, K=K, H=Hk) as tm:
        # every argument after Z (dW = NULL: the partials are reduced by ONE launch after the loop)
        args = (sv.mean.data_ptr(), sv.rstd.data_ptr(), cA.data_ptr(), m1.data_ptr(), m2.data_ptr(), sv.x_in.data_ptr(),
                sv.x_in.stride(0), *pro, W.data_ptr(), W.stride(0), ptr(dA), dA.stride(0) if need_dA else 0, None,
                dW.stride(0), db.data_ptr(), ws.data_ptr(), N, K, Hk, *los, ptr(lo_part), stream)
        rc = -2
        # (mirrors gnm_linear_bwd_fused_rz's own decline rules in csrc/linear.hip: a foreign call less per Linear)
        if Hk == 64 and lo_part is None and ((K == 64 and need_dA) or (K <= 16 and not sv.pro)):
            # sv.z = Linear(sv.x_in) as gnm_linear_fwd left it: the pass recomputes it instead of reading it
            rc = lib.gnm_linear_bwd_fused_rz(G.data_ptr(), G.stride(0), bias.data_ptr(), *args)
        if rc == -2:
            rc = lib.gnm_linear_bwd_fused(G.data_ptr(), G.stride(0), sv.z.data_ptr(), sv.z.stride(0), *args)
        if rc != 0:
            tm.cancel()
    if rc == 0:
        return _LinBwd(dA, _BnSums(dA, lo_part, lo_part.shape[0]) if lo_part is not None else None,
                       _ReduceJob(ws, dW, db, Hk, K))
    if rc != -2:
        check(rc, "gnm_linear_bwd_fused")
    # GNM_ERR_UNSUPPORTED: the generic three-kernel path, dZ in place of G
    check(lib.gnm_bn_bwd_apply(G.data_ptr(), G.stride(0), sv.z.data_ptr(), sv.z.stride(0), sv.mean.data_ptr(),
                               sv.rstd.data_ptr(), cA.data_ptr(), m1.data_ptr(), m2.data_ptr(), G.data_ptr(),
                               G.stride(0), N, Hk, stream), "gnm_bn_bwd_apply")
    ws = torch.empty(int(lib.gnm_wgrad_workspace_floats(N, Hk, K)), **f32)
    with _timed("wgrad_K%d_H%d" % (K, Hk), N=N, K=K, H=Hk):
        check(lib.gnm_linear_wgrad(G.data_ptr(), G.stride(0), sv.x_in.data_ptr(), sv.x_in.stride(0), N, Hk, K, *pro,
                                   dW.data_ptr(), dW.stride(0), db.data_ptr(), ws.data_ptr(), stream),
              "gnm_linear_wgrad")
    lo_sums = None
    if need_dA:
        rc = -2
        if lo is not None and K == 128 and Hk == 128:
            # dX = dZ W with the ReLU mask of the BatchNorm + ReLU below and that BatchNorm's backward sums taken in
            # the epilogue (replaces its gnm_bn_relu_bwd_stats pass)
            lo_part = torch.empty((int(lib.gnm_linear_grid(N)), 2, K), dtype=torch.float64, device=G.device)
            rc = lib.gnm_linear_dgrad_masked(G.data_ptr(), G.stride(0), W.data_ptr(), W.stride(0), dA.data_ptr(),
                                             dA.stride(0), N, K, Hk, *los, lo_part.data_ptr(), stream)
            if rc == 0:
                lo_sums = _BnSums(dA, lo_part, lo_part.shape[0])
            elif rc != -2:
                check(rc, "gnm_linear_dgrad_masked")
        if rc == -2:
            _linear_wide(G, W, 1, None, dA, N, Hk, K, None, None)      # dX = dZ W
    return _LinBwd(dA, lo_sums, None)


# the three [B, L*H]-sized products of the Infomax tail run on the hand-written kernel (csrc/sgemm.hip)
def _small_gemm(A, a_cols, B, b_cols, out, M, N, K):
    """out[M,N] = A' B' (csrc/sgemm.hip: gnm_small_gemm); False when the kernel declines and the caller uses torch."""
    if A.stride(1) != 1 or B.stride(1) != 1 or out.stride(1) != 1:
        return False
    rc = lib.gnm_small_gemm(A.data_ptr(), A.stride(0), int(a_cols), B.data_ptr(), B.stride(0), int(b_cols), out.data_ptr(),
                            out.stride(0), M, N, K, _stream())
    if rc == -2:
        return False
    check(rc, "gnm_small_gemm")
    return True


class _LinSave:
    __slots__ = ("x_in", "pro", "z", "scale", "shift", "mean", "rstd", "K", "H", "Ng")


# what encoder_forward keeps of one layer.  h_in: the layer's input (X, an array, or a ZAct); pooled: its aggregation;
# lins: the _LinSave of each Linear of its MLP; aux: what max pooling's backward needs
_LayerSave = collections.namedtuple("_LayerSave", "h_in pooled lins aux")


def encoder_forward(spec, batch, X, P, training, update_running, P0=None, z0=None):
    """The L GIN layers + readout.  P: dict of parameter/buffer tensors keyed by the
    reference's state_dict names.  P0: the arena's cached parameter-independent part of layer 0's
    aggregation (GraphArena.features_and_agg0) or None.  z0: the pre-BatchNorm output [N, H] of layer 0's first Linear,
    given (eval mode only; integrated_gradients_hip): layer 0's aggregation and that Linear are not run and X is not
    read (it may be None).  Returns (hidden list, g_f [B, L*H], saved)."""
    if z0 is not None and training:
        raise GnmError("encoder_forward: z0 is an eval-mode entry")
    dev = X.device if z0 is None else z0.device
    N, B = batch.N, batch.B
    L, m = spec.L, spec.m
    H = P["batch_norms.0.weight"].shape[0]
    f32 = dict(dtype=torch.float32, device=dev)
    g_f = torch.empty((B, L * H), **f32)
    hidden, saved = [], []
    h = X
    sync = spec.sync_bn if training else None
    Ng = sync.global_count(N, dev) if sync is not None else N        # rows of the union batch
    pending = None      # (z, scale, shift, hout, gslice) of the previous layer: its BatchNorm+ReLU+readout not yet run

    def readout(z, scale, shift, hout, gslice):
        check(lib.gnm_bn_relu_readout(z.data_ptr(), z.stride(0), scale.data_ptr(), shift.data_ptr(),
                                      ptr(hout), hout.stride(0) if hout is not None else 0,
                                      batch.node_off.data_ptr(), B, H, 1,
                                      gslice.data_ptr(), g_f.stride(0), int(spec.g_avg), _stream()),
              "gnm_bn_relu_readout")                                          # graphcnn.py:163-166, 228-229

    for l in range(L):
        given = l == 0 and z0 is not None         # layer 0 starts behind its first Linear
        F_l = h.shape[1] if not given else 0
        eps_ptr = P["eps"].data_ptr() + 4 * l if spec.learn_eps else None
        aux = None          # max pooling: what its backward needs
        if given:
            pooled = None
        elif l == 0 and P0 is not None:
            # A X [/deg] comes from the arena's cache; only the (1 + eps_0) X self term depends on a parameter
            pooled = torch.addcmul(P0, h, P["eps"][0:1] + 1.0) if spec.learn_eps else P0
        else:
            pooled = torch.empty((N, F_l), **f32)
            fused = False
            if pending is not None:
                # the previous layer's BatchNorm + ReLU + readout ride on this aggregation's tile load; unless the
                # caller wants the arrays (spec.keep_hidden) the activation itself is not written
                z, scale, shift, hout, gslice = pending
                rc, _ = agg_launch(batch, "fwd_bnrelu", F_l, (
                    z.data_ptr(), z.stride(0), scale.data_ptr(), shift.data_ptr(), ptr(hout),
                    hout.stride(0) if hout is not None else 0, gslice.data_ptr(), g_f.stride(0), int(spec.g_avg),
                    pooled.data_ptr(), pooled.stride(0), F_l, eps_ptr, int(spec.n_avg), int(not spec.learn_eps)), spec)
                if rc == -2:
                    if hout is None:                 # declined: the unfused pair of kernels needs the array after all
                        hout = torch.empty((N, z.shape[1]), **f32)
                        hidden[-1] = hout
                        h = hout
                    readout(z, scale, shift, hout, gslice)
                else:
                    fused = True
                pending = None
            if spec.n_max:
                aux = _max_fwd(batch, hidden_tensor(h), pooled, F_l, eps_ptr)
            elif not fused:
                _agg(batch, hidden_tensor(h), pooled, F_l, eps_ptr, spec, backward=False)    # graphcnn.py:154-161 / 178-182
        x_in, pro, lins = pooled, None, []
        for k in range(m):                                                   # mlp.py:40-49
            if m == 1:
                W, bias = P[f"mlps.{l}.linear.weight"], P[f"mlps.{l}.linear.bias"]
            else:
                W, bias = P[f"mlps.{l}.linears.{k}.weight"], P[f"mlps.{l}.linears.{k}.bias"]
            bn = f"batch_norms.{l}" if k == m - 1 else f"mlps.{l}.batch_norms.{k}"
            Hk, K = W.shape
            grid = lib.gnm_linear_grid(N)
            stats = torch.empty((grid, 2, Hk), dtype=torch.float64, device=dev) if training else None
            if given and k == 0:
                z = z0
            else:
                z = torch.empty((N, Hk), **f32)
                _linear(x_in, W, 0, bias, z, N, K, Hk, pro, stats)
            sv = _LinSave()
            sv.x_in, sv.pro, sv.z, sv.K, sv.H = x_in, pro, z, K, Hk
            sv.scale, sv.shift, sv.mean, sv.rstd = (torch.empty(Hk, **f32) for _ in range(4))
            sv.Ng = Ng
            if sync is not None:
                stats = stats.sum(0, keepdim=True)            # [1,2,Hk] column sum / sum of squares (fp64)
                sync.all_reduce(stats)
                grid = 1
            check(lib.gnm_bn_finalize(ptr(stats), grid, Hk, Ng, P[bn + ".weight"].data_ptr(),
                                      P[bn + ".bias"].data_ptr(), P[bn + ".running_mean"].data_ptr(),
                                      P[bn + ".running_var"].data_ptr(),
                                      P[bn + ".num_batches_tracked"].data_ptr(), BN_MOMENTUM, BN_EPS,
                                      int(training), int(update_running), sv.scale.data_ptr(), sv.shift.data_ptr(),
                                      sv.mean.data_ptr(), sv.rstd.data_ptr(), _stream()), "gnm_bn_finalize")
            lins.append(sv)
            x_in, pro = z, (sv.scale, sv.shift)
        gslice = g_f[:, l * H:(l + 1) * H]
        if l < L - 1:
            # deferred into the next layer's aggregation, which (on its fused path) does not write the activation
            hout = torch.empty((N, H), **f32) if getattr(spec, "keep_hidden", False) else None
            pending = (x_in, pro[0], pro[1], hout, gslice)
            hnew = hout if hout is not None else ZAct(x_in, pro[0], pro[1])
        else:
            # the top layer: only its readout is needed now; the discriminator re-forms the activation like the others
            hout = torch.empty((N, H), **f32) if getattr(spec, "keep_hidden", False) else None
            readout(x_in, pro[0], pro[1], hout, gslice)
            hnew = hout if hout is not None else ZAct(x_in, pro[0], pro[1])
        saved.append(_LayerSave(h, pooled, lins, aux))
        hidden.append(hnew)
        h = hnew
    return hidden, g_f, saved


class DiscUnit:
    """Hand-over between the discriminator scores' forward, the loss and the backward (round 3).

    With the reference's loss on d_logit -- BCEWithLogits against ones / zeros, main.py:32-37 -- the backward's
    per-graph reductions (dU, s2sum, dsum of gnm_disc_score_bwd) are k x quantities that depend on the FORWARD values
    only, k being the loss's scalar factor times the upstream gradient.  gnm_disc_score_fwd_unit leaves them in `unit`
    from the hidden rows it holds in registers anyway; a loss that knows it has that form (gnm.train.infomax_loss with
    its default targets) records k and the gradient tensor it handed to autograd; GinInfoMaxFn.backward then scales
    `unit` instead of reading the five hidden layers a second time (gnm_disc_du_kernel: 539 MB, ~90 us at B = 1024).
    Any other loss (main.py's torch losses, explicit d_labels, a d_logit that also feeds something else so that
    autograd SUMS gradients into a new tensor) leaves k unset or the pointer different, and the backward runs
    gnm_disc_score_bwd exactly as before."""
    __slots__ = ("unit", "inv_perm", "k", "kscale", "dD_ptr", "dD_version")

    def __init__(self):
        self.unit = self.inv_perm = self.k = self.dD_ptr = self.dD_version = None
        self.kscale = 1.0


class ZAct:
    """A layer output that is not in memory: h = relu(z * scale + shift) (graphcnn.py:163-166) with z the pre-BatchNorm
    output of the layer's last Linear and (scale, shift) its folded BatchNorm.  Its BatchNorm + ReLU ran on the tile
    load of the next layer's aggregation, which did not write it (105 MB per layer at the
    headline shape); the only other consumer, the discriminator, re-forms it in its kernels from the same three
    tensors.  tensor() materialises it for the rare paths that want the array (unfused fallbacks, test hooks)."""
    __slots__ = ("z", "scale", "shift", "_h")

    def __init__(self, z, scale, shift):
        self.z, self.scale, self.shift, self._h = z, scale, shift, None

    @property
    def shape(self):
        return self.z.shape

    def tensor(self):
        if self._h is None:
            self._h = torch.relu(torch.addcmul(self.shift, self.z, self.scale))
        return self._h


def hidden_tensor(h):
    """the [N, H] array of a layer output, whichever way encoder_forward holds it"""
    return h.tensor() if isinstance(h, ZAct) else h


def _ptr_array(tensors):
    return (C.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])


def _hidden_ptr_arrays(hidden):
    """(pointers, scale pointers, shift pointers, leading dimension) for gnm_disc_score_fwd / _bwd: a ZAct layer is
    passed as its z with the BatchNorm vectors, a materialised one as itself (NULL vectors)"""
    n = len(hidden)
    hp, sp, tp = (C.c_void_p * n)(), (C.c_void_p * n)(), (C.c_void_p * n)()
    ld = None
    for l, h in enumerate(hidden):
        if isinstance(h, ZAct):
            hp[l], sp[l], tp[l] = h.z.data_ptr(), h.scale.data_ptr(), h.shift.data_ptr()
            stride = h.z.stride(0)
        else:
            hp[l], sp[l], tp[l] = h.data_ptr(), None, None
            stride = h.stride(0)
        if ld is not None and stride != ld:
            raise GnmError("hidden layers with different leading dimensions (%d, %d)" % (ld, stride))
        ld = stride
    return hp, sp, tp, ld


def eval_fused_ok(spec, batch, X, P, mode=True):
    """can this eval-mode forward run as the one-launch encoder (csrc/evalfwd.hip; mode True) / as one launch per layer
    with a workgroup per 32-row block (csrc/evallayer.hip; mode "layers")?"""
    if spec.n_max or spec.sync_bn is not None or spec.keep_hidden:
        return False
    layers = mode == "layers"
    if not getattr(batch, "has_bits", False) or batch.B < 1 or batch.n_max > (416 if layers else int(lib.gnm_eval_max_nodes())):
        return False
    if spec.n_avg and spec.learn_eps and getattr(batch, "iso", False):
        return False            # the 0/0 row of an isolated node must stay confined to its row (see _dense)
    H = P["batch_norms.0.weight"].shape[0]
    C_ = P["linears_prediction.0.weight"].shape[0]
    if layers:
        return H in (32, 64, 128) and 1 <= spec.m <= 3 and spec.L <= 16 and X.shape[1] <= 128 and C_ <= 256 and X.is_cuda
    return H == 64 and 1 <= spec.m <= 3 and spec.L <= 16 and X.shape[1] <= 64 and C_ <= 64 and X.is_cuda


def check_permutation(perm, B):
    """The Infomax shuffle (graphcnn.py:199: np.random.permutation(B)) as a host int array, validated: the kernels
    scatter its inverse and index rows with it unchecked, so anything that is not a permutation of 0 .. B-1 must stop
    here (round 3 clamped on the device instead and would have trained on wrong gradients)."""
    p = np.asarray(perm)
    if p.ndim != 1 or p.shape[0] != B or p.dtype.kind not in "iu":
        raise GnmError("perm must be %d integers (np.random.permutation(B), graphcnn.py:199); got shape %s dtype %s"
                       % (B, p.shape, p.dtype))
    if B and (int(p.min()) < 0 or int(p.max()) >= B or not bool((np.bincount(p, minlength=B) == 1).all())):
        raise GnmError("perm is not a permutation of 0 .. %d" % (B - 1))
    return p


def perm_to_device(perm, B, dev, out=None):
    """perm -> int32 device tensor (or into the static buffer `out`).  Host permutations are validated and go through
    pinned memory (a pageable copy would stall the host behind everything queued); a CUDA tensor is taken as it is --
    it can only come from a buffer that was filled through this function."""
    if torch.is_tensor(perm) and perm.is_cuda:
        t = perm.to(torch.int32)
        if out is not None and out.data_ptr() != t.data_ptr():
            out.copy_(t, non_blocking=True)
        return t if out is None else out
    host = torch.as_tensor(check_permutation(perm.cpu().numpy() if torch.is_tensor(perm) else perm, B).astype(np.int32))
    if dev.type == "cuda":
        host = host.pin_memory()
    if out is not None:
        out.copy_(host, non_blocking=True)
        return out
    return host.to(dev, non_blocking=True)


def _eval_table(spec, P, dev):
    """The DEVICE table of parameter addresses gnm_eval_encoder / gnm_eval_layers / gnm_occlusion read
    (include/gnm_hip.h), cached on the spec."""
    L, m = spec.L, spec.m
    words = []
    for l in range(L):
        for k in range(m):
            wn = f"mlps.{l}.linear" if m == 1 else f"mlps.{l}.linears.{k}"
            bn = f"batch_norms.{l}" if k == m - 1 else f"mlps.{l}.batch_norms.{k}"
            W = P[wn + ".weight"]
            if W.stride(1) != 1:
                raise GnmError("Linear weights must be row-contiguous")
            words += [W.data_ptr(), P[wn + ".bias"].data_ptr(), P[bn + ".weight"].data_ptr(), P[bn + ".bias"].data_ptr(),
                      P[bn + ".running_mean"].data_ptr(), P[bn + ".running_var"].data_ptr(), W.stride(0)]
    for l in range(L):
        wp, bp = P[f"linears_prediction.{l}.weight"], P[f"linears_prediction.{l}.bias"]
        if not wp.is_contiguous() or not bp.is_contiguous():
            raise GnmError("classifier parameters must be contiguous")
        words += [wp.data_ptr(), bp.data_ptr()]
    assert len(words) == int(lib.gnm_eval_table_words(L, m))
    # the table of parameter addresses lives on the device; rebuilt only when a parameter moved (a few hundred bytes,
    # one pinned asynchronous copy -- capturable)
    key = tuple(words)
    cached = getattr(spec, "_eval_table", None)
    if cached is None or cached[0] != key or cached[1].device != dev:
        host = torch.tensor(words, dtype=torch.int64).pin_memory()
        cached = spec._eval_table = (key, host.to(dev, non_blocking=True), host)
    return cached[1]


def eval_forward_fused(spec, batch, perm, P, X, want_disc, mode=True):
    """GIN_InfoMaxReg.forward in eval() mode (graphcnn.py:194-251 with BatchNorm on its running statistics and dropout
    off) as ONE encoder launch (gnm_eval_encoder: layers + readout + classifier, a workgroup per graph) plus, for the
    Infomax scores, U = sigmoid(g_f) W^T and the score kernel.  No autograd graph: callers use it under no_grad only
    (models/graphcnn.py).  Returns (c_logit, d_logit, g_f) like GinInfoMaxFn."""
    dev = launch_device(X, *[t for t in P.values() if torch.is_tensor(t)][:1])
    L, m = spec.L, spec.m
    N, B = batch.N, batch.B
    H = P["batch_norms.0.weight"].shape[0]
    Cn = P["linears_prediction.0.weight"].shape[0]
    f32 = dict(dtype=torch.float32, device=dev)
    X = X.contiguous()
    table = _eval_table(spec, P, dev)
    hidden_all = torch.empty((L, N, H), **f32)
    hidden = [hidden_all[l] for l in range(L)]
    g_f = torch.empty((B, L * H), **f32)
    c = torch.empty_like(g_f) if want_disc else None
    c_logit = torch.empty((B, Cn), **f32)
    shared = (*batch.bits_ptrs(), batch.node_off.data_ptr(), *batch.deg_ptrs(), B, batch.n_max, X.data_ptr(), X.stride(0),
              X.shape[1], H, L, m, Cn, int(spec.n_avg), int(not spec.learn_eps), int(spec.g_avg), BN_EPS, table.data_ptr(),
              P["eps"].data_ptr() if spec.learn_eps else None, hidden_all.data_ptr(), hidden_all.stride(0), H)
    with _stream_scope(dev):
        outs = (g_f.data_ptr(), g_f.stride(0), ptr(c), c_logit.data_ptr(), c_logit.stride(0), _stream())
        if mode == "layers":
            scratch = torch.empty(int(lib.gnm_eval_layers_scratch_floats(B, batch.n_max, H, L)), **f32)
            check(lib.gnm_eval_layers(*shared, scratch.data_ptr(), *outs), "gnm_eval_layers")
        else:
            s0, s1 = torch.empty((N, H), **f32), torch.empty((N, H), **f32)
            check(lib.gnm_eval_encoder(*shared, s0.data_ptr(), s1.data_ptr(), H, *outs), "gnm_eval_encoder")
        d_logit = torch.zeros((0, 1), **f32)
        if want_disc:
            d_logit = _disc_forward(spec, batch, P, hidden, c, perm, timed=False)[0]
    return c_logit, d_logit, g_f


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


# occlusion_hip's scratch (two [sum n^2, H] activation arrays and the readout shares) stays under this many bytes: the
# source graphs of a batch are run in chunks.  One 416-node graph at H = 128, L = 16 needs 0.22 GB.
OCCLUSION_SCRATCH_BYTES = 2 << 30


def occlusion_hip(spec, batch, X, P, classes, out=None):
    """The eval-mode class scores of every node-deleted copy of every graph of a batch (csrc/occlusion.hip,
    include/gnm_hip.h gnm_occlusion): out[ci, node_off[g] + v] = c_logit[classes[ci]] of graph g without node v.  Per
    batch XW = X W0^T (the split-precision Linear, any input width) and S = (A + I) XW (the CSR gather: one kernel
    whatever the batch's density, so a graph's result does not depend on its batch-mates); then, per chunk of source
    graphs whose scratch fits OCCLUSION_SCRATCH_BYTES, L layer launches and the finish launch.  The shapes
    occlusion_decline takes.  Parameters, buffers and the numpy RNG are not touched; the device parameter table is
    eval_forward_fused's.  Returns a float32 [len(classes), N] tensor (`out` when given)."""
    d = _launch_dims(spec, batch, X, P)
    dev, L, m, N, B, H, Cn, F0, X = d.dev, d.L, d.m, d.N, d.B, d.H, d.Cn, d.F0, d.X
    out = _out_array(out, (len(classes), N), dev)
    cls = (C.c_int * len(classes))(*[int(c) for c in classes])
    offs = np.asarray(batch.node_off_host, dtype=np.int64)
    ns = np.diff(offs)
    sq = np.concatenate([[0], np.cumsum(ns * ns)])          # activation rows before graph g: sum of n^2
    with torch.no_grad(), _stream_scope(dev):
        table = _eval_table(spec, P, dev)
        f32 = dict(dtype=torch.float32, device=dev)
        XW, S = _first_linear_product(X, P, m, N, F0, H), torch.empty((N, H), **f32)
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
                                        XW.stride(0), S[r0:].data_ptr(), S.stride(0), H, L, m, Cn, cls, len(classes),
                                        int(spec.n_avg), int(not spec.learn_eps), int(spec.g_avg), BN_EPS,
                                        table.data_ptr(), d.eps, scratch.data_ptr(), dst.data_ptr(), out.stride(0),
                                        _stream()), "gnm_occlusion")
    return out


def lesion_decline(spec, batch, X, P):
    """None if csrc/lesion.hip takes this batch, else the condition it declines: occlusion_decline's conditions (a
    virtual graph whose NaN stays in its own score is taken; a set leaves at least one node, so a graph needs two)."""
    return occlusion_decline(spec, batch, X, P)


# lesion_hip's scratch (two [sum of n over the virtual graphs, H] activation arrays and the readout shares) stays under
# this many bytes: the virtual graphs of a batch are run in chunks.  8 graphs x 20 sets at n = 400, H = 128: 0.07 GB.
LESION_SCRATCH_BYTES = 2 << 30


def lesion_hip(spec, batch, X, P, classes, removed, vgraph, out=None):
    """The eval-mode class scores of set-deleted copies of the graphs of a batch (csrc/lesion.hip, include/gnm_hip.h
    gnm_lesion): out[ci, q] = c_logit[classes[ci]] of graph vgraph[q] of the batch without the nodes r with
    removed[q, r] != 0.  removed: a host uint8 / bool array [V, >= n_max] (entries past a graph's n are ignored);
    vgraph: V host ints in [0, B).  Per batch XW = X W0^T (the split-precision Linear, any input width); then, per chunk
    of whole virtual graphs whose scratch fits LESION_SCRATCH_BYTES, the mask-packing launch, ONE read-back of the
    kept counts, L layer launches and the finish launch.  The shapes lesion_decline takes.  Parameters, buffers and the
    numpy RNG are not touched; the device parameter table is eval_forward_fused's.  Returns a float32
    [len(classes), V] tensor (`out` when given)."""
    d = _launch_dims(spec, batch, X, P)
    dev, L, m, N, B, H, Cn, F0, X = d.dev, d.L, d.m, d.N, d.B, d.H, d.Cn, d.F0, d.X
    removed = np.ascontiguousarray(np.asarray(removed) != 0, dtype=np.uint8)
    vgraph = np.ascontiguousarray(vgraph, dtype=np.int32)
    Vt = int(vgraph.shape[0])
    nm = int(batch.n_max)
    if removed.ndim != 2 or removed.shape[0] != Vt or removed.shape[1] < nm:
        raise GnmError("removed must be [%d, >= %d], got %s" % (Vt, nm, list(removed.shape)))
    if Vt and (vgraph.min() < 0 or vgraph.max() >= B):
        raise GnmError("vgraph entries must be graphs of the batch, 0 .. %d" % (B - 1))
    out = _out_array(out, (len(classes), Vt), dev)
    cls = (C.c_int * len(classes))(*[int(c) for c in classes])
    offs = np.asarray(batch.node_off_host, dtype=np.int64)
    vn = np.diff(offs)[vgraph].astype(np.int32)             # node count of each virtual graph
    cum = np.concatenate([[0], np.cumsum(vn, dtype=np.int64)])      # activation rows before virtual graph q
    with torch.no_grad(), _stream_scope(dev):
        table = _eval_table(spec, P, dev)
        f32 = dict(dtype=torch.float32, device=dev)
        XW = _first_linear_product(X, P, m, N, F0, H)
        up = batch.arena._upload

        def floats(q0, q1):
            return int(lib.gnm_lesion_scratch_floats(int(cum[q1] - cum[q0]), q1 - q0, int(vn[q0:q1].max()), H, L))
        for q0, q1 in _runs_within(Vt, floats, LESION_SCRATCH_BYTES):
            V, nc = q1 - q0, vn[q0:q1]
            n_max, rows = int(nc.max()), int(cum[q1] - cum[q0])
            mstride = int(lib.gnm_lesion_mask_words(n_max))
            vg = up(torch.as_tensor(vgraph[q0:q1]))
            vrow_off = up(torch.as_tensor(cum[q0:q1] - cum[q0]))
            rem = up(torch.as_tensor(removed[q0:q1]))
            masks = torch.empty((V, mstride), dtype=torch.int32, device=dev)
            kept = torch.empty(V, dtype=torch.int32, device=dev)
            check(lib.gnm_lesion_pack(rem.data_ptr(), rem.stride(0), vg.data_ptr(), batch.node_off.data_ptr(), B,
                                      n_max, V, mstride, masks.data_ptr(), kept.data_ptr(), _stream()),
                  "gnm_lesion_pack")
            kept_host = kept.cpu().numpy()                  # the one read-back of the chunk
            scratch = torch.empty(floats(q0, q1), **f32)
            dst = out[:, q0:q1]
            with _timed("lesion_hip", B=B, N=V, H=H, L=L):
                check(lib.gnm_lesion(batch.arena.bits.buf.data_ptr(), batch.bits_off.data_ptr(),
                                     batch.node_off.data_ptr(), vg.data_ptr(), vrow_off.data_ptr(), masks.data_ptr(),
                                     mstride, kept.data_ptr(), kept_host.ctypes.data, nc.ctypes.data, B, n_max, V,
                                     rows, XW.data_ptr(), XW.stride(0), H, L, m, Cn, cls, len(classes),
                                     int(spec.n_avg), int(not spec.learn_eps), int(spec.g_avg), BN_EPS,
                                     table.data_ptr(), d.eps, scratch.data_ptr(), dst.data_ptr(), out.stride(0),
                                     _stream()), "gnm_lesion")
    return out


# csrc/disconnect.hip takes what csrc/lesion.hip takes, for the same reasons (no node is removed, but the virtual graphs
# run through the same row-block forward): one predicate, one set of strings
disconnect_decline = lesion_decline


def disconnect_hip(spec, batch, X, P, classes, in_a, in_b, vgraph, out=None):
    """The eval-mode class scores of edge-cut copies of the graphs of a batch (csrc/disconnect.hip, include/gnm_hip.h
    gnm_disconnect): out[ci, q] = c_logit[classes[ci]] of graph vgraph[q] of the batch without the edges (u, v) with
    (in_a[q, u] and in_b[q, v]) or (in_b[q, u] and in_a[q, v]); every node and feature row stays.  in_a, in_b: host
    uint8 / bool arrays [V, >= n_max] (entries past a graph's n are ignored); vgraph: V host ints in [0, B).  Per batch
    XW = X W0^T (the split-precision Linear, any input width); then, per chunk of whole virtual graphs whose scratch fits
    LESION_SCRATCH_BYTES, ONE gnm_lesion_pack launch over the chunk's A rows followed by its B rows (the two keep masks),
    L layer launches and the finish launch.  Nothing is read back: the readout runs over n, which the host knows.  The
    shapes disconnect_decline takes.  Parameters, buffers and the numpy RNG are not touched; the device parameter table
    is eval_forward_fused's.  Returns a float32 [len(classes), V] tensor (`out` when given)."""
    d = _launch_dims(spec, batch, X, P)
    dev, L, m, N, B, H, Cn, F0, X = d.dev, d.L, d.m, d.N, d.B, d.H, d.Cn, d.F0, d.X
    in_a = np.ascontiguousarray(np.asarray(in_a) != 0, dtype=np.uint8)
    in_b = np.ascontiguousarray(np.asarray(in_b) != 0, dtype=np.uint8)
    vgraph = np.ascontiguousarray(vgraph, dtype=np.int32)
    Vt = int(vgraph.shape[0])
    nm = int(batch.n_max)
    for name, a in (("in_a", in_a), ("in_b", in_b)):
        if a.ndim != 2 or a.shape[0] != Vt or a.shape[1] < nm:
            raise GnmError("%s must be [%d, >= %d], got %s" % (name, Vt, nm, list(a.shape)))
    if in_a.shape != in_b.shape:
        raise GnmError("in_a and in_b must have one shape, got %s and %s" % (list(in_a.shape), list(in_b.shape)))
    if Vt and (vgraph.min() < 0 or vgraph.max() >= B):
        raise GnmError("vgraph entries must be graphs of the batch, 0 .. %d" % (B - 1))
    out = _out_array(out, (len(classes), Vt), dev)
    cls = (C.c_int * len(classes))(*[int(c) for c in classes])
    offs = np.asarray(batch.node_off_host, dtype=np.int64)
    vn = np.diff(offs)[vgraph].astype(np.int32)             # node count of each virtual graph
    cum = np.concatenate([[0], np.cumsum(vn, dtype=np.int64)])      # activation rows before virtual graph q
    with torch.no_grad(), _stream_scope(dev):
        table = _eval_table(spec, P, dev)
        f32 = dict(dtype=torch.float32, device=dev)
        XW = _first_linear_product(X, P, m, N, F0, H)
        up = batch.arena._upload

        def floats(q0, q1):
            return int(lib.gnm_disconnect_scratch_floats(int(cum[q1] - cum[q0]), q1 - q0, int(vn[q0:q1].max()), H, L))
        for q0, q1 in _runs_within(Vt, floats, LESION_SCRATCH_BYTES):
            V, nc = q1 - q0, np.ascontiguousarray(vn[q0:q1])
            n_max, rows = int(nc.max()), int(cum[q1] - cum[q0])
            mstride = int(lib.gnm_lesion_mask_words(n_max))
            vg2 = up(torch.as_tensor(np.concatenate([vgraph[q0:q1], vgraph[q0:q1]])))       # A's rows, then B's (gnm_disconnect reads the first V)
            vrow_off = up(torch.as_tensor(cum[q0:q1] - cum[q0]))
            rem = up(torch.as_tensor(np.concatenate([in_a[q0:q1], in_b[q0:q1]])))
            kept = up(torch.as_tensor(nc))                  # the readout's divisor: every node stays
            masks = torch.empty((2 * V, mstride), dtype=torch.int32, device=dev)
            counts = torch.empty(2 * V, dtype=torch.int32, device=dev)      # gnm_lesion_pack's kept counts: not used
            check(lib.gnm_lesion_pack(rem.data_ptr(), rem.stride(0), vg2.data_ptr(), batch.node_off.data_ptr(), B,
                                      n_max, 2 * V, mstride, masks.data_ptr(), counts.data_ptr(), _stream()),
                  "gnm_lesion_pack")
            scratch = torch.empty(floats(q0, q1), **f32)
            dst = out[:, q0:q1]
            with _timed("disconnect_hip", B=B, N=V, H=H, L=L):
                check(lib.gnm_disconnect(batch.arena.bits.buf.data_ptr(), batch.bits_off.data_ptr(),
                                         batch.node_off.data_ptr(), vg2.data_ptr(), vrow_off.data_ptr(),
                                         masks.data_ptr(), masks[V:].data_ptr(), mstride, kept.data_ptr(),
                                         nc.ctypes.data, B, n_max, V, rows, XW.data_ptr(), XW.stride(0), H, L, m, Cn,
                                         cls, len(classes), int(spec.n_avg), int(not spec.learn_eps), int(spec.g_avg),
                                         BN_EPS, table.data_ptr(), d.eps, scratch.data_ptr(), dst.data_ptr(),
                                         out.stride(0), _stream()), "gnm_disconnect")
    return out


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

    lesion_hip's chunk loop (whole virtual graphs under LESION_SCRATCH_BYTES, the chunk's scratch bounded through the
    batch's largest graph) with three differences: a virtual graph costs 4 bytes of description (its id; the labels go
    up once per batch) instead of a removed row; the kept counts gnm_lesion checks are computed here from the group
    sizes, so nothing is read back; and a coalition that keeps no node at all is left out of the launch and scored
    sum_l linears_prediction[l].bias[c], added in fp32 in layer order -- the head's score of a zero pooled vector.
    The shapes lesion_decline takes.  Returns a float32 [len(classes), V] tensor (`out` when given)."""
    d = _launch_dims(spec, batch, X, P)
    dev, L, m, N, B, H, Cn, F0, X = d.dev, d.L, d.m, d.N, d.B, d.H, d.Cn, d.F0, d.X
    nm, K = int(batch.n_max), int(K)
    vgraph = np.ascontiguousarray(vgraph, dtype=np.int32)
    ids = np.ascontiguousarray(ids, dtype=np.int64)
    labels = np.asarray(labels)
    Vt = int(vgraph.shape[0])
    if labels.ndim != 2 or labels.shape[0] != B or labels.shape[1] < nm or labels.dtype.kind not in "iu":
        raise GnmError("labels must be an int [%d, >= %d] array, got %s %s" % (B, nm, labels.dtype, list(labels.shape)))
    if ids.shape != (Vt,):
        raise GnmError("ids must be [%d], got %s" % (Vt, list(ids.shape)))
    if Vt and (vgraph.min() < 0 or vgraph.max() >= B):
        raise GnmError("vgraph entries must be graphs of the batch, 0 .. %d" % (B - 1))
    offs = np.asarray(batch.node_off_host, dtype=np.int64)
    ns = np.diff(offs)
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
    cls = (C.c_int * len(classes))(*[int(c) for c in classes])
    run = np.nonzero(kept_all > 0)[0]
    Vr = int(run.shape[0])
    vg_r, ids_r = vgraph[run], ids[run].astype(np.int32)
    kept_r = np.ascontiguousarray(kept_all[run], dtype=np.int32)
    vn = ns[vg_r].astype(np.int32)                          # node count of each virtual graph that runs
    cum = np.concatenate([[0], np.cumsum(vn, dtype=np.int64)])      # activation rows before it
    # gnm_lesion_scratch_floats with the chunk's largest graph bounded by the batch's: a prefix array
    cost = 2 * cum * H + L * np.arange(Vr + 1, dtype=np.int64) * ((nm + 31) // 32) * H
    with torch.no_grad(), _stream_scope(dev):
        res = out if Vr == Vt else torch.empty((len(classes), Vr), dtype=torch.float32, device=dev)
        up = batch.arena._upload
        if Vr:
            table = _eval_table(spec, P, dev)
            XW = _first_linear_product(X, P, m, N, F0, H)
            lab16 = np.full((B, nm), -1, dtype=np.int16)
            lab16[inside] = lab[inside]
            lab_d = up(torch.as_tensor(lab16))              # once per batch
            ranks_d = up(torch.as_tensor(ranks.astype(np.int16))) if ranks is not None else None
        for q0, q1 in _runs_under(cost, LESION_SCRATCH_BYTES // 4):
            V, nc = q1 - q0, np.ascontiguousarray(vn[q0:q1])
            n_max, rows = int(nc.max()), int(cum[q1] - cum[q0])
            mstride = int(lib.gnm_lesion_mask_words(n_max))
            vg = up(torch.as_tensor(vg_r[q0:q1]))
            idd = up(torch.as_tensor(ids_r[q0:q1]))
            vrow_off = up(torch.as_tensor(cum[q0:q1] - cum[q0]))
            masks = torch.empty((V, mstride), dtype=torch.int32, device=dev)
            kept = torch.empty(V, dtype=torch.int32, device=dev)
            check(lib.gnm_coalition_pack(lab_d.data_ptr(), lab_d.stride(0), vg.data_ptr(), idd.data_ptr(),
                                         ranks_d.data_ptr() if ranks is not None else None,
                                         ranks.shape[0] if ranks is not None else 0, K, batch.node_off.data_ptr(), B,
                                         n_max, V, mstride, masks.data_ptr(), kept.data_ptr(), _stream()),
                  "gnm_coalition_pack")
            kept_host = np.ascontiguousarray(kept_r[q0:q1])
            scratch = torch.empty(int(lib.gnm_lesion_scratch_floats(rows, V, n_max, H, L)), dtype=torch.float32,
                                  device=dev)
            dst = res[:, q0:q1]
            with _timed("shapley_hip", B=B, N=V, H=H, L=L):
                check(lib.gnm_lesion(batch.arena.bits.buf.data_ptr(), batch.bits_off.data_ptr(),
                                     batch.node_off.data_ptr(), vg.data_ptr(), vrow_off.data_ptr(), masks.data_ptr(),
                                     mstride, kept.data_ptr(), kept_host.ctypes.data, nc.ctypes.data, B, n_max, V,
                                     rows, XW.data_ptr(), XW.stride(0), H, L, m, Cn, cls, len(classes),
                                     int(spec.n_avg), int(not spec.learn_eps), int(spec.g_avg), BN_EPS,
                                     table.data_ptr(), d.eps, scratch.data_ptr(), dst.data_ptr(), res.stride(0),
                                     _stream()), "gnm_lesion")
        if Vr != Vt:
            # the coalitions that keep no node: the head's score of a zero pooled vector at every layer
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
        eps_ptr = d.eps

        def pooled_product(src, rows):
            """pool(src) W0^T as pool(src W0^T): src is [rows, F0] (the batch's features, or ONE graph's baseline)"""
            XW = _first_linear_product(src, P, m, rows, F0, H)
            if rows != N:
                XW = XW.repeat(B, 1)
            Pz = torch.empty((N, H), **f32)
            _agg(batch, XW, Pz, H, eps_ptr, spec, backward=False)
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
                        table.data_ptr(), eps_ptr, scratch.data_ptr(), vb.t_bits_off.data_ptr(),
                        vb.node_off.data_ptr(), vb.rp_off.data_ptr(), K, wt.data_ptr(), X[r0:].data_ptr(), X.stride(0),
                        ptr(baseline), baseline.stride(0) if baseline is not None else 0,
                        int(baseline.shape[0]) if baseline is not None else 0, dst.data_ptr(), out.stride(1),
                        _stream()), "gnm_integrated_gradients")
            del saved, table, scratch, z0
    return out


class _Grads:
    """The parameter gradients of one backward.  With a sink (spec.grad_sink) the kernels write into its tensors,
    overwriting them, and autograd gets None; without one, into fresh tensors that autograd gets."""

    def __init__(self, sink):
        self.sink, self.fresh = sink, {}

    def out(self, name, like):
        """the tensor a kernel writes gradient `name` into"""
        if self.sink is not None:
            return self.sink[name]
        t = self.fresh[name] = torch.empty_like(like)
        return t

    def put(self, name, value):
        """record a gradient computed by a torch op"""
        if self.sink is not None:
            self.sink[name].copy_(value.reshape(self.sink[name].shape))
        else:
            self.fresh[name] = value

    def result(self, names, needs):
        """one entry per parameter name: its fresh tensor where `needs` asks for one, else None"""
        return tuple(self.fresh.get(name) if need else None for name, need in zip(names, needs))


def _head_forward(spec, P, g_f, H, training, dropout_p, want_c):
    """Classifier head (graphcnn.py:224-231) and c = sigmoid(g_f) (:239, only when want_c): one launch (csrc/head.hip),
    or batched matrix products for shapes outside the kernel.  Returns (c_logit, c, masks, Wp, fused_head, wps)."""
    L, B, dev = spec.L, g_f.shape[0], g_f.device
    wps = [P[f"linears_prediction.{l}.weight"] for l in range(L)]
    bps = [P[f"linears_prediction.{l}.bias"] for l in range(L)]
    Cn = wps[0].shape[0]
    masks = None
    if training and dropout_p > 0:
        # (F.dropout of a cached tensor of ones: the fill it would otherwise need is a launch per step)
        ones = getattr(spec, "_ones_mask", None)
        if ones is None or ones.shape != (L, B, Cn) or ones.device != dev:
            ones = spec._ones_mask = torch.ones((L, B, Cn), dtype=torch.float32, device=dev)
        masks = F.dropout(ones, dropout_p, True)                                                      # :230
    c_logit = torch.empty((B, Cn), dtype=torch.float32, device=dev)
    c = torch.empty_like(g_f) if want_c else None
    fused_head = all(w.is_contiguous() for w in wps) and all(b_.is_contiguous() for b_ in bps)
    if fused_head:
        rc = lib.gnm_head_fwd(g_f.data_ptr(), g_f.stride(0), B, L, H, Cn, _ptr_array(wps), _ptr_array(bps),
                              ptr(masks), c_logit.data_ptr(), c_logit.stride(0), ptr(c),
                              c.stride(0) if c is not None else 0, _stream())
        if rc == -2:
            fused_head = False
        else:
            check(rc, "gnm_head_fwd")
    Wp = None
    if not fused_head:          # shapes outside the head kernel (C > 256 classes): batched matrix products
        Wp = torch.stack(wps)                                                            # [L,C,H]
        G3 = g_f.view(B, L, H).transpose(0, 1)                                           # [L,B,H] view
        lg = torch.baddbmm(torch.stack(bps).unsqueeze(1), G3, Wp.transpose(1, 2))        # [L,B,C]
        if masks is not None:
            lg = lg * masks
        c_logit = lg.sum(0)
        if want_c:
            c = torch.sigmoid(g_f)
    return c_logit, c, masks, Wp, fused_head, wps


def _disc_forward(spec, batch, P, hidden, c, perm, unit=None, timed=True):
    """The Infomax discriminator scores (discriminator.py:20-36 on graphcnn.py:198-201,239-248): U = c W^T, then one
    score kernel over the hidden layers, which also fills the DiscUnit `unit` when given one and the shape allows.
    Returns (d_logit, U, perm_rows, `unit` if it was filled else None)."""
    if not batch.equal_n:
        raise RuntimeError("Discriminator expands each graph summary N//B times (discriminator.py:24): "
                           "all graphs of a batch must have the same number of nodes")
    L, N, B, dev = spec.L, batch.N, batch.B, c.device
    H = hidden[0].shape[1]
    Wd = P["disc.f_k.weight"][0]
    U = torch.empty((B, Wd.shape[0]), dtype=torch.float32, device=dev)
    if not _small_gemm(c, 0, Wd, 0, U, B, Wd.shape[0], Wd.shape[1]):
        U = c @ Wd.t()                                                # U[g] = W c_g
    # row index = perm[g] (:198-201,242): validated on the host, pinned staging + async copy (a device tensor --
    # a captured step's static buffer -- passes as it is: graph-capture safe)
    perm_rows = perm_to_device(perm, B, dev)
    d_logit = torch.empty((2 * N, 1), dtype=torch.float32, device=dev)
    hp_, sp_, tp_, ldh_ = _hidden_ptr_arrays(hidden)
    score_args = (hp_, sp_, tp_, ldh_, L, H, U.data_ptr(), U.stride(0), perm_rows.data_ptr(),
                  P["disc.f_k.bias"].data_ptr(), batch.node_off.data_ptr(), N, B, d_logit.data_ptr())
    disc_unit = None
    with _timed("disc_score" if timed else None, N=N, L=L, H=H):
        rc = -2
        if unit is not None:
            # also leave the backward's per-graph reductions (up to the loss's scalar factor): see DiscUnit
            ldunit = (L * H + 2 + 3) & ~3
            sums = torch.empty((B, ldunit), dtype=torch.float32, device=dev)
            inv_perm = torch.empty(B, dtype=torch.int32, device=dev)
            rc = lib.gnm_disc_score_fwd_unit(*score_args, sums.data_ptr(), ldunit, inv_perm.data_ptr(), _stream())
            if rc == 0:
                unit.unit, unit.inv_perm = sums, inv_perm
                disc_unit = unit
            elif rc != -2:
                check(rc, "gnm_disc_score_fwd_unit")
        if rc == -2:
            check(lib.gnm_disc_score_fwd(*score_args, _stream()), "gnm_disc_score_fwd")
    return d_logit, U, perm_rows, disc_unit


class _Backward:
    """What the stages of one GinInfoMaxFn.backward share: the forward's context, the gradient collector, and what one
    stage leaves for a later one."""

    def __init__(self, ctx):
        self.ctx, self.spec, self.batch, self.P = ctx, ctx.spec, ctx.batch, ctx.P
        self.H, self.st, self.need_dx = ctx.hidden[0].shape[1], _stream(), ctx.needs_input_grad[9]
        self.f32 = dict(dtype=torch.float32, device=ctx.g_f.device)
        self.grads = _Grads(ctx.spec.grad_sink)
        # the discriminator's terms of every layer's gradient (_disc_backward): d sc_1, U, the inverse permutation, s2sum
        self.dsc1 = self.U = self.inv_perm = self.s2sum = None
        self.dph = [None] * ctx.spec.L      # d loss / d (layer l's readout)  (_head_backward)
        self.deps = self.eps_parts = None   # d eps, and its fp64 partials [L, .] from the L aggregation backwards ...
        self.eps_counts = [0] * ctx.spec.L  # ... with how many each wrote: summed by ONE launch at the end
        self.jobs = []                      # the _ReduceJob of every fused Linear backward

    def disc_args(self, l):
        """(d sc_1, layer l's columns of U, its leading dimension, inverse permutation, s2sum) as the kernels that add
        the discriminator's term to a layer's gradient take them; NULLs for l = None or without a discriminator"""
        if l is None or self.dsc1 is None:
            return None, None, 0, None, None
        return (self.dsc1.data_ptr(), self.U[:, l * self.H:(l + 1) * self.H].data_ptr(), self.U.stride(0),
                self.inv_perm.data_ptr(), self.s2sum.data_ptr())


def _disc_backward(s, dD):
    """Discriminator backward (discriminator.py:28-36): the per-graph reductions -- scaled from what the forward left
    (DiscUnit) or by gnm_disc_score_bwd over the hidden layers --, the Bilinear's gradients, and T = d loss /
    d sigmoid(g_f), which it returns.  Leaves the per-node terms in s (disc_args)."""
    ctx, spec, batch, st = s.ctx, s.spec, s.batch, s.st
    L, N, B, H = spec.L, batch.N, batch.B, s.H
    dD = dD.contiguous().view(-1)
    U, c = ctx.U, ctx.c
    dU = torch.empty_like(U)
    s2sum = torch.empty(B, **s.f32)
    dsum = torch.empty(B, **s.f32)
    dbias = None
    hold = ctx.disc_unit
    if (hold is not None and hold.k is not None and hold.dD_ptr == dD.data_ptr()
            and hold.dD_version == dD._version):      # (same tensor AND untouched since the loss wrote it)
        # dD = k (sigmoid(d_logit) - target) came straight from the loss that recorded k: the reductions are k
        # times what the forward left (DiscUnit) -- no second pass over the hidden layers
        inv_perm = hold.inv_perm
        # (the Bilinear bias gradient -- the total of dsum -- comes out of the same launch)
        dbias = s.grads.out("disc.f_k.bias", s.P["disc.f_k.bias"])
        check(lib.gnm_disc_unit_scale(hold.unit.data_ptr(), hold.unit.stride(0), L * H, hold.k.data_ptr(),
                                      float(getattr(hold, "kscale", 1.0)), B,
                                      dU.data_ptr(), dU.stride(0), s2sum.data_ptr(), dsum.data_ptr(),
                                      dbias.data_ptr(), st),
              "gnm_disc_unit_scale")
    else:
        inv_perm = torch.empty(B, dtype=torch.int32, device=U.device)      # inverse permutation, on the device
        hp_, sp_, tp_, ldh_ = _hidden_ptr_arrays(ctx.hidden)
        with _timed("disc_du", N=N, L=L, H=H):
            check(lib.gnm_disc_score_bwd(hp_, sp_, tp_, ldh_, L, H, dD.data_ptr(),
                                         ctx.perm_rows.data_ptr(), batch.node_off.data_ptr(), N, B,
                                         dU.data_ptr(), dU.stride(0), s2sum.data_ptr(), dsum.data_ptr(),
                                         inv_perm.data_ptr(), st), "gnm_disc_score_bwd")
    if hold is not None:
        hold.k = hold.dD_ptr = hold.dD_version = None
    Wd = s.P["disc.f_k.weight"][0]
    dWd = s.grads.out("disc.f_k.weight", s.P["disc.f_k.weight"])[0]       # ([0] of the Bilinear's 3-D parameter)
    if not _small_gemm(dU, 1, c, 1, dWd, dU.shape[1], c.shape[1], B):          # dWd = dU^T c
        torch.mm(dU.t(), c, out=dWd)
    if dbias is None:
        if s.grads.sink is not None:
            torch.sum(dsum, 0, keepdim=True, out=s.grads.sink["disc.f_k.bias"])
        else:
            s.grads.put("disc.f_k.bias", dsum.sum().reshape(1))
    T = torch.empty((B, Wd.shape[1]), **s.f32)
    if not _small_gemm(dU, 0, Wd, 1, T, B, Wd.shape[1], Wd.shape[0]):            # d loss / d sigmoid(g_f) = dU Wd
        T = dU @ Wd
    s.dsc1, s.U, s.inv_perm, s.s2sum = dD, U, inv_perm, s2sum                 # first N entries of dD = d sc_1
    return T


def _head_backward(s, dC, T):
    """Classifier head backward (graphcnn.py:224-231, :239): the classifier gradients and s.dph, d loss / d g_f through
    both the classifier and the sigmoid (T, from _disc_backward) -- one launch, or torch for the forward's fallback."""
    ctx, g_f, grads = s.ctx, s.ctx.g_f, s.grads
    L, B, H = s.spec.L, s.batch.B, s.H
    if ctx.fused_head and (dC is not None or T is not None):
        wps = ctx.wps
        Cn = wps[0].shape[0]
        dCc = dC.contiguous() if dC is not None else torch.zeros((B, Cn), **s.f32)
        dws = [grads.out(f"linears_prediction.{l}.weight", wps[l]) for l in range(L)]
        dbs = [grads.out(f"linears_prediction.{l}.bias", wps[l][:, 0]) for l in range(L)]
        dph_all = torch.empty((B, L * H), **s.f32)
        check(lib.gnm_head_bwd(dCc.data_ptr(), dCc.stride(0), ptr(ctx.masks), g_f.data_ptr(), g_f.stride(0),
                               ptr(ctx.c), ctx.c.stride(0) if ctx.c is not None else 0, ptr(T),
                               T.stride(0) if T is not None else 0, B, L, H, Cn, _ptr_array(wps),
                               _ptr_array(dws), _ptr_array(dbs), dph_all.data_ptr(), dph_all.stride(0), s.st),
              "gnm_head_bwd")
        s.dph = [dph_all[:, l * H:(l + 1) * H] for l in range(L)]
    elif not ctx.fused_head:
        dg_f = T * ctx.c * (1 - ctx.c) if T is not None else None                        # sigmoid backward
        dph_all = None
        G3 = g_f.view(B, L, H).transpose(0, 1)                                           # [L,B,H]
        if dC is not None:
            dlg = dC.unsqueeze(0).expand(L, -1, -1)
            if ctx.masks is not None:
                dlg = dlg * ctx.masks
            dWp = torch.bmm(dlg.transpose(1, 2), G3)                                     # [L,C,H]
            dbp = dlg.sum(1)                                                             # [L,C]
            for l in range(L):
                grads.put(f"linears_prediction.{l}.weight", dWp[l])
                grads.put(f"linears_prediction.{l}.bias", dbp[l])
            if dg_f is not None:
                dph_all = torch.baddbmm(dg_f.view(B, L, H).transpose(0, 1), dlg, ctx.Wp)   # [L,B,H] contiguous
            else:
                dph_all = torch.bmm(dlg, ctx.Wp)
        elif dg_f is not None:
            dph_all = dg_f.view(B, L, H).transpose(0, 1).contiguous()
        s.dph = [dph_all[l] if dph_all is not None else None for l in range(L)]


def _bn_backward_coefs(s, sv, bn, sums, incoming, dp, disc_l):
    """One train/eval BatchNorm + ReLU (mlp.py:48, graphcnn.py:163-166) up to its backward coefficients.  Unless the
    kernel that produced the incoming gradient left `sums` (_BnSums), gnm_bn_relu_bwd_stats forms G = the gradient
    (incoming + the readout's dp + layer disc_l's discriminator term) under the ReLU mask with its sums; then
    gnm_bn_bwd_finalize: d gamma, d beta and dZ = cA (G - m1 - xhat m2).  Returns (G, (cA, m1, m2))."""
    spec, batch, st = s.spec, s.batch, s.st
    N, B, Hk = batch.N, batch.B, sv.H
    if sums is not None:
        G, part, nblk = sums
    else:
        G = torch.empty((N, Hk), **s.f32)
        part = torch.empty((B, 2, Hk), dtype=torch.float64, device=G.device)
        nblk = B
        check(lib.gnm_bn_relu_bwd_stats(
            ptr(incoming), incoming.stride(0) if incoming is not None else 0,
            ptr(dp), dp.stride(0) if dp is not None else 0, int(spec.g_avg), *s.disc_args(disc_l),
            sv.z.data_ptr(), sv.z.stride(0), sv.scale.data_ptr(), sv.shift.data_ptr(), sv.mean.data_ptr(),
            sv.rstd.data_ptr(), 1, G.data_ptr(), G.stride(0), batch.node_off.data_ptr(), B, Hk,
            part.data_ptr(), st), "gnm_bn_relu_bwd_stats")
    gamma = s.P[bn + ".weight"]
    dgamma, dbeta = s.grads.out(bn + ".weight", sv.scale), s.grads.out(bn + ".bias", sv.scale)
    cA, m1, m2 = (torch.empty(Hk, **s.f32) for _ in range(3))
    check(lib.gnm_bn_bwd_finalize(part.data_ptr(), nblk, Hk, N, gamma.data_ptr(), sv.rstd.data_ptr(),
                                  int(s.ctx.training), dgamma.data_ptr(), dbeta.data_ptr(), cA.data_ptr(),
                                  m1.data_ptr(), m2.data_ptr(), st), "gnm_bn_bwd_finalize")
    if spec.sync_bn is not None and s.ctx.training:
        # d gamma / d beta stay LOCAL sums (the gradient all-reduce averages them, as for every other
        # parameter); the two means inside dZ = cA (G - m1 - xhat m2) are over the union batch
        red = part.view(-1, 2, Hk)[:nblk].sum(0, keepdim=True)
        spec.sync_bn.all_reduce(red)
        scratch = torch.empty((2, Hk), **s.f32)
        check(lib.gnm_bn_bwd_finalize(red.data_ptr(), 1, Hk, sv.Ng, gamma.data_ptr(), sv.rstd.data_ptr(), 1,
                                      scratch[0].data_ptr(), scratch[1].data_ptr(), cA.data_ptr(), m1.data_ptr(),
                                      m2.data_ptr(), st), "gnm_bn_bwd_finalize")
    return G, (cA, m1, m2)


def _agg_backward(s, l, dpooled):
    """Layer l's aggregation backward (graphcnn.py:137-161, 173-182 under autograd): d h_{l-1} = A^T (dpooled [/deg]) +
    (1 + eps) dpooled and the partials of d eps[l].  Over a lower layer the fused form also runs pass 1 of that layer's
    outer BatchNorm backward; with no consumer of d h only the d-eps dot product runs.  Returns (d h or None, the
    _BnSums the fused form left or None)."""
    spec, batch, st = s.spec, s.batch, s.st
    N, B = batch.N, batch.B
    h_in, aux = s.ctx.saved[l].h_in, s.ctx.saved[l].aux
    F_l = h_in.shape[1]
    want_dh = l > 0 or s.need_dx
    dh = torch.empty((N, F_l), **s.f32) if want_dh else None
    part = s.eps_parts[l] if spec.learn_eps else None
    eps_ptr = s.P["eps"].data_ptr() + 4 * l if spec.learn_eps else None
    if l > 0 and want_dh and not spec.n_max:
        lo = s.ctx.saved[l - 1].lins[-1]
        dplo = s.dph[l - 1]
        spart = torch.empty((B, 2, F_l), dtype=torch.float64, device=dh.device)
        rc, cnt = agg_launch(batch, "bwd_stats", F_l, (
            dpooled.data_ptr(), dpooled.stride(0), dh.data_ptr(), dh.stride(0), F_l, eps_ptr,
            int(spec.n_avg), int(not spec.learn_eps),
            None, 0,      # h_in is recomputed from lo.z in the epilogue (d eps)
            ptr(part), lo.z.data_ptr(), lo.z.stride(0), lo.scale.data_ptr(), lo.shift.data_ptr(),
            lo.mean.data_ptr(), lo.rstd.data_ptr(), ptr(dplo), dplo.stride(0) if dplo is not None else 0,
            int(spec.g_avg), *s.disc_args(l - 1), spart.data_ptr()), spec, backward=True, stream=st)
        if rc == 0:
            if spec.learn_eps:
                s.eps_counts[l] = cnt
            return dh, _BnSums(dh, spart, B)
    if dh is None:
        # nothing below consumes d h: only d eps[l] = sum dpooled . h is needed -- a flat dot product
        cnt = int(lib.gnm_rowdot_num_partials())
        with _timed("deps_dot_F%d" % F_l, N=N, F=F_l):
            hin_t = hidden_tensor(h_in)
            check(lib.gnm_rowdot_partials(dpooled.data_ptr(), dpooled.stride(0), hin_t.data_ptr(),
                                          hin_t.stride(0), N, F_l, part.data_ptr(), st),
                  "gnm_rowdot_partials")
    elif spec.n_max:
        cnt = _max_bwd(batch, dpooled, dh, F_l, eps_ptr, aux, hidden_tensor(h_in) if spec.learn_eps else None, part)
    else:
        cnt = _agg(batch, dpooled, dh, F_l, eps_ptr, spec, backward=True,
                   hfwd=hidden_tensor(h_in) if spec.learn_eps else None, deps_partial=part)
    if spec.learn_eps:
        s.eps_counts[l] = cnt
    return dh, None


def _reduce_deferred(s):
    """The reductions nothing in the backward waits for, after its last kernel: the dW / db partials of the fused
    Linear backwards (gnm_reduce_partials_multi, 32 jobs per launch) and the d eps partials (gnm_sum_partials_multi)."""
    L, N = s.spec.L, s.batch.N
    for j0 in range(0, len(s.jobs), 32):
        jb = s.jobs[j0:j0 + 32]
        nj = len(jb)
        check(lib.gnm_reduce_partials_multi(
            (C.c_void_p * nj)(*[j.ws.data_ptr() for j in jb]), (C.c_void_p * nj)(*[j.dW.data_ptr() for j in jb]),
            (C.c_int * nj)(*[j.dW.stride(0) for j in jb]), (C.c_void_p * nj)(*[j.db.data_ptr() for j in jb]),
            (C.c_int * nj)(*[j.H for j in jb]), (C.c_int * nj)(*[j.K for j in jb]), nj, N, s.st),
            "gnm_reduce_partials_multi")
    if s.spec.learn_eps:
        # layers whose aggregation backward did not run (no incoming gradient) have count 0 -> d eps = 0
        check(lib.gnm_sum_partials_multi(s.eps_parts.data_ptr(), s.eps_parts.stride(0), (C.c_int * L)(*s.eps_counts), L,
                                         s.deps.data_ptr(), s.st), "gnm_sum_partials_multi")


class GinInfoMaxFn(torch.autograd.Function):
    """(P0, X, *params) -> (c_logit [B,C], d_logit [2N,1], g_f [B,L*H])."""

    @staticmethod
    def forward(ctx, spec, batch, perm, names, buffers, training, dropout_p, want_disc, P0, X, *tensors):
        dev = launch_device(X, P0, *tensors)
        adev = batch.arena.device
        if adev.type != "cuda" or (adev.index is not None and adev.index != dev.index):
            raise GnmError("the batch's graph arena lives on %s, the model on %s" % (adev, dev))
        ctx.set_materialize_grads(False)
        with _stream_scope(dev):
            return GinInfoMaxFn._forward(ctx, spec, batch, perm, names, buffers, training, dropout_p, want_disc, P0,
                                         X, tensors)

    @staticmethod
    def _forward(ctx, spec, batch, perm, names, buffers, training, dropout_p, want_disc, P0, X, tensors):
        P = {**dict(zip(names, tensors)), **buffers}
        X = X.contiguous()
        hidden, g_f, saved = encoder_forward(spec, batch, X, P, training, update_running=training, P0=P0)
        c_logit, c, masks, Wp, fused_head, wps = _head_forward(spec, P, g_f, hidden[0].shape[1], training, dropout_p,
                                                               want_disc)
        d_logit, U, perm_rows, disc_unit = torch.zeros((0, 1), dtype=torch.float32, device=X.device), None, None, None
        if want_disc:
            d_logit, U, perm_rows, disc_unit = _disc_forward(
                spec, batch, P, hidden, c, perm, want_disc if training and isinstance(want_disc, DiscUnit) else None)
        ctx.spec, ctx.batch, ctx.names, ctx.P, ctx.training, ctx.X = spec, batch, names, P, training, X
        ctx.hidden, ctx.saved, ctx.g_f, ctx.masks, ctx.Wp = hidden, saved, g_f, masks, Wp
        ctx.fused_head, ctx.wps = fused_head, wps
        ctx.c, ctx.U, ctx.perm_rows, ctx.perm, ctx.disc_unit = c, U, perm_rows, perm, disc_unit
        ctx.mark_non_differentiable(g_f)
        return c_logit, d_logit, g_f

    @staticmethod
    def backward(ctx, dC, dD, _dgf):
        with _stream_scope(ctx.g_f.device):
            return GinInfoMaxFn._backward(ctx, dC, dD)

    @staticmethod
    def _backward(ctx, dC, dD):
        s = _Backward(ctx)
        spec, batch, P, grads = s.spec, s.batch, s.P, s.grads
        L, m, N = spec.L, spec.m, batch.N
        T = _disc_backward(s, dD) if dD is not None and ctx.U is not None else None
        _head_backward(s, dC, T)
        if spec.learn_eps:
            s.deps = grads.out("eps", P["eps"])
            eps_stride = max([agg_partials_capacity(batch, sv.h_in.shape[1]) for sv in ctx.saved] +
                             [int(lib.gnm_rowdot_num_partials())])
            s.eps_parts = torch.empty((L, eps_stride), dtype=torch.float64, device=ctx.g_f.device)
        dh = None           # the gradient arriving at the BatchNorm + ReLU in turn, from the layer or the Linear above ...
        sums = None         # ... and that BatchNorm's _BnSums when the kernel that produced the gradient took them
        for l in reversed(range(L)):
            lins = ctx.saved[l].lins
            for k in reversed(range(m)):
                sv, last = lins[k], k == m - 1
                bn = f"batch_norms.{l}" if last else f"mlps.{l}.batch_norms.{k}"
                G, coef = _bn_backward_coefs(s, sv, bn, sums, dh, s.dph[l] if last else None, l if last else None)
                wname = f"mlps.{l}.linear" if m == 1 else f"mlps.{l}.linears.{k}"
                W = P[wname + ".weight"]
                dW, db = grads.out(wname + ".weight", W), grads.out(wname + ".bias", sv.scale)
                # dX of this Linear: always for inner Linears; for the first one only when the
                # aggregation backward below has a consumer (a lower layer, dX, or d eps[l])
                need_dA = k > 0 or l > 0 or s.need_dx or spec.learn_eps
                r = linear_bwd_launch(sv, lins[k - 1] if k > 0 else None, G, coef, W, P[wname + ".bias"], dW, db,
                                      need_dA, N, s.st)
                if r.job is not None:
                    s.jobs.append(r.job)
                dh, sums = r.dA, r.lo_sums
            if dh is not None:
                dh, sums = _agg_backward(s, l, dh)
        _reduce_deferred(s)
        return (None,) * 9 + (dh if s.need_dx else None,) + grads.result(ctx.names, ctx.needs_input_grad[10:])
