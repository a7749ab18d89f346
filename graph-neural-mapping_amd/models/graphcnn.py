"""GIN_InfoMaxReg on MI355X: the reference's model interface over the HIP hot path.

Drop-in for /root/reference models/graphcnn.py (class at :12, constructor :13, forward
:194, compute_saliency :254): `from models.graphcnn import *` in the reference's main.py
(main.py:9) resolves to this file when main.py is run from graph-neural-mapping_amd/.
Constructor arguments, submodule names / creation order (=> identical seeded init and
state_dict keys), numpy-RNG consumption (one np.random.permutation(B) per forward,
graphcnn.py:199), return values and error behaviour follow the reference.

What differs is how the work is done: graphs are converted once to a device-resident CSR
arena (gnm/arena.py), and everything from `X_concat` on runs in libgnm_hip.so through one
autograd.Function with a hand-written backward (gnm/core.py).  There is no CPU or eager
fallback -- on a CPU device forward() raises.  neighbor_pooling_type == "max" (outside
BASELINE.json's north_star) runs through the same engine with
csrc/maxpool.hip in place of the aggregation kernels (gnm/maxnb.py builds its neighbour
lists from graph.neighbors, as graphcnn.py:55-81 does); only the hipGraph replays and the
layer-0 cache are not offered for it.
"""
import contextlib
import functools
import os
import sys

import numpy as np
import torch
import torch.nn as nn

_HERE = os.path.dirname(os.path.abspath(__file__))
_PKG = os.path.dirname(_HERE)
for _p in (_PKG, _HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from mlp import MLP  # noqa: E402
from discriminator import Discriminator  # noqa: E402
from gnm.arena import GraphArena  # noqa: E402
from gnm.core import DiscUnit, GinInfoMaxFn, GinSpec, eval_forward_fused, eval_fused_ok, launch_device  # noqa: E402
from gnm.attribution import (class_activation_hip, disconnect_decline, disconnect_hip, edge_saliency_hip,  # noqa: E402
                             integrated_gradients_hip, lesion_decline, lesion_hip, occlusion_decline, occlusion_hip,
                             saliency_decline, saliency_hip, saliency_maps_hip, shapley_exact_hip, shapley_hip,
                             shapley_permutation_hip)
from gnm import shapley as shapley_host  # noqa: E402
from gnm.intgrad import quadrature  # noqa: E402
from gnm.lesion import curve_area, default_fractions, masks_from_ranking, pair_sets  # noqa: E402

__all__ = ["GIN_InfoMaxReg", "GraphCNN", "MLP", "Discriminator"]


def _as_np(v):
    """a tensor (detached, on the host) or anything array-like as a numpy array"""
    return v.detach().cpu().numpy() if torch.is_tensor(v) else np.asarray(v)


def _nonfinite_graphs(batch, X):
    """None when every feature of the batch is finite, else per graph whether it has a non-finite feature (numpy)"""
    if bool(torch.isfinite(X).all()):
        return None
    counts = torch.as_tensor(np.diff(batch.node_off_host), device=X.device)
    gid = torch.repeat_interleave(torch.arange(batch.B, device=X.device), counts)
    return torch.zeros(batch.B, dtype=torch.int32, device=X.device).index_add_(
        0, gid, (~torch.isfinite(X).all(1)).to(torch.int32)).cpu().numpy() > 0


class _LazyEvalGrad(torch.autograd.Function):
    """Outputs of a replayed eval forward, attached to the parameters: backward() recomputes the forward eagerly
    (same graphs, same permutation) and differentiates that.  Nobody in the reference backpropagates through an
    eval-mode forward; this only keeps doing so correct."""

    @staticmethod
    def forward(ctx, model, gh, perm, c_logit, d_logit, *params):
        ctx.model, ctx.gh, ctx.perm = model, gh, perm
        return c_logit.view_as(c_logit), d_logit.view_as(d_logit)

    @staticmethod
    def backward(ctx, dC, dD):
        m = ctx.model
        names, tensors, _ = m._param_lists()
        with torch.enable_grad():
            batch = m.arena().batch_from_gids(ctx.gh)
            X, P0 = batch.arena.features_and_agg0(batch, m._spec.n_avg, not m._spec.learn_eps)
            sink, m._spec.grad_sink = m._spec.grad_sink, None          # plain autograd gradients here
            try:
                c, d, _ = m._run(batch, X, ctx.perm, want_disc=True, P0=P0, allow_fused=False)
                outs, gouts = [], []
                for o, g in ((c, dC), (d, dD)):
                    if g is not None:
                        outs.append(o)
                        gouts.append(g)
                req = [t for t in tensors if t.requires_grad]
                grads = torch.autograd.grad(outs, req, gouts, allow_unused=True)
            finally:
                m._spec.grad_sink = sink
        it = iter(grads)
        return (None, None, None, None, None) + tuple(next(it) if t.requires_grad else None for t in tensors)


class _LazyEvalGradBatch(torch.autograd.Function):
    """Outputs of an eval-mode forward that ran on the evaluation encoder (no autograd graph), attached to the
    parameters like _LazyEvalGrad: backward() runs the differentiable forward on the same batch and differentiates that."""

    @staticmethod
    def forward(ctx, model, batch, X, P0, perm, c_logit, d_logit, *params):
        ctx.model, ctx.batch, ctx.X, ctx.P0, ctx.perm = model, batch, X, P0, perm
        return c_logit.view_as(c_logit), d_logit.view_as(d_logit)

    @staticmethod
    def backward(ctx, dC, dD):
        m = ctx.model
        names, tensors, _ = m._param_lists()
        with torch.enable_grad():
            sink, m._spec.grad_sink = m._spec.grad_sink, None          # plain autograd gradients here
            try:
                c, d, _ = m._run(ctx.batch, ctx.X, ctx.perm, want_disc=True, P0=ctx.P0, allow_fused=False)
                outs, gouts = [], []
                for o, g in ((c, dC), (d, dD)):
                    if g is not None and o.requires_grad:
                        outs.append(o)
                        gouts.append(g)
                req = [t for t in tensors if t.requires_grad]
                grads = torch.autograd.grad(outs, req, gouts, allow_unused=True) if outs else [None] * len(req)
            finally:
                m._spec.grad_sink = sink
        it = iter(grads)
        return (None,) * 7 + tuple(next(it) if t.requires_grad else None for t in tensors)


class _TrainReplayFn(torch.autograd.Function):
    """A train-mode forward replayed from a captured hipGraph (gnm/graphs.py CapturedTrain), attached to the parameters
    so that the caller's loss.backward() replays the captured backward.  Outputs are copies (the static buffers belong
    to the next replay)."""

    @staticmethod
    def forward(ctx, cap, gh, perm, *params):
        c_logit, d_logit = cap.forward(gh, perm)
        ctx.cap = cap
        # The capture's activations belong to THIS forward until its backward has run.  `hold` lives exactly as long as
        # this autograd node -- i.e. while either output or anything computed from them is alive (a weak reference to
        # c_logit alone, as in round 3, let `_, d = model(b)` look finished) -- and the generation number lets backward
        # prove that no later replay has overwritten them.
        ctx.gen, ctx.hold = cap.claim()
        ctx.set_materialize_grads(False)
        return c_logit.clone(), d_logit.clone()

    @staticmethod
    def backward(ctx, dC, dD):
        if ctx.gen != ctx.cap.gen:
            raise RuntimeError("train replay: the captured activations of this forward were overwritten by a later "
                               "forward before its backward ran (generation %d, now %d); set model.train_replay = False "
                               "for this pattern" % (ctx.gen, ctx.cap.gen))
        return (None, None, None) + tuple(ctx.cap.backward(dC, dD))


class GIN_InfoMaxReg(nn.Module):
    def __init__(self, num_layers, num_mlp_layers, input_dim, hidden_dim, output_dim, final_dropout, learn_eps,
                 graph_pooling_type, neighbor_pooling_type, device):
        super().__init__()
        self._check_kernel_limits(num_layers, input_dim, hidden_dim)
        # creation order follows graphcnn.py:29-52 so torch.manual_seed(s) yields the same weights
        self.disc = Discriminator(hidden_dim * num_layers)
        self.sigm = nn.Sigmoid()
        self.relu = nn.ReLU()
        self.final_dropout = final_dropout
        self.device = device
        self.num_layers = num_layers
        self.num_mlp_layers = num_mlp_layers
        self.graph_pooling_type = graph_pooling_type
        self.neighbor_pooling_type = neighbor_pooling_type
        self.learn_eps = learn_eps
        self.eps = nn.Parameter(torch.zeros(num_layers))
        self.mlps = nn.ModuleList()
        self.batch_norms = nn.ModuleList()
        self.linears_prediction = nn.ModuleList()
        for layer in range(num_layers):
            self.mlps.append(MLP(num_mlp_layers, input_dim if layer == 0 else hidden_dim, hidden_dim, hidden_dim))
            self.batch_norms.append(nn.BatchNorm1d(hidden_dim))
            self.linears_prediction.append(nn.Linear(hidden_dim, output_dim))
        self._spec = GinSpec(num_layers, num_mlp_layers, learn_eps, graph_pooling_type, neighbor_pooling_type)
        self._arena = None
        self._plist = None
        # eval-mode forwards of small batches are replayed from captured hipGraphs (gnm/graphs.py CapturedEval):
        # {(B, n): CapturedEval}, a few entries; eval_replay = False turns it off
        self.eval_replay = True
        self._eval_cache = {}
        # train-mode forwards (and their backwards) of small batches are replayed too (gnm/graphs.py CapturedTrain):
        # what makes the reference's own loop (main.py:19-47, batch 32) GPU-bound instead of launch-bound.
        # train_replay = False turns it off
        self.train_replay = True
        self._train_cache = {}
        # eval_fused = True: eval-mode forwards under torch.no_grad() (incl. the replayed ones) run the L layers as ONE
        # encoder launch, a workgroup per graph (csrc/evalfwd.hip), when the shape allows.  Off by default: measured
        # at one 400-node graph per forward it is SLOWER than the replayed layer-by-layer kernels (0.245 vs 0.188 ms per
        # graph, gpurun_out/r03i_time_eval.log) -- one CU runs a graph's whole chain (MFMA floor ~57 us + 50 barriers)
        # where the ~110 replayed launches (~1.4 us apiece) each spread over several CUs.  DESIGN.md section 6.
        # eval_fused = "layers": one launch per LAYER with a workgroup per 32-row block of every graph
        # (csrc/evallayer.hip): 13 CUs work on a 400-node graph, ~10 launches per forward.  0.130 ms per graph -- the
        # default.  False: the training kernels in eval mode.
        self.eval_fused = "layers"

    @staticmethod
    def _check_kernel_limits(num_layers, input_dim, hidden_dim):
        """Shapes the HIP kernels are built for (narrower than the reference, which takes anything torch does):
        said here, at construction, rather than as GNM_ERR_BAD_ARG from the first forward."""
        from gnm._cabi import lib
        if hidden_dim < 4 or hidden_dim > 128 or hidden_dim % 4:
            raise ValueError("hidden_dim=%d: the MI355X kernels take a multiple of 4 in [4, 128] (BatchNorm / Linear "
                             "column tiles; csrc/norm.hip, csrc/linear.hip)" % hidden_dim)
        if num_layers < 1 or num_layers > 16:
            raise ValueError("num_layers=%d: 1..16 GIN layers are supported (csrc/disc.hip GNM_MAX_LAYERS)" % num_layers)
        kmax = int(lib.gnm_linear_max_k(hidden_dim))
        if input_dim < 1 or input_dim > kmax:
            raise ValueError("input_dim=%d with hidden_dim=%d: the first Linear keeps its [input_dim x hidden_dim] "
                             "weight in LDS, which bounds input_dim to %d (csrc/linear.hip)"
                             % (input_dim, hidden_dim, kmax))

    # ------------------------------------------------------------------ plumbing
    def arena(self):
        """Device-resident graph store; created lazily on the parameters' device."""
        dev = self.eps.device
        if self._arena is None or self._arena.device != dev:
            self._arena = GraphArena(dev)
        return self._arena

    def _apply(self, fn, *args, **kwargs):
        # .to() / .cuda() / .float() may replace buffer tensors: drop the cached lists and captured graphs
        self._plist = None
        self._eval_cache = {}
        self._train_cache = {}
        return super()._apply(fn, *args, **kwargs)

    def _param_lists(self):
        """(names, parameters, buffers) in state_dict order, cached: walking the module
        tree on every forward costs ~0.4 ms of Python."""
        pl = getattr(self, "_plist", None)
        if pl is None:
            names, tensors = zip(*self.named_parameters())
            pl = self._plist = (names, tensors, dict(self.named_buffers()))
        return pl

    def _named_tensors(self):
        """{name: tensor} over _param_lists()' parameters and buffers: the P the eval-mode drivers of gnm/ read"""
        names, tensors, buffers = self._param_lists()
        P = dict(zip(names, tensors))
        P.update(buffers)
        return P

    @contextlib.contextmanager
    def _eval_mode(self):
        """eval mode (BatchNorm on its running statistics, no dropout), the previous mode restored on exit"""
        was_training = self.training
        self.eval()
        try:
            yield
        finally:
            self.train(was_training)

    def _run(self, batch, X, perm, want_disc, P0=None, hand_over=True, allow_fused=True):
        names, tensors, buffers = self._param_lists()
        if (allow_fused and not self.training and self.eval_fused and not X.requires_grad
                and not (P0 is not None and P0.requires_grad)):
            # evaluation (the replayed eval forward, callers under torch.no_grad(), and -- so that every eval-mode
            # forward of a model gives the same bits -- callers in grad mode too): the evaluation encoder
            # (csrc/evallayer.hip / csrc/evalfwd.hip) instead of ~20 training-kernel launches per layer.  It records
            # no autograd graph; in grad mode the outputs are attached lazily (_LazyEvalGradBatch), as the reference's
            # eval outputs carry one (main.py:54 detaches them).  Saliency (X.requires_grad) takes the path below.
            P = self._named_tensors()
            if eval_fused_ok(self._spec, batch, X, P, self.eval_fused):
                with torch.no_grad():
                    c_logit, d_logit, g_f = eval_forward_fused(self._spec, batch, perm, P, X, want_disc, self.eval_fused)
                if torch.is_grad_enabled() and any(t.requires_grad for t in tensors):
                    c_logit, d_logit = _LazyEvalGradBatch.apply(self, batch, X, P0, perm, c_logit, d_logit, *tensors)
                return c_logit, d_logit, g_f
        hold = None
        if want_disc and self.training and hand_over and torch.is_grad_enabled():
            # let the score kernel leave the backward's reductions for the reference's BCE loss (gnm/core.py DiscUnit);
            # only a loss that recognises the hand-over on d_logit (gnm.train.infomax_loss) makes use of it
            hold = want_disc = DiscUnit()
        out = GinInfoMaxFn.apply(self._spec, batch, perm, names, buffers, self.training, float(self.final_dropout),
                                 want_disc, P0, X, *tensors)
        if hold is not None and hold.unit is not None:
            out[1]._gnm_disc_unit = hold
        return out

    def forward_batch(self, batch, X=None, perm=None, latent=False):
        """forward() for an already assembled gnm.arena.Batch (what bench.py and the
        data-parallel driver call: no per-graph Python work)."""
        if perm is None:
            perm = np.random.permutation(batch.B)                             # graphcnn.py:199
        P0 = None
        if X is None and self._spec.n_max:
            X = batch.arena.features(batch)
        elif X is None:
            # layer 0's A X [/deg] does not depend on the parameters: gathered from the arena's per-graph cache
            X, P0 = batch.arena.features_and_agg0(batch, self._spec.n_avg, not self._spec.learn_eps)
        c_logit, d_logit, g_f = self._run(batch, X, perm, want_disc=True, P0=P0)
        if latent:
            return g_f.detach().cpu().numpy()                                  # graphcnn.py:248-249
        return c_logit, d_logit

    @torch.no_grad()
    def predict(self, graphs, batch_size=256, latent=False):
        """Evaluation over many graphs in batches (not in the reference: its test() / get_latent_space() call
        forward([g]) once per graph, main.py:49-57,71-82, which is launch-bound).  Eval mode -- BatchNorm uses its
        running statistics, so batching does not change a graph's result.  Returns c_logit [len(graphs), C], or
        the [len(graphs), L*H] latent array when latent=True.  Graphs of a batch must have equal node counts
        (discriminator.py:24), as in forward()."""
        with self._eval_mode():
            out = []
            for i in range(0, len(graphs), batch_size):
                chunk = graphs[i:i + batch_size]
                r = self.forward(chunk, latent=latent)
                out.append(r if latent else r[0])
            if latent:
                return np.concatenate(out, 0) if out else np.zeros((0, 0), dtype=np.float32)
            return torch.cat(out, 0) if out else torch.zeros((0, 0), device=self.eps.device)

    def saliency(self, graphs, cls, batch_size=256):
        """Input saliency of many graphs in batches: what main.py:60-68 builds from one compute_saliency([g], c) call
        per graph and class (not in the reference).  Eval mode -- BatchNorm on its running statistics, no dropout --
        so graphs do not interact and a batch gives each graph's per-graph result (to fp32 rounding).

        cls: an int, or a sequence of ints such as (0, 1); the forward pass of a batch is shared by all of them.
        Returns a float32 device tensor [len(graphs), n, F0] for an int `cls` and [len(cls), len(graphs), n, F0] for a
        sequence -- np.stack of compute_saliency's results.  Graphs of different node counts are allowed (no
        discriminator is involved); the result is then a list of [n_g, F0] tensors (a list of such lists for a
        sequence `cls`).

        Unlike compute_saliency, which leaves the model in eval mode and zeroes and then fills every parameter's .grad,
        this computes only the input gradient: no .grad is touched, BatchNorm buffers and the numpy RNG are left alone,
        and the model's train / eval mode is restored on exit.  The route each batch took ("hip": csrc/saliency.hip;
        "autograd": the whole batch differentiated through GinInfoMaxFn, for shapes the kernel declines -- max
        neighbour pooling, graphs over 416 nodes or without a bit adjacency, H outside {32, 64, 128}, ...) is left in
        self.saliency_routes.  A graph with a non-finite feature takes the autograd route on its own (one more
        "autograd" entry), so its NaN / inf pattern is compute_saliency's."""
        F0 = self.mlps[0].linear.in_features if self.num_mlp_layers == 1 else self.mlps[0].linears[0].in_features
        routes = []
        out = self._interpret(graphs, *self._interpret_args("saliency", graphs, cls, batch_size), batch_size, (F0,),
                              functools.partial(self._saliency_batch, routes=routes))
        self.saliency_routes = routes
        return out

    def _interpret_args(self, name, graphs, cls, batch_size):
        """The argument checks every batched attribution method shares (`name` prefixes the errors): (whether cls is
        one int, the classes as a list)"""
        single = isinstance(cls, (int, np.integer))
        classes = [int(cls)] if single else [int(c) for c in cls]
        n_cls = self.linears_prediction[0].out_features
        if len(graphs) == 0:
            raise ValueError("%s: empty list of graphs" % name)
        if not classes:
            raise ValueError("%s: empty sequence of classes" % name)
        for c in classes:
            if not 0 <= c < n_cls:
                raise ValueError("%s: class %d out of range for a %d-class model" % (name, c, n_cls))
        if batch_size < 1:
            raise ValueError("%s: batch_size must be positive" % name)
        return single, classes

    def _interpret(self, graphs, single, classes, batch_size, tail, run_batch, square=False):
        """The batching saliency(), class_activation() and edge_saliency() share, after _interpret_args (which gives
        `single` and `classes`): eval mode with the previous mode restored on exit, chunks of batch_size graphs, and the
        result layout.  run_batch(chunk, batch, P, classes, dst) returns one batch's [len(classes), N, *tail] result
        (or a list of per-class [N, *tail] tensors), written into dst when that is given: the batch's view of the dense
        [len(classes), len(graphs), n, *tail] result.  Graphs of different node counts get per-graph lists instead;
        square: an [n, n] map per graph (tail (n,), each graph's map cropped to its n_g columns)."""
        with self._eval_mode():
            P = self._named_tensors()
            ns = [len(g.g) for g in graphs]
            ragged = any(k != ns[0] for k in ns)
            if square:
                tail = (ns[0],)
            full = None if ragged else torch.empty((len(classes), len(graphs), ns[0]) + tail, dtype=torch.float32,
                                                   device=self.eps.device)
            per_graph = [[] for _ in classes]
            for i0 in range(0, len(graphs), batch_size):
                chunk = graphs[i0:i0 + batch_size]
                batch = self._batch_of(chunk)
                if full is not None:
                    run_batch(chunk, batch, P, classes, full[:, i0:i0 + len(chunk)].view(len(classes), -1, *tail))
                    continue
                res = run_batch(chunk, batch, P, classes, None)
                offs = np.asarray(batch.node_off_host)
                for ci in range(len(classes)):
                    per_graph[ci] += [res[ci][offs[j]:offs[j + 1], :offs[j + 1] - offs[j]] if square
                                      else res[ci][offs[j]:offs[j + 1]] for j in range(len(chunk))]
            if full is not None:
                return full[0] if single else full
            return per_graph[0] if single else per_graph

    def _saliency_batch(self, chunk, batch, P, classes, dst, routes):
        """saliency() of one batch: a list of [N, F0] tensors (written into dst when given), one per class"""
        X = batch.arena.features(batch)
        if saliency_decline(self._spec, batch, X, P, dx=True) is not None:
            routes.append("autograd")
            res = self._saliency_autograd(batch, classes)
        else:
            bad = _nonfinite_graphs(batch, X)
            if bad is None:
                routes.append("hip")
                return saliency_hip(self._spec, batch, X.detach(), P, classes, outs=dst)
            # a graph with a non-finite feature: its saliency is whatever compute_saliency's backward makes of the
            # NaN / inf (the kernel's masks would quietly turn it into zeros), so such a graph takes the autograd route
            # on its own -- exactly compute_saliency's kernels -- and the others stay on the kernel
            B = batch.B
            parts = [None] * B
            good = [j for j in range(B) if not bad[j]]
            if good:
                sub = self._batch_of([chunk[j] for j in good])
                routes.append("hip")
                r = saliency_hip(self._spec, sub, sub.arena.features(sub).detach(), P, classes)
                for k, j in enumerate(good):
                    parts[j] = [x[sub.node_off_host[k]:sub.node_off_host[k + 1]] for x in r]
            for j in range(B):
                if bad[j]:
                    routes.append("autograd")
                    parts[j] = self._saliency_autograd(self._batch_of([chunk[j]]), classes)
            res = [torch.cat([parts[j][ci] for j in range(B)], 0) for ci in range(len(classes))]
        if dst is not None:
            for d, r in zip(dst, res):
                d.copy_(r)
        return res

    def _saliency_autograd(self, batch, classes):
        """saliency()'s route for every shape csrc/saliency.hip declines: d score[:, c] / d X of the whole batch through
        GinInfoMaxFn's backward (exact: graphs are independent in eval mode), one forward per class.  torch.autograd.grad
        with inputs=X leaves every parameter's .grad alone; a gradient sink (data-parallel training) is set aside."""
        sink, self._spec.grad_sink = self._spec.grad_sink, None
        try:
            out = []
            for c in classes:
                X = batch.arena.features(batch).detach().requires_grad_()
                with torch.enable_grad():
                    score, _, _ = self._run(batch, X, np.arange(batch.B, dtype=np.int64), want_disc=False)
                    seed = torch.zeros_like(score)
                    seed[:, c] = 1
                    (g,) = torch.autograd.grad(score, X, seed)
                out.append(g)
            return out
        finally:
            self._spec.grad_sink = sink

    CAM_KINDS = ("activation", "gradient")

    def class_activation(self, graphs, cls, kind="activation", batch_size=256):
        """Per-node class activation maps of many graphs in batches: the two [n] vectors compute_saliency allocates
        (graphcnn.py:284,288-289) and never fills, plotted as method 'cam' by evaluate/visualize_saliency.py:33.  Eval
        mode -- BatchNorm on its running statistics, no dropout -- so a batch gives each graph's per-graph result.

        kind="activation" (class_activation): cam[v] = p_g sum_l <h_l[v], linears_prediction[l].weight[c]>, p_g = 1 for
        sum graph pooling and the fp32 1/n_g for average; sum_v cam[v] + sum_l linears_prediction[l].bias[c] is the eval
        logit.  Every neighbour pooling and graph size the forward takes (csrc/cam.hip).
        kind="gradient" (grad_class_activation): gcam[v] = sum_l <d score_c / d h_l[v], h_l[v]>, the full gradient at
        h_l -- the h.grad compute_saliency([g], c) leaves on its retained hidden_rep[l] (csrc/saliency.hip,
        gnm_saliency_maps).  The shapes saliency()'s kernel takes; any other batch raises ValueError naming the
        condition (max pooling, n > 416 or no bit adjacency, hidden_dim not in {32, 64, 128}, average pooling with
        learned eps and an isolated node).  A graph with a non-finite feature gets an all-NaN map.

        cls: an int, or a sequence of ints; one forward per batch serves all of them.  Returns a float32 device tensor
        [len(graphs), n] for an int `cls` and [len(cls), len(graphs), n] for a sequence; for graphs of different node
        counts a list of [n_g] tensors (a list of such lists for a sequence `cls`).  No parameter .grad, BatchNorm
        buffer or numpy RNG state is touched, and the train / eval mode is restored on exit."""
        if kind not in self.CAM_KINDS:
            raise ValueError("class_activation: kind must be one of %s, not %r" % (self.CAM_KINDS, kind))
        return self._interpret(graphs, *self._interpret_args("class_activation", graphs, cls, batch_size), batch_size, (),
                               functools.partial(self._cam_batch, kind=kind))

    def _cam_batch(self, chunk, batch, P, classes, dst, kind):
        """class_activation() of one batch: [len(classes), N] (dst when given)"""
        X = batch.arena.features(batch).detach()
        launch_device(X, P["eps"])                          # no CPU fallback: GnmError before any shape question
        if kind == "activation":
            return class_activation_hip(self._spec, batch, X, P, classes, out=dst)
        why = saliency_decline(self._spec, batch, X, P, dx=False)
        if why is not None:
            raise ValueError("class_activation(kind='gradient') does not cover this batch: %s" % why)
        bad = _nonfinite_graphs(batch, X)
        if bad is None:
            return saliency_maps_hip(self._spec, batch, X, P, classes, out=dst)
        return self._clean_graphs_apart(chunk, batch, bad, dst, (len(classes), batch.N),
                                        lambda sub, Xs: saliency_maps_hip(self._spec, sub, Xs, P, classes))

    def edge_saliency(self, graphs, cls, batch_size=64):
        """Connectivity saliency of many graphs in batches: which CONNECTION matters for a class.  For graph g with n
        nodes, out[u, v] = d score_c / d A[u, v] for ALL u, v < n, A the dense form of the reference's Adj_block
        (graphcnn.py:84-106: 1 at every edge_mat pair, row u = destination, plus the diagonal when learn_eps is False),
        which every layer's aggregation multiplies by and, under neighbour "average", also divides by (degree = A 1).
        score_c is compute_saliency's eval logit (BatchNorm on running statistics, no dropout).  Entries where A is 0
        are the sensitivity to adding that connection -- what a leaf adjacency's .grad holds in torch.

        csrc/edgesal.hip over gnm_saliency's layer launches (include/gnm_hip.h gnm_edge_saliency).  The shapes
        class_activation(kind="gradient") takes; any other batch raises ValueError naming the condition (max pooling,
        n > 416 or no bit adjacency, hidden_dim not in {32, 64, 128}, average pooling with learned eps and an isolated
        node, ...).  A graph with a non-finite feature gets an all-NaN map.

        cls: an int, or a sequence of ints; one forward per batch serves all of them.  Returns a float32 device tensor
        [len(graphs), n, n] for an int `cls` and [len(cls), len(graphs), n, n] for a sequence; for graphs of different
        node counts a list of [n_g, n_g] tensors (a list of such lists for a sequence `cls`).  The output is n^2 per
        graph and class, hence the smaller default batch.  No parameter .grad, BatchNorm buffer or numpy RNG state is
        touched, and the train / eval mode is restored on exit."""
        return self._interpret(graphs, *self._interpret_args("edge_saliency", graphs, cls, batch_size), batch_size, (),
                               self._edge_saliency_batch, square=True)

    def _edge_saliency_batch(self, chunk, batch, P, classes, dst):
        """edge_saliency() of one batch: [len(classes), N, n_max] (dst when given)"""
        X = batch.arena.features(batch).detach()
        launch_device(X, P["eps"])                          # no CPU fallback: GnmError before any shape question
        why = saliency_decline(self._spec, batch, X, P, dx=False)
        if why is not None:
            raise ValueError("edge_saliency does not cover this batch: %s" % why)
        bad = _nonfinite_graphs(batch, X)
        if bad is None:
            return edge_saliency_hip(self._spec, batch, X, P, classes, out=dst)
        return self._clean_graphs_apart(chunk, batch, bad, dst, (len(classes), batch.N, batch.n_max),
                                        lambda sub, Xs: edge_saliency_hip(self._spec, sub, Xs, P, classes))

    def occlusion(self, graphs, cls, batch_size=8, return_scores=False):
        """Per-ROI occlusion maps (virtual lesioning) of many graphs in batches: how far the class score moves when a
        node is taken out of the graph -- the fidelity check of the gradient maps above.  With G \\ v the graph without
        node v (the node, its feature row and its edges in both directions removed; the other nodes keep their feature
        rows) and score_c the eval logit c_logit[:, c] of forward() (BatchNorm on its running statistics, no dropout;
        the readout over n - 1 nodes, graph "average" with the fp32 1/(n - 1), neighbour "average" by the reduced
        graph's own degree, self loops kept):

            occluded[c, g, v] = score_c(G_g \\ v),   base[c, g] = score_c(G_g),   delta = base - occluded  (fp32)

        a positive delta: the ROI supports the class.  No copy of a graph is built: csrc/occlusion.hip runs every
        (graph, deleted node) pair as a virtual graph over the source graph's bit adjacency (include/gnm_hip.h
        gnm_occlusion); base is the model's ordinary eval forward.  delta is a difference of two nearly equal numbers,
        so accuracy is a statement about base and occluded (return_scores=True returns (delta, base, occluded)).

        cls: an int, or a sequence of ints; one pass per batch serves all of them.  Returns a float32 device tensor
        [len(graphs), n] for an int `cls` and [len(cls), len(graphs), n] for a sequence; for graphs of different node
        counts a list of [n_g] tensors (a list of such lists for a sequence `cls`), as class_activation() lays them out.
        base: [len(graphs)] / [len(cls), len(graphs)].

        If G \\ v leaves a node without neighbours under neighbour "average" with learned eps, the reference's 0/0 row
        makes that score NaN: occluded[:, g, v] is NaN and no other entry is.  A graph with a non-finite feature gets
        an all-NaN map; its batch-mates are unaffected.  The shapes class_activation(kind="gradient") takes, at any
        input width the model is built with; any other batch raises ValueError naming the condition (max pooling,
        n > 416 or no bit adjacency, hidden_dim not in {32, 64, 128}, num_mlp_layers outside 1..3, more than 16 layers,
        synchronised BatchNorm), and so does a graph of fewer than 2 nodes.

        The n deleted copies of an n-node graph need 2 n^2 hidden_dim floats of scratch: the default batch_size keeps a
        batch of 400-node graphs at hidden_dim 128 under 2 GiB (8 x 0.16 GiB + the readout shares), and a larger batch
        is run in chunks under that budget (gnm/attribution.py OCCLUSION_SCRATCH_BYTES).  The result is bitwise the same
        run to run and for any batch_size.  No parameter .grad, BatchNorm buffer or numpy RNG state is touched, and the
        train / eval mode is restored on exit."""
        for g in graphs:
            if len(g.g) < 2:
                raise ValueError("occlusion: a graph of fewer than 2 nodes has no node-deleted copy")
        bases = []
        single, classes = self._interpret_args("occlusion", graphs, cls, batch_size)
        occ = self._interpret(graphs, single, classes, batch_size, (),
                              functools.partial(self._occlusion_batch, bases=bases))
        base = torch.cat(bases, 1)                          # [len(classes), len(graphs)]
        if single:
            base = base[0]
        if torch.is_tensor(occ):
            delta = base.unsqueeze(-1) - occ
        elif single:
            delta = [base[j] - o for j, o in enumerate(occ)]
        else:
            delta = [[base[ci, j] - o for j, o in enumerate(row)] for ci, row in enumerate(occ)]
        return (delta, base, occ) if return_scores else delta

    def _virtual_prologue(self, method, decline, batch, P, classes):
        """What occlusion() and lesion() do first with a batch: its features on the device, ValueError(`method` ...) if
        decline(...) declines it, and its base scores [len(classes), B] from the ordinary eval forward"""
        X = batch.arena.features(batch).detach()
        launch_device(X, P["eps"])                          # no CPU fallback: GnmError before any shape question
        why = decline(self._spec, batch, X, P)
        if why is not None:
            raise ValueError("%s does not cover this batch: %s" % (method, why))
        with torch.no_grad():
            c_logit, _, _ = self._run(batch, X, np.arange(batch.B, dtype=np.int64), want_disc=False)
        return X, c_logit.detach()[:, classes].t().contiguous()

    def _occlusion_batch(self, chunk, batch, P, classes, dst, bases):
        """occlusion() of one batch: the occluded scores [len(classes), N] (dst when given); the batch's base scores
        [len(classes), B] are appended to `bases`"""
        X, base = self._virtual_prologue("occlusion", occlusion_decline, batch, P, classes)
        bases.append(base)
        bad = _nonfinite_graphs(batch, X)
        if bad is None:
            return occlusion_hip(self._spec, batch, X, P, classes, out=dst)
        return self._clean_graphs_apart(chunk, batch, bad, dst, (len(classes), batch.N),
                                        lambda sub, Xs: occlusion_hip(self._spec, sub, Xs, P, classes))

    def lesion(self, graphs, cls, rois, batch_size=8, return_scores=False):
        """Virtual lesions of ROI SETS of many graphs in batches: how far the class score moves when a whole set of
        nodes -- a resting-state network, a hemisphere, the top of an attribution map -- is taken out of the graph.
        occlusion()'s contract with the node replaced by a set D, 0 <= |D| <= n - 1 (the nodes of D, their feature rows
        and their edges in both directions removed; the other rows unchanged; the readout over n - |D| nodes, graph
        "average" with the fp32 1/(n - |D|), neighbour "average" by the reduced graph's own degree, self loops kept):

            lesioned[c, g, s] = score_c(G_g \\ D_s),   base[c, g] = score_c(G_g),   delta = base - lesioned  (fp32)

        rois (True / 1 = removed): ONE bool or 0/1 array or tensor [S, n] applied to every graph, which then all have n
        nodes, or a list of len(graphs) arrays [S_g, n_g].  No copy of a graph is built: csrc/lesion.hip runs every
        (graph, set) pair as a virtual graph over the source graph's bit adjacency under a keep mask (include/gnm_hip.h
        gnm_lesion); base is the model's ordinary eval forward.  The empty set is taken (lesioned = the kernel's score
        of the whole graph, base to fp32 rounding).

        cls: an int, or a sequence of ints; one pass per batch serves all of them.  Returns a float32 device tensor
        [len(graphs), S] for an int `cls` and [len(cls), len(graphs), S] for a sequence; when the S_g differ a list
        of [S_g] tensors (a list of such lists for a sequence `cls`).  return_scores=True returns
        (delta, base, lesioned), base [len(graphs)] / [len(cls), len(graphs)].

        If G \\ D leaves a kept node without neighbours under neighbour "average" with learned eps, the reference's
        0/0 row makes that score NaN: lesioned[:, g, s] is NaN and no other entry is.  A graph with a non-finite
        feature gets all-NaN results and its batch-mates run as a clean batch (a stated deviation: the explicit copy
        would be clean if the bad row were in D).  The shapes occlusion() takes; any other batch raises ValueError
        naming the condition, as do a set that removes every node of its graph, a mask of the wrong width or with an
        entry other than 0 / 1, and a shared mask over graphs of different node counts.

        The result is bitwise the same run to run, for any batch_size and whatever other sets share the call (no
        atomics, fixed summation orders, one virtual graph per workgroup column).  A virtual graph needs 2 n
        hidden_dim floats of scratch; the virtual graphs of a batch run in chunks under gnm/attribution.py
        LESION_SCRATCH_BYTES.  No parameter .grad, BatchNorm buffer or numpy RNG state is touched, and the
        train / eval mode is restored on exit."""
        single, classes = self._interpret_args("lesion", graphs, cls, batch_size)
        sets = self._lesion_sets(graphs, rois)
        return self._set_scores(graphs, single, classes, batch_size, [int(s.shape[0]) for s in sets], return_scores,
                                lambda chunk, batch, P, i0: self._lesion_batch(chunk, batch, P, classes,
                                                                               sets[i0:i0 + len(chunk)]))

    def _set_scores(self, graphs, single, classes, batch_size, counts, return_scores, run_batch):
        """The batching and the result layout lesion() and disconnect() share: eval mode with the previous mode restored
        on exit, chunks of batch_size graphs -- run_batch(chunk, batch, P, i0) returns (base [len(classes), B], scores
        [len(classes), sum of S_g over the chunk]) of the chunk that starts at graph i0 -- then delta = base - scores
        as a [.., len(graphs), S] tensor when every graph has S = counts[g] sets and as per-graph lists otherwise."""
        with self._eval_mode():
            P = self._named_tensors()
            bases, parts = [], []
            for i0 in range(0, len(graphs), batch_size):
                chunk = graphs[i0:i0 + batch_size]
                base, les = run_batch(chunk, self._batch_of(chunk), P, i0)
                bases.append(base)
                parts.append(les)
        base = torch.cat(bases, 1)                          # [len(classes), len(graphs)]
        flat = torch.cat(parts, 1)                          # [len(classes), sum of S_g]
        if all(k == counts[0] for k in counts):
            les = flat.view(len(classes), len(graphs), counts[0])
            delta = base.unsqueeze(-1) - les
            if single:
                delta, base, les = delta[0], base[0], les[0]
        else:
            les = [list(torch.split(row, counts)) for row in flat]
            delta = [[base[ci, j] - o for j, o in enumerate(row)] for ci, row in enumerate(les)]
            if single:
                delta, base, les = delta[0], base[0], les[0]
        return (delta, base, les) if return_scores else delta

    @staticmethod
    def _shared_mask(rois):
        """whether `rois` is ONE [S, n] mask for all graphs (an array, a tensor or nested rows), not a per-graph list"""
        return torch.is_tensor(rois) or isinstance(rois, np.ndarray) or (
            isinstance(rois, (list, tuple)) and len(rois) > 0 and np.ndim(rois[0]) == 1 and not torch.is_tensor(rois[0]))

    @staticmethod
    def _shared_labels(labels):
        """whether `labels` is ONE [n] labelling for all graphs (an array, a tensor or a flat sequence), not a per-graph
        list"""
        return torch.is_tensor(labels) or isinstance(labels, np.ndarray) or (
            isinstance(labels, (list, tuple)) and len(labels) > 0 and np.ndim(labels[0]) == 0)

    @staticmethod
    def _lesion_sets(graphs, rois, method="lesion", name="rois", proper=True):
        """lesion()'s `rois` (disconnect()'s `a` / `b`: `method`, `name`) as one bool [S_g, n_g] array per graph,
        checked; proper: a set must leave a node of its graph (a lesion; a cut may name every node)"""
        def as_mask(a, what):
            a = _as_np(a)
            if a.ndim != 2:
                raise ValueError("%s: %s must be a 2-D [sets, nodes] array, got shape %s" % (method, what, list(a.shape)))
            if a.dtype != np.bool_:
                if a.dtype.kind not in "iuf" or not np.isin(a, (0, 1)).all():
                    raise ValueError("%s: %s must be bool or hold only 0 and 1" % (method, what))
                a = a != 0
            return a
        ns = [len(g.g) for g in graphs]
        if GIN_InfoMaxReg._shared_mask(rois):
            a = as_mask(rois, name)
            if any(k != ns[0] for k in ns):
                raise ValueError("%s: a shared [S, n] mask needs graphs of one node count" % method)
            sets = [a] * len(graphs)
        else:
            if not isinstance(rois, (list, tuple)) or len(rois) != len(graphs):
                raise ValueError("%s: %s must be one [S, n] array or a list of one [S_g, n_g] array per graph"
                                 % (method, name))
            sets = [as_mask(a, "%s[%d]" % (name, j)) for j, a in enumerate(rois)]
        for j, (a, n) in enumerate(zip(sets, ns)):
            if n < 2:
                raise ValueError("%s: a graph of fewer than 2 nodes has no %s copy"
                                 % (method, "lesioned" if proper else "edge-cut"))
            if a.shape[1] != n:
                raise ValueError("%s: the mask of graph %d is %d wide for a %d-node graph" % (method, j, a.shape[1], n))
            if proper and a.shape[0] and a.all(1).any():
                raise ValueError("%s: a set removes every node of graph %d" % (method, j))
        return sets

    @staticmethod
    def _stacked_sets(sets, which, nm):
        """The sets of graphs `which` of a chunk (bool [S_j, n_j] each), graph by graph, as the rows of one uint8
        [sum of S_j, nm] array, and the row's graph as its position in `which` (int32): the virtual graphs of a batch"""
        rows = np.zeros((sum(sets[j].shape[0] for j in which), nm), dtype=np.uint8)
        vgraph = np.concatenate([np.full(sets[j].shape[0], k, dtype=np.int32) for k, j in enumerate(which)])
        q = 0
        for j in which:
            s = sets[j]
            rows[q:q + s.shape[0], :s.shape[1]] = s
            q += s.shape[0]
        return rows, vgraph

    def _lesion_batch(self, chunk, batch, P, classes, sets):
        """lesion() of one batch: (base [len(classes), B], lesioned [len(classes), sum of S_g], graph by graph)"""
        def run(b, Xb, which):
            """the virtual graphs of graphs `which` of the chunk, which are the graphs of batch b, in order"""
            removed, vgraph = self._stacked_sets(sets, which, int(b.n_max))
            return lesion_hip(self._spec, b, Xb, P, classes, removed, vgraph)
        return self._sets_batch("lesion", lesion_decline, chunk, batch, P, classes,
                                [sets[j].shape[0] for j in range(batch.B)], run)

    def _sets_batch(self, method, decline, chunk, batch, P, classes, cnt, run):
        """One batch of lesion() / disconnect(): (base [len(classes), B], scores [len(classes), sum of cnt], graph by
        graph) with graph j's cnt[j] virtual graphs from run(batch, X, which) -- see _lesion_batch"""
        X, base = self._virtual_prologue(method, decline, batch, P, classes)
        bad = _nonfinite_graphs(batch, X)
        if bad is None:
            return base, run(batch, X, list(range(batch.B)))
        # a graph with a non-finite feature: all-NaN results; the others run as a batch of their own
        out = torch.full((len(classes), sum(cnt)), float("nan"), dtype=torch.float32, device=self.eps.device)
        good = [j for j in range(batch.B) if not bad[j]]
        if good:
            sub = self._batch_of([chunk[j] for j in good])
            r = run(sub, sub.arena.features(sub).detach(), good)
            starts = np.concatenate([[0], np.cumsum(cnt)])
            q = 0
            for j in good:
                out[:, starts[j]:starts[j] + cnt[j]] = r[:, q:q + cnt[j]]
                q += cnt[j]
        return base, out

    def deletion_curve(self, graphs, cls, ranking, fractions=None, order="descending", batch_size=8):
        """The deletion curve of a per-ROI attribution map, the standard fidelity figure for comparing attribution
        methods: the class score as the top-ranked 5 %, 10 %, ... of ROIs are lesioned, and the curve's area.

        ranking: a [len(graphs), n] array or tensor, or a list of per-graph [n_g] vectors -- any per-ROI map, such as
        occlusion()'s delta or a row-reduced saliency().  Per graph the nodes are sorted by it (a stable sort, ties to
        the lower index; order "descending" removes the highest-ranked first, "ascending" the lowest first -- read
        backwards, the insertion curve) and point k lesions the first min(n - 1, floor(fractions[k] n)) of them
        (gnm/lesion.py masks_from_ranking).  fractions: numbers in [0, 1], default 0, 0.05, ..., 0.95.

        Returns (scores, area): scores [len(graphs), K] for an int `cls` and [len(cls), len(graphs), K] for a
        sequence, float32 on the device -- lesion()'s `lesioned` on those sets, bitwise -- and area [len(graphs)] /
        [len(cls), len(graphs)], fp64 numpy: the trapezoid rule over the realised fractions count / n divided by their
        span (gnm/lesion.py curve_area), the mean score along the curve.  A faithful map gives a descending curve that
        falls fast: a small area.  A non-finite ranking value, a fraction outside [0, 1], an empty fraction list and a
        ranking of the wrong length raise ValueError; otherwise as lesion()."""
        self._interpret_args("deletion_curve", graphs, cls, batch_size)
        fr = default_fractions() if fractions is None else np.asarray(fractions, dtype=np.float64).reshape(-1)
        if fr.shape[0] == 0:
            raise ValueError("deletion_curve: empty list of fractions")
        if torch.is_tensor(ranking):
            ranking = ranking.detach().cpu().numpy()
        elif not isinstance(ranking, np.ndarray):
            ranking = [r.detach().cpu().numpy() if torch.is_tensor(r) else np.asarray(r) for r in ranking]
        if len(ranking) != len(graphs):
            raise ValueError("deletion_curve: %d rankings for %d graphs" % (len(ranking), len(graphs)))
        masks, counts = masks_from_ranking(ranking, fr, order)
        _, _, scores = self.lesion(graphs, cls, masks, batch_size=batch_size, return_scores=True)
        realised = np.stack([c / float(len(g.g)) for c, g in zip(counts, graphs)])       # [G, K]
        return scores, curve_area(scores.cpu().numpy(), realised)

    def disconnect(self, graphs, cls, a, b=None, batch_size=8, return_scores=False):
        """Virtual disconnection of ROI-SET PAIRS of many graphs in batches: how far the class score moves when the
        connections between two sets of nodes -- two resting-state networks, the hemispheres -- are cut; the
        perturbation check of edge_saliency(), as occlusion() / lesion() are of the node maps.  With G (/) (A, B) the
        graph G without every edge (u, v) of edge_mat for which (u in A and v in B) or (u in B and v in A) -- ALL n
        nodes, all feature rows and every other edge untouched -- and score_c the eval logit of lesion():

            disconnected[c, g, s] = score_c(G_g (/) (A_s, B_s)),   base[c, g] = score_c(G_g),
            delta = base - disconnected  (fp32)

        The readout runs over all n nodes (graph "average": the fp32 1/n); neighbour "average" divides by the cut
        graph's own degree.  The self loop added when learn_eps is off is not an edge and is never cut; an explicit
        (v, v) edge is cut when v is in A and in B.  The rule is symmetric, so directed graphs need no special case and
        disconnect(a, b) is disconnect(b, a).  b=None means b = a: the connections INSIDE each set.  Empty sets (an empty
        cut) and sets holding every node (A = B = all: the edgeless graph) are taken.

        a, b (True / 1 = in the set): lesion()'s forms of `rois` -- ONE bool or 0/1 array or tensor [S, n] applied to
        every graph, which then all have n nodes, or a list of len(graphs) arrays [S_g, n_g] -- agreeing in form and
        shape.  No copy of a graph is built: csrc/disconnect.hip runs every (graph, pair) as a virtual graph over the
        source graph's bit adjacency under a keep mask chosen per row (include/gnm_hip.h gnm_disconnect); base is the
        model's ordinary eval forward.  gnm/lesion.py cut_edge_counts gives the number of edges a cut removes, which a
        delta is to be read against.

        cls, the result shapes, return_scores (-> (delta, base, disconnected)), the declined shapes (ValueError naming
        the condition, through lesion()'s predicate) and the policy for a non-finite feature (all-NaN results for that
        graph, its batch-mates run as a clean batch) are lesion()'s.  If a cut leaves a node without neighbours under
        neighbour "average" with learned eps, the reference's 0/0 row makes that score NaN: disconnected[:, g, s] is NaN
        and no other entry is.  A mask of the wrong width or with an entry other than 0 / 1, a and b of different
        shapes and a shared mask over graphs of different node counts raise ValueError.

        The result is bitwise the same run to run, for any batch_size, any chunking (gnm/attribution.py
        LESION_SCRATCH_BYTES) and whatever other pairs share the call.  No parameter .grad, BatchNorm buffer or numpy
        RNG state is touched, and the train / eval mode is restored on exit."""
        single, classes = self._interpret_args("disconnect", graphs, cls, batch_size)
        sa = self._lesion_sets(graphs, a, "disconnect", "a", proper=False)
        if b is None:
            sb = sa
        else:
            if self._shared_mask(a) != self._shared_mask(b):
                raise ValueError("disconnect: a and b must take one form, one [S, n] array or a list of per-graph arrays")
            sb = self._lesion_sets(graphs, b, "disconnect", "b", proper=False)
            for j, (x, y) in enumerate(zip(sa, sb)):
                if x.shape != y.shape:
                    raise ValueError("disconnect: a and b of graph %d have shapes %s and %s"
                                     % (j, list(x.shape), list(y.shape)))
        return self._set_scores(graphs, single, classes, batch_size, [int(s.shape[0]) for s in sa], return_scores,
                                lambda chunk, batch, P, i0: self._disconnect_batch(
                                    chunk, batch, P, classes, sa[i0:i0 + len(chunk)], sb[i0:i0 + len(chunk)]))

    def _disconnect_batch(self, chunk, batch, P, classes, sa, sb):
        """disconnect() of one batch: (base [len(classes), B], disconnected [len(classes), sum of S_g], graph by graph)"""
        def run(bt, Xb, which):
            """the virtual graphs of graphs `which` of the chunk, which are the graphs of batch bt, in order"""
            in_a, vgraph = self._stacked_sets(sa, which, int(bt.n_max))
            in_b, _ = self._stacked_sets(sb, which, int(bt.n_max))
            return disconnect_hip(self._spec, bt, Xb, P, classes, in_a, in_b, vgraph)
        return self._sets_batch("disconnect", disconnect_decline, chunk, batch, P, classes,
                                [sa[j].shape[0] for j in range(batch.B)], run)

    def disconnection_matrix(self, graphs, cls, labels, batch_size=8, return_scores=False):
        """The network-by-network disconnection matrix: disconnect() on every unordered pair of the networks of a
        labelling.  labels: ONE int [n] vector for all graphs (which then all have n nodes) or a list of per-graph
        [n_g] vectors; entry r is the network id of node r in 0 .. K - 1, or -1 for no network; K is the largest id
        over all graphs + 1.  The K (K + 1) / 2 pairs (p <= q) with A = network p, B = network q (gnm/lesion.py
        pair_sets) run in ONE disconnect() call, and delta is scattered into a symmetric float32 device tensor
        [len(graphs), K, K] for an int `cls` ([len(cls), len(graphs), K, K] for a sequence): entry (p, q) = (q, p) is the
        score lost by cutting networks p and q apart, entry (p, p) by cutting the connections inside network p.
        return_scores=True returns (delta, base, scores), scores laid out as delta -- bitwise disconnect()'s values
        for those pairs.  A network without nodes in a graph gives an empty cut.  Otherwise as disconnect()."""
        self._interpret_args("disconnection_matrix", graphs, cls, batch_size)
        shared = self._shared_labels(labels)
        per = [_as_np(labels)] if shared else [_as_np(v) for v in labels]
        if not shared and len(per) != len(graphs):
            raise ValueError("disconnection_matrix: %d label vectors for %d graphs" % (len(per), len(graphs)))
        for v in per:
            if v.ndim != 1 or v.dtype.kind not in "iu":
                raise ValueError("disconnection_matrix: labels must be int [n] vectors, got dtype %s shape %s"
                                 % (v.dtype, list(v.shape)))
        K = max([int(v.max()) + 1 for v in per if v.size] + [0])
        if K < 1:
            raise ValueError("disconnection_matrix: the labels name no network")
        try:
            sets = [pair_sets(v, K) for v in per]
        except ValueError as e:
            raise ValueError("disconnection_matrix: %s" % e) from None
        pairs = sets[0][2]
        a, b = (sets[0][0], sets[0][1]) if shared else ([s[0] for s in sets], [s[1] for s in sets])
        delta, base, scores = self.disconnect(graphs, cls, a, b, batch_size=batch_size, return_scores=True)
        p, q = torch.as_tensor(pairs[:, 0], device=delta.device), torch.as_tensor(pairs[:, 1], device=delta.device)

        def square(flat):
            mat = flat.new_empty(flat.shape[:-1] + (K, K))
            mat[..., p, q] = flat
            mat[..., q, p] = flat
            return mat
        delta = square(delta)
        return (delta, base, square(scores)) if return_scores else delta

    def shapley(self, graphs, cls, labels, method="exact", permutations=None, seed=0, interactions=False, batch_size=8,
                return_scores=False):
        """Shapley values of the ROI networks of a labelling: the average loss of the class score when a network is
        lesioned, over all orders of removal -- the figures that, unlike one lesion() per network, add up and do not
        depend on which other networks are still present.

        labels: as disconnection_matrix() -- ONE int [n] vector for all graphs (which then all have n nodes) or a list
        of per-graph [n_g] vectors; entry r is the group of node r in 0 .. K - 1, or -1 for BACKGROUND, a node of no
        group that is never removed; K is the largest id over all graphs + 1.  The players are the K groups.  For a
        coalition S of them, v_c(g, S) = score_c(G_g without every labelled node whose group is not in S): lesion()'s
        contract on that set (rows and edges removed, the readout over the kept nodes, the reduced graph's own degrees,
        0/0 NaN), so v(N) is the kernel's score of the whole graph.  A coalition that keeps no node at all (no
        background, every group of S empty in the graph) is not run: its value is sum_l linears_prediction[l].bias[c],
        added in fp32 in layer order, the head's score of a zero pooled vector -- the reference's own value under graph
        "sum" pooling, a stated deviation under "average" (0/0 there).

        method="exact" (K <= 16): all 2^K coalitions per graph.  Returns phi, an fp64 device tensor [len(graphs), K] for
        an int `cls` and [len(cls), len(graphs), K] for a sequence,
            phi[c, g, i] = sum over S in N \\ {i} of (v(S + i) - v(S)) / (K C(K - 1, |S|)),
        with sum_i phi_i = v(N) - v(empty).  interactions=True returns (phi, inter), inter [.., K, K] fp64 the Shapley
        interaction index sum over S in N \\ {i, j} of (v(S+ij) - v(S+i) - v(S+j) + v(S)) / ((K - 1) C(K - 2, |S|)):
        symmetric, zero diagonal -- the principled counterpart of disconnection_matrix().  return_scores=True appends
        values, float32 [.., len(graphs), 2^K]: entry id is the coalition whose bit p says group p is present, bitwise
        lesion()'s score of that set.

        method="permutation": sampled Shapley values for larger K, up to one player per node (labels = arange(n) gives
        per-ROI values).  permutations: an int M -- M rows np.random.default_rng(seed).permutation(K), the numpy global
        RNG untouched -- or an explicit int [M, K] array of permutations; the same rows serve every graph.  Each row
        contributes v(its prefix through i) - v(its prefix before i) to player i.  Returns (phi, stderr): the fp64 mean
        over the M rows and std(ddof=1) / sqrt(M) (NaN at M = 1).  v(empty) and v(N) are scored once per graph.
        interactions=True raises; return_scores=True appends values [.., len(graphs), M, K + 1], entry (m, j) the score
        with the first j players of row m present.

        No copy of a graph and no mask is built on the host: a coalition is 4 bytes (csrc/shapley.hip
        gnm_coalition_pack writes lesion()'s keep masks on the device), the forward is lesion()'s kernels unchanged, and
        the scores are combined on the device in fp64 from the fp32 scores -- differences first, fixed summation
        orders, no atomics (gnm_shapley_exact / gnm_shapley_permutation; gnm/shapley.py restates them in numpy).  The
        results are bitwise the same run to run, for any batch_size, any chunking (gnm/attribution.py
        LESION_SCRATCH_BYTES) and any set of classes.  A group with no node in a graph has phi exactly 0.0 there (and a
        zero inter row) wherever the graph's scores are finite.

        NaN: every coalition enters every player's sum, so ONE NaN coalition score makes that graph's phi and inter
        NaN for that class (and no other graph's).  Under neighbour "average" with learned eps this is common: any
        coalition that leaves a kept node without a kept neighbour scores NaN, as the reference's 0/0 row does on the
        explicit copy -- a few background nodes joined to every node avoid it.  A graph with a non-finite feature gets
        all-NaN results and its batch-mates run as a clean batch, as in lesion().

        The shapes lesion() takes; any other batch raises ValueError naming the condition, as do K > 16 under "exact"
        (use method="permutation"), labels of the wrong length or dtype or below -1, a labelling that names no group, a
        shared labelling over graphs of different node counts, and rows that are not permutations of 0 .. K - 1.  No
        parameter .grad, BatchNorm buffer or numpy RNG state is touched, and the train / eval mode is restored."""
        single, classes = self._interpret_args("shapley", graphs, cls, batch_size)
        if method not in ("exact", "permutation"):
            raise ValueError("shapley: method must be 'exact' or 'permutation', not %r" % (method,))
        ns = [len(g.g) for g in graphs]
        shared = self._shared_labels(labels)
        if shared and any(k != ns[0] for k in ns):
            raise ValueError("shapley: a shared [n] labelling needs graphs of one node count")
        if not shared and (not isinstance(labels, (list, tuple)) or len(labels) != len(graphs)):
            raise ValueError("shapley: labels must be one [n] vector or a list of one [n_g] vector per graph")
        try:
            per = [shapley_host.check_labels(_as_np(labels), ns[0])] * len(graphs) if shared else \
                [shapley_host.check_labels(_as_np(v), n) for v, n in zip(labels, ns)]
        except ValueError as e:
            raise ValueError("shapley: %s" % e) from None
        K = max([int(v.max()) + 1 for v in per if v.size] + [0])
        if K < 1:
            raise ValueError("shapley: the labels name no group")
        if method == "exact":
            if permutations is not None:
                raise ValueError("shapley: permutations belong to method='permutation'")
            if K > shapley_host.EXACT_MAX_PLAYERS:
                raise ValueError("shapley: method='exact' scores 2^K coalitions per graph and takes at most %d groups, "
                                 "got %d; use method='permutation'" % (shapley_host.EXACT_MAX_PLAYERS, K))
            ranks, ids, where = None, np.arange(1 << K, dtype=np.int64), None
        else:
            if interactions:
                raise ValueError("shapley: interactions need method='exact'")
            if K > shapley_host.PREFIX_MAX_PLAYERS:
                raise ValueError("shapley: at most %d groups, got %d" % (shapley_host.PREFIX_MAX_PLAYERS, K))
            if permutations is None:
                raise ValueError("shapley: method='permutation' needs permutations, an int M or an int [M, K] array")
            try:
                if isinstance(permutations, (int, np.integer)):
                    perms = shapley_host.draw_permutations(int(permutations), K, seed)
                else:
                    perms = shapley_host.check_permutations(_as_np(permutations), K)
            except ValueError as e:
                raise ValueError("shapley: %s" % e) from None
            ranks, M = shapley_host.ranks_of(perms), perms.shape[0]
            # the coalitions that run, per graph: every prefix of row 0, and the proper prefixes of the other rows
            # (j = 0 and j = K are v(empty) and v(N) whatever the row); where[m, j]: entry (m, j)'s place among them
            mj = [(0, j) for j in range(K + 1)] + [(m, j) for m in range(1, M) for j in range(1, K)]
            ids = np.array([m * (K + 1) + j for m, j in mj], dtype=np.int64)
            where = np.zeros((M, K + 1), dtype=np.int64)
            where[:, K] = K
            for k, (m, j) in enumerate(mj):
                where[m, j] = k
        cnt = int(ids.shape[0])

        def run_batch(chunk, batch, P, i0):
            def run(b, Xb, which):
                """the coalitions of graphs `which` of the chunk, which are the graphs of batch b, in order"""
                rows = np.full((len(which), int(b.n_max)), -1, dtype=np.int64)
                for k, j in enumerate(which):
                    rows[k, :ns[i0 + j]] = per[i0 + j]
                vgraph = np.repeat(np.arange(len(which), dtype=np.int32), cnt)
                return shapley_hip(self._spec, b, Xb, P, classes, rows, vgraph, np.tile(ids, len(which)), K, ranks)
            return self._sets_batch("shapley", lesion_decline, chunk, batch, P, classes, [cnt] * batch.B, run)
        _, _, values = self._set_scores(graphs, False, classes, batch_size, [cnt] * len(graphs), True, run_batch)
        if method == "exact":
            phi, inter = shapley_exact_hip(values, K, interactions)
            res = (phi, inter) if interactions else (phi,)
        else:
            values = values[:, :, torch.as_tensor(where, device=values.device)]          # [C, G, M, K + 1]
            res = shapley_permutation_hip(values, ranks)
        if return_scores:
            res = res + (values,)
        if single:
            res = tuple(r[0] for r in res)
        return res[0] if len(res) == 1 else res

    def integrated_gradients(self, graphs, cls, steps=32, baseline=None, method="midpoint", batch_size=8,
                             return_scores=False):
        """Integrated-gradients attribution of many graphs in batches: the path method for ReLU networks, whose
        attributions add up to score(X) - score(baseline).  With x' the baseline, (alpha_k, w_k), k < K = steps, the
        quadrature of `method` on [0, 1] (gnm/intgrad.py) and score_c the eval logit c_logit[:, c] of forward()
        (BatchNorm on its running statistics, no dropout -- the score of saliency() and occlusion()):

            attr[c, g] = (X_g - x') * sum_k w_k d score_c / d X (x' + alpha_k (X_g - x'))          [n_g, F0], fp32

        baseline: None for zeros (natural for one-hot node features, where the gradient at the input itself says
        least), or ONE [n, F0] float array or tensor shared by all graphs, which then all have n nodes.  method:
        "midpoint" (alpha_k = (k + 1/2) / K, w = 1 / K), "trapezoid" (endpoints included, K >= 2) or "gausslegendre".

        No copy of a graph and no rescaled feature array is built: every (graph, step) pair runs as a virtual graph
        over the source graph's adjacency, layer 0 is formed from one product per source graph (it is affine in alpha),
        and the steps are summed at hidden width before the one input-width launch per source graph
        (csrc/intgrad.hip, include/gnm_hip.h gnm_integrated_gradients).

        cls: an int, or a sequence of ints; one forward per batch serves all of them.  Returns a float32 device tensor
        [len(graphs), n, F0] for an int `cls` and [len(cls), len(graphs), n, F0] for a sequence; for graphs of
        different node counts a list of [n_g, F0] tensors (a list of such lists for a sequence `cls`), as saliency()
        lays them out.  return_scores=True returns (attr, base, base0, delta): base[c, g] = score_c(X_g) and
        base0[c, g] = score_c(x'), both from the model's ordinary eval forward on the batch, and
        delta[c, g] = sum attr[c, g] - (base - base0), the completeness residual of the quadrature, in fp32
        ([len(graphs)] each for an int `cls`).

        The shapes saliency()'s kernel takes; any other batch raises ValueError naming the condition (max pooling,
        n > 416 or no bit adjacency, hidden_dim not in {32, 64, 128}, average pooling with learned eps and an isolated
        node, ...), as do steps < 1 (< 2 for "trapezoid"), an unknown method, a baseline of the wrong shape or with a
        non-finite entry, and a shared baseline with graphs of different node counts.  A graph with a non-finite
        feature gets an all-NaN map; its batch-mates are unaffected.  There is no CPU fallback.

        The K virtual copies of a batch hold (m L + L + 3) K N hidden_dim floats on the device (0.47 GB at K = 32 for 8
        graphs of 400 nodes, hidden_dim 64, 5 layers of 2 Linears), hence the small default batch; a larger batch is run
        in chunks of whole graphs under gnm/attribution.py INTGRAD_SCRATCH_BYTES.  The result is bitwise the same run to
        run (no atomics, fixed summation orders); it may differ in the last bits between batch sizes, because the
        forward chooses its aggregation kernel per batch.  No parameter .grad, BatchNorm buffer or numpy RNG state is
        touched, and the train / eval mode is restored on exit."""
        alphas, weights = quadrature(method, steps)
        F0 = self.mlps[0].linear.in_features if self.num_mlp_layers == 1 else self.mlps[0].linears[0].in_features
        if baseline is not None and len(graphs):
            baseline = torch.as_tensor(np.asarray(baseline) if not torch.is_tensor(baseline) else baseline)
            if not baseline.dtype.is_floating_point:
                raise ValueError("integrated_gradients: the baseline must be a float array")
            baseline = baseline.detach().to(device=self.eps.device, dtype=torch.float32)
            if any(len(g.g) != len(graphs[0].g) for g in graphs):
                raise ValueError("integrated_gradients: a shared baseline needs graphs of one node count")
            if tuple(baseline.shape) != (len(graphs[0].g), F0):
                raise ValueError("integrated_gradients: the baseline must be [%d, %d], got %s"
                                 % (len(graphs[0].g), F0, list(baseline.shape)))
            if not bool(torch.isfinite(baseline).all()):
                raise ValueError("integrated_gradients: the baseline has a non-finite entry")
        scores = [] if return_scores else None
        single, classes = self._interpret_args("integrated_gradients", graphs, cls, batch_size)
        attr = self._interpret(graphs, single, classes, batch_size, (F0,), functools.partial(
            self._intgrad_batch, alphas=alphas, weights=weights, baseline=baseline, scores=scores))
        if not return_scores:
            return attr
        base =torch.cat([s[0] for s in scores], 1)         # [len(classes), len(graphs)]
        base0 = torch.cat([s[1] for s in scores], 1)
        if torch.is_tensor(attr):
            total = attr.sum((-2, -1))
        elif single:
            total = torch.stack([a.sum() for a in attr])
        else:
            total = torch.stack([torch.stack([a.sum() for a in row]) for row in attr])
        if single:
            base, base0 = base[0], base0[0]
        return attr, base, base0, total - (base - base0)

    def _intgrad_batch(self, chunk, batch, P, classes, dst, alphas, weights, baseline, scores):
        """integrated_gradients() of one batch: [len(classes), N, F0] (dst when given); with `scores` a list, the
        batch's (base, base0) scores [len(classes), B] are appended to it"""
        X = batch.arena.features(batch).detach()
        launch_device(X, P["eps"])                          # no CPU fallback: GnmError before any shape question
        why = saliency_decline(self._spec, batch, X, P, dx=True)
        if why is not None:
            raise ValueError("integrated_gradients does not cover this batch: %s" % why)
        if scores is not None:
            ident = np.arange(batch.B, dtype=np.int64)
            X0 = torch.zeros_like(X) if baseline is None else baseline.repeat(batch.B, 1)
            with torch.no_grad():
                # base is predict()'s logit to the bit: layer 0's aggregate from the arena's cache, as forward_batch
                # takes it (an input wider than the evaluation encoder's 128 columns runs the training kernels,
                # where A X formed per batch differs from the cached one in the last bits)
                P0 = batch.arena.features_and_agg0(batch, self._spec.n_avg, not self._spec.learn_eps)[1]
                c1 = self._run(batch, X, ident, want_disc=False, P0=P0)[0]
                c0 = self._run(batch, X0, ident, want_disc=False)[0]
            scores.append((c1.detach()[:, classes].t().contiguous(), c0.detach()[:, classes].t().contiguous()))
        run = functools.partial(integrated_gradients_hip, alphas=alphas, weights=weights, baseline=baseline)
        bad = _nonfinite_graphs(batch, X)
        if bad is None:
            return run(self._spec, batch, X, P, classes, out=dst)
        return self._clean_graphs_apart(chunk, batch, bad, dst, (len(classes), batch.N, X.shape[1]),
                                        lambda sub, Xs: run(self._spec, sub, Xs, P, classes), crop=False)

    def _clean_graphs_apart(self, chunk, batch, bad, dst, shape, run, crop=True):
        """The gradient class activation and edge maps of a batch with non-finite graphs (`bad`): an all-NaN map for
        each of those (its ReLU masks are meaningless), and the others run(sub, X) on a batch of their own, so their
        maps are those of a clean batch, scattered into place.  crop: the last axis holds n_j entries for graph j (an
        edge map's columns; False for a feature axis).  Returns dst, or a new array of `shape`, [C, N, ...]."""
        out = dst if dst is not None else torch.empty(shape, dtype=torch.float32, device=self.eps.device)
        out.fill_(float("nan"))
        good = [j for j in range(batch.B) if not bad[j]]
        if good:
            sub = self._batch_of([chunk[j] for j in good])
            r = run(sub, sub.arena.features(sub).detach())
            offs, so = np.asarray(batch.node_off_host), np.asarray(sub.node_off_host)
            for k, j in enumerate(good):
                nj = int(so[k + 1] - so[k]) if crop else None
                # (the last axis cropped to the graph's n_j: an edge map's columns; a no-op for a [C, N] map)
                out[:, offs[j]:offs[j + 1]][..., :nj] = r[:, so[k]:so[k + 1]][..., :nj]
        return out

    # ------------------------------------------------------------------ replays
    def _replay_ids(self, batch_graph):
        """(arena ids, (B, n)) of a batch of equal-size graphs, with the layer-0 cache brought up to date (a replay
        only gathers from it); None for graphs of different sizes or an arena off the GPU"""
        arena = self.arena()
        if arena.device.type != "cuda":
            return None
        gh = np.asarray(arena.add_many(batch_graph), dtype=np.int64)
        n_host = arena._tables()["n_host"]
        n = int(n_host[gh[0]])
        if gh.shape[0] > 1 and not (n_host[gh] == n).all():
            return None
        arena.refresh_agg0(self._spec.n_avg, not self._spec.learn_eps)
        return gh, (int(gh.shape[0]), n)

    def _captured(self, cache, key, kind, gh, entries, mode):
        """The capture for `key` in `cache` ({(B, n): capture}, at most `entries` of them): the cached one when it is
        valid_for(gh), else a new kind(self, gh), which takes the place of a stale one for the same key and otherwise
        evicts the oldest entry.  None when the capture fails (e.g. a user hook that synchronises inside the forward):
        no entry is left, `mode`-mode replay is switched off with a warning, the numpy RNG is put back, and the caller
        runs eagerly."""
        c = cache.get(key)
        if c is not None and c.valid_for(gh):
            return c
        cache.pop(key, None)
        if len(cache) >= entries:
            cache.pop(next(iter(cache)))
        rng_state = np.random.get_state()
        try:
            with torch.cuda.device(self.arena().device):
                c = cache[key] = kind(self, gh)
        except Exception as e:
            import warnings
            warnings.warn("%s-mode hipGraph capture failed (%s: %s); running eagerly from now on"
                          % (mode, type(e).__name__, e))
            setattr(self, mode + "_replay", False)
            np.random.set_state(rng_state)
            return None
        return c

    EVAL_REPLAY_MAX_B = 64          # larger eval batches are GPU-bound anyway (and hold more captured activations)
    EVAL_REPLAY_ENTRIES = 6

    def _forward_eval_replay(self, batch_graph, latent):
        """forward() in eval mode for a small batch of equal-size graphs: the eager path's kernels replayed from
        a captured hipGraph (bitwise the same results, ~0.1 ms of host time instead of ~1.4 ms).  None when the batch
        does not qualify -- the caller then takes the eager path."""
        ids = self._replay_ids(batch_graph)
        if ids is None:
            return None
        gh, key = ids
        from gnm.graphs import CapturedEval
        ce = self._captured(self._eval_cache, key, CapturedEval, gh, self.EVAL_REPLAY_ENTRIES, "eval")
        if ce is None:
            return None
        perm = np.random.permutation(key[0])                                  # graphcnn.py:199, consumed as always
        c_logit, d_logit, g_f = ce.run(gh, perm)
        if latent:
            return g_f.cpu().numpy()                                          # graphcnn.py:248-249
        c_logit, d_logit = c_logit.clone(), d_logit.clone()                  # the static buffers are reused
        if torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters()):
            # the reference's outputs carry an autograd graph even in eval mode (main.py:54 detaches them):
            # keep that contract lazily -- a backward through these outputs re-runs the eager forward
            names, tensors, _ = self._param_lists()
            return _LazyEvalGrad.apply(self, gh, perm, c_logit, d_logit, *tensors)
        return c_logit, d_logit

    # ------------------------------------------------------------------ training replay
    TRAIN_REPLAY_MAX_B = 128        # beyond this a step is GPU-bound from Python too (and activations get large)
    TRAIN_REPLAY_ENTRIES = 3

    def _forward_train_replay(self, batch_graph):
        """forward() in train mode for a small batch of equal-size graphs: forward and backward replayed from captured
        hipGraphs (same kernels, same order as the eager path).  None when the batch does not qualify -- other shapes,
        a forward still outstanding on the capture, a gradient sink / cross-rank BatchNorm installed, parameters that
        moved -- and the caller then takes the eager path."""
        sp = self._spec
        if sp.grad_sink is not None or sp.sync_bn is not None or sp.keep_hidden:
            return None
        ids = self._replay_ids(batch_graph)
        if ids is None:
            return None
        gh, key = ids
        ct = self._train_cache.get(key)
        if ct is not None and ct.busy():
            return None                                   # its activations belong to a forward not yet backpropagated
        from gnm.graphs import CapturedTrain
        ct = self._captured(self._train_cache, key, CapturedTrain, gh, self.TRAIN_REPLAY_ENTRIES, "train")
        if ct is None:
            return None
        perm = np.random.permutation(key[0])                                  # graphcnn.py:199, consumed as always
        names, tensors, _ = self._param_lists()
        c_logit, d_logit = _TrainReplayFn.apply(ct, gh, perm, *tensors)
        return c_logit, d_logit

    # ------------------------------------------------------------------ reference API
    def _batch_of(self, batch_graph):
        batch = self.arena().batch(batch_graph)
        if self._spec.n_max:
            from gnm.maxnb import MaxNeighbours
            batch.maxnb = MaxNeighbours(batch_graph, not self.learn_eps, self.arena().device)   # graphcnn.py:55-81
        return batch

    def forward(self, batch_graph, latent=False):
        if (not self.training and self.eval_replay and not self._spec.n_max
                and 0 < len(batch_graph) <= self.EVAL_REPLAY_MAX_B):
            out = self._forward_eval_replay(batch_graph, latent)
            if out is not None:
                return out
        if (self.training and self.train_replay and not latent and not self._spec.n_max and torch.is_grad_enabled()
                and 0 < len(batch_graph) <= self.TRAIN_REPLAY_MAX_B):
            out = self._forward_train_replay(batch_graph)
            if out is not None:
                return out
        return self.forward_batch(self._batch_of(batch_graph), latent=latent)

    def compute_saliency(self, batch_graph, cls):
        self.eval()
        self.zero_grad()
        assert len(batch_graph) == 1                                           # graphcnn.py:257
        batch = self._batch_of(batch_graph)
        X = batch.arena.features(batch).detach().requires_grad_()
        score, _, _ = self._run(batch, X, np.zeros(1, dtype=np.int64), want_disc=False)
        predicting_class = torch.zeros([1, 2], device=X.device)                # two classes hard-coded (:263)
        predicting_class[0, cls] = 1
        score.backward(predicting_class)
        return X.grad


GraphCNN = GIN_InfoMaxReg  # the name BASELINE.json's north_star uses
