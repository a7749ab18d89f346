"""The evaluation encoders across their envelope, against the fp64 oracle: gnm_eval_layers (csrc/evallayer.hip, the
default eval route, model.eval_fused = "layers") and gnm_eval_encoder (csrc/evalfwd.hip, eval_fused = True).

Each case of the matrix below is there to reach a kernel form (its id names it): the column-tile / k-split of the
aggregation (NCA = 1, 2, 4 by F0), the stage-B split (NCT / KSB by H) with its W prefetch per m, the row blocks around
32 and the second bit-row vector (n > 256), the finish kernel's class loop (C up to 256), deep models (L = 16), every
pooling / learn_eps combination, directed, edgeless and isolated-node graphs, and batches below and above the replay
cache.  Parameters are never trivial: running statistics, BatchNorm affine parameters and eps are drawn, and each
Linear is rescaled on the case's own data (in fp64, before anything runs) so that activations stay O(1) at any depth.

Every case asserts its route (a spy on the C entry point: one call per forward), then checks c_logit, d_logit (a
fixed perm through forward_batch), each layer block of the latent g_f and every hidden layer per node against the
fp64 oracle (oracle/gin_oracle.py).  Bounds never come from a HIP output: 1e-5 (max-norm relative) where L <= 5 and
n <= 64; elsewhere max(1e-5, TRUE_SHAPE_FACTOR x the error of an independent fp32 CPU forward through the reference's
ATen ops, oracle/gin_torch_cpu.py), which must itself stay <= 1e-4 -- a case that needs more is badly conditioned.
The measured worst error per case is printed, and collected in the JSON file GNM_EVAL_ENVELOPE_REPORT names when it
is set (profiles/eval_envelope_parity.md)."""
import json
import os
import zlib

import numpy as np
import pytest
import torch

from helpers import TRUE_SHAPE_FACTOR, Calibrated

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CEILING = 1e-4
ENTRY = {True: "gnm_eval_encoder", "layers": "gnm_eval_layers"}
NAN_BITS = 0x7FC0DEAD          # the padding sentinel of the C-ABI tests: a NaN with a payload of its own
# GNM_EVAL_ENVELOPE_REPORT=<file.json>: where record() collects the measured errors of every case (unset: printed only)
REPORT = os.environ.get("GNM_EVAL_ENVELOPE_REPORT")


# --------------------------------------------------------------------------- graphs and models
class EG:
    """the S2VGraph fields the arena and both oracles read"""

    def __init__(self, n, src, dst, feats):
        self.g = range(n)
        self.num_nodes = n
        self.edge_mat = torch.from_numpy(np.ascontiguousarray(np.stack([src, dst]).astype(np.int64)))
        self.node_features = torch.from_numpy(np.ascontiguousarray(feats, dtype=np.float32))
        self.label = 0


def make_graph(rng, n, kind, f0, feats):
    """kind: "sym" (undirected), "dir" (a directed ring plus random arcs: every node has an out-edge, in-degree !=
    out-degree), "empty" (no edges), "iso" (undirected with a few nodes cut off), "multi" (one edge listed twice)"""
    dens = 0.3 if n <= 64 else 0.15
    A = rng.random((n, n)) < dens
    np.fill_diagonal(A, False)
    if kind == "dir":
        if n > 1:
            A[np.arange(n), (np.arange(n) + 1) % n] = True
    elif kind == "empty":
        A[:] = False
    else:
        A = np.triu(A, 1)
        A = A | A.T
        if kind == "iso":
            cut = rng.choice(n, size=max(1, n // 8), replace=False)
            A[cut, :] = False
            A[:, cut] = False
    src, dst = np.nonzero(A)
    if kind == "multi":
        src, dst = np.append(src, src[0]), np.append(dst, dst[0])
    if feats == "onehot":
        X = np.eye(f0, dtype=np.float32)[rng.integers(0, f0, n)]
    else:                      # mixed scale: columns from 0.03 to 30
        X = rng.standard_normal((n, f0)) * 10.0 ** rng.uniform(-1.5, 1.5, f0)
    return EG(n, src, dst, X)


def oracle_graphs(graphs):
    from oracle import gin_oracle as O
    return [O.OGraph(g.num_nodes, g.edge_mat.numpy(), g.node_features.numpy()) for g in graphs]


def _lin_names(l, k, m):
    wn = f"mlps.{l}.linear" if m == 1 else f"mlps.{l}.linears.{k}"
    bn = f"batch_norms.{l}" if k == m - 1 else f"mlps.{l}.batch_norms.{k}"
    return wn, bn


def build_model(graphs, L, m, f0, H, C, learn_eps, gpool, npool, seed, tiny_var=False):
    """GIN_InfoMaxReg with drawn running statistics (mean ~ N(0, 0.3^2), var in [0.2, 3], or about 1e-3 with
    tiny_var), BatchNorm gamma in [0.5, 1.5], beta ~ N(0, 0.2^2), eps in [-0.4, 0.4]; each Linear then divided by the
    RMS of its output on this batch (an fp64 forward), so that every layer's activations are O(1)"""
    from models.graphcnn import GIN_InfoMaxReg
    from oracle import gin_oracle as O
    torch.manual_seed(seed)
    model = GIN_InfoMaxReg(L, m, f0, H, C, 0.5, learn_eps, gpool, npool, torch.device("cpu"))
    g = np.random.default_rng(seed + 1000)
    sd = model.state_dict()
    with torch.no_grad():
        for k, t in sd.items():
            if k.endswith("running_mean"):
                t.copy_(torch.from_numpy(g.normal(0, 0.3, t.shape)))
            elif k.endswith("running_var"):
                t.copy_(torch.from_numpy(g.uniform(5e-4, 2e-3, t.shape) if tiny_var else g.uniform(0.2, 3.0, t.shape)))
            elif "batch_norms" in k and k.endswith("weight"):
                t.copy_(torch.from_numpy(g.uniform(0.5, 1.5, t.shape)))
            elif "batch_norms" in k and k.endswith("bias"):
                t.copy_(torch.from_numpy(g.normal(0, 0.2, t.shape)))
        sd["eps"].copy_(torch.from_numpy(g.uniform(-0.4, 0.4, L)))
        p = {k: t.numpy().astype(np.float64) for k, t in sd.items()}
        idx, val, shape = O.build_adj_block(oracle_graphs(graphs), learn_eps)
        A = O.coo_to_csr(idx, val, shape, np.float64)
        deg = np.asarray(A.sum(1)).reshape(-1, 1)
        h = np.concatenate([gr.node_features.numpy() for gr in graphs]).astype(np.float64)
        for l in range(L):
            x = A @ h
            if npool == "average":
                x = np.divide(x, deg, out=np.zeros_like(x), where=deg > 0)
            if learn_eps:
                x = x + (1 + p["eps"][l]) * h
            for k in range(m):
                wn, bn = _lin_names(l, k, m)
                z = x @ p[wn + ".weight"].T + p[wn + ".bias"]
                s = float(np.sqrt(np.mean(z * z))) or 1.0
                sd[wn + ".weight"].div_(s)
                sd[wn + ".bias"].div_(s)
                p[wn + ".weight"], p[wn + ".bias"] = sd[wn + ".weight"].numpy().astype(np.float64), sd[wn + ".bias"].numpy().astype(np.float64)
                z = x @ p[wn + ".weight"].T + p[wn + ".bias"]
                y = (z - p[bn + ".running_mean"]) / np.sqrt(p[bn + ".running_var"] + 1e-5) * p[bn + ".weight"] + p[bn + ".bias"]
                x = np.maximum(y, 0)
            h = x
    return model.to(torch.device(DEV)).eval()


def state_of(model):
    return {k: v.detach().cpu().numpy() for k, v in model.state_dict().items()}


def count_calls(monkeypatch, name):
    from gnm import core
    calls = []
    real = getattr(core.lib, name)

    def spy(*a):
        calls.append(1)
        return real(*a)
    monkeypatch.setattr(core.lib, name, spy, raising=False)
    return calls


# --------------------------------------------------------------------------- the C entry points, called directly
def param_table(model):
    """the device parameter table both entry points read (gnm_eval_table_words; gnm/core.py eval_forward_fused)"""
    from gnm.core import lib
    P = dict(model.named_parameters())
    P.update(dict(model.named_buffers()))
    L, m = model.num_layers, model.num_mlp_layers
    words = []
    for l in range(L):
        for k in range(m):
            wn, bn = _lin_names(l, k, m)
            W = P[wn + ".weight"]
            words += [W.data_ptr(), P[wn + ".bias"].data_ptr(), P[bn + ".weight"].data_ptr(), P[bn + ".bias"].data_ptr(),
                      P[bn + ".running_mean"].data_ptr(), P[bn + ".running_var"].data_ptr(), W.stride(0)]
    for l in range(L):
        words += [P[f"linears_prediction.{l}.weight"].data_ptr(), P[f"linears_prediction.{l}.bias"].data_ptr()]
    assert len(words) == int(lib.gnm_eval_table_words(L, m))
    return torch.tensor(words, dtype=torch.int64, device=DEV)


def launch(model, batch, mode, X, ldx, hidden, hidden_stride, ldh, g_f, ldgf, c_sig, c_logit, ldc):
    """one gnm_eval_layers / gnm_eval_encoder call on explicit buffers and leading dimensions; returns its status"""
    from gnm.core import BN_EPS, lib
    a, sp = batch.arena, model._spec
    H = model.batch_norms[0].num_features
    C = model.linears_prediction[0].out_features
    F0 = model.mlps[0].linear.in_features if sp.m == 1 else model.mlps[0].linears[0].in_features
    table = param_table(model)
    eps = model.eps.data_ptr() if sp.learn_eps else None
    common = (a.bits.buf.data_ptr(), batch.bits_off.data_ptr(), batch.node_off.data_ptr(), a.rowptr.buf.data_ptr(),
              batch.rp_off.data_ptr(), batch.B, batch.n_max, X.data_ptr(), ldx, F0, H, sp.L, sp.m, C, int(sp.n_avg),
              int(not sp.learn_eps), int(sp.g_avg), BN_EPS, table.data_ptr(), eps, hidden.data_ptr(), hidden_stride, ldh)
    tail = (g_f.data_ptr(), ldgf, None if c_sig is None else c_sig.data_ptr(), c_logit.data_ptr(), ldc,
            torch.cuda.current_stream().cuda_stream)
    if mode == "layers":
        scratch = torch.empty(int(lib.gnm_eval_layers_scratch_floats(batch.B, batch.n_max, H, sp.L)),
                              dtype=torch.float32, device=DEV)
        rc = lib.gnm_eval_layers(*common, scratch.data_ptr(), *tail)
    else:
        s0 = torch.empty((batch.N, H), dtype=torch.float32, device=DEV)
        s1 = torch.empty_like(s0)
        rc = lib.gnm_eval_encoder(*common, s0.data_ptr(), s1.data_ptr(), H, *tail)
    torch.cuda.synchronize()
    return rc


def eval_kernel(model, batch, mode):
    """(hidden [L, N, H], g_f [B, L H], c_logit [B, C]) of one plain call of the entry point (numpy)"""
    H, L = model.batch_norms[0].num_features, model.num_layers
    C = model.linears_prediction[0].out_features
    X = batch.arena.features(batch).detach().contiguous()
    f32 = dict(dtype=torch.float32, device=DEV)
    hidden = torch.empty((L, batch.N, H), **f32)
    g_f = torch.empty((batch.B, L * H), **f32)
    c_logit = torch.empty((batch.B, C), **f32)
    assert launch(model, batch, mode, X, X.stride(0), hidden, hidden.stride(0), H, g_f, L * H, None, c_logit, C) == 0
    return hidden.cpu().numpy(), g_f.cpu().numpy(), c_logit.cpu().numpy()


# --------------------------------------------------------------------------- checking
def record(case, form, cal):
    """the measured errors of a case (vs fp64, the fp32 CPU forward's own error, the bound): printed, and into REPORT"""
    worst = max(cal.log, key=lambda t: t[1])
    print("%-36s %s: worst %.2e (%s), bound %.1e" % (case, form, worst[1], worst[0], max(t[3] for t in cal.log)))
    if not REPORT:
        return
    try:
        os.makedirs(os.path.dirname(os.path.abspath(REPORT)), exist_ok=True)
        data = json.load(open(REPORT)) if os.path.exists(REPORT) else {}
        data[case] = {"form": form, "worst": worst[1], "worst_what": worst[0], "bound": max(t[3] for t in cal.log),
                      "flat": cal.factor == 0, "checks": [list(t) for t in cal.log]}
        json.dump(data, open(REPORT, "w"), indent=1)
    except OSError:
        pass


def check_against_oracle(case, form, graphs, model, perm, c_logit, d_logit, lat, hidden, flat):
    """c_logit, d_logit (or None), each layer block of the latent and every hidden layer (or None) against the fp64
    oracle, bound by the fp32 CPU forward's own error (helpers.Calibrated; factor 0 = the flat 1e-5)"""
    from oracle import gin_oracle as O
    from oracle.gin_torch_cpu import TorchCpuGIN
    sp, state = model._spec, state_of(model)
    ob = oracle_graphs(graphs)
    want_disc = d_logit is not None
    om = O.OracleGIN(state, sp.L, sp.m, sp.learn_eps, model.graph_pooling_type, model.neighbor_pooling_type,
                     dtype=np.float64)
    with np.errstate(all="ignore"):
        tc, td, tcache = om.forward(ob, perm, training=False, want_disc=want_disc)
    t32, o32 = TorchCpuGIN(state, sp.L, sp.m, sp.learn_eps, model.graph_pooling_type, model.neighbor_pooling_type), {}
    with torch.no_grad():
        c32, d32 = t32.forward(ob, perm, training=False, want_disc=want_disc, out=o32)
    cal = Calibrated(factor=0.0 if flat else TRUE_SHAPE_FACTOR)
    H = tcache["hidden"][0].shape[1]
    N = tcache["hidden"][0].shape[0]
    rs = slice(None, None, max(1, N // 4096))

    def chk(a, r32, t, what):
        cal.check(a, r32, t, what=what)
        assert cal.log[-1][3] <= CEILING, "%s: the fp32 CPU forward is %.2e from fp64: a badly conditioned case" % (
            what, cal.log[-1][2])

    if hidden is not None:
        for l in range(sp.L):
            chk(hidden[l][rs], o32["hidden"][l].numpy()[rs], tcache["hidden"][l][rs], "hidden %d" % l)
    for l in range(sp.L):
        blk = slice(l * H, (l + 1) * H)
        chk(lat[:, blk], o32["g_f"].numpy()[:, blk], tcache["g_f"][:, blk], "latent %d" % l)
    chk(c_logit, c32.numpy(), tc, "c_logit")
    if want_disc:
        chk(d_logit, d32.numpy(), td, "d_logit")
    record(case, form, cal)
    return cal


# --------------------------------------------------------------------------- the envelope matrix
# (id, mode, H, m, F0, n, B, L, C, gpool, npool, learn_eps, graph, features)
LAYER_CASES = [
    ("H32m1-F1-n1-L1-C1", "layers", 32, 1, 1, 1, 3, 1, 1, "sum", "sum", True, "sym", "mixed"),
    ("H32m2-F15-n16-dir-avg", "layers", 32, 2, 15, 16, 3, 2, 2, "average", "average", True, "dir", "mixed"),
    ("H32m3-F16-n17-C5-dir", "layers", 32, 3, 16, 17, 3, 5, 5, "sum", "average", False, "dir", "mixed"),
    ("H32m1-F17-n31-C64-onehot", "layers", 32, 1, 17, 31, 1, 2, 64, "average", "sum", False, "sym", "onehot"),
    ("H32m2-F32-n32-C65-B70", "layers", 32, 2, 32, 32, 70, 2, 65, "sum", "sum", True, "sym", "mixed"),
    ("H32m3-F33-NCA2-n33-L16", "layers", 32, 3, 33, 33, 3, 16, 2, "average", "average", False, "sym", "mixed"),
    ("H32m2-F64-n256-C256-dir", "layers", 32, 2, 64, 256, 3, 5, 256, "sum", "average", True, "dir", "mixed"),
    ("H32m1-F65-NCA4-n257-iso", "layers", 32, 1, 65, 257, 3, 2, 5, "average", "sum", True, "iso", "mixed"),
    ("H32m2-F128-NCA4-n416", "layers", 32, 2, 128, 416, 1, 5, 2, "sum", "sum", False, "sym", "mixed"),
    ("H32m3-F100-NCA4-n400", "layers", 32, 3, 100, 400, 3, 2, 2, "average", "average", True, "sym", "mixed"),
    ("H32m2-F7-n416-L16", "layers", 32, 2, 7, 416, 2, 16, 2, "sum", "sum", True, "sym", "mixed"),
    ("H64m1-F1-n17-B300", "layers", 64, 1, 1, 17, 300, 2, 2, "sum", "sum", False, "sym", "mixed"),
    ("H64m2-F15-n33-L16-C5", "layers", 64, 2, 15, 33, 3, 16, 5, "sum", "sum", True, "sym", "mixed"),
    ("H64m3-F16-n1-B70-C1", "layers", 64, 3, 16, 1, 70, 5, 1, "average", "average", False, "sym", "mixed"),
    ("H64m1-F33-NCA2-n400-C64-dir", "layers", 64, 1, 33, 400, 3, 5, 64, "average", "average", True, "dir", "mixed"),
    ("H64m2-F65-NCA4-n32-C65-dir", "layers", 64, 2, 65, 32, 3, 2, 65, "sum", "average", False, "dir", "mixed"),
    ("H64m3-F100-NCA4-n257-L16-iso", "layers", 64, 3, 100, 257, 3, 16, 2, "sum", "sum", False, "iso", "mixed"),
    ("H64m2-F128-NCA4-n31-C256-onehot", "layers", 64, 2, 128, 31, 3, 5, 256, "average", "sum", True, "sym", "onehot"),
    ("H64m1-F64-n256-L1-edgeless", "layers", 64, 1, 64, 256, 1, 1, 5, "sum", "sum", True, "empty", "mixed"),
    ("H64m2-F32-n416-B2", "layers", 64, 2, 32, 416, 2, 5, 2, "average", "average", False, "sym", "mixed"),
    ("H64m2-F17-n16-tinyvar", "layers", 64, 2, 17, 16, 3, 2, 2, "sum", "average", True, "sym", "mixed"),
    ("H128m1-F1-n33-avg", "layers", 128, 1, 1, 33, 3, 5, 2, "average", "average", True, "sym", "mixed"),
    ("H128m2-F15-n257-C64-dir", "layers", 128, 2, 15, 257, 3, 2, 64, "sum", "sum", True, "dir", "mixed"),
    ("H128m3-F17-n16-B300-C5", "layers", 128, 3, 17, 16, 300, 2, 5, "average", "sum", False, "sym", "mixed"),
    ("H128m1-F32-n17-L16-C65", "layers", 128, 1, 32, 17, 3, 16, 65, "sum", "average", True, "sym", "mixed"),
    ("H128m2-F64-n31-C1-iso", "layers", 128, 2, 64, 31, 3, 5, 1, "sum", "sum", False, "iso", "mixed"),
    ("H128m3-F65-NCA4-n416-dir", "layers", 128, 3, 65, 416, 2, 5, 2, "average", "average", False, "dir", "mixed"),
    ("H128m2-F100-NCA4-n1-C256", "layers", 128, 2, 100, 1, 3, 2, 256, "sum", "sum", True, "sym", "mixed"),
    ("H128m1-F128-NCA4-n400-L16-onehot", "layers", 128, 1, 128, 400, 1, 16, 5, "average", "sum", False, "sym", "onehot"),
    ("H128m2-F33-NCA2-n256-B70-edgeless", "layers", 128, 2, 33, 256, 70, 2, 2, "sum", "average", False, "empty", "mixed"),
    ("H128m3-F128-NCA4-n32", "layers", 128, 3, 128, 32, 3, 2, 2, "average", "sum", True, "sym", "mixed"),
    ("H128m2-F7-n33-iso-sum", "layers", 128, 2, 7, 33, 3, 5, 2, "sum", "sum", True, "iso", "mixed"),
]
ENCODER_CASES = [
    ("enc-m1-F1-n17", True, 64, 1, 1, 17, 3, 5, 2, "sum", "sum", True, "sym", "mixed"),
    ("enc-m2-F33-n400-C64-dir", True, 64, 2, 33, 400, 2, 5, 64, "average", "average", True, "dir", "mixed"),
    ("enc-m3-F64-n1-C5", True, 64, 3, 64, 1, 3, 2, 5, "sum", "average", False, "sym", "mixed"),
    ("enc-m2-F64-n17-B70-L16", True, 64, 2, 64, 17, 70, 16, 2, "average", "sum", False, "sym", "mixed"),
    ("enc-m3-F33-n400-L16-C1-iso", True, 64, 3, 33, 400, 1, 16, 1, "sum", "sum", False, "iso", "mixed"),
    ("enc-m1-F1-n400-C64-edgeless", True, 64, 1, 1, 400, 3, 2, 64, "average", "average", False, "empty", "mixed"),
    ("enc-m2-F7-n17-onehot-dir", True, 64, 2, 7, 17, 3, 5, 2, "sum", "average", True, "dir", "onehot"),
]


def kernel_form(mode, H, m, F0, n, L, C):
    if mode is True:
        return "encoder H64 m%d F0 %d n %d (W %d) L %d C %d" % (m, F0, n, (n + 31) // 32, L, C)
    nca = 1 if F0 <= 32 else (2 if F0 <= 64 else 4)
    nct = H // 32
    return "layers NCA %d KS %d, NCT %d KSB %d m %d, W %d%s, L %d, C %d (C %% 4 = %d)" % (
        nca, 4 // nca, nct, 4 // nct, m, (n + 31) // 32, " rp[1]" if n > 256 else "", L, C, C % 4)


def run_case(case, mode, H, m, F0, n, B, L, C, gpool, npool, learn_eps, kind, feats, monkeypatch, expect_route=True):
    rng = np.random.default_rng(zlib.crc32(case.encode()))
    # (isolated nodes in the first graph only: under average pooling with learn_eps their 0/0 rows make that graph's
    # readout NaN, and the others keep finite values to compare)
    graphs = [make_graph(rng, n, kind if kind != "iso" or j == 0 else "sym", F0, feats) for j in range(B)]
    model = build_model(graphs, L, m, F0, H, C, learn_eps, gpool, npool, seed=H + 7 * m + F0 + n + L,
                        tiny_var="tinyvar" in case)
    model.eval_fused = mode
    model.eval_replay = False          # the route of each forward is counted below (the replay: test_gpu_eval_fused.py)
    batch = model._batch_of(graphs)
    perm = rng.permutation(B)
    calls = {e: count_calls(monkeypatch, e) for e in ENTRY.values()}
    from gnm import core
    fallback = {}
    real_encoder = core.encoder_forward

    def layer_by_layer(*a, **k):       # the hidden layers of the training kernels, where those run instead
        out = real_encoder(*a, **k)
        fallback.setdefault("hidden", [core.hidden_tensor(h).detach().cpu().numpy() for h in out[0]])
        return out
    monkeypatch.setattr(core, "encoder_forward", layer_by_layer)
    with torch.no_grad():
        c_logit, d_logit = model.forward_batch(batch, perm=perm)
        lat = model.forward_batch(batch, perm=perm, latent=True)
    c_logit, d_logit = c_logit.cpu().numpy(), d_logit.cpu().numpy()
    mine, other = ENTRY[mode], ENTRY[True if mode == "layers" else "layers"]
    assert len(calls[other]) == 0
    if expect_route:
        assert batch.has_bits
        assert len(calls[mine]) == 2, "%s: %d calls of %s for two forwards" % (case, len(calls[mine]), mine)
        hidden, g_f, c_k = eval_kernel(model, batch, mode)
        assert np.array_equal(g_f, lat) and np.array_equal(c_k, c_logit)     # the same kernel, the same bits
    else:
        assert len(calls[mine]) == 0, "%s: outside the envelope, yet %s ran" % (case, mine)
        hidden = fallback["hidden"]
    flat = L <= 5 and n <= 64
    return check_against_oracle(case, kernel_form(mode, H, m, F0, n, L, C) if expect_route else "fallback",
                                graphs, model, perm, c_logit, d_logit, lat, hidden, flat)


@pytest.mark.parametrize("case,mode,H,m,F0,n,B,L,C,gpool,npool,learn_eps,kind,feats",
                         LAYER_CASES + ENCODER_CASES, ids=[c[0] for c in LAYER_CASES + ENCODER_CASES])
def test_eval_envelope_vs_fp64(case, mode, H, m, F0, n, B, L, C, gpool, npool, learn_eps, kind, feats, monkeypatch):
    run_case(case, mode, H, m, F0, n, B, L, C, gpool, npool, learn_eps, kind, feats, monkeypatch)


OUTSIDE_CASES = [
    ("out-H48", "layers", 48, 2, 7, 33, 3, 2, 2, "sum", "sum", True, "sym", "mixed"),
    ("out-F129", "layers", 64, 2, 129, 33, 3, 2, 2, "sum", "sum", True, "sym", "mixed"),
    ("out-C257", "layers", 64, 2, 7, 33, 3, 2, 257, "average", "sum", True, "sym", "mixed"),
    ("out-n417", "layers", 64, 2, 7, 417, 2, 2, 2, "sum", "average", False, "sym", "mixed"),
    ("out-multigraph", "layers", 64, 2, 7, 33, 3, 2, 2, "sum", "sum", True, "multi", "mixed"),
    ("out-avg-learn_eps-iso", "layers", 64, 2, 7, 33, 3, 2, 2, "sum", "average", True, "iso", "mixed"),
    ("out-enc-H128", True, 128, 2, 7, 33, 3, 2, 2, "sum", "sum", True, "sym", "mixed"),
    ("out-enc-F65", True, 64, 2, 65, 33, 3, 2, 2, "sum", "sum", True, "sym", "mixed"),
    ("out-enc-n401", True, 64, 2, 7, 401, 2, 2, 2, "sum", "sum", True, "sym", "mixed"),
]


@pytest.mark.parametrize("case,mode,H,m,F0,n,B,L,C,gpool,npool,learn_eps,kind,feats", OUTSIDE_CASES,
                         ids=[c[0] for c in OUTSIDE_CASES])
def test_just_outside_the_envelope_falls_back(case, mode, H, m, F0, n, B, L, C, gpool, npool, learn_eps, kind, feats,
                                              monkeypatch):
    """one step past each limit of eval_fused_ok: the encoder is not called and the layer-by-layer path that runs
    instead meets the same bounds against the fp64 oracle"""
    run_case(case, mode, H, m, F0, n, B, L, C, gpool, npool, learn_eps, kind, feats, monkeypatch, expect_route=False)


# --------------------------------------------------------------------------- C-ABI edges
@pytest.mark.parametrize("mode,sizes", [("layers", [1, 33, 416, 17, 256, 257]), (True, [1, 33, 400, 17, 256, 257])],
                         ids=["layers", "encoder"])
def test_ragged_batch_in_one_launch(mode, sizes):
    """graphs of 1 .. 416 nodes in one launch (the row-block grid sized by the largest, W < wmax early exits, the
    finish kernel's per-graph W and 1/n), no discriminator: every graph's values are the oracle's"""
    rng = np.random.default_rng(len(sizes) + (mode is True))
    H = 64 if mode is True else 128
    graphs = [make_graph(rng, n, "sym", 40, "mixed") for n in sizes]
    model = build_model(graphs, 3, 2, 40, H, 5, False, "average", "average", seed=17)
    batch = model._batch_of(graphs)
    assert batch.has_bits and not batch.equal_n and batch.n_max == max(sizes)
    hidden, g_f, c_logit = eval_kernel(model, batch, mode)
    check_against_oracle("ragged-" + ("encoder" if mode is True else "layers"),
                         kernel_form(mode, H, 2, 40, max(sizes), 3, 5) + ", ragged %s" % sizes, graphs, model,
                         np.arange(len(sizes)), c_logit, None, g_f, hidden, flat=False)


def _sentinel(shape):
    return torch.full(shape, NAN_BITS, dtype=torch.int32, device=DEV).view(torch.float32)


@pytest.mark.parametrize("mode", ["layers", True], ids=["layers", "encoder"])
def test_padded_leading_dimensions(mode):
    """ldx = F0 + 5, ldh = H + 4, a hidden_stride beyond N ldh, padded ldgf and ldc: the padding holds a NaN
    sentinel before the call and is bit-identical after it (no write outside the logical arrays, no read of X's
    padding), and the logical values are those of the contiguous call"""
    rng = np.random.default_rng(5)
    H, L, C, F0 = 64, 3, 6, 21
    graphs = [make_graph(rng, 45, "sym", F0, "mixed") for _ in range(3)]
    model = build_model(graphs, L, 2, F0, H, C, True, "sum", "sum", seed=23)
    batch = model._batch_of(graphs)
    N, B = batch.N, batch.B
    ldx, ldh, ldgf, ldc = F0 + 5, H + 4, L * H + 3, C + 3
    hstride = N * ldh + 37
    X = _sentinel((N, ldx))
    X[:, :F0] = batch.arena.features(batch)
    hidden = _sentinel((L * hstride,))
    g_f, c_sig, c_logit = _sentinel((B, ldgf)), _sentinel((B, ldgf)), _sentinel((B, ldc))
    before = [t.clone() for t in (hidden, g_f, c_sig, c_logit)]
    assert launch(model, batch, mode, X, ldx, hidden, hstride, ldh, g_f, ldgf, c_sig, c_logit, ldc) == 0
    hv = hidden.view(-1)
    logical = torch.zeros(L * hstride, dtype=torch.bool, device=DEV)
    for l in range(L):
        logical[l * hstride:l * hstride + N * ldh].view(N, ldh)[:, :H] = True
    for got, was, mask, what in ((hv, before[0], logical, "hidden"), (g_f, before[1], None, "g_f"),
                                 (c_sig, before[2], None, "c_sig"), (c_logit, before[3], None, "c_logit")):
        if mask is None:
            mask = torch.zeros_like(got, dtype=torch.bool)
            mask[:, :(C if what == "c_logit" else L * H)] = True
        gi, wi = got.view(torch.int32), was.view(torch.int32)
        assert torch.equal(gi[~mask], wi[~mask]), "%s: the padding was written" % what
        assert bool(torch.isfinite(got[mask]).all()), "%s: a logical value is not finite" % what
    h_ref, gf_ref, c_ref = eval_kernel(model, batch, mode)
    hid = np.stack([hv[l * hstride:l * hstride + N * ldh].view(N, ldh)[:, :H].cpu().numpy() for l in range(L)])
    assert np.array_equal(hid, h_ref)
    assert np.array_equal(g_f[:, :L * H].cpu().numpy(), gf_ref)
    assert np.array_equal(c_logit[:, :C].cpu().numpy(), c_ref)
    assert np.allclose(c_sig[:, :L * H].cpu().numpy(), 1 / (1 + np.exp(-gf_ref.astype(np.float64))), rtol=1e-6, atol=0)
