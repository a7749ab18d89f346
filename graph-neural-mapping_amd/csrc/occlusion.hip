// Per-ROI occlusion (virtual lesioning): the eval-mode class scores of every node-deleted copy G \ v of every graph of a
// batch (GIN_InfoMaxReg.occlusion(); the reference's forward in eval(), graphcnn.py:194-231, on a graph with node v, its
// edges in both directions and its feature row removed), without building a single copy.
//
// A VIRTUAL graph is (source graph g, deleted node v): it reads g's bit rows, rowptr and node_off and owns n_g rows of
// two ping-pong activation arrays.  Virtual graph q of a batch is node q of the batch (v = q - node_off[g]), so there
// are N of them.  Deleting v is three things in csrc/evallayer.hip's layer (whose structure this file keeps: bits as
// the B operand of the aggregation, three exact bf16 planes of the activations, six-term split Linears from the LDS
// tile, folded BatchNorm, the NaN-propagating ReLU):
//   * row v of every layer's output is written as ZEROS, so the next layer's product A h drops column v by itself;
//   * row v is left out of the graph readout (which then runs over n - 1 nodes);
//   * a row's degree under neighbour "average" is its rowptr degree minus bit (r, v).
// Layer 0 never multiplies by the features: they are shared by the n virtual graphs of a source graph and the first
// Linear is linear, so the caller forms XW = X W0^T and S = (A + I) XW once per SOURCE graph (gnm_linear_fwd, gnm_agg /
// gnm_aggm at width H -- any input width) and the first pre-activation of row r != v of (g, v) is
//     self loops:   (S[r] - a_rv XW[v]) [/ (deg_r + 1 - a_rv)] + b
//     learned eps:  (S[r] - a_rv XW[v]) + eps0 XW[r] + b                              (sum)
//                   (S[r] - XW[r] - a_rv XW[v]) / (deg_r - a_rv) + (1 + eps0) XW[r] + b   (average; 0/0 -> NaN as in
//                                                                                        the reference: a leaf of v)
// One launch per layer over (virtual graph, 32-row block), then a launch that adds the readout shares in fixed order,
// scales by the fp32 1/(n - 1) under graph "average" and applies the classifier head.  No float atomics; every sum has
// a fixed order, so results are bitwise reproducible and do not depend on how the caller chunks the graphs.
#include "gnm_rowblock.h"
#include <string.h>

static constexpr int kOcMaxClasses = 8;           // classes per finish launch

struct OcArgs : RbVirtualArgs {                   // vrow_off [B]: sum of n^2 before graph g
    const int32_t* rowptr; const int64_t* b_rp_off;
    const float* S; int lds;                      // layer 0: (A + I) X W0^T of the SOURCE graphs, [N, H]
};

// FIRST: layer 0 (the first pre-activation from XW and S, see the file header; no product with the adjacency and no
// first Linear); otherwise a layer >= 1 on the virtual graph's own activations (input width H).
template <bool FIRST>
__global__ void __launch_bounds__(256) gnm_occlusion_layer_kernel(const OcArgs p) {
    __shared__ __attribute__((aligned(16))) float T0[32 * kRbTS];
    __shared__ __attribute__((aligned(16))) float T1[32 * kRbTS];
    __shared__ __attribute__((aligned(16))) float part[4][32][33];
    __shared__ __attribute__((aligned(16))) char lut[128];
    __shared__ unsigned bitsw[8][256];            // word j of thread t's half row of the block's adjacency bits
    __shared__ float aff[3][3][kRbMaxH];          // per Linear of the MLP: bias, scale, shift (the BatchNorm behind it, folded)
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int i = lane & 31, h = lane >> 5;
    const int q = blockIdx.x / p.wmax, rb = blockIdx.x - q * p.wmax;
    const int b = p.vgraph[q];
    const int node0 = p.node_off[b];
    const int n = p.node_off[b + 1] - node0;
    const int v = q - node0;                                      // the deleted node
    const int W = (n + 31) >> 5;
    if (rb >= W) return;
    const size_t row0 = (size_t)p.vrow_off[b] + (size_t)v * n;    // the virtual graph's rows of Hin / Hout
    const int H = p.H;
    const int HPW = rb_half_words(W);
    const uint32_t* gbits = p.adj_bits + p.b_bits_off[b];
    if (!FIRST) rb_lut_init(lut, tid);
    // what the MLP needs that does not depend on the tile, requested now (layer 0's first Linear ran on the source graphs)
    RbMlp M;
    rb_mlp_prefetch<FIRST ? 1 : 0>(M, aff, p.table, p.l, p.m, p.bn_eps, H, H, tid, wave, i, h);
    const int NCT = M.NCT;
    // the combine pass's operands (8 threads per tile row): the row, whether it is a row of the deleted graph, bit
    // (row, v) of the adjacency and the row's reduced degree
    const int row = tid >> 3, c8 = tid & 7;
    const int vr = min(rb * 32 + row, n - 1);
    const bool vrow = rb * 32 + row < n;
    const bool keep = vrow && vr != v;
    const unsigned arv = rb_row_bit(gbits + (size_t)vr * (2 * HPW), HPW, v);
    float deg = 1.f;
    if (p.average) {
        const int32_t* rp = p.rowptr + p.b_rp_off[b];
        deg = (float)(rp[vr + 1] - rp[vr] - (int)arv + p.self_loop);
    }
    const float eps_l = p.eps ? p.eps[p.l] : 0.f;
    // what the layer's last Linear leaves of column c of this thread's row
    auto last_rule = [&](int c, float y) {
        if (!keep) y = 0.f;                                       // the deleted row (and rows past n): zeros, not in the readout
        if (vrow && p.l + 1 < p.L) p.Hout[(row0 + vr) * H + c] = y;
        return y;
    };
    if (FIRST) {
        // ---- layer 0: the first Linear's output of the deleted graph from the source graph's XW and S ----------------
        __syncthreads();                                          // the vectors
        const float* xwr = p.XW + (size_t)(node0 + vr) * p.ldxw;
        const float* xwv = p.XW + (size_t)(node0 + v) * p.ldxw;
        const float* sr = p.S + (size_t)(node0 + vr) * p.lds;
        const float selfw = 1.f + eps_l;                          // graphcnn.py:161 (1 + eps[layer]) h
        const bool last = p.m == 1;
        for (int c = c8; c < H; c += 8) {
            const float xw = xwr[c];
            float t = sr[c];
            if (!p.self_loop && p.average) t -= xw;
            if (arv) t -= xwv[c];
            t = rb_pool_combine<true, true>(t, xw, deg, p.average ? selfw : eps_l, p.self_loop, p.average);
            float y = gnm_relu((t + aff[0][0][c]) * aff[0][1][c] + aff[0][2][c]);
            if (last) y = last_rule(c, y);
            T1[row * kRbTS + c] = y;
        }
    } else {
        // ---- A. aggregation over the virtual graph's activations (row v of them is zero) ---------------------------
        const int NCA = NCT;
        const float* Hg = p.Hin + row0 * H;
        for (int c = c8; c < H; c += 8) T1[row * kRbTS + c] = Hg[(size_t)vr * H + c];       // the self term, parked
        rb_stage_bits(bitsw, gbits, rb, i, h, HPW, tid);
        rb_rows_product(part, lut, bitsw, Hg, H, n, H, NCA, tid, wave, i, h);
        __syncthreads();
        const int KS = 4 / NCA;
        const float selfw = 1.f + eps_l;                          // graphcnn.py:161 (1 + eps[layer]) h
        for (int c = c8; c < H; c += 8) {
            float t = 0.f;
            for (int k = 0; k < KS; ++k) t += part[(c >> 5) + NCA * k][row][c & 31];
            t = rb_pool_combine<true>(t, T1[row * kRbTS + c], deg, selfw, p.self_loop, p.average);
            T0[row * kRbTS + c] = vrow ? t : 0.f;
        }
    }
    // ---- B. the MLP (layer 0: from its second Linear) ----------------------------------------------------------
    float* Tin = FIRST ? T1 : T0;
    float* Tout = FIRST ? T0 : T1;
    rb_mlp_forward<FIRST ? 1 : 0>(M, aff, part, Tin, Tout, p.m, H, H, wave, i, h, row, c8, last_rule);
    // the block's share of the deleted graph's readout
    rb_readout_share(Tin, H, tid, p.rpart + ((size_t)q * p.wmax + rb) * H);
}

// The finish launch of the virtual-graph forwards (gnm_virtual_forward)
struct OcFinArgs {
    const int32_t* node_off; const int32_t* vgraph;
    const int32_t* kept;                          // [V]: nodes left in virtual graph q, or null: n - 1
    const float* rpart;                           // [L][V][wmax][H]
    const long long* table;
    int V, wmax, L, m, H, graph_avg;
    int ncls; int cls[kOcMaxClasses];
    float* out; long long ldo;                    // out[ci * ldo + q]
};

__device__ __forceinline__ void oc_finish(const OcFinArgs& p) {
    extern __shared__ float gfl[];                // [L * H]
    const int q = blockIdx.x, tid = threadIdx.x;
    const int b = p.vgraph[q];
    const int n = p.node_off[b + 1] - p.node_off[b];
    const int W = (n + 31) >> 5, H = p.H, LH = p.L * p.H;
    // the reference stores 1./len(graph.g) as fp32 (graphcnn.py:123,130)
    const float scale = p.graph_avg ? 1.0f / (float)(p.kept ? p.kept[q] : n - 1) : 1.f;
    for (int e = tid; e < LH; e += 256) {
        const int l = e / H, c = e - l * H;
        float s = rb_readout_sum(p.rpart, p.V, q, p.wmax, W, H, l, c);
        if (p.graph_avg) s *= scale;
        gfl[e] = s;
    }
    __syncthreads();
    const int lane = tid & 63, wave = tid >> 6;   // a wave per class
    for (int ci = wave; ci < p.ncls; ci += 4) {
        const float acc = rb_readout_head(gfl, p.table, p.L, p.m, H, p.cls[ci], lane);
        if (lane == 0) p.out[(size_t)ci * p.ldo + q] = acc;
    }
}
// One finish under the name of each forward (profiles and the code-object tests know a forward's launches by its name)
__global__ void __launch_bounds__(256) gnm_occlusion_finish_kernel(const OcFinArgs p) { oc_finish(p); }
__global__ void __launch_bounds__(256) gnm_lesion_finish_kernel(const OcFinArgs p) { oc_finish(p); }
__global__ void __launch_bounds__(256) gnm_disconnect_finish_kernel(const OcFinArgs p) { oc_finish(p); }

// Floats of scratch gnm_occlusion / gnm_lesion need: two [rows, H] activation arrays (rows = sum of n_g^2 over the batch
// / of n_g over the virtual graphs) and the readout shares [L][V][ceil(n_max / 32)][H] (occlusion: V = N virtual graphs).
extern "C" long long gnm_occlusion_scratch_floats(long long rows, long long V, int n_max, int H, int L) {
    if (rows < 0 || V < 0 || n_max < 0 || H < 0 || L < 0) return 0;
    return 2 * rows * H + (long long)L * V * ((n_max + 31) / 32) * H;
}

// What gnm_occlusion, gnm_lesion and gnm_disconnect share on the host: the checks of the arguments all have (`a` holds
// the call's own, filled by the entry; own_ok(ctx): the entry's further BAD_ARG conditions, asked where those return),
// the split of `scratch`, the ping-pong layer launches through launch(ctx, first, grid, stream) -- `a` is part of *ctx
// -- and the finish launches under the name `finish` says, 8 classes at a time.  kept: OcFinArgs'.
extern "C" __attribute__((visibility("hidden"))) int gnm_virtual_forward(
    RbVirtualArgs* a, int B, int n_max, long long V, long long rows, int C, const int* classes_host, int n_classes,
    int graph_avg, RbFinish finish, const int32_t* kept, float* scratch, float* out, long long ldo, hipStream_t s,
    bool (*own_ok)(const void* ctx), void (*launch)(const void* ctx, bool first, unsigned grid, hipStream_t s),
    const void* ctx) {
    const int H = a->H, L = a->L, m = a->m;
    if (B == 0 || V == 0) return GNM_OK;
    if (!(H == 32 || H == 64 || H == 128) || m < 1 || m > 3 || L < 1 || L > 16 || C < 1 || C > 256 || n_max < 2 ||
        n_max > kRbMaxN)
        return GNM_ERR_UNSUPPORTED;
    if (B < 0 || V < 0 || rows < V || ldo < V || !classes_host || n_classes < 1) return GNM_ERR_BAD_ARG;
    for (int k = 0; k < n_classes; ++k)
        if (classes_host[k] < 0 || classes_host[k] >= C) return GNM_ERR_BAD_ARG;
    if (!a->adj_bits || !a->b_bits_off || !a->node_off || !a->vgraph || !a->vrow_off || !a->XW || !a->table || !scratch ||
        !out || a->ldxw < H || !own_ok(ctx))
        return GNM_ERR_BAD_ARG;
    if (reinterpret_cast<uintptr_t>(a->adj_bits) & 15) return GNM_ERR_UNSUPPORTED;
    const int wmax = (n_max + 31) / 32;
    if (V * wmax >= (1LL << 31)) return GNM_ERR_UNSUPPORTED;
    float* act[2] = {scratch, scratch + (size_t)rows * H};
    float* rpart = scratch + 2 * (size_t)rows * H;
    a->V = (int)V; a->wmax = wmax;
    for (int l = 0; l < L; ++l) {
        a->l = l;
        a->Hin = act[(l + 1) & 1];
        a->Hout = act[l & 1];
        a->rpart = rpart + (size_t)l * V * wmax * H;
        launch(ctx, l == 0, (unsigned)(V * wmax), s);
        GNM_CHECK_LAUNCH();
    }
    for (int c0 = 0; c0 < n_classes; c0 += kOcMaxClasses) {
        OcFinArgs f;
        memset(&f, 0, sizeof(f));
        f.node_off = a->node_off; f.vgraph = a->vgraph; f.kept = kept; f.rpart = rpart; f.table = a->table;
        f.V = (int)V; f.wmax = wmax; f.L = L; f.m = m; f.H = H; f.graph_avg = graph_avg;
        f.ncls = n_classes - c0 < kOcMaxClasses ? n_classes - c0 : kOcMaxClasses;
        for (int k = 0; k < f.ncls; ++k) f.cls[k] = classes_host[c0 + k];
        f.out = out + (size_t)c0 * ldo; f.ldo = ldo;
        void (*fin)(const OcFinArgs) = finish == kRbFinishDisconnect ? gnm_disconnect_finish_kernel
                                       : finish == kRbFinishLesion   ? gnm_lesion_finish_kernel
                                                                     : gnm_occlusion_finish_kernel;
        hipLaunchKernelGGL(fin, dim3((unsigned)V), dim3(256), (size_t)L * H * 4, s, f);
        GNM_CHECK_LAUNCH();
    }
    return GNM_OK;
}

// The class scores of every node-deleted copy of every graph of a batch (see the file header and include/gnm_hip.h).
extern "C" int gnm_occlusion(const uint32_t* adj_bits, const int64_t* b_bits_off, const int32_t* node_off,
                             const int32_t* rowptr, const int64_t* b_rp_off, const int32_t* vgraph,
                             const int64_t* vrow_off, int B, int n_max, long long V, long long rows, const float* XW,
                             int ldxw, const float* S, int lds, int H, int L, int m, int C, const int* classes_host,
                             int n_classes, int average, int self_loop, int graph_avg, float bn_eps,
                             const long long* table, const float* eps, float* scratch, float* out, long long ldo,
                             void* stream) {
    OcArgs a;
    memset(&a, 0, sizeof(a));
    a.adj_bits = adj_bits; a.b_bits_off = b_bits_off; a.node_off = node_off; a.vgraph = vgraph; a.vrow_off = vrow_off;
    a.XW = XW; a.ldxw = ldxw; a.L = L; a.m = m; a.H = H;
    a.average = average; a.self_loop = self_loop; a.bn_eps = bn_eps; a.eps = eps; a.table = table;
    a.rowptr = rowptr; a.b_rp_off = b_rp_off; a.S = S; a.lds = lds;
    return gnm_virtual_forward(
        &a, B, n_max, V, rows, C, classes_host, n_classes, graph_avg, kRbFinishOcclusion, nullptr, scratch, out, ldo,
        reinterpret_cast<hipStream_t>(stream),
        [](const void* ctx) {
            const OcArgs& o = *static_cast<const OcArgs*>(ctx);
            return o.rowptr && o.b_rp_off && o.S && o.lds >= o.H;
        },
        [](const void* ctx, bool first, unsigned grid, hipStream_t s) {
            const OcArgs& o = *static_cast<const OcArgs*>(ctx);
            if (first) hipLaunchKernelGGL(gnm_occlusion_layer_kernel<true>, dim3(grid), dim3(256), 0, s, o);
            else hipLaunchKernelGGL(gnm_occlusion_layer_kernel<false>, dim3(grid), dim3(256), 0, s, o);
        },
        &a);
}
