// Virtual disconnection of ROI-SET PAIRS: the eval-mode class scores of edge-cut copies G (/) (A, B) of the graphs of a
// batch (GIN_InfoMaxReg.disconnect() / disconnection_matrix(); the reference's forward in eval(), graphcnn.py:194-231,
// on a graph whose edges (u, v) with (u in A and v in B) or (u in B and v in A) are removed), without building a copy.
//
// A VIRTUAL graph is (source graph g, set pair (A, B)): it reads g's bit rows and owns n_g rows of two ping-pong
// activation arrays and TWO keep masks in the bit adjacency's half-row layout, KA = the complement of A within n and KB
// likewise (gnm_lesion_pack's masks of the "removed" arrays A and B; zero at columns >= n).  The structure is
// csrc/lesion.hip's (bits as the B operand of the aggregation, three exact bf16 planes, the six-term split Linears from
// the LDS tile, folded BatchNorm, the NaN-propagating ReLU, layer 0 as the masked product over the source graph's
// XW = X W0^T); what a cut changes against a lesion:
//   * the mask depends on the ROW: row r's adjacency words are ANDed with KB if r is in A and with KA if r is in B -- both
//     if it is in both, neither if in neither (rb_stage_bits_cut).  The rule is symmetric in (A, B) and in (u, v), so a
//     directed graph needs no special case, and an explicit (v, v) edge is cut exactly when v is in A and in B.  The
//     self loop the reference adds when learn_eps is off is not a bit of the adjacency: it is never cut;
//   * a row's degree under neighbour "average" is the popcount of its masked words (+ 1 under self loops) -- the cut
//     graph's own degree, 0 / 0 -> NaN for a row left without a neighbour under learned eps, as the reference computes it
//     on the explicit copy;
//   * NO row is removed: every row of the graph keeps its features and its place in the readout, which runs over all n
//     nodes (graph "average": the fp32 1 / n; the finish takes n as its device `kept` array).  Rows past n are written
//     as zeros and stay out of the readout share.
// One launch per layer over (virtual graph, 32-row block), then a launch that adds the readout shares in fixed order and
// applies the classifier head.  No float atomics; every sum has a fixed order, so results are bitwise reproducible and
// do not depend on how the caller chunks the virtual graphs or on which other pairs share the call.
#include "gnm_rowblock.h"
#include <string.h>

struct DcArgs : RbVirtualArgs {                   // vrow_off [V]: sum of n before virtual graph q
    const uint32_t* keep_a; const uint32_t* keep_b; int mstride;   // [V][mstride] each: the complements of A and of B
};

// FIRST: layer 0 (the cut product over the source graph's XW; the first Linear ran on the source graphs, its bias and
// BatchNorm are applied here); otherwise a layer >= 1 on the virtual graph's own activations.
template <bool FIRST>
__global__ void __launch_bounds__(256) gnm_disconnect_layer_kernel(const DcArgs p) {
    __shared__ __attribute__((aligned(16))) float T0[32 * kRbTS];
    __shared__ __attribute__((aligned(16))) float T1[32 * kRbTS];
    __shared__ __attribute__((aligned(16))) float part[4][32][33];
    __shared__ __attribute__((aligned(16))) char lut[128];
    __shared__ unsigned bitsw[8][256];            // word j of thread t's half row of the block's CUT adjacency bits
    __shared__ float aff[3][3][kRbMaxH];          // per Linear of the MLP: bias, scale, shift (the BatchNorm behind it, folded)
    __shared__ int degs[32];                      // the block's rows' degrees in the cut graph (without the self loop)
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int i = lane & 31, h = lane >> 5;
    const int q = blockIdx.x / p.wmax, rb = blockIdx.x - q * p.wmax;
    const int b = p.vgraph[q];
    const int node0 = p.node_off[b];
    const int n = p.node_off[b + 1] - node0;
    const int W = (n + 31) >> 5;
    if (rb >= W) return;
    const size_t row0 = (size_t)p.vrow_off[q];                    // the virtual graph's rows of Hin / Hout
    const int H = p.H;
    const int HPW = rb_half_words(W);
    const uint32_t* gbits = p.adj_bits + p.b_bits_off[b];
    const uint32_t* ka = p.keep_a + (size_t)q * p.mstride;
    const uint32_t* kb = p.keep_b + (size_t)q * p.mstride;
    rb_lut_init(lut, tid);
    // what the MLP needs that does not depend on the tile, requested now (layer 0's first Linear ran on the source graphs)
    RbMlp M;
    rb_mlp_prefetch<FIRST ? 1 : 0>(M, aff, p.table, p.l, p.m, p.bn_eps, H, H, tid, wave, i, h);
    const int NCT = M.NCT;
    // the combine pass's operands (8 threads per tile row): the row and whether it is a row of the graph
    const int row = tid >> 3, c8 = tid & 7;
    const int vr = min(rb * 32 + row, n - 1);
    const bool vrow = rb * 32 + row < n;
    const float eps_l = p.eps ? p.eps[p.l] : 0.f;
    // what the layer's last Linear leaves of column c of this thread's row
    auto last_rule = [&](int c, float y) {
        if (!vrow) y = 0.f;                                       // rows past n: zeros, not in the readout
        if (vrow && p.l + 1 < p.L) p.Hout[(row0 + vr) * H + c] = y;
        return y;
    };
    // ---- A. aggregation: (the cut adjacency) x the rows of the source graph's XW (layer 0) or of the virtual graph's
    //         own activations (layers >= 1) ----------------------------------------------------------------------------
    const int NCA = NCT;
    const float* Hg = FIRST ? p.XW + (size_t)node0 * p.ldxw : p.Hin + row0 * H;
    const int ld = FIRST ? p.ldxw : H;
    for (int c = c8; c < H; c += 8) T1[row * kRbTS + c] = Hg[(size_t)vr * ld + c];           // the self term, parked
    const int pc = rb_stage_bits_cut(bitsw, gbits, ka, kb, rb, i, h, HPW, n, tid);
    const int pcr = pc + __shfl_xor(pc, 32, 64);                  // both halves of row 32 rb + i
    if (wave == 0 && h == 0) degs[i] = pcr;
    rb_rows_product(part, lut, bitsw, Hg, ld, n, H, NCA, tid, wave, i, h);      // (its barrier: the degrees too)
    __syncthreads();
    {
        const int KS = 4 / NCA;
        const float selfw = 1.f + eps_l;                          // graphcnn.py:161 (1 + eps[layer]) h
        const float deg = p.average ? (float)(degs[row] + p.self_loop) : 1.f;
        const bool first_last = FIRST && p.m == 1;
        for (int c = c8; c < H; c += 8) {
            float t = 0.f;
            for (int k = 0; k < KS; ++k) t += part[(c >> 5) + NCA * k][row][c & 31];
            t = rb_pool_combine<true>(t, T1[row * kRbTS + c], deg, selfw, p.self_loop, p.average);
            if (!vrow) t = 0.f;
            if (FIRST) {                                          // the first Linear's bias and folded BatchNorm
                t = gnm_relu((t + aff[0][0][c]) * aff[0][1][c] + aff[0][2][c]);
                if (first_last) t = last_rule(c, t);
            }
            T0[row * kRbTS + c] = t;
        }
    }
    // ---- B. the MLP (layer 0: from its second Linear) ----------------------------------------------------------
    float* Tin = T0;
    float* Tout = T1;
    rb_mlp_forward<FIRST ? 1 : 0>(M, aff, part, Tin, Tout, p.m, H, H, wave, i, h, row, c8, last_rule);
    // the block's share of the cut graph's readout
    rb_readout_share(Tin, H, tid, p.rpart + ((size_t)q * p.wmax + rb) * H);
}

extern "C" int gnm_lesion_mask_words(int n_max);                  // lesion.hip: the masks are gnm_lesion_pack's

// Floats of scratch gnm_disconnect needs: gnm_lesion's, with rows = sum of n_g over the virtual graphs.
extern "C" long long gnm_disconnect_scratch_floats(long long rows, long long V, int n_max, int H, int L) {
    return gnm_occlusion_scratch_floats(rows, V, n_max, H, L);
}

// The class scores of the edge-cut copies of the graphs of a batch (see the file header and include/gnm_hip.h).
extern "C" int gnm_disconnect(const uint32_t* adj_bits, const int64_t* b_bits_off, const int32_t* node_off,
                              const int32_t* vgraph, const int64_t* vrow_off, const uint32_t* keep_a,
                              const uint32_t* keep_b, int mstride, const int32_t* kept, const int32_t* vn_host, int B,
                              int n_max, long long V, long long rows, const float* XW, int ldxw, int H, int L, int m,
                              int C, const int* classes_host, int n_classes, int average, int self_loop, int graph_avg,
                              float bn_eps, const long long* table, const float* eps, float* scratch, float* out,
                              long long ldo, void* stream) {
    struct Call { DcArgs a; const int32_t *kept, *vn_host; int n_max; long long V; } k;
    memset(&k, 0, sizeof(k));
    DcArgs& a = k.a;
    a.adj_bits = adj_bits; a.b_bits_off = b_bits_off; a.node_off = node_off; a.vgraph = vgraph; a.vrow_off = vrow_off;
    a.XW = XW; a.ldxw = ldxw; a.L = L; a.m = m; a.H = H;
    a.average = average; a.self_loop = self_loop; a.bn_eps = bn_eps; a.eps = eps; a.table = table;
    a.keep_a = keep_a; a.keep_b = keep_b; a.mstride = mstride;
    k.kept = kept; k.vn_host = vn_host; k.n_max = n_max; k.V = V;
    return gnm_virtual_forward(
        &a, B, n_max, V, rows, C, classes_host, n_classes, graph_avg, kRbFinishDisconnect, kept, scratch, out, ldo,
        reinterpret_cast<hipStream_t>(stream),
        [](const void* ctx) {
            const Call& k = *static_cast<const Call*>(ctx);
            if (!k.a.keep_a || !k.a.keep_b || !k.kept || !k.vn_host) return false;
            if (k.a.mstride < gnm_lesion_mask_words(k.n_max) || k.a.mstride > 16) return false;
            for (long long q = 0; q < k.V; ++q)     // the node counts the device `kept` array repeats
                if (k.vn_host[q] < 1 || k.vn_host[q] > k.n_max) return false;
            return true;
        },
        [](const void* ctx, bool first, unsigned grid, hipStream_t s) {
            const DcArgs& a = static_cast<const Call*>(ctx)->a;
            if (first) hipLaunchKernelGGL(gnm_disconnect_layer_kernel<true>, dim3(grid), dim3(256), 0, s, a);
            else hipLaunchKernelGGL(gnm_disconnect_layer_kernel<false>, dim3(grid), dim3(256), 0, s, a);
        },
        &k);
}
