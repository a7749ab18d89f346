// Virtual lesions of ROI SETS: the eval-mode class scores of set-deleted copies G \ D of the graphs of a batch
// (GIN_InfoMaxReg.lesion() / deletion_curve(); the reference's forward in eval(), graphcnn.py:194-231, on a graph with
// the nodes of D, their feature rows and their edges in both directions removed), without building a single copy.
//
// A VIRTUAL graph is (source graph g, removed set D), 0 <= |D| <= n_g - 1: it reads g's bit rows and owns n_g rows of
// two ping-pong activation arrays and a KEEP MASK in the bit adjacency's own half-row layout (2 rb_half_words(W) words,
// bit of column v where rb_row_bit finds it, zero at columns >= n).  The contract and the structure are
// csrc/occlusion.hip's with v replaced by D (bits as the B operand of the aggregation, three exact bf16 planes, the
// six-term split Linears from the LDS tile, folded BatchNorm, the NaN-propagating ReLU); what a set changes:
//   * the block's adjacency words are ANDed with the mask on their way to LDS (rb_stage_bits_masked), so the product
//     drops the columns of D, and a row's degree under neighbour "average" is the popcount of its masked words
//     (+ 1 under self loops) -- the reduced graph's own degree, 0 / 0 -> NaN for a kept row whose neighbours are all in
//     D under learned eps, as the reference computes it on the explicit copy;
//   * rows of D (and rows past n) are written as ZEROS in every layer's output and are left out of the readout, which
//     runs over kept = n - |D| nodes (graph "average": the fp32 1 / kept);
//   * layer 0 runs the masked product too: occlusion's subtraction S[r] - a_rv XW[v] does not extend to sets without
//     one.  The caller forms XW = X W0^T once per SOURCE graph (any input width); layer 0 computes (A & keep) XW over
//     the source graph's rows, adds the self term or (1 + eps0) XW[r], divides by the degree and applies the first
//     Linear's bias and folded BatchNorm -- the first Linear commutes with the pooling.
// gnm_lesion_pack builds the masks and the kept counts on the device from a uint8 "removed" array.  One launch per
// layer over (virtual graph, 32-row block), then a launch that adds the readout shares in fixed order and applies the
// classifier head.  No float atomics; every sum has a fixed order, so results are bitwise reproducible and do not
// depend on how the caller chunks the virtual graphs or on which other sets share the call.
#include "gnm_rowblock.h"
#include <string.h>

struct LsArgs : RbVirtualArgs {                   // vrow_off [V]: sum of n before virtual graph q
    const uint32_t* masks; int mstride;           // [V][mstride]: the keep masks
};

// FIRST: layer 0 (the masked product over the source graph's XW; the first Linear ran on the source graphs, its bias
// and BatchNorm are applied here); otherwise a layer >= 1 on the virtual graph's own activations.
template <bool FIRST>
__global__ void __launch_bounds__(256) gnm_lesion_layer_kernel(const LsArgs p) {
    __shared__ __attribute__((aligned(16))) float T0[32 * kRbTS];
    __shared__ __attribute__((aligned(16))) float T1[32 * kRbTS];
    __shared__ __attribute__((aligned(16))) float part[4][32][33];
    __shared__ __attribute__((aligned(16))) char lut[128];
    __shared__ unsigned bitsw[8][256];            // word j of thread t's half row of the block's MASKED adjacency bits
    __shared__ float aff[3][3][kRbMaxH];          // per Linear of the MLP: bias, scale, shift (the BatchNorm behind it, folded)
    __shared__ int degs[32];                      // the block's rows' degrees in the reduced graph (without the self loop)
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
    const uint32_t* mask = p.masks + (size_t)q * p.mstride;
    float* rdst = p.rpart + ((size_t)q * p.wmax + rb) * H;
    // a block whose rows are all removed: its zero rows and a zero readout share, no product (workgroup-uniform; the
    // block's rows are columns 32 rb .. 32 rb + 31 of the mask: two bytes of word rb >> 1 of either half)
    if ((((mask[rb >> 1] | mask[HPW + (rb >> 1)]) >> (16 * (rb & 1))) & 0xFFFFu) == 0u) {
        if (p.l + 1 < p.L) {
            const int nr = min(32, n - rb * 32);
            float* dst = p.Hout + (row0 + (size_t)rb * 32) * H;
            for (int e = tid; e < nr * H; e += 256) dst[e] = 0.f;
        }
        if (tid < H) rdst[tid] = 0.f;
        return;
    }
    rb_lut_init(lut, tid);
    // what the MLP needs that does not depend on the tile, requested now (layer 0's first Linear ran on the source graphs)
    RbMlp M;
    rb_mlp_prefetch<FIRST ? 1 : 0>(M, aff, p.table, p.l, p.m, p.bn_eps, H, H, tid, wave, i, h);
    const int NCT = M.NCT;
    // the combine pass's operands (8 threads per tile row): the row and whether it is a kept row of the graph
    const int row = tid >> 3, c8 = tid & 7;
    const int vr = min(rb * 32 + row, n - 1);
    const bool vrow = rb * 32 + row < n;
    const bool keep = vrow && rb_row_bit(mask, HPW, vr) != 0u;
    const float eps_l = p.eps ? p.eps[p.l] : 0.f;
    // what the layer's last Linear leaves of column c of this thread's row
    auto last_rule = [&](int c, float y) {
        if (!keep) y = 0.f;                                       // removed rows (and rows past n): zeros, not in the readout
        if (vrow && p.l + 1 < p.L) p.Hout[(row0 + vr) * H + c] = y;
        return y;
    };
    // ---- A. aggregation: (A & keep) x the rows of the source graph's XW (layer 0) or of the virtual graph's own
    //         activations, whose removed rows are zero (layers >= 1) -------------------------------------------------
    const int NCA = NCT;
    const float* Hg = FIRST ? p.XW + (size_t)node0 * p.ldxw : p.Hin + row0 * H;
    const int ld = FIRST ? p.ldxw : H;
    for (int c = c8; c < H; c += 8) T1[row * kRbTS + c] = Hg[(size_t)vr * ld + c];           // the self term, parked
    const int pc = rb_stage_bits_masked(bitsw, gbits, mask, rb, i, h, HPW, tid);
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
            if (!keep) t = 0.f;
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
    // the block's share of the lesioned graph's readout
    rb_readout_share(Tin, H, tid, rdst);
}

// The keep masks and kept counts of V virtual graphs from removed [V, ld] (uint8, non-zero = removed; entries at columns
// >= n are ignored).  16 lanes per virtual graph, one mask word per lane (2 x 8 words at most); the lane of word 0 adds
// the group's 16 popcounts in order.
__global__ void __launch_bounds__(256) gnm_lesion_pack_kernel(const uint8_t* removed, long long ld, const int32_t* vgraph,
                                                              const int32_t* node_off, int V, int mstride,
                                                              uint32_t* masks, int32_t* kept) {
    __shared__ int pcs[16][16];
    const int tid = threadIdx.x, grp = tid >> 4, w = tid & 15;
    const long long q = (long long)blockIdx.x * 16 + grp;
    unsigned word = 0u;
    if (q < V) {
        const int b = vgraph[q];
        const int n = node_off[b + 1] - node_off[b];
        const int HPW = rb_half_words((n + 31) >> 5);
        if (w < 2 * HPW) {
            const int hh = w / HPW, j = w - hh * HPW;
            const uint8_t* rm = removed + (size_t)q * ld;
            for (int mbyte = 0; mbyte < 4; ++mbyte) {
                const int c0 = 16 * (4 * j + mbyte) + 8 * hh;     // byte mbyte of word j of half hh: step 4 j + mbyte
                for (int k = 0; k < 8; ++k)
                    if (c0 + k < n && rm[c0 + k] == 0) word |= 1u << (8 * mbyte + k);
            }
        }
        if (w < mstride) masks[(size_t)q * mstride + w] = word;
    }
    pcs[grp][w] = __popc(word);
    __syncthreads();
    if (q < V && w == 0) {
        int s = 0;
        for (int k = 0; k < 16; ++k) s += pcs[grp][k];
        kept[q] = s;
    }
}

// Floats of scratch gnm_lesion needs: gnm_occlusion's with rows = sum of n_g over the virtual graphs.
extern "C" long long gnm_lesion_scratch_floats(long long rows, long long V, int n_max, int H, int L) {
    return gnm_occlusion_scratch_floats(rows, V, n_max, H, L);
}

// Words of a keep mask that serves graphs of up to n_max nodes: both half rows (the mstride of the two entries below)
extern "C" int gnm_lesion_mask_words(int n_max) { return 2 * rb_half_words((n_max + 31) / 32); }

// masks [V][mstride] and kept [V] of the virtual graphs from removed [V, ld] (see include/gnm_hip.h)
extern "C" int gnm_lesion_pack(const uint8_t* removed, long long ld, const int32_t* vgraph, const int32_t* node_off,
                               int B, int n_max, long long V, int mstride, uint32_t* masks, int32_t* kept,
                               void* stream) {
    if (B == 0 || V == 0) return GNM_OK;
    if (n_max < 1 || n_max > kRbMaxN) return GNM_ERR_UNSUPPORTED;
    if (B < 0 || V < 0 || ld < n_max || mstride < gnm_lesion_mask_words(n_max) || mstride > 16) return GNM_ERR_BAD_ARG;
    if (!removed || !vgraph || !node_off || !masks || !kept) return GNM_ERR_BAD_ARG;
    if ((V + 15) / 16 >= (1LL << 31)) return GNM_ERR_UNSUPPORTED;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(gnm_lesion_pack_kernel, dim3((unsigned)((V + 15) / 16)), dim3(256), 0, s, removed, ld, vgraph,
                       node_off, (int)V, mstride, masks, kept);
    GNM_CHECK_LAUNCH();
    return GNM_OK;
}

// The class scores of the set-deleted copies of the graphs of a batch (see the file header and include/gnm_hip.h).
extern "C" int gnm_lesion(const uint32_t* adj_bits, const int64_t* b_bits_off, const int32_t* node_off,
                          const int32_t* vgraph, const int64_t* vrow_off, const uint32_t* masks, int mstride,
                          const int32_t* kept, const int32_t* kept_host, const int32_t* vn_host, int B, int n_max,
                          long long V, long long rows, const float* XW, int ldxw, int H, int L, int m, int C,
                          const int* classes_host, int n_classes, int average, int self_loop, int graph_avg,
                          float bn_eps, const long long* table, const float* eps, float* scratch, float* out,
                          long long ldo, void* stream) {
    struct Call { LsArgs a; const int32_t *kept, *kept_host, *vn_host; int n_max; long long V; } k;
    memset(&k, 0, sizeof(k));
    LsArgs& a = k.a;
    a.adj_bits = adj_bits; a.b_bits_off = b_bits_off; a.node_off = node_off; a.vgraph = vgraph; a.vrow_off = vrow_off;
    a.XW = XW; a.ldxw = ldxw; a.L = L; a.m = m; a.H = H;
    a.average = average; a.self_loop = self_loop; a.bn_eps = bn_eps; a.eps = eps; a.table = table;
    a.masks = masks; a.mstride = mstride;
    k.kept = kept; k.kept_host = kept_host; k.vn_host = vn_host; k.n_max = n_max; k.V = V;
    return gnm_virtual_forward(
        &a, B, n_max, V, rows, C, classes_host, n_classes, graph_avg, kRbFinishLesion, kept, scratch, out, ldo,
        reinterpret_cast<hipStream_t>(stream),
        [](const void* ctx) {
            const Call& k = *static_cast<const Call*>(ctx);
            if (!k.a.masks || !k.kept || !k.kept_host || !k.vn_host) return false;
            if (k.a.mstride < gnm_lesion_mask_words(k.n_max) || k.a.mstride > 16) return false;
            for (long long q = 0; q < k.V; ++q)     // a virtual graph keeps 1 .. n of its nodes (gnm_lesion_pack's counts)
                if (k.vn_host[q] < 1 || k.vn_host[q] > k.n_max || k.kept_host[q] < 1 || k.kept_host[q] > k.vn_host[q])
                    return false;
            return true;
        },
        [](const void* ctx, bool first, unsigned grid, hipStream_t s) {
            const LsArgs& a = static_cast<const Call*>(ctx)->a;
            if (first) hipLaunchKernelGGL(gnm_lesion_layer_kernel<true>, dim3(grid), dim3(256), 0, s, a);
            else hipLaunchKernelGGL(gnm_lesion_layer_kernel<false>, dim3(grid), dim3(256), 0, s, a);
        },
        &k);
}
