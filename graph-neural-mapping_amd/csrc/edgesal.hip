// Eval-mode connectivity saliency, batched: d score[b, cls] / d A[u, v] for every graph b of a batch and EVERY pair
// (u, v) of its nodes, A the dense form of the reference's Adj_block (models/graphcnn.py:84-106: 1 at every edge_mat
// pair, row u = destination, plus the diagonal when learn_eps is False), shared by all L layers
// (pooled_l = A h_{l-1}, :154-161 / :178-182) and, under neighbour "average", by the degree d = A 1 (:158-160, :182-184).
//
// With G_l = d score / d pooled_l, h_{-1} = X:
//   sum:     out[u, v] = sum_l <G_l[u], h_{l-1}[v]>
//   average: out[u, v] = sum_l (<G_l[u], h_{l-1}[v]> - <G_l[u], pooled_avg_l[u]>) / d_u
// gnm_edge_saliency (saliency.hip) runs gnm_saliency's layer launches with every layer's S_l = G_l / d (G_l under sum
// pooling) kept, layer 0's being dZ_0 / d at the first Linear's output: <G_0[u], X[v]> = <dZ_0[u], Y[v]>, Y = X W0^T.
// This kernel then forms, per workgroup of (graph, 32-row block), the [32, n] strip of
//   E[u, v] = sum_l <S_l[u], h_{l-1}[v]>          (a GEMM with K = L H; h_{l-1} = relu(z * scale + shift) of layer
//                                                  l-1's last Linear, re-formed as the forward does; Y for l = 0)
// as split-bf16 MFMA products with fp32 accumulation (the six-term split of gnm_split.h), and writes
//   sum:     out = E
//   average: out[u, v] = E[u, v] - c[u],  c[u] = (1 / d_u) sum_w A[u, w] E[u, w]   (a masked row mean of the strip)
// Every output element is written once, from LDS, with a fixed summation order: deterministic, no atomics.
#include "gnm_rowblock.h"

static constexpr int kEsLinWords = 6;             // gnm_saliency's table: per (layer, Linear) W, ld W, z, ld z, scale, shift
static constexpr int kEsMaxTiles = (kRbMaxN + 31) / 32 / 4 + 1;   // 32-column tiles per wave (13 tiles, 4 waves: 4)

struct EsArgs {
    const uint32_t* adj_bits; const int64_t* b_bits_off;    // the FORWARD bit rows (row u: the v with A[u, v] = 1)
    const int32_t* node_off; const int32_t* rowptr; const int64_t* b_rp_off;
    int wmax, L, m, H, average, self_loop;
    const long long* table;                       // gnm_saliency_table_words(L, m) words
    const float* S; long long s_layer;            // S_l = S + l * s_layer, [N, H] row-contiguous
    const float* Y; int ldy;                      // X W0^T, [N, H]
    float* out; long long ldo;                    // OUTPUT: graph b's row u at out + (node_off[b] + u) * ldo
    int lde;                                      // row stride of the E strip in LDS (floats)
};

__global__ void __launch_bounds__(256) gnm_edge_saliency_kernel(const EsArgs p) {
    extern __shared__ __attribute__((aligned(16))) float es_smem[];
    float* Ts = es_smem;                          // [32][kRbTS]: the block's rows of S_l
    float* Es = es_smem + 32 * kRbTS;             // [32][lde]: the E strip
    float* cs = Es + 32 * p.lde;                  // [32]: the average pooling's row correction
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int i = lane & 31, h = lane >> 5;
    const int b = blockIdx.x / p.wmax, rb = blockIdx.x - b * p.wmax;
    const int row0 = p.node_off[b];
    const int n = p.node_off[b + 1] - row0;
    const int W = (n + 31) >> 5;                  // 32-column tiles = 32-row blocks of the graph
    if (rb >= W) return;                          // (also an empty graph)
    const int H = p.H;
    const int row = tid >> 3, c8 = tid & 7;       // the staging passes: 8 threads per tile row
    const bool vrow = rb * 32 + row < n;
    const int vr = min(rb * 32 + row, n - 1);
    f32x16 acc[kEsMaxTiles];
#pragma unroll
    for (int t = 0; t < kEsMaxTiles; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
    // this lane's B rows, one per tile (rows past n repeat row n - 1: their columns are never written)
    int vcol[kEsMaxTiles];
#pragma unroll
    for (int t = 0; t < kEsMaxTiles; ++t) vcol[t] = row0 + min(32 * (wave + 4 * t) + i, n - 1);
    for (int l = 0; l < p.L; ++l) {               // workgroup-uniform
        __syncthreads();                          // the previous layer's tile reads complete
        {
            const float* srow = p.S + (size_t)l * p.s_layer + (size_t)(row0 + vr) * H;
            for (int c = 4 * c8; c < H; c += 32) {
                float4 v = *reinterpret_cast<const float4*>(srow + c);
                if (!vrow) v = make_float4(0.f, 0.f, 0.f, 0.f);
                *reinterpret_cast<float4*>(Ts + row * kRbTS + c) = v;
            }
        }
        const float* src; int lds;
        const float* sc = nullptr; const float* sh = nullptr;
        if (l == 0) {
            src = p.Y; lds = p.ldy;
        } else {                                  // h_{l-1}: layer l-1's last Linear, its outer BatchNorm + ReLU
            const long long* te = p.table + (size_t)((l - 1) * p.m + p.m - 1) * kEsLinWords;
            src = reinterpret_cast<const float*>(te[2]); lds = (int)te[3];
            sc = reinterpret_cast<const float*>(te[4]); sh = reinterpret_cast<const float*>(te[5]);
        }
        __syncthreads();                          // the tile
#pragma nounroll
        for (int s = 0; s < (H >> 4); ++s) {
            const int k0 = 16 * s + 8 * h;
            gnm_bf16x8 a1, a2, a3;
            gnm_tile_split(Ts, kRbTS, i, h, s, a1, a2, a3);
            float scv[8], shv[8];
            if (sc) {
                const float4 s0 = *reinterpret_cast<const float4*>(sc + k0), s1 = *reinterpret_cast<const float4*>(sc + k0 + 4);
                const float4 t0 = *reinterpret_cast<const float4*>(sh + k0), t1 = *reinterpret_cast<const float4*>(sh + k0 + 4);
                scv[0] = s0.x; scv[1] = s0.y; scv[2] = s0.z; scv[3] = s0.w; scv[4] = s1.x; scv[5] = s1.y; scv[6] = s1.z; scv[7] = s1.w;
                shv[0] = t0.x; shv[1] = t0.y; shv[2] = t0.z; shv[3] = t0.w; shv[4] = t1.x; shv[5] = t1.y; shv[6] = t1.z; shv[7] = t1.w;
            }
#pragma unroll
            for (int t = 0; t < kEsMaxTiles; ++t) {
                if (wave + 4 * t >= W) break;     // wave-uniform
                const float* r = src + (size_t)vcol[t] * lds + k0;
                const float4 v0 = *reinterpret_cast<const float4*>(r);
                const float4 v1 = *reinterpret_cast<const float4*>(r + 4);
                float fb[8] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w};
                if (sc) {
#pragma unroll
                    for (int j = 0; j < 8; ++j) fb[j] = gnm_relu(fb[j] * scv[j] + shv[j]);   // graphcnn.py:163-166
                }
                gnm_bf16x8 b1, b2, b3;
                gnm_split8(fb, b1, b2, b3);
                gnm_mma6(acc[t], a1, a2, a3, b1, b2, b3);
            }
        }
    }
    // accumulator (r, lane) of tile t: row (r & 3) + 8 (r >> 2) + 4 h of the block, column 32 t' + i, t' = wave + 4 t
#pragma unroll
    for (int t = 0; t < kEsMaxTiles; ++t) {
        if (wave + 4 * t >= W) break;
#pragma unroll
        for (int r = 0; r < 16; ++r) Es[((r & 3) + 8 * (r >> 2) + 4 * h) * p.lde + 32 * (wave + 4 * t) + i] = acc[t][r];
    }
    __syncthreads();
    if (p.average) {                              // c[u] = (1 / d_u) sum_w A[u, w] E[u, w], 8 lanes per row
        const int HPW = rb_half_words(W);
        const uint32_t* brow = p.adj_bits + p.b_bits_off[b] + (size_t)(rb * 32 + row) * (2 * HPW);
        const float* er = Es + row * p.lde;
        float sum = 0.f;
        for (int j = c8; 8 * j < n; j += 8) {     // byte j of the row: columns 8 j .. 8 j + 7
            const unsigned byte = (brow[(j & 1) * HPW + (j >> 3)] >> (8 * ((j >> 1) & 3))) & 0xFFu;
#pragma unroll
            for (int k = 0; k < 8; ++k)
                if (byte & (1u << k)) sum += er[8 * j + k];
        }
        sum += __shfl_xor(sum, 4, 8);             // the row's 8 lanes: a fixed butterfly
        sum += __shfl_xor(sum, 2, 8);
        sum += __shfl_xor(sum, 1, 8);
        if (c8 == 0) {
            if (p.self_loop) sum += er[rb * 32 + row];                 // the diagonal (graphcnn.py:97-102)
            const float deg = (float)(p.rowptr[p.b_rp_off[b] + vr + 1] - p.rowptr[p.b_rp_off[b] + vr] + p.self_loop);
            cs[row] = sum / deg;
        }
        __syncthreads();
    }
    // the strip, a row per wave at a time: 64 consecutive columns per store
    for (int rr = wave; rr < 32; rr += 4) {
        const int u = rb * 32 + rr;
        if (u >= n) break;                        // wave-uniform
        const float cu = p.average ? cs[rr] : 0.f;
        float* orow = p.out + (size_t)(row0 + u) * p.ldo;
        for (int v = lane; v < n; v += 64) orow[v] = Es[rr * p.lde + v] - cu;
    }
}

// LDS bytes of gnm_edge_saliency_kernel for graphs of at most n_max nodes
static size_t es_lds_bytes(int n_max, int* lde) {
    *lde = 32 * ((n_max + 31) / 32) + 4;
    return (size_t)(32 * kRbTS + 32 * *lde + 32) * sizeof(float);
}

// The contraction of gnm_edge_saliency (saliency.hip), after its layer launches; arguments as there, checked there.
extern "C" __attribute__((visibility("hidden"))) int gnm_edge_saliency_contract(
    const uint32_t* adj_bits, const int64_t* b_bits_off, const int32_t* node_off, const int32_t* rowptr,
    const int64_t* b_rp_off, int B, int n_max, long long N, int H, int L, int m, int average, int self_loop,
    const long long* table, const float* S, const float* Y, int ldy, float* out, long long ldo, hipStream_t s) {
    if (n_max < 1 || n_max > kRbMaxN || !(H == 32 || H == 64 || H == 128)) return GNM_ERR_UNSUPPORTED;
    EsArgs a;
    a.adj_bits = adj_bits; a.b_bits_off = b_bits_off; a.node_off = node_off; a.rowptr = rowptr; a.b_rp_off = b_rp_off;
    a.wmax = (n_max + 31) / 32; a.L = L; a.m = m; a.H = H; a.average = average; a.self_loop = self_loop;
    a.table = table; a.S = S; a.s_layer = N * (long long)H; a.Y = Y; a.ldy = ldy; a.out = out; a.ldo = ldo;
    const size_t lds = es_lds_bytes(n_max, &a.lde);
    GNM_ALLOW_FULL_LDS(gnm_edge_saliency_kernel);
    hipLaunchKernelGGL(gnm_edge_saliency_kernel, dim3(B * a.wmax), dim3(256), lds, s, a);
    GNM_CHECK_LAUNCH();
    return GNM_OK;
}
