// The building blocks of the eval-mode kernels whose workgroup (4 waves, 256 threads) owns one 32-row block of a graph
// (evallayer.hip, occlusion.hip, lesion.hip, disconnect.hip, saliency.hip, edgesal.hip; aggm.hip and evalfwd.hip take single pieces):
//   * the product of the block's adjacency BITS with rows of activations read from global memory (rb_bits_product and
//     what feeds it): the activations are the A operand, "eight consecutive rows of one column per lane", split in
//     registers into three exact bf16 planes; the bits are the B operand, expanded through a 16-entry LDS table;
//   * the two ways an accumulator goes to the part[wave] tiles in LDS where the waves' partial tiles meet;
//   * the aggregation stage of the forward layer kernels (rb_rows_product: the product over a graph's rows, to the part
//     tiles) and the pooling rule of their combine pass (rb_pool_combine);
//   * the forward MLP on the 32 x F tile in LDS (rb_mlp_*): folded BatchNorm, six-term split Linears (gnm_split.h);
//   * the readout sum and the classifier head of the finish kernels;
//   * the layer arguments that the virtual-graph forwards share (RbVirtualArgs; their finish body and host driver,
//     gnm_virtual_forward, are defined in occlusion.hip and used by lesion.hip and disconnect.hip too).
// Each kernel keeps what is its own: how it stages the bits, which rows it multiplies, its epilogue.  saliency.hip
// addresses its rows differently (the row offset in the vector offset) and keeps its own product call.
#pragma once
#include "gnm_split.h"

static constexpr int kRbMaxN = 416;               // 13 row blocks, 26 steps: a lane's half row of a block's bits is 8 words
static constexpr int kRbMaxH = 128;
static constexpr int kRbTS = kRbMaxH + 4;         // row stride of the LDS tiles (floats)
static constexpr int kRbLinWords = 7;             // the parameter table of evalfwd.hip (gnm_eval_table_words)

// words per HALF row of the bit adjacency of a graph of W row blocks (layout: aggm.hip gnm_adj_bits_build)
__host__ __device__ __forceinline__ int rb_half_words(int W) { return (((W + 1) >> 1) + 3) & ~3; }

// lut[128]: nibble e -> bf16 (bit 0, bit 1, bit 2, bit 3) as two words.  Visible after the next barrier.
__device__ __forceinline__ void rb_lut_init(char* lut, int tid) {
    if (tid < 16) {
        const unsigned one = 0x3F80u;
        gnm_u32x2 v;
        v.x = ((tid & 1) ? one : 0u) | ((tid & 2) ? one << 16 : 0u);
        v.y = ((tid & 4) ? one : 0u) | ((tid & 8) ? one << 16 : 0u);
        *reinterpret_cast<gnm_u32x2*>(lut + 8 * tid) = v;
    }
}

// This lane's half row (i, h) of block rb's adjacency bits -> LDS, one word per (word index, thread)
__device__ __forceinline__ void rb_stage_bits(unsigned (*bitsw)[256], const uint32_t* gbits, int rb, int i, int h, int HPW,
                                              int tid) {
    const gnm_u32x4* rp = reinterpret_cast<const gnm_u32x4*>(gbits + (size_t)(rb * 32 + i) * (2 * HPW) + h * HPW);
    const gnm_u32x4 z4 = {0u, 0u, 0u, 0u};
    const gnm_u32x4 a0 = rp[0];
    const gnm_u32x4 a1 = HPW > 4 ? rp[1] : z4;
#pragma unroll
    for (int j = 0; j < 4; ++j) { bitsw[j][tid] = a0[j]; bitsw[4 + j][tid] = a1[j]; }
}

// Bit of column v in a row (or a keep mask) of the half-row layout: `row` points at its 2 HPW words
__device__ __forceinline__ unsigned rb_row_bit(const uint32_t* row, int HPW, int v) {
    return (row[((v >> 3) & 1) * HPW + (v >> 6)] >> ((((v >> 4) & 3) << 3) + (v & 7))) & 1u;
}

// rb_stage_bits with every staged word ANDed with a keep mask of the same half-row layout (lesion.hip: `mask` is the
// virtual graph's 2 HPW words, a bit per kept COLUMN).  Returns the popcount of this lane's masked half row: with the
// other half's (lane ^ 32) the row's degree in the reduced graph.
__device__ __forceinline__ int rb_stage_bits_masked(unsigned (*bitsw)[256], const uint32_t* gbits, const uint32_t* mask,
                                                    int rb, int i, int h, int HPW, int tid) {
    const gnm_u32x4* rp = reinterpret_cast<const gnm_u32x4*>(gbits + (size_t)(rb * 32 + i) * (2 * HPW) + h * HPW);
    const uint32_t* mp = mask + h * HPW;
    const gnm_u32x4 z4 = {0u, 0u, 0u, 0u};
    const gnm_u32x4 a0 = rp[0];
    const gnm_u32x4 a1 = HPW > 4 ? rp[1] : z4;
    int pc = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const unsigned w0 = a0[j] & mp[j];
        const unsigned w1 = HPW > 4 ? a1[j] & mp[4 + j] : 0u;
        bitsw[j][tid] = w0; bitsw[4 + j][tid] = w1;
        pc += __popc(w0) + __popc(w1);
    }
    return pc;
}

// rb_stage_bits with a keep mask that depends on the ROW (disconnect.hip: the edges between two node sets A and B cut).
// ka / kb: the virtual graph's two masks of the half-row layout, the complements of A and of B within n (zero at
// columns >= n).  Row r = 32 rb + i is in A iff its own column is clear in ka, in B iff clear in kb; its words are ANDed
// with kb if it is in A and with ka if it is in B -- both, or neither.  The choice is per lane, so each mask word is
// selected against an all-ones word (two v_cndmask and two v_and per staged word) rather than taken as one operand.
// Rows at or past n (zero rows of the bit adjacency) are in neither set: they stage their words as rb_stage_bits does.
// Returns the popcount of this lane's masked half row, as rb_stage_bits_masked.
__device__ __forceinline__ int rb_stage_bits_cut(unsigned (*bitsw)[256], const uint32_t* gbits, const uint32_t* ka,
                                                 const uint32_t* kb, int rb, int i, int h, int HPW, int n, int tid) {
    const int r = rb * 32 + i;
    const gnm_u32x4* rp = reinterpret_cast<const gnm_u32x4*>(gbits + (size_t)r * (2 * HPW) + h * HPW);
    const int rc = min(r, n - 1);
    const bool in_a = r < n && rb_row_bit(ka, HPW, rc) == 0u;
    const bool in_b = r < n && rb_row_bit(kb, HPW, rc) == 0u;
    const uint32_t* pa = ka + h * HPW;
    const uint32_t* pb = kb + h * HPW;
    const gnm_u32x4 z4 = {0u, 0u, 0u, 0u};
    const gnm_u32x4 a0 = rp[0];
    const gnm_u32x4 a1 = HPW > 4 ? rp[1] : z4;
    int pc = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const unsigned ma0 = pa[j], mb0 = pb[j];                  // loaded whatever the row is in: no divergent load
        const unsigned w0 = a0[j] & (in_a ? mb0 : ~0u) & (in_b ? ma0 : ~0u);
        unsigned w1 = 0u;
        if (HPW > 4) {                                            // (workgroup-uniform)
            const unsigned ma1 = pa[4 + j], mb1 = pb[4 + j];
            w1 = a1[j] & (in_a ? mb1 : ~0u) & (in_b ? ma1 : ~0u);
        }
        bitsw[j][tid] = w0; bitsw[4 + j][tid] = w1;
        pc += __popc(w0) + __popc(w1);
    }
    return pc;
}

// The 8 bits of (row 32 rb + i, columns 16 s + 8 h ..) as a bf16x8 operand: byte s & 3 of word s >> 2 of the lane's half row
__device__ __forceinline__ gnm_bf16x8 rb_bits_operand(const char* lut, const unsigned (*bitsw)[256], int s, int tid) {
    const unsigned pkw = bitsw[s >> 2][tid];
    const unsigned byte3 = ((pkw >> (8 * (s & 3))) & 0xFFu) << 3;
    const unsigned lo = byte3 & 0x78u, hi = (byte3 >> 4) & 0x78u;
    const gnm_u32x2 l2 = *reinterpret_cast<const gnm_u32x2*>(lut + lo);
    const gnm_u32x2 h2 = *reinterpret_cast<const gnm_u32x2*>(lut + hi);
    const gnm_u32x4 q = {l2.x, l2.y, h2.x, h2.y};
    return __builtin_bit_cast(gnm_bf16x8, q);
}

// acc += (rows of activations)^T x bits over this wave's steps s = kh + KS u (< ksteps, wave-uniform), four to an
// iteration, three requests ahead of the one being multiplied.  request(d, s) loads step s's eight rows of the lane's
// column into d (rows past the graph: zeros) -- the one thing the kernels do differently.
// This is a real loop and must stay one: fully unrolled, 26 steps x 3 Linears were 54 KB of straight-line code that
// every workgroup ran once from a cold instruction cache -- 17 us per launch, two thirds of it instruction fetch.
template <class Request>
__device__ __forceinline__ void rb_bits_product(f32x16& acc, Request request, int kh, int KS, int ksteps, const char* lut,
                                                const unsigned (*bitsw)[256], int tid) {
    auto multiply = [&](const float (&d)[8], int s) {
        gnm_bf16x8 a1, a2, a3;
        gnm_split8(d, a1, a2, a3);
        const gnm_bf16x8 bq = rb_bits_operand(lut, bitsw, s, tid);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a3, bq, acc, 0, 0, 0);      // small planes first
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a2, bq, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1, bq, acc, 0, 0, 0);
    };
    float hb0[8], hb1[8], hb2[8], hb3[8];
    request(hb0, kh); request(hb1, kh + KS); request(hb2, kh + 2 * KS);
#pragma nounroll
    for (int s = kh; s < ksteps; s += 4 * KS) {
        request(hb3, s + 3 * KS);
        multiply(hb0, s);
        if (s + KS < ksteps) { request(hb0, s + 4 * KS); multiply(hb1, s + KS); }
        if (s + 2 * KS < ksteps) { request(hb1, s + 5 * KS); multiply(hb2, s + 2 * KS); }
        if (s + 3 * KS < ksteps) { request(hb2, s + 6 * KS); multiply(hb3, s + 3 * KS); }
    }
}

// Accumulator element (r, lane) is tile position ((r & 3) + 8 (r >> 2) + 4 h, i).  Two ways to LDS:
// lane = ROW of the part tile (rb_bits_product: output row i, input column (r ..)) ...
__device__ __forceinline__ void rb_acc_to_part_rows(float (*part)[32][33], int wave, int i, int h, const f32x16& acc) {
#pragma unroll
    for (int r = 0; r < 16; ++r) part[wave][i][(r & 3) + 8 * (r >> 2) + 4 * h] = acc[r];
}
// ... lane = COLUMN of the part tile (gnm_tile_step: tile row (r ..), output column i)
__device__ __forceinline__ void rb_acc_to_part_cols(float (*part)[32][33], int wave, int i, int h, const f32x16& acc) {
#pragma unroll
    for (int r = 0; r < 16; ++r) part[wave][(r & 3) + 8 * (r >> 2) + 4 * h][i] = acc[r];
}

// The aggregation stage of a forward layer kernel: this wave's share of (the block's bits, already staged in bitsw by
// rb_stage_bits / rb_stage_bits_masked / rb_stage_bits_cut) x (rows 0 .. n - 1 of `base`, row stride ld floats, columns 0 .. width - 1; NCA
// column tiles, the rest of the waves split k) -> part[wave].  Holds the barrier after which the lut, the staged bits
// and whatever else the caller wrote to LDS before the call are visible.
__device__ __forceinline__ void rb_rows_product(float (*part)[32][33], const char* lut, const unsigned (*bitsw)[256],
                                                const float* base, int ld, int n, int width, int NCA, int tid, int wave,
                                                int i, int h) {
    const int ksteps = (n + 15) >> 4;
    const int ct = wave % NCA, kh = wave / NCA, KS = 4 / NCA;
    const unsigned xbytes = (unsigned)(((size_t)(n - 1) * ld + width) * 4);
    const __amdgpu_buffer_rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(base), 0, (int)xbytes, 0x00020000);
    const int c = 32 * ct + i;
    const unsigned xvo = c < width ? (unsigned)((8 * h * ld + c) * 4) : 0x80000000u;   // (a column past width reads zero: past any buffer, and no wrap with the row offset)
    const int xrow = ld * 4;
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    __syncthreads();
    auto request = [&](float (&d)[8], int s) {                    // rows past n: offsets past the descriptor, zeros
#pragma unroll
        for (int j = 0; j < 8; ++j) d[j] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rx, xvo, (16 * s + j) * xrow, 0));
    };
    rb_bits_product(acc, request, kh, KS, ksteps, lut, bitsw, tid);
    // accumulator (r, lane): input column 32 ct + (r & 3) + 8 (r >> 2) + 4 h, output row i
    rb_acc_to_part_rows(part, wave, i, h, acc);
}

// The pooling rule of the combine pass for one element: t the neighbour sum (the waves' partial tiles added), hin the
// row's own input, selfw = 1 + eps[layer] (graphcnn.py:161).  ZERO_DEG: a row with no neighbour left gives 0 / 0 -> NaN
// as the reference does on the explicit copy, whatever its partial sum held.  SELF_IN_T: t already holds the self term
// (occlusion's layer 0, whose S = (A + I) XW).
template <bool ZERO_DEG, bool SELF_IN_T = false>
__device__ __forceinline__ float rb_pool_combine(float t, float hin, float deg, float selfw, int self_loop, int average) {
    if (self_loop && !SELF_IN_T) t += hin;
    if (average) {
        if (ZERO_DEG && deg == 0.f) t = 0.f;
        t /= deg;                                                 // 0 / 0 -> NaN as in the reference
    }
    if (!self_loop) t += selfw * hin;
    return t;
}

// ---- the forward MLP of a GIN layer on the 32 x F tile -------------------------------------------------------------
// What it needs that does not depend on the tile.  H = 32 NCT: the waves split (column tile ct, k range kh of KSB).
struct RbMlp {
    int NCT, KSB, ct, kh, ncol;                   // ncol: output column of this lane = row of W
    const float* W[3];
    int ldw[3];
    float fbw[3][2][8];                           // this wave's first two W fragments per Linear
};

// Requested at kernel entry: the parameter table -> the pointers -> the vectors and the W fragments are three dependent
// round trips to memory per Linear; taken one Linear at a time behind the aggregation they were most of the layer
// kernel's 17 us.  aff[k]: bias, scale, shift of Linear k (the BatchNorm behind it, folded); visible after the next
// barrier.  Linears below kFirstLinear get no fragments (their product ran elsewhere); K0: input width of Linear 0.
template <int kFirstLinear>
__device__ __forceinline__ void rb_mlp_prefetch(RbMlp& M, float (*aff)[3][kRbMaxH], const long long* table, int l, int m,
                                                float bn_eps, int H, int K0, int tid, int wave, int i, int h) {
    M.NCT = H >> 5; M.KSB = 4 / M.NCT;
    M.ct = wave % M.NCT; M.kh = wave / M.NCT;
    M.ncol = 32 * M.ct + i;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        M.W[k] = nullptr; M.ldw[k] = 0;
        if (k < m) {
            const long long* te = table + (size_t)(l * m + k) * kRbLinWords;
            M.W[k] = reinterpret_cast<const float*>(te[0]);
            M.ldw[k] = (int)te[6];
            const int K = k == 0 ? K0 : H;
            if (tid < H) {
                const float gam = reinterpret_cast<const float*>(te[2])[tid], bet = reinterpret_cast<const float*>(te[3])[tid];
                const float rm = reinterpret_cast<const float*>(te[4])[tid], rv = reinterpret_cast<const float*>(te[5])[tid];
                const float rstd = (float)(1.0 / sqrt((double)rv + (double)bn_eps));
                const float sc = gam * rstd;
                aff[k][0][tid] = reinterpret_cast<const float*>(te[1])[tid];
                aff[k][1][tid] = sc;
                aff[k][2][tid] = bet - rm * sc;
            }
            if (k >= kFirstLinear) {
#pragma unroll
                for (int u = 0; u < 2; ++u) {
                    const int k0 = 16 * (M.kh + M.KSB * u) + 8 * h;
#pragma unroll
                    for (int j = 0; j < 8; ++j) M.fbw[k][u][j] = k0 + j < K ? M.W[k][(size_t)M.ncol * M.ldw[k] + k0 + j] : 0.f;
                }
            }
        }
    }
}

// Linears kFirstLinear .. m - 1 on the tile Tin (ping-pong with Tout; both are left pointing at the result / the spare):
// each as the six-term product with W rows straight from global memory, then bias + folded BatchNorm + ReLU (mlp.py:48
// inner, graphcnn.py:163-166, 187-190 outer) back into LDS by 8 threads per tile row (row, c8).  last(c, y) -> the value
// of column c of this thread's row that the LAST Linear leaves in the tile: the kernel's own store / zeroing rule.
template <int kFirstLinear, class Last>
__device__ __forceinline__ void rb_mlp_forward(const RbMlp& M, const float (*aff)[3][kRbMaxH], float (*part)[32][33],
                                               float*& Tin, float*& Tout, int m, int H, int K0, int wave, int i, int h,
                                               int row, int c8, Last last) {
#pragma unroll
    for (int k = kFirstLinear; k < 3; ++k) {
        if (k >= m) break;                                        // workgroup-uniform
        const int K = k == 0 ? K0 : H;
        const int nst = (K + 15) >> 4;
        __syncthreads();                                          // the input tile (and, the first time, the vectors) complete
        {
            f32x16 acc;
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[r] = 0.f;
            // the wave's first two steps: W fragments requested at kernel entry; the rest (K = 128 with one k range per
            // wave) in a real loop, on demand
            if (M.kh < nst) gnm_tile_step(acc, Tin, kRbTS, i, h, M.kh, M.fbw[k][0]);
            if (M.kh + M.KSB < nst) gnm_tile_step(acc, Tin, kRbTS, i, h, M.kh + M.KSB, M.fbw[k][1]);
#pragma nounroll
            for (int s = M.kh + 2 * M.KSB; s < nst; s += M.KSB) {
                const int k0 = 16 * s + 8 * h;
                float fb[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) fb[j] = k0 + j < K ? M.W[k][(size_t)M.ncol * M.ldw[k] + k0 + j] : 0.f;
                gnm_tile_step(acc, Tin, kRbTS, i, h, s, fb);
            }
            rb_acc_to_part_cols(part, wave, i, h, acc);
        }
        __syncthreads();
        for (int c = c8; c < H; c += 8) {
            float z = aff[k][0][c];
            for (int q = 0; q < M.KSB; ++q) z += part[(c >> 5) + M.NCT * q][row][c & 31];
            float y = gnm_relu(z * aff[k][1][c] + aff[k][2][c]);
            if (k == m - 1) y = last(c, y);
            Tout[row * kRbTS + c] = y;
        }
        float* t = Tin; Tin = Tout; Tout = t;
    }
}

// The block's share of the graph readout (graphcnn.py:228-229): column sums of the tile's rows, fixed order -> dst[H]
__device__ __forceinline__ void rb_readout_share(const float* T, int H, int tid, float* dst) {
    __syncthreads();                                              // the tile complete
    if (tid < H) {
        float ssum = 0.f;
        for (int r = 0; r < 32; ++r) ssum += T[r * kRbTS + tid];
        dst[tid] = ssum;
    }
}

// ---- the finish kernels ----------------------------------------------------------------------------------------------
// Column c of layer l of the readout of graph g (of ng): the shares of its W row blocks, rpart [L][ng][wmax][H], in order
__device__ __forceinline__ float rb_readout_sum(const float* rpart, int ng, int g, int wmax, int W, int H, int l, int c) {
    float s = 0.f;
    for (int rb = 0; rb < W; ++rb) s += rpart[(((size_t)l * ng + g) * wmax + rb) * H + c];
    return s;
}

// The classifier head (graphcnn.py:224-231, eval: no dropout) for one class, by one wave: lanes over the L*H products of
// the readout gfl [L * H] in LDS; `table` is the kRbLinWords-per-Linear parameter table.  The logit, in every lane.
__device__ __forceinline__ float rb_readout_head(const float* gfl, const long long* table, int L, int m, int H, int cls,
                                                 int lane) {
    const long long* th = table + (size_t)L * m * kRbLinWords;   // per layer l: Wp, bp
    const int LH = L * H;
    float acc = 0.f;
    for (int e = lane; e < LH; e += 64) {
        const int l = e / H, c = e - l * H;
        acc += gfl[e] * reinterpret_cast<const float*>(th[2 * l])[(size_t)cls * H + c];
    }
    if (lane < L) acc += reinterpret_cast<const float*>(th[2 * lane + 1])[cls];
    return wave_sum(acc);
}

// ---- the virtual-graph forwards (occlusion.hip, lesion.hip, disconnect.hip) ------------------------------------------
// What their layer kernels' arguments share (OcArgs, LsArgs and DcArgs derive from it).  The entry fills what holds for the whole
// call; gnm_virtual_forward (occlusion.hip) checks that and fills the rest per layer.
struct RbVirtualArgs {
    const uint32_t* adj_bits; const int64_t* b_bits_off; const int32_t* node_off;
    const int32_t* vgraph;                        // [V]: source graph of virtual graph q
    const int64_t* vrow_off;                      // first activation row of a graph's virtual graphs / of a virtual graph
    const float* XW; int ldxw;                    // layer 0: X W0^T of the SOURCE graphs, [N, H]
    int L, m, H;
    int average, self_loop;
    float bn_eps;
    const float* eps;                             // [L] on the device, or null (learn_eps False)
    const long long* table;
    // per layer:
    const float* Hin;                             // layers >= 1: [rows, H]
    int V, wmax, l;
    float* Hout;                                  // [rows, H]
    float* rpart;                                 // [V][wmax][H]: this layer's readout shares
};

// Which finish kernel gnm_virtual_forward launches: one body (oc_finish) under the name of the forward it serves
enum RbFinish { kRbFinishOcclusion = 0, kRbFinishLesion = 1, kRbFinishDisconnect = 2 };

// occlusion.hip: the scratch size, and the checks, layer loop and finish launches the virtual-graph forwards share
extern "C" long long gnm_occlusion_scratch_floats(long long rows, long long V, int n_max, int H, int L);
extern "C" __attribute__((visibility("hidden"))) int gnm_virtual_forward(
    RbVirtualArgs* a, int B, int n_max, long long V, long long rows, int C, const int* classes_host, int n_classes,
    int graph_avg, RbFinish finish, const int32_t* kept, float* scratch, float* out, long long ldo, hipStream_t s,
    bool (*own_ok)(const void* ctx), void (*launch)(const void* ctx, bool first, unsigned grid, hipStream_t s),
    const void* ctx);
