// Eval-mode input saliency, batched: d score[b, cls] / d X for every graph b of a batch (/root/reference
// models/graphcnn.py:254-266, called per graph and class from main.py:60-68).  The gradient mirror of evallayer.hip:
// one launch per GIN layer from the top layer down, one workgroup (4 waves) per (graph, 32-row block), then one launch
// that forms dX.
//
// In eval mode the chain is linear: BatchNorm on its running statistics is a per-column scale (gamma * rstd, the
// `scale` vector the forward's gnm_bn_finalize wrote), ReLU a fixed mask (z * scale + shift > 0, the test norm.hip and
// agg.hip apply in their backwards), the aggregation its transpose, a Linear dX = dZ W.  Per workgroup of layer l:
//   A. the transposed aggregation of the layer above's gradient (l < L - 1): Y = Adj^T S over the block's 32 rows,
//      S = dpooled_{l+1} / deg (written so by the launch above), as evallayer.hip's stage A with the TRANSPOSED bit
//      matrix (three exact bf16 planes of S times the 0/1 bits, fp32 accumulation); the self term (S for self loops,
//      (1 + eps_{l+1}) dpooled_{l+1} otherwise) is added in the combine pass;
//   B. plus the head term linears_prediction[l].weight[cls] (x 1/n under average graph pooling), then the outer
//      BatchNorm + ReLU: dZ = mask * scale;
//   C. the MLP backward, Linear m-1 down to 1 (down to 0 for l > 0): dX_k = dZ_k W_k with W in torch layout [out, in]
//      read as the B operand (the six-term split-precision product of evallayer.hip), the inner BatchNorm's mask and
//      scale between Linears;
//   D. the block's rows of S_l = g / deg (and of g itself where the self term needs it), g = dpooled_l -- or, for
//      l = 0, the gradient at the first Linear's OUTPUT: by linearity (Adj^T + (1+e) I)(dZ W0) = ((Adj^T + (1+e) I) dZ) W0,
//      so the final launch aggregates at width H and multiplies by W0 last, instead of aggregating F0-wide rows.
// The masks come from the pre-BatchNorm outputs z of every Linear, which the eval forward (gnm/core.py encoder_forward)
// leaves in memory anyway.
// gnm_saliency_maps runs the same layer launches (kMaps = true) to form the gradient class activation map
// sum_l <dscore/dh_l[v], h_l[v]> in stage B instead of dX: L launches, no final one.
#include "gnm_rowblock.h"
#include <string.h>

static constexpr int kSlMaxL = 16;              // layers (the S / R placement arrays of the launchers)
static constexpr int kSlLinWords = 6;             // per (layer, Linear): W, ld W, z, ld z, scale, shift

extern "C" int gnm_linear_max_k(int H);

struct SlArgs {
    const uint32_t* adj_bits; const int64_t* b_tbits_off; const int32_t* node_off;
    const int32_t* rowptr; const int64_t* b_rp_off;
    int B, wmax, L, m, l, H, F0, cls;
    int average, self_loop, graph_avg;
    const float* eps;                             // [L] on the device, or null (learn_eps False)
    const long long* table;                       // gnm_saliency_table_words(L, m) words
    const float* Sin; const float* Rin;           // the layer above's S = dpooled / deg and dpooled (Rin: average with
                                                  // learned eps only); null for the top layer
    float* Sout; float* Rout;                     // this layer's (l > 0: of dpooled_l; l = 0: of the first Linear's dZ)
    int lds;                                      // leading dimension of S / R
    float* out; int ldo;                          // the final launch: dX [N, F0]
    int final_launch;
    float* gcam;                                  // gnm_saliency_maps: OUTPUT [N], the gradient class activation map
};

// kMaps (gnm_saliency_maps): stage B also forms the row's gradient class activation <dscore/dh_l[v], h_l[v]>
// (graphcnn.py:284,289) and stores (top layer) or adds it to p.gcam[v]; layer 0 stops there.  kMaps = false is
// gnm_saliency's kernel, whose code the other form leaves as it was.
template <bool kMaps>
__global__ void __launch_bounds__(256) gnm_saliency_layer_kernel(const SlArgs p) {
    __shared__ __attribute__((aligned(16))) float T0[32 * kRbTS];
    __shared__ __attribute__((aligned(16))) float T1[32 * kRbTS];
    __shared__ __attribute__((aligned(16))) float part[4][32][33];
    __shared__ __attribute__((aligned(16))) char lut[128];
    __shared__ unsigned bitsw[8][256];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int i = lane & 31, h = lane >> 5;
    const int b = blockIdx.x / p.wmax, rb = blockIdx.x - b * p.wmax;
    const int row0 = p.node_off[b];
    const int n = p.node_off[b + 1] - row0;
    const int W = (n + 31) >> 5;
    if (rb >= W) return;                          // (also an empty graph)
    const int H = p.H, l = p.l;
    const int ksteps = (n + 15) >> 4;
    rb_lut_init(lut, tid);
    // the combine passes: 8 threads per tile row
    const int row = tid >> 3, c8 = tid & 7;
    const int vr = min(rb * 32 + row, n - 1);
    const int grow = row0 + vr;
    const bool vrow = rb * 32 + row < n;
    const float deg = p.average ? (float)(p.rowptr[p.b_rp_off[b] + vr + 1] - p.rowptr[p.b_rp_off[b] + vr] + p.self_loop)
                                : 1.f;
    const int NCT = H >> 5, KSB = 4 / NCT;
    // ---- A. Y = Adj^T S over the block's rows (the layer above's gradient, or layer 0's for the final launch) -----
    const bool agg = p.Sin != nullptr;
    if (agg) {
        const int ct = wave % NCT, kh = wave / NCT;
        rb_stage_bits(bitsw, p.adj_bits + p.b_tbits_off[b], rb, i, h, rb_half_words(W), tid);
        // rows past n read zero: the row offset travels in the VECTOR offset, which the descriptor's range check covers
        const unsigned sbytes = (unsigned)(((size_t)(n - 1) * p.lds + H) * 4);
        const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(
            const_cast<float*>(p.Sin) + (size_t)row0 * p.lds, 0, (int)sbytes, 0x00020000);
        const unsigned svo = (unsigned)((8 * h * p.lds + 32 * ct + i) * 4);
        const unsigned srow = (unsigned)(p.lds * 4);
        f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.f;
        __syncthreads();                                          // the table
        auto request = [&](float (&d)[8], int s) {
#pragma unroll
            for (int j = 0; j < 8; ++j)
                d[j] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rs, svo + (unsigned)(16 * s + j) * srow, 0, 0));
        };
        rb_bits_product(acc, request, kh, KSB, ksteps, lut, bitsw, tid);
        // accumulator (r, lane): column 32 ct + (r & 3) + 8 (r >> 2) + 4 h of S, output row i
        rb_acc_to_part_rows(part, wave, i, h, acc);
    }
    __syncthreads();
    // ---- B. gradient at h_l (or, final launch, at pooled_0 before W0) -> T0 --------------------------------------
    {
        const int le = p.final_launch ? 0 : l + 1;               // the aggregation that read this layer's output
        const float selfw = p.eps ? 1.f + p.eps[le] : 1.f;       // graphcnn.py:161 (1 + eps[layer]) h
        const long long* te = p.table + (size_t)(l * p.m + p.m - 1) * kSlLinWords;
        const float* zo = reinterpret_cast<const float*>(te[2]);
        const float* sco = reinterpret_cast<const float*>(te[4]);
        const float* sho = reinterpret_cast<const float*>(te[5]);
        const int ldz = (int)te[3];
        const long long* th = p.table + (size_t)p.L * p.m * kSlLinWords + 2 * l;
        const float* wpred = reinterpret_cast<const float*>(th[0]) + (size_t)p.cls * th[1];
        const float inv_n = p.graph_avg ? 1.0f / (float)n : 1.f;  // the readout's fp32 1/n (graphcnn.py:123,130)
        float dot = 0.f;                                          // (kMaps) this lane's part of <g, h_l> for the row
        for (int c = c8; c < H; c += 8) {
            float g = 0.f;
            if (agg) {
                float v = 0.f;
                for (int q = 0; q < KSB; ++q) v += part[(c >> 5) + NCT * q][row][c & 31];
                const float s = p.Sin[(size_t)grow * p.lds + c];
                if (p.self_loop) v += s;
                else v += selfw * (p.Rin ? p.Rin[(size_t)grow * p.lds + c] : s);
                g = v;
            }
            if (!p.final_launch) {
                g += wpred[c] * inv_n;                             // graphcnn.py:228-231, eval: no dropout
                const float z = zo[(size_t)grow * ldz + c], sc = sco[c];
                const float y = z * sc + sho[c];
                if constexpr (kMaps) dot += g * gnm_relu(y);       // g = dscore / dh_l, before the mask
                g = (y > 0.f) ? g * sc : 0.f;                      // outer BatchNorm + ReLU (graphcnn.py:163-166)
            }
            T0[row * kRbTS + c] = vrow ? g : 0.f;
        }
        if constexpr (kMaps) {                                    // the row's 8 lanes: a fixed butterfly
            dot += __shfl_xor(dot, 4, 8);
            dot += __shfl_xor(dot, 2, 8);
            dot += __shfl_xor(dot, 1, 8);
            if (c8 == 0 && vrow) p.gcam[grow] = l == p.L - 1 ? dot : p.gcam[grow] + dot;   // layers L-1 .. 0, in order
            if (l == 0) return;                                   // layer 0's map term needs no gradient below it
        }
    }
    // ---- C. the MLP backward: dX_k = dZ_k W_k (W [out, in] as the B operand), inner BatchNorm + ReLU between -------
    float* Tin = T0;
    float* Tout = T1;
    const int kstop = l == 0 ? 1 : 0;
    if (!p.final_launch) {
        const int ct = wave % NCT, kh = wave / NCT;
        const int ncol = 32 * ct + i;
        const int nst = H >> 4;
        for (int k = p.m - 1; k >= kstop; --k) {                 // workgroup-uniform
            const long long* te = p.table + (size_t)(l * p.m + k) * kSlLinWords;
            const float* Wk = reinterpret_cast<const float*>(te[0]);
            const int ldw = (int)te[1];
            __syncthreads();                                      // the input tile complete
            f32x16 acc;
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma nounroll
            for (int s = kh; s < nst; s += KSB) {
                const int k0 = 16 * s + 8 * h;
                float fb[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) fb[j] = Wk[(size_t)(k0 + j) * ldw + ncol];
                gnm_tile_step(acc, Tin, kRbTS, i, h, s, fb);
            }
            rb_acc_to_part_cols(part, wave, i, h, acc);
            __syncthreads();
            const float* zp = nullptr; const float* scp = nullptr; const float* shp = nullptr;
            int ldz = 0;
            if (k > 0) {                                          // the inner BatchNorm + ReLU of Linear k - 1 (mlp.py:48)
                const long long* tp = p.table + (size_t)(l * p.m + k - 1) * kSlLinWords;
                zp = reinterpret_cast<const float*>(tp[2]); ldz = (int)tp[3];
                scp = reinterpret_cast<const float*>(tp[4]); shp = reinterpret_cast<const float*>(tp[5]);
            }
            for (int c = c8; c < H; c += 8) {
                float v = 0.f;
                for (int q = 0; q < KSB; ++q) v += part[(c >> 5) + NCT * q][row][c & 31];
                if (k > 0) {
                    const float z = zp[(size_t)grow * ldz + c], sc = scp[c];
                    v = (z * sc + shp[c] > 0.f) ? v * sc : 0.f;
                }
                Tout[row * kRbTS + c] = vrow ? v : 0.f;
            }
            float* t = Tin; Tin = Tout; Tout = t;
        }
        // ---- D. S = g / deg (and g where the self term of the launch below needs it) -------------------------
        __syncthreads();
        if (vrow) {
            for (int c = c8; c < H; c += 8) {
                const float g = Tin[row * kRbTS + c];
                p.Sout[(size_t)grow * p.lds + c] = p.average ? g / deg : g;
                if (p.Rout) p.Rout[(size_t)grow * p.lds + c] = g;
            }
        }
        return;
    }
    // ---- the final launch: dX = Y W0 over F0 columns, W0 [H, F0] as the B operand --------------------------------
    __syncthreads();
    const long long* t0 = p.table;
    const float* W0 = reinterpret_cast<const float*>(t0[0]);
    const int ldw0 = (int)t0[1];
    const int F0 = p.F0;
    const int NCO = (F0 + 31) >> 5;
    const int nst = H >> 4;
    if (NCO >= 4) {                               // a wave per column tile, whole contraction, straight to memory
        for (int ct = wave; ct < NCO; ct += 4) {  // wave-uniform
            const int ncol = 32 * ct + i;
            f32x16 acc;
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma nounroll
            for (int s = 0; s < nst; ++s) {
                const int k0 = 16 * s + 8 * h;
                float fb[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) fb[j] = ncol < F0 ? W0[(size_t)(k0 + j) * ldw0 + ncol] : 0.f;
                gnm_tile_step(acc, Tin, kRbTS, i, h, s, fb);
            }
            if (ncol < F0) {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int rr = rb * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
                    if (rr < n) p.out[(size_t)(row0 + rr) * p.ldo + ncol] = acc[r];
                }
            }
        }
        return;
    }
    {                                             // 1..3 column tiles: the waves split the contraction
        const int KS = 4 / NCO;
        const int ct = wave % NCO, kh = wave / NCO;
        const int ncol = 32 * ct + i;
        f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.f;
        if (ct < NCO && kh < KS) {                // (NCO = 3: the fourth wave idles)
#pragma nounroll
            for (int s = kh; s < nst; s += KS) {
                const int k0 = 16 * s + 8 * h;
                float fb[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) fb[j] = ncol < F0 ? W0[(size_t)(k0 + j) * ldw0 + ncol] : 0.f;
                gnm_tile_step(acc, Tin, kRbTS, i, h, s, fb);
            }
        }
        rb_acc_to_part_cols(part, wave, i, h, acc);
        __syncthreads();
        if (vrow) {
            for (int c = c8; c < F0; c += 8) {
                float v = 0.f;
                for (int q = 0; q < KS; ++q) v += part[(c >> 5) + NCO * q][row][c & 31];
                p.out[(size_t)grow * p.ldo + c] = v;
            }
        }
    }
}

// Words of the device parameter table gnm_saliency reads (see include/gnm_hip.h).
extern "C" long long gnm_saliency_table_words(int L, int m) { return (long long)L * m * kSlLinWords + 2LL * L; }

// Floats of scratch gnm_saliency needs for N rows of hidden width H: two (S, R) pairs, one per parity of the layer.
extern "C" long long gnm_saliency_scratch_floats(long long N, int H) { return 4 * N * (long long)H; }

// The checks gnm_saliency, gnm_saliency_maps and gnm_edge_saliency share, then the SlArgs all their launches share
// (F0 = 0, gcam = null).  The steps run in one order -- shape (UNSUPPORTED), arguments and null pointers (BAD_ARG),
// alignment, sizes (UNSUPPORTED) -- and an entry's own conditions join the step they belong to (bad_shape, bad_arg,
// null_arg, misaligned), so an input gets the same code from every entry.  row_floats: the widest row, in floats, of
// the entry's N-row arrays.
static int sl_setup(SlArgs& a, const uint32_t* adj_bits, const int64_t* b_tbits_off, const int32_t* node_off,
                    const int32_t* rowptr, const int64_t* b_rp_off, int B, int n_max, long long N, int H, int L, int m,
                    int C, int cls, int average, int self_loop, int graph_avg, const long long* table, const float* eps,
                    const float* scratch, bool bad_shape, bool bad_arg, bool null_arg, bool misaligned,
                    long long row_floats) {
    if (!(H == 32 || H == 64 || H == 128) || m < 1 || m > 3 || L < 1 || L > kSlMaxL || n_max < 1 || n_max > kRbMaxN ||
        C < 1 || bad_shape)
        return GNM_ERR_UNSUPPORTED;
    if (cls < 0 || cls >= C || N < 1 || bad_arg) return GNM_ERR_BAD_ARG;
    if (!adj_bits || !b_tbits_off || !node_off || !rowptr || !b_rp_off || !table || !scratch || null_arg)
        return GNM_ERR_BAD_ARG;
    if ((reinterpret_cast<uintptr_t>(adj_bits) & 15) || misaligned) return GNM_ERR_UNSUPPORTED;
    if ((long long)(n_max + 128) * H * 4 >= (1LL << 31) || N * row_floats >= (1LL << 40)) return GNM_ERR_UNSUPPORTED;
    memset(&a, 0, sizeof(a));
    a.adj_bits = adj_bits; a.b_tbits_off = b_tbits_off; a.node_off = node_off; a.rowptr = rowptr; a.b_rp_off = b_rp_off;
    a.B = B; a.wmax = (n_max + 31) / 32; a.L = L; a.m = m; a.H = H; a.cls = cls;
    a.average = average; a.self_loop = self_loop; a.graph_avg = graph_avg;
    a.eps = eps; a.table = table; a.lds = H;
    return GNM_OK;
}

// gnm_saliency's scratch placement: two (S, R) pairs, layer l on pair l & 1.  R only where average pooling without
// self loops needs the undivided gradient (1 + eps) dpooled.
static void sl_pingpong(float** S, float** R, float* scratch, long long N, int H, int L, bool need_r) {
    for (int l = 0; l < L; ++l) {
        S[l] = scratch + 2 * (l & 1) * N * H;
        R[l] = need_r ? scratch + (2 * (l & 1) + 1) * N * H : nullptr;
    }
}

// The L layer launches from the top layer down: layer l reads the layer above's S[l + 1] / R[l + 1] (none for the top
// layer) and writes its own to S[l] / R[l] (null: not kept).
template <bool kMaps>
static int sl_layers(SlArgs& a, float* const* S, float* const* R, hipStream_t s) {
    for (int l = a.L - 1; l >= 0; --l) {
        a.l = l;
        a.Sin = l < a.L - 1 ? S[l + 1] : nullptr;
        a.Rin = l < a.L - 1 ? R[l + 1] : nullptr;
        a.Sout = S[l];
        a.Rout = R[l];
        hipLaunchKernelGGL(gnm_saliency_layer_kernel<kMaps>, dim3(a.B * a.wmax), dim3(256), 0, s, a);
        GNM_CHECK_LAUNCH();
    }
    return GNM_OK;
}

// The final launch: dX [N, F0] from layer 0's S (and R), the gradient at the first Linear's output over a.B graphs.
static int sl_final(SlArgs& a, const float* S0, const float* R0, float* dX, int ldx, hipStream_t s) {
    a.l = 0;
    a.Sin = S0;
    a.Rin = R0;
    a.Sout = nullptr; a.Rout = nullptr;
    a.out = dX; a.ldo = ldx; a.final_launch = 1;
    hipLaunchKernelGGL(gnm_saliency_layer_kernel<false>, dim3(a.B * a.wmax), dim3(256), 0, s, a);
    GNM_CHECK_LAUNCH();
    return GNM_OK;
}

extern "C" int gnm_saliency(const uint32_t* adj_bits, const int64_t* b_tbits_off, const int32_t* node_off,
                            const int32_t* rowptr, const int64_t* b_rp_off, int B, int n_max, long long N, int F0, int H,
                            int L, int m, int C, int cls, int average, int self_loop, int graph_avg,
                            const long long* table, const float* eps, float* scratch, float* dX, int ldx, void* stream) {
    if (B <= 0) return GNM_OK;
    SlArgs a;
    int rc = sl_setup(a, adj_bits, b_tbits_off, node_off, rowptr, b_rp_off, B, n_max, N, H, L, m, C, cls, average,
                      self_loop, graph_avg, table, eps, scratch, F0 < 1 || F0 > gnm_linear_max_k(H), ldx < F0, !dX,
                      false, ldx > H ? ldx : H);
    if (rc != GNM_OK) return rc;
    a.F0 = F0;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    float* S[kSlMaxL];
    float* R[kSlMaxL];
    sl_pingpong(S, R, scratch, N, H, L, average && !self_loop);
    if ((rc = sl_layers<false>(a, S, R, s)) != GNM_OK) return rc;
    return sl_final(a, S[0], R[0], dX, ldx, s);
}

extern "C" int gnm_intgrad_reduce(const float* Sv, const float* Rv, const int32_t* node_off, int B, int n_max,
                                  const float* weights, int K, int H, float* Sbar, float* Rbar, hipStream_t s);
extern "C" int gnm_intgrad_scale(float* attr, int lda, const float* X, int ldx, const float* base, int ldb,
                                 const int32_t* node_off, int B, int n_max, int F0, hipStream_t s);

// Integrated gradients of class cls (csrc/intgrad.hip, include/gnm_hip.h): gnm_saliency's layer launches over the K B
// virtual graphs (v_*: their descriptors, K consecutive ones per source graph, over the forward that `table` describes),
// layer 0's S (and R) reduced over the steps with the quadrature weights, then ONE final launch over the B source
// graphs and the (X - baseline) pass.  The checks are gnm_saliency's, in its order, on the source batch and then on the
// virtual one.
extern "C" int gnm_integrated_gradients(const uint32_t* adj_bits, const int64_t* b_tbits_off, const int32_t* node_off,
                                        const int32_t* rowptr, const int64_t* b_rp_off, int B, int n_max, long long N,
                                        int F0, int H, int L, int m, int C, int cls, int average, int self_loop,
                                        int graph_avg, const long long* table, const float* eps, float* scratch,
                                        const int64_t* v_tbits_off, const int32_t* v_node_off, const int64_t* v_rp_off,
                                        int K, const float* weights, const float* X, int ldxin, const float* base,
                                        int ldb, int n_base, float* attr, int lda, void* stream) {
    if (B <= 0) return GNM_OK;
    SlArgs a, v;
    const bool bad_shape = F0 < 1 || F0 > gnm_linear_max_k(H);
    const bool bad_arg = lda < F0 || ldxin < F0 || K < 1 || (base && (ldb < F0 || n_base < n_max));
    const bool null_arg = !attr || !X || !weights || !v_tbits_off || !v_node_off || !v_rp_off;
    const long long row_floats = lda > H ? lda : H;
    int rc = sl_setup(a, adj_bits, b_tbits_off, node_off, rowptr, b_rp_off, B, n_max, N, H, L, m, C, cls, average,
                      self_loop, graph_avg, table, eps, scratch, bad_shape, bad_arg, null_arg, false, row_floats);
    if (rc != GNM_OK) return rc;
    const long long Nv = N * K;                   // virtual rows are indexed in int32, as node_off is
    if (K > (1 << 20) || Nv >= (1LL << 31) || (long long)B * K >= (1LL << 31) / a.wmax) return GNM_ERR_UNSUPPORTED;
    rc = sl_setup(v, adj_bits, v_tbits_off, v_node_off, rowptr, v_rp_off, B * K, n_max, Nv, H, L, m, C, cls, average,
                  self_loop, graph_avg, table, eps, scratch, false, false, false,
                  (reinterpret_cast<uintptr_t>(scratch) & 15) != 0, H);
    if (rc != GNM_OK) return rc;
    a.F0 = F0;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const bool need_r = average && !self_loop;
    float* S[kSlMaxL];
    float* R[kSlMaxL];
    sl_pingpong(S, R, scratch, Nv, H, L, need_r);
    if ((rc = sl_layers<false>(v, S, R, s)) != GNM_OK) return rc;
    float* Sbar = scratch + 4 * Nv * H;
    float* Rbar = need_r ? Sbar + N * H : nullptr;
    if ((rc = gnm_intgrad_reduce(S[0], R[0], node_off, B, n_max, weights, K, H, Sbar, Rbar, s)) != GNM_OK) return rc;
    if ((rc = sl_final(a, Sbar, Rbar, attr, lda, s)) != GNM_OK) return rc;
    return gnm_intgrad_scale(attr, lda, X, ldxin, base, ldb, node_off, B, n_max, F0, s);
}

// The gradient class activation map of class cls (graphcnn.py:284,288-289): gcam[v] = sum_l <dscore/dh_l[v], h_l[v]>.
// gnm_saliency's layer launches with the map formed in stage B; no dX launch, and layer 0 stops after stage B.
extern "C" int gnm_saliency_maps(const uint32_t* adj_bits, const int64_t* b_tbits_off, const int32_t* node_off,
                                 const int32_t* rowptr, const int64_t* b_rp_off, int B, int n_max, long long N, int H,
                                 int L, int m, int C, int cls, int average, int self_loop, int graph_avg,
                                 const long long* table, const float* eps, float* scratch, float* gcam, void* stream) {
    if (B <= 0) return GNM_OK;
    SlArgs a;
    const int rc = sl_setup(a, adj_bits, b_tbits_off, node_off, rowptr, b_rp_off, B, n_max, N, H, L, m, C, cls, average,
                            self_loop, graph_avg, table, eps, scratch, false, false, !gcam, false, H);
    if (rc != GNM_OK) return rc;
    a.gcam = gcam;
    float* S[kSlMaxL];
    float* R[kSlMaxL];
    sl_pingpong(S, R, scratch, N, H, L, average && !self_loop);
    return sl_layers<true>(a, S, R, reinterpret_cast<hipStream_t>(stream));
}

extern "C" int gnm_edge_saliency_contract(const uint32_t* adj_bits, const int64_t* b_bits_off, const int32_t* node_off,
                                          const int32_t* rowptr, const int64_t* b_rp_off, int B, int n_max, long long N,
                                          int H, int L, int m, int average, int self_loop, const long long* table,
                                          const float* S, const float* Y, int ldy, float* out, long long ldo,
                                          hipStream_t s);

// Floats of scratch gnm_edge_saliency needs: every layer's S_l (L x [N, H]) and one (R) pair.
extern "C" long long gnm_edge_saliency_scratch_floats(long long N, int H, int L) {
    return (long long)(L + 2) * N * (long long)H;
}

// The connectivity saliency of class cls (edgesal.hip): out[u, v] = d score / d A[u, v] over every node pair of each
// graph.  gnm_saliency's layer launches with each layer's S_l in a buffer of its own (layer 0's: dZ_0 / deg) and no dX
// launch, then one contraction launch.
extern "C" int gnm_edge_saliency(const uint32_t* adj_bits, const int64_t* b_bits_off, const int64_t* b_tbits_off,
                                 const int32_t* node_off, const int32_t* rowptr, const int64_t* b_rp_off, int B,
                                 int n_max, long long N, int H, int L, int m, int C, int cls, int average,
                                 int self_loop, int graph_avg, const long long* table, const float* eps,
                                 float* scratch, const float* Y, int ldy, float* out, long long ldo, void* stream) {
    if (B <= 0) return GNM_OK;
    SlArgs a;
    int rc = sl_setup(a, adj_bits, b_tbits_off, node_off, rowptr, b_rp_off, B, n_max, N, H, L, m, C, cls, average,
                      self_loop, graph_avg, table, eps, scratch, false, ldy < H || ldo < n_max, !b_bits_off || !Y || !out,
                      (reinterpret_cast<uintptr_t>(Y) & 15) || (ldy & 3), (long long)H * (L + 2));
    if (rc != GNM_OK) return rc;
    if (N * ldo >= (1LL << 40)) return GNM_ERR_UNSUPPORTED;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const bool need_r = average && !self_loop;
    float* S[kSlMaxL];
    float* R[kSlMaxL];
    for (int l = 0; l < L; ++l) {                 // R: one pair after the L S_l; layer 0 writes none (no layer below)
        S[l] = scratch + (size_t)l * N * H;
        R[l] = need_r && l > 0 ? scratch + (size_t)(L + (l & 1)) * N * H : nullptr;
    }
    if ((rc = sl_layers<false>(a, S, R, s)) != GNM_OK) return rc;
    return gnm_edge_saliency_contract(adj_bits, b_bits_off, node_off, rowptr, b_rp_off, B, n_max, N, H, L, m, average,
                                      self_loop, table, scratch, Y, ldy, out, ldo, s);
}
