// Evaluation encoder, one launch PER LAYER with one workgroup per 32-row block of a graph (round 3): the L GIN layers
// of GIN_InfoMaxReg.forward in eval() mode (/root/reference models/graphcnn.py:208-231 with BatchNorm on its running
// statistics, mlp.py:40-49) for the reference's evaluation pattern -- one graph per forward (main.py:49-57, :71-82).
//
// Why a third form: replayed through the training kernels such a forward is ~100 dependent launches (~190 us of GPU time
// per 400-node graph); the one-workgroup-per-graph encoder (evalfwd.hip) is one launch but runs the whole graph's matrix
// work on ONE CU (~200 us).  Here a layer is one launch whose grid is (graph, 32-row block): 13 workgroups per 400-node
// graph run on 13 CUs, and the only thing a row block needs from the others is the previous layer's activations -- which
// the launch boundary provides.  Per workgroup (4 waves):
//   A. aggregation of its 32 output rows, operand roles swapped (Y^T = H^T x Adj^T): the activations are the A operand,
//      loaded straight from global memory as "eight consecutive rows of one column per lane" (4-byte loads with
//      lane = column), split in registers into three exact bf16 planes; the block's adjacency bits are the B operand
//      (expanded through a 16-entry LDS table, as csrc/aggm.hip does).  The waves split (column tile, k range); partial
//      tiles meet in LDS, where the self term / degree division are applied.
//   B. the MLP on the 32 x F tile in LDS: each Linear as the six-term split-precision product (csrc/linear.hip), A
//      fragments from the LDS tile, W rows straight from global memory, bias + folded BatchNorm + ReLU on the way back
//      into LDS; the last Linear's epilogue applies the layer's outer BatchNorm + ReLU, writes the block's rows of the
//      hidden layer and its share of the graph readout (fixed order).
// A last small launch adds the readout shares, applies the classifier head (graphcnn.py:224-231, dropout off) and
// sigmoid(g_f) (:239).  Arithmetic is fp32-faithful (three-plane splits, fp32 accumulation): results agree with the
// training kernels to fp32 rounding, not bitwise.
#include "gnm_rowblock.h"
#include <string.h>

struct ElArgs {
    const uint32_t* adj_bits; const int64_t* b_bits_off; const int32_t* node_off;
    const int32_t* rowptr; const int64_t* b_rp_off;
    const float* Hin; int ldin, Fin;
    int B, wmax, L, m, l, H;
    int average, self_loop;
    float bn_eps;
    const float* eps;                             // [L] on the device, or null (learn_eps False)
    const long long* table;
    float* Hout; int ldh;
    float* rpart;                                 // [B][wmax][H]: this layer's readout shares
};

__global__ void __launch_bounds__(256) gnm_eval_layer_kernel(const ElArgs p) {
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
    const int b = blockIdx.x / p.wmax, rb = blockIdx.x - b * p.wmax;
    const int row0 = p.node_off[b];
    const int n = p.node_off[b + 1] - row0;
    const int W = (n + 31) >> 5;
    if (rb >= W) return;                          // (also an empty graph: no rows, no readout share)
    const int H = p.H, Fin = p.Fin;
    rb_lut_init(lut, tid);
    RbMlp M;
    rb_mlp_prefetch<0>(M, aff, p.table, p.l, p.m, p.bn_eps, H, Fin, tid, wave, i, h);
    // ---- A. aggregation ----------------------------------------------------------------------------------------
    const int NCA = Fin <= 32 ? 1 : (Fin <= 64 ? 2 : 4);          // column tiles of the input; the rest of the waves split k
    // the combine pass's own operands (8 threads per tile row): this thread's elements of the self term and its row's
    // degree -- requested now, used after the product (fetched inside the combine loop they were eight dependent
    // round trips to L2)
    const int row = tid >> 3, c8 = tid & 7;
    const int grow = row0 + min(rb * 32 + row, n - 1);
    const bool vrow = rb * 32 + row < n;
    // (parked in the second LDS tile, which the MLP does not touch before the combine pass has read it)
    for (int c = c8; c < NCA * 32; c += 8)
        T1[row * kRbTS + c] = c < Fin ? p.Hin[(size_t)grow * p.ldin + c] : 0.f;
    float deg = 1.f;
    if (p.average) {
        const int32_t* rp = p.rowptr + p.b_rp_off[b];
        const int vr = min(rb * 32 + row, n - 1);
        deg = (float)(rp[vr + 1] - rp[vr] + p.self_loop);
    }
    rb_stage_bits(bitsw, p.adj_bits + p.b_bits_off[b], rb, i, h, rb_half_words(W), tid);
    rb_rows_product(part, lut, bitsw, p.Hin + (size_t)row0 * p.ldin, p.ldin, n, Fin, NCA, tid, wave, i, h);
    __syncthreads();
    {
        const int KP = (Fin + 15) & ~15;                          // the first Linear's contraction width (zero padded)
        const int KS = 4 / NCA;
        const float selfw = p.eps ? 1.f + p.eps[p.l] : 1.f;       // graphcnn.py:161 (1 + eps[layer]) h
        for (int c = c8; c < NCA * 32; c += 8) {
            float v = 0.f;
            for (int k = 0; k < KS; ++k) v += part[(c >> 5) + NCA * k][row][c & 31];
            v = rb_pool_combine<false>(v, T1[row * kRbTS + c], deg, selfw, p.self_loop, p.average);
            if (c < KP) T0[row * kRbTS + c] = (vrow && c < Fin) ? v : 0.f;
        }
    }
    // ---- B. the MLP: the last Linear's epilogue writes the block's rows of the hidden layer ----------------------
    float* Tin = T0;
    float* Tout = T1;
    rb_mlp_forward<0>(M, aff, part, Tin, Tout, p.m, H, Fin, wave, i, h, row, c8, [&](int c, float y) {
        if (vrow) p.Hout[(size_t)grow * p.ldh + c] = y;
        else y = 0.f;                                             // (rows past n: not part of the readout)
        return y;
    });
    rb_readout_share(Tin, H, tid, p.rpart + ((size_t)b * p.wmax + rb) * H);
}

struct ElFinArgs {
    const int32_t* node_off;
    const float* rpart;                           // [L][B][wmax][H]
    const long long* table;
    int B, wmax, L, m, H, C, graph_avg;
    float* g_f; int ldgf;
    float* c_sig;
    float* c_logit; int ldc;
};

__global__ void __launch_bounds__(256) gnm_eval_finish_kernel(const ElFinArgs p) {
    extern __shared__ float gfl[];                // [L * H]
    const int b = blockIdx.x, tid = threadIdx.x;
    const int n = p.node_off[b + 1] - p.node_off[b];
    const int W = (n + 31) >> 5, H = p.H, LH = p.L * p.H;
    for (int e = tid; e < LH; e += 256) {
        const int l = e / H, c = e - l * H;
        float s = rb_readout_sum(p.rpart, p.B, b, p.wmax, W, H, l, c);
        if (p.graph_avg) s *= 1.0f / (float)n;    // the reference stores 1./len(graph.g) as fp32 (graphcnn.py:123,130)
        gfl[e] = s;
        p.g_f[(size_t)b * p.ldgf + e] = s;
        if (p.c_sig) p.c_sig[(size_t)b * p.ldgf + e] = 1.f / (1.f + expf(-s));
    }
    __syncthreads();
    const int lane = tid & 63, wave = tid >> 6;   // a wave per class
    for (int cls = wave; cls < p.C; cls += 4) {
        const float acc = rb_readout_head(gfl, p.table, p.L, p.m, H, cls, lane);
        if (lane == 0) p.c_logit[(size_t)b * p.ldc + cls] = acc;
    }
}

// Floats of scratch gnm_eval_layers needs (the readout shares of every layer).
extern "C" long long gnm_eval_layers_scratch_floats(int B, int n_max, int H, int L) {
    return (long long)L * B * ((n_max + 31) / 32) * H;
}

// The eval-mode encoder + readout + classifier of B graphs as L + 1 launches (see the file header).  Arguments as
// gnm_eval_encoder (evalfwd.hip; the same DEVICE parameter table), with `scratch` (gnm_eval_layers_scratch_floats) in
// place of its two [N, H] arrays.  H in {32, 64, 128}, 1 <= m <= 3, F0 <= 128, C <= 256, every graph with a bit adjacency
// and at most 416 nodes: GNM_ERR_UNSUPPORTED otherwise (the caller then runs the layer-by-layer path).
extern "C" int gnm_eval_layers(const uint32_t* adj_bits, const int64_t* b_bits_off, const int32_t* node_off,
                               const int32_t* rowptr, const int64_t* b_rp_off, int B, int n_max, const float* X, int ldx,
                               int F0, int H, int L, int m, int C, int average, int self_loop, int graph_avg,
                               float bn_eps, const long long* table, const float* eps, float* hidden,
                               long long hidden_stride, int ldh, float* scratch, float* g_f, int ldgf, float* c_sig,
                               float* c_logit, int ldc, void* stream) {
    if (B <= 0) return GNM_OK;
    if (!(H == 32 || H == 64 || H == 128) || m < 1 || m > 3 || L < 1 || L > 16 || F0 < 1 || F0 > kRbMaxH || C < 1 || C > 256 ||
        n_max < 1 || n_max > kRbMaxN)
        return GNM_ERR_UNSUPPORTED;
    if (!adj_bits || !b_bits_off || !node_off || !rowptr || !b_rp_off || !X || !table || !hidden || !scratch || !g_f || !c_logit)
        return GNM_ERR_BAD_ARG;
    if (reinterpret_cast<uintptr_t>(adj_bits) & 15) return GNM_ERR_UNSUPPORTED;
    if ((long long)(n_max + 64) * (ldx > ldh ? ldx : ldh) * 4 >= (1LL << 31)) return GNM_ERR_UNSUPPORTED;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const int wmax = (n_max + 31) / 32;
    for (int l = 0; l < L; ++l) {
        ElArgs a;
        memset(&a, 0, sizeof(a));
        a.adj_bits = adj_bits; a.b_bits_off = b_bits_off; a.node_off = node_off; a.rowptr = rowptr; a.b_rp_off = b_rp_off;
        a.Hin = l == 0 ? X : hidden + (size_t)(l - 1) * hidden_stride;
        a.ldin = l == 0 ? ldx : ldh;
        a.Fin = l == 0 ? F0 : H;
        a.B = B; a.wmax = wmax; a.L = L; a.m = m; a.l = l; a.H = H;
        a.average = average; a.self_loop = self_loop; a.bn_eps = bn_eps;
        a.eps = eps;
        a.table = table;
        a.Hout = hidden + (size_t)l * hidden_stride; a.ldh = ldh;
        a.rpart = scratch + (size_t)l * B * wmax * H;
        hipLaunchKernelGGL(gnm_eval_layer_kernel, dim3(B * wmax), dim3(256), 0, s, a);
        GNM_CHECK_LAUNCH();
    }
    ElFinArgs f;
    f.node_off = node_off; f.rpart = scratch; f.table = table; f.B = B; f.wmax = wmax; f.L = L; f.m = m; f.H = H; f.C = C;
    f.graph_avg = graph_avg; f.g_f = g_f; f.ldgf = ldgf; f.c_sig = c_sig; f.c_logit = c_logit; f.ldc = ldc;
    hipLaunchKernelGGL(gnm_eval_finish_kernel, dim3(B), dim3(256), (size_t)L * H * 4, s, f);
    GNM_CHECK_LAUNCH();
    return GNM_OK;
}
