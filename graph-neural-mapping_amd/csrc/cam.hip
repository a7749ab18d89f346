// Eval-mode per-node class activation maps, batched: the `class_activation` vector that the reference's
// models/graphcnn.py:288 allocates in compute_saliency and never fills, plotted as method 'cam' by
// evaluate/visualize_saliency.py:33.  For graph g, node v and class c
//     cam[v] = p_g * sum_l < h_l[v], linears_prediction[l].weight[c] >,
// p_g = 1 (sum readout) or the fp32 1/n_g (average readout, graphcnn.py:123,130) -- the node's share of the eval logit:
// sum_v cam[v] + sum_l bias_l[c] = c_logit[g, c] (graphcnn.py:226-231 with dropout off).
//
// One launch after the eval forward (gnm/core.py encoder_forward), one workgroup (4 waves) per (graph, 64-row block).
// h_l = relu(z_l * scale_l + shift_l) is re-formed from the pre-BatchNorm output of the layer's last Linear and its
// folded BatchNorm, exactly as gnm_bn_relu_readout forms it (NaN-propagating ReLU).  8 lanes per row, each lane a
// float4 column chunk every 8 chunks; the 8 partial dots are reduced by a fixed butterfly, layers are summed in order
// 0 .. L-1, and every output is written by one lane: no atomics, the result is deterministic.  Nothing but z, scale,
// shift, the classifier rows and node_off is read, so the adjacency form (bits, CSR, max pooling) does not matter.
#include "gnm_common.h"
#include <string.h>

static constexpr int kCamMaxH = 128;
static constexpr int kCamMaxC = 8;                // classes per launch
static constexpr int kCamMaxL = 16;
static constexpr int kCamWords = 6;               // per layer: z, ld z, scale, shift, classifier weight, its ld
static constexpr int kCamRows = 64;               // rows per workgroup: 256 threads / 8 lanes x 2 rows per lane group

struct CamArgs {
    const int32_t* node_off;
    const long long* table;
    float* out;
    long long ldo;
    int wmax, L, H, ncls, graph_avg;
    int cls[kCamMaxC];
};

__global__ void __launch_bounds__(256) gnm_class_activation_kernel(const CamArgs p) {
    __shared__ __attribute__((aligned(16))) float wsh[kCamMaxC * kCamMaxH];
    __shared__ __attribute__((aligned(16))) float ssh[2 * kCamMaxH];
    const int tid = threadIdx.x;
    const int b = blockIdx.x / p.wmax, rb = blockIdx.x - b * p.wmax;
    const int row0 = p.node_off[b];
    const int n = p.node_off[b + 1] - row0;
    if (rb * kCamRows >= n) return;               // (also an empty graph)
    const int H = p.H, H4 = H >> 2, ncls = p.ncls;
    const int c8 = tid & 7;
    const int r0 = rb * kCamRows + (tid >> 3), r1 = r0 + 32;
    const bool v0 = r0 < n, v1 = r1 < n;
    const size_t g0 = (size_t)row0 + (v0 ? r0 : 0), g1 = (size_t)row0 + (v1 ? r1 : 0);
    float acc0[kCamMaxC], acc1[kCamMaxC];
#pragma unroll
    for (int j = 0; j < kCamMaxC; ++j) { acc0[j] = 0.f; acc1[j] = 0.f; }
    for (int l = 0; l < p.L; ++l) {               // workgroup-uniform
        const long long* te = p.table + (size_t)l * kCamWords;
        const float* z = reinterpret_cast<const float*>(te[0]);
        const long long ldz = te[1];
        const float* sc = reinterpret_cast<const float*>(te[2]);
        const float* sh = reinterpret_cast<const float*>(te[3]);
        const float* wp = reinterpret_cast<const float*>(te[4]);
        const long long ldw = te[5];
        __syncthreads();                          // the previous layer's reads of the staged rows are done
        for (int k = tid; k < ncls * H; k += 256) {
            const int j = k / H, c = k - j * H;
            wsh[j * kCamMaxH + c] = wp[(size_t)p.cls[j] * ldw + c];
        }
        for (int k = tid; k < H; k += 256) { ssh[k] = sc[k]; ssh[kCamMaxH + k] = sh[k]; }
        __syncthreads();
        float d0[kCamMaxC], d1[kCamMaxC];
#pragma unroll
        for (int j = 0; j < kCamMaxC; ++j) { d0[j] = 0.f; d1[j] = 0.f; }
        for (int q = c8; q < H4; q += 8) {
            const float4 s4 = *reinterpret_cast<const float4*>(ssh + 4 * q);
            const float4 t4 = *reinterpret_cast<const float4*>(ssh + kCamMaxH + 4 * q);
            float4 a = *reinterpret_cast<const float4*>(z + g0 * ldz + 4 * q);
            float4 c = *reinterpret_cast<const float4*>(z + g1 * ldz + 4 * q);
            a.x = gnm_relu(a.x * s4.x + t4.x); a.y = gnm_relu(a.y * s4.y + t4.y);        // graphcnn.py:163-166
            a.z = gnm_relu(a.z * s4.z + t4.z); a.w = gnm_relu(a.w * s4.w + t4.w);
            c.x = gnm_relu(c.x * s4.x + t4.x); c.y = gnm_relu(c.y * s4.y + t4.y);
            c.z = gnm_relu(c.z * s4.z + t4.z); c.w = gnm_relu(c.w * s4.w + t4.w);
#pragma unroll
            for (int j = 0; j < kCamMaxC; ++j) {
                if (j < ncls) {
                    const float4 w = *reinterpret_cast<const float4*>(wsh + j * kCamMaxH + 4 * q);
                    d0[j] += a.x * w.x + a.y * w.y + a.z * w.z + a.w * w.w;
                    d1[j] += c.x * w.x + c.y * w.y + c.z * w.z + c.w * w.w;
                }
            }
        }
#pragma unroll
        for (int j = 0; j < kCamMaxC; ++j) {
            if (j < ncls) {                       // the 8 lanes of a row: a fixed butterfly, every lane the same sum
                d0[j] += __shfl_xor(d0[j], 4, 8); d1[j] += __shfl_xor(d1[j], 4, 8);
                d0[j] += __shfl_xor(d0[j], 2, 8); d1[j] += __shfl_xor(d1[j], 2, 8);
                d0[j] += __shfl_xor(d0[j], 1, 8); d1[j] += __shfl_xor(d1[j], 1, 8);
                acc0[j] += d0[j]; acc1[j] += d1[j];
            }
        }
    }
    const float pg = p.graph_avg ? 1.0f / (float)n : 1.f;   // the readout's fp32 1/n (graphcnn.py:123,130)
#pragma unroll
    for (int j = 0; j < kCamMaxC; ++j) {
        if (j < ncls && c8 == 0) {
            if (v0) p.out[(size_t)j * p.ldo + row0 + r0] = pg * acc0[j];
            if (v1) p.out[(size_t)j * p.ldo + row0 + r1] = pg * acc1[j];
        }
    }
}

// Words of the device parameter table gnm_class_activation reads (see include/gnm_hip.h).
extern "C" long long gnm_class_activation_table_words(int L) { return (long long)L * kCamWords; }

// Classes one gnm_class_activation call can serve.
extern "C" int gnm_class_activation_max_classes(void) { return kCamMaxC; }

extern "C" int gnm_class_activation(const int32_t* node_off, int B, int n_max, long long N, int H, int L, int C,
                                    const int* cls, int ncls, int graph_avg, const long long* table, float* out,
                                    long long ldo, void* stream) {
    if (B < 0 || n_max < 0 || N < 0 || H < 4 || H > kCamMaxH || (H & 3) || L < 1 || L > kCamMaxL || C < 1 ||
        ncls < 1 || ncls > kCamMaxC || !cls || ldo < N)
        return GNM_ERR_BAD_ARG;
    for (int j = 0; j < ncls; ++j)
        if (cls[j] < 0 || cls[j] >= C) return GNM_ERR_BAD_ARG;
    if (B == 0 || N == 0) return GNM_OK;
    if (n_max < 1 || !node_off || !table || !out) return GNM_ERR_BAD_ARG;
    CamArgs a;
    memset(&a, 0, sizeof(a));
    a.node_off = node_off; a.table = table; a.out = out; a.ldo = ldo;
    a.wmax = (n_max + kCamRows - 1) / kCamRows;
    a.L = L; a.H = H; a.ncls = ncls; a.graph_avg = graph_avg;
    for (int j = 0; j < ncls; ++j) a.cls[j] = cls[j];
    if ((long long)B * a.wmax >= (1LL << 31)) return GNM_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(gnm_class_activation_kernel, dim3(B * a.wmax), dim3(256), 0,
                       reinterpret_cast<hipStream_t>(stream), a);
    GNM_CHECK_LAUNCH();
    return GNM_OK;
}
