// Integrated gradients (GIN_InfoMaxReg.integrated_gradients, include/gnm_hip.h gnm_integrated_gradients): the pieces
// that surround csrc/saliency.hip's layer launches.  A VIRTUAL graph is (source graph g, quadrature step k): n_g rows
// over g's own adjacency, K of them per source graph, graph-major -- virtual graph g K + k owns rows
// K node_off[g] + k n_g .. + n_g of every virtual array.  No graph copy and no [K N, F0] feature array exists:
//   z0      layer 0 is affine in alpha because the adjacency is shared: with P = pool(X) W0^T and Q = pool(x') W0^T of
//           the SOURCE graph, the first Linear's pre-BatchNorm output of virtual row (g, k, r) is
//           alpha_k P[g, r] + (1 - alpha_k) Q[g, r] + b0;
//   reduce  gnm_saliency's final launch dX = ((Adj^T + (1 + eps0) I) dZ0 [/deg]) W0 is linear in dZ0 with an adjacency
//           common to all steps, so the steps are summed FIRST, at width H: Dbar[g, r] = sum_k w_k dZ0[(g, k), r] in
//           fixed k order (the same for the undivided copy R that average pooling with learned eps keeps), and the
//           final launch runs once per source graph;
//   scale   attr = (X - x') dX, one elementwise pass.
// All three are bandwidth-shaped: one pass, float4 rows (z0, reduce), plain vector stores, no atomics.
#include "gnm_common.h"

// element e of graph g's [n_g, H] block as (row, float4 column); false past the block
__device__ __forceinline__ bool ig_element(const int32_t* node_off, int H4, int& row0, int& n, int& r, int& c4) {
    const int g = blockIdx.y;
    row0 = node_off[g];
    n = node_off[g + 1] - row0;
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n * H4) return false;
    r = e / H4;
    c4 = e - r * H4;
    return true;
}

__global__ void __launch_bounds__(256) gnm_intgrad_z0_kernel(const float* __restrict__ P, int ldp,
                                                             const float* __restrict__ Q, int ldq,
                                                             const float* __restrict__ bias,
                                                             const int32_t* __restrict__ node_off,
                                                             const float* __restrict__ alphas, int K, int H4,
                                                             float* __restrict__ Z, int ldz) {
    int row0, n, r, c4;
    if (!ig_element(node_off, H4, row0, n, r, c4)) return;
    const float4 p = *reinterpret_cast<const float4*>(P + (size_t)(row0 + r) * ldp + 4 * c4);
    const float4 b = *reinterpret_cast<const float4*>(bias + 4 * c4);
    float4 q = {0.f, 0.f, 0.f, 0.f};
    if (Q) q = *reinterpret_cast<const float4*>(Q + (size_t)(row0 + r) * ldq + 4 * c4);
    float* z = Z + ((size_t)K * row0 + r) * ldz + 4 * c4;
    const size_t step = (size_t)n * ldz;
    for (int k = 0; k < K; ++k) {
        const float a = alphas[k];                                // (uniform: a scalar load)
        const float a1 = 1.f - a;
        float4 v;
        v.x = fmaf(a, p.x, fmaf(a1, q.x, b.x));
        v.y = fmaf(a, p.y, fmaf(a1, q.y, b.y));
        v.z = fmaf(a, p.z, fmaf(a1, q.z, b.z));
        v.w = fmaf(a, p.w, fmaf(a1, q.w, b.w));
        *reinterpret_cast<float4*>(z + k * step) = v;
    }
}

// Sbar[g, r] = sum_k w_k Sv[(g, k), r], k = 0 .. K - 1 in order; blockIdx.z = 1 does the same for (Rv, Rbar)
__global__ void __launch_bounds__(256) gnm_intgrad_reduce_kernel(const float* __restrict__ Sv,
                                                                 const float* __restrict__ Rv,
                                                                 const int32_t* __restrict__ node_off,
                                                                 const float* __restrict__ weights, int K, int H4,
                                                                 float* __restrict__ Sbar, float* __restrict__ Rbar) {
    int row0, n, r, c4;
    if (!ig_element(node_off, H4, row0, n, r, c4)) return;
    const int ld = 4 * H4;
    const float* src = (blockIdx.z ? Rv : Sv) + ((size_t)K * row0 + r) * ld + 4 * c4;
    float* dst = (blockIdx.z ? Rbar : Sbar) + (size_t)(row0 + r) * ld + 4 * c4;
    const size_t step = (size_t)n * ld;
    float4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int k = 0; k < K; ++k) {
        const float w = weights[k];
        const float4 v = *reinterpret_cast<const float4*>(src + k * step);
        acc.x = fmaf(w, v.x, acc.x);
        acc.y = fmaf(w, v.y, acc.y);
        acc.z = fmaf(w, v.z, acc.z);
        acc.w = fmaf(w, v.w, acc.w);
    }
    *reinterpret_cast<float4*>(dst) = acc;
}

// attr[row, c] *= X[row, c] - base[r, c] (base: one [n_base, F0] block every graph shares, or null: zeros)
__global__ void __launch_bounds__(256) gnm_intgrad_scale_kernel(float* __restrict__ attr, int lda,
                                                                const float* __restrict__ X, int ldx,
                                                                const float* __restrict__ base, int ldb,
                                                                const int32_t* __restrict__ node_off, int F0) {
    int row0, n, r, c;
    if (!ig_element(node_off, F0, row0, n, r, c)) return;
    float d = X[(size_t)(row0 + r) * ldx + c];
    if (base) d -= base[(size_t)r * ldb + c];
    attr[(size_t)(row0 + r) * lda + c] *= d;
}

// Floats of scratch gnm_integrated_gradients needs for N source rows, K steps: gnm_saliency's two (S, R) pairs over the
// K N virtual rows and the reduced (Sbar, Rbar) pair.
extern "C" long long gnm_integrated_gradients_scratch_floats(long long N, int H, int K) {
    return (4LL * K + 2) * N * (long long)H;
}

static inline bool ig_misaligned(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) != 0; }

extern "C" int gnm_intgrad_z0(const float* P, int ldp, const float* Q, int ldq, const float* bias,
                              const int32_t* node_off, int B, int n_max, const float* alphas, int K, int H, float* Z,
                              int ldz, void* stream) {
    if (B <= 0) return GNM_OK;
    if (!(H == 32 || H == 64 || H == 128) || n_max < 1 || n_max > 416) return GNM_ERR_UNSUPPORTED;
    if (K < 1 || ldp < H || ldz < H || (Q && ldq < H)) return GNM_ERR_BAD_ARG;
    if (!P || !bias || !node_off || !alphas || !Z) return GNM_ERR_BAD_ARG;
    if (ig_misaligned(P) || ig_misaligned(Q) || ig_misaligned(bias) || ig_misaligned(Z) || (ldp & 3) || (ldz & 3) ||
        (Q && (ldq & 3)))
        return GNM_ERR_UNSUPPORTED;
    const int H4 = H / 4;
    hipLaunchKernelGGL(gnm_intgrad_z0_kernel, dim3((n_max * H4 + 255) / 256, B), dim3(256), 0,
                       reinterpret_cast<hipStream_t>(stream), P, ldp, Q, ldq, bias, node_off, alphas, K, H4, Z, ldz);
    GNM_CHECK_LAUNCH();
    return GNM_OK;
}

// gnm_integrated_gradients' launches around the layer launches (csrc/saliency.hip validates their arguments)
extern "C" int gnm_intgrad_reduce(const float* Sv, const float* Rv, const int32_t* node_off, int B, int n_max,
                                  const float* weights, int K, int H, float* Sbar, float* Rbar, hipStream_t s) {
    const int H4 = H / 4;
    hipLaunchKernelGGL(gnm_intgrad_reduce_kernel, dim3((n_max * H4 + 255) / 256, B, Rv ? 2 : 1), dim3(256), 0, s, Sv, Rv,
                       node_off, weights, K, H4, Sbar, Rbar);
    GNM_CHECK_LAUNCH();
    return GNM_OK;
}

extern "C" int gnm_intgrad_scale(float* attr, int lda, const float* X, int ldx, const float* base, int ldb,
                                 const int32_t* node_off, int B, int n_max, int F0, hipStream_t s) {
    hipLaunchKernelGGL(gnm_intgrad_scale_kernel, dim3((n_max * F0 + 255) / 256, B), dim3(256), 0, s, attr, lda, X, ldx,
                       base, ldb, node_off, F0);
    GNM_CHECK_LAUNCH();
    return GNM_OK;
}
