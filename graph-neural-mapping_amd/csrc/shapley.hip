// Shapley values of ROI networks (GIN_InfoMaxReg.shapley()): the players are the K groups of a node labelling, the
// value of a coalition S is the class score of the graph with every labelled node of a group outside S lesioned
// (csrc/lesion.hip's virtual graphs, unchanged).  Two things live here:
//   * gnm_coalition_pack: the keep masks and kept counts of V virtual graphs in gnm_lesion_pack's layout, bitwise what
//     gnm_lesion_pack writes for the equivalent "removed" array, from 4 bytes per virtual graph -- a coalition id --
//     and the batch's label rows.  BITSET form: node r is kept iff its label is negative (background) or bit `label`
//     of the id is set.  PREFIX form: id = m (K + 1) + j names the first j players of permutation m; node r is kept
//     iff its label is negative or rank[m][label] < j.
//   * gnm_shapley_exact / gnm_shapley_permutation: the fp32 coalition scores combined into fp64 Shapley values,
//     pairwise interaction indices, and the mean and standard error over sampled permutations.  Differences are formed
//     first, every sum has a fixed order and no atomics are used: bitwise reproducible.  fp contraction is off in
//     these kernels: the fp64 numpy restatement (gnm/shapley.py) rounds the product before it adds.
#include "gnm_rowblock.h"

static constexpr int kShMaxBits = 32;             // BITSET form: a coalition id is one 32-bit word
static constexpr int kShMaxExact = 16;            // gnm_shapley_exact: 2^16 scores per (class, graph)

// 16 lanes per virtual graph, one mask word per lane (2 x 8 words at most), plain vector stores; the lane of word 0
// adds the group's 16 popcounts in order -- gnm_lesion_pack_kernel with the removed byte replaced by the rule above.
// A label >= K (the host rejects it) is treated as background: nothing is read outside ranks [M][K].
template <bool PREFIX>
__global__ void __launch_bounds__(256) gnm_coalition_pack_kernel(const int16_t* labels, long long ldl,
                                                                 const int32_t* vgraph, const int32_t* ids,
                                                                 const int16_t* ranks, int M, int K,
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
            const int16_t* lab = labels + (size_t)b * ldl;
            const unsigned id = (unsigned)ids[q];
            const int pm = PREFIX ? (int)(id / (unsigned)(K + 1)) : 0;            // the permutation and
            const int pj = PREFIX ? (int)(id - (unsigned)pm * (unsigned)(K + 1)) : 0;   // how many of its players are present
            const int16_t* rk = PREFIX ? ranks + (size_t)min(pm, M - 1) * K : nullptr;
            for (int mbyte = 0; mbyte < 4; ++mbyte) {
                const int c0 = 16 * (4 * j + mbyte) + 8 * hh;     // byte mbyte of word j of half hh: step 4 j + mbyte
                for (int k = 0; k < 8; ++k) {
                    if (c0 + k >= n) continue;
                    const int l = lab[c0 + k];
                    bool keep = l < 0 || l >= K;
                    if (!keep) keep = PREFIX ? (pm < M && rk[l] < pj) : ((id >> l) & 1u) != 0u;
                    if (keep) word |= 1u << (8 * mbyte + k);
                }
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

// masks [V][mstride] and kept [V] of the virtual graphs from their coalition ids (see include/gnm_hip.h)
extern "C" int gnm_coalition_pack(const int16_t* labels, long long ldl, const int32_t* vgraph, const int32_t* ids,
                                  const int16_t* ranks, int M, int K, const int32_t* node_off, int B, int n_max,
                                  long long V, int mstride, uint32_t* masks, int32_t* kept, void* stream) {
    if (B == 0 || V == 0) return GNM_OK;
    if (n_max < 1 || n_max > kRbMaxN) return GNM_ERR_UNSUPPORTED;
    const int need = 2 * rb_half_words((n_max + 31) / 32);        // gnm_lesion_mask_words(n_max)
    if (B < 0 || V < 0 || ldl < n_max || mstride < need || mstride > 16) return GNM_ERR_BAD_ARG;
    if (!labels || !vgraph || !ids || !node_off || !masks || !kept) return GNM_ERR_BAD_ARG;
    if (ranks ? (K < 1 || K > kRbMaxN || M < 1) : (K < 1 || K > kShMaxBits)) return GNM_ERR_BAD_ARG;
    if (ranks && (long long)M * (K + 1) >= (1LL << 31)) return GNM_ERR_BAD_ARG;
    if ((V + 15) / 16 >= (1LL << 31)) return GNM_ERR_UNSUPPORTED;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)((V + 15) / 16));
    if (ranks)
        hipLaunchKernelGGL(gnm_coalition_pack_kernel<true>, grid, dim3(256), 0, s, labels, ldl, vgraph, ids, ranks, M, K,
                           node_off, (int)V, mstride, masks, kept);
    else
        hipLaunchKernelGGL(gnm_coalition_pack_kernel<false>, grid, dim3(256), 0, s, labels, ldl, vgraph, ids, ranks, 0, K,
                           node_off, (int)V, mstride, masks, kept);
    GNM_CHECK_LAUNCH();
    return GNM_OK;
}

// ---- the reductions ------------------------------------------------------------------------------------------------
struct ShWeights { double w[kShMaxExact]; };      // by value: w_K(s) or u_K(s) at s = 0 .. K - 1 (K - 2)

// the fixed-order tree over the workgroup's 256 partial sums: sh[t] += sh[t + 128], then + 64, ... + 1
__device__ __forceinline__ double sh_block_sum(double* sh, int t, double acc) {
    sh[t] = acc;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (t < s) sh[t] += sh[t + s];
        __syncthreads();
    }
    return sh[0];
}

// c with a zero bit inserted at position i: the compact index of a subset of the players other than i -> its id
__device__ __forceinline__ unsigned sh_insert_zero(unsigned c, int i) {
    const unsigned low = c & ((1u << i) - 1u);
    return ((c >> i) << (i + 1)) | low;
}

// phi[c, g, i]: one workgroup per (class, graph, player); thread t takes the compact subsets t, t + 256, ... ascending.
// With `inter` given the workgroup also writes the zero diagonal entry inter[c, g, i, i].
__global__ void __launch_bounds__(256) gnm_shapley_phi_kernel(const float* scores, long long lds, int G, int K,
                                                              const ShWeights wt, double* phi, double* inter) {
#pragma clang fp contract(off)
    __shared__ double sh[256];
    const int t = threadIdx.x;
    const int i = blockIdx.x % K;
    const long long cg = blockIdx.x / K;
    const long long c = cg / G, g = cg - c * G;
    const float* v = scores + c * lds + (g << K);
    const unsigned half = 1u << (K - 1);
    double acc = 0.0;
    for (unsigned s = t; s < half; s += 256) {
        const unsigned id0 = sh_insert_zero(s, i);
        const double d = (double)v[id0 | (1u << i)] - (double)v[id0];
        const double term = wt.w[__popc(s)] * d;
        acc = acc + term;
    }
    const double sum = sh_block_sum(sh, t, acc);
    if (t == 0) {
        phi[cg * K + i] = sum;
        if (inter) inter[(cg * K + i) * K + i] = 0.0;
    }
}

// inter[c, g, i, j] = inter[c, g, j, i]: one workgroup per (class, graph, pair i < j), the pairs in the order (0, 1),
// (0, 2), ..., (0, K - 1), (1, 2), ...; the difference of differences (v(S+ij) - v(S+i)) - (v(S+j) - v(S)), so that a
// player whose presence changes no score contributes an exact zero
__global__ void __launch_bounds__(256) gnm_shapley_inter_kernel(const float* scores, long long lds, int G, int K,
                                                                const ShWeights wt, double* inter) {
#pragma clang fp contract(off)
    __shared__ double sh[256];
    const int t = threadIdx.x;
    const int P = K * (K - 1) / 2;
    int pr = blockIdx.x % P;
    const long long cg = blockIdx.x / P;
    const long long c = cg / G, g = cg - c * G;
    int i = 0;
    while (pr >= K - 1 - i) { pr -= K - 1 - i; ++i; }             // (workgroup-uniform; at most K - 1 steps)
    const int j = i + 1 + pr;
    const float* v = scores + c * lds + (g << K);
    const unsigned quarter = 1u << (K - 2);
    const unsigned bi = 1u << i, bj = 1u << j;
    double acc = 0.0;
    for (unsigned s = t; s < quarter; s += 256) {
        const unsigned id0 = sh_insert_zero(sh_insert_zero(s, i), j);             // i < j: the lower bit first
        const double with_i = (double)v[id0 | bi | bj] - (double)v[id0 | bi];
        const double without = (double)v[id0 | bj] - (double)v[id0];
        const double term = wt.w[__popc(s)] * (with_i - without);
        acc = acc + term;
    }
    const double sum = sh_block_sum(sh, t, acc);
    if (t == 0) {
        inter[(cg * K + i) * K + j] = sum;
        inter[(cg * K + j) * K + i] = sum;
    }
}

// scores [n_classes][lds] fp32, entry g 2^K + id the score of coalition id of graph g -> phi [n_classes][G][K] and,
// with inter != NULL, inter [n_classes][G][K][K] (see include/gnm_hip.h)
extern "C" int gnm_shapley_exact(const float* scores, long long lds, int n_classes, long long G, int K,
                                 const double* w_host, const double* u_host, double* phi, double* inter, void* stream) {
    if (n_classes == 0 || G == 0) return GNM_OK;
    if (K < 1 || K > kShMaxExact) return GNM_ERR_UNSUPPORTED;
    if (n_classes < 0 || G < 0 || lds < (G << K) || !scores || !w_host || !phi) return GNM_ERR_BAD_ARG;
    if (inter && K > 1 && !u_host) return GNM_ERR_BAD_ARG;
    const long long pairs = (long long)K * (K - 1) / 2;
    if (n_classes * G * K >= (1LL << 31) || n_classes * G * pairs >= (1LL << 31)) return GNM_ERR_UNSUPPORTED;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    ShWeights wt;
    for (int k = 0; k < kShMaxExact; ++k) wt.w[k] = k < K ? w_host[k] : 0.0;
    hipLaunchKernelGGL(gnm_shapley_phi_kernel, dim3((unsigned)(n_classes * G * K)), dim3(256), 0, s, scores, lds, (int)G,
                       K, wt, phi, inter);
    GNM_CHECK_LAUNCH();
    if (inter && K > 1) {
        for (int k = 0; k < kShMaxExact; ++k) wt.w[k] = k < K - 1 ? u_host[k] : 0.0;
        hipLaunchKernelGGL(gnm_shapley_inter_kernel, dim3((unsigned)(n_classes * G * pairs)), dim3(256), 0, s, scores,
                           lds, (int)G, K, wt, inter);
        GNM_CHECK_LAUNCH();
    }
    return GNM_OK;
}

// mean[c, g, i] and err[c, g, i] over the M permutations: one thread per (class, graph, player), sequential over m.
// Player i sits at rank r = ranks[m][i] of permutation m and contributes v[m][r + 1] - v[m][r].  Two passes: the mean,
// then the squared deviations from it; err = sqrt(sum / (M - 1)) / sqrt(M), NaN at M = 1.
__global__ void __launch_bounds__(256) gnm_shapley_permutation_kernel(const float* scores, long long lds, long long total,
                                                                      int G, int M, int K, const int16_t* ranks,
                                                                      double* mean, double* err) {
#pragma clang fp contract(off)
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    const int i = (int)(e % K);
    const long long cg = e / K;
    const long long c = cg / G, g = cg - c * G;
    const float* v = scores + c * lds + g * (long long)M * (K + 1);
    double sum = 0.0;
    for (int m = 0; m < M; ++m) {
        const int r = min(max((int)ranks[(size_t)m * K + i], 0), K - 1);
        const float* vm = v + (size_t)m * (K + 1);
        sum = sum + ((double)vm[r + 1] - (double)vm[r]);
    }
    const double mu = sum / (double)M;
    double ss = 0.0;
    for (int m = 0; m < M; ++m) {
        const int r = min(max((int)ranks[(size_t)m * K + i], 0), K - 1);
        const float* vm = v + (size_t)m * (K + 1);
        const double d = ((double)vm[r + 1] - (double)vm[r]) - mu;
        const double d2 = d * d;
        ss = ss + d2;
    }
    mean[e] = mu;
    err[e] = M > 1 ? sqrt(ss / (double)(M - 1)) / sqrt((double)M) : __builtin_nan("");
}

// scores [n_classes][lds] fp32, entry (g M + m) (K + 1) + j the score of the first j players of permutation m present
// in graph g; ranks [M][K] int16 on the DEVICE, a permutation of 0 .. K - 1 per row (the HOST validates it: an entry
// indexes the scores) -> mean and err [n_classes][G][K] (see include/gnm_hip.h)
extern "C" int gnm_shapley_permutation(const float* scores, long long lds, int n_classes, long long G, int M, int K,
                                       const int16_t* ranks, double* mean, double* err, void* stream) {
    if (n_classes == 0 || G == 0) return GNM_OK;
    if (K < 1 || K > kRbMaxN) return GNM_ERR_UNSUPPORTED;
    if (n_classes < 0 || G < 0 || M < 1 || lds < G * M * (long long)(K + 1)) return GNM_ERR_BAD_ARG;
    if (!scores || !ranks || !mean || !err) return GNM_ERR_BAD_ARG;
    const long long total = n_classes * G * K;
    if ((total + 255) / 256 >= (1LL << 31)) return GNM_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(gnm_shapley_permutation_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0,
                       reinterpret_cast<hipStream_t>(stream), scores, lds, total, (int)G, M, K, ranks, mean, err);
    GNM_CHECK_LAUNCH();
    return GNM_OK;
}
