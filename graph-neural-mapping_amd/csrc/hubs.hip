// Hub measures of the arena's graphs, on the device: betweenness centrality (Brandes' algorithm with every order fixed)
// and, against a labelling of the nodes into modules, module degrees, participation coefficient, within-module degree
// z-score, the module edge matrix and Newman's modularity.  One workgroup owns one graph and stages its bit rows in LDS
// exactly as topology.hip does (gnm_topology.h), so both kernels see a simple undirected graph and a graph's results do
// not depend on what shares the launch.
//
// Betweenness.  Thread v owns node v for the whole kernel (the launch has at least n_max threads a workgroup): its
// level, sigma, delta and running total live in registers; sigma and delta are mirrored in LDS for the neighbours to
// read.  The workgroup walks the sources s = 0, 1, .. in order.  Forward, level k: a node not yet reached ANDs its row
// with the bit mask of level k - 1 word by word and adds sigma of the set bits in ascending order (a pull step: sigma is
// a sum over predecessors); the mask of level k is then formed from __ballot(level == k), two words a wave, into the
// other of two mask buffers.  Backward, level k from the deepest - 1 down to 1: a node at level k walks row & mask of
// level k + 1 in ascending order and adds (sigma[v] / sigma[w]) * (1.0 + delta[w]).  One barrier a level in each
// direction.  Whether a level is empty is read, after the barrier, from an LDS flag that the waves set before it, so
// every thread of the workgroup runs the same trip counts.  total[v] receives delta_s[v] in ascending s by construction.
//
// Modules.  K label masks of W words are built in LDS from the labels; k_v,m = sum over words of
// popcount(row_v & mask_m), a thread per node.  The sums several nodes add to (S1, S2, D_m, module sizes, edge counts
// between modules, the degree total) go through integer LDS atomics; after a barrier each fp64 value is formed once, by
// one lane, from finished integers, in ascending m.  No float atomic, no float reduction across lanes, contraction off.
#include "gnm_topology.h"

namespace {

constexpr int kHubMaxModules = 64;
constexpr int kHubMaskWords = kTopoMaxN / 32;       // one level mask; two of them are kept
constexpr int kModThreads = 256;

// the mask of the nodes with p true, this wave's two words of it; returns whether any lane of the wave had p
__device__ __forceinline__ bool hub_write_mask(uint32_t* mask, bool p) {
    const unsigned long long b = __ballot(p);
    if ((threadIdx.x & 63) == 0) {
        const int w = threadIdx.x >> 6;
        mask[2 * w] = (uint32_t)b;
        mask[2 * w + 1] = (uint32_t)(b >> 32);
    }
    return b != 0ull;
}

// LDS: [n_max doubles: sigma][n_max doubles: delta][2 x 32 words: level masks][4 ints: level flags][rows].
template <int T>
__global__ void __launch_bounds__(T) gnm_topology_betweenness_kernel(
    const int32_t* __restrict__ rowptr, const uint16_t* __restrict__ col, const int64_t* __restrict__ b_rp_off,
    const int64_t* __restrict__ b_col_off, const int32_t* __restrict__ node_off, int n_max,
    double* __restrict__ betweenness, double* __restrict__ betweenness_normalized) {
#pragma clang fp contract(off)
    extern __shared__ double hub_lds[];
    const int b = blockIdx.x, v = threadIdx.x;
    const TopoGraph g = topo_graph(rowptr, col, b_rp_off, b_col_off, node_off, b);
    const int n = g.n;
    if (n < 0 || n > n_max || n_max > T) return;        // not this launch's to hold: nothing is written
    double* s_sig = hub_lds;
    double* s_del = s_sig + n_max;
    uint32_t* s_mask = reinterpret_cast<uint32_t*>(s_del + n_max);
    int* s_flag = reinterpret_cast<int*>(s_mask + 2 * kHubMaskWords);
    uint32_t* rows = reinterpret_cast<uint32_t*>(s_flag + 4);
    const int W = topo_words(n), stride = topo_stride(n);
    topo_stage(rows, n, stride, g.rp, g.col);

    const bool live = v < n;
    const uint32_t* row = rows + (live ? v : 0) * stride;
    const bool lane0 = (v & 63) == 0;
    double total = 0.0;
    for (int s = 0; s < n; ++s) {
        int lvl = live ? (v == s ? 0 : -1) : -2;        // -1: not reached yet; -2: no node
        double sig = v == s ? 1.0 : 0.0, del = 0.0;
        if (live) {
            s_sig[v] = sig;
            s_del[v] = 0.0;
        }
        hub_write_mask(s_mask, lvl == 0);
        if (v == 0) s_flag[0] = s_flag[1] = s_flag[2] = 0;
        __syncthreads();
        int k = 1;
        for (;; ++k) {                                  // level k from the mask of level k - 1
            const uint32_t* prev = s_mask + ((k - 1) & 1) * kHubMaskWords;
            if (lvl == -1) {
                double acc = 0.0;
                bool any = false;
                for (int j = 0; j < W; ++j) {
                    uint32_t m = row[j] & prev[j];
                    while (m) {
                        const int u = (j << 5) + __builtin_ctz(m);
                        m &= m - 1;
                        acc = acc + s_sig[u];
                        any = true;
                    }
                }
                if (any) {
                    lvl = k;
                    sig = acc;
                    s_sig[v] = acc;                     // read from level k + 1 on: nobody reads it before the barrier
                }
            }
            const bool some = hub_write_mask(s_mask + (k & 1) * kHubMaskWords, lvl == k);
            if (lane0 && some) s_flag[k % 3] = 1;
            if (v == 0) s_flag[(k + 1) % 3] = 0;        // last read after the barrier of level k - 2
            __syncthreads();
            if (!s_flag[k % 3]) break;                  // the whole workgroup reads the same word
        }
        // levels 0 .. k - 1 hold nodes; the mask of level k - 1 is in buffer (k - 1) & 1, the other one is empty
        for (int kk = k - 2; kk >= 1; --kk) {
            const uint32_t* next = s_mask + ((kk + 1) & 1) * kHubMaskWords;
            if (lvl == kk) {
                double acc = 0.0;
                for (int j = 0; j < W; ++j) {
                    uint32_t m = row[j] & next[j];
                    while (m) {
                        const int w = (j << 5) + __builtin_ctz(m);
                        m &= m - 1;
                        const double t = (sig / s_sig[w]) * (1.0 + s_del[w]);
                        acc = acc + t;
                    }
                }
                del = acc;
                s_del[v] = acc;
            }
            hub_write_mask(s_mask + (kk & 1) * kHubMaskWords, lvl == kk);
            __syncthreads();
        }
        if (live && v != s) total = total + del;
    }
    if (live) {
        const double bc = total * 0.5;
        betweenness[g.row0 + v] = bc;
        betweenness_normalized[g.row0 + v] = n < 3 ? 0.0 : bc / (double)((long long)(n - 1) * (n - 2) / 2);
    }
}

struct HubModuleOut {
    int32_t* module_degree;
    double *participation, *within_module_z;
    long long* module_edges;
    double* modularity;
};

// LDS: [K x K ints: ordered pairs between modules][K ints each: S1, S2, D_m, module sizes][8 ints: 0 the degree total]
// [K masks at the row stride of n_max][rows].  The int32 sums hold at n <= 1024: the largest is S2 <= n (n - 1)^2 < 2^31.
__global__ void __launch_bounds__(kModThreads) gnm_topology_modules_kernel(
    const int32_t* __restrict__ rowptr, const uint16_t* __restrict__ col, const int64_t* __restrict__ b_rp_off,
    const int64_t* __restrict__ b_col_off, const int32_t* __restrict__ node_off, const int32_t* __restrict__ label,
    int n_max, int K, HubModuleOut o) {
#pragma clang fp contract(off)
    extern __shared__ double hub_lds[];
    const int b = blockIdx.x, tid = threadIdx.x;
    const TopoGraph g = topo_graph(rowptr, col, b_rp_off, b_col_off, node_off, b);
    const int n = g.n;
    if (n < 0 || n > n_max) return;
    int* s_pair = reinterpret_cast<int*>(hub_lds);
    int* s_s1 = s_pair + K * K;
    int* s_s2 = s_s1 + K;
    int* s_dm = s_s2 + K;
    int* s_size = s_dm + K;
    int* s_tot = s_size + K;
    uint32_t* s_mask = reinterpret_cast<uint32_t*>(s_tot + 8);
    uint32_t* rows = s_mask + K * topo_stride(n_max);
    const int W = topo_words(n), stride = topo_stride(n);
    for (int i = tid; i < K * K + 4 * K + 8 + K * stride; i += kModThreads) s_pair[i] = 0;     // sums and masks
    topo_stage(rows, n, stride, g.rp, g.col);
    const int32_t* lab_g = label + g.row0;
    for (int v = tid; v < n; v += kModThreads) {
        const int lab = lab_g[v];
        if (lab >= 0 && lab < K) {
            atomicOr(&s_mask[lab * stride + (v >> 5)], 1u << (v & 31));
            atomicAdd(&s_size[lab], 1);
        }
    }
    __syncthreads();
    for (int v = tid; v < n; v += kModThreads) {
        const uint32_t* row = rows + v * stride;
        const int lab = lab_g[v];
        const bool member = lab >= 0 && lab < K;
        int deg = 0, d = 0, own = 0;
        for (int j = 0; j < W; ++j) deg += __popc(row[j]);
        int32_t* out = o.module_degree + (size_t)(g.row0 + v) * K;
        for (int m = 0; m < K; ++m) {
            const uint32_t* mask = s_mask + m * stride;
            int k = 0;
            for (int j = 0; j < W; ++j) k += __popc(row[j] & mask[j]);
            out[m] = k;
            d += k;
            if (member && k) atomicAdd(&s_pair[lab * K + m], k);
            if (m == lab) own = k;
        }
        if (member) {
            atomicAdd(&s_s1[lab], own);
            atomicAdd(&s_s2[lab], own * own);
            atomicAdd(&s_dm[lab], deg);
        }
        atomicAdd(&s_tot[0], deg);
        double acc = 0.0;
        if (d) {
            for (int m = 0; m < K; ++m) {
                const uint32_t* mask = s_mask + m * stride;
                int k = 0;
                for (int j = 0; j < W; ++j) k += __popc(row[j] & mask[j]);
                const double r = (double)k / (double)d;
                acc = acc + r * r;
            }
        }
        o.participation[g.row0 + v] = d ? 1.0 - acc : 0.0;
    }
    __syncthreads();
    for (int v = tid; v < n; v += kModThreads) {
        const int lab = lab_g[v];
        double z = 0.0;
        if (lab >= 0 && lab < K) {
            const uint32_t *row = rows + v * stride, *mask = s_mask + lab * stride;
            int k = 0;
            for (int j = 0; j < W; ++j) k += __popc(row[j] & mask[j]);
            const long long s = s_size[lab], s1 = s_s1[lab], s2 = s_s2[lab];
            const long long rad = s * s2 - s1 * s1;
            if (rad > 0) z = (double)((long long)k * s - s1) / __dsqrt_rn((double)rad);
        }
        o.within_module_z[g.row0 + v] = z;
    }
    long long* edges = o.module_edges + (size_t)b * K * K;
    for (int i = tid; i < K * K; i += kModThreads)      // a pair inside a module was counted from both ends
        edges[i] = (i / K == i % K) ? (long long)(s_pair[i] >> 1) : (long long)s_pair[i];
    if (tid == 0) {
        const long long E = s_tot[0] >> 1;
        double acc = 0.0;
        if (E) {
            for (int m = 0; m < K; ++m) {
                const double a = (double)s_dm[m] / (double)(2 * E);
                acc = acc + ((double)(long long)(s_pair[m * K + m] >> 1) / (double)E - a * a);
            }
        }
        o.modularity[b] = acc;
    }
}

size_t hub_betweenness_lds(int n_max) {
    return (size_t)n_max * 16 + (2 * (size_t)kHubMaskWords + 4) * 4 + (size_t)n_max * topo_stride(n_max) * 4;
}
size_t hub_modules_lds(int n_max, int K) {
    return ((size_t)K * K + 4 * (size_t)K + 8) * 4 + ((size_t)K + n_max) * topo_stride(n_max) * 4;
}
constexpr size_t kHubRowWords = kTopoMaxN / 32 + 1;
static_assert((size_t)kTopoMaxN * 16 + (2 * (size_t)kHubMaskWords + 4) * 4 + (size_t)kTopoMaxN * kHubRowWords * 4
                  <= (size_t)kLdsBudget, "sigma, delta, the level masks and the largest graph's rows must fit one CU's LDS");
static_assert(((size_t)kHubMaxModules * kHubMaxModules + 4 * (size_t)kHubMaxModules + 8) * 4
                  + ((size_t)kHubMaxModules + kTopoMaxN) * kHubRowWords * 4 <= (size_t)kLdsBudget,
              "the module sums, the label masks and the largest graph's rows must fit one CU's LDS");

}  // namespace

extern "C" int gnm_topology_max_modules(void) { return kHubMaxModules; }

// All scratch of the betweenness kernel is in the owning workgroup's LDS.
extern "C" long long gnm_topology_betweenness_workspace_bytes(int B, int n_max) {
    return topo_check(B, n_max) == GNM_OK ? 0 : -1;
}

extern "C" int gnm_topology_betweenness(const int32_t* rowptr, const uint16_t* col, const int64_t* b_rp_off,
                                        const int64_t* b_col_off, const int32_t* node_off, int B, int n_max,
                                        void* workspace, double* betweenness, double* betweenness_normalized,
                                        void* stream) {
    (void)workspace;
    if (int e = topo_check(B, n_max)) return e;
    if (B == 0) return GNM_OK;
    if (!rowptr || !col || !b_rp_off || !b_col_off || !node_off || !betweenness || !betweenness_normalized)
        return GNM_ERR_BAD_ARG;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const size_t lds = hub_betweenness_lds(n_max);
    if (n_max <= 512) {
        GNM_ALLOW_FULL_LDS(gnm_topology_betweenness_kernel<512>);
        hipLaunchKernelGGL(gnm_topology_betweenness_kernel<512>, dim3((unsigned)B), dim3(512), lds, s, rowptr, col,
                           b_rp_off, b_col_off, node_off, n_max, betweenness, betweenness_normalized);
    } else {
        GNM_ALLOW_FULL_LDS(gnm_topology_betweenness_kernel<1024>);
        hipLaunchKernelGGL(gnm_topology_betweenness_kernel<1024>, dim3((unsigned)B), dim3(1024), lds, s, rowptr, col,
                           b_rp_off, b_col_off, node_off, n_max, betweenness, betweenness_normalized);
    }
    GNM_CHECK_LAUNCH();
    return GNM_OK;
}

extern "C" int gnm_topology_modules(const int32_t* rowptr, const uint16_t* col, const int64_t* b_rp_off,
                                    const int64_t* b_col_off, const int32_t* node_off, const int32_t* label, int B,
                                    int n_max, int K, int32_t* module_degree, double* participation,
                                    double* within_module_z, long long* module_edges, double* modularity,
                                    void* stream) {
    if (int e = topo_check(B, n_max)) return e;
    if (K < 1) return GNM_ERR_BAD_ARG;
    if (K > kHubMaxModules) return GNM_ERR_UNSUPPORTED;
    if (B == 0) return GNM_OK;
    if (!rowptr || !col || !b_rp_off || !b_col_off || !node_off || !label || !module_degree || !participation ||
        !within_module_z || !module_edges || !modularity)
        return GNM_ERR_BAD_ARG;
    HubModuleOut o{module_degree, participation, within_module_z, module_edges, modularity};
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    GNM_ALLOW_FULL_LDS(gnm_topology_modules_kernel);
    hipLaunchKernelGGL(gnm_topology_modules_kernel, dim3((unsigned)B), dim3(kModThreads), hub_modules_lds(n_max, K), s,
                       rowptr, col, b_rp_off, b_col_off, node_off, label, n_max, K, o);
    GNM_CHECK_LAUNCH();
    return GNM_OK;
}
