// What the graph-measure units (topology.hip, hubs.hip) share: the node limit, the bit-row layout in LDS, the staging of
// a graph's rows from its CSR, and the launchers' argument check.  The layout is described at the top of topology.hip.
#pragma once
#include "gnm_common.h"

namespace {

constexpr int kTopoMaxN = 1024;         // 1024 rows of 33 words are 132 KiB; the largest scratch beside them is 25.3 KiB

__host__ __device__ inline int topo_words(int n) { return (n + 31) >> 5; }
__host__ __device__ inline int topo_stride(int n) { return topo_words(n) | 1; }

// Zero the rows, then set the bits of the graph's CSR: a wave per row, its lanes over the row's entries.
__device__ __forceinline__ void topo_stage(uint32_t* rows, int n, int stride, const int32_t* __restrict__ rp,
                                           const uint16_t* __restrict__ col) {
    const int tid = threadIdx.x, nthr = blockDim.x;
    for (int i = tid; i < n * stride; i += nthr) rows[i] = 0u;
    __syncthreads();
    const int lane = tid & 63, wave = tid >> 6, nwave = nthr >> 6;
    for (int r = wave; r < n; r += nwave) {
        const int beg = rp[r], end = rp[r + 1];
        for (int e = beg + lane; e < end; e += 64) {
            const int c = col[e];
            if (c != r && c < n) atomicOr(&rows[r * stride + (c >> 5)], 1u << (c & 31));
        }
    }
    __syncthreads();
}

struct TopoGraph {
    const int32_t* rp;
    const uint16_t* col;
    int n, row0;
};

__device__ __forceinline__ TopoGraph topo_graph(const int32_t* rowptr, const uint16_t* col, const int64_t* b_rp_off,
                                                const int64_t* b_col_off, const int32_t* node_off, int b) {
    TopoGraph g;
    g.rp = rowptr + b_rp_off[b];
    g.col = col + b_col_off[b];
    g.row0 = node_off[b];
    g.n = node_off[b + 1] - g.row0;
    return g;
}

inline int topo_check(int B, int n_max) {
    if (B < 0 || n_max < 1) return GNM_ERR_BAD_ARG;
    if (n_max > kTopoMaxN) return GNM_ERR_UNSUPPORTED;
    return GNM_OK;
}

}  // namespace
