// Graph-theoretic measures of the arena's graphs, on the device: degree, triangles, clustering, the shortest-path
// measures (eccentricity, reach, distance sums, components, nodal and global efficiency, the distance histogram,
// diameter, characteristic path length), transitivity and local efficiency.  One workgroup owns one graph, so a graph's
// results do not depend on what shares the launch.
//
// LDS image.  The graph is staged from its CSR as plain bit rows: row u is W = ceil(n / 32) words, bit (v & 31) of
// word (v >> 5) set for an edge {u, v}, at a stride of W | 1 words (odd: consecutive rows start on every bank in turn).
// Bits are set with LDS integer OR, so a repeated CSR entry collapses; an entry (u, u) and a column >= n are skipped.
// Every kernel below therefore sees a simple graph.  The de-interleaved bit matrix of csrc/aggm.hip is not read.
//
// Lane mapping.  A breadth-first search is held by a lane group of G lanes in "lane = word" form: lane j of the group
// holds word j of the visited set and of the frontier.  G = 16 while the launch's largest graph has W <= 16 (n <= 512),
// else 32, so a 64-lane wave runs four or two searches side by side.  One level: the group's non-empty frontier words
// are found with one 64-bit __ballot, each is broadcast with __shfl, and for each of its set bits u every lane ORs its
// word of row u into `next`; next &= allowed & ~visited; c_k = the group's popcount, added with __shfl_xor.  All control
// flow inside a search depends on values the whole group shares, so a group's lanes never diverge from each other.
//
// Exactness.  Everything up to the last step is integer work.  Counts that several groups add to (the distance
// histogram, a node's local-efficiency histogram, the per-graph totals) go through integer LDS atomics, which are exact
// in any order.  Each floating-point output is then formed once, by one lane, from finished integers, in a fixed order:
//     eff(H, m) = acc = 0.0; for k = 1, 2, ..: if H[k]: acc = acc + (double)H[k] / (double)k;  acc / (double)m
// and the two means are sequential sums over the nodes in ascending order followed by one division.  There is no float
// atomic and no float reduction across lanes; contraction is off.
#include "gnm_topology.h"

namespace {

constexpr int kTopoSmallW = 16;         // words a 16-lane group holds: above it the launch runs 32-lane groups

constexpr int topo_threads(int G) { return G == 16 ? 256 : 1024; }      // 16 or 32 groups per workgroup

template <int G>
__device__ __forceinline__ int group_sum(int v) {
#pragma unroll
    for (int off = G / 2; off > 0; off >>= 1) v += __shfl_xor(v, off, G);
    return v;
}
template <int G>
__device__ __forceinline__ int group_min(int v) {
#pragma unroll
    for (int off = G / 2; off > 0; off >>= 1) v = min(v, __shfl_xor(v, off, G));
    return v;
}

// the non-empty words of a group's distributed bit set, as a mask over the group's lanes
template <int G>
__device__ __forceinline__ uint32_t group_nonzero(uint32_t w, int gshift) {
    const unsigned long long b = __ballot(w != 0u);
    return (uint32_t)(b >> gshift) & (G == 32 ? 0xffffffffu : 0xffffu);
}

// One search of a lane group from node src inside the node set `allowed` (this lane's word of it; 0 on a lane past the
// last word), over the rows in LDS.  jj: the word this lane reads (0 on a lane past the last word, whose `allowed`
// discards it).  level(k, c) is called by every lane of the group for each distance k >= 1 with c > 0 nodes at it.
// kTri: also count, into tri, the bits that the rows of the nodes at distance 1 share with tri_row (twice the
// triangles through src once the group's lanes are added).  Returns this lane's word of the visited set.
template <int G, bool kTri, class Level>
__device__ __forceinline__ uint32_t topo_bfs(const uint32_t* rows, int stride, int jj, int gl, int gshift, int src,
                                             uint32_t allowed, uint32_t tri_row, int& tri, Level&& level) {
    uint32_t vis = (gl == (src >> 5)) ? 1u << (src & 31) : 0u;
    uint32_t front = vis;
    for (int k = 1;; ++k) {
        uint32_t m = group_nonzero<G>(front, gshift);
        uint32_t next = 0u;
        while (m) {
            const int q = __builtin_ctz(m);
            m &= m - 1;
            uint32_t w = __shfl(front, q, G);
            while (w) {
                const int u = (q << 5) + __builtin_ctz(w);
                w &= w - 1;
                const uint32_t r = rows[u * stride + jj];
                next |= r;
                if (kTri && k == 2) tri += __popc(r & tri_row);
            }
        }
        next &= allowed & ~vis;
        const int c = group_sum<G>(__popc(next));
        if (c == 0) break;
        vis |= next;
        front = next;
        level(k, c);
    }
    return vis;
}

__device__ __forceinline__ double topo_nan() { return __longlong_as_double(0x7ff8000000000000LL); }

struct TopoNodeOut {
    int32_t *degree, *triangles, *eccentricity, *reachable, *distance_sum, *component;
    double *clustering, *nodal_efficiency;
    long long *edges, *distance_histogram;
    int32_t *components, *diameter;
    double *global_efficiency, *characteristic_path_length, *transitivity, *mean_clustering;
};

// ---------------------------------------------------------------------------------------------- node and graph measures
// Group g searches from the nodes g, g + NG, ..  LDS: [n_max doubles: clustering][n_max ints: histogram][8 ints: totals]
// [rows].  Totals: 0 sum of degrees, 1 sum of triangles per node, 2 connected triples, 3 components, 4 diameter.
template <int G>
__global__ void __launch_bounds__(topo_threads(G)) gnm_topology_nodes_kernel(
    const int32_t* __restrict__ rowptr, const uint16_t* __restrict__ col, const int64_t* __restrict__ b_rp_off,
    const int64_t* __restrict__ b_col_off, const int32_t* __restrict__ node_off, int n_max, TopoNodeOut o) {
#pragma clang fp contract(off)
    extern __shared__ double topo_lds[];
    const int b = blockIdx.x, tid = threadIdx.x;
    const TopoGraph g = topo_graph(rowptr, col, b_rp_off, b_col_off, node_off, b);
    const int n = g.n;
    if (n < 0 || n > n_max) return;                     // not this launch's to hold: nothing is written
    double* s_clu = topo_lds;
    int* s_hist = reinterpret_cast<int*>(s_clu + n_max);
    int* s_tot = s_hist + n_max;
    uint32_t* rows = reinterpret_cast<uint32_t*>(s_tot + 8);
    const int W = topo_words(n), stride = topo_stride(n);
    for (int i = tid; i < n_max + 8; i += blockDim.x) s_hist[i] = 0;          // histogram and totals
    topo_stage(rows, n, stride, g.rp, g.col);

    constexpr int NG = topo_threads(G) / G;
    const int grp = tid / G, gl = tid & (G - 1), gshift = (tid & 63) & ~(G - 1);
    const int jj = gl < W ? gl : 0;
    const uint32_t live = gl < W ? 0xffffffffu : 0u;
    for (int v = grp; v < n; v += NG) {
        const uint32_t row_v = rows[v * stride + jj] & live;
        int tri = 0, ecc = 0, reach = 0, dsum = 0, deg = 0;
        double acc = 0.0;
        const uint32_t vis = topo_bfs<G, true>(rows, stride, jj, gl, gshift, v, live, row_v, tri, [&](int k, int c) {
            if (k == 1) deg = c;
            ecc = k;
            reach += c;
            dsum += k * c;
            acc = acc + (double)c / (double)k;
            if (gl == 0) atomicAdd(&s_hist[k], c);
        });
        const int t = group_sum<G>(tri) >> 1;
        const int comp = group_min<G>(vis ? (gl << 5) + __builtin_ctz(vis) : 0x7fffffff);
        if (gl == 0) {
            const double clu = deg < 2 ? 0.0 : (2.0 * (double)t) / (double)(deg * (deg - 1));
            const int row = g.row0 + v;
            o.degree[row] = deg;
            o.triangles[row] = t;
            o.clustering[row] = clu;
            o.eccentricity[row] = ecc;
            o.reachable[row] = reach;
            o.distance_sum[row] = dsum;
            o.component[row] = comp;
            o.nodal_efficiency[row] = n < 2 ? 0.0 : acc / (double)(n - 1);
            s_clu[v] = clu;
            atomicAdd(&s_tot[0], deg);
            atomicAdd(&s_tot[1], t);
            atomicAdd(&s_tot[2], deg * (deg - 1) / 2);
            if (comp == v) atomicAdd(&s_tot[3], 1);
            atomicMax(&s_tot[4], ecc);
        }
    }
    __syncthreads();
    long long* hist = o.distance_histogram + (size_t)b * n_max;
    for (int k = tid; k < n_max; k += blockDim.x) hist[k] = (k >= 1 && k < n) ? (long long)s_hist[k] : 0ll;
    if (tid == 0) {
        const int diam = s_tot[4];
        double acc = 0.0;
        long long pairs = 0, dist = 0;
        for (int k = 1; k <= diam; ++k) {
            const int c = s_hist[k];
            if (c) acc = acc + (double)c / (double)k;
            pairs += c;
            dist += (long long)k * c;
        }
        o.edges[b] = (long long)(s_tot[0] >> 1);
        o.components[b] = s_tot[3];
        o.diameter[b] = diam;
        o.global_efficiency[b] = n < 2 ? 0.0 : acc / (double)((long long)n * (n - 1));
        o.characteristic_path_length[b] = pairs ? (double)dist / (double)pairs : topo_nan();
        o.transitivity[b] = s_tot[2] ? (double)s_tot[1] / (double)s_tot[2] : 0.0;
    }
    if (tid == 64) {                                    // another wave: the sequential mean beside the pass above
        double acc = 0.0;
        for (int v = 0; v < n; ++v) acc = acc + s_clu[v];
        o.mean_clustering[b] = n ? acc / (double)n : 0.0;
    }
}

// ---------------------------------------------------------------------------------------------- local efficiency
// The workgroup walks the nodes v in order.  The neighbours of v are dealt to the groups in turn; each group searches
// from its share inside the subgraph induced by N(v) (allowed = row v) and adds the level counts to the node's histogram
// with integer LDS atomics.  After a barrier thread 0 forms the node's value from the finished histogram and clears it
// while the other groups start on v + 1, whose histogram is the other of two buffers: one barrier per node.
// LDS: [n_max doubles: values][2 x n_max ints: histograms][8 ints: 0, 1 the largest distance in each buffer][rows].
template <int G>
__global__ void __launch_bounds__(topo_threads(G)) gnm_topology_local_kernel(
    const int32_t* __restrict__ rowptr, const uint16_t* __restrict__ col, const int64_t* __restrict__ b_rp_off,
    const int64_t* __restrict__ b_col_off, const int32_t* __restrict__ node_off, int n_max,
    double* __restrict__ local_efficiency, double* __restrict__ mean_local_efficiency) {
#pragma clang fp contract(off)
    extern __shared__ double topo_lds[];
    const int b = blockIdx.x, tid = threadIdx.x;
    const TopoGraph g = topo_graph(rowptr, col, b_rp_off, b_col_off, node_off, b);
    const int n = g.n;
    if (n < 0 || n > n_max) return;
    double* s_val = topo_lds;
    int* s_hist = reinterpret_cast<int*>(s_val + n_max);
    int* s_kmax = s_hist + 2 * n_max;
    uint32_t* rows = reinterpret_cast<uint32_t*>(s_kmax + 8);
    const int W = topo_words(n), stride = topo_stride(n);
    for (int i = tid; i < 2 * n_max + 8; i += blockDim.x) s_hist[i] = 0;
    topo_stage(rows, n, stride, g.rp, g.col);

    constexpr int NG = topo_threads(G) / G;
    const int grp = tid / G, gl = tid & (G - 1), gshift = (tid & 63) & ~(G - 1);
    const int jj = gl < W ? gl : 0;
    const uint32_t live = gl < W ? 0xffffffffu : 0u;
    for (int v = 0; v < n; ++v) {
        int* hist = s_hist + (v & 1) * n_max;
        const uint32_t row_v = rows[v * stride + jj] & live;
        const int d = group_sum<G>(__popc(row_v));      // the same in every group
        if (d >= 2) {
            int turn = 0, kmax = 0, unused = 0;
            uint32_t m = group_nonzero<G>(row_v, gshift);
            while (m) {
                const int q = __builtin_ctz(m);
                m &= m - 1;
                uint32_t w = __shfl(row_v, q, G);
                while (w) {
                    const int u = (q << 5) + __builtin_ctz(w);
                    w &= w - 1;
                    if (turn == grp) {
                        topo_bfs<G, false>(rows, stride, jj, gl, gshift, u, row_v, 0u, unused, [&](int k, int c) {
                            kmax = max(kmax, k);
                            if (gl == 0) atomicAdd(&hist[k], c);
                        });
                    }
                    turn = turn + 1 == NG ? 0 : turn + 1;
                }
            }
            if (gl == 0 && kmax) atomicMax(&s_kmax[v & 1], kmax);
        }
        __syncthreads();
        if (tid == 0) {
            const int kmax = s_kmax[v & 1];
            double acc = 0.0;
            for (int k = 1; k <= kmax; ++k) {
                const int c = hist[k];
                if (c) acc = acc + (double)c / (double)k;
                hist[k] = 0;
            }
            s_kmax[v & 1] = 0;
            const double val = d < 2 ? 0.0 : acc / (double)(d * (d - 1));
            s_val[v] = val;
            local_efficiency[g.row0 + v] = val;
        }
    }
    __syncthreads();
    if (tid == 0) {
        double acc = 0.0;
        for (int v = 0; v < n; ++v) acc = acc + s_val[v];
        mean_local_efficiency[b] = n ? acc / (double)n : 0.0;
    }
}

size_t topo_nodes_lds(int n_max) {
    return (size_t)n_max * 8 + ((size_t)n_max + 8) * 4 + (size_t)n_max * topo_stride(n_max) * 4;
}
size_t topo_local_lds(int n_max) {
    return (size_t)n_max * 8 + (2 * (size_t)n_max + 8) * 4 + (size_t)n_max * topo_stride(n_max) * 4;
}
static_assert((size_t)kTopoMaxN * 8 + (2 * (size_t)kTopoMaxN + 8) * 4 + (size_t)kTopoMaxN * (kTopoMaxN / 32 + 1) * 4
                  <= (size_t)kLdsBudget, "the largest graph's rows and scratch must fit one CU's LDS");

}  // namespace

extern "C" int gnm_topology_max_nodes(void) { return kTopoMaxN; }

// No entry point needs global scratch: every count lives in the owning workgroup's LDS.
extern "C" long long gnm_topology_workspace_bytes(int B, int n_max, int flags) {
    (void)flags;
    return topo_check(B, n_max) == GNM_OK ? 0 : -1;
}

extern "C" int gnm_topology_nodes(const int32_t* rowptr, const uint16_t* col, const int64_t* b_rp_off,
                                  const int64_t* b_col_off, const int32_t* node_off, int B, int n_max, int32_t* degree,
                                  int32_t* triangles, double* clustering, int32_t* eccentricity, int32_t* reachable,
                                  int32_t* distance_sum, int32_t* component, double* nodal_efficiency, long long* edges,
                                  int32_t* components, long long* distance_histogram, int32_t* diameter,
                                  double* global_efficiency, double* characteristic_path_length, double* transitivity,
                                  double* mean_clustering, void* stream) {
    if (int e = topo_check(B, n_max)) return e;
    if (B == 0) return GNM_OK;
    if (!rowptr || !col || !b_rp_off || !b_col_off || !node_off || !degree || !triangles || !clustering ||
        !eccentricity || !reachable || !distance_sum || !component || !nodal_efficiency || !edges || !components ||
        !distance_histogram || !diameter || !global_efficiency || !characteristic_path_length || !transitivity ||
        !mean_clustering)
        return GNM_ERR_BAD_ARG;
    TopoNodeOut o{degree, triangles, eccentricity, reachable, distance_sum, component, clustering, nodal_efficiency,
                  edges, distance_histogram, components, diameter, global_efficiency, characteristic_path_length,
                  transitivity, mean_clustering};
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const size_t lds = topo_nodes_lds(n_max);
    if (topo_words(n_max) <= kTopoSmallW) {
        GNM_ALLOW_FULL_LDS(gnm_topology_nodes_kernel<16>);
        hipLaunchKernelGGL(gnm_topology_nodes_kernel<16>, dim3((unsigned)B), dim3(topo_threads(16)), lds, s, rowptr, col,
                           b_rp_off, b_col_off, node_off, n_max, o);
    } else {
        GNM_ALLOW_FULL_LDS(gnm_topology_nodes_kernel<32>);
        hipLaunchKernelGGL(gnm_topology_nodes_kernel<32>, dim3((unsigned)B), dim3(topo_threads(32)), lds, s, rowptr, col,
                           b_rp_off, b_col_off, node_off, n_max, o);
    }
    GNM_CHECK_LAUNCH();
    return GNM_OK;
}

extern "C" int gnm_topology_local(const int32_t* rowptr, const uint16_t* col, const int64_t* b_rp_off,
                                  const int64_t* b_col_off, const int32_t* node_off, int B, int n_max, void* workspace,
                                  double* local_efficiency, double* mean_local_efficiency, void* stream) {
    (void)workspace;
    if (int e = topo_check(B, n_max)) return e;
    if (B == 0) return GNM_OK;
    if (!rowptr || !col || !b_rp_off || !b_col_off || !node_off || !local_efficiency || !mean_local_efficiency)
        return GNM_ERR_BAD_ARG;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const size_t lds = topo_local_lds(n_max);
    if (topo_words(n_max) <= kTopoSmallW) {
        GNM_ALLOW_FULL_LDS(gnm_topology_local_kernel<16>);
        hipLaunchKernelGGL(gnm_topology_local_kernel<16>, dim3((unsigned)B), dim3(topo_threads(16)), lds, s, rowptr, col,
                           b_rp_off, b_col_off, node_off, n_max, local_efficiency, mean_local_efficiency);
    } else {
        GNM_ALLOW_FULL_LDS(gnm_topology_local_kernel<32>);
        hipLaunchKernelGGL(gnm_topology_local_kernel<32>, dim3((unsigned)B), dim3(topo_threads(32)), lds, s, rowptr, col,
                           b_rp_off, b_col_off, node_off, n_max, local_efficiency, mean_local_efficiency);
    }
    GNM_CHECK_LAUNCH();
    return GNM_OK;
}
