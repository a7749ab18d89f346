// Connectome graphs from functional-connectivity matrices, on the device: the first stage of the reference's data path
// (util.py:20-122 load_data, dataset.py:93-101 DataEdges.get_adjacency) for a whole [S, n, n] fp64 stack at once.
//
//   gnm_connectome_thresholds  np.percentile(fc[s], 100 - sparsity) per matrix (dataset.py:94), bitwise: an exact radix
//                              select of the two order statistics numpy's "linear" method reads, then numpy's _lerp.
//   gnm_connectome_structure   the upper-triangle edges fc[s, u, v] > thr[s] (dataset.py:94-100) as bit rows, node
//                              degrees, and the node order networkx gives the graph load_data builds (util.py:43-76):
//                              rank[y] = place of y in pi, the nodes sorted by (t(y), y), t(y) the first row i < y with
//                              an edge {i, y} (y itself if none).  Per graph: edge count and "has an isolated node".
//   gnm_connectome_knn_structure  the same workspace from another edge rule: row i selects its k largest entries, and
//                              {u, v} is an edge when either end (or, "mutual", each end) selects the other.
//   gnm_connectome_emit        the graph's arena CSR (util.py:97-103 edge_mat, then GraphArena.add's host CSR,
//                              gnm_csr_from_edge_mat + gnm_csr_parity_order): row x lists its later-in-pi neighbours by
//                              ascending id, then its earlier-in-pi neighbours in pi order, then the parity reorder.
//
// One workgroup per matrix in every kernel; graphs are independent.  Every store of the emission kernel is guarded by
// the row's reserved length, so a workspace that does not come from gnm_connectome_structure cannot write past it.
#include "gnm_common.h"

namespace {

constexpr int kCtThreads = 1024;
constexpr int kCtWaves = kCtThreads / kWave;
constexpr int kCtMaxN = 4096;           // uint16 columns; n^2 fp64 = 128 MiB per matrix at the limit
constexpr unsigned long long kEvenLanes = 0x5555555555555555ull;

// fp64 -> unsigned key with the same order (negative values bit-inverted, positive ones with the sign bit set)
__device__ __forceinline__ unsigned long long ct_key(double x) {
    const unsigned long long u = (unsigned long long)__double_as_longlong(x);
    return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}
__device__ __forceinline__ double ct_unkey(unsigned long long k) {
    const unsigned long long u = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
    return __longlong_as_double((long long)u);
}

__device__ __forceinline__ unsigned long long lanes_below() {
    const unsigned lane = threadIdx.x & 63;
    return lane ? (~0ull >> (64 - lane)) : 0ull;
}

// words per bit row of the upper-triangle edge matrix, and the per-graph workspace layout (32-bit words):
// [n * W bit rows][n ranks][n degrees], rounded up to 4 words
__host__ __device__ inline int ct_row_words(int n) { return (n + 31) >> 5; }
__host__ __device__ inline long long ct_graph_words(int n) {
    return (((long long)n * ct_row_words(n) + 2LL * n) + 3) & ~3LL;
}

// exclusive prefix sum of v[0..n) in place (n <= kCtMaxN, every thread of the block calls it); returns the total
__device__ int ct_block_scan(int* v, int n, int* s_wave) {
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int per = (n + kCtThreads - 1) / kCtThreads;       // <= 4
    const int b = t * per;
    int local = 0;
    for (int i = 0; i < per; ++i)
        if (b + i < n) local += v[b + i];
    int incl = local;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int o = __shfl_up(incl, off, 64);
        if (lane >= off) incl += o;
    }
    if (lane == 63) s_wave[wave] = incl;
    __syncthreads();
    int before = 0, total = 0;
    for (int w = 0; w < kCtWaves; ++w) {
        before += w < wave ? s_wave[w] : 0;
        total += s_wave[w];
    }
    int run = before + incl - local;
    for (int i = 0; i < per; ++i)
        if (b + i < n) {
            const int x = v[b + i];
            v[b + i] = run;
            run += x;
        }
    __syncthreads();
    return total;
}

// ---------------------------------------------------------------------------------------------------- thresholds
// Order statistics k_lo and k_hi (= k_lo or k_lo + 1) of the N = n^2 values of one matrix by an 8-bit radix select on
// ct_key (per-wave histograms in LDS), then numpy's _lerp (numpy/lib/_function_base_impl.py):
//   diff = b - a;  r = a + diff * gamma;  r = b - diff * (1 - gamma) where gamma >= 0.5
// A NaN anywhere makes the threshold NaN (numpy's slices_having_nans).
__global__ void __launch_bounds__(kCtThreads) gnm_connectome_thr_kernel(const double* __restrict__ fc, int n,
                                                                       long long k_lo, long long k_hi, double gamma,
                                                                       double* __restrict__ thr) {
    __shared__ unsigned s_hist[kCtWaves][256];
    __shared__ unsigned long long s_sel[3];                   // prefix, rank left inside the bucket, bucket count
    __shared__ unsigned long long s_min[kCtWaves];
    __shared__ int s_nan;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const long long N = (long long)n * n;
    const double* m = fc + (size_t)blockIdx.x * (size_t)N;
    if (t == 0) { s_sel[0] = 0; s_sel[1] = (unsigned long long)k_lo; s_nan = 0; }
    unsigned long long mask = 0;
    for (int shift = 56; shift >= 0; shift -= 8) {
        for (int i = t; i < kCtWaves * 256; i += kCtThreads) (&s_hist[0][0])[i] = 0u;
        __syncthreads();
        const unsigned long long prefix = s_sel[0];
        int nan = 0;
        for (long long i = t; i < N; i += kCtThreads) {
            const double x = m[i];
            nan |= (x != x);
            const unsigned long long k = ct_key(x);
            if ((k & mask) == prefix) atomicAdd(&s_hist[wave][(unsigned)(k >> shift) & 255u], 1u);
        }
        if (shift == 56 && __any(nan) && lane == 0) s_nan = 1;
        __syncthreads();
        if (s_nan) {
            if (t == 0) thr[blockIdx.x] = __longlong_as_double(0x7ff8000000000000ll);
            return;
        }
        if (t < 256) {
            unsigned c = 0;
            for (int w = 0; w < kCtWaves; ++w) c += s_hist[w][t];
            s_hist[0][t] = c;
        }
        __syncthreads();
        if (t == 0) {
            unsigned long long r = s_sel[1];
            int d = 0;
            while (r >= s_hist[0][d]) { r -= s_hist[0][d]; ++d; }
            s_sel[0] = prefix | ((unsigned long long)d << shift);
            s_sel[1] = r;
            s_sel[2] = s_hist[0][d];
        }
        mask |= 255ull << shift;
        __syncthreads();
    }
    const unsigned long long ka = s_sel[0];
    unsigned long long kb = ka;
    // k_hi = k_lo + 1 lies past the equal run of a: the smallest key above a
    if (k_hi != k_lo && s_sel[1] + 1 >= s_sel[2]) {
        unsigned long long best = ~0ull;
        for (long long i = t; i < N; i += kCtThreads) {
            const unsigned long long k = ct_key(m[i]);
            if (k > ka && k < best) best = k;
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const unsigned long long o = __shfl_xor(best, off, 64);
            best = o < best ? o : best;
        }
        if (lane == 0) s_min[wave] = best;
        __syncthreads();
        kb = s_min[0];
        for (int w = 1; w < kCtWaves; ++w) kb = s_min[w] < kb ? s_min[w] : kb;
    }
    if (t == 0) {
#pragma clang fp contract(off)
        const double a = ct_unkey(ka), b = ct_unkey(kb);
        const double diff = b - a;
        double r = a + diff * gamma;
        if (gamma >= 0.5) r = b - diff * (1.0 - gamma);
        thr[blockIdx.x] = r;
    }
}

// ---------------------------------------------------------------------------------------------------- structure
// From an edge rule to the workspace of one graph: upper-triangle bit rows, degrees, the node order, nnz and iso.  The
// rule is a type with  load(i, v) -> value  (called for i < v < n, all loads of four chunks before their tests) and
// test(value) -> bool: the percentile rule reads fc and compares, the kNN rule reads two selection bits.
struct CtLds {
    int *t, *deg, *cnt;     // [kCtMaxN] each
    int *wave;              // [kCtWaves]
    int *red;               // [2]
};

template <class Rule>
__device__ __forceinline__ void ct_structure(const Rule& rule, int n, int g, uint32_t* __restrict__ work,
                                             int32_t* __restrict__ nnz_out, int32_t* __restrict__ iso_out,
                                             const CtLds& s) {
    int *s_t = s.t, *s_deg = s.deg, *s_cnt = s.cnt, *s_wave = s.wave, *s_red = s.red;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int W = ct_row_words(n);
    uint32_t* bits = work + (size_t)g * (size_t)ct_graph_words(n);
    int32_t* rank = reinterpret_cast<int32_t*>(bits + (size_t)n * W);
    int32_t* deg = rank + n;
    for (int v = t; v < n; v += kCtThreads) { s_t[v] = v; s_deg[v] = 0; s_cnt[v] = 0; }
    if (t < 2) s_red[t] = 0;
    __syncthreads();
    // upper-triangle edges, one wave per row i: bits of v > i, degrees of both ends, t(v) = min i
    for (int i = wave; i < n; i += kCtWaves) {
        uint32_t* ub = bits + (size_t)i * W;
        const int first = (i + 1) & ~63;                      // 64-column chunk holding column i + 1
        for (int w = lane; w < (first >> 5) && w < W; w += 64) ub[w] = 0u;
        int up = 0;
        for (int base = first; base < n; base += 256) {
            typename Rule::value x[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int v = base + 64 * u + lane;
                x[u] = (v > i && v < n) ? rule.load(i, v) : typename Rule::value(0);
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int b0 = base + 64 * u;
                if (b0 >= n) break;
                const int v = b0 + lane;
                const bool e = v > i && v < n && rule.test(x[u]);
                const unsigned long long bm = __ballot(e);
                if (lane == 0) {
                    ub[b0 >> 5] = (uint32_t)bm;
                    if ((b0 >> 5) + 1 < W) ub[(b0 >> 5) + 1] = (uint32_t)(bm >> 32);
                }
                if (e) { atomicMin(&s_t[v], i); atomicAdd(&s_deg[v], 1); }
                up += __popcll(bm);
            }
        }
        if (lane == 0 && up) atomicAdd(&s_deg[i], up);
    }
    __syncthreads();
    int e2 = 0, iso = 0;
    for (int v = t; v < n; v += kCtThreads) {
        const int d = s_deg[v];
        deg[v] = d;
        e2 += d;
        iso |= d == 0;
        atomicAdd(&s_cnt[s_t[v]], 1);
    }
    if (e2) atomicAdd(&s_red[0], e2);
    if (iso) s_red[1] = 1;
    __syncthreads();
    ct_block_scan(s_cnt, n, s_wave);                           // s_cnt[j]: first place in pi of bucket t = j
    // inside bucket j the nodes keep ascending id: one wave per bucket, ballot compaction over v >= j
    for (int j = wave; j < n; j += kCtWaves) {
        int run = s_cnt[j];
        for (int base = j & ~63; base < n; base += 64) {
            const int v = base + lane;
            const bool f = v >= j && v < n && s_t[v] == j;
            const unsigned long long bm = __ballot(f);
            if (f) rank[v] = run + __popcll(bm & lanes_below());
            run += __popcll(bm);
        }
    }
    if (t == 0) { nnz_out[g] = s_red[0]; iso_out[g] = s_red[1]; }
}

// dataset.py:94-100: fc[s, i, v] > thr[s]
struct CtPercentileRule {
    typedef double value;
    const double* __restrict__ m;
    int n;
    double th;
    __device__ __forceinline__ double load(int i, int v) const { return m[(size_t)i * n + v]; }
    __device__ __forceinline__ bool test(double x) const { return x > th; }
};

__global__ void __launch_bounds__(kCtThreads) gnm_connectome_structure_kernel(const double* __restrict__ fc, int n,
                                                                             const double* __restrict__ thr,
                                                                             uint32_t* __restrict__ work,
                                                                             int32_t* __restrict__ nnz_out,
                                                                             int32_t* __restrict__ iso_out) {
    __shared__ int s_t[kCtMaxN], s_deg[kCtMaxN], s_cnt[kCtMaxN];
    __shared__ int s_wave[kCtWaves];
    __shared__ int s_red[2];
    const int g = blockIdx.x;
    const CtPercentileRule rule{fc + (size_t)g * (size_t)n * (size_t)n, n, thr[g]};
    ct_structure(rule, n, g, work, nnz_out, iso_out, CtLds{s_t, s_deg, s_cnt, s_wave, s_red});
}

// ---------------------------------------------------------------------------------------------------- kNN structure
// k-nearest-neighbour edges of one matrix fc[s] ([n, n], read as stored: it need not be symmetric):
//   candidates  of row i: the columns v != i with fc[s, i, v] not NaN;
//   key         fc[s, i, v], or |fc[s, i, v]| (flags bit 1, "absolute"); +0.0 and -0.0 are one key, +-inf ordinary;
//   order       descending key, ascending column among equal keys;
//   selection   row i selects its first min(k, number of candidates) candidates in that order;
//   edge        {u, v}, u < v: u selects v or v selects u; with flags bit 0 ("mutual"): and.
// Phase 1, one wave per row: the min(k, candidates)-th key by an 8-bit radix select over ct_key (the wave's histogram in
// LDS, the digit found by a wave scan from the top bin down), left as soon as the bucket of the sought key is wanted
// whole; then one pass takes every column above the found prefix and the first `need` columns equal to it, ascending
// (ballot prefix per 64-column chunk), and writes the row's directed selection bits to sel.  Phase 2, after a barrier:
// ct_structure with the rule sel[i][v] | sel[v][i] (or &).  No float arithmetic, no float atomics: the bits depend on
// the matrix alone.  The histograms of phase 1 lie in the LDS that phase 2 uses for its bucket counts.
__device__ __forceinline__ void ct_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// the key of a candidate value: -0.0 made +0.0 (ct_key orders them apart), the sign dropped under `absolute`
__device__ __forceinline__ unsigned long long ct_knn_key(double x, bool absolute) {
    if (absolute) x = fabs(x);
    if (x == 0.0) x = 0.0;
    return ct_key(x);
}

struct CtKnnRule {
    typedef uint32_t value;
    const uint32_t* sel;    // [n, W] of this graph, written by this workgroup in phase 1
    int W;
    bool mutual;
    __device__ __forceinline__ uint32_t load(int i, int v) const {
        const uint32_t a = (sel[(size_t)i * W + (v >> 5)] >> (v & 31)) & 1u;
        const uint32_t b = (sel[(size_t)v * W + (i >> 5)] >> (i & 31)) & 1u;
        return mutual ? (a & b) : (a | b);
    }
    __device__ __forceinline__ bool test(uint32_t x) const { return x != 0u; }
};

static_assert(kCtWaves * 256 <= kCtMaxN, "the per-wave histograms of the kNN select alias the bucket counts");

__global__ void __launch_bounds__(kCtThreads) gnm_connectome_knn_kernel(const double* __restrict__ fc, int n, int k,
                                                                       int flags, uint32_t* sel_all,
                                                                       uint32_t* __restrict__ work,
                                                                       int32_t* __restrict__ nnz_out,
                                                                       int32_t* __restrict__ iso_out) {
    __shared__ int s_t[kCtMaxN], s_deg[kCtMaxN], s_cnt[kCtMaxN];
    __shared__ int s_wave[kCtWaves];
    __shared__ int s_red[2];
    const int g = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int W = ct_row_words(n);
    const bool absolute = flags & 2;
    const double* m = fc + (size_t)g * (size_t)n * (size_t)n;
    uint32_t* sel = sel_all + (size_t)g * (size_t)n * W;
    unsigned* hist = reinterpret_cast<unsigned*>(s_cnt) + wave * 256;
    const unsigned long long below = lanes_below();
    for (int i = wave; i < n; i += kCtWaves) {
        const double* row = m + (size_t)i * n;
        unsigned long long prefix = 0, mask = 0;
        int need = min(k, n - 1);
        for (int shift = 56; shift >= 0; shift -= 8) {
#pragma unroll
            for (int j = 0; j < 4; ++j) hist[4 * lane + j] = 0u;
            ct_wave_sync();
            for (int base = 0; base < n; base += 256) {
                double x[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int v = base + 64 * u + lane;
                    x[u] = (v < n && v != i) ? row[v] : __longlong_as_double(0x7ff8000000000000ll);
                }
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    if (x[u] == x[u]) {
                        const unsigned long long key = ct_knn_key(x[u], absolute);
                        if ((key & mask) == prefix) atomicAdd(&hist[(unsigned)(key >> shift) & 255u], 1u);
                    }
                }
            }
            ct_wave_sync();
            // bins 4 lane .. 4 lane + 3 in this lane; above = keys in the bins of higher lanes
            int h[4], mine = 0;
#pragma unroll
            for (int j = 0; j < 4; ++j) { h[j] = (int)hist[4 * lane + j]; mine += h[j]; }
            int incl = mine;
#pragma unroll
            for (int off = 1; off < 64; off <<= 1) {
                const int o = __shfl_up(incl, off, 64);
                if (lane >= off) incl += o;
            }
            const int total = __shfl(incl, 63, 64);
            if (shift == 56) need = min(need, total);          // total: the row's candidates
            if (need == 0) { prefix = mask = ~0ull; break; }   // nothing to select: no key is above or equal
            int above = total - incl, digit = 0, count = 0;
            const bool here = above < need && need <= above + mine;
            if (here) {
#pragma unroll
                for (int j = 3; j >= 0; --j) {
                    if (need <= above + h[j]) { digit = 4 * lane + j; count = h[j]; break; }
                    above += h[j];
                }
            }
            const int src = __ffsll((long long)__ballot(here)) - 1;      // exactly one lane
            digit = __shfl(digit, src, 64);
            above = __shfl(above, src, 64);
            count = __shfl(count, src, 64);
            need -= above;
            prefix |= (unsigned long long)digit << shift;
            mask |= 255ull << shift;
            if (need == count) break;                          // the whole bucket is selected
        }
        // every column above the prefix, then the first `need` columns equal to it
        uint32_t* sb = sel + (size_t)i * W;
        int taken = 0;
        for (int base = 0; base < n; base += 64) {
            const int v = base + lane;
            bool gt = false, eq = false;
            if (v < n && v != i) {
                const double x = row[v];
                if (x == x) {
                    const unsigned long long km = ct_knn_key(x, absolute) & mask;
                    gt = km > prefix;
                    eq = km == prefix;
                }
            }
            const unsigned long long be = __ballot(eq);
            const unsigned long long bm = __ballot(gt || (eq && taken + __popcll(be & below) < need));
            if (lane == 0) {
                sb[base >> 5] = (uint32_t)bm;
                if ((base >> 5) + 1 < W) sb[(base >> 5) + 1] = (uint32_t)(bm >> 32);
            }
            taken += __popcll(be);
        }
    }
    __syncthreads();                                           // sel complete and visible; the histograms are free
    const CtKnnRule rule{sel, W, (flags & 1) != 0};
    ct_structure(rule, n, g, work, nnz_out, iso_out, CtLds{s_t, s_deg, s_cnt, s_wave, s_red});
}

// ---------------------------------------------------------------------------------------------------- emission
// Final place of the m-th even (odd) id of a row with ne even and no odd ids after gnm_csr_parity_order: the pattern
// E E O O E E O O ... holds until the first position whose kind has run out; the other kind fills the rest in order.
__device__ __forceinline__ int ct_pe(int m) { return 4 * (m >> 1) + (m & 1); }
__device__ __forceinline__ int ct_po(int m) { return 4 * (m >> 1) + 2 + (m & 1); }
__device__ __forceinline__ int ct_place(int m, bool odd, int cut) {
    const int p = odd ? ct_po(m) : ct_pe(m);
    if (p < cut) return p;
    const int before = 2 * (cut >> 2) + (odd ? max((cut & 3) - 2, 0) : min(cut & 3, 2));
    return cut + m - before;
}

__global__ void __launch_bounds__(kCtThreads) gnm_connectome_emit_kernel(const uint32_t* __restrict__ work, int n,
                                                                        int32_t* __restrict__ rowptr,
                                                                        uint16_t* __restrict__ col,
                                                                        const int64_t* __restrict__ g_rp_off,
                                                                        const int64_t* __restrict__ g_col_off) {
    __shared__ int s_rank[kCtMaxN], s_pi[kCtMaxN], s_rp[kCtMaxN + 1];
    __shared__ int s_wave[kCtWaves];
    const int g = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int W = ct_row_words(n);
    const uint32_t* bits = work + (size_t)g * (size_t)ct_graph_words(n);
    const int32_t* rank = reinterpret_cast<const int32_t*>(bits + (size_t)n * W);
    const int32_t* deg = rank + n;
    int32_t* rp = rowptr + g_rp_off[g];
    uint16_t* cl = col + g_col_off[g];
    for (int v = t; v < n; v += kCtThreads) {
        const int r = rank[v];
        s_rank[v] = r;
        if ((unsigned)r < (unsigned)n) s_pi[r] = v;
        s_rp[v] = deg[v];
    }
    __syncthreads();
    const int total = ct_block_scan(s_rp, n, s_wave);
    if (t == 0) s_rp[n] = total;
    __syncthreads();
    for (int v = t; v <= n; v += kCtThreads) rp[v] = s_rp[v];
    // edge {x, v}: the bit of the lower id's row
    auto edge = [&](int x, int v) -> bool {
        if (v == x || v < 0 || v >= n) return false;
        const int a = min(x, v), b = max(x, v);
        return (bits[(size_t)a * W + (b >> 5)] >> (b & 31)) & 1u;
    };
    for (int x = wave; x < n; x += kCtWaves) {
        const int start = s_rp[x], dx = s_rp[x + 1] - start;
        if (dx == 0) continue;
        const int rx = s_rank[x];
        int ne = 0;
        for (int base = 0; base < n; base += 64) ne += __popcll(__ballot(edge(x, base + lane)) & kEvenLanes);
        const int cut = min(ct_pe(ne), ct_po(dx - ne));
        int me = 0, mo = 0;
        const unsigned long long below = lanes_below();
        // later in pi, ascending id
        for (int base = 0; base < n; base += 64) {
            const int v = base + lane;
            const bool f = edge(x, v) && s_rank[v] > rx;
            const unsigned long long bm = __ballot(f);
            const unsigned long long be = bm & kEvenLanes, bo = bm & ~kEvenLanes;
            if (f) {
                const bool odd = v & 1;
                const int mm = odd ? mo + __popcll(bo & below) : me + __popcll(be & below);
                const int pos = ct_place(mm, odd, cut);
                if (pos < dx) cl[start + pos] = (uint16_t)v;
            }
            me += __popcll(be);
            mo += __popcll(bo);
        }
        // earlier in pi, in pi order
        for (int base = 0; base < rx; base += 64) {
            const int p = base + lane;
            const int y = p < rx ? s_pi[p] : -1;
            const bool f = y >= 0 && edge(x, y);
            const bool odd = y & 1;
            const unsigned long long be = __ballot(f && !odd), bo = __ballot(f && odd);
            if (f) {
                const int mm = odd ? mo + __popcll(bo & below) : me + __popcll(be & below);
                const int pos = ct_place(mm, odd, cut);
                if (pos < dx) cl[start + pos] = (uint16_t)y;
            }
            me += __popcll(be);
            mo += __popcll(bo);
        }
    }
}

}  // namespace

extern "C" int gnm_connectome_max_nodes(void) { return kCtMaxN; }

extern "C" long long gnm_connectome_workspace_words(int S, int n) {
    if (S < 0 || n < 1 || n > kCtMaxN) return -1;
    return (long long)S * ct_graph_words(n);
}

// dataset.py:94 np.percentile(self.df, threshold), one matrix per workgroup
extern "C" int gnm_connectome_thresholds(const double* fc, int S, int n, long long k_lo, long long k_hi, double gamma,
                                         double* thr, void* stream) {
    if (S < 0 || n < 1) return GNM_ERR_BAD_ARG;
    if (n > kCtMaxN) return GNM_ERR_UNSUPPORTED;
    const long long N = (long long)n * n;
    if (k_lo < 0 || k_hi < k_lo || k_hi - k_lo > 1 || k_hi >= N || !(gamma >= 0.0)) return GNM_ERR_BAD_ARG;
    if (S == 0) return GNM_OK;
    if (!fc || !thr) return GNM_ERR_BAD_ARG;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(gnm_connectome_thr_kernel, dim3(S), dim3(kCtThreads), 0, s, fc, n, k_lo, k_hi, gamma, thr);
    GNM_CHECK_LAUNCH();
    return GNM_OK;
}

// dataset.py:94-100 (mask > percentile, upper triangle) and util.py:43-76 (the networkx graph's node order)
extern "C" int gnm_connectome_structure(const double* fc, int S, int n, const double* thr, uint32_t* work,
                                        int32_t* nnz, int32_t* iso, void* stream) {
    if (S < 0 || n < 1) return GNM_ERR_BAD_ARG;
    if (n > kCtMaxN) return GNM_ERR_UNSUPPORTED;
    if (S == 0) return GNM_OK;
    if (!fc || !thr || !work || !nnz || !iso || (reinterpret_cast<uintptr_t>(work) & 15)) return GNM_ERR_BAD_ARG;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(gnm_connectome_structure_kernel, dim3(S), dim3(kCtThreads), 0, s, fc, n, thr, work, nnz, iso);
    GNM_CHECK_LAUNCH();
    return GNM_OK;
}

extern "C" long long gnm_connectome_knn_scratch_words(int S, int n) {
    if (S < 0 || n < 1 || n > kCtMaxN) return -1;
    return (long long)S * n * ct_row_words(n);
}

// the kNN edge rule (contract above gnm_connectome_knn_kernel) into the workspace layout of gnm_connectome_structure;
// flags: bit 0 mutual, bit 1 absolute; k >= n behaves as n - 1
extern "C" int gnm_connectome_knn_structure(const double* fc, int S, int n, int k, int flags, uint32_t* sel,
                                            uint32_t* work, int32_t* nnz, int32_t* iso, void* stream) {
    if (S < 0 || n < 1 || k < 1 || (flags & ~3)) return GNM_ERR_BAD_ARG;
    if (n > kCtMaxN) return GNM_ERR_UNSUPPORTED;
    if (S == 0) return GNM_OK;
    if (!fc || !sel || !work || !nnz || !iso || (reinterpret_cast<uintptr_t>(work) & 15) ||
        (reinterpret_cast<uintptr_t>(sel) & 3))
        return GNM_ERR_BAD_ARG;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(gnm_connectome_knn_kernel, dim3(S), dim3(kCtThreads), 0, s, fc, n, k, flags, sel, work, nnz,
                       iso);
    GNM_CHECK_LAUNCH();
    return GNM_OK;
}

// util.py:97-103 (edge_mat from g.g.edges()) and the host CSR GraphArena.add builds from it (gnm/arena.py _host_csr)
extern "C" int gnm_connectome_emit(const uint32_t* work, int S, int n, int32_t* rowptr, uint16_t* col,
                                   const int64_t* g_rp_off, const int64_t* g_col_off, void* stream) {
    if (S < 0 || n < 1) return GNM_ERR_BAD_ARG;
    if (n > kCtMaxN) return GNM_ERR_UNSUPPORTED;
    if (S == 0) return GNM_OK;
    if (!work || !rowptr || !col || !g_rp_off || !g_col_off || (reinterpret_cast<uintptr_t>(work) & 15))
        return GNM_ERR_BAD_ARG;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(gnm_connectome_emit_kernel, dim3(S), dim3(kCtThreads), 0, s, work, n, rowptr, col, g_rp_off,
                       g_col_off);
    GNM_CHECK_LAUNCH();
    return GNM_OK;
}
