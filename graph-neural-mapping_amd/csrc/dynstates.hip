// Connectivity states: Lloyd's k-means over the window FC matrices the sliding-window kernels make (csrc/timeseries.hip,
// gnm_dynfc_corr), on the device and all in fp64.  The features of a window are the P = n (n - 1) / 2 entries
// fc[w, i, j] with i < j; the lower triangle is never read (gnm_dynfc_corr writes R_ij and R_ji by different division
// orders, so the triangles differ in the last bit).
//
//   gnm_states_assign       dist[w, c] = sum_{i < j} (fc[w, i, j] - M[c, i, j])^2, formed directly (the expanded form
//                           |x|^2 - 2 x.m + |m|^2 cancels); label[w] = the smallest c with the least distance, or -1 when
//                           one of the k distances is not finite (a NaN or inf above the diagonal: a constant ROI).
//   gnm_states_accumulate   sum[c, i, j] (i <= j) += fc[w, i, j] over the windows with label[w] == c, one after the other
//                           in ascending w, carried in `sum` from one call to the next; count[c] beside it.
//   gnm_states_finish       M[c, i, j] = M[c, j, i] = sum[c, i, j] / count[c], one IEEE division; a cluster without
//                           members keeps its centroid.
//   gnm_states_inertia      the assigned distances of the valid windows added in ascending w.
//
// No atomics.  Every sum has an order that depends on the window's own entries alone (assign) or on the global window
// order alone (accumulate, inertia), so a window's dist row does not depend on the call it is part of and a centroid
// does not depend on how the windows are chunked.
#include "gnm_common.h"

namespace {

constexpr int kStMaxN = 4096;           // = gnm_timeseries_max_nodes(): the windows come from gnm_dynfc_corr
constexpr int kStMaxK = 16;             // accumulators per thread of the assignment kernel
constexpr int kBlk = 64;                // block of the 64 x 64 upper block pairs, gnm_dynfc_corr's partition
constexpr int kThreads = 256;
constexpr int kRowsPer = kBlk * kBlk / kThreads;    // entries of a block one thread owns (16): rows wave + 4 u
// windows one pass over the centroid tiles serves in the assignment kernel at k centroids
constexpr int st_windows_per_pass(int k) { return k <= 8 ? 4 : 2; }
constexpr int kSlices = kBlk * kBlk / kThreads;     // accumulate: workgroups per block pair, 4 rows each
constexpr int kListLen = kThreads;      // accumulate: windows scanned per round, one label per thread
constexpr int kInFlight = 8;            // accumulate / inertia: loads issued before the first is added

// upper block pair p of nb blocks per side -> (bi, bj), bi <= bj, row-major over the upper triangle
__device__ __forceinline__ void st_block_pair(int p, int nb, int& bi, int& bj) {
    int i = 0;
    while (p >= nb - i) { p -= nb - i; ++i; }
    bi = i;
    bj = i + p;
}

// ---------------------------------------------------------------------------------------------------- assignment
// Workgroup (block pair p, group g of G): the windows kWin g .. kWin g + kWin - 1, then those kWin G further on, and so on.  Thread (wave, lane) owns
// the entries (row wave + 4 u, column lane), u < 16, of the block; per window and centroid it adds its 16 squared
// differences in ascending u, the wave adds its 64 lanes in wave_sum_d's butterfly, the four waves are added as
// (p0 + p1) + (p2 + p3).  An entry with i >= j or j >= n is loaded from entry (0, 0) instead (always inside the matrix)
// and its term replaced by 0.0 with a select.  The centroid tiles are read again for every kWin windows: they stay in
// L2 (k P 8 bytes in all).  K is a template parameter so that the kWin K accumulators are registers; kWin is 4 up to
// k = 8 and 2 above, where four windows' accumulators would halve the waves a SIMD holds.
template <int K>
__global__ void __launch_bounds__(kThreads) gnm_states_assign_kernel(const double* __restrict__ fc,
                                                                     const double* __restrict__ cen, long long W,
                                                                     int n, int nb, int P,
                                                                     double* __restrict__ partial) {
#pragma clang fp contract(off)
    constexpr int kWin = st_windows_per_pass(K);
    constexpr int kRowsAhead = K <= 4 ? 4 : 2;
    __shared__ double s_red[kWin][K][4];
    int bi, bj;
    st_block_pair(blockIdx.x, nb, bi, bj);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const size_t nn = (size_t)n * n;
    const int i0 = bi * kBlk + wave, j = bj * kBlk + lane;
    for (long long w = (long long)blockIdx.y * kWin; w < W; w += (long long)gridDim.y * kWin) {
        const double* x[kWin];                          // a slot past the last window reads the last one again
#pragma unroll
        for (int q = 0; q < kWin; ++q) x[q] = fc + (size_t)(w + q < W ? w + q : W - 1) * nn;
        double a[kWin][K];
#pragma unroll
        for (int q = 0; q < kWin; ++q)
#pragma unroll
            for (int c = 0; c < K; ++c) a[q][c] = 0.0;
#pragma unroll kRowsAhead
        for (int u = 0; u < kRowsPer; ++u) {            // a few rows' loads in flight, not all sixteen: registers
            const int i = i0 + 4 * u;
            const bool valid = i < j && j < n;
            const size_t off = valid ? (size_t)i * n + j : 0;
            double v[kWin];
#pragma unroll
            for (int q = 0; q < kWin; ++q) v[q] = x[q][off];
#pragma unroll
            for (int c = 0; c < K; ++c) {
                const double m = cen[(size_t)c * nn + off];
#pragma unroll
                for (int q = 0; q < kWin; ++q) {
                    const double d = v[q] - m;
                    const double dd = d * d;
                    a[q][c] += valid ? dd : 0.0;
                }
            }
        }
#pragma unroll
        for (int q = 0; q < kWin; ++q)
#pragma unroll
            for (int c = 0; c < K; ++c) {
                const double r = wave_sum_d(a[q][c]);
                if (lane == 0) s_red[q][c][wave] = r;
            }
        __syncthreads();
        if (tid < kWin * K) {
            const int q = tid / K, c = tid % K;
            const double r = (s_red[q][c][0] + s_red[q][c][1]) + (s_red[q][c][2] + s_red[q][c][3]);
            if (w + q < W) partial[((size_t)(w + q) * P + blockIdx.x) * K + c] = r;
        }
        __syncthreads();                                // s_red is written again in the next round
    }
}

// one thread per window: the block pairs added in ascending order, then the argmin (the first of equal distances)
__global__ void __launch_bounds__(kThreads) gnm_states_argmin_kernel(const double* __restrict__ partial, long long W,
                                                                     int P, int k, double* __restrict__ dist,
                                                                     int* __restrict__ label) {
#pragma clang fp contract(off)
    for (long long w = (long long)blockIdx.x * kThreads + threadIdx.x; w < W; w += (long long)gridDim.x * kThreads) {
        const double* pw = partial + (size_t)w * P * k;
        double best = 0.0;
        int arg = 0;
        bool finite = true;
        for (int c = 0; c < k; ++c) {
            double s = pw[c];
            for (int p = 1; p < P; ++p) s += pw[(size_t)p * k + c];
            dist[(size_t)w * k + c] = s;
            finite = finite && isfinite(s);
            if (c == 0 || s < best) {
                best = s;
                arg = c;
            }
        }
        label[w] = finite ? arg : -1;
    }
}

// ---------------------------------------------------------------------------------------------------- update
// Workgroup (block pair, slice of 4 rows, cluster c): one thread per entry, the running sum in a register from
// sum[c, i, j] at the start to sum[c, i, j] at the end.  The windows are scanned kListLen at a time: each thread reads
// one label, the members of c are compacted in ascending order into s_list (ballot and prefix, no atomics), and every
// thread walks the list with kInFlight loads issued before the first is added, still one after the other.
__global__ void __launch_bounds__(kThreads) gnm_states_accumulate_kernel(const double* __restrict__ fc,
                                                                         const int* __restrict__ label, long long W,
                                                                         int n, int nb, double* __restrict__ sum,
                                                                         long long* __restrict__ count) {
#pragma clang fp contract(off)
    __shared__ long long s_list[kListLen];
    __shared__ int s_cnt[4];
    int bi, bj;
    st_block_pair(blockIdx.x / kSlices, nb, bi, bj);
    const int slice = blockIdx.x % kSlices, c = blockIdx.y;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int i = bi * kBlk + slice * 4 + wave, j = bj * kBlk + lane;
    if (bi * kBlk + slice * 4 >= n) return;             // the whole slice lies below the matrix: uniform
    const bool valid = i <= j && j < n;
    const size_t nn = (size_t)n * n, e = valid ? (size_t)i * n + j : 0;
    double s = valid ? sum[(size_t)c * nn + e] : 0.0;
    long long members = 0;
    for (long long w0 = 0; w0 < W; w0 += kListLen) {
        const long long w = w0 + tid;
        const bool mine = w < W && label[w] == c;
        const unsigned long long votes = __ballot(mine);
        if (lane == 0) s_cnt[wave] = __popcll(votes);
        __syncthreads();
        int before = 0, total = 0;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            before += q < wave ? s_cnt[q] : 0;
            total += s_cnt[q];
        }
        if (mine) s_list[before + __popcll(votes & ((1ull << lane) - 1ull))] = w;
        __syncthreads();
        members += total;
        if (valid) {
            for (int q0 = 0; q0 < total; q0 += kInFlight) {
                double v[kInFlight];
#pragma unroll
                for (int u = 0; u < kInFlight; ++u) {
                    const int q = q0 + u < total ? q0 + u : total - 1;
                    v[u] = fc[(size_t)s_list[q] * nn + e];
                }
#pragma unroll
                for (int u = 0; u < kInFlight; ++u)
                    if (q0 + u < total) s = s + v[u];
            }
        }
        __syncthreads();                                // s_list and s_cnt are written again in the next round
    }
    if (valid) sum[(size_t)c * nn + e] = s;
    if (blockIdx.x == 0 && tid == 0) count[c] += members;
}

// one thread per entry i <= j of every centroid
__global__ void __launch_bounds__(kThreads) gnm_states_finish_kernel(const double* __restrict__ sum,
                                                                     const long long* __restrict__ count, int n,
                                                                     double* __restrict__ cen) {
#pragma clang fp contract(off)
    const int c = blockIdx.y;
    const long long e = (long long)blockIdx.x * kThreads + threadIdx.x;
    const long long nn = (long long)n * n;
    if (e >= nn) return;
    const int i = (int)(e / n), j = (int)(e % n);
    const long long m = count[c];
    if (i > j || m == 0) return;
    const double v = sum[(size_t)c * nn + e] / (double)m;
    cen[(size_t)c * nn + e] = v;
    cen[(size_t)c * nn + (size_t)j * n + i] = v;
}

// one thread: W additions one after the other is the contract; kInFlight loads are issued ahead of them
__global__ void __launch_bounds__(64) gnm_states_inertia_kernel(const double* __restrict__ dist,
                                                                const int* __restrict__ label, long long W, int k,
                                                                double* __restrict__ inertia) {
#pragma clang fp contract(off)
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    double s = 0.0;
    for (long long w0 = 0; w0 < W; w0 += kInFlight) {
        int lab[kInFlight];
        double v[kInFlight];
#pragma unroll
        for (int u = 0; u < kInFlight; ++u) lab[u] = w0 + u < W ? label[w0 + u] : -1;
#pragma unroll
        for (int u = 0; u < kInFlight; ++u) v[u] = lab[u] >= 0 ? dist[(size_t)(w0 + u) * k + lab[u]] : 0.0;
#pragma unroll
        for (int u = 0; u < kInFlight; ++u)
            if (lab[u] >= 0) s = s + v[u];
    }
    inertia[0] = s;
}

int st_check(long long W, int n, int k) {
    if (W < 0 || n < 1 || k < 1) return GNM_ERR_BAD_ARG;
    if (n > kStMaxN || k > kStMaxK) return GNM_ERR_UNSUPPORTED;
    return GNM_OK;
}

int st_pairs(int n) {
    const int nb = (n + kBlk - 1) / kBlk;
    return nb * (nb + 1) / 2;
}

template <int K>
void st_launch_assign(dim3 grid, hipStream_t s, const double* fc, const double* cen, long long W, int n, int nb, int P,
                      double* partial) {
    hipLaunchKernelGGL(gnm_states_assign_kernel<K>, grid, dim3(kThreads), 0, s, fc, cen, W, n, nb, P, partial);
}

}  // namespace

extern "C" int gnm_states_max_k(void) { return kStMaxK; }

// doubles of the workspace gnm_states_assign needs for W windows: one partial per (window, block pair, centroid)
extern "C" long long gnm_states_workspace_doubles(long long W, int n, int k) {
    if (st_check(W, n, k)) return 0;
    return W * st_pairs(n) * k;
}

// dist [W, k] and label [W] of fc [W, n, n] against cen [k, n, n].  groups: workgroups per block pair, each striding
// over the windows (0: as many as the windows need, up to the grid's limit); the result does not depend on it.
extern "C" int gnm_states_assign(const double* fc, const double* cen, long long W, int n, int k, int groups,
                                 double* work, double* dist, int* label, void* stream) {
    if (int e = st_check(W, n, k)) return e;
    if (groups < 0) return GNM_ERR_BAD_ARG;
    if (W == 0) return GNM_OK;
    if (!fc || !cen || !work || !dist || !label) return GNM_ERR_BAD_ARG;
    const int nb = (n + kBlk - 1) / kBlk, P = st_pairs(n);
    const int win = st_windows_per_pass(k);
    const long long want = (W + win - 1) / win, cap = groups > 0 ? (groups < 65535 ? groups : 65535) : 65535;
    const dim3 grid((unsigned)P, (unsigned)(want < cap ? want : cap));
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    switch (k) {
#define GNM_ST_CASE(K) case K: st_launch_assign<K>(grid, s, fc, cen, W, n, nb, P, work); break;
        GNM_ST_CASE(1) GNM_ST_CASE(2) GNM_ST_CASE(3) GNM_ST_CASE(4) GNM_ST_CASE(5) GNM_ST_CASE(6) GNM_ST_CASE(7)
        GNM_ST_CASE(8) GNM_ST_CASE(9) GNM_ST_CASE(10) GNM_ST_CASE(11) GNM_ST_CASE(12) GNM_ST_CASE(13) GNM_ST_CASE(14)
        GNM_ST_CASE(15) GNM_ST_CASE(16)
#undef GNM_ST_CASE
    }
    GNM_CHECK_LAUNCH();
    const long long blocks = (W + kThreads - 1) / kThreads;
    hipLaunchKernelGGL(gnm_states_argmin_kernel, dim3((unsigned)(blocks < (1 << 20) ? blocks : (1 << 20))),
                       dim3(kThreads), 0, s, work, W, P, k, dist, label);
    GNM_CHECK_LAUNCH();
    return GNM_OK;
}

// sum [k, n, n] (entries i <= j) and count [k] (int64) take the windows of fc [W, n, n] in ascending w on top of what
// they hold: zero both before the first chunk of an update.  Labels outside 0 .. k - 1 enter nothing.
extern "C" int gnm_states_accumulate(const double* fc, const int* label, long long W, int n, int k, double* sum,
                                     long long* count, void* stream) {
    if (int e = st_check(W, n, k)) return e;
    if (W == 0) return GNM_OK;
    if (!fc || !label || !sum || !count) return GNM_ERR_BAD_ARG;
    const int nb = (n + kBlk - 1) / kBlk;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(gnm_states_accumulate_kernel, dim3((unsigned)(st_pairs(n) * kSlices), (unsigned)k),
                       dim3(kThreads), 0, s, fc, label, W, n, nb, sum, count);
    GNM_CHECK_LAUNCH();
    return GNM_OK;
}

// cen[c] = sum[c] / count[c] on both triangles from the upper one; count[c] == 0 leaves cen[c] as it is
extern "C" int gnm_states_finish(const double* sum, const long long* count, int n, int k, double* cen, void* stream) {
    if (int e = st_check(0, n, k)) return e;
    if (!sum || !count || !cen) return GNM_ERR_BAD_ARG;
    const long long nn = (long long)n * n;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(gnm_states_finish_kernel, dim3((unsigned)((nn + kThreads - 1) / kThreads), (unsigned)k),
                       dim3(kThreads), 0, s, sum, count, n, cen);
    GNM_CHECK_LAUNCH();
    return GNM_OK;
}

// inertia[0] = sum over the windows with label[w] >= 0 of dist[w, label[w]], added in ascending w
extern "C" int gnm_states_inertia(const double* dist, const int* label, long long W, int k, double* inertia,
                                  void* stream) {
    if (int e = st_check(W, 1, k)) return e;
    if (!inertia || (W > 0 && (!dist || !label))) return GNM_ERR_BAD_ARG;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(gnm_states_inertia_kernel, dim3(1), dim3(64), 0, s, dist, label, W, k, inertia);
    GNM_CHECK_LAUNCH();
    return GNM_OK;
}
