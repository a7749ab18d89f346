// Functional connectivity and mean_bold node features from ROI time series, on the device: the step in front of the
// connectome builder (csrc/connectome.hip).  Per subject s, rows t_off[s] .. t_off[s + 1] of a packed [sum T, n]
// array (fp32 or fp64, time in rows, ROIs in columns, as the reference's DataNodes holds it: dataset.py:45-46):
//
//   gnm_timeseries_means      the fp64 column means, summed in numpy's pairwise order over time (what np.mean computes
//                             for the loader's column-major pandas array), divided by T.
//   gnm_timeseries_zscores    mean_bold (dataset.py:72-78): z = (m - m.mean()) / (m.std() + 1e-8), numpy's pairwise
//                             sums over the n ROIs, fp64 and its fp32 rounding (util.py:118-121).
//   gnm_timeseries_gram       C = (Xc^T Xc) * (1 / (T - 1)) with Xc = X - mean (np.cov, two passes: centred as staged)
//                             on v_mfma_f64_16x16x4_f64, 64 x 64 output blocks of the upper triangle only; writes the
//                             entries i <= j of fc and the diagonal into diag.
//   gnm_timeseries_normalize  R_ij = (C_ij / s_i) / s_j, s = sqrt(diag), for both triangles from the upper one, then
//                             np.clip(R, -1, 1) with NaN kept (np.corrcoef); n = 1 is numpy's c / c.
//
// Sliding windows of the same packed series, described and never copied: window w is the `window` rows from row
// w_beg[w] on (any order, overlapping freely).
//
//   gnm_dynfc_means           the means kernel on (w_beg[w], window) instead of (t_off[s], t_off[s + 1] - t_off[s]).
//   gnm_dynfc_corr            finished R of every window in one launch: the Gram's grid and staging, the standard
//                             deviations from column sums taken while staging, the normalisation from an LDS tile of the
//                             accumulators; rectangular (np.corrcoef) or tapered (np.cov's aweights form).
//
// Every sum has a fixed order inside one workgroup (no atomics, no split of T across workgroups), so a subject's or
// window's results do not depend on the other subjects or windows of the launch.
#include "gnm_common.h"

namespace {

typedef __attribute__((ext_vector_type(4))) double f64x4;

constexpr int kTsMaxN = 4096;           // = gnm_connectome_max_nodes(): the FC goes straight into that builder
constexpr int kMeanThreads = 64;
constexpr int kZThreads = 256;
constexpr int kBlk = 64;                // Gram / normalise output block (64 x 64 entries)
constexpr int kGramThreads = 256;       // 4 waves, a 32 x 32 quadrant each (2 x 2 MFMA tiles of 16 x 16)
constexpr int kKt = 16;                 // time rows per LDS stage
constexpr int kLdsRow = 80;             // doubles per staged row: 640 B, so rows t and t + 1 fall on other banks
constexpr int kStagePer = kKt * kBlk / kGramThreads;   // values of one tile one thread stages (4)

// numpy's pairwise summation (numpy/_core/src/umath/loops_utils.h.src, pairwise_sum) of n values a[0], a[stride], ..:
// below 8 values a plain loop; up to 128 eight accumulators combined as ((r0 + r1) + (r2 + r3)) + ((r4 + r5) +
// (r6 + r7)), then the tail; above that the halves n2 = n / 2 - (n / 2) % 8 and n - n2 summed the same way and added.
template <typename T>
__device__ double np_leaf_sum(const T* a, long long n, long long stride) {
#pragma clang fp contract(off)
    if (n < 8) {
        double r = 0.0;
        for (long long i = 0; i < n; ++i) r += (double)a[i * stride];
        return r;
    }
    double r[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) r[j] = (double)a[j * stride];
    long long i = 8;
    for (; i < n - (n % 8); i += 8) {
#pragma unroll
        for (int j = 0; j < 8; ++j) r[j] += (double)a[(i + j) * stride];
    }
    double res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
    for (; i < n; ++i) res += (double)a[i * stride];
    return res;
}

template <typename T>
__device__ double np_pairwise_sum(const T* a, long long n, long long stride) {
#pragma clang fp contract(off)
    // the recursion unrolled onto a stack: stage 0 = not started, 1 = left half pending, 2 = right half pending
    constexpr int kDepth = 48;                                  // n halves per level: 2^48 values
    long long off[kDepth], len[kDepth];
    double left[kDepth];
    int stage[kDepth];
    int sp = 0;
    off[0] = 0; len[0] = n; stage[0] = 0;
    double r = 0.0;
    for (;;) {
        const long long h = len[sp] / 2 - (len[sp] / 2) % 8;
        if (stage[sp] == 0 && len[sp] > 128) {
            stage[sp] = 1;
            off[sp + 1] = off[sp]; len[sp + 1] = h; stage[sp + 1] = 0;
            ++sp;
            continue;
        }
        if (stage[sp] == 0) {
            r = np_leaf_sum(a + off[sp] * stride, len[sp], stride);
        } else if (stage[sp] == 1) {
            left[sp] = r;
            stage[sp] = 2;
            off[sp + 1] = off[sp] + h; len[sp + 1] = len[sp] - h; stage[sp + 1] = 0;
            ++sp;
            continue;
        } else {
            r = left[sp] + r;
        }
        if (sp == 0) return r;
        --sp;
    }
}

// ---------------------------------------------------------------------------------------------------- means
// one thread per (subject, ROI): the reduce numpy runs is 0 + pairwise_sum(column), then true_divide by T.
// window = 0: subject s owns rows t_off[s] .. t_off[s + 1]; window > 0: `window` rows from t_off[s] on (t_off = w_beg).
template <typename T>
__global__ void __launch_bounds__(kMeanThreads) gnm_ts_means_kernel(const T* __restrict__ x,
                                                                    const int64_t* __restrict__ t_off, int window,
                                                                    int n, int bps, double* __restrict__ mean) {
#pragma clang fp contract(off)
    const int s = blockIdx.x / bps;
    const int c = (blockIdx.x % bps) * kMeanThreads + threadIdx.x;
    if (c >= n) return;
    const long long t0 = t_off[s], T_s = window > 0 ? (long long)window : t_off[s + 1] - t0;
    const double sum = 0.0 + np_pairwise_sum(x + t0 * n + c, T_s, (long long)n);
    mean[(size_t)s * n + c] = sum / (double)T_s;
}

// ---------------------------------------------------------------------------------------------------- z-scores
// numpy's _mean / _var of the n column means (numpy/_core/_methods.py): mu = sum(m) / n; var = sum((m - mu)^2) / n;
// z = (m - mu) / (sqrt(var) + 1e-8).  The two pairwise sums are one thread's (n <= 4096); the rest is elementwise.
__global__ void __launch_bounds__(kZThreads) gnm_ts_zscore_kernel(const double* __restrict__ mean, int n,
                                                                  double* __restrict__ z64, float* __restrict__ z32) {
#pragma clang fp contract(off)
    __shared__ double s_v[kTsMaxN];             // the means, then their squared deviations
    __shared__ double s_mu, s_sd;
    const int s = blockIdx.x, t = threadIdx.x;
    const double* m = mean + (size_t)s * n;
    for (int i = t; i < n; i += kZThreads) s_v[i] = m[i];
    __syncthreads();
    if (t == 0) s_mu = (0.0 + np_pairwise_sum(s_v, n, 1)) / (double)n;
    __syncthreads();
    const double mu = s_mu;
    for (int i = t; i < n; i += kZThreads) {
        const double d = s_v[i] - mu;
        s_v[i] = d * d;
    }
    __syncthreads();
    if (t == 0) s_sd = sqrt((0.0 + np_pairwise_sum(s_v, n, 1)) / (double)n);
    __syncthreads();
    const double den = s_sd + 1e-8;
    for (int i = t; i < n; i += kZThreads) {
        const double z = (m[i] - mu) / den;
        if (z64) z64[(size_t)s * n + i] = z;
        if (z32) z32[(size_t)s * n + i] = (float)z;
    }
}

// upper block pair p of nb blocks per side -> (bi, bj), bi <= bj, row-major over the upper triangle
__device__ __forceinline__ void ts_block_pair(int p, int nb, int& bi, int& bj) {
    int i = 0;
    while (p >= nb - i) { p -= nb - i; ++i; }
    bi = i;
    bj = i + p;
}

// ---------------------------------------------------------------------------------------------------- Gram
// Workgroup (subject s, block pair bi <= bj): G = Xc[:, bi block]^T Xc[:, bj block] over the subject's T rows.  Time
// rows stream through two LDS stages of kKt rows: each stage holds the bi and bj column blocks of those rows, centred
// as they are staged (x - mean, numpy's X -= avg); rows past T and columns past n are staged as exact zeros, so
// padding adds nothing.  The next stage's values are loaded into registers while the MFMAs read the current one.
// MFMA operand maps (v_mfma_f64_16x16x4_f64): lane l holds A[row l & 15][k = l >> 4] and B[k = l >> 4][col l & 15];
// result register r of lane l is row (l >> 4) + 4 r, column l & 15.
template <typename T>
__global__ void __launch_bounds__(kGramThreads) gnm_ts_gram_kernel(const T* __restrict__ x,
                                                                   const int64_t* __restrict__ t_off,
                                                                   const double* __restrict__ mean, int n, int nb,
                                                                   int P, double* __restrict__ fc,
                                                                   double* __restrict__ diag) {
    __shared__ double s_a[2][kKt][kLdsRow], s_b[2][kKt][kLdsRow];
    const int s = blockIdx.x / P;
    int bi, bj;
    ts_block_pair(blockIdx.x % P, nb, bi, bj);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long t0 = t_off[s], T_s = t_off[s + 1] - t0;
    const T* xs = x + t0 * n;
    // staging: thread tid stages column (tid & 63) of rows (tid >> 6) + 4 u, u < kStagePer, of both blocks
    const int sc = lane, sr = wave;
    const int ca = bi * kBlk + sc, cb = bj * kBlk + sc;
    const bool va = ca < n, vb = cb < n;
    const double ma = va ? mean[(size_t)s * n + ca] : 0.0;
    const double mb = vb ? mean[(size_t)s * n + cb] : 0.0;
    double ra[kStagePer], rb[kStagePer];
    auto load = [&](long long k0) {
#pragma unroll
        for (int u = 0; u < kStagePer; ++u) {
            const long long t = k0 + sr + 4 * u;
            const bool in = t < T_s;
            ra[u] = (in && va) ? (double)xs[t * n + ca] - ma : 0.0;
            rb[u] = (in && vb) ? (double)xs[t * n + cb] - mb : 0.0;
        }
    };
    auto store = [&](int buf) {
#pragma unroll
        for (int u = 0; u < kStagePer; ++u) {
            s_a[buf][sr + 4 * u][sc] = ra[u];
            s_b[buf][sr + 4 * u][sc] = rb[u];
        }
    };
    // wave w owns rows 32 (w >> 1) .., columns 32 (w & 1) .. of the block; a diagonal block's strictly lower
    // quadrant is never read (normalise reads i <= j), so that wave only stages
    const int wr = wave >> 1, wc = wave & 1;
    const bool busy = !(bi == bj && wr > wc);
    f64x4 acc[2][2];
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
        for (int c = 0; c < 2; ++c) acc[r][c] = f64x4{0.0, 0.0, 0.0, 0.0};
    const long long nk = (T_s + kKt - 1) / kKt;
    load(0);
    store(0);
    __syncthreads();
    const int fr = lane & 15, fk = lane >> 4;
    for (long long kc = 0; kc < nk; ++kc) {
        const int buf = (int)(kc & 1);
        if (kc + 1 < nk) load((kc + 1) * kKt);
        if (busy) {
#pragma unroll
            for (int kk = 0; kk < kKt / 4; ++kk) {
                const int k = 4 * kk + fk;
                double a[2], b[2];
#pragma unroll
                for (int r = 0; r < 2; ++r) a[r] = s_a[buf][k][32 * wr + 16 * r + fr];
#pragma unroll
                for (int c = 0; c < 2; ++c) b[c] = s_b[buf][k][32 * wc + 16 * c + fr];
#pragma unroll
                for (int r = 0; r < 2; ++r)
#pragma unroll
                    for (int c = 0; c < 2; ++c)
                        acc[r][c] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[r], b[c], acc[r][c], 0, 0, 0);
            }
        }
        if (kc + 1 < nk) store(buf ^ 1);
        __syncthreads();
    }
    if (!busy) return;
    // np.cov: c *= np.true_divide(1, T - 1); T = 1 gives 1 / 0 = inf and 0 * inf = NaN, as in numpy
    const double inv = 1.0 / (double)(T_s - 1);
    double* out = fc + (size_t)s * n * n;
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
        for (int c = 0; c < 2; ++c)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int i = bi * kBlk + 32 * wr + 16 * r + fk + 4 * q;
                const int j = bj * kBlk + 32 * wc + 16 * c + fr;
                if (i < n && j < n && i <= j) {
                    const double v = acc[r][c][q] * inv;
                    out[(size_t)i * n + j] = v;
                    if (i == j) diag[(size_t)s * n + i] = v;
                }
            }
}

// ---------------------------------------------------------------------------------------------------- normalise
// Workgroup (subject s, block pair bi <= bj): reads the C entries i <= j of the pair into LDS, then writes R of the
// upper block (bi, bj) and of its mirror (bj, bi) from them: R_ij = (C_ij / s_i) / s_j and R_ji = (C_ij / s_j) / s_i,
// numpy's c /= stddev[:, None]; c /= stddev[None, :] with C exactly symmetric.  The clip keeps NaN (np.clip), where
// fmin / fmax would return a number.  Only this workgroup reads or writes its two blocks.
__device__ __forceinline__ double ts_clip(double r) { return r < -1.0 ? -1.0 : (r > 1.0 ? 1.0 : r); }

__global__ void __launch_bounds__(kGramThreads) gnm_ts_normalize_kernel(const double* __restrict__ diag, int n,
                                                                        int nb, int P, double* __restrict__ fc) {
    __shared__ double s_c[kBlk][kBlk + 1];
    __shared__ double s_si[kBlk], s_sj[kBlk];
    const int s = blockIdx.x / P;
    int bi, bj;
    ts_block_pair(blockIdx.x % P, nb, bi, bj);
    const int tid = threadIdx.x;
    double* m = fc + (size_t)s * n * n;
    const double* d = diag + (size_t)s * n;
    const int i0 = bi * kBlk, j0 = bj * kBlk;
    if (n == 1) {                                   // np.corrcoef of one ROI: cov is a scalar, returned as c / c
        if (tid == 0) m[0] = m[0] / m[0];
        return;
    }
    if (tid < kBlk) {
        s_si[tid] = i0 + tid < n ? sqrt(d[i0 + tid]) : 0.0;
        s_sj[tid] = j0 + tid < n ? sqrt(d[j0 + tid]) : 0.0;
    }
    for (int e = tid; e < kBlk * kBlk; e += kGramThreads) {
        const int r = e >> 6, c = e & 63, i = i0 + r, j = j0 + c;
        s_c[r][c] = (i < n && j < n && i <= j) ? m[(size_t)i * n + j] : 0.0;
    }
    __syncthreads();
    // upper block: row i = i0 + r, column j = j0 + c (a diagonal block reads C_ji below its diagonal)
    for (int e = tid; e < kBlk * kBlk; e += kGramThreads) {
        const int r = e >> 6, c = e & 63, i = i0 + r, j = j0 + c;
        if (i >= n || j >= n) continue;
        const double cij = (i <= j) ? s_c[r][c] : s_c[c][r];
        m[(size_t)i * n + j] = ts_clip((cij / s_si[r]) / s_sj[c]);
    }
    if (bi == bj) return;
    // mirror block: row j = j0 + r, column i = i0 + c: R_ji = (C_ij / s_j) / s_i
    for (int e = tid; e < kBlk * kBlk; e += kGramThreads) {
        const int r = e >> 6, c = e & 63, j = j0 + r, i = i0 + c;
        if (i >= n || j >= n) continue;
        m[(size_t)j * n + i] = ts_clip((s_c[c][r] / s_sj[r]) / s_si[c]);
    }
}

// ---------------------------------------------------------------------------------------------------- windows
// Workgroup (window w, block pair bi <= bj): the Gram kernel's grid, staging and MFMA loop over the window's rows, and
// the normalise kernel's epilogue from an LDS tile of the accumulators instead of a C read back from memory, so each R
// entry is written once and nothing else is.
//   * rectangular (kTaper false, np.corrcoef): centre = mean[w] (the means kernel's), C = (Xc^T Xc) * (1 / (window - 1)).
//   * tapered (kTaper true, np.cov's aweights): centre avg = sum_t w_t x_t / sum_t w_t, C = (Xc^T (w * Xc)) * (1 / fact),
//     fact = sum w - sum w^2 / sum w; the B side is staged as w_t * xc.  Thread (column, wave) sums the rows
//     t = wave, wave + 4, .. in ascending t and the four waves' parts are added as (p0 + p1) + (p2 + p3).
//   * s_i = sqrt(C_ii) of the workgroup's two column blocks: column sums of xc * (w * xc) taken while staging, in the
//     same per-wave order and the same combine, times the same reciprocal.  The order depends on the column and the
//     window alone, so every workgroup that serves a column gets the same bits, on the A side or the B side.
//   * rows past the window and columns past n are staged as exact zeros by select; a value outside the window is
//     never part of a product.
// The tile s_c and the small sums alias the staging buffers: the K loop ends on a barrier, after which no wave reads
// them.
template <typename T, bool kTaper>
__global__ void __launch_bounds__(kGramThreads) gnm_dynfc_corr_kernel(const T* __restrict__ x,
                                                                      const int64_t* __restrict__ w_beg, int window,
                                                                      const double* __restrict__ mean,
                                                                      const double* __restrict__ taper, int n, int nb,
                                                                      int P, double* __restrict__ fc) {
#pragma clang fp contract(off)
    constexpr int kSide = 2 * kKt * kLdsRow;            // doubles of one side's two stages
    constexpr int kTile = kBlk * (kBlk + 1);            // doubles of the accumulator tile
    static_assert(2 * kSide >= kTile + 2 * 4 * kBlk + 2 * kBlk + 2 * 4, "tile and sums must fit the staging buffers");
    // one 40 KiB buffer, four workgroups to a CU: the two sides' stages during the K loop; before it (taper) and after
    // it the tile in front and the small sums behind it, each use fenced from the next by a barrier
    __shared__ double s_raw[2 * kSide];
    double (*s_a)[kKt][kLdsRow] = reinterpret_cast<double (*)[kKt][kLdsRow]>(s_raw);
    double (*s_b)[kKt][kLdsRow] = reinterpret_cast<double (*)[kKt][kLdsRow]>(s_raw + kSide);
    double (*s_c)[kBlk + 1] = reinterpret_cast<double (*)[kBlk + 1]>(s_raw);
    double (*s_part)[4][kBlk] = reinterpret_cast<double (*)[4][kBlk]>(s_raw + kTile);   // per-wave parts, column sums
    double* s_si = s_raw + kTile + 2 * 4 * kBlk;
    double* s_sj = s_si + kBlk;
    double (*s_wpart)[4] = reinterpret_cast<double (*)[4]>(s_sj + kBlk);                // parts of sum w and sum w^2
    const int w = blockIdx.x / P;
    int bi, bj;
    ts_block_pair(blockIdx.x % P, nb, bi, bj);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const T* xs = x + (long long)w_beg[w] * n;
    // staging: thread tid stages column (tid & 63) of rows (tid >> 6) + 4 u, u < kStagePer, of both blocks
    const int sc = lane, sr = wave;
    const int ca = bi * kBlk + sc, cb = bj * kBlk + sc;
    const bool va = ca < n, vb = cb < n;
    const int ka = va ? ca : 0, kb = vb ? cb : 0;       // a column that exists, for loads whose value is not used
    double ma, mb, inv;
    if constexpr (kTaper) {
        double pa = 0.0, pb = 0.0, q1 = 0.0, q2 = 0.0;
        for (int t0 = sr; t0 < window; t0 += 4 * kStagePer) {      // kStagePer rows in flight, added in ascending t
            T ga[kStagePer], gb[kStagePer];
            double gw[kStagePer];
#pragma unroll
            for (int u = 0; u < kStagePer; ++u) {
                const int tt = t0 + 4 * u < window ? t0 + 4 * u : 0;
                ga[u] = xs[(long long)tt * n + ka];
                gb[u] = xs[(long long)tt * n + kb];
                gw[u] = taper[tt];
            }
#pragma unroll
            for (int u = 0; u < kStagePer; ++u) {
                if (t0 + 4 * u >= window) break;
                const double wt = gw[u];
                if (va) pa += wt * (double)ga[u];
                if (vb) pb += wt * (double)gb[u];
                q1 += wt;
                q2 += wt * wt;
            }
        }
        s_part[0][sr][sc] = pa;
        s_part[1][sr][sc] = pb;
        if (sc == 0) {
            s_wpart[0][sr] = q1;
            s_wpart[1][sr] = q2;
        }
        __syncthreads();
        const double sw = (s_wpart[0][0] + s_wpart[0][1]) + (s_wpart[0][2] + s_wpart[0][3]);
        const double sw2 = (s_wpart[1][0] + s_wpart[1][1]) + (s_wpart[1][2] + s_wpart[1][3]);
        ma = ((s_part[0][0][sc] + s_part[0][1][sc]) + (s_part[0][2][sc] + s_part[0][3][sc])) / sw;
        mb = ((s_part[1][0][sc] + s_part[1][1][sc]) + (s_part[1][2][sc] + s_part[1][3][sc])) / sw;
        inv = 1.0 / (sw - sw2 / sw);
        __syncthreads();                                // s_part is written again below
    } else {
        ma = va ? mean[(size_t)w * n + ca] : 0.0;
        mb = vb ? mean[(size_t)w * n + cb] : 0.0;
        inv = 1.0 / (double)(window - 1);               // np.cov: c *= np.true_divide(1, T - 1)
    }
    // Global loads are fetched raw, kDepth stages ahead and from an address that is always inside the window (row 0 or
    // column 0 of it where the thread's own lies outside), so nothing waits on them until stage() centres, weights and
    // stores them: a 50-row window has all its rows in flight at once instead of one round trip per stage.
    constexpr int kDepth = kTaper ? 2 : 4;              // the taper's weights and products leave registers for two
    T ga[kDepth][kStagePer], gb[kDepth][kStagePer];
    double da = 0.0, db = 0.0;                          // this thread's rows of sum_t xc * (w * xc), columns ca and cb
    auto fetch = [&](int slot, int k0) {
#pragma unroll
        for (int u = 0; u < kStagePer; ++u) {
            const int t = k0 + sr + 4 * u;
            const int tt = t < window ? t : 0;
            ga[slot][u] = xs[(long long)tt * n + ka];
            gb[slot][u] = xs[(long long)tt * n + kb];
        }
    };
    auto stage = [&](int slot, int buf, int k0) {
#pragma unroll
        for (int u = 0; u < kStagePer; ++u) {
            const int t = k0 + sr + 4 * u;
            const bool in = t < window;
            const double xa = (in && va) ? (double)ga[slot][u] - ma : 0.0;
            const double xb = (in && vb) ? (double)gb[slot][u] - mb : 0.0;
            double wa = xa, wb = xb;
            if constexpr (kTaper) {
                const double wt = in ? taper[t] : 0.0;
                wa = wt * xa;
                wb = wt * xb;
            }
            da += xa * wa;
            db += xb * wb;
            s_a[buf][sr + 4 * u][sc] = xa;
            s_b[buf][sr + 4 * u][sc] = wb;
        }
    };
    // wave w owns rows 32 (w >> 1) .., columns 32 (w & 1) .. of the block; a diagonal block's strictly lower
    // quadrant is never read (the epilogue reads i <= j), so that wave only stages
    const int wr = wave >> 1, wc = wave & 1;
    const bool busy = !(bi == bj && wr > wc);
    f64x4 acc[2][2];
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
        for (int c = 0; c < 2; ++c) acc[r][c] = f64x4{0.0, 0.0, 0.0, 0.0};
    const int nk = (window + kKt - 1) / kKt;
#pragma unroll
    for (int j = 0; j < kDepth; ++j)
        if (j < nk) fetch(j, j * kKt);
    stage(0, 0, 0);
    __syncthreads();
    const int fr = lane & 15, fk = lane >> 4;
    for (int kc0 = 0; kc0 < nk; kc0 += kDepth) {
#pragma unroll
        for (int j = 0; j < kDepth; ++j) {              // stage kc lives in slot kc % kDepth = j and buffer kc & 1
            const int kc = kc0 + j;
            if (kc >= nk) break;
            const int buf = j & 1;
            if (kc + kDepth < nk) fetch(j, (kc + kDepth) * kKt);        // slot j was staged an iteration ago
            if (busy) {
#pragma unroll
                for (int kk = 0; kk < kKt / 4; ++kk) {
                    if (kc * kKt + 4 * kk >= window) break;     // the last stage's all-zero row quads: windows are short
                    const int k = 4 * kk + fk;
                    double a[2], b[2];
#pragma unroll
                    for (int r = 0; r < 2; ++r) a[r] = s_a[buf][k][32 * wr + 16 * r + fr];
#pragma unroll
                    for (int c = 0; c < 2; ++c) b[c] = s_b[buf][k][32 * wc + 16 * c + fr];
#pragma unroll
                    for (int r = 0; r < 2; ++r)
#pragma unroll
                        for (int c = 0; c < 2; ++c)
                            acc[r][c] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[r], b[c], acc[r][c], 0, 0, 0);
                }
            }
            if (kc + 1 < nk) stage((j + 1) % kDepth, buf ^ 1, (kc + 1) * kKt);
            __syncthreads();
        }
    }
    // C of the block into the tile (row = block row, column = block column), the column sums into s_part
    s_part[0][sr][sc] = da;
    s_part[1][sr][sc] = db;
    if (busy) {
#pragma unroll
        for (int r = 0; r < 2; ++r)
#pragma unroll
            for (int c = 0; c < 2; ++c)
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    s_c[32 * wr + 16 * r + fk + 4 * q][32 * wc + 16 * c + fr] = acc[r][c][q] * inv;
    }
    __syncthreads();
    double* m = fc + (size_t)w * n * n;
    if (n == 1) {                                       // np.corrcoef of one ROI: cov is a scalar, returned as c / c
        if (tid == 0) m[0] = s_c[0][0] / s_c[0][0];
        return;
    }
    if (tid < 2 * kBlk) {
        const int side = tid >> 6, c = tid & 63;
        const double sum = (s_part[side][0][c] + s_part[side][1][c]) + (s_part[side][2][c] + s_part[side][3][c]);
        (side ? s_sj : s_si)[c] = sqrt(sum * inv);
    }
    __syncthreads();
    const int i0 = bi * kBlk, j0 = bj * kBlk;
    // upper block: row i = i0 + r, column j = j0 + c (a diagonal block reads C_ji below its diagonal)
#pragma unroll 4
    for (int e = tid; e < kBlk * kBlk; e += kGramThreads) {
        const int r = e >> 6, c = e & 63, i = i0 + r, j = j0 + c;
        if (i >= n || j >= n) continue;
        const double cij = (i <= j) ? s_c[r][c] : s_c[c][r];
        m[(size_t)i * n + j] = ts_clip((cij / s_si[r]) / s_sj[c]);
    }
    if (bi == bj) return;
    // mirror block: row j = j0 + r, column i = i0 + c: R_ji = (C_ij / s_j) / s_i
#pragma unroll 4
    for (int e = tid; e < kBlk * kBlk; e += kGramThreads) {
        const int r = e >> 6, c = e & 63, j = j0 + r, i = i0 + c;
        if (i >= n || j >= n) continue;
        m[(size_t)j * n + i] = ts_clip((s_c[c][r] / s_sj[r]) / s_si[c]);
    }
}

int ts_check(int S, int n) {
    if (S < 0 || n < 1) return GNM_ERR_BAD_ARG;
    if (n > kTsMaxN) return GNM_ERR_UNSUPPORTED;
    return GNM_OK;
}

// block pairs per subject, and the grid S * P must stay within one dimension's launch limit
long long ts_pairs(int n) {
    const long long nb = (n + kBlk - 1) / kBlk;
    return nb * (nb + 1) / 2;
}

}  // namespace

extern "C" int gnm_timeseries_max_nodes(void) { return kTsMaxN; }

// numpy's column means of each subject's rows t_off[s] .. t_off[s + 1] (T_s >= 1, checked by the caller)
extern "C" int gnm_timeseries_means(const void* x, int x_f64, const int64_t* t_off, int S, int n, double* mean,
                                    void* stream) {
    if (int e = ts_check(S, n)) return e;
    if (S == 0) return GNM_OK;
    if (!x || !t_off || !mean) return GNM_ERR_BAD_ARG;
    const int bps = (n + kMeanThreads - 1) / kMeanThreads;
    if ((long long)S * bps > 0x7fffffffLL / kMeanThreads) return GNM_ERR_UNSUPPORTED;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (x_f64)
        hipLaunchKernelGGL(gnm_ts_means_kernel<double>, dim3(S * bps), dim3(kMeanThreads), 0, s,
                           static_cast<const double*>(x), t_off, 0, n, bps, mean);
    else
        hipLaunchKernelGGL(gnm_ts_means_kernel<float>, dim3(S * bps), dim3(kMeanThreads), 0, s,
                           static_cast<const float*>(x), t_off, 0, n, bps, mean);
    GNM_CHECK_LAUNCH();
    return GNM_OK;
}

// the most windows one gnm_dynfc_corr launch takes at n ROIs (0 for an unsupported n): the caller splits above it
extern "C" long long gnm_dynfc_max_windows(int n) {
    if (n < 1 || n > kTsMaxN) return 0;
    return (0x7fffffffLL / kGramThreads) / ts_pairs(n);
}

// the same column means for window w = rows w_beg[w] .. w_beg[w] + window: bitwise gnm_timeseries_means of those rows
extern "C" int gnm_dynfc_means(const void* x, int x_f64, const int64_t* w_beg, int window, int W, int n, double* mean,
                               void* stream) {
    if (int e = ts_check(W, n)) return e;
    if (window < 2) return GNM_ERR_BAD_ARG;
    if (W == 0) return GNM_OK;
    if (!x || !w_beg || !mean) return GNM_ERR_BAD_ARG;
    const int bps = (n + kMeanThreads - 1) / kMeanThreads;
    if ((long long)W * bps > 0x7fffffffLL / kMeanThreads) return GNM_ERR_UNSUPPORTED;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (x_f64)
        hipLaunchKernelGGL(gnm_ts_means_kernel<double>, dim3(W * bps), dim3(kMeanThreads), 0, s,
                           static_cast<const double*>(x), w_beg, window, n, bps, mean);
    else
        hipLaunchKernelGGL(gnm_ts_means_kernel<float>, dim3(W * bps), dim3(kMeanThreads), 0, s,
                           static_cast<const float*>(x), w_beg, window, n, bps, mean);
    GNM_CHECK_LAUNCH();
    return GNM_OK;
}

// finished R of every window, one launch: taper NULL is np.corrcoef of the window's rows (mean: gnm_dynfc_means'),
// taper [window] is the aweights form (mean is not read)
extern "C" int gnm_dynfc_corr(const void* x, int x_f64, const int64_t* w_beg, int window, const double* mean,
                              const double* taper, int W, int n, double* fc, void* stream) {
    if (int e = ts_check(W, n)) return e;
    if (window < 2) return GNM_ERR_BAD_ARG;
    if (W == 0) return GNM_OK;
    if (!x || !w_beg || !fc || (!mean && !taper)) return GNM_ERR_BAD_ARG;
    const long long P = ts_pairs(n);
    if ((long long)W * P > 0x7fffffffLL / kGramThreads) return GNM_ERR_UNSUPPORTED;
    const int nb = (n + kBlk - 1) / kBlk;
    const dim3 grid((unsigned)(W * P)), block(kGramThreads);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (x_f64 && taper)
        hipLaunchKernelGGL((gnm_dynfc_corr_kernel<double, true>), grid, block, 0, s, static_cast<const double*>(x),
                           w_beg, window, mean, taper, n, nb, (int)P, fc);
    else if (x_f64)
        hipLaunchKernelGGL((gnm_dynfc_corr_kernel<double, false>), grid, block, 0, s, static_cast<const double*>(x),
                           w_beg, window, mean, taper, n, nb, (int)P, fc);
    else if (taper)
        hipLaunchKernelGGL((gnm_dynfc_corr_kernel<float, true>), grid, block, 0, s, static_cast<const float*>(x),
                           w_beg, window, mean, taper, n, nb, (int)P, fc);
    else
        hipLaunchKernelGGL((gnm_dynfc_corr_kernel<float, false>), grid, block, 0, s, static_cast<const float*>(x),
                           w_beg, window, mean, taper, n, nb, (int)P, fc);
    GNM_CHECK_LAUNCH();
    return GNM_OK;
}

// dataset.py:73-74 on the means: fp64 z-scores into z64 and their fp32 rounding into z32 (either may be NULL)
extern "C" int gnm_timeseries_zscores(const double* mean, int S, int n, double* z64, float* z32, void* stream) {
    if (int e = ts_check(S, n)) return e;
    if (S == 0) return GNM_OK;
    if (!mean || (!z64 && !z32)) return GNM_ERR_BAD_ARG;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(gnm_ts_zscore_kernel, dim3(S), dim3(kZThreads), 0, s, mean, n, z64, z32);
    GNM_CHECK_LAUNCH();
    return GNM_OK;
}

// np.cov's (Xc^T Xc) * (1 / (T - 1)): the entries i <= j of fc[s] and the diagonal into diag[s]
extern "C" int gnm_timeseries_gram(const void* x, int x_f64, const int64_t* t_off, const double* mean, int S, int n,
                                   double* fc, double* diag, void* stream) {
    if (int e = ts_check(S, n)) return e;
    if (S == 0) return GNM_OK;
    if (!x || !t_off || !mean || !fc || !diag) return GNM_ERR_BAD_ARG;
    const long long P = ts_pairs(n);
    if ((long long)S * P > 0x7fffffffLL / kGramThreads) return GNM_ERR_UNSUPPORTED;
    const int nb = (n + kBlk - 1) / kBlk;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (x_f64)
        hipLaunchKernelGGL(gnm_ts_gram_kernel<double>, dim3((unsigned)(S * P)), dim3(kGramThreads), 0, s,
                           static_cast<const double*>(x), t_off, mean, n, nb, (int)P, fc, diag);
    else
        hipLaunchKernelGGL(gnm_ts_gram_kernel<float>, dim3((unsigned)(S * P)), dim3(kGramThreads), 0, s,
                           static_cast<const float*>(x), t_off, mean, n, nb, (int)P, fc, diag);
    GNM_CHECK_LAUNCH();
    return GNM_OK;
}

// np.corrcoef's normalisation and clip, in place on the Gram's output
extern "C" int gnm_timeseries_normalize(const double* diag, int S, int n, double* fc, void* stream) {
    if (int e = ts_check(S, n)) return e;
    if (S == 0) return GNM_OK;
    if (!diag || !fc) return GNM_ERR_BAD_ARG;
    const long long P = ts_pairs(n);
    if ((long long)S * P > 0x7fffffffLL / kGramThreads) return GNM_ERR_UNSUPPORTED;
    const int nb = (n + kBlk - 1) / kBlk;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(gnm_ts_normalize_kernel, dim3((unsigned)(S * P)), dim3(kGramThreads), 0, s, diag, n, nb, (int)P,
                       fc);
    GNM_CHECK_LAUNCH();
    return GNM_OK;
}
