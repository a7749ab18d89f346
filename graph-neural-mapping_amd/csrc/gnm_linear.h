// What the three units of the Linear family share: linear.hip (forward and dX = dZ W), linear_wgrad.hip (weight
// gradient and the partial reductions) and linear_bwd.hip (fused BatchNorm backward + dgrad + wgrad).  The knobs, the
// tile walk, the tuning stamps, the weight-plane staging and split dgrad, the tile descriptor and the one summation
// order of the partial reductions.
#pragma once
#include "gnm_split.h"

// tuning knobs, read once per process and unit
static inline bool lin_force_generic() { static const bool v = getenv("GNM_LIN_GENERIC") != nullptr; return v; }
static inline bool lin_no_stream() { static const bool v = getenv("GNM_LIN_NO_STREAM") != nullptr; return v; }   // tuning: A/B
static inline bool lin_no_split() {
    static const bool v = gnm_env_int("GNM_LIN_NO_SPLIT", 0) != 0;     // A/B knob: keep the fp32 matrix instruction
    return v;
}

// First tile of a wave in the strided tile walk (stride = all active waves of the launch).  Numbering the waves
// workgroup by workgroup hands the remainder tiles (ntiles mod stride) to the FIRST workgroups only -- at the headline
// shape 12,800 tiles over 3,072 waves: five tiles for every wave of workgroups 0-42 and four for the rest, and the
// launch lasts as long as those 43 CUs need for 60 tiles while the other 213 have 48.  Numbered slot-major instead
// (one wave of every group of every workgroup first, on different SIMDs, then the next ...) every CU gets 50.
// `groups` groups of four waves per workgroup, `rows` groups in the launch; a launch whose last workgroup is not full
// (rows != groups * gridDim.x: small N) keeps the plain numbering, and waves past the last row get no tile.
__host__ __device__ __forceinline__ int lin_first_tile_of(int wave, int groups, int rows, int nwg, int b) {
    const int grp = wave >> 2;
    if (rows == groups * nwg) {
        const int slot = ((wave & 3) + grp * (groups == 2 ? 2 : 1)) & 3;
        return (slot * groups + grp) * nwg + b;
    }
    const int gw = b * groups * 4 + wave;
    return gw < 4 * rows ? gw : 0x3fffffff;
}
__device__ __forceinline__ int lin_first_tile(int wave, int groups, int rows) {
    return lin_first_tile_of(wave, groups, rows, (int)gridDim.x, (int)blockIdx.x);
}

#ifdef GNM_LIN_TUNING
extern __attribute__((visibility("hidden"))) unsigned long long* g_lin_stamps;   // linear.hip, gnm_debug_set_lin_stamps
#define GNM_LSTAMP(k)                                                                                         \
    if (p.stamps && (threadIdx.x & 63) == 0)                                                                  \
        p.stamps[((size_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * 64 + (k)] = __builtin_amdgcn_s_memtime();
#define GNM_RSTAMP(k)      /* gnm_linear_bwd_rz_kernel: eight waves per workgroup */                        \
    if (p.stamps && (threadIdx.x & 63) == 0)                                                                  \
        p.stamps[((size_t)blockIdx.x * 8 + (threadIdx.x >> 6)) * 64 + (k)] = __builtin_amdgcn_s_memtime();
#define GNM_SSTAMP(k)      /* gnm_lin_split_kernel: twelve waves per workgroup, six stamps per tile */        \
    if (p.stamps && (threadIdx.x & 63) == 0)                                                                  \
        p.stamps[((size_t)blockIdx.x * kSplitWaves + (threadIdx.x >> 6)) * 64 + (k)] = __builtin_amdgcn_s_memtime();
#else
static unsigned long long* const g_lin_stamps = nullptr;
#define GNM_LSTAMP(k)
#define GNM_RSTAMP(k)
#define GNM_SSTAMP(k)
#endif

// W -> its three bf16 plane images in LDS (plane stride ew entries), for the six-term product with a 32-row tile whose
// lanes hold k = KGS kg + 8 m + 0..7.  Entry (m, c, lane = 32 kg + n) is the eight contraction indices
// kk = 8 m + KGS kg + 0..7 of output column nn = 32 c + n (CT column tiles): W[kk][nn] in the k-major form (dgrad: the
// contraction runs over W's rows), W[nn][kk] in the forward form.  CLIP: W's columns at or past wcols read as zero.
template <int CT, int KGS, bool KMAJOR, bool CLIP>
__device__ __forceinline__ void lin_stage_planes(gnm_u32x4* Wp, int ew, const float* W, int ldw, int wcols, int tid, int nt) {
    for (int e = tid; e < ew; e += nt) {
        const int n = e & 31, kg = (e >> 5) & 1, c = (e >> 6) % CT, m = e / (64 * CT);
        const int kk = 8 * m + KGS * kg, nn = 32 * c + n;
        float f[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            if (KMAJOR) f[j] = (!CLIP || nn < wcols) ? W[(size_t)(kk + j) * ldw + nn] : 0.f;
            else f[j] = (!CLIP || kk + j < wcols) ? W[(size_t)nn * ldw + kk + j] : 0.f;
        }
        gnm_u32x4 p1, p2, p3;
        gnm_split8(f, p1, p2, p3);
        Wp[e] = p1; Wp[ew + e] = p2; Wp[2 * ew + e] = p3;
    }
}

// dacc += dZ W on the bf16 pipe for H = 64: lane (i, h) takes row i, k = 32 h + 8 m + 0..7 of the wave's dZ image Xs (row
// stride xs floats) and multiplies by the k-major plane image Wp of lin_stage_planes.  (The caller zeroes dacc: with
// the zeroing in here the narrow fused kernel's tile loop came out scheduled differently.)
template <int KT, int HP>
__device__ __forceinline__ void lin_dgrad_split(f32x16 (&dacc)[KT], const float* Xs, int xs, const gnm_u32x4* Wp, int i, int h,
                                                int lane) {
    static_assert(HP == 64, "four steps of 16 over H = 64: a lane half starts at k = 32 h");
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        gnm_bf16x8 x1, x2, x3;
        gnm_load_split8(Xs + i * xs + 32 * h + 8 * m, x1, x2, x3);
#pragma unroll
        for (int c = 0; c < KT; ++c) gnm_mma6_planes(dacc[c], x1, x2, x3, Wp, 4 * KT * 64, (m * KT + c) * 64 + lane);
    }
}

// The buffer descriptor of a tile's valid rows: `rows` rows of `width` floats at leading dimension ld from `base`.
// Rows past N, and whole tiles past the last, are dropped by the address check, so every access of a tile is issued
// unconditionally (gnm_lin_stream_kernel in linear.hip describes why the kernels want that).
__device__ __forceinline__ __amdgpu_buffer_rsrc_t gnm_tile_rsrc(const float* base, long long rows, int ld, int width) {
    // raw buffer (stride 0): byte offsets >= num_records read 0 / are not written.  On gfx950 the check covers the
    // scalar offset too (tools/ubench/soffset_check.hip: a load that leaves the range only through soffset returns 0),
    // so the loads below may carry their row step in soffset; the STORES carry it in the vector offset for another
    // reason (the data-register hazard described at gnm_lin_stream_kernel).
#ifdef GNM_ABLATE_TILE_TRAFFIC       // tuning builds: every tile descriptor empty -- the kernels' time without tile traffic
    const unsigned bytes = 0u;
    (void)rows; (void)ld; (void)width;
#else
    const unsigned bytes = rows > 0 ? (unsigned)(((rows - 1) * ld + width) * 4) : 0u;
#endif
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(base), 0, (int)bytes, 0x00020000);
}

// Element e of the sum over `nblk` partials, in the one summation order both reduce kernels use: thread group g
// (32 groups of 32 lanes) sums partials g, g + 32, ... four at a time, and the groups are added in order through LDS.
// The sum is returned to the first 32 threads of the workgroup.
__device__ __forceinline__ float reduce_partials_element(const float* __restrict__ partial, int nblk, long long stride, int e,
                                                         int count, float (&red)[32][32]) {
    const int tid = threadIdx.x;
    const int grp = tid >> 5, ngrp = (int)blockDim.x >> 5;
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
    if (e < count) {
        int b = grp;
        for (; b + 3 * ngrp < nblk; b += 4 * ngrp) {       // 4 independent loads in flight, fixed summation order
            const float v0 = partial[(size_t)(b + 0 * ngrp) * stride + e], v1 = partial[(size_t)(b + 1 * ngrp) * stride + e];
            const float v2 = partial[(size_t)(b + 2 * ngrp) * stride + e], v3 = partial[(size_t)(b + 3 * ngrp) * stride + e];
            s0 += v0; s1 += v1; s2 += v2; s3 += v3;
        }
        for (; b < nblk; b += ngrp) s0 += partial[(size_t)b * stride + e];
    }
    red[grp][tid & 31] = (s0 + s1) + (s2 + s3);
    __syncthreads();
    float s = 0.f;
    if (tid < 32 && e < count)
        for (int g = 0; g < ngrp; ++g) s += red[g][tid];
    return s;
}

// linear_wgrad.hip: one such reduction, `nblk` partials of [H * kw + H] floats in `workspace` into columns
// k0 .. k0 + kw of dW, and db (gnm_linear_wgrad, and the fused backward entries when they are given a dW)
extern "C" __attribute__((visibility("hidden"))) int gnm_reduce_partials(const float* workspace, int nblk, int H, int kw,
                                                                         int k0, float* dW, int ldw, float* db,
                                                                         hipStream_t s);
