// ------------------------------------------------------------------------------
// Fused backward of one Linear that is followed by a train/eval BatchNorm (mlp.py:48,
// graphcnn.py:163): replaces  gnm_bn_bwd_apply -> gnm_linear_wgrad -> gnm_linear_fwd(dgrad)
// (10 passes over [N,H] arrays) by ONE pass that reads G (masked incoming gradient), Z (this
// Linear's output = the BatchNorm input) and X (this Linear's input) and writes dX:
//     dZ = cA * (G - m1 - xhat * m2),  xhat = (Z - mean) * rstd        (BatchNorm backward)
//     dX = dZ W                                                          (64 MFMAs per 32 rows)
//     dW = dZ^T f(X),  db = sum dZ                                       (64 MFMAs per 32 rows)
// The dZ tile lives only in the wave's LDS staging image: dgrad reads it row-wise
// (ds_read_b128 A fragments), wgrad column-wise (ds_read_b32, lane = column).  f(X) operands
// come straight from global memory (128 B per half-wave), all loads of a tile are issued
// before its MFMAs.  K, H in {32, 64} (accumulators: 32*K/32 + 16*(H/32)*(K/32) registers), or K < 32 (NARROW).
// ------------------------------------------------------------------------------
// (The forward Linear kernels are in linear.hip, the stand-alone weight gradient and the partial reductions in
// linear_wgrad.hip; what the three units share is in gnm_linear.h.)
#include "gnm_linear.h"

struct LbArgs {
    const float* G; const float* Z; const float* X; const float* W;
    const float* mean; const float* rstd; const float* cA; const float* m1; const float* m2;
    const float* pro_scale; const float* pro_shift;
    float* dA; float* partial;
    // optional: dA is the gradient arriving at relu(bn_lo(sZ)) -- apply that ReLU mask to it on the way
    // out and reduce the lower BatchNorm's backward sums (replaces gnm_bn_relu_bwd_stats for it)
    const float* sZ; const float* s_scale; const float* s_shift; const float* s_mean; const float* s_rstd;
    double* s_partial;         // [gridDim.x][2][K]
    int ldg, ldz, ldx, ldw, lda, ldsz;
    int N, K, H;
    int pro_relu;
    unsigned long long* stamps;   // tuning builds only, as LinArgs::stamps
    const float* bias;            // gnm_linear_bwd_rz_kernel only: Z is not read but recomputed as f(X) W^T + bias
    int part_rows;                // ... and the rows of `partial` / `s_partial` its launch writes (two per workgroup)
};

// What both fused-backward entries fill the same way.  Every other field is zero: gnm_linear_bwd_fused then sets Z,
// gnm_linear_bwd_fused_rz the bias and part_rows.
static inline LbArgs lb_args(const float* G, int ldg, const float* mean, const float* rstd, const float* cA,
                             const float* m1, const float* m2, const float* X, int ldx, const float* pro_scale,
                             const float* pro_shift, int pro_relu, const float* W, int ldw, float* dA, int lda,
                             float* workspace, int N, int K, int H, const float* sZ, int ldsz, const float* s_scale,
                             const float* s_shift, const float* s_mean, const float* s_rstd, double* s_partial) {
    LbArgs a = {};
    a.sZ = sZ; a.s_scale = s_scale; a.s_shift = s_shift; a.s_mean = s_mean; a.s_rstd = s_rstd;
    a.s_partial = s_partial; a.ldsz = ldsz;
    a.G = G; a.X = X; a.W = W; a.mean = mean; a.rstd = rstd; a.cA = cA; a.m1 = m1; a.m2 = m2;
    a.pro_scale = pro_scale; a.pro_shift = pro_shift; a.dA = dA; a.partial = workspace;
    a.ldg = ldg; a.ldx = ldx; a.ldw = ldw; a.lda = lda; a.N = N; a.K = K; a.H = H; a.pro_relu = pro_relu;
    a.stamps = g_lin_stamps;
    return a;
}

// LDS layouts of the fused backward kernels, in bytes, used by each kernel and by its launcher.  The dW / db dump of
// lb_combine (NW waves of HT x KT tiles and HT db rows) reuses the kernel's LDS from the start, so a launch asks for
// the larger of the two.
constexpr size_t lb_dump_bytes(int HT, int KT, int NW) { return ((size_t)NW * HT * KT * 1024 + (size_t)NW * HT * 64) * 4; }
// gnm_linear_bwd_fused_kernel (COEF = false) and gnm_linear_bwd_pipe_kernel (COEF = true): the weight image (fp32
// [HP][KP], or SPLITD: three planes of EW operand entries), the four waves' tile images [32][XS], coef [5][HP]
template <int KT, int HT, bool SPLITD, bool COEF>
struct LbLds {
    static constexpr int KP = KT * 32, HP = HT * 32, XS = (KP > HP ? KP : HP) + 4, EW = 4 * KT * 64;
    static constexpr size_t xs_off = SPLITD ? (size_t)3 * EW * 16 : (size_t)HP * KP * 4;
    static constexpr size_t coef_off = xs_off + (size_t)4 * 32 * XS * 4;
    static constexpr size_t body = coef_off + (COEF ? (size_t)5 * HP * 4 : 0);
    static constexpr size_t total = body > lb_dump_bytes(HT, KT, 4) ? body : lb_dump_bytes(HT, KT, 4);
    static_assert((size_t)4 * 2 * KP * 8 <= body, "the lower BatchNorm's sums [4][2][KP] fp64 reuse the body");
};
// gnm_linear_bwd_rz_kernel and (NARROW) gnm_linear_bwd_rzn_kernel: forward planes Wf [3][EWF], k-major planes Wb
// [3][EWB], the waves' tile images [32][XS], coef [6][64] and (not NARROW) the prologue vectors psv [2][64]
static constexpr int kRzWaves = 8;
template <bool NARROW>
struct RzLds {
    static constexpr int EWF = NARROW ? 128 : 512, EWB = NARROW ? 256 : 512, XS = 68, KT = NARROW ? 1 : 2;
    static constexpr size_t wb_off = (size_t)3 * EWF * 16;
    static constexpr size_t xs_off = wb_off + (size_t)3 * EWB * 16;
    static constexpr size_t coef_off = xs_off + (size_t)kRzWaves * 32 * XS * 4;
    static constexpr size_t psv_off = coef_off + (size_t)6 * 64 * 4;
    static constexpr size_t body = psv_off + (NARROW ? 0 : (size_t)2 * 64 * 4);
    static constexpr size_t total = body > lb_dump_bytes(2, KT, kRzWaves) ? body : lb_dump_bytes(2, KT, kRzWaves);
};

// The BatchNorm-backward coefficient vectors of a Linear's output columns into LDS: coef[5 or 6][HP] = mean, rstd, cA,
// m1, m2 and (BIAS) the Linear's bias, zero when it has none.
template <int HP, bool BIAS>
__device__ __forceinline__ void lb_stage_coef(float* coef, const float* mean, const float* rstd, const float* cA,
                                              const float* m1, const float* m2, const float* bias, int tid, int nt) {
    for (int idx = tid; idx < HP; idx += nt) {
        coef[idx] = mean[idx]; coef[HP + idx] = rstd[idx]; coef[2 * HP + idx] = cA[idx];
        coef[3 * HP + idx] = m1[idx]; coef[4 * HP + idx] = m2[idx];
        if (BIAS) coef[5 * HP + idx] = bias ? bias[idx] : 0.f;
    }
}

// The dW / db epilogue of the fused backward kernels.  Every wave dumps its HT x KT accumulator tiles and its HT db
// rows to LDS (over everything the tile loop kept there); each group of four waves is then summed, in the order
// w = 0, 1, 2, 3, into one partial row [H * K + H]: row blockIdx.x * GROUPS + grp, when below part_rows (GROUPS > 1).
// CLIP: columns of dW at or past K (a narrow input's zero padding) are not written.
template <int HT, int KT, int GROUPS, bool CLIP>
__device__ __forceinline__ void lb_combine(char* smem, const f32x16 (&wacc)[HT][KT], const float (&dbacc)[HT], float* partial,
                                           int H, int K, int part_rows, int tid, int lane, int wave) {
    constexpr int TILE = 16 * 64, WT = HT * KT * TILE, NW = 4 * GROUPS, NT = NW * 64;
    __syncthreads();
    float* dump = reinterpret_cast<float*>(smem);                 // [NW][HT*KT][16][64] + [NW][HT][64]
    float* mine = dump + (size_t)wave * WT;
#pragma unroll
    for (int a = 0; a < HT; ++a)
#pragma unroll
        for (int b = 0; b < KT; ++b)
#pragma unroll
            for (int r = 0; r < 16; ++r) mine[(a * KT + b) * TILE + r * 64 + lane] = wacc[a][b][r];
    float* dbdump = dump + (size_t)NW * WT;
#pragma unroll
    for (int a = 0; a < HT; ++a) dbdump[(wave * HT + a) * 64 + lane] = dbacc[a];
    __syncthreads();
    const size_t pstride = (size_t)H * K + H;
    for (int idx = tid; idx < GROUPS * WT; idx += NT) {
        const int grp = idx / WT, rem = idx - grp * WT;
        const int prow = blockIdx.x * GROUPS + grp;
        if (GROUPS > 1 && prow >= part_rows) continue;
        const int ab = rem / TILE;
        const int rl = rem - ab * TILE;
        const int r = rl >> 6, ln = rl & 63;
        const int a = ab / KT, b = ab - a * KT;
        const int row = 32 * a + (r & 3) + 8 * (r >> 2) + 4 * (ln >> 5);
        const int col = 32 * b + (ln & 31);
        if (CLIP && col >= K) continue;
        float sum = 0.f;
#pragma unroll
        for (int w = 0; w < 4; ++w) sum += dump[(size_t)(4 * grp + w) * WT + rem];
        partial[(size_t)prow * pstride + (size_t)row * K + col] = sum;
    }
    for (int idx = tid; idx < GROUPS * HT * 32; idx += NT) {
        const int grp = idx / (HT * 32), a = (idx >> 5) % HT, ii = idx & 31;
        const int prow = blockIdx.x * GROUPS + grp;
        if (GROUPS > 1 && prow >= part_rows) continue;
        float sum = 0.f;
#pragma unroll
        for (int w = 0; w < 4; ++w) sum += dbdump[((4 * grp + w) * HT + a) * 64 + ii] + dbdump[((4 * grp + w) * HT + a) * 64 + 32 + ii];
        partial[(size_t)prow * pstride + (size_t)H * K + 32 * a + ii] = sum;
    }
}

// NARROW: K < 32 (the first Linear of layer 0, K = F0): one zero-padded 32-column tile, guarded scalar
// accesses to X / W / dX, which are small next to the [N,H] streams G and Z.
// SAMEZ (with STATS): the lower BatchNorm's input sZ IS this Linear's input X and its scale/shift ARE the prologue
// (the second Linear of every MLP) -- the ReLU mask and the BatchNorm sums are then taken from the X values the
// weight-gradient product already holds in registers: the wgrad contraction index is permuted so that a lane's X
// rows are its dX accumulator rows, and no second pass over that array is made.
template <int KT, int HT, bool STATS, bool NARROW = false, bool SAMEZ = false, bool SPLITD = false>
__global__ void __launch_bounds__(256, 2) gnm_linear_bwd_fused_kernel(const LbArgs p) {   // 2 waves/SIMD: <= 256 registers
    static_assert(!SPLITD || (HT == 2 && NARROW), "SPLITD: H = 64, the narrow form (SAMEZ K = 64: gnm_linear_bwd_pipe_sz_kernel)");
    static_assert(!NARROW || (KT == 1 && !STATS), "narrow K: one tile, no lower BatchNorm");
    static_assert(!SAMEZ || STATS, "SAMEZ is a STATS variant");
    using L = LbLds<KT, HT, SPLITD, false>;
    constexpr int KP = L::KP, HP = L::HP, XS = L::XS, EW = L::EW;
    constexpr int H4 = HP / 4;                    // float4 per dZ row
    constexpr int NLD = (32 * H4) / 64;           // float4 loads per lane for a [32][HP] tile
    constexpr int RSTEP = 64 / H4;
    constexpr int KH = HP / 2;                    // dgrad MFMA steps (contraction over H)
    constexpr int O4 = KP / 4;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    // SPLITD (the narrow H = 64 form): the dgrad product runs on the bf16 matrix pipe with dZ and W split into three
    // exact bf16 planes each (see gnm_lin_split_kernel); the weight image is then the three operand planes
    float* Wt = reinterpret_cast<float*>(smem);                   // [HP][KP]: W itself (contraction index first)
    gnm_u32x4* Wp = reinterpret_cast<gnm_u32x4*>(smem);                   // SPLITD: [3][EW] operand entries instead
    float* Xs_all = reinterpret_cast<float*>(smem + L::xs_off);   // [4][32][XS]
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int i = lane & 31, h = lane >> 5;
    float* Xs = Xs_all + wave * 32 * XS;
    GNM_LSTAMP(0)
    if constexpr (SPLITD) {
        for (int e = tid; e < EW; e += 256) {
            const int n = e & 31, kg = (e >> 5) & 1, c = (e >> 6) % KT, m = e / (64 * KT);
            float f[8];
#pragma unroll
            for (int j = 0; j < 8; ++j)
                f[j] = (!NARROW || 32 * c + n < p.K) ? p.W[(size_t)(8 * m + 32 * kg + j) * p.ldw + 32 * c + n] : 0.f;
            gnm_u32x4 p1, p2, p3;
            gnm_split8(f, p1, p2, p3);
            Wp[e] = p1; Wp[EW + e] = p2; Wp[2 * EW + e] = p3;
        }
    } else {
        for (int idx = tid; idx < HP * KP; idx += 256) {
            const int hh = idx / KP, k = idx - hh * KP;
            Wt[idx] = (!NARROW || k < p.K) ? p.W[(size_t)hh * p.ldw + k] : 0.f;
        }
    }
    __syncthreads();
    GNM_LSTAMP(1)
    int tk = 0;

    const int c4 = lane % H4, lrow0 = lane / H4;
    // BatchNorm-backward coefficients of this lane's column chunk: kept in registers for the whole kernel, except in
    // the SAMEZ variant, which needs those 20 registers across the MFMA phases and re-reads them (L1 hits) per tile
    float4 mu, rs, ca, a1, a2;
    if constexpr (!SAMEZ) {
        mu = *reinterpret_cast<const float4*>(p.mean + 4 * c4);
        rs = *reinterpret_cast<const float4*>(p.rstd + 4 * c4);
        ca = *reinterpret_cast<const float4*>(p.cA + 4 * c4);
        a1 = *reinterpret_cast<const float4*>(p.m1 + 4 * c4);
        a2 = *reinterpret_cast<const float4*>(p.m2 + 4 * c4);
    }
    float psc[KT], psh[KT];
#pragma unroll
    for (int b = 0; b < KT; ++b) {
        const bool kin = !NARROW || 32 * b + i < p.K;
        psc[b] = (p.pro_scale && kin) ? p.pro_scale[32 * b + i] : 1.f;
        psh[b] = (p.pro_scale && kin) ? p.pro_shift[32 * b + i] : 0.f;
    }
    f32x16 wacc[HT][KT];                          // dW accumulators
#pragma unroll
    for (int a = 0; a < HT; ++a)
#pragma unroll
        for (int b = 0; b < KT; ++b)
#pragma unroll
            for (int r = 0; r < 16; ++r) wacc[a][b][r] = 0.f;
    float dbacc[HT];
#pragma unroll
    for (int a = 0; a < HT; ++a) dbacc[a] = 0.f;
    // lower-BatchNorm statistics of the masked dX (this lane's 16-B column chunk oc4 of the output rows)
    constexpr int OR = 64 / O4;                   // output rows covered per pass of the store loop
    const int oc4 = lane % O4, orow0 = lane / O4;
    float4 ss1 = make_float4(0.f, 0.f, 0.f, 0.f), ss2 = ss1;
    float cmu[KT], crs[KT], cs1[KT], cs2[KT];     // SAMEZ: this lane's columns 32b + i of the lower BatchNorm
#pragma unroll
    for (int b = 0; b < KT; ++b) {
        cmu[b] = SAMEZ ? p.s_mean[32 * b + i] : 0.f;
        crs[b] = SAMEZ ? p.s_rstd[32 * b + i] : 0.f;
        cs1[b] = 0.f; cs2[b] = 0.f;
    }

    const int ntiles = (p.N + 31) / 32;
    const int nlast = p.N - 1;
    for (int t = lin_first_tile(wave, 1, gridDim.x); t < ntiles; t += gridDim.x * 4) {
        const int r0 = t * 32;
        GNM_LSTAMP(2 + 5 * min(tk, 11))
        // ---- all global loads of the tile first -------------------------------------
        float4 g4[NLD], z4[NLD];
#pragma unroll
        for (int j = 0; j < NLD; ++j) {
            const int grow = min(r0 + lrow0 + j * RSTEP, nlast);
            g4[j] = *reinterpret_cast<const float4*>(p.G + (size_t)grow * p.ldg + 4 * c4);
            z4[j] = *reinterpret_cast<const float4*>(p.Z + (size_t)grow * p.ldz + 4 * c4);
        }
        if constexpr (SAMEZ) {
            mu = *reinterpret_cast<const float4*>(p.mean + 4 * c4);
            rs = *reinterpret_cast<const float4*>(p.rstd + 4 * c4);
            ca = *reinterpret_cast<const float4*>(p.cA + 4 * c4);
            a1 = *reinterpret_cast<const float4*>(p.m1 + 4 * c4);
            a2 = *reinterpret_cast<const float4*>(p.m2 + 4 * c4);
        }
        __builtin_amdgcn_sched_barrier(0);
        // ---- dZ tile -> LDS (rows past N are zero: they must not contribute) ----------
#pragma unroll
        for (int j = 0; j < NLD; ++j) {
            const int lrow = lrow0 + j * RSTEP;
            float4 d;
            d.x = ca.x * (g4[j].x - a1.x - (z4[j].x - mu.x) * rs.x * a2.x);
            d.y = ca.y * (g4[j].y - a1.y - (z4[j].y - mu.y) * rs.y * a2.y);
            d.z = ca.z * (g4[j].z - a1.z - (z4[j].z - mu.z) * rs.z * a2.z);
            d.w = ca.w * (g4[j].w - a1.w - (z4[j].w - mu.w) * rs.w * a2.w);
            if (r0 + lrow >= p.N) d = make_float4(0.f, 0.f, 0.f, 0.f);
            *reinterpret_cast<float4*>(Xs + lrow * XS + 4 * c4) = d;
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        // f(X) operands of the wgrad product: issued now (the G/Z registers are dead), they are in
        // flight during the 64 dgrad MFMAs below
        float xv[16][KT];                         // X[r0 + 2s + h][32b + i]
#pragma unroll
        for (int s = 0; s < 16; ++s) {
            // contraction index of the wgrad product: any order, as long as dZ (below) uses the same one.  SAMEZ takes
            // the 32x32 accumulator's row order, so that xv[s] sits on the rows of dacc[.][s]
            const int krow = SAMEZ ? (s & 3) + 8 * (s >> 2) + 4 * h : 2 * s + h;
            const int grow = min(r0 + krow, nlast);
#pragma unroll
            for (int b = 0; b < KT; ++b)
                xv[s][b] = (!NARROW || 32 * b + i < p.K) ? p.X[(size_t)grow * p.ldx + 32 * b + i] : 0.f;
        }
        __builtin_amdgcn_sched_barrier(0);
        GNM_LSTAMP(3 + 5 * min(tk, 11))
        // ---- dX = dZ W ------------------------------------------------------------------
        f32x16 dacc[KT];
        if constexpr (SPLITD) {
            if (p.dA) {
#pragma unroll
                for (int c = 0; c < KT; ++c)
#pragma unroll
                    for (int r = 0; r < 16; ++r) dacc[c][r] = 0.f;
                lin_dgrad_split<KT, HP>(dacc, Xs, XS, Wp, i, h, lane);
            }
        } else if (p.dA) {
            float a[KH];
#pragma unroll
            for (int j = 0; j < KH / 4; ++j) {
                const float4 v = *reinterpret_cast<const float4*>(Xs + i * XS + KH * h + 4 * j);
                a[4 * j + 0] = v.x; a[4 * j + 1] = v.y; a[4 * j + 2] = v.z; a[4 * j + 3] = v.w;
            }
#pragma unroll
            for (int c = 0; c < KT; ++c)
#pragma unroll
                for (int r = 0; r < 16; ++r) dacc[c][r] = 0.f;
            const float* wrow = Wt + (size_t)(KH * h) * KP + i;
#pragma unroll
            for (int s = 0; s < KH; ++s) {
#pragma unroll
                for (int c = 0; c < KT; ++c)
                    dacc[c] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[s], wrow[s * KP + 32 * c], dacc[c], 0, 0, 0);
            }
        }
        GNM_LSTAMP(4 + 5 * min(tk, 11))
        // ---- dW += dZ^T f(X), db += column sums of dZ -----------------------------------
#pragma unroll
        for (int s = 0; s < 16; ++s) {
            float av[HT];
            const int krow = SAMEZ ? (s & 3) + 8 * (s >> 2) + 4 * h : 2 * s + h;
#pragma unroll
            for (int a = 0; a < HT; ++a) av[a] = Xs[krow * XS + 32 * a + i];
            float xf[KT];
#pragma unroll
            for (int b = 0; b < KT; ++b) {
                float x = xv[s][b];
                if (p.pro_scale) {
                    x = x * psc[b] + psh[b];
                    if (p.pro_relu) x = gnm_relu(x);
                    if (NARROW && !(32 * b + i < p.K)) x = 0.f;      // padding columns stay zero
                }
                xf[b] = x;                                          // (SAMEZ keeps the raw Z in xv for the epilogue)
            }
#pragma unroll
            for (int a = 0; a < HT; ++a) {
                dbacc[a] += av[a];
#pragma unroll
                for (int b = 0; b < KT; ++b)
                    wacc[a][b] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[a], xf[b], wacc[a][b], 0, 0, 0);
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();          // everyone is done reading the dZ image
        GNM_LSTAMP(5 + 5 * min(tk, 11))
        // ---- store dX through the staging image (16-B row-contiguous stores) ---------------
        if (p.dA) {
            if constexpr (SAMEZ) {
                // ReLU mask of the lower BatchNorm and its backward sums, on the accumulator itself: lane (i, h) holds
                // column 32c + i of rows (r & 3) + 8 (r >> 2) + 4h, and xv[r][c] is Z of exactly that element
#pragma unroll
                for (int c = 0; c < KT; ++c)
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const float z = xv[r][c];
                        float g = dacc[c][r];
                        if (z * psc[c] + psh[c] <= 0.f) g = 0.f;
                        if (r0 + (r & 3) + 8 * (r >> 2) + 4 * h < p.N) {
                            cs1[c] += g;
                            cs2[c] += g * ((z - cmu[c]) * crs[c]);
                        }
                        dacc[c][r] = g;
                    }
            }
#pragma unroll
            for (int c = 0; c < KT; ++c)
#pragma unroll
                for (int r = 0; r < 16; ++r) Xs[((r & 3) + 8 * (r >> 2) + 4 * h) * XS + 32 * c + i] = dacc[c][r];
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            if constexpr (STATS && !SAMEZ) {
                __builtin_amdgcn_sched_barrier(0);   // keep these loads below the MFMA phases (register peak)
                // coefficient vectors are (re)loaded here, not kept across the MFMA phases: they are
                // L1/L2 hits and 16 registers held for the whole tile would cost a wave of occupancy
                const float4 lsc = *reinterpret_cast<const float4*>(p.s_scale + 4 * oc4);
                const float4 lsh = *reinterpret_cast<const float4*>(p.s_shift + 4 * oc4);
                const float4 lmu = *reinterpret_cast<const float4*>(p.s_mean + 4 * oc4);
                const float4 lrs = *reinterpret_cast<const float4*>(p.s_rstd + 4 * oc4);
                constexpr int NJ = 32 / OR, HB = NJ > 4 ? 4 : NJ;     // 4 rows (16 registers of Z) at a time
#pragma unroll
                for (int j0 = 0; j0 < NJ; j0 += HB) {
                float4 zl[HB];
#pragma unroll
                for (int j = 0; j < HB; ++j) {
                    const int grow = min(r0 + orow0 + (j0 + j) * OR, nlast);
                    zl[j] = *reinterpret_cast<const float4*>(p.sZ + (size_t)grow * p.ldsz + 4 * oc4);
                }
#pragma unroll
                for (int j = 0; j < HB; ++j) {
                    const int row = orow0 + (j0 + j) * OR;
                    float4 g = *reinterpret_cast<const float4*>(Xs + row * XS + 4 * oc4);
                    const float4 z = zl[j];
                    if (z.x * lsc.x + lsh.x <= 0.f) g.x = 0.f;
                    if (z.y * lsc.y + lsh.y <= 0.f) g.y = 0.f;
                    if (z.z * lsc.z + lsh.z <= 0.f) g.z = 0.f;
                    if (z.w * lsc.w + lsh.w <= 0.f) g.w = 0.f;
                    if (r0 + row < p.N) {
                        *reinterpret_cast<float4*>(p.dA + (size_t)(r0 + row) * p.lda + 4 * oc4) = g;
                        ss1.x += g.x; ss1.y += g.y; ss1.z += g.z; ss1.w += g.w;
                        ss2.x += g.x * ((z.x - lmu.x) * lrs.x); ss2.y += g.y * ((z.y - lmu.y) * lrs.y);
                        ss2.z += g.z * ((z.z - lmu.z) * lrs.z); ss2.w += g.w * ((z.w - lmu.w) * lrs.w);
                    }
                }
                }
            } else if constexpr (NARROW) {
                for (int idx = lane; idx < 32 * p.K; idx += 64) {
                    const int row = idx / p.K, col = idx - row * p.K;
                    if (r0 + row < p.N) p.dA[(size_t)(r0 + row) * p.lda + col] = Xs[row * XS + col];
                }
            } else {
#pragma unroll
                for (int idx = lane; idx < 32 * O4; idx += 64) {
                    const int row = idx / O4, oc = idx - row * O4;
                    if (r0 + row < p.N)
                        *reinterpret_cast<float4*>(p.dA + (size_t)(r0 + row) * p.lda + 4 * oc) =
                            *reinterpret_cast<const float4*>(Xs + row * XS + 4 * oc);
                }
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
        }
        GNM_LSTAMP(6 + 5 * min(tk, 11))
        ++tk;
    }
    GNM_LSTAMP(62)

    // ---- lower-BatchNorm sums: lanes with the same column chunk, then the 4 waves (fixed order) ----
    if constexpr (STATS) {
        __syncthreads();
        double* sred = reinterpret_cast<double*>(smem);           // [4 waves][2][KP]
        if constexpr (SAMEZ) {
#pragma unroll
            for (int c = 0; c < KT; ++c) {                          // the two half-waves hold the same columns
                double d1 = (double)cs1[c], d2 = (double)cs2[c];
                d1 += __shfl_xor(d1, 32, 64);
                d2 += __shfl_xor(d2, 32, 64);
                if (h == 0) {
                    sred[(wave * 2 + 0) * KP + 32 * c + i] = d1;
                    sred[(wave * 2 + 1) * KP + 32 * c + i] = d2;
                }
            }
        }
        float v1[4] = {ss1.x, ss1.y, ss1.z, ss1.w}, v2[4] = {ss2.x, ss2.y, ss2.z, ss2.w};
#pragma unroll
        for (int c = 0; c < (SAMEZ ? 0 : 4); ++c) {
            double d1 = (double)v1[c], d2 = (double)v2[c];
#pragma unroll
            for (int off = O4; off < 64; off <<= 1) {
                d1 += __shfl_xor(d1, off, 64);
                d2 += __shfl_xor(d2, off, 64);
            }
            if (lane < O4) {
                sred[(wave * 2 + 0) * KP + 4 * oc4 + c] = d1;
                sred[(wave * 2 + 1) * KP + 4 * oc4 + c] = d2;
            }
        }
        __syncthreads();
        for (int idx = tid; idx < 2 * KP; idx += 256) {
            const int which = idx / KP, col = idx - which * KP;
            double sum = 0.0;
            for (int w = 0; w < 4; ++w) sum += sred[(w * 2 + which) * KP + col];
            p.s_partial[((size_t)blockIdx.x * 2 + which) * p.K + col] = sum;
        }
    }

    lb_combine<HT, KT, 1, NARROW>(smem, wacc, dbacc, p.partial, p.H, p.K, 0, tid, lane, wave);
    GNM_LSTAMP(63)
}

// ---------------------------------------------------------------------------------
// The same fused backward for the form that has no statistics to reduce (the FIRST Linear of an MLP: its input is
// the aggregation output), software-pipelined across tiles: the G / Z tile of the wave's NEXT tile is requested in the
// middle of the current one -- behind the dgrad MFMAs, when the A fragments' 32 registers are free -- and travels
// under the wgrad MFMAs and the epilogue (the in-kernel timeline had a wave of the kernel above waiting for G and Z
// for 30-38 % of its life).  gfx950 retires vector-memory operations in issue order, so for that wait to be a counted
// one (not a drain that also waits for the dX stores issued after the request) every access between them is
// unconditional: tile loads and dX stores go through buffer descriptors that clip rows past N, and the first tile is
// peeled so that the loop is entered with the same queue its back edge carries (see gnm_lin_stream_kernel).
// The statistics variants above stay as they are: at 256 registers they have no room for a tile in flight in their phase
// order (tried, in the shared template and as a SAMEZ flavour of this kernel with the request behind the wgrad MFMAs:
// 31-150 spills), and any restructuring of that kernel's body moved its register allocation.  The one the step runs,
// SAMEZ at K = H = 64, is pipelined in a kernel of its own with the epilogue IN FRONT of the weight-gradient product,
// which frees the dX accumulators before the request: gnm_linear_bwd_pipe_sz_kernel below.
// ---------------------------------------------------------------------------------
// SPLITD (K = H = 64): the dgrad product on the bf16 matrix pipe, dZ and W as three exact bf16 planes each (see
// gnm_lin_split_kernel).  wgrad keeps the fp32 instruction: on the bf16 pipe as well (a separate kernel, batch row as
// the contraction index, dZ columns from the LDS image and X rows from global split per tile) it was 12 % faster than
// the fp32 kernel stand-alone but spilled 18 dwords, and in the step it came out 0.3 % behind this form.
template <int KT, int HT, bool SPLITD = false>
__global__ void __launch_bounds__(256, 2) gnm_linear_bwd_pipe_kernel(const LbArgs p) {
    static_assert(!SPLITD || (KT == 2 && HT == 2), "SPLITD: K = H = 64 only");
    using L = LbLds<KT, HT, SPLITD, true>;
    constexpr int KP = L::KP, HP = L::HP, XS = L::XS, EW = L::EW;
    constexpr int H4 = HP / 4;
    constexpr int NLD = (32 * H4) / 64;
    constexpr int RSTEP = 64 / H4;
    constexpr int KH = HP / 2;
    constexpr int O4 = KP / 4;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* Wt = reinterpret_cast<float*>(smem);                   // [HP][KP]
    gnm_u32x4* Wp = reinterpret_cast<gnm_u32x4*>(smem);                   // SPLITD: [3][EW] bf16 operand entries of W instead
    float* Xs_all = reinterpret_cast<float*>(smem + L::xs_off);   // [4][32][XS]
    float* coef = reinterpret_cast<float*>(smem + L::coef_off);   // [5][HP]: mean, rstd, cA, m1, m2 of the BatchNorm
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int i = lane & 31, h = lane >> 5;
    float* Xs = Xs_all + wave * 32 * XS;
    if constexpr (SPLITD) {
        lin_stage_planes<KT, 32, true, false>(Wp, EW, p.W, p.ldw, 0, tid, 256);
    } else {
        for (int idx = tid; idx < HP * KP; idx += 256) {
            const int hh = idx / KP, k = idx - hh * KP;
            Wt[idx] = p.W[(size_t)hh * p.ldw + k];
        }
    }
    // the BatchNorm-backward coefficient vectors live in LDS and are read per tile (5 ds_read_b128: they count on
    // lgkmcnt, so re-reading them costs no place in the in-order vector-memory queue and no registers across the tile)
    lb_stage_coef<HP, false>(coef, p.mean, p.rstd, p.cA, p.m1, p.m2, nullptr, tid, 256);
    const int c4 = lane % H4, lrow0 = lane / H4;
    float psc[KT], psh[KT];
#pragma unroll
    for (int b = 0; b < KT; ++b) {
        psc[b] = p.pro_scale ? p.pro_scale[32 * b + i] : 1.f;
        psh[b] = p.pro_scale ? p.pro_shift[32 * b + i] : 0.f;
    }
    __builtin_amdgcn_s_waitcnt(0x0F70);           // vmcnt(0): nothing from the preamble is pending inside the tile loop
    __syncthreads();
    f32x16 wacc[HT][KT];
#pragma unroll
    for (int a = 0; a < HT; ++a)
#pragma unroll
        for (int b = 0; b < KT; ++b)
#pragma unroll
            for (int r = 0; r < 16; ++r) wacc[a][b][r] = 0.f;
    float dbacc[HT];
#pragma unroll
    for (int a = 0; a < HT; ++a) dbacc[a] = 0.f;

    const int ntiles = (p.N + 31) / 32;
    const int tstride = gridDim.x * 4;
    const int gz_voff_g = (lrow0 * p.ldg + 4 * c4) * 4, gz_step_g = RSTEP * p.ldg * 4;
    const int gz_voff_z = (lrow0 * p.ldz + 4 * c4) * 4, gz_step_z = RSTEP * p.ldz * 4;
    const int x_voff = (h * p.ldx + i) * 4;                       // X[r0 + 2 s + h][32 b + i]
    const int out_voff = ((lane / O4) * p.lda + 4 * (lane % O4)) * 4, out_step = (64 / O4) * p.lda * 4;
    // (no dX wanted: an empty descriptor over any readable address -- the stores stay unconditional)
    const float* dxbase = p.dA ? p.dA : p.G;

    gnm_u32x4 g4[NLD], z4[NLD];
    auto load_gz = [&](int tile) {
        const long long row0 = (long long)tile * 32;
        const long long rows = min((long long)p.N - row0, 32LL);
        const __amdgpu_buffer_rsrc_t rg = gnm_tile_rsrc(p.G + row0 * p.ldg, rows, p.ldg, HP);
        const __amdgpu_buffer_rsrc_t rz = gnm_tile_rsrc(p.Z + row0 * p.ldz, rows, p.ldz, HP);
#pragma unroll
        for (int j = 0; j < NLD; ++j) {
            g4[j] = __builtin_amdgcn_raw_buffer_load_b128(rg, gz_voff_g, j * gz_step_g, 0);
            z4[j] = __builtin_amdgcn_raw_buffer_load_b128(rz, gz_voff_z, j * gz_step_z, 0);
        }
    };
    auto do_tile = [&](int t, int t_next) {
        const int r0 = t * 32;
        const int rows = min(p.N - r0, 32);
        // ---- dZ tile -> LDS (rows past N are zero: they must not contribute) ----------
        const float4 mu = *reinterpret_cast<const float4*>(coef + 4 * c4);
        const float4 rs = *reinterpret_cast<const float4*>(coef + HP + 4 * c4);
        const float4 ca = *reinterpret_cast<const float4*>(coef + 2 * HP + 4 * c4);
        const float4 a1 = *reinterpret_cast<const float4*>(coef + 3 * HP + 4 * c4);
        const float4 a2 = *reinterpret_cast<const float4*>(coef + 4 * HP + 4 * c4);
#pragma unroll
        for (int j = 0; j < NLD; ++j) {
            const int lrow = lrow0 + j * RSTEP;
            const float4 gj = __builtin_bit_cast(float4, g4[j]), zj = __builtin_bit_cast(float4, z4[j]);
            float4 d;
            d.x = ca.x * (gj.x - a1.x - (zj.x - mu.x) * rs.x * a2.x);
            d.y = ca.y * (gj.y - a1.y - (zj.y - mu.y) * rs.y * a2.y);
            d.z = ca.z * (gj.z - a1.z - (zj.z - mu.z) * rs.z * a2.z);
            d.w = ca.w * (gj.w - a1.w - (zj.w - mu.w) * rs.w * a2.w);
            if (lrow >= rows) d = make_float4(0.f, 0.f, 0.f, 0.f);
            *reinterpret_cast<float4*>(Xs + lrow * XS + 4 * c4) = d;
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        // f(X) operands of the wgrad product: in flight during the dgrad MFMAs (clipped rows read 0; their dZ is 0)
        float xv[16][KT];
        {
            const __amdgpu_buffer_rsrc_t rx = gnm_tile_rsrc(p.X + (size_t)r0 * p.ldx, rows, p.ldx, KP);
#pragma unroll
            for (int s = 0; s < 16; ++s)
#pragma unroll
                for (int b = 0; b < KT; ++b)
                    xv[s][b] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rx, x_voff, (2 * s * p.ldx + 32 * b) * 4, 0));
        }
        __builtin_amdgcn_sched_barrier(0);
        // ---- dX = dZ W ------------------------------------------------------------------
        f32x16 dacc[KT];
        if constexpr (SPLITD) {
#pragma unroll
            for (int c = 0; c < KT; ++c)
#pragma unroll
                for (int r = 0; r < 16; ++r) dacc[c][r] = 0.f;
            lin_dgrad_split<KT, HP>(dacc, Xs, XS, Wp, i, h, lane);
        } else {
            float a[KH];
#pragma unroll
            for (int j = 0; j < KH / 4; ++j) {
                const float4 v = *reinterpret_cast<const float4*>(Xs + i * XS + KH * h + 4 * j);
                a[4 * j + 0] = v.x; a[4 * j + 1] = v.y; a[4 * j + 2] = v.z; a[4 * j + 3] = v.w;
            }
#pragma unroll
            for (int c = 0; c < KT; ++c)
#pragma unroll
                for (int r = 0; r < 16; ++r) dacc[c][r] = 0.f;
            const float* wrow = Wt + (size_t)(KH * h) * KP + i;
#pragma unroll
            for (int s = 0; s < KH; ++s) {
#pragma unroll
                for (int c = 0; c < KT; ++c)
                    dacc[c] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[s], wrow[s * KP + 32 * c], dacc[c], 0, 0, 0);
            }
        }
        load_gz(t_next);                          // past the wave's last tile: empty descriptors, no traffic
        // ---- dW += dZ^T f(X), db += column sums of dZ -----------------------------------
#pragma unroll
        for (int s = 0; s < 16; ++s) {
            float av[HT];
            const int krow = 2 * s + h;
#pragma unroll
            for (int a = 0; a < HT; ++a) av[a] = Xs[krow * XS + 32 * a + i];
            float xf[KT];
#pragma unroll
            for (int b = 0; b < KT; ++b) {
                float x = xv[s][b];
                if (p.pro_scale) {
                    x = x * psc[b] + psh[b];
                    if (p.pro_relu) x = gnm_relu(x);
                }
                xf[b] = x;
            }
#pragma unroll
            for (int a = 0; a < HT; ++a) {
                dbacc[a] += av[a];
#pragma unroll
                for (int b = 0; b < KT; ++b)
                    wacc[a][b] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[a], xf[b], wacc[a][b], 0, 0, 0);
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();          // everyone is done reading the dZ image
        // ---- store dX through the staging image (16-B row-contiguous, clipped buffer stores) ---------
#pragma unroll
        for (int c = 0; c < KT; ++c)
#pragma unroll
            for (int r = 0; r < 16; ++r) Xs[((r & 3) + 8 * (r >> 2) + 4 * h) * XS + 32 * c + i] = dacc[c][r];
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        {
            const __amdgpu_buffer_rsrc_t rd = gnm_tile_rsrc(dxbase + (p.dA ? (size_t)r0 * p.lda : 0), p.dA ? rows : 0, p.lda, KP);
#pragma unroll
            for (int st = 0; st < (32 * O4) / 64; ++st) {
                const int idx = lane + 64 * st;
                const int row = idx / O4, oc = idx - row * O4;
                const gnm_u32x4 v = *reinterpret_cast<const gnm_u32x4*>(Xs + row * XS + 4 * oc);
                __builtin_amdgcn_raw_buffer_store_b128(v, rd, out_voff + st * out_step, 0, kStoreStream);
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
    };
    {
        int t = lin_first_tile(wave, 1, gridDim.x);
        load_gz(t);
        if (t < ntiles) {
            do_tile(t, t + tstride);                  // peeled
            for (t += tstride; t < ntiles; t += tstride) do_tile(t, t + tstride);
        }
    }

    lb_combine<HT, KT, 1, false>(smem, wacc, dbacc, p.partial, p.H, p.K, 0, tid, lane, wave);
}

template <int KT, int HT, bool SPLITD = false>
static int launch_lb_pipe(const LbArgs& a, int grid, hipStream_t s) {
    const size_t lds = LbLds<KT, HT, SPLITD, true>::total;
    GNM_ALLOW_FULL_LDS((&gnm_linear_bwd_pipe_kernel<KT, HT, SPLITD>));
    hipLaunchKernelGGL((gnm_linear_bwd_pipe_kernel<KT, HT, SPLITD>), dim3(grid), dim3(256), lds, s, a);
    GNM_CHECK_LAUNCH();
    return GNM_OK;
}

// ---------------------------------------------------------------------------------
// The SAMEZ + SPLITD form of gnm_linear_bwd_fused_kernel (K = H = 64, the second Linear of every MLP: five launches of
// the headline step), software-pipelined across tiles like the kernel above.  What makes room for a G / Z tile in
// flight is the phase order: the epilogue (ReLU mask of the lower BatchNorm, its two sums, the dX stores) runs straight
// behind dgrad, IN FRONT of the weight-gradient product, so the 32 dX accumulators are dead when the next tile is
// requested and the product runs with  wacc 64 + xv 32 + G/Z in flight 64  live.  The dZ image is still needed by that
// product, so dX is not transposed through it but through a second, 16-row image per wave: 16 rows at a time, with the
// 16-byte row-contiguous stores of the other kernels (76 KB of LDS per workgroup: two still share a CU).  (4-byte buffer
// stores straight from the accumulators -- one instruction = two 128-byte row segments, no second image -- came out
// 2-3 us per launch behind in the step and were not consistently ahead of the unpipelined kernel: profiles/linbwd_pipeline_ab.md.)
// Between the next-tile request and its wait (the top of the next tile) the wave issues no vector-memory operation at
// all, so that wait is a plain drain; X of a tile is requested in the accumulator row order (SAMEZ's contraction order)
// through the tile's descriptor, which returns 0 for rows past N (their dZ is 0 and they are kept out of the sums).
// Every fp32 sum keeps the order of the unpipelined form it replaces (gnm_linear_bwd_fused_kernel<2, 2, true, false,
// true, true>, DESIGN_HISTORY.md "Retired variants"): same tiles per wave, same MFMA sequence into wacc, cs1 / cs2 added
// c-major, r ascending -- the results are that kernel's bit for bit.  256 registers, no scratch.
// Not here: the weight gradient on the bf16 pipe (gnm_linear_bwd_rz_kernel's 48 instructions: 84-228 bytes of scratch in
// three arrangements, never launched); the X request in front of the dZ phase (no faster, paired); GNM_LSTAMP stamps
// (their guarded stores turn the counted waits into drains: a stamped build ran 152 us against 94).
// ---------------------------------------------------------------------------------
struct LbSzLds {
    using L = LbLds<2, 2, true, true>;
    static constexpr size_t half_off = L::body;                   // [4 waves][16][XS]
    static constexpr size_t body = L::body + (size_t)4 * 16 * L::XS * 4;
    static constexpr size_t total = body > lb_dump_bytes(2, 2, 4) ? body : lb_dump_bytes(2, 2, 4);
    static_assert(total <= 80 * 1024, "two workgroups share a CU");
};
__global__ void __launch_bounds__(256, 2) gnm_linear_bwd_pipe_sz_kernel(const LbArgs p) {
    constexpr int KT = 2, HT = 2;
    using L = LbLds<KT, HT, true, true>;
    constexpr int KP = L::KP, HP = L::HP, XS = L::XS, EW = L::EW;
    constexpr int H4 = HP / 4;
    constexpr int NLD = (32 * H4) / 64;
    constexpr int RSTEP = 64 / H4;
    constexpr int O4 = KP / 4;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    gnm_u32x4* Wp = reinterpret_cast<gnm_u32x4*>(smem);           // [3][EW] bf16 operand entries of W
    float* Xs_all = reinterpret_cast<float*>(smem + L::xs_off);   // [4][32][XS]
    float* coef = reinterpret_cast<float*>(smem + L::coef_off);   // [5][HP]
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int i = lane & 31, h = lane >> 5;
    float* Xs = Xs_all + wave * 32 * XS;
    float* Hs = reinterpret_cast<float*>(smem + LbSzLds::half_off) + wave * 16 * XS;   // the dX half image
    lin_stage_planes<KT, 32, true, false>(Wp, EW, p.W, p.ldw, 0, tid, 256);
    lb_stage_coef<HP, false>(coef, p.mean, p.rstd, p.cA, p.m1, p.m2, nullptr, tid, 256);
    const int c4 = lane % H4, lrow0 = lane / H4;
    float psc[KT], psh[KT], cmu[KT], crs[KT], cs1[KT], cs2[KT];   // this lane's columns 32b + i: prologue = lower BatchNorm
#pragma unroll
    for (int b = 0; b < KT; ++b) {
        psc[b] = p.pro_scale ? p.pro_scale[32 * b + i] : 1.f;
        psh[b] = p.pro_scale ? p.pro_shift[32 * b + i] : 0.f;
        cmu[b] = p.s_mean[32 * b + i];
        crs[b] = p.s_rstd[32 * b + i];
        cs1[b] = 0.f; cs2[b] = 0.f;
    }
    __builtin_amdgcn_s_waitcnt(0x0F70);           // vmcnt(0): nothing from the preamble is pending inside the tile loop
    __syncthreads();
    f32x16 wacc[HT][KT];
#pragma unroll
    for (int a = 0; a < HT; ++a)
#pragma unroll
        for (int b = 0; b < KT; ++b)
#pragma unroll
            for (int r = 0; r < 16; ++r) wacc[a][b][r] = 0.f;
    float dbacc[HT];
#pragma unroll
    for (int a = 0; a < HT; ++a) dbacc[a] = 0.f;

    const int ntiles = (p.N + 31) / 32;
    const int tstride = gridDim.x * 4;
    const int gz_voff_g = (lrow0 * p.ldg + 4 * c4) * 4, gz_step_g = RSTEP * p.ldg * 4;
    const int gz_voff_z = (lrow0 * p.ldz + 4 * c4) * 4, gz_step_z = RSTEP * p.ldz * 4;
    const int x_voff = (4 * h * p.ldx + i) * 4;                   // X[r0 + (s & 3) + 8 (s >> 2) + 4 h][32 b + i]
    const int out_voff = ((lane / O4) * p.lda + 4 * (lane % O4)) * 4;   // dX: 16-byte chunk lane % O4 of the half image's row lane / O4

    gnm_u32x4 g4[NLD], z4[NLD];
    auto load_gz = [&](int tile) {
        const long long row0 = (long long)tile * 32;
        const long long rows = min((long long)p.N - row0, 32LL);
        const __amdgpu_buffer_rsrc_t rg = gnm_tile_rsrc(p.G + row0 * p.ldg, rows, p.ldg, HP);
        const __amdgpu_buffer_rsrc_t rz = gnm_tile_rsrc(p.Z + row0 * p.ldz, rows, p.ldz, HP);
#pragma unroll
        for (int j = 0; j < NLD; ++j) {
            g4[j] = __builtin_amdgcn_raw_buffer_load_b128(rg, gz_voff_g, j * gz_step_g, kLoadOnce);
            z4[j] = __builtin_amdgcn_raw_buffer_load_b128(rz, gz_voff_z, j * gz_step_z, kLoadOnce);
        }
    };
    auto do_tile = [&](int t, int t_next) {
        const int r0 = t * 32;
        const int rows = min(p.N - r0, 32);
        // ---- 1. dZ tile -> LDS (rows past N are zero: they must not contribute) ----------
        const float4 mu = *reinterpret_cast<const float4*>(coef + 4 * c4);
        const float4 rs = *reinterpret_cast<const float4*>(coef + HP + 4 * c4);
        const float4 ca = *reinterpret_cast<const float4*>(coef + 2 * HP + 4 * c4);
        const float4 a1 = *reinterpret_cast<const float4*>(coef + 3 * HP + 4 * c4);
        const float4 a2 = *reinterpret_cast<const float4*>(coef + 4 * HP + 4 * c4);
#pragma unroll
        for (int j = 0; j < NLD; ++j) {
            const int lrow = lrow0 + j * RSTEP;
            const float4 gj = __builtin_bit_cast(float4, g4[j]), zj = __builtin_bit_cast(float4, z4[j]);
            float4 d;
            d.x = ca.x * (gj.x - a1.x - (zj.x - mu.x) * rs.x * a2.x);
            d.y = ca.y * (gj.y - a1.y - (zj.y - mu.y) * rs.y * a2.y);
            d.z = ca.z * (gj.z - a1.z - (zj.z - mu.z) * rs.z * a2.z);
            d.w = ca.w * (gj.w - a1.w - (zj.w - mu.w) * rs.w * a2.w);
            if (lrow >= rows) d = make_float4(0.f, 0.f, 0.f, 0.f);
            *reinterpret_cast<float4*>(Xs + lrow * XS + 4 * c4) = d;
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        // ---- 2. X of the tile, in the accumulator row order: xv[s] sits on the rows of dacc[.][s]; in flight during dgrad
        float xv[16][KT];
        {
            const __amdgpu_buffer_rsrc_t rx = gnm_tile_rsrc(p.X + (size_t)r0 * p.ldx, rows, p.ldx, KP);
#pragma unroll
            for (int s = 0; s < 16; ++s)
#pragma unroll
                for (int b = 0; b < KT; ++b)
                    xv[s][b] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(
                        rx, x_voff, (((s & 3) + 8 * (s >> 2)) * p.ldx + 32 * b) * 4, 0));
        }
        __builtin_amdgcn_sched_barrier(0);
        // ---- 3. dX = dZ W ------------------------------------------------------------------
        f32x16 dacc[KT];
#pragma unroll
        for (int c = 0; c < KT; ++c)
#pragma unroll
            for (int r = 0; r < 16; ++r) dacc[c][r] = 0.f;
        lin_dgrad_split<KT, HP>(dacc, Xs, XS, Wp, i, h, lane);
        // ---- 4. ReLU mask of the lower BatchNorm and its backward sums on the accumulator, dX out ----------------
        {
            const __amdgpu_buffer_rsrc_t rd = gnm_tile_rsrc(p.dA + (size_t)r0 * p.lda, rows, p.lda, KP);
            auto mask_sum = [&](int c, int r) {
                const float z = xv[r][c];
                float g = dacc[c][r];
                if (z * psc[c] + psh[c] <= 0.f) g = 0.f;
                if ((r & 3) + 8 * (r >> 2) + 4 * h < rows) {
                    cs1[c] += g;
                    cs2[c] += g * ((z - cmu[c]) * crs[c]);
                }
                return g;
            };
#pragma unroll
            for (int q = 0; q < 2; ++q) {                           // accumulator registers 8q .. 8q + 7 are rows 16q .. 16q + 15
                float gq[KT][8];
#pragma unroll
                for (int c = 0; c < KT; ++c)
#pragma unroll
                    for (int r = 0; r < 8; ++r) gq[c][r] = mask_sum(c, 8 * q + r);
#pragma unroll
                for (int c = 0; c < KT; ++c)
#pragma unroll
                    for (int r = 0; r < 8; ++r) Hs[((r & 3) + 8 * (r >> 2) + 4 * h) * XS + 32 * c + i] = gq[c][r];
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
                for (int st = 0; st < (16 * O4) / 64; ++st) {
                    const int idx = lane + 64 * st;
                    const int row = idx / O4, oc = idx - row * O4;
                    const gnm_u32x4 v = *reinterpret_cast<const gnm_u32x4*>(Hs + row * XS + 4 * oc);
                    // (row step in the vector offset: see gnm_lin_stream_kernel)
                    __builtin_amdgcn_raw_buffer_store_b128(v, rd, out_voff + (16 * q + (64 / O4) * st) * p.lda * 4, 0, kStoreStream);
                }
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();          // the half image has been read
            }
        }
        // ---- 5. G and Z of the wave's next tile (past its last tile: empty descriptors, no traffic) ---------------
        // (pinned between the stores and the product: left alone, the scheduler sinks the 16 loads behind the last MFMAs)
        __builtin_amdgcn_sched_barrier(0);
        load_gz(t_next);
        __builtin_amdgcn_sched_barrier(0);
        // ---- 6. dW += dZ^T f(X), db += column sums of dZ -----------------------------------
#pragma unroll
        for (int s = 0; s < 16; ++s) {
            float av[HT];
            const int krow = (s & 3) + 8 * (s >> 2) + 4 * h;
#pragma unroll
            for (int a = 0; a < HT; ++a) av[a] = Xs[krow * XS + 32 * a + i];
            float xf[KT];
#pragma unroll
            for (int b = 0; b < KT; ++b) {
                float x = xv[s][b];
                if (p.pro_scale) {
                    x = x * psc[b] + psh[b];
                    if (p.pro_relu) x = gnm_relu(x);
                }
                xf[b] = x;
            }
#pragma unroll
            for (int a = 0; a < HT; ++a) {
                dbacc[a] += av[a];
#pragma unroll
                for (int b = 0; b < KT; ++b)
                    wacc[a][b] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[a], xf[b], wacc[a][b], 0, 0, 0);
            }
        }
        // ---- 7. everyone is done reading the dZ image ---------------------------------------
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
    };
    {
        int t = lin_first_tile(wave, 1, gridDim.x);
        load_gz(t);
        if (t < ntiles) {
            do_tile(t, t + tstride);                  // peeled
            for (t += tstride; t < ntiles; t += tstride) do_tile(t, t + tstride);
        }
    }

    // ---- lower-BatchNorm sums: the two half-waves hold the same columns, then the 4 waves (fixed order) ----
    __syncthreads();
    double* sred = reinterpret_cast<double*>(smem);               // [4 waves][2][KP]
#pragma unroll
    for (int c = 0; c < KT; ++c) {
        double d1 = (double)cs1[c], d2 = (double)cs2[c];
        d1 += __shfl_xor(d1, 32, 64);
        d2 += __shfl_xor(d2, 32, 64);
        if (h == 0) {
            sred[(wave * 2 + 0) * KP + 32 * c + i] = d1;
            sred[(wave * 2 + 1) * KP + 32 * c + i] = d2;
        }
    }
    __syncthreads();
    for (int idx = tid; idx < 2 * KP; idx += 256) {
        const int which = idx / KP, col = idx - which * KP;
        double sum = 0.0;
        for (int w = 0; w < 4; ++w) sum += sred[(w * 2 + which) * KP + col];
        p.s_partial[((size_t)blockIdx.x * 2 + which) * p.K + col] = sum;
    }

    lb_combine<HT, KT, 1, false>(smem, wacc, dbacc, p.partial, p.H, p.K, 0, tid, lane, wave);
}

static int launch_lb_pipe_sz(const LbArgs& a, int grid, hipStream_t s) {
    const size_t lds = LbSzLds::total;
    GNM_ALLOW_FULL_LDS((&gnm_linear_bwd_pipe_sz_kernel));
    hipLaunchKernelGGL(gnm_linear_bwd_pipe_sz_kernel, dim3(grid), dim3(256), lds, s, a);
    GNM_CHECK_LAUNCH();
    return GNM_OK;
}

template <int KT, int HT, bool STATS, bool NARROW = false, bool SAMEZ = false, bool SPLITD = false>
static int launch_lb(const LbArgs& a, int grid, hipStream_t s) {
    const size_t lds = LbLds<KT, HT, SPLITD, false>::total;
    GNM_ALLOW_FULL_LDS((&gnm_linear_bwd_fused_kernel<KT, HT, STATS, NARROW, SAMEZ, SPLITD>));
    hipLaunchKernelGGL((gnm_linear_bwd_fused_kernel<KT, HT, STATS, NARROW, SAMEZ, SPLITD>), dim3(grid), dim3(256), lds, s, a);
    GNM_CHECK_LAUNCH();
    return GNM_OK;
}

// ---------------------------------------------------------------------------------
// The fused backward of a K = H = 64 Linear WITHOUT the Z stream (round 3).  The kernels above read four [N,64] arrays
// (G, Z, X in; dX out = 420 MB per launch of the headline batch) and Z -- this Linear's own output, needed only for
// xhat = (Z - mean) rstd inside the BatchNorm backward -- is a function of X, which the pass reads anyway for the weight
// gradient: Z = f(X) W^T + b is recomputed on the bf16 matrix pipe with exactly the instruction sequence of
// gnm_lin_split_kernel (48 MFMAs per 32 rows, the same values bit for bit) and a quarter of the traffic is gone.
// (Timing the old kernels with the Z loads stubbed out gave 96.5 -> 85.8 us and 92.5 -> 72.6 us: the bound of this form.)
// What changes around that:
//  * the recomputed Z arrives in the accumulator layout (lane = column, 16 rows in registers), so G is loaded in that
//    layout too (4-byte loads, 128 contiguous bytes per half-wave) and dZ is formed there; the BatchNorm coefficients
//    are per-lane scalars;
//  * the weight-gradient product takes its dZ operand from those registers (no column reads of the LDS image) and its
//    X operand from lane = column loads of the rows in the same order; both are split into three bf16 planes and the
//    product runs as 48 bf16 instructions instead of 64 fp32 ones (a quarter of the matrix-pipe time);
//  * only dgrad still needs the transpose: dZ goes through the wave's LDS image once, row-wise out;
//  * G AND the row-wise X fragments of the wave's next tile are requested before the weight-gradient product (the
//    registers Z used to occupy) -- the statistics form had no room for that in its phase order (its pipelined
//    kernel, gnm_linear_bwd_pipe_sz_kernel, moves the epilogue in front of this product to make it);
//  * eight waves per workgroup share the two weight images (forward orientation for Z, k-major for dgrad: 48 KB) and the
//    workgroup writes TWO rows of partials (waves 0-3, 4-7), so gnm_linear_bwd_grid(N) rows exist as before.
// No lower BatchNorm statistics: the second Linear of an MLP keeps the stored-Z pass, gnm_linear_bwd_pipe_sz_kernel
// (DESIGN_HISTORY.md, "Retired variants").
// ---------------------------------------------------------------------------------
// What gnm_linear_bwd_rz_kernel and its narrow form share beyond the helpers above.
// G of a tile in the accumulator layout (lane = column 32 a + i, rows (r & 3) + 8 (r >> 2) + 4 h): 4-byte loads clipped by
// the tile's descriptor; a tile past the end gets an empty one and no traffic.  AUX: the loads' cache policy (the wide
// kernel reads G once and takes kLoadOnce; on the narrow one that measured a tie and it stays at the default).
template <int AUX>
__device__ __forceinline__ void rz_load_g(float (&g)[2][16], const float* G, int ldg, int N, int tile, int g_voff) {
    const long long row0 = (long long)tile * 32;
    const long long rows = min((long long)N - row0, 32LL);
    const __amdgpu_buffer_rsrc_t rg = gnm_tile_rsrc(G + row0 * ldg, rows, ldg, 64);
#pragma unroll
    for (int r = 0; r < 16; ++r)
#pragma unroll
        for (int a = 0; a < 2; ++a)
            g[a][r] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rg, g_voff + 128 * a, ((r & 3) + 8 * (r >> 2)) * ldg * 4, AUX));
}
// The BatchNorm backward on one column tile of the accumulators (lane = column col): dz holds Z - bias on entry and
// dZ = cA (G - m1 - xhat m2) on exit, zero in rows past `rows`; dZ is also written to the wave's image Xs (for dgrad).
// Returns the lane's column sum of dZ.
__device__ __forceinline__ float rz_bn_bwd(f32x16& dz, const float (&g)[16], const float* coef, int col, int rows, float* Xs,
                                           int xs, int h) {
    const float mu = coef[col], rs = coef[64 + col], ca = coef[128 + col], a1 = coef[192 + col], a2 = coef[256 + col],
                bz = coef[320 + col];
    float dsum = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int lrow = (r & 3) + 8 * (r >> 2) + 4 * h;
        const float z = dz[r] + bz;
        float d = ca * (g[r] - a1 - (z - mu) * rs * a2);
        if (lrow >= rows) d = 0.f;
        dz[r] = d;
        dsum += d;
        Xs[lrow * xs + col] = d;
    }
    return dsum;
}

__global__ void __launch_bounds__(kRzWaves * 64) gnm_linear_bwd_rz_kernel(const LbArgs p) {
    using L = RzLds<false>;
    constexpr int KP = 64, HP = 64, XS = L::XS, EW = 512, NW = kRzWaves, NT = NW * 64;
    static_assert(L::EWF == EW && L::EWB == EW, "both plane images hold 4 m x 2 c x 64 entries");
    extern __shared__ __attribute__((aligned(16))) char smem[];
    gnm_u32x4* Wf = reinterpret_cast<gnm_u32x4*>(smem);                   // [3][EW]: (m, c, lane = 32 kg + n) = W[32c+n][8m+32kg+j]
    gnm_u32x4* Wb = reinterpret_cast<gnm_u32x4*>(smem + L::wb_off);       // [3][EW]: (m, c, lane = 32 kg + n) = W[8m+32kg+j][32c+n]
    float* Xs_all = reinterpret_cast<float*>(smem + L::xs_off);   // [NW][32][XS]
    float* coef = reinterpret_cast<float*>(smem + L::coef_off);   // [6][64]: mean, rstd, cA, m1, m2, bias
    float* psv = reinterpret_cast<float*>(smem + L::psv_off);     // [2][64]: prologue scale, shift
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int i = lane & 31, h = lane >> 5;
    float* Xs = Xs_all + wave * 32 * XS;
    const bool pro = p.pro_scale != nullptr;
    GNM_RSTAMP(0)
    lin_stage_planes<2, 32, false, false>(Wf, EW, p.W, p.ldw, 0, tid, NT);
    lin_stage_planes<2, 32, true, false>(Wb, EW, p.W, p.ldw, 0, tid, NT);
    lb_stage_coef<64, true>(coef, p.mean, p.rstd, p.cA, p.m1, p.m2, p.bias, tid, NT);
    for (int idx = tid; idx < 64; idx += NT) {
        psv[idx] = pro ? p.pro_scale[idx] : 1.f;
        psv[64 + idx] = pro ? p.pro_shift[idx] : 0.f;
    }
    // the wgrad prologue's per-lane scale / shift in registers (256 registers exactly; read from LDS it spilled 34)
    float psc[2], psh[2];
#pragma unroll
    for (int b = 0; b < 2; ++b) {
        psc[b] = pro ? p.pro_scale[32 * b + i] : 1.f;
        psh[b] = pro ? p.pro_shift[32 * b + i] : 0.f;
    }
    __builtin_amdgcn_s_waitcnt(0x0F70);           // vmcnt(0): nothing from the preamble is pending inside the tile loop
    __syncthreads();
    GNM_RSTAMP(1)
    int tk = 0;

    f32x16 wacc[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int r = 0; r < 16; ++r) wacc[a][b][r] = 0.f;
    float dbacc[2] = {0.f, 0.f};

    const int gw = lin_first_tile(wave, NW / 4, p.part_rows);
    const int ntiles = (p.N + 31) / 32;
    const int tstride = p.part_rows * 4;
    const int g_voff = (4 * h * p.ldg + i) * 4;                   // G[row(r, h)][32 a + i], row(r, h) = (r&3) + 8(r>>2) + 4h
    const int xa_voff = (i * p.ldx + 32 * h) * 4;                 // X[i][32 h + 8 m + 0..7]: the forward's A fragments
    const int xc_voff = (4 * h * p.ldx + i) * 4;                  // X[row(r, h)][32 b + i]
    const int out_voff = ((lane >> 4) * p.lda + 4 * (lane & 15)) * 4, out_step = 4 * p.lda * 4;

    float g[2][16];
    gnm_u32x4 xa[4][2];
    auto load_next_x = [&](int tile) {
        const long long row0 = (long long)tile * 32;
        const long long rows = min((long long)p.N - row0, 32LL);
        const __amdgpu_buffer_rsrc_t rx = gnm_tile_rsrc(p.X + row0 * p.ldx, rows, p.ldx, KP);
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            xa[m][0] = __builtin_amdgcn_raw_buffer_load_b128(rx, xa_voff, 32 * m, 0);
            xa[m][1] = __builtin_amdgcn_raw_buffer_load_b128(rx, xa_voff, 32 * m + 16, 0);
        }
    };
    auto do_tile = [&](int t, int t_next) {
        const int r0 = t * 32;
        const int rows = min(p.N - r0, 32);
        GNM_RSTAMP(2 + 6 * min(tk, 9))
        // ---- Z = f(X) W^T (+ bias below): gnm_lin_split_kernel's sequence ------------------------------------
        f32x16 dz[2];
#pragma unroll
        for (int c = 0; c < 2; ++c)
#pragma unroll
            for (int r = 0; r < 16; ++r) dz[c][r] = 0.f;
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            const float4 v0 = __builtin_bit_cast(float4, xa[m][0]), v1 = __builtin_bit_cast(float4, xa[m][1]);
            float f[8] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w};
            if (pro) {
                const int k0 = 32 * h + 8 * m;
#pragma unroll
                for (int q = 0; q < 2; ++q) {
                    const float4 sc = *reinterpret_cast<const float4*>(psv + k0 + 4 * q);
                    const float4 sh = *reinterpret_cast<const float4*>(psv + 64 + k0 + 4 * q);
                    f[4 * q + 0] = f[4 * q + 0] * sc.x + sh.x; f[4 * q + 1] = f[4 * q + 1] * sc.y + sh.y;
                    f[4 * q + 2] = f[4 * q + 2] * sc.z + sh.z; f[4 * q + 3] = f[4 * q + 3] * sc.w + sh.w;
                }
                if (p.pro_relu) {
#pragma unroll
                    for (int j = 0; j < 8; ++j) f[j] = gnm_relu(f[j]);
                }
            }
            gnm_bf16x8 a1, a2, a3;
            gnm_split8(f, a1, a2, a3);
#pragma unroll
            for (int c = 0; c < 2; ++c) gnm_mma6_planes(dz[c], a1, a2, a3, Wf, EW, (m * 2 + c) * 64 + lane);
        }
        GNM_RSTAMP(3 + 6 * min(tk, 9))
        // ---- dZ = cA (G - m1 - xhat m2) on the accumulators; rows past N are zero; image for dgrad ------------
#pragma unroll
        for (int a = 0; a < 2; ++a) dbacc[a] += rz_bn_bwd(dz[a], g[a], coef, 32 * a + i, rows, Xs, XS, h);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        // X in the accumulators' row order (wgrad operand): in flight
        // during the dgrad MFMAs (cache hits: the tile was read row-wise for Z)
        float xv[16][2];
        {
            const __amdgpu_buffer_rsrc_t rx = gnm_tile_rsrc(p.X + (size_t)r0 * p.ldx, rows, p.ldx, KP);
#pragma unroll
            for (int r = 0; r < 16; ++r)
#pragma unroll
                for (int b = 0; b < 2; ++b)
                    xv[r][b] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rx, xc_voff + 128 * b, ((r & 3) + 8 * (r >> 2)) * p.ldx * 4, 0));
        }
        __builtin_amdgcn_sched_barrier(0);
        GNM_RSTAMP(4 + 6 * min(tk, 9))
        // ---- dX = dZ W -------------------------------------------------------------------------------------------
        f32x16 dacc[2];
#pragma unroll
        for (int c = 0; c < 2; ++c)
#pragma unroll
            for (int r = 0; r < 16; ++r) dacc[c][r] = 0.f;
        lin_dgrad_split<2, HP>(dacc, Xs, XS, Wb, i, h, lane);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();          // the dZ image has been read
        GNM_RSTAMP(5 + 6 * min(tk, 9))
        // ---- dX out ------------------------------------------------------------------------------------------------
#pragma unroll
        for (int c = 0; c < 2; ++c)
#pragma unroll
            for (int r = 0; r < 16; ++r) Xs[((r & 3) + 8 * (r >> 2) + 4 * h) * XS + 32 * c + i] = dacc[c][r];
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        {
            const __amdgpu_buffer_rsrc_t rd = gnm_tile_rsrc(p.dA + (size_t)r0 * p.lda, rows, p.lda, KP);
#pragma unroll
            for (int st = 0; st < 8; ++st) {
                const int idx = lane + 64 * st;
                const int row = idx >> 4, oc = idx & 15;
                const gnm_u32x4 v = *reinterpret_cast<const gnm_u32x4*>(Xs + row * XS + 4 * oc);
                __builtin_amdgcn_raw_buffer_store_b128(v, rd, out_voff + st * out_step, 0, kStoreStream);
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        GNM_RSTAMP(6 + 6 * min(tk, 9))
        // the next tile: G and the row-wise X fragments before the weight-gradient product
        rz_load_g<kLoadOnce>(g, p.G, p.ldg, p.N, t_next, (int)g_voff);                      // past the wave's last tile: empty descriptors, no traffic
        load_next_x(t_next);
        // ---- dW += dZ^T f(X): both operands from registers, batch rows in the accumulators' order ---------------------
#pragma unroll
        for (int m = 0; m < 2; ++m) {
            gnm_bf16x8 dp[2][3], xp[2][3];
#pragma unroll
            for (int a = 0; a < 2; ++a) {
                float f[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) f[j] = dz[a][8 * m + j];
                gnm_split8(f, dp[a][0], dp[a][1], dp[a][2]);
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    float x = xv[8 * m + j][a];
                    if (pro) {
                        x = x * psc[a] + psh[a];
                        if (p.pro_relu) x = gnm_relu(x);
                    }
                    f[j] = x;
                }
                gnm_split8(f, xp[a][0], xp[a][1], xp[a][2]);
            }
#pragma unroll
            for (int a = 0; a < 2; ++a)
#pragma unroll
                for (int b = 0; b < 2; ++b) gnm_mma6(wacc[a][b], dp[a][0], dp[a][1], dp[a][2], xp[b][0], xp[b][1], xp[b][2]);
        }
        GNM_RSTAMP(7 + 6 * min(tk, 9))
        ++tk;
    };
    {
        int t = gw;
        load_next_x(t);
        rz_load_g<kLoadOnce>(g, p.G, p.ldg, p.N, t, (int)g_voff);
        if (t < ntiles) {
            do_tile(t, t + tstride);                  // peeled (see gnm_linear_bwd_pipe_kernel)
            for (t += tstride; t < ntiles; t += tstride) do_tile(t, t + tstride);
        }
    }
    __builtin_amdgcn_s_waitcnt(0x0F70);
    GNM_RSTAMP(62)

    lb_combine<2, 2, 2, false>(smem, wacc, dbacc, p.partial, HP, KP, p.part_rows, tid, lane, wave);
    GNM_RSTAMP(63)
}

static int launch_lb_rz(const LbArgs& a, int grid, hipStream_t s) {
    const size_t lds = RzLds<false>::total;
    GNM_ALLOW_FULL_LDS((&gnm_linear_bwd_rz_kernel));
    hipLaunchKernelGGL(gnm_linear_bwd_rz_kernel, dim3((grid + 1) / 2), dim3(kRzWaves * 64), lds, s, a);
    GNM_CHECK_LAUNCH();
    return GNM_OK;
}

// ---------------------------------------------------------------------------------
// gnm_linear_bwd_rz_kernel for a NARROW input (K <= 16: the first Linear of the input layer, K = F0 = 7 in the benchmark),
// H = 64, no lower BatchNorm.  The Z-reading narrow form moves G and Z (210 MB at the headline batch) for an input that
// is 11 MB; here Z = X W^T + b is one 16-wide MFMA step per column tile, the weight gradient [64 x K] is one column tile
// (32 accumulators) and dX [32 x K] one: G is the only large stream.  Same structure as the K = 64 kernel (eight waves,
// two rows of partials per workgroup, G of the next tile requested before the weight-gradient product); X and dX rows
// are K floats wide and not 16-byte addressable: 4-byte accesses, clipped by their buffer descriptors.
// ---------------------------------------------------------------------------------
__global__ void __launch_bounds__(kRzWaves * 64) gnm_linear_bwd_rzn_kernel(const LbArgs p) {
    using L = RzLds<true>;
    constexpr int HP = 64, XS = L::XS, NW = kRzWaves, NT = NW * 64, TILE = 16 * 64;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    gnm_u32x4* Wf = reinterpret_cast<gnm_u32x4*>(smem);                   // [3][2 c][64]: (c, lane = 32 kg + n) = W[32c+n][8kg+j], k < K
    gnm_u32x4* Wb = reinterpret_cast<gnm_u32x4*>(smem + L::wb_off);       // [3][4 m][64]: (m, lane = 32 kg + n) = W[8m+32kg+j][n], n < K
    float* Xs_all = reinterpret_cast<float*>(smem + L::xs_off);   // [NW][32][XS]
    float* coef = reinterpret_cast<float*>(smem + L::coef_off);   // [6][64]: mean, rstd, cA, m1, m2, bias
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int i = lane & 31, h = lane >> 5;
    float* Xs = Xs_all + wave * 32 * XS;
    const int K = p.K;
    lin_stage_planes<2, 8, false, true>(Wf, L::EWF, p.W, p.ldw, K, tid, NT);
    lin_stage_planes<1, 32, true, true>(Wb, L::EWB, p.W, p.ldw, K, tid, NT);
    lb_stage_coef<64, true>(coef, p.mean, p.rstd, p.cA, p.m1, p.m2, p.bias, tid, NT);
    __builtin_amdgcn_s_waitcnt(0x0F70);
    __syncthreads();

    f32x16 wacc[2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int r = 0; r < 16; ++r) wacc[a][r] = 0.f;
    float dbacc[2] = {0.f, 0.f};
    const int gw = lin_first_tile(wave, NW / 4, p.part_rows);
    const int ntiles = (p.N + 31) / 32;
    const int tstride = p.part_rows * 4;
    const unsigned g_voff = (unsigned)((4 * h * p.ldg + i) * 4);
    const unsigned kclip = 0x80000000u;                           // past any buffer, no wrap with the row offsets
    const unsigned xc_voff = i < K ? (unsigned)((4 * h * p.ldx + i) * 4) : kclip;     // X[row(r, h)][i]
    const unsigned da_voff = i < K ? (unsigned)((4 * h * p.lda + i) * 4) : kclip;     // dX[row(r, h)][i]

    float g[2][16];
    auto do_tile = [&](int t, int t_next) {
        const int r0 = t * 32;
        const int rows = min(p.N - r0, 32);
        const __amdgpu_buffer_rsrc_t rx = gnm_tile_rsrc(p.X + (size_t)r0 * p.ldx, rows, p.ldx, K);
        // ---- Z = X W^T: one step of 16 (zero past K) -------------------------------------------------------------
        float fx[8];
#pragma unroll
        for (int j = 0; j < 8; ++j)
            fx[j] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(
                rx, 8 * h + j < K ? (unsigned)((i * p.ldx + 8 * h + j) * 4) : kclip, 0, 0));
        float xv[16];                             // X in the accumulators' row order, column i: the wgrad operand
#pragma unroll
        for (int r = 0; r < 16; ++r)
            xv[r] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rx, xc_voff, ((r & 3) + 8 * (r >> 2)) * p.ldx * 4, 0));
        f32x16 dz[2];
#pragma unroll
        for (int c = 0; c < 2; ++c)
#pragma unroll
            for (int r = 0; r < 16; ++r) dz[c][r] = 0.f;
        {
            gnm_bf16x8 a1, a2, a3;
            gnm_split8(fx, a1, a2, a3);
#pragma unroll
            for (int c = 0; c < 2; ++c) gnm_mma6_planes(dz[c], a1, a2, a3, Wf, L::EWF, c * 64 + lane);
        }
        // ---- dZ = cA (G - m1 - xhat m2) on the accumulators; image for dgrad -----------------------------------------
#pragma unroll
        for (int a = 0; a < 2; ++a) dbacc[a] += rz_bn_bwd(dz[a], g[a], coef, 32 * a + i, rows, Xs, XS, h);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        // ---- dX = dZ W: one column tile (columns past K are zero and not stored) ------------------------------------
        if (p.dA) {
            f32x16 dacc[1];
#pragma unroll
            for (int r = 0; r < 16; ++r) dacc[0][r] = 0.f;
            lin_dgrad_split<1, HP>(dacc, Xs, XS, Wb, i, h, lane);
            const __amdgpu_buffer_rsrc_t rd = gnm_tile_rsrc(p.dA + (size_t)r0 * p.lda, rows, p.lda, K);
#pragma unroll
            for (int r = 0; r < 16; ++r)
                __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(dacc[0][r]), rd, da_voff, ((r & 3) + 8 * (r >> 2)) * p.lda * 4, 0);
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();          // the dZ image has been read
        rz_load_g<0>(g, p.G, p.ldg, p.N, t_next, (int)g_voff);                      // past the wave's last tile: empty descriptors, no traffic
        // ---- dW += dZ^T X: both operands from registers, batch rows in the accumulators' order -----------------------
#pragma unroll
        for (int m = 0; m < 2; ++m) {
            float f[8];
            gnm_bf16x8 x1, x2, x3, d1, d2, d3;
#pragma unroll
            for (int j = 0; j < 8; ++j) f[j] = xv[8 * m + j];
            gnm_split8(f, x1, x2, x3);
#pragma unroll
            for (int a = 0; a < 2; ++a) {
#pragma unroll
                for (int j = 0; j < 8; ++j) f[j] = dz[a][8 * m + j];
                gnm_split8(f, d1, d2, d3);
                gnm_mma6(wacc[a], d1, d2, d3, x1, x2, x3);
            }
        }
    };
    {
        int t = gw;
        rz_load_g<0>(g, p.G, p.ldg, p.N, t, (int)g_voff);
        if (t < ntiles) {
            do_tile(t, t + tstride);
            for (t += tstride; t < ntiles; t += tstride) do_tile(t, t + tstride);
        }
    }
    __builtin_amdgcn_s_waitcnt(0x0F70);
    // ---- dW [64 x K] / db: the waves of each half in a fixed order (lb_combine<2, 1, 2, true>, spelled out: through the
    //      helper hipcc of ROCm 7.2 moved an MFMA inside this kernel's tile loop; fold it in when the toolchain changes) ----
    __syncthreads();
    float* dump = reinterpret_cast<float*>(smem);                 // [NW][2][16][64] + [NW][2][64]
    float* mine = dump + (size_t)wave * 2 * TILE;
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int r = 0; r < 16; ++r) mine[a * TILE + r * 64 + lane] = wacc[a][r];
    float* dbdump = dump + (size_t)NW * 2 * TILE;
#pragma unroll
    for (int a = 0; a < 2; ++a) dbdump[(wave * 2 + a) * 64 + lane] = dbacc[a];
    __syncthreads();
    const size_t pstride = (size_t)HP * K + HP;
    for (int idx = tid; idx < 2 * 2 * TILE; idx += NT) {
        const int grp = idx / (2 * TILE), rem = idx - grp * 2 * TILE;
        const int prow = blockIdx.x * 2 + grp;
        if (prow >= p.part_rows) continue;
        const int a = rem / TILE;
        const int rl = rem - a * TILE;
        const int r = rl >> 6, ln = rl & 63;
        const int row = 32 * a + (r & 3) + 8 * (r >> 2) + 4 * (ln >> 5);
        const int col = ln & 31;
        if (col >= K) continue;
        float sum = 0.f;
#pragma unroll
        for (int w = 0; w < 4; ++w) sum += dump[(size_t)(4 * grp + w) * 2 * TILE + rem];
        p.partial[(size_t)prow * pstride + (size_t)row * K + col] = sum;
    }
    for (int idx = tid; idx < 2 * 64; idx += NT) {
        const int grp = idx >> 6, a = (idx >> 5) & 1, ii = idx & 31;
        const int prow = blockIdx.x * 2 + grp;
        if (prow >= p.part_rows) continue;
        float sum = 0.f;
#pragma unroll
        for (int w = 0; w < 4; ++w) sum += dbdump[((4 * grp + w) * 2 + a) * 64 + ii] + dbdump[((4 * grp + w) * 2 + a) * 64 + 32 + ii];
        p.partial[(size_t)prow * pstride + (size_t)HP * K + 32 * a + ii] = sum;
    }
}

static int launch_lb_rzn(const LbArgs& a, int grid, hipStream_t s) {
    const size_t lds = RzLds<true>::total;
    GNM_ALLOW_FULL_LDS((&gnm_linear_bwd_rzn_kernel));
    hipLaunchKernelGGL(gnm_linear_bwd_rzn_kernel, dim3((grid + 1) / 2), dim3(kRzWaves * 64), lds, s, a);
    GNM_CHECK_LAUNCH();
    return GNM_OK;
}

extern "C" int gnm_linear_bwd_grid(int N) {
    int g = ((N + 31) / 32 + 3) / 4;
    static const int cap = gnm_env_int("GNM_LINBWD_GRID", 512);   // tuning knob
    if (g > cap) g = cap;
    return g < 1 ? 1 : g;
}
extern "C" long long gnm_linear_bwd_workspace_floats(int N, int H, int K) {
    return (long long)gnm_linear_bwd_grid(N) * ((long long)H * K + H);
}

// Returns GNM_ERR_UNSUPPORTED (and launches nothing) when the shape/alignment is not
// eligible; the caller then uses gnm_bn_bwd_apply + gnm_linear_wgrad + gnm_linear_fwd.
extern "C" int gnm_linear_bwd_fused(const float* G, int ldg, const float* Z, int ldz, const float* mean,
                                    const float* rstd, const float* cA, const float* m1, const float* m2,
                                    const float* X, int ldx, const float* pro_scale, const float* pro_shift,
                                    int pro_relu, const float* W, int ldw, float* dA, int lda, float* dW, int lddw,
                                    float* db, float* workspace, int N, int K, int H, const float* sZ, int ldsz,
                                    const float* s_scale, const float* s_shift, const float* s_mean,
                                    const float* s_rstd, double* s_partial, void* stream) {
    if (N <= 0) return GNM_ERR_UNSUPPORTED;
    const bool narrow = K >= 1 && K < 32 && !sZ;            // zero-padded single K tile, scalar X / dX accesses
    if ((K != 32 && K != 64 && !narrow) || (H != 32 && H != 64)) return GNM_ERR_UNSUPPORTED;
    if ((ldg & 3) || (ldz & 3) || (dA && !narrow && (lda & 3)) || lin_force_generic()) return GNM_ERR_UNSUPPORTED;
    const uintptr_t al = reinterpret_cast<uintptr_t>(G) | reinterpret_cast<uintptr_t>(Z) |
                         (narrow ? 0 : reinterpret_cast<uintptr_t>(dA)) | reinterpret_cast<uintptr_t>(mean) |
                         reinterpret_cast<uintptr_t>(rstd) | reinterpret_cast<uintptr_t>(cA) |
                         reinterpret_cast<uintptr_t>(m1) | reinterpret_cast<uintptr_t>(m2);
    if (al & 15) return GNM_ERR_UNSUPPORTED;
    if (sZ) {
        if (!dA || !s_partial || (ldsz & 3)) return GNM_ERR_BAD_ARG;
        const uintptr_t al2 = reinterpret_cast<uintptr_t>(sZ) | reinterpret_cast<uintptr_t>(s_scale) |
                              reinterpret_cast<uintptr_t>(s_shift) | reinterpret_cast<uintptr_t>(s_mean) |
                              reinterpret_cast<uintptr_t>(s_rstd);
        if (al2 & 15) return GNM_ERR_UNSUPPORTED;
    }
    LbArgs a = lb_args(G, ldg, mean, rstd, cA, m1, m2, X, ldx, pro_scale, pro_shift, pro_relu, W, ldw, dA, lda, workspace,
                       N, K, H, sZ, ldsz, s_scale, s_shift, s_mean, s_rstd, s_partial);
    a.Z = Z; a.ldz = ldz;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const int grid = gnm_linear_bwd_grid(N);
    int rc = GNM_ERR_UNSUPPORTED;
    const int KT = narrow ? 0 : K / 32, HT = H / 32;
    // no statistics to reduce (the first Linear of an MLP): the cross-tile pipelined kernel
    if (!narrow && !sZ) {
        if (KT == 1 && HT == 1) rc = launch_lb_pipe<1, 1>(a, grid, s);
        if (KT == 2 && HT == 1) rc = launch_lb_pipe<2, 1>(a, grid, s);
        if (KT == 1 && HT == 2) rc = launch_lb_pipe<1, 2>(a, grid, s);
        if (KT == 2 && HT == 2) rc = lin_no_split() ? launch_lb_pipe<2, 2>(a, grid, s) : launch_lb_pipe<2, 2, true>(a, grid, s);
    }
    if (narrow && HT == 1) rc = launch_lb<1, 1, false, true>(a, grid, s);
    if (narrow && HT == 2)
        rc = lin_no_split() ? launch_lb<1, 2, false, true>(a, grid, s) : launch_lb<1, 2, false, true, false, true>(a, grid, s);
    if (sZ && KT == 1 && HT == 1) rc = launch_lb<1, 1, true>(a, grid, s);
    if (sZ && KT == 2 && HT == 1) rc = launch_lb<2, 1, true>(a, grid, s);
    if (sZ && KT == 1 && HT == 2) rc = launch_lb<1, 2, true>(a, grid, s);
    // the second Linear of an MLP: the lower BatchNorm's input is this Linear's input and its affine is the prologue
    const bool samez = sZ && sZ == X && ldsz == ldx && s_scale == pro_scale && s_shift == pro_shift && pro_relu;
    if (sZ && KT == 2 && HT == 2)
        rc = samez ? (lin_no_split() ? launch_lb<2, 2, true, false, true>(a, grid, s) : launch_lb_pipe_sz(a, grid, s))
                   : launch_lb<2, 2, true>(a, grid, s);
    if (rc != GNM_OK || !dW) return rc;      // dW = NULL: the partials stay in `workspace` for gnm_reduce_partials_multi
    return gnm_reduce_partials(workspace, grid, H, K, 0, dW, lddw, db, s);
}

// gnm_linear_bwd_fused for a Linear whose output Z the caller does NOT pass: Z = f(X) W^T + bias is recomputed
// (gnm_linear_bwd_rz_kernel).  K = H = 64 with dA wanted and no lower BatchNorm (sZ = NULL: the first Linear of the
// headline model's MLPs), or the input layer's narrow first Linear; anything else, every sZ != NULL included, returns
// GNM_ERR_UNSUPPORTED and the caller takes gnm_linear_bwd_fused with the stored Z.  Workspace, partial rows and the
// deferred reduction (dW = NULL) are those of gnm_linear_bwd_fused.
extern "C" int gnm_linear_bwd_fused_rz(const float* G, int ldg, const float* bias, const float* mean, const float* rstd,
                                       const float* cA, const float* m1, const float* m2, const float* X, int ldx,
                                       const float* pro_scale, const float* pro_shift, int pro_relu, const float* W,
                                       int ldw, float* dA, int lda, float* dW, int lddw, float* db, float* workspace,
                                       int N, int K, int H, const float* sZ, int ldsz, const float* s_scale,
                                       const float* s_shift, const float* s_mean, const float* s_rstd,
                                       double* s_partial, void* stream) {
    // (a form with the lower BatchNorm's statistics measured behind the stored-Z kernel: DESIGN_HISTORY.md, "Retired variants")
    if (sZ) return GNM_ERR_UNSUPPORTED;
    const bool narrow = K >= 1 && K <= 16 && !pro_scale;    // the input layer's first Linear (one 16-wide step of Z): gnm_linear_bwd_rzn_kernel
    if (N <= 0 || (K != 64 && !narrow) || H != 64 || (!dA && !narrow) || lin_force_generic() || lin_no_split())
        return GNM_ERR_UNSUPPORTED;
    if (!narrow && ((ldx & 3) || (lda & 3))) return GNM_ERR_UNSUPPORTED;
    if (!narrow && ((reinterpret_cast<uintptr_t>(X) | reinterpret_cast<uintptr_t>(dA)) & 15)) return GNM_ERR_UNSUPPORTED;
    if ((long long)32 * (ldg > ldx ? (ldg > lda ? ldg : lda) : (ldx > lda ? ldx : lda)) * 4 >= (1LL << 31)) return GNM_ERR_UNSUPPORTED;
    LbArgs a = lb_args(G, ldg, mean, rstd, cA, m1, m2, X, ldx, pro_scale, pro_shift, pro_relu, W, ldw, dA, lda, workspace,
                       N, K, H, sZ, ldsz, s_scale, s_shift, s_mean, s_rstd, s_partial);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const int grid = gnm_linear_bwd_grid(N);
    a.bias = bias; a.part_rows = grid;
    const int rc = narrow ? launch_lb_rzn(a, grid, s) : launch_lb_rz(a, grid, s);
    if (rc != GNM_OK || !dW) return rc;
    return gnm_reduce_partials(workspace, grid, H, K, 0, dW, lddw, db, s);
}
