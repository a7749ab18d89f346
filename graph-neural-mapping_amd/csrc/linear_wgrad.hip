// The weight gradient of nn.Linear (dW = dZ^T f(X), db = sum dZ: the second backward product autograd derives, see
// linear.hip) as per-workgroup partials, and the reductions that sum partials in a fixed order -- gnm_linear_wgrad's
// own and those of the fused backward kernels of linear_bwd.hip.
#include "gnm_linear.h"

extern "C" int gnm_linear_bwd_grid(int N);       // linear_bwd.hip: the partial rows a fused backward launch writes

// ------------------------------------------------------------------------------
// weight gradient: dW[h][k] = sum_n dZ[n][h] * f(X)[n][k],  db[h] = sum_n dZ[n][h]
// MFMA 32x32x2 with the batch row as the contraction index: lane (i, half) feeds
// A = dZ[n+half][32*ti+i] and B = f(X)[n+half][32*tj+i] straight from global memory
// (128-B contiguous per half-wave).  Each block reduces its row range to one
// [H x KW] partial; gnm_reduce_partials sums the partials in a fixed order.
// ------------------------------------------------------------------------------
struct WgArgs {
    const float* dZ;
    const float* X;
    const float* pro_scale;  // [K] or null
    const float* pro_shift;
    float* partial;          // [gridDim.x][H*kw + H]
    int ldd, ldx;
    int N, H, K;
    int k0, kw;              // column window of X handled by this launch (kw <= 128)
    int rows_per_block;      // even
    int pro_relu;
};

template <int WI, int WJ, int QI, int QJ>
__global__ void __launch_bounds__(256) gnm_wgrad_kernel(const WgArgs p) {
    constexpr int NQ = QI * QJ;          // quadrants of the output, one per wave group
    constexpr int RSPLIT = 4 / NQ;       // waves sharing a quadrant split the rows
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* dump = reinterpret_cast<float*>(smem);   // [4][WI*WJ][16][64] (+ db [4][WI][64])
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int i = lane & 31, h = lane >> 5;
    const int q = wave % NQ, rs = wave / NQ;
    const int qi = q / QJ, qj = q % QJ;

    f32x16 acc[WI][WJ];
#pragma unroll
    for (int a = 0; a < WI; ++a)
#pragma unroll
        for (int b = 0; b < WJ; ++b)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;
    float dbacc[WI];
#pragma unroll
    for (int a = 0; a < WI; ++a) dbacc[a] = 0.f;

    int hcol[WI], kcol[WJ];
    bool hok[WI], kok[WJ];
    float sc[WJ], sh[WJ];
#pragma unroll
    for (int a = 0; a < WI; ++a) { hcol[a] = 32 * (qi * WI + a) + i; hok[a] = hcol[a] < p.H; }
#pragma unroll
    for (int b = 0; b < WJ; ++b) {
        const int kl = 32 * (qj * WJ + b) + i;       // column inside the window
        kcol[b] = p.k0 + kl;
        kok[b] = (kl < p.kw) && (kcol[b] < p.K);
        sc[b] = (p.pro_scale && kok[b]) ? p.pro_scale[kcol[b]] : 1.f;
        sh[b] = (p.pro_scale && kok[b]) ? p.pro_shift[kcol[b]] : 0.f;
    }

    const int rb = blockIdx.x * p.rows_per_block;
    const int re = min(p.N, rb + p.rows_per_block);
#pragma unroll 4
    for (int n0 = rb + 2 * rs; n0 < re; n0 += 2 * RSPLIT) {
        const int n = n0 + h;
        const bool rok = n < re;
        float av[WI], bv[WJ];
#pragma unroll
        for (int a = 0; a < WI; ++a) av[a] = (rok && hok[a]) ? p.dZ[(size_t)n * p.ldd + hcol[a]] : 0.f;
#pragma unroll
        for (int b = 0; b < WJ; ++b) {
            float x = 0.f;
            if (rok && kok[b]) {
                x = p.X[(size_t)n * p.ldx + kcol[b]];
                if (p.pro_scale) {
                    x = x * sc[b] + sh[b];
                    if (p.pro_relu) x = gnm_relu(x);
                }
            }
            bv[b] = x;
        }
#pragma unroll
        for (int a = 0; a < WI; ++a) {
            dbacc[a] += av[a];
#pragma unroll
            for (int b = 0; b < WJ; ++b)
                acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[a], bv[b], acc[a][b], 0, 0, 0);
        }
    }

    // ---- dump per-wave accumulators, then combine waves in a fixed order ---------
    constexpr int TILE = 16 * 64;
    float* mine = dump + (size_t)wave * WI * WJ * TILE;
#pragma unroll
    for (int a = 0; a < WI; ++a)
#pragma unroll
        for (int b = 0; b < WJ; ++b)
#pragma unroll
            for (int r = 0; r < 16; ++r) mine[(a * WJ + b) * TILE + r * 64 + lane] = acc[a][b][r];
    float* dbdump = dump + (size_t)4 * WI * WJ * TILE;   // [4][WI][64]
#pragma unroll
    for (int a = 0; a < WI; ++a) dbdump[(wave * WI + a) * 64 + lane] = dbacc[a];
    __syncthreads();

    float* out = p.partial + (size_t)blockIdx.x * ((size_t)p.H * p.kw + p.H);
    for (int idx = tid; idx < NQ * WI * WJ * TILE; idx += 256) {
        const int qq = idx / (WI * WJ * TILE);
        const int rem = idx - qq * (WI * WJ * TILE);
        const int ab = rem / TILE;
        const int rl = rem - ab * TILE;
        const int r = rl >> 6, ln = rl & 63;
        const int a = ab / WJ, b = ab - a * WJ;
        const int row = 32 * ((qq / QJ) * WI + a) + (r & 3) + 8 * (r >> 2) + 4 * (ln >> 5);
        const int colw = 32 * ((qq % QJ) * WJ + b) + (ln & 31);
        if (row < p.H && colw < p.kw) {
            float s = 0.f;
#pragma unroll
            for (int w = 0; w < RSPLIT; ++w) s += dump[(size_t)(w * NQ + qq) * WI * WJ * TILE + rem];
            out[(size_t)row * p.kw + colw] = s;
        }
    }
    // bias gradient: only the qj == 0 quadrants hold each dZ column exactly once
    for (int idx = tid; idx < QI * WI * 32; idx += 256) {
        const int qqi = idx / (WI * 32);
        const int rem = idx - qqi * (WI * 32);
        const int a = rem >> 5, ii = rem & 31;
        const int hh = 32 * (qqi * WI + a) + ii;
        if (hh < p.H) {
            float s = 0.f;
            const int qq = qqi * QJ;     // qj == 0
#pragma unroll
            for (int w = 0; w < RSPLIT; ++w) {
                const int wv = w * NQ + qq;
                s += dbdump[(wv * WI + a) * 64 + ii] + dbdump[(wv * WI + a) * 64 + 32 + ii];
            }
            out[(size_t)p.H * p.kw + hh] = s;
        }
    }
}

// Pipelined wgrad for H % 32 == 0 and K-window % 32 == 0: no column guards, rows clamped on
// load and zeroed by select, and U row-pairs (U*(WI+WJ) loads) in flight before their MFMAs.
// The generic kernel above waits for every pair's 4 loads before its 4 MFMAs.
template <int WI, int WJ, int QI, int QJ>
__global__ void __launch_bounds__(256) gnm_wgrad_fast_kernel(const WgArgs p) {
    constexpr int NQ = QI * QJ;
    constexpr int RSPLIT = 4 / NQ;
    constexpr int U = 8;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* dump = reinterpret_cast<float*>(smem);
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int i = lane & 31, h = lane >> 5;
    const int q = wave % NQ, rs = wave / NQ;
    const int qi = q / QJ, qj = q % QJ;

    f32x16 acc[WI][WJ];
#pragma unroll
    for (int a = 0; a < WI; ++a)
#pragma unroll
        for (int b = 0; b < WJ; ++b)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;
    float dbacc[WI];
    int hcol[WI], kcol[WJ];
    bool kok[WJ];                 // columns past the window / K are clamped on load and zeroed by select
    float sc[WJ], sh[WJ];
#pragma unroll
    for (int a = 0; a < WI; ++a) {
        dbacc[a] = 0.f;
        hcol[a] = 32 * (qi * WI + a) + i;
        // Two row quadrants of an odd number of 32-column tiles (H = 96): quadrant 1's second tile lies past H, and in the
        // last row its loads would leave dZ.  Clamped like kcol; none of that tile's accumulators is written out below.
        // With one quadrant the WI tiles are exactly H, and those instances keep the unclamped index.
        if constexpr (QI > 1) hcol[a] = min(hcol[a], p.H - 1);
    }
#pragma unroll
    for (int b = 0; b < WJ; ++b) {
        const int kl = 32 * (qj * WJ + b) + i;
        kok[b] = (kl < p.kw) && (p.k0 + kl < p.K);
        kcol[b] = min(p.k0 + kl, p.K - 1);
        sc[b] = p.pro_scale ? p.pro_scale[kcol[b]] : 1.f;
        sh[b] = p.pro_scale ? p.pro_shift[kcol[b]] : 0.f;
    }
    const int rb = blockIdx.x * p.rows_per_block;
    const int re = min(p.N, rb + p.rows_per_block);
    const int nlast = p.N - 1;
    for (int n0 = rb + 2 * rs; n0 < re; n0 += 2 * RSPLIT * U) {
        float av[U][WI], bv[U][WJ];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int n = n0 + u * 2 * RSPLIT + h;
            const int nc = min(n, nlast);
#pragma unroll
            for (int a = 0; a < WI; ++a) av[u][a] = p.dZ[(size_t)nc * p.ldd + hcol[a]];
#pragma unroll
            for (int b = 0; b < WJ; ++b) bv[u][b] = p.X[(size_t)nc * p.ldx + kcol[b]];
        }
        __builtin_amdgcn_sched_barrier(0);     // keep all U*(WI+WJ) loads ahead of the MFMAs
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const bool rok = (n0 + u * 2 * RSPLIT + h) < re;
#pragma unroll
            for (int b = 0; b < WJ; ++b) {
                float x = bv[u][b];
                if (p.pro_scale) {
                    x = x * sc[b] + sh[b];
                    if (p.pro_relu) x = gnm_relu(x);
                }
                bv[u][b] = (rok && kok[b]) ? x : 0.f;
            }
#pragma unroll
            for (int a = 0; a < WI; ++a) {
                const float d = rok ? av[u][a] : 0.f;
                dbacc[a] += d;
#pragma unroll
                for (int b = 0; b < WJ; ++b)
                    acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x2f32(d, bv[u][b], acc[a][b], 0, 0, 0);
            }
        }
    }

    constexpr int TILE = 16 * 64;
    float* mine = dump + (size_t)wave * WI * WJ * TILE;
#pragma unroll
    for (int a = 0; a < WI; ++a)
#pragma unroll
        for (int b = 0; b < WJ; ++b)
#pragma unroll
            for (int r = 0; r < 16; ++r) mine[(a * WJ + b) * TILE + r * 64 + lane] = acc[a][b][r];
    float* dbdump = dump + (size_t)4 * WI * WJ * TILE;
#pragma unroll
    for (int a = 0; a < WI; ++a) dbdump[(wave * WI + a) * 64 + lane] = dbacc[a];
    __syncthreads();

    float* out = p.partial + (size_t)blockIdx.x * ((size_t)p.H * p.kw + p.H);
    for (int idx = tid; idx < NQ * WI * WJ * TILE; idx += 256) {
        const int qq = idx / (WI * WJ * TILE);
        const int rem = idx - qq * (WI * WJ * TILE);
        const int ab = rem / TILE;
        const int rl = rem - ab * TILE;
        const int r = rl >> 6, ln = rl & 63;
        const int a = ab / WJ, b = ab - a * WJ;
        const int row = 32 * ((qq / QJ) * WI + a) + (r & 3) + 8 * (r >> 2) + 4 * (ln >> 5);
        const int colw = 32 * ((qq % QJ) * WJ + b) + (ln & 31);
        if (row < p.H && colw < p.kw) {
            float s = 0.f;
#pragma unroll
            for (int w = 0; w < RSPLIT; ++w) s += dump[(size_t)(w * NQ + qq) * WI * WJ * TILE + rem];
            out[(size_t)row * p.kw + colw] = s;
        }
    }
    for (int idx = tid; idx < QI * WI * 32; idx += 256) {
        const int qqi = idx / (WI * 32);
        const int rem = idx - qqi * (WI * 32);
        const int a = rem >> 5, ii = rem & 31;
        const int hh = 32 * (qqi * WI + a) + ii;
        if (hh < p.H) {
            float s = 0.f;
            const int qq = qqi * QJ;
#pragma unroll
            for (int w = 0; w < RSPLIT; ++w) {
                const int wv = w * NQ + qq;
                s += dbdump[(wv * WI + a) * 64 + ii] + dbdump[(wv * WI + a) * 64 + 32 + ii];
            }
            out[(size_t)p.H * p.kw + hh] = s;
        }
    }
}

template <int WI, int WJ, int QI, int QJ>
static int launch_wgrad_fast(const WgArgs& a, int grid, hipStream_t s) {
    const size_t lds = ((size_t)4 * WI * WJ * 1024 + (size_t)4 * WI * 64) * 4;
    GNM_ALLOW_FULL_LDS((&gnm_wgrad_fast_kernel<WI, WJ, QI, QJ>));
    hipLaunchKernelGGL((gnm_wgrad_fast_kernel<WI, WJ, QI, QJ>), dim3(grid), dim3(256), lds, s, a);
    GNM_CHECK_LAUNCH();
    return GNM_OK;
}

template <int WI, int WJ, int QI, int QJ>
static int launch_wgrad(const WgArgs& a, int grid, hipStream_t s) {
    const size_t lds = ((size_t)4 * WI * WJ * 1024 + (size_t)4 * WI * 64) * 4;
    GNM_ALLOW_FULL_LDS((&gnm_wgrad_kernel<WI, WJ, QI, QJ>));
    hipLaunchKernelGGL((gnm_wgrad_kernel<WI, WJ, QI, QJ>), dim3(grid), dim3(256), lds, s, a);
    GNM_CHECK_LAUNCH();
    return GNM_OK;
}

// ---------------------------------------------------------------------------------
// K = H = 128 weight gradient on the bf16 matrix pipe (round 3: the hidden Linears of BASELINE configs[3]; the fp32
// instruction kernel above runs this shape at 124 us per 256,000 rows with one wave per SIMD).  The contraction index
// is the batch row, so an operand fragment is "eight consecutive rows of one column" per lane: exactly what a 4-byte
// load with lane = column delivers (128 contiguous bytes per half-wave), no transpose through LDS.  Both operands are
// split in registers into three exact bf16 planes (see gnm_lin_split_kernel) and six terms per 16 rows are issued.
// Eight waves per workgroup: wave (q, rs) owns the 64 x 64 quadrant q of dW and every second 16-row group of the
// workgroup's row range; the two row halves are added in a fixed order and the workgroup writes the same
// [H * kw + H] partial the fp32 kernels write, so gnm_reduce_partials_kernel and the workspace are unchanged.
// ---------------------------------------------------------------------------------
__global__ void __launch_bounds__(512) gnm_wgrad_split128_kernel(const WgArgs p) {
    constexpr int TILE = 16 * 64;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* dump = reinterpret_cast<float*>(smem);                 // [8 waves][4 tiles][16][64] + [8][2][64]
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int i = lane & 31, hh = lane >> 5;
    const int q = wave & 3, rs = wave >> 2;
    const int qi = q >> 1, qj = q & 1;
    const long long row0 = (long long)blockIdx.x * p.rows_per_block;
    const long long rows = min((long long)p.N - row0, (long long)p.rows_per_block);
    const __amdgpu_buffer_rsrc_t rd = gnm_tile_rsrc(p.dZ + row0 * p.ldd, rows, p.ldd, 128);
    const __amdgpu_buffer_rsrc_t rx = gnm_tile_rsrc(p.X + row0 * p.ldx + p.k0, rows, p.ldx, 128);
    int dvo[8], xvo[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        dvo[j] = ((8 * hh + j) * p.ldd + 64 * qi + i) * 4;
        xvo[j] = ((8 * hh + j) * p.ldx + 64 * qj + i) * 4;
    }
    float psc[2], psh[2];
#pragma unroll
    for (int b = 0; b < 2; ++b) {
        psc[b] = p.pro_scale ? p.pro_scale[p.k0 + 64 * qj + 32 * b + i] : 1.f;
        psh[b] = p.pro_scale ? p.pro_shift[p.k0 + 64 * qj + 32 * b + i] : 0.f;
    }
    f32x16 acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;
    float dbs[2] = {0.f, 0.f};
    const int ngroups = rows > 0 ? (int)((rows + 15) / 16) : 0;

    // a group past the end reads zeros (the descriptor's range check covers the scalar offset: see gnm_tile_rsrc)
    auto load = [&](float (&d)[2][8], float (&x)[2][8], int g) {
        const int sd = g * 16 * p.ldd * 4, sx = g * 16 * p.ldx * 4;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
#pragma unroll
            for (int a = 0; a < 2; ++a) d[a][j] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rd, dvo[j] + 128 * a, sd, 0));
#pragma unroll
            for (int b = 0; b < 2; ++b) x[b][j] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rx, xvo[j] + 128 * b, sx, 0));
        }
    };
    auto compute = [&](float (&d)[2][8], float (&x)[2][8]) {
        if (p.pro_scale) {
            // (a clipped row read zero and the affine map moves it: it meets a zero of dZ)
#pragma unroll
            for (int b = 0; b < 2; ++b)
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    float v = x[b][j] * psc[b] + psh[b];
                    x[b][j] = p.pro_relu ? gnm_relu(v) : v;
                }
        }
        gnm_bf16x8 dp[2][3], xp[2][3];
#pragma unroll
        for (int a = 0; a < 2; ++a) {
            dbs[a] += ((d[a][0] + d[a][1]) + (d[a][2] + d[a][3])) + ((d[a][4] + d[a][5]) + (d[a][6] + d[a][7]));
            gnm_split8(d[a], dp[a][0], dp[a][1], dp[a][2]);
            gnm_split8(x[a], xp[a][0], xp[a][1], xp[a][2]);
        }
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int b = 0; b < 2; ++b) gnm_mma6(acc[a][b], dp[a][0], dp[a][1], dp[a][2], xp[b][0], xp[b][1], xp[b][2]);
    };
    // two register images: group g + 2 is requested before group g is split and multiplied
    float dA_[2][8], xA_[2][8], dB_[2][8], xB_[2][8];
    load(dA_, xA_, rs);
#pragma nounroll
    for (int g = rs; g < ngroups; g += 4) {
        load(dB_, xB_, g + 2);
        compute(dA_, xA_);
        load(dA_, xA_, g + 4);
        compute(dB_, xB_);
    }
    __builtin_amdgcn_s_waitcnt(0x0F70);           // (the last, unused request)

    float* mine = dump + (size_t)wave * 4 * TILE;
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int r = 0; r < 16; ++r) mine[(a * 2 + b) * TILE + r * 64 + lane] = acc[a][b][r];
    float* dbdump = dump + (size_t)8 * 4 * TILE;
#pragma unroll
    for (int a = 0; a < 2; ++a) dbdump[(wave * 2 + a) * 64 + lane] = dbs[a];
    __syncthreads();
    float* out = p.partial + (size_t)blockIdx.x * ((size_t)p.H * p.kw + p.H);
    for (int idx = tid; idx < 4 * 4 * TILE; idx += 512) {
        const int qq = idx / (4 * TILE);
        const int rem = idx - qq * (4 * TILE);
        const int ab = rem / TILE;
        const int rl = rem - ab * TILE;
        const int r = rl >> 6, ln = rl & 63;
        const int row = 64 * (qq >> 1) + 32 * (ab >> 1) + (r & 3) + 8 * (r >> 2) + 4 * (ln >> 5);
        const int col = 64 * (qq & 1) + 32 * (ab & 1) + (ln & 31);
        out[(size_t)row * p.kw + col] = dump[(size_t)qq * 4 * TILE + rem] + dump[(size_t)(4 + qq) * 4 * TILE + rem];
    }
    for (int idx = tid; idx < 128; idx += 512) {
        const int qqi = idx >> 6, a = (idx >> 5) & 1, ii = idx & 31;
        float s = 0.f;
#pragma unroll
        for (int w = 0; w < 2; ++w) {
            const int wv = 4 * w + 2 * qqi;       // the quadrant with qj = 0 of this row half
            s += dbdump[(wv * 2 + a) * 64 + ii] + dbdump[(wv * 2 + a) * 64 + 32 + ii];
        }
        out[(size_t)p.H * p.kw + idx] = s;
    }
}

static int launch_wgrad_split128(const WgArgs& a, int grid, hipStream_t s) {
    const size_t lds = ((size_t)8 * 4 * 1024 + (size_t)8 * 2 * 64) * 4;
    GNM_ALLOW_FULL_LDS((&gnm_wgrad_split128_kernel));
    hipLaunchKernelGGL(gnm_wgrad_split128_kernel, dim3(grid), dim3(512), lds, s, a);
    GNM_CHECK_LAUNCH();
    return GNM_OK;
}

extern "C" int gnm_wgrad_grid(int N) {
    int g = (N + 511) / 512;            // >= 512 rows per block
    if (g > 256) g = 256;               // one block per CU: fewer partials to reduce
    return g < 1 ? 1 : g;
}

// Floats of workspace gnm_linear_wgrad needs: grid * (H*min(K,128) + H).
extern "C" long long gnm_wgrad_workspace_floats(int N, int H, int K) {
    const int kw = K < 128 ? K : 128;
    return (long long)gnm_wgrad_grid(N) * ((long long)H * kw + H);
}

// Second stage: sum the per-block partials in a fixed order and scatter the
// [H x kw] window into dW (leading dimension ldw, column offset k0) and db.
// 32 output elements per workgroup, 32 thread groups each summing every 32nd partial (so the
// ~8 MB of partials are streamed by ~130 workgroups instead of 17), combined through LDS.
__global__ void __launch_bounds__(1024) gnm_reduce_partials_kernel(const float* __restrict__ partial, int nblk,
                                                                   long long stride, int H, int kw, int k0,
                                                                   float* __restrict__ dW, int ldw,
                                                                   float* __restrict__ db) {
    __shared__ float red[32][32];
    const int tid = threadIdx.x;
    const int e = blockIdx.x * 32 + (tid & 31);
    const int count = H * kw + H;
    const float s = reduce_partials_element(partial, nblk, stride, e, count, red);
    if (tid < 32 && e < count) {
        if (e < H * kw) {
            const int row = e / kw, col = e - row * kw;
            dW[(size_t)row * ldw + k0 + col] = s;
        } else if (db && k0 == 0) {
            db[e - H * kw] = s;
        }
    }
}

// One such reduction: `nblk` partials of [H * kw + H] floats in `workspace` into columns k0 .. k0 + kw of dW, and db.
extern "C" __attribute__((visibility("hidden"))) int gnm_reduce_partials(const float* workspace, int nblk, int H, int kw,
                                                                         int k0, float* dW, int ldw, float* db,
                                                                         hipStream_t s) {
    const long long stride = (long long)H * kw + H;
    const int count = H * kw + H;
    hipLaunchKernelGGL(gnm_reduce_partials_kernel, dim3((count + 31) / 32), dim3(1024), 0, s, workspace, nblk, stride,
                       H, kw, k0, dW, ldw, db);
    GNM_CHECK_LAUNCH();
    return GNM_OK;
}

// The dW / db partial reductions of several gnm_linear_bwd_fused calls (dW = NULL there) in ONE launch: nothing in
// the backward depends on a weight gradient, so the ten ~5-us reductions of a step need not sit between its kernels.
// The per-element summation is gnm_reduce_partials_kernel's (reduce_partials_element).
#define GNM_MAX_REDUCE_JOBS 32
struct ReduceJobs {
    const float* partial[GNM_MAX_REDUCE_JOBS];
    float* dW[GNM_MAX_REDUCE_JOBS];
    float* db[GNM_MAX_REDUCE_JOBS];
    int nblk[GNM_MAX_REDUCE_JOBS], H[GNM_MAX_REDUCE_JOBS], K[GNM_MAX_REDUCE_JOBS], ldw[GNM_MAX_REDUCE_JOBS];
    int first_block[GNM_MAX_REDUCE_JOBS + 1];
    int njobs;
};
__global__ void __launch_bounds__(1024) gnm_reduce_partials_multi_kernel(const ReduceJobs J) {
    __shared__ float red[32][32];
    int j = 0;
    while (j + 1 < J.njobs && (int)blockIdx.x >= J.first_block[j + 1]) ++j;      // workgroup-uniform
    const float* __restrict__ partial = J.partial[j];
    const int nblk = J.nblk[j], H = J.H[j], kw = J.K[j];
    const long long stride = (long long)H * kw + H;
    const int tid = threadIdx.x;
    const int e = ((int)blockIdx.x - J.first_block[j]) * 32 + (tid & 31);
    const int count = H * kw + H;
    const float s = reduce_partials_element(partial, nblk, stride, e, count, red);
    if (tid < 32 && e < count) {
        if (e < H * kw) {
            const int row = e / kw, col = e - row * kw;
            J.dW[j][(size_t)row * J.ldw[j] + col] = s;
        } else if (J.db[j]) {
            J.db[j][e - H * kw] = s;
        }
    }
}

// workspaces[i]: the workspace of the i-th gnm_linear_bwd_fused(N, K = Ks[i], H = Hs[i], dW = NULL) call of the same N.
extern "C" int gnm_reduce_partials_multi(const float* const* workspaces_host, float* const* dW_host, const int* lddw_host,
                                         float* const* db_host, const int* Hs_host, const int* Ks_host, int njobs, int N,
                                         void* stream) {
    if (njobs <= 0) return GNM_OK;
    if (njobs > GNM_MAX_REDUCE_JOBS || N <= 0) return GNM_ERR_BAD_ARG;
    ReduceJobs J;
    int blocks = 0;
    for (int i = 0; i < njobs; ++i) {
        if (!workspaces_host[i] || !dW_host[i] || Hs_host[i] <= 0 || Ks_host[i] <= 0) return GNM_ERR_BAD_ARG;
        J.partial[i] = workspaces_host[i]; J.dW[i] = dW_host[i]; J.db[i] = db_host[i];
        J.nblk[i] = gnm_linear_bwd_grid(N); J.H[i] = Hs_host[i]; J.K[i] = Ks_host[i]; J.ldw[i] = lddw_host[i];
        J.first_block[i] = blocks;
        blocks += (Hs_host[i] * Ks_host[i] + Hs_host[i] + 31) / 32;
    }
    J.first_block[njobs] = blocks;
    J.njobs = njobs;
    hipLaunchKernelGGL(gnm_reduce_partials_multi_kernel, dim3(blocks), dim3(1024), 0, reinterpret_cast<hipStream_t>(stream), J);
    GNM_CHECK_LAUNCH();
    return GNM_OK;
}

// dW[H,K] (row-major, ld = ldw) and db[H] from dZ[N,H] and f(X)[N,K].  `workspace`
// must hold gnm_wgrad_workspace_floats(N,H,K) floats.
extern "C" int gnm_linear_wgrad(const float* dZ, int ldd, const float* X, int ldx, int N, int H, int K,
                                const float* pro_scale, const float* pro_shift, int pro_relu, float* dW, int ldw,
                                float* db, float* workspace, void* stream) {
    if (H <= 0 || K <= 0 || H > 128) return GNM_ERR_BAD_ARG;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const int grid = gnm_wgrad_grid(N > 0 ? N : 1);
    int rpb = ((N > 0 ? N : 1) + grid - 1) / grid;
    rpb = (rpb + 1) & ~1;
    const int HT = (H + 31) / 32;
    for (int k0 = 0; k0 < K; k0 += 128) {
        const int kw = (K - k0) < 128 ? (K - k0) : 128;
        const int KT = (kw + 31) / 32;
        WgArgs a;
        a.dZ = dZ; a.X = X; a.pro_scale = pro_scale; a.pro_shift = pro_shift; a.partial = workspace;
        a.ldd = ldd; a.ldx = ldx; a.N = N; a.H = H; a.K = K; a.k0 = k0; a.kw = kw; a.rows_per_block = rpb;
        a.pro_relu = pro_relu;
        const int WI = HT < 2 ? HT : 2, WJ = KT < 2 ? KT : 2;
        const int QI = (HT + WI - 1) / WI, QJ = (KT + WJ - 1) / WJ;
        int rc = GNM_ERR_UNSUPPORTED;
        const bool fast = (H % 32) == 0 && N > 0 && !lin_force_generic();
        // H = 128 and a full 128-column window, 32-bit offsets inside a workgroup's row range: the bf16-pipe kernel
        if (fast && H == 128 && kw == 128 && !lin_no_split() && (long long)(rpb + 64) * (ldd > ldx ? ldd : ldx) * 4 < (1LL << 31)) {
            rc = launch_wgrad_split128(a, grid, s);
            if (rc != GNM_OK) return rc;
        } else {
#define GNM_WG_CASE(WI_, WJ_, QI_, QJ_)                                                       \
    if (WI == WI_ && WJ == WJ_ && QI == QI_ && QJ == QJ_)                                     \
        rc = fast ? launch_wgrad_fast<WI_, WJ_, QI_, QJ_>(a, grid, s) : launch_wgrad<WI_, WJ_, QI_, QJ_>(a, grid, s);
        GNM_WG_CASE(1, 1, 1, 1) GNM_WG_CASE(1, 2, 1, 1) GNM_WG_CASE(1, 2, 1, 2)
        GNM_WG_CASE(2, 1, 1, 1) GNM_WG_CASE(2, 2, 1, 1) GNM_WG_CASE(2, 2, 1, 2)
        GNM_WG_CASE(2, 1, 2, 1) GNM_WG_CASE(2, 2, 2, 1) GNM_WG_CASE(2, 2, 2, 2)
#undef GNM_WG_CASE
        }
        if (rc == GNM_OK) rc = gnm_reduce_partials(workspace, grid, H, kw, k0, dW, ldw, db, s);
        if (rc != GNM_OK) return rc;
    }
    return GNM_OK;
}
