// The per-layer MLP contraction of the GIN update (K4 of SURVEY.md section 2.2):
// nn.Linear at /root/reference models/mlp.py:25,32-35,43,48,49, forward and the two
// backward products autograd derives (dX = dZ W, dW = dZ^T X, db = sum dZ), on the
// exact-fp32 matrix cores of gfx950 (v_mfma_f32_32x32x2_f32; gfx950 has no xf32).
//
// Shapes are tall and skinny ([N, K] x [K, H], N ~ 4e5, K, H <= 128), so:
//   * the whole weight matrix lives in LDS, k-major, for the kernel's lifetime;
//   * each wave owns 32-row tiles of X.  A tile is staged through a wave-private,
//     padded LDS image with full-line 16-B loads (fragment-shaped global loads
//     would touch 32 lines per instruction), where the fused prologue
//     relu(x*scale+shift) -- the BatchNorm+ReLU of the previous Linear
//     (mlp.py:48) -- is applied on the fly;
//   * the MFMA k order is permuted (k = (KC/2)*half + step) so a lane's KC/2
//     A-operands are contiguous in LDS and come in with ds_read_b128, conflict-free
//     at a row stride of KC+4 floats;
//   * the epilogue adds the bias, stores Z, and accumulates per-column sum and sum
//     of squares (fp64) for the BatchNorm that follows (mlp.py:48, graphcnn.py:163):
//     in the 32x32 C/D layout a lane owns one output COLUMN, so the statistics are
//     register adds.
//
// This unit holds the forward kernels, which also run dX = dZ W (w_kmajor = 1).  The weight gradient and the partial
// reductions are in linear_wgrad.hip, the fused BatchNorm backward + dgrad + wgrad in linear_bwd.hip; what they share
// is in gnm_linear.h.
#include "gnm_linear.h"

struct LinArgs {
    const float* X;
    const float* W;
    const float* bias;       // [H] or null
    float* Z;
    const float* pro_scale;  // [K] prologue x*scale+shift (then relu if pro_relu), or null
    const float* pro_shift;
    double* stats_partial;   // [gridDim.x][2][H] or null
    int ldx, ldw, ldz;
    int N, K, H;
    int w_kmajor;            // 0: W[h*ldw+k] (torch Linear weight);  1: W[k*ldw+h]
    int pro_relu;
    unsigned long long* stamps;   // tuning builds only (gnm_debug_set_lin_stamps): [block][4 waves][64] s_memtime
    int stat_rows;           // gnm_lin_split_kernel: rows of stats_partial = groups of four waves that take tiles
    int stage_out;           // gnm_lin_kernel: the launch reserved LDS for the output staging image
    // gnm_lin_split128_kernel, dX form (gnm_linear_dgrad_masked): the output is the gradient arriving at relu(bn(mZ)) of
    // the BatchNorm + ReLU below -- apply that ReLU mask on the way out and reduce that BatchNorm's backward sums
    // (sum G, sum G xhat) into stats_partial instead of the forward's (sum Z, sum Z^2)
    const float* mZ; const float* m_scale; const float* m_shift; const float* m_mean; const float* m_rstd;
    int ldmz;
};

// The tile map of lin_first_tile (gnm_linear.h) on the host, for tests/test_host_logic.py: every tile index below 4 x rows must belong to exactly one
// (workgroup, wave) of the launch, whatever the launch shape.
extern "C" int gnm_debug_lin_first_tile(int wave, int groups, int rows, int nwg, int b) {
    return lin_first_tile_of(wave, groups, rows, nwg, b);
}

#ifdef GNM_LIN_TUNING
unsigned long long* g_lin_stamps = nullptr;      // the one stamp buffer of the three units (declared in gnm_linear.h)
extern "C" void gnm_debug_set_lin_stamps(void* p) { g_lin_stamps = reinterpret_cast<unsigned long long*>(p); }
#endif

// What gnm_linear_fwd and gnm_linear_dgrad_masked fill the same way; every other field is zero (the masked form then
// sets its m* fields, a launcher its stat_rows / stage_out).
static inline LinArgs lin_args(const float* X, int ldx, const float* W, int ldw, int w_kmajor, const float* bias, float* Z,
                               int ldz, int N, int K, int H, const float* pro_scale, const float* pro_shift, int pro_relu,
                               double* stats_partial) {
    LinArgs a = {};
    a.X = X; a.W = W; a.bias = bias; a.Z = Z; a.pro_scale = pro_scale; a.pro_shift = pro_shift;
    a.stats_partial = stats_partial; a.ldx = ldx; a.ldw = ldw; a.ldz = ldz; a.N = N; a.K = K; a.H = H;
    a.w_kmajor = w_kmajor; a.pro_relu = pro_relu; a.stamps = g_lin_stamps;
    return a;
}

template <int KC, int HT>
__global__ void __launch_bounds__(256) gnm_lin_kernel(const LinArgs p) {
    constexpr int HP = HT * 32;          // padded output width
    constexpr int XS = KC + 4;           // staging row stride (floats): conflict-free ds_read_b128
    constexpr int C4 = KC / 4;           // float4 per staged row
    constexpr int KH = KC / 2;           // MFMA steps per chunk
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int nchunks = (p.K + KC - 1) / KC;
    const int KP = nchunks * KC;
    float* Wt = reinterpret_cast<float*>(smem);                   // [KP][HP]
    float* Xs_all = Wt + (size_t)KP * HP;                         // [4][32][XS]
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int i = lane & 31;
    const int h = lane >> 5;
    float* Xs = Xs_all + wave * 32 * XS;
    // output staging (aligned full-width outputs): the tile leaves as 16-byte row-contiguous stores -- 1 KiB per
    // wave-instruction instead of 128-byte column pieces; the input layer's Linear (K = F0) is all output traffic
    constexpr int OS = HP + 4, O4 = HP / 4;
    float* Os = Xs_all + 4 * 32 * XS + wave * 32 * OS;
    const bool vec_out = p.stage_out && p.H == HP && (p.ldz & 3) == 0 && (reinterpret_cast<uintptr_t>(p.Z) & 15) == 0;

    // ---- stage W^T (k-major, zero padded) --------------------------------------
    if (p.w_kmajor) {
        for (int idx = tid; idx < KP * HP; idx += 256) {
            const int k = idx / HP, hh = idx - k * HP;
            Wt[idx] = (k < p.K && hh < p.H) ? p.W[(size_t)k * p.ldw + hh] : 0.f;
        }
    } else {
        for (int idx = tid; idx < KP * HP; idx += 256) {
            const int hh = idx / KP, k = idx - hh * KP;
            Wt[k * HP + hh] = (k < p.K && hh < p.H) ? p.W[(size_t)hh * p.ldw + k] : 0.f;
        }
    }
    __syncthreads();

    const bool vec_in = ((p.ldx & 3) == 0) && ((reinterpret_cast<uintptr_t>(p.X) & 15) == 0);
    const int ntiles = (p.N + 31) / 32;
    double st1[HT], st2[HT];
#pragma unroll
    for (int c = 0; c < HT; ++c) { st1[c] = 0.0; st2[c] = 0.0; }
    float bias_r[HT];
#pragma unroll
    for (int c = 0; c < HT; ++c) {
        const int col = 32 * c + i;
        bias_r[c] = (p.bias && col < p.H) ? p.bias[col] : 0.f;
    }
    const int c4 = lane % C4;            // loop-invariant: 64 % C4 == 0

    for (int t = lin_first_tile(wave, 1, gridDim.x); t < ntiles; t += gridDim.x * 4) {
        const int r0 = t * 32;
        f32x16 acc[HT];
#pragma unroll
        for (int c = 0; c < HT; ++c)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[c][r] = 0.f;

        for (int kc = 0; kc < nchunks; ++kc) {
            const int kb = kc * KC;
            // -- stage the [32][KC] chunk of X (coalesced), fused prologue --
            const int k4 = kb + 4 * c4;
            float4 sc = make_float4(1.f, 1.f, 1.f, 1.f), sh = make_float4(0.f, 0.f, 0.f, 0.f);
            if (p.pro_scale) {
                sc.x = (k4 + 0 < p.K) ? p.pro_scale[k4 + 0] : 0.f; sh.x = (k4 + 0 < p.K) ? p.pro_shift[k4 + 0] : 0.f;
                sc.y = (k4 + 1 < p.K) ? p.pro_scale[k4 + 1] : 0.f; sh.y = (k4 + 1 < p.K) ? p.pro_shift[k4 + 1] : 0.f;
                sc.z = (k4 + 2 < p.K) ? p.pro_scale[k4 + 2] : 0.f; sh.z = (k4 + 2 < p.K) ? p.pro_shift[k4 + 2] : 0.f;
                sc.w = (k4 + 3 < p.K) ? p.pro_scale[k4 + 3] : 0.f; sh.w = (k4 + 3 < p.K) ? p.pro_shift[k4 + 3] : 0.f;
            }
#pragma unroll
            for (int idx = lane; idx < 32 * C4; idx += 64) {
                const int row = idx / C4;
                const int grow = r0 + row;
                float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
                if (grow < p.N) {
                    const float* src = p.X + (size_t)grow * p.ldx + k4;
                    if (vec_in && k4 + 3 < p.K) {
                        v = *reinterpret_cast<const float4*>(src);
                    } else {
                        if (k4 + 0 < p.K) v.x = src[0];
                        if (k4 + 1 < p.K) v.y = src[1];
                        if (k4 + 2 < p.K) v.z = src[2];
                        if (k4 + 3 < p.K) v.w = src[3];
                    }
                    if (p.pro_scale) {
                        v.x = v.x * sc.x + sh.x; v.y = v.y * sc.y + sh.y;
                        v.z = v.z * sc.z + sh.z; v.w = v.w * sc.w + sh.w;
                        if (p.pro_relu) {
                            v.x = gnm_relu(v.x); v.y = gnm_relu(v.y);
                            v.z = gnm_relu(v.z); v.w = gnm_relu(v.w);
                        }
                    }
                }
                *reinterpret_cast<float4*>(Xs + row * XS + 4 * c4) = v;
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            // -- A fragments: lane (i, h) takes X[r0+i][kb + KH*h + s], s = 0..KH-1 --
            float a[KH];
#pragma unroll
            for (int j = 0; j < KH / 4; ++j) {
                const float4 v = *reinterpret_cast<const float4*>(Xs + i * XS + KH * h + 4 * j);
                a[4 * j + 0] = v.x; a[4 * j + 1] = v.y; a[4 * j + 2] = v.z; a[4 * j + 3] = v.w;
            }
            const float* wrow = Wt + (size_t)(kb + KH * h) * HP + i;
#pragma unroll
            for (int s = 0; s < KH; ++s) {
#pragma unroll
                for (int c = 0; c < HT; ++c) {
                    const float bv = wrow[s * HP + 32 * c];
                    acc[c] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[s], bv, acc[c], 0, 0, 0);
                }
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();   // A fragments are in registers before Xs is overwritten
        }

        // ---- epilogue: bias, store, BatchNorm statistics ----------------------
#pragma unroll
        for (int c = 0; c < HT; ++c) {
            const int col = 32 * c + i;
            float s1 = 0.f, s2 = 0.f;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int lrow = (r & 3) + 8 * (r >> 2) + 4 * h;
                const int grow = r0 + lrow;
                const float z = acc[c][r] + bias_r[c];
                if (vec_out) Os[lrow * OS + col] = z;
                if (grow < p.N && col < p.H) {
                    if (!vec_out) p.Z[(size_t)grow * p.ldz + col] = z;
                    s1 += z;
                    s2 += z * z;
                }
            }
            st1[c] += (double)s1;
            st2[c] += (double)s2;
        }
        if (vec_out) {                                           // (kernel-uniform)
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
            for (int idx = lane; idx < 32 * O4; idx += 64) {
                const int row = idx / O4, oc = idx - row * O4;
                if (r0 + row < p.N)
                    *reinterpret_cast<float4*>(p.Z + (size_t)(r0 + row) * p.ldz + 4 * oc) =
                        *reinterpret_cast<const float4*>(Os + row * OS + 4 * oc);
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
        }
    }

    if (p.stats_partial) {   // block-level combine in a fixed order, one partial row per block
        __syncthreads();
        double* red = reinterpret_cast<double*>(smem);   // [4 waves][2][HP]
#pragma unroll
        for (int c = 0; c < HT; ++c) {
            const double a1 = st1[c] + __shfl_xor(st1[c], 32, 64);
            const double a2 = st2[c] + __shfl_xor(st2[c], 32, 64);
            if (h == 0) {
                red[(wave * 2 + 0) * HP + 32 * c + i] = a1;
                red[(wave * 2 + 1) * HP + 32 * c + i] = a2;
            }
        }
        __syncthreads();
        for (int idx = tid; idx < 2 * HP; idx += 256) {
            const int which = idx / HP, col = idx - which * HP;
            if (col < p.H) {
                double s = 0.0;
                for (int w = 0; w < 4; ++w) s += red[(w * 2 + which) * HP + col];
                p.stats_partial[((size_t)blockIdx.x * 2 + which) * p.H + col] = s;
            }
        }
    }
}

// ---------------------------------------------------------------------------------
// Pipelined variant for the common case: 16-B aligned rows, K a multiple of the chunk KC,
// H == 32*HT.  No column guards; rows past N are clamped on load and masked in the
// epilogue.  Differences from the generic kernel above:
//   * the NEXT tile's global loads are issued right after this tile's A fragments are in
//     registers, so they fly under the MFMAs (the generic kernel serialises load -> MFMA);
//   * the output tile is transposed through the wave's staging image and stored as full
//     16-B row-contiguous chunks (1 KiB per wave-instruction) instead of 4-B column pieces.
// ---------------------------------------------------------------------------------
template <int KC, int HT>
__global__ void __launch_bounds__(256) gnm_lin_fast_kernel(const LinArgs p) {
    constexpr int HP = HT * 32;
    constexpr int XS = (KC > HP ? KC : HP) + 4;   // staging row stride: holds an input chunk or the output tile
    constexpr int C4 = KC / 4;
    constexpr int KH = KC / 2;
    constexpr int NLD = (32 * C4) / 64;           // float4 loads per lane per chunk (KC >= 8)
    constexpr int O4 = HP / 4;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int nchunks = p.K / KC;
    float* Wt = reinterpret_cast<float*>(smem);                   // [K][HP]
    float* Xs_all = Wt + (size_t)p.K * HP;                        // [4][32][XS]
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int i = lane & 31;
    const int h = lane >> 5;
    float* Xs = Xs_all + wave * 32 * XS;
    GNM_LSTAMP(0)

    if (p.w_kmajor) {
        for (int idx = tid; idx < p.K * HP; idx += 256) {
            const int k = idx / HP, hh = idx - k * HP;
            Wt[idx] = p.W[(size_t)k * p.ldw + hh];
        }
    } else {
        for (int idx = tid; idx < p.K * HP; idx += 256) {
            const int hh = idx / p.K, k = idx - hh * p.K;
            Wt[k * HP + hh] = p.W[(size_t)hh * p.ldw + k];
        }
    }
    __syncthreads();
    GNM_LSTAMP(1)
    int tk = 0;

    const int ntiles = (p.N + 31) / 32;
    double st1[HT], st2[HT];
    float bias_r[HT];
#pragma unroll
    for (int c = 0; c < HT; ++c) {
        st1[c] = 0.0; st2[c] = 0.0;
        bias_r[c] = p.bias ? p.bias[32 * c + i] : 0.f;
    }
    const int c4 = lane % C4;
    const int lrow0 = lane / C4;                  // row of this lane's first float4; later ones are +64/C4 rows
    constexpr int RSTEP = 64 / C4;
    const int tstride = gridDim.x * 4;
    const int nlast = p.N - 1;

    float4 raw[NLD];
    int t = lin_first_tile(wave, 1, gridDim.x);
    if (t < ntiles) {
#pragma unroll
        for (int j = 0; j < NLD; ++j) {
            const int grow = min(t * 32 + lrow0 + j * RSTEP, nlast);
            raw[j] = *reinterpret_cast<const float4*>(p.X + (size_t)grow * p.ldx + 4 * c4);
        }
    }
    for (; t < ntiles; t += tstride) {
        const int r0 = t * 32;
        GNM_LSTAMP(2 + 4 * min(tk, 14))
        f32x16 acc[HT];
#pragma unroll
        for (int c = 0; c < HT; ++c)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[c][r] = 0.f;

        for (int kc = 0; kc < nchunks; ++kc) {
            const int kb = kc * KC;
            if (p.pro_scale) {
                const float4 sc = *reinterpret_cast<const float4*>(p.pro_scale + kb + 4 * c4);
                const float4 sh = *reinterpret_cast<const float4*>(p.pro_shift + kb + 4 * c4);
#pragma unroll
                for (int j = 0; j < NLD; ++j) {
                    float4 v = raw[j];
                    v.x = v.x * sc.x + sh.x; v.y = v.y * sc.y + sh.y; v.z = v.z * sc.z + sh.z; v.w = v.w * sc.w + sh.w;
                    if (p.pro_relu) {
                        v.x = gnm_relu(v.x); v.y = gnm_relu(v.y); v.z = gnm_relu(v.z); v.w = gnm_relu(v.w);
                    }
                    raw[j] = v;
                }
            }
#pragma unroll
            for (int j = 0; j < NLD; ++j)
                *reinterpret_cast<float4*>(Xs + (lrow0 + j * RSTEP) * XS + 4 * c4) = raw[j];
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            float a[KH];
#pragma unroll
            for (int j = 0; j < KH / 4; ++j) {
                const float4 v = *reinterpret_cast<const float4*>(Xs + i * XS + KH * h + 4 * j);
                a[4 * j + 0] = v.x; a[4 * j + 1] = v.y; a[4 * j + 2] = v.z; a[4 * j + 3] = v.w;
            }
            // next chunk (of this tile, or chunk 0 of this wave's next tile): loads fly under the MFMAs
            {
                const bool more_k = kc + 1 < nchunks;
                const int tn = more_k ? t : t + tstride;
                const int kn = more_k ? kb + KC : 0;
                if (tn < ntiles) {
#pragma unroll
                    for (int j = 0; j < NLD; ++j) {
                        const int grow = min(tn * 32 + lrow0 + j * RSTEP, nlast);
                        raw[j] = *reinterpret_cast<const float4*>(p.X + (size_t)grow * p.ldx + kn + 4 * c4);
                    }
                }
            }
            GNM_LSTAMP(3 + 4 * min(tk, 14))
            const float* wrow = Wt + (size_t)(kb + KH * h) * HP + i;
#pragma unroll
            for (int s = 0; s < KH; ++s) {
#pragma unroll
                for (int c = 0; c < HT; ++c) {
                    const float bv = wrow[s * HP + 32 * c];
                    acc[c] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[s], bv, acc[c], 0, 0, 0);
                }
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
        }
        GNM_LSTAMP(4 + 4 * min(tk, 14))

        // epilogue: bias, statistics (valid rows only), transpose through LDS, 16-B stores
#pragma unroll
        for (int c = 0; c < HT; ++c) {
            float s1 = 0.f, s2 = 0.f;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int lrow = (r & 3) + 8 * (r >> 2) + 4 * h;
                const float z = acc[c][r] + bias_r[c];
                Xs[lrow * XS + 32 * c + i] = z;
                if (r0 + lrow < p.N) {
                    s1 += z;
                    s2 += z * z;
                }
            }
            st1[c] += (double)s1;
            st2[c] += (double)s2;
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
        for (int idx = lane; idx < 32 * O4; idx += 64) {
            const int row = idx / O4, oc = idx - row * O4;
            if (r0 + row < p.N)
                *reinterpret_cast<float4*>(p.Z + (size_t)(r0 + row) * p.ldz + 4 * oc) =
                    *reinterpret_cast<const float4*>(Xs + row * XS + 4 * oc);
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        GNM_LSTAMP(5 + 4 * min(tk, 14))
        ++tk;
    }
    GNM_LSTAMP(62)

    if (p.stats_partial) {
        __syncthreads();
        double* red = reinterpret_cast<double*>(smem);   // [4 waves][2][HP]
#pragma unroll
        for (int c = 0; c < HT; ++c) {
            const double a1 = st1[c] + __shfl_xor(st1[c], 32, 64);
            const double a2 = st2[c] + __shfl_xor(st2[c], 32, 64);
            if (h == 0) {
                red[(wave * 2 + 0) * HP + 32 * c + i] = a1;
                red[(wave * 2 + 1) * HP + 32 * c + i] = a2;
            }
        }
        __syncthreads();
        for (int idx = tid; idx < 2 * HP; idx += 256) {
            const int which = idx / HP, col = idx - which * HP;
            double s = 0.0;
            for (int w = 0; w < 4; ++w) s += red[(w * 2 + which) * HP + col];
            p.stats_partial[((size_t)blockIdx.x * 2 + which) * p.H + col] = s;
        }
    }
}

template <int KC, int HT>
static int launch_lin_fast(const LinArgs& a, int grid, hipStream_t s) {
    constexpr int HP = HT * 32;
    constexpr int XS = (KC > HP ? KC : HP) + 4;
    size_t lds = (size_t)a.K * HP * 4 + (size_t)4 * 32 * XS * 4;
    const size_t red = (size_t)4 * 2 * HP * 8;
    if (red > lds) lds = red;
    if (lds > (size_t)kLdsBudget) return GNM_ERR_UNSUPPORTED;
    GNM_ALLOW_FULL_LDS((&gnm_lin_fast_kernel<KC, HT>));
    hipLaunchKernelGGL((gnm_lin_fast_kernel<KC, HT>), dim3(grid), dim3(256), lds, s, a);
    GNM_CHECK_LAUNCH();
    return GNM_OK;
}

// ---------------------------------------------------------------------------------
// Streaming variant for K == KC (the whole input row is one chunk: every hidden Linear of the model).  Same tile
// arithmetic as the pipelined kernel above; what changes is how a wave's memory operations are ordered and counted.
// gfx950 retires vector-memory operations IN ORDER, stores included, and `s_waitcnt vmcnt(n)` waits until at most n are
// outstanding.  The pipelined kernel issues  loads(t+1) .. stores(t)  and then needs loads(t+1): the compiler could
// not prove that the stores behind them had been issued on every path (row guards, the first trip through the loop),
// so it waited for vmcnt(7..0) -- i.e. for the STORES of the previous tile to land in HBM -- before staging the next
// tile, and for vmcnt(0) (bias load, never counted down) in front of every epilogue.  The in-kernel timeline showed
// those two waits as ~22 % + part of the epilogue's 25 % of a tile's time.  Here
//   * loads and stores are buffer instructions whose descriptor covers exactly the tile's valid rows: rows past N
//     (and whole tiles past the last) are dropped by the address check, so every access is issued unconditionally;
//   * the first tile is peeled, so the loop is entered with the same  loads, stores  queue its back edge carries;
//   * bias / prologue constants are waited for once, before the first tile.
// The wait in front of the staging writes becomes vmcnt(15..8): the previous tile's stores drain under this tile's
// MFMAs instead of in front of them.
// ---------------------------------------------------------------------------------
template <int KC, int HT>
__global__ void __launch_bounds__(256) gnm_lin_stream_kernel(const LinArgs p) {
    constexpr int HP = HT * 32;
    constexpr int XS = (KC > HP ? KC : HP) + 4;
    constexpr int C4 = KC / 4;
    constexpr int KH = KC / 2;
    constexpr int NLD = (32 * C4) / 64;           // 16-B loads per lane per tile
    constexpr int RSTEP = 64 / C4;                // rows between a lane's consecutive loads
    constexpr int O4 = HP / 4;
    constexpr int NST = (32 * O4) / 64;           // 16-B stores per lane per tile
    constexpr int WSTEP = 64 / O4;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* Wt = reinterpret_cast<float*>(smem);                   // [KC][HP]
    float* Xs_all = Wt + (size_t)KC * HP;                         // [4][32][XS]
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int i = lane & 31;
    const int h = lane >> 5;
    float* Xs = Xs_all + wave * 32 * XS;
    GNM_LSTAMP(0)

    const int c4 = lane % C4;
    const int lrow0 = lane / C4;
    float bias_r[HT];
#pragma unroll
    for (int c = 0; c < HT; ++c) bias_r[c] = p.bias ? p.bias[32 * c + i] : 0.f;
    float4 sc = make_float4(1.f, 1.f, 1.f, 1.f), sh = make_float4(0.f, 0.f, 0.f, 0.f);
    const bool pro = p.pro_scale != nullptr;
    if (pro) {
        sc = *reinterpret_cast<const float4*>(p.pro_scale + 4 * c4);
        sh = *reinterpret_cast<const float4*>(p.pro_shift + 4 * c4);
    }
    const int ntiles = (p.N + 31) / 32;
    const int tstride = gridDim.x * 4;
    const int in_voff = (lrow0 * p.ldx + 4 * c4) * 4;            // byte offsets inside a tile's descriptor
    const int in_step = RSTEP * p.ldx * 4;
    const int out_voff = ((lane / O4) * p.ldz + 4 * (lane % O4)) * 4;
    const int out_step = WSTEP * p.ldz * 4;

    gnm_u32x4 raw[NLD];
    auto load_tile = [&](int tile) {
        const long long row0 = (long long)tile * 32;
        const __amdgpu_buffer_rsrc_t rs = gnm_tile_rsrc(p.X + row0 * p.ldx, min((long long)p.N - row0, 32LL), p.ldx, KC);
#pragma unroll
        for (int j = 0; j < NLD; ++j) raw[j] = __builtin_amdgcn_raw_buffer_load_b128(rs, in_voff, j * in_step, 0);
    };
    int t = lin_first_tile(wave, 1, gridDim.x);
    load_tile(t);                                 // the first tile arrives while the weight is staged

    // weight -> LDS as Wt[k][h].  torch layout W[h][k]: a lane takes 4 consecutive k of one h (16-B global read) and
    // consecutive lanes take consecutive h, so the four transposed LDS writes of a wave fall in consecutive banks.
    // (a weight inside a flat parameter buffer need not be 16-byte aligned: four 4-byte loads then)
    const bool w_vec = (p.ldw & 3) == 0 && (reinterpret_cast<uintptr_t>(p.W) & 15) == 0;
    auto load_w4 = [&](const float* src) -> float4 {
        if (w_vec) return *reinterpret_cast<const float4*>(src);
        return make_float4(src[0], src[1], src[2], src[3]);
    };
    if (p.w_kmajor) {
#pragma unroll
        for (int it = 0; it < (KC * O4) / 256; ++it) {
            const int idx = tid + 256 * it;
            const int k = idx / O4, h4 = idx - k * O4;
            *reinterpret_cast<float4*>(Wt + k * HP + 4 * h4) = load_w4(p.W + (size_t)k * p.ldw + 4 * h4);
        }
    } else {
        float4 w[(C4 * HP) / 256];
#pragma unroll
        for (int it = 0; it < (C4 * HP) / 256; ++it) {
            const int idx = tid + 256 * it;
            const int k4 = idx / HP, hh = idx - k4 * HP;
            w[it] = load_w4(p.W + (size_t)hh * p.ldw + 4 * k4);
        }
#pragma unroll
        for (int it = 0; it < (C4 * HP) / 256; ++it) {
            const int idx = tid + 256 * it;
            const int k4 = idx / HP, hh = idx - k4 * HP;
            Wt[(4 * k4 + 0) * HP + hh] = w[it].x;
            Wt[(4 * k4 + 1) * HP + hh] = w[it].y;
            Wt[(4 * k4 + 2) * HP + hh] = w[it].z;
            Wt[(4 * k4 + 3) * HP + hh] = w[it].w;
        }
    }
    __builtin_amdgcn_s_waitcnt(0x0F70);           // vmcnt(0): nothing from the preamble is pending inside the tile loop
    __syncthreads();
    GNM_LSTAMP(1)
    int tk = 0;

    double st1[HT], st2[HT];
#pragma unroll
    for (int c = 0; c < HT; ++c) { st1[c] = 0.0; st2[c] = 0.0; }
    auto do_tile = [&](int t) {
        const int r0 = t * 32;
        GNM_LSTAMP(2 + 4 * min(tk, 14))
        f32x16 acc[HT];
#pragma unroll
        for (int c = 0; c < HT; ++c)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[c][r] = 0.f;
#pragma unroll
        for (int j = 0; j < NLD; ++j) {
            float4 v = __builtin_bit_cast(float4, raw[j]);
            if (pro) {
                v.x = v.x * sc.x + sh.x; v.y = v.y * sc.y + sh.y; v.z = v.z * sc.z + sh.z; v.w = v.w * sc.w + sh.w;
                if (p.pro_relu) {
                    v.x = gnm_relu(v.x); v.y = gnm_relu(v.y); v.z = gnm_relu(v.z); v.w = gnm_relu(v.w);
                }
            }
            *reinterpret_cast<float4*>(Xs + (lrow0 + j * RSTEP) * XS + 4 * c4) = v;
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        float a[KH];
#pragma unroll
        for (int j = 0; j < KH / 4; ++j) {
            const float4 v = *reinterpret_cast<const float4*>(Xs + i * XS + KH * h + 4 * j);
            a[4 * j + 0] = v.x; a[4 * j + 1] = v.y; a[4 * j + 2] = v.z; a[4 * j + 3] = v.w;
        }
        load_tile(t + tstride);                   // past the last tile: an empty descriptor, no memory traffic
        GNM_LSTAMP(3 + 4 * min(tk, 14))
        const float* wrow = Wt + (size_t)(KH * h) * HP + i;
#pragma unroll
        for (int s = 0; s < KH; ++s) {
#pragma unroll
            for (int c = 0; c < HT; ++c) {
                const float bv = wrow[s * HP + 32 * c];
                acc[c] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[s], bv, acc[c], 0, 0, 0);
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();          // A fragments are in registers before the staging image is reused
        GNM_LSTAMP(4 + 4 * min(tk, 14))
#pragma unroll
        for (int c = 0; c < HT; ++c) {
            float s1 = 0.f, s2 = 0.f;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int lrow = (r & 3) + 8 * (r >> 2) + 4 * h;
                const float z = acc[c][r] + bias_r[c];
                Xs[lrow * XS + 32 * c + i] = z;
                if (r0 + lrow < p.N) {
                    s1 += z;
                    s2 += z * z;
                }
            }
            st1[c] += (double)s1;
            st2[c] += (double)s2;
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        const __amdgpu_buffer_rsrc_t rz = gnm_tile_rsrc(p.Z + (size_t)r0 * p.ldz, min(p.N - r0, 32), p.ldz, HP);
#pragma unroll
        for (int st = 0; st < NST; ++st) {
            const int idx = lane + 64 * st;
            const int row = idx / O4, oc = idx - row * O4;
            const gnm_u32x4 v = *reinterpret_cast<const gnm_u32x4*>(Xs + row * XS + 4 * oc);
            // row step in the VECTOR offset, scalar offset 0: with an SGPR soffset hipcc (ROCm 7.2) schedules a VALU
            // write of the data registers straight behind a 16-byte buffer store (its hazard table exempts that form)
            // and on gfx950 the store then picks up the new value in some lanes -- seen as address integers in Z.
            __builtin_amdgcn_raw_buffer_store_b128(v, rz, out_voff + st * out_step, 0, 0);
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        GNM_LSTAMP(5 + 4 * min(tk, 14))
        ++tk;
    };

    if (t < ntiles) {
        do_tile(t);                               // peeled: the loop below starts with loads(t+1), stores(t) in flight
        for (t += tstride; t < ntiles; t += tstride) do_tile(t);
    }
    GNM_LSTAMP(62)

    if (p.stats_partial) {
        __syncthreads();
        double* red = reinterpret_cast<double*>(smem);   // [4 waves][2][HP]
#pragma unroll
        for (int c = 0; c < HT; ++c) {
            const double a1 = st1[c] + __shfl_xor(st1[c], 32, 64);
            const double a2 = st2[c] + __shfl_xor(st2[c], 32, 64);
            if (h == 0) {
                red[(wave * 2 + 0) * HP + 32 * c + i] = a1;
                red[(wave * 2 + 1) * HP + 32 * c + i] = a2;
            }
        }
        __syncthreads();
        for (int idx = tid; idx < 2 * HP; idx += 256) {
            const int which = idx / HP, col = idx - which * HP;
            double s = 0.0;
            for (int w = 0; w < 4; ++w) s += red[(w * 2 + which) * HP + col];
            p.stats_partial[((size_t)blockIdx.x * 2 + which) * p.H + col] = s;
        }
    }
}

template <int KC, int HT>
static int launch_lin_stream(const LinArgs& a, int grid, hipStream_t s) {
    constexpr int HP = HT * 32;
    constexpr int XS = (KC > HP ? KC : HP) + 4;
    size_t lds = (size_t)KC * HP * 4 + (size_t)4 * 32 * XS * 4;
    const size_t red = (size_t)4 * 2 * HP * 8;
    if (red > lds) lds = red;
    if (lds > (size_t)kLdsBudget) return GNM_ERR_UNSUPPORTED;
    GNM_ALLOW_FULL_LDS((&gnm_lin_stream_kernel<KC, HT>));
    hipLaunchKernelGGL((gnm_lin_stream_kernel<KC, HT>), dim3(grid), dim3(256), lds, s, a);
    GNM_CHECK_LAUNCH();
    return GNM_OK;
}

// ---------------------------------------------------------------------------------
// Split-precision variant of the streaming kernel for K = 64, H = 64 (every hidden Linear of the headline model).
// The fp32 matrix instruction (v_mfma_f32_32x32x2_f32, 64 FLOP/clk per SIMD) kept a wave in its product for 41 % of
// its life with three waves per SIMD -- the matrix pipe was the resource the waves queued for, not HBM.  Here both
// operands are split by truncation into three bf16 planes each (x = x1 + x2 + x3 EXACTLY: 8 + 8 + 8 mantissa bits) and
// the product runs as six bf16 matrix instructions per 16 k (x1w1, x1w2, x2w1, x2w2, x1w3, x3w1; 16x the fp32 rate):
// every partial product is exact in the fp32 accumulator, the three dropped terms are below 2^-24 of |x||w| each --
// the size of the accumulator's own rounding -- and the instruction count falls from 64 x 64 to 48 x 32 cycles per tile.
// One 768-thread workgroup per CU (12 waves share one 24 KB image of the weight planes; three 256-thread workgroups
// with a copy each do not fit the LDS); its waves form three groups of four that write three rows of statistics
// partials, so the launch produces exactly the gnm_linear_grid(N) rows the BatchNorm finalize expects.
// ---------------------------------------------------------------------------------
#ifndef GNM_SPLIT_WAVES           // tuning builds: 16 = four waves per SIMD (needs GNM_LIN_GRID=1024 to fill 256 CUs)
#define GNM_SPLIT_WAVES 12
#endif
static constexpr int kSplitWaves = GNM_SPLIT_WAVES;
#ifndef GNM_L64_ABLATE           // tuning builds (-DGNM_L64_ABLATE=n): 1 = no output stores, 2 = no input traffic
#define GNM_L64_ABLATE 0
#endif

template <int HT>
__global__ void __launch_bounds__(kSplitWaves * 64) gnm_lin_split_kernel(const LinArgs p) {
    constexpr int KC = 64, NW = kSplitWaves, NT = NW * 64;
    constexpr int HP = HT * 32;
    constexpr int XS = (KC > HP ? KC : HP) + 4;
    constexpr int C4 = KC / 4;
    constexpr int KH = KC / 2;
    constexpr int NLD = (32 * C4) / 64;
    constexpr int RSTEP = 64 / C4;
    constexpr int O4 = HP / 4;
    constexpr int NST = (32 * O4) / 64;
    constexpr int WSTEP = 64 / O4;
    constexpr int E = 4 * HT * 64;                // operand entries (16 B) per weight plane: [m][c][lane]
    GNM_SSTAMP(0)
    extern __shared__ __attribute__((aligned(16))) char smem[];
    gnm_u32x4* Wp = reinterpret_cast<gnm_u32x4*>(smem);                               // [3][E]
    float* Xs_all = reinterpret_cast<float*>(smem + (size_t)3 * E * 16);      // [NW][32][XS]; first the fp32 weight image
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int i = lane & 31;
    const int h = lane >> 5;
    float* Xs = Xs_all + wave * 32 * XS;

    const int c4 = lane % C4;
    const int lrow0 = lane / C4;
    float bias_r[HT];
#pragma unroll
    for (int c = 0; c < HT; ++c) bias_r[c] = p.bias ? p.bias[32 * c + i] : 0.f;
    float4 sc = make_float4(1.f, 1.f, 1.f, 1.f), sh = make_float4(0.f, 0.f, 0.f, 0.f);
    const bool pro = p.pro_scale != nullptr;
    if (pro) {
        sc = *reinterpret_cast<const float4*>(p.pro_scale + 4 * c4);
        sh = *reinterpret_cast<const float4*>(p.pro_shift + 4 * c4);
    }
    // waves are numbered across the launch; groups of four own one row of statistics partials, exactly the tile ->
    // row map of the 4-wave kernels; waves past the last row (a grid that is not a multiple of 3) take no tiles
    const int gw = lin_first_tile(wave, NW / 4, p.stat_rows);
    const int ntiles = (p.N + 31) / 32;
    const int tstride = 4 * p.stat_rows;
    const int in_voff = (lrow0 * p.ldx + 4 * c4) * 4;
    const int in_step = RSTEP * p.ldx * 4;
    const int out_voff = ((lane / O4) * p.ldz + 4 * (lane % O4)) * 4;
    const int out_step = WSTEP * p.ldz * 4;

    gnm_u32x4 raw[NLD];
    auto load_tile = [&](int tile) {
        const long long row0 = (long long)tile * 32;
        const __amdgpu_buffer_rsrc_t rs = gnm_tile_rsrc(p.X + row0 * p.ldx, (GNM_L64_ABLATE & 2) ? 0LL : min((long long)p.N - row0, 32LL), p.ldx, KC);
#pragma unroll
        for (int j = 0; j < NLD; ++j) raw[j] = __builtin_amdgcn_raw_buffer_load_b128(rs, in_voff, j * in_step, kLoadOnce);
    };
    int t = gw;
    load_tile(t);

    // weight -> fp32 image Wt[k][h] in the staging region, then -> the three bf16 operand planes
    float* Wt = Xs_all;
    const bool w_vec = (p.ldw & 3) == 0 && (reinterpret_cast<uintptr_t>(p.W) & 15) == 0;
    auto load_w4 = [&](const float* src) -> float4 {
        if (w_vec) return *reinterpret_cast<const float4*>(src);
        return make_float4(src[0], src[1], src[2], src[3]);
    };
    // entry (m, c, lane = 32 kg + n): W[k = 8 m + 32 kg + 0..7][h = 32 c + n] -- the k numbering the A fragments use
    if (!p.w_kmajor) {
        // torch's layout W[h][k]: an entry's eight k are 32 contiguous bytes of row h -- straight from global memory
        // (L2) into the split; the fp32 image, its transposing scalar LDS writes and one of the two barriers were a
        // fifth of a wave's lifetime (in-kernel timeline, tools/lin_timeline.py --kernel fwd_split)
        for (int e = tid; e < E; e += NT) {
            const int n = e & 31, kg = (e >> 5) & 1, c = (e >> 6) % HT, m = e / (64 * HT);
            const float* src = p.W + (size_t)(32 * c + n) * p.ldw + 8 * m + 32 * kg;
            const float4 w0 = load_w4(src), w1 = load_w4(src + 4);
            const float f[8] = {w0.x, w0.y, w0.z, w0.w, w1.x, w1.y, w1.z, w1.w};
            gnm_u32x4 p1, p2, p3;
            gnm_split8(f, p1, p2, p3);
            Wp[e] = p1; Wp[E + e] = p2; Wp[2 * E + e] = p3;
        }
    } else {
        for (int idx = tid; idx < KC * O4; idx += NT) {
            const int k = idx / O4, h4 = idx - k * O4;
            *reinterpret_cast<float4*>(Wt + k * HP + 4 * h4) = load_w4(p.W + (size_t)k * p.ldw + 4 * h4);
        }
        __syncthreads();
        for (int e = tid; e < E; e += NT) {
            const int n = e & 31, kg = (e >> 5) & 1, c = (e >> 6) % HT, m = e / (64 * HT);
            float f[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) f[j] = Wt[(8 * m + 32 * kg + j) * HP + 32 * c + n];
            gnm_u32x4 p1, p2, p3;
            gnm_split8(f, p1, p2, p3);
            Wp[e] = p1; Wp[E + e] = p2; Wp[2 * E + e] = p3;
        }
    }
    __builtin_amdgcn_s_waitcnt(0x0F70);           // vmcnt(0): nothing from the preamble is pending inside the tile loop
    __syncthreads();

    GNM_SSTAMP(1)
    double st1[HT], st2[HT];
#pragma unroll
    for (int c = 0; c < HT; ++c) { st1[c] = 0.0; st2[c] = 0.0; }
    int tk = 0;               // (tuning builds: tile counter of the timeline stamps)
    auto do_tile = [&](int t) {
        GNM_SSTAMP(2 + 6 * min(tk, 9))
        const int r0 = t * 32;
        f32x16 acc[HT];
#pragma unroll
        for (int c = 0; c < HT; ++c)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[c][r] = 0.f;
#pragma unroll
        for (int j = 0; j < NLD; ++j) {
            float4 v = __builtin_bit_cast(float4, raw[j]);
            if (pro) {
                v.x = v.x * sc.x + sh.x; v.y = v.y * sc.y + sh.y; v.z = v.z * sc.z + sh.z; v.w = v.w * sc.w + sh.w;
                if (p.pro_relu) {
                    v.x = gnm_relu(v.x); v.y = gnm_relu(v.y); v.z = gnm_relu(v.z); v.w = gnm_relu(v.w);
                }
            }
            *reinterpret_cast<float4*>(Xs + (lrow0 + j * RSTEP) * XS + 4 * c4) = v;
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        GNM_SSTAMP(3 + 6 * min(tk, 9))
        load_tile(t + tstride);                   // past the last tile: an empty descriptor, no memory traffic
        // row i, k = 32 h + 0..31 -> four A fragments (m: k = 8 m + 32 h + 0..7) x three planes, each split right in
        // front of its MFMAs (GNM_L64_SPLIT_AHEAD: all four first, as until round 4 -- 36 more registers, and the
        // splits cannot run in the MFMAs' shadow)
#ifdef GNM_L64_SPLIT_AHEAD
        gnm_u32x4 A1[4], A2[4], A3[4];
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            const float4 v0 = *reinterpret_cast<const float4*>(Xs + i * XS + KH * h + 8 * m);
            const float4 v1 = *reinterpret_cast<const float4*>(Xs + i * XS + KH * h + 8 * m + 4);
            const float f[8] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w};
            gnm_split8(f, A1[m], A2[m], A3[m]);
        }
        GNM_SSTAMP(4 + 6 * min(tk, 9))
#endif
#pragma unroll
        for (int m = 0; m < 4; ++m) {
#ifdef GNM_L64_SPLIT_AHEAD
            const gnm_bf16x8 a1 = __builtin_bit_cast(gnm_bf16x8, A1[m]), a2 = __builtin_bit_cast(gnm_bf16x8, A2[m]),
                             a3 = __builtin_bit_cast(gnm_bf16x8, A3[m]);
#else
            gnm_u32x4 A1m, A2m, A3m;
            {
                const float4 v0 = *reinterpret_cast<const float4*>(Xs + i * XS + KH * h + 8 * m);
                const float4 v1 = *reinterpret_cast<const float4*>(Xs + i * XS + KH * h + 8 * m + 4);
                const float f[8] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w};
                gnm_split8(f, A1m, A2m, A3m);
            }
            const gnm_bf16x8 a1 = __builtin_bit_cast(gnm_bf16x8, A1m), a2 = __builtin_bit_cast(gnm_bf16x8, A2m),
                             a3 = __builtin_bit_cast(gnm_bf16x8, A3m);
#endif
#pragma unroll
            for (int c = 0; c < HT; ++c) gnm_mma6_planes(acc[c], a1, a2, a3, Wp, E, (m * HT + c) * 64 + lane);
        }
        GNM_SSTAMP(5 + 6 * min(tk, 9))
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();          // A fragments are in registers before the staging image is reused
        // (only the launch's last tile can have rows past N: every other tile sums without the per-element row guard --
        //  two selects per element, a fifth of the tile's vector instructions)
        const bool full = r0 + 32 <= p.N;                  // wave-uniform
        float* const xo = Xs + (4 * h) * XS + i;
#pragma unroll
        for (int c = 0; c < HT; ++c) {
            float s1 = 0.f, s2 = 0.f;
            if (full) {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const float z = acc[c][r] + bias_r[c];
                    xo[((r & 3) + 8 * (r >> 2)) * XS + 32 * c] = z;
                    s1 += z;
                    s2 += z * z;
                }
            } else {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int lrow = (r & 3) + 8 * (r >> 2) + 4 * h;
                    const float z = acc[c][r] + bias_r[c];
                    xo[((r & 3) + 8 * (r >> 2)) * XS + 32 * c] = z;
                    if (r0 + lrow < p.N) {
                        s1 += z;
                        s2 += z * z;
                    }
                }
            }
            st1[c] += (double)s1;
            st2[c] += (double)s2;
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        GNM_SSTAMP(6 + 6 * min(tk, 9))
        const __amdgpu_buffer_rsrc_t rz = gnm_tile_rsrc(p.Z + (size_t)r0 * p.ldz, (GNM_L64_ABLATE & 1) ? 0 : min(p.N - r0, 32), p.ldz, HP);
        // (idx = lane + 64 st -> row = lane / O4 + WSTEP st, chunk = lane % O4: one address per lane, the rest immediates)
        const float* const xi = Xs + (lane / O4) * XS + 4 * (lane % O4);
#pragma unroll
        for (int st = 0; st < NST; ++st) {
            const gnm_u32x4 v = *reinterpret_cast<const gnm_u32x4*>(xi + st * WSTEP * XS);
            __builtin_amdgcn_raw_buffer_store_b128(v, rz, out_voff + st * out_step, 0, kStoreStream);     // (row step in the vector offset: see above)
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        GNM_SSTAMP(7 + 6 * min(tk, 9))
        ++tk;
    };

    if (t < ntiles) {
        do_tile(t);
        for (t += tstride; t < ntiles; t += tstride) do_tile(t);
    }
    GNM_SSTAMP(62)

    if (p.stats_partial) {
        __syncthreads();
        double* red = reinterpret_cast<double*>(smem);   // [NW waves][2][HP]
#pragma unroll
        for (int c = 0; c < HT; ++c) {
            const double a1 = st1[c] + __shfl_xor(st1[c], 32, 64);
            const double a2 = st2[c] + __shfl_xor(st2[c], 32, 64);
            if (h == 0) {
                red[(wave * 2 + 0) * HP + 32 * c + i] = a1;
                red[(wave * 2 + 1) * HP + 32 * c + i] = a2;
            }
        }
        __syncthreads();
        // three rows of partials per workgroup (waves 0-3, 4-7, 8-11): gnm_linear_grid(N) rows per launch, as always
        for (int idx = tid; idx < (NW / 4) * 2 * HP; idx += NT) {
            const int grp = idx / (2 * HP), rest = idx - grp * 2 * HP;
            const int which = rest / HP, col = rest - which * HP;
            const int row = blockIdx.x * (NW / 4) + grp;
            if (row >= p.stat_rows) continue;
            double s = 0.0;
            for (int w = 4 * grp; w < 4 * grp + 4; ++w) s += red[(w * 2 + which) * HP + col];
            p.stats_partial[((size_t)row * 2 + which) * p.H + col] = s;
        }
    }
}

template <int HT>
static int launch_lin_split(const LinArgs& a0, int grid, hipStream_t s) {
    LinArgs a = a0;
    a.stat_rows = grid;
    const int grid3 = (grid + kSplitWaves / 4 - 1) / (kSplitWaves / 4);
    constexpr int HP = HT * 32;
    constexpr int XS = (64 > HP ? 64 : HP) + 4;
    const size_t lds = (size_t)3 * 4 * HT * 64 * 16 + (size_t)kSplitWaves * 32 * XS * 4;
    if (lds > (size_t)kLdsBudget) return GNM_ERR_UNSUPPORTED;
    GNM_ALLOW_FULL_LDS((&gnm_lin_split_kernel<HT>));
    hipLaunchKernelGGL((gnm_lin_split_kernel<HT>), dim3(grid3), dim3(kSplitWaves * 64), lds, s, a);
    GNM_CHECK_LAUNCH();
    return GNM_OK;
}

// ---------------------------------------------------------------------------------
// Split-precision Linear for K = 128, H = 128 (round 3: every hidden Linear of BASELINE configs[3], forward and dgrad).
// The fp32-instruction kernels run this shape at 121 us per [256,000 x 128 x 128] launch = 69 TFLOP/s, 44 % of the
// fp32 matrix peak, while moving 2.1 TB/s: matrix-pipe bound.  The K = 64 kernel above does not stretch -- three weight
// planes of [128 x 128] are 98 KB and its per-wave fp32 staging image would be 17 KB: room for 3 waves -- so this one
// keeps the weight planes in LDS and stages the input ONE 16-k SLICE of a tile at a time through a 2.5 KB per-wave
// image: four lanes read a row's 64 contiguous bytes of the slice (16 rows per instruction, whole 64-byte sectors), the
// image is read back in operand order (lane (i, h): row i, k = 16 step + 8 h + 0..7), split in registers (optionally
// after the BatchNorm + ReLU prologue, whose vectors sit in LDS) and multiplied as six bf16 terms against the planes.
// (Round 3 loaded the operands straight from global memory, every lane its own row: 64 requests of 16 useful bytes per
//  instruction, each 128-byte line touched by eight instructions -- the launch ran at 6.8 B/clk per CU where the K = 64
//  kernel, whose loads are row-contiguous, gets 9.5: round 4.)  The next slice -- across tile boundaries too, under the
// epilogue's stores -- is requested before the current one is multiplied.
// Twelve waves per CU (one workgroup; 168 registers), tiles of 32 rows dealt to the waves as in the K = 64 kernel, so
// the launch writes the same gnm_linear_grid(N) rows of statistics partials.  The accumulators are stored as they stand
// (lane = column: 128-byte row segments, 4 bytes per lane).
// ---------------------------------------------------------------------------------
static constexpr int kSplit128Waves = 12;
#ifndef GNM_L128_ABLATE          // tuning builds (tools/build_variant.py -DGNM_L128_ABLATE=n): 1 = no output stores,
#define GNM_L128_ABLATE 0        // 2 = slices come from an empty descriptor (no input traffic)
#endif

template <bool MASKED>
__global__ void __launch_bounds__(kSplit128Waves * 64) gnm_lin_split128_kernel(const LinArgs p) {
    constexpr int K = 128, HT = 4, HP = 128, NW = kSplit128Waves, NT = NW * 64;
    constexpr int E = 2 * 4 * HT * 64;              // 16-byte operand entries per weight plane: [kk][m][c][lane]
    extern __shared__ __attribute__((aligned(16))) char smem[];
    gnm_u32x4* Wp = reinterpret_cast<gnm_u32x4*>(smem);                              // [3][E]
    float* psv = reinterpret_cast<float*>(smem + (size_t)3 * E * 16);        // [3][K]: prologue scale / shift, bias
    // column statistics of this wave, fp64, in LDS ([2][HP] per wave: 16 registers a lane could not spare -- with them
    // in registers the tile loop spilled 21)
    double* wst = reinterpret_cast<double*>(smem + (size_t)3 * E * 16 + 3 * K * 4) + (size_t)(threadIdx.x >> 6) * 2 * HP;
    // the wave's slice image: [32 rows][16 k + 4 floats of padding] (80-byte rows: the 32-byte operand reads of 16
    // consecutive rows fall on 64 distinct banks)
    constexpr int XS = 20;
    float* xs = reinterpret_cast<float*>(smem + (size_t)3 * E * 16 + 3 * K * 4 + (size_t)NW * 2 * HP * 8) +
                (size_t)(threadIdx.x >> 6) * 32 * XS;
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int i = lane & 31;
    const int h = lane >> 5;
    const bool pro = p.pro_scale != nullptr;
    // weight planes: entry (step, c, lane = 32 kg + n) = W[h = 32 c + n][k = 16 step + 8 kg + 0..7]
    for (int e = tid; e < E; e += NT) {
        const int n = e & 31, kg = (e >> 5) & 1, c = (e >> 6) & 3, step = e >> 8;
        const int k0 = 16 * step + 8 * kg, hh = 32 * c + n;
        float f[8];
        if (!p.w_kmajor && (p.ldw & 3) == 0 && (reinterpret_cast<uintptr_t>(p.W) & 15) == 0) {     // (kernel-uniform)
            // torch's layout: the entry's eight k are 32 contiguous bytes of row hh
            const float4 w0 = *reinterpret_cast<const float4*>(p.W + (size_t)hh * p.ldw + k0);
            const float4 w1 = *reinterpret_cast<const float4*>(p.W + (size_t)hh * p.ldw + k0 + 4);
            f[0] = w0.x; f[1] = w0.y; f[2] = w0.z; f[3] = w0.w; f[4] = w1.x; f[5] = w1.y; f[6] = w1.z; f[7] = w1.w;
        } else {
#pragma unroll
            for (int j = 0; j < 8; ++j)
                f[j] = p.w_kmajor ? p.W[(size_t)(k0 + j) * p.ldw + hh] : p.W[(size_t)hh * p.ldw + k0 + j];
        }
        gnm_u32x4 p1, p2, p3;
        gnm_split8(f, p1, p2, p3);
        Wp[e] = p1; Wp[E + e] = p2; Wp[2 * E + e] = p3;
    }
    for (int e = tid; e < K; e += NT) {
        psv[e] = pro ? p.pro_scale[e] : 1.f;
        psv[K + e] = pro ? p.pro_shift[e] : 0.f;
        psv[2 * K + e] = p.bias ? p.bias[e] : 0.f;           // (H == K == 128)
    }
    __builtin_amdgcn_s_waitcnt(0x0F70);           // vmcnt(0): nothing from the preamble is pending inside the tile loop
    __syncthreads();

    const int gw = lin_first_tile(wave, NW / 4, p.stat_rows);
    const int ntiles = (p.N + 31) / 32;
    const int tstride = 4 * p.stat_rows;
    // a slice request: lane -> row (lane >> 2) (+ 16 for the second instruction), 16-byte chunk (lane & 3) of the 64 bytes
    const int ld_voff = ((lane >> 2) * p.ldx + 4 * (lane & 3)) * 4, ld_row16 = 16 * p.ldx * 4;
    float* const xs_w = xs + (lane >> 2) * XS + 4 * (lane & 3);
    const float* const xs_r = xs + i * XS + 8 * h;
    for (int e = lane; e < 2 * HP; e += 64) wst[e] = 0.0;       // (wave-private: no barrier needed)

    auto tile_rsrc_of = [&](int t) {          // (a tile past the end: an empty descriptor, every load returns zeros)
        const int r0 = min(t, ntiles - 1) * 32;
        return gnm_tile_rsrc(p.X + (size_t)r0 * p.ldx, (t < ntiles && !(GNM_L128_ABLATE & 2)) ? min(p.N - r0, 32) : 0, p.ldx, K);
    };
    // Slices are requested D steps ahead into a register ring (slot = slice index mod D): with one slice of 2 KB in
    // flight per wave a CU had 24 KB on its way -- 12 GB/s per CU at the ~2 us a loaded HBM round trip takes, the 3.7 TB/s
    // this kernel ran at; D = 4 (the plain form; the masked form has registers for 2) keeps up to 96 KB in flight.
    constexpr int D = MASKED ? 2 : 4;
    int t = gw;
    gnm_u32x4 ring0[D], ring1[D];
#pragma unroll
    for (int q = 0; q < D; ++q) { ring0[q] = gnm_u32x4{0u, 0u, 0u, 0u}; ring1[q] = ring0[q]; }
    if (t < ntiles) {
        const __amdgpu_buffer_rsrc_t rs0 = tile_rsrc_of(t);
#pragma unroll
        for (int q = 0; q < D; ++q) {
            ring0[q] = __builtin_amdgcn_raw_buffer_load_b128(rs0, ld_voff, q * 64, 0);
            ring1[q] = __builtin_amdgcn_raw_buffer_load_b128(rs0, ld_voff + ld_row16, q * 64, 0);
        }
    }
    // (the first tile is peeled below: the loop is then entered with the queue its back edge carries -- two slice loads
    //  followed by the epilogue's stores -- and the wait for the slice is a counted one instead of a drain of the stores)
    auto do_tile = [&](const int t) {
        const int r0 = t * 32;
        const int rows = min(p.N - r0, 32);
        const __amdgpu_buffer_rsrc_t rs = tile_rsrc_of(t);
        const __amdgpu_buffer_rsrc_t rs_next = tile_rsrc_of(t + tstride);
        f32x16 acc[HT];
#pragma unroll
        for (int c = 0; c < HT; ++c)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[c][r] = 0.f;
        // slice 0 (requested under the previous tile's epilogue) into the image; LDS operations of one wave execute in
        // order, so the image needs no second buffer and no barrier
        *reinterpret_cast<gnm_u32x4*>(xs_w) = ring0[0];
        *reinterpret_cast<gnm_u32x4*>(xs_w + 16 * XS) = ring1[0];
        // eight k steps of 16, unrolled (the ring slots are compile-time) with a scheduling fence per step: left alone,
        // the scheduler hoists every load and split of the 192-MFMA body (295 spilled registers in round 3)
#pragma unroll
        for (int step = 0; step < 8; ++step) {
            __builtin_amdgcn_sched_barrier(0);
            {   // slice step + D -- of the next tile past the end of this one -- into the slot slice `step` has left
                const int sl = step + D;
                const __amdgpu_buffer_rsrc_t rq = sl < 8 ? rs : rs_next;
                ring0[step % D] = __builtin_amdgcn_raw_buffer_load_b128(rq, ld_voff, (sl & 7) * 64, 0);
                ring1[step % D] = __builtin_amdgcn_raw_buffer_load_b128(rq, ld_voff + ld_row16, (sl & 7) * 64, 0);
            }
            const float4 v0 = *reinterpret_cast<const float4*>(xs_r), v1 = *reinterpret_cast<const float4*>(xs_r + 4);
            float f[8] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w};
            if (pro) {
                // (a clipped row read zeros and the affine map moves them: its products land in accumulator rows that
                //  are neither stored nor counted)
                const int k0 = 16 * step + 8 * h;
#pragma unroll
                for (int q = 0; q < 2; ++q) {
                    const float4 sc = *reinterpret_cast<const float4*>(psv + k0 + 4 * q);
                    const float4 sh = *reinterpret_cast<const float4*>(psv + K + k0 + 4 * q);
                    f[4 * q + 0] = f[4 * q + 0] * sc.x + sh.x; f[4 * q + 1] = f[4 * q + 1] * sc.y + sh.y;
                    f[4 * q + 2] = f[4 * q + 2] * sc.z + sh.z; f[4 * q + 3] = f[4 * q + 3] * sc.w + sh.w;
                }
                if (p.pro_relu) {
#pragma unroll
                    for (int j = 0; j < 8; ++j) f[j] = gnm_relu(f[j]);
                }
            }
            gnm_u32x4 A1, A2, A3;
            gnm_split8(f, A1, A2, A3);
            const gnm_bf16x8 a1 = __builtin_bit_cast(gnm_bf16x8, A1), a2 = __builtin_bit_cast(gnm_bf16x8, A2),
                             a3 = __builtin_bit_cast(gnm_bf16x8, A3);
#pragma unroll
            for (int c = 0; c < HT; ++c) gnm_mma6_planes(acc[c], a1, a2, a3, Wp, E, ((step * HT + c) << 6) + lane);
            if (step < 7) {       // the next slice into the image (behind this step's reads, in order)
                *reinterpret_cast<gnm_u32x4*>(xs_w) = ring0[(step + 1) % D];
                *reinterpret_cast<gnm_u32x4*>(xs_w + 16 * XS) = ring1[(step + 1) % D];
            }
        }
        __builtin_amdgcn_sched_barrier(0);
        // ---- epilogue: bias, column statistics, stores (lane = column; rows past N clipped by the descriptor) ----
        const __amdgpu_buffer_rsrc_t rz = gnm_tile_rsrc(p.Z + (size_t)r0 * p.ldz, (GNM_L128_ABLATE & 1) ? 0 : rows, p.ldz, HP);
        if constexpr (MASKED) {
            // masked dX: the values under the accumulators of the lower BatchNorm's input (lane = column: 128-byte row
            // pieces), one column block requested ahead of the one being finished
            const __amdgpu_buffer_rsrc_t rm = gnm_tile_rsrc(p.mZ + (size_t)r0 * p.ldmz, rows, p.ldmz, HP);
            // (one vector offset per lane and the (row, column block) part in the scalar offset: with a vector offset per
            //  element the compiler kept 128 of them across the tile loop -- 77 spilled registers)
            const unsigned mvo = (unsigned)((4 * h * p.ldmz + i) * 4), zvo = (unsigned)((4 * h * p.ldz + i) * 4);
            float zm[2][16];
            auto req = [&](float (&d)[16], int c) {
#pragma unroll
                for (int r = 0; r < 16; ++r)
                    d[r] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(
                        rm, mvo, (((r & 3) + 8 * (r >> 2)) * p.ldmz + 32 * c) * 4, 0));
            };
            __builtin_amdgcn_sched_barrier(0);            // (hoisted into the product loop these requests spilled 77 registers)
            req(zm[0], 0);
#pragma unroll
            for (int c = 0; c < HT; ++c) {
                if (c + 1 < HT) req(zm[(c + 1) & 1], c + 1);
                __builtin_amdgcn_sched_barrier(0);
                const int col = 32 * c + i;
                const float msc = p.m_scale[col], msh = p.m_shift[col], mmu = p.m_mean[col];
                float s1 = 0.f, s2 = 0.f;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int lrow = (r & 3) + 8 * (r >> 2) + 4 * h;
                    const float zv = zm[c & 1][r];
                    float g = acc[c][r];
                    if (zv * msc + msh <= 0.f) g = 0.f;
                    __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(g), rz, zvo, (((r & 3) + 8 * (r >> 2)) * p.ldz + 32 * c) * 4, 0);
                    if (lrow < rows) {
                        s1 += g;
                        s2 += g * (zv - mmu);
                    }
                }
                s1 += __shfl_xor(s1, 32, 64);
                s2 += __shfl_xor(s2, 32, 64);
                if (h == 0) {
                    wst[col] += (double)s1;
                    wst[HP + col] += (double)s2 * (double)p.m_rstd[col];      // sum G (Z - mean) rstd = sum G xhat
                }
            }
        } else {
        // (one vector offset per lane, the (row, column block) part in the scalar offset: a vector offset per store is 64
        //  registers the compiler keeps -- and spills -- across the tile loop)
        const unsigned zvo = (unsigned)((4 * h * p.ldz + i) * 4);
#pragma unroll
        for (int c = 0; c < HT; ++c) {
            float s1 = 0.f, s2 = 0.f;
            const float bz = psv[2 * K + 32 * c + i];
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int lrow = (r & 3) + 8 * (r >> 2) + 4 * h;
                const float z = acc[c][r] + bz;
                __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(z), rz, zvo, (((r & 3) + 8 * (r >> 2)) * p.ldz + 32 * c) * 4, 0);
                if (lrow < rows) {
                    s1 += z;
                    s2 += z * z;
                }
            }
            s1 += __shfl_xor(s1, 32, 64);
            s2 += __shfl_xor(s2, 32, 64);
            if (h == 0) {
                wst[32 * c + i] += (double)s1;
                wst[HP + 32 * c + i] += (double)s2;
            }
        }
        }
    };
    if (t < ntiles) {
        do_tile(t);
        for (t += tstride; t < ntiles; t += tstride) do_tile(t);
    }

    if (p.stats_partial) {
        const double* red = reinterpret_cast<const double*>(smem + (size_t)3 * E * 16 + 3 * K * 4);   // [NW waves][2][HP]
        __syncthreads();
        for (int idx = tid; idx < 3 * 2 * HP; idx += NT) {        // three rows of partials per workgroup, as above
            const int grp = idx / (2 * HP), rest = idx - grp * 2 * HP;
            const int which = rest / HP, col = rest - which * HP;
            const int row = blockIdx.x * 3 + grp;
            if (row >= p.stat_rows) continue;
            double sacc = 0.0;
            for (int w = 4 * grp; w < 4 * grp + 4; ++w) sacc += red[(w * 2 + which) * HP + col];
            p.stats_partial[((size_t)row * 2 + which) * p.H + col] = sacc;
        }
    }
}

static int launch_lin_split128(const LinArgs& a0, int grid, hipStream_t s) {
    LinArgs a = a0;
    a.stat_rows = grid;
    const int grid3 = (grid + 2) / 3;
    const size_t lds = (size_t)3 * (2 * 4 * 4 * 64) * 16 + (size_t)3 * 128 * 4 + (size_t)kSplit128Waves * 2 * 128 * 8 +
                       (size_t)kSplit128Waves * 32 * 20 * 4;          // planes, prologue vectors, statistics, slice images
    if (a.mZ) {
        GNM_ALLOW_FULL_LDS((&gnm_lin_split128_kernel<true>));
        hipLaunchKernelGGL(gnm_lin_split128_kernel<true>, dim3(grid3), dim3(kSplit128Waves * 64), lds, s, a);
    } else {
        GNM_ALLOW_FULL_LDS((&gnm_lin_split128_kernel<false>));
        hipLaunchKernelGGL(gnm_lin_split128_kernel<false>, dim3(grid3), dim3(kSplit128Waves * 64), lds, s, a);
    }
    GNM_CHECK_LAUNCH();
    return GNM_OK;
}

// gnm_lin_kernel's LDS: the zero-padded weight image and the four waves' input chunks ...
static size_t lin_image_bytes(int K, int KC, int HT) {
    const int KP = ((K + KC - 1) / KC) * KC;
    return (size_t)KP * HT * 32 * 4 + (size_t)4 * 32 * (KC + 4) * 4;
}
// ... or the statistics combine that reuses it, whichever is larger
static size_t lin_lds_bytes(int K, int KC, int HT) {
    const size_t b = lin_image_bytes(K, KC, HT), red = (size_t)4 * 2 * HT * 32 * 8;
    return b > red ? b : red;
}

template <int KC, int HT>
static int launch_lin(const LinArgs& a0, int grid, hipStream_t s) {
    LinArgs a = a0;
    size_t lds = lin_lds_bytes(a.K, KC, HT);
    if (lds > (size_t)kLdsBudget) return GNM_ERR_UNSUPPORTED;
    // room for the output staging image (a wide first layer, K = 400 one-hot, has none: 4-byte column stores then)
    const size_t wbytes = lin_image_bytes(a.K, KC, HT);
    const size_t obytes = (size_t)4 * 32 * (HT * 32 + 4) * 4;
    a.stage_out = wbytes + obytes <= (size_t)kLdsBudget / 2 ? 1 : 0;      // only while two workgroups still share a CU
    if (a.stage_out && wbytes + obytes > lds) lds = wbytes + obytes;
    GNM_ALLOW_FULL_LDS((&gnm_lin_kernel<KC, HT>));
    hipLaunchKernelGGL((gnm_lin_kernel<KC, HT>), dim3(grid), dim3(256), lds, s, a);
    GNM_CHECK_LAUNCH();
    return GNM_OK;
}

// Largest input width K that gnm_linear_fwd accepts for output width H (the weight [K x H] stays in LDS for the
// kernel's lifetime): what a caller checks before building a model around it.  0 when H itself is unsupported.
extern "C" int gnm_linear_max_k(int H) {
    if (H <= 0 || H > 128) return 0;
    const int HT = (H + 31) / 32;
    int k = 0;
    while (lin_lds_bytes(k + 64, 64, HT) <= (size_t)kLdsBudget) k += 64;
    return k;
}

// Blocks gnm_linear_fwd launches for N rows (= rows of stats_partial it writes).
extern "C" int gnm_linear_grid(int N) {
    const int ntiles = (N + 31) / 32;
    int g = (ntiles + 3) / 4;
    static const int cap = gnm_env_int("GNM_LIN_GRID", 768);   // tuning knob
    if (g > cap) g = cap;
    return g < 1 ? 1 : g;
}

// Z[N,H] = f(X)[N,K] * W^T + bias, f = optional fused affine(+ReLU) prologue; optional
// per-column (sum, sum of squares) partials for the following BatchNorm.
extern "C" int gnm_linear_fwd(const float* X, int ldx, const float* W, int ldw, int w_kmajor, const float* bias,
                              float* Z, int ldz, int N, int K, int H, const float* pro_scale,
                              const float* pro_shift, int pro_relu, double* stats_partial, void* stream) {
    if (N <= 0) return GNM_OK;
    if (K <= 0 || H <= 0 || H > 128) return GNM_ERR_BAD_ARG;
    const LinArgs a = lin_args(X, ldx, W, ldw, w_kmajor, bias, Z, ldz, N, K, H, pro_scale, pro_shift, pro_relu, stats_partial);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const int grid = gnm_linear_grid(N);
    const int HT = (H + 31) / 32;
    const int kc = K <= 8 ? 8 : (K <= 16 ? 16 : (K <= 32 ? 32 : 64));
    // pipelined variant: aligned rows in and out, no partial chunks or partial output tiles
    const bool aligned = ((ldx & 3) == 0) && ((ldz & 3) == 0) && ((reinterpret_cast<uintptr_t>(X) & 15) == 0) &&
                         ((reinterpret_cast<uintptr_t>(Z) & 15) == 0) &&
                         (!pro_scale || (((reinterpret_cast<uintptr_t>(pro_scale) | reinterpret_cast<uintptr_t>(pro_shift)) & 15) == 0));
    if (aligned && (H % 32) == 0 && (K % 32) == 0 && !lin_force_generic()) {
        const int kcf = (K % 64) == 0 ? 64 : 32;
        int rc = GNM_ERR_UNSUPPORTED;
        // one chunk per row and descriptors that fit 32-bit offsets: the streaming kernel
        const bool small_ld = (long long)ldx * 32 * 4 < (1LL << 31) && (long long)ldz * 32 * 4 < (1LL << 31);
        // K = H = 64: the split-precision kernel
        if (K == 64 && HT == 2 && small_ld && !lin_no_stream() && !lin_no_split()) {
            rc = launch_lin_split<2>(a, grid, s);
            if (rc != GNM_ERR_UNSUPPORTED) return rc;
        }
        // K = H = 128 (configs[3]): its own split-precision kernel
        if (K == 128 && H == 128 && small_ld && !lin_no_split()) return launch_lin_split128(a, grid, s);
        if ((K == 32 || K == 64) && small_ld && !lin_no_stream()) {
#define GNM_LINS_CASE(KC_, HT_) if (K == KC_ && HT == HT_) rc = launch_lin_stream<KC_, HT_>(a, grid, s);
            GNM_LINS_CASE(32, 1) GNM_LINS_CASE(32, 2) GNM_LINS_CASE(32, 3) GNM_LINS_CASE(32, 4)
            GNM_LINS_CASE(64, 1) GNM_LINS_CASE(64, 2) GNM_LINS_CASE(64, 3) GNM_LINS_CASE(64, 4)
#undef GNM_LINS_CASE
            if (rc != GNM_ERR_UNSUPPORTED) return rc;
        }
#define GNM_LINF_CASE(KC_, HT_) if (kcf == KC_ && HT == HT_) rc = launch_lin_fast<KC_, HT_>(a, grid, s);
        GNM_LINF_CASE(32, 1) GNM_LINF_CASE(32, 2) GNM_LINF_CASE(32, 3) GNM_LINF_CASE(32, 4)
        GNM_LINF_CASE(64, 1) GNM_LINF_CASE(64, 2) GNM_LINF_CASE(64, 3) GNM_LINF_CASE(64, 4)
#undef GNM_LINF_CASE
        if (rc != GNM_ERR_UNSUPPORTED) return rc;      // too large for LDS: fall through to the generic kernel
    }
#define GNM_LIN_CASE(KC_, HT_) if (kc == KC_ && HT == HT_) return launch_lin<KC_, HT_>(a, grid, s);
    GNM_LIN_CASE(8, 1) GNM_LIN_CASE(8, 2) GNM_LIN_CASE(8, 3) GNM_LIN_CASE(8, 4)
    GNM_LIN_CASE(16, 1) GNM_LIN_CASE(16, 2) GNM_LIN_CASE(16, 3) GNM_LIN_CASE(16, 4)
    GNM_LIN_CASE(32, 1) GNM_LIN_CASE(32, 2) GNM_LIN_CASE(32, 3) GNM_LIN_CASE(32, 4)
    GNM_LIN_CASE(64, 1) GNM_LIN_CASE(64, 2) GNM_LIN_CASE(64, 3) GNM_LIN_CASE(64, 4)
#undef GNM_LIN_CASE
    return GNM_ERR_UNSUPPORTED;
}

// dX = dZ W for a K = H = 128 Linear whose input came through BatchNorm + ReLU (mlp.py:48), with that ReLU's mask and
// that BatchNorm's backward sums taken on the way out (replaces gnm_linear_fwd(w_kmajor = 1) + gnm_bn_relu_bwd_stats for
// the inner BatchNorms of an H = 128 model; the K = H = 64 shapes have gnm_linear_bwd_fused):
//     G[n, k] = (dZ W)[n, k] if relu(mZ[n, k] m_scale[k] + m_shift[k]) > 0 else 0
//     stats_partial[row][0][k] = partial sum G,  [1][k] = partial sum G (mZ - m_mean) m_rstd     (gnm_linear_grid(N) rows)
// dZ [N, H = 128], W [H][K = 128] row-major (the Linear's weight), G [N, K].  GNM_ERR_UNSUPPORTED for other shapes.
extern "C" int gnm_linear_dgrad_masked(const float* dZ, int ldd, const float* W, int ldw, float* G, int ldg, int N, int K,
                                       int H, const float* mZ, int ldmz, const float* m_scale, const float* m_shift,
                                       const float* m_mean, const float* m_rstd, double* stats_partial, void* stream) {
    if (N <= 0) return GNM_OK;
    if (K != 128 || H != 128 || lin_no_split() || lin_force_generic()) return GNM_ERR_UNSUPPORTED;
    if (!dZ || !W || !G || !mZ || !m_scale || !m_shift || !m_mean || !m_rstd || !stats_partial) return GNM_ERR_BAD_ARG;
    if ((ldd & 3) || (reinterpret_cast<uintptr_t>(dZ) & 15)) return GNM_ERR_UNSUPPORTED;
    if ((long long)(ldd > ldg ? (ldd > ldmz ? ldd : ldmz) : (ldg > ldmz ? ldg : ldmz)) * 32 * 4 >= (1LL << 31)) return GNM_ERR_UNSUPPORTED;
    LinArgs a = lin_args(dZ, ldd, W, ldw, 1, nullptr, G, ldg, N, H, K, nullptr, nullptr, 0, stats_partial);
    a.mZ = mZ; a.m_scale = m_scale; a.m_shift = m_shift; a.m_mean = m_mean; a.m_rstd = m_rstd; a.ldmz = ldmz;
    return launch_lin_split128(a, gnm_linear_grid(N), reinterpret_cast<hipStream_t>(stream));
}
