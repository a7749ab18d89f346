// The project's "fp32-faithful on the bf16 pipe" arithmetic, in one place: the exact three-plane bf16 split of an fp32
// value and the six-term matrix product built on it (v_mfma_f32_32x32x16_bf16, 16x the rate of the fp32 instruction).
// Every kernel that multiplies this way -- the eval kernels through gnm_tile_step, the training kernels of linear*.hip
// through gnm_mma6 / gnm_mma6_planes -- includes this header and issues the product nowhere else; a change here changes
// all of them together.
#pragma once
#include "gnm_common.h"

typedef __bf16 gnm_bf16x8 __attribute__((ext_vector_type(8)));
typedef unsigned int gnm_u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int gnm_u32x2 __attribute__((ext_vector_type(2)));

// f = a1 + a2 + a3 EXACTLY, by truncation (8 + 8 + 8 mantissa bits); each plane is the TOP half of its word
__device__ __forceinline__ void gnm_split3(const float f, unsigned& a1, unsigned& a2, unsigned& a3) {
    a1 = __float_as_uint(f) & 0xFFFF0000u;
    const float r1 = f - __uint_as_float(a1);
    a2 = __float_as_uint(r1) & 0xFFFF0000u;
    a3 = __float_as_uint(r1 - __uint_as_float(a2));        // <= 8 significant bits left: its top half is all of it
}
// (top 16 bits of hi_word) : (top 16 bits of lo_word)
__device__ __forceinline__ unsigned gnm_bf16_pair(unsigned lo_word, unsigned hi_word) {
    return __builtin_amdgcn_perm(hi_word, lo_word, 0x07060302u);
}
// eight consecutive-k floats -> the three bf16x8 operands, as words (staging through LDS) ...
__device__ __forceinline__ void gnm_split8(const float* f, gnm_u32x4& p1, gnm_u32x4& p2, gnm_u32x4& p3) {
    unsigned a1[8], a2[8], a3[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) gnm_split3(f[j], a1[j], a2[j], a3[j]);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        p1[j] = gnm_bf16_pair(a1[2 * j], a1[2 * j + 1]);
        p2[j] = gnm_bf16_pair(a2[2 * j], a2[2 * j + 1]);
        p3[j] = gnm_bf16_pair(a3[2 * j], a3[2 * j + 1]);
    }
}
// ... or as the matrix instruction's operand type
__device__ __forceinline__ void gnm_split8(const float* f, gnm_bf16x8& p1, gnm_bf16x8& p2, gnm_bf16x8& p3) {
    gnm_u32x4 q1, q2, q3;
    gnm_split8(f, q1, q2, q3);
    p1 = __builtin_bit_cast(gnm_bf16x8, q1); p2 = __builtin_bit_cast(gnm_bf16x8, q2); p3 = __builtin_bit_cast(gnm_bf16x8, q3);
}

// acc += (a1 + a2 + a3) x (b1 + b2 + b3) without the terms a2 b3, a3 b2, a3 b3: every partial product kept is exact in
// the fp32 accumulator, and the three dropped ones are below 2^-24 of |a||b| each -- the size of the accumulator's own
// rounding.  Small terms first.  The order is part of every result's bits: do not change it.
__device__ __forceinline__ void gnm_mma6(f32x16& acc, const gnm_bf16x8 a1, const gnm_bf16x8 a2, const gnm_bf16x8 a3,
                                         const gnm_bf16x8 b1, const gnm_bf16x8 b2, const gnm_bf16x8 b3) {
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1, b3, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a3, b1, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a2, b2, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1, b2, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a2, b1, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1, b1, acc, 0, 0, 0);
}

// The same with the B operand taken from a three-plane LDS image (plane stride ew entries), entry e
__device__ __forceinline__ void gnm_mma6_planes(f32x16& acc, const gnm_bf16x8 a1, const gnm_bf16x8 a2, const gnm_bf16x8 a3,
                                                const gnm_u32x4* Wp, int ew, int e) {
    gnm_mma6(acc, a1, a2, a3, __builtin_bit_cast(gnm_bf16x8, Wp[e]), __builtin_bit_cast(gnm_bf16x8, Wp[ew + e]),
             __builtin_bit_cast(gnm_bf16x8, Wp[2 * ew + e]));
}
// Eight consecutive floats at a 16-byte aligned address (an LDS tile row) -> the three operands
__device__ __forceinline__ void gnm_load_split8(const float* src, gnm_bf16x8& a1, gnm_bf16x8& a2, gnm_bf16x8& a3) {
    const float4 v0 = *reinterpret_cast<const float4*>(src), v1 = *reinterpret_cast<const float4*>(src + 4);
    const float f[8] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w};
    gnm_split8(f, a1, a2, a3);
}

// The A operand of step s from a 32-row LDS tile T of row stride ts floats: row i of the lane, k = 16 s + 8 h + 0..7
__device__ __forceinline__ void gnm_tile_split(const float* T, int ts, int i, int h, int s, gnm_bf16x8& a1, gnm_bf16x8& a2,
                                               gnm_bf16x8& a3) {
    const int k0 = 16 * s + 8 * h;
    float fa[8];
    const float4 v0 = *reinterpret_cast<const float4*>(T + i * ts + k0);
    const float4 v1 = *reinterpret_cast<const float4*>(T + i * ts + k0 + 4);
    fa[0] = v0.x; fa[1] = v0.y; fa[2] = v0.z; fa[3] = v0.w; fa[4] = v1.x; fa[5] = v1.y; fa[6] = v1.z; fa[7] = v1.w;
    gnm_split8(fa, a1, a2, a3);
}
// acc += T[32 x 16 s ..] x B[16 s .., col]: A from the LDS tile, B = eight consecutive k of the lane's column, in fb
__device__ __forceinline__ void gnm_tile_step(f32x16& acc, const float* T, int ts, int i, int h, int s, const float (&fb)[8]) {
    gnm_bf16x8 a1, a2, a3, b1, b2, b3;
    gnm_tile_split(T, ts, i, h, s, a1, a2, a3);
    gnm_split8(fb, b1, b2, b3);
    gnm_mma6(acc, a1, a2, a3, b1, b2, b3);
}
