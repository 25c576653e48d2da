// Device helpers the tap-GEMM kernel families share (conv_dma.hip, conv_halo.hip, conv_wreg.hip, conv_wreg_f32.hip, conv_phase4.hip): the
// pieces of the gsum epilogue and the MFMA step on one 16-byte fragment per operand tile.
#pragma once
#include "tapgemm.h"

// which part of a split output a channel belongs to, its channel index inside the part and the part's channel count
__device__ __forceinline__ int gsum_part(const TapGemmArgs& a, int n, int& nl, int& pc) {
    const int p = n < a.n1 ? 0 : 1;
    nl = p ? n - a.n1 : n;
    pc = p ? a.nout - a.n1 : a.n1;
    return p;
}

// value of the activation-typed tensor `aux` (float or bf16) as float
template <typename T>
__device__ __forceinline__ float gsum_aux(const void* aux, size_t idx) {
    return (float)((const T*)aux)[idx];
}

// LDS-staged (bf16) epilogues: a lane holds eight consecutive channels of one pixel as stored (v) and loads the same eight of
// aux (16 bytes); per-lane partial sums over the rows the lane visits
__device__ __forceinline__ void gsum_wide_accum(const u32x4& v, const u32x4& av, float (&t1)[8], float (&t2)[8]) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const float v0 = __uint_as_float(v[e] << 16), v1 = __uint_as_float(v[e] & 0xffff0000u);
        const float a0 = __uint_as_float(av[e] << 16), a1 = __uint_as_float(av[e] & 0xffff0000u);
        t1[2 * e] += v0;
        t1[2 * e + 1] += v1;
        t2[2 * e] += v0 * a0;
        t2[2 * e + 1] += v1 * a1;
    }
}

// CW = 4 (a wave tile of 32 channels: lane = 4 rr + ch): reduce-scatter of the sixteen per-lane sums over the sixteen lanes rr that
// share a channel group -- fifteen shuffles instead of 64, no values carried across patches -- after which lane (rr, ch) holds the
// wave's total of ONE (moment, channel) pair: moment rr >> 3, channel 8 ch + (rr & 7).  One 64-lane atomic instruction per call.
__device__ __forceinline__ float gsum_scatter16(float (&t1)[8], float (&t2)[8], int lane) {
    float v[16];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        v[e] = t1[e];
        v[8 + e] = t2[e];
    }
    // step s (lane bit 5, 4, 3, 2): keep the half of the remaining values selected by that bit, add the partner's copy of them
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        const int half = 8 >> s, bit = 32 >> s;
        const bool up = (lane & bit) != 0;
#pragma unroll
        for (int e = 0; e < half; ++e) {
            const float keep = up ? v[half + e] : v[e];
            const float send = up ? v[e] : v[half + e];
            v[e] = keep + __shfl_xor(send, bit, 64);
        }
    }
    return v[0];          // value index = lane >> 2 (step s fixes index bit 3 - s from lane bit 5 - s)
}

// ... combined over the lanes that hold the same channels (lane % CW equal) and added to dst[(channel) * 2 + {0, 1}]
template <int CW>
__device__ __forceinline__ void gsum_wide_flush(float (&t1)[8], float (&t2)[8], int lane, double* dst) {
#pragma unroll
    for (int e = 0; e < 8; ++e) {
#pragma unroll
        for (int o = CW; o < 64; o <<= 1) {
            t1[e] += __shfl_xor(t1[e], o, 64);
            t2[e] += __shfl_xor(t2[e], o, 64);
        }
    }
    if (lane < CW && dst) {
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            atomicAdd(dst + 2 * e, (double)t1[e]);
            atomicAdd(dst + 2 * e + 1, (double)t2[e]);
        }
    }
}

// One 16-byte fragment per operand tile: four f32 MFMAs (K = 2 each) or one bf16 MFMA (K = 16).
template <typename T, int TM, int TN>
__device__ __forceinline__ void tap_mfma(const f32x4 (&av)[TM], const f32x4 (&bv)[TN], f32x16 (&acc)[TM][TN]) {
    if constexpr (sizeof(T) == 4) {
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[i][e], bv[j][e], acc[i][j], 0, 0, 0);
    } else {
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j)
                acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, av[i]), __builtin_bit_cast(bf16x8, bv[j]),
                                                                   acc[i][j], 0, 0, 0);
    }
}
