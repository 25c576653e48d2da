// Developing a polariser mosaic inside the demosaic launch: black level, white balance, colour matrix and tone curve applied to the
// UNROUNDED channel numerators, before the cut to 8 bits (include/shmgan_hip.h states the arithmetic).
//
//   shm_dofp_develop   shm_dofp_views' launch geometry and tap walk (dofp_dev.h: df_numerators), another finish.  Per output byte: a
//                      subtract-and-hold, the product D M, a funnel shift, the rounding add, a hold and one table read.  D < 2^23 always;
//                      M < 2^36 is split into its low 24 bits and the 12 above.  When the high part is 0 for every channel -- the kernel
//                      tests that once, on uniform values -- the product is one 24 x 24 -> 48-bit multiply (two full-rate instructions);
//                      otherwise a third 24-bit multiply adds the high part (dv_lin).  No 32- or 64-bit multiplier anywhere.  Which side a
//                      sensor is on follows from its depth: mul = 65535 * 65536 wb / (white - black) is at least 2^24 for every 8-bit
//                      sensor, so uint8 sources instantiate the three-multiply side only; a 10-bit one crosses at a combined gain of about 4,
//                      a 12-bit one at about 15, a 16-bit one never within the gains the header allows.  The parameter block is read through
//                      uniform addresses, so it and the multipliers live in scalar registers.  The tone table (4 KB) is copied into
//                      LDS once per block, 16 bytes per thread: 60 (colour) or 20 (mono) byte reads per thread at data-dependent
//                      addresses would otherwise each be a vector-memory access; in LDS neighbouring pixels, whose values are close, mostly
//                      fall into one dword and are served as a broadcast.  The matrix is a uniform branch: three signed 24-bit multiplies
//                      per channel.
//   shm_dofp_wb_gray   two launches: per-block sums over a grid-stride walk of the 4 x 4 periods, then one block that adds the
//                      per-block sums, finishes the gains and writes the parameter block the development reads.  The sums are integers
//                      below 2^53, where addition in double is exact, so shm_block_sum's fixed order is not even needed for equal bits.
#include "dofp_dev.h"

namespace {

struct DvParams {                                // uniform: scalar registers
    unsigned black[3];
    unsigned Ml[3], Mh[3];                       // M = Mh 2^24 + Ml, Ml < 2^24, Mh < 2^12
    int ccm[9];
};

// lin of one numerator: steps 1 and 3 of the header.  bk = black << K; D < 2^23; S - 1 = 15 + K lies in 15 .. 22.
//   (P + 2^(S-1)) >> S == ((P >> (S-1)) + 1) >> 1                      for every P
//   WIDE == false: Mh == 0, P = D Ml < 2^47, so P >> (S-1) fits 32 bits.
//   WIDE == true:  P = a + b 2^24 with a = D Ml and b = D Mh.  2^24 is a multiple of 2^(S-1), so P >> (S-1) == (a >> (S-1)) + (b << (25 - S))
//                  exactly.  Anything from 2^17 up ends at 65535, so each term is first held at 2^20, which keeps every intermediate
//                  inside 32 bits and changes no result: D is held before the multiply (D Mh >= 2^20 either way once D >= 2^20 and
//                  Mh >= 1; 2^20 * 4095 < 2^32), then b, then a >> (S-1).
template <int K, bool WIDE>
__device__ __forceinline__ unsigned dv_lin(unsigned n, unsigned bk, unsigned Ml, unsigned Mh) {
    constexpr int S = 16 + K;
    static_assert(S - 1 >= 15 && S - 1 <= 24, "the shift the two identities above rely on");
    const unsigned D = n > bk ? n - bk : 0u;
    const unsigned long long a = (unsigned long long)(D & 0xffffffu) * (unsigned long long)(Ml & 0xffffffu);
    unsigned q = (unsigned)(a >> (S - 1));
    if (WIDE) {
        const unsigned hold = 1u << 20;
        const unsigned b = __umul24(D < hold ? D : hold, Mh);
        q = (q < hold ? q : hold) + ((b < hold ? b : hold) << (25 - S));
    }
    const unsigned v = (q + 1u) >> 1;
    return v > 65535u ? 65535u : v;
}

__device__ __forceinline__ unsigned dv_clamp16(int v) { return v < 0 ? 0u : v > 65535 ? 65535u : (unsigned)v; }

// one plane's four pixels from their numerators n[channel][pixel]; KT: 0 for a view, 2 for the total
template <int NCH, int KB, int KT, bool WIDE, bool CCM>
__device__ __forceinline__ void dv_plane(unsigned char* p, const unsigned (&n)[NCH][4], const DvParams& q, const unsigned char* lut, int nvalid) {
    unsigned o[3][4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if (NCH == 1) {
            o[0][j] = o[1][j] = o[2][j] = lut[dv_lin<KB + KT, WIDE>(n[0][j], q.black[0] << (KB + KT), q.Ml[0], q.Mh[0]) >> 4];
        } else {
            unsigned lin[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                constexpr int G = 1;
                const int k = KB + KT + (c == G ? 1 : 0);
                lin[c] = c == G ? dv_lin<KB + KT + 1, WIDE>(n[c][j], q.black[c] << k, q.Ml[c], q.Mh[c]) : dv_lin<KB + KT, WIDE>(n[c][j], q.black[c] << k, q.Ml[c], q.Mh[c]);
            }
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                unsigned v = lin[c];
                if (CCM)          // |ccm| < 2^13 and lin < 2^16: the signed 24-bit multiplier is exact and the sum stays inside 32 bits
                    v = dv_clamp16((__mul24(q.ccm[3 * c], (int)lin[0]) + __mul24(q.ccm[3 * c + 1], (int)lin[1]) + __mul24(q.ccm[3 * c + 2], (int)lin[2]) + 512) >> 10);
                o[c][j] = lut[v >> 4];
            }
        }
    }
    df_store4(p, o[0], o[1], o[2], nvalid);
}

template <int NCH, int KB, bool WIDE, bool CCM>
__device__ __forceinline__ void dv_planes(const DofpArgs& a, const unsigned (&acc)[4][NCH][4], const DvParams& q, const unsigned char* lut, size_t off,
                                          int nvalid) {
    unsigned tot[NCH][4];
#pragma unroll
    for (int c = 0; c < NCH; ++c)
#pragma unroll
        for (int j = 0; j < 4; ++j) tot[c][j] = (acc[0][c][j] + acc[1][c][j]) + (acc[2][c][j] + acc[3][c][j]);
#pragma unroll
    for (int p = 0; p < 4; ++p) dv_plane<NCH, KB, 0, WIDE, CCM>(a.plane[p] + off, acc[p], q, lut, nvalid);
    if (a.total) dv_plane<NCH, KB, 2, WIDE, CCM>(a.total + off, tot, q, lut, nvalid);
}

// Five waves per SIMD (at most 96 VGPRs): left alone the allocator takes 97 .. 101 on some Bayer instances, one granule past that, and the kernel,
// which is bound by its arithmetic and hides its loads behind other waves, runs 5 % slower at four.  No instance spills under the limit.
template <int PATTERN, int MODE, typename T>
__global__ void __launch_bounds__(DF_BX* DF_BY) __attribute__((amdgpu_waves_per_eu(5))) dofp_develop_kernel(const DofpArgs a, const T* __restrict__ src, int h, int w, size_t pitch, int ho,
                                                                     int wo, int aligned, const int* __restrict__ params,
                                                                     const uint4* __restrict__ lut) {
    constexpr int P = PATTERN == SHM_DOFP_MONO ? 2 : 4;
    constexpr int NCH = PATTERN == SHM_DOFP_MONO ? 1 : 3;
    constexpr int KB = MODE == SHM_DOFP_BILINEAR ? (P == 4 ? 4 : 2) : 0;
    static_assert(DF_BX * DF_BY * 16 == SHM_DOFP_LUT, "one 16-byte piece of the table per thread");
    __shared__ uint4 s_lut[SHM_DOFP_LUT / 16];
    const int tid = threadIdx.y * DF_BX + threadIdx.x;
    s_lut[tid] = lut[tid];
    __syncthreads();
    const int y = blockIdx.y * DF_BY + threadIdx.y;
    const int xg = 4 * (blockIdx.x * DF_BX + threadIdx.x);
    if (y >= ho || xg >= wo) return;
    DvParams q;
    bool wide = false;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        q.black[c] = (unsigned)params[SHM_DOFP_P_BLACK + c];
        const unsigned long long M =
            ((unsigned long long)(unsigned)params[SHM_DOFP_P_MUL + c] * (unsigned long long)(unsigned)params[SHM_DOFP_P_GAIN + c] + 512ull) >> 10;
        q.Ml[c] = (unsigned)M & 0xffffffu;
        q.Mh[c] = (M >> 24) > 4095ull ? 4095u : (unsigned)(M >> 24);          // a gain beyond the header's 16383 saturates; it cannot reach memory
        wide = wide || (c < NCH && q.Mh[c] != 0u);
    }
    const bool ccm = NCH == 3 && (params[SHM_DOFP_P_FLAGS] & 1);
#pragma unroll
    for (int i = 0; i < 9; ++i) q.ccm[i] = params[SHM_DOFP_P_CCM + i];
    unsigned acc[4][NCH][4];
#pragma unroll
    for (int p = 0; p < 4; ++p)
#pragma unroll
        for (int c = 0; c < NCH; ++c)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[p][c][j] = 0u;
    const bool fast = aligned && (MODE == SHM_DOFP_BILINEAR ? (xg >= 4 && xg + 7 < w) : (xg + 4 <= wo));
    if (fast)
        df_numerators<PATTERN, MODE, T, true, NCH>(acc, src, h, w, pitch, y, xg, wo);
    else
        df_numerators<PATTERN, MODE, T, false, NCH>(acc, src, h, w, pitch, y, xg, wo);
    const int nvalid = wo - xg < 4 ? wo - xg : 4;
    const size_t off = ((size_t)y * wo + xg) * 3;
    const unsigned char* t = (const unsigned char*)s_lut;
    // uniform branches: the parameters are the same for every thread.  An 8-bit sensor's multiplier never fits 24 bits (file comment)
    if (sizeof(T) == 1 || wide) {
        if (NCH == 3 && ccm) dv_planes<NCH, KB, true, NCH == 3>(a, acc, q, t, off, nvalid);
        else dv_planes<NCH, KB, true, false>(a, acc, q, t, off, nvalid);
    } else {
        if (NCH == 3 && ccm) dv_planes<NCH, KB, false, NCH == 3>(a, acc, q, t, off, nvalid);
        else dv_planes<NCH, KB, false, false>(a, acc, q, t, off, nvalid);
    }
}

template <int PATTERN, int MODE, typename T>
void dv_launch(const DofpArgs& a, const void* src, int h, int w, size_t pitch, int ho, int wo, const int* params, const unsigned char* lut,
               hipStream_t st) {
    const dim3 grid(shm_cdiv(shm_cdiv(wo, 4), DF_BX), shm_cdiv(ho, DF_BY)), block(DF_BX, DF_BY);
    const int aligned = (uintptr_t)src % (4 * sizeof(T)) == 0 && pitch % 4 == 0;
    hipLaunchKernelGGL((dofp_develop_kernel<PATTERN, MODE, T>), grid, block, 0, st, a, (const T*)src, h, w, pitch, ho, wo, aligned, params,
                       (const uint4*)lut);
}

template <int PATTERN>
void dv_launch_pattern(const DofpArgs& a, const void* src, int bits, int h, int w, size_t pitch, int mode, int ho, int wo, const int* params,
                       const unsigned char* lut, hipStream_t st) {
    if (mode == SHM_DOFP_BILINEAR) {
        if (bits == 8) dv_launch<PATTERN, SHM_DOFP_BILINEAR, unsigned char>(a, src, h, w, pitch, ho, wo, params, lut, st);
        else dv_launch<PATTERN, SHM_DOFP_BILINEAR, unsigned short>(a, src, h, w, pitch, ho, wo, params, lut, st);
    } else {
        if (bits == 8) dv_launch<PATTERN, SHM_DOFP_BIN, unsigned char>(a, src, h, w, pitch, ho, wo, params, lut, st);
        else dv_launch<PATTERN, SHM_DOFP_BIN, unsigned short>(a, src, h, w, pitch, ho, wo, params, lut, st);
    }
}

// ---- grey-world sums ------------------------------------------------------------------------------------------------------------------
constexpr int WB_NT = 256;
constexpr int WB_PART = 16;                      // ws[WB_PART + 6 b + k]: block b's sum k (S_r, S_g, S_b, n_r, n_g, n_b)

// One thread per 4 x 4 period, grid-stride.  A thread walks at most 8192^2 / (SHM_DOFP_WB_BLOCKS * WB_NT) = 512 periods of at most 8 samples
// of a colour: its own sums fit 32 bits.
template <int PATTERN, typename T>
__global__ void __launch_bounds__(WB_NT) dofp_wb_sums_kernel(const T* __restrict__ src, int ph, int pw, size_t pitch, const int* __restrict__ params,
                                                             unsigned sat, unsigned long long* __restrict__ ws) {
    unsigned black[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) black[c] = (unsigned)params[SHM_DOFP_P_BLACK + c];
    unsigned S[3] = {0u, 0u, 0u}, cnt = 0u;
    const size_t np = (size_t)ph * pw;
    for (size_t i = (size_t)blockIdx.x * WB_NT + threadIdx.x; i < np; i += (size_t)gridDim.x * WB_NT) {
        const int py = (int)(i / pw), px = (int)(i - (size_t)py * pw);
        const T* p = src + (size_t)(4 * py) * pitch + 4 * px;
        unsigned s[3] = {0u, 0u, 0u};
        bool ok = true;
#pragma unroll
        for (int dy = 0; dy < 4; ++dy)
#pragma unroll
            for (int dx = 0; dx < 4; ++dx) {
                const unsigned v = (unsigned)p[(size_t)dy * pitch + dx];
                const int c = df_channel<PATTERN>((dy >> 1) * 2 + (dx >> 1));
                ok = ok && v < sat;
                s[c] += v > black[c] ? v - black[c] : 0u;
            }
        if (ok) {
#pragma unroll
            for (int c = 0; c < 3; ++c) S[c] += s[c];
            ++cnt;
        }
    }
    // a block's sums stay below 256 * 2^32 = 2^40: exact in double
    double r[6];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        r[c] = shm_block_sum<WB_NT>((double)S[c]);
        r[3 + c] = shm_block_sum<WB_NT>((double)(cnt * (c == 1 ? 8u : 4u)));
    }
    if (threadIdx.x < 6) {
        double v = r[0];
#pragma unroll
        for (int k = 1; k < 6; ++k) v = threadIdx.x == k ? r[k] : v;
        ws[WB_PART + 6 * (size_t)blockIdx.x + threadIdx.x] = (unsigned long long)v;
    }
}

// the frame's sums stay below 2^30 samples * 2^16 = 2^46: exact in double
__global__ void __launch_bounds__(WB_NT) dofp_wb_finish_kernel(unsigned long long* __restrict__ ws, int nblocks, const int* params_in, int* params_out) {
    unsigned long long sum[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        double v = 0.0;
        for (int b = threadIdx.x; b < nblocks; b += WB_NT) v += (double)ws[WB_PART + 6 * (size_t)b + k];
        sum[k] = (unsigned long long)shm_block_sum<WB_NT>(v);
    }
    unsigned long long mean[3], top = 0ull;
    bool any0 = false;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        mean[c] = sum[3 + c] ? (sum[c] << 8) / sum[3 + c] : 0ull;
        any0 = any0 || mean[c] == 0ull;
        top = mean[c] > top ? mean[c] : top;
    }
    unsigned gain[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const unsigned long long g = any0 ? 1024ull : (top << 10) / mean[c];
        gain[c] = g > 16383ull ? 16383u : (unsigned)g;
    }
    const int i = threadIdx.x;
    if (i < SHM_DOFP_PARAMS) {
        int v = params_in[i];
#pragma unroll
        for (int c = 0; c < 3; ++c) v = i == SHM_DOFP_P_GAIN + c ? (int)gain[c] : v;
        params_out[i] = v;
    }
    if (i < 9) {
        unsigned long long v = 0ull;
#pragma unroll
        for (int k = 0; k < 6; ++k) v = i == k ? sum[k] : v;
#pragma unroll
        for (int c = 0; c < 3; ++c) v = i == 6 + c ? (unsigned long long)gain[c] : v;
        ws[i] = v;
    }
}

template <int PATTERN>
void wb_launch(const void* src, int bits, int ph, int pw, size_t pitch, const int* params, unsigned sat, unsigned long long* ws, int blocks, hipStream_t st) {
    if (bits == 8)
        hipLaunchKernelGGL((dofp_wb_sums_kernel<PATTERN, unsigned char>), dim3(blocks), dim3(WB_NT), 0, st, (const unsigned char*)src, ph, pw, pitch, params,
                           sat, ws);
    else
        hipLaunchKernelGGL((dofp_wb_sums_kernel<PATTERN, unsigned short>), dim3(blocks), dim3(WB_NT), 0, st, (const unsigned short*)src, ph, pw, pitch, params,
                           sat, ws);
}

}  // namespace

extern "C" int shm_dofp_develop(const void* src, int bits, int h, int w, size_t src_pitch, int pattern, const int* quad, int mode,
                                unsigned char* const* dst_ptrs, unsigned char* total, const int* params, const unsigned char* lut,
                                const int* params_host, void* stream) {
    if (int rc = df_check_args("shm_dofp_develop", src, bits, h, w, src_pitch, pattern, quad, mode, dst_ptrs)) return rc;
    SHM_REQUIRE(params && lut && params_host, SHM_E_SHAPE, "shm_dofp_develop: null pointer (params, lut or params_host)");
    SHM_REQUIRE((uintptr_t)lut % 16 == 0, SHM_E_SHAPE, "shm_dofp_develop: lut is not 16-byte aligned");
    const int* m = params_host;
    for (int c = 0; c < 3; ++c) {
        SHM_REQUIRE(m[SHM_DOFP_P_BLACK + c] >= 0 && m[SHM_DOFP_P_BLACK + c] <= 65535 - 16, SHM_E_SHAPE, "shm_dofp_develop: black[%d] = %d outside [0, 65519]", c,
                    m[SHM_DOFP_P_BLACK + c]);
        SHM_REQUIRE((unsigned)m[SHM_DOFP_P_MUL + c] >= 65536u, SHM_E_SHAPE, "shm_dofp_develop: mul[%d] = %u below 65536", c, (unsigned)m[SHM_DOFP_P_MUL + c]);
    }
    for (int i = 0; i < 9; ++i)
        SHM_REQUIRE(m[SHM_DOFP_P_CCM + i] >= -8191 && m[SHM_DOFP_P_CCM + i] <= 8191, SHM_E_SHAPE, "shm_dofp_develop: ccm[%d] = %d outside [-8191, 8191]", i,
                    m[SHM_DOFP_P_CCM + i]);
    SHM_REQUIRE((m[SHM_DOFP_P_FLAGS] & ~1) == 0, SHM_E_SHAPE, "shm_dofp_develop: unknown flag bits %d", m[SHM_DOFP_P_FLAGS]);
    if (pattern == SHM_DOFP_MONO) {
        SHM_REQUIRE(!(m[SHM_DOFP_P_FLAGS] & 1), SHM_E_SHAPE, "shm_dofp_develop: SHM_DOFP_MONO with a colour matrix");
        for (int c = 1; c < 3; ++c)
            SHM_REQUIRE(m[SHM_DOFP_P_BLACK + c] == m[SHM_DOFP_P_BLACK] && m[SHM_DOFP_P_MUL + c] == m[SHM_DOFP_P_MUL], SHM_E_SHAPE,
                        "shm_dofp_develop: SHM_DOFP_MONO with parameters that differ between the channels (channel %d)", c);
    }
    const int P = pattern == SHM_DOFP_MONO ? 2 : 4;
    DofpArgs a;
    for (int i = 0; i < 4; ++i) a.plane[i] = dst_ptrs[quad[i]];
    a.total = total;
    const int ho = mode == SHM_DOFP_BIN ? h / P : h, wo = mode == SHM_DOFP_BIN ? w / P : w;
    hipStream_t st = (hipStream_t)stream;
    switch (pattern) {
        case SHM_DOFP_MONO: dv_launch_pattern<SHM_DOFP_MONO>(a, src, bits, h, w, src_pitch, mode, ho, wo, params, lut, st); break;
        case SHM_DOFP_RGGB: dv_launch_pattern<SHM_DOFP_RGGB>(a, src, bits, h, w, src_pitch, mode, ho, wo, params, lut, st); break;
        case SHM_DOFP_BGGR: dv_launch_pattern<SHM_DOFP_BGGR>(a, src, bits, h, w, src_pitch, mode, ho, wo, params, lut, st); break;
        case SHM_DOFP_GRBG: dv_launch_pattern<SHM_DOFP_GRBG>(a, src, bits, h, w, src_pitch, mode, ho, wo, params, lut, st); break;
        default: dv_launch_pattern<SHM_DOFP_GBRG>(a, src, bits, h, w, src_pitch, mode, ho, wo, params, lut, st); break;
    }
    SHM_LAUNCH_CHECK("shm_dofp_develop");
    return SHM_OK;
}

extern "C" int shm_dofp_wb_gray(const void* src, int bits, int h, int w, size_t src_pitch, int pattern, const int* params_in, int sat, int* params_out,
                                unsigned long long* ws, void* stream) {
    SHM_REQUIRE(src && params_in && params_out && ws, SHM_E_SHAPE, "shm_dofp_wb_gray: null pointer (src, params_in, params_out or ws)");
    SHM_REQUIRE(bits >= 8 && bits <= 16, SHM_E_SHAPE, "shm_dofp_wb_gray: bits %d outside [8, 16]", bits);
    SHM_REQUIRE(pattern >= SHM_DOFP_RGGB && pattern <= SHM_DOFP_GBRG, SHM_E_SHAPE, "shm_dofp_wb_gray: pattern %d is not a Bayer pattern", pattern);
    SHM_REQUIRE(h >= 4 && h <= DF_DIM_MAX && w >= 4 && w <= DF_DIM_MAX, SHM_E_SHAPE, "shm_dofp_wb_gray: sizes h %d, w %d outside [4, %d]", h, w, DF_DIM_MAX);
    SHM_REQUIRE(src_pitch >= (size_t)w, SHM_E_SHAPE, "shm_dofp_wb_gray: src_pitch %zu below w %d", src_pitch, w);
    SHM_REQUIRE(sat >= 1 && sat <= 65536, SHM_E_SHAPE, "shm_dofp_wb_gray: sat %d outside [1, 65536]", sat);
    const int ph = h / 4, pw = w / 4;
    const int blocks = shm_grid_cap((size_t)ph * pw, WB_NT, SHM_DOFP_WB_BLOCKS);
    hipStream_t st = (hipStream_t)stream;
    switch (pattern) {
        case SHM_DOFP_RGGB: wb_launch<SHM_DOFP_RGGB>(src, bits, ph, pw, src_pitch, params_in, (unsigned)sat, ws, blocks, st); break;
        case SHM_DOFP_BGGR: wb_launch<SHM_DOFP_BGGR>(src, bits, ph, pw, src_pitch, params_in, (unsigned)sat, ws, blocks, st); break;
        case SHM_DOFP_GRBG: wb_launch<SHM_DOFP_GRBG>(src, bits, ph, pw, src_pitch, params_in, (unsigned)sat, ws, blocks, st); break;
        default: wb_launch<SHM_DOFP_GBRG>(src, bits, ph, pw, src_pitch, params_in, (unsigned)sat, ws, blocks, st); break;
    }
    SHM_LAUNCH_CHECK("shm_dofp_wb_gray");
    hipLaunchKernelGGL(dofp_wb_finish_kernel, dim3(1), dim3(WB_NT), 0, st, ws, blocks, params_in, params_out);
    SHM_LAUNCH_CHECK("shm_dofp_wb_gray");
    return SHM_OK;
}
