// The tap walk of the polariser-mosaic kernels (dofp.hip: shm_dofp_views; dofp_develop.hip: shm_dofp_develop): launch geometry, the
// Bayer tile's channel table, the sample loads, the plane store and df_numerators, which leaves a thread's four pixels' channel numerators
// of all four views in registers.  What a kernel makes of the numerators (the 8-bit cut, or the development) is its own.  Also the
// eight-sample group accesses of the passes over the mosaic itself (dofp_calibrate.hip, dofp_merge.hip).  Everything
// here has internal linkage: each source that includes it gets its own copy.
#pragma once
#include "common.h"

namespace {

constexpr int DF_BX = 64;                       // threads along a row: 256 output pixels
constexpr int DF_BY = 4;                        // rows per block
constexpr int DF_DIM_MAX = 32768;               // h, w

struct DofpArgs {
    unsigned char* plane[4];                    // by QUAD POSITION (0,0), (0,1), (1,0), (1,1): dst_ptrs[quad[pos]]
    unsigned char* total;                       // or null
};

// colour channel (0 R, 1 G, 2 B) of colour block blk = 2 by + bx of the Bayer tile
template <int PATTERN>
__device__ constexpr int df_channel(int blk) {
    return PATTERN == SHM_DOFP_RGGB ? (blk == 0 ? 0 : blk == 3 ? 2 : 1)
         : PATTERN == SHM_DOFP_BGGR ? (blk == 0 ? 2 : blk == 3 ? 0 : 1)
         : PATTERN == SHM_DOFP_GRBG ? (blk == 1 ? 0 : blk == 2 ? 2 : 1)
                                    : (blk == 1 ? 2 : blk == 2 ? 0 : 1);          // GBRG
}

__device__ __forceinline__ int df_clamp(int i, int n) { return i < 0 ? 0 : i > n - 1 ? n - 1 : i; }

// four pixels (r, g, b)[4] of one plane at p = the first pixel's address; nvalid of them lie inside the row
__device__ __forceinline__ void df_store4(unsigned char* p, const unsigned (&r)[4], const unsigned (&g)[4], const unsigned (&b)[4], int nvalid) {
    if (nvalid == 4 && ((uintptr_t)p & 3) == 0) {
        unsigned* q = (unsigned*)p;
        q[0] = r[0] | g[0] << 8 | b[0] << 16 | r[1] << 24;
        q[1] = g[1] | b[1] << 8 | r[2] << 16 | g[2] << 24;
        q[2] = b[2] | r[3] << 8 | g[3] << 16 | b[3] << 24;
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (j < nvalid) {
                p[3 * j] = (unsigned char)r[j];
                p[3 * j + 1] = (unsigned char)g[j];
                p[3 * j + 2] = (unsigned char)b[j];
            }
    }
}

// the two tap rows of a column combined: weights <= P and samples < 2^16, so the 24-bit multiplier (full rate; the 32-bit one runs at a
// quarter of it, and this kernel is bound by its vector arithmetic) gives the exact product
__device__ __forceinline__ unsigned df_rows(unsigned w0, unsigned a, unsigned w1, unsigned b) { return __umul24(w0, a) + __umul24(w1, b); }

// four consecutive samples in one access: p is aligned to four samples
__device__ __forceinline__ void df_load4(const unsigned short* p, unsigned* out) {
    const uint2 u = *(const uint2*)p;
    out[0] = u.x & 0xffffu;
    out[1] = u.x >> 16;
    out[2] = u.y & 0xffffu;
    out[3] = u.y >> 16;
}
__device__ __forceinline__ void df_load4(const unsigned char* p, unsigned* out) {
    const unsigned u = *(const unsigned*)p;
    out[0] = u & 0xffu;
    out[1] = (u >> 8) & 0xffu;
    out[2] = (u >> 16) & 0xffu;
    out[3] = u >> 24;
}

// The bandwidth passes over a mosaic (dofp_calibrate.hip, dofp_merge.hip) give a thread DF_GROUP consecutive samples of a row.  `vec`: p is
// aligned to the group and all of it lies inside the row: one 16-byte (uint16) or 8-byte (uint8) access; otherwise one access per element
// for the first nvalid, the same values.
constexpr int DF_GROUP = 8;

__device__ __forceinline__ void df_load8(const unsigned short* p, bool vec, int nvalid, unsigned (&o)[DF_GROUP]) {
    if (vec) {
        const uint4 u = *(const uint4*)p;
        o[0] = u.x & 0xffffu, o[1] = u.x >> 16, o[2] = u.y & 0xffffu, o[3] = u.y >> 16;
        o[4] = u.z & 0xffffu, o[5] = u.z >> 16, o[6] = u.w & 0xffffu, o[7] = u.w >> 16;
    } else {
#pragma unroll
        for (int j = 0; j < DF_GROUP; ++j) o[j] = j < nvalid ? (unsigned)p[j] : 0u;
    }
}
__device__ __forceinline__ void df_load8(const unsigned char* p, bool vec, int nvalid, unsigned (&o)[DF_GROUP]) {
    if (vec) {
        const uint2 u = *(const uint2*)p;
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = (u.x >> (8 * j)) & 0xffu, o[4 + j] = (u.y >> (8 * j)) & 0xffu;
    } else {
#pragma unroll
        for (int j = 0; j < DF_GROUP; ++j) o[j] = j < nvalid ? (unsigned)p[j] : 0u;
    }
}
__device__ __forceinline__ void df_store8(unsigned short* p, bool vec, int nvalid, const unsigned (&o)[DF_GROUP]) {
    if (vec) {
        *(uint4*)p = make_uint4(o[0] | o[1] << 16, o[2] | o[3] << 16, o[4] | o[5] << 16, o[6] | o[7] << 16);
    } else {
#pragma unroll
        for (int j = 0; j < DF_GROUP; ++j)
            if (j < nvalid) p[j] = (unsigned short)o[j];
    }
}
__device__ __forceinline__ void df_store8(unsigned char* p, bool vec, int nvalid, const unsigned (&o)[DF_GROUP]) {
    if (vec) {
        *(uint2*)p = make_uint2(o[0] | o[1] << 8 | o[2] << 16 | o[3] << 24, o[4] | o[5] << 8 | o[6] << 16 | o[7] << 24);
    } else {
#pragma unroll
        for (int j = 0; j < DF_GROUP; ++j)
            if (j < nvalid) p[j] = (unsigned char)o[j];
    }
}

// The numerators acc[quad position][channel][pixel] of the thread's four pixels (y, xg .. xg + 3).  FAST: every sample the thread needs lies in
// one window of consecutive columns inside the row -- xg - 4 .. xg + 7 in bilinear mode (no column clamp is active there), P xg .. P xg + 4 P - 1
// in bin mode -- whose start is aligned to four samples: the window is read with df_load4, three (bilinear) or P (bin) accesses per row, which
// neighbouring lanes coalesce.  Otherwise one access per sample at its clamped column.  Same integers either way.
template <int PATTERN, int MODE, typename T, bool FAST, int NCH>
__device__ __forceinline__ void df_numerators(unsigned (&acc)[4][NCH][4], const T* __restrict__ src, int h, int w, size_t pitch, int y, int xg, int wo) {
    constexpr int P = PATTERN == SHM_DOFP_MONO ? 2 : 4;
    constexpr int NC = P == 4 ? 3 : 4;                                   // lattice columns that serve the thread's four pixels
    constexpr int NWIN = MODE == SHM_DOFP_BILINEAR ? 12 : 4 * P;
#pragma unroll
    for (int dy = 0; dy < P; ++dy) {
        size_t row0, row1;
        unsigned wy0, wy1;
        if (MODE == SHM_DOFP_BILINEAR) {
            const int ny = (h - 1 - dy) / P + 1;
            const int q = y - dy, i0 = (q + P) / P - 1, f = q - P * i0;          // floor division; q >= -(P - 1)
            row0 = (size_t)(dy + P * df_clamp(i0, ny)) * pitch;
            row1 = (size_t)(dy + P * df_clamp(i0 + 1, ny)) * pitch;
            wy0 = (unsigned)(P - f);
            wy1 = (unsigned)f;
        } else {
            row0 = row1 = (size_t)(P * y + dy) * pitch;
            wy0 = 1u;
            wy1 = 0u;
        }
        unsigned win[NWIN];                                                      // FAST: the window, its two rows combined
        if (FAST) {
#pragma unroll
            for (int k = 0; k < NWIN / 4; ++k) {
                if (MODE == SHM_DOFP_BILINEAR) {
                    unsigned r0[4], r1[4];
                    df_load4(src + row0 + (xg - 4 + 4 * k), r0);
                    df_load4(src + row1 + (xg - 4 + 4 * k), r1);
#pragma unroll
                    for (int i = 0; i < 4; ++i) win[4 * k + i] = df_rows(wy0, r0[i], wy1, r1[i]);
                } else {
                    df_load4(src + row0 + ((size_t)P * xg + 4 * k), &win[4 * k]);
                }
            }
        }
#pragma unroll
        for (int dx = 0; dx < P; ++dx) {
            const int pos = (dy & 1) * 2 + (dx & 1);
            const int ch = PATTERN == SHM_DOFP_MONO ? 0 : df_channel<PATTERN>((dy >> 1) * 2 + (dx >> 1));
            if (MODE == SHM_DOFP_BILINEAR) {
                const int nx = (w - 1 - dx) / P + 1;
                const int mb = xg / P - (dx + P - 1) / P;                        // floor((xg - dx) / P): xg is a multiple of 4
                unsigned v[NC];                                                  // rows combined, per lattice column mb + c (clamped)
#pragma unroll
                for (int c = 0; c < NC; ++c) {
                    if (FAST) {                                                  // column dx + P (mb + c), counted from xg - 4: a constant
                        v[c] = win[dx + P * c - P * ((dx + P - 1) / P) + 4];
                    } else {
                        const int col = dx + P * df_clamp(mb + c, nx);
                        v[c] = df_rows(wy0, (unsigned)src[row0 + col], wy1, (unsigned)src[row1 + col]);
                    }
                }
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    // floor((xg + j - dx) / P) - mb and the remainder: constants, since xg is a multiple of P
                    const int t = j - dx + P * ((dx + P - 1) / P);               // >= 0
                    const int c = t / P, f = t % P;
                    acc[pos][ch][j] += (unsigned)(P - f) * v[c] + (unsigned)f * v[c + 1 < NC ? c + 1 : c];
                }
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    if (FAST) acc[pos][ch][j] += win[P * j + dx];
                    else if (xg + j < wo) acc[pos][ch][j] += (unsigned)src[row0 + (size_t)(P * (xg + j) + dx)];
                }
            }
        }
    }
}

// The refusals the mosaic entry points share (include/shmgan_hip.h lists them); `who` names the entry point in the message.
inline int df_check_args(const char* who, const void* src, int bits, int h, int w, size_t src_pitch, int pattern, const int* quad, int mode,
                         unsigned char* const* dst_ptrs) {
    SHM_REQUIRE(src && quad && dst_ptrs, SHM_E_SHAPE, "%s: null pointer (src, quad or dst_ptrs)", who);
    for (int v = 0; v < 4; ++v) SHM_REQUIRE(dst_ptrs[v], SHM_E_SHAPE, "%s: null pointer (destination view %d)", who, v);
    SHM_REQUIRE(bits >= 8 && bits <= 16, SHM_E_SHAPE, "%s: bits %d outside [8, 16]", who, bits);
    SHM_REQUIRE(pattern >= SHM_DOFP_MONO && pattern <= SHM_DOFP_GBRG, SHM_E_SHAPE, "%s: pattern %d unknown", who, pattern);
    SHM_REQUIRE(mode == SHM_DOFP_BILINEAR || mode == SHM_DOFP_BIN, SHM_E_SHAPE, "%s: mode %d unknown", who, mode);
    const int P = pattern == SHM_DOFP_MONO ? 2 : 4;
    SHM_REQUIRE(h >= P && h <= DF_DIM_MAX && w >= P && w <= DF_DIM_MAX, SHM_E_SHAPE, "%s: sizes h %d, w %d outside [%d, %d]", who, h, w, P,
                DF_DIM_MAX);
    SHM_REQUIRE(src_pitch >= (size_t)w, SHM_E_SHAPE, "%s: src_pitch %zu below w %d", who, src_pitch, w);
    int seen = 0;
    for (int i = 0; i < 4; ++i) {
        SHM_REQUIRE(quad[i] >= 0 && quad[i] <= 3, SHM_E_SHAPE, "%s: quad[%d] = %d is not a view index 0..3", who, i, quad[i]);
        seen |= 1 << quad[i];
    }
    SHM_REQUIRE(seen == 15, SHM_E_SHAPE, "%s: quad (%d, %d, %d, %d) is not a permutation of 0..3", who, quad[0], quad[1], quad[2], quad[3]);
    return SHM_OK;
}

}  // namespace
