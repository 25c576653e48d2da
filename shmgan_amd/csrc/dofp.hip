// Division-of-focal-plane (DoFP) polarisation sensors: one raw mosaic -> the four polariser views the rest of the pipeline reads.
//
//   shm_dofp_views   every 2 x 2 quad of the mosaic sits behind four micro-polarisers; on the colour parts every quad sits behind one
//                    Bayer filter, so the period P is 2 (mono) or 4.  The sample at quad position (ay, ax) under colour block
//                    (by, bx) lies on the lattice with offsets dy = 2 by + ay, dx = 2 bx + ax and period P: P * P lattices, each of
//                    which belongs to one view and one colour.  SHM_DOFP_BILINEAR interpolates every lattice to the mosaic's size
//                    (integer weights, total P^2), SHM_DOFP_BIN takes each super-pixel's own sample; include/shmgan_hip.h states
//                    the arithmetic, which is integer and exact.
//
// One thread makes four consecutive output pixels of one row, in all four views (and the total plane).  The interpolation is
// separable: per lattice the thread combines the two tap rows once per tap column (three columns at P = 4, four at P = 2 serve all four
// pixels) and then lerps along the row.  All lattices together need, per tap row, the twelve consecutive samples xg - 4 .. xg + 7: away
// from the left and right edges, and when the source's base and pitch are multiples of four samples, a thread reads them as three
// 4-sample accesses per row (24 per thread for colour, 12 for mono, each coalesced across the wave); elsewhere it reads one sample at
// a time at its clamped column (96 / 32 per thread).  Every index of the per-thread arrays is a compile-time constant after
// unrolling, which is why the pattern and the mode are template parameters: nothing is indexed by a run-time value, so nothing lives
// in scratch.  The mosaic is not staged in LDS: the windows of neighbouring threads overlap by two thirds, and that reuse, like the
// reuse between rows (each sample feeds up to P^2 outputs per view), is left to L1 / L2.  A plane's four pixels are 12 bytes: three
// dword stores when they start 4-byte aligned and all four lie inside the row, byte stores otherwise.
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
__device__ __forceinline__ unsigned df_finish(unsigned n, int sh) {
    const unsigned v = (n + ((1u << sh) >> 1)) >> sh;
    return v > 255u ? 255u : v;
}

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

template <int PATTERN, int MODE, typename T>
__global__ void __launch_bounds__(DF_BX* DF_BY) dofp_views_kernel(const DofpArgs a, const T* __restrict__ src, int h, int w, size_t pitch, int ho,
                                                                   int wo, int s, int aligned) {
    constexpr int P = PATTERN == SHM_DOFP_MONO ? 2 : 4;
    constexpr int NCH = PATTERN == SHM_DOFP_MONO ? 1 : 3;                 // mono: one numerator serves R, G and B
    const int y = blockIdx.y * DF_BY + threadIdx.y;
    const int xg = 4 * (blockIdx.x * DF_BX + threadIdx.x);
    if (y >= ho || xg >= wo) return;
    unsigned acc[4][NCH][4];                                             // [quad position][channel][pixel]: numerators
#pragma unroll
    for (int p = 0; p < 4; ++p)
#pragma unroll
        for (int c = 0; c < NCH; ++c)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[p][c][j] = 0u;
    // `aligned`: the source's base and pitch are multiples of four samples, so a window that starts at a multiple of 4 columns is aligned
    const bool fast = aligned && (MODE == SHM_DOFP_BILINEAR ? (xg >= 4 && xg + 7 < w) : (xg + 4 <= wo));
    if (fast)
        df_numerators<PATTERN, MODE, T, true, NCH>(acc, src, h, w, pitch, y, xg, wo);
    else
        df_numerators<PATTERN, MODE, T, false, NCH>(acc, src, h, w, pitch, y, xg, wo);
    // k = 2 log2 P in bilinear mode, 0 in bin mode; one more for G, the sum of two lattices
    constexpr int K = MODE == SHM_DOFP_BILINEAR ? (P == 4 ? 4 : 2) : 0;
    const int nvalid = wo - xg < 4 ? wo - xg : 4;
    const size_t off = ((size_t)y * wo + xg) * 3;
    unsigned tot[NCH][4];
#pragma unroll
    for (int c = 0; c < NCH; ++c)
#pragma unroll
        for (int j = 0; j < 4; ++j) tot[c][j] = 0u;
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        unsigned o[3][4];
#pragma unroll
        for (int c = 0; c < 3; ++c)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int cc = NCH == 1 ? 0 : c;
                o[c][j] = df_finish(acc[p][cc][j], K + (NCH == 3 && c == 1 ? 1 : 0) + s);
            }
#pragma unroll
        for (int c = 0; c < NCH; ++c)
#pragma unroll
            for (int j = 0; j < 4; ++j) tot[c][j] += acc[p][c][j];
        df_store4(a.plane[p] + off, o[0], o[1], o[2], nvalid);
    }
    if (a.total) {
        unsigned o[3][4];
#pragma unroll
        for (int c = 0; c < 3; ++c)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int cc = NCH == 1 ? 0 : c;
                o[c][j] = df_finish(tot[cc][j], K + (NCH == 3 && c == 1 ? 1 : 0) + s + 2);
            }
        df_store4(a.total + off, o[0], o[1], o[2], nvalid);
    }
}

template <int PATTERN, int MODE, typename T>
void df_launch(const DofpArgs& a, const void* src, int h, int w, size_t pitch, int ho, int wo, int s, hipStream_t st) {
    const dim3 grid(shm_cdiv(shm_cdiv(wo, 4), DF_BX), shm_cdiv(ho, DF_BY)), block(DF_BX, DF_BY);
    const int aligned = (uintptr_t)src % (4 * sizeof(T)) == 0 && pitch % 4 == 0;          // windows of four samples can be read in one access
    hipLaunchKernelGGL((dofp_views_kernel<PATTERN, MODE, T>), grid, block, 0, st, a, (const T*)src, h, w, pitch, ho, wo, s, aligned);
}

template <int PATTERN>
void df_launch_pattern(const DofpArgs& a, const void* src, int bits, int h, int w, size_t pitch, int mode, int ho, int wo, hipStream_t st) {
    const int s = bits - 8;
    if (mode == SHM_DOFP_BILINEAR) {
        if (bits == 8) df_launch<PATTERN, SHM_DOFP_BILINEAR, unsigned char>(a, src, h, w, pitch, ho, wo, s, st);
        else df_launch<PATTERN, SHM_DOFP_BILINEAR, unsigned short>(a, src, h, w, pitch, ho, wo, s, st);
    } else {
        if (bits == 8) df_launch<PATTERN, SHM_DOFP_BIN, unsigned char>(a, src, h, w, pitch, ho, wo, s, st);
        else df_launch<PATTERN, SHM_DOFP_BIN, unsigned short>(a, src, h, w, pitch, ho, wo, s, st);
    }
}

}  // namespace

extern "C" int shm_dofp_views(const void* src, int bits, int h, int w, size_t src_pitch, int pattern, const int* quad, int mode,
                              unsigned char* const* dst_ptrs, unsigned char* total, void* stream) {
    SHM_REQUIRE(src && quad && dst_ptrs, SHM_E_SHAPE, "shm_dofp_views: null pointer (src, quad or dst_ptrs)");
    for (int v = 0; v < 4; ++v) SHM_REQUIRE(dst_ptrs[v], SHM_E_SHAPE, "shm_dofp_views: null pointer (destination view %d)", v);
    SHM_REQUIRE(bits >= 8 && bits <= 16, SHM_E_SHAPE, "shm_dofp_views: bits %d outside [8, 16]", bits);
    SHM_REQUIRE(pattern >= SHM_DOFP_MONO && pattern <= SHM_DOFP_GBRG, SHM_E_SHAPE, "shm_dofp_views: pattern %d unknown", pattern);
    SHM_REQUIRE(mode == SHM_DOFP_BILINEAR || mode == SHM_DOFP_BIN, SHM_E_SHAPE, "shm_dofp_views: mode %d unknown", mode);
    const int P = pattern == SHM_DOFP_MONO ? 2 : 4;
    SHM_REQUIRE(h >= P && h <= DF_DIM_MAX && w >= P && w <= DF_DIM_MAX, SHM_E_SHAPE, "shm_dofp_views: sizes h %d, w %d outside [%d, %d]", h, w, P,
                DF_DIM_MAX);
    SHM_REQUIRE(src_pitch >= (size_t)w, SHM_E_SHAPE, "shm_dofp_views: src_pitch %zu below w %d", src_pitch, w);
    int seen = 0;
    for (int i = 0; i < 4; ++i) {
        SHM_REQUIRE(quad[i] >= 0 && quad[i] <= 3, SHM_E_SHAPE, "shm_dofp_views: quad[%d] = %d is not a view index 0..3", i, quad[i]);
        seen |= 1 << quad[i];
    }
    SHM_REQUIRE(seen == 15, SHM_E_SHAPE, "shm_dofp_views: quad (%d, %d, %d, %d) is not a permutation of 0..3", quad[0], quad[1], quad[2], quad[3]);
    DofpArgs a;
    for (int i = 0; i < 4; ++i) a.plane[i] = dst_ptrs[quad[i]];
    a.total = total;
    const int ho = mode == SHM_DOFP_BIN ? h / P : h, wo = mode == SHM_DOFP_BIN ? w / P : w;
    hipStream_t st = (hipStream_t)stream;
    switch (pattern) {
        case SHM_DOFP_MONO: df_launch_pattern<SHM_DOFP_MONO>(a, src, bits, h, w, src_pitch, mode, ho, wo, st); break;
        case SHM_DOFP_RGGB: df_launch_pattern<SHM_DOFP_RGGB>(a, src, bits, h, w, src_pitch, mode, ho, wo, st); break;
        case SHM_DOFP_BGGR: df_launch_pattern<SHM_DOFP_BGGR>(a, src, bits, h, w, src_pitch, mode, ho, wo, st); break;
        case SHM_DOFP_GRBG: df_launch_pattern<SHM_DOFP_GRBG>(a, src, bits, h, w, src_pitch, mode, ho, wo, st); break;
        default: df_launch_pattern<SHM_DOFP_GBRG>(a, src, bits, h, w, src_pitch, mode, ho, wo, st); break;
    }
    SHM_LAUNCH_CHECK("shm_dofp_views");
    return SHM_OK;
}
