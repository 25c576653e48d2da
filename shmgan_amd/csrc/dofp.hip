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
// dword stores when they start 4-byte aligned and all four lie inside the row, byte stores otherwise.  The tap walk, the loads and the
// store are in dofp_dev.h, which dofp_develop.hip shares; this file keeps the finish that cuts the numerators to 8 bits.
#include "dofp_dev.h"

namespace {

__device__ __forceinline__ unsigned df_finish(unsigned n, int sh) {
    const unsigned v = (n + ((1u << sh) >> 1)) >> sh;
    return v > 255u ? 255u : v;
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
    if (int rc = df_check_args("shm_dofp_views", src, bits, h, w, src_pitch, pattern, quad, mode, dst_ptrs)) return rc;
    const int P = pattern == SHM_DOFP_MONO ? 2 : 4;
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
