// Calibrating a polariser mosaic before it is demosaiced: dark frame, flat field, defect map.
//
//   shm_dofp_calibrate   dst = the mosaic with every sample's fixed-pattern dark offset removed and its gain equalised around the
//                        pedestal, and every defective photosite replaced by the rounded mean of the corrected good neighbours on its
//                        OWN lattice (period P: the same polariser and the same colour).  It runs on the raw mosaic because each view
//                        is built from one photosite per quad: a bad sample that reaches shm_dofp_views is spread over a (2P-1)^2
//                        footprint of one view only, which everything downstream reads as polarisation.  include/shmgan_hip.h states
//                        the arithmetic, which is integer and exact.
//
// A bandwidth pass.  One thread makes CAL_N = 8 consecutive samples of one row.  A full group whose first address is aligned is read and
// written in one access per array: 16 bytes of a uint16 mosaic, dark or gain row, 8 bytes of a uint8 mosaic or of the defect row.  Source,
// destination and tables are judged separately (base and pitch multiples of 8 elements; the tables are tight, so w % 8 == 0), and the
// group at the end of a ragged row, or any array that fails its test, goes one element at a time with the same integers.  A defective site
// is rare: its four neighbours are read straight from global memory (all four before any is judged, so the loads do not wait for one
// another), corrected again and averaged in that branch; nothing is staged.
#include "dofp_dev.h"

namespace {

constexpr int CAL_N = DF_GROUP;                 // samples per thread (dofp_dev.h: df_load8, df_store8)
constexpr int CAL_BX = 64;                      // threads along a row: 512 samples
constexpr int CAL_BY = 4;                       // rows per block

struct CalArgs {
    const unsigned short* dark;                 // tight [h,w], or null: pedestal everywhere
    const unsigned short* gain;                 // tight [h,w] Q12, or null: 4096 everywhere
    const unsigned char* defect;                // tight [h,w], or null: none
    int pedestal, white, maxv;
    int vsrc, vdst, vtab;                       // groups of CAL_N start aligned in the source / the destination / the tables
};

// corr of the header: |v - dark| <= 65535 and gain <= 16383 keep the product inside int32; >> of a negative int is arithmetic here
__device__ __forceinline__ unsigned cal_corr(unsigned v, unsigned dark, unsigned gain, const CalArgs& a) {
    if ((int)v >= a.white) return v;
    const int e = (((int)v - (int)dark) * (int)gain + 2048) >> 12;
    const int r = a.pedestal + e;
    return (unsigned)(r < 0 ? 0 : r > a.maxv ? a.maxv : r);
}

template <typename T>
__global__ void __launch_bounds__(CAL_BX* CAL_BY) dofp_calibrate_kernel(const CalArgs a, const T* __restrict__ src, T* __restrict__ dst, int h, int w,
                                                                         size_t spitch, size_t dpitch, int P) {
    const int y = blockIdx.y * CAL_BY + threadIdx.y;
    const int xg = CAL_N * (blockIdx.x * CAL_BX + threadIdx.x);
    if (y >= h || xg >= w) return;
    const int nvalid = w - xg < CAL_N ? w - xg : CAL_N;
    const bool full = nvalid == CAL_N;
    const size_t t0 = (size_t)y * w + xg;                                  // the group's first element in the tight tables
    unsigned v[CAL_N], d[CAL_N], g[CAL_N], bad[CAL_N], o[CAL_N];
    df_load8(src + (size_t)y * spitch + xg, full && a.vsrc, nvalid, v);
    if (a.dark) {
        df_load8(a.dark + t0, full && a.vtab, nvalid, d);
    } else {
#pragma unroll
        for (int j = 0; j < CAL_N; ++j) d[j] = (unsigned)a.pedestal;
    }
    if (a.gain) {
        df_load8(a.gain + t0, full && a.vtab, nvalid, g);
    } else {
#pragma unroll
        for (int j = 0; j < CAL_N; ++j) g[j] = 4096u;
    }
    unsigned any = 0u;
    if (a.defect) {
        df_load8(a.defect + t0, full && a.vtab, nvalid, bad);
#pragma unroll
        for (int j = 0; j < CAL_N; ++j) any |= bad[j];
    }
#pragma unroll
    for (int j = 0; j < CAL_N; ++j) o[j] = cal_corr(v[j], d[j], g[j], a);
    if (any) {                                                             // rare: the good same-lattice neighbours, from global memory
#pragma unroll
        for (int j = 0; j < CAL_N; ++j) {
            if (j >= nvalid || !bad[j]) continue;
            const int x = xg + j;
            // all four neighbours are read before any is judged, an outside one at the site itself: independent loads, two round trips
            bool in[4];
            size_t t[4];
            unsigned nb[4], nv[4], nd[4], ng[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int ny = y + (k == 0 ? -P : k == 1 ? P : 0), nx = x + (k == 2 ? -P : k == 3 ? P : 0);
                in[k] = ny >= 0 && ny < h && nx >= 0 && nx < w;
                const int cy = in[k] ? ny : y, cx = in[k] ? nx : x;
                t[k] = (size_t)cy * w + cx;
                nb[k] = a.defect[t[k]];
                nv[k] = (unsigned)src[(size_t)cy * spitch + cx];
                nd[k] = a.dark ? (unsigned)a.dark[t[k]] : (unsigned)a.pedestal;
                ng[k] = a.gain ? (unsigned)a.gain[t[k]] : 4096u;
            }
            unsigned S = 0u, n = 0u;
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (in[k] && !nb[k]) {
                    S += cal_corr(nv[k], nd[k], ng[k], a);
                    ++n;
                }
            if (n) o[j] = (2u * S + n) / (2u * n);
        }
    }
    df_store8(dst + (size_t)y * dpitch + xg, full && a.vdst, nvalid, o);
}

template <typename T>
void cal_launch(CalArgs a, const void* src, void* dst, int h, int w, size_t spitch, size_t dpitch, int P, hipStream_t st) {
    const dim3 grid(shm_cdiv(shm_cdiv(w, CAL_N), CAL_BX), shm_cdiv(h, CAL_BY)), block(CAL_BX, CAL_BY);
    a.vsrc = (uintptr_t)src % (CAL_N * sizeof(T)) == 0 && spitch % CAL_N == 0;
    a.vdst = (uintptr_t)dst % (CAL_N * sizeof(T)) == 0 && dpitch % CAL_N == 0;
    a.vtab = w % CAL_N == 0 && (uintptr_t)a.dark % 16 == 0 && (uintptr_t)a.gain % 16 == 0 && (uintptr_t)a.defect % 8 == 0;          // null passes
    hipLaunchKernelGGL((dofp_calibrate_kernel<T>), grid, block, 0, st, a, (const T*)src, (T*)dst, h, w, spitch, dpitch, P);
}

}  // namespace

extern "C" int shm_dofp_calibrate(const void* src, int bits, int h, int w, size_t src_pitch, int pattern, const unsigned short* dark,
                                  const unsigned short* gain, const unsigned char* defect, int pedestal, int white, void* dst, size_t dst_pitch,
                                  void* stream) {
    const char* who = "shm_dofp_calibrate";
    SHM_REQUIRE(src && dst, SHM_E_SHAPE, "%s: null pointer (src or dst)", who);
    SHM_REQUIRE(bits >= 8 && bits <= 16, SHM_E_SHAPE, "%s: bits %d outside [8, 16]", who, bits);
    SHM_REQUIRE(pattern >= SHM_DOFP_MONO && pattern <= SHM_DOFP_GBRG, SHM_E_SHAPE, "%s: pattern %d unknown", who, pattern);
    const int P = pattern == SHM_DOFP_MONO ? 2 : 4;
    SHM_REQUIRE(h >= P && h <= DF_DIM_MAX && w >= P && w <= DF_DIM_MAX, SHM_E_SHAPE, "%s: sizes h %d, w %d outside [%d, %d]", who, h, w, P,
                DF_DIM_MAX);
    SHM_REQUIRE(src_pitch >= (size_t)w, SHM_E_SHAPE, "%s: src_pitch %zu below w %d", who, src_pitch, w);
    SHM_REQUIRE(dst_pitch >= (size_t)w, SHM_E_SHAPE, "%s: dst_pitch %zu below w %d", who, dst_pitch, w);
    SHM_REQUIRE(dst != src, SHM_E_SHAPE, "%s: dst == src (a defective site reads its neighbours from the source: not in place)", who);
    SHM_REQUIRE(pedestal >= 0 && pedestal <= 65535 - 16, SHM_E_SHAPE, "%s: pedestal %d outside [0, 65519]", who, pedestal);
    SHM_REQUIRE(white >= 1 && white <= 65536, SHM_E_SHAPE, "%s: white %d outside [1, 65536]", who, white);
    CalArgs a;
    a.dark = dark, a.gain = gain, a.defect = defect;
    a.pedestal = pedestal, a.white = white, a.maxv = (1 << bits) - 1;
    a.vsrc = a.vdst = a.vtab = 0;
    hipStream_t st = (hipStream_t)stream;
    if (bits == 8) cal_launch<unsigned char>(a, src, dst, h, w, src_pitch, dst_pitch, P, st);
    else cal_launch<unsigned short>(a, src, dst, h, w, src_pitch, dst_pitch, P, st);
    SHM_LAUNCH_CHECK(who);
    return SHM_OK;
}
