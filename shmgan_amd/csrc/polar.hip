// Polarimetry on the device: the estimated-diffuse target the reference only ever reads from a pre-computed ED/ directory
// (utils.py:68-123 calculate_estimate_diffuse, whose imwrite is commented out), and the Stokes / DoP / AoLP maps of calcDOP
// (SHM.py:1157-1169).
//
//   shm_polar_views_u8   the four decoded uint8 views of ONE sample -> the sample's five training planes: views 0..3 resized by
//                        the sampler of bilinear.h, plane 4 the same interpolation of a per-tap estimate e(v0..v3): the per-pixel
//                        body of augment_px.h without crop, horizontal mirror or view mix.  The estimate is made at SOURCE
//                        resolution (per tap) and then resized, which is what the reference's helper followed by its loader
//                        computes; min and sqrt do not commute with the interpolation.
//                        One thread per output pixel, 48 byte loads (3 channels x 4 views x 4 corners), every tap read once and
//                        used for both its view and the estimate.  The nine pointers travel by value in the argument struct.
//   shm_polar_maps       (S0, S1, S2) = C v per element of four float32 views; s0, dop = sqrt(S1^2 + S2^2) / S0 (0 where
//                        S0 == 0), aolp = 0.5 atan2(S2, S1).  Grid-stride, float4 when everything is 16-byte aligned.
// Both are launch- and latency-bound elementwise kernels; nothing here is tuned beyond coalesced access.
#include "augment_px.h"

#include <math.h>

namespace {

constexpr int PL_NT = 256;
constexpr int PL_DIM_MAX = 32768;               // hin, win, ho, wo
constexpr int PL_MAPS_BLOCKS = 2048;            // grid cap of the maps kernel (grid-stride beyond it)

struct PolarViewArgs {
    const unsigned char* src[4];
    float* dst[5];
    float coef[12];                             // row-major 3x4: (S0, S1, S2) = coef . (v0..v3); STOKES only
};

struct PolarMapArgs {
    const float* view[4];
    float* s0;
    float* dop;
    float* aolp;
    float coef[12];
};

template <int MODE>
__global__ void __launch_bounds__(PL_NT) polar_views_u8_kernel(const PolarViewArgs a, int hin, int win, int ho, int wo, float hs, float ws,
                                                               float scale, int flip_ud) {
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;       // (oy, ox)
    if (idx >= (size_t)ho * wo) return;
    augment_pixel<MODE, false>(a, idx, hin, win, ho, wo, hs, ws, 0.f, 0.f, scale, flip_ud, 0);      // augment_px.h: no crop, no mix
}

__device__ __forceinline__ void polar_map_one(const float* c, float v0, float v1, float v2, float v3, float& s0, float& dop, float& aolp) {
    s0 = c[0] * v0 + c[1] * v1 + c[2] * v2 + c[3] * v3;
    const float s1 = c[4] * v0 + c[5] * v1 + c[6] * v2 + c[7] * v3;
    const float s2 = c[8] * v0 + c[9] * v1 + c[10] * v2 + c[11] * v3;
    dop = s0 != 0.f ? sqrtf(s1 * s1 + s2 * s2) / s0 : 0.f;          // divide_no_nan
    aolp = 0.5f * atan2f(s2, s1);
}

template <bool VEC>
__global__ void __launch_bounds__(PL_NT) polar_maps_kernel(const PolarMapArgs a, size_t n) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    const size_t i0 = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (VEC) {
        for (size_t i = i0; i < n / 4; i += stride) {
            const f32x4 v0 = ld4(a.view[0] + 4 * i), v1 = ld4(a.view[1] + 4 * i), v2 = ld4(a.view[2] + 4 * i), v3 = ld4(a.view[3] + 4 * i);
            f32x4 s0, dop, aolp;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                float s, d, t;
                polar_map_one(a.coef, v0[q], v1[q], v2[q], v3[q], s, d, t);
                s0[q] = s;
                dop[q] = d;
                aolp[q] = t;
            }
            if (a.s0) st4(a.s0 + 4 * i, s0);
            if (a.dop) st4(a.dop + 4 * i, dop);
            if (a.aolp) st4(a.aolp + 4 * i, aolp);
        }
    } else {
        for (size_t i = i0; i < n; i += stride) {
            float s, d, t;
            polar_map_one(a.coef, a.view[0][i], a.view[1][i], a.view[2][i], a.view[3][i], s, d, t);
            if (a.s0) a.s0[i] = s;
            if (a.dop) a.dop[i] = d;
            if (a.aolp) a.aolp[i] = t;
        }
    }
}

}  // namespace

extern "C" int shm_polar_views_u8(const unsigned char* const* src_ptrs, int hin, int win, const float* coef, int mode, float* const* dst_ptrs,
                                  int ho, int wo, float scale, int flip_ud, void* stream) {
    SHM_REQUIRE(src_ptrs && dst_ptrs, SHM_E_SHAPE, "shm_polar_views_u8: null pointer (src_ptrs or dst_ptrs)");
    PolarViewArgs a;
    for (int v = 0; v < 4; ++v) {
        SHM_REQUIRE(src_ptrs[v], SHM_E_SHAPE, "shm_polar_views_u8: null pointer (source view %d)", v);
        a.src[v] = src_ptrs[v];
    }
    for (int v = 0; v < 5; ++v) {
        SHM_REQUIRE(dst_ptrs[v], SHM_E_SHAPE, "shm_polar_views_u8: null pointer (destination plane %d)", v);
        a.dst[v] = dst_ptrs[v];
    }
    SHM_REQUIRE(hin >= 1 && hin <= PL_DIM_MAX && win >= 1 && win <= PL_DIM_MAX && ho >= 1 && ho <= PL_DIM_MAX && wo >= 1 && wo <= PL_DIM_MAX,
                SHM_E_SHAPE, "shm_polar_views_u8: sizes hin %d, win %d, ho %d, wo %d outside [1, %d]", hin, win, ho, wo, PL_DIM_MAX);
    SHM_REQUIRE(mode == SHM_POLAR_MIN || mode == SHM_POLAR_STOKES, SHM_E_SHAPE, "shm_polar_views_u8: mode %d unknown", mode);
    SHM_REQUIRE(mode != SHM_POLAR_STOKES || coef, SHM_E_SHAPE, "shm_polar_views_u8: SHM_POLAR_STOKES needs coef (float[12])");
    for (int i = 0; i < 12; ++i) a.coef[i] = mode == SHM_POLAR_STOKES ? coef[i] : 0.f;
    const dim3 grid(shm_cdiv((long)ho * wo, PL_NT)), block(PL_NT);
    const float hs = (float)hin / (float)ho, ws = (float)win / (float)wo;
    hipStream_t st = (hipStream_t)stream;
    if (mode == SHM_POLAR_MIN)
        hipLaunchKernelGGL(polar_views_u8_kernel<SHM_POLAR_MIN>, grid, block, 0, st, a, hin, win, ho, wo, hs, ws, scale, flip_ud);
    else
        hipLaunchKernelGGL(polar_views_u8_kernel<SHM_POLAR_STOKES>, grid, block, 0, st, a, hin, win, ho, wo, hs, ws, scale, flip_ud);
    SHM_LAUNCH_CHECK("shm_polar_views_u8");
    return SHM_OK;
}

extern "C" int shm_polar_maps(const float* const* view_ptrs, size_t n, const float* coef, float* s0, float* dop, float* aolp, void* stream) {
    SHM_REQUIRE(view_ptrs && coef, SHM_E_SHAPE, "shm_polar_maps: null pointer (view_ptrs or coef)");
    SHM_REQUIRE(n >= 1, SHM_E_SHAPE, "shm_polar_maps: n is 0");
    PolarMapArgs a;
    uintptr_t bits = (uintptr_t)s0 | (uintptr_t)dop | (uintptr_t)aolp;
    for (int v = 0; v < 4; ++v) {
        SHM_REQUIRE(view_ptrs[v], SHM_E_SHAPE, "shm_polar_maps: null pointer (view %d)", v);
        a.view[v] = view_ptrs[v];
        bits |= (uintptr_t)view_ptrs[v];
    }
    if (!s0 && !dop && !aolp) return SHM_OK;          // nothing asked for
    a.s0 = s0;
    a.dop = dop;
    a.aolp = aolp;
    for (int i = 0; i < 12; ++i) a.coef[i] = coef[i];
    const bool vec = n % 4 == 0 && (bits & 15) == 0;
    const size_t items = vec ? n / 4 : n;
    const dim3 grid(shm_grid_cap(items, PL_NT, PL_MAPS_BLOCKS)), block(PL_NT);
    hipStream_t st = (hipStream_t)stream;
    if (vec)
        hipLaunchKernelGGL(polar_maps_kernel<true>, grid, block, 0, st, a, n);
    else
        hipLaunchKernelGGL(polar_maps_kernel<false>, grid, block, 0, st, a, n);
    SHM_LAUNCH_CHECK("shm_polar_maps");
    return SHM_OK;
}
