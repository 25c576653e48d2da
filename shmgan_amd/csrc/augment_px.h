// The per-pixel body of the augmenting resize, shared by the kernel of one sample (augment.hip), the batched one (augment_batch.hip)
// and, at identity parameters, shm_polar_views_u8 (polar.hip): one definition of the mirrors, the view mix and the estimate around
// the sampler of bilinear.h, so that they agree bit for bit.
#pragma once
#include "bilinear.h"
#include "polar_est.h"

#include <math.h>

constexpr int AU_NT = 256;
constexpr int AU_DIM_MAX = 32768;               // hin, win, ho, wo

// Output pixel idx = (oy, ox) of one sample.  ARGS has the members src[5] (uint8 [hin,win,3]; [4] only for SHM_AUG_DIR), dst[5]
// (float32 [ho,wo,3]), coef (the row-major 3x4 Stokes matrix; STOKES only) and mix (the row-major 4x4 view mix; MIX only), arrays
// or pointers.  Every argument but idx is block-uniform.
template <int MODE, bool MIX, class ARGS>
__device__ __forceinline__ void augment_pixel(const ARGS& a, size_t idx, int hin, int win, int ho, int wo, float hs, float ws, float cy, float cx,
                                              float scale, int flip_ud, int flip_lr) {
    constexpr int NSRC = MODE == SHM_AUG_DIR ? 5 : 4;
    const int ox = (int)(idx % wo), oy = (int)(idx / wo);
    // the mirrors on the READ side: (oy, ox) samples at the position of output pixel (sy, sx) of the unmirrored result
    const int sy = flip_ud ? ho - 1 - oy : oy, sx = flip_lr ? wo - 1 - ox : ox;
    const BilinearTaps at = bilinear_taps(sx, sy, hin, win, win, hs, ws, cy, cx);
    const float ly = at.ly, lx = at.lx;
    const size_t itl = at.tl * 3, itr = at.tr * 3, ibl = at.bl * 3, ibr = at.br * 3;
    const size_t o = ((size_t)oy * wo + ox) * 3;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        float tl[5], tr[5], bl[5], br[5];
#pragma unroll
        for (int v = 0; v < NSRC; ++v) {
            tl[v] = a.src[v][itl + k];
            tr[v] = a.src[v][itr + k];
            bl[v] = a.src[v][ibl + k];
            br[v] = a.src[v][ibr + k];
        }
        if constexpr (MODE != SHM_AUG_DIR) {
            tl[4] = polar_estimate<MODE>(a.coef, tl[0], tl[1], tl[2], tl[3]);
            tr[4] = polar_estimate<MODE>(a.coef, tr[0], tr[1], tr[2], tr[3]);
            bl[4] = polar_estimate<MODE>(a.coef, bl[0], bl[1], bl[2], bl[3]);
            br[4] = polar_estimate<MODE>(a.coef, br[0], br[1], br[2], br[3]);
        }
        if constexpr (MIX) {
            float* const taps[4] = {tl, tr, bl, br};
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                float* q = taps[t];
                const float v0 = q[0], v1 = q[1], v2 = q[2], v3 = q[3];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const float* m = a.mix + 4 * i;
                    q[i] = fminf(fmaxf(((m[0] * v0 + m[1] * v1) + m[2] * v2) + m[3] * v3, 0.f), 255.f);
                }
            }
        }
#pragma unroll
        for (int v = 0; v < 5; ++v) a.dst[v][o + k] = bilinear_lerp(tl[v], tr[v], bl[v], br[v], lx, ly) * scale;
    }
}
