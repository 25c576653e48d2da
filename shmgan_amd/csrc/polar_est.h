// The per-tap estimated-diffuse value e(v0..v3) of include/shmgan_hip.h ("polarimetry"), shared by the two kernels that make the
// loader's fifth plane from the four views (polar.hip, augment.hip): one definition, so that the two agree bit for bit.
#pragma once
#include "common.h"

#include <math.h>

// S1^2 + S2^2 of one tap: the square of the polarised intensity that polar_estimate<SHM_POLAR_STOKES> subtracts (specmask.hip takes its
// maximum over the channels BEFORE the root).  Rows 1 and 2 of the matrix, summed left to right as below.
__device__ __forceinline__ float polar_strength2(const float* c, float v0, float v1, float v2, float v3) {
    const float s1 = c[4] * v0 + c[5] * v1 + c[6] * v2 + c[7] * v3;
    const float s2 = c[8] * v0 + c[9] * v1 + c[10] * v2 + c[11] * v3;
    return s1 * s1 + s2 * s2;
}

template <int MODE>
__device__ __forceinline__ float polar_estimate(const float* c, float v0, float v1, float v2, float v3) {
    if (MODE == SHM_POLAR_MIN) return fminf(fminf(v0, v1), fminf(v2, v3));
    const float s0 = c[0] * v0 + c[1] * v1 + c[2] * v2 + c[3] * v3;
    const float s1 = c[4] * v0 + c[5] * v1 + c[6] * v2 + c[7] * v3;
    const float s2 = c[8] * v0 + c[9] * v1 + c[10] * v2 + c[11] * v3;
    // the fitted intensity minimum over all polariser angles, 0.5 (S0 - P), kept inside the byte range
    return fminf(fmaxf(0.5f * (s0 - sqrtf(s1 * s1 + s2 * s2)), 0.f), 255.f);
}
