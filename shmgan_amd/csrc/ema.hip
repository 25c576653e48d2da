// Exponential moving average of a flat fp32 weight buffer (shm_ema_update): one streaming pass, 12 bytes per element (read ema and w,
// write ema), no LDS, no atomics -- every element is computed by exactly one lane from its own two inputs, so the result is bitwise
// reproducible and does not depend on the launch geometry or on which of the two access forms ran.
#include "common.h"

#define EMA_NT 256

// The pinned arithmetic (include/shmgan_hip.h): t = w - ema in fp32, then ONE fused multiply-add.  COPY (decay == 0): ema = w, bit for bit.
template <bool COPY>
__device__ __forceinline__ float ema_one(float e, float w, float om) {
    return COPY ? w : __builtin_fmaf(om, w - e, e);
}
template <bool COPY>
__device__ __forceinline__ f32x4 ema_four(f32x4 e, f32x4 w, float om) {
    f32x4 r;
#pragma unroll
    for (int k = 0; k < 4; ++k) r[k] = ema_one<COPY>(e[k], w[k], om);
    return r;
}

// VEC: ema and w share their misalignment to 16 bytes.  `head` (< 4) elements up to the first 16-byte boundary and the `n - head - 4 nvec`
// (< 4) behind the last whole vector are done by the first lanes of the grid, one element each; the vectors in between go 16 bytes per
// lane, one per trip of the grid-stride loop.  !VEC: 4-byte lanes, any 4-byte alignment.
// Measured on the generator's 18.5 M floats: one vector per trip under 8192 blocks streams faster than two or four
// per trip with the loads issued ahead (30 against 35 us), than a cap of 2048 or 4096 blocks (34, 31 us) and than non-temporal accesses.
template <bool VEC, bool COPY>
__global__ __launch_bounds__(EMA_NT) void ema_update_kernel(float* __restrict__ ema, const float* __restrict__ w, size_t n, size_t head, float om,
                                                            const unsigned* __restrict__ abort_word) {
    // a kernel of this step gave up (shm_adam_clip's abort word: the weights were not updated either) -- write nothing
    if (abort_word && __hip_atomic_load(abort_word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0u) return;
    const size_t g = (size_t)blockIdx.x * EMA_NT + threadIdx.x;
    const size_t stride = (size_t)gridDim.x * EMA_NT;
    if (!VEC) {
        for (size_t i = g; i < n; i += stride) ema[i] = ema_one<COPY>(COPY ? 0.f : ema[i], w[i], om);
        return;
    }
    const size_t nvec = (n - head) / 4;              // the host passes head <= n
    const size_t tail0 = head + 4 * nvec;
    if (g < head) ema[g] = ema_one<COPY>(COPY ? 0.f : ema[g], w[g], om);
    if (g < n - tail0) ema[tail0 + g] = ema_one<COPY>(COPY ? 0.f : ema[tail0 + g], w[tail0 + g], om);
    f32x4* __restrict__ e4 = (f32x4*)(ema + head);
    const f32x4* __restrict__ w4 = (const f32x4*)(w + head);
    for (size_t i = g; i < nvec; i += stride) {
        const f32x4 wa = w4[i];
        e4[i] = ema_four<COPY>(COPY ? wa : e4[i], wa, om);
    }
}

extern "C" int shm_ema_update(float* ema, const float* w, size_t n, float decay, const unsigned* abort_word, void* stream) {
    SHM_REQUIRE(decay >= 0.0f && decay < 1.0f, SHM_E_SHAPE, "shm_ema_update: decay %g is not in [0, 1)", (double)decay);      // a NaN fails both
    if (n == 0) return SHM_OK;
    SHM_REQUIRE(ema, SHM_E_SHAPE, "shm_ema_update: ema is a null pointer");
    SHM_REQUIRE(w, SHM_E_SHAPE, "shm_ema_update: w is a null pointer");
    const uintptr_t pe = (uintptr_t)ema, pw = (uintptr_t)w;
    SHM_REQUIRE(n <= (SIZE_MAX - (pe > pw ? pe : pw)) / sizeof(float), SHM_E_SHAPE, "shm_ema_update: n = %zu floats do not fit the address space", n);
    SHM_REQUIRE(pe + n * sizeof(float) <= pw || pw + n * sizeof(float) <= pe, SHM_E_SHAPE, "shm_ema_update: ema and w overlap (%zu floats at %p and %p)", n,
                (void*)ema, (const void*)w);
    SHM_REQUIRE(pe % 4 == 0 && pw % 4 == 0, SHM_E_SHAPE, "shm_ema_update: ema and w must be 4-byte aligned");
    const float om = 1.0f - decay;
    const bool copy = decay == 0.0f;
    const bool vec = pe % 16 == pw % 16;
    size_t head = vec ? ((16 - pe % 16) % 16) / 4 : 0;
    if (head > n) head = n;
    // 16 bytes per lane (4-byte lanes in the scalar form), grid-stride under the cap (shm_adam_clip's)
    const int blocks = shm_grid_cap(n, vec ? 4 * EMA_NT : EMA_NT, SHM_EMA_MAX_BLOCKS);
    const dim3 grid(blocks), block(EMA_NT);
    hipStream_t st = (hipStream_t)stream;
    if (vec && copy) hipLaunchKernelGGL((ema_update_kernel<true, true>), grid, block, 0, st, ema, w, n, head, om, abort_word);
    else if (vec) hipLaunchKernelGGL((ema_update_kernel<true, false>), grid, block, 0, st, ema, w, n, head, om, abort_word);
    else if (copy) hipLaunchKernelGGL((ema_update_kernel<false, true>), grid, block, 0, st, ema, w, n, head, om, abort_word);
    else hipLaunchKernelGGL((ema_update_kernel<false, false>), grid, block, 0, st, ema, w, n, head, om, abort_word);
    SHM_LAUNCH_CHECK("shm_ema_update");
    return SHM_OK;
}
