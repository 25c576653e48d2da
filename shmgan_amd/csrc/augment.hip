// Train-time augmentation at the decoded bytes: the four (or five) uint8 images of ONE sample -> the sample's five training planes,
// cropped, mirrored and -- where a mirror changes which polariser a view stands for -- re-mixed, in the one pass that resizes them.
//
//   shm_augment_views_u8   shm_polar_views_u8 (polar.hip) with a sampling window and two mirrors on the READ side: output pixel
//                          (oy, ox) samples the source at the position of output pixel (sy, sx) of the unmirrored result, so a
//                          block's stores stay 60 contiguous bytes per thread whatever the flips.  A crop only moves and scales
//                          the sampling positions; the taps are clamped to the image, so a crop edge interpolates against its
//                          real neighbours.  SHM_AUG_DIR resamples a fifth source for plane 4; MIN / STOKES make it from the
//                          four views per tap (polar_est.h).  With `mix` the four view bytes of a tap become M . v, clamped to
//                          the byte range, before the lerp; the estimate is made from the unmixed bytes (the unpolarised part
//                          is mirror-invariant) and a fifth source is never mixed.
// One thread per output pixel, 4 taps x n_src x 3 byte loads; pointers and the two small matrices travel by value.  The per-pixel
// body is augment_px.h (the sampler: bilinear.h), which the batched kernel (augment_batch.hip) and polar.hip include too.
#include "augment_px.h"

namespace {

struct AugmentArgs {
    const unsigned char* src[5];                // [4] only for SHM_AUG_DIR
    float* dst[5];
    float coef[12];                             // row-major 3x4 Stokes matrix; STOKES only
    float mix[16];                              // row-major 4x4 view mix; MIX only
};

template <int MODE, bool MIX>
__global__ void __launch_bounds__(AU_NT) augment_views_u8_kernel(const AugmentArgs a, int hin, int win, int ho, int wo, float hs, float ws,
                                                                 float cy, float cx, float scale, int flip_ud, int flip_lr) {
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;       // (oy, ox)
    if (idx >= (size_t)ho * wo) return;
    augment_pixel<MODE, MIX>(a, idx, hin, win, ho, wo, hs, ws, cy, cx, scale, flip_ud, flip_lr);     // augment_px.h
}

template <int MODE>
void launch(bool mix, dim3 grid, hipStream_t st, const AugmentArgs& a, int hin, int win, int ho, int wo, float hs, float ws, float cy, float cx,
            float scale, int flip_ud, int flip_lr) {
    if (mix)
        hipLaunchKernelGGL((augment_views_u8_kernel<MODE, true>), grid, dim3(AU_NT), 0, st, a, hin, win, ho, wo, hs, ws, cy, cx, scale, flip_ud, flip_lr);
    else
        hipLaunchKernelGGL((augment_views_u8_kernel<MODE, false>), grid, dim3(AU_NT), 0, st, a, hin, win, ho, wo, hs, ws, cy, cx, scale, flip_ud, flip_lr);
}

}  // namespace

extern "C" int shm_augment_views_u8(const unsigned char* const* src_ptrs, int n_src, int hin, int win, int mode, const float* coef, const float* mix,
                                    float crop_y, float crop_x, float crop_h, float crop_w, int flip_ud, int flip_lr, float* const* dst_ptrs, int ho,
                                    int wo, float scale, void* stream) {
    SHM_REQUIRE(src_ptrs && dst_ptrs, SHM_E_SHAPE, "shm_augment_views_u8: null pointer (src_ptrs or dst_ptrs)");
    SHM_REQUIRE(mode == SHM_POLAR_MIN || mode == SHM_POLAR_STOKES || mode == SHM_AUG_DIR, SHM_E_SHAPE, "shm_augment_views_u8: mode %d unknown", mode);
    const int want = mode == SHM_AUG_DIR ? 5 : 4;
    SHM_REQUIRE(n_src == want, SHM_E_SHAPE, "shm_augment_views_u8: n_src %d does not fit mode %d, which takes %d sources", n_src, mode, want);
    AugmentArgs a;
    for (int v = 0; v < 5; ++v) {
        SHM_REQUIRE(v >= n_src || src_ptrs[v], SHM_E_SHAPE, "shm_augment_views_u8: null pointer (source %d)", v);
        a.src[v] = v < n_src ? src_ptrs[v] : nullptr;
    }
    for (int v = 0; v < 5; ++v) {
        SHM_REQUIRE(dst_ptrs[v], SHM_E_SHAPE, "shm_augment_views_u8: null pointer (destination plane %d)", v);
        a.dst[v] = dst_ptrs[v];
    }
    SHM_REQUIRE(hin >= 1 && hin <= AU_DIM_MAX && win >= 1 && win <= AU_DIM_MAX && ho >= 1 && ho <= AU_DIM_MAX && wo >= 1 && wo <= AU_DIM_MAX,
                SHM_E_SHAPE, "shm_augment_views_u8: sizes hin %d, win %d, ho %d, wo %d outside [1, %d]", hin, win, ho, wo, AU_DIM_MAX);
    // written so that a NaN fails them
    SHM_REQUIRE(crop_h > 0.f && crop_w > 0.f, SHM_E_SHAPE, "shm_augment_views_u8: empty crop (crop_h %g, crop_w %g)", (double)crop_h, (double)crop_w);
    SHM_REQUIRE(crop_y >= 0.f && crop_x >= 0.f && (double)crop_y + (double)crop_h <= (double)hin && (double)crop_x + (double)crop_w <= (double)win,
                SHM_E_SHAPE, "shm_augment_views_u8: the crop %g x %g at (%g, %g) does not lie inside the %d x %d image", (double)crop_h,
                (double)crop_w, (double)crop_y, (double)crop_x, hin, win);
    SHM_REQUIRE(mode != SHM_POLAR_STOKES || coef, SHM_E_SHAPE, "shm_augment_views_u8: SHM_POLAR_STOKES needs coef (float[12])");
    for (int i = 0; i < 12; ++i) a.coef[i] = mode == SHM_POLAR_STOKES ? coef[i] : 0.f;
    for (int i = 0; i < 16; ++i) a.mix[i] = mix ? mix[i] : 0.f;
    const dim3 grid(shm_cdiv((long)ho * wo, AU_NT));
    const float hs = crop_h / (float)ho, ws = crop_w / (float)wo;
    hipStream_t st = (hipStream_t)stream;
    if (mode == SHM_AUG_DIR)
        launch<SHM_AUG_DIR>(mix != nullptr, grid, st, a, hin, win, ho, wo, hs, ws, crop_y, crop_x, scale, flip_ud, flip_lr);
    else if (mode == SHM_POLAR_MIN)
        launch<SHM_POLAR_MIN>(mix != nullptr, grid, st, a, hin, win, ho, wo, hs, ws, crop_y, crop_x, scale, flip_ud, flip_lr);
    else
        launch<SHM_POLAR_STOKES>(mix != nullptr, grid, st, a, hin, win, ho, wo, hs, ws, crop_y, crop_x, scale, flip_ud, flip_lr);
    SHM_LAUNCH_CHECK("shm_augment_views_u8");
    return SHM_OK;
}
