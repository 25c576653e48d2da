// A whole batch through the augmenting resize in one launch: the decoded uint8 images of up to SHM_AUG_GROUP samples, each of its
// own size and with its own crop, mirrors, view mix and plane order -> the samples' slices of the loader's five [B,ho,wo,3] tensors.
//
//   shm_augment_batch_u8   grid (cdiv(ho*wo, 256), n): block row blockIdx.y reads its own sample descriptor from the kernel arguments
//                          (by value, block-uniform: the pointers, sizes and crop sit in SGPRs) and then runs the per-pixel body of
//                          shm_augment_views_u8 (augment_px.h: ONE definition of the arithmetic), so a sample's bits are those of that
//                          entry point called for the sample alone.  The view mix is a per-sample flag: a block-uniform branch between
//                          the two instantiations of the body.  Where a mirror permutes the views, the descriptor names the plane
//                          every view lands in.  n > SHM_AUG_GROUP is cut into cdiv(n, SHM_AUG_GROUP) launches here.
// A descriptor is 72 bytes on the device, so 8 of them with the shared part (two small matrices, five plane pointers) are 760 bytes
// of kernel arguments, far below the 4 KiB limit: SHM_AUG_GROUP is 8, a training batch, and nothing forces less.
#include "augment_px.h"

namespace {

static_assert(SHM_AUG_GROUP == 8, "the descriptor table is sized for the header's group");

struct BatchSample {
    const unsigned char* src[5];                // [4] only for SHM_AUG_DIR
    int hin, win;
    float hs, ws, cy, cx;                       // crop extent / output size, crop origin
    int flags;                                  // bit 0 flip_ud, bit 1 flip_lr, bit 2 mix
    int planes;                                 // view v lands in plane (planes >> 2 v) & 3
};

struct BatchArgs {
    BatchSample s[SHM_AUG_GROUP];
    float* dst[5];                              // the five tensors at the group's first sample
    size_t stride;                              // floats from one sample's plane to the next
    float coef[12];                             // row-major 3x4 Stokes matrix; STOKES only
    float mix[16];                              // row-major 4x4 view mix; samples with the mix flag only
};

struct PixelArgs {                              // what augment_pixel reads, for one sample
    const unsigned char* src[5];
    float* dst[5];
    const float* coef;
    const float* mix;
};

template <int MODE>
__global__ void __launch_bounds__(AU_NT) augment_batch_u8_kernel(const BatchArgs a, int ho, int wo, float scale) {
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;       // (oy, ox)
    if (idx >= (size_t)ho * wo) return;
    const BatchSample& d = a.s[blockIdx.y];
    const size_t off = (size_t)blockIdx.y * a.stride;
    PixelArgs p;
#pragma unroll
    for (int v = 0; v < 5; ++v) p.src[v] = d.src[v];
#pragma unroll
    for (int v = 0; v < 4; ++v) {
        const int pl = (d.planes >> (2 * v)) & 3;
        p.dst[v] = (pl == 0 ? a.dst[0] : pl == 1 ? a.dst[1] : pl == 2 ? a.dst[2] : a.dst[3]) + off;
    }
    p.dst[4] = a.dst[4] + off;
    p.coef = a.coef;
    p.mix = a.mix;
    if (d.flags & 4)
        augment_pixel<MODE, true>(p, idx, d.hin, d.win, ho, wo, d.hs, d.ws, d.cy, d.cx, scale, d.flags & 1, d.flags & 2);
    else
        augment_pixel<MODE, false>(p, idx, d.hin, d.win, ho, wo, d.hs, d.ws, d.cy, d.cx, scale, d.flags & 1, d.flags & 2);
}

template <int MODE>
void launch(dim3 grid, hipStream_t st, const BatchArgs& a, int ho, int wo, float scale) {
    hipLaunchKernelGGL((augment_batch_u8_kernel<MODE>), grid, dim3(AU_NT), 0, st, a, ho, wo, scale);
}

}  // namespace

extern "C" int shm_augment_batch_u8(const shm_aug_sample* samples, int n, int n_src, int mode, const float* coef, const float* mix,
                                    float* const* dst_ptrs, size_t sample_stride, int ho, int wo, float scale, void* stream) {
    SHM_REQUIRE(samples && dst_ptrs, SHM_E_SHAPE, "shm_augment_batch_u8: null pointer (samples or dst_ptrs)");
    SHM_REQUIRE(n >= 1, SHM_E_SHAPE, "shm_augment_batch_u8: n %d < 1", n);
    SHM_REQUIRE(mode == SHM_POLAR_MIN || mode == SHM_POLAR_STOKES || mode == SHM_AUG_DIR, SHM_E_SHAPE, "shm_augment_batch_u8: mode %d unknown", mode);
    const int want = mode == SHM_AUG_DIR ? 5 : 4;
    SHM_REQUIRE(n_src == want, SHM_E_SHAPE, "shm_augment_batch_u8: n_src %d does not fit mode %d, which takes %d sources", n_src, mode, want);
    for (int v = 0; v < 5; ++v) SHM_REQUIRE(dst_ptrs[v], SHM_E_SHAPE, "shm_augment_batch_u8: null pointer (destination plane %d)", v);
    SHM_REQUIRE(ho >= 1 && ho <= AU_DIM_MAX && wo >= 1 && wo <= AU_DIM_MAX, SHM_E_SHAPE, "shm_augment_batch_u8: sizes ho %d, wo %d outside [1, %d]", ho,
                wo, AU_DIM_MAX);
    SHM_REQUIRE(n == 1 || sample_stride >= (size_t)ho * wo * 3, SHM_E_SHAPE, "shm_augment_batch_u8: sample_stride %zu is less than a plane of %d x %d x 3",
                sample_stride, ho, wo);
    SHM_REQUIRE(mode != SHM_POLAR_STOKES || coef, SHM_E_SHAPE, "shm_augment_batch_u8: SHM_POLAR_STOKES needs coef (float[12])");
    // every sample before the first launch: the rules of shm_augment_views_u8, and the plane list
    for (int i = 0; i < n; ++i) {
        const shm_aug_sample& s = samples[i];
        for (int v = 0; v < n_src; ++v) SHM_REQUIRE(s.src[v], SHM_E_SHAPE, "shm_augment_batch_u8: sample %d: null pointer (source %d)", i, v);
        SHM_REQUIRE(s.hin >= 1 && s.hin <= AU_DIM_MAX && s.win >= 1 && s.win <= AU_DIM_MAX, SHM_E_SHAPE,
                    "shm_augment_batch_u8: sample %d: sizes hin %d, win %d outside [1, %d]", i, s.hin, s.win, AU_DIM_MAX);
        // written so that a NaN fails them
        SHM_REQUIRE(s.crop_h > 0.f && s.crop_w > 0.f, SHM_E_SHAPE, "shm_augment_batch_u8: sample %d: empty crop (crop_h %g, crop_w %g)", i,
                    (double)s.crop_h, (double)s.crop_w);
        SHM_REQUIRE(s.crop_y >= 0.f && s.crop_x >= 0.f && (double)s.crop_y + (double)s.crop_h <= (double)s.hin &&
                        (double)s.crop_x + (double)s.crop_w <= (double)s.win,
                    SHM_E_SHAPE, "shm_augment_batch_u8: sample %d: the crop %g x %g at (%g, %g) does not lie inside the %d x %d image", i,
                    (double)s.crop_h, (double)s.crop_w, (double)s.crop_y, (double)s.crop_x, s.hin, s.win);
        SHM_REQUIRE(!s.mix || mix, SHM_E_SHAPE, "shm_augment_batch_u8: sample %d: the mix flag needs mix (float[16])", i);
        int seen = 0;
        for (int v = 0; v < 4; ++v)
            if (s.plane[v] >= 0 && s.plane[v] < 4) seen |= 1 << s.plane[v];
        SHM_REQUIRE(seen == 15, SHM_E_SHAPE, "shm_augment_batch_u8: sample %d: planes (%d, %d, %d, %d) are not a permutation of 0..3", i, s.plane[0],
                    s.plane[1], s.plane[2], s.plane[3]);
    }
    BatchArgs a;
    a.stride = sample_stride;
    for (int i = 0; i < 12; ++i) a.coef[i] = mode == SHM_POLAR_STOKES ? coef[i] : 0.f;
    for (int i = 0; i < 16; ++i) a.mix[i] = mix ? mix[i] : 0.f;
    hipStream_t st = (hipStream_t)stream;
    for (int i0 = 0; i0 < n; i0 += SHM_AUG_GROUP) {
        const int m = n - i0 < SHM_AUG_GROUP ? n - i0 : SHM_AUG_GROUP;
        for (int v = 0; v < 5; ++v) a.dst[v] = dst_ptrs[v] + (size_t)i0 * sample_stride;
        for (int j = 0; j < SHM_AUG_GROUP; ++j) {
            const shm_aug_sample& s = samples[i0 + (j < m ? j : 0)];        // rows past m are never read: no block has that blockIdx.y
            BatchSample& d = a.s[j];
            for (int v = 0; v < 5; ++v) d.src[v] = v < n_src ? s.src[v] : nullptr;
            d.hin = s.hin;
            d.win = s.win;
            d.hs = s.crop_h / (float)ho;
            d.ws = s.crop_w / (float)wo;
            d.cy = s.crop_y;
            d.cx = s.crop_x;
            d.flags = (s.flip_ud ? 1 : 0) | (s.flip_lr ? 2 : 0) | (s.mix ? 4 : 0);
            d.planes = s.plane[0] | s.plane[1] << 2 | s.plane[2] << 4 | s.plane[3] << 6;
        }
        const dim3 grid(shm_cdiv((long)ho * wo, AU_NT), m);
        if (mode == SHM_AUG_DIR)
            launch<SHM_AUG_DIR>(grid, st, a, ho, wo, scale);
        else if (mode == SHM_POLAR_MIN)
            launch<SHM_POLAR_MIN>(grid, st, a, ho, wo, scale);
        else
            launch<SHM_POLAR_STOKES>(grid, st, a, ho, wo, scale);
        SHM_LAUNCH_CHECK("shm_augment_batch_u8");
    }
    return SHM_OK;
}
