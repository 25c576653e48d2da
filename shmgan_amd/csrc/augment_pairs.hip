// The mask network's training pairs in one call: the decoded uint8 image [hin,win,3] and mask [hin,win] of up to SHM_AUG_GROUP
// samples per launch, each of its own size and with its own crop and mirrors -> the samples' slices of the two [n,ho,wo,1] tensors
// SpecSeg.train_step takes: x, the standardised Y plane, and y, the mask in [0,1].
//
//   shm_augment_pairs_u8   two launches per group, both with grid (pairs_blocks(ho*wo), samples of the group); block row blockIdx.y
//                          reads its own descriptor from the kernel arguments (by value, block-uniform: pointers, sizes and crop sit
//                          in SGPRs), as augment_batch.hip does.
//     resample   per output pixel the coordinate, taps and lerp of bilinear.h (ONE definition, shared with shm_augment_views_u8):
//                the mask's lerp times 1/255 goes to y; the three channels' lerps times 1/255 are converted by rgb2yuv (yuv.h, the
//                function shm_rgb2yuv_std calls) in registers; the unscaled Y goes to x, and Y, U and V enter the block's two f64
//                sums, which the block writes to ITS slot of the caller's workspace.  No atomics.
//     finish     every block adds its sample's slots in one fixed order (shm_block_sum), takes scale = max(std, 1/256) over the
//                3*ho*wo values (yuv_std_scale, the formula of yuv_scale_kernel) and divides its pixels of x by it.
// The number of blocks per sample is a function of ho*wo alone, and so is the pixel set of every block and thread: a sample's bits
// do not depend on n, on its slot in the batch or on its neighbours, and two calls give the same bits.  Neither the float RGB tensor
// nor the YUV tensor of the path this replaces (2 x shm_resize_bilinear_u8 per sample, then shm_rgb2yuv_std) goes to memory: per
// output pixel 16 tap bytes are read, 4 + 4 bytes written, and x is read and written once more by the finish.
#include "augment_px.h"
#include "yuv.h"

namespace {

static_assert(SHM_AUG_GROUP == 8, "the descriptor table is sized for the header's group");

constexpr int PAIRS_BLOCKS_MAX = 256;           // blocks per sample: one pixel per thread up to 256 x 256, a grid-stride loop above
constexpr float PAIRS_SCALE = 1.0f / 255.0f;    // bytes -> [0,1], the float the loaders hand shm_resize_bilinear_u8

inline int pairs_blocks(size_t npix) { return shm_grid_cap(npix, AU_NT, PAIRS_BLOCKS_MAX); }

struct PairSample {
    const unsigned char* image;                 // [hin,win,3]
    const unsigned char* mask;                  // [hin,win]
    int hin, win;
    float hs, ws, cy, cx;                       // crop extent / output size, crop origin
    int flags;                                  // bit 0 flip_ud, bit 1 flip_lr
};

struct PairArgs {
    PairSample s[SHM_AUG_GROUP];
    float* x;                                   // the two tensors at the group's first sample
    float* y;
    double* part;                               // the group's slots: [sample][block][2]
    float* scale_out;                           // the group's divisors, or null
    size_t stride;                              // floats from one sample's plane to the next
};

__global__ void __launch_bounds__(AU_NT) pairs_resample_kernel(const PairArgs a, int ho, int wo) {
    const PairSample& d = a.s[blockIdx.y];
    const size_t npix = (size_t)ho * wo, off = (size_t)blockIdx.y * a.stride;
    float* const x = a.x + off;
    float* const y = a.y + off;
    double s = 0.0, q = 0.0;
    for (size_t p = (size_t)blockIdx.x * AU_NT + threadIdx.x; p < npix; p += (size_t)gridDim.x * AU_NT) {
        const int ox = (int)(p % wo), oy = (int)(p / wo);              // the mirrors on the read side, as augment_pixel
        const BilinearTaps t = bilinear_taps(d.flags & 2 ? wo - 1 - ox : ox, d.flags & 1 ? ho - 1 - oy : oy, d.hin, d.win, d.win, d.hs, d.ws, d.cy, d.cx);
        y[p] = bilinear_lerp(d.mask[t.tl], d.mask[t.tr], d.mask[t.bl], d.mask[t.br], t.lx, t.ly) * PAIRS_SCALE;
        float c[3];
#pragma unroll
        for (int k = 0; k < 3; ++k)
            c[k] = bilinear_lerp(d.image[t.tl * 3 + k], d.image[t.tr * 3 + k], d.image[t.bl * 3 + k], d.image[t.br * 3 + k], t.lx, t.ly) * PAIRS_SCALE;
        float yy, u, v;
        rgb2yuv(c[0], c[1], c[2], yy, u, v);
        x[p] = yy;
        s += (double)yy + (double)u + (double)v;
        q += (double)yy * yy + (double)u * u + (double)v * v;
    }
    s = shm_block_sum<AU_NT>(s);
    q = shm_block_sum<AU_NT>(q);
    if (threadIdx.x == 0) {
        double* slot = a.part + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * 2;
        slot[0] = s;
        slot[1] = q;
    }
}

__global__ void __launch_bounds__(AU_NT) pairs_finish_kernel(const PairArgs a, int ho, int wo) {
    static_assert(PAIRS_BLOCKS_MAX <= AU_NT, "one slot per thread");
    const size_t npix = (size_t)ho * wo;
    const double* part = a.part + (size_t)blockIdx.y * gridDim.x * 2;
    const bool has = threadIdx.x < gridDim.x;
    const double s = shm_block_sum<AU_NT>(has ? part[2 * threadIdx.x] : 0.0);
    const double q = shm_block_sum<AU_NT>(has ? part[2 * threadIdx.x + 1] : 0.0);
    const float scale = yuv_std_scale(s, q, (double)npix * 3.0);
    if (a.scale_out && blockIdx.x == 0 && threadIdx.x == 0) a.scale_out[blockIdx.y] = scale;
    float* const x = a.x + (size_t)blockIdx.y * a.stride;
    for (size_t p = (size_t)blockIdx.x * AU_NT + threadIdx.x; p < npix; p += (size_t)gridDim.x * AU_NT) x[p] = x[p] / scale;
}

}  // namespace

extern "C" size_t shm_augment_pairs_ws_doubles(int n, int ho, int wo) {
    if (n < 1 || ho < 1 || ho > AU_DIM_MAX || wo < 1 || wo > AU_DIM_MAX) return 0;
    return (size_t)n * pairs_blocks((size_t)ho * wo) * 2;
}

extern "C" int shm_augment_pairs_u8(const shm_pair_sample* samples, int n, float* x, float* y, size_t sample_stride, int ho, int wo, double* ws,
                                    float* scale_out, void* stream) {
    SHM_REQUIRE(n >= 1, SHM_E_SHAPE, "shm_augment_pairs_u8: n %d < 1", n);
    SHM_REQUIRE(samples && x && y && ws, SHM_E_SHAPE, "shm_augment_pairs_u8: null pointer (samples, x, y or ws)");
    SHM_REQUIRE(ho >= 1 && ho <= AU_DIM_MAX && wo >= 1 && wo <= AU_DIM_MAX, SHM_E_SHAPE, "shm_augment_pairs_u8: sizes ho %d, wo %d outside [1, %d]", ho,
                wo, AU_DIM_MAX);
    SHM_REQUIRE(n == 1 || sample_stride >= (size_t)ho * wo, SHM_E_SHAPE, "shm_augment_pairs_u8: sample_stride %zu is less than a plane of %d x %d",
                sample_stride, ho, wo);
    // every sample before the first launch: the rules of shm_augment_batch_u8
    for (int i = 0; i < n; ++i) {
        const shm_pair_sample& s = samples[i];
        SHM_REQUIRE(s.image && s.mask, SHM_E_SHAPE, "shm_augment_pairs_u8: sample %d: null pointer (%s)", i, s.image ? "mask" : "image");
        SHM_REQUIRE(s.hin >= 1 && s.hin <= AU_DIM_MAX && s.win >= 1 && s.win <= AU_DIM_MAX, SHM_E_SHAPE,
                    "shm_augment_pairs_u8: sample %d: sizes hin %d, win %d outside [1, %d]", i, s.hin, s.win, AU_DIM_MAX);
        // written so that a NaN fails them
        SHM_REQUIRE(s.crop_h > 0.f && s.crop_w > 0.f, SHM_E_SHAPE, "shm_augment_pairs_u8: sample %d: empty crop (crop_h %g, crop_w %g)", i,
                    (double)s.crop_h, (double)s.crop_w);
        SHM_REQUIRE(s.crop_y >= 0.f && s.crop_x >= 0.f && (double)s.crop_y + (double)s.crop_h <= (double)s.hin &&
                        (double)s.crop_x + (double)s.crop_w <= (double)s.win,
                    SHM_E_SHAPE, "shm_augment_pairs_u8: sample %d: the crop %g x %g at (%g, %g) does not lie inside the %d x %d image", i,
                    (double)s.crop_h, (double)s.crop_w, (double)s.crop_y, (double)s.crop_x, s.hin, s.win);
    }
    const int nblk = pairs_blocks((size_t)ho * wo);
    PairArgs a;
    a.stride = sample_stride;
    hipStream_t st = (hipStream_t)stream;
    for (int i0 = 0; i0 < n; i0 += SHM_AUG_GROUP) {
        const int m = n - i0 < SHM_AUG_GROUP ? n - i0 : SHM_AUG_GROUP;
        a.x = x + (size_t)i0 * sample_stride;
        a.y = y + (size_t)i0 * sample_stride;
        a.part = ws + (size_t)i0 * nblk * 2;
        a.scale_out = scale_out ? scale_out + i0 : nullptr;
        for (int j = 0; j < SHM_AUG_GROUP; ++j) {
            const shm_pair_sample& s = samples[i0 + (j < m ? j : 0)];       // rows past m are never read: no block has that blockIdx.y
            PairSample& d = a.s[j];
            d.image = s.image;
            d.mask = s.mask;
            d.hin = s.hin;
            d.win = s.win;
            d.hs = s.crop_h / (float)ho;
            d.ws = s.crop_w / (float)wo;
            d.cy = s.crop_y;
            d.cx = s.crop_x;
            d.flags = (s.flip_ud ? 1 : 0) | (s.flip_lr ? 2 : 0);
        }
        const dim3 grid(nblk, m);
        hipLaunchKernelGGL(pairs_resample_kernel, grid, dim3(AU_NT), 0, st, a, ho, wo);
        SHM_LAUNCH_CHECK("shm_augment_pairs_u8(resample)");
        hipLaunchKernelGGL(pairs_finish_kernel, grid, dim3(AU_NT), 0, st, a, ho, wo);
        SHM_LAUNCH_CHECK("shm_augment_pairs_u8(finish)");
    }
    return SHM_OK;
}
