// Input pipeline step of datasetLoader.py:47-60 on the device: tf.image.resize (the sampler of bilinear.h) of a decoded
// uint8 RGB image to image_size x image_size, x / 255, tf.image.flip_up_down.
// The decoded file is uploaded as bytes (3 B/pixel instead of 12) and everything after the decode is one kernel.
#include "bilinear.h"

__global__ void resize_bilinear_u8_kernel(const unsigned char* __restrict__ src, int hin, int win, int c, float* __restrict__ dst, int ho, int wo,
                                          float hs, float ws, float scale, int flip_ud) {
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;       // (oy, ox)
    if (idx >= (size_t)ho * wo) return;
    const int ox = (int)(idx % wo), oy = (int)(idx / wo);
    const BilinearTaps t = bilinear_taps(ox, flip_ud ? ho - 1 - oy : oy, hin, win, win, hs, ws, 0.f, 0.f);      // the flip on the read side
    float* o = dst + idx * c;
    for (int k = 0; k < c; ++k)
        o[k] = bilinear_lerp(src[t.tl * c + k], src[t.tr * c + k], src[t.bl * c + k], src[t.br * c + k], t.lx, t.ly) * scale;
}

extern "C" int shm_resize_bilinear_u8(const unsigned char* src, int hin, int win, int c, float* dst, int ho, int wo, float scale, int flip_ud,
                                      void* stream) {
    SHM_REQUIRE(src && dst && hin > 0 && win > 0 && ho > 0 && wo > 0 && c > 0, SHM_E_SHAPE, "shm_resize_bilinear_u8: bad arguments");
    const size_t n = (size_t)ho * wo;
    hipLaunchKernelGGL(resize_bilinear_u8_kernel, dim3(shm_cdiv((long)n, 256)), dim3(256), 0, (hipStream_t)stream, src, hin, win, c, dst, ho, wo,
                       (float)hin / (float)ho, (float)win / (float)wo, scale, flip_ud);
    SHM_LAUNCH_CHECK("shm_resize_bilinear_u8");
    return SHM_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// Native-resolution test mode: a decoded uint8 image [h,w,c] into the float32 frame [hp,wp,c] the networks run on, the photo
// at (top, left) and the border filled by reflection without repeating the edge sample (NumPy's mode="reflect"):
// dst[y][x] = float(src[ry][rx]) * scale, ry = reflect(y - top, h), rx = reflect(x - left, w).  One thread per four consecutive
// floats of the frame (one 16-byte store when dst is 16-byte aligned and hp*wp*c % 4 == 0, four scalar stores otherwise: the
// values are the same), grid-stride free: the grid covers the frame once.
__device__ __forceinline__ int reflect_index(int i, int n) {
    i = i < 0 ? -i : i;
    return i >= n ? 2 * (n - 1) - i : i;
}

template <bool VEC>
__global__ void __launch_bounds__(256) load_pad_u8_kernel(const unsigned char* __restrict__ src, int h, int w, int c, float* __restrict__ dst,
                                                          int wp, int top, int left, float scale, size_t total) {
    const size_t e0 = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) * 4;
    if (e0 >= total) return;
    const size_t p = e0 / c;
    int ch = (int)(e0 - p * c);
    int y = (int)(p / wp), x = (int)(p - (size_t)y * wp);
    const int nq = total - e0 < 4 ? (int)(total - e0) : 4;
    float v[4] = {0.f, 0.f, 0.f, 0.f};
    const unsigned char* row = src + (size_t)reflect_index(y - top, h) * w * c;
    for (int q = 0; q < nq; ++q) {
        v[q] = (float)row[(size_t)reflect_index(x - left, w) * c + ch] * scale;
        if (++ch == c) {
            ch = 0;
            if (++x == wp && q + 1 < nq) {                                  // another element follows: y + 1 < hp
                x = 0;
                ++y;
                row = src + (size_t)reflect_index(y - top, h) * w * c;
            }
        }
    }
    if (VEC) {
        *reinterpret_cast<float4*>(dst + e0) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
        for (int q = 0; q < nq; ++q) dst[e0 + q] = v[q];
    }
}

extern "C" int shm_load_pad_u8(const unsigned char* src, int h, int w, int c, float* dst, int hp, int wp, int top, int left, float scale,
                               void* stream) {
    SHM_REQUIRE(src && dst, SHM_E_SHAPE, "shm_load_pad_u8: null pointer");
    SHM_REQUIRE(h >= 1 && w >= 1 && c >= 1 && h <= 32768 && w <= 32768 && hp <= 32768 && wp <= 32768 && c <= 16, SHM_E_SHAPE,
                "shm_load_pad_u8: sizes h %d, w %d, c %d, hp %d, wp %d outside [1, 32768] (c: [1, 16])", h, w, c, hp, wp);
    SHM_REQUIRE(top >= 0 && left >= 0 && hp >= top + h && wp >= left + w, SHM_E_SHAPE,
                "shm_load_pad_u8: the %d x %d image at (%d, %d) does not lie inside the %d x %d frame", h, w, top, left, hp, wp);
    // a reflection without the edge sample reaches at most n - 1 samples past either edge
    SHM_REQUIRE(top <= h - 1 && hp - top - h <= h - 1 && left <= w - 1 && wp - left - w <= w - 1, SHM_E_SHAPE,
                "shm_load_pad_u8: a pad wider than the image less one (%d x %d image, %d x %d frame, origin (%d, %d))", h, w, hp, wp, top, left);
    const size_t total = (size_t)hp * wp * c;
    const bool vec = ((uintptr_t)dst & 15) == 0 && total % 4 == 0;
    const dim3 grid(shm_cdiv((long)((total + 3) / 4), 256));
    if (vec)
        hipLaunchKernelGGL(load_pad_u8_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, src, h, w, c, dst, wp, top, left, scale, total);
    else
        hipLaunchKernelGGL(load_pad_u8_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, src, h, w, c, dst, wp, top, left, scale, total);
    SHM_LAUNCH_CHECK("shm_load_pad_u8");
    return SHM_OK;
}
