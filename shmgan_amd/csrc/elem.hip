// Small elementwise passes: memset and casts, average pooling, dropout mask, the attention branch's mask helpers.
#include "elem.h"

extern "C" int shm_zero(void* p, size_t bytes, void* stream) {
    if (bytes == 0) return SHM_OK;
    hipError_t e = hipMemsetAsync(p, 0, bytes, (hipStream_t)stream);
    SHM_REQUIRE(e == hipSuccess, SHM_E_HIP, "shm_zero: %s", hipGetErrorString(e));
    return SHM_OK;
}

__global__ void cvt_f64_f32_kernel(const double* __restrict__ s, float* __restrict__ d, size_t n, int acc) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) d[i] = acc ? d[i] + (float)s[i] : (float)s[i];          // not 0.f + v: that would turn v = -0.0 into +0.0
}

extern "C" int shm_cvt_f64_f32(const double* src, float* dst, size_t n, int accumulate, void* stream) {
    if (n == 0) return SHM_OK;
    hipLaunchKernelGGL(cvt_f64_f32_kernel, dim3(shm_cdiv((long)n, 256)), dim3(256), 0, (hipStream_t)stream, src, dst, n, accumulate);
    SHM_LAUNCH_CHECK("shm_cvt_f64_f32");
    return SHM_OK;
}

// f32 -> activation dtype copy (bf16 operand copies of the fp32 master weights)
template <typename T>
__global__ void cast_f32_kernel(const float* __restrict__ s, T* __restrict__ d, size_t n) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) d[i] = (T)s[i];
}

extern "C" int shm_cast_f32(const float* src, void* dst, size_t n, int dtype, void* stream) {
    if (n == 0) return SHM_OK;
    SHM_DISPATCH(dtype, "shm_cast_f32", hipLaunchKernelGGL(cast_f32_kernel<T>, dim3(shm_grid_cap(n, 256, 4096)), dim3(256), 0, (hipStream_t)stream, src, (T*)dst, n));
    SHM_LAUNCH_CHECK("shm_cast_f32");
    return SHM_OK;
}

// -------------------------------------------------------------------------------- pooling
template <typename T>
__global__ void avgpool2_kernel(const T* __restrict__ x, int ldx, T* __restrict__ y, int ldy, int h, int w, int c4, size_t total) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    int cl = (int)(i % c4);
    size_t q = i / c4;                     // output pixel (n, oy, ox)
    int wo = w >> 1, ho = h >> 1;
    int ox = (int)(q % wo);
    size_t t = q / wo;
    int oy = (int)(t % ho);
    size_t n = t / ho;
    const T* b = x + ((n * h + 2 * oy) * w + 2 * ox) * ldx + cl * 4;
    f32x4 s = ld4(b) + ld4(b + ldx) + ld4(b + (size_t)w * ldx) + ld4(b + (size_t)(w + 1) * ldx);
    st4(y + q * ldy + cl * 4, s * 0.25f);
}

extern "C" int shm_avgpool2_fwd(const void* x, int ldx, void* y, int ldy, int batch, int h, int w, int c, int dtype, void* stream) {
    SHM_REQUIRE(c % 4 == 0 && ldx % 4 == 0 && ldy % 4 == 0, SHM_E_SHAPE, "shm_avgpool2_fwd: channels/pitch must be multiples of 4");
    SHM_REQUIRE(ldx >= c && ldy >= c, SHM_E_SHAPE, "shm_avgpool2_fwd: pitch %d / %d below the %d channels", ldx, ldy, c);
    SHM_REQUIRE(h % 2 == 0 && w % 2 == 0, SHM_E_SHAPE, "shm_avgpool2_fwd: odd size %dx%d", h, w);
    size_t total = (size_t)batch * (h / 2) * (w / 2) * (c / 4);
    if (total == 0) return SHM_OK;
    SHM_DISPATCH(dtype, "shm_avgpool2_fwd",
                 hipLaunchKernelGGL(avgpool2_kernel<T>, dim3(shm_cdiv((long)total, 256)), dim3(256), 0, (hipStream_t)stream, (const T*)x, ldx, (T*)y, ldy, h, w,
                                    c / 4, total));
    SHM_LAUNCH_CHECK("shm_avgpool2_fwd");
    return SHM_OK;
}

// --------------------------------------------------------------------------- dropout mask
template <typename T>
__global__ void mul_mask_kernel(const T* __restrict__ x, const float* __restrict__ m, T* __restrict__ y, size_t n4, float scale) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n4) return;
    f32x4 a = ld4(x + i * 4), b = ((const f32x4*)m)[i];
    st4(y + i * 4, a * b * scale);
}

extern "C" int shm_mul_mask(const void* x, const float* mask, void* y, size_t n, float scale, int dtype, void* stream) {
    SHM_REQUIRE(n % 4 == 0, SHM_E_SHAPE, "shm_mul_mask: n must be a multiple of 4");
    if (n == 0) return SHM_OK;
    SHM_DISPATCH(dtype, "shm_mul_mask",
                 hipLaunchKernelGGL(mul_mask_kernel<T>, dim3(shm_cdiv((long)(n / 4), 256)), dim3(256), 0, (hipStream_t)stream, (const T*)x, mask, (T*)y, n / 4, scale));
    SHM_LAUNCH_CHECK("shm_mul_mask");
    return SHM_OK;
}

// ------------------------------------------------------ live attention branch (SHM.py:404-412, 290-293, 359)
// MaxPooling2D(pool k x k, 'same' on sizes that are multiples of k) of the one-channel mask, written as channel 0 of an
// activation tensor of pitch ld (the other channels zero): the 1 -> C convolution of attention_layer then runs on the
// ordinary tap GEMM.  k = 1 copies (attention_layer(pool=False)).  The mask is [batch,h,w,1]: the square call has h = w = s.
template <typename T>
__global__ void mask_pool_pack_kernel(const float* __restrict__ m, T* __restrict__ dst, int ld, int h, int w, int k, size_t total) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;          // output pixel (b, y, x)
    if (i >= total) return;
    const int ho = h / k, wo = w / k;
    const int x = (int)(i % wo), y = (int)((i / wo) % ho);
    const size_t b = i / ((size_t)ho * wo);
    const float* src = m + (b * h + (size_t)y * k) * w + (size_t)x * k;
    float v = src[0];
    for (int dy = 0; dy < k; ++dy)
        for (int dx = 0; dx < k; ++dx) v = fmaxf(v, src[(size_t)dy * w + dx]);
    T* o = dst + i * ld;
    o[0] = (T)v;
    for (int c = 1; c < ld; ++c) o[c] = (T)0.f;
}

// both entry points behind their own checks: nothing to do for an empty output, else one launch
static int mask_pool_pack(const char* who, const float* mask, void* dst, int lddst, int batch, int h, int w, int k, int dtype, void* stream) {
    const size_t total = (size_t)batch * (h / k) * (w / k);
    if (total == 0) return SHM_OK;
    SHM_DISPATCH(dtype, who,
                 hipLaunchKernelGGL(mask_pool_pack_kernel<T>, dim3(shm_cdiv((long)total, 256)), dim3(256), 0, (hipStream_t)stream, mask, (T*)dst, lddst, h, w, k, total));
    SHM_LAUNCH_CHECK(who);
    return SHM_OK;
}

// the square form takes s == 0 (an empty output) and does not look at batch's sign; the _hw form refuses h < 1 and batch < 0
extern "C" int shm_mask_pool_pack(const float* mask, void* dst, int lddst, int batch, int s, int k, int dtype, void* stream) {
    SHM_REQUIRE(mask && dst && k >= 1 && s % k == 0 && lddst >= 1, SHM_E_SHAPE, "shm_mask_pool_pack: bad shape (s %d, k %d)", s, k);
    return mask_pool_pack("shm_mask_pool_pack", mask, dst, lddst, batch, s, s, k, dtype, stream);
}

extern "C" int shm_mask_pool_pack_hw(const float* mask, void* dst, int lddst, int batch, int h, int w, int k, int dtype, void* stream) {
    SHM_REQUIRE(mask && dst && k >= 1 && h >= 1 && w >= 1 && h % k == 0 && w % k == 0 && lddst >= 1 && batch >= 0, SHM_E_SHAPE,
                "shm_mask_pool_pack_hw: bad shape (h %d, w %d, k %d)", h, w, k);
    return mask_pool_pack("shm_mask_pool_pack_hw", mask, dst, lddst, batch, h, w, k, dtype, stream);
}

// out[i] = a[i] + b[(i0 + i) % nb]  over images of `per` elements each: the skip tensor plus the attention map of its sample
// (`down_k + attn_k`, SHM.py:290-293; `x + attn_disc`, SHM.py:359), the attention map shared by every copy of a sample in the
// batched plan (image i of the batch belongs to sample (i0 + i) % nb).
template <typename T>
__global__ void add_bcast_kernel(const T* __restrict__ a, const T* __restrict__ b, T* __restrict__ out, size_t per4, int nb, int i0, size_t total4) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total4) return;
    const size_t img = i / per4, r = i - img * per4;
    const size_t j = ((size_t)i0 + img) % (size_t)nb;
    st4(out + i * 4, ld4(a + i * 4) + ld4(b + (j * per4 + r) * 4));
}

extern "C" int shm_add_bcast(const void* a, const void* b, void* out, int nimg, size_t per, int nb, int i0, int dtype, void* stream) {
    SHM_REQUIRE(a && b && out && per % 4 == 0 && nb >= 1 && i0 >= 0, SHM_E_SHAPE, "shm_add_bcast: bad arguments");
    const size_t total4 = (size_t)nimg * per / 4;
    if (total4 == 0) return SHM_OK;
    SHM_DISPATCH(dtype, "shm_add_bcast",
                 hipLaunchKernelGGL(add_bcast_kernel<T>, dim3(shm_cdiv((long)total4, 256)), dim3(256), 0, (hipStream_t)stream, (const T*)a, (const T*)b, (T*)out,
                                    per / 4, nb, i0, total4));
    SHM_LAUNCH_CHECK("shm_add_bcast");
    return SHM_OK;
}

// dst[j] (+)= sum over the images i of src with (i0 + i) % nb == j: the gradient of the broadcast above (fp32 accumulation).
template <typename T>
__global__ void sum_groups_kernel(const T* __restrict__ src, T* __restrict__ dst, size_t per4, int nimg, int nb, int i0, int accumulate, size_t total4) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;          // (sample j, element r)
    if (i >= total4) return;
    const size_t j = i / per4, r = i - j * per4;
    f32x4 s = accumulate ? ld4(dst + i * 4) : f32x4{0.f, 0.f, 0.f, 0.f};
    int first = (int)((j + (size_t)nb - (size_t)(i0 % nb)) % (size_t)nb);
    for (int img = first; img < nimg; img += nb) s += ld4(src + ((size_t)img * per4 + r) * 4);
    st4(dst + i * 4, s);
}

extern "C" int shm_sum_groups(const void* src, void* dst, int nimg, size_t per, int nb, int i0, int accumulate, int dtype, void* stream) {
    SHM_REQUIRE(src && dst && per % 4 == 0 && nb >= 1 && i0 >= 0, SHM_E_SHAPE, "shm_sum_groups: bad arguments");
    const size_t total4 = (size_t)nb * per / 4;
    if (total4 == 0) return SHM_OK;
    SHM_DISPATCH(dtype, "shm_sum_groups",
                 hipLaunchKernelGGL(sum_groups_kernel<T>, dim3(shm_cdiv((long)total4, 256)), dim3(256), 0, (hipStream_t)stream, (const T*)src, (T*)dst, per / 4, nimg,
                                    nb, i0, accumulate, total4));
    SHM_LAUNCH_CHECK("shm_sum_groups");
    return SHM_OK;
}
