// InstanceNormalization forward: statistics and their finalize pass, the normalisation table, apply, apply + AveragePooling2D, pooling alone.
#include "elem.h"

// ------------------------------------------------------------------------- IN statistics
template <typename T>
__global__ __launch_bounds__(256) void in_stats_kernel(const T* __restrict__ a, int lda, double* __restrict__ stats, int hw, int c, int chunk) {
    PixMap pm(c);
    const int n = blockIdx.y;
    const int p0 = blockIdx.x * chunk, p1 = min(hw, p0 + chunk);
    double v[2][4] = {};
    if (pm.active) {
        const T* base = a + (size_t)n * hw * lda + pm.cl * 4;
        for (int p = p0 + pm.pp; p < p1; p += pm.PP) {
            f32x4 x = ld4(base + (size_t)p * lda);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                v[0][e] += (double)x[e];
                v[1][e] += (double)x[e] * (double)x[e];
            }
        }
    }
    block_reduce_atomic<2>(v, pm, stats + (size_t)n * c * 2, c, true);
}

// part != null: the sums were accumulated over `nslot` slot copies part[slot][total][2]; the copies are zeroed
// again as they are consumed, so the scratch is zero whenever no call is in flight (no memset per launch)
// nt != null: also the float table [batch][4][c] = (mean, inv, beta, ring) of the consumers that normalise on the fly (common.h)
__global__ void in_finalize_kernel(double* __restrict__ stats, double* __restrict__ part, int nslot, int total, int hw, double eps, float* __restrict__ nt,
                                   const float* __restrict__ beta, int c) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    double s, q;
    if (part) {
        s = q = 0.0;
        for (int k = 0; k < nslot; ++k) {
            double* pk = part + ((size_t)k * total + i) * 2;
            s += pk[0];
            q += pk[1];
            pk[0] = 0.0;
            pk[1] = 0.0;
        }
    } else {
        s = stats[2 * i];
        q = stats[2 * i + 1];
    }
    double mean = s / hw;
    double var = q / hw - mean * mean;
    if (var < 0.0) var = 0.0;
    const double inv = 1.0 / sqrt(var + eps);
    stats[2 * i] = mean;
    stats[2 * i + 1] = inv;
    if (nt) {
        const int n = i / c, ch = i - n * c;
        float* t = nt + (size_t)n * SHM_NT_PLANES * c + ch;
        t[0] = (float)mean;
        t[c] = (float)inv;
        t[2 * c] = beta[ch];
        t[3 * c] = (float)mean - beta[ch] / (float)inv;
    }
}

int shm_in_finalize_internal(double* stats, double* part, int nslot, int total, int hw, double eps, float* nt, const float* beta, int c, hipStream_t st) {
    hipLaunchKernelGGL(in_finalize_kernel, dim3(shm_cdiv((long)total, 256)), dim3(256), 0, st, stats, part, nslot, total, hw, eps, nt, beta, c);
    SHM_LAUNCH_CHECK("shm_in_finalize");
    return SHM_OK;
}

// the table alone, from finalized statistics (mean, inv)
__global__ void in_norm_table_kernel(const double* __restrict__ stats, const float* __restrict__ beta, float* __restrict__ nt, int total, int c) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int n = i / c, ch = i - n * c;
    float* t = nt + (size_t)n * SHM_NT_PLANES * c + ch;
    t[0] = (float)stats[2 * i];
    t[c] = (float)stats[2 * i + 1];
    t[2 * c] = beta[ch];
    t[3 * c] = (float)stats[2 * i] - beta[ch] / (float)stats[2 * i + 1];
}

extern "C" int shm_in_norm_table(const double* stats, const float* beta, float* nt, int batch, int c, void* stream) {
    SHM_REQUIRE(stats && beta && nt, SHM_E_SHAPE, "shm_in_norm_table: null pointer");
    SHM_REQUIRE(c % 4 == 0 && c > 0, SHM_E_SHAPE, "shm_in_norm_table: channels %d must be a positive multiple of 4", c);
    if (batch == 0) return SHM_OK;
    hipLaunchKernelGGL(in_norm_table_kernel, dim3(shm_cdiv((long)batch * c, 256)), dim3(256), 0, (hipStream_t)stream, stats, beta, nt, batch * c, c);
    SHM_LAUNCH_CHECK("shm_in_norm_table");
    return SHM_OK;
}

extern "C" int shm_in_stats(const void* a, int lda, double* stats, int batch, int hw, int c, float eps, int dtype, void* stream) {
    SHM_CHECK_C(c, "shm_in_stats");
    SHM_REQUIRE(lda % 4 == 0 && lda >= c, SHM_E_SHAPE, "shm_in_stats: bad pitch %d", lda);
    hipStream_t st = (hipStream_t)stream;
    if (batch == 0 || hw == 0) return SHM_OK;
    int r = shm_zero(stats, (size_t)batch * c * 2 * sizeof(double), stream);
    if (r) return r;
    int nch = pix_chunks(hw, batch, c, 4096);
    int chunk = shm_cdiv(hw, nch);
    SHM_DISPATCH(dtype, "shm_in_stats",
                 hipLaunchKernelGGL(in_stats_kernel<T>, dim3(shm_cdiv(hw, chunk), batch), dim3(256), 0, st, (const T*)a, lda, stats, hw, c, chunk));
    SHM_LAUNCH_CHECK("shm_in_stats");
    hipLaunchKernelGGL(in_finalize_kernel, dim3(shm_cdiv((long)batch * c, 256)), dim3(256), 0, st, stats, (double*)nullptr, 0, batch * c, hw, (double)eps,
                       (float*)nullptr, (const float*)nullptr, c);
    SHM_LAUNCH_CHECK("shm_in_stats(finalize)");
    return SHM_OK;
}

// rev: walk the tensor back to front.  The producing convolution wrote the samples in ascending order, so the LAST ones are
// still in the 256 MiB Infinity Cache: reading them first turns up to 256 MiB of this pass's reads into cache hits (front to
// back, an LRU cache smaller than the tensor yields none), and it leaves sample 0 written last -- where the
// consuming convolution starts.
template <typename T>
__global__ __launch_bounds__(256) void in_apply_kernel(const T* __restrict__ a, int lda, const double* __restrict__ stats, const float* __restrict__ beta,
                                                       T* __restrict__ out, int ldo, int hw, int c, int chunk, int rev) {
    PixMap pm(c);
    if (!pm.active) return;
    const int n = rev ? gridDim.y - 1 - blockIdx.y : blockIdx.y;
    const int bx = rev ? gridDim.x - 1 - blockIdx.x : blockIdx.x;
    const int p0 = bx * chunk, p1 = min(hw, p0 + chunk);
    float mean[4], inv[4], bt[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        int ch = pm.cl * 4 + e;
        mean[e] = (float)stats[((size_t)n * c + ch) * 2];
        inv[e] = (float)stats[((size_t)n * c + ch) * 2 + 1];
        bt[e] = beta[ch];
    }
    const T* base = a + (size_t)n * hw * lda + pm.cl * 4;
    T* ob = out + (size_t)n * hw * ldo + pm.cl * 4;
    constexpr int U = sizeof(T) == 2 ? 8 : 4;
    int p = p0 + pm.pp;
    for (; p + (U - 1) * pm.PP < p1; p += U * pm.PP) {
        f32x4 x[U];
#pragma unroll
        for (int u = 0; u < U; ++u) x[u] = ld4(base + (size_t)(p + u * pm.PP) * lda);
#pragma unroll
        for (int u = 0; u < U; ++u) {
            f32x4 y;
#pragma unroll
            for (int e = 0; e < 4; ++e) y[e] = shm_in_norm(x[u][e], mean[e], inv[e], bt[e]);
            st4(ob + (size_t)(p + u * pm.PP) * ldo, y);
        }
    }
    for (; p < p1; p += pm.PP) {
        f32x4 x = ld4(base + (size_t)p * lda);
        f32x4 y;
#pragma unroll
        for (int e = 0; e < 4; ++e) y[e] = shm_in_norm(x[e], mean[e], inv[e], bt[e]);
        st4(ob + (size_t)p * ldo, y);
    }
}

extern "C" int shm_in_apply(const void* a, int lda, const double* stats, const float* beta, void* out, int ldo, int batch, int hw, int c, int dtype,
                            void* stream) {
    SHM_CHECK_C(c, "shm_in_apply");
    SHM_REQUIRE(lda % 4 == 0 && ldo % 4 == 0 && lda >= c && ldo >= c, SHM_E_SHAPE, "shm_in_apply: bad pitch %d / %d (multiples of 4, at least %d channels)", lda, ldo, c);
    if (batch == 0 || hw == 0) return SHM_OK;
    int nch = pix_chunks(hw, batch, c);
    int chunk = shm_cdiv(hw, nch);
    SHM_DISPATCH(dtype, "shm_in_apply",
                 hipLaunchKernelGGL(in_apply_kernel<T>, dim3(shm_cdiv(hw, chunk), batch), dim3(256), 0, (hipStream_t)stream, (const T*)a, lda, stats, beta,
                                    (T*)out, ldo, hw, c, chunk, shm_tune(SHM_TUNE_ELEM_REVERSE)));
    SHM_LAUNCH_CHECK("shm_in_apply");
    return SHM_OK;
}

// InstanceNorm apply + AveragePooling2D(2) in one pass (the second block of every encoder level feeds both the skip and the
// pool): a thread normalises the four pixels of a 2 x 2 quad for its four channels, writes them, and writes their mean -- the
// pooled tensor is formed from the values as stored (rounded to T), in avgpool2_kernel's order, so it is bit-identical to
// shm_in_apply followed by shm_avgpool2_fwd; the separate pooling pass (a full read of the normalised tensor) is gone.
// OUT = false (shm_in_pool): only the pooled tensor is written -- the skip connection's consumers normalise the stored activation
// on the fly (shm_conv2d_in_fwd_norm / shm_conv2d_wgrad_norm); the pooled values are the same bits as with OUT = true.
template <typename T, bool OUT = true>
__global__ __launch_bounds__(256) void in_apply_pool_kernel(const T* __restrict__ a, int lda, const double* __restrict__ stats, const float* __restrict__ beta,
                                                            T* __restrict__ out, int ldo, T* __restrict__ pooled, int ldp, int h, int w, int c, int chunk,
                                                            int rev) {
    PixMap pm(c);
    if (!pm.active) return;
    const int n = rev ? gridDim.y - 1 - blockIdx.y : blockIdx.y;
    const int bx = rev ? gridDim.x - 1 - blockIdx.x : blockIdx.x;
    const int wo = w >> 1, hq = (h >> 1) * wo;
    const int q0 = bx * chunk, q1 = min(hq, q0 + chunk);
    float mean[4], inv[4], bt[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        int ch = pm.cl * 4 + e;
        mean[e] = (float)stats[((size_t)n * c + ch) * 2];
        inv[e] = (float)stats[((size_t)n * c + ch) * 2 + 1];
        bt[e] = beta[ch];
    }
    const T* base = a + (size_t)n * h * w * lda + pm.cl * 4;
    T* ob = out + (size_t)n * h * w * ldo + pm.cl * 4;
    T* pb = pooled + (size_t)n * hq * ldp + pm.cl * 4;
    constexpr int U = 2;
    auto quad = [&](int q, f32x4 (&x)[4]) {
        const int oy = q / wo, ox = q - oy * wo;
        const size_t p = (size_t)(2 * oy) * w + 2 * ox;
        x[0] = ld4(base + p * lda);
        x[1] = ld4(base + (p + 1) * lda);
        x[2] = ld4(base + (p + w) * lda);
        x[3] = ld4(base + (p + w + 1) * lda);
    };
    auto finish = [&](int q, const f32x4 (&x)[4]) {
        const int oy = q / wo, ox = q - oy * wo;
        const size_t p = (size_t)(2 * oy) * w + 2 * ox;
        f32x4 y[4], s;
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int e = 0; e < 4; ++e) y[t][e] = rnd_as((const T*)nullptr, shm_in_norm(x[t][e], mean[e], inv[e], bt[e]));
        if constexpr (OUT) {
            st4(ob + p * ldo, y[0]);
            st4(ob + (p + 1) * ldo, y[1]);
            st4(ob + (p + w) * ldo, y[2]);
            st4(ob + (p + w + 1) * ldo, y[3]);
        }
        s = ((y[0] + y[1]) + y[2]) + y[3];
        st4(pb + (size_t)q * ldp, s * 0.25f);
    };
    int q = q0 + pm.pp;
    for (; q + (U - 1) * pm.PP < q1; q += U * pm.PP) {
        f32x4 x[U][4];
#pragma unroll
        for (int u = 0; u < U; ++u) quad(q + u * pm.PP, x[u]);
#pragma unroll
        for (int u = 0; u < U; ++u) finish(q + u * pm.PP, x[u]);
    }
    for (; q < q1; q += pm.PP) {
        f32x4 x[4];
        quad(q, x);
        finish(q, x);
    }
}

extern "C" int shm_in_apply_pool(const void* a, int lda, const double* stats, const float* beta, void* out, int ldo, void* pooled, int ldp, int batch,
                                 int h, int w, int c, int dtype, void* stream) {
    SHM_CHECK_C(c, "shm_in_apply_pool");
    SHM_REQUIRE(lda % 4 == 0 && ldo % 4 == 0 && ldp % 4 == 0 && lda >= c && ldo >= c && ldp >= c, SHM_E_SHAPE,
                "shm_in_apply_pool: bad pitch %d / %d / %d (multiples of 4, at least %d channels)", lda, ldo, ldp, c);
    SHM_REQUIRE(h % 2 == 0 && w % 2 == 0, SHM_E_SHAPE, "shm_in_apply_pool: odd size %dx%d", h, w);
    SHM_REQUIRE(a && stats && beta && out && pooled, SHM_E_SHAPE, "shm_in_apply_pool: null pointer");
    if (batch == 0 || h * w == 0) return SHM_OK;
    const int hq = (h / 2) * (w / 2);
    int nch = pix_chunks(hq, batch, c);
    int chunk = shm_cdiv(hq, nch);
    SHM_DISPATCH(dtype, "shm_in_apply_pool",
                 hipLaunchKernelGGL((in_apply_pool_kernel<T, true>), dim3(shm_cdiv(hq, chunk), batch), dim3(256), 0, (hipStream_t)stream, (const T*)a, lda, stats, beta,
                                    (T*)out, ldo, (T*)pooled, ldp, h, w, c, chunk, shm_tune(SHM_TUNE_ELEM_REVERSE)));
    SHM_LAUNCH_CHECK("shm_in_apply_pool");
    return SHM_OK;
}

extern "C" int shm_in_pool(const void* a, int lda, const double* stats, const float* beta, void* pooled, int ldp, int batch, int h, int w, int c, int dtype,
                           void* stream) {
    SHM_CHECK_C(c, "shm_in_pool");
    SHM_REQUIRE(lda % 4 == 0 && ldp % 4 == 0 && lda >= c && ldp >= c, SHM_E_SHAPE, "shm_in_pool: bad pitch %d / %d (multiples of 4, at least %d channels)", lda, ldp, c);
    SHM_REQUIRE(h % 2 == 0 && w % 2 == 0, SHM_E_SHAPE, "shm_in_pool: odd size %dx%d", h, w);
    SHM_REQUIRE(a && stats && beta && pooled, SHM_E_SHAPE, "shm_in_pool: null pointer");
    if (batch == 0 || h * w == 0) return SHM_OK;
    const int hq = (h / 2) * (w / 2);
    int nch = pix_chunks(hq, batch, c);
    int chunk = shm_cdiv(hq, nch);
    SHM_DISPATCH(dtype, "shm_in_pool",
                 hipLaunchKernelGGL((in_apply_pool_kernel<T, false>), dim3(shm_cdiv(hq, chunk), batch), dim3(256), 0, (hipStream_t)stream, (const T*)a, lda, stats,
                                    beta, (T*)nullptr, 0, (T*)pooled, ldp, h, w, c, chunk, shm_tune(SHM_TUNE_ELEM_REVERSE)));
    SHM_LAUNCH_CHECK("shm_in_pool");
    return SHM_OK;
}
