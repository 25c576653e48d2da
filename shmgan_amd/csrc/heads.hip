// The 1-output-channel layers: generator head (plain and with the last block's InstanceNorm folded in), PatchGAN logits, Dense(5).
#include "elem.h"

// -------------------------------------------------------------------------- generator head
// y[p] = lrelu(sum_c x[p][c] w[c] + b); C/4 lanes per pixel (power of two <= 64).
// NORM: x is the UN-normalised activation of the last decoder block and the kernel applies its InstanceNorm on the fly
// (xh = (x - mean) * inv + beta, the expression of in_apply_kernel: identical fp32 values) -- the apply pass of that block and
// the normalised tensor do not exist.  grid.y = sample, npix = pixels per sample.
template <typename T, bool NORM>
__global__ __launch_bounds__(256) void head_fwd_kernel(const T* __restrict__ x, int ldx, const float* __restrict__ w, const float* __restrict__ bias,
                                                       float* __restrict__ y, size_t npix, int c, float slope, const double* __restrict__ stats,
                                                       const float* __restrict__ beta) {
    const int lanes_c = c >> 2, PP = 256 / lanes_c;
    const int pp = threadIdx.x / lanes_c, cl = threadIdx.x % lanes_c;
    f32x4 wv = *(const f32x4*)(w + cl * 4);
    const float b = bias ? bias[0] : 0.f;
    float mean[4] = {0.f, 0.f, 0.f, 0.f}, inv[4] = {1.f, 1.f, 1.f, 1.f}, bt[4] = {0.f, 0.f, 0.f, 0.f};
    if constexpr (NORM) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int ch = cl * 4 + e;
            mean[e] = (float)stats[((size_t)blockIdx.y * c + ch) * 2];
            inv[e] = (float)stats[((size_t)blockIdx.y * c + ch) * 2 + 1];
            bt[e] = beta[ch];
        }
        x += (size_t)blockIdx.y * npix * ldx;
        y += (size_t)blockIdx.y * npix;
    }
    for (size_t p = (size_t)blockIdx.x * PP + pp; p < npix; p += (size_t)gridDim.x * PP) {
        f32x4 xv = ld4(x + p * ldx + cl * 4);
        if constexpr (NORM) {
#pragma unroll
            for (int e = 0; e < 4; ++e) xv[e] = (xv[e] - mean[e]) * inv[e] + bt[e];
        }
        float s = xv[0] * wv[0] + xv[1] * wv[1] + xv[2] * wv[2] + xv[3] * wv[3];
        for (int o = lanes_c >> 1; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
        if (cl == 0) y[p] = shm_lrelu(s + b, slope);
    }
}

extern "C" int shm_head_fwd(const void* x, int ldx, const float* w, const float* bias, float* y, size_t npix, int c, float slope, int dtype, void* stream) {
    SHM_REQUIRE(c % 4 == 0 && pow2_le64(c / 4) && ldx % 4 == 0, SHM_E_SHAPE, "shm_head_fwd: channels %d unsupported", c);
    if (npix == 0) return SHM_OK;
    const int blocks = shm_grid_cap(npix, 256 / (c / 4), 8192);
    SHM_DISPATCH(dtype, "shm_head_fwd",
                 hipLaunchKernelGGL((head_fwd_kernel<T, false>), dim3(blocks), dim3(256), 0, (hipStream_t)stream, (const T*)x, ldx, w, bias, y, npix, c, slope,
                                    (const double*)nullptr, (const float*)nullptr));
    SHM_LAUNCH_CHECK("shm_head_fwd");
    return SHM_OK;
}

template <typename T, typename TG, bool NORM>
__global__ __launch_bounds__(256) void head_bwd_kernel(const T* __restrict__ x, int ldx, const float* __restrict__ w, const float* __restrict__ y, const float* __restrict__ dy,
                                                       TG* __restrict__ dx, int lddx, double* dpart, size_t npix, int c, float slope,
                                                       const double* __restrict__ stats, const float* __restrict__ beta, float* __restrict__ dz_out) {
    PixMap pm(c);
    f32x4 wv = *(const f32x4*)(w + pm.cl * 4);
    // NORM (see head_fwd_kernel): x un-normalised, grid.y = sample, npix = pixels per sample; dx is the gradient at the NORMALISED
    // activation (what shm_in_bwd takes), the weight gradient uses the normalised value
    float mean[4] = {0.f, 0.f, 0.f, 0.f}, inv[4] = {1.f, 1.f, 1.f, 1.f}, bt[4] = {0.f, 0.f, 0.f, 0.f};
    if constexpr (NORM) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int ch = pm.cl * 4 + e;
            mean[e] = (float)stats[((size_t)blockIdx.y * c + ch) * 2];
            inv[e] = (float)stats[((size_t)blockIdx.y * c + ch) * 2 + 1];
            bt[e] = beta[ch];
        }
        x += (size_t)blockIdx.y * npix * ldx;
        y += (size_t)blockIdx.y * npix;
        dy += (size_t)blockIdx.y * npix;
        if (dx) dx += (size_t)blockIdx.y * npix * lddx;
        if (dz_out) dz_out += (size_t)blockIdx.y * npix;
    }
    auto norm = [&](f32x4 v) {
        if constexpr (NORM) {
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = (v[e] - mean[e]) * inv[e] + bt[e];
        }
        return v;
    };
    double v[1][4] = {};
    double dbs = 0.0;
    constexpr int U = 4;                   // pixels in flight per thread; partial sums in fp32, accumulated in f64
    const size_t stride = (size_t)gridDim.x * pm.PP;
    size_t p = (size_t)blockIdx.x * pm.PP + pm.pp;
    for (; p + (U - 1) * stride < npix; p += U * stride) {
        float dz[U];
        f32x4 xv[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const size_t q = p + u * stride;
            const float g = dy[q];
            dz[u] = y[q] > 0.f ? g : g * slope;
            xv[u] = norm(ld4(x + q * ldx + pm.cl * 4));
        }
        float sw[4] = {0.f, 0.f, 0.f, 0.f}, sb = 0.f;
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (dx) st4(dx + (p + u * stride) * lddx + pm.cl * 4, wv * dz[u]);
            if (dz_out && pm.cl == 0) dz_out[p + u * stride] = dz[u];
#pragma unroll
            for (int e = 0; e < 4; ++e) sw[e] += xv[u][e] * dz[u];
            sb += dz[u];
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) v[0][e] += (double)sw[e];
        if (pm.cl == 0) dbs += (double)sb;
    }
    for (; p < npix; p += stride) {
        const float g = dy[p];
        const float dz = y[p] > 0.f ? g : g * slope;
        const f32x4 xv = norm(ld4(x + p * ldx + pm.cl * 4));
        if (dx) st4(dx + p * lddx + pm.cl * 4, wv * dz);
        if (dz_out && pm.cl == 0) dz_out[p] = dz;
#pragma unroll
        for (int e = 0; e < 4; ++e) v[0][e] += (double)xv[e] * (double)dz;
        if (pm.cl == 0) dbs += (double)dz;
    }
    // staged per slot (slot = block % SHM_LRELU_RED_SLOTS): [slot][c] weight-gradient sums, then [slot] bias sums
    const int slot = (int)((blockIdx.x + blockIdx.y) % SHM_LRELU_RED_SLOTS);
    double* slotw = dpart + (size_t)slot * c;
    block_reduce_atomic<1>(v, pm, slotw, c, true);
    dbs = shm_wave_sum(dbs);
    if ((threadIdx.x & 63) == 0 && dbs != 0.0) atomicAdd(dpart + (size_t)SHM_LRELU_RED_SLOTS * c + slot, dbs);
}

__global__ void head_fold_kernel(const double* __restrict__ dpart, double* __restrict__ dw_acc, double* __restrict__ db_acc, int c) {
    const int ch = blockIdx.x * blockDim.x + threadIdx.x;
    if (ch > c) return;
    double s = 0.0;
    if (ch < c) {
        for (int i = 0; i < SHM_LRELU_RED_SLOTS; ++i) s += dpart[(size_t)i * c + ch];
        dw_acc[ch] += s;
    } else {
        for (int i = 0; i < SHM_LRELU_RED_SLOTS; ++i) s += dpart[(size_t)SHM_LRELU_RED_SLOTS * c + i];
        db_acc[0] += s;
    }
}

extern "C" int shm_head_bwd(const void* x, int ldx, const float* w, const float* y, const float* dy, void* dx,
                            int lddx, double* dw_acc, double* db_acc, double* red, size_t npix, int c, float slope, int dtype, void* stream) {
    SHM_REQUIRE(c % 4 == 0 && pow2_le64(c / 4) && ldx % 4 == 0 && lddx % 4 == 0, SHM_E_SHAPE, "shm_head_bwd: channels %d unsupported", c);
    SHM_REQUIRE(red && dw_acc && db_acc, SHM_E_SHAPE, "shm_head_bwd: null accumulator / scratch");
    if (npix == 0) return SHM_OK;
    int r = shm_zero(red, (size_t)SHM_LRELU_RED_SLOTS * (c + 1) * sizeof(double), stream);
    if (r) return r;
    const int blocks = shm_grid_cap(npix, 256 / (c / 4) * 8, 4096);
    SHM_DISPATCH_G(dtype, "shm_head_bwd",
                 hipLaunchKernelGGL((head_bwd_kernel<T, TG, false>), dim3(blocks), dim3(256), 0, (hipStream_t)stream, (const T*)x, ldx, w, y, dy, (TG*)dx, lddx, red,
                                    npix, c, slope, (const double*)nullptr, (const float*)nullptr, (float*)nullptr));
    SHM_LAUNCH_CHECK("shm_head_bwd");
    hipLaunchKernelGGL(head_fold_kernel, dim3(shm_cdiv(c + 1, 256)), dim3(256), 0, (hipStream_t)stream, (const double*)red, dw_acc, db_acc, c);
    SHM_LAUNCH_CHECK("shm_head_bwd(fold)");
    return SHM_OK;
}

// The generator head on the UN-normalised activation of the last decoder block + that block's InstanceNorm statistics: the
// block's apply pass (a read and a write of the largest activation of the network) is folded into the head's forward and backward.
extern "C" int shm_head_in_fwd(const void* a, int lda, const double* stats, const float* beta, const float* w, const float* bias, float* y, int batch,
                               int hw, int c, float slope, int dtype, void* stream) {
    SHM_REQUIRE(c % 4 == 0 && pow2_le64(c / 4) && lda % 4 == 0, SHM_E_SHAPE, "shm_head_in_fwd: channels %d unsupported", c);
    SHM_REQUIRE(a && stats && beta && w && y, SHM_E_SHAPE, "shm_head_in_fwd: null pointer");
    if (batch == 0 || hw == 0) return SHM_OK;
    int PP = 256 / (c / 4);
    long blocks = ((long)hw + PP - 1) / PP;
    const long cap = 8192 / batch > 1 ? 8192 / batch : 1;
    if (blocks > cap) blocks = cap;
    SHM_DISPATCH(dtype, "shm_head_in_fwd",
                 hipLaunchKernelGGL((head_fwd_kernel<T, true>), dim3((int)blocks, batch), dim3(256), 0, (hipStream_t)stream, (const T*)a, lda, w, bias, y,
                                    (size_t)hw, c, slope, stats, beta));
    SHM_LAUNCH_CHECK("shm_head_in_fwd");
    return SHM_OK;
}

extern "C" int shm_head_in_bwd(const void* a, int lda, const double* stats, const float* beta, const float* w, const float* y, const float* dy, void* dx,
                               int lddx, float* dz_out, double* dw_acc, double* db_acc, double* red, int batch, int hw, int c, float slope, int dtype,
                               void* stream) {
    SHM_REQUIRE(c % 4 == 0 && pow2_le64(c / 4) && lda % 4 == 0 && (!dx || lddx % 4 == 0), SHM_E_SHAPE, "shm_head_in_bwd: channels %d unsupported", c);
    SHM_REQUIRE(dx || dz_out, SHM_E_SHAPE, "shm_head_in_bwd: neither dx nor dz_out");
    SHM_REQUIRE(a && stats && beta && red && dw_acc && db_acc, SHM_E_SHAPE, "shm_head_in_bwd: null pointer");
    if (batch == 0 || hw == 0) return SHM_OK;
    int r = shm_zero(red, (size_t)SHM_LRELU_RED_SLOTS * (c + 1) * sizeof(double), stream);
    if (r) return r;
    int PP = 256 / (c / 4);
    long blocks = ((long)hw + (long)PP * 8 - 1) / ((long)PP * 8);
    const long cap = 4096 / batch > 1 ? 4096 / batch : 1;
    if (blocks > cap) blocks = cap;
    if (blocks < 1) blocks = 1;
    SHM_DISPATCH_G(dtype, "shm_head_in_bwd",
                 hipLaunchKernelGGL((head_bwd_kernel<T, TG, true>), dim3((int)blocks, batch), dim3(256), 0, (hipStream_t)stream, (const T*)a, lda, w, y, dy, (TG*)dx,
                                    lddx, red, (size_t)hw, c, slope, stats, beta, dz_out));
    SHM_LAUNCH_CHECK("shm_head_in_bwd");
    hipLaunchKernelGGL(head_fold_kernel, dim3(shm_cdiv(c + 1, 256)), dim3(256), 0, (hipStream_t)stream, (const double*)red, dw_acc, db_acc, c);
    SHM_LAUNCH_CHECK("shm_head_in_bwd(fold)");
    return SHM_OK;
}

// ------------------------------------------------------------------------ PatchGAN logits
// one block per output pixel
template <typename T>
__global__ __launch_bounds__(256) void patch_fwd_kernel(const T* __restrict__ x, int ldx, const float* __restrict__ w, float* __restrict__ y, int h, int wd, int c, float slope) {
    const int q = blockIdx.x;              // (n, i, j)
    const int j = q % wd, t = q / wd;
    const int i = t % h, n = t / h;
    const int c4 = c >> 2;
    float s = 0.f;
    for (int it = threadIdx.x; it < 9 * c4; it += 256) {
        int tap = it / c4, cl = it - tap * c4;
        int ii = i + tap / 3 - 1, jj = j + tap % 3 - 1;
        if ((unsigned)ii < (unsigned)h && (unsigned)jj < (unsigned)wd) {
            f32x4 xv = ld4(x + ((size_t)(n * h + ii) * wd + jj) * ldx + cl * 4);
            f32x4 wv = *(const f32x4*)(w + (size_t)tap * c + cl * 4);
            s += xv[0] * wv[0] + xv[1] * wv[1] + xv[2] * wv[2] + xv[3] * wv[3];
        }
    }
    s = shm_block_sum<256>(s);
    if (threadIdx.x == 0) y[q] = shm_lrelu(s, slope);
}

extern "C" int shm_patch_fwd(const void* x, int ldx, const float* w, float* y, int batch, int h, int wd, int c, float slope, int dtype, void* stream) {
    SHM_REQUIRE(c % 4 == 0 && ldx % 4 == 0, SHM_E_SHAPE, "shm_patch_fwd: channels must be a multiple of 4");
    int total = batch * h * wd;
    if (total == 0) return SHM_OK;
    SHM_DISPATCH(dtype, "shm_patch_fwd", hipLaunchKernelGGL(patch_fwd_kernel<T>, dim3(total), dim3(256), 0, (hipStream_t)stream, (const T*)x, ldx, w, y, h, wd, c, slope));
    SHM_LAUNCH_CHECK("shm_patch_fwd");
    return SHM_OK;
}

__global__ void patch_dz_kernel(const float* __restrict__ y, const float* __restrict__ dy, float* __restrict__ dz, int n, float slope) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) dz[i] = y[i] > 0.f ? dy[i] : dy[i] * slope;
}

// dx[n,i,j,c] = sum_tap dz[n, i-(kh-1), j-(kw-1)] * w[tap][c]
template <typename T>
__global__ void patch_dx_kernel(const float* __restrict__ dz, const float* __restrict__ w, T* __restrict__ dx, int lddx, int h, int wd, int c4, size_t total) {
    size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= total) return;
    int cl = (int)(idx % c4);
    size_t q = idx / c4;
    int j = (int)(q % wd);
    size_t t = q / wd;
    int i = (int)(t % h);
    size_t n = t / h;
    f32x4 s = {0.f, 0.f, 0.f, 0.f};
    for (int tap = 0; tap < 9; ++tap) {
        int ii = i - (tap / 3 - 1), jj = j - (tap % 3 - 1);
        if ((unsigned)ii < (unsigned)h && (unsigned)jj < (unsigned)wd) {
            float g = dz[(n * h + ii) * wd + jj];
            s += *(const f32x4*)(w + (size_t)tap * c4 * 4 + cl * 4) * g;
        }
    }
    st4(dx + q * lddx + cl * 4, s);
}

// dw[tap][c] = sum_{n,i,j} x[n,i+kh-1,j+kw-1,c] * dz[n,i,j]; block = (tap, 64 channels), 16 pixel groups
template <typename T>
__global__ __launch_bounds__(1024) void patch_dw_kernel(const T* __restrict__ x, int ldx, const float* __restrict__ dz, float* __restrict__ dw, int batch, int h, int wd, int c) {
    __shared__ double red[16][64];
    const int tap = blockIdx.x, ch = blockIdx.y * 64 + (threadIdx.x & 63), g = threadIdx.x >> 6;
    const int dh = tap / 3 - 1, dwv = tap % 3 - 1;
    double s = 0.0;
    if (ch < c) {
        // pixel group g takes samples g, g + 16, ...; the tap's valid output window is a rectangle, so the inner loop has no index
        // division and no branch and its loads are independent (the flat loop over pixels it replaces ran one dependent load per
        // ~1 us: 193 us for 12.6 MB)
        const int i0 = dh < 0 ? -dh : 0, i1 = dh > 0 ? h - dh : h;
        const int j0 = dwv < 0 ? -dwv : 0, j1 = dwv > 0 ? wd - dwv : wd;
        for (int n = g; n < batch; n += 16) {
            const T* xn = x + (size_t)n * h * wd * ldx + ch;
            const float* dzn = dz + (size_t)n * h * wd;
            for (int i = i0; i < i1; ++i) {
                const T* xr = xn + (size_t)((i + dh) * wd + dwv) * ldx;
                const float* dr = dzn + i * wd;
#pragma unroll 8
                for (int j = j0; j < j1; ++j) s += (double)(float)xr[(size_t)j * ldx] * (double)dr[j];
            }
        }
    }
    red[g][threadIdx.x & 63] = s;
    __syncthreads();
    if (g == 0 && ch < c) {
        double t = 0.0;
        for (int k = 0; k < 16; ++k) t += red[k][threadIdx.x & 63];
        dw[(size_t)tap * c + ch] = (float)t;
    }
}

extern "C" int shm_patch_bwd(const void* x, int ldx, const float* w, const float* y, const float* dy, float* dz,
                             void* dx, int lddx, float* dw, int batch, int h, int wd, int c, float slope, int dtype, void* stream) {
    SHM_REQUIRE(c % 4 == 0 && ldx % 4 == 0 && lddx % 4 == 0, SHM_E_SHAPE, "shm_patch_bwd: channels must be a multiple of 4");
    int npx = batch * h * wd;
    if (npx == 0) return SHM_OK;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(patch_dz_kernel, dim3(shm_cdiv(npx, 256)), dim3(256), 0, st, y, dy, dz, npx, slope);
    SHM_LAUNCH_CHECK("shm_patch_bwd(dz)");
    size_t total = (size_t)npx * (c / 4);
    SHM_DISPATCH_G(dtype, "shm_patch_bwd",
                 hipLaunchKernelGGL(patch_dx_kernel<TG>, dim3(shm_cdiv((long)total, 256)), dim3(256), 0, st, (const float*)dz, w, (TG*)dx, lddx, h, wd, c / 4, total));
    SHM_LAUNCH_CHECK("shm_patch_bwd(dx)");
    if (dw) {
        SHM_DISPATCH_G(dtype, "shm_patch_bwd",
                     hipLaunchKernelGGL(patch_dw_kernel<T>, dim3(9, shm_cdiv(c, 64)), dim3(1024), 0, st, (const T*)x, ldx, (const float*)dz, dw, batch, h, wd, c));
        SHM_LAUNCH_CHECK("shm_patch_bwd(dw)");
    }
    return SHM_OK;
}

// --------------------------------------------------------------------------------- Dense(5)
constexpr int DENSE_MAX_OUT = 8;

template <typename T>
__global__ __launch_bounds__(256) void dense_fwd_kernel(const T* __restrict__ x, const float* __restrict__ w, float* __restrict__ y, int k, int nout) {
    const int n = blockIdx.x;
    float acc[DENSE_MAX_OUT] = {};
    const T* xr = x + (size_t)n * k;
    if (nout == 5 && (k & 3) == 0 && ((size_t)xr & (4 * sizeof(T) - 1)) == 0 && ((size_t)w & 15) == 0) {
        // the classifier's shape (Dense(5)): four inputs x five outputs per iteration = one 8/16-byte load of x and five 16-byte
        // loads of w per lane, eight of them in flight (the scalar loop below is one dependent 4-byte load chain per lane:
        // 233 us for 96 samples of 65536 inputs, where the data is 14 MB)
        const int k4 = k >> 2;
#pragma unroll 2
        for (int i4 = threadIdx.x; i4 < k4; i4 += 256) {
            float xv[4];
            if constexpr (sizeof(T) == 4) {
                const f32x4 v = *(const f32x4*)(xr + 4 * (size_t)i4);
                xv[0] = v[0], xv[1] = v[1], xv[2] = v[2], xv[3] = v[3];
            } else {
                const uint2 v = *(const uint2*)(xr + 4 * (size_t)i4);
                xv[0] = __builtin_bit_cast(float, v.x << 16), xv[1] = __builtin_bit_cast(float, v.x & 0xffff0000u);
                xv[2] = __builtin_bit_cast(float, v.y << 16), xv[3] = __builtin_bit_cast(float, v.y & 0xffff0000u);
            }
            const f32x4* wp = (const f32x4*)(w + 20 * (size_t)i4);
            float wv[20];
#pragma unroll
            for (int q = 0; q < 5; ++q) {
                const f32x4 t = wp[q];
                wv[4 * q] = t[0], wv[4 * q + 1] = t[1], wv[4 * q + 2] = t[2], wv[4 * q + 3] = t[3];
            }
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
                for (int j = 0; j < 5; ++j) acc[j] += xv[e] * wv[5 * e + j];
        }
    } else {
        for (int i = threadIdx.x; i < k; i += 256) {
            float xv = (float)xr[i];
            for (int j = 0; j < nout; ++j) acc[j] += xv * w[(size_t)i * nout + j];
        }
    }
    for (int j = 0; j < nout; ++j) {
        float s = shm_block_sum<256>(acc[j]);
        if (threadIdx.x == 0) y[(size_t)n * nout + j] = s;
    }
}

extern "C" int shm_dense_fwd(const void* x, const float* w, float* y, int batch, int k, int nout, int dtype, void* stream) {
    SHM_REQUIRE(nout >= 1 && nout <= DENSE_MAX_OUT, SHM_E_SHAPE, "shm_dense_fwd: nout %d > %d", nout, DENSE_MAX_OUT);
    if (batch == 0) return SHM_OK;
    SHM_DISPATCH(dtype, "shm_dense_fwd", hipLaunchKernelGGL(dense_fwd_kernel<T>, dim3(batch), dim3(256), 0, (hipStream_t)stream, (const T*)x, w, y, k, nout));
    SHM_LAUNCH_CHECK("shm_dense_fwd");
    return SHM_OK;
}

// thread per k: dx[n][k] += sum_j dy[n][j] w[k][j];  dw[k][j] = sum_n x[n][k] dy[n][j]
template <typename T, typename TG>
__global__ __launch_bounds__(256) void dense_bwd_kernel(const T* __restrict__ x, const float* __restrict__ w, const float* __restrict__ dy, TG* __restrict__ dx,
                                                        float* __restrict__ dw, int batch, int k, int nout) {
    extern __shared__ float sdy[];          // [batch][nout]
    for (int i = threadIdx.x; i < batch * nout; i += 256) sdy[i] = dy[i];
    __syncthreads();
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= k) return;
    float wv[DENSE_MAX_OUT], acc[DENSE_MAX_OUT] = {};
    for (int j = 0; j < nout; ++j) wv[j] = w[(size_t)i * nout + j];
    int n = 0;
    for (; n + 4 <= batch; n += 4) {                  // four samples per iteration: eight independent loads in flight before the stores
        float xv[4], dv[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            xv[u] = (float)x[(size_t)(n + u) * k + i];
            dv[u] = (float)dx[(size_t)(n + u) * k + i];
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            float s = 0.f;
            for (int j = 0; j < nout; ++j) {
                float g = sdy[(n + u) * nout + j];
                s += g * wv[j];
                acc[j] += xv[u] * g;
            }
            dx[(size_t)(n + u) * k + i] = (TG)(dv[u] + s);
        }
    }
    for (; n < batch; ++n) {
        float xv = (float)x[(size_t)n * k + i];
        float s = 0.f;
        for (int j = 0; j < nout; ++j) {
            float g = sdy[n * nout + j];
            s += g * wv[j];
            acc[j] += xv * g;
        }
        dx[(size_t)n * k + i] = (TG)((float)dx[(size_t)n * k + i] + s);
    }
    if (dw)
        for (int j = 0; j < nout; ++j) dw[(size_t)i * nout + j] = acc[j];
}

extern "C" int shm_dense_bwd(const void* x, const float* w, const float* dy, void* dx, float* dw, int batch, int k, int nout, int dtype, void* stream) {
    SHM_REQUIRE(nout >= 1 && nout <= DENSE_MAX_OUT, SHM_E_SHAPE, "shm_dense_bwd: nout %d > %d", nout, DENSE_MAX_OUT);
    SHM_REQUIRE((size_t)batch * nout * 4 <= 48 * 1024, SHM_E_SHAPE, "shm_dense_bwd: batch %d too large", batch);
    if (batch == 0 || k == 0) return SHM_OK;
    SHM_DISPATCH_G(dtype, "shm_dense_bwd",
                 hipLaunchKernelGGL((dense_bwd_kernel<T, TG>), dim3(shm_cdiv(k, 256)), dim3(256), (size_t)batch * nout * 4, (hipStream_t)stream, (const T*)x, w,
                                    dy, (TG*)dx, dw, batch, k, nout));
    SHM_LAUNCH_CHECK("shm_dense_bwd");
    return SHM_OK;
}
