// Per-(sample, channel) gradient sums around the InstanceNorm and LeakyReLU backward: the stand-alone gsum pass (conv_igemm.hip's *_gsum entry points
// fall back to it), shm_in_bwd_apply's finish, the bias-gradient fold every backward ends in, and the LeakyReLU backward of the blocks without a
// normalisation, which ends in the same fold.
#include "in_bwd.h"

// shm_in_bwd_apply's last launch: fold the staged bias gradient (dbias[ch] += sum over samples) and clear the gsum slot copies the
// apply pass consumed -- "zero on entry, zero on return" for every f64 scratch, no memset in front of a launch.
// keep != null: the per-sample sums are also copied out ([nslot = batch][c]: the entry points' dz_sums)
__global__ __launch_bounds__(256) void gsum_finish_kernel(double* __restrict__ part, double* __restrict__ dbias, int nslot, int c, double* __restrict__ clr1,
                                                          size_t n1, double* __restrict__ clr2, size_t n2, double* __restrict__ keep) {
    __shared__ double red[4][64];
    if (dbias && blockIdx.x * 64 < (unsigned)c) {
        const int cl = threadIdx.x & 63, g = threadIdx.x >> 6;
        const int ch = blockIdx.x * 64 + cl;
        double s = 0.0;
        if (ch < c)
            for (int i = g; i < nslot; i += 4) {
                const double v = part[(size_t)i * c + ch];
                s += v;
                if (keep) keep[(size_t)i * c + ch] = v;
                part[(size_t)i * c + ch] = 0.0;
            }
        red[g][cl] = s;
        __syncthreads();
        if (g == 0 && ch < c) dbias[ch] += (red[0][cl] + red[1][cl]) + (red[2][cl] + red[3][cl]);
    }
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n1; i += stride) clr1[i] = 0.0;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n2; i += stride) clr2[i] = 0.0;
}

// nred = doubles of `red` (and of `redp`, where given) to clear
void shm_gsum_finish_launch(double* dstage, double* dbias, int batch, int c, double* red, size_t nred, double* redp, double* keep, hipStream_t st) {
    const size_t nclr = (nred * (redp ? 2 : 1) + 2047) / 2048;
    int nb = nclr < 64 ? (int)nclr : 64;
    if (nb < shm_cdiv(c, 64)) nb = shm_cdiv(c, 64);
    hipLaunchKernelGGL(gsum_finish_kernel, dim3(nb), dim3(256), 0, st, dstage, dbias, batch, c, red, nred, redp, redp ? nred : (size_t)0, keep);
}

// Stand-alone gsum: (sum g, sum g * aux) per (sample, channel) into slot 0 of red -- what the convolution epilogues produce for
// the launches they can take it in (conv_igemm.hip); the *_gsum entry points fall back to this pass otherwise.
template <typename TG, typename T>
__global__ __launch_bounds__(256) void gsum_reduce_kernel(const TG* __restrict__ g, int ldg, const T* __restrict__ aux, int ldaux, double* __restrict__ red,
                                                          int hw, int c, int chunk) {
    PixMap pm(c);
    const int n = blockIdx.y;
    const int p0 = blockIdx.x * chunk, p1 = min(hw, p0 + chunk);
    double v[2][4] = {};
    if (pm.active) {
        constexpr int U = 4;
        int p = p0 + pm.pp;
        for (; p + (U - 1) * pm.PP < p1; p += U * pm.PP) {
            f32x4 gv[U], x[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                gv[u] = ld4(g + ((size_t)n * hw + p + u * pm.PP) * ldg + pm.cl * 4);
                x[u] = ld4(aux + ((size_t)n * hw + p + u * pm.PP) * ldaux + pm.cl * 4);
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float sg = 0.f, sx = 0.f;
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    sg += gv[u][e];
                    sx += gv[u][e] * x[u][e];
                }
                v[0][e] += (double)sg;
                v[1][e] += (double)sx;
            }
        }
        for (; p < p1; p += pm.PP) {
            const f32x4 gv = ld4(g + ((size_t)n * hw + p) * ldg + pm.cl * 4);
            const f32x4 x = ld4(aux + ((size_t)n * hw + p) * ldaux + pm.cl * 4);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                v[0][e] += (double)gv[e];
                v[1][e] += (double)gv[e] * (double)x[e];
            }
        }
    }
    block_reduce_atomic<2>(v, pm, red + (size_t)n * c * 2, c, true);
}

int shm_gsum_reduce_internal(const void* g, int ldg, const void* aux, int ldaux, double* red, int batch, int hw, int c, int dtype, hipStream_t st) {
    SHM_CHECK_C(c, "gsum reduce");
    SHM_REQUIRE(ldg % 4 == 0 && ldaux % 4 == 0, SHM_E_SHAPE, "gsum reduce: bad pitch");
    if (batch == 0 || hw == 0) return SHM_OK;
    const int chunk = shm_cdiv(hw, pix_chunks(hw, batch, c, 1024));
    const dim3 grid(shm_cdiv(hw, chunk), batch);
    SHM_DISPATCH_G(dtype, "gsum reduce", hipLaunchKernelGGL((gsum_reduce_kernel<TG, T>), grid, dim3(256), 0, st, (const TG*)g, ldg, (const T*)aux, ldaux, red, hw, c, chunk));
    SHM_LAUNCH_CHECK("gsum reduce");
    return SHM_OK;
}

// dbias[ch] += sum over slots of part[slot*c + ch]
// `keep` != null: the slots -- per-sample channel sums of dz, [batch][c] -- are also copied out (the entry points' dz_sums: the second term of a
// SHM_NORM_SCALED weight gradient needs them per sample)
// `clear` != null: also zero the 2*nslot*c reduction sums in front of `part` (shm_in_bwd's scratch is zero on return).
// Block = 64 channels x 4 slot groups (a serial loop over the slots per channel was latency bound: 10 us per launch).
__global__ __launch_bounds__(256) void dbias_fold_kernel(double* __restrict__ part, double* __restrict__ dbias, int nslot, int c,
                                                         double* __restrict__ clear, double* __restrict__ keep) {
    __shared__ double red[4][64];
    const int cl = threadIdx.x & 63, g = threadIdx.x >> 6;
    const int ch = blockIdx.x * 64 + cl;
    double s = 0.0;
    if (ch < c)
        for (int i = g; i < nslot; i += 4) {
            const double v = part[(size_t)i * c + ch];
            s += v;
            if (keep) keep[(size_t)i * c + ch] = v;
            part[(size_t)i * c + ch] = 0.0;
            if (clear) {
                clear[((size_t)i * c + ch) * 2] = 0.0;
                clear[((size_t)i * c + ch) * 2 + 1] = 0.0;
            }
        }
    red[g][cl] = s;
    __syncthreads();
    if (g == 0 && ch < c) dbias[ch] += (red[0][cl] + red[1][cl]) + (red[2][cl] + red[3][cl]);
}

void shm_dbias_fold_launch(double* part, double* dbias, int nslot, int c, double* clear, double* keep, hipStream_t st) {
    hipLaunchKernelGGL(dbias_fold_kernel, dim3(shm_cdiv(c, 64)), dim3(256), 0, st, part, dbias, nslot, c, clear, keep);
}

// ---------------------------------------------------------------------- LeakyReLU backward
template <typename T, typename TG>
__global__ __launch_bounds__(256) void lrelu_bwd_kernel(const TG* __restrict__ dy, int lddy, const T* __restrict__ y, int ldy, T* __restrict__ dz, int lddz,
                                                        double* dpart, size_t npix, int c, size_t chunk, float slope) {
    PixMap pm(c);
    const size_t p0 = (size_t)blockIdx.x * chunk;
    const size_t p1 = p0 + chunk < npix ? p0 + chunk : npix;
    double v[1][4] = {};
    if (pm.active) {
        constexpr int U = sizeof(T) == 2 ? 8 : 4;
        size_t p = p0 + pm.pp;
        for (; p + (size_t)(U - 1) * pm.PP < p1; p += (size_t)U * pm.PP) {
            f32x4 g[U], x[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                g[u] = ld4(dy + (p + (size_t)u * pm.PP) * lddy + pm.cl * 4);
                x[u] = ld4(y + (p + (size_t)u * pm.PP) * ldy + pm.cl * 4);
            }
            float sd[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int u = 0; u < U; ++u) {
                f32x4 d;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    d[e] = x[u][e] > 0.f ? g[u][e] : g[u][e] * slope;
                    sd[e] += d[e];
                }
                st4(dz + (p + (size_t)u * pm.PP) * lddz + pm.cl * 4, d);
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) v[0][e] += (double)sd[e];
        }
        for (; p < p1; p += pm.PP) {
            f32x4 g = ld4(dy + p * lddy + pm.cl * 4);
            f32x4 x = ld4(y + p * ldy + pm.cl * 4);
            f32x4 d;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                d[e] = x[e] > 0.f ? g[e] : g[e] * slope;
                v[0][e] += (double)d[e];
            }
            st4(dz + p * lddz + pm.cl * 4, d);
        }
    }
    if (dpart) block_reduce_atomic<1>(v, pm, dpart + (size_t)(blockIdx.x % SHM_LRELU_RED_SLOTS) * c, c, true);
}

extern "C" int shm_lrelu_bwd(const void* dy, int lddy, const void* y, int ldy, void* dz, int lddz,
                             double* dbias, double* red, size_t npix, int c, float slope, int dtype, void* stream) {
    SHM_REQUIRE(!dbias || red, SHM_E_SHAPE, "shm_lrelu_bwd: dbias needs the f64 scratch `red`");
    SHM_CHECK_C(c, "shm_lrelu_bwd");
    SHM_REQUIRE(lddy % 4 == 0 && ldy % 4 == 0 && lddz % 4 == 0, SHM_E_SHAPE, "shm_lrelu_bwd: bad pitch");
    if (npix == 0) return SHM_OK;
    int nch = pix_chunks((long)npix, 1, c, 4096);
    size_t chunk = (npix + nch - 1) / nch;
    SHM_DISPATCH_G(dtype, "shm_lrelu_bwd",
                 hipLaunchKernelGGL((lrelu_bwd_kernel<T, TG>), dim3(shm_cdiv((long)npix, (long)chunk)), dim3(256), 0, (hipStream_t)stream, (const TG*)dy, lddy,
                                    (const T*)y, ldy, (T*)dz, lddz, dbias ? red : nullptr, npix, c, chunk, slope));
    SHM_LAUNCH_CHECK("shm_lrelu_bwd");
    if (dbias) {
        shm_dbias_fold_launch(red, dbias, SHM_LRELU_RED_SLOTS, c, nullptr, nullptr, (hipStream_t)stream);
        SHM_LAUNCH_CHECK_CLEAR("shm_lrelu_bwd(fold)", red, (size_t)SHM_LRELU_RED_SLOTS * c * sizeof(double), (hipStream_t)stream);
    }
    return SHM_OK;
}
