// InstanceNormalization backward in two passes over the tensors, fused with LeakyReLU' and the AveragePooling2D gradient: the reduce pass
// (four or, for bf16 activations, eight channels per thread) and the apply pass, also in its RAW form (shm_in_bwd_apply: sums from the gsum epilogues).
#include "in_bwd.h"

// G2 is a template parameter: a run-time `if (k.g2)` between the loads makes hipcc wait for each load
// before the branch (s_waitcnt vmcnt(0) + s_cbranch per pixel), which serialises the whole stream
// (measured 2.0 TB/s instead of 5+).
template <typename TG, bool G2, bool R1 = false>
__device__ __forceinline__ f32x4 in_bwd_dout(const InBwdArgs& k, int n, int p, int cl, const f32x4& wv = f32x4{0.f, 0.f, 0.f, 0.f}) {
    if constexpr (R1) {
        const float d = k.r1_dz[(size_t)n * k.h * k.w + p];
        return wv * d;
    }
    f32x4 g = k.nt ? ld4nt((const TG*)k.g1 + ((size_t)n * k.h * k.w + p) * k.ldg1 + cl * 4)
                   : ld4((const TG*)k.g1 + ((size_t)n * k.h * k.w + p) * k.ldg1 + cl * 4);
    if constexpr (G2) {
        int y = p / k.w, x = p - y * k.w;
        size_t q = ((size_t)n * (k.h >> 1) + (y >> 1)) * (k.w >> 1) + (x >> 1);
        f32x4 u = ld4((const TG*)k.g2 + q * k.ldg2 + cl * 4);
#pragma unroll
        for (int e = 0; e < 4; ++e) g[e] += 0.25f * u[e];
    }
    return g;
}

// The reduce pass walks the tensor back to front when k.rev is set (the input-gradient product that wrote g1 went front to back:
// its last samples are still in the Infinity Cache), the apply pass that follows front to back again (it starts where the
// reduce pass ended).
template <typename T, typename TG, bool G2, bool R1 = false>
__global__ __launch_bounds__(256) void in_bwd_reduce_kernel(const InBwdArgs k) {
    PixMap pm(k.c);
    f32x4 wr = {0.f, 0.f, 0.f, 0.f};
    if constexpr (R1) {
        if (pm.active) wr = *(const f32x4*)(k.r1_w + pm.cl * 4);
    }
    const int n = k.n0 + (k.rev ? gridDim.y - 1 - blockIdx.y : blockIdx.y), hw = k.h * k.w;
    const int bx = k.rev ? gridDim.x - 1 - blockIdx.x : blockIdx.x;
    const int p0 = bx * k.chunk, p1 = min(hw, p0 + k.chunk);
    double v[2][4] = {};
    if (pm.active) {
        float mean[4], inv[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            mean[e] = (float)k.stats[((size_t)n * k.c + pm.cl * 4 + e) * 2];
            inv[e] = (float)k.stats[((size_t)n * k.c + pm.cl * 4 + e) * 2 + 1];
        }
        // U pixels per iteration: the kernel is bound by bytes in flight, not by arithmetic -- 4 pixels of
        // 16-byte loads in fp32, 8 pixels of 8-byte loads in bf16 keep the same 8-12 x 16 B outstanding
        // per thread; the per-pixel partial sums are combined in fp32 before the fp64 accumulation
        constexpr int U = sizeof(T) == 2 ? 8 : 4;
        int p = p0 + pm.pp;
        for (; p + (U - 1) * pm.PP < p1; p += U * pm.PP) {
            f32x4 g[U], x[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                g[u] = in_bwd_dout<TG, G2, R1>(k, n, p + u * pm.PP, pm.cl, wr);
                x[u] = ld4((const T*)k.a + ((size_t)n * hw + p + u * pm.PP) * k.lda + pm.cl * 4);
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float sg = 0.f, sx = 0.f;
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    float xh = (x[u][e] - mean[e]) * inv[e];
                    sg += g[u][e];
                    sx += g[u][e] * xh;
                }
                v[0][e] += (double)sg;
                v[1][e] += (double)sx;
            }
        }
        for (; p < p1; p += pm.PP) {
            f32x4 g = in_bwd_dout<TG, G2, R1>(k, n, p, pm.cl, wr);
            f32x4 x = ld4((const T*)k.a + ((size_t)n * hw + p) * k.lda + pm.cl * 4);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float xh = (x[e] - mean[e]) * inv[e];
                v[0][e] += (double)g[e];
                v[1][e] += (double)g[e] * (double)xh;
            }
        }
    }
    block_reduce_atomic<2>(v, pm, k.red + (size_t)n * k.c * 2, k.c, true);
}

// bf16 form of the reduce pass with EIGHT channels (16 bytes) per thread: with four (8-byte loads) the pass reached 2.2-2.8 TB/s
// where its fp32 twin, whose four channels are 16 bytes, reaches 4.0 (rocprofv3, profiles/r02_*): the loads per wave are what
// limits a read-only stream.  Same sums, same scratch layout as in_bwd_reduce_kernel.
__device__ __forceinline__ f32x8 ld8(const bf16_t* p) {
    const uint4 u = *(const uint4*)p;
    f32x8 r;
    r[0] = __uint_as_float(u.x << 16);
    r[1] = __uint_as_float(u.x & 0xffff0000u);
    r[2] = __uint_as_float(u.y << 16);
    r[3] = __uint_as_float(u.y & 0xffff0000u);
    r[4] = __uint_as_float(u.z << 16);
    r[5] = __uint_as_float(u.z & 0xffff0000u);
    r[6] = __uint_as_float(u.w << 16);
    r[7] = __uint_as_float(u.w & 0xffff0000u);
    return r;
}
__device__ __forceinline__ f32x8 ld8(const float* p) {
    const f32x4 a = *(const f32x4*)p, b = *(const f32x4*)(p + 4);
    return f32x8{a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]};
}

template <typename TG, bool G2, bool R1 = false>
__global__ __launch_bounds__(256) void in_bwd_reduce8_kernel(const InBwdArgs k) {
    __shared__ double red[256 * 8];
    const int lanes_c = k.c >> 3, PP = 256 / lanes_c;
    const int pp = threadIdx.x / lanes_c, cl = threadIdx.x - pp * lanes_c;
    const bool active = pp < PP;
    const int n = k.n0 + (k.rev ? gridDim.y - 1 - blockIdx.y : blockIdx.y), hw = k.h * k.w;
    const int bx = k.rev ? gridDim.x - 1 - blockIdx.x : blockIdx.x;
    const int p0 = bx * k.chunk, p1 = min(hw, p0 + k.chunk);
    double v[2][8] = {};
    if (active) {
        float mean[8], inv[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            mean[e] = (float)k.stats[((size_t)n * k.c + cl * 8 + e) * 2];
            inv[e] = (float)k.stats[((size_t)n * k.c + cl * 8 + e) * 2 + 1];
        }
        f32x8 wr8 = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        if constexpr (R1) wr8 = ld8(k.r1_w + cl * 8);
        auto dout = [&](int p) {
            if constexpr (R1) {
                const float d = k.r1_dz[(size_t)n * hw + p];
                return wr8 * d;
            }
            f32x8 g = ld8((const TG*)k.g1 + ((size_t)n * hw + p) * k.ldg1 + cl * 8);
            if constexpr (G2) {
                const int y = p / k.w, x = p - y * k.w;
                const size_t q = ((size_t)n * (k.h >> 1) + (y >> 1)) * (k.w >> 1) + (x >> 1);
                const f32x8 u = ld8((const TG*)k.g2 + q * k.ldg2 + cl * 8);
#pragma unroll
                for (int e = 0; e < 8; ++e) g[e] += 0.25f * u[e];
            }
            return g;
        };
        constexpr int U = 4;
        int p = p0 + pp;
        // k.interleave ("elem.interleave"): a sample's blocks take tiles of U * PP pixels round-robin (back to front under k.rev) instead of
        // one contiguous chunk each: see in_bwd_apply_kernel
        const int tile = U * PP, ntiles = hw / tile;
        int pstep = tile, pend = p1;
        if (k.interleave) {
            p = (k.rev ? ntiles - 1 - (int)blockIdx.x : (int)blockIdx.x) * tile + pp;
            pstep = (k.rev ? -(int)gridDim.x : (int)gridDim.x) * tile;
            pend = ntiles * tile;
        }
        for (; p >= 0 && p + (U - 1) * PP < pend; p += pstep) {
            f32x8 g[U], x[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                g[u] = dout(p + u * PP);
                x[u] = ld8((const bf16_t*)k.a + ((size_t)n * hw + p + u * PP) * k.lda + cl * 8);
            }
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                float sg = 0.f, sx = 0.f;
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const float xh = (x[u][e] - mean[e]) * inv[e];
                    sg += g[u][e];
                    sx += g[u][e] * xh;
                }
                v[0][e] += (double)sg;
                v[1][e] += (double)sx;
            }
        }
        int ptail = p, ptend = p1;
        if (k.interleave) {                  // the pixels beyond the last whole tile: block 0, one at a time
            ptail = blockIdx.x == 0 ? pend + pp : hw;
            ptend = hw;
        }
        p = ptail;
        for (; p < ptend; p += PP) {
            const f32x8 g = dout(p);
            const f32x8 x = ld8((const bf16_t*)k.a + ((size_t)n * hw + p) * k.lda + cl * 8);
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const float xh = (x[e] - mean[e]) * inv[e];
                v[0][e] += (double)g[e];
                v[1][e] += (double)g[e] * (double)xh;
            }
        }
    }
    // combine over the PP pixel slots, then one atomic per (channel, value): red[(n*c + ch)*2 + q]
    double* dst = k.red + (size_t)n * k.c * 2;
    for (int q = 0; q < 2; ++q) {
        __syncthreads();
        if (active) {
#pragma unroll
            for (int e = 0; e < 8; ++e) red[(pp * lanes_c + cl) * 8 + e] = v[q][e];
        }
        __syncthreads();
        if (active && pp == 0) {
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                double s = 0.0;
                for (int t = 0; t < PP; ++t) s += red[(t * lanes_c + cl) * 8 + e];
                atomicAdd(&dst[(cl * 8 + e) * 2 + q], s);
            }
        }
    }
}

// RAW: the two means come from gsum slot sums (InBwdArgs::gred / gredp) instead of the reduce pass's `red`:
//   sum g     = sum g1 + sum g2                      (g2 is the gradient of the 2x2 average pool: each value reaches 4 pixels x 1/4)
//   sum g*xh  = inv * (sum g1*a - mean * sum g1)  +  (sum g2*pooled - beta * sum g2)      (pooled = avgpool(xh) + beta)
template <typename T, typename TG, bool G2, bool R1 = false, bool RAW = false>
__global__ __launch_bounds__(256) void in_bwd_apply_kernel(const InBwdArgs k) {
    PixMap pm(k.c);
    f32x4 wr = {0.f, 0.f, 0.f, 0.f};
    if constexpr (R1) {
        if (pm.active) wr = *(const f32x4*)(k.r1_w + pm.cl * 4);
    }
    const int n = k.n0 + blockIdx.y, hw = k.h * k.w;
    const int p0 = blockIdx.x * k.chunk, p1 = min(hw, p0 + k.chunk);
    // interleaved pixel mapping ("elem.interleave"): bf16 activations only -- a compile-time property of the instantiation, because the
    // float32 pass gains nothing from it and loses 5 % to the extra loop bookkeeping when it is a run-time option (4.12 -> 4.34 ms per step)
    constexpr bool IL = sizeof(T) == 2;
    // RAW: the two means of every channel, formed ONCE per block from the slot copies (thread ch sums channel ch's slots: with every
    // thread summing the slots of its own four channels the pass spent a third of its time re-reading 64 doubles per thread)
    __shared__ float sm12[RAW ? 2048 : 2];
    if constexpr (RAW) {
        for (int ch = threadIdx.x; ch < k.c; ch += 256) {
            const size_t i = ((size_t)n * k.c + ch) * 2;
            const size_t sstride = (size_t)k.nbatch * k.c * 2;
            double sg = 0.0, sga = 0.0, pg = 0.0, pgx = 0.0;
            for (int sl = 0; sl < k.gslots; ++sl) {
                sg += k.gred[sl * sstride + i];
                sga += k.gred[sl * sstride + i + 1];
            }
            if (k.gredp) {
                for (int sl = 0; sl < k.gslots; ++sl) {
                    pg += k.gredp[sl * sstride + i];
                    pgx += k.gredp[sl * sstride + i + 1];
                }
            }
            const double bt = k.gredp ? (double)k.beta[ch] : 0.0;
            sm12[ch * 2] = (float)((sg + pg) / hw);
            sm12[ch * 2 + 1] = (float)((k.stats[i + 1] * (sga - k.stats[i] * sg) + (pgx - bt * pg)) / hw);
        }
        __syncthreads();
    }
    double v[1][4] = {};
    if (pm.active) {
        float mean[4], inv[4], m1[4], m2[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            size_t i = ((size_t)n * k.c + pm.cl * 4 + e) * 2;
            mean[e] = (float)k.stats[i];
            inv[e] = (float)k.stats[i + 1];
            if constexpr (RAW) {
                m1[e] = sm12[(pm.cl * 4 + e) * 2];
                m2[e] = sm12[(pm.cl * 4 + e) * 2 + 1];
            } else {
                m1[e] = (float)(k.red[i] / hw);
                m2[e] = (float)(k.red[i + 1] / hw);
            }
        }
        constexpr int U = sizeof(T) == 2 ? 8 : 4;
        int p = p0 + pm.pp;
        // k.interleave (experiment "elem.interleave"): the blocks of a sample take tiles of U * PP pixels round-robin instead of one
        // contiguous chunk each -- at any instant the chip then reads a narrow band of the tensors instead of ~2000 separate places
        const int tile = U * pm.PP;
        int pstep = tile, pend = p1;
        if constexpr (IL)
            if (k.interleave) {
                p = blockIdx.x * tile + pm.pp;
                pstep = gridDim.x * tile;
                pend = hw - hw % tile;
            }
        for (; p + (U - 1) * pm.PP < (IL ? pend : p1); p += (IL ? pstep : tile)) {
            f32x4 g[U], x[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                g[u] = in_bwd_dout<TG, G2, R1>(k, n, p + u * pm.PP, pm.cl, wr);
                x[u] = ld4((const T*)k.a + ((size_t)n * hw + p + u * pm.PP) * k.lda + pm.cl * 4);
            }
            float sd[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int u = 0; u < U; ++u) {
                f32x4 d;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    float xh = (x[u][e] - mean[e]) * inv[e];
                    float da = inv[e] * (g[u][e] - m1[e] - xh * m2[e]);
                    d[e] = x[u][e] > 0.f ? da : da * k.slope;
                    sd[e] += d[e];
                }
                st4((T*)k.dz + ((size_t)n * hw + p + u * pm.PP) * k.lddz + pm.cl * 4, d);
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) v[0][e] += (double)sd[e];
        }
        int ptend = p1;
        if constexpr (IL)
            if (k.interleave) {              // the pixels beyond the last whole tile: block 0, one at a time
                p = blockIdx.x == 0 ? pend + pm.pp : hw;
                ptend = hw;
            }
        for (; p < (IL ? ptend : p1); p += pm.PP) {
            f32x4 g = in_bwd_dout<TG, G2, R1>(k, n, p, pm.cl, wr);
            f32x4 x = ld4((const T*)k.a + ((size_t)n * hw + p) * k.lda + pm.cl * 4);
            f32x4 d;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float xh = (x[e] - mean[e]) * inv[e];
                float da = inv[e] * (g[e] - m1[e] - xh * m2[e]);
                d[e] = x[e] > 0.f ? da : da * k.slope;
                v[0][e] += (double)d[e];
            }
            st4((T*)k.dz + ((size_t)n * hw + p) * k.lddz + pm.cl * 4, d);
        }
    }
    // bias gradient: staged per sample in red[2*batch*c + n*c + ch] -- one f64 atomic address per (n, ch)
    // instead of per ch (4096 blocks on 64 addresses cost 90-210 us per launch), folded by dbias_fold_kernel
    if (k.dbias) block_reduce_atomic<1>(v, pm, (RAW ? k.dstage : k.red + (size_t)k.nbatch * k.c * 2) + (size_t)n * k.c, k.c, true);
}

int shm_in_bwd_reduce_launch(const char* who, const InBwdArgs& k, int dtype, bool wide8, bool g2, bool r1, dim3 grid, hipStream_t st) {
    if (wide8) {                 // bf16 activations (the plan); TG = float under SHM_BF16_GF32 and for the rank-1 factors
        if (r1) hipLaunchKernelGGL((in_bwd_reduce8_kernel<float, false, true>), grid, dim3(256), 0, st, k);
        else if (dtype == SHM_BF16 && g2) hipLaunchKernelGGL((in_bwd_reduce8_kernel<bf16_t, true>), grid, dim3(256), 0, st, k);
        else if (dtype == SHM_BF16) hipLaunchKernelGGL((in_bwd_reduce8_kernel<bf16_t, false>), grid, dim3(256), 0, st, k);
        else if (g2) hipLaunchKernelGGL((in_bwd_reduce8_kernel<float, true>), grid, dim3(256), 0, st, k);
        else hipLaunchKernelGGL((in_bwd_reduce8_kernel<float, false>), grid, dim3(256), 0, st, k);
    } else if (r1) {
        SHM_DISPATCH_G(dtype, who, hipLaunchKernelGGL((in_bwd_reduce_kernel<T, TG, false, true>), grid, dim3(256), 0, st, k));
    } else if (g2) {
        SHM_DISPATCH_G(dtype, who, hipLaunchKernelGGL((in_bwd_reduce_kernel<T, TG, true>), grid, dim3(256), 0, st, k));
    } else {
        SHM_DISPATCH_G(dtype, who, hipLaunchKernelGGL((in_bwd_reduce_kernel<T, TG, false>), grid, dim3(256), 0, st, k));
    }
    return SHM_OK;
}

int shm_in_bwd_apply_launch(const char* who, const InBwdArgs& k, int dtype, bool g2, bool r1, bool raw, dim3 grid, hipStream_t st) {
    if (raw && g2) SHM_DISPATCH_G(dtype, who, hipLaunchKernelGGL((in_bwd_apply_kernel<T, TG, true, false, true>), grid, dim3(256), 0, st, k));
    else if (raw) SHM_DISPATCH_G(dtype, who, hipLaunchKernelGGL((in_bwd_apply_kernel<T, TG, false, false, true>), grid, dim3(256), 0, st, k));
    else if (r1) SHM_DISPATCH_G(dtype, who, hipLaunchKernelGGL((in_bwd_apply_kernel<T, TG, false, true>), grid, dim3(256), 0, st, k));
    else if (g2) SHM_DISPATCH_G(dtype, who, hipLaunchKernelGGL((in_bwd_apply_kernel<T, TG, true>), grid, dim3(256), 0, st, k));
    else SHM_DISPATCH_G(dtype, who, hipLaunchKernelGGL((in_bwd_apply_kernel<T, TG, false>), grid, dim3(256), 0, st, k));
    return SHM_OK;
}
