// InstanceNormalization backward, fused with LeakyReLU' and the AveragePooling2D gradient: the reduce + apply passes, the one-pass bf16
// kernels with their per-sample barrier, the gsum (apply-only) form and the bias-gradient folds; and the LeakyReLU backward of the blocks
// without a normalisation, which ends in the same bias-gradient fold (dbias_fold_kernel).
#include "elem.h"

// --------------------------------------------------------------------------- IN backward
struct InBwdArgs {               // g1, g2, a, dz: tensors of the kernels' element type T
    const void* g1;
    const void* g2;
    const void* a;
    const double* stats;
    double* red;
    void* dz;
    double* dbias;
    int ldg1, ldg2, lda, lddz;
    int h, w, c, chunk;
    float slope;
    int rev;
    const float* r1_dz;          // rank-1 gradient (R1 kernels): d_out[n, p, ch] = r1_dz[n * hw + p] * r1_w[ch] -- the generator head's
    const float* r1_w;           // input gradient, formed on the fly instead of being written by the head and read twice here
    // RAW apply kernels (shm_in_bwd_apply): the sums come from the epilogues of the launches that wrote g1 / g2 (gsum), as slot
    // copies [gslots][batch][c][2]: gred = (sum g1, sum g1 * a), gredp = (sum g2, sum g2 * pooled) or null; dstage = f64 [batch][c]
    // staging of the bias gradient
    const double* gred;
    const double* gredp;
    const float* beta;
    double* dstage;
    int gslots;
    int nt;                      // apply pass: g1 is read for the last time -> non-temporal loads
    int n0, nbatch;              // sample chunking (in_bwd_impl): this launch covers samples [n0, n0 + gridDim.y) of nbatch
    int interleave;              // apply pass: tiles of pixels dealt round-robin over a sample's blocks ("elem.interleave")
    int fold;                    // one-pass kernels: the launch's last group folds the staged bias gradient into dbias itself
};

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
typedef float f32x8 __attribute__((ext_vector_type(8)));
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

// ------------------------------------------------------------------------------------------------------------------------------------
// bf16 InstanceNorm backward in ONE pass over HBM (round 5).  The two-pass form reads g and a twice (reduce, apply): the
// second read of a 34-335 MB tensor pair comes from HBM again (l2_hit 0.02-0.26 in profiles/r05_bf16_traffic_pmc.json).  Here a block
// KEEPS its slice of g and a (and of the pooled gradient g2) in registers between the two phases: 8 pixels x 8 channels x 2-3 tensors per
// thread as raw bf16 (64-96 VGPRs), and the blocks of one SAMPLE meet at a per-sample barrier between the phases:
//   phase 1: partial sums (sum g, sum g * xhat) of the slice -> LDS combine -> the block's own row of a partials table (plain coherent stores:
//            no float atomics anywhere -- the first version's 192 f64 atomics per block, 2 M per launch, WERE the launch: 1.36 ms against 0.38)
//   barrier: arrival counter of the sample; the LAST ARRIVER adds the rows in block order (bitwise reproducible), publishes the two means of every
//            channel and raises the release flags (details at the code).  The blocks of a sample are consecutive block ids (blockIdx.y = sample)
//            and at most 256 of them (the launcher falls back to two passes otherwise): a whole sample is resident long before the chip is
//            full (>= 512 blocks fit), blocks are dispatched in id order, so the earliest incomplete sample always completes.  A block that
//            would spin for more than ~1 s raises the scratch's timeout word and goes on (wrong numbers, never a hang).
//   phase 2: every block applies from its registers with the published means, stores dz and writes its row of bias-gradient partials; the last
//            block to leave adds those rows in block order into the per-sample staging and clears the sample's counters, flags and means
//            (scratch: zero on entry, zero on return -- the partial rows are rewritten in full by every launch and need no clearing).
// HBM traffic: g + a read once, dz written once = 3 tensor passes instead of 5.  Phase stamps (tools/probes/in_bwd_fused_stamps.py, n = 40 at
// 256 x 256 x 64, median per block): slices loaded 3.1 us, rows written 2.4, arrival to release 13.8 (of which ~5 waiting for the sample's last
// block), phase 2 stores 1.2, departure 2.3: 23 us per block with 768 resident.  Starting the samples of the first resident generation a fraction
// of a period apart changed nothing (the launch is bound by that latency chain times the residency, not by a memory phase all blocks share).
constexpr int SHM_FUSED_FLAGS = 16, SHM_FUSED_SYNC_WORDS = 32 * (SHM_FUSED_FLAGS + 2);
// scratch (float64 units): partials f32 [batch][c / CB][bpi][3 CB] (sum g, sum g * xhat interleaved, then sum dz) | means f32 [batch][c][2] | sync u32
// [batch][c / CB][SYNC_WORDS] | timeout word.  CB = min(c, 64) channels per barrier group, bpi = blocks per group = h * w * CB / 16384.
static size_t fused_row_doubles(int batch, size_t bpi, int c) { return ((size_t)batch * bpi * 3 * c + 1) / 2; }        // fp32 rows: [batch][c / CB][bpi][3 CB]
static size_t fused_scratch_doubles(int batch, int hw, int c) {
    const int cb = c < 64 ? c : 64;
    const size_t bpi = (size_t)hw * cb / 16384;
    return fused_row_doubles(batch, bpi, c) + (size_t)batch * c + (size_t)batch * (c / cb) * (SHM_FUSED_SYNC_WORDS / 2) + 1;
}
__device__ __forceinline__ f32x8 unpack8(const shm_u32x4 u) {
    f32x8 r;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        r[2 * i] = __uint_as_float(u[i] << 16);
        r[2 * i + 1] = __uint_as_float(u[i] & 0xffff0000u);
    }
    return r;
}
// coherent (device-scope, L2-bypassing) accesses without fences: see the barrier below
template <typename V>
__device__ __forceinline__ V coh_load(const V* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
template <typename V>
__device__ __forceinline__ void coh_store(V* p, V v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// The launch's last group folds the staged bias gradient (round 6: dbias_fold_kernel was one more launch behind each of the step's ~44 one-pass
// calls).  `staging` = f64 [batch][c], written by every group's last departer (its CB channels of its sample, coherent stores, acknowledged before
// the group takes a ticket at `ticket`); the group whose ticket is the last adds the samples in dbias_fold_kernel's order -- four interleaved partial
// sums, (s0 + s1) + (s2 + s3): the same bits as the separate launch -- into dbias, and leaves staging and ticket zero.  Called by all 256 threads of a
// group's last departer, after its staging stores.
__device__ __forceinline__ void fused_fold_dbias(double* __restrict__ staging, double* __restrict__ dbias, unsigned* __restrict__ ticket, int batch, int c,
                                                 unsigned ngroups, int* s_flag) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0) *s_flag = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) + 1u == ngroups;
    __syncthreads();
    if (!*s_flag) return;
    for (int ch = threadIdx.x; ch < c; ch += 256) {
        double sg[4] = {0.0, 0.0, 0.0, 0.0};
        int i = 0;
        for (; i + 8 <= batch; i += 8) {             // eight loads in flight (one at a time, 160 samples were 160 round trips)
            double v[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = coh_load(staging + (size_t)(i + j) * c + ch);
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                sg[j & 3] += v[j];                   // (i is a multiple of 8: (i + j) & 3 == j & 3)
                coh_store(staging + (size_t)(i + j) * c + ch, 0.0);
            }
        }
        for (; i < batch; ++i) {
            sg[i & 3] += coh_load(staging + (size_t)i * c + ch);
            coh_store(staging + (size_t)i * c + ch, 0.0);
        }
        dbias[ch] += (sg[0] + sg[1]) + (sg[2] + sg[3]);
    }
    if (threadIdx.x == 0) coh_store(ticket, 0u);
}

template <bool G2>
__global__ __launch_bounds__(256, G2 ? 3 : 4) void in_bwd_fused8_kernel(const InBwdArgs k, float* __restrict__ fpart, float* __restrict__ fres,
                                                                         unsigned* __restrict__ fsync, unsigned* __restrict__ ferr,
                                                                         unsigned* __restrict__ abort_dev, unsigned* __restrict__ abort_host,
                                                                         const unsigned arrivals) {
    // arrivals: blocks a group's barrier waits for = gridDim.x (one more under "elem.fused_test_stall": the timeout path under test)
    constexpr int U = 8;
    __shared__ double red[256 * 8];
    __shared__ float sm12[128], smi[128];
    __shared__ int s_last;
    // A barrier GROUP is (sample, block of CB = min(c, 64) channels): its blocks are the 16384 / CB-pixel slices of the map, blockIdx.x.  (With the
    // whole channel range in one group the 256- and 512-channel levels had short slices, rows of 3 c values and a last arriver adding
    // bpi * c / 256 values per thread: slower than the two passes at n = 20.)  A pixel's CB channels are one 128-byte line (c >= 64).
    const int CB = k.c < 64 ? k.c : 64, c0 = blockIdx.y * CB;
    const int lanes_c = CB >> 3, PP = 256 / lanes_c;                   // CB is a power of two (launcher): every thread is active
    const int pp = threadIdx.x / lanes_c, cl = threadIdx.x - pp * lanes_c;
    const int n = k.rev ? (int)gridDim.z - 1 - (int)blockIdx.z : (int)blockIdx.z, hw = k.h * k.w;
    const int gidx = n * gridDim.y + blockIdx.y;                       // the group
    const int pbase = blockIdx.x * (U * PP) + pp;                      // pixel of slot u: pbase + u * PP (hw % (U * PP) == 0)
    const int bpi = gridDim.x, c3 = 3 * CB;
    float* const prow0 = fpart + (size_t)gidx * bpi * c3;              // the group's rows; row b = [CB][2] sums, then [CB] bias-gradient partials
    float* const prow = prow0 + (size_t)blockIdx.x * c3;               // (fp32: a row holds sums over one slice, and the means are fp32 in the end)

#ifdef SHM_FUSED_STAMP
    unsigned long long* const stamp = (unsigned long long*)(ferr + 2) + ((size_t)gidx * gridDim.x + blockIdx.x) * 12;
#define FSTAMP(i) do { if (threadIdx.x == 0) stamp[i] = __builtin_amdgcn_s_memrealtime(); } while (0)
#else
#define FSTAMP(i) do { } while (0)
#endif
    FSTAMP(0);
    // Pixel of slot u.  Plain form: pbase + u * PP (a slice is 256 consecutive pixels).  Pooled form (CB = 64, PP = 32): a slice is a tile of
    // R rows x Wt = min(w, 128) columns, R * Wt = 256, and a thread owns two 2 x 2 QUADS of it (quad pp and pp + 32 of the tile's 64): one pooled
    // gradient value serves four pixels, two loads instead of eight -- with eight the form needs 204 registers and two blocks per CU.
    int qbase = 0, wt2 = 1;                                              // pooled form: pixel index of the tile's origin, quads per tile row
    if constexpr (G2) {
        const int wt = k.w < 128 ? k.w : 128, tpr = k.w / wt, ty = blockIdx.x / tpr, tx = blockIdx.x - ty * tpr;
        wt2 = wt >> 1;
        qbase = ty * (256 / wt) * k.w + tx * wt;
    }
    auto pix = [&](int u, int base) {
        if constexpr (G2) {
            const int q = pp + 32 * (u >> 2), qy = q / wt2, qx = q - qy * wt2;
            return base + (2 * qy + ((u >> 1) & 1)) * k.w + 2 * qx + (u & 1);
        } else {
            return base + u * PP;
        }
    };
    shm_u32x4 gq[U], aq[U];
    [[maybe_unused]] shm_u32x4 hq[2];
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const int p = pix(u, G2 ? qbase : pbase);
        const size_t off = (size_t)n * hw + p;
        gq[u] = *(const shm_u32x4*)((const bf16_t*)k.g1 + off * k.ldg1 + c0 + cl * 8);
        aq[u] = *(const shm_u32x4*)((const bf16_t*)k.a + off * k.lda + c0 + cl * 8);
        if constexpr (G2) {
            if ((u & 3) == 0) {
                const int y = p / k.w, x = p - y * k.w;
                const size_t q = ((size_t)n * (k.h >> 1) + (y >> 1)) * (k.w >> 1) + (x >> 1);
                hq[u >> 2] = *(const shm_u32x4*)((const bf16_t*)k.g2 + q * k.ldg2 + c0 + cl * 8);
            }
        }
    }
    float mean[8], inv[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        mean[e] = (float)k.stats[((size_t)n * k.c + c0 + cl * 8 + e) * 2];
        inv[e] = (float)k.stats[((size_t)n * k.c + c0 + cl * 8 + e) * 2 + 1];
    }
    if (pp == 0) {                    // phase 2 takes them from LDS again: sixteen registers less across the barrier
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            smi[(cl * 8 + e) * 2] = mean[e];
            smi[(cl * 8 + e) * 2 + 1] = inv[e];
        }
    }
    auto gval = [&](int u) {
        f32x8 g = unpack8(gq[u]);
        if constexpr (G2) {
            const f32x8 h = unpack8(hq[u >> 2]);
#pragma unroll
            for (int e = 0; e < 8; ++e) g[e] += 0.25f * h[e];
        }
        return g;
    };
    // Combine NV x 8 per-thread values over the PP pixel slots and store them: value j of channel ch lands at dst[ch * stride + j].  Every thread
    // parks its values in LDS (fp32, [j][pp][c]), thread t < NV * c adds the PP terms of one output (consecutive threads read consecutive words).
    // (The first version -- eight threads adding 32 LDS doubles each, twice -- took 21 of a block's 46 us; xor-shuffles spilled 116 registers.)
    float* const redf = (float*)red;
    auto park = [&](const float (&v)[8], int j) {
        *(f32x4*)&redf[j * 2048 + threadIdx.x * 8] = f32x4{v[0], v[1], v[2], v[3]};
        *(f32x4*)&redf[j * 2048 + threadIdx.x * 8 + 4] = f32x4{v[4], v[5], v[6], v[7]};
    };
    auto finish = [&](int nv, float* dst, int stride) {
        __syncthreads();
        for (int t = threadIdx.x; t < CB * nv; t += 256) {
            const int j = t / CB, ch = t - j * CB;
            float sum = 0.f;
            for (int q = 0; q < PP; ++q) sum += redf[j * 2048 + q * CB + ch];
            coh_store(&dst[ch * stride + j], sum);
        }
    };
    // Sums of `npairs` consecutive float PAIRS of every row of the sample, in a fixed order (bitwise reproducible): thread (rg, q) adds pair q of
    // rows rg, rg + RG, ... (sixteen 8-byte coherent loads in flight), the RG partial sums meet in LDS; on return thread v < 2 * npairs calls
    // total(v).  (One thread per value walking all 256 rows, eight loads at a time, made the barrier 45 us long.)
    auto rowsum = [&](const float* base, int npairs) {
        const int P = npairs < 256 ? npairs : 256, RG = 256 / P, rg = threadIdx.x / P;
        __syncthreads();
        for (int q = threadIdx.x % P; q < npairs; q += P) {
            double s0 = 0.0, s1 = 0.0;
            const unsigned long long* col = (const unsigned long long*)base + q;
            const size_t rs = (size_t)c3 / 2;                                // row stride in pairs (c3 is even)
            int b = rg;
            for (; b + 15 * RG < bpi; b += 16 * RG) {
                unsigned long long t[16];
#pragma unroll
                for (int j = 0; j < 16; ++j) t[j] = coh_load(col + (size_t)(b + j * RG) * rs);
#pragma unroll
                for (int j = 0; j < 16; ++j) {
                    s0 += (double)__uint_as_float((unsigned)t[j]);
                    s1 += (double)__uint_as_float((unsigned)(t[j] >> 32));
                }
            }
            for (; b < bpi; b += RG) {
                const unsigned long long t = coh_load(col + (size_t)b * rs);
                s0 += (double)__uint_as_float((unsigned)t);
                s1 += (double)__uint_as_float((unsigned)(t >> 32));
            }
            red[(rg * npairs + q) * 2] = s0;
            red[(rg * npairs + q) * 2 + 1] = s1;
        }
        __syncthreads();
        return RG;
    };
    auto total = [&](int v, int npairs, int RG) {
        double s = 0.0;
        for (int r = 0; r < RG; ++r) s += red[(r * npairs + (v >> 1)) * 2 + (v & 1)];
        return s;
    };
    // ---- phase 1
    {
        float sg[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, sx[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#ifdef SHM_FUSED_STAMP
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        FSTAMP(1);
#endif
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const f32x8 g = gval(u), x = unpack8(aq[u]);
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const float xh = (x[e] - mean[e]) * inv[e];
                sg[e] += g[e];
                sx[e] += g[e] * xh;
            }
        }
        __syncthreads();
        park(sg, 0);
        park(sx, 1);
        finish(2, prow, 2);
    }
    // ---- the sample's barrier.  No agent-scope FENCES: on a multi-XCD chip a release fence is buffer_wbl2 (write the XCD's dirty L2 lines back)
    // and every acquire -- one per poll -- a buffer_inv of the L2 (0.65 ms per launch with ~1000 resident blocks; even ONE acq_rel arrival, one
    // release flag store and one acquire fence behind the poll loop per block: 1 191 us against 291 for the n = 40 level, step 31.7 against 22.8 ms).
    // Everything the blocks exchange
    // moves through device-scope relaxed atomics (loads, stores, the two counters), which are performed at the device's coherence point: a block
    // waits for the acknowledgement of its stores (vmcnt) and then counts its arrival.  And no crowd on one address: 256 blocks polling the arrival
    // counter queue their reads in front of the arrivals themselves (measured: 41 us per sample).  The LAST ARRIVER (it alone knows every row is
    // in) publishes the means and raises SHM_FUSED_FLAGS copies of the release flag, each in its own 128-byte line; block b polls copy b % 16.
    unsigned* const sy = fsync + (size_t)gidx * SHM_FUSED_SYNC_WORDS;     // [0] arrivals, [32] departures, [64 + 32 j] flag copy j
    float* const res = fres + ((size_t)n * k.c + c0) * 2;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    FSTAMP(2);
    if (threadIdx.x == 0) s_last = __hip_atomic_fetch_add(sy, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) + 1u == arrivals;
    __syncthreads();
    FSTAMP(3);
    if (s_last) {
        FSTAMP(8);
        const int RG = rowsum(prow0, CB);
        FSTAMP(9);
        for (int v = threadIdx.x; v < 2 * CB; v += 256) {
            const float r = (float)(total(v, CB, RG) / hw);
            sm12[v] = r;
            coh_store(res + v, r);
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");          // the means are written before a flag goes up
        __syncthreads();
        FSTAMP(10);
        if (threadIdx.x < SHM_FUSED_FLAGS) coh_store(sy + 64 + 32 * threadIdx.x, 1u);
    } else {
        if (threadIdx.x == 0) {
            const unsigned* const flag = sy + 64 + 32 * (blockIdx.x % SHM_FUSED_FLAGS);
            int spins = 0;
            while (coh_load(flag) == 0u) {
                __builtin_amdgcn_s_sleep(16);
                if (++spins > (arrivals == gridDim.x ? 1 << 20 : 1 << 10)) {          // (the stalled test form gives up after ~1 ms)
                    // gave up: this launch goes on with wrong means.  The scratch's own word names the buffer; the caller's abort words
                    // (shm_in_bwd's abort_dev / abort_host) make it fatal: shm_adam_clip applies nothing while the device word is set, and the host word
                    // (mapped host memory) lets the trainer see it without a synchronisation
                    __hip_atomic_fetch_or(ferr, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    if (abort_dev) __hip_atomic_fetch_or(abort_dev, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    if (abort_host) __hip_atomic_store(abort_host, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                    break;
                }
            }
        }
        __syncthreads();
        for (int i = threadIdx.x; i < CB * 2; i += 256) sm12[i] = coh_load(res + i);
    }
    __syncthreads();
    FSTAMP(4);
    // ---- phase 2 (the raw slices pass through an opaque copy: otherwise hipcc keeps phase 1's UNPACKED values alive across the barrier and spills)
#pragma unroll
    for (int u = 0; u < U; ++u) {
        asm volatile("" : "+v"(gq[u]), "+v"(aq[u]));
        if constexpr (G2)
            if ((u & 3) == 0) asm volatile("" : "+v"(hq[u >> 2]));
    }
    int pb2 = G2 ? qbase : pbase;     // (opaque as well: the store addresses are formed here, not carried from the loads at the top)
    asm volatile("" : "+v"(pb2));
    // d = inv * (g - m1 - xhat * m2) with xhat = (x - mean) * inv, as three constants per channel: d = A g - (B x + C)
    float cA[8], cB[8], cC[8], sd[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const float m1 = sm12[(cl * 8 + e) * 2], m2 = sm12[(cl * 8 + e) * 2 + 1], mu = smi[(cl * 8 + e) * 2], iv = smi[(cl * 8 + e) * 2 + 1];
        cA[e] = iv;
        cB[e] = iv * iv * m2;
        cC[e] = iv * m1 - cB[e] * mu;
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const f32x8 g = gval(u), x = unpack8(aq[u]);
        typedef bf16_t bf16x8_t __attribute__((ext_vector_type(8)));
        bf16x8_t o;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const float da = cA[e] * g[e] - (cB[e] * x[e] + cC[e]);
            const float d = x[e] > 0.f ? da : da * k.slope;
            sd[e] += d;
            o[e] = (bf16_t)d;
        }
        *(bf16x8_t*)((bf16_t*)k.dz + ((size_t)n * hw + pix(u, pb2)) * k.lddz + c0 + cl * 8) = o;
    }
    FSTAMP(5);
    if (k.dbias) {
        __syncthreads();
        park(sd, 0);
        finish(1, prow + 2 * CB, 1);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");          // this block's row is written before its departure is counted
    }
    __syncthreads();
    if (threadIdx.x == 0) s_last = __hip_atomic_fetch_add(sy + 32, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) + 1u == gridDim.x;
    __syncthreads();
    FSTAMP(6);
    if (s_last) {                     // every block of the sample is through: the bias-gradient staging of the sample, then a clean scratch
        if (k.dbias) {
            const int RG = rowsum(prow0 + 2 * CB, CB / 2);
            for (int ch = threadIdx.x; ch < CB; ch += 256) coh_store(k.red + (size_t)k.nbatch * k.c * 2 + (size_t)n * k.c + c0 + ch, total(ch, CB / 2, RG));
        }
        for (int i = threadIdx.x; i < CB * 2; i += 256) coh_store(res + i, 0.f);
        if (threadIdx.x < SHM_FUSED_FLAGS + 2) coh_store(sy + 32 * threadIdx.x, 0u);
        // fold = 1: this launch also folds the staged bias gradient (no dbias_fold_kernel behind it); ferr[1] is the launch's group ticket
        if (k.dbias && k.fold) fused_fold_dbias(k.red + (size_t)k.nbatch * k.c * 2, k.dbias, ferr + 1, k.nbatch, k.c, gridDim.y * gridDim.z, &s_last);
    }
#ifdef SHM_FUSED_STAMP
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    FSTAMP(7);
#endif
#undef FSTAMP
}

// ------------------------------------------------------------------------------------------------------------------------------------
// Round 6: the same one-pass protocol with HALF the registers per byte of traffic.  in_bwd_fused8_kernel is bound by residency x latency (a
// block holds its 64 KiB of g and a for ~23 us; 4 blocks per CU fill the register file: 768-1024 x 96 KiB of traffic per 23 us = 3.2-4.3 TB/s,
// LABNOTES 11.6).  Here a block holds ONLY g (the gradient is dead after this kernel; the activation stays in HBM and the Infinity Cache): a slice
// is 16 pixel slots per thread (32768 / CB pixels), g raw bf16 in 64 registers, and `a` is streamed through 16-byte transient registers twice --
// phase 1 for sum g * (x - mean), phase 2 for the apply (the second read, 20-30 us after the first, was meant to hit the Infinity Cache; the
// counters of profiles/r06_* say it comes from HBM: 1.38 x the algorithmic bytes -- the kernel is residency bound and faster all the same).  The
// same 4 blocks per CU now cover 192 KiB of traffic each, and a barrier group has HALF the blocks (128 on the 256 x 256 x 64 maps: the last
// arriver's row sums, 5.9 of 13.3 us there, halve; the 512 x 512 maps of BASELINE configs[3] get 512-block groups, which twice fit the chip).
// The register budget decides the form: 64 (g) + 16 (sums) + 8 (means) leave room for TWO transient loads of `a` per batch at four blocks per CU
// (<2, 2, 4>: 8 spills; eight batches per phase, each a round trip); eight per batch need three blocks per CU (<8, 8, 3>).  hipcc has to be held
// to the batches by data dependences (below).  Measured, n = 40 / 160 at 256 x 256 x 64: 287 / 1072 us (in_bwd_fused8_kernel) -> 252 / 879 (<2, 2, 4>),
// 262 / 920 (<8, 8, 3>); on maps with fewer blocks per group the extra round trips lose (128 x 128 x 128: 122 -> 147): see the launcher.
// Sums: sum g and sum g * (x - mean) per slice in fp32 (the centring keeps the second one free of the cancellation a raw sum g * x would meet
// when |mean| >> 1 / inv), times inv at the end; everything else -- rows, last arriver, flags, timeout and abort words, departure -- as above.
#define FG_LOAD(rs, base, voff, soff) __builtin_bit_cast(shm_u32x4, __builtin_amdgcn_raw_buffer_load_b128(rs, voff, soff, 0))
#define FG_STORE(v, rs, base, voff) __builtin_amdgcn_raw_buffer_store_b128(v, rs, voff, 0, 0)
template <int AB, int AB2, int BPC>          // transient `a` loads in flight per batch in phase 1 / phase 2; blocks per CU the register budget is cut for
__global__ __launch_bounds__(256, BPC) void in_bwd_fusedg_kernel(const InBwdArgs k, float* __restrict__ fpart, float* __restrict__ fres,
                                                               unsigned* __restrict__ fsync, unsigned* __restrict__ ferr,
                                                               unsigned* __restrict__ abort_dev, unsigned* __restrict__ abort_host, const unsigned arrivals) {
    constexpr int U = 16;
    __shared__ double red[256 * 8];
    __shared__ float sm12[128], smi[128];
    __shared__ int s_last;
    const int CB = k.c < 64 ? k.c : 64, c0 = blockIdx.y * CB;
    const int lanes_c = CB >> 3, PP = 256 / lanes_c;
    const int pp = threadIdx.x / lanes_c, cl = threadIdx.x - pp * lanes_c;
    const int n = k.rev ? (int)gridDim.z - 1 - (int)blockIdx.z : (int)blockIdx.z, hw = k.h * k.w;
    const int gidx = n * gridDim.y + blockIdx.y;
    const int pbase = blockIdx.x * (U * PP) + pp;
    const int bpi = gridDim.x, c3 = 3 * CB;
    float* const prow0 = fpart + (size_t)gidx * bpi * c3;
    float* const prow = prow0 + (size_t)blockIdx.x * c3;
    // buffer accesses: one descriptor per tensor and SAMPLE (a sample is below 4 GiB: launcher), the lane's byte offset in ONE register, the pixel
    // slot as a scalar offset -- with flat 64-bit addresses hipcc kept sixteen address pairs alive beside the 64 registers of g and spilled 216
    const unsigned samp_g = (unsigned)hw * (unsigned)k.ldg1 * 2u, samp_a = (unsigned)hw * (unsigned)k.lda * 2u, samp_z = (unsigned)hw * (unsigned)k.lddz * 2u;
    const __amdgpu_buffer_rsrc_t rsg = __builtin_amdgcn_make_buffer_rsrc((char*)k.g1 + (size_t)n * samp_g, 0, samp_g, 0x00020000);
    const __amdgpu_buffer_rsrc_t rsa = __builtin_amdgcn_make_buffer_rsrc((char*)k.a + (size_t)n * samp_a, 0, samp_a, 0x00020000);
    const __amdgpu_buffer_rsrc_t rsz = __builtin_amdgcn_make_buffer_rsrc((char*)k.dz + (size_t)n * samp_z, 0, samp_z, 0x00020000);
    const unsigned og = (unsigned)(pbase * k.ldg1 + c0 + cl * 8) * 2u, oa = (unsigned)(pbase * k.lda + c0 + cl * 8) * 2u;
    const unsigned sg_step = (unsigned)(PP * k.ldg1) * 2u, sa_step = (unsigned)(PP * k.lda) * 2u, sz_step = (unsigned)(PP * k.lddz) * 2u;      // scalars
    shm_u32x4 gq[U];
#pragma unroll
    for (int u = 0; u < U; ++u) gq[u] = FG_LOAD(rsg, (const char*)k.g1 + (size_t)n * samp_g, og, (unsigned)u * sg_step);
    float* const redf = (float*)red;
    auto park = [&](const float (&v)[8], int j) {
        *(f32x4*)&redf[j * 2048 + threadIdx.x * 8] = f32x4{v[0], v[1], v[2], v[3]};
        *(f32x4*)&redf[j * 2048 + threadIdx.x * 8 + 4] = f32x4{v[4], v[5], v[6], v[7]};
    };
    auto finish = [&](int nv, float* dst, int stride) {
        __syncthreads();
        for (int t = threadIdx.x; t < CB * nv; t += 256) {
            const int j = t / CB, ch = t - j * CB;
            float sum = 0.f;
            for (int q = 0; q < PP; ++q) sum += redf[j * 2048 + q * CB + ch];
            coh_store(&dst[ch * stride + j], sum);
        }
    };
    auto rowsum = [&](const float* base, int npairs) {
        const int P = npairs < 256 ? npairs : 256, RG = 256 / P, rg = threadIdx.x / P;
        __syncthreads();
        for (int q = threadIdx.x % P; q < npairs; q += P) {
            double s0 = 0.0, s1 = 0.0;
            const unsigned long long* col = (const unsigned long long*)base + q;
            const size_t rs = (size_t)c3 / 2;
            int b = rg;
            for (; b + 15 * RG < bpi; b += 16 * RG) {
                unsigned long long t[16];
#pragma unroll
                for (int j = 0; j < 16; ++j) t[j] = coh_load(col + (size_t)(b + j * RG) * rs);
#pragma unroll
                for (int j = 0; j < 16; ++j) {
                    s0 += (double)__uint_as_float((unsigned)t[j]);
                    s1 += (double)__uint_as_float((unsigned)(t[j] >> 32));
                }
            }
            for (; b < bpi; b += RG) {
                const unsigned long long t = coh_load(col + (size_t)b * rs);
                s0 += (double)__uint_as_float((unsigned)t);
                s1 += (double)__uint_as_float((unsigned)(t >> 32));
            }
            red[(rg * npairs + q) * 2] = s0;
            red[(rg * npairs + q) * 2 + 1] = s1;
        }
        __syncthreads();
        return RG;
    };
    auto total = [&](int v, int npairs, int RG) {
        double s = 0.0;
        for (int r = 0; r < RG; ++r) s += red[(r * npairs + (v >> 1)) * 2 + (v & 1)];
        return s;
    };
    // ---- phase 1: `a` passes through sixteen-byte transients; (sum g, inv * sum g * (x - mean)) of the slice -> the block's row
    {
        float mean[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) mean[e] = (float)k.stats[((size_t)n * k.c + c0 + cl * 8 + e) * 2];
        if (pp == 0) {
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                smi[(cl * 8 + e) * 2] = mean[e];
                smi[(cl * 8 + e) * 2 + 1] = (float)k.stats[((size_t)n * k.c + c0 + cl * 8 + e) * 2 + 1];
            }
        }
        float sg[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, sx[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        unsigned oab = oa;
        // `a` in batches of AB transient loads (the register budget of four blocks per CU: 64 for g + 16 sums + 8 means leave ~32); the
        // sched_barrier keeps hipcc from hoisting the next batch's loads over this batch's arithmetic (it would: 168 spills)
#pragma unroll
        for (int b = 0; b < U / AB; ++b) {
            shm_u32x4 aq[AB];
#pragma unroll
            for (int u = 0; u < AB; ++u) aq[u] = FG_LOAD(rsa, (const char*)k.a + (size_t)n * samp_a, oab, (unsigned)(b * AB + u) * sa_step);
            // (the g-only half of the arithmetic -- unpack, sum g -- is pure register work: left visible, LLVM hoists it for all sixteen slots to
            // the top of the kernel, 128 live floats; the opaque copy ties it to its batch)
#pragma unroll
            for (int u = 0; u < AB; ++u) asm volatile("" : "+v"(gq[b * AB + u]));
#pragma unroll
            for (int u = 0; u < AB; ++u) {
                const f32x8 x = unpack8(aq[u]), g = unpack8(gq[b * AB + u]);
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    sg[e] += g[e];
                    sx[e] += g[e] * (x[e] - mean[e]);
                }
            }
            // the next batch's loads wait (as far as hipcc can see) for this batch's sums: otherwise all sixteen are hoisted to the top
            asm volatile("" : "+v"(oab) : "v"(sg[0]), "v"(sg[1]), "v"(sg[2]), "v"(sg[3]), "v"(sg[4]), "v"(sg[5]), "v"(sg[6]), "v"(sg[7]), "v"(sx[0]), "v"(sx[1]), "v"(sx[2]), "v"(sx[3]),
                         "v"(sx[4]), "v"(sx[5]), "v"(sx[6]), "v"(sx[7]));
        }
        __syncthreads();                    // smi is written
#pragma unroll
        for (int e = 0; e < 8; ++e) sx[e] *= smi[(cl * 8 + e) * 2 + 1];
        park(sg, 0);
        park(sx, 1);
        finish(2, prow, 2);
    }
    // ---- the group's barrier (in_bwd_fused8_kernel: relaxed device-scope atomics, the last arriver adds the rows in block order and raises the flags)
    unsigned* const sy = fsync + (size_t)gidx * SHM_FUSED_SYNC_WORDS;
    float* const res = fres + ((size_t)n * k.c + c0) * 2;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0) s_last = __hip_atomic_fetch_add(sy, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) + 1u == arrivals;
    __syncthreads();
    if (s_last) {
        const int RG = rowsum(prow0, CB);
        for (int v = threadIdx.x; v < 2 * CB; v += 256) {
            const float r = (float)(total(v, CB, RG) / hw);
            sm12[v] = r;
            coh_store(res + v, r);
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (threadIdx.x < SHM_FUSED_FLAGS) coh_store(sy + 64 + 32 * threadIdx.x, 1u);
    } else {
        if (threadIdx.x == 0) {
            const unsigned* const flag = sy + 64 + 32 * (blockIdx.x % SHM_FUSED_FLAGS);
            int spins = 0;
            while (coh_load(flag) == 0u) {
                __builtin_amdgcn_s_sleep(16);
                if (++spins > (arrivals == gridDim.x ? 1 << 20 : 1 << 10)) {
                    __hip_atomic_fetch_or(ferr, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    if (abort_dev) __hip_atomic_fetch_or(abort_dev, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    if (abort_host) __hip_atomic_store(abort_host, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                    break;
                }
            }
        }
        __syncthreads();
        for (int i = threadIdx.x; i < CB * 2; i += 256) sm12[i] = coh_load(res + i);
    }
    __syncthreads();
    // ---- phase 2: d = A g - (B x + C) from the held g and a second read of a
#pragma unroll
    for (int u = 0; u < U; ++u) asm volatile("" : "+v"(gq[u]));
    int pb2 = pbase;
    asm volatile("" : "+v"(pb2));
    const unsigned oa2 = (unsigned)(pb2 * k.lda + c0 + cl * 8) * 2u, oz = (unsigned)(pb2 * k.lddz + c0 + cl * 8) * 2u;
    float cA[8], cB[8], cC[8], sd[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const float m1 = sm12[(cl * 8 + e) * 2], m2 = sm12[(cl * 8 + e) * 2 + 1], mu = smi[(cl * 8 + e) * 2], iv = smi[(cl * 8 + e) * 2 + 1];
        cA[e] = iv;
        cB[e] = iv * iv * m2;
        cC[e] = iv * m1 - cB[e] * mu;
    }
    unsigned oa2b = oa2;
#pragma unroll
    for (int b = 0; b < U / AB2; ++b) {
        shm_u32x4 aq[AB2];
#pragma unroll
        for (int u = 0; u < AB2; ++u) aq[u] = FG_LOAD(rsa, (const char*)k.a + (size_t)n * samp_a, oa2b, (unsigned)(b * AB2 + u) * sa_step);
#pragma unroll
        for (int u = 0; u < AB2; ++u) asm volatile("" : "+v"(gq[b * AB2 + u]));
#pragma unroll
        for (int u = 0; u < AB2; ++u) {
            const f32x8 g = unpack8(gq[b * AB2 + u]), x = unpack8(aq[u]);
            typedef bf16_t bf16x8_t __attribute__((ext_vector_type(8)));
            bf16x8_t o;
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const float da = cA[e] * g[e] - (cB[e] * x[e] + cC[e]);
                const float d = x[e] > 0.f ? da : da * k.slope;
                sd[e] += d;
                o[e] = (bf16_t)d;
            }
            // the slot offset goes into the VECTOR offset: behind a 16-byte buffer store whose soffset is an SGPR hipcc leaves no wait states in front of
            // a VALU write of the store's data registers, and the MI355X needs them (common.h, round 4; tools/check_isa_hazards.py flags the form)
            FG_STORE(__builtin_bit_cast(shm_u32x4, o), rsz, (char*)k.dz + (size_t)n * samp_z, oz + (unsigned)(b * AB2 + u) * sz_step);
        }
        asm volatile("" : "+v"(oa2b) : "v"(sd[0]), "v"(sd[1]), "v"(sd[2]), "v"(sd[3]), "v"(sd[4]), "v"(sd[5]), "v"(sd[6]), "v"(sd[7]));
    }
    if (k.dbias) {
        __syncthreads();
        park(sd, 0);
        finish(1, prow + 2 * CB, 1);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    __syncthreads();
    if (threadIdx.x == 0) s_last = __hip_atomic_fetch_add(sy + 32, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) + 1u == gridDim.x;
    __syncthreads();
    if (s_last) {
        if (k.dbias) {
            const int RG = rowsum(prow0 + 2 * CB, CB / 2);
            for (int ch = threadIdx.x; ch < CB; ch += 256) coh_store(k.red + (size_t)k.nbatch * k.c * 2 + (size_t)n * k.c + c0 + ch, total(ch, CB / 2, RG));
        }
        for (int i = threadIdx.x; i < CB * 2; i += 256) coh_store(res + i, 0.f);
        if (threadIdx.x < SHM_FUSED_FLAGS + 2) coh_store(sy + 32 * threadIdx.x, 0u);
        // fold = 1: this launch also folds the staged bias gradient (no dbias_fold_kernel behind it); ferr[1] is the launch's group ticket
        if (k.dbias && k.fold) fused_fold_dbias(k.red + (size_t)k.nbatch * k.c * 2, k.dbias, ferr + 1, k.nbatch, k.c, gridDim.y * gridDim.z, &s_last);
    }
}

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

// Blocks of in_bwd_fused8_kernel<G2> the current device holds at once (CUs x occupancy; queried once per device and form).  The kernel's
// barrier only completes if a whole group is resident, and two such launches may run side by side (two streams), each stuck with LESS than a
// group resident only while free slots remain -- so a group is limited to HALF of this figure (advisor, round 5: a CPX partition, a CU mask or a
// smaller part holds far fewer than the 1024 / 768 blocks of a whole MI355X, and the launcher used to assume them).  0 if the query fails.
static int fused_resident_blocks(int form) {          // 0: in_bwd_fused8_kernel<false>, 1: <true> (pooled), 2: in_bwd_fusedg_kernel<2, 2, 4>, 3: <8, 8, 3>
    static int cache[16][4];                 // 0 = not asked yet, -1 = the query failed
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 16) return 0;
    int v = __atomic_load_n(&cache[dev][form], __ATOMIC_RELAXED);
    if (v == 0) {
        int cus = 0, per_cu = 0;
        hipError_t e = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
        if (e == hipSuccess)
            e = form == 1   ? hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, in_bwd_fused8_kernel<true>, 256, 0)
                : form == 0 ? hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, in_bwd_fused8_kernel<false>, 256, 0)
                : form == 2 ? hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, in_bwd_fusedg_kernel<2, 2, 4>, 256, 0)
                            : hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, in_bwd_fusedg_kernel<8, 8, 3>, 256, 0);
        if (e != hipSuccess) (void)hipGetLastError();
        v = (e == hipSuccess && cus > 0 && per_cu > 0) ? cus * per_cu : -1;
        __atomic_store_n(&cache[dev][form], v, __ATOMIC_RELAXED);
    }
    return v > 0 ? v : 0;
}

static int in_bwd_impl(const char* who, const void* g1, int ldg1, const void* g2, int ldg2, const float* r1_dz, const float* r1_w, const void* a, int lda,
                       const double* stats, double* red, void* dz, int lddz, double* dbias, double* keep, double* fscr, size_t fscr_n, unsigned* abort_dev,
                       unsigned* abort_host, int batch, int h, int w, int c, float slope, int dtype, void* stream) {
    const bool r1 = r1_dz != nullptr;
    SHM_REQUIRE(!keep || dbias, SHM_E_SHAPE, "%s: the per-sample dz sums are staged only with a bias gradient", who);
    SHM_CHECK_C(c, who);
    SHM_REQUIRE((r1 || ldg1 % 4 == 0) && lda % 4 == 0 && lddz % 4 == 0 && (!g2 || ldg2 % 4 == 0), SHM_E_SHAPE, "%s: bad pitch", who);
    SHM_REQUIRE(!g2 || (h % 2 == 0 && w % 2 == 0), SHM_E_SHAPE, "%s: pooled gradient needs even h,w", who);
    SHM_REQUIRE(!(r1 && g2), SHM_E_SHAPE, "%s: the rank-1 form takes no pooled gradient", who);
    if (batch == 0 || h * w == 0) return SHM_OK;
    hipStream_t st = (hipStream_t)stream;
    // `red` is zero on entry by contract and zero again on return (no memset in front of every launch)
    InBwdArgs k{g1, g2, a, stats, red, dz, dbias, ldg1, ldg2, lda, lddz, h, w, c, 0, slope, shm_tune(SHM_TUNE_ELEM_REVERSE), r1_dz, r1_w};
    const int hw = h * w;
    k.nbatch = batch;
    InBwdArgs kr = k;
    k.interleave = kr.interleave = shm_tune(SHM_TUNE_ELEM_INTERLEAVE);
    k.nt = shm_tune(SHM_TUNE_ELEM_NT);          // the apply pass is the last reader of g1
    const int rb = shm_tune(SHM_TUNE_ELEM_REDUCE_BLOCKS);
    // bf16 activations: the reduce pass with eight channels (16 bytes) per thread
    const bool wide8 = (dtype == SHM_BF16 || dtype == SHM_BF16_GF32) && c % 8 == 0 && c >= 8 && c <= 1024 && (r1 || ldg1 % 8 == 0) && lda % 8 == 0 &&
                       (!g2 || ldg2 % 8 == 0) && 256 / (c / 8) >= 1;
    // The one-pass form (in_bwd_fused8_kernel, "elem.fused_bwd"): bf16 tensors, barrier groups of (sample, CB = min(c, 64) channels), whole slices of
    // 16384 / CB pixels, at most "elem.fused_max_slices" (256) blocks per group; with a pooled gradient: 64-channel groups and whole tiles
    {
        const int cb = c < 64 ? c : 64;
        const bool cb_ok = c >= 8 && (c < 64 ? (c & (c - 1)) == 0 : c % 64 == 0);
        const int slice = cb_ok ? 16384 / cb : 1;
        // pooled form: tiles of (256 / Wt) rows x Wt = min(w, 128) columns
        const int wt = w < 128 ? w : 128;
        const bool g2_tiles = cb == 64 && wt >= 2 && (wt & (wt - 1)) == 0 && w % wt == 0 && 256 % wt == 0 && (256 / wt) % 2 == 0 && h % (256 / wt) == 0;
        const bool base_ok = fscr && shm_tune(SHM_TUNE_ELEM_FUSED_BWD) && dtype == SHM_BF16 && !r1 && cb_ok && c <= 1024 && ldg1 % 8 == 0 && lda % 8 == 0 &&
                             lddz % 8 == 0 && (!g2 || ldg2 % 8 == 0) && batch <= 65535 && fscr_n >= fused_scratch_doubles(batch, hw, c);
        const int max_slices = shm_tune(SHM_TUNE_ELEM_FUSED_MAX_SLICES);
        const int hold = shm_tune(SHM_TUNE_ELEM_FUSED_HOLD);          // 0 automatic, 1 the round-5 kernel only (g and a held), 2 the g-held kernel only
        const int ncb = c / cb;
        const size_t red_bytes = (size_t)batch * c * 3 * sizeof(double);
        k.fold = keep ? 0 : 1;             // (the per-sample sums are wanted too -- SHM_NORM_SCALED's second term: the separate fold kernel copies them out)
        // round 6: g held, a streamed twice; slices of 32768 / CB pixels (sixteen pixel slots per thread), half the blocks per group.  Groups of up
        // to 512 blocks where twice that fits the device (the 512 x 512 x 64 maps of BASELINE configs[3]): the knob's default 256 bounds the round-5
        // kernel, this one takes 2 x its value
        // Measured (tools/probes/in_bwd_fusedg_ab.py, n = 40 / 160): it wins where a group has many blocks -- 256 x 256 x 64: 287 -> 252 us, n = 160:
        // 1072 -> 879 us -- and loses on the smaller maps, whose short groups do not cover its two extra round trips (128 x 128 x 128: 122 -> 147 us):
        // automatic dispatch takes it from 256 slices of the 8-slot kind per group on.
        const int slice16 = 2 * slice;
        const int fgv = shm_tune(SHM_TUNE_ELEM_FUSED_GVARIANT);
        // the tail both one-pass forms share: `blocks` per group, scratch carved behind `rows` partial rows per group; then the bias-gradient fold
        const auto fused = [&](void (*kernel)(const InBwdArgs, float*, float*, unsigned*, unsigned*, unsigned*, unsigned*, const unsigned), const char* name,
                               int blocks, size_t rows) -> int {
            float* const fres = (float*)(fscr + fused_row_doubles(batch, rows, c));
            unsigned* const fsync = (unsigned*)(fres + (size_t)batch * c * 2);
            unsigned* const ferr = fsync + (size_t)batch * ncb * SHM_FUSED_SYNC_WORDS;
            const dim3 gridf(blocks, ncb, batch);
            const unsigned arrivals = gridf.x + (shm_tune(SHM_TUNE_ELEM_FUSED_TEST_STALL) ? 1u : 0u);
            hipLaunchKernelGGL(kernel, gridf, dim3(256), 0, st, k, (float*)fscr, fres, fsync, ferr, abort_dev, abort_host, arrivals);
            shm_set_last_kernel("%s", name);
            SHM_LAUNCH_CHECK_CLEAR("shm_in_bwd(fused)", red, red_bytes, st);
            if (dbias && !k.fold) {       // (the two sum planes in front of the staging were not used: nothing to clear)
                hipLaunchKernelGGL(dbias_fold_kernel, dim3(shm_cdiv(c, 64)), dim3(256), 0, st, red + (size_t)batch * c * 2, dbias, batch, c, (double*)nullptr, keep);
                SHM_LAUNCH_CHECK_CLEAR("shm_in_bwd(fold)", red, red_bytes, st);
            }
            return SHM_OK;
        };
        if (base_ok && hold != 1 && !g2 && hw % slice16 == 0 && (hold == 2 || hw / slice >= 256) && hw / slice16 <= 2 * max_slices &&
            2 * (hw / slice16) <= fused_resident_blocks(fgv == 1 ? 3 : 2)) {
            // ONE scratch layout for both kernels (the caller's buffer is "zero behind the partial rows" whichever kernel ran last): means, counters
            // and flags sit behind the rows region of the 16384 / CB-pixel slicing; this kernel's rows fill half of it
            return fused(fgv == 1 ? in_bwd_fusedg_kernel<8, 8, 3> : in_bwd_fusedg_kernel<2, 2, 4>,
                         fgv == 1 ? "in_bwd_fusedg_kernel<8, 8, 3>" : "in_bwd_fusedg_kernel<2, 2, 4>", hw / slice16, (size_t)hw * cb / 16384);
        }
        if (base_ok && hold != 2 && hw % slice == 0 && hw / slice <= max_slices && (!g2 || g2_tiles) && 2 * (hw / slice) <= fused_resident_blocks(g2 ? 1 : 0)) {
            return fused(g2 ? in_bwd_fused8_kernel<true> : in_bwd_fused8_kernel<false>, g2 ? "in_bwd_fused8_kernel<true>" : "in_bwd_fused8_kernel<false>",
                         hw / slice, hw / slice);
        }
    }
    // Sample chunks ("elem.chunk_mb", round 3): the apply pass re-reads what the reduce pass read.  On tensors larger than the 256 MiB
    // Infinity Cache that second read comes from HBM again (the back-to-front / front-to-back walk only saves the turning point);
    // run as reduce(chunk), apply(chunk) over chunks whose g + a fit the cache, the second read stays on die.  0 = one chunk.
    const int esz_a = dtype == SHM_F32 ? 4 : 2, esz_g = dtype == SHM_BF16 ? 2 : 4;
    const size_t per_sample = (size_t)hw * c * (esz_a + (r1 ? 0 : esz_g)) + (g2 ? (size_t)hw / 4 * c * esz_g : 0);
    const size_t chunk_bytes = (size_t)shm_tune(SHM_TUNE_ELEM_CHUNK_MB) << 20;
    int per_chunk = batch;
    if (chunk_bytes && per_sample * batch > chunk_bytes) {
        per_chunk = (int)(chunk_bytes / per_sample);
        if (per_chunk < 1) per_chunk = 1;
    }
    for (int n0 = 0; n0 < batch; n0 += per_chunk) {
        const int nb = min(per_chunk, batch - n0);
        k.n0 = kr.n0 = n0;
        // The reduce pass ends every block with an LDS combine and 2c f64 atomics onto the 2c addresses of its sample: with the
        // streaming pass's ~4096 blocks a sample's address takes up to 256 serialized adds (n = 8, 256 x 256: 125 us for a pass whose
        // data moves in 40) and the 512-channel maps issue 1.3 M atomics per launch.  Fewer, longer blocks -- about the same bytes per
        // block in both dtypes: bf16 step 27.8 -> 27.1 ms, fp32 123.4 -> 122.9.  (The apply pass, one atomic per channel and block, is faster with
        // its 4096 blocks: same grid for both measured +0.15 / +0.6 ms.)
        k.chunk = shm_cdiv(hw, pix_chunks(hw, nb, c, shm_tune(SHM_TUNE_ELEM_APPLY_BLOCKS)));
        kr.chunk = shm_cdiv(hw, pix_chunks(hw, nb, c, rb ? rb : (dtype == SHM_F32 ? 1024 : 512)));
        const dim3 grid(shm_cdiv(hw, k.chunk), nb), gridr(shm_cdiv(hw, kr.chunk), nb);
        if (wide8) {
            if (r1) {
                hipLaunchKernelGGL((in_bwd_reduce8_kernel<float, false, true>), gridr, dim3(256), 0, st, kr);
            } else if (dtype == SHM_BF16) {
                if (g2) hipLaunchKernelGGL((in_bwd_reduce8_kernel<bf16_t, true>), gridr, dim3(256), 0, st, kr);
                else hipLaunchKernelGGL((in_bwd_reduce8_kernel<bf16_t, false>), gridr, dim3(256), 0, st, kr);
            } else {
                if (g2) hipLaunchKernelGGL((in_bwd_reduce8_kernel<float, true>), gridr, dim3(256), 0, st, kr);
                else hipLaunchKernelGGL((in_bwd_reduce8_kernel<float, false>), gridr, dim3(256), 0, st, kr);
            }
        } else if (r1) {
            SHM_DISPATCH_G(dtype, who, hipLaunchKernelGGL((in_bwd_reduce_kernel<T, TG, false, true>), gridr, dim3(256), 0, st, kr));
        } else if (g2) {
            SHM_DISPATCH_G(dtype, who, hipLaunchKernelGGL((in_bwd_reduce_kernel<T, TG, true>), gridr, dim3(256), 0, st, kr));
        } else {
            SHM_DISPATCH_G(dtype, who, hipLaunchKernelGGL((in_bwd_reduce_kernel<T, TG, false>), gridr, dim3(256), 0, st, kr));
        }
        SHM_LAUNCH_CHECK("shm_in_bwd(reduce)");
        if (r1)
            SHM_DISPATCH_G(dtype, who, hipLaunchKernelGGL((in_bwd_apply_kernel<T, TG, false, true>), grid, dim3(256), 0, st, k));
        else if (g2)
            SHM_DISPATCH_G(dtype, who, hipLaunchKernelGGL((in_bwd_apply_kernel<T, TG, true>), grid, dim3(256), 0, st, k));
        else
            SHM_DISPATCH_G(dtype, who, hipLaunchKernelGGL((in_bwd_apply_kernel<T, TG, false>), grid, dim3(256), 0, st, k));
    }
    shm_set_last_kernel(wide8 ? "in_bwd_reduce8_kernel + in_bwd_apply_kernel" : "in_bwd_reduce_kernel + in_bwd_apply_kernel");
    const size_t red_bytes = (size_t)batch * c * 3 * sizeof(double);
    SHM_LAUNCH_CHECK_CLEAR("shm_in_bwd(apply)", red, red_bytes, st);
    if (dbias) {
        hipLaunchKernelGGL(dbias_fold_kernel, dim3(shm_cdiv(c, 64)), dim3(256), 0, st, red + (size_t)batch * c * 2, dbias, batch, c, red, keep);
    } else {
        int r = shm_zero(red, (size_t)batch * c * 2 * sizeof(double), stream);
        if (r) return r;
    }
    SHM_LAUNCH_CHECK_CLEAR("shm_in_bwd(fold)", red, red_bytes, st);
    return SHM_OK;
}

extern "C" int shm_in_bwd(const void* g1, int ldg1, const void* g2, int ldg2, const void* a, int lda,
                          const double* stats, double* red, void* dz, int lddz, double* dbias, double* dz_sums, double* fused_scratch,
                          size_t fused_doubles, unsigned* abort_dev, unsigned* abort_host, int batch, int h, int w, int c, float slope, int dtype,
                          void* stream) {
    SHM_REQUIRE(g1, SHM_E_SHAPE, "shm_in_bwd: null gradient");
    return in_bwd_impl("shm_in_bwd", g1, ldg1, g2, ldg2, nullptr, nullptr, a, lda, stats, red, dz, lddz, dbias, dz_sums, fused_scratch, fused_doubles, abort_dev,
                       abort_host, batch, h, w, c, slope, dtype, stream);
}

// InstanceNorm + LeakyReLU backward WITHOUT its reduce pass: the per-(sample, channel) sums were formed in the epilogues of the
// launches that wrote g1 / g2 (shm_conv2d_dgrad_gsum, shm_conv2d_fwd_gsum), so this is one pass over the tensors -- read g1 [+ g2],
// read a, write dz -- where shm_in_bwd makes two.
extern "C" int shm_in_bwd_apply(const void* g1, int ldg1, const void* g2, int ldg2, const void* a, int lda, const double* stats, const float* beta,
                                double* red, double* redp, double* dstage, void* dz, int lddz, double* dbias, double* keep, int batch, int h, int w, int c,
                                float slope, int dtype, void* stream) {
    const char* who = "shm_in_bwd_apply";
    SHM_REQUIRE(!keep || dbias, SHM_E_SHAPE, "%s: the per-sample dz sums are staged only with a bias gradient", who);
    SHM_REQUIRE(g1 && a && stats && red && dz, SHM_E_SHAPE, "%s: null pointer", who);
    SHM_REQUIRE((g2 != nullptr) == (redp != nullptr), SHM_E_SHAPE, "%s: the pooled gradient g2 and its sums redp come together", who);
    SHM_REQUIRE(!redp || beta, SHM_E_SHAPE, "%s: the pooled form needs beta", who);
    SHM_REQUIRE(!dbias || dstage, SHM_E_SHAPE, "%s: the bias gradient needs its staging scratch", who);
    SHM_CHECK_C(c, who);
    SHM_REQUIRE(ldg1 % 4 == 0 && lda % 4 == 0 && lddz % 4 == 0 && (!g2 || ldg2 % 4 == 0), SHM_E_SHAPE, "%s: bad pitch", who);
    SHM_REQUIRE(!g2 || (h % 2 == 0 && w % 2 == 0), SHM_E_SHAPE, "%s: pooled gradient needs even h,w", who);
    if (batch == 0 || h * w == 0) return SHM_OK;
    hipStream_t st = (hipStream_t)stream;
    InBwdArgs k{g1, g2, a, stats, nullptr, dz, dbias, ldg1, ldg2, lda, lddz, h, w, c, 0, slope, 0, nullptr, nullptr, red, redp, beta, dstage, SHM_GSUM_SLOTS,
                shm_tune(SHM_TUNE_ELEM_NT), 0, batch};
    k.interleave = shm_tune(SHM_TUNE_ELEM_INTERLEAVE);
    const int hw = h * w;
    k.chunk = shm_cdiv(hw, pix_chunks(hw, batch, c, shm_tune(SHM_TUNE_ELEM_APPLY_BLOCKS)));
    const dim3 grid(shm_cdiv(hw, k.chunk), batch);
    if (g2)
        SHM_DISPATCH_G(dtype, who, hipLaunchKernelGGL((in_bwd_apply_kernel<T, TG, true, false, true>), grid, dim3(256), 0, st, k));
    else
        SHM_DISPATCH_G(dtype, who, hipLaunchKernelGGL((in_bwd_apply_kernel<T, TG, false, false, true>), grid, dim3(256), 0, st, k));
    const size_t nred = (size_t)SHM_GSUM_SLOTS * batch * c * 2;
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) {
        const size_t nclr = (nred * (redp ? 2 : 1) + 2047) / 2048;
        int nb = nclr < 64 ? (int)nclr : 64;
        if (nb < shm_cdiv(c, 64)) nb = shm_cdiv(c, 64);
        hipLaunchKernelGGL(gsum_finish_kernel, dim3(nb), dim3(256), 0, st, dstage, dbias, batch, c, red, nred, redp, redp ? nred : (size_t)0, keep);
        e = hipGetLastError();
    }
    if (e != hipSuccess) {           // zero on return also on the error path
        (void)hipMemsetAsync(red, 0, nred * sizeof(double), st);
        if (redp) (void)hipMemsetAsync(redp, 0, nred * sizeof(double), st);
        if (dstage) (void)hipMemsetAsync(dstage, 0, (size_t)batch * c * sizeof(double), st);
        shm_set_error("%s: launch failed: %s", who, hipGetErrorString(e));
        return SHM_E_HIP;
    }
    return SHM_OK;
}

// The same backward for the block in front of the generator head, whose output gradient is the rank-1 tensor
// d_out[n, p, ch] = hdz[n * h * w + p] * hw_[ch] (shm_head_in_bwd's dz_out and the head kernel): formed on the fly, so the head
// never writes its input gradient and neither pass here reads it (three passes over the largest activation of the network).
extern "C" int shm_in_bwd_rank1(const float* hdz, const float* hw_, const void* a, int lda, const double* stats, double* red, void* dz, int lddz,
                                double* dbias, double* dz_sums, int batch, int h, int w, int c, float slope, int dtype, void* stream) {
    SHM_REQUIRE(hdz && hw_, SHM_E_SHAPE, "shm_in_bwd_rank1: null gradient");
    return in_bwd_impl("shm_in_bwd_rank1", nullptr, 0, nullptr, 0, hdz, hw_, a, lda, stats, red, dz, lddz, dbias, dz_sums, nullptr, 0, nullptr, nullptr, batch, h, w, c,
                       slope, dtype, stream);
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
        hipLaunchKernelGGL(dbias_fold_kernel, dim3(shm_cdiv(c, 64)), dim3(256), 0, (hipStream_t)stream, red, dbias, SHM_LRELU_RED_SLOTS, c, (double*)nullptr, (double*)nullptr);
        SHM_LAUNCH_CHECK_CLEAR("shm_lrelu_bwd(fold)", red, (size_t)SHM_LRELU_RED_SLOTS * c * sizeof(double), (hipStream_t)stream);
    }
    return SHM_OK;
}
