// The one-pass bf16 InstanceNorm backward that holds g and a (in_bwd_fused8_kernel), behind shm_in_bwd_fused8_launch.  Which calls take it:
// in_bwd_plan (instnorm_bwd.hip).  Scratch layout and the helpers shared with in_bwd_fusedg_kernel: in_bwd.h.
#include "in_bwd.h"

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

void shm_in_bwd_fused8_launch(const InBwdArgs& k, bool g2, const InBwdFusedScratch& s, unsigned* abort_dev, unsigned* abort_host, dim3 grid, unsigned arrivals,
                              hipStream_t st) {
    const auto kernel = g2 ? in_bwd_fused8_kernel<true> : in_bwd_fused8_kernel<false>;
    hipLaunchKernelGGL(kernel, grid, dim3(256), 0, st, k, s.part, s.res, s.sync, s.err, abort_dev, abort_host, arrivals);
}

hipError_t shm_in_bwd_fused8_occupancy(bool g2, int* per_cu) {
    return g2 ? hipOccupancyMaxActiveBlocksPerMultiprocessor(per_cu, in_bwd_fused8_kernel<true>, 256, 0)
              : hipOccupancyMaxActiveBlocksPerMultiprocessor(per_cu, in_bwd_fused8_kernel<false>, 256, 0);
}
