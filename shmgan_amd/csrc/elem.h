// Helpers shared by the HBM-bound kernels around the convolutions (elem.hip, instnorm.hip, the InstanceNorm-backward
// families behind in_bwd.h -- instnorm_bwd_2pass.hip, instnorm_bwd_fused8.hip, instnorm_bwd_fusedg.hip, grad_sums.hip --, heads.hip, dgrad_sum1.hip).
//
// Layout: NHWC with a channel pitch; every thread moves 16 bytes (4 channels of one
// pixel); a block covers PP = 256/(C/4) pixels per iteration, so a wave reads whole
// contiguous channel rows.  Per-(sample,channel) sums are accumulated in fp64 per thread,
// combined through LDS and added with one f64 atomic per (block, channel).
#pragma once
#include "common.h"

// ------------------------------------------------------------------ pixel-chunk skeleton
// thread -> (pp, cl): pixel slot and 4-channel lane.  PP pixel slots per block iteration.
struct PixMap {
    int lanes_c, PP, pp, cl;
    bool active;
    __device__ PixMap(int c) {
        lanes_c = c >> 2;
        PP = 256 / lanes_c;
        pp = threadIdx.x / lanes_c;
        cl = threadIdx.x - pp * lanes_c;
        active = pp < PP;
    }
};

// blocks = 0: the target of the passes without a per-block prologue or reduction (InstanceNorm apply, its pooling forms),
// "elem.stream_blocks", default 32768: short blocks keep the addresses in flight a narrow band that sweeps through the tensors
// (tools/probes/elem_probe.hip: a 2-read / 1-write pass over 3 x 671 MB runs at 5.5 TB/s with 4k blocks of 160 KB each and at 7.0 TB/s with
// 16k blocks of 40 KB; shm_in_apply on the same tensor 5.16 -> 5.85 TB/s in fp32, 5.24 -> 6.01 in bf16).  The passes that start with
// a per-block prologue and end in an LDS reduction + atomics (InstanceNorm backward) keep 4096: they get SLOWER with more blocks.
static inline int pix_chunks(long npix_per_sample, int batch, int c, int blocks = 0) {
    // enough blocks to fill the chip, but at least 8 (streaming target) / 16 pixel iterations per thread so the
    // per-block LDS reduction + f64 atomics (one per channel and block) stay a small fraction
    if (blocks == 0) blocks = shm_tune(SHM_TUNE_ELEM_STREAM_BLOCKS);
    const int min_iter = blocks > 4096 ? 8 : 16;
    int lanes_c = c / 4;
    int PP = 256 / lanes_c;
    long want = (blocks + batch - 1) / batch;
    long maxc = npix_per_sample / ((long)PP * min_iter);
    if (want > maxc) want = maxc;
    if (want < 1) want = 1;
    return (int)want;
}

#define SHM_CHECK_C(c, who) SHM_REQUIRE((c) % 4 == 0 && (c) >= 4 && (c) <= 1024, SHM_E_SHAPE, "%s: channels %d must be a multiple of 4 in [4,1024]", who, (c))

// Combine per-thread double[NV][4] partials over the PP pixel slots, then one atomic per
// (channel, value).  dst index = base + (ch * NV + v) when interleaved, or v*c + ch otherwise.
template <int NV>
__device__ __forceinline__ void block_reduce_atomic(double (&v)[NV][4], const PixMap& pm, double* dst, int c, bool interleaved) {
    __shared__ double red[256 * 4];
    for (int q = 0; q < NV; ++q) {
        __syncthreads();
        if (pm.active) {
#pragma unroll
            for (int e = 0; e < 4; ++e) red[(pm.pp * pm.lanes_c + pm.cl) * 4 + e] = v[q][e];
        }
        __syncthreads();
        if (pm.active && pm.pp == 0) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                double s = 0.0;
                for (int p = 0; p < pm.PP; ++p) s += red[(p * pm.lanes_c + pm.cl) * 4 + e];
                int ch = pm.cl * 4 + e;
                if (ch < c) atomicAdd(&dst[interleaved ? ch * NV + q : q * c + ch], s);
            }
        }
    }
}

static inline bool pow2_le64(int v) { return v >= 1 && v <= 64 && (v & (v - 1)) == 0; }
