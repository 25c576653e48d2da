// Device pieces the halo-staged weight-gradient kernels share (conv_wgrad_halo.hip, conv_wgrad_halo16.hip, conv_wgrad_halo8.hip,
// conv_wgrad_x3.hip): the order a block walks its patches in, the edge bits of a patch and of a halo pixel, the even / odd-run image of
// the stride-2 forms, the transposed-read addresses of the bf16-MFMA kernels and the three-stage DMA ring.  Only forceinline templates
// and constexpr structs: no state, no translation unit of its own.  (The slab epilogue is wgrad.h's: conv_wgrad_gen.hip stores the same slab.)
#pragma once
#include "wgrad.h"

// The running patch of a block (block-uniform): sample n and origin (pr, pc) of a patch of R x PW pixels, in OUTPUT pixels of an
// ho x wo map.  The host plan (conv_wgrad.hip: prow, pcol, npatch) counts the same patches.
// Patches are numbered DOWN the columns of an image (round 4; until then along the rows): a block walks a contiguous range, and the
// halos of vertically adjacent patches share two of their four rows (half the halo) where horizontally adjacent ones share two of
// eighteen columns -- walking down, the shared rows were fetched one stage ago (L2 / L1 hits), walking along, 16 stages and a few
// hundred KiB per resident block ago, i.e. from beyond L2 (r03: 1291 MB HBM-side per launch for 805 MB of operands, L2 hit 0.19)
template <int R, int PW>
struct PatchWalk {
    int n, pr, pc;

    __device__ __forceinline__ void start(int pid, int npatch, int ho, int wo) {
        const int ppc = ho / R, ppi = ppc * (wo / PW);
        const int p = pid < npatch ? pid : 0;
        n = p / ppi;
        const int r = p - n * ppi;
        pc = (r / ppc) * PW;
        pr = (r % ppc) * R;
    }
    __device__ __forceinline__ void next(int ho, int wo) {
        pr += R;
        if (pr == ho) {
            pr = 0;
            pc += PW;
            if (pc == wo) {
                pc = 0;
                ++n;
            }
        }
    }
    // which edges of the image the patch touches: 1 top, 2 bottom, 4 left, 8 right, and 16, which is always asked for (a per-item mask
    // sets it for lanes with nothing to fetch).  PAD = false: SAME padding of an even map at stride 2 -- nothing before the first row /
    // column, so no halo pixel lies above or left of the image
    template <bool PAD>
    __device__ __forceinline__ unsigned edges(int ho, int wo) const {
        return 16u | ((PAD && pr == 0) ? 1u : 0u) | (pr + R == ho ? 2u : 0u) | ((PAD && pc == 0) ? 4u : 0u) | (pc + PW == wo ? 8u : 0u);
    }
    // the whole halo of the (unit-stride) patch lies inside the h x w image
    __device__ __forceinline__ bool interior(int h, int w) const { return pr > 0 && pr + R < h && pc > 0 && pc + PW < w; }
};

// On which edges of the halo a lane's pixel (r, c) sits, in the bits of PatchWalk::edges: the pixel lies outside the image exactly when
// the patch touches that edge of the image (mask & edges != 0).  pad = false: the halo has no row / column before the patch
__device__ __forceinline__ unsigned halo_pixel_bits(int r, int c, int r_last, int c_last, bool pad) {
    return ((pad && r == 0) ? 1u : 0u) | (r == r_last ? 2u : 0u) | ((pad && c == 0) ? 4u : 0u) | (c == c_last ? 8u : 0u);
}

// Stride-2 halo image: a halo row is HRP LDS rows, [PW + 1 even input columns | unused up to HP | PW odd columns], so that the sixteen
// (eight) pixels of a K step are consecutive LDS rows for every kw (wgrad_halo8_bf16_kernel's header comment).  LDS row -> halo pixel
// (r, c); ok = false for the unused rows of the even run
struct S2RunPixel {
    int r, c;
    bool ok;
};
template <int HRP, int HP, int PW>
__device__ __forceinline__ S2RunPixel s2_run_pixel(int row) {
    S2RunPixel p;
    p.r = row / HRP;
    const int t = row - p.r * HRP;
    p.c = t < HP ? 2 * t : 2 * (t - HP) + 1;
    p.ok = t < HP ? t <= PW : true;
    return p;
}

// Transposed-read addresses (bf16 elements) of the bf16-MFMA kernels: the lane supplies row 8 hh + (i >> 2) [+ 4 for the second read of
// tr_frag] and channels [32 tile + 16 (g & 1) + 4 (i & 3), + 4) of rows of 64 channels whose halves are swapped where bit 1 of the row
// index is set.  Tap (kh, kw) and K step enter as immediates, except that at unit stride kw shifts the row and with it bit 1 of the row
// index: one address per kw.  S2: kw = 0 / 2 read the even run (2 = one row on), kw = 1 the odd run HP rows further (same bit 1:
// HP % 4 == 0).  HH2: a K step is two output rows of eight pixels, so the lane half hh sits two halo rows (2 HRP LDS rows, 0 mod 4)
// further down in the x image instead of eight rows further on.  fa is relative to the x image, fb0 is where the wave's dY image (rows in
// pixel order) begins.
template <bool S2, int HP, int HRP, bool HH2 = false>
__device__ __forceinline__ void wgrad_tr_addrs(int lane, int mi, int ni, int fb0, int (&fa)[3], int& fb) {
    static_assert(HP % 4 == 0 && (!HH2 || (2 * HRP) % 4 == 0), "bit 1 of the row index");
    const int hh = lane >> 5;
    const int fq = 8 * hh + ((lane & 15) >> 2);                          // pixel of the K step this lane supplies
    const int fqx = (HH2 ? 2 * HRP * hh : 8 * hh) + ((lane & 15) >> 2);  // ... and its row in the x image
    const int fcol = 16 * ((lane >> 4) & 1) + 4 * (lane & 3);
#pragma unroll
    for (int kw = 0; kw < 3; ++kw) {
        const int row = fqx + (S2 ? (kw == 2 ? 1 : 0) : kw);
        fa[kw] = row * 64 + ((mi * 32 + fcol) ^ (((row >> 1) & 1) << 5)) + ((S2 && kw == 1) ? HP * 64 : 0);
    }
    fb = fb0 + fq * 64 + ((ni * 32 + fcol) ^ (((fq >> 1) & 1) << 5));
}

// The ring of NST LDS stages, DMA two stages ahead: dma(stage) issues the next patch's LDS-DMA into a stage, wait_older(younger) waits
// until this wave's DMA items of every stage but the youngest one in flight (if any) have landed, compute(stage) is the stage's MFMA
// loop, norm_x(stage) (NM) normalises in LDS the halo items this wave DMA'd itself.
template <int NST, bool NM, typename Dma, typename Compute, typename WaitOlder, typename NormX>
__device__ __forceinline__ void wgrad_stage_ring(int nstages, bool nm_on, Dma&& dma, Compute&& compute, WaitOlder&& wait_older, NormX&& norm_x) {
    static_assert(NST == 3, "two stages in flight behind the one computed");
    if (nstages > 0) {
        dma(0);
        if (nstages > 1) dma(1);
        if constexpr (NM)
            if (nm_on) {
                wait_older(nstages > 1);
                norm_x(0);
            }
        int cur = 0, nxt2 = 2;
        for (int s = 0; s < nstages; ++s) {
            wait_older(s + 1 < nstages);
            SHM_LDS_BARRIER();
            asm volatile("" ::: "memory");
            if (s + 2 < nstages) dma(nxt2);
            compute(cur);
            asm volatile("" ::: "memory");
            cur = (cur == NST - 1) ? 0 : cur + 1;
            nxt2 = (nxt2 == NST - 1) ? 0 : nxt2 + 1;
            // NM: stage s + 1 (issued before the stage in flight): every wave normalises its own items of it behind this stage's last
            // MFMA (issued, not finished: they and the partner block's keep the matrix pipe busy); the barrier of step s + 1 publishes
            // them.  The MFMA loop itself stays the plain kernel's: with the normalisation inside it (one piece at K step 8, or an
            // item per K step) the loop falls into basic blocks -- 47-63 s_waitcnt instead of 20, +5-7 % on the kernel even for
            // blocks that normalise nothing.  Timing-only builds: with the normalisation removed and the wait kept the kernel is as
            // fast as the plain one (+0.2-0.5 %); the pass itself costs 3-6 % -- its read / fma / write chain (~500 cycles per
            // 9216-cycle stage) is serial in every wave at the same time, and the two blocks of a CU run in lockstep.
            if constexpr (NM)
                if (nm_on && s + 1 < nstages) {
                    wait_older(s + 2 < nstages);
                    norm_x(cur);
                    asm volatile("" ::: "memory");
                }
        }
    }
}
