// wgrad_halo_kernel and wgrad_halo_thin_kernel: the fp32 3x3 weight gradient with an LDS halo patch (see conv_wgrad.hip's header comment).
#include "wgrad_halo_dev.h"

// ------------------------------------------------------------------------------------------
// 3x3 / stride-1 weight gradient with an LDS halo patch.
//
// A stage is a patch of 2 x 16 output pixels of one image.  Its 4 x 18 input halo (64 channels)
// and its 2 x 16 dY pixels are brought in ONCE by LDS-DMA (buffer_load ... lds, out-of-image
// pixels read as zeros through the descriptor range check); the nine taps are then nine shifted
// views of the same LDS image, i.e. only an immediate offset on the ds_read_b32 that feeds each
// MFMA.  Compared with fetching nine shifted tiles through L1 this moves 3x fewer bytes and
// needs ~5x fewer address instructions per MFMA.  Three stages, DMA two stages ahead, counted
// s_waitcnt vmcnt, raw s_barrier.  Work split: block = (64 ci, 64 co, slice of patches); wave w
// owns the 32x32 sub-tile (w>>1, w&1) of all nine taps; partial slabs as in wgrad_kernel.

// NM: a wave normalises the halo items it DMA'd itself, one stage ahead of their use.  A lane's four channels are the same for
// every item and patch (no swizzle in this image), so their (mean, inv, beta) live in registers and are re-read when the image
// changes (at most a few times per block).
// S2 (round 3; IS = conv stride 2): the stride-2 3x3 layers (SAME padding of an even map: no pad before, one row / column after).  A stage is a patch of
// 2 x 8 OUTPUT pixels and its 5 x 17 input halo -- 22 + 4 DMA items, the same 26 KiB stage, per-wave DMA counts and waits as the
// unit-stride form, with half the MFMAs per barrier; tap (kh, kw) of output pixel (qr, qc) is halo pixel (2 qr + kh, 2 qc + kw), still an
// immediate offset on the ds_read_b32 (a lane reads one float of a 128-byte run whatever the pixel stride: no bank conflicts).
// Against wgrad_kernel<9> (nine shifted tiles through registers, a barrier per 8 pixels): 5.3 input pixels fetched per output pixel
// instead of 9, no VGPR staging, no ds_write, a barrier per 16 pixels.
template <int NM = 0, bool S2 = false>
__global__ __launch_bounds__(256, 2) void wgrad_halo_kernel(const WgradHaloArgs a) {
    static_assert(!S2 || NM == 0, "norm: unit-stride form");
    constexpr int IS = S2 ? 2 : 1;
    constexpr int PW = IS == 1 ? 16 : 8, HC = IS * PW + 3 - IS, HR = 2 * IS + 3 - IS;    // patch 2 x 16, halo 4 x 18 | 2 x 8, 5 x 17
    constexpr int PAD = IS == 1 ? 1 : 0;
    constexpr int NHP = HR * HC, NPX = 2 * PW;          // 72 halo pixels, 32 output pixels | 85, 16
    constexpr int NXI = (NHP + 3) / 4, NDI = NPX / 4;   // DMA items (4 pixel rows each): 18 + 8 | 22 + 4
    constexpr int NXJ = (NXI + 3) / 4;                  // X items per wave, at most
    static_assert(NXI + NDI == 26, "26 items per stage: waves 0, 1 issue seven, waves 2, 3 six (wait_older)");
    constexpr int STAGE = (NXI + NDI) * 256;            // floats per stage
    constexpr int NST = 3;
    __shared__ __attribute__((aligned(1024))) float smem[NST * STAGE];
    typedef __attribute__((address_space(3))) void* lds_ptr;

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l31 = lane & 31, hh = lane >> 5;
    const int mi = wave >> 1, ni = wave & 1;
    // XCD-aware block order (round 3): the (ci, co) tiles of one patch slice share their x and dY tiles; dealt round-robin
    // over the eight XCDs every tile was fetched into eight L2s (r02 PMC: 1141 MB HBM-side per launch against ~530 MB of
    // operands, L2 hit rate 0.36); remapped, a slice's tiles run on one XCD
    const Blk3 blk = xcd_block_order();
    const int ci0 = blk.x * 64, co0 = blk.y * 64;
    const int pid0 = blk.z * a.patches_per_split;
    const int pid1 = min(a.npatch, pid0 + a.patches_per_split);
    const int nstages = pid1 - pid0;

    // DMA lane mapping: one instruction = 4 pixel rows x 64 channels; lane -> (pixel l>>4, c4 = l&15)
    const int dpx = lane >> 4, c4 = lane & 15;
    const bool second = ci0 >= a.c1;
    const int ldX = second ? a.ldx2 : a.ldx;
    const int cX = ci0 + c4 * 4;
    const bool xvalid = cX < a.cin_ld;
    const int ccX = second ? cX - a.c1 : cX;
    const int coD = co0 + c4 * 4;
    const bool dvalid = coD < a.cout;
    const __amdgpu_buffer_rsrc_t rsx = second ? __builtin_amdgcn_make_buffer_rsrc((void*)a.x2, 0, a.x2bytes, 0x00020000)
                                              : __builtin_amdgcn_make_buffer_rsrc((void*)a.x, 0, a.xbytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t rsd = __builtin_amdgcn_make_buffer_rsrc((void*)a.dy, 0, a.dybytes, 0x00020000);
    // items 0..17: halo rows [4i,4i+4); items 18..25: dY rows.  Wave w takes items w, w+4, ...
    // per-lane constants of the X items (j = 0..4): halo coordinates of this lane's pixel
    [[maybe_unused]] int hr[NXJ], hc[NXJ];                 // (NM: norm_x)
#pragma unroll
    for (int j = 0; j < NXJ; ++j) {
        const int hp = 4 * (wave + 4 * j) + dpx;
        hr[j] = hp / HC;
        hc[j] = hp - hr[j] * HC;
    }

    // running patch coordinate (block-uniform), in OUTPUT pixels (ho x wo = h / IS x w / IS)
    const int ho = a.h / IS, wo = a.w / IS;
    PatchWalk<2, PW> pw;
    pw.start(pid0, a.npatch, ho, wo);
    // DMA addressing, one v_add and one masked select per instruction: a lane's byte offset in item j is a per-lane constant plus the
    // patch origin, and whether its halo pixel lies outside the image depends only on which edges of the image the patch touches
    // (block-uniform, four bits) and on which edges of the halo the lane's pixel sits (per-lane constant, four bits per item; a fifth
    // marks lanes with nothing to fetch -- channel tail, tail of the last halo item -- and is always asked for).  (Until round 3 every
    // stage recomputed coordinates, range tests and exec-masked selects per item: ~450 instructions between the barrier and the
    // stage's first MFMA.)  The LDS destination is item * 1 KiB for both kinds of item (the dY rows follow the halo); descriptor and
    // origin are scalar selects.
    unsigned off0[7], bma = 0, bmb = 0;
#pragma unroll
    for (int j = 0; j < 7; ++j) {
        const int item = wave + 4 * j;
        unsigned bits;
        if (item < NXI) {
            const int hp = 4 * item + dpx;
            const int r = hp / HC, c = hp - r * HC;
            off0[j] = (unsigned)((r * a.w + c) * ldX + ccX) * 4u;
            bits = !(xvalid && hp < NHP) ? 16u : halo_pixel_bits(r, c, HR - 1, HC - 1, PAD);
        } else {
            const int q = 4 * (item - NXI) + dpx;
            off0[j] = (unsigned)(((q / PW) * (a.w / IS) + q % PW) * a.lddy + coD) * 4u;
            bits = (dvalid && item < NXI + NDI) ? 0u : 16u;
        }
        if (j < 4)
            bma |= bits << (8 * j);
        else
            bmb |= bits << (8 * (j - 4));
    }
    auto dma = [&](int stage) {
        float* sx = smem + stage * STAGE;
        const int org = (pw.n * a.h + IS * pw.pr - PAD) * a.w + (IS * pw.pc - PAD);       // pixel index of halo (0,0)
        const unsigned edges = pw.template edges<PAD != 0>(ho, wo);
        const unsigned xb = (unsigned)(org * ldX) * 4u, db = (unsigned)(((pw.n * ho + pw.pr) * wo + pw.pc) * a.lddy) * 4u;
#pragma unroll
        for (int j = 0; j < 7; ++j) {
            const int item = wave + 4 * j;
            if (j < 6 || wave < 2) {
                const bool isx = item < NXI;                   // wave-uniform
                const unsigned out = (j < 4 ? bma : bmb) & (edges << (8 * (j & 3)));
                const unsigned off = out ? 0xffffffffu : off0[j] + (isx ? xb : db);
                __builtin_amdgcn_raw_ptr_buffer_load_lds(isx ? rsx : rsd, (lds_ptr)(sx + item * 256), 16, (int)off, 0, 0, 0);
            }
        }
        pw.next(ho, wo);
    };

    // NM: coordinates of the next stage to normalise (they run one stage behind dma()'s), the lane's table entries and their image
    const bool nm_on = NM && a.nt != nullptr && (int)second == a.ntpart;        // block-uniform
    [[maybe_unused]] PatchWalk<2, PW> pw2 = pw;
    [[maybe_unused]] int nimg = -1;
    [[maybe_unused]] f32x4 nmean = {0.f, 0.f, 0.f, 0.f}, ninv = nmean, nbeta = nmean;
    // One straight-line piece per stage (interior patches: no per-lane tests).
    const int n_blk = pw.n;                                    // NM = 2: the sample of this block's patches
    [[maybe_unused]] auto norm_x = [&](int stage) {
        if (pw2.n != nimg) {                                   // block-uniform
            nimg = pw2.n;
            if (xvalid) {
                const float* t = a.nt + (size_t)pw2.n * SHM_NT_PLANES * a.ntc + ccX;
                if constexpr (NM == 2) {
                    nbeta = load16_drained(t + 3 * a.ntc);              // ring
                } else {
                    nmean = load16_drained(t);
                    ninv = load16_drained(t + a.ntc);
                    nbeta = load16_drained(t + 2 * a.ntc);
                }
            }
        }
        float* sx = smem + stage * STAGE + lane * 4;
        if constexpr (NM == 2) {
            // SHM_NORM_SCALED: `ring` over the out-of-image halo entries of a border patch; nothing to do inside the image
            if (!pw2.interior(a.h, a.w)) {
#pragma unroll
                for (int j = 0; j < 5; ++j) {
                    const int item = wave + 4 * j;
                    if (item < 18) {
                        const int iy = pw2.pr - 1 + hr[j], ix = pw2.pc - 1 + hc[j];
                        if (xvalid && !((unsigned)iy < (unsigned)a.h && (unsigned)ix < (unsigned)a.w)) *(f32x4*)(sx + item * 256) = nbeta;
                    }
                }
            }
        } else
        // interior patch (the whole 4 x 18 halo inside the image) of a full 64-channel tile: every lane of every item normalises, no
        // per-lane tests -- block-uniform, 7 of 8 patches of a 256 x 256 map
        if (pw2.interior(a.h, a.w) && ci0 + 64 <= a.cin_ld) {
            f32x4 x[5];
#pragma unroll
            for (int j = 0; j < 4; ++j) x[j] = *(const f32x4*)(sx + (wave + 4 * j) * 256);
            if (wave < 2) x[4] = *(const f32x4*)(sx + (wave + 16) * 256);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
#pragma unroll
                for (int e = 0; e < 4; ++e) x[j][e] = shm_in_norm(x[j][e], nmean[e], ninv[e], nbeta[e]);
                *(f32x4*)(sx + (wave + 4 * j) * 256) = x[j];
            }
            if (wave < 2) {
#pragma unroll
                for (int e = 0; e < 4; ++e) x[4][e] = shm_in_norm(x[4][e], nmean[e], ninv[e], nbeta[e]);
                *(f32x4*)(sx + (wave + 16) * 256) = x[4];
            }
        } else {
#pragma unroll
            for (int j = 0; j < 5; ++j) {
                const int item = wave + 4 * j;
                if (item < 18) {
                    const int iy = pw2.pr - 1 + hr[j], ix = pw2.pc - 1 + hc[j];
                    if (xvalid && (unsigned)iy < (unsigned)a.h && (unsigned)ix < (unsigned)a.w) {
                        f32x4 x = *(const f32x4*)(sx + item * 256);
#pragma unroll
                        for (int e = 0; e < 4; ++e) x[e] = shm_in_norm(x[e], nmean[e], ninv[e], nbeta[e]);
                        *(f32x4*)(sx + item * 256) = x;
                    }
                }
            }
        }
        pw2.next(a.h, a.w);
    };

    f32x16 acc[9];
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;

    const int xl = hh * 64 * IS + mi * 32 + l31;  // + ((IS*qr+kh)*HC + IS*qc + kw)*64, qc even part
    const int dl = hh * 64 + ni * 32 + l31;       // + 2*kk*64
    auto compute = [&](int stage) {
        const float* X = smem + stage * STAGE + xl;
        const float* D = smem + stage * STAGE + NXI * 256 + dl;
#pragma unroll
        for (int kk = 0; kk < NPX / 2; ++kk) {
            const int qr = kk / (PW / 2), qc = 2 * (kk % (PW / 2));
            const float bv = D[kk * 128];
#pragma unroll
            for (int t = 0; t < 9; ++t) {
                const float av = X[((IS * qr + t / 3) * HC + IS * qc + t % 3) * 64];
                acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv, acc[t], 0, 0, 0);
            }
        }
    };

    // wait until this wave's DMA items of every stage but the youngest one in flight have landed
    auto wait_older = [&](bool younger_in_flight) {
        if (younger_in_flight) {
            if (wave < 2)
                asm volatile("s_waitcnt vmcnt(7)" ::: "memory");
            else
                asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
        } else {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
    };
    wgrad_stage_ring<NST, NM != 0>(nstages, nm_on, dma, compute, wait_older, norm_x);

    // NM = 2: the slab's rows times inv of the block's sample
    float sc[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) sc[r] = 1.f;
    if constexpr (NM == 2)
        if (nm_on) wgrad_row_scale(sc, a.nt + ((size_t)n_blk * SHM_NT_PLANES + 1) * a.ntc + (ci0 - (second ? a.c1 : 0)) + mi * 32 + 4 * hh);
    wgrad_store_slab<9, NM == 2>(acc, a.part + (size_t)blk.z * 9 * a.cin * a.cout, a.cin, a.cout, ci0, mi, hh, co0 + ni * 32 + l31, sc);
}

// ------------------------------------------------------------------------------------------
// Thin-input variant of wgrad_halo_kernel (fp32, 3x3, 9*cin <= 96: the generator's 10-channel and the
// discriminator's 3-channel first layers).  The general kernels give every tap its own 64-row ci tile, of which
// 10 (3) rows are real (22 / 6 TFLOP/s, 2.6 ms per step).  Here the (tap, ci) pairs are PACKED into the MFMA rows --
// row r holds (tap r / cin, ci r % cin) -- which only changes the per-lane offset of the ds_read_b32 into the same
// LDS halo image (16 floats = one 64-byte row per halo pixel).  IS = conv stride: the halo of a 2 x 16 output patch
// is 4 x 18 input pixels at stride 1 (SAME pad 1 before) and 5 x 33 at stride 2 (pad 0 before).  Wave w takes column
// tile w & 1 and patch row w >> 1; the two patch rows write separate split-K slabs.
template <int NRT, int IS>
__global__ __launch_bounds__(256, 2) void wgrad_halo_thin_kernel(const WgradHaloArgs a) {
    constexpr int PW = 16, XP = 16;
    constexpr int HR = 2 * IS + 3 - IS, HC = PW * IS + 3 - IS, PAD = IS == 1 ? 1 : 0;
    constexpr int NHP = HR * HC, NPX = 2 * PW;
    constexpr int NXI = (NHP * XP * 4 + 1023) / 1024;    // DMA items (1 KiB = 16 halo pixels) for the halo; 8 more for dY
    constexpr int XF = NXI * 256;                        // halo region padded to whole items
    constexpr int STAGE = XF + NPX * 64;                 // floats
    constexpr int NST = 3;
    constexpr int NIT = NXI + 8, CHI = (NIT + 3) / 4, CLO = NIT / 4, NHI = NIT % 4;   // items per wave: CHI for waves < NHI
    __shared__ __attribute__((aligned(1024))) float smem[NST * STAGE];
    typedef __attribute__((address_space(3))) void* lds_ptr;

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l31 = lane & 31, hh = lane >> 5;
    const int ni = wave & 1, qr = wave >> 1;
    const int co0 = blockIdx.y * 64;
    const int pid0 = blockIdx.z * a.patches_per_split;
    const int pid1 = min(a.npatch, pid0 + a.patches_per_split);
    const int nstages = pid1 - pid0;
    const int ho = a.h / IS, wo = a.w / IS;

    const __amdgpu_buffer_rsrc_t rsx = __builtin_amdgcn_make_buffer_rsrc((void*)a.x, 0, a.xbytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t rsd = __builtin_amdgcn_make_buffer_rsrc((void*)a.dy, 0, a.dybytes, 0x00020000);
    // X items: lane -> (halo pixel 16 i + (l >> 2), 4-float chunk l & 3); D items: lane -> (pixel 4 j + (l >> 4), chunk l & 15)
    const int xpx = lane >> 2, xch = lane & 3;
    const bool xcv = xch * 4 < a.cin_ld;
    const int dpx = lane >> 4, dch = lane & 15;
    const int coD = co0 + dch * 4;
    const bool dvalid = coD < a.cout;

    int n, pr, pc;                                       // patch origin in OUTPUT pixels; the one kernel that walks ALONG the rows (not PatchWalk's order)
    {
        const int ppr = wo / PW, ppi = (ho / 2) * ppr;
        const int p = pid0 < a.npatch ? pid0 : 0;
        n = p / ppi;
        const int r = p - n * ppi;
        pr = (r / ppr) * 2;
        pc = (r % ppr) * PW;
    }
    auto dma = [&](int stage) {
        float* sx = smem + stage * STAGE;
        float* sd = sx + XF;
        const int y0 = IS * pr - PAD, x0 = IS * pc - PAD;       // input pixel of halo (0,0)
#pragma unroll
        for (int j = 0; j < CHI; ++j) {
            const int item = wave + 4 * j;
            if (item < NXI) {
                const int hp = 16 * item + xpx;
                const int hr = hp / HC, hc = hp - hr * HC;
                const int iy = y0 + hr, ix = x0 + hc;
                const bool v = xcv && hp < NHP && (unsigned)iy < (unsigned)a.h && (unsigned)ix < (unsigned)a.w;
                const unsigned off = v ? (unsigned)(((n * a.h + iy) * a.w + ix) * a.ldx + xch * 4) * 4u : 0xffffffffu;
                __builtin_amdgcn_raw_ptr_buffer_load_lds(rsx, (lds_ptr)(sx + item * 256), 16, (int)off, 0, 0, 0);
            } else if (item < NIT) {
                const int q = 4 * (item - NXI) + dpx;
                const int oy = pr + (q >> 4), ox = pc + (q & 15);
                const unsigned off = dvalid ? (unsigned)(((n * ho + oy) * wo + ox) * a.lddy + coD) * 4u : 0xffffffffu;
                __builtin_amdgcn_raw_ptr_buffer_load_lds(rsd, (lds_ptr)(sd + (item - NXI) * 256), 16, (int)off, 0, 0, 0);
            }
        }
        pc += PW;
        if (pc == wo) {
            pc = 0;
            pr += 2;
            if (pr == ho) {
                pr = 0;
                ++n;
            }
        }
    };

    f32x16 acc[NRT];
#pragma unroll
    for (int t = 0; t < NRT; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;

    // packed rows: lane's row of row-tile rt is (tap, ci) = divmod(rt*32 + l31, cin); rows >= 9*cin read a valid
    // address and are never stored
    const int rows = 9 * a.cin;
    int xoff[NRT];
#pragma unroll
    for (int rt = 0; rt < NRT; ++rt) {
        const int idx = rt * 32 + l31;
        const int tap = idx < rows ? idx / a.cin : 0, ci = idx < rows ? idx - tap * a.cin : 0;
        xoff[rt] = ((tap / 3) * HC + tap % 3) * XP + ci;
    }
    const int xb = (IS * qr * HC + IS * hh) * XP;         // + IS*2*kk*XP
    const int db = (qr * PW + hh) * 64 + ni * 32 + l31;   // + 2*kk*64
    auto compute = [&](int stage) {
        const float* X = smem + stage * STAGE + xb;
        const float* D = smem + stage * STAGE + XF + db;
#pragma unroll
        for (int kk = 0; kk < PW / 2; ++kk) {
            const float bv = D[kk * 128];
#pragma unroll
            for (int rt = 0; rt < NRT; ++rt) {
                const float av = X[kk * 2 * IS * XP + xoff[rt]];
                acc[rt] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv, acc[rt], 0, 0, 0);
            }
        }
    };

    auto wait_older = [&](bool younger_in_flight) {
        if (younger_in_flight) {                   // one younger stage in flight: CHI or CLO DMA instructions of this wave
            if (NHI != 0 && wave < NHI)
                asm volatile("s_waitcnt vmcnt(%0)" ::"n"(CHI) : "memory");
            else
                asm volatile("s_waitcnt vmcnt(%0)" ::"n"(CLO) : "memory");
        } else {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
    };
    wgrad_stage_ring<NST, false>(nstages, false, dma, compute, wait_older, [](int) {});

    float* out = a.part + ((size_t)blockIdx.z * 2 + qr) * 9 * a.cin * a.cout;
    const int con = co0 + ni * 32 + l31;
#pragma unroll
    for (int rt = 0; rt < NRT; ++rt) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int idx = rt * 32 + (r & 3) + 8 * (r >> 2) + 4 * hh;       // = tap*cin + ci
            if (idx < rows && con < a.cout) out[(size_t)idx * a.cout + con] = acc[rt][r];
        }
    }
}

template <int NM, bool S2 = false>
static void halo_launch(const WgradHaloArgs& a, const WgradPlan& p, hipStream_t st) {
    hipLaunchKernelGGL((wgrad_halo_kernel<NM, S2>), dim3(shm_cdiv(a.cin, 64), shm_cdiv(a.cout, 64), p.splits), dim3(256), 0, st, a);
    shm_set_last_kernel(S2 ? "wgrad_halo_kernel<0, true>" : NM == 2 ? "wgrad_halo_kernel<2>" : NM == 1 ? "wgrad_halo_kernel<1>" : "wgrad_halo_kernel");
}

// two slabs per block (one per patch row)
template <int NRT, int IS>
static void thin_launch(const WgradHaloArgs& a, const WgradPlan& p, hipStream_t st) {
    hipLaunchKernelGGL((wgrad_halo_thin_kernel<NRT, IS>), dim3(1, shm_cdiv(a.cout, 64), p.splits), dim3(256), 0, st, a);
    shm_set_last_kernel("wgrad_halo_thin_kernel<%d, %d>", NRT, IS);
}

int shm_wgrad_halo_launch(const WgradHaloArgs& a, const WgradPlan& p, hipStream_t st) {
    if (p.family == SHM_WG_THIN) {
        if (p.thin_is == 1)
            thin_launch<3, 1>(a, p, st);
        else if (p.thin_nrt == 1)
            thin_launch<1, 2>(a, p, st);
        else
            thin_launch<3, 2>(a, p, st);
    } else if (p.stride2)
        halo_launch<0, true>(a, p, st);
    else if (p.nmode == 2)
        halo_launch<2>(a, p, st);
    else if (p.nmode == 1)
        halo_launch<1>(a, p, st);
    else
        halo_launch<0>(a, p, st);
    return SHM_OK;
}
