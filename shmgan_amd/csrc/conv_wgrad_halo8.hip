// wgrad_halo8_bf16_kernel: the eight-wave bf16 3x3 weight gradient, unit stride and stride 2 (see conv_wgrad.hip's header comment).
#include "wgrad_halo_dev.h"

// ------------------------------------------------------------------------------------------
// Round 4: the bf16 halo weight gradient as an EIGHT-wave block that owns 64 input channels x 128 output channels -- two
// 64 x 64 tiles that share one x halo image -- for unit stride (S2 = false: stages of 4 x 16 output pixels, the LDS image of
// wgrad_halo_bf16_kernel<4>) and for stride 2 (S2 = true: the 3x3 / stride-2 convolutions and, with the roles of x and dY swapped,
// Conv2DTranspose; stages of 2 x 16 output pixels).
//
// Why: with the split-K target the two-stream step wants (256 blocks: every slab is 9 * cin * cout floats written and read again,
// 45-90 % of the operand bytes on the deep layers) the four-wave kernel runs ONE block = one wave per SIMD on a CU, and a wave's
// DMA issue, fragment reads and MFMAs are then serial (MFMA busy 0.34 against 0.56 with two blocks per CU).  Here a CU holds two
// waves per SIMD at the same number of slabs, and the two co tiles share the x halo -- the larger part of a stage (15 of 23 KiB):
// 31 DMA items per 72 wave-MFMAs instead of 46, and x is fetched from L2 / HBM once for 128 output channels.
//
// Stride 2 (SAME padding of an even map: nothing before the first row / column, one after the last): output pixel (qr, qc), tap
// (kh, kw) reads input pixel (2 qr + kh, 2 qc + kw).  A K step is 16 consecutive output pixels of one row, i.e. input columns
// 2 k + kw: the halo image therefore keeps the EVEN and ODD input columns of a halo row as two runs of consecutive LDS rows
// ([17 even | 3 unused | 16 odd] = 36 rows of 128 B per halo row; the DMA source address is per lane, so the order of the LDS rows is
// free).  Tap column kw = 0 / 1 / 2 is then run (even, k) / (odd, k) / (even, k + 1): sixteen consecutive rows, exactly the access of
// the unit-stride image (same half-swap swizzle on bit 1 of the row index, no bank conflicts), and because every offset between taps
// and K steps is a multiple of four rows, (even, k) and (odd, k) share one swizzled address register.  5 halo rows x 36 = 180 rows
// (23 items) + 2 x 32 dY rows (8 items): the same 31 items and 31 KiB per stage as the unit-stride form, with 18 MFMAs per wave.
// Against wgrad_bf16_kernel<9> (nine shifted tiles through registers and ds_write, a barrier per 16 pixels, MFMA busy 0.18): 5.2
// input pixels fetched per output pixel instead of 9, no VGPR staging, a barrier per 32 pixels.
// MODE 0: unit stride, stages of 4 x 16 pixels.  MODE 1: stride 2, stages of 2 x 16 output pixels (5 x 33 halo).  MODE 2: stride 2 on maps
// whose output width is only a multiple of 8 (the discriminator's last layer, 16 x 16 -> 8 x 8): stages of 4 x 8 output pixels, 9 x 17 halo
// stored as [9 even | 3 unused | 8 odd] = 20 LDS rows per halo row -- the same 180 rows; a K step is two output rows of eight pixels, so the
// lane half hh of a fragment sits two halo rows (40 LDS rows) further down instead of eight plane entries further on.
// Stage geometry of wgrad_halo8_bf16_kernel<MODE>: the kernel and its launcher read it
template <int MODE>
struct Halo8Shape {
    static constexpr bool S2 = MODE != 0;
    static constexpr int R = MODE == 1 ? 2 : 4;                // output rows per stage
    static constexpr int PW = MODE == 2 ? 8 : 16;
    static constexpr int HP = MODE == 2 ? 12 : 20;             // S1: LDS pitch of a halo row (18 valid); S2: pitch of the even run
    static constexpr int HRP = MODE == 1 ? 36 : 20;            // LDS rows per halo row
    static constexpr int NHROW = S2 ? 2 * R + 1 : R + 2;       // halo rows: 6 | 5 | 9
    static constexpr int NHR = NHROW * HRP;                    // 120 | 180 | 180
    static constexpr int KSTEPS = R * PW / 16;                 // K steps (16 output pixels) per stage
    static constexpr int NXI = (NHR + 7) / 8, NDT = R * PW / 8;       // x items 15 | 23 | 23, dY items per co tile 8 | 4 | 4
    static constexpr int NIT = NXI + 2 * NDT;                  // 31 | 31 | 31
    static_assert(NIT == 31, "31 items per stage: waves 0-6 issue four, wave 7 three");
    static constexpr int NJ = 4;
    static constexpr int XROWS = NXI * 8, DROWS = NDT * 8;     // LDS rows of the x region, of one dY tile
    static constexpr int STAGE = (XROWS + 2 * DROWS) * 64;     // bf16 elements: 248 rows of 128 B
    static constexpr int NST = 3;
    static constexpr unsigned lds_bytes = NST * STAGE * 2u;    // 93 KiB
};

template <int MODE>
__global__ __launch_bounds__(512, 2) void wgrad_halo8_bf16_kernel(const WgradHaloArgs a) {
    typedef Halo8Shape<MODE> SH;
    constexpr bool S2 = SH::S2;
    constexpr int R = SH::R, PW = SH::PW, HP = SH::HP, HRP = SH::HRP, NHROW = SH::NHROW, NHR = SH::NHR, KSTEPS = SH::KSTEPS;
    constexpr int NXI = SH::NXI, NDT = SH::NDT, NIT = SH::NIT, NJ = SH::NJ, XROWS = SH::XROWS, DROWS = SH::DROWS, STAGE = SH::STAGE, NST = SH::NST;
    extern __shared__ __attribute__((aligned(1024))) unsigned short smem[];
    typedef __attribute__((address_space(3))) void* lds_ptr;

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l31 = lane & 31, hh = lane >> 5;
    const int cot = wave >> 2, mi = (wave >> 1) & 1, ni = wave & 1;       // co tile of the pair, 32 x 32 sub-tile
    const Blk3 blk = xcd_block_order();
    const int ci0 = blk.x * 64, co0 = blk.y * 128;
    const int pid0 = blk.z * a.patches_per_split;
    const int pid1 = min(a.npatch, pid0 + a.patches_per_split);
    const int nstages = pid1 - pid0;
    const int ho = S2 ? a.h / 2 : a.h, wo = S2 ? a.w / 2 : a.w;

    // DMA lane mapping: lane -> (row l >> 3 of the item, 16-byte chunk l & 7); LDS chunk j of row r holds source chunk j ^ (4 * bit1(r))
    const int drow = lane >> 3;
    const int sch = (lane & 7) ^ (((drow >> 1) & 1) << 2);
    const bool second = ci0 >= a.c1;
    const int ldX = second ? a.ldx2 : a.ldx;
    const int cX = ci0 + sch * 8;
    const bool xvalid = cX < a.cin_ld;
    const int ccX = second ? cX - a.c1 : cX;
    // descriptors as words: the DMA is issued as inline asm (common.h, shm_dma16)
    const shm_u32x4 rsx = second ? shm_rsrc_words(a.x2, a.x2bytes) : shm_rsrc_words(a.x, a.xbytes);
    const shm_u32x4 rsd = shm_rsrc_words(a.dy, a.dybytes);

    PatchWalk<R, PW> pw;                                // patch origin in OUTPUT pixels
    pw.start(pid0, a.npatch, ho, wo);
    // per-lane constants of this wave's items (item = wave + 8 j): byte offset inside the halo / patch, and five mask bits -- which
    // edges of the halo the lane's pixel sits on (1 top, 2 bottom, 4 left, 8 right) and 16 for lanes with nothing to fetch
    unsigned off0[NJ], bm = 0;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int item = wave + 8 * j;
        unsigned bits;
        if (item < NXI) {
            const int row = 8 * item + drow;
            int r_, c_;
            bool ok;
            if constexpr (S2) {
                const S2RunPixel px = s2_run_pixel<HRP, HP, PW>(row);
                r_ = px.r;
                c_ = px.c;
                ok = row < NHR && px.ok;
                bits = halo_pixel_bits(r_, c_, NHROW - 1, 2 * PW, false);
            } else {
                r_ = row / HP;
                c_ = row - r_ * HP;
                ok = c_ < PW + 2;
                bits = halo_pixel_bits(r_, c_, R + 1, PW + 1, true);
            }
            off0[j] = (unsigned)((r_ * a.w + c_) * ldX + ccX) * 2u;
            if (!(xvalid && ok)) bits = 16u;
        } else {
            const int d = item - NXI, tile = d / NDT;
            const int q = 8 * (d - tile * NDT) + drow;
            const int coD = co0 + 64 * tile + sch * 8;
            off0[j] = (unsigned)(((q / PW) * wo + (q % PW)) * a.lddy + coD) * 2u;
            bits = (coD < a.cout && item < NIT) ? 0u : 16u;
        }
        bm |= bits << (5 * j);
    }
    auto dma = [&](int stage) {
        unsigned short* sx = smem + stage * STAGE;
        const int org = S2 ? (pw.n * a.h + 2 * pw.pr) * a.w + 2 * pw.pc : (pw.n * a.h + pw.pr - 1) * a.w + (pw.pc - 1);       // input pixel of halo (0, 0)
        const unsigned edges = pw.template edges<!S2>(ho, wo);
        const unsigned xb = (unsigned)(org * ldX) * 2u, db = (unsigned)(((pw.n * ho + pw.pr) * wo + pw.pc) * a.lddy) * 2u;
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            const int item = wave + 8 * j;
            if (j < NJ - 1 || item < NIT) {
                const bool isx = item < NXI;                   // wave-uniform
                const unsigned off = (bm & (edges << (5 * j))) ? 0xffffffffu : off0[j] + (isx ? xb : db);
                shm_dma16(isx ? rsx : rsd, shm_lds_addr(sx + item * 512), off);
            }
        }
        pw.next(ho, wo);
    };

    f32x16 acc[9];
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;

    int fa[3], fb;                                      // transposed-read addresses: one per kw, and the dY fragment's in this wave's co tile
    wgrad_tr_addrs<S2, HP, HRP, MODE == 2>(lane, mi, ni, (XROWS + cot * DROWS) * 64, fa, fb);
    auto compute = [&](int stage) {
        const unsigned short* X = smem + stage * STAGE;
#pragma unroll
        for (int qr = 0; qr < KSTEPS; ++qr) {
            const bf16x8 bv = tr_frag(X + fb + qr * 16 * 64);
#pragma unroll
            for (int t = 0; t < 9; ++t) {
                const int hrow = MODE == 0 ? qr + t / 3 : MODE == 1 ? 2 * qr + t / 3 : 4 * qr + t / 3;
                const bf16x8 av = tr_frag(X + fa[t % 3] + hrow * HRP * 64);
                acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(av, bv, acc[t], 0, 0, 0);
            }
        }
    };

    // wait until this wave's DMA items of every stage but the youngest one in flight have landed (four items per stage; wave 7: three)
    auto wait_older = [&](bool younger_in_flight) {
        if (younger_in_flight) {
            if (wave < 7)
                asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
            else
                asm volatile("s_waitcnt vmcnt(3)" ::: "memory");
        } else {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
    };
    // The ring of wgrad_stage_ring (wgrad_halo_dev.h), written out: through the helper hipcc lays the loop out as wait / barrier / DMA / MFMA
    // instead of MFMA-first -- the same instructions per stage, +0.2 to 0.6 % on n40 h32 1024x512 (311.5 -> 312.2 us) in three A/B runs, none this way
    if (nstages > 0) {
        dma(0);
        if (nstages > 1) dma(1);
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
        }
    }

    wgrad_store_slab<9, false>(acc, a.part + (size_t)blk.z * 9 * a.cin * a.cout, a.cin, a.cout, ci0, mi, hh, co0 + 64 * cot + ni * 32 + l31, nullptr);
}

template <int MODE>
static int halo8_launch(const WgradHaloArgs& a, const WgradPlan& p, hipStream_t st) {
    constexpr unsigned lds = Halo8Shape<MODE>::lds_bytes;
    static const hipError_t attr = hipFuncSetAttribute((const void*)wgrad_halo8_bf16_kernel<MODE>, hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    SHM_REQUIRE(attr == hipSuccess, SHM_E_HIP, "shm_conv2d_wgrad: cannot reserve %g KiB of LDS: %s", lds / 1024.0, hipGetErrorString(attr));
    hipLaunchKernelGGL((wgrad_halo8_bf16_kernel<MODE>), dim3(shm_cdiv(a.cin, 64), shm_cdiv(a.cout, 64 * kWgradHalo8CoTiles), p.splits), dim3(512), lds, st, a);
    shm_set_last_kernel("wgrad_halo8_bf16_kernel<%d>", MODE);
    return SHM_OK;
}

int shm_wgrad_halo8_launch(const WgradHaloArgs& a, const WgradPlan& p, hipStream_t st) {
    return p.mode8 == 0 ? halo8_launch<0>(a, p, st) : p.mode8 == 1 ? halo8_launch<1>(a, p, st) : halo8_launch<2>(a, p, st);
}
