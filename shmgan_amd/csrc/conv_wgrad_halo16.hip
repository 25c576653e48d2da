// wgrad_halo_bf16_kernel: the four-wave bf16 3x3 unit-stride weight gradient with an LDS halo patch (see conv_wgrad.hip's header comment).
#include "wgrad_halo_dev.h"

// ------------------------------------------------------------------------------------------
// bf16 version of the halo-patch weight gradient (3x3, stride 1): the LDS image of wgrad_halo_kernel in
// the row format of wgrad_bf16_kernel.  Stage = 2 x 16 output pixels: a 4 x 20 halo image (18 columns
// used; the pitch of 20 keeps bit 1 of the row index independent of the tap's row offset, so one
// swizzled address per kw serves all taps through immediates) of 128-byte rows (64 channels) and 32 dY
// rows, brought in by LDS-DMA with the half-swap swizzle applied on the source side; two K steps of 16
// pixels, nine v_mfma_f32_32x32x16_bf16 each, operands via ds_read_b64_tr_b16.
// R = pixel rows per stage (2 or 4).  The x fragment of tap row kh at K step (pixel row) q is the fragment of tap row 0 at
// q + kh, so a stage of R rows needs (R + 2) x 3 fragment reads for 9 R MFMAs (hipcc keeps the shared ones in registers):
// R = 4 reads 22 fragments per 36 MFMAs where two R = 2 stages read 28, with half the barriers and 3/4 of the halo bytes.
// NM: as in wgrad_halo_kernel (a lane's eight channels are the same for every item and patch: 24 table registers).

// Stage geometry of wgrad_halo_bf16_kernel<R, *>: the kernel and its launcher read it
template <int R>
struct Halo16Shape {
    static constexpr int PW = 16, HP = 20;                     // patch R x 16; halo R + 2 rows, LDS pitch 20 (18 valid)
    static constexpr int NHR = (R + 2) * HP, NPX = R * PW;     // R = 2: 80 halo rows, 32 dY rows (14 KiB); R = 4: 120 + 64 (23 KiB)
    static constexpr int STAGE = (NHR + NPX) * 64;             // bf16 elements per stage
    static constexpr int NST = 3;
    static constexpr int NXI = NHR / 8, NDI = NPX / 8;         // DMA items (8 rows of 128 B each): 10 + 4 / 15 + 8
    static constexpr int NIT = NXI + NDI, NJ = (NIT + 3) / 4;  // items per wave: waves below NIT % 4 (or all) take NJ, the others NJ - 1
    static constexpr int NXJ = (NXI + 3) / 4;                  // halo items per wave (at most)
    static constexpr unsigned lds_bytes = NST * STAGE * 2u;    // R = 2: 42 KiB, R = 4: 69 KiB
};

template <int R, int NM = 0>
__global__ __launch_bounds__(256, 2) void wgrad_halo_bf16_kernel(const WgradHaloArgs a) {
    typedef Halo16Shape<R> SH;
    constexpr int PW = SH::PW, HP = SH::HP, NHR = SH::NHR, STAGE = SH::STAGE, NST = SH::NST, NXI = SH::NXI, NIT = SH::NIT, NJ = SH::NJ, NXJ = SH::NXJ;
    extern __shared__ __attribute__((aligned(1024))) unsigned short smem[];
    typedef __attribute__((address_space(3))) void* lds_ptr;

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l31 = lane & 31, hh = lane >> 5;
    const int mi = wave >> 1, ni = wave & 1;
    const Blk3 blk = xcd_block_order();
    const int ci0 = blk.x * 64, co0 = blk.y * 64;
    const int pid0 = blk.z * a.patches_per_split;
    const int pid1 = min(a.npatch, pid0 + a.patches_per_split);
    const int nstages = pid1 - pid0;

    // DMA lane mapping: lane -> (row l>>3 of the item, 16-byte chunk l&7); LDS chunk j of row r holds source
    // chunk j ^ (4 * bit1(r)).  Items are 8 rows, so bit1(r) = bit1(l>>3).
    const int drow = lane >> 3;
    const int sch = (lane & 7) ^ (((drow >> 1) & 1) << 2);
    const bool second = ci0 >= a.c1;
    const int ldX = second ? a.ldx2 : a.ldx;
    const int cX = ci0 + sch * 8;
    const bool xvalid = cX < a.cin_ld;
    const int ccX = second ? cX - a.c1 : cX;
    const int coD = co0 + sch * 8;
    const bool dvalid = coD < a.cout;
    // descriptors as words: the DMA is issued as inline asm (common.h, shm_dma16)
    const shm_u32x4 rsx = second ? shm_rsrc_words(a.x2, a.x2bytes) : shm_rsrc_words(a.x, a.xbytes);
    const shm_u32x4 rsd = shm_rsrc_words(a.dy, a.dybytes);
    // items 0..9: halo rows [8i, 8i+8); items 10..13: dY rows.  Wave w takes items w, w+4, w+8, w+12.
    [[maybe_unused]] int hr[NXJ], hc[NXJ];                 // (NM: norm_x)
#pragma unroll
    for (int j = 0; j < NXJ; ++j) {
        const int hp = 8 * (wave + 4 * j) + drow;
        hr[j] = hp / HP;
        hc[j] = hp - hr[j] * HP;
    }

    PatchWalk<R, PW> pw;
    pw.start(pid0, a.npatch, a.h, a.w);
    // DMA addressing as in wgrad_halo_kernel: per-lane constant offset + patch origin, edge bits (five per item, one register)
    static_assert(NJ <= 6, "five mask bits per item in one register");
    unsigned off0[NJ], bm = 0;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int item = wave + 4 * j;
        unsigned bits;
        if (item < NXI) {
            const int hp = 8 * item + drow;
            const int r_ = hp / HP, c_ = hp - r_ * HP;
            off0[j] = (unsigned)((r_ * a.w + c_) * ldX + ccX) * 2u;
            bits = !(xvalid && c_ < PW + 2) ? 16u : halo_pixel_bits(r_, c_, R + 1, PW + 1, true);
        } else {
            const int q = 8 * (item - NXI) + drow;
            off0[j] = (unsigned)(((q >> 4) * a.w + (q & 15)) * a.lddy + coD) * 2u;
            bits = (dvalid && item < NIT) ? 0u : 16u;
        }
        bm |= bits << (5 * j);
    }
    auto dma = [&](int stage) {
        unsigned short* sx = smem + stage * STAGE;
        const int org = (pw.n * a.h + pw.pr - 1) * a.w + (pw.pc - 1);       // pixel index of halo (0,0)
        const unsigned edges = pw.template edges<true>(a.h, a.w);
        const unsigned xb = (unsigned)(org * ldX) * 2u, db = (unsigned)(((pw.n * a.h + pw.pr) * a.w + pw.pc) * a.lddy) * 2u;
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            const int item = wave + 4 * j;
            if (j < NJ - 1 || item < NIT) {
                const bool isx = item < NXI;                   // wave-uniform
                const unsigned off = (bm & (edges << (5 * j))) ? 0xffffffffu : off0[j] + (isx ? xb : db);
                shm_dma16(isx ? rsx : rsd, shm_lds_addr(sx + item * 512), off);
            }
        }
        pw.next(a.h, a.w);
    };

    const bool nm_on = NM && a.nt != nullptr && (int)second == a.ntpart;        // block-uniform
    [[maybe_unused]] PatchWalk<R, PW> pw2 = pw;              // the next stage to normalise: one stage behind dma()'s
    [[maybe_unused]] int nimg = -1;
    [[maybe_unused]] f32x4 nmean[2] = {}, ninv[2] = {}, nbeta[2] = {};
    const int n_blk = pw.n;                                    // NM = 2: the sample of this block's patches
    [[maybe_unused]] auto norm_x = [&](int stage) {
        if (pw2.n != nimg) {                                   // block-uniform
            nimg = pw2.n;
            if (xvalid) {
                const float* t = a.nt + (size_t)pw2.n * SHM_NT_PLANES * a.ntc + ccX;
#pragma unroll
                for (int hf = 0; hf < 2; ++hf) {
                    if constexpr (NM == 2) {
                        nbeta[hf] = load16_drained(t + 3 * a.ntc + 4 * hf);        // ring
                    } else {
                        nmean[hf] = load16_drained(t + 4 * hf);
                        ninv[hf] = load16_drained(t + a.ntc + 4 * hf);
                        nbeta[hf] = load16_drained(t + 2 * a.ntc + 4 * hf);
                    }
                }
            }
        }
        typedef unsigned u32x4_t __attribute__((ext_vector_type(4)));
        unsigned short* sx = smem + stage * STAGE + lane * 8;
        if constexpr (NM == 2) {
            // SHM_NORM_SCALED: `ring` over the out-of-image halo entries of a border patch (the two dummy columns of the pitch stay zero)
            if (!pw2.interior(a.h, a.w)) {
                u32x4_t rg;
#pragma unroll
                for (int hf = 0; hf < 2; ++hf)
#pragma unroll
                    for (int e = 0; e < 2; ++e)
                        rg[2 * hf + e] = (unsigned)__builtin_bit_cast(unsigned short, (bf16_t)nbeta[hf][2 * e]) |
                                         ((unsigned)__builtin_bit_cast(unsigned short, (bf16_t)nbeta[hf][2 * e + 1]) << 16);
#pragma unroll
                for (int j = 0; j < NXJ; ++j) {
                    const int item = wave + 4 * j;
                    if (item < NXI) {
                        const int iy = pw2.pr - 1 + hr[j], ix = pw2.pc - 1 + hc[j];
                        if (xvalid && hc[j] < PW + 2 && !((unsigned)iy < (unsigned)a.h && (unsigned)ix < (unsigned)a.w)) *(u32x4_t*)(sx + item * 512) = rg;
                    }
                }
            }
        } else {
#pragma unroll
        for (int j = 0; j < NXJ; ++j) {
            const int item = wave + 4 * j;
            if (item < NXI) {
                const int iy = pw2.pr - 1 + hr[j], ix = pw2.pc - 1 + hc[j];
                if (xvalid && hc[j] < PW + 2 && (unsigned)iy < (unsigned)a.h && (unsigned)ix < (unsigned)a.w) {
                    u32x4_t x = *(const u32x4_t*)(sx + item * 512);
#pragma unroll
                    for (int hf = 0; hf < 2; ++hf)
#pragma unroll
                        for (int e = 0; e < 2; ++e) {
                            const unsigned u = x[2 * hf + e];
                            const bf16_t lo = (bf16_t)shm_in_norm(__uint_as_float(u << 16), nmean[hf][2 * e], ninv[hf][2 * e], nbeta[hf][2 * e]);
                            const bf16_t hi = (bf16_t)shm_in_norm(__uint_as_float(u & 0xffff0000u), nmean[hf][2 * e + 1], ninv[hf][2 * e + 1], nbeta[hf][2 * e + 1]);
                            x[2 * hf + e] = (unsigned)__builtin_bit_cast(unsigned short, lo) | ((unsigned)__builtin_bit_cast(unsigned short, hi) << 16);
                        }
                    *(u32x4_t*)(sx + item * 512) = x;
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

    int fa[3], fb;                                          // transposed-read addresses: one per kw, and the dY fragment's
    wgrad_tr_addrs<false, HP, HP>(lane, mi, ni, 0, fa, fb);
    auto compute = [&](int stage) {
        const unsigned short* X = smem + stage * STAGE;
        const unsigned short* D = X + NHR * 64;
#pragma unroll
        for (int qr = 0; qr < R; ++qr) {
            const bf16x8 bv = tr_frag(D + fb + qr * PW * 64);
#pragma unroll
            for (int t = 0; t < 9; ++t) {
                const bf16x8 av = tr_frag(X + fa[t % 3] + (qr + t / 3) * HP * 64);
                acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(av, bv, acc[t], 0, 0, 0);
            }
        }
    };

    // wait until this wave's DMA items of every stage but the youngest one in flight (NJ or NJ - 1 instructions) have landed
    auto wait_older = [&](bool younger_in_flight) {
        if (younger_in_flight) {
            if (NIT % 4 == 0 || wave < NIT % 4)
                asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NJ) : "memory");
            else
                asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NJ - 1) : "memory");
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

template <int R, int NM>
static int halo16_launch(const WgradHaloArgs& a, const WgradPlan& p, hipStream_t st) {
    constexpr unsigned lds = Halo16Shape<R>::lds_bytes;
    if constexpr (R == 4) {                              // above the 64 KiB a kernel gets unasked
        static const hipError_t attr = hipFuncSetAttribute((const void*)wgrad_halo_bf16_kernel<R, NM>, hipFuncAttributeMaxDynamicSharedMemorySize, lds);
        SHM_REQUIRE(attr == hipSuccess, SHM_E_HIP, "shm_conv2d_wgrad: cannot reserve %g KiB of LDS: %s", lds / 1024.0, hipGetErrorString(attr));
    }
    hipLaunchKernelGGL((wgrad_halo_bf16_kernel<R, NM>), dim3(shm_cdiv(a.cin, 64), shm_cdiv(a.cout, 64), p.splits), dim3(256), lds, st, a);
    if (NM)
        shm_set_last_kernel("wgrad_halo_bf16_kernel<%d, %d>", R, NM);
    else
        shm_set_last_kernel("wgrad_halo_bf16_kernel<%d>", R);
    return SHM_OK;
}

template <int R>
static int halo16_launch_r(const WgradHaloArgs& a, const WgradPlan& p, hipStream_t st) {
    return p.nmode == 2 ? halo16_launch<R, 2>(a, p, st) : p.nmode == 1 ? halo16_launch<R, 1>(a, p, st) : halo16_launch<R, 0>(a, p, st);
}

int shm_wgrad_halo16_launch(const WgradHaloArgs& a, const WgradPlan& p, hipStream_t st) {
    return p.rows == 4 ? halo16_launch_r<4>(a, p, st) : halo16_launch_r<2>(a, p, st);
}
