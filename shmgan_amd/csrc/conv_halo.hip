// tapgemm_halo_kernel: the unit-stride 3x3 tap GEMM with an LDS halo, and its six SHM_TG_HALO* forms (see conv_igemm.hip's header comment).
#include "tapgemm_dev.h"

// ------------------------------------------------------------------------------------------
// 3x3 / stride-1 tap GEMM with an LDS halo for the A operand (forward conv and its dgrad).
//
// Block = 16 x 16 output pixels of one image (M = 256) x 128 output channels, 8 waves of 64x64.
// Per 16-channel chunk the 18 x 18 input halo is DMA'd into LDS ONCE (double buffered, fetched
// while the previous chunk's nine taps are computed); the nine taps read it through nine shifted
// fragment addresses.  Only the weight slice (128 rows x 64 B) is streamed per tap (3 stages, DMA
// two taps ahead).  Per tap a wave issues 1 DMA instruction instead of 4, and the A operand moves
// 6.4x fewer bytes.  Same LDS row format as tapgemm_dma_kernel: 64-byte rows, chunk ^= (row>>2)&3
// applied on the DMA source side; halo pixels outside the image use offset 0xffffffff (zeros).
// PH = patch height (16 or 8 pixel rows of 16): M = PH*16 rows, PH/4 row-waves.  PH = 8 halves the A stages
// (3 four-wave blocks per CU instead of 2 eight-wave ones: smaller barrier groups) at 11 % more halo traffic.
// ST (round 2): the nine taps of a chunk are unrolled, which makes every fragment address a patch- and chunk-independent
// register (one per (tap, tile); the second k group is an XOR, the B stage an immediate) -- no address arithmetic between the
// barrier and the first ds_read of a K step -- and lets the halo use the conflict-free swizzle ((R >> 1) + R / 18) & 3 that
// cost 3 % when its arithmetic sat on that path.
// TM = 32-row MFMA tiles per wave along M (2: wave tile 64 pixels x 64 channels; 4, static taps only: 128 x 64 -- half the waves,
// six fragment reads per eight MFMAs instead of four per four, twice the MFMAs per barrier: the bf16 form, whose K step is 8x shorter).
// GS: the gsum epilogue (input-gradient launches, see TapGemmArgs) -- an instantiation of its own, so that the forward kernels
// carry none of its code or registers.
// NM: "norm" -- one source is the UN-normalised activation of an InstanceNorm block (TapGemmArgs::nt): every wave applies
// shm_in_norm to the halo items it DMA'd itself, in LDS, once they have landed and before the barrier that opens the chunk -- the
// stand-alone normalisation pass (a read and a write of the whole activation) is gone, for 3 ds_read_b128 + 4 fma + 1 ds_write_b128 per
// 1 KiB item and 2304 (fp32) MFMAs.  Out-of-image halo pixels were DMA'd as zeros and are left alone: zero padding of the
// NORMALISED tensor, as the layer defines it.  The (mean, inv, beta) planes of the block's image sit in LDS (3 x ntc floats).
// NM = 0: none; 1: SHM_NORM_EXACT (above); 2: SHM_NORM_SCALED (TapGemmArgs: per-sample weights and bias rows, `ring` over the out-of-image entries).
template <typename T, typename TO, int BN, int PH = 16, bool ST = false, int TM = 2, bool GS = false, int NM = 0>
__global__ __launch_bounds__(BN * PH / (2 * TM), ST ? BN * PH / (256 * TM) : 1) void tapgemm_halo_kernel(const TapGemmArgs a) {
    static_assert(TM == 2 || (TM == 4 && ST), "four M tiles per wave: static-tap form only");
    static_assert(!NM || (ST && TM == 2 && !GS), "norm: static-tap forward form");
    constexpr int ESZ = sizeof(T), CHE = 16 / ESZ, BKE = 64 / ESZ;      // channels per 16-byte chunk / per 64-byte row
    constexpr int WGM = PH / (2 * TM), WGN = BN / 64, NW = WGM * WGN;   // waves: PH / (2 TM) (M) x (BN/64) (N)
    constexpr int HC = 18, NIT = PH == 16 ? 24 : 12;  // halo (PH+2) x 18 rows, padded to NIT DMA items of 16 rows
    constexpr int NHR = NIT * 16;
    constexpr int ASTG = NHR * 16, BSTG = BN * 16;    // floats per stage
    constexpr int NA = NIT / NW, NB = (BN / 16) / NW; // DMA instructions per wave: A per chunk, B per tap
    static_assert(NIT % NW == 0 && (BN / 16) % NW == 0, "DMA items divide over the waves");
    __shared__ __attribute__((aligned(1024))) float smem[2 * ASTG + 3 * BSTG];
    __shared__ __attribute__((aligned(1024))) float snt[NM ? SHM_NT_PLANES * SHM_NT_MAXC : 4];
    float* const sA = smem;
    float* const sB = smem + 2 * ASTG;
    typedef __attribute__((address_space(3))) void* lds_ptr;

    const TapPhase& P = a.ph[0];
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l31 = lane & 31, h = lane >> 5;
    const int wm = wave / WGN, wn = wave % WGN;
    // block -> (image, patch)
    const int ppr = a.wi >> 4, ppi = (a.hi / PH) * ppr;
    const int img = blockIdx.x / ppi, prem = blockIdx.x - img * ppi;
    const int y0 = (prem / ppr) * PH, x0 = (prem % ppr) << 4;
    const int n0 = blockIdx.y * BN;
    // NM = 2: only a patch on the image border reads the table (its `ring` plane) -- an interior block skips the table, the barrier that
    // publishes it and every norm_a (in bf16 the extra DMA round trip in the prologue is 10-25 % of a block's life)
    [[maybe_unused]] const bool nm_table = NM == 1 || (NM == 2 && (y0 == 0 || y0 + PH == a.hi || x0 == 0 || x0 + 16 == a.wi));      // block-uniform

    // ---- DMA lane constants.  A item it (0..23) = halo rows [16 it, 16 it + 16); wave w owns items w, w+NW, ...
    const int drow = lane >> 2, dq = lane & 3;
    unsigned arow1[NA], arow2[NA];
    // NM: c = first channel (within its 64-byte row) of the lane's 16 bytes of item j: c for an image pixel, -1 - c for a halo pixel
    // outside the image, INT_MIN for the unused tail rows of the last item
    [[maybe_unused]] int nmv[NA];
#pragma unroll
    for (int j = 0; j < NA; ++j) {
        const int hrow = 16 * (wave + NW * j) + drow;
        const int hr = hrow / HC, hc = hrow - hr * HC;
        const int iy = y0 - 1 + hr, ix = x0 - 1 + hc;
        const bool v = hrow < (PH + 2) * HC && (unsigned)iy < (unsigned)a.hi && (unsigned)ix < (unsigned)a.wi;
        const int pix = (img * a.hi + iy) * a.wi + ix;
        const int coff = (dq ^ (ST ? ((hrow >> 1) + hr) & 3 : (hrow >> 2) & 3)) * CHE;
        arow1[j] = v ? (unsigned)(pix * a.ldx + coff) * (unsigned)ESZ : 0xffffffffu;
        arow2[j] = v ? (unsigned)(pix * a.ldx2 + coff) * (unsigned)ESZ : 0xffffffffu;
        nmv[j] = v ? coff : hrow < (PH + 2) * HC ? -1 - coff : (int)0x80000000;
    }
    unsigned wrow[NB];
#pragma unroll
    for (int j = 0; j < NB; ++j) {
        const int row = (wave + NW * j) * 16 + drow;       // B item wave + NW j = rows [16 item, 16 item + 16)
        const int nn = n0 + row;
        wrow[j] = nn < a.nout ? (unsigned)(nn * a.K + (dq ^ ((row >> 2) & 3)) * CHE) * (unsigned)ESZ : 0xffffffffu;
    }
    const __amdgpu_buffer_rsrc_t rsx = __builtin_amdgcn_make_buffer_rsrc((void*)a.x, 0, a.xbytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t rsx2 = __builtin_amdgcn_make_buffer_rsrc((void*)a.x2, 0, a.x2bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t rsw = __builtin_amdgcn_make_buffer_rsrc((void*)a.w, 0, a.wbytes, 0x00020000);

    const int nch = a.K / BKE;
    const int ksteps = 9 * nch;
    // tap table in VGPR lanes: halo row shift (dh*18 + dw) and weight slice of tap `lane`
    const int tl = lane < 9 ? lane : 0;
    const int tapsh_v = P.dh[tl] * HC + P.dw[tl];
    const int tapw_v = P.widx[tl];

    auto dma_a = [&](int chunk) {                  // halo of 64-byte channel chunk `chunk` into A stage chunk & 1
        const int c0 = chunk * BKE;
        const bool second = c0 >= a.c1;
        const unsigned cb = (unsigned)(second ? c0 - a.c1 : c0) * (unsigned)ESZ;
        float* dst = sA + (chunk & 1) * ASTG + wave * 256;
#pragma unroll
        for (int j = 0; j < NA; ++j) {
            const unsigned r = second ? arow2[j] : arow1[j];
            const unsigned off = r == 0xffffffffu ? r : r + cb;
            if (second)
                __builtin_amdgcn_raw_ptr_buffer_load_lds(rsx2, (lds_ptr)(dst + j * NW * 256), 16, (int)off, 0, 0, 0);
            else
                __builtin_amdgcn_raw_ptr_buffer_load_lds(rsx, (lds_ptr)(dst + j * NW * 256), 16, (int)off, 0, 0, 0);
        }
    };
    int ld_tap = 0, ld_chunk = 0, ld_stage = 0;    // position of the next weight DMA
    auto dma_b = [&]() {
        const int t_wi = __builtin_amdgcn_readlane(tapw_v, ld_tap);
        const unsigned wbase = (unsigned)((t_wi * a.nout) * a.K + ld_chunk * BKE) * (unsigned)ESZ + (NM == 2 ? (unsigned)img * a.wimg : 0u);
#pragma unroll
        for (int j = 0; j < NB; ++j) {
            const unsigned off = wrow[j] == 0xffffffffu ? wrow[j] : wrow[j] + wbase;
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rsw, (lds_ptr)(sB + ld_stage * BSTG + (wave + NW * j) * 256), 16, (int)off, 0, 0, 0);
        }
        if (++ld_tap == 9) {
            ld_tap = 0;
            ++ld_chunk;
        }
        ld_stage = ld_stage == 2 ? 0 : ld_stage + 1;
    };

    f32x16 acc[TM][2];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    // fragment addressing.  A: lane -> patch pixel (4 wm + 2 i + (l31 >> 4), l31 & 15), halo row of the
    // centre tap; B: as in tapgemm_dma_kernel
    // Swizzle (R >> 2) & 3 on the halo row index R: because halo rows start at arbitrary offsets, a third of the
    // fragment reads see a 2-way bank conflict (SQ_LDS_BANK_CONFLICT).  The conflict-free function for this access
    // pattern is ((R >> 1) + R / 18) & 3 (exhaustive check over taps and lane groups); it was measured 3 % SLOWER in
    // both dtypes -- its per-tap address work sits on the barrier -> first ds_read critical path, the conflicts do not.
    int hb[TM];
#pragma unroll
    for (int i = 0; i < TM; ++i) hb[i] = (2 * TM * wm + 2 * i + (l31 >> 4) + 1) * HC + (l31 & 15) + 1;
    const int swb = (l31 >> 2) & 3;
    const int fb0 = l31 * 16 + ((0 + h) ^ swb) * 4, fb1 = l31 * 16 + ((2 + h) ^ swb) * 4;

    [[maybe_unused]] f32x4 abl_frag = {0.f, 0.f, 0.f, 0.f};
    if constexpr (abl::nolds) abl_frag = *(const f32x4*)(sA + lane * 4);
    auto compute = [&](int chunk, int tap, int bstage) {
        const float* Ab = sA + (chunk & 1) * ASTG;
        const float* Bb = sB + bstage * BSTG + wn * 64 * 16;
        const int sh = __builtin_amdgcn_readlane(tapsh_v, tap);
        int fa[2][2];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int hrow = hb[i] + sh;
            const int sw = (hrow >> 2) & 3;
            fa[i][0] = hrow * 16 + ((0 + h) ^ sw) * 4;
            fa[i][1] = hrow * 16 + ((2 + h) ^ sw) * 4;
        }
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
            f32x4 av[2], bv[2];
            if constexpr (abl::nolds) {
                // timing only: fragments from registers (one read per block), MFMAs + barriers + DMA unchanged
                for (int i = 0; i < 2; ++i) av[i] = abl_frag;
                for (int j = 0; j < 2; ++j) bv[j] = abl_frag;
                asm volatile("" : "+v"(av[0]), "+v"(av[1]), "+v"(bv[0]), "+v"(bv[1]));
            } else {
#pragma unroll
                for (int i = 0; i < 2; ++i) av[i] = *(const f32x4*)(Ab + fa[i][kk]);
#pragma unroll
                for (int j = 0; j < 2; ++j) bv[j] = *(const f32x4*)(Bb + j * 512 + (kk ? fb1 : fb0));
            }
            if constexpr (TM == 2) tap_mfma<T, 2, 2>(av, bv, acc);
        }
    };

    // NM: normalise this wave's own items of the A stage of `chunk` in place (they have landed: the caller waited)
    // (the plane pitch as an opaque scalar: re-read from the kernel arguments inside the tap loop it is a scalar memory load whose
    // s_waitcnt lgkmcnt(0) drains the ds_reads)
    [[maybe_unused]] int ntc_s = NM ? a.ntc : 0;
    if constexpr (NM != 0) asm volatile("" : "+s"(ntc_s));
    [[maybe_unused]] auto norm_a = [&](int chunk) {
        const int c0 = chunk * BKE;
        const bool second = c0 >= a.c1;
        if ((int)second != a.ntpart) return;                      // block-uniform: this chunk's source is used as stored
        const float* tb0 = snt + (second ? c0 - a.c1 : c0);
        float* dst = sA + (chunk & 1) * ASTG + wave * 256 + lane * 4;
        if constexpr (NM == 2) {
            // SHM_NORM_SCALED: only a patch on the image border has anything to do -- its out-of-image halo entries (DMA'd as zeros) get
            // `ring`; (w * inv) * ring + w * (beta - mean * inv) = 0, the tap's contribution under zero padding of the normalised tensor
            if (!nm_table) return;          // block-uniform
#pragma unroll
            for (int j = 0; j < NA; ++j) {
                const int m = nmv[j];
                if (m < 0 && m != (int)0x80000000) {
                    const float* tb = tb0 + (-1 - m) + 3 * ntc_s;
                    float* p = dst + j * NW * 256;
                    if constexpr (ESZ == 4) {
                        *(f32x4*)p = *(const f32x4*)tb;
                    } else {
                        const f32x4 r0 = *(const f32x4*)tb, r1 = *(const f32x4*)(tb + 4);
                        u32x4 x;
#pragma unroll
                        for (int e = 0; e < 2; ++e) {
                            x[e] = (unsigned)__builtin_bit_cast(unsigned short, (bf16_t)r0[2 * e]) |
                                   ((unsigned)__builtin_bit_cast(unsigned short, (bf16_t)r0[2 * e + 1]) << 16);
                            x[2 + e] = (unsigned)__builtin_bit_cast(unsigned short, (bf16_t)r1[2 * e]) |
                                       ((unsigned)__builtin_bit_cast(unsigned short, (bf16_t)r1[2 * e + 1]) << 16);
                        }
                        *(u32x4*)p = x;
                    }
                }
            }
            return;
        } else {
#pragma unroll
        for (int j = 0; j < NA; ++j) {
            if (nmv[j] >= 0) {
                const float* tb = tb0 + nmv[j];
                float* p = dst + j * NW * 256;
                if constexpr (ESZ == 4) {
                    f32x4 x = *(const f32x4*)p;
                    const f32x4 mean = *(const f32x4*)tb, inv = *(const f32x4*)(tb + ntc_s), beta = *(const f32x4*)(tb + 2 * ntc_s);
#pragma unroll
                    for (int e = 0; e < 4; ++e) x[e] = shm_in_norm(x[e], mean[e], inv[e], beta[e]);
                    *(f32x4*)p = x;
                } else {
                    u32x4 x = *(const u32x4*)p;
#pragma unroll
                    for (int hf = 0; hf < 2; ++hf) {
                        const f32x4 mean = *(const f32x4*)(tb + 4 * hf), inv = *(const f32x4*)(tb + ntc_s + 4 * hf),
                                    beta = *(const f32x4*)(tb + 2 * ntc_s + 4 * hf);
#pragma unroll
                        for (int e = 0; e < 2; ++e) {
                            const unsigned u = x[2 * hf + e];
                            const bf16_t lo = (bf16_t)shm_in_norm(__uint_as_float(u << 16), mean[2 * e], inv[2 * e], beta[2 * e]);
                            const bf16_t hi = (bf16_t)shm_in_norm(__uint_as_float(u & 0xffff0000u), mean[2 * e + 1], inv[2 * e + 1], beta[2 * e + 1]);
                            x[2 * hf + e] = (unsigned)__builtin_bit_cast(unsigned short, lo) | ((unsigned)__builtin_bit_cast(unsigned short, hi) << 16);
                        }
                    }
                    *(u32x4*)p = x;
                }
            }
        }
        }
    };

    // ---- pipeline.  DMA issue order per wave: [NM: table piece]; A(0); B(0); B(1); then at step s: [A(chunk+1) if tap == 0]; B(s+2).
    if constexpr (NM) if (nm_table) {
        // the (mean, inv, beta, ring) planes of this block's image, 4 x ntc floats, in 1 KiB pieces (reads past the table give zeros)
        const __amdgpu_buffer_rsrc_t rsn = __builtin_amdgcn_make_buffer_rsrc((void*)a.nt, 0, a.ntbytes, 0x00020000);
        if (wave < SHM_NT_PLANES)
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rsn, (lds_ptr)(snt + wave * 256), 16,
                                                     (int)((unsigned)img * 16u * (unsigned)a.ntc + (unsigned)wave * 1024u + (unsigned)lane * 16u), 0, 0, 0);
    }
    dma_a(0);
    dma_b();
    if (ksteps > 1) dma_b();
    if constexpr (NM) if (nm_table) {
        asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * NB) : "memory");        // table piece and A(0) of this wave
        SHM_LDS_BARRIER();                                                    // ... the table pieces of every wave
        asm volatile("" ::: "memory");
        norm_a(0);
    }
    if constexpr (ST) {
        // fragment addresses of the nine taps (floats, relative to the A stage): registers for the whole block
        // (tile i sits 2 i patch rows = 36 i halo rows further on: (R >> 1) + R / 18 grows by 20 i, the swizzle does not change, and
        // the tile offset 2304 i bytes leaves bit 5 alone -- one register per tap, tiles and k groups as immediates / one XOR)
        int fs[9];
#pragma unroll
        for (int t = 0; t < 9; ++t) {
            const int hrow = hb[0] + P.dh[t] * HC + P.dw[t];
            fs[t] = hrow * 16 + ((h ^ (((hrow >> 1) + hrow / HC) & 3)) << 2);        // k group 1: this address ^ 8
        }
        typedef const __attribute__((address_space(3))) f32x4* lds_f4;
        const unsigned sA_lds = (unsigned)(size_t)(__attribute__((address_space(3))) float*)sA;
        int tw[9];                                     // weight slice of tap t (scalars)
#pragma unroll
        for (int t = 0; t < 9; ++t) tw[t] = __builtin_amdgcn_readlane(tapw_v, t);
        auto dma_b_at = [&](int t_wi, int chunk2, int stage2) {
            const unsigned wbase = (unsigned)((t_wi * a.nout) * a.K + chunk2 * BKE) * (unsigned)ESZ + (NM == 2 ? (unsigned)img * a.wimg : 0u);
#pragma unroll
            for (int j = 0; j < NB; ++j) {
                const unsigned off = wrow[j] == 0xffffffffu ? wrow[j] : wrow[j] + wbase;
                __builtin_amdgcn_raw_ptr_buffer_load_lds(rsw, (lds_ptr)(sB + stage2 * BSTG + (wave + NW * j) * 256), 16, (int)off, 0, 0, 0);
            }
        };
        for (int chunk = 0; chunk < nch; ++chunk) {
            // LDS byte address of the A stage: the k-group-1 address is formed as (stage + offset) ^ 32 inside the chunk loop,
            // so that the compiler keeps 18 address registers, not 36 (the stage base is a multiple of 64 bytes)
            const unsigned Ab = sA_lds + (unsigned)((chunk & 1) * ASTG * 4);
#pragma unroll
            for (int tap = 0; tap < 9; ++tap) {
                // B(s) (and, in order before it, the halo of this chunk) must have landed; issued after B(s): B(s+1),
                // preceded by the A items of step s-1 if that step opened a chunk
                if (tap == 8 && chunk + 1 == nch)
                    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                else if (tap == 1 && chunk + 1 < nch)
                    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NA + NB) : "memory");
                else
                    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NB) : "memory");
                SHM_LDS_BARRIER();
                asm volatile("" ::: "memory");
                if constexpr (!abl::nodma) {
                    if (tap == 0 && chunk + 1 < nch) dma_a(chunk + 1);
                    // the weight slice of step s + 2: tap, chunk carry and stage are compile-time here (9 % 3 == 0) -- the running
                    // (tap, chunk, stage) state of dma_b() cost ~25 scalar / vector instructions per tap, against eight bf16 MFMAs
                    if (tap < 7 || chunk + 1 < nch) dma_b_at(tw[(tap + 2) % 9], chunk + (tap + 2) / 9, (tap + 2) % 3);
                }
                const float* Bb = sB + (tap % 3) * BSTG + wn * 64 * 16;
#pragma unroll
                for (int kk = 0; kk < 2; ++kk) {
                    f32x4 av[TM], bv[2];
                    if constexpr (abl::nolds) {
                        for (int i = 0; i < TM; ++i) av[i] = abl_frag;
                        for (int j = 0; j < 2; ++j) bv[j] = abl_frag;
                        asm volatile("" : "+v"(av[0]), "+v"(av[1]), "+v"(bv[0]), "+v"(bv[1]));
                    } else {
                        const lds_f4 ap = (lds_f4)(size_t)((Ab + (unsigned)(fs[tap] << 2)) ^ (unsigned)(kk << 5));
#pragma unroll
                        for (int i = 0; i < TM; ++i) av[i] = ap[i * (2 * HC * 4)];               // 36 halo rows of 64 bytes per tile
#pragma unroll
                        for (int j = 0; j < 2; ++j) bv[j] = *(const f32x4*)(Bb + j * 512 + (kk ? fb1 : fb0));
                    }
                    if constexpr (!abl::nomfma)
                        tap_mfma<T, TM, 2>(av, bv, acc);
                    else
                        asm volatile("" :: "v"(av[0]), "v"(av[1]), "v"(bv[0]), "v"(bv[1]));
                }
                asm volatile("" ::: "memory");
                // NM: A(chunk + 1) was issued at tap 0 in front of B(2), which this step's wait covered: the wave's own items have
                // landed; the other waves read them after the barriers of taps 3..8 and of the next chunk's tap 0
                if constexpr (NM)
                    if (tap == 2 && chunk + 1 < nch && nm_table) {
                        norm_a(chunk + 1);
                        asm volatile("" ::: "memory");
                    }
            }
        }
    } else {
    int tap = 0, chunk = 0, bst = 0;
    for (int s = 0; s < ksteps; ++s) {
        // B(s) (and, in order before it, the halo of this chunk) must have landed.  Issued after B(s):
        // B(s+1), preceded by the A items of step s-1 if that step opened a chunk.
        if (s + 1 < ksteps) {
            if (tap == 1 && chunk + 1 < nch)
                asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NA + NB) : "memory");
            else
                asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NB) : "memory");
        } else {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        SHM_LDS_BARRIER();
        asm volatile("" ::: "memory");
        if constexpr (!abl::nodma) {
            if (tap == 0 && chunk + 1 < nch) dma_a(chunk + 1);      // other A stage: last read in the previous chunk
            if (s + 2 < ksteps) dma_b();
        }
        if constexpr (!abl::nomfma) compute(chunk, tap, bst);
        asm volatile("" ::: "memory");
        bst = bst == 2 ? 0 : bst + 1;
        if (++tap == 9) {
            tap = 0;
            ++chunk;
        }
    }
    }

    // ---- epilogue: bias + LeakyReLU + store (+ InstanceNorm statistics)
    float s1[2], s2[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) s1[j] = s2[j] = 0.f;
    // the bias of the lane's columns, once (see tapgemm_dma_kernel: a per-element fetch serialises the stores)
    float bj[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int n = n0 + wn * 64 + j * 32 + l31;
        bj[j] = (a.bias && n < a.nout) ? a.bias[(NM == 2 ? (size_t)img * a.bias_img : (size_t)0) + n] : 0.f;
        asm volatile("" : "+v"(bj[j]));           // waited for here, once (see tapgemm_dma_kernel)
    }
    // bf16 outputs: the MFMA accumulator layout gives each lane one 2-byte element per row, i.e. 64 two-byte
    // store instructions per wave -- measured 29 % of a 64-channel 256x256 layer.  Stage the wave's 64 x 64 tile
    // through LDS (free once every wave is past its last fragment read) and write 16 bytes per lane instead:
    // 8 store instructions per wave, each covering 8 pixel rows of 128 contiguous bytes.
    constexpr bool kWide = sizeof(TO) == 2;
    const bool wide = kWide && (a.nout % 8 == 0) && (a.n1 % 8 == 0) && (a.ldy % 8 == 0) && (((size_t)a.y & 15) == 0) &&
                      (a.y2 == nullptr || ((a.ldy2 % 8 == 0) && (((size_t)a.y2 & 15) == 0)));
    if constexpr (kWide) if (wide) {
        __syncthreads();
        unsigned short* tile = (unsigned short*)smem + wave * (TM * 32 * 64);
#pragma unroll
        for (int i = 0; i < TM; ++i) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = i * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    const int n = n0 + wn * 64 + j * 32 + l31;
                    float v = acc[i][j][r] + bj[j];
                    const TO vo = (TO)shm_lrelu(v, a.slope);
                    v = n < a.nout ? (float)vo : 0.f;
                    s1[j] += v;
                    s2[j] = __builtin_fmaf(v, v, s2[j]);          // (an explicit fma: left to hipcc, one instantiation contracts and another does not)
                    // 16-byte chunk c of row `row` lives at chunk c ^ (row & 7): conflict-free 16-byte reads below
                    const int col = j * 32 + l31;
                    tile[row * 64 + ((((col >> 3) ^ (row & 7)) << 3) | (col & 7))] = __builtin_bit_cast(unsigned short, vo);
                }
            }
        }
        // same-wave LDS hand-off: the ds ops of one wave complete in order; keep the compiler from moving the
        // (differently typed) reads above the writes
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        const int rr = lane >> 3, ch = lane & 7;
        const int n = n0 + wn * 64 + ch * 8;
        // gsum: the wave's 64 columns lie in one output part (n1 % 64 == 0, checked by the launcher): part, pitch and descriptor are
        // scalars, aux is read with 32-bit offsets (the part is below 4 GiB)
        const int gp = __builtin_amdgcn_readfirstlane(n0 + wn * 64) < a.n1 ? 0 : 1;
        const int gpc = gp ? a.nout - a.n1 : a.n1, gnl = n - (gp ? a.n1 : 0);
        const bool gon = GS && a.gred[gp] != nullptr;
        const bool gs = gon && n < a.nout;
        const __amdgpu_buffer_rsrc_t rsa = __builtin_amdgcn_make_buffer_rsrc((void*)a.gaux[gp], 0, gon ? 0xfffffff0u : 0u, 0x00020000);
        const unsigned ldab = (unsigned)a.ldgaux[gp] * 2u;
        float t1[8], t2[8];
        u32x4 gav[4 * TM];
        if constexpr (GS) {
#pragma unroll
            for (int e = 0; e < 8; ++e) t1[e] = t2[e] = 0.f;
            // every aux row of the lane first (the accumulators are dead by now: 32 registers are free), then the stores -- left to
            // itself hipcc also hoists the LDS reads and the store addresses of all eight rows and spills 200 registers
#pragma unroll
            for (int it = 0; it < 4 * TM; ++it) {
                const int row = it * 8 + rr;
                const int i = row >> 5, r32 = row & 31;
                const int py = 2 * TM * wm + 2 * i + (r32 >> 4), px = r32 & 15;
                const unsigned opix = (unsigned)((img * a.hi + (y0 + py)) * a.wi + (x0 + px));
                gav[it] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(rsa, opix * ldab + (unsigned)(n < a.nout ? gnl : 0) * 2u, 0, 0));
            }
            asm volatile("" ::: "memory");
        }
#pragma unroll
        for (int it = 0; it < 4 * TM; ++it) {
            const int row = it * 8 + rr;
            const u32x4 v = *(const u32x4*)(tile + row * 64 + ((ch ^ (row & 7)) << 3));
            const int i = row >> 5, r32 = row & 31;
            const int py = 2 * TM * wm + 2 * i + (r32 >> 4), px = r32 & 15;
            const size_t opix = ((size_t)img * a.hi + (y0 + py)) * a.wi + (x0 + px);
            if (!abl::nostore && n < a.nout) {
                if (n < a.n1)
                    *(u32x4*)((unsigned short*)a.y + opix * a.ldy + n) = v;
                else
                    *(u32x4*)((unsigned short*)a.y2 + opix * a.ldy2 + (n - a.n1)) = v;
            }
            if constexpr (GS) {
                gsum_wide_accum(v, gav[it], t1, t2);
                asm volatile("" ::: "memory");             // one row at a time
            }
        }
        if constexpr (GS) {
            if (gon) {                                     // wave-uniform
                const int slot = (prem * WGM + wm) % a.gslots;
                double* dst = gs ? a.gred[gp] + ((size_t)slot * a.gbatch * gpc + (size_t)img * gpc + gnl) * 2 : nullptr;
                gsum_wide_flush<8>(t1, t2, lane, dst);
            }
        }
    }
    // narrow path, gsum.  The 32 columns of a (wave, j) group lie in one output part (n1 % 32 == 0, checked by the launcher), so
    // "this group takes sums", its aux tensor and pitch are scalars: the sixteen aux loads of a 32 x 32 tile are issued back to
    // back in front of the tile's stores (a per-element conditional load made hipcc wait for every load AND the store before it:
    // 64 serialized round trips per wave tile).
    // (bf16 outputs take their sums in the LDS-staged path above: the launcher only fuses when that path's alignment conditions hold)
    const bool gs_any = GS && sizeof(TO) == 4 && (a.gred[0] != nullptr || a.gred[1] != nullptr);
    if constexpr (GS && sizeof(TO) == 4) if (!wide && gs_any) {
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int nb = __builtin_amdgcn_readfirstlane(n0 + wn * 64 + j * 32);
            const int gp = nb < a.n1 ? 0 : 1;
            const bool on = a.gred[gp] != nullptr && nb < a.nout;
            const int n = nb + l31;
            const int nl = n - (gp ? a.n1 : 0);
            const int pc = gp ? a.nout - a.n1 : a.n1;
            // aux through a scalar descriptor and 32-bit offsets (the part is below 4 GiB); zero-length when the group takes no sums
            const __amdgpu_buffer_rsrc_t rsa = __builtin_amdgcn_make_buffer_rsrc((void*)a.gaux[gp], 0, on ? 0xfffffff0u : 0u, 0x00020000);
            const unsigned ldab = (unsigned)a.ldgaux[gp] * (unsigned)sizeof(T), nlb = (unsigned)(n < a.nout ? nl : 0) * (unsigned)sizeof(T);
            // ... and so is the group's output part (the launcher fuses the sums only when the outputs are below 4 GiB).  A lane's
            // address is ONE register per 32 x 32 tile -- its pixel of accumulator row 0 -- plus a scalar offset per row (row r of a lane
            // is pixel (r >> 3, 8 ((r >> 2) & 1) + (r & 3)) of the tile's two patch rows): no address arithmetic and no address
            // registers in the element loops (with 64-bit element addresses hipcc kept a pixel index per row and spilled 37 of them
            // to scratch around the sixteen loads)
            const __amdgpu_buffer_rsrc_t rsy = __builtin_amdgcn_make_buffer_rsrc(gp ? a.y2 : a.y, 0, gp ? a.y2bytes : a.ybytes, 0x00020000);
            const unsigned ldyb = (unsigned)(gp ? a.ldy2 : a.ldy) * (unsigned)sizeof(TO), nyb = (unsigned)(n < a.nout ? nl : 0) * (unsigned)sizeof(TO);
#pragma unroll
            for (int i = 0; i < TM; ++i) {
                const unsigned pix0 = (unsigned)((img * a.hi + (y0 + 2 * TM * wm + 2 * i)) * a.wi + x0 + 4 * h);
                const unsigned ao = pix0 * ldab + nlb, yo = pix0 * ldyb + nyb;
                float q[16];
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const unsigned cr = (unsigned)((r >> 3) * a.wi + 8 * ((r >> 2) & 1) + (r & 3));         // scalar
                    if constexpr (sizeof(T) == 4)
                        q[r] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rsa, ao, cr * ldab, 0));
                    else
                        q[r] = __uint_as_float((unsigned)__builtin_amdgcn_raw_buffer_load_b16(rsa, ao, cr * ldab, 0) << 16);
                }
                if (n < a.nout) {
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const unsigned cr = (unsigned)((r >> 3) * a.wi + 8 * ((r >> 2) & 1) + (r & 3));
                        float v = acc[i][j][r] + bj[j];
                        const TO vo = (TO)shm_lrelu(v, a.slope);
                        v = (float)vo;
                        s1[j] += v;
                        s2[j] += v * q[r];
                        __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, vo), rsy, yo, cr * ldyb, 0);
                    }
                }
            }
            if (on) {
                const int slot = (prem * WGM + wm) % a.gslots;
                const float t1 = s1[j] + __shfl_xor(s1[j], 32, 64);
                const float t2 = s2[j] + __shfl_xor(s2[j], 32, 64);
                if (h == 0 && n < a.nout) {
                    double* dst = a.gred[gp] + ((size_t)slot * a.gbatch * pc + (size_t)img * pc + nl) * 2;
                    atomicAdd(dst, (double)t1);
                    atomicAdd(dst + 1, (double)t2);
                }
            }
        }
    }
    // plain element stores: as in the gsum path above, through a scalar descriptor with one address register per 32 x 32 tile and a
    // scalar offset per row when the outputs are below 4 GiB and a 32-column group lies in one output part
    const bool ybuf = !abl::nostore && a.ybytes != 0 && (a.y2 == nullptr || (a.y2bytes != 0 && a.n1 % 32 == 0));
    if (!wide && !gs_any && ybuf) {
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int nb = __builtin_amdgcn_readfirstlane(n0 + wn * 64 + j * 32);
            const int gp = nb < a.n1 ? 0 : 1;
            const int n = nb + l31;
            const __amdgpu_buffer_rsrc_t rsy = __builtin_amdgcn_make_buffer_rsrc(gp ? a.y2 : a.y, 0, gp ? a.y2bytes : a.ybytes, 0x00020000);
            const unsigned ldyb = (unsigned)(gp ? a.ldy2 : a.ldy) * (unsigned)sizeof(TO);
            const unsigned nyb = (unsigned)(n < a.nout ? n - (gp ? a.n1 : 0) : 0) * (unsigned)sizeof(TO);
            if (n < a.nout) {
#pragma unroll
                for (int i = 0; i < TM; ++i) {
                    const unsigned yo = (unsigned)((img * a.hi + (y0 + 2 * TM * wm + 2 * i)) * a.wi + x0 + 4 * h) * ldyb + nyb;
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const unsigned cr = (unsigned)((r >> 3) * a.wi + 8 * ((r >> 2) & 1) + (r & 3));         // scalar
                        float v = acc[i][j][r] + bj[j];
                        const TO vo = (TO)shm_lrelu(v, a.slope);
                        v = (float)vo;
                        s1[j] += v;
                        s2[j] = __builtin_fmaf(v, v, s2[j]);
                        if constexpr (sizeof(TO) == 4)
                            __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, vo), rsy, yo, cr * ldyb, 0);
                        else
                            __builtin_amdgcn_raw_buffer_store_b16(__builtin_bit_cast(unsigned short, vo), rsy, yo, cr * ldyb, 0);
                    }
                }
            }
        }
    }
    if (!wide && !gs_any && !ybuf) {
#pragma unroll
    for (int i = 0; i < TM; ++i) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = (r & 3) + 8 * (r >> 2) + 4 * h;
            const int py = 2 * TM * wm + 2 * i + (row >> 4), px = row & 15;
            const size_t opix = ((size_t)img * a.hi + (y0 + py)) * a.wi + (x0 + px);
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int n = n0 + wn * 64 + j * 32 + l31;
                if (n < a.nout) {
                    float v = acc[i][j][r] + bj[j];
                    const TO vo = (TO)shm_lrelu(v, a.slope);
                    v = (float)vo;
                    s1[j] += v;
                    s2[j] = __builtin_fmaf(v, v, s2[j]);          // (an explicit fma: left to hipcc, one instantiation contracts and another does not)
                    if (!abl::nostore || v == 123.456f)         // (timing-only build: keep the value live, store nothing)
                    {
                        if (n < a.n1)
                            ((TO*)a.y)[opix * a.ldy + n] = vo;
                        else
                            ((TO*)a.y2)[opix * a.ldy2 + (n - a.n1)] = vo;
                    }
                }
            }
        }
    }
    }
    if (a.stats) {
        const int slot = (prem * WGM + wm) % a.stats_slots;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            float t1 = s1[j] + __shfl_xor(s1[j], 32, 64);
            float t2 = s2[j] + __shfl_xor(s2[j], 32, 64);
            const int n = n0 + wn * 64 + j * 32 + l31;
            if (h == 0 && n < a.nout) {
                double* dst = a.stats + (size_t)slot * a.stats_stride + ((size_t)img * a.nout + n) * 2;
                atomicAdd(dst, (double)t1);
                atomicAdd(dst + 1, (double)t2);
            }
        }
    }
}

// One form: its instantiation and the name the profiler gives it (which ends at the last argument that is not a default)
template <typename T, typename TO, int BN, int PH = 16, bool ST = false, int TM = 2, bool GS = false, int NM = 0>
static void halo_launch(const TapGemmArgs& a, int batch, hipStream_t st) {
    hipLaunchKernelGGL((tapgemm_halo_kernel<T, TO, BN, PH, ST, TM, GS, NM>), dim3(batch * (a.hi / PH) * (a.wi / 16), shm_cdiv(a.nout, BN), 1), dim3(BN * PH / (2 * TM)), 0, st, a);
    shm_set_last_kernel("tapgemm_halo_kernel<%s, %s, %d, %d, %s, %d%s>", shm_tg_name<T>(), shm_tg_name<TO>(), BN, PH, ST ? "true" : "false", TM,
                        NM == 2 ? ", false, 2" : NM == 1 ? ", false, 1" : GS ? ", true" : "");
}

// The static-tap block of BN output channels: plain, with the gsum epilogue, or normalising its source (operands and outputs of one type)
template <typename T, typename TO, int BN>
static void halo_st_launch(const TapGemmArgs& a, const TapGemmPlan& p, int batch, hipStream_t st) {
    if (p.gs_fused)
        halo_launch<T, TO, BN, 16, true, 2, true>(a, batch, st);
    else if (a.nt) {
        if constexpr (sizeof(T) == sizeof(TO)) {
            if (a.ntmode)
                halo_launch<T, TO, BN, 16, true, 2, false, 2>(a, batch, st);
            else
                halo_launch<T, TO, BN, 16, true, 2, false, 1>(a, batch, st);
        }
    } else
        halo_launch<T, TO, BN, 16, true>(a, batch, st);
}

template <typename T, typename TO>
static int halo_launch_t(const TapGemmArgs& a, const TapGemmPlan& p, int batch, hipStream_t st, const char* who) {
    const int v = p.variant;
    // 8-row patches (3 four-wave blocks per CU, 4-wave barriers): measured equal or slower than 16-row patches in
    // bf16 (806-975 vs 795-994 TFLOP/s over the four big layer shapes).  Kept selectable.
    SHM_REQUIRE(v != SHM_TG_HALO128_PH8 || (p.halo_ok && sizeof(T) == 2), SHM_E_SHAPE, "%s: forced variant halo128/ph8 is bf16, unit-stride 3x3, map multiple of 16", who);
    SHM_REQUIRE(p.halo_ok, SHM_E_SHAPE, "%s: forced variant %s needs a unit-stride 3x3 layer on a map that is a multiple of 16", who,
                v == SHM_TG_HALO128 ? "halo128" : v == SHM_TG_HALO64 ? "halo64" : v == SHM_TG_HALO128_ST ? "halo128/static-taps" : v == SHM_TG_HALO64_ST ? "halo64/static-taps"
                                                                                                                                   : "halo128/static-taps/4 waves");
    switch (v) {
    case SHM_TG_HALO128: halo_launch<T, TO, 128>(a, batch, st); break;
    case SHM_TG_HALO64: halo_launch<T, TO, 64>(a, batch, st); break;
    case SHM_TG_HALO128_ST: halo_st_launch<T, TO, 128>(a, p, batch, st); break;
    case SHM_TG_HALO64_ST: halo_st_launch<T, TO, 64>(a, p, batch, st); break;
    case SHM_TG_HALO128_ST_W4: halo_launch<T, TO, 128, 16, true, 4>(a, batch, st); break;
    case SHM_TG_HALO128_PH8:
        if constexpr (sizeof(T) == 2) halo_launch<T, TO, 128, 8>(a, batch, st);
        break;
    }
    return SHM_OK;
}

int shm_halo_launch(const TapGemmArgs& a, const TapGemmPlan& p, int batch, int dtype, hipStream_t st, const char* who) {
    int rc = SHM_OK;
    SHM_DISPATCH_G(dtype, who, rc = halo_launch_t<T, TG>(a, p, batch, st, who));
    return rc;
}
