// tapgemm_dma_kernel: the LDS-DMA tap GEMM of conv_igemm.hip's header comment, and its eight SHM_TG_DMA_* tiles.
#include "tapgemm_dev.h"

#include <type_traits>

// ------------------------------------------------------------------------------------------
// LDS-DMA variant: operands go HBM/L2 -> LDS directly (buffer_load_dwordx4 ... lds), no VGPR
// staging and no ds_write.  One wave-instruction fills 16 LDS rows of 64 bytes (lane l -> byte
// 16*l of the destination), so rows are unpadded; bank conflicts of the ds_read_b128 fragment
// reads are removed by an XOR swizzle applied on the SOURCE side: LDS chunk q of row r holds
// channel chunk q ^ ((r >> 2) & 3).  Out-of-image taps / tail rows use byte offset 0xffffffff:
// the descriptor's range check makes the DMA write zeros (tools/probes/ldsdma_probe.hip).
// Three LDS stages; the DMA of step s+2 is issued right after the barrier of step s, waits are
// counted (s_waitcnt vmcnt(N)), barriers are raw s_barrier (a __syncthreads would drain vmcnt).
// T = float or bf16_t.  BK counts 4-byte words per LDS row (16 -> 64-byte rows); a K step covers
// BKE = BK*4/sizeof(T) channels.
template <typename T, typename TO, int BM, int BN, int WGM, int WGN, int NST, int BK>
// (eight-wave blocks with element-store epilogues: two blocks per CU fit in LDS, i.e. four waves per SIMD -- the second launch bound
// keeps them at 128 VGPRs, where hipcc left to itself lands between 121 and 155 depending on the epilogue code around the loop)
__global__ __launch_bounds__(64 * WGM * WGN, (WGM * WGN == 8 && sizeof(TO) == 4) ? 4 : 1) void tapgemm_dma_kernel(const TapGemmArgs a) {
    static_assert(BK == 16 || BK == 32, "K step of 16 words (64-byte LDS rows) or 32 (128-byte rows)");
    constexpr int ESZ = sizeof(T);
    constexpr int BKE = BK * 4 / ESZ;                // channels per K step
    constexpr int CHE = 16 / ESZ;                    // channels per 16-byte chunk
    constexpr int NW = WGM * WGN;                    // waves per block (4 or 8)
    constexpr int WTM = BM / WGM, WTN = BN / WGN;
    constexpr int TM = WTM / 32, TN = WTN / 32;
    constexpr int RPI = 256 / BK;                    // rows per DMA instruction (1 KiB)
    constexpr int CPR = BK / 4;                      // 16-byte chunks per row
    constexpr int SWS = BK == 16 ? 2 : 1, SWM = CPR - 1;      // swizzle: chunk ^= (row >> SWS) & SWM
    constexpr int NKK = BK / 8;                      // 8-wide k groups per step
    constexpr int NA = BM / (RPI * NW), NB = BN / (RPI * NW);   // DMA instructions per wave and stage
    static_assert(NA >= 1 && NB >= 1 && BM % (RPI * NW) == 0 && BN % (RPI * NW) == 0, "whole DMA instructions per wave");
    constexpr int NLD = NA + NB;
    constexpr int STAGE = (BM + BN) * BK;            // floats
    static_assert(NST >= 2 && NST <= 4, "NST stages: DMA NST-1 steps ahead");
    __shared__ __attribute__((aligned(1024))) float smem[NST * STAGE];

    const TapPhase& P = a.ph[blockIdx.z];
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l31 = lane & 31, h = lane >> 5;
    const int wm = wave / WGN, wn = wave % WGN;
    // (an XCD-aware tile order -- contiguous M ranges per XCD, N tiles innermost -- was measured
    // 1 % slower in fp32 (round 1) and 0.6 % slower on the whole bf16 step (round 2): the kernel is not L2/HBM bound)
    const int m0 = blockIdx.x * BM, n0 = blockIdx.y * BN;

    // DMA lane mapping: instruction j of this wave covers rows wave*(BM/4)+16j .. +15
    const int drow = lane / CPR, dq = lane % CPR;
    // Per row: byte offset of the centre pixel in each source, and a bitmask of the taps that fall
    // inside the image (bit t of okm) -- the per-step address work is one add and one select.
    unsigned rowb1[NA], rowb2[NA], okm[NA];
#pragma unroll
    for (int j = 0; j < NA; ++j) {
        const int row = wave * (BM / NW) + RPI * j + drow;
        const int m = m0 + row;
        const bool mv = m < a.M;
        const int mm = mv ? m : 0;
        const int ow = mm % a.wg, t = mm / a.wg;
        const int oh = t % a.hg, n = t / a.hg;
        const int ih0 = oh * a.is, iw0 = ow * a.is;
        const int pixbase = (n * a.hi + ih0) * a.wi + iw0;
        const int acoff = (dq ^ ((row >> SWS) & SWM)) * CHE;   // swizzled channel offset inside the K step
        rowb1[j] = (unsigned)(pixbase * a.ldx + acoff) * (unsigned)ESZ;
        rowb2[j] = (unsigned)(pixbase * a.ldx2 + acoff) * (unsigned)ESZ;
        unsigned mk = 0;
        for (int tp = 0; tp < P.ntaps; ++tp) {
            const int ih = ih0 + P.dh[tp], iw = iw0 + P.dw[tp];
            mk |= (mv && (unsigned)ih < (unsigned)a.hi && (unsigned)iw < (unsigned)a.wi) ? (1u << tp) : 0u;
        }
        okm[j] = mk;
    }
    unsigned wrow[NB];
#pragma unroll
    for (int j = 0; j < NB; ++j) {
        const int row = wave * (BN / NW) + RPI * j + drow;
        const int nn = n0 + row;
        wrow[j] = nn < a.nout ? (unsigned)(nn * a.K + (dq ^ ((row >> SWS) & SWM)) * CHE) * (unsigned)ESZ : 0xffffffffu;
    }
    const __amdgpu_buffer_rsrc_t rsx = __builtin_amdgcn_make_buffer_rsrc((void*)a.x, 0, a.xbytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t rsx2 = __builtin_amdgcn_make_buffer_rsrc((void*)a.x2, 0, a.x2bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t rsw = __builtin_amdgcn_make_buffer_rsrc((void*)a.w, 0, a.wbytes, 0x00020000);

    const int ntaps = P.ntaps;
    const int nch = a.K / BKE;
    const int ksteps = ntaps * nch;
    // The tap table lives in two VGPRs (lane t holds tap t) and is read with v_readlane: a scalar
    // memory load inside the K loop would share lgkmcnt with the ds_reads and force every fragment
    // wait to lgkmcnt(0) (SMEM returns out of order).
    const int tl = lane < ntaps ? lane : 0;
    const int tapoff_v = P.dh[tl] * a.wi + P.dw[tl];      // pixel displacement of tap `lane`
    const int tapw_v = P.widx[tl];                        // its weight slice
    int ld_g = 0, ld_tap = 0, ld_sub = 0, ld_c0 = 0;
    auto advance = [&]() {
        if (BK == 32) {                          // (chunk, tap): a step already covers a whole 128-B line
            if (++ld_tap == ntaps) {
                ld_tap = 0;
                ld_c0 += BKE;
            }
            return;
        }
        const int nsub = (nch - ld_g) >= 2 ? 2 : 1;
        if (++ld_sub == nsub) {
            ld_sub = 0;
            if (++ld_tap == ntaps) {
                ld_tap = 0;
                ld_g += 2;
            }
        }
        ld_c0 = (ld_g + ld_sub) * BKE;
    };
    typedef __attribute__((address_space(3))) void* lds_ptr;
    // the two pixel pitches as opaque scalars: hipcc otherwise re-reads the selected one from the kernel arguments in every K step -- a
    // scalar memory load whose s_waitcnt lgkmcnt(0) also drains the wave's ds_reads (found in the ISA of the 256 x 128 tile)
    int ldx_s = a.ldx, ldx2_s = a.ldx2;
    asm volatile("" : "+s"(ldx_s), "+s"(ldx2_s));
    auto dma = [&](int stage) {
        float* sa = smem + stage * STAGE + wave * (BM / NW) * BK;
        float* sb = smem + stage * STAGE + BM * BK + wave * (BN / NW) * BK;
        const int c0 = ld_c0;
        const bool second = c0 >= a.c1;
        const int ld = second ? ldx2_s : ldx_s;
        const int cc = second ? c0 - a.c1 : c0;
        const int t_off = __builtin_amdgcn_readlane(tapoff_v, ld_tap);
        const int t_wi = __builtin_amdgcn_readlane(tapw_v, ld_tap);
        const unsigned stepb = (unsigned)(t_off * ld + cc) * (unsigned)ESZ;          // wave-uniform
        const unsigned tbit = 1u << ld_tap;
#pragma unroll
        for (int j = 0; j < NA; ++j) {
            unsigned off = (okm[j] & tbit) ? (second ? rowb2[j] : rowb1[j]) + stepb : 0xffffffffu;
            if constexpr (abl::fixaddr) off = rowb1[j];                       // timing only: constant address, no per-step work
            if constexpr (abl::sameline) off = (okm[j] & tbit) ? (unsigned)(dq * 16 + (off & 0x40u)) : 0xffffffffu;      // timing only
            if (second)
                __builtin_amdgcn_raw_ptr_buffer_load_lds(rsx2, (lds_ptr)(sa + j * 256), 16, (int)off, 0, 0, 0);
            else
                __builtin_amdgcn_raw_ptr_buffer_load_lds(rsx, (lds_ptr)(sa + j * 256), 16, (int)off, 0, 0, 0);
        }
        const unsigned wbase = (unsigned)((t_wi * a.nout) * a.K + c0) * (unsigned)ESZ;
#pragma unroll
        for (int j = 0; j < NB; ++j) {
            unsigned off = wrow[j] == 0xffffffffu ? 0xffffffffu : wrow[j] + wbase;
            if constexpr (abl::fixaddr || abl::sameline) off = wrow[j] == 0xffffffffu ? 0xffffffffu : (unsigned)(dq * 16);
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rsw, (lds_ptr)(sb + j * 256), 16, (int)off, 0, 0, 0);
        }
        if constexpr (!abl::fixaddr) advance();
    };

    f32x16 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    // fragment reads: row = tile row (l31 + 32*i), logical chunk 2*kk+h, physical chunk ^ swizzle(row)
    const int sw = (l31 >> SWS) & SWM;
    int fo[NKK];
#pragma unroll
    for (int kk = 0; kk < NKK; ++kk) fo[kk] = l31 * BK + ((2 * kk + h) ^ sw) * 4;       // floats
    auto compute = [&](int stage) {
        const float* Ab = smem + stage * STAGE + wm * WTM * BK;
        const float* Bb = smem + stage * STAGE + BM * BK + wn * WTN * BK;
#pragma unroll
        for (int kk = 0; kk < NKK; ++kk) {
            f32x4 av[TM], bv[TN];
#pragma unroll
            for (int i = 0; i < TM; ++i) av[i] = *(const f32x4*)(Ab + i * 32 * BK + fo[kk]);
#pragma unroll
            for (int j = 0; j < TN; ++j) bv[j] = *(const f32x4*)(Bb + j * 32 * BK + fo[kk]);
            tap_mfma<T, TM, TN>(av, bv, acc);
        }
    };

    constexpr int AHEAD = NST - 1;                  // stages in flight beyond the one being computed
#pragma unroll
    for (int t = 0; t < AHEAD; ++t)
        if (t < ksteps) dma(t);
    int cur = 0, nxt = AHEAD % NST;
    for (int s = 0; s < ksteps; ++s) {
        // stage s must have landed: everything but the DMAs of the (up to AHEAD-1) stages issued after it
        const int younger = min(AHEAD - 1, ksteps - 1 - s);
        if (younger >= 2)
            asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * NLD) : "memory");
        else if (younger == 1)
            asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NLD) : "memory");
        else
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        SHM_LDS_BARRIER();          // all waves: stage s landed, compute(s-1) finished
        asm volatile("" ::: "memory");
        if constexpr (!abl::nodma)
            if (s + AHEAD < ksteps) dma(nxt);      // overwrites the buffer compute(s-1) was reading
        compute(cur);
        asm volatile("" ::: "memory");
        cur = (cur == NST - 1) ? 0 : cur + 1;
        nxt = (nxt == NST - 1) ? 0 : nxt + 1;
    }

    const bool direct = (a.os == 1);
    float s1[TN], s2[TN];
#pragma unroll
    for (int j = 0; j < TN; ++j) s1[j] = s2[j] = 0.f;
    // the bias of the lane's columns, once: read inside the store loops it is re-fetched per element (the stores may alias it for
    // all hipcc knows) and every fetch waits with vmcnt(0), i.e. for the stores of the element before as well -- the epilogue
    // became a chain of store round trips
    float bj[TN];
#pragma unroll
    for (int j = 0; j < TN; ++j) {
        const int n = n0 + wn * WTN + j * 32 + l31;
        bj[j] = (a.bias && n < a.nout) ? a.bias[n] : 0.f;
        // consume the value here, in straight-line code: first used inside the exec-masked element blocks below, hipcc's waitcnt
        // pass keeps the load "pending" along the skipped paths and puts s_waitcnt vmcnt(0) -- a drain of the stores -- in
        // front of every element
        asm volatile("" : "+v"(bj[j]));
    }
    // bf16 outputs (round 2): as in the halo kernels the wave's tile goes through LDS (free once every wave is past its last
    // fragment read) and leaves as 16-byte stores -- the accumulator layout gives a lane one 2-byte element per row, i.e.
    // TM*TN*16 two-byte store instructions per wave.  Works for the strided (four-phase) outputs too: a pixel's channels are
    // contiguous whatever the pixel stride.
    constexpr bool kWide = sizeof(TO) == 2 && WTM * WTN * 2 * NW <= NST * STAGE * 4;
    const bool wide = kWide && (a.nout % 8 == 0) && (a.n1 % 8 == 0) && (a.ldy % 8 == 0) && (((size_t)a.y & 15) == 0) &&
                      (a.y2 == nullptr || ((a.ldy2 % 8 == 0) && (((size_t)a.y2 & 15) == 0)));
    if constexpr (kWide) if (wide) {
        constexpr int CW = WTN / 8;                      // 16-byte chunks per tile row
        constexpr int RPW = 64 / CW;                     // tile rows per store instruction
        __syncthreads();
        unsigned short* tile = (unsigned short*)smem + wave * (WTM * WTN);
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = i * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
                const bool mv = m0 + wm * WTM + row < a.M;
#pragma unroll
                for (int j = 0; j < TN; ++j) {
                    const int n = n0 + wn * WTN + j * 32 + l31;
                    float v = acc[i][j][r] + bj[j];
                    const TO vo = (TO)shm_lrelu(v, a.slope);
                    v = (mv && n < a.nout) ? (float)vo : 0.f;          // statistics of the value as stored
                    s1[j] += v;
                    s2[j] = __builtin_fmaf(v, v, s2[j]);          // (an explicit fma: left to hipcc, one instantiation contracts and another does not)
                    const int col = j * 32 + l31;
                    tile[row * WTN + ((((col >> 3) ^ (row & (CW - 1))) << 3) | (col & 7))] = __builtin_bit_cast(unsigned short, vo);
                }
            }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");        // same-wave LDS hand-off
        const int rr = lane / CW, ch = lane % CW;
        const int n = n0 + wn * WTN + ch * 8;
        int gnl, gpc;
        const int gp = gsum_part(a, n, gnl, gpc);
        const bool gs = a.gred[gp] != nullptr && n < a.nout;         // per lane: its eight channels lie in one part
        const unsigned short* gaux = (const unsigned short*)a.gaux[gp] + gnl;
        float t1[8], t2[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) t1[e] = t2[e] = 0.f;
#pragma unroll
        for (int it = 0; it < WTM / RPW; ++it) {
            const int row = it * RPW + rr;
            const u32x4 v = *(const u32x4*)(tile + row * WTN + ((ch ^ (row & (CW - 1))) << 3));
            const int m = m0 + wm * WTM + row;
            if (m < a.M && n < a.nout) {
                size_t opix;
                if (direct) {
                    opix = (size_t)m;
                } else {
                    const int ow = m % a.wg, t = m / a.wg;
                    const int oh = t % a.hg, ni = t / a.hg;
                    opix = ((size_t)ni * a.ho + (oh * a.os + P.oph)) * a.wo + (ow * a.os + P.opw);
                }
                if (n < a.n1)
                    *(u32x4*)((unsigned short*)a.y + opix * a.ldy + n) = v;
                else
                    *(u32x4*)((unsigned short*)a.y2 + opix * a.ldy2 + (n - a.n1)) = v;
                if (gs) gsum_wide_accum(v, *(const u32x4*)(gaux + opix * a.ldgaux[gp]), t1, t2);
            }
        }
        if (a.gred[0] || a.gred[1]) {                      // wave-uniform
            const int mw = m0 + wm * WTM;
            const int img = mw / a.hw;
            const int slot = ((mw - img * a.hw) / WTM) % a.gslots;
            double* dst = (gs && mw < a.M) ? a.gred[gp] + ((size_t)slot * a.gbatch * gpc + (size_t)img * gpc + gnl) * 2 : nullptr;
            gsum_wide_flush<CW>(t1, t2, lane, dst);
        }
    }
    // narrow path, gsum.  The 32 columns of a (wave, j) group lie in one output part (n1 % 32 == 0, checked by the launcher), so
    // "this group takes sums", its aux tensor and pitch are scalars: the sixteen aux loads of a 32 x 32 tile are issued back to
    // back in front of the tile's stores (a per-element conditional load made hipcc wait for every load AND the store before it).
    const bool gs_any = a.gred[0] != nullptr || a.gred[1] != nullptr;
    auto out_pix = [&](int m) -> size_t {
        if (direct) return (size_t)m;
        const int ow = m % a.wg, t = m / a.wg;
        const int oh = t % a.hg, n = t / a.hg;
        return ((size_t)n * a.ho + (oh * a.os + P.oph)) * a.wo + (ow * a.os + P.opw);
    };
    // Element stores (and the gsum aux loads) without per-element address arithmetic: the rows of a lane's 32 x 32 accumulator tile are
    // GEMM rows mb + 8 g + 4 h + e (g = r >> 2, e = r & 3, mb a multiple of 32), so when the phase grid is a multiple of 8 pixels wide
    // the output pixel of a row is a SCALAR -- (n, oh, ow) of row mb + 8 g, four scalar decompositions per tile -- plus e and 4 h pixel
    // steps: one per-lane address register for the whole wave tile, everything else in the instruction's scalar offset.  (Per
    // element it was a 64-bit address from two integer divisions: ~40 VALU instructions, 64 elements per lane.)  Needs outputs below
    // 4 GiB (scalar descriptors) and every 32-column group inside one output part.
    const bool fastep = !abl::nostore && a.ybytes != 0 && (a.y2 == nullptr || (a.y2bytes != 0 && a.n1 % 32 == 0)) && (direct || a.wg % 8 == 0) &&
                        a.M % 8 == 0;
    if (!wide && fastep) {
        unsigned sp[TM][4];                // scalar: output pixel of GEMM row mb + 8 g of tile i (one decomposition per tile, then steps of 8)
        bool sv[TM][4];                    // ... and whether that row group exists (M % 8 == 0)
#pragma unroll
        for (int i = 0; i < TM; ++i) {
            const int mb = __builtin_amdgcn_readfirstlane(m0 + wm * WTM + i * 32);
            int ow = mb % a.wg, t = mb / a.wg;
            int oh = t % a.hg, ni = t / a.hg;
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                sv[i][g] = mb + 8 * g < a.M;
                sp[i][g] = direct ? (unsigned)(mb + 8 * g) : (unsigned)((ni * a.ho + (oh * a.os + P.oph)) * a.wo + (ow * a.os + P.opw));
                ow += 8;
                if (ow >= a.wg) {          // wg % 8 == 0: a step of 8 ends exactly on the row end
                    ow = 0;
                    if (++oh == a.hg) {
                        oh = 0;
                        ++ni;
                    }
                }
            }
        }
        auto elem_stores = [&](auto gsx) {
            constexpr bool GSX = decltype(gsx)::value;
#pragma unroll
        for (int j = 0; j < TN; ++j) {
            const int nb = __builtin_amdgcn_readfirstlane(n0 + wn * WTN + j * 32);
            const int gp = nb < a.n1 ? 0 : 1;
            const bool on = GSX && a.gred[gp] != nullptr && nb < a.nout;
            const int n = nb + l31;
            const int nl = n - (gp ? a.n1 : 0);
            const int pc = gp ? a.nout - a.n1 : a.n1;
            const __amdgpu_buffer_rsrc_t rsy = __builtin_amdgcn_make_buffer_rsrc(gp ? a.y2 : a.y, 0, gp ? a.y2bytes : a.ybytes, 0x00020000);
            const __amdgpu_buffer_rsrc_t rsa = __builtin_amdgcn_make_buffer_rsrc((void*)a.gaux[gp], 0, on ? 0xfffffff0u : 0u, 0x00020000);
            const unsigned ldyb = (unsigned)(gp ? a.ldy2 : a.ldy) * (unsigned)sizeof(TO), ldab = (unsigned)a.ldgaux[gp] * (unsigned)sizeof(T);
            const unsigned lanepix = (unsigned)(4 * h * a.os);
            const unsigned yo = lanepix * ldyb + (unsigned)(n < a.nout ? nl : 0) * (unsigned)sizeof(TO);
            const unsigned ao = lanepix * ldab + (unsigned)(n < a.nout ? nl : 0) * (unsigned)sizeof(T);
#pragma unroll
            for (int i = 0; i < TM; ++i) {
                [[maybe_unused]] float q[GSX ? 16 : 1];
#pragma unroll
                for (int r = 0; r < (GSX ? 16 : 1); ++r) q[r] = 0.f;
                if constexpr (GSX) if (on) {
#pragma unroll
                    for (int g = 0; g < 4; ++g)
                        if (sv[i][g]) {
#pragma unroll
                            for (int e = 0; e < 4; ++e) {
                                const unsigned so = (sp[i][g] + (unsigned)(e * a.os)) * ldab;
                                if constexpr (sizeof(T) == 4)
                                    q[4 * g + e] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rsa, ao, so, 0));
                                else
                                    q[4 * g + e] = __uint_as_float((unsigned)__builtin_amdgcn_raw_buffer_load_b16(rsa, ao, so, 0) << 16);
                            }
                        }
                }
                if (n < a.nout) {
#pragma unroll
                    for (int g = 0; g < 4; ++g)
                        if (sv[i][g]) {
#pragma unroll
                            for (int e = 0; e < 4; ++e) {
                                const int r = 4 * g + e;
                                float v = acc[i][j][r] + bj[j];
                                const TO vo = (TO)shm_lrelu(v, a.slope);
                                v = (float)vo;                       // statistics of the value as stored
                                s1[j] += v;
                                if constexpr (GSX)
                                    s2[j] += v * q[r];
                                else
                                    s2[j] = __builtin_fmaf(v, v, s2[j]);
                                const unsigned so = (sp[i][g] + (unsigned)(e * a.os)) * ldyb;
                                if constexpr (sizeof(TO) == 4)
                                    __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, vo), rsy, yo, so, 0);
                                else
                                    __builtin_amdgcn_raw_buffer_store_b16(__builtin_bit_cast(unsigned short, vo), rsy, yo, so, 0);
                            }
                        }
                }
            }
            const int mw = m0 + wm * WTM;
            if (on && mw < a.M) {
                const int img = mw / a.hw;
                const int slot = ((mw - img * a.hw) / WTM) % a.gslots;
                const float t1 = s1[j] + __shfl_xor(s1[j], 32, 64);
                const float t2 = s2[j] + __shfl_xor(s2[j], 32, 64);
                if (h == 0 && n < a.nout) {
                    double* dst = a.gred[gp] + ((size_t)slot * a.gbatch * pc + (size_t)img * pc + nl) * 2;
                    atomicAdd(dst, (double)t1);
                    atomicAdd(dst + 1, (double)t2);
                }
            }
        }
        };
        if (gs_any)
            elem_stores(std::true_type{});
        else
            elem_stores(std::false_type{});
    }
    if (!wide && gs_any && !fastep) {
#pragma unroll
        for (int j = 0; j < TN; ++j) {
            const int nb = __builtin_amdgcn_readfirstlane(n0 + wn * WTN + j * 32);
            const int gp = nb < a.n1 ? 0 : 1;
            const bool on = a.gred[gp] != nullptr && nb < a.nout;
            const int n = nb + l31;
            const int nl = n - (gp ? a.n1 : 0);
            const int pc = gp ? a.nout - a.n1 : a.n1;
            const T* gaux = (const T*)a.gaux[gp] + (n < a.nout ? nl : 0);
            const size_t ldg = (size_t)a.ldgaux[gp];
#pragma unroll
            for (int i = 0; i < TM; ++i) {
                float q[16];
                if (on) {
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int m = m0 + wm * WTM + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
                        q[r] = m < a.M ? (float)gaux[out_pix(m) * ldg] : 0.f;
                    }
                } else {
#pragma unroll
                    for (int r = 0; r < 16; ++r) q[r] = 0.f;
                }
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int m = m0 + wm * WTM + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
                    if (m >= a.M || n >= a.nout) continue;
                    const size_t opix = out_pix(m);
                    float v = acc[i][j][r] + bj[j];
                    const TO vo = (TO)shm_lrelu(v, a.slope);
                    v = (float)vo;
                    s1[j] += v;
                    s2[j] += v * q[r];
                    if (n < a.n1)
                        ((TO*)a.y)[opix * a.ldy + n] = vo;
                    else
                        ((TO*)a.y2)[opix * a.ldy2 + (n - a.n1)] = vo;
                }
            }
            const int mw = m0 + wm * WTM;
            if (on && mw < a.M) {
                const int img = mw / a.hw;
                const int slot = ((mw - img * a.hw) / WTM) % a.gslots;
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
    if (!wide && !gs_any && !fastep) {
#pragma unroll
    for (int i = 0; i < TM; ++i) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = (r & 3) + 8 * (r >> 2) + 4 * h;
            const int m = m0 + wm * WTM + i * 32 + row;
            if (m >= a.M) continue;
            const size_t opix = out_pix(m);
#pragma unroll
            for (int j = 0; j < TN; ++j) {
                const int n = n0 + wn * WTN + j * 32 + l31;
                if (n < a.nout) {
                    float v = acc[i][j][r] + bj[j];
                    const TO vo = (TO)shm_lrelu(v, a.slope);
                    v = (float)vo;                       // statistics of the value as stored
                    s1[j] += v;
                    s2[j] = __builtin_fmaf(v, v, s2[j]);          // (an explicit fma: left to hipcc, one instantiation contracts and another does not)
                    if (n < a.n1)
                        ((TO*)a.y)[opix * a.ldy + n] = vo;
                    else
                        ((TO*)a.y2)[opix * a.ldy2 + (n - a.n1)] = vo;
                }
            }
        }
    }
    }
    // InstanceNorm statistics of the tile just written: the 64 rows of a wave belong to one sample
    // (hw % 64 == 0), so one f64 atomic per (wave, column, moment).
    // InstanceNorm statistics of the tile just written: the 64 rows of a wave belong to one sample
    // (hw % 64 == 0), so one f64 atomic per (wave, column, moment).  (Combining the row-waves of a block
    // through LDS first was measured: the two extra block barriers cost more than the atomics they save,
    // -3.5 % fp32 / -12 % bf16 on this kernel.)
    if (a.stats) {
        const int mw = m0 + wm * WTM;
        if (mw < a.M) {
            const int img = mw / a.hw;
            const int slot = ((mw - img * a.hw) / WTM) % a.stats_slots;
#pragma unroll
            for (int j = 0; j < TN; ++j) {
                float t1 = s1[j] + __shfl_xor(s1[j], 32, 64);
                float t2 = s2[j] + __shfl_xor(s2[j], 32, 64);
                const int n = n0 + wn * WTN + j * 32 + l31;
                if (h == 0 && n < a.nout) {
                    double* dst = a.stats + (size_t)slot * a.stats_stride + ((size_t)img * a.nout + n) * 2;
                    atomicAdd(dst, (double)t1);
                    atomicAdd(dst + 1, (double)t2);
                }
            }
        }
    }
}

// One tile: its instantiation and the name the profiler gives it
template <typename T, typename TO, int BM, int BN, int WGM, int WGN, int NST, int BK>
static void dma_launch(const TapGemmArgs& a, int nphase, hipStream_t st) {
    hipLaunchKernelGGL((tapgemm_dma_kernel<T, TO, BM, BN, WGM, WGN, NST, BK>), dim3(shm_cdiv(a.M, BM), shm_cdiv(a.nout, BN), nphase), dim3(64 * WGM * WGN), 0, st, a);
    shm_set_last_kernel("tapgemm_dma_kernel<%s, %s, %d, %d, %d, %d, %d, %d>", shm_tg_name<T>(), shm_tg_name<TO>(), BM, BN, WGM, WGN, NST, BK);
}

template <typename T, typename TO>
static int dma_launch_t(const TapGemmArgs& a, const TapGemmPlan& p, int nphase, hipStream_t st, const char* who) {
    SHM_REQUIRE(p.variant != SHM_TG_DMA_128x128_BK32 || p.bk32_ok, SHM_E_SHAPE, "%s: forced variant bk32 needs channel counts that are multiples of %d", who,
                2 * 64 / (int)sizeof(T));
    switch (p.variant) {
    case SHM_TG_DMA_128x128: dma_launch<T, TO, 128, 128, 2, 2, 3, 16>(a, nphase, st); break;
    case SHM_TG_DMA_64x128: dma_launch<T, TO, 64, 128, 2, 2, 3, 16>(a, nphase, st); break;
    case SHM_TG_DMA_128x64: dma_launch<T, TO, 128, 64, 2, 2, 3, 16>(a, nphase, st); break;
    case SHM_TG_DMA_64x64: dma_launch<T, TO, 64, 64, 2, 2, 3, 16>(a, nphase, st); break;
    case SHM_TG_DMA_256x64: dma_launch<T, TO, 256, 64, 4, 1, 3, 16>(a, nphase, st); break;
    case SHM_TG_DMA_256x128: dma_launch<T, TO, 256, 128, 4, 2, 3, 16>(a, nphase, st); break;
    case SHM_TG_DMA_128x128_BK32: dma_launch<T, TO, 128, 128, 2, 2, 2, 32>(a, nphase, st); break;
    case SHM_TG_DMA_128x128_NST4: dma_launch<T, TO, 128, 128, 2, 2, 4, 16>(a, nphase, st); break;
    }
    return SHM_OK;
}

int shm_dma_launch(const TapGemmArgs& a, const TapGemmPlan& p, int nphase, int dtype, hipStream_t st, const char* who) {
    int rc = SHM_OK;
    SHM_DISPATCH_G(dtype, who, rc = dma_launch_t<T, TG>(a, p, nphase, st, who));
    return rc;
}
