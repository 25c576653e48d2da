// wgrad_kernel / wgrad_bf16_kernel: the generic weight-gradient kernels (any 1x1 / 3x3 layer, either stride, both concat sources in one tile);
// see conv_wgrad.hip's header comment.
#include "wgrad.h"

// Stage = 8 pixels.  Thread -> (half, k, c4): pixel slot k (0..7), 4-channel lane c4 (0..15), and
// the taps {half, half+2, ...}.  Two LDS stages + two register sets (loads two stages ahead),
// raw buffer loads with out-of-range offsets for padding / tails (no divergent load branches).
// STRADDLE: the 64-channel tile may contain channels of both concat sources (c1 % 64 != 0; only the
// small-filter test configurations): every X load is then issued against both descriptors with one
// of them masked out of range, so the descriptor stays wave-uniform (no waterfall loop).
template <int NT, bool STRADDLE>
__global__ __launch_bounds__(256, 2) void wgrad_kernel(const WgradArgs a) {
    constexpr int BKP = 8;
    constexpr int NTL = (NT + 1) / 2;          // tap loads per thread
    __shared__ __attribute__((aligned(16))) float Xs[2][NT][BKP][64];
    __shared__ __attribute__((aligned(16))) float Ds[2][BKP][64];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l31 = lane & 31, h = lane >> 5;
    const int mi = wave >> 1, ni = wave & 1;
    // XCD-aware block order (round 3, as in the bf16 kernels): the blocks of one pixel split -- same operand tiles, different
    // (ci, co) tile -- are dealt to ONE XCD's L2 instead of eight (r02 PMC: 969 MB HBM-side per launch, L2 hit rate 0.38)
    const Blk3 blk = xcd_block_order();
    const int ci0 = blk.x * 64, co0 = blk.y * 64;
    const int p_begin = blk.z * a.pix_per_split;
    const int p_end = min(a.M, p_begin + a.pix_per_split);
    const int nstages = (p_end - p_begin + BKP - 1) / BKP;

    const int half = __builtin_amdgcn_readfirstlane(tid >> 7);      // wave-uniform: waves 0,1 / 2,3
    const int k = (tid >> 4) & 7, c4 = tid & 15;
    const int c = ci0 + c4 * 4;
    const bool second = STRADDLE ? (c >= a.c1) : (ci0 >= a.c1);
    const bool xvalid = c < a.cin_ld;
    const int ld = second ? a.ldx2 : a.ldx;
    const int cc = second ? c - a.c1 : c;
    const __amdgpu_buffer_rsrc_t rs1 = __builtin_amdgcn_make_buffer_rsrc((void*)a.x, 0, a.xbytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t rs2 = __builtin_amdgcn_make_buffer_rsrc((void*)a.x2, 0, a.x2bytes, 0x00020000);
    // tap table of this wave pair, hoisted out of the loop (wave-uniform -> SGPRs)
    constexpr int KS = NT == 9 ? 3 : 1;
    int tofb[NTL];            // byte offset of tap j relative to the centre pixel
    unsigned tbit[NTL];       // its bit in the 9-bit validity mask (0: tap not owned by this wave)
#pragma unroll
    for (int j = 0; j < NTL; ++j) {
        const int t = half + 2 * j;
        const bool tv = t < NT;
        const int tt = tv ? t : 0;
        tofb[j] = (a.dh[tt] * a.wi + a.dw[tt]) * ld * 4;
        tbit[j] = tv ? (1u << tt) : 0u;
    }
    int rdh[KS], cdw[KS];     // the KS distinct row / column displacements (tap = kh*KS + kw)
#pragma unroll
    for (int i = 0; i < KS; ++i) {
        rdh[i] = a.dh[i * KS];
        cdw[i] = a.dw[i];
    }
    const __amdgpu_buffer_rsrc_t rsd = __builtin_amdgcn_make_buffer_rsrc((void*)a.dy, 0, a.dybytes, 0x00020000);
    const int co = co0 + c4 * 4;
    const bool dvalid = (co < a.cout) && half == 0;

    // running pixel coordinate of this thread's slot (advances by BKP per stage)
    int p = p_begin + k;
    int ow, oh, n;
    {
        const int pp = p < a.M ? p : 0;
        ow = pp % a.wo;
        const int t2 = pp / a.wo;
        oh = t2 % a.ho;
        n = t2 / a.ho;
    }

    f32x16 acc[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;

    auto gload = [&](f32x4 (&rx)[NTL], f32x4& rd) {
        const bool ok = p < p_end;
        const int ihb = oh * a.is, iwb = ow * a.is;
        const unsigned base = (unsigned)(((n * a.hi + ihb) * a.wi + iwb) * ld + cc) * 4u;
        // 9-bit tap validity mask of this pixel: bit kh*KS+kw = row kh inside AND column kw inside
        unsigned rm = 0, cm = 0;
#pragma unroll
        for (int i = 0; i < KS; ++i) {
            rm |= ((unsigned)(ihb + rdh[i]) < (unsigned)a.hi ? 1u : 0u) << i;
            cm |= ((unsigned)(iwb + cdw[i]) < (unsigned)a.wi ? 1u : 0u) << i;
        }
        unsigned m9 = 0;
#pragma unroll
        for (int i = 0; i < KS; ++i) m9 |= (rm & (1u << i)) ? (cm << (i * KS)) : 0u;
        if (!(ok && xvalid)) m9 = 0;
#pragma unroll
        for (int j = 0; j < NTL; ++j) {
            unsigned off = (m9 & tbit[j]) ? base + (unsigned)tofb[j] : 0xffffffffu;
            if constexpr (abl::sameline) off = (m9 & tbit[j]) ? (unsigned)(c4 * 16 + (off & 0x300u)) : 0xffffffffu;        // timing only
            if (STRADDLE) {
                u32x4 v1 = __builtin_amdgcn_raw_buffer_load_b128(rs1, (int)(second ? 0xffffffffu : off), 0, 0);
                u32x4 v2 = __builtin_amdgcn_raw_buffer_load_b128(rs2, (int)(second ? off : 0xffffffffu), 0, 0);
                rx[j] = __builtin_bit_cast(f32x4, v1 | v2);
            } else {
                u32x4 v1 = second ? __builtin_amdgcn_raw_buffer_load_b128(rs2, (int)off, 0, 0)
                                  : __builtin_amdgcn_raw_buffer_load_b128(rs1, (int)off, 0, 0);
                rx[j] = __builtin_bit_cast(f32x4, v1);
            }
        }
        const unsigned offd = (ok && dvalid) ? (unsigned)(p * a.lddy + co) * 4u : 0xffffffffu;
        rd = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rsd, (int)offd, 0, 0));
        // advance to the next stage
        p += BKP;
        ow += BKP;
        if (ow >= a.wo) {                      // at most one wrap when wo >= BKP (every real layer)
            do {
                ow -= a.wo;
                if (++oh == a.ho) {
                    oh = 0;
                    ++n;
                }
            } while (ow >= a.wo);
        }
    };
    auto sstore = [&](int buf, const f32x4 (&rx)[NTL], const f32x4& rd) {
#pragma unroll
        for (int j = 0; j < NTL; ++j) {
            const int t = half + 2 * j;
            if (t < NT) *(f32x4*)(&Xs[buf][t][k][c4 * 4]) = rx[j];
        }
        if (half == 0) *(f32x4*)(&Ds[buf][k][c4 * 4]) = rd;
    };
    auto compute = [&](int buf) {
#pragma unroll
        for (int kk = 0; kk < BKP / 2; ++kk) {
            const int kr = 2 * kk + h;
            const float bv = Ds[buf][kr][ni * 32 + l31];
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                const float av = Xs[buf][t][kr][mi * 32 + l31];
                acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv, acc[t], 0, 0, 0);
            }
        }
    };

    if (nstages > 0) {
        f32x4 rx0[NTL], rx1[NTL], rd0, rd1;
        gload(rx0, rd0);
        if (nstages > 1) gload(rx1, rd1);
        sstore(0, rx0, rd0);
        __syncthreads();
        int s = 0;
#define WG_BAR()                                  \
    do {                                          \
        if constexpr (!abl::nobar) __syncthreads(); \
    } while (0)
#define WG_GLOAD(a_, b_)                            \
    do {                                            \
        if constexpr (!abl::noload) gload(a_, b_);    \
    } while (0)
#define WG_SSTORE(i_, a_, b_)                            \
    do {                                                 \
        if constexpr (!abl::nostore) sstore(i_, a_, b_);   \
    } while (0)
        for (; s + 3 < nstages; s += 2) {
            WG_GLOAD(rx0, rd0);
            compute(0);
            WG_SSTORE(1, rx1, rd1);
            WG_BAR();
            WG_GLOAD(rx1, rd1);
            compute(1);
            WG_SSTORE(0, rx0, rd0);
            WG_BAR();
        }
        const int left = nstages - s;
        if (left >= 3) gload(rx0, rd0);
        compute(0);
        if (left >= 2) {
            sstore(1, rx1, rd1);
            __syncthreads();
            compute(1);
            if (left >= 3) {
                sstore(0, rx0, rd0);
                __syncthreads();
                compute(0);
            }
        }
    }

    // partial slab [split][tap][cin][cout]
    wgrad_store_slab<NT, false>(acc, a.part + (size_t)blk.z * NT * a.cin * a.cout, a.cin, a.cout, ci0, mi, h, co0 + ni * 32 + l31, nullptr);
}

// ------------------------------------------------------------------------------------------
// bf16 operands, fp32 accumulation: v_mfma_f32_32x32x16_bf16 contracts 16 pixels per instruction.
// Both operands are pixel-major ([pixel][channel], channels contiguous) but the MFMA wants, per lane,
// 8 consecutive PIXELS of one channel: the LDS image keeps the HBM layout (128-byte rows of 64
// channels) and the fragments are fetched with ds_read_b64_tr_b16 (hardware transpose: a 16-lane group
// reads a 4-pixel x 16-channel block column-major).  Rows whose index has bit 1 set hold their two
// 64-byte halves swapped, which makes the four rows x two channel blocks a 32-lane half reads hit 32
// distinct 8-byte bank pairs.  Stage = 16 pixels; same work split, split-K slabs and (register
// staged, two-stages-ahead) pipeline as wgrad_kernel.
template <int NT, bool STRADDLE>
__global__ __launch_bounds__(256, 2) void wgrad_bf16_kernel(const WgradArgs a) {
    constexpr int BKP = 16;
    constexpr int NTL = (NT + 1) / 2;          // tap loads per thread
    __shared__ __attribute__((aligned(16))) unsigned short Xs[2][NT][BKP][64];
    __shared__ __attribute__((aligned(16))) unsigned short Ds[2][BKP][64];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l31 = lane & 31, h = lane >> 5;
    const int mi = wave >> 1, ni = wave & 1;
    const Blk3 blk = xcd_block_order();
    const int ci0 = blk.x * 64, co0 = blk.y * 64;
    const int p_begin = blk.z * a.pix_per_split;
    const int p_end = min(a.M, p_begin + a.pix_per_split);
    const int nstages = (p_end - p_begin + BKP - 1) / BKP;

    const int half = __builtin_amdgcn_readfirstlane(tid >> 7);      // wave-uniform: waves 0,1 / 2,3
    const int k = (tid >> 3) & 15, c8 = tid & 7;                    // pixel slot, 8-channel (16-byte) lane
    const int c = ci0 + c8 * 8;
    const bool second = STRADDLE ? (c >= a.c1) : (ci0 >= a.c1);
    const bool xvalid = c < a.cin_ld;
    const int ld = second ? a.ldx2 : a.ldx;
    const int cc = second ? c - a.c1 : c;
    const __amdgpu_buffer_rsrc_t rs1 = __builtin_amdgcn_make_buffer_rsrc((void*)a.x, 0, a.xbytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t rs2 = __builtin_amdgcn_make_buffer_rsrc((void*)a.x2, 0, a.x2bytes, 0x00020000);
    constexpr int KS = NT == 9 ? 3 : 1;
    int tofb[NTL];
    unsigned tbit[NTL];
#pragma unroll
    for (int j = 0; j < NTL; ++j) {
        const int t = half + 2 * j;
        const bool tv = t < NT;
        const int tt = tv ? t : 0;
        tofb[j] = (a.dh[tt] * a.wi + a.dw[tt]) * ld * 2;
        tbit[j] = tv ? (1u << tt) : 0u;
    }
    int rdh[KS], cdw[KS];
#pragma unroll
    for (int i = 0; i < KS; ++i) {
        rdh[i] = a.dh[i * KS];
        cdw[i] = a.dw[i];
    }
    const __amdgpu_buffer_rsrc_t rsd = __builtin_amdgcn_make_buffer_rsrc((void*)a.dy, 0, a.dybytes, 0x00020000);
    const int co = co0 + c8 * 8;
    const bool dvalid = (co < a.cout) && half == 0;

    int p = p_begin + k;
    int ow, oh, n;
    {
        const int pp = p < a.M ? p : 0;
        ow = pp % a.wo;
        const int t2 = pp / a.wo;
        oh = t2 % a.ho;
        n = t2 / a.ho;
    }

    f32x16 acc[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;

    auto gload = [&](u32x4 (&rx)[NTL], u32x4& rd) {
        const bool ok = p < p_end;
        const int ihb = oh * a.is, iwb = ow * a.is;
        const unsigned base = (unsigned)(((n * a.hi + ihb) * a.wi + iwb) * ld + cc) * 2u;
        unsigned rm = 0, cm = 0;
#pragma unroll
        for (int i = 0; i < KS; ++i) {
            rm |= ((unsigned)(ihb + rdh[i]) < (unsigned)a.hi ? 1u : 0u) << i;
            cm |= ((unsigned)(iwb + cdw[i]) < (unsigned)a.wi ? 1u : 0u) << i;
        }
        unsigned m9 = 0;
#pragma unroll
        for (int i = 0; i < KS; ++i) m9 |= (rm & (1u << i)) ? (cm << (i * KS)) : 0u;
        if (!(ok && xvalid)) m9 = 0;
#pragma unroll
        for (int j = 0; j < NTL; ++j) {
            const unsigned off = (m9 & tbit[j]) ? base + (unsigned)tofb[j] : 0xffffffffu;
            if (STRADDLE) {
                u32x4 v1 = __builtin_amdgcn_raw_buffer_load_b128(rs1, (int)(second ? 0xffffffffu : off), 0, 0);
                u32x4 v2 = __builtin_amdgcn_raw_buffer_load_b128(rs2, (int)(second ? off : 0xffffffffu), 0, 0);
                rx[j] = v1 | v2;
            } else {
                rx[j] = second ? __builtin_amdgcn_raw_buffer_load_b128(rs2, (int)off, 0, 0)
                               : __builtin_amdgcn_raw_buffer_load_b128(rs1, (int)off, 0, 0);
            }
        }
        const unsigned offd = (ok && dvalid) ? (unsigned)(p * a.lddy + co) * 2u : 0xffffffffu;
        rd = __builtin_amdgcn_raw_buffer_load_b128(rsd, (int)offd, 0, 0);
        p += BKP;
        ow += BKP;
        if (ow >= a.wo) {
            do {
                ow -= a.wo;
                if (++oh == a.ho) {
                    oh = 0;
                    ++n;
                }
            } while (ow >= a.wo);
        }
    };
    const int scol = (c8 ^ (((k >> 1) & 1) << 2)) * 8;              // swizzled 16-byte chunk of this thread's row
    auto sstore = [&](int buf, const u32x4 (&rx)[NTL], const u32x4& rd) {
#pragma unroll
        for (int j = 0; j < NTL; ++j) {
            const int t = half + 2 * j;
            if (t < NT) *(u32x4*)(&Xs[buf][t][k][scol]) = rx[j];
        }
        if (half == 0) *(u32x4*)(&Ds[buf][k][scol]) = rd;
    };
    // transposed-read addressing: lane (group g = lane>>4, i = lane&15) supplies row 8h + (i>>2) (+4 for the
    // second read) and the 4 channels [32*tile + 16*(g&1) + 4*(i&3), +4)
    const int frow = 8 * h + ((lane & 15) >> 2);
    const int fsw = ((frow >> 1) & 1) << 5;
    const int fcol = 16 * ((lane >> 4) & 1) + 4 * (lane & 3);
    const int fa = frow * 64 + ((mi * 32 + fcol) ^ fsw);
    const int fb = frow * 64 + ((ni * 32 + fcol) ^ fsw);
    auto compute = [&](int buf) {
        const bf16x8 bv = tr_frag(&Ds[buf][0][0] + fb);
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            const bf16x8 av = tr_frag(&Xs[buf][t][0][0] + fa);
            acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(av, bv, acc[t], 0, 0, 0);
        }
    };

    if (nstages > 0) {
        u32x4 rx0[NTL], rx1[NTL], rd0, rd1;
        gload(rx0, rd0);
        if (nstages > 1) gload(rx1, rd1);
        sstore(0, rx0, rd0);
        __syncthreads();
        int s = 0;
        for (; s + 3 < nstages; s += 2) {
            gload(rx0, rd0);
            compute(0);
            sstore(1, rx1, rd1);
            __syncthreads();
            gload(rx1, rd1);
            compute(1);
            sstore(0, rx0, rd0);
            __syncthreads();
        }
        const int left = nstages - s;
        if (left >= 3) gload(rx0, rd0);
        compute(0);
        if (left >= 2) {
            sstore(1, rx1, rd1);
            __syncthreads();
            compute(1);
            if (left >= 3) {
                sstore(0, rx0, rd0);
                __syncthreads();
                compute(0);
            }
        }
    }

    wgrad_store_slab<NT, false>(acc, a.part + (size_t)blk.z * NT * a.cin * a.cout, a.cin, a.cout, ci0, mi, h, co0 + ni * 32 + l31, nullptr);
}

template <int NT, bool STRADDLE>
static void gen_launch(const WgradArgs& a, const WgradPlan& p, hipStream_t st) {
    const dim3 grid(shm_cdiv(a.cin, 64), shm_cdiv(a.cout, 64), p.splits);
    if (p.bf16)
        hipLaunchKernelGGL((wgrad_bf16_kernel<NT, STRADDLE>), grid, dim3(256), 0, st, a);
    else
        hipLaunchKernelGGL((wgrad_kernel<NT, STRADDLE>), grid, dim3(256), 0, st, a);
    shm_set_last_kernel(p.bf16 ? "wgrad_bf16_kernel<%d, %s>" : "wgrad_kernel<%d, %s>", NT, STRADDLE ? "true" : "false");
}

int shm_wgrad_gen_launch(const WgradArgs& a, const WgradPlan& p, hipStream_t st) {
    if (p.ntaps == 9) {
        if (p.straddle)
            gen_launch<9, true>(a, p, st);
        else
            gen_launch<9, false>(a, p, st);
    } else {
        if (p.straddle)
            gen_launch<1, true>(a, p, st);
        else
            gen_launch<1, false>(a, p, st);
    }
    return SHM_OK;
}
