// tapgemm_wreg_f32_kernel (SHM_TG_WREG, fp32 operands): the eight-wave weights-in-registers kernel on v_mfma_f32_16x16x4_f32.
#include "tapgemm_dev.h"

// ------------------------------------------------------------------------------------------
// The fp32 counterpart of tapgemm_wreg_kernel: 3x3 / stride-1 tap GEMM for K <= 64 input channels with the weights in
// registers, on v_mfma_f32_16x16x4_f32 (exact fp32, the same 64 FLOP/clk/SIMD as the 32x32x2 form).
//
// With 16-column MFMA tiles a wave's slice of the weight tensor is 9 taps x 64 channels x 16 columns = 144 VGPRs; one block
// per CU (8 waves: 2 (M) x 4 (N), wave tile 64 pixels x 16 channels, 8 x 16-pixel patches) keeps it for its whole range of
// patches.  A K step (one tap, 16 channels) is four 16-byte fragment reads and sixteen MFMAs per wave, there is no weight
// traffic and ONE barrier per patch (576 MFMAs = 18 432 MFMA cycles per wave): the per-K-step barrier / DMA-issue /
// first-ds_read bubble that holds the 128x64 DMA tile at 65-70 % of the fp32 peak on the Cout <= 64 layers does not exist.
// Outputs are stored straight from the accumulators (lane = channel: 64-byte segments, four pixel rows per instruction);
// InstanceNorm sums are carried in registers (f64) across the patches of an image.  LDS rows are 64 bytes (16 channels) with
// the DMA source-side swizzle chunk' = (chunk + (R >> 1)) & 3 on the halo row R: conflict free for this instruction's lane
// groups (pixel = lane & 15, chunk = lane >> 4) over all nine taps (tools/probes/halo_swizzle_check.py).
// GS: the gsum epilogue (input-gradient launches, see TapGemmArgs): S2 carries sum(v * aux) instead of sum(v * v).
// NM: "norm" (see tapgemm_halo_kernel) -- the source is the un-normalised activation of an InstanceNorm block; a wave normalises
// the halo items it DMA'd itself at the end of the patch in front (they have landed by then), from its own 1 KiB copy of the
// image's (mean, inv, beta) planes, which travels with the halo DMA.
// LDS pitch (halo rows per patch row, 18 of them used) and DMA items per 16-channel chunk of tapgemm_wreg_f32_kernel.  The 64-channel
// form (WN = 4, the hot one) pads its halo image to 24 rows per patch row: the chunk swizzle (lq + (R >> 1)) & 3 then repeats from one
// patch row to the next (12 = 0 mod 4), so the four M tiles of a tap read at ONE address register plus immediates -- 9 fragment address
// registers instead of 36, which is what lets the gsum form keep them across patches (recomputing them per patch, as it had to at
// pitch 18, was 4 % of the kernel) -- for 15 instead of 12 DMA items per chunk (the padding rows are out-of-range reads: zeros, no
// memory traffic).  The narrow forms keep pitch 18 (their 18- and 34-row halos would not fit at 24).
constexpr int wreg32_pitch(int wn) { return wn == 4 ? 24 : 18; }
constexpr int wreg32_nit(int wn) { return ((32 / wn + 2) * wreg32_pitch(wn) + 15) / 16; }
// T = bf16_t (round 3, "tapgemm.wreg16"): the same kernel on bf16 operands and outputs -- the LDS image, the DMA and every address are
// the fp32 kernel's (64-byte rows = 32 channels, a lane's 16-byte fragment = 8 channels = ONE v_mfma_f32_16x16x32_bf16 where fp32
// issues four 16x16x4), the weights of a 16-column wave tile are 9 x NCH x 4 registers -- 72 at 64 input channels, against 144 in the
// four-wave tapgemm_wreg_kernel -- so the kernel fits 128 VGPRs and a SIMD holds four waves of two blocks instead of two
// (profiles/r03_bf16_wreg_ablation.txt: at two waves per SIMD the MFMA phase and the epilogue / store / DMA-wait phase of that kernel add up
// instead of overlapping).  Plain forward form only (no gsum, no norm, one source).
template <int NCH, int WN = 4, bool TWO = false, bool GS = false, int NM = 0, typename T = float>
__global__ __launch_bounds__(512, sizeof(T) == 2 ? 4 : 2) void tapgemm_wreg_f32_kernel(const TapGemmArgs a, const int npatch) {
    static_assert(!NM || (!TWO && !GS), "norm: one source, forward form");
    static_assert(sizeof(T) == 4 || (WN == 4 && !TWO && !GS && !NM), "bf16: plain 64-channel form");
    constexpr int ESZ = sizeof(T), CHE = 16 / ESZ, BKE = 64 / ESZ;       // channels per 16-byte fragment / per 64-byte row
    // WN waves along N (16 columns each), WM = 8 / WN along M (four patch rows each): 64 / 32 / 16 output channels per block on
    // patches of 8 / 16 / 32 rows -- the narrow forms serve SpecSeg's 16- and 32-channel layers without idle N waves
    constexpr int WM = 8 / WN, PH = 4 * WM, HC = 18, HP = wreg32_pitch(WN), NIT = wreg32_nit(WN);     // halo (PH + 2) x 18 pixels at pitch HP, in DMA items of 16 rows
    constexpr int ASTG = NIT * 256;                     // floats per 16-channel chunk
    constexpr int ABUF = NCH * ASTG;                    // floats per halo buffer
    extern __shared__ __attribute__((aligned(1024))) float smem[];      // two halo buffers
    typedef __attribute__((address_space(3))) void* lds_ptr;

    const TapPhase& P = a.ph[0];
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l15 = lane & 15, lq = lane >> 4;
    const int wm = wave / WN, wn = wave % WN;
    const int n0 = blockIdx.y * (16 * WN);
    const int ppr = a.wi >> 4, ppi = (a.hi / PH) * ppr;

    const int per = (npatch + gridDim.x - 1) / gridDim.x;
    const int q0 = blockIdx.x * per, q1 = min(npatch, q0 + per);
    if (q0 >= q1) return;

    // ---- weights -> registers: lane (l15, lq) holds W[tap][n][c*16 + 4 lq .. +3] for its column n; MFMA e of a K step
    // contracts channel 4 k' + e of the chunk over k' = lane >> 4 (the same permutation on the A side)
    const int ncol = n0 + wn * 16 + l15;
    f32x4 bw[9][NCH];
    float bias;
    // (NM = 2, SHM_NORM_SCALED: the weight copy and the bias row of image `img`, re-read when the block's patch range moves on to the
    // next image -- outside the patch loop, so that hipcc's waitcnt pass drains these loads in the loop's preheader, not at every use)
    auto load_w = [&](int img) {
        const T* wp = (const T*)a.w + (NM == 2 ? (size_t)img * (a.wimg / ESZ) : (size_t)0);
#pragma unroll
        for (int t = 0; t < 9; ++t)
#pragma unroll
            for (int c = 0; c < NCH; ++c) bw[t][c] = *(const f32x4*)(wp + ((size_t)P.widx[t] * a.nout + ncol) * a.K + c * BKE + lq * CHE);
        bias = a.bias ? a.bias[(NM == 2 ? (size_t)img * a.bias_img : (size_t)0) + ncol] : 0.f;
    };
    load_w(NM == 2 ? q0 / ppi : 0);

    // ---- halo DMA: item (c, ri) = 16-channel chunk c, halo rows [16 ri, 16 ri + 16) of the LDS image; wave w owns row items w, w + 8, ...
    // of EVERY chunk, so a lane's pixel inside the halo depends on the row item only: per lane and row item one pixel offset and five
    // edge bits (top / bottom / left / right edge of the halo, "nothing to fetch"), per patch four scalar edge bits and the origin --
    // an add, a masked test, a multiply-add and one select per DMA instruction.  (Until round 3 every patch recomputed coordinates,
    // range tests and exec-masked selects per item, ~25 VALU instructions each, from the lane id -- the registers to keep them were
    // not there before the fragment addresses went from 36 to 9, see wreg32_pitch.)
    constexpr int NR = (NIT + 7) / 8;                    // row items per wave (the last one may be idle)
    static_assert(NR <= 6, "five edge bits per row item in one register");
    const int drow = lane >> 2, dq = lane & 3;
    const __amdgpu_buffer_rsrc_t rsx = __builtin_amdgcn_make_buffer_rsrc((void*)a.x, 0, a.xbytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t rsx2 = __builtin_amdgcn_make_buffer_rsrc((void*)a.x2, 0, a.x2bytes, 0x00020000);
    const unsigned pixb = (unsigned)a.ldx * (unsigned)ESZ, pixb2 = (unsigned)a.ldx2 * (unsigned)ESZ;
    const int nc1 = a.c1 / BKE;                           // TWO: chunks [0, nc1) come from x, the rest from x2 (Concatenate)
    float* const tbl = smem + 2 * ABUF + wave * 256;     // NM: this wave's copy of the planes of the image of the halo in flight
    [[maybe_unused]] const __amdgpu_buffer_rsrc_t rsn = __builtin_amdgcn_make_buffer_rsrc((void*)a.nt, 0, NM ? a.ntbytes : 0u, 0x00020000);
    // LDS chunk dq of row R holds channel chunk (dq - (R >> 1)) & 3; items start at multiples of 16 rows, so the term depends on the lane only
    const unsigned swb = (unsigned)(((dq - (drow >> 1)) & 3) << 4);
    unsigned po[NR], bm = 0;
#pragma unroll
    for (int jr = 0; jr < NR; ++jr) {
        const int ri = wave + 8 * jr;
        const int hrow = 16 * ri + drow;
        const int hr = hrow / HP, hc = hrow - hr * HP;
        po[jr] = (unsigned)(hr * a.wi + hc);
        const unsigned bits = (ri >= NIT || hr >= PH + 2 || hc >= HC) ? 16u : (hr == 0 ? 1u : 0u) | (hr == PH + 1 ? 2u : 0u) | (hc == 0 ? 4u : 0u) | (hc == HC - 1 ? 8u : 0u);
        bm |= bits << (5 * jr);
    }
    auto patch_edges = [&](int y0, int x0) {             // which edges of the image the halo of the patch at (y0, x0) sticks out of (+ bit 4)
        return 16u | (y0 == 0 ? 1u : 0u) | (y0 + PH == a.hi ? 2u : 0u) | (x0 == 0 ? 4u : 0u) | (x0 + 16 == a.wi ? 8u : 0u);
    };
    auto dma = [&](int q, int buf) {
        const int img = q / ppi, prem = q - img * ppi;
        const int y0 = (prem / ppr) * PH, x0 = (prem % ppr) << 4;
        float* dst = smem + buf * ABUF;
        // 4 x ntc <= 256 floats (checked by the launcher); the previous table was last read a patch ago.  NM = 2: only a patch on the
        // image border reads it (the `ring` plane)
        if constexpr (NM)
            if (NM == 1 || y0 == 0 || y0 + PH == a.hi || x0 == 0 || x0 + 16 == a.wi)
                __builtin_amdgcn_raw_ptr_buffer_load_lds(rsn, (lds_ptr)tbl, 16, (int)((unsigned)img * 16u * (unsigned)a.ntc + (unsigned)lane * 16u), 0, 0, 0);
        const unsigned edges = patch_edges(y0, x0);
        const unsigned basepix = (unsigned)((img * a.hi + y0 - 1) * a.wi + x0 - 1);          // pixel index of halo (0, 0); may wrap below zero
#pragma unroll
        for (int jr = 0; jr < NR; ++jr) {
            const int ri = wave + 8 * jr;                // wave-uniform
            if (jr < NR - 1 || ri < NIT) {
                const bool out = (bm & (edges << (5 * jr))) != 0;
                const unsigned pp = po[jr] + basepix;
                const unsigned o1 = pp * pixb + swb;
                [[maybe_unused]] const unsigned o2 = TWO ? pp * pixb2 + swb : 0u;
#pragma unroll
                for (int c = 0; c < NCH; ++c) {
                    if (!TWO || c < nc1) {
                        const unsigned off = out ? 0xffffffffu : o1 + (unsigned)(c * 64);
                        __builtin_amdgcn_raw_ptr_buffer_load_lds(rsx, (lds_ptr)(dst + (c * NIT + ri) * 256), 16, (int)off, 0, 0, 0);
                    } else {
                        const unsigned off = out ? 0xffffffffu : o2 + (unsigned)((c - nc1) * 64);
                        __builtin_amdgcn_raw_ptr_buffer_load_lds(rsx2, (lds_ptr)(dst + (c * NIT + ri) * 256), 16, (int)off, 0, 0, 0);
                    }
                }
            }
        }
    };

    // NM: normalise this wave's items of halo(q) in buffer buf (landed: the caller waited)
    [[maybe_unused]] auto norm_a = [&](int q, int buf) {
        const int img = q / ppi, prem = q - img * ppi;
        const int y0 = (prem / ppr) * PH, x0 = (prem % ppr) << 4;
        if (NM == 2 && !(y0 == 0 || y0 + PH == a.hi || x0 == 0 || x0 + 16 == a.wi)) return;       // block-uniform: no out-of-image halo entry
        const unsigned edges = patch_edges(y0, x0);
        float* dst = smem + buf * ABUF + lane * 4;
#pragma unroll
        for (int jr = 0; jr < NR; ++jr) {
            const int ri = wave + 8 * jr;
            if (jr < NR - 1 || ri < NIT) {
                const unsigned m = (bm >> (5 * jr)) & 31u;
                const bool halo = (m & 16u) == 0;                  // (not a padding row of the LDS image)
                const bool inside = (m & edges & 15u) == 0;
#pragma unroll
                for (int c = 0; c < NCH; ++c) {
                    float* p = dst + (c * NIT + ri) * 256;
                    if constexpr (NM == 2) {        // SHM_NORM_SCALED: `ring` over the out-of-image entries (see tapgemm_halo_kernel)
                        if (halo && !inside) *(f32x4*)p = *(const f32x4*)(tbl + 3 * a.ntc + c * 16 + (swb >> 2));
                    } else if (halo && inside) {
                        const float* tb = tbl + c * 16 + (swb >> 2);
                        f32x4 x = *(const f32x4*)p;
                        const f32x4 mean = *(const f32x4*)tb, inv = *(const f32x4*)(tb + a.ntc), beta = *(const f32x4*)(tb + 2 * a.ntc);
#pragma unroll
                        for (int e = 0; e < 4; ++e) x[e] = shm_in_norm(x[e], mean[e], inv[e], beta[e]);
                        *(f32x4*)p = x;
                    }
                }
            }
        }
    };

    // ---- fragment addressing: M tile m = patch row 4 wm + m, pixel = l15; halo row of the centre tap
    const int hb0 = (4 * wm + 1) * HP + l15 + 1;
    int tsh[9];
#pragma unroll
    for (int t = 0; t < 9; ++t) tsh[t] = P.dh[t] * HP + P.dw[t];

    double S1 = 0.0, S2 = 0.0;
    int simg = q0 / ppi;
    // gsum: the wave's 16 columns lie in one part (n1 % 16 == 0): gp, the pitch and the "this part takes sums" test are scalars
    const int gp = __builtin_amdgcn_readfirstlane(n0 + wn * 16) < a.n1 ? 0 : 1;
    const int gpc = gp ? a.nout - a.n1 : a.n1, gnl = ncol - (gp ? a.n1 : 0);
    const bool gson = GS && a.gred[gp] != nullptr;
    // (aux has the extent of its output part, which the launcher checked to be below 4 GiB: 32-bit offsets, scalar descriptor)
    const __amdgpu_buffer_rsrc_t rsa = __builtin_amdgcn_make_buffer_rsrc((void*)a.gaux[gp], 0, gson ? 0xfffffff0u : 0u, 0x00020000);
    const unsigned ldab = (unsigned)a.ldgaux[gp] * 4u;
    const float* const gaux = gson ? (const float*)a.gaux[gp] : nullptr;
    auto flush = [&](int img) {
        double t1 = S1 + __shfl_xor(S1, 16, 64), t2 = S2 + __shfl_xor(S2, 16, 64);
        t1 += __shfl_xor(t1, 32, 64);
        t2 += __shfl_xor(t2, 32, 64);
        if (lane < 16) {
            if constexpr (GS) {
                if (gaux) {
                    double* dst = a.gred[gp] + ((size_t)((WM * blockIdx.x + wm) % a.gslots) * a.gbatch * gpc + (size_t)img * gpc + gnl) * 2;
                    atomicAdd(dst, t1);
                    atomicAdd(dst + 1, t2);
                }
            } else {
                double* dst = a.stats + (size_t)((WM * blockIdx.x + wm) % a.stats_slots) * a.stats_stride + ((size_t)img * a.nout + ncol) * 2;
                atomicAdd(dst, t1);
                atomicAdd(dst + 1, t2);
            }
        }
        S1 = S2 = 0.0;
    };
    const __amdgpu_buffer_rsrc_t rsy = __builtin_amdgcn_make_buffer_rsrc(a.y, 0, a.ybytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t rsy2 = __builtin_amdgcn_make_buffer_rsrc(a.y2, 0, a.y2bytes, 0x00020000);
    const bool part0 = __builtin_amdgcn_readfirstlane(n0 + wn * 16) < a.n1;

    dma(q0, 0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    if constexpr (NM) norm_a(q0, 0);
    auto patch = [&](const int q) {
        const int buf = (q - q0) & 1;
        SHM_LDS_BARRIER();                   // halo(q) landed for every wave; everyone is done with the other buffer
        asm volatile("" ::: "memory");
        if (q + 1 < q1) dma(q + 1, buf ^ 1);
        // gsum: aux at the sixteen output positions of this lane (the same 64-byte segments as the epilogue's stores), issued here so
        // that their latency passes under the 576 MFMAs of the patch.  A part without sums has a zero-length descriptor: zeros.
        float gq[4][4];
        if constexpr (GS) {
            const int img = q / ppi, prem = q - img * ppi;
            const int y0 = (prem / ppr) * PH, x0 = (prem % ppr) << 4;
            // one address register (the lane's pixel of tile 0, register 0); tile m / register r is a scalar offset
            const unsigned ao = (unsigned)((img * a.hi + (y0 + 4 * wm)) * a.wi + (x0 + 4 * lq)) * ldab + (unsigned)gnl * 4u;
#pragma unroll
            for (int m = 0; m < 4; ++m)
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    gq[m][r] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rsa, ao, (unsigned)(m * a.wi + r) * ldab, 0));
        }

        f32x4 acc[4];
#pragma unroll
        for (int m = 0; m < 4; ++m)
#pragma unroll
            for (int r = 0; r < 4; ++r) acc[m][r] = bias;
        const float* Ab = smem + buf * ABUF;
        // gsum form: the 36 fragment addresses are formed per patch -- hoisted out of the patch loop (as hipcc does) they no longer fit
        // beside the sixteen aux values, and the spills landed in the DMA issue path (a scratch reload + vmcnt(0) in front of every
        // halo DMA: the DMAs of a patch ran one after the other, 84 instead of 131 TFLOP/s)
        int hbq = hb0;
        if constexpr (GS && HP % 8 != 0) asm volatile("" : "+v"(hbq));
#pragma unroll
        for (int t = 0; t < 9; ++t) {
            // rows of the four M tiles are HP halo rows apart.  Pitch 18: the swizzle term (R >> 1) grows by 9 per tile, per-tile addresses;
            // pitch 24: by 12, the same chunk -- one address per tap, the tiles are immediates
            int fa[4];
#pragma unroll
            for (int m = 0; m < 4; ++m) {
                const int hrow = hbq + (HP % 8 == 0 ? 0 : m * HP) + tsh[t];
                fa[m] = hrow * 16 + (((lq + (hrow >> 1)) & 3) << 2) + (HP % 8 == 0 ? m * HP * 16 : 0);
            }
#pragma unroll
            for (int c = 0; c < NCH; ++c) {
                if constexpr (ESZ == 4) {
                    f32x4 av[4];
#pragma unroll
                    for (int m = 0; m < 4; ++m) av[m] = *(const f32x4*)(Ab + c * ASTG + fa[m]);
#pragma unroll
                    for (int e = 0; e < 4; ++e)
#pragma unroll
                        for (int m = 0; m < 4; ++m) acc[m] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[m][e], bw[t][c][e], acc[m], 0, 0, 0);
                } else {
                    // two fragments at a time (128 VGPRs: 72 of weights, 16 accumulators)
#pragma unroll
                    for (int mh = 0; mh < 4; mh += 2) {
                        const f32x4 a0 = *(const f32x4*)(Ab + c * ASTG + fa[mh]), a1 = *(const f32x4*)(Ab + c * ASTG + fa[mh + 1]);
                        acc[mh] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a0), __builtin_bit_cast(bf16x8, bw[t][c]), acc[mh], 0, 0, 0);
                        acc[mh + 1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a1), __builtin_bit_cast(bf16x8, bw[t][c]), acc[mh + 1], 0, 0, 0);
                        asm volatile("" ::: "memory");
                    }
                }
            }
        }

        // ---- epilogue of patch q: accumulator register r of tile m = pixel (row 4 wm + m, column 4 lq + r), channel ncol
        const int img = q / ppi, prem = q - img * ppi;
        const int y0 = (prem / ppr) * PH, x0 = (prem % ppr) << 4;
        if ((GS || a.stats) && img != simg) {
            flush(simg);
            simg = img;
        }
        float s1 = 0.f, s2 = 0.f;
        // the wave's 16 channels lie in one output part (n1 % 16 == 0): descriptor, pitch and channel offset are scalar selects (a per-lane
        // choice of the descriptor makes hipcc wrap every store in a readfirstlane loop); one address register -- the lane's pixel of
        // tile 0, register 0 -- and a scalar offset per (tile, register)
        const unsigned ldyb = (unsigned)(part0 ? a.ldy : a.ldy2) * (unsigned)ESZ;
        const unsigned yo = (unsigned)((img * a.hi + (y0 + 4 * wm)) * a.wi + (x0 + 4 * lq)) * ldyb + (unsigned)(part0 ? ncol : ncol - a.n1) * (unsigned)ESZ;
#pragma unroll
        for (int m = 0; m < 4; ++m)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float u = acc[m][r];
                const T vo = (T)shm_lrelu_max(u, a.slope);           // LeakyReLU for 0 <= slope <= 1 (checked by the launcher)
                const float v = (float)vo;                           // statistics of the value as stored
                s1 += v;
                if constexpr (GS) s2 += v * gq[m][r];
                else s2 = __builtin_fmaf(v, v, s2);
                if constexpr (abl::nostore)
                    asm volatile("" ::"v"(v));                           // timing only
                else if constexpr (ESZ == 4)
                    __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, vo), part0 ? rsy : rsy2, yo, (unsigned)(m * a.wi + r) * ldyb, 0);
                else
                    __builtin_amdgcn_raw_buffer_store_b16(__builtin_bit_cast(unsigned short, vo), part0 ? rsy : rsy2, yo, (unsigned)(m * a.wi + r) * ldyb, 0);
            }
        S1 += (double)s1;
        S2 += (double)s2;
        // halo(q + 1) was issued at the top of this patch; younger: this epilogue's sixteen stores (plus the rare flush; the gsum
        // form's aux loads were issued right behind the halo and have been consumed: loads return in order)
        if constexpr (abl::nostore)
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");           // timing only: no stores behind the halo DMA
        else
            asm volatile("s_waitcnt vmcnt(16)" ::: "memory");
        if constexpr (NM)
            if (q + 1 < q1) norm_a(q + 1, buf ^ 1);
    };
    if constexpr (NM == 2) {                 // one weight copy per image -> one segment of the patch range per image
        int q = q0;
        while (q < q1) {
            const int qe = min(q1, (q / ppi + 1) * ppi);
            if (q != q0) load_w(q / ppi);
            for (; q < qe; ++q) patch(q);
        }
    } else {
        for (int q = q0; q < q1; ++q) patch(q);
    }
    if (GS || a.stats) flush(simg);
}

// One form: its LDS reservation (once per process), its instantiation and the name the profiler gives it (which ends at the last argument
// that is not a default).  lds = two halo buffers (+ norm: 1 KiB of planes per wave), what the caller sized the launch with.
template <int NCH, int WN, bool TWO = false, bool GS = false, int NM = 0>
static hipError_t wreg32_launch(const TapGemmArgs& a, dim3 grid, unsigned lds, int npw, hipStream_t st) {
    static const hipError_t attr = hipFuncSetAttribute((const void*)tapgemm_wreg_f32_kernel<NCH, WN, TWO, GS, NM>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                                       2 * NCH * wreg32_nit(WN) * 1024 + (NM ? 8 * 1024 : 0));
    if (attr != hipSuccess) return attr;
    hipLaunchKernelGGL((tapgemm_wreg_f32_kernel<NCH, WN, TWO, GS, NM>), grid, dim3(512), lds, st, a, npw);
    shm_set_last_kernel("tapgemm_wreg_f32_kernel<%d, %d, %s%s>", NCH, WN, TWO ? "true" : "false", NM == 2 ? ", false, 2" : NM == 1 ? ", false, 1" : GS ? ", true" : "");
    return hipSuccess;
}

int shm_wreg_f32_launch(const TapGemmArgs& a, const TapGemmPlan& p, int batch, int ncu, hipStream_t st, const char* who) {
    const bool want_nm = a.nt != nullptr, gs_fused = p.gs_fused;
    const int wn = p.wreg32_wn;
    // one 8-wave block per CU; patches of 8 (64 channels per block), 16 (32) or 32 (16) rows
    const int ph = 32 / wn, npw = batch * (a.hi / ph) * (a.wi / 16), nyw = a.nout / (16 * wn);
    const int nch = a.K / 16;
    // one 8-wave block per CU; the plain 16-input-channel, 64-column form (100 VGPRs, 30 KiB of LDS) fits two: 399 -> 382 us on the
    // generator's first layer (16 -> 64 @256^2, n = 40)
    const int per_cu = (nch == 1 && wn == 4 && !want_nm && !gs_fused) ? 2 : 1;
    int gx = per_cu * ncu / nyw;
    if (gx < 1) gx = 1;
    if (gx > npw) gx = npw;
    const dim3 grid(gx, nyw, 1);
    const unsigned lds = 2u * (unsigned)nch * (unsigned)wreg32_nit(wn) * 1024u + (want_nm ? 8u * 1024u : 0u);      // two halo buffers (+ norm: 1 KiB of planes per wave)
    hipError_t attr;
    if (want_nm && nch == 4 && a.ntmode) attr = wreg32_launch<4, 4, false, false, 2>(a, grid, lds, npw, st);
    else if (want_nm && nch == 4) attr = wreg32_launch<4, 4, false, false, 1>(a, grid, lds, npw, st);
    else if (want_nm && nch == 2 && a.ntmode) attr = wreg32_launch<2, 4, false, false, 2>(a, grid, lds, npw, st);
    else if (want_nm && nch == 2) attr = wreg32_launch<2, 4, false, false, 1>(a, grid, lds, npw, st);
    else if (want_nm && a.ntmode) attr = wreg32_launch<1, 4, false, false, 2>(a, grid, lds, npw, st);
    else if (want_nm) attr = wreg32_launch<1, 4, false, false, 1>(a, grid, lds, npw, st);
    else if (gs_fused && nch == 4) attr = wreg32_launch<4, 4, false, true>(a, grid, lds, npw, st);
    else if (gs_fused && nch == 2) attr = wreg32_launch<2, 4, false, true>(a, grid, lds, npw, st);
    else if (gs_fused) attr = wreg32_launch<1, 4, false, true>(a, grid, lds, npw, st);
    else if (wn == 4 && nch == 4) attr = wreg32_launch<4, 4>(a, grid, lds, npw, st);
    else if (wn == 4 && nch == 2) attr = wreg32_launch<2, 4>(a, grid, lds, npw, st);
    else if (wn == 4) attr = wreg32_launch<1, 4>(a, grid, lds, npw, st);
    else if (wn == 2 && nch == 2) attr = wreg32_launch<2, 2>(a, grid, lds, npw, st);
    else if (wn == 2) attr = wreg32_launch<1, 2>(a, grid, lds, npw, st);
    else if (nch == 2 && a.x2) attr = wreg32_launch<2, 1, true>(a, grid, lds, npw, st);
    else if (nch == 2) attr = wreg32_launch<2, 1>(a, grid, lds, npw, st);
    else attr = wreg32_launch<1, 1>(a, grid, lds, npw, st);
    SHM_REQUIRE(attr == hipSuccess, SHM_E_HIP, "%s: cannot reserve %u bytes of LDS: %s", who, lds, hipGetErrorString(attr));
    return SHM_OK;
}
