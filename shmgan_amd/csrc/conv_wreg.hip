// tapgemm_wreg_kernel (SHM_TG_WREG, bf16 operands): the four-wave weights-in-registers kernel.  Plain bf16 -> bf16 launches take the eight-wave
// kernels of conv_wreg16.hip / conv_pingpong.hip where the plan says so; this one keeps the fp32-output, gsum and norm forms.
#include "tapgemm_dev.h"

// ------------------------------------------------------------------------------------------
// bf16 3x3 / stride-1 tap GEMM for K <= 64 input channels with the WEIGHTS IN REGISTERS (persistent blocks).
//
// The 64-channel 256 x 256 layers are the HBM-side layers of the bf16 step (3 FLOP per byte and tap): in
// tapgemm_halo_kernel a block lives for 18 K-steps between a 2-3 us halo prologue and its store epilogue, with a
// barrier and a weight DMA per tap.  Here the whole weight tensor of a 32-column slice -- 9 taps x K <= 64
// channels = 144 VGPRs per lane -- is loaded ONCE per block and kept in registers; a block (4 waves: 2 (M) x 2 (N),
// wave tile 64 pixels x 32 channels) then walks a contiguous range of 8 x 16-pixel patches:
//   * the 10 x 18 halo of patch p+1 is DMA'd into the other LDS buffer right after the barrier that opens patch p,
//     i.e. it lands under the 72 MFMAs and the epilogue of patch p;
//   * ONE barrier per patch (halo landed for all waves = everybody is done reading the other buffer), no weight
//     traffic, no per-tap synchronisation: the nine taps are nine shifted fragment addresses into the halo;
//   * epilogue as in the halo kernel (LeakyReLU, bf16 rounding, LDS-staged 16-byte stores; the bias is the accumulators'
//     initial value); the InstanceNorm
//     sums are kept in registers (f64) across the patches of one image and flushed with one atomic per column when the
//     image changes: ~40x fewer atomics.
// Two blocks per CU (64 KB of LDS, 256 VGPRs each): they run out of step, so one block's epilogue (VALU, stores)
// overlaps the other's MFMAs on the same SIMDs.  (An explicit ping-pong -- one 8-wave block whose two halves swap MFMA and
// epilogue roles at every barrier -- was built and measured 30 % SLOWER: a wave's MFMA chain waits on its own ds_reads, and
// with the partner pinned to the epilogue nobody fills those bubbles.)  LDS rows are 64 bytes as in the other kernels (DMA
// source-side swizzle, 0xffffffff offsets -> zeros for halo pixels outside the image); the chunk swizzle is
// ((R >> 1) + R / 18) & 3 on the halo row R, which makes every 16-lane group of the fragment reads hit 16 distinct 16-byte
// bank units for all nine taps (brute-force check: tools/probes/halo_swizzle_check.py).  Its address arithmetic is patch independent
// here, so unlike in tapgemm_halo_kernel it costs nothing per tap.
// GS: the gsum epilogue (input-gradient launches, see TapGemmArgs) for bf16 outputs.
// NM: "norm" (see tapgemm_halo_kernel / tapgemm_wreg_f32_kernel).
template <typename TO, int NCH, bool GS = false, int NM = 0>
__global__ __launch_bounds__(256, 2) void tapgemm_wreg_kernel(const TapGemmArgs a, const int npatch) {
    typedef bf16_t T;
    static_assert(!GS || sizeof(TO) == 2, "the gsum epilogue of this kernel is the LDS-staged bf16 one");
    static_assert(!NM || !GS, "norm: forward form");
    constexpr int PH = 8, HC = 18, NIT = 12;            // halo (PH + 2) x 18 = 180 rows, padded to 12 DMA items of 16 rows
    constexpr int ASTG = NIT * 256;                     // floats per 32-channel chunk
    constexpr int ABUF = NCH * ASTG;                    // floats per halo buffer
    static_assert(NIT * NCH % 4 == 0, "DMA items divide over the four waves");
    __shared__ __attribute__((aligned(1024))) float smem[2 * ABUF + 4 * 1024 + (NM ? 4 * 256 : 0)];       // + 4 KB store staging per wave (+ NM: 1 KB table)
    typedef __attribute__((address_space(3))) void* lds_ptr;

    const TapPhase& P = a.ph[0];
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l31 = lane & 31, h = lane >> 5;
    const int wm = wave >> 1, wn = wave & 1;
    const int n0 = blockIdx.y * 64;
    const int ppr = a.wi >> 4, ppi = (a.hi / PH) * ppr;

    // contiguous patch range of this block
    const int per = (npatch + gridDim.x - 1) / gridDim.x;
    const int q0 = blockIdx.x * per, q1 = min(npatch, q0 + per);
    if (q0 >= q1) return;

    // ---- weights -> registers: lane (l31, h) holds W[tap][n][c*32 + kk*16 + 8h .. +7] for its column n
    const int ncol = n0 + wn * 32 + l31;
    bf16x8 bw[9][NCH][2];
    float bias;
    // (NM, SHM_NORM_SCALED: the weight copy and the bias row of image `img`, see tapgemm_wreg_f32_kernel)
    auto load_w = [&](int img) {
        const bf16_t* wp = (const bf16_t*)a.w + (NM == 2 ? (size_t)img * (a.wimg >> 1) : (size_t)0);
#pragma unroll
        for (int t = 0; t < 9; ++t)
#pragma unroll
            for (int c = 0; c < NCH; ++c)
#pragma unroll
                for (int kk = 0; kk < 2; ++kk) {
                    bf16x8 v = {};
                    if (ncol < a.nout) v = *(const bf16x8*)(wp + ((size_t)P.widx[t] * a.nout + ncol) * a.K + c * 32 + kk * 16 + h * 8);
                    bw[t][c][kk] = v;
                }
        bias = (a.bias && ncol < a.nout) ? a.bias[(NM == 2 ? (size_t)img * a.bias_img : (size_t)0) + ncol] : 0.f;
    };
    load_w(NM == 2 ? q0 / ppi : 0);

    // ---- halo DMA: item it (0 .. NIT*NCH-1) = chunk it / NIT, halo rows [16 (it % NIT), +16); wave w owns items w, w+4, ...
    // NIT / 4 = 3 items per wave and chunk: item j of chunk c covers halo rows 16 (wave + 4 j) + drow, so the lane keeps
    // three halo row numbers and derives the rest per patch (registers are what this kernel is short of).
    const int drow = lane >> 2, dq = lane & 3;
    static_assert(NIT == 12, "three DMA items per wave and chunk");
    const __amdgpu_buffer_rsrc_t rsx = __builtin_amdgcn_make_buffer_rsrc((void*)a.x, 0, a.xbytes, 0x00020000);
    const unsigned pixb = (unsigned)a.ldx * 2u;
    float* const tbl = smem + 2 * ABUF + 4 * 1024 + wave * 256;     // NM: this wave's copy of the planes of the image of the halo in flight
    [[maybe_unused]] const __amdgpu_buffer_rsrc_t rsn = __builtin_amdgcn_make_buffer_rsrc((void*)a.nt, 0, NM ? a.ntbytes : 0u, 0x00020000);
    // (the instantiations that are out of registers -- gsum, SHM_NORM_SCALED with two chunks: neither runs in the default bf16 step --
    // keep recomputing the halo coordinates per patch from the lane id: four more live registers would be four more spills)
    constexpr bool kDmaConst = !(NCH == 2 && (GS || NM == 2));
    [[maybe_unused]] unsigned doff[3], dbm = 0;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const int hrow = 16 * (wave + 4 * j) + drow;
        const int hr = hrow / HC, hc = hrow - hr * HC;
        doff[j] = (unsigned)(hr * a.wi + hc) * pixb + (unsigned)((dq ^ (((hrow >> 1) + hr) & 3)) << 4);
        dbm |= (hrow >= (PH + 2) * HC ? 16u : (hr == 0 ? 1u : 0u) | (hr == PH + 1 ? 2u : 0u) | (hc == 0 ? 4u : 0u) | (hc == HC - 1 ? 8u : 0u)) << (5 * j);
    }
    auto dma = [&](int q, int buf) {
        const int img = q / ppi, prem = q - img * ppi;
        const int y0 = (prem / ppr) * PH, x0 = (prem % ppr) << 4;
        float* dst = smem + buf * ABUF + wave * 256;
        // 4 x ntc <= 256 floats (checked by the launcher); the previous table was last read a patch ago.  NM = 2: only a patch on the
        // image border reads it (the `ring` plane)
        if constexpr (NM)
            if (NM == 1 || y0 == 0 || y0 + PH == a.hi || x0 == 0 || x0 + 16 == a.wi)
                __builtin_amdgcn_raw_ptr_buffer_load_lds(rsn, (lds_ptr)tbl, 16, (int)((unsigned)img * 16u * (unsigned)a.ntc + (unsigned)lane * 16u), 0, 0, 0);
        if constexpr (!kDmaConst) {
            int dr = drow;
            asm volatile("" : "+v"(dr));        // recompute the halo coordinates per patch: hoisted, they are spilled
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                const int hrow = 16 * (wave + 4 * j) + dr;
                const int hr = hrow / HC, hc = hrow - hr * HC;
                const int iy = y0 - 1 + hr, ix = x0 - 1 + hc;
                const bool v = hrow < (PH + 2) * HC && (unsigned)iy < (unsigned)a.hi && (unsigned)ix < (unsigned)a.wi;
                const unsigned off = v ? (unsigned)((img * a.hi + iy) * a.wi + ix) * pixb + (unsigned)((dq ^ (((hrow >> 1) + hr) & 3)) << 4) : 0xffffffffu;
#pragma unroll
                for (int c = 0; c < NCH; ++c)
                    __builtin_amdgcn_raw_ptr_buffer_load_lds(rsx, (lds_ptr)(dst + c * ASTG + j * 4 * 256), 16,
                                                             (int)(v ? off + 64u * c : 0xffffffffu), 0, 0, 0);
            }
            return;
        }
        // per-lane constants (byte offset of the lane's pixel inside the halo incl. the source-side swizzle, five edge bits per item)
        // + the patch's origin and edge bits: see tapgemm_wreg_f32_kernel
        const unsigned edges = 16u | (y0 == 0 ? 1u : 0u) | (y0 + PH == a.hi ? 2u : 0u) | (x0 == 0 ? 4u : 0u) | (x0 + 16 == a.wi ? 8u : 0u);
        const unsigned baseb = (unsigned)((img * a.hi + y0 - 1) * a.wi + x0 - 1) * pixb;           // halo (0, 0); may wrap below zero
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const bool out = (dbm & (edges << (5 * j))) != 0;
            const unsigned off = doff[j] + baseb;
#pragma unroll
            for (int c = 0; c < NCH; ++c)
                __builtin_amdgcn_raw_ptr_buffer_load_lds(rsx, (lds_ptr)(dst + c * ASTG + j * 4 * 256), 16,
                                                         (int)(out ? 0xffffffffu : off + 64u * c), 0, 0, 0);
        }
    };

    // NM: normalise this wave's items of halo(q) in buffer buf (landed: the caller waited)
    [[maybe_unused]] auto norm_a = [&](int q, int buf) {
        const int img = q / ppi, prem = q - img * ppi;
        const int y0 = (prem / ppr) * PH, x0 = (prem % ppr) << 4;
        if (NM == 2 && !(y0 == 0 || y0 + PH == a.hi || x0 == 0 || x0 + 16 == a.wi)) return;       // block-uniform: no out-of-image halo entry
        float* dst = smem + buf * ABUF + wave * 256 + lane * 4;
        int dr = drow;
        asm volatile("" : "+v"(dr));        // as in dma(): nothing of this is kept across the MFMA loop
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const int hrow = 16 * (wave + 4 * j) + dr;
            const int hr = hrow / HC, hc = hrow - hr * HC;
            const int iy = y0 - 1 + hr, ix = x0 - 1 + hc;
            const bool inside = (unsigned)iy < (unsigned)a.hi && (unsigned)ix < (unsigned)a.wi;
            if constexpr (NM == 2) {                // SHM_NORM_SCALED: `ring` over the out-of-image entries (see tapgemm_halo_kernel)
                if (hrow < (PH + 2) * HC && !inside) {
                    const int g8 = (dq ^ (((hrow >> 1) + hr) & 3)) << 3;
#pragma unroll
                    for (int c = 0; c < NCH; ++c) {
                        const float* tb = tbl + 3 * a.ntc + c * 32 + g8;
                        const f32x4 r0 = *(const f32x4*)tb, r1 = *(const f32x4*)(tb + 4);
                        u32x4 x;
#pragma unroll
                        for (int e = 0; e < 2; ++e) {
                            x[e] = (unsigned)__builtin_bit_cast(unsigned short, (bf16_t)r0[2 * e]) |
                                   ((unsigned)__builtin_bit_cast(unsigned short, (bf16_t)r0[2 * e + 1]) << 16);
                            x[2 + e] = (unsigned)__builtin_bit_cast(unsigned short, (bf16_t)r1[2 * e]) |
                                       ((unsigned)__builtin_bit_cast(unsigned short, (bf16_t)r1[2 * e + 1]) << 16);
                        }
                        *(u32x4*)(dst + c * ASTG + j * 4 * 256) = x;
                    }
                }
            } else if (hrow < (PH + 2) * HC && inside) {
                const int g8 = (dq ^ (((hrow >> 1) + hr) & 3)) << 3;
#pragma unroll
                for (int c = 0; c < NCH; ++c) {
                    const float* tb = tbl + c * 32 + g8;
                    float* p = dst + c * ASTG + j * 4 * 256;
                    u32x4 x = *(const u32x4*)p;
#pragma unroll
                    for (int hf = 0; hf < 2; ++hf) {
                        const f32x4 mean = *(const f32x4*)(tb + 4 * hf), inv = *(const f32x4*)(tb + a.ntc + 4 * hf),
                                    beta = *(const f32x4*)(tb + 2 * a.ntc + 4 * hf);
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
    };

    // ---- fragment addressing (patch independent): byte address of the centre tap's halo row for the two 32-pixel tiles
    const int hb0 = (4 * wm + (l31 >> 4) + 1) * HC + (l31 & 15) + 1;      // second tile: + 2 * HC
    int tsh[9];
#pragma unroll
    for (int t = 0; t < 9; ++t) tsh[t] = P.dh[t] * HC + P.dw[t];

    // statistics carried over the patches of one image (fp32 per lane: at most a few thousand bf16-rounded terms; the
    // cross-block sums are f64 atomics)
    float S1 = 0.f, S2 = 0.f;
    int simg = q0 / ppi;
    auto flush = [&](int img) {
        const float t1 = S1 + __shfl_xor(S1, 32, 64), t2 = S2 + __shfl_xor(S2, 32, 64);
        if (h == 0 && ncol < a.nout) {
            double* dst = a.stats + (size_t)(blockIdx.x % a.stats_slots) * a.stats_stride + ((size_t)img * a.nout + ncol) * 2;
            atomicAdd(dst, (double)t1);
            atomicAdd(dst + 1, (double)t2);
        }
        S1 = S2 = 0.f;
    };

    unsigned short* const tile = (unsigned short*)(smem + 2 * ABUF) + wave * 2048;      // 64 rows x 32 bf16
    // bf16 outputs leave through LDS-staged 16-byte stores: the launcher guarantees Cout % 64 == 0 (every wave owns 32 valid
    // columns: no conditionals in the epilogue, which cost this kernel VGPRs it does not have), 16-byte aligned pitches and
    // bases.  fp32 outputs (SHM_BF16_GF32) use element stores.
    constexpr bool kWide = sizeof(TO) == 2;
    // outputs through buffer stores: one 32-bit offset register per store instead of a 64-bit address
    const __amdgpu_buffer_rsrc_t rsy = __builtin_amdgcn_make_buffer_rsrc(a.y, 0, a.ybytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t rsy2 = __builtin_amdgcn_make_buffer_rsrc(a.y2, 0, a.y2bytes, 0x00020000);

    dma(q0, 0);
    // (Starting the block in the odd HW wave slot of its SIMDs half a patch late, to put the two blocks of a CU in anti-phase,
    // was measured with delays of 1300-5800 clocks: no effect.)
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    if constexpr (NM) norm_a(q0, 0);
    auto patch = [&](const int q) {
        const int buf = (q - q0) & 1;
        SHM_LDS_BARRIER();                   // halo(q) landed for every wave (each waited for its own part at the end
        asm volatile("" ::: "memory");                  // of the previous patch); everyone is done with the other buffer
        if constexpr (!abl::nodma)
            if (q + 1 < q1) dma(q + 1, buf ^ 1);

        f32x16 acc[2];
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][r] = bias;
        const float* Ab = smem + buf * ABUF;
        // gsum form: the nine fragment addresses are formed per patch -- kept across patches (hipcc hoists them) they no longer fit
        // beside the epilogue's sums and were spilled INSIDE the MFMA loop (27 scratch reloads per patch)
        int hbq = hb0;
        if constexpr (GS) asm volatile("" : "+v"(hbq));
        if constexpr (abl::wreg_prio) __builtin_amdgcn_s_setprio(1);
        // (An explicit software pipeline -- fragment reads pinned two or three steps ahead of their MFMAs with sched_barrier --
        // was measured: no gain on the forward, 15 % slower input gradients.  With two waves per SIMD the partner's MFMAs cover
        // a wave's LDS latency; hipcc's just-in-time reads keep the VGPR count at the 256 limit.)
#pragma unroll
        for (int t = 0; t < 9; ++t) {
            // the swizzle is invariant under a shift by two halo lines (36 rows: (R >> 1) + R / 18 grows by 20), so the second
            // 32-pixel tile reads at a constant offset from the first: one address register per (tap, kk), the tile and the
            // channel chunk go into the instruction's offset field
            int fa[2];
            {
                const int hrow = hbq + tsh[t];
                fa[0] = hrow * 16 + ((h ^ (((hrow >> 1) + hrow / HC) & 3)) << 2);      // floats; the kk = 1 group is this address ^ 8
                fa[1] = fa[0] + 2 * HC * 16;
            }
#pragma unroll
            for (int c = 0; c < NCH; ++c)
#pragma unroll
                for (int kk = 0; kk < 2; ++kk)
#pragma unroll
                    for (int i = 0; i < 2; ++i) {
                        f32x4 av;
                        if constexpr (abl::nolds) {
                            av = __builtin_bit_cast(f32x4, bw[t][c][kk]);         // timing only: no fragment reads
                            asm volatile("" : "+v"(av));
                        } else {
                            av = *(const f32x4*)(Ab + c * ASTG + (fa[i] ^ (kk << 3)));
                        }
                        if constexpr (abl::nomfma)
                            asm volatile("" ::"v"(av), "v"(bw[t][c][kk]));          // timing only: fragment reads without the MFMAs
                        else
                            acc[i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, av), bw[t][c][kk], acc[i], 0, 0, 0);
                    }
        }

        if constexpr (abl::wreg_prio) __builtin_amdgcn_s_setprio(0);
        // ---- epilogue of patch q
        const int img = q / ppi, prem = q - img * ppi;
        const int y0 = (prem / ppr) * PH, x0 = (prem % ppr) << 4;
        if (a.stats && img != simg) {
            flush(simg);
            simg = img;
        }
        float s1 = 0.f, s2 = 0.f;
        if constexpr (abl::noepi) asm volatile("" ::"v"(acc[0]), "v"(acc[1]));       // timing only: no epilogue at all
        if constexpr (kWide && !abl::noepi) {
            // the wave's 64 x 32 tile through LDS (64-byte rows; a 16-lane group of the 16-byte reads below covers four
            // whole rows = all 64 banks once)
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int row = i * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
                    const float u = acc[i][r];
                    const bf16_t vo = (bf16_t)shm_lrelu_max(u, a.slope);      // LeakyReLU for 0 <= slope <= 1 (checked by the launcher)
                    const float v = (float)vo;
                    s1 += v;
                    s2 = __builtin_fmaf(v, v, s2);
                    tile[row * 32 + l31] = __builtin_bit_cast(unsigned short, vo);
                }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");        // same-wave LDS hand-off
            const int rr = lane >> 2, ch = lane & 3;
            const int n = n0 + wn * 32 + ch * 8;
            const bool part0 = __builtin_amdgcn_readfirstlane(n0 + wn * 32) < a.n1;
            int gpc = 0, gp = 0;
            const unsigned short* gaux = nullptr;
            if constexpr (GS) {
                // A wave's 32 channels lie in one part (n1 % 32 == 0).  aux is read eight bytes (four channels) at a time, in two
                // passes over the tile: 16-byte reads with eight channels of partial sums per lane put the kernel over its 256 VGPRs
                // (the weights were spilled inside the MFMA loop)
                gp = part0 ? 0 : 1;                        // wave-uniform: pointers, pitches and the part test stay in SGPRs
                gpc = gp ? a.nout - a.n1 : a.n1;
                gaux = a.gred[gp] ? (const unsigned short*)a.gaux[gp] : nullptr;
            }
#pragma unroll
            for (int it = 0; it < 4; ++it) {
                const int row = it * 16 + rr;
                const u32x4 v = *(const u32x4*)(tile + row * 32 + (ch << 3));
                const int py = 4 * wm + (row >> 4), px = row & 15;
                const unsigned opix = (unsigned)((img * a.hi + (y0 + py)) * a.wi + (x0 + px));
                // the wave's 32 channels lie in one output part (n1 % 32 == 0): a scalar branch -- a per-lane choice of the buffer
                // descriptor makes hipcc wrap every store in a readfirstlane (waterfall) loop
                if constexpr (abl::nostore)
                    asm volatile("" ::"v"(v), "v"(opix));                           // timing only
                else if (part0)
                    __builtin_amdgcn_raw_buffer_store_b128(v, rsy, (opix * (unsigned)a.ldy + (unsigned)n) * 2u, 0, 0);
                else
                    __builtin_amdgcn_raw_buffer_store_b128(v, rsy2, (opix * (unsigned)a.ldy2 + (unsigned)(n - a.n1)) * 2u, 0, 0);
            }
            if constexpr (GS) {
                if (gaux) {                                               // wave-uniform
                    // recompute the lane's coordinates per patch: hoisted out of the patch loop they (and every address derived
                    // from them) stay live across the MFMA loop, which has no registers to spare
                    int ln = lane;
                    asm volatile("" : "+v"(ln));
                    const int rr = ln >> 2, ch = ln & 3;
                    const int gnl = n0 + wn * 32 + ch * 8 - (gp ? a.n1 : 0);
                    const int slot = (int)(blockIdx.x % (unsigned)a.gslots);
                    double* const dst = a.gred[gp] + ((size_t)slot * a.gbatch * gpc + (size_t)img * gpc + gnl) * 2;
                    // (aux has the extent of its output part, which the launcher checked to be below 4 GiB: 32-bit offsets)
                    const __amdgpu_buffer_rsrc_t rsa = __builtin_amdgcn_make_buffer_rsrc((void*)gaux, 0, 0xfffffff0u, 0x00020000);
                    const unsigned ldab = (unsigned)a.ldgaux[gp] * 2u;
#pragma unroll
                    for (int half = 0; half < 2; ++half) {
                        typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
                        u32x2 av[4];
#pragma unroll
                        for (int it = 0; it < 4; ++it) {
                            const int row = it * 16 + rr;
                            const unsigned opix = (unsigned)((img * a.hi + (y0 + 4 * wm + (row >> 4))) * a.wi + (x0 + (row & 15)));
                            av[it] = __builtin_bit_cast(u32x2, __builtin_amdgcn_raw_buffer_load_b64(rsa, opix * ldab + (unsigned)(gnl + 4 * half) * 2u, 0, 0));
                        }
                        float t[8];            // t[0..3] = sum v, t[4..7] = sum v * aux of channels 4 half .. 4 half + 3
#pragma unroll
                        for (int e = 0; e < 8; ++e) t[e] = 0.f;
#pragma unroll
                        for (int it = 0; it < 4; ++it) {
                            const int row = it * 16 + rr;
                            const u32x2 v = *(const u32x2*)(tile + row * 32 + (ch << 3) + 4 * half);
#pragma unroll
                            for (int e = 0; e < 2; ++e) {
                                const float v0 = __uint_as_float(v[e] << 16), v1 = __uint_as_float(v[e] & 0xffff0000u);
                                const float a0 = __uint_as_float(av[it][e] << 16), a1 = __uint_as_float(av[it][e] & 0xffff0000u);
                                t[2 * e] += v0;
                                t[2 * e + 1] += v1;
                                t[4 + 2 * e] += v0 * a0;
                                t[4 + 2 * e + 1] += v1 * a1;
                            }
                        }
                        // reduce-scatter of the eight sums over the sixteen lanes rr of a channel group: three halving steps over
                        // lane bits 5, 4, 3 leave value index rr >> 1 (bit 2 of rr = moment, bits 1-0 = channel), a last add over
                        // lane bit 2 completes it; the even-rr lane adds it: one atomic instruction per pass
#pragma unroll
                        for (int st = 0; st < 3; ++st) {
                            const int hf = 4 >> st, bit = 32 >> st;
                            const bool up = (ln & bit) != 0;
#pragma unroll
                            for (int e = 0; e < hf; ++e) {
                                const float keep = up ? t[hf + e] : t[e];
                                const float send = up ? t[e] : t[hf + e];
                                t[e] = keep + __shfl_xor(send, bit, 64);
                            }
                        }
                        const float tot = t[0] + __shfl_xor(t[0], 4, 64);
                        const int vi = rr >> 1;                                   // 0..3: sum v of channel vi; 4..7: sum v * aux of channel vi - 4
                        if ((rr & 1) == 0) atomicAdd(dst + (size_t)(4 * half + (vi & 3)) * 2 + (vi >> 2), (double)tot);
                    }
                }
            }
        } else if constexpr (!abl::noepi) {
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int row = i * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
                    const int py = 4 * wm + (row >> 4), px = row & 15;
                    const unsigned opix = (unsigned)((img * a.hi + (y0 + py)) * a.wi + (x0 + px));
                    const float u = acc[i][r];
                    const float v = shm_lrelu_max(u, a.slope);
                    s1 += v;
                    s2 = __builtin_fmaf(v, v, s2);
                    if (__builtin_amdgcn_readfirstlane(n0 + wn * 32) < a.n1) {        // wave-uniform (n1 % 32 == 0): no waterfall loop
                        if (ncol < a.nout)
                            __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v), rsy, (opix * (unsigned)a.ldy + (unsigned)ncol) * 4u, 0, 0);
                    } else if (ncol < a.nout) {
                        __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v), rsy2, (opix * (unsigned)a.ldy2 + (unsigned)(ncol - a.n1)) * 4u, 0, 0);
                    }
                }
        }
        S1 += s1;
        S2 += s2;
        // halo(q + 1) was issued at the top of this patch; the only younger operations of this wave are this epilogue's
        // stores (bf16 outputs: exactly four 16-byte store instructions, plus the rare statistics flush), which stay in flight
        if constexpr (abl::nostore || abl::noepi) {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        } else if constexpr (kWide && GS) {
            if (a.gred[n0 + wn * 32 < a.n1 ? 0 : 1])                 // wave-uniform: four stores and the gsum atomic
                asm volatile("s_waitcnt vmcnt(5)" ::: "memory");
            else
                asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
        } else if constexpr (kWide)
            asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
        else
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
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
    if (a.stats) flush(simg);
}

// One form: its instantiation and the name the profiler gives it (which ends at the last argument that is not a default)
template <typename TO, int NCH, bool GS = false, int NM = 0>
static void wreg_launch(const TapGemmArgs& a, dim3 grid, int np8, hipStream_t st) {
    hipLaunchKernelGGL((tapgemm_wreg_kernel<TO, NCH, GS, NM>), grid, dim3(256), 0, st, a, np8);
    shm_set_last_kernel("tapgemm_wreg_kernel<%s, %d%s>", shm_tg_name<TO>(), NCH, NM == 2 ? ", false, 2" : NM == 1 ? ", false, 1" : GS ? ", true" : "");
}

// NCH 32-channel chunks of input; the gsum and norm forms exist for bf16 outputs only
template <typename TO, int NCH>
static void wreg_launch_t(const TapGemmArgs& a, const TapGemmPlan& p, dim3 grid, int np8, hipStream_t st) {
    if constexpr (sizeof(TO) == 2) {
        if (p.gs_fused) return wreg_launch<TO, NCH, true>(a, grid, np8, st);
        if (a.nt && a.ntmode) return wreg_launch<TO, NCH, false, 2>(a, grid, np8, st);
        if (a.nt) return wreg_launch<TO, NCH, false, 1>(a, grid, np8, st);
    }
    wreg_launch<TO, NCH>(a, grid, np8, st);
}

int shm_wreg_launch(const TapGemmArgs& a, const TapGemmPlan& p, int np8, int ncu, int dtype, hipStream_t st, const char* who) {
    const int ny = shm_cdiv(a.nout, 64);
    int gx = 2 * ncu / ny;             // two 4-wave blocks per CU (LDS, VGPRs).  tests/stats_ref.py (wreg_per) mirrors this grid: a lane adds one 32-value sum per patch to its fp32 statistics
    if (gx < 1) gx = 1;
    if (gx > np8) gx = np8;
    const dim3 grid(gx, ny, 1);
    if (dtype == SHM_BF16)
        a.K == 64 ? wreg_launch_t<bf16_t, 2>(a, p, grid, np8, st) : wreg_launch_t<bf16_t, 1>(a, p, grid, np8, st);
    else
        a.K == 64 ? wreg_launch_t<float, 2>(a, p, grid, np8, st) : wreg_launch_t<float, 1>(a, p, grid, np8, st);
    return SHM_OK;
}
