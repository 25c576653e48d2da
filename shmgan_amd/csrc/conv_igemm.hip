// Implicit-GEMM convolution family on v_mfma_f32_32x32x2_f32 (exact fp32) and, for the bf16 path,
// v_mfma_f32_32x32x16_bf16 (bf16 operands, fp32 accumulate) -- gfx950.
//
// One kernel ("tap GEMM") serves Conv2D forward (k=1/3, stride 1/2), its input-gradient
// (stride 1: flipped taps; stride 2: four output phases) and Conv2DTranspose forward
// (= input-gradient of the stride-2 conv):
//
//     out[pix(m), n] = act( bias[n] + sum_{tap} sum_{k<K} A[src(m, tap), k] * B[tap][n][k] )
//
//   M = batch * grid_h * grid_w output positions of one phase, N = output channels,
//   K = channels of the A tensor (multiple of 16 fp32 / 32 bf16).  A is NHWC (optionally the
//   channel concat of two tensors), B is [tap][N][K] (K contiguous), so both operands are staged
//   as 64-byte rows (16 floats or 32 bf16) and each lane feeds four consecutive f32 MFMAs (or one
//   bf16 MFMA) from one 16-byte LDS read (the k order inside a group is permuted identically for
//   A and B, which a dot product does not see).
//
// Block = 4 waves of 64x64 outputs each (2x2 MFMA tiles), block tile 128x128 (Cout > 64) or
// 128x64; operands go HBM/L2 -> LDS by DMA three stages deep (tapgemm_dma_kernel), or through an
// 18x18 LDS halo for unit-stride 3x3 layers (tapgemm_halo_kernel).
//
// This file: the entry points, the argument block's finishing step, the variant choice (tapgemm_plan) and the launcher that switches on it.
// The kernels live one family per translation unit, each behind a launch function of tapgemm.h: conv_dma.hip (tapgemm_dma_kernel),
// conv_halo.hip (tapgemm_halo_kernel), conv_wreg.hip / conv_wreg_f32.hip (the weights-in-registers kernels), conv_phase4.hip
// (tapgemm_phase4_kernel), beside conv_wreg16.hip, conv_pingpong.hip and conv_fwd_x3.hip; their shared device helpers are tapgemm_dev.h.
#include "tapgemm.h"

// What a composite entry point asks of a product beyond the product itself, and what the launcher tells it back
struct ConvExtras {
    double* stats = nullptr;            // shm_conv2d_in_fwd: fused forward statistics (TapGemmArgs::stats, hw, stats_slots)
    int stats_hw = 0, stats_slots = 1;
    const void* gaux[2] = {};           // the *_gsum entry points (TapGemmArgs::gaux, ldgaux, gred)
    int ldgaux[2] = {};
    double* gred[2] = {};
    ShmNormReq norm = {};               // shm_conv2d_in_fwd_norm (TapGemmArgs::nt, ntpart, ntc, ntmode)
    // out: the kernel that ran took the gsum request in its epilogue (otherwise the entry point follows up with the stand-alone reduce
    // pass, shm_gsum_reduce_internal)
    bool gsum_fused = false;
};

// Variant choice, for the finished argument block of a product with operands of `esz` and outputs of `oesz` bytes per element; it launches
// nothing and calls no HIP API.  `forced` (shm_set_tuning("tapgemm.variant", SHM_TG_*)) overrides the automatic choice; a forced
// variant the shape is not eligible for is an error (SHM_E_SHAPE) at its launch, so a parity test that forces a variant knows it ran.
// two_src: the A operand is the concat of two tensors (a launch has x2 for it; shm_conv2d_norm_supported describes a shape and has no
// operands: its null pointers read as "aligned").  want_norm: source a.ntpart with a.ntc channels is to be normalised on the fly.
static TapGemmPlan tapgemm_plan(const TapGemmArgs& a, int batch, int nphase, int esz, int oesz, bool two_src, bool want_norm) {
    const int BKE = 64 / esz;
    const int forced = shm_tune(SHM_TUNE_TAPGEMM_VARIANT);
    // the 16x16-patch halo kernels: unit-stride 3x3 (forward or flipped taps), whole patches
    bool halo_ok = nphase == 1 && a.is == 1 && a.os == 1 && a.ph[0].ntaps == 9 && a.hi % 16 == 0 && a.wi % 16 == 0 && a.hg == a.hi && a.wg == a.wi;
    if (halo_ok)
        for (int t = 0; t < 9; ++t)             // every tap within the 1-pixel halo
            halo_ok = halo_ok && a.ph[0].dh[t] >= -1 && a.ph[0].dh[t] <= 1 && a.ph[0].dw[t] >= -1 && a.ph[0].dw[t] <= 1;
    const bool bk32_ok = a.K % (2 * BKE) == 0 && (!two_src || a.c1 % (2 * BKE) == 0);
    // weights-in-registers kernel: bf16, one source tensor with 32 or 64 channels
    const bool wreg_ok = esz == 2 && halo_ok && !two_src && (a.K == 32 || a.K == 64) && a.ybytes != 0 && (a.y2 == nullptr || a.y2bytes != 0) &&
                         a.slope >= 0.f && a.slope <= 1.f &&
                         (oesz == 4 || (a.nout % 64 == 0 && a.n1 % 32 == 0 && a.ldy % 8 == 0 && ((size_t)a.y & 15) == 0 &&
                                        (a.y2 == nullptr || (a.ldy2 % 8 == 0 && ((size_t)a.y2 & 15) == 0))));
    // ... and its fp32 form: 16 or 64 input channels
    // (also 16 / 32 output channels on 32- / 16-row patches, K = 32, and SpecSeg's Concatenate of two 16-channel tensors into 16)
    const int wreg32_wn = a.nout % 64 == 0 ? 4 : a.nout == 32 ? 2 : a.nout == 16 ? 1 : 0;
    const bool wreg32_ok = esz == 4 && oesz == 4 && halo_ok && (!two_src || (a.c1 == 16 && a.K == 32 && a.nout == 16)) && a.ybytes != 0 &&
                           (a.y2 == nullptr || a.y2bytes != 0) && a.slope >= 0.f && a.slope <= 1.f && a.n1 % 16 == 0 &&
                           ((wreg32_wn == 4 && (a.K == 16 || a.K == 32 || a.K == 64)) || (wreg32_wn == 2 && a.hi % 16 == 0 && (a.K == 16 || a.K == 32)) ||
                            (wreg32_wn == 1 && a.hi % 32 == 0 && (a.K == 16 || a.K == 32)));
    // the four phases of a stride-2 transposed product fused in one block: 16 x 16 input patches, 64-channel output slices
    bool phase4_ok = nphase == 4 && a.is == 1 && a.os == 2 && !two_src && a.y2 == nullptr && a.stats == nullptr && a.hi % 16 == 0 &&
                     a.wi % 16 == 0 && a.hg == a.hi && a.wg == a.wi && a.ho == 2 * a.hi && a.wo == 2 * a.wi && a.nout % 64 == 0 &&
                     a.ph[0].ntaps == 4 && a.ph[1].ntaps == 2 && a.ph[2].ntaps == 2 && a.ph[3].ntaps == 1;
    if (phase4_ok)
        for (int p = 0; p < 4; ++p)
            for (int t = 0; t < a.ph[p].ntaps; ++t)
                phase4_ok = phase4_ok && a.ph[p].dh[t] >= -1 && a.ph[p].dh[t] <= 1 && a.ph[p].dw[t] >= -1 && a.ph[p].dw[t] <= 1;
    int v = forced;
    if (v == SHM_TG_AUTO) {
        const long tiles128 = (long)shm_cdiv(a.M, 128) * shm_cdiv(a.nout, 128) * nphase;
        if (wreg_ok || wreg32_ok) {
            v = SHM_TG_WREG;
        } else if (phase4_ok && (long)batch * (a.hi / 16) * (a.wi / 16) * (a.nout / 64) >= shm_tune(SHM_TUNE_TAPGEMM_PHASE4_MIN) &&
                   (esz == 2 || a.K <= 256)) {
            // tools/bench_phase4.py, n = 40 / 8: Conv2DTranspose 128 -> 64 fp32 832 vs 1153 us (bf16 184 vs 304), 256 -> 128 751 vs 863
            // (135 vs 229); stride-2 input gradient 64 <- 128, n = 96: 498 vs 645 (113 vs 148).  One 8-wave block per CU (120 KiB of
            // LDS), so from 512 input channels on the fp32 DMA tiles (two blocks per CU, long K loops) are level or ahead
            // (512 -> 256: 850 vs 820 us); bf16 stays ahead (129 vs 176) down to one round of blocks.
            v = SHM_TG_PHASE4;
        } else if (halo_ok) {
            // The static-tap halo kernels beat the DMA tiles on every unit-stride 3x3 layer they can take, small grids included
            // (round-2 A/B, tools/bench_variants.py: fp32 n = 8 maps 120-134 vs 107-121 TFLOP/s).  128 or 64 output channels per
            // block: the 128-wide block is ~3 % faster when both fill the chip, but it has half the blocks -- two 8-wave (or
            // 4-wave) blocks fit a CU, i.e. 512 slots -- so below two rounds (bf16: below one) the choice goes by how full the last
            // round is (bf16 n = 8 at 32 x 32: 62 us on the 64-wide block against 76).
            const long np16 = (long)batch * (a.hi / 16) * (a.wi / 16);
            const long nb128 = np16 * shm_cdiv(a.nout, 128), nb64 = np16 * shm_cdiv(a.nout, 64);
            auto fill = [](long nb) { return (double)nb / (double)(((nb + 511) / 512) * 512); };
            if (esz == 4 && nb64 < 256)
                // fewer 64-wide halo blocks than CUs (SpecSeg's deep layers at n = 8, any model at batch 1): the 64 x 64 DMA tile
                // has four times the blocks -- fp32 n = 8: 128 -> 128 @32x32 99 -> 50 us, 256 -> 256 @16x16 165 -> 77,
                // 128 -> 64 @64x64 100 -> 70; level with the halo block in bf16, where it is not taken
                v = SHM_TG_DMA_64x64;
            else if (a.nout <= 64)
                v = SHM_TG_HALO64_ST;
            else if (esz == 4 && nb128 < shm_tune(SHM_TUNE_TAPGEMM_HALO_MIN))
                // fp32 is MFMA bound, so what counts is the busiest CU: blocks are dealt out over 256 CUs, a 64-wide block is half
                // the work at ~4 % less efficiency.  Matches every A/B point of tools/bench_variants.py (n = 2..40 on the 128-, 256-
                // and 512-channel layers), e.g. 320 blocks (n = 40, 32 x 32, 256 <- 512): 2 units against 3 x 0.52 -- 1085 vs 865 us
                v = (double)((nb128 + 255) / 256) <= (double)((nb64 + 255) / 256) * 0.52 ? SHM_TG_HALO128_ST : SHM_TG_HALO64_ST;
            else if (nb128 >= (esz == 2 ? 512 : shm_tune(SHM_TUNE_TAPGEMM_HALO_MIN)) || fill(nb128) * 1.03 >= fill(nb64))
                v = SHM_TG_HALO128_ST;
            else
                v = SHM_TG_HALO64_ST;
        } else if ((long)shm_cdiv(a.M, 64) * shm_cdiv(a.nout, 128) * nphase < 256) {
            v = SHM_TG_DMA_64x64;           // not even one 64x128 tile per CU
        } else if (nphase == 1 && a.nout > 64 && a.K <= (esz == 2 ? 256 : 128) &&
                   (long)shm_cdiv(a.M, 256) * shm_cdiv(a.nout, 128) >= 256) {
            // stride-2 forward products with a short K loop (discriminator blocks, Conv2DTranspose input gradients): eight waves on a
            // 256 x 128 tile amortise the per-step barrier and the weight slice over twice the rows (tools/bench_s2.py: bf16 64 -> 128
            // @256x256 n = 40 230 -> 183 us, n = 96 @128x128 135 -> 110; fp32 859 -> 801, 522 -> 490; from K = 256 (fp32) / 512 (bf16) on it loses)
            v = SHM_TG_DMA_256x128;
        } else if (nphase == 1 && a.nout > 64 && bk32_ok && (esz == 2 ? a.K >= 256 : (a.K >= 256 && a.K < 512 && a.is == 2 && tiles128 >= 512))) {
            // long K: twice the channels per K step -- twice the MFMAs per barrier (bf16 256 -> 512 @32x32 n = 96: 109 -> 88 us, 512 -> 1024
            // @16x16: 108 -> 83; fp32 stride-2 forward 256 -> 512 @64x64 n = 40: 807 -> 749 us, @32x32 n = 96: 486 -> 462, round 3 tools/bench_s2.py)
            v = SHM_TG_DMA_128x128_BK32;
        } else if (a.nout > 64 && tiles128 < shm_tune(SHM_TUNE_TAPGEMM_SMALL_GRID)) {
            // small grids (16x16 maps, the n = 8 pass of the stride-2 / transposed layers): 64-row tiles double the number of
            // blocks, so a CU holds two waves per SIMD instead of one and the K-step bubbles of one wave hide behind the other's MFMAs
            v = SHM_TG_DMA_64x128;
        } else if (a.nout > 64) {
            v = SHM_TG_DMA_128x128;
        } else {
            v = SHM_TG_DMA_128x64;
        }
    }
    // gsum (input-gradient launches): which kernels take the sums in their epilogue.  The LDS-staged bf16 epilogues read aux 16
    // bytes at a time; the DMA tiles need whole wave tiles per sample; the weights-in-registers kernels have gsum instantiations for
    // 64 output channels per block; the fused four-phase kernel has none.  Anything else: the entry point runs the reduce pass.
    const bool want_gs = a.gred[0] || a.gred[1];
    bool gs_fused = false;
    if (want_gs) {
        bool al = true;
        for (int p = 0; p < 2; ++p)
            if (a.gred[p]) al = al && (oesz == 4 || (a.ldgaux[p] % 8 == 0 && ((size_t)a.gaux[p] & 15) == 0));
        al = al && (a.y2 == nullptr || a.n1 % 32 == 0);
        // the epilogues read aux with 32-bit offsets under a descriptor of 0xfffffff0 bytes.  aux has the output's pixels but a pitch of its own,
        // so its extent is checked by itself: an aux the offsets cannot reach sends the sums to the reduce pass (64-bit addresses)
        bool aux32 = true;
        for (int p = 0; p < 2; ++p)
            if (a.gred[p]) aux32 = aux32 && (size_t)batch * a.ho * a.wo * a.ldgaux[p] * esz < 0xfffffff0ull;
        al = al && aux32;
        const bool small = aux32 && a.ybytes != 0 && (a.y2 == nullptr || a.y2bytes != 0);        // 32-bit offsets into aux and the outputs
        // bf16 outputs: the sums are taken in the LDS-staged 16-byte store path, which has its own alignment conditions
        const bool wide_ok = oesz == 4 || ((a.nout % 8 == 0) && (a.n1 % 8 == 0) && (a.ldy % 8 == 0) && (((size_t)a.y & 15) == 0) &&
                                           (a.y2 == nullptr || ((a.ldy2 % 8 == 0) && (((size_t)a.y2 & 15) == 0))));
        al = al && wide_ok;
        switch (v) {
        case SHM_TG_HALO128_ST: case SHM_TG_HALO64_ST:          // (the other halo forms are forced-only variants: reduce pass)
            gs_fused = al && small && (a.y2 == nullptr || a.n1 % 64 == 0);
            break;
        case SHM_TG_DMA_128x128: case SHM_TG_DMA_64x128: case SHM_TG_DMA_128x64: case SHM_TG_DMA_64x64: case SHM_TG_DMA_256x64:
        case SHM_TG_DMA_256x128: case SHM_TG_DMA_128x128_BK32: case SHM_TG_DMA_128x128_NST4:
            // (al holds aux32 for the 32-bit aux offsets of the fast element-store epilogue, conv_dma.hip "fastep"; the wide and the plain
            // element-store epilogues index aux through size_t and would not need it)
            gs_fused = al && (a.hg * a.wg) % 64 == 0;
            break;
        case SHM_TG_WREG:
            gs_fused = al && small && ((wreg_ok && oesz == 2) || (wreg32_ok && wreg32_wn == 4 && !two_src));
            break;
        case SHM_TG_PHASE4:                                     // fp32 outputs only (the element-store epilogue)
            gs_fused = oesz == 4 && small && a.gred[1] == nullptr;
            break;
        default:
            break;
        }
    }
    // norm: the kernels that stage the A operand as a halo image in LDS (static-tap halo blocks, weights-in-registers kernels) can
    // normalise it there; the part's channels must fit the LDS table and be whole 64-byte rows
    bool norm_ok = false;
    if (want_norm) {
        const int pc = a.ntpart ? a.K - a.c1 : a.c1;
        norm_ok = !want_gs && nphase == 1 && a.ntc == pc && pc % BKE == 0 && pc <= SHM_NT_MAXC && (a.ntpart == 0 || two_src);
        switch (v) {
        case SHM_TG_HALO128_ST: case SHM_TG_HALO64_ST:
            norm_ok = norm_ok && halo_ok && oesz == esz;
            break;
        case SHM_TG_WREG:           // one source; its planes travel as one 1 KiB DMA piece per wave
            norm_ok = norm_ok && a.ntpart == 0 && pc <= 64 && ((wreg_ok && oesz == 2) || (wreg32_ok && wreg32_wn == 4 && !two_src));
            break;
        default:
            norm_ok = false;
        }
    }
    // "conv.f32_split" (opt-in): the fp32 static-tap halo layers (and the weights-in-registers layers) as six bf16 MFMA products (conv_fwd_x3.hip)
    const bool x3 = esz == 4 && oesz == 4 && shm_tune(SHM_TUNE_CONV_F32_SPLIT) == 1 && halo_ok && (!want_norm || a.ntmode == 0) &&
                    (v == SHM_TG_HALO128_ST || v == SHM_TG_HALO64_ST || (v == SHM_TG_WREG && forced == SHM_TG_AUTO)) && (!want_gs || gs_fused) && shm_x3_fwd_eligible(a);
    // "tapgemm.wreg16": the eight-wave kernel with 16-column wave tiles and line-wide stores (tapgemm_wreg16_bf16_kernel): plain bf16 -> bf16
    // launches from one source tensor whose 64-channel blocks lie in one output part
    // "tapgemm.wreg16" = 2 (default): the K = 64 layers on maps of 8 x 32-pixel patches take the ping-pong kernel (conv_pingpong.hip)
    const int w16 = shm_tune(SHM_TUNE_TAPGEMM_WREG16);
    int wreg16 = 0;
    if (v == SHM_TG_WREG && wreg_ok && oesz == 2 && w16 != 0 && !gs_fused && !want_norm && a.nout % 64 == 0 && (a.y2 == nullptr || a.n1 % 64 == 0) && !two_src &&
        a.ybytes != 0 && (a.y2 == nullptr || a.y2bytes != 0))
        wreg16 = w16 == 2 && shm_pp_eligible(a) ? 2 : 1;
    return TapGemmPlan{v, gs_fused, norm_ok, halo_ok, bk32_ok, wreg_ok, wreg32_ok, phase4_ok, wreg32_wn, x3, wreg16};
}

// The rest of the argument block, after the product (operands, geometry, phase table) its entry point filled: the requests of `ex`, the
// operand checks and the buffer extents.  An empty product (a.M == 0 or a.nout == 0) is left without extents: there is nothing to launch.
static int finish_args(TapGemmArgs& a, int batch, int nphase, int dtype, bool two_src, const char* who, const ConvExtras& ex) {
    SHM_REQUIRE(dtype == SHM_F32 || dtype == SHM_BF16 || dtype == SHM_BF16_GF32, SHM_E_DTYPE,
                "%s: dtype %d not in {SHM_F32, SHM_BF16, SHM_BF16_GF32}", who, dtype);
    a.stats = ex.stats;
    a.hw = ex.stats_hw;
    a.stats_slots = ex.stats_slots;
    a.stats_stride = (unsigned)batch * (unsigned)a.nout * 2u;
    for (int p = 0; p < 2; ++p) {
        a.gaux[p] = ex.gaux[p];
        a.ldgaux[p] = ex.ldgaux[p];
        a.gred[p] = ex.gred[p];
    }
    a.gslots = SHM_GSUM_SLOTS;
    a.gbatch = batch;
    a.nt = ex.norm.nt;
    a.ntpart = ex.norm.part;
    a.ntc = ex.norm.c;
    a.ntmode = ex.norm.mode;
    a.ntbytes = (unsigned)((size_t)batch * SHM_NT_PLANES * ex.norm.c * sizeof(float));
    a.wimg = 0;
    a.bias_img = 0;
    if (a.gred[0] || a.gred[1]) {
        SHM_REQUIRE(a.stats == nullptr, SHM_E_SHAPE, "%s: fused forward statistics and gsum are exclusive", who);
        a.hw = a.hg * a.wg;           // pixels per sample in the M index space of one phase
    }
    SHM_REQUIRE(dtype != SHM_BF16_GF32 || a.stats == nullptr, SHM_E_DTYPE, "%s: SHM_BF16_GF32 has no fused statistics", who);
    const int esz = dtype == SHM_F32 ? 4 : 2, bke = 64 / esz, che = 16 / esz;
    SHM_REQUIRE(a.K % bke == 0 && a.K > 0, SHM_E_SHAPE, "%s: contraction channels %d must be a multiple of %d", who, a.K, bke);
    SHM_REQUIRE(a.c1 % bke == 0, SHM_E_SHAPE, "%s: concat split %d must be a multiple of %d", who, a.c1, bke);
    SHM_REQUIRE(a.ldx % che == 0 && (!two_src || a.ldx2 % che == 0), SHM_E_SHAPE, "%s: input pitch must be a multiple of 16 bytes", who);
    // the A operand travels to LDS in 16-byte pieces, one per lane, addressed as base + a multiple of 16 bytes: the bases are 16-byte aligned
    // (a shape query has no operands: its null pointers read as aligned)
    SHM_REQUIRE(((size_t)a.x & 15) == 0 && ((size_t)a.x2 & 15) == 0, SHM_E_SHAPE, "%s: input tensors must be 16-byte aligned", who);
    // a pitch is at least the channel count of its tensor (rows of a smaller pitch overlap: the result would depend on the store order).  The one
    // exception is the compact RGB image: one 16-byte chunk per pixel under a 64-byte weight row (include/shmgan_hip.h, conv_rgb.hip)
    const bool compact_rgb = !two_src && a.ldx * esz == 16 && a.K * esz == 64;
    SHM_REQUIRE(compact_rgb || a.ldx >= a.c1, SHM_E_SHAPE, "%s: input pitch %d below the source's %d channels", who, a.ldx, a.c1);
    SHM_REQUIRE(!two_src || a.ldx2 >= a.K - a.c1, SHM_E_SHAPE, "%s: input pitch %d of the second source below its %d channels", who, a.ldx2, a.K - a.c1);
    SHM_REQUIRE(a.ldy >= a.n1, SHM_E_SHAPE, "%s: output pitch %d below the part's %d channels", who, a.ldy, a.n1);
    SHM_REQUIRE(a.y2 == nullptr || a.ldy2 >= a.nout - a.n1, SHM_E_SHAPE, "%s: output pitch %d of the second part below its %d channels", who, a.ldy2, a.nout - a.n1);
    for (int p = 0; p < 2; ++p)
        SHM_REQUIRE(a.gred[p] == nullptr || a.ldgaux[p] >= (p ? a.nout - a.n1 : a.n1), SHM_E_SHAPE, "%s: aux pitch %d below the part's %d channels", who,
                    a.ldgaux[p], p ? a.nout - a.n1 : a.n1);
    SHM_REQUIRE((size_t)batch * a.hi * a.wi < (1u << 31) && (size_t)batch * a.ho * a.wo < (1u << 31), SHM_E_SHAPE, "%s: pixel count overflows int32", who);
    a.M = batch * a.hg * a.wg;
    if (a.M == 0 || a.nout == 0) return SHM_OK;
    {
        const size_t lim = 0xfffffff0ull;
        size_t xb = (size_t)batch * a.hi * a.wi * a.ldx * esz, x2b = two_src ? (size_t)batch * a.hi * a.wi * a.ldx2 * esz : 0;
        size_t wb = 0;
        for (int p = 0; p < nphase; ++p)
            for (int t = 0; t < a.ph[p].ntaps; ++t) {
                size_t e = (size_t)(a.ph[p].widx[t] + 1) * a.nout * a.K * esz;
                if (e > wb) wb = e;
            }
        if (a.nt && a.ntmode) {                   // SHM_NORM_SCALED: one weight copy and one bias row per sample
            SHM_REQUIRE(nphase == 1 && a.bias, SHM_E_SHAPE, "%s: SHM_NORM_SCALED takes per-sample weights AND per-sample bias rows", who);
            a.wimg = (unsigned)((size_t)a.ph[0].ntaps * a.nout * a.K * esz);
            a.bias_img = a.nout;
            wb = (size_t)batch * a.wimg;
        }
        SHM_REQUIRE(xb < lim && x2b < lim && wb < lim, SHM_E_SHAPE, "%s: operand larger than 4 GiB (32-bit buffer offsets)", who);
        a.xbytes = (unsigned)xb;
        a.x2bytes = (unsigned)x2b;
        a.wbytes = (unsigned)wb;
        const int oesz = dtype == SHM_BF16 ? 2 : 4;
        const size_t yb = (size_t)batch * a.ho * a.wo * a.ldy * oesz, y2b = a.y2 ? (size_t)batch * a.ho * a.wo * a.ldy2 * oesz : 0;
        // ("tapgemm.flat_epilogue": the >= 4 GiB behaviour on demand -- keeps the 64-bit-address epilogues and the variant choice without
        // the buffer-store kernels under test at sizes a test can afford)
        const bool flat = shm_tune(SHM_TUNE_TAPGEMM_FLAT_EPILOGUE) != 0;
        a.ybytes = (yb < lim && !flat) ? (unsigned)yb : 0u;
        a.y2bytes = (y2b < lim && !flat) ? (unsigned)y2b : 0u;
    }
    return SHM_OK;
}

// compute units of the device (the persistent weights-in-registers kernels size their grids by it)
static int device_cus() {
    static const int ncu = [] {
        int dev = 0, n = 0;
        if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) n = 256;
        return n;
    }();
    return ncu;
}

// The launch the plan chose.  The forced-variant checks sit with the launches: here for SHM_TG_WREG, which four kernels share, else in the family's file.
static int launch_plan(const TapGemmArgs& a, const TapGemmPlan& p, int batch, int nphase, int dtype, hipStream_t st, const char* who) {
    if (p.x3) return shm_x3_fwd_launch(a, batch, p.gs_fused, st, who);
    switch (p.variant) {
    case SHM_TG_HALO128: case SHM_TG_HALO64: case SHM_TG_HALO128_ST: case SHM_TG_HALO128_ST_W4: case SHM_TG_HALO64_ST: case SHM_TG_HALO128_PH8:
        return shm_halo_launch(a, p, batch, dtype, st, who);
    case SHM_TG_PHASE4:
        return shm_phase4_launch(a, p, batch, dtype, st, who);
    case SHM_TG_WREG: {
        SHM_REQUIRE(p.wreg_ok || p.wreg32_ok, SHM_E_SHAPE,
                    "%s: forced variant wreg needs a unit-stride 3x3 layer on a map that is a multiple of 16, slope in [0,1] and: bf16 -- one source "
                    "tensor with 32/64 channels, Cout %% 64 == 0; fp32 -- one source with 16/32/64 input channels and "
                    "Cout %% 64 == 0, or 16/32 input channels with Cout = 32 (map a multiple of 16) or 16 (map a multiple of 32; also 16 + 16 from two tensors)", who);
        const int np8 = batch * (a.hi / 8) * (a.wi / 16), ncu = device_cus();
        if (p.wreg16 == 2) return shm_pp_launch(a, batch, ncu, st, who);
        if (p.wreg16 == 1) return shm_wreg16_launch(a, np8, ncu, st, who);
        return p.wreg_ok ? shm_wreg_launch(a, p, np8, ncu, dtype, st, who) : shm_wreg_f32_launch(a, p, batch, ncu, st, who);
    }
    case SHM_TG_DMA_128x128: case SHM_TG_DMA_64x128: case SHM_TG_DMA_128x64: case SHM_TG_DMA_64x64: case SHM_TG_DMA_256x64:
    case SHM_TG_DMA_256x128: case SHM_TG_DMA_128x128_BK32: case SHM_TG_DMA_128x128_NST4:
        return shm_dma_launch(a, p, nphase, dtype, st, who);
    default:
        SHM_REQUIRE(false, SHM_E_SHAPE, "%s: unknown tapgemm.variant %d", who, p.variant);
    }
    return SHM_OK;
}

// `a`: the product (operands, geometry, phase table) as its entry point filled it; the rest of the block comes from `ex` and from here
static int launch_tapgemm(TapGemmArgs& a, int batch, int nphase, int dtype, hipStream_t st, const char* who, ConvExtras& ex) {
    const bool two_src = a.x2 != nullptr;
    if (const int r = finish_args(a, batch, nphase, dtype, two_src, who, ex)) return r;
    if (a.M == 0 || a.nout == 0) return SHM_OK;
    const int esz = dtype == SHM_F32 ? 4 : 2, oesz = dtype == SHM_BF16 ? 2 : 4;
    // the 3-channel stride-2 first layer of the discriminator on the compact image layout (conv_rgb.hip); a forced tapgemm.variant keeps
    // the generic kernels (which read K channels per tap from the 16-byte pixels: the neighbours' values times the zero weight columns)
    if (nphase == 1 && a.is == 2 && a.os == 1 && a.ph[0].ntaps == 9 && a.ph[0].dh[0] == 0 && a.ph[0].dw[0] == 0 && !a.x2 && !a.y2 && !a.gred[0] && !a.gred[1] &&
        !a.nt && a.ldx * esz == 16 && a.K * esz == 64 && a.ybytes != 0 && dtype != SHM_BF16_GF32 &&
        shm_tune(SHM_TUNE_TAPGEMM_VARIANT) == SHM_TG_AUTO) {
        const int r = shm_rgb_s2_fwd_launch(a.x, a.ldx, a.w, a.K, a.bias, a.y, a.ldy, batch, a.hi, a.wi, a.nout, a.slope, a.stats, a.stats_slots, a.stats_stride,
                                            a.xbytes, a.ybytes, dtype, st);
        if (r < 0) return r;
        if (r == 1) return SHM_OK;
    }
    const TapGemmPlan p = tapgemm_plan(a, batch, nphase, esz, oesz, two_src, a.nt != nullptr);
    ex.gsum_fused = p.gs_fused;
    if (!p.gs_fused) a.gred[0] = a.gred[1] = nullptr;          // the entry point follows up with the reduce pass
    SHM_REQUIRE(a.nt == nullptr || p.norm_ok, SHM_E_SHAPE,
                "%s: the kernel this shape runs on (tapgemm variant %d) cannot normalise its source in LDS (unit-stride 3x3 on a map that is a "
                "multiple of 16, normalised part of at most %d channels; ask shm_conv2d_norm_supported) -- use shm_in_apply", who, p.variant, SHM_NT_MAXC);
    if (const int r = launch_plan(a, p, batch, nphase, dtype, st, who)) return r;
    SHM_LAUNCH_CHECK(who);
    return SHM_OK;
}

// ------------------------------------------------------------------------------------
// [ntaps][rows][cols] -> [ntaps][cols][rows_pad]
template <typename T>
__global__ void transpose_taps_kernel(const float* __restrict__ w, T* __restrict__ wt, int rows, int cols, int rows_pad) {
    __shared__ float tile[32][33];
    const int t = blockIdx.z;
    const int r0 = blockIdx.y * 32, c0 = blockIdx.x * 32;
    const float* src = w + (size_t)t * rows * cols;
    T* dst = wt + (size_t)t * cols * rows_pad;
    for (int i = threadIdx.y; i < 32; i += blockDim.y) {
        int r = r0 + i, c = c0 + threadIdx.x;
        tile[i][threadIdx.x] = (r < rows && c < cols) ? src[(size_t)r * cols + c] : 0.f;
    }
    __syncthreads();
    for (int i = threadIdx.y; i < 32; i += blockDim.y) {
        int c = c0 + i, r = r0 + threadIdx.x;
        if (c < cols && r < rows_pad) dst[(size_t)c * rows_pad + r] = (T)tile[threadIdx.x][i];
    }
}

extern "C" int shm_transpose_taps(const float* w, void* wt, int ntaps, int rows, int cols, int rows_pad, int dtype, void* stream) {
    SHM_REQUIRE(rows_pad >= rows && ntaps > 0 && rows > 0 && cols > 0, SHM_E_SHAPE, "shm_transpose_taps: bad shape");
    SHM_REQUIRE(dtype == SHM_F32 || dtype == SHM_BF16, SHM_E_DTYPE, "shm_transpose_taps: bad dtype %d", dtype);
    dim3 grid(shm_cdiv(cols, 32), shm_cdiv(rows_pad, 32), ntaps);
    if (dtype == SHM_BF16)
        hipLaunchKernelGGL(transpose_taps_kernel<bf16_t>, grid, dim3(32, 8), 0, (hipStream_t)stream, w, (bf16_t*)wt, rows, cols, rows_pad);
    else
        hipLaunchKernelGGL(transpose_taps_kernel<float>, grid, dim3(32, 8), 0, (hipStream_t)stream, w, (float*)wt, rows, cols, rows_pad);
    SHM_LAUNCH_CHECK("shm_transpose_taps");
    return SHM_OK;
}

// Every layer's transpose of one model in ONE launch (the per-layer launches are 4.5 us each, 27 per step, in front of the
// forward pass): block -> (layer, tap, 32 x 32 tile) through a prefix table in the kernel arguments.
constexpr int kMaxTransposes = 48;
struct TransposeBatch {
    const float* w[kMaxTransposes];
    void* wt[kMaxTransposes];
    int rows[kMaxTransposes], cols[kMaxTransposes], rows_pad[kMaxTransposes];
    int tx[kMaxTransposes], ty[kMaxTransposes];      // tiles along cols / rows_pad
    int block0[kMaxTransposes + 1];                  // first block of each layer
    int count;
};

template <typename T>
__global__ void transpose_taps_multi_kernel(const TransposeBatch b) {
    __shared__ float tile[32][33];
    int l = 0;
    while (l + 1 < b.count && (int)blockIdx.x >= b.block0[l + 1]) ++l;            // block-uniform scan (<= 48 entries)
    const int rows = b.rows[l], cols = b.cols[l], rows_pad = b.rows_pad[l];
    int rem = (int)blockIdx.x - b.block0[l];
    const int per_tap = b.tx[l] * b.ty[l];
    const int t = rem / per_tap;
    rem -= t * per_tap;
    const int r0 = (rem / b.tx[l]) * 32, c0 = (rem % b.tx[l]) * 32;
    const float* src = b.w[l] + (size_t)t * rows * cols;
    T* dst = (T*)b.wt[l] + (size_t)t * cols * rows_pad;
    for (int i = threadIdx.y; i < 32; i += blockDim.y) {
        int r = r0 + i, c = c0 + threadIdx.x;
        tile[i][threadIdx.x] = (r < rows && c < cols) ? src[(size_t)r * cols + c] : 0.f;
    }
    __syncthreads();
    for (int i = threadIdx.y; i < 32; i += blockDim.y) {
        int c = c0 + i, r = r0 + threadIdx.x;
        if (c < cols && r < rows_pad) dst[(size_t)c * rows_pad + r] = (T)tile[threadIdx.x][i];
    }
}

extern "C" int shm_transpose_taps_multi(int count, const void* const* w, void* const* wt, const int* ntaps, const int* rows, const int* cols,
                                        const int* rows_pad, int dtype, void* stream) {
    SHM_REQUIRE(count >= 0 && count <= kMaxTransposes, SHM_E_SHAPE, "shm_transpose_taps_multi: %d layers (at most %d)", count, kMaxTransposes);
    SHM_REQUIRE(dtype == SHM_F32 || dtype == SHM_BF16, SHM_E_DTYPE, "shm_transpose_taps_multi: bad dtype %d", dtype);
    if (count == 0) return SHM_OK;
    SHM_REQUIRE(w && wt && ntaps && rows && cols && rows_pad, SHM_E_SHAPE, "shm_transpose_taps_multi: null table");
    TransposeBatch b{};
    b.count = count;
    int total = 0;
    for (int l = 0; l < count; ++l) {
        SHM_REQUIRE(w[l] && wt[l] && rows_pad[l] >= rows[l] && ntaps[l] > 0 && rows[l] > 0 && cols[l] > 0, SHM_E_SHAPE,
                    "shm_transpose_taps_multi: bad shape of layer %d", l);
        b.w[l] = (const float*)w[l];
        b.wt[l] = wt[l];
        b.rows[l] = rows[l];
        b.cols[l] = cols[l];
        b.rows_pad[l] = rows_pad[l];
        b.tx[l] = shm_cdiv(cols[l], 32);
        b.ty[l] = shm_cdiv(rows_pad[l], 32);
        b.block0[l] = total;
        total += ntaps[l] * b.tx[l] * b.ty[l];
    }
    b.block0[count] = total;
    if (dtype == SHM_BF16)
        hipLaunchKernelGGL(transpose_taps_multi_kernel<bf16_t>, dim3(total), dim3(32, 8), 0, (hipStream_t)stream, b);
    else
        hipLaunchKernelGGL(transpose_taps_multi_kernel<float>, dim3(total), dim3(32, 8), 0, (hipStream_t)stream, b);
    SHM_LAUNCH_CHECK("shm_transpose_taps_multi");
    return SHM_OK;
}

// ------------------------------------------------------------------------------------
// SHM_NORM_SCALED operands of a convolution whose source part [part_lo, part_lo + c) is the un-normalised activation a of an
// InstanceNorm block with table nt (common.h): conv(w, (a - mean) * inv + beta) = conv(w * inv, a) + sum w * (beta - mean * inv) inside
// the image, so per sample n
//   wk_n[n][tap][co][k] = wk[tap][co][k] * inv_n[k - part_lo]  (k in the part; the other channels are copied)
//   bias_n[n][co]       = bias[co] + sum_{tap, k in part} wk[tap][co][k] * (beta[k'] - mean_n[k'] * inv_n[k'])
// (the kernels write `ring` over out-of-image taps, whose product with the scaled weight cancels that tap's share of bias_n).
// One block per (co, sample).
template <typename T>
__global__ __launch_bounds__(256) void norm_prepare_kernel(const T* __restrict__ wk, const float* __restrict__ bias, const float* __restrict__ nt, int c,
                                                           int part_lo, T* __restrict__ wk_n, float* __restrict__ bias_n, int ntaps, int cout, int K) {
    const int co = blockIdx.x, n = blockIdx.y;
    const float* mean = nt + (size_t)n * SHM_NT_PLANES * c;
    const float *inv = mean + c, *beta = mean + 2 * c;
    float acc = 0.f;
    for (int i = threadIdx.x; i < ntaps * K; i += 256) {
        const int tap = i / K, k = i - tap * K;
        const size_t src = ((size_t)tap * cout + co) * K + k;
        const float w = (float)wk[src];
        float o = w;
        const int kp = k - part_lo;
        if (kp >= 0 && kp < c) {
            o = w * inv[kp];
            acc += w * (beta[kp] - mean[kp] * inv[kp]);
        }
        wk_n[(size_t)n * ntaps * cout * K + src] = (T)o;
    }
    __shared__ float red[4];
    acc = shm_wave_sum(acc);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) bias_n[(size_t)n * cout + co] = (bias ? bias[co] : 0.f) + ((red[0] + red[1]) + (red[2] + red[3]));
}

extern "C" int shm_conv2d_norm_prepare(const void* wk, const float* bias, const float* nt, int c, int part_lo, void* wk_n, float* bias_n, int batch,
                                       int cin, int cout, int ksize, int dtype, void* stream) {
    SHM_REQUIRE(wk && nt && wk_n && bias_n, SHM_E_SHAPE, "shm_conv2d_norm_prepare: null pointer");
    SHM_REQUIRE(ksize == 1 || ksize == 3, SHM_E_SHAPE, "shm_conv2d_norm_prepare: ksize %d not in {1,3}", ksize);
    SHM_REQUIRE(c > 0 && part_lo >= 0 && part_lo + c <= cin, SHM_E_SHAPE, "shm_conv2d_norm_prepare: part [%d, %d) outside %d channels", part_lo, part_lo + c, cin);
    if (batch == 0 || cout == 0) return SHM_OK;
    SHM_DISPATCH(dtype, "shm_conv2d_norm_prepare",
                 hipLaunchKernelGGL(norm_prepare_kernel<T>, dim3(cout, batch), dim3(256), 0, (hipStream_t)stream, (const T*)wk, bias, nt, c, part_lo, (T*)wk_n,
                                    bias_n, ksize * ksize, cout, cin));
    SHM_LAUNCH_CHECK("shm_conv2d_norm_prepare");
    return SHM_OK;
}

// ------------------------------------------------------------------------------------
// The part of the argument block the forward forms share: one source of K channels, weights [taps][nout][K], bias and LeakyReLU, one
// destination of nout channels.  Callers add a second source / destination and the output geometry with its phase table.
static TapGemmArgs fwd_args(const void* x, int ldx, const void* w, const float* bias, void* y, int ldy, int hi, int wi, int K, int nout, float slope) {
    TapGemmArgs a{};
    a.x = x;
    a.c1 = K;
    a.ldx = ldx;
    a.w = w;
    a.bias = bias;
    a.y = y;
    a.n1 = nout;
    a.ldy = ldy;
    a.hi = hi;
    a.wi = wi;
    a.K = K;
    a.nout = nout;
    a.slope = slope;
    return a;
}

// One phase of ksize x ksize taps: tap (kh, kw) reads the source at sign * ((kh, kw) - (pt, pl)) from the output pixel
static void fill_taps(TapPhase& P, int ksize, int pt, int pl, int sign) {
    P.oph = P.opw = 0;
    P.ntaps = ksize * ksize;
    for (int kh = 0; kh < ksize; ++kh)
        for (int kw = 0; kw < ksize; ++kw) {
            int t = kh * ksize + kw;
            P.dh[t] = sign * (kh - pt);
            P.dw[t] = sign * (kw - pl);
            P.widx[t] = t;
        }
}

// The forward product: SAME padding, one phase of ksize x ksize taps.  c1 = channels of the first source (cin when there is no second)
static TapGemmArgs conv_fwd_args(const void* x, const void* x2, int c1, int ldx, int ldx2, const void* wk, const float* bias, void* y, int ldy, int hi, int wi,
                                 int cin, int cout, int ksize, int stride, float slope) {
    TapGemmArgs a = fwd_args(x, ldx, wk, bias, y, ldy, hi, wi, cin, cout, slope);
    a.x2 = x2;
    a.c1 = c1;
    a.ldx2 = ldx2;
    int ho, wo, pt, pl;
    shm_same_pad(hi, ksize, stride, &ho, &pt);
    shm_same_pad(wi, ksize, stride, &wo, &pl);
    a.hg = a.ho = ho;
    a.wg = a.wo = wo;
    a.is = stride;
    a.os = 1;
    fill_taps(a.ph[0], ksize, pt, pl, 1);
    return a;
}

// shm_conv2d_fwd and every entry point that is a forward product with extras
static int conv_fwd_impl(const void* x, const void* x2, int c1, int ldx, int ldx2, const void* wk, const float* bias, void* y, int ldy, int batch, int hi,
                         int wi, int cin, int cout, int ksize, int stride, float slope, int dtype, void* stream, ConvExtras& ex) {
    SHM_REQUIRE(ksize == 1 || ksize == 3, SHM_E_SHAPE, "shm_conv2d_fwd: ksize %d not in {1,3}", ksize);
    SHM_REQUIRE(stride == 1 || stride == 2, SHM_E_SHAPE, "shm_conv2d_fwd: stride %d not in {1,2}", stride);
    SHM_REQUIRE(x && wk && y, SHM_E_SHAPE, "shm_conv2d_fwd: null pointer");
    TapGemmArgs a = conv_fwd_args(x, x2, x2 ? c1 : cin, ldx, ldx2, wk, bias, y, ldy, hi, wi, cin, cout, ksize, stride, slope);
    return launch_tapgemm(a, batch, 1, dtype, (hipStream_t)stream, "shm_conv2d_fwd", ex);
}

extern "C" int shm_conv2d_fwd(const void* x, const void* x2, int c1, int ldx, int ldx2, const void* wk,
                              const float* bias, void* y, int ldy, int batch, int hi, int wi, int cin,
                              int cout, int ksize, int stride, float slope, int dtype, void* stream) {
    ConvExtras ex;
    return conv_fwd_impl(x, x2, c1, ldx, ldx2, wk, bias, y, ldy, batch, hi, wi, cin, cout, ksize, stride, slope, dtype, stream, ex);
}

extern "C" int shm_conv2d_in_fwd(const void* x, const void* x2, int c1, int ldx, int ldx2, const void* wk,
                                 const float* bias, void* y, int ldy, int batch, int hi, int wi, int cin,
                                 int cout, int ksize, int stride, float slope, double* stats, double* scratch,
                                 float eps, int dtype, void* stream) {
    return shm_conv2d_in_fwd_norm(x, x2, c1, ldx, ldx2, nullptr, nullptr, SHM_NORM_EXACT, wk, bias, y, ldy, batch, hi, wi, cin, cout, ksize, stride, slope, stats,
                                  scratch, eps, nullptr, nullptr, dtype, stream);
}

// Does the kernel that shm_conv2d_in_fwd_norm would run for this shape normalise its source in LDS?  The launcher's own argument-finishing
// step and plan (which depends on the shape, the batch and the tuning knobs) on the shape's argument block without operands, as for a
// SHM_NORM_EXACT request for source norm_part: nothing is launched.
extern "C" int shm_conv2d_norm_supported(int batch, int hi, int wi, int cin, int c1, int cout, int ksize, int stride, int norm_part, int dtype) {
    if (dtype != SHM_F32 && dtype != SHM_BF16) return 0;
    if ((ksize != 1 && ksize != 3) || (stride != 1 && stride != 2) || batch <= 0 || cin <= 0 || cout <= 0) return 0;
    if (norm_part != 0 && norm_part != 1) return 0;
    const bool two = c1 > 0 && c1 < cin;
    if (norm_part == 1 && !two) return 0;
    ConvExtras ex;
    ex.norm.part = norm_part;
    ex.norm.c = two ? (norm_part ? cin - c1 : c1) : cin;
    TapGemmArgs a = conv_fwd_args(nullptr, nullptr, two ? c1 : cin, two ? c1 : cin, two ? cin - c1 : 0, nullptr, nullptr, nullptr, cout, hi, wi, cin, cout, ksize,
                                  stride, 0.2f);
    if (finish_args(a, batch, 1, dtype, two, "shm_conv2d_fwd", ex) != SHM_OK || a.M == 0 || a.nout == 0) return 0;
    const int esz = dtype == SHM_F32 ? 4 : 2;
    return tapgemm_plan(a, batch, 1, esz, esz, two, true).norm_ok ? 1 : 0;
}

extern "C" int shm_conv2d_in_fwd_norm(const void* x, const void* x2, int c1, int ldx, int ldx2, const float* nt_x, const float* nt_x2, int norm_mode,
                                      const void* wk, const float* bias, void* y, int ldy, int batch, int hi, int wi, int cin, int cout, int ksize,
                                      int stride, float slope, double* stats, double* scratch, float eps, float* nt_out, const float* beta_out, int dtype,
                                      void* stream) {
    SHM_REQUIRE(stats, SHM_E_SHAPE, "shm_conv2d_in_fwd: null stats");
    ConvExtras ex;
    if (const int r = shm_norm_request(&ex.norm, "shm_conv2d_in_fwd_norm", nt_x, nt_x2, norm_mode, x2, c1, cin)) return r;
    SHM_REQUIRE(!nt_out || beta_out, SHM_E_SHAPE, "shm_conv2d_in_fwd_norm: nt_out needs beta_out");
    int ho, wo, pt;
    shm_same_pad(hi, ksize, stride, &ho, &pt);
    shm_same_pad(wi, ksize, stride, &wo, &pt);
    const int hw = ho * wo;
    if (!shm_tune(SHM_TUNE_STATS_FUSION) || hw % 64 != 0) {       // tiny maps: separate statistics pass
        int r = conv_fwd_impl(x, x2, c1, ldx, ldx2, wk, bias, y, ldy, batch, hi, wi, cin, cout, ksize, stride, slope, dtype, stream, ex);
        if (r) return r;
        r = shm_in_stats(y, ldy, stats, batch, hw, cout, eps, dtype, stream);
        if (r == SHM_OK && nt_out) r = shm_in_norm_table(stats, beta_out, nt_out, batch, cout, stream);
        return r;
    }
    // Every wave tile of a sample adds its column sums with f64 atomics: on one copy that is hw/64 atomics
    // per address, a serial chain worth ~100 us at 256x256 whatever the batch (measured, bf16 and fp32).
    // With `scratch` the chain is cut SHM_STATS_SLOTS-fold and the finalize kernel sums the copies.
    // `scratch` is zero on entry by contract and left zero (the finalize kernel clears what it sums); without it the
    // sums go to `stats`, which is zeroed here.
    ex.stats = scratch ? scratch : stats;
    ex.stats_slots = scratch ? SHM_STATS_SLOTS : 1;
    ex.stats_hw = hw;
    int r = scratch ? SHM_OK : shm_zero(stats, (size_t)batch * cout * 2 * sizeof(double), stream);
    if (r) return r;
    r = conv_fwd_impl(x, x2, c1, ldx, ldx2, wk, bias, y, ldy, batch, hi, wi, cin, cout, ksize, stride, slope, dtype, stream, ex);
    if (r == SHM_OK) r = shm_in_finalize_internal(stats, scratch, ex.stats_slots, batch * cout, hw, (double)eps, nt_out, beta_out, cout, (hipStream_t)stream);
    // "zero on entry, zero on return" also on the error path: a failed launch must not leave sums behind
    if (r != SHM_OK && scratch) (void)hipMemsetAsync(scratch, 0, (size_t)SHM_STATS_SLOTS * batch * cout * 2 * sizeof(double), (hipStream_t)stream);
    return r;
}

// Transposed stride-2 product shared by Conv2DTranspose forward and the stride-2 dgrad:
//   out[2a+ph] = sum_{k : k = ph+pt (mod 2)} A[a + (ph+pt-k)/2] * B[k]
static void fill_s2_phases(TapGemmArgs& a, int pt, int pl) {
    for (int ph = 0; ph < 2; ++ph)
        for (int pw = 0; pw < 2; ++pw) {
            TapPhase& P = a.ph[ph * 2 + pw];
            P.oph = ph;
            P.opw = pw;
            int nt = 0;
            for (int kh = 0; kh < 3; ++kh) {
                if (((ph + pt - kh) & 1) != 0) continue;
                for (int kw = 0; kw < 3; ++kw) {
                    if (((pw + pl - kw) & 1) != 0) continue;
                    P.dh[nt] = (ph + pt - kh) / 2;   // exact
                    P.dw[nt] = (pw + pl - kw) / 2;
                    P.widx[nt] = kh * 3 + kw;
                    ++nt;
                }
            }
            P.ntaps = nt;
        }
}

// 2x upsampling geometry: every pixel of the A map owns a 2 x 2 block of output pixels, one phase each
static void up2_geometry(TapGemmArgs& a) {
    a.hg = a.hi;
    a.wg = a.wi;
    a.ho = 2 * a.hi;
    a.wo = 2 * a.wi;
    a.is = 1;
    a.os = 2;
}

// shm_conv2d_dgrad and shm_conv2d_dgrad_gsum
static int conv_dgrad_impl(const void* dy, int lddy, const void* w, void* dx, void* dx2, int n1, int lddx, int lddx2, int batch, int hi, int wi, int cin,
                           int cout, int ksize, int stride, int dtype, void* stream, ConvExtras& ex) {
    SHM_REQUIRE(ksize == 1 || ksize == 3, SHM_E_SHAPE, "shm_conv2d_dgrad: ksize %d not in {1,3}", ksize);
    SHM_REQUIRE(stride == 1 || (stride == 2 && ksize == 3), SHM_E_SHAPE, "shm_conv2d_dgrad: stride %d unsupported", stride);
    SHM_REQUIRE(dy && w && dx, SHM_E_SHAPE, "shm_conv2d_dgrad: null pointer");
    int ho, wo, pt, pl;
    shm_same_pad(hi, ksize, stride, &ho, &pt);
    shm_same_pad(wi, ksize, stride, &wo, &pl);
    // HWIO [t][cin][cout] == [t][N=cin][K=cout]; no bias, no activation (slope 1)
    TapGemmArgs a = fwd_args(dy, lddy, w, nullptr, dx, lddx, ho, wo, cout, cin, 1.f);
    a.y2 = dx2;
    a.n1 = dx2 ? n1 : cin;
    a.ldy2 = lddx2;
    if (stride == 1) {
        a.hg = a.ho = hi;
        a.wg = a.wo = wi;
        a.is = a.os = 1;
        fill_taps(a.ph[0], ksize, pt, pl, -1);      // dx[p] = sum_t dy[p - (k - pad)] * W_t^T
        return launch_tapgemm(a, batch, 1, dtype, (hipStream_t)stream, "shm_conv2d_dgrad", ex);
    }
    SHM_REQUIRE(hi % 2 == 0 && wi % 2 == 0, SHM_E_SHAPE, "shm_conv2d_dgrad: stride 2 needs even input size");
    up2_geometry(a);            // (hi, wi even: 2 * ho == hi)
    fill_s2_phases(a, pt, pl);
    return launch_tapgemm(a, batch, 4, dtype, (hipStream_t)stream, "shm_conv2d_dgrad", ex);
}

extern "C" int shm_conv2d_dgrad(const void* dy, int lddy, const void* w, void* dx, void* dx2, int n1,
                                int lddx, int lddx2, int batch, int hi, int wi, int cin, int cout,
                                int ksize, int stride, int dtype, void* stream) {
    ConvExtras ex;
    return conv_dgrad_impl(dy, lddy, w, dx, dx2, n1, lddx, lddx2, batch, hi, wi, cin, cout, ksize, stride, dtype, stream, ex);
}

extern "C" int shm_conv2d_transpose_fwd(const void* x, int ldx, const void* w, const float* bias, void* y,
                                        int ldy, int batch, int hi, int wi, int cin, int cout, float slope,
                                        int dtype, void* stream) {
    SHM_REQUIRE(x && w && y, SHM_E_SHAPE, "shm_conv2d_transpose_fwd: null pointer");
    // the stride-2 SAME conv that maps [2hi,2wi] back to [hi,wi] has pad_before = 0
    int ho2, wo2, pt, pl;
    shm_same_pad(2 * hi, 3, 2, &ho2, &pt);
    shm_same_pad(2 * wi, 3, 2, &wo2, &pl);
    TapGemmArgs a = fwd_args(x, ldx, w, bias, y, ldy, hi, wi, cin, cout, slope);       // Keras [t][cout][cin] == [t][N=cout][K=cin]
    up2_geometry(a);
    fill_s2_phases(a, pt, pl);
    ConvExtras ex;
    return launch_tapgemm(a, batch, 4, dtype, (hipStream_t)stream, "shm_conv2d_transpose_fwd", ex);
}

// Keras Conv2DTranspose(k=2, strides=2) (SpecSeg.py:63,69,75,81): non-overlapping, every output
// phase (ph, pw) is a 1x1 product with its own tap: y[2a+ph, 2b+pw] = bias + x[a, b] . w[ph][pw].
extern "C" int shm_conv2d_transpose2x2_fwd(const void* x, int ldx, const void* w, const float* bias, void* y,
                                           int ldy, int batch, int hi, int wi, int cin, int cout, float slope,
                                           int dtype, void* stream) {
    SHM_REQUIRE(x && w && y, SHM_E_SHAPE, "shm_conv2d_transpose2x2_fwd: null pointer");
    TapGemmArgs a = fwd_args(x, ldx, w, bias, y, ldy, hi, wi, cin, cout, slope);       // Keras [2][2][cout][cin] == [t][N=cout][K=cin]
    up2_geometry(a);
    for (int p = 0; p < 4; ++p) {
        TapPhase& P = a.ph[p];
        P.oph = p >> 1;
        P.opw = p & 1;
        P.ntaps = 1;
        P.dh[0] = P.dw[0] = 0;
        P.widx[0] = p;
    }
    ConvExtras ex;
    return launch_tapgemm(a, batch, 4, dtype, (hipStream_t)stream, "shm_conv2d_transpose2x2_fwd", ex);
}

// ------------------------------------------------------------------------------------
// gsum entry points: an input-gradient product that also delivers, per (sample, channel) of its output, sum(g) and sum(g * aux)
// -- the two sums the InstanceNorm backward of the block whose OUTPUT gradient it writes would otherwise collect in a pass of its
// own over g and the stored activation (shm_in_bwd's reduce pass).  red = f64 [SHM_GSUM_SLOTS][batch][channels][2], zero on entry
// (slot copies cut the per-address atomic chains; shm_in_bwd_apply sums and clears them).  Kernels that cannot take the sums in
// their epilogue (tapgemm_plan lists which can) are followed by the stand-alone reduce pass: callers always get the sums.
extern "C" int shm_conv2d_dgrad_gsum(const void* dy, int lddy, const void* w, void* dx, void* dx2, int n1, int lddx, int lddx2, int batch, int hi,
                                     int wi, int cin, int cout, int ksize, int stride, const void* aux, int ldaux, double* red, const void* aux2,
                                     int ldaux2, double* red2, int dtype, void* stream) {
    const char* who = "shm_conv2d_dgrad_gsum";
    SHM_REQUIRE((aux != nullptr) == (red != nullptr) && (aux2 != nullptr) == (red2 != nullptr), SHM_E_SHAPE, "%s: aux and red come in pairs", who);
    SHM_REQUIRE(red || red2, SHM_E_SHAPE, "%s: no sums requested (use shm_conv2d_dgrad)", who);
    SHM_REQUIRE(!red2 || dx2, SHM_E_SHAPE, "%s: sums of the second part need dx2", who);
    ConvExtras ex;
    ex.gaux[0] = aux, ex.ldgaux[0] = ldaux, ex.gred[0] = red;
    ex.gaux[1] = aux2, ex.ldgaux[1] = ldaux2, ex.gred[1] = red2;
    int r = conv_dgrad_impl(dy, lddy, w, dx, dx2, n1, lddx, lddx2, batch, hi, wi, cin, cout, ksize, stride, dtype, stream, ex);
    if (r == SHM_OK && !ex.gsum_fused) {
        const int c0 = dx2 ? n1 : cin;
        if (red) r = shm_gsum_reduce_internal(dx, lddx, aux, ldaux, red, batch, hi * wi, c0, dtype, (hipStream_t)stream);
        if (r == SHM_OK && red2) r = shm_gsum_reduce_internal(dx2, lddx2, aux2, ldaux2, red2, batch, hi * wi, cin - n1, dtype, (hipStream_t)stream);
    }
    return r;
}

// The stride-2 forward form is the input gradient of Conv2DTranspose (model.py runs it with slope 1 and no bias); any forward
// product may ask for the sums of its output.
extern "C" int shm_conv2d_fwd_gsum(const void* x, const void* x2, int c1, int ldx, int ldx2, const void* wk, const float* bias, void* y, int ldy,
                                   int batch, int hi, int wi, int cin, int cout, int ksize, int stride, float slope, const void* aux, int ldaux,
                                   double* red, int dtype, void* stream) {
    const char* who = "shm_conv2d_fwd_gsum";
    SHM_REQUIRE(aux && red, SHM_E_SHAPE, "%s: null aux / red", who);
    ConvExtras ex;
    ex.gaux[0] = aux, ex.ldgaux[0] = ldaux, ex.gred[0] = red;
    int r = conv_fwd_impl(x, x2, c1, ldx, ldx2, wk, bias, y, ldy, batch, hi, wi, cin, cout, ksize, stride, slope, dtype, stream, ex);
    if (r == SHM_OK && !ex.gsum_fused) {
        int ho, wo, pt;
        shm_same_pad(hi, ksize, stride, &ho, &pt);
        shm_same_pad(wi, ksize, stride, &wo, &pt);
        r = shm_gsum_reduce_internal(y, ldy, aux, ldaux, red, batch, ho * wo, cout, dtype, (hipStream_t)stream);
    }
    return r;
}
