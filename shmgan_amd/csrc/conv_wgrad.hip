// Convolution weight gradient on v_mfma_f32_32x32x2_f32 (exact fp32) and, for the bf16 path, on
// v_mfma_f32_32x32x16_bf16 with transposed LDS reads (wgrad_bf16_kernel) -- gfx950.
//
//   dW[tap][ci][co] = sum_{pixels p} X[src(p, tap)][ci] * dY[p][co]
//
// GEMM view per tap: M = ci, N = co, K = pixels.  Both operands are pixel-major in HBM
// (channels contiguous), which is exactly the [k][m] / [k][n] LDS image the f32 MFMA's
// one-float-per-lane operands want: 32 lanes read 32 consecutive floats (conflict-free
// ds_read_b32), the two lane halves read two consecutive pixels.
//
// One block = a 64(ci) x 64(co) tile for ALL taps over one slice of the pixels (split-K):
// the dY tile is staged once per 16 pixels and shared by the 9 taps; the 9 shifted X tiles
// are fetched through L1/L2.  Wave w owns the 32x32 sub-tile (w>>1, w&1) of every tap
// (9 accumulators).  Partial slabs go to a workspace and are summed in a fixed order by
// wgrad_reduce_kernel (deterministic, no float atomics).
//
// This file: the entry points, the kernel choice and split (wgrad_plan), the launcher that switches on it, the slab reduction and the norm-finish
// kernel.  The kernels live one family per translation unit, each behind a launch function of wgrad.h: conv_wgrad_gen.hip (wgrad_kernel,
// wgrad_bf16_kernel: described above), conv_wgrad_halo.hip (wgrad_halo_kernel, wgrad_halo_thin_kernel), conv_wgrad_halo16.hip
// (wgrad_halo_bf16_kernel), conv_wgrad_halo8.hip (wgrad_halo8_bf16_kernel), beside conv_wgrad_x3.hip and conv_rgb.hip's first-layer kernel.
// The halo-staged ones share their patch order, edge bits and stage ring through wgrad_halo_dev.h; the plan below counts patches in that order.
#include "wgrad.h"

#include <stdint.h>

// dw[i] (+)= sum_k part[k][i], summed in a fixed order (4 interleaved chains, then 0+1+2+3).
__global__ __launch_bounds__(256) void wgrad_reduce_kernel(const float* __restrict__ part, float* __restrict__ dw, size_t n, int nsplit, int accumulate) {
    __shared__ float red[4][64];
    const int e = threadIdx.x & 63, g = threadIdx.x >> 6;
    const size_t i = (size_t)blockIdx.x * 64 + e;
    float s = 0.f;
    if (i < n)
        for (int k = g; k < nsplit; k += 4) s += part[(size_t)k * n + i];
    red[g][e] = s;
    __syncthreads();
    if (g == 0 && i < n) {
        float t = ((red[0][e] + red[1][e]) + red[2][e]) + red[3][e];
        dw[i] = accumulate ? dw[i] + t : t;
    }
}

// 16 bytes per lane and SIXTEEN interleaved chains per element group (slab k goes to chain k % 16, four loads in flight per
// chain, chains combined as a fixed tree): a reduce is a chain of dependent slab loads -- with four chains and up to 1024 slabs
// every launch took 13 (bf16) to 26 us (fp32) whatever its size, 49 launches per step.  Deterministic (fixed order); the order
// differs from wgrad_reduce_kernel's, which keeps serving element counts that are not a multiple of four.  n % 4 == 0.
__global__ __launch_bounds__(256) void wgrad_reduce4_kernel(const float* __restrict__ part, float* __restrict__ dw, size_t n4, int nsplit, int accumulate) {
    __shared__ f32x4 red[16][16];
    const int e = threadIdx.x & 15, g = threadIdx.x >> 4;
    const size_t i = (size_t)blockIdx.x * 16 + e;               // group of four elements
    f32x4 s = {0.f, 0.f, 0.f, 0.f};
    if (i < n4) {
        const f32x4* p = (const f32x4*)part + i;
        int k = g;
        for (; k + 48 < nsplit; k += 64) {
            const f32x4 a = p[(size_t)k * n4], b = p[(size_t)(k + 16) * n4], c = p[(size_t)(k + 32) * n4], d = p[(size_t)(k + 48) * n4];
            s += a;
            s += b;
            s += c;
            s += d;
        }
        for (; k < nsplit; k += 16) s += p[(size_t)k * n4];
    }
    red[g][e] = s;
    __syncthreads();
    if (g == 0 && i < n4) {
        f32x4 t[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) t[q] = red[2 * q][e] + red[2 * q + 1][e];
        const f32x4 r = ((t[0] + t[1]) + (t[2] + t[3])) + ((t[4] + t[5]) + (t[6] + t[7]));
        f32x4* o = (f32x4*)dw + i;
        *o = accumulate ? *o + r : r;
    }
}

// Splits for a block target: `tiles` (ci, co) tiles share one slice of the M pixels; "wgrad.blocks" overrides the default target
static int wgrad_block_splits(long M, int tiles, int default_target) {
    const int target_tuned = shm_tune(SHM_TUNE_WGRAD_BLOCKS);
    const int target = target_tuned ? target_tuned : default_target;
    int want = shm_cdiv(target, tiles);
    long maxs = (M + 255) / 256;                 // at least 256 pixels per split
    if (want > maxs) want = (int)maxs;
    if (want < 1) want = 1;
    return want;
}

static int wgrad_splits(int batch, int ho, int wo, int cin, int cout, int esz = 4) {
    // two 256-thread blocks fit per CU (LDS): two rounds of 512 blocks keep every CU busy and
    // the split-K slab traffic (ns * 9*cin*cout floats written + read) small
    long M = (long)batch * ho * wo;
    int tiles = shm_cdiv(cin, 64) * shm_cdiv(cout, 64);
    // (bf16: the MFMA kernel is ~6x faster, so the slab traffic of the split weighs more and the launches, which run on the
    // second stream beside the input-gradient chain, should leave that chain room: 256 blocks measured best with the four-row
    // stages -- step 25.8 ms at 512, 24.9 at 256, 25.3 at 384, 26.1 at 192, 29.7 at 128; fp32: 1024 (122.3 ms; 512: 123.3, 2048: 122.9))
    return wgrad_block_splits(M, tiles, esz == 2 ? 256 : 1024);
}

// What the shape alone can promise (no dtype, no stride: the trainer sizes its arena with it).  Beside the fp32 split-K target it allows for
// the kernels that write more slabs than that target has splits:
extern "C" size_t shm_conv2d_wgrad_workspace(int batch, int ho, int wo, int cin, int cout, int ksize) {
    int ns = wgrad_splits(batch, ho, wo, cin, cout);
    if (9 * cin <= kWgradThinRows) ns *= kWgradThinSlabs;                               // wgrad_halo_thin_kernel writes two slabs per split
    if (9 * cin <= kWgradRgbRows && ns < kWgradRgbSlabs) ns = kWgradRgbSlabs;           // conv3x3s2_rgb_wgrad_kernel (conv_rgb.hip): one slab per block, streaming -- blocks are what it needs
    if (shm_tune(SHM_TUNE_WGRAD_BLOCKS)) ns *= kWgradHalo8CoTiles;                      // wgrad_halo8_bf16_kernel: half as many (ci, co) tiles, twice the splits for a given block target
    return (size_t)ns * ksize * ksize * cin * cout * sizeof(float);
}

// SHM_NORM_SCALED: a block's patches must lie in one sample -- the largest divisor of the patches per image that does not exceed
// the split the automatic choice would take
static int wgrad_norm_aligned_pps(int pps, int ppi) {
    int d = pps > ppi ? ppi : pps;
    if (d < 1) d = 1;
    while (ppi % d) --d;
    return d;
}

// The split cut: at most `want` splits of the npatch patches, whole patches per split (align_ppi != 0: a divisor of the align_ppi patches
// per image, wgrad_norm_aligned_pps), and the count of splits that are not empty
struct WgradCut {
    int pps, splits;
};
static WgradCut wgrad_cut(int npatch, int want, int align_ppi = 0) {
    const int n = want < npatch ? want : npatch;
    int pps = shm_cdiv(npatch, n < 1 ? 1 : n);
    if (align_ppi) pps = wgrad_norm_aligned_pps(pps, align_ppi);
    if (pps < 1) pps = 1;                        // (an empty batch: no split, the launch fails)
    return WgradCut{pps, shm_cdiv(npatch, pps)};
}

// Pixel rows per stage of the bf16-operand halo kernels (wgrad_halo_bf16_kernel, wgrad_halo8_bf16_kernel<0>, wgrad_halo_x3_kernel): four where
// the kernel has that form and the map allows, "wgrad.bf16_rows" = 2 keeps two
static int wgrad_stage_rows(int hi, bool has_four = true) { return has_four && hi % 4 == 0 && shm_tune(SHM_TUNE_WGRAD_BF16_ROWS) != 2 ? 4 : 2; }

// One weight gradient as its entry point describes it: the shape, the operand type and the pitches (elements).  two: the input is the concat
// of two tensors (a launch has x2 for it; shm_conv2d_wgrad_norm_supported describes a shape and has no operands).
struct WgradShape {
    int batch, hi, wi, cin, cin_ld, c1, cout, ksize, stride, dtype;
    bool two;
    int ldx, ldx2, lddy;
    int esz() const { return dtype == SHM_BF16 ? 2 : 4; }
};

// The kernel choice and the split for a checked shape; it launches nothing, calls no HIP API and dereferences nothing.  want_nm: source nm_part
// (nm_c channels) is to be normalised on the fly in mode nm_mode (SHM_NORM_*); norm_ok says whether the shape's kernel can, and a launch
// refuses the request where it cannot.  Every "wgrad.*" tuning knob is read here (and in the helpers above), none in the launch path.
static WgradPlan wgrad_plan(const WgradShape& s, bool want_nm, int nm_part, int nm_c, int nm_mode) {
    const int batch = s.batch, hi = s.hi, wi = s.wi, cin = s.cin, cin_ld = s.cin_ld, c1 = s.c1, cout = s.cout, ksize = s.ksize, stride = s.stride;
    const int esz = s.esz(), vec = 16 / esz;
    const bool bf16 = s.dtype == SHM_BF16, two = s.two;
    int ho, wo, pt, pl;
    shm_same_pad(hi, ksize, stride, &ho, &pt);
    shm_same_pad(wi, ksize, stride, &wo, &pl);
    WgradPlan p{};
    p.bf16 = bf16;
    p.ntaps = ksize * ksize;
    const size_t slab = (size_t)p.ntaps * cin * cout * sizeof(float);
    const int ns = wgrad_splits(batch, ho, wo, cin, cout, esz);
    p.early_bytes = (size_t)ns * slab;
    const int wv = shm_tune(SHM_TUNE_WGRAD_VARIANT);       // 0 automatic, 1 generic kernels only, 2 no thin-input packing, 3 no stride-2 halo form
    // the 3-channel stride-2 first layer on the compact image layout (conv_rgb.hip); wgrad.variant 1 keeps the generic kernel
    p.try_rgb = ksize == 3 && stride == 2 && !two && s.ldx * esz == 16 && !want_nm && wv != 1;
    const bool straddle = two && (c1 % 64 != 0);
    const int no_halo = wv == 1;
    const bool halo_ok = ksize == 3 && stride == 1 && wi % 16 == 0 && hi % 2 == 0 && !straddle && !no_halo;
    const int no_thin = wv == 2;
    // thin first layers: (tap, ci) pairs packed into the MFMA rows; patches of 2 x 16 OUTPUT pixels
    const bool thin_ok = !no_thin && !no_halo && ksize == 3 && !two && 9 * cin <= kWgradThinRows && s.ldx == 16 && cin_ld <= 16 && wo % 16 == 0 && ho % 2 == 0 &&
                         hi % stride == 0 && wi % stride == 0;
    // stride 2 (wv == 3: not this form): SAME padding of an even map puts nothing before the first row / column
    const bool s2_even = ksize == 3 && stride == 2 && pt == 0 && pl == 0 && hi % 2 == 0 && wi % 2 == 0 && !straddle && !no_halo && wv != 3;
    const bool halo2_ok = s2_even && wo % 8 == 0 && ho % 2 == 0 && !(thin_ok && !bf16);
    // norm: the halo-image kernels normalise their x halo in LDS (a block's 64 input channels lie in one source: no straddle)
    if (want_nm) {
        const int pc = two ? (nm_part ? cin_ld - c1 : c1) : cin_ld;
        p.norm_ok = halo_ok && (bf16 || !thin_ok) && nm_c == pc && (nm_part == 0 || two) && pc % vec == 0;
    }
    // bf16, eight-wave block over 64 ci x 128 co (round 4): unit stride on maps whose height is a multiple of four, stride 2 on even maps
    // whose output width is a multiple of 16; "wgrad.bf16_wide" = 1 keeps the four-wave kernels
    const bool w8_s1 = halo_ok && wgrad_stage_rows(hi) == 4;
    const bool w8_s2_16 = s2_even && wo % 16 == 0 && ho % 2 == 0, w8_s2_8 = s2_even && !w8_s2_16 && wo % 8 == 0 && ho % 4 == 0;
    const bool w8_s2 = w8_s2_16 || w8_s2_8;
    // "wgrad.bf16_wide": 0 automatic = stride 2 only, 1 never, 2 stride 2 only, 3 unit stride only, 4 both.  Unit stride is NOT the
    // automatic choice although the eight-wave block is 9-27 % faster than wgrad_halo_bf16_kernel<4> launch for launch (tools/bench_wgrad_bf16.py):
    // in the two-stream step the weight gradients run on the second stream beside the input-gradient chain, which is the critical path;
    // a block that fills a CU (eight waves at 210 VGPRs, 93 KiB of LDS) for the whole launch keeps that chain's kernels off the CU, the
    // four-wave kernel at one block per CU leaves them half of it (bf16 step, S=256 B=8 / S=512 B=4 / B=32: both 25.5 / 48.9 / 89.6 ms, stride 2
    // only 25.0 / 47.8 / 88.5, neither 25.1 / 48.6 / 89.8, unit stride only 25.8 / 50.6 / 91.6).  At stride 2 it replaces wgrad_bf16_kernel<9>, which
    // needs 30-43 % more time on every layer and is no lighter on a CU.
    const int wide = shm_tune(SHM_TUNE_WGRAD_BF16_WIDE);
    const bool wide_s1 = wide == 3 || wide == 4, wide_s2 = wide == 0 || wide == 2 || wide == 4;
    // (64 output channels -- the discriminator's 3-channel first layer -- stay on wgrad_bf16_kernel<9>: with the pair's second co tile empty
    // the eight-wave block measured 296 us against 271)
    const bool w8_take_s1 = w8_s1 && wide_s1 && cout >= 128, w8_take_s2 = w8_s2 && wide_s2 && cout >= 128 && !w8_take_s1;

    // the family and its patch; `want` splits are asked of the cut (the generic kernels cut pixels, below)
    int want = ns, align_ppi = 0, slabs_per_split = 1;
    p.prow = 2;
    p.pcol = 16;
    p.rows = 2;
    if (bf16 && (w8_take_s1 || w8_take_s2) && !want_nm) {
        p.family = SHM_WG_HALO8;
        p.mode8 = w8_take_s1 ? 0 : w8_s2_16 ? 1 : 2;
        p.over_out = true;                      // (unit stride: the two maps are one)
        p.prow = p.mode8 == 1 ? 2 : 4;          // output rows / columns per stage
        p.pcol = p.mode8 == 2 ? 8 : 16;
        // one block per CU (93 KiB of LDS): the block target counts 64 x 128 tiles, i.e. twice the splits of the four-wave kernel's choice
        want = wgrad_block_splits((long)batch * ho * wo, shm_cdiv(cin, 64) * shm_cdiv(cout, 64 * kWgradHalo8CoTiles), 256);
    } else if (bf16 && halo_ok) {
        p.family = SHM_WG_HALO16;
        p.rows = p.prow = wgrad_stage_rows(hi);      // pixel rows per stage
        p.nmode = want_nm ? 1 + nm_mode : 0;
    } else if (bf16) {
        p.family = SHM_WG_GEN;
    } else if (thin_ok && stride == 2) {
        // first layer of the discriminator (3 channels, stride 2): patches over the OUTPUT map
        p.family = SHM_WG_THIN;
        p.thin_nrt = 9 * cin <= 32 ? 1 : 3;
        p.thin_is = 2;
        p.over_out = true;
    } else if (halo2_ok) {
        // stride-2 3x3 layers: patches of 2 x 8 OUTPUT pixels with a 5 x 17 input halo
        // "wgrad.f32_split" (opt-in, round 6): the six-bf16-product form on patches of 2 x 16 output pixels (conv_wgrad_x3.hip, S2)
        const bool x3s2 = shm_tune(SHM_TUNE_WGRAD_F32_SPLIT) == 1 && wo % 16 == 0 && !want_nm;
        p.family = x3s2 ? SHM_WG_X3 : SHM_WG_HALO;
        p.stride2 = true;
        p.over_out = true;
        p.pcol = x3s2 ? 16 : 8;
    } else if (halo_ok && thin_ok) {
        p.family = SHM_WG_THIN;
        p.thin_nrt = 3;
        p.thin_is = 1;
    } else if (halo_ok) {
        p.nmode = want_nm ? 1 + nm_mode : 0;
        if (p.nmode < 2 && shm_tune(SHM_TUNE_WGRAD_F32_SPLIT) == 1) {        // "wgrad.f32_split": conv_wgrad_x3.hip (plain and SHM_NORM_EXACT sources)
            // stages of four pixel rows where the map allows ("wgrad.bf16_rows" = 2 keeps two): the patches and the split are cut for them
            // (the normalising form keeps two rows: with four its 24 table values spill)
            p.family = SHM_WG_X3;
            p.rows = p.prow = wgrad_stage_rows(hi, !want_nm);
        } else
            p.family = SHM_WG_HALO;
    } else {
        p.family = SHM_WG_GEN;
    }
    if (p.family == SHM_WG_THIN) slabs_per_split = kWgradThinSlabs;
    if (p.family == SHM_WG_GEN) {
        // pixels, sixteen at a time
        p.straddle = straddle;
        p.prow = p.pcol = 1;
        p.over_out = true;
        p.npatch = batch * ho * wo;
        int pps = shm_cdiv(p.npatch, ns);
        pps = (pps + 15) / 16 * 16;
        p.patches_per_split = pps < 1 ? 1 : pps;                 // (an empty batch: no split, the launch fails)
        p.splits = shm_cdiv(p.npatch, p.patches_per_split);
    } else {
        const int ppi = p.over_out ? (ho / p.prow) * (wo / p.pcol) : (hi / p.prow) * (wi / p.pcol);
        if (p.nmode == 2) align_ppi = ppi;          // SHM_NORM_SCALED: a block's patches lie in one sample
        p.npatch = batch * ppi;
        const WgradCut cut = wgrad_cut(p.npatch, want, align_ppi);
        p.patches_per_split = cut.pps;
        p.splits = cut.splits;
    }
    p.nsplit = slabs_per_split * p.splits;
    p.ws_bytes = (size_t)p.nsplit * slab;
    if (p.ws_bytes < p.early_bytes) p.ws_bytes = p.early_bytes;
    return p;
}

// Argument checks of a launch and of shm_conv2d_wgrad_norm_supported (which has operands_ok = true and no workspace: ws_bytes = SIZE_MAX), with
// the plan in their middle: *plan is valid when this returns SHM_OK.
static int wgrad_check(const WgradShape& s, bool operands_ok, size_t ws_bytes, const ShmNormReq& nm, bool want_nm, WgradPlan* plan) {
    SHM_REQUIRE(s.dtype == SHM_F32 || s.dtype == SHM_BF16, SHM_E_DTYPE, "shm_conv2d_wgrad: dtype %d not in {SHM_F32, SHM_BF16}", s.dtype);
    const int esz = s.esz(), vec = 16 / esz;      // 16-byte loads: 4 floats / 8 bf16
    SHM_REQUIRE(s.ksize == 1 || s.ksize == 3, SHM_E_SHAPE, "shm_conv2d_wgrad: ksize %d not in {1,3}", s.ksize);
    SHM_REQUIRE(s.stride == 1 || s.stride == 2, SHM_E_SHAPE, "shm_conv2d_wgrad: stride %d not in {1,2}", s.stride);
    SHM_REQUIRE(operands_ok, SHM_E_SHAPE, "shm_conv2d_wgrad: null pointer");
    SHM_REQUIRE(s.cin_ld % vec == 0 && s.cin_ld >= s.cin && s.cout % vec == 0, SHM_E_SHAPE,
                "shm_conv2d_wgrad: cin_ld %d / cout %d must be multiples of %d", s.cin_ld, s.cout, vec);
    SHM_REQUIRE(s.ldx % vec == 0 && s.lddy % vec == 0 && (!s.two || (s.ldx2 % vec == 0 && s.c1 % vec == 0)), SHM_E_SHAPE,
                "shm_conv2d_wgrad: pitches must be multiples of %d", vec);
    // a pitch is at least the channels read through it; the compact RGB image (one 16-byte chunk per pixel under a 64-byte row, conv_rgb.hip) is the exception
    const bool compact_rgb = !s.two && s.ldx * esz == 16 && s.cin_ld * esz == 64;
    SHM_REQUIRE(compact_rgb || s.ldx >= (s.two ? s.c1 : s.cin_ld), SHM_E_SHAPE, "shm_conv2d_wgrad: input pitch %d below the source's %d channels", s.ldx,
                s.two ? s.c1 : s.cin_ld);
    SHM_REQUIRE(!s.two || s.ldx2 >= s.cin_ld - s.c1, SHM_E_SHAPE, "shm_conv2d_wgrad: input pitch %d of the second source below its %d channels", s.ldx2,
                s.cin_ld - s.c1);
    SHM_REQUIRE(s.lddy >= s.cout, SHM_E_SHAPE, "shm_conv2d_wgrad: gradient pitch %d below %d channels", s.lddy, s.cout);
    SHM_REQUIRE((size_t)s.batch * s.hi * s.wi < (1u << 31), SHM_E_SHAPE, "shm_conv2d_wgrad: pixel count overflows int32");
    *plan = wgrad_plan(s, want_nm, nm.part, nm.c, nm.mode);
    SHM_REQUIRE(ws_bytes >= plan->early_bytes, SHM_E_WORKSPACE, "shm_conv2d_wgrad: workspace %zu < %zu bytes", ws_bytes, plan->early_bytes);
    int ho, wo, pad;
    shm_same_pad(s.hi, s.ksize, s.stride, &ho, &pad);
    shm_same_pad(s.wi, s.ksize, s.stride, &wo, &pad);
    const size_t lim = 0xfffffff0ull;
    const size_t xb = (size_t)s.batch * s.hi * s.wi * s.ldx * esz, x2b = s.two ? (size_t)s.batch * s.hi * s.wi * s.ldx2 * esz : 0;
    const size_t db = (size_t)s.batch * ho * wo * s.lddy * esz;
    SHM_REQUIRE(xb < lim && x2b < lim && db < lim, SHM_E_SHAPE, "shm_conv2d_wgrad: operand larger than 4 GiB (32-bit buffer offsets)");
    return SHM_OK;
}

// Phase 1 of shm_conv2d_wgrad: the MFMA kernel the plan chose; *nsplit_out receives the number of partial slabs written.  nm: the norm request
// of shm_conv2d_wgrad_norm (WgradHaloArgs::nt).
static int launch_plan(const WgradShape& s, const WgradPlan& p, const void* x, const void* x2, const void* dy, void* workspace, size_t ws_bytes, const ShmNormReq& nm,
                       int* nsplit_out, hipStream_t st) {
    const int esz = s.esz();
    int ho, wo, pt, pl;
    shm_same_pad(s.hi, s.ksize, s.stride, &ho, &pt);
    shm_same_pad(s.wi, s.ksize, s.stride, &wo, &pl);
    const unsigned xbytes = (unsigned)((size_t)s.batch * s.hi * s.wi * s.ldx * esz), x2bytes = x2 ? (unsigned)((size_t)s.batch * s.hi * s.wi * s.ldx2 * esz) : 0;
    const unsigned dybytes = (unsigned)((size_t)s.batch * ho * wo * s.lddy * esz);
    if (p.try_rgb) {
        const int r = shm_rgb_s2_wgrad_launch(x, s.ldx, dy, s.lddy, (float*)workspace, ws_bytes, s.batch, s.hi, s.wi, s.cin, s.cout, xbytes, dybytes, s.dtype, nsplit_out, st);
        if (r < 0) return r;
        if (r == 1) return SHM_OK;
    }
    SHM_REQUIRE(ws_bytes >= p.ws_bytes, SHM_E_WORKSPACE, "shm_conv2d_wgrad: workspace %zu < %zu bytes (SHM_NORM_SCALED: shm_conv2d_wgrad_norm_workspace)", ws_bytes,
                p.ws_bytes);
    int rc;
    if (p.family == SHM_WG_GEN) {
        WgradArgs a{};
        a.x = x;
        a.x2 = x2;
        a.c1 = x2 ? s.c1 : s.cin_ld;
        a.ldx = s.ldx;
        a.ldx2 = s.ldx2;
        a.dy = dy;
        a.lddy = s.lddy;
        a.part = (float*)workspace;
        a.hi = s.hi;
        a.wi = s.wi;
        a.ho = ho;
        a.wo = wo;
        a.cin_ld = s.cin_ld;
        a.cin = s.cin;
        a.cout = s.cout;
        a.is = s.stride;
        a.ntaps = p.ntaps;
        for (int kh = 0; kh < s.ksize; ++kh)
            for (int kw = 0; kw < s.ksize; ++kw) {
                a.dh[kh * s.ksize + kw] = kh - pt;
                a.dw[kh * s.ksize + kw] = kw - pl;
            }
        a.M = p.npatch;
        a.pix_per_split = p.patches_per_split;
        a.xbytes = xbytes;
        a.x2bytes = x2bytes;
        a.dybytes = dybytes;
        rc = shm_wgrad_gen_launch(a, p, st);
    } else {
        WgradHaloArgs hgs{};
        hgs.x = x;
        hgs.x2 = x2;
        hgs.c1 = x2 ? s.c1 : s.cin_ld;
        hgs.ldx = s.ldx;
        hgs.ldx2 = s.ldx2;
        hgs.dy = dy;
        hgs.lddy = s.lddy;
        hgs.part = (float*)workspace;
        hgs.h = s.hi;
        hgs.w = s.wi;
        hgs.cin_ld = s.cin_ld;
        hgs.cin = s.cin;
        hgs.cout = s.cout;
        hgs.npatch = p.npatch;
        hgs.patches_per_split = p.patches_per_split;
        hgs.xbytes = xbytes;
        hgs.x2bytes = x2bytes;
        hgs.dybytes = dybytes;
        hgs.nt = nm.nt;
        hgs.ntpart = nm.part;
        hgs.ntc = nm.c;
        rc = p.family == SHM_WG_HALO8    ? shm_wgrad_halo8_launch(hgs, p, st)
             : p.family == SHM_WG_HALO16 ? shm_wgrad_halo16_launch(hgs, p, st)
             : p.family == SHM_WG_X3     ? shm_wgrad_x3_launch(hgs, p, st)
                                         : shm_wgrad_halo_launch(hgs, p, st);
    }
    if (rc != SHM_OK) return rc;
    SHM_LAUNCH_CHECK("shm_conv2d_wgrad");
    if (nsplit_out) *nsplit_out = p.nsplit;
    return SHM_OK;
}

static int wgrad_partial_impl(const void* x, const void* x2, int c1, int ldx, int ldx2, const void* dy, int lddy, int batch, int hi, int wi, int cin,
                              int cin_ld, int cout, int ksize, int stride, void* workspace, size_t ws_bytes, int dtype, int* nsplit_out, void* stream,
                              const ShmNormReq& nm) {
    const WgradShape s{batch, hi, wi, cin, cin_ld, c1, cout, ksize, stride, dtype, x2 != nullptr, ldx, ldx2, lddy};
    WgradPlan p;
    if (const int r = wgrad_check(s, x && dy && workspace, ws_bytes, nm, nm.nt != nullptr, &p)) return r;
    // both operands travel in 16-byte pieces addressed as base + a multiple of 16 bytes
    SHM_REQUIRE(((size_t)x & 15) == 0 && ((size_t)x2 & 15) == 0 && ((size_t)dy & 15) == 0, SHM_E_SHAPE, "shm_conv2d_wgrad: x, x2 and dy must be 16-byte aligned");
    SHM_REQUIRE(!nm.nt || p.norm_ok, SHM_E_SHAPE,
                "shm_conv2d_wgrad_norm: the kernel this shape runs on cannot normalise its source in LDS (unit-stride 3x3, map width a multiple of "
                "16, concat split a multiple of 64; ask shm_conv2d_wgrad_norm_supported) -- use shm_in_apply");
    return launch_plan(s, p, x, x2, dy, workspace, ws_bytes, nm, nsplit_out, (hipStream_t)stream);
}

// Phase 2: dw[i] (+)= sum over the nsplit slabs, in a fixed order.
extern "C" int shm_conv2d_wgrad_reduce(const void* workspace, float* dw, size_t n, int nsplit, int accumulate, void* stream) {
    SHM_REQUIRE(workspace && dw && nsplit >= 1, SHM_E_SHAPE, "shm_conv2d_wgrad_reduce: bad arguments");
    if (n == 0) return SHM_OK;
    if (n % 4 == 0 && ((size_t)workspace & 15) == 0 && ((size_t)dw & 15) == 0)
        hipLaunchKernelGGL(wgrad_reduce4_kernel, dim3(shm_cdiv((long)(n / 4), 16)), dim3(256), 0, (hipStream_t)stream, (const float*)workspace, dw, n / 4,
                           nsplit, accumulate);
    else
        hipLaunchKernelGGL(wgrad_reduce_kernel, dim3(shm_cdiv((long)n, 64)), dim3(256), 0, (hipStream_t)stream, (const float*)workspace, dw, n, nsplit,
                           accumulate);
    SHM_LAUNCH_CHECK("shm_conv2d_wgrad(reduce)");
    return SHM_OK;
}

// Would shm_conv2d_wgrad_norm run on a kernel that normalises its source in LDS?  The argument checks and the plan of a SHM_NORM_EXACT request
// for source norm_part on packed operands (pitch = channel count); nothing is launched.
extern "C" int shm_conv2d_wgrad_norm_supported(int batch, int hi, int wi, int cin, int cin_ld, int c1, int cout, int ksize, int stride, int norm_part, int dtype) {
    if (dtype != SHM_F32 && dtype != SHM_BF16) return 0;
    if (norm_part != 0 && norm_part != 1) return 0;
    const bool two = c1 > 0 && c1 < cin_ld;
    if (norm_part == 1 && !two) return 0;
    const ShmNormReq nm{nullptr, norm_part, two ? (norm_part ? cin_ld - c1 : c1) : cin_ld, SHM_NORM_EXACT};
    const WgradShape s{batch, hi, wi, cin, cin_ld, two ? c1 : 0, cout, ksize, stride, dtype, two, two ? c1 : cin_ld, two ? cin_ld - c1 : 0, cout};
    WgradPlan p;
    return wgrad_check(s, true, SIZE_MAX, nm, true, &p) == SHM_OK && p.norm_ok ? 1 : 0;
}

// Workspace of shm_conv2d_wgrad_norm(SHM_NORM_SCALED): the splits are cut on sample boundaries, which can take more slabs than
// shm_conv2d_wgrad_workspace allows for.
extern "C" size_t shm_conv2d_wgrad_norm_workspace(int batch, int hi, int wi, int cin, int cout, int ksize, int dtype) {
    const int esz = dtype == SHM_BF16 ? 2 : 4;
    const int ns = wgrad_splits(batch, hi, wi, cin, cout, esz);
    const int rows = dtype == SHM_BF16 ? wgrad_stage_rows(hi) : 2;
    if (hi % rows || wi % 16) return shm_conv2d_wgrad_workspace(batch, hi, wi, cin, cout, ksize);
    const int ppi = (hi / rows) * (wi / 16);
    const size_t aligned = (size_t)wgrad_cut(batch * ppi, ns, ppi).splits * ksize * ksize * cin * cout * sizeof(float);
    const size_t plain = shm_conv2d_wgrad_workspace(batch, hi, wi, cin, cout, ksize);
    return aligned > plain ? aligned : plain;
}

// SHM_NORM_SCALED, the second term of the weight gradient: dw[tap][part_lo + k][co] += sum_n (beta[k] - mean_n[k] * inv_n[k]) * dzsum[n][co]
// for every tap (with `ring` in the out-of-image taps the sum over the pixels does not depend on the tap).  dzsum = per-sample channel
// sums of dz (the dz_sums output of shm_in_bwd and its kin).
__global__ __launch_bounds__(256) void wgrad_norm_finish_kernel(float* __restrict__ dw, const float* __restrict__ nt, const double* __restrict__ dzsum, int batch,
                                                                int c, int part_lo, int cin, int cout, int ntaps) {
    // a thread owns one (k, co) pair and walks the samples four at a time (independent loads in flight: as a chain of `batch`
    // round trips the kernel took 60-80 us)
    const int co = blockIdx.x * 64 + (threadIdx.x & 63), k = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (co >= cout || k >= c) return;
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
    const size_t ts = (size_t)SHM_NT_PLANES * c;
    int n = 0;
    for (; n + 3 < batch; n += 4) {
        const float* t = nt + (size_t)n * ts + k;
        const float m0 = t[0], i0 = t[c], b0 = t[2 * c], m1 = t[ts], i1 = t[ts + c], b1 = t[ts + 2 * c];
        const float m2 = t[2 * ts], i2 = t[2 * ts + c], b2 = t[2 * ts + 2 * c], m3 = t[3 * ts], i3 = t[3 * ts + c], b3 = t[3 * ts + 2 * c];
        const double d0 = dzsum[(size_t)n * cout + co], d1 = dzsum[(size_t)(n + 1) * cout + co], d2 = dzsum[(size_t)(n + 2) * cout + co],
                     d3 = dzsum[(size_t)(n + 3) * cout + co];
        s0 += ((double)b0 - (double)m0 * (double)i0) * d0;
        s1 += ((double)b1 - (double)m1 * (double)i1) * d1;
        s2 += ((double)b2 - (double)m2 * (double)i2) * d2;
        s3 += ((double)b3 - (double)m3 * (double)i3) * d3;
    }
    for (; n < batch; ++n) {
        const float* t = nt + (size_t)n * ts + k;
        s0 += ((double)t[2 * c] - (double)t[0] * (double)t[c]) * dzsum[(size_t)n * cout + co];
    }
    const float sf = (float)((s0 + s1) + (s2 + s3));
    for (int tap = 0; tap < ntaps; ++tap) dw[((size_t)tap * cin + part_lo + k) * cout + co] += sf;
}

extern "C" int shm_conv2d_wgrad_norm_finish(float* dw, const float* nt, const double* dzsum, int batch, int c, int part_lo, int cin, int cout, int ksize,
                                            void* stream) {
    SHM_REQUIRE(dw && nt && dzsum, SHM_E_SHAPE, "shm_conv2d_wgrad_norm_finish: null pointer");
    SHM_REQUIRE(c > 0 && part_lo >= 0 && part_lo + c <= cin, SHM_E_SHAPE, "shm_conv2d_wgrad_norm_finish: part [%d, %d) outside %d channels", part_lo,
                part_lo + c, cin);
    if (batch == 0 || cout == 0) return SHM_OK;
    hipLaunchKernelGGL(wgrad_norm_finish_kernel, dim3(shm_cdiv(cout, 64), shm_cdiv(c, 4)), dim3(256), 0, (hipStream_t)stream, dw, nt, dzsum, batch, c, part_lo,
                       cin, cout, ksize * ksize);
    SHM_LAUNCH_CHECK("shm_conv2d_wgrad_norm_finish");
    return SHM_OK;
}

extern "C" int shm_conv2d_wgrad_partial(const void* x, const void* x2, int c1, int ldx, int ldx2, const void* dy,
                                        int lddy, int batch, int hi, int wi, int cin, int cin_ld, int cout,
                                        int ksize, int stride, void* workspace, size_t ws_bytes, int dtype,
                                        int* nsplit_out, void* stream) {
    return wgrad_partial_impl(x, x2, c1, ldx, ldx2, dy, lddy, batch, hi, wi, cin, cin_ld, cout, ksize, stride, workspace, ws_bytes, dtype, nsplit_out, stream,
                              ShmNormReq{});
}

extern "C" int shm_conv2d_wgrad_partial_norm(const void* x, const void* x2, int c1, int ldx, int ldx2, const float* nt_x, const float* nt_x2, int norm_mode,
                                             const void* dy, int lddy, int batch, int hi, int wi, int cin, int cin_ld, int cout, int ksize, int stride,
                                             void* workspace, size_t ws_bytes, int dtype, int* nsplit_out, void* stream) {
    ShmNormReq nm;
    if (const int r = shm_norm_request(&nm, "shm_conv2d_wgrad_norm", nt_x, nt_x2, norm_mode, x2, c1, cin_ld)) return r;
    return wgrad_partial_impl(x, x2, c1, ldx, ldx2, dy, lddy, batch, hi, wi, cin, cin_ld, cout, ksize, stride, workspace, ws_bytes, dtype, nsplit_out, stream, nm);
}

// shm_conv2d_wgrad on a source that is the UN-normalised activation of an InstanceNorm block (nt_x / nt_x2: that block's table, at
// most one of the two)
extern "C" int shm_conv2d_wgrad_norm(const void* x, const void* x2, int c1, int ldx, int ldx2, const float* nt_x, const float* nt_x2, int norm_mode,
                                     const void* dy, int lddy, float* dw, int batch, int hi, int wi, int cin, int cin_ld, int cout, int ksize, int stride,
                                     int accumulate, void* workspace, size_t ws_bytes, int dtype, void* stream) {
    ShmNormReq nm;
    if (const int r = shm_norm_request(&nm, "shm_conv2d_wgrad_norm", nt_x, nt_x2, norm_mode, x2, c1, cin_ld)) return r;
    SHM_REQUIRE(dw, SHM_E_SHAPE, "shm_conv2d_wgrad: null pointer");
    int ns = 0;
    const int r = wgrad_partial_impl(x, x2, c1, ldx, ldx2, dy, lddy, batch, hi, wi, cin, cin_ld, cout, ksize, stride, workspace, ws_bytes, dtype, &ns, stream, nm);
    if (r) return r;
    return shm_conv2d_wgrad_reduce(workspace, dw, (size_t)ksize * ksize * cin * cout, ns, accumulate, stream);
}

extern "C" int shm_conv2d_wgrad(const void* x, const void* x2, int c1, int ldx, int ldx2, const void* dy,
                                int lddy, float* dw, int batch, int hi, int wi, int cin, int cin_ld,
                                int cout, int ksize, int stride, int accumulate, void* workspace,
                                size_t ws_bytes, int dtype, void* stream) {
    return shm_conv2d_wgrad_norm(x, x2, c1, ldx, ldx2, nullptr, nullptr, SHM_NORM_EXACT, dy, lddy, dw, batch, hi, wi, cin, cin_ld, cout, ksize, stride, accumulate,
                                 workspace, ws_bytes, dtype, stream);
}
