// Shared pieces of the weight-gradient kernels: block order, the argument blocks, the transposed bf16 fragment read, the slab epilogue, the
// launcher's plan, and the launch function each kernel family's translation unit sits behind (conv_wgrad_gen.hip, conv_wgrad_halo.hip,
// conv_wgrad_halo16.hip, conv_wgrad_halo8.hip, conv_wgrad_x3.hip).  wgrad_halo_dev.h has what only the halo-staged kernels share (patch walk, edge
// bits, stage ring).  conv_wgrad.hip has the entry points, the plan (wgrad_plan) and the launcher: see its header comment.
#pragma once
#include "common.h"
#include "ablate.h"

// XCD-aware block order (speed only): the dispatcher deals consecutive workgroups round-robin over the 8 XCDs, each with its
// own L2, so the blocks that share an operand tile -- same pixels, different (ci, co) tile -- land on eight different L2s and
// every tile is fetched from HBM up to eight times (wgrad_halo_bf16_kernel: L2 hit rate 0.33, 3.3 TB/s HBM-side at 38 % MFMA
// utilisation).  Remapped, XCD j works through the contiguous range [j*total/8, (j+1)*total/8) of the x-fastest block order,
// i.e. through whole pixel splits: both operand tiles of a split are fetched once per XCD and reused from its L2.  Bijective
// for any grid (guide, "XCD swizzle must be bijective").  Whatever the real placement, results are unchanged.
struct Blk3 {
    int x, y, z;
};
__device__ __forceinline__ Blk3 xcd_block_order() {
    const unsigned nx = gridDim.x, ny = gridDim.y, total = nx * ny * gridDim.z;
    const unsigned lin = blockIdx.x + nx * (blockIdx.y + ny * blockIdx.z);
    const unsigned q = total >> 3, r = total & 7u, xcd = lin & 7u, idx = lin >> 3;
    const unsigned nw = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
    Blk3 b;
    b.x = (int)(nw % nx);
    b.y = (int)((nw / nx) % ny);
    b.z = (int)(nw / (nx * ny));
    return b;
}

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

struct WgradArgs {            // x, x2, dy: float (wgrad_kernel) or bf16 (wgrad_bf16_kernel) tensors
    const void* x;
    const void* x2;
    int c1, ldx, ldx2;
    const void* dy;
    int lddy;
    float* part;
    int hi, wi, ho, wo;
    int cin_ld, cin, cout;
    int is, ntaps;
    int dh[9], dw[9];
    int M, pix_per_split;
    unsigned xbytes, x2bytes, dybytes;
};

struct WgradHaloArgs {
    const void* x;
    const void* x2;
    int c1, ldx, ldx2;
    const void* dy;
    int lddy;
    float* part;
    int h, w, cin_ld, cin, cout;
    int npatch, patches_per_split;
    unsigned xbytes, x2bytes, dybytes;
    // "norm" (shm_conv2d_wgrad_norm): source `ntpart` (0 = x, 1 = x2) is the UN-normalised activation a of an InstanceNorm block with
    // table nt = float [batch][4][ntc] (mean, inv, beta, ring).  SHM_NORM_EXACT (kernels <1>): shm_in_norm on its halo pixels in LDS, see
    // tapgemm_halo_kernel.  SHM_NORM_SCALED (kernels <2>): sum x_hat * dz = inv * sum a_ext * dz + (beta - mean * inv) * sum dz with
    // a_ext = a inside the image and `ring` outside -- the kernels write `ring` over the out-of-image halo entries of border patches and
    // scale the rows of their slab by inv (a block's patches lie in ONE sample: the launcher cuts the splits that way); the second
    // term is shm_conv2d_wgrad_norm_finish's.
    const float* nt;
    int ntpart, ntc;
};

typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef short s16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __attribute__((address_space(3))) s16x4* lds_s16x4_ptr;

__device__ __forceinline__ bf16x8 tr_frag(const unsigned short* base) {
    // pixels [0,4) and [4,8) of this lane's k group: two transposed reads 4 rows (512 B) apart
    s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4_ptr)(base));
    s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4_ptr)(base + 4 * 64));
    s16x8 v = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
    return __builtin_bit_cast(bf16x8, v);
}

// A 16-byte global load the COMPILER does not see as a vector-memory operation (inline asm, drained on the spot).  The table
// registers of the NM kernels are re-read when a block moves on to the next image, i.e. under a branch: as plain loads hipcc has
// to assume them outstanding at every later use and puts s_waitcnt vmcnt(0) in front of each normalisation -- which also waits
// for the LDS-DMA of the stage just issued, in the middle of the MFMA stream (measured: +6-10 % on the kernel).
__device__ __forceinline__ f32x4 load16_drained(const float* p) {
    f32x4 v;
    asm volatile("global_load_dwordx4 %0, %1, off\n\ts_waitcnt vmcnt(0)" : "=&v"(v) : "v"(p) : "memory");
    return v;
}

// A wave's 32 x 32 sub-tile (mi, column con) of all NT taps of the partial slab `out` = [tap][cin][cout] of this block's split.  Row r of lane
// half hh of an MFMA accumulator is channel ci0 + 32 mi + (r & 3) + 8 (r >> 2) + 4 hh.  SCALED (SHM_NORM_SCALED): row r times sc[r] on the way
// out (scaling the accumulators in place made hipcc spill 100 registers).
template <int NT, bool SCALED>
__device__ __forceinline__ void wgrad_store_slab(const f32x16 (&acc)[NT], float* out, int cin, int cout, int ci0, int mi, int hh, int con, const float* sc) {
#pragma unroll
    for (int t = 0; t < NT; ++t) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int ci = ci0 + mi * 32 + (r & 3) + 8 * (r >> 2) + 4 * hh;
            if (ci < cin && con < cout) out[((size_t)t * cin + ci) * cout + con] = SCALED ? acc[t][r] * sc[r] : acc[t][r];
        }
    }
}

// SHM_NORM_SCALED: the slab's row scales = inv of the block's sample; iv points at the table entry of the lane's row 0 (channel ci0 + 32 mi + 4 hh
// of its source), rows 4 g .. 4 g + 3 are eight channels on per g
__device__ __forceinline__ void wgrad_row_scale(float (&sc)[16], const float* iv) {
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const f32x4 s4 = *(const f32x4*)(iv + 8 * g);
#pragma unroll
        for (int e = 0; e < 4; ++e) sc[4 * g + e] = s4[e];
    }
}

// What the shape-only sizing of shm_conv2d_wgrad_workspace allows for beside the split-K target (the plan uses the same constants)
constexpr int kWgradThinRows = 96;          // wgrad_halo_thin_kernel: 9 * cin packed MFMA rows at most ...
constexpr int kWgradThinSlabs = 2;          // ... and two slabs per split (one per patch row)
constexpr int kWgradRgbRows = 32;           // conv3x3s2_rgb_wgrad_kernel (conv_rgb.hip): 9 * cin at most ...
constexpr int kWgradRgbSlabs = 1024;        // ... and one slab per block, streaming -- blocks are what it needs
constexpr int kWgradHalo8CoTiles = 2;       // wgrad_halo8_bf16_kernel: a block owns two 64-wide co tiles -- half as many (ci, co) tiles, twice the splits for a given block target

enum {
    SHM_WG_GEN,           // wgrad_kernel / wgrad_bf16_kernel <ntaps, straddle>
    SHM_WG_HALO,          // wgrad_halo_kernel <nmode> or, stride2, <0, true>
    SHM_WG_THIN,          // wgrad_halo_thin_kernel <thin_nrt, thin_is>
    SHM_WG_HALO16,        // wgrad_halo_bf16_kernel <rows, nmode>
    SHM_WG_HALO8,         // wgrad_halo8_bf16_kernel <mode8>
    SHM_WG_X3,            // wgrad_halo_x3_kernel <rows, nmode == 1, stride2>
};

// What conv_wgrad.hip's wgrad_plan decided for one weight gradient.  The launches below read no tuning knob and test no shape beyond their grid.
struct WgradPlan {
    int family;                   // SHM_WG_*
    bool bf16;                    // operand type (SHM_WG_GEN: which of the two kernels)
    int ntaps;                    // ksize * ksize
    bool straddle;                // a 64-channel ci tile holds channels of both concat sources (generic kernels only)
    int rows;                     // pixel rows per stage (SHM_WG_HALO16, SHM_WG_X3: 2 or 4)
    int nmode;                    // 0 = plain source, 1 + SHM_NORM_* = the source is normalised in LDS
    bool stride2;                 // SHM_WG_HALO, SHM_WG_X3: the stride-2 form
    int mode8;                    // SHM_WG_HALO8: MODE
    int thin_nrt, thin_is;        // SHM_WG_THIN: row tiles, conv stride
    bool try_rgb;                 // shm_rgb_s2_wgrad_launch (conv_rgb.hip) is tried first; it has its own eligibility and split
    // the split: patches of prow x pcol pixels of the output map (over_out) or the input map; the generic kernels cut pixels (1 x 1 "patches",
    // patches_per_split = WgradArgs::pix_per_split)
    int prow, pcol;
    bool over_out;
    int npatch, patches_per_split;
    int splits;                   // grid z
    int nsplit;                   // slabs written = what *nsplit_out receives (SHM_WG_THIN: kWgradThinSlabs per split)
    size_t early_bytes;           // the workspace of the uncut split-K target: asked of every call, before the RGB kernel is tried
    size_t ws_bytes;              // workspace the launch needs: max(early_bytes, nsplit slabs)
    bool norm_ok;                 // this shape's kernel can normalise its source in LDS
};

// One kernel family each, launching the form the plan chose on a grid of (cin / 64, cout / 64 or 128, p.splits) blocks
int shm_wgrad_gen_launch(const WgradArgs& a, const WgradPlan& p, hipStream_t st);             // conv_wgrad_gen.hip: SHM_WG_GEN
int shm_wgrad_halo_launch(const WgradHaloArgs& a, const WgradPlan& p, hipStream_t st);        // conv_wgrad_halo.hip: SHM_WG_HALO, SHM_WG_THIN
int shm_wgrad_halo16_launch(const WgradHaloArgs& a, const WgradPlan& p, hipStream_t st);      // conv_wgrad_halo16.hip: SHM_WG_HALO16
int shm_wgrad_halo8_launch(const WgradHaloArgs& a, const WgradPlan& p, hipStream_t st);       // conv_wgrad_halo8.hip: SHM_WG_HALO8

// conv_wgrad_x3.hip ("wgrad.f32_split" = 1): the fp32 3x3 unit-stride weight gradient as six bf16 MFMA products of three-plane splits of x and dY.
// hgs as for wgrad_halo_kernel<0> with patches of p.rows x 16 pixels (2 or 4); grid = (cin / 64, cout / 64, p.splits).
// p.stride2: patches of 2 x 16 OUTPUT pixels of a 3x3 stride-2 layer on an even map (hgs as for wgrad_halo_kernel<0, true>, cut to that patch)
int shm_wgrad_x3_launch(const WgradHaloArgs& hgs, const WgradPlan& p, hipStream_t st);        // SHM_WG_X3
