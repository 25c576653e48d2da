/*
 * libshmgan_hip.so -- C ABI of the MI355X (gfx950) kernels behind SHMGAN's
 * generator + discriminator train_step.
 *
 * The reference (Atif-Anwer/SHMGAN, /root/reference/ShmGANwithSSpecSeg.py = "SHM.py")
 * has no FFI: every op below replaces a TensorFlow/Keras call made from Python.  Each
 * entry point cites the reference call site it stands in for.  See INTEGRATION.md for
 * the ctypes binding a maintainer of the reference would add.
 *
 * Conventions
 *  - tensors are NHWC device pointers (the caller owns every buffer, the library never
 *    allocates device memory and keeps no pointer after return);
 *  - `void*` tensors are ACTIVATION-typed: float32 when the call's `dtype` is SHM_F32, bfloat16
 *    when it is SHM_BF16 (BASELINE configs 4-5: bf16 operands on v_mfma_f32_32x32x16_bf16, fp32
 *    accumulation and fp32 arithmetic inside every kernel).  `float*` / `double*` arguments keep
 *    their type in both modes: master weights, biases, IN beta, statistics, weight gradients,
 *    image-space tensors and losses are always fp32 / f64;
 *  - "ld*" arguments are channel pitches in ELEMENTS, at least the channel count of their tensor (its part of a split
 *    destination, its source of a concat): a tensor may be a channel slice of a wider buffer.  A smaller pitch is refused
 *    with SHM_E_SHAPE before any launch (rows would overlap); a pitch is looked at only when its tensor is given (pass 0
 *    with a NULL x2 / dx2 / g2).  The one exception is the compact 3-channel image below.  MFMA operands are staged as
 *    64-byte rows that travel to LDS in 16-byte pieces, so contraction channel counts and concat splits are multiples of
 *    16 (fp32) or 32 (bf16), and convolution INPUTS (x, x2, the dy of a gradient product; the aux of a gsum call where
 *    the epilogue is to take the sums) have pitches that are multiples of 4 (fp32) or 8 (bf16) on 16-byte-aligned bases --
 *    enforced for x, x2 and dy.  Convolution OUTPUTS take any pitch and any element-aligned base (the statistics pass of
 *    shm_conv2d_in_fwd on small maps and the gsum reduce pass read them four channels at a time and refuse a pitch that is
 *    no multiple of 4): bf16 outputs
 *    whose pitches are multiples of 8 on 16-byte-aligned bases (and whose channel counts are multiples of 8) leave in 16-byte
 *    stores, others element by element -- same values, slower -- and a bf16 layer then leaves the weights-in-registers
 *    kernels, and gsum sums their epilogue for the reduce pass.  The InstanceNorm, pooling and LeakyReLU entry points work
 *    on four channels per thread: channel counts and pitches are multiples of 4 in either type (8-byte-aligned bases in
 *    bf16), and bf16 calls whose pitches are not multiples of 8 or whose bases are not 16-byte aligned take the four-channel
 *    forms (shm_in_bwd: two passes; its one-pass form also wants a 16-byte-aligned dz).  The
 *    3- and 10-channel images are stored in a 16-float / 32-bf16 pitch (zero padded); tests/test_pitch_gpu.py runs every
 *    entry point on such views;
 *  - "f64 scratch" arguments are small double accumulators; where a comment says "zero on entry" the caller
 *    zeroes them ONCE (at allocation) and every call leaves them zero again -- also when it returns an error
 *    (the entry point clears the scratch itself if a launch after the one that filled it fails); otherwise
 *    the call zeroes them;
 *  - every call is asynchronous on `stream` (a hipStream_t passed as void*);
 *  - return value: SHM_OK or a negative error; shm_last_error() gives the text.
 */
#ifndef SHMGAN_HIP_H
#define SHMGAN_HIP_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SHM_OK 0
#define SHM_E_SHAPE (-1)
#define SHM_E_DTYPE (-2)
#define SHM_E_WORKSPACE (-3)
#define SHM_E_HIP (-4)

#define SHM_F32 0
#define SHM_BF16 1
/* bf16 activations and MFMA operands, but fp32 for the tensors marked [G] below: the gradient
 * signal on its way from an input-gradient product into the next InstanceNorm/LeakyReLU backward.
 * An option for callers that want that signal unrounded; measured on the whole step it changes no
 * per-tensor gradient cosine beyond the 4th digit and costs 1.7 % (DESIGN.md, bf16 path), so the
 * host side defaults to plain SHM_BF16.  Accepted by the functions that have a [G] argument. */
#define SHM_BF16_GF32 2

int shm_version(void);
const char* shm_last_error(void);
/* Symbol (as rocprofv3 prints it, without the "void " prefix and the argument list) of the MFMA kernel
 * the calling thread's last convolution entry point dispatched to: the tile/variant choice depends on
 * shape and dtype, and bench.py's per-kernel roofline keys its HIP-event timings by it. */
const char* shm_last_kernel(void);

/* ---- dispatch tuning ---------------------------------------------------------------
 * The convolution entry points choose among several MFMA kernel variants by shape and dtype.  These
 * process-wide integer knobs override that choice (parity tests force every variant; tools sweep them):
 *   "tapgemm.variant"           0 automatic (default), or one of SHM_TG_*: a forced variant the shape is not
 *                               eligible for makes the conv call return SHM_E_SHAPE (it never falls back silently)
 *   "tapgemm.halo_min_blocks"   fp32: from this many 128-channel halo blocks on the 128-wide halo block is taken without comparing
 *                               the fill of its last round with the 64-wide block's (default 1024)
 *   "tapgemm.small_grid_blocks" grids with fewer 128x128 tiles take the 64x128 tile (default 1024)
 *   "tapgemm.phase4_min_blocks" stride-2 transposed 3x3 products with at least this many fused (16x16 input pixels x 64 channels) blocks
 *                               take the four-phases-in-one-block kernel (default 256)
 *   "tapgemm.wreg16"            bf16 weights-in-registers layers (one source, 32 / 64 input channels): 2 (default) = the one-block-per-CU ping-pong
 *                               kernel (tapgemm_pp_bf16_kernel, v_mfma_f32_32x32x16_bf16) where the shape allows (64 input channels, map of whole
 *                               8 x 32-pixel patches) and the eight-wave form elsewhere, 1 = the eight-wave form with 16-column wave tiles
 *                               (tapgemm_wreg16_bf16_kernel, v_mfma_f32_16x16x32_bf16, four waves per SIMD), 0 = four-wave form with 32-column tiles
 *   "tapgemm.flat_epilogue"     1 = treat every output as larger than 4 GiB: element stores through 64-bit addresses, no buffer-store kernels (tests), default 0
 *   "wgrad.variant"             0 automatic, 1 generic kernels only, 2 halo kernels without thin-input packing, 3 no stride-2 halo form
 *   "wgrad.blocks"              split-K block target, 0 automatic (1024 fp32 / 256 bf16)
 *   "wgrad.bf16_rows"           bf16 halo weight gradient: pixel rows per LDS stage, 0 automatic (4 when the map height allows), 2, 4
 *   "wgrad.f32_split"           fp32 3x3 unit-stride weight gradient (the halo kernel's shapes, plain and SHM_NORM_EXACT sources): 1 = six v_mfma_f32_32x32x16_bf16
 *                               products of the exact three-plane bf16 splits of x and dY with fp32 accumulation (wgrad_halo_x3_kernel; rel-L2 ~2.5e-7
 *                               on random-sign operands; NOT a bit-faithful fp32 dot product -- see "conv.f32_split" below), 0 (default) = exact-fp32 MFMA.
 *                               Opt-in: bench.py --dtype f32x3
 *   "conv.f32_split"            fp32 3x3 unit-stride forward / input gradient: 1 = six bf16 MFMA products of exact three-plane splits where
 *                               the shape fits (tapgemm_halo_x3_kernel), 0 (default) = exact-fp32 MFMA.  Opt-in
 *   "elem.fused_bwd"            bf16 shm_in_bwd: 1 (default) = the one-pass form where fused_scratch was given and the shape fits, 0 = two passes
 *   "wgrad.bf16_wide"           bf16 weight gradient, the eight-wave 64 ci x 128 co block (cout >= 128): 0 automatic (= 2), 1 never, 2 at stride 2 only,
 *                               3 at unit stride only, 4 both
 *   "stats.fusion"              1 InstanceNorm statistics in the conv epilogue (default), 0 separate pass
 *   "elem.fused_max_slices"     the one-pass form: most slices (= blocks that must be resident together) per barrier group, default 256, at most 512; the launcher also
 *                               requires twice the group's blocks to fit the device (the one-pass form of shm_in_bwd below)
 *   "elem.fused_hold"           the one-pass form's kernel: 0 automatic (in_bwd_fusedg_kernel -- the gradient held in registers, the activation streamed
 *                               twice, slices of 32768 / min(c, 64) pixels, up to 2 x "elem.fused_max_slices" blocks per group -- on maps of at least
 *                               256 x 16384 / min(c, 64) pixels without a pooled gradient, where it is measured faster; in_bwd_fused8_kernel otherwise),
 *                               1 in_bwd_fused8_kernel only, 2 in_bwd_fusedg_kernel wherever the map has whole slices
 *   "elem.fused_gvariant"       in_bwd_fusedg_kernel's register-budget form: 0 <2, 2, 4> (four blocks per CU; default), 1 <8, 8, 3>
 *   "elem.fused_test_stall"     tests only: 1 = the one-pass form's barriers wait for one block more than the grid has, i.e. every barrier
 *                               times out (this form gives up after 2^10 polls, ~1 ms per resident generation of blocks, where a real launch waits
 *                               ~1 s) and the abort words given to the call are set; default 0
 *   "elem.reverse"              1 InstanceNorm apply / backward-reduce passes walk the tensor back to front (default: the tail the
 *                               producer just wrote is still in the Infinity Cache), 0 front to back
 *   "elem.reduce_blocks"        block target of the InstanceNorm-backward reduce pass, 0 automatic (1024 fp32 / 512 bf16: every block ends
 *                               in f64 atomics on its sample's 2c sums)
 *   "elem.nt_loads"             1 the InstanceNorm-backward apply pass reads its gradient tensor (dead after that read) with non-temporal
 *                               loads, 0 plain loads (default; round-3 A/B in DESIGN.md section 8)
 *   "elem.chunk_mb"             shm_in_bwd runs its reduce and apply passes per chunk of samples whose tensors fit this many MiB, so that
 *                               the apply pass re-reads them from the Infinity Cache; 0 = the whole batch at once (default)
 *   "elem.interleave"           bf16 activations: 1 (default) the InstanceNorm-backward passes deal a sample's pixel tiles round-robin over its
 *                               blocks, 0 one contiguous chunk per block (bf16 step 26.2 -> 26.0 ms; float32 always takes the chunk form)
 *   "elem.stream_blocks"        block target of the passes without a per-block prologue or reduction (InstanceNorm apply and its pooling
 *                               forms), default 32768: short blocks keep the addresses in flight a narrow band of the tensors
 *   "elem.apply_blocks"         block target of the InstanceNorm-backward apply pass, default 4096 (every block ends in an LDS reduction and
 *                               one f64 atomic per channel for the bias gradient: 5.2 TB/s at 4-8k blocks, 4.3 at 32k; without a bias
 *                               gradient the pass keeps gaining up to 32k: tools/probes/bwd_blocks.py)
 * value < 0 restores the knob's default; key "reset" restores all.  Initial values may be given in the
 * environment (SHM_TAPGEMM_VARIANT, SHM_TAPGEMM_HALO_MIN, SHM_TAPGEMM_SMALLM, SHM_TAPGEMM_PHASE4_MIN, SHM_WGRAD_VARIANT, SHM_WGRAD_BF16_ROWS,
 * SHM_WGRAD_BLOCKS, SHM_STATS_FUSION, SHM_ELEM_REVERSE, SHM_ELEM_REDUCE_BLOCKS, SHM_ELEM_NT, SHM_ELEM_CHUNK_MB, SHM_ELEM_INTERLEAVE, SHM_ELEM_STREAM_BLOCKS, SHM_ELEM_APPLY_BLOCKS), read once.  Knobs change scheduling only, never results beyond the
 * summation order of a tile shape. */
#define SHM_TG_AUTO 0
#define SHM_TG_HALO128 1
#define SHM_TG_HALO64 2
#define SHM_TG_DMA_128x128 3
#define SHM_TG_DMA_64x128 4
#define SHM_TG_DMA_128x64 5
#define SHM_TG_DMA_256x64 6
#define SHM_TG_DMA_256x128 7
#define SHM_TG_HALO128_PH8 8
#define SHM_TG_DMA_128x128_BK32 9
#define SHM_TG_DMA_128x128_NST4 10
#define SHM_TG_HALO128_ST 12            /* halo kernels with the nine taps unrolled: static fragment addresses, conflict-free swizzle */
#define SHM_TG_HALO64_ST 13
#define SHM_TG_PHASE4 14               /* 3x3 stride-2 transposed products (Conv2DTranspose forward, stride-2 input gradient): four phases fused in one block */
#define SHM_TG_DMA_64x64 15             /* DMA tap GEMM, 64 x 64 tile (four waves of 32 x 32): grids too small to fill the chip with larger tiles */
#define SHM_TG_HALO128_ST_W4 16         /* static-tap halo block of four waves, wave tile 128 pixels x 64 channels */
#define SHM_TG_WREG 11                 /* bf16, 3x3 s1, <= 64 input channels: weights in registers, persistent blocks */
#define SHM_TG_COUNT 17                /* the variants are 0 .. SHM_TG_COUNT - 1 */
int shm_set_tuning(const char* key, int value);
int shm_get_tuning(const char* key, int* value);

/* ---- weight layout ---------------------------------------------------------------
 * [ntaps][rows][cols] -> [ntaps][cols][rows_pad] (zero padded): HWIO -> K-contiguous
 * [tap][Cout][Cin] for the implicit-GEMM B operand. */
int shm_transpose_taps(const float* w, void* wt, int ntaps, int rows, int cols, int rows_pad,
                       int dtype, void* stream);
/* `count` (<= 48) such transposes in one launch: the host arrays hold one entry per layer (weights of a whole model after an
 * optimizer step). */
int shm_transpose_taps_multi(int count, const void* const* w, void* const* wt, const int* ntaps, const int* rows,
                             const int* cols, const int* rows_pad, int dtype, void* stream);
/* dst[i] = (dtype) src[i]: operand copies of weights that are already K-contiguous as stored. */
int shm_cast_f32(const float* src, void* dst, size_t n, int dtype, void* stream);

/* ---- convolutions (implicit GEMM on v_mfma_f32_32x32x2_f32 / v_mfma_f32_32x32x16_bf16) ------
 * Keras Conv2D(k in {1,3}, strides in {1,2}, padding='same') + bias + LeakyReLU(slope)
 * (SHM.py:244-245, 254-326, 365-369, 387).  y is [G]-typed under SHM_BF16_GF32 (the call is then the
 * input-gradient of a Conv2DTranspose).  Input = channel concat of x (c1 channels,
 * pitch ldx) and optional x2 (cin-c1 channels, pitch ldx2): Concatenate() SHM.py:299,306,
 * 313,320 is never materialised.  wk = [k*k][cout][cin] (shm_transpose_taps of HWIO, in the call's dtype),
 * cin and c1 multiples of 16 (fp32) / 32 (bf16).  bias may be NULL; slope 1.0f = no activation, 0.0f = ReLU.
 * hi and wi are independent (any rectangle; tests/test_rect_gpu.py), and the stride-2 forward and weight gradient take odd sizes with TF SAME
 * padding (pad_before = 1 on an odd axis, 0 on an even one); shm_conv2d_dgrad at stride 2 needs even sizes.
 * Compact 3-channel images (the discriminator's input, SHM.py:353): x may hold ONE 16-byte chunk per pixel -- ldx = 4 (fp32: r, g, b, 0) or 8
 * (bf16: r, g, b, five zeros) -- under a weight copy of cin = 16 / 32 whose channels >= 3 are zero; k = 3, stride 2 and an output width that is a
 * multiple of 16 then run the streaming kernels of conv_rgb.hip (forward and shm_conv2d_wgrad alike), other shapes the generic ones. */
int shm_conv2d_fwd(const void* x, const void* x2, int c1, int ldx, int ldx2, const void* wk,
                   const float* bias, void* y, int ldy, int batch, int hi, int wi, int cin,
                   int cout, int ksize, int stride, float slope, int dtype, void* stream);

/* The same convolution fused with the InstanceNormalization statistics of its output
 * (Conv2D -> LeakyReLU -> InstanceNormalization, SHM.py:244-245): the epilogue accumulates
 * sum / sum of squares per (sample, channel); on return (stream order) stats holds
 * (mean, rsqrt(var + eps)) exactly as shm_in_stats would leave it.  stats = f64 [batch*cout*2];
 * scratch = f64 [SHM_STATS_SLOTS*batch*cout*2] or NULL: slot copies of the running sums, so that the
 * hw/64 atomic adds per (sample, channel) do not queue on one address.  The scratch must be ZERO on entry
 * (zero it once when allocating) and is zero again on return: no memset per call. */
#define SHM_STATS_SLOTS 16
int shm_conv2d_in_fwd(const void* x, const void* x2, int c1, int ldx, int ldx2, const void* wk,
                      const float* bias, void* y, int ldy, int batch, int hi, int wi, int cin,
                      int cout, int ksize, int stride, float slope, double* stats, double* scratch,
                      float eps, int dtype, void* stream);

/* Input-gradient of the same conv.  dy [batch,ho,wo,cout] (pitch lddy), w = HWIO
 * [k*k][cin][cout] as stored (it is already K-contiguous for this product; in bf16 mode the shm_cast_f32 copy),
 * cout a multiple of 16 (fp32) / 32 (bf16).
 * dx channels [0,n1) go to dx (pitch lddx), [n1,cin) to dx2 (pitch lddx2): the split of a
 * concat gradient.  Pass dx2=NULL, n1=cin for a single destination.  dx, dx2 are [G] tensors. */
int shm_conv2d_dgrad(const void* dy, int lddy, const void* w, void* dx, void* dx2, int n1,
                     int lddx, int lddx2, int batch, int hi, int wi, int cin, int cout,
                     int ksize, int stride, int dtype, void* stream);

/* Keras Conv2DTranspose(k=3, strides=2, 'same') + bias + LeakyReLU (SHM.py:298,305,312,319).
 * x [batch,hi,wi,cin]; w = Keras layout [3][3][cout][cin] as stored; y [batch,2hi,2wi,cout]. */
int shm_conv2d_transpose_fwd(const void* x, int ldx, const void* w, const float* bias, void* y,
                             int ldy, int batch, int hi, int wi, int cin, int cout, float slope,
                             int dtype, void* stream);

/* Weight gradient: dw[t][ci][co] (+)= sum_pixels x[pix*stride + tap][ci] * dy[pix][co]
 * (HWIO).  For Conv2DTranspose pass x = dz of the transposed conv (2H res), dy = its input
 * (H res), stride 2: the result is the Keras [3][3][cout][cin] layout.  cin_ld = number of
 * input channels to read (multiple of 4 fp32 / 8 bf16, pad channels must be zero), cin = rows stored; dw is
 * always fp32.  workspace: split-K partial slabs (fp32), at least shm_conv2d_wgrad_workspace() bytes; the
 * slabs are summed in a fixed order (deterministic, no float atomics). */
size_t shm_conv2d_wgrad_workspace(int batch, int ho, int wo, int cin, int cout, int ksize);
/* The two phases of shm_conv2d_wgrad as separate calls (bench.py times the MFMA kernel on its own):
 * _partial writes *nsplit_out slabs [ksize*ksize][cin][cout] to workspace; _reduce sums them into dw. */
int shm_conv2d_wgrad_partial(const void* x, const void* x2, int c1, int ldx, int ldx2, const void* dy,
                             int lddy, int batch, int hi, int wi, int cin, int cin_ld, int cout,
                             int ksize, int stride, void* workspace, size_t ws_bytes, int dtype,
                             int* nsplit_out, void* stream);
int shm_conv2d_wgrad_reduce(const void* workspace, float* dw, size_t n, int nsplit, int accumulate,
                            void* stream);
int shm_conv2d_wgrad(const void* x, const void* x2, int c1, int ldx, int ldx2, const void* dy,
                     int lddy, float* dw, int batch, int hi, int wi, int cin, int cin_ld,
                     int cout, int ksize, int stride, int accumulate, void* workspace,
                     size_t ws_bytes, int dtype, void* stream);

/* ---- The fused block: InstanceNormalization applied by the CONSUMER (SHM.py:244-245 "Conv -> LeakyReLU -> IN", north-star
 * "IN apply folded into the consumer's load") ------------------------------------------------------------------------
 * A Conv -> LeakyReLU -> InstanceNorm block stores its un-normalised activation a and its statistics; instead of a pass that reads a
 * and writes the normalised tensor (shm_in_apply: 2x the activation's bytes), the convolution and the weight gradient that consume
 * the block's output read a itself and apply (a - mean) * inv + beta to their operand tile in LDS -- the kernels that stage the A
 * operand as a halo image (unit-stride 3x3 layers on maps that are multiples of 16; *_norm_supported says whether a shape runs on
 * one).  Out-of-image taps stay zero (zero padding of the NORMALISED tensor) and the arithmetic is shm_in_apply's, so results
 * are bit-identical to shm_in_apply followed by the plain entry point.
 *   nt = float [batch][4][c]: per sample the planes mean[c], inv[c], beta[c], ring[c] = mean - beta / inv (the raw value whose
 *   normalised image is 0) of the producing block (c = its channel count = the channel count of the source it describes), written
 *   by shm_conv2d_in_fwd_norm(nt_out, beta_out) or shm_in_norm_table.
 *   norm_mode SHM_NORM_EXACT / SHM_NORM_SCALED (below); with SHM_NORM_SCALED `wk` and `bias` are shm_conv2d_norm_prepare's wk_n, bias_n.
 *   nt_x / nt_x2: table of source x / x2, or NULL = that source is used as stored; at most one of the two. */
#define SHM_NORM_EXACT 0       /* the kernel applies (a - mean) * inv + beta to its operand tile in LDS: bit-identical to shm_in_apply + plain call */
#define SHM_NORM_SCALED 1      /* the normalisation is in the operands: per-sample weights w * inv and bias rows (shm_conv2d_norm_prepare);
                                  the kernels only write `ring` over out-of-image taps.  Same result to rounding, no per-element work in
                                  the MFMA kernels */
int shm_in_norm_table(const double* stats, const float* beta, float* nt, int batch, int c, void* stream);
/* SHM_NORM_SCALED operands: wk_n [batch][taps][cout][cin] (activation dtype) = wk with the channels [part_lo, part_lo + c) of the
 * folded source scaled by that sample's inv, bias_n [batch][cout] = bias + sum wk * (beta - mean * inv) over those channels.  nt is the
 * folded source's table, c its channel count. */
int shm_conv2d_norm_prepare(const void* wk, const float* bias, const float* nt, int c, int part_lo, void* wk_n, float* bias_n,
                            int batch, int cin, int cout, int ksize, int dtype, void* stream);
/* shm_conv2d_in_fwd with (a) sources normalised on the fly and (b) optionally this block's own table as a by-product of the
 * statistics finalisation (nt_out [batch][4][cout] with beta_out [cout]; NULL = not wanted).  With nt_x == nt_x2 == NULL it is
 * shm_conv2d_in_fwd.  SHM_E_SHAPE if the kernel chosen for the shape cannot normalise in LDS (never a silent fallback). */
int shm_conv2d_in_fwd_norm(const void* x, const void* x2, int c1, int ldx, int ldx2, const float* nt_x, const float* nt_x2,
                           int norm_mode, const void* wk, const float* bias, void* y, int ldy, int batch, int hi, int wi, int cin,
                           int cout, int ksize, int stride, float slope, double* stats, double* scratch, float eps, float* nt_out,
                           const float* beta_out, int dtype, void* stream);
/* 1 if shm_conv2d_in_fwd_norm would take a normalised source `norm_part` (0 = x, 1 = x2; c1 = channels of x when there are two
 * sources, else 0) for this shape, batch and the current tuning knobs; 0 otherwise.  Launches nothing. */
int shm_conv2d_norm_supported(int batch, int hi, int wi, int cin, int c1, int cout, int ksize, int stride, int norm_part, int dtype);
/* shm_conv2d_wgrad on sources normalised on the fly, and its query.  SHM_NORM_SCALED: the kernels compute
 * inv * sum a_ext * dz (a_ext = a inside the image, `ring` outside) per sample -- the workspace must then hold
 * shm_conv2d_wgrad_norm_workspace() bytes (splits on sample boundaries) -- and the caller completes the gradient with
 * shm_conv2d_wgrad_norm_finish: dw[tap][part_lo + k][co] += sum_n (beta[k] - mean_n[k] * inv_n[k]) * dzsum[n][co], dzsum = float64
 * [batch][cout] per-sample channel sums of dz = the `dz_sums` output of shm_in_bwd / shm_in_bwd_apply / shm_in_bwd_rank1. */
int shm_conv2d_wgrad_norm(const void* x, const void* x2, int c1, int ldx, int ldx2, const float* nt_x, const float* nt_x2,
                          int norm_mode, const void* dy, int lddy, float* dw, int batch, int hi, int wi, int cin, int cin_ld, int cout,
                          int ksize, int stride, int accumulate, void* workspace, size_t ws_bytes, int dtype, void* stream);
int shm_conv2d_wgrad_partial_norm(const void* x, const void* x2, int c1, int ldx, int ldx2, const float* nt_x, const float* nt_x2,
                                  int norm_mode, const void* dy, int lddy, int batch, int hi, int wi, int cin, int cin_ld, int cout,
                                  int ksize, int stride, void* workspace, size_t ws_bytes, int dtype, int* nsplit_out, void* stream);
int shm_conv2d_wgrad_norm_supported(int batch, int hi, int wi, int cin, int cin_ld, int c1, int cout, int ksize, int stride,
                                    int norm_part, int dtype);
size_t shm_conv2d_wgrad_norm_workspace(int batch, int hi, int wi, int cin, int cout, int ksize, int dtype);
int shm_conv2d_wgrad_norm_finish(float* dw, const float* nt, const double* dzsum, int batch, int c, int part_lo, int cin, int cout,
                                 int ksize, void* stream);
/* One-pass bf16 form of shm_in_bwd (round 5, in_bwd_fused8_kernel: a block keeps its slice of g1 / g2 / a in registers between the reduce and
 * the apply phase, the blocks of a sample meet at a per-sample barrier; 3 tensor passes over HBM instead of 5).  shm_in_bwd may take it when
 * it is given `fused_scratch` = f64 [fused_doubles], fused_doubles >= SHM_IN_BWD_FUSED_DOUBLES(batch, h * w, c), zero on entry and zero again on
 * return (outside the per-block partial rows at its front, which every launch rewrites in full and which may hold anything).
 * Taken for dtype SHM_BF16, c in {8, 16, 32} or a multiple of 64 up to 1024, h * w a multiple of the
 * 16384 / min(c, 64) pixel slice and at most 256 slices per map ("elem.fused_max_slices"; with a pooled gradient g2: c a multiple of 64 and
 * whole tiles of (256 / Wt) rows x Wt = min(w, 128) columns), tuning
 * "elem.fused_bwd" = 1 (default); every other call runs the two passes.  No float atomics: the sums are added in block order (bitwise
 * reproducible). */
#define SHM_IN_BWD_FUSED_CB(c) ((c) < 64 ? (c) : 64)
#define SHM_IN_BWD_FUSED_DOUBLES(batch, hw, c)                                                                                      \
    (((size_t)(batch) * ((size_t)(hw) * SHM_IN_BWD_FUSED_CB(c) / 16384) * 3 * (size_t)(c) + 1) / 2 + (size_t)(batch) * (size_t)(c) + \
     (size_t)(batch) * ((size_t)(c) / SHM_IN_BWD_FUSED_CB(c)) * 288 + 1)
/* The one-pass form's barrier needs every block of a group resident at once.  The launcher takes it only when TWICE the group's blocks fit the
 * current device (its CU count x hipOccupancyMaxActiveBlocksPerMultiprocessor of the kernel, queried once: a partitioned or smaller part falls
 * back to the two passes), and a barrier that still waits ~1 s gives up instead of hanging: the launch then completes with wrong means, sets the
 * last u32 of `fused_scratch` and the ABORT WORDS the call was given, shm_in_bwd's two arguments behind the scratch:
 *   abort_dev   u32 in device memory, OR-ed to non-zero.  shm_adam_clip, given the same word as its `abort_word`, reads it ON THE DEVICE and
 *               applies nothing while it is set: gradients built on unfinished sums never reach the weights, however far the host has run
 *               ahead of the stream;
 *   abort_host  u32 in mapped (pinned) host memory, set to 1: the host sees it without synchronising.
 * Both stay set until the caller clears them.  Either may be NULL: a timeout is then recorded in the words that were given, with NULL / NULL
 * in the scratch's own last word only.  The library keeps neither pointer beyond the launch it is passed to: the caller owns the pair, and
 * its lifetime has to cover the launches that were given it (one pair per trainer, whichever thread steps it). */
/* Measurement hook (bench.py, north_star_block.ceiling): while dev2 (two u64 in device memory) is set on the calling thread, one wave of the
 * middle block of every tapgemm_pp_bf16_kernel launch writes dev2[0] = shader-clock ticks (s_memtime) and dev2[1] = 100 MHz ticks (s_memrealtime)
 * of its patch loop: the clock the kernel actually held = dev2[0] / dev2[1] x 0.1 GHz.  NULL disarms (default). */
int shm_set_clock_probe(unsigned long long* dev2);

/* Opt-in fp32 arithmetic from bf16 MFMAs for the 3x3 unit-stride forward / input-gradient layers: tuning "conv.f32_split" = 1 (round 5,
 * csrc/conv_fwd_x3.hip; the weight gradient's twin is "wgrad.f32_split").  Every fp32 operand is split EXACTLY into three bf16 planes and the six
 * plane products with i + j <= 2 accumulate in fp32: rel-L2 ~4e-7 against float64 on random-sign operands, the exact-fp32 MFMA's own figure.
 * Accuracy limits (round 6, tests/test_x3_gpu.py): the bf16 MFMA truncates what falls below its alignment window when it adds its products to the
 * accumulator, ~0.3-0.5 ulp per accumulation step and always towards zero -- on operands of ONE sign the error is a one-sided shrink that grows with
 * the accumulation chain: -5.3e-6 relative on the step's longest weight-gradient reduction (K = 2.6 M, ~320 steps per split-K slab; exact-fp32 MFMA:
 * 2.4e-7) and -1.1e-5 on the deepest forward product (K = 4608), i.e. outside the 1e-5 single-op bound there; operands below 2^-110 lose the third
 * plane (7e-5 at 2^-120).  The step's own operands (random-sign weights and gradients, O(1) activations) stay at the exact kernels' figures.  shm_conv2d_fwd / shm_conv2d_in_fwd(_norm, SHM_NORM_EXACT) / shm_conv2d_dgrad and their _gsum forms then run
 * tapgemm_halo_x3_kernel where the launcher would have taken a static-tap halo or weights-in-registers kernel: fp32 tensors, K % 32 == 0, outputs
 * below 4 GiB, more than 64 output channels or a map height that is a multiple of 32.  Nothing else changes: no extra arguments, no workspace. */
/* pooled = AveragePooling2D(2)(InstanceNorm apply(a)) WITHOUT writing the normalised tensor: the encoder level's skip consumers
 * normalise a on the fly, only the pool's consumer needs a tensor.  Same bits as shm_in_apply_pool's `pooled`. */
int shm_in_pool(const void* a, int lda, const double* stats, const float* beta, void* pooled, int ldp, int batch, int h, int w,
                int c, int dtype, void* stream);

/* ---- InstanceNormalization (tfa, axis=-1, eps, gamma==1, constant beta) -----------
 * SHM.py:245...:388; op chain Generator_summary.txt:9-36.
 * stats = f64 [batch*c*2]; on return (stream order) stats[(n*c+ch)*2] = mean over H*W,
 * stats[(n*c+ch)*2+1] = rsqrt(biased variance + eps). */
int shm_in_stats(const void* a, int lda, double* stats, int batch, int hw, int c, float eps,
                 int dtype, void* stream);
/* out = (a - mean) * inv + beta[c]  (out may alias a). */
int shm_in_apply(const void* a, int lda, const double* stats, const float* beta, void* out,
                 int ldo, int batch, int hw, int c, int dtype, void* stream);
/* out = InstanceNorm apply as above AND pooled = AveragePooling2D(2)(out) in the same pass (the second block of an
 * encoder level feeds both the skip connection and the pool, SHM.py:246-247): bit-identical to shm_in_apply followed by
 * shm_avgpool2_fwd, without the pooling pass's read of the normalised tensor.  h, w even; pooled [batch, h/2, w/2, c], pitch ldp. */
int shm_in_apply_pool(const void* a, int lda, const double* stats, const float* beta, void* out, int ldo,
                      void* pooled, int ldp, int batch, int h, int w, int c, int dtype, void* stream);
/* Backward of LeakyReLU -> IN given the gradient at the IN output:
 *   d_out = g1 + 0.25 * g2[h/2][w/2]   (g2 = gradient of AveragePooling2D(2,2), may be NULL)
 *   dz = lrelu'(a) * inv * (d_out - mean(d_out) - xhat * mean(d_out * xhat))
 * red = f64 scratch [batch*c*3], ZERO on entry and zero again on return; dbias = f64 accumulator [c]
 * (NOT zeroed, may be NULL).  dz_sums (may be NULL; needs dbias) = f64 [batch][c], receives the per-sample channel sums of dz
 * staged on the way to dbias.  fused_scratch / fused_doubles (may be NULL / 0 = two passes): scratch of the one-pass bf16 form, above;
 * abort_dev / abort_host (may be NULL): the abort words of that form, ignored by the two passes.
 * g1, g2 are [G] tensors; a and dz are activation-typed. */
int shm_in_bwd(const void* g1, int ldg1, const void* g2, int ldg2, const void* a, int lda,
               const double* stats, double* red, void* dz, int lddz, double* dbias, double* dz_sums,
               double* fused_scratch, size_t fused_doubles, unsigned* abort_dev, unsigned* abort_host, int batch, int h, int w, int c,
               float slope, int dtype, void* stream);

/* ---- the fused block's backward: InstanceNorm sums in the producing epilogue ("gsum") -------------------------------------
 * The IN backward needs, per (sample, channel), sum(d_out) and sum(d_out * xhat) before it can write dz: shm_in_bwd collects
 * them in a reduce pass of its own over d_out and the stored activation a.  But d_out is itself the OUTPUT of an input-gradient
 * product -- the dgrad of the next layer (SHM.py:244-245 block order), or the stride-2 product that is Conv2DTranspose's input
 * gradient -- so that product's epilogue, which holds d_out in registers, adds the sums itself:
 *
 *   shm_conv2d_dgrad_gsum = shm_conv2d_dgrad + for each output part (dx: channels [0,n1), dx2: the rest) an optional pair
 *       (aux, red): red[(slot, n, ch)][0] += sum_pixels g, red[...][1] += sum_pixels g * aux, g = the value as stored.
 *       aux = activation-typed tensor [batch, hi, wi] (pitch ldaux) aligned with the part: the consumer block's stored
 *       activation a (so that sum g*xhat = inv * (sum g*a - mean * sum g)), or -- when dx is the gradient of an
 *       AveragePooling2D output -- the pooled NORMALISED tensor, i.e. this layer's own input (sum g*avgpool(xhat) =
 *       sum g*pooled - beta * sum g).
 *   shm_conv2d_fwd_gsum = shm_conv2d_fwd + the same for its single output (the stride-2 forward form is the input gradient
 *       of Conv2DTranspose).
 *   red = f64 [SHM_GSUM_SLOTS][batch][channels of the part][2], ZERO on entry; the slot copies cut the per-address atomic
 *       chains.  Whether the sums were taken in the epilogue or by a follow-up reduce pass (kernels without a gsum epilogue:
 *       the fused four-phase kernel, odd alignments, tiny maps, an output or an aux of 0xfffffff0 bytes or more) is the library's
 *       business: red is complete on return.  aux may be of any size: unlike the operands it is not bound by the 4 GiB limit.
 *   shm_in_bwd_apply = shm_in_bwd without its reduce pass: d_out = g1 + 0.25 * unpool(g2); red = sums of g1 against a,
 *       redp = sums of g2 against the pooled normalised tensor (NULL iff g2 is NULL; needs beta [c]); dstage = f64 [batch*c]
 *       staging of the bias gradient (required with dbias).  red / redp / dstage are zero again on return.  dz_sums as for shm_in_bwd. */
#define SHM_GSUM_SLOTS 8
int shm_conv2d_dgrad_gsum(const void* dy, int lddy, const void* w, void* dx, void* dx2, int n1, int lddx, int lddx2, int batch,
                          int hi, int wi, int cin, int cout, int ksize, int stride, const void* aux, int ldaux, double* red,
                          const void* aux2, int ldaux2, double* red2, int dtype, void* stream);
int shm_conv2d_fwd_gsum(const void* x, const void* x2, int c1, int ldx, int ldx2, const void* wk, const float* bias, void* y,
                        int ldy, int batch, int hi, int wi, int cin, int cout, int ksize, int stride, float slope,
                        const void* aux, int ldaux, double* red, int dtype, void* stream);
int shm_in_bwd_apply(const void* g1, int ldg1, const void* g2, int ldg2, const void* a, int lda, const double* stats,
                     const float* beta, double* red, double* redp, double* dstage, void* dz, int lddz, double* dbias,
                     double* dz_sums, int batch, int h, int w, int c, float slope, int dtype, void* stream);

/* Input gradient of a FIRST layer when only its sum over a set of input channels is needed (the step never
 * uses more: d genY sums the cyclic inputs' view channels, SHM.py:576-580; yuv_to_rgb's backward sums r,g,b).
 * Conv is linear, so the weights are summed first and the 64 -> 10 / 3 channel dgrad becomes a 64 -> 1 stencil:
 *   shm_sum_input_channels: weff[t][co] = sum_{j : mask bit j} w[t][j][co]   (w = HWIO [9][cin][cout], cin <= 32)
 *   shm_conv3x3_dgrad_sum1: out[b,y,x] (+)= sum_k sum_taps sum_co dz[k*batch+b, oy, ox, co] * weff[k][tap][co]
 * dz [nk*batch, ho, wo, c] activation-typed (the layer's pre-activation gradient), weff f32 [nk][9][c],
 * out f32 [batch, hi, wi]; stride 1 or 2 with TF SAME padding. */
int shm_sum_input_channels(const float* w, int cin, int cout, unsigned mask, float* weff, void* stream);
int shm_conv3x3_dgrad_sum1(const void* dz, int lddz, const float* weff, float* out, int nk, int batch,
                           int hi, int wi, int c, int stride, int accumulate, int dtype, void* stream);

/* LeakyReLU backward for blocks without IN (Conv2DTranspose, SHM.py:298): dz = dy*lrelu'(y); dy is [G].
 * dbias = f64 accumulator [c] (NOT zeroed, may be NULL); red = f64 scratch [SHM_LRELU_RED_SLOTS*c], zero on
 * entry and on return (needed when dbias is given: the per-channel sums are staged over slots, not on c
 * addresses). */
#define SHM_LRELU_RED_SLOTS 64
int shm_lrelu_bwd(const void* dy, int lddy, const void* y, int ldy, void* dz, int lddz,
                  double* dbias, double* red, size_t npix, int c, float slope, int dtype, void* stream);

/* AveragePooling2D(2,2,'same') on even sizes (SHM.py:249,258,267,276). */
int shm_avgpool2_fwd(const void* x, int ldx, void* y, int ldy, int batch, int h, int w, int c,
                     int dtype, void* stream);

/* f64 accumulator -> f32 (dst = or += src). */
int shm_cvt_f64_f32(const double* src, float* dst, size_t n, int accumulate, void* stream);
int shm_zero(void* p, size_t bytes, void* stream);

/* ---- 1-output-channel layers ------------------------------------------------------
 * Generator head Conv2D(1, k=1) + LeakyReLU (SHM.py:326). */
int shm_head_fwd(const void* x, int ldx, const float* w, const float* bias, float* y, size_t npix,
                 int c, float slope, int dtype, void* stream);
/* dz = dy*lrelu'(y); dx [G] = dz (x) w; dw_acc[c] += sum x*dz; db_acc[0] += sum dz (f64, not zeroed);
 * red = f64 scratch [SHM_LRELU_RED_SLOTS*(c+1)] (slot staging of the two sums). */
int shm_head_bwd(const void* x, int ldx, const float* w, const float* y, const float* dy, void* dx,
                 int lddx, double* dw_acc, double* db_acc, double* red, size_t npix, int c, float slope,
                 int dtype, void* stream);
/* The same two on the UN-normalised activation a [batch, hw, c] of the block in front of the head + its InstanceNorm statistics
 * (shm_conv2d_in_fwd's `stats`) and beta: the head applies (a - mean) * inv + beta on the fly, so that block needs no
 * shm_in_apply and its normalised tensor is never written.  dx [G] (may be NULL) is the gradient at the NORMALISED activation
 * (shm_in_bwd's g1); dz_out [batch*hw] fp32 (may be NULL) = dy * lrelu'(y), the scalar factor of that gradient (dx = dz_out (x) w). */
int shm_head_in_fwd(const void* a, int lda, const double* stats, const float* beta, const float* w, const float* bias,
                    float* y, int batch, int hw, int c, float slope, int dtype, void* stream);
int shm_head_in_bwd(const void* a, int lda, const double* stats, const float* beta, const float* w, const float* y,
                    const float* dy, void* dx, int lddx, float* dz_out, double* dw_acc, double* db_acc, double* red,
                    int batch, int hw, int c, float slope, int dtype, void* stream);
/* shm_in_bwd for the block in front of the head: its output gradient is the rank-1 tensor hdz[n*h*w + p] * hw_[ch] (hdz =
 * shm_head_in_bwd's dz_out [batch*h*w] with dx = NULL, hw_ = the head kernel [c]), formed on the fly: the head writes no input
 * gradient and neither pass of the backward reads one.  Otherwise as shm_in_bwd (red, dz, dbias, dz_sums, slope). */
int shm_in_bwd_rank1(const float* hdz, const float* hw_, const void* a, int lda, const double* stats, double* red, void* dz,
                     int lddz, double* dbias, double* dz_sums, int batch, int h, int w, int c, float slope, int dtype, void* stream);
/* PatchGAN logits Conv2D(1, k=3, no bias) + LeakyReLU (SHM.py:365-369). x [batch,h,w,c]. */
int shm_patch_fwd(const void* x, int ldx, const float* w, float* y, int batch, int h, int wd, int c,
                  float slope, int dtype, void* stream);
/* dz = dy*lrelu'(y) (written to dz [batch,h,w]); dx [G] = transposed conv of dz (overwritten);
 * dw[9*c] = sum x*dz (overwritten; may be NULL). */
int shm_patch_bwd(const void* x, int ldx, const float* w, const float* y, const float* dy, float* dz,
                  void* dx, int lddx, float* dw, int batch, int h, int wd, int c, float slope,
                  int dtype, void* stream);
/* Flatten + Dense(5, no bias) (SHM.py:371-375): logits[n][j] = sum_k x[n][k] * w[k][j]. */
int shm_dense_fwd(const void* x, const float* w, float* y, int batch, int k, int nout, int dtype,
                  void* stream);
/* dx[n][k] += sum_j dy[n][j]*w[k][j] (accumulates onto dx, a [G] tensor); dw[k][j] = sum_n x[n][k]*dy[n][j]
 * (dw may be NULL). */
int shm_dense_bwd(const void* x, const float* w, const float* dy, void* dx, float* dw, int batch,
                  int k, int nout, int dtype, void* stream);
/* Dropout(0.2) as keep-mask multiply (SHM.py:363): y = x * mask * scale. */
int shm_mul_mask(const void* x, const float* mask, void* y, size_t n, float scale, int dtype,
                 void* stream);

/* ---- colour / standardisation / input assembly (SHM.py:480-531, 544-553, 576-624) -- */
/* tf.image.rgb_to_yuv + custom_per_image_standardization (SHM.py:1271-1309), per sample.
 * acc = f64 scratch [batch*2]; scale_out[batch] receives max(std, 1/256). */
int shm_rgb2yuv_std(const float* rgb, float* yuv, double* acc, float* scale_out, int batch,
                    size_t npix, void* stream);
/* averageCbCr (SHM.py:505): out[b,p,0:2] = mean_k yuv_k[b,p,1:3]. */
int shm_avg_cbcr(const float* y0, const float* y1, const float* y2, const float* y3,
                 const float* y4, float* out, size_t n_pix_total, void* stream);
/* 10-channel generator inputs in a pitch of ldo elements, zero padded (SHM.py:517-531, 576-594).
 * mode 0: G(1) input  -> out [batch,...]: view k = flags[k] ? 0 : Y_k ; one-hot tail = ED.
 * mode 1: cyclic inputs -> out [5*batch,...] (k-major): view j = (j==k) ? 0 : (flags[j] ? genY : Y_j);
 * one-hot k.  yuv_k are the standardised [batch,S,S,3] tensors, genY [batch,S,S,1]. */
int shm_build_gen_input(const float* y0, const float* y1, const float* y2, const float* y3,
                        const float* y4, const float* gen_y, int flags_mask, int mode, void* out,
                        int ldo, int batch, size_t npix, int dtype, void* stream);
/* Gradient of the cyclic inputs back into genY (G o G chain): dgenY[b,p] += sum over k, j!=k with
 * flags[j] of dcyc[k*batch+b, p, j]. */
int shm_cyc_input_bwd(const void* dcyc, int ld, int flags_mask, float* dgen_y, int batch,
                      size_t npix, int dtype, void* stream);
/* tf.image.yuv_to_rgb of concat([Y, avgCbCr]) (SHM.py:544-553, 613-624) for nimg = reps*batch
 * images (image i uses cbcr[i % batch]); writes rgb [nimg,S,S,3] and, if dpad != NULL, the padded
 * discriminator input of pitch ldp (rgb + optional GaussianNoise `noise` [nimg,S,S,3], SHM.py:352). */
int shm_yuv2rgb(const float* ych, const float* cbcr, const float* noise, float* rgb, void* dpad,
                int ldp, int nimg, int batch, size_t npix, int dtype, void* stream);
/* Pack raw rgb [nimg,S,S,3] (+ noise) into the padded discriminator input of pitch ldp. */
int shm_pack_rgb16(const float* rgb, const float* noise, void* dpad, int ldp, size_t npix_total,
                   int dtype, void* stream);
/* dY[i,p] (+)= sum_c d_pad[i,p,c], c<3 (yuv_to_rgb backward: every channel has dRGB/dY = 1). */
int shm_rgb16_to_dy(const void* d16, int ld, float* dy, size_t npix_total, int accumulate, int dtype,
                    void* stream);

/* Step-level random draws (GaussianNoise(0.1) SHM.py:352, Dropout(0.2) SHM.py:363): counter-based Philox-4x32-10, reproducible
 * from (seed, stream_id) whatever the launch geometry.  out[n] ~ N(0, stddev^2);  mask[n] = 1 with probability 1 - rate, else 0
 * (the keep mask shm_mul_mask multiplies by, scaled 1/(1-rate)). */
int shm_randn(float* out, size_t n, float stddev, unsigned long long seed, unsigned stream_id, void* stream);
int shm_keep_mask(float* out, size_t n, float rate, unsigned long long seed, unsigned stream_id, void* stream);

/* ---- losses (SHM.py:669-844) ------------------------------------------------------
 * Discriminator-head losses and their gradients.  Sample order in the D batch:
 * [D1: B][D3: 5B, k-major][D2: B][D4: 5B, k-major].  rf [12B, np], cls [12B,5].
 * Outputs: loss[16] (f64 sums over the batch of: D1_RF, D3_RF, D2_RF, D4_RF, D1_cls, D3_cls,
 * D4_cls), drf_D/dcls_D = gradient of mean_b(total_D+total_Class), drf_G [6B,np] = gradient of
 * mean_b((D1_RF + D3_RF)/6).
 * xent_mode selects the class-logit gradient of tf.nn.softmax_cross_entropy_with_logits (SHM.py:695-713):
 *   SHM_XENT_TF_FUSED (the reference AS EXECUTED): TF's fused kernel returns backprop = softmax - labels and the registered
 *     gradient is grad_loss * backprop, which is the derivative only for labels that sum to 1.  The D1 term's label row is
 *     [0,0,0,0,TARGET_LABELS] (SHM.py:477, 533, 688, 702; TARGET_LABELS ~ U(0.8,1.2), SHM.py:986), so the executed gradient
 *     is softmax - T*onehot;
 *   SHM_XENT_INTENDED: the true derivative sum(labels)*softmax - labels = T*(softmax - onehot).
 * The loss values are the same in both modes; the modes coincide when target == 1 and for every one-hot row (D3, D4). */
#define SHM_XENT_TF_FUSED 0
#define SHM_XENT_INTENDED 1
int shm_dhead_losses(const float* rf, const float* cls, double* loss, float* drf_d, float* dcls_d,
                     float* drf_g, int batch, int np, float target, int xent_mode, void* stream);
/* Image-space generator losses + gradient wrt the generated Y planes.
 * gen_rgb [B,S,S,3], cyc_rgb [5B,S,S,3] (k-major), cyc_y [5B,S,S,1], cbcr [B,S,S,2],
 * orig_k [B,S,S,3] raw rgb, ds_k [B,S,S,3] standardised yuv.
 * loss (f64 [32]): sums over the batch, see shmgan_amd/losses.py for the slot map.
 * dgen_y [B,S,S,1], dcyc_y [5B,S,S,1] are overwritten with d mean_b(10*L1 + 10*ssim + 10*NST).
 * ws: f64/f32 scratch of shm_image_losses_workspace() bytes. */
size_t shm_image_losses_workspace(int batch, int s);
int shm_image_losses(const float* gen_rgb, const float* cyc_rgb, const float* cyc_y,
                     const float* cbcr, const float* const* orig, const float* const* ds,
                     int flags_mask, float style_factor, double* loss, float* dgen_y, float* dcyc_y,
                     void* ws, size_t ws_bytes, int batch, int s, void* stream);
/* The same on rectangular frames: every tensor is [.,h,w,c], same arguments, loss slots and gradient definitions.  SSIM is VALID
 * over (h-10) x (w-10) positions, every mean is taken over h*w pixels and the gram matrices are divided by h*w.  This is the one
 * implementation: shm_image_losses(s) is this call with h = w = s.  SHM_E_SHAPE for a side below 11 (the SSIM window) or a bad
 * batch, SHM_E_WORKSPACE for less than shm_image_losses_hw_workspace(batch, h, w) bytes (0 for a side below 11), all before any
 * launch. */
size_t shm_image_losses_hw_workspace(int batch, int h, int w);
int shm_image_losses_hw(const float* gen_rgb, const float* cyc_rgb, const float* cyc_y,
                        const float* cbcr, const float* const* orig, const float* const* ds,
                        int flags_mask, float style_factor, double* loss, float* dgen_y, float* dcyc_y,
                        void* ws, size_t ws_bytes, int batch, int h, int w, void* stream);

/* ---- image-quality metrics of the reference's test mode (test.py:332-392, --calc_metrics True) ----------------------
 * pred = gen_rgb (the G1 output in RGB, not clipped), target = the diffuse image, both [batch,s,s,3] fp32.  Per image b,
 * out[b][0..4] (f64) = {mse, psnr, ssim, de76, de94}:
 *   mse   mean over s*s*3 of (pred - target)^2                                (test.py:346-347, Keras MeanSquaredError)
 *   psnr  -10 log10(mse), +inf when mse == 0                                 (test.py:338-342, tf.image.psnr, max_val 1)
 *   ssim  tf.image.ssim(rescale_01(pred), rescale_01(target), 5): 11-tap gaussian (sigma 1.5), VALID, k1 0.01, k2 0.03,
 *         mean over (s-10)^2 * 3; rescale_01 (utils.py:190) = (x - min) / (max - min) over the whole image, all three
 *         channels, divide_no_nan (a constant image becomes 0)                (test.py:336)
 *   de76  mean over pixels of |Lab(pred) - Lab(target)|_2                     (test.py:351-353, skimage deltaE_cie76)
 *   de94  mean over pixels of sqrt(max(dL^2 + (dC/(1 + 0.045 C1))^2 + dH^2/(1 + 0.015 C1)^2, 0)), C = hypot(a, b),
 *         dH^2 = 2 (C1 C2 - a1 a2 - b1 b2), C1 of pred (asymmetric)          (test.py:354, skimage deltaE_ciede94)
 * Lab = tfio rgb_to_lab (D65, 2 degree observer): x > 0.04045 ? ((x + 0.055)/1.055)^2.4 : x/12.92; the sRGB -> XYZ matrix;
 * / white (0.95047, 1, 1.08883); f = v > 0.008856 ? cbrt(v) : 7.787 v + 16/116; L = 116 fy - 16, a = 500 (fx - fy),
 * b = 200 (fy - fz).
 * Deterministic and batch-invariant: image b's numbers do not depend on batch or on the other images (per-block partials in
 * workspace slots reduced in a fixed order, no atomics).  ws: shm_image_metrics_workspace() bytes, no initial contents.
 * SHM_E_SHAPE for s < 11 or batch < 1, SHM_E_WORKSPACE for a short workspace, both before any launch. */
size_t shm_image_metrics_workspace(int batch, int s);
int shm_image_metrics(const float* pred, const float* target, double* out, void* ws, size_t ws_bytes, int batch, int s,
                      void* stream);
/* The same five numbers, same definitions, on a window of a padded prediction (native-resolution test mode): pred is
 * [batch,hp,wp,3], the photo is its window of h x w pixels at (top, left), target is tight [batch,h,w,3].  Every mean, the
 * rescale_01 min / max and the VALID 11-tap SSIM ((h-10)(w-10)*3 terms) are taken over the window only; nothing outside it is
 * read.  Deterministic and batch-invariant like the square call; with (hp,wp) = (h,w) = (s,s) and (top,left) = (0,0) it runs the
 * same kernels in the same order.  ws: shm_image_metrics_hw_workspace(batch, h, w) bytes.  SHM_E_SHAPE for a window side < 11, a
 * window outside the frame or batch < 1, SHM_E_WORKSPACE for a short workspace, all before any launch. */
size_t shm_image_metrics_hw_workspace(int batch, int h, int w);
int shm_image_metrics_hw(const float* pred, int hp, int wp, int top, int left, const float* target, int h, int w, double* out,
                         void* ws, size_t ws_bytes, int batch, void* stream);

/* ---- the same metrics split by a region (the highlight, and everything else) ----------------------------------------
 * shm_highlight_region_hw: one launch writes region [batch,h,w] (uint8, 0 or 1) for the window (top, left, h, w) of a frame.
 *   SHM_REGION_RESIDUAL  src [batch,hp,wp,3] fp32 (the photo fed to the generator: the padded frame, pitch and window as pred
 *                        below), target tight [batch,h,w,3] fp32: region = max_c(src_c - target_c) > tau, the subtraction in
 *                        fp32 first, the maximum over the channels after (specular residue is additive and positive); plane unused
 *   SHM_REGION_PLANE     plane [batch,hp,wp] fp32 (the SpecSeg output of the inference): region = plane > tau on the window;
 *                        src and target unused
 * The comparison is strict and a NaN is outside (RESIDUAL: a NaN difference in any channel).  Nothing outside the window is
 * read.  SHM_E_SHAPE before any launch for a null pointer among the ones the mode uses, an unknown mode, batch < 1, a window
 * outside the frame or a window side outside [1, 32768]. */
#define SHM_REGION_RESIDUAL 0
#define SHM_REGION_PLANE 1
int shm_highlight_region_hw(int mode, const float* src, const float* target, const float* plane, int hp, int wp, int top, int left,
                            int h, int w, float tau, unsigned char* region, int batch, void* stream);
/* shm_image_metrics_hw split by region (uint8 [batch,h,w] over the window; any non-zero byte is inside).  Per image b,
 * out[b][0..SHM_REGION_METRICS-1] (f64):
 *   0..4   {mse, psnr, ssim, de76, de94} over the pixels with region != 0 ("in")
 *   5..9   the same over the pixels with region == 0 ("out")
 *   10     n_in, the window's pixels inside; 11: p_in, the SSIM positions inside (exact integers)
 * For a set R of n_R pixels: mse_R = sum over R and the 3 channels of (pred - target)^2 / (3 n_R); psnr_R = -10 log10(mse_R),
 * +inf at 0; de76_R / de94_R = means over R, Lab and dE as above.  The SSIM map is the one shm_image_metrics_hw averages
 * (rescale_01 with the min / max of the WHOLE window, 11-tap gaussian, VALID, (h-10)(w-10) positions per channel); position
 * (i, j) belongs to R when its centre pixel (i+5, j+5) of the window does, and ssim_R is the mean over those positions and the
 * 3 channels.  An empty set (no pixels; for ssim no positions) gives NaN.  So n_in mse_in + n_out mse_out = h w mse, the same
 * for de76 and de94, and p_in ssim_in + p_out ssim_out = (h-10)(w-10) ssim of shm_image_metrics_hw.
 * The same three kernels, grids and fixed-order reduction as shm_image_metrics_hw with a second set of accumulators:
 * deterministic and batch-invariant, and with region all ones out[b][0..4] is bit for bit shm_image_metrics_hw's result
 * (all zeros: out[b][5..9]).  ws: shm_image_metrics_region_hw_workspace(batch, h, w) bytes, no initial contents.  SHM_E_SHAPE
 * for a window side < 11, a window outside the frame, batch < 1 or a null pointer, SHM_E_WORKSPACE for a short workspace, all
 * before any launch. */
#define SHM_REGION_METRICS 12
size_t shm_image_metrics_region_hw_workspace(int batch, int h, int w);
int shm_image_metrics_region_hw(const float* pred, int hp, int wp, int top, int left, const float* target, int h, int w,
                                const unsigned char* region, double* out, void* ws, size_t ws_bytes, int batch, void* stream);

/* ---- SpecSeg mask network, inference only (SpecSeg.py:27-98; SpecSeg.predict at SHM.py:492) --
 * Its Conv2D(3x3, relu) layers are shm_conv2d_fwd with slope 0.  The rest: */
/* dst[p, 0:nc] = src[p, c0:c0+nc], dst[p, nc:lddst] = 0 (the Y plane into a 16-float pitch). */
int shm_pack_channels(const float* src, int ldsrc, int c0, int nc, float* dst, int lddst, size_t npix,
                      void* stream);
/* Keras BatchNormalization(axis=-1) in inference mode (SpecSeg.py:37,43,49,55,60):
 * out = (a - moving_mean) * gamma / sqrt(moving_var + eps) + beta. */
int shm_bn_apply(const float* a, int lda, const float* gamma, const float* beta, const float* mean,
                 const float* var, float eps, float* out, int ldo, size_t npix, int c, void* stream);
/* MaxPooling2D((2,2)) on even sizes (SpecSeg.py:38,44,50,56). */
int shm_maxpool2_fwd(const float* x, int ldx, float* y, int ldy, int batch, int h, int w, int c,
                     void* stream);
/* Conv2DTranspose(k=2, strides=2, 'same') + bias (SpecSeg.py:63,69,75,81).  w = Keras layout
 * [2][2][cout][cin] as stored; y [batch,2hi,2wi,cout]; slope 1.0f = linear. */
int shm_conv2d_transpose2x2_fwd(const void* x, int ldx, const void* w, const float* bias, void* y,
                                int ldy, int batch, int hi, int wi, int cin, int cout, float slope,
                                int dtype, void* stream);
/* Conv2D(1, (1,1), activation='sigmoid') (SpecSeg.py:88). */
int shm_head_sigmoid_fwd(const float* x, int ldx, const float* w, const float* bias, float* y,
                         size_t npix, int c, void* stream);
/* Spec_loss terms (SHM.py:792-796, logged only): loss[k] (f64 [5], zeroed by the call) = sum over
 * samples, pixels and the 3 yuv channels of (mask * cyc_k_yuv - mask * ds_k)^2, where
 * cyc_k_yuv = concat(cyc_y[k*batch + b], cbcr[b]); mask [batch,S,S,1].  ds = host array of 5
 * device pointers.  reduce_mean = loss / (batch*npix*3). */
int shm_spec_loss(const float* cyc_y, const float* cbcr, const float* const* ds, const float* mask,
                  double* loss, int batch, size_t npix, void* stream);

/* ---- live attention branch: attention_layer SHM.py:404-412, its use at SHM.py:248-275, 290-293, 358-359 ------------
 * The reference evaluates attention_layer on a constant zero mask at model-build time (SURVEY finding 3), so the executed
 * graph adds zeros; these entry points serve the "as-intended" mode (attention="live"): the SpecSeg mask of the step goes
 * through MaxPooling2D -> Conv2D(1->C, 3x3, leaky_relu) -> Conv2D(C->C, 3x3, leaky_relu) (the two convolutions are
 * shm_conv2d_fwd / _dgrad / _wgrad + shm_lrelu_bwd) and is added to the skip tensor. */
/* MaxPooling2D(k x k) of mask [batch,s,s,1] (fp32) into channel 0 of dst [batch,s/k,s/k,lddst] (activation-typed, other
 * channels zeroed); k = 1 copies (attention_layer(pool=False), SHM.py:248). */
int shm_mask_pool_pack(const float* mask, void* dst, int lddst, int batch, int s, int k, int dtype, void* stream);
/* The rectangular form: mask [batch,h,w,1] into dst [batch,h/k,w/k,lddst]; h and w multiples of k. */
int shm_mask_pool_pack_hw(const float* mask, void* dst, int lddst, int batch, int h, int w, int k, int dtype, void* stream);
/* out[i] = a[i] + b[(i0 + i) % nb] for nimg images of `per` elements (per % 4 == 0): skip + attention map of the image's
 * sample (SHM.py:290-293, 359); in the batched plan image i0 + i of the batch is a copy of sample (i0 + i) % nb. */
int shm_add_bcast(const void* a, const void* b, void* out, int nimg, size_t per, int nb, int i0, int dtype, void* stream);
/* Its gradient wrt b: dst[j] (+)= sum of src[i] over the images with (i0 + i) % nb == j. */
int shm_sum_groups(const void* src, void* dst, int nimg, size_t per, int nb, int i0, int accumulate, int dtype, void* stream);

/* ---- input pipeline (datasetLoader.py:47-60: image_dataset_from_directory -> /255 -> flip_up_down) ----
 * tf.image.resize(bilinear, half-pixel centres, no antialias) of one decoded uint8 image [hin,win,c] to
 * float32 [ho,wo,c], times `scale` (1/255), optionally flipped top-to-bottom. */
int shm_resize_bilinear_u8(const unsigned char* src, int hin, int win, int c, float* dst, int ho, int wo,
                           float scale, int flip_ud, void* stream);
/* Native-resolution test mode: one decoded uint8 image [h,w,c] into the float32 frame [hp,wp,c] without resampling, the image at
 * (top, left), the border filled by reflection WITHOUT repeating the edge sample (NumPy's mode="reflect"):
 *   dst[y][x][k] = (float)src[r(y - top, h)][r(x - left, w)][k] * scale,   r(i, n) = i < 0 ? -i : i >= n ? 2 (n-1) - i : i
 * One launch; 16-byte stores when dst is 16-byte aligned and hp*wp*c % 4 == 0, scalar stores otherwise (same values).
 * SHM_E_SHAPE for a null pointer, a size outside [1, 32768], c > 16, an image that does not lie inside the frame or a pad wider
 * than the image less one (the reflection would leave the image), before any launch. */
int shm_load_pad_u8(const unsigned char* src, int h, int w, int c, float* dst, int hp, int wp, int top, int left, float scale,
                    void* stream);

/* ---- polarimetry: the estimated-diffuse target and the Stokes maps (utils.py:68-123 calculate_estimate_diffuse, whose imwrite
 * is commented out; SHM.py:1157-1169 calcDOP; neither is called by the reference's training path, which reads a pre-computed ED/
 * directory) ---------------------------------------------------------------------------------------------------------------------
 * The four decoded views of ONE sample -> that sample's five training planes, one launch, one thread per output pixel.
 * src_ptrs: host array of 4 device pointers to uint8 [hin,win,3] images of the same size; dst_ptrs: host array of 5 device
 * pointers to float32 [ho,wo,3] planes (the sample's slices of the loader's five [B,S,S,3] tensors); both arrays are read during
 * the call and the nine pointers travel to the kernel by value.  Per output pixel, channel and tap position t in {tl, tr, bl, br}
 * (the taps, weights lx / ly and the row flip of shm_resize_bilinear_u8: half-pixel centres, lower = max(floor, 0),
 * upper = min(ceil, n-1)) the four bytes v0..v3 are read once, and with lerp(q) = (top + (bot - top) ly) * scale,
 * top = q_tl + (q_tr - q_tl) lx, bot = q_bl + (q_br - q_bl) lx, all in fp32:
 *   dst[i] = lerp(v_i)        i = 0..3: the arithmetic of shm_resize_bilinear_u8 on view i
 *   dst[4] = lerp(e)          e_t = e(v0_t, v1_t, v2_t, v3_t): the estimate is made PER TAP, at source resolution, and then
 *                             resized -- the resize of the reference's estimated-diffuse image, not the estimate of resized views
 *   SHM_POLAR_MIN      e = min(v0, v1, v2, v3) (the reference's definition); coef is not read and may be null
 *   SHM_POLAR_STOKES   coef = host float[12], a row-major 3x4 matrix C with (S0, S1, S2) = C (v0..v3);
 *                      e = clamp(0.5 (S0 - sqrt(S1^2 + S2^2)), 0, 255): the minimum over ALL polariser angles of the fitted
 *                      I(theta) = 0.5 (S0 + S1 cos 2 theta + S2 sin 2 theta), which the minimum of four samples overestimates
 * With (ho,wo) = (hin,win) every weight is 0 and dst[i] = v_i * scale, dst[4] = e * scale exactly.  SHM_E_SHAPE for a null
 * pointer (either array or any entry), a size outside [1, 32768], an unknown mode or SHM_POLAR_STOKES without coef; all before
 * any launch. */
#define SHM_POLAR_MIN 0
#define SHM_POLAR_STOKES 1
int shm_polar_views_u8(const unsigned char* const* src_ptrs, int hin, int win, const float* coef, int mode,
                       float* const* dst_ptrs, int ho, int wo, float scale, int flip_ud, void* stream);
/* Train-time augmentation of ONE sample in the launch that resizes it: shm_polar_views_u8 with a crop window, two mirrors and
 * an optional re-mix of the four views, or (SHM_AUG_DIR) the same for five sources.  One launch, one thread per output pixel.
 * src_ptrs: host array of n_src device pointers to uint8 [hin,win,3] images of one size; dst_ptrs: host array of 5 device pointers
 * to float32 [ho,wo,3] planes; both arrays, coef and mix are read during the call and travel to the kernel by value.
 *   mode   SHM_AUG_DIR: n_src = 5, plane 4 is source 4 resampled like the views.  SHM_POLAR_MIN / SHM_POLAR_STOKES: n_src = 4,
 *          plane 4 is the per-tap estimate e(v0..v3) exactly as shm_polar_views_u8 defines it (coef as there).
 *   sampling   output pixel (oy, ox) samples at sy = flip_ud ? ho-1-oy : oy, sx = flip_lr ? wo-1-ox : ox (the mirrors are on the
 *          read side); fy = ((sy + 0.5f) * (crop_h / ho) - 0.5f) + crop_y, fx alike with crop_w / wo and crop_x, in fp32; taps and
 *          weights as shm_resize_bilinear_u8: lower = max(floor(fy), 0), upper = min(ceil(fy), hin-1), ly = fy - floor(fy).  The
 *          taps are held inside the IMAGE, not the crop: a crop edge interpolates against its real neighbours.
 *   mix    null, or a host float[16], a row-major 4x4 matrix M: the four view bytes of every tap are replaced by
 *          v'_i = clamp(((M[i][0] v0 + M[i][1] v1) + M[i][2] v2) + M[i][3] v3, 0, 255) before the lerp (polar.mirror_views: the
 *          views a polariser at 180 - theta_i would have seen, from the Stokes fit).  The fifth plane is never mixed: a fifth
 *          source is read as it is, and an estimate is made from the UNMIXED bytes (the unpolarised part is mirror-invariant).
 * dst[i] = lerp(v'_i) * scale, dst[4] = lerp(source 4 or e) * scale, in the lerp order of shm_polar_views_u8.
 * Identity parameters -- crop (0, 0, hin, win), flip_lr = 0, mix null -- give bitwise the planes of five shm_resize_bilinear_u8
 * calls (SHM_AUG_DIR) and of shm_polar_views_u8 (MIN / STOKES) for either flip_ud: the same expressions, then + 0.0f.
 * SHM_E_SHAPE for a null array or entry, an unknown mode, an n_src that does not fit the mode, a size outside [1, 32768],
 * crop_h <= 0 or crop_w <= 0, a crop that does not lie inside [0,hin] x [0,win] (a NaN anywhere fails these) or SHM_POLAR_STOKES
 * without coef; all before any launch. */
#define SHM_AUG_DIR 2
int shm_augment_views_u8(const unsigned char* const* src_ptrs, int n_src, int hin, int win, int mode, const float* coef,
                         const float* mix, float crop_y, float crop_x, float crop_h, float crop_w, int flip_ud, int flip_lr,
                         float* const* dst_ptrs, int ho, int wo, float scale, void* stream);
/* shm_augment_views_u8 for a whole batch: sample i of `samples` (a host array of n >= 1 descriptors, read during the call) is
 * resampled into slice i of five float32 [n,ho,wo,3] tensors, dst_ptrs[p] + i * sample_stride (floats) being its plane p.  One
 * launch per SHM_AUG_GROUP samples, grid (cdiv(ho*wo, 256), samples of the group): every block row reads its own descriptor, which
 * travels to the kernel by value; n may exceed the group and is cut into cdiv(n, SHM_AUG_GROUP) launches.
 *   descriptor   src: n_src device pointers to uint8 [hin,win,3] images (src[4] is read only with SHM_AUG_DIR); hin, win and the crop
 *          are the sample's own; flip_ud, flip_lr and mix are flags (nonzero = on); plane[v] is the destination plane of view v =
 *          0..3, a permutation of 0..3 (identity (0,1,2,3); a mirror that exchanges two polariser angles exchanges their planes).
 *          Plane 4 is always plane 4.
 *   shared   n_src, mode, coef, scale, ho, wo as shm_augment_views_u8; mix: a host float[16] used by the samples whose mix flag is
 *          set, and may be null when none is.
 * The bits written for a sample are those of shm_augment_views_u8 called for that sample alone with dst_ptrs permuted by `plane`
 * (the same per-pixel code: csrc/augment_px.h), so at identity parameters those of shm_resize_bilinear_u8 / shm_polar_views_u8.
 * SHM_E_SHAPE for n < 1, a null array or destination, an unknown mode, an n_src that does not fit it, ho or wo outside [1, 32768],
 * a sample_stride below ho*wo*3 with n > 1, SHM_POLAR_STOKES without coef, and per sample -- the message names its index -- a null
 * source, hin or win outside [1, 32768], an empty crop or one outside the image (checked in double; a NaN fails), a mix flag
 * without mix, or planes that are no permutation of 0..3.  Every sample is checked before the first launch. */
#define SHM_AUG_GROUP 8
typedef struct shm_aug_sample {
    const unsigned char* src[5];
    int hin, win;
    float crop_y, crop_x, crop_h, crop_w;
    int flip_ud, flip_lr, mix;
    int plane[4];
} shm_aug_sample;
int shm_augment_batch_u8(const shm_aug_sample* samples, int n, int n_src, int mode, const float* coef, const float* mix,
                         float* const* dst_ptrs, size_t sample_stride, int ho, int wo, float scale, void* stream);
/* The mask network's training pairs (SpecSeg.train_step's x and y) from decoded bytes, a whole batch in one call: sample i of
 * `samples` (a host array of n >= 1 descriptors, read during the call; they travel to the kernels by value) is written to
 * x + i * sample_stride and y + i * sample_stride (floats), each a float32 [ho,wo] plane.  Launches cover SHM_AUG_GROUP samples
 * each (two per group: resample with partial sums, then finish); n may exceed the group.
 *   descriptor   image: device uint8 [hin,win,3]; mask: device uint8 [hin,win]; hin, win and the crop (y, x, h, w) are the
 *          sample's own; flip_ud and flip_lr are flags (nonzero = on).
 *   sampling   the coordinate, taps and lerp of shm_augment_views_u8 (the same code: csrc/augment_px.h): mirrors on the read side,
 *          taps held inside the image, not the crop.
 *   y      lerp(mask bytes) * (1/255): bitwise what shm_resize_bilinear_u8 (c = 1, scale 1/255) writes at identity parameters, and
 *          for any parameters bitwise the plane shm_augment_views_u8 (SHM_AUG_DIR, scale 1/255) writes for a 3-channel copy of the mask.
 *   x      r, g, b = lerp(image bytes) * (1/255) per channel; (Y, U, V) = tf.image.rgb_to_yuv with the constants and expression
 *          order of shm_rgb2yuv_std; x = Y / scale, scale = max(std, 1/256), std over all 3*ho*wo values of Y, U and V of the
 *          resampled sample from f64 sums (the formulas of shm_rgb2yuv_std).  U and V enter the statistics and are not written;
 *          no float RGB or YUV tensor goes to memory.
 *   statistics   no atomics: every block writes its two f64 sums to its own slot of `ws`, and the finish adds a sample's slots in a
 *          fixed order.  The blocks per sample depend on ho*wo alone, so a sample's bits do not depend on n, on its slot in the
 *          batch or on its neighbours, and two calls give the same bits.  ws: device f64, shm_augment_pairs_ws_doubles(n, ho, wo)
 *          doubles (0 for arguments the call would refuse); it needs no initial value and holds nothing of use afterwards.
 *   scale_out   null, or device float32 [n]: receives every sample's scale.
 * SHM_E_SHAPE for n < 1, a null array, x, y or ws, ho or wo outside [1, 32768], a sample_stride below ho*wo with n > 1, and per
 * sample -- the message names its index -- a null image or mask, hin or win outside [1, 32768], an empty crop or one outside the
 * image (checked in double; a NaN fails).  Every sample is checked before the first launch. */
typedef struct shm_pair_sample {
    const unsigned char* image;
    const unsigned char* mask;
    int hin, win;
    float crop_y, crop_x, crop_h, crop_w;
    int flip_ud, flip_lr;
} shm_pair_sample;
size_t shm_augment_pairs_ws_doubles(int n, int ho, int wo);
int shm_augment_pairs_u8(const shm_pair_sample* samples, int n, float* x, float* y, size_t sample_stride, int ho, int wo,
                         double* ws, float* scale_out, void* stream);
/* Stokes maps of four float32 views of n elements each (any shape: the loaded RGB views or their Y channels).  view_ptrs: host
 * array of 4 device pointers; coef: host float[12], the 3x4 matrix above.  Per element (S0, S1, S2) = C (v0..v3) and
 *   s0 = S0;  dop = sqrt(S1^2 + S2^2) / S0, 0 where S0 == 0 (divide_no_nan, as calcDOP);  aolp = 0.5 atan2f(S2, S1)
 * Each of s0, dop, aolp (device float32 [n]) may be null and is then not written; with all three null nothing is launched.
 * One grid-stride launch; 16-byte accesses when n % 4 == 0 and every pointer is 16-byte aligned, scalar ones otherwise (same
 * values).  SHM_E_SHAPE for a null view_ptrs, view or coef, or n == 0, before any launch. */
int shm_polar_maps(const float* const* view_ptrs, size_t n, const float* coef, float* s0, float* dop, float* aolp,
                   void* stream);

/* ---- division-of-focal-plane (DoFP) polarisation sensors: one raw mosaic -> the four views (csrc/dofp.hip) --
 * On such a sensor (Sony IMX250MZR / MYR and relatives) every 2 x 2 quad of pixels sits behind four micro-polarisers, and on the
 * colour parts every quad sits behind one Bayer filter.  The period P is 2 for SHM_DOFP_MONO and 4 for the Bayer patterns.
 *   src       the mosaic on the device: uint8 when bits == 8, uint16 when 9 <= bits <= 16, the significant bits LSB-aligned (a 12-bit
 *             value stored in 16 bits is bits = 12, an MSB-aligned file is bits = 16); h rows of w samples, consecutive rows
 *             src_pitch >= w ELEMENTS apart.  A 16-bit sample above 2^bits - 1 is not masked: the clamp below handles it.
 *   quad      host int[4], read during the call: the view index 0..3 at quad positions (0,0), (0,1), (1,0), (1,1), a permutation
 *             of 0..3.  Sony's 90 / 45 / 135 / 0 with the views in ascending angle is {2, 1, 3, 0}.
 *   dst_ptrs  host array of 4 device pointers to uint8 [ho,wo,3] planes, read during the call; total: null, or a fifth such plane.
 * Lattices: the sample at quad position (ay, ax) under colour block (by, bx) of the Bayer tile lies on the lattice with offsets
 * dy = 2 by + ay, dx = 2 bx + ax and period P (SHM_DOFP_MONO: by = bx = 0).  A view's channel has one lattice for R, one for B and
 * two for G; SHM_DOFP_MONO gives the view's single lattice to all three channels.  All arithmetic is integer and exact:
 *   SHM_DOFP_BILINEAR   (ho, wo) = (h, w).  Per axis of length N a lattice with offset d has n = (N - 1 - d) / P + 1 samples; for the
 *             output coordinate y: q = y - d, i0 = floor(q / P), f = q - P i0, taps clamp(i0, 0, n - 1) with weight P - f and
 *             clamp(i0 + 1, 0, n - 1) with weight f.  A lattice's numerator is the product-weighted sum of its 2 x 2 taps (total
 *             weight P^2); a channel's numerator N is the sum over its lattices, and k = 2 log2 P, plus 1 for G.
 *   SHM_DOFP_BIN        (ho, wo) = (h / P, w / P), remainder rows and columns dropped: N is the lattice's own sample of that
 *             super-pixel, summed over the channel's lattices; k = 0, or 1 for G.  No interpolation.
 *   finish    with s = bits - 8:  view = min(255, (N + (1 << (k + s) >> 1)) >> (k + s));
 *             total = min(255, (sum of the four views' N + (1 << (k + s + 2) >> 1)) >> (k + s + 2)): the round-half-up of the
 *             UNROUNDED mean of the four views, S0 / 2.
 * In bilinear mode the mono, R and B channels return the sample itself at its own site; G is half the own sample plus half the mean of
 * the diagonal neighbours.  One launch, no atomics, no host synchronisation; four consecutive pixels of a plane are three dword stores
 * when they start 4-byte aligned, byte stores otherwise (same values).  SHM_E_SHAPE before any launch for a null src, quad or
 * dst_ptrs or a null entry of dst_ptrs, bits outside [8, 16], an unknown pattern or mode, h or w outside [P, 32768], src_pitch < w, or
 * a quad that is not a permutation of 0..3. */
#define SHM_DOFP_MONO 0
#define SHM_DOFP_RGGB 1
#define SHM_DOFP_BGGR 2
#define SHM_DOFP_GRBG 3
#define SHM_DOFP_GBRG 4
#define SHM_DOFP_BILINEAR 0
#define SHM_DOFP_BIN 1
int shm_dofp_views(const void* src, int bits, int h, int w, size_t src_pitch, int pattern, const int* quad, int mode,
                   unsigned char* const* dst_ptrs, unsigned char* total, void* stream);

/* ---- developing a polariser mosaic: black level, white balance, colour matrix, tone curve (csrc/dofp_develop.hip) ----
 * shm_dofp_develop is shm_dofp_views with another finish: the same arguments, lattices, taps and numerators, and then, instead of the cut
 * to 8 bits, a development of the UNROUNDED numerator.  Two more device arrays and one host array:
 *   params       device int[SHM_DOFP_PARAMS], read by the kernel (so a balance estimated on the device needs no round trip):
 *                [SHM_DOFP_P_BLACK + c]  black_c, the sensor's count for darkness, 0 .. 65535 - 16, c = 0 R, 1 G, 2 B
 *                [SHM_DOFP_P_MUL + c]    mul_c, a uint32 in Q16 (its bit pattern), 65536 <= mul_c < 2^32: the host's round-half-up of
 *                                        65535 * 65536 * wb_c / (white - black_c), wb normalised to a smallest entry of 1, every wb_c <= 16,
 *                                        white - black_c >= 16
 *                [SHM_DOFP_P_GAIN + c]   gain_c in Q10, 1024 = 1, 1 .. 16383: 1024 from the host, shm_dofp_wb_gray's estimate otherwise
 *                [SHM_DOFP_P_FLAGS]      bit 0: apply the matrix
 *                [SHM_DOFP_P_CCM + 3c + j]  ccm[c][j], signed Q10, |ccm| <= 8191 (row-major: output channel c from linear channel j)
 *                [SHM_DOFP_P_WHITE]      white, the count of a saturated sample: not read by shm_dofp_develop, shm_dofp_wb_gray's
 *                                        callers take their default `sat` from it
 *   lut          device uint8[4096], 16-byte aligned: the tone table, indexed by the top 12 of 16 bits
 *   params_host  host int[SHM_DOFP_PARAMS]: the caller's mirror of `params`; the refusals below are made from it (its gains are not read)
 * Arithmetic, all integer.  N is a view's channel numerator exactly as above, with total weight 2^k (k as in `finish`, the 1 for G
 * included); for `total`, N is the sum of the four views' numerators and k is 2 larger -- the UNROUNDED mean is developed, not the rounded
 * views.  With c in {R, G, B}:
 *   1. D = max(0, N - (black_c << k))                                   the pedestal, removed at numerator scale: no rounding
 *   2. M_c = (mul_c * gain_c + 512) >> 10                               in 64 bits; M_c < 2^36
 *   3. lin_c = min(65535, (D * M_c + (1 << (15 + k))) >> (16 + k))      in 64 bits: D < 2^23
 *   4. with the matrix: lin'_c = clamp((sum_j ccm[c][j] * lin_j + 512) >> 10, 0, 65535)     arithmetic shift; the sum fits 32 bits because
 *      of the clamp in 3, which is also what keeps a saturated highlight from wrapping.  Without: lin'_c = lin_c
 *   5. out_c = lut[lin'_c >> 4]
 * lin is within 1 unit of 65535 of the real-valued (N / 2^k - black_c) * 65535 wb_c gain_c / (white - black_c): 0.5 from its own rounding, at
 * most 0.5 from mul_c, which is within 2^-17 relative of the real factor.  Gains of at least 1 and the clamp make an all-saturated pixel
 * (255, 255, 255) under every balance.  SHM_DOFP_MONO develops its one numerator with channel 0's parameters and writes it to R, G and B.
 * One launch, no atomics, no host synchronisation; the stores are shm_dofp_views'.  SHM_E_SHAPE before any launch for everything
 * shm_dofp_views refuses, and for a null params, lut or params_host, a lut that is not 16-byte aligned, a mirror with black outside
 * [0, 65519], mul below 65536, |ccm| above 8191 or unknown flag bits, and SHM_DOFP_MONO with a mirror whose three channels differ (black or
 * mul) or whose matrix flag is set. */
#define SHM_DOFP_P_BLACK 0
#define SHM_DOFP_P_MUL 3
#define SHM_DOFP_P_GAIN 6
#define SHM_DOFP_P_FLAGS 9
#define SHM_DOFP_P_CCM 10
#define SHM_DOFP_P_WHITE 19
#define SHM_DOFP_PARAMS 20
#define SHM_DOFP_LUT 4096
int shm_dofp_develop(const void* src, int bits, int h, int w, size_t src_pitch, int pattern, const int* quad, int mode,
                     unsigned char* const* dst_ptrs, unsigned char* total, const int* params, const unsigned char* lut,
                     const int* params_host, void* stream);
/* Grey-world gains of one frame, left on the device (Bayer patterns only).  Over the COMPLETE 4 x 4 periods of the mosaic in which all 16
 * samples are below `sat` (a clipped highlight must not pull the estimate), for every sample v of colour c:
 *   S_c += max(0, v - black_c);  n_c += 1                               uint64, black_c from params_in
 * and then  mean_c = (S_c << 8) / n_c, 0 when n_c == 0;  if any mean is 0 all three gains are 1024, otherwise
 *   gain_c = min(16383, (max_j mean_j << 10) / mean_c)
 * params_out (device int[SHM_DOFP_PARAMS]; may be params_in) becomes params_in with the three gains replaced: shm_dofp_develop on the
 * same stream reads it.  ws: device unsigned long long[SHM_DOFP_WB_WS]; after the call ws[0..2] = S_c, ws[3..5] = n_c, ws[6..8] = the
 * gains; it needs no clearing.  Integer sums: every reduction order gives the same bits.  Two launches (per-block sums of a
 * grid-stride walk over the periods, then one block that adds them and finishes), no atomics, no host synchronisation.  SHM_E_SHAPE
 * before any launch for a null pointer, bits outside [8, 16], a pattern that is not one of the four Bayer ones, h or w outside
 * [4, 32768], src_pitch < w, or sat outside [1, 65536]. */
#define SHM_DOFP_WB_BLOCKS 512
#define SHM_DOFP_WB_WS 3088 /* 16 + 6 * SHM_DOFP_WB_BLOCKS */
int shm_dofp_wb_gray(const void* src, int bits, int h, int w, size_t src_pitch, int pattern, const int* params_in, int sat,
                     int* params_out, unsigned long long* ws, void* stream);

/* ---- calibrating a polariser mosaic: dark frame, flat field, defect map (csrc/dofp_calibrate.hip) ---------------
 * Runs on the raw mosaic, in front of shm_dofp_views / shm_dofp_develop / shm_dofp_wb_gray: each view is built from one photosite per quad,
 * so a hot sample or a gain difference inside a quad exists in one view only and reads as polarisation once it is interpolated.
 *   src, dst   uint8 when bits == 8, uint16 otherwise, as shm_dofp_views takes its src; h rows of w samples, rows src_pitch / dst_pitch
 *              ELEMENTS apart.  dst must not overlap src (a defective site reads its neighbours from src); dst == src is refused.
 *   dark       device uint16 [h,w], tight: the master dark frame, pedestal included.  Null: `pedestal` everywhere.
 *   gain       device uint16 [h,w], tight, Q12 (4096 = 1), every entry in [SHM_DOFP_GAIN_MIN, SHM_DOFP_GAIN_MAX].  Null: 4096 everywhere.
 *   defect     device uint8 [h,w], tight: non-zero marks a photosite to be replaced.  Null: none.
 *   pedestal   the count the corrected dark level is put back to, 0 .. 65519: it is kept, not removed, so that the black level of
 *              shm_dofp_develop and the grey-world estimate go on meaning what they mean and noise around black is not clipped at zero.
 *   white      samples at or above it are saturated and pass through untouched, 1 .. 65536 (65536: none is).
 * P = 2 for SHM_DOFP_MONO and 4 for the Bayer patterns (the pattern is read for nothing else); maxv = 2^bits - 1.  All integer, exact:
 *   corr(y,x):  v = src[y,x]
 *               if v >= white: return v                                    a saturated sample stays saturated
 *               e = ((v - dark[y,x]) * gain[y,x] + 2048) >> 12             signed, arithmetic shift (floor); fits int32: |v - dark| <= 65535,
 *                                                                          gain <= 16383
 *               return clamp(pedestal + e, 0, maxv)
 *   dst[y,x] = corr(y,x)                    where defect is null or defect[y,x] == 0
 *            = (2 S + n) / (2 n)  (floor)   otherwise: S, n = sum and count of corr over those of the four same-lattice neighbours
 *                                           (y-P,x) (y+P,x) (y,x-P) (y,x+P) that lie inside the image and are not themselves defective:
 *                                           the round-half-up of their mean
 *            = corr(y,x)                    if n == 0
 * With dark == pedestal, gain == 4096 and no defects dst equals src for every sample <= maxv.  One launch, no atomics, no host
 * synchronisation; a thread makes 8 consecutive samples of a row with one 8- or 16-byte access per array where base, pitch (tables: w)
 * are multiples of 8 elements, single-element accesses otherwise (same values).  SHM_E_SHAPE before any launch, dst untouched, for
 * everything shm_dofp_views refuses about src, bits, h, w, src_pitch and pattern, a null dst, dst_pitch < w, dst == src, pedestal outside
 * [0, 65519] or white outside [1, 65536]. */
#define SHM_DOFP_GAIN_MIN 1024
#define SHM_DOFP_GAIN_MAX 16383
int shm_dofp_calibrate(const void* src, int bits, int h, int w, size_t src_pitch, int pattern, const unsigned short* dark,
                       const unsigned short* gain, const unsigned char* defect, int pedestal, int white, void* dst, size_t dst_pitch,
                       void* stream);

/* ---- merging an exposure bracket of polariser mosaics (csrc/dofp_merge.hip) ----------------------------------------
 * A highlight is the part of a scene one exposure cannot hold: where all four photosites of a quad sit at the white level the four views are
 * equal and the Stokes fit reads no polarisation exactly where the highlight is strongest.  A bracket of n exposures of a static scene is
 * merged per photosite, on the raw mosaic, in front of shm_dofp_views / shm_dofp_develop / shm_dofp_wb_gray (and behind shm_dofp_calibrate
 * of every page).
 *   src_ptrs    HOST array of n DEVICE pointers, 2 <= n <= SHM_DOFP_MERGE_MAX: the pages, each uint8 when bits == 8 and uint16 otherwise, h
 *               rows of w samples, rows src_pitch ELEMENTS apart (one pitch for all pages).  Read during the call; the pointers travel to the
 *               kernel by value.  Page k was taken with exposure e_k, a positive integer <= 65535 in any unit (only ratios matter); e_min is
 *               the smallest.
 *   table       DEVICE uint32 [SHM_DOFP_MERGE_TABLE], indexed by the mask m of valid pages (bit k = page k), 1 <= m <= 2^n - 1:
 *                 T_m    = sum of e_k over the set bits k of m
 *                 mul[m] = floor((2 * (e_min << (f + SHM_DOFP_MERGE_Q)) + T_m) / (2 * T_m)),  f = 16 - bits
 *               the round-half-up of e_min * 2^f * 2^20 / T_m, in [1, 2^(f+20)].  mul[0] and the entries from 2^n on are not read.
 *   table_host  the caller's HOST mirror of table: the refusals are made from it (as shm_dofp_develop does with params_host).
 *   black       the count for darkness.   white: the count from which a sample is saturated, 1 .. 2^bits (2^bits: none is).
 *   dst         device uint16, rows dst_pitch elements apart; not one of the pages.
 *   counts      device unsigned [SHM_DOFP_MERGE_MAX + 1] or null: counts[j] = the number of photosites with exactly j valid pages, so
 *               counts[0] is what is still clipped in every page.  Cleared on the stream by this call and filled with integer atomics (the
 *               same bits on every run); null: nothing is counted.
 * Per photosite, all integer, exact:
 *   page k is valid when v_k < white;  m = the mask of valid pages
 *   E   = sum over the valid pages of (v_k - black)                        signed; |E| < 2^19
 *   R   = (E * mul[m] + 2^19) >> 20                                        in int64, arithmetic shift (floor)
 *   dst = clamp((black << f) + R, 0, 65535)                                m != 0
 *       = min(65535, white << f)                                           m == 0
 * Every unsaturated page votes, weighted by its exposure time (the maximum-likelihood estimate under photon noise, so no lower threshold is
 * needed); the result is a 16-bit mosaic on the scale of the SHORTEST exposure with f fractional bits.  A site valid in the shortest page
 * only comes out as exactly v << f; a valid site is always strictly below white << f.  mul is within 1/2 of the real factor and |E| < 2^19,
 * so dst is within 0.75 of the real-valued quotient (0.5 from its own rounding, at most 0.25 from mul).
 * One launch; the clear of counts is a second action on the stream; no host synchronisation.  A thread makes 8 consecutive samples of a row
 * with one 16-byte (uint16) or 8-byte (uint8) access per page and one 16-byte store where base and pitch are multiples of 8 elements (each
 * page and dst judged separately), single-element accesses otherwise (same values).  SHM_E_SHAPE before any launch, dst and counts untouched,
 * for: a null src_ptrs, entry, table, table_host or dst; n outside [2, 8]; bits outside [8, 16]; h or w outside [1, 32768]; a pitch below w;
 * dst equal to a page; black below 0 or black << f above 65519 (shm_dofp_develop's limit for a black level); white outside [1, 2^bits] or
 * not above black; a table_host entry m in 1 .. 2^n - 1 outside [1, 2^(f+20)]. */
#define SHM_DOFP_MERGE_MAX 8
#define SHM_DOFP_MERGE_TABLE 256
#define SHM_DOFP_MERGE_Q 20
int shm_dofp_merge(const void* const* src_ptrs, int n, int bits, int h, int w, size_t src_pitch, const unsigned* table,
                   const unsigned* table_host, int black, int white, unsigned short* dst, size_t dst_pitch, unsigned* counts, void* stream);

/* ---- specular masks from the polarised views (csrc/specmask.hip) ------------------------------------------
 * Specular reflection is polarised, diffuse reflection is not: the polarised intensity sqrt(S1^2 + S2^2) of the Stokes fit, the part
 * SHM_POLAR_STOKES subtracts, thresholded and cleaned up, is a highlight mask of ONE sample that needs no label.  Three calls on one
 * stream make it; none synchronises with the host, the threshold travels in device memory (stats).
 *   stats   device int[3]: [0] Otsu's t, [1] the threshold applied t_eff, [2] the number of set mask pixels
 * Strength and histogram.  src_ptrs: host array of 4 device pointers to contiguous uint8 [h,w,3] views; coef: host float[12], the 3x4
 * Stokes matrix of shm_polar_views_u8 (rows 1 and 2 are read).  Per pixel, with S1_c = ((C10 v0 + C11 v1) + C12 v2) + C13 v3 of channel c
 * and S2_c alike from row 2, all in fp32:
 *   e = max_c (S1_c^2 + S2_c^2);  p = sqrtf(e);  q = min(255, (int)p)        q: device uint8 [h,w]
 * The maximum is taken BEFORE the root: for integer matrices e is an exact integer below 2^24 and q its integer square root.
 * hist: device unsigned[256], cleared on the stream by the call and then holding exactly the counts of q (integer atomics: the same
 * on every run).  SHM_E_SHAPE for a null pointer, h or w below 1, or h * w * 3 beyond the 32-bit index range; before any launch. */
int shm_specmask_strength(const unsigned char* const* src_ptrs, int h, int w, const float* coef, unsigned char* q,
                          unsigned* hist, void* stream);
/* Otsu's threshold of a 256-bin histogram (device unsigned[256]; one block).  With bins <= t as class 0: N0(t), M0(t) the exact 64-bit
 * prefix counts and first moments, N1 = N - N0, M1 = M - M0, and in double
 *   var(t) = ((N0 * N1) * d) * d,  d = M1 / N1 - M0 / N0;   var(t) = 0 where a class is empty
 * stats[0] = the lowest t of maximal var(t) (0 for an empty or one-bin histogram); stats[1] = fixed_t when fixed_t >= 0, else
 * max(stats[0], floor_t): Otsu splits anything, sensor noise included, and the floor keeps such a split from becoming a mask.
 * SHM_E_SHAPE for a null pointer, floor_t outside [0, 255] or fixed_t outside [-1, 255]. */
int shm_specmask_otsu(const unsigned* hist, int floor_t, int fixed_t, int* stats, void* stream);
/* b = q > stats[1] (read on the device), opened with a (2 open_radius + 1)^2 square (erosion, then dilation) and dilated with a
 * (2 dilate_radius + 1)^2 square; a tap outside the image is skipped (the min / max runs over the taps inside it); radius 0 is the
 * identity.  Two launches: threshold + erosion into tmp (device uint8 [h,w], 0 / 1, a buffer of its own), then one dilation by
 * open_radius + dilate_radius into mask (device uint8 [h,w], 0 / 255), which also counts the set pixels into stats[2] (cleared on
 * the stream by the call).  SHM_E_SHAPE for a null pointer, tmp aliasing q or mask, sizes as above, open_radius outside
 * [0, SHM_SPECMASK_MAX_OPEN] or dilate_radius outside [0, SHM_SPECMASK_MAX_DILATE]; before any launch. */
#define SHM_SPECMASK_MAX_OPEN 4
#define SHM_SPECMASK_MAX_DILATE 8
int shm_specmask_morph(const unsigned char* q, int h, int w, int open_radius, int dilate_radius, unsigned char* tmp,
                       unsigned char* mask, int* stats, void* stream);
/* The chain: shm_specmask_strength, shm_specmask_otsu and shm_specmask_morph on `stream`, with every refusal of the three (and
 * mask sharing q's buffer) made before the first launch; four launches and two small clears, no host synchronisation.  q, hist and
 * stats are results like mask; tmp is scratch. */
int shm_specmask(const unsigned char* const* src_ptrs, int h, int w, const float* coef, int floor_t, int fixed_t,
                 int open_radius, int dilate_radius, unsigned char* q, unsigned* hist, unsigned char* tmp,
                 unsigned char* mask, int* stats, void* stream);

/* ---- test-mode image export (the images test.py:305-317 logs; test_plot at test.py:410-425) ----------------------------
 * Batched, ragged float32 -> uint8 export.  One job = one plane of one image: source src[j], float32 [s,s,c] NHWC with channel
 * pitch ld >= c, c in {1,3}; destination [ho,wo,c] uint8, tightly packed, at byte offset dst_off (a multiple of 4) of dst.
 * desc holds SHM_EXPORT_DESC size_t per job: {s, c, ld, ho, wo, mode, k, dst_off}.  src and desc are host arrays of up to
 * SHM_EXPORT_MAX_JOBS jobs, read during the call.  Per output byte of channel ch at (oy, ox):
 *   v  (ho,wo) = (s,s): the source value at (oy, ox, ch).  Otherwise tf.image.resize(bilinear, half-pixel centres, no
 *      antialias), the mapping of shm_resize_bilinear_u8, in fp32 on the raw values: fy = (oy + 0.5) s/ho - 0.5,
 *      y0 = max(floor(fy), 0), y1 = min(ceil(fy), s-1), ly = fy - floor(fy) (x alike); top = tl + (tr - tl) lx,
 *      bot = bl + (br - bl) lx, v = top + (bot - top) ly
 *   t  SHM_EXPORT_RESCALE: (v - min) / (max - min), min and max over the whole s*s*c source plane, 0 when max == min
 *      (rescale_01, utils.py:190-195, divide_no_nan);  SHM_EXPORT_SCALE: v * mul[k] (mul: device float[nmul]; with mul the
 *      running mean of shm_running_scale_mean this is gen_rgb_output / 255 of test.py:246-250);  SHM_EXPORT_CLIP: v
 *   q  rint(clamp(t, 0, 1) * 255) in fp32, round half to even; a NaN t gives 0
 * At most two launches: a min / max pass (only if some job is RESCALE) and the export pass.  A job's bytes depend on that job
 * alone (not on the other jobs, their order or the launch geometry).  ws: shm_export_u8_workspace(njobs) bytes, 4-byte
 * aligned, no initial contents; dst 4-byte aligned.  SHM_E_SHAPE for njobs outside [1, SHM_EXPORT_MAX_JOBS], a null pointer,
 * c, ld, a size outside [1, 32768], an unknown mode, k >= nmul, a destination outside [0, dst_bytes); SHM_E_WORKSPACE for a
 * short workspace; all before any launch. */
#define SHM_EXPORT_RESCALE 0
#define SHM_EXPORT_SCALE 1
#define SHM_EXPORT_CLIP 2
#define SHM_EXPORT_DESC 8
#define SHM_EXPORT_MAX_JOBS 64
size_t shm_export_u8_workspace(int njobs);
int shm_export_u8(const float* const* src, const size_t* desc, int njobs, const float* mul, int nmul, unsigned char* dst,
                  size_t dst_bytes, void* ws, size_t ws_bytes, void* stream);
/* The job model of shm_export_u8 with a rectangular source and a source window (native-resolution test mode: the photo inside its
 * padded frame).  desc holds SHM_EXPORT_HW_DESC size_t per job: {hs, ws, c, ld, y0, x0, hc, wc, ho, wo, mode, k, dst_off}: source
 * src[j] float32 [hs,ws,c] with channel pitch ld, the window of hc x wc pixels at (y0, x0), destination [ho,wo,c].  RESCALE takes
 * min and max over the window; the resampling maps the window to (ho,wo) (fy = (oy + 0.5) hc/ho - 0.5 clamped to the window's
 * rows, x alike); (ho,wo) = (hc,wc) copies.  Nothing outside the window is read.  Value maps, quantisation, workspace
 * (shm_export_u8_workspace) and argument checks as in shm_export_u8, plus SHM_E_SHAPE for a window outside the source. */
#define SHM_EXPORT_HW_DESC 13
int shm_export_u8_hw(const float* const* src, const size_t* desc, int njobs, const float* mul, int nmul, unsigned char* dst,
                     size_t dst_bytes, void* ws, size_t ws_bytes, void* stream);
/* The reference's running mean of the standardisation scales (test.py:77, 218, 246: stddev_arr is reset once per test run and
 * grows by one entry per image; each image uses the mean of every scale so far, its own included).  acc = caller-owned device
 * f64 {sum, count} ({0, 0} at the start of a run).  In image order, one thread: sum += scale[b], count += 1,
 * mul[b] = (float)(sum / count); acc is updated.  One block, deterministic. */
int shm_running_scale_mean(const float* scale, int batch, double* acc, float* mul, void* stream);

/* ---- full-resolution test output: guided detail transfer (csrc/detail.hip) -------------------------------
 * The generator changes one plane, the standardised Y, at model resolution.  The change is fitted locally against the Y it was fed
 * (the fast guided filter of He & Sun with the correction as the target), the fit's two coefficients are upsampled and applied to
 * the photo's own Y at the photo's own size.
 * shm_detail_coeffs.  Per image two planes [h,w]: I = guide (pixel pitch ldg: channel 0 of the standardised YUV has pitch 3),
 * p = target (pitch ldt), images h*w pixels apart; d = p - I.  box_r(x)[y][x] = the mean of x over the part of the
 * (2 radius + 1)^2 window around (y, x) that lies inside the plane, divided by that part's own count (no padding):
 *   var = box(I I) - box(I)^2      cov = box(I d) - box(I) box(d)      a = cov / (var + eps)      b = box(d) - a box(I)
 *   coef[b][y][x] = (box(a), box(b)), interleaved float32 [batch,h,w,2]
 * all in fp32.  var and cov are formed from I - c, c a block-uniform reference value near I's local mean (both are shift-invariant;
 * Y is not mean-free), and c is added back in b; d is not shifted, so that radius 0 gives (0, d) with d = p - I bit for bit: the
 * plain residual transfer is this call at radius 0.  A window that holds a NaN or an Inf (in I or p) gives NaN a and b, whatever c
 * is.  A window's sum runs over that window's elements alone in a fixed order (rows, then columns; no running sums), so one NaN
 * spreads to the (4 radius + 1)^2 coefficients whose fit could see it and no further.  One launch, no atomics: an image's
 * coefficients do not depend on the batch, and are bitwise the same from run to run.  A plane smaller than the window is legal
 * (every window is then the whole plane).  SHM_E_SHAPE before any launch, with a message that names the argument: a null pointer,
 * radius outside [0, 8], eps not a positive finite number, batch outside [1, 65535], h or w outside [1, 32768], a pitch below 1,
 * coef not 8-byte aligned.
 * shm_detail_apply_u8.  photo uint8 [h,w,3] (any ratio to the coefficients' H x W, larger or smaller), coef float32 [H,W,2] of
 * one image, scale = device pointer to that image's standardisation scale (shm_rgb2yuv_std's scale_out[b]; read on the device).
 * Per photo pixel (oy, ox), in fp32:
 *   (y, u, v) = rgb_to_yuv(byte * (1/255)) * (1 / scale)                           constants and order of shm_rgb2yuv_std (which
 *               divides by scale: the two agree to an ulp)
 *   (a', b')  = the sample of coef at (oy, ox): the taps and the lerp of shm_resize_bilinear_u8 (csrc/bilinear.h) with
 *               scales H/h and W/w, on each of the two coefficients; (h,w) = (H,W) reads the coefficient itself
 *   Y' = y + (a' y + b');   out[oy][ox] = yuv_to_rgb(Y', u, v) = (Y' + 1.13988303 v, Y' - 0.394642334 u - 0.58062185 v,
 *   Y' + 2.03206185 u)                                                             float32 [h,w,3], the units of shm_yuv2rgb
 * One launch over the flat photo, four pixels per lane, 64-bit element offsets; 3 bytes read and 12 written per pixel.
 * SHM_E_SHAPE before any launch: a null pointer, a side of the photo or of coef outside [1, 32768], photo not 4-byte, coef not
 * 8-byte or out not 16-byte aligned.  Neither call allocates. */
int shm_detail_coeffs(const float* guide, int ldg, const float* target, int ldt, float* coef, int batch, int h, int w, int radius,
                      float eps, void* stream);
int shm_detail_apply_u8(const unsigned char* photo, int h, int w, const float* coef, int hm, int wm, const float* scale,
                        float* out, void* stream);

/* ---- optimizer (SHM.py:169-175, 859-872) ------------------------------------------
 * tf.clip_by_value(g,-1,1) + Keras adam_v2.Adam: m += (g-m)(1-b1); v += (g^2-v)(1-b2);
 * w -= alpha * m / (sqrt(v) + eps); alpha = lr_t*sqrt(1-b2^t)/(1-b1^t) computed by the caller.
 * gscale multiplies g before the clip (1/world_size for data parallel).  abort_word (may be NULL): the device abort word of the
 * step's shm_in_bwd calls; the kernel checks it first and leaves w, m, v untouched while it is non-zero. */
int shm_adam_clip(float* w, float* m, float* v, const float* g, size_t n, float alpha, float beta1,
                  float beta2, float eps, float gscale, const unsigned* abort_word, void* stream);
/* Exponential moving average of a flat fp32 weight buffer (the trainer's `ema_decay`: the generator weights one evaluates with), in
 * place, one launch.  Per element, all in fp32 and in exactly this form, so that a float64 restatement can bound it:
 *   om = 1.0f - decay;   t = w[i] - ema[i];   ema[i] = fmaf(om, t, ema[i])          (one rounding of t, one of the fused multiply-add)
 * decay == 0 is a plain copy, ema[i] = w[i] bit for bit: how the average is initialised.  A non-finite w[i] propagates into ema[i]
 * and stays there (NaN for good, Inf until decay == 0 copies over it): the kernel does not look for them, the trainer's `nonfinite`
 * option is the detector.  abort_word (may be NULL) as in shm_adam_clip: one relaxed agent-scope load at kernel entry, nothing is
 * written while the word is non-zero -- the step whose weights were not updated does not move the average either.
 * ema and w are device float32 [n], 4-byte aligned (slices of flat buffers) and must not overlap.  With the same misalignment to 16
 * bytes on both, the (< 4) elements in front of the first boundary and behind the last whole vector go one per lane and the rest 16
 * bytes per lane; otherwise 4-byte lanes (same values).  256-thread blocks, a grid-stride loop under SHM_EMA_MAX_BLOCKS blocks; no
 * LDS, no atomics: results are bitwise the same from run to run.  12 bytes of traffic per element (8 for decay == 0).
 * SHM_E_SHAPE, before any launch, with a message that names the argument: decay NaN, < 0 or >= 1 (for any n); with n > 0 a null ema
 * or w, overlapping [ema, ema + n) and [w, w + n), or a pointer that is not 4-byte aligned.  n == 0 is SHM_OK without a launch. */
#define SHM_EMA_MAX_BLOCKS 8192
int shm_ema_update(float* ema, const float* w, size_t n, float decay, const unsigned* abort_word, void* stream);

/* ---- training telemetry (the reference logs its loss scalars every 25 steps, SHM.py:1035-1053, and a histogram of every clipped
 * gradient tensor every 100, SHM.py:1085-1091) --------------------------------------------------------------------------------
 * Segmented statistics of a flat fp32 device buffer x of n floats (P.grad or P.flat of a model).  Segment s is
 * x[seg_off[s] : seg_off[s] + seg_len[s]], one variable; seg_off and seg_len are host arrays of nseg <= SHM_TSTAT_MAX_SEGS entries
 * read during the call.  Segments must not overlap (the workspace size assumes it), need not be sorted and need not cover x; an
 * empty segment gives zeros.  Every value is first scaled as shm_adam_clip scales it, v = x[i] * scale in one fp32 multiply
 * (denormals kept), so with scale = 1 / world v is the value the optimizer clips.  Per segment:
 *   stats[s][SHM_TSTAT_N] (f64): SHM_TSTAT_FINITE count of finite v, _NAN count of NaN, _INF count of +-Inf, _MIN / _MAX over the
 *     finite v (0 when there is none), _SUM / _SUMSQ of the finite v accumulated in f64, _CLIPPED count of finite |v| > 1 (the
 *     values tf.clip_by_value(g, -1, 1) moves)
 *   hist[s][2][SHM_THIST_BINS] (u64): counts by sign bit and magnitude class.  The class comes from the bits of v; E = its biased
 *     exponent field:
 *       0          E == 0: zeros and subnormals, under sign 0 whatever the sign bit (a flush-to-zero multiply cannot move a value)
 *       1          normal, |v| < 2^SHM_THIST_EMIN
 *       2 .. 41    floor(log2 |v|) = e for e in [SHM_THIST_EMIN, -1]: class e - SHM_THIST_EMIN + 2
 *       42         finite |v| >= 1; with _CLIPPED this gives the histogram AFTER the clip exactly (these values land on +-1)
 *       43         NaN and Inf, under sign 0
 * Two launches whatever nseg is: a pass over fixed-size chunks cut relative to each segment's start (bin counts aggregated per
 * block in LDS; no global atomics) and a per-segment finalize that adds the chunk partials, the f64 sums in chunk order.  A
 * segment's results are bitwise the same from run to run and depend on that segment alone (not on the other segments or their
 * order).  x is only read.  ws: shm_tensor_stats_workspace(nseg, n) bytes (enough for any nseg disjoint segments of [0, n)),
 * 16-byte aligned, no initial contents.  SHM_E_SHAPE for nseg outside [1, SHM_TSTAT_MAX_SEGS], a null pointer, a segment outside
 * [0, n); SHM_E_WORKSPACE for a short workspace; both before any launch. */
#define SHM_TSTAT_N 8
#define SHM_TSTAT_FINITE 0
#define SHM_TSTAT_NAN 1
#define SHM_TSTAT_INF 2
#define SHM_TSTAT_MIN 3
#define SHM_TSTAT_MAX 4
#define SHM_TSTAT_SUM 5
#define SHM_TSTAT_SUMSQ 6
#define SHM_TSTAT_CLIPPED 7
#define SHM_THIST_BINS 44
#define SHM_THIST_EMIN (-40)
#define SHM_TSTAT_MAX_SEGS 128
size_t shm_tensor_stats_workspace(int nseg, size_t n);
int shm_tensor_stats(const float* x, size_t n, const size_t* seg_off, const size_t* seg_len, int nseg, float scale,
                     double* stats, unsigned long long* hist, void* ws, size_t ws_bytes, void* stream);
/* One step's raw loss sums into row `row` of a device ring of f64 [rows][SHM_LOSS_ROW], one tiny launch, no host sync:
 * {dl[SHM_LOSS_ROW_DL] (shm_dhead_losses), il[SHM_LOSS_ROW_IL] (shm_image_losses), sl[SHM_LOSS_ROW_SL] (shm_spec_loss), step,
 * abort word}, the last two as f64.  abort_word: the device abort word of shm_in_bwd / shm_adam_clip (u32) or null (stored as 0).  The caller
 * chooses the row (the n-th logged step goes to row n % rows) and copies the ring out before a row comes round again. */
#define SHM_LOSS_ROW_DL 16
#define SHM_LOSS_ROW_IL 32
#define SHM_LOSS_ROW_SL 5
#define SHM_LOSS_ROW_STEP 53
#define SHM_LOSS_ROW_ABORT 54
#define SHM_LOSS_ROW 56
int shm_loss_ring_put(const double* dl, const double* il, const double* sl, const void* abort_word, double* ring, int rows,
                      int row, long long step, void* stream);

/* ---- training the SpecSeg mask network (specseg_train.hip) -----------------------------------------------------------------------
 * The reference builds SpecSeg's optimiser (SHM.py:175) and a Dice + focal loss with IoU / F-score metrics (SpecSeg.py:92-96) and
 * runs neither; its checkpoint is not available, so the weights are made here.  fp32 tensors only.  The 3x3 convolutions' gradients
 * are shm_conv2d_dgrad / shm_conv2d_wgrad, ReLU's is shm_lrelu_bwd at slope 0, Dropout is shm_keep_mask / shm_mul_mask.  Every
 * reduction below keeps f64 partial sums in a workspace slot per block and adds the slots in a fixed order: no global atomics, results
 * bitwise the same from run to run.  Workspaces need no initial contents and are 16-byte aligned.  All shape errors are SHM_E_SHAPE
 * and a short workspace SHM_E_WORKSPACE, before any launch. */
#define SHM_SST_MAX_BLOCKS 256
/* f64 elements of the workspace of shm_bn_train_fwd / shm_bn_train_bwd / shm_head_logit_bwd on c channels */
#define SHM_BN_TRAIN_WS_DOUBLES(c) ((size_t)SHM_SST_MAX_BLOCKS * 2 * (c) + 2 * (size_t)(c))
/* Keras BatchNormalization(axis=-1) in training mode over the npix = N*H*W pixels of a [npix, c] (pitch lda): per channel
 * mean and the biased variance var, in two passes (sum, then sum of squared deviations from the f64 mean: data with |mean| >> std
 * does not cancel); out = (a - mean) * gamma / sqrt(var + eps) + beta.  save (f64 [2c]) receives mean [c] and 1 / sqrt(var + eps) [c]
 * for the backward.  moving_mean / moving_var (may be NULL) are updated in place: moving = moving * momentum + value * (1 - momentum),
 * where the variance's value is the unbiased estimate var * npix / max(npix - 1, 1) (TensorFlow's fused kernel).  c a power of two
 * in 16..256, pitches multiples of 4. */
int shm_bn_train_fwd(const float* a, int lda, const float* gamma, const float* beta, float* moving_mean, float* moving_var,
                     float momentum, float eps, float* out, int ldo, double* save, double* ws, size_t ws_bytes, size_t npix, int c,
                     void* stream);
/* Its backward, with xhat = (a - mean) * inv_std from `save`: dbeta = sum dy, dgamma = sum dy * xhat (both overwritten),
 * dx = gamma * inv_std * (dy - mean(dy) - xhat * mean(dy * xhat)).  dx may be dy when their pitches agree. */
int shm_bn_train_bwd(const float* dy, int lddy, const float* a, int lda, const float* gamma, const double* save, float* dx, int lddx,
                     float* dgamma, float* dbeta, double* ws, size_t ws_bytes, size_t npix, int c, void* stream);
/* MaxPooling2D((2,2)) backward on even sizes: x [batch,h,w,c] is the pool's input, dy [batch,h/2,w/2,c] its output gradient.  The
 * gradient of each window goes to the window's FIRST maximum in row-major order ((0,0), (0,1), (1,0), (1,1)), recomputed from x;
 * the other three positions get 0.  accumulate != 0: dx += (the skip gradient is already there), else dx is overwritten. */
int shm_maxpool2_bwd(const float* x, int ldx, const float* dy, int lddy, float* dx, int lddx, int batch, int h, int w, int c,
                     int accumulate, void* stream);
/* Conv2DTranspose(k=2, strides=2) backward; w = Keras layout [2][2][cout][cin] as stored, dy [batch,2hi,2wi,cout], x and dx
 * [batch,hi,wi,cin]; cout a multiple of 16, cin a multiple of 32, any hi, wi >= 1.  v_mfma_f32_16x16x4_f32 GEMMs, LDS-staged.
 *   dgrad  dx[a,b,ci] = sum_{p,q,co} dy[2a+p,2b+q,co] * w[p,q,co,ci]
 *   wgrad  dw[p,q,co,ci] = sum_{n,a,b} dy[n,2a+p,2b+q,co] * x[n,a,b,ci] (split over the pixels, the splits added in split order);
 *          dbias[co] (may be NULL; cout a power of two in 16..256) = sum over every pixel of dy.  Both overwritten. */
int shm_conv2d_transpose2x2_dgrad(const float* dy, int lddy, const float* w, float* dx, int lddx, int batch, int hi, int wi,
                                  int cin, int cout, void* stream);
size_t shm_conv2d_transpose2x2_wgrad_workspace(int batch, int hi, int wi, int cin, int cout);
int shm_conv2d_transpose2x2_wgrad(const float* x, int ldx, const float* dy, int lddy, float* dw, float* dbias, void* ws,
                                  size_t ws_bytes, int batch, int hi, int wi, int cin, int cout, void* stream);
/* The head Conv2D(1, (1,1)) without its sigmoid: z[p] = sum_c x[p,c] w[c] + bias (shm_head_sigmoid_fwd stays what predict uses). */
int shm_head_logit_fwd(const float* x, int ldx, const float* w, const float* bias, float* z, size_t npix, int c, void* stream);
/* Its backward: dx[p,c] = dz[p] w[c], dw[c] = sum_p dz[p] x[p,c], db = sum_p dz[p] (all overwritten);
 * ws = SHM_BN_TRAIN_WS_DOUBLES(c) f64. */
int shm_head_logit_bwd(const float* x, int ldx, const float* w, const float* dz, float* dx, int lddx, float* dw, float* db,
                       double* ws, size_t ws_bytes, size_t npix, int c, void* stream);
/* Dice + binary focal loss of the logits z [npix] against the target g [npix] in [0, 1], over the whole batch, p = sigmoid(z):
 *   dice  = 1 - (2 sum(g p) + s) / (sum(p) + sum(g) + s),  s = 1e-5
 *   focal = mean(-g 0.25 (1-p)^2 log p - (1-g) 0.75 p^2 log(1-p)),  log p = -softplus(-z), log(1-p) = -softplus(z)
 *   tp = sum g [z > 0], fp = sum (1-g) [z > 0], fn = sum g [z <= 0]  (p > 0.5 <=> z > 0);
 *   iou = (tp + s) / (tp + fp + fn + s), f1 = (2 tp + s) / (2 tp + fp + fn + s)
 * out (f64 [SHM_SEG_LOSS_OUT]) = {dice + focal, dice, focal, iou, f1, tp, fp, fn}; dz (may be NULL: evaluation) = d(dice + focal)/dz.
 * Per-pixel arithmetic in f64: finite values and gradients at |z| = 40.  ws = SHM_SEG_LOSS_WS_DOUBLES f64. */
#define SHM_SEG_LOSS_OUT 8
#define SHM_SEG_LOSS_WS_DOUBLES ((size_t)SHM_SST_MAX_BLOCKS * 7 + 8)
int shm_seg_loss(const float* z, const float* g, float* dz, double* out, double* ws, size_t ws_bytes, size_t npix, void* stream);
/* shm_adam_clip's kernel with the clip bound as an argument (clip <= 0: no clip) and no abort word. */
int shm_adam(float* w, float* m, float* v, const float* g, size_t n, float alpha, float beta1, float beta2, float eps,
             float gscale, float clip, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SHMGAN_HIP_H */
