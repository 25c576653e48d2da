// Image-quality metrics of the reference's test mode (test.py:332-392, `--calc_metrics True`):
// per image, from gen_rgb (the G1 output in RGB, NOT clipped) against the diffuse target, both [B,S,S,3] fp32.
// Every sample is an independent B=1 reference call.
//
//   MSE    test.py:346-347 (Keras MeanSquaredError): mean over H*W*3 of (g-t)^2
//   PSNR   test.py:338-342 (tf.image.psnr, max_val 1; convert_image_dtype f32->f32 is the identity): -10 log10(MSE), +inf at MSE 0
//   SSIM   test.py:336 tf.image.ssim(rescale_01(g), rescale_01(t), 5): the loss's SSIM (11-tap gaussian, sigma 1.5, VALID,
//          k1 0.01, k2 0.03, max_val 5, mean over HO*WO*3); rescale_01 (utils.py:190-195) takes min/max over the whole image,
//          all three channels, with divide_no_nan (a constant image becomes 0)
//   dE76   test.py:351-353 (tfio rgb_to_lab, skimage deltaE_cie76): mean over pixels of |Lab(g) - Lab(t)|_2
//   dE94   test.py:354 (skimage deltaE_ciede94, kL = kC = kH = 1, k1 0.045, k2 0.015): mean over pixels of
//          sqrt(max(dL^2 + (dC / (1 + k1 C1))^2 + dH^2 / (1 + k2 C1)^2, 0)), C = hypot(a, b), dH^2 = 2 (C1 C2 - a1 a2 - b1 b2),
//          C1 of the GENERATED image (the metric is asymmetric)
//
// Lab: tfio's rgb_to_lab (D65, 2 degree observer), restated here because neither tfio nor skimage is part of this project: the
// constants below are our restatement, like the rest of the oracle (oracle/, tests/test_eval_cpu.py).  Both branches of tfio's
// tf.where are evaluated there, but a NaN of the branch not chosen never reaches the result: here they are selects as well.
//
// Reproducibility: results are bitwise reproducible and batch-invariant.  The grid per image depends on S only, every block writes
// its partial into a workspace slot of its own, and the partials are reduced in a fixed slot order (no atomics anywhere).
//   pixel pass  grid (NP, B): sums of (g-t)^2, dE76, dE94 (per-thread fp32, per-block f64) and min / max of g and of t
//   ssim pass   grid (tiles, B, 3): reduces the min / max partials, stages the 26x26 halo of one 16x16 output tile in LDS, separable
//               11-tap gaussian (as ssim_fwd_kernel of imgloss.hip, without the gradient maps), one f64 partial per block
//   finalize    grid (B): out[b][5] = {mse, psnr, ssim, de76, de94} (f64)
//
// shm_image_metrics_hw is the same three kernels on a window (top, left, h, w) of a padded prediction [B,Hp,Wp,3] against a tight
// target [B,h,w,3] (native-resolution test mode): every sum, the min / max and the SSIM run over the window's pixels only, in the
// window's own row-major order -- nothing outside the window is read.  The square call is the window (0, 0, s, s) of an s x s frame.
//
// shm_image_metrics_region_hw is the REGION = true instantiation of the same three kernels: a uint8 [B,h,w] region splits every sum
// into the pixels (SSIM positions: by their centre pixel) inside it and the ones outside -- a second set of sums in the same loop,
// block and slot order, a select of which sums a pixel or position is added to -- plus exact counts.  Both instantiations run the same
// instructions per pixel (pixel_step), so with the region all ones the "in" sums ARE the whole-window sums, bit for bit; the min / max
// of rescale_01 stay those of the whole window.  An empty set gives NaN (finish5).
// shm_highlight_region_hw builds such a region in one launch: src - target above tau in any channel, or a plane above tau.
#include "common.h"

#include <math.h>

namespace {

constexpr int MWIN = SHM_SSIM_WIN;
constexpr int MTILE = 16;
constexpr int MHALO = MTILE + MWIN - 1;     // 26
constexpr int NT = 256;                     // threads per block, all three kernels

// the window of the prediction frame the metrics are taken on: frame pitch pw (pixels per row), origin (top, left), size h x w
struct MetricWin {
    int pw, top, left, h, w;
};

// blocks per image of the pixel pass: a function of the window's size alone (batch invariance)
int pixel_blocks(int h, int w) {
    int n = shm_cdiv((long)h * w, 4 * NT);
    return n > 256 ? 256 : n;
}

int ssim_tiles(int h, int w) {
    return shm_cdiv(h - MWIN + 1, MTILE) * shm_cdiv(w - MWIN + 1, MTILE);
}

struct MetricWs {
    size_t pix, mm, ssim, total;
};

size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }

// doubles per workspace slot.  Plain: {sq, e76, e94} per pixel block and one SSIM sum per tile block.  With a region: the three
// sums inside, the three outside and the pixels inside; the SSIM sum inside, outside and the positions inside
template <bool REGION>
struct Slots {
    static constexpr int SETS = REGION ? 2 : 1, PIX = REGION ? 7 : 3, SSIM = REGION ? 3 : 1;
};

template <bool REGION>
MetricWs plan_metric_ws(int batch, int h, int wd) {
    MetricWs w;
    size_t off = 0;
    w.pix = off;  off = align256(off + (size_t)batch * pixel_blocks(h, wd) * Slots<REGION>::PIX * sizeof(double));
    w.mm = off;   off = align256(off + (size_t)batch * pixel_blocks(h, wd) * 4 * sizeof(float));
    w.ssim = off; off = align256(off + (size_t)batch * 3 * ssim_tiles(h, wd) * Slots<REGION>::SSIM * sizeof(double));
    w.total = off;
    return w;
}

// ---- tfio rgb_to_lab (D65, 2 degree observer), restated
__device__ __forceinline__ float srgb_linear(float x) {
    const float hi = powf((x + 0.055f) / 1.055f, 2.4f);     // NaN for x < -0.055: never selected
    const float lo = x / 12.92f;
    return x > 0.04045f ? hi : lo;
}

__device__ __forceinline__ float lab_f(float v) {
    const float hi = cbrtf(v), lo = 7.787f * v + 16.0f / 116.0f;
    return v > 0.008856f ? hi : lo;
}

__device__ __forceinline__ void rgb_to_lab(float r, float g, float b, float& L, float& A, float& Bc) {
    r = srgb_linear(r);
    g = srgb_linear(g);
    b = srgb_linear(b);
    const float x = (0.412453f * r + 0.357580f * g + 0.180423f * b) / 0.95047f;
    const float y = (0.212671f * r + 0.715160f * g + 0.072169f * b) / 1.0f;
    const float z = (0.019334f * r + 0.119193f * g + 0.950227f * b) / 1.08883f;
    const float fx = lab_f(x), fy = lab_f(y), fz = lab_f(z);
    L = 116.0f * fy - 16.0f;
    A = 500.0f * (fx - fy);
    Bc = 200.0f * (fy - fz);
}

// ---------------------------------------------------------------------------------- pixel pass
// a thread's running sums of (g-t)^2, dE76 and dE94
struct PixelSums {
    float sq, e76, e94;
};

// `acc` plus one pixel's three terms.  Not inlined on purpose: the plain and the region kernel then run the very same instructions for a
// pixel.  Inlined, the compiler fuses and pairs the products of this arithmetic differently in the two kernels (it depends on the code
// around it), and a full region's sums would differ from the plain ones in their last bits
__device__ __noinline__ PixelSums pixel_step(PixelSums acc, float g0, float g1, float g2, float t0, float t1, float t2) {
    const float d0 = g0 - t0, d1 = g1 - t1, d2 = g2 - t2;
    acc.sq += d0 * d0 + d1 * d1 + d2 * d2;
    float L1, a1, b1, L2, a2, b2;
    rgb_to_lab(g0, g1, g2, L1, a1, b1);
    rgb_to_lab(t0, t1, t2, L2, a2, b2);
    const float dL = L1 - L2, da = a1 - a2, db = b1 - b2;
    acc.e76 += sqrtf(dL * dL + da * da + db * db);
    // skimage's dH^2 = 2 (C1 C2 - a1 a2 - b1 b2) cancels for near-identical colours: evaluated in f64 from the fp32 Lab values
    const double A1 = a1, B1 = b1, A2 = a2, B2 = b2;
    const double C1 = sqrt(A1 * A1 + B1 * B1), C2 = sqrt(A2 * A2 + B2 * B2);
    const double dH2 = 2.0 * (C1 * C2 - A1 * A2 - B1 * B2);
    const double sc = 1.0 + 0.045 * C1, sh = 1.0 + 0.015 * C1, dC = C1 - C2;
    const double e2 = (double)dL * dL + (dC / sc) * (dC / sc) + dH2 / (sh * sh);
    acc.e94 += (float)sqrt(e2 > 0.0 ? e2 : 0.0);
    return acc;
}

// grid (NP, B); pix[b][blk][3] = partial sums of (g-t)^2, dE76, dE94; mm[b][blk][4] = min g, max g, min t, max t
// REGION: pix[b][blk][7] = the three sums over the block's pixels inside the region, the three outside, the number inside; mm unchanged
template <bool REGION>
__global__ __launch_bounds__(NT) void metrics_pixel_kernel(const float* __restrict__ g, const float* __restrict__ t,
                                                          const unsigned char* __restrict__ region, double* __restrict__ pix,
                                                          float* __restrict__ mm, const MetricWin win, size_t frame) {
    constexpr int SETS = Slots<REGION>::SETS, PIX = Slots<REGION>::PIX;
    const int b = blockIdx.y, np = gridDim.x;
    const size_t npix = (size_t)win.h * win.w;
    const float* gi = g + ((size_t)b * frame + (size_t)win.top * win.pw + win.left) * 3;      // the window's first pixel
    const float* ti = t + (size_t)b * npix * 3;
    PixelSums acc[SETS] = {};                                // [0]: the whole window, or inside the region; [1]: outside it
    unsigned nin = 0;                                        // this thread's pixels inside (at most 2^30 / NT)
    float gmn = INFINITY, gmx = -INFINITY, tmn = INFINITY, tmx = -INFINITY;
    for (size_t p = (size_t)blockIdx.x * NT + threadIdx.x; p < npix; p += (size_t)np * NT) {
        // p in the frame's pitch: p itself when the window spans whole rows (always in the square call); otherwise one 32-bit
        // division (a padded frame has sides <= 32768: p < 2^30)
        size_t gp = p;
        if (win.pw != win.w) {
            const unsigned y = (unsigned)p / (unsigned)win.w;
            gp = (size_t)y * win.pw + ((unsigned)p - y * (unsigned)win.w);
        }
        const float g0 = gi[gp * 3], g1 = gi[gp * 3 + 1], g2 = gi[gp * 3 + 2];
        const float t0 = ti[p * 3], t1 = ti[p * 3 + 1], t2 = ti[p * 3 + 2];
        gmn = fminf(gmn, fminf(g0, fminf(g1, g2)));
        gmx = fmaxf(gmx, fmaxf(g0, fmaxf(g1, g2)));
        tmn = fminf(tmn, fminf(t0, fminf(t1, t2)));
        tmx = fmaxf(tmx, fmaxf(t0, fmaxf(t1, t2)));
        if constexpr (REGION) {
            // the pixel's side picks the sums it is added to (selects of whole sums: a NaN or Inf on one side never reaches the other)
            const bool in = region[(size_t)b * npix + p] != 0;
            nin += in;
            const PixelSums u = pixel_step(in ? acc[0] : acc[1], g0, g1, g2, t0, t1, t2);
            acc[0] = in ? u : acc[0];
            acc[1] = in ? acc[1] : u;
        } else {
            acc[0] = pixel_step(acc[0], g0, g1, g2, t0, t1, t2);
        }
    }
    double s[PIX];
    for (int k = 0; k < SETS; ++k) {
        s[3 * k] = shm_block_sum<NT>((double)acc[k].sq);
        s[3 * k + 1] = shm_block_sum<NT>((double)acc[k].e76);
        s[3 * k + 2] = shm_block_sum<NT>((double)acc[k].e94);
    }
    if constexpr (REGION) s[6] = shm_block_sum<NT>((double)nin);      // integers below 2^53: exact in any order
    gmn = shm_wave_min(gmn);
    gmx = shm_wave_max(gmx);
    tmn = shm_wave_min(tmn);
    tmx = shm_wave_max(tmx);
    __shared__ float wmm[NT / 64][4];
    if ((threadIdx.x & 63) == 0) {
        wmm[threadIdx.x >> 6][0] = gmn;
        wmm[threadIdx.x >> 6][1] = gmx;
        wmm[threadIdx.x >> 6][2] = tmn;
        wmm[threadIdx.x >> 6][3] = tmx;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const size_t slot = (size_t)b * np + blockIdx.x;
        for (int k = 0; k < PIX; ++k) pix[slot * PIX + k] = s[k];
        float r[4] = {wmm[0][0], wmm[0][1], wmm[0][2], wmm[0][3]};
        for (int w = 1; w < NT / 64; ++w) {
            r[0] = fminf(r[0], wmm[w][0]);
            r[1] = fmaxf(r[1], wmm[w][1]);
            r[2] = fminf(r[2], wmm[w][2]);
            r[3] = fmaxf(r[3], wmm[w][3]);
        }
        for (int k = 0; k < 4; ++k) mm[slot * 4 + k] = r[k];
    }
}

// ----------------------------------------------------------------------------------- ssim pass
// grid (tiles, B, 3); ssim[b][c][tile] = sum over the tile's valid outputs of luminance * contrast-structure
// REGION: ssim[b][c][tile][3] = that sum over the outputs whose centre pixel (oy + 5, ox + 5) is inside the region, over the others, and
// the number inside (the same for the three channels: the finalize pass counts channel 0's)
template <bool REGION>
__global__ __launch_bounds__(NT) void metrics_ssim_kernel(const float* __restrict__ g, const float* __restrict__ t,
                                                         const unsigned char* __restrict__ region, const float* __restrict__ mm,
                                                         double* __restrict__ ssim, const MetricWin win, size_t frame, int np) {
    __shared__ float xs[MHALO][MHALO + 1], ys[MHALO][MHALO + 1];
    __shared__ float hx[MHALO][MTILE + 1], hy[MHALO][MTILE + 1], hxy[MHALO][MTILE + 1], hsq[MHALO][MTILE + 1];
    __shared__ float w1[MWIN];
    __shared__ float wmm[NT / 64][4];
    const int HO = win.h - MWIN + 1, WO = win.w - MWIN + 1;
    const int tiles_x = (WO + MTILE - 1) / MTILE, ntiles = tiles_x * ((HO + MTILE - 1) / MTILE);
    const int ty = blockIdx.x / tiles_x, tx = blockIdx.x % tiles_x;
    const int b = blockIdx.y, c = blockIdx.z;
    const size_t npix = (size_t)win.h * win.w;
    // rescale_01's min / max of the whole image (min / max are exact: any order gives the same values)
    float r0 = INFINITY, r1 = -INFINITY, r2 = INFINITY, r3 = -INFINITY;
    for (int i = threadIdx.x; i < np; i += NT) {
        const float* m = mm + ((size_t)b * np + i) * 4;
        r0 = fminf(r0, m[0]);
        r1 = fmaxf(r1, m[1]);
        r2 = fminf(r2, m[2]);
        r3 = fmaxf(r3, m[3]);
    }
    r0 = shm_wave_min(r0);
    r1 = shm_wave_max(r1);
    r2 = shm_wave_min(r2);
    r3 = shm_wave_max(r3);
    if ((threadIdx.x & 63) == 0) {
        wmm[threadIdx.x >> 6][0] = r0;
        wmm[threadIdx.x >> 6][1] = r1;
        wmm[threadIdx.x >> 6][2] = r2;
        wmm[threadIdx.x >> 6][3] = r3;
    }
    if (threadIdx.x == 0) shm_ssim_gauss1d(w1);
    __syncthreads();
    float xmn = wmm[0][0], xmx = wmm[0][1], ymn = wmm[0][2], ymx = wmm[0][3];
    for (int w = 1; w < NT / 64; ++w) {
        xmn = fminf(xmn, wmm[w][0]);
        xmx = fmaxf(xmx, wmm[w][1]);
        ymn = fminf(ymn, wmm[w][2]);
        ymx = fmaxf(ymx, wmm[w][3]);
    }
    const float xr = xmx - xmn, yr = ymx - ymn;       // divide_no_nan below: a zero range maps the image to 0
    const int oy0 = ty * MTILE, ox0 = tx * MTILE;
    const float* gi = g + ((size_t)b * frame + (size_t)win.top * win.pw + win.left) * 3 + c;
    const float* ti = t + (size_t)b * npix * 3 + c;
    for (int i = threadIdx.x; i < MHALO * MHALO; i += NT) {
        const int r = i / MHALO, cc = i % MHALO;
        const int yy = oy0 + r, xx = ox0 + cc;
        float xv = 0.f, yv = 0.f;
        if (yy < win.h && xx < win.w) {
            const size_t gp = (size_t)yy * win.pw + xx, p = (size_t)yy * win.w + xx;
            xv = xr != 0.f ? (gi[gp * 3] - xmn) / xr : 0.f;
            yv = yr != 0.f ? (ti[p * 3] - ymn) / yr : 0.f;
        }
        xs[r][cc] = xv;
        ys[r][cc] = yv;
    }
    __syncthreads();
    // separable window: row sums of the four moments per (halo row, output column), then eleven taps down the column
    for (int i = threadIdx.x; i < MHALO * MTILE; i += NT) {
        const int r = i / MTILE, cx = i % MTILE;
        float rx = 0.f, ry = 0.f, rxy = 0.f, rsq = 0.f;
        for (int j = 0; j < MWIN; ++j) {
            const float xv = xs[r][cx + j], yv = ys[r][cx + j], w = w1[j];
            rx += w * xv;
            ry += w * yv;
            rxy += w * xv * yv;
            rsq += w * (xv * xv + yv * yv);
        }
        hx[r][cx] = rx;
        hy[r][cx] = ry;
        hxy[r][cx] = rxy;
        hsq[r][cx] = rsq;
    }
    __syncthreads();
    const int ly = threadIdx.x / MTILE, lx = threadIdx.x % MTILE;
    const int oy = oy0 + ly, ox = ox0 + lx;
    double v = 0.0;
    const bool valid = oy < HO && ox < WO;
    if (valid) {
        float mx_ = 0.f, my_ = 0.f, exy = 0.f, esq = 0.f;
        for (int i = 0; i < MWIN; ++i) {
            mx_ += w1[i] * hx[ly + i][lx];
            my_ += w1[i] * hy[ly + i][lx];
            exy += w1[i] * hxy[ly + i][lx];
            esq += w1[i] * hsq[ly + i][lx];
        }
        const float c1 = 0.0025f, c2 = 0.0225f;      // (0.01 * 5)^2, (0.03 * 5)^2: max_val = 5 (test.py:336)
        const float A1 = 2.f * mx_ * my_ + c1, B1 = mx_ * mx_ + my_ * my_ + c1;
        const float A2 = 2.f * exy - 2.f * mx_ * my_ + c2, B2 = esq - mx_ * mx_ - my_ * my_ + c2;
        v = (double)((A1 / B1) * (A2 / B2));
    }
    const size_t slot = ((size_t)b * 3 + c) * ntiles + blockIdx.x;
    if constexpr (REGION) {
        const bool in = valid && region[(size_t)b * npix + (size_t)(oy + MWIN / 2) * win.w + (ox + MWIN / 2)] != 0;
        const double vin = shm_block_sum<NT>(in ? v : 0.0);
        const double vout = shm_block_sum<NT>(in ? 0.0 : v);          // v is 0 at an invalid output
        const double pin = shm_block_sum<NT>(in ? 1.0 : 0.0);
        if (threadIdx.x == 0) {
            ssim[slot * 3] = vin;
            ssim[slot * 3 + 1] = vout;
            ssim[slot * 3 + 2] = pin;
        }
    } else {
        v = shm_block_sum<NT>(v);
        if (threadIdx.x == 0) ssim[slot] = v;
    }
}

// ------------------------------------------------------------------------------------ finalize
// o[0..4] = {mse, psnr, ssim, de76, de94} of one set from its four sums, its npix pixels and nssim SSIM positions.  An empty set
// (possible with a region only) has NaN where the mean is 0 / 0; the whole window never is empty
__device__ __forceinline__ void finish5(double* o, const double a[4], double npix, double nssim) {
    const double mse = npix > 0.0 ? a[0] / (3.0 * npix) : (double)NAN;
    o[0] = mse;
    o[1] = mse > 0.0 ? -10.0 * log10(mse) : npix > 0.0 ? (double)INFINITY : (double)NAN;
    o[2] = nssim > 0.0 ? a[3] / (3.0 * nssim) : (double)NAN;
    o[3] = npix > 0.0 ? a[1] / npix : (double)NAN;
    o[4] = npix > 0.0 ? a[2] / npix : (double)NAN;
}

// grid (B): every thread sums a fixed stride of slots in slot order, then the block sums in thread order
// REGION: out[b][12] = the five inside, the five outside, the pixels inside, the SSIM positions inside
template <bool REGION>
__global__ __launch_bounds__(NT) void metrics_finalize_kernel(const double* __restrict__ pix, const double* __restrict__ ssim, double* __restrict__ out,
                                                             int h, int w, int np, int ntiles) {
    constexpr int SETS = Slots<REGION>::SETS, PIX = Slots<REGION>::PIX, SSIM = Slots<REGION>::SSIM;
    const int b = blockIdx.x;
    double a[SETS][4] = {};
    double nin = 0.0, pin = 0.0;
    for (int i = threadIdx.x; i < np; i += NT) {
        const double* q = pix + ((size_t)b * np + i) * PIX;
        for (int k = 0; k < SETS; ++k) {
            a[k][0] += q[3 * k];
            a[k][1] += q[3 * k + 1];
            a[k][2] += q[3 * k + 2];
        }
        if constexpr (REGION) nin += q[6];
    }
    for (int i = threadIdx.x; i < 3 * ntiles; i += NT) {
        const double* q = ssim + ((size_t)b * 3 * ntiles + i) * SSIM;
        for (int k = 0; k < SETS; ++k) a[k][3] += q[k];
        if constexpr (REGION) pin += i < ntiles ? q[2] : 0.0;      // channel 0's tiles
    }
    for (int k = 0; k < SETS; ++k)
        for (int j = 0; j < 4; ++j) a[k][j] = shm_block_sum<NT>(a[k][j]);
    if constexpr (REGION) {
        nin = shm_block_sum<NT>(nin);
        pin = shm_block_sum<NT>(pin);
    }
    if (threadIdx.x == 0) {
        const double npix = (double)h * w, nssim = (double)(h - MWIN + 1) * (double)(w - MWIN + 1);
        if constexpr (REGION) {
            double* o = out + (size_t)b * SHM_REGION_METRICS;
            finish5(o, a[0], nin, pin);
            finish5(o + 5, a[1], npix - nin, nssim - pin);
            o[10] = nin;
            o[11] = pin;
        } else {
            finish5(out + (size_t)b * 5, a[0], npix, nssim);
        }
    }
}

// -------------------------------------------------------------------------------------- region
// grid (blocks, B): region[b][p] = 1 where the window's pixel p is a highlight, else 0.  RESIDUAL: a = src [B,Hp,Wp,3] (the frame of the
// window), t = target tight [B,h,w,3], highlight = max_c(a_c - t_c) > tau with a NaN difference in any channel outside; PLANE: a = plane
// [B,Hp,Wp], highlight = a > tau (a NaN compares false).  Reads the window only
__global__ __launch_bounds__(NT) void highlight_region_kernel(int mode, const float* __restrict__ a, const float* __restrict__ t, float tau,
                                                             unsigned char* __restrict__ region, const MetricWin win, size_t frame) {
    const int b = blockIdx.y;
    const size_t npix = (size_t)win.h * win.w;
    const float* ai = a + ((size_t)b * frame + (size_t)win.top * win.pw + win.left) * (mode == SHM_REGION_PLANE ? 1 : 3);
    for (size_t p = (size_t)blockIdx.x * NT + threadIdx.x; p < npix; p += (size_t)gridDim.x * NT) {
        const unsigned y = (unsigned)p / (unsigned)win.w;                  // p < 2^30: sides <= 32768
        const size_t fp = (size_t)y * win.pw + ((unsigned)p - y * (unsigned)win.w);
        bool in;
        if (mode == SHM_REGION_PLANE) {
            in = ai[fp] > tau;
        } else {
            const float* tp = t + ((size_t)b * npix + p) * 3;
            const float d0 = ai[fp * 3] - tp[0], d1 = ai[fp * 3 + 1] - tp[1], d2 = ai[fp * 3 + 2] - tp[2];
            in = d0 == d0 && d1 == d1 && d2 == d2 && fmaxf(d0, fmaxf(d1, d2)) > tau;
        }
        region[(size_t)b * npix + p] = in ? 1 : 0;
    }
}

// the three launches of every entry point; frame = pixels per image of pred; region is read with REGION only
template <bool REGION>
int metrics_launch(const float* pred, const float* target, const unsigned char* region, double* out, void* ws, const MetricWs& w, int batch,
                   const MetricWin& win, size_t frame, void* stream, const char* who) {
    hipStream_t st = (hipStream_t)stream;
    char* base = (char*)ws;
    double* pix = (double*)(base + w.pix);
    float* mm = (float*)(base + w.mm);
    double* ssim = (double*)(base + w.ssim);
    const int np = pixel_blocks(win.h, win.w), nt = ssim_tiles(win.h, win.w);
    hipLaunchKernelGGL(metrics_pixel_kernel<REGION>, dim3(np, batch), dim3(NT), 0, st, pred, target, region, pix, mm, win, frame);
    SHM_LAUNCH_CHECK(who);
    hipLaunchKernelGGL(metrics_ssim_kernel<REGION>, dim3(nt, batch, 3), dim3(NT), 0, st, pred, target, region, mm, ssim, win, frame, np);
    SHM_LAUNCH_CHECK(who);
    hipLaunchKernelGGL(metrics_finalize_kernel<REGION>, dim3(batch), dim3(NT), 0, st, pix, ssim, out, win.h, win.w, np, nt);
    SHM_LAUNCH_CHECK(who);
    return SHM_OK;
}

// bytes of workspace of every entry point; 0 for a window or batch the entry point refuses
template <bool REGION>
size_t metrics_workspace(int batch, int h, int w) {
    if (h < MWIN || w < MWIN || batch < 1) return 0;
    return plan_metric_ws<REGION>(batch, h, w).total;
}

// The one body of the three entry points: the checks, the plan and the launches.  `square`: shm_image_metrics, the window (0, 0, s, s) of
// an s x s frame, with its own wording and no limit on the frame's sides
template <bool REGION>
int metrics_entry(const char* who, bool square, const float* pred, int hp, int wp, int top, int left, const float* target, int h, int w,
                  const unsigned char* region, double* out, void* ws, size_t ws_bytes, int batch, void* stream) {
    SHM_REQUIRE(!square || h >= MWIN, SHM_E_SHAPE, "%s: image size %d < 11 (ssim window)", who, h);
    SHM_REQUIRE(h >= MWIN && w >= MWIN, SHM_E_SHAPE, "%s: window %d x %d has a side < 11 (ssim window)", who, h, w);
    SHM_REQUIRE(square || (top >= 0 && left >= 0 && hp >= 1 && wp >= 1 && hp <= 32768 && wp <= 32768 && top <= hp - h && left <= wp - w),
                SHM_E_SHAPE, "%s: window (%d, %d, %d, %d) outside the %d x %d frame", who, top, left, h, w, hp, wp);
    SHM_REQUIRE(batch >= 1 && batch <= 65535, SHM_E_SHAPE, "%s: bad batch %d", who, batch);
    SHM_REQUIRE(pred && target && out && (!REGION || region), SHM_E_SHAPE, "%s: null pointer", who);
    const MetricWs pl = plan_metric_ws<REGION>(batch, h, w);
    SHM_REQUIRE(ws && ws_bytes >= pl.total, SHM_E_WORKSPACE, "%s: workspace %zu < %zu bytes", who, ws_bytes, pl.total);
    const MetricWin win = {wp, top, left, h, w};
    return metrics_launch<REGION>(pred, target, region, out, ws, pl, batch, win, (size_t)hp * wp, stream, who);
}

}  // namespace

extern "C" size_t shm_image_metrics_workspace(int batch, int s) { return metrics_workspace<false>(batch, s, s); }

extern "C" int shm_image_metrics(const float* pred, const float* target, double* out, void* ws, size_t ws_bytes, int batch, int s,
                                 void* stream) {
    return metrics_entry<false>("shm_image_metrics", true, pred, s, s, 0, 0, target, s, s, nullptr, out, ws, ws_bytes, batch, stream);
}

extern "C" size_t shm_image_metrics_hw_workspace(int batch, int h, int w) { return metrics_workspace<false>(batch, h, w); }

extern "C" int shm_image_metrics_hw(const float* pred, int hp, int wp, int top, int left, const float* target, int h, int w, double* out,
                                    void* ws, size_t ws_bytes, int batch, void* stream) {
    return metrics_entry<false>("shm_image_metrics_hw", false, pred, hp, wp, top, left, target, h, w, nullptr, out, ws, ws_bytes, batch, stream);
}

extern "C" size_t shm_image_metrics_region_hw_workspace(int batch, int h, int w) { return metrics_workspace<true>(batch, h, w); }

extern "C" int shm_image_metrics_region_hw(const float* pred, int hp, int wp, int top, int left, const float* target, int h, int w,
                                           const unsigned char* region, double* out, void* ws, size_t ws_bytes, int batch, void* stream) {
    return metrics_entry<true>("shm_image_metrics_region_hw", false, pred, hp, wp, top, left, target, h, w, region, out, ws, ws_bytes, batch,
                               stream);
}

extern "C" int shm_highlight_region_hw(int mode, const float* src, const float* target, const float* plane, int hp, int wp, int top, int left,
                                       int h, int w, float tau, unsigned char* region, int batch, void* stream) {
    SHM_REQUIRE(mode == SHM_REGION_RESIDUAL || mode == SHM_REGION_PLANE, SHM_E_SHAPE, "shm_highlight_region_hw: unknown mode %d", mode);
    SHM_REQUIRE(h >= 1 && w >= 1 && h <= 32768 && w <= 32768, SHM_E_SHAPE, "shm_highlight_region_hw: window %d x %d has a side outside [1, 32768]",
                h, w);
    SHM_REQUIRE(top >= 0 && left >= 0 && hp >= 1 && wp >= 1 && hp <= 32768 && wp <= 32768 && top <= hp - h && left <= wp - w, SHM_E_SHAPE,
                "shm_highlight_region_hw: window (%d, %d, %d, %d) outside the %d x %d frame", top, left, h, w, hp, wp);
    SHM_REQUIRE(batch >= 1 && batch <= 65535, SHM_E_SHAPE, "shm_highlight_region_hw: bad batch %d", batch);
    const bool residual = mode == SHM_REGION_RESIDUAL;
    SHM_REQUIRE(region && (residual ? src && target : plane != nullptr), SHM_E_SHAPE, "shm_highlight_region_hw: null pointer");
    const MetricWin win = {wp, top, left, h, w};
    const int nb = shm_grid_cap((size_t)h * w, 4 * NT, 1024);
    hipLaunchKernelGGL(highlight_region_kernel, dim3(nb, batch), dim3(NT), 0, (hipStream_t)stream, mode, residual ? src : plane, target, tau, region,
                       win, (size_t)hp * wp);
    SHM_LAUNCH_CHECK("shm_highlight_region_hw");
    return SHM_OK;
}
