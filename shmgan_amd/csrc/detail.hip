// Guided detail transfer: the generator changes one plane, the standardised Y, at model resolution.  That change is fitted locally
// against the Y the network was fed (the fast guided filter of He & Sun, target = the correction gen_Y - Y_in), the fit's two
// coefficients are upsampled with the sampler of bilinear.h and applied to the photo's own Y at the photo's own size; chroma and
// fine detail stay the camera's.  include/shmgan_hip.h states the arithmetic of both entry points.
//
//   shm_detail_coeffs     one launch, grid (cdiv(w, 32), cdiv(h, 16), batch), 256 threads; a block makes a 16 x 32 tile of coef from the
//                         guide and the target on a halo of 2r, all in LDS: raw planes -> row sums of (I', d, I'I', I'd) -> column sums,
//                         a and b on a halo of r -> row sums of (a, b) -> column sums, coef.  Every window sum runs over that window's
//                         own elements, left to right or top to bottom: no running sums, no atomics.
//   shm_detail_apply_u8   one launch over the flat photo, 1024 pixels per block of 256 threads, four pixels per lane: three coalesced
//                         4-byte loads per lane into LDS, each lane reads its 12 bytes back, and the 12 floats go through LDS to
//                         three coalesced 16-byte stores per lane.  coef (8 bytes per model pixel) stays in cache.
#include "bilinear.h"
#include "yuv.h"

#include <math.h>

namespace {

constexpr int DC_NT = 256;
constexpr int DC_TH = 16, DC_TW = 32;           // coef tile of one block
constexpr int DC_RMAX = 8;                      // radius
constexpr int DC_DIM_MAX = 32768;               // sides of a plane and of a photo
constexpr int DC_IN_H = DC_TH + 4 * DC_RMAX, DC_IN_W = DC_TW + 4 * DC_RMAX;      // raw planes: the tile and a halo of 2r
constexpr int DC_MID_W = DC_TW + 2 * DC_RMAX;                                    // a, b and the first row sums: a halo of r

// first and last index of the window of radius r around i that lie inside [0, n)
__device__ __forceinline__ void clip_window(int i, int r, int n, int& lo, int& hi) {
    lo = max(i - r, 0);
    hi = min(i + r, n - 1);
}

__global__ void __launch_bounds__(DC_NT) detail_coeffs_kernel(const float* __restrict__ guide, int ldg, const float* __restrict__ target, int ldt,
                                                              float* __restrict__ coef, int h, int w, int r, float eps) {
#pragma clang fp contract(off)              // var and cov at radius 0 are x * y - x * y = 0 exactly: no product may be fused into the subtraction
    __shared__ float s_i[DC_IN_H * DC_IN_W];            // I, later a
    __shared__ float s_d[DC_IN_H * DC_IN_W];            // d, later b
    __shared__ float s_row[4][DC_IN_H * DC_MID_W];      // row sums of (I', d, I'I', I'd), later of (a, b)
    const int tid = threadIdx.x;
    const int x0 = blockIdx.x * DC_TW, y0 = blockIdx.y * DC_TH;
    const size_t img = (size_t)blockIdx.z * h * w;
    const float* gi = guide + img * ldg;
    const float* gt = target + img * ldt;
    const int in_w = DC_TW + 4 * r, in_h = DC_TH + 4 * r, mid_w = DC_TW + 2 * r, mid_h = DC_TH + 2 * r;
    const int gx0 = x0 - 2 * r, gy0 = y0 - 2 * r;        // plane position of s_i[0]
    const int mx0 = x0 - r, my0 = y0 - r;                // plane position of the first a / b

    // ---- the raw planes: I and d = p - I on the tile and its halo of 2r; what lies outside the plane is never read again
    float part = 0.f;
    for (int e = tid; e < in_h * in_w; e += DC_NT) {
        const int yy = e / in_w, xx = e - yy * in_w;
        const int gy = gy0 + yy, gx = gx0 + xx;
        float vi = 0.f, vd = 0.f;
        if (gy >= 0 && gy < h && gx >= 0 && gx < w) {
            const size_t p = (size_t)gy * w + gx;
            vi = gi[p * ldg];
            vd = gt[p * ldt] - vi;
            part += vi;
        }
        s_i[e] = vi;
        s_d[e] = vd;
    }
    // the block's reference value: the mean of I over the part of its region inside the plane (any block-uniform number would do:
    // var and cov are shift-invariant); 0 when that mean is not finite
    const int rows_in = min(gy0 + in_h, h) - max(gy0, 0), cols_in = min(gx0 + in_w, w) - max(gx0, 0);
    float ref = shm_block_sum<DC_NT>(part) / (float)(rows_in * cols_in);      // its barriers also publish s_i / s_d
    if (!(fabsf(ref) <= 3.0e38f)) ref = 0.f;

    // ---- row sums over the clipped (2r + 1) columns, for every row of the region and the columns a / b need
    for (int e = tid; e < in_h * mid_w; e += DC_NT) {
        const int yy = e / mid_w, xx = e - yy * mid_w;
        const int gy = gy0 + yy, gx = mx0 + xx;
        if (gy < 0 || gy >= h || gx < 0 || gx >= w) continue;
        int lo, hi;
        clip_window(gx, r, w, lo, hi);
        float si = 0.f, sd = 0.f, sii = 0.f, sid = 0.f;
        for (int c = lo; c <= hi; ++c) {
            const float vi = s_i[yy * in_w + (c - gx0)] - ref, vd = s_d[yy * in_w + (c - gx0)];
            si += vi;
            sd += vd;
            sii += vi * vi;
            sid += vi * vd;
        }
        s_row[0][e] = si;
        s_row[1][e] = sd;
        s_row[2][e] = sii;
        s_row[3][e] = sid;
    }
    __syncthreads();
    // ---- column sums over the clipped (2r + 1) rows: the four box means, then a and b on the tile and its halo of r
    for (int e = tid; e < mid_h * mid_w; e += DC_NT) {
        const int yy = e / mid_w, xx = e - yy * mid_w;
        const int gy = my0 + yy, gx = mx0 + xx;
        if (gy < 0 || gy >= h || gx < 0 || gx >= w) continue;
        int lo, hi, xlo, xhi;
        clip_window(gy, r, h, lo, hi);
        clip_window(gx, r, w, xlo, xhi);
        float si = 0.f, sd = 0.f, sii = 0.f, sid = 0.f;
        for (int y = lo; y <= hi; ++y) {
            const int q = (y - gy0) * mid_w + xx;
            si += s_row[0][q];
            sd += s_row[1][q];
            sii += s_row[2][q];
            sid += s_row[3][q];
        }
        const float cnt = (float)((hi - lo + 1) * (xhi - xlo + 1));
        const float mi = si / cnt, md = sd / cnt, mii = sii / cnt, mid = sid / cnt;
        const float var = mii - mi * mi, cov = mid - mi * md;
        // 0 * (mi + md): 0 for a finite window, NaN for one that holds a NaN or an Inf -- what a and b are then does not depend on ref
        const float a = cov / (var + eps) + 0.f * (mi + md);
        const float b = md - a * (mi + ref);
        s_i[e] = a;                     // the raw planes are dead: every reader is behind the barrier above
        s_d[e] = b;
    }
    __syncthreads();
    // ---- coef = (box(a), box(b)): rows, then columns
    for (int e = tid; e < mid_h * DC_TW; e += DC_NT) {
        const int yy = e / DC_TW, xx = e - yy * DC_TW;
        const int gy = my0 + yy, gx = x0 + xx;
        if (gy < 0 || gy >= h || gx >= w) continue;
        int lo, hi;
        clip_window(gx, r, w, lo, hi);
        float sa = 0.f, sb = 0.f;
        for (int c = lo; c <= hi; ++c) {
            sa += s_i[yy * mid_w + (c - mx0)];
            sb += s_d[yy * mid_w + (c - mx0)];
        }
        s_row[0][e] = sa;
        s_row[1][e] = sb;
    }
    __syncthreads();
    for (int e = tid; e < DC_TH * DC_TW; e += DC_NT) {
        const int yy = e / DC_TW, xx = e - yy * DC_TW;
        const int gy = y0 + yy, gx = x0 + xx;
        if (gy >= h || gx >= w) continue;
        int lo, hi, xlo, xhi;
        clip_window(gy, r, h, lo, hi);
        clip_window(gx, r, w, xlo, xhi);
        float sa = 0.f, sb = 0.f;
        for (int y = lo; y <= hi; ++y) {
            sa += s_row[0][(y - my0) * DC_TW + xx];
            sb += s_row[1][(y - my0) * DC_TW + xx];
        }
        const float cnt = (float)((hi - lo + 1) * (xhi - xlo + 1));
        *reinterpret_cast<float2*>(coef + (img + (size_t)gy * w + gx) * 2) = make_float2(sa / cnt, sb / cnt);
    }
}

constexpr int DA_NT = 256;
constexpr int DA_PX = 4;                        // pixels per lane
constexpr int DA_BLOCK_PX = DA_NT * DA_PX;      // 1024 pixels = 768 input words = 768 output 16-byte words per block

// One block's 1024 pixels.  FULL: all of them lie inside the photo (every block but the last), so no load, pixel or store looks at the end
template <bool FULL>
__device__ __forceinline__ void detail_apply_block(unsigned* s_in, f32x4* s_out, const unsigned char* __restrict__ photo, int h, int w,
                                                   const float* __restrict__ coef, int hm, int wm, const float* __restrict__ scale_ptr,
                                                   float* __restrict__ out) {
    const int tid = threadIdx.x;
    const size_t npix = (size_t)h * w, nbytes = npix * 3;                 // bytes in, floats out
    const size_t word0 = (size_t)blockIdx.x * (DA_NT * 3);                // the block's first 4-byte input word = its first 16-byte output word
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const size_t e = (word0 + j * DA_NT + tid) * 4;
        unsigned v = 0;
        if (FULL || e + 4 <= nbytes) {
            v = *reinterpret_cast<const unsigned*>(photo + e);
        } else {
            for (int q = 0; q < 4; ++q)
                if (e + q < nbytes) v |= (unsigned)photo[e + q] << (8 * q);
        }
        s_in[j * DA_NT + tid] = v;
    }
    __syncthreads();
    const float inv = 1.0f / scale_ptr[0];          // one division per lane, not three per pixel: the kernel is VALU-bound before it is HBM-bound
    const float hs = (float)hm / (float)h, ws = (float)wm / (float)w;
    const size_t p0 = (size_t)blockIdx.x * DA_BLOCK_PX + (size_t)tid * DA_PX;
    int oy = (int)((unsigned)p0 / (unsigned)w), ox = (int)((unsigned)p0 - (unsigned)oy * (unsigned)w);      // pixels fit 32 bits (sides <= 32768); elements do not
    const unsigned w3[3] = {s_in[tid * 3], s_in[tid * 3 + 1], s_in[tid * 3 + 2]};
    float o[12];
#pragma unroll
    for (int q = 0; q < DA_PX; ++q) {
        float rgb[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const int byte = q * 3 + k;
            rgb[k] = (float)((w3[byte >> 2] >> (8 * (byte & 3))) & 0xffu) * (1.0f / 255.0f);
        }
        float r = 0.f, g = 0.f, b = 0.f;
        if (FULL || p0 + q < npix) {
            float y, u, v;
            rgb2yuv(rgb[0], rgb[1], rgb[2], y, u, v);
            y *= inv;
            u *= inv;
            v *= inv;
            const BilinearTaps t = bilinear_taps(ox, oy, hm, wm, wm, hs, ws, 0.f, 0.f);
            const float2 tl = *reinterpret_cast<const float2*>(coef + t.tl * 2), tr = *reinterpret_cast<const float2*>(coef + t.tr * 2);
            const float2 bl = *reinterpret_cast<const float2*>(coef + t.bl * 2), br = *reinterpret_cast<const float2*>(coef + t.br * 2);
            const float ca = bilinear_lerp(tl.x, tr.x, bl.x, br.x, t.lx, t.ly), cb = bilinear_lerp(tl.y, tr.y, bl.y, br.y, t.lx, t.ly);
            const float yn = y + (ca * y + cb);
            r = yn + Y2R_V_R * v;
            g = yn + Y2R_U_G * u + Y2R_V_G * v;
            b = yn + Y2R_U_B * u;
            if (++ox == w) {
                ox = 0;
                ++oy;
            }
        }
        o[q * 3] = r;
        o[q * 3 + 1] = g;
        o[q * 3 + 2] = b;
    }
#pragma unroll
    for (int j = 0; j < 3; ++j) s_out[tid * 3 + j] = (f32x4){o[4 * j], o[4 * j + 1], o[4 * j + 2], o[4 * j + 3]};
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const size_t e = (word0 + j * DA_NT + tid) * 4;                   // float offset of this lane's 16-byte word
        const f32x4 v = s_out[j * DA_NT + tid];
        if (FULL || e + 4 <= nbytes) {
            *reinterpret_cast<f32x4*>(out + e) = v;
        } else {
#pragma unroll
            for (int q = 0; q < 4; ++q)
                if (e + q < nbytes) out[e + q] = v[q];
        }
    }
}

__global__ void __launch_bounds__(DA_NT) detail_apply_u8_kernel(const unsigned char* __restrict__ photo, int h, int w, const float* __restrict__ coef,
                                                                int hm, int wm, const float* __restrict__ scale_ptr, float* __restrict__ out) {
    __shared__ unsigned s_in[DA_NT * 3];
    __shared__ f32x4 s_out[DA_NT * 3];
    if (((size_t)blockIdx.x + 1) * DA_BLOCK_PX <= (size_t)h * w)
        detail_apply_block<true>(s_in, s_out, photo, h, w, coef, hm, wm, scale_ptr, out);
    else
        detail_apply_block<false>(s_in, s_out, photo, h, w, coef, hm, wm, scale_ptr, out);
}

}  // namespace

extern "C" int shm_detail_coeffs(const float* guide, int ldg, const float* target, int ldt, float* coef, int batch, int h, int w, int radius,
                                 float eps, void* stream) {
    SHM_REQUIRE(guide && target && coef, SHM_E_SHAPE, "shm_detail_coeffs: null pointer (guide, target or coef)");
    SHM_REQUIRE(radius >= 0 && radius <= DC_RMAX, SHM_E_SHAPE, "shm_detail_coeffs: radius %d outside [0, %d]", radius, DC_RMAX);
    SHM_REQUIRE(eps > 0.f && eps <= 3.0e38f, SHM_E_SHAPE, "shm_detail_coeffs: eps %g is not a positive finite number", (double)eps);
    SHM_REQUIRE(batch >= 1 && batch <= 65535, SHM_E_SHAPE, "shm_detail_coeffs: batch %d outside [1, 65535]", batch);
    SHM_REQUIRE(h >= 1 && h <= DC_DIM_MAX && w >= 1 && w <= DC_DIM_MAX, SHM_E_SHAPE, "shm_detail_coeffs: sides h %d, w %d outside [1, %d]", h, w, DC_DIM_MAX);
    SHM_REQUIRE(ldg >= 1 && ldt >= 1, SHM_E_SHAPE, "shm_detail_coeffs: pitches ldg %d, ldt %d smaller than 1", ldg, ldt);
    SHM_REQUIRE(((uintptr_t)coef & 7) == 0, SHM_E_SHAPE, "shm_detail_coeffs: coef is not 8-byte aligned");
    const dim3 grid(shm_cdiv(w, DC_TW), shm_cdiv(h, DC_TH), batch);
    hipLaunchKernelGGL(detail_coeffs_kernel, grid, dim3(DC_NT), 0, (hipStream_t)stream, guide, ldg, target, ldt, coef, h, w, radius, eps);
    SHM_LAUNCH_CHECK("shm_detail_coeffs");
    return SHM_OK;
}

extern "C" int shm_detail_apply_u8(const unsigned char* photo, int h, int w, const float* coef, int hm, int wm, const float* scale, float* out,
                                   void* stream) {
    SHM_REQUIRE(photo && coef && scale && out, SHM_E_SHAPE, "shm_detail_apply_u8: null pointer (photo, coef, scale or out)");
    SHM_REQUIRE(h >= 1 && h <= DC_DIM_MAX && w >= 1 && w <= DC_DIM_MAX, SHM_E_SHAPE, "shm_detail_apply_u8: photo sides h %d, w %d outside [1, %d]", h, w,
                DC_DIM_MAX);
    SHM_REQUIRE(hm >= 1 && hm <= DC_DIM_MAX && wm >= 1 && wm <= DC_DIM_MAX, SHM_E_SHAPE, "shm_detail_apply_u8: coef sides H %d, W %d outside [1, %d]", hm, wm,
                DC_DIM_MAX);
    SHM_REQUIRE(((uintptr_t)photo & 3) == 0, SHM_E_SHAPE, "shm_detail_apply_u8: photo is not 4-byte aligned");
    SHM_REQUIRE(((uintptr_t)coef & 7) == 0, SHM_E_SHAPE, "shm_detail_apply_u8: coef is not 8-byte aligned");
    SHM_REQUIRE(((uintptr_t)out & 15) == 0, SHM_E_SHAPE, "shm_detail_apply_u8: out is not 16-byte aligned");
    const size_t npix = (size_t)h * w;
    hipLaunchKernelGGL(detail_apply_u8_kernel, dim3((unsigned)((npix + DA_BLOCK_PX - 1) / DA_BLOCK_PX)), dim3(DA_NT), 0, (hipStream_t)stream, photo, h, w,
                       coef, hm, wm, scale, out);
    SHM_LAUNCH_CHECK("shm_detail_apply_u8");
    return SHM_OK;
}
