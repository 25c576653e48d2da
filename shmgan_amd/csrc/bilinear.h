// The one bilinear sampler of the image kernels: tf.image.resize(bilinear, half-pixel centres, no antialias), ResizeBilinear with
// half_pixel_centers.  Per axis in = (out + 0.5) * scale - 0.5 + origin, lower = floor(in), upper = ceil(in), frac = in - floor(in);
// scale = sampled extent / output extent and origin = where the sampled extent begins (0 for a plain resize, the crop's origin for
// an augmenting one: + 0.0f changes no value).  Both taps are held inside [0, n - 1].  For a sampled extent inside the image only
// max(lower, 0) and min(upper, n - 1) ever act, which is all that TensorFlow's kernel applies; the other two are there so that no
// rounding can index outside the image.  Every kernel that resamples (data.hip, polar.hip, augment*.hip, export.hip) calls these two
// functions and nothing else, so they agree bit for bit wherever their parameters do.
#pragma once
#include "common.h"

#include <math.h>

// The four taps of one output pixel as PIXEL indices y * pitch + x of the source (times the pixel pitch gives the element), and the
// two weights
struct BilinearTaps {
    size_t tl, tr, bl, br;
    float lx, ly;
};

// Output pixel (ox, oy) on a source of hin x win pixels, rows `pitch` pixels apart.  Every argument but ox / oy is block-uniform.
__device__ __forceinline__ BilinearTaps bilinear_taps(int ox, int oy, int hin, int win, int pitch, float hs, float ws, float cy, float cx) {
    const float fy = (((float)oy + 0.5f) * hs - 0.5f) + cy, fx = (((float)ox + 0.5f) * ws - 0.5f) + cx;
    const float fly = floorf(fy), flx = floorf(fx);
    // held inside the image as floats, one v_med3_f32 a tap (exact: sides are at most 32768), then converted
    const float ym = (float)(hin - 1), xm = (float)(win - 1);
    const int y0 = (int)__builtin_amdgcn_fmed3f(fly, 0.f, ym), y1 = (int)__builtin_amdgcn_fmed3f(ceilf(fy), 0.f, ym);
    const int x0 = (int)__builtin_amdgcn_fmed3f(flx, 0.f, xm), x1 = (int)__builtin_amdgcn_fmed3f(ceilf(fx), 0.f, xm);
    BilinearTaps t;
    t.ly = fy - fly;
    t.lx = fx - flx;
    t.tl = (size_t)y0 * pitch + x0;
    t.tr = (size_t)y0 * pitch + x1;
    t.bl = (size_t)y1 * pitch + x0;
    t.br = (size_t)y1 * pitch + x1;
    return t;
}

// The lerp of the four tap values, before any output scale
__device__ __forceinline__ float bilinear_lerp(float tl, float tr, float bl, float br, float lx, float ly) {
    const float top = tl + (tr - tl) * lx, bot = bl + (br - bl) * lx;
    return top + (bot - top) * ly;
}
