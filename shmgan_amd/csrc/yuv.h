// tf.image.rgb_to_yuv: the constants and the expression order, in one place for the kernels of color.hip (shm_rgb2yuv_std) and the
// image / mask pair kernel (augment_pairs.hip), which converts in registers what color.hip reads from memory.  The constants of
// tf.image.yuv_to_rgb stand beside them for color.hip (shm_yuv2rgb), imgloss.hip and detail.hip (shm_detail_apply_u8).
#pragma once
#include "common.h"

#include <math.h>

// tf.image.rgb_to_yuv kernel (column j of yuv = sum_i rgb[i] * K[i][j])
#define R2Y_00 0.299f
#define R2Y_01 -0.14714119f
#define R2Y_02 0.61497538f
#define R2Y_10 0.587f
#define R2Y_11 -0.28886916f
#define R2Y_12 -0.51496512f
#define R2Y_20 0.114f
#define R2Y_21 0.43601035f
#define R2Y_22 -0.10001026f

// tf.image.yuv_to_rgb kernel
#define Y2R_V_R 1.13988303f
#define Y2R_U_G -0.394642334f
#define Y2R_V_G -0.58062185f
#define Y2R_U_B 2.03206185f

__device__ __forceinline__ void rgb2yuv(float r, float g, float b, float& y, float& u, float& v) {
    y = r * R2Y_00 + g * R2Y_10 + b * R2Y_20;
    u = r * R2Y_01 + g * R2Y_11 + b * R2Y_21;
    v = r * R2Y_02 + g * R2Y_12 + b * R2Y_22;
}

// custom_per_image_standardization's divisor from a sample's two f64 sums over cnt values: max(std, 1/256) (rsqrt(65536), SHM.py:1280,1293)
__device__ __forceinline__ float yuv_std_scale(double sum, double sumsq, double cnt) {
    double mean = sum / cnt;
    double var = sumsq / cnt - mean * mean;
    if (var < 0.0) var = 0.0;
    return fmaxf((float)sqrt(var), 1.0f / 256.0f);
}
