// Specular-highlight masks from the four polarised views of ONE sample (include/shmgan_hip.h, "specular masks"): light reflected
// specularly is polarised, the diffuse part is not, so the polarised intensity sqrt(S1^2 + S2^2) of the Stokes fit -- the part
// polar_estimate<SHM_POLAR_STOKES> subtracts -- is a highlight map that needs no label.  Three stages, four launches, all on
// the caller's stream and without a host synchronisation: the threshold stays in device memory and the next kernel reads it there.
// shm_specmask runs the chain (every argument checked before the first launch); each stage is an entry point of its own as well.
//
//   shm_specmask_strength   q = min(255, (int) sqrt(max_c (S1_c^2 + S2_c^2))) as a uint8 map and its 256-bin histogram in the same
//                           launch.  Four pixels per thread and step (three dword loads per view, one dword store) when every pointer is
//                           4-byte aligned, byte accesses otherwise and in the last, partial group; grid-stride beyond SM_BLOCKS blocks.
//                           A block counts into 256 LDS words with integer LDS atomics and adds its non-empty bins to the global
//                           histogram with one integer atomic each: integer sums, so the histogram is exact and the same on every run,
//                           whatever the arrival order.  An LDS word cannot wrap: a block's share is below the 2^31 / 3 pixels the
//                           entry point admits.  The maximum over the channels is taken BEFORE the root: with integer coefficients
//                           S1^2 + S2^2 is an exact integer below 2^24 and (int) sqrtf of it is the integer square root.
//   shm_specmask_otsu       one block: exact 64-bit prefix counts and moments, the between-class variance N0 N1 (M1/N1 - M0/N0)^2 in
//                           double, arg-max with the lowest t on ties; writes t and t_eff = max(t, floor) (or the fixed threshold).
//   shm_specmask_morph      b = q > t_eff, opened with a (2 ro + 1)^2 square and dilated with a (2 rd + 1)^2 one.  Two launches of one
//                           LDS-tiled separable kernel: threshold + erosion by ro, then ONE dilation by ro + rd (two dilations of a
//                           rectangle's subset by squares compose, also with the border rule below).  A tile and its halo are loaded
//                           once; the row pass runs over the tile's rows and halo rows, the column pass over the tile.  Out-of-image
//                           taps are skipped, i.e. read as the neutral element (1 under min, 0 under max).  The second launch counts
//                           the set pixels: LDS integer atomics, then one global integer atomic per block with a non-zero count.
// Every kernel is byte-wide streaming or a 256-element scan: launch- and latency-bound at the sizes of a capture.
#include "common.h"
#include "polar_est.h"

#include <limits.h>
#include <math.h>

namespace {

constexpr int SM_NT = 256;                      // threads of every block here; also the number of bins
constexpr int SM_PX = 4;                        // pixels per thread and step of the strength kernel
constexpr int SM_BLOCKS = 1024;                 // grid cap of the strength kernel (grid-stride beyond it)
constexpr int MO_TW = 64, MO_TH = 32;           // output tile of the morphology kernel
constexpr int MO_RMAX = SHM_SPECMASK_MAX_OPEN + SHM_SPECMASK_MAX_DILATE;
constexpr int MO_LW = MO_TW + 2 * MO_RMAX, MO_LH = MO_TH + 2 * MO_RMAX;

struct SpecStrengthArgs {
    const unsigned char* src[4];
    float coef[12];
};

__device__ __forceinline__ float sm_byte(const unsigned* w, int k) { return (float)((w[k >> 2] >> ((k & 3) * 8)) & 255u); }

template <bool VEC>
__global__ void __launch_bounds__(SM_NT) specmask_strength_kernel(const SpecStrengthArgs a, int n, unsigned char* __restrict__ q,
                                                                  unsigned* __restrict__ hist) {
    __shared__ unsigned bins[SM_NT];
    bins[threadIdx.x] = 0;
    __syncthreads();
    const int groups = (n + SM_PX - 1) / SM_PX;
    for (int g = blockIdx.x * SM_NT + threadIdx.x; g < groups; g += gridDim.x * SM_NT) {
        const int p0 = g * SM_PX, cnt = min(SM_PX, n - p0);
        const size_t b0 = (size_t)p0 * 3;
        unsigned wv[4][3];
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            if (VEC && cnt == SM_PX) {
                const unsigned* p = (const unsigned*)(a.src[v] + b0);
                wv[v][0] = p[0];
                wv[v][1] = p[1];
                wv[v][2] = p[2];
            } else {
                wv[v][0] = wv[v][1] = wv[v][2] = 0;
#pragma unroll
                for (int i = 0; i < 3 * SM_PX; ++i)
                    if (i < 3 * cnt) wv[v][i >> 2] |= (unsigned)a.src[v][b0 + i] << ((i & 3) * 8);
            }
        }
        unsigned out = 0;
#pragma unroll
        for (int px = 0; px < SM_PX; ++px) {
            if (px < cnt) {
                float e = 0.f;
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const int k = px * 3 + c;
                    e = fmaxf(e, polar_strength2(a.coef, sm_byte(wv[0], k), sm_byte(wv[1], k), sm_byte(wv[2], k), sm_byte(wv[3], k)));
                }
                const unsigned qi = (unsigned)(int)fminf(sqrtf(e), 255.f);          // = min(255, (int) p); the clamp first, so no cast overflows
                atomicAdd(&bins[qi], 1u);
                out |= qi << (8 * px);
            }
        }
        if (VEC && cnt == SM_PX) {
            *(unsigned*)(q + p0) = out;
        } else {
#pragma unroll
            for (int px = 0; px < SM_PX; ++px)
                if (px < cnt) q[p0 + px] = (unsigned char)(out >> (8 * px));
        }
    }
    __syncthreads();
    const unsigned c = bins[threadIdx.x];
    if (c) atomicAdd(&hist[threadIdx.x], c);
}

__global__ void __launch_bounds__(SM_NT) specmask_otsu_kernel(const unsigned* __restrict__ hist, int floor_t, int fixed_t, int* __restrict__ stats) {
    __shared__ unsigned long long pn[SM_NT], pm[SM_NT];
    __shared__ double var[SM_NT];
    __shared__ int arg[SM_NT];
    const int t = threadIdx.x;
    // bins <= t are class 0: inclusive prefix sums of the counts and of count * bin, eight doubling steps; integers, so exact in any order
    const unsigned long long c = hist[t];
    pn[t] = c;
    pm[t] = c * (unsigned long long)t;
    __syncthreads();
    for (int off = 1; off < SM_NT; off <<= 1) {
        const unsigned long long an = t >= off ? pn[t - off] : 0ull, am = t >= off ? pm[t - off] : 0ull;
        __syncthreads();
        pn[t] += an;
        pm[t] += am;
        __syncthreads();
    }
    const unsigned long long n0 = pn[t], m0 = pm[t], n = pn[SM_NT - 1], m = pm[SM_NT - 1];
    const unsigned long long n1 = n - n0, m1 = m - m0;
    double v = 0.0;                                                    // an empty class scores 0
    if (n0 != 0 && n1 != 0) {
        const double d = (double)m1 / (double)n1 - (double)m0 / (double)n0;
        v = (double)n0 * (double)n1 * d * d;
    }
    var[t] = v;
    arg[t] = t;
    __syncthreads();
    for (int s = SM_NT / 2; s > 0; s >>= 1) {
        if (t < s) {
            const double vo = var[t + s];
            const int ao = arg[t + s];
            if (vo > var[t] || (vo == var[t] && ao < arg[t])) {     // the lowest t among equal maxima
                var[t] = vo;
                arg[t] = ao;
            }
        }
        __syncthreads();
    }
    if (t == 0) {
        stats[0] = arg[0];
        stats[1] = fixed_t >= 0 ? fixed_t : max(arg[0], floor_t);
    }
}

// ERODE: in = q, a pixel is set where q > stats[1]; min over the square; out = 0 / 1.  Otherwise: in = that 0 / 1 map; max over the square;
// out = 0 / 255 and stats[2] += the set pixels.  R = 0 is the identity (after the threshold).
template <bool ERODE>
__global__ void __launch_bounds__(SM_NT) specmask_morph_kernel(const unsigned char* __restrict__ in, unsigned char* __restrict__ out, int h, int w,
                                                               int tiles_x, int R, int* __restrict__ stats) {
    __shared__ unsigned char a[MO_LH * MO_LW];          // the tile and its halo, 0 / 1
    __shared__ unsigned char b[MO_LH * MO_TW];          // after the row pass
    __shared__ unsigned total;
    const int tid = threadIdx.x;
    const int x0 = (int)(blockIdx.x % tiles_x) * MO_TW, y0 = (int)(blockIdx.x / tiles_x) * MO_TH;
    const int lw = MO_TW + 2 * R, lh = MO_TH + 2 * R;
    const int thr = ERODE ? stats[1] : 0;
    const unsigned neutral = ERODE ? 1u : 0u;
    if (tid == 0) total = 0;
    for (int i = tid; i < lh * lw; i += SM_NT) {
        const int r = i / lw, c = i - r * lw;
        const int gy = y0 - R + r, gx = x0 - R + c;
        unsigned v = neutral;                           // a tap outside the image is skipped: it reads as the neutral element
        if (gy >= 0 && gy < h && gx >= 0 && gx < w) {
            const int px = in[(size_t)gy * w + gx];
            v = ERODE ? (px > thr) : (px != 0);
        }
        a[r * MO_LW + c] = (unsigned char)v;
    }
    __syncthreads();
    for (int i = tid; i < lh * MO_TW; i += SM_NT) {
        const int r = i / MO_TW, c = i % MO_TW;
        unsigned acc = neutral;
        for (int d = 0; d <= 2 * R; ++d) {
            const unsigned x = a[r * MO_LW + c + d];
            acc = ERODE ? (acc & x) : (acc | x);
        }
        b[r * MO_TW + c] = (unsigned char)acc;
    }
    __syncthreads();
    unsigned mine = 0;
    for (int i = tid; i < MO_TH * MO_TW; i += SM_NT) {
        const int r = i / MO_TW, c = i % MO_TW;
        const int gy = y0 + r, gx = x0 + c;
        if (gy < h && gx < w) {
            unsigned acc = neutral;
            for (int d = 0; d <= 2 * R; ++d) {
                const unsigned x = b[(r + d) * MO_TW + c];
                acc = ERODE ? (acc & x) : (acc | x);
            }
            out[(size_t)gy * w + gx] = (unsigned char)(ERODE ? acc : acc * 255u);
            mine += acc;
        }
    }
    if (!ERODE) {
        if (mine) atomicAdd(&total, mine);
        __syncthreads();
        if (tid == 0 && total) atomicAdd(&stats[2], (int)total);
    }
}

// h, w >= 1 and every byte offset of a [h,w,3] view within a 32-bit index
int specmask_shape(const char* who, int h, int w) {
    SHM_REQUIRE(h >= 1 && w >= 1, SHM_E_SHAPE, "%s: h %d, w %d must be at least 1", who, h, w);
    SHM_REQUIRE((long long)h * w * 3 <= (long long)INT_MAX, SHM_E_SHAPE, "%s: h %d x w %d x 3 bytes is outside the 32-bit index range", who, h, w);
    return SHM_OK;
}

// The checks of the three stages, each complete before its stage launches anything; shm_specmask makes all of them before the first launch
int check_strength(const char* who, const unsigned char* const* src_ptrs, int h, int w, const float* coef, const unsigned char* q, const unsigned* hist) {
    SHM_REQUIRE(src_ptrs && coef && q && hist, SHM_E_SHAPE, "%s: null pointer (src_ptrs, coef, q or hist)", who);
    for (int v = 0; v < 4; ++v) SHM_REQUIRE(src_ptrs[v], SHM_E_SHAPE, "%s: null pointer (source view %d)", who, v);
    return specmask_shape(who, h, w);
}

int check_otsu(const char* who, const unsigned* hist, int floor_t, int fixed_t, const int* stats) {
    SHM_REQUIRE(hist && stats, SHM_E_SHAPE, "%s: null pointer (hist or stats)", who);
    SHM_REQUIRE(floor_t >= 0 && floor_t <= 255, SHM_E_SHAPE, "%s: floor %d outside [0, 255]", who, floor_t);
    SHM_REQUIRE(fixed_t >= -1 && fixed_t <= 255, SHM_E_SHAPE, "%s: fixed threshold %d outside [0, 255] (-1 = none)", who, fixed_t);
    return SHM_OK;
}

int check_morph(const char* who, const unsigned char* q, int h, int w, int open_radius, int dilate_radius, const unsigned char* tmp, const unsigned char* mask,
                const int* stats) {
    SHM_REQUIRE(q && tmp && mask && stats, SHM_E_SHAPE, "%s: null pointer (q, tmp, mask or stats)", who);
    SHM_REQUIRE(tmp != q && tmp != mask, SHM_E_SHAPE, "%s: tmp must be a buffer of its own", who);
    if (int rc = specmask_shape(who, h, w)) return rc;
    SHM_REQUIRE(open_radius >= 0 && open_radius <= SHM_SPECMASK_MAX_OPEN, SHM_E_SHAPE, "%s: open_radius %d outside [0, %d]", who, open_radius,
                SHM_SPECMASK_MAX_OPEN);
    SHM_REQUIRE(dilate_radius >= 0 && dilate_radius <= SHM_SPECMASK_MAX_DILATE, SHM_E_SHAPE, "%s: dilate_radius %d outside [0, %d]", who, dilate_radius,
                SHM_SPECMASK_MAX_DILATE);
    return SHM_OK;
}

int clear_words(const char* who, const char* what, void* p, size_t bytes, hipStream_t st) {
    if (hipMemsetAsync(p, 0, bytes, st) != hipSuccess) {
        (void)hipGetLastError();
        shm_set_error("%s: clearing the %s failed", who, what);
        return SHM_E_HIP;
    }
    return SHM_OK;
}

int launch_strength(const char* who, const unsigned char* const* src_ptrs, int h, int w, const float* coef, unsigned char* q, unsigned* hist, hipStream_t st) {
    SpecStrengthArgs a;
    uintptr_t bits = (uintptr_t)q;
    for (int v = 0; v < 4; ++v) {
        a.src[v] = src_ptrs[v];
        bits |= (uintptr_t)src_ptrs[v];
    }
    for (int i = 0; i < 12; ++i) a.coef[i] = coef[i];
    const int n = h * w;
    // the histogram holds this image's counts whatever it held before
    if (int rc = clear_words(who, "histogram", hist, SM_NT * sizeof(unsigned), st)) return rc;
    const dim3 grid(shm_grid_cap((size_t)n, SM_NT * SM_PX, SM_BLOCKS)), block(SM_NT);
    if ((bits & 3) == 0)
        hipLaunchKernelGGL(specmask_strength_kernel<true>, grid, block, 0, st, a, n, q, hist);
    else
        hipLaunchKernelGGL(specmask_strength_kernel<false>, grid, block, 0, st, a, n, q, hist);
    SHM_LAUNCH_CHECK(who);
    return SHM_OK;
}

int launch_otsu(const char* who, const unsigned* hist, int floor_t, int fixed_t, int* stats, hipStream_t st) {
    hipLaunchKernelGGL(specmask_otsu_kernel, dim3(1), dim3(SM_NT), 0, st, hist, floor_t, fixed_t, stats);
    SHM_LAUNCH_CHECK(who);
    return SHM_OK;
}

int launch_morph(const char* who, const unsigned char* q, int h, int w, int open_radius, int dilate_radius, unsigned char* tmp, unsigned char* mask, int* stats,
                 hipStream_t st) {
    if (int rc = clear_words(who, "pixel count", stats + 2, sizeof(int), st)) return rc;
    const int tiles_x = shm_cdiv(w, MO_TW);
    const dim3 grid((unsigned)((long long)tiles_x * shm_cdiv(h, MO_TH))), block(SM_NT);
    hipLaunchKernelGGL(specmask_morph_kernel<true>, grid, block, 0, st, q, tmp, h, w, tiles_x, open_radius, stats);
    SHM_LAUNCH_CHECK(who);
    hipLaunchKernelGGL(specmask_morph_kernel<false>, grid, block, 0, st, (const unsigned char*)tmp, mask, h, w, tiles_x, open_radius + dilate_radius, stats);
    SHM_LAUNCH_CHECK(who);
    return SHM_OK;
}

}  // namespace

extern "C" int shm_specmask_strength(const unsigned char* const* src_ptrs, int h, int w, const float* coef, unsigned char* q, unsigned* hist,
                                     void* stream) {
    const char* who = "shm_specmask_strength";
    if (int rc = check_strength(who, src_ptrs, h, w, coef, q, hist)) return rc;
    return launch_strength(who, src_ptrs, h, w, coef, q, hist, (hipStream_t)stream);
}

extern "C" int shm_specmask_otsu(const unsigned* hist, int floor_t, int fixed_t, int* stats, void* stream) {
    const char* who = "shm_specmask_otsu";
    if (int rc = check_otsu(who, hist, floor_t, fixed_t, stats)) return rc;
    return launch_otsu(who, hist, floor_t, fixed_t, stats, (hipStream_t)stream);
}

extern "C" int shm_specmask_morph(const unsigned char* q, int h, int w, int open_radius, int dilate_radius, unsigned char* tmp, unsigned char* mask,
                                  int* stats, void* stream) {
    const char* who = "shm_specmask_morph";
    if (int rc = check_morph(who, q, h, w, open_radius, dilate_radius, tmp, mask, stats)) return rc;
    return launch_morph(who, q, h, w, open_radius, dilate_radius, tmp, mask, stats, (hipStream_t)stream);
}

extern "C" int shm_specmask(const unsigned char* const* src_ptrs, int h, int w, const float* coef, int floor_t, int fixed_t, int open_radius,
                            int dilate_radius, unsigned char* q, unsigned* hist, unsigned char* tmp, unsigned char* mask, int* stats, void* stream) {
    const char* who = "shm_specmask";
    if (int rc = check_strength(who, src_ptrs, h, w, coef, q, hist)) return rc;
    if (int rc = check_otsu(who, hist, floor_t, fixed_t, stats)) return rc;
    if (int rc = check_morph(who, q, h, w, open_radius, dilate_radius, tmp, mask, stats)) return rc;
    SHM_REQUIRE(mask != q, SHM_E_SHAPE, "%s: mask and q are both results and must not share a buffer", who);
    hipStream_t st = (hipStream_t)stream;
    if (int rc = launch_strength(who, src_ptrs, h, w, coef, q, hist, st)) return rc;
    if (int rc = launch_otsu(who, hist, floor_t, fixed_t, stats, st)) return rc;
    return launch_morph(who, q, h, w, open_radius, dilate_radius, tmp, mask, stats, st);
}
