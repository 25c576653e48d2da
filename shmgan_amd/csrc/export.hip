// Image export of the reference's test mode (test.py:305-317 logs these images to Comet; here they become files): float32
// planes [S,S,C] (C in {1,3}, channel pitch ld) -> uint8 [ho,wo,C], resampled to the source photo's size and mapped to bytes.
//
//   resampling  the sampler of bilinear.h on the raw float values, in fp32; at (ho,wo) = (S,S) the pixel itself
//   value maps  RESCALE rescale_01 (utils.py:190-195, test_plot at test.py:410-425): (v - min) / (max - min), min / max over the
//               whole S*S*C source plane, divide_no_nan;  SCALE v * mul[k];  CLIP v
//   bytes       rint(clamp(t, 0, 1) * 255) in fp32, round half to even (a NaN becomes 0)
//
// Two launches at most per call, each over the ragged set of jobs (a per-job block prefix, no grid sized by the largest job):
//   min / max pass  only when some job is RESCALE: per plane nmm(S,C) blocks, each writes its (min, max) into a workspace slot
//                   of its own; min and max do not depend on the order, so the result is exact whatever the grid
//   export pass     4096 output bytes per block, four 4-byte words per lane, consecutive lanes on consecutive words; a RESCALE
//                   block first reduces its plane's partials
// A job's bytes are a function of that job alone: batch composition, job order and launch geometry do not enter.
// The job table travels as a kernel argument (SHM_EXPORT_MAX_JOBS jobs); the library allocates nothing and keeps no pointers.
//
// shm_export_u8_hw is the same two kernels on a window (y0, x0, hc, wc) of a rectangular source [hs,ws,C] (native-resolution test
// mode: the photo inside its padded frame): a job carries the pointer to the window's first pixel, the window's size and the
// frame's row pitch, so min / max and the resampling see the window only.  The square call is the window (0, 0, s, s) of pitch s.
#include "bilinear.h"

#include <limits.h>
#include <math.h>

namespace {

constexpr int EX_NT = 256;                      // threads per block, both passes
constexpr int EX_WORDS = 4;                     // 4-byte output words per lane in an export block
constexpr int EX_BLOCK_BYTES = EX_NT * EX_WORDS * 4;
constexpr int EX_MM = 32;                       // most min / max partial blocks per plane (workspace slots per job)
constexpr int EX_DIM_MAX = 32768;               // s, ho, wo

struct ExJob {
    const float* src;
    unsigned long long dst;                     // byte offset of the job's output in dst
    int blk0;                                   // first export block
    int mblk0;                                  // first min / max block (RESCALE jobs only own any)
    int pitch, hc, wc;                          // the source window: hc x wc pixels, rows `pitch` pixels apart; src is its first pixel
    int ho, wo, ld;
    int k;                                      // SCALE: index into mul
    int cmn;                                    // c | mode << 2 | nmm << 4
};

struct ExArgs {
    ExJob job[SHM_EXPORT_MAX_JOBS];
    unsigned char* dst;
    const float* mul;
    float* mm;                                  // workspace: [job][EX_MM][2] (min, max)
    int njobs;
};

int nmm_blocks(long n) {
    const int b = shm_cdiv(n, (long)EX_NT * 16);
    return b > EX_MM ? EX_MM : b;
}

// the job of block `bid`: the last one whose first block is <= bid (zero-width jobs never win: the job behind one starts at
// the same block)
__device__ __forceinline__ int find_job(const ExArgs& a, int bid, bool mm) {
    int j = 0;
    for (int i = 1; i < a.njobs; ++i)
        if ((mm ? a.job[i].mblk0 : a.job[i].blk0) <= bid) j = i;
    return j;
}

// element e of the hc x wc x c window, rows `pitch` pixels apart
__device__ __forceinline__ float load_elem(const float* src, int e, int c, int ld, int wc, int pitch) {
    const int p = c == 1 ? e : e / 3;
    if (pitch == wc) return src[(size_t)p * ld + (e - p * c)];          // whole rows (always in the square call): no second division
    const int y = p / wc;
    return src[((size_t)y * pitch + (p - y * wc)) * ld + (e - p * c)];
}

__global__ void __launch_bounds__(EX_NT) export_minmax_kernel(const ExArgs a) {
    __shared__ float red[2][EX_NT / 64];
    const int j = find_job(a, blockIdx.x, true);
    const ExJob& jb = a.job[j];
    const int c = jb.cmn & 3, nmm = jb.cmn >> 4;
    const int b = blockIdx.x - jb.mblk0;
    const int n = jb.hc * jb.wc * c;
    float lo = INFINITY, hi = -INFINITY;
    for (int e = b * EX_NT + threadIdx.x; e < n; e += nmm * EX_NT) {
        const float v = load_elem(jb.src, e, c, jb.ld, jb.wc, jb.pitch);
        lo = fminf(lo, v);
        hi = fmaxf(hi, v);
    }
    lo = shm_wave_min(lo);
    hi = shm_wave_max(hi);
    if ((threadIdx.x & 63) == 0) {
        red[0][threadIdx.x >> 6] = lo;
        red[1][threadIdx.x >> 6] = hi;
    }
    __syncthreads();
    if (threadIdx.x < 2) {
        const float* r = red[threadIdx.x];
        const float v = threadIdx.x == 0 ? fminf(fminf(r[0], r[1]), fminf(r[2], r[3]))
                                         : fmaxf(fmaxf(r[0], r[1]), fmaxf(r[2], r[3]));
        a.mm[((size_t)j * EX_MM + b) * 2 + threadIdx.x] = v;
    }
}

__device__ __forceinline__ unsigned to_byte(float t) {
    t = fminf(fmaxf(t, 0.f), 1.f);                  // fmaxf(NaN, 0) = 0
    return (unsigned)rintf(t * 255.f);
}

__global__ void __launch_bounds__(EX_NT) export_u8_kernel(const ExArgs a) {
    __shared__ float range[2];
    const int j = find_job(a, blockIdx.x, false);
    const ExJob& jb = a.job[j];
    const int c = jb.cmn & 3, mode = (jb.cmn >> 2) & 3;
    const int hc = jb.hc, wc = jb.wc, pitch = jb.pitch, ho = jb.ho, wo = jb.wo, ld = jb.ld;
    const float* src = jb.src;
    float lo = 0.f, rng = 0.f, mul = 1.f;
    if (mode == SHM_EXPORT_RESCALE) {
        if (threadIdx.x < 64) {
            const int nmm = jb.cmn >> 4;
            const float* part = a.mm + (size_t)j * EX_MM * 2;
            float l = INFINITY, h = -INFINITY;
            if ((int)threadIdx.x < nmm) {
                l = part[threadIdx.x * 2];
                h = part[threadIdx.x * 2 + 1];
            }
            l = shm_wave_min(l);
            h = shm_wave_max(h);
            if (threadIdx.x == 0) {
                range[0] = l;
                range[1] = h;
            }
        }
        __syncthreads();
        lo = range[0];
        rng = range[1] - range[0];
    } else if (mode == SHM_EXPORT_SCALE) {
        mul = a.mul[jb.k];
    }
    const bool resample = ho != hc || wo != wc;
    const float hs = (float)hc / (float)ho, ws = (float)wc / (float)wo;
    const int nbytes = ho * wo * c;
    unsigned char* out = a.dst + jb.dst;
    const int w0 = (blockIdx.x - jb.blk0) * (EX_NT * EX_WORDS) + threadIdx.x;
#pragma unroll 1
    for (int i = 0; i < EX_WORDS; ++i) {
        const int e0 = (w0 + i * EX_NT) * 4;
        if (e0 >= nbytes) break;
        int p = c == 1 ? e0 : e0 / 3;
        int ch = e0 - p * c;
        int oy = p / wo, ox = p - oy * wo;
        unsigned word = 0;
        const int nq = min(4, nbytes - e0);
        for (int q = 0; q < nq; ++q) {
            float v;
            if (resample) {
                const BilinearTaps t = bilinear_taps(ox, oy, hc, wc, pitch, hs, ws, 0.f, 0.f);
                v = bilinear_lerp(src[t.tl * ld + ch], src[t.tr * ld + ch], src[t.bl * ld + ch], src[t.br * ld + ch], t.lx, t.ly);
            } else {
                v = src[((size_t)oy * pitch + ox) * ld + ch];
            }
            const float t = mode == SHM_EXPORT_RESCALE ? (rng != 0.f ? (v - lo) / rng : 0.f)
                          : mode == SHM_EXPORT_SCALE   ? v * mul
                                                       : v;
            word |= to_byte(t) << (8 * q);
            if (++ch == c) {
                ch = 0;
                if (++ox == wo) {
                    ox = 0;
                    ++oy;
                }
            }
        }
        if (nq == 4) {
            *reinterpret_cast<unsigned*>(out + e0) = word;
        } else {
            for (int q = 0; q < nq; ++q) out[e0 + q] = (unsigned char)(word >> (8 * q));
        }
    }
}

__global__ void __launch_bounds__(64) running_scale_mean_kernel(const float* __restrict__ scale, int batch, double* acc,
                                                                float* __restrict__ mul) {
    if (threadIdx.x != 0) return;
    double sum = acc[0], cnt = acc[1];
    for (int b = 0; b < batch; ++b) {               // one thread, image order: the reference's running list
        sum += (double)scale[b];
        cnt += 1.0;
        mul[b] = (float)(sum / cnt);
    }
    acc[0] = sum;
    acc[1] = cnt;
}

// one job's checked fields into the table; blk / mblk: the running block prefixes of the two passes
void add_job(ExArgs& a, int j, const float* window, int pitch, int hc, int wc, int c, int ld, int ho, int wo, int mode, int k, size_t off,
             int& blk, int& mblk) {
    ExJob& jb = a.job[j];
    jb.src = window;
    jb.dst = off;
    jb.pitch = pitch;
    jb.hc = hc;
    jb.wc = wc;
    jb.ho = ho;
    jb.wo = wo;
    jb.ld = ld;
    jb.k = mode == SHM_EXPORT_SCALE ? k : 0;
    const int nmm = mode == SHM_EXPORT_RESCALE ? nmm_blocks((long)hc * wc * c) : 0;
    jb.cmn = c | mode << 2 | nmm << 4;
    jb.blk0 = blk;
    jb.mblk0 = mblk;
    blk += shm_cdiv((long)ho * wo * c, EX_BLOCK_BYTES);
    mblk += nmm;
}

int export_launch(const ExArgs& a, int blk, int mblk, void* stream, const char* who) {
    hipStream_t st = (hipStream_t)stream;
    if (mblk > 0) {
        hipLaunchKernelGGL(export_minmax_kernel, dim3(mblk), dim3(EX_NT), 0, st, a);
        SHM_LAUNCH_CHECK(who);
    }
    hipLaunchKernelGGL(export_u8_kernel, dim3(blk), dim3(EX_NT), 0, st, a);
    SHM_LAUNCH_CHECK(who);
    return SHM_OK;
}

}  // namespace

extern "C" size_t shm_export_u8_workspace(int njobs) {
    return njobs > 0 ? (size_t)njobs * EX_MM * 2 * sizeof(float) : 0;
}

// Both entry points: a descriptor row of `width` words is {s, c, ld, ho, wo, mode, k, off} (SHM_EXPORT_DESC: the window (0, 0, s, s) of
// an s x s plane) or {hs, ws, c, ld, y0, x0, hc, wc, ho, wo, mode, k, off} (SHM_EXPORT_HW_DESC)
static int export_entry(const char* who, int width, const float* const* src, const size_t* desc, int njobs, const float* mul, int nmul,
                        unsigned char* dst, size_t dst_bytes, void* ws, size_t ws_bytes, void* stream) {
    const bool sq = width == SHM_EXPORT_DESC;
    SHM_REQUIRE(njobs >= 1 && njobs <= SHM_EXPORT_MAX_JOBS, SHM_E_SHAPE, "%s: njobs %d outside [1, %d]", who, njobs, SHM_EXPORT_MAX_JOBS);
    SHM_REQUIRE(src && desc && dst, SHM_E_SHAPE, "%s: null pointer (src, desc or dst)", who);
    SHM_REQUIRE(((uintptr_t)dst & 3) == 0, SHM_E_SHAPE, "%s: dst is not 4-byte aligned", who);
    ExArgs a;
    a.dst = dst;
    a.mul = mul;
    a.mm = (float*)ws;
    a.njobs = njobs;
    int blk = 0, mblk = 0;
    for (int j = 0; j < njobs; ++j) {
        const size_t* d = desc + (size_t)j * width;
        const size_t hs = d[0], wsrc = sq ? d[0] : d[1], c = sq ? d[1] : d[2], ld = sq ? d[2] : d[3];
        const size_t y0 = sq ? 0 : d[4], x0 = sq ? 0 : d[5], hc = sq ? hs : d[6], wc = sq ? hs : d[7];
        const size_t* t = d + (sq ? 3 : 8);
        const size_t ho = t[0], wo = t[1], mode = t[2], k = t[3], off = t[4];
        SHM_REQUIRE(src[j], SHM_E_SHAPE, "%s: job %d: null pointer (source plane)", who, j);
        SHM_REQUIRE(c == 1 || c == 3, SHM_E_SHAPE, "%s: job %d: c %zu not in {1, 3}", who, j, c);
        const bool sizes = hs >= 1 && hs <= EX_DIM_MAX && wsrc >= 1 && wsrc <= EX_DIM_MAX && ho >= 1 && ho <= EX_DIM_MAX && wo >= 1 && wo <= EX_DIM_MAX;
        SHM_REQUIRE(sizes || !sq, SHM_E_SHAPE, "%s: job %d: sizes s %zu, ho %zu, wo %zu outside [1, %d]", who, j, hs, ho, wo, EX_DIM_MAX);
        SHM_REQUIRE(sizes, SHM_E_SHAPE, "%s: job %d: sizes hs %zu, ws %zu, ho %zu, wo %zu outside [1, %d]", who, j, hs, wsrc, ho, wo, EX_DIM_MAX);
        SHM_REQUIRE(hc >= 1 && wc >= 1 && y0 <= hs && hc <= hs - y0 && x0 <= wsrc && wc <= wsrc - x0, SHM_E_SHAPE,
                    "%s: job %d: window (%zu, %zu, %zu, %zu) outside the %zu x %zu source", who, j, y0, x0, hc, wc, hs, wsrc);
        SHM_REQUIRE(ld >= c && ld <= 65536, SHM_E_SHAPE, "%s: job %d: ld %zu outside [c, 65536]", who, j, ld);
        const size_t nbytes = ho * wo * c;
        SHM_REQUIRE(nbytes <= (size_t)INT_MAX - EX_BLOCK_BYTES && hc * wc * c <= (size_t)INT_MAX, SHM_E_SHAPE, "%s: job %d: plane too large", who, j);
        SHM_REQUIRE(mode <= SHM_EXPORT_CLIP, SHM_E_SHAPE, "%s: job %d: mode %zu unknown", who, j, mode);
        SHM_REQUIRE(mode != SHM_EXPORT_SCALE || (mul && nmul > 0 && k < (size_t)nmul), SHM_E_SHAPE, "%s: job %d: SCALE needs mul and k %zu < nmul %d",
                    who, j, k, nmul);
        SHM_REQUIRE((off & 3) == 0, SHM_E_SHAPE, "%s: job %d: destination offset %zu not a multiple of 4", who, j, off);
        SHM_REQUIRE(off <= dst_bytes && nbytes <= dst_bytes - off, SHM_E_SHAPE, "%s: job %d: destination [%zu, %zu) outside dst_bytes %zu", who, j,
                    off, off + nbytes, dst_bytes);
        add_job(a, j, src[j] + (y0 * wsrc + x0) * ld, (int)wsrc, (int)hc, (int)wc, (int)c, (int)ld, (int)ho, (int)wo, (int)mode, (int)k, off, blk,
                mblk);
    }
    const size_t need = shm_export_u8_workspace(njobs);
    SHM_REQUIRE(ws && ((uintptr_t)ws & 3) == 0 && ws_bytes >= need, SHM_E_WORKSPACE, "%s: workspace of %zu bytes (4-byte aligned) needed, %zu given",
                who, need, ws ? ws_bytes : 0);
    return export_launch(a, blk, mblk, stream, who);
}

extern "C" int shm_export_u8(const float* const* src, const size_t* desc, int njobs, const float* mul, int nmul, unsigned char* dst,
                             size_t dst_bytes, void* ws, size_t ws_bytes, void* stream) {
    return export_entry("shm_export_u8", SHM_EXPORT_DESC, src, desc, njobs, mul, nmul, dst, dst_bytes, ws, ws_bytes, stream);
}

extern "C" int shm_export_u8_hw(const float* const* src, const size_t* desc, int njobs, const float* mul, int nmul, unsigned char* dst,
                                size_t dst_bytes, void* ws, size_t ws_bytes, void* stream) {
    return export_entry("shm_export_u8_hw", SHM_EXPORT_HW_DESC, src, desc, njobs, mul, nmul, dst, dst_bytes, ws, ws_bytes, stream);
}

extern "C" int shm_running_scale_mean(const float* scale, int batch, double* acc, float* mul, void* stream) {
    SHM_REQUIRE(scale && acc && mul, SHM_E_SHAPE, "shm_running_scale_mean: null pointer");
    SHM_REQUIRE(batch >= 1, SHM_E_SHAPE, "shm_running_scale_mean: batch %d < 1", batch);
    hipLaunchKernelGGL(running_scale_mean_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, scale, batch, acc, mul);
    SHM_LAUNCH_CHECK("shm_running_scale_mean");
    return SHM_OK;
}
