// Training of the SpecSeg mask network (SpecSeg.py:27-98 built with Dropout active and BatchNormalization on batch statistics; the reference
// constructs the optimiser, SHM.py:175, and the Dice + focal loss, SpecSeg.py:92-96, and never runs them).  fp32 tensors throughout.
// The 3x3 convolutions' gradients are shm_conv2d_dgrad / shm_conv2d_wgrad, the ReLU backward is shm_lrelu_bwd at slope 0, Dropout is
// shm_keep_mask / shm_mul_mask; what is here is the rest:
//   BatchNormalization, training mode       shm_bn_train_fwd / shm_bn_train_bwd
//   MaxPooling2D(2) backward                shm_maxpool2_bwd
//   Conv2DTranspose(2x2, stride 2) backward shm_conv2d_transpose2x2_dgrad / _wgrad   (MFMA GEMMs, v_mfma_f32_16x16x4_f32, LDS-staged)
//   head: its backward, the loss            shm_head_logit_bwd / shm_seg_loss   (the logit itself, shm_head_logit_fwd, is the predict head's kernel: specseg.hip)
// The optimiser is shm_adam (color.hip).
//
// Reproducibility (the conventions of metrics.hip / telemetry.hip): every reduction keeps f64 partial sums, every block writes its partial
// into a workspace slot of its own, the slots are summed in a fixed order (slot_sum below), and no kernel uses a global atomic: results are bitwise
// reproducible from run to run.  The grid of every reduction is a function of the call's shape alone.
#include "common.h"

#include <math.h>

namespace {

constexpr int NT = 256;              // threads per block, every kernel of this file
constexpr int MAXB = SHM_SST_MAX_BLOCKS;

bool pow2_channels(int c) { return c >= 16 && c <= 256 && (c & (c - 1)) == 0; }

// ------------------------------------------------------------------------------------------- per-channel sums
// One pass over a [npix, c] tensor (pitch lda; c a power of two in 16..256), c / 4 lanes across the channels (16-byte loads) and
// 256 / (c / 4) pixels side by side; every thread sums its pixels in f64, the block sums its pixel lanes in lane order and writes
// part[block][v][c].  What is summed:
//   CS_SUM     v0 = a                                  (mean; the bias gradient of Conv2DTranspose)
//   CS_SQDEV   v0 = (a - mean)^2, mean = stat[c] f64   (second pass of the variance: nothing cancels when |mean| >> std)
//   CS_BNBWD   v0 = b, v1 = b * xhat, xhat = (a - mean) * inv_std (stat = mean [c], inv_std [c]; b = the output gradient)
//   CS_HEAD    v0 = a * b[p], v1 = b[p] (b = dz [npix], one value per pixel); also writes dx[p][c] = b[p] * w[c]
enum { CS_SUM = 0, CS_SQDEV = 1, CS_BNBWD = 2, CS_HEAD = 3 };

template <int MODE>
__global__ __launch_bounds__(NT) void chan_sums_kernel(const float* __restrict__ a, int lda, const float* __restrict__ b, int ldb,
                                                       const double* __restrict__ stat, const float* __restrict__ w, float* __restrict__ dx, int lddx,
                                                       double* __restrict__ part, size_t npix, int c) {
    constexpr int NV = MODE >= CS_BNBWD ? 2 : 1;
    __shared__ double sm[NT * 4];                     // [pixel lane][c]
    const int lanes_c = c >> 2, PP = NT / lanes_c;
    const int pp = threadIdx.x / lanes_c, cl = threadIdx.x % lanes_c;
    double s[NV][4];
#pragma unroll
    for (int v = 0; v < NV; ++v)
#pragma unroll
        for (int j = 0; j < 4; ++j) s[v][j] = 0.0;
    double mean[4] = {0.0, 0.0, 0.0, 0.0}, inv[4] = {0.0, 0.0, 0.0, 0.0};
    f32x4 wv = {0.f, 0.f, 0.f, 0.f};
    if (MODE == CS_SQDEV || MODE == CS_BNBWD)
#pragma unroll
        for (int j = 0; j < 4; ++j) mean[j] = stat[cl * 4 + j];
    if (MODE == CS_BNBWD)
#pragma unroll
        for (int j = 0; j < 4; ++j) inv[j] = stat[c + cl * 4 + j];
    if (MODE == CS_HEAD) wv = *(const f32x4*)(w + cl * 4);
    for (size_t p = (size_t)blockIdx.x * PP + pp; p < npix; p += (size_t)gridDim.x * PP) {
        const f32x4 av = *(const f32x4*)(a + p * lda + cl * 4);
        if (MODE == CS_SUM) {
#pragma unroll
            for (int j = 0; j < 4; ++j) s[0][j] += (double)av[j];
        } else if (MODE == CS_SQDEV) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const double d = (double)av[j] - mean[j];
                s[0][j] += d * d;
            }
        } else if (MODE == CS_BNBWD) {
            const f32x4 bv = *(const f32x4*)(b + p * ldb + cl * 4);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float xh = (float)(((double)av[j] - mean[j]) * inv[j]);
                s[0][j] += (double)bv[j];
                s[NV - 1][j] += (double)bv[j] * (double)xh;
            }
        } else {
            const float dz = b[p];
            f32x4 r;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                s[0][j] += (double)av[j] * (double)dz;
                s[NV - 1][j] += (double)dz;
                r[j] = dz * wv[j];
            }
            *(f32x4*)(dx + p * lddx + cl * 4) = r;
        }
    }
#pragma unroll
    for (int v = 0; v < NV; ++v) {
        __syncthreads();
#pragma unroll
        for (int j = 0; j < 4; ++j) sm[pp * c + cl * 4 + j] = s[v][j];
        __syncthreads();
        for (int ch = threadIdx.x; ch < c; ch += NT) {
            double t = 0.0;
            for (int q = 0; q < PP; ++q) t += sm[q * c + ch];
            part[((size_t)blockIdx.x * NV + v) * c + ch] = t;
        }
    }
}

int chan_blocks(size_t npix, int c) {
    const int PP = NT / (c / 4);
    return shm_grid_cap(npix, PP * 4, MAXB);
}

// Sum of value v of channel ch over the nblk slots by ONE WAVE (the finish kernels run a block of 64 threads per channel): lane i adds slots
// i, i + 64, ... in slot order, then the lanes are added by the shuffle tree of shm_wave_sum -- a fixed order for a given nblk.  Lane 0 holds
// the result.  (One thread walking 256 slots took 60-110 us per launch: a chain of dependent, uncoalesced f64 loads.)
__device__ __forceinline__ double slot_sum(const double* part, int nblk, int nv, int v, int c, int ch) {
    double t = 0.0;
    for (int i = threadIdx.x; i < nblk; i += 64) t += part[((size_t)i * nv + v) * c + ch];
    return shm_wave_sum(t);
}

// ------------------------------------------------------------------------- BatchNormalization, training mode
// stage 0: save[ch] = mean.  stage 1: save[c + ch] = 1 / sqrt(var + eps) and the moving statistics.
__global__ __launch_bounds__(64) void bn_fwd_finish_kernel(const double* __restrict__ part, int nblk, int stage, double* __restrict__ save, float* __restrict__ mmean,
                                     float* __restrict__ mvar, double momentum, double eps, double n, int c) {
    const int ch = blockIdx.x;
    const double t = slot_sum(part, nblk, 1, 0, c, ch) / n;
    if (threadIdx.x != 0) return;
    if (stage == 0) {
        save[ch] = t;
        return;
    }
    save[c + ch] = 1.0 / sqrt(t + eps);
    if (mmean) mmean[ch] = (float)((double)mmean[ch] * momentum + save[ch] * (1.0 - momentum));
    // TensorFlow's fused kernel feeds the moving variance the unbiased estimate (Bessel's correction), and the biased one to the output
    if (mvar) mvar[ch] = (float)((double)mvar[ch] * momentum + t * (n / fmax(n - 1.0, 1.0)) * (1.0 - momentum));
}

__global__ __launch_bounds__(NT) void bn_train_apply_kernel(const float* __restrict__ a, int lda, const float* __restrict__ gamma, const float* __restrict__ beta,
                                                            const double* __restrict__ save, float* __restrict__ out, int ldo, size_t npix, int c) {
    const int c4 = c >> 2;
    const size_t total = npix * c4;
    for (size_t i = (size_t)blockIdx.x * NT + threadIdx.x; i < total; i += (size_t)gridDim.x * NT) {
        const size_t p = i / c4;
        const int ch = (int)(i % c4) * 4;
        const f32x4 v = *(const f32x4*)(a + p * lda + ch);
        f32x4 r;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float xh = (float)(((double)v[j] - save[ch + j]) * save[c + ch + j]);
            r[j] = xh * gamma[ch + j] + beta[ch + j];
        }
        *(f32x4*)(out + p * ldo + ch) = r;
    }
}

// dgamma = sum dy * xhat, dbeta = sum dy; the two sums stay in stat[2c] (f64) for the apply pass
__global__ __launch_bounds__(64) void bn_bwd_finish_kernel(const double* __restrict__ part, int nblk, double* __restrict__ stat, float* __restrict__ dgamma, float* __restrict__ dbeta, int c) {
    const int ch = blockIdx.x;
    const double s0 = slot_sum(part, nblk, 2, 0, c, ch), s1 = slot_sum(part, nblk, 2, 1, c, ch);
    if (threadIdx.x != 0) return;
    stat[ch] = s0;
    stat[c + ch] = s1;
    dbeta[ch] = (float)s0;
    dgamma[ch] = (float)s1;
}

// dx = gamma * inv_std * (dy - mean(dy) - xhat * mean(dy * xhat))
__global__ __launch_bounds__(NT) void bn_train_bwd_apply_kernel(const float* __restrict__ dy, int lddy, const float* __restrict__ a, int lda,
                                                                const float* __restrict__ gamma, const double* __restrict__ save, const double* __restrict__ stat,
                                                                float* __restrict__ dx, int lddx, size_t npix, int c) {
    const int c4 = c >> 2;
    const size_t total = npix * c4;
    const double rn = 1.0 / (double)npix;
    for (size_t i = (size_t)blockIdx.x * NT + threadIdx.x; i < total; i += (size_t)gridDim.x * NT) {
        const size_t p = i / c4;
        const int ch = (int)(i % c4) * 4;
        const f32x4 g = *(const f32x4*)(dy + p * lddy + ch);
        const f32x4 v = *(const f32x4*)(a + p * lda + ch);
        f32x4 r;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const double inv = save[c + ch + j];
            const float xh = (float)(((double)v[j] - save[ch + j]) * inv);
            const float k1 = (float)(stat[ch + j] * rn), k2 = (float)(stat[c + ch + j] * rn);
            r[j] = gamma[ch + j] * (float)inv * (g[j] - k1 - xh * k2);
        }
        *(f32x4*)(dx + p * lddx + ch) = r;
    }
}

// ----------------------------------------------------------------------------------- MaxPooling2D(2) backward
// the window's gradient goes to its FIRST maximum in row-major order ((0,0), (0,1), (1,0), (1,1)): strict comparisons
__global__ __launch_bounds__(NT) void maxpool2_bwd_kernel(const float* __restrict__ x, int ldx, const float* __restrict__ dy, int lddy, float* __restrict__ dx,
                                                          int lddx, int h, int w, int c4, size_t total, int accumulate) {
    for (size_t i = (size_t)blockIdx.x * NT + threadIdx.x; i < total; i += (size_t)gridDim.x * NT) {
        const int cl = (int)(i % c4);
        const size_t q = i / c4;
        const int wo = w >> 1, ho = h >> 1;
        const int ox = (int)(q % wo);
        const size_t t = q / wo;
        const int oy = (int)(t % ho);
        const size_t n = t / ho;
        const size_t pix = (n * h + 2 * oy) * w + 2 * ox;
        const size_t off[4] = {pix, pix + 1, pix + w, pix + w + 1};
        f32x4 v[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = *(const f32x4*)(x + off[k] * ldx + cl * 4);
        const f32x4 g = *(const f32x4*)(dy + q * lddy + cl * 4);
        f32x4 r[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            int best = 0;
            float m = v[0][j];
#pragma unroll
            for (int k = 1; k < 4; ++k)
                if (v[k][j] > m) {
                    m = v[k][j];
                    best = k;
                }
#pragma unroll
            for (int k = 0; k < 4; ++k) r[k][j] = best == k ? g[j] : 0.f;
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            float* d = dx + off[k] * lddx + cl * 4;
            if (accumulate) {
                const f32x4 o = *(const f32x4*)d;
#pragma unroll
                for (int j = 0; j < 4; ++j) r[k][j] += o[j];
            }
            *(f32x4*)d = r[k];
        }
    }
}

// --------------------------------------------------------------------- Conv2DTranspose(2x2, stride 2) backward
// Input gradient: dx[m][ci] = sum_k A[m][k] W[k][ci], m = (n, a, b), k = (p, q, co), A[m][k] = dy[n][2a + p][2b + q][co] and W = the kernel as
// stored ([2][2][cout][cin] = [4 cout][cin]).  Block tile 64 rows x 32 columns, four waves of 16 rows x 32 columns (two 16x16x4 accumulators),
// K in steps of 16 (cout % 16 == 0: a step stays inside one (p, q)), both operand tiles staged in LDS.
__global__ __launch_bounds__(NT) void convt2_dgrad_kernel(const float* __restrict__ dy, int lddy, const float* __restrict__ w, float* __restrict__ dx, int lddx,
                                                          int hi, int wi, int cin, int cout, size_t M) {
    __shared__ float As[64][17];
    __shared__ float Bs[16][33];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, l15 = lane & 15, lq = lane >> 4;
    const size_t m0 = (size_t)blockIdx.x * 64;
    const int n0 = blockIdx.y * 32;
    const int ar = tid >> 2, ac = (tid & 3) * 4;
    const size_t m = m0 + ar;
    const bool ok = m < M;
    const float* arow = dy;
    if (ok) {
        const int bb = (int)(m % wi);
        const size_t t = m / wi;
        const int aa = (int)(t % hi);
        const size_t n = t / hi;
        arow = dy + ((n * 2 * hi + 2 * aa) * (size_t)(2 * wi) + 2 * bb) * lddy + ac;
    }
    const int br = tid >> 3, bc = (tid & 7) * 4;
    f32x4 acc[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
    const int K = 4 * cout;
    for (int k0 = 0; k0 < K; k0 += 16) {
        const int pq = k0 / cout, co0 = k0 % cout;
        f32x4 av = {0.f, 0.f, 0.f, 0.f}, bv = {0.f, 0.f, 0.f, 0.f};
        if (ok) av = *(const f32x4*)(arow + ((size_t)(pq >> 1) * 2 * wi + (pq & 1)) * lddy + co0);
        if (tid < 128) bv = *(const f32x4*)(w + (size_t)(k0 + br) * cin + n0 + bc);
        __syncthreads();                      // the previous step's fragment reads are done
#pragma unroll
        for (int j = 0; j < 4; ++j) As[ar][ac + j] = av[j];
        if (tid < 128)
#pragma unroll
            for (int j = 0; j < 4; ++j) Bs[br][bc + j] = bv[j];
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) {
            const float af = As[wave * 16 + l15][kk * 4 + lq];
#pragma unroll
            for (int j = 0; j < 2; ++j) acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(af, Bs[kk * 4 + lq][j * 16 + l15], acc[j], 0, 0, 0);
        }
    }
    // accumulator register r = row 4 lq + r, column l15
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const size_t row = m0 + wave * 16 + lq * 4 + r;
            if (row < M) dx[row * lddx + n0 + j * 16 + l15] = acc[j][r];
        }
}

// Weight gradient: for each (p, q) the cout x cin product dk[p][q][co][ci] = sum_m dy[n][2a + p][2b + q][co] x[m][ci] over K = M = batch hi wi.
// grid (tiles of 16 co x 32 ci, 4 (p, q), nsplit): a block walks its split's 64-pixel chunks, both tiles staged in LDS; its four waves take
// 16 pixels of the chunk each and their accumulators are summed through LDS in wave order.  part[split][p][q][cout][cin]; the splits are
// summed in split order by convt2_wgrad_reduce_kernel.
__global__ __launch_bounds__(NT) void convt2_wgrad_kernel(const float* __restrict__ x, int ldx, const float* __restrict__ dy, int lddy, float* __restrict__ part,
                                                          int hi, int wi, int cin, int cout, size_t M, int nchunks, int cps) {
    __shared__ __attribute__((aligned(16))) float Ds[64][16];
    __shared__ __attribute__((aligned(16))) float Xs[64][32];
    __shared__ float Rs[4][16 * 32];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, l15 = lane & 15, lq = lane >> 4;
    const int tco = blockIdx.x % (cout / 16), tci = blockIdx.x / (cout / 16);
    const int co0 = tco * 16, ci0 = tci * 32, pq = blockIdx.y, split = blockIdx.z;
    const int dr = tid >> 2, dc = (tid & 3) * 4;
    f32x4 acc[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
    const int cbeg = split * cps, cend = min(cbeg + cps, nchunks);
    for (int ch = cbeg; ch < cend; ++ch) {
        const size_t mb = (size_t)ch * 64;
        f32x4 dv = {0.f, 0.f, 0.f, 0.f}, xv[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
        const size_t m = mb + dr;
        if (m < M) {
            const int bb = (int)(m % wi);
            const size_t t = m / wi;
            const int aa = (int)(t % hi);
            const size_t n = t / hi;
            dv = *(const f32x4*)(dy + ((n * 2 * hi + 2 * aa + (pq >> 1)) * (size_t)(2 * wi) + 2 * bb + (pq & 1)) * lddy + co0 + dc);
        }
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int idx = tid + NT * i, xr = idx >> 3, xc = (idx & 7) * 4;
            if (mb + xr < M) xv[i] = *(const f32x4*)(x + (mb + xr) * ldx + ci0 + xc);
        }
        __syncthreads();                      // the previous chunk's fragment reads are done
        *(f32x4*)&Ds[dr][dc] = dv;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int idx = tid + NT * i;
            *(f32x4*)&Xs[idx >> 3][(idx & 7) * 4] = xv[i];
        }
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) {
            const int k = wave * 16 + kk * 4 + lq;
            const float af = Ds[k][l15];
#pragma unroll
            for (int j = 0; j < 2; ++j) acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(af, Xs[k][j * 16 + l15], acc[j], 0, 0, 0);
        }
    }
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) Rs[wave][(lq * 4 + r) * 32 + j * 16 + l15] = acc[j][r];
    __syncthreads();
    for (int e = tid; e < 16 * 32; e += NT) {
        const float s = ((Rs[0][e] + Rs[1][e]) + Rs[2][e]) + Rs[3][e];
        const int co = e >> 5, ci = e & 31;
        part[(((size_t)split * 4 + pq) * cout + co0 + co) * cin + ci0 + ci] = s;
    }
}

__global__ void convt2_wgrad_reduce_kernel(const float* __restrict__ part, float* __restrict__ dw, size_t n, int nsplit) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        float s = part[i];
        for (int k = 1; k < nsplit; ++k) s += part[(size_t)k * n + i];
        dw[i] = s;
    }
}

// out[ch] = sum of value v of the slots, in slot order (the Conv2DTranspose bias gradient, the head's dw and db)
__global__ __launch_bounds__(64) void chan_finish_kernel(const double* __restrict__ part, int nblk, int nv, int v, int c, float* __restrict__ out) {
    const int ch = blockIdx.x;          // grid = nout blocks of one wave
    const double t = slot_sum(part, nblk, nv, v, c, ch);
    if (threadIdx.x == 0) out[ch] = (float)t;
}

struct Convt2WgradPlan {
    int nchunks, nsplit, cps;
    size_t bias_bytes, total;
};

Convt2WgradPlan plan_convt2_wgrad(int batch, int hi, int wi, int cin, int cout) {
    Convt2WgradPlan p;
    const size_t M = (size_t)batch * hi * wi;
    p.nchunks = (int)((M + 63) / 64);
    int ns = p.nchunks < 32 ? p.nchunks : 32;
    if (ns < 1) ns = 1;
    p.cps = (p.nchunks + ns - 1) / ns;
    if (p.cps < 1) p.cps = 1;
    p.nsplit = p.nchunks > 0 ? (p.nchunks + p.cps - 1) / p.cps : 1;
    p.bias_bytes = (size_t)MAXB * cout * sizeof(double);
    p.total = p.bias_bytes + (size_t)p.nsplit * 4 * cout * cin * sizeof(float);
    return p;
}

// ------------------------------------------------------------------------------------------- head and loss
// Per pixel, from the logit z and the target g, all in f64: p = sigmoid(z), q = 1 - p = sigmoid(-z), log p = -softplus(-z), log q = -softplus(z)
// (finite at |z| = 40, where 1 - p rounds to 0 in fp32 and log(1 - p) would be -inf)
struct SegPix {
    double p, q, lp, lq;
};
__device__ __forceinline__ SegPix seg_pix(float zf) {
    const double z = (double)zf, e = exp(-fabs(z)), l = log1p(e), r = 1.0 / (1.0 + e);
    SegPix s;
    s.p = z >= 0.0 ? r : e * r;
    s.q = z >= 0.0 ? e * r : r;
    s.lp = -(fmax(-z, 0.0) + l);
    s.lq = -(fmax(z, 0.0) + l);
    return s;
}

constexpr int SEG_NV = 7;        // sum g p, sum p, sum g, sum focal, tp, fp, fn
constexpr double SEG_SMOOTH = 1e-5, FOCAL_ALPHA = 0.25;

__global__ __launch_bounds__(NT) void seg_loss_sums_kernel(const float* __restrict__ z, const float* __restrict__ g, double* __restrict__ part, size_t npix) {
    double s[SEG_NV];
#pragma unroll
    for (int k = 0; k < SEG_NV; ++k) s[k] = 0.0;
    for (size_t i = (size_t)blockIdx.x * NT + threadIdx.x; i < npix; i += (size_t)gridDim.x * NT) {
        const SegPix x = seg_pix(z[i]);
        const double gt = (double)g[i], on = z[i] > 0.f ? 1.0 : 0.0;          // p > 0.5 <=> z > 0
        s[0] += gt * x.p;
        s[1] += x.p;
        s[2] += gt;
        s[3] += -gt * FOCAL_ALPHA * x.q * x.q * x.lp - (1.0 - gt) * (1.0 - FOCAL_ALPHA) * x.p * x.p * x.lq;
        s[4] += gt * on;
        s[5] += (1.0 - gt) * on;
        s[6] += gt * (1.0 - on);
    }
#pragma unroll
    for (int k = 0; k < SEG_NV; ++k) {
        const double t = shm_block_sum<NT>(s[k]);
        if (threadIdx.x == 0) part[(size_t)blockIdx.x * SEG_NV + k] = t;
    }
}

// one block: tot[7] = the slots summed (every thread a fixed stride of slots in slot order, then the block in thread order);
// out = {loss, dice, focal, iou, f1, tp, fp, fn}
__global__ __launch_bounds__(NT) void seg_loss_finish_kernel(const double* __restrict__ part, int nblk, double* __restrict__ tot, double* __restrict__ out, double n) {
    double t[SEG_NV];
#pragma unroll
    for (int k = 0; k < SEG_NV; ++k) {
        double a = 0.0;
        for (int i = threadIdx.x; i < nblk; i += NT) a += part[(size_t)i * SEG_NV + k];
        t[k] = shm_block_sum<NT>(a);
    }
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < SEG_NV; ++k) tot[k] = t[k];
        const double dice = 1.0 - (2.0 * t[0] + SEG_SMOOTH) / (t[1] + t[2] + SEG_SMOOTH);
        const double focal = t[3] / n;
        out[0] = dice + focal;
        out[1] = dice;
        out[2] = focal;
        out[3] = (t[4] + SEG_SMOOTH) / (t[4] + t[5] + t[6] + SEG_SMOOTH);
        out[4] = (2.0 * t[4] + SEG_SMOOTH) / (2.0 * t[4] + t[5] + t[6] + SEG_SMOOTH);
        out[5] = t[4];
        out[6] = t[5];
        out[7] = t[6];
    }
}

__global__ __launch_bounds__(NT) void seg_loss_grad_kernel(const float* __restrict__ z, const float* __restrict__ g, const double* __restrict__ tot,
                                                           float* __restrict__ dz, size_t npix) {
    const double I2 = 2.0 * tot[0] + SEG_SMOOTH, D = tot[1] + tot[2] + SEG_SMOOTH, rn = 1.0 / (double)npix;
    for (size_t i = (size_t)blockIdx.x * NT + threadIdx.x; i < npix; i += (size_t)gridDim.x * NT) {
        const SegPix x = seg_pix(z[i]);
        const double gt = (double)g[i], pq = x.p * x.q;
        const double ddice = -(2.0 * gt * D - I2) / (D * D) * pq;
        const double dpos = x.q * x.q * x.q - 2.0 * x.p * x.q * x.q * x.lp;          // d/dz (1-p)^2 log p
        const double dneg = 2.0 * x.p * x.p * x.q * x.lq - x.p * x.p * x.p;          // d/dz p^2 log(1-p)
        const double dfocal = (-gt * FOCAL_ALPHA * dpos - (1.0 - gt) * (1.0 - FOCAL_ALPHA) * dneg) * rn;
        dz[i] = (float)(ddice + dfocal);
    }
}

}  // namespace

// ====================================================================================================== entry points
#define CHAN_SUMS(MODE, nblk, st, ...) hipLaunchKernelGGL(chan_sums_kernel<MODE>, dim3(nblk), dim3(NT), 0, st, __VA_ARGS__)

extern "C" int shm_bn_train_fwd(const float* a, int lda, const float* gamma, const float* beta, float* moving_mean, float* moving_var, float momentum,
                                float eps, float* out, int ldo, double* save, double* ws, size_t ws_bytes, size_t npix, int c, void* stream) {
    SHM_REQUIRE(a && gamma && beta && out && save && ws, SHM_E_SHAPE, "shm_bn_train_fwd: null pointer");
    SHM_REQUIRE(pow2_channels(c), SHM_E_SHAPE, "shm_bn_train_fwd: channels %d not a power of two in 16..256", c);
    SHM_REQUIRE(lda % 4 == 0 && ldo % 4 == 0 && lda >= c && ldo >= c, SHM_E_SHAPE, "shm_bn_train_fwd: pitches %d / %d must be multiples of 4, at least %d", lda, ldo, c);
    SHM_REQUIRE(npix >= 1, SHM_E_SHAPE, "shm_bn_train_fwd: no pixels");
    SHM_REQUIRE(ws_bytes >= SHM_BN_TRAIN_WS_DOUBLES(c) * sizeof(double), SHM_E_WORKSPACE, "shm_bn_train_fwd: workspace %zu < %zu bytes", ws_bytes,
                (size_t)SHM_BN_TRAIN_WS_DOUBLES(c) * sizeof(double));
    hipStream_t st = (hipStream_t)stream;
    const int nblk = chan_blocks(npix, c), fb = c;          // the finish kernels: one wave per channel
    const float* nf = nullptr;
    float* nfm = nullptr;
    CHAN_SUMS(CS_SUM, nblk, st, a, lda, nf, 0, (const double*)nullptr, nf, nfm, 0, ws, npix, c);
    SHM_LAUNCH_CHECK("shm_bn_train_fwd");
    hipLaunchKernelGGL(bn_fwd_finish_kernel, dim3(fb), dim3(64), 0, st, ws, nblk, 0, save, moving_mean, moving_var, (double)momentum, (double)eps, (double)npix, c);
    SHM_LAUNCH_CHECK("shm_bn_train_fwd");
    CHAN_SUMS(CS_SQDEV, nblk, st, a, lda, nf, 0, (const double*)save, nf, nfm, 0, ws, npix, c);
    SHM_LAUNCH_CHECK("shm_bn_train_fwd");
    hipLaunchKernelGGL(bn_fwd_finish_kernel, dim3(fb), dim3(64), 0, st, ws, nblk, 1, save, moving_mean, moving_var, (double)momentum, (double)eps, (double)npix, c);
    SHM_LAUNCH_CHECK("shm_bn_train_fwd");
    hipLaunchKernelGGL(bn_train_apply_kernel, dim3(shm_grid_cap(npix * (c / 4), NT, 8192)), dim3(NT), 0, st, a, lda, gamma, beta, (const double*)save, out, ldo, npix, c);
    SHM_LAUNCH_CHECK("shm_bn_train_fwd");
    return SHM_OK;
}

extern "C" int shm_bn_train_bwd(const float* dy, int lddy, const float* a, int lda, const float* gamma, const double* save, float* dx, int lddx,
                                float* dgamma, float* dbeta, double* ws, size_t ws_bytes, size_t npix, int c, void* stream) {
    SHM_REQUIRE(dy && a && gamma && save && dx && dgamma && dbeta && ws, SHM_E_SHAPE, "shm_bn_train_bwd: null pointer");
    SHM_REQUIRE(pow2_channels(c), SHM_E_SHAPE, "shm_bn_train_bwd: channels %d not a power of two in 16..256", c);
    SHM_REQUIRE(lddy % 4 == 0 && lda % 4 == 0 && lddx % 4 == 0 && lddy >= c && lda >= c && lddx >= c, SHM_E_SHAPE,
                "shm_bn_train_bwd: pitches %d / %d / %d must be multiples of 4, at least %d", lddy, lda, lddx, c);
    SHM_REQUIRE(npix >= 1, SHM_E_SHAPE, "shm_bn_train_bwd: no pixels");
    SHM_REQUIRE(ws_bytes >= SHM_BN_TRAIN_WS_DOUBLES(c) * sizeof(double), SHM_E_WORKSPACE, "shm_bn_train_bwd: workspace %zu < %zu bytes", ws_bytes,
                (size_t)SHM_BN_TRAIN_WS_DOUBLES(c) * sizeof(double));
    hipStream_t st = (hipStream_t)stream;
    const int nblk = chan_blocks(npix, c);
    double* stat = ws + (size_t)MAXB * 2 * c;
    const float* nf = nullptr;
    float* nfm = nullptr;
    CHAN_SUMS(CS_BNBWD, nblk, st, a, lda, dy, lddy, save, nf, nfm, 0, ws, npix, c);
    SHM_LAUNCH_CHECK("shm_bn_train_bwd");
    hipLaunchKernelGGL(bn_bwd_finish_kernel, dim3(c), dim3(64), 0, st, (const double*)ws, nblk, stat, dgamma, dbeta, c);
    SHM_LAUNCH_CHECK("shm_bn_train_bwd");
    hipLaunchKernelGGL(bn_train_bwd_apply_kernel, dim3(shm_grid_cap(npix * (c / 4), NT, 8192)), dim3(NT), 0, st, dy, lddy, a, lda, gamma, save, (const double*)stat, dx,
                       lddx, npix, c);
    SHM_LAUNCH_CHECK("shm_bn_train_bwd");
    return SHM_OK;
}

extern "C" int shm_maxpool2_bwd(const float* x, int ldx, const float* dy, int lddy, float* dx, int lddx, int batch, int h, int w, int c, int accumulate,
                                void* stream) {
    SHM_REQUIRE(x && dy && dx, SHM_E_SHAPE, "shm_maxpool2_bwd: null pointer");
    SHM_REQUIRE(c >= 4 && c % 4 == 0 && ldx % 4 == 0 && lddy % 4 == 0 && lddx % 4 == 0 && ldx >= c && lddy >= c && lddx >= c, SHM_E_SHAPE,
                "shm_maxpool2_bwd: channels/pitch must be multiples of 4, pitch >= channels");
    SHM_REQUIRE(batch >= 1 && h >= 2 && w >= 2 && h % 2 == 0 && w % 2 == 0, SHM_E_SHAPE, "shm_maxpool2_bwd: bad size %d x %d x %d", batch, h, w);
    const size_t total = (size_t)batch * (h / 2) * (w / 2) * (c / 4);
    hipLaunchKernelGGL(maxpool2_bwd_kernel, dim3(shm_grid_cap(total, NT, 8192)), dim3(NT), 0, (hipStream_t)stream, x, ldx, dy, lddy, dx, lddx, h, w, c / 4, total,
                       accumulate);
    SHM_LAUNCH_CHECK("shm_maxpool2_bwd");
    return SHM_OK;
}

static int convt2_shape_ok(const char* who, int batch, int hi, int wi, int cin, int cout) {
    SHM_REQUIRE(batch >= 1 && hi >= 1 && wi >= 1 && hi <= 16384 && wi <= 16384, SHM_E_SHAPE, "%s: bad size %d x %d x %d", who, batch, hi, wi);
    SHM_REQUIRE(cout >= 16 && cout % 16 == 0 && cin >= 32 && cin % 32 == 0 && cout <= 1024 && cin <= 2048, SHM_E_SHAPE,
                "%s: cout %d must be a multiple of 16, cin %d a multiple of 32", who, cout, cin);
    return SHM_OK;
}

extern "C" int shm_conv2d_transpose2x2_dgrad(const float* dy, int lddy, const float* w, float* dx, int lddx, int batch, int hi, int wi, int cin, int cout,
                                             void* stream) {
    SHM_REQUIRE(dy && w && dx, SHM_E_SHAPE, "shm_conv2d_transpose2x2_dgrad: null pointer");
    int r = convt2_shape_ok("shm_conv2d_transpose2x2_dgrad", batch, hi, wi, cin, cout);
    if (r) return r;
    SHM_REQUIRE(lddy % 4 == 0 && lddy >= cout && lddx >= cin, SHM_E_SHAPE, "shm_conv2d_transpose2x2_dgrad: pitches %d / %d", lddy, lddx);
    const size_t M = (size_t)batch * hi * wi;
    SHM_REQUIRE((M + 63) / 64 <= 0x7fffffffu, SHM_E_SHAPE, "shm_conv2d_transpose2x2_dgrad: too many pixels");
    hipLaunchKernelGGL(convt2_dgrad_kernel, dim3((unsigned)((M + 63) / 64), cin / 32), dim3(NT), 0, (hipStream_t)stream, dy, lddy, w, dx, lddx, hi, wi, cin, cout, M);
    SHM_LAUNCH_CHECK("shm_conv2d_transpose2x2_dgrad");
    return SHM_OK;
}

extern "C" size_t shm_conv2d_transpose2x2_wgrad_workspace(int batch, int hi, int wi, int cin, int cout) {
    if (batch < 1 || hi < 1 || wi < 1 || cin < 1 || cout < 1) return 0;
    return plan_convt2_wgrad(batch, hi, wi, cin, cout).total;
}

extern "C" int shm_conv2d_transpose2x2_wgrad(const float* x, int ldx, const float* dy, int lddy, float* dw, float* dbias, void* ws, size_t ws_bytes, int batch,
                                             int hi, int wi, int cin, int cout, void* stream) {
    SHM_REQUIRE(x && dy && dw && ws, SHM_E_SHAPE, "shm_conv2d_transpose2x2_wgrad: null pointer");
    int r = convt2_shape_ok("shm_conv2d_transpose2x2_wgrad", batch, hi, wi, cin, cout);
    if (r) return r;
    SHM_REQUIRE(ldx % 4 == 0 && lddy % 4 == 0 && ldx >= cin && lddy >= cout, SHM_E_SHAPE, "shm_conv2d_transpose2x2_wgrad: pitches %d / %d", ldx, lddy);
    SHM_REQUIRE(!dbias || pow2_channels(cout), SHM_E_SHAPE, "shm_conv2d_transpose2x2_wgrad: the bias gradient takes cout a power of two in 16..256, got %d", cout);
    const Convt2WgradPlan p = plan_convt2_wgrad(batch, hi, wi, cin, cout);
    SHM_REQUIRE(ws_bytes >= p.total, SHM_E_WORKSPACE, "shm_conv2d_transpose2x2_wgrad: workspace %zu < %zu bytes", ws_bytes, p.total);
    hipStream_t st = (hipStream_t)stream;
    const size_t M = (size_t)batch * hi * wi;
    float* part = (float*)((char*)ws + p.bias_bytes);
    hipLaunchKernelGGL(convt2_wgrad_kernel, dim3((cout / 16) * (cin / 32), 4, p.nsplit), dim3(NT), 0, st, x, ldx, dy, lddy, part, hi, wi, cin, cout, M, p.nchunks,
                       p.cps);
    SHM_LAUNCH_CHECK("shm_conv2d_transpose2x2_wgrad");
    const size_t n = (size_t)4 * cout * cin;
    hipLaunchKernelGGL(convt2_wgrad_reduce_kernel, dim3(shm_grid_cap(n, NT, 4096)), dim3(NT), 0, st, (const float*)part, dw, n, p.nsplit);
    SHM_LAUNCH_CHECK("shm_conv2d_transpose2x2_wgrad");
    if (dbias) {
        double* bp = (double*)ws;
        const size_t opix = M * 4;
        const int nblk = chan_blocks(opix, cout);
        const float* nf = nullptr;
        float* nfm = nullptr;
        CHAN_SUMS(CS_SUM, nblk, st, dy, lddy, nf, 0, (const double*)nullptr, nf, nfm, 0, bp, opix, cout);
        SHM_LAUNCH_CHECK("shm_conv2d_transpose2x2_wgrad");
        hipLaunchKernelGGL(chan_finish_kernel, dim3(cout), dim3(64), 0, st, (const double*)bp, nblk, 1, 0, cout, dbias);
        SHM_LAUNCH_CHECK("shm_conv2d_transpose2x2_wgrad");
    }
    return SHM_OK;
}

extern "C" int shm_head_logit_bwd(const float* x, int ldx, const float* w, const float* dz, float* dx, int lddx, float* dw, float* db, double* ws,
                                  size_t ws_bytes, size_t npix, int c, void* stream) {
    SHM_REQUIRE(x && w && dz && dx && dw && db && ws, SHM_E_SHAPE, "shm_head_logit_bwd: null pointer");
    SHM_REQUIRE(pow2_channels(c) && ldx % 4 == 0 && lddx % 4 == 0 && ldx >= c && lddx >= c, SHM_E_SHAPE, "shm_head_logit_bwd: channels %d / pitches %d, %d unsupported",
                c, ldx, lddx);
    SHM_REQUIRE(npix >= 1, SHM_E_SHAPE, "shm_head_logit_bwd: no pixels");
    SHM_REQUIRE(ws_bytes >= SHM_BN_TRAIN_WS_DOUBLES(c) * sizeof(double), SHM_E_WORKSPACE, "shm_head_logit_bwd: workspace %zu < %zu bytes", ws_bytes,
                (size_t)SHM_BN_TRAIN_WS_DOUBLES(c) * sizeof(double));
    hipStream_t st = (hipStream_t)stream;
    const int nblk = chan_blocks(npix, c);
    CHAN_SUMS(CS_HEAD, nblk, st, x, ldx, dz, 1, (const double*)nullptr, w, dx, lddx, ws, npix, c);
    SHM_LAUNCH_CHECK("shm_head_logit_bwd");
    hipLaunchKernelGGL(chan_finish_kernel, dim3(c), dim3(64), 0, st, (const double*)ws, nblk, 2, 0, c, dw);
    SHM_LAUNCH_CHECK("shm_head_logit_bwd");
    hipLaunchKernelGGL(chan_finish_kernel, dim3(1), dim3(64), 0, st, (const double*)ws, nblk, 2, 1, c, db);
    SHM_LAUNCH_CHECK("shm_head_logit_bwd");
    return SHM_OK;
}

extern "C" int shm_seg_loss(const float* z, const float* g, float* dz, double* out, double* ws, size_t ws_bytes, size_t npix, void* stream) {
    SHM_REQUIRE(z && g && out && ws, SHM_E_SHAPE, "shm_seg_loss: null pointer");
    SHM_REQUIRE(npix >= 1, SHM_E_SHAPE, "shm_seg_loss: no pixels");
    SHM_REQUIRE(ws_bytes >= SHM_SEG_LOSS_WS_DOUBLES * sizeof(double), SHM_E_WORKSPACE, "shm_seg_loss: workspace %zu < %zu bytes", ws_bytes,
                (size_t)SHM_SEG_LOSS_WS_DOUBLES * sizeof(double));
    hipStream_t st = (hipStream_t)stream;
    const int nblk = shm_grid_cap(npix, NT * 4, MAXB);
    double* tot = ws + (size_t)MAXB * SEG_NV;
    hipLaunchKernelGGL(seg_loss_sums_kernel, dim3(nblk), dim3(NT), 0, st, z, g, ws, npix);
    SHM_LAUNCH_CHECK("shm_seg_loss");
    hipLaunchKernelGGL(seg_loss_finish_kernel, dim3(1), dim3(NT), 0, st, (const double*)ws, nblk, tot, out, (double)npix);
    SHM_LAUNCH_CHECK("shm_seg_loss");
    if (dz) {
        hipLaunchKernelGGL(seg_loss_grad_kernel, dim3(shm_grid_cap(npix, NT, 8192)), dim3(NT), 0, st, z, g, (const double*)tot, dz, npix);
        SHM_LAUNCH_CHECK("shm_seg_loss");
    }
    return SHM_OK;
}
