// Training telemetry (the reference's loss scalars every 25 steps and gradient histograms every 100, SHM.py:1035-1053, 1085-1091):
//   shm_tensor_stats   per-variable statistics and a sign / exponent histogram of a flat fp32 buffer (P.grad or P.flat of a model)
//   shm_loss_ring_put  one step's raw loss vectors into a row of a device ring
//
// shm_tensor_stats, two launches whatever the number of segments:
//   chunk pass  one block per TS_CHUNK floats of one segment.  Chunks are cut relative to the segment's start, and the segment table
//               travels in the kernel arguments (a block finds its segment by bisection over the chunk prefix), so nothing is uploaded
//               and nothing is kept between calls.  Per value: one fp32 multiply by `scale`, a class from the bits (header), one LDS
//               integer add into the block's histogram, and per-thread min / max / f64 sum / f64 sum of squares.  Gradient values sit in
//               a handful of exponents, so most lanes of a wave want the same bin (HIP guide, guideline 12): the histogram is kept in 32
//               copies, lane l adds into copy l mod 32, and copy c of every bin lies in LDS bank c -- no two lanes of an instruction
//               meet in a bank whatever the data.  The copies are added per bin and the chunk's partial goes to a workspace slot of
//               its own: no global atomics, nothing to zero beforehand.
//   finalize    one block per segment: adds the segment's slots (the f64 sums in chunk order: every thread a fixed stride of slots, then
//               the block in thread order, the convention of metrics.hip), so a segment's result depends on that segment alone.
// The kernels only read x.  Denormals are kept (hipcc's default for gfx9 fp32), so min / max / sums see a subnormal as numpy does.
#include "common.h"

namespace {

constexpr int TS_NT = 256;                      // threads per block of the chunk pass
constexpr int TS_WAVES = TS_NT / 64;
constexpr int TS_VEC = 8;                       // 16-byte loads per thread
constexpr int TS_CHUNK = TS_NT * TS_VEC * 4;    // 8192 floats per block
constexpr int TS_COPIES = 32;                   // copies of the block's LDS histogram: one per LDS bank
constexpr int TS_FNT = 1024;                    // threads per block of the finalize
constexpr int TS_BINS = 2 * SHM_THIST_BINS;     // [sign][class]
constexpr int TS_SLOT_WORDS = 96;               // u32 per chunk slot: TS_BINS counts, NaN count, |v| > 1 count, min, max (float bits), 4 unused
constexpr int TS_W_NAN = TS_BINS, TS_W_CLIP = TS_BINS + 1, TS_W_MIN = TS_BINS + 2, TS_W_MAX = TS_BINS + 3;
constexpr int TS_CLS_NONFINITE = SHM_THIST_BINS - 1, TS_CLS_ONE = SHM_THIST_BINS - 2;
constexpr int TS_SLOT_VECS = TS_SLOT_WORDS / 4;
constexpr int TS_FGROUPS = TS_FNT / TS_SLOT_VECS;      // 42 groups of 24 threads
static_assert(TS_BINS + 4 <= TS_SLOT_WORDS && TS_BINS < TS_NT && TS_W_MIN % 4 == 2, "slot layout: {NaN, clipped, min, max} share a 16-byte vector");
static_assert(TS_CLS_ONE == -SHM_THIST_EMIN + 2, "classes 2 .. 41 are the exponents EMIN .. -1");

struct TsSeg {
    size_t off, len;
    unsigned chunk0;            // first chunk (= block of the chunk pass, = workspace slot) of the segment
};

struct TsArgs {
    const float* x;
    unsigned* slots;            // [nchunks][TS_SLOT_WORDS]
    double* sums;               // [nchunks][2]: sum, sum of squares
    double* stats;              // [nseg][SHM_TSTAT_N]
    unsigned long long* hist;   // [nseg][2][SHM_THIST_BINS]
    float scale;
    int nseg;
    unsigned nchunks;
    TsSeg seg[SHM_TSTAT_MAX_SEGS];
};
static_assert(sizeof(TsArgs) <= 4096, "kernel argument block");

struct TsAcc {
    float mn, mx;
    double s, q;
    unsigned nan, clip;
};

// class of a scaled value from its bits (include/shmgan_hip.h); sign bit only for normal finite values
__device__ __forceinline__ int ts_bin(unsigned u) {
    const int e = (int)((u >> 23) & 0xffu);
    if (e == 0) return 0;
    if (e == 255) return TS_CLS_NONFINITE;
    int cls = e - (127 - TS_CLS_ONE);                       // floor(log2|v|) + 42
    cls = cls < 1 ? 1 : (cls > TS_CLS_ONE ? TS_CLS_ONE : cls);
    return (int)(u >> 31) * SHM_THIST_BINS + cls;
}

__device__ __forceinline__ void ts_value(float x, float scale, TsAcc& a, int& bin) {
    const float v = x * scale;
    const unsigned u = __float_as_uint(v), mag = u & 0x7fffffffu;
    bin = ts_bin(u);
    if (mag < 0x7f800000u) {
        a.mn = fminf(a.mn, v);
        a.mx = fmaxf(a.mx, v);
        const double d = (double)v;
        a.s += d;
        a.q += d * d;
        a.clip += mag > 0x3f800000u;
    } else {
        a.nan += mag > 0x7f800000u;
    }
}

__global__ __launch_bounds__(TS_NT) void tensor_stats_chunk_kernel(const TsArgs a) {
    __shared__ unsigned hb[TS_BINS * TS_COPIES];             // [bin][copy]
    __shared__ double ws[TS_WAVES], wq[TS_WAVES];
    __shared__ float wmn[TS_WAVES], wmx[TS_WAVES];
    __shared__ unsigned wnan[TS_WAVES], wclip[TS_WAVES];
    const unsigned blk = blockIdx.x;
    // the segment of this chunk: the last one with chunk0 <= blk (block-uniform, scalar loads from the kernel arguments)
    int lo = 0, hi = a.nseg - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (a.seg[mid].chunk0 <= blk) lo = mid; else hi = mid - 1;
    }
    const size_t slen = a.seg[lo].len;
    const size_t rel = (size_t)(blk - a.seg[lo].chunk0) * TS_CHUNK;
    if (rel >= slen) return;                                 // cannot happen with the host's table; never read out of a segment
    const int n = (int)(slen - rel < (size_t)TS_CHUNK ? slen - rel : (size_t)TS_CHUNK);
    const float* p = a.x + a.seg[lo].off + rel;
    const float scale = a.scale;

    // scalar head up to the first 16-byte boundary, 16-byte body, scalar tail
    int head = (int)((16u - (unsigned)((uintptr_t)p & 15u)) & 15u) >> 2;
    if (head > n) head = n;
    const int nvec = (n - head) >> 2;
    const int tail0 = head + 4 * nvec;
    // the whole body is in flight before the first value is looked at
    const f32x4* pv = (const f32x4*)(p + head);
    f32x4 v[TS_VEC];
#pragma unroll
    for (int k = 0; k < TS_VEC; ++k) {
        const int i = k * TS_NT + threadIdx.x;
        v[k] = i < nvec ? pv[i] : f32x4{0.f, 0.f, 0.f, 0.f};
    }
    for (int i = threadIdx.x; i < TS_BINS * TS_COPIES; i += TS_NT) hb[i] = 0u;
    __syncthreads();
    // bin counts: LDS integer adds into the block's histogram, one copy per lane (mod 32).  Copy c of every bin lives in bank c, so the
    // lanes of a wave never meet in a bank however the values cluster (gradients sit in a handful of exponents: HIP guide, guideline 12)
    unsigned* h = hb + (threadIdx.x & (TS_COPIES - 1));
    TsAcc acc = {INFINITY, -INFINITY, 0.0, 0.0, 0u, 0u};
    int bin;
    if ((int)threadIdx.x < head) {
        ts_value(p[threadIdx.x], scale, acc, bin);
        atomicAdd(&h[bin * TS_COPIES], 1u);
    }
#pragma unroll
    for (int k = 0; k < TS_VEC; ++k) {
        if (k * TS_NT + (int)threadIdx.x < nvec) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                ts_value(v[k][j], scale, acc, bin);
                atomicAdd(&h[bin * TS_COPIES], 1u);
            }
        }
    }
    if (tail0 + (int)threadIdx.x < n) {
        ts_value(p[tail0 + threadIdx.x], scale, acc, bin);
        atomicAdd(&h[bin * TS_COPIES], 1u);
    }

    // block partial in a fixed order: wave shuffles, then the waves in wave order
    acc.s = shm_wave_sum(acc.s);
    acc.q = shm_wave_sum(acc.q);
    acc.mn = shm_wave_min(acc.mn);
    acc.mx = shm_wave_max(acc.mx);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        acc.nan += __shfl_down(acc.nan, o, 64);
        acc.clip += __shfl_down(acc.clip, o, 64);
    }
    if ((threadIdx.x & 63) == 0) {
        const int w = threadIdx.x >> 6;
        ws[w] = acc.s;
        wq[w] = acc.q;
        wmn[w] = acc.mn;
        wmx[w] = acc.mx;
        wnan[w] = acc.nan;
        wclip[w] = acc.clip;
    }
    __syncthreads();
    unsigned* slot = a.slots + (size_t)blk * TS_SLOT_WORDS;
    if (threadIdx.x < TS_BINS) {
        unsigned c = 0;
#pragma unroll
        for (int k = 0; k < TS_COPIES; ++k) c += hb[threadIdx.x * TS_COPIES + ((k + threadIdx.x) & (TS_COPIES - 1))];
        slot[threadIdx.x] = c;
    } else if (threadIdx.x == TS_BINS) {
        float mn = wmn[0], mx = wmx[0];
        unsigned nn = wnan[0], nc = wclip[0];
        double s = ws[0], q = wq[0];
        for (int w = 1; w < TS_WAVES; ++w) {
            mn = fminf(mn, wmn[w]);
            mx = fmaxf(mx, wmx[w]);
            nn += wnan[w];
            nc += wclip[w];
            s += ws[w];
            q += wq[w];
        }
        slot[TS_W_NAN] = nn;
        slot[TS_W_CLIP] = nc;
        slot[TS_W_MIN] = __float_as_uint(mn);
        slot[TS_W_MAX] = __float_as_uint(mx);
        a.sums[(size_t)blk * 2] = s;
        a.sums[(size_t)blk * 2 + 1] = q;
    }
}

// grid (nseg).  The integer words of a slot are read 16 bytes at a time: 24 threads cover a slot, TS_FGROUPS such groups take the
// segment's chunks round-robin (a 3x3x512x1024 kernel has 576 of them), LDS adds the groups.  Integer sums do not depend on the order;
// the f64 sums go through shm_block_sum: every thread a fixed stride of slots in chunk order, then the block in thread order.
__global__ __launch_bounds__(TS_FNT) void tensor_stats_finalize_kernel(const TsArgs a) {
    __shared__ unsigned long long cnt[TS_FGROUPS][TS_SLOT_WORDS];
    __shared__ float gmn[TS_FGROUPS], gmx[TS_FGROUPS];
    __shared__ unsigned long long tot[TS_SLOT_WORDS];
    const int s = blockIdx.x;
    const unsigned c0 = a.seg[s].chunk0;
    const unsigned nc = (unsigned)((a.seg[s].len + TS_CHUNK - 1) / TS_CHUNK);
    const shm_u32x4* slots = (const shm_u32x4*)(a.slots + (size_t)c0 * TS_SLOT_WORDS);
    const double* sums = a.sums + (size_t)c0 * 2;
    const int q = threadIdx.x % TS_SLOT_VECS, g = threadIdx.x / TS_SLOT_VECS;
    if (g < TS_FGROUPS) {
        unsigned long long acc[4] = {0, 0, 0, 0};
        float mn = INFINITY, mx = -INFINITY;
#pragma unroll 4
        for (unsigned c = g; c < nc; c += TS_FGROUPS) {
            const shm_u32x4 w = slots[(size_t)c * TS_SLOT_VECS + q];
            acc[0] += w[0];
            acc[1] += w[1];
            acc[2] += w[2];
            acc[3] += w[3];
            mn = fminf(mn, __uint_as_float(w[2]));           // meaningful in the vector that holds TS_W_MIN / TS_W_MAX only
            mx = fmaxf(mx, __uint_as_float(w[3]));
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) cnt[g][q * 4 + j] = acc[j];
        if (q == TS_W_MIN / 4) {
            gmn[g] = mn;
            gmx[g] = mx;
        }
    }
    double sv = 0.0, qv = 0.0;
    for (unsigned c = threadIdx.x; c < nc; c += TS_FNT) {
        sv += sums[(size_t)c * 2];
        qv += sums[(size_t)c * 2 + 1];
    }
    sv = shm_block_sum<TS_FNT>(sv);                             // its barriers also publish cnt / gmn / gmx
    qv = shm_block_sum<TS_FNT>(qv);
    if (threadIdx.x < TS_BINS + 2) {
        unsigned long long c = 0;
        for (int k = 0; k < TS_FGROUPS; ++k) c += cnt[k][threadIdx.x];
        tot[threadIdx.x] = c;
        if (threadIdx.x < TS_BINS) a.hist[(size_t)s * TS_BINS + threadIdx.x] = c;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long finite = 0;
        for (int b = 0; b < TS_BINS; ++b)
            if (b % SHM_THIST_BINS != TS_CLS_NONFINITE) finite += tot[b];
        const unsigned long long nonfinite = tot[TS_CLS_NONFINITE] + tot[SHM_THIST_BINS + TS_CLS_NONFINITE];
        float mn = gmn[0], mx = gmx[0];
        for (int k = 1; k < TS_FGROUPS; ++k) {
            mn = fminf(mn, gmn[k]);
            mx = fmaxf(mx, gmx[k]);
        }
        double* o = a.stats + (size_t)s * SHM_TSTAT_N;
        o[SHM_TSTAT_FINITE] = (double)finite;
        o[SHM_TSTAT_NAN] = (double)tot[TS_W_NAN];
        o[SHM_TSTAT_INF] = (double)(nonfinite - tot[TS_W_NAN]);
        o[SHM_TSTAT_MIN] = finite ? (double)mn : 0.0;
        o[SHM_TSTAT_MAX] = finite ? (double)mx : 0.0;
        o[SHM_TSTAT_SUM] = sv;
        o[SHM_TSTAT_SUMSQ] = qv;
        o[SHM_TSTAT_CLIPPED] = (double)tot[TS_W_CLIP];
    }
}

size_t ts_align256(size_t v) { return (v + 255) & ~(size_t)255; }
size_t ts_ws_bytes(size_t nchunks) {
    return ts_align256(nchunks * TS_SLOT_WORDS * sizeof(unsigned)) + ts_align256(nchunks * 2 * sizeof(double));
}

// ---- loss ring ----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void loss_ring_put_kernel(const double* __restrict__ dl, const double* __restrict__ il,
                                                           const double* __restrict__ sl, const unsigned* __restrict__ abort_word,
                                                           double* __restrict__ row, double step) {
    const int t = threadIdx.x;
    double v;
    if (t < SHM_LOSS_ROW_DL) v = dl[t];
    else if (t < SHM_LOSS_ROW_DL + SHM_LOSS_ROW_IL) v = il[t - SHM_LOSS_ROW_DL];
    else if (t < SHM_LOSS_ROW_STEP) v = sl[t - SHM_LOSS_ROW_DL - SHM_LOSS_ROW_IL];
    else if (t == SHM_LOSS_ROW_STEP) v = step;
    else if (t == SHM_LOSS_ROW_ABORT) v = abort_word ? (double)*abort_word : 0.0;
    else return;
    row[t] = v;
}

}  // namespace

extern "C" size_t shm_tensor_stats_workspace(int nseg, size_t n) {
    if (nseg < 1 || nseg > SHM_TSTAT_MAX_SEGS) return 0;
    return ts_ws_bytes(n / TS_CHUNK + (size_t)nseg);     // disjoint segments of [0, n): at most one short chunk each
}

extern "C" int shm_tensor_stats(const float* x, size_t n, const size_t* seg_off, const size_t* seg_len, int nseg, float scale,
                                double* stats, unsigned long long* hist, void* ws, size_t ws_bytes, void* stream) {
    SHM_REQUIRE(nseg >= 1 && nseg <= SHM_TSTAT_MAX_SEGS, SHM_E_SHAPE, "shm_tensor_stats: nseg %d outside [1, %d]", nseg,
                SHM_TSTAT_MAX_SEGS);
    SHM_REQUIRE(x && seg_off && seg_len && stats && hist, SHM_E_SHAPE, "shm_tensor_stats: null pointer");
    SHM_REQUIRE(((uintptr_t)x & 3) == 0, SHM_E_SHAPE, "shm_tensor_stats: x is not 4-byte aligned");
    TsArgs a;
    a.x = x;
    a.stats = stats;
    a.hist = hist;
    a.scale = scale;
    a.nseg = nseg;
    size_t chunks = 0;
    for (int s = 0; s < nseg; ++s) {
        SHM_REQUIRE(seg_off[s] <= n && seg_len[s] <= n - seg_off[s], SHM_E_SHAPE,
                    "shm_tensor_stats: segment %d [%zu, %zu + %zu) outside [0, %zu)", s, seg_off[s], seg_off[s], seg_len[s], n);
        a.seg[s].off = seg_off[s];
        a.seg[s].len = seg_len[s];
        a.seg[s].chunk0 = (unsigned)chunks;
        chunks += (seg_len[s] + TS_CHUNK - 1) / TS_CHUNK;
        SHM_REQUIRE(chunks <= 0x7fffffffu, SHM_E_SHAPE, "shm_tensor_stats: more than 2^31 chunks of %d floats", TS_CHUNK);
    }
    for (int s = nseg; s < SHM_TSTAT_MAX_SEGS; ++s) a.seg[s] = TsSeg{0, 0, (unsigned)chunks};
    a.nchunks = (unsigned)chunks;
    const size_t need = ts_ws_bytes(chunks);
    SHM_REQUIRE(chunks == 0 || (ws && ((uintptr_t)ws & 15) == 0 && ws_bytes >= need), SHM_E_WORKSPACE,
                "shm_tensor_stats: workspace of %zu bytes (16-byte aligned) needed, %zu given", need, ws ? ws_bytes : 0);
    a.slots = (unsigned*)ws;
    a.sums = (double*)((char*)ws + ts_align256(chunks * TS_SLOT_WORDS * sizeof(unsigned)));
    hipStream_t st = (hipStream_t)stream;
    if (chunks > 0) {
        hipLaunchKernelGGL(tensor_stats_chunk_kernel, dim3((unsigned)chunks), dim3(TS_NT), 0, st, a);
        SHM_LAUNCH_CHECK("shm_tensor_stats (chunks)");
    }
    hipLaunchKernelGGL(tensor_stats_finalize_kernel, dim3(nseg), dim3(TS_FNT), 0, st, a);
    SHM_LAUNCH_CHECK("shm_tensor_stats (finalize)");
    return SHM_OK;
}

extern "C" int shm_loss_ring_put(const double* dl, const double* il, const double* sl, const void* abort_word, double* ring,
                                 int rows, int row, long long step, void* stream) {
    SHM_REQUIRE(dl && il && sl && ring, SHM_E_SHAPE, "shm_loss_ring_put: null pointer");
    SHM_REQUIRE(rows >= 1 && row >= 0 && row < rows, SHM_E_SHAPE, "shm_loss_ring_put: row %d outside [0, %d)", row, rows);
    hipLaunchKernelGGL(loss_ring_put_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, dl, il, sl, (const unsigned*)abort_word,
                       ring + (size_t)row * SHM_LOSS_ROW, (double)step);
    SHM_LAUNCH_CHECK("shm_loss_ring_put");
    return SHM_OK;
}
