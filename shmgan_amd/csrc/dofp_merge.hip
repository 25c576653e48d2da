// Merging an exposure bracket of polariser-mosaic frames into one 16-bit mosaic.
//
//   shm_dofp_merge   n pages of one mosaic, taken with exposures e_0 .. e_(n-1), become one uint16 mosaic on the scale of the shortest
//                    exposure with f = 16 - bits fractional bits: per photosite every page below the white level votes, weighted by its
//                    exposure time (the sum of the black-subtracted counts times a factor that depends on WHICH pages are valid), and a site
//                    clipped in every page comes out at the white level.  include/shmgan_hip.h states the arithmetic, which is integer and
//                    exact.  It runs in front of shm_dofp_views / shm_dofp_develop, behind shm_dofp_calibrate of each page.
//
// A bandwidth pass shaped like dofp_calibrate.hip.  One thread makes DF_GROUP = 8 consecutive samples of one row: it reads that group from
// every page (df_load8: one 16- or 8-byte access where the page's base and pitch are multiples of 8 elements and the group is full, one
// access per element otherwise; each page and the destination are judged separately) and writes it once.  The kernel is instantiated per
// page count, so the page walk is unrolled, the page pointers are named kernel arguments and all loads of a group are issued before the
// first is used.  The factor table (2^n <= 256 entries) is indexed by a mask that differs per lane, so it goes into LDS once per block; the
// product is one 64-bit multiply-add (v_mad_i64_i32), and there is no division.
//
// counts: a thread packs how many of its sites have 0 .. n valid pages into 16-bit fields, a wave adds the fields with shuffles, the four
// waves of a block meet in LDS and the block leaves with at most n + 1 integer atomics; a wave-uniform branch skips all of that when
// nothing is counted.
#include "dofp_dev.h"

namespace {

constexpr int MG_BX = 64;                       // threads along a row: 512 samples; one wave
constexpr int MG_BY = 4;                        // rows per block
static_assert(MG_BX * MG_BY == SHM_DOFP_MERGE_TABLE, "one thread stages one table entry");

struct MergeArgs {
    const void* page[SHM_DOFP_MERGE_MAX];
    const unsigned* table;                      // device uint32 [SHM_DOFP_MERGE_TABLE]
    unsigned* counts;                           // device unsigned [SHM_DOFP_MERGE_MAX + 1], cleared on the stream in front of the launch, or null
    unsigned vpage;                             // bit k: groups of DF_GROUP start aligned in page k
    int vdst;                                   // ... in the destination
    int black, white, f, allsat;                // allsat = min(65535, white << f)
};

template <typename T, int N>
__global__ void __launch_bounds__(MG_BX* MG_BY) dofp_merge_kernel(const MergeArgs a, unsigned short* __restrict__ dst, int h, int w, size_t spitch,
                                                                   size_t dpitch) {
    __shared__ unsigned s_tab[SHM_DOFP_MERGE_TABLE];
    __shared__ unsigned s_cnt[SHM_DOFP_MERGE_MAX + 1];
    const int tid = threadIdx.y * MG_BX + threadIdx.x;
    s_tab[tid] = a.table[tid];
    if (a.counts && tid <= N) s_cnt[tid] = 0u;
    __syncthreads();
    const int y = blockIdx.y * MG_BY + threadIdx.y;
    const int xg = DF_GROUP * (blockIdx.x * MG_BX + threadIdx.x);
    const bool live = y < h && xg < w;                                     // no early return: every thread reaches the barriers below
    const int nvalid = !live ? 0 : w - xg < DF_GROUP ? w - xg : DF_GROUP;
    unsigned o[DF_GROUP], m[DF_GROUP] = {};                                // m: which pages are valid, per site
    if (live) {
        const bool full = nvalid == DF_GROUP;
        const size_t s0 = (size_t)y * spitch + xg;
        unsigned v[N][DF_GROUP];
#pragma unroll
        for (int k = 0; k < N; ++k) df_load8((const T*)a.page[k] + s0, full && ((a.vpage >> k) & 1u), nvalid, v[k]);
        int E[DF_GROUP];
#pragma unroll
        for (int j = 0; j < DF_GROUP; ++j) E[j] = 0;
#pragma unroll
        for (int k = 0; k < N; ++k)
#pragma unroll
            for (int j = 0; j < DF_GROUP; ++j) {
                const bool ok = (int)v[k][j] < a.white;
                E[j] += ok ? (int)v[k][j] - a.black : 0;
                m[j] |= ok ? 1u << k : 0u;
            }
        const int base = a.black << a.f;
#pragma unroll
        for (int j = 0; j < DF_GROUP; ++j) {
            // |E| < 2^19 and mul <= 2^28: the sum is inside int64 and R inside int32; >> of a negative value is arithmetic here
            const int R = (int)(((long long)E[j] * (int)s_tab[m[j]] + (1ll << (SHM_DOFP_MERGE_Q - 1))) >> SHM_DOFP_MERGE_Q);
            const int r = base + R;
            o[j] = m[j] ? (unsigned)(r < 0 ? 0 : r > 65535 ? 65535 : r) : (unsigned)a.allsat;
        }
        df_store8(dst + (size_t)y * dpitch + xg, full && a.vdst, nvalid, o);
    }
    if (a.counts) {                                                        // wave-uniform: a kernel argument
        unsigned long long nib = 0ull;                                     // class c in bits 4 c .. 4 c + 3: at most 8 sites per thread
#pragma unroll
        for (int j = 0; j < DF_GROUP; ++j)
            if (j < nvalid) nib += 1ull << (4 * __popc(m[j]));
        constexpr int NW = (N + 2) / 2;                                    // classes 0 .. N, two 16-bit fields per word: a wave's sum is <= 512
        unsigned acc[NW];
#pragma unroll
        for (int i = 0; i < NW; ++i) {
            acc[i] = (unsigned)(nib >> (8 * i)) & 15u;
            if (2 * i + 1 <= N) acc[i] |= ((unsigned)(nib >> (8 * i + 4)) & 15u) << 16;
        }
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1)
#pragma unroll
            for (int i = 0; i < NW; ++i) acc[i] += __shfl_xor(acc[i], d, 64);
        if (threadIdx.x == 0) {
#pragma unroll
            for (int c = 0; c <= N; ++c) {
                const unsigned t = (acc[c >> 1] >> (16 * (c & 1))) & 0xffffu;
                if (t) atomicAdd(&s_cnt[c], t);
            }
        }
        __syncthreads();
        if (tid <= N && s_cnt[tid]) atomicAdd(&a.counts[tid], s_cnt[tid]);
    }
}

template <typename T, int N>
void mg_launch_n(const MergeArgs& a, unsigned short* dst, int h, int w, size_t spitch, size_t dpitch, hipStream_t st) {
    const dim3 grid(shm_cdiv(shm_cdiv(w, DF_GROUP), MG_BX), shm_cdiv(h, MG_BY)), block(MG_BX, MG_BY);
    hipLaunchKernelGGL((dofp_merge_kernel<T, N>), grid, block, 0, st, a, dst, h, w, spitch, dpitch);
}

template <typename T>
void mg_launch(MergeArgs a, int n, unsigned short* dst, int h, int w, size_t spitch, size_t dpitch, hipStream_t st) {
    a.vpage = 0u;
    for (int k = 0; k < n; ++k)
        if ((uintptr_t)a.page[k] % (DF_GROUP * sizeof(T)) == 0 && spitch % DF_GROUP == 0) a.vpage |= 1u << k;
    a.vdst = (uintptr_t)dst % (DF_GROUP * sizeof(unsigned short)) == 0 && dpitch % DF_GROUP == 0;
    switch (n) {
        case 2: mg_launch_n<T, 2>(a, dst, h, w, spitch, dpitch, st); break;
        case 3: mg_launch_n<T, 3>(a, dst, h, w, spitch, dpitch, st); break;
        case 4: mg_launch_n<T, 4>(a, dst, h, w, spitch, dpitch, st); break;
        case 5: mg_launch_n<T, 5>(a, dst, h, w, spitch, dpitch, st); break;
        case 6: mg_launch_n<T, 6>(a, dst, h, w, spitch, dpitch, st); break;
        case 7: mg_launch_n<T, 7>(a, dst, h, w, spitch, dpitch, st); break;
        default: mg_launch_n<T, 8>(a, dst, h, w, spitch, dpitch, st); break;
    }
}

}  // namespace

extern "C" int shm_dofp_merge(const void* const* src_ptrs, int n, int bits, int h, int w, size_t src_pitch, const unsigned* table,
                              const unsigned* table_host, int black, int white, unsigned short* dst, size_t dst_pitch, unsigned* counts,
                              void* stream) {
    const char* who = "shm_dofp_merge";
    SHM_REQUIRE(src_ptrs && table && table_host && dst, SHM_E_SHAPE, "%s: null pointer (src_ptrs, table, table_host or dst)", who);
    SHM_REQUIRE(n >= 2 && n <= SHM_DOFP_MERGE_MAX, SHM_E_SHAPE, "%s: n %d outside [2, %d]", who, n, SHM_DOFP_MERGE_MAX);
    for (int k = 0; k < n; ++k) SHM_REQUIRE(src_ptrs[k], SHM_E_SHAPE, "%s: null pointer (src_ptrs[%d])", who, k);
    SHM_REQUIRE(bits >= 8 && bits <= 16, SHM_E_SHAPE, "%s: bits %d outside [8, 16]", who, bits);
    SHM_REQUIRE(h >= 1 && h <= DF_DIM_MAX && w >= 1 && w <= DF_DIM_MAX, SHM_E_SHAPE, "%s: sizes h %d, w %d outside [1, %d]", who, h, w, DF_DIM_MAX);
    SHM_REQUIRE(src_pitch >= (size_t)w, SHM_E_SHAPE, "%s: src_pitch %zu below w %d", who, src_pitch, w);
    SHM_REQUIRE(dst_pitch >= (size_t)w, SHM_E_SHAPE, "%s: dst_pitch %zu below w %d", who, dst_pitch, w);
    for (int k = 0; k < n; ++k) SHM_REQUIRE((const void*)dst != src_ptrs[k], SHM_E_SHAPE, "%s: dst == src_ptrs[%d] (not in place)", who, k);
    const int f = 16 - bits;
    SHM_REQUIRE(black >= 0 && black <= (65535 - 16) >> f, SHM_E_SHAPE, "%s: black %d outside [0, %d] (black << %d above 65519)", who, black,
                (65535 - 16) >> f, f);
    SHM_REQUIRE(white >= 1 && white <= 1 << bits, SHM_E_SHAPE, "%s: white %d outside [1, %d]", who, white, 1 << bits);
    SHM_REQUIRE(white > black, SHM_E_SHAPE, "%s: white %d not above black %d", who, white, black);
    for (int m = 1; m < 1 << n; ++m)
        SHM_REQUIRE(table_host[m] >= 1u && table_host[m] <= 1u << (f + SHM_DOFP_MERGE_Q), SHM_E_SHAPE, "%s: table_host[%d] = %u outside [1, %u]", who,
                    m, table_host[m], 1u << (f + SHM_DOFP_MERGE_Q));
    MergeArgs a;
    for (int k = 0; k < SHM_DOFP_MERGE_MAX; ++k) a.page[k] = k < n ? src_ptrs[k] : nullptr;
    a.table = table, a.counts = counts;
    a.vpage = 0u, a.vdst = 0;
    a.black = black, a.white = white, a.f = f;
    a.allsat = (white << f) > 65535 ? 65535 : white << f;
    hipStream_t st = (hipStream_t)stream;
    if (counts) {
        const hipError_t e = hipMemsetAsync(counts, 0, (SHM_DOFP_MERGE_MAX + 1) * sizeof(unsigned), st);
        SHM_REQUIRE(e == hipSuccess, SHM_E_HIP, "%s: clearing counts failed: %s", who, hipGetErrorString(e));
    }
    if (bits == 8) mg_launch<unsigned char>(a, n, dst, h, w, src_pitch, dst_pitch, st);
    else mg_launch<unsigned short>(a, n, dst, h, w, src_pitch, dst_pitch, st);
    SHM_LAUNCH_CHECK(who);
    return SHM_OK;
}
