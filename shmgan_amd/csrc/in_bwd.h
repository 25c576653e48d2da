// Shared pieces of the InstanceNorm-backward kernels: the argument block, the one-pass forms' scratch layout and device helpers, the launcher's
// plan, and the launch function each kernel family's translation unit sits behind (instnorm_bwd_2pass.hip, instnorm_bwd_fused8.hip,
// instnorm_bwd_fusedg.hip, grad_sums.hip).  instnorm_bwd.hip has the entry points, the plan (in_bwd_plan) and the launcher.
#pragma once
#include "elem.h"

struct InBwdArgs {               // g1, g2, a, dz: tensors of the kernels' element type T
    const void* g1;
    const void* g2;
    const void* a;
    const double* stats;
    double* red;
    void* dz;
    double* dbias;
    int ldg1, ldg2, lda, lddz;
    int h, w, c, chunk;
    float slope;
    int rev;
    const float* r1_dz;          // rank-1 gradient (R1 kernels): d_out[n, p, ch] = r1_dz[n * hw + p] * r1_w[ch] -- the generator head's
    const float* r1_w;           // input gradient, formed on the fly instead of being written by the head and read twice here
    // RAW apply kernels (shm_in_bwd_apply): the sums come from the epilogues of the launches that wrote g1 / g2 (gsum), as slot
    // copies [gslots][batch][c][2]: gred = (sum g1, sum g1 * a), gredp = (sum g2, sum g2 * pooled) or null; dstage = f64 [batch][c]
    // staging of the bias gradient
    const double* gred;
    const double* gredp;
    const float* beta;
    double* dstage;
    int gslots;
    int nt;                      // apply pass: g1 is read for the last time -> non-temporal loads
    int n0, nbatch;              // sample chunking (in_bwd_impl): this launch covers samples [n0, n0 + gridDim.y) of nbatch
    int interleave;              // apply pass: tiles of pixels dealt round-robin over a sample's blocks ("elem.interleave")
    int fold;                    // one-pass kernels: the launch's last group folds the staged bias gradient into dbias itself
};

// ------------------------------------------------------------------------------------------------------------------ one-pass forms: scratch
constexpr int SHM_FUSED_FLAGS = 16, SHM_FUSED_SYNC_WORDS = 32 * (SHM_FUSED_FLAGS + 2);
// SHM_IN_BWD_FUSED_DOUBLES (include/shmgan_hip.h) spells a group's counters and flags as the literal 288 doubles: the one size formula on this side
static_assert(SHM_FUSED_SYNC_WORDS / 2 == 288, "SHM_IN_BWD_FUSED_DOUBLES counts 288 doubles of counters and flags per barrier group");
// scratch (float64 units): partials f32 [batch][c / CB][bpi][3 CB] (sum g, sum g * xhat interleaved, then sum dz) | means f32 [batch][c][2] | sync u32
// [batch][c / CB][SYNC_WORDS] | timeout word.  CB = min(c, 64) channels per barrier group, bpi = blocks per group = h * w * CB / 16384.
static inline size_t fused_row_doubles(int batch, size_t bpi, int c) { return ((size_t)batch * bpi * 3 * c + 1) / 2; }        // fp32 rows: [batch][c / CB][bpi][3 CB]
typedef float f32x8 __attribute__((ext_vector_type(8)));
__device__ __forceinline__ f32x8 unpack8(const shm_u32x4 u) {
    f32x8 r;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        r[2 * i] = __uint_as_float(u[i] << 16);
        r[2 * i + 1] = __uint_as_float(u[i] & 0xffff0000u);
    }
    return r;
}
// coherent (device-scope, L2-bypassing) accesses without fences: see the barrier of in_bwd_fused8_kernel
template <typename V>
__device__ __forceinline__ V coh_load(const V* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
template <typename V>
__device__ __forceinline__ void coh_store(V* p, V v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// The launch's last group folds the staged bias gradient (round 6: dbias_fold_kernel was one more launch behind each of the step's ~44 one-pass
// calls).  `staging` = f64 [batch][c], written by every group's last departer (its CB channels of its sample, coherent stores, acknowledged before
// the group takes a ticket at `ticket`); the group whose ticket is the last adds the samples in dbias_fold_kernel's order -- four interleaved partial
// sums, (s0 + s1) + (s2 + s3): the same bits as the separate launch -- into dbias, and leaves staging and ticket zero.  Called by all 256 threads of a
// group's last departer, after its staging stores.
__device__ __forceinline__ void fused_fold_dbias(double* __restrict__ staging, double* __restrict__ dbias, unsigned* __restrict__ ticket, int batch, int c,
                                                 unsigned ngroups, int* s_flag) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0) *s_flag = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) + 1u == ngroups;
    __syncthreads();
    if (!*s_flag) return;
    for (int ch = threadIdx.x; ch < c; ch += 256) {
        double sg[4] = {0.0, 0.0, 0.0, 0.0};
        int i = 0;
        for (; i + 8 <= batch; i += 8) {             // eight loads in flight (one at a time, 160 samples were 160 round trips)
            double v[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = coh_load(staging + (size_t)(i + j) * c + ch);
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                sg[j & 3] += v[j];                   // (i is a multiple of 8: (i + j) & 3 == j & 3)
                coh_store(staging + (size_t)(i + j) * c + ch, 0.0);
            }
        }
        for (; i < batch; ++i) {
            sg[i & 3] += coh_load(staging + (size_t)i * c + ch);
            coh_store(staging + (size_t)i * c + ch, 0.0);
        }
        dbias[ch] += (sg[0] + sg[1]) + (sg[2] + sg[3]);
    }
    if (threadIdx.x == 0) coh_store(ticket, 0u);
}

// ------------------------------------------------------------------------------------------------------------------ plan and launch functions
enum {
    SHM_INB_2PASS,        // in_bwd_reduce_kernel or in_bwd_reduce8_kernel, then in_bwd_apply_kernel, per chunk of samples
    SHM_INB_FUSED8,       // in_bwd_fused8_kernel <g2>: g and a held
    SHM_INB_FUSEDG,       // in_bwd_fusedg_kernel <2, 2, 4> or <8, 8, 3>: g held
};

// What instnorm_bwd.hip's in_bwd_plan decided for one call.  The launches below read no tuning knob and test no shape.
struct InBwdPlan {
    int form;                     // SHM_INB_*
    int dtype;                    // element types of the two-pass kernels
    bool g2, r1;                  // pooled gradient / rank-1 gradient (template arguments)
    bool wide8;                   // two passes: the reduce pass is in_bwd_reduce8_kernel
    int gvariant;                 // SHM_INB_FUSEDG: 0 = <2, 2, 4>, 1 = <8, 8, 3>
    // one pass: grid = (blocks, ncb, batch); the scratch is carved behind `rows` partial rows per group, offsets in 4-byte words
    int cb, ncb, blocks;
    size_t rows, res_word, sync_word, err_word;
    unsigned arrivals;            // blocks a group's barrier waits for
    int fold;                     // the launch's last group folds the staged bias gradient (InBwdArgs::fold)
    // two passes: samples per chunk, block targets of the apply and the reduce pass
    int per_chunk, apply_blocks, reduce_blocks;
    int rev, nt, interleave;      // InBwdArgs::rev / nt (apply pass) / interleave
    const char* name;             // what shm_last_kernel() reports
};

struct InBwdFusedScratch {        // the caller's fused_scratch, carved
    float* part;                  // partial rows
    float* res;                   // means
    unsigned* sync;               // counters and flags
    unsigned* err;                // timeout word, group ticket
};

// instnorm_bwd_2pass.hip: one pass each on `grid` = (pixel chunks, samples of the chunk).  SHM_OK, or SHM_E_DTYPE (nothing launched); the caller checks the launch.
int shm_in_bwd_reduce_launch(const char* who, const InBwdArgs& k, int dtype, bool wide8, bool g2, bool r1, dim3 grid, hipStream_t st);
int shm_in_bwd_apply_launch(const char* who, const InBwdArgs& k, int dtype, bool g2, bool r1, bool raw, dim3 grid, hipStream_t st);
// instnorm_bwd_fused8.hip / instnorm_bwd_fusedg.hip: the one-pass launch, and hipOccupancyMaxActiveBlocksPerMultiprocessor of the instantiation
void shm_in_bwd_fused8_launch(const InBwdArgs& k, bool g2, const InBwdFusedScratch& s, unsigned* abort_dev, unsigned* abort_host, dim3 grid, unsigned arrivals,
                              hipStream_t st);
void shm_in_bwd_fusedg_launch(const InBwdArgs& k, int gvariant, const InBwdFusedScratch& s, unsigned* abort_dev, unsigned* abort_host, dim3 grid, unsigned arrivals,
                              hipStream_t st);
hipError_t shm_in_bwd_fused8_occupancy(bool g2, int* per_cu);
hipError_t shm_in_bwd_fusedg_occupancy(int gvariant, int* per_cu);
// grad_sums.hip: dbias[ch] += sum over slots of part[slot][ch] (see dbias_fold_kernel), and shm_in_bwd_apply's last launch (gsum_finish_kernel)
void shm_dbias_fold_launch(double* part, double* dbias, int nslot, int c, double* clear, double* keep, hipStream_t st);
void shm_gsum_finish_launch(double* dstage, double* dbias, int batch, int c, double* red, size_t nred, double* redp, double* keep, hipStream_t st);
