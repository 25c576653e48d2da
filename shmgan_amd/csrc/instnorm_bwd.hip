// InstanceNormalization backward, fused with LeakyReLU' and the AveragePooling2D gradient: the entry points (shm_in_bwd, shm_in_bwd_apply,
// shm_in_bwd_rank1), the choice between two passes and the two one-pass bf16 kernels (in_bwd_plan) and the launcher that switches on it.  The
// kernels sit in one translation unit per family behind the launch functions of in_bwd.h: instnorm_bwd_2pass.hip, instnorm_bwd_fused8.hip,
// instnorm_bwd_fusedg.hip, and grad_sums.hip for the bias-gradient fold and the gsum finish.
#include "in_bwd.h"

// Blocks of a one-pass kernel the current device holds at once (CUs x occupancy; queried once per device and form).  The kernel's
// barrier only completes if a whole group is resident, and two such launches may run side by side (two streams), each stuck with LESS than a
// group resident only while free slots remain -- so a group is limited to HALF of this figure (advisor, round 5: a CPX partition, a CU mask or a
// smaller part holds far fewer than the 1024 / 768 blocks of a whole MI355X, and the launcher used to assume them).  0 if the query fails.
static int fused_resident_blocks(int form) {          // 0: in_bwd_fused8_kernel<false>, 1: <true> (pooled), 2: in_bwd_fusedg_kernel<2, 2, 4>, 3: <8, 8, 3>
    static int cache[16][4];                 // 0 = not asked yet, -1 = the query failed
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 16) return 0;
    int v = __atomic_load_n(&cache[dev][form], __ATOMIC_RELAXED);
    if (v == 0) {
        int cus = 0, per_cu = 0;
        hipError_t e = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
        if (e == hipSuccess) e = form < 2 ? shm_in_bwd_fused8_occupancy(form == 1, &per_cu) : shm_in_bwd_fusedg_occupancy(form - 2, &per_cu);
        if (e != hipSuccess) (void)hipGetLastError();
        v = (e == hipSuccess && cus > 0 && per_cu > 0) ? cus * per_cu : -1;
        __atomic_store_n(&cache[dev][form], v, __ATOMIC_RELAXED);
    }
    return v > 0 ? v : 0;
}

struct InBwdReq {                // one call, after the argument checks (4 <= c <= 1024, c % 4 == 0, batch * h * w > 0)
    int dtype, batch, h, w, c;
    int ldg1, ldg2, lda, lddz;
    bool g2, r1, keep;           // pooled gradient, rank-1 gradient, the per-sample dz sums are wanted
    bool scratch;                // the one-pass forms' fused_scratch was given, ...
    size_t scratch_n;            // ... of this many doubles
    bool src_al16, dz_al16;      // the sources (g1, g2, a) / dz start on 16-byte boundaries
};

// Which form a call takes.  Host only; the only reader of the "elem.*" knobs in this launcher.  `resident(form)`: fused_resident_blocks, asked
// last, so that a call that could never take a one-pass form makes no HIP query.
//
// One pass ("elem.fused_bwd"): bf16 tensors, barrier groups of (sample, CB = min(c, 64) channels), at most "elem.fused_max_slices" (256) blocks per
// group of the kernel that holds g and a (in_bwd_fused8_kernel: slices of 16384 / CB pixels; with a pooled gradient 64-channel groups and whole
// tiles).  Round 6, in_bwd_fusedg_kernel: g held, a streamed twice; slices of 32768 / CB pixels (sixteen pixel slots per thread), half the blocks
// per group, and groups of up to 512 blocks where twice that fits the device (the 512 x 512 x 64 maps of BASELINE configs[3]): it takes 2 x the
// knob's value.  Measured (tools/probes/in_bwd_fusedg_ab.py, n = 40 / 160): it wins where a group has many blocks -- 256 x 256 x 64: 287 -> 252 us,
// n = 160: 1072 -> 879 us -- and loses on the smaller maps, whose short groups do not cover its two extra round trips (128 x 128 x 128: 122 -> 147
// us): automatic dispatch takes it from 256 slices of the 8-slot kind per group on.
//
// Two passes, sample chunks ("elem.chunk_mb", round 3): the apply pass re-reads what the reduce pass read.  On tensors larger than the 256 MiB
// Infinity Cache that second read comes from HBM again (the back-to-front / front-to-back walk only saves the turning point); run as
// reduce(chunk), apply(chunk) over chunks whose g + a fit the cache, the second read stays on die.  0 = one chunk.
//
// ONE scratch layout for both one-pass kernels (the caller's buffer is "zero behind the partial rows" whichever kernel ran last): means, counters
// and flags sit behind the rows region of the 16384 / CB-pixel slicing; the g-held kernel's rows fill half of it.
//
// Block targets: the reduce pass ends every block with an LDS combine and 2c f64 atomics onto the 2c addresses of its sample: with the
// streaming pass's ~4096 blocks a sample's address takes up to 256 serialized adds (n = 8, 256 x 256: 125 us for a pass whose
// data moves in 40) and the 512-channel maps issue 1.3 M atomics per launch.  Fewer, longer blocks -- about the same bytes per
// block in both dtypes: bf16 step 27.8 -> 27.1 ms, fp32 123.4 -> 122.9.  (The apply pass, one atomic per channel and block, is faster with
// its 4096 blocks: same grid for both measured +0.15 / +0.6 ms.)
static InBwdPlan in_bwd_plan(const InBwdReq& q, int (*resident)(int form)) {
    InBwdPlan p{};
    const int c = q.c, hw = q.h * q.w;
    p.dtype = q.dtype, p.g2 = q.g2, p.r1 = q.r1;
    p.rev = shm_tune(SHM_TUNE_ELEM_REVERSE);
    p.nt = shm_tune(SHM_TUNE_ELEM_NT);          // the apply pass is the last reader of g1
    p.interleave = shm_tune(SHM_TUNE_ELEM_INTERLEAVE);
    p.fold = q.keep ? 0 : 1;     // (the per-sample sums are wanted too -- SHM_NORM_SCALED's second term: the separate fold kernel copies them out)
    // 16-byte accesses of the bf16 sources: pitches AND bases (a slice 8 bytes into a 16-byte row takes the four-channel forms).  c >= 8 and c <= 1024 of the earlier spelling follow from c % 8 == 0 and the argument check, and
    // 256 / (c / 8) >= 1 from c <= 1024
    const bool src16 = (q.r1 || q.ldg1 % 8 == 0) && q.lda % 8 == 0 && (!q.g2 || q.ldg2 % 8 == 0) && q.src_al16;
    p.wide8 = (q.dtype == SHM_BF16 || q.dtype == SHM_BF16_GF32) && c % 8 == 0 && src16;          // eight channels per thread in the reduce pass
    // ---- one pass
    const int cb = c < 64 ? c : 64;
    const bool groups_ok = c < 64 ? c >= 8 && pow2_le64(c) : c % 64 == 0;            // whole groups; every thread of a block active
    const int slice = groups_ok ? 16384 / cb : 1, slice16 = 2 * slice;
    // pooled form: tiles of (256 / Wt) rows x Wt = min(w, 128) columns.  Consulted with a pooled gradient only, i.e. on even h and w: Wt >= 2, and
    // a power of two up to 128 divides 256 into an even number of rows
    const int wt = q.w < 128 ? q.w : 128;
    const bool g2_tiles = cb == 64 && (wt & (wt - 1)) == 0 && q.w % wt == 0 && q.h % (256 / wt) == 0;
    const bool base_ok = q.scratch && shm_tune(SHM_TUNE_ELEM_FUSED_BWD) && q.dtype == SHM_BF16 && !q.r1 && groups_ok && src16 && q.lddz % 8 == 0 && q.dz_al16 &&
                         q.batch <= 65535 && q.scratch_n >= SHM_IN_BWD_FUSED_DOUBLES(q.batch, hw, c);
    const int max_slices = shm_tune(SHM_TUNE_ELEM_FUSED_MAX_SLICES);
    const int hold = shm_tune(SHM_TUNE_ELEM_FUSED_HOLD);          // 0 automatic, 1 the round-5 kernel only (g and a held), 2 the g-held kernel only
    const int fgv = shm_tune(SHM_TUNE_ELEM_FUSED_GVARIANT);
    const int n8 = hw / slice, n16 = hw / slice16;                // blocks per group of either kernel
    // the g-held kernel addresses each tensor through one buffer descriptor per SAMPLE and 32-bit byte offsets: a sample of every pitch below 4 GiB
    const int ldmax = q.ldg1 > q.lda ? (q.ldg1 > q.lddz ? q.ldg1 : q.lddz) : (q.lda > q.lddz ? q.lda : q.lddz);
    const bool samp32 = (size_t)hw * ldmax * 2 < 0xfffffff0ull;
    const bool g_held = base_ok && hold != 1 && !q.g2 && samp32 && hw % slice16 == 0 && (hold == 2 || n8 >= 256) && n16 <= 2 * max_slices &&
                        2 * n16 <= resident(fgv == 1 ? 3 : 2);
    const bool ga_held = !g_held && base_ok && hold != 2 && hw % slice == 0 && n8 <= max_slices && (!q.g2 || g2_tiles) && 2 * n8 <= resident(q.g2 ? 1 : 0);
    if (g_held || ga_held) {
        p.form = g_held ? SHM_INB_FUSEDG : SHM_INB_FUSED8;
        p.gvariant = fgv, p.cb = cb, p.ncb = c / cb, p.blocks = g_held ? n16 : n8;
        p.rows = n8;                  // ONE scratch layout (above)
        p.res_word = 2 * fused_row_doubles(q.batch, p.rows, c);
        p.sync_word = p.res_word + (size_t)q.batch * c * 2;
        p.err_word = p.sync_word + (size_t)q.batch * p.ncb * SHM_FUSED_SYNC_WORDS;
        p.arrivals = p.blocks + (shm_tune(SHM_TUNE_ELEM_FUSED_TEST_STALL) ? 1u : 0u);
        p.name = !g_held ? (q.g2 ? "in_bwd_fused8_kernel<true>" : "in_bwd_fused8_kernel<false>") : fgv == 1 ? "in_bwd_fusedg_kernel<8, 8, 3>" : "in_bwd_fusedg_kernel<2, 2, 4>";
        return p;
    }
    // ---- two passes
    const int esz_a = q.dtype == SHM_F32 ? 4 : 2, esz_g = q.dtype == SHM_BF16 ? 2 : 4;
    const size_t per_sample = (size_t)hw * c * (esz_a + (q.r1 ? 0 : esz_g)) + (q.g2 ? (size_t)hw / 4 * c * esz_g : 0);
    const size_t chunk_bytes = (size_t)shm_tune(SHM_TUNE_ELEM_CHUNK_MB) << 20;
    p.per_chunk = q.batch;
    if (chunk_bytes && per_sample * q.batch > chunk_bytes) p.per_chunk = chunk_bytes / per_sample < 1 ? 1 : (int)(chunk_bytes / per_sample);
    const int rb = shm_tune(SHM_TUNE_ELEM_REDUCE_BLOCKS);
    p.reduce_blocks = rb ? rb : (q.dtype == SHM_F32 ? 1024 : 512);
    p.apply_blocks = shm_tune(SHM_TUNE_ELEM_APPLY_BLOCKS);        // (at least 256: pix_chunks never falls back to its own knob)
    p.name = p.wide8 ? "in_bwd_reduce8_kernel + in_bwd_apply_kernel" : "in_bwd_reduce_kernel + in_bwd_apply_kernel";
    return p;
}

// `red` is zero on entry by contract and zero again on return (no memset in front of every launch), also on the error paths behind the launch
// that filled it
static int launch_plan(const char* who, const InBwdPlan& p, InBwdArgs k, double* keep, double* fscr, unsigned* abort_dev, unsigned* abort_host, hipStream_t st) {
    const int batch = k.nbatch, c = k.c, hw = k.h * k.w;
    const size_t red_bytes = (size_t)batch * c * 3 * sizeof(double);
    double* const staging = k.red + (size_t)batch * c * 2;        // per-sample bias-gradient sums, behind the two sum planes
    k.rev = p.rev, k.nt = p.nt, k.interleave = p.interleave, k.fold = p.fold;
    if (p.form != SHM_INB_2PASS) {
        const InBwdFusedScratch s{(float*)fscr, (float*)fscr + p.res_word, (unsigned*)fscr + p.sync_word, (unsigned*)fscr + p.err_word};
        const dim3 grid(p.blocks, p.ncb, batch);
        if (p.form == SHM_INB_FUSEDG) shm_in_bwd_fusedg_launch(k, p.gvariant, s, abort_dev, abort_host, grid, p.arrivals, st);
        else shm_in_bwd_fused8_launch(k, p.g2, s, abort_dev, abort_host, grid, p.arrivals, st);
        shm_set_last_kernel("%s", p.name);
        SHM_LAUNCH_CHECK_CLEAR("shm_in_bwd(fused)", k.red, red_bytes, st);
        if (k.dbias && !p.fold) {       // (the two sum planes in front of the staging were not used: nothing to clear)
            shm_dbias_fold_launch(staging, k.dbias, batch, c, nullptr, keep, st);
            SHM_LAUNCH_CHECK_CLEAR("shm_in_bwd(fold)", k.red, red_bytes, st);
        }
        return SHM_OK;
    }
    for (int n0 = 0; n0 < batch; n0 += p.per_chunk) {
        const int nb = min(p.per_chunk, batch - n0);
        k.n0 = n0;
        InBwdArgs kr = k;                // the reduce pass: its own grid, and g1 is read again behind it
        kr.nt = 0;
        kr.chunk = shm_cdiv(hw, pix_chunks(hw, nb, c, p.reduce_blocks));
        k.chunk = shm_cdiv(hw, pix_chunks(hw, nb, c, p.apply_blocks));
        int r = shm_in_bwd_reduce_launch(who, kr, p.dtype, p.wide8, p.g2, p.r1, dim3(shm_cdiv(hw, kr.chunk), nb), st);
        if (r) return r;
        SHM_LAUNCH_CHECK("shm_in_bwd(reduce)");
        r = shm_in_bwd_apply_launch(who, k, p.dtype, p.g2, p.r1, false, dim3(shm_cdiv(hw, k.chunk), nb), st);
        if (r) return r;
    }
    shm_set_last_kernel("%s", p.name);
    SHM_LAUNCH_CHECK_CLEAR("shm_in_bwd(apply)", k.red, red_bytes, st);
    if (k.dbias) {
        shm_dbias_fold_launch(staging, k.dbias, batch, c, k.red, keep, st);
    } else {
        int r = shm_zero(k.red, (size_t)batch * c * 2 * sizeof(double), st);
        if (r) return r;
    }
    SHM_LAUNCH_CHECK_CLEAR("shm_in_bwd(fold)", k.red, red_bytes, st);
    return SHM_OK;
}

// shm_in_bwd and shm_in_bwd_rank1 (r1_dz != null) behind their null checks: the shared argument checks, the plan, the launch
static int in_bwd_impl(const char* who, const void* g1, int ldg1, const void* g2, int ldg2, const float* r1_dz, const float* r1_w, const void* a, int lda,
                       const double* stats, double* red, void* dz, int lddz, double* dbias, double* keep, double* fscr, size_t fscr_n, unsigned* abort_dev,
                       unsigned* abort_host, int batch, int h, int w, int c, float slope, int dtype, void* stream) {
    const bool r1 = r1_dz != nullptr;
    SHM_REQUIRE(!keep || dbias, SHM_E_SHAPE, "%s: the per-sample dz sums are staged only with a bias gradient", who);
    SHM_CHECK_C(c, who);
    SHM_REQUIRE((r1 || ldg1 % 4 == 0) && lda % 4 == 0 && lddz % 4 == 0 && (!g2 || ldg2 % 4 == 0), SHM_E_SHAPE, "%s: bad pitch", who);
    SHM_REQUIRE((r1 || ldg1 >= c) && lda >= c && lddz >= c && (!g2 || ldg2 >= c), SHM_E_SHAPE, "%s: pitch below the %d channels", who, c);
    SHM_REQUIRE(!g2 || (h % 2 == 0 && w % 2 == 0), SHM_E_SHAPE, "%s: pooled gradient needs even h,w", who);
    SHM_REQUIRE(!(r1 && g2), SHM_E_SHAPE, "%s: the rank-1 form takes no pooled gradient", who);
    if (batch == 0 || h * w == 0) return SHM_OK;
    const InBwdPlan p = in_bwd_plan(InBwdReq{dtype, batch, h, w, c, ldg1, ldg2, lda, lddz, g2 != nullptr, r1, keep != nullptr, fscr != nullptr, fscr_n,
                                                (((size_t)g1 | (size_t)g2 | (size_t)a) & 15) == 0, ((size_t)dz & 15) == 0},
                                       fused_resident_blocks);
    InBwdArgs k{g1, g2, a, stats, red, dz, dbias, ldg1, ldg2, lda, lddz, h, w, c, 0, slope, 0, r1_dz, r1_w};
    k.nbatch = batch;
    return launch_plan(who, p, k, keep, fscr, abort_dev, abort_host, (hipStream_t)stream);
}

extern "C" int shm_in_bwd(const void* g1, int ldg1, const void* g2, int ldg2, const void* a, int lda,
                          const double* stats, double* red, void* dz, int lddz, double* dbias, double* dz_sums, double* fused_scratch,
                          size_t fused_doubles, unsigned* abort_dev, unsigned* abort_host, int batch, int h, int w, int c, float slope, int dtype,
                          void* stream) {
    SHM_REQUIRE(g1, SHM_E_SHAPE, "shm_in_bwd: null gradient");
    return in_bwd_impl("shm_in_bwd", g1, ldg1, g2, ldg2, nullptr, nullptr, a, lda, stats, red, dz, lddz, dbias, dz_sums, fused_scratch, fused_doubles, abort_dev,
                       abort_host, batch, h, w, c, slope, dtype, stream);
}

// InstanceNorm + LeakyReLU backward WITHOUT its reduce pass: the per-(sample, channel) sums were formed in the epilogues of the
// launches that wrote g1 / g2 (shm_conv2d_dgrad_gsum, shm_conv2d_fwd_gsum), so this is one pass over the tensors -- read g1 [+ g2],
// read a, write dz -- where shm_in_bwd makes two.
extern "C" int shm_in_bwd_apply(const void* g1, int ldg1, const void* g2, int ldg2, const void* a, int lda, const double* stats, const float* beta,
                                double* red, double* redp, double* dstage, void* dz, int lddz, double* dbias, double* keep, int batch, int h, int w, int c,
                                float slope, int dtype, void* stream) {
    const char* who = "shm_in_bwd_apply";
    SHM_REQUIRE(!keep || dbias, SHM_E_SHAPE, "%s: the per-sample dz sums are staged only with a bias gradient", who);
    SHM_REQUIRE(g1 && a && stats && red && dz, SHM_E_SHAPE, "%s: null pointer", who);
    SHM_REQUIRE((g2 != nullptr) == (redp != nullptr), SHM_E_SHAPE, "%s: the pooled gradient g2 and its sums redp come together", who);
    SHM_REQUIRE(!redp || beta, SHM_E_SHAPE, "%s: the pooled form needs beta", who);
    SHM_REQUIRE(!dbias || dstage, SHM_E_SHAPE, "%s: the bias gradient needs its staging scratch", who);
    SHM_CHECK_C(c, who);
    SHM_REQUIRE(ldg1 % 4 == 0 && lda % 4 == 0 && lddz % 4 == 0 && (!g2 || ldg2 % 4 == 0), SHM_E_SHAPE, "%s: bad pitch", who);
    SHM_REQUIRE(ldg1 >= c && lda >= c && lddz >= c && (!g2 || ldg2 >= c), SHM_E_SHAPE, "%s: pitch below the %d channels", who, c);
    SHM_REQUIRE(!g2 || (h % 2 == 0 && w % 2 == 0), SHM_E_SHAPE, "%s: pooled gradient needs even h,w", who);
    if (batch == 0 || h * w == 0) return SHM_OK;
    hipStream_t st = (hipStream_t)stream;
    InBwdArgs k{g1, g2, a, stats, nullptr, dz, dbias, ldg1, ldg2, lda, lddz, h, w, c, 0, slope, 0, nullptr, nullptr, red, redp, beta, dstage, SHM_GSUM_SLOTS,
                shm_tune(SHM_TUNE_ELEM_NT), 0, batch};
    k.interleave = shm_tune(SHM_TUNE_ELEM_INTERLEAVE);
    const int hw = h * w;
    k.chunk = shm_cdiv(hw, pix_chunks(hw, batch, c, shm_tune(SHM_TUNE_ELEM_APPLY_BLOCKS)));
    const int r = shm_in_bwd_apply_launch(who, k, dtype, g2 != nullptr, false, true, dim3(shm_cdiv(hw, k.chunk), batch), st);
    if (r) return r;
    const size_t nred = (size_t)SHM_GSUM_SLOTS * batch * c * 2;
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) {
        shm_gsum_finish_launch(dstage, dbias, batch, c, red, nred, redp, keep, st);
        e = hipGetLastError();
    }
    if (e != hipSuccess) {           // zero on return also on the error path
        (void)hipMemsetAsync(red, 0, nred * sizeof(double), st);
        if (redp) (void)hipMemsetAsync(redp, 0, nred * sizeof(double), st);
        if (dstage) (void)hipMemsetAsync(dstage, 0, (size_t)batch * c * sizeof(double), st);
        shm_set_error("%s: launch failed: %s", who, hipGetErrorString(e));
        return SHM_E_HIP;
    }
    return SHM_OK;
}

// The same backward for the block in front of the generator head, whose output gradient is the rank-1 tensor
// d_out[n, p, ch] = hdz[n * h * w + p] * hw_[ch] (shm_head_in_bwd's dz_out and the head kernel): formed on the fly, so the head
// never writes its input gradient and neither pass here reads it (three passes over the largest activation of the network).
extern "C" int shm_in_bwd_rank1(const float* hdz, const float* hw_, const void* a, int lda, const double* stats, double* red, void* dz, int lddz,
                                double* dbias, double* dz_sums, int batch, int h, int w, int c, float slope, int dtype, void* stream) {
    SHM_REQUIRE(hdz && hw_, SHM_E_SHAPE, "shm_in_bwd_rank1: null gradient");
    return in_bwd_impl("shm_in_bwd_rank1", nullptr, 0, nullptr, 0, hdz, hw_, a, lda, stats, red, dz, lddz, dbias, dz_sums, nullptr, 0, nullptr, nullptr, batch, h, w, c,
                       slope, dtype, stream);
}
