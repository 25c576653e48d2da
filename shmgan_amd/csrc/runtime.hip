// The library's runtime, host code only: this thread's error string and last-kernel name, the process-wide tuning table behind
// shm_set_tuning / shm_get_tuning, the version, and the clock probe.  The clock probe is the one per-thread pointer a launcher still reads
// implicitly: it is a measurement hook that bench.py arms through shm_set_clock_probe, not data-path state (the abort words are arguments
// of shm_in_bwd and shm_adam_clip).
#include "common.h"

#include <stdarg.h>

// ---------------------------------------------------------------------------- core API
static thread_local char g_err[512] = "";

void shm_set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

static thread_local char g_kernel[128] = "";

void shm_set_last_kernel(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_kernel, sizeof(g_kernel), fmt, ap);
    va_end(ap);
}

// ---- dispatch tuning (shm_set_tuning / shm_get_tuning) -------------------------------------------------
#include <atomic>
#include <stdlib.h>
#include <string.h>
namespace {
struct TuneDef {
    const char* key;
    const char* env;       // initial value (read once) -- keeps the ablation tools' environment knobs alive
    int dflt, lo, hi;
};
const TuneDef kTune[SHM_TUNE_COUNT] = {
    {"tapgemm.variant", "SHM_TAPGEMM_VARIANT", 0, 0, SHM_TG_COUNT - 1},
    {"tapgemm.halo_min_blocks", "SHM_TAPGEMM_HALO_MIN", 1024, 0, 1 << 30},
    {"tapgemm.small_grid_blocks", "SHM_TAPGEMM_SMALLM", 1024, 0, 1 << 30},
    {"tapgemm.phase4_min_blocks", "SHM_TAPGEMM_PHASE4_MIN", 256, 0, 1 << 30},
    {"wgrad.variant", "SHM_WGRAD_VARIANT", 0, 0, 3},
    {"wgrad.blocks", "SHM_WGRAD_BLOCKS", 0, 0, 1 << 20},
    {"wgrad.bf16_rows", "SHM_WGRAD_BF16_ROWS", 0, 0, 4},
    {"stats.fusion", "SHM_STATS_FUSION", 1, 0, 1},
    {"elem.reverse", "SHM_ELEM_REVERSE", 1, 0, 1},
    {"elem.reduce_blocks", "SHM_ELEM_REDUCE_BLOCKS", 0, 0, 1 << 20},
    {"elem.nt_loads", "SHM_ELEM_NT", 0, 0, 1},
    {"elem.chunk_mb", "SHM_ELEM_CHUNK_MB", 0, 0, 1 << 20},
    {"elem.interleave", "SHM_ELEM_INTERLEAVE", 1, 0, 1},
    {"elem.stream_blocks", "SHM_ELEM_STREAM_BLOCKS", 32768, 256, 1 << 20},
    {"elem.apply_blocks", "SHM_ELEM_APPLY_BLOCKS", 4096, 256, 1 << 20},
    {"tapgemm.wreg16", "SHM_TAPGEMM_WREG16", 2, 0, 2},
    {"wgrad.bf16_wide", "SHM_WGRAD_BF16_WIDE", 0, 0, 4},
    {"wgrad.f32_split", "SHM_WGRAD_F32_SPLIT", 0, 0, 1},
    {"tapgemm.flat_epilogue", "SHM_TAPGEMM_FLAT_EPILOGUE", 0, 0, 1},
    {"elem.fused_bwd", "SHM_ELEM_FUSED_BWD", 1, 0, 1},
    {"elem.fused_max_slices", "SHM_ELEM_FUSED_MAX_SLICES", 256, 1, 512},
    {"conv.f32_split", "SHM_CONV_F32_SPLIT", 0, 0, 1},
    {"elem.fused_test_stall", "SHM_ELEM_FUSED_TEST_STALL", 0, 0, 1},
    {"elem.fused_hold", "SHM_ELEM_FUSED_HOLD", 0, 0, 2},
    {"elem.fused_gvariant", "SHM_ELEM_FUSED_GVARIANT", 0, 0, 1},
};
std::atomic<int> g_tune[SHM_TUNE_COUNT];
std::atomic<int> g_tune_init{0};
void tune_init() {
    if (g_tune_init.load(std::memory_order_acquire) == 2) return;
    int expect = 0;
    if (g_tune_init.compare_exchange_strong(expect, 1)) {
        for (int i = 0; i < SHM_TUNE_COUNT; ++i) {
            const char* e = getenv(kTune[i].env);
            int v = e ? atoi(e) : kTune[i].dflt;
            if (v < kTune[i].lo || v > kTune[i].hi) v = kTune[i].dflt;
            g_tune[i].store(v);
        }
        g_tune_init.store(2, std::memory_order_release);
    } else {
        while (g_tune_init.load(std::memory_order_acquire) != 2) {
        }
    }
}
int tune_find(const char* key) {
    if (!key) return -1;
    for (int i = 0; i < SHM_TUNE_COUNT; ++i)
        if (strcmp(key, kTune[i].key) == 0) return i;
    return -1;
}
}  // namespace

int shm_tune(int id) {
    tune_init();
    return g_tune[id].load(std::memory_order_relaxed);
}

extern "C" int shm_set_tuning(const char* key, int value) {
    tune_init();
    if (key && strcmp(key, "reset") == 0) {            // every knob back to its built-in default
        for (int i = 0; i < SHM_TUNE_COUNT; ++i) g_tune[i].store(kTune[i].dflt);
        return SHM_OK;
    }
    const int i = tune_find(key);
    SHM_REQUIRE(i >= 0, SHM_E_SHAPE, "shm_set_tuning: unknown key '%s'", key ? key : "(null)");
    if (value < 0) value = kTune[i].dflt;                // negative = default
    SHM_REQUIRE(value >= kTune[i].lo && value <= kTune[i].hi, SHM_E_SHAPE, "shm_set_tuning: %s = %d outside [%d, %d]", key, value,
                kTune[i].lo, kTune[i].hi);
    g_tune[i].store(value);
    return SHM_OK;
}

extern "C" int shm_get_tuning(const char* key, int* value) {
    tune_init();
    const int i = tune_find(key);
    SHM_REQUIRE(i >= 0 && value, SHM_E_SHAPE, "shm_get_tuning: unknown key '%s'", key ? key : "(null)");
    *value = g_tune[i].load();
    return SHM_OK;
}

extern "C" const char* shm_last_error(void) { return g_err; }
extern "C" const char* shm_last_kernel(void) { return g_kernel; }
extern "C" int shm_version(void) { return 203; }

// shm_set_clock_probe: measurement hook (bench.py's north-star ceiling).  While set on this thread, the ping-pong convolution kernel
// (tapgemm_pp_bf16_kernel) writes, from one wave of its middle block, dev2[0] = s_memtime ticks (shader clock) and dev2[1] = s_memrealtime ticks
// (100 MHz) spent in its patch loop: dev2[0] / dev2[1] x 0.1 = the clock in GHz the kernel held.  NULL (default) disarms; no other kernel reads it.
static thread_local unsigned long long* g_clock_probe = nullptr;
extern "C" int shm_set_clock_probe(unsigned long long* dev2) {
    g_clock_probe = dev2;
    return SHM_OK;
}
unsigned long long* shm_clock_probe() { return g_clock_probe; }
