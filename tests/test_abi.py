"""The C-ABI shared library loads on a CPU-only box and exports exactly what include/shmgan_hip.h
declares; the ctypes signature table and the constants are read from the header.  No compute call is made here."""
import ctypes as C
from pathlib import Path
import re

import pytest

from shmgan_amd import _lib


def exported_functions(lib):
    """The unmangled shm_* functions in the dynamic symbol table of `lib`: its C ABI as the linker sees it."""
    import subprocess
    out = subprocess.run(["/opt/rocm/lib/llvm/bin/llvm-readelf", "--dyn-syms", "--wide", str(lib)], check=True, capture_output=True, text=True).stdout
    rows = [ln.split() for ln in out.splitlines()]
    return {r[7] for r in rows if len(r) == 8 and r[3] == "FUNC" and r[4] in ("GLOBAL", "WEAK") and r[6] != "UND" and re.fullmatch(r"shm_[a-z0-9_]+", r[7])}


def test_header_table_and_exports_agree():
    hdr = _lib.header_functions()
    assert len(hdr) == len(set(hdr)), "duplicate declaration in the header"
    assert set(hdr) == set(_lib.SIGNATURES), (set(hdr) ^ set(_lib.SIGNATURES))
    _lib.build()
    L = _lib.lib()
    for name in hdr:
        assert hasattr(L, name), f"{name} not exported by libshmgan_hip.so"
    # ... and nothing else: an entry point that left the header (the per-thread request and abort-word setters did) has left the library too
    exports = exported_functions(_lib.LIB_PATH)
    assert exports == set(hdr), (exports ^ set(hdr))


SYNTHETIC_HEADER = r"""
/* a comment that holds a prototype: int shm_fake(int); */
#ifndef SHM_GUARD
#define SHM_GUARD
#define SHM_EMIN (-40)
#define SHM_BINS 44            /* a trailing comment
                                  that goes on */
#define SHM_RATIO 0.5
#define SHM_SIZED ((size_t)SHM_BINS * 7 + 8)
#define SHM_DECLARE(n, c)                        \
    int shm_in_macro(int n, short c);            \
    int shm_in_macro_too(int n)
typedef struct shm_thing {
    int shm_member(short x);
    const unsigned char* src[5];
    int plane[4];
} shm_thing;
int shm_three_lines(const void* const* w, const char* key,
                    unsigned long long seed, long long step, unsigned mask,
                    float coef[12], double d, const shm_thing* things, int n, void* stream);
const char* shm_text(void);
size_t shm_bytes(int n, size_t m, float);
void shm_nothing();
#endif
"""


def test_header_parser_on_a_synthetic_header():
    """_lib.parse_header, which _lib.SIGNATURES and _lib.CONSTANTS are the result of: declarations over several lines, prototypes inside
    comments, macros and struct bodies, every scalar type it knows, pointers and arrays, and a type it does not know."""
    P = C.c_void_p
    sigs, consts = _lib.parse_header(SYNTHETIC_HEADER)
    assert list(sigs) == ["shm_three_lines", "shm_text", "shm_bytes", "shm_nothing"]
    assert sigs["shm_three_lines"] == (C.c_int, [P, C.c_char_p, C.c_ulonglong, C.c_longlong, C.c_uint, P, C.c_double, P, C.c_int, P])
    assert sigs["shm_text"] == (C.c_char_p, [])
    assert sigs["shm_bytes"] == (C.c_size_t, [C.c_int, C.c_size_t, C.c_float])
    assert sigs["shm_nothing"] == (None, [])
    assert consts == {"SHM_EMIN": -40, "SHM_BINS": 44}           # not the guard, the float, the expression or the function-like macro
    with pytest.raises(ValueError, match=r"shm_bad.*short x"):
        _lib.parse_header(SYNTHETIC_HEADER + "int shm_bad(int n, short x);\n")
    with pytest.raises(ValueError, match=r"shm_worse.*long"):
        _lib.parse_header("long shm_worse(void);\n")
    with pytest.raises(ValueError, match="shm_text.*twice"):
        _lib.parse_header(SYNTHETIC_HEADER + "const char* shm_text(void);\n")


def test_header_signatures_are_pinned_by_type():
    """The table is read from the header, so its argument counts agree with it by construction; these entries are written out, restype and
    every argtype, for the declarations with the types a wrong guess would corrupt silently (tests/test_native_cpu.py pins five more)."""
    I, P, Z, F = C.c_int, C.c_void_p, C.c_size_t, C.c_float
    pins = {
        "shm_randn": (I, [P, Z, F, C.c_ulonglong, C.c_uint, P]),
        "shm_loss_ring_put": (I, [P, P, P, P, P, I, I, C.c_longlong, P]),
        "shm_sum_input_channels": (I, [P, I, I, C.c_uint, P, P]),
        "shm_set_tuning": (I, [C.c_char_p, I]),
        "shm_get_tuning": (I, [C.c_char_p, P]),
        "shm_last_error": (C.c_char_p, []),
        "shm_conv2d_wgrad_workspace": (Z, [I, I, I, I, I, I]),
        "shm_in_bwd": (I, [P, I, P, I, P, I, P, P, P, I, P, P, P, Z, P, P, I, I, I, I, F, I, P]),
        "shm_augment_batch_u8": (I, [P, I, I, I, P, P, P, Z, I, I, F, P]),
    }
    for name, sig in pins.items():
        assert _lib.SIGNATURES[name] == sig, name
    assert _lib.header_functions() == list(_lib.SIGNATURES)
    assert (_lib.F32, _lib.BF16, _lib.CONSTANTS["SHM_BF16_GF32"], _lib.CONSTANTS["SHM_E_HIP"], _lib.CONSTANTS["SHM_THIST_EMIN"]) == (0, 1, 2, -4, -40)
    assert not any("(" in k or k.endswith("_DOUBLES") for k in _lib.CONSTANTS)      # the function-like and computed macros stay Python functions


def test_default_arena_is_made_once_per_device():
    import torch
    from shmgan_amd import ops
    dev = torch.device("cpu")
    a = ops._default_arena(dev)
    assert ops._default_arena(dev) is a and ops._default_arena(torch.device("cpu")) is a and ops._METRIC_ARENAS[dev] is a


def test_square_export_descriptor_words():
    """Host side of ops.export_u8: the SHM_EXPORT_DESC words per job handed to shm_export_u8 are {S, C, ld, ho, wo, mode, k, destination
    offset} (include/shmgan_hip.h), written out here for a 4x4x3 plane of pixel pitch 5 and a one-channel plane behind it."""
    import torch
    from shmgan_amd import ops

    class Plane:            # what _export_jobs reads of a device tensor
        dtype, is_cuda, device = torch.float32, True, "cuda:0"

        def __init__(self, shape, strides):
            self.shape, self.strides = shape, strides

        def dim(self):
            return len(self.shape)

        def stride(self, i=None):
            return self.strides if i is None else self.strides[i]

    mul = torch.ones(3)
    desc, offs, total = ops._export_jobs("export_u8", [Plane((4, 4, 3), (20, 5, 1)), Plane((4, 4, 1), (20, 5, 1))], None, [(6, 7), (4, 4)],
                                         ["clip", ("scale", 2)], mul)
    assert desc == [[4, 3, 5, 6, 7, 2, 0, 0], [4, 1, 5, 4, 4, 1, 2, 128]]          # 6 * 7 * 3 = 126 bytes, the next job from 128
    assert offs == [0, 128] and total == 144 and all(len(d) == ops.EXPORT_DESC == 8 for d in desc)
    # the windowed form's SHM_EXPORT_HW_DESC words: {Hs, Ws, C, ld, y0, x0, hc, wc, ho, wo, mode, k, destination offset}
    desc, offs, total = ops._export_jobs("export_u8_hw", [Plane((4, 6, 3), (30, 5, 1))], [(1, 2, 3, 4)], [(6, 7)], ["rescale"], None)
    assert desc == [[4, 6, 3, 5, 1, 2, 3, 4, 6, 7, 0, 0, 0]] and len(desc[0]) == ops.EXPORT_HW_DESC == 13 and (offs, total) == ([0], 128)
    with pytest.raises(ValueError, match=r"export_u8 takes \[S,S,C\] planes"):
        ops._export_jobs("export_u8", [Plane((4, 6, 3), (30, 5, 1))], None, [(6, 7)], ["clip"], None)
    with pytest.raises(ValueError, match=r"export_u8_hw: window \(1, 2, 4, 4\) outside the 4 x 6 plane"):
        ops._export_jobs("export_u8_hw", [Plane((4, 6, 3), (30, 5, 1))], [(1, 2, 4, 4)], [(6, 7)], ["clip"], None)


def test_version_and_error_string_without_gpu():
    L = _lib.lib()
    assert L.shm_version() >= 100
    # shape errors are detected on the host before any launch: safe without a GPU
    rc = L.shm_conv2d_fwd(None, None, 0, 24, 0, None, None, None, 24, 1, 4, 4, 24, 16, 3, 1, 1.0, _lib.F32, None)
    assert rc == -1 and b"null pointer" in L.shm_last_error()
    rc = L.shm_conv2d_wgrad(1, None, 0, 16, 0, 1, 16, 1, 1, 4, 4, 16, 16, 16, 5, 1, 0, 1, 0, _lib.F32, None)
    assert rc == -1 and b"ksize" in L.shm_last_error()
    rc = L.shm_conv2d_wgrad(None, None, 0, 16, 0, None, 16, None, 1, 4, 4, 16, 16, 16, 3, 1, 0, None, 0, _lib.F32, None)
    assert rc == -1 and b"null pointer" in L.shm_last_error()
    # an unknown element type is SHM_E_DTYPE (-2), also detected before any launch
    rc = L.shm_conv2d_wgrad(1, None, 0, 16, 0, 1, 16, 1, 1, 4, 4, 16, 16, 16, 3, 1, 0, 1, 0, 7, None)
    assert rc == -2 and b"dtype" in L.shm_last_error()
    assert L.shm_conv2d_wgrad_workspace(8, 256, 256, 64, 64, 3) > 0
    assert L.shm_image_losses_workspace(8, 256) > 0


def test_in_bwd_requests_are_arguments_not_thread_state():
    """The InstanceNorm backward takes its dz_sums / fused scratch / abort words as arguments: no kernel source keeps per-thread request state
    (runtime.hip holds the error string, the last kernel's name and the clock probe, its one per-thread pointer), and the entry points that
    armed it are gone from the header, the table and the library."""
    csrc = Path(_lib.__file__).resolve().parent / "csrc"
    for f in sorted([*csrc.glob("*.hip"), *csrc.glob("*.h")]):
        if f.name != "runtime.hip":
            assert "thread_local" not in f.read_text(), f.name
    runtime = re.sub(r"//.*", "", (csrc / "runtime.hip").read_text())
    assert re.findall(r"thread_local[^;=]*\*\s*(\w+)", runtime) == ["g_clock_probe"]
    L = _lib.lib()
    for name in ("shm_in_bwd_keep_dz_sums", "shm_in_bwd_fused_scratch"):
        assert name not in _lib.HEADER.read_text() and name not in _lib.SIGNATURES and not hasattr(L, name), name


def test_every_source_is_built():
    csrc = Path(_lib.__file__).resolve().parent / "csrc"
    assert sorted(f.name for f in csrc.glob("*.hip")) == sorted(_lib.SOURCES)
    assert all(h.exists() for h in _lib.SHARED_HEADERS)


def test_dz_sums_need_a_bias_gradient_without_gpu():
    """dz_sums are copied out of the bias gradient's staging: asked for without dbias, all three entry points answer SHM_E_SHAPE with the
    same message, before any launch (and before their other pointer checks)."""
    L = _lib.lib()
    p, f32 = 1, _lib.F32            # a non-null pointer nobody dereferences
    rc = L.shm_in_bwd(p, 64, None, 0, p, 64, p, p, p, 64, None, p, None, 0, None, None, 1, 8, 8, 64, 0.2, f32, None)
    assert rc == -1 and b"bias gradient" in L.shm_last_error()
    rc = L.shm_in_bwd_apply(None, 64, None, 0, None, 64, None, None, None, None, None, None, 64, None, p, 1, 8, 8, 64, 0.2, f32, None)
    assert rc == -1 and b"bias gradient" in L.shm_last_error()
    rc = L.shm_in_bwd_rank1(p, p, p, 64, p, p, p, 64, None, p, 1, 8, 8, 64, 0.2, f32, None)
    assert rc == -1 and b"bias gradient" in L.shm_last_error()


def test_product_refuses_to_run_without_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from shmgan_amd import ShmGANwithSSpecSeg
    with pytest.raises(RuntimeError):
        ShmGANwithSSpecSeg(image_size=64, filter_size=16)


def test_product_does_not_import_oracle():
    import pathlib
    pat = re.compile(r"^\s*(from|import)\s+oracle\b", re.M)
    for p in pathlib.Path(_lib.__file__).resolve().parent.glob("*.py"):
        assert not pat.search(p.read_text()), f"{p} imports the oracle (test infrastructure only)"


def test_trainer_surface_matches_the_reference_object():
    """The methods and signatures main.py / test.py use on the reference's trainer object:
    __init__(args), build_generator(), build_discriminator(), train_step(5 tensors), train(args) (main.py:107),
    custom_per_image_standardization, gram_matrix."""
    import inspect
    from shmgan_amd import ShmGANwithSSpecSeg as T
    assert list(inspect.signature(T.train).parameters)[:2] == ["self", "args"]
    assert list(inspect.signature(T.train_step).parameters)[:6] == ["self", "orig0", "orig45", "orig90", "orig135", "origED"]
    for name in ("build_generator", "build_discriminator", "custom_per_image_standardization", "gram_matrix", "infer",
                 "save_npz", "load_npz"):
        assert callable(getattr(T, name))


def test_tuning_keys_roundtrip_without_gpu():
    L = _lib.lib()
    v = C.c_int(-5)
    assert L.shm_get_tuning(b"tapgemm.variant", C.addressof(v)) == 0 and v.value == 0
    assert L.shm_set_tuning(b"tapgemm.variant", 3) == 0
    assert L.shm_get_tuning(b"tapgemm.variant", C.addressof(v)) == 0 and v.value == 3
    assert L.shm_set_tuning(b"tapgemm.variant", 99) == -1 and b"outside" in L.shm_last_error()
    assert L.shm_set_tuning(b"bogus", 1) == -1 and b"unknown key" in L.shm_last_error()
    assert L.shm_set_tuning(b"reset", 0) == 0
    assert L.shm_get_tuning(b"tapgemm.variant", C.addressof(v)) == 0 and v.value == 0
    for key, dflt in ((b"tapgemm.halo_min_blocks", 1024), (b"tapgemm.small_grid_blocks", 1024), (b"wgrad.variant", 0),
                      (b"wgrad.blocks", 0), (b"stats.fusion", 1), (b"elem.reverse", 1), (b"tapgemm.phase4_min_blocks", 256),
                      (b"wgrad.bf16_rows", 0), (b"elem.reduce_blocks", 0)):
        assert L.shm_get_tuning(key, C.addressof(v)) == 0 and v.value == dflt, key


def test_generator_gradient_buckets_partition_the_flat_buffer():
    """The data-parallel bucket plan (G gradients in reverse-layer buckets) covers every element of the flat
    gradient exactly once, and every bucket's trigger layer is the lowest layer stored in it."""
    import torch
    from shmgan_amd.model import Arena, Generator
    dev = torch.device("cpu")
    for F in (16, 64):
        g = Generator(64, F, dev, Arena(dev), lambda n: None)
        plan = g.grad_buckets()
        seen = torch.zeros(g.P.n, dtype=torch.int32)
        for trig, slices in plan:
            for lo, hi in slices:
                assert 0 <= lo < hi <= g.P.n
                seen[lo:hi] += 1
            if trig is not None:
                assert slices[0][0] == g.P.offsets[2 * trig]
        assert int(seen.min()) == 1 and int(seen.max()) == 1
        assert [t for t, _ in plan] == [16, 10, 4, None]
        if F == 64:
            mb = [sum(hi - lo for lo, hi in sl) * 4 / 1e6 for _, sl in plan]
            assert abs(sum(mb) - 74.1) < 0.1 and mb[1] > 45


def test_fused_in_bwd_scratch_size_and_timeout_report():
    """Host side of the one-pass bf16 InstanceNorm backward (include/shmgan_hip.h: SHM_IN_BWD_FUSED_DOUBLES): ops.in_bwd_fused_doubles is the
    header's macro, the scratch exists only for bfloat16 activations, and a set timeout word is reported by name (Trainer.losses raises on it)."""
    import re
    import torch
    from shmgan_amd import ops
    from shmgan_amd.model import Arena, _fused_scratch
    hdr = (Path(__file__).resolve().parent.parent / "include" / "shmgan_hip.h").read_text()
    m = re.search(r"#define SHM_IN_BWD_FUSED_DOUBLES\(batch, hw, c\)\s*\\\n((?:.*\\\n)*.*)", hdr)
    assert m, "macro not found"
    expr = re.sub(r"\(size_t\)", "", m.group(1)).replace("\\\n", " ").replace("/", "//").replace("SHM_IN_BWD_FUSED_CB(c)", "min(c, 64)")
    for batch, hw, c in ((40, 65536, 64), (8, 16384, 128), (3, 1024, 512), (1, 4096, 8)):
        assert ops.in_bwd_fused_doubles(batch, hw, c) == eval(expr, {"batch": batch, "hw": hw, "c": c}), (batch, hw, c)
    # ... and so are the two workspace sizes of the SpecSeg training kernels
    bn = re.search(r"#define SHM_BN_TRAIN_WS_DOUBLES\(c\) (.*)", hdr).group(1).replace("(size_t)", "")
    for c in (1, 16, 256):
        assert ops.bn_train_ws_doubles(c) == eval(bn, {"c": c, **_lib.CONSTANTS}), c
    seg = re.search(r"#define SHM_SEG_LOSS_WS_DOUBLES (.*)", hdr).group(1).replace("(size_t)", "")
    assert ops.SEG_LOSS_WS_DOUBLES == eval(seg, dict(_lib.CONSTANTS)) == 1800
    A = Arena(torch.device("cpu"))
    assert _fused_scratch(A, torch.float32, 2, 4096, 64) is None
    t = _fused_scratch(A, torch.bfloat16, 2, 4096, 64)
    assert t.dtype == torch.float64 and t.numel() == ops.in_bwd_fused_doubles(2, 4096, 64) and float(t.abs().max()) == 0.0
    assert _fused_scratch(A, torch.bfloat16, 2, 4096, 64) is t
    u = _fused_scratch(A, torch.bfloat16, 4, 1024, 128)
    assert A.fused_timeouts() == []
    u[-1] = 4.9e-324          # the timeout word is a uint32 in the last float64: any set bit
    assert A.fused_timeouts() == ["bwd/fused/4x1024x128"]


def test_every_pipeline_barrier_waits_for_its_lds_reads():
    """Source lint for the race fixed in round 2: a raw s_barrier in a kernel source would let a wave enter the barrier with
    fragment reads still queued (the refill of the stage is issued right after it); kernels use SHM_LDS_BARRIER() -- s_waitcnt
    lgkmcnt(0) + s_barrier -- or __syncthreads()."""
    from pathlib import Path
    csrc = Path(_lib.__file__).resolve().parent / "csrc"
    for f in sorted(csrc.glob("*.hip")):
        assert "__builtin_amdgcn_s_barrier" not in f.read_text(), f.name
    common = (csrc / "common.h").read_text()
    i = common.index("#define SHM_LDS_BARRIER()")
    body = common[i:i + 400]
    assert body.index("s_waitcnt lgkmcnt(0)") < body.index("__builtin_amdgcn_s_barrier()")


def test_built_library_has_no_store_data_hazard():
    """ISA lint for the fault found in round 4 (tools/check_isa_hazards.py): no VALU write into the data registers of a 12- / 16-byte store
    within two wait states of it, anywhere in the library's gfx950 code -- hipcc does not space that out after buffer stores with an SGPR
    soffset, and an inline-asm v_max landed there.  The scanner itself is checked on a crafted listing."""
    import importlib.util
    from pathlib import Path
    root = Path(_lib.__file__).resolve().parents[1]
    spec = importlib.util.spec_from_file_location("check_isa_hazards", root / "tools" / "check_isa_hazards.py")
    chk = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(chk)
    bad = "0000 <k>:\n\tbuffer_store_dwordx4 v[16:19], v104, s[36:39], s66 offen\n\tv_max_f32_e32 v17, v12, v0\n"
    ok1 = "0000 <k>:\n\tbuffer_store_dwordx4 v[16:19], v104, s[36:39], s66 offen\n\ts_nop 1\n\tv_max_f32_e32 v17, v12, v0\n"
    ok2 = "0000 <k>:\n\tglobal_store_dwordx4 v[16:17], v[20:23], off\n\tv_lshl_add_u64 v[16:17], v[16:17], 0, 16\n\tv_mov_b32_e32 v1, v2\n\tv_mov_b32_e32 v20, v2\n"
    bad2 = "0000 <k>:\n\tglobal_store_dwordx4 v[16:17], v[20:23], off\n\tv_mov_b32_e32 v1, v2\n\tv_pk_add_f32 v[22:23], v[2:3], v[4:5]\n"
    assert len(chk.scan(bad)) == 1 and len(chk.scan(bad2)) == 1 and not chk.scan(ok1) and not chk.scan(ok2)
    # ... and its second rule: no VALU read of an MFMA's VGPR result within passes + 2 wait states of it, per MFMA shape (another MFMA may
    # chain on it and counts as its own passes; a VALU write to the register supersedes the result; an unconditional branch ends the window)
    bad3 = "0000 <k>:\n\tv_mfma_f32_16x16x4_f32 v[0:3], v4, v5, v[0:3]\n\tv_mov_b32_e32 v7, v8\n\tv_max_f32_e32 v9, v1, v2\n"
    bad4 = "0000 <k>:\n\tv_mfma_f32_16x16x4_f32 v[0:3], v4, v5, v[0:3]\n\ts_nop 4\n\tv_max_f32_e32 v9, v1, v2\n"          # 8 passes want 10
    bad5 = "0000 <k>:\n\tv_mfma_f32_16x16x32_bf16 v[0:3], v[4:7], v[8:11], v[0:3]\n\ts_nop 3\n\tv_cvt_pk_bf16_f32 v9, v0, v1\n"   # 4 passes want 6
    ok3 = "0000 <k>:\n\tv_mfma_f32_16x16x4_f32 v[0:3], v4, v5, v[0:3]\n\ts_nop 7\n\ts_nop 1\n\tv_max_f32_e32 v9, v1, v2\n"
    ok4 = "0000 <k>:\n\tv_mfma_f32_16x16x4_f32 v[0:3], v4, v5, v[0:3]\n\tv_mfma_f32_16x16x4_f32 v[0:3], v6, v7, v[0:3]\n\tv_mfma_f32_16x16x4_f32 a[0:3], v6, v7, a[0:3]\n"
    ok5 = "0000 <k>:\n\tv_mfma_f32_16x16x32_bf16 v[0:3], v[4:7], v[8:11], v[0:3]\n\ts_nop 5\n\tv_cvt_pk_bf16_f32 v9, v0, v1\n"
    ok6 = "0000 <k>:\n\tv_mfma_f32_16x16x4_f32 v[0:3], v4, v5, v[0:3]\n\tv_mov_b32_e32 v1, 0\n\tv_max_f32_e32 v9, v1, v1\n"                 # v1 rewritten
    ok7 = "0000 <k>:\n\tv_mfma_f32_16x16x4_f32 v[0:3], v4, v5, v[0:3]\n\ts_branch 12\n\tv_max_f32_e32 v9, v1, v2\n"                       # not fall-through
    assert len(chk.scan(bad3)) == 1 and len(chk.scan(bad4)) == 1 and len(chk.scan(bad5)) == 1
    assert not chk.scan(ok3) and not chk.scan(ok4) and not chk.scan(ok5) and not chk.scan(ok6) and not chk.scan(ok7)
    assert chk.main(["check_isa_hazards.py", str(_lib.LIB_PATH)]) == 0


def test_bench_refuses_a_rank_count_that_disagrees_with_the_launcher():
    """bench.py --gpus N is the contract the driver computes scaling from: with WORLD_SIZE != N it must not print a line at all
    (round 2 printed n_gpus: 1 for `--gpus 8` launched as plain python).  The check runs before anything touches the GPU."""
    import os
    import subprocess
    import sys
    from pathlib import Path
    root = Path(__file__).resolve().parent.parent
    env = dict(os.environ, WORLD_SIZE="1", RANK="0", LOCAL_RANK="0")
    r = subprocess.run([sys.executable, str(root / "bench.py"), "--gpus", "4", "--steps", "1", "--warmup", "0"], env=env, capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 2 and r.stdout.strip() == "" and "WORLD_SIZE=1" in r.stderr
