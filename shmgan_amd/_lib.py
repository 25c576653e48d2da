"""ctypes binding of libshmgan_hip.so (the C ABI declared in include/shmgan_hip.h).

The product path has no CPU fallback: if the shared library is missing or a call fails
this module raises.  `build()` (re)compiles the library in-tree with hipcc for gfx950.
"""
from __future__ import annotations

import ctypes as C
import os
import re
import subprocess
from pathlib import Path

_HERE = Path(__file__).resolve().parent
# SHM_LIB_PATH: load another build of the same ABI (tools/ablate_conv.py times ablated kernels this way)
LIB_PATH = Path(os.environ["SHM_LIB_PATH"]) if os.environ.get("SHM_LIB_PATH") else _HERE / "libshmgan_hip.so"
CSRC = _HERE / "csrc"
HEADER = _HERE.parent / "include" / "shmgan_hip.h"
SOURCES = ["runtime.hip", "conv_igemm.hip", "conv_dma.hip", "conv_halo.hip", "conv_wreg.hip", "conv_wreg_f32.hip", "conv_phase4.hip", "conv_wreg16.hip", "conv_pingpong.hip", "conv_wgrad.hip", "conv_wgrad_gen.hip", "conv_wgrad_halo.hip", "conv_wgrad_halo16.hip", "conv_wgrad_halo8.hip", "conv_wgrad_x3.hip", "conv_fwd_x3.hip", "conv_rgb.hip", "elem.hip", "instnorm.hip", "instnorm_bwd.hip", "instnorm_bwd_2pass.hip", "instnorm_bwd_fused8.hip", "instnorm_bwd_fusedg.hip", "grad_sums.hip", "heads.hip", "dgrad_sum1.hip", "color.hip", "ema.hip", "imgloss.hip", "metrics.hip", "specseg.hip", "data.hip", "polar.hip", "dofp.hip", "dofp_develop.hip", "dofp_calibrate.hip", "dofp_merge.hip", "specmask.hip", "augment.hip", "augment_batch.hip", "augment_pairs.hip", "export.hip", "detail.hip", "telemetry.hip", "specseg_train.hip"]
# headers every source may include: a change of any of them rebuilds every object (tools/sanitize_host.py goes by the same list)
SHARED_HEADERS = [CSRC / "common.h", CSRC / "elem.h", CSRC / "ablate.h", CSRC / "tapgemm.h", CSRC / "tapgemm_dev.h", CSRC / "wgrad.h", CSRC / "wgrad_halo_dev.h", CSRC / "in_bwd.h", CSRC / "x3split.h", CSRC / "polar_est.h", CSRC / "dofp_dev.h", CSRC / "augment_px.h", CSRC / "bilinear.h", CSRC / "yuv.h", HEADER]
HIPCC_FLAGS = ["--offload-arch=gfx950", "-O3", "-fPIC", "-shared", "-munsafe-fp-atomics",
               "-Wall", "-Wno-unused-function", "-Wno-unused-local-typedef"]

# per-source extra flags.  conv_pingpong.hip: its epilogue runs beside the partner wave's MFMAs, where the packed f32 instructions the SLP vectoriser
# forms (v_pk_add_f32 / v_pk_mul_f32) cost several times their scalar pairs (MI355X guide, cycle constants)
EXTRA_FLAGS = {"conv_pingpong.hip": ["-fno-slp-vectorize"]}

# C scalar types of the header -> ctypes; every pointer or array is c_void_p, except `const char*`
_C_SCALARS = {"void": None, "int": C.c_int, "float": C.c_float, "double": C.c_double, "size_t": C.c_size_t, "unsigned": C.c_uint,
              "long long": C.c_longlong, "unsigned long long": C.c_ulonglong}


def _ctype(decl, fn):
    """ctypes class of one return type or parameter declaration (its name, if any, included) of function `fn`."""
    words = re.sub(r"\bconst\b", " ", decl).split()
    if "*" in decl or "[" in decl:
        return C.c_char_p if "".join(words).startswith("char*") and decl.count("*") == 1 and "[" not in decl else C.c_void_p
    for t in (" ".join(words), " ".join(words[:-1])):          # without a parameter name, with one
        if t in _C_SCALARS:
            return _C_SCALARS[t]
    raise ValueError(f"{fn}: no ctypes class for the C type in {decl.strip()!r}")


def parse_header(txt):
    """(SIGNATURES, CONSTANTS) of a C header's text: name -> (restype, argtypes) for every `ret shm_name(args);` in declaration order,
    and name -> int for every object-like `#define SHM_X <integer>` or `(-<integer>)`.  A type outside _C_SCALARS raises."""
    txt = re.sub(r"/\*.*?\*/", " ", txt, flags=re.S)
    consts = {m.group(1): int(m.group(2).strip("()"))
              for m in re.finditer(r"^[ \t]*#[ \t]*define[ \t]+(SHM_\w+)[ \t]+(\(-\d+\)|\d+)[ \t]*$", txt, flags=re.M)}
    txt = re.sub(r"^[ \t]*#(?:.*\\\n)*.*$", "", txt, flags=re.M)                  # preprocessor lines and their continuations
    txt = re.sub(r"\btypedef\s+struct\b[^{};]*\{[^{}]*\}[^;]*;", "", txt)      # struct bodies: their members are no prototypes
    sigs = {}
    for m in re.finditer(r"([\w\s*]+?)\b(shm_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", txt):
        ret, fn, args = m.group(1), m.group(2), m.group(3).strip()
        if fn in sigs:
            raise ValueError(f"{fn}: declared twice")
        sigs[fn] = (_ctype(ret, fn), [] if args in ("", "void") else [_ctype(a, fn) for a in args.split(",")])
    return sigs, consts


# name -> (restype, argtypes), and the header's integer constants: read from include/shmgan_hip.h, which is the one statement of the ABI
SIGNATURES, CONSTANTS = parse_header(HEADER.read_text())
F32, BF16 = CONSTANTS["SHM_F32"], CONSTANTS["SHM_BF16"]


def header_functions():
    """Names declared in include/shmgan_hip.h, in its order."""
    return list(SIGNATURES)


def build(force=False, verbose=False, jobs=None):
    """Compile csrc/*.hip into libshmgan_hip.so with hipcc (cross-compiles without a GPU): one object per source under
    csrc/_obj/ (rebuilt when older than its source or a shared header, or when the compile command changed; up to `jobs` at a
    time), then one link.  Objects and the library are written under temporary names and renamed into place, so that
    several ranks building a stale tree at once never read each other's half-written files."""
    import hashlib
    from concurrent.futures import ThreadPoolExecutor
    srcs = [CSRC / s for s in SOURCES]
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    cflags = [f for f in HIPCC_FLAGS if f != "-shared"]
    # what the objects were built WITH: compiler, flags and source list (a change of HIPCC_FLAGS must not relink stale objects)
    stamp_txt = hashlib.sha256(" ".join([hipcc, *cflags, *SOURCES, repr(sorted(EXTRA_FLAGS.items()))]).encode()).hexdigest()
    objdir = CSRC / "_obj"
    objdir.mkdir(exist_ok=True)
    stamp = objdir / "flags.sha256"
    same_cmd = stamp.exists() and stamp.read_text().strip() == stamp_txt
    deps = srcs + SHARED_HEADERS
    if not force and same_cmd and LIB_PATH.exists():
        newest = max(p.stat().st_mtime for p in deps)
        if LIB_PATH.stat().st_mtime >= newest:
            return LIB_PATH
    hdr_time = max(p.stat().st_mtime for p in SHARED_HEADERS)
    todo = []
    for src in srcs:
        obj = objdir / (src.stem + ".o")
        if force or not same_cmd or not obj.exists() or obj.stat().st_mtime < max(src.stat().st_mtime, hdr_time):
            todo.append((obj, [hipcc, *cflags, *EXTRA_FLAGS.get(src.name, []), "-c", str(src)]))

    def run(cmd, out):
        tmp = out.with_name(f".{out.name}.{os.getpid()}.tmp")
        if verbose:
            print(" ".join(cmd + ["-o", str(out)]), flush=True)
        try:
            subprocess.run(cmd + ["-o", str(tmp)], check=True)
            os.replace(tmp, out)
        finally:
            if tmp.exists():
                tmp.unlink()
    with ThreadPoolExecutor(max_workers=jobs or min(4, os.cpu_count() or 1)) as ex:
        list(ex.map(lambda t: run(t[1], t[0]), todo))
    run([hipcc, "--offload-arch=gfx950", "-fPIC", "-shared", *[str(objdir / (src.stem + ".o")) for src in srcs]], LIB_PATH)
    stamp.write_text(stamp_txt + "\n")
    return LIB_PATH


_lib = None


def lib():
    """Load the shared library (once).  Raises if it is missing: there is no fallback."""
    global _lib
    if _lib is None:
        if not LIB_PATH.exists():
            raise RuntimeError(
                f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(hipcc --offload-arch=gfx950).  shmgan_amd has no CPU/PyTorch fallback.")
        L = C.CDLL(str(LIB_PATH))
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


class ShmError(RuntimeError):
    pass


def check(rc, name):
    if rc != 0:
        msg = lib().shm_last_error()
        raise ShmError(f"{name} failed ({rc}): {msg.decode() if msg else ''}")
