"""shm_dofp_views (csrc/dofp.hip) on 2448 x 2048 frames, the Sony IMX250MZR / MYR's: microseconds per frame, achieved bytes/s and the
share of the HBM peak, for 8-bit mono, 12-bit mono, 12-bit RGGB bilinear and 12-bit RGGB bin, with and without the total plane;
and the host time PIL takes to decode the four view PNGs the one mosaic replaces; then shm_dofp_develop (csrc/dofp_develop.hip) on the
same frames by the same protocol, beside the plain launch in the same run: 12-bit mono and RGGB, bilinear and bin, and 8-bit bilinear, without and with the
colour matrix, and with wb "gray" including its two estimation launches; then shm_dofp_calibrate (csrc/dofp_calibrate.hip) at 8 and 12 bits, with
all three tables and with the dark frame alone, beside a device copy of the same bytes and the plain RGGB demosaic launch of the same frame;
then shm_dofp_merge (csrc/dofp_merge.hip) of a bracket of three pages at 8 and 12 bits, with and without counts, beside a device copy of the
same bytes (three pages read, one 16-bit page written) and the calibrate launch (dark frame alone) of one page.
A record for kernel work, not an acceptance number.

Bytes are algorithmic and computed from the shapes here: the mosaic read once plus the planes written.  Device events around
LAUNCHES launches, 2 warm-ups and 5 timed iterations, seeded data.  The launches rotate over SETS source / destination sets (more
than the 256 MiB Infinity Cache together), so that a frame comes from and goes to HBM as a camera's next frame would.
python tools/bench_dofp.py [--launches N] [--no-views] [--no-decode] [--no-develop] [--no-calibrate] [--no-merge]"""
import argparse
import ctypes as C
import io
import sys
import time
from pathlib import Path
sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import numpy as np
import torch
from shmgan_amd import _lib, ops

W, H = 2448, 2048
HBM_PEAK = 8.0e12            # bytes/s, the MI355X's specification; ~6.3e12 is what a float4 copy achieves
HBM_COPY = 6.29e12
SETS = 6
CONFIGS = [("8-bit mono bilinear", "mono", 8, "bilinear"), ("12-bit mono bilinear", "mono", 12, "bilinear"),
           ("12-bit RGGB bilinear", "rggb", 12, "bilinear"), ("12-bit RGGB bin", "rggb", 12, "bin")]
QUAD = (2, 1, 3, 0)          # Sony: 90 / 45 / 135 / 0


def launcher(pattern, bits, mode, total, rng):
    """(fn that launches on set i, bytes per launch)."""
    L = _lib.lib()
    ho, wo = ops.dofp_shape(H, W, pattern, mode)
    dt = np.uint8 if bits == 8 else np.uint16
    nplanes = 5 if total else 4
    quad = (C.c_int * 4)(*QUAD)
    sets = []
    for _ in range(SETS):
        src = torch.from_numpy(rng.integers(0, 1 << bits, (H, W)).astype(dt)).cuda()
        out = torch.empty((nplanes, ho, wo, 3), dtype=torch.uint8, device="cuda")
        sets.append((src, out, (C.c_void_p * 4)(*[out[v].data_ptr() for v in range(4)]), out[4].data_ptr() if total else None))
    st = torch.cuda.current_stream().cuda_stream
    pc, mc = ops.DOFP_PATTERNS[pattern], ops.DOFP_MODES[mode]

    def fn(i):
        src, _, dp, tp = sets[i % SETS]
        _lib.check(L.shm_dofp_views(src.data_ptr(), bits, H, W, W, pc, quad, mc, dp, tp, st), "shm_dofp_views")
    return fn, H * W * np.dtype(dt).itemsize + nplanes * ho * wo * 3


# the 8-bit rows: an 8-bit sensor's multiplier never fits 24 bits, so its product takes three multiplies where a 12-bit one takes two
DEVELOP_CONFIGS = [("12-bit mono bilinear", "mono", 12, "bilinear"), ("12-bit mono bin", "mono", 12, "bin"),
                   ("12-bit RGGB bilinear", "rggb", 12, "bilinear"), ("12-bit RGGB bin", "rggb", 12, "bin"),
                   ("8-bit mono bilinear", "mono", 8, "bilinear"), ("8-bit RGGB bilinear", "rggb", 8, "bilinear")]
CCM = ((1.6, -0.4, -0.2), (-0.3, 1.5, -0.2), (0.1, -0.6, 1.5))


def develop_launcher(pattern, bits, mode, total, rng, what):
    """(fn that launches on set i, bytes per launch) for what = "views" (the plain launch), "develop", "matrix" or "gray" (the two
    grey-world launches and the development that reads their gains)."""
    from shmgan_amd.polar import DofpDevelop, DofpLayout
    L = _lib.lib()
    ho, wo = ops.dofp_shape(H, W, pattern, mode)
    nplanes = 5 if total else 4
    quad = (C.c_int * 4)(*QUAD)
    mono = pattern == "mono"
    dt = np.uint8 if bits == 8 else np.uint16
    lay = DofpLayout(pattern, bits=bits, develop=DofpDevelop(black=240 >> (12 - bits) if bits < 12 else 240, wb="gray" if what == "gray" else (1, 1, 1) if mono else (1.9, 1, 1.6),
                                                             ccm=CCM if what == "matrix" else None, tone="srgb"))
    params, lut, mirror = ops._dofp_tables(lay, torch.device("cuda", torch.cuda.current_device()))
    sets = []
    for _ in range(SETS):
        src = torch.from_numpy(rng.integers(0, 1 << bits, (H, W)).astype(dt)).cuda()
        out = torch.empty((nplanes, ho, wo, 3), dtype=torch.uint8, device="cuda")
        sets.append((src, out, (C.c_void_p * 4)(*[out[v].data_ptr() for v in range(4)]), out[4].data_ptr() if total else None,
                     torch.empty(ops.DOFP_WB_WS, dtype=torch.int64, device="cuda"), torch.empty(ops.DOFP_PARAMS, dtype=torch.int32, device="cuda")))
    st = torch.cuda.current_stream().cuda_stream
    pc, mc = ops.DOFP_PATTERNS[pattern], ops.DOFP_MODES[mode]

    def fn(i):
        src, _, dp, tp, ws, pout = sets[i % SETS]
        if what == "views":
            _lib.check(L.shm_dofp_views(src.data_ptr(), bits, H, W, W, pc, quad, mc, dp, tp, st), "shm_dofp_views")
            return
        p = params
        if what == "gray":
            _lib.check(L.shm_dofp_wb_gray(src.data_ptr(), bits, H, W, W, pc, params.data_ptr(), (1 << bits) - 1, pout.data_ptr(), ws.data_ptr(), st), "shm_dofp_wb_gray")
            p = pout
        _lib.check(L.shm_dofp_develop(src.data_ptr(), bits, H, W, W, pc, quad, mc, dp, tp, p.data_ptr(), lut.data_ptr(), mirror, st), "shm_dofp_develop")
    return fn, H * W * np.dtype(dt).itemsize + nplanes * ho * wo * 3 + (4096 if what != "views" else 0)


def calibrate_launcher(bits, tables, rng, what):
    """(fn that launches on set i, bytes per launch) for what = "calibrate", "copy" (one device-to-device copy that moves the same bytes:
    half of them read, half written) or "views" (the plain RGGB bilinear demosaic of the same frame).  tables: which of dark, gain, defect
    are given.  Every set has its own tables (0.1 % of the sites defective): the worst case -- a sensor's one calibration would stay in
    the Infinity Cache between frames."""
    L = _lib.lib()
    dt = np.uint8 if bits == 8 else np.uint16
    size = np.dtype(dt).itemsize
    nbytes = 2 * H * W * size + H * W * sum(b for b, use in zip((2, 2, 1), tables) if use)
    st = torch.cuda.current_stream().cuda_stream
    pc = ops.DOFP_PATTERNS["rggb"]
    quad = (C.c_int * 4)(*QUAD)
    ped = ((1 << bits) - 1) // 16
    sets = []
    for _ in range(SETS):
        src = torch.from_numpy(rng.integers(0, 1 << bits, (H, W)).astype(dt)).cuda()
        if what == "copy":
            sets.append((torch.empty(nbytes // 2, dtype=torch.uint8, device="cuda"), torch.empty(nbytes // 2, dtype=torch.uint8, device="cuda")))
        elif what == "views":
            out = torch.empty((4, H, W, 3), dtype=torch.uint8, device="cuda")
            sets.append((src, out, (C.c_void_p * 4)(*[out[v].data_ptr() for v in range(4)])))
        else:
            dark = torch.from_numpy(rng.integers(ped // 2, 2 * ped, (H, W)).astype(np.uint16)).cuda() if tables[0] else None
            gain = torch.from_numpy(rng.integers(3600, 4700, (H, W)).astype(np.uint16)).cuda() if tables[1] else None
            defect = torch.from_numpy((rng.random((H, W)) < 1e-3).astype(np.uint8)).cuda() if tables[2] else None
            sets.append((src, torch.empty_like(src), dark, gain, defect))
    ptr = lambda t: None if t is None else t.data_ptr()

    def fn(i):
        s = sets[i % SETS]
        if what == "copy":
            s[1].copy_(s[0], non_blocking=True)
        elif what == "views":
            _lib.check(L.shm_dofp_views(s[0].data_ptr(), bits, H, W, W, pc, quad, 0, s[2], None, st), "shm_dofp_views")
        else:
            _lib.check(L.shm_dofp_calibrate(s[0].data_ptr(), bits, H, W, W, pc, ptr(s[2]), ptr(s[3]), ptr(s[4]), ped, (1 << bits) - 1, s[1].data_ptr(), W, st),
                       "shm_dofp_calibrate")
    return fn, (H * W * size + 4 * H * W * 3 if what == "views" else nbytes)


MERGE_EXPOSURES = (1, 4, 16)


def merge_launcher(bits, counts, rng, what):
    """(fn that launches on set i, bytes per launch) for what = "merge", "copy" (one device-to-device copy that moves the same bytes: n
    pages read, one 16-bit page written) or "calibrate" (shm_dofp_calibrate of ONE page with the dark frame alone: the launch a bracketed
    layout with a calibration makes n times in front of the merge).  The pages are a radiance ramp through the three exposures, so that
    every number of valid pages occurs."""
    from shmgan_amd import polar
    L = _lib.lib()
    n = len(MERGE_EXPOSURES)
    dt = np.uint8 if bits == 8 else np.uint16
    size = np.dtype(dt).itemsize
    maxv = (1 << bits) - 1
    black, white = maxv // 16, maxv - maxv // 8
    nbytes = n * H * W * size + H * W * 2
    st = torch.cuda.current_stream().cuda_stream
    mul = polar.DofpBracket(MERGE_EXPOSURES).table(bits)
    table, mirror = torch.from_numpy(mul.copy()).cuda(), (C.c_uint * 256)(*[int(v) for v in mul])
    sets = []
    for _ in range(SETS):
        if what == "copy":
            sets.append((torch.empty(nbytes // 2, dtype=torch.uint8, device="cuda"), torch.empty(nbytes // 2, dtype=torch.uint8, device="cuda")))
            continue
        light = rng.random((H, W)) ** 2 * 1.3 * (white - black)
        pages = torch.from_numpy(np.stack([np.clip(black + light * e + rng.normal(0, 2, (H, W)), 0, maxv) for e in MERGE_EXPOSURES]).astype(dt)).cuda()
        if what == "calibrate":
            sets.append((pages[0], torch.empty_like(pages[0]), torch.from_numpy(rng.integers(black // 2, 2 * black, (H, W)).astype(np.uint16)).cuda()))
        else:
            sets.append((pages, (C.c_void_p * n)(*[pages[k].data_ptr() for k in range(n)]), torch.empty((H, W), dtype=torch.uint16, device="cuda"),
                         torch.empty(9, dtype=torch.int32, device="cuda") if counts else None))

    def fn(i):
        s = sets[i % SETS]
        if what == "copy":
            s[1].copy_(s[0], non_blocking=True)
        elif what == "calibrate":
            _lib.check(L.shm_dofp_calibrate(s[0].data_ptr(), bits, H, W, W, ops.DOFP_PATTERNS["rggb"], s[2].data_ptr(), None, None, black, white,
                                            s[1].data_ptr(), W, st), "shm_dofp_calibrate")
        else:
            _lib.check(L.shm_dofp_merge(s[1], n, bits, H, W, W, table.data_ptr(), mirror, black, white, s[2].data_ptr(), W,
                                        None if s[3] is None else s[3].data_ptr(), st), "shm_dofp_merge")
    return fn, (2 * H * W * size + 2 * H * W if what == "calibrate" else nbytes)


def timed(fn, launches, warm=2, n=5):
    """Median microseconds per launch over n timed iterations of `launches` launches (device events)."""
    us = []
    for it in range(warm + n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(launches):
            fn(i)
        e1.record()
        e1.synchronize()
        if it >= warm:
            us.append(e0.elapsed_time(e1) * 1e3 / launches)
    return float(np.median(us)), us


def decode_time(rng, n=3):
    """Host milliseconds PIL takes to decode the four 8-bit RGB view PNGs of one frame (the mosaic's own demosaiced views)."""
    from PIL import Image
    from shmgan_amd.polar import DofpLayout, demosaic
    views = [v.cpu().numpy() for v in demosaic(rng.integers(0, 256, (H, W)).astype(np.uint8), DofpLayout())]
    files = []
    for v in views:
        b = io.BytesIO()
        Image.fromarray(v).save(b, format="PNG", compress_level=1)
        files.append(b.getvalue())
    best = []
    for _ in range(n):
        t0 = time.perf_counter()
        for f in files:
            np.asarray(Image.open(io.BytesIO(f)).convert("RGB"))
        best.append((time.perf_counter() - t0) * 1e3)
    return min(best), sum(len(f) for f in files)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=1000)
    ap.add_argument("--no-decode", action="store_true")
    ap.add_argument("--no-develop", action="store_true")
    ap.add_argument("--no-views", action="store_true")
    ap.add_argument("--no-calibrate", action="store_true")
    ap.add_argument("--no-merge", action="store_true")
    a = ap.parse_args()
    rng = np.random.default_rng(0)
    print(f"shm_dofp_views, {W} x {H} frames, {SETS} buffer sets in rotation, {a.launches} launches per timed iteration")
    for name, pattern, bits, mode in ([] if a.no_views else CONFIGS):
        for total in (False, True):
            fn, nbytes = launcher(pattern, bits, mode, total, rng)
            us, all_us = timed(fn, a.launches)
            bw = nbytes / (us * 1e-6)
            print(f"  {name:22s} {'+ total' if total else '       '}: {us:8.2f} us  ({min(all_us):.2f} .. {max(all_us):.2f})  {nbytes / 1e6:7.2f} MB  "
                  f"{bw / 1e12:5.2f} TB/s = {100 * bw / HBM_PEAK:4.1f} % of the {HBM_PEAK / 1e12:.1f} TB/s peak, "
                  f"{100 * bw / HBM_COPY:4.1f} % of a copy's {HBM_COPY / 1e12:.2f} TB/s", flush=True)
    if not a.no_decode:
        ms, nb = decode_time(rng)
        print(f"  PIL decode of the four {W} x {H} RGB view PNGs one mosaic replaces: {ms:.1f} ms on the host ({nb / 1e6:.1f} MB of files; noise "
              f"images at compress_level 1)")
    if not a.no_develop:
        print(f"shm_dofp_develop beside shm_dofp_views, same frames and protocol (black 240 of 4095, sRGB table; \"gray\" = the two estimation launches + the development)")
        for name, pattern, bits, mode in DEVELOP_CONFIGS:
            for total in (False, True):
                row = {}
                for what in ("views", "develop") + (() if pattern == "mono" else ("matrix", "gray")):
                    fn, nbytes = develop_launcher(pattern, bits, mode, total, rng, what)
                    row[what] = timed(fn, a.launches)[0]
                    bw = nbytes / (row[what] * 1e-6)
                    print(f"  {name:22s} {'+ total' if total else '       '} {what:8s}: {row[what]:8.2f} us  {bw / 1e12:5.2f} TB/s = {100 * bw / HBM_PEAK:4.1f} % of peak"
                          f"   x{row[what] / row['views']:.2f} of the plain launch", flush=True)
    if not a.no_calibrate:
        print("shm_dofp_calibrate beside a device copy of the same bytes and the plain RGGB bilinear demosaic of the same frame (every set has its own tables)")
        for bits in (8, 12):
            for name, tables in (("dark + gain + defect", (True, True, True)), ("dark only", (True, False, False))):
                row = {}
                for what in ("calibrate", "copy", "views"):
                    fn, nbytes = calibrate_launcher(bits, tables, rng, what)
                    row[what] = timed(fn, a.launches)[0]
                    bw = nbytes / (row[what] * 1e-6)
                    print(f"  {bits:2d}-bit {name:22s} {what:9s}: {row[what]:8.2f} us  {nbytes / 1e6:7.2f} MB  {bw / 1e12:5.2f} TB/s = {100 * bw / HBM_PEAK:4.1f} % of peak", flush=True)
                print(f"  {bits:2d}-bit {name:22s} calibrate = x{row['calibrate'] / row['copy']:.2f} of the copy, x{row['calibrate'] / row['views']:.2f} of the demosaic launch", flush=True)
    if not a.no_merge:
        print(f"shm_dofp_merge of {len(MERGE_EXPOSURES)} pages (exposures {MERGE_EXPOSURES}) beside a device copy of the same bytes and the calibrate launch (dark frame alone) of one page")
        for bits in (8, 12):
            for counts in (False, True):
                row = {}
                for what in ("merge", "copy", "calibrate"):
                    fn, nbytes = merge_launcher(bits, counts, rng, what)
                    row[what] = timed(fn, a.launches)[0]
                    bw = nbytes / (row[what] * 1e-6)
                    print(f"  {bits:2d}-bit {'with counts' if counts else 'no counts  '} {what:9s}: {row[what]:8.2f} us  {nbytes / 1e6:7.2f} MB  {bw / 1e12:5.2f} TB/s = {100 * bw / HBM_PEAK:4.1f} % of peak", flush=True)
                print(f"  {bits:2d}-bit {'with counts' if counts else 'no counts  '} merge = x{row['merge'] / row['copy']:.2f} of the copy, x{row['merge'] / row['calibrate']:.2f} of one calibrate launch", flush=True)
