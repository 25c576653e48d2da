"""Native-resolution inference (evaluate.test(eval_size="native") = trainer.infer on a padded frame): ms per image for G1 alone
and for G1 plus the five cyclic passes, on one 1024 x 1536 image and one whose sides are no multiples of 16, in float32 and
bfloat16, and the per-kernel table of one G1 + cyclic run (ops.KernelTimer).  A record for kernel work, not an acceptance number.
python tools/bench_native.py [float32|bfloat16 ...]"""
import sys
import time
from pathlib import Path
sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import numpy as np
import torch
from shmgan_amd import ShmGANwithSSpecSeg, ops
from shmgan_amd.data import pad_geometry
from shmgan_amd.evaluate import check_native_limits

SIZES = [(1024, 1536), (1000, 1531)]
F = 64


def frame_of(h, w):
    u8 = torch.from_numpy(np.random.default_rng(h).integers(0, 256, (h, w, 3), dtype=np.uint8)).cuda()
    hp, wp, top, left = pad_geometry(h, w)
    x = torch.empty((1, hp, wp, 3), device="cuda")
    ops.load_pad_u8(u8, x[0], top, left)
    return x


def timed(fn, warm=2, n=5):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n


for dt in (sys.argv[1:] or ["float32", "bfloat16"]):
    m = ShmGANwithSSpecSeg(image_size=256, filter_size=F, batch_size=1, compute_dtype=dt).build()
    for h, w in SIZES:
        need = check_native_limits(f"{h}x{w}", h, w, F, m.compute_dtype, True, False, free_bytes=torch.cuda.mem_get_info()[0])
        x = frame_of(h, w)
        hp, wp = x.shape[1:3]
        g1 = timed(lambda: m.infer(x, cyclic=False))
        allp = timed(lambda: m.infer(x, cyclic=True))
        print(f"{dt} {h} x {w} (frame {hp} x {wp}, {need / 2**30:.2f} GiB counted, arena {m.arena.nbytes() / 2**30:.2f} GiB): G1 {g1 * 1e3:.2f} ms, "
              f"G1 + cyclic {allp * 1e3:.2f} ms per image; {g1 * 1e9 / (hp * wp):.2f} / {allp * 1e9 / (hp * wp):.2f} ns per frame pixel", flush=True)
        ops.TIMER = ops.KernelTimer()
        m.infer(x, cyclic=True)
        torch.cuda.synchronize()
        timer, ops.TIMER = ops.TIMER, None
        print(f"per-kernel table, {dt}, {h} x {w}, G1 + cyclic (launches, ms, TFLOP/s):")
        for sym, d in sorted(timer.summary().items(), key=lambda kv: -kv[1]["ms"]):
            print(f"  {sym:72s} {d['launches']:4d} {d['ms']:9.3f} {d['flops'] / max(d['ms'], 1e-9) / 1e9:8.1f}")
        for (sym, label), d in sorted(timer.per_shape().items(), key=lambda kv: -kv[1]["ms"])[:12]:
            print(f"    {label:40s} {sym:60s} {d['launches']:4d} {d['ms']:9.3f}")
    m.release()
