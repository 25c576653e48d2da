"""The averaged generator weights: (1) shm_ema_update beside shm_adam_clip on the generator's own flat buffers at F = 64
(n = G.P.n floats each): one HIP-event pair per launch, the two kernels taking turns, the median over --repeats launches after a
warm-up, and the algorithmic GB/s (12 bytes per element for the average, 28 for clip + Adam); the 4-byte-lane form of the average
(buffers one element apart in alignment) is timed the same way; (2) the S = 256, B = 8 train_step in float32 and bfloat16 with
ema_decay 0 and 0.999 on one trainer, in alternating blocks of --block steps.  One JSON line per row.
python tools/bench_ema.py [--repeats N] [--warmup W] [--blocks K] [--block STEPS] [--no-step] [--size S] [--batch B]"""
import argparse
import json
import sys
from pathlib import Path
sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import numpy as np
import torch
from shmgan_amd import ShmGANwithSSpecSeg, ops

ap = argparse.ArgumentParser()
ap.add_argument("--repeats", type=int, default=200)
ap.add_argument("--warmup", type=int, default=20)
ap.add_argument("--blocks", type=int, default=3, help="alternating off / on blocks per dtype")
ap.add_argument("--block", type=int, default=20, help="steps per block")
ap.add_argument("--no-step", action="store_true")
ap.add_argument("--size", type=int, default=256)
ap.add_argument("--batch", type=int, default=8)
a = ap.parse_args()


def interleaved_us(fns, repeats, warmup):
    """Per-launch times of several launches taking turns: {name: sorted list of us}."""
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    evs = {k: [] for k in fns}
    for _ in range(repeats):
        for k, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            evs[k].append((e0, e1))
    torch.cuda.synchronize()
    return {k: sorted(e0.elapsed_time(e1) * 1e3 for e0, e1 in v) for k, v in evs.items()}


def row(us, nbytes):
    med = us[len(us) // 2]
    return {"median_us": round(med, 2), "p10_us": round(us[len(us) // 10], 2), "p90_us": round(us[(9 * len(us)) // 10], 2),
            "GB_s": round(nbytes / med / 1e3, 1)}


m = ShmGANwithSSpecSeg(image_size=a.size, filter_size=64, batch_size=a.batch).build()
P = m.G.P
n = P.n
rng = np.random.default_rng(0)
P.grad.copy_(torch.from_numpy((rng.standard_normal(n) * 1e-3).astype(np.float32)))
ema = torch.empty_like(P.flat)
ops.ema_update(ema, P.flat, n, 0.0)
spare = torch.empty(n + 4, device="cuda")                   # spare[1:] is 4 bytes off the 16-byte alignment of P.flat: the 4-byte-lane form
ops.ema_update(spare[1:n + 1], P.flat, n, 0.0)
us = interleaved_us({"ema": lambda: ops.ema_update(ema, P.flat, n, 0.999),
                     "adam": lambda: ops.adam_clip(P.flat, P.m, P.v, P.grad, n, 1e-9, 0.5, 0.99, 1e-7, 1.0),
                     "ema_scalar": lambda: ops.ema_update(spare[1:n + 1], P.flat, n, 0.999),
                     "ema_copy": lambda: ops.ema_update(ema, P.flat, n, 0.0)}, a.repeats, a.warmup)
out = {"tool": "bench_ema", "F": 64, "n": n, "repeats": a.repeats, "ema_update": row(us["ema"], 12.0 * n), "adam_clip": row(us["adam"], 28.0 * n),
       "ema_update_4B_lanes": row(us["ema_scalar"], 12.0 * n), "ema_update_decay0": row(us["ema_copy"], 8.0 * n)}
out["ema_GB_s_over_adam_GB_s"] = round(out["ema_update"]["GB_s"] / out["adam_clip"]["GB_s"], 3)
print(json.dumps(out), flush=True)
m.release()
del ema, spare, P

if not a.no_step:
    S, B = a.size, a.batch
    inp = [torch.from_numpy(rng.random((B, S, S, 3), dtype=np.float32)).cuda() for _ in range(5)]
    for dt in ("float32", "bfloat16"):
        m = ShmGANwithSSpecSeg(image_size=S, filter_size=64, batch_size=B, compute_dtype=dt).build()
        for decay in (0.999, 0.0):                          # warm both forms up
            m.args.ema_decay = decay
            for _ in range(3):
                m.train_step(*inp)
        torch.cuda.synchronize()
        res = {0.0: [], 0.999: []}
        for blk in range(2 * a.blocks):
            m.args.ema_decay = decay = 0.0 if blk % 2 == 0 else 0.999
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.block):
                m.train_step(*inp)
            e1.record()
            torch.cuda.synchronize()
            res[decay].append(e0.elapsed_time(e1) / a.block)
        off, on = np.array(res[0.0]), np.array(res[0.999])
        print(json.dumps({"tool": "bench_ema", "step": f"{dt} S={S} B={B}", "blocks": a.blocks, "steps_per_block": a.block,
                          "off_ms": [round(v, 3) for v in off], "on_ms": [round(v, 3) for v in on],
                          "off_median_ms": round(float(np.median(off)), 3), "on_median_ms": round(float(np.median(on)), 3),
                          "on_minus_off_ms": round(float(np.median(on) - np.median(off)), 3),
                          "off_spread_ms": round(float(off.max() - off.min()), 3)}), flush=True)
        m.release()
