"""Training telemetry: (1) shm_tensor_stats on the real G and D segment tables at F = 64 beside shm_adam_clip on the same buffers
(us per call and algorithmic GB/s: 4 bytes per element read against 28 moved), on gradient-like data (exponents clustered as a
normal distribution's) and on exponents spread over 2^-45 .. 2^2 (a round of the bin count per distinct bin in a wave: the worst
case); (2) an S = 256, B = 8 fp32 train_step with telemetry off and with the reference's intervals (loss_log_step 25,
histogram_step 100) in the same process, in alternating blocks of 100 steps.  HIP events; one JSON line per row.
python tools/bench_telemetry.py [--steps N] [--warmup W] [--blocks K] [--no-step] [--dtype float32]"""
import argparse
import json
import sys
import tempfile
from pathlib import Path
sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import numpy as np
import torch
from shmgan_amd import ops
from shmgan_amd import telemetry as tel

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=50)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--blocks", type=int, default=3, help="alternating off / on blocks of 100 steps each")
ap.add_argument("--no-step", action="store_true")
ap.add_argument("--dtype", default="float32")
ap.add_argument("--size", type=int, default=256)
ap.add_argument("--batch", type=int, default=8)
a = ap.parse_args()


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / steps


from shmgan_amd import ShmGANwithSSpecSeg
m = ShmGANwithSSpecSeg(image_size=a.size, filter_size=64, batch_size=a.batch, compute_dtype=a.dtype).build()
rng = np.random.default_rng(0)
for tag, M in (("G", m.G), ("D", m.D)):
    tab = tel.variable_table(M, tag)
    seg = ops.SegmentTable([o for _, o, _, _ in tab], [z for _, _, z, _ in tab])
    n = M.P.n
    w, mm, vv = (torch.zeros(n, device="cuda") for _ in range(3))
    for data in ("normal", "spread"):
        if data == "normal":
            g = (rng.standard_normal(n) * 1e-3).astype(np.float32)
        else:
            g = (np.exp2(rng.uniform(-45.0, 2.0, n)) * rng.choice([-1.0, 1.0], n)).astype(np.float32)
        gd = torch.from_numpy(g).cuda()
        out = ops.tensor_stats(gd, seg)
        us_s = timed(lambda: ops.tensor_stats(gd, seg, out=out), a.steps, a.warmup)
        us_a = timed(lambda: ops.adam_clip(w, mm, vv, gd, n, 1e-5, 0.5, 0.99, 1e-7, 1.0), a.steps, a.warmup)
        print(json.dumps({"tool": "bench_telemetry", "model": tag, "F": 64, "data": data, "n": n, "segments": seg.n,
                          "tensor_stats_us": round(us_s, 1), "tensor_stats_GB_s": round(4.0 * n / us_s / 1e3, 1),
                          "adam_clip_us": round(us_a, 1), "adam_clip_GB_s": round(28.0 * n / us_a / 1e3, 1),
                          "stats_over_adam": round(us_s / us_a, 3)}), flush=True)
    del w, mm, vv

if not a.no_step:
    S, B = a.size, a.batch
    inp = [torch.from_numpy(rng.random((B, S, S, 3), dtype=np.float32)).cuda() for _ in range(5)]
    for _ in range(a.warmup):
        m.train_step(*inp)
    torch.cuda.synchronize()
    res = {"off": [], "on": []}
    with tempfile.TemporaryDirectory() as logs:
        for blk in range(2 * a.blocks):
            mode = "off" if blk % 2 == 0 else "on"
            if mode == "on":
                m.start_telemetry(log_dir=logs, loss_log_step=25, histogram_step=100)
            res[mode].append(timed(lambda: m.train_step(*inp), 100, 0) / 1e3)
            if mode == "on":
                m.stop_telemetry()
        lines = {k: len(v) for k, v in tel.read_log(logs).items()}
    off, on = np.array(res["off"]), np.array(res["on"])
    print(json.dumps({"tool": "bench_telemetry", "step": f"{a.dtype} S={S} B={B}", "blocks_of_100_steps": a.blocks,
                      "off_ms": [round(v, 3) for v in off], "on_ms": [round(v, 3) for v in on],
                      "off_mean_ms": round(float(off.mean()), 3), "on_mean_ms": round(float(on.mean()), 3),
                      "off_spread_ms": round(float(off.max() - off.min()), 3), "on_spread_ms": round(float(on.max() - on.min()), 3),
                      "log_lines": lines}), flush=True)
m.release()
