"""Test-mode throughput (the reference's test.py with --calc_metrics True = trainer.evaluate): infer (six generator forwards) plus
the three image-metric kernels, at S = 256, F = 64, float32 and bfloat16, B = 1 and B = 8, on synthetic images from a seed.
Prints one JSON line per configuration: evaluation batch time, images/s, and the metric kernels alone (HIP events), also as a
share of the batch.  python tools/bench_eval.py [--steps N] [--warmup W] [--dtypes float32,bfloat16] [--batches 1,8]"""
import argparse
import json
import sys
import time
from pathlib import Path
sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import numpy as np
import torch
from shmgan_amd import ShmGANwithSSpecSeg, ops

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=10)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--size", type=int, default=256)
ap.add_argument("--filters", type=int, default=64)
ap.add_argument("--dtypes", default="float32,bfloat16")
ap.add_argument("--batches", default="1,8")
ap.add_argument("--seed", type=int, default=0)
a = ap.parse_args()
S = a.size
for dt in a.dtypes.split(","):
    for B in (int(b) for b in a.batches.split(",")):
        rng = np.random.default_rng(a.seed)
        rgb = torch.from_numpy(rng.random((B, S, S, 3), dtype=np.float32)).cuda()
        dif = torch.from_numpy(rng.random((B, S, S, 3), dtype=np.float32)).cuda()
        m = ShmGANwithSSpecSeg(image_size=S, filter_size=a.filters, batch_size=B, compute_dtype=dt).build()
        for _ in range(a.warmup):
            m.evaluate(rgb, dif)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.steps):
            _, _, met = m.evaluate(rgb, dif)
        torch.cuda.synchronize()
        batch_s = (time.perf_counter() - t0) / a.steps
        # the metric kernels alone, on the last generated images
        gen = m.gen_rgb
        out = torch.empty((B, 5), dtype=torch.float64, device="cuda")
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ops.image_metrics(gen, dif, out)
        e0.record()
        for _ in range(a.steps):
            ops.image_metrics(gen, dif, out)
        e1.record()
        torch.cuda.synchronize()
        metrics_ms = e0.elapsed_time(e1) / a.steps
        assert torch.isfinite(met).all()
        print(json.dumps({"tool": "bench_eval", "dtype": dt, "S": S, "F": a.filters, "B": B, "batch_ms": round(batch_s * 1e3, 3),
                          "images_per_s": round(B / batch_s, 2), "metrics_ms": round(metrics_ms, 4),
                          "metrics_share": round(metrics_ms / (batch_s * 1e3), 5)}), flush=True)
        m.release()
        del m
        torch.cuda.empty_cache()
