"""Test-mode image export (shm_export_u8, the per-batch call of evaluate.test with save_images="all"): B images x the 8 planes of
evaluate.IMAGE_TAGS (six RGB, G1 Y, mask) at S = 256, rescale_01 on the generated planes and the clip on the mask, as test mode
does by default.  Two output sizes: "model" (S x S, no resampling) and a 1224 x 1024 source photo.  Timed with HIP events;
prints one JSON line per size with us per call and the algorithmic GB/s (the source floats read once plus the bytes written).
python tools/bench_export.py [--steps N] [--warmup W] [--batch 8] [--size 256]"""
import argparse
import json
import sys
from pathlib import Path
sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import numpy as np
import torch
from shmgan_amd import ops
from shmgan_amd.evaluate import IMAGE_TAGS

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=50)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--batch", type=int, default=8)
ap.add_argument("--size", type=int, default=256)
ap.add_argument("--seed", type=int, default=0)
a = ap.parse_args()
B, S = a.batch, a.size
rng = np.random.default_rng(a.seed)
rgb = torch.from_numpy(rng.uniform(-0.5, 1.5, (6 * B, S, S, 3)).astype(np.float32)).cuda()   # G1 + five cyclic, per image
y = torch.from_numpy(rng.uniform(-0.5, 1.5, (B, S, S, 1)).astype(np.float32)).cuda()
mask = torch.from_numpy(rng.uniform(0.0, 1.0, (B, S, S, 1)).astype(np.float32)).cuda()
planes, modes = [], []
for b in range(B):
    for tag in IMAGE_TAGS:
        if tag == "G1_Y":
            planes.append(y[b])
        elif tag == "mask":
            planes.append(mask[b])
        else:
            planes.append(rgb[(0 if tag == "G1" else IMAGE_TAGS.index(tag) - 1) * B + b])
        modes.append("clip" if tag == "mask" else "rescale")
for name, (ho, wo) in (("model", (S, S)), ("source_1224x1024", (1024, 1224))):
    sizes = [(ho, wo)] * len(planes)
    chans = [int(p.shape[2]) for p in planes]
    _, total = ops.export_layout(sizes, chans)
    out = torch.empty(total, dtype=torch.uint8, device="cuda")
    for _ in range(a.warmup):
        ops.export_u8(planes, sizes, modes, None, out)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(a.steps):
        ops.export_u8(planes, sizes, modes, None, out)
    e1.record()
    torch.cuda.synchronize()
    us = e0.elapsed_time(e1) * 1e3 / a.steps
    nbytes = sum(S * S * c * 4 + ho * wo * c for c in chans)
    print(json.dumps({"tool": "bench_export", "B": B, "S": S, "planes": len(planes), "out": name, "ho": ho, "wo": wo,
                      "us": round(us, 2), "bytes": nbytes, "GB_s": round(nbytes / (us * 1e-6) / 1e9, 1)}), flush=True)
