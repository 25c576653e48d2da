"""Guided detail transfer: shm_detail_coeffs (batch 1, radius 2 and 8) and shm_detail_apply_u8 at frame 256 x 256 -> photo 1024 x 1024 and
-> 3000 x 4000, beside the bilinear export_u8 of the model-size gen_rgb plane to the same photo size (what test mode does without
image_detail).  HIP events around `--iters` back-to-back calls after `--warmup`, repeated `--repeats` times (the spread is printed).  The
apply kernel is reported against its byte roof: 3 bytes read and 12 written per photo pixel over the achievable HBM bandwidth (6.3 TB/s
of the 8 TB/s peak); the coefficients (512 KiB) stay in cache.  One JSON line per shape.
python tools/bench_detail.py [--iters N] [--warmup W] [--repeats R]"""
import argparse
import json
import sys
from pathlib import Path
sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import numpy as np
import torch
from shmgan_amd import ops

HBM_ACHIEVABLE_TB_S, HBM_PEAK_TB_S = 6.3, 8.0

ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=200)
ap.add_argument("--warmup", type=int, default=20)
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--frame", type=int, default=256)
a = ap.parse_args()


def timed(fn):
    """us per call: the median over the repeats, and their (min, max)."""
    for _ in range(a.warmup):
        fn()
    us = []
    for _ in range(a.repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        us.append(e0.elapsed_time(e1) * 1e3 / a.iters)
    return float(np.median(us)), (round(min(us), 2), round(max(us), 2))


rng = np.random.default_rng(0)
S = a.frame
yuv = torch.from_numpy(rng.normal(2.0, 0.8, (1, S, S, 3)).astype(np.float32)).cuda()
gen_y = (yuv[..., :1] + torch.from_numpy(rng.normal(0.0, 0.5, (1, S, S, 1)).astype(np.float32)).cuda()).contiguous()
gen_rgb = torch.from_numpy(rng.random((S, S, 3), dtype=np.float32)).cuda()
scale = torch.tensor([0.23], dtype=torch.float32, device="cuda")
coef = torch.empty((1, S, S, 2), dtype=torch.float32, device="cuda")
coeffs = {}
for r in (0, 2, 8):
    us, spread = timed(lambda: ops.detail_coeffs(yuv[..., 0], gen_y, r, 1e-2, out=coef))
    coeffs[f"r{r}"] = {"us": round(us, 2), "min_max_us": spread}
ops.detail_coeffs(yuv[..., 0], gen_y, 2, 1e-2, out=coef)
print(json.dumps({"tool": "bench_detail", "kernel": "detail_coeffs", "frame": [S, S], "batch": 1, **coeffs}), flush=True)

for h, w in ((1024, 1024), (3000, 4000)):
    photo = torch.from_numpy(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)).cuda()
    out = torch.empty((h, w, 3), dtype=torch.float32, device="cuda")
    us_apply, sp_apply = timed(lambda: ops.detail_apply_u8(photo, coef[0], scale, out=out))
    buf = torch.empty(ops.export_layout([(h, w)], [3])[1], dtype=torch.uint8, device="cuda")
    us_export, sp_export = timed(lambda: ops.export_u8([gen_rgb], [(h, w)], ["rescale"], out=buf))
    us_export_full, sp_full = timed(lambda: ops.export_u8_hw([out], [(0, 0, h, w)], [(h, w)], ["rescale"], out=buf))
    nbytes = 15.0 * h * w
    roof_us = nbytes / (HBM_ACHIEVABLE_TB_S * 1e6)
    print(json.dumps({"tool": "bench_detail", "kernel": "detail_apply_u8", "frame": [S, S], "photo": [h, w],
                      "apply_us": round(us_apply, 2), "apply_min_max_us": sp_apply, "bytes": int(nbytes), "apply_TB_s": round(nbytes / us_apply / 1e6, 3),
                      "roof_us_at_6.3_TB_s": round(roof_us, 2), "share_of_achievable": round(roof_us / us_apply, 3),
                      "share_of_peak_8_TB_s": round(nbytes / (HBM_PEAK_TB_S * 1e6) / us_apply, 3),
                      "bilinear_export_u8_us": round(us_export, 2), "bilinear_export_min_max_us": sp_export,
                      "export_of_refined_plane_us": round(us_export_full, 2), "export_of_refined_min_max_us": sp_full}), flush=True)
    del photo, out, buf
