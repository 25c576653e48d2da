"""Specular masks from the polarised views (shmgan_amd.polar.specular_mask, csrc/specmask.hip): what one sample costs on the device,
and what the directory writer costs per file, on a synthetic HxH capture (smooth background, a few polarised highlight blobs, sensor
noise; PSD angles).

Device figures, HIP events on the current stream, median [min, max] over the repeats after a warm-up; every stage is timed as K calls
back to back between one pair of events, divided by K (so the launch gaps of a real chain are in, the enqueue of the first call is not):
  chain_us      shm_specmask: strength + histogram, Otsu, threshold + erosion, dilation + count (4 launches, 2 small clears)
  strength_us   shm_specmask_strength alone, and its achieved bytes/s from the bytes the algorithm needs: 12 read + 1 written per pixel
  otsu_us       shm_specmask_otsu alone (one block)
  morph_us      shm_specmask_morph alone (2 launches, 1 clear)
  single_us     one chain call between its own pair of events, as a caller that does nothing else sees it (enqueue included)
Writer figures, host clock, per sample: write_specular_masks end to end over --files samples (compress_level of the inputs is 1), and
apart from it the PIL decode of a sample's four views and the PNG encode of its mask.
Prints one JSON line per group.
python tools/bench_specmask.py [--size 1024] [--repeats 30] [--warmup 5] [--calls 20] [--files 4]"""
import argparse
import json
import statistics
import sys
import tempfile
import time
from pathlib import Path
sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import numpy as np
import torch
from shmgan_amd import ops, polar

ap = argparse.ArgumentParser()
ap.add_argument("--size", type=int, default=1024)
ap.add_argument("--repeats", type=int, default=30)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--calls", type=int, default=20)
ap.add_argument("--files", type=int, default=4)
ap.add_argument("--seed", type=int, default=0)
a = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("bench_specmask needs a GPU: there is nothing to time without one")
H = a.size
ANGLES = [0.0, 60.0, 90.0, 150.0]
SUBDIRS = ("I0", "I60", "I90", "I150")


def capture_sample(rng):
    """Four uint8 [H,H,3] views: 0.5 * base + spec * cos^2(theta - phi) + N(0, 3)."""
    yy, xx = np.mgrid[0:H, 0:H].astype(np.float32)
    base = np.stack([100.0 + 10 * c + 25.0 * np.cos(rng.uniform(0.005, 0.03) * yy + rng.uniform(0.005, 0.03) * xx + rng.uniform(0, 6.28))
                     for c in range(3)], axis=-1)
    spec = np.zeros((4, H, H), dtype=np.float32)
    for _ in range(8):
        r = rng.uniform(0.01, 0.04) * H
        cy, cx, phi = rng.uniform(0, H), rng.uniform(0, H), rng.uniform(0, np.pi)
        g = 150.0 * np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2.0 * (0.5 * r) ** 2))
        for k, th in enumerate(ANGLES):
            spec[k] += g * np.cos(np.deg2rad(th) - phi) ** 2
    return [np.clip(np.rint(0.5 * base + spec[k][..., None] + rng.normal(0.0, 3.0, (H, H, 3))), 0, 255).astype(np.uint8) for k in range(4)]


def med(v):
    v = sorted(v)
    return round(statistics.median(v), 3), [round(v[0], 3), round(v[-1], 3)]


rng = np.random.default_rng(a.seed)
views = capture_sample(rng)
srcs = [torch.from_numpy(v).cuda() for v in views]
coef = polar.stokes_matrix(ANGLES)
q, tmp, mask = (torch.empty((H, H), dtype=torch.uint8, device="cuda") for _ in range(3))
hist = torch.empty(256, dtype=torch.int32, device="cuda")
stats = torch.empty(3, dtype=torch.int32, device="cuda")
stages = {
    "chain": lambda: ops.specmask(srcs, coef, q, hist, tmp, mask, stats),
    "strength": lambda: ops.specmask_strength(srcs, coef, q, hist),
    "otsu": lambda: ops.specmask_otsu(hist, stats),
    "morph": lambda: ops.specmask_morph(q, stats, tmp, mask),
}
times = {k: [] for k in stages}
single = []
for r in range(a.warmup + a.repeats):
    for name, fn in stages.items():                     # the stages alternate within every repeat
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.calls):
            fn()
        e1.record()
        e1.synchronize()
        if r >= a.warmup:
            times[name].append(e0.elapsed_time(e1) * 1e3 / a.calls)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    stages["chain"]()
    e1.record()
    e1.synchronize()
    if r >= a.warmup:
        single.append(e0.elapsed_time(e1) * 1e3)
st = stats.cpu().tolist()
out = {"tool": "bench_specmask", "what": "device", "size": f"{H}x{H}", "calls_per_window": a.calls, "repeats": a.repeats,
       "t": st[0], "t_eff": st[1], "masked_fraction": round(st[2] / (H * H), 4)}
for name in stages:
    out[f"{name}_us"], out[f"{name}_us_min_max"] = med(times[name])
out["single_us"], out["single_us_min_max"] = med(single)
out["strength_bytes"] = 13 * H * H
out["strength_GBps"] = round(13 * H * H / (out["strength_us"] * 1e-6) / 1e9, 1)
print(json.dumps(out), flush=True)

with tempfile.TemporaryDirectory() as root:
    from PIL import Image
    root = Path(root)
    for i in range(a.files):
        vs = views if i == 0 else capture_sample(rng)
        for sub, v in zip(SUBDIRS, vs):
            (root / sub).mkdir(exist_ok=True)
            Image.fromarray(v).save(root / sub / f"img_{i:03d}.png", compress_level=1)
    e2e, dec, enc = [], [], []
    for r in range(1 + 3):                              # one warm-up pass, three timed
        t0 = time.perf_counter()
        written = polar.write_specular_masks(str(root), str(root / "masks"))
        dt = (time.perf_counter() - t0) * 1e3 / a.files
        t0 = time.perf_counter()
        for sub in SUBDIRS:
            polar._decode(str(root / sub / "img_000.png"))
        d = (time.perf_counter() - t0) * 1e3
        m = np.asarray(Image.open(written[0]))
        t0 = time.perf_counter()
        Image.fromarray(m).save(root / "encode_probe.png")
        e = (time.perf_counter() - t0) * 1e3
        if r >= 1:
            e2e.append(dt)
            dec.append(d)
            enc.append(e)
    w = {"tool": "bench_specmask", "what": "write_specular_masks", "size": f"{H}x{H}", "files": a.files, "passes": 3}
    w["per_sample_ms"], w["per_sample_ms_min_max"] = med(e2e)
    w["decode_4_views_ms"], w["decode_4_views_ms_min_max"] = med(dec)
    w["encode_mask_ms"], w["encode_mask_ms_min_max"] = med(enc)
    w["rest_ms"] = round(w["per_sample_ms"] - w["decode_4_views_ms"] - w["encode_mask_ms"], 3)
    print(json.dumps(w), flush=True)
