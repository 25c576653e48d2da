"""Batch preparation of the training loader (shmgan_amd.data.PolarDataset): one batch of B samples at S x S from a synthetic
capture of HxH PNG files, with the diffuse target read from the ED/ directory (diffuse_source="dir": 5 B decodes, 5 B uploads,
5 B shm_resize_bilinear_u8 launches) and computed on the device ("min": 4 B decodes, 4 B uploads, B shm_polar_views_u8 launches),
and the "dir" loader through the augmenting kernel (5 B uploads, B shm_augment_views_u8 launches): "dir/identity" with
Augment() -- identity parameters, the same numbers as "dir" -- and "dir/augment" with a random crop of at least half the area and
both mirrors at probability 0.5, another pass (so other draws) every repeat.  On a tree without data.Augment the last two are
left out, so the same tool gives the first figure on an older commit.  "dir/cached", "min/cached" and "dir/augment/cached" are "dir",
"min" and "dir/augment" with cache="device" (on a tree that has it): the capture holds exactly one batch, which the warm-up makes
resident, so every timed batch is built from the arena by shm_augment_batch_u8 launches alone (checked: resident == B, no refusal).

Three figures per configuration, the configurations alternating within every repeat, median over the repeats after a warm-up:
  device_ms   HIP events on the loader stream around the uploads and kernels alone: the decoded bytes are already in the pinned
              staging buffers (the decode is replaced by a lookup), so this is what the GPU side of a batch costs
  total_ms    host clock around prepare() -> the batch's event has completed, decode included (PIL, one worker thread)
  host_ms     wall time of the loader's worker (_prepare_worker) for the same batches: decode, staging, descriptors and enqueues --
              what the worker thread is busy for, which is what has to hide under a training step
Launches, uploads and decodes per batch are counted, not assumed (a shm_augment_batch_u8 call counts its cdiv(n, 8) launches).
Prints one JSON line per configuration.
python tools/bench_loader.py [--batch 8] [--size 256] [--source-size 1024] [--repeats 20] [--warmup 3]"""
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
from shmgan_amd import data, ops
from shmgan_amd.data import PSD_SUBDIRS, PolarDataset

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=8)
ap.add_argument("--size", type=int, default=256)
ap.add_argument("--source-size", type=int, default=1024)
ap.add_argument("--repeats", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--seed", type=int, default=0)
a = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("bench_loader needs a GPU: there is nothing to time without one")
B, S, H = a.batch, a.size, a.source_size

counts = {"launches": 0, "uploads": 0}


def counted(fn):
    def call(*args, **kw):
        counts["launches"] += 1
        return fn(*args, **kw)
    return call


ops.resize_bilinear_u8 = counted(ops.resize_bilinear_u8)
ops.polar_views_u8 = counted(ops.polar_views_u8)
Augment = getattr(data, "Augment", None)
if Augment is not None:
    ops.augment_views_u8 = counted(ops.augment_views_u8)
CACHED = hasattr(ops, "augment_batch_u8")
if CACHED:
    def batch_counted(fn):
        def call(samples, *args, **kw):
            counts["launches"] += -(-len(samples) // ops.AUG_GROUP)
            return fn(samples, *args, **kw)
        return call
    ops.augment_batch_u8 = batch_counted(ops.augment_batch_u8)

with tempfile.TemporaryDirectory() as root:
    from PIL import Image
    rng = np.random.default_rng(a.seed)
    for sub in PSD_SUBDIRS:
        (Path(root) / sub).mkdir()
        for i in range(B):
            Image.fromarray(rng.integers(0, 256, (H, H, 3)).astype(np.uint8)).save(Path(root) / sub / f"img_{i:03d}.png", compress_level=1)
    sets = {src: PolarDataset(root, S, batch_size=B, diffuse_source=src, rank=0, world=1) for src in ("dir", "min")}
    if Augment is not None:
        sets["dir/identity"] = PolarDataset(root, S, batch_size=B, rank=0, world=1, augment=Augment())
        sets["dir/augment"] = PolarDataset(root, S, batch_size=B, rank=0, world=1, seed=a.seed,
                                           augment=Augment(flip_lr=0.5, flip_ud=0.5, crop_min=0.5))
    if CACHED:
        sets["dir/cached"] = PolarDataset(root, S, batch_size=B, rank=0, world=1, cache="device")
        sets["min/cached"] = PolarDataset(root, S, batch_size=B, diffuse_source="min", rank=0, world=1, cache="device")
        sets["dir/augment/cached"] = PolarDataset(root, S, batch_size=B, rank=0, world=1, seed=a.seed, cache="device",
                                                  augment=Augment(flip_lr=0.5, flip_ud=0.5, crop_min=0.5))
        if a.warmup < 1:
            sys.exit("the cached configurations are timed on resident samples: --warmup must be at least 1")
    passes = {src: 0 for src in sets}
    host, decodes = {src: [] for src in sets}, {src: 0 for src in sets}
    for src, ds in sets.items():
        def timed_worker(*args, src=src, fn=ds._prepare_worker, **kw):
            t0 = time.perf_counter()
            try:
                return fn(*args, **kw)
            finally:
                host[src].append((time.perf_counter() - t0) * 1e3)

        def counted_decode(path, key, src=src, fn=ds._decode):
            decodes[src] += 1
            return fn(path, key)
        ds._prepare_worker, ds._decode = timed_worker, counted_decode

    def prepare(src, ds):
        """Batch 0; the augmenting configurations take the next pass each time (the identity one draws nothing either way)."""
        if ds.__dict__.get("augment") is None:
            return ds.prepare(0)
        passes[src] += 1
        return ds.prepare(0, passes[src])

    def run(src, ds):
        """One batch through the loader's own worker; (host seconds until the batch's event completed, its tensors)."""
        t0 = time.perf_counter()
        outs, ev = prepare(src, ds).result()
        ev.synchronize()
        return time.perf_counter() - t0, outs

    total = {src: [] for src in sets}
    for r in range(a.warmup + a.repeats):
        if r == a.warmup:
            for src, ds in sets.items():
                host[src].clear()
                decodes[src] = 0
                if src.endswith("/cached"):
                    st = ds.cache_stats()
                    assert st["resident"] == B and st["refused"] == 0, (src, st)
        for src, ds in sets.items():
            dt, _ = run(src, ds)
            if r >= a.warmup:
                total[src].append(dt * 1e3)
    host = {src: sorted(v) for src, v in host.items()}             # the timed batches only
    decodes = {src: n // a.repeats for src, n in decodes.items()}

    # the GPU side alone: both staging generations are filled by now, so the decode becomes a lookup (the upload still reads the pinned buffer)
    device, per_batch = {src: [] for src in sets}, {}
    for src, ds in sets.items():
        def staged(path, key, ds=ds):
            counts["uploads"] += 1
            return ds._pin[key]
        ds._decode = staged
        del ds._prepare_worker                                     # the class's own again: the pass below is not host-timed
    for r in range(a.warmup + a.repeats):
        for src, ds in sets.items():
            counts["launches"] = counts["uploads"] = 0
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(ds.stream)
            prepare(src, ds).result()
            e1.record(ds.stream)
            e1.synchronize()
            per_batch[src] = dict(counts)
            if r >= a.warmup:
                device[src].append(e0.elapsed_time(e1))
    for src in sets:
        d, t, h = sorted(device[src]), sorted(total[src]), host[src]
        print(json.dumps({"tool": "bench_loader", "diffuse_source": src.split("/")[0], "config": src, "B": B, "S": S, "source": f"{H}x{H}",
                          "launches": per_batch[src]["launches"], "uploads": per_batch[src]["uploads"], "decodes": decodes[src],
                          "device_ms": round(statistics.median(d), 4), "device_ms_min_max": [round(d[0], 4), round(d[-1], 4)],
                          "total_ms": round(statistics.median(t), 3), "total_ms_min_max": [round(t[0], 3), round(t[-1], 3)],
                          "host_ms": round(statistics.median(h), 3), "host_ms_min_max": [round(h[0], 3), round(h[-1], 3)],
                          "repeats": a.repeats}), flush=True)
