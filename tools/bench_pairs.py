"""The mask network's pair loader (shmgan_amd.data.MaskDataset with augment / shuffle): what a batch of B pairs at S x S from HxH
sources costs on the device, and what an epoch of SpecSeg.fit costs with and without it.

  pairs_call      ONE ops.augment_pairs_u8 call on B resident pairs (two launches per 8 samples), every sample with its own random
                  crop of at least half the area and both mirrors at probability 0.5, other draws every call
  pairs_identity  the same call at identity parameters (what a shuffle alone asks for)
  replaced        what that call replaces per batch: per sample shm_resize_bilinear_u8 of the image and of the mask (2 B launches),
                  then one shm_rgb2yuv_std over the batch (a memset and two launches) and the copy of the Y channel -- today's
                  MaskDataset.tensors() arithmetic, on the same resident bytes
ms: HIP events around `--inner` back-to-back batches on the current stream, divided by it; host_ms: the host clock around the same
enqueues (descriptors, ctypes, launches) alone.  Where the two agree the stream ran dry between calls and the figure is the host's
launch rate, not kernel time (kernel time alone: rocprofv3 --kernel-trace --stats on this tool, in a run of its own).  The three
alternate within every repeat; median (and min, max) over the repeats after a warm-up.  Launches are counted per batch.

  fit_epoch       host clock around one SpecSeg.fit epoch, ending in a device synchronise, on `--pairs` pairs: "tensors" = fit(x, y) on
                  the tensors loaded once (today's path; the load is not in the figure), "dataset" = fit(dataset) with augmentation and
                  shuffle, pairs resident after the warm-up epoch (cache_stats is checked), another pass every epoch
Prints one JSON line per figure.
python tools/bench_pairs.py [--batch 8] [--size 256] [--source-size 1024] [--pairs 32] [--repeats 20] [--inner 20] [--epochs 5]"""
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
from shmgan_amd import ops
from shmgan_amd.cache import AugSample
from shmgan_amd.data import Augment, MaskDataset, augment_params

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=8)
ap.add_argument("--size", type=int, default=256)
ap.add_argument("--source-size", type=int, default=1024)
ap.add_argument("--pairs", type=int, default=32)
ap.add_argument("--repeats", type=int, default=20)
ap.add_argument("--inner", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--epochs", type=int, default=5)
ap.add_argument("--seed", type=int, default=0)
a = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("bench_pairs needs a GPU: there is nothing to time without one")
B, S, H = a.batch, a.size, a.source_size
dev = torch.device("cuda")
rng = np.random.default_rng(a.seed)
aug = Augment(flip_lr=0.5, flip_ud=0.5, crop_min=0.5)


def report(what, ms, **more):
    ms = sorted(ms)
    print(json.dumps({"tool": "bench_pairs", "what": what, "B": B, "S": S, "source": f"{H}x{H}", "ms": round(statistics.median(ms), 4),
                      "ms_min_max": [round(ms[0], 4), round(ms[-1], 4)], **more}), flush=True)


# ---- the call and what it replaces, on resident bytes
imgs = [torch.from_numpy(rng.integers(0, 256, (H, H, 3)).astype(np.uint8)).to(dev) for _ in range(B)]
masks = [torch.from_numpy((rng.random((H, H)) < 0.2).astype(np.uint8) * 255).to(dev) for _ in range(B)]
x, y = torch.empty((B, S, S, 1), device=dev), torch.empty((B, S, S, 1), device=dev)
ws = torch.empty(ops.augment_pairs_ws_doubles(B, S, S), dtype=torch.float64, device=dev)
rgb, yuv = torch.empty((B, S, S, 3), device=dev), torch.empty((B, S, S, 3), device=dev)
acc, scale = torch.zeros(2 * B, dtype=torch.float64, device=dev), torch.empty(B, device=dev)
# the draws are made before the timed window (numpy's generator costs more host time than the call's two launches take on the device)
drawn = []
for k in range(a.inner):
    ps = [augment_params(a.seed, k, b, H, H, aug) for b in range(B)]
    drawn.append([AugSample((imgs[b], masks[b]), H, H, p.crop, p.flip_ud, p.flip_lr) for b, p in enumerate(ps)])
turn = [0]


def pairs_call():
    turn[0] += 1
    ops.augment_pairs_u8(drawn[turn[0] % a.inner], x, y, ws)
    return 2 * -(-B // ops.AUG_GROUP)


identity = [AugSample((imgs[b], masks[b]), H, H) for b in range(B)]


def pairs_identity():
    ops.augment_pairs_u8(identity, x, y, ws)
    return 2 * -(-B // ops.AUG_GROUP)


def replaced():
    for b in range(B):
        ops.resize_bilinear_u8(imgs[b], rgb[b], 1.0 / 255.0, False)
        ops.resize_bilinear_u8(masks[b].unsqueeze(2), y[b], 1.0 / 255.0, False)
    ops.rgb2yuv_std(rgb, yuv, acc, scale, B, S * S)
    x.copy_(yuv[..., 0:1])
    return 2 * B + 2 + 2          # the resizes; shm_rgb2yuv_std's memset and two kernels; the channel copy


configs = {"pairs_call": pairs_call, "pairs_identity": pairs_identity, "replaced": replaced}
times, host, launches = {k: [] for k in configs}, {k: [] for k in configs}, {}
for r in range(a.warmup + a.repeats):
    for name, fn in configs.items():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        t0 = time.perf_counter()
        for _ in range(a.inner):
            launches[name] = fn()
        t1 = time.perf_counter()
        e1.record()
        e1.synchronize()
        if r >= a.warmup:
            times[name].append(e0.elapsed_time(e1) / a.inner)
            host[name].append((t1 - t0) * 1e3 / a.inner)
for name in configs:
    # ms: events around the window / inner -- the larger of what the device and what the enqueuing host takes per batch; host_ms: the
    # host clock around the same enqueues alone.  ms ~ host_ms says the stream ran dry between calls: launch-bound.
    report(name, times[name], host_ms=round(statistics.median(host[name]), 4), launches=launches[name], repeats=a.repeats, inner=a.inner)

# ---- one epoch of fit
with tempfile.TemporaryDirectory() as root:
    from PIL import Image
    from shmgan_amd.model import Arena
    from shmgan_amd.specseg import SpecSeg
    for sub in ("img", "mask"):
        (Path(root) / sub).mkdir()
    for i in range(a.pairs):
        Image.fromarray(rng.integers(0, 256, (H, H, 3)).astype(np.uint8)).save(Path(root) / "img" / f"p_{i:03d}.png", compress_level=1)
        Image.fromarray((rng.random((H, H)) < 0.2).astype(np.uint8) * 255).save(Path(root) / "mask" / f"p_{i:03d}.png", compress_level=1)
    plain = MaskDataset(str(Path(root) / "img"), str(Path(root) / "mask"), S, B)
    loaded = MaskDataset(str(Path(root) / "img"), str(Path(root) / "mask"), S, B, augment=aug, shuffle=True, seed=a.seed)
    t0 = time.perf_counter()
    xs, ys = plain.tensors()
    torch.cuda.synchronize()
    load_ms = (time.perf_counter() - t0) * 1e3
    nets = {k: SpecSeg(S, dev, Arena(dev)).init_random() for k in ("tensors", "dataset")}
    epoch = {k: [] for k in nets}
    for e in range(1 + a.epochs):                 # epoch 0 warms up: kernels, arenas, and the dataset's decode into its cache
        if e == 1:
            st = loaded.cache_stats()
            assert st["resident"] == a.pairs and st["refused"] == 0, st
        for k, net in nets.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            if k == "tensors":
                net.fit(xs, ys, batch_size=B, epochs=1, lr=1e-3, shuffle=True)
            else:
                net.fit(loaded, epochs=1, lr=1e-3)
            torch.cuda.synchronize()
            if e >= 1:
                epoch[k].append((time.perf_counter() - t0) * 1e3)
    for k in nets:
        report("fit_epoch/" + k, epoch[k], pairs=a.pairs, steps=len(plain), epochs=a.epochs,
               **({"load_once_ms": round(load_ms, 1)} if k == "tensors" else {"cache": loaded.cache_stats()}))
