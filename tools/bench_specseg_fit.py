"""Training the mask network end to end on a synthetic task (smooth background plus bright discs, mask = the discs): writes image / mask PNG
pairs to a temporary directory, builds a trainer from init_random(), scores the untrained SpecSeg on held-out pairs (SpecSeg.evaluate), runs
ShmGANwithSSpecSeg.train_specseg on the training pairs, scores again, and times one train_step with HIP events (median over --repeats).
The default is 600 steps: BatchNormalization's moving statistics, which evaluate / predict use, move by 1 % per step (momentum 0.99) and
are still 30 % initial values after 120.  Prints one JSON line: IoU / F1 / loss before and after, step_ms.  Under `rocprofv3 --kernel-trace --stats -- python tools/bench_specseg_fit.py`
the kernel table of the run is the per-kernel baseline of LABNOTES.md section 18.
python tools/bench_specseg_fit.py [--size 64] [--train 32] [--held-out 8] [--batch 8] [--epochs 150] [--lr 2e-3] [--repeats 10]"""
import argparse
import json
import statistics
import sys
import tempfile
from pathlib import Path
from types import SimpleNamespace
sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import numpy as np
import torch

ap = argparse.ArgumentParser()
ap.add_argument("--size", type=int, default=64)
ap.add_argument("--train", type=int, default=32)
ap.add_argument("--held-out", type=int, default=8)
ap.add_argument("--batch", type=int, default=8)
ap.add_argument("--epochs", type=int, default=150)
ap.add_argument("--lr", type=float, default=2e-3)
ap.add_argument("--repeats", type=int, default=10)
ap.add_argument("--seed", type=int, default=0)
a = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("bench_specseg_fit needs a GPU: there is nothing to train without one")
from PIL import Image
from shmgan_amd import ShmGANwithSSpecSeg
from shmgan_amd.data import MaskDataset


def discs(n, S, rng):
    yy, xx = np.mgrid[0:S, 0:S].astype(np.float64) / S
    out = []
    for _ in range(n):
        p, q, r = rng.uniform(-1, 1, 3)
        img = 0.35 + 0.15 * (p * xx + q * yy) + 0.05 * np.sin(6.28 * (xx * r + yy))
        m = np.zeros((S, S))
        for _ in range(rng.integers(1, 4)):
            cx, cy, rad = rng.uniform(0.15, 0.85), rng.uniform(0.15, 0.85), rng.uniform(0.08, 0.2)
            m = np.maximum(m, ((xx - cx) ** 2 + (yy - cy) ** 2 < rad * rad).astype(np.float64))
        out.append((np.clip(img + 0.4 * m, 0, 1), m))
    return out


def write(pairs, root):
    (root / "img").mkdir(parents=True)
    (root / "msk").mkdir()
    for k, (img, m) in enumerate(pairs):
        g = np.uint8(img * 255)
        Image.fromarray(np.stack([g, g, g], -1)).save(root / "img" / f"{k:04d}.png")
        Image.fromarray(np.uint8(m * 255)).save(root / "msk" / f"{k:04d}.png")


rng = np.random.default_rng(a.seed)
with tempfile.TemporaryDirectory() as tmp:
    tmp = Path(tmp)
    write(discs(a.train, a.size, rng), tmp / "train")
    write(discs(a.held_out, a.size, rng), tmp / "held")
    m = ShmGANwithSSpecSeg(image_size=a.size, filter_size=16, batch_size=a.batch).build()
    hx, hy = MaskDataset(str(tmp / "held" / "img"), str(tmp / "held" / "msk"), a.size, a.batch).tensors()
    before = m.SpecSeg.evaluate(hx, hy, batch_size=a.batch)
    hist = m.train_specseg(SimpleNamespace(specseg_image_dir=str(tmp / "train" / "img"), specseg_mask_dir=str(tmp / "train" / "msk"),
                                           specseg_epochs=a.epochs, specseg_lr=a.lr, specseg_batch_size=a.batch), print_fn=lambda s: print(s, file=sys.stderr))
    after = m.SpecSeg.evaluate(hx, hy, batch_size=a.batch)
    tx, ty = MaskDataset(str(tmp / "train" / "img"), str(tmp / "train" / "msk"), a.size, a.batch).tensors()
    xb, yb = tx[:a.batch].contiguous(), ty[:a.batch].contiguous()
    ms = []
    for _ in range(a.repeats + 2):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        m.SpecSeg.train_step(xb, yb)
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
print(json.dumps(dict(size=a.size, batch=a.batch, train=a.train, epochs=a.epochs, lr=a.lr, held_out_before=before, held_out_after=after,
                      train_loss_first=hist["loss"][0], train_loss_last=hist["loss"][-1], step_ms=statistics.median(ms[2:]))))
