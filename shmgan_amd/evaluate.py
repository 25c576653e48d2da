"""The reference's test mode: `test(shmgan, args)` of test.py:40-392, called by main.py:110 for `--mode test`.

Every test image goes through the generator once plus five cyclic passes (`ShmGANwithSSpecSeg.infer`); with `calc_metrics` the
G1 output (gen_rgb, not clipped) is scored against the paired diffuse image with MSE, PSNR, SSIM, dE76 and dE94 on the library's
kernels (`ops.image_metrics`; include/shmgan_hip.h states the definitions).

Differences from the reference, all outside the arithmetic:
  - checkpoints are the .npz files `train()` writes (the newest `ckpt-*.npz` of `checkpoint_save_dir`, restored through the same
    path as training); with none there the run warns and goes on with the initial weights, as the reference's restore(None) does;
  - the model summaries go to `log_dir` (as in `train()`), and SSIM.txt / MSE.txt / PSNR.txt to `result_dir` rather than the
    working directory; the pickled lists hold Python floats;
  - images are evaluated `eval_batch_size` at a time (default 1, as the reference); every sample is an independent B=1
    reference call and the last batch may be partial.  The per-image "Time" is the batch's time over its size: from the loaded
    batch to the metrics on the host, device synchronised;
  - a test / diffuse count mismatch raises (tf.data's zip would stop at the shorter list);
  - no Comet logging, no FID (commented out in the reference), no display-only image outputs.
"""
from __future__ import annotations

import os
import pickle
import time
import warnings

import torch

from .data import EvalDataset

TABLE_HEADERS = ["Image#", "Time", "MSE", "SSIM", "PSNR", "delE76", "delE94"]                  # test.py:371
MEAN_HEADERS = ["Mean MSE", "Mean SSIM", "Mean PSNR", "Mean dleE76", "Mean delE94"]           # test.py:381 (sic)
METRIC_KEYS = ["MSE", "PSNR", "SSIM", "delE76", "delE94"]     # the columns of ops.image_metrics, in order (ops.METRIC_NAMES)


def format_table(rows, headers):
    """tabulate(rows, headers=headers) when tabulate is installed, else plain aligned columns."""
    try:
        from tabulate import tabulate
    except ImportError:
        tabulate = None
    if tabulate is not None:
        return tabulate(rows, headers=headers)
    cells = [[str(h) for h in headers]] + [[f"{v:.6g}" if isinstance(v, float) else str(v) for v in r] for r in rows]
    width = [max(len(c[i]) for c in cells) for i in range(len(headers))]
    lines = ["  ".join(c[i].rjust(width[i]) for i in range(len(headers))) for c in cells]
    lines.insert(1, "  ".join("-" * w for w in width))
    return "\n".join(lines)


def _arg(shmgan, args, name, default=None):
    if args is not None and hasattr(args, name):
        return getattr(args, name)
    return getattr(shmgan.args, name, default)


def test(shmgan, args, *, print_fn=print):
    """main.py:110 `test(shmgan, args)`.  Reads args.test_dir, args.diffuse_dir, args.calc_metrics and args.eval_batch_size
    (default 1); model and folder settings come from the trainer (`image_size`, `checkpoint_save_dir`, `log_dir`,
    `result_dir`).  Returns a dict: "index" (1-based image numbers), "time" (seconds per image) and "images"; with
    calc_metrics also the per-image lists "MSE", "SSIM", "PSNR", "delE76", "delE94" and "means" (a dict of their means,
    None without metrics)."""
    test_dir = _arg(shmgan, args, "test_dir", "")
    calc = bool(_arg(shmgan, args, "calc_metrics", False))
    diffuse_dir = _arg(shmgan, args, "diffuse_dir", "") if calc else None
    B = int(_arg(shmgan, args, "eval_batch_size", 1) or 1)
    if not test_dir:
        raise ValueError("test mode needs args.test_dir")
    if calc and not diffuse_dir:
        raise ValueError("calc_metrics needs args.diffuse_dir (the ground-truth diffuse images)")
    shmgan.random_flip, shmgan.TARGET_LABELS = 0.0, 1.0                        # test.py:65-67
    dataset = EvalDataset(test_dir, shmgan.image_size, B, diffuse_dir, shmgan.device)
    shmgan.number_of_test_images = dataset.n                                   # test.py:123
    if shmgan.G is None:
        shmgan.build()                                                          # test.py:139-140, 156
    shmgan._write_summaries()                                                   # test.py:142-158
    latest = shmgan._restore_latest()                                           # test.py:162-169
    if latest is None:
        warnings.warn(f"no checkpoint in {shmgan.checkpoint_save_dir}: evaluating the initial weights")
    else:
        print_fn(f"Latest checkpoint restored!! ({latest})")

    index, times, rows = [], [], []
    cols = {k: [] for k in METRIC_KEYS}
    stream = torch.cuda.current_stream()
    for bi, (rgb, diffuse) in enumerate(dataset):
        stream.synchronize()                         # the batch's upload and resize are not part of its time
        t0 = time.perf_counter()
        _, _, m = shmgan.evaluate(rgb, diffuse)
        m = None if m is None else m.cpu().tolist()  # a synchronising copy (without metrics: the synchronize below)
        stream.synchronize()
        n = rgb.shape[0]
        dt = (time.perf_counter() - t0) / n
        lo, _ = dataset.batch_range(bi)
        for b in range(n):
            index.append(lo + b + 1)
            times.append(dt)
            if m is not None:
                for k, v in zip(METRIC_KEYS, m[b]):
                    cols[k].append(float(v))
                rows.append([lo + b + 1, dt, cols["MSE"][-1], cols["SSIM"][-1], cols["PSNR"][-1], cols["delE76"][-1],
                             cols["delE94"][-1]])

    out = {"images": dataset.n, "index": index, "time": times, "means": None}
    if not calc:
        return out
    out.update(cols)
    means = {k: (sum(v) / len(v) if v else float("nan")) for k, v in cols.items()}
    out["means"] = means
    print_fn("\n\n --- PRINTING ALL CALCUATED METRICS --- ")                  # test.py:370-371
    print_fn(format_table(rows, TABLE_HEADERS))
    print_fn("\n\n --- PRINTING MEAN METRICS --- ")                             # test.py:373-381
    print_fn(format_table([[means["MSE"], means["SSIM"], means["PSNR"], means["delE76"], means["delE94"]]], MEAN_HEADERS))
    print_fn("\n\n")
    os.makedirs(shmgan.result_dir, exist_ok=True)
    for name, key in (("SSIM.txt", "SSIM"), ("MSE.txt", "MSE"), ("PSNR.txt", "PSNR")):      # test.py:385-392
        with open(os.path.join(shmgan.result_dir, name), "wb+") as f:
            pickle.dump(cols[key], f)
    return out
