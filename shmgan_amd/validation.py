"""Held-out validation of a trainer: scoring the generator on captures that training never sees (`validate`), and the validation step
of train() with its log line and best.npz (`validate_and_log`).  The options and the comparison rule are telemetry.py's."""
import os

import numpy as np
import torch

from . import checkpoint, dist, ops
from .data import capture_options, gib_to_bytes, trainer_frame, validation_loader
from .telemetry import VALIDATION_FILE, WEIGHT_SETS, improves, nan_to_none, region_means, region_options, write_lines


def _loader(t):
    """The held-out loader of the trainer's val_dir / val_fraction options (None with both off), made once."""
    if t.valDataset is None:
        a = t.args
        subdirs, capture = capture_options(a)
        t.valDataset = validation_loader(
            t.data_dir, trainer_frame(t), t.batch_size, val_dir=a.val_dir, val_fraction=float(a.val_fraction or 0.0), val_seed=int(a.val_seed),
            val_batch_size=a.val_batch_size, subdirs=subdirs, device=t.device, diffuse_source=a.diffuse_source, cache=a.cache,
            cache_bytes=gib_to_bytes(a.cache_gb), **capture)
    return t.valDataset


def validate(t, dataset=None, weights=("raw",), region="args"):
    """Score the generator on held-out captures with test mode's protocol (evaluate.test): view 0 as the photo, the other views
    zero, target label ED (infer without the cyclic passes), gen_rgb against the sample's ED image with ops.image_metrics (ops.image_metrics_hw on a
    rectangular model frame).
    dataset: a data.PolarDataset (default: the held-out loader of the trainer's val_dir / val_fraction options); only its full
    batches are scored.  weights: the weight sets to score, each under generator_weights().  Per set every batch's rows go into one
    [n,5] float64 device buffer; ONE device-to-host copy ends the pass and the means are taken in float64 on the host.
    Returns {"n": images scored, "held_out": images listed, <set>: {"mse", "psnr", "ssim", "de76", "de94" (means), "rows" ([n,5])}}.
    region: None, or (source, threshold) as telemetry.region_options returns it (default: the trainer's val_region / val_region_threshold
    options) -- every batch's metrics are then also split by the highlight (trainer._region_metrics: the photo is batch[0], the target
    batch[4]) into the same device buffer, still one copy per pass, and each set also holds "region_rows" ([n,12],
    ops.REGION_METRIC_NAMES), the ten "in_*" / "out_*" means over the images whose set is not empty (NaN when there is none) and
    "n_in_images" / "n_out_images".
    Reads no draw stream and writes nothing a training step relies on (its buffers are infer's and its own), so a run that
    validates takes bitwise the steps of one that does not."""
    if t.G is None:
        t.build()
    if dataset is None:
        dataset = _loader(t)
        if dataset is None:
            raise ValueError("validate: no held-out set (give a dataset, or set val_dir or val_fraction)")
    for w in weights:
        if w not in WEIGHT_SETS:
            raise ValueError(f"validate: {w!r} is not one of {WEIGHT_SETS}")
    if region == "args":
        region = region_options(getattr(t.args, "val_region", "off"), getattr(t.args, "val_region_threshold", None), "val_region")
    B, nb = int(dataset.B), len(dataset)
    n = nb * B
    out = {"n": n, "held_out": int(dataset.n)}
    if region is None:
        rows = t.arena.get("val/rows", (max(n, 1), 5), torch.float64)
    else:                       # one buffer for both tables: [n,5] in front, [n,12] behind it
        both = t.arena.get("val/rows+region", (max(n, 1) * (5 + ops.REGION_METRICS),), torch.float64)
        rows, rrows = both[:max(n, 1) * 5].view(-1, 5), both[max(n, 1) * 5:].view(-1, ops.REGION_METRICS)
    for w in weights:
        with t.generator_weights(w):
            for i, batch in enumerate(dataset):
                gen_rgb, _ = t.infer(batch[0], cyclic=False)
                H, W = int(gen_rgb.shape[1]), int(gen_rgb.shape[2])
                ops.image_metrics_hw(gen_rgb, (0, 0, H, W), t._dev(batch[4]), out=rows[i * B:(i + 1) * B], arena=t.arena)     # the model frame, scored whole
                if region is not None:
                    t._region_metrics(region, t._dev(batch[0]), gen_rgb, t._dev(batch[4]), (0, 0, H, W), out=rrows[i * B:(i + 1) * B])
            # the pass's one device-to-host copy (it synchronises)
            host = (rows[:n] if region is None else both).cpu().numpy().astype(np.float64, copy=True)
        if region is not None:
            host, rhost = host[:max(n, 1) * 5].reshape(-1, 5)[:n], host[max(n, 1) * 5:].reshape(-1, ops.REGION_METRICS)[:n]
        means = host.mean(axis=0) if n else np.full(5, np.nan)
        out[w] = dict({k: float(v) for k, v in zip(ops.METRIC_NAMES, means)}, rows=host)
        if region is not None:
            H, W = t.image_hw
            rmeans, n_in_images, n_out_images = region_means(rhost, H * W, (H - 10) * (W - 10))
            out[w].update(rmeans, region_rows=rhost, n_in_images=n_in_images, n_out_images=n_out_images)
    return out


def validate_and_log(t, print_fn=print):
    """One validation of train(): every rank scores the whole held-out set (raw weights, and the average with ema_decay on), rank 0
    appends one line per weight set to <log_dir>/validation.jsonl, and when the monitored value -- val_monitor of the average
    with ema_decay on, of the raw weights otherwise -- beats the best so far, rank 0 writes <checkpoint_save_dir>/best.npz.  The
    step counts optimizer updates; weights that have been scored already (the end of a run right behind an epoch's validation) are
    not scored again."""
    step = int(t.D.P.iterations)
    if t._last_val_step == step:
        return None
    t._last_val_step = step
    t._check_abort(sync=True)     # never score (or keep as the best) weights behind a step whose kernels gave up
    sets = ("raw", "ema") if t._ema_on() else ("raw",)
    res = t.validate(weights=sets, region=t._val_region)
    monitored, mon = sets[-1], t._val_monitor
    best_now = False
    if res["n"]:
        value = res[monitored][mon]
        if improves(mon, value, None if t._best is None else t._best["value"]):
            best_now = True
            t._best = {"monitor": mon, "weights": monitored, "value": value, "step": step}
    if dist.rank() == 0:
        os.makedirs(t.log_dir, exist_ok=True)
        write_lines(os.path.join(t.log_dir, VALIDATION_FILE),
                    [dict({"step": step, "epoch": int(t.epoch), "weights": w, "n": res["n"], "held_out": res["held_out"]},
                          **{k: res[w][k] for k in ops.METRIC_NAMES},
                          **({} if t._val_region is None else dict({k: nan_to_none(res[w][k]) for k in ops.REGION_METRIC_NAMES[:10]},
                                                                   n_in_images=res[w]["n_in_images"])),
                          best=bool(best_now and w == monitored)) for w in sets])
        if best_now:
            checkpoint.write_atomic(t, os.path.join(t.checkpoint_save_dir, checkpoint.BEST_CHECKPOINT))
        print_fn(f"Validation at step {step} ({res['n']} of {res['held_out']} held-out images): " +
                 "; ".join(f"{w} {mon} {res[w][mon]:.6g}" for w in sets) + (" -- best so far, saved" if best_now else ""))
    return res
