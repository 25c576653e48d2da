"""Training telemetry: the loss log and the on-device gradient / weight histograms of the reference's train loop.

The reference logs its named loss scalars every 25 steps (SHM.py:1035-1053) and a histogram of every clipped gradient
tensor, gradmapD and gradmapG, every 100 steps (SHM.py:1085-1091).  Here both are JSON lines under `log_dir`, written
by a thread of their own, and nothing on the training thread waits for the device:

  losses.jsonl     one line per logged step: step, epoch, TARGET_LABELS, the 18 LOSS_NAMES, ssim (five values)
  gradients.jsonl  one line per variable and logged step: step, model, name, shape, the eight statistics of
                   ops.TSTAT_NAMES and `hist`, the non-empty bins as [sign, class, count] (shm_tensor_stats,
                   include/shmgan_hip.h, defines the classes); the values are the gradients times 1 / world, i.e. what
                   the optimizer clips
  weights.jsonl    the same records of the weights after that step's update

A variable's name is its checkpoint key in save_npz: G/var00.., D/var00.. in Keras variable order.

A logged step costs one tiny launch (shm_loss_ring_put: the raw loss vectors into a row of a device ring); a histogram
step costs two launches per model and buffer (shm_tensor_stats).  The ring and the statistics are copied into one of two
pinned staging generations behind an event; the writer thread waits on the event, composes the scalars and writes.
The training thread blocks only when the generation it is about to fill is still being written (the flush before last).
"""
from __future__ import annotations

import json
import os
import threading
import warnings
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from . import checkpoint, ops

LOSS_NAMES = ["total_Generator_loss", "total_Discriminator_loss", "total_Classification_loss", "G_gan_loss",
              "G_clsf_loss", "D1_RealFake_loss", "D3_RealFake_cyc", "D2_RealFake_target", "D4_RealFake_cyc",
              "D1_classification_loss", "D3_classification_loss", "D4_classification_loss", "L1_loss_Gen",
              "ssim_cyc_loss", "content_loss", "style_loss", "total_NST_loss", "Spec_loss"]

NONFINITE_MODES = ("ignore", "warn", "raise")
LOG_FILES = {"losses": "losses.jsonl", "gradients": "gradients.jsonl", "weights": "weights.jsonl"}
RING_ROWS = 64


class NonFiniteGradientError(RuntimeError):
    """A gradient histogram that reached the host counted NaN or Inf values (nonfinite="raise").  The check runs when the
    record arrives, so the step it names lies at most one flush back."""


def compose_losses(dl, il, sl, B, npix):
    """The reference's named loss scalars (mean over the batch) from the raw sums the kernels leave on the device: dl
    (shm_dhead_losses, 16), il (shm_image_losses, 32), sl (shm_spec_loss, 5), as float64 arrays.  A pure function, used by
    Trainer.losses() and by the log writer, so both give the same bits."""
    d = (np.asarray(dl, dtype=np.float64) / B).tolist()
    i = (np.asarray(il, dtype=np.float64) / B).tolist()
    D1_RF, D3_RF = d[0], d[1]
    D2_RF = d[4] + d[2]
    D4_RF = d[5] + d[3] + D2_RF
    D1_cls, D3_cls, D4_cls = d[6], d[7], d[8]
    L1 = (i[1] + i[2] + i[3] + i[4] + i[0]) / 5.0 + i[5] * 10.0
    ssim_loss = (i[11] + i[12] + i[13] + i[14] + i[15] * 10.0) / 5.0
    content, style = i[16], i[17]
    nst = 100.0 * style + content
    sp = (np.asarray(sl, dtype=np.float64) / (B * npix * 3.0)).tolist()       # reduce_mean over [B,S,S,3]
    return {
        "total_Generator_loss": (D1_RF + D3_RF) / 6.0 + 10.0 * L1 + 10.0 * ssim_loss + 10.0 * nst,
        "total_Discriminator_loss": (D1_cls + D3_cls) / 6.0 + (D2_RF + D4_RF) / 6.0 + 0.5 * D4_cls + 10.0 * nst,
        "total_Classification_loss": (D4_cls + nst) * 10.0,
        "G_gan_loss": (D3_RF + D1_RF) / 6.0, "G_clsf_loss": (D3_cls + D1_cls) / 6.0,
        "D1_RealFake_loss": D1_RF, "D3_RealFake_cyc": D3_RF, "D2_RealFake_target": D2_RF,
        "D4_RealFake_cyc": D4_RF, "D1_classification_loss": D1_cls, "D3_classification_loss": D3_cls,
        "D4_classification_loss": D4_cls, "L1_loss_Gen": L1, "ssim_cyc_loss": ssim_loss,
        "content_loss": content, "style_loss": style, "total_NST_loss": nst,
        "Spec_loss": (sp[0] + sp[1] + sp[2] + sp[3]) / 5.0 + sp[4] * 5.0,
        "ssim": [i[6 + k] for k in range(5)],
    }


def telemetry_options(loss_log_step=0, histogram_step=0, nonfinite=None):
    """The three options, checked: (loss_log_step, histogram_step, nonfinite).  A step option of 0 / None / False is off;
    nonfinite defaults to "warn" when either is on and to "ignore" otherwise."""
    steps = []
    for name, v in (("loss_log_step", loss_log_step), ("histogram_step", histogram_step)):
        if v in (None, False, ""):
            v = 0
        if isinstance(v, bool) or not isinstance(v, (int, np.integer, str)) or (isinstance(v, str) and not v.strip().isdigit()):
            raise ValueError(f"{name} {v!r} is not a step count (0 = off)")
        v = int(v)
        if v < 0:
            raise ValueError(f"{name} {v!r} is negative")
        steps.append(v)
    if nonfinite in (None, ""):
        nonfinite = "warn" if any(steps) else "ignore"
    if nonfinite not in NONFINITE_MODES:
        raise ValueError(f"nonfinite {nonfinite!r} is not one of {NONFINITE_MODES}")
    return steps[0], steps[1], nonfinite


def variable_table(model, tag):
    """[(name, offset, size, shape)] of a model's variables in Keras variable order: name = the checkpoint key."""
    P = model.P
    return [(name, int(P.offsets[i]), int(np.prod(P.shapes[i])), tuple(int(d) for d in P.shapes[i]))
            for name, i in checkpoint.variable_keys(model, tag)]


def stats_record(step, model, name, shape, stats, hist):
    """One gradients.jsonl / weights.jsonl line (a dict) from a variable's stats [8] and hist [2, 44]."""
    rec = {"step": int(step), "model": model, "name": name, "shape": list(shape)}
    for k, key in enumerate(ops.TSTAT_NAMES):
        rec[key] = float(stats[k]) if key in ("min", "max", "sum", "sumsq") else int(stats[k])
    rec["hist"] = [[int(s), int(c), int(hist[s, c])] for s in range(2) for c in range(ops.THIST_BINS) if hist[s, c]]
    return rec


def hist_dense(record):
    """The [2, 44] histogram of a gradients.jsonl / weights.jsonl record."""
    h = np.zeros((2, ops.THIST_BINS), dtype=np.int64)
    for s, c, n in record["hist"]:
        h[s, c] = n
    return h


def read_log(log_dir):
    """{"losses": [...], "gradients": [...], "weights": [...]}: the three files as lists of dicts (an absent file: [])."""
    out = {}
    for key, fn in LOG_FILES.items():
        path = os.path.join(log_dir, fn)
        out[key] = []
        if os.path.exists(path):
            with open(path) as f:
                out[key] = [json.loads(line) for line in f if line.strip()]
    return out


VALIDATION_FILE = "validation.jsonl"
# what `val_monitor` may name (the columns of ops.image_metrics) and the sign that makes a larger value the better one
VAL_MONITORS = {"mse": -1.0, "psnr": 1.0, "ssim": 1.0, "de76": -1.0, "de94": -1.0}
# with a region (val_region / metrics_region): where the highlight comes from, each source's default threshold -- 16/255 is the project's
# 16-byte-unit noise floor of photo - diffuse, 0.5 the middle of SpecSeg's sigmoid -- and what val_monitor may then name as well: a
# metric inside ("in_") or outside ("out_") the highlight, judged by that metric's own sign
REGION_SOURCES = ("off", "residual", "specseg")
REGION_THRESHOLDS = {"residual": 16.0 / 255.0, "specseg": 0.5}
REGION_MONITORS = {f"{side}_{k}": sign for side in ("in", "out") for k, sign in VAL_MONITORS.items()}
WEIGHT_SETS = ("raw", "ema")                               # the generator weights one can infer with (trainer.generator_weights)


def region_options(source="off", threshold=None, name="metrics_region"):
    """The option pair `name` / `<name>_threshold` (test mode's metrics_region, validation's val_region), checked: None when off, else
    (source, threshold) with the source's default threshold (REGION_THRESHOLDS) when none is given.  An unknown source and a threshold
    that is not a finite number raise ValueError naming the option."""
    source = "off" if source in (None, False, "") else source
    if source not in REGION_SOURCES:
        raise ValueError(f"{name} {source!r} is not one of {REGION_SOURCES}")
    if source == "off":
        return None
    if threshold is None:
        return source, REGION_THRESHOLDS[source]
    if isinstance(threshold, bool) or not isinstance(threshold, (int, float, np.integer, np.floating)) or not np.isfinite(threshold):
        raise ValueError(f"{name}_threshold {threshold!r} is not a finite number")
    return source, float(threshold)


def validation_options(val_dir="", val_fraction=0.0, val_seed=0, val_step=1, val_batch_size=None, val_monitor="psnr", val_region="off"):
    """The held-out validation options of train(), checked: (on, val_step, val_monitor).  `on` is whether a held-out set was asked for
    (val_dir or val_fraction; both together raise ValueError).  An unknown val_monitor, a val_step below 1, a val_batch_size below 1 and
    a val_fraction outside [0, 1) raise ValueError whether validation is on or not.  With val_region on (region_options checks it),
    val_monitor may also name one of REGION_MONITORS ("in_psnr", ...)."""
    val_fraction = float(val_fraction or 0.0)
    if val_dir and val_fraction:
        raise ValueError(f"val_dir ({val_dir!r}) and val_fraction ({val_fraction}) are two sources of one held-out set: give one of them")
    if not 0.0 <= val_fraction < 1.0:
        raise ValueError(f"val_fraction {val_fraction!r} is not a fraction in [0, 1)")
    region_on = region_options(val_region, None, "val_region") is not None
    if val_monitor not in VAL_MONITORS and not (region_on and val_monitor in REGION_MONITORS):
        if val_monitor in REGION_MONITORS:
            raise ValueError(f"val_monitor {val_monitor!r} needs val_region ('residual' or 'specseg'): the region metrics are off")
        raise ValueError(f"val_monitor {val_monitor!r} is not one of {tuple(VAL_MONITORS) + (tuple(REGION_MONITORS) if region_on else ())}")
    if isinstance(val_step, bool) or not isinstance(val_step, (int, np.integer)) or val_step < 1:
        raise ValueError(f"val_step {val_step!r} is not a number of epochs (at least 1)")
    if val_batch_size is not None and (isinstance(val_batch_size, bool) or not isinstance(val_batch_size, (int, np.integer)) or val_batch_size < 1):
        raise ValueError(f"val_batch_size {val_batch_size!r} is not a batch size (at least 1, or None for the training batch size)")
    int(val_seed)
    return bool(val_dir or val_fraction), int(val_step), val_monitor


def improves(monitor, value, best):
    """Whether `value` of metric `monitor` beats `best` (None: nothing to beat).  psnr and ssim are maximised, the others minimised, inside
    or outside a region ("in_psnr", "out_de94") as over the whole image; a NaN (a region metric's mean when no image had the set) never
    improves."""
    if value != value:
        return False
    sign = VAL_MONITORS[monitor] if monitor in VAL_MONITORS else REGION_MONITORS[monitor]
    return best is None or sign * (value - best) > 0.0


def region_means(rows, npix, npos):
    """Host side of the region metrics: rows [n,12] (ops.REGION_METRIC_NAMES per image), npix / npos the window's pixels and SSIM
    positions (one number, or one per image).  Returns (means, n_in_images, n_out_images): for each of the ten in_* / out_* values the
    float64 mean over the images whose set is not empty -- pixels for mse, psnr and the dE values, SSIM positions for ssim -- NaN when no
    image has it, and the number of images with pixels inside / outside."""
    rows = np.asarray(rows, np.float64).reshape(-1, ops.REGION_METRICS)
    n_in, p_in = rows[:, 10], rows[:, 11]
    counts = ((n_in, p_in), (np.asarray(npix, np.float64) - n_in, np.asarray(npos, np.float64) - p_in))
    means = {}
    for s, (pixels, positions) in enumerate(counts):
        for j, k in enumerate(ops.METRIC_NAMES):
            v = rows[(positions if k == "ssim" else pixels) > 0, 5 * s + j]
            means[ops.REGION_METRIC_NAMES[5 * s + j]] = float(v.mean()) if v.size else float("nan")
    return means, int((counts[0][0] > 0).sum()), int((counts[1][0] > 0).sum())


def nan_to_none(v):
    """A float for a JSON line: NaN becomes None (null), everything else stays."""
    return None if isinstance(v, float) and v != v else v


def read_validation(log_dir):
    """The rows of `log_dir`/validation.jsonl as a list of dicts, in file order (an absent file: [])."""
    path = os.path.join(log_dir, VALIDATION_FILE)
    if not os.path.exists(path):
        return []
    with open(path) as f:
        return [json.loads(line) for line in f if line.strip()]


def write_lines(path, records):
    """Append records to a JSON-lines file (float64 values round-trip exactly through repr)."""
    with open(path, "a") as f:
        for r in records:
            f.write(json.dumps(r) + "\n")


class _Table:
    def __init__(self, model, tag):
        self.tag = tag
        self.vars = variable_table(model, tag)
        self.seg = ops.SegmentTable([o for _, o, _, _ in self.vars], [z for _, _, z, _ in self.vars])
        self.n = len(self.vars)


class Telemetry:
    """Owned by the trainer (Trainer.start_telemetry).  Holds the segment tables of G and D, the device ring and result
    buffers, two pinned staging generations per kind and the writer thread.  Everything is issued on the current stream, in
    step order; one Telemetry serves one trainer on one thread."""

    def __init__(self, trainer, log_dir=None, loss_log_step=0, histogram_step=0, nonfinite=None, ring_rows=RING_ROWS):
        self.loss_log_step, self.histogram_step, self.nonfinite = telemetry_options(loss_log_step, histogram_step, nonfinite)
        self.log_dir = log_dir
        self.dev = trainer.device
        self.abort_dev = trainer.arena.abort.dev
        self.tables = {"G": _Table(trainer.G, "G"), "D": _Table(trainer.D, "D")}
        self.models = {"G": trainer.G, "D": trainer.D}
        self.arena = trainer.arena
        # result rows of one histogram step: [G grad | D grad | G weights | D weights]
        nG, nD = self.tables["G"].n, self.tables["D"].n
        self.rows = {("gradients", "G"): 0, ("gradients", "D"): nG, ("weights", "G"): nG + nD, ("weights", "D"): 2 * nG + nD}
        self.nrows = 2 * (nG + nD)
        self.stats = torch.zeros((self.nrows, ops.TSTAT_N), dtype=torch.float64, device=self.dev)
        self.hist = torch.zeros((self.nrows, 2, ops.THIST_BINS), dtype=torch.int64, device=self.dev)
        self.ring = torch.zeros((int(ring_rows), ops.LOSS_ROW), dtype=torch.float64, device=self.dev)
        torch.cuda.current_stream(self.dev).synchronize()           # the zero fills, once
        self.ring_meta = []                 # per filled row: (step, epoch, TARGET_LABELS, B, npix)
        self.ring_stage = [None, None]      # pinned copies of the ring, two generations
        self.hist_stage = [None, None]      # pinned (stats, hist), two generations
        self.pending = {"ring": [None, None], "hist": [None, None]}
        self.gen = {"ring": 0, "hist": 0}
        self.issued = []                    # (kind, model) filled since the last stage copy
        self.pool = None
        self._lock = threading.Lock()
        self._found = []                    # non-finite findings the writer made, not yet reported

    # ------------------------------------------------------------------ schedule
    def wants_loss(self, step):
        return self.loss_log_step > 0 and step % self.loss_log_step == 0

    def wants_histograms(self, step):
        return self.histogram_step > 0 and step % self.histogram_step == 0

    # ------------------------------------------------------------------ device side (training thread, current stream)
    def _run(self, kind, tag, scale):
        M, tab, r0 = self.models[tag], self.tables[tag], self.rows[(kind, tag)]
        x = M.P.grad if kind == "gradients" else M.P.flat
        out = (self.stats[r0:r0 + tab.n], self.hist[r0:r0 + tab.n])
        ops.tensor_stats(x, tab.seg, scale=scale, out=out, arena=self.arena)
        return out

    def record_gradients(self, tag, scale=1.0):
        """Statistics of model `tag`'s flat gradient times `scale`; stage_histograms() sends them to the writer."""
        self._run("gradients", tag, scale)
        self.issued.append(("gradients", tag))

    def record_weights(self, tag):
        self._run("weights", tag, 1.0)
        self.issued.append(("weights", tag))

    def record_loss(self, step, epoch, target_label, last):
        """The raw loss vectors of the step just issued (`last` = trainer._last) into the next ring row."""
        if len(self.ring_meta) == self.ring.shape[0]:
            self.stage_ring()
        ops.loss_ring_put(last.dl, last.il, last.sl, self.abort_dev, self.ring, len(self.ring_meta), step)
        self.ring_meta.append((int(step), int(epoch), float(target_label), int(last.B), int(last.npix)))

    def _submit(self, kind, g, fn, *args):
        if self.pool is None:
            self.pool = ThreadPoolExecutor(max_workers=1, thread_name_prefix="shm-telemetry")
        self.pending[kind][g] = self.pool.submit(fn, *args)

    def _wait(self, kind, g):
        fut, self.pending[kind][g] = self.pending[kind][g], None
        if fut is not None:
            fut.result()                    # re-raises a writer's exception

    def stage_ring(self):
        """Copy the filled ring rows to pinned memory behind an event and hand them to the writer."""
        meta, self.ring_meta = self.ring_meta, []
        if not meta:
            return
        g = self.gen["ring"]
        self._wait("ring", g)
        if self.ring_stage[g] is None:
            self.ring_stage[g] = torch.empty(tuple(self.ring.shape), dtype=torch.float64, pin_memory=True)
        stage = self.ring_stage[g]
        stage[:len(meta)].copy_(self.ring[:len(meta)], non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        self._submit("ring", g, self._write_losses, ev, stage, meta)
        self.gen["ring"] ^= 1

    def stage_histograms(self, step):
        """The same for the statistics recorded since the last call (they belong to `step`)."""
        issued, self.issued = self.issued, []
        if not issued:
            return
        g = self.gen["hist"]
        self._wait("hist", g)
        if self.hist_stage[g] is None:
            self.hist_stage[g] = (torch.empty(tuple(self.stats.shape), dtype=torch.float64, pin_memory=True),
                                  torch.empty(tuple(self.hist.shape), dtype=torch.int64, pin_memory=True))
        st, hi = self.hist_stage[g]
        st.copy_(self.stats, non_blocking=True)
        hi.copy_(self.hist, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        self._submit("hist", g, self._write_histograms, ev, st, hi, int(step), issued)
        self.gen["hist"] ^= 1

    def after_step(self, step, epoch, target_label, last, histograms, update_g):
        """End of train_step `step` (gradient statistics of a histogram step are already recorded, beside the optimizer
        launches): the weights after the update, the loss row, and the copies to the host."""
        if self.wants_loss(step):
            self.record_loss(step, epoch, target_label, last)
        if histograms:
            for tag in ("G", "D") if update_g else ("D",):
                self.record_weights(tag)
            self.stage_histograms(step)
            self.stage_ring()               # a histogram step also brings the loss lines up to date

    # ------------------------------------------------------------------ host side
    def flush(self):
        """Send what is pending, wait for the writer, report non-finite findings.  Synchronises with the device."""
        self.stage_ring()
        for kind in ("ring", "hist"):
            for g in (0, 1):
                self._wait(kind, g)
        self.check()

    def check(self):
        """Report the writer's non-finite findings on the calling thread: a warning, or NonFiniteGradientError."""
        with self._lock:
            found, self._found = self._found, []
        if not found or self.nonfinite == "ignore":
            return
        msg = "; ".join(f"step {s}: {name} has {nan} NaN and {inf} Inf of {n} gradient values" for s, name, nan, inf, n in found[:8])
        if len(found) > 8:
            msg += f"; and {len(found) - 8} more variables"
        if self.nonfinite == "raise":
            raise NonFiniteGradientError(msg)
        warnings.warn(msg, RuntimeWarning, stacklevel=2)

    def close(self):
        """Flush and stop the writer thread."""
        try:
            self.flush()
        finally:
            if self.pool is not None:
                self.pool.shutdown(wait=True)
                self.pool = None

    # -- writer thread
    def _path(self, key):
        os.makedirs(self.log_dir, exist_ok=True)
        return os.path.join(self.log_dir, LOG_FILES[key])

    def _write_losses(self, ev, stage, meta):
        ev.synchronize()
        rows = stage[:len(meta)].numpy()
        recs = []
        for row, (step, epoch, target, B, npix) in zip(rows, meta):
            if int(row[ops.LOSS_ROW_STEP]) != step:
                raise RuntimeError(f"loss ring: row of step {int(row[ops.LOSS_ROW_STEP])} where step {step} was expected")
            a, b = ops.LOSS_ROW_DL, ops.LOSS_ROW_DL + ops.LOSS_ROW_IL
            rec = {"step": step, "epoch": epoch, "TARGET_LABELS": target}
            rec.update(compose_losses(row[:a], row[a:b], row[b:b + ops.LOSS_ROW_SL], B, npix))
            if row[ops.LOSS_ROW_ABORT] != 0:
                rec["abort"] = int(row[ops.LOSS_ROW_ABORT])       # a kernel of this run gave up (KernelAbortError): not a healthy step
            recs.append(rec)
        if self.log_dir is not None:
            write_lines(self._path("losses"), recs)

    def _records(self, st, hi, step, kind, tag):
        tab, r0 = self.tables[tag], self.rows[(kind, tag)]
        return [stats_record(step, tag, name, shape, st[r0 + k], hi[r0 + k]) for k, (name, _, _, shape) in enumerate(tab.vars)]

    def _write_histograms(self, ev, st, hi, step, issued):
        ev.synchronize()
        st, hi = st.numpy(), hi.numpy()
        out = {"gradients": [], "weights": []}
        for kind, tag in issued:
            out[kind].extend(self._records(st, hi, step, kind, tag))
        bad = [(step, r["name"], r["nan"], r["inf"], int(np.prod(r["shape"]))) for r in out["gradients"] if r["nan"] or r["inf"]]
        if bad:
            with self._lock:
                self._found.extend(bad)
        if self.log_dir is not None:
            for kind, recs in out.items():
                if recs:
                    write_lines(self._path(kind), recs)

    # ------------------------------------------------------------------ interactive
    def stats_now(self, kind, scale=1.0):
        """{name: {"stats": float64 [8], "hist": int64 [2, 44], "shape": ...}} of both models' gradients (times `scale`) or
        weights as they are now.  Synchronises; not for the step."""
        res = {}
        for tag in ("G", "D"):
            st, hi = self._run(kind, tag, scale)
            st, hi = st.cpu().numpy(), hi.cpu().numpy()
            for k, (name, _, _, shape) in enumerate(self.tables[tag].vars):
                res[name] = {"stats": st[k].copy(), "hist": hi[k].copy(), "shape": shape}
        return res
