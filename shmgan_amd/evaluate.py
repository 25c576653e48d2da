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
  - no Comet logging and no FID (commented out in the reference).  The images the reference logs to Comet (test.py:305-317) are
    written to disk instead when `save_images` is set (below).

Image export (`save_images`: False, "g1" or "all"): per test image, `<image_dir>/<stem>_<tag>.png` for the tags of
IMAGE_TAGS -- G1 RGB, G1 Y, the five cyclic reconstructions and the SpecSeg mask, the reference's log_image set without the
user's own input and diffuse files ("g1": G1 only).  `image_values` "rescale" maps each plane with rescale_01 (the reference's
test_plot display); "output" scales the RGB and Y planes by the running mean of the standardisation scales, the reference's
gen_rgb_output / 255, and clips.  The mask is always clipped.  `image_out_size` "source" resamples to the photo's own size
(bilinear, half-pixel centres: the inverse direction of the loader's resize), "model" writes S x S.  `image_dir` defaults to
`<result_dir>/images`.  The bytes come from the library's exporter (ops.export_u8, one call per batch); PNG encoding runs on a
pool of writer threads while the next batch is evaluated.
"""
from __future__ import annotations

import os
import pickle
import time
import warnings
from concurrent.futures import ThreadPoolExecutor

import torch

from . import ops
from .data import EvalDataset

TABLE_HEADERS = ["Image#", "Time", "MSE", "SSIM", "PSNR", "delE76", "delE94"]                  # test.py:371
MEAN_HEADERS = ["Mean MSE", "Mean SSIM", "Mean PSNR", "Mean dleE76", "Mean delE94"]           # test.py:381 (sic)
METRIC_KEYS = ["MSE", "PSNR", "SSIM", "delE76", "delE94"]     # the columns of ops.image_metrics, in order (ops.METRIC_NAMES)
IMAGE_TAGS = ("G1", "G1_Y", "cyc0", "cyc45", "cyc90", "cyc135", "cycED", "mask")                # test.py:305-317, in order
SAVE_IMAGES = {"g1": IMAGE_TAGS[:1], "all": IMAGE_TAGS}
IMAGE_VALUES = ("rescale", "output")
IMAGE_OUT_SIZES = ("source", "model")
IMAGE_WRITERS = 4                                             # PNG encoder threads (at most 16)


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


def image_name(stem, tag):
    """File name of one exported image: `<source stem>_<tag>.png`."""
    return f"{stem}_{tag}.png"


def source_stem(path):
    return os.path.splitext(os.path.basename(path))[0]


def check_stems(files):
    """Exported names are built from the source's stem: two sources with one stem (a.png, a.jpg) would overwrite each
    other's images, so that raises ValueError naming them."""
    seen = {}
    for f in files:
        seen.setdefault(source_stem(f), []).append(os.path.basename(f))
    dup = {s: v for s, v in seen.items() if len(v) > 1}
    if dup:
        raise ValueError("save_images names its files after the source's stem, and these sources share one: "
                         + "; ".join(f"{s}: {', '.join(sorted(v))}" for s, v in sorted(dup.items())))


def image_options(save, values, out_size):
    """The tags to write (an empty tuple: export off), checked against the accepted values."""
    if save in (False, None, ""):
        tags = ()
    elif save in SAVE_IMAGES:
        tags = SAVE_IMAGES[save]
    else:
        raise ValueError(f"save_images {save!r} is not False, 'g1' or 'all'")
    if values not in IMAGE_VALUES:
        raise ValueError(f"image_values {values!r} is not one of {IMAGE_VALUES}")
    if out_size not in IMAGE_OUT_SIZES:
        raise ValueError(f"image_out_size {out_size!r} is not one of {IMAGE_OUT_SIZES}")
    return tags


class ImageExporter:
    """Writes a batch's images after its evaluation: one ops.export_u8 call on the current stream into a device byte buffer, a
    copy into one of two pinned staging generations, an event, then the PNG encode and write on a pool of writer threads.
    The main thread blocks only when the generation it is about to fill is still being written by the batch before last."""

    def __init__(self, image_dir, tags, values, out_size, device, workers=IMAGE_WRITERS):
        self.dir, self.tags, self.values, self.out_size = image_dir, tuple(tags), values, out_size
        os.makedirs(image_dir, exist_ok=True)
        self.pool = ThreadPoolExecutor(max_workers=max(1, min(int(workers), 16)), thread_name_prefix="shm-png")
        self.dev = device
        self.buf = None                     # device bytes of one batch
        self.stage = [None, None]           # pinned host copies, two generations
        self.pending = [[], []]             # writer futures reading each generation
        self.gen = 0
        self.files = []
        # running {sum, count} of the standardisation scales over the whole run (test.py:77: stddev_arr is reset once)
        self.acc = torch.zeros(2, dtype=torch.float64, device=device) if values == "output" else None
        self.mul = None

    def _plane(self, tag, b, gen_rgb, cyc, gen_y, mask):
        if tag == "G1":
            return gen_rgb[b]
        if tag == "G1_Y":
            return gen_y[b]
        if tag == "mask":
            return mask[b]
        return cyc[IMAGE_TAGS.index(tag) - 2][b]

    def submit(self, shmgan, gen_rgb, cyc, sources):
        """Enqueue batch `sources` ((path, (h, w)) per image, in batch order) of the evaluation just issued."""
        B, S = int(gen_rgb.shape[0]), int(gen_rgb.shape[1])
        mul = None
        if self.values == "output":
            if self.mul is None or self.mul.numel() < B:
                self.mul = torch.empty(B, dtype=torch.float32, device=self.dev)
            mul = self.mul[:B]
            ops.running_scale_mean(shmgan.stddev_arr[0], self.acc, mul)
        planes, sizes, modes, jobs = [], [], [], []
        for b, (path, hw) in enumerate(sources):
            size = tuple(hw) if self.out_size == "source" else (S, S)
            for tag in self.tags:
                p = self._plane(tag, b, gen_rgb, cyc, shmgan.gen_Y, shmgan.specular_candidate)
                planes.append(p)
                sizes.append(size)
                modes.append("clip" if tag == "mask" else ("scale", b) if mul is not None else "rescale")
                jobs.append((os.path.join(self.dir, image_name(source_stem(path), tag)), size, int(p.shape[2])))
        offs, total = ops.export_layout(sizes, [c for _, _, c in jobs])
        if self.buf is None or self.buf.numel() < total:
            self.buf = torch.empty(total, dtype=torch.uint8, device=self.dev)
        # gen_rgb, the cyclic images, gen_Y and the mask are arena tensors that the next evaluate() overwrites: the export
        # reads them before that only because both are ordered on this one stream.  The same holds for self.buf and the copy.
        ops.export_u8(planes, sizes, modes, mul, self.buf, arena=shmgan.arena)
        g = self.gen
        self._wait(g)                       # the batch before last: its writers read this generation
        if self.stage[g] is None or self.stage[g].numel() < total:
            self.stage[g] = torch.empty(total, dtype=torch.uint8, pin_memory=True)
        stage = self.stage[g]
        stage[:total].copy_(self.buf[:total], non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        self.pending[g] = [self.pool.submit(_write_png, ev, stage, off, size, c, path)
                           for off, (path, size, c) in zip(offs, jobs)]
        self.files.extend(path for path, _, _ in jobs)
        self.gen ^= 1

    def _wait(self, g):
        futs, self.pending[g] = self.pending[g], []
        for f in futs:
            f.result()                      # re-raises a writer's exception

    def finish(self):
        """Wait for every writer; re-raises the first writer exception.  Returns the written paths in batch order."""
        self._wait(self.gen)
        self._wait(self.gen ^ 1)
        return list(self.files)


def _write_png(ev, stage, off, size, c, path):
    from PIL import Image
    ev.synchronize()
    h, w = size
    a = stage[off:off + h * w * c].numpy().reshape(h, w, c)
    Image.fromarray(a[:, :, 0] if c == 1 else a).save(path)
    return path


def test(shmgan, args, *, print_fn=print):
    """main.py:110 `test(shmgan, args)`.  Reads args.test_dir, args.diffuse_dir, args.calc_metrics and args.eval_batch_size
    (default 1), and the image export's args.save_images, image_values, image_out_size, image_dir (module docstring); model
    and folder settings come from the trainer (`image_size`, `checkpoint_save_dir`, `log_dir`, `result_dir`).  Returns a
    dict: "index" (1-based image numbers), "time" (seconds per image), "images" and "files" (the exported image paths, in
    batch order; empty without save_images); with calc_metrics also the per-image lists "MSE", "SSIM", "PSNR", "delE76",
    "delE94" and "means" (a dict of their means, None without metrics)."""
    test_dir = _arg(shmgan, args, "test_dir", "")
    calc = bool(_arg(shmgan, args, "calc_metrics", False))
    diffuse_dir = _arg(shmgan, args, "diffuse_dir", "") if calc else None
    B = int(_arg(shmgan, args, "eval_batch_size", 1) or 1)
    if not test_dir:
        raise ValueError("test mode needs args.test_dir")
    if calc and not diffuse_dir:
        raise ValueError("calc_metrics needs args.diffuse_dir (the ground-truth diffuse images)")
    tags = image_options(_arg(shmgan, args, "save_images", False), _arg(shmgan, args, "image_values", "rescale"),
                         _arg(shmgan, args, "image_out_size", "source"))
    shmgan.random_flip, shmgan.TARGET_LABELS = 0.0, 1.0                        # test.py:65-67
    dataset = EvalDataset(test_dir, shmgan.image_size, B, diffuse_dir, shmgan.device)
    if tags:
        check_stems(dataset.test_files)
    shmgan.number_of_test_images = dataset.n                                   # test.py:123
    if shmgan.G is None:
        shmgan.build()                                                          # test.py:139-140, 156
    shmgan._write_summaries()                                                   # test.py:142-158
    latest = shmgan._restore_latest()                                           # test.py:162-169
    if latest is None:
        warnings.warn(f"no checkpoint in {shmgan.checkpoint_save_dir}: evaluating the initial weights")
    else:
        print_fn(f"Latest checkpoint restored!! ({latest})")

    exporter = None
    if tags:
        image_dir = _arg(shmgan, args, "image_dir", "") or os.path.join(shmgan.result_dir, "images")
        exporter = ImageExporter(image_dir, tags, _arg(shmgan, args, "image_values", "rescale"),
                                 _arg(shmgan, args, "image_out_size", "source"), shmgan.device)
    index, times, rows = [], [], []
    cols = {k: [] for k in METRIC_KEYS}
    stream = torch.cuda.current_stream()
    try:
        for bi, (rgb, diffuse) in enumerate(dataset):
            stream.synchronize()                         # the batch's upload and resize are not part of its time
            t0 = time.perf_counter()
            gen_rgb, cyc, m = shmgan.evaluate(rgb, diffuse)
            m = None if m is None else m.cpu().tolist()  # a synchronising copy (without metrics: the synchronize below)
            stream.synchronize()
            n = rgb.shape[0]
            dt = (time.perf_counter() - t0) / n
            if exporter is not None:                     # after the timing window: the export is not part of "Time"
                exporter.submit(shmgan, gen_rgb, cyc, dataset.sources(bi))
            lo, _ = dataset.batch_range(bi)
            for b in range(n):
                index.append(lo + b + 1)
                times.append(dt)
                if m is not None:
                    for k, v in zip(METRIC_KEYS, m[b]):
                        cols[k].append(float(v))
                    rows.append([lo + b + 1, dt, cols["MSE"][-1], cols["SSIM"][-1], cols["PSNR"][-1], cols["delE76"][-1],
                                 cols["delE94"][-1]])
        files = exporter.finish() if exporter is not None else []
    finally:
        if exporter is not None:
            exporter.pool.shutdown(wait=True)       # also after an error: no writer outlives test()

    out = {"images": dataset.n, "index": index, "time": times, "means": None, "files": files}
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
