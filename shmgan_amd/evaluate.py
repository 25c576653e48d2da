"""The reference's test mode: `test(shmgan, args)` of test.py:40-392, called by main.py:110 for `--mode test`.

Every test image goes through the generator once plus five cyclic passes (`ShmGANwithSSpecSeg.infer`); with `calc_metrics` the
G1 output (gen_rgb, not clipped) is scored against the paired diffuse image with MSE, PSNR, SSIM, dE76 and dE94 on the library's
kernels (`ops.image_metrics`; include/shmgan_hip.h states the definitions).

Differences from the reference, all outside the arithmetic:
  - checkpoints are the .npz files `train()` writes (the newest `ckpt-*.npz` of `checkpoint_save_dir`, restored through the same
    path as training); with none there the run warns and goes on with the initial weights, as the reference's restore(None) does.
    `eval_checkpoint` = "best" (the best.npz train() keeps with validation on) or a path scores another file, `eval_weights` = "ema" the
    average of the generator's weights inside it (the whole loop runs under trainer.generator_weights); a missing file or a file
    without an average raises before any image is processed;
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
(bilinear, half-pixel centres: the inverse direction of the loader's resize), "model" writes the trainer's frame, S x S or the H x W of image_hw.  `image_dir` defaults to
`<result_dir>/images`.  The bytes come from the library's exporter (ops.export_u8, one call per batch); PNG encoding runs on a
pool of writer threads while the next batch is evaluated.

Native resolution (`eval_size`: "model", the default, is everything above; "native"): every test image and its diffuse partner
are loaded at their own h x w, padded by reflection to multiples of 16 (data.pad_geometry: the one place that states the rule),
standardised, segmented and generated on that frame, and scored and exported on the photo's window of it -- no resize anywhere.
G1 always runs; the five cyclic passes run only with `save_images="all"` (nothing else uses them), one after the other.
`image_out_size` is ignored: the output is the photo's size.  `eval_batch_size` must be 1 (sizes differ per image).  The
per-image "Time" covers whatever passes were run (G1, or G1 and the cyclic passes), SpecSeg and the metrics.  An image is
refused with ValueError, before anything is allocated or launched for it, when a tensor of its frame would pass
MAX_TENSOR_BYTES or MAX_FRAME_SIDE, or when native_frame_bytes() of its frame does not fit the free device memory
(MEMORY_HEADROOM); the message names the file and points to eval_size="model".  InstanceNorm statistics are per whole image,
so a frame is never tiled.

Region metrics (`metrics_region`: "off", the default, "residual" or "specseg"; needs `calc_metrics`): the five metrics once more, split
by the highlight -- "residual": where the photo exceeds its diffuse partner by more than `region_threshold` in any channel (default
16/255, the 16-byte-unit noise floor); "specseg": where the inference's SpecSeg mask exceeds it (default 0.5) -- into the pixels inside
and the ones outside (include/shmgan_hip.h, shm_image_metrics_region_hw, states the definitions; trainer.eval_region runs it).  The
returned dict gains "region": per-image lists "in_mse" ... "out_de94" (ops.REGION_METRIC_NAMES; NaN where an image has no such pixels)
and "fraction" (the part of the photo inside), "means" (per value, over the images whose set is not empty), "n_in_images" and
"n_out_images"; a second table is printed behind the reference's two, and `<result_dir>/region_metrics.jsonl` gets one line per image:
{"image": source stem, "fraction", the ten values}, NaN written as null.  Works at both eval sizes; "Time" then includes it.

Full-resolution output (`image_detail`: "off", the default, "residual" or "guided"; needs eval_size="model"): with image_out_size="source"
the G1 image above is a bilinear blow-up of the model-size plane -- a 1024 x 768 photo comes back as a 4x enlargement of 256 x 256.  The
generator only changes the standardised Y, so with image_detail on that change is transferred to the photo instead: fitted at model
resolution against the Y the network was fed (the fast guided filter of He & Sun; `detail_radius` 1..8 model pixels, default 2, and
`detail_eps`, default 1e-2), the fit's two coefficients upsampled with the library's bilinear sampler and applied to the photo's own Y at
its own size (trainer.refine; include/shmgan_hip.h, shm_detail_coeffs / shm_detail_apply_u8, states the arithmetic).  "residual" is the
same at radius 0: the upsampled correction added to the photo's Y.  Chroma and fine detail are the camera's, the highlight correction the
network's.  The `G1` file is then written from that plane (the photo's size, no resampling; image_values keeps its meaning on it), the
other tags as before; save_images therefore needs image_out_size="source".  With calc_metrics the tables, lists and pickles above are
computed as ever at model size, and the refined plane is scored in addition against the diffuse image at ITS own size (a partner of another
size than its photo raises ValueError naming both files): the returned dict gains "detail": {"mode", "radius", "eps", per-image lists
"MSE", "PSNR", "SSIM", "delE76", "delE94", "means"}, one more table is printed behind the others, and `<result_dir>/detail_metrics.jsonl`
gets one line per image: {"image": source stem, "size": [h, w], the five values}, NaN written as null.  The refinement runs outside the
timing window, like the export: "Time" stays what it is.  Off: nothing of this runs and nothing changes.
"""
from __future__ import annotations

import os
import pickle
import time
import warnings
from concurrent.futures import ThreadPoolExecutor
from types import SimpleNamespace

import torch

from . import ops
from .data import CAPTURE_OPTIONS, EvalDataset, NativeEvalDataset, capture_options, pad_geometry, trainer_frame
from .model import Arena, generator_layers, pad_channels
from .specseg import WIDTHS as SPECSEG_WIDTHS
from .telemetry import nan_to_none, region_means, region_options, write_lines

TABLE_HEADERS = ["Image#", "Time", "MSE", "SSIM", "PSNR", "delE76", "delE94"]                  # test.py:371
MEAN_HEADERS = ["Mean MSE", "Mean SSIM", "Mean PSNR", "Mean dleE76", "Mean delE94"]           # test.py:381 (sic)
METRIC_KEYS = ["MSE", "PSNR", "SSIM", "delE76", "delE94"]     # the columns of ops.image_metrics, in order (ops.METRIC_NAMES)
IMAGE_TAGS = ("G1", "G1_Y", "cyc0", "cyc45", "cyc90", "cyc135", "cycED", "mask")                # test.py:305-317, in order
SAVE_IMAGES = {"g1": IMAGE_TAGS[:1], "all": IMAGE_TAGS}
IMAGE_VALUES = ("rescale", "output")
IMAGE_OUT_SIZES = ("source", "model")
IMAGE_WRITERS = 4                                             # PNG encoder threads (at most 16)
EVAL_SIZES = ("model", "native")
# Largest per-tensor extent, in bytes, the native path supports: every convolution of the generator and of SpecSeg goes through
# launch_tapgemm (csrc/conv_igemm.hip), whose kernels address their operands with 32-bit byte offsets into buffer descriptors
# (0xffffffff is the "outside the image" offset) and which therefore requires `xb < lim`, xb = batch * hi * wi * ldx * esz and
# lim = 0xfffffff0, for every operand.  The widest tensors of a frame are the level-0 activations (filter_size channels) and
# the 64-byte-per-pixel network inputs (native_max_tensor_bytes).  The elementwise, InstanceNorm, head and colour kernels index
# with size_t; the pixel count (int32 in the launcher) and the exporter's 2^31 elements per plane bind later than this.
# A module attribute on purpose: tests lower it instead of allocating a huge image.
MAX_TENSOR_BYTES = 0xfffffff0
MAX_FRAME_SIDE = 32768                                        # shm_load_pad_u8, shm_image_metrics_hw, shm_export_u8_hw: sides in [1, 32768]
REGION_FILE = "region_metrics.jsonl"
REGION_HEADERS = ["Image#", "Inside"] + [f"{side} {k}" for side in ("in", "out") for k in ("MSE", "PSNR", "SSIM", "delE76", "delE94")]
DETAIL_FILE = "detail_metrics.jsonl"
IMAGE_DETAILS = ("off", "residual", "guided")
MEMORY_HEADROOM = 0.9                                         # fraction of the free device memory a frame's buffers may take


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


def detail_options(image_detail="off", detail_radius=2, detail_eps=1e-2):
    """The full-resolution output's options, checked: None for "off" (or None / False), else (mode, radius, eps) with mode "residual"
    (radius 0 whatever detail_radius says) or "guided" (detail_radius an integer in 1..8), detail_eps a positive finite number.
    Anything else raises ValueError naming the option."""
    if image_detail in (None, False, "", "off"):
        return None
    if image_detail not in IMAGE_DETAILS:
        raise ValueError(f"image_detail {image_detail!r} is not one of {IMAGE_DETAILS}")
    radius = 2 if detail_radius is None else detail_radius
    if image_detail == "guided" and (isinstance(radius, bool) or not isinstance(radius, int) or not 1 <= radius <= ops.DETAIL_MAX_RADIUS):
        raise ValueError(f"detail_radius {detail_radius!r} is not an integer in 1..{ops.DETAIL_MAX_RADIUS}")
    eps = 1e-2 if detail_eps is None else detail_eps
    if isinstance(eps, bool) or not isinstance(eps, (int, float)) or not (eps > 0 and eps < float("inf")):
        raise ValueError(f"detail_eps {detail_eps!r} is not a positive finite number")
    return image_detail, (0 if image_detail == "residual" else int(radius)), float(eps)


EVAL_WEIGHTS = ("raw", "ema")
EVAL_CHECKPOINTS = ("latest", "best")                         # or a path


def eval_options(eval_weights="raw", eval_checkpoint="latest"):
    """The two options that say WHAT test mode scores, checked: eval_weights "raw" or "ema" (the average train() keeps with ema_decay),
    eval_checkpoint "latest" (the newest ckpt-*.npz, as the reference), "best" (the best.npz train() keeps with validation on) or the
    path of a save_npz file.  Anything else raises ValueError."""
    if eval_weights not in EVAL_WEIGHTS:
        raise ValueError(f"eval_weights {eval_weights!r} is not one of {EVAL_WEIGHTS}")
    if eval_checkpoint not in EVAL_CHECKPOINTS and not (isinstance(eval_checkpoint, (str, os.PathLike)) and str(eval_checkpoint).endswith(".npz")):
        raise ValueError(f"eval_checkpoint {eval_checkpoint!r} is not one of {EVAL_CHECKPOINTS} or the path of an .npz checkpoint")
    return eval_weights, eval_checkpoint if eval_checkpoint in EVAL_CHECKPOINTS else os.fspath(eval_checkpoint)


def _restore_for_test(shmgan, eval_weights, eval_checkpoint, print_fn):
    """Load the weights test mode scores and check, before any image is processed, that they are there: the chosen file (a missing
    best.npz or path raises FileNotFoundError naming eval_checkpoint) and, for "ema", an average inside it (ValueError naming
    eval_weights)."""
    shmgan.args.eval_weights = eval_weights               # checkpoint.apply takes the average out of the file only for a trainer that wants it
    if eval_checkpoint == "latest":
        path = shmgan._restore_latest()                                         # test.py:162-169
        if path is None:
            warnings.warn(f"no checkpoint in {shmgan.checkpoint_save_dir}: evaluating the initial weights")
    else:
        path = os.path.join(shmgan.checkpoint_save_dir, shmgan.BEST_CHECKPOINT) if eval_checkpoint == "best" else eval_checkpoint
        if not os.path.exists(path):
            raise FileNotFoundError(f"eval_checkpoint={eval_checkpoint!r}: {path} does not exist" +
                                    (" (train() writes it with val_dir or val_fraction set)" if eval_checkpoint == "best" else ""))
        shmgan.load_npz(path)
    if path is not None:
        print_fn(f"Latest checkpoint restored!! ({path})" if eval_checkpoint == "latest" else f"Checkpoint restored ({path})")
    if eval_weights == "ema" and not (path is not None and shmgan._loaded_ema):
        raise ValueError(f"eval_weights='ema': {path or 'no checkpoint'} holds no average of the generator's weights (G/ema; train() writes "
                         f"it with ema_decay > 0)")
    return path


def _esz(dtype):
    return torch.empty((), dtype=dtype).element_size()


def native_max_tensor_bytes(hp, wp, filter_size, dtype=torch.float32):
    """Bytes of the largest single tensor a batch-1 native forward on an hp x wp frame hands a kernel: the level-0 activations
    [hp,wp,filter_size] in the activation dtype, or the 64-byte-per-pixel inputs (the generator's padded input, SpecSeg's
    float32 [hp,wp,16]), whichever is wider.  Deeper levels have twice the channels on a quarter of the pixels."""
    return int(hp) * int(wp) * max(int(filter_size) * _esz(dtype), pad_channels(dtype) * _esz(dtype), 16 * 4)


def native_frame_bytes(hp, wp, filter_size, dtype=torch.float32, cyclic=True, attention=False):
    """Device bytes the buffers of one native-resolution image on an hp x wp frame (multiples of 16) take, counted from the layer
    tables (model.generator_layers, specseg.WIDTHS) exactly as trainer.infer / Generator.forward / SpecSeg.forward_plane name
    them: every buffer proportional to the frame (per-channel statistics and workspaces, some kilobytes, are left out), no
    InstanceNorm folding (folding only removes buffers).  Linear in hp * wp.  The cyclic passes reuse the G1 pass's activations:
    `cyclic` adds only their 5 inputs and 5 outputs."""
    hp, wp, F = int(hp), int(wp), int(filter_size)
    if hp % 16 or wp % 16:
        raise ValueError(f"a frame has sides that are multiples of 16, got {hp} x {wp}")
    e, pad = _esz(dtype), pad_channels(dtype)
    px = hp * wp

    def lvl(l):
        return (hp >> l) * (wp >> l)
    n = 0
    # ---- loader and trainer.infer: frame + tight target (float32 RGB), yuv, cbcr, generator input, gen_rgb
    n += px * (12 + 12 + 12 + 8 + pad * e + 12)
    if cyclic:
        n += px * (4 + 4 + 5 * pad * e + 5 * 12)                  # orig_Ych, G1's Y kept beside the cyclic passes, cyc_in, cyc_rgb
    # ---- Generator.forward ("inf1"): per Conv -> LeakyReLU -> InstanceNorm block the conv output and the normalised tensor
    L = generator_layers(F)
    for l in range(4):                                            # encoder level l: two blocks, the pooled tensor
        c = L[2 * l][4]
        n += lvl(l) * c * e * 4 + lvl(l + 1) * c * e
        if attention:                                             # skip + attention map, and the branch's mask / y1 / y2
            n += lvl(l) * e * (c + pad + 2 * c)
    n += lvl(4) * L[8][4] * e * 4                                 # the two 1x1 blocks
    for j in range(4):                                            # decoder level 3 - j: Conv2DTranspose output, two blocks
        l, li = 3 - j, 10 + 3 * j
        n += lvl(l) * e * (L[li][4] + 2 * L[li + 1][4] + 2 * L[li + 2][4])
    n -= px * L[21][4] * e                                        # the last block is normalised by the head on the fly
    n += px * 4                                                   # gen_Y
    # ---- SpecSeg.forward_plane (float32): packed input, per level two conv outputs + BN, pooled; decoder: up + two convs; mask
    n += px * 16 * 4
    for l, w in enumerate(SPECSEG_WIDTHS):
        n += lvl(l) * w * 4 * 3 + (lvl(l + 1) * w * 4 if l < 4 else 0)
    for l in (3, 2, 1, 0):
        n += lvl(l) * SPECSEG_WIDTHS[l] * 4 * 3
    n += px * 4
    # ---- image export: up to 8 planes of bytes (6 RGB, 2 single-channel) on the device
    n += px * (6 * 3 + 2)
    return n


def check_native_limits(path, h, w, filter_size, dtype=torch.float32, cyclic=True, attention=False, free_bytes=None):
    """Raise ValueError if the native path cannot take the h x w image `path`: a frame side over MAX_FRAME_SIDE, a tensor over
    MAX_TENSOR_BYTES, or (free_bytes given) native_frame_bytes over MEMORY_HEADROOM * free_bytes.  Host arithmetic only."""
    hp, wp, _, _ = pad_geometry(h, w)
    why = None
    big = native_max_tensor_bytes(hp, wp, filter_size, dtype)
    need = native_frame_bytes(hp, wp, filter_size, dtype, cyclic, attention)
    if max(hp, wp) > MAX_FRAME_SIDE:
        why = f"a side of its {hp} x {wp} frame is over {MAX_FRAME_SIDE}"
    elif big >= MAX_TENSOR_BYTES:
        why = (f"the largest tensor of its {hp} x {wp} frame takes {big} bytes, and the convolution kernels address a tensor with "
               f"32-bit byte offsets (limit {MAX_TENSOR_BYTES})")
    elif free_bytes is not None and need > MEMORY_HEADROOM * free_bytes:
        why = (f"its {hp} x {wp} frame needs {need / 2**30:.2f} GiB of device buffers and {free_bytes / 2**30:.2f} GiB are free "
               f"(headroom {MEMORY_HEADROOM})")
    if why is not None:
        raise ValueError(f"{path} ({h} x {w}) is too large for eval_size='native': {why}.  Evaluate it with eval_size='model' "
                         f"(resized to image_size x image_size), or downscale the file")
    return need


class ImageExporter:
    """Writes a batch's images after its evaluation: one ops.export_u8 call on the current stream into a device byte buffer, a
    copy into one of two pinned staging generations, an event, then the PNG encode and write on a pool of writer threads.
    The main thread blocks only when the generation it is about to fill is still being written by the batch before last."""

    def __init__(self, image_dir, tags, values, out_size, device, workers=IMAGE_WRITERS):
        """out_size "native": submit() is given each image's window of the frame and writes exactly that window
        (ops.export_u8_hw: min / max of "rescale" over the window, no resampling)."""
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

    def submit(self, shmgan, gen_rgb, cyc, sources, windows=None, refined=None):
        """Enqueue batch `sources` ((path, (h, w)) per image, in batch order) of the evaluation just issued.  windows (out_size
        "native"): (top, left, h, w) per image, the photo inside the frame.  refined (image_detail; out_size "source"): per image the
        float32 [h,w,3] plane of trainer.refine, which the G1 tag is then written from -- the whole plane at its own size."""
        B, H, W = (int(v) for v in gen_rgb.shape[:3])
        native = self.out_size == "native"
        # a rectangular model frame, or refined planes of the photos' sizes: the windowed export over the whole plane
        whole = None if native or (H == W and refined is None) else (0, 0, H, W)
        wins = []
        mul = None
        if self.values == "output":
            if self.mul is None or self.mul.numel() < B:
                self.mul = torch.empty(B, dtype=torch.float32, device=self.dev)
            mul = self.mul[:B]
            ops.running_scale_mean(shmgan.stddev_arr[0], self.acc, mul)
        planes, sizes, modes, jobs = [], [], [], []
        for b, (path, hw) in enumerate(sources):
            size = tuple(windows[b][2:]) if native else tuple(hw) if self.out_size == "source" else (H, W)
            for tag in self.tags:
                if refined is not None and tag == "G1":
                    p = refined[b]
                    wins.append((0, 0, int(p.shape[0]), int(p.shape[1])))
                else:
                    wins.append(tuple(windows[b]) if native else whole)
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
        if native or whole is not None:
            ops.export_u8_hw(planes, wins, sizes, modes, mul, self.buf, arena=shmgan.arena)
        else:
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
    (default 1), args.eval_size ("model", the default: every image resized to the trainer's frame, image_size x image_size or image_hw; "native": every image at
    its own size -- eval_batch_size must then be 1, image_out_size is ignored, and "Time" covers the passes that were run: G1,
    plus the five cyclic passes with save_images="all"; module docstring), and the image export's args.save_images, image_values,
    image_out_size, image_dir (module docstring), and args.eval_weights / args.eval_checkpoint (eval_options: which file and which of its
    weight sets is scored; defaults "raw" / "latest"); model
    and folder settings come from the trainer (`image_size`, `checkpoint_save_dir`, `log_dir`, `result_dir`).  Returns a
    dict: "index" (1-based image numbers), "time" (seconds per image), "images" and "files" (the exported image paths, in
    batch order; empty without save_images); with calc_metrics also the per-image lists "MSE", "SSIM", "PSNR", "delE76",
    "delE94" and "means" (a dict of their means, None without metrics).  args.metrics_region / args.region_threshold (module docstring;
    default "off") add "region", a further table behind the two and region_metrics.jsonl, and nothing when off.  args.image_detail /
    detail_radius / detail_eps (detail_options; module docstring, "Full-resolution output"; default "off") write G1 from the plane
    trainer.refine makes at the photo's own size and, with calc_metrics, add "detail", one more table and detail_metrics.jsonl."""
    test_dir = _arg(shmgan, args, "test_dir", "")
    calc = bool(_arg(shmgan, args, "calc_metrics", False))
    diffuse_dir = _arg(shmgan, args, "diffuse_dir", "") if calc else None
    B = int(_arg(shmgan, args, "eval_batch_size", 1) or 1)
    eval_size = _arg(shmgan, args, "eval_size", "model") or "model"
    if eval_size not in EVAL_SIZES:
        raise ValueError(f"eval_size {eval_size!r} is not one of {EVAL_SIZES}")
    native = eval_size == "native"
    eval_weights, eval_checkpoint = eval_options(_arg(shmgan, args, "eval_weights", "raw") or "raw",
                                                 _arg(shmgan, args, "eval_checkpoint", "latest") or "latest")
    if native and B != 1:
        raise ValueError(f"eval_size='native' evaluates one image at a time (sizes differ per image): eval_batch_size must be 1, got {B}")
    if not test_dir:
        raise ValueError("test mode needs args.test_dir")
    if calc and not diffuse_dir:
        raise ValueError("calc_metrics needs args.diffuse_dir (the ground-truth diffuse images)")
    tags = image_options(_arg(shmgan, args, "save_images", False), _arg(shmgan, args, "image_values", "rescale"),
                         _arg(shmgan, args, "image_out_size", "source"))
    detail = detail_options(_arg(shmgan, args, "image_detail", "off"), _arg(shmgan, args, "detail_radius", 2), _arg(shmgan, args, "detail_eps", 1e-2))
    if detail is not None and native:
        raise ValueError(f"image_detail={detail[0]!r} transfers the model-size result to the photo: it needs eval_size='model' (at "
                         f"eval_size='native' the network already ran at the photo's size and there is nothing to transfer)")
    if detail is not None and tags and _arg(shmgan, args, "image_out_size", "source") != "source":
        raise ValueError(f"image_detail={detail[0]!r} writes G1 at the photo's size: save_images needs image_out_size='source'")
    region = region_options(_arg(shmgan, args, "metrics_region", "off"), _arg(shmgan, args, "region_threshold", None), "metrics_region")
    if region is not None and not calc:
        raise ValueError(f"metrics_region={region[0]!r} splits the image metrics: it needs calc_metrics (and diffuse_dir)")
    shmgan.random_flip, shmgan.TARGET_LABELS = 0.0, 1.0                        # test.py:65-67
    cyclic = not native or len(tags) > 1                                       # native: the cyclic images are only ever exported

    def check(path, h, w):
        """Before anything is allocated or launched for an image: the derived size limit, then the device memory.  The frame
        buffers the arena already holds are reused (same frame shape) or dropped (trainer._frame_changed: any other shape, the
        model-size one included) for this image, so they count as free."""
        free, _ = torch.cuda.mem_get_info(shmgan.device)
        held = sum(t.numel() * t.element_size() for k, t in shmgan.arena.t.items()
                   if isinstance(k[0], str) and k[0].startswith(shmgan._FRAME_BUFFERS))
        cached = torch.cuda.memory_reserved(shmgan.device) - torch.cuda.memory_allocated(shmgan.device)
        check_native_limits(path, h, w, shmgan.filter_size, shmgan.compute_dtype, cyclic, shmgan.attention == "live",
                            free_bytes=free + cached + held)

    # a polariser-mosaic test set (capture_format="dofp"): test_dir holds mosaics, dofp_test_view says which demosaiced plane is the photo
    _, capture = capture_options(SimpleNamespace(**{k: v for k in CAPTURE_OPTIONS if (v := _arg(shmgan, args, k)) is not None}))
    capture["dofp_test_view"] = _arg(shmgan, args, "dofp_test_view", "total")
    if native:
        dataset = NativeEvalDataset(test_dir, diffuse_dir, shmgan.device, check=check, **capture)
    else:
        dataset = EvalDataset(test_dir, trainer_frame(shmgan), B, diffuse_dir, shmgan.device, keep_source=detail is not None, **capture)
    if tags:
        check_stems(dataset.test_files)
    shmgan.number_of_test_images = dataset.n                                   # test.py:123
    if shmgan.G is None:
        shmgan.build()                                                          # test.py:139-140, 156
    shmgan._write_summaries()                                                   # test.py:142-158
    _restore_for_test(shmgan, eval_weights, eval_checkpoint, print_fn)

    exporter = None
    if tags:
        image_dir = _arg(shmgan, args, "image_dir", "") or os.path.join(shmgan.result_dir, "images")
        exporter = ImageExporter(image_dir, tags, _arg(shmgan, args, "image_values", "rescale"),
                                 "native" if native else _arg(shmgan, args, "image_out_size", "source"), shmgan.device)
    index, times, rows = [], [], []
    cols = {k: [] for k in METRIC_KEYS}
    region_rows, region_size, stems = [], [], []      # per image: the 12 region values, (pixels, SSIM positions) of its window, source stem
    detail_rows = []                                  # per image: (source stem, (h, w), the five values of the refined plane)
    refine_on = detail is not None and (bool(tags) or calc)
    detail_arena = Arena(shmgan.device) if refine_on and calc else None      # the metrics' workspace at the photos' sizes
    stream = torch.cuda.current_stream()
    eval_region_before = shmgan.eval_region
    try:
        if region is not None:
            shmgan.eval_region = region
        with shmgan.generator_weights(eval_weights):     # "raw": nothing; "ema": the whole loop runs on the average
            for bi, item in enumerate(dataset):
                rgb, diffuse, window = item if native else (*item, None)
                stream.synchronize()                         # the batch's upload and resize are not part of its time
                t0 = time.perf_counter()
                gen_rgb, cyc, m = shmgan.evaluate_frame(rgb, diffuse, window, cyclic) if native else shmgan.evaluate(rgb, diffuse)
                m = None if m is None else m.cpu().tolist()  # a synchronising copy (without metrics: the synchronize below)
                if region is not None:
                    region_rows.extend(shmgan.region_metrics.cpu().tolist())
                    h, w = window[2:] if native else gen_rgb.shape[1:3]
                    region_size.extend([(int(h) * int(w), (int(h) - 10) * (int(w) - 10))] * rgb.shape[0])
                    stems.extend(source_stem(path) for path, _ in dataset.sources(bi))
                stream.synchronize()
                n = rgb.shape[0]
                dt = (time.perf_counter() - t0) / n
                refined = None
                if refine_on:                                # after the timing window, like the export
                    refined = shmgan.refine(dataset.last_source[0], detail[0], detail[1] or 2, detail[2])
                    if calc:
                        detail_rows.extend(_score_refined(refined, dataset, bi, detail_arena))
                if exporter is not None:                     # after the timing window: the export is not part of "Time"
                    exporter.submit(shmgan, gen_rgb, cyc, dataset.sources(bi), [window] if native else None, refined)
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
        shmgan.eval_region = eval_region_before
        if exporter is not None:
            exporter.pool.shutdown(wait=True)       # also after an error: no writer outlives test()

    out = {"images": dataset.n, "index": index, "time": times, "means": None, "files": files}
    if not calc:
        if detail is not None:                      # what was applied; nothing was scored: empty lists, NaN means, no table, no file
            out["detail"] = _report_detail(shmgan, detail, index, [], print_fn)
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
    if region is not None:
        out["region"] = _report_regions(shmgan, index, stems, region_rows, region_size, print_fn)
    if detail is not None:
        out["detail"] = _report_detail(shmgan, detail, index, detail_rows, print_fn)
    return out


def _score_refined(refined, dataset, bi, arena):
    """The five image metrics of each refined plane of batch `bi` against its diffuse partner at the photo's own size: the partner's bytes
    (dataset.last_source) go to float32 on the device (ops.load_pad_u8 without a pad) and ops.image_metrics_hw scores the whole plane.
    Returns (source stem, (h, w), [mse, psnr, ssim, de76, de94]) per image; synchronises (the values come to the host), after which the
    workspace of this image's size leaves `arena`: sizes differ per image."""
    lo, _ = dataset.batch_range(bi)
    rows = []
    for b, (plane, src) in enumerate(zip(refined, dataset.last_source[1])):
        h, w = (int(v) for v in plane.shape[:2])
        if tuple(src.shape[:2]) != (h, w):
            raise ValueError(f"image_detail scores the refined image against its diffuse partner pixel by pixel: {dataset.test_files[lo + b]} is "
                             f"{h} x {w}, {dataset.diffuse_files[lo + b]} is {int(src.shape[0])} x {int(src.shape[1])}")
        target = torch.empty((1, h, w, 3), dtype=torch.float32, device=plane.device)
        ops.load_pad_u8(src, target[0], 0, 0, 1.0 / 255.0)
        m = ops.image_metrics_hw(plane.unsqueeze(0), (0, 0, h, w), target, arena=arena)
        rows.append((source_stem(dataset.test_files[lo + b]), (h, w), [float(v) for v in m.cpu()[0].tolist()]))
        arena.drop("metrics/ws")
    return rows


def _report_detail(shmgan, detail, index, rows, print_fn):
    """The "detail" entry of test()'s result from the per-image rows of _score_refined (none without calc_metrics: the lists are then
    empty and the means NaN); prints its table and writes <result_dir>/detail_metrics.jsonl (module docstring)."""
    mode, radius, eps = detail
    res = {"mode": mode, "radius": radius, "eps": eps}
    res.update({k: [r[2][j] for r in rows] for j, k in enumerate(METRIC_KEYS)})
    res["means"] = {k: (sum(res[k]) / len(res[k]) if res[k] else float("nan")) for k in METRIC_KEYS}
    if not rows:
        return res
    order = [METRIC_KEYS.index(k) for k in ("MSE", "SSIM", "PSNR", "delE76", "delE94")]           # the columns of TABLE_HEADERS
    print_fn(f" --- PRINTING METRICS AT THE PHOTOS' OWN SIZE (image_detail={mode!r}, radius {radius}, eps {eps:g}) --- ")
    print_fn(format_table([[i, f"{h}x{w}"] + [v[j] for j in order] for i, (_, (h, w), v) in zip(index, rows)] +
                          [["mean", ""] + [res["means"][METRIC_KEYS[j]] for j in order]], ["Image#", "Size"] + TABLE_HEADERS[2:]))
    print_fn("\n\n")
    os.makedirs(shmgan.result_dir, exist_ok=True)
    path = os.path.join(shmgan.result_dir, DETAIL_FILE)
    if os.path.exists(path):
        os.remove(path)                             # one file per run (write_lines appends)
    write_lines(path, [dict({"image": stem, "size": [h, w]}, **{k: nan_to_none(v[j]) for j, k in enumerate(METRIC_KEYS)}) for stem, (h, w), v in rows])
    return res


def _report_regions(shmgan, index, stems, rows, sizes, print_fn):
    """The "region" entry of test()'s result from the per-image rows (ops.REGION_METRIC_NAMES) and (pixels, SSIM positions) of each
    window; prints its table and writes <result_dir>/region_metrics.jsonl (module docstring)."""
    names = ops.REGION_METRIC_NAMES[:10]
    npix, npos = [a for a, _ in sizes], [b for _, b in sizes]
    means, n_in_images, n_out_images = region_means(rows, npix, npos) if rows else ({k: float("nan") for k in names}, 0, 0)
    res = {k: [float(r[j]) for r in rows] for j, k in enumerate(names)}
    res["fraction"] = [float(r[10]) / n for r, n in zip(rows, npix)]
    res.update(means=means, n_in_images=n_in_images, n_out_images=n_out_images)
    print_fn(" --- PRINTING METRICS INSIDE / OUTSIDE THE HIGHLIGHT --- ")
    print_fn(format_table([[i, f] + [float(v) for v in r[:10]] for i, f, r in zip(index, res["fraction"], rows)] +
                          [["mean", sum(res["fraction"]) / len(rows) if rows else float("nan")] + [means[k] for k in names]], REGION_HEADERS))
    print_fn("\n\n")
    path = os.path.join(shmgan.result_dir, REGION_FILE)
    if os.path.exists(path):
        os.remove(path)                             # one file per run (write_lines appends)
    write_lines(path, [dict({"image": stem, "fraction": f}, **{k: nan_to_none(float(r[j])) for j, k in enumerate(names)})
                       for stem, f, r in zip(stems, res["fraction"], rows)])
    return res
