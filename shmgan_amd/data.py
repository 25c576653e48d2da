"""Dataset loader: the caller side of `train_step` for real data.

Mirrors /root/reference/datasetLoader.py:19-170 (`datasetLoad(self)`): five sibling directories of the
polarimetric views are listed in sorted order (image_dataset_from_directory(labels=None, shuffle=False)),
zipped, every file decoded to RGB, resized to image_size x image_size with tf.image.resize's bilinear kernel,
scaled by 1/255 and flipped top-to-bottom.  As executed the flip is unconditional: the `map` lambda
`x if self.random_flip else flip_up_down(x)` (datasetLoader.py:61) is traced once with the constructor's
`self.random_flip = 0.0` (SHM.py:203); `flip_ud=` makes it explicit.

Decode is PIL on the host, in a WORKER THREAD: the decoded bytes land in pinned uint8 staging buffers, go to the GPU
with non-blocking copies on the loader's side stream, and the rest is one kernel (shm_resize_bilinear_u8) per image on
that stream.  The training thread only enqueues the next batch and, when it takes a batch, waits for the worker's
future and makes its stream wait for the batch's event -- the 5 B decodes of batch j+1 run under step j.

`diffuse_source` says where the fifth tensor comes from.  "dir" (default) is the reference's path above: a fifth directory of
pre-computed estimated-diffuse images.  "min" / "stokes" need only the four view directories: the worker decodes 4 B files and
one kernel per SAMPLE (shm_polar_views_u8) writes all five tensors, the diffuse estimate made per source pixel from the four
decoded views ("Estimated diffuse on the device") -- B launches and 4 B uploads per batch instead of 5 B of each.

`shuffle` and `augment` are the as-intended train-time loader (the reference's --flip, whose per-step draw its traced `map` lambda
never sees): an epoch-wise shuffle, and per sample one random crop / mirror drawn by the stateless `augment_params`, applied by ONE
kernel per sample (shm_augment_views_u8) at the decoded bytes for all three `diffuse_source` modes.  A single mirror turns a polariser
angle theta into 180 - theta, so the four views are permuted or re-mixed with it (polar.mirror_views).  Without
either option the loader calls exactly the kernels described above.

`cache="device"` keeps every sample's decoded bytes on the device after its first decode (shmgan_amd/cache.py: an arena of uint8
chunks under a byte budget, keyed by the sample's position in the sorted file lists; the reference's `.cache()`), and builds every
batch -- all three `diffuse_source` modes, with or without `shuffle` and `augment` -- with ONE shm_augment_batch_u8 launch from
per-sample descriptors: no decode and no upload for a resident sample.  A sample the budget does not hold takes the decode-and-upload
path every time.  Files that change on disk during a run are not noticed; under data parallelism each rank caches the samples it
sees (with `shuffle`, eventually the whole set).  `cache="none"` (default) calls exactly the kernels described above.

`capture="dofp"` reads a polariser-mosaic (division-of-focal-plane) sensor: ONE raw frame per sample instead of four view files.  The
worker decodes it once, the loader stream uploads it once and demosaics it once (shm_dofp_views, csrc/dofp.hip) into the four uint8
views, which then stand where the uploaded files stood in every path above (`PolarDataset._sources` is that one place; the device cache
stores the demosaiced views).  DESIGN.md section 6m.

Under torch.distributed the loader shards by rank: global batch i of rank r is images [(i*world + r)*B, +B), so N ranks
consume N*B distinct samples per step (the data-parallel identity of shmgan_amd/dist.py) and len() = n // (B*world).
"""
from __future__ import annotations

import os
from concurrent.futures import ThreadPoolExecutor
from dataclasses import dataclass
from pathlib import Path
from typing import NamedTuple

import numpy as np
import torch

from . import dist, ops
from .model import frame_hw

PSD_SUBDIRS = ("I0", "I60", "I90", "I150", "ED")          # datasetLoader.py:30-34 (PSD polar dataset)
SHMGAN_SUBDIRS = ("I0", "I45", "I90", "I135", "ED")       # datasetLoader.py:23-27 (commented alternative)
DIFFUSE_SOURCES = ("dir", "min", "stokes")                # where the fifth tensor comes from (PolarDataset)
CACHE_MODES = ("none", "device")                          # where decoded samples are kept between passes (PolarDataset)
_EXT = (".bmp", ".gif", ".jpeg", ".jpg", ".png")          # Keras' ALLOWLIST_FORMATS
BRACKET_EXT = (".tif", ".tiff")       # a bracketed sample is one multi-page TIFF: listed for the mosaic directory of a bracketed layout only


def gib_to_bytes(cache_gb):
    """The `cache_gb` / `specseg_cache_gb` option (GiB of device memory; None = half of what is free) as a loader's cache_bytes."""
    return None if cache_gb is None else int(float(cache_gb) * 2 ** 30)


def list_images(directory, also=()):
    """Sorted file list as image_dataset_from_directory(shuffle=False) yields it; `also`: further extensions to list (mosaic_extensions)."""
    d = Path(directory)
    ext = _EXT + tuple(also)
    return sorted(str(p) for p in d.iterdir() if p.suffix.lower() in ext)


def mosaic_extensions(dofp):
    """What list_images lists `also` in the mosaic directory of layout `dofp`: the TIFFs of a bracketed layout, nothing otherwise."""
    return BRACKET_EXT if getattr(dofp, "bracket", None) is not None else ()


AUGMENT_VIEWS = ("physical", "keep")


@dataclass(frozen=True)
class Augment:
    """Per-sample random augmentation of PolarDataset.  flip_lr / flip_ud: probabilities of a left-right / top-bottom mirror (the
    drawn flip_ud is XOR-ed onto the loader's fixed flip_ud orientation).  crop_min: the crop keeps the source aspect and covers a
    fraction a ~ U(crop_min, 1) of its area (side fraction sqrt(a)), its origin uniform over the positions that fit; 1.0 = no crop.
    views: "physical" = when exactly one mirror is drawn the four views follow it (a polariser at theta sees of the mirrored scene
    what one at 180 - theta saw: polar.mirror_views); "keep" = the reference's plain geometric flip."""
    flip_lr: float = 0.0
    flip_ud: float = 0.0
    crop_min: float = 1.0
    views: str = "physical"

    def __post_init__(self):
        for name in ("flip_lr", "flip_ud"):
            p = getattr(self, name)
            if not isinstance(p, (int, float)) or not 0.0 <= p <= 1.0:
                raise ValueError(f"Augment: {name} {p!r} is not a probability in [0, 1]")
        if not isinstance(self.crop_min, (int, float)) or not 0.0 < self.crop_min <= 1.0:
            raise ValueError(f"Augment: crop_min {self.crop_min!r} is not an area fraction in (0, 1]")
        if self.views not in AUGMENT_VIEWS:
            raise ValueError(f"Augment: views {self.views!r} is not one of {AUGMENT_VIEWS}")


class AugmentParams(NamedTuple):
    crop: tuple          # (y, x, h, w) in source pixels: floats that float32 holds exactly, inside [0,hin] x [0,win]
    flip_ud: bool        # the DRAWN top-bottom mirror (before the loader's fixed orientation)
    flip_lr: bool
    remap: bool          # exactly one mirror drawn: the views stand for other polariser angles


def _fit_origin(u, size, extent):
    """u * (size - extent) as a float32 value with origin + extent <= size in exact arithmetic (what the kernel's host check adds)."""
    o = np.float32(u * (size - float(extent)))
    if float(o) + float(extent) > size:
        o = np.nextafter(o, np.float32(0.0))
    return o


def augment_params(seed, pass_index, position, hin, win, augment):
    """The draw of the sample at `position` of the sorted file list in pass `pass_index`: a pure function of its arguments, so the
    worker thread, the rank and a resume do not change what a sample gets.  Five uniforms from default_rng((seed, pass_index,
    position)), always in this order: crop area, crop row, crop column, flip_ud, flip_lr.  crop_min = 1 and zero probabilities give
    the identity (0, 0, hin, win), no flips.  Both mirrors together are a rotation by 180 degrees, the identity on polariser
    angles: `remap` is set when exactly one is drawn."""
    u = np.random.default_rng((int(seed), int(pass_index), int(position))).random(5)
    side = np.sqrt(augment.crop_min + (1.0 - augment.crop_min) * u[0])
    ch, cw = np.float32(min(side * hin, hin)), np.float32(min(side * win, win))
    cy, cx = _fit_origin(u[1], hin, ch), _fit_origin(u[2], win, cw)
    fud, flr = bool(u[3] < augment.flip_ud), bool(u[4] < augment.flip_lr)
    return AugmentParams((float(cy), float(cx), float(ch), float(cw)), fud, flr, fud != flr)


def pass_order(n, seed, pass_index, shuffle):
    """Dataset position of every slot of pass `pass_index`: the sorted order, or with `shuffle` a permutation that depends on (seed,
    pass_index) alone -- the same on every rank, which then takes its slots by PolarDataset.image_index."""
    return np.random.default_rng((int(seed), int(pass_index))).permutation(n) if shuffle else np.arange(n)


class PolarDataset:
    """Iterable of 5-tuples of [B,H,W,3] float32 device tensors in [0,1].  image_size: the output frame, a side S (H = W = S) or a
    pair (H, W); every image is resized to it whole (a crop drawn by `augment` keeps the source's aspect).

    diffuse_source: "dir" = the fifth of `subdirs` holds the estimated-diffuse images (the reference's loader); "min" = the
    per-channel minimum of the four views (utils.calculate_estimate_diffuse), "stokes" = the fitted minimum over all polariser
    angles, both computed on the device from the first four `subdirs` alone.  angles: the polariser angles in degrees for
    "stokes" (default: read from the directory names, polar.angles_from_subdirs).

    shuffle: every pass visits the samples in the order pass_order(n, seed, pass) instead of the sorted one.  augment: an Augment,
    or None; with one, every sample goes through shm_augment_views_u8 with the draw augment_params(seed, pass, position, ...), and
    views="physical" needs the polariser angles (`angles`, or the directory names).  Passes count from `first_pass` (a resumed run
    sets it, so that it does not replay pass 0).

    cache: "none", or "device" = decoded samples stay on the device after their first decode (cache.SampleCache) and every batch is
    one shm_augment_batch_u8 launch; cache_bytes: the device memory the cache may take (default: half of what is free when the first
    sample is stored).  With "device" the images of a sample must have one decoded size, whatever the other options.

    capture: "views" = one file per polariser angle (the above); "dofp" = a polariser-mosaic sensor: the FIRST of `subdirs` holds one
    raw mosaic per sample (8-bit "L" or 16-bit "I;16" files, polar.decode_mosaic), laid out as `dofp` (a polar.DofpLayout) says, and
    the second -- read only for diffuse_source "dir" -- the diffuse images, which must have the demosaiced size.  Every sample is
    decoded once, uploaded once and demosaiced once on the loader stream (shm_dofp_views, `dofp_demosaic` = "bilinear" or "bin");
    its four views, in ascending angle, then take every path above unchanged, and the device cache stores them as it stores
    decoded views.  `angles` defaults to dofp.angles."""

    def __init__(self, data_dir, image_size, batch_size=1, subdirs=PSD_SUBDIRS, flip_ud=True, device=None, epochs=1,
                 rank=None, world=None, diffuse_source="dir", angles=None, shuffle=False, augment=None, seed=0, first_pass=0,
                 cache="none", cache_bytes=None, select=None, capture="views", dofp=None, dofp_demosaic="bilinear"):
        from . import polar
        polar.check_capture(capture, dofp, dofp_demosaic, "PolarDataset")
        self.capture, self.dofp, self.dofp_demosaic = capture, dofp, dofp_demosaic
        # what split() builds its two parts from: this dataset's own options (rank / world as given: None = torch.distributed's)
        self._options = dict(data_dir=data_dir, image_size=image_size, batch_size=batch_size, subdirs=tuple(subdirs), flip_ud=flip_ud,
                             device=device, epochs=epochs, rank=rank, world=world, diffuse_source=diffuse_source, angles=angles,
                             shuffle=shuffle, augment=augment, seed=seed, first_pass=first_pass, cache=cache, cache_bytes=cache_bytes,
                             capture=capture, dofp=dofp, dofp_demosaic=dofp_demosaic)
        if capture == "dofp" and angles is None:          # the views come out in ascending angle
            angles = dofp.angles
        self.S, self.B, self.flip_ud, self.epochs = image_size, batch_size, flip_ud, epochs
        self.H, self.W = frame_hw(image_size)
        if cache not in CACHE_MODES:
            raise ValueError(f"cache {cache!r} is not one of {CACHE_MODES}")
        if cache_bytes is not None and (not isinstance(cache_bytes, int) or cache_bytes < 0):
            raise ValueError(f"cache_bytes {cache_bytes!r} is not a byte count")
        self.cache, self.cache_bytes, self._cache, self._scratch = cache, cache_bytes, None, {}
        if augment is not None and not isinstance(augment, Augment):
            raise ValueError(f"augment must be a data.Augment or None, got {augment!r}")
        self.shuffle, self.augment, self.seed, self.first_pass = bool(shuffle), augment, int(seed), int(first_pass)
        self._mirror = ("identity", None)
        if augment is not None and augment.views == "physical" and (augment.flip_lr > 0 or augment.flip_ud > 0):
            ang = list(angles if angles is not None else polar.angles_from_subdirs(tuple(subdirs)[:4]))
            if len(ang) != 4:
                raise ValueError(f"augment views='physical' takes four angles, got {ang}")
            self._mirror = polar.mirror_views(ang)
        if diffuse_source not in DIFFUSE_SOURCES:
            raise ValueError(f"diffuse_source {diffuse_source!r} is not one of {DIFFUSE_SOURCES}")
        self.diffuse_source, self.coef = diffuse_source, None
        if capture == "dofp":          # the first of subdirs holds the mosaics, the second (read for "dir" only) the diffuse images
            subdirs = tuple(subdirs)[:2 if diffuse_source == "dir" else 1]
            if len(subdirs) != (2 if diffuse_source == "dir" else 1):
                raise ValueError(f"capture 'dofp' with diffuse_source {diffuse_source!r} needs the mosaic directory" +
                                 (" and the diffuse directory" if diffuse_source == "dir" else "") + f" in subdirs, got {subdirs}")
            if diffuse_source == "stokes":
                self.coef = polar.stokes_matrix(angles)
                if self.coef.shape != (3, 4):
                    raise ValueError(f"diffuse_source 'stokes' takes four angles, got {angles}")
        elif diffuse_source != "dir":
            subdirs = tuple(subdirs)[:4]
            if len(subdirs) != 4:
                raise ValueError(f"diffuse_source {diffuse_source!r} needs four view directories, got {subdirs}")
            if diffuse_source == "stokes":
                self.coef = polar.stokes_matrix(angles if angles is not None else polar.angles_from_subdirs(subdirs))
                if self.coef.shape != (3, 4):
                    raise ValueError(f"diffuse_source 'stokes' takes four angles, got {angles}")
        self.files = [list_images(os.path.join(data_dir, s), also=mosaic_extensions(dofp) if capture == "dofp" and i == 0 else ())
                      for i, s in enumerate(subdirs)]
        n = len(self.files[0])
        if any(len(f) != n for f in self.files):
            raise ValueError(f"the {len(self.files)} {'sample' if capture == 'dofp' else 'view'} directories hold different numbers of images: "
                             f"{[len(f) for f in self.files]}")
        self.select = None
        if select is not None:           # a subset: everything below (n, positions, shuffle, augmentation draws, cache keys) counts within it
            select = [int(i) for i in select]
            if select != sorted(set(select)) or (select and not 0 <= select[0] <= select[-1] < n):
                raise ValueError(f"select must be a sorted list of distinct indices into the {n} listed samples, got {select[:8]}...")
            self.select = select
            self.files = [[f[i] for i in select] for f in self.files]
            n = len(select)
        self.n = n
        if rank is None or world is None:
            rank, world = dist.rank(), dist.world_size()
        self.rank, self.world = int(rank), int(world)
        self._dev, self._stream = device, None
        self._pool = ThreadPoolExecutor(max_workers=1, thread_name_prefix="shm-loader")
        # pinned staging, two generations (a batch in preparation + the one just handed over): {(gen, view, b): uint8 [H,W,3]}
        self._pin = {}
        self._gen_event = [None, None]
        self._prepared = 0

    @property
    def dev(self):
        if self._dev is None:
            self._dev = torch.device("cuda", torch.cuda.current_device())
        return torch.device(self._dev)

    @property
    def stream(self):
        """The loader's side stream (created on first use: listing and sharding need no GPU)."""
        if self._stream is None:
            self._stream = torch.cuda.Stream(device=self.dev)
        return self._stream

    def __len__(self):
        return self.n // (self.B * self.world)

    def image_index(self, index, b):
        """Dataset position of sample b of this rank's batch `index`."""
        return (index * self.world + self.rank) * self.B + b

    def position(self, index, b, pass_index=0):
        """Index in the sorted file lists of sample b of this rank's batch `index` in pass `pass_index`."""
        return int(pass_order(self.n, self.seed, pass_index, self.shuffle)[self.image_index(index, b)])

    def _decode(self, path, key):
        from PIL import Image
        with Image.open(path) as im:
            a = np.asarray(im.convert("RGB"), dtype=np.uint8)
        buf = self._pin.get(key)
        if buf is None or tuple(buf.shape) != a.shape:
            buf = torch.empty(a.shape, dtype=torch.uint8).pin_memory()
            self._pin[key] = buf
        buf.numpy()[...] = a
        return buf

    def _decode_mosaic(self, path, key):
        """_decode for a polariser mosaic: a pinned uint8 or uint16 [h,w] buffer (polar.decode_mosaic)."""
        from . import polar
        a = polar.decode_mosaic(path, self.dofp)
        buf = self._pin.get(key)
        if buf is None or tuple(buf.shape) != a.shape or buf.numpy().dtype != a.dtype:
            buf = torch.empty(a.shape, dtype=torch.uint8 if a.dtype == np.uint8 else torch.uint16).pin_memory()
            self._pin[key] = buf
        buf.numpy()[...] = a
        return buf

    def _decode_files(self, paths, gen, b):
        """One sample's files, paths[f], decoded into this generation's pinned buffers: its four or five images, or with
        capture="dofp" its mosaic (file 0) and, for diffuse_source "dir", its diffuse image."""
        mosaic = self.capture == "dofp"
        return [self._decode_mosaic(p, (gen, f, b)) if mosaic and f == 0 else self._decode(p, (gen, f, b)) for f, p in enumerate(paths)]

    def _nfiles(self, nsrc):
        """Files behind a sample's `nsrc` (4 or 5) source images: one each, or a mosaic for the four views."""
        return nsrc - 3 if self.capture == "dofp" else nsrc

    def _stage(self, index, gen, pass_index, nsrc):
        """Decode the files behind the `nsrc` source images of every sample of the batch into this generation's pinned buffers:
        (staged[f][b], paths[f][b], the samples' positions in the sorted file lists)."""
        pos = [self.position(index, b, pass_index) for b in range(self.B)]
        paths = [[self.files[f][p] for p in pos] for f in range(self._nfiles(nsrc))]
        per_sample = [self._decode_files([paths[f][b] for f in range(len(paths))], gen, b) for b in range(self.B)]
        return [[per_sample[b][f] for b in range(self.B)] for f in range(len(paths))], paths, pos

    def _sources(self, staged, paths, b, nsrc):
        """The choke point "sample b -> its `nsrc` uint8 [h,w,3] device images", on the current (loader) stream: the decoded files
        uploaded -- or, with capture="dofp", the mosaic uploaded once and demosaiced once (shm_dofp_views: the four views in
        ascending angle), with the diffuse image behind them, which must have the demosaiced size."""
        if self.capture != "dofp":
            return [staged[v][b].to(self.dev, non_blocking=True) for v in range(nsrc)]
        srcs = list(ops.dofp_views(staged[0][b].to(self.dev, non_blocking=True), self.dofp, self.dofp_demosaic))
        if nsrc == 5:
            if tuple(staged[1][b].shape) != tuple(srcs[0].shape):
                raise ValueError("the demosaiced views and the diffuse image of a sample must have the same size: "
                                 f"{paths[0][b]} {srcs[0].shape[0]}x{srcs[0].shape[1]} ({self.dofp_demosaic}), "
                                 f"{paths[1][b]} {staged[1][b].shape[0]}x{staged[1][b].shape[1]}")
            srcs.append(staged[1][b].to(self.dev, non_blocking=True))
        return srcs

    @staticmethod
    def _same_size(staged, paths, b):
        n = len(staged)
        if any(staged[v][b].shape != staged[0][b].shape for v in range(n)):
            raise ValueError(("the four views of a sample" if n == 4 else "the four views and the diffuse image of a sample") +
                             " must have the same decoded size: " +
                             ", ".join(f"{paths[v][b]} {staged[v][b].shape[0]}x{staged[v][b].shape[1]}" for v in range(n)))

    def _prepare_worker(self, index, gen, pass_index=0):
        """Runs on the loader thread (torch's current stream is per thread): decode into this generation's pinned buffers,
        then enqueue copy + resize per image on the loader stream and record the batch's event."""
        if self._gen_event[gen] is not None:         # the copies that last read this generation's staging buffers
            self._gen_event[gen].synchronize()       # (a host wait, but on the loader thread)
        if self.cache == "device":
            return self._prepare_cached(index, gen, pass_index)
        if self.augment is not None:
            return self._prepare_augmented(index, gen, pass_index)
        if self.diffuse_source != "dir":
            return self._prepare_estimated(index, gen, pass_index)
        staged, paths, _ = self._stage(index, gen, pass_index, 5)
        with torch.cuda.device(self.dev), torch.cuda.stream(self.stream):
            # allocated, filled and consumed on the loader stream: the caching allocator hands a block back to loader-stream
            # allocations only, which are ordered behind the resize kernel that read it
            outs = [torch.empty((self.B, self.H, self.W, 3), device=self.dev) for _ in range(5)]
            for b in range(self.B):
                for v, src in enumerate(self._sources(staged, paths, b, 5)):
                    ops.resize_bilinear_u8(src, outs[v][b], 1.0 / 255.0, self.flip_ud)
            ev = torch.cuda.Event()
            ev.record(self.stream)
        self._gen_event[gen] = ev
        return tuple(outs), ev

    def _prepare_estimated(self, index, gen, pass_index=0):
        """_prepare_worker for diffuse_source "min" / "stokes": 4 B decodes and uploads, then one shm_polar_views_u8 per sample
        writes that sample's slice of all five tensors."""
        staged, paths, _ = self._stage(index, gen, pass_index, 4)
        if self.capture == "views":          # a mosaic's four views have one size by construction
            for b in range(self.B):
                self._same_size(staged, paths, b)
        with torch.cuda.device(self.dev), torch.cuda.stream(self.stream):
            outs = [torch.empty((self.B, self.H, self.W, 3), device=self.dev) for _ in range(5)]       # on the loader stream, as above
            for b in range(self.B):
                srcs = self._sources(staged, paths, b, 4)
                ops.polar_views_u8(srcs, [outs[v][b] for v in range(5)], self.diffuse_source, self.coef, 1.0 / 255.0, self.flip_ud)
            ev = torch.cuda.Event()
            ev.record(self.stream)
        self._gen_event[gen] = ev
        return tuple(outs), ev

    def _prepare_augmented(self, index, gen, pass_index):
        """_prepare_worker with `augment`, for every diffuse_source: 5 B ("dir") or 4 B decodes and uploads, then one
        shm_augment_views_u8 per sample writes that sample's slice of all five tensors with the sample's own draw.  A mirror that
        permutes the views is applied by handing the kernel the view planes in the permuted order (exact); one that does not is the
        kernel's 4x4 mix."""
        nsrc = 5 if self.diffuse_source == "dir" else 4
        staged, paths, pos = self._stage(index, gen, pass_index, nsrc)
        if self.capture == "views":          # a mosaic: _sources compares the diffuse image with the demosaiced size
            for b in range(self.B):
                self._same_size(staged, paths, b)
        kind, how = self._mirror
        with torch.cuda.device(self.dev), torch.cuda.stream(self.stream):
            outs = [torch.empty((self.B, self.H, self.W, 3), device=self.dev) for _ in range(5)]       # on the loader stream, as above
            for b in range(self.B):
                srcs = self._sources(staged, paths, b, nsrc)
                hin, win = srcs[0].shape[:2]
                p = augment_params(self.seed, pass_index, pos[b], hin, win, self.augment)
                dsts = [outs[v][b] for v in range(5)]
                if p.remap and kind == "permute":     # mirrored view i is view how[i]: source how[i] lands in plane i
                    dsts = [dsts[how.index(v)] for v in range(4)] + dsts[4:]
                ops.augment_views_u8(srcs, dsts, self.diffuse_source, self.coef, how if p.remap and kind == "mix" else None, p.crop,
                                     bool(self.flip_ud) != p.flip_ud, p.flip_lr, 1.0 / 255.0)
            ev = torch.cuda.Event()
            ev.record(self.stream)
        self._gen_event[gen] = ev
        return tuple(outs), ev

    def _sample_cache(self):
        """The arena, made on first use; its chunks are torch.uint8 tensors allocated where it is called from: the loader stream."""
        if self._cache is None:
            from .cache import SampleCache
            budget = self.cache_bytes if self.cache_bytes is not None else lambda: torch.cuda.mem_get_info(self.dev)[0] // 2
            self._cache = SampleCache(lambda nbytes: torch.empty(nbytes, dtype=torch.uint8, device=self.dev), budget)
        return self._cache

    def cache_stats(self):
        """cache.SampleCache.stats() of this loader: {"resident", "bytes", "chunks", "hits", "misses", "refused"} (zeros before the
        first batch and with cache="none")."""
        if self._cache is None:
            return {"resident": 0, "bytes": 0, "chunks": 0, "hits": 0, "misses": 0, "refused": 0}
        return self._cache.stats()

    def _prepare_cached(self, index, gen, pass_index):
        """_prepare_worker with cache="device", for every diffuse_source, with or without `augment`: a resident sample is its arena
        pointers; any other is decoded into this generation's pinned buffers and copied into its arena slot -- or, refused by the
        budget, into this generation's scratch -- on the loader stream.  Then ONE shm_augment_batch_u8 writes the batch from the
        samples' descriptors: identity crop and the fixed flip_ud without `augment` (bitwise the default path's kernels), the
        sample's draw and the permute / mix logic of _prepare_augmented with it."""
        from .cache import sample_bytes, sample_descriptor
        nsrc = 5 if self.diffuse_source == "dir" else 4
        pos = [self.position(index, b, pass_index) for b in range(self.B)]
        kind, how = self._mirror
        with torch.cuda.device(self.dev), torch.cuda.stream(self.stream):
            arena = self._sample_cache()
            outs = [torch.empty((self.B, self.H, self.W, 3), device=self.dev) for _ in range(5)]       # on the loader stream, as above
            samples = []
            for b, p in enumerate(pos):
                e = arena.lookup(p)
                if e is not None:
                    ptrs, hin, win = e.ptrs, e.hin, e.win
                else:
                    paths = [[self.files[f][p]] for f in range(self._nfiles(nsrc))]
                    staged = [[a] for a in self._decode_files([q[0] for q in paths], gen, b)]
                    if self.capture == "dofp":          # the cache holds the DEMOSAICED views: one demosaic per sample per run
                        staged = [[a] for a in self._sources(staged, paths, 0, nsrc)]
                    else:
                        self._same_size(staged, paths, 0)
                    hin, win = staged[0][0].shape[:2]
                    e = arena.store(p, nsrc, hin, win)
                    if e is not None:
                        room, offsets = arena.chunks[e.chunk], e.offsets
                    else:           # refused: this generation's scratch, free again once the generation's event has completed
                        need = sample_bytes(nsrc, hin, win)
                        room = self._scratch.get((gen, b))
                        if room is None or room.numel() < need:
                            room = self._scratch[(gen, b)] = torch.empty(need, dtype=torch.uint8, device=self.dev)
                        offsets = tuple(v * (need // nsrc) for v in range(nsrc))
                    for v in range(nsrc):
                        room[offsets[v]:offsets[v] + hin * win * 3].view(hin, win, 3).copy_(staged[v][0], non_blocking=True)
                    ptrs = tuple(room.data_ptr() + o for o in offsets)
                params = None if self.augment is None else augment_params(self.seed, pass_index, p, hin, win, self.augment)
                samples.append(sample_descriptor(ptrs, hin, win, self.flip_ud, params, self._mirror))
            ops.augment_batch_u8(samples, outs, self.diffuse_source, self.coef, how if kind == "mix" else None, 1.0 / 255.0)
            ev = torch.cuda.Event()
            ev.record(self.stream)
        self._gen_event[gen] = ev
        return tuple(outs), ev

    def prepare(self, index, pass_index=0):
        """Start batch `index` (0-based, of this rank) of pass `pass_index` on the loader thread / stream; returns a future of
        (five [B,H,W,3] tensors, ready event).  The outputs are ALLOCATED on the loader stream: a block the consumer has
        dropped is then only reused after the consumer stream's work recorded by `take()` has finished (train_step is
        fully asynchronous and reads its inputs late in the step, so allocating them on the consumer stream would let the
        next batch's resize kernels overwrite images that queued step kernels still read)."""
        gen = self._prepared & 1
        self._prepared += 1
        return self._pool.submit(self._prepare_worker, index, gen, pass_index)

    def take(self, prepared):
        """Hand a prepared batch to the current stream (waits for the loader thread's host work, not for the GPU)."""
        outs, ev = prepared.result() if hasattr(prepared, "result") else prepared
        cur = torch.cuda.current_stream()
        cur.wait_event(ev)
        for t in outs:
            t.record_stream(cur)
        return outs

    def batch(self, index, pass_index=0):
        """Batch `index` (0-based) of pass `pass_index` as five [B,H,W,3] tensors; prepared on the loader's stream."""
        return self.take(self.prepare(index, pass_index))

    def __iter__(self):
        """One batch is always in preparation on the loader thread while the previous one is consumed.  Pass e of the iteration
        is pass first_pass + e of the shuffle and the augmentation draws."""
        order = [(i, self.first_pass + e) for e in range(self.epochs) for i in range(len(self))]
        nxt = self.prepare(*order[0]) if order else None
        for j in range(len(order)):
            cur = nxt
            nxt = self.prepare(*order[j + 1]) if j + 1 < len(order) else None
            yield self.take(cur)

    def split(self, val_fraction, seed=0):
        """(train, val): two PolarDatasets over disjoint samples whose union is this one's (split_indices over the first view's stems:
        a pure function of the names, the fraction and the seed).  `train` keeps this dataset's options; `val` is a held-out set
        (held_out_options: one pass in sorted order, no augmentation, rank 0 of a world of 1).  Both renumber their samples from 0."""
        train, val = split_indices(self.files[0], val_fraction, seed)
        base = self.select if self.select is not None else list(range(self.n))
        return (PolarDataset(**self._options, select=[base[i] for i in train]),
                PolarDataset(**held_out_options(self._options), select=[base[i] for i in val]))


def split_indices(files, val_fraction, seed=0):
    """(train, val): the sorted positions in `files` (one view's file list) of the two parts of split_names over the files' stems."""
    at = {Path(f).stem: i for i, f in enumerate(files)}
    train, val = split_names([Path(f).stem for f in files], val_fraction, seed)           # two files with one stem raise there
    return sorted(at[s] for s in train), sorted(at[s] for s in val)


def held_out_options(options):
    """PolarDataset options of a held-out (validation) loader next to a training loader with `options`: the same images, size, batch
    size, orientation, diffuse source, angles and cache; ONE pass in sorted order without augmentation; and rank 0 of a world of 1
    EXPLICITLY, whatever torch.distributed says -- every rank scores the whole held-out set (the kernels are deterministic, so all get
    the same numbers), which needs no collective, so a slow rank cannot hang its peers."""
    return dict(options, shuffle=False, augment=None, epochs=1, first_pass=0, rank=0, world=1)


def validation_loader(data_dir, image_size, batch_size, *, val_dir="", val_fraction=0.0, val_seed=0, val_batch_size=None, subdirs=PSD_SUBDIRS,
                      flip_ud=True, device=None, diffuse_source="dir", angles=None, cache="none", cache_bytes=None, capture="views", dofp=None,
                      dofp_demosaic="bilinear"):
    """The held-out loader of `train()` from plain options (no trainer, no GPU needed to build it), or None with both sources off:
    `val_dir` = a directory laid out like data_dir, `val_fraction` = that part of data_dir (split_indices with val_seed; datasetLoad
    then trains on the rest).  Giving both raises ValueError.  The other options are the training loader's (held_out_options says what a
    held-out loader does with them); val_batch_size defaults to batch_size.  Only full batches are yielded: len() = n // val_batch_size."""
    if val_dir and val_fraction:
        raise ValueError(f"val_dir ({val_dir!r}) and val_fraction ({val_fraction}) are two sources of one held-out set: give one of them")
    if not val_dir and not val_fraction:
        return None
    B = int(batch_size if val_batch_size is None else val_batch_size)
    if B < 1:
        raise ValueError(f"val_batch_size {val_batch_size!r} < 1")
    opts = held_out_options(dict(image_size=image_size, batch_size=B, subdirs=tuple(subdirs), flip_ud=flip_ud, device=device,
                                 diffuse_source=diffuse_source, angles=angles, seed=0, cache=cache, cache_bytes=cache_bytes,
                                 capture=capture, dofp=dofp, dofp_demosaic=dofp_demosaic))
    if val_dir:
        return PolarDataset(val_dir, **opts)
    _, val = split_indices(list_images(os.path.join(data_dir, tuple(subdirs)[0]), also=mosaic_extensions(dofp) if capture == "dofp" else ()),
                           val_fraction, val_seed)
    return PolarDataset(data_dir, **opts, select=val)


def trainer_frame(trainer):
    """The frame a trainer's loaders produce: its frame_arg() (the side, or the image_hw pair), or image_size of a plain options
    object that has no such method."""
    frame = getattr(trainer, "frame_arg", None)
    return frame() if callable(frame) else trainer.image_size


DEVELOP_OPTIONS = ("dofp_black", "dofp_white", "dofp_wb", "dofp_ccm", "dofp_tone", "dofp_sat")       # polar.DofpDevelop's fields; all None = no development
CALIBRATION_OPTIONS = ("dofp_calibration",)       # the path of a saved polar.DofpCalibration; None = the frames are read as they are
BRACKET_OPTIONS = ("dofp_exposures", "dofp_bracket_black", "dofp_bracket_white")       # polar.DofpBracket's fields; dofp_exposures None = one exposure per sample
CAPTURE_OPTIONS = ("capture_format", "dofp_dir", "dofp_pattern", "dofp_quad_angles", "dofp_bits", "dofp_demosaic") + DEVELOP_OPTIONS + BRACKET_OPTIONS + CALIBRATION_OPTIONS


def capture_options(args, subdirs=PSD_SUBDIRS):
    """The capture options of a trainer's `args` as (subdirs, loader keywords): capture_format "views" (default: `subdirs` and
    today's loader) or "dofp" = a polariser-mosaic sensor, whose frames lie in dofp_dir ("DOFP") next to the diffuse directory
    (the last of `subdirs`) and are laid out as polar.DofpLayout(dofp_pattern, dofp_quad_angles, dofp_bits) says; dofp_demosaic
    "bilinear" / "bin".  dofp_black, dofp_white, dofp_wb, dofp_ccm, dofp_tone, dofp_sat: when at least one of them is given (not
    None) the layout carries polar.DofpDevelop(black, white, wb, ccm, tone, sat) and the frames are developed inside the demosaic
    launch; the development rides on the layout, so the loader keywords stay the three they were (given with capture_format "views",
    where nothing could carry it, it is refused).  dofp_calibration: the path of the sensor's calibration (polar.build_calibration(...)
    .save(path); a polar.DofpCalibration itself is taken too): it is loaded here and rides on the layout in the same way, so every
    frame is corrected on the device before it is demosaiced; refused with capture_format "views" like the development.
    dofp_exposures (with dofp_bracket_black, dofp_bracket_white): the layout carries polar.DofpBracket(exposures, black, white): a sample
    is one multi-page TIFF of that many exposures, merged on the device before it is demosaiced; refused with capture_format "views",
    and the two levels are refused without dofp_exposures.  An unknown
    value raises ValueError naming the option, before anything is listed or allocated."""
    from . import polar
    opt = lambda k, dflt: getattr(args, k, dflt)
    capture, demosaic = opt("capture_format", "views"), opt("dofp_demosaic", "bilinear")
    if capture not in polar.CAPTURES:
        raise ValueError(f"capture_format {capture!r} is not one of {polar.CAPTURES}")
    if demosaic not in polar.DOFP_DEMOSAIC:
        raise ValueError(f"dofp_demosaic {demosaic!r} is not one of {polar.DOFP_DEMOSAIC}")
    given = {k[5:]: opt(k, None) for k in DEVELOP_OPTIONS if opt(k, None) is not None}
    calibration = opt("dofp_calibration", None)
    bracket = {k: opt(k, None) for k in BRACKET_OPTIONS if opt(k, None) is not None}
    if capture == "views":
        if calibration is not None:
            raise ValueError(f"dofp_calibration {calibration!r} needs capture_format 'dofp', got 'views'")
        for k, v in bracket.items():
            raise ValueError(f"{k} {v!r} needs capture_format 'dofp', got 'views'")
        for k, v in given.items():          # it would be ignored: a development is a property of a mosaic's layout
            raise ValueError(f"dofp_{k} {v!r} needs capture_format 'dofp', got 'views'")
        return tuple(subdirs), dict(capture="views", dofp=None, dofp_demosaic=demosaic)
    try:
        develop = polar.DofpDevelop(**given) if given else None
        if calibration is not None and not isinstance(calibration, polar.DofpCalibration):
            if not isinstance(calibration, (str, os.PathLike)):
                raise ValueError(f"DofpLayout: calibration {calibration!r} is not the path of a saved polar.DofpCalibration")
            calibration = polar.DofpCalibration.load(calibration)
        for k, v in bracket.items():
            if "dofp_exposures" not in bracket:
                raise ValueError(f"{k} {v!r} needs dofp_exposures: it is a level of the bracket's merge")
        if bracket:
            bracket = polar.DofpBracket(bracket["dofp_exposures"], bracket.get("dofp_bracket_black"), bracket.get("dofp_bracket_white"))
        layout = polar.DofpLayout(opt("dofp_pattern", "mono"), opt("dofp_quad_angles", (90, 45, 135, 0)), opt("dofp_bits", 8), develop, calibration,
                                  bracket or None)
    except ValueError as e:
        msg = str(e).replace("DofpLayout: bracket ", "dofp_bracket_", 1).replace("DofpBracket: exposures", "dofp_exposures", 1)
        msg = msg.replace("DofpBracket: ", "dofp_bracket_", 1)
        raise ValueError(msg.replace("DofpLayout: ", "dofp_", 1).replace("DofpDevelop: ", "dofp_", 1).replace("DofpCalibration: ", "dofp_calibration: ", 1)) from None
    dofp_dir = opt("dofp_dir", "DOFP")
    if not isinstance(dofp_dir, str) or not dofp_dir:
        raise ValueError(f"dofp_dir {dofp_dir!r} is not a directory name")
    return (dofp_dir, tuple(subdirs)[-1]), dict(capture="dofp", dofp=layout, dofp_demosaic=demosaic)


def datasetLoad(trainer, subdirs=PSD_SUBDIRS, flip_ud=True):
    """Reference signature (datasetLoader.py:19): returns (length_dataset, loadedDataset) and sets the same
    attributes on the trainer object.  The trainer's `diffuse_source` option (default "dir") goes to PolarDataset; it is NOT
    keyed on the reference's `est_diffuse`, which main.py's parser makes True for every run.  `shuffle`, `data_seed`
    and `aug_flip_lr` / `aug_flip_ud` / `aug_crop_min` / `aug_views` become the loader's shuffle, seed and Augment; `cache` ("none" /
    "device") and `cache_gb` (GiB of device memory the cache may take; None = half of what is free) its cache and cache_bytes.
    `val_dir` / `val_fraction` (with `val_seed`, `val_batch_size`) set trainer.valDataset (validation_loader; None when both are off);
    with `val_fraction` the returned loader and length are those of the training part.  `capture_format` = "dofp" with `dofp_dir`,
    `dofp_pattern`, `dofp_quad_angles`, `dofp_bits` and `dofp_demosaic` (capture_options) reads a polariser-mosaic capture instead."""
    opt = lambda k, dflt: getattr(trainer.args, k, dflt)
    subdirs, capture = capture_options(trainer.args, subdirs)
    draws = (float(opt("aug_flip_lr", 0.0)), float(opt("aug_flip_ud", 0.0)), float(opt("aug_crop_min", 1.0)))
    # no augmentation asked for: the loader's default path, not the augmenting kernel at identity parameters
    augment = Augment(*draws, views=opt("aug_views", "physical")) if draws != (0.0, 0.0, 1.0) else None
    cache = dict(cache=opt("cache", "none"), cache_bytes=gib_to_bytes(opt("cache_gb", None)))
    source = dict(capture, diffuse_source=getattr(trainer.args, "diffuse_source", "dir"))
    # held-out validation (`val_dir` / `val_fraction`, both off by default): the loader train() validates on, and with val_fraction
    # the training loader is the rest of data_dir
    val_dir, val_fraction, val_seed = opt("val_dir", ""), float(opt("val_fraction", 0.0) or 0.0), int(opt("val_seed", 0))
    trainer.valDataset = validation_loader(trainer.data_dir, trainer_frame(trainer), trainer.batch_size, val_dir=val_dir, val_fraction=val_fraction,
                                           val_seed=val_seed, val_batch_size=opt("val_batch_size", None), subdirs=subdirs, flip_ud=flip_ud,
                                           device=trainer.device, **source, **cache)
    select = None
    if val_fraction:
        select, _ = split_indices(list_images(os.path.join(trainer.data_dir, tuple(subdirs)[0]),
                                              also=mosaic_extensions(capture["dofp"]) if capture["capture"] == "dofp" else ()), val_fraction, val_seed)
    ds = PolarDataset(trainer.data_dir, trainer_frame(trainer), trainer.batch_size, subdirs, flip_ud, trainer.device,
                      epochs=trainer.num_epochs, shuffle=bool(opt("shuffle", False)), augment=augment, seed=int(opt("data_seed", 0)),
                      select=select, **source, **cache)
    trainer.stddev_arr, trainer.mean_arr, trainer.variance_arr = [], [], []
    # per-rank length: batches_per_epoch = length // batch_size (SHM.py:957) then counts this rank's batches
    trainer.length_dataset, trainer.loadedDataset = ds.n // ds.world, ds
    return trainer.length_dataset, ds


def split_names(names, val_fraction, seed=0):
    """(train, val): two sorted, disjoint lists whose union is `names`, a pure function of the sorted names, the fraction and the
    seed: val is the round(N * val_fraction) names at the first places of default_rng(seed).permutation(N) over the sorted names.
    A fraction outside (0, 1), or one that would leave either side empty, raises ValueError.  No torch call."""
    names = sorted(names)
    n = len(names)
    if len(set(names)) != n:
        raise ValueError("split_names: the names are not distinct")
    if not isinstance(val_fraction, (int, float)) or not 0.0 < float(val_fraction) < 1.0:
        raise ValueError(f"split: val_fraction {val_fraction!r} is not a fraction in (0, 1)")
    n_val = int(round(n * float(val_fraction)))
    if n_val < 1 or n_val >= n:
        raise ValueError(f"split: val_fraction {val_fraction} of {n} samples leaves {n - n_val} for training and {n_val} for validation; "
                         f"both sides need at least one")
    val = set(int(i) for i in np.random.default_rng(int(seed)).permutation(n)[:n_val])
    return [names[i] for i in range(n) if i not in val], [names[i] for i in range(n) if i in val]


class MaskDataset:
    """Image / mask pairs for SpecSeg training (SpecSeg.fit, trainer.train_specseg): the files of `image_dir` and `mask_dir` are
    paired by name (the stem, whatever the extension; a file without its partner raises).  Images are decoded to RGB, resized with
    shm_resize_bilinear_u8 (the training loader's kernel), and go through shm_rgb2yuv_std; the standardised Y plane is kept --
    exactly what train_step feeds `SpecSeg.predict`.  Masks are decoded to one channel, resized the same way and divided by 255:
    soft values at the resized edges, not thresholded.  flip_ud flips image and mask alike.  The whole set is held on the device
    ([N,S,S,1] each): mask sets are small next to the polarimetric data.

    augment (a data.Augment) / shuffle / seed: the train-time loader of PolarDataset for pairs.  With either
    set, `batch(index, pass_index)` makes (x, y) with ONE ops.augment_pairs_u8 call from the pairs' decoded bytes: the order of the
    pass is pass_order(N, seed, pass_index, shuffle), the draw of the sample at sorted position p is augment_params(seed, pass_index,
    p, hin, win, augment), and image and mask get the same crop and mirrors.  The bytes (for the polar source: view 2 and the
    finished mask) stay on the device in a cache.SampleCache arena of at most cache_bytes (default: half of the free device memory
    when the first pair is stored); a pair that does not fit is decoded -- and its polar mask recomputed -- every time it comes up.
    Image and mask of a pair must then have one decoded size.  Without both options nothing changes: tensors() and iteration make
    the calls described above, and batch() slices tensors()."""

    def __init__(self, image_dir, mask_dir, image_size, batch_size=1, flip_ud=False, device=None, augment=None, shuffle=False, seed=0,
                 cache_bytes=None):
        imgs = {Path(p).stem: p for p in list_images(image_dir)}
        masks = {Path(p).stem: p for p in list_images(mask_dir)}
        if set(imgs) != set(masks) or not imgs:
            raise ValueError(f"{image_dir} and {mask_dir} must hold the same, non-empty set of names; without a partner: "
                             f"{sorted(set(imgs) ^ set(masks))[:8]}")
        self.names = sorted(imgs)
        self.files = [(imgs[n], masks[n]) for n in self.names]
        self.S, self.B, self.flip_ud, self._dev, self._xy = int(image_size), int(batch_size), bool(flip_ud), device, None
        self._polar = None
        self._loader_options(augment, shuffle, seed, cache_bytes, None)

    @classmethod
    def from_polar(cls, data_dir, image_size, batch_size=1, subdirs=PSD_SUBDIRS, angles=None, flip_ud=False, device=None, augment=None,
                   shuffle=False, seed=0, cache_bytes=None, capture="views", dofp=None, dofp_demosaic="bilinear", **mask_options):
        """The same (x, y) tensors from a raw four-directory capture, without a mask anybody drew and without the PNG round trip:
        the image of sample i is its view subdirs[2] (the one whose Y plane train_step feeds SpecSeg.predict), the mask is
        polar.specular_mask of its four views (`angles`, or those read from the directory names; `mask_options` = threshold, floor,
        open_radius, dilate_radius), computed at source size and then resized like a decoded mask file.  Bit-equal to
        polar.write_specular_masks(data_dir, out) followed by MaskDataset(<data_dir>/<subdirs[2]>, out, ...): PNG is lossless.
        Same refusals as write_specular_masks: four directories, equal counts, equal sizes.
        augment / shuffle / seed / cache_bytes as the directory form.  The mask is mirror-invariant (S2 only changes sign), but the
        image is view 2: with augment.views == "physical" and a mirror probability above zero, the angles must be such that a
        mirror leaves view 2 in place (polar.mirror_keeps_view: true for 0/45/90/135 and 0/60/90/150), else ValueError.
        capture="dofp" (with dofp = a polar.DofpLayout and dofp_demosaic): the first of `subdirs` holds one polariser mosaic per
        sample; its four demosaiced views (polar.sample_views, in ascending angle) take the place of the four files, the angles
        default to the layout's and the names are the mosaics' stems."""
        from . import polar
        polar.check_capture(capture, dofp, dofp_demosaic, "MaskDataset.from_polar")
        bad = sorted(set(mask_options) - set(polar.MASK_OPTIONS))
        if bad:
            raise TypeError(f"MaskDataset.from_polar: unknown option(s) {bad}; polar.specular_mask takes {polar.MASK_OPTIONS}")
        views, files = polar.polar_sample_files(data_dir, subdirs, "MaskDataset.from_polar", capture, dofp)
        if not files[0]:
            raise ValueError(f"{data_dir}: the view directories {views} hold no images")
        self = cls.__new__(cls)
        named = 2 if capture == "views" else 0          # the file a sample is named after: its image (view 2), or its mosaic
        self.files = sorted(zip(*files), key=lambda paths: Path(paths[named]).stem)      # the order of the directory form: by name
        self.names = [Path(paths[named]).stem for paths in self.files]
        self.S, self.B, self.flip_ud, self._dev, self._xy = int(image_size), int(batch_size), bool(flip_ud), device, None
        ang = list(angles if angles is not None else dofp.angles if capture == "dofp" else polar.angles_from_subdirs(views))
        self._polar = dict(coef=polar.stokes_matrix(ang), options=dict(mask_options), capture=(capture, dofp, dofp_demosaic))
        self._loader_options(augment, shuffle, seed, cache_bytes, ang)
        return self

    def _loader_options(self, augment, shuffle, seed, cache_bytes, angles):
        if augment is not None and not isinstance(augment, Augment):
            raise ValueError(f"augment must be a data.Augment or None, got {augment!r}")
        if cache_bytes is not None and (not isinstance(cache_bytes, int) or cache_bytes < 0):
            raise ValueError(f"cache_bytes {cache_bytes!r} is not a byte count")
        if angles is not None and augment is not None and augment.views == "physical" and (augment.flip_lr > 0 or augment.flip_ud > 0):
            from . import polar
            if not polar.mirror_keeps_view(angles, 2):
                raise ValueError(f"MaskDataset.from_polar: a mirror does not leave view 2 (the image) of the angles {list(angles)} in place, so a "
                                 f"mirrored pair is not one this capture could have produced; use Augment(views=\"keep\") for the plain "
                                 f"geometric flip, or no mirror")
        self.augment, self.shuffle, self.seed, self.cache_bytes = augment, bool(shuffle), int(seed), cache_bytes
        self.first_pass = 0
        self._cache, self._ws = None, None

    @property
    def active(self):
        """Whether batches are made from the decoded bytes by ops.augment_pairs_u8 (augment or shuffle set)."""
        return self.augment is not None or self.shuffle

    def _pair(self, k):
        """Sample k as decoded bytes on the device: (uint8 [h,w,3] image, uint8 [h,w,1] mask)."""
        if self._polar is None:
            fi, fm = self.files[k]
            return self._decode(fi, "RGB").to(self.dev), self._decode(fm, "L").to(self.dev)
        from . import polar
        srcs = polar.sample_views(self.files[k], k, self.dev, *self._polar["capture"])
        with torch.cuda.device(self.dev):
            mask, _, _ = polar.specular_mask(srcs, matrix=self._polar["coef"], **self._polar["options"])
        return srcs[2], mask.unsqueeze(2)

    @property
    def dev(self):
        if self._dev is None:
            self._dev = torch.device("cuda", torch.cuda.current_device())
        return torch.device(self._dev)

    def __len__(self):
        return -(-len(self.files) // self.B)

    @staticmethod
    def _decode(path, mode):
        from PIL import Image
        with Image.open(path) as im:
            a = np.asarray(im.convert(mode), dtype=np.uint8)
        return torch.from_numpy(np.ascontiguousarray(a.reshape(a.shape[0], a.shape[1], -1)))

    def tensors(self):
        """(x, y): the standardised Y planes and the masks, float32 [N,S,S,1] on the device (loaded once), in sorted order and
        without augmentation, whatever the loader options."""
        if self._xy is None:
            N, S = len(self.files), self.S
            rgb = torch.empty((N, S, S, 3), device=self.dev)
            y = torch.empty((N, S, S, 1), device=self.dev)
            for k in range(N):
                img, mask = self._pair(k)
                ops.resize_bilinear_u8(img, rgb[k], 1.0 / 255.0, self.flip_ud)
                ops.resize_bilinear_u8(mask, y[k], 1.0 / 255.0, self.flip_ud)
            yuv = torch.empty_like(rgb)
            acc = torch.zeros(2 * N, dtype=torch.float64, device=self.dev)
            scale = torch.empty(N, device=self.dev)
            ops.rgb2yuv_std(rgb, yuv, acc, scale, N, S * S)
            self._xy = (yuv[..., 0:1].contiguous(), y)
        return self._xy

    def cache_stats(self):
        """cache.SampleCache.stats() of the pair arena: {"resident", "bytes", "chunks", "hits", "misses", "refused"} (zeros before the
        first batch made from bytes, and always without augment / shuffle)."""
        if self._cache is None:
            return {"resident": 0, "bytes": 0, "chunks": 0, "hits": 0, "misses": 0, "refused": 0}
        return self._cache.stats()

    def _resident(self, p):
        """The pair at sorted position p as (image address, mask address, hin, win, what keeps the bytes alive): from the arena, or
        decoded now and -- where the budget holds it -- copied into its arena slot (two images per sample; the mask takes the
        first hin * win bytes of the second)."""
        if self._cache is None:
            from .cache import SampleCache
            budget = self.cache_bytes if self.cache_bytes is not None else lambda: torch.cuda.mem_get_info(self.dev)[0] // 2
            self._cache = SampleCache(lambda nbytes: torch.empty(nbytes, dtype=torch.uint8, device=self.dev), budget)
        e = self._cache.lookup(p)
        if e is not None:
            return e.ptrs[0], e.ptrs[1], e.hin, e.win, None
        img, mask = self._pair(p)
        hin, win = int(img.shape[0]), int(img.shape[1])
        if tuple(mask.shape[:2]) != (hin, win):
            raise ValueError(f"image and mask of a pair must have the same decoded size to be augmented together: {self.files[p][0]} is "
                             f"{hin}x{win}, {self.files[p][-1]} {mask.shape[0]}x{mask.shape[1]}")
        img, mask = img.contiguous(), mask.contiguous()
        e = self._cache.store(p, 2, hin, win)
        if e is None:                   # refused by the budget: these tensors are the sources, for this batch only
            return img.data_ptr(), mask.data_ptr(), hin, win, (img, mask)
        room = self._cache.chunks[e.chunk]
        room[e.offsets[0]:e.offsets[0] + hin * win * 3].view(hin, win, 3).copy_(img)
        room[e.offsets[1]:e.offsets[1] + hin * win].view(hin, win).copy_(mask.view(hin, win))
        return e.ptrs[0], e.ptrs[1], hin, win, None

    def positions(self, index, pass_index=0):
        """Sorted positions of the samples of batch `index` in pass `pass_index`; the last batch of a pass holds N mod B samples
        when that is not zero."""
        order = pass_order(len(self.files), self.seed, pass_index, self.shuffle)
        return [int(p) for p in order[index * self.B:(index + 1) * self.B]]

    def batch(self, index, pass_index=0):
        """(x, y) of batch `index` of pass `pass_index`, float32 [b,S,S,1] each.  With augment or shuffle: one ops.augment_pairs_u8
        call on the current stream.  Without: slices of tensors()."""
        if not 0 <= index < len(self):
            raise IndexError(f"batch {index} of {len(self)}")
        if not self.active:
            x, y = self.tensors()
            return x[index * self.B:(index + 1) * self.B], y[index * self.B:(index + 1) * self.B]
        from .cache import AugSample
        pos = self.positions(index, pass_index)
        with torch.cuda.device(self.dev):
            samples, keep = [], []
            for p in pos:
                iptr, mptr, hin, win, alive = self._resident(p)
                keep.append(alive)
                if self.augment is None:
                    samples.append(AugSample((iptr, mptr), hin, win, None, self.flip_ud, False))
                else:
                    d = augment_params(self.seed, pass_index, p, hin, win, self.augment)
                    samples.append(AugSample((iptr, mptr), hin, win, d.crop, self.flip_ud != d.flip_ud, d.flip_lr))
            x = torch.empty((len(pos), self.S, self.S, 1), device=self.dev)
            y = torch.empty_like(x)
            need = ops.augment_pairs_ws_doubles(len(pos), self.S, self.S)
            if self._ws is None or self._ws.numel() < need:
                self._ws = torch.empty(ops.augment_pairs_ws_doubles(self.B, self.S, self.S), dtype=torch.float64, device=self.dev)
            ops.augment_pairs_u8(samples, x, y, self._ws)
        return x, y

    def __iter__(self):
        if self.active:
            for i in range(len(self)):
                yield self.batch(i, self.first_pass)
            return
        x, y = self.tensors()
        for b0 in range(0, len(self.files), self.B):
            yield x[b0:b0 + self.B], y[b0:b0 + self.B]

    def _subset(self, names, augment, shuffle):
        import copy
        want = set(names)
        sub = copy.copy(self)
        sub.files = [f for n, f in zip(self.names, self.files) if n in want]
        sub.names = [n for n in self.names if n in want]
        sub.augment, sub.shuffle = augment, bool(shuffle)
        sub._xy = sub._cache = sub._ws = None
        return sub

    def split(self, val_fraction, seed=0):
        """(train, val): two datasets over disjoint name sets whose union is this one's (split_names: a pure function of the sorted
        names, the fraction and the seed).  `train` keeps this dataset's options; `val` has no augmentation and no shuffle."""
        train, val = split_names(self.names, val_fraction, seed)
        return self._subset(train, self.augment, self.shuffle), self._subset(val, None, False)


DOFP_TEST_VIEWS = ("total", 0, 1, 2, 3)       # the demosaiced plane test mode reads of a mosaic: the reference feeds "I0 (or Itot)"


class _MosaicArray(np.ndarray):
    """A decoded mosaic as _EvalCapture hands it on: the [n,h,w] pages of a bracket are three-dimensional like an RGB photo, so the class
    and not the rank says which of the two an array is."""


class _EvalCapture:
    """What test mode reads as a photo's decoded bytes (the capture options of EvalDataset and NativeEvalDataset): the RGB file, or
    with capture="dofp" one plane of a polariser mosaic -- dofp_test_view "total" (the rounded mean of the four views, default) or
    the view 0..3 in ascending angle -- which then stands wherever the decoded photo stands.  The host side (decode, size) runs on
    the worker thread; `photo` uploads, and demosaics on the current stream."""

    def __init__(self, capture, dofp, dofp_demosaic, dofp_test_view, who):
        from . import polar
        polar.check_capture(capture, dofp, dofp_demosaic, who)
        if dofp_test_view not in DOFP_TEST_VIEWS or isinstance(dofp_test_view, bool):
            raise ValueError(f"{who}: dofp_test_view {dofp_test_view!r} is not one of {DOFP_TEST_VIEWS}")
        self.mosaic, self.dofp, self.demosaic, self.view = capture == "dofp", dofp, dofp_demosaic, dofp_test_view

    def decode(self, path):
        """(decoded array, (h, w) of the photo it stands for)."""
        if not self.mosaic:
            a = EvalDataset._decode(path)
            return a, a.shape[:2]
        from . import polar
        a = polar.decode_mosaic(path, self.dofp).view(_MosaicArray)          # [h,w], or the [n,h,w] pages of a bracketed layout
        return a, self.dofp.view_shape(a.shape[-2], a.shape[-1], self.demosaic)

    def size(self, h, w):
        """(h, w) of the photo a file of h x w pixels stands for."""
        return self.dofp.view_shape(h, w, self.demosaic) if self.mosaic else (h, w)

    def photo(self, a, dev):
        """The uint8 [h,w,3] device image of a decoded test file."""
        if a.ndim == 3 and not isinstance(a, _MosaicArray):
            return torch.from_numpy(a).to(dev)
        from . import polar
        with torch.cuda.device(dev):
            out = polar.demosaic(np.asarray(a), self.dofp, self.demosaic, total=self.view == "total", device=dev)
        return out[4 if self.view == "total" else self.view]


def eval_file_lists(test_dir, diffuse_dir=None, also=()):
    """File lists of the evaluation loader: the sorted flat `test_dir` (with the extensions `also`: mosaic_extensions of a bracketed
    layout) and, when given, the sorted flat `diffuse_dir` (None otherwise), paired by position.  The reference zips the two datasets (test.py:130), and tf.data's zip stops at the
    shorter one without a word; a count mismatch here raises instead, since it means the pairs are not what was meant."""
    test = list_images(test_dir, also=also)
    if not diffuse_dir:
        return test, None
    diffuse = list_images(diffuse_dir)
    if len(diffuse) != len(test):
        raise ValueError(f"{test_dir} holds {len(test)} images and {diffuse_dir} {len(diffuse)}: the evaluation pairs them by "
                         f"sorted position and needs the same number in both")
    return test, diffuse


class EvalDataset:
    """The test-mode loader (test.py:80-137): batches of ([b,S,S,3] test images, [b,S,S,3] diffuse images or None), float32
    device tensors in [0,1], b = batch_size except for a partial last batch -- every image is yielded once, in sorted order.

    Same decode and resize as PolarDataset (PIL, then shm_resize_bilinear_u8 scaled by 1/255) but NO flip: test.py:93,118 map
    only x / 255.  `sources(index)` gives each test image's path and (h, w) before the resize (the image export writes at that
    size).  Evaluation is not sharded: rank 0 of a world of 1, whatever torch.distributed says.  The next batch is decoded
    on a worker thread while the current one is consumed; uploads and resizes run on the consumer's current stream.
    keep_source=True leaves the last batch's decoded bytes on the device in `last_source` (the full-resolution output of
    evaluate.test reads the photos there); what the iterator yields is the same either way.
    capture="dofp" (with dofp = a polar.DofpLayout, dofp_demosaic, dofp_test_view = "total" | 0..3): test_dir holds polariser
    mosaics, and the chosen demosaiced plane (_EvalCapture) stands wherever the decoded photo stands: the resize, the sizes of
    sources() and last_source."""

    def __init__(self, test_dir, image_size, batch_size=1, diffuse_dir=None, device=None, keep_source=False, capture="views", dofp=None,
                 dofp_demosaic="bilinear", dofp_test_view="total"):
        self._capture = _EvalCapture(capture, dofp, dofp_demosaic, dofp_test_view, "EvalDataset")
        if batch_size < 1:
            raise ValueError(f"batch_size {batch_size} < 1")
        self.H, self.W = frame_hw(image_size)                # image_size: a side, or a pair (H, W)
        self.S, self.B = (self.H if self.H == self.W else None), int(batch_size)
        self.test_files, self.diffuse_files = eval_file_lists(test_dir, diffuse_dir, mosaic_extensions(dofp) if capture == "dofp" else ())
        self.n = len(self.test_files)
        self.rank, self.world = 0, 1
        self._dev = device
        self._pool = ThreadPoolExecutor(max_workers=1, thread_name_prefix="shm-eval-loader")
        self._sizes = {}             # dataset position -> (h, w) of the decoded test image, filled by the decode
        # keep_source: the decoded bytes of the last batch, as uploaded before the resize, stay reachable: (test, diffuse), each a list
        # of uint8 device tensors [h,w,3] in batch order (diffuse None without a diffuse_dir).  Off: they are temporaries, nothing is kept
        self.keep_source, self.last_source = bool(keep_source), None

    @property
    def dev(self):
        if self._dev is None:
            self._dev = torch.device("cuda", torch.cuda.current_device())
        return torch.device(self._dev)

    def __len__(self):
        return (self.n + self.B - 1) // self.B

    def batch_range(self, index):
        """Dataset positions [lo, hi) of batch `index`."""
        lo = index * self.B
        return lo, min(lo + self.B, self.n)

    @staticmethod
    def _decode(path):
        from PIL import Image
        with Image.open(path) as im:
            return np.array(im.convert("RGB"), dtype=np.uint8)

    def _decode_batch(self, index):
        lo, hi = self.batch_range(index)
        test = []
        for i, p in enumerate(self.test_files[lo:hi]):
            a, self._sizes[lo + i] = self._capture.decode(p)
            test.append(a)
        diffuse = None if self.diffuse_files is None else [self._decode(p) for p in self.diffuse_files[lo:hi]]
        return test, diffuse

    def _upload(self, decoded, kept=None):
        out = torch.empty((len(decoded), self.H, self.W, 3), dtype=torch.float32, device=self.dev)
        for b, a in enumerate(decoded):
            src = self._capture.photo(a, self.dev)
            if kept is not None:
                kept.append(src)
            ops.resize_bilinear_u8(src, out[b], 1.0 / 255.0, False)
        return out

    def sources(self, index):
        """(path, (h, w)) of every test image of batch `index`: the file and its size before the resize (the image export
        writes at that size).  The sizes come from the decode, so this is free once the batch has been loaded."""
        lo, hi = self.batch_range(index)
        out = []
        for i in range(lo, hi):
            if i not in self._sizes:
                from PIL import Image
                with Image.open(self.test_files[i]) as im:
                    self._sizes[i] = self._capture.size(im.size[1], im.size[0])
            out.append((self.test_files[i], tuple(int(v) for v in self._sizes[i])))
        return out

    def batch(self, index, decoded=None):
        test, diffuse = decoded if decoded is not None else self._decode_batch(index)
        if not self.keep_source:
            return self._upload(test), (None if diffuse is None else self._upload(diffuse))
        kept = ([], None if diffuse is None else [])
        out = self._upload(test, kept[0]), (None if diffuse is None else self._upload(diffuse, kept[1]))
        self.last_source = kept
        return out

    def __iter__(self):
        nxt = self._pool.submit(self._decode_batch, 0) if len(self) else None
        for i in range(len(self)):
            cur = nxt.result()
            nxt = self._pool.submit(self._decode_batch, i + 1) if i + 1 < len(self) else None
            yield self.batch(i, cur)


# ---------------------------------------------------------------------------------------------------------------------
# Native-resolution test mode (evaluate.test(eval_size="native")): a photo runs at its own h x w.  The networks pool four times,
# so the frame they see has sides that are multiples of 16; THIS is the one place that says how a photo becomes such a frame.
FRAME_MULTIPLE = 16          # four 2 x 2 pools (generator and SpecSeg)
MIN_NATIVE_SIDE = 32         # the deepest map is then 2 x 2, and a pad of at most 15 stays inside the image (reflection needs pad <= side - 1)


def pad_geometry(h, w):
    """(Hp, Wp, top, left) of the frame of an h x w photo: Hp = ceil16(h), Wp = ceil16(w), the photo centred with the odd pixel
    of the pad below / to the right: top = (Hp - h) // 2, left = (Wp - w) // 2.  The border is filled by reflection without
    repeating the edge sample (NumPy's mode="reflect"; shm_load_pad_u8).  Standardisation, SpecSeg and the generator see the
    frame; metrics and export see the window (top, left, h, w).  A side below MIN_NATIVE_SIDE raises ValueError."""
    h, w = int(h), int(w)
    if h < MIN_NATIVE_SIDE or w < MIN_NATIVE_SIDE:
        raise ValueError(f"native-resolution evaluation takes images of at least {MIN_NATIVE_SIDE} x {MIN_NATIVE_SIDE} pixels, got {h} x {w}")
    m = FRAME_MULTIPLE
    hp, wp = (h + m - 1) // m * m, (w + m - 1) // m * m
    return hp, wp, (hp - h) // 2, (wp - w) // 2


class NativeEvalDataset:
    """The test-mode loader at each photo's own resolution: per image (frame [1,Hp,Wp,3], target [1,h,w,3] or None, window
    (top, left, h, w)), float32 device tensors in [0,1].  Same file listing and pairing as EvalDataset (eval_file_lists), same
    decode (PIL on a worker thread, one image ahead); the frame is ONE shm_load_pad_u8 call on the decoded bytes (pad_geometry),
    the diffuse target is uploaded tight (the same call without a pad).  Batch size is 1: sizes differ per image.
    check(path, h, w): called after the decode and before anything is allocated or launched for the image (evaluate.test refuses
    images over its limits there).  A diffuse partner of another size than its test image raises ValueError naming both files.
    capture="dofp": as EvalDataset; the photo's size, the one the diffuse partner must have, is the demosaiced plane's."""

    def __init__(self, test_dir, diffuse_dir=None, device=None, check=None, capture="views", dofp=None, dofp_demosaic="bilinear",
                 dofp_test_view="total"):
        self._capture = _EvalCapture(capture, dofp, dofp_demosaic, dofp_test_view, "NativeEvalDataset")
        self.B = 1
        self.test_files, self.diffuse_files = eval_file_lists(test_dir, diffuse_dir, mosaic_extensions(dofp) if capture == "dofp" else ())
        self.n = len(self.test_files)
        self.rank, self.world = 0, 1
        self._dev, self._check = device, check
        self._pool = ThreadPoolExecutor(max_workers=1, thread_name_prefix="shm-eval-loader")
        self._sizes = {}

    dev = EvalDataset.dev
    _decode = staticmethod(EvalDataset._decode)

    def __len__(self):
        return self.n

    def batch_range(self, index):
        return index, index + 1

    def _decode_pair(self, index):
        test, self._sizes[index] = self._capture.decode(self.test_files[index])
        diffuse = None if self.diffuse_files is None else self._decode(self.diffuse_files[index])
        return test, diffuse

    def sources(self, index):
        """[(path, (h, w))] of image `index`, as EvalDataset.sources."""
        if index not in self._sizes:
            from PIL import Image
            with Image.open(self.test_files[index]) as im:
                self._sizes[index] = self._capture.size(im.size[1], im.size[0])
        return [(self.test_files[index], tuple(int(v) for v in self._sizes[index]))]

    def _upload(self, a, hp, wp, top, left):
        out = torch.empty((1, hp, wp, 3), dtype=torch.float32, device=self.dev)
        ops.load_pad_u8(self._capture.photo(a, self.dev), out[0], top, left, 1.0 / 255.0)
        return out

    def batch(self, index, decoded=None):
        test, diffuse = decoded if decoded is not None else self._decode_pair(index)
        h, w = (int(v) for v in self._capture.size(*(test.shape[-2:] if isinstance(test, _MosaicArray) else test.shape[:2])))
        if diffuse is not None and tuple(diffuse.shape[:2]) != (h, w):
            raise ValueError(f"native-resolution evaluation compares a test image with its diffuse partner pixel by pixel: "
                             f"{self.test_files[index]} is {h} x {w}, {self.diffuse_files[index]} is {diffuse.shape[0]} x {diffuse.shape[1]}")
        hp, wp, top, left = pad_geometry(h, w)
        if self._check is not None:
            self._check(self.test_files[index], h, w)
        frame = self._upload(test, hp, wp, top, left)
        target = None if diffuse is None else self._upload(diffuse, h, w, 0, 0)
        return frame, target, (top, left, h, w)

    def __iter__(self):
        nxt = self._pool.submit(self._decode_pair, 0) if self.n else None
        for i in range(self.n):
            cur = nxt.result()
            nxt = self._pool.submit(self._decode_pair, i + 1) if i + 1 < self.n else None
            yield self.batch(i, cur)
