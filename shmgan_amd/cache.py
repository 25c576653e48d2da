"""Decoded-sample cache of the training loader (PolarDataset(cache="device")): the counterpart of the `.cache()` that ends every
pipeline of the reference's datasetLoad (datasetLoader.py:59-164), which decodes every file once, in epoch 0.

What is kept is a sample's DECODED BYTES (uint8, before crop, mirror and resize): shuffle and augmentation change the finished
float tensors every pass, the bytes never, and they are a quarter of the size.  `SampleCache` is an arena: device memory is taken in
chunks (256 MiB by default) only as samples arrive; the four or five images of a sample sit back to back in one chunk, each at a
16-byte aligned offset; a sample never straddles chunks, and one larger than a chunk gets a chunk of its own.  The budget
`cache_bytes` bounds the device memory taken (the sum of the chunk sizes; the last chunk is cut to what the budget leaves).  A sample
that does not fit is REFUSED: it is decoded and uploaded every time it comes up, as without a cache.  Nothing is ever evicted: first
come, first kept.  The cache is keyed by the sample's position in the sorted file lists; a file that changes on disk during a run is
not noticed (tf.data's cache does not notice either).

The planning here (offsets, alignment, chunking, budget, counters) makes no torch call: device memory comes from the injected
`alloc(nbytes)`, which returns an object with `data_ptr()` -- the loader hands in a torch.uint8 allocation on its stream, a test a
fake.  `sample_descriptor` turns a sample's pointers and its augmentation draw into the descriptor of ops.augment_batch_u8.
"""
from __future__ import annotations

from typing import NamedTuple

ALIGN = 16                       # every image starts at a multiple of this
CHUNK_BYTES = 256 << 20


def _align(n):
    return (n + ALIGN - 1) // ALIGN * ALIGN


def sample_bytes(n_images, hin, win):
    """Arena bytes of one sample: n_images images of hin x win x 3 bytes, each padded to the alignment."""
    return n_images * _align(hin * win * 3)


class Entry(NamedTuple):
    chunk: int           # index into SampleCache.chunks
    offsets: tuple       # byte offset of every image inside the chunk
    ptrs: tuple          # device address of every image
    hin: int
    win: int


class AugSample(NamedTuple):
    """One sample of ops.augment_batch_u8 (shm_aug_sample of include/shmgan_hip.h)."""
    srcs: tuple                          # device addresses (int) of the uint8 [hin,win,3] images, or such tensors
    hin: int
    win: int
    crop: tuple = None                   # (y, x, h, w) in source pixels; None = the whole image
    flip_ud: bool = False
    flip_lr: bool = False
    mix: bool = False
    planes: tuple = (0, 1, 2, 3)         # destination plane of view 0..3


def sample_descriptor(ptrs, hin, win, fixed_flip_ud, params=None, mirror=("identity", None)):
    """The descriptor of one sample.  params: the sample's data.AugmentParams, or None without augmentation: the identity crop and
    only the loader's fixed flip_ud orientation.  mirror: polar.mirror_views of the loader's angles; when the draw remaps the views,
    a "permute" mirror names the plane every source view lands in (mirrored view i is view how[i], so source v goes to plane
    how.index(v)) and a "mix" mirror sets the mix flag -- the logic of PolarDataset._prepare_augmented."""
    if params is None:
        return AugSample(tuple(ptrs), int(hin), int(win), (0.0, 0.0, float(hin), float(win)), bool(fixed_flip_ud), False, False, (0, 1, 2, 3))
    kind, how = mirror
    planes = tuple(list(how).index(v) for v in range(4)) if params.remap and kind == "permute" else (0, 1, 2, 3)
    return AugSample(tuple(ptrs), int(hin), int(win), tuple(float(c) for c in params.crop), bool(fixed_flip_ud) != bool(params.flip_ud),
                     bool(params.flip_lr), bool(params.remap and kind == "mix"), planes)


class SampleCache:
    """position -> Entry.  alloc(nbytes) -> chunk with data_ptr(); budget: bytes of device memory the cache may take, or a callable
    that says so when the first sample is stored (the loader's default: half of the free device memory at that moment)."""

    def __init__(self, alloc, budget, chunk_bytes=CHUNK_BYTES):
        if chunk_bytes < ALIGN:
            raise ValueError(f"chunk_bytes {chunk_bytes} < {ALIGN}")
        self._alloc, self._budget, self.chunk_bytes = alloc, budget, int(chunk_bytes)
        self.chunks, self._sizes = [], []            # the allocations and their sizes
        self._fill = 0                               # bytes used in the last chunk
        self._table, self._refused = {}, set()
        self.hits = self.misses = 0

    @property
    def budget(self):
        if callable(self._budget):
            self._budget = int(self._budget())
        return int(self._budget)

    def lookup(self, position):
        """The Entry of a resident sample (a hit), or None (a miss: not seen yet, or refused)."""
        e = self._table.get(position)
        if e is None:
            self.misses += 1
        else:
            self.hits += 1
        return e

    def store(self, position, n_images, hin, win):
        """Reserve the arena slot of a sample that lookup() missed: its Entry (the caller copies the bytes in), or None when the
        budget does not hold it."""
        if position in self._table:
            return self._table[position]
        each, need = _align(hin * win * 3), sample_bytes(n_images, hin, win)
        if not self.chunks or self._fill + need > self._sizes[-1]:
            left = self.budget - sum(self._sizes)
            size = need if need > self.chunk_bytes else min(self.chunk_bytes, left)
            if need > left:
                self._refused.add(position)
                return None
            self.chunks.append(self._alloc(size))
            self._sizes.append(size)
            self._fill = 0
        k, base = len(self.chunks) - 1, self.chunks[-1].data_ptr()
        if base % ALIGN:
            raise ValueError(f"the allocator returned a chunk at {base:#x}, which is not {ALIGN}-byte aligned")
        offsets = tuple(self._fill + i * each for i in range(n_images))
        self._fill += need
        e = Entry(k, offsets, tuple(base + o for o in offsets), int(hin), int(win))
        self._table[position] = e
        self._refused.discard(position)
        return e

    def stats(self):
        """resident / refused: samples held / turned away (distinct positions); bytes: device memory taken (the chunks);
        hits / misses: lookups answered from the arena / not."""
        return {"resident": len(self._table), "bytes": sum(self._sizes), "chunks": len(self.chunks), "hits": self.hits,
                "misses": self.misses, "refused": len(self._refused)}
