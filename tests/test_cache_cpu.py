"""The decoded-sample cache without a GPU: the arena's planning (shmgan_amd.cache.SampleCache behind a fake allocator), its counters,
the descriptors the cached loader hands to shm_augment_batch_u8, the loader / trainer options, and the argument checks of the C entry
point (all before any launch)."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest

from shmgan_amd import cache as ch


class FakeChunk:
    def __init__(self, base, size):
        self.base, self.size = base, size

    def data_ptr(self):
        return self.base


class FakeAlloc:
    """Hands out 256-byte aligned address ranges and remembers them."""

    def __init__(self):
        self.chunks, self.next = [], 0x10000

    def __call__(self, nbytes):
        c = FakeChunk(self.next, nbytes)
        self.chunks.append(c)
        self.next += (nbytes + 255) // 256 * 256 + 4096
        return c


def _inside_one_chunk(alloc, e, n_images, hin, win):
    c = alloc.chunks[e.chunk]
    each = hin * win * 3
    assert len(e.ptrs) == len(e.offsets) == n_images
    for i, (p, o) in enumerate(zip(e.ptrs, e.offsets)):
        assert p == c.base + o and p % 16 == 0 and o % 16 == 0
        assert c.base <= p and p + each <= c.base + c.size
        if i:                       # back to back: the next image starts at the previous one's end, rounded up to 16
            assert o == e.offsets[i - 1] + (each + 15) // 16 * 16


def test_offsets_are_aligned_and_samples_stay_inside_one_chunk():
    alloc = FakeAlloc()
    sc = ch.SampleCache(alloc, budget=1 << 20, chunk_bytes=4096)
    shapes = [(5, 37, 53), (4, 9, 7), (5, 16, 16), (4, 5, 5), (5, 1, 1), (5, 11, 13), (4, 17, 3)]      # 37*53*3 = 5883 > 4096 / 5: own chunk
    spans = []
    for pos, (n, h, w) in enumerate(shapes):
        e = sc.store(pos, n, h, w)
        assert e is not None and (e.hin, e.win) == (h, w)
        _inside_one_chunk(alloc, e, n, h, w)
        spans.append((e.chunk, e.offsets[0], e.offsets[0] + ch.sample_bytes(n, h, w)))
    for i, a in enumerate(spans):                 # no two samples overlap
        for b in spans[i + 1:]:
            assert a[0] != b[0] or a[2] <= b[1] or b[2] <= a[1]
    st = sc.stats()
    assert st["resident"] == len(shapes) and st["chunks"] == len(alloc.chunks) and st["bytes"] == sum(c.size for c in alloc.chunks)
    assert sc.store(0, 5, 37, 53) is sc.lookup(0)              # storing again changes nothing
    assert sc.stats()["bytes"] == st["bytes"]


def test_a_sample_larger_than_the_chunk_gets_its_own_chunk():
    alloc = FakeAlloc()
    sc = ch.SampleCache(alloc, budget=1 << 20, chunk_bytes=1024)
    small = sc.store(0, 4, 4, 4)                                # 4 * 48 bytes
    big = sc.store(1, 5, 32, 32)                                # 5 * 3072 > 1024
    after = sc.store(2, 4, 4, 4)
    assert small.chunk == 0 and alloc.chunks[0].size == 1024
    assert big.chunk == 1 and alloc.chunks[1].size == ch.sample_bytes(5, 32, 32) == 5 * 3072
    assert after.chunk == 2 and alloc.chunks[2].size == 1024     # a sample never straddles: the next one opens a new chunk
    _inside_one_chunk(alloc, big, 5, 32, 32)


def test_chunks_are_taken_only_as_samples_arrive():
    alloc = FakeAlloc()
    sc = ch.SampleCache(alloc, budget=1 << 20, chunk_bytes=1024)
    assert not alloc.chunks and sc.stats()["bytes"] == 0
    for pos in range(5):                                        # 192 bytes each: five fit one chunk
        sc.store(pos, 4, 4, 4)
    assert len(alloc.chunks) == 1
    sc.store(5, 4, 4, 4)
    assert len(alloc.chunks) == 2


def test_budget_refuses_later_samples_and_keeps_earlier_ones():
    alloc = FakeAlloc()
    per = ch.sample_bytes(5, 8, 8)                              # 5 * 192
    sc = ch.SampleCache(alloc, budget=2 * per + 100, chunk_bytes=1 << 20)
    kept = [sc.store(pos, 5, 8, 8) for pos in range(4)]
    assert kept[0] is not None and kept[1] is not None and kept[2] is None and kept[3] is None
    assert sum(c.size for c in alloc.chunks) <= 2 * per + 100 and sc.stats()["bytes"] <= 2 * per + 100
    assert sc.lookup(0) == kept[0] and sc.lookup(1) == kept[1] and sc.lookup(2) is None
    assert sc.store(2, 5, 8, 8) is None                         # asked again: refused again, counted once
    assert sc.store(4, 4, 2, 2) is not None                     # first come, first kept -- and whatever still fits is kept
    st = sc.stats()
    assert (st["resident"], st["refused"]) == (3, 2) and st["bytes"] <= 2 * per + 100
    # a budget across several chunks: the last chunk is cut to what is left, and the total never passes the budget
    alloc = FakeAlloc()
    sc = ch.SampleCache(alloc, budget=2500, chunk_bytes=1024)
    got = [sc.store(pos, 4, 8, 8) for pos in range(6)]          # 768 bytes each: one per 1024-byte chunk
    assert [c.size for c in alloc.chunks] == [1024, 1024] and [g is not None for g in got] == [True, True, False, False, False, False]
    assert sc.stats()["bytes"] == 2048 <= 2500
    assert ch.SampleCache(FakeAlloc(), budget=0).store(0, 4, 1, 1) is None


def test_default_budget_is_asked_for_when_the_first_sample_is_stored():
    asked = []

    def budget():
        asked.append(1)
        return 4096
    sc = ch.SampleCache(FakeAlloc(), budget)
    assert sc.lookup(3) is None and not asked
    assert sc.store(3, 4, 4, 4) is not None and sc.store(4, 4, 4, 4) is not None and asked == [1]


def test_stats_count_hits_misses_and_refusals():
    sc = ch.SampleCache(FakeAlloc(), budget=ch.sample_bytes(5, 4, 4) * 2, chunk_bytes=4096)
    for pos in (0, 1, 2, 0, 1, 2, 2, 0):                        # the loader's sequence: look up, store on a miss
        if sc.lookup(pos) is None:
            sc.store(pos, 5, 4, 4)
    assert sc.stats() == {"resident": 2, "bytes": 480, "chunks": 1, "hits": 3, "misses": 5, "refused": 1}


# ------------------------------------------------------------------------------------------------ descriptors
def test_descriptor_without_augment_is_the_identity_crop():
    for flip in (True, False):
        d = ch.sample_descriptor((16, 32, 48, 64, 80), 37, 53, flip)
        assert d == ch.AugSample((16, 32, 48, 64, 80), 37, 53, (0.0, 0.0, 37.0, 53.0), flip, False, False, (0, 1, 2, 3))


def _todays_call(p, fixed_flip_ud, mirror):
    """What PolarDataset._prepare_augmented hands to ops.augment_views_u8 for a draw p: (order of the destination planes, mix or
    None, crop, flip_ud, flip_lr)."""
    kind, how = mirror
    dsts = [0, 1, 2, 3, 4]
    if p.remap and kind == "permute":
        dsts = [dsts[how.index(v)] for v in range(4)] + dsts[4:]
    return dsts[:4], (how if p.remap and kind == "mix" else None), p.crop, bool(fixed_flip_ud) != p.flip_ud, p.flip_lr


@pytest.mark.parametrize("angles,kind", [((0.0, 45.0, 90.0, 135.0), "permute"), ((0.0, 60.0, 90.0, 150.0), "mix")])
def test_descriptor_with_augment_is_todays_call(angles, kind):
    from shmgan_amd.data import Augment, augment_params
    from shmgan_amd.polar import mirror_views
    mirror = mirror_views(list(angles))
    assert mirror[0] == kind
    aug, seen = Augment(0.5, 0.5, 0.5), set()
    for pos in range(24):
        p = augment_params(7, 2, pos, 37, 53, aug)
        seen.add((p.flip_ud, p.flip_lr))
        for fixed in (True, False):
            d = ch.sample_descriptor((1, 2, 3, 4), 37, 53, fixed, p, mirror)
            planes, mix, crop, fud, flr = _todays_call(p, fixed, mirror)
            assert (d.planes, d.mix, d.crop, d.flip_ud, d.flip_lr) == (tuple(planes), mix is not None, crop, fud, flr), (pos, fixed)
            assert (d.hin, d.win, d.srcs) == (37, 53, (1, 2, 3, 4))
            if kind == "permute" and p.remap:
                assert d.planes == (0, 3, 2, 1)                 # 45 <-> 135
    assert len(seen) == 4
    keep = ch.sample_descriptor((1, 2, 3, 4), 37, 53, True, augment_params(7, 2, 0, 37, 53, aug), ("identity", None))
    assert keep.planes == (0, 1, 2, 3) and not keep.mix         # views="keep": a plain geometric flip


# ------------------------------------------------------------------------------------------------ options
def _listing(root, subdirs, n):
    for sub in subdirs:
        (root / sub).mkdir(parents=True, exist_ok=True)
        for i in range(n):
            (root / sub / f"img_{i:02d}.png").write_bytes(b"")
    return str(root)


def test_loader_and_trainer_options(tmp_path):
    from shmgan_amd.data import PSD_SUBDIRS, PolarDataset, datasetLoad
    from shmgan_amd.trainer import _DEFAULTS
    root = _listing(tmp_path, PSD_SUBDIRS, 4)
    ds = PolarDataset(root, 32, rank=0, world=1, device="cpu")
    assert ds.cache == "none" and ds.cache_bytes is None
    assert ds.cache_stats() == {"resident": 0, "bytes": 0, "chunks": 0, "hits": 0, "misses": 0, "refused": 0}
    with pytest.raises(ValueError, match="cache"):
        PolarDataset(root, 32, rank=0, world=1, cache="host")
    with pytest.raises(ValueError, match="cache_bytes"):
        PolarDataset(root, 32, rank=0, world=1, cache="device", cache_bytes=-1)

    def load(**args):
        t = SimpleNamespace(data_dir=root, image_size=32, batch_size=1, device="cpu", num_epochs=1, args=SimpleNamespace(**args))
        return datasetLoad(t)[1]
    assert load().cache == "none"
    ds = load(cache="device", cache_gb=0.5)
    assert ds.cache == "device" and ds.cache_bytes == 2 ** 29
    assert load(cache="device").cache_bytes is None
    assert (_DEFAULTS["cache"], _DEFAULTS["cache_gb"]) == ("none", None)


# ------------------------------------------------------------------------------------------------ the C ABI's argument checks
def test_shape_errors_name_the_sample_before_any_launch():
    from shmgan_amd import _lib, ops
    L = _lib.lib()
    S = ops._aug_sample_struct()
    assert C.sizeof(S) == 96 and ops.AUG_GROUP == 8
    p5 = (C.c_void_p * 5)(1, 1, 1, 1, 1)                        # non-null pointers nobody dereferences
    MIN, STOKES, DIR = 0, 1, 2
    nan = float("nan")

    def samples(n=3, **bad):
        """n good 8x8 samples; `bad` = {field: (sample index, value)}."""
        arr = (S * n)()
        for s in arr:
            for v in range(5):
                s.src[v] = 1
            s.hin = s.win = 8
            s.crop_h = s.crop_w = 8.0
            for v in range(4):
                s.plane[v] = v
        for k, (i, val) in bad.items():
            if k == "src":
                arr[i].src[val] = None
            elif k == "plane":
                for v in range(4):
                    arr[i].plane[v] = val[v]
            elif k == "crop":
                arr[i].crop_y, arr[i].crop_x, arr[i].crop_h, arr[i].crop_w = val
            else:
                setattr(arr[i], k, val)
        return arr

    def call(arr, n=None, n_src=5, mode=DIR, coef=None, mix=None, dst=p5, stride=48, ho=4, wo=4):
        return L.shm_augment_batch_u8(arr, len(arr) if n is None else n, n_src, mode, coef, mix, dst, stride, ho, wo, 1.0, None)

    cases = [(dict(arr=None, n=1), b"null pointer"), (dict(dst=None), b"null pointer"), (dict(n=0), b"n 0 < 1"), (dict(n=-2), b"n -2 < 1"),
             (dict(dst=(C.c_void_p * 5)(1, 1, None, 1, 1)), b"destination plane 2"),
             (dict(n_src=4), b"n_src 4"), (dict(n_src=5, mode=MIN), b"n_src 5"), (dict(n_src=4, mode=7), b"mode 7"),
             (dict(ho=0), b"outside [1, 32768]"), (dict(wo=40000), b"outside [1, 32768]"), (dict(stride=47), b"sample_stride 47"),
             (dict(n_src=4, mode=STOKES), b"needs coef"),
             (dict(arr=samples(src=(2, 3))), b"sample 2: null pointer (source 3)"),
             (dict(arr=samples(hin=(1, 0))), b"sample 1: sizes hin 0"), (dict(arr=samples(win=(0, 32769))), b"sample 0: sizes hin 8, win 32769"),
             (dict(arr=samples(crop=(1, (0.0, 0.0, 0.0, 8.0)))), b"sample 1: empty crop"),
             (dict(arr=samples(crop=(1, (0.0, 0.0, nan, 8.0)))), b"sample 1: empty crop"),
             (dict(arr=samples(crop=(1, (0.5, 0.0, 8.0, 8.0)))), b"sample 1: the crop 8 x 8 at (0.5, 0) does not lie inside the 8 x 8 image"),
             (dict(arr=samples(crop=(2, (0.0, nan, 4.0, 4.0)))), b"sample 2: the crop"),
             (dict(arr=samples(crop=(0, (-0.5, 0.0, 8.0, 8.0)))), b"sample 0: the crop"),
             (dict(arr=samples(mix=(1, 1))), b"sample 1: the mix flag needs mix"),
             (dict(arr=samples(plane=(1, (0, 1, 1, 3)))), b"sample 1: planes (0, 1, 1, 3) are not a permutation"),
             (dict(arr=samples(plane=(2, (0, 1, 2, 4)))), b"sample 2: planes (0, 1, 2, 4)"),
             (dict(arr=samples(n=9, plane=(8, (-1, 1, 2, 3)))), b"sample 8: planes (-1, 1, 2, 3)")]       # past the first group
    for kw, msg in cases:
        kw = dict(kw)
        arr = kw.pop("arr", samples())
        assert call(arr, **kw) == -1 and msg in L.shm_last_error(), (kw, msg, L.shm_last_error())
        assert b"shm_augment_batch_u8" in L.shm_last_error()
    # a source past n_src is not read: four sources and a null fifth are fine for MIN ... up to the launch, which this test must not reach
    assert call(samples(src=(0, 4)), n_src=4, mode=MIN, ho=0) == -1 and b"outside [1, 32768]" in L.shm_last_error()


def test_the_two_kernels_share_one_definition_of_the_arithmetic():
    """Both kernel sources include csrc/augment_px.h and neither restates the coordinate, the mix or the lerp; the coordinate and the
    lerp themselves are the sampler of csrc/bilinear.h, which augment_px.h includes and does not restate either."""
    from pathlib import Path
    from shmgan_amd import _lib
    body, sampler = (_lib.CSRC / "augment_px.h").read_text(), (_lib.CSRC / "bilinear.h").read_text()
    assert "augment_pixel" in body and '#include "bilinear.h"' in body and "floorf" not in body and "* lx" not in body
    assert "* hs - 0.5f) + cy" in sampler and "bilinear_lerp" in sampler
    assert (_lib.CSRC / "augment_px.h") in _lib.SHARED_HEADERS and (_lib.CSRC / "bilinear.h") in _lib.SHARED_HEADERS
    for name in ("augment.hip", "augment_batch.hip"):
        src = (_lib.CSRC / name).read_text()
        assert '#include "augment_px.h"' in src and "augment_pixel<MODE" in src, name
        assert "floorf" not in src and "* lx" not in src and "polar_estimate" not in src, name
