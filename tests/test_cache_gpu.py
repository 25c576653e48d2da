"""The decoded-sample cache on the device.  Kernel level: shm_augment_batch_u8 against shm_augment_views_u8 called once per sample,
bit for bit, for mixed source sizes, crops, mirrors, the view mix and a plane permutation in one call; at identity parameters also
against shm_resize_bilinear_u8 / shm_polar_views_u8; one case against the float64 restatement (tests/augment_ref.py); and its
refusals.  Loader level: PolarDataset(cache="device") against cache="none", bit for bit over three passes; decode and launch
counts; a budget that holds two samples; the size-mismatch error; the trainer options.

Tolerance of the float64 case: polar_ref.bound -- the larger of 2e-6 and four times the error the float32 restatement shows against
float64 on the same inputs (printed).  Everything else is bitwise."""
import argparse
import functools

import numpy as np
import pytest
import torch

import augment_ref as ar
import polar_ref as pr
from util import host

pytestmark = pytest.mark.gpu

PSD_ANGLES = (0.0, 60.0, 90.0, 150.0)
MODES = {"min": ar.MIN, "stokes": ar.STOKES, "dir": ar.DIR}
SIZES3 = [(37, 53), (16, 16), (9, 7)]                                  # 9 x 7 upsamples
SIZES9 = SIZES3 + [(40, 24), (5, 5), (37, 53), (9, 7), (16, 16), (40, 24)]
SENTINEL = -7.0


@functools.lru_cache(maxsize=None)
def _images(hin, win, k=0):
    """Five random byte images of one sample (shared by the tests; never modified)."""
    rng = np.random.default_rng(1000 * hin + win + 77 * k)
    out = [rng.integers(0, 256, (hin, win, 3)).astype(np.uint8) for _ in range(5)]
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _psd():
    from shmgan_amd.polar import mirror_views, stokes_matrix
    kind, mix = mirror_views(PSD_ANGLES)
    assert kind == "mix"
    return stokes_matrix(PSD_ANGLES), mix


def _edge_crop(i, hin, win):
    """A crop of half the sides that touches the top, bottom, left or right edge (i mod 4), or a fractional inner one; every number
    is a multiple of 0.25, so float32 holds it and origin + extent <= size exactly."""
    h, w = hin / 2.0, win / 2.0
    return [(0.0, win / 4.0, h, w), (hin - h, win / 4.0, h, w), (hin / 4.0, 0.0, h, w), (hin / 4.0, win - w, h, w),
            (hin / 4.0 + 0.25, win / 4.0 - 0.25, h, w)][i % 5]


def _params(sizes):
    """Per sample (hin, win, crop, flip_ud, flip_lr, mix, planes): all four flip combinations, a crop at each image edge, the mix on
    some samples and not on others, a plane permutation on one (and an identity sample first)."""
    out = []
    for i, (hin, win) in enumerate(sizes):
        crop = None if i == 0 else _edge_crop(i - 1, hin, win)
        out.append((hin, win, crop, bool(i & 1), bool(i & 2), i % 3 == 1, (0, 3, 2, 1) if i == 2 else (0, 1, 2, 3)))
    return out


def _device_samples(params, mode):
    from shmgan_amd.cache import AugSample
    nsrc = 5 if mode == "dir" else 4
    return [AugSample(tuple(torch.from_numpy(a.copy()).cuda() for a in _images(hin, win, i)[:nsrc]), hin, win, crop, fud, flr, mix, planes)
            for i, (hin, win, crop, fud, flr, mix, planes) in enumerate(params)]


def _batched(samples, ho, wo, mode, fill=float("nan"), n_out=None):
    """The five [n,ho,wo,3] tensors of one ops.augment_batch_u8 call (NaN-filled before it: every element must be written)."""
    from shmgan_amd import ops
    outs = [torch.full((n_out or len(samples), ho, wo, 3), fill, device="cuda") for _ in range(5)]
    ops.augment_batch_u8(samples, outs, mode, _psd()[0] if mode == "stokes" else None, _psd()[1], 1.0 / 255.0)
    return outs


def _one_by_one(samples, ho, wo, mode):
    """The same tensors from ops.augment_views_u8 called for every sample alone, view v handed the sample's plane planes[v]."""
    from shmgan_amd import ops
    outs = [torch.full((len(samples), ho, wo, 3), float("nan"), device="cuda") for _ in range(5)]
    for i, s in enumerate(samples):
        dsts = [outs[s.planes[v]][i] for v in range(4)] + [outs[4][i]]
        ops.augment_views_u8(list(s.srcs), dsts, mode, _psd()[0] if mode == "stokes" else None, _psd()[1] if s.mix else None, s.crop,
                             s.flip_ud, s.flip_lr, 1.0 / 255.0)
    return outs


# ------------------------------------------------------------------------------------------------ kernel against the per-sample kernel
@pytest.mark.parametrize("ho,wo", [(16, 16), (17, 19)])
@pytest.mark.parametrize("sizes", [SIZES3[:1], SIZES3, SIZES9], ids=["n1", "n3", "n9"])
@pytest.mark.parametrize("mode", ["dir", "min", "stokes"])
def test_batch_is_the_per_sample_kernel_bitwise(mode, sizes, ho, wo):
    samples = _device_samples(_params(sizes), mode)
    got, want = _batched(samples, ho, wo, mode), _one_by_one(samples, ho, wo, mode)
    for v in range(5):
        assert torch.isfinite(want[v]).all()
        assert torch.equal(got[v], want[v]), (mode, len(sizes), v)
    if len(sizes) > 2:          # the permuted sample is not the unpermuted one: planes 1 and 3 really changed places
        plain = _batched([samples[2]._replace(planes=(0, 1, 2, 3))], ho, wo, mode)
        assert torch.equal(plain[1][0], got[3][2]) and torch.equal(plain[3][0], got[1][2]) and not torch.equal(plain[1][0], got[1][2])


@pytest.mark.parametrize("mode", ["dir", "min", "stokes"])
def test_one_pixel_outputs_from_5x5(mode):
    samples = _device_samples(_params([(5, 5)] * 5), mode)
    got, want = _batched(samples, 1, 1, mode), _one_by_one(samples, 1, 1, mode)
    assert all(torch.equal(g, w) and torch.isfinite(w).all() for g, w in zip(got, want))


@pytest.mark.parametrize("ho,wo", [(16, 16), (17, 19), (1, 1)])
def test_identity_parameters_are_the_resize_and_polar_kernels_bitwise(ho, wo):
    from shmgan_amd import ops
    from shmgan_amd.cache import AugSample
    sizes = SIZES3 + [(5, 5)]
    srcs = [[torch.from_numpy(a.copy()).cuda() for a in _images(h, w, i)] for i, (h, w) in enumerate(sizes)]
    for flip in (False, True):
        want = [torch.full((len(sizes), ho, wo, 3), float("nan"), device="cuda") for _ in range(5)]
        for i in range(len(sizes)):
            for v in range(5):
                ops.resize_bilinear_u8(srcs[i][v], want[v][i], 1.0 / 255.0, flip)
        whole = [AugSample(tuple(s), h, w, None, flip) for s, (h, w) in zip(srcs, sizes)]
        stated = [AugSample(tuple(s), h, w, (0.0, 0.0, float(h), float(w)), flip) for s, (h, w) in zip(srcs, sizes)]
        for samples in (whole, stated):
            assert all(torch.equal(g, w) for g, w in zip(_batched(samples, ho, wo, "dir"), want)), ("dir", flip)
        for mode in ("min", "stokes"):
            for i in range(len(sizes)):
                ops.polar_views_u8(srcs[i][:4], [want[v][i] for v in range(5)], mode, _psd()[0], 1.0 / 255.0, flip)
            got = _batched([s._replace(srcs=s.srcs[:4]) for s in whole], ho, wo, mode)
            assert all(torch.equal(g, w) for g, w in zip(got, want)), (mode, flip)


@pytest.mark.parametrize("mode", ["dir", "min", "stokes"])
def test_mixed_sizes_against_float64(mode):
    params = _params(SIZES3)
    got = [host(t) for t in _batched(_device_samples(params, mode), 17, 19, mode)]
    n = 5 if mode == "dir" else 4
    for i, (hin, win, crop, fud, flr, mix, planes) in enumerate(params):
        crop = crop and tuple(float(np.float32(c)) for c in crop)
        kw = dict(coef=_psd()[0], mix=_psd()[1] if mix else None, crop=crop, flip_ud=fud, flip_lr=flr)
        ref = ar.augment_views(_images(hin, win, i)[:n], 17, 19, MODES[mode], dtype=np.float64, **kw)
        r32 = ar.augment_views(_images(hin, win, i)[:n], 17, 19, MODES[mode], dtype=np.float32, **kw)
        for v in range(5):
            plane = planes[v] if v < 4 else 4
            e32 = float(np.abs(r32[v] - ref[v]).max())
            err = float(np.abs(got[plane][i] - ref[v]).max())
            print(f"batch {mode} sample {i} view {v} -> plane {plane}: device error {err:.3e}, float32 restatement {e32:.3e}, bound {pr.bound(e32):.3e}")
            assert np.isfinite(got[plane][i]).all() and err <= pr.bound(e32), (mode, i, v, err, e32)


def test_refusals_name_the_sample_and_write_nothing():
    from shmgan_amd import ops
    from shmgan_amd._lib import ShmError
    good = _device_samples(_params(SIZES3), "dir")
    nan = float("nan")
    cases = [([good[0], good[1], good[2]._replace(srcs=good[2].srcs[:2] + (0,) + good[2].srcs[3:])], "sample 2: null pointer (source 2)"),
             ([good[0], good[1]._replace(crop=(8.5, 0.0, 8.0, 8.0)), good[2]], "sample 1: the crop 8 x 8 at (8.5, 0) does not lie inside the 16 x 16 image"),
             ([good[0], good[1]._replace(crop=(0.0, nan, 8.0, 8.0)), good[2]], "sample 1: the crop"),
             ([good[0]._replace(crop=(0.0, 0.0, nan, 8.0))], "sample 0: empty crop"),
             ([good[0], good[1], good[2]._replace(planes=(0, 1, 1, 3))], "sample 2: planes (0, 1, 1, 3) are not a permutation"),
             ([], "n 0 < 1")]
    for samples, msg in cases:
        outs = [torch.full((3, 16, 16, 3), SENTINEL, device="cuda") for _ in range(5)]
        with pytest.raises(ShmError) as e:
            ops.augment_batch_u8(samples, outs, "dir", None, _psd()[1])
        assert "(-1)" in str(e.value) and msg in str(e.value) and "shm_augment_batch_u8" in str(e.value), str(e.value)
        torch.cuda.synchronize()
        assert all(bool((t == SENTINEL).all()) for t in outs), msg
    # a bad sample in the SECOND group of a call stops the first group's launch too
    nine = _device_samples(_params(SIZES9), "dir")
    nine[8] = nine[8]._replace(planes=(0, 1, 2, 4))
    outs = [torch.full((9, 16, 16, 3), SENTINEL, device="cuda") for _ in range(5)]
    with pytest.raises(ShmError, match="sample 8: planes"):
        ops.augment_batch_u8(nine, outs, "dir", None, _psd()[1])
    torch.cuda.synchronize()
    assert all(bool((t == SENTINEL).all()) for t in outs)
    # fewer samples than the tensors hold: the slices past them stay as they were
    outs = _batched(good[:2], 16, 16, "dir", fill=SENTINEL, n_out=3)
    assert all(bool((t[2] == SENTINEL).all()) and bool((t[:2] != SENTINEL).all()) for t in outs)


# ------------------------------------------------------------------------------------------------ the loader
SAMPLE_SIZES = [(40, 56), (37, 53), (16, 16), (9, 7), (24, 40), (33, 21), (20, 20)]
S, B = 16, 3


def _write(root, subdirs, sizes, seed):
    from PIL import Image
    rng = np.random.default_rng(seed)
    for sub in subdirs:
        (root / sub).mkdir(parents=True, exist_ok=True)
    for i, hw in enumerate(sizes):
        for sub in subdirs:
            Image.fromarray(rng.integers(0, 256, (*hw, 3)).astype(np.uint8)).save(root / sub / f"img_{i:02d}.png")
    return str(root)


@pytest.fixture(scope="module")
def captures(tmp_path_factory):
    from shmgan_amd.data import PSD_SUBDIRS, SHMGAN_SUBDIRS
    return {"psd": (_write(tmp_path_factory.mktemp("cache_psd"), PSD_SUBDIRS, SAMPLE_SIZES, 51), PSD_SUBDIRS),
            "45": (_write(tmp_path_factory.mktemp("cache_45"), SHMGAN_SUBDIRS, SAMPLE_SIZES, 52), SHMGAN_SUBDIRS)}


def _passes(ds):
    """Every batch of an iteration over `ds`, as host arrays [batch][plane] of [B,S,S,3] (float32, untouched)."""
    return [[t.cpu().numpy() for t in batch] for batch in ds]


def _same(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y) for p, q in zip(a, b) for x, y in zip(p, q))


@pytest.mark.parametrize("views", ["psd", "45"])
@pytest.mark.parametrize("augmented", [False, True], ids=["plain", "augment_shuffle"])
@pytest.mark.parametrize("source", ["dir", "min", "stokes"])
def test_cached_loader_is_the_uncached_loader_bitwise(captures, source, augmented, views):
    from shmgan_amd.data import Augment, PolarDataset
    root, subdirs = captures[views]
    kw = dict(batch_size=B, subdirs=subdirs, rank=0, world=1, epochs=3, diffuse_source=source, seed=6)
    if augmented:
        kw.update(augment=Augment(0.5, 0.5, 0.5), shuffle=True)
    want = _passes(PolarDataset(root, S, cache="none", **kw))
    ds = PolarDataset(root, S, cache="device", **kw)
    got = _passes(ds)
    assert len(want) == 3 * (len(SAMPLE_SIZES) // B) == 6
    for j, (g, w) in enumerate(zip(got, want)):
        for v in range(5):
            assert np.isfinite(w[v]).all() and np.array_equal(g[v], w[v]), (source, augmented, views, j, v)
    st = ds.cache_stats()
    assert st["refused"] == 0 and st["chunks"] == 1 and st["hits"] + st["misses"] == 18 and st["misses"] == st["resident"] <= 7
    if not augmented:
        assert st["resident"] == 6 and _same(want[:2], want[2:4])                        # without augmentation the passes repeat


class _Counts:
    """Counts PolarDataset._decode and the ops wrappers the loader calls."""
    NAMES = ("resize_bilinear_u8", "polar_views_u8", "augment_views_u8", "augment_batch_u8")

    def __init__(self, monkeypatch):
        from shmgan_amd import ops
        from shmgan_amd.data import PolarDataset
        self.n = dict.fromkeys(self.NAMES + ("decode",), 0)
        for name in self.NAMES:
            monkeypatch.setattr(ops, name, self._counted(name, getattr(ops, name)))
        monkeypatch.setattr(PolarDataset, "_decode", self._counted("decode", PolarDataset._decode))

    def _counted(self, name, fn):
        def call(*a, **kw):
            self.n[name] += 1
            return fn(*a, **kw)
        return call

    def take(self):
        out, self.n = self.n, dict.fromkeys(self.n, 0)
        return out


def _one_pass(ds, p):
    return [[t.cpu().numpy() for t in ds.batch(i, p)] for i in range(len(ds))]


def test_decode_and_launch_counts(captures, monkeypatch):
    from shmgan_amd.data import Augment, PolarDataset
    root, subdirs = captures["psd"]
    c = _Counts(monkeypatch)
    zero = dict.fromkeys(_Counts.NAMES + ("decode",), 0)
    ds = PolarDataset(root, S, batch_size=B, rank=0, world=1, cache="device")
    _one_pass(ds, 0)
    assert c.take() == dict(zero, decode=5 * 6, augment_batch_u8=2)
    for p in (1, 2):
        _one_pass(ds, p)
        assert c.take() == dict(zero, augment_batch_u8=2), p                         # no decode, one launch per batch
    assert ds.cache_stats()["hits"] == 12
    # cache="none": the calls of today's three paths, and never the new kernel
    for kw, want in ((dict(), dict(zero, decode=30, resize_bilinear_u8=30)),
                     (dict(diffuse_source="min"), dict(zero, decode=24, polar_views_u8=6)),
                     (dict(augment=Augment(0.5, 0.5, 0.5)), dict(zero, decode=30, augment_views_u8=6)),
                     (dict(diffuse_source="stokes", augment=Augment(0.5, 0.5, 0.5), shuffle=True), dict(zero, decode=24, augment_views_u8=6))):
        plain = PolarDataset(root, S, batch_size=B, rank=0, world=1, **kw)
        for p in (0, 1):
            _one_pass(plain, p)
            assert c.take() == want, (kw, p)
        assert plain.cache_stats()["resident"] == 0


def test_budget_for_two_samples(captures, monkeypatch):
    from shmgan_amd.cache import sample_bytes
    from shmgan_amd.data import PolarDataset
    root, subdirs = captures["psd"]
    budget = sample_bytes(5, *SAMPLE_SIZES[0]) + sample_bytes(5, *SAMPLE_SIZES[1])
    plain = PolarDataset(root, S, batch_size=B, rank=0, world=1)
    want = [_one_pass(plain, p) for p in range(3)]
    c = _Counts(monkeypatch)
    ds = PolarDataset(root, S, batch_size=B, rank=0, world=1, cache="device", cache_bytes=budget)
    for p in range(3):
        got = _one_pass(ds, p)
        n = c.take()
        assert n["decode"] == (30 if p == 0 else 20) and n["augment_batch_u8"] == 2, (p, n)    # later passes decode the four refused samples
        assert _same(got, want[p]), p
        st = ds.cache_stats()
        assert (st["resident"], st["refused"], st["chunks"]) == (2, 4, 1) and st["bytes"] <= budget, st
    assert st["hits"] == 4 and st["misses"] == 6 + 4 + 4


def test_a_view_of_another_size_raises_under_the_cache(tmp_path):
    from PIL import Image
    from shmgan_amd.data import PSD_SUBDIRS, Augment, PolarDataset
    _write(tmp_path, PSD_SUBDIRS, [(40, 56)] * 2, 53)
    Image.fromarray(np.zeros((41, 56, 3), np.uint8)).save(tmp_path / "ED" / "img_00.png")           # the views are 40 x 56
    for kw in (dict(), dict(augment=Augment(flip_lr=0.5))):
        ds = PolarDataset(str(tmp_path), S, batch_size=1, rank=0, world=1, cache="device", **kw)
        with pytest.raises(ValueError, match=r"same decoded size.*ED.*img_00\.png 41x56"):
            ds.batch(0)
        assert tuple(ds.batch(1)[4].shape) == (1, S, S, 3)                                             # the next sample is fine
        assert ds.cache_stats()["resident"] == 1
    # four views suffice for "min": the odd ED file is never read
    ds = PolarDataset(str(tmp_path), S, batch_size=1, rank=0, world=1, cache="device", diffuse_source="min")
    assert tuple(ds.batch(0)[4].shape) == (1, S, S, 3)


def test_trainer_options_reach_the_loader_and_stats_answer(tmp_path):
    from shmgan_amd import ShmGANwithSSpecSeg
    from shmgan_amd.data import PSD_SUBDIRS
    _write(tmp_path / "data", PSD_SUBDIRS, [(40, 56)] * 3, 54)
    args = argparse.Namespace(mode="train", image_size=64, batch_size=1, filter_size=16, num_epochs=2, data_dir=str(tmp_path / "data"),
                              checkpoint_save_dir=str(tmp_path / "ckpt"), log_dir=str(tmp_path / "logs"), checkpoint_save_step=10,
                              cache="device", cache_gb=0.25)
    m = ShmGANwithSSpecSeg(args)
    assert m.train(args, max_steps=4, print_fn=lambda *a: None) == 4
    ds = m.loadedDataset
    assert ds.cache == "device" and ds.cache_bytes == 2 ** 28
    st = ds.cache_stats()
    assert set(st) == {"resident", "bytes", "chunks", "hits", "misses", "refused"}
    assert st["resident"] == 3 and st["hits"] >= 1 and 0 < st["bytes"] <= 2 ** 28 and st["refused"] == 0
    assert np.isfinite(m.losses()["total_Generator_loss"])
