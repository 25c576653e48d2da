"""The mask network's augmenting pair loader on the device.

Kernel level (shm_augment_pairs_u8): y bit for bit against shm_augment_views_u8 fed a 3-channel copy of the mask (and, at identity
parameters, against shm_resize_bilinear_u8); x against the float64 restatement of tests/pairs_ref.py and against today's path on the
device (the RGB plane of shm_augment_views_u8, then shm_rgb2yuv_std, channel 0); batches of 1, 8 and 9 with mixed source sizes;
special images; reproducibility and independence of the slot; the refusals.  Dataset level: MaskDataset's defaults bit for bit
against the existing kernels, the augmented batches against the restatement of the draws, a budget that refuses pairs, the polar
against the directory source.  Then SpecSeg.fit / evaluate on a dataset, validation, and the trainer's options.

Bounds.  x: the rule of DESIGN.md section 6b as pairs_ref.compare states it -- the larger of 1e-5 of the reference's max-abs and four
times the error the float32 restatement shows against float64 on the same inputs.  y against float64: polar_ref.bound.  The device
against today's device path: the same x bound (both are held to the float64 restatement by it); whether the two also agree bit
for bit is printed per case ("bitwise x"), not asserted: today's path adds its sums with atomics.  Everything else is bitwise.
Every figure is printed before it is asserted."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import augment_ref as ar
import pairs_ref as pf
from oracle.specseg_torch import init_specseg

pytestmark = pytest.mark.gpu

SENTINEL = -7.0
NAN = float("nan")


def _ops():
    from shmgan_amd import ops
    return ops


@functools.lru_cache(maxsize=None)
def _dev_pair(hin, win, k=0, kind="random"):
    """The pair of pairs_ref.images on the device (shared by the tests; never written)."""
    img, mask = pf.images(hin, win, k, kind)
    return torch.from_numpy(img.copy()).cuda(), torch.from_numpy(mask.copy()).cuda()


def _sample(hin, win, k=0, kind="random", crop=None, flip_ud=False, flip_lr=False):
    from shmgan_amd.cache import AugSample
    return AugSample(_dev_pair(hin, win, k, kind), hin, win, crop, flip_ud, flip_lr)


def _pairs(samples, ho, wo, fill=NAN, n_out=None, ws_fill=NAN):
    """(x, y, scale) of one ops.augment_pairs_u8 call.  The outputs are filled before it (every element must be written) and so is
    the workspace (it needs no initial value)."""
    ops = _ops()
    n = n_out or len(samples)
    x, y = torch.full((n, ho, wo, 1), fill, device="cuda"), torch.full((n, ho, wo, 1), fill, device="cuda")
    scale = torch.full((n,), fill, device="cuda")
    ws = torch.full((max(ops.augment_pairs_ws_doubles(max(len(samples), 1), ho, wo), 1),), ws_fill, dtype=torch.float64, device="cuda")
    ops.augment_pairs_u8(samples, x, y, ws, scale)
    return x, y, scale


def _todays_path(s, ho, wo):
    """(x, y, scale) of one sample from the kernels that were there before: shm_augment_views_u8 (SHM_AUG_DIR) on five copies of the
    image, then shm_rgb2yuv_std, channel 0; and the same kernel on a 3-channel copy of the mask, any channel."""
    ops = _ops()
    img, mask = s.srcs
    rgb = [torch.full((ho, wo, 3), NAN, device="cuda") for _ in range(5)]
    ops.augment_views_u8([img] * 5, rgb, "dir", None, None, s.crop, s.flip_ud, s.flip_lr, 1.0 / 255.0)
    m3 = mask.reshape(s.hin, s.win, 1).expand(s.hin, s.win, 3).contiguous()
    mk = [torch.full((ho, wo, 3), NAN, device="cuda") for _ in range(5)]
    ops.augment_views_u8([m3] * 5, mk, "dir", None, None, s.crop, s.flip_ud, s.flip_lr, 1.0 / 255.0)
    assert torch.equal(mk[4][..., 0], mk[4][..., 2]) and torch.equal(mk[4], mk[0])
    yuv, acc, scale = torch.empty((1, ho, wo, 3), device="cuda"), torch.zeros(2, dtype=torch.float64, device="cuda"), torch.empty(1, device="cuda")
    ops.rgb2yuv_std(rgb[4].reshape(1, ho, wo, 3), yuv, acc, scale, 1, ho * wo)
    return yuv[0, ..., 0:1].contiguous(), mk[4][..., 0:1].contiguous(), scale


CASES = [(src, out, name, "random") for src, out in pf.SHAPES for name in pf.VARIANTS] + \
        [(src, out, name, kind) for src, out in pf.SHAPES for name in ("identity", "crop_flip_lr") for kind in ("const", "zeros", "ones")]


# ------------------------------------------------------------------------------------------------ the kernel, one sample
@pytest.mark.parametrize("src,out,name,kind", CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_one_sample_against_float64_and_todays_kernels(src, out, name, kind):
    ops = _ops()
    (hin, win), (ho, wo) = src, out
    crop, fud, flr = pf.variant(name, hin, win)
    s = _sample(hin, win, 0, kind, crop, fud, flr)
    x, y, scale = _pairs([s], ho, wo)
    img, mask = pf.images(hin, win, 0, kind)
    label = f"pairs {src}->{out} {name} {kind}"
    # y: the plane shm_augment_views_u8 writes for a 3-channel copy of the mask, bit for bit; at identity parameters shm_resize_bilinear_u8's
    tx, ty, tscale = _todays_path(s, ho, wo)
    assert torch.isfinite(ty).all() and torch.equal(y[0], ty), label
    if name == "identity":
        want = torch.full((ho, wo, 1), NAN, device="cuda")
        ops.resize_bilinear_u8(s.srcs[1].reshape(hin, win, 1), want, 1.0 / 255.0, False)
        assert torch.equal(y[0], want), label
    # x and y against the float64 restatement
    ok, text = pf.compare(x[0].cpu().numpy(), y[0].cpu().numpy(), img, mask, ho, wo, crop, fud, flr, label=label)
    print(text)
    assert ok, text
    # x against today's path on the device, under the bound both are held to against float64
    x64, _, s64 = pf.pair(img, mask, ho, wo, crop, fud, flr, np.float64)
    x32, _, _ = pf.pair(img, mask, ho, wo, crop, fud, flr, np.float32)
    bound = pf.x_bound(x64, np.abs(x32 - x64).max())
    err = float((x[0] - tx).abs().max())
    print(f"{label}: x against today's device path: {err:.3e}, bound {bound:.3e}; bitwise x: {torch.equal(x[0], tx)}; "
          f"scale {float(scale[0])!r} today's {float(tscale[0])!r} float64 {s64!r}")
    assert torch.isfinite(tx).all() and err <= bound, (label, err, bound)
    assert abs(float(scale[0]) - s64) <= 1e-6 * s64
    if kind == "const":
        assert float(scale[0]) == 1.0 / 256.0 and torch.isfinite(x).all() and float(x.abs().max()) > 1.0, label
    if kind == "zeros":
        assert bool((y == 0).all()), label
    if kind == "ones":
        assert bool((y == float(np.float32(255.0) * pf.BYTE)).all()) and float(y.max()) <= 1.0, label


# ------------------------------------------------------------------------------------------------ batches
SIZES9 = [(37, 53), (9, 7), (40, 24), (5, 5), (16, 16), (37, 53), (24, 40), (9, 7), (33, 21)]


def _batch_samples(n):
    out = []
    for i, (hin, win) in enumerate(SIZES9[:n]):
        crop, fud, flr = pf.variant(pf.VARIANTS[i % len(pf.VARIANTS)], hin, win)
        out.append(_sample(hin, win, i, ("random", "random", "const", "zeros")[i % 4] if i else "random", crop, fud, flr))
    return out


@pytest.mark.parametrize("ho,wo", [(16, 16), (17, 19), (32, 32)])
@pytest.mark.parametrize("n", [1, 8, 9])
def test_a_batch_is_its_samples_alone_bitwise(n, ho, wo):
    samples = _batch_samples(n)
    x, y, scale = _pairs(samples, ho, wo)
    assert torch.isfinite(x).all() and torch.isfinite(y).all() and torch.isfinite(scale).all()
    for i, s in enumerate(samples):
        x1, y1, s1 = _pairs([s], ho, wo)
        assert torch.equal(x[i], x1[0]) and torch.equal(y[i], y1[0]) and torch.equal(scale[i], s1[0]), (n, i)
    # two calls give the same bits, whatever the workspace held
    x2, y2, scale2 = _pairs(samples, ho, wo, ws_fill=123.0)
    assert torch.equal(x, x2) and torch.equal(y, y2) and torch.equal(scale, scale2)
    # one sample of the batch against the float64 restatement (the others are the single-sample test's cases)
    j = n - 1
    img, mask = pf.images(samples[j].hin, samples[j].win, j, ("random", "random", "const", "zeros")[j % 4] if j else "random")
    ok, text = pf.compare(x[j].cpu().numpy(), y[j].cpu().numpy(), img, mask, ho, wo, samples[j].crop, samples[j].flip_ud, samples[j].flip_lr,
                          label=f"batch of {n}, sample {j}, {ho}x{wo}")
    print(text)
    assert ok, text


def test_more_pixels_than_one_sweep_of_the_capped_grid():
    """300 x 260 outputs are 78000 pixels: 256 blocks per sample, and the first 12464 threads of a sample take a second pixel"""
    ops = _ops()
    ho, wo = 300, 260
    assert ops.augment_pairs_ws_doubles(2, ho, wo) == 2 * 256 * 2 == ops.augment_pairs_ws_doubles(2, 256, 256)
    samples = [_sample(37, 53, 0, "random", pf.edge_crop(37, 53), True, False), _sample(9, 7, 1, "random", None, False, True)]
    x, y, scale = _pairs(samples, ho, wo)
    for i, s in enumerate(samples):
        tx, ty, tscale = _todays_path(s, ho, wo)
        assert torch.equal(y[i], ty)
        img, mask = pf.images(s.hin, s.win, i)
        ok, text = pf.compare(x[i].cpu().numpy(), y[i].cpu().numpy(), img, mask, ho, wo, s.crop, s.flip_ud, s.flip_lr, label=f"{s.hin}x{s.win} -> {ho}x{wo}")
        print(text, f"; bitwise x against today's device path: {torch.equal(x[i], tx)}; scale {float(scale[i])!r} today's {float(tscale[0])!r}")
        assert ok, text
        x1, y1, s1 = _pairs([s], ho, wo)
        assert torch.equal(x[i], x1[0]) and torch.equal(y[i], y1[0]) and torch.equal(scale[i], s1[0])


def test_a_samples_bits_do_not_depend_on_slot_or_neighbours():
    nine = _batch_samples(9)
    s = _sample(40, 24, 3, "random", pf.edge_crop(40, 24), True, False)
    alone = _pairs([s], 17, 19)
    other = nine[:7] + [s] + nine[8:]
    at7 = _pairs(other, 17, 19)
    assert all(torch.equal(a[0], b[7]) for a, b in zip(alone, at7))
    at0 = _pairs([s] + nine[:3], 17, 19)                   # slot 0 of 4, other neighbours
    assert all(torch.equal(a[0], b[0]) for a, b in zip(alone, at0))
    # fewer samples than the tensors hold: the slices past them stay as they were
    x, y, scale = _pairs(nine[:2], 16, 16, fill=SENTINEL, n_out=3)
    assert bool((x[2] == SENTINEL).all()) and bool((y[2] == SENTINEL).all()) and float(scale[2]) == SENTINEL and bool((y[:2] != SENTINEL).all())


def test_addresses_instead_of_tensors_and_a_mask_with_a_channel_axis():
    from shmgan_amd.cache import AugSample
    img, mask = _dev_pair(37, 53)
    want = _pairs([AugSample((img, mask), 37, 53, None, True, False)], 16, 16)
    got = _pairs([AugSample((img.data_ptr(), mask.data_ptr()), 37, 53, None, True, False)], 16, 16)
    got1 = _pairs([AugSample((img, mask.reshape(37, 53, 1)), 37, 53, (0.0, 0.0, 37.0, 53.0), True, False)], 16, 16)
    assert all(torch.equal(a, b) and torch.equal(a, c) for a, b, c in zip(want, got, got1))
    with pytest.raises(ValueError, match="mask of sample 0"):
        _pairs([AugSample((img, mask[:36].contiguous()), 37, 53)], 16, 16)


def test_refusals_name_the_sample_and_launch_nothing():
    from shmgan_amd._lib import ShmError
    ops = _ops()
    good = _batch_samples(9)
    img, mask = good[1].srcs
    cases = [([], 16, "n 0 < 1"),
             ([good[0], good[1]._replace(srcs=(0, mask)), good[2]], 16, "sample 1: null pointer (image)"),
             ([good[0], good[1], good[2]._replace(srcs=(good[2].srcs[0], 0))], 16, "sample 2: null pointer (mask)"),
             ([good[0], good[1]._replace(srcs=(img.data_ptr(), mask.data_ptr()), hin=0)], 16, "sample 1: sizes hin 0, win 7 outside [1, 32768]"),
             ([good[0]._replace(srcs=tuple(t.data_ptr() for t in good[0].srcs), win=32769)], 16, "sample 0: sizes hin 37, win 32769"),
             ([good[0], good[1]._replace(crop=(2.5, 0.0, 7.0, 7.0))], 16, "sample 1: the crop 7 x 7 at (2.5, 0) does not lie inside the 9 x 7 image"),
             ([good[0], good[1]._replace(crop=(0.0, NAN, 4.0, 4.0))], 16, "sample 1: the crop"),
             ([good[0]._replace(crop=(0.0, 0.0, NAN, 8.0))], 16, "sample 0: empty crop"),
             ([good[0]._replace(crop=(0.0, 0.0, 8.0, 0.0))], 16, "sample 0: empty crop"),
             (good[:8] + [good[8]._replace(crop=(0.0, -0.5, 8.0, 8.0))], 16, "sample 8: the crop"),         # in the SECOND group of the call
             (good[:2], 32769, "sizes ho 16, wo 32769 outside")]
    for samples, wo, msg in cases:
        x, y = torch.full((9, 16, 16, 1), SENTINEL, device="cuda"), torch.full((9, 16, 16, 1), SENTINEL, device="cuda")
        ws = torch.zeros(64, dtype=torch.float64, device="cuda")
        with pytest.raises(ShmError) as e:
            if wo == 16:
                ops.augment_pairs_u8(samples, x, y, ws)
            else:                   # sizes the tensors do not have: the entry point itself, which refuses them before anything else
                _raw_call(samples, x, y, ws, 16, wo, 256)
        assert "(-1)" in str(e.value) and msg in str(e.value) and "shm_augment_pairs_u8" in str(e.value), str(e.value)
        torch.cuda.synchronize()
        assert bool((x == SENTINEL).all()) and bool((y == SENTINEL).all()) and bool((ws == 0).all()), msg
    # null outputs or workspace, and a stride below a plane, through the C entry point itself
    x, y = torch.full((2, 16, 16, 1), SENTINEL, device="cuda"), torch.full((2, 16, 16, 1), SENTINEL, device="cuda")
    ws = torch.zeros(64, dtype=torch.float64, device="cuda")
    for kw, msg in ((dict(x=None), "null pointer"), (dict(y=None), "null pointer"), (dict(ws=None), "null pointer"),
                    (dict(stride=255), "sample_stride 255 is less than a plane of 16 x 16")):
        with pytest.raises(ShmError, match="shm_augment_pairs_u8") as e:
            _raw_call(good[:2], kw.get("x", x), kw.get("y", y), kw.get("ws", ws), 16, 16, kw.get("stride", 256))
        assert msg in str(e.value)
        torch.cuda.synchronize()
        assert bool((x == SENTINEL).all()) and bool((y == SENTINEL).all())
    # the wrapper's own checks
    with pytest.raises(ValueError, match="ws must be"):
        ops.augment_pairs_u8(good[:2], x, y, torch.zeros(1, dtype=torch.float64, device="cuda"))
    with pytest.raises(ValueError, match="2 samples|3 samples"):
        ops.augment_pairs_u8(good[:3], x, y)


def _raw_call(samples, x, y, ws, ho, wo, stride):
    """shm_augment_pairs_u8 without the wrapper's shape checks."""
    from shmgan_amd import _lib
    ops = _ops()
    arr = (ops._pair_sample_struct() * max(len(samples), 1))()
    for i, s in enumerate(samples):
        arr[i].image, arr[i].mask = (t.data_ptr() if isinstance(t, torch.Tensor) else t for t in s.srcs)
        arr[i].hin, arr[i].win = s.hin, s.win
        arr[i].crop_y, arr[i].crop_x, arr[i].crop_h, arr[i].crop_w = s.crop or (0.0, 0.0, float(s.hin), float(s.win))
        arr[i].flip_ud, arr[i].flip_lr = int(s.flip_ud), int(s.flip_lr)
    p = lambda t: None if t is None else t.data_ptr()
    _lib.check(_lib.lib().shm_augment_pairs_u8(arr, len(samples), p(x), p(y), stride, ho, wo, p(ws), None, torch.cuda.current_stream().cuda_stream),
               "shm_augment_pairs_u8")


# ------------------------------------------------------------------------------------------------ the dataset
S, B, N = 32, 4, 6
SOURCE_SIZES = [(40, 56), (37, 53)]


def _write_capture(root, subdirs, n, seed):
    """n samples of four views in two source sizes: noise, plus a strongly polarised rectangle (bright at 0 degrees, dark at 90) so
    that the specular mask is neither empty nor full."""
    from PIL import Image
    rng = np.random.default_rng(seed)
    for sub in subdirs:
        (root / sub).mkdir(parents=True, exist_ok=True)
    for i in range(n):
        h, w = SOURCE_SIZES[i % 2]
        base = rng.integers(30, 90, (h, w, 3))
        y0, x0 = int(rng.integers(2, h // 2)), int(rng.integers(2, w // 2))
        for v, sub in enumerate(subdirs):
            a = base + rng.integers(0, 12, (h, w, 3))
            a[y0:y0 + h // 3, x0:x0 + w // 3] += (150, 75, 0, 75)[v]
            Image.fromarray(np.clip(a, 0, 255).astype(np.uint8)).save(root / sub / f"s_{(7 * i) % n:02d}.png")
    return str(root)


@pytest.fixture(scope="module")
def capture(tmp_path_factory):
    """(root, mask directory, {name: (view-2 image, mask)} as host arrays) of a PSD capture with the masks of
    polar.write_specular_masks; made once, never changed."""
    from PIL import Image
    from shmgan_amd import polar
    from shmgan_amd.data import PSD_SUBDIRS
    root = tmp_path_factory.mktemp("pairs_capture")
    _write_capture(root, PSD_SUBDIRS[:4], N, 61)
    masks = root / "masks"
    written = polar.write_specular_masks(str(root), str(masks))
    assert len(written) == N
    pairs = {}
    for f in sorted(masks.glob("*.png")):
        with Image.open(root / "I90" / f.name) as im:
            img = np.asarray(im.convert("RGB"), dtype=np.uint8)
        with Image.open(f) as im:
            mk = np.asarray(im.convert("L"), dtype=np.uint8)
        assert 0 < mk.mean() < 255 and img.shape[:2] == mk.shape
        pairs[f.stem] = (img, mk)
    return str(root), str(masks), pairs


def _polar(capture, **kw):
    from shmgan_amd.data import MaskDataset
    return MaskDataset.from_polar(capture[0], S, kw.pop("batch_size", B), **kw)


def _dirs(capture, **kw):
    from shmgan_amd.data import MaskDataset
    return MaskDataset(capture[0] + "/I90", capture[1], S, kw.pop("batch_size", B), **kw)


def _aug():
    from shmgan_amd.data import Augment
    return Augment(flip_lr=0.5, flip_ud=0.5, crop_min=0.4)


class _Counts:
    """Counts the ops wrappers a MaskDataset may call."""
    NAMES = ("resize_bilinear_u8", "rgb2yuv_std", "augment_pairs_u8", "specmask")

    def __init__(self, monkeypatch):
        ops = _ops()
        self.n = dict.fromkeys(self.NAMES, 0)
        for name in self.NAMES:
            monkeypatch.setattr(ops, name, self._counted(name, getattr(ops, name)))

    def _counted(self, name, fn):
        def call(*a, **kw):
            self.n[name] += 1
            return fn(*a, **kw)
        return call

    def take(self):
        out, self.n = self.n, dict.fromkeys(self.n, 0)
        return out


@pytest.mark.parametrize("flip_ud", [False, True])
def test_defaults_are_the_existing_kernels_bitwise(capture, monkeypatch, flip_ud):
    ops = _ops()
    names = sorted(capture[2])
    rgb, want_y = torch.empty((N, S, S, 3), device="cuda"), torch.empty((N, S, S, 1), device="cuda")
    for k, nm in enumerate(names):
        img, mk = (torch.from_numpy(a.copy()).cuda() for a in capture[2][nm])
        ops.resize_bilinear_u8(img, rgb[k], 1.0 / 255.0, flip_ud)
        ops.resize_bilinear_u8(mk.unsqueeze(2), want_y[k], 1.0 / 255.0, flip_ud)
    yuv, acc, scale = torch.empty_like(rgb), torch.zeros(2 * N, dtype=torch.float64, device="cuda"), torch.empty(N, device="cuda")
    ops.rgb2yuv_std(rgb, yuv, acc, scale, N, S * S)
    want_x = yuv[..., 0:1].contiguous()
    c = _Counts(monkeypatch)
    for make in (_polar, _dirs):
        ds = make(capture, flip_ud=flip_ud)
        assert not ds.active and ds.names == names and len(ds) == 2
        x, y = ds.tensors()
        n = c.take()
        assert (n["resize_bilinear_u8"], n["rgb2yuv_std"], n["augment_pairs_u8"]) == (2 * N, 1, 0), n
        assert torch.equal(x, want_x) and torch.equal(y, want_y), make.__name__
        got = list(ds)
        assert [tuple(b[0].shape) for b in got] == [(4, S, S, 1), (2, S, S, 1)]
        assert torch.equal(torch.cat([b[0] for b in got]), want_x) and torch.equal(torch.cat([b[1] for b in got]), want_y)
        assert torch.equal(ds.batch(1, 3)[0], want_x[4:]) and torch.equal(ds.batch(0)[1], want_y[:4])
        assert sum(c.take().values()) == 0                                              # loaded once
        assert ds.cache_stats() == {"resident": 0, "bytes": 0, "chunks": 0, "hits": 0, "misses": 0, "refused": 0}


def test_augmented_batches_are_the_restatement_of_the_draws(capture, monkeypatch):
    names = sorted(capture[2])
    aug = _aug()
    ds = _polar(capture, augment=aug, shuffle=True, seed=6, flip_ud=True)
    c = _Counts(monkeypatch)
    seen_flips = set()
    for p in (0, 1, 2):
        order = [int(v) for v in ar.order(N, 6, p, True)]
        got_positions = []
        for i in range(len(ds)):
            x, y = ds.batch(i, p)
            n = c.take()
            assert n["augment_pairs_u8"] == 1 and n["resize_bilinear_u8"] == 0 and n["rgb2yuv_std"] == 0, n           # ONE call per batch
            pos = order[i * B:(i + 1) * B]
            assert ds.positions(i, p) == pos and tuple(x.shape) == tuple(y.shape) == (len(pos), S, S, 1)
            got_positions += pos
            for b, k in enumerate(pos):
                img, mk = capture[2][names[k]]
                crop, fud, flr, _ = ar.draw(6, p, k, *img.shape[:2], flip_lr=aug.flip_lr, flip_ud=aug.flip_ud, crop_min=aug.crop_min)
                seen_flips.add((fud, flr))
                ok, text = pf.compare(x[b].cpu().numpy(), y[b].cpu().numpy(), img, mk, S, S, crop, not fud, flr, label=f"pass {p} batch {i} slot {b} = {names[k]}")
                print(text)
                assert ok, text
        assert sorted(got_positions) == list(range(N)) and len(pos) == N % B == 2                        # every sample once per pass
    assert len(seen_flips) >= 3
    st = ds.cache_stats()
    assert (st["resident"], st["refused"], st["chunks"]) == (N, 0, 1) and st["misses"] == N and st["hits"] == 2 * N, st
    # the draws depend on (seed, pass, position) alone: another batch size, no shuffle, the directory source -- the same bits per sample
    one = _dirs(capture, batch_size=1, augment=aug, seed=6, flip_ud=True)
    for p in (0, 2):
        for i in range(len(ds)):
            x, y = ds.batch(i, p)
            for b, k in enumerate(ds.positions(i, p)):
                x1, y1 = one.batch(k, p)
                assert torch.equal(x[b], x1[0]) and torch.equal(y[b], y1[0]), (p, i, b)
    assert not torch.equal(ds.batch(0, 0)[0], ds.batch(0, 1)[0])
    other = _polar(capture, augment=aug, shuffle=True, seed=7, flip_ud=True)
    assert not torch.equal(other.batch(0, 0)[0], ds.batch(0, 0)[0])
    # shuffle alone: the identity crop in the pass's order is the default tensors, bit for bit in y
    plain = _polar(capture, shuffle=True, seed=6)
    xs, ys = _polar(capture).tensors()
    idx = torch.tensor(plain.positions(0, 4), device="cuda")
    x, y = plain.batch(0, 4)
    assert plain.active and torch.equal(y, ys.index_select(0, idx)) and torch.allclose(x, xs.index_select(0, idx), rtol=1e-5, atol=1e-6)


def test_a_budget_that_refuses_pairs_gives_the_same_batches(capture, monkeypatch):
    from shmgan_amd.cache import sample_bytes
    aug = _aug()
    full = _polar(capture, augment=aug, shuffle=True, seed=3)
    want = [[full.batch(i, p) for i in range(len(full))] for p in range(3)]
    budget = sample_bytes(2, *SOURCE_SIZES[0]) + sample_bytes(2, *SOURCE_SIZES[1])              # two pairs
    c = _Counts(monkeypatch)
    small = _polar(capture, augment=aug, shuffle=True, seed=3, cache_bytes=budget)
    for p in range(3):
        for i in range(len(small)):
            x, y = small.batch(i, p)
            assert torch.equal(x, want[p][i][0]) and torch.equal(y, want[p][i][1]), (p, i)
        n = c.take()
        assert n["specmask"] == (N if p == 0 else N - 2) and n["augment_pairs_u8"] == 2, (p, n)       # a refused pair's mask is made again
        st = small.cache_stats()
        assert st["resident"] == 2 and st["refused"] == N - 2 > 0 and st["bytes"] <= budget, st
    none = _polar(capture, augment=aug, shuffle=True, seed=3, cache_bytes=0)
    assert torch.equal(none.batch(1, 2)[0], want[2][1][0]) and none.cache_stats()["resident"] == 0 and none.cache_stats()["refused"] == 2


def test_the_polar_and_the_directory_source_give_the_same_batches(capture):
    from shmgan_amd.data import Augment, MaskDataset
    aug = _aug()
    a, b = _polar(capture, augment=aug, shuffle=True, seed=11), _dirs(capture, augment=aug, shuffle=True, seed=11)
    assert a.names == b.names
    for p in (0, 1):
        for i in range(len(a)):
            (xa, ya), (xb, yb) = a.batch(i, p), b.batch(i, p)
            assert torch.isfinite(xa).all() and torch.equal(xa, xb) and torch.equal(ya, yb), (p, i)
    assert [tuple(t[0].shape) for t in a] == [(4, S, S, 1), (2, S, S, 1)]                         # iteration: the batches of first_pass
    assert torch.equal(next(iter(a))[0], a.batch(0, 0)[0])
    with pytest.raises(ValueError, match=r"view 2.*views=\"keep\""):
        MaskDataset.from_polar(capture[0], S, B, angles=[0, 30, 60, 120], augment=Augment(flip_lr=0.5))
    keep = MaskDataset.from_polar(capture[0], S, B, angles=[0, 30, 60, 120], augment=Augment(flip_lr=0.5, views="keep"))
    assert tuple(keep.batch(0, 0)[0].shape) == (4, S, S, 1)


def test_image_and_mask_of_other_sizes_raise_when_augmented(capture, tmp_path):
    from PIL import Image
    from shmgan_amd.data import MaskDataset
    for sub in ("img", "msk"):
        (tmp_path / sub).mkdir()
    Image.fromarray(np.zeros((20, 24, 3), np.uint8)).save(tmp_path / "img" / "a.png")
    Image.fromarray(np.zeros((20, 25), np.uint8)).save(tmp_path / "msk" / "a.png")
    assert tuple(MaskDataset(str(tmp_path / "img"), str(tmp_path / "msk"), S).tensors()[0].shape) == (1, S, S, 1)      # resized apart: fine
    with pytest.raises(ValueError, match="same decoded size"):
        MaskDataset(str(tmp_path / "img"), str(tmp_path / "msk"), S, shuffle=True).batch(0)


# ------------------------------------------------------------------------------------------------ fit, evaluate, validation
def _net():
    from shmgan_amd.model import Arena
    from shmgan_amd.specseg import SpecSeg
    d = torch.device("cuda")
    net = SpecSeg(S, d, Arena(d))
    net.set_weights(init_specseg(trained_like=True))
    return net


def _state(net):
    return net.flat.clone(), net.m.clone(), net.v.clone()


def _same_state(a, b):
    return all(torch.equal(p, q) for p, q in zip(_state(a), _state(b))) and a.iterations == b.iterations


def test_fit_on_a_dataset_is_the_loop_of_train_steps_bitwise(capture):
    ds = _dirs(capture, augment=_aug(), shuffle=True, seed=2)
    a, b = _net(), _net()
    lines = []
    hist = a.fit(ds, epochs=2, lr=1e-3, seed=5, print_fn=lines.append)
    assert a.iterations == 4 and len(hist["loss"]) == 2 and len(lines) == 2 and "val_loss" not in hist
    b.configure_optimizer(1e-3)
    b.trainable, b.train_seed = True, 5
    rows = []
    for p in range(2):
        recs = [(b.train_step(*ds.batch(i, p)), len(ds.positions(i, p))) for i in range(len(ds))]
        rows.append((sum(r.out * k for r, k in recs) / N).cpu().numpy())
    assert _same_state(a, b)
    assert [hist["loss"][p] for p in range(2)] == [float(rows[p][0]) for p in range(2)]
    with pytest.raises(ValueError, match="y must be None"):
        a.fit(ds, ds.tensors()[1])
    with pytest.raises(ValueError, match="needs y"):
        a.fit(ds.tensors()[0])
    # tensors as before: positional x, y
    x, y = ds.tensors()
    c, d = _net(), _net()
    c.fit(x, y, 4, 1, 1e-3)
    d.fit(x, y=y, batch_size=4, epochs=1, lr=1e-3)
    assert _same_state(c, d) and c.iterations == 2


def test_a_resumed_fit_goes_on_with_the_next_pass(capture, tmp_path):
    from shmgan_amd import ShmGANwithSSpecSeg
    ds = _dirs(capture, augment=_aug(), shuffle=True, seed=2)

    def trainer():
        m = ShmGANwithSSpecSeg(image_size=S, filter_size=16, batch_size=1)
        m.build()
        return m
    a, b = trainer(), trainer()
    a.SpecSeg.fit(ds, epochs=2, lr=1e-3)
    b.SpecSeg.fit(ds, epochs=1, lr=1e-3)
    assert not _same_state(a.SpecSeg, b.SpecSeg)
    b.save_npz(tmp_path / "ck.npz")
    c = trainer()
    c.load_npz(tmp_path / "ck.npz")
    assert c.SpecSeg.iterations == 2 == len(ds)
    c.SpecSeg.fit(ds, epochs=1, lr=1e-3)                     # first_pass = 2 // 2 = 1: the order and draws of pass 1
    assert _same_state(a.SpecSeg, c.SpecSeg)


def test_validation_reports_evaluate_and_leaves_training_alone(capture):
    full = _dirs(capture, augment=_aug(), shuffle=True, seed=2)
    train, val = full.split(1 / 3, seed=1)
    assert len(train.names) == 4 and len(val.names) == 2 and not val.active and train.active
    a, b, c = _net(), _net(), _net()
    lines = []
    hist = {}
    for ep in range(2):                                      # one epoch per call: what evaluate says after it is the epoch's val_ row
        h = a.fit(train, epochs=1, lr=1e-3, validation_data=val, print_fn=lines.append)
        ev = a.evaluate(val)
        assert {k: h["val_" + k][0] for k in ev} == ev and set(h) == {"loss", "dice", "focal", "iou", "f1"} | {"val_" + k for k in ev}
        assert ev == a.evaluate(*val.tensors(), batch_size=val.B)
        hist[ep] = h
    assert all("val_loss" in ln and "val_f1" in ln for ln in lines) and len(lines) == 2
    hb = b.fit(train, epochs=2, lr=1e-3)                     # the same training without validation: the same weights
    assert _same_state(a, b) and hb["loss"] == [hist[0]["loss"][0], hist[1]["loss"][0]]
    hc = c.fit(train, epochs=2, lr=1e-3, validation_data=val.tensors())          # an (xv, yv) pair; both epochs in one call
    assert _same_state(a, c) and hc["val_loss"] == [hist[0]["val_loss"][0], hist[1]["val_loss"][0]]
    with pytest.raises(ValueError, match="y must be None"):
        a.evaluate(val, val.tensors()[1])


# ------------------------------------------------------------------------------------------------ the trainer
def _trainer():
    from shmgan_amd import ShmGANwithSSpecSeg
    return ShmGANwithSSpecSeg(image_size=S, filter_size=16, batch_size=1)


def test_trainer_defaults_take_todays_path(capture, monkeypatch):
    from shmgan_amd.data import MaskDataset
    args = SimpleNamespace(specseg_image_dir=capture[0] + "/I90", specseg_mask_dir=capture[1], specseg_epochs=2, specseg_lr=1e-3, specseg_batch_size=B)
    m, ref = _trainer(), _trainer()
    c = _Counts(monkeypatch)
    hist = m.train_specseg(args, print_fn=lambda *a: None)
    assert c.take()["augment_pairs_u8"] == 0 and m.specseg_datasets is None
    ref.SpecSeg = ref.build_specseg()
    x, y = MaskDataset(args.specseg_image_dir, args.specseg_mask_dir, S, B, device=ref.device).tensors()
    want = ref.SpecSeg.fit(x, y, batch_size=B, epochs=2, lr=1e-3, beta1=ref.beta1, beta2=ref.beta2, shuffle=True)
    assert hist == want and _same_state(m.SpecSeg, ref.SpecSeg)
    from shmgan_amd.trainer import _DEFAULTS as d
    assert [d[k] for k in ("specseg_aug_flip_lr", "specseg_aug_flip_ud", "specseg_aug_crop_min", "specseg_aug_views", "specseg_shuffle",
                           "specseg_data_seed", "specseg_val_fraction", "specseg_cache_gb")] == [0.0, 0.0, 1.0, "physical", False, 0, 0.0, None]


@pytest.mark.parametrize("source", ["dir", "polar"])
def test_trainer_options_reach_the_datasets(capture, source):
    from shmgan_amd.data import Augment, split_names
    args = SimpleNamespace(specseg_mask_source=source, specseg_image_dir=capture[0] + "/I90", specseg_mask_dir=capture[1], data_dir=capture[0],
                           specseg_epochs=1, specseg_lr=1e-3, specseg_batch_size=2, specseg_aug_flip_lr=0.5, specseg_aug_crop_min=0.6,
                           specseg_shuffle=True, specseg_data_seed=4, specseg_val_fraction=0.34, specseg_cache_gb=0.25)
    m = _trainer()
    ds = m.specseg_dataset(args)
    assert ds.augment == Augment(0.5, 0.0, 0.6, "physical") and ds.shuffle and ds.seed == 4 and ds.cache_bytes == 2 ** 28 and ds.B == 2
    assert (ds._polar is not None) == (source == "polar")
    lines = []
    hist = m.train_specseg(args, print_fn=lines.append)
    train, val = m.specseg_datasets
    assert (train.names, val.names) == split_names(sorted(capture[2]), 0.34, 4) and len(val.names) == 2
    assert train.augment == ds.augment and train.shuffle and train.seed == 4 and val.augment is None and not val.shuffle
    assert len(hist["loss"]) == len(hist["val_loss"]) == 1 and np.isfinite(hist["val_loss"][0]) and "val_dice" in lines[0]
    assert m.SpecSeg.iterations == 2 and train.cache_stats()["resident"] == 4 and val.cache_stats()["resident"] == 0
    # a split alone keeps the tensor path for the training side
    m2 = _trainer()
    h2 = m2.train_specseg(SimpleNamespace(**{**vars(args), "specseg_aug_flip_lr": 0.0, "specseg_aug_crop_min": 1.0, "specseg_shuffle": False}),
                          print_fn=lambda *a: None)
    assert not m2.specseg_datasets[0].active and len(h2["val_loss"]) == 1 and m2.specseg_datasets[0].cache_stats()["resident"] == 0
