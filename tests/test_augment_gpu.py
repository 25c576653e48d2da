"""Train-time augmentation on the device: shm_augment_views_u8 against the kernels it must equal bit for bit at identity
parameters, against the float64 restatement (tests/augment_ref.py) for crops, mirrors and the view mix, the loader with
`shuffle` / `augment` end to end, and the trainer options.

Tolerances: polar_ref.bound -- the larger of 2e-6 and four times the error the float32 restatement shows against float64 on the
same inputs (printed).  Where the definition gives exact numbers (weights of zero, a permutation of planes, the same draw twice)
the comparison is bitwise."""
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
FLIPS = [(False, False), (False, True), (True, False), (True, True)]


@functools.lru_cache(maxsize=None)
def _images(hin, win):
    """Five random byte images of one sample (shared by the tests of a size; never modified)."""
    rng = np.random.default_rng(1000 * hin + win)
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


def _run(images, ho, wo, mode, mix=None, crop=None, flip_ud=False, flip_lr=False, scale=1.0 / 255.0):
    """The five device planes of one call (NaN-filled before it: every element must be written)."""
    from shmgan_amd import ops
    srcs = [torch.from_numpy(a.copy()).cuda() for a in images[:5 if mode == "dir" else 4]]
    planes = torch.full((5, ho, wo, 3), float("nan"), device="cuda")
    ops.augment_views_u8(srcs, list(planes), mode, _psd()[0] if mode == "stokes" else None, mix, crop, flip_ud, flip_lr, scale)
    return planes


def _check(images, ho, wo, mode, what, **kw):
    """Device against the float64 restatement under the bound of the float32 restatement, plane by plane."""
    got = host(_run(images, ho, wo, mode, **kw))
    n = 5 if mode == "dir" else 4
    ref = ar.augment_views(images[:n], ho, wo, MODES[mode], _psd()[0], dtype=np.float64, **kw)
    r32 = ar.augment_views(images[:n], ho, wo, MODES[mode], _psd()[0], dtype=np.float32, **kw)
    assert np.isfinite(got).all()
    for v in range(5):
        e32 = float(np.abs(r32[v] - ref[v]).max())
        err = float(np.abs(got[v] - ref[v]).max())
        print(f"augment {what} {mode} plane {v}: device error {err:.3e}, float32 restatement {e32:.3e}, bound {pr.bound(e32):.3e}")
        assert err <= pr.bound(e32), (what, mode, v, err, e32)
    return got, ref


# ------------------------------------------------------------------------------------------------ identity parameters
@pytest.mark.parametrize("hin,win,ho,wo", [(37, 53, 16, 16), (16, 16, 16, 16), (9, 7, 32, 32), (40, 24, 17, 19), (5, 5, 1, 1)])
def test_identity_parameters_are_the_existing_kernels_bitwise(hin, win, ho, wo):
    from shmgan_amd import ops
    images = _images(hin, win)
    srcs = [torch.from_numpy(a.copy()).cuda() for a in images]
    for flip in (False, True):
        want = torch.full((5, ho, wo, 3), float("nan"), device="cuda")
        for v in range(5):
            ops.resize_bilinear_u8(srcs[v], want[v], 1.0 / 255.0, flip)
        for crop in (None, (0.0, 0.0, float(hin), float(win))):
            assert torch.equal(_run(images, ho, wo, "dir", crop=crop, flip_ud=flip), want), ("dir", flip)
        for mode in ("min", "stokes"):
            ops.polar_views_u8(srcs[:4], list(want), mode, _psd()[0], 1.0 / 255.0, flip)
            assert torch.equal(_run(images, ho, wo, mode, flip_ud=flip), want), (mode, flip)


# ------------------------------------------------------------------------------------------------ crops and mirrors
CROPS = [("top", (0.0, 8.0, 16.0, 24.0), 32, 32), ("bottom", (24.0, 8.0, 16.0, 24.0), 32, 32), ("left", (8.0, 0.0, 16.0, 24.0), 32, 32),
         ("right", (8.0, 32.0, 16.0, 24.0), 32, 32), ("fractional", (3.5, 2.25, 24.0, 40.0), 32, 32),
         ("one_row", (17.25, 4.0, 1.0, 48.0), 32, 32), ("upsample", (10.0, 12.0, 8.0, 16.0), 32, 32),
         ("rect_out", (2.0, 3.0, 36.0, 50.0), 24, 40), ("odd_ratio", (1.3, 2.7, 23.7, 31.3), 17, 19),
         ("whole", (0.0, 0.0, 40.0, 56.0), 32, 32)]


@pytest.mark.parametrize("name,crop,ho,wo", CROPS, ids=[c[0] for c in CROPS])
def test_crops_and_flips_against_float64(name, crop, ho, wo):
    images = _images(40, 56)
    crop = tuple(float(np.float32(v)) for v in crop)
    for fud, flr in FLIPS:
        for mode in ("dir", "stokes"):
            _check(images, ho, wo, mode, f"{name} ud={int(fud)} lr={int(flr)}", crop=crop, flip_ud=fud, flip_lr=flr)
    _check(images, ho, wo, "min", name, crop=crop, flip_lr=True)


def test_integer_crop_of_the_output_size_is_exact():
    images = _images(40, 56)
    crop, sc = (4.0, 8.0, 32.0, 32.0), np.float32(1.0 / 255.0)
    win = [a[4:36, 8:40].astype(np.float32) for a in images]
    for fud, flr in FLIPS:
        got = _run(images, 32, 32, "dir", crop=crop, flip_ud=fud, flip_lr=flr).cpu().numpy()
        for v in range(5):
            assert np.array_equal(got[v], win[v][::-1 if fud else 1, ::-1 if flr else 1] * sc), (fud, flr, v)
    got = _run(images, 32, 32, "min", crop=crop, flip_lr=True, scale=1.0).cpu().numpy()
    assert np.array_equal(got[4], np.minimum.reduce(win[:4])[:, ::-1])


# ------------------------------------------------------------------------------------------------ the view mix
@pytest.mark.parametrize("mode", ["min", "stokes", "dir"])
def test_psd_mix_against_float64_and_the_fifth_plane_is_never_mixed(mode):
    images = _images(40, 56)
    mix = _psd()[1]
    raw = np.asarray(mix, np.float64) @ np.stack([v.reshape(-1) for v in images[:4]]).astype(np.float64)
    assert (raw < 0).mean() > 0.01 and (raw > 255).mean() > 0.01          # the clamp works on both sides
    for kw in (dict(crop=(3.5, 2.25, 24.0, 40.0), flip_lr=True), dict(flip_ud=True), dict()):
        got, ref = _check(images, 32, 32, mode, f"mix {sorted(kw)}", mix=mix, **kw)
        assert 0.0 <= got[:4].min() and got[:4].max() <= 1.0
        plain = _run(images, 32, 32, mode, **kw).cpu().numpy()
        assert np.array_equal(got[4], plain[4].astype(np.float64))
        assert all(np.abs(got[v] - plain[v]).max() > 0.1 for v in range(4))
    # at the source size every weight is 0: the clamped mix of the bytes itself (multiples of 0.25: exact in float32)
    full = _run(images, 40, 56, mode, mix=mix, scale=1.0).cpu().numpy()
    assert np.array_equal(full[:4].reshape(4, -1), np.clip(raw, 0, 255))


# ------------------------------------------------------------------------------------------------ the loader
N, HW, S, B = 6, (40, 56), 32, 2


def _write(root, subdirs, n, seed, same_views=False):
    from PIL import Image
    rng = np.random.default_rng(seed)
    ref = {}
    for i in range(n):
        one = rng.integers(0, 256, (*HW, 3)).astype(np.uint8)
        for v, sub in enumerate(subdirs):
            (root / sub).mkdir(parents=True, exist_ok=True)
            img = one if same_views else rng.integers(0, 256, (*HW, 3)).astype(np.uint8)
            Image.fromarray(img).save(root / sub / f"img_{i:02d}.png")
            ref[(v, i)] = img
    return ref


@pytest.fixture(scope="module")
def capture(tmp_path_factory):
    from shmgan_amd.data import PSD_SUBDIRS
    root = tmp_path_factory.mktemp("augment_capture")
    return str(root), _write(root, PSD_SUBDIRS, N, 41)


def _passes(ds):
    """Every batch of an iteration over `ds`, as host arrays [batch][plane] of [B,S,S,3] (float32, untouched)."""
    return [[t.cpu().numpy() for t in batch] for batch in ds]


@pytest.fixture(scope="module")
def aug():
    from shmgan_amd.data import Augment
    return Augment(flip_lr=0.5, flip_ud=0.5, crop_min=0.4)


@pytest.fixture(scope="module")
def two_passes(capture, aug):
    """Passes 0 and 1 of the augmented "dir" loader (computed once)."""
    from shmgan_amd.data import PolarDataset
    return _passes(PolarDataset(capture[0], S, batch_size=B, rank=0, world=1, epochs=2, augment=aug, seed=5))


@pytest.mark.parametrize("source", ["dir", "min", "stokes"])
def test_augmented_batches_are_the_restatement_of_the_draws(capture, aug, two_passes, source):
    from shmgan_amd.data import PolarDataset
    root, ref = capture
    batches = two_passes if source == "dir" else _passes(
        PolarDataset(root, S, batch_size=B, rank=0, world=1, epochs=2, augment=aug, seed=5, diffuse_source=source))
    assert len(batches) == 2 * (N // B)
    coef, mix = _psd()
    nsrc, kinds = 5 if source == "dir" else 4, set()
    for j, batch in enumerate(batches):
        p, i = divmod(j, N // B)
        for b in range(B):
            pos = i * B + b
            crop, fud, flr, remap = ar.draw(5, p, pos, *HW, flip_lr=0.5, flip_ud=0.5, crop_min=0.4)
            kinds.add((fud, flr))
            srcs = [ref[(v, pos)] for v in range(nsrc)]
            kw = dict(coef=coef, mix=mix if remap else None, crop=crop, flip_ud=not fud, flip_lr=flr)      # the loader's fixed flip_ud, XOR the draw
            want = ar.augment_views(srcs, S, S, MODES[source], dtype=np.float64, **kw)
            w32 = ar.augment_views(srcs, S, S, MODES[source], dtype=np.float32, **kw)
            for v in range(5):
                e32 = float(np.abs(w32[v] - want[v]).max())
                err = float(np.abs(batch[v][b].astype(np.float64) - want[v]).max())
                assert err <= pr.bound(e32), (source, p, pos, v, err, e32)
    assert len(kinds) == 4                                   # the 12 draws cover all four flip combinations


def test_draws_depend_on_seed_pass_and_position_only(capture, aug, two_passes):
    from shmgan_amd.data import PolarDataset
    root, _ = capture
    n = N // B
    again = _passes(PolarDataset(root, S, batch_size=B, rank=0, world=1, epochs=1, augment=aug, seed=5))
    assert all(np.array_equal(a, b) for x, y in zip(again, two_passes[:n]) for a, b in zip(x, y))
    assert all(not np.array_equal(two_passes[i][0], two_passes[n + i][0]) for i in range(n))          # pass 1 is not pass 0
    resumed = _passes(PolarDataset(root, S, batch_size=B, rank=0, world=1, epochs=1, augment=aug, seed=5, first_pass=1))
    assert all(np.array_equal(a, b) for x, y in zip(resumed, two_passes[n:]) for a, b in zip(x, y))
    other = PolarDataset(root, S, batch_size=B, rank=0, world=1, augment=aug, seed=6).batch(0)
    assert not np.array_equal(other[0].cpu().numpy(), two_passes[0][0])
    # B = 1 on "rank 1 of 2" sees the same sample with the same draw: the draw belongs to the position
    shard = PolarDataset(root, S, batch_size=1, rank=1, world=2, augment=aug, seed=5).batch(0)
    assert all(np.array_equal(shard[v][0].cpu().numpy(), two_passes[0][v][1]) for v in range(5))


def test_one_draw_per_sample(tmp_path):
    from shmgan_amd.data import PSD_SUBDIRS, Augment, PolarDataset
    _write(tmp_path, PSD_SUBDIRS, 4, 42, same_views=True)
    ds = PolarDataset(str(tmp_path), S, batch_size=B, rank=0, world=1, augment=Augment(0.5, 0.5, 0.4, views="keep"), seed=1)
    for batch in ds:
        for v in range(1, 5):
            assert torch.equal(batch[v], batch[0]), v
        assert not torch.equal(batch[0][0], batch[0][1])


def test_physical_views_of_the_45_degree_set_exchange_two_planes(tmp_path):
    from shmgan_amd.data import SHMGAN_SUBDIRS, Augment, PolarDataset
    _write(tmp_path, SHMGAN_SUBDIRS, 2, 43)
    for source in ("dir", "min"):
        for flips in (dict(flip_lr=1.0), dict(flip_ud=1.0)):
            got = {views: PolarDataset(str(tmp_path), S, batch_size=2, subdirs=SHMGAN_SUBDIRS, rank=0, world=1, diffuse_source=source,
                                       augment=Augment(crop_min=0.5, views=views, **flips), seed=2).batch(0) for views in ("physical", "keep")}
            for v, w in ((0, 0), (1, 3), (2, 2), (3, 1), (4, 4)):
                assert torch.equal(got["physical"][v], got["keep"][w]), (source, flips, v)
            assert not torch.equal(got["keep"][1], got["keep"][3])
        both = {views: PolarDataset(str(tmp_path), S, batch_size=2, subdirs=SHMGAN_SUBDIRS, rank=0, world=1, diffuse_source=source,
                                    augment=Augment(1.0, 1.0, views=views), seed=2).batch(0) for views in ("physical", "keep")}
        assert all(torch.equal(a, b) for a, b in zip(both["physical"], both["keep"]))          # a rotation by 180 degrees: no remap


def test_shuffle_yields_every_sample_once_per_pass(capture):
    from shmgan_amd.data import PolarDataset
    root, _ = capture
    plain = _passes(PolarDataset(root, S, batch_size=1, rank=0, world=1))
    ds = PolarDataset(root, S, batch_size=B, rank=0, world=1, epochs=2, shuffle=True, seed=3)
    got = _passes(ds)
    orders = []
    for p in range(2):
        pos = [ds.position(i, b, p) for i in range(N // B) for b in range(B)]
        assert sorted(pos) == list(range(N)) and pos == ar.order(N, 3, p, True).tolist()
        for k, q in enumerate(pos):
            batch = got[p * (N // B) + k // B]
            assert all(np.array_equal(batch[v][k % B], plain[q][v][0]) for v in range(5)), (p, k, q)
        orders.append(pos)
    assert orders[0] != orders[1]


def test_a_diffuse_image_of_another_size_raises_under_augmentation(tmp_path):
    from PIL import Image
    from shmgan_amd.data import PSD_SUBDIRS, Augment, PolarDataset
    _write(tmp_path, PSD_SUBDIRS, 2, 44)
    Image.fromarray(np.zeros((41, 56, 3), np.uint8)).save(tmp_path / "ED" / "img_00.png")           # the views are 40 x 56
    ds = PolarDataset(str(tmp_path), S, batch_size=1, rank=0, world=1, augment=Augment(flip_lr=0.5))
    with pytest.raises(ValueError, match=r"same decoded size.*ED.*img_00\.png 41x56"):
        ds.batch(0)
    assert tuple(ds.batch(1)[4].shape) == (1, S, S, 3)                                                 # the next sample is fine
    # the default path resizes every file on its own and never needed the sizes to agree
    assert tuple(PolarDataset(str(tmp_path), S, batch_size=1, rank=0, world=1).batch(0)[4].shape) == (1, S, S, 3)


# ------------------------------------------------------------------------------------------------ the trainer
def test_trainer_options_and_resume(tmp_path):
    from shmgan_amd import ShmGANwithSSpecSeg
    from shmgan_amd.data import PSD_SUBDIRS, Augment
    _write(tmp_path / "data", PSD_SUBDIRS, 4, 45)
    args = argparse.Namespace(mode="train", image_size=64, batch_size=1, filter_size=16, num_epochs=2, data_dir=str(tmp_path / "data"),
                              checkpoint_save_dir=str(tmp_path / "ckpt"), log_dir=str(tmp_path / "logs"), checkpoint_save_step=10,
                              shuffle=True, data_seed=4, aug_flip_ud=0.5, aug_crop_min=0.6)
    m = ShmGANwithSSpecSeg(args)
    assert m.train(args, max_steps=2, print_fn=lambda *a: None) == 2
    ds = m.loadedDataset
    assert ds.shuffle and ds.seed == 4 and ds.augment == Augment(flip_ud=0.5, crop_min=0.6) and ds.first_pass == 0 and len(ds) == 4
    assert np.isfinite(m.losses()["total_Generator_loss"])
    # the same trainer goes on from its checkpoint (2 steps in: still pass 0), then a new one resumes 4 steps in: pass 1
    assert m.train(args, max_steps=2, print_fn=lambda *a: None) == 2
    assert m.D.P.iterations == 4 and m.loadedDataset.first_pass == 0
    again = ShmGANwithSSpecSeg(args)
    lines = []
    assert again.train(args, max_steps=1, print_fn=lines.append) == 1
    assert any("Latest checkpoint restored" in l for l in lines)
    assert again.D.P.iterations == 5 and again.loadedDataset.first_pass == 1
