"""Train-time augmentation, the part that needs no GPU: polar.mirror_views, the stateless draws and the shuffle of the loader,
the argument checks of shm_augment_views_u8 (all before any launch), Augment's validation, the trainer options, and the teeth of
the float64 restatement the device is compared with in test_augment_gpu.py (tests/augment_ref.py)."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest

import augment_ref as ar
import polar_ref as pr

PSD_ANGLES = (0.0, 60.0, 90.0, 150.0)


# ------------------------------------------------------------------------------------------------ mirror_views
def test_mirror_of_the_45_degree_set_is_a_permutation():
    from shmgan_amd.polar import mirror_views
    assert mirror_views((0, 45, 90, 135)) == ("permute", [0, 3, 2, 1])
    assert mirror_views((135, 90, 45, 0)) == ("permute", [2, 1, 0, 3])
    assert mirror_views((0, 45, 90, 135 + 180)) == ("permute", [0, 3, 2, 1])          # theta and theta + 180 are one polariser


@pytest.mark.parametrize("angles", [PSD_ANGLES, (10.0, 50.0, 95.0, 140.0), (0.0, 45.0, 90.0, 120.0)])
def test_mirror_mix_reproduces_the_mirrored_polarisers(angles):
    """Views rendered from random Stokes vectors, mixed in float64, are the views at 180 - theta_i: 1e-12 on values of order 1."""
    from shmgan_amd.polar import _model_rows, _stokes_f64, mirror_views
    kind, m32 = mirror_views(angles)
    assert kind == "mix" and m32.dtype == np.float32 and m32.shape == (4, 4)
    m64 = _model_rows(ar.mirror_angles(angles)) @ _stokes_f64(angles)
    assert np.abs(m64 - m32).max() < 1e-7
    rng = np.random.default_rng(5)
    s0, s1, s2 = rng.uniform(0.5, 1.0, 1000), rng.uniform(-0.4, 0.4, 1000), rng.uniform(-0.4, 0.4, 1000)
    views = np.stack([ar.intensity(s0, s1, s2, t) for t in angles])
    want = np.stack([ar.intensity(s0, s1, s2, t) for t in ar.mirror_angles(angles)])
    err = float(np.abs(m64 @ views - want).max())
    print(f"mirror mix {angles}: float64 error {err:.3e}")
    assert err < 1e-12
    if angles == PSD_ANGLES:                            # multiples of 0.25: exact in float32, and exact on bytes
        assert np.array_equal(m32 * 4, np.round(m32 * 4)), m32
        assert np.array_equal(m32 * 4, [[3, 1, -1, 1], [-1, -1, 3, 3], [-1, 1, 3, 1], [3, 3, -1, -1]])


def test_mirror_needs_three_distinct_angles():
    from shmgan_amd.polar import mirror_views
    for bad in ((0, 90), (0, 90, 180, 270), (30, 30, 30, 30)):
        with pytest.raises(ValueError, match="three polariser angles"):
            mirror_views(bad)


# ------------------------------------------------------------------------------------------------ augment_params
def test_draws_stay_inside_keep_the_aspect_and_are_stateless():
    from shmgan_amd.data import Augment, augment_params
    aug = Augment(flip_lr=0.5, flip_ud=0.5, crop_min=0.3)
    n, hin, win = 10000, 37, 53
    draws = [augment_params(7, k % 3, k, hin, win, aug) for k in range(n)]
    eps = 1e-6                                           # the crop values are float32 values: 2^-24 relative per side
    for k, p in enumerate(draws):
        cy, cx, ch, cw = p.crop
        assert all(isinstance(v, float) and np.float32(v) == v for v in p.crop)
        assert cy >= 0 and cx >= 0 and ch > 0 and cw > 0 and cy + ch <= hin and cx + cw <= win, (k, p)
        area = (ch * cw) / (hin * win)
        assert 0.3 * (1 - eps) <= area <= 1.0, (k, area)
        assert abs(ch / hin - cw / win) <= eps, (k, p)
        assert p.remap == (p.flip_ud != p.flip_lr)
        assert p == augment_params(7, k % 3, k, hin, win, aug)
        want = ar.draw(7, k % 3, k, hin, win, 0.5, 0.5, 0.3)
        assert (p.crop, p.flip_ud, p.flip_lr, p.remap) == want, (k, p, want)
    for name in ("flip_ud", "flip_lr"):
        freq = np.mean([getattr(p, name) for p in draws])
        assert abs(freq - 0.5) <= 0.02, (name, freq)
    assert abs(np.mean([p.remap for p in draws]) - 0.5) <= 0.02
    areas = np.array([p.crop[2] * p.crop[3] for p in draws]) / (hin * win)
    assert abs(areas.mean() - 0.65) < 0.01 and areas.min() < 0.31 and areas.max() > 0.99         # U(0.3, 1)
    # the key is (seed, pass, position): changing any of them changes the draw
    base = augment_params(7, 0, 11, hin, win, aug)
    assert all(augment_params(*key, hin, win, aug).crop != base.crop for key in ((8, 0, 11), (7, 1, 11), (7, 0, 12)))


def test_default_augment_is_the_identity():
    from shmgan_amd.data import Augment, augment_params
    for k in range(200):
        p = augment_params(k, k + 1, 2 * k, 37, 53, Augment())
        assert p.crop == (0.0, 0.0, 37.0, 53.0) and not p.flip_ud and not p.flip_lr and not p.remap
    # a probability of one always flips; both together leave the views alone
    p = augment_params(0, 0, 0, 8, 8, Augment(flip_lr=1.0, flip_ud=1.0))
    assert p.flip_ud and p.flip_lr and not p.remap
    assert augment_params(0, 0, 0, 8, 8, Augment(flip_lr=1.0)).remap


def test_augment_validation():
    from shmgan_amd.data import Augment, PolarDataset
    for kw, name in ((dict(flip_lr=1.5), "flip_lr"), (dict(flip_ud=-0.1), "flip_ud"), (dict(flip_ud="yes"), "flip_ud"),
                     (dict(crop_min=0.0), "crop_min"), (dict(crop_min=1.2), "crop_min"), (dict(views="rotate"), "views")):
        with pytest.raises(ValueError, match=name):
            Augment(**kw)
    with pytest.raises(Exception):                       # frozen
        Augment().flip_lr = 0.5
    with pytest.raises(ValueError, match="Augment"):
        PolarDataset("/nonexistent", 32, augment=dict(flip_lr=0.5), rank=0, world=1)


# ------------------------------------------------------------------------------------------------ shuffle and sharding
def _listing(root, subdirs, n):
    for s in subdirs:
        (root / s).mkdir()
        for i in range(n):
            (root / s / f"img_{i:03d}.png").write_bytes(b"")          # listed, never decoded here
    return str(root)


def test_shuffle_is_a_permutation_per_pass_shared_by_the_ranks(tmp_path):
    from shmgan_amd.data import PSD_SUBDIRS, PolarDataset, pass_order
    n, B = 11, 2
    for p in range(4):
        o = pass_order(n, 3, p, True)
        assert sorted(o.tolist()) == list(range(n)) and np.array_equal(o, ar.order(n, 3, p, True))
        assert np.array_equal(pass_order(n, 3, p, False), np.arange(n))
    assert len({tuple(pass_order(n, 3, p, True).tolist()) for p in range(4)}) == 4
    assert not np.array_equal(pass_order(n, 3, 0, True), pass_order(n, 4, 0, True))
    root = _listing(tmp_path, PSD_SUBDIRS, n)
    ranks = [PolarDataset(root, 32, batch_size=B, rank=r, world=2, shuffle=True, seed=3) for r in range(2)]
    assert [len(d) for d in ranks] == [2, 2]
    for p in (0, 1):
        seen = [[d.position(i, b, p) for i in range(len(d)) for b in range(B)] for d in ranks]
        assert not set(seen[0]) & set(seen[1])
        both = seen[0] + seen[1]
        assert len(set(both)) == 2 * B * len(ranks[0]) == 8 and set(both) <= set(range(n))
        assert [d.position(0, 0, p) for d in ranks] == [int(ar.order(n, 3, p, True)[0]), int(ar.order(n, 3, p, True)[B])]
    # without the option: today's order, whatever the pass
    plain = PolarDataset(root, 32, batch_size=B, rank=1, world=2)
    assert [plain.position(i, b, 5) for i in range(2) for b in range(B)] == [2, 3, 6, 7]
    assert plain.augment is None and not plain.shuffle and plain.first_pass == 0


def test_trainer_options_reach_the_loader(tmp_path):
    from shmgan_amd.data import PSD_SUBDIRS, Augment, datasetLoad
    root = _listing(tmp_path, PSD_SUBDIRS, 4)

    def load(**args):
        t = SimpleNamespace(data_dir=root, image_size=32, batch_size=1, device="cpu", num_epochs=1, args=SimpleNamespace(**args))
        return datasetLoad(t)[1]
    ds = load()
    assert ds.augment is None and not ds.shuffle and ds.seed == 0          # the default path
    ds = load(shuffle=True, data_seed=9, aug_flip_ud=0.5, aug_crop_min=0.6)
    assert ds.shuffle and ds.seed == 9 and ds.augment == Augment(flip_ud=0.5, crop_min=0.6) and ds._mirror[0] == "mix"
    assert load(aug_flip_lr=0.25, aug_views="keep").augment == Augment(flip_lr=0.25, views="keep")
    with pytest.raises(ValueError, match="views"):
        load(aug_flip_lr=0.25, aug_views="bogus")
    from shmgan_amd.trainer import _DEFAULTS
    assert {k: _DEFAULTS[k] for k in ("shuffle", "data_seed", "aug_flip_lr", "aug_flip_ud", "aug_crop_min", "aug_views")} == dict(
        shuffle=False, data_seed=0, aug_flip_lr=0.0, aug_flip_ud=0.0, aug_crop_min=1.0, aug_views="physical")


# ------------------------------------------------------------------------------------------------ the C ABI's argument checks
def test_shape_errors_before_any_launch():
    from shmgan_amd import _lib
    L = _lib.lib()
    p5, p4 = (C.c_void_p * 5)(1, 1, 1, 1, 1), (C.c_void_p * 4)(1, 1, 1, 1)          # non-null pointers nobody dereferences
    hole = (C.c_void_p * 5)(1, 1, None, 1, 1)
    MIN, STOKES, DIR = 0, 1, 2

    def call(src=p5, n_src=5, hin=8, win=8, mode=DIR, coef=None, mix=None, crop=(0.0, 0.0, 8.0, 8.0), dst=p5, ho=4, wo=4):
        return L.shm_augment_views_u8(src, n_src, hin, win, mode, coef, mix, *crop, 0, 0, dst, ho, wo, 1.0, None)

    nan = float("nan")
    cases = [(dict(src=None), b"null pointer"), (dict(dst=None), b"null pointer"), (dict(src=hole), b"null pointer (source 2)"),
             (dict(dst=hole), b"null pointer (destination plane 2)"),
             (dict(n_src=4), b"n_src 4"), (dict(src=p4, n_src=5, mode=MIN), b"n_src 5"), (dict(src=p4, n_src=4, mode=7), b"mode 7"),
             (dict(hin=0), b"outside [1, 32768]"), (dict(win=32769, crop=(0.0, 0.0, 8.0, 8.0)), b"outside [1, 32768]"),
             (dict(ho=0), b"outside [1, 32768]"), (dict(wo=40000), b"outside [1, 32768]"),
             (dict(crop=(0.0, 0.0, 0.0, 8.0)), b"empty crop"), (dict(crop=(0.0, 0.0, 8.0, -1.0)), b"empty crop"),
             (dict(crop=(0.0, 0.0, nan, 8.0)), b"empty crop"),
             (dict(crop=(-0.5, 0.0, 8.0, 8.0)), b"does not lie inside"), (dict(crop=(0.5, 0.0, 8.0, 8.0)), b"does not lie inside"),
             (dict(crop=(0.0, 1.0, 4.0, 7.5)), b"does not lie inside"), (dict(crop=(0.0, nan, 4.0, 4.0)), b"does not lie inside"),
             (dict(src=p4, n_src=4, mode=STOKES), b"needs coef")]
    for kw, msg in cases:
        assert call(**kw) == -1 and msg in L.shm_last_error(), (kw, L.shm_last_error())
    assert b"shm_augment_views_u8" in L.shm_last_error()


# ------------------------------------------------------------------------------------------------ the restatement has teeth
def test_restatement_agrees_with_polar_ref_at_identity_parameters():
    """Identity parameters restate polar_ref.polar_views (sizes whose scale is a dyadic ratio: the coordinate product is exact, so
    the fused coordinate of augment_ref.coords and the unfused one of polar_ref.taps are the same float32 numbers)."""
    rng = np.random.default_rng(2)
    coef = np.asarray([[0.5, 0.5, 0.5, 0.5], [1, 0, -1, 0], [0.57735026, 1.1547005, -0.57735026, -1.1547005]], np.float32)
    for (hin, win, ho, wo) in ((37, 53, 16, 16), (9, 7, 32, 32), (5, 5, 1, 1), (16, 16, 16, 16)):
        views = [rng.integers(0, 256, (hin, win, 3)).astype(np.uint8) for _ in range(5)]
        for flip in (False, True):
            for dt in (np.float32, np.float64):
                want = pr.polar_views(views[:4], ho, wo, pr.STOKES, coef, flip_ud=flip, dtype=dt)
                got = ar.augment_views(views[:4], ho, wo, ar.STOKES, coef, flip_ud=flip, dtype=dt)
                assert all(np.array_equal(a, b) for a, b in zip(got, want)), (hin, win, flip, dt)
                got = ar.augment_views(views, ho, wo, ar.DIR, flip_ud=flip, dtype=dt)
                want = [pr.resize(v, ho, wo, dt) * dt(np.float32(1.0 / 255.0)) for v in views]
                want = [w[::-1] if flip else w for w in want]
                assert all(np.array_equal(a, b) for a, b in zip(got, want))


def test_restatement_sees_a_dropped_remap_and_a_mixed_fifth_plane():
    """The two mistakes the issue names move the float64 result by far more than the bound of the device comparison on the inputs
    test_augment_gpu.py uses: so that comparison can see them."""
    from shmgan_amd.polar import mirror_views, stokes_matrix
    _, mix = mirror_views(PSD_ANGLES)
    coef = stokes_matrix(PSD_ANGLES)
    rng = np.random.default_rng(1000 * 40 + 56)
    views = [rng.integers(0, 256, (40, 56, 3)).astype(np.uint8) for _ in range(4)]
    raw = np.asarray(mix, np.float64) @ np.stack([v.reshape(-1) for v in views]).astype(np.float64)
    assert raw.min() < -20 and raw.max() > 275                       # the clamp is exercised on both sides
    kw = dict(crop=(3.5, 2.25, 24.0, 40.0), flip_lr=True)
    ref = ar.augment_views(views, 32, 32, ar.STOKES, coef, mix, dtype=np.float64, **kw)
    r32 = ar.augment_views(views, 32, 32, ar.STOKES, coef, mix, dtype=np.float32, **kw)
    bound = pr.bound(max(float(np.abs(a - b).max()) for a, b in zip(r32, ref)))
    assert bound < 1e-5
    no_remap = ar.augment_views(views, 32, 32, ar.STOKES, coef, None, dtype=np.float64, **kw)
    assert min(float(np.abs(no_remap[v] - ref[v]).max()) for v in range(4)) > 1000 * bound
    assert np.array_equal(no_remap[4], ref[4])                         # the fifth plane does not depend on the mix
    for mode in (ar.MIN, ar.STOKES):
        good = ar.augment_views(views, 32, 32, mode, coef, mix, dtype=np.float64, **kw)
        mixed5 = ar.augment_views(views, 32, 32, mode, coef, mix, dtype=np.float64, mix_fifth=True, **kw)
        assert float(np.abs(mixed5[4] - good[4]).max()) > 1000 * bound, mode
    # ... and a forgotten mirror or crop origin
    assert float(np.abs(ar.augment_views(views, 32, 32, ar.STOKES, coef, mix, crop=kw["crop"])[0] - ref[0]).max()) > 1000 * bound
    assert float(np.abs(ar.augment_views(views, 32, 32, ar.STOKES, coef, mix, crop=(3.5, 2.0, 24.0, 40.0), flip_lr=True)[0] - ref[0]).max()) > 1000 * bound
