"""Polarimetry on the device: shm_polar_views_u8 (the four decoded views of a sample -> its five training planes) against the
oracle's loader arithmetic and the NumPy restatement (tests/polar_ref.py), shm_polar_maps against the restatement, the loader
with a computed diffuse target end to end, and write_estimated_diffuse.

Tolerances.  The view planes and the MIN estimate are the arithmetic shm_resize_bilinear_u8 is held to 2e-6 for
(tests/test_step_gpu.py), on bytes: 2e-6.  Everything that goes through the Stokes matrix is compared with the float64
restatement under polar_ref.bound: the larger of 2e-6 and four times the error the float32 restatement shows against float64 on the
same inputs (printed by each test; LABNOTES.md records the figures of the run this was written on)."""
import functools
import os

import numpy as np
import pytest
import torch

import polar_ref as pr
from oracle import data_np as dn
from util import host

pytestmark = pytest.mark.gpu

SIZES = [(37, 53, 32), (64, 64, 64), (20, 24, 48), (300, 200, 64)]
PSD_ANGLES = [0.0, 60.0, 90.0, 150.0]


@functools.lru_cache(maxsize=None)
def _views(hin, win):
    """Four random byte images of one sample (shared by the tests of a size; never modified)."""
    rng = np.random.default_rng(1000 * hin + win)
    out = [rng.integers(0, 256, (hin, win, 3)).astype(np.uint8) for _ in range(4)]
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _psd_matrix():
    from shmgan_amd.polar import stokes_matrix
    return stokes_matrix(PSD_ANGLES)


def _run_views(views, ho, wo, mode, coef=None, scale=1.0 / 255.0, flip=False):
    from shmgan_amd import ops
    srcs = [torch.from_numpy(a.copy()).cuda() for a in views]
    planes = torch.full((5, ho, wo, 3), float("nan"), device="cuda")
    ops.polar_views_u8(srcs, list(planes), mode, coef, scale, flip)
    return [host(p) for p in planes]


@pytest.mark.parametrize("hin,win,S", SIZES)
def test_views_and_minimum(hin, win, S):
    views = _views(hin, win)
    emin = np.minimum.reduce(views)
    for flip in (False, True):
        got = _run_views(views, S, S, "min", flip=flip)
        errs = [float(np.abs(got[v] - dn.load_view(views[v], S, flip)).max()) for v in range(4)]
        errs.append(float(np.abs(got[4] - dn.load_view(emin, S, flip)).max()))
        print(f"polar views/min {hin}x{win}->{S} flip={flip}: max errors {errs}")
        assert max(errs) < 2e-6, errs
    # at the source size with scale 1 every weight is 0: the bytes themselves, and the integer minimum, exactly
    got = _run_views(views, hin, win, "min", scale=1.0)
    for v in range(4):
        assert np.array_equal(got[v], views[v].astype(np.float64))
    assert np.array_equal(got[4], emin.astype(np.float64))


def _check_stokes(views, S, flip):
    coef = _psd_matrix()
    got = _run_views(views, S, S, "stokes", coef, flip=flip)
    ref = pr.polar_views(views, S, S, pr.STOKES, coef, flip_ud=flip, dtype=np.float64)
    r32 = pr.polar_views(views, S, S, pr.STOKES, coef, flip_ud=flip, dtype=np.float32)
    e32 = float(np.abs(r32[4] - ref[4]).max())
    err = float(np.abs(got[4] - ref[4]).max())
    print(f"polar stokes {views[0].shape[0]}x{views[0].shape[1]}->{S} flip={flip}: device error {err:.3e}, float32 restatement "
          f"{e32:.3e}, bound {pr.bound(e32):.3e}")
    assert err <= pr.bound(e32), (err, e32)
    for v in range(4):                               # the view planes do not depend on the mode
        assert np.abs(got[v] - dn.load_view(views[v], S, flip)).max() < 2e-6
    return got, ref


@pytest.mark.parametrize("hin,win,S", SIZES)
def test_stokes_estimate(hin, win, S):
    for flip in (False, True):
        _check_stokes(_views(hin, win), S, flip)


def test_stokes_estimate_clamps_at_zero():
    """Views no polarisation state explains (one bright view, three dark ones) fit S0 < sqrt(S1^2 + S2^2): the estimate is held
    at 0 there, per tap and before the interpolation."""
    hin, win, S = 37, 53, 32
    views = [a.copy() for a in _views(hin, win)]
    views[0][8:30, 10:40] = 255
    for v in (1, 2, 3):
        views[v][8:30, 10:40] = 0
    raw = pr.estimate_raw(views, pr.STOKES, _psd_matrix())
    assert raw[8:30, 10:40].max() < -50 and (raw > 0).any()
    got, ref = _check_stokes(views, S, False)
    inside = (ref[4] == 0).sum()
    assert inside > 100 and np.all(got[4][ref[4] == 0] == 0)
    # at the source size the clamped pixels are exact zeros, and nothing is negative anywhere
    full = _run_views(views, hin, win, "stokes", _psd_matrix(), scale=1.0)[4]
    assert np.all(full[8:30, 10:40] == 0) and full.min() >= 0 and full.max() <= 255


def _synthetic_views(n, seed):
    """S0 in [0.5, 1], DoP in [0.2, 0.8], uniform angle, rendered through the model at the PSD angles; float32 inputs."""
    rng = np.random.default_rng(seed)
    s0 = rng.uniform(0.5, 1.0, n)
    p = s0 * rng.uniform(0.2, 0.8, n)
    psi = rng.uniform(-np.pi / 2, np.pi / 2, n)
    return [(0.5 * (s0 + p * np.cos(2 * (np.deg2rad(t) - psi)))).astype(np.float32) for t in PSD_ANGLES], psi


def _check_maps(dev_views, np_views, coef):
    from shmgan_amd import ops
    out = ops.polar_maps(dev_views, coef)
    ref = pr.polar_maps(np_views, coef, np.float64)
    r32 = pr.polar_maps(np_views, coef, np.float32)
    for i, name in enumerate(("s0", "dop")):
        e32 = float(np.abs(r32[i] - ref[i]).max())
        err = float(np.abs(host(out[name]).reshape(-1) - ref[i]).max())
        print(f"polar maps {name} n={np_views[0].size}: device error {err:.3e}, float32 restatement {e32:.3e}, bound {pr.bound(e32):.3e}")
        assert err <= pr.bound(e32), (name, err, e32)
    e32 = float(pr.circ_dist(r32[2], ref[2]).max())
    err = float(pr.circ_dist(host(out["aolp"]).reshape(-1), ref[2]).max())
    print(f"polar maps aolp n={np_views[0].size}: device error {err:.3e}, float32 restatement {e32:.3e}, bound {pr.bound(e32):.3e}")
    assert err <= pr.bound(e32), ("aolp", err, e32)
    return out, ref


@pytest.mark.parametrize("n,shape", [(3 * 40 * 50, (40, 50, 3)), (4096, (4096,))])
def test_maps_against_the_restatement(n, shape):
    views, psi = _synthetic_views(n, n)
    out, ref = _check_maps([torch.from_numpy(a.reshape(shape)).cuda() for a in views], views, _psd_matrix())
    assert tuple(out["dop"].shape) == shape
    # and the maps are the ones the fields were rendered from (float32 inputs: 1e-5 is ample and not the check above)
    assert pr.circ_dist(ref[2], psi).max() < 1e-5 and ref[1].min() > 0.19 and ref[1].max() < 0.81


def test_maps_scalar_path_subset_of_outputs_and_zero_intensity():
    from shmgan_amd import ops
    n = 1003                                           # odd, and the views start 4 bytes into their buffers: the scalar kernel
    views, _ = _synthetic_views(n, 7)
    for a in views:
        a[17] = 0.0                                    # a black pixel: S0 == 0
    bufs = [torch.from_numpy(np.concatenate([[np.float32(9.0)], a])).cuda() for a in views]
    dev_views = [b[1:] for b in bufs]
    assert all(v.data_ptr() % 16 == 4 and v.is_contiguous() for v in dev_views)
    out, ref = _check_maps(dev_views, views, _psd_matrix())
    assert float(out["dop"][17]) == 0.0 and float(out["s0"][17]) == 0.0 and np.isfinite(host(out["dop"])).all()
    # the aligned kernel on the same values (n + 1 = 1004 elements, a multiple of 4) agrees with the scalar one bit for bit
    pad = [torch.cat([v, v[:1]]) for v in dev_views]
    vec = ops.polar_maps(pad, _psd_matrix())
    for k in ("s0", "dop", "aolp"):
        assert torch.equal(vec[k][:n], out[k])
    only = ops.polar_maps(dev_views, _psd_matrix(), want=("dop",))
    assert list(only) == ["dop"] and torch.equal(only["dop"], out["dop"])


def test_calcdop_is_the_reference_formula():
    from shmgan_amd import ShmGANwithSSpecSeg
    rng = np.random.default_rng(21)
    y = [rng.uniform(0.0, 1.0, (2, 16, 16, 1)).astype(np.float32) for _ in range(4)]
    y[0][0, 3, 3, 0] = y[2][0, 3, 3, 0] = 0.0          # S0 = I0 + I90 = 0: divide_no_nan gives 0
    m = ShmGANwithSSpecSeg(image_size=32, filter_size=16, batch_size=1)
    got = host(m.calcDOP(*[torch.from_numpy(a).cuda() for a in y]))
    assert got.shape == (2, 16, 16, 1) and got[0, 3, 3, 0] == 0.0

    def formula(dt):                                    # SHM.py:1158-1163
        i0, i45, i90, i135 = [a.astype(dt) for a in y]
        s0, s1, s2 = i0 + i90, i0 - i90, i45 - i135
        p = np.sqrt(s1 * s1 + s2 * s2)
        return np.divide(p, s0, out=np.zeros_like(p), where=s0 != 0)
    ref, r32 = formula(np.float64), formula(np.float32)
    e32 = float(np.abs(r32 - ref).max())
    err = float(np.abs(got - ref).max())
    print(f"calcDOP: device error {err:.3e}, float32 restatement {e32:.3e}, bound {pr.bound(e32):.3e}")
    assert err <= pr.bound(e32)
    maps = m.polar_maps([torch.from_numpy(a).cuda() for a in y], [0, 45, 90, 135], want=("s0",))
    assert np.abs(host(maps["s0"]) - 0.5 * sum(a.astype(np.float64) for a in y)).max() < 2e-6


# ------------------------------------------------------------------ loader end to end
def _write_capture(root, subdirs, n, seed, hw=(40, 50)):
    """n samples of differing heights in each directory; {(view, i): image}, i in sorted-name order."""
    from PIL import Image
    rng = np.random.default_rng(seed)
    ref = {}
    for v, sub in enumerate(subdirs):
        (root / sub).mkdir(parents=True)
        for i in range(n):
            img = rng.integers(0, 256, (hw[0] + 3 * i, hw[1], 3)).astype(np.uint8)
            Image.fromarray(img).save(root / sub / f"img_{i:02d}.png")
            ref[(v, i)] = img
    return ref


@pytest.fixture(scope="module")
def capture(tmp_path_factory):
    from shmgan_amd.data import PSD_SUBDIRS
    root = tmp_path_factory.mktemp("capture")
    return root, _write_capture(root, PSD_SUBDIRS[:4], 3, 31)


@pytest.mark.parametrize("B", [1, 2])
def test_loader_computes_the_diffuse_target(capture, B):
    from shmgan_amd.data import PolarDataset
    root, ref = capture
    S, n = 32, 3
    ds = PolarDataset(str(root), S, batch_size=B, diffuse_source="min", rank=0, world=1)
    assert len(ds) == n // B
    seen = 0
    for i, batch in enumerate(ds):
        assert len(batch) == 5 and all(tuple(t.shape) == (B, S, S, 3) for t in batch)
        for b in range(B):
            k = i * B + b
            for v in range(4):
                assert np.abs(host(batch[v][b]) - dn.load_view(ref[(v, k)], S, True)).max() < 2e-6, (k, v)
            emin = np.minimum.reduce([ref[(v, k)] for v in range(4)])
            assert np.abs(host(batch[4][b]) - dn.load_view(emin, S, True)).max() < 2e-6, k
            seen += 1
    assert seen == (n // B) * B


def test_loader_stokes_target_and_train_step(capture):
    from shmgan_amd import ShmGANwithSSpecSeg
    from shmgan_amd.data import PolarDataset
    root, ref = capture
    S = 32
    ds = PolarDataset(str(root), S, batch_size=1, diffuse_source="stokes", rank=0, world=1)
    batch = ds.batch(1)
    views = [ref[(v, 1)] for v in range(4)]
    want = pr.polar_views(views, S, S, pr.STOKES, _psd_matrix(), flip_ud=True, dtype=np.float64)
    e32 = float(np.abs(pr.polar_views(views, S, S, pr.STOKES, _psd_matrix(), flip_ud=True, dtype=np.float32)[4] - want[4]).max())
    assert np.abs(host(batch[4][0]) - want[4]).max() <= pr.bound(e32)
    # the trainer takes what the loader yields
    m = ShmGANwithSSpecSeg(image_size=S, filter_size=16, batch_size=1).build()
    m.train_step(*PolarDataset(str(root), S, batch_size=1, diffuse_source="min", rank=0, world=1).batch(0))
    torch.cuda.synchronize()
    losses = m.losses()
    assert all(np.isfinite(v) for k, v in losses.items() if k != "ssim"), losses


def test_default_source_still_reads_the_directory(tmp_path):
    """With an ED/ directory and default options nothing changes: the fifth tensor is the resized ED file, not an estimate."""
    from shmgan_amd.data import PSD_SUBDIRS, PolarDataset
    S, n = 32, 3
    ref = _write_capture(tmp_path, PSD_SUBDIRS, n, 32)
    ds = PolarDataset(str(tmp_path), S, batch_size=1, rank=0, world=1)
    assert ds.diffuse_source == "dir" and len(ds.files) == 5
    for i, batch in enumerate(ds):
        for v in range(5):
            assert np.abs(host(batch[v][0]) - dn.load_view(ref[(v, i)], S, True)).max() < 2e-6, (i, v)


def test_mismatched_view_sizes_raise(tmp_path):
    from PIL import Image
    from shmgan_amd.data import PSD_SUBDIRS, PolarDataset
    _write_capture(tmp_path, PSD_SUBDIRS[:4], 2, 33)
    Image.fromarray(np.zeros((41, 50, 3), np.uint8)).save(tmp_path / "I90" / "img_00.png")       # the others are 40 x 50
    ds = PolarDataset(str(tmp_path), 32, batch_size=1, diffuse_source="min", rank=0, world=1)
    with pytest.raises(ValueError, match="I90.*img_00.png 41x50"):
        ds.batch(0)
    assert tuple(ds.batch(1)[4].shape) == (1, 32, 32, 3)                                           # the next sample is fine


def test_write_estimated_diffuse_round_trip(capture, tmp_path):
    from PIL import Image
    from shmgan_amd.data import PSD_SUBDIRS, PolarDataset
    from shmgan_amd.polar import write_estimated_diffuse
    root, ref = capture
    S, n = 32, 3
    ed = tmp_path / "ED"
    written = write_estimated_diffuse(str(root), str(ed), PSD_SUBDIRS)
    assert [os.path.basename(p) for p in written] == [f"img_{i:02d}.png" for i in range(n)]
    for i, p in enumerate(written):
        with Image.open(p) as im:
            assert np.array_equal(np.asarray(im), np.minimum.reduce([ref[(v, i)] for v in range(4)])), p
    # fed back as the ED/ directory, the reference's path gives the batches the computed target gave
    for sub in PSD_SUBDIRS[:4]:
        (tmp_path / sub).symlink_to(root / sub, target_is_directory=True)
    from_dir = PolarDataset(str(tmp_path), S, batch_size=1, diffuse_source="dir", rank=0, world=1)
    computed = PolarDataset(str(root), S, batch_size=1, diffuse_source="min", rank=0, world=1)
    for a, b in zip(from_dir, computed):
        for v in range(5):
            assert np.abs(host(a[v]) - host(b[v])).max() < 2e-6, v
