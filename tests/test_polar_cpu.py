"""Host side of the polarimetry feature (csrc/polar.hip, shmgan_amd/polar.py, PolarDataset(diffuse_source=)): the C ABI is in
sync and refuses bad calls before any launch, the Stokes matrices are the hand-derivable ones, the NumPy restatement the device
tests compare against gives hand-computed answers, and the loader lists a four-directory capture.  No GPU is touched."""
import ctypes as C

import numpy as np
import pytest

import polar_ref as pr
from shmgan_amd import _lib


def test_entry_points_are_declared_bound_and_exported():
    L = _lib.lib()
    hdr = _lib.header_functions()
    for name in ("shm_polar_views_u8", "shm_polar_maps"):
        assert name in hdr and name in _lib.SIGNATURES and hasattr(L, name), name
    assert "polar.hip" in _lib.SOURCES
    txt = _lib.HEADER.read_text()
    assert "#define SHM_POLAR_MIN 0" in txt and "#define SHM_POLAR_STOKES 1" in txt


def _fake(n):
    """A host array of n non-null 'device pointers' nobody dereferences (the refusals come before any launch)."""
    return (C.c_void_p * n)(*([16] * n))


def test_views_refusals_without_gpu():
    L = _lib.lib()
    src, dst, coef = _fake(4), _fake(5), (C.c_float * 12)()
    assert L.shm_polar_views_u8(None, 8, 8, None, 0, dst, 4, 4, 1.0, 0, None) == -1 and b"null pointer" in L.shm_last_error()
    assert L.shm_polar_views_u8(src, 8, 8, None, 0, None, 4, 4, 1.0, 0, None) == -1 and b"null pointer" in L.shm_last_error()
    hole = (C.c_void_p * 4)(16, 16, None, 16)
    assert L.shm_polar_views_u8(hole, 8, 8, None, 0, dst, 4, 4, 1.0, 0, None) == -1 and b"view 2" in L.shm_last_error()
    hole = (C.c_void_p * 5)(16, 16, 16, 16, None)
    assert L.shm_polar_views_u8(src, 8, 8, None, 0, hole, 4, 4, 1.0, 0, None) == -1 and b"plane 4" in L.shm_last_error()
    for hin, win, ho, wo in ((0, 8, 4, 4), (8, -1, 4, 4), (8, 8, 0, 4), (8, 8, 4, -3)):
        assert L.shm_polar_views_u8(src, hin, win, None, 0, dst, ho, wo, 1.0, 0, None) == -1 and b"sizes" in L.shm_last_error()
    assert L.shm_polar_views_u8(src, 8, 8, coef, 7, dst, 4, 4, 1.0, 0, None) == -1 and b"mode" in L.shm_last_error()
    assert L.shm_polar_views_u8(src, 8, 8, None, 1, dst, 4, 4, 1.0, 0, None) == -1 and b"coef" in L.shm_last_error()


def test_maps_refusals_without_gpu():
    L = _lib.lib()
    views, coef = _fake(4), (C.c_float * 12)()
    assert L.shm_polar_maps(None, 16, coef, 16, 16, 16, None) == -1 and b"null pointer" in L.shm_last_error()
    assert L.shm_polar_maps(views, 16, None, 16, 16, 16, None) == -1 and b"null pointer" in L.shm_last_error()
    hole = (C.c_void_p * 4)(16, None, 16, 16)
    assert L.shm_polar_maps(hole, 16, coef, 16, 16, 16, None) == -1 and b"view 1" in L.shm_last_error()
    assert L.shm_polar_maps(views, 0, coef, 16, 16, 16, None) == -1 and b"n is 0" in L.shm_last_error()
    assert L.shm_polar_maps(views, 16, coef, None, None, None, None) == 0          # nothing asked for: no launch


def test_wrappers_validate_before_the_library_is_called():
    import torch
    from shmgan_amd import ops
    u8 = [torch.zeros((4, 4, 3), dtype=torch.uint8) for _ in range(4)]
    f32 = [torch.zeros((2, 2, 3)) for _ in range(5)]
    with pytest.raises(ValueError):
        ops.polar_views_u8(u8[:3], f32)
    with pytest.raises(ValueError):
        ops.polar_views_u8(u8, f32, mode="max")
    with pytest.raises(ValueError):
        ops.polar_views_u8(u8, f32, mode="stokes")
    with pytest.raises(TypeError):
        ops.polar_views_u8(u8, f32)                       # host tensors
    with pytest.raises(TypeError):
        ops.polar_maps([torch.zeros(8)] * 4, [[0.0] * 4] * 3)
    with pytest.raises(ValueError):
        ops.polar_maps([torch.zeros(8)] * 4, [[0.0] * 4] * 3, want=("dolp",))
    with pytest.raises(ValueError):
        ops._polar_coef([[1.0, 0.0, 0.0]] * 3, "test")


def test_stokes_matrix_of_the_textbook_angles():
    """0/45/90/135: A = 0.5 [1, cos 2t, sin 2t] has A^T A = diag(1, .5, .5), so C = diag(1, 2, 2) A^T."""
    from shmgan_amd.polar import stokes_matrix
    c = stokes_matrix([0, 45, 90, 135])
    assert c.dtype == np.float32 and c.shape == (3, 4)
    assert np.abs(c - np.array([[.5, .5, .5, .5], [1, 0, -1, 0], [0, 1, 0, -1]])).max() <= 1e-6


def test_stokes_matrix_recovers_a_synthetic_state_at_the_psd_angles():
    from shmgan_amd.polar import stokes_matrix
    s = np.array([0.9, 0.31, -0.22])
    th = np.deg2rad([0.0, 60.0, 90.0, 150.0])
    inten = 0.5 * (s[0] + s[1] * np.cos(2 * th) + s[2] * np.sin(2 * th))
    assert np.abs(stokes_matrix([0, 60, 90, 150]).astype(np.float64) @ inten - s).max() <= 1e-5
    # angles are polariser orientations: theta + 180 is the same polariser, and the order of the views is the caller's
    assert np.abs(stokes_matrix([180, 240, 90, 330]) - stokes_matrix([0, 60, 90, 150])).max() <= 1e-6


def test_stokes_matrix_refuses_an_underdetermined_fit():
    from shmgan_amd.polar import stokes_matrix
    with pytest.raises(ValueError):
        stokes_matrix([0, 90, 180, 270])                  # two distinct polarisers
    with pytest.raises(ValueError):
        stokes_matrix([10, 10, 190, 100])


def test_angles_from_subdirs():
    from shmgan_amd.data import PSD_SUBDIRS, SHMGAN_SUBDIRS
    from shmgan_amd.polar import REFERENCE_DOP_MATRIX, angles_from_subdirs
    assert angles_from_subdirs() == [0, 60, 90, 150]
    assert angles_from_subdirs(PSD_SUBDIRS[:4]) == [0, 60, 90, 150]
    assert angles_from_subdirs(SHMGAN_SUBDIRS[:4]) == [0, 45, 90, 135]
    with pytest.raises(ValueError):
        angles_from_subdirs(("ED",))
    with pytest.raises(ValueError):
        angles_from_subdirs(PSD_SUBDIRS)
    assert REFERENCE_DOP_MATRIX == [[1, 0, 1, 0], [1, 0, -1, 0], [0, 1, 0, -1]]


def test_restatement_minimum_by_hand():
    v = [np.array([[[9, 9, 9], [1, 200, 3]], [[50, 60, 70], [255, 0, 128]]], np.uint8),
         np.array([[[8, 10, 9], [2, 100, 3]], [[50, 61, 69], [254, 1, 127]]], np.uint8),
         np.array([[[7, 11, 9], [3, 150, 2]], [[49, 62, 71], [253, 2, 129]]], np.uint8),
         np.array([[[6, 12, 8], [4, 250, 4]], [[51, 63, 72], [252, 3, 126]]], np.uint8)]
    want = np.array([[[6, 9, 8], [1, 100, 2]], [[49, 60, 69], [252, 0, 126]]], np.float64)
    assert np.array_equal(pr.estimate(v, pr.MIN), want)
    # at the source size every interpolation weight is 0: the planes are the bytes (times scale), the fifth the minimum
    planes = pr.polar_views(v, 2, 2, pr.MIN, scale=1.0)
    assert all(np.array_equal(planes[i], v[i].astype(np.float64)) for i in range(4)) and np.array_equal(planes[4], want)
    assert np.array_equal(pr.polar_views(v, 2, 2, pr.MIN, scale=1.0, flip_ud=True)[4], want[::-1])


def test_restatement_stokes_by_hand():
    """Unpolarised light, v0 = v1 = v2 = v3 = k at 0/45/90/135: S0 = 0.5 * 4k = 2k, S1 = S2 = 0, e = 0.5 * (2k - 0) = k.
    Fully polarised along 0 degrees with S0 = 200: v = (200, 100, 0, 100), S1 = 200, S2 = 0, e = 0 (the minimum of the four samples is
    0 as well: a polariser sits at the minimum).  v = (255, 0, 0, 0) fits no polarisation state: S0 = 127.5, S1 = 255, e = -63.75
    before the clamp and 0 after it."""
    from shmgan_amd.polar import stokes_matrix
    c = stokes_matrix([0, 45, 90, 135])
    for dt in (np.float64, np.float32):
        k = 37.0
        assert pr.estimate([np.full((1, 1, 3), k)] * 4, pr.STOKES, c, dt)[0, 0, 0] == k
        v = [np.full((1, 1, 3), x) for x in (200.0, 100.0, 0.0, 100.0)]
        assert pr.estimate(v, pr.STOKES, c, dt)[0, 0, 0] == 0.0
        v = [np.full((1, 1, 3), x) for x in (255.0, 0.0, 0.0, 0.0)]
        assert pr.estimate_raw(v, pr.STOKES, c, dt)[0, 0, 0] == -63.75 and pr.estimate(v, pr.STOKES, c, dt)[0, 0, 0] == 0.0
    # partial polarisation at 30 degrees, PSD angles: the fitted minimum lies below the smallest of the four samples
    s0, p, psi = 180.0, 90.0, np.deg2rad(30.0)
    th = np.deg2rad([0.0, 60.0, 90.0, 150.0])
    v = [np.full((1, 1, 3), 0.5 * (s0 + p * np.cos(2 * (t - psi)))) for t in th]
    e = pr.estimate(v, pr.STOKES, stokes_matrix([0, 60, 90, 150]))[0, 0, 0]
    assert abs(e - 0.5 * (s0 - p)) < 1e-4 and e < min(float(a[0, 0, 0]) for a in v) - 5.0


def test_restatement_maps_by_hand_and_resize_agrees_with_the_oracle():
    from oracle import data_np as dn
    from shmgan_amd.polar import REFERENCE_DOP_MATRIX
    v = [np.array([3.0, 0.0, 2.0]), np.array([2.0, 0.0, 3.0]), np.array([1.0, 0.0, 2.0]), np.array([2.0, 0.0, 1.0])]
    s0, dop, aolp = pr.polar_maps(v, REFERENCE_DOP_MATRIX)
    # S0 = I0 + I90 = (4, 0, 4); S1 = I0 - I90 = (2, 0, 0); S2 = I45 - I135 = (0, 0, 2)
    assert np.array_equal(s0, [4, 0, 4]) and np.array_equal(dop, [0.5, 0.0, 0.5])
    assert np.allclose(aolp, [0.0, 0.0, np.pi / 4], atol=1e-15)
    assert pr.circ_dist(np.pi / 2 - 1e-3, -np.pi / 2 + 1e-3) < 2.1e-3
    img = np.random.default_rng(0).integers(0, 256, (37, 53, 3)).astype(np.uint8)
    assert np.array_equal(pr.resize(img, 32, 32, np.float32), dn.resize_bilinear(img, 32, 32))
    assert np.array_equal(pr.polar_views([img] * 4, 32, 32, pr.MIN, flip_ud=True, dtype=np.float32)[4], dn.load_view(img, 32, True))


def _write_views(root, subdirs, n=3):
    from PIL import Image
    rng = np.random.default_rng(3)
    for sub in subdirs:
        (root / sub).mkdir()
        for i in range(n):
            Image.fromarray(rng.integers(0, 256, (10 + i, 12, 3)).astype(np.uint8)).save(root / sub / f"img_{i:02d}.png")


def test_loader_lists_a_four_directory_capture_without_gpu(tmp_path):
    from shmgan_amd.data import PSD_SUBDIRS, PolarDataset
    _write_views(tmp_path, PSD_SUBDIRS[:4])
    ds = PolarDataset(str(tmp_path), 32, diffuse_source="min")
    assert len(ds) == 3 and len(ds.files) == 4 and ds.coef is None
    ds = PolarDataset(str(tmp_path), 32, batch_size=2, diffuse_source="stokes", rank=0, world=1)
    assert len(ds) == 1 and np.abs(ds.coef[0] - 0.5).max() < 1e-6
    assert PolarDataset(str(tmp_path), 32, diffuse_source="stokes", angles=[0, 45, 90, 135]).coef[1].tolist() == [1, 0, -1, 0]
    with pytest.raises(OSError):
        PolarDataset(str(tmp_path), 32)                   # "dir" (the default) still wants its fifth directory
    with pytest.raises(OSError):
        PolarDataset(str(tmp_path), 32, diffuse_source="dir")
    with pytest.raises(ValueError):
        PolarDataset(str(tmp_path), 32, diffuse_source="median")
    with pytest.raises(ValueError):
        PolarDataset(str(tmp_path), 32, subdirs=("I0", "I60", "I90"), diffuse_source="min")


def test_trainer_option_defaults_to_the_directory():
    import inspect
    from shmgan_amd import ShmGANwithSSpecSeg, trainer
    assert trainer._DEFAULTS["diffuse_source"] == "dir"
    assert list(inspect.signature(ShmGANwithSSpecSeg.calcDOP).parameters) == ["self", "I0_Ych", "I45_Ych", "I90_Ych", "I135_Ych"]
    assert callable(ShmGANwithSSpecSeg.polar_maps)
