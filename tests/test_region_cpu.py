"""The region metrics' reference against itself (tests/region_ref.py), without a GPU: a full region reproduces metrics_ref, the two
decomposition identities hold in float64, every case of the table lands in the branch it is named for, and four modelled faults of the
kernels -- each of which the comparison of tests/test_region_gpu.py must catch -- exceed its tolerance on the table's own data."""
import numpy as np
import pytest

from oracle import tf_ops_np as tfn

import metrics_ref as mr
import region_ref as rr

SMALL = [s for s in rr.SIZES if s[0] * s[1] <= 64 * 64]


def test_the_window_is_the_outer_product_of_its_marginal():
    w1 = rr.gauss_1d()
    assert np.allclose(np.outer(w1, w1), tfn.gauss_window(11, 1.5, np.float64), rtol=1e-13, atol=0.0)
    g, t, smap = rr.pair(26, 27)
    x, y = tfn.rescale_01(g.astype(np.float64)), tfn.rescale_01(t.astype(np.float64))
    assert np.abs(rr.ssim_map(x, y, separable=False) - smap).max() <= 1e-12
    # the map's mean is the oracle's ssim
    assert np.abs(smap.mean(axis=(1, 2, 3)) - tfn.ssim(x, y, 5.0)).max() <= 1e-13


@pytest.mark.parametrize("h,w", SMALL)
def test_full_and_empty_regions_reproduce_the_whole_image(h, w):
    g, t, smap = rr.pair(h, w)
    whole = mr.image_metrics(g, t) if h == w else None
    full = rr.region_metrics(g, t, rr.make_region("full", 3, h, w), smap)
    empty = rr.region_metrics(g, t, rr.make_region("empty", 3, h, w), smap)
    assert np.isnan(full[:, 5:10]).all() and np.isnan(empty[:, 0:5]).all()
    assert np.array_equal(full[:, 0:5], empty[:, 5:10])
    assert np.all(full[:, 10] == h * w) and np.all(full[:, 11] == (h - 10) * (w - 10)) and np.all(empty[:, 10:] == 0)
    if whole is not None:
        assert np.abs(full[:, 0:5] - whole).max() <= 1e-12 * np.abs(whole).max()


@pytest.mark.parametrize("h,w", SMALL)
def test_decomposition_identities(h, w):
    g, t, smap = rr.pair(h, w)
    whole = rr.region_metrics(g, t, rr.make_region("full", 3, h, w), smap)[:, 0:5]
    npix, npos = h * w, (h - 10) * (w - 10)
    for name in rr.REGIONS:
        m = rr.region_metrics(g, t, rr.make_region(name, 3, h, w, seed=h), smap)
        n_in, p_in = m[:, 10], m[:, 11]
        z = np.nan_to_num(m, nan=0.0)                          # an empty set contributes 0 * NaN -> nothing
        for j in (0, 3, 4):
            lhs = n_in * z[:, j] + (npix - n_in) * z[:, 5 + j]
            assert np.all(np.abs(lhs - npix * whole[:, j]) <= 1e-12 * npix * np.abs(whole[:, j])), (name, j)
        lhs = p_in * z[:, 2] + (npos - p_in) * z[:, 7]
        assert np.all(np.abs(lhs - npos * whole[:, 2]) <= 1e-12 * npos), name


@pytest.mark.parametrize("h,w", rr.SIZES)
def test_every_region_lands_in_its_branch(h, w):
    npix, npos = h * w, (h - 10) * (w - 10)
    count = {}
    for name in rr.REGIONS:
        r = rr.make_region(name, 3, h, w, seed=h)
        assert r.dtype == np.uint8 and r.shape == (3, h, w) and set(np.unique(r)) <= {0, 1}
        count[name] = (r.sum(axis=(1, 2)), r[:, 5:h - 5, 5:w - 5].sum(axis=(1, 2)))
    assert np.all(count["empty"][0] == 0) and np.all(count["full"][0] == npix) and np.all(count["full"][1] == npos)
    assert np.all(count["corner"][0] == 1) and np.all(count["corner"][1] == 0)          # a pixel, no SSIM position: ssim_in is NaN
    assert np.all(count["centre"][0] == 1) and np.all(count["centre"][1] == 1)          # one position: 3 of 3 * npos map entries
    assert np.all(count["checker"][0] == (npix + 1) // 2) and np.all(count["checker"][1] == (npos + 1) // 2)      # (5, 5) is a set square
    assert np.all(count["block16"][0] == min(16, h - 2) * min(16, w - 4))
    assert np.all(count["left"][0] == h * (w // 2)) and np.all(count["left"][1] == (h - 10) * max(w // 2 - 5, 0))
    if npix >= 37 * 37:
        assert np.all(count["bernoulli"][0] > 0.05 * npix) and np.all(count["bernoulli"][0] < 0.15 * npix)
        assert len(set(count["bernoulli"][0])) > 1                                          # per image, not one mask repeated
    # the sizes: one position; the tile edge; past the pixel pass's cap of 256 blocks of 1024 pixels
    assert (11, 11) in rr.SIZES and (26 - 10, 27 - 10) == (16, 17) and 520 * 520 > 256 * 1024


def test_metrics_cases_land_in_the_nan_branches():
    g, t, smap = rr.pair(37, 37)
    m = rr.region_metrics(g, t, rr.make_region("corner", 3, 37, 37), smap)
    assert np.all(m[:, 10] == 1) and np.all(m[:, 11] == 0) and np.isnan(m[:, 2]).all() and np.isfinite(m[:, [0, 1, 3, 4]]).all()
    assert np.isfinite(m[:, 5:10]).all()
    # +inf: identical images inside the region
    t2 = t.copy()
    r = rr.make_region("left", 3, 37, 37)
    t2[r != 0] = g[r != 0]
    m = rr.region_metrics(g, t2, r)
    assert np.all(m[:, 0] == 0.0) and np.all(m[:, 1] == np.inf) and np.isfinite(m[:, 5:10]).all()


def test_residual_cases_land_in_their_branches():
    for seed, (fh, fw, win) in enumerate(rr.FRAMES):
        src, target, tau, spots = rr.residual_case(2, fh, fw, win, 16.0 / 255.0, seed)
        reg = rr.region_residual(src, win, target, tau).reshape(2, -1)
        assert np.all(reg[:, spots] == [0, 1, 0, 0, 1]), reg[:, spots]
        assert 0.8 < reg.mean() < 0.95         # three differences spread evenly around tau: 7 pixels of 8 have one above it
        d = rr.crop(src, win).reshape(2, -1, 3) - target.reshape(2, -1, 3)
        assert np.all(d[:, spots[0]].max(axis=-1) == np.float32(tau)) and np.isnan(d[:, spots[3], 0]).all()
        assert np.all(d[:, spots[1]].max(axis=-1) == np.nextafter(np.float32(tau), np.float32(1)))
        outside = np.ones((2, fh, fw), bool)
        outside[:, win[0]:win[0] + win[2], win[1]:win[1] + win[3]] = False
        assert not np.isfinite(src[outside]).all() and np.all((src[outside] == np.float32(1e30)) | np.isnan(src[outside]))


# ------------------------------------------------------------------------------------------- modelled faults
def _caught(got, ref):
    return len(rr.mismatches(got, ref)) > 0


def test_modelled_faults_exceed_the_tolerance():
    h = w = 37
    g, t, smap = rr.pair(h, w)
    for name in ("left", "block16", "bernoulli"):
        r = rr.make_region(name, 3, h, w, seed=h)
        ref = rr.region_metrics(g, t, r, smap)
        assert not rr.mismatches(ref, ref)
        # 1. the SSIM position attributed to its top-left pixel instead of its centre
        assert _caught(rr.region_metrics(g, t, r, smap, centre_of=lambda m: m[:h - 10, :w - 10]), ref), name
        # 2. rescale_01 over the region instead of the window: the extremes of the window moved outside the region's range
        g2 = np.array(g)
        inside = r != 0
        g2[~inside] *= 1.5
        ref2 = rr.region_metrics(g2, t, r)
        lo, hi = np.where(inside[..., None], g2, np.inf).min(axis=(1, 2, 3)), np.where(inside[..., None], g2, -np.inf).max(axis=(1, 2, 3))
        x = (g2.astype(np.float64) - lo[:, None, None, None]) / (hi - lo)[:, None, None, None]
        wrong = rr.region_metrics(g2, t, r, rr.ssim_map(x, tfn.rescale_01(t.astype(np.float64))))
        assert _caught(wrong, ref2), name
    # 3. >= instead of >: the pixel planted exactly at tau flips
    fh, fw, win = rr.FRAMES[0]
    src, target, tau, spots = rr.residual_case(2, fh, fw, win, 16.0 / 255.0)
    d = rr.crop(src, win) - target
    with np.errstate(invalid="ignore"):
        ge = (np.max(d, axis=-1) >= np.float32(tau)).astype(np.uint8)
    assert not np.array_equal(ge, rr.region_residual(src, win, target, tau))
    plane = np.full((1, 32, 32), 0.5, np.float32)
    assert rr.region_plane(plane, (0, 0, 32, 32), 0.5).sum() == 0
    # 4. an empty set giving 0
    for name in ("empty", "full", "corner"):
        r = rr.make_region(name, 3, h, w)
        assert _caught(rr.region_metrics(g, t, r, smap, empty=0.0), rr.region_metrics(g, t, r, smap)), name


def test_names_and_header_constants_agree():
    from shmgan_amd import _lib, ops
    assert ops.REGION_METRIC_NAMES == rr.NAMES and len(ops.REGION_METRIC_NAMES) == _lib.CONSTANTS["SHM_REGION_METRICS"] == ops.REGION_METRICS == 12
    assert ops.REGION_METRIC_NAMES[:5] == tuple("in_" + k for k in ops.METRIC_NAMES)
    assert ops.REGION_MODES == {"residual": _lib.CONSTANTS["SHM_REGION_RESIDUAL"], "plane": _lib.CONSTANTS["SHM_REGION_PLANE"]} == {"residual": 0, "plane": 1}
    for fn in ("shm_highlight_region_hw", "shm_image_metrics_region_hw", "shm_image_metrics_region_hw_workspace"):
        assert fn in _lib.SIGNATURES
    import ctypes as C
    I, P, Z = C.c_int, C.c_void_p, C.c_size_t
    assert _lib.SIGNATURES["shm_highlight_region_hw"] == (I, [I, P, P, P, I, I, I, I, I, I, C.c_float, P, I, P])
    assert _lib.SIGNATURES["shm_image_metrics_region_hw"] == (I, [P, I, I, I, I, P, I, I, P, P, P, Z, I, P])


def test_refusals_without_gpu():
    """Shape errors are found on the host before any launch: safe without a GPU (a non-null pointer nobody dereferences)."""
    from shmgan_amd import _lib
    L = _lib.lib()
    p = 1
    assert L.shm_image_metrics_region_hw_workspace(1, 10, 32) == 0 and L.shm_image_metrics_region_hw_workspace(0, 32, 32) == 0
    need = L.shm_image_metrics_region_hw_workspace(2, 32, 40)
    assert need > L.shm_image_metrics_hw_workspace(2, 32, 40) > 0
    for args, code, word in (((p, 32, 40, 0, 0, p, 10, 40, p, p, p, need, 2, None), -1, b"< 11"),
                             ((p, 32, 40, 1, 0, p, 32, 40, p, p, p, need, 2, None), -1, b"outside"),
                             ((p, 32, 40, 0, -1, p, 32, 40, p, p, p, need, 2, None), -1, b"outside"),
                             ((p, 32, 40, 0, 0, p, 32, 40, p, p, p, need, 0, None), -1, b"batch"),
                             ((p, 32, 40, 0, 0, p, 32, 40, None, p, p, need, 2, None), -1, b"null"),
                             ((p, 32, 40, 0, 0, p, 32, 40, p, p, p, need - 1, 2, None), -3, b"workspace")):
        assert L.shm_image_metrics_region_hw(*args) == code and word in L.shm_last_error(), args
    R, PL = 0, 1
    for args, word in (((7, p, p, p, 32, 40, 0, 0, 32, 40, 0.5, p, 1, None), b"mode"),
                       ((R, None, p, None, 32, 40, 0, 0, 32, 40, 0.5, p, 1, None), b"null"),
                       ((R, p, None, None, 32, 40, 0, 0, 32, 40, 0.5, p, 1, None), b"null"),
                       ((PL, p, p, None, 32, 40, 0, 0, 32, 40, 0.5, p, 1, None), b"null"),
                       ((PL, None, None, p, 32, 40, 0, 0, 32, 40, 0.5, None, 1, None), b"null"),
                       ((PL, None, None, p, 32, 40, 0, 0, 32, 40, 0.5, p, 0, None), b"batch"),
                       ((PL, None, None, p, 32, 40, 0, 0, 0, 40, 0.5, p, 1, None), b"side"),
                       ((PL, None, None, p, 32768, 40000, 0, 0, 32, 32769, 0.5, p, 1, None), b"side"),
                       ((PL, None, None, p, 32, 40, 1, 0, 32, 40, 0.5, p, 1, None), b"outside"),
                       ((PL, None, None, p, 32, 40, 0, 9, 32, 32, 0.5, p, 1, None), b"outside")):
        assert L.shm_highlight_region_hw(*args) == -1 and word in L.shm_last_error(), args


def test_region_options_and_monitors():
    from shmgan_amd.telemetry import REGION_MONITORS, improves, region_means, region_options, validation_options
    from shmgan_amd.trainer import _DEFAULTS
    assert {k: _DEFAULTS[k] for k in ("val_region", "val_region_threshold", "metrics_region", "region_threshold")} == \
        {"val_region": "off", "val_region_threshold": None, "metrics_region": "off", "region_threshold": None}
    assert region_options() is None and region_options("off", 0.3) is None
    assert region_options("residual") == ("residual", 16.0 / 255.0) and region_options("specseg") == ("specseg", 0.5)
    assert region_options("specseg", 0.25, "val_region") == ("specseg", 0.25)
    with pytest.raises(ValueError, match="metrics_region"):
        region_options("mask")
    with pytest.raises(ValueError, match="val_region_threshold"):
        region_options("residual", float("nan"), "val_region")
    assert validation_options(val_dir="/x", val_monitor="in_psnr", val_region="residual") == (True, 1, "in_psnr")
    with pytest.raises(ValueError, match="val_monitor.*val_region"):
        validation_options(val_dir="/x", val_monitor="in_psnr")
    with pytest.raises(ValueError, match="val_region"):
        validation_options(val_region="mask")
    assert set(REGION_MONITORS) == set(rr.NAMES[:10])
    assert improves("in_psnr", 2.0, 1.0) and not improves("in_psnr", 1.0, 2.0) and improves("out_mse", 1.0, 2.0) and improves("out_ssim", 0.2, None)
    assert not improves("in_psnr", float("nan"), None) and not improves("in_de94", float("nan"), 3.0)
    # the means: over the images whose set is not empty (ssim: by positions)
    rows = np.full((3, 12), np.nan)
    rows[0, :5], rows[0, 5:10], rows[0, 10:] = 1.0, 10.0, (4, 2)
    rows[1, 5:10], rows[1, 10:] = 20.0, (0, 0)                      # nothing inside
    rows[2, :5], rows[2, 10:] = 3.0, (1369, 729)                    # nothing outside
    rows[0, 2] = 5.0
    means, n_in, n_out = region_means(rows, 37 * 37, 27 * 27)
    assert (n_in, n_out) == (2, 2) and means["in_mse"] == 2.0 and means["in_ssim"] == 4.0 and means["out_de94"] == 15.0
    rows[0, 11] = 0                                                  # a pixel inside, no position: that image leaves the ssim mean only
    means, n_in, _ = region_means(rows, 37 * 37, 27 * 27)
    assert n_in == 2 and means["in_ssim"] == 3.0 and means["in_mse"] == 2.0
    means, n_in, n_out = region_means(rows[1:2], 37 * 37, 27 * 27)
    assert (n_in, n_out) == (0, 1) and np.isnan(means["in_psnr"]) and means["out_psnr"] == 20.0
