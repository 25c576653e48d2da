"""Guided detail transfer, the parts that need no GPU: the float64 restatement (tests/detail_ref.py) against an independent box filter and
its exact properties, how one NaN spreads, the quality conditions on the two synthetic scenes, the options, and the host-side refusals
of the two entry points and of test mode."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest

from shmgan_amd import _lib
from shmgan_amd import evaluate as ev

import detail_ref as dr

P, I, F = C.c_void_p, C.c_int, C.c_float


def test_box_mean_against_an_independent_formulation():
    """The brute-force clipped mean against scipy's uniform_filter where no window is clipped, and against an integral image everywhere."""
    try:
        from scipy.ndimage import uniform_filter
    except ImportError:                     # the integral image alone is then the independent formulation
        uniform_filter = None
    rng = np.random.default_rng(0)
    for (H, W), r in (((32, 48), 1), ((33, 70), 3), ((48, 80), 8), ((5, 7), 8), ((1, 64), 2), ((64, 1), 2), ((9, 11), 0)):
        x = rng.normal(2.0, 0.8, (H, W))
        got = dr.box_mean(x, r)
        np.testing.assert_allclose(got, dr.box_mean_integral(x, r), rtol=0, atol=1e-12)
        if uniform_filter is not None and H > 2 * r and W > 2 * r:
            want = uniform_filter(x, size=2 * r + 1, mode="constant")
            np.testing.assert_allclose(got[r:H - r, r:W - r], want[r:H - r, r:W - r], rtol=0, atol=1e-12)
    # a corner window of a 4 x 5 plane at radius 1 holds 4 values, an edge window 6, the interior 9
    x = np.arange(20.0).reshape(4, 5)
    got = dr.box_mean(x, 1)
    assert got[0, 0] == (0 + 1 + 5 + 6) / 4 and got[0, 2] == (1 + 2 + 3 + 6 + 7 + 8) / 6 and got[1, 1] == x[0:3, 0:3].mean()


def test_exact_properties_of_the_restatement():
    rng = np.random.default_rng(1)
    I_ = rng.normal(2.0, 0.8, (12, 17))
    p = I_ + rng.normal(0.0, 0.5, I_.shape)
    # radius 0: (0, p - I) exactly -- the plain residual transfer, in float64 and in the float32 restatement
    c = dr.coeffs(I_, p, 0, 1e-2)
    assert np.array_equal(c[..., 0], np.zeros_like(I_)) and np.array_equal(c[..., 1], p - I_)
    I32, p32 = I_.astype(np.float32), p.astype(np.float32)
    c32 = dr.coeffs_f32(I32, p32, 0, 1e-2)
    assert c32.dtype == np.float32 and np.array_equal(c32[..., 0], np.zeros_like(I32)) and np.array_equal(c32[..., 1], p32 - I32)
    # a plane smaller than the window: constant coefficients, the global regression of d on I
    Is = rng.normal(2.0, 0.8, (5, 7))
    ds = rng.normal(0.0, 0.5, (5, 7))
    eps = 1e-4
    c = dr.coeffs(Is, Is + ds, 8, eps)
    a = ((Is * ds).mean() - Is.mean() * ds.mean()) / (Is.var() + eps)
    b = ds.mean() - a * Is.mean()
    np.testing.assert_allclose(c[..., 0], a, rtol=0, atol=1e-12)
    np.testing.assert_allclose(c[..., 1], b, rtol=0, atol=1e-12)
    # d = alpha I + beta: a = alpha var / (var + eps) in every window
    alpha, beta, r, eps = -0.7, 0.3, 2, 1e-2
    var = dr.box_mean(I_ * I_, r) - dr.box_mean(I_, r) ** 2
    a = alpha * var / (var + eps)
    c = dr.coeffs(I_, I_ + alpha * I_ + beta, r, eps)
    np.testing.assert_allclose(c[..., 0], dr.box_mean(a, r), rtol=0, atol=1e-12)
    # the reference value does not enter (var and cov are shift-invariant)
    np.testing.assert_allclose(dr.coeffs(I_, p, 2, 1e-2, ref=0.0), dr.coeffs(I_, p, 2, 1e-2, ref=1.7), rtol=0, atol=1e-12)


def test_one_nan_spreads_to_its_5x5_block_and_no_further():
    rng = np.random.default_rng(2)
    I_ = rng.normal(2.0, 0.8, (32, 48))
    p = I_ + rng.normal(0.0, 0.5, I_.shape)
    p[13, 29] = np.nan
    c = dr.coeffs(I_, p, 1, 1e-2)
    want = np.zeros((32, 48), bool)
    want[11:16, 27:32] = True
    assert np.array_equal(np.isnan(c[..., 0]), want) and np.array_equal(np.isnan(c[..., 1]), want)
    assert np.isfinite(c[~want]).all()
    # an infinity: the same block, and NaN there (Inf - Inf in cov), not an infinity of either sign
    p[13, 29] = np.inf
    c = dr.coeffs(I_, p, 1, 1e-2)
    assert np.array_equal(np.isnan(c[..., 0]), want) and np.array_equal(np.isnan(c[..., 1]), want) and not np.isinf(c).any()
    # the sampler: a NaN tap poisons a pixel even at weight 0 (identity size: tr = tl, weight 0)
    s = dr.sample(c, 32, 48)
    assert np.array_equal(np.isnan(s), np.isnan(c))


@pytest.fixture(scope="module")
def scenes():
    return {kind: dr.scene_mses(dr.scene(kind, seed)) for kind, seed in (("smooth", 11), ("hard", 12))}


def test_quality_conditions_on_the_two_scenes(scenes):
    """192 x 256 photo, 64 x 64 frame, eps 1e-2, an ideal network: MSE against the full-resolution diffuse image in gen_rgb's units."""
    for kind, m in scenes.items():
        print(kind, {str(k): round(v, 6) for k, v in m.items()}, {str(k): round(v / m["bilinear"], 4) for k, v in m.items()})
        for key in ("residual", ("guided", 1), ("guided", 2)):
            assert m[key] < m["bilinear"] / 5, (kind, key, m[key], m["bilinear"])
    assert scenes["hard"][("guided", 1)] < scenes["hard"]["residual"]           # the bilinear residual leaves a halo along the edge
    assert scenes["smooth"]["residual"] < scenes["smooth"][("guided", 1)]


def test_detail_options_accept_and_refuse_by_name():
    from shmgan_amd.trainer import _DEFAULTS
    assert {k: _DEFAULTS[k] for k in ("image_detail", "detail_radius", "detail_eps")} == dict(image_detail="off", detail_radius=2, detail_eps=1e-2)
    assert ev.detail_options() is None and ev.detail_options("off", 99, -1) is None
    assert ev.detail_options("guided") == ("guided", 2, 1e-2)
    assert ev.detail_options("guided", 8, 0.5) == ("guided", 8, 0.5) and ev.detail_options("guided", 1, 1) == ("guided", 1, 1.0)
    assert ev.detail_options("residual", 5, 1e-3) == ("residual", 0, 1e-3)
    for bad in ("on", "Guided", 1, "bilinear"):
        with pytest.raises(ValueError, match="image_detail"):
            ev.detail_options(bad)
    for bad in (0, 9, -1, 2.0, "2", True):
        with pytest.raises(ValueError, match="detail_radius"):
            ev.detail_options("guided", bad)
    for bad in (0, -1e-2, float("nan"), float("inf"), "1e-2"):
        with pytest.raises(ValueError, match="detail_eps"):
            ev.detail_options("guided", 2, bad)
        with pytest.raises(ValueError, match="detail_eps"):
            ev.detail_options("residual", 2, bad)


def test_entry_points_refuse_on_the_host():
    """Both entry points check their arguments before any launch: safe without a GPU.  Each refusal is SHM_E_SHAPE and names the argument."""
    want = {"shm_detail_coeffs": (I, [P, I, P, I, P, I, I, I, I, F, P]), "shm_detail_apply_u8": (I, [P, I, I, P, I, I, P, P, P])}
    L = _lib.lib()
    for name, sig in want.items():
        assert name in _lib.header_functions() and _lib.SIGNATURES[name] == sig and hasattr(L, name), name
    p = 256                     # a non-null, aligned pointer nobody dereferences

    def coeffs(guide=p, ldg=3, target=p, ldt=1, coef=p, batch=1, h=32, w=48, radius=2, eps=1e-2):
        return L.shm_detail_coeffs(guide, ldg, target, ldt, coef, batch, h, w, radius, eps, None), L.shm_last_error()

    def apply(photo=p, h=100, w=75, coef=p, hm=32, wm=48, scale=p, out=p):
        return L.shm_detail_apply_u8(photo, h, w, coef, hm, wm, scale, out, None), L.shm_last_error()

    for kw, word in ((dict(guide=None), b"null pointer"), (dict(target=None), b"null pointer"), (dict(coef=None), b"null pointer"),
                     (dict(radius=9), b"radius 9"), (dict(radius=-1), b"radius -1"), (dict(eps=0.0), b"eps"), (dict(eps=-1.0), b"eps"),
                     (dict(eps=float("nan")), b"eps"), (dict(h=0), b"h 0"), (dict(w=0), b"w 0"), (dict(h=32769), b"h 32769"),
                     (dict(w=32769), b"w 32769"), (dict(ldg=0), b"ldg 0"), (dict(ldt=0), b"ldt 0"), (dict(batch=0), b"batch 0"),
                     (dict(coef=260), b"coef")):
        rc, msg = coeffs(**kw)
        assert rc == -1 and msg.startswith(b"shm_detail_coeffs:") and word in msg, (kw, rc, msg)
    for kw, word in ((dict(photo=None), b"null pointer"), (dict(coef=None), b"null pointer"), (dict(scale=None), b"null pointer"),
                     (dict(out=None), b"null pointer"), (dict(h=0), b"h 0"), (dict(w=32769), b"w 32769"), (dict(hm=0), b"H 0"),
                     (dict(wm=32769), b"W 32769"), (dict(photo=258), b"photo"), (dict(out=264), b"out"), (dict(coef=260), b"coef")):
        rc, msg = apply(**kw)
        assert rc == -1 and msg.startswith(b"shm_detail_apply_u8:") and word in msg, (kw, rc, msg)


def test_test_mode_refuses_before_touching_the_device(tmp_path):
    stub = SimpleNamespace(args=SimpleNamespace(), image_size=32, device=None, result_dir=str(tmp_path / "r"))
    base = dict(test_dir=str(tmp_path / "absent"))
    with pytest.raises(ValueError, match="image_detail='guided'.*eval_size='model'"):
        ev.test(stub, SimpleNamespace(image_detail="guided", eval_size="native", **base))
    with pytest.raises(ValueError, match="image_detail='residual'.*image_out_size='source'"):
        ev.test(stub, SimpleNamespace(image_detail="residual", save_images="g1", image_out_size="model", **base))
    with pytest.raises(ValueError, match="detail_radius"):
        ev.test(stub, SimpleNamespace(image_detail="guided", detail_radius=0, **base))
    with pytest.raises(ValueError, match="image_detail"):
        ev.test(stub, SimpleNamespace(image_detail="sharp", **base))
    # off (or absent): none of these options is looked at, and the run goes on to its file lists as it always did
    with pytest.raises((FileNotFoundError, ValueError), match="absent"):
        ev.test(stub, SimpleNamespace(image_detail="off", detail_radius=0, eval_size="model", save_images="g1", image_out_size="model", **base))


def test_ops_refuse_by_shape_and_dtype_without_a_launch():
    """ops.detail_coeffs / detail_apply_u8 check dtype, device, shape and contiguity before they call the library."""
    import torch
    from shmgan_amd import ops
    g = torch.zeros(1, 4, 6)
    with pytest.raises(TypeError, match="float32 device planes"):
        ops.detail_coeffs(g, g, 1, 1e-2)
    with pytest.raises(TypeError, match="float32 device planes"):
        ops.detail_coeffs(g.double(), g, 1, 1e-2)
    with pytest.raises(ValueError, match="uint8"):
        ops.detail_apply_u8(torch.zeros(4, 6, 3), torch.zeros(4, 6, 2), torch.ones(1))
    with pytest.raises(ValueError, match="uint8"):
        ops.detail_apply_u8(torch.zeros(4, 6, 3, dtype=torch.uint8), torch.zeros(4, 6, 2), torch.ones(1))     # a host photo
