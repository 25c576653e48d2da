"""Host-side checks of the rectangular training frame (image_hw): the float64 reference of tests/rect_step_ref.py against the
oracle on squares, its gradients at the GPU parity shapes, modelled kernel faults against the GPU test's tolerances, and the
option's host checks.  No device is needed."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F_

import rect_step_ref as R
from loss_edge_ref import image_oracle, loss_slot_bounds, loss_slots
from oracle import step_torch as st


# ------------------------------------------------------------------------------------------------------- (a) square agreement
def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(1.0, float(np.abs(b).max())))


@pytest.mark.parametrize("B", [1, 2])
def test_square_frame_equals_the_oracle(B):
    """S = 32, F = 16: the four restated functions are array-equal to the oracle's, and train_step_hw gives the oracle's losses,
    outputs and every gradient tensor to 1e-12 relative."""
    S, F = 32, 16
    a, b = R.init_params_hw(F, S, S), st.init_params(F, S)
    for x, y in zip(a, b):
        assert len(x) == len(y) and all(np.array_equal(p, q) for p, q in zip(x, y))
    da, db = R.make_draws_hw(B, B, S, S, F), st.make_draws(B, B, S, F)
    assert da.flags == db.flags and da.target_label == db.target_label
    assert np.array_equal(da.noise, db.noise) and np.array_equal(da.keep_mask, db.keep_mask)
    ia, ib = R.make_inputs_hw(B, S, S), st.make_inputs(B, S)
    assert all(np.array_equal(p, q) for p, q in zip(ia, ib))
    assert R.style_factor_hw(S, S) == st.style_factor_intended(S)
    sf = st.style_factor_intended(S)
    got = R.train_step_hw(*a, ia, da, sf, F)
    ref = st.train_step(*b, ib, db, sf, F)
    for k, v in ref["losses"].items():
        assert abs(got["losses"][k] - v) <= 1e-12 * max(1.0, abs(v)), k
    for k in ("gen_Y", "gen_rgb", "rf_D1", "cls_D1"):
        assert _rel(got["outs"][k], ref["outs"][k]) <= 1e-12, k
    for k in ("gG", "gD"):
        assert len(got[k]) == len(ref[k])
        for i, (x, y) in enumerate(zip(got[k], ref[k])):
            assert _rel(x, y) <= 1e-12, (k, i)


# ------------------------------------------------------------------------------------------------------- (b) gradient norms
@pytest.mark.parametrize("H,W,F,B,step", R.STEP_SHAPES)
def test_no_reference_gradient_vanishes_at_the_parity_shapes(H, W, F, B, step):
    """Every gradient tensor of the float64 reference has norm above 1e-12 at the shapes of the GPU parity test, so that test
    compares all of them (test_train_step_parity skips a tensor below that norm)."""
    g, d, gb, db = R.init_params_hw(F, H, W)
    assert d[6].shape == ((H // 32) * (W // 32) * 16 * F, 5)
    ref = R.train_step_hw(g, d, gb, db, R.make_inputs_hw(B, H, W), R.make_draws_hw(step, B, H, W, F), R.style_factor_hw(H, W), F)
    norms = [float(t.norm()) for t in ref["gD"] + ref["gG"]]
    assert len(norms) == 7 + 46 and min(norms) > 1e-12, norms
    assert all(np.isfinite(v) for v in ref["losses"].values())
    assert tuple(ref["outs"]["gen_Y"].shape) == (B, H, W, 1) and tuple(ref["outs"]["rf_D1"].shape) == (B, H // 32, W // 32, 1)


# ------------------------------------------------------------------------------------------------------- (c) modelled faults
def ssim_map(x, y, max_val=5.0, k1=0.01, k2=0.03):
    """The per-position map oracle.step_torch.ssim averages, [B,3,h-10,w-10]."""
    c = x.shape[-1]
    win = st._gauss_window(x.dtype).view(1, 1, 11, 11).repeat(c, 1, 1, 1)
    xn, yn = x.permute(0, 3, 1, 2), y.permute(0, 3, 1, 2)
    filt = lambda z: F_.conv2d(z, win, groups=c)
    c1, c2 = (k1 * max_val) ** 2, (k2 * max_val) ** 2
    mx, my = filt(xn), filt(yn)
    num0, den0 = mx * my * 2.0, mx * mx + my * my
    return ((num0 + c1) / (den0 + c1)) * ((filt(xn * yn) * 2.0 - num0 + c2) / (filt(xn * xn + yn * yn) - den0 + c2))


@functools.lru_cache(maxsize=None)
def _image_case(B, h, w):
    inp = R.image_inputs_hw(B, h, w, seed=2300 + h + w)
    o = image_oracle(inp, R.IMAGE_FLAGS[0])
    cyuv = [torch.cat([o.cyc_y[k * B:(k + 1) * B], inp.cbcr], 3) for k in range(5)]
    x = [st.rescale_01(c) for c in cyuv]
    y = [st.rescale_01(d) for d in inp.ds]
    return inp, o, x, y


def _scramble(t, h, w):
    """What a kernel that addresses pixel (y, x) as y*h + x reads: element (y*h + x) of the row-major h x w plane (wrapped into the
    plane where the real kernel would leave it)."""
    yy, xx = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    idx = torch.as_tensor(((yy * h + xx) % (h * w)).reshape(-1))
    B, _, _, c = t.shape
    return t.reshape(B, h * w, c)[:, idx].reshape(B, h, w, c)


@pytest.mark.parametrize("B,h,w", R.IMAGE_SHAPES)
def test_modelled_faults_leave_the_tolerances(B, h, w):
    """Four ways a kernel generalised from one side to two can go wrong, each modelled on the float64 reference at the shapes of the
    stand-alone GPU test and held against that test's tolerances (SSIM slots 2e-5 B, the style slot 1e-5 max(1, style), gradients
    rel-L2 1e-4): each of them is visible there."""
    inp, o, x, y = _image_case(B, h, w)
    ho, wo = h - 10, w - 10
    maps = [ssim_map(x[k], y[k]) for k in range(5)]
    true = np.array([float(m.mean(dim=(1, 2, 3)).sum()) for m in maps])
    assert np.abs(true - np.array([float(s.sum()) for s in o.ssims])).max() < 1e-12          # ssim_map restates the oracle's ssim
    tol = 2e-5 * B
    # the SSIM mean over (h-10)^2 positions instead of (h-10)(w-10)
    wrong = np.array([float(m.sum()) / (3.0 * ho * ho) for m in maps])
    assert np.abs(wrong - true).min() > tol
    # p = y*h + x: both images of every window come from the wrong pixels
    wrong = np.array([float(ssim_map(_scramble(x[k], h, w), _scramble(y[k], h, w)).mean(dim=(1, 2, 3)).sum()) for k in range(5)])
    assert np.abs(wrong - true).min() > tol
    # tiles_x on both tile axes: a grid of tiles_x^2 forward tiles, decoded row-major by tiles_x.  On a tall map the tile rows from
    # tiles_x on are never computed; on a wide one the surplus tiles lie below the map and are masked, which is why every wide
    # shape has its transpose in the list
    ty, tx = -(-ho // 16), -(-wo // 16)
    done = torch.zeros(ho, wo)
    done[:min(ty, tx) * 16] = 1.0
    wrong = np.array([float((m * done).sum()) / (3.0 * ho * wo) for m in maps])
    if ty > tx:
        assert np.abs(wrong - true).min() > tol
    else:
        assert np.abs(wrong - true).max() < 1e-12
    # a style factor (or a gram normaliser) from h*h instead of h*w: the style term scales by (w / h)^2
    bad = image_oracle(inp, R.IMAGE_FLAGS[0], sf=3.0e-3 * (w / h) ** 2)
    slot = abs(float(bad.style.sum()) - float(o.style.sum()))
    grad = float((bad.rc - o.rc).norm() / o.rc.norm())
    print(f"({B}, {h}, {w}): style slot moves by {slot:.3g} (bound {loss_slot_bounds(o)[17]:.3g}), dcyc_y by rel-L2 {grad:.3g} (bound 1e-4)")
    assert slot > loss_slot_bounds(o)[17] or grad > 1e-4
    assert loss_slots(o).shape == (18,)


def test_every_tall_shape_shows_the_tile_fault():
    """At least the two tall shapes have more forward tile rows than tile columns."""
    tall = [(B, h, w) for B, h, w in R.IMAGE_SHAPES if -(-(h - 10) // 16) > -(-(w - 10) // 16)]
    assert (1, 43, 11) in tall and (2, 59, 26) in tall


# ------------------------------------------------------------------------------------------------------- (d) host checks
@pytest.mark.parametrize("bad", [(48, 64), (64, 48), (0, 64), (64, 0), (16, 64), (64, 16), 64, (64,), (64, 96, 3), "64x96", (64.0, 96), (-32, 64)])
def test_frame_rule_refusals(bad):
    from shmgan_amd.model import IMAGE_HW_RULE, check_image_hw
    with pytest.raises(ValueError) as e:
        check_image_hw(bad)
    assert "multiples of 32" in str(e.value) and IMAGE_HW_RULE in str(e.value)


def test_frame_rule_accepts_and_the_dense_shape():
    from shmgan_amd.model import check_image_hw, dense_inputs, frame_hw
    assert check_image_hw(None) is None
    assert check_image_hw((64, 96)) == (64, 96) and check_image_hw([32, 32]) == (32, 32) and check_image_hw((np.int64(96), 64)) == (96, 64)
    assert frame_hw(128) == (128, 128) and frame_hw((64, 96)) == (64, 96)
    for H, W, F in [(64, 96, 16), (96, 64, 16), (64, 128, 32), (256, 384, 64)]:
        assert dense_inputs((H, W), F) == (H // 32) * (W // 32) * 16 * F == R.discriminator_spec_hw(F, H, W)[-1][2][0]
    for S, F in [(128, 64), (256, 64), (64, 16)]:
        assert (dense_inputs(S, F), 5) == st.discriminator_spec(F, S)[-1][2]


def test_trainer_refuses_a_bad_frame_before_it_needs_a_device():
    """The option is checked in the constructor, in front of the device lookup."""
    from shmgan_amd import ShmGANwithSSpecSeg
    from types import SimpleNamespace
    for bad in [(48, 64), (16, 32), 96]:
        with pytest.raises(ValueError, match="multiples of 32"):
            ShmGANwithSSpecSeg(image_hw=bad, device="cpu")
        with pytest.raises(ValueError, match="multiples of 32"):
            ShmGANwithSSpecSeg(SimpleNamespace(image_hw=bad), device="cpu")


def test_native_frame_bytes_is_untouched():
    """The memory estimate of native-resolution test mode does not depend on the training frame: the values of the previous
    release."""
    from shmgan_amd.evaluate import native_frame_bytes as nb
    assert nb(48, 64, 16) == NATIVE_48_64_16 and nb(256, 384, 64, torch.bfloat16, cyclic=False, attention=True) == NATIVE_256_384_64
    assert nb(64, 96, 16) == nb(96, 64, 16)


NATIVE_48_64_16, NATIVE_256_384_64 = 7421952, 382107648
