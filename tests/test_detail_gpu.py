"""Guided detail transfer on the GPU: ops.detail_coeffs (shm_detail_coeffs) and ops.detail_apply_u8 (shm_detail_apply_u8) against the float64
restatement (tests/detail_ref.py), their exact properties, how non-finite values spread, and trainer.refine / evaluate.test(image_detail=...)
end to end on the tiny model."""
import functools
import json
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from shmgan_amd import ops
from shmgan_amd import evaluate as ev

import detail_ref as dr
import export_ref as xr
from util import host

pytestmark = pytest.mark.gpu

# (H, W), radius, eps, guide pitch
COEF_CASES = [((32, 48), 1, 1e-2, 3), ((32, 32), 2, 1e-2, 1), ((48, 80), 8, 1e-3, 1), ((33, 70), 3, 1e-2, 1), ((5, 7), 8, 1e-4, 1),
              ((1, 64), 2, 1e-2, 1), ((64, 1), 2, 1e-2, 1)]
CASE_IDS = [f"{h}x{w}-r{r}" for (h, w), r, _, _ in COEF_CASES]


@functools.lru_cache(maxsize=None)
def _inputs(hw, seed=0, batch=3):
    """I = N(2, 0.8) and p = I + N(0, 0.5) as the device holds them (float32), [batch,H,W]."""
    rng = np.random.default_rng([seed, hw[0], hw[1]])
    I = rng.normal(2.0, 0.8, (batch,) + hw).astype(np.float32)
    p = (I + rng.normal(0.0, 0.5, I.shape).astype(np.float32)).astype(np.float32)
    return I, p


@functools.lru_cache(maxsize=None)
def _reference(case):
    """Per image of the case: (float64 coefficients, tolerance, the float32 restatement's own error).  Computed once per session."""
    hw, r, eps, _ = COEF_CASES[case]
    I, p = _inputs(hw)
    out = []
    for b in range(I.shape[0]):
        ref = dr.coeffs(I[b], p[b], r, eps)
        tol, err = dr.coeff_tolerance(I[b], p[b], r, eps, ref)
        out.append((ref, tol, err))
    return out


def _device_planes(I, p, pitch):
    """The two planes on the device: the guide as channel 0 of a [B,H,W,pitch] tensor whose other channels hold a sentinel, the target tight."""
    g = torch.full(I.shape + (pitch,), 1.0e30, dtype=torch.float32, device="cuda")
    g[..., 0] = torch.from_numpy(I).cuda()
    return g[..., 0], torch.from_numpy(p).cuda().unsqueeze(-1).contiguous()


RATIOS = {}


@pytest.mark.parametrize("batch", [1, 3])
@pytest.mark.parametrize("case", range(len(COEF_CASES)), ids=CASE_IDS)
def test_coefficients_match_the_restatement(case, batch):
    hw, r, eps, pitch = COEF_CASES[case]
    I, p = _inputs(hw)
    g, t = _device_planes(I[:batch], p[:batch], pitch)
    assert g.stride(2) == pitch
    got = host(ops.detail_coeffs(g, t, r, eps))
    assert got.shape == (batch,) + hw + (2,)
    for b, (ref, tol, err) in enumerate(_reference(case)[:batch]):
        d = float(np.abs(got[b] - ref).max())
        RATIOS[(CASE_IDS[case], batch, b)] = d / tol
        print(f"{CASE_IDS[case]} batch {batch} image {b}: device error {d:.3e}, float32 restatement {err:.3e}, tolerance {tol:.3e}, ratio {d / tol:.3f}")
        assert d <= tol, (CASE_IDS[case], batch, b, d, tol)
    # radius 0, any eps: (0, p - I) bit for bit
    c0 = ops.detail_coeffs(g, t, 0, eps).cpu().numpy()
    assert np.array_equal(c0[..., 0], np.zeros_like(I[:batch])) and np.array_equal(c0[..., 1], p[:batch] - I[:batch])


def test_coefficients_are_deterministic_and_batch_invariant():
    for case in (0, 2, 3):
        hw, r, eps, pitch = COEF_CASES[case]
        I, p = _inputs(hw)
        g, t = _device_planes(I, p, pitch)
        a = ops.detail_coeffs(g, t, r, eps).clone()
        assert torch.equal(a, ops.detail_coeffs(g, t, r, eps))
        for b in range(3):
            g1, t1 = _device_planes(I[b:b + 1], p[b:b + 1], 1)
            assert torch.equal(a[b:b + 1], ops.detail_coeffs(g1, t1, r, eps)), (case, b)


def _photo(hw, seed):
    return np.random.default_rng([7, seed, hw[0], hw[1]]).integers(0, 256, hw + (3,), dtype=np.uint8)


def _apply_check(photo, coef_dev, scale, what):
    """The device's apply against the restatement fed the device's own coefficients; the tolerance comes from these inputs."""
    sc = torch.tensor([scale], dtype=torch.float32, device="cuda")
    got = ops.detail_apply_u8(torch.from_numpy(photo).cuda(), coef_dev, sc)
    assert got.shape == photo.shape and got.dtype == torch.float32
    want, (ymax, amax, bmax) = dr.apply(photo, host(coef_dev), float(sc.cpu()[0]))
    tol = dr.apply_tolerance(ymax, amax, bmax)
    g = host(got)
    assert np.array_equal(np.isnan(g), np.isnan(want)), (what, int(np.isnan(g).sum()), int(np.isnan(want).sum()))
    assert np.array_equal(np.isposinf(g), np.isposinf(want)) and np.array_equal(np.isneginf(g), np.isneginf(want)), what
    fin = np.isfinite(want)
    d = float(np.abs(g[fin] - want[fin]).max()) if fin.any() else 0.0
    print(f"{what}: apply error {d:.3e}, tolerance {tol:.3e} (M = {ymax * (1 + amax) + bmax:.3f})")
    assert d <= tol, (what, d, tol)
    return got


APPLY_CASES = [(0, (37, 53)), (0, (100, 75)), (0, (32, 48)), (0, (20, 24)), (0, (1, 1)), (4, (64, 64)), (0, (3, 5)), (0, (257, 4))]


@pytest.mark.parametrize("case,photo_hw", APPLY_CASES, ids=[f"{CASE_IDS[c]}-to-{h}x{w}" for c, (h, w) in APPLY_CASES])
def test_apply_matches_the_restatement(case, photo_hw):
    """Photos larger and smaller than the frame, the identity, one pixel, and pixel counts that are no multiple of four (37 x 53, 3 x 5, 1 x 1:
    the tail of the flat four-per-lane walk) or of a block (257 x 4 = 1028)."""
    hw, r, eps, pitch = COEF_CASES[case]
    I, p = _inputs(hw)
    g, t = _device_planes(I[:1], p[:1], pitch)
    coef = ops.detail_coeffs(g, t, r, eps)[0]
    _apply_check(_photo(photo_hw, case), coef, 0.23, (CASE_IDS[case], photo_hw))


def test_target_equal_to_guide_changes_nothing():
    hw = (32, 48)
    I, _ = _inputs(hw)
    g, _ = _device_planes(I[:1], I[:1], 3)
    t = g.clone().unsqueeze(-1).contiguous()
    photo = torch.from_numpy(_photo((100, 75), 1)).cuda()
    sc = torch.tensor([0.31], dtype=torch.float32, device="cuda")
    base = ops.detail_apply_u8(photo, ops.detail_coeffs(g, t, 0, 1e-2)[0], sc)
    for r in (0, 1, 2, 5, 8):
        coef = ops.detail_coeffs(g, t, r, 1e-2)
        assert float(coef.abs().max()) == 0.0, r
        assert torch.equal(ops.detail_apply_u8(photo, coef[0], sc), base), r
    # ... and what it leaves is the photo itself in gen_rgb's units
    want = dr.yuv_to_rgb(dr.photo_yuv(photo.cpu().numpy(), float(sc.cpu()[0])))
    assert float(np.abs(host(base) - want).max()) <= dr.apply_tolerance(float(np.abs(want).max()), 0.0, 0.0)


def test_identity_size_and_radius_0_is_yuv2rgb_of_the_generated_plane():
    """At photo size == frame size the residual transfer returns yuv_to_rgb([gen_Y, CbCr of the input]) = gen_rgb, within the apply's
    bound ((p - I) + I is not p in fp32)."""
    H, W = 32, 48
    photo = torch.from_numpy(_photo((H, W), 2)).cuda()
    rgb = torch.empty((1, H, W, 3), dtype=torch.float32, device="cuda")
    ops.load_pad_u8(photo, rgb[0], 0, 0)
    yuv, acc, scale = torch.empty_like(rgb), torch.zeros(2, dtype=torch.float64, device="cuda"), torch.empty(1, device="cuda")
    ops.rgb2yuv_std(rgb, yuv, acc, scale, 1, H * W)
    _, p = _inputs((H, W))
    gen_y = torch.from_numpy(p[:1]).cuda().unsqueeze(-1).contiguous()
    want = torch.empty_like(rgb)
    ops.yuv2rgb(gen_y, yuv[..., 1:].contiguous(), None, want, None, 1, 1, H * W)
    coef = ops.detail_coeffs(yuv[..., 0], gen_y, 0, 1e-2)
    got = ops.detail_apply_u8(photo, coef[0], scale)
    y = host(yuv[..., 0])
    tol = dr.apply_tolerance(float(np.abs(host(yuv)).max()), 0.0, float(np.abs(host(gen_y)[..., 0] - y).max()))
    d = float((got - want[0]).abs().max())
    print(f"identity, radius 0 against yuv2rgb: {d:.3e}, tolerance {tol:.3e}")
    assert d <= tol
    assert torch.equal(got, ops.detail_apply_u8(photo, coef[0], scale))          # two runs, the same bits


NONFINITE_AT = (((12, 12), np.nan), ((19, 24), np.inf), ((12, 35), -np.inf))      # at least 12 pixels from each other and from the border


@pytest.mark.parametrize("r", [1, 2])
def test_non_finite_values_stay_where_the_restatement_puts_them(r):
    """One NaN, one +Inf and one -Inf in the target of a 32 x 48 plane: the coefficients are non-finite on the (4r+1)^2 blocks around them
    and nowhere else -- a running box sum would carry them down the row -- and so is the refined plane at 100 x 75."""
    hw, eps = (32, 48), 1e-2
    I, p = _inputs(hw, seed=3, batch=1)
    p = p.copy()
    for (y, x), v in NONFINITE_AT:
        p[0, y, x] = v
    ref = dr.coeffs(I[0], p[0], r, eps)
    tol, err = dr.coeff_tolerance(I[0], p[0], r, eps, ref)
    block = np.zeros(hw, bool)
    for (y, x), _ in NONFINITE_AT:
        block[y - 2 * r:y + 2 * r + 1, x - 2 * r:x + 2 * r + 1] = True
    assert np.array_equal(~np.isfinite(ref[..., 0]), block) and np.array_equal(~np.isfinite(ref[..., 1]), block)
    g, t = _device_planes(I, p, 3)
    coef = ops.detail_coeffs(g, t, r, eps)
    got = host(coef)[0]
    assert np.array_equal(np.isnan(got), np.isnan(ref)), (int(np.isnan(got).sum()), int(np.isnan(ref).sum()))
    assert np.array_equal(np.isposinf(got), np.isposinf(ref)) and np.array_equal(np.isneginf(got), np.isneginf(ref))
    fin = np.isfinite(ref)
    d = float(np.abs(got[fin] - ref[fin]).max())
    print(f"non-finite, r {r}: device error {d:.3e}, float32 restatement {err:.3e}, tolerance {tol:.3e}")
    assert d <= tol
    out = _apply_check(_photo((100, 75), 3), coef[0], 0.23, ("non-finite", r))
    bad = ~np.isfinite(host(out)).all(axis=-1)
    assert bad.any() and not bad.all(axis=0).any() and not bad.all(axis=1).any()          # three patches: no row and no column is lost


# ---------------------------------------------------------------------------------------------------------------------
# trainer.refine and evaluate.test(image_detail=...) on the tiny model the other end-to-end tests use
S_E2E, F_E2E = 64, 16
SIZES = [(80, 112), (45, 70)]


def _write_images(tmp_path):
    from PIL import Image
    rng = np.random.default_rng(5)
    for sub in ("test", "diffuse"):
        d = tmp_path / sub
        d.mkdir()
        for i, (h, w) in enumerate(SIZES):
            Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)).save(d / f"img{i:02d}.png")
    return tmp_path / "test", tmp_path / "diffuse"


def _trainer(tmp_path, tag):
    from shmgan_amd import ShmGANwithSSpecSeg
    return ShmGANwithSSpecSeg(image_size=S_E2E, filter_size=F_E2E, batch_size=1, checkpoint_save_dir=str(tmp_path / "ckpt"),
                              log_dir=str(tmp_path / f"logs_{tag}"), result_dir=str(tmp_path / f"results_{tag}"))


def _args(tmp_path, **kw):
    return SimpleNamespace(test_dir=str(tmp_path / "test"), diffuse_dir=str(tmp_path / "diffuse"), calc_metrics=True, eval_batch_size=2, **kw)


def _png(path):
    from PIL import Image
    with Image.open(path) as im:
        return np.array(im)


def test_refine_and_test_mode(tmp_path):
    from shmgan_amd.data import EvalDataset
    test_dir, diffuse_dir = _write_images(tmp_path)
    m = _trainer(tmp_path, "a").build(seed=7, beta_seed=8)
    (tmp_path / "ckpt").mkdir()
    m.save_npz(str(tmp_path / "ckpt" / "ckpt-1.npz"))
    with pytest.raises(ValueError, match="refine follows an infer"):
        m.refine([])

    # ---- the loader keeps the decoded bytes only when asked, and yields the same either way
    plain = EvalDataset(test_dir, S_E2E, 2, diffuse_dir)
    rgb0, dif0 = plain.batch(0)
    assert plain.last_source is None
    ds = EvalDataset(test_dir, S_E2E, 2, diffuse_dir, keep_source=True)
    rgb, dif = ds.batch(0)
    assert torch.equal(rgb, rgb0) and torch.equal(dif, dif0)
    photos, partners = ds.last_source
    assert [tuple(t.shape) for t in photos] == [s + (3,) for s in SIZES] == [tuple(t.shape) for t in partners]
    assert all(t.dtype == torch.uint8 and t.is_cuda for t in photos + partners)
    assert np.array_equal(photos[1].cpu().numpy(), _png(test_dir / "img01.png"))

    # ---- refine() after infer() is the ops path, for both modes
    m.infer(rgb)
    yuv, gen_y, scale = m._inf_planes
    planes = {}
    for mode, r in (("residual", 0), ("guided", 2)):
        got = m.refine(photos, mode=mode)
        coef = ops.detail_coeffs(yuv[..., 0], gen_y, r, 1e-2)
        for b in range(2):
            assert tuple(got[b].shape) == SIZES[b] + (3,)
            assert torch.equal(got[b], ops.detail_apply_u8(photos[b], coef[b], scale[b:b + 1])), (mode, b)
        planes[mode] = got
    assert not torch.equal(planes["residual"][0], planes["guided"][0])
    assert any(k[0] == "inf/detail_coef" for k in m.arena.t)                 # under the prefix _frame_changed drops
    with pytest.raises(ValueError, match="3 photos for the batch of 2"):
        m.refine(photos + photos[:1])
    with pytest.raises(ValueError, match="radius"):
        m.refine(photos, radius=9)
    # ... and the float64 restatement of the whole path, fed the device's planes
    c64 = dr.coeffs(host(yuv[0, ..., 0]), host(gen_y[0, ..., 0]), 2, 1e-2)
    want, (ymax, amax, bmax) = dr.apply(photos[0].cpu().numpy(), c64, float(scale[0]))
    ctol, _ = dr.coeff_tolerance(yuv[0, ..., 0].cpu().numpy(), gen_y[0, ..., 0].cpu().numpy(), 2, 1e-2, c64)
    tol = dr.apply_tolerance(ymax, amax, bmax) + dr.Y2R_ROW_SUM * ctol * (ymax + 1.0)      # the apply's rounding + the coefficients' tolerance carried through
    assert float(np.abs(host(planes["guided"][0]) - want).max()) <= tol

    # ---- test mode: off (or absent) is the parent's path
    r_absent = ev.test(m, _args(tmp_path, save_images="g1", image_dir=str(tmp_path / "img_absent")))
    r_off = ev.test(m, _args(tmp_path, save_images="g1", image_dir=str(tmp_path / "img_off"), image_detail="off"))
    names = [ev.image_name(f"img{i:02d}", "G1") for i in range(2)]
    for r_ in (r_absent, r_off):
        assert "detail" not in r_
    for n in names:
        assert (tmp_path / "img_absent" / n).read_bytes() == (tmp_path / "img_off" / n).read_bytes()
    assert not (tmp_path / "results_a" / ev.DETAIL_FILE).exists()

    # ---- test mode with the option: G1 from the refined plane at the photo's size, the refined plane scored, the rest untouched
    r_on = ev.test(m, _args(tmp_path, save_images="g1", image_dir=str(tmp_path / "img_on"), image_detail="guided"))
    for key in ev.METRIC_KEYS + ["means", "index", "images"]:
        assert r_on[key] == r_off[key], key
    assert len(r_on["time"]) == len(r_off["time"]) == 2 and set(r_on) == set(r_off) | {"detail"}
    assert sorted(os.listdir(tmp_path / "img_on")) == names
    rgb, dif = ds.batch(0)                         # the same batch again: the planes test() refined are these, bit for bit
    m.evaluate(rgb, dif)
    photos, partners = ds.last_source
    refined = m.refine(photos, "guided", 2, 1e-2)
    det = r_on["detail"]
    assert (det["mode"], det["radius"], det["eps"]) == ("guided", 2, 1e-2)
    for i, (h, w) in enumerate(SIZES):
        a = _png(tmp_path / "img_on" / names[i])
        assert a.shape == (h, w, 3)
        want, y = xr.export(host(refined[i]), h, w, "rescale")
        dlt = np.abs(a.astype(np.int64) - want.astype(np.int64))
        far = ~xr.near_half(y)
        assert np.all(dlt[far] == 0) and dlt.max() <= 1, (i, int(dlt.max()))
        assert not np.array_equal(a, _png(tmp_path / "img_off" / names[i]))
        target = torch.empty((1, h, w, 3), dtype=torch.float32, device="cuda")
        ops.load_pad_u8(partners[i], target[0], 0, 0)
        mt = ops.image_metrics_hw(refined[i].unsqueeze(0), (0, 0, h, w), target).cpu()[0].tolist()
        assert [det[k][i] for k in ev.METRIC_KEYS] == mt, i
    assert det["means"] == {k: sum(det[k]) / 2 for k in ev.METRIC_KEYS}
    lines = [json.loads(s) for s in (tmp_path / "results_a" / ev.DETAIL_FILE).read_text().splitlines()]
    assert [ln["image"] for ln in lines] == ["img00", "img01"] and [tuple(ln["size"]) for ln in lines] == SIZES
    assert [lines[1][k] for k in ev.METRIC_KEYS] == [det[k][1] for k in ev.METRIC_KEYS]
    # residual mode reports radius 0; without save_images and metrics nothing is refined
    r_res = ev.test(m, _args(tmp_path, image_detail="residual"))
    assert r_res["detail"]["radius"] == 0 and len(r_res["detail"]["MSE"]) == 2 and r_res["files"] == []
    assert r_res["detail"]["MSE"] != det["MSE"]
    # without calc_metrics the planes are still made and written; nothing is scored
    r_nc = ev.test(m, SimpleNamespace(test_dir=str(test_dir), eval_batch_size=1, save_images="g1", image_dir=str(tmp_path / "img_nc"),
                                      image_detail="residual"))
    assert r_nc["detail"]["mode"] == "residual" and r_nc["detail"]["MSE"] == [] and r_nc["means"] is None
    assert [_png(tmp_path / "img_nc" / n).shape for n in names] == [s + (3,) for s in SIZES]
    # a diffuse partner of another size than its photo
    from PIL import Image
    Image.fromarray(np.zeros((45, 71, 3), np.uint8)).save(diffuse_dir / "img01.png")
    with pytest.raises(ValueError, match=r"img01\.png is 45 x 70.*img01\.png is 45 x 71"):
        ev.test(m, _args(tmp_path, image_detail="guided"))
