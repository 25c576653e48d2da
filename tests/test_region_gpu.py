"""The region metrics on the GPU: ops.highlight_region (shm_highlight_region_hw) and ops.image_metrics_region
(shm_image_metrics_region_hw) against the float64 restatement of tests/region_ref.py on its whole case table, their equality with
ops.image_metrics_hw for a full and an empty region, the two decomposition identities, reproducibility, batch invariance, the
refusals, and the option end to end: test mode per region source, and validation with val_monitor="in_psnr"."""
import argparse
import json
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from shmgan_amd import _lib, ops
from shmgan_amd import evaluate as ev

import region_ref as rr
from util import dev as _dev, host

pytestmark = pytest.mark.gpu

TAU = 16.0 / 255.0


def dev(a):
    """util.dev of a copy: the shared arrays of region_ref.pair are read-only."""
    return _dev(np.array(a, dtype=np.float32))


def _u8(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint8)).cuda()


# ------------------------------------------------------------------------------------------------- the region builder
@pytest.mark.parametrize("B", rr.BATCHES)
def test_residual_region_is_exact(B):
    cases = [(fh, fw, win) for fh, fw, win in rr.FRAMES] + [(h, w, (0, 0, h, w)) for h, w in rr.SIZES[:7]] + [(1, 1, (0, 0, 1, 1))]
    for seed, (fh, fw, win) in enumerate(cases):
        if win[2] * win[3] >= 5:
            src, target, tau, spots = rr.residual_case(B, fh, fw, win, TAU, seed)
        else:
            src, target, tau = np.full((B, 1, 1, 3), 0.5, np.float32), np.zeros((B, 1, 1, 3), np.float32), TAU
        want = rr.region_residual(src, win, target, tau)
        got = ops.highlight_region("residual", win, src=dev(src), target=dev(target), tau=tau)
        assert got.dtype == torch.uint8 and tuple(got.shape) == (B, win[2], win[3])
        assert np.array_equal(got.cpu().numpy(), want), (fh, fw, win)
        if win[2] * win[3] >= 5:
            assert np.all(want.reshape(B, -1)[:, spots] == [0, 1, 0, 0, 1])          # at tau, an ulp above, an ulp below, NaN, one channel
    # into a given buffer, every byte written (0 or 1 over a fill of 7)
    fh, fw, win = rr.FRAMES[0]
    src, target, tau, _ = rr.residual_case(B, fh, fw, win, TAU)
    out = torch.full((B, win[2], win[3]), 7, dtype=torch.uint8, device="cuda")
    assert ops.highlight_region("residual", win, src=dev(src), target=dev(target), tau=tau, out=out) is out
    assert np.array_equal(out.cpu().numpy(), rr.region_residual(src, win, target, tau))


@pytest.mark.parametrize("B", rr.BATCHES)
def test_plane_region_is_exact(B):
    for seed, (fh, fw, win) in enumerate(rr.FRAMES + [(64, 64, (0, 0, 64, 64)), (520, 528, (0, 3, 520, 520))]):
        top, left, h, w = win
        rng = np.random.default_rng(50 + seed)
        p = rng.uniform(0.0, 1.0, (B, h, w)).astype(np.float32)
        p[:, 0, 0], p[:, h - 1, w - 1], p[:, h // 2, w // 2] = 0.5, np.nextafter(np.float32(0.5), np.float32(1)), np.nan
        p[:, 0, w - 1], p[:, h - 1, 0] = np.inf, -np.inf
        plane = rr.in_frame(p, fh, fw, win)
        want = rr.region_plane(plane, win, 0.5)
        assert np.all(want[:, 0, 0] == 0) and np.all(want[:, h - 1, w - 1] == 1) and np.all(want[:, h // 2, w // 2] == 0)
        got = ops.highlight_region("plane", win, plane=dev(plane), tau=0.5)
        assert np.array_equal(got.cpu().numpy(), want), win
        got = ops.highlight_region("plane", win, plane=dev(plane[..., None]), tau=0.5)          # [B,Hp,Wp,1], as SpecSeg hands it over
        assert np.array_equal(got.cpu().numpy(), want), win


# ------------------------------------------------------------------------------------------------- the metrics
def _run(g, win, t, region):
    out = ops.image_metrics_region(dev(g), win, dev(t), _u8(region))
    assert out.dtype == torch.float64 and tuple(out.shape) == (g.shape[0], 12)
    return host(out)


@pytest.mark.parametrize("h,w", rr.SIZES)
def test_region_metrics_match_the_restatement(h, w):
    g, t, smap = rr.pair(h, w)
    win = (0, 0, h, w)
    for B in rr.BATCHES:
        for name in rr.REGIONS:
            r = rr.make_region(name, B, h, w, seed=h)
            got = _run(g[:B], win, t[:B], r)
            ref = rr.region_metrics(g[:B], t[:B], r, smap[:B])
            print(h, w, B, name, "worst |got - ref|:", np.nanmax(np.abs(np.where(np.isfinite(ref), got - ref, 0.0)), axis=0)[:10])
            assert not rr.mismatches(got, ref), (B, name, rr.mismatches(got, ref))


@pytest.mark.parametrize("fh,fw,win", rr.FRAMES)
def test_region_metrics_on_offset_windows(fh, fw, win):
    """The window off the frame's origin, NaN and 1e30 everywhere else in the frame: nothing outside the window is read."""
    h, w = win[2:]
    g, t, smap = rr.pair(h, w)
    frame = rr.in_frame(g, fh, fw, win)
    assert not np.isfinite(frame).all()
    for B in rr.BATCHES:
        for name in rr.REGIONS:
            r = rr.make_region(name, B, h, w, seed=h)
            got = _run(frame[:B], win, t[:B], r)
            ref = rr.region_metrics(g[:B], t[:B], r, smap[:B])
            assert not rr.mismatches(got, ref), (B, name, rr.mismatches(got, ref))
            # the same numbers as on the tight frame, bit for bit
            assert np.array_equal(got, _run(g[:B], (0, 0, h, w), t[:B], r), equal_nan=True), (B, name)


def test_nan_and_inf_sit_where_the_reference_has_them():
    h = w = 37
    g, t, _ = rr.pair(h, w)
    r = rr.make_region("left", 3, h, w)
    t2 = np.array(t)
    t2[r != 0] = g[r != 0]                                  # identical inside: mse_in 0, psnr_in +inf
    got, ref = _run(g, (0, 0, h, w), t2, r), rr.region_metrics(g, t2, r)
    # identical colours: the reference's dE inside is 0 (dE94: 1e-7 of float64 cancellation), which no relative bound can hold; they get
    # the absolute 1e-5 that tests/test_metrics_gpu.py gives identical pairs, everything else the table's tolerances
    bad = [m for m in rr.mismatches(got, ref) if m[1] not in ("in_de76", "in_de94")]
    assert np.all(ref[:, 1] == np.inf) and np.all(got[:, 0] == 0.0) and not bad, bad
    assert np.all(np.abs(got[:, 3:5]) <= 1e-5) and np.all(np.abs(ref[:, 3:5]) <= 1e-5), (got[:, 3:5], ref[:, 3:5])
    # a NaN and an Inf pixel of the prediction outside the region stay out of the sums inside it (a select, not a product)
    g2 = np.array(g)
    g2[:, 3, w - 2], g2[:, 9, w - 3] = np.nan, np.inf
    a, b = _run(g2, (0, 0, h, w), t, r), _run(g, (0, 0, h, w), t, r)
    assert np.array_equal(a[:, [0, 1, 3, 4, 10, 11]], b[:, [0, 1, 3, 4, 10, 11]])


@pytest.mark.parametrize("h,w", [(11, 11), (26, 27), (64, 64), (520, 520)])
def test_full_and_empty_regions_equal_the_whole_window_metrics(h, w):
    g, t, _ = rr.pair(h, w)
    for fh, fw, win in ((h, w, (0, 0, h, w)), (h + 16, w + 7, (9, 2, h, w))):
        frame = rr.in_frame(g, fh, fw, win)
        whole = host(ops.image_metrics_hw(dev(frame), win, dev(t)))
        full = _run(frame, win, t, rr.make_region("full", 3, h, w))
        empty = _run(frame, win, t, rr.make_region("empty", 3, h, w))
        assert np.array_equal(full[:, 0:5], whole) and np.isnan(full[:, 5:10]).all()
        assert np.array_equal(empty[:, 5:10], whole) and np.isnan(empty[:, 0:5]).all()
        assert np.all(full[:, 10] == h * w) and np.all(full[:, 11] == (h - 10) * (w - 10)) and np.all(empty[:, 10:] == 0)
        # any non-zero byte is inside
        assert np.array_equal(_run(frame, win, t, 255 * rr.make_region("full", 3, h, w))[:, :5], whole)
    if h == w:
        assert np.array_equal(host(ops.image_metrics(dev(g), dev(t))), whole)


@pytest.mark.parametrize("h,w", [(12, 11), (40, 13), (37, 37), (64, 64), (520, 520)])
def test_decomposition_identities(h, w):
    g, t, _ = rr.pair(h, w)
    win = (0, 0, h, w)
    whole = host(ops.image_metrics_hw(dev(g), win, dev(t)))
    npix, npos = h * w, (h - 10) * (w - 10)
    for name in rr.REGIONS:
        m = _run(g, win, t, rr.make_region(name, 3, h, w, seed=h))
        z = np.nan_to_num(m, nan=0.0)
        n_in, p_in = m[:, 10], m[:, 11]
        for j, rel in ((0, 1e-5), (3, 1e-4), (4, 1e-4)):
            got = (n_in * z[:, j] + (npix - n_in) * z[:, 5 + j]) / npix
            assert np.all(np.abs(got - whole[:, j]) <= rel * np.abs(whole[:, j])), (name, j, got, whole[:, j])
        got = (p_in * z[:, 2] + (npos - p_in) * z[:, 7]) / npos
        assert np.all(np.abs(got - whole[:, 2]) <= 5e-5), (name, got, whole[:, 2])


def test_bitwise_reproducible_and_batch_invariant():
    h, w = 64, 64
    g, t, _ = rr.pair(h, w)
    win = (0, 0, h, w)
    r = rr.make_region("bernoulli", 3, h, w, seed=1)
    a = _run(g, win, t, r)
    assert np.array_equal(a, _run(g, win, t, r), equal_nan=True)
    for i in range(3):
        assert np.array_equal(_run(g[i:i + 1], win, t[i:i + 1], r[i:i + 1])[0], a[i]), i
    # the same image among other neighbours
    g2, t2, _ = rr.pair(64, 64)
    g2, t2, r2 = np.array(g2[::-1]), np.array(t2[::-1]), np.array(rr.make_region("checker", 3, h, w))
    g2[1], t2[1], r2[1] = g[0], t[0], r[0]
    assert np.array_equal(_run(g2, win, t2, r2)[1], a[0])
    # the builder too
    fh, fw, fwin = rr.FRAMES[0]
    src, target, tau, _ = rr.residual_case(3, fh, fw, fwin, TAU)
    one = ops.highlight_region("residual", fwin, src=dev(src[1:2]), target=dev(target[1:2]), tau=tau)
    assert torch.equal(one[0], ops.highlight_region("residual", fwin, src=dev(src), target=dev(target), tau=tau)[1])


def test_refusals_leave_the_output_untouched():
    L = _lib.lib()
    x = torch.zeros((2, 32, 40, 3), device="cuda")
    reg = torch.ones((2, 32, 40), dtype=torch.uint8, device="cuda")
    out = torch.full((2, 12), 7.0, dtype=torch.float64, device="cuda")
    need = L.shm_image_metrics_region_hw_workspace(2, 32, 40)
    ws = torch.zeros(need, dtype=torch.uint8, device="cuda")
    P = lambda t: t.data_ptr()
    calls = [((P(x), 32, 40, 0, 0, P(x), 32, 40, P(reg), P(out), P(ws), need - 1, 2, None), -3),
             ((P(x), 32, 40, 0, 0, P(x), 10, 40, P(reg), P(out), P(ws), need, 2, None), -1),
             ((P(x), 32, 40, 1, 0, P(x), 32, 40, P(reg), P(out), P(ws), need, 2, None), -1),
             ((P(x), 32, 40, 0, 0, P(x), 32, 40, P(reg), P(out), P(ws), need, 0, None), -1),
             ((P(x), 32, 40, 0, 0, P(x), 32, 40, None, P(out), P(ws), need, 2, None), -1)]
    for args, code in calls:
        assert L.shm_image_metrics_region_hw(*args) == code, args
    rout = torch.full((2, 32, 40), 7, dtype=torch.uint8, device="cuda")
    for args in ((5, P(x), P(x), None, 32, 40, 0, 0, 32, 40, 0.5, P(rout), 2, None),
                 (0, P(x), None, None, 32, 40, 0, 0, 32, 40, 0.5, P(rout), 2, None),
                 (1, None, None, None, 32, 40, 0, 0, 32, 40, 0.5, P(rout), 2, None),
                 (0, P(x), P(x), None, 32, 40, 0, 0, 32, 40, 0.5, P(rout), 0, None),
                 (0, P(x), P(x), None, 32, 40, 0, 9, 32, 32, 0.5, P(rout), 2, None),
                 (0, P(x), P(x), None, 32, 40, 0, 0, 0, 40, 0.5, P(rout), 2, None)):
        assert L.shm_highlight_region_hw(*args) == -1, args
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((rout == 7).all())
    # the Python surface: dtypes, shapes, contiguity
    with pytest.raises(_lib.ShmError, match="< 11"):
        ops.image_metrics_region(torch.zeros((1, 10, 16, 3), device="cuda"), (0, 0, 10, 16), torch.zeros((1, 10, 16, 3), device="cuda"),
                                 torch.zeros((1, 10, 16), dtype=torch.uint8, device="cuda"))
    with pytest.raises(TypeError, match="uint8"):
        ops.image_metrics_region(x, (0, 0, 32, 40), x, reg.float())
    with pytest.raises(ValueError, match="region"):
        ops.image_metrics_region(x, (0, 0, 32, 40), x, reg[:, :31])
    with pytest.raises(ValueError, match="contiguous"):
        ops.image_metrics_region(x, (0, 0, 32, 20), x[:, :, ::2], reg[:, :, ::2].contiguous())
    with pytest.raises(ValueError, match="mode"):
        ops.highlight_region("mask", (0, 0, 32, 40), plane=x[..., 0].contiguous(), tau=0.5)
    with pytest.raises(ValueError, match="residual"):
        ops.highlight_region("residual", (0, 0, 32, 40), src=x, tau=0.5)
    with pytest.raises(TypeError, match="float32"):
        ops.highlight_region("plane", (0, 0, 32, 40), plane=x[..., 0].double().contiguous(), tau=0.5)
    with pytest.raises(ValueError, match="out must be"):
        ops.highlight_region("plane", (0, 0, 32, 40), plane=x[..., 0].contiguous(), tau=0.5, out=reg.float())


# ------------------------------------------------------------------------------------------------- end to end
S_E2E, F_E2E = 32, 16
NAMES10 = rr.NAMES[:10]


def _blob_pair(rng, hw):
    """A diffuse image and the photo of it: the same pixels plus a bright blob (additive, clipped at 255)."""
    dif = rng.integers(0, 160, (hw[0], hw[1], 3)).astype(np.uint8)
    photo = dif.astype(np.int32)
    y0, x0 = int(rng.integers(4, hw[0] - 20)), int(rng.integers(4, hw[1] - 20))
    photo[y0:y0 + 14, x0:x0 + 16] += 90
    return np.clip(photo, 0, 255).astype(np.uint8), dif


def _write_images(tmp_path, n=4, hw=(40, 48)):
    from PIL import Image
    rng = np.random.default_rng(3)
    for sub in ("test", "diffuse"):
        (tmp_path / sub).mkdir()
    for i in range(n):
        photo, dif = _blob_pair(rng, hw)
        Image.fromarray(photo).save(tmp_path / "test" / f"img{i:02d}.png")
        Image.fromarray(dif).save(tmp_path / "diffuse" / f"img{i:02d}.png")


def _trainer(tmp_path, tag, **kw):
    from shmgan_amd import ShmGANwithSSpecSeg
    return ShmGANwithSSpecSeg(image_size=S_E2E, filter_size=F_E2E, batch_size=1, checkpoint_save_dir=str(tmp_path / "ckpt"),
                              log_dir=str(tmp_path / f"logs_{tag}"), result_dir=str(tmp_path / f"results_{tag}"), **kw)


def _targs(tmp_path, **kw):
    return SimpleNamespace(test_dir=str(tmp_path / "test"), diffuse_dir=str(tmp_path / "diffuse"), calc_metrics=True, **kw)


def _check_report(r, tmp_path, tag, rows, sizes, stems):
    """The "region" entry, the printed table's file twin and the means, against the rows [n,12] computed by hand."""
    from shmgan_amd.telemetry import region_means
    reg = r["region"]
    assert set(reg) == {*NAMES10, "fraction", "means", "n_in_images", "n_out_images"}
    for j, k in enumerate(NAMES10):
        assert np.array_equal(np.array(reg[k]), rows[:, j], equal_nan=True), k
    assert reg["fraction"] == [float(row[10]) / n for row, (n, _) in zip(rows, sizes)]
    means, n_in, n_out = region_means(rows, [n for n, _ in sizes], [p for _, p in sizes])
    assert (reg["n_in_images"], reg["n_out_images"]) == (n_in, n_out) and set(reg["means"]) == set(NAMES10)
    for k in NAMES10:
        assert reg["means"][k] == means[k] or (np.isnan(means[k]) and np.isnan(reg["means"][k])), k
    lines = [json.loads(ln) for ln in (tmp_path / f"results_{tag}" / ev.REGION_FILE).read_text().splitlines()]
    assert [ln["image"] for ln in lines] == stems and all(set(ln) == {"image", "fraction", *NAMES10} for ln in lines)
    for i, ln in enumerate(lines):
        assert ln["fraction"] == reg["fraction"][i]
        for k in NAMES10:
            assert ln[k] == (None if np.isnan(reg[k][i]) else reg[k][i]), (i, k)


def test_test_mode_with_the_residual_region(tmp_path, monkeypatch):
    from shmgan_amd.data import EvalDataset
    _write_images(tmp_path)
    monkeypatch.setattr(ev, "time", SimpleNamespace(perf_counter=lambda: 0.0))          # "Time" is 0 in every run: the tables compare
    m = _trainer(tmp_path, "res").build()
    printed = []
    with pytest.warns(UserWarning, match="no checkpoint"):
        r = ev.test(m, _targs(tmp_path, eval_batch_size=2, metrics_region="residual"), print_fn=printed.append)
    assert m.eval_region is None                                                          # the option is test()'s, not left on the trainer
    assert all(h in "\n".join(printed) for h in ev.REGION_HEADERS + ev.TABLE_HEADERS)
    # by hand: the loader's batches through evaluate with eval_region set, and the float64 restatement on what it produced
    ds = EvalDataset(tmp_path / "test", S_E2E, 2, tmp_path / "diffuse")
    m.eval_region = ("residual", TAU)
    rows = []
    for bi in range(len(ds)):
        rgb, dif = ds.batch(bi)
        gen, _, met = m.evaluate(rgb, dif)
        assert m.highlight_region.dtype == torch.uint8 and tuple(m.highlight_region.shape) == (2, S_E2E, S_E2E)
        assert tuple(m.region_metrics.shape) == (2, 12) and m.region_metrics.dtype == torch.float64
        region = m.highlight_region.cpu().numpy()
        assert np.array_equal(region, rr.region_residual(host(rgb).astype(np.float32), (0, 0, S_E2E, S_E2E), host(dif).astype(np.float32), TAU))
        got = host(m.region_metrics)
        assert not rr.mismatches(got, rr.region_metrics(host(gen), host(dif), region)), bi
        assert np.array_equal(host(met), host(ops.image_metrics(gen, dif)))                 # the return value is what it was
        rows.append(got)
    m.eval_region = None
    rows = np.concatenate(rows)
    assert np.all(rows[:, 10] > 0) and np.all(rows[:, 10] < S_E2E * S_E2E) and np.isfinite(rows).all()      # the blob: both sets, every image
    _check_report(r, tmp_path, "res", rows, [(S_E2E * S_E2E, (S_E2E - 10) ** 2)] * 4, [f"img{i:02d}" for i in range(4)])
    assert r["region"]["n_in_images"] == r["region"]["n_out_images"] == 4
    # another threshold is another region; the option needs calc_metrics and a known source
    m2 = _trainer(tmp_path, "res2").build()
    with pytest.warns(UserWarning, match="no checkpoint"):
        r2 = ev.test(m2, _targs(tmp_path, eval_batch_size=2, metrics_region="residual", region_threshold=0.5), print_fn=lambda *a: None)
    assert r2["MSE"] == r["MSE"] and r2["region"]["fraction"] != r["region"]["fraction"]
    with pytest.raises(ValueError, match="metrics_region"):
        ev.test(m2, SimpleNamespace(test_dir=str(tmp_path / "test"), calc_metrics=False, metrics_region="residual"))
    with pytest.raises(ValueError, match="metrics_region"):
        ev.test(m2, _targs(tmp_path, metrics_region="mask"))

    # off: what a run that never heard of the options returns, prints and writes
    outs = {}
    for tag, extra in (("never", {}), ("off", dict(metrics_region="off", region_threshold=0.3))):
        mt = _trainer(tmp_path, tag).build()
        lines = []
        alloc = None
        with pytest.warns(UserWarning, match="no checkpoint"):
            res = ev.test(mt, _targs(tmp_path, eval_batch_size=2, **extra), print_fn=lines.append)
        assert "region" not in res and mt.highlight_region is None and mt.region_metrics is None and mt._inf_photo is None
        assert not [k for k in mt.arena.t if isinstance(k[0], str) and "region" in k[0]]
        files = {p.name: p.read_bytes() for p in sorted((tmp_path / f"results_{tag}").iterdir())}
        outs[tag] = (res, lines, files)
    assert outs["never"] == outs["off"] and sorted(outs["off"][2]) == ["MSE.txt", "PSNR.txt", "SSIM.txt"]
    assert {k: v for k, v in r.items() if k != "region"} == outs["never"][0]                # and the rest of the dict with the option on
    assert printed[:len(outs["never"][1])] == outs["never"][1]


def test_test_mode_with_the_specseg_region_at_native_size(tmp_path):
    from shmgan_amd.data import NativeEvalDataset
    _write_images(tmp_path, n=3, hw=(40, 50))                   # padded to 48 x 64: the window is off the frame's origin
    m = _trainer(tmp_path, "seg").build()
    ds = NativeEvalDataset(tmp_path / "test", tmp_path / "diffuse", m.device)
    # an untrained SpecSeg has no meaningful level: take the median of its first mask, so that both sets exist
    rgb, dif, window = ds.batch(0)
    m.infer(rgb, cyclic=False)
    top, left, h, w = window
    assert (top, left) != (0, 0) and (h, w) == (40, 50)
    tau = float(m.specular_candidate[0, top:top + h, left:left + w, 0].median())
    m.eval_region = ("specseg", tau)
    rows = []
    for i in range(ds.n):
        rgb, dif, window = ds.batch(i)
        gen, _, met = m.evaluate_frame(rgb, dif, window, cyclic=False)
        region = m.highlight_region.cpu().numpy()
        assert region.shape == (1, h, w)
        assert np.array_equal(region, rr.region_plane(host(m.specular_candidate)[..., 0], window, tau))
        got = host(m.region_metrics)
        assert not rr.mismatches(got, rr.region_metrics(rr.crop(host(gen), window), host(dif), region)), i
        assert np.array_equal(host(met), host(ops.image_metrics_hw(gen, window, dif)))
        rows.append(got)
    m.eval_region = None
    rows = np.concatenate(rows)
    assert 0 < rows[0, 10] < h * w
    with pytest.warns(UserWarning, match="no checkpoint"):
        r = ev.test(m, _targs(tmp_path, eval_batch_size=1, eval_size="native", metrics_region="specseg", region_threshold=tau),
                    print_fn=lambda *a: None)
    _check_report(r, tmp_path, "seg", rows, [(h * w, (h - 10) * (w - 10))] * 3, [f"img{i:02d}" for i in range(3)])


# ------------------------------------------------------------------------------------------------- validation
def _write_captures(root, n, rng, hw=(40, 50)):
    from PIL import Image
    from shmgan_amd.data import PSD_SUBDIRS
    for sub in PSD_SUBDIRS:
        (root / sub).mkdir(parents=True)
    for i in range(n):
        photo, dif = _blob_pair(rng, hw)
        for sub in PSD_SUBDIRS:
            Image.fromarray(dif if sub == "ED" else photo).save(root / sub / f"img_{i:03d}.png")


def _vargs(tmp_path, tag, **kw):
    base = dict(mode="train", image_size=S_E2E, batch_size=1, filter_size=F_E2E, num_epochs=2, g_lr=2e-5, d_lr=2e-5, beta1=0.5, beta2=0.99,
                data_dir=str(tmp_path / "data"), checkpoint_save_dir=str(tmp_path / f"ckpt_{tag}"), log_dir=str(tmp_path / f"logs_{tag}"),
                result_dir=str(tmp_path / f"results_{tag}"), log_step=1, checkpoint_save_step=1, val_dir=str(tmp_path / "val"))
    base.update(kw)
    return argparse.Namespace(**base)


def _train(args):
    from shmgan_amd import ShmGANwithSSpecSeg
    m = ShmGANwithSSpecSeg(args)
    m.train(args, print_fn=lambda *a: None)
    torch.cuda.synchronize()
    return m


def _state(m):
    return [t.detach().cpu().numpy().view(np.uint32).copy() for P in (m.G.P, m.D.P) for t in (P.flat, P.m, P.v)]


def test_validation_with_a_region_and_its_monitor(tmp_path):
    from shmgan_amd.telemetry import improves, read_validation
    _write_captures(tmp_path / "data", 4, np.random.default_rng(1))
    _write_captures(tmp_path / "val", 3, np.random.default_rng(2))
    on = _train(_vargs(tmp_path, "on", val_region="residual", val_monitor="in_psnr"))
    off = _train(_vargs(tmp_path, "off"))
    # training is bitwise what it is without the option, and the lines without it are the lines they were
    assert all(np.array_equal(a, b) for a, b in zip(_state(on), _state(off)))
    rows_off = read_validation(str(tmp_path / "logs_off"))
    metrics = ("mse", "psnr", "ssim", "de76", "de94")
    assert all(set(r) == {"step", "epoch", "weights", "n", "held_out", *metrics, "best"} for r in rows_off)
    rows = read_validation(str(tmp_path / "logs_on"))
    assert [(r["step"], r["weights"]) for r in rows] == [(3, "raw"), (6, "raw")] == [(r["step"], r["weights"]) for r in rows_off]
    assert all(set(r) == {"step", "epoch", "weights", "n", "held_out", *metrics, *NAMES10, "n_in_images", "best"} for r in rows)
    assert [{k: r[k] for k in metrics} for r in rows] == [{k: r[k] for k in metrics} for r in rows_off]
    # the last line is validate() on the final weights; its rows are the restatement's, its means region_means'
    hand = on.validate()
    raw = hand["raw"]
    assert set(raw) == {*metrics, "rows", *NAMES10, "region_rows", "n_in_images", "n_out_images"}
    assert raw["region_rows"].shape == (3, 12) and raw["n_in_images"] == raw["n_out_images"] == 3 == rows[-1]["n_in_images"]
    assert [rows[-1][k] for k in metrics + NAMES10] == [raw[k] for k in metrics + NAMES10]
    for j, k in enumerate(NAMES10):
        assert raw[k] == float(raw["region_rows"][:, j].mean()), k
    plain = on.validate(region=None)
    assert set(plain["raw"]) == {*metrics, "rows"} and np.array_equal(plain["raw"]["rows"], raw["rows"])
    for i, batch in enumerate(on.valDataset):
        gen, _ = on.infer(batch[0], cyclic=False)
        region = rr.region_residual(host(batch[0]).astype(np.float32), (0, 0, S_E2E, S_E2E), host(batch[4]).astype(np.float32), TAU)
        assert 0 < region.sum() < S_E2E * S_E2E
        assert not rr.mismatches(raw["region_rows"][i:i + 1], rr.region_metrics(host(gen), host(batch[4]), region)), i
    # best.npz follows in_psnr by telemetry.improves
    best, flags = None, []
    for r in rows:
        flags.append(improves("in_psnr", r["in_psnr"], best))
        best = r["in_psnr"] if flags[-1] else best
    assert [r["best"] for r in rows] == flags and flags[0]
    want = [r for r in rows if r["best"]][-1]
    with np.load(str(tmp_path / "ckpt_on" / "best.npz")) as z:
        state = json.loads(str(z["trainer/state"]))
        assert state["best"] == {"monitor": "in_psnr", "weights": "raw", "value": want["in_psnr"], "step": want["step"]}
        assert int(z["G/iterations"]) == want["step"]
    # a region monitor without a region is refused before anything runs
    from shmgan_amd import ShmGANwithSSpecSeg
    bad = _vargs(tmp_path, "bad", val_monitor="out_mse")
    with pytest.raises(ValueError, match="val_region"):
        ShmGANwithSSpecSeg(bad).train(bad, print_fn=lambda *a: None)
    assert not (tmp_path / "ckpt_bad").exists()
