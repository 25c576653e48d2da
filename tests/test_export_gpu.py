"""Test-mode image export on the GPU: ops.export_u8 (shm_export_u8) against the float64 restatement (tests/export_ref.py), its
determinism and batch invariance, ops.running_scale_mean, and shmgan_amd.evaluate.test(save_images=...) end to end against the
oracle's inference path (the reference's test.py:218-317)."""
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from oracle import step_torch as st
from shmgan_amd import ops
from shmgan_amd import evaluate as ev

import export_ref as xr
from util import dev, host

pytestmark = pytest.mark.gpu


def _check_bytes(got, want_bytes, y, what):
    """Exact wherever the float64 value is more than 1e-3 from a half-integer, else within 1."""
    got = np.asarray(got).astype(np.int64)
    want = want_bytes.astype(np.int64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    d = np.abs(got - want)
    far = ~xr.near_half(y)
    assert np.all(d[far] == 0), (what, int((d[far] != 0).sum()), np.argwhere((d != 0) & far)[:5])
    assert np.all(d <= 1), (what, int(d.max()))


def _unpack(out, offs, sizes, chans):
    o = out.cpu().numpy()
    return [o[off:off + h * w * c].reshape(h, w, c) for off, (h, w), c in zip(offs, sizes, chans)]


def _jobs(rng):
    """A ragged job list: S in {32, 64}, targets (S,S), (40,48), (300,451), (17,23), C in {1,3}, one plane with ld > C, all
    three modes.  Returns (device planes, host planes, sizes, modes, mul)."""
    mul_h = np.array([0.8, 1.3, 0.55], np.float32)
    spec = [(32, (32, 32), 3, 3, "rescale"), (64, (40, 48), 3, 3, ("scale", 1)), (32, (300, 451), 1, 1, "clip"),
            (64, (17, 23), 3, 3, "rescale"), (64, (64, 64), 1, 1, ("scale", 2)), (32, (40, 48), 3, 4, "clip"),
            (32, (17, 23), 1, 1, "rescale"), (64, (300, 451), 3, 3, "rescale"), (32, (32, 32), 3, 3, ("scale", 0)),
            (64, (40, 48), 1, 1, "clip")]
    planes_d, planes_h, sizes, modes = [], [], [], []
    for S, size, C, ld, mode in spec:
        x = rng.uniform(-0.4, 1.4, (S, S, ld)).astype(np.float32)
        t = dev(x)[..., :C] if ld > C else dev(x)
        planes_d.append(t)
        planes_h.append(x[..., :C])
        sizes.append(size)
        modes.append(mode)
    return planes_d, planes_h, sizes, modes, mul_h


def _want(planes_h, sizes, modes, mul_h):
    out = []
    for x, (h, w), m in zip(planes_h, sizes, modes):
        if isinstance(m, tuple):
            out.append(xr.export(x, h, w, "scale", float(mul_h[m[1]])))
        else:
            out.append(xr.export(x, h, w, m))
    return out


def test_kernel_matches_the_restatement():
    rng = np.random.default_rng(21)
    planes_d, planes_h, sizes, modes, mul_h = _jobs(rng)
    assert planes_d[5].stride(1) == 4                                     # the ld > C job
    out, offs = ops.export_u8(planes_d, sizes, modes, dev(mul_h))
    got = _unpack(out, offs, sizes, [p.shape[2] for p in planes_d])
    for j, ((b, y), g) in enumerate(zip(_want(planes_h, sizes, modes, mul_h), got)):
        _check_bytes(g, b, y, (j, sizes[j], modes[j]))


def test_constant_plane_and_round_trip():
    rng = np.random.default_rng(5)
    S = 48
    src = rng.integers(0, 256, (S, S, 3), dtype=np.uint8)
    f = torch.empty((S, S, 3), dtype=torch.float32, device="cuda")
    ops.resize_bilinear_u8(torch.from_numpy(src).cuda(), f, 1.0 / 255.0, False)
    one = torch.ones(1, dtype=torch.float32, device="cuda")
    const = torch.full((S, S, 1), 0.3, device="cuda")
    out, offs = ops.export_u8([f, const], [(S, S), (20, 30)], [("scale", 0), "rescale"], one)
    back, flat = _unpack(out, offs, [(S, S), (20, 30)], [3, 1])
    assert np.array_equal(back, src)
    assert not flat.any()                                                 # divide_no_nan: a constant plane is 0


def test_deterministic_and_batch_invariant():
    rng = np.random.default_rng(8)
    planes_d, _, sizes, modes, mul_h = _jobs(rng)
    mul = dev(mul_h)
    chans = [p.shape[2] for p in planes_d]
    full, offs = ops.export_u8(planes_d, sizes, modes, mul)
    ref = _unpack(full, offs, sizes, chans)
    again, _ = ops.export_u8(planes_d, sizes, modes, mul)       # (the alignment padding between jobs is never written)
    for g, r in zip(_unpack(again, offs, sizes, chans), ref):
        assert np.array_equal(g, r)
    for j in (0, 3, 7):
        alone, o1 = ops.export_u8([planes_d[j]], [sizes[j]], [modes[j]], mul)
        assert np.array_equal(_unpack(alone, o1, [sizes[j]], [chans[j]])[0], ref[j]), j
    perm = list(rng.permutation(len(planes_d)))
    sh, o2 = ops.export_u8([planes_d[i] for i in perm], [sizes[i] for i in perm], [modes[i] for i in perm], mul)
    got = _unpack(sh, o2, [sizes[i] for i in perm], [chans[i] for i in perm])
    for g, i in zip(got, perm):
        assert np.array_equal(g, ref[i]), i


def test_running_scale_mean_over_batches():
    rng = np.random.default_rng(2)
    scales = rng.uniform(0.05, 0.4, 5).astype(np.float32)
    acc = torch.zeros(2, dtype=torch.float64, device="cuda")
    got = []
    for lo, hi in ((0, 2), (2, 4), (4, 5)):
        mul = torch.empty(hi - lo, dtype=torch.float32, device="cuda")
        ops.running_scale_mean(dev(scales[lo:hi]), acc, mul)
        got.extend(host(mul).tolist())
    want = np.cumsum(scales.astype(np.float64)) / np.arange(1, 6)
    assert np.all(np.abs(np.array(got) - want) <= 1e-6 * want), (got, want)
    assert host(acc)[1] == 5.0 and abs(host(acc)[0] - scales.astype(np.float64).sum()) <= 1e-12


# ------------------------------------------------------------------------------------------------- end to end
S_E2E, F_E2E = 32, 16
SIZES = [(40, 48), (37, 29), (64, 64), (50, 33), (31, 70)]


def _write_images(tmp_path):
    from PIL import Image
    rng = np.random.default_rng(4)
    for sub in ("test", "diffuse"):
        d = tmp_path / sub
        d.mkdir()
        for i, (h, w) in enumerate(SIZES):
            Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)).save(d / f"img{i:02d}.png")
    return tmp_path / "test", tmp_path / "diffuse"


def _trainer(tmp_path, tag, F=F_E2E, **kw):
    from shmgan_amd import ShmGANwithSSpecSeg
    return ShmGANwithSSpecSeg(image_size=S_E2E, filter_size=F, batch_size=1, checkpoint_save_dir=str(tmp_path / "ckpt"),
                              log_dir=str(tmp_path / f"logs_{tag}"), result_dir=str(tmp_path / f"results_{tag}"), **kw)


def _args(tmp_path, **kw):
    return SimpleNamespace(test_dir=str(tmp_path / "test"), diffuse_dir=str(tmp_path / "diffuse"), calc_metrics=True,
                           eval_batch_size=2, **kw)


def _png(path):
    from PIL import Image
    with Image.open(path) as im:
        return np.array(im)


def _close(got, want, what):
    d = np.abs(got.astype(np.int64) - want.astype(np.int64))
    assert d.max() <= 1, (what, int(d.max()))
    assert (d == 0).mean() >= 0.99, (what, float((d == 0).mean()))


def test_test_mode_writes_the_images(tmp_path):
    from shmgan_amd.data import EvalDataset
    test_dir, _ = _write_images(tmp_path)
    src = _trainer(tmp_path, "src").build(seed=7, beta_seed=8)
    (tmp_path / "ckpt").mkdir()
    src.save_npz(str(tmp_path / "ckpt" / "ckpt-1.npz"))
    gw = src.G.get_weights()
    gb = [b.detach().cpu().numpy() for b in src.G.betas]

    m = _trainer(tmp_path, "a").build()
    r_off = ev.test(m, _args(tmp_path))
    assert r_off["files"] == [] and not (tmp_path / "results_a" / "images").exists()
    r = ev.test(m, _args(tmp_path, save_images="all"))
    img_dir = tmp_path / "results_a" / "images"
    names = sorted(os.listdir(img_dir))
    assert len(names) == 8 * len(SIZES) and len(r["files"]) == len(names)
    assert r["files"][:8] == [str(img_dir / ev.image_name("img00", t)) for t in ev.IMAGE_TAGS]
    for i, (h, w) in enumerate(SIZES):
        for tag in ev.IMAGE_TAGS:
            a = _png(img_dir / ev.image_name(f"img{i:02d}", tag))
            assert a.shape == ((h, w) if tag in ("G1_Y", "mask") else (h, w, 3)), (i, tag, a.shape)
    for key in ev.METRIC_KEYS:                                           # the export changes no metric
        assert r[key] == r_off[key], key
    assert r["index"] == r_off["index"]

    # the oracle: its inference path on the loader's resized images, then the float64 restatement of the export
    ds = EvalDataset(test_dir, S_E2E, len(SIZES))
    rgb, _ = ds.batch(0)
    ref = st.infer(gw, gb, host(rgb), F_E2E)
    gen = ref["gen_rgb"].numpy()
    for i, (h, w) in enumerate(SIZES):
        want, _ = xr.export(gen[i], h, w, "rescale")
        _close(_png(img_dir / ev.image_name(f"img{i:02d}", "G1")), want, ("G1", i))

    # image_values="output": gen_rgb times the running mean of the standardisation scales (gen_rgb_output / 255), S x S
    out_dir = tmp_path / "out_model"
    r2 = ev.test(m, _args(tmp_path, save_images="g1", image_values="output", image_out_size="model", image_dir=str(out_dir)))
    assert sorted(os.listdir(out_dir)) == [ev.image_name(f"img{i:02d}", "G1") for i in range(len(SIZES))]
    assert len(r2["files"]) == len(SIZES)
    scales = np.asarray(ref["scale"], np.float64).reshape(-1)
    running = np.cumsum(scales) / np.arange(1, len(SIZES) + 1)
    for i in range(len(SIZES)):
        want, _ = xr.export(gen[i], S_E2E, S_E2E, "scale", running[i])
        _close(_png(out_dir / ev.image_name(f"img{i:02d}", "G1")), want, ("output", i))


def test_bf16_trainer_writes_images(tmp_path):
    _write_images(tmp_path)
    m = _trainer(tmp_path, "bf16", F=32, compute_dtype="bfloat16").build()
    with pytest.warns(UserWarning, match="no checkpoint"):
        r = ev.test(m, _args(tmp_path, save_images="all"))
    assert len(r["files"]) == 8 * len(SIZES)
    for f in r["files"]:
        a = _png(f)
        assert a.max() > a.min(), f
