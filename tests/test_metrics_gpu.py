"""Test mode on the GPU: ops.image_metrics (shm_image_metrics) against the float64 restatement (tests/metrics_ref.py, SSIM from
oracle.tf_ops_np), its reproducibility and batch invariance, and shmgan_amd.evaluate.test end to end against the oracle's
inference path (the reference's test.py:40-392)."""
import pickle
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from oracle import step_torch as st
from shmgan_amd import _lib, ops
from shmgan_amd import evaluate as ev

from metrics_ref import image_metrics as ref_metrics
from util import dev, host

pytestmark = pytest.mark.gpu


def _pair(rng, B, S):
    g = rng.uniform(-0.3, 1.3, (B, S, S, 3))
    t = rng.uniform(-0.3, 1.3, (B, S, S, 3))
    return g.astype(np.float32), t.astype(np.float32)


def _check(got, ref):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert np.all(np.abs(got[:, 0] - ref[:, 0]) <= 1e-5 * np.abs(ref[:, 0])), (got[:, 0], ref[:, 0])
    assert np.all(np.abs(got[:, 1] - ref[:, 1]) <= 1e-4), (got[:, 1], ref[:, 1])
    assert np.all(np.abs(got[:, 2] - ref[:, 2]) <= 5e-5), (got[:, 2], ref[:, 2])
    for k in (3, 4):
        assert np.all(np.abs(got[:, k] - ref[:, k]) <= 1e-4 * np.abs(ref[:, k])), (k, got[:, k], ref[:, k])


@pytest.mark.parametrize("S", [11, 16, 37, 64])
@pytest.mark.parametrize("B", [1, 3])
def test_image_metrics_match_the_restatement(S, B):
    rng = np.random.default_rng(1000 + 10 * S + B)
    g, t = _pair(rng, B, S)
    out = ops.image_metrics(dev(g), dev(t))
    assert out.dtype == torch.float64 and tuple(out.shape) == (B, 5)
    _check(host(out), ref_metrics(g, t))


def test_identical_constant_and_near_identical_pairs():
    rng = np.random.default_rng(7)
    S = 37
    g, _ = _pair(rng, 2, S)
    same = host(ops.image_metrics(dev(g), dev(g)))
    assert np.all(same[:, 0] == 0.0) and np.all(same[:, 1] == np.inf)
    assert np.all(np.abs(same[:, 2] - 1.0) <= 1e-6)
    assert np.all(np.abs(same[:, 3:]) <= 1e-5)
    # a constant target: rescale_01 divides by a zero range (divide_no_nan -> 0)
    t = np.full_like(g, 0.5)
    got = host(ops.image_metrics(dev(g), dev(t)))
    assert np.isfinite(got).all()
    _check(got, ref_metrics(g, t))
    # near-identical colours: dH^2 of dE94 cancels; both dE within 1e-3 absolute
    t = (g + rng.normal(0.0, 1e-3, g.shape)).astype(np.float32)
    got, ref = host(ops.image_metrics(dev(g), dev(t))), ref_metrics(g, t)
    assert np.all(np.abs(got[:, 3:] - ref[:, 3:]) <= 1e-3), (got[:, 3:], ref[:, 3:])
    _check(got, ref)


def test_bitwise_reproducible_and_batch_invariant():
    rng = np.random.default_rng(11)
    S = 64
    g, t = _pair(rng, 3, S)
    a = host(ops.image_metrics(dev(g), dev(t)))
    b = host(ops.image_metrics(dev(g), dev(t)))
    assert np.array_equal(a, b)
    for i in range(3):
        one = host(ops.image_metrics(dev(g[i:i + 1]), dev(t[i:i + 1])))
        assert np.array_equal(one[0], a[i]), i
    # the same image among other neighbours
    g2, t2 = _pair(rng, 3, S)
    g2[1], t2[1] = g[0], t[0]
    assert np.array_equal(host(ops.image_metrics(dev(g2), dev(t2)))[1], a[0])


def test_error_codes_before_any_launch():
    L = _lib.lib()
    x = torch.zeros((1, 10, 10, 3), device="cuda")
    out = torch.zeros((1, 5), dtype=torch.float64, device="cuda")
    with pytest.raises(_lib.ShmError, match="< 11"):
        ops.image_metrics(x, x)
    y = torch.zeros((2, 32, 32, 3), device="cuda")
    out2 = torch.zeros((2, 5), dtype=torch.float64, device="cuda")
    need = L.shm_image_metrics_workspace(2, 32)
    ws = torch.zeros(need, dtype=torch.uint8, device="cuda")
    rc = L.shm_image_metrics(y.data_ptr(), y.data_ptr(), out2.data_ptr(), ws.data_ptr(), need - 1, 2, 32, None)
    assert rc == -3 and b"workspace" in L.shm_last_error()
    rc = L.shm_image_metrics(x.data_ptr(), x.data_ptr(), out.data_ptr(), ws.data_ptr(), need, 1, 10, None)
    assert rc == -1
    rc = L.shm_image_metrics(y.data_ptr(), y.data_ptr(), out2.data_ptr(), ws.data_ptr(), need, 0, 32, None)
    assert rc == -1
    torch.cuda.synchronize()
    assert float(out2.abs().sum()) == 0.0


# ------------------------------------------------------------------------------------------------- end to end
S_E2E, F_E2E = 32, 16        # the smallest filter count the float32 generator takes (a multiple of 16; bfloat16: 32)


def _write_images(tmp_path, n=5):
    from PIL import Image
    rng = np.random.default_rng(3)
    for sub in ("test", "diffuse"):
        d = tmp_path / sub
        d.mkdir()
        for i in range(n):
            Image.fromarray(rng.integers(0, 256, (40, 48, 3), dtype=np.uint8)).save(d / f"img{i:02d}.png")
    return tmp_path / "test", tmp_path / "diffuse"


def _args(tmp_path, calc, batch, diffuse_dir):
    return SimpleNamespace(test_dir=str(tmp_path / "test"), diffuse_dir=str(diffuse_dir) if diffuse_dir else "",
                           calc_metrics=calc, eval_batch_size=batch)


def _trainer(tmp_path, tag, F=F_E2E, **kw):
    from shmgan_amd import ShmGANwithSSpecSeg
    return ShmGANwithSSpecSeg(image_size=S_E2E, filter_size=F, batch_size=1, checkpoint_save_dir=str(tmp_path / "ckpt"),
                              log_dir=str(tmp_path / f"logs_{tag}"), result_dir=str(tmp_path / f"results_{tag}"), **kw)


def test_test_mode_end_to_end(tmp_path, capsys):
    from shmgan_amd.data import EvalDataset
    test_dir, diffuse_dir = _write_images(tmp_path)
    # a checkpoint of weights other than the ones a fresh trainer starts from
    src = _trainer(tmp_path, "src").build(seed=7, beta_seed=8)
    (tmp_path / "ckpt").mkdir()
    src.save_npz(str(tmp_path / "ckpt" / "ckpt-1.npz"))
    gw = src.G.get_weights()
    gb = [b.detach().cpu().numpy() for b in src.G.betas]

    m2 = _trainer(tmp_path, "b2").build()
    r2 = ev.test(m2, _args(tmp_path, True, 2, diffuse_dir))
    assert torch.equal(m2.G.P.flat, src.G.P.flat)                      # restored
    assert r2["images"] == 5 and r2["index"] == [1, 2, 3, 4, 5] and len(r2["time"]) == 5
    out = capsys.readouterr().out
    for h in ev.TABLE_HEADERS + ev.MEAN_HEADERS:
        assert h in out
    for name, key in (("SSIM.txt", "SSIM"), ("MSE.txt", "MSE"), ("PSNR.txt", "PSNR")):
        with open(tmp_path / "results_b2" / name, "rb") as f:
            assert pickle.load(f) == r2[key]
    for fn in ("Generator_summary.txt", "Discriminator_summary.txt", "SpecSeg_summary.txt"):
        assert (tmp_path / "logs_b2" / fn).stat().st_size > 0

    # the oracle: its inference path on the loader's resized images, then the float64 restatement
    ds = EvalDataset(test_dir, S_E2E, 5, diffuse_dir)
    rgb, dif = ds.batch(0)
    rgb, dif = host(rgb), host(dif)
    ref = st.infer(gw, gb, rgb, F_E2E)
    want = ref_metrics(ref["gen_rgb"].numpy(), dif)
    for j, key in enumerate(ev.METRIC_KEYS):
        got = np.array(r2[key])
        if key == "SSIM":
            assert np.all(np.abs(got - want[:, j]) <= 1e-3), (key, got, want[:, j])
        else:
            assert np.all(np.abs(got - want[:, j]) <= 1e-3 * np.abs(want[:, j])), (key, got, want[:, j])
        assert abs(r2["means"][key] - got.mean()) <= 1e-12 * max(1.0, abs(got.mean()))

    # batch 1 against batch 2 (the tail batch of 2 is partial)
    m1 = _trainer(tmp_path, "b1").build()
    r1 = ev.test(m1, _args(tmp_path, True, 1, diffuse_dir))
    for key in ev.METRIC_KEYS:
        a, b = np.array(r1[key]), np.array(r2[key])
        assert np.all(np.abs(a - b) <= 1e-4 * np.abs(b) + 1e-7), (key, a, b)

    # without metrics: no diffuse directory needed, no metrics returned
    r0 = ev.test(m1, _args(tmp_path, False, 2, None))
    assert r0["means"] is None and "MSE" not in r0 and r0["index"] == [1, 2, 3, 4, 5]


def test_bf16_trainer_metrics(tmp_path):
    from shmgan_amd.data import EvalDataset
    test_dir, diffuse_dir = _write_images(tmp_path)
    m = _trainer(tmp_path, "bf16", F=32, compute_dtype="bfloat16").build()
    with pytest.warns(UserWarning, match="no checkpoint"):
        r = ev.test(m, _args(tmp_path, True, 2, diffuse_dir))
    assert r["images"] == 5
    for key in ev.METRIC_KEYS:
        assert len(r[key]) == 5 and np.isfinite(np.array(r[key])).all(), (key, r[key])
    ds = EvalDataset(test_dir, S_E2E, 2, diffuse_dir)
    rgb, dif = ds.batch(0)
    gen, cyc, met = m.evaluate(rgb, dif)
    own = ops.image_metrics(gen.clone(), dif)
    assert torch.equal(met, own)
    assert np.isfinite(host(met)).all()
