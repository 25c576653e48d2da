"""Held-out validation inside train(): validate() against evaluate() by hand, that validating (and averaging) leaves the training
trajectory bitwise alone, validation.jsonl, best.npz across pruning and resume, val_fraction, and test mode on the best file's
averaged weights.  Tiny PNG captures (40 x 50 files, S = 32, F = 16) as in tests/test_train_loop_gpu.py."""
import argparse
import json
from types import SimpleNamespace

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

S, F = 32, 16
METRICS = ("mse", "psnr", "ssim", "de76", "de94")


def _write_dataset(root, n, rng, hw=(40, 50)):
    from PIL import Image
    from shmgan_amd.data import PSD_SUBDIRS
    for sub in PSD_SUBDIRS:
        (root / sub).mkdir(parents=True)
        for i in range(n):
            Image.fromarray(rng.integers(0, 256, (hw[0], hw[1], 3)).astype(np.uint8)).save(root / sub / f"img_{i:03d}.png")
    return root


def _args(tmp_path, tag, **kw):
    base = dict(mode="train", image_size=S, batch_size=1, filter_size=F, num_epochs=2, g_lr=2e-5, d_lr=2e-5, beta1=0.5, beta2=0.99,
                data_dir=str(tmp_path / "data"), checkpoint_save_dir=str(tmp_path / f"ckpt_{tag}"), log_dir=str(tmp_path / f"logs_{tag}"),
                result_dir=str(tmp_path / f"results_{tag}"), log_step=1, checkpoint_save_step=1)
    base.update(kw)
    return argparse.Namespace(**base)


def _train(args, **kw):
    from shmgan_amd import ShmGANwithSSpecSeg
    m = ShmGANwithSSpecSeg(args)
    n = m.train(args, print_fn=lambda *a: None, **kw)
    torch.cuda.synchronize()
    return m, n


def _bits(t):
    return t.detach().cpu().numpy().view(np.uint32).copy()


def _state(m):
    return [_bits(t) for P in (m.G.P, m.D.P) for t in (P.flat, P.m, P.v)]


@pytest.fixture()
def captures(tmp_path):
    _write_dataset(tmp_path / "data", 4, np.random.default_rng(1))
    _write_dataset(tmp_path / "val", 3, np.random.default_rng(2))
    return tmp_path


def test_validate_scores_what_evaluate_scores(captures):
    from shmgan_amd import ShmGANwithSSpecSeg
    from shmgan_amd.data import validation_loader
    tmp_path = captures
    res = {}
    for Bv in (1, 2):
        m = ShmGANwithSSpecSeg(image_size=S, filter_size=F, batch_size=1, data_dir=str(tmp_path / "data"), val_dir=str(tmp_path / "val"),
                               val_batch_size=Bv).build()
        draws = (m._rng.bit_generator.state, m._draw_count)
        r = res[Bv] = m.validate()
        assert (r["n"], r["held_out"]) == ((3, 3) if Bv == 1 else (2, 3)) and set(r) == {"n", "held_out", "raw"}
        assert r["raw"]["rows"].shape == (r["n"], 5) and r["raw"]["rows"].dtype == np.float64
        assert (m._rng.bit_generator.state, m._draw_count) == draws and m._prefetched is None
        # by hand, on the same loader batches
        ds = validation_loader(str(tmp_path / "data"), S, 1, val_dir=str(tmp_path / "val"), val_batch_size=Bv, device=m.device)
        hand = []
        for batch in ds:
            _, _, met = m.evaluate(batch[0], batch[4])
            hand.append(met.cpu().numpy())
        hand = np.concatenate(hand)
        assert np.array_equal(r["raw"]["rows"], hand)
        for j, k in enumerate(METRICS):
            assert r["raw"][k] == float(hand[:, j].astype(np.float64).mean())
        assert np.isfinite(hand).all()
    # B = 1 against B = 2: the bound test mode's own batch-1-against-batch-2 check states (tests/test_metrics_gpu.py: the generator's
    # InstanceNorm sums are float64 atomics and its tile choice follows the batch, the metrics kernels are batch invariant)
    a, b = res[1]["raw"]["rows"][:2], res[2]["raw"]["rows"]
    assert np.all(np.abs(a - b) <= 1e-4 * np.abs(b) + 1e-7), (a, b)
    with pytest.raises(ValueError, match="no held-out set"):
        ShmGANwithSSpecSeg(image_size=S, filter_size=F, batch_size=1).build().validate()


def test_validation_and_average_change_nothing(captures):
    """Two epochs of train() (look-ahead active, as the loop runs by default) with val_dir and ema_decay on, and with both off: the
    weights and Adam moments of both models are bitwise equal, and so are the draw streams."""
    tmp_path = captures
    on, n_on = _train(_args(tmp_path, "on", val_dir=str(tmp_path / "val"), ema_decay=0.9))
    off, n_off = _train(_args(tmp_path, "off"))
    assert n_on == n_off == 6
    assert all(np.array_equal(a, b) for a, b in zip(_state(on), _state(off)))
    assert on._rng.bit_generator.state == off._rng.bit_generator.state and on._draw_count == off._draw_count
    assert (tmp_path / "logs_on" / "validation.jsonl").exists() and not (tmp_path / "logs_off" / "validation.jsonl").exists()
    assert not (tmp_path / "ckpt_off" / "best.npz").exists()
    with np.load(str(tmp_path / "ckpt_off" / "ckpt-3.npz")) as z:          # with the options off: the keys and the state a file always had
        assert not [k for k in z.files if k.startswith("G/ema")]
        assert set(json.loads(str(z["trainer/state"]))) == {"attention", "epoch", "draw_count", "rng", "batch_step"}


def _expected_best_flags(rows, monitor, weights):
    from shmgan_amd.telemetry import improves
    best, flags = None, []
    for r in rows:
        hit = r["weights"] == weights and improves(monitor, r[monitor], best)
        if hit:
            best = r[monitor]
        flags.append(hit)
    return flags


def _best_row(rows, monitor, weights):
    """The row best.npz must hold: the first one to reach the best monitored value."""
    from shmgan_amd.telemetry import VAL_MONITORS
    mon = [r for r in rows if r["weights"] == weights]
    top = max(VAL_MONITORS[monitor] * r[monitor] for r in mon)
    return next(r for r in mon if VAL_MONITORS[monitor] * r[monitor] == top)


def _best_state(path):
    with np.load(str(path)) as z:
        return json.loads(str(z["trainer/state"])), int(z["G/iterations"])


def test_validation_log_and_best_checkpoint(captures):
    from shmgan_amd import ShmGANwithSSpecSeg
    from shmgan_amd.telemetry import read_validation
    tmp_path = captures
    common = dict(val_dir=str(tmp_path / "val"), ema_decay=0.9, val_monitor="psnr")
    # one epoch, then the same run for two: the rows of step 3 are the first run's, whose weights can still be scored by hand
    one, _ = _train(_args(tmp_path, "one", num_epochs=1, **common))
    rows1 = read_validation(str(tmp_path / "logs_one"))
    assert [(r["step"], r["epoch"], r["weights"]) for r in rows1] == [(3, 0, "raw"), (3, 0, "ema")]          # the end of the run is not scored twice
    hand = one.validate(weights=("raw", "ema"))
    for r in rows1:
        assert (r["n"], r["held_out"]) == (3, 3) and [r[k] for k in METRICS] == [hand[r["weights"]][k] for k in METRICS]
    two, _ = _train(_args(tmp_path, "two", num_epochs=2, **common))
    rows2 = read_validation(str(tmp_path / "logs_two"))
    assert [(r["step"], r["epoch"], r["weights"]) for r in rows2] == [(3, 0, "raw"), (3, 0, "ema"), (6, 1, "raw"), (6, 1, "ema")]
    assert set(rows2[0]) == {"step", "epoch", "weights", "n", "held_out", *METRICS, "best"}
    assert [{k: r[k] for k in METRICS} for r in rows2[:2]] == [{k: r[k] for k in METRICS} for r in rows1]
    hand = two.validate(weights=("raw", "ema"))
    for r in rows2[2:]:
        assert [r[k] for k in METRICS] == [hand[r["weights"]][k] for k in METRICS]
    assert rows2[0]["psnr"] != rows2[1]["psnr"] and rows2[1]["psnr"] != rows2[3]["psnr"]                  # two weight sets, two moments
    assert [r["best"] for r in rows2] == _expected_best_flags(rows2, "psnr", "ema") and rows2[1]["best"] and not rows2[0]["best"]
    state, iters = _best_state(tmp_path / "ckpt_two" / "best.npz")
    want = _best_row(rows2, "psnr", "ema")
    assert state["best"] == {"monitor": "psnr", "weights": "ema", "value": want["psnr"], "step": want["step"]} and iters == want["step"]

    # a run long enough to prune: best.npz survives, _restore_latest never picks it, a resumed run appends and keeps the better file
    args = _args(tmp_path, "long", num_epochs=4, val_monitor="mse", val_dir=str(tmp_path / "val"), ema_decay=0.9)
    _train(args)
    ck = tmp_path / "ckpt_long"
    assert sorted(p.name for p in ck.iterdir()) == ["best.npz", "ckpt-3.npz", "ckpt-4.npz", "ckpt-5.npz"]
    rows = read_validation(str(tmp_path / "logs_long"))
    assert [r["step"] for r in rows] == [3, 3, 6, 6, 9, 9, 12, 12]
    state, iters = _best_state(ck / "best.npz")
    want = _best_row(rows, "mse", "ema")
    assert (state["best"]["step"], state["best"]["value"], iters) == (want["step"], want["mse"], want["step"])
    fresh = ShmGANwithSSpecSeg(args)
    assert fresh._restore_latest().endswith("ckpt-5.npz")
    (tmp_path / "only_best").mkdir()
    (tmp_path / "only_best" / "best.npz").write_bytes((ck / "best.npz").read_bytes())
    assert ShmGANwithSSpecSeg(_args(tmp_path, "x", checkpoint_save_dir=str(tmp_path / "only_best")))._restore_latest() is None
    args.num_epochs = 2
    resumed, _ = _train(args)
    assert resumed.G.P.iterations == 18
    rows = read_validation(str(tmp_path / "logs_long"))
    assert [r["step"] for r in rows] == [3, 3, 6, 6, 9, 9, 12, 12, 15, 15, 18, 18]
    assert [r["best"] for r in rows] == _expected_best_flags(rows, "mse", "ema")
    state, iters = _best_state(ck / "best.npz")
    want = _best_row(rows, "mse", "ema")
    assert (state["best"]["step"], state["best"]["value"], iters) == (want["step"], want["mse"], want["step"])
    assert "best.npz" in [p.name for p in ck.iterdir()] and len(list(ck.glob("ckpt-*.npz"))) == 3


def test_val_fraction_holds_files_out(tmp_path, monkeypatch):
    from shmgan_amd.data import PolarDataset, split_indices
    _write_dataset(tmp_path / "data", 8, np.random.default_rng(4))
    decoded = []
    real = PolarDataset._decode
    monkeypatch.setattr(PolarDataset, "_decode", lambda self, path, key: (decoded.append((id(self), path)), real(self, path, key))[1])
    m, n = _train(_args(tmp_path, "frac", val_fraction=0.25, val_seed=5, shuffle=True, data_seed=2))
    train, val = m.loadedDataset, m.valDataset
    whole = PolarDataset(str(tmp_path / "data"), S, 1, device=m.device, rank=0, world=1)
    tr, va = split_indices(whole.files[0], 0.25, 5)
    for v in range(5):
        assert train.files[v] == [whole.files[v][i] for i in tr] and val.files[v] == [whole.files[v][i] for i in va]
    assert (train.n, val.n, m.length_dataset, n) == (6, 2, 6, 2 * 5)
    by_train = {p for who, p in decoded if who == id(train)}
    by_val = {p for who, p in decoded if who == id(val)}
    held_out = {f for v in range(5) for f in val.files[v]}
    assert by_train and by_train <= {f for v in range(5) for f in train.files[v]} and not by_train & held_out and by_val == held_out
    from shmgan_amd.telemetry import read_validation
    rows = read_validation(str(tmp_path / "logs_frac"))
    assert [(r["step"], r["weights"], r["n"], r["held_out"]) for r in rows] == [(5, "raw", 2, 2), (10, "raw", 2, 2)]


def test_test_mode_on_the_best_average(captures):
    """eval_checkpoint="best" + eval_weights="ema": the metrics of validate() on that file's average.  Test mode's loader does not
    flip the photos (test.py maps only x / 255) while the training and held-out loaders do, so the comparison is with validate() on a
    held-out loader of the same files built with flip_ud=False."""
    from shmgan_amd import ShmGANwithSSpecSeg, evaluate as ev
    from shmgan_amd.data import PolarDataset
    tmp_path = captures
    args = _args(tmp_path, "t", val_dir=str(tmp_path / "val"), ema_decay=0.9)
    _train(args)
    targs = SimpleNamespace(test_dir=str(tmp_path / "val" / "I0"), diffuse_dir=str(tmp_path / "val" / "ED"), calc_metrics=True, eval_batch_size=1,
                            eval_weights="ema", eval_checkpoint="best")
    t = ShmGANwithSSpecSeg(_args(tmp_path, "t", mode="test"))
    r = ev.test(t, targs, print_fn=lambda *a: None)
    ref = ShmGANwithSSpecSeg(_args(tmp_path, "t", ema_decay=0.9)).build()
    ref.load_npz(str(tmp_path / "ckpt_t" / "best.npz"))
    ds = PolarDataset(str(tmp_path / "val"), S, 1, flip_ud=False, device=ref.device, rank=0, world=1)
    v = ref.validate(dataset=ds, weights=("raw", "ema"))
    for j, key in enumerate(ev.METRIC_KEYS):
        assert r[key] == [float(x) for x in v["ema"]["rows"][:, j]], key
        assert r[key] != [float(x) for x in v["raw"]["rows"][:, j]], key
    assert torch.equal(t.G.P.flat, ref.G.P.flat)                                   # the raw weights are back after the run
    # the raw weights of the same file, by path
    targs.eval_weights, targs.eval_checkpoint = "raw", str(tmp_path / "ckpt_t" / "best.npz")
    r = ev.test(ShmGANwithSSpecSeg(_args(tmp_path, "t", mode="test")), targs, print_fn=lambda *a: None)
    assert r["MSE"] == [float(x) for x in v["raw"]["rows"][:, 0]]
    # both refusals, by name, before any image is processed
    off = _args(tmp_path, "plain", num_epochs=1)
    _train(off)
    for weights, ckpt, exc, what in (("ema", "latest", ValueError, "eval_weights"), ("raw", "best", FileNotFoundError, "eval_checkpoint"),
                                     ("raw", str(tmp_path / "nowhere.npz"), FileNotFoundError, "eval_checkpoint")):
        targs.eval_weights, targs.eval_checkpoint = weights, ckpt
        targs.save_images, targs.image_dir = "g1", str(tmp_path / "never")
        with pytest.raises(exc, match=what):
            ev.test(ShmGANwithSSpecSeg(_args(tmp_path, "plain", mode="test")), targs, print_fn=lambda *a: None)
        assert not (tmp_path / "never").exists()
