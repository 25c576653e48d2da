"""The checkpoint file and its handling, on the CPU: the keys and types save_npz writes, the bitwise round trip in both attention
modes, "nothing is touched before the whole file has been checked", the numbered files with their pruning, the restore with its
damaged-file fallback, and the best held-out value a resumed run has to beat.  No test launches a kernel: the models, their
optimizer state and SpecSeg allocate on any torch device, and a checkpoint only copies them."""
import json
import os

import numpy as np
import pytest
import torch

from shmgan_amd import ShmGANwithSSpecSeg, checkpoint

STATE_KEYS = {"attention", "epoch", "draw_count", "rng", "batch_step"}


# ---- the three places where a test reaches below the trainer's public surface
def _listing(m):
    return checkpoint.checkpoints(m.checkpoint_save_dir)


def _to_beat(ckdir, record, monitor, weights):
    return checkpoint.best_to_beat(record, os.path.join(str(ckdir), checkpoint.BEST_CHECKPOINT), monitor, weights)


def _break_reader(m, error):
    def boom(path):
        raise error
    m._read_npz = boom


# ---- trainers
def _trainer(monkeypatch, tmp_path, seed=42, **kw):
    monkeypatch.setenv("SHM_NO_WGRAD_LANE", "1")
    kw.setdefault("checkpoint_save_dir", str(tmp_path))
    return ShmGANwithSSpecSeg(device="cpu", image_size=32, filter_size=16, batch_size=1, **kw).build(seed=seed)


def _perturb(m, seed=1):
    """State no freshly built trainer has: random Adam moments, betas and SpecSeg variables, counters and an advanced draw stream."""
    g = torch.Generator().manual_seed(seed)
    for P in (m.G.P, m.D.P):
        P.m.copy_(torch.randn(P.n, generator=g))
        P.v.copy_(torch.rand(P.n, generator=g))
    for b in m.G.betas + m.D.betas:
        b.copy_(torch.randn(b.shape, generator=g))
    m.SpecSeg.flat.add_(torch.randn(m.SpecSeg.n, generator=g))
    m.G.P.iterations, m.D.P.iterations = 7, 9
    m.epoch, m._draw_count = 3, 5
    m._rng.random(4)
    return m


def _bits(t):
    return t.detach().cpu().numpy().view(np.uint32).copy()


def _snapshot(m):
    """(buffers as bit patterns, everything else a checkpoint restores)."""
    bufs = [_bits(t) for P in (m.G.P, m.D.P) for t in (P.flat, P.m, P.v)] + [_bits(b) for b in m.G.betas + m.D.betas] + [_bits(m.SpecSeg.flat)]
    return bufs, (m.G.P.iterations, m.D.P.iterations, m.epoch, m._draw_count, m._rng.bit_generator.state)


def _same(a, b):
    return len(a[0]) == len(b[0]) and all(np.array_equal(x, y) for x, y in zip(a[0], b[0])) and a[1] == b[1]


def _keys(m):
    """The key set of a save_npz file from the model sizes: per model its variables, betas, Adam moments and counter, SpecSeg's
    variables, and the trainer state."""
    keys = {"trainer/state"}
    for name, M in (("G", m.G), ("D", m.D)):
        keys |= {f"{name}/var{i:02d}" for i in range(len(M.P.vars))} | {f"{name}/beta{i:02d}" for i in range(len(M.betas))}
        keys |= {f"{name}/adam_m", f"{name}/adam_v", f"{name}/iterations"}
    return keys | {f"SpecSeg/var{i:02d}" for i in range(len(m.SpecSeg.vars))}


def _rewrite(src, dst, **changes):
    with np.load(src) as z:
        d = {k: z[k] for k in z.files}
    d.update(changes)
    np.savez(dst, **d)
    return d


# ---- 1. keys and types
def test_keys_and_types(monkeypatch, tmp_path):
    m = _trainer(monkeypatch, tmp_path)
    p = str(tmp_path / "a.npz")
    m.save_npz(p)
    with np.load(p) as z:
        assert set(z.files) == _keys(m)
        for name, M in (("G", m.G), ("D", m.D)):
            assert z[f"{name}/iterations"].dtype == np.int64 and z[f"{name}/iterations"].shape == ()
            for k in ("adam_m", "adam_v"):
                assert z[f"{name}/{k}"].dtype == np.float32 and z[f"{name}/{k}"].shape == (M.P.n,)
            for i, w in enumerate(M.get_weights()):                  # Keras variable order and layouts
                assert z[f"{name}/var{i:02d}"].dtype == np.float32 and np.array_equal(z[f"{name}/var{i:02d}"], w)
        assert set(json.loads(str(z["trainer/state"]))) == STATE_KEYS
    # with the average on: exactly two more keys.  The average is there already, so that _ensure_ema has nothing to launch
    e = _trainer(monkeypatch, tmp_path, ema_decay=0.999)
    e.G.P.ema = e.G.P.flat.clone()
    e.save_npz(p)
    with np.load(p) as z:
        assert set(z.files) == _keys(e) | {"G/ema", "G/ema_updates"}
        assert z["G/ema"].shape == (e.G.P.n,) and z["G/ema"].dtype == np.float32 and z["G/ema_updates"].dtype == np.int64
        assert set(json.loads(str(z["trainer/state"]))) == STATE_KEYS


# ---- 2. and 5. the round trip
@pytest.mark.parametrize("attention", ["executed", "live"])
def test_round_trip(monkeypatch, tmp_path, attention):
    a = _perturb(_trainer(monkeypatch, tmp_path, attention=attention))
    b = _trainer(monkeypatch, tmp_path, seed=7, attention=attention)
    assert not _same(_snapshot(a), _snapshot(b))
    p = str(tmp_path / "a.npz")
    a.save_npz(p)
    b.load_npz(p)
    assert _same(_snapshot(a), _snapshot(b))
    assert (b.G.P.iterations, b.D.P.iterations, b.epoch, b._draw_count) == (7, 9, 3, 5)
    assert b.G.weights_dirty and b.D.weights_dirty


# ---- 3. nothing is touched before the whole file has been checked
def test_a_mismatching_file_touches_nothing(monkeypatch, tmp_path):
    a = _perturb(_trainer(monkeypatch, tmp_path))
    b = _trainer(monkeypatch, tmp_path, seed=7)
    p, bad = str(tmp_path / "a.npz"), str(tmp_path / "bad.npz")
    a.save_npz(p)
    with np.load(p) as z:
        v = z["D/var03"]
    _rewrite(p, bad, **{"D/var03": v.reshape(-1)})
    before = _snapshot(b)
    with pytest.raises(KeyError, match="D/var03"):
        b.load_npz(bad)
    assert _same(_snapshot(b), before)


# ---- 4. attention mode
def test_a_file_of_the_other_attention_mode_is_refused(monkeypatch, tmp_path):
    a = _perturb(_trainer(monkeypatch, tmp_path))
    p = str(tmp_path / "a.npz")
    a.save_npz(p)
    live = _trainer(monkeypatch, tmp_path, attention="live")
    before = _snapshot(live)
    with pytest.raises(KeyError, match="attention"):
        live.load_npz(p)
    assert _same(_snapshot(live), before)


# ---- 6. numbered files
def test_numbered_checkpoints_keep_the_newest_three(monkeypatch, tmp_path):
    m = _trainer(monkeypatch, tmp_path)
    paths = [m._save_checkpoint() for _ in range(5)]
    assert [os.path.basename(p) for p in paths] == [f"ckpt-{n}.npz" for n in range(1, 6)]
    assert sorted(os.listdir(tmp_path)) == ["ckpt-3.npz", "ckpt-4.npz", "ckpt-5.npz"]


def test_listing_is_numeric_and_holds_numbered_files_only(monkeypatch, tmp_path):
    for fn in ("ckpt-2.npz", "ckpt-10.npz", "best.npz", "ckpt-3.npz.tmp"):
        (tmp_path / fn).write_bytes(b"")
    m = ShmGANwithSSpecSeg(device="cpu", image_size=32, filter_size=16, batch_size=1, checkpoint_save_dir=str(tmp_path))
    assert _listing(m) == [str(tmp_path / "ckpt-2.npz"), str(tmp_path / "ckpt-10.npz")]


# ---- 7. restore
def test_restore_falls_back_from_a_damaged_file(monkeypatch, tmp_path):
    a = _perturb(_trainer(monkeypatch, tmp_path))
    p1 = a._save_checkpoint()
    first = _snapshot(a)
    p2 = _perturb(a, seed=2)._save_checkpoint()
    assert not _same(_snapshot(a), first)
    with open(p2, "r+b") as f:
        f.truncate(1000)
    b = _trainer(monkeypatch, tmp_path, seed=7)
    assert b._restore_latest() == p1
    assert _same(_snapshot(b), first)


def test_restore_without_a_numbered_file_changes_nothing(monkeypatch, tmp_path):
    b = _trainer(monkeypatch, tmp_path, seed=7)
    before = _snapshot(b)
    assert b._restore_latest() is None
    _perturb(_trainer(monkeypatch, tmp_path)).save_npz(str(tmp_path / "best.npz"))
    assert b._restore_latest() is None
    assert _same(_snapshot(b), before)


def test_restore_does_not_take_an_io_error_for_a_damaged_file(monkeypatch, tmp_path):
    a = _trainer(monkeypatch, tmp_path)
    a._save_checkpoint()
    a._save_checkpoint()
    before = _snapshot(a)
    _break_reader(a, OSError(5, "Input/output error"))
    with pytest.raises(OSError, match="Input/output"):
        a._restore_latest()
    assert _same(_snapshot(a), before)


# ---- 8. the best value a resumed run has to beat
def _record(value, monitor="psnr", weights="raw", step=10):
    return {"monitor": monitor, "weights": weights, "value": value, "step": step}


def _write_best(ckdir, record):
    state = {"attention": "executed"} if record is None else {"attention": "executed", "best": record}
    np.savez(os.path.join(str(ckdir), "best.npz"), **{"trainer/state": np.array(json.dumps(state))})


def test_best_value_on_resume(tmp_path):
    assert _to_beat(tmp_path, None, "psnr", "raw") is None                          # no file, no record
    assert _to_beat(tmp_path, _record(30.0), "psnr", "raw") == _record(30.0)       # no file
    _write_best(tmp_path, None)                                                     # a file written without validation
    assert _to_beat(tmp_path, None, "psnr", "raw") is None
    _write_best(tmp_path, _record(31.0, step=12))
    assert _to_beat(tmp_path, None, "psnr", "raw") == _record(31.0, step=12)
    assert _to_beat(tmp_path, _record(30.0), "psnr", "raw") == _record(31.0, step=12)      # the file is the newer and better one
    assert _to_beat(tmp_path, _record(32.0), "psnr", "raw") == _record(32.0)
    # "better" is telemetry.improves for the monitor: mse is minimised
    _write_best(tmp_path, _record(0.2, "mse"))
    assert _to_beat(tmp_path, _record(0.1, "mse"), "mse", "raw") == _record(0.1, "mse")
    assert _to_beat(tmp_path, _record(0.3, "mse"), "mse", "raw") == _record(0.2, "mse")
    # a record for another monitor or another weight set does not count
    assert _to_beat(tmp_path, _record(40.0), "mse", "raw") == _record(0.2, "mse")
    assert _to_beat(tmp_path, _record(0.01, "mse", "ema"), "mse", "raw") == _record(0.2, "mse")
    assert _to_beat(tmp_path, _record(0.01, "mse", "ema"), "mse", "ema") == _record(0.01, "mse", "ema")
    assert _to_beat(tmp_path, _record(40.0), "ssim", "raw") is None
