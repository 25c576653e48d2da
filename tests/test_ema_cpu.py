"""The averaged generator weights and the held-out validation without a device: the float64 restatement (tests/ema_ref.py) against
the closed form, the decay schedule, every refusal of shm_ema_update (made on the host, before any launch), option validation, the
split of a capture and the held-out loader."""
import ctypes as C
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest

import ema_ref as er
from shmgan_amd import _lib


# ---------------------------------------------------------------------------------------------------------------- the restatement
def test_restatement_equals_the_closed_form():
    rng = np.random.default_rng(0)
    for decays in ((0.5,) * 6, (0.1, 0.5, 0.999, 0.9999, 0.9), [er.decay_at(0.9, t) for t in range(12)]):
        ema0 = er.values(rng, 64)
        ws = [er.values(rng, 64) for _ in decays]
        ema = ema0.astype(np.float64)
        for w, d in zip(ws, decays):
            ema = er.update(ema, w, d)
        ref = er.closed_form(ema0, ws, decays)
        big = max(float(np.abs(ema0).max()), max(float(np.abs(w).max()) for w in ws))
        assert np.all(np.abs(ema - ref) <= 64 * 2.0 ** -52 * big)          # both float64: a few of ITS roundings per step
    # decay 0 is the copy, and the weights of the closed form sum to one (a constant input is a fixed point)
    w = er.values(rng, 16)
    assert np.array_equal(er.update(er.values(rng, 16), w, 0.0), w.astype(np.float64))
    c = np.full(8, 3.0, np.float32)
    assert np.allclose(er.closed_form(c, [c] * 5, [0.9] * 5), 3.0, rtol=0, atol=1e-14)


def test_restatement_is_fed_the_fp32_om():
    assert er.om32(0.999) == np.float32(1) - np.float32(0.999) and float(er.om32(0.999)) != 1.0 - 0.999
    assert er.om32(0.5) == np.float32(0.5) and er.om32(0.0) == np.float32(1)
    # the bound: 4 u M, elementwise, K-fold over K updates
    assert np.array_equal(er.bound([1.0, -8.0], [2.0, 4.0], 3), 3 * 4 * er.U * np.array([2.0, 8.0]))


def test_warmup_schedule():
    from shmgan_amd import ops
    assert er.decay_at(0.999, 0) == 0.1 == ops.ema_decay_at(0.999, 0)
    assert ops.ema_decay_at(0.999, 0, warmup=False) == 0.999 == er.decay_at(0.999, 0, False)
    for d in (0.9, 0.99, 0.999):
        reach = next(t for t in range(100000) if (1.0 + t) / (10.0 + t) >= d)
        assert reach == {0.9: 80, 0.99: 890, 0.999: 8990}[d]
        assert ops.ema_decay_at(d, reach - 1) < d and ops.ema_decay_at(d, reach) == d == ops.ema_decay_at(d, 10 * reach)
        assert all(ops.ema_decay_at(d, t) == er.decay_at(d, t) for t in (0, 1, 7, reach - 1, reach, reach + 1))
    for bad in (-0.1, 1.0, 1.5, float("nan")):
        with pytest.raises(ValueError, match="ema_decay"):
            ops.ema_decay_at(bad, 0)


# ---------------------------------------------------------------------------------------------------------------- the entry point
def test_ema_update_is_in_the_header_table():
    I, P, Z, F = C.c_int, C.c_void_p, C.c_size_t, C.c_float
    assert _lib.SIGNATURES["shm_ema_update"] == (I, [P, P, Z, F, P, P])
    assert _lib.CONSTANTS["SHM_EMA_MAX_BLOCKS"] >= 256 and "ema.hip" in _lib.SOURCES
    from shmgan_amd import ops
    assert ops.EMA_MAX_BLOCKS == _lib.CONSTANTS["SHM_EMA_MAX_BLOCKS"]


def test_ema_update_refusals_without_gpu():
    """Every refusal is made on the host before any launch, so it can be provoked here with pointers nobody dereferences."""
    L = _lib.lib()
    E = _lib.CONSTANTS["SHM_E_SHAPE"]
    a, b = 0x1000, 0x2000
    for decay in (float("nan"), -0.5, -1e-30, 1.0, 1.5, float("inf")):
        assert L.shm_ema_update(a, b, 4, decay, None, None) == E and b"decay" in L.shm_last_error(), decay
    assert L.shm_ema_update(a, b, 0, 1.0, None, None) == E and b"decay" in L.shm_last_error()         # also with nothing to do
    assert L.shm_ema_update(None, b, 4, 0.5, None, None) == E and b"ema is a null" in L.shm_last_error()
    assert L.shm_ema_update(a, None, 4, 0.5, None, None) == E and b"w is a null" in L.shm_last_error()
    # overlap: w inside ema, ema inside w, the same buffer, and by one element at either end; touching ranges are fine (below)
    for e, w, n in ((a, a + 8, 4), (a + 8, a, 4), (a, a, 1), (a, a + 12, 4), (a + 12, a, 4)):
        assert L.shm_ema_update(e, w, n, 0.5, None, None) == E and b"overlap" in L.shm_last_error(), (e, w, n)
    assert L.shm_ema_update(a + 2, b, 4, 0.5, None, None) == E and b"aligned" in L.shm_last_error()
    # n == 0: SHM_OK without a launch, whatever the pointers
    assert L.shm_ema_update(None, None, 0, 0.5, None, None) == 0 and L.shm_ema_update(a, a, 0, 0.0, None, None) == 0
    import torch
    if not torch.cuda.is_available():
        # ranges that only touch pass every check and reach the launch, which is what fails here: SHM_E_HIP, not SHM_E_SHAPE
        assert L.shm_ema_update(a, a + 16, 4, 0.5, None, None) == _lib.CONSTANTS["SHM_E_HIP"]


# ---------------------------------------------------------------------------------------------------------------- options
def test_validation_options():
    from shmgan_amd.telemetry import VAL_MONITORS, improves, validation_options
    assert validation_options() == (False, 1, "psnr")
    assert validation_options(val_dir="/x", val_step=3, val_monitor="de94") == (True, 3, "de94")
    assert validation_options(val_fraction=0.25, val_batch_size=1) == (True, 1, "psnr")
    with pytest.raises(ValueError, match="val_dir.*val_fraction"):
        validation_options(val_dir="/x", val_fraction=0.2)
    with pytest.raises(ValueError, match="val_monitor"):
        validation_options(val_dir="/x", val_monitor="fid")
    with pytest.raises(ValueError, match="val_monitor"):
        validation_options(val_monitor="PSNR")
    for bad in (0, -1, 1.5, True):
        with pytest.raises(ValueError, match="val_step"):
            validation_options(val_dir="/x", val_step=bad)
    with pytest.raises(ValueError, match="val_batch_size"):
        validation_options(val_dir="/x", val_batch_size=0)
    with pytest.raises(ValueError, match="val_fraction"):
        validation_options(val_fraction=1.0)
    assert set(VAL_MONITORS) == {"mse", "psnr", "ssim", "de76", "de94"}
    assert improves("psnr", 2.0, 1.0) and not improves("psnr", 1.0, 1.0) and improves("ssim", 0.5, None)
    assert improves("mse", 1.0, 2.0) and not improves("de76", 3.0, 2.0) and not improves("de94", float("nan"), None)


def test_trainer_defaults_leave_everything_off():
    from shmgan_amd.trainer import _DEFAULTS
    want = dict(ema_decay=0.0, ema_warmup=True, val_dir="", val_fraction=0.0, val_seed=0, val_step=1, val_batch_size=None,
                val_monitor="psnr", eval_weights="raw", eval_checkpoint="latest")
    assert {k: _DEFAULTS[k] for k in want} == want


def test_eval_options(tmp_path):
    from shmgan_amd import evaluate as ev
    assert ev.eval_options() == ("raw", "latest") and ev.eval_options("ema", "best") == ("ema", "best")
    assert ev.eval_options("raw", tmp_path / "some.npz") == ("raw", str(tmp_path / "some.npz"))
    for bad in ("avg", "EMA", None, 1):
        with pytest.raises(ValueError, match="eval_weights"):
            ev.eval_options(bad, "latest")
    for bad in ("newest", "", 3, "ckpt-1"):
        with pytest.raises(ValueError, match="eval_checkpoint"):
            ev.eval_options("raw", bad)
    # test() makes the check before it looks at a single file
    stub = SimpleNamespace(args=SimpleNamespace(), image_size=32, device=None, result_dir=str(tmp_path / "r"))
    with pytest.raises(ValueError, match="eval_weights"):
        ev.test(stub, SimpleNamespace(test_dir=str(tmp_path / "absent"), eval_weights="mean"))
    with pytest.raises(ValueError, match="eval_checkpoint"):
        ev.test(stub, SimpleNamespace(test_dir=str(tmp_path / "absent"), eval_checkpoint="newest"))


def test_read_validation(tmp_path):
    from shmgan_amd.telemetry import VALIDATION_FILE, read_log, read_validation, write_lines
    assert read_validation(str(tmp_path)) == []
    rows = [{"step": 3, "epoch": 0, "weights": "raw", "n": 2, "held_out": 3, "mse": 0.1, "psnr": 10.000000000000002, "ssim": 0.5,
             "de76": 1.0, "de94": 0.9, "best": True}, {"step": 6, "epoch": 1, "weights": "ema", "best": False}]
    write_lines(str(tmp_path / VALIDATION_FILE), rows[:1])
    write_lines(str(tmp_path / VALIDATION_FILE), rows[1:])
    assert read_validation(str(tmp_path)) == rows
    assert set(read_log(str(tmp_path))) == {"losses", "gradients", "weights"}          # read_log's result is what it was


# ---------------------------------------------------------------------------------------------------------------- the split
def _capture(root, names, hw=(12, 10), subdirs=None):
    from PIL import Image
    from shmgan_amd.data import PSD_SUBDIRS
    rng = np.random.default_rng(5)
    for sub in subdirs or PSD_SUBDIRS:
        (root / sub).mkdir(parents=True)
        for nm in names:
            Image.fromarray(rng.integers(0, 256, (*hw, 3)).astype(np.uint8)).save(root / sub / nm)
    return root


def test_split_is_a_disjoint_cover_and_a_pure_function(tmp_path):
    from shmgan_amd.data import PolarDataset, split_indices, split_names
    names = [f"img_{i:03d}.png" for i in range(10)] + ["a-b.png", "a.png"]          # 'a-b.png' < 'a.png' as paths, 'a' < 'a-b' as stems
    root = _capture(tmp_path / "cap", names)
    ds = PolarDataset(str(root), 8, 2, device="cpu", rank=0, world=1, shuffle=True, seed=3)
    files = ds.files[0]
    tr, va = split_indices(files, 0.25, seed=7)
    assert len(va) == 3 and sorted(tr + va) == list(range(12)) and not set(tr) & set(va) and tr == sorted(tr) and va == sorted(va)
    assert (tr, va) == split_indices(list(files), 0.25, seed=7) and (tr, va) != split_indices(files, 0.25, seed=8)
    stems = [Path(f).stem for f in files]
    assert (sorted(stems[i] for i in tr), sorted(stems[i] for i in va)) == tuple(split_names(stems, 0.25, 7))       # both lists sorted by stem
    train, val = ds.split(0.25, seed=7)
    assert [train.files[0], val.files[0]] == [[files[i] for i in tr], [files[i] for i in va]]
    for v in range(5):                                                       # the five views stay paired
        assert [Path(f).name for f in val.files[v]] == [Path(f).name for f in val.files[0]]
    assert (train.n, val.n, len(train), len(val)) == (9, 3, 4, 1)
    # the training part keeps the loader's options, the held-out part is one sorted pass of rank 0 of 1
    assert (train.shuffle, train.seed, train.epochs, train.B) == (True, 3, 1, 2)
    assert (val.shuffle, val.augment, val.epochs, val.rank, val.world, val.B) == (False, None, 1, 0, 1, 2)
    # select= renumbers: positions, and with them shuffle, draws and cache keys, count within the subset
    sub = PolarDataset(str(root), 8, 1, device="cpu", rank=0, world=1, select=[2, 5, 11])
    assert sub.n == 3 and len(sub) == 3 and [sub.position(i, 0) for i in range(3)] == [0, 1, 2]
    assert sub.files[4] == [ds.files[4][i] for i in (2, 5, 11)]
    sh = PolarDataset(str(root), 8, 1, device="cpu", rank=0, world=1, select=[2, 5, 11], shuffle=True, seed=1)
    assert sorted(sh.position(i, 0) for i in range(3)) == [0, 1, 2]
    for bad in ([5, 2], [2, 2], [0, 12], [-1, 3]):
        with pytest.raises(ValueError, match="select"):
            PolarDataset(str(root), 8, 1, device="cpu", rank=0, world=1, select=bad)
    # a split of a split stays inside it
    t2, v2 = train.split(1 / 3, seed=0)
    assert set(t2.files[0]) | set(v2.files[0]) == set(train.files[0]) and not set(t2.files[0]) & set(v2.files[0])


def test_validation_loader_is_never_sharded(tmp_path, monkeypatch):
    """Every rank validates the whole held-out set: under a torch.distributed that reports rank 1 of 2 the training loader is
    sharded, the held-out one is not."""
    import torch.distributed as dist
    from shmgan_amd.data import PolarDataset, datasetLoad, split_indices, validation_loader
    names = [f"s{i:02d}.png" for i in range(11)]
    root = _capture(tmp_path / "train", names)
    vroot = _capture(tmp_path / "val", names[:7])
    monkeypatch.setattr(dist, "is_available", lambda: True)
    monkeypatch.setattr(dist, "is_initialized", lambda: True)
    monkeypatch.setattr(dist, "get_rank", lambda *a: 1)
    monkeypatch.setattr(dist, "get_world_size", lambda *a: 2)
    sharded = PolarDataset(str(root), 8, 2, device="cpu")
    assert (sharded.rank, sharded.world, len(sharded)) == (1, 2, 11 // 4)
    B = 2
    val = validation_loader(str(root), 8, B, val_dir=str(vroot), device="cpu")
    assert (val.rank, val.world, val.n, len(val)) == (0, 1, 7, 7 // B)
    val = validation_loader(str(root), 8, 4, val_fraction=0.4, val_seed=2, val_batch_size=B, device="cpu")
    n_val = round(11 * 0.4)
    assert (val.rank, val.world, val.n, len(val), val.B) == (0, 1, n_val, n_val // B, B)
    assert val.files[0] == [sharded.files[0][i] for i in split_indices(sharded.files[0], 0.4, 2)[1]]
    assert (val.shuffle, val.augment, val.epochs, val.flip_ud, val.diffuse_source) == (False, None, 1, True, "dir")
    assert validation_loader(str(root), 8, B, device="cpu") is None
    with pytest.raises(ValueError, match="val_dir.*val_fraction"):
        validation_loader(str(root), 8, B, val_dir=str(vroot), val_fraction=0.4)
    # datasetLoad: with val_fraction the training loader is the other part, sharded as ever, and length_dataset is its length
    tr = SimpleNamespace(args=SimpleNamespace(val_fraction=0.4, val_seed=2, val_batch_size=1, cache="none"), data_dir=str(root), image_size=8,
                         batch_size=2, device="cpu", num_epochs=3)
    length, ds = datasetLoad(tr)
    assert ds.n == 11 - n_val and length == ds.n // 2 == tr.length_dataset and (ds.rank, ds.world) == (1, 2)
    assert not set(ds.files[0]) & set(tr.valDataset.files[0]) and sorted(ds.files[0] + tr.valDataset.files[0]) == sharded.files[0]
    assert (tr.valDataset.world, len(tr.valDataset)) == (1, n_val)
    tr.args = SimpleNamespace()
    _, ds = datasetLoad(tr)
    assert ds.n == 11 and ds.select is None and tr.valDataset is None
