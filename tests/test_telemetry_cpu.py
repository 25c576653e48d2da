"""Training telemetry without a GPU: the numpy restatement of shm_tensor_stats against worked answers, the host-side
errors of the C entry points, the loss composition, the log files and the option parsing."""
import ctypes as C
import json

import numpy as np
import pytest

import telemetry_ref as tr
from shmgan_amd import _lib, ops
from shmgan_amd import telemetry as tel


def test_restatement_against_worked_answers():
    sub = np.array([1], dtype=np.uint32).view(np.float32)[0]              # the smallest subnormal
    vals = [0.0, -0.0, sub, 2.0 ** -41, -2.0 ** -40, 0.75, 1.0, -1.0, 1.5, np.nan, np.inf, -np.inf]
    x = np.array(vals, dtype=np.float32)
    sign, cls = tr.classify(x)
    #                 0  -0  sub 2^-41 -2^-40 .75 1   -1  1.5 nan inf -inf
    assert cls.tolist() == [0, 0, 0, 1, 2, 41, 42, 42, 42, 43, 43, 43]
    assert sign.tolist() == [0, 0, 0, 0, 1, 0, 0, 1, 0, 0, 0, 0]
    stats, hist = tr.segment_stats(x)
    want = np.zeros((2, tr.BINS), dtype=np.int64)
    want[0, 0], want[0, 1], want[1, 2], want[0, 41], want[0, 42], want[1, 42], want[0, 43] = 3, 1, 1, 1, 2, 1, 3
    assert (hist == want).all() and hist.sum() == x.size
    s = float(sub) + 2.0 ** -41 - 2.0 ** -40 + 0.75 + 1.0 - 1.0 + 1.5
    q = float(sub) ** 2 + 2.0 ** -82 + 2.0 ** -80 + 0.5625 + 1.0 + 1.0 + 2.25
    assert stats.tolist() == [9.0, 1.0, 2.0, -1.0, 1.5, s, q, 1.0]
    # the scale is applied first, in float32: 1.5 * 0.5 = 0.75 leaves the clip range and joins 1.0 * 0.5 in class 41, 0.75 * 0.5 is
    # class 40, -1.0 * 0.5 is class 41 under sign 1, -2^-40 * 0.5 and 2^-41 * 0.5 drop below EMIN
    stats, hist = tr.segment_stats(x, 0.5)
    assert stats[7] == 0 and hist[0, 41] == 2 and hist[0, 40] == 1 and hist[1, 41] == 1 and hist[1, 1] == 1 and hist[0, 1] == 1
    assert hist[:, 42].sum() == 0 and hist[0, 0] == 3 and hist[0, 43] == 3
    # no finite value at all
    stats, hist = tr.segment_stats(np.array([np.nan, np.inf], dtype=np.float32))
    assert stats.tolist() == [0.0, 1.0, 1.0, 0.0, 0.0, 0.0, 0.0, 0.0] and hist[0, 43] == 2


def test_restatement_counts_every_value_once_and_fills_every_class():
    rng = np.random.default_rng(7)
    n = 1_000_000
    x = (np.exp2(rng.uniform(-43.0, 3.0, n)) * rng.choice([-1.0, 1.0], n)).astype(np.float32)
    x[:100] = 0.0
    x[100:200] = np.array([5], dtype=np.uint32).view(np.float32)[0]
    x[200:300] = np.nan
    x[300:400] = -np.inf
    stats, hist = tr.segment_stats(x, 1.0 / 3.0)
    assert hist.sum() == n and stats[0] + stats[1] + stats[2] == n
    assert (hist[0] > 0).all() and (hist[1, 1:43] > 0).all() and hist[1, 0] == 0 and hist[1, 43] == 0
    assert stats[1] == 100 and stats[2] == 100 and hist[0, 0] == 200
    v = tr.scaled(x, 1.0 / 3.0)
    fin = np.isfinite(v)
    for e in (-40, -20, -1):
        m = fin & (np.abs(v) >= 2.0 ** e) & (np.abs(v) < 2.0 ** (e + 1))
        assert hist[0, e + 42] + hist[1, e + 42] == np.count_nonzero(m)
    assert stats[7] == np.count_nonzero(fin & (np.abs(v) > 1)) <= hist[:, 42].sum()


def test_header_constants_match_python():
    txt = _lib.HEADER.read_text()
    import re
    macros = {m.group(1): int(m.group(2).strip("()")) for m in re.finditer(r"#define (SHM_T(?:STAT|HIST)_[A-Z_]+|SHM_LOSS_ROW[A-Z_]*) (\(?-?\d+\)?)", txt)}
    assert macros["SHM_THIST_BINS"] == ops.THIST_BINS == tr.BINS == 44
    assert macros["SHM_THIST_EMIN"] == ops.THIST_EMIN == tr.EMIN == -40
    assert macros["SHM_TSTAT_N"] == ops.TSTAT_N == tr.NSTAT == len(ops.TSTAT_NAMES)
    assert macros["SHM_TSTAT_MAX_SEGS"] == ops.TSTAT_MAX_SEGS
    assert [macros["SHM_TSTAT_" + k.upper()] for k in ops.TSTAT_NAMES] == list(range(8))
    assert (macros["SHM_LOSS_ROW_DL"], macros["SHM_LOSS_ROW_IL"], macros["SHM_LOSS_ROW_SL"], macros["SHM_LOSS_ROW_STEP"],
            macros["SHM_LOSS_ROW_ABORT"], macros["SHM_LOSS_ROW"]) == (ops.LOSS_ROW_DL, ops.LOSS_ROW_IL, ops.LOSS_ROW_SL,
                                                                      ops.LOSS_ROW_STEP, ops.LOSS_ROW_ABORT, ops.LOSS_ROW)
    assert ops.LOSS_ROW_STEP == ops.LOSS_ROW_DL + ops.LOSS_ROW_IL + ops.LOSS_ROW_SL < ops.LOSS_ROW_ABORT < ops.LOSS_ROW


def test_tensor_stats_host_side_errors_without_gpu():
    """SHM_E_SHAPE / SHM_E_WORKSPACE are detected before any launch: no device is touched (the pointers are never read)."""
    L = _lib.lib()
    off = (C.c_size_t * 2)(0, 16)
    ln = (C.c_size_t * 2)(16, 100)
    x, st, hi, ws = 0x1000, 0x2000, 0x3000, 0x4000          # non-null stand-ins
    need = L.shm_tensor_stats_workspace(2, 116)
    assert need > 0 and L.shm_tensor_stats_workspace(1, 0) > 0
    assert L.shm_tensor_stats_workspace(53, 18_500_000) >= 18_500_000 // 8192 * 16
    assert L.shm_tensor_stats_workspace(0, 116) == 0
    for nseg in (0, -1, ops.TSTAT_MAX_SEGS + 1):
        assert L.shm_tensor_stats(x, 116, off, ln, nseg, 1.0, st, hi, ws, need, None) == -1 and b"nseg" in L.shm_last_error()
    for args in ((None, 116, off, ln), (x, 116, None, ln), (x, 116, off, None)):
        assert L.shm_tensor_stats(*args, 2, 1.0, st, hi, ws, need, None) == -1 and b"null pointer" in L.shm_last_error()
    assert L.shm_tensor_stats(x, 116, off, ln, 2, 1.0, None, hi, ws, need, None) == -1 and b"null pointer" in L.shm_last_error()
    assert L.shm_tensor_stats(x, 116, off, ln, 2, 1.0, st, None, ws, need, None) == -1 and b"null pointer" in L.shm_last_error()
    assert L.shm_tensor_stats(x, 115, off, ln, 2, 1.0, st, hi, ws, need, None) == -1 and b"segment 1" in L.shm_last_error()
    far = (C.c_size_t * 2)(0, 2 ** 63)
    assert L.shm_tensor_stats(x, 116, far, ln, 2, 1.0, st, hi, ws, need, None) == -1 and b"segment 1" in L.shm_last_error()
    huge = (C.c_size_t * 2)(16, 2 ** 64 - 8)                # offset + length wraps round
    assert L.shm_tensor_stats(x, 116, off, huge, 2, 1.0, st, hi, ws, need, None) == -1 and b"segment 1" in L.shm_last_error()
    assert L.shm_tensor_stats(x, 116, off, ln, 2, 1.0, st, hi, ws, 8, None) == -3 and b"workspace" in L.shm_last_error()
    assert L.shm_tensor_stats(x, 116, off, ln, 2, 1.0, st, hi, None, need, None) == -3 and b"workspace" in L.shm_last_error()
    # the loss ring's row is checked as well
    assert L.shm_loss_ring_put(x, x, x, None, x, 4, 4, 0, None) == -1 and b"row" in L.shm_last_error()
    assert L.shm_loss_ring_put(None, x, x, None, x, 4, 0, 0, None) == -1 and b"null pointer" in L.shm_last_error()


def _losses_by_formula(dl, il, sl, B, npix):
    """The formulas of Trainer.losses() as they stood before the composition moved into telemetry.compose_losses."""
    d = (dl / B).tolist()
    i = (il / B).tolist()
    D1_RF, D3_RF = d[0], d[1]
    D2_RF = d[4] + d[2]
    D4_RF = d[5] + d[3] + D2_RF
    D1_cls, D3_cls, D4_cls = d[6], d[7], d[8]
    L1 = (i[1] + i[2] + i[3] + i[4] + i[0]) / 5.0 + i[5] * 10.0
    ssim_loss = (i[11] + i[12] + i[13] + i[14] + i[15] * 10.0) / 5.0
    content, style = i[16], i[17]
    nst = 100.0 * style + content
    sp = (sl / (B * npix * 3.0)).tolist()
    return {
        "total_Generator_loss": (D1_RF + D3_RF) / 6.0 + 10.0 * L1 + 10.0 * ssim_loss + 10.0 * nst,
        "total_Discriminator_loss": (D1_cls + D3_cls) / 6.0 + (D2_RF + D4_RF) / 6.0 + 0.5 * D4_cls + 10.0 * nst,
        "total_Classification_loss": (D4_cls + nst) * 10.0,
        "G_gan_loss": (D3_RF + D1_RF) / 6.0, "G_clsf_loss": (D3_cls + D1_cls) / 6.0,
        "D1_RealFake_loss": D1_RF, "D3_RealFake_cyc": D3_RF, "D2_RealFake_target": D2_RF,
        "D4_RealFake_cyc": D4_RF, "D1_classification_loss": D1_cls, "D3_classification_loss": D3_cls,
        "D4_classification_loss": D4_cls, "L1_loss_Gen": L1, "ssim_cyc_loss": ssim_loss,
        "content_loss": content, "style_loss": style, "total_NST_loss": nst,
        "Spec_loss": (sp[0] + sp[1] + sp[2] + sp[3]) / 5.0 + sp[4] * 5.0,
        "ssim": [i[6 + k] for k in range(5)],
    }


def test_loss_composition_and_log_round_trip(tmp_path):
    rng = np.random.default_rng(3)
    dl, il, sl = rng.normal(size=16) * 7, rng.normal(size=32) * 1e3, rng.random(5) * 1e5
    for B, npix in ((1, 64 * 64), (8, 256 * 256)):
        got = tel.compose_losses(dl, il, sl, B, npix)
        want = _losses_by_formula(dl, il, sl, B, npix)
        assert list(got) == list(want) == tel.LOSS_NAMES + ["ssim"]
        assert got == want                                  # the same float64 bits
    assert got["G_gan_loss"] == (dl[1] / 8 + dl[0] / 8) / 6.0
    from shmgan_amd import LOSS_NAMES
    assert LOSS_NAMES is tel.LOSS_NAMES and len(LOSS_NAMES) == 18
    # one line through the file and back: float64 survives json exactly
    rec = {"step": 25, "epoch": 0, "TARGET_LABELS": 0.9}
    rec.update(got)
    tel.write_lines(tmp_path / "losses.jsonl", [rec])
    stats, hist = tr.segment_stats(np.array([0.5, -3.0, np.nan, 1e-30], dtype=np.float32))
    grec = tel.stats_record(100, "G", "G/var03", (2, 2), stats, hist)
    tel.write_lines(tmp_path / "gradients.jsonl", [grec, grec])
    log = tel.read_log(tmp_path)
    assert log["losses"] == [rec] and log["weights"] == [] and len(log["gradients"]) == 2
    back = log["gradients"][1]
    assert back["name"] == "G/var03" and back["shape"] == [2, 2] and back["nan"] == 1 and back["finite"] == 3 and back["clipped"] == 1
    assert back["sum"] == stats[5] and back["min"] == -3.0
    assert all(n > 0 for _, _, n in back["hist"]) and (tel.hist_dense(back) == hist).all()
    assert set(json.loads((tmp_path / "losses.jsonl").read_text())) == {"step", "epoch", "TARGET_LABELS", "ssim", *tel.LOSS_NAMES}


def test_option_parsing():
    assert tel.telemetry_options() == (0, 0, "ignore")
    assert tel.telemetry_options(25, 100) == (25, 100, "warn")
    assert tel.telemetry_options(None, "100", None) == (0, 100, "warn")
    assert tel.telemetry_options(0, 0, "raise") == (0, 0, "raise")
    assert tel.telemetry_options(5, 0, "ignore") == (5, 0, "ignore")
    for bad in ("abort", "Warn", 1):
        with pytest.raises(ValueError, match="nonfinite"):
            tel.telemetry_options(25, 100, bad)
    for bad in (-1, 2.5, "often", True):
        with pytest.raises(ValueError, match="loss_log_step"):
            tel.telemetry_options(bad, 0)
    with pytest.raises(ValueError, match="histogram_step"):
        tel.telemetry_options(0, -100)
    from shmgan_amd.trainer import _DEFAULTS
    assert (_DEFAULTS["loss_log_step"], _DEFAULTS["histogram_step"], _DEFAULTS["nonfinite"]) == (0, 0, None)


def test_variable_names_follow_the_checkpoint_keys():
    """A variable's name is its save_npz key: position in Keras variable order, offset and size of its storage slot."""
    import torch
    from shmgan_amd.model import Arena, Discriminator, Generator
    dev = torch.device("cpu")
    for attention in (False, True):
        g = Generator(64, 16, dev, Arena(dev), lambda n: None, attention=attention)
        d = Discriminator(64, 16, dev, Arena(dev), lambda n: None, 0.2, attention=attention)
        for M, tag in ((g, "G"), (d, "D")):
            tab = tel.variable_table(M, tag)
            assert [n for n, _, _, _ in tab] == [f"{tag}/var{k:02d}" for k in range(len(M.P.vars))]
            assert len(tab) <= ops.TSTAT_MAX_SEGS
            seen = np.zeros(M.P.n, dtype=np.int32)
            for (name, off, size, shape), w in zip(tab, M.trainable_variables):
                assert tuple(w.shape) == shape and w.numel() == size
                assert w.data_ptr() == M.P.flat.data_ptr() + 4 * off
                seen[off:off + size] += 1
            assert (seen == 1).all()
