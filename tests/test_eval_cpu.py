"""Test mode without a GPU: the float64 restatement of the metrics against known answers, the C ABI of shm_image_metrics,
the signature of shmgan_amd.evaluate.test and the evaluation loader's listing and pairing."""
import inspect
import re

import numpy as np
import pytest

from shmgan_amd import _lib

from metrics_ref import delta_e76, delta_e94, psnr, rgb_to_lab


def test_lab_known_answers():
    want = {(1.0, 1.0, 1.0): (100.0, -0.002455, 0.004653),
            (0.5, 0.5, 0.5): (53.38896, -0.001468, 0.002784),
            (1.0, 0.0, 0.0): (53.24059, 80.09231, 67.20275)}
    for rgb, lab in want.items():
        got = rgb_to_lab(np.array(rgb))
        assert np.allclose(got, lab, rtol=0, atol=6e-6), (rgb, got)
    # out-of-range inputs (gen_rgb is not clipped) take the linear branches: finite, no NaN from the branch not chosen
    assert np.isfinite(rgb_to_lab(np.array([-0.3, 1.3, -0.06]))).all()


def test_delta_e_known_answers_and_asymmetry():
    red, black = rgb_to_lab(np.array([1.0, 0.0, 0.0])), rgb_to_lab(np.array([0.0, 0.0, 0.0]))
    assert abs(delta_e94(red, black) - 56.30661) < 1e-5
    assert abs(delta_e94(black, red) - 117.32667) < 1e-5
    assert abs(delta_e76(red, black) - 117.32667) < 1e-5
    assert abs(delta_e76(black, red) - 117.32667) < 1e-5
    assert delta_e94(red, red) == 0.0


def test_psnr_of_a_known_mse():
    assert abs(float(psnr(0.01)) - 20.0) < 1e-12
    assert abs(float(psnr(1e-4)) - 40.0) < 1e-12
    assert float(psnr(0.0)) == np.inf


def test_header_declares_the_metric_entry_points():
    txt = re.sub(r"/\*.*?\*/", "", _lib.HEADER.read_text(), flags=re.S)
    for name, nargs in (("shm_image_metrics_workspace", 2), ("shm_image_metrics", 8)):
        m = re.search(r"\b" + name + r"\s*\(([^;]*?)\)\s*;", txt, flags=re.S)
        assert m, name
        assert len(m.group(1).split(",")) == nargs == len(_lib.SIGNATURES[name][1])
    assert "metrics.hip" in _lib.SOURCES


def test_workspace_query_without_gpu():
    L = _lib.lib()
    assert L.shm_image_metrics_workspace(1, 10) == 0 and L.shm_image_metrics_workspace(0, 64) == 0
    w1, w8 = L.shm_image_metrics_workspace(1, 256), L.shm_image_metrics_workspace(8, 256)
    assert 0 < w1 < w8 <= 8 * w1
    # errors are detected on the host before any launch: safe without a GPU
    assert L.shm_image_metrics(None, None, None, None, 0, 1, 10, None) == -1 and b"< 11" in L.shm_last_error()
    assert L.shm_image_metrics(None, None, None, None, 0, 0, 64, None) == -1


def test_evaluate_test_signature():
    import shmgan_amd
    from shmgan_amd import evaluate
    assert list(inspect.signature(evaluate.test).parameters)[:2] == ["shmgan", "args"]
    assert shmgan_amd.test is evaluate.test
    from shmgan_amd.trainer import _DEFAULTS, ShmGANwithSSpecSeg
    assert _DEFAULTS["calc_metrics"] is False and _DEFAULTS["test_dir"] == "" and _DEFAULTS["diffuse_dir"] == ""
    assert list(inspect.signature(ShmGANwithSSpecSeg.evaluate).parameters) == ["self", "rgb", "diffuse"]


def test_table_headers_and_plain_format():
    from shmgan_amd import evaluate
    assert evaluate.TABLE_HEADERS == ["Image#", "Time", "MSE", "SSIM", "PSNR", "delE76", "delE94"]
    assert evaluate.MEAN_HEADERS[3] == "Mean dleE76"
    txt = evaluate.format_table([[1, 0.5, 0.25]], ["a", "b", "c"])
    assert "a" in txt and "0.25" in txt


def test_plain_table_without_tabulate(monkeypatch):
    import sys
    from shmgan_amd import evaluate
    monkeypatch.setitem(sys.modules, "tabulate", None)          # import tabulate -> ImportError
    lines = evaluate.format_table([[1, 0.5, float("inf")], [2, 0.25, 30.0]], ["Image#", "MSE", "PSNR"]).splitlines()
    assert len(lines) == 4 and lines[0].split() == ["Image#", "MSE", "PSNR"] and set(lines[1]) <= {"-", " "}
    assert lines[2].split() == ["1", "0.5", "inf"] and lines[3].split() == ["2", "0.25", "30"]


def _touch(d, names):
    d.mkdir()
    for n in names:
        (d / n).write_bytes(b"")


def test_eval_loader_listing_pairing_and_mismatch(tmp_path):
    from shmgan_amd.data import EvalDataset, eval_file_lists
    _touch(tmp_path / "test", ["b.png", "a.jpg", "c.PNG", "notes.txt", "d.bmp", "e.png"])
    _touch(tmp_path / "diffuse", ["5.png", "1.png", "3.png", "2.png", "4.png"])
    _touch(tmp_path / "short", ["1.png", "2.png"])
    t, d = eval_file_lists(tmp_path / "test", tmp_path / "diffuse")
    assert [p.rsplit("/", 1)[1] for p in t] == ["a.jpg", "b.png", "c.PNG", "d.bmp", "e.png"]
    assert [p.rsplit("/", 1)[1] for p in d] == ["1.png", "2.png", "3.png", "4.png", "5.png"]
    assert eval_file_lists(tmp_path / "test", "")[1] is None
    with pytest.raises(ValueError, match="same number"):
        eval_file_lists(tmp_path / "test", tmp_path / "short")
    ds = EvalDataset(tmp_path / "test", 32, 2, tmp_path / "diffuse", device="cpu")
    assert len(ds) == 3 and (ds.rank, ds.world) == (0, 1)
    assert [ds.batch_range(i) for i in range(3)] == [(0, 2), (2, 4), (4, 5)]      # the tail batch is kept
    assert len(EvalDataset(tmp_path / "test", 32, 5, device="cpu")) == 1
    assert len(EvalDataset(tmp_path / "test", 32, 1, device="cpu")) == 5
