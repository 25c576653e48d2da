"""Test-mode image export without a GPU: the float64 restatement (tests/export_ref.py) against answers worked by hand, the C ABI
of shm_export_u8 (host-side errors, workspace query), the export options and file naming of shmgan_amd.evaluate, and the
source sizes the evaluation loader reports."""
import ctypes as C
import re
from types import SimpleNamespace

import numpy as np
import pytest

from shmgan_amd import _lib

import export_ref as xr

E_SHAPE, E_WORKSPACE = -1, -3


def test_resize_2x2_to_4x4_by_hand():
    # f = (o + 0.5) / 2 - 0.5 = -0.25, 0.25, 0.75, 1.25 -> taps (0,0) w 0, (0,1) w .25, (0,1) w .75, (1,1) w 0
    x = np.array([[0.0, 1.0], [2.0, 3.0]])[..., None]
    want = np.array([[0.0, 0.25, 0.75, 1.0],
                     [0.5, 0.75, 1.25, 1.5],
                     [1.5, 1.75, 2.25, 2.5],
                     [2.0, 2.25, 2.75, 3.0]])
    assert np.array_equal(xr.resize_bilinear(x, 4, 4)[..., 0], want)


def test_resize_4x4_to_2x2_by_hand():
    # f = (o + 0.5) * 2 - 0.5 = 0.5, 2.5: the mean of each 2x2 quad
    x = np.arange(16, dtype=np.float64).reshape(4, 4, 1)
    assert np.array_equal(xr.resize_bilinear(x, 2, 2)[..., 0], np.array([[2.5, 4.5], [10.5, 12.5]]))


def test_rescale_of_a_constant_plane_is_zero():
    assert np.array_equal(xr.rescale_01(np.full((3, 3, 3), 0.7)), np.zeros((3, 3, 3)))
    b, _ = xr.export(np.full((4, 4, 3), -2.0), 6, 5, "rescale")
    assert b.shape == (6, 5, 3) and not b.any()
    b, _ = xr.export(np.array([[0.0, 1.0], [2.0, 4.0]])[..., None], 2, 2, "rescale")
    assert b[..., 0].tolist() == [[0, 64], [128, 255]]             # 63.75 -> 64, 127.5 -> 128 (even)


def test_quantize_rounds_half_to_even_and_clamps():
    b, y = xr.quantize(np.array([0.5, 1.5, 2.5, 3.5, 254.5]) / 255.0)
    assert y.tolist() == [0.5, 1.5, 2.5, 3.5, 254.5]
    assert b.tolist() == [0, 2, 2, 4, 254]
    b, _ = xr.quantize(np.array([-1.0, 0.0, 1.0, 7.0]))
    assert b.tolist() == [0, 0, 255, 255]
    assert xr.near_half(np.array([0.5, 0.5004, 0.502, 3.0])).tolist() == [True, True, False, False]


def test_header_declares_the_export_entry_points():
    txt = re.sub(r"/\*.*?\*/", "", _lib.HEADER.read_text(), flags=re.S)
    for name, nargs in (("shm_export_u8_workspace", 1), ("shm_export_u8", 10), ("shm_running_scale_mean", 5)):
        m = re.search(r"\b" + name + r"\s*\(([^;]*?)\)\s*;", txt, flags=re.S)
        assert m, name
        assert len(m.group(1).split(",")) == nargs == len(_lib.SIGNATURES[name][1])
    assert "export.hip" in _lib.SOURCES
    from shmgan_amd import ops
    for macro, value in (("SHM_EXPORT_RESCALE", ops.EXPORT_MODES["rescale"]), ("SHM_EXPORT_SCALE", ops.EXPORT_MODES["scale"]),
                         ("SHM_EXPORT_CLIP", ops.EXPORT_MODES["clip"]), ("SHM_EXPORT_DESC", ops.EXPORT_DESC),
                         ("SHM_EXPORT_MAX_JOBS", ops.EXPORT_MAX_JOBS)):
        assert re.search(r"#define " + macro + r" " + str(value) + r"\b", txt), macro


def test_workspace_query_is_monotonic():
    L = _lib.lib()
    assert L.shm_export_u8_workspace(0) == 0 and L.shm_export_u8_workspace(-3) == 0
    w = [L.shm_export_u8_workspace(n) for n in range(1, 70)]
    assert w[0] > 0 and all(a < b for a, b in zip(w, w[1:]))


FAKE = 4096          # a non-null, aligned address: every call below is refused on the host, before any launch


def _call(jobs, njobs=None, mul=FAKE, nmul=4, dst=FAKE, dst_bytes=1 << 20, ws=FAKE, ws_bytes=None, src=None):
    L = _lib.lib()
    n = len(jobs)
    srcs = (C.c_void_p * max(n, 1))(*(src if src is not None else [FAKE] * n))
    desc = (C.c_size_t * (8 * max(n, 1)))(*[v for d in jobs for v in d])
    if ws_bytes is None:
        ws_bytes = L.shm_export_u8_workspace(max(n, 1))
    return L.shm_export_u8(srcs, desc, len(jobs) if njobs is None else njobs, mul, nmul, dst, dst_bytes, ws, ws_bytes, None)


def test_errors_before_any_launch():
    L = _lib.lib()
    ok = [16, 3, 3, 20, 24, 0, 0, 0]                # s, c, ld, ho, wo, mode, k, dst_off
    cases = [
        ([], dict(njobs=0), E_SHAPE, b"njobs"),
        ([ok] * 65, {}, E_SHAPE, b"njobs"),
        ([ok], dict(dst=None), E_SHAPE, b"null pointer"),
        ([ok], dict(src=[None]), E_SHAPE, b"null pointer"),
        ([ok], dict(dst=FAKE + 2), E_SHAPE, b"aligned"),
        ([[16, 2, 3, 20, 24, 0, 0, 0]], {}, E_SHAPE, b"not in {1, 3}"),
        ([[16, 3, 2, 20, 24, 0, 0, 0]], {}, E_SHAPE, b"ld"),
        ([[0, 3, 3, 20, 24, 0, 0, 0]], {}, E_SHAPE, b"sizes"),
        ([[16, 3, 3, 0, 24, 0, 0, 0]], {}, E_SHAPE, b"sizes"),
        ([[16, 3, 3, 20, 40000, 0, 0, 0]], {}, E_SHAPE, b"sizes"),
        ([[16, 3, 3, 20, 24, 3, 0, 0]], {}, E_SHAPE, b"mode"),
        ([[16, 3, 3, 20, 24, 1, 4, 0]], {}, E_SHAPE, b"SCALE"),
        ([[16, 3, 3, 20, 24, 1, 0, 0]], dict(mul=None), E_SHAPE, b"SCALE"),
        ([[16, 3, 3, 20, 24, 0, 0, 2]], {}, E_SHAPE, b"multiple of 4"),
        ([ok], dict(dst_bytes=20 * 24 * 3 - 1), E_SHAPE, b"destination"),
        ([[16, 3, 3, 20, 24, 2, 0, 1 << 21]], {}, E_SHAPE, b"destination"),
        ([ok, ok], dict(ws_bytes=L.shm_export_u8_workspace(2) - 1), E_WORKSPACE, b"workspace"),
        ([ok], dict(ws=None), E_WORKSPACE, b"workspace"),
    ]
    for jobs, kw, rc, msg in cases:
        assert _call(jobs, **kw) == rc, (jobs, kw)
        assert msg in L.shm_last_error(), (jobs, kw, L.shm_last_error())
    # the bad job is named by its index
    assert _call([ok, ok, [16, 3, 3, 20, 24, 7, 0, 0]]) == E_SHAPE and b"job 2" in L.shm_last_error()
    assert L.shm_running_scale_mean(None, 2, FAKE, FAKE, None) == E_SHAPE
    assert L.shm_running_scale_mean(FAKE, 0, FAKE, FAKE, None) == E_SHAPE and b"batch" in L.shm_last_error()


def test_export_layout_aligns_every_job():
    from shmgan_amd import ops
    offs, total = ops.export_layout([(3, 5), (2, 2), (7, 1)], [3, 1, 3])
    assert offs == [0, 48, 64] and total == 96
    assert all(o % 4 == 0 for o in offs)


def test_new_defaults_are_off():
    from shmgan_amd.trainer import _DEFAULTS
    assert _DEFAULTS["save_images"] is False
    assert _DEFAULTS["image_values"] == "rescale" and _DEFAULTS["image_out_size"] == "source" and _DEFAULTS["image_dir"] == ""


def test_output_naming_and_options():
    from shmgan_amd import evaluate as ev
    assert ev.IMAGE_TAGS == ("G1", "G1_Y", "cyc0", "cyc45", "cyc90", "cyc135", "cycED", "mask")
    assert ev.image_name("img01", "G1") == "img01_G1.png" and ev.image_name("a.b", "cycED") == "a.b_cycED.png"
    assert ev.source_stem("/x/y/photo.v2.jpg") == "photo.v2"
    assert ev.image_options(False, "rescale", "source") == ()
    assert ev.image_options(None, "output", "model") == ()
    assert ev.image_options("g1", "rescale", "source") == ("G1",)
    assert ev.image_options("all", "output", "model") == ev.IMAGE_TAGS
    for bad in ((True, "rescale", "source"), ("G1", "rescale", "source"), ("all", "raw", "source"), ("all", "rescale", "full")):
        with pytest.raises(ValueError):
            ev.image_options(*bad)


def _write(d, names_sizes):
    from PIL import Image
    d.mkdir()
    rng = np.random.default_rng(0)
    for name, (h, w) in names_sizes:
        Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)).save(d / name)
    return d


def test_stem_collision_raises_before_anything_runs(tmp_path):
    from shmgan_amd import evaluate as ev
    with pytest.raises(ValueError, match=r"a: a\.jpg, a\.png"):
        ev.check_stems(["/d/a.png", "/d/b.png", "/d/a.jpg"])
    ev.check_stems(["/d/a.png", "/d/b.png"])
    d = _write(tmp_path / "test", [("a.png", (8, 8)), ("a.bmp", (8, 8)), ("c.png", (8, 8))])
    # a stand-in trainer with nothing to run: test() must refuse before it builds, restores or evaluates anything
    fake = SimpleNamespace(args=SimpleNamespace(), image_size=8, device=None, result_dir=str(tmp_path / "r"))
    with pytest.raises(ValueError, match=r"a\.bmp, a\.png"):
        ev.test(fake, SimpleNamespace(test_dir=str(d), save_images="all"))
    assert not (tmp_path / "r").exists()


def test_loader_reports_source_sizes_and_names(tmp_path):
    from shmgan_amd.data import EvalDataset
    d = _write(tmp_path / "test", [("p0.png", (40, 48)), ("p1.png", (37, 29)), ("p2.png", (64, 64))])
    ds = EvalDataset(str(d), 32, 2)
    assert [(p.rsplit("/", 1)[1], hw) for p, hw in ds.sources(0)] == [("p0.png", (40, 48)), ("p1.png", (37, 29))]
    test, _ = ds._decode_batch(1)                   # the sizes of a decoded batch come from the decode
    assert test[0].shape == (64, 64, 3)
    assert [(p.rsplit("/", 1)[1], hw) for p, hw in ds.sources(1)] == [("p2.png", (64, 64))]
