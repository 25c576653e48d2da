"""shm_dofp_calibrate (csrc/dofp_calibrate.hip) and everything built on it, on the device.

The kernel is compared bit for bit with the NumPy restatement (tests/calibrate_ref.py, which tests/test_calibrate_cpu.py holds against a
per-photosite brute force): P x P frames, ragged and multi-block shapes, uint8 and uint16 at 8 / 12 / 16 bits, mono and a Bayer pattern, all
eight null / non-null combinations of the three tables, random / all-maximum / over-range / half-defective data, and both access paths --
pitched sources whose gap holds the largest value, destinations carved out of a poisoned pool at aligned and at odd element offsets with
nothing outside them written, sources and tables that start 0, 1, 2 and 4 samples off.  The plumbing is tested by equivalence: a layout
with a calibration must give exactly what the same layout without one gives of the restatement-corrected mosaic.  No tolerance anywhere."""
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import calibrate_ref as cr
import dofp_ref as dr

pytestmark = pytest.mark.gpu

POISON = 0xA5
E_SHAPE = -1


def _lib():
    from shmgan_amd import _lib as L
    return L.lib()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _poisoned(n, dtype):
    """A pool of n elements whose every byte is the poison."""
    return torch.full((n * dtype.itemsize,), POISON, dtype=torch.uint8, device="cuda"), int.from_bytes(bytes([POISON]) * dtype.itemsize, "little")


def _run(src_t, src_off, spitch, shape, pattern, bits, tables, ped, white, dst_off, dpitch, np_dtype):
    """The kernel from element src_off of the device buffer src_t into a poisoned pool, from element dst_off on, rows dpitch apart:
    (dst [h,w], True if every element of the pool outside the h rows of w still holds the poison)."""
    h, w = shape
    size = np_dtype.itemsize
    pool, word = _poisoned(dst_off + h * dpitch + 64, np_dtype)
    ptr = lambda t: None if t is None else t.data_ptr()
    rc = _lib().shm_dofp_calibrate(src_t.data_ptr() + src_off * size, bits, h, w, spitch, dr.PATTERNS.index(pattern), ptr(tables[0]), ptr(tables[1]),
                                   ptr(tables[2]), ped, white, pool.data_ptr() + dst_off * size, dpitch, _stream())
    assert rc == 0, (rc, _lib().shm_last_error())
    got = pool.cpu().numpy().view(np_dtype)
    rows = got[dst_off:dst_off + h * dpitch].reshape(h, dpitch)
    outside = np.ones(got.shape, dtype=bool)
    for y in range(h):
        outside[dst_off + y * dpitch:dst_off + y * dpitch + w] = False
    return rows[:, :w], bool(np.all(got[outside] == word))


@pytest.fixture(scope="module")
def device_tables():
    """(dark, gain, defect) of a case on the device: uploaded once per case."""
    made = {}

    def get(shape, pattern, bits, kind):
        key = (shape, pattern, bits, kind)
        if key not in made:
            made[key] = tuple(torch.from_numpy(np.array(t)).cuda() for t in cr.case(shape, pattern, bits, kind)[1:4])
        return made[key]
    return get


@pytest.mark.parametrize("shape,pattern", [(s, p) for s in cr.SHAPES for p in cr.PATTERNS], ids=str)
def test_kernel_bit_exact(shape, pattern, device_tables):
    """cr.MULTI_BLOCK (9 x 1032) is the shape that needs more than one block along each axis of the launch as built -- 64 x 4 threads of 8
    samples: 3 x 3 blocks -- with every access wide; cr.MULTI_BLOCK_RAGGED (6 x 1030) is the same with a last group of 6 samples."""
    h, w = cr.shape_of(shape, pattern)
    for bits in cr.BITS:
        for kind in cr.kinds_of(bits):
            src, _, _, _, ped, white = cr.case(shape, pattern, bits, kind)
            top = np.iinfo(src.dtype).max
            extra = cr.pitch_extra(w)
            tight = torch.from_numpy(np.array(src)).cuda()
            wide = torch.from_numpy(dr.pitched(src, w + extra, top)[0]).cuda()          # a pitch of a multiple of 8: the wide accesses
            odd = torch.from_numpy(dr.pitched(src, w + 5, top)[0]).cuda()
            dev = device_tables(shape, pattern, bits, kind)
            for which in cr.TABLES:
                ref = cr.case_reference(shape, pattern, bits, kind, which)
                tables = tuple(t if use else None for t, use in zip(dev, which))
                # tight to tight; pitched to pitched, both aligned; a pitch that is no multiple of 8 to an odd element offset
                for name, s, spitch, dst_off, dpitch in (("tight", tight, w, 64, w), ("pitched", wide, w + extra, 64, w + extra), ("odd", odd, w + 5, 61, w + 3)):
                    got, clean = _run(s, 0, spitch, (h, w), pattern, bits, tables, ped, white, dst_off, dpitch, src.dtype)
                    what = (shape, pattern, bits, kind, which, name)
                    assert clean, ("an element outside the destination rows was written", what)
                    assert np.array_equal(got, ref), (what, np.argwhere(got != ref)[:4])


@pytest.mark.parametrize("pattern,bits", [("mono", 8), ("rggb", 12), ("rggb", 16)])
def test_source_destination_and_table_alignment(pattern, bits, device_tables):
    """Groups of 8 are read and written in one access where base and pitch allow it and one element at a time elsewhere, per array: a frame
    that starts 0, 1, 2 or 4 samples into a row of a wider buffer, a destination at the same offsets, and tables that start off their
    alignment although the width would allow the wide path, all give the same bits."""
    shape, kind, which = (20, 40), "half", (True, True, True)
    h, w = shape
    src, dark, gain, defect, ped, white = cr.case(shape, pattern, bits, kind)
    ref = cr.case_reference(shape, pattern, bits, kind, which)
    dev = device_tables(shape, pattern, bits, kind)
    for shift in (0, 1, 2, 4):
        buf = np.full((h, 48), np.iinfo(src.dtype).max, dtype=src.dtype)
        buf[:, shift:shift + w] = src
        s = torch.from_numpy(buf).cuda()
        for dst_off in (64, 64 + shift):
            got, clean = _run(s, shift, 48, shape, pattern, bits, dev, ped, white, dst_off, 48, src.dtype)
            assert clean and np.array_equal(got, ref), (shift, dst_off)
        # the tables from a buffer `shift` elements in
        moved = []
        for t in (dark, gain, defect):
            flat = np.zeros(t.size + 8, dtype=t.dtype)
            flat[shift:shift + t.size] = t.reshape(-1)
            moved.append(torch.from_numpy(flat).cuda()[shift:shift + t.size])
        got, clean = _run(s, shift, 48, shape, pattern, bits, moved, ped, white, 64, 48, src.dtype)
        assert clean and np.array_equal(got, ref), ("tables", shift)


def test_refusals_leave_the_destination_untouched():
    h, w = 8, 12
    src = torch.zeros((h, w + 4), dtype=torch.uint16, device="cuda")
    pool, word = _poisoned(h * (w + 4) + 64, np.dtype(np.uint16))
    tabs = [torch.from_numpy(t).cuda() for t in cr.identity_tables((h, w), 240)]
    good = dict(src=src.data_ptr(), bits=12, h=h, w=w, spitch=w + 4, pattern=1, dark=tabs[0].data_ptr(), gain=tabs[1].data_ptr(), defect=tabs[2].data_ptr(),
                pedestal=240, white=4095, dst=pool.data_ptr() + 32, dpitch=w + 4)
    call = lambda a: _lib().shm_dofp_calibrate(a["src"], a["bits"], a["h"], a["w"], a["spitch"], a["pattern"], a["dark"], a["gain"], a["defect"],
                                               a["pedestal"], a["white"], a["dst"], a["dpitch"], _stream())
    assert call(good) == 0 and call(dict(good, pattern=0, h=2, w=2)) == 0
    torch.cuda.synchronize()
    pool.fill_(POISON)
    # dst == src is refused with dst pointing at the pool, so that a launch would show there
    for change in (dict(src=None), dict(dst=None), dict(bits=7), dict(bits=17), dict(h=3), dict(w=3), dict(pattern=0, h=1), dict(h=32769),
                   dict(w=32769, spitch=40000, dpitch=40000), dict(spitch=w - 1), dict(dpitch=w - 1), dict(pattern=5), dict(pattern=-1),
                   dict(src=pool.data_ptr() + 32), dict(pedestal=-1), dict(pedestal=65520), dict(white=0), dict(white=65537)):
        rc = call(dict(good, **change))
        assert rc == E_SHAPE, (change, rc)
        assert b"shm_dofp_calibrate" in _lib().shm_last_error(), change
    torch.cuda.synchronize()
    assert bool((pool == POISON).all())


# ---- equivalence through the stack ------------------------------------------------------------------------------------------------------------
ANGLES = (0, 45, 90, 135)


def _layout(pattern, bits, develop=None, calibration=None, quad=dr.SONY_QUAD):
    from shmgan_amd.polar import DofpLayout
    return DofpLayout(pattern, tuple(ANGLES[q] for q in quad), bits, develop, calibration)


def _calibration(shape, pattern, bits, kind="random", which=(True, True, True)):
    from shmgan_amd.polar import DofpCalibration
    src, _, _, _, ped, white = cr.case(shape, pattern, bits, kind)
    dark, gain, defect = cr.case_tables(shape, pattern, bits, kind, which)
    return src, DofpCalibration(dark, gain, defect, ped, white, pattern, bits), cr.case_reference(shape, pattern, bits, kind, which)


def _equal(a, b):
    return len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("pattern,bits", [("rggb", 12), ("mono", 8), ("rggb", 16)])
def test_ops_calibrate_and_views(pattern, bits):
    from shmgan_amd import ops, polar
    shape = (37, 66)
    src, cal, ref = _calibration(shape, pattern, bits, "half")
    host = dr.pitched(src, shape[1] + 5, np.iinfo(src.dtype).max)[0]
    wide = torch.from_numpy(host.copy()).cuda()
    m, fixed = wide[:, :shape[1]], torch.from_numpy(np.array(ref)).cuda()
    # the call on its own: from a calibration, from a layout that carries one; a new contiguous tensor, the source unwritten
    for arg in (cal, _layout(pattern, bits, calibration=cal)):
        out = ops.dofp_calibrate(m, arg)
        assert out.is_contiguous() and out.dtype == m.dtype and out.data_ptr() != m.data_ptr() and np.array_equal(out.cpu().numpy(), ref)
    assert np.array_equal(wide.cpu().numpy(), host)
    dev = torch.device("cuda", torch.cuda.current_device())
    kept = ops._DOFP_CALIBRATIONS[(cal, dev)]                      # uploaded once per (calibration, device), kept
    ops.dofp_calibrate(m, polar.DofpCalibration(cal.dark, cal.gain, cal.defect, cal.pedestal, cal.white, pattern, bits))          # an equal one
    assert ops._DOFP_CALIBRATIONS[(cal, dev)] is kept
    top = 1 << bits
    develops = [None, polar.DofpDevelop(black=top // 16, wb=(1.9, 1, 1.6) if pattern != "mono" else (1, 1, 1), tone="srgb")]
    if pattern != "mono":
        develops.append(polar.DofpDevelop(black=top // 16, wb="gray", sat=top - top // 8))
    for develop in develops:
        with_cal, without = _layout(pattern, bits, develop, cal), _layout(pattern, bits, develop)
        for mode in dr.MODES:
            for total in (False, True):
                assert _equal(ops.dofp_views(m, with_cal, mode, total), ops.dofp_views(fixed, without, mode, total)), (develop, mode, total)
        if pattern != "mono":
            for sat in (None, top // 2):
                assert _equal(ops.dofp_wb_gray(m, with_cal, sat), ops.dofp_wb_gray(fixed, without, sat)), (develop, sat)
    # the plain views against the restatements of both steps
    v, t = dr.views(ref, pattern, dr.SONY_QUAD, bits)
    out = polar.demosaic(np.array(src), _layout(pattern, bits, None, cal), total=True)
    assert all(np.array_equal(out[k].cpu().numpy(), v[k]) for k in range(4)) and np.array_equal(out[4].cpu().numpy(), t)
    # an identity calibration equals none
    ident = polar.DofpCalibration(*cr.identity_tables(shape, cal.pedestal), cal.pedestal, None, pattern, bits)
    inside = torch.from_numpy(np.minimum(src, top - 1)).cuda()
    for develop in develops:
        for mode in dr.MODES:
            assert _equal(ops.dofp_views(inside, _layout(pattern, bits, develop, ident), mode, True), ops.dofp_views(inside, _layout(pattern, bits, develop), mode, True))
    assert np.array_equal(ops.dofp_calibrate(inside, ident).cpu().numpy(), np.minimum(src, top - 1))
    # a frame of another size: both sizes, before any launch
    with pytest.raises(ValueError, match=r"dofp_views: the mosaic is 37 x 62, the calibration tables are 37 x 66"):
        ops.dofp_views(m[:, :62], _layout(pattern, bits, None, cal))
    with pytest.raises(ValueError, match=r"dofp_calibrate: the mosaic is 33 x 66, the calibration tables are 37 x 66"):
        ops.dofp_calibrate(m[:33], cal)


N_SAMPLES = 3


@pytest.fixture(scope="module", params=dr.MODES)
def capture(request, tmp_path_factory):
    """Random 12-bit RGGB mosaics of 48 x 64 in RAW/, the restatement-corrected ones in FIXED/, and the calibration saved beside them."""
    from PIL import Image
    from shmgan_amd import polar
    mode = request.param
    root = tmp_path_factory.mktemp(f"calibrate_{mode}")
    pattern, bits, shape = "rggb", 12, (48, 64)
    rng = np.random.default_rng(dr.MODES.index(mode) + 31)
    dark = rng.integers(200, 300, shape).astype(np.uint16)
    gain = rng.integers(3500, 5000, shape).astype(np.uint16)
    defect = (rng.random(shape) < 0.02).astype(np.uint8)
    dark[defect != 0] = 3000
    cal = polar.DofpCalibration(dark, gain, defect, 250, 4000, pattern, bits)
    path = str(root / "sensor.npz")
    cal.save(path)
    for d in ("RAW", "FIXED", "ED"):
        (root / d).mkdir(parents=True)
    for i in range(N_SAMPLES):
        m = rng.integers(0, 1 << bits, shape).astype(np.uint16)
        Image.fromarray(m).save(root / "RAW" / f"s{i}.png")
        Image.fromarray(cr.calibrate(m, pattern, bits, dark, gain, defect, 250, 4000)).save(root / "FIXED" / f"s{i}.png")
        Image.fromarray(rng.integers(0, 256, (shape[0] // (4 if mode == "bin" else 1), shape[1] // (4 if mode == "bin" else 1), 3)).astype(np.uint8)).save(root / "ED" / f"s{i}.png")
    args = dict(capture_format="dofp", dofp_pattern=pattern, dofp_bits=bits, dofp_demosaic=mode, dofp_black=240, dofp_wb=(1.8, 1, 1.5))
    return SimpleNamespace(root=str(root), mode=mode, path=path, cal=cal, args=args)


def _options(capture, calibrated, dofp_dir):
    """The loader keywords data.capture_options makes of the trainer's options: with the saved calibration, or without it."""
    from shmgan_amd.data import capture_options
    subdirs, kw = capture_options(SimpleNamespace(**capture.args, dofp_dir=dofp_dir, dofp_calibration=capture.path if calibrated else None))
    assert (kw["dofp"].calibration == capture.cal) if calibrated else (kw["dofp"].calibration is None)
    return subdirs, kw


def _passes(ds, passes):
    out = [[t.clone() for t in ds.batch(i, p)] for p in range(passes) for i in range(len(ds))]
    torch.cuda.synchronize()
    return out


def _same(a, b):
    return len(a) == len(b) and all(len(x) == len(y) and all(torch.equal(s, t) for s, t in zip(x, y)) for x, y in zip(a, b))


@pytest.mark.parametrize("source", ["dir", "stokes"])
def test_loader_equivalence(capture, source):
    from shmgan_amd.data import PolarDataset
    kw = dict(image_size=32, batch_size=1, rank=0, world=1, diffuse_source=source)
    sub_raw, raw = _options(capture, True, "RAW")
    sub_fix, fix = _options(capture, False, "FIXED")
    ref = _passes(PolarDataset(capture.root, subdirs=sub_fix, **fix, **kw), 1)
    assert _same(ref, _passes(PolarDataset(capture.root, subdirs=sub_raw, **raw, **kw), 1))
    assert not _same(ref, _passes(PolarDataset(capture.root, subdirs=sub_raw, **_options(capture, False, "RAW")[1], **kw), 1))          # it does something
    cached = PolarDataset(capture.root, subdirs=sub_raw, **raw, cache="device", cache_bytes=8 << 20, **kw)
    assert _same(ref + ref, _passes(cached, 2))                      # the second pass from the cache, which holds the views of the corrected frames
    stats = cached.cache_stats()
    assert stats["resident"] == N_SAMPLES and stats["hits"] == N_SAMPLES and stats["refused"] == 0


def test_mask_loader_writers_and_test_mode_equivalence(capture, tmp_path):
    from shmgan_amd import polar
    from shmgan_amd.data import EvalDataset, MaskDataset
    raw, fix = _options(capture, True, "RAW")[1], _options(capture, False, "FIXED")[1]
    mr = MaskDataset.from_polar(capture.root, 32, 2, subdirs=("RAW",), **raw)
    mf = MaskDataset.from_polar(capture.root, 32, 2, subdirs=("FIXED",), **fix)
    assert mr.names == mf.names == [f"s{i}" for i in range(N_SAMPLES)] and all(torch.equal(a, b) for a, b in zip(mr.tensors(), mf.tensors()))
    files = lambda written: [(os.path.basename(p), open(p, "rb").read()) for p in written]
    wr = polar.write_specular_masks(capture.root, str(tmp_path / "mr"), subdirs=("RAW",), **raw)
    wf = polar.write_specular_masks(capture.root, str(tmp_path / "mf"), subdirs=("FIXED",), **fix)
    assert files(wr) == files(wf) and len(wr) == N_SAMPLES
    assert open(tmp_path / "mr" / "masks.jsonl").read() == open(tmp_path / "mf" / "masks.jsonl").read()
    er = polar.write_estimated_diffuse(capture.root, str(tmp_path / "er"), subdirs=("RAW",), mode="stokes", **raw)
    ef = polar.write_estimated_diffuse(capture.root, str(tmp_path / "ef"), subdirs=("FIXED",), mode="stokes", **fix)
    assert files(er) == files(ef) and len(er) == N_SAMPLES
    ed = os.path.join(capture.root, "ED")
    for view in ("total", 2):
        tr = EvalDataset(os.path.join(capture.root, "RAW"), 32, 2, ed, keep_source=True, **dict(raw, dofp_test_view=view))
        tf = EvalDataset(os.path.join(capture.root, "FIXED"), 32, 2, ed, keep_source=True, **dict(fix, dofp_test_view=view))
        assert len(tr) == len(tf) == 2
        for (a, da), (b, db) in zip(tr, tf):
            assert torch.equal(a, b) and torch.equal(da, db)
            assert all(torch.equal(p, q) for p, q in zip(tr.last_source[0], tf.last_source[0]))
    # a frame of another size is refused by file name and both sizes before anything is launched
    from PIL import Image
    os.makedirs(tmp_path / "cap" / "RAW")
    Image.fromarray(np.zeros((48, 60), dtype=np.uint16)).save(tmp_path / "cap" / "RAW" / "s0.png")
    with pytest.raises(ValueError, match=r"s0\.png is 48 x 60, the layout's calibration tables are 48 x 64"):
        polar.write_specular_masks(str(tmp_path / "cap"), str(tmp_path / "out"), subdirs=("RAW",), **raw)


@pytest.mark.parametrize("pattern", ["mono", "rggb"])
def test_hot_photosites_on_the_device(pattern):
    """The flat, unpolarised frame with two hot samples: its specular mask is not empty, and empty once the sites are in the defect map."""
    from shmgan_amd import polar
    clean, hot, defect = cr.hot_frame()
    cal = polar.DofpCalibration(defect=defect, pattern=pattern, bits=12)

    def count(layout):
        mask, q, stats = polar.specular_mask(polar.demosaic(hot, layout), layout.angles)
        return int(stats.cpu()[2]), int((mask > 0).sum()), int(q.max())
    n, set_pixels, strength = count(_layout(pattern, 12))
    assert n == set_pixels > 0 and strength == 180
    assert count(_layout(pattern, 12, None, cal)) == (0, 0, 0)
    assert torch.equal(polar.demosaic(hot, _layout(pattern, 12, None, cal))[0], polar.demosaic(clean, _layout(pattern, 12))[0])
