"""Sensor calibration of polariser-mosaic frames without a GPU: the restatement of shm_dofp_calibrate (tests/calibrate_ref.py) against a
per-photosite brute force in Python integers, its properties, the modelled faults its comparison catches, polar.build_calibration on a
noise-free synthetic sensor, the motivating case (a hot photosite read as a highlight), and every refusal by name -- the entry point's
SHM_E_SHAPE returns included, which are made before any launch.  Every comparison is an equality."""
import ctypes as C
import os
from types import SimpleNamespace

import numpy as np
import pytest

import calibrate_ref as cr
import dofp_ref as dr
import specmask_ref as sm


# ---- the restatement ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,pattern", [(s, p) for s in cr.SMALL for p in cr.PATTERNS], ids=str)
def test_restatement_against_brute_force(shape, pattern):
    for bits in cr.BITS:
        for kind in cr.kinds_of(bits):
            src, _, _, _, ped, white = cr.case(shape, pattern, bits, kind)
            for which in cr.TABLES:
                dark, gain, defect = cr.case_tables(shape, pattern, bits, kind, which)
                ref = cr.case_reference(shape, pattern, bits, kind, which)
                assert ref.dtype == src.dtype
                assert np.array_equal(ref, cr.brute(src, pattern, bits, dark, gain, defect, ped, white)), (bits, kind, which)


def test_identity_tables_reproduce_the_input():
    for shape, pattern, bits, kind in cr.all_cases():
        src, _, _, _, ped, _ = cr.case(shape, pattern, bits, kind)
        maxv = (1 << bits) - 1
        inside = src <= maxv
        for white in (None, 65536):
            for tables in ((None, None, None), cr.identity_tables(src.shape, ped)):
                out = cr.calibrate(src, pattern, bits, *tables, pedestal=ped, white=white)
                assert np.array_equal(out[inside], src[inside])
                # above the range: passed through below the default white level, clamped when nothing counts as saturated
                assert np.array_equal(out[~inside], src[~inside] if white is None else np.full(int((~inside).sum()), maxv))


def test_saturated_samples_pass_through():
    for shape, pattern in (((13, 18), "mono"), ((37, 66), "rggb")):
        for bits in cr.BITS:
            for kind in ("random",) + (("over",) if bits == 12 else ()):
                src, dark, gain, _, ped, white = cr.case(shape, pattern, bits, kind)
                out = cr.calibrate(src, pattern, bits, dark, gain, None, ped, white)
                sat = src >= white
                assert sat.any() and (~sat).any() and np.array_equal(out[sat], src[sat])
                assert not np.array_equal(out[~sat], src[~sat])
                if kind == "over":
                    assert (src > 4095).any() and np.array_equal(out[src > 4095], src[src > 4095])          # uint16 values above maxv at bits = 12


def test_every_neighbour_count_occurs():
    seen = set()
    for shape, pattern, bits, kind in cr.all_cases():
        defect = cr.case(shape, pattern, bits, kind)[3]
        n = cr.neighbour_counts(defect, dr.period(pattern))
        seen |= set(n[defect != 0].tolist())
        if shape == "period":
            assert not n.any()                      # P x P: every neighbour is outside
    assert seen == {0, 1, 2, 3, 4}
    # ... and inside one shape, so that a single GPU case meets them all
    defect = cr.case((37, 66), "rggb", 12, "half")[3]
    assert set(cr.neighbour_counts(defect, 4)[defect != 0].tolist()) == {0, 1, 2, 3, 4}


def test_case_table_meets_what_the_kernel_branches_on():
    shapes = [cr.shape_of(s, p) for s in cr.SHAPES for p in cr.PATTERNS]
    assert (2, 2) in shapes and (4, 4) in shapes and {(5, 7), (13, 18), (37, 66), (20, 40)} <= set(shapes)
    assert any(w % cr.PER_THREAD for _, w in shapes) and any(w % cr.PER_THREAD == 0 for _, w in shapes)
    per_block = 64 * cr.PER_THREAD
    for h, w in (cr.MULTI_BLOCK, cr.MULTI_BLOCK_RAGGED):
        assert w > per_block and h > 4                      # more than one block along both axes of the 64 x 4 launch
    assert cr.MULTI_BLOCK[1] % cr.PER_THREAD == 0 and cr.MULTI_BLOCK_RAGGED[1] % cr.PER_THREAD
    assert len(cr.TABLES) == 8 and len(set(cr.TABLES)) == 8
    for shape in ((20, 40), (13, 18)):
        assert (shape[1] + cr.pitch_extra(shape[1])) % cr.PER_THREAD == 0 and cr.pitch_extra(shape[1]) > 0


# ---- modelled faults: equality with the restatement catches each ----------------------------------------------------------------------------
@pytest.mark.parametrize("fault", [f for f in cr.FAULTS if f != "pitch_w"])
def test_modelled_fault_is_caught(fault):
    caught = 0
    for shape, pattern, bits, kind in cr.all_cases(cr.SHAPES[:5]):
        src, dark, gain, defect, ped, white = cr.case(shape, pattern, bits, kind)
        got = cr.calibrate(src, pattern, bits, dark, gain, defect, ped, white, fault=fault)
        hit = not np.array_equal(got, cr.case_reference(shape, pattern, bits, kind, (True, True, True)))
        caught += hit
        if fault == "lattice2" and pattern == "mono":
            assert not hit                                    # a step of 2 is right for a mono sensor: the fault is a Bayer pattern's
        elif shape == (37, 66) and kind == "half":
            assert hit, (pattern, bits)                       # this case shows every fault on its own
    assert caught


def test_pitch_fault_is_caught():
    for pattern in cr.PATTERNS:
        shape = (13, 18)
        src, dark, gain, defect, ped, white = cr.case(shape, pattern, 12, "random")
        buf, view = dr.pitched(src, shape[1] + cr.pitch_extra(shape[1]), np.iinfo(src.dtype).max)
        assert np.array_equal(view, src)
        got = cr.calibrate(dr.read_with_pitch_w(buf, *shape), pattern, 12, dark, gain, defect, ped, white)
        assert not np.array_equal(got, cr.case_reference(shape, pattern, 12, "random", (True, True, True)))


# ---- the builder ----------------------------------------------------------------------------------------------------------------------------
def _write_stack(directory, frames):
    from PIL import Image
    os.makedirs(directory)
    for i, f in enumerate(frames):
        Image.fromarray(f).save(os.path.join(directory, f"f{i:02d}.png"))


@pytest.mark.parametrize("pattern", ["mono", "rggb", "gbrg"])
@pytest.mark.parametrize("bits", [8, 12, 16])
def test_builder_on_a_synthetic_sensor(tmp_path, pattern, bits):
    from shmgan_amd import polar
    darks, flats, model, planted = cr.sensor(pattern, bits)
    _write_stack(tmp_path / "dark", darks)
    _write_stack(tmp_path / "flat", flats)
    lay = polar.DofpLayout(pattern, bits=bits)
    cal = polar.build_calibration(lay, tmp_path / "dark", tmp_path / "flat")
    ref = cr.build(darks, flats, pattern, bits)
    assert (cal.pattern, cal.bits, cal.shape, cal.pedestal, cal.white) == (pattern, bits, cr.SENSOR_SHAPE, ref["pedestal"], None)
    assert np.array_equal(cal.dark, model) and np.array_equal(cal.dark, ref["dark"])                     # the model's dark, exactly
    assert np.array_equal(cal.defect != 0, planted)                                                      # the planted set, exactly
    assert np.array_equal(cal.defect, ref["defect"]) and np.array_equal(cal.gain, ref["gain"]) and cal.reference == ref["reference"]
    assert len(cal.reference) == (1 if pattern == "mono" else 3)
    for group, flag in (("hot", cr.HOT), ("dead", cr.UNUSABLE), ("stuck", cr.HOT | cr.UNUSABLE), ("weak", cr.RANGE)):
        for p in cr.PLANTED[group]:
            assert cal.defect[p] & flag == flag, (group, p, int(cal.defect[p]))
    s = cal.summary()
    assert (s["hot"], s["out_of_range"], s["defective"], s["sites"]) == (len(cr.PLANTED["hot"]) + 1, 1, int(planted.sum()), model.size)
    assert s["unusable"] == len(cr.PLANTED["hot"]) + 1 + len(cr.PLANTED["dead"]) and 2048 <= s["gain_min"] < 4096 < s["gain_max"] <= 8192
    assert bool((cal.gain[planted] == 4096).all())
    # the calibrated flat: |dst - pedestal - S_c / n_c| <= f / 8192 + 1/2 on every good site (g is within 1/2 of the real gain, then one
    # rounding), checked in integers after multiplying by 8192 n_c
    fm = cr.stack_mean(flats)
    dst = cr.calibrate(fm.astype(flats[0].dtype), pattern, bits, cal.dark, cal.gain, cal.defect, cal.pedestal, cal.white_level).astype(np.int64)
    f = fm - model
    chan = cr.channels(pattern, *cr.SENSOR_SHAPE)
    for c, (S, n) in enumerate(cal.reference):
        sel = ~planted & (chan == c)
        assert sel.any()
        excess = np.abs(8192 * n * (dst[sel] - cal.pedestal) - 8192 * S) - (n * f[sel] + 4096 * n)
        assert int(excess.max()) <= 0, (c, int(excess.max()))
    # the four orientations of a colour come out equal within that bound although their responses differ by 3 %: the spread of the raw flat
    # inside a quad is far above it
    raw_spread = int(np.abs(f[0:-1:2, 0:-1:2] - f[0:-1:2, 1::2])[~planted[0:-1:2, 0:-1:2] & ~planted[0:-1:2, 1::2]].max())
    assert raw_spread > 3 * (int(f.max()) // 8192 + 1)
    # a defective site of the calibrated flat takes its good neighbours' level
    for p in cr.PLANTED["dead"] + cr.PLANTED["stuck"]:
        S, n = cal.reference[int(chan[p])]
        assert abs(int(dst[p]) - cal.pedestal - S // n) <= int(f.max()) // 8192 + 2


def test_builder_without_flats_and_its_refusals(tmp_path):
    from shmgan_amd import polar
    darks, flats, model, planted = cr.sensor("rggb", 12)
    _write_stack(tmp_path / "dark", darks)
    lay = polar.DofpLayout("rggb", bits=12)
    cal = polar.build_calibration(lay, tmp_path / "dark")
    ref = cr.build(darks, None, "rggb", 12)
    assert cal.gain is None and cal.reference is None and np.array_equal(cal.dark, model) and np.array_equal(cal.defect, ref["defect"])
    hot = np.zeros_like(planted)
    for p in cr.PLANTED["hot"] + cr.PLANTED["stuck"]:
        hot[p] = True
    assert np.array_equal(cal.defect != 0, hot) and cal.summary()["gain_min"] == cal.summary()["gain_max"] == 4096
    # a higher threshold keeps the hot sites (40 byte units) out; a layout that carries a calibration of another size still builds a new one
    assert not polar.build_calibration(lay, tmp_path / "dark", hot_threshold=41 << 4).defect[8, 8]
    small = polar.DofpCalibration(defect=np.zeros((8, 8), dtype=np.uint8), pattern="rggb", bits=12)
    assert polar.build_calibration(polar.DofpLayout("rggb", bits=12, calibration=small), tmp_path / "dark") == cal
    os.makedirs(tmp_path / "empty")
    with pytest.raises(ValueError, match=r"build_calibration: no dark frames in .*empty"):
        polar.build_calibration(lay, tmp_path / "empty")
    with pytest.raises(ValueError, match=r"build_calibration: no flat frames in .*empty"):
        polar.build_calibration(lay, tmp_path / "dark", tmp_path / "empty")
    _write_stack(tmp_path / "mixed", [darks[0], darks[1][:, :-4]])
    with pytest.raises(ValueError, match=r"f01\.png is 24 x 28, the frames before it are 24 x 32"):
        polar.build_calibration(lay, tmp_path / "mixed")
    _write_stack(tmp_path / "flat_small", [flats[0][:-4]])
    with pytest.raises(ValueError, match=r"flat_small.*f00\.png is 20 x 32"):
        polar.build_calibration(lay, tmp_path / "dark", tmp_path / "flat_small")
    _write_stack(tmp_path / "flat_dark", darks)          # flats that are no brighter than the darks: no usable site of any colour
    with pytest.raises(ValueError, match=r"build_calibration: no usable R site in the flat frames of .*flat_dark"):
        polar.build_calibration(lay, tmp_path / "dark", tmp_path / "flat_dark")
    for bad in ((0.1, 2.0), (0.5, 4.5), (1.5, 2.0), "ab"):
        with pytest.raises(ValueError, match="build_calibration: gain_limits"):
            polar.build_calibration(lay, tmp_path / "dark", gain_limits=bad)
    with pytest.raises(ValueError, match="build_calibration: layout"):
        polar.build_calibration("rggb", tmp_path / "dark")
    assert "UNPOLARISED, UNIFORM" in polar.build_calibration.__doc__


# ---- the motivating case --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pattern", ["mono", "rggb"])
def test_hot_photosites_are_not_highlights_once_calibrated(pattern):
    from shmgan_amd.polar import stokes_matrix
    clean, hot, defect = cr.hot_frame()
    coef = stokes_matrix([0, 45, 90, 135])

    def mask_count(mosaic):
        views = dr.views(mosaic, pattern, dr.SONY_QUAD, 12)[0]
        mask, q, _ = sm.pipeline(list(views), coef)
        return int((mask > 0).sum()), int(q.max())
    assert mask_count(clean) == (0, 0)
    count, strength = mask_count(hot)
    assert count > 0 and strength == 180                      # a "specular mask" where nothing is specular: first, so the rest is not vacuous
    fixed = cr.calibrate(hot, pattern, 12, None, None, defect, 0, None)
    assert np.array_equal(fixed, clean) and mask_count(fixed) == (0, 0)


# ---- the calibration object, the layout, the options ----------------------------------------------------------------------------------------
def _tables(shape=(8, 12)):
    rng = np.random.default_rng(5)
    return (rng.integers(200, 300, shape).astype(np.uint16), rng.integers(3000, 6000, shape).astype(np.uint16),
            (rng.random(shape) < 0.1).astype(np.uint8))


def test_calibration_equality_hash_and_round_trip(tmp_path):
    from shmgan_amd.polar import DofpCalibration, DofpLayout
    dark, gain, defect = _tables()
    a = DofpCalibration(dark, gain, defect, pedestal=250, white=4000, pattern="rggb", bits=12, reference=[(10, 2), (30, 4), (5, 1)])
    b = DofpCalibration(dark.copy(), gain.copy(), defect.copy(), 250, 4000, "rggb", 12, ((10, 2), (30, 4), (5, 1)))
    assert a == b and hash(a) == hash(b) and a.digest == b.digest and {a: 1}[b] == 1 and a != "x"
    assert (a.shape, a.period, a.white_level, a.reference) == ((8, 12), 4, 4000, ((10, 2), (30, 4), (5, 1)))
    assert DofpCalibration(pattern="mono", bits=10).white_level == 1023 and DofpCalibration().shape is None
    changed = gain.copy()
    changed[3, 3] += 1
    for other in (DofpCalibration(dark, changed, defect, 250, 4000, "rggb", 12), DofpCalibration(dark, gain, defect, 251, 4000, "rggb", 12),
                  DofpCalibration(dark, gain, None, 250, 4000, "rggb", 12), DofpCalibration(dark, gain, defect, 250, None, "rggb", 12),
                  DofpCalibration(dark, gain, defect, 250, 4000, "bggr", 12), DofpCalibration(dark, gain, defect, 250, 4000, "rggb", 14)):
        assert other != a and other.digest != a.digest
    # the arrays are copies and read-only, the object is frozen
    dark[0, 0] += 1
    assert a.dark[0, 0] == b.dark[0, 0] and not a.dark.flags.writeable and not a.gain.flags.writeable and not a.defect.flags.writeable
    with pytest.raises(ValueError):
        a.gain[0, 0] = 4096
    with pytest.raises(AttributeError, match="read-only"):
        a.pedestal = 3
    # save / load: an .npz without pickle; two loads of one file are equal, to each other and to the original
    path = tmp_path / "cal.npz"
    a.save(path)
    with np.load(path, allow_pickle=False) as z:
        assert {"dark", "gain", "defect", "pedestal", "white", "pattern", "bits", "reference"} == set(z.files)
    l1, l2 = DofpCalibration.load(path), DofpCalibration.load(str(path))
    assert l1 == l2 == a and hash(l1) == hash(a) and l1.reference == a.reference and np.array_equal(l1.gain, a.gain)
    sparse = DofpCalibration(defect=defect, pattern="mono", bits=8)
    sparse.save(tmp_path / "sparse.npz")
    back = DofpCalibration.load(tmp_path / "sparse.npz")
    assert back == sparse and back.dark is None and back.gain is None and back.white is None and back.reference is None
    # a layout with a calibration stays hashable and compares by content
    lay = DofpLayout("rggb", bits=12, calibration=a)
    assert lay == DofpLayout("rggb", bits=12, calibration=l1) and hash(lay) == hash(DofpLayout("rggb", bits=12, calibration=l2))
    assert lay != DofpLayout("rggb", bits=12) and {lay: 1}[DofpLayout("rggb", bits=12, calibration=b)] == 1
    assert DofpLayout("rggb", bits=12) == DofpLayout("rggb", (90, 45, 135, 0), 12, None, None) and DofpLayout().calibration is None
    np.savez(tmp_path / "other.npz", x=np.zeros(3))
    with pytest.raises(ValueError, match=r"DofpCalibration: .*other\.npz is not a saved calibration"):
        DofpCalibration.load(tmp_path / "other.npz")
    with pytest.raises(ValueError, match=r"DofpCalibration: .*missing\.npz is not a saved calibration"):
        DofpCalibration.load(tmp_path / "missing.npz")


def test_calibration_refuses_by_name():
    from shmgan_amd.polar import DofpCalibration
    dark, gain, defect = _tables()
    low, high = gain.copy(), gain.copy()
    low[0, 0], high[1, 1] = 1023, 16384
    for kw, msg in [(dict(dark=dark.astype(np.int32)), "dark must be a uint16 array, got int32"), (dict(gain=gain.astype(np.float32)), "gain must be a uint16 array"),
                    (dict(defect=defect.astype(bool)), "defect must be a uint8 array, got bool"), (dict(dark=[[1, 2]]), "dark must be a uint16 array, got list"),
                    (dict(dark=dark, gain=gain[:, :-1]), r"gain has shape \(8, 11\), the other tables have \(8, 12\)"),
                    (dict(dark=dark, defect=defect[:-1]), r"defect has shape \(7, 12\)"), (dict(dark=dark.reshape(-1)), r"dark has shape \(96,\), the tables are 2-D"),
                    (dict(gain=low), r"gain spans \[1023, .*outside the Q12 range \[1024, 16383\]"), (dict(gain=high), r"gain spans .*16384\]"),
                    (dict(pedestal=-1), "pedestal -1"), (dict(pedestal=65520), "pedestal 65520"), (dict(pedestal=1.5), "pedestal 1.5"),
                    (dict(pedestal=True), "pedestal True"), (dict(white=0), "white 0"), (dict(white=65537), "white 65537"), (dict(white="x"), "white 'x'"),
                    (dict(pattern="rgbg"), "pattern 'rgbg'"), (dict(bits=7), "bits 7"), (dict(bits=17), "bits 17"), (dict(bits=True), "bits True"),
                    (dict(reference=[(1, 2)], pattern="rggb"), "reference"), (dict(reference=3), "reference")]:
        with pytest.raises(ValueError, match="DofpCalibration: " + msg):
            DofpCalibration(**kw)
    assert DofpCalibration(pedestal=65519, white=65536).white_level == 65536 and DofpCalibration(white=1).white == 1


def test_layout_and_decode_refusals(tmp_path):
    from PIL import Image
    from shmgan_amd.polar import DofpCalibration, DofpLayout, decode_mosaic
    cal = DofpCalibration(defect=np.zeros((8, 12), dtype=np.uint8), pattern="rggb", bits=12)
    with pytest.raises(ValueError, match="DofpLayout: calibration is of pattern 'rggb', the layout is 'bggr'"):
        DofpLayout("bggr", bits=12, calibration=cal)
    with pytest.raises(ValueError, match="DofpLayout: calibration is of bits = 12, the layout says bits = 10"):
        DofpLayout("rggb", bits=10, calibration=cal)
    with pytest.raises(ValueError, match="DofpLayout: calibration .* is not a polar.DofpCalibration or None"):
        DofpLayout("rggb", bits=12, calibration="cal.npz")
    lay = DofpLayout("rggb", bits=12, calibration=cal)
    Image.fromarray(np.zeros((8, 12), dtype=np.uint16)).save(tmp_path / "fits.png")
    Image.fromarray(np.zeros((8, 16), dtype=np.uint16)).save(tmp_path / "wide.png")
    assert decode_mosaic(tmp_path / "fits.png", lay).shape == (8, 12)
    with pytest.raises(ValueError, match=r"wide\.png is 8 x 16, the layout's calibration tables are 8 x 12"):          # the file and both sizes
        decode_mosaic(tmp_path / "wide.png", lay)
    assert decode_mosaic(tmp_path / "wide.png", DofpLayout("rggb", bits=12)).shape == (8, 16)


def test_trainer_options(tmp_path):
    from shmgan_amd import data
    from shmgan_amd.polar import DofpCalibration, DofpLayout
    from shmgan_amd.trainer import _DEFAULTS
    assert _DEFAULTS["dofp_calibration"] is None
    assert data.CALIBRATION_OPTIONS == ("dofp_calibration",) and data.CAPTURE_OPTIONS[-1:] == data.CALIBRATION_OPTIONS
    assert set(data.DEVELOP_OPTIONS) < set(data.CAPTURE_OPTIONS) and all(k in _DEFAULTS for k in data.CAPTURE_OPTIONS)
    dark, gain, defect = _tables()
    cal = DofpCalibration(dark, gain, defect, 250, None, "rggb", 12)
    path = str(tmp_path / "cal.npz")
    cal.save(path)
    base = dict(capture_format="dofp", dofp_pattern="rggb", dofp_bits=12)
    # None: today's layout and exactly the three keys
    subdirs, kw = data.capture_options(SimpleNamespace(**base, dofp_calibration=None))
    assert kw == dict(capture="dofp", dofp=DofpLayout("rggb", (90, 45, 135, 0), 12), dofp_demosaic="bilinear") and kw["dofp"].calibration is None
    for given in (path, tmp_path / "cal.npz", cal):
        subdirs, kw = data.capture_options(SimpleNamespace(**base, dofp_calibration=given, dofp_black=240))
        assert sorted(kw) == ["capture", "dofp", "dofp_demosaic"] and subdirs == ("DOFP", "ED")
        assert kw["dofp"].calibration == cal and kw["dofp"].develop.black == (240, 240, 240)
    with pytest.raises(ValueError, match="dofp_calibration .* needs capture_format 'dofp', got 'views'"):
        data.capture_options(SimpleNamespace(dofp_calibration=path))
    with pytest.raises(ValueError, match="dofp_calibration is of pattern 'rggb', the layout is 'mono'"):
        data.capture_options(SimpleNamespace(capture_format="dofp", dofp_bits=12, dofp_calibration=path))
    with pytest.raises(ValueError, match="dofp_calibration is of bits = 12, the layout says bits = 16"):
        data.capture_options(SimpleNamespace(**dict(base, dofp_bits=16), dofp_calibration=path))
    with pytest.raises(ValueError, match=r"dofp_calibration: .*nothing\.npz is not a saved calibration"):
        data.capture_options(SimpleNamespace(**base, dofp_calibration=str(tmp_path / "nothing.npz")))
    with pytest.raises(ValueError, match="dofp_calibration 7 is not the path"):
        data.capture_options(SimpleNamespace(**base, dofp_calibration=7))


def test_ops_refusals_without_a_device():
    """What ops.dofp_calibrate refuses before it touches the device."""
    import torch
    from shmgan_amd import ops
    from shmgan_amd.polar import DofpCalibration, DofpLayout
    cal = DofpCalibration(defect=np.zeros((8, 12), dtype=np.uint8), pattern="rggb", bits=12)
    with pytest.raises(TypeError, match="dofp_calibrate takes a uint8 or uint16 device tensor"):
        ops.dofp_calibrate(torch.zeros((8, 12), dtype=torch.uint16), cal)
    with pytest.raises(ValueError, match="dofp_calibrate takes a polar.DofpCalibration or a polar.DofpLayout that has one"):
        ops.dofp_calibrate(torch.zeros((8, 12), dtype=torch.uint16), DofpLayout("rggb", bits=12))
    with pytest.raises(ValueError, match="dofp_calibrate takes a polar.DofpCalibration"):
        ops.dofp_calibrate(torch.zeros((8, 12), dtype=torch.uint16), None)


# ---- the entry point's refusals: made before any launch, so they run without a GPU -----------------------------------------------------------
def test_entry_point_refusals_without_gpu():
    from shmgan_amd import _lib
    assert "dofp_calibrate.hip" in _lib.SOURCES and "shm_dofp_calibrate" in _lib.header_functions()
    I, P, Z = C.c_int, C.c_void_p, C.c_size_t
    assert _lib.SIGNATURES["shm_dofp_calibrate"] == (I, [P, I, I, I, Z, I, P, P, P, I, I, P, Z, P])
    assert (_lib.CONSTANTS["SHM_DOFP_GAIN_MIN"], _lib.CONSTANTS["SHM_DOFP_GAIN_MAX"]) == (cr.GAIN_MIN, cr.GAIN_MAX) == (1024, 16383)
    L = _lib.lib()
    src, dst = 4096, 8192          # non-null pointers nobody dereferences: every call below is refused before a launch
    good = dict(src=src, bits=12, h=8, w=12, spitch=12, pattern=1, dark=None, gain=None, defect=None, pedestal=240, white=4095, dst=dst, dpitch=12)
    call = lambda a: L.shm_dofp_calibrate(a["src"], a["bits"], a["h"], a["w"], a["spitch"], a["pattern"], a["dark"], a["gain"], a["defect"], a["pedestal"],
                                          a["white"], a["dst"], a["dpitch"], None)
    for change, word in [(dict(src=None), b"null pointer"), (dict(dst=None), b"null pointer"), (dict(bits=7), b"bits 7"), (dict(bits=17), b"bits 17"),
                         (dict(h=3), b"sizes"), (dict(w=3), b"sizes"), (dict(pattern=0, h=1), b"sizes"), (dict(h=32769), b"sizes"),
                         (dict(w=32769, spitch=40000, dpitch=40000), b"sizes"), (dict(spitch=11), b"src_pitch 11"), (dict(dpitch=11), b"dst_pitch 11"),
                         (dict(pattern=5), b"pattern 5"), (dict(pattern=-1), b"pattern -1"), (dict(dst=src), b"dst == src"),
                         (dict(pedestal=-1), b"pedestal -1"), (dict(pedestal=65520), b"pedestal 65520"), (dict(white=0), b"white 0"),
                         (dict(white=65537), b"white 65537")]:
        rc = call(dict(good, **change))
        err = L.shm_last_error()
        assert rc == _lib.CONSTANTS["SHM_E_SHAPE"] == -1 and b"shm_dofp_calibrate" in err and word in err, (change, rc, err)
