"""Exposure brackets of polariser-mosaic frames without a GPU: the restatement of shm_dofp_merge (tests/merge_ref.py) against a
per-photosite brute force in Python integers and the exact quotient, its properties, the modelled faults its comparison catches,
polar.DofpBracket / DofpLayout.merged, the options, the multi-page TIFF round trip, pack_brackets, the motivating scene, and the entry
point's SHM_E_SHAPE returns, which are made before any launch."""
import ctypes as C
import os
from fractions import Fraction
from types import SimpleNamespace

import numpy as np
import pytest

import dofp_ref as dr
import merge_ref as mr
import specmask_ref as sm


# ---- the restatement ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", mr.SMALL, ids=str)
def test_restatement_against_brute_force_and_the_exact_quotient(shape):
    worst = Fraction(0)
    for _, bits, exposures, kind in mr.all_cases((shape,)):
        pages, black, white = mr.case(shape, bits, exposures, kind)
        ref, cnt = mr.case_reference(shape, bits, exposures, kind)
        got, exact = mr.brute(pages, exposures, bits, black, white)
        assert ref.dtype == np.uint16 and np.array_equal(ref, got), (bits, exposures, kind)
        err = max(abs(Fraction(int(r)) - e) for r, e in zip(ref.ravel(), exact.ravel()))
        assert err <= Fraction(3, 4), (bits, exposures, kind, float(err))          # 1/2 from the rounding, at most 1/4 from mul
        worst = max(worst, err)
        assert int(cnt.sum()) == ref.size
    print("largest distance from the exact quotient:", float(worst))


def test_table():
    for bits in mr.BITS:
        f = 16 - bits
        for exposures in mr.BRACKETS:
            t = mr.table(exposures, bits)
            n = len(exposures)
            assert t.dtype == np.uint32 and t.shape == (256,) and t[0] == 0 and not t[1 << n:].any()
            assert all(1 <= int(v) <= 1 << (f + 20) for v in t[1:1 << n])
            for m in range(1, 1 << n):
                T = sum(e for k, e in enumerate(exposures) if m >> k & 1)
                assert abs(Fraction(int(t[m])) - Fraction(min(exposures) << (f + 20), T)) <= Fraction(1, 2)
            # a common factor of the exposures changes nothing
            assert np.array_equal(t, mr.table(tuple(5 * e for e in exposures), bits))
        assert int(mr.table((3, 7), bits)[1]) == 1 << (f + 20)                      # the shortest page alone: the factor is 2^f exactly


def test_properties():
    for shape, bits, exposures, kind in mr.all_cases():
        pages, black, white = mr.case(shape, bits, exposures, kind)
        ref, cnt = mr.case_reference(shape, bits, exposures, kind)
        f = 16 - bits
        m = mr.masks(pages, white)
        short = int(np.argmin(exposures))
        only = m == 1 << short
        assert np.array_equal(ref[only], pages[short][only].astype(np.int64) << f)          # valid in the shortest page only: exactly v << f
        assert (ref[m != 0] < (white << f)).all()                                         # a valid site is strictly below white << f
        assert (ref[m == 0] == min(65535, white << f)).all()
        assert int(cnt.sum()) == ref.size and int(cnt[0]) == int((m == 0).sum()) and not cnt[len(exposures) + 1:].any()
    # equal pages of equal exposure: v << f
    rng = np.random.default_rng(5)
    for bits in mr.BITS:
        black, white = mr.levels_of(bits)
        v = rng.integers(0, white, (9, 17)).astype(np.uint16 if bits > 8 else np.uint8)
        for n in (2, 3, 8):
            assert np.array_equal(mr.merge(np.stack([v] * n), (9,) * n, bits, black, white), v.astype(np.int64) << (16 - bits))
        # white = 2^bits: nothing is saturated, every site has all pages
        top = rng.integers(0, 1 << bits, (2, 9, 17))
        assert mr.counts(top, 1 << bits)[2] == 9 * 17


def test_every_mask_and_every_count_occurs():
    for shape, bits, exposures, kind in mr.all_cases():
        pages, _, white = mr.case(shape, bits, exposures, kind)
        n = len(exposures)
        h, w = mr.shape_of(shape)
        if h * w >= 1 << n:
            assert set(np.unique(mr.masks(pages, white)).tolist()) == set(range(1 << n)), (shape, bits, exposures, kind)
            assert (mr.case_reference(shape, bits, exposures, kind)[1][:n + 1] > 0).all()
    shapes = [mr.shape_of(s) for s in mr.SHAPES]
    assert (1, 1) in shapes and any(h * w >= 256 for h, w in shapes)
    assert any(w % mr.PER_THREAD for _, w in shapes) and any(w % mr.PER_THREAD == 0 for _, w in shapes)
    assert sum(w > 64 * mr.PER_THREAD and h > 4 for h, w in shapes) == 2                  # more than one block along both axes of the launch


# ---- modelled faults: equality with the restatement catches each in every case it can touch ---------------------------------------------------
def _touches(fault, pages, exposures, bits, black, white):
    """Whether the fault's precondition holds somewhere in the case (the reason a case may be out of its reach is the comment)."""
    v = pages.astype(np.int64)
    n = len(exposures)
    m = mr.masks(v, white)
    if fault == "sat_in":                   # needs a saturated sample
        return bool((v >= white).any())
    if fault == "equal_weights":            # needs a site with two valid pages (the exposures of every bracket differ)
        return bool(((v < white).sum(axis=0) >= 2).any())
    if fault == "black_kept":               # needs a valid site other than "the shortest page alone", whose factor 2^f scales black like the shift
        return bool(((m != 0) & (m != 1 << int(np.argmin(exposures)))).any())
    if fault == "mask_reversed":            # needs a mask whose mirror image selects another sum of exposures
        T = lambda mm: sum(e for k, e in enumerate(exposures) if mm >> k & 1)
        rev = lambda mm: sum(1 << (n - 1 - k) for k in range(n) if mm >> k & 1)
        return any(mm and T(mm) != T(rev(mm)) for mm in np.unique(m).tolist())
    if fault == "truncate":                 # needs an unclamped site whose fraction is at least a half
        E = np.where(v < white, v - black, 0).sum(axis=0)
        prod = E * mr.table(exposures, bits).astype(np.int64)[m]
        r = (black << (16 - bits)) + (prod >> 20)
        return bool(((m != 0) & ((prod & ((1 << 20) - 1)) >= 1 << 19) & (r >= 0) & (r < 65535)).any())
    if fault == "allsat_zero":              # needs a site clipped in every page
        return bool((m == 0).any())
    if fault == "page0":                    # needs a page that differs from page 0
        return bool((v[1:] != v[:1]).any())
    raise AssertionError(fault)


@pytest.mark.parametrize("fault", [f for f in mr.FAULTS if f != "pitch_w"])
def test_modelled_fault_is_caught(fault):
    touched = 0
    for shape, bits, exposures, kind in mr.all_cases():
        pages, black, white = mr.case(shape, bits, exposures, kind)
        got = mr.merge(pages, exposures, bits, black, white, fault=fault)
        if _touches(fault, pages, exposures, bits, black, white):
            touched += 1
            assert not np.array_equal(got, mr.case_reference(shape, bits, exposures, kind)[0]), (shape, bits, exposures, kind)
        if mr.shape_of(shape)[0] * mr.shape_of(shape)[1] >= 256:
            assert _touches(fault, pages, exposures, bits, black, white), (shape, bits, exposures, kind)          # the larger shapes meet every fault
    assert touched > len(mr.all_cases()) // 2


def test_pitch_fault_is_caught():
    for shape, bits, exposures, kind in mr.all_cases():
        h, w = mr.shape_of(shape)
        if h == 1:
            continue                        # one row: the pitch is never used
        pages, black, white = mr.case(shape, bits, exposures, kind)
        read = np.stack([dr.read_with_pitch_w(dr.pitched(p, w + mr.pitch_extra(w), np.iinfo(p.dtype).max)[0], h, w) for p in pages])
        assert not np.array_equal(mr.merge(read, exposures, bits, black, white), mr.case_reference(shape, bits, exposures, kind)[0])


# ---- polar.DofpBracket, DofpLayout.merged ---------------------------------------------------------------------------------------------------
def test_bracket_and_layout():
    from shmgan_amd import polar
    for exposures in mr.BRACKETS:
        b = polar.DofpBracket(exposures)
        for bits in mr.BITS:
            t = b.table(bits)
            assert np.array_equal(t, mr.table(exposures, bits)) and t.dtype == np.uint32 and not t.flags.writeable and b.table(bits) is t
    a, b = polar.DofpBracket([1, 4, 16], 64, 4000), polar.DofpBracket((1, 4, 16), black=64, white=4000)
    assert a == b and hash(a) == hash(b) and a != polar.DofpBracket((1, 4, 16)) and a.pages == 3 and a.exposures == (1, 4, 16)
    with pytest.raises(Exception):
        a.black = 3
    for bad, what in (((1,), "exposures"), ((1,) * 9, "exposures"), ((1, 0), "exposures"), ((1, 65536), "exposures"), ((1, 2.5), "exposures"),
                      ("12", "exposures"), (None, "exposures"), ((True, 2), "exposures")):
        with pytest.raises(ValueError, match=f"DofpBracket: {what}"):
            polar.DofpBracket(bad)
    for kw, what in ((dict(black=-1), "black"), (dict(black=65520), "black"), (dict(white=0), "white"), (dict(white=65537), "white"),
                     (dict(black="3"), "black"), (dict(black=10, white=10), "white")):
        with pytest.raises(ValueError, match=f"DofpBracket: {what}"):
            polar.DofpBracket((1, 2), **kw)
    # layouts without a bracket compare and hash as before; the bracket is the sixth field
    plain = polar.DofpLayout("rggb", bits=12)
    assert plain == polar.DofpLayout("rggb", (90, 45, 135, 0), 12, None, None, None) and hash(plain) == hash(polar.DofpLayout("rggb", bits=12))
    assert plain.bracket is None and plain.merged is plain
    lay = polar.DofpLayout("rggb", bits=12, bracket=a)
    assert lay != plain and lay == polar.DofpLayout("rggb", bits=12, bracket=b) and hash(lay) == hash(polar.DofpLayout("rggb", bits=12, bracket=b))
    assert lay.bracket_levels == (64, 4000)
    assert lay.merged == polar.DofpLayout("rggb", bits=16) and lay.merged.quad == lay.quad
    # the defaults of the levels: the calibration's, else 0 and 2^bits - 1
    cal = polar.DofpCalibration(pedestal=100, white=3900, pattern="rggb", bits=12)
    assert polar.DofpLayout("rggb", bits=12, bracket=polar.DofpBracket((1, 2))).bracket_levels == (0, 4095)
    assert polar.DofpLayout("rggb", bits=12, calibration=cal, bracket=polar.DofpBracket((1, 2))).bracket_levels == (100, 3900)
    assert polar.DofpLayout("rggb", bits=12, calibration=cal, bracket=polar.DofpBracket((1, 2), 90)).bracket_levels == (90, 3900)
    assert polar.DofpLayout("rggb", bits=12, calibration=cal, bracket=a).merged.calibration is None
    # the development moves onto the merged scale
    dev = polar.DofpDevelop(black=(60, 64, 68), wb=(2, 1, 1.5), tone="linear", sat=3500)
    md = polar.DofpLayout("rggb", bits=12, develop=dev, bracket=a).merged.develop
    assert md == polar.DofpDevelop(black=(960, 1024, 1088), white=64000, wb=(2, 1, 1.5), tone="linear", sat=56000)
    md = polar.DofpLayout("rggb", bits=12, develop=polar.DofpDevelop(black=64, white=4090), bracket=a).merged.develop
    assert md.white == 65440 and md.sat is None
    md = polar.DofpLayout("mono", bits=8, develop=polar.DofpDevelop(black=3, sat=256), bracket=polar.DofpBracket((1, 2))).merged.develop
    assert md.black == (768, 768, 768) and md.white == 65280 and md.sat == 65536
    md = polar.DofpLayout("mono", bits=16, develop=polar.DofpDevelop(black=300), bracket=polar.DofpBracket((1, 2))).merged.develop
    assert md.black == (300, 300, 300) and md.white == 65535
    # refusals when the layout is built, by name
    with pytest.raises(ValueError, match=r"DofpLayout: bracket black 4095 << 4 is above 65519"):
        polar.DofpLayout("mono", bits=12, bracket=polar.DofpBracket((1, 2), black=4095, white=4096))
    with pytest.raises(ValueError, match=r"DofpLayout: develop black .* << 4 is above 65519"):
        polar.DofpLayout("mono", bits=12, develop=polar.DofpDevelop(black=4095, white=5000), bracket=polar.DofpBracket((1, 2)))
    with pytest.raises(ValueError, match=r"DofpLayout: bracket white 4097 outside \[1, 4096\]"):
        polar.DofpLayout("mono", bits=12, bracket=polar.DofpBracket((1, 2), white=4097))
    with pytest.raises(ValueError, match=r"DofpLayout: bracket white 100 is not above black 100"):
        polar.DofpLayout("mono", bits=12, calibration=polar.DofpCalibration(pedestal=100, bits=12), bracket=polar.DofpBracket((1, 2), white=100))
    with pytest.raises(ValueError, match=r"DofpLayout: bracket .* is not a polar.DofpBracket"):
        polar.DofpLayout("mono", bits=12, bracket=(1, 2))


def test_options():
    from shmgan_amd import data, polar, trainer
    assert data.BRACKET_OPTIONS == ("dofp_exposures", "dofp_bracket_black", "dofp_bracket_white")
    assert set(data.BRACKET_OPTIONS) <= set(data.CAPTURE_OPTIONS) and all(trainer._DEFAULTS[k] is None for k in data.BRACKET_OPTIONS)
    opts = lambda **kw: data.capture_options(SimpleNamespace(capture_format="dofp", dofp_bits=12, **kw))[1]["dofp"]
    assert opts().bracket is None and opts() == polar.DofpLayout("mono", bits=12)
    assert opts(dofp_exposures=(1, 4, 16)).bracket == polar.DofpBracket((1, 4, 16))
    assert opts(dofp_exposures=[1, 4], dofp_bracket_black=64, dofp_bracket_white=4000).bracket == polar.DofpBracket((1, 4), 64, 4000)
    for kw, msg in ((dict(dofp_exposures=(1,)), r"^dofp_exposures \(1,\) are not 2 to 8"), (dict(dofp_exposures=(1, 70000)), r"^dofp_exposures .* \[1, 65535\]"),
                    (dict(dofp_bracket_black=3), r"^dofp_bracket_black 3 needs dofp_exposures"), (dict(dofp_bracket_white=3), r"^dofp_bracket_white 3 needs dofp_exposures"),
                    (dict(dofp_exposures=(1, 2), dofp_bracket_black=-1), r"^dofp_bracket_black -1 is not a count"),
                    (dict(dofp_exposures=(1, 2), dofp_bracket_white=70000), r"^dofp_bracket_white 70000 is not a count"),
                    (dict(dofp_exposures=(1, 2), dofp_bracket_black=4095), r"^dofp_bracket_black 4095 << 4 is above 65519"),
                    (dict(dofp_exposures=(1, 2), dofp_bracket_white=5000), r"^dofp_bracket_white 5000 outside")):
        with pytest.raises(ValueError, match=msg):
            opts(**kw)
    for k, v in (("dofp_exposures", (1, 2)), ("dofp_bracket_black", 3), ("dofp_bracket_white", 300)):
        with pytest.raises(ValueError, match=f"^{k} .* needs capture_format 'dofp', got 'views'"):
            data.capture_options(SimpleNamespace(capture_format="views", **{k: v}))
    # TIFFs are listed only where a bracketed layout asks for them
    assert data.mosaic_extensions(opts()) == () and data.mosaic_extensions(opts(dofp_exposures=(1, 2))) == data.BRACKET_EXT == (".tif", ".tiff")
    assert data._EXT == (".bmp", ".gif", ".jpeg", ".jpg", ".png")


# ---- files ----------------------------------------------------------------------------------------------------------------------------------
def test_tiff_round_trip_and_refusals(tmp_path):
    from PIL import Image
    from shmgan_amd import data, polar
    rng = np.random.default_rng(3)
    for bits, dt in ((8, np.uint8), (16, np.uint16)):
        pages = rng.integers(0, 1 << bits, (3, 10, 14)).astype(dt)
        lay = polar.DofpLayout("mono", bits=bits, bracket=polar.DofpBracket((1, 4, 16)))
        f = polar.write_bracket(str(tmp_path / f"b{bits}.tif"), pages)
        got = polar.decode_mosaic(f, lay)
        assert got.dtype == dt and got.shape == (3, 10, 14) and np.array_equal(got, pages)
        assert np.array_equal(polar.decode_mosaic(polar.write_bracket(str(tmp_path / f"l{bits}.tiff"), list(pages)), lay), pages)
        with pytest.raises(ValueError, match=rf"b{bits}\.tif holds 3 page\(s\), the layout's bracket has 2 exposures"):
            polar.decode_mosaic(f, polar.DofpLayout("mono", bits=bits, bracket=polar.DofpBracket((1, 4))))
        with pytest.raises(ValueError, match=rf"b{bits}\.tif holds {bits}-bit samples"):
            polar.decode_mosaic(f, polar.DofpLayout("mono", bits=12 if bits == 8 else 8, bracket=polar.DofpBracket((1, 4, 16))))
        # an unbracketed layout reads the file as it reads any other: its first page
        assert np.array_equal(polar.decode_mosaic(f, polar.DofpLayout("mono", bits=bits)), pages[0])
    assert data.list_images(str(tmp_path)) == [] and len(data.list_images(str(tmp_path), also=data.BRACKET_EXT)) == 4
    lay = polar.DofpLayout("mono", bits=16, bracket=polar.DofpBracket((1, 4)))
    single = str(tmp_path / "single.png")
    Image.fromarray(np.zeros((10, 14), dtype=np.uint16)).save(single)
    with pytest.raises(ValueError, match=r"single\.png holds 1 page\(s\)"):
        polar.decode_mosaic(single, lay)
    a, b = Image.fromarray(np.zeros((10, 14), dtype=np.uint16)), Image.fromarray(np.zeros((10, 12), dtype=np.uint16))
    a.save(str(tmp_path / "sizes.tif"), save_all=True, append_images=[b])
    with pytest.raises(ValueError, match=r"sizes\.tif: page 1 is 10 x 12 .* page 0 is 10 x 14"):
        polar.decode_mosaic(str(tmp_path / "sizes.tif"), lay)
    a.save(str(tmp_path / "modes.tif"), save_all=True, append_images=[Image.fromarray(np.zeros((10, 14), dtype=np.uint8))])
    with pytest.raises(ValueError, match=r"modes\.tif: page 1 is 10 x 14 of PIL mode 'L'"):
        polar.decode_mosaic(str(tmp_path / "modes.tif"), lay)
    cal = polar.DofpCalibration(dark=np.zeros((10, 16), dtype=np.uint16), bits=16)
    a.save(str(tmp_path / "cal.tif"), save_all=True, append_images=[a])
    with pytest.raises(ValueError, match=r"cal\.tif is 10 x 14, the layout's calibration tables are 10 x 16"):
        polar.decode_mosaic(str(tmp_path / "cal.tif"), polar.DofpLayout("mono", bits=16, calibration=cal, bracket=polar.DofpBracket((1, 4))))
    for bad in ([np.zeros((4, 4), dtype=np.uint16)], [np.zeros((4, 4), dtype=np.uint16), np.zeros((4, 5), dtype=np.uint16)],
                [np.zeros((4, 4), dtype=np.uint16), np.zeros((4, 4), dtype=np.uint8)], [np.zeros((4, 4), dtype=np.float32)] * 2):
        with pytest.raises(ValueError, match="write_bracket takes two or more"):
            polar.write_bracket(str(tmp_path / "bad.tif"), bad)
    with pytest.raises(ValueError, match="is not a TIFF name"):
        polar.write_bracket(str(tmp_path / "bad.png"), np.zeros((2, 4, 4), dtype=np.uint8))


def test_pack_brackets(tmp_path):
    from PIL import Image
    from shmgan_amd import polar
    rng = np.random.default_rng(4)
    frames = rng.integers(0, 4096, (3, 2, 8, 12)).astype(np.uint16)          # [exposure, sample, h, w]
    dirs = [str(tmp_path / f"e{k}") for k in range(3)]
    for k, d in enumerate(dirs):
        os.makedirs(d)
        for i in range(2):
            Image.fromarray(frames[k, i]).save(os.path.join(d, f"s{i}.png"))
    out = polar.pack_brackets(dirs, str(tmp_path / "out"))
    assert [os.path.basename(p) for p in out] == ["s0.tif", "s1.tif"]
    lay = polar.DofpLayout("mono", bits=12, bracket=polar.DofpBracket((1, 4, 16)))
    for i, p in enumerate(out):
        assert np.array_equal(polar.decode_mosaic(p, lay), frames[:, i])
    Image.fromarray(frames[0, 0]).save(os.path.join(dirs[2], "s9.png"))
    with pytest.raises(ValueError, match="different numbers of frames"):
        polar.pack_brackets(dirs, str(tmp_path / "out2"))
    os.remove(os.path.join(dirs[2], "s1.png"))
    with pytest.raises(ValueError, match="do not hold the same names"):
        polar.pack_brackets(dirs, str(tmp_path / "out2"))
    with pytest.raises(ValueError, match="takes 2 to 8 directories"):
        polar.pack_brackets(dirs[:1], str(tmp_path / "out2"))


# ---- the motivating scene -------------------------------------------------------------------------------------------------------------------
def scene_masks(s):
    """(mask, strength) per quad from the longest page alone and from the merged bracket, by the restatements; and the two RMS errors."""
    coef = np.linalg.pinv(0.5 * np.array([[1, np.cos(2 * t), np.sin(2 * t)] for t in np.deg2rad([0.0, 45.0, 90.0, 135.0])]))
    merged = mr.merge(s["pages"], mr.SCENE_EXPOSURES, mr.SCENE_BITS, mr.SCENE_BLACK, 4095)
    out = {}
    for name, mosaic, bits in (("longest", s["pages"][2], 12), ("merged", merged, 16)):
        views, _ = dr.views(mosaic, "mono", dr.SONY_QUAD, bits, "bin")
        mask, q, _ = sm.pipeline(list(views), coef)
        out[name] = (mask > 0, q)
    bg = np.kron(s["background"], np.ones((2, 2), dtype=bool))
    rms = lambda m: float(np.sqrt(np.mean((m.astype(np.float64)[bg] - s["truth"][bg]) ** 2)))
    return out, rms(s["pages"][0].astype(np.int64) << 4), rms(merged)


def test_scene():
    s = mr.scene()
    assert (s["pages"][2][np.kron(s["disc"], np.ones((2, 2), dtype=bool))] == 4095).all()          # the longest page clips the whole disc
    out, rms_short, rms_merged = scene_masks(s)
    mask, q = out["longest"]
    assert not q[s["core"]].any() and not mask.any()                    # strength 0 in the core, and an empty mask
    mask, q = out["merged"]
    assert mask[s["core"]].all() and mask[s["disc"]].all() and int(q[s["core"]].min()) > 100
    print(f"background RMS error: shortest page {rms_short:.1f}, merged {rms_merged:.1f} (1/16 count): a factor of {rms_short / rms_merged:.1f}")
    assert rms_short / rms_merged >= 6.0                                # theory: 21 / sqrt(3) = 12.1; the margin is for the quantisation and the seed


# ---- the entry point's refusals: made before any launch, so they need no GPU ----------------------------------------------------------------
def test_entry_point_refusals():
    from shmgan_amd import _lib
    L = _lib.lib()
    assert "shm_dofp_merge" in _lib.header_functions() and "dofp_merge.hip" in _lib.SOURCES
    assert (_lib.CONSTANTS["SHM_DOFP_MERGE_MAX"], _lib.CONSTANTS["SHM_DOFP_MERGE_TABLE"], _lib.CONSTANTS["SHM_DOFP_MERGE_Q"]) == (8, 256, 20)
    mirror = (C.c_uint * 256)(*[int(v) for v in mr.table((1, 4, 16), 12)])
    fake = 1 << 20           # never dereferenced: every call below is refused first
    good = dict(ptrs=[fake, 2 * fake, 3 * fake], n=3, bits=12, h=8, w=12, spitch=12, table=4 * fake, mirror=mirror, black=64, white=4000, dst=5 * fake,
                dpitch=12, counts=6 * fake)

    def call(a):
        ptrs = None if a["ptrs"] is None else (C.c_void_p * 8)(*(a["ptrs"] + [None] * (8 - len(a["ptrs"]))))
        return L.shm_dofp_merge(ptrs, a["n"], a["bits"], a["h"], a["w"], a["spitch"], a["table"], a["mirror"], a["black"], a["white"], a["dst"],
                                a["dpitch"], a["counts"], None)
    bad_low, bad_high = (C.c_uint * 256)(*mirror), (C.c_uint * 256)(*mirror)
    bad_low[5], bad_high[7] = 0, (1 << 24) + 1
    for change, word in ((dict(ptrs=None), "null"), (dict(ptrs=[fake, None, fake]), "src_ptrs[1]"), (dict(table=None), "null"), (dict(mirror=None), "null"),
                         (dict(dst=None), "null"), (dict(n=1), "n 1"), (dict(n=9), "n 9"), (dict(bits=7), "bits"), (dict(bits=17), "bits"), (dict(h=0), "h 0"),
                         (dict(w=0), "w 0"), (dict(h=32769), "h 32769"), (dict(w=32769, spitch=40000, dpitch=40000), "w 32769"), (dict(spitch=11), "src_pitch"),
                         (dict(dpitch=11), "dst_pitch"), (dict(dst=2 * fake), "dst == src_ptrs[1]"), (dict(black=-1), "black"), (dict(black=4095, white=4096), "black"),
                         (dict(white=0), "white"), (dict(white=4097), "white"), (dict(white=64), "white 64 not above black 64"),
                         (dict(mirror=bad_low), "table_host[5]"), (dict(mirror=bad_high), "table_host[7]")):
        rc = call(dict(good, **change))
        msg = L.shm_last_error().decode()
        assert rc == -1 and "shm_dofp_merge" in msg and word in msg, (change, rc, msg)
