"""The definition behind shm_dofp_develop / shm_dofp_wb_gray and the host side of the development options; needs no GPU.

  * tests/develop_ref.py (the restatement the GPU test compares the kernels with) against a per-pixel brute force in Python integers and
    fractions, and its `lin` against the real-valued ideal: within 1 unit of 65535
  * polar.DofpDevelop.table against the restatement's own table; the tone tables' shape
  * the properties the definition has: saturation stays neutral, darkness maps to lut[0], monotone without a matrix, a balanced grey is grey,
    grey-world gains return the balance and ignore saturated periods
  * modelled faults, each shown to be caught by the comparison the GPU test makes (equality with develop_ref)
  * the options: develop=None layouts are today's, refusals by name, capture_options keeps its three keys"""
from fractions import Fraction
from math import floor
from types import SimpleNamespace

import numpy as np
import pytest

import develop_ref as dv
import dofp_ref as dr


# ---- the restatement against a brute force --------------------------------------------------------------------------------------------
def _taps(y, d, N, P):
    n = (N - 1 - d) // P + 1
    q = y - d
    i0 = q // P
    f = q - P * i0
    clip = lambda i: min(max(i, 0), n - 1)
    return [(d + P * clip(i0), Fraction(P - f, P)), (d + P * clip(i0 + 1), Fraction(f, P))]


def _means(m, pattern, quad, mode):
    """{(view, channel, y, x): the rational mean over the channel's lattices of the rationally weighted taps (or own samples)}."""
    h, w = m.shape
    P = dr.period(pattern)
    ho, wo = (h, w) if mode == "bilinear" else (h // P, w // P)
    out = {}
    for y in range(ho):
        for x in range(wo):
            parts = {}
            for dy, dx, v, chans in dr.lattices(pattern, quad):
                if mode == "bin":
                    val = Fraction(int(m[P * y + dy, P * x + dx]))
                else:
                    val = sum(wr * wc * int(m[r, c]) for r, wr in _taps(y, dy, h, P) for c, wc in _taps(x, dx, w, P))
                for c in chans:
                    parts.setdefault((v, c), []).append(val)
            for (v, c), vals in parts.items():
                out[v, c, y, x] = sum(vals) / len(vals)
    return out, ho, wo


def _brute_pixel(mean3, params, lut, white_real=None):
    """One pixel from its three rational channel means, by the header's steps on exact rationals scaled to integers: (out [3], lin [3], ideal [3])."""
    black, mul, gain, flag, ccm = dv.fields(params)
    lin, ideal = [], []
    for c in range(3):
        # N / 2^k is the mean itself: D * M / 2^(16 + k) = max(0, mean - black) * M / 2^16, rounded half up
        d = max(Fraction(0), mean3[c] - int(black[c]))
        M = (int(mul[c]) * int(gain[c]) + 512) >> 10
        lin.append(min(65535, floor(d * M / 65536 + Fraction(1, 2))))
        ideal.append(d * M / 65536)
    if flag:
        lin = [min(65535, max(0, (sum(int(ccm[c][j]) * lin[j] for j in range(3)) + 512) >> 10)) for c in range(3)]
    return [int(lut[v >> 4]) for v in lin], lin, ideal


BRUTE_SHAPES = ((4, 4), (5, 7), (13, 18))


@pytest.mark.parametrize("pattern", ["mono", "rggb", "gbrg"])
@pytest.mark.parametrize("bits", [8, 12, 16])
def test_restatement_against_brute_force(pattern, bits):
    for shape in BRUTE_SHAPES:
        quad = dr.QUADS[(shape[0] + bits) % 2]
        m = dr.case_mosaic(shape, pattern, quad, bits, "random")
        for mode in dr.MODES:
            means, ho, wo = _means(m, pattern, quad, mode)
            for name in dv.SETS:
                p, lut = dv.param_set(name, pattern, bits)
                v, t = dv.develop(m, pattern, quad, bits, mode, p, lut)
                for y in range(ho):
                    for x in range(wo):
                        per_view = [[means[view, c, y, x] for c in range(3)] for view in range(4)]
                        for view in range(4):
                            assert list(v[view, y, x]) == _brute_pixel(per_view[view], p, lut)[0], (shape, mode, name, view, y, x)
                        mean_of_views = [sum(per_view[view][c] for view in range(4)) / 4 for c in range(3)]
                        assert list(t[y, x]) == _brute_pixel(mean_of_views, p, lut)[0], (shape, mode, name, "total", y, x)


@pytest.mark.parametrize("bits", [8, 12, 16])
def test_lin_is_within_one_unit_of_the_real_valued_ideal(bits):
    """lin against (mean - black) * 65535 wb gain / (white - black) in exact rationals: 0.5 from its own rounding, at most 0.5 from the
    multiplier, which is within 2^-17 relative of the real factor."""
    pattern, quad, shape = "rggb", dr.SONY_QUAD, (13, 18)
    top = 1 << bits
    black, white, wb = (top // 16, top // 16 + 1, top // 16 - 1), top - 1 - top // 32, (Fraction(19, 10), Fraction(1), Fraction(8, 5))
    p, lut = dv.table(bits, black=black, white=white, wb=wb, tone="linear")
    _, mul, _, _, _ = dv.fields(p)
    for c in range(3):
        real = Fraction(65535 * 65536) * wb[c] / (white - black[c])
        assert 65536 <= mul[c] < 1 << 32 and abs(int(mul[c]) - real) <= Fraction(1, 2) and abs(int(mul[c]) - real) / real <= Fraction(1, 1 << 17)
    m = dr.case_mosaic(shape, pattern, quad, bits, "random")
    for mode in dr.MODES:
        means, ho, wo = _means(m, pattern, quad, mode)
        N, nl, wt = dr.numerators(m, pattern, quad, mode)
        k = int(np.log2(wt)) + (nl == 2).astype(np.int64)
        lin = dv.linear(N, k, p)
        worst = Fraction(0)
        for (view, c, y, x), mean in means.items():
            ideal = max(Fraction(0), mean - black[c]) * 65535 * wb[c] / (white - black[c])
            if ideal <= 65535:
                worst = max(worst, abs(int(lin[view, y, x, c]) - ideal))
            else:
                assert lin[view, y, x, c] == 65535
        assert Fraction(1, 4) < worst <= 1, float(worst)


def test_table_equals_the_restatements():
    from shmgan_amd.polar import DofpDevelop, DofpLayout
    sets = [dict(), dict(black=240, tone="linear"), dict(black=(250, 240, 245), white=4000, wb=(1.9, 1, 1.6)),
            dict(black=16, wb=(3.8, 2, 3.2), ccm=dv.CCM_MILD, tone=2.2), dict(black=1536, white=2048, wb=(16, 1, 4), ccm=dv.CCM_WILD)]
    for kw in sets:
        lay = DofpLayout("rggb", bits=12, develop=DofpDevelop(**kw))
        params, lut, mirror = lay.develop.table(lay)
        ref_p, ref_lut = dv.table(12, **kw)
        assert params.dtype == np.int32 and params.shape == (dv.NPARAMS,) and np.array_equal(params, ref_p), kw
        assert lut.dtype == np.uint8 and lut.shape == (4096,) and np.array_equal(lut, ref_lut), kw
        assert np.array_equal(np.asarray(mirror), params)
    # wb "gray": the balance is left to the device, the table is the unbalanced one; white follows the layout's depth
    for bits in (8, 10, 16):
        lay = DofpLayout("bggr", bits=bits, develop=DofpDevelop(black=3, wb="gray", tone="linear"))
        assert np.array_equal(lay.develop.table(lay)[0], dv.table(bits, black=3, tone="linear")[0])
        assert lay.develop.saturation(lay) == (1 << bits) - 1
    lay = DofpLayout("bggr", bits=12, develop=DofpDevelop(wb="gray", sat=3900))
    assert lay.develop.saturation(lay) == 3900
    # the sets the GPU test runs are tables DofpDevelop makes, too (the extreme set's gains are the device's to write)
    for pattern in ("mono", "rggb"):
        mono = pattern == "mono"
        lay = DofpLayout(pattern, bits=12, develop=DofpDevelop(black=256 if mono else (255, 256, 257), wb=(1, 1, 1) if mono else (1.9, 1, 1.6),
                                                               ccm=None if mono else dv.CCM_MILD, tone=2.2))
        assert all(np.array_equal(a, b) for a, b in zip(lay.develop.table(lay)[:2], dv.param_set("ccm_gamma", pattern, 12)))


@pytest.mark.parametrize("tone", ["linear", "srgb", 1.0, 2.2, 4.0])
def test_tone_tables(tone):
    from shmgan_amd.polar import tone_table
    lut = dv.tone_table(tone)
    assert np.array_equal(tone_table(tone), lut)
    assert lut[0] == 0 and lut[4095] == 255 and np.all(np.diff(lut.astype(int)) >= 0)
    if tone in ("linear", "srgb", 1.0):          # slope below one code per entry everywhere: no code is skipped
        assert np.all(np.diff(lut.astype(int)) <= 1) and len(set(lut.tolist())) == 256
    if tone == 1.0:
        assert np.array_equal(lut, dv.tone_table("linear"))


# ---- properties ---------------------------------------------------------------------------------------------------------------------------
WBS = ((1, 1, 1), (1.9, 1, 1.6), (16, 1, 4), (1, 16, 16))


@pytest.mark.parametrize("pattern", ["rggb", "grbg"])
@pytest.mark.parametrize("bits", [8, 12, 16])
def test_saturation_is_neutral_and_darkness_is_black(pattern, bits):
    top = 1 << bits
    for wb in WBS:
        for tone in ("linear", "srgb", 2.2):
            for ccm in (None, ((1, 0, 0), (0, 1, 0), (0, 0, 1))):
                p, lut = dv.table(bits, black=top // 16, wb=wb, tone=tone, ccm=ccm)
                for mode in dr.MODES:
                    v, t = dv.develop(np.full((8, 12), top - 1, dtype=np.uint16), pattern, dr.SONY_QUAD, bits, mode, p, lut)
                    assert v.min() == 255 and t.min() == 255, (wb, tone, mode)
                    dark = np.random.default_rng(bits).integers(0, top // 16 + 1, (8, 12)).astype(np.uint16)
                    v, t = dv.develop(dark, pattern, dr.SONY_QUAD, bits, mode, p, lut)
                    assert v.max() == lut[0] == 0 and t.max() == 0, (wb, tone, mode)


def test_monotone_without_a_matrix():
    """Raising any one sample lowers no output byte."""
    pattern, quad, bits = "gbrg", dr.QUADS[1], 12
    p, lut = dv.param_set("wb_srgb", pattern, bits)
    rng = np.random.default_rng(7)
    m = rng.integers(0, 4096, (9, 13)).astype(np.uint16)
    for mode in dr.MODES:
        v0, t0 = dv.develop(m, pattern, quad, bits, mode, p, lut)
        for _ in range(40):
            y, x = int(rng.integers(0, 9)), int(rng.integers(0, 13))
            m2 = m.copy()
            m2[y, x] = min(65535, int(m[y, x]) + int(rng.integers(1, 3000)))
            v1, t1 = dv.develop(m2, pattern, quad, bits, mode, p, lut)
            assert np.all(v1 >= v0) and np.all(t1 >= t0)


def _tinted_grey(pattern, bits, wb, black, shape=(16, 24), level=None):
    """The mosaic of a flat grey scene seen through channel responses (1/r, 1/g, 1/b) on top of the pedestal: exact integers where wb divides."""
    top = 1 << bits
    level = top // 2 if level is None else level
    h, w = shape
    y, x = np.mgrid[0:h, 0:w]
    c = np.asarray(dr.CHANNEL[pattern])[2 * ((y // 2) % 2) + ((x // 2) % 2)]
    val = np.array([black + Fraction(level) / Fraction(g) for g in wb])
    return np.array([[int(round(float(val[c[i, j]]))) for j in range(w)] for i in range(h)], dtype=np.uint16 if bits > 8 else np.uint8)


@pytest.mark.parametrize("pattern", ["rggb", "bggr", "grbg", "gbrg"])
def test_balanced_grey_is_grey_and_gray_world_finds_the_balance(pattern):
    bits, black = 12, 240
    for wb in ((2, 1, 1.6), (1.25, 1, 2.5), (1, 4, 2)):
        m = _tinted_grey(pattern, bits, wb, black)
        p, lut = dv.table(bits, black=black, wb=wb, tone="linear")
        N, nl, wt = dr.numerators(m, pattern, dr.SONY_QUAD, "bilinear")
        lin = dv.linear(N, int(np.log2(wt)) + (nl == 2).astype(np.int64), p)
        # the scene values were rounded to whole counts (half a count, times the gain, in units of 65535 / (white - black)): within one 8-bit
        # code, 257 units, before the tone table
        assert np.abs(lin[..., 0] - lin[..., 1]).max() <= 257 and np.abs(lin[..., 1] - lin[..., 2]).max() <= 257
        codes = lin >> 8
        assert np.abs(codes[..., 0] - codes[..., 1]).max() <= 1 and np.abs(codes[..., 1] - codes[..., 2]).max() <= 1
        # grey-world: the triple, normalised to its smallest entry, to within the Q10 step
        sums, gains = dv.wb_gray(m, pattern, dv.table(bits, black=black)[0], (1 << bits) - 1)
        assert sums[3] == sums[5] == m.size // 4 and sums[4] == m.size // 2
        for c in range(3):
            want = Fraction(wb[c]) / min(Fraction(g) for g in wb)
            assert abs(Fraction(gains[c], 1024) - want) <= Fraction(1, 1024), (wb, c, gains)


def test_gray_world_ignores_saturated_periods():
    pattern, bits, black = "rggb", 12, 240
    m = _tinted_grey(pattern, bits, (2, 1, 1.6), black)
    p = dv.table(bits, black=black)[0]
    clean = dv.wb_gray(m, pattern, p, 4095)
    hot = m.copy()
    hot[0:4, 4:8] = 4095                     # one whole period clipped, one period with a single clipped sample
    hot[9, 13] = 4095
    sums, gains = dv.wb_gray(hot, pattern, p, 4095)
    assert sums[3] == clean[0][3] - 2 * 4 and gains == clean[1]
    assert dv.wb_gray(hot, pattern, p, 4095, fault="sat_included")[1] != clean[1]
    # every period holds a saturated sample: nothing is counted, identity gains
    every = m.copy()
    every[1::4, 2::4] = 4095
    assert dv.wb_gray(every, pattern, p, 4095) == ((0,) * 6, (1024, 1024, 1024))
    assert dv.wb_gray(np.full((8, 8), 4095, dtype=np.uint16), pattern, p, 4095)[1] == (1024, 1024, 1024)
    # a frame at or below black: the means are 0, identity gains
    assert dv.wb_gray(np.full((8, 8), 200, dtype=np.uint16), pattern, p, 4095) == ((0, 0, 0, 16, 32, 16), (1024, 1024, 1024))
    from shmgan_amd.polar import gray_gains
    assert gray_gains(sums) == gains and gray_gains((0,) * 6) == (1024, 1024, 1024)


# ---- modelled faults: the comparison the GPU test makes (equality with develop_ref) catches each -------------------------------------------
def _caught(fault, patterns):
    hits = 0
    for pattern in patterns:
        for shape in dv.SHAPES:
            for quad, bits, kind in dv.cases_of(shape, pattern):
                for mode in dr.MODES:
                    for name in dv.SETS:
                        m, v, t = dv.case_reference(shape, pattern, quad, bits, kind, mode, name)
                        p, lut = dv.param_set(name, pattern, bits)
                        fv, ft = dv.develop(m, pattern, quad, bits, mode, p, lut, fault=fault)
                        hits += not (np.array_equal(v, fv) and np.array_equal(t, ft))
    return hits


@pytest.mark.parametrize("fault", ["black_sample_scale", "black_after_gain", "total_from_views", "no_clamp", "ccm_transposed", "ccm_before_gain",
                                   "lut_low_bits", "swap_rb_gain"])
def test_modelled_fault_is_caught(fault):
    assert _caught(fault, ("rggb",)) > 0
    if fault in ("black_sample_scale", "black_after_gain", "total_from_views", "lut_low_bits"):          # faults a mono sensor can have
        assert _caught(fault, ("mono",)) > 0


def test_gray_and_pitch_faults_are_caught():
    hits = 0
    for shape in dv.SHAPES:
        for kind in ("mixed", "over"):
            m = dv.gray_frame(shape, "grbg", 12, kind)
            p = dv.param_set("wb_srgb", "grbg", 12)[0]
            hits += dv.wb_gray(m, "grbg", p, 4095) != dv.wb_gray(m, "grbg", p, 4095, fault="sat_included")
    assert hits
    shape, pattern, quad = (9, 1031), "rggb", dr.QUADS[0]
    m, v, _ = dv.case_reference(shape, pattern, quad, 12, "random", "bilinear", "wb_srgb")
    buf, view = dr.pitched(m, shape[1] + 5, np.iinfo(m.dtype).max)
    p, lut = dv.param_set("wb_srgb", pattern, 12)
    assert np.array_equal(view, m)
    assert not np.array_equal(dv.develop(dr.read_with_pitch_w(buf, *shape), pattern, quad, 12, "bilinear", p, lut)[0], v)
    assert dv.wb_gray(dr.read_with_pitch_w(buf, *shape), pattern, p, 4095) != dv.wb_gray(m, pattern, p, 4095)
    assert set(dv.FAULTS) == {"black_sample_scale", "black_after_gain", "total_from_views", "no_clamp", "ccm_transposed", "ccm_before_gain",
                              "lut_low_bits", "swap_rb_gain", "sat_included", "pitch_w"}


# ---- the options -------------------------------------------------------------------------------------------------------------------------
def test_layouts_without_development_are_todays():
    from shmgan_amd.polar import DofpDevelop, DofpLayout
    assert DofpLayout("bggr", (90, 45, 135, 0), 12) == DofpLayout("bggr", (90, 45, 135, 0), 12, None) == DofpLayout("bggr", bits=12, develop=None)
    assert DofpLayout().develop is None and hash(DofpLayout()) == hash(DofpLayout(develop=None))
    d = DofpDevelop(black=240, white=4095, wb=[2, 1, 1.5])
    assert (d.black, d.white, d.wb, d.ccm, d.tone, d.sat) == ((240, 240, 240), 4095, (2.0, 1.0, 1.5), None, "srgb", None)
    assert d == DofpDevelop((240, 240, 240), 4095, (2, 1, 1.5)) and hash(d) == hash(DofpDevelop((240, 240, 240), 4095, (2, 1, 1.5)))
    lay = DofpLayout("rggb", bits=12, develop=d)
    assert lay != DofpLayout("rggb", bits=12) and lay == DofpLayout("rggb", bits=12, develop=DofpDevelop(240, 4095, (2, 1, 1.5)))
    assert {lay: 1}[DofpLayout("rggb", bits=12, develop=d)] == 1
    with pytest.raises(Exception):
        d.black = 0          # frozen


@pytest.mark.parametrize("bad,name", [(dict(black=-1), "black"), (dict(black=(1, 2)), "black"), (dict(black="x"), "black"), (dict(black=1.5), "black"),
                                      (dict(black=65520), "black"), (dict(white=8), "white"), (dict(black=100, white=110), "white"), (dict(white="x"), "white"),
                                      (dict(wb=(1, 2)), "wb"), (dict(wb="grey"), "wb"), (dict(wb=(0, 1, 1)), "wb"), (dict(wb=(1, 17, 1)), "wb"),
                                      (dict(wb=(1, float("nan"), 1)), "wb"), (dict(ccm=(1, 2, 3)), "ccm"), (dict(ccm=[[8, 0, 0], [0, 1, 0], [0, 0, 1]]), "ccm"),
                                      (dict(ccm="x"), "ccm"), (dict(tone="log"), "tone"), (dict(tone=0.5), "tone"), (dict(tone=5), "tone"), (dict(tone=True), "tone"),
                                      (dict(sat=0), "sat"), (dict(sat=70000), "sat"), (dict(sat="x"), "sat")])
def test_develop_refuses_by_name(bad, name):
    from shmgan_amd.polar import DofpDevelop
    with pytest.raises(ValueError, match=f"DofpDevelop: {name} "):
        DofpDevelop(**bad)


def test_layout_refuses_a_development_it_cannot_run():
    from shmgan_amd.polar import DofpDevelop, DofpLayout
    with pytest.raises(ValueError, match="DofpLayout: develop"):
        DofpLayout(develop=dict(black=3))
    with pytest.raises(ValueError, match="DofpDevelop: wb 'gray' needs a Bayer pattern"):
        DofpLayout("mono", develop=DofpDevelop(wb="gray"))
    with pytest.raises(ValueError, match="DofpDevelop: ccm needs a Bayer pattern"):
        DofpLayout("mono", develop=DofpDevelop(ccm=np.eye(3)))
    with pytest.raises(ValueError, match="DofpDevelop: black .* must be the same for all channels"):
        DofpLayout("mono", develop=DofpDevelop(black=(1, 2, 3)))
    with pytest.raises(ValueError, match="DofpDevelop: black .* must be the same for all channels"):
        DofpLayout("mono", develop=DofpDevelop(wb=(1, 2, 1)))
    with pytest.raises(ValueError, match=r"DofpDevelop: white 255 \(8 bits\)"):
        DofpLayout("rggb", bits=8, develop=DofpDevelop(black=240))
    assert DofpLayout("mono", bits=12, develop=DofpDevelop(black=240, wb=(2, 2, 2))).develop.table(DofpLayout("mono", bits=12))[0][dv.MUL] == \
        dv.table(12, black=240)[0][dv.MUL]


def test_trainer_options():
    from shmgan_amd.data import CAPTURE_OPTIONS, capture_options
    from shmgan_amd.polar import DofpDevelop, DofpLayout
    from shmgan_amd.trainer import _DEFAULTS
    names = ("dofp_black", "dofp_white", "dofp_wb", "dofp_ccm", "dofp_tone", "dofp_sat")
    assert all(n in CAPTURE_OPTIONS and n in _DEFAULTS and _DEFAULTS[n] is None for n in names)
    base = dict(capture_format="dofp", dofp_pattern="rggb", dofp_bits=12)
    # none given (or all None, as the trainer's defaults are): today's layout, and exactly the three keys
    for extra in ({}, {n: None for n in names}):
        subdirs, kw = capture_options(SimpleNamespace(**base, **extra))
        assert kw == dict(capture="dofp", dofp=DofpLayout("rggb", (90, 45, 135, 0), 12), dofp_demosaic="bilinear") and kw["dofp"].develop is None
    subdirs, kw = capture_options(SimpleNamespace(**base, dofp_black=240, dofp_wb=(2, 1, 1.5), dofp_tone="linear"))
    assert sorted(kw) == ["capture", "dofp", "dofp_demosaic"] and subdirs == ("DOFP", "ED")
    assert kw["dofp"] == DofpLayout("rggb", (90, 45, 135, 0), 12, DofpDevelop(black=240, wb=(2, 1, 1.5), tone="linear"))
    _, kw = capture_options(SimpleNamespace(**base, dofp_sat=4000))
    assert kw["dofp"].develop == DofpDevelop(sat=4000)
    # a development option on a four-directory capture would be ignored: refused by name instead
    for n, val in zip(names, (3, 4000, "gray", (1, 0, 0, 0, 1, 0, 0, 0, 1), "linear", 4000)):
        with pytest.raises(ValueError, match=f"{n} .* needs capture_format 'dofp'"):
            capture_options(SimpleNamespace(**{n: val}))
    assert capture_options(SimpleNamespace(**{n: None for n in names}))[1] == dict(capture="views", dofp=None, dofp_demosaic="bilinear")
    for bad, name in [(dict(dofp_black=-3), "dofp_black -3"), (dict(dofp_white=4), "dofp_white 4"), (dict(dofp_wb="auto"), "dofp_wb 'auto'"),
                      (dict(dofp_ccm=(1, 2)), "dofp_ccm"), (dict(dofp_tone="log"), "dofp_tone 'log'"), (dict(dofp_sat=0), "dofp_sat 0"),
                      (dict(dofp_pattern="mono", dofp_wb="gray"), "dofp_wb 'gray' needs a Bayer pattern")]:
        with pytest.raises(ValueError, match=name):
            capture_options(SimpleNamespace(**dict(base, **bad)))
