"""The definition behind shm_dofp_views and the host side of the polariser-mosaic capture; needs no GPU.

  * tests/dofp_ref.py (the restatement the GPU test compares the kernel with) against a per-pixel brute force with rational weights
  * the properties the definition has: linear precision, the sample at its own site, the bin identity, total = the rounded exact mean
  * polar.DofpLayout, polar.decode_mosaic, and the refusals of the loader and trainer options that need no device
  * modelled faults, each shown to be caught by the comparison the GPU test makes (equality with dofp_ref.views)
Everything is integer and every comparison is equality."""
from fractions import Fraction
from math import floor
from types import SimpleNamespace

import numpy as np
import pytest

import dofp_ref as dr


# ---- the restatement against a brute force ----------------------------------------------------------------------------------------
def _taps(y, d, N, P):
    n = (N - 1 - d) // P + 1
    q = y - d
    i0 = q // P
    f = q - P * i0
    clip = lambda i: min(max(i, 0), n - 1)
    return [(d + P * clip(i0), Fraction(P - f, P)), (d + P * clip(i0 + 1), Fraction(f, P))]


def _brute(m, pattern, quad, bits, mode):
    """Per pixel, view and channel: the mean over the channel's lattices of the rationally weighted taps (bilinear) or of the
    super-pixel's own samples (bin), scaled to 8 bits, rounded half up, held at 255; total: the same of the mean of the four."""
    h, w = m.shape
    P = dr.period(pattern)
    ho, wo = (h, w) if mode == "bilinear" else (h // P, w // P)
    lat = dr.lattices(pattern, quad)
    scale = Fraction(1, 1 << (bits - 8))
    rnd = lambda v: min(255, floor(v + Fraction(1, 2)))
    views = np.zeros((4, ho, wo, 3), dtype=np.uint8)
    total = np.zeros((ho, wo, 3), dtype=np.uint8)
    for y in range(ho):
        for x in range(wo):
            parts = {}
            for dy, dx, v, chans in lat:
                if mode == "bin":
                    val = Fraction(int(m[P * y + dy, P * x + dx]))
                else:
                    val = sum(wr * wc * int(m[r, c]) for r, wr in _taps(y, dy, h, P) for c, wc in _taps(x, dx, w, P))
                for c in chans:
                    parts.setdefault((v, c), []).append(val)
            for c in range(3):
                means = [sum(parts[(v, c)]) / len(parts[(v, c)]) * scale for v in range(4)]
                for v in range(4):
                    views[v, y, x, c] = rnd(means[v])
                total[y, x, c] = rnd(sum(means) / 4)
    return views, total


BRUTE_SHAPES = ((2, 2), (3, 5), (4, 4), (5, 7), (8, 8), (13, 18))


@pytest.mark.parametrize("pattern", ["mono", "rggb", "gbrg"])
@pytest.mark.parametrize("bits", [8, 12, 16])
def test_restatement_against_brute_force(pattern, bits):
    P = dr.period(pattern)
    for shape in BRUTE_SHAPES:
        if min(shape) < P:
            continue
        for quad in dr.QUADS:
            m = dr.case_mosaic(shape, pattern, quad, bits, "random")
            for mode in dr.MODES:
                bv, bt = _brute(m, pattern, quad, bits, mode)
                for form in (dr.views, dr.views_general):
                    v, t = form(m, pattern, quad, bits, mode)
                    assert np.array_equal(v, bv) and np.array_equal(t, bt), (form.__name__, shape, quad, mode)


@pytest.mark.parametrize("shape,pattern", dr.shape_pattern_pairs(), ids=lambda v: v if isinstance(v, str) else f"{v[0]}x{v[1]}")
def test_two_forms_agree_on_the_case_table(shape, pattern):
    for quad, bits, kind in dr.cases_of(shape, pattern):
        for mode in dr.MODES:
            if mode == "bin" and min(shape) < dr.period(pattern):
                continue
            m, v, t = dr.case_reference(shape, pattern, quad, bits, kind, mode)
            v2, t2 = dr.views_general(m, pattern, quad, bits, mode)
            assert np.array_equal(v, v2) and np.array_equal(t, t2)
            # total is the rounding of the UNROUNDED mean: within 1 of the mean of the rounded views, not always equal to it
            # (for samples within `bits`: a view held at 255 by the clamp says nothing about its numerator)
            if kind != "over":
                assert np.abs(t.astype(np.int64) * 4 - v.astype(np.int64).sum(axis=0)).max() <= 4
            if kind == "max":
                assert v.min() == 255 and t.min() == 255
            if kind == "over":
                assert v.max() == 255           # samples above 2^bits - 1 are not masked: the clamp holds them


# ---- properties ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pattern", dr.PATTERNS)
def test_linear_precision(pattern):
    """Views that are integer planes a + b x + c y come back exactly in the interior, in every channel."""
    P = dr.period(pattern)
    H, W = 16, 24
    y, x = np.mgrid[0:H, 0:W]
    coef = [(3, 2, 5), (90, -1, 4), (20, 6, 0), (200, -3, -7)]
    planes = np.stack([np.repeat((a + b * x + c * y)[..., None], 3, axis=2) for a, b, c in coef])
    assert planes.min() >= 0 and planes.max() <= 255
    for quad in dr.QUADS:
        m = dr.mosaic_from_views(planes, pattern, quad)
        v, t = dr.views(m, pattern, quad, 8)
        inner = (slice(None), slice(P - 1, H - P + 1), slice(P - 1, W - P + 1))
        assert np.array_equal(v[inner], planes[inner])
        assert not np.array_equal(v, planes)            # the border is held, not extrapolated
        mean = planes.sum(axis=0)                      # total: the rounded mean of four exact planes
        assert np.array_equal(t[inner[1:]], ((mean + 2) >> 2)[inner[1:]])


@pytest.mark.parametrize("pattern", dr.PATTERNS)
def test_sites(pattern):
    """Bilinear mode returns the sample itself at its own site in the mono, R and B channels; G is half the own sample plus half
    the mean of the four diagonal neighbours (documented; `bin` is the mode without interpolation)."""
    P, quad = dr.period(pattern), dr.SONY_QUAD
    m = dr.case_mosaic((13, 18), pattern, quad, 8, "random")
    v, _ = dr.views(m, pattern, quad, 8)
    mi = m.astype(np.int64)
    for dy, dx, view, chans in dr.lattices(pattern, quad):
        for c in chans:
            if pattern == "mono" or c != 1:
                assert np.array_equal(v[view, dy::P, dx::P, c], m[dy::P, dx::P])
            else:
                ys, xs = np.arange(dy + P, 13 - 2, P), np.arange(dx + P, 18 - 2, P)          # sites with all four diagonal neighbours
                Y, X = np.meshgrid(ys, xs, indexing="ij")
                diag = mi[Y - 2, X - 2] + mi[Y - 2, X + 2] + mi[Y + 2, X - 2] + mi[Y + 2, X + 2]
                assert np.array_equal(v[view, Y, X, 1], (16 * mi[Y, X] + 4 * diag + 16) >> 5)


def test_bin_identity():
    for quad in dr.QUADS:
        m = dr.case_mosaic((13, 18), "mono", quad, 8, "random")
        v, _ = dr.views(m, "mono", quad, 8, "bin")
        assert v.shape == (4, 6, 9, 3)
        for pos in range(4):
            for c in range(3):
                assert np.array_equal(v[quad[pos], :, :, c], m[pos // 2::2, pos % 2::2][:6, :9])


# ---- modelled faults: the comparison the GPU test makes (equality with dofp_ref.views) catches each ----------------------------------
@pytest.mark.parametrize("pattern,fault", [(p, f) for p in dr.PATTERNS for f in ("quad_rows", "swap_rb", "clamp_n", "truncate")
                                           if (p, f) != ("mono", "swap_rb")])          # a mono sensor has no R and B to exchange
def test_modelled_fault_is_caught(pattern, fault):
    caught = 0
    for shape in dr.SHAPES:
        for quad, bits, kind in dr.cases_of(shape, pattern):
            m, v, t = dr.case_reference(shape, pattern, quad, bits, kind, "bilinear")
            fv, ft = dr.views(m, pattern, quad, bits, "bilinear", fault=fault)
            hit = not (np.array_equal(v, fv) and np.array_equal(t, ft))
            caught += hit
            if kind == "random" and bits > 8:
                assert hit, (shape, quad, bits)          # every random case deeper than 8 bits shows it on its own
    assert caught


def test_pitch_fault_is_caught():
    for pattern in dr.PATTERNS:
        shape, quad = (13, 18), dr.SONY_QUAD
        m, v, t = dr.case_reference(shape, pattern, quad, 12, "random", "bilinear")
        buf, view = dr.pitched(m, shape[1] + 5, np.iinfo(m.dtype).max)
        assert np.array_equal(view, m)
        fv, _ = dr.views(dr.read_with_pitch_w(buf, *shape), pattern, quad, 12)
        assert not np.array_equal(fv, v)


# ---- the layout ------------------------------------------------------------------------------------------------------------------------
def test_layout_orders_views_by_angle():
    from shmgan_amd.polar import DofpLayout, mirror_views, stokes_matrix
    sony = DofpLayout()
    assert (sony.pattern, sony.bits, sony.period) == ("mono", 8, 2)
    assert sony.angles == [0.0, 45.0, 90.0, 135.0] and sony.quad == dr.SONY_QUAD
    other = DofpLayout("rggb", (0, 135, 45, 90), 12)          # another maker's quad
    assert other.angles == [0.0, 45.0, 90.0, 135.0] and other.quad == (0, 3, 1, 2) and other.period == 4
    psd = DofpLayout("gbrg", (150, 0, 60, 90), 16)
    assert psd.angles == [0.0, 60.0, 90.0, 150.0] and psd.quad == (3, 0, 1, 2)
    # delivered in ascending angle, the views take the textbook matrix and the exact 45 / 135 exchange as they are
    assert np.array_equal(stokes_matrix(other.angles), stokes_matrix([0, 45, 90, 135]))
    assert mirror_views(sony.angles) == ("permute", [0, 3, 2, 1])
    assert sony.view_shape(13, 18) == (13, 18) and sony.view_shape(13, 18, "bin") == (6, 9) and other.view_shape(13, 18, "bin") == (3, 4)
    with pytest.raises(Exception):
        sony.bits = 12          # frozen
    # a mosaic sampled from four views by the layout's quad comes back as those views, in ascending angle
    flat = np.stack([np.full((8, 8, 3), 10 * (i + 1)) for i in range(4)])
    got, _ = dr.views(dr.mosaic_from_views(flat, "mono", psd.quad), "mono", psd.quad, 8)
    assert np.array_equal(got, flat)


@pytest.mark.parametrize("bad", [dict(pattern="bayer"), dict(pattern=None), dict(quad_angles=(0, 45, 90)), dict(quad_angles=(0, 45, 90, 90)),
                                 dict(quad_angles=(0, 45, 90, 180)), dict(quad_angles=(0, 45, 90, "x")), dict(quad_angles=(0, 45, 90, float("nan"))),
                                 dict(bits=7), dict(bits=17), dict(bits=12.0), dict(bits=True), dict(bits="12")])
def test_layout_refuses(bad):
    from shmgan_amd.polar import DofpLayout
    with pytest.raises(ValueError, match="DofpLayout"):
        DofpLayout(**bad)


# ---- files ---------------------------------------------------------------------------------------------------------------------------
def test_decode_mosaic_round_trip(tmp_path):
    from PIL import Image
    from shmgan_amd.polar import DofpLayout, decode_mosaic
    rng = np.random.default_rng(5)
    m8 = rng.integers(0, 256, (11, 14)).astype(np.uint8)
    m16 = rng.integers(0, 1 << 16, (11, 14)).astype(np.uint16)
    Image.fromarray(m8).save(tmp_path / "m8.png")
    Image.fromarray(m16).save(tmp_path / "m16.png")
    Image.fromarray(np.stack([m8] * 3, axis=2)).save(tmp_path / "rgb.png")
    a = decode_mosaic(tmp_path / "m8.png", DofpLayout(bits=8))
    assert a.dtype == np.uint8 and np.array_equal(a, m8)
    for bits in (10, 12, 16):
        a = decode_mosaic(tmp_path / "m16.png", DofpLayout("rggb", bits=bits))
        assert a.dtype == np.uint16 and a.flags.c_contiguous and np.array_equal(a, m16)
    with pytest.raises(ValueError, match=r"rgb\.png.*'RGB'"):
        decode_mosaic(tmp_path / "rgb.png", DofpLayout())
    with pytest.raises(ValueError, match=r"m16\.png.*bits = 8"):
        decode_mosaic(tmp_path / "m16.png", DofpLayout(bits=8))
    with pytest.raises(ValueError, match=r"m8\.png.*bits = 12"):
        decode_mosaic(tmp_path / "m8.png", DofpLayout(bits=12))


# ---- options that are refused before anything is listed or allocated -------------------------------------------------------------------
def _capture_dir(tmp_path, n=3):
    from PIL import Image
    for d in ("DOFP", "ED"):
        (tmp_path / d).mkdir()
    for i in range(n):
        Image.fromarray(np.full((8, 8), i, dtype=np.uint8)).save(tmp_path / "DOFP" / f"s{i}.png")
        Image.fromarray(np.full((8, 8, 3), i, dtype=np.uint8)).save(tmp_path / "ED" / f"s{i}.png")
    return str(tmp_path)


def test_polar_dataset_options(tmp_path):
    from shmgan_amd.data import Augment, PolarDataset
    from shmgan_amd.polar import DofpLayout, mirror_views, stokes_matrix
    missing = str(tmp_path / "nowhere")                 # never listed: the refusals come first
    with pytest.raises(ValueError, match="capture 'raw'"):
        PolarDataset(missing, 32, capture="raw")
    with pytest.raises(ValueError, match="needs dofp=polar.DofpLayout"):
        PolarDataset(missing, 32, capture="dofp")
    with pytest.raises(ValueError, match="needs dofp=polar.DofpLayout"):
        PolarDataset(missing, 32, capture="dofp", dofp=("mono", (90, 45, 135, 0), 8))
    with pytest.raises(ValueError, match="dofp_demosaic 'nearest'"):
        PolarDataset(missing, 32, capture="dofp", dofp=DofpLayout(), dofp_demosaic="nearest")
    with pytest.raises(ValueError, match="mosaic directory and the diffuse directory"):
        PolarDataset(missing, 32, subdirs=("DOFP",), capture="dofp", dofp=DofpLayout())
    root = _capture_dir(tmp_path)
    lay = DofpLayout("mono", (0, 135, 45, 90))
    ds = PolarDataset(root, 32, subdirs=("DOFP", "ED"), capture="dofp", dofp=lay, diffuse_source="stokes", rank=0, world=1,
                      augment=Augment(flip_lr=0.5), dofp_demosaic="bin")
    assert ds.n == 3 and len(ds.files) == 1                                   # "stokes" reads the mosaics alone
    assert np.array_equal(ds.coef, stokes_matrix([0, 45, 90, 135])) and ds._mirror == mirror_views([0, 45, 90, 135])
    assert len(PolarDataset(root, 32, subdirs=("DOFP", "ED"), capture="dofp", dofp=lay, rank=0, world=1).files) == 2
    train, val = ds.split(0.34, seed=1)                                       # the parts keep the capture options
    assert train.n + val.n == 3 and val.n == 1
    for part in (train, val):
        assert (part.capture, part.dofp, part.dofp_demosaic) == ("dofp", lay, "bin") and len(part.files) == 1
    (tmp_path / "ED" / "s2.png").unlink()
    with pytest.raises(ValueError, match="different numbers of images"):
        PolarDataset(root, 32, subdirs=("DOFP", "ED"), capture="dofp", dofp=lay, rank=0, world=1)


def _plain_trainer(root, **args):
    return SimpleNamespace(args=SimpleNamespace(**args), data_dir=root, image_size=32, batch_size=1, device=None, num_epochs=1)


def test_trainer_options(tmp_path):
    from shmgan_amd.data import capture_options, datasetLoad
    from shmgan_amd.polar import DofpLayout
    missing = str(tmp_path / "nowhere")
    for bad, name in [(dict(capture_format="raw"), "capture_format 'raw'"), (dict(dofp_demosaic="nearest"), "dofp_demosaic 'nearest'"),
                      (dict(capture_format="dofp", dofp_pattern="bayer"), "dofp_pattern 'bayer'"),
                      (dict(capture_format="dofp", dofp_quad_angles=(0, 0, 45, 90)), "dofp_quad_angles"),
                      (dict(capture_format="dofp", dofp_bits=20), "dofp_bits 20"), (dict(capture_format="dofp", dofp_dir=""), "dofp_dir ''")]:
        with pytest.raises(ValueError, match=name):
            datasetLoad(_plain_trainer(missing, **bad))
    assert capture_options(SimpleNamespace()) == (("I0", "I60", "I90", "I150", "ED"), dict(capture="views", dofp=None, dofp_demosaic="bilinear"))
    subdirs, kw = capture_options(SimpleNamespace(capture_format="dofp", dofp_dir="RAW", dofp_pattern="bggr", dofp_bits=12, dofp_demosaic="bin"))
    assert subdirs == ("RAW", "ED") and kw == dict(capture="dofp", dofp=DofpLayout("bggr", (90, 45, 135, 0), 12), dofp_demosaic="bin")
    root = _capture_dir(tmp_path)
    t = _plain_trainer(root, capture_format="dofp", val_fraction=0.34)
    n, ds = datasetLoad(t)
    assert n == 2 and ds.capture == "dofp" and ds.dofp == DofpLayout() and t.valDataset.n == 1 and t.valDataset.capture == "dofp"
    from shmgan_amd.trainer import _DEFAULTS
    assert _DEFAULTS["capture_format"] == "views" and _DEFAULTS["dofp_dir"] == "DOFP" and _DEFAULTS["dofp_test_view"] == "total"


def test_eval_and_writer_options(tmp_path):
    from shmgan_amd import polar
    from shmgan_amd.data import EvalDataset, MaskDataset, NativeEvalDataset
    root = _capture_dir(tmp_path)
    lay = polar.DofpLayout()
    for cls, lead in ((EvalDataset, (root + "/DOFP", 32)), (NativeEvalDataset, (root + "/DOFP",))):
        with pytest.raises(ValueError, match="dofp_test_view 4"):
            cls(*lead, capture="dofp", dofp=lay, dofp_test_view=4)
        with pytest.raises(ValueError, match="needs dofp=polar.DofpLayout"):
            cls(*lead, capture="dofp")
        ds = cls(*lead, capture="dofp", dofp=lay, dofp_demosaic="bin", dofp_test_view=2)
        assert ds.n == 3 and ds.sources(0)[0][1] == (4, 4)                   # the photo's size is the demosaiced plane's
    for fn in (polar.write_specular_masks, polar.write_estimated_diffuse):
        with pytest.raises(ValueError, match="capture 'raw'"):
            fn(root, str(tmp_path / "out"), capture="raw")
        with pytest.raises(ValueError, match="needs dofp=polar.DofpLayout"):
            fn(root, str(tmp_path / "out"), subdirs=("DOFP",), capture="dofp")
    with pytest.raises(ValueError, match="needs dofp=polar.DofpLayout"):
        MaskDataset.from_polar(root, 32, subdirs=("DOFP",), capture="dofp")
    ds = MaskDataset.from_polar(root, 32, subdirs=("DOFP",), capture="dofp", dofp=lay)
    assert ds.names == ["s0", "s1", "s2"] and all(len(f) == 1 for f in ds.files)
