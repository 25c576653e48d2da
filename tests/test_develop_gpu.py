"""shm_dofp_develop and shm_dofp_wb_gray (csrc/dofp_develop.hip) and everything built on them, on the device.

The kernels are compared bit for bit with the NumPy restatement (tests/develop_ref.py, which tests/test_develop_cpu.py holds against a
brute force in exact rationals): five parameter sets, every pattern, 8 / 12 / 16 bits, both modes, random / all-maximum / over-range data,
with and without the total plane, destinations carved out of a poisoned buffer at 4-byte-aligned and at odd addresses (both store paths),
pitched sources whose gap holds the largest value.  The plumbing is tested by equivalence: a mosaic directory read with a developing
layout must give exactly what four view directories give that hold the restatement's developed views.  No tolerance anywhere."""
import ctypes as C
import inspect
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import develop_ref as dv
import dofp_ref as dr

pytestmark = pytest.mark.gpu

POISON = 0xA5
E_SHAPE = -1


def _lib():
    from shmgan_amd import _lib as L
    return L.lib()


def _stream():
    return torch.cuda.current_stream().cuda_stream


@pytest.fixture(scope="module")
def tables():
    """(params, lut) of a parameter set on the device, and the host mirror: uploaded once per set."""
    made = {}

    def get(name, pattern, bits):
        key = (name, pattern, bits)
        if key not in made:
            p, lut = dv.param_set(name, pattern, bits)
            made[key] = (torch.from_numpy(np.array(p)).cuda(), torch.from_numpy(np.array(lut)).cuda(), (C.c_int * dv.NPARAMS)(*[int(x) for x in p]))
        return made[key]
    return get


def _call(src, bits, h, w, pitch, pattern, quad, mode, ptrs, total, params, lut, mirror):
    q = (C.c_int * 4)(*quad) if quad is not None else None
    dp = (C.c_void_p * 4)(*ptrs) if ptrs is not None else None
    return _lib().shm_dofp_develop(src, bits, h, w, pitch, pattern, q, mode, dp, total, params, lut, mirror, _stream())


def _out_shape(h, w, pattern, mode):
    P = dr.period(pattern)
    return (h, w) if mode == "bilinear" else (h // P, w // P)


def _carve(n, aligned):
    """(pool, offsets of five planes of n bytes): 4-byte-aligned planes, or planes at odd addresses, each with guard bytes around."""
    first, stride = (64, (n + 3) // 4 * 4 + 8) if aligned else (61, n + 37)
    pool = torch.full((first + 5 * stride + 64,), POISON, dtype=torch.uint8, device="cuda")
    return pool, [first + i * stride for i in range(5)]


def _run(mosaic, pattern, quad, bits, mode, tab, aligned, pitch_extra, with_total):
    """The kernel on `mosaic` (host array) from a source of row pitch w + pitch_extra whose gap holds the largest value, into carved planes:
    (views [4,ho,wo,3], total or None, True if every byte outside the planes still holds the poison)."""
    h, w = mosaic.shape
    buf = dr.pitched(mosaic, w + pitch_extra, np.iinfo(mosaic.dtype).max)[0] if pitch_extra else mosaic
    src = torch.from_numpy(np.array(buf)).cuda()
    ho, wo = _out_shape(h, w, pattern, mode)
    n = ho * wo * 3
    pool, offs = _carve(n, aligned)
    base = pool.data_ptr()
    rc = _call(src.data_ptr(), bits, h, w, w + pitch_extra, dr.PATTERNS.index(pattern), quad, dr.MODES.index(mode), [base + o for o in offs[:4]],
               base + offs[4] if with_total else None, tab[0].data_ptr(), tab[1].data_ptr(), tab[2])
    assert rc == 0, (rc, _lib().shm_last_error())
    got = pool.cpu().numpy()
    outside = np.ones(got.shape, dtype=bool)
    planes = []
    for o in offs[:5 if with_total else 4]:
        planes.append(got[o:o + n].reshape(ho, wo, 3))
        outside[o:o + n] = False
    return np.stack(planes[:4]), (planes[4] if with_total else None), bool(np.all(got[outside] == POISON))


@pytest.mark.parametrize("shape,pattern", [(s, p) for s in dv.SHAPES for p in dr.PATTERNS], ids=lambda v: v if isinstance(v, str) else f"{v[0]}x{v[1]}")
def test_kernel_bit_exact(shape, pattern, tables):
    h, w = shape
    for quad, bits, kind in dv.cases_of(shape, pattern):
        for mode in dr.MODES:
            for name in dv.SETS:
                m, ref_v, ref_t = dv.case_reference(shape, pattern, quad, bits, kind, mode, name)
                tab = tables(name, pattern, bits)
                # both store paths (aligned planes, planes at odd addresses), each with and without the total plane, from a plain and from a
                # pitched source
                for aligned, extra, with_total in ((True, dv.pitch_extra(shape), True), (False, 5, True), (True, 5, False), (False, dv.pitch_extra(shape), False)):
                    v, t, clean = _run(m, pattern, quad, bits, mode, tab, aligned, extra, with_total)
                    what = (shape, pattern, quad, bits, kind, mode, name, "aligned" if aligned else "odd address, pitched")
                    assert clean, ("a byte outside the planes was written", what)
                    assert np.array_equal(v, ref_v), ("views", what, np.argwhere(v != ref_v)[:4])
                    assert t is None or np.array_equal(t, ref_t), ("total", what, np.argwhere(t != ref_t)[:4])


@pytest.mark.parametrize("pattern,bits", [("mono", 8), ("rggb", 12)])
def test_odd_planes_with_total_and_source_alignment(pattern, bits, tables):
    """The total plane through the byte-store path, and a frame that starts 0, 1, 2 or 4 samples into a row of a wider buffer (the 4-sample
    accesses and the single ones): the same bits."""
    shape, quad, name = (20, 40), dr.SONY_QUAD, "wb_srgb"
    tab = tables(name, pattern, bits)
    for mode in dr.MODES:
        m, ref_v, ref_t = dv.case_reference(shape, pattern, quad, bits, "random", mode, name)
        v, t, clean = _run(m, pattern, quad, bits, mode, tab, False, 5, True)
        assert clean and np.array_equal(v, ref_v) and np.array_equal(t, ref_t)
        for shift in (0, 1, 2, 4):
            buf = np.full((shape[0], 48), np.iinfo(m.dtype).max, dtype=m.dtype)
            buf[:, shift:shift + shape[1]] = m
            src = torch.from_numpy(buf).cuda()
            n = ref_t.size
            pool, offs = _carve(n, True)
            base = pool.data_ptr()
            rc = _call(src.data_ptr() + shift * m.dtype.itemsize, bits, shape[0], shape[1], 48, dr.PATTERNS.index(pattern), quad, dr.MODES.index(mode),
                       [base + o for o in offs[:4]], base + offs[4], tab[0].data_ptr(), tab[1].data_ptr(), tab[2])
            assert rc == 0, _lib().shm_last_error()
            got = pool.cpu().numpy()
            assert all(np.array_equal(got[offs[k]:offs[k] + n].reshape(ref_t.shape), ref_v[k]) for k in range(4)), (mode, shift)
            assert np.array_equal(got[offs[4]:offs[4] + n].reshape(ref_t.shape), ref_t), (mode, shift)


def test_refusals_leave_the_destination_untouched(tables):
    h, w = 8, 12
    src = torch.zeros((h, w + 3), dtype=torch.uint16, device="cuda")
    pool, offs = _carve(h * w * 3, True)
    base = pool.data_ptr()
    ptrs = [base + o for o in offs[:4]]
    params, lut, mirror = tables("ccm_gamma", "rggb", 12)
    mono = tables("pedestal", "mono", 12)
    good = dict(src=src.data_ptr(), bits=12, h=h, w=w, pitch=w + 3, pattern=1, quad=dr.SONY_QUAD, mode=0, ptrs=ptrs, total=base + offs[4],
                params=params.data_ptr(), lut=lut.data_ptr(), mirror=mirror)
    assert _call(**good) == 0 and _call(**dict(good, pattern=0, mirror=mono[2], params=mono[0].data_ptr())) == 0
    torch.cuda.synchronize()
    pool.fill_(POISON)

    def changed(**words):
        m = (C.c_int * dv.NPARAMS)(*mirror)
        for k, val in words.items():
            m[int(k[1:])] = val
        return dict(mirror=m)
    bad = [dict(src=None), dict(quad=None), dict(ptrs=None), dict(ptrs=ptrs[:2] + [None] + ptrs[3:]), dict(bits=7), dict(bits=17), dict(h=3), dict(w=3),
           dict(h=32769), dict(w=32769, pitch=40000), dict(pattern=0, h=1, mirror=mono[2]), dict(pitch=w - 1), dict(pattern=5), dict(pattern=-1), dict(mode=2),
           dict(mode=-1), dict(quad=(0, 1, 2, 2)), dict(quad=(0, 1, 2, 4)), dict(quad=(-1, 1, 2, 3)),
           # what the development adds: null tables, a misaligned table, a mirror out of range, and a mono sensor with colour parameters
           dict(params=None), dict(lut=None), dict(mirror=None), dict(lut=lut.data_ptr() + 4), changed(w0=-1), changed(w2=65520), changed(w4=65535),
           changed(w9=2), changed(w9=3), changed(w10=8192), changed(w18=-8192), dict(pattern=0),
           dict(pattern=0, **changed(w9=0, w1=mirror[0] + 1)), dict(pattern=0, **changed(w9=0, w5=mirror[3] + 1))]
    for change in bad:
        rc = _call(**dict(good, **change))
        assert rc == E_SHAPE, (change, rc)
        assert b"shm_dofp_develop" in _lib().shm_last_error(), change
    # ... and the grey-world entry point's
    ws = torch.full((dv_ws(),), -1, dtype=torch.int64, device="cuda")
    out = torch.full((dv.NPARAMS,), -1, dtype=torch.int32, device="cuda")
    gw = dict(src=src.data_ptr(), bits=12, h=h, w=w, pitch=w + 3, pattern=1, params=params.data_ptr(), sat=4095, out=out.data_ptr(), ws=ws.data_ptr())
    wb = lambda a: _lib().shm_dofp_wb_gray(a["src"], a["bits"], a["h"], a["w"], a["pitch"], a["pattern"], a["params"], a["sat"], a["out"], a["ws"], _stream())
    for change in (dict(src=None), dict(params=None), dict(out=None), dict(ws=None), dict(bits=7), dict(bits=17), dict(pattern=0), dict(pattern=5),
                   dict(h=3), dict(w=3), dict(h=32769), dict(pitch=w - 1), dict(sat=0), dict(sat=65537)):
        assert wb(dict(gw, **change)) == E_SHAPE, change
        assert b"shm_dofp_wb_gray" in _lib().shm_last_error(), change
    torch.cuda.synchronize()
    assert bool((pool == POISON).all()) and bool((ws == -1).all()) and bool((out == -1).all())
    assert wb(gw) == 0
    torch.cuda.synchronize()


def dv_ws():
    from shmgan_amd import ops
    return ops.DOFP_WB_WS


# ---- grey-world ----------------------------------------------------------------------------------------------------------------------------
BIG = (1500, 1504)          # 375 x 376 periods: more than one pass of the capped grid (512 blocks of 256 threads); 12-bit mixed data only
GRAY_SHAPES = ((4, 4), (5, 7), (37, 66), (9, 1031), (261, 12), BIG)


def _layout(pattern, quad, bits, develop=None):
    from shmgan_amd.polar import DofpLayout
    angles = (0, 45, 90, 135)
    return DofpLayout(pattern, tuple(angles[q] for q in quad), bits, develop)


@pytest.mark.parametrize("pattern", dr.PATTERNS[1:])
def test_wb_gray_sums_and_gains(pattern):
    from shmgan_amd import ops, polar
    for shape in GRAY_SHAPES:
        for bits, kinds in ((8, ("random", "max")), (12, ("random", "mixed", "max", "over")), (16, ("mixed",))):
            top = 1 << bits
            develop = polar.DofpDevelop(black=(top // 16, top // 16 + 1, top // 16 - 1), wb="gray")
            lay = _layout(pattern, dr.SONY_QUAD, bits, develop)
            params = develop.table(lay)[0]
            for kind in kinds:
                if shape == BIG and (bits, kind) != (12, "mixed"):
                    continue
                m = dv.gray_frame(shape, pattern, bits, kind)
                extra = dv.pitch_extra(shape)
                wide = torch.from_numpy(np.array(dr.pitched(m, shape[1] + extra, np.iinfo(m.dtype).max)[0] if extra else m)).cuda()
                for sat in (None, top // 2):
                    sums, gains = ops.dofp_wb_gray(wide[:, :shape[1]], lay, sat)
                    ref = dv.wb_gray(m, pattern, params, top - 1 if sat is None else sat)
                    assert (tuple(sums.cpu().tolist()), tuple(gains.cpu().tolist())) == ref, (shape, bits, kind, sat)
                    if kind == "max":
                        assert ref == ((0,) * 6, (1024,) * 3)


@pytest.mark.parametrize("pattern,bits,mode", [("rggb", 12, "bilinear"), ("gbrg", 16, "bin"), ("bggr", 8, "bilinear")])
def test_gray_through_ops_dofp_views(pattern, bits, mode):
    """wb="gray" through the tensor-level wrapper equals the restatement fed its own gains; and a fixed development through it."""
    from shmgan_amd import ops, polar
    shape, quad = (37, 66), dr.QUADS[1]
    top = 1 << bits
    develop = polar.DofpDevelop(black=top // 16, wb="gray", ccm=dv.CCM_MILD, tone="srgb", sat=top - top // 8)
    lay = _layout(pattern, quad, bits, develop)
    params, lut, _ = develop.table(lay)
    m = np.array(dv.gray_frame(shape, pattern, bits, "mixed"))
    m[:, : shape[1] // 2] //= 3                     # a frame that is not grey
    _, gains = dv.wb_gray(m, pattern, params, top - top // 8)
    assert gains != (1024, 1024, 1024)
    ref_v, ref_t = dv.develop(m, pattern, quad, bits, mode, dv.with_gains(params, gains), lut)
    wide = torch.from_numpy(np.array(dr.pitched(m, shape[1] + 5, np.iinfo(m.dtype).max)[0])).cuda()
    out = ops.dofp_views(wide[:, :shape[1]], lay, mode, total=True)
    assert len(out) == 5 and all(np.array_equal(out[k].cpu().numpy(), ref_v[k]) for k in range(4)) and np.array_equal(out[4].cpu().numpy(), ref_t)
    fixed = _layout(pattern, quad, bits, polar.DofpDevelop(black=top // 16, wb=(1.9, 1, 1.6), tone=2.2))
    fp, fl, _ = fixed.develop.table(fixed)
    ref_v, _ = dv.develop(m, pattern, quad, bits, mode, fp, fl)
    out = polar.demosaic(m, fixed, mode)
    assert len(out) == 4 and all(np.array_equal(out[k].cpu().numpy(), ref_v[k]) for k in range(4))
    assert (fixed, torch.device("cuda", torch.cuda.current_device())) in ops._DOFP_TABLES          # uploaded once, kept
    kept = ops._DOFP_TABLES[(fixed, torch.device("cuda", torch.cuda.current_device()))]
    polar.demosaic(m, fixed, mode)
    assert ops._DOFP_TABLES[(fixed, torch.device("cuda", torch.cuda.current_device()))] is kept


def test_nothing_between_the_estimate_and_the_development_waits_for_the_device():
    """By inspection of the code, not by timing: the path from ops.dofp_views to its two entry points names nothing that synchronises the host
    (a read-back, an item(), a synchronize) once the tables are on the device; the gains travel in the parameter block."""
    from shmgan_amd import ops
    for fn in (ops.dofp_views, ops._dofp_wb_gray):
        src = inspect.getsource(fn)
        for word in (".cpu(", ".item(", ".tolist(", "synchronize", ".numpy(", "non_blocking=False"):
            assert word not in src, (fn.__name__, word)
    body = inspect.getsource(ops.dofp_views)
    assert body.index("_dofp_tables(") < body.index("_dofp_wb_gray(") < body.index("shm_dofp_develop(")
    assert ".to(" not in inspect.getsource(ops._dofp_wb_gray) and ".to(" not in body          # the one upload is _dofp_tables', once per layout


# ---- plumbing by equivalence ----------------------------------------------------------------------------------------------------------------
N_SAMPLES = 3
VIEW_DIRS = ("I0", "I45", "I90", "I135")


@pytest.fixture(scope="module", params=dr.MODES)
def capture(request, tmp_path_factory):
    """Random 12-bit RGGB mosaics of 48 x 64 and the restatement's developed views of them as PNGs in four view directories."""
    from PIL import Image
    from shmgan_amd import polar
    mode = request.param
    root = tmp_path_factory.mktemp(f"develop_{mode}")
    pattern, quad, bits = "rggb", dr.QUADS[1], 12
    develop = polar.DofpDevelop(black=(250, 240, 245), white=4000, wb=(1.9, 1, 1.6), ccm=dv.CCM_MILD, tone="srgb")
    lay = _layout(pattern, quad, bits, develop)
    params, lut, _ = develop.table(lay)
    for d in ("DOFP", "ED", "TOT") + VIEW_DIRS:
        (root / d).mkdir(parents=True)
    rng = np.random.default_rng(dr.MODES.index(mode) + 11)
    for i in range(N_SAMPLES):
        m = rng.integers(0, 1 << bits, (48, 64)).astype(np.uint16)
        v, t = dv.develop(m, pattern, quad, bits, mode, params, lut)
        Image.fromarray(m).save(root / "DOFP" / f"s{i}.png")
        for k, d in enumerate(VIEW_DIRS):
            Image.fromarray(v[k]).save(root / d / f"s{i}.png")
        Image.fromarray(t).save(root / "TOT" / f"s{i}.png")
        Image.fromarray(rng.integers(0, 256, t.shape).astype(np.uint8)).save(root / "ED" / f"s{i}.png")
    return SimpleNamespace(root=str(root), mode=mode, dofp=dict(capture="dofp", dofp=lay, dofp_demosaic=mode))


def _passes(ds, passes):
    out = [[t.clone() for t in ds.batch(i, p)] for p in range(passes) for i in range(len(ds))]
    torch.cuda.synchronize()
    return out


def _same(a, b):
    return len(a) == len(b) and all(len(x) == len(y) and all(torch.equal(s, t) for s, t in zip(x, y)) for x, y in zip(a, b))


def _loaders(capture, **kw):
    from shmgan_amd.data import PolarDataset
    kw = dict(dict(image_size=32, batch_size=1, rank=0, world=1), **kw)
    return (PolarDataset(capture.root, subdirs=VIEW_DIRS + ("ED",), **kw), PolarDataset(capture.root, subdirs=("DOFP", "ED"), **capture.dofp, **kw))


@pytest.mark.parametrize("source", ["dir", "min", "stokes"])
def test_loader_equivalence(capture, source):
    plain_v, plain_d = _loaders(capture, diffuse_source=source)
    ref = _passes(plain_v, 1)
    assert plain_d.n == N_SAMPLES and _same(ref, _passes(plain_d, 1))
    cv, cd = _loaders(capture, cache="device", cache_bytes=8 << 20, diffuse_source=source)
    got_v, got_d = _passes(cv, 2), _passes(cd, 2)
    assert _same(ref + ref, got_v) and _same(ref + ref, got_d)
    stats = cd.cache_stats()                      # the cache holds the DEVELOPED views, under the same keys
    assert stats == cv.cache_stats() and stats["resident"] == N_SAMPLES and stats["hits"] == N_SAMPLES and stats["refused"] == 0


def test_eval_loader_equivalence(capture):
    from shmgan_amd.data import EvalDataset
    photos, mosaics, ed = (os.path.join(capture.root, d) for d in ("TOT", "DOFP", "ED"))
    ev = EvalDataset(photos, 32, 2, ed, keep_source=True)
    ed_ = EvalDataset(mosaics, 32, 2, ed, keep_source=True, **dict(capture.dofp, dofp_test_view="total"))
    assert len(ev) == len(ed_) == 2
    for i, ((a, da), (b, db)) in enumerate(zip(ev, ed_)):
        assert torch.equal(a, b) and torch.equal(da, db)
        assert all(torch.equal(p, q) for p, q in zip(ev.last_source[0], ed_.last_source[0]))


def test_estimate_white_balance(capture, tmp_path):
    """The capture-wide balance: the sums of every frame added, finished by the same integer arithmetic."""
    from PIL import Image
    from shmgan_amd import polar
    lay = capture.dofp["dofp"]
    params = lay.develop.table(lay)[0]
    total = [0] * 6
    for i in range(N_SAMPLES):
        m = np.array(Image.open(os.path.join(capture.root, "DOFP", f"s{i}.png"))).astype(np.uint16)
        total = [a + b for a, b in zip(total, dv.wb_gray(m, "rggb", params, 3000)[0])]
    gains = dv.gains_of(total)
    assert polar.estimate_white_balance(capture.root, lay, sat=3000) == tuple(g / min(gains) for g in gains)
    with pytest.raises(ValueError, match="Bayer"):
        polar.estimate_white_balance(capture.root, polar.DofpLayout())
