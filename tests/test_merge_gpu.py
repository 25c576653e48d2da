"""shm_dofp_merge (csrc/dofp_merge.hip) and everything built on it, on the device.

The kernel is compared bit for bit with the NumPy restatement (tests/merge_ref.py, which tests/test_merge_cpu.py holds against a
per-photosite brute force and the exact quotient): 1 x 1, ragged and multi-block shapes, uint8 and uint16 at 8 / 12 / 16 bits, brackets of
2, 3 and 8 pages, physical and junk data with every mask of valid pages, with and without counts, and the access paths -- pages as offset,
pitched views of one buffer of which some pass the wide test and others fail it, destinations carved out of a poisoned pool at aligned and
odd element offsets with nothing outside them written.  The plumbing is tested by equivalence: a bracketed layout must give exactly what
layout.merged gives of the restatement-merged mosaic.  No tolerance anywhere."""
import ctypes as C
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import calibrate_ref as cr
import dofp_ref as dr
import merge_ref as mr

pytestmark = pytest.mark.gpu

POISON = 0xA5
WORD = 0xA5A5
E_SHAPE = -1


def _lib():
    from shmgan_amd import _lib as L
    return L.lib()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _mirror(exposures, bits):
    return (C.c_uint * 256)(*[int(v) for v in mr.table(exposures, bits)])


@pytest.fixture(scope="module")
def device_table():
    made = {}

    def get(exposures, bits):
        if (exposures, bits) not in made:
            made[(exposures, bits)] = (torch.from_numpy(mr.table(exposures, bits)).cuda(), _mirror(exposures, bits))
        return made[(exposures, bits)]
    return get


def _run(pages, shifts, spitch, bits, tab, black, white, dst_off, dpitch, counts):
    """The kernel on pages laid into ONE device buffer, page k starting shifts[k] elements past its slot of h * spitch + 16, gaps holding
    the largest value, into a poisoned pool from element dst_off on, rows dpitch apart: (dst [h,w], True if everything else in the pool
    still holds the poison, counts int64 [9] or None)."""
    n, h, w = pages.shape
    top = np.iinfo(pages.dtype).max
    slot = h * spitch + 16
    buf = np.full(n * slot, top, dtype=pages.dtype)
    offs = [k * slot + shifts[k] for k in range(n)]
    for k in range(n):
        buf[offs[k]:offs[k] + h * spitch].reshape(h, spitch)[:, :w] = pages[k]          # shifts are at most 8: inside the slot
    dev = torch.from_numpy(buf).cuda()
    size = pages.dtype.itemsize
    ptrs = (C.c_void_p * n)(*[dev.data_ptr() + o * size for o in offs])
    pool = torch.full((2 * (dst_off + h * dpitch + 64),), POISON, dtype=torch.uint8, device="cuda")
    cnt = torch.full((9 * 4,), POISON, dtype=torch.uint8, device="cuda").view(torch.int32) if counts else None          # the call clears it
    rc = _lib().shm_dofp_merge(ptrs, n, bits, h, w, spitch, tab[0].data_ptr(), tab[1], black, white, pool.data_ptr() + 2 * dst_off, dpitch,
                               None if cnt is None else cnt.data_ptr(), _stream())
    assert rc == 0, (rc, _lib().shm_last_error())
    got = pool.cpu().numpy().view(np.uint16)
    outside = np.ones(got.shape, dtype=bool)
    for y in range(h):
        outside[dst_off + y * dpitch:dst_off + y * dpitch + w] = False
    dst = got[dst_off:dst_off + h * dpitch].reshape(h, dpitch)[:, :w]
    return dst, bool(np.all(got[outside] == WORD)), None if cnt is None else cnt.cpu().numpy().astype(np.int64)


@pytest.mark.parametrize("shape", mr.SHAPES, ids=str)
def test_kernel_bit_exact(shape, device_table):
    """cr.MULTI_BLOCK (9 x 1032) needs 3 x 3 blocks of the launch as built -- 64 x 4 threads of 8 samples -- with every access wide;
    cr.MULTI_BLOCK_RAGGED (6 x 1030) is the same with a last group of 6 samples."""
    h, w = mr.shape_of(shape)
    extra = mr.pitch_extra(w)
    for _, bits, exposures, kind in mr.all_cases((shape,)):
        pages, black, white = mr.case(shape, bits, exposures, kind)
        ref, ref_counts = mr.case_reference(shape, bits, exposures, kind)
        n = len(exposures)
        tab = device_table(exposures, bits)
        # tight to tight; pitched to pitched, all aligned; a pitch that is no multiple of 8 to an odd element offset
        for name, spitch, dst_off, dpitch in (("tight", w, 64, w), ("pitched", w + extra, 64, w + extra), ("odd", w + 5, 61, w + 3)):
            for counts in (False, True):
                got, clean, cnt = _run(pages, [0] * n, spitch, bits, tab, black, white, dst_off, dpitch, counts)
                what = (shape, bits, exposures, kind, name, counts)
                assert clean, ("an element outside the destination rows was written", what)
                assert np.array_equal(got, ref), (what, np.argwhere(got != ref)[:4])
                if counts:
                    assert np.array_equal(cnt, ref_counts), (what, cnt, ref_counts)


@pytest.mark.parametrize("bits,exposures", [(8, (1, 4, 16)), (12, (1000, 250, 62)), (16, (1, 2, 4, 8, 16, 32, 64, 128))])
def test_page_and_destination_alignment(bits, exposures, device_table):
    """Each page and the destination are judged separately: pages that start 0, 1, 2, 4 or 8 samples into their slots of one buffer with a
    pitch of a multiple of 8 -- so that some are read wide and others one element at a time in the same launch -- and destinations at
    aligned and odd offsets, give the same bits; so does a width that is no multiple of 8."""
    tab = device_table(exposures, bits)
    n = len(exposures)
    for shape in ((20, 40), (13, 18)):
        h, w = shape
        pages, black, white = mr.case(shape, bits, exposures, "junk")
        ref, ref_counts = mr.case_reference(shape, bits, exposures, "junk")
        for shifts in ([0] * n, [(0, 1, 8, 4, 2, 0, 3, 8)[k] for k in range(n)], [(1, 0, 0, 0, 0, 0, 0, 0)[k] for k in range(n)]):
            for dst_off, dpitch in ((64, 48), (65, 48), (64, 43)):
                got, clean, cnt = _run(pages, shifts, 48, bits, tab, black, white, dst_off, dpitch, True)
                assert clean and np.array_equal(got, ref) and np.array_equal(cnt, ref_counts), (shape, shifts, dst_off, dpitch)


def test_refusals_leave_destination_and_counts_untouched(device_table):
    h, w = 8, 12
    exposures = (1, 4, 16)
    tab = device_table(exposures, 12)
    pages = torch.zeros((3, h, w + 4), dtype=torch.uint16, device="cuda")
    pool = torch.full((2 * (h * (w + 4) + 64),), POISON, dtype=torch.uint8, device="cuda")
    cnt = torch.full((9 * 4,), POISON, dtype=torch.uint8, device="cuda")
    good = dict(ptrs=[pages[k].data_ptr() for k in range(3)], n=3, bits=12, h=h, w=w, spitch=w + 4, table=tab[0].data_ptr(), mirror=tab[1], black=64,
                white=4000, dst=pool.data_ptr() + 64, dpitch=w + 4, counts=cnt.data_ptr())

    def call(a):
        ptrs = None if a["ptrs"] is None else (C.c_void_p * 8)(*(a["ptrs"] + [None] * (8 - len(a["ptrs"]))))
        return _lib().shm_dofp_merge(ptrs, a["n"], a["bits"], a["h"], a["w"], a["spitch"], a["table"], a["mirror"], a["black"], a["white"], a["dst"],
                                     a["dpitch"], a["counts"], _stream())
    assert call(good) == 0 and call(dict(good, counts=None, h=1, w=1)) == 0
    torch.cuda.synchronize()
    assert int(cnt.view(torch.int32)[3]) == h * w and int(cnt.view(torch.int32).sum()) == h * w          # zeros are valid in all three pages
    pool.fill_(POISON)
    cnt.fill_(POISON)
    low, high = _mirror(exposures, 12), _mirror(exposures, 12)
    low[5], high[7] = 0, (1 << 24) + 1
    # dst == a page is refused with that page pointing at the pool, so that a launch would show there
    for change in (dict(ptrs=None), dict(ptrs=[good["ptrs"][0], None, good["ptrs"][2]]), dict(table=None), dict(mirror=None), dict(dst=None), dict(n=1),
                   dict(n=9), dict(bits=7), dict(bits=17), dict(h=0), dict(w=0), dict(h=32769), dict(w=32769, spitch=40000, dpitch=40000),
                   dict(spitch=w - 1), dict(dpitch=w - 1), dict(ptrs=[good["ptrs"][0], pool.data_ptr() + 64, good["ptrs"][2]]), dict(black=-1),
                   dict(black=4095, white=4096), dict(white=0), dict(white=4097), dict(white=64), dict(mirror=low), dict(mirror=high)):
        rc = call(dict(good, **change))
        assert rc == E_SHAPE, (change, rc)
        assert b"shm_dofp_merge" in _lib().shm_last_error(), change
    torch.cuda.synchronize()
    assert bool((pool == POISON).all()) and bool((cnt == POISON).all())


# ---- equivalence through the stack ------------------------------------------------------------------------------------------------------------
ANGLES = (0, 45, 90, 135)


def _layout(pattern, bits, develop=None, calibration=None, bracket=None):
    from shmgan_amd.polar import DofpLayout
    return DofpLayout(pattern, tuple(ANGLES[q] for q in dr.SONY_QUAD), bits, develop, calibration, bracket)


def _equal(a, b):
    return len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))


def _calibration(shape, pattern, bits):
    from shmgan_amd.polar import DofpCalibration
    _, dark, gain, defect, ped, white = cr.case(shape, pattern, bits, "random")
    return DofpCalibration(dark, gain, defect, ped, white, pattern, bits)


def _merged_ref(pages, layout):
    """The restatement of what a bracketed layout does to its pages: each calibrated, then merged at the layout's levels."""
    cal = layout.calibration
    if cal is not None:
        pages = np.stack([cr.calibrate(p, cal.pattern, cal.bits, cal.dark, cal.gain, cal.defect, cal.pedestal, cal.white_level) for p in pages])
    black, white = layout.bracket_levels
    return mr.merge(pages, layout.bracket.exposures, layout.bits, black, white)


@pytest.mark.parametrize("pattern,bits", [("rggb", 12), ("mono", 8), ("rggb", 16)])
def test_ops_merge_and_views(pattern, bits):
    from shmgan_amd import ops, polar
    shape, exposures = (37, 66), (1, 4, 16)
    pages, black, white = mr.case(shape, bits, exposures, "physical")
    ref, ref_counts = mr.case_reference(shape, bits, exposures, "physical")
    bracket = polar.DofpBracket(exposures, black, white)
    host = np.stack([dr.pitched(p, shape[1] + 5, np.iinfo(p.dtype).max)[0] for p in pages])
    wide = torch.from_numpy(host.copy()).cuda()
    dev = wide[:, :, :shape[1]]
    # the call on its own: from a bracket (its bits given), from a layout; a tensor or a list; a new contiguous tensor, the pages unwritten
    for arg, kw in ((bracket, dict(bits=bits)), (_layout(pattern, bits, bracket=bracket), {})):
        for p in (dev, list(dev.unbind(0))):
            out = ops.dofp_merge(p, arg, **kw)
            assert out.is_contiguous() and out.dtype == torch.uint16 and np.array_equal(out.cpu().numpy(), ref)
            out, cnt = ops.dofp_merge(p, arg, counts=True, **kw)
            assert np.array_equal(out.cpu().numpy(), ref) and np.array_equal(cnt.cpu().numpy().astype(np.int64), ref_counts)
    assert np.array_equal(wide.cpu().numpy(), host)
    key = (exposures, bits, torch.device("cuda", torch.cuda.current_device()))
    kept = ops._DOFP_MERGE_TABLES[key]                              # uploaded once per (bracket, bits, device), kept
    ops.dofp_merge(dev, polar.DofpBracket(exposures), bits=bits)
    assert ops._DOFP_MERGE_TABLES[key] is kept
    top = 1 << bits
    develops = [None, polar.DofpDevelop(black=top // 16, wb=(1.9, 1, 1.6) if pattern != "mono" else (1, 1, 1), tone="srgb")]
    if pattern != "mono":
        develops.append(polar.DofpDevelop(black=top // 16, wb="gray", sat=top - top // 8))
    for cal in (None, _calibration(shape, pattern, bits)):
        for br in (bracket, polar.DofpBracket(exposures)):          # given levels; the calibration's, or 0 and 2^bits - 1
            for develop in develops:
                lay = _layout(pattern, bits, develop, cal, br)
                fixed = torch.from_numpy(_merged_ref(pages, lay)).cuda()
                for mode in dr.MODES:
                    for total in (False, True):
                        assert _equal(ops.dofp_views(dev, lay, mode, total), ops.dofp_views(fixed, lay.merged, mode, total)), (cal, br, develop, mode, total)
                if pattern != "mono":
                    for sat in (None, top // 2):
                        want = ops.dofp_wb_gray(fixed, lay.merged, None if sat is None else min(65536, sat << (16 - bits)))
                        assert _equal(ops.dofp_wb_gray(dev, lay, sat), want), (cal, br, develop, sat)
                assert _equal(polar.demosaic(np.array(pages), lay, total=True), ops.dofp_views(fixed, lay.merged, "bilinear", True))
                out, cnt = polar.merge_bracket(np.array(pages), lay, counts=True)
                assert torch.equal(out, fixed) and int(cnt.sum()) == shape[0] * shape[1]
    # without a development the views are the top 8 bits of the merged frame
    v, t = dr.views(ref, pattern, dr.SONY_QUAD, 16)
    out = polar.demosaic(np.array(pages), _layout(pattern, bits, bracket=bracket), total=True)
    assert all(np.array_equal(out[k].cpu().numpy(), v[k]) for k in range(4)) and np.array_equal(out[4].cpu().numpy(), t)
    with pytest.raises(ValueError, match=r"dofp_views: 2 page\(s\) for a bracket of 3 exposures"):
        ops.dofp_views(dev[:2], _layout(pattern, bits, bracket=bracket))
    with pytest.raises(ValueError, match=r"dofp_merge: page 1 has a row pitch"):
        ops.dofp_merge([dev[0], dev[1].contiguous(), dev[2]], bracket, bits=bits)


def test_ops_merge_is_asynchronous():
    """By inspection of the code, not by timing: the path from ops.dofp_merge to the entry point names nothing that waits for the device."""
    import inspect
    from shmgan_amd import ops
    src = "".join(inspect.getsource(f) for f in (ops.dofp_merge, ops._dofp_merged, ops._dofp_pages, ops._dofp_merge_layout))
    assert not any(word in src for word in ("synchronize", ".cpu()", ".item()", ".tolist()", ".numpy()"))


N_SAMPLES = 3


@pytest.fixture(scope="module", params=dr.MODES)
def capture(request, tmp_path_factory):
    """Random 12-bit RGGB brackets of 48 x 64 as multi-page TIFFs in BRACKET/, the restatement-merged 16-bit PNGs in MERGED/."""
    from PIL import Image
    from shmgan_amd import polar
    mode = request.param
    root = tmp_path_factory.mktemp(f"merge_{mode}")
    pattern, bits, shape, exposures = "rggb", 12, (48, 64), (1, 4, 16)
    rng = np.random.default_rng(dr.MODES.index(mode) + 41)
    for d in ("BRACKET", "MERGED", "ED"):
        (root / d).mkdir(parents=True)
    for i in range(N_SAMPLES):
        L = rng.random(shape) ** 3 * 4500.0
        pages = np.stack([np.clip(np.rint(240 + L * e + rng.normal(0, 3, shape)), 0, 4095) for e in exposures]).astype(np.uint16)
        polar.write_bracket(str(root / "BRACKET" / f"s{i}.tif"), pages)
        Image.fromarray(mr.merge(pages, exposures, bits, 240, 4000)).save(root / "MERGED" / f"s{i}.png")
        Image.fromarray(rng.integers(0, 256, (shape[0] // (4 if mode == "bin" else 1), shape[1] // (4 if mode == "bin" else 1), 3)).astype(np.uint8)).save(root / "ED" / f"s{i}.png")
    common = dict(capture_format="dofp", dofp_pattern=pattern, dofp_demosaic=mode, dofp_wb=(1.8, 1, 1.5))
    bracketed = dict(common, dofp_bits=bits, dofp_dir="BRACKET", dofp_black=240, dofp_exposures=exposures, dofp_bracket_black=240, dofp_bracket_white=4000)
    merged = dict(common, dofp_bits=16, dofp_dir="MERGED", dofp_black=240 << 4, dofp_white=4000 << 4)
    return SimpleNamespace(root=str(root), mode=mode, bracketed=bracketed, merged=merged)


def _options(capture, which):
    from shmgan_amd.data import capture_options
    subdirs, kw = capture_options(SimpleNamespace(**getattr(capture, which)))
    return subdirs, kw


def _passes(ds, passes):
    out = [[t.clone() for t in ds.batch(i, p)] for p in range(passes) for i in range(len(ds))]
    torch.cuda.synchronize()
    return out


def _same(a, b):
    return len(a) == len(b) and all(len(x) == len(y) and all(torch.equal(s, t) for s, t in zip(x, y)) for x, y in zip(a, b))


def test_options_describe_the_same_merged_layout(capture):
    assert _options(capture, "bracketed")[1]["dofp"].merged == _options(capture, "merged")[1]["dofp"]


@pytest.mark.parametrize("source", ["dir", "stokes"])
def test_loader_equivalence(capture, source):
    from shmgan_amd.data import PolarDataset
    kw = dict(image_size=32, batch_size=1, rank=0, world=1, diffuse_source=source)
    sub_b, br = _options(capture, "bracketed")
    sub_m, mg = _options(capture, "merged")
    ref = _passes(PolarDataset(capture.root, subdirs=sub_m, **mg, **kw), 1)
    assert len(ref) == N_SAMPLES and _same(ref, _passes(PolarDataset(capture.root, subdirs=sub_b, **br, **kw), 1))
    cached = PolarDataset(capture.root, subdirs=sub_b, **br, cache="device", cache_bytes=8 << 20, **kw)
    assert _same(ref + ref, _passes(cached, 2))                      # the second pass from the cache, which holds the views of the merged frames
    stats = cached.cache_stats()
    assert stats["resident"] == N_SAMPLES and stats["hits"] == N_SAMPLES and stats["refused"] == 0


def test_mask_loader_writers_and_test_mode_equivalence(capture, tmp_path):
    from shmgan_amd import polar
    from shmgan_amd.data import EvalDataset, MaskDataset, NativeEvalDataset
    br, mg = _options(capture, "bracketed")[1], _options(capture, "merged")[1]
    mb = MaskDataset.from_polar(capture.root, 32, 2, subdirs=("BRACKET",), **br)
    mm = MaskDataset.from_polar(capture.root, 32, 2, subdirs=("MERGED",), **mg)
    assert mb.names == mm.names == [f"s{i}" for i in range(N_SAMPLES)] and all(torch.equal(a, b) for a, b in zip(mb.tensors(), mm.tensors()))
    files = lambda written: [(os.path.basename(p), open(p, "rb").read()) for p in written]
    wb = polar.write_specular_masks(capture.root, str(tmp_path / "mb"), subdirs=("BRACKET",), **br)
    wm = polar.write_specular_masks(capture.root, str(tmp_path / "mm"), subdirs=("MERGED",), **mg)
    assert files(wb) == files(wm) and len(wb) == N_SAMPLES
    assert open(tmp_path / "mb" / "masks.jsonl").read() == open(tmp_path / "mm" / "masks.jsonl").read()
    eb = polar.write_estimated_diffuse(capture.root, str(tmp_path / "eb"), subdirs=("BRACKET",), mode="stokes", **br)
    em = polar.write_estimated_diffuse(capture.root, str(tmp_path / "em"), subdirs=("MERGED",), mode="stokes", **mg)
    assert files(eb) == files(em) and len(eb) == N_SAMPLES
    assert polar.estimate_white_balance(capture.root, br["dofp"], "BRACKET") == polar.estimate_white_balance(capture.root, mg["dofp"], "MERGED")
    ed = os.path.join(capture.root, "ED")
    for view in ("total", 2):
        tb = EvalDataset(os.path.join(capture.root, "BRACKET"), 32, 2, ed, keep_source=True, **dict(br, dofp_test_view=view))
        tm = EvalDataset(os.path.join(capture.root, "MERGED"), 32, 2, ed, keep_source=True, **dict(mg, dofp_test_view=view))
        assert len(tb) == len(tm) == 2 and tb.sources(0) == [(p.replace("MERGED", "BRACKET").replace(".png", ".tif"), hw) for p, hw in tm.sources(0)]
        for (a, da), (b, db) in zip(tb, tm):
            assert torch.equal(a, b) and torch.equal(da, db)
            assert all(torch.equal(p, q) for p, q in zip(tb.last_source[0], tm.last_source[0]))
    nb = NativeEvalDataset(os.path.join(capture.root, "BRACKET"), ed, **br)
    nm = NativeEvalDataset(os.path.join(capture.root, "MERGED"), ed, **mg)
    if capture.mode == "bilinear":          # the binned planes are 12 x 16, below native mode's smallest side
        for i in range(N_SAMPLES):
            fb, fm = nb.batch(i), nm.batch(i)
            assert torch.equal(fb[0], fm[0]) and torch.equal(fb[1], fm[1]) and fb[2] == fm[2]
    # a file with another number of pages is refused by name before anything is launched
    os.makedirs(tmp_path / "cap" / "BRACKET")
    polar.write_bracket(str(tmp_path / "cap" / "BRACKET" / "s0.tif"), np.zeros((2, 48, 64), dtype=np.uint16))
    with pytest.raises(ValueError, match=r"s0\.tif holds 2 page\(s\)"):
        polar.write_specular_masks(str(tmp_path / "cap"), str(tmp_path / "out"), subdirs=("BRACKET",), **br)


def test_highlight_on_the_device():
    """The scene of tests/test_merge_cpu.py: from the longest page alone the mask has a hole at the core; from the bracket it covers it."""
    from shmgan_amd import polar
    s = mr.scene()
    plain = _layout("mono", 12)
    bracketed = _layout("mono", 12, bracket=polar.DofpBracket(mr.SCENE_EXPOSURES, mr.SCENE_BLACK, 4095))
    core = torch.from_numpy(s["core"]).cuda()
    mask, q, _ = polar.specular_mask(polar.demosaic(s["pages"][2], plain, "bin"), plain.angles)
    assert not bool(mask[core].any()) and int(q[core].max()) == 0
    mask, q, _ = polar.specular_mask(polar.demosaic(s["pages"], bracketed, "bin"), bracketed.angles)
    assert bool((mask[core] == 255).all()) and int(q[core].min()) > 100
    merged, cnt = polar.merge_bracket(s["pages"], bracketed, counts=True)
    assert np.array_equal(merged.cpu().numpy(), mr.merge(s["pages"], mr.SCENE_EXPOSURES, 12, mr.SCENE_BLACK, 4095)) and int(cnt[0]) == 0
