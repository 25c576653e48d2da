"""shm_dofp_views (csrc/dofp.hip) and everything built on it, on the device.

The kernel is compared bit for bit with the NumPy restatement (tests/dofp_ref.py, whose two forms tests/test_dofp_cpu.py holds
against a brute force with rational weights): views and total, both modes, every pattern, two quad layouts, 8 / 10 / 12 / 16 bits,
pitched sources, and destinations carved out of a poisoned buffer at 4-byte-aligned and at odd addresses (the dword and the byte
store paths).  The plumbing -- loader, mask loader, the two writers, test mode, one training run -- is tested by equivalence: a
mosaic directory must give exactly what today's four view directories give when they hold the restatement's views of those mosaics.
No tolerance anywhere: the arithmetic is integer and every comparison is equality."""
import ctypes as C
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import dofp_ref as dr

pytestmark = pytest.mark.gpu

POISON = 0xA5
E_SHAPE = -1


def _lib():
    from shmgan_amd import _lib as L
    return L.lib()


def _call(src, bits, h, w, pitch, pattern, quad, mode, ptrs, total):
    L = _lib()
    q = (C.c_int * 4)(*quad) if quad is not None else None
    dp = (C.c_void_p * 4)(*ptrs) if ptrs is not None else None
    return L.shm_dofp_views(src, bits, h, w, pitch, pattern, q, mode, dp, total, torch.cuda.current_stream().cuda_stream)


def _out_shape(h, w, pattern, mode):
    P = dr.period(pattern)
    return (h, w) if mode == "bilinear" else (h // P, w // P)


def _carve(n, aligned):
    """(pool, offsets of five planes of n bytes): 4-byte-aligned planes, or planes at odd addresses, each with guard bytes around."""
    first, stride = (64, (n + 3) // 4 * 4 + 8) if aligned else (61, n + 37)
    pool = torch.full((first + 5 * stride + 64,), POISON, dtype=torch.uint8, device="cuda")
    return pool, [first + i * stride for i in range(5)]


def _run(mosaic, pattern, quad, bits, mode, aligned, pitch_extra, with_total=True):
    """The kernel on `mosaic` (host array), from a source with row pitch w + pitch_extra whose gap holds the largest value, into
    carved planes: (views [4,ho,wo,3], total, True if every byte outside the planes still holds the poison)."""
    h, w = mosaic.shape
    buf = dr.pitched(mosaic, w + pitch_extra, np.iinfo(mosaic.dtype).max)[0] if pitch_extra else mosaic
    src = torch.from_numpy(np.array(buf)).cuda()            # a writable copy: the shared reference stays read-only
    ho, wo = _out_shape(h, w, pattern, mode)
    n = ho * wo * 3
    pool, offs = _carve(n, aligned)
    base = pool.data_ptr()
    rc = _call(src.data_ptr(), bits, h, w, w + pitch_extra, dr.PATTERNS.index(pattern), quad, dr.MODES.index(mode),
               [base + o for o in offs[:4]], base + offs[4] if with_total else None)
    assert rc == 0, (rc, _lib().shm_last_error())
    got = pool.cpu().numpy()
    outside = np.ones(got.shape, dtype=bool)
    planes = []
    for o in offs[:5 if with_total else 4]:
        planes.append(got[o:o + n].reshape(ho, wo, 3))
        outside[o:o + n] = False
    clean = bool(np.all(got[outside] == POISON))
    return np.stack(planes[:4]), (planes[4] if with_total else None), clean


@pytest.mark.parametrize("shape,pattern", dr.shape_pattern_pairs(), ids=lambda v: v if isinstance(v, str) else f"{v[0]}x{v[1]}")
def test_kernel_bit_exact(shape, pattern):
    h, w = shape
    for quad, bits, kind in dr.cases_of(shape, pattern):
        for mode in dr.MODES:
            if min(_out_shape(h, w, pattern, mode)) < 1:
                continue
            m, ref_v, ref_t = dr.case_reference(shape, pattern, quad, bits, kind, mode)
            for aligned, extra in ((True, 0), (False, 5)):
                v, t, clean = _run(m, pattern, quad, bits, mode, aligned, extra)
                what = (shape, pattern, quad, bits, kind, mode, "aligned" if aligned else "odd address, pitched")
                assert clean, ("a byte outside the planes was written", what)
                assert np.array_equal(v, ref_v), ("views", what, np.argwhere(v != ref_v)[:4])
                assert np.array_equal(t, ref_t), ("total", what, np.argwhere(t != ref_t)[:4])


def test_without_total_writes_four_planes():
    shape, pattern, quad = (13, 18), "rggb", dr.SONY_QUAD
    m, ref_v, _ = dr.case_reference(shape, pattern, quad, 12, "random", "bilinear")
    v, _, clean = _run(m, pattern, quad, 12, "bilinear", True, 0, with_total=False)
    assert clean and np.array_equal(v, ref_v)


@pytest.mark.parametrize("pattern,bits", [("mono", 8), ("mono", 12), ("bggr", 8), ("rggb", 12)])
def test_source_alignment(pattern, bits):
    """The kernel reads four samples at a time where base and pitch allow it and one at a time elsewhere: a frame that starts 0, 1, 2 or 4
    samples into a row of a wider buffer gives the same bits."""
    shape, quad = (20, 40), dr.SONY_QUAD
    for mode in dr.MODES:
        m, ref_v, ref_t = dr.case_reference(shape, pattern, quad, bits, "random", mode)
        for shift in (0, 1, 2, 4):
            buf = np.full((shape[0], 48), np.iinfo(m.dtype).max, dtype=m.dtype)
            buf[:, shift:shift + shape[1]] = m
            src = torch.from_numpy(buf).cuda()
            n = ref_t.size
            pool, offs = _carve(n, True)
            base = pool.data_ptr()
            rc = _call(src.data_ptr() + shift * m.dtype.itemsize, bits, shape[0], shape[1], 48, dr.PATTERNS.index(pattern), quad,
                       dr.MODES.index(mode), [base + o for o in offs[:4]], base + offs[4])
            assert rc == 0, _lib().shm_last_error()
            got = pool.cpu().numpy()
            assert all(np.array_equal(got[offs[v]:offs[v] + n].reshape(ref_t.shape), ref_v[v]) for v in range(4)), (mode, shift)
            assert np.array_equal(got[offs[4]:offs[4] + n].reshape(ref_t.shape), ref_t), (mode, shift)


def test_refusals_leave_the_destination_untouched():
    h, w = 8, 12
    src = torch.zeros((h, w + 3), dtype=torch.uint16, device="cuda")
    pool, offs = _carve(h * w * 3, True)
    base = pool.data_ptr()
    ptrs = [base + o for o in offs[:4]]
    tot = base + offs[4]
    good = dict(src=src.data_ptr(), bits=12, h=h, w=w, pitch=w + 3, pattern=1, quad=dr.SONY_QUAD, mode=0, ptrs=ptrs, total=tot)
    assert _call(**good) == 0
    torch.cuda.synchronize()
    pool.fill_(POISON)
    bad = [dict(src=None), dict(quad=None), dict(ptrs=None), dict(ptrs=ptrs[:2] + [None] + ptrs[3:]),
           dict(bits=7), dict(bits=17), dict(h=3), dict(w=3), dict(h=32769), dict(w=32769, pitch=40000),
           dict(pattern=0, h=1), dict(pattern=0, w=1), dict(pitch=w - 1), dict(pattern=5), dict(pattern=-1), dict(mode=2), dict(mode=-1),
           dict(quad=(0, 1, 2, 2)), dict(quad=(0, 1, 2, 4)), dict(quad=(-1, 1, 2, 3))]
    for change in bad:
        rc = _call(**dict(good, **change))
        assert rc == E_SHAPE, (change, rc)
        assert b"shm_dofp_views" in _lib().shm_last_error(), change
    torch.cuda.synchronize()
    assert bool((pool == POISON).all())
    # the smallest frames that are accepted: one period
    assert _call(**dict(good, h=4, w=4)) == 0 and _call(**dict(good, pattern=0, h=2, w=2)) == 0
    torch.cuda.synchronize()


def _layout(pattern, quad, bits):
    from shmgan_amd.polar import DofpLayout
    angles = (0, 45, 90, 135)
    return DofpLayout(pattern, tuple(angles[q] for q in quad), bits)


@pytest.mark.parametrize("pattern,bits", [("mono", 8), ("gbrg", 12), ("rggb", 16)])
def test_ops_dofp_views(pattern, bits):
    """The tensor-level wrapper: a layout's quad table, a pitched tensor view, new tensors of the right shape, the total on request."""
    from shmgan_amd import ops, polar
    shape, quad = (37, 66), dr.QUADS[1]
    lay = _layout(pattern, quad, bits)
    assert lay.quad == quad
    for mode in dr.MODES:
        m, ref_v, ref_t = dr.case_reference(shape, pattern, quad, bits, "random", mode)
        wide = torch.from_numpy(np.array(dr.pitched(m, shape[1] + 5, np.iinfo(m.dtype).max)[0])).cuda()
        out = ops.dofp_views(wide[:, :shape[1]], lay, mode, total=True)
        assert len(out) == 5 and all(o.dtype == torch.uint8 and tuple(o.shape) == ref_t.shape for o in out)
        assert all(np.array_equal(out[v].cpu().numpy(), ref_v[v]) for v in range(4)) and np.array_equal(out[4].cpu().numpy(), ref_t)
        out = polar.demosaic(np.array(m), lay, mode)                  # a host array is uploaded first
        assert len(out) == 4 and all(np.array_equal(out[v].cpu().numpy(), ref_v[v]) for v in range(4))
    with pytest.raises(ValueError):
        ops.dofp_views(torch.zeros((8, 8), dtype=torch.uint8, device="cuda"), lay if bits != 8 else _layout(pattern, quad, 12))
    with pytest.raises(TypeError):
        ops.dofp_views(torch.zeros((8, 8), dtype=torch.float32, device="cuda"), lay)


# ---- plumbing by equivalence ----------------------------------------------------------------------------------------------------------
# A capture of N_SAMPLES random mosaics, its views computed by the restatement and written as PNGs (lossless) into four view
# directories: whatever reads the mosaic directory must give exactly what today's code gives on the four directories.
N_SAMPLES = 3
VIEW_DIRS = ("I0", "I45", "I90", "I135")
CAPTURES = {"mono8": ("mono", dr.SONY_QUAD, 8), "rggb12": ("rggb", dr.QUADS[1], 12)}


@pytest.fixture(scope="module", params=[(c, m) for c in CAPTURES for m in dr.MODES], ids=lambda p: f"{p[0]}-{p[1]}")
def capture(request, tmp_path_factory):
    name, mode = request.param
    return _make_capture(tmp_path_factory.mktemp(f"dofp_{name}_{mode}"), name, mode)


def _make_capture(root, name, mode, view_dirs=VIEW_DIRS):
    from PIL import Image
    pattern, quad, bits = CAPTURES[name]
    for d in ("DOFP", "ED", "TOT") + tuple(view_dirs):
        (root / d).mkdir(parents=True)
    rng = np.random.default_rng(sorted(CAPTURES).index(name) * 2 + dr.MODES.index(mode))
    for i in range(N_SAMPLES):
        m = rng.integers(0, 1 << bits, (48, 64)).astype(np.uint8 if bits == 8 else np.uint16)
        v, t = dr.views(m, pattern, quad, bits, mode)
        Image.fromarray(m).save(root / "DOFP" / f"s{i}.png")
        for k, d in enumerate(view_dirs):
            Image.fromarray(v[k]).save(root / d / f"s{i}.png")
        Image.fromarray(t).save(root / "TOT" / f"s{i}.png")
        Image.fromarray(rng.integers(0, 256, t.shape).astype(np.uint8)).save(root / "ED" / f"s{i}.png")
    return SimpleNamespace(root=str(root), layout=_layout(pattern, quad, bits), mode=mode, bits=bits,
                           dofp=dict(capture="dofp", dofp=_layout(pattern, quad, bits), dofp_demosaic=mode))


def _passes(ds, passes):
    out = [[t.clone() for t in ds.batch(i, p)] for p in range(passes) for i in range(len(ds))]
    torch.cuda.synchronize()
    return out


def _same(a, b):
    return len(a) == len(b) and all(len(x) == len(y) and all(torch.equal(s, t) for s, t in zip(x, y)) for x, y in zip(a, b))


def _loaders(capture, **kw):
    from shmgan_amd.data import PolarDataset
    kw = dict(dict(image_size=32, batch_size=2, rank=0, world=1), **kw)
    return (PolarDataset(capture.root, subdirs=VIEW_DIRS + ("ED",), **kw),
            PolarDataset(capture.root, subdirs=("DOFP", "ED"), **capture.dofp, **kw))


@pytest.mark.parametrize("source", ["dir", "min", "stokes"])
def test_loader_equivalence(capture, source):
    from shmgan_amd.data import Augment
    plain_v, plain_d = _loaders(capture, diffuse_source=source)
    assert len(plain_d) == 1 and plain_d.n == N_SAMPLES
    ref = _passes(plain_v, 1)
    assert _same(ref, _passes(plain_d, 1))
    aug = dict(diffuse_source=source, augment=Augment(flip_lr=0.5, flip_ud=0.5, crop_min=0.5, views="physical"), shuffle=True, seed=3)
    aug_v, aug_d = _loaders(capture, **aug)
    assert aug_d._mirror[0] == "permute"                         # the layout's angles: the exact 45 / 135 exchange
    ref_aug = _passes(aug_v, 3)
    assert _same(ref_aug, _passes(aug_d, 3)) and not _same(ref_aug[:1], ref)
    for opts in (dict(diffuse_source=source), aug):
        cv, cd = _loaders(capture, cache="device", cache_bytes=8 << 20, batch_size=1, **opts)
        want1 = _passes(_loaders(capture, batch_size=1, **opts)[0], 2)
        got_v, got_d = _passes(cv, 2), _passes(cd, 2)
        assert _same(want1, got_v) and _same(want1, got_d)
        if "augment" not in opts:
            assert _same(got_d[:N_SAMPLES], got_d[N_SAMPLES:])  # the second pass, from the cache, equals the first
        stats = cd.cache_stats()                                 # the cache holds the demosaiced views, as it holds decoded ones
        assert stats == cv.cache_stats() and stats["resident"] == N_SAMPLES and stats["hits"] == N_SAMPLES and stats["refused"] == 0


def test_loader_refuses_a_diffuse_image_of_another_size(capture, tmp_path):
    import shutil
    from PIL import Image
    from shmgan_amd.data import PolarDataset
    shutil.copytree(os.path.join(capture.root, "DOFP"), tmp_path / "DOFP")
    (tmp_path / "ED").mkdir()
    for i in range(N_SAMPLES):
        Image.fromarray(np.zeros((47, 64, 3), dtype=np.uint8)).save(tmp_path / "ED" / f"s{i}.png")
    ds = PolarDataset(str(tmp_path), 32, 1, subdirs=("DOFP", "ED"), rank=0, world=1, **capture.dofp)
    with pytest.raises(ValueError, match=r"DOFP.s0\.png.*ED.s0\.png 47x64"):
        ds.batch(0)


def test_mask_loader_and_writers_equivalence(capture, tmp_path):
    from shmgan_amd import polar
    from shmgan_amd.data import MaskDataset
    mv = MaskDataset.from_polar(capture.root, 32, 2, subdirs=VIEW_DIRS)
    md = MaskDataset.from_polar(capture.root, 32, 2, subdirs=("DOFP",), **capture.dofp)
    assert md.names == mv.names == [f"s{i}" for i in range(N_SAMPLES)]
    assert all(torch.equal(a, b) for a, b in zip(mv.tensors(), md.tensors()))
    files = lambda written: [(os.path.basename(p), open(p, "rb").read()) for p in written]
    wv = polar.write_specular_masks(capture.root, str(tmp_path / "mv"), subdirs=VIEW_DIRS)
    wd = polar.write_specular_masks(capture.root, str(tmp_path / "md"), subdirs=("DOFP",), **capture.dofp)
    assert files(wv) == files(wd) and len(wd) == N_SAMPLES
    assert open(tmp_path / "mv" / "masks.jsonl").read() == open(tmp_path / "md" / "masks.jsonl").read()
    for mode in ("min", "stokes"):
        ev = polar.write_estimated_diffuse(capture.root, str(tmp_path / f"ev_{mode}"), subdirs=VIEW_DIRS, mode=mode)
        ed = polar.write_estimated_diffuse(capture.root, str(tmp_path / f"ed_{mode}"), subdirs=("DOFP",), mode=mode, **capture.dofp)
        assert files(ev) == files(ed) and len(ed) == N_SAMPLES


@pytest.mark.parametrize("view,views_dir", [(0, "I0"), (2, "I90"), ("total", "TOT")])
def test_eval_loader_equivalence(capture, view, views_dir):
    from shmgan_amd.data import EvalDataset, NativeEvalDataset
    photos, mosaics, ed = (os.path.join(capture.root, d) for d in (views_dir, "DOFP", "ED"))
    kw = dict(capture.dofp, dofp_test_view=view)
    ev = EvalDataset(photos, 32, 2, ed, keep_source=True)
    ed_ = EvalDataset(mosaics, 32, 2, ed, keep_source=True, **kw)
    assert len(ev) == len(ed_) == 2
    for i, ((a, da), (b, db)) in enumerate(zip(ev, ed_)):
        assert torch.equal(a, b) and torch.equal(da, db)
        assert [s[1] for s in ev.sources(i)] == [s[1] for s in ed_.sources(i)]
        assert all(torch.equal(p, q) for p, q in zip(ev.last_source[0], ed_.last_source[0]))         # what the detail transfer reads
    if capture.mode == "bilinear":                          # the binned planes are below the native mode's smallest side
        nv, nd = NativeEvalDataset(photos, ed), NativeEvalDataset(mosaics, ed, **kw)
        for i, ((fa, ta, wa), (fb, tb, wb)) in enumerate(zip(nv, nd)):
            assert torch.equal(fa, fb) and torch.equal(ta, tb) and wa == wb and nv.sources(i)[0][1] == nd.sources(i)[0][1]
    else:
        with pytest.raises(ValueError, match="at least 32 x 32"):
            NativeEvalDataset(mosaics, ed, **kw).batch(0)


def test_train_from_a_mosaic_directory(tmp_path):
    """One train() of two steps from the mosaic directory: it runs, and its losses are those of the four-directory run, bit for bit.
    (One capture: the loader's batches are compared above for all of them.)"""
    import argparse
    from shmgan_amd import ShmGANwithSSpecSeg
    from shmgan_amd.data import PSD_SUBDIRS
    capture = _make_capture(tmp_path / "data", "rggb12", "bilinear", PSD_SUBDIRS[:4])          # train() lists the PSD directory names
    losses = []
    for tag, extra in (("views", {}), ("dofp", dict(capture_format="dofp", dofp_pattern=capture.layout.pattern,
                                                     dofp_quad_angles=capture.layout.quad_angles, dofp_bits=capture.layout.bits))):
        args = argparse.Namespace(mode="train", image_size=32, batch_size=1, filter_size=16, num_epochs=1, data_dir=str(tmp_path / "data"),
                                  checkpoint_save_dir=str(tmp_path / tag / "ckpt"), log_dir=str(tmp_path / tag / "logs"), log_step=1,
                                  checkpoint_save_step=1, **extra)
        m = ShmGANwithSSpecSeg(args)
        assert m.train(args, max_steps=2, print_fn=lambda *a: None) == 2
        torch.cuda.synchronize()
        assert m.loadedDataset.capture == tag
        losses.append(m.losses())
    assert np.isfinite(losses[0]["total_Generator_loss"]) and sorted(losses[0]) == sorted(losses[1])
    assert all(np.array_equal(losses[0][k], losses[1][k]) for k in losses[0]), (losses[0], losses[1])
