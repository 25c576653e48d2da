"""The NumPy restatement of the specular-mask kernels (tests/specmask_ref.py) checked against independent formulations, the
teeth of the GPU comparison (modelled kernel faults change the result on the very inputs tests/test_specmask_gpu.py uses), the
host surface that needs no GPU, and the quality of the reference pipeline on the synthetic scenes, from which the floors of the
GPU suite come.  No GPU."""
import numpy as np
import pytest

import specmask_ref as R


def _psd():
    from shmgan_amd.polar import stokes_matrix
    return stokes_matrix(R.PSD_ANGLES)


def test_textbook_matrices_are_integer_and_strengths_agree_exactly():
    """Rows 1 and 2 of stokes_matrix([0,45,90,135]) are exactly 0 / +-1, as are REFERENCE_DOP_MATRIX's: the integer strength, the
    float64 one and the float32 one give the same q, and (int) sqrt of the float32 e is the integer square root for every e the
    kernel can meet."""
    from shmgan_amd.polar import REFERENCE_DOP_MATRIX, stokes_matrix
    tb = stokes_matrix(R.TEXTBOOK_ANGLES)
    assert tb.dtype == np.float32 and np.array_equal(tb[1:], np.array([[1, 0, -1, 0], [0, 1, 0, -1]], dtype=np.float32))
    assert REFERENCE_DOP_MATRIX == R.DOP_MATRIX
    ints = np.vstack([np.zeros((1, 4)), tb[1:]])
    for h, w in R.SHAPES:
        views = R.random_views(h, w)
        e = R.strength_int(views, ints)
        assert np.array_equal(R.strength_int(views, R.DOP_MATRIX), e)            # the same rows 1 and 2
        for dtype in (np.float64, np.float32):
            p = R.strength(views, tb, dtype)
            assert float(p.max()) ** 2 < 2 ** 24
            assert np.array_equal(R.quantise(p), R.q_int(views, ints)), (h, w, dtype)
    # every e <= 2 * 510^2: float32 holds it, and floor(sqrtf(e)) is the integer square root
    e = np.arange(0, 2 * 510 * 510 + 1, dtype=np.int64)
    assert np.array_equal(np.floor(np.sqrt(e.astype(np.float32))).astype(np.int64), R.isqrt(e))


def test_clamp_and_near_integer_cap_on_the_gpu_suite_inputs():
    """Random bytes clamp about a quarter of the pixels at 255, and the pixels at which the PSD comparison excuses a difference
    stay under the 1 % cap at every shape of the GPU suite (a property of the inputs and the float32 restatement alone)."""
    coef = _psd()
    for h, w in R.SHAPES + [R.PAST_CAP_SHAPE]:
        views = R.random_views(h, w)
        p64, err32, bound, excusable = R.near_integer(views, coef)
        q64, q32 = R.quantise(p64), R.quantise(R.strength(views, coef, np.float32))
        print(f"specmask {h}x{w}: float32 restatement error {err32:.2e}, excusable {int(excusable.sum())} of {h * w}, q32 != q64 at {int((q32 != q64).sum())}, "
              f"clamped {float((q64 == 255).mean()):.3f}")
        assert excusable.sum() <= 0.01 * h * w
        diff = q32 != q64
        assert np.all(excusable[diff]) and np.abs(q32.astype(int) - q64.astype(int)).max(initial=0) <= 1
        if h * w >= 1000:
            assert 0.2 < (q64 == 255).mean() < 0.35


def _brute_otsu(hist):
    """Two-class between-class variance from the definition: w0 w1 (mu1 - mu0)^2 over the pixel list, scaled by N^2."""
    vals = np.repeat(np.arange(256), hist)
    scores = np.zeros(256)
    for t in range(256):
        a, b = vals[vals <= t], vals[vals > t]
        if a.size and b.size:
            scores[t] = float(a.size) * float(b.size) * (b.mean() - a.mean()) ** 2
    return scores


def test_otsu_against_brute_force():
    rng = np.random.default_rng(5)
    hists = [rng.integers(0, 50, 256), rng.integers(0, 3, 256) * rng.integers(0, 2, 256), R.histogram(R.quantise(R.strength(R.random_views(37, 53), _psd()))),
             R.OTSU_CASES["two_spikes"][0], R.OTSU_CASES["uniform"][0]]
    for h in hists:
        ref, brute = R.otsu_scores(h), _brute_otsu(h)
        assert np.allclose(ref, brute, rtol=1e-10, atol=0)
        top = brute.max()
        assert ref[R.otsu(h)] >= top * (1 - 1e-10)
    for name, (h, t) in R.OTSU_CASES.items():
        sc = R.otsu_scores(h)
        assert R.otsu(h) == t, name
        # a unique best PARTITION (or no split at all): the t of maximal var(t) all cut between the same two occupied bins, so their
        # scores come from identical integers and the lowest-t rule decides exactly, not by rounding
        best = np.flatnonzero(sc == sc.max())
        assert sc.max() == 0 or len(set(np.cumsum(h)[best])) == 1, name
    assert R.t_eff(0) == R.FLOOR and R.t_eff(40) == 40 and R.t_eff(40, fixed=7) == 7 and R.t_eff(3, floor=0) == 3


def test_morphology_against_scipy():
    ndi = pytest.importorskip("scipy.ndimage")
    for h, w in R.SHAPES:
        for kind in ("busy", "single", "full"):
            b = np.asarray(R.morph_q(h, w, kind)) > 100
            for r in (0, 1, 2, 4, 8, 12):
                if r == 0:
                    assert np.array_equal(R.erode(b, 0), b) and np.array_equal(R.dilate(b, 0), b)
                    continue
                st = np.ones((2 * r + 1, 2 * r + 1), dtype=bool)
                assert np.array_equal(R.erode(b, r), ndi.binary_erosion(b, st, border_value=1)), (h, w, kind, r)
                assert np.array_equal(R.dilate(b, r), ndi.binary_dilation(b, st, border_value=0)), (h, w, kind, r)


def test_two_dilations_are_one():
    """What lets the kernel run the opening's dilation and the rim dilation as ONE launch, border rule included."""
    for h, w in R.SHAPES:
        b = np.asarray(R.morph_q(h, w, "busy")) > 100
        for ro, rd in R.RADII:
            e = R.erode(b, ro)
            assert np.array_equal(R.dilate(R.dilate(e, ro), rd), R.dilate(e, ro + rd)), (h, w, ro, rd)


def test_opening_removes_a_single_pixel_and_keeps_a_full_frame():
    for h, w in R.SHAPES:
        for ro, rd in R.RADII:
            m, c = R.morph(R.morph_q(h, w, "single"), 100, ro, rd)
            if ro >= 1 and (h, w) != (1, 1):
                assert c == 0 and not m.any(), (h, w, ro, rd)
            else:
                assert c >= 1
            m, c = R.morph(R.morph_q(h, w, "full"), 100, ro, rd)
            assert c == h * w and np.all(m == 255)                           # no erosion from the border: outside taps are skipped


def test_modelled_faults_change_the_result_on_the_gpu_suite_inputs():
    """The exact comparisons of the GPU suite have teeth: each modelled kernel fault gives another mask / histogram on inputs
    the suite uses."""
    # an off-by-one threshold: q >= t_eff.  The busy maps hold the value t_eff itself when t_eff is taken from the map
    hit = 0
    for h, w in R.SHAPES:
        q = R.morph_q(h, w, "busy")
        te = int(np.sort(q.ravel())[q.size // 2])                             # a value the map contains
        for ro, rd in R.RADII:
            hit += R.fault_threshold_off_by_one(q, te, ro, rd)[1] != R.morph(q, te, ro, rd)[1]
    assert hit > 0
    views = R.random_views(64, 64)
    mask, q, (t, te, count) = R.pipeline(views, _psd(), ro=0, rd=0)
    assert (q == te).any() and R.fault_threshold_off_by_one(q, te, 0, 0)[1] > count
    # a border that eats the edge: the busy maps' bands lean on a border and survive an erosion only under the skip-outside rule (a
    # full frame would not show it: the opening's dilation grows the eaten rim back)
    for h, w in R.SHAPES:
        if h >= 37 and w >= 53:
            q = R.morph_q(h, w, "busy")
            for ro, rd in R.RADII:
                if ro >= 1:
                    assert not np.array_equal(R.fault_border_eats_edge(q, 100, ro, rd)[0], R.morph(q, 100, ro, rd)[0]), (h, w, ro, rd)
    # a histogram that drops the last partial block, at every shape that is no multiple of the block
    for h, w in R.SHAPES + [R.PAST_CAP_SHAPE]:
        q = R.quantise(R.strength(R.random_views(h, w), _psd()))
        if (h * w) % 1024:
            assert not np.array_equal(R.fault_histogram_drops_tail(q), R.histogram(q)), (h, w)
    # 16-bit counters: the constant image
    h, w = R.CONSTANT_SHAPE
    assert h * w > 2 ** 16
    q = np.full((h, w), 93, dtype=np.uint8)
    assert R.histogram(q)[93] == h * w and not np.array_equal(R.fault_histogram_wraps16(q), R.histogram(q))


def test_past_cap_shape_is_past_the_cap():
    csrc = (__import__("pathlib").Path(__file__).resolve().parent.parent / "shmgan_amd" / "csrc" / "specmask.hip").read_text()
    import re
    nt, px, blocks = (int(re.search(rf"constexpr int {k} = (\d+);", csrc).group(1)) for k in ("SM_NT", "SM_PX", "SM_BLOCKS"))
    h, w = R.PAST_CAP_SHAPE
    assert h * w > nt * px * blocks and (h * w) % px != 0


def test_reference_finds_the_planted_highlights():
    """The reference pipeline on the twelve synthetic scenes (PSD angles, default options): the measured minima are the ones
    written in specmask_ref.py, from which the floors of the GPU suite come; a scene without highlights gives an empty mask
    with t_eff at the floor."""
    coef = _psd()
    ious, recs = [], []
    for h, w in R.SCENE_SHAPES:
        for seed in R.SCENE_SEEDS:
            views, truth = R.scene(h, w, seed)
            mask, q, (t, te, count) = R.pipeline(views, coef)
            iou, rec = R.iou_recall(mask, truth)
            bg = float(np.percentile(q[~R.dilate(truth, 4)], 99))
            print(f"specmask scene {h}x{w} seed {seed}: t {t} t_eff {te} IoU {iou:.4f} recall {rec:.4f} background p99 {bg:.0f}")
            assert te == t > 2 * bg
            ious.append(iou)
            recs.append(rec)
    print(f"specmask scenes: min IoU {min(ious):.4f}, min recall {min(recs):.4f}")
    assert abs(min(ious) - R.MEASURED_MIN_IOU) < 1e-3 and abs(min(recs) - R.MEASURED_MIN_RECALL) < 1e-3
    assert R.IOU_FLOOR == R.MEASURED_MIN_IOU - 0.05 and R.RECALL_FLOOR == R.MEASURED_MIN_RECALL - 0.05
    views, truth = R.scene(64, 80, 0, blobs=0)
    mask, q, (t, te, count) = R.pipeline(views, coef)
    print(f"specmask scene without blobs: t {t} t_eff {te} count {count} max strength {int(q.max())}")
    assert not truth.any() and t < R.FLOOR == te and count == 0 and q.max() > te


def test_entry_points_refuse_on_the_host():
    """Null pointers, sizes, the 32-bit index range (by name) and the radii are refused before any launch: safe without a GPU."""
    from shmgan_amd import _lib
    import ctypes as C
    L = _lib.lib()
    p = 1                                                      # a non-null pointer nobody dereferences
    four = (C.c_void_p * 4)(p, p, p, p)
    coef = (C.c_float * 12)()
    err = lambda: L.shm_last_error()
    assert L.shm_specmask_strength(None, 8, 8, coef, p, p, None) == -1 and b"null pointer" in err()
    assert L.shm_specmask_strength((C.c_void_p * 4)(p, p, None, p), 8, 8, coef, p, p, None) == -1 and b"source view 2" in err()
    assert L.shm_specmask_strength(four, 0, 8, coef, p, p, None) == -1 and b"at least 1" in err()
    assert L.shm_specmask_strength(four, 30000, 30000, coef, p, p, None) == -1 and b"32-bit index range" in err()
    assert L.shm_specmask_otsu(None, 16, -1, p, None) == -1 and b"null pointer" in err()
    assert L.shm_specmask_otsu(p, 256, -1, p, None) == -1 and b"floor 256" in err()
    assert L.shm_specmask_otsu(p, 16, -2, p, None) == -1 and b"fixed threshold -2" in err()
    assert L.shm_specmask_morph(p, 8, 8, 1, 2, None, p + 2, p, None) == -1 and b"null pointer" in err()
    assert L.shm_specmask_morph(p, 8, 8, 1, 2, p, p + 2, p, None) == -1 and b"of its own" in err()
    assert L.shm_specmask_morph(p, 8, 8, 5, 2, p + 1, p + 2, p, None) == -1 and b"open_radius 5 outside [0, 4]" in err()
    assert L.shm_specmask_morph(p, 8, 8, 4, 9, p + 1, p + 2, p, None) == -1 and b"dilate_radius 9 outside [0, 8]" in err()
    assert L.shm_specmask_morph(p, 8, -1, 1, 2, p + 1, p + 2, p, None) == -1 and b"at least 1" in err()
    # the chain makes every one of these checks before its first launch
    assert L.shm_specmask(four, 8, 8, coef, 16, -1, 1, -1, p, p, p + 1, p + 2, p, None) == -1 and b"shm_specmask: dilate_radius -1" in err()
    assert L.shm_specmask(four, 8, 8, coef, 300, -1, 1, 2, p, p, p + 1, p + 2, p, None) == -1 and b"floor 300" in err()
    assert L.shm_specmask(four, 8, 8, coef, 16, -1, 1, 2, p, p, p + 1, p, p, None) == -1 and b"share a buffer" in err()
    assert L.shm_specmask(four, 65536, 65536, coef, 16, -1, 1, 2, p, p, p + 1, p + 2, p, None) == -1 and b"32-bit index range" in err()
    from shmgan_amd import ops
    assert (ops.SPECMASK_MAX_OPEN, ops.SPECMASK_MAX_DILATE) == (4, 8)
    hdr = _lib.HEADER.read_text()
    assert "#define SHM_SPECMASK_MAX_OPEN 4" in hdr and "#define SHM_SPECMASK_MAX_DILATE 8" in hdr


def test_host_surface_without_gpu(tmp_path):
    """Defaults, refusals that come before any device work, and that importing the module needs no GPU."""
    from types import SimpleNamespace
    from shmgan_amd import polar, trainer
    from shmgan_amd.data import MaskDataset
    d = trainer._DEFAULTS
    assert (d["specseg_mask_source"], d["specseg_mask_threshold"], d["specseg_mask_floor"], d["specseg_mask_open"], d["specseg_mask_dilate"]) == (
        "dir", "otsu", 16, 1, 2)
    assert trainer.SPECSEG_MASK_SOURCES == ("dir", "polar")
    with pytest.raises(ValueError, match="angles or a 3x4"):
        polar.specular_mask([None] * 4)
    with pytest.raises(ValueError, match="three polariser angles"):
        polar.specular_mask([None] * 4, [0, 90, 180, 270])
    with pytest.raises(ValueError, match="threshold"):
        polar.specular_mask([None] * 4, R.PSD_ANGLES, threshold="mean")
    with pytest.raises(ValueError, match="byte range"):
        polar.specular_mask([None] * 4, R.PSD_ANGLES, threshold=300)
    for s in ("I0", "I60", "I90"):
        (tmp_path / s).mkdir()
    with pytest.raises(ValueError, match="four view directories"):
        polar.write_specular_masks(str(tmp_path), str(tmp_path / "out"), subdirs=("I0", "I60", "I90"))
    with pytest.raises(TypeError, match="unknown option"):
        polar.write_specular_masks(str(tmp_path), str(tmp_path / "out"), radius=3)
    with pytest.raises(TypeError, match="unknown option"):
        MaskDataset.from_polar(str(tmp_path), 32, radius=3)
    with pytest.raises(ValueError, match="four view directories"):
        MaskDataset.from_polar(str(tmp_path), 32, subdirs=("I0", "I60", "I90"))
    (tmp_path / "I150").mkdir()
    from PIL import Image
    Image.fromarray(np.zeros((4, 4, 3), np.uint8)).save(tmp_path / "I0" / "a.png")
    with pytest.raises(ValueError, match="different numbers"):
        MaskDataset.from_polar(str(tmp_path), 32)
    # an unknown mask source is refused by name, before the trainer looks at a directory or the device
    t = trainer.ShmGANwithSSpecSeg.__new__(trainer.ShmGANwithSSpecSeg)
    t.args = SimpleNamespace(**d)
    with pytest.raises(ValueError, match="specseg_mask_source 'png'"):
        t.train_specseg(SimpleNamespace(specseg_mask_source="png"))
