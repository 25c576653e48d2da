"""TEST INFRASTRUCTURE ONLY -- NumPy restatement of csrc/specmask.hip (include/shmgan_hip.h, "specular masks", states the
definitions): the polarised-intensity byte map, its histogram, Otsu's threshold, the open + dilate morphology with the
skip-outside border rule, the whole pipeline, the case tables of the CPU and GPU suites, the faults the GPU comparison has to
catch, and a synthetic scene with planted highlights.

The GPU suite compares every stage with this file FED THE DEVICE'S OWN UPSTREAM OUTPUT, so everything after the square root is an
exact comparison; only the strength of a non-integer matrix needs a tolerance (near_integer below, built like polar_ref.bound).
"""
import functools

import numpy as np

import polar_ref as pr

TEXTBOOK_ANGLES = [0.0, 45.0, 90.0, 135.0]
PSD_ANGLES = [0.0, 60.0, 90.0, 150.0]
DOP_MATRIX = [[1, 0, 1, 0], [1, 0, -1, 0], [0, 1, 0, -1]]          # polar.REFERENCE_DOP_MATRIX

# (1,1) (1,37) (37,1): degenerate axes; (5,7): smaller than the radii; (130,67): partial tiles on both axes over several 32 x 64 tiles
SHAPES = [(1, 1), (1, 37), (37, 1), (5, 7), (37, 53), (64, 64), (130, 67), (300, 200)]
RADII = [(0, 0), (1, 2), (4, 8), (0, 3), (2, 0)]                    # (open, dilate)
CONSTANT_SHAPE = (300, 230)                                         # 69000 > 2^16 pixels in one bin
# the strength kernel caps its grid at 1024 blocks of 256 threads x 4 pixels = 2^20 pixels a sweep: one case past it, not a multiple of 4
PAST_CAP_SHAPE = (1031, 1029)
FLOOR = 16


# ---- strength ---------------------------------------------------------------------------------------------------------------
def strength(views_u8, coef, dtype=np.float64):
    """p = sqrt(max_c (S1_c^2 + S2_c^2)) [h,w] in `dtype`; the rows of `coef` (cast to float32 first, as the device gets it) summed
    left to right (polar_ref.stokes)."""
    _, s1, s2 = pr.stokes(views_u8, coef, dtype)
    return np.sqrt((s1 * s1 + s2 * s2).max(axis=2))


def isqrt(e):
    """Exact integer square root of a non-negative int64 array."""
    e = np.asarray(e, dtype=np.int64)
    r = np.floor(np.sqrt(e.astype(np.float64))).astype(np.int64)
    r -= (r * r > e)
    r += ((r + 1) * (r + 1) <= e)
    assert np.all(r * r <= e) and np.all((r + 1) * (r + 1) > e)
    return r


def strength_int(views_u8, matrix):
    """e = max_c (S1_c^2 + S2_c^2) in exact integers for an integer matrix."""
    m = np.asarray(matrix)
    mi = np.rint(m).astype(np.int64)
    assert np.array_equal(mi, m), "strength_int takes an integer matrix"
    v = [np.asarray(a, dtype=np.int64) for a in views_u8]
    s1 = sum(mi[1, k] * v[k] for k in range(4))
    s2 = sum(mi[2, k] * v[k] for k in range(4))
    return (s1 * s1 + s2 * s2).max(axis=2)


def quantise(p):
    """q = min(255, (int) p) as uint8."""
    return np.minimum(255, np.floor(np.asarray(p, dtype=np.float64))).astype(np.uint8)


def q_int(views_u8, matrix):
    return np.minimum(255, isqrt(strength_int(views_u8, matrix))).astype(np.uint8)


def near_integer(views_u8, coef):
    """For a non-integer matrix: (p64, err32, bound, excusable) -- the float64 strength, the tolerance built as polar_ref.bound builds its
    own (the larger of 2e-6 relative and four times the float32 restatement's error against float64 on the same inputs), and the
    pixels where p64 lies within that tolerance of an integer: the only ones at which q may differ from floor(p64), by one."""
    p64 = strength(views_u8, coef, np.float64)
    p32 = strength(views_u8, coef, np.float32)
    err32 = float(np.abs(p32.astype(np.float64) - p64).max())
    bound = np.maximum(2e-6 * p64, 4.0 * err32)
    # ... below the clamp: where p64 is past 256 by more than the tolerance, q is 255 and nothing is excused
    excusable = (np.abs(p64 - np.rint(p64)) <= bound) & (p64 < 256.0 + bound)
    return p64, err32, bound, excusable


# ---- histogram and Otsu -----------------------------------------------------------------------------------------------------
def histogram(q):
    return np.bincount(np.asarray(q, dtype=np.uint8).ravel(), minlength=256).astype(np.int64)


def otsu_scores(hist):
    """var(t) = ((N0 N1) d) d, d = M1 / N1 - M0 / N0, bins <= t being class 0; 0 where a class is empty.  Exact integer prefix sums,
    then float64 in the device's order."""
    h = np.asarray(hist, dtype=np.int64)
    assert h.shape == (256,) and h.min() >= 0
    n0, m0 = np.cumsum(h), np.cumsum(h * np.arange(256, dtype=np.int64))
    n1, m1 = n0[-1] - n0, m0[-1] - m0
    ok = (n0 > 0) & (n1 > 0)
    var = np.zeros(256, dtype=np.float64)
    a, b = n0[ok].astype(np.float64), n1[ok].astype(np.float64)
    d = m1[ok].astype(np.float64) / b - m0[ok].astype(np.float64) / a
    var[ok] = ((a * b) * d) * d
    return var


def otsu(hist):
    """The lowest t of maximal var(t) (np.argmax returns the first)."""
    return int(np.argmax(otsu_scores(hist)))


def t_eff(t, floor=FLOOR, fixed=None):
    return int(fixed) if fixed is not None else max(int(t), int(floor))


def spikes(*pairs):
    h = np.zeros(256, dtype=np.int64)
    for b, c in pairs:
        h[b] = c
    return h


# histograms with a UNIQUE best partition (every t between two occupied bins cuts the same way and scores the same bits; the lowest
# is taken) or no split at all (t = 0): name -> (histogram, t)
OTSU_CASES = {
    "two_spikes": (spikes((10, 900), (200, 100)), 10),
    "two_spikes_adjacent": (spikes((254, 7), (255, 5)), 254),
    "one_spike": (spikes((77, 1234)), 0),                     # every var(t) is 0: t = 0 and t_eff = floor
    "uniform": (np.full(256, 37, dtype=np.int64), 127),
    "all_in_255": (spikes((255, 4321)), 0),
    "empty": (np.zeros(256, dtype=np.int64), 0),
    "large": (spikes((3, 2_000_000_000), (40, 147_483_647)), 3),      # N0 N1 beyond 2^53: the product is rounded once, as in the kernel
}


# ---- morphology -------------------------------------------------------------------------------------------------------------
def _window(b, r, neutral, op):
    """op over the (2r+1)^2 square with out-of-image taps skipped (= read as the neutral element), separably."""
    b = np.asarray(b, dtype=bool)
    if r == 0:
        return b.copy()
    h, w = b.shape
    p = np.full((h + 2 * r, w + 2 * r), bool(neutral))
    p[r:r + h, r:r + w] = b
    rows = functools.reduce(op, [p[:, d:d + w] for d in range(2 * r + 1)])
    return functools.reduce(op, [rows[d:d + h] for d in range(2 * r + 1)])


def erode(b, r):
    return _window(b, r, True, np.logical_and)


def dilate(b, r):
    return _window(b, r, False, np.logical_or)


def morph(q, teff, ro, rd):
    """(mask uint8 0 / 255, count): b = q > teff, opened by ro (erode, then dilate), dilated by rd."""
    b = np.asarray(q) > teff
    m = dilate(dilate(erode(b, ro), ro), rd)
    return (m * np.uint8(255)).astype(np.uint8), int(m.sum())


def pipeline(views_u8, coef, threshold="otsu", floor=FLOOR, ro=1, rd=2, dtype=np.float64):
    """The whole chain on the host: (mask, q, (t, t_eff, count))."""
    q = quantise(strength(views_u8, coef, dtype))
    t = otsu(histogram(q))
    te = t_eff(t, floor, None if threshold == "otsu" else int(threshold))
    mask, count = morph(q, te, ro, rd)
    return mask, q, (t, te, count)


# ---- inputs -----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def random_views(h, w):
    """Four random byte images (shared by the tests of a size; never modified).  About a quarter of the pixels clamp at 255."""
    rng = np.random.default_rng(7000 * h + w)
    out = [rng.integers(0, 256, (h, w, 3)).astype(np.uint8) for _ in range(4)]
    for a in out:
        a.setflags(write=False)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def morph_q(h, w, kind):
    """A strength map for the morphology checks.  "busy": dim noise, bright rectangles, isolated bright pixels (an opening with
    ro >= 1 removes them), bright runs on all four borders and all four corners; "single": one bright pixel; "full": every pixel
    bright.  Bright is >= 200 and dim < 60, so that any threshold between them gives the same binary map."""
    rng = np.random.default_rng(31 * h + w)
    q = rng.integers(0, 60, (h, w)).astype(np.uint8)
    if kind == "single":
        q[h // 2, w // 3] = 240
    elif kind == "full":
        q[:] = rng.integers(200, 256, (h, w)).astype(np.uint8)
    else:
        assert kind == "busy"
        for _ in range(max(2, h * w // 900)):
            y, x = int(rng.integers(0, h)), int(rng.integers(0, w))
            q[y:y + int(rng.integers(1, 14)), x:x + int(rng.integers(1, 14))] = 220
        # bands that lean on a border, 2, 3 and 5 pixels thick: an erosion by 1, 2, 4 keeps their border row only because the taps
        # outside the image are skipped
        q[h // 4:h // 4 + 12, 0:2] = 225
        q[0:3, w // 3:w // 3 + 12] = 225
        q[h // 2:h // 2 + 14, max(w - 5, 0):] = 225
        iso = rng.random((h, w)) < 0.01
        q[iso] = 230
        q[0, ::3] = 210
        q[-1, 1::4] = 210
        q[::5, 0] = 210
        q[2::3, -1] = 210
        q[0, 0] = q[0, -1] = q[-1, 0] = q[-1, -1] = 255
    q.setflags(write=False)
    return q


# ---- the faults the GPU comparison must catch (tests/test_specmask_cpu.py shows that it does, on the inputs above) ------------
def fault_threshold_off_by_one(q, teff, ro, rd):
    """b = q >= t_eff instead of q > t_eff."""
    return morph(q, teff - 1, ro, rd)


def fault_border_eats_edge(q, teff, ro, rd):
    """An erosion that reads out-of-image taps as 0 instead of skipping them."""
    b = np.asarray(q) > teff
    m = dilate(dilate(_window(b, ro, False, np.logical_and), ro), rd)
    return (m * np.uint8(255)).astype(np.uint8), int(m.sum())


def fault_histogram_drops_tail(q, block=1024):
    """A histogram that forgets the last, partial block of `block` pixels."""
    flat = np.asarray(q).ravel()
    return histogram(flat[:flat.size // block * block])


def fault_histogram_wraps16(q):
    """Counters of 16 bits."""
    return histogram(q) % 65536


# ---- synthetic scene --------------------------------------------------------------------------------------------------------
SCENE_SHAPES = [(64, 80), (96, 96)]
SCENE_SEEDS = [0, 1, 2, 3, 4, 5]
BLOB_AMPLITUDE = 150.0


def scene(h, w, seed, angles=PSD_ANGLES, blobs=3):
    """(views, truth): four uint8 [h,w,3] views of a smooth unpolarised textured background with `blobs` Gaussian highlights of
    amplitude ~150, each fully polarised at its own random angle phi and of radius r (sigma = r / 2); truth [h,w] bool = the discs
    of radius r.  View at polariser angle theta: 0.5 * base + spec * cos^2(theta - phi) + N(0, 3), rounded to bytes."""
    rng = np.random.default_rng([h, w, seed])
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    base = np.zeros((h, w, 3))
    for c in range(3):
        f = 90.0 + 10.0 * c
        for _ in range(4):                                         # a few low spatial frequencies with random phase ...
            ky, kx = rng.uniform(-0.12, 0.12, 2)
            f = f + 14.0 * np.cos(ky * yy + kx * xx + rng.uniform(0, 2 * np.pi))
        base[..., c] = f + rng.normal(0.0, 4.0, (h, w))            # ... and a fine texture
    base = np.clip(base, 10.0, 170.0)
    spec = np.zeros((4, h, w))
    truth = np.zeros((h, w), dtype=bool)
    for _ in range(blobs):
        r = rng.uniform(5.0, 9.0)
        cy, cx = rng.uniform(r + 3, h - r - 3), rng.uniform(r + 3, w - r - 3)
        phi = rng.uniform(0.0, np.pi)
        amp = BLOB_AMPLITUDE * rng.uniform(0.9, 1.1)
        d2 = (yy - cy) ** 2 + (xx - cx) ** 2
        g = amp * np.exp(-d2 / (2.0 * (0.5 * r) ** 2))
        truth |= d2 <= r * r
        for k, th in enumerate(angles):
            spec[k] += g * np.cos(np.deg2rad(th) - phi) ** 2
    views = []
    for k in range(4):
        v = 0.5 * base + spec[k][..., None] + rng.normal(0.0, 3.0, (h, w, 3))
        a = np.clip(np.rint(v), 0, 255).astype(np.uint8)
        a.setflags(write=False)
        views.append(a)
    return views, truth


def iou_recall(mask, truth):
    m = np.asarray(mask) > 0
    inter = float((m & truth).sum())
    return inter / max(float((m | truth).sum()), 1.0), inter / max(float(truth.sum()), 1.0)


# Quality of THIS file's pipeline (float64, PSD angles, default options) on the twelve scenes above, measured on the CPU by
# tests/test_specmask_cpu.py::test_reference_finds_the_planted_highlights, which prints every figure and re-derives the minima:
#   IoU 0.769 .. 0.906, recall 0.978 .. 1.000, Otsu t 49 .. 54 against a 99th-percentile background strength of 17 .. 19;
#   a scene without blobs: t = 9, t_eff = the floor of 16, empty mask.
# The floors are the minima over shapes and seeds less 0.05; the GPU suite holds the device's masks to the same floors.
MEASURED_MIN_IOU = 0.7694
MEASURED_MIN_RECALL = 0.9775
IOU_FLOOR = MEASURED_MIN_IOU - 0.05
RECALL_FLOOR = MEASURED_MIN_RECALL - 0.05
