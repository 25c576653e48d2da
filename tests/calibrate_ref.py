"""NumPy restatement of shm_dofp_calibrate (include/shmgan_hip.h) and of polar.build_calibration, with the case tables of their tests.

  calibrate()   the header's arithmetic on whole arrays: corr, then the rounded mean of the good same-lattice neighbours at defects
  brute()       the same one photosite at a time in Python integers, which tests/test_calibrate_cpu.py holds calibrate() against
  build()       the builder's arithmetic from two stacks of frames
  sensor()      a noise-free synthetic sensor: fixed-pattern dark, vignetting times pixel response, planted hot / dead / stuck / weak sites
and modelled faults (`fault=`) that the CPU test shows the GPU test's comparison catches.  All integer, all exact.
"""
from __future__ import annotations

import functools

import numpy as np

import dofp_ref as dr

GAIN_MIN, GAIN_MAX = 1024, 16383
FAULTS = ("lattice2", "bad_neighbour", "floor", "gain_first", "sat_corrected", "no_pedestal", "pitch_w")


def corr(v, dark, gain, pedestal, white, maxv, fault=None):
    """corr of the header on int64 arrays."""
    if fault == "gain_first":
        e = ((v * gain + 2048) >> 12) - dark
    else:
        e = ((v - dark) * gain + 2048) >> 12
    c = np.clip((0 if fault == "no_pedestal" else pedestal) + e, 0, maxv)
    return c if fault == "sat_corrected" else np.where(v >= white, v, c)


def neighbour_counts(defect, P):
    """n of the header for every site: how many of its four same-lattice neighbours lie inside the image and are not defective."""
    good = np.pad(np.asarray(defect) == 0, P)
    h, w = np.asarray(defect).shape
    n = np.zeros((h, w), dtype=np.int64)
    for dy, dx in ((-P, 0), (P, 0), (0, -P), (0, P)):
        n += good[P + dy:P + dy + h, P + dx:P + dx + w]
    return n


def calibrate(src, pattern, bits, dark=None, gain=None, defect=None, pedestal=0, white=None, fault=None):
    """dst of the header, in src's dtype.  dark / gain / defect: [h,w] arrays or None; white None = 2^bits - 1."""
    src = np.asarray(src)
    h, w = src.shape
    P = dr.period(pattern)
    maxv = (1 << bits) - 1
    white = maxv if white is None else white
    v = src.astype(np.int64)
    d = np.full((h, w), pedestal, dtype=np.int64) if dark is None else np.asarray(dark).astype(np.int64)
    g = np.full((h, w), 4096, dtype=np.int64) if gain is None else np.asarray(gain).astype(np.int64)
    c = corr(v, d, g, pedestal, white, maxv, fault)
    if defect is None:
        return c.astype(src.dtype)
    bad = np.asarray(defect) != 0
    step = 2 if fault == "lattice2" else P
    good = np.pad(np.ones_like(bad) if fault == "bad_neighbour" else ~bad, step)
    cp = np.pad(c, step)
    S = np.zeros((h, w), dtype=np.int64)
    n = np.zeros((h, w), dtype=np.int64)
    for dy, dx in ((-step, 0), (step, 0), (0, -step), (0, step)):
        gs = good[step + dy:step + dy + h, step + dx:step + dx + w]
        S += np.where(gs, cp[step + dy:step + dy + h, step + dx:step + dx + w], 0)
        n += gs
    mean = (S // np.maximum(n, 1)) if fault == "floor" else (2 * S + n) // np.maximum(2 * n, 1)
    return np.where(bad & (n > 0), mean, c).astype(src.dtype)


def brute(src, pattern, bits, dark=None, gain=None, defect=None, pedestal=0, white=None):
    """calibrate() one photosite at a time, in Python integers."""
    src = np.asarray(src)
    h, w = src.shape
    P = 2 if pattern == "mono" else 4
    maxv = 2 ** bits - 1
    white = maxv if white is None else white

    def one(y, x):
        v = int(src[y, x])
        if v >= white:
            return v
        d = pedestal if dark is None else int(dark[y, x])
        g = 4096 if gain is None else int(gain[y, x])
        e = ((v - d) * g + 2048) // 4096                 # floor division: the arithmetic shift
        return min(max(pedestal + e, 0), maxv)
    out = np.zeros((h, w), dtype=src.dtype)
    for y in range(h):
        for x in range(w):
            if defect is None or int(defect[y, x]) == 0:
                out[y, x] = one(y, x)
                continue
            near = [(yy, xx) for yy, xx in ((y - P, x), (y + P, x), (y, x - P), (y, x + P))
                    if 0 <= yy < h and 0 <= xx < w and int(defect[yy, xx]) == 0]
            if not near:
                out[y, x] = one(y, x)
            else:
                S, n = sum(one(yy, xx) for yy, xx in near), len(near)
                out[y, x] = (2 * S + n) // (2 * n)
    return out


# ---- the kernel's case table ---------------------------------------------------------------------------------------------------------------
PATTERNS = ("mono", "rggb")                 # P = 2 and one Bayer pattern: the pattern is read for P alone
BITS = (8, 12, 16)
PER_THREAD = 8                              # samples a thread makes; a block is 64 x 4 threads: 512 samples by 4 rows
# a launch of 3 x 3 blocks whose groups of 8 are all full (every array on its wide accesses), and one of 3 x 2 blocks with a ragged last group
MULTI_BLOCK = (9, 1032)
MULTI_BLOCK_RAGGED = (6, 1030)
# (5,7) (13,18) (37,66) (6,1030): widths that are no multiple of PER_THREAD; (20,40) (9,1032): widths that are, so the tight tables are read wide too
SHAPES = ("period", (5, 7), (13, 18), (37, 66), (20, 40), MULTI_BLOCK, MULTI_BLOCK_RAGGED)
SMALL = ("period", (5, 7), (13, 18), (20, 40))          # what the brute force walks
TABLES = tuple((d, g, f) for d in (False, True) for g in (False, True) for f in (False, True))          # which of dark, gain, defect are given


def shape_of(shape, pattern):
    """"period" is P x P: every neighbour of every site lies outside the image."""
    P = dr.period(pattern)
    return (P, P) if shape == "period" else shape


def kinds_of(bits):
    """random: the full range with white an eighth below the top, so some samples pass through; max: every sample 2^bits - 1 and white out of
    reach, so all of them are corrected and clamped; half: random with every second site defective; over / over_corrected (12 bits only):
    samples up to 65535, passed through (white = 4095) or corrected and clamped (white = 65536)."""
    return ("random", "max", "half") + (("over", "over_corrected") if bits == 12 else ())


def pedestal_of(bits):
    return ((1 << bits) - 1) // 16


@functools.lru_cache(maxsize=None)
def case(shape, pattern, bits, kind):
    """(src, dark, gain, defect, pedestal, white) of one case, read-only: the tables are those of the shape, pattern and depth (defect: of the
    kind too), so that the eight null / non-null combinations differ in nothing else."""
    h, w = shape_of(shape, pattern)
    maxv = (1 << bits) - 1
    ped = pedestal_of(bits)
    rng = np.random.default_rng((h, w, PATTERNS.index(pattern), bits))
    dark = rng.integers(ped // 2, 2 * ped, (h, w))
    hot = rng.random((h, w)) < 0.05
    dark[hot] = rng.integers(0, maxv + 1, (h, w))[hot]                              # a hot site's dark level is anywhere
    gain = rng.integers(3600, 4700, (h, w))
    pick = rng.random((h, w))
    gain[pick < 0.04] = GAIN_MIN
    gain[pick > 0.96] = GAIN_MAX
    wide = (pick > 0.45) & (pick < 0.55)
    gain[wide] = rng.integers(GAIN_MIN, GAIN_MAX + 1, (h, w))[wide]
    krng = np.random.default_rng((h, w, PATTERNS.index(pattern), bits, ("random", "max", "half", "over", "over_corrected").index(kind)))
    defect = np.where(krng.random((h, w)) < (0.5 if kind == "half" else 0.08), krng.choice([1, 2, 4, 255], (h, w)), 0)
    if kind == "max":
        src = np.full((h, w), maxv)
    else:
        src = krng.integers(0, (1 << 16) if kind.startswith("over") else maxv + 1, (h, w))
    white = {"random": maxv - maxv // 8, "half": maxv - maxv // 8, "max": 65536, "over": maxv, "over_corrected": 65536}[kind]
    out = (src.astype(np.uint8 if bits == 8 else np.uint16), dark.astype(np.uint16), gain.astype(np.uint16), defect.astype(np.uint8))
    for a in out:
        a.setflags(write=False)
    return out + (ped, white)


def case_tables(shape, pattern, bits, kind, which):
    """(dark, gain, defect) of the case with those not in `which` = (dark?, gain?, defect?) replaced by None."""
    _, dark, gain, defect, _, _ = case(shape, pattern, bits, kind)
    return tuple(t if use else None for t, use in zip((dark, gain, defect), which))


@functools.lru_cache(maxsize=None)
def case_reference(shape, pattern, bits, kind, which):
    """dst of one case under one combination of tables: computed once, shared, read-only."""
    src, _, _, _, ped, white = case(shape, pattern, bits, kind)
    out = calibrate(src, pattern, bits, *case_tables(shape, pattern, bits, kind, which), pedestal=ped, white=white)
    out.setflags(write=False)
    return out


def all_cases(shapes=SHAPES):
    return [(s, p, b, k) for s in shapes for p in PATTERNS for b in BITS for k in kinds_of(b)]


def identity_tables(shape, pedestal):
    """The tables that change nothing: dark = pedestal, gain = 4096, no defects."""
    return np.full(shape, pedestal, dtype=np.uint16), np.full(shape, 4096, dtype=np.uint16), np.zeros(shape, dtype=np.uint8)


def pitch_extra(w):
    """Gap that makes the pitch w + gap the next multiple of PER_THREAD above w: a pitched buffer that keeps the wide accesses."""
    return PER_THREAD - w % PER_THREAD


# ---- the builder ---------------------------------------------------------------------------------------------------------------------------
HOT, UNUSABLE, RANGE = 1, 2, 4


def channels(pattern, h, w):
    """Colour class of every site: 0 for mono; R, G, B = 0, 1, 2 from dofp_ref.CHANNEL."""
    y, x = np.mgrid[0:h, 0:w]
    return np.zeros((h, w), dtype=np.int64) if pattern == "mono" else np.asarray(dr.CHANNEL[pattern])[2 * ((y // 2) % 2) + ((x // 2) % 2)]


def stack_mean(frames):
    n = len(frames)
    return (2 * sum(np.asarray(f).astype(np.int64) for f in frames) + n) // (2 * n)


def build(darks, flats, pattern, bits, hot_threshold=None, gain_limits=(0.5, 2.0), white=None):
    """dict(dark, gain, defect, pedestal, reference) by the arithmetic polar.build_calibration documents; gain and reference None without flats."""
    dark = stack_mean(darks)
    thr = 8 << (bits - 8) if hot_threshold is None else hot_threshold
    white = (1 << bits) - 1 if white is None else white
    pedestal = int(sorted(dark.ravel().tolist())[(dark.size - 1) // 2])
    hot = dark > pedestal + thr
    if flats is None:
        return dict(dark=dark, gain=None, defect=np.where(hot, HOT, 0), pedestal=pedestal, reference=None)
    fm = stack_mean(flats)
    f = fm - dark
    usable = ~hot & (f > 0) & (fm < white)
    chan = channels(pattern, *dark.shape)
    lo, hi = (int(np.floor(x * 4096 + 0.5)) for x in gain_limits)
    gain = np.full(dark.shape, 4096, dtype=np.int64)
    out = np.zeros(dark.shape, dtype=bool)
    reference = []
    for c in range(1 if pattern == "mono" else 3):
        sel = usable & (chan == c)
        S, n = int(f[sel].sum()), int(sel.sum())
        reference.append((S, n))
        for y, x in np.argwhere(sel):
            fv = int(f[y, x])
            g = (8192 * S + n * fv) // (2 * n * fv)
            if lo <= g <= hi:
                gain[y, x] = g
            else:
                out[y, x] = True
    defect = np.where(hot, HOT, 0) | np.where(~usable, UNUSABLE, 0) | np.where(out, RANGE, 0)
    return dict(dark=dark, gain=gain, defect=defect, pedestal=pedestal, reference=tuple(reference))


SENSOR_SHAPE = (24, 32)
# planted sites (y, x): two hot lattice neighbours at period 4 AND a third at period 2 from the first, hot corners, dead, stuck-high, weak
PLANTED = dict(hot=((8, 8), (8, 12), (8, 10), (0, 0), (23, 31)), dead=((5, 17), (23, 0)), stuck=((14, 3),), weak=((17, 22),))


def sensor(pattern, bits, shape=SENSOR_SHAPE):
    """A noise-free sensor: (dark frames [3], flat frames [2], the model's dark, the planted defect set as a bool map).  Dark: a pedestal
    plus a fixed pattern of +-3 byte units; the three frames are the model minus 1 at frame 0 only, so the rounded mean is the model.
    Flat: dark + level_c * vignetting * response, response = 3 % per quad position (the polarisers) times 2 % per pixel.  Hot sites sit
    40 byte units above their dark level and still respond; dead sites do not respond; a stuck site reads 2^bits - 1 always; a weak site
    responds at 30 %, outside the gain limits (0.5, 2)."""
    h, w = shape
    s = bits - 8
    maxv = (1 << bits) - 1
    y, x = np.mgrid[0:h, 0:w]
    model = (20 << s) + (((3 * y + 5 * x) % 7 - 3) << s) + (y * x) % (1 << s)
    for p in PLANTED["hot"]:
        model[p] += 40 << s
    for p in PLANTED["stuck"]:
        model[p] = maxv
    r2 = ((y - (h - 1) / 2) ** 2 + (x - (w - 1) / 2) ** 2) / (((h - 1) / 2) ** 2 + ((w - 1) / 2) ** 2)
    vign = 1.0 - 0.3 * r2
    resp = (1.0 + 0.03 * (np.array([0.0, 1.0, -1.0, 0.5])[2 * (y % 2) + (x % 2)])) * (1.0 + 0.02 * np.cos(1.7 * y + 2.9 * x))
    level = np.array([0.55, 0.62, 0.48])[channels(pattern, h, w)] * maxv
    light = np.floor(level * vign * resp).astype(np.int64)
    for p in PLANTED["dead"]:
        light[p] = 0
    for p in PLANTED["weak"]:
        light[p] = light[p] * 3 // 10
    flat = np.minimum(maxv, model + light)
    for p in PLANTED["stuck"]:
        flat[p] = maxv
    dt = np.uint8 if bits == 8 else np.uint16
    darks = [(model - (1 if i == 0 else 0)).astype(dt) for i in range(3)]          # (2 (3 m - 1) + 3) // 6 = m
    flats = [flat.astype(dt), flat.astype(dt)]
    planted = np.zeros(shape, dtype=bool)
    for sites in PLANTED.values():
        for p in sites:
            planted[p] = True
    return darks, flats, model, planted


# ---- the motivating case: a flat, unpolarised frame with two hot samples ---------------------------------------------------------------------
HOT_FRAME_SHAPE = (32, 40)
HOT_SITES = ((9, 14), (20, 24))             # under RGGB a green site and a red one (a green view pixel is the mean of two lattices: half the excess)


def hot_frame(bits=12):
    """(clean, hot, defect): every sample 1200; the hot frame has two samples 60 and 200 byte units above it, the second clipped at the top."""
    clean = np.full(HOT_FRAME_SHAPE, 1200, dtype=np.uint16)
    hot = clean.copy()
    for p, up in zip(HOT_SITES, (60, 200)):
        hot[p] = min((1 << bits) - 1, 1200 + (up << (bits - 8)))
    defect = np.zeros(HOT_FRAME_SHAPE, dtype=np.uint8)
    for p in HOT_SITES:
        defect[p] = 1
    return clean, hot, defect
