"""NumPy restatement of shm_dofp_merge (include/shmgan_hip.h), with the case table of its tests.

  table()     mul[m] of the header from the exposures, in Python integers
  merge()     the header's arithmetic on whole arrays;  counts() the photosites per number of valid pages
  brute()     the same one photosite at a time in Python integers, with the exact quotient as a Fraction beside it, which
              tests/test_merge_cpu.py holds merge() against
  scene()     the motivating case: a polarised disc that clips in the long exposures over a dim unpolarised background
and modelled faults (`fault=`) that the CPU test shows the GPU test's comparison catches.  All integer, all exact.
"""
from __future__ import annotations

import functools
from fractions import Fraction

import numpy as np

import calibrate_ref as cr
import dofp_ref as dr

MERGE_MAX, MERGE_TABLE, Q = 8, 256, 20
FAULTS = ("sat_in", "equal_weights", "black_kept", "mask_reversed", "truncate", "allsat_zero", "page0", "pitch_w")


def table(exposures, bits):
    """mul of the header: uint32 [256]; entry m is floor((2 (e_min << (f + 20)) + T_m) / (2 T_m))."""
    f, n = 16 - bits, len(exposures)
    top = min(int(e) for e in exposures) << (f + Q)
    mul = np.zeros(MERGE_TABLE, dtype=np.uint32)
    for m in range(1, 1 << n):
        T = sum(int(e) for k, e in enumerate(exposures) if m >> k & 1)
        mul[m] = (2 * top + T) // (2 * T)
    return mul


def masks(pages, white, fault=None):
    """m of the header per photosite, int64 [h,w]."""
    v = np.asarray(pages).astype(np.int64)
    n = v.shape[0]
    m = np.zeros(v.shape[1:], dtype=np.int64)
    for k in range(n):
        m |= (v[k] < white).astype(np.int64) << ((n - 1 - k) if fault == "mask_reversed" else k)
    return m


def merge(pages, exposures, bits, black, white, fault=None):
    """dst of the header, uint16 [h,w].  pages: [n,h,w].  fault "pitch_w" is modelled on the buffer, not here (dr.read_with_pitch_w)."""
    v = np.asarray(pages).astype(np.int64)
    n = v.shape[0]
    f = 16 - bits
    if fault == "page0":
        v = np.repeat(v[:1], n, axis=0)
    if fault == "sat_in":
        valid = np.ones(v.shape, dtype=bool)
        m = np.full(v.shape[1:], (1 << n) - 1, dtype=np.int64)
    else:
        valid = v < white
        m = masks(v, white, fault)
    E = np.where(valid, v - (0 if fault == "black_kept" else black), 0).sum(axis=0)
    half = 0 if fault == "truncate" else 1 << (Q - 1)
    if fault == "equal_weights":          # the mean of the pages' own estimates: each (v_k - black) e_min / e_k, unweighted
        emin = min(int(e) for e in exposures)
        q = [((2 * (emin << (f + Q))) + int(e)) // (2 * int(e)) for e in exposures]
        num = sum(np.where(valid[k], v[k] - black, 0) * q[k] for k in range(n))
        R = (num // np.maximum(valid.sum(axis=0), 1) + half) >> Q
    else:
        R = (E * table(exposures, bits).astype(np.int64)[m] + half) >> Q
    out = np.clip((0 if fault == "black_kept" else black << f) + R, 0, 65535)
    return np.where(m != 0, out, 0 if fault == "allsat_zero" else min(65535, white << f)).astype(np.uint16)


def counts(pages, white):
    """counts of the header: int64 [9], entry j = the photosites with exactly j valid pages."""
    v = np.asarray(pages)
    return np.bincount((v < white).sum(axis=0).ravel(), minlength=MERGE_MAX + 1).astype(np.int64)


def brute(pages, exposures, bits, black, white):
    """(dst uint16 [h,w], exact): merge() one photosite at a time in Python integers, and the real-valued result before rounding as a
    Fraction per site -- clamp((black << f) + E e_min 2^f / T_m, 0, 65535), or the all-saturated value."""
    v = np.asarray(pages)
    n, h, w = v.shape
    f = 16 - bits
    e = [int(x) for x in exposures]
    emin = min(e)
    out = np.zeros((h, w), dtype=np.uint16)
    exact = np.empty((h, w), dtype=object)
    for y in range(h):
        for x in range(w):
            ok = [k for k in range(n) if int(v[k, y, x]) < white]
            if not ok:
                out[y, x] = min(65535, white << f)
                exact[y, x] = Fraction(int(out[y, x]))
                continue
            T = sum(e[k] for k in ok)
            E = sum(int(v[k, y, x]) - black for k in ok)
            mul = (2 * (emin << (f + Q)) + T) // (2 * T)
            R = (E * mul + (1 << (Q - 1))) // (1 << Q)               # floor division: the arithmetic shift
            out[y, x] = min(max((black << f) + R, 0), 65535)
            exact[y, x] = min(max(Fraction(black << f) + Fraction(E * emin * (1 << f), T), Fraction(0)), Fraction(65535))
    return out, exact


# ---- the case table --------------------------------------------------------------------------------------------------------------------------
SHAPES = cr.SHAPES                          # "period" is 1 x 1 here: the merge has no lattice
SMALL = cr.SMALL                            # what the brute force walks
BITS = (8, 12, 16)
BRACKETS = ((3, 7), (1, 4, 16), (1000, 250, 62), (1, 2, 4, 8, 16, 32, 64, 128))          # the third unsorted and no power of two
KINDS = ("physical", "junk")
PER_THREAD = cr.PER_THREAD


def shape_of(shape):
    return (1, 1) if shape == "period" else shape


def levels_of(bits):
    """(black, white): a pedestal of a sixteenth of the range, saturation an eighth below the top."""
    maxv = (1 << bits) - 1
    return maxv // 16, maxv - maxv // 8


@functools.lru_cache(maxsize=None)
def case(shape, bits, exposures, kind):
    """(pages [n,h,w], black, white) of one case, read-only.  physical: one radiance ramp, from below darkness to past the saturation of
    the shortest exposure, through every page with noise, so that every count of valid pages occurs; junk: independent random pages with
    samples at white - 1, white and 2^bits - 1.  Where h * w >= 2^n every mask 0 .. 2^n - 1 is planted at a site of its own."""
    h, w = shape_of(shape)
    n = len(exposures)
    maxv = (1 << bits) - 1
    black, white = levels_of(bits)
    rng = np.random.default_rng((h, w, bits, BRACKETS.index(exposures), KINDS.index(kind)))
    if kind == "physical":
        emin = min(exposures)
        L = rng.permutation(np.linspace(-0.02, 1.3, h * w)).reshape(h, w) * (white - black)
        sigma = max(1.0, maxv / 1000.0)
        pages = np.stack([np.clip(np.rint(black + L * (e / emin) + rng.normal(0.0, sigma, (h, w))), 0, maxv) for e in exposures]).astype(np.int64)
    else:
        pages = rng.integers(0, maxv + 1, (n, h, w))
        pick = rng.random((n, h, w))
        pages[pick < 0.06] = white - 1
        pages[(pick >= 0.06) & (pick < 0.12)] = white
        pages[(pick >= 0.12) & (pick < 0.18)] = maxv
    if h * w >= 1 << n:
        sites = rng.choice(h * w, 1 << n, replace=False)
        for m, s in enumerate(sites):
            y, x = divmod(int(s), w)
            for k in range(n):
                pages[k, y, x] = rng.integers(0, white) if m >> k & 1 else rng.integers(white, maxv + 1)
    pages = pages.astype(np.uint8 if bits == 8 else np.uint16)
    pages.setflags(write=False)
    return pages, black, white


@functools.lru_cache(maxsize=None)
def case_reference(shape, bits, exposures, kind):
    """(dst, counts) of one case: computed once, shared, read-only."""
    pages, black, white = case(shape, bits, exposures, kind)
    out, cnt = merge(pages, exposures, bits, black, white), counts(pages, white)
    out.setflags(write=False)
    cnt.setflags(write=False)
    return out, cnt


def all_cases(shapes=SHAPES):
    return [(s, b, e, k) for s in shapes for b in BITS for e in BRACKETS for k in KINDS]


def pitch_extra(w):
    return cr.pitch_extra(w)


# ---- the motivating case ---------------------------------------------------------------------------------------------------------------------
SCENE_SHAPE, SCENE_BITS, SCENE_EXPOSURES, SCENE_BLACK, SCENE_NOISE = (64, 64), 12, (1, 4, 16), 64, 3.0
SCENE_ANGLES = (90.0, 45.0, 135.0, 0.0)     # Sony's quad; the views come out in ascending angle (dr.SONY_QUAD)
SCENE_DISC, SCENE_CORE = 8.0, 4.0           # radii in quads around the centre: the disc, and the core the assertions look at


def scene(seed=0):
    """dict(pages uint16 [3,64,64], truth, disc, core, background): a mono 12-bit sensor under Sony's quad, exposures 1 : 4 : 16, a
    pedestal of 64 counts and Gaussian noise of 3 counts per frame.  Radiance is constant per 2 x 2 quad (the views are compared in "bin"
    mode, one pixel per quad, so that a sharp edge does not read as polarisation): an unpolarised background of 20 counts of the shortest
    exposure everywhere, and inside a disc of 8 quads radius light of 3000 counts fully polarised at 20 degrees -- behind the polariser at
    theta it is 3000 cos^2(theta - 20), between 351 (90 degrees) and 2649 (0 degrees) counts, so the shortest page holds all four
    orientations, the 4x page clips three of them and the 16x page all four.  truth: the noise-free scene in the merged mosaic's units
    (1/16 count of the shortest exposure), float [64,64]; disc, core, background: bool maps per quad [32,32] (the background excludes the
    quads within 3 of the disc, which the mask's dilation may reach)."""
    h, w = SCENE_SHAPE
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    theta = np.deg2rad(np.asarray(SCENE_ANGLES))[2 * (y % 2) + (x % 2)]
    qy, qx = np.mgrid[0:h // 2, 0:w // 2]
    r = np.hypot(qy - (h // 2 - 1) / 2, qx - (w // 2 - 1) / 2)
    disc = r <= SCENE_DISC
    light = 20.0 + np.where(np.kron(disc, np.ones((2, 2), dtype=bool)), 3000.0 * np.cos(theta - np.deg2rad(20.0)) ** 2, 0.0)
    pages = np.stack([np.clip(np.rint(SCENE_BLACK + e * light + rng.normal(0.0, SCENE_NOISE, (h, w))), 0, 4095) for e in SCENE_EXPOSURES])
    return dict(pages=pages.astype(np.uint16), truth=(SCENE_BLACK + light) * 16.0, disc=disc, core=r <= SCENE_CORE, background=r > SCENE_DISC + 3)
