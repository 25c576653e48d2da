"""NumPy restatement of shm_dofp_views (include/shmgan_hip.h): polariser-mosaic frame -> four uint8 [ho,wo,3] views and their total.

Two forms of the same definition:
  views()          the lattice form the header states: per lattice integer tap weights, numerators summed per channel, one
                   shift with round-half-up
  views_general()  the general numerator form: value = floor(N / D + 1/2) with D = (weight total) * (lattices) * 2^s as an integer
                   division, no shifts; the two agree because D is a power of two
and mosaic_from_views(), which samples four full-resolution views into the mosaic a sensor would have recorded, the case table of the
GPU test, and modelled faults (`fault=`) that tests/test_dofp_cpu.py shows the GPU test's comparison catches.  All integer, all exact.
"""
from __future__ import annotations

import functools

import numpy as np

PATTERNS = ("mono", "rggb", "bggr", "grbg", "gbrg")
MODES = ("bilinear", "bin")
# colour channel (0 R, 1 G, 2 B) of colour block 2 by + bx of the Bayer tile
CHANNEL = {"rggb": (0, 1, 1, 2), "bggr": (2, 1, 1, 0), "grbg": (1, 0, 2, 1), "gbrg": (1, 2, 0, 1)}
SONY_QUAD = (2, 1, 3, 0)            # 90 / 45 / 135 / 0 with the views in ascending angle
FAULTS = ("quad_rows", "swap_rb", "clamp_n", "truncate", "pitch_w")


def period(pattern):
    return 2 if pattern == "mono" else 4


def lattices(pattern, quad, fault=None):
    """[(dy, dx, view, channels)]: every lattice of the mosaic, the view it belongs to and the channels it feeds."""
    if fault == "quad_rows":
        quad = (quad[2], quad[3], quad[0], quad[1])
    out = []
    for ay in range(2):
        for ax in range(2):
            v = quad[2 * ay + ax]
            if pattern == "mono":
                out.append((ay, ax, v, (0, 1, 2)))
                continue
            for by in range(2):
                for bx in range(2):
                    c = CHANNEL[pattern][2 * by + bx]
                    if fault == "swap_rb":
                        c = 2 - c
                    out.append((2 * by + ay, 2 * bx + ax, v, (c,)))
    return out


def axis_taps(N, d, P, fault=None):
    """Per output coordinate 0..N-1 of an axis of length N, for the lattice with offset d: (sample coordinate of tap 0, of tap 1,
    weight of tap 0, weight of tap 1)."""
    n = (N - 1 - d) // P + 1
    y = np.arange(N)
    q = y - d
    i0 = np.floor_divide(q, P)
    f = q - P * i0
    hi = n if fault == "clamp_n" else n - 1
    return d + P * np.clip(i0, 0, hi), d + P * np.clip(i0 + 1, 0, hi), P - f, f


def numerators(mosaic, pattern, quad, mode, fault=None):
    """(N int64 [4,ho,wo,3], lattices per channel int [3], weight total per lattice): the channel numerators before the finish."""
    m = np.asarray(mosaic).astype(np.int64)
    h, w = m.shape
    P = period(pattern)
    if fault == "clamp_n":          # the faulty clamp reads one lattice step past the frame: whatever lies there (here: zeros)
        m = np.pad(m, ((0, P), (0, P)))
    if mode == "bilinear":
        ho, wo, wt = h, w, P * P
    else:
        ho, wo, wt = h // P, w // P, 1
    N = np.zeros((4, ho, wo, 3), dtype=np.int64)
    nl = np.array([1, 1, 1] if pattern == "mono" else [1, 2, 1], dtype=np.int64)
    for dy, dx, v, chans in lattices(pattern, quad, fault):
        if mode == "bilinear":
            r0, r1, wy0, wy1 = axis_taps(h, dy, P, fault)
            c0, c1, wx0, wx1 = axis_taps(w, dx, P, fault)
            val = (wy0[:, None] * (wx0[None, :] * m[r0[:, None], c0[None, :]] + wx1[None, :] * m[r0[:, None], c1[None, :]]) +
                   wy1[:, None] * (wx0[None, :] * m[r1[:, None], c0[None, :]] + wx1[None, :] * m[r1[:, None], c1[None, :]]))
        else:
            val = m[dy:P * ho:P, dx:P * wo:P]
        for c in chans:
            N[v, :, :, c] += val
    return N, nl, wt


def _finish(N, shift, fault=None):
    half = 0 if fault == "truncate" else (1 << shift) >> 1
    return np.minimum(255, (N + half) >> shift).astype(np.uint8)


def views(mosaic, pattern, quad, bits, mode="bilinear", fault=None):
    """(views uint8 [4,ho,wo,3], total uint8 [ho,wo,3]) in the lattice form of the header."""
    N, nl, wt = numerators(mosaic, pattern, quad, mode, fault)
    s = bits - 8
    k0 = int(np.log2(wt))
    out = np.empty(N.shape, dtype=np.uint8)
    total = np.empty(N.shape[1:], dtype=np.uint8)
    tot = N.sum(axis=0)
    for c in range(3):
        k = k0 + (1 if nl[c] == 2 else 0)
        out[..., c] = _finish(N[..., c], k + s, fault)
        total[..., c] = _finish(tot[..., c], k + s + 2, fault)
    return out, total


def views_general(mosaic, pattern, quad, bits, mode="bilinear"):
    """The same in the general numerator form: round-half-up of N / D by one integer division."""
    N, nl, wt = numerators(mosaic, pattern, quad, mode)
    D = wt * nl * (1 << (bits - 8))                       # [3]
    out = np.minimum(255, (2 * N + D) // (2 * D)).astype(np.uint8)
    total = np.minimum(255, (2 * N.sum(axis=0) + 4 * D) // (8 * D)).astype(np.uint8)
    return out, total


def mosaic_from_views(full, pattern, quad, bits=8):
    """The mosaic a sensor with this layout records of four full-resolution integer views full[v] = [H,W,3] (values within `bits`):
    at (y, x) the view of its quad position and the channel of its colour block (mono: channel 0)."""
    full = np.asarray(full)
    _, H, W, _ = full.shape
    y, x = np.mgrid[0:H, 0:W]
    v = np.asarray(quad)[2 * (y % 2) + (x % 2)]
    c = np.zeros_like(y) if pattern == "mono" else np.asarray(CHANNEL[pattern])[2 * ((y // 2) % 2) + ((x // 2) % 2)]
    return full[v, y, x, c].astype(np.uint8 if bits == 8 else np.uint16)


def pitched(mosaic, pitch, fill):
    """(buffer [h, pitch] with the mosaic in its first w columns and `fill` in the gap, the mosaic as a view of it)."""
    h, w = mosaic.shape
    buf = np.full((h, pitch), fill, dtype=mosaic.dtype)
    buf[:, :w] = mosaic
    return buf, buf[:, :w]


def read_with_pitch_w(buf, h, w):
    """Fault model "pitch_w": what a kernel sees that takes the row pitch of a pitched buffer to be w."""
    return buf.reshape(-1)[:h * w].reshape(h, w)


# ---- the GPU test's case table ---------------------------------------------------------------------------------------------------------
SHAPES_MONO_ONLY = ((2, 2), (3, 5))
# the last: a width and pitch of a multiple of four samples with columns away from both edges (the kernel's 4-sample accesses; of the
# others only 261 x 12, and 9 x 1031 at its pitch of w + 5 = 1036, reach them)
SHAPES = ((4, 4), (5, 7), (8, 8), (13, 18), (37, 66), (9, 1031), (261, 12), (20, 40))
QUADS = (SONY_QUAD, (0, 3, 1, 2))
BITS = (8, 10, 12, 16)


def shape_pattern_pairs():
    return [(s, "mono") for s in SHAPES_MONO_ONLY] + [(s, p) for s in SHAPES for p in PATTERNS]


def cases_of(shape, pattern):
    """[(quad, bits, kind)] for one shape and pattern: random full-range data for both quads and all depths; all-maximum samples for
    every depth; samples above 2^bits - 1 (the clamp) for the depths that leave room in 16 bits."""
    out = [(q, b, "random") for q in QUADS for b in BITS]
    out += [(QUADS[0], b, "max") for b in BITS]
    out += [(QUADS[1], b, "over") for b in (10, 12)]
    return out


def case_mosaic(shape, pattern, quad, bits, kind):
    h, w = shape
    seed = (h, w, PATTERNS.index(pattern), QUADS.index(quad), bits, ("random", "max", "over").index(kind))
    rng = np.random.default_rng(seed)
    dt = np.uint8 if bits == 8 else np.uint16
    if kind == "max":
        return np.full((h, w), (1 << bits) - 1, dtype=dt)
    top = (1 << bits) if kind == "random" else (1 << 16)
    return rng.integers(0, top, size=(h, w)).astype(dt)


@functools.lru_cache(maxsize=None)
def case_reference(shape, pattern, quad, bits, kind, mode):
    """(mosaic, views, total) of one case: computed once, shared, read-only."""
    m = case_mosaic(shape, pattern, quad, bits, kind)
    v, t = views(m, pattern, quad, bits, mode)
    for a in (m, v, t):
        a.setflags(write=False)
    return m, v, t
