"""NumPy restatement of shm_dofp_develop and shm_dofp_wb_gray (include/shmgan_hip.h): a polariser-mosaic frame developed -- black level,
white balance, colour matrix, tone table -- from the UNROUNDED channel numerators of tests/dofp_ref.py, which this file imports and does
not restate.

  table()     the parameter block and tone table of a set of options, computed here from the header's formulas (fractions for the
              multipliers, math for the curves): polar.DofpDevelop.table must equal it
  develop()   (views uint8 [4,ho,wo,3], total uint8 [ho,wo,3]) of a mosaic under a parameter block and a table
  wb_gray()   the six grey-world sums and the three gains of a frame
and the parameter sets and case table of the GPU test, and modelled faults (`fault=`) that tests/test_develop_cpu.py shows the GPU test's
comparison (equality with develop() / wb_gray()) catches.  All integer, all exact."""
from __future__ import annotations

import functools
import math
from fractions import Fraction

import numpy as np

import dofp_ref as dr

# offsets into the int32 parameter block (include/shmgan_hip.h: SHM_DOFP_P_*)
BLACK, MUL, GAIN, FLAGS, CCM, WHITE, NPARAMS = 0, 3, 6, 9, 10, 19, 20
FAULTS = ("black_sample_scale", "black_after_gain", "total_from_views", "no_clamp", "ccm_transposed", "ccm_before_gain", "lut_low_bits",
          "swap_rb_gain", "sat_included", "pitch_w")


# ---- the tables, from the formulas ------------------------------------------------------------------------------------------------------
def tone_table(tone):
    """4096 uint8: round-to-nearest of 255 f(i / 4095); f the identity, the piecewise sRGB encoding, or x^(1/g)."""
    out = np.empty(4096, dtype=np.uint8)
    for i in range(4096):
        x = i / 4095
        if tone == "linear":
            f = x
        elif tone == "srgb":
            f = 12.92 * x if x <= 0.0031308 else 1.055 * x ** (1 / 2.4) - 0.055
        else:
            f = x ** (1 / float(tone))
        out[i] = math.floor(255 * f + 0.5)
    return out


def table(bits, black=0, white=None, wb=(1, 1, 1), ccm=None, tone="srgb", gains=(1024, 1024, 1024)):
    """(params int32 [20], lut uint8 [4096]).  mul_c = round-half-up of 65535 * 65536 * wb_c / (white - black_c) with wb normalised to a
    smallest entry of 1; `gains` are what shm_dofp_wb_gray would have left there (Q10)."""
    black = (black,) * 3 if isinstance(black, int) else tuple(black)
    white = (1 << bits) - 1 if white is None else white
    low = min(Fraction(g) for g in wb)
    p = [0] * NPARAMS
    for c in range(3):
        assert white - black[c] >= 16 and Fraction(wb[c]) / low <= 16
        mul = Fraction(65535 * 65536) * (Fraction(wb[c]) / low) / (white - black[c])
        p[BLACK + c], p[MUL + c], p[GAIN + c] = black[c], math.floor(mul + Fraction(1, 2)), gains[c]
        assert 65536 <= p[MUL + c] < 1 << 32
    if ccm is not None:
        p[FLAGS] = 1
        p[CCM:CCM + 9] = [math.floor(Fraction(x) * 1024 + Fraction(1, 2)) for row in ccm for x in row]
    p[WHITE] = white
    return np.array(p, dtype=np.int64).astype(np.uint32).view(np.int32), tone_table(tone)


def fields(params):
    """(black [3], mul [3], gain [3], matrix flag, ccm [3,3]) of a parameter block, as Python / int64 integers."""
    p = np.asarray(params).view(np.uint32).astype(np.int64)
    ccm = np.asarray(params)[CCM:CCM + 9].astype(np.int64).reshape(3, 3)
    return p[BLACK:BLACK + 3], p[MUL:MUL + 3], p[GAIN:GAIN + 3], int(p[FLAGS]) & 1, ccm


# ---- the development ----------------------------------------------------------------------------------------------------------------------
def linear(N, k, params, fault=None):
    """lin' int64 [...,3] (steps 1 to 4) of numerators N [...,3] whose channel c has total weight 2^k[c]."""
    black, mul, gain, flag, ccm = fields(params)
    M = (mul * gain + 512) >> 10                                   # < 2^36
    if fault == "swap_rb_gain":
        M = M[::-1]
    lin = np.empty(N.shape, dtype=np.int64)
    for c in range(3):
        kc = int(k[c])
        if fault == "black_sample_scale":                          # the pedestal taken from the sample-scale value: the fraction bits are lost
            D = np.maximum(0, (N[..., c] >> kc) - black[c]) << kc
        elif fault == "black_after_gain":
            D = N[..., c]
        else:
            D = np.maximum(0, N[..., c] - (black[c] << kc))
        v = (D * M[c] + (1 << (15 + kc))) >> (16 + kc)             # D < 2^23, M < 2^36: inside int64
        if not (fault == "no_clamp" and flag):
            v = np.minimum(65535, v)
        if fault == "black_after_gain":
            v = np.maximum(0, v - ((black[c] * M[c] + (1 << 15)) >> 16))
        lin[..., c] = v
    if flag:
        m = ccm.T if fault == "ccm_transposed" else ccm
        if fault == "ccm_before_gain":                             # matrix on the unbalanced values, the balance after it
            base = int(M.min())
            raw = np.stack([np.minimum(65535, (np.maximum(0, N[..., c] - (black[c] << int(k[c]))) * base + (1 << (15 + int(k[c])))) >> (16 + int(k[c])))
                            for c in range(3)], axis=-1)
            mixed = np.clip((raw @ m.T + 512) >> 10, 0, 65535)
            lin = np.minimum(65535, (mixed * M[None, :] + base // 2) // base)
        else:
            lin = np.clip((lin @ m.T + 512) >> 10, 0, 65535)
        if fault == "no_clamp":
            lin = np.clip(lin, 0, 65535)
    return lin


def develop(mosaic, pattern, quad, bits, mode, params, lut, fault=None):
    """(views uint8 [4,ho,wo,3], total uint8 [ho,wo,3]): dofp_ref's numerators, developed.  The total develops the SUM of the four views'
    numerators with k + 2."""
    N, nl, wt = dr.numerators(mosaic, pattern, quad, mode)
    k = int(np.log2(wt)) + (nl == 2).astype(np.int64)
    idx = (lambda lin: lin & 4095) if fault == "lut_low_bits" else (lambda lin: lin >> 4)
    lut = np.asarray(lut)
    views = lut[idx(linear(N, k, params, fault))]
    if fault == "total_from_views":                                # the rounded sample-scale views, averaged
        tot, kt = ((N + ((1 << k) >> 1)) >> k).sum(axis=0), np.zeros(3, dtype=np.int64) + 2
    else:
        tot, kt = N.sum(axis=0), k + 2
    return views.astype(np.uint8), lut[idx(linear(tot, kt, params, fault))].astype(np.uint8)


def gains_of(sums):
    S, n = [int(x) for x in sums[:3]], [int(x) for x in sums[3:]]
    mean = [(S[c] << 8) // n[c] if n[c] else 0 for c in range(3)]
    if not all(mean):
        return (1024, 1024, 1024)
    return tuple(min(16383, (max(mean) << 10) // m) for m in mean)


def wb_gray(mosaic, pattern, params, sat, fault=None):
    """((S_r, S_g, S_b, n_r, n_g, n_b), (gain_r, gain_g, gain_b)) over the complete 4 x 4 periods whose 16 samples are all below sat."""
    m = np.asarray(mosaic).astype(np.int64)
    ph, pw = m.shape[0] // 4, m.shape[1] // 4
    per = m[:4 * ph, :4 * pw].reshape(ph, 4, pw, 4).transpose(0, 2, 1, 3)              # [ph,pw,4,4]
    ok = (per < sat).all(axis=(2, 3))
    if fault == "sat_included":
        ok[:] = True
    black = fields(params)[0]
    sums = [0] * 6
    for dy in range(4):
        for dx in range(4):
            c = dr.CHANNEL[pattern][2 * (dy // 2) + dx // 2]
            sums[c] += int(np.maximum(0, per[:, :, dy, dx] - black[c])[ok].sum())
            sums[3 + c] += int(ok.sum())
    return tuple(sums), gains_of(sums)


def with_gains(params, gains):
    p = np.array(params)
    p[GAIN:GAIN + 3] = gains
    return p


# ---- the GPU test's parameter sets and case table ---------------------------------------------------------------------------------------
SETS = ("pedestal", "wb_srgb", "ccm_gamma", "extreme", "high_gain")
CCM_MILD = ((1.6, -0.4, -0.2), (-0.3, 1.5, -0.2), (0.1, -0.6, 1.5))
CCM_WILD = ((7.9, -3.0, -3.0), (-7.9, 2.0, 1.0), (3.0, 3.0, 3.0))          # drives the lower and the upper clamp


@functools.lru_cache(maxsize=None)
def param_set(name, pattern, bits):
    """(params, lut) of one of SETS for a sensor of this pattern and depth.  A mono sensor has one channel: the same black and balance
    for all three, no matrix; its sets keep the pedestal, the curve and (extreme) the gain.
      pedestal   black = 1/16 of the range, linear tone
      wb_srgb    per-channel blacks, a balance triple, the sRGB curve
      ccm_gamma  that balance, a matrix with negative entries, gamma 2.2
      extreme    black above 3/8 of the range (above part of the data), white at half the range, a balance of 16 and device gains up to
                 16383 (the multiplier leaves 24 bits: the kernel's three-multiply product), a matrix that drives both clamps
      high_gain  wb_srgb's blacks and balance under device gains of 9000 / 2000 / 16383 and a gamma of 3, no matrix: the multiplier leaves
                 24 bits at every depth without the matrix (which `extreme` always has on a Bayer sensor)
    An 8-bit sensor's multiplier never fits 24 bits (65535 * 65536 / 255 > 2^24), so at 8 bits every set runs the three-multiply product;
    at 12 and 16 bits the first three sets run the two-multiply one."""
    top = 1 << bits
    b = top // 16
    mono = pattern == "mono"
    if name == "pedestal":
        out = table(bits, black=b, tone="linear")
    elif name == "wb_srgb":
        out = table(bits, black=b if mono else (b, b + 1, b - 1), wb=(1, 1, 1) if mono else (1.9, 1, 1.6), tone="srgb")
    elif name == "ccm_gamma":
        out = table(bits, black=b if mono else (b - 1, b, b + 1), wb=(1, 1, 1) if mono else (1.9, 1, 1.6), ccm=None if mono else CCM_MILD, tone=2.2)
    elif name == "high_gain":
        out = table(bits, black=b if mono else (b, b + 1, b - 1), wb=(1, 1, 1) if mono else (1.9, 1, 1.6), tone=3.0,
                    gains=(9000,) * 3 if mono else (9000, 2000, 16383))
    else:
        p, lut = table(bits, black=3 * top // 8, white=top // 2, wb=(1, 1, 1) if mono else (16, 1, 4), ccm=None if mono else CCM_WILD, tone="srgb",
                       gains=(16383,) * 3 if mono else (16383, 1024, 5000))
        out = p, lut
    for a in out:
        a.setflags(write=False)
    return out


SHAPES = ((4, 4), (5, 7), (13, 18), (37, 66), (9, 1031), (261, 12), (20, 40))
BITS = (8, 12, 16)
KINDS = ("random", "max", "over")


def pitch_extra(shape):
    return 5 if shape == (9, 1031) else 0


def cases_of(shape, pattern):
    """[(quad, bits, kind)]: random and all-maximum data at every depth, samples above 2^bits - 1 at 12 bits; the quads alternate."""
    out = [(dr.QUADS[i % 2], b, "random") for i, b in enumerate(BITS)]
    out += [(dr.QUADS[(i + 1) % 2], b, "max") for i, b in enumerate(BITS)]
    out += [(dr.QUADS[1], 12, "over")]
    return out


@functools.lru_cache(maxsize=None)
def case_reference(shape, pattern, quad, bits, kind, mode, name):
    """(mosaic, views, total) of one case under one parameter set: computed once, shared, read-only."""
    m = dr.case_mosaic(shape, pattern, quad, bits, kind)
    p, lut = param_set(name, pattern, bits)
    v, t = develop(m, pattern, quad, bits, mode, p, lut)
    for a in (m, v, t):
        a.setflags(write=False)
    return m, v, t


def gray_frame(shape, pattern, bits, kind):
    """A frame for the grey-world tests: dofp_ref's case data; "mixed" = random data with saturated samples sprinkled into a third of the
    periods."""
    if kind != "mixed":
        return dr.case_mosaic(shape, pattern, dr.QUADS[0], bits, kind)
    m = np.array(dr.case_mosaic(shape, pattern, dr.QUADS[0], bits, "random"))
    rng = np.random.default_rng((shape[0], shape[1], bits))
    hit = rng.random(m.shape) < 0.03
    m[hit] = (1 << bits) - 1
    return m
