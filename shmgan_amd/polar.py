"""Polarimetry helpers: the Stokes fit behind the loader's estimated-diffuse target and the DoP / AoLP maps.

The reference carries two dead helpers: utils.calculate_estimate_diffuse (utils.py:68-123: per pixel and channel the minimum of
the four views at source size; its imwrite is commented out) and calcDOP (SHM.py:1157-1169: Stokes parameters from the
0/45/90/135 views with hard-coded coefficients).  Its training path reads a pre-computed ED/ directory instead.  Here both have a
device implementation (csrc/polar.hip) and this module holds the host side: the least-squares Stokes matrix for any set of
polariser angles, the reference's own coefficients, and the `imwrite` the reference left out.

The same fit gives a label the capture already contains: the polarised intensity sqrt(S1^2 + S2^2) is the specular part, and
`specular_mask` / `write_specular_masks` (csrc/specmask.hip) threshold it into the highlight masks SpecSeg is trained on
(data.MaskDataset.from_polar, trainer.train_specseg with specseg_mask_source="polar").

A polariser-mosaic sensor records the four views in one raw frame: `DofpLayout` describes such a sensor, `decode_mosaic` reads a frame
file, `demosaic` (csrc/dofp.hip) splits it into the four views in ascending angle, and `sample_views` is the one place where "a sample's
files" become "its four uint8 device views" for either kind of capture.  A layout with a `DofpDevelop` has its
frames developed inside that launch -- black level, white balance, colour matrix, tone curve (csrc/dofp_develop.hip; DESIGN.md section
6o); `estimate_white_balance` gives the one grey-world balance of a whole capture.  A layout with a `DofpCalibration` has every frame
corrected on the device first -- master dark, flat-field gain, defective photosites (csrc/dofp_calibrate.hip);
`build_calibration` makes one from a stack of dark frames and a stack of flats.  A layout with a `DofpBracket` reads an exposure bracket
per sample -- one multi-page TIFF (`write_bracket`, `pack_brackets`) -- and merges its pages on the device into a 16-bit mosaic
(`merge_bracket`; csrc/dofp_merge.hip) that everything else reads under `layout.merged`.

Importing this module needs no GPU; `polar_maps`, `specular_mask`, `demosaic`, `estimate_white_balance`, `write_estimated_diffuse` and
`write_specular_masks` run on one.

Model: a linear polariser at angle theta in front of light with Stokes parameters (S0, S1, S2) passes
    I(theta) = 0.5 * (S0 + S1 cos 2 theta + S2 sin 2 theta)
whose minimum over theta is 0.5 * (S0 - sqrt(S1^2 + S2^2)): the unpolarised (diffuse) half of the light.  The minimum of four
sampled angles is an upper bound of it (exact only when one polariser happens to sit at the minimum).
"""
from __future__ import annotations

import functools
import os
import re
from dataclasses import dataclass
from pathlib import Path

import numpy as np

from ._lib import CONSTANTS
from .data import BRACKET_EXT, PSD_SUBDIRS, list_images, mosaic_extensions

# S0 = I0 + I90, S1 = I0 - I90, S2 = I45 - I135: the coefficients calcDOP hard-codes (SHM.py:1158-1160).  Its S0 uses two of the
# four views; stokes_matrix([0, 45, 90, 135]) gives the least-squares S0 = (I0 + I45 + I90 + I135) / 2 with the same S1, S2.
REFERENCE_DOP_MATRIX = [[1, 0, 1, 0], [1, 0, -1, 0], [0, 1, 0, -1]]

_ANGLE_NAME = re.compile(r"^I(\d+(?:\.\d+)?)$")


def angles_from_subdirs(subdirs=("I0", "I60", "I90", "I150")):
    """Polariser angles in degrees from view directory names of the form I<degrees> (PSD: I0 I60 I90 I150; SHMGAN: I0 I45 I90
    I135).  Any other name (such as "ED") raises ValueError: pass `angles` explicitly for directories named otherwise."""
    out = []
    for s in subdirs:
        m = _ANGLE_NAME.match(str(s))
        if not m:
            raise ValueError(f"cannot read a polariser angle from the directory name {s!r} (expected I<degrees>, as in I60)")
        out.append(float(m.group(1)))
    return out


def _model_rows(angles_deg):
    """A[i] = 0.5 * (1, cos 2 theta_i, sin 2 theta_i) in float64, cos / sin of multiples of 90 degrees exactly, so that the textbook
    angle sets give the textbook matrices."""
    r = np.deg2rad(2.0 * np.asarray(angles_deg, dtype=np.float64).reshape(-1))
    return 0.5 * np.stack([np.ones_like(r), np.round(np.cos(r), 15), np.round(np.sin(r), 15)], axis=1)


def _stokes_f64(angles_deg):
    """stokes_matrix before the cast to float32."""
    th = np.asarray(angles_deg, dtype=np.float64).reshape(-1)
    distinct = []
    for t in np.mod(th, 180.0):
        if not any(min(abs(t - u), 180.0 - abs(t - u)) < 1e-9 for u in distinct):
            distinct.append(float(t))
    if len(distinct) < 3:
        raise ValueError(f"a Stokes fit needs at least three polariser angles that are distinct modulo 180 degrees, got "
                         f"{[float(t) for t in th]}")
    A = _model_rows(th)
    return np.linalg.solve(A.T @ A, A.T)


def stokes_matrix(angles_deg):
    """The least-squares 3 x n matrix C with (S0, S1, S2) = C . (I(theta_1) .. I(theta_n)) for the model above: the
    pseudo-inverse of A, A[i] = 0.5 * (1, cos 2 theta_i, sin 2 theta_i).  Computed in float64, returned as float32.  The fit
    needs three angles that are distinct modulo 180 degrees (theta and theta + 180 are the same polariser); fewer raise."""
    return _stokes_f64(angles_deg).astype(np.float32)


def mirror_views(angles_deg):
    """What mirroring the scene about one image axis does to views taken at `angles_deg`: a polariser at theta sees of the mirrored
    scene what a polariser at (180 - theta) mod 180 saw of the original.  Returns
      ("permute", perm)   every mirrored angle is in the set (within the 1e-9 of stokes_matrix): mirrored view i is view perm[i],
                          exactly -- [0, 3, 2, 1] for 0/45/90/135
      ("mix", M)          otherwise: M = A' . pinv(A), A'[i] = 0.5 (1, cos 2 theta'_i, sin 2 theta'_i), the views a polariser at
                          theta'_i = 180 - theta_i passes of the Stokes fit of the given ones; float64 arithmetic with the exact
                          multiples of 90 degrees of stokes_matrix, returned as float32 [n, n]
      ("identity", None)  the permutation is the identity
    Both mirrors together are a rotation by 180 degrees and leave every angle alone.  Fewer than three distinct angles raise, as
    stokes_matrix does."""
    pinv = _stokes_f64(angles_deg)
    th = np.mod(np.asarray(angles_deg, dtype=np.float64).reshape(-1), 180.0)
    mirrored = np.mod(180.0 - th, 180.0)
    perm = []
    for t in mirrored:
        hit = [j for j, u in enumerate(th) if min(abs(t - u), 180.0 - abs(t - u)) < 1e-9]
        if not hit:
            return "mix", (_model_rows(mirrored) @ pinv).astype(np.float32)
        perm.append(hit[0])
    return ("identity", None) if perm == list(range(len(perm))) else ("permute", perm)


def mirror_keeps_view(angles_deg, view=2):
    """Whether mirroring the scene leaves view `view` what it was: then that view of a mirrored capture is the mirrored view, and an
    (image, mask) pair made from it may take the plain geometric flip (data.MaskDataset.from_polar).  In terms of mirror_views:
    "identity", a "permute" with perm[view] == view, or a "mix" in which the view's own angle is mirror-invariant ((180 - theta)
    mod 180 == theta mod 180 within the 1e-9 of stokes_matrix, i.e. 0 or 90 degrees).  The last is decided on the angle and not on
    the matrix: with four views and three Stokes parameters row `view` of the mix is the least-squares FIT of that view -- for
    0/60/90/150 row 2 is (-0.25, 0.25, 0.75, 0.25), not the unit row -- although the polariser at 90 degrees sees of the mirrored
    scene exactly what it saw.  True for view 2 of both 0/45/90/135 and 0/60/90/150; false for 0/30/60/120, where 60 becomes 120."""
    kind, how = mirror_views(angles_deg)
    if kind == "identity":
        return True
    if kind == "permute":
        return how[view] == view
    th = float(np.mod(np.asarray(angles_deg, dtype=np.float64).reshape(-1)[view], 180.0))
    d = abs(float(np.mod(180.0 - th, 180.0)) - th)
    return min(d, 180.0 - d) < 1e-9


def polar_maps(views, angles, want=("s0", "dop", "aolp")):
    """Stokes maps of four float32 device views taken at `angles` (degrees): ops.polar_maps with the least-squares matrix."""
    from . import ops
    return ops.polar_maps(views, stokes_matrix(angles), want)


def _decode(path):
    from PIL import Image
    with Image.open(path) as im:
        return np.array(im.convert("RGB"), dtype=np.uint8)


# ---- polariser-mosaic (division-of-focal-plane) sensors: one raw frame per sample (csrc/dofp.hip) ----------
DOFP_PATTERNS = ("mono", "rggb", "bggr", "grbg", "gbrg")       # no colour filter, or the Bayer tile that lies over the 2 x 2 quads
DOFP_DEMOSAIC = ("bilinear", "bin")                            # views at the mosaic's size / one pixel per super-pixel
CAPTURES = ("views", "dofp")                                   # one file per polariser angle / one mosaic per sample


DOFP_TONES = ("linear", "srgb")                                # or a gamma g in [1, 4]: x^(1/g)
# the parameter block of shm_dofp_develop: offsets into its int32 words, from include/shmgan_hip.h
DEVELOP_BLACK, DEVELOP_MUL, DEVELOP_GAIN, DEVELOP_FLAGS, DEVELOP_CCM, DEVELOP_WHITE, DEVELOP_PARAMS = (
    CONSTANTS["SHM_DOFP_" + k] for k in ("P_BLACK", "P_MUL", "P_GAIN", "P_FLAGS", "P_CCM", "P_WHITE", "PARAMS"))


def _triple(v, kind):
    """v as a 3-tuple of `kind`: a scalar is repeated; anything else must hold three."""
    if isinstance(v, (str, bytes, bool)):
        raise TypeError
    if isinstance(v, (int, float, np.integer, np.floating)):
        v = (v, v, v)
    v = tuple(v)
    if len(v) != 3 or any(isinstance(x, (str, bytes, bool)) for x in v):
        raise TypeError
    return tuple(kind(x) for x in v)


def _whole(x):
    if isinstance(x, (float, np.floating)) and float(x) != int(x):
        raise ValueError
    return int(x)


def tone_table(tone):
    """The 4096 uint8 entries of a tone curve, indexed by the top 12 of 16 linear bits: round-to-nearest of 255 f(i / 4095), f the
    identity ("linear"), the piecewise sRGB encoding ("srgb") or x^(1/g) for a gamma g."""
    x = np.arange(4096, dtype=np.float64) / 4095.0
    if tone == "linear":
        f = x
    elif tone == "srgb":
        f = np.where(x <= 0.0031308, 12.92 * x, 1.055 * np.power(x, 1.0 / 2.4) - 0.055)
    else:
        f = np.power(x, 1.0 / float(tone))
    return np.floor(255.0 * f + 0.5).astype(np.uint8)


@dataclass(frozen=True)
class DofpDevelop:
    """How a polariser-mosaic frame is developed inside the demosaic launch (shm_dofp_develop, include/shmgan_hip.h): the sensor's
    black level is removed, the colours are balanced, optionally mixed by a 3 x 3 matrix, and the 16-bit linear result is encoded
    to 8 bits by a tone table.  black: the count for darkness, a scalar or an (R, G, B) triple.  white: the count of a saturated
    sample, default 2^bits - 1 of the layout.  wb: the (R, G, B) balance, normalised so that its smallest entry is 1 (every entry
    then at most 16), or "gray": grey-world gains estimated from every frame on the device (shm_dofp_wb_gray; Bayer patterns only;
    estimate_white_balance gives ONE triple for a whole capture, which is what a rig under one illuminant should use).  ccm: a 3 x 3
    row-major matrix applied to the balanced linear values (entries within +-7.99; Bayer patterns only).  tone: "srgb", "linear"
    or a gamma in [1, 4].  sat: samples at or above it exclude their 4 x 4 period from the "gray" estimate, default `white`.
    `table(layout)` is the one quantisation of these options: the kernel and the tests read nothing else."""
    black: object = 0
    white: object = None
    wb: object = (1, 1, 1)
    ccm: object = None
    tone: object = "srgb"
    sat: object = None

    def __post_init__(self):
        put = lambda k, v: object.__setattr__(self, k, v)
        try:
            black = _triple(self.black, _whole)
        except (TypeError, ValueError, OverflowError):
            raise ValueError(f"DofpDevelop: black {self.black!r} is not a count or three counts") from None
        if not all(0 <= b <= 65535 - 16 for b in black):
            raise ValueError(f"DofpDevelop: black {self.black!r} outside [0, 65519]")
        put("black", black)
        if self.white is not None:
            try:
                if isinstance(self.white, (bool, str)):
                    raise TypeError
                white = _whole(self.white)
            except (TypeError, ValueError, OverflowError):
                raise ValueError(f"DofpDevelop: white {self.white!r} is not a count") from None
            if not 16 <= white <= 65535 or any(white - b < 16 for b in black):
                raise ValueError(f"DofpDevelop: white {self.white!r} is not in [16, 65535] and at least 16 above black {black}")
            put("white", white)
        if isinstance(self.wb, str):
            if self.wb != "gray":
                raise ValueError(f"DofpDevelop: wb {self.wb!r} is not three gains or 'gray'")
        else:
            try:
                wb = _triple(self.wb, float)
            except (TypeError, ValueError):
                raise ValueError(f"DofpDevelop: wb {self.wb!r} is not three gains or 'gray'") from None
            if not all(np.isfinite(g) and g > 0 for g in wb):
                raise ValueError(f"DofpDevelop: wb {self.wb!r} is not three positive gains")
            if max(wb) > 16 * min(wb):
                raise ValueError(f"DofpDevelop: wb {self.wb!r} spans more than a factor of 16")
            put("wb", wb)
        if self.ccm is not None:
            try:
                ccm = tuple(float(x) for x in np.asarray(self.ccm, dtype=np.float64).reshape(-1))
            except (TypeError, ValueError):
                raise ValueError(f"DofpDevelop: ccm {self.ccm!r} is not a 3 x 3 matrix") from None
            if len(ccm) != 9 or not all(np.isfinite(x) for x in ccm):
                raise ValueError(f"DofpDevelop: ccm {self.ccm!r} is not a 3 x 3 matrix")
            if any(abs(int(np.floor(x * 1024 + 0.5))) > 8191 for x in ccm):
                raise ValueError(f"DofpDevelop: ccm {self.ccm!r} has an entry outside +-8191 / 1024")
            put("ccm", ccm)
        if isinstance(self.tone, str):
            if self.tone not in DOFP_TONES:
                raise ValueError(f"DofpDevelop: tone {self.tone!r} is not one of {DOFP_TONES} or a gamma in [1, 4]")
        else:
            try:
                if isinstance(self.tone, bool):
                    raise TypeError
                g = float(self.tone)
            except (TypeError, ValueError):
                raise ValueError(f"DofpDevelop: tone {self.tone!r} is not one of {DOFP_TONES} or a gamma in [1, 4]") from None
            if not 1.0 <= g <= 4.0:
                raise ValueError(f"DofpDevelop: tone {self.tone!r} is not one of {DOFP_TONES} or a gamma in [1, 4]")
            put("tone", g)
        if self.sat is not None:
            try:
                if isinstance(self.sat, (bool, str)):
                    raise TypeError
                sat = _whole(self.sat)
            except (TypeError, ValueError, OverflowError):
                raise ValueError(f"DofpDevelop: sat {self.sat!r} is not a count") from None
            if not 1 <= sat <= 65536:
                raise ValueError(f"DofpDevelop: sat {self.sat!r} outside [1, 65536]")
            put("sat", sat)

    def table(self, layout):
        """(params int32 [20], lut uint8 [4096], mirror): the parameter block and tone table shm_dofp_develop reads for a sensor laid
        out as `layout` (its pattern and bits), and the host copy of the block the entry point makes its refusals from.  Gains are
        1024; wb "gray" leaves the balance to the device.  Arrays are read-only and shared between calls."""
        return _develop_table(self, layout.pattern, layout.bits)

    def saturation(self, layout):
        """The count from which a sample excludes its period from the grey-world sums: `sat`, or the white level."""
        return self.sat if self.sat is not None else int(self.table(layout)[0][DEVELOP_WHITE])


@functools.lru_cache(maxsize=None)
def _develop_table(dev, pattern, bits):
    from fractions import Fraction
    white = dev.white if dev.white is not None else (1 << bits) - 1
    if any(white - b < 16 for b in dev.black):
        raise ValueError(f"DofpDevelop: white {white} ({bits} bits) is not at least 16 above black {dev.black}")
    wb = (1.0, 1.0, 1.0) if dev.wb == "gray" else dev.wb
    if pattern == "mono":
        if dev.wb == "gray":
            raise ValueError("DofpDevelop: wb 'gray' needs a Bayer pattern, the layout is 'mono'")
        if dev.ccm is not None:
            raise ValueError("DofpDevelop: ccm needs a Bayer pattern, the layout is 'mono'")
        if len(set(dev.black)) != 1 or len(set(wb)) != 1:
            raise ValueError(f"DofpDevelop: black {dev.black} and wb {wb} must be the same for all channels of a 'mono' layout")
    low = min(Fraction(g) for g in wb)
    p = np.zeros(DEVELOP_PARAMS, dtype=np.int64)
    for c in range(3):
        mul = Fraction(65535 * 65536) * (Fraction(wb[c]) / low) / (white - dev.black[c])
        p[DEVELOP_BLACK + c] = dev.black[c]
        p[DEVELOP_MUL + c] = int(mul + Fraction(1, 2))              # floor(x + 1/2): round half up; 65536 <= mul < 2^32
        p[DEVELOP_GAIN + c] = 1024
    if dev.ccm is not None:
        p[DEVELOP_FLAGS] = 1
        p[DEVELOP_CCM:DEVELOP_CCM + 9] = [int(np.floor(x * 1024 + 0.5)) for x in dev.ccm]
    p[DEVELOP_WHITE] = white
    params = p.astype(np.uint32).view(np.int32)                     # mul travels as its bit pattern
    lut = tone_table(dev.tone)
    mirror = params.copy()
    for a in (params, lut, mirror):
        a.setflags(write=False)
    return params, lut, mirror


# ---- calibrating the sensor: master dark, flat field, defect map (csrc/dofp_calibrate.hip) -------------------
GAIN_MIN, GAIN_MAX = CONSTANTS["SHM_DOFP_GAIN_MIN"], CONSTANTS["SHM_DOFP_GAIN_MAX"]       # Q12, 4096 = 1
DEFECT_HOT, DEFECT_UNUSABLE, DEFECT_RANGE = 1, 2, 4       # why build_calibration marked a site; the kernel reads non-zero


def pattern_channels(pattern, h, w):
    """The colour class of every photosite of an [h,w] mosaic under `pattern`, int [h,w]: 0 everywhere for "mono"; 0 R, 1 G, 2 B for a
    Bayer tile, whose letter at colour block (by, bx) = ((y % 4) // 2, (x % 4) // 2) is pattern[2 by + bx]."""
    if pattern not in DOFP_PATTERNS:
        raise ValueError(f"pattern {pattern!r} is not one of {DOFP_PATTERNS}")
    if pattern == "mono":
        return np.zeros((h, w), dtype=np.int64)
    blk = ((np.arange(h) % 4) // 2)[:, None] * 2 + ((np.arange(w) % 4) // 2)[None, :]
    return np.array(["rgb".index(c) for c in pattern], dtype=np.int64)[blk]


class DofpCalibration:
    """What shm_dofp_calibrate (include/shmgan_hip.h states the arithmetic) corrects a polariser-mosaic frame with, before it is
    demosaiced: dark = the master dark frame (uint16 [h,w], pedestal included; None = `pedestal` everywhere), gain = the flat-field gain
    in Q12 (uint16 [h,w], 4096 = 1, every entry in [1024, 16383]; None = 1 everywhere), defect = the map of photosites to replace by the
    mean of their good same-lattice neighbours (uint8 [h,w], non-zero = defective; build_calibration sets DEFECT_HOT, DEFECT_UNUSABLE or
    DEFECT_RANGE; None = none).  pedestal: the count the corrected dark level is put back to (it is kept, so DofpDevelop.black goes on
    meaning the sensor's black level).  white: samples at or above it are saturated and pass through untouched, default 2^bits - 1.
    pattern, bits: the sensor's, as DofpLayout's; a layout takes only a calibration of its own pattern and bits.  reference: the
    per-colour (S_c, n_c) build_calibration equalised the flat to, or None.

    The arrays are copied and read-only.  Equality and hash go by a digest of the contents computed once here, so two loads of one file
    are equal and a layout that carries a calibration stays hashable.  Refusals are ValueErrors by name."""

    def __init__(self, dark=None, gain=None, defect=None, pedestal=0, white=None, pattern="mono", bits=8, reference=None):
        import hashlib
        if pattern not in DOFP_PATTERNS:
            raise ValueError(f"DofpCalibration: pattern {pattern!r} is not one of {DOFP_PATTERNS}")
        if isinstance(bits, bool) or not isinstance(bits, (int, np.integer)) or not 8 <= int(bits) <= 16:
            raise ValueError(f"DofpCalibration: bits {bits!r} is not an integer in 8..16")
        if isinstance(pedestal, (bool, str)) or not isinstance(pedestal, (int, np.integer)) or not 0 <= int(pedestal) <= 65535 - 16:
            raise ValueError(f"DofpCalibration: pedestal {pedestal!r} is not a count in [0, 65519]")
        if white is not None and (isinstance(white, (bool, str)) or not isinstance(white, (int, np.integer)) or not 1 <= int(white) <= 65536):
            raise ValueError(f"DofpCalibration: white {white!r} is not a count in [1, 65536]")
        shape, arrays = None, {}
        for name, a, dtype in (("dark", dark, np.uint16), ("gain", gain, np.uint16), ("defect", defect, np.uint8)):
            if a is not None:
                if not isinstance(a, np.ndarray) or a.dtype != dtype:
                    raise ValueError(f"DofpCalibration: {name} must be a {np.dtype(dtype).name} array, got "
                                     f"{a.dtype if isinstance(a, np.ndarray) else type(a).__name__}")
                if a.ndim != 2 or a.shape[0] < 1 or a.shape[1] < 1 or (shape is not None and a.shape != shape):
                    raise ValueError(f"DofpCalibration: {name} has shape {a.shape}, " + ("the tables are 2-D [h,w]" if shape is None or a.ndim != 2 else
                                                                                        f"the other tables have {shape}"))
                shape = a.shape
                a = np.array(a, dtype=dtype, order="C", copy=True)
                a.setflags(write=False)
            arrays[name] = a
        if arrays["gain"] is not None and (int(arrays["gain"].min()) < GAIN_MIN or int(arrays["gain"].max()) > GAIN_MAX):
            raise ValueError(f"DofpCalibration: gain spans [{int(arrays['gain'].min())}, {int(arrays['gain'].max())}], outside the Q12 range "
                             f"[{GAIN_MIN}, {GAIN_MAX}]")
        if reference is not None:
            try:
                reference = tuple((int(s), int(n)) for s, n in reference)
            except (TypeError, ValueError):
                raise ValueError(f"DofpCalibration: reference {reference!r} is not a (S, n) pair per colour") from None
            if len(reference) != (1 if pattern == "mono" else 3):
                raise ValueError(f"DofpCalibration: reference {reference!r} is not a (S, n) pair per colour of pattern {pattern!r}")
        self.dark, self.gain, self.defect = arrays["dark"], arrays["gain"], arrays["defect"]
        self.pedestal, self.white, self.pattern, self.bits = int(pedestal), None if white is None else int(white), pattern, int(bits)
        self.shape = None if shape is None else (int(shape[0]), int(shape[1]))
        self._reference = reference
        m = hashlib.sha256(repr((self.pedestal, self.white, self.pattern, self.bits, self.shape, reference)).encode())
        for a in (self.dark, self.gain, self.defect):
            m.update(b"-" if a is None else a.tobytes())
        self.digest = m.hexdigest()
        self._frozen = True

    def __setattr__(self, k, v):
        if getattr(self, "_frozen", False):
            raise AttributeError(f"DofpCalibration is read-only (cannot set {k})")
        object.__setattr__(self, k, v)

    def __eq__(self, other):
        return isinstance(other, DofpCalibration) and other.digest == self.digest

    def __hash__(self):
        return hash(self.digest)

    def __repr__(self):
        return (f"DofpCalibration({self.pattern!r}, bits={self.bits}, shape={self.shape}, pedestal={self.pedestal}, white={self.white}, "
                f"digest={self.digest[:12]})")

    @property
    def period(self):
        return 2 if self.pattern == "mono" else 4

    @property
    def white_level(self):
        """The count from which a sample passes through untouched: `white`, or 2^bits - 1."""
        return self.white if self.white is not None else (1 << self.bits) - 1

    @property
    def reference(self):
        """The per-colour (S_c, n_c) of build_calibration: the sum and count of the dark-subtracted flat over the usable sites of colour
        c (one class for "mono"; R, G, B otherwise); every good site's corrected flat is pedestal + S_c / n_c within the rounding.
        None for a calibration without a flat field."""
        return self._reference

    def summary(self):
        """dict(sites, hot, unusable, out_of_range, defective, gain_min, gain_max): the counts of the defect map's three reasons (a site may
        have more than one), of its non-zero entries, and the gain's range in Q12 (4096, 4096 without a gain table)."""
        d = self.defect if self.defect is not None else np.zeros((0, 0), dtype=np.uint8)
        g = self.gain
        return dict(sites=0 if self.shape is None else self.shape[0] * self.shape[1],
                    hot=int(np.count_nonzero(d & DEFECT_HOT)), unusable=int(np.count_nonzero(d & DEFECT_UNUSABLE)),
                    out_of_range=int(np.count_nonzero(d & DEFECT_RANGE)), defective=int(np.count_nonzero(d)),
                    gain_min=4096 if g is None else int(g.min()), gain_max=4096 if g is None else int(g.max()))

    def save(self, path):
        """Write the calibration as an .npz (no pickle): the arrays that are not None, the scalars, and the reference as int64 [n, 2]."""
        out = {k: getattr(self, k) for k in ("dark", "gain", "defect") if getattr(self, k) is not None}
        out.update(pedestal=np.int64(self.pedestal), white=np.int64(-1 if self.white is None else self.white), bits=np.int64(self.bits),
                   pattern=np.array(self.pattern))
        if self._reference is not None:
            out["reference"] = np.array(self._reference, dtype=np.int64).reshape(-1, 2)
        with open(path, "wb") as f:
            np.savez(f, **out)

    @classmethod
    def load(cls, path):
        """The calibration `save` wrote; a file that is not one raises ValueError naming it."""
        try:
            with np.load(path, allow_pickle=False) as z:
                white = int(z["white"])
                return cls(*(z[k] if k in z.files else None for k in ("dark", "gain", "defect")), pedestal=int(z["pedestal"]),
                           white=None if white < 0 else white, pattern=str(z["pattern"]), bits=int(z["bits"]),
                           reference=[tuple(r) for r in z["reference"].tolist()] if "reference" in z.files else None)
        except (KeyError, OSError, TypeError) as e:
            raise ValueError(f"DofpCalibration: {path} is not a saved calibration ({type(e).__name__}: {e})") from None
        except ValueError as e:
            raise ValueError(f"{e} (loading {path})" if str(e).startswith("DofpCalibration: ") else
                             f"DofpCalibration: {path} is not a saved calibration ({e})") from None


def _stack_mean(files, layout, shape, who):
    """(2 sum + N) // (2 N) of the decoded frames, int64 [h,w], and their shape: the round-half-up mean of a stack."""
    total = None
    for f in files:
        a = decode_mosaic(f, layout)
        if shape is not None and a.shape != shape:
            raise ValueError(f"{who}: {f} is {a.shape[0]} x {a.shape[1]}, the frames before it are {shape[0]} x {shape[1]}")
        shape = a.shape
        total = a.astype(np.int64) if total is None else total + a
    n = len(files)
    return (2 * total + n) // (2 * n), shape


def build_calibration(layout, dark_dir, flat_dir=None, hot_threshold=None, gain_limits=(0.5, 2.0), white=None):
    """A DofpCalibration from a stack of dark frames and, optionally, a stack of flat frames of the sensor `layout` describes (its pattern
    and bits; files as decode_mosaic reads them).  Exact integer NumPy on the host: a one-off, not a loader path.

    The dark frames are taken with the lens capped, at the exposure and gain of the capture.  The FLAT FRAMES NEED UNPOLARISED, UNIFORM
    ILLUMINATION -- an integrating sphere or a diffuser in front of the lens, and no polarising surface in the path: the reference level
    is taken per colour over all four orientations, which is what equalises the four micro-polarisers, so any polarisation of the flat
    light is calibrated INTO the gains and then out of every capture.  They should be well exposed and below saturation.

      dark      = (2 sum D_i + N) // (2 N)                            the rounded mean of the dark stack
      pedestal  = the lower median of dark
      hot       = dark > pedestal + hot_threshold                     default 8 << (bits - 8): 8 byte units
    Without flats: defect = hot, no gain table.  With flats:
      fm        = the same rounded mean of the flat stack;  f = fm - dark
      usable    = ~hot & (f > 0) & (fm < white)                       white: default 2^bits - 1
      S_c, n_c  = sum and count of f over the usable sites of colour c (one class for "mono")
      g         = (8192 S_c + n_c f) // (2 n_c f)                     the round-half-up of 4096 (S_c / n_c) / f
      defect    = ~usable | g outside the Q12 images of gain_limits;  gain = g, 4096 at defects
    The defect map holds the reason (DEFECT_HOT | DEFECT_UNUSABLE | DEFECT_RANGE).  ValueError naming the directory or file for an empty
    directory, a frame of another size, or a colour without a usable site."""
    if not isinstance(layout, DofpLayout):
        raise ValueError(f"build_calibration: layout must be a polar.DofpLayout, got {layout!r}")
    bits = layout.bits
    thr = 8 << (bits - 8) if hot_threshold is None else int(hot_threshold)
    if thr < 0:
        raise ValueError(f"build_calibration: hot_threshold {hot_threshold!r} is negative")
    try:
        lo, hi = (int(np.floor(float(x) * 4096 + 0.5)) for x in gain_limits)
    except (TypeError, ValueError):
        raise ValueError(f"build_calibration: gain_limits {gain_limits!r} are not two factors") from None
    if not GAIN_MIN <= lo <= 4096 <= hi <= GAIN_MAX:
        raise ValueError(f"build_calibration: gain_limits {gain_limits!r} must enclose 1 inside [{GAIN_MIN / 4096}, {GAIN_MAX / 4096:.4f}]")
    white_level = (1 << bits) - 1 if white is None else int(white)
    plain = DofpLayout(layout.pattern, layout.quad_angles, bits)          # decode only: no size check against an older calibration
    files = list_images(str(dark_dir))
    if not files:
        raise ValueError(f"build_calibration: no dark frames in {dark_dir}")
    dark, shape = _stack_mean(files, plain, None, "build_calibration")
    pedestal = int(np.sort(dark, axis=None)[(dark.size - 1) // 2])
    hot = dark > pedestal + thr
    defect = np.where(hot, DEFECT_HOT, 0).astype(np.uint8)
    if flat_dir is None:
        return DofpCalibration(dark.astype(np.uint16), None, defect, pedestal, white, layout.pattern, bits)
    files = list_images(str(flat_dir))
    if not files:
        raise ValueError(f"build_calibration: no flat frames in {flat_dir}")
    fm, _ = _stack_mean(files, plain, shape, "build_calibration")
    f = fm - dark
    usable = ~hot & (f > 0) & (fm < white_level)
    chan = pattern_channels(layout.pattern, *shape)
    gain = np.full(shape, 4096, dtype=np.int64)
    reference = []
    for c in range(1 if layout.pattern == "mono" else 3):
        sel = usable & (chan == c)
        S, n = int(f[sel].sum()), int(np.count_nonzero(sel))
        if n == 0:
            raise ValueError(f"build_calibration: no usable {'site' if layout.pattern == 'mono' else 'RGB'[c] + ' site'} in the flat frames of "
                             f"{flat_dir} (hot, not above the dark frame, or at the white level {white_level})")
        reference.append((S, n))
        fc = f[sel]
        gain[sel] = (8192 * S + n * fc) // (2 * n * fc)
    out = usable & ((gain < lo) | (gain > hi))
    defect |= np.where(~usable, DEFECT_UNUSABLE, 0).astype(np.uint8) | np.where(out, DEFECT_RANGE, 0).astype(np.uint8)
    gain[defect != 0] = 4096
    return DofpCalibration(dark.astype(np.uint16), gain.astype(np.uint16), defect, pedestal, white, layout.pattern, bits, reference)


# ---- exposure brackets: n pages of one mosaic merged into a 16-bit one (csrc/dofp_merge.hip) -------------------
MERGE_MAX, MERGE_TABLE, MERGE_Q = CONSTANTS["SHM_DOFP_MERGE_MAX"], CONSTANTS["SHM_DOFP_MERGE_TABLE"], CONSTANTS["SHM_DOFP_MERGE_Q"]


def _count_or_none(who, name, v, lo, hi):
    if v is None:
        return None
    if isinstance(v, (bool, str)) or not isinstance(v, (int, np.integer)) or not lo <= int(v) <= hi:
        raise ValueError(f"{who}: {name} {v!r} is not a count in [{lo}, {hi}]")
    return int(v)


@dataclass(frozen=True)
class DofpBracket:
    """An exposure bracket of a static scene: shm_dofp_merge (include/shmgan_hip.h states the arithmetic) merges its pages into one 16-bit
    mosaic on the scale of the shortest exposure, every unsaturated page voting with its exposure time.  exposures: 2 to 8 positive
    integers of at most 65535 in PAGE order, in any unit (only the ratios matter; they need not be sorted).  black: the count for
    darkness; None = the pedestal of the layout's calibration when it has one, else 0.  white: the count from which a sample is
    saturated; None = the calibration's white level when there is one, else 2^bits - 1.  `table(bits)` is the one quantisation of the
    exposures: the kernel and the tests read nothing else.  Refusals are ValueErrors by name."""
    exposures: tuple
    black: object = None
    white: object = None

    def __post_init__(self):
        try:
            if isinstance(self.exposures, (str, bytes)):
                raise TypeError
            raw = tuple(self.exposures)
        except TypeError:
            raise ValueError(f"DofpBracket: exposures {self.exposures!r} are not 2 to {MERGE_MAX} positive integers") from None
        if not 2 <= len(raw) <= MERGE_MAX or any(isinstance(e, bool) or not isinstance(e, (int, np.integer)) for e in raw):
            raise ValueError(f"DofpBracket: exposures {self.exposures!r} are not 2 to {MERGE_MAX} positive integers")
        if not all(1 <= int(e) <= 65535 for e in raw):
            raise ValueError(f"DofpBracket: exposures {self.exposures!r} are not all in [1, 65535]")
        object.__setattr__(self, "exposures", tuple(int(e) for e in raw))
        object.__setattr__(self, "black", _count_or_none("DofpBracket", "black", self.black, 0, 65535 - 16))
        object.__setattr__(self, "white", _count_or_none("DofpBracket", "white", self.white, 1, 65536))
        if self.black is not None and self.white is not None and self.white <= self.black:
            raise ValueError(f"DofpBracket: white {self.white} is not above black {self.black}")

    @property
    def pages(self):
        return len(self.exposures)

    def table(self, bits):
        """mul of shm_dofp_merge for samples of `bits` bits: uint32 [256], read-only and shared between calls; entry m, the mask of the
        valid pages, is the round-half-up of e_min * 2^(16 - bits) * 2^20 / (the sum of the valid pages' exposures)."""
        if isinstance(bits, bool) or not isinstance(bits, (int, np.integer)) or not 8 <= int(bits) <= 16:
            raise ValueError(f"DofpBracket: bits {bits!r} is not an integer in 8..16")
        return _merge_table(self.exposures, int(bits))

    def levels(self, bits, calibration=None):
        """(black, white) as the merge takes them for samples of `bits` bits: the given counts, else the calibration's pedestal and
        white level, else 0 and 2^bits - 1.  What shm_dofp_merge would refuse is refused here, by name."""
        f = 16 - int(bits)
        black = self.black if self.black is not None else calibration.pedestal if calibration is not None else 0
        white = self.white if self.white is not None else calibration.white_level if calibration is not None else (1 << bits) - 1
        if (black << f) > 65535 - 16:
            raise ValueError(f"DofpBracket: black {black} << {f} is above 65519, the merged mosaic's limit for a black level")
        if not 1 <= white <= 1 << bits:
            raise ValueError(f"DofpBracket: white {white} outside [1, {1 << bits}] for {bits}-bit samples")
        if white <= black:
            raise ValueError(f"DofpBracket: white {white} is not above black {black}")
        return black, white


@functools.lru_cache(maxsize=None)
def _merge_table(exposures, bits):
    f, n = 16 - bits, len(exposures)
    top = min(exposures) << (f + MERGE_Q)
    mul = np.zeros(MERGE_TABLE, dtype=np.uint32)
    for m in range(1, 1 << n):
        T = sum(e for k, e in enumerate(exposures) if m >> k & 1)
        mul[m] = (2 * top + T) // (2 * T)
    mul.setflags(write=False)
    return mul


@dataclass(frozen=True)
class DofpLayout:
    """How a polariser-mosaic sensor lays its samples out.  pattern: "mono", or the Bayer tile over the quads ("rggb", "bggr",
    "grbg", "gbrg": period 4).  quad_angles: the micro-polariser angles in degrees at quad positions (0,0), (0,1), (1,0), (1,1); Sony's
    IMX250MZR / MYR is (90, 45, 135, 0).  bits: the significant bits of a sample, LSB-aligned, 8..16 (8 = a uint8 mosaic; a
    12-bit value stored in 16 bits is 12, an MSB-aligned 16-bit file is 16).  develop: None = the views are the raw counts cut to 8
    bits (shm_dofp_views), or a DofpDevelop: black level, white balance, matrix and tone curve inside the demosaic launch.
    calibration: None, or the sensor's DofpCalibration (of this pattern and these bits): every frame is corrected on the device --
    dark frame, flat field, defect map (shm_dofp_calibrate) -- before anything else reads it.
    bracket: None, or a DofpBracket: a sample is then n pages [n,h,w] of one mosaic (one multi-page TIFF), each page is calibrated, the
    pages are merged on the device (shm_dofp_merge) into a 16-bit mosaic on the scale of the shortest exposure, and everything after
    that reads it as `merged` says.
    Views are always delivered in ASCENDING angle (`angles`), whatever the quad's order, so stokes_matrix(layout.angles) and the
    exact 45 / 135 exchange of mirror_views apply as they are; `quad` is the kernel's table, the view index at each quad position."""
    pattern: str = "mono"
    quad_angles: tuple = (90, 45, 135, 0)
    bits: int = 8
    develop: DofpDevelop | None = None
    calibration: DofpCalibration | None = None
    bracket: DofpBracket | None = None

    def __post_init__(self):
        if self.pattern not in DOFP_PATTERNS:
            raise ValueError(f"DofpLayout: pattern {self.pattern!r} is not one of {DOFP_PATTERNS}")
        try:
            ang = tuple(float(a) for a in self.quad_angles)
        except (TypeError, ValueError):
            raise ValueError(f"DofpLayout: quad_angles {self.quad_angles!r} are not four angles in degrees") from None
        if len(ang) != 4 or not all(np.isfinite(a) for a in ang):
            raise ValueError(f"DofpLayout: quad_angles {self.quad_angles!r} are not four angles in degrees")
        mod = sorted(a % 180.0 for a in ang)
        if any(min(b - a, 180.0 - (b - a)) < 1e-9 for i, a in enumerate(mod) for b in mod[i + 1:]):
            raise ValueError(f"DofpLayout: quad_angles {self.quad_angles!r} are not distinct modulo 180 degrees")
        if isinstance(self.bits, bool) or not isinstance(self.bits, (int, np.integer)) or not 8 <= int(self.bits) <= 16:
            raise ValueError(f"DofpLayout: bits {self.bits!r} is not an integer in 8..16")
        object.__setattr__(self, "quad_angles", ang)
        object.__setattr__(self, "bits", int(self.bits))
        if self.develop is not None:
            if not isinstance(self.develop, DofpDevelop):
                raise ValueError(f"DofpLayout: develop {self.develop!r} is not a polar.DofpDevelop or None")
            self.develop.table(self)          # what this sensor cannot be developed with is refused here, by name
        if self.calibration is not None:
            cal = self.calibration
            if not isinstance(cal, DofpCalibration):
                raise ValueError(f"DofpLayout: calibration {cal!r} is not a polar.DofpCalibration or None")
            if cal.pattern != self.pattern:
                raise ValueError(f"DofpLayout: calibration is of pattern {cal.pattern!r}, the layout is {self.pattern!r}")
            if cal.bits != self.bits:
                raise ValueError(f"DofpLayout: calibration is of bits = {cal.bits}, the layout says bits = {self.bits}")
        if self.bracket is not None:
            if not isinstance(self.bracket, DofpBracket):
                raise ValueError(f"DofpLayout: bracket {self.bracket!r} is not a polar.DofpBracket or None")
            self.merged          # a level the 16-bit mosaic cannot hold is refused here, by name

    @property
    def bracket_levels(self):
        """(black, white) of the merge in counts of one page: the bracket's, else the calibration's pedestal and white level, else 0 and
        2^bits - 1."""
        try:
            return self.bracket.levels(self.bits, self.calibration)
        except ValueError as e:
            raise ValueError(str(e).replace("DofpBracket: ", "DofpLayout: bracket ", 1)) from None

    @property
    def merged(self):
        """The layout of the mosaic shm_dofp_merge makes of this layout's pages (the layout itself without a bracket): the same pattern
        and quad, bits = 16, no calibration and no bracket, and the development moved onto the merged scale, f = 16 - bits: its blacks
        << f, its white min(65535, W << f) with W the development's white when given, else the bracket's, its sat min(65536, sat << f)
        when given.  So dofp_black / dofp_white stay in counts of the shortest exposure, and without a development the views are the top
        8 bits of the merged frame."""
        if self.bracket is None:
            return self
        return _merged_layout(self)

    @property
    def angles(self):
        """The four angles in ascending order: the order of the delivered views."""
        return sorted(self.quad_angles)

    @property
    def quad(self):
        """View index (into `angles`) at quad positions (0,0), (0,1), (1,0), (1,1): (2, 1, 3, 0) for Sony's layout."""
        order = self.angles
        return tuple(order.index(a) for a in self.quad_angles)

    @property
    def period(self):
        return 2 if self.pattern == "mono" else 4

    def view_shape(self, h, w, mode="bilinear"):
        """(ho, wo) of the views of an [h,w] mosaic."""
        if mode not in DOFP_DEMOSAIC:
            raise ValueError(f"dofp_demosaic {mode!r} is not one of {DOFP_DEMOSAIC}")
        return (int(h), int(w)) if mode == "bilinear" else (int(h) // self.period, int(w) // self.period)


@functools.lru_cache(maxsize=None)
def _merged_layout(layout):
    f = 16 - layout.bits
    _, white = layout.bracket_levels
    dev = layout.develop
    if dev is not None:
        if any((b << f) > 65535 - 16 for b in dev.black):
            raise ValueError(f"DofpLayout: develop black {dev.black} << {f} is above 65519, the merged mosaic's limit for a black level")
        try:
            dev = DofpDevelop(tuple(b << f for b in dev.black), min(65535, (dev.white if dev.white is not None else white) << f), dev.wb, dev.ccm,
                              dev.tone, None if dev.sat is None else min(65536, dev.sat << f))
            return DofpLayout(layout.pattern, layout.quad_angles, 16, dev)
        except ValueError as e:
            raise ValueError(f"DofpLayout: the development of the merged mosaic (levels << {f}): {e}") from None
    return DofpLayout(layout.pattern, layout.quad_angles, 16)


def check_capture(capture, dofp, dofp_demosaic="bilinear", who="PolarDataset"):
    """The refusals every entry point that takes the capture options shares, by name and before anything is listed or allocated."""
    if capture not in CAPTURES:
        raise ValueError(f"{who}: capture {capture!r} is not one of {CAPTURES}")
    if dofp_demosaic not in DOFP_DEMOSAIC:
        raise ValueError(f"{who}: dofp_demosaic {dofp_demosaic!r} is not one of {DOFP_DEMOSAIC}")
    if capture == "dofp" and not isinstance(dofp, DofpLayout):
        raise ValueError(f"{who}: capture 'dofp' needs dofp=polar.DofpLayout(...), got {dofp!r}")
    if capture == "views" and dofp is not None and not isinstance(dofp, DofpLayout):
        raise ValueError(f"{who}: dofp must be a polar.DofpLayout or None, got {dofp!r}")


def decode_mosaic(path, layout):
    """One raw mosaic file as a 2-D array: PIL mode "L" gives uint8 and needs layout.bits == 8; "I;16" / "I;16B" give uint16 (native
    byte order) and need bits 9..16.  Anything else -- an RGB file is not a mosaic -- raises ValueError naming the file and its mode, and
    so does a frame whose size is not that of the layout's calibration tables, naming both sizes.  With a bracketed layout the file is one
    multi-page TIFF, pages in the order of the bracket's exposures, and the result is [n,h,w]; a page count other than n, or pages of
    unequal size or mode, raise ValueError naming the file."""
    from PIL import Image

    def page(im):
        if im.mode == "L":
            return np.array(im, dtype=np.uint8)
        if im.mode in ("I;16", "I;16B", "I;16L"):
            return np.ascontiguousarray(np.array(im).astype(np.uint16, copy=False))
        raise ValueError(f"{path} is not a polariser mosaic: PIL mode {im.mode!r} (a mosaic is one channel: 'L' for 8 bits, 'I;16' for 9..16)")
    bracket = getattr(layout, "bracket", None)
    with Image.open(path) as im:
        mode = im.mode
        if bracket is None:
            a = page(im)
        else:
            n = int(getattr(im, "n_frames", 1))
            if n != bracket.pages:
                raise ValueError(f"{path} holds {n} page(s), the layout's bracket has {bracket.pages} exposures {bracket.exposures}")
            pages = []
            for k in range(n):
                im.seek(k)
                if im.mode != mode or (pages and (im.size[1], im.size[0]) != pages[0].shape):
                    raise ValueError(f"{path}: page {k} is {im.size[1]} x {im.size[0]} of PIL mode {im.mode!r}, page 0 is "
                                     f"{pages[0].shape[0]} x {pages[0].shape[1]} of mode {mode!r}: the pages of a bracket are one mosaic")
                pages.append(page(im))
            a = np.stack(pages)
    if (a.dtype == np.uint8) != (layout.bits == 8):
        raise ValueError(f"{path} holds {8 * a.dtype.itemsize}-bit samples (PIL mode {mode!r}), the layout says bits = {layout.bits}")
    cal = getattr(layout, "calibration", None)
    if cal is not None and cal.shape is not None and tuple(a.shape[-2:]) != cal.shape:          # here, where the file still has a name
        raise ValueError(f"{path} is {a.shape[-2]} x {a.shape[-1]}, the layout's calibration tables are {cal.shape[0]} x {cal.shape[1]}")
    return a


def demosaic(mosaic, layout, mode="bilinear", total=False, device=None):
    """The four views (and with `total` their rounded mean) of one mosaic: ops.dofp_views, which develops them when the layout has
    a `develop`.  mosaic: a uint8 / uint16 2-D device
    tensor, or a NumPy array, which is uploaded first (to `device`, default the current one); with a bracketed layout the [n,h,w] pages,
    which ops.dofp_views merges first.  Returns uint8 [ho,wo,3] device
    tensors in ascending polariser angle (layout.angles).  Asynchronous on the current stream."""
    import torch
    from . import ops
    if not isinstance(layout, DofpLayout):
        raise ValueError(f"demosaic: layout must be a polar.DofpLayout, got {layout!r}")
    if isinstance(mosaic, np.ndarray):
        mosaic = _upload_mosaic("demosaic", mosaic, layout, device)
    return ops.dofp_views(mosaic, layout, mode, total)


def _upload_mosaic(who, mosaic, layout, device):
    """A decoded mosaic ([h,w], or the [n,h,w] pages of a bracketed layout) on `device` (default the current one)."""
    import torch
    ndim = 2 if layout.bracket is None else 3
    if mosaic.dtype not in (np.uint8, np.uint16) or mosaic.ndim != ndim:
        raise ValueError(f"{who} takes a {'2-D' if ndim == 2 else '3-D [n,h,w]'} uint8 or uint16 mosaic, got {mosaic.dtype} {mosaic.shape}")
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    return torch.from_numpy(np.ascontiguousarray(mosaic)).to(dev)


def merge_bracket(pages, layout, counts=False, device=None):
    """The merged 16-bit mosaic of one bracketed sample, uint16 [h,w] on the device (ops.dofp_merge: each page calibrated first when the
    layout has a calibration), and with `counts` the tensor of how many photosites have 0 .. 8 valid pages -- counts[0] is what is
    still clipped in every page, which tells whether the bracket goes deep enough.  pages: [n,h,w] as decode_mosaic gives them, or a
    device tensor.  layout.merged is the layout of the result.  Asynchronous on the current stream."""
    from . import ops
    if not isinstance(layout, DofpLayout) or layout.bracket is None:
        raise ValueError(f"merge_bracket: layout must be a polar.DofpLayout with a bracket, got {layout!r}")
    if isinstance(pages, np.ndarray):
        pages = _upload_mosaic("merge_bracket", pages, layout, device)
    return ops.dofp_merge(pages, layout, counts)


def write_bracket(path, pages):
    """One bracketed sample as ONE multi-page TIFF, pages in the given (exposure) order: uint8 pages as mode "L", uint16 as "I;16" --
    what decode_mosaic reads with a bracketed layout, and what scientific camera SDKs write.  pages: [n,h,w] or a list of [h,w]."""
    from PIL import Image
    pages = [np.asarray(a) for a in pages]
    if len(pages) < 2 or any(a.ndim != 2 or a.dtype != pages[0].dtype or a.shape != pages[0].shape for a in pages) or \
            pages[0].dtype not in (np.uint8, np.uint16):
        raise ValueError(f"write_bracket takes two or more uint8 or uint16 [h,w] pages of one size, got "
                         f"{[(str(a.dtype), a.shape) for a in pages]}")
    if Path(path).suffix.lower() not in BRACKET_EXT:
        raise ValueError(f"write_bracket: {path} is not a TIFF name (one of {BRACKET_EXT})")
    ims = [Image.fromarray(np.ascontiguousarray(a)) for a in pages]          # uint8 -> "L", uint16 -> "I;16"
    ims[0].save(path, format="TIFF", save_all=True, append_images=ims[1:])
    return str(path)


def pack_brackets(dirs, out_dir):
    """One directory of single-frame mosaics per exposure (in exposure order; files as decode_mosaic reads them) -> one multi-page
    TIFF per sample in out_dir, named after the sample.  The directories must hold the same file names (by stem): unequal counts or
    names raise ValueError.  Returns the files written."""
    from PIL import Image
    dirs = [str(d) for d in dirs]
    if not 2 <= len(dirs) <= MERGE_MAX:
        raise ValueError(f"pack_brackets takes 2 to {MERGE_MAX} directories, one per exposure, got {len(dirs)}")
    lists = [list_images(d, also=BRACKET_EXT) for d in dirs]
    if any(len(f) != len(lists[0]) for f in lists):
        raise ValueError(f"pack_brackets: the directories hold different numbers of frames: {dict(zip(dirs, (len(f) for f in lists)))}")
    stems = [[Path(p).stem for p in f] for f in lists]
    for d, st in zip(dirs[1:], stems[1:]):
        if st != stems[0]:
            odd = sorted(set(st) ^ set(stems[0]))
            raise ValueError(f"pack_brackets: {d} and {dirs[0]} do not hold the same names (e.g. {odd[:3]})")
    if len(set(stems[0])) != len(stems[0]):
        raise ValueError(f"pack_brackets: {dirs[0]} holds two files of one name")
    os.makedirs(out_dir, exist_ok=True)
    written = []
    for i, stem in enumerate(stems[0]):
        pages = []
        for f in lists:
            with Image.open(f[i]) as im:
                if im.mode not in ("L", "I;16", "I;16B", "I;16L"):
                    raise ValueError(f"{f[i]} is not a polariser mosaic: PIL mode {im.mode!r}")
                pages.append(np.array(im, dtype=np.uint8) if im.mode == "L" else np.array(im).astype(np.uint16, copy=False))
        try:
            written.append(write_bracket(os.path.join(out_dir, stem + ".tif"), pages))
        except ValueError:
            raise ValueError(f"pack_brackets: the frames of sample {stem!r} differ in size or depth: "
                             f"{[(p[i], str(a.dtype), a.shape) for p, a in zip(lists, pages)]}") from None
    return written


def gray_gains(sums):
    """The grey-world gains (Q10, 1024 = 1) of the six sums S_r, S_g, S_b, n_r, n_g, n_b of shm_dofp_wb_gray, by its own integer
    arithmetic: mean_c = (S_c << 8) // n_c (0 for n_c == 0); identity gains if any mean is 0, else min(16383, (max mean << 10) // mean_c)."""
    S, n = [int(x) for x in sums[:3]], [int(x) for x in sums[3:6]]
    mean = [(S[c] << 8) // n[c] if n[c] else 0 for c in range(3)]
    if not all(mean):
        return (1024, 1024, 1024)
    return tuple(min(16383, (max(mean) << 10) // m) for m in mean)


def estimate_white_balance(data_dir, layout, dofp_dir="DOFP", sat=None, device=None):
    """The grey-world balance of a WHOLE capture: the sums of shm_dofp_wb_gray (every complete 4 x 4 period without a sample at or
    above `sat`, black level removed) added over all mosaics of data_dir/dofp_dir and finished on the host.  Returns the (R, G, B)
    triple for DofpDevelop(wb=...), smallest entry 1.  One device round trip per frame: a one-off, not a loader path.  `sat`
    defaults to the layout's development's (its white level), or 2^bits - 1 without one.  A bracketed layout has every sample merged
    first: the sums are those of the merged mosaics, under layout.merged."""
    import torch
    from . import ops
    if not isinstance(layout, DofpLayout):
        raise ValueError(f"estimate_white_balance: layout must be a polar.DofpLayout, got {layout!r}")
    if layout.pattern == "mono":
        raise ValueError("estimate_white_balance needs a Bayer pattern, the layout is 'mono'")
    files = list_images(os.path.join(data_dir, dofp_dir), also=mosaic_extensions(layout))
    if not files:
        raise ValueError(f"estimate_white_balance: no mosaics in {os.path.join(data_dir, dofp_dir)}")
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    total = [0] * 6
    with torch.cuda.device(dev):
        for f in files:
            m = torch.from_numpy(decode_mosaic(f, layout)).to(dev)
            sums, _ = ops.dofp_wb_gray(m, layout, sat)
            total = [a + int(b) for a, b in zip(total, sums.cpu().tolist())]
    gains = gray_gains(total)
    return tuple(g / min(gains) for g in gains)


MASK_OPTIONS = ("threshold", "floor", "open_radius", "dilate_radius")       # the keyword options of specular_mask


def specular_mask(views_u8, angles=None, *, matrix=None, threshold="otsu", floor=16, open_radius=1, dilate_radius=2):
    """Highlight mask of one sample from its four polarised views (csrc/specmask.hip): specular reflection is
    polarised, diffuse reflection is not, so the polarised intensity sqrt(S1^2 + S2^2) -- what diffuse_source="stokes" subtracts --
    marks the highlights without a label.

    views_u8: four contiguous uint8 [h,w,3] device tensors; the Stokes matrix is stokes_matrix(angles) or `matrix` (3x4, e.g.
    REFERENCE_DOP_MATRIX); exactly one of the two.  strength = min(255, int(sqrt(max over channels of S1^2 + S2^2))); the
    threshold is Otsu's on the strength histogram, held at `floor` byte units from below (Otsu splits anything, sensor noise
    included; 16 is 6 % of full scale, a documented default and not a measured constant), or `threshold` itself when it is a number
    in byte units (pixels with strength > floor(threshold) are set).  The thresholded map is opened with a (2 open_radius + 1)^2
    square (isolated noise pixels go) and dilated with a (2 dilate_radius + 1)^2 one (the soft rim of a highlight); taps outside the
    image are skipped.  Radii: open 0..4, dilate 0..8, 0 = identity.

    Returns (mask uint8 [h,w] 0 / 255, strength uint8 [h,w], stats int32 [3] = Otsu's t, the threshold applied, the number of set
    pixels), all on the device, filled asynchronously on the current stream: nothing is read back here."""
    import torch
    from . import ops
    if (angles is None) == (matrix is None):
        raise ValueError("specular_mask needs the polariser angles or a 3x4 Stokes matrix (one of `angles`, `matrix`)")
    coef = stokes_matrix(angles) if matrix is None else matrix
    if isinstance(threshold, str):
        if threshold != "otsu":
            raise ValueError(f"specular_mask: threshold {threshold!r} is not 'otsu' or a number in byte units")
        fixed = None
    else:
        if not 0 <= float(threshold) <= 255:
            raise ValueError(f"specular_mask: threshold {threshold!r} is outside the byte range [0, 255]")
        fixed = int(float(threshold))
    views_u8 = list(views_u8)
    if len(views_u8) != 4:
        raise ValueError(f"specular_mask takes four views, got {len(views_u8)}")
    v0 = views_u8[0]
    if not isinstance(v0, torch.Tensor) or v0.dim() != 3:
        raise ValueError("specular_mask takes four uint8 [h,w,3] device tensors")
    h, w = int(v0.shape[0]), int(v0.shape[1])
    q, tmp, mask = (torch.empty((h, w), dtype=torch.uint8, device=v0.device) for _ in range(3))
    hist = torch.empty(256, dtype=torch.int32, device=v0.device)
    stats = torch.empty(3, dtype=torch.int32, device=v0.device)
    ops.specmask(views_u8, coef, q, hist, tmp, mask, stats, floor, fixed, open_radius, dilate_radius)
    return mask, q, stats


def polar_sample_files(data_dir, subdirs, who, capture="views", dofp=None):
    """The sorted file lists of the first four `subdirs` of `data_dir`, with the refusals of write_estimated_diffuse: four
    directories, equal counts.  capture="dofp": the one list of the first of `subdirs`, which holds a mosaic per sample (a multi-page
    TIFF per sample when the layout `dofp` has a bracket)."""
    if capture == "dofp":
        views = tuple(subdirs)[:1]
        if len(views) != 1:
            raise ValueError(f"{who} needs the mosaic directory as the first of subdirs, got {tuple(subdirs)}")
        return views, [list_images(os.path.join(data_dir, views[0]), also=mosaic_extensions(dofp))]
    views = tuple(subdirs)[:4]
    if len(views) != 4:
        raise ValueError(f"{who} needs four view directories, got {views}")
    files = [list_images(os.path.join(data_dir, s)) for s in views]
    if any(len(f) != len(files[0]) for f in files):
        raise ValueError(f"the four view directories hold different numbers of images: {[len(f) for f in files]}")
    return views, files


def decode_sample(paths, index):
    """The four decoded views of one sample; views of unequal size raise, naming the files."""
    imgs = [_decode(p) for p in paths]
    if any(a.shape != imgs[0].shape for a in imgs):
        raise ValueError(f"the four views of sample {index} differ in size: " + ", ".join(f"{p} {a.shape[0]}x{a.shape[1]}" for p, a in zip(paths, imgs)))
    return imgs


def sample_views(paths, index, dev, capture="views", dofp=None, dofp_demosaic="bilinear"):
    """The four uint8 [h,w,3] device views of one sample: its four files decoded and uploaded (decode_sample), or with
    capture="dofp" its one mosaic decoded once, uploaded once and demosaiced once on the current stream."""
    import torch
    if capture == "dofp":
        with torch.cuda.device(dev):
            return list(demosaic(decode_mosaic(paths[0], dofp), dofp, dofp_demosaic, device=dev))
    return [torch.from_numpy(a).to(dev) for a in decode_sample(paths, index)]


def _view_angles(angles, views, capture, dofp):
    """The polariser angles of the four delivered views: `angles` when given, the layout's for a mosaic, else the directory names'."""
    if angles is not None:
        return angles
    return dofp.angles if capture == "dofp" else angles_from_subdirs(views)


def write_specular_masks(data_dir, out_dir, subdirs=PSD_SUBDIRS, angles=None, name_from=2, device=None, capture="views", dofp=None,
                         dofp_demosaic="bilinear", **mask_options):
    """Materialise the specular mask of every sample as a one-channel PNG (0 / 255) at the sample's own size: the sibling of
    write_estimated_diffuse.  The first four `subdirs` of `data_dir` are listed as the loader lists them; sample i's mask is
    specular_mask of its four views (`angles`, or the angles read from the directory names; `mask_options` = its threshold, floor,
    open_radius and dilate_radius), written to `out_dir` under the stem of view `name_from` -- by default the third view (I90), the
    one whose Y plane train_step feeds SpecSeg.predict, so that train_specseg(specseg_image_dir=<data_dir>/I90,
    specseg_mask_dir=out_dir) pairs them as they are.  `out_dir`/masks.jsonl gets one line per sample: name, t (Otsu's), t_eff
    (applied), fraction (of the frame that is masked) -- samples whose mask is empty or covers most of the frame show there.
    Same refusals as write_estimated_diffuse: four directories, equal counts, equal sizes.  capture="dofp" (with dofp = a DofpLayout
    and dofp_demosaic): the first of `subdirs` holds one polariser mosaic per sample, the four views are its demosaiced planes
    (sample_views), the angles default to the layout's and the mask is named after the mosaic.  Returns the list of PNG files written."""
    import json
    import torch
    from PIL import Image
    bad = sorted(set(mask_options) - set(MASK_OPTIONS))
    if bad:
        raise TypeError(f"write_specular_masks: unknown option(s) {bad}; specular_mask takes {MASK_OPTIONS}")
    if name_from not in (0, 1, 2, 3):
        raise ValueError(f"write_specular_masks: name_from {name_from!r} is not a view index 0..3")
    check_capture(capture, dofp, dofp_demosaic, "write_specular_masks")
    views, files = polar_sample_files(data_dir, subdirs, "write_specular_masks", capture, dofp)
    coef = stokes_matrix(_view_angles(angles, views, capture, dofp))
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    os.makedirs(out_dir, exist_ok=True)
    written, rows = [], []
    for i in range(len(files[0])):
        paths = [f[i] for f in files]
        with torch.cuda.device(dev):
            mask, _, stats = specular_mask(sample_views(paths, i, dev, capture, dofp, dofp_demosaic), matrix=coef, **mask_options)
        m, st = mask.cpu().numpy(), stats.cpu().numpy()
        name = Path(paths[name_from if capture == "views" else 0]).stem
        out = os.path.join(out_dir, name + ".png")
        Image.fromarray(m).save(out)                   # uint8 [h,w]: mode "L"
        written.append(out)
        rows.append(dict(name=name, t=int(st[0]), t_eff=int(st[1]), fraction=int(st[2]) / m.size))
    with open(os.path.join(out_dir, "masks.jsonl"), "w") as f:
        for r in rows:
            f.write(json.dumps(r) + "\n")
    return written


def write_estimated_diffuse(data_dir, out_dir, subdirs=PSD_SUBDIRS, mode="min", angles=None, device=None, capture="views", dofp=None,
                            dofp_demosaic="bilinear"):
    """Materialise the estimated-diffuse image of every sample as a PNG at the sample's own size: the imwrite that
    utils.calculate_estimate_diffuse left commented out.  The first four `subdirs` of `data_dir` are listed as the loader lists
    them; sample i's estimate (mode "min": per pixel and channel the minimum of the four views, the reference's definition;
    "stokes": the fitted minimum, with `angles` or the angles read from the directory names) is computed by shm_polar_views_u8 at
    (ho, wo) = (hin, win), scale 1, no flip, rounded to the nearest byte and written to `out_dir` under the first view's file
    name (with the extension .png).  The result can go to any other tool, or back to PolarDataset as its ED/ directory.
    capture="dofp" (with dofp = a DofpLayout and dofp_demosaic): the first of `subdirs` holds one polariser mosaic per sample, whose
    demosaiced views (sample_views) take the place of the four files; the image is named after the mosaic.
    Returns the list of files written."""
    import torch
    from PIL import Image
    from . import ops
    if mode not in ops.POLAR_MODES:
        raise ValueError(f"write_estimated_diffuse: mode {mode!r} is not 'min' or 'stokes'")
    check_capture(capture, dofp, dofp_demosaic, "write_estimated_diffuse")
    views, files = polar_sample_files(data_dir, subdirs, "write_estimated_diffuse", capture, dofp)
    coef = stokes_matrix(_view_angles(angles, views, capture, dofp)) if mode == "stokes" else None
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    os.makedirs(out_dir, exist_ok=True)
    written = []
    for i in range(len(files[0])):
        paths = [f[i] for f in files]
        srcs = sample_views(paths, i, dev, capture, dofp, dofp_demosaic)
        h, w, _ = srcs[0].shape
        planes = torch.empty((5, h, w, 3), dtype=torch.float32, device=dev)
        ops.polar_views_u8(srcs, list(planes), mode, coef, 1.0, False)
        ed = torch.round(planes[4]).clamp_(0, 255).to(torch.uint8).cpu().numpy()
        out = os.path.join(out_dir, Path(paths[0]).stem + ".png")
        Image.fromarray(ed).save(out)
        written.append(out)
    return written
