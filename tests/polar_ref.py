"""TEST INFRASTRUCTURE ONLY -- NumPy restatement of csrc/polar.hip (include/shmgan_hip.h states the definitions).

Every function takes the floating-point type to compute in: float64 is the reference the device is held to, float32 the same
formula at the device's precision.  The error of the float32 restatement against float64 on the SAME inputs measures what fp32
arithmetic costs for that formula and those inputs; `bound` turns it into the tolerance of a device check (the issue's rule: the
larger of 2e-6 and four times that error -- the factor covers another legal operation order and FMA contraction).

What is NOT redone in float64: the tap positions and the interpolation weights.  They are part of the definition (a float32
computation, as in tf.image.resize and oracle.data_np.resize_bilinear: which two rows a pixel reads is a discrete choice), so both
precisions use the same float32 weights, converted exactly.
"""
import numpy as np

MIN, STOKES = 0, 1


def taps(n_out, n_in):
    """lower index, upper index and float32 weight per output position: half-pixel centres, as oracle.data_np.resize_bilinear."""
    scale = np.float32(n_in) / np.float32(n_out)
    f = (np.arange(n_out, dtype=np.float32) + np.float32(0.5)) * scale - np.float32(0.5)
    fl = np.floor(f)
    lo = np.maximum(fl.astype(np.int64), 0)
    hi = np.minimum(np.ceil(f).astype(np.int64), n_in - 1)
    return lo, hi, (f - fl).astype(np.float32)


def resize(img, ho, wo, dtype):
    """[H,W,C] -> [ho,wo,C] in `dtype`: top + (bot - top) * ly with top = tl + (tr - tl) * lx."""
    img = np.asarray(img, dtype=dtype)
    y0, y1, ly = taps(ho, img.shape[0])
    x0, x1, lx = taps(wo, img.shape[1])
    lx = lx.astype(dtype)[None, :, None]
    ly = ly.astype(dtype)[:, None, None]
    top = img[y0][:, x0] + (img[y0][:, x1] - img[y0][:, x0]) * lx
    bot = img[y1][:, x0] + (img[y1][:, x1] - img[y1][:, x0]) * lx
    return (top + (bot - top) * ly).astype(dtype)


def stokes(views, coef, dtype):
    """(S0, S1, S2) = coef . views, the four products of a row summed left to right in `dtype`."""
    v = [np.asarray(a, dtype=dtype) for a in views]
    c = np.asarray(coef, dtype=np.float32).reshape(3, 4).astype(dtype)
    return [((c[r, 0] * v[0] + c[r, 1] * v[1]) + c[r, 2] * v[2]) + c[r, 3] * v[3] for r in range(3)]


def estimate_raw(views, mode, coef=None, dtype=np.float64):
    """The per-pixel diffuse estimate at source resolution BEFORE the clamp (MIN has none)."""
    if mode == MIN:
        return np.minimum.reduce([np.asarray(a, dtype=dtype) for a in views])
    s0, s1, s2 = stokes(views, coef, dtype)
    return dtype(0.5) * (s0 - np.sqrt(s1 * s1 + s2 * s2))


def estimate(views, mode, coef=None, dtype=np.float64):
    e = estimate_raw(views, mode, coef, dtype)
    return e if mode == MIN else np.clip(e, dtype(0), dtype(255))


def polar_views(views_u8, ho, wo, mode, coef=None, scale=1.0 / 255.0, flip_ud=False, dtype=np.float64):
    """Five [ho,wo,3] planes: the four resized views and the resized estimate (estimate first, at source size, then resize)."""
    planes = [resize(a, ho, wo, dtype) for a in views_u8] + [resize(estimate(views_u8, mode, coef, dtype), ho, wo, dtype)]
    planes = [p * dtype(np.float32(scale)) for p in planes]
    return [p[::-1].copy() if flip_ud else p for p in planes]


def polar_maps(views, coef, dtype=np.float64):
    """(s0, dop, aolp) of shm_polar_maps."""
    s0, s1, s2 = stokes(views, coef, dtype)
    p = np.sqrt(s1 * s1 + s2 * s2)
    dop = np.divide(p, s0, out=np.zeros_like(p), where=s0 != 0)
    return s0, dop, dtype(0.5) * np.arctan2(s2, s1)


def circ_dist(a, b):
    """Distance of two angles modulo pi (an angle of linear polarisation is a direction, not a vector)."""
    d = np.mod(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)), np.pi)
    return np.minimum(d, np.pi - d)


def bound(err32):
    """Tolerance of a device check from the float32 restatement's own maximum error against float64."""
    return max(2e-6, 4.0 * float(err32))
