"""Float64 NumPy restatement of the test-mode image exporter (shm_export_u8, include/shmgan_hip.h): tf.image.resize (bilinear,
half-pixel centres, no antialias), the three value maps (rescale_01 of utils.py:190-195, a scale, a clip) and the byte
quantisation rint(clamp(t, 0, 1) * 255) with round half to even."""
import numpy as np


def _axis(n_out, n_in):
    f = (np.arange(n_out, dtype=np.float64) + 0.5) * (n_in / n_out) - 0.5
    fl = np.floor(f)
    i0 = np.maximum(fl, 0).astype(np.int64)
    i1 = np.minimum(np.ceil(f), n_in - 1).astype(np.int64)
    return i0, i1, f - fl


def resize_bilinear(x, ho, wo):
    """[H,W,C] -> [ho,wo,C] in float64, ResizeBilinear with half_pixel_centers."""
    x = np.asarray(x, np.float64)
    y0, y1, ly = _axis(ho, x.shape[0])
    x0, x1, lx = _axis(wo, x.shape[1])
    lx = lx[None, :, None]
    top = x[y0][:, x0] + (x[y0][:, x1] - x[y0][:, x0]) * lx
    bot = x[y1][:, x0] + (x[y1][:, x1] - x[y1][:, x0]) * lx
    return top + (bot - top) * ly[:, None, None]


def rescale_01(x):
    """utils.py:190-195: (x - min) / (max - min) over the whole array, divide_no_nan (a constant array gives 0)."""
    x = np.asarray(x, np.float64)
    lo, hi = x.min(), x.max()
    return np.zeros_like(x) if hi == lo else (x - lo) / (hi - lo)


def quantize(t):
    """(bytes, y): y = clamp(t, 0, 1) * 255 in float64 and its round-half-to-even bytes."""
    y = np.clip(np.asarray(t, np.float64), 0.0, 1.0) * 255.0
    return np.rint(y).astype(np.uint8), y


def export(plane, ho, wo, mode, mul=1.0):
    """One job: plane [S,S,C] (C real channels), mode "rescale" | "scale" | "clip" -> (bytes [ho,wo,C], y before rounding)."""
    x = np.asarray(plane, np.float64)
    S = x.shape[0]
    lo, hi = x.min(), x.max()
    v = x if (ho, wo) == (S, S) else resize_bilinear(x, ho, wo)
    if mode == "rescale":
        t = np.zeros_like(v) if hi == lo else (v - lo) / (hi - lo)
    elif mode == "scale":
        t = v * float(mul)
    elif mode == "clip":
        t = v
    else:
        raise ValueError(mode)
    return quantize(t)


def near_half(y, tol=1e-3):
    """Where y is within tol of a half-integer: there an fp32 computation may round the other way."""
    return np.abs(y - np.floor(y) - 0.5) <= tol
