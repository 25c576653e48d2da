"""NumPy restatement of shm_tensor_stats (include/shmgan_hip.h): per-segment statistics and the sign / exponent histogram of
a flat float32 buffer.  The classes are read from the bits of v = x * scale (one float32 multiply) through view(np.uint32),
never from a logarithm; sums are float64."""
import numpy as np

BINS = 44                  # SHM_THIST_BINS
EMIN = -40                 # SHM_THIST_EMIN
NSTAT = 8                  # SHM_TSTAT_N: finite, nan, inf, min, max, sum, sumsq, clipped
CLS_ONE, CLS_NONFINITE = 42, 43


def scaled(x, scale):
    return (np.asarray(x, dtype=np.float32) * np.float32(scale)).astype(np.float32)


def classify(v):
    """(sign, class) of every float32 value of v."""
    u = np.ascontiguousarray(v, dtype=np.float32).view(np.uint32)
    E = ((u >> np.uint32(23)) & np.uint32(0xFF)).astype(np.int64)
    sign = (u >> np.uint32(31)).astype(np.int64)
    cls = np.clip(E - 127 - EMIN + 2, 1, CLS_ONE)          # normal values: floor(log2|v|) - EMIN + 2, clamped to [1, 42]
    cls = np.where(E == 0, 0, cls)
    cls = np.where(E == 255, CLS_NONFINITE, cls)
    sign = np.where((E == 0) | (E == 255), 0, sign)
    return sign, cls


def segment_stats(x, scale=1.0):
    """(stats float64 [8], hist int64 [2, 44]) of one segment."""
    v = scaled(x, scale)
    sign, cls = classify(v)
    hist = np.bincount((sign * BINS + cls).ravel(), minlength=2 * BINS).astype(np.int64).reshape(2, BINS)
    finite = np.isfinite(v)
    f = v[finite].astype(np.float64)
    stats = np.zeros(NSTAT, dtype=np.float64)
    stats[0] = f.size
    stats[1] = np.count_nonzero(np.isnan(v))
    stats[2] = np.count_nonzero(np.isinf(v))
    if f.size:
        stats[3], stats[4] = f.min(), f.max()
    stats[5] = f.sum()
    stats[6] = (f * f).sum()
    stats[7] = np.count_nonzero(np.abs(f) > 1.0)
    return stats, hist


def tensor_stats(x, offsets, sizes, scale=1.0):
    """(stats [nseg, 8], hist [nseg, 2, 44]) of the segments x[offsets[s] : offsets[s] + sizes[s]]."""
    res = [segment_stats(x[o:o + z], scale) for o, z in zip(offsets, sizes)]
    return np.stack([r[0] for r in res]), np.stack([r[1] for r in res])


def sum_bounds(x, scale=1.0):
    """Bounds on |sum - exact| and |sumsq - exact| of a float64 summation of the segment in ANY order: n * 2^-53 * sum|v| and
    n * 2^-53 * sum v^2 (Higham, Accuracy and Stability of Numerical Algorithms, section 4.2; v^2 is exact in float64)."""
    v = scaled(x, scale)
    f = v[np.isfinite(v)].astype(np.float64)
    u = 2.0 ** -53
    return f.size * u * np.abs(f).sum(), f.size * u * (f * f).sum()
