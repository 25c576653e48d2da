"""Float64 NumPy restatement of the region metrics (shm_highlight_region_hw / shm_image_metrics_region_hw, include/shmgan_hip.h) and the
case table their tests share.  The region rules compare in float32, as the kernel does, so the expected region is exact; the SSIM map
is oracle.tf_ops_np's ssim before its mean (same window, same rescale_01); Lab and the dE values are metrics_ref's."""
import functools

import numpy as np

from oracle import tf_ops_np as tfn

import metrics_ref as mr

NAMES = tuple(f"{side}_{k}" for side in ("in", "out") for k in ("mse", "psnr", "ssim", "de76", "de94")) + ("n_in", "p_in")
WIN, HALF = 11, 5


# ------------------------------------------------------------------------------------------------- the region rules
def crop(frame, window):
    top, left, h, w = window
    return frame[:, top:top + h, left:left + w]


def region_residual(src, window, target, tau):
    """max_c(src_c - target_c) > tau on the window, float32 throughout; np.max propagates a NaN, which compares false."""
    d = crop(np.asarray(src, np.float32), window) - np.asarray(target, np.float32)
    assert d.dtype == np.float32
    with np.errstate(invalid="ignore"):
        return (np.max(d, axis=-1) > np.float32(tau)).astype(np.uint8)


def region_plane(plane, window, tau):
    with np.errstate(invalid="ignore"):
        return (crop(np.asarray(plane, np.float32), window) > np.float32(tau)).astype(np.uint8)


# ------------------------------------------------------------------------------------------------- the SSIM map
def gauss_1d():
    """The marginal of the oracle's 2-D window: the window is its outer product (test_region_cpu checks that), which lets the map of
    a 520 x 520 image be filtered in 22 passes instead of 121."""
    return tfn.gauss_window(WIN, 1.5, np.float64).sum(axis=0)


def ssim_map(x, y, max_val=5.0, k1=0.01, k2=0.03, separable=True):
    """oracle.tf_ops_np.ssim without its last line: [B,h-10,w-10,3] of luminance * contrast-structure (x, y already rescaled)."""
    n, h, w, c = x.shape
    ho, wo = h - WIN + 1, w - WIN + 1
    c1, c2 = (k1 * max_val) ** 2, (k2 * max_val) ** 2
    win = tfn.gauss_window(WIN, 1.5, np.float64)
    w1 = gauss_1d()

    def filt(z):
        if not separable:
            out = np.zeros((n, ho, wo, c), np.float64)
            for a in range(WIN):
                for b in range(WIN):
                    out += win[a, b] * z[:, a:a + ho, b:b + wo]
            return out
        rows = sum(w1[b] * z[:, :, b:b + wo] for b in range(WIN))
        return sum(w1[a] * rows[:, a:a + ho] for a in range(WIN))

    mx, my = filt(x), filt(y)
    num0, den0 = mx * my * 2.0, mx * mx + my * my
    lum = (num0 + c1) / (den0 + c1)
    cs = (filt(x * y) * 2.0 - num0 + c2) / (filt(x * x + y * y) - den0 + c2)
    return lum * cs


def window_ssim_map(g, t):
    """The map shm_image_metrics_hw averages: rescale_01 over each whole image (g, t: the window's pixels, float64)."""
    return ssim_map(tfn.rescale_01(g), tfn.rescale_01(t))


# ------------------------------------------------------------------------------------------------- the twelve values
def _five(sq, e76, e94, smap, mask, centre, empty=np.nan):
    """{mse, psnr, ssim, de76, de94} of one image over the pixels of `mask` and the SSIM positions of `centre`; an empty set: `empty`."""
    n, p = int(mask.sum()), int(centre.sum())
    mse = sq[mask].sum() / (3.0 * n) if n else empty
    psnr = float(mr.psnr(mse)) if n else empty
    ssim = smap[centre].mean() if p else empty
    return [mse, psnr, ssim, e76[mask].mean() if n else empty, e94[mask].mean() if n else empty]


def region_metrics(g, t, region, smap=None, centre_of=lambda m: m[HALF:m.shape[0] - HALF, HALF:m.shape[1] - HALF], empty=np.nan):
    """g, t [B,h,w,3] (the window's pixels), region [B,h,w] -> [B,12] (NAMES).  smap: window_ssim_map(g, t) when the caller has it.
    centre_of and empty exist for the modelled faults of test_region_cpu."""
    g, t = np.asarray(g, np.float64), np.asarray(t, np.float64)
    smap = window_ssim_map(g, t) if smap is None else smap
    sq = ((g - t) ** 2).sum(axis=-1)
    lg, lt = mr.rgb_to_lab(g), mr.rgb_to_lab(t)
    e76, e94 = mr.delta_e76(lg, lt), mr.delta_e94(lg, lt)
    out = np.empty((g.shape[0], 12))
    for b in range(g.shape[0]):
        m = np.asarray(region[b]) != 0
        c = centre_of(m)
        out[b, 0:5] = _five(sq[b], e76[b], e94[b], smap[b], m, c, empty)
        out[b, 5:10] = _five(sq[b], e76[b], e94[b], smap[b], ~m, ~c, empty)
        out[b, 10], out[b, 11] = m.sum(), c.sum()
    return out


# tolerances of tests/test_metrics_gpu.py::_check for the same arithmetic: (relative, absolute) per metric
TOL = {"mse": (1e-5, 0.0), "psnr": (0.0, 1e-4), "ssim": (0.0, 5e-5), "de76": (1e-4, 0.0), "de94": (1e-4, 0.0)}


def mismatches(got, ref):
    """Where [B,12] `got` misses `ref`: NaN and +inf exactly where the reference has them, the finite values within TOL, the counts
    exact.  Returns a list of (image, name, got, ref); empty when everything agrees."""
    got, ref = np.asarray(got, np.float64).reshape(-1, 12), np.asarray(ref, np.float64).reshape(-1, 12)
    bad = []
    for b in range(ref.shape[0]):
        for j, name in enumerate(NAMES):
            a, r = got[b, j], ref[b, j]
            if j >= 10 or not np.isfinite(r):
                ok = (np.isnan(a) and np.isnan(r)) or a == r
            else:
                rel, ab = TOL[name.split("_")[1]]
                ok = np.isfinite(a) and abs(a - r) <= rel * abs(r) + ab
            if not ok:
                bad.append((b, name, a, r))
    return bad


# ------------------------------------------------------------------------------------------------- the case table
# 11x11: one SSIM position; 26x27: the edge of the 16-output tile (16 x 17 positions); 520x520: past the 256-block cap of the pixel pass
SIZES = [(11, 11), (12, 11), (11, 29), (40, 13), (26, 27), (37, 37), (64, 64), (520, 520)]
# (frame h, frame w, window): windows off the frame's origin, the frame filled with NaN and 1e30 outside them
FRAMES = [(48, 64, (3, 5, 37, 41)), (32, 48, (21, 0, 11, 48)), (40, 40, (0, 29, 40, 11))]
BATCHES = (1, 3)
REGIONS = ("empty", "full", "corner", "centre", "checker", "block16", "left", "bernoulli")


def make_region(name, B, h, w, seed=0):
    """uint8 [B,h,w].  corner: the pixel (0, 0) -- n_in 1, no SSIM position (p_in 0, ssim_in NaN); centre: the pixel (h//2, w//2) -- one
    position; block16: one 16 x 16 block at (2, 4), cut at the window's edge; left: the columns below w//2; bernoulli: p = 0.1 per image."""
    r = np.zeros((B, h, w), np.uint8)
    if name == "full":
        r[:] = 1
    elif name == "corner":
        r[:, 0, 0] = 1
    elif name == "centre":
        r[:, h // 2, w // 2] = 1
    elif name == "checker":
        r[:] = (np.add.outer(np.arange(h), np.arange(w)) % 2 == 0)
    elif name == "block16":
        r[:, 2:18, 4:20] = 1
    elif name == "left":
        r[:, :, :w // 2] = 1
    elif name == "bernoulli":
        r[:] = np.random.default_rng(9000 + seed).random((B, h, w)) < 0.1
    else:
        assert name == "empty", name
    return r


@functools.lru_cache(maxsize=None)
def pair(h, w):
    """The shared data of size h x w: three images g, t (float32, as tests/test_metrics_gpu.py draws them) and their SSIM map.  Computed
    once per size; callers must not write into it."""
    rng = np.random.default_rng(1000 * h + w)
    g = rng.uniform(-0.3, 1.3, (3, h, w, 3)).astype(np.float32)
    t = rng.uniform(-0.3, 1.3, (3, h, w, 3)).astype(np.float32)
    smap = window_ssim_map(g.astype(np.float64), t.astype(np.float64))
    for a in (g, t, smap):
        a.setflags(write=False)
    return g, t, smap


def in_frame(x, fh, fw, window, fill=(np.nan, 1e30)):
    """[B,h,w,C] (or [B,h,w]) placed at `window` of a [B,fh,fw,...] frame whose other pixels alternate between the two fills."""
    top, left, h, w = window
    f = np.empty((x.shape[0], fh, fw) + x.shape[3:], np.float32)
    f[:] = fill[0]
    f[:, ::2, 1::2] = fill[1]
    f[:, 1::2, ::2] = fill[1]
    f[:, top:top + h, left:left + w] = x
    return f


def residual_case(B, fh, fw, window, tau, seed=0):
    """src frame, tight target and tau for the builder: random photos whose differences lie around tau, with, per image, a pixel whose
    largest difference is exactly tau (outside), one an ulp above (inside), one an ulp below (outside), one with a NaN in src (outside, the
    other channels far above tau), one with all three differences NaN-free but only one channel above tau (inside)."""
    top, left, h, w = window
    rng = np.random.default_rng(7000 + seed)
    tau32 = np.float32(tau)
    target = rng.uniform(0.0, 0.9, (B, h, w, 3)).astype(np.float32)
    diff = rng.uniform(-0.1, 0.1, (B, h, w, 3)).astype(np.float32) + tau32
    src = (target + diff).astype(np.float32)
    flat = src.reshape(B, h * w, 3)
    tflat = target.reshape(B, h * w, 3)
    spots = rng.permutation(h * w)[:5]
    for b in range(B):
        tflat[b, spots[:4]] = 0.0                                # src - 0 is src: the difference is the planted value exactly
        flat[b, spots[0]] = (tau32, -1.0, tau32)                                                   # at tau
        flat[b, spots[1]] = (np.nextafter(tau32, np.float32(np.inf)), tau32, 0.0)                  # an ulp above
        flat[b, spots[2]] = (np.nextafter(tau32, np.float32(-np.inf)), -np.inf, tau32 * 0)         # an ulp below
        flat[b, spots[3]] = (np.nan, 10.0, 10.0)                                                   # NaN in src
        flat[b, spots[4]] = tflat[b, spots[4]] + np.float32([-0.5, 0.5, -0.5])                     # one channel above
    return in_frame(src, fh, fw, window), target, float(tau32), spots
