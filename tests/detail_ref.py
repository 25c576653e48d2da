"""Float64 NumPy restatement of the guided detail transfer (shm_detail_coeffs / shm_detail_apply_u8, include/shmgan_hip.h): the clipped
box mean by brute force, the guided filter's coefficients, the sampler of csrc/bilinear.h with its lerp order (so that non-finite
values spread exactly as on the device), the apply, a float32 version of the coefficient formulas (it sizes the tolerances of the
device tests) and the two synthetic scenes of the feature's quality conditions."""
import numpy as np

R2Y = np.array([[0.299, -0.14714119, 0.61497538],
                [0.587, -0.28886916, -0.51496512],
                [0.114, 0.43601035, -0.10001026]])          # tf.image.rgb_to_yuv: yuv = rgb @ R2Y
Y2R_V_R, Y2R_U_G, Y2R_V_G, Y2R_U_B = 1.13988303, -0.394642334, -0.58062185, 2.03206185      # tf.image.yuv_to_rgb
Y2R_ROW_SUM = 3.1                                           # bounds the largest row sum of |yuv_to_rgb|: 1 + 2.03206185


def box_mean(x, r):
    """Mean of x [H,W] over the part of the (2r+1)^2 window around each pixel that lies inside the plane, divided by that part's own
    count.  Brute force, one window at a time; the dtype of x is kept (float64, or float32 for the tolerance restatement)."""
    x = np.asarray(x)
    H, W = x.shape
    out = np.empty_like(x)
    for y in range(H):
        y0, y1 = max(y - r, 0), min(y + r, H - 1) + 1
        for c in range(W):
            c0, c1 = max(c - r, 0), min(c + r, W - 1) + 1
            win = x[y0:y1, c0:c1]
            out[y, c] = win.sum(dtype=x.dtype) / x.dtype.type(win.size)
    return out


def box_mean_integral(x, r):
    """The same mean from an integral image: an independent formulation (finite inputs only)."""
    x = np.asarray(x, np.float64)
    H, W = x.shape
    S = np.zeros((H + 1, W + 1))
    S[1:, 1:] = x.cumsum(0).cumsum(1)
    y0, y1 = np.maximum(np.arange(H) - r, 0), np.minimum(np.arange(H) + r, H - 1) + 1
    c0, c1 = np.maximum(np.arange(W) - r, 0), np.minimum(np.arange(W) + r, W - 1) + 1
    tot = S[y1][:, c1] - S[y0][:, c1] - S[y1][:, c0] + S[y0][:, c0]
    return tot / ((y1 - y0)[:, None] * (c1 - c0)[None, :])


def coeffs(I, p, r, eps, dtype=np.float64, ref=None):
    """coef [H,W,2] = (box(a), box(b)) of one image, as include/shmgan_hip.h states it: d = p - I; var and cov from I - ref (ref: a
    number near I's mean, here the plane's own mean; both are shift-invariant, and d is not shifted); a = cov / (var + eps);
    b = box(d) - a box(I); a window that holds a NaN or an Inf gives NaN a and b.  dtype float32 runs every operation in float32."""
    t = np.dtype(dtype).type
    I, p = np.asarray(I, dtype), np.asarray(p, dtype)
    d = p - I
    if ref is None:
        m = I.mean(dtype=np.float64)
        ref = m if np.isfinite(m) else 0.0
    ref = t(ref)
    Is = I - ref
    with np.errstate(invalid="ignore", over="ignore"):
        mi, md, mii, mid = box_mean(Is, r), box_mean(d, r), box_mean(Is * Is, r), box_mean(Is * d, r)
        var, cov = mii - mi * mi, mid - mi * md
        a = cov / (var + t(eps))
        a = np.where(np.isfinite(mi + md), a, t(np.nan))
        b = md - a * (mi + ref)
        return np.stack([box_mean(a, r), box_mean(b, r)], axis=-1)


def coeffs_f32(I, p, r, eps):
    """The same formulas with every operation in float32 (inputs as the device holds them)."""
    return coeffs(np.asarray(I, np.float32), np.asarray(p, np.float32), r, np.float32(eps), dtype=np.float32)


def coeff_tolerance(I, p, r, eps, ref64=None):
    """Tolerance of a device coefficient plane on these inputs: 4 x the largest error of the float32 restatement against float64
    (the factor covers another summation order and fused multiply-adds), with a floor of 1e-6 (the restatement can be lucky on a
    35-pixel plane).  Returns (tolerance, the restatement's own largest error)."""
    if ref64 is None:
        ref64 = coeffs(I, p, r, eps)
    got = coeffs_f32(I, p, r, eps).astype(np.float64)
    ok = np.isfinite(ref64)
    err = float(np.abs(got[ok] - ref64[ok]).max()) if ok.any() else 0.0
    return max(4.0 * err, 1e-6), err


def _axis(n_out, n_in):
    """Taps and weight of one axis as csrc/bilinear.h computes them IN FLOAT32: in = (out + 0.5) * scale - 0.5, scale = n_in / n_out
    rounded to float32, the product and the subtraction as the one fused multiply-add hipcc makes of them (the float64 product of two
    float32 numbers is exact, so rounding its difference once is that fma); the weight in - floor(in) is exact."""
    f32 = np.float32
    s = f32(n_in) / f32(n_out)
    f = ((np.arange(n_out, dtype=f32) + f32(0.5)).astype(np.float64) * np.float64(s) - 0.5).astype(f32)
    fl = np.floor(f)
    i0 = np.clip(fl, 0, n_in - 1).astype(np.int64)
    i1 = np.clip(np.ceil(f), 0, n_in - 1).astype(np.int64)
    return i0, i1, (f - fl).astype(np.float64)


def sample(coef, h, w):
    """coef [H,W,C] -> [h,w,C]: the taps of bilinear_taps (coordinates in float32, as the device forms them) and the lerp of
    bilinear_lerp in its order, top = tl + (tr - tl) lx, bot = bl + (br - bl) lx, top + (bot - top) ly, in float64 -- the order
    matters for where a NaN or an Inf goes: a tap with weight 0 still poisons the pixel."""
    c = np.asarray(coef, np.float64)
    y0, y1, ly = _axis(h, c.shape[0])
    x0, x1, lx = _axis(w, c.shape[1])
    lx, ly = lx[None, :, None], ly[:, None, None]
    with np.errstate(invalid="ignore"):
        tl, tr, bl, br = c[y0][:, x0], c[y0][:, x1], c[y1][:, x0], c[y1][:, x1]
        top = tl + (tr - tl) * lx
        bot = bl + (br - bl) * lx
        return top + (bot - top) * ly


def photo_yuv(photo_u8, scale):
    """(y, u, v) = rgb_to_yuv(photo / 255) / scale, [h,w,3] float64."""
    return (np.asarray(photo_u8, np.float64) / 255.0) @ R2Y / float(scale)


def yuv_to_rgb(yuv):
    y, u, v = yuv[..., 0], yuv[..., 1], yuv[..., 2]
    return np.stack([y + Y2R_V_R * v, y + Y2R_U_G * u + Y2R_V_G * v, y + Y2R_U_B * u], axis=-1)


def apply(photo_u8, coef, scale):
    """out [h,w,3] = yuv_to_rgb(y + (a' y + b'), u, v) with (a', b') the sample of coef at the photo's size.  Returns (out, bound
    ingredients (max |y|, max |a'|, max |b'|) over the finite samples)."""
    h, w = photo_u8.shape[:2]
    yuv = photo_yuv(photo_u8, scale)
    ab = sample(coef, h, w)
    with np.errstate(invalid="ignore"):
        yn = yuv[..., 0] + (ab[..., 0] * yuv[..., 0] + ab[..., 1])
        out = yuv_to_rgb(np.stack([yn, yuv[..., 1], yuv[..., 2]], axis=-1))
    fin = np.isfinite(ab)
    amax = float(np.abs(ab[..., 0][fin[..., 0]]).max()) if fin[..., 0].any() else 0.0
    bmax = float(np.abs(ab[..., 1][fin[..., 1]]).max()) if fin[..., 1].any() else 0.0
    return out, (float(np.abs(yuv).max()), amax, bmax)


def apply_tolerance(ymax, amax, bmax):
    """Per-channel bound of the apply's own float32 rounding: about a dozen fp32 operations on values bounded by
    M = max|y| (1 + max|a'|) + max|b'|, so 16 * 2^-24 * 3.1 * M (3.1: the largest row sum of |yuv_to_rgb|)."""
    return 16.0 * 2.0 ** -24 * Y2R_ROW_SUM * (ymax * (1.0 + amax) + bmax)


def resize_bilinear(x, ho, wo):
    """[H,W,C] -> [ho,wo,C]: the loader's and the exporter's resize (tf.image.resize bilinear, half-pixel centres), float64."""
    return sample(x, ho, wo)


# ---------------------------------------------------------------------------------------------------------------------
# The two synthetic scenes of the quality conditions: a textured full-resolution photo with an additive highlight, a model frame
# the loader would resize it to, and an ideal "network" that outputs the low-resolution diffuse Y.

def scene(kind, seed, photo_hw=(192, 256), frame_hw=(64, 64)):
    """kind "smooth" (a gaussian blob) or "hard" (a hard-edged ellipse).  Returns a dict: photo_u8 / diffuse_u8 [h,w,3] (the capture
    and its highlight-free partner), and at the frame: I (the standardised Y fed to the network), p (the ideal network's Y: the
    diffuse frame's Y in the photo's standardisation), scale, cbcr."""
    rng = np.random.default_rng(seed)
    h, w = photo_hw
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    # texture: smooth colour fields plus fine grain the model frame cannot hold
    base = np.stack([0.35 + 0.15 * np.sin(xx / 23.0 + k) * np.cos(yy / 31.0 - k) for k in range(3)], axis=-1)
    grain = 0.04 * rng.standard_normal((h, w, 1)) + 0.02 * rng.standard_normal((h, w, 3))
    stripes = 0.024 * np.sin(xx / 1.7)[..., None]
    diffuse = np.clip(base + grain + stripes, 0.02, 0.65)
    cy, cx = 0.45 * h, 0.55 * w
    if kind == "smooth":
        hl = 0.3 * np.exp(-(((yy - cy) / (0.16 * h)) ** 2 + ((xx - cx) / (0.14 * w)) ** 2))
    elif kind == "hard":
        hl = 0.3 * ((((yy - cy) / (0.2 * h)) ** 2 + ((xx - cx) / (0.17 * w)) ** 2) < 1.0)
    else:
        raise ValueError(kind)
    photo = np.clip(diffuse + hl[..., None], 0.0, 1.0)
    photo_u8 = np.rint(photo * 255.0).astype(np.uint8)
    diffuse_u8 = np.rint(diffuse * 255.0).astype(np.uint8)
    H, W = frame_hw
    frame = resize_bilinear(photo_u8 / 255.0, H, W)
    dframe = resize_bilinear(diffuse_u8 / 255.0, H, W)
    yuv = frame @ R2Y
    scale = max(float(yuv.std()), 1.0 / 256.0)                    # custom_per_image_standardization: std over all three channels
    I = yuv[..., 0] / scale
    p = (dframe @ R2Y)[..., 0] / scale
    return {"photo_u8": photo_u8, "diffuse_u8": diffuse_u8, "I": I, "p": p, "scale": scale, "cbcr": yuv[..., 1:] / scale}


def scene_mses(sc, eps=1e-2, radii=(1, 2)):
    """MSE against the full-resolution diffuse image, in gen_rgb's units (rgb / scale), of: the bilinear export of the model-size
    gen_rgb ("bilinear", what test mode writes without the feature), the residual transfer ("residual") and the guided fit per
    radius (("guided", r))."""
    h, w = sc["photo_u8"].shape[:2]
    want = yuv_to_rgb(photo_yuv(sc["diffuse_u8"], sc["scale"]))
    gen_rgb = yuv_to_rgb(np.concatenate([sc["p"][..., None], sc["cbcr"]], axis=-1))
    out = {"bilinear": float(((resize_bilinear(gen_rgb, h, w) - want) ** 2).mean())}
    for key, r in [("residual", 0)] + [(("guided", r), r) for r in radii]:
        got, _ = apply(sc["photo_u8"], coeffs(sc["I"], sc["p"], r, eps), sc["scale"])
        out[key] = float(((got - want) ** 2).mean())
    return out
