"""TEST INFRASTRUCTURE ONLY -- NumPy restatement of csrc/augment.hip (include/shmgan_hip.h states the definitions) and of the
loader's draws (shmgan_amd.data.augment_params, pass_order), written from the definitions and not from the product code.

As tests/polar_ref.py: every function takes the floating-point type to compute in, float64 is the reference, float32 the same
formula at the device's precision, and `polar_ref.bound` turns the float32 restatement's own error into a tolerance.  The tap
positions and weights are part of the definition and stay float32 in both precisions.

The coordinate.  fy = ((sy + 0.5f) * (crop_h / ho) - 0.5f) + crop_y is the expression of shm_resize_bilinear_u8 followed by one
addition, and the kernel must equal that kernel bit for bit at identity parameters.  The compiler contracts the product and the
difference of that expression into ONE fused multiply-add in all three kernels (one rounding; checked in their gfx950 code), so
that is what the weights are.  `coords` restates it: the product of two float32 values is exact in float64, and so is the
difference at image-sized magnitudes, so rounding that difference to float32 is the fused result.  Where the product is itself a
float32 value (crop / output a dyadic ratio) the unfused polar_ref.taps gives the same numbers; test_augment_cpu.py checks that.
"""
import numpy as np

import polar_ref as pr

MIN, STOKES, DIR = 0, 1, 2


def coords(n_out, n_in, origin, extent, flip):
    """lower index, upper index and float32 weight per OUTPUT position of one axis: position o samples at s = n_out-1-o with
    `flip`, else o; f = fma(s + 0.5, extent / n_out, -0.5) + origin; taps clamped to the image [0, n_in-1]."""
    f32 = np.float32
    scale = f32(extent) / f32(n_out)
    s = np.arange(n_out, dtype=np.int64)
    if flip:
        s = n_out - 1 - s
    a = s.astype(f32) + f32(0.5)
    fused = (a.astype(np.float64) * np.float64(scale) - 0.5).astype(f32)
    f = fused + f32(origin)
    fl = np.floor(f)
    lo = np.clip(fl.astype(np.int64), 0, n_in - 1)
    hi = np.clip(np.ceil(f).astype(np.int64), 0, n_in - 1)
    return lo, hi, (f - fl).astype(f32)


def lerp(img, ytaps, xtaps, dtype):
    """polar_ref.resize's interpolation of [H,W,C] at given taps: top + (bot - top) * ly with top = tl + (tr - tl) * lx."""
    img = np.asarray(img, dtype=dtype)
    (y0, y1, ly), (x0, x1, lx) = ytaps, xtaps
    lx = lx.astype(dtype)[None, :, None]
    ly = ly.astype(dtype)[:, None, None]
    top = img[y0][:, x0] + (img[y0][:, x1] - img[y0][:, x0]) * lx
    bot = img[y1][:, x0] + (img[y1][:, x1] - img[y1][:, x0]) * lx
    return (top + (bot - top) * ly).astype(dtype)


def mix_views(views, mix, dtype):
    """v'_i = clamp(((M[i][0] v0 + M[i][1] v1) + M[i][2] v2) + M[i][3] v3, 0, 255) per source pixel (= per tap)."""
    v = [np.asarray(a, dtype=dtype) for a in views]
    m = np.asarray(mix, dtype=np.float32).reshape(4, 4).astype(dtype)
    return [np.clip(((m[i, 0] * v[0] + m[i, 1] * v[1]) + m[i, 2] * v[2]) + m[i, 3] * v[3], dtype(0), dtype(255)) for i in range(4)]


def augment_views(srcs_u8, ho, wo, mode, coef=None, mix=None, crop=None, flip_ud=False, flip_lr=False, scale=1.0 / 255.0, dtype=np.float64,
                  mix_fifth=False):
    """Five [ho,wo,3] planes of shm_augment_views_u8.  srcs_u8: five images (DIR) or four (MIN / STOKES).  mix_fifth=True is a
    deliberate MISTAKE (the fifth plane made from the mixed views): test_augment_cpu.py shows the device comparison would see it."""
    hin, win = srcs_u8[0].shape[:2]
    cy, cx, ch, cw = (0.0, 0.0, float(hin), float(win)) if crop is None else crop
    views = list(srcs_u8[:4])
    mixed = mix_views(views, mix, dtype) if mix is not None else views
    if mode == DIR:
        fifth = srcs_u8[4]
    else:
        fifth = pr.estimate(mixed if mix_fifth else views, mode, coef, dtype)
    yt, xt = coords(ho, hin, cy, ch, flip_ud), coords(wo, win, cx, cw, flip_lr)
    return [lerp(p, yt, xt, dtype) * dtype(np.float32(scale)) for p in mixed + [fifth]]


# ------------------------------------------------------------------------------------------------ the loader's draws
def draw(seed, pass_index, position, hin, win, flip_lr=0.0, flip_ud=0.0, crop_min=1.0):
    """(crop (y, x, h, w), flip_ud, flip_lr, remap) of the sample at `position` in pass `pass_index`: five uniforms of
    default_rng((seed, pass, position)) in the order area, row, column, flip_ud, flip_lr; the crop keeps the aspect with side
    fraction sqrt(area fraction); every crop value is a float32 value and origin + extent <= size holds exactly."""
    u = np.random.default_rng((seed, pass_index, position)).random(5)
    side = np.sqrt(crop_min + (1.0 - crop_min) * u[0])
    out = []
    for size, uo in ((hin, u[1]), (win, u[2])):
        ext = np.float32(min(side * size, size))
        org = np.float32(uo * (size - float(ext)))
        if float(org) + float(ext) > size:
            org = np.nextafter(org, np.float32(0))
        out.append((float(org), float(ext)))
    fud, flr = bool(u[3] < flip_ud), bool(u[4] < flip_lr)
    return (out[0][0], out[1][0], out[0][1], out[1][1]), fud, flr, fud != flr


def order(n, seed, pass_index, shuffle):
    return np.random.default_rng((seed, pass_index)).permutation(n) if shuffle else np.arange(n)


def mirror_angles(angles):
    return [(180.0 - float(t)) % 180.0 for t in angles]


def intensity(s0, s1, s2, theta_deg):
    """I(theta) = 0.5 (S0 + S1 cos 2 theta + S2 sin 2 theta) in float64."""
    t = np.deg2rad(2.0 * float(theta_deg))
    return 0.5 * (s0 + s1 * np.cos(t) + s2 * np.sin(t))
