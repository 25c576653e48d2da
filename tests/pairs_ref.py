"""TEST INFRASTRUCTURE ONLY -- NumPy restatement of csrc/augment_pairs.hip (include/shmgan_hip.h states the definitions), written
from the definitions and not from the product code, and the case table tests/test_pairs_cpu.py and tests/test_pairs_gpu.py share.

Built on tests/augment_ref.py: `coords` (the float32 tap positions and weights, part of the definition in both precisions), `lerp`
and `draw` / `order` (the loader's draws).  Added here: the tf.image.rgb_to_yuv matrix, the statistics over all three channels of
the RESAMPLED sample, and the 1/256 floor of the divisor.

As tests/polar_ref.py: every function takes the floating-point type to compute in; float64 is the reference, float32 the same
formula at the device's precision.  The two sums behind the standard deviation are float64 in BOTH (the definition says so: the
device adds float64 values of its float32 Y, U and V); what differs is the precision of the lerp, the matrix and the division.

`compare` is THE comparison of the device tests (the rule of DESIGN.md section 6b as the issue states it for x: the larger of 1e-5
of the reference's max-abs and four times the float32 restatement's own error; for y, whose values lie in [0, 1], polar_ref.bound).
`pair(..., fault=...)` restates four mistakes the kernel could make; test_pairs_cpu.py shows `compare` sees each of them.
"""
import numpy as np

import augment_ref as ar
import polar_ref as pr

# tf.image.rgb_to_yuv: yuv[j] = sum_i rgb[i] * K[i][j], the float32 constants of the kernel
YUV = np.array([[0.299, -0.14714119, 0.61497538],
                [0.587, -0.28886916, -0.51496512],
                [0.114, 0.43601035, -0.10001026]], dtype=np.float32)
BYTE = np.float32(1.0 / 255.0)
FLOOR = 1.0 / 256.0
FAULTS = ("no_uv", "no_floor", "mask_unmirrored", "source_stats")

# ------------------------------------------------------------------------------------------------ the case table
# (hin, win) -> (ho, wo): one full block; upsampling, four blocks; 323 pixels, so the last block is partial; one pixel
SHAPES = [((37, 53), (16, 16)), ((9, 7), (32, 32)), ((40, 24), (17, 19)), ((5, 5), (1, 1))]
VARIANTS = ("identity", "crop", "flip_ud", "flip_lr", "both", "crop_flip_lr")


def edge_crop(hin, win):
    """A fractional crop of a little over half the sides that touches the right and the bottom edge; every number is a multiple of
    0.25, so float32 holds it and origin + extent == size exactly."""
    ch, cw = hin / 2.0 + 0.25, win / 2.0 + 0.25
    return (hin - ch, win - cw, ch, cw)


def variant(name, hin, win):
    """(crop or None, flip_ud, flip_lr) of a named variant."""
    crop = edge_crop(hin, win) if name.startswith("crop") else None
    return crop, name in ("flip_ud", "both"), name in ("flip_lr", "both", "crop_flip_lr")


def images(hin, win, k=0, kind="random"):
    """(uint8 [hin,win,3] image, uint8 [hin,win] mask) of a sample; read-only.  kind: "random"; "const" = an image of the one byte
    2, whose standard deviation over (Y, U, V) = (2/255, ~0, ~0) lies below 1/256, so the floor decides; "zeros" / "ones" = an
    all-0 / all-255 mask under a random image."""
    rng = np.random.default_rng(100000 + 1000 * hin + win + 77 * k)
    img = rng.integers(0, 256, (hin, win, 3)).astype(np.uint8)
    mask = (rng.integers(0, 256, (hin, win)) * (rng.random((hin, win)) < 0.6)).astype(np.uint8)
    if kind == "const":
        img = np.full((hin, win, 3), 2, np.uint8)
    elif kind == "zeros":
        mask = np.zeros((hin, win), np.uint8)
    elif kind == "ones":
        mask = np.full((hin, win), 255, np.uint8)
    else:
        assert kind == "random", kind
    img.setflags(write=False)
    mask.setflags(write=False)
    return img, mask


# ------------------------------------------------------------------------------------------------ the restatement
def rgb_to_yuv(rgb, dtype):
    """[...,3] -> [...,3]: every output channel r * K[0][j] + g * K[1][j] + b * K[2][j], summed left to right in `dtype`."""
    rgb = np.asarray(rgb, dtype=dtype)
    k = YUV.astype(dtype)
    return np.stack([(rgb[..., 0] * k[0, j] + rgb[..., 1] * k[1, j]) + rgb[..., 2] * k[2, j] for j in range(3)], axis=-1).astype(dtype)


def std_scale(values, dtype, floor=True):
    """max(std, 1/256) over ALL of `values`, from the float64 sums of the values and of their squares (variance held at >= 0)."""
    v = np.asarray(values).astype(np.float64).reshape(-1)
    mean = v.sum() / v.size
    var = max((v * v).sum() / v.size - mean * mean, 0.0)
    std = np.sqrt(var)
    if dtype == np.float32:
        std = np.float32(std)
        return max(std, np.float32(FLOOR)) if floor else std
    return max(std, FLOOR) if floor else std


def pair(img_u8, mask_u8, ho, wo, crop=None, flip_ud=False, flip_lr=False, dtype=np.float64, fault=None):
    """(x [ho,wo,1], y [ho,wo,1], scale) of one sample of shm_augment_pairs_u8 in `dtype`.  fault: None, or one of FAULTS -- a
    deliberate MISTAKE: "no_uv" = U and V left out of the statistics, "no_floor" = the divisor without its 1/256 floor,
    "mask_unmirrored" = the mask sampled without the mirrors, "source_stats" = statistics over the whole source image instead of
    the resampled crop."""
    assert fault is None or fault in FAULTS, fault
    hin, win = img_u8.shape[:2]
    cy, cx, ch, cw = (0.0, 0.0, float(hin), float(win)) if crop is None else crop
    yt, xt = ar.coords(ho, hin, cy, ch, flip_ud), ar.coords(wo, win, cx, cw, flip_lr)
    yuv = rgb_to_yuv(ar.lerp(img_u8, yt, xt, dtype) * dtype(BYTE), dtype)
    stats = yuv[..., 0] if fault == "no_uv" else yuv
    if fault == "source_stats":
        stats = rgb_to_yuv(np.asarray(img_u8, dtype=dtype) * dtype(BYTE), dtype)
    scale = std_scale(stats, dtype, floor=fault != "no_floor")
    with np.errstate(divide="ignore", invalid="ignore"):
        x = (yuv[..., 0:1] / dtype(scale)).astype(dtype)
    if fault == "mask_unmirrored":
        yt, xt = ar.coords(ho, hin, cy, ch, False), ar.coords(wo, win, cx, cw, False)
    y = ar.lerp(np.asarray(mask_u8).reshape(hin, win, 1), yt, xt, dtype) * dtype(BYTE)
    return x, y.astype(dtype), float(scale)


def x_bound(ref64, e32):
    """The issue's rule for x: the larger of 1e-5 of the reference's max-abs and four times the float32 restatement's error."""
    return max(1e-5 * float(np.abs(ref64).max()), 4.0 * float(e32))


def compare(got_x, got_y, img_u8, mask_u8, ho, wo, crop=None, flip_ud=False, flip_lr=False, label=""):
    """The device comparison: (ok, text).  got_x / got_y: [ho,wo,1] arrays.  Both must be finite; x within x_bound and y within
    polar_ref.bound of the float64 restatement, each bound from the float32 restatement's own error on these inputs."""
    x64, y64, _ = pair(img_u8, mask_u8, ho, wo, crop, flip_ud, flip_lr, np.float64)
    x32, y32, _ = pair(img_u8, mask_u8, ho, wo, crop, flip_ud, flip_lr, np.float32)
    ex32, ey32 = float(np.abs(x32 - x64).max()), float(np.abs(y32 - y64).max())
    got_x, got_y = np.asarray(got_x, dtype=np.float64).reshape(x64.shape), np.asarray(got_y, dtype=np.float64).reshape(y64.shape)
    finite = bool(np.isfinite(got_x).all() and np.isfinite(got_y).all())
    with np.errstate(invalid="ignore"):
        ex = float(np.nan_to_num(np.abs(got_x - x64), nan=np.inf).max())
        ey = float(np.nan_to_num(np.abs(got_y - y64), nan=np.inf).max())
    bx, by = x_bound(x64, ex32), pr.bound(ey32)
    text = (f"{label}: x error {ex:.3e} (float32 restatement {ex32:.3e}, bound {bx:.3e}), y error {ey:.3e} (float32 restatement "
            f"{ey32:.3e}, bound {by:.3e}), finite {finite}")
    return finite and ex <= bx and ey <= by, text


def plain_numpy_path(img_u8, mask_u8, ho, wo):
    """Today's MaskDataset.tensors() for one sample in float64, without this module's functions: polar_ref.resize of the image, a
    plain rgb-to-yuv matrix product, standardise; polar_ref.resize of the mask."""
    rgb = pr.resize(img_u8, ho, wo, np.float64) * np.float64(BYTE)
    yuv = rgb @ YUV.astype(np.float64)
    std = max(float(yuv.std()), FLOOR)
    mask = pr.resize(np.asarray(mask_u8).reshape(*mask_u8.shape[:2], 1), ho, wo, np.float64) * np.float64(BYTE)
    return yuv[..., 0:1] / std, mask
