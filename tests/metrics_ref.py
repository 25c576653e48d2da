"""Float64 NumPy restatement of the test-mode image metrics (the reference's test.py:332-392): tfio's rgb_to_lab, skimage's
deltaE_cie76 / deltaE_ciede94, tf.image.psnr and Keras' MeanSquaredError.  Neither tfio nor skimage is installed, so the constants
are restated from their definitions (include/shmgan_hip.h, shm_image_metrics); SSIM comes from oracle.tf_ops_np."""
import numpy as np

from oracle import tf_ops_np as tfn

_M = np.array([[0.412453, 0.357580, 0.180423],
               [0.212671, 0.715160, 0.072169],
               [0.019334, 0.119193, 0.950227]])
_WHITE = np.array([0.95047, 1.0, 1.08883])


def rgb_to_lab(rgb):
    """tfio.experimental.color.rgb_to_lab (D65, 2 degree observer) on [..., 3]; np.where on both branches, as tf.where."""
    x = np.asarray(rgb, np.float64)
    with np.errstate(invalid="ignore"):
        lin = np.where(x > 0.04045, ((x + 0.055) / 1.055) ** 2.4, x / 12.92)
    xyz = lin @ _M.T / _WHITE
    f = np.where(xyz > 0.008856, np.cbrt(xyz), 7.787 * xyz + 16.0 / 116.0)
    L = 116.0 * f[..., 1] - 16.0
    a = 500.0 * (f[..., 0] - f[..., 1])
    b = 200.0 * (f[..., 1] - f[..., 2])
    return np.stack([L, a, b], axis=-1)


def delta_e76(lab1, lab2):
    return np.sqrt(((lab1 - lab2) ** 2).sum(axis=-1))


def delta_e94(lab1, lab2, k1=0.045, k2=0.015):
    """skimage deltaE_ciede94 (kL = kC = kH = 1): C1 is lab1's, so the metric is not symmetric."""
    L1, a1, b1 = np.moveaxis(lab1, -1, 0)
    L2, a2, b2 = np.moveaxis(lab2, -1, 0)
    C1, C2 = np.hypot(a1, b1), np.hypot(a2, b2)
    dH2 = 2.0 * (C1 * C2 - a1 * a2 - b1 * b2)
    e2 = (L1 - L2) ** 2 + ((C1 - C2) / (1.0 + k1 * C1)) ** 2 + dH2 / (1.0 + k2 * C1) ** 2
    return np.sqrt(np.maximum(e2, 0.0))


def psnr(mse):
    mse = np.asarray(mse, np.float64)
    with np.errstate(divide="ignore"):
        return np.where(mse == 0.0, np.inf, -10.0 * np.log10(np.where(mse == 0.0, 1.0, mse)))


def image_metrics(g, t):
    """[B,S,S,3] x 2 -> [B,5] {mse, psnr, ssim, de76, de94}, every image on its own."""
    g = np.asarray(g, np.float64)
    t = np.asarray(t, np.float64)
    mse = ((g - t) ** 2).mean(axis=(1, 2, 3))
    ssim = tfn.ssim(tfn.rescale_01(g), tfn.rescale_01(t), 5.0)
    lg, lt = rgb_to_lab(g), rgb_to_lab(t)
    e76 = delta_e76(lg, lt).mean(axis=(1, 2))
    e94 = delta_e94(lg, lt).mean(axis=(1, 2))
    return np.stack([mse, psnr(mse), ssim, e76, e94], axis=1)
