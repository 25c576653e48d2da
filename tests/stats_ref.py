"""Reference and error bound for the InstanceNorm statistics the convolution epilogues take in ONE pass ("conditioning of the
fused statistics"): per lane `s += v; q = fma(v, v, q)` in fp32 over a short chain, float64 (atomics, slots, finalize) across chains,
var = q / hw - mean^2.  The reference is the two-pass float64 moments of the tensor AS STORED, so no convolution is recomputed.

CHAIN gives, per kernel family, the depth L of the fp32 part: the largest number of fp32 additions any stored value passes through before
the sum is widened to float64.  The classical bound |fl(sum x) - sum x| <= gamma_L * sum |x| holds for ANY order of additions of depth L
(Higham, Accuracy and Stability of Numerical Algorithms, 4.2), so a correct kernel cannot exceed onepass_bound with its family's L.
"""
import numpy as np

U32 = 2.0 ** -24          # unit roundoff of fp32
U64 = 2.0 ** -53
EPS = float(np.float32(1e-6))       # the float the entry points receive (shm_conv2d_in_fwd / shm_in_stats take eps as float)

# |mean| / std of the pre-normalisation activations: the largest value over every InstanceNorm block of the float64 oracle's step at the
# S = 64, F = 16, B = 2 fixture configuration (initial weights).  test_stats_conditioning_cpu.py recomputes it.
R_WORK = 8.0865
RUNGS = (0.0, R_WORK, 4.0, 16.0, 64.0, 256.0)          # bias of channel c = +-RUNGS[c % 6] * sigma_out

# the project's tolerance on fused statistics (test_variants_gpu.py: _check_stats), which must hold for r <= R_WORK
PROJECT_TOL = {"f32": 1e-5, "bf16": 1e-3}


def gamma(k, u=U32):
    k = np.asarray(k, np.float64)
    return k * u / (1.0 - k * u)


def moments64(y):
    """Two-pass float64 (mean, variance) per (sample, channel) of an NHWC tensor as stored (bf16: pass y.float())."""
    a = y.detach().cpu().numpy() if hasattr(y, "detach") else np.asarray(y)
    n, c = a.shape[0], a.shape[-1]
    a = a.reshape(n, -1, c)
    mu = a.mean(1, dtype=np.float64)
    var = np.zeros((n, c))
    for i in range(n):                                   # per sample: bounds the float64 temporary of a large tensor
        d = a[i].astype(np.float64) - mu[i]
        var[i] = (d * d).mean(0)
    return mu, var


def inv_ref(var, eps=EPS):
    return 1.0 / np.sqrt(var + eps)


def onepass_bound(mu, sigma, L, n64=0, eps=EPS):
    """Worst-case error of the one-pass statistics: fp32 sums of depth L, then n64 float64 additions and the float64 finalize.
    Returns (|d mean|, |d var|, |d inv| / inv).  The inv bound is the exact expression: the larger of the changes of 1 / sqrt(var + eps) for
    the variance moving down by |d var| (no further than the finalize kernel's clamp var >= 0) and up by |d var|."""
    mu, sigma = np.abs(np.asarray(mu, np.float64)), np.asarray(sigma, np.float64)
    g1 = gamma(L) + gamma(n64 + 2, U64)                  # + the division by hw
    # + the product v * v (an fma rounds once: within L + 1 either way); L = 0: the float64 product of two floats is exact
    g2 = np.where(np.asarray(L) > 0, gamma(np.asarray(L) + 1), 0.0) + gamma(n64 + 2, U64)
    m2 = mu * mu + sigma * sigma
    # mean |v| <= sqrt(mean v^2) <= |mu| + sigma
    dmean = g1 * (mu + sigma)
    dvar = g2 * m2 + 2.0 * mu * dmean + dmean * dmean + 3.0 * U64 * m2          # + the float64 subtraction and square
    v = sigma * sigma + eps
    down = np.minimum(dvar, sigma * sigma)               # the clamp: the device's variance is never below 0
    dinv = np.maximum(np.sqrt(v / (v - down)) - 1.0, 1.0 - np.sqrt(v / (v + dvar)))
    return dmean, dvar, dinv


# ---------------------------------------------------------------------------------------------------------------------------------------
# depth of the fp32 part per kernel family.  per = patches a persistent block (ping-pong: a wave group) walks, all of one image in the
# worst case; the persistent kernels widen to float64 only at an image boundary or at the end of their range.

def per_block(npatch, blocks):
    return -(-npatch // blocks)


def pp_per(batch, h, w, cout, ncu):
    """conv_pingpong.hip:517-521, 129: one block per CU and 64-channel slice, two wave groups per block, 8 x 32-pixel patches"""
    npatch = batch * (h // 8) * (w // 32)
    gx = max(1, min(ncu // (cout // 64), (npatch + 1) // 2))
    return per_block(npatch, 2 * gx)


def wreg_per(batch, h, w, cout, ncu):
    """conv_wreg.hip:465-468, 52 and conv_wreg16.hip:291-294, 55: two blocks per CU and 64-channel slice, 8 x 16-pixel patches"""
    np8 = batch * (h // 8) * (w // 16)
    gx = max(1, min(2 * ncu // (-(-cout // 64)), np8))
    return per_block(np8, gx)


def rgb_groups_per_wave(batch, ho, wo, dt):
    """conv_rgb.hip:302-312: runs of 16-pixel groups a wave walks"""
    gpi = ho * (wo // 16)
    gpw = 2 if dt == "f32" else 4
    while gpw < 32 and gpi % (2 * gpw) == 0 and batch * (gpi // (2 * gpw)) >= 4096:
        gpw *= 2
    return gpw


CHAIN = {
    # conv_dma.hip:27, 459-498: a lane adds the 16 * TM rows it owns (TM = BM / WGM / 32), then one shuffle add across the lane halves
    "dma128x128": lambda **k: 33,
    "dma256x128": lambda **k: 33,
    "dma64x64": lambda **k: 17,
    # conv_halo.hip:30 (TM = 2), 395-411 / 545-604: as the DMA tile
    "halo128_st": lambda **k: 33,
    "halo64_st": lambda **k: 33,
    # conv_fwd_x3.hip:284-301: two 32 x 32 tiles of 16 rows per lane and column, one shuffle add
    "x3": lambda **k: 33,
    # conv_wreg.hip:289-305, 415-416, 205-212: 32 values per lane and patch, one add per patch into the lane's running sum, one shuffle add
    "wreg": lambda per, **k: 32 + per + 1,
    # conv_wreg_f32.hip:285-300, 308-309: 16 values per lane and patch; the running sums over patches are float64
    "wreg_f32": lambda **k: 16,
    # conv_wreg16.hip:254-267, 139-148: four K = 32 MFMAs per patch (128 pixels) into ONE fp32 accumulator that lives across the patches
    # of an image; an MFMA's internal order is not documented: counted as 32 sequential additions each
    "wreg16": lambda per, **k: 128 * per,
    # conv_pingpong.hip:386-394 (eight K = 32 MFMAs per 256-pixel patch), 369-376 (one add per patch into the per-lane sums), 208-216
    "pingpong": lambda per, **k: 256 + per,
    # conv_rgb.hip:207-208 / 222-225 (one value per 16-pixel group), 40-46 (four DPP adds)
    "rgb": lambda gpw, **k: gpw + 4,
    # instnorm.hip:10-22: float64 from the first addition
    "in_stats": lambda **k: 0,
    # gsum sums (sum g, sum g * aux): conv_dma.hip:360-395 / conv_halo.hip:500-527 as the statistics;
    "gsum_dma128x128": lambda **k: 33,
    "gsum_halo128_st_f32": lambda **k: 33,
    # tapgemm_dev.h:22-32, 61-69 from conv_halo.hip:443-465: 4 * TM rows per lane, three shuffle adds
    "gsum_halo128_st_bf16": lambda **k: 11,
    # conv_wreg.hip:358-391: four rows per lane and pass, three halving steps and one more shuffle add, then the atomics (per patch)
    "gsum_wreg_bf16": lambda **k: 8,
    # conv_wreg_f32.hip:298-299, 308-309
    "gsum_wreg_f32": lambda **k: 16,
}


# COUNT: an upper limit of how many stored values of one channel a persistent kernel folds into ONE fp32 number before it widens (not the
# depth: a shuffle add is one level of depth and doubles the count).  The worst-case bound cannot see a chain that grows (the typical error
# moves with sqrt(L) and sits far below it); sums that are exactly representable up to a known count can: see exact_planes.
COUNT = {
    # conv_wreg.hip:289-305 (32 values per lane and patch), 415-416 (carried over the patches), 206 (the other lane half)
    "wreg": lambda per, **k: 64 * per,
    # conv_wreg16.hip:254-267: 4 MFMAs x K = 32 pixels per patch on the diagonal of one accumulator, carried over the patches; 141-149: no add at the flush
    "wreg16": lambda per, **k: 128 * per,
    # conv_pingpong.hip:386-394 (8 MFMAs x K = 32), 369-376 (folded into one float per lane, carried over the patches), 208-216
    "pingpong": lambda per, **k: 256 * per,
    # conv_wreg_f32.hip:292-309: 16 values per lane and patch, then float64
    "wreg_f32": lambda **k: 16,
}

EXACT_SMALL = 2.0 ** -4          # the odd pixel of every 8 x 16 patch
EXACT_BIG = np.arange(4, 20)     # the value V of every other pixel, plane c: EXACT_BIG[c % 16]


def exact_planes(n, h, w, cout=64):
    """Planes whose one-pass sums are EXACT up to a known count.  Plane c holds V = EXACT_BIG[c % 16] (sign alternating with c // 16) except
    for one pixel per 8 x 16 patch, which holds 2^-4: all of them bf16 numbers.  Every v * v is a multiple of 2^-8 and at most V^2, so any
    partial result of an fp32 sum over at most k stored values -- in any order, by fma or on the matrix pipe -- is a multiple of 2^-8 no
    larger than k V^2: an fp32 number while k V^2 <= 2^16.  Nothing rounds (the sums of v are further away still), the device's float64
    finalize sees the exact sums and (mean, inv) agree with the two-pass reference to the float64 roundoff.  A count past 2^16 / V^2 needs a
    25th bit as soon as the sum carries an odd number of the small squares.  Returns (y [n, h, w, cout] float32, V [cout])."""
    c = np.arange(cout)
    big = EXACT_BIG[c % len(EXACT_BIG)].astype(np.float32)
    y = np.empty((n, h, w, cout), np.float32)
    y[:] = big * np.where((c // len(EXACT_BIG)) % 2 == 0, 1.0, -1.0).astype(np.float32)
    y[:, ::8, ::16, :] = EXACT_SMALL
    return y, big


def exact_up_to(big):
    """the largest count of stored values of a plane of exact_planes whose fp32 sum of squares cannot round"""
    return (1 << 16) // (np.asarray(big, np.int64) ** 2)


# ---------------------------------------------------------------------------------------------------------------------------------------
# the design in numpy: chains of L sequential fp32 additions, float64 across chains (test_stats_conditioning_cpu.py)

def emulate_onepass(y, L, eps=EPS):
    """y: float32 [hw, c] (the stored values).  Returns (mean, var, inv) per channel as the design computes them."""
    y = np.ascontiguousarray(y, np.float32)
    hw, c = y.shape
    if L <= 0:
        s, q = y.sum(0, dtype=np.float64), (y.astype(np.float64) ** 2).sum(0)
    else:
        nch = -(-hw // L)
        pad = np.zeros((nch * L, c), np.float32)
        pad[:hw] = y
        v = pad.reshape(nch, L, c)
        s1 = np.zeros((nch, c), np.float32)
        s2 = np.zeros((nch, c), np.float32)
        for i in range(L):
            vi = v[:, i]
            s1 = s1 + vi                                                      # float32 + float32 rounds to float32
            s2 = (vi.astype(np.float64) * vi + s2).astype(np.float32)         # fma: the float64 product of two floats is exact
        s, q = s1.sum(0, dtype=np.float64), s2.sum(0, dtype=np.float64)
    mean = s / hw
    var = np.maximum(q / hw - mean * mean, 0.0)
    return mean, var, 1.0 / np.sqrt(var + eps)


def ladder_bias(cout, sigma_out):
    """bias of channel c: +-RUNGS[c % 6] * sigma_out, alternating sign; rung index per channel"""
    c = np.arange(cout)
    rung = c % len(RUNGS)
    sign = np.where((c // len(RUNGS)) % 2 == 0, 1.0, -1.0)
    return (sign * np.asarray(RUNGS)[rung] * sigma_out).astype(np.float32), rung
