"""Float64 restatement of shm_ema_update (include/shmgan_hip.h) and of the trainer's decay schedule, with the error bound the GPU
tests hold the kernel to.

The kernel computes, per element and in fp32: om = 1.0f - decay, t = w - ema, ema' = fmaf(om, t, ema).  The restatement is fed the
SAME fp32-rounded om (the only rounding that is not the kernel's own) and does the rest in float64.

Bound of one update on normal inputs with 0 <= om <= 1, u = 2^-24, M = max(|w|, |ema|):
  rounding t = w - ema costs at most u |w - ema| <= 2 u M, and om <= 1 does not enlarge it;
  the single rounding of the fused multiply-add costs at most u |result| <= u M (the result lies between ema and w);
so |got - ref| <= 3 u M, stated as 4 u M: the fourth u is slack for the second-order terms.  Over K updates the map
ema -> ema + om (w - ema) is a contraction in ema (factor 1 - om), so the errors of the steps at most add: K * 4 u M with M the largest
magnitude on the trajectory."""
import numpy as np

U = 2.0 ** -24
DECAYS = (0.1, 0.5, 0.999, 0.9999)                              # the kernel cases
SIZES = (1, 3, 4, 5, 255, 256, 257, 1023, 1025)
OFFSETS = tuple((a, b) for a in range(4) for b in range(4))      # element offsets of ema and w, independently
GUARD = 8                                                        # sentinel floats on both sides of a view
SENTINEL = np.float32(-7.25e11)


def om32(decay):
    """1.0f - decay as the kernel has it: both operands fp32, one fp32 subtraction."""
    return np.float32(1) - np.float32(decay)


def update(ema, w, decay):
    """One shm_ema_update in float64 (ema, w: arrays of fp32 VALUES): ema + om (w - ema); decay == 0 returns w."""
    ema, w = np.asarray(ema, np.float64), np.asarray(w, np.float64)
    if np.float32(decay) == 0:
        return w.copy()
    return ema + np.float64(om32(decay)) * (w - ema)


def bound(ema, w, updates=1):
    """updates * 4 u M elementwise, M = max(|w|, |ema|) (arrays, or the trajectory's largest magnitude as a scalar)."""
    return updates * 4.0 * U * np.maximum(np.abs(np.asarray(w, np.float64)), np.abs(np.asarray(ema, np.float64)))


def decay_at(ema_decay, t, warmup=True):
    """The trainer's schedule: min(ema_decay, (1 + t) / (10 + t)) with warm-up (tf.train.ExponentialMovingAverage's num_updates)."""
    return min(float(ema_decay), (1.0 + t) / (10.0 + t)) if warmup else float(ema_decay)


def trajectory(ema0, ws, ema_decay, warmup=True):
    """The average after len(ws) updates from ema0 (update t uses decay_at(ema_decay, t)), and per element the largest magnitude of
    weight or average met on the way (the M of the K-update bound)."""
    ema = np.asarray(ema0, np.float64).copy()
    big = np.abs(ema)
    for t, w in enumerate(ws):
        ema = update(ema, w, decay_at(ema_decay, t, warmup))
        big = np.maximum(big, np.maximum(np.abs(np.asarray(w, np.float64)), np.abs(ema)))
    return ema, big


def closed_form(ema0, ws, decays):
    """ema_K = prod_k (1 - om_k) ema0 + sum_k om_k prod_{j > k} (1 - om_j) w_k, with the fp32-rounded om of every step."""
    oms = [np.float64(om32(d)) for d in decays]
    out = np.asarray(ema0, np.float64) * np.prod([1.0 - o for o in oms])
    for k, (w, o) in enumerate(zip(ws, oms)):
        out = out + o * np.prod([1.0 - p for p in oms[k + 1:]]) * np.asarray(w, np.float64)
    return out


def values(rng, n):
    """fp32 values of mixed sign and scale (2^-20 .. 2^20), no zeros, denormals or non-finite values."""
    return (rng.standard_normal(n) * np.exp2(rng.integers(-20, 21, n))).astype(np.float32)
