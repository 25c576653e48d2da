"""Case tables and float64 NumPy references for the small kernels around the convolutions -- the one-channel heads, PatchGAN logits and
Dense(5) (csrc/heads.hip), lrelu_bwd_kernel (csrc/grad_sums.hip), the SpecSeg passes (csrc/specseg.hip) and the casts (csrc/elem.hip) -- at the
shapes where they take another path than on test_ops_gpu.py's friendly ones: one lane or a whole wave per pixel, a ragged last wave, pitches
wider than the channel count, NULL options, grid-stride loops behind a block cap that iterate and end ragged, more than 16 samples in the patch
weight gradient, Dense's scalar fallback.  test_heads_edges_cpu.py proves on the CPU that every case is in the branch it claims and that the
comparison has teeth; test_heads_edges_gpu.py runs the kernels.

The references are written from the contracts in include/shmgan_hip.h and the SHM.py lines they cite, not from the kernels.  Every function
takes `dtype` (float64: the reference; float32: the same arithmetic in single precision, the noise floor the bounds are held against).
Inputs are float64 arrays holding float32 (or bf16) VALUES, so the device and the reference see the same numbers; the backward references
take the LeakyReLU mask from the `y` array handed to the kernel (y > 0, oracle/tf_ops_np.leaky_relu_grad).
"""
from types import SimpleNamespace

import numpy as np
import torch

from loss_edge_ref import GUARD_ROWS, SENT_BYTE, guard_intact, guarded, r32, t64          # noqa: F401  (re-exported for the tests)
from oracle import specseg_torch as sp
from oracle import tf_ops_np as tn
from util import rel_l2

F32_TOL = 1e-5          # TOL of test_ops_gpu.py: fp32 results of fp32 operands
BF16_TOL32 = 1e-4       # TOL32 of test_bf16_gpu.py: fp32 / f64 results of bf16 operands
BF16_TOL = 4e-3         # TOL of test_bf16_gpu.py: bf16-stored results
SLOPE = float(np.float32(0.2))          # the slope reaches every kernel as a float
DTYPES = ("f32", "bf16", "gf32")        # SHM_F32, SHM_BF16, SHM_BF16_GF32 (bf16 activations, fp32 [G] tensors)


def rb(a):
    """float64 array of the bf16 roundings of a"""
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(torch.bfloat16).double().numpy()


def act(a, dt):
    """a as the values an activation tensor of the call's dtype holds"""
    return r32(a) if dt == "f32" else rb(a)


def grad(a, dt):
    """a as the values a [G] tensor of the call's dtype holds"""
    return rb(a) if dt == "bf16" else r32(a)


def gtol(dt):
    """bound on a [G] result"""
    return {"f32": F32_TOL, "bf16": BF16_TOL, "gf32": BF16_TOL32}[dt]


def ftol(dt):
    """bound on an fp32 / f64 result"""
    return F32_TOL if dt == "f32" else BF16_TOL32


def err(got, ref):
    """The figure every comparison of test_heads_edges_gpu.py bounds: rel-L2 over the elements that are finite in the reference -- and
    infinity unless NaN sits exactly where the reference has NaN, +-Inf where it has +-Inf, and everything else is finite."""
    ref = np.asarray(ref, np.float64)
    got = np.asarray(got, np.float64).reshape(ref.shape)
    fin, inf = np.isfinite(ref), np.isinf(ref)
    if not (np.array_equal(np.isnan(got), np.isnan(ref)) and np.array_equal(got[inf], ref[inf]) and np.isfinite(got[fin]).all()):
        return float("inf")
    return rel_l2(got[fin], ref[fin]) if fin.any() else 0.0


def _lrelu(z, slope):
    return np.where(z > 0, z, slope * z)


def _colsum(a):
    """sum over every axis but the last, along contiguous memory (NumPy's pairwise summation, so that a float32 evaluation is not a naive
    running sum over 10^5 rows)"""
    return np.ascontiguousarray(a.reshape(-1, a.shape[-1]).T).sum(-1)


# ---------------------------------------------------------------------------------------------------------------------------------------
# generator head, plain and with InstanceNorm folded in, and SpecSeg's sigmoid head (the same lane mapping)

HEAD_C = (4, 8, 64, 256)
HEAD_FWD_CAP = 8192          # heads.hip shm_head_fwd / shm_head_in_fwd, specseg.hip shm_head_sigmoid_fwd: "shm_grid_cap(npix, ..., 8192)", "8192 / batch"
HEAD_BWD_CAP = 4096          # heads.hip shm_head_bwd / shm_head_in_bwd: "shm_grid_cap(npix, ..., 4096)", "4096 / batch"
HEAD_BWD_ITERS = 8           # the same two: blocks = cdiv(npix, PP * 8)
HEAD_BWD_U = 4               # heads.hip head_bwd_kernel: "constexpr int U = 4"
HEAD_IN_BATCH = 3
HEAD_OVER_C = 256
HEAD_FWD_OVER = HEAD_FWD_CAP * 4 + 5                                  # c = 256: PP = 4
HEAD_BWD_OVER = HEAD_BWD_CAP * 4 * HEAD_BWD_ITERS + 5
HEAD_IN_FWD_OVER_HW = 10925                                           # x 3 samples = 32775
HEAD_IN_BWD_OVER_HW = 43693                                           # x 3 samples = 131079


def lanes(c):
    return c // 4                # elem.h PixMap, heads.hip head_fwd_kernel: "lanes_c = c >> 2"


def pp(c):
    return 256 // lanes(c)       # the same: "PP = 256 / lanes_c" pixels per block iteration


def pix_per_wave(c):
    return max(64 // lanes(c), 1)


def head_npix(c):
    """1; PP - 1; PP + 1 (a second block forward, a second trip of the backward's tail loop); 5 PP + 3: the backward's U = 4 main loop runs
    once and its tail loop twice, the last trip with three pixels -- no multiple of the pixels per wave where a wave holds several.  All odd."""
    P = pp(c)
    return (1, P - 1, P + 1, 5 * P + 3)


def head_grid(npix, c, batch=1, bwd=False):
    """blocks in x of the launch, as the entry points choose them"""
    per = pp(c) * (HEAD_BWD_ITERS if bwd else 1)
    cap = max((HEAD_BWD_CAP if bwd else HEAD_FWD_CAP) // batch, 1)
    return min(max(-(-npix // per), 1), cap)


def head_trips(npix, c, batch=1, bwd=False):
    """(trips of the main loop, trips of the tail loop) of the thread that makes most of them: pixel slot 0 of block 0.  Forward: one
    grid-stride loop, counted as the tail."""
    stride = head_grid(npix, c, batch, bwd) * pp(c)
    p, main = 0, 0
    if bwd:
        while p + (HEAD_BWD_U - 1) * stride < npix:
            p, main = p + HEAD_BWD_U * stride, main + 1
    return main, len(range(p, npix, stride))


def head_case(c, npix, dt, batch=1, seed=0):
    """x [batch * npix, c] in the activation dtype, w [c], bias, dy [batch * npix] (mean 0.5: the sums do not cancel), and for the folded
    form statistics (mean, inv) [batch, c] as float32 values (the kernel reads the doubles as floats) and beta [c]"""
    rng = np.random.default_rng(7000 + 13 * c + npix % 9973 + 101 * batch + seed)
    n = batch * npix
    k = SimpleNamespace(c=c, npix=npix, batch=batch, dt=dt)
    k.x = act(rng.standard_normal((n, c), dtype=np.float32), dt)
    k.w = r32(rng.standard_normal(c) / np.sqrt(c))
    k.b = float(np.float32(0.3))
    k.dy = r32(rng.standard_normal(n) + 0.5)
    k.mean = r32(rng.standard_normal((batch, c)) * 0.1 + 0.3)
    k.inv = r32(rng.uniform(0.5, 2.0, (batch, c)))
    k.beta = r32(rng.standard_normal(c) * 0.02)
    return k


def head_norm(x, mean, inv, beta, dtype=np.float64):
    """InstanceNorm apply of the block in front of the head: (a - mean) * inv + beta per (sample, channel)"""
    b, c = mean.shape
    a = x.astype(dtype).reshape(b, -1, c)
    return ((a - mean.astype(dtype)[:, None]) * inv.astype(dtype)[:, None] + beta.astype(dtype)).reshape(-1, c)


def head_fwd_ref(x, w, b, slope=SLOPE, dtype=np.float64):
    """Conv2D(1, k=1) + LeakyReLU (SHM.py:326); b = None: no bias"""
    z = (x.astype(dtype) * w.astype(dtype)).sum(-1) + dtype(0.0 if b is None else b)
    return _lrelu(z, dtype(slope))


def head_bwd_ref(x, w, y, dy, slope=SLOPE, dtype=np.float64):
    """(dz, dx, dw, db): dz = dy * lrelu'(y), dx = dz (x) w, dw = sum x dz, db = sum dz"""
    dz = tn.leaky_relu_grad(y.astype(dtype), dy.astype(dtype), dtype(slope))
    return dz, dz[:, None] * w.astype(dtype)[None, :], _colsum(x.astype(dtype) * dz[:, None]), dz.sum()


def sigmoid_head_ref(x, w, b, dtype=np.float64):
    """Conv2D(1, (1, 1), activation='sigmoid') (SpecSeg.py:88)"""
    with np.errstate(over="ignore"):
        return dtype(1.0) / (dtype(1.0) + np.exp(-((x.astype(dtype) * w.astype(dtype)).sum(-1) + dtype(0.0 if b is None else b))))


def saturate_rows(k, logit=100.0):
    """every row of k.x becomes +-logit * w / |w|^2 (alternating): x . w = +-logit up to rounding"""
    sign = np.where(np.arange(k.x.shape[0]) % 2 == 0, 1.0, -1.0)
    k.x = r32(sign[:, None] * logit * k.w[None, :] / (k.w ** 2).sum())
    return k


# ---------------------------------------------------------------------------------------------------------------------------------------
# PatchGAN logits: Conv2D(1, k=3, no bias) + LeakyReLU (SHM.py:365-369)

PATCH_SAMPLE_STRIDE = 16          # heads.hip patch_dw_kernel: "for (int n = g; n < batch; n += 16)"
PATCH_CH_PER_BLOCK = 64           # the same kernel: "ch = blockIdx.y * 64 + ...", grid.y = cdiv(c, 64)
PATCH_BATCHES = (1, 17, 33)
PATCH_C = (4, 68, 256)
PATCH_CASES = tuple((b, 2, 3, c) for b in PATCH_BATCHES for c in PATCH_C) + ((2, 1, 5, 68), (2, 5, 1, 68), (1, 1, 1, 4))


def patch_case(batch, h, w, c, dt, seed=0):
    rng = np.random.default_rng(8000 + 7 * batch + 31 * h + 3 * w + c + seed)
    k = SimpleNamespace(batch=batch, h=h, w=w, c=c, dt=dt)
    k.x = act(rng.standard_normal((batch, h, w, c)), dt)
    k.wt = r32(rng.standard_normal((9, c)) / np.sqrt(9 * c))
    k.dy = r32(rng.standard_normal((batch, h, w)) + 0.5)
    return k


def _taps(h, w):
    """per tap: (tap, output rows, output columns, input rows, input columns) of the pixels the tap connects -- windows, not zero padding:
    a product with a pixel outside the map does not exist (so 0 * Inf never arises)"""
    for tap in range(9):
        dh, dw = tap // 3 - 1, tap % 3 - 1
        i0, i1, j0, j1 = max(0, -dh), min(h, h - dh), max(0, -dw), min(w, w - dw)
        yield tap, slice(i0, i1), slice(j0, j1), slice(i0 + dh, i1 + dh), slice(j0 + dw, j1 + dw)


def patch_fwd_ref(x, wt, slope=SLOPE, dtype=np.float64):
    x, wt = x.astype(dtype), wt.astype(dtype)
    z = np.zeros(x.shape[:3], dtype)
    for tap, oi, oj, ii, ij in _taps(x.shape[1], x.shape[2]):
        z[:, oi, oj] += (x[:, ii, ij, :] * wt[tap]).sum(-1)
    return _lrelu(z, dtype(slope))


def patch_bwd_ref(x, wt, y, dy, slope=SLOPE, dtype=np.float64, samples=None):
    """(dz, dx, dw); samples: the samples whose products enter dw (all; the teeth tests pass fewer)"""
    x, wt = x.astype(dtype), wt.astype(dtype)
    dz = tn.leaky_relu_grad(y.astype(dtype), dy.astype(dtype), dtype(slope))
    dx, dw = np.zeros(x.shape, dtype), np.zeros(wt.shape, dtype)
    s = slice(None) if samples is None else samples
    for tap, oi, oj, ii, ij in _taps(x.shape[1], x.shape[2]):
        dx[:, ii, ij, :] += dz[:, oi, oj, None] * wt[tap]
        dw[tap] = _colsum(x[s, ii, ij, :] * dz[s, oi, oj, None])
    return dz, dx, dw


# ---------------------------------------------------------------------------------------------------------------------------------------
# Flatten + Dense(nout, no bias) (SHM.py:371-375)

DENSE_NOUT = (1, 5, 8)
DENSE_K = (3, 1020, 1022, 2052)
DENSE_BATCH = (1, 4, 7)
DENSE_UNROLL = 4                  # heads.hip dense_bwd_kernel: "for (; n + 4 <= batch; n += 4)"
DENSE_LDS_BYTES = 48 * 1024       # heads.hip shm_dense_bwd: "batch * nout * 4 <= 48 * 1024"
DENSE_REFUSED = (1537, 8)         # (batch, nout): 49184 bytes of dy


def dense_fast_path(nout, k, offset, itemsize):
    """heads.hip dense_fwd_kernel: "nout == 5 && (k & 3) == 0 && ((size_t)xr & (4 * sizeof(T) - 1)) == 0" for every row, x starting `offset`
    elements behind an allocation (whose start is aligned far beyond 16 bytes)"""
    return nout == 5 and k % 4 == 0 and (offset * itemsize) % (4 * itemsize) == 0


def dense_case(batch, k, nout, dt, seed=0):
    rng = np.random.default_rng(9000 + 5 * batch + k + 17 * nout + seed)
    d = SimpleNamespace(batch=batch, k=k, nout=nout, dt=dt)
    d.x = act(rng.standard_normal((batch, k)), dt)
    d.w = r32(rng.standard_normal((k, nout)) / np.sqrt(k))
    d.dy = r32(rng.standard_normal((batch, nout)) + 0.5)
    d.dx0 = grad(rng.standard_normal((batch, k)), dt)
    return d


def dense_fwd_ref(x, w, dtype=np.float64):
    return (x.astype(dtype)[:, :, None] * w.astype(dtype)[None]).sum(1)


def dense_bwd_ref(x, w, dy, dx0, dtype=np.float64, accumulate=True):
    """(dx, dw): dx = dx0 + dy w^T (the contract is +=), dw = x^T dy"""
    x, w, dy = x.astype(dtype), w.astype(dtype), dy.astype(dtype)
    s = (dy[:, None, :] * w[None]).sum(-1)
    return (dx0.astype(dtype) + s if accumulate else s), (x[:, :, None] * dy[:, None, :]).sum(0)


# ---------------------------------------------------------------------------------------------------------------------------------------
# LeakyReLU backward of the blocks without InstanceNorm (SHM.py:298)

LRELU_C = (4, 48, 1024)
LRELU_BLOCKS = 4096               # grad_sums.hip shm_lrelu_bwd: "pix_chunks((long)npix, 1, c, 4096)"
LRELU_MIN_ITER = 16               # elem.h pix_chunks: "min_iter = blocks > 4096 ? 8 : 16"
LRELU_U = {"f32": 4, "bf16": 8, "gf32": 8}          # grad_sums.hip lrelu_bwd_kernel: "U = sizeof(T) == 2 ? 8 : 4"
LRELU_SLOTS = 64                  # SHM_LRELU_RED_SLOTS
LRELU_BIG = 4099
SUBNORMAL = {"f32": 2.0 ** -149, "bf16": 2.0 ** -133, "gf32": 2.0 ** -133}          # the smallest positive value of y's type


def lrelu_npix(c, dt):
    return (1, pp(c) * LRELU_U[dt] + 1, LRELU_BIG)


def lrelu_chunk(npix, c):
    """pixels per block (elem.h pix_chunks with batch = 1, then "chunk = (npix + nch - 1) / nch")"""
    nch = max(min(LRELU_BLOCKS, npix // (pp(c) * LRELU_MIN_ITER)), 1)
    return -(-npix // nch)


def lrelu_case(c, npix, dt, seed=0):
    """y holds +0.0, -0.0 and the smallest subnormal of its type in channels 0..2 of the first and of the last pixel"""
    rng = np.random.default_rng(9500 + c + npix + seed)
    k = SimpleNamespace(c=c, npix=npix, dt=dt)
    k.y = act(rng.standard_normal((npix, c)), dt)
    k.special = [(p, ch) for p in sorted({0, npix - 1}) for ch in range(3)]
    for p in {0, npix - 1}:
        k.y[p, :3] = (0.0, -0.0, SUBNORMAL[dt])
    k.dy = grad(rng.standard_normal((npix, c)) + 0.5, dt)
    k.db0 = rng.standard_normal(c)
    return k


def lrelu_bwd_ref(y, dy, slope=SLOPE, dtype=np.float64):
    """(dz, dbias sums)"""
    dz = tn.leaky_relu_grad(y.astype(dtype), dy.astype(dtype), dtype(slope))
    return dz, _colsum(dz)


def lrelu_special_ok(dz, k, tol):
    """the elements of dz under y = +0.0, -0.0 (slope applies) and y = subnormal (it does not), each within tol of its own reference"""
    ref = lrelu_bwd_ref(k.y, k.dy)[0]
    return all(abs(float(dz[p, ch]) - ref[p, ch]) <= tol * abs(ref[p, ch]) for p, ch in k.special)


# ---------------------------------------------------------------------------------------------------------------------------------------
# SpecSeg passes (SpecSeg.py:27-98) and the specular loss (SHM.py:792-806)

SPEC_GRID = 8192 * 256            # specseg.hip: "shm_grid_cap(total, 256, 8192)"
SPEC_LOSS_GRID = 256 * 256        # specseg.hip shm_spec_loss: "shm_grid_cap(n, 256, 256)"
BN_EPS = float(np.float32(1e-3))
SPEC_PITCH_MAP = (2, 6, 10, 8)    # batch, h, w, c; lda = c + 4, ldo = c + 8
# Sixteen channels are four vectors a pixel, so no pixel count gives 8192 * 256 + 77 vectors; this map gives 8192 * 256 + 1000: the
# grid-stride loop makes a second trip that ends inside a block (1000 = 3 * 256 + 232) and inside a wave (232 = 3 * 64 + 40)
SPEC_OVER_MAP = (1, 362, 1449, 16)          # batch, OUTPUT rows, columns, c (maxpool2 reads 724 x 2898)
PACK_CASES = ((1, 4), (1, 16), (3, 4), (3, 16))          # (nc, lddst)
PACK_SRC = (5, 1)                 # ldsrc, c0
PACK_NPIX = (77, SPEC_GRID + 77)  # lddst = 4: one vector a pixel
# 256 * 256 + 37 is no multiple of three; 3 * 21858 = 256 * 256 + 38 is the next count past the cap that three samples give
SPEC_LOSS_SHAPES = ((2, 77), (3, 21858))          # (batch, npix)


def bn_ref(a, gamma, beta, mean, var, eps=BN_EPS, dtype=np.float64):
    """Keras BatchNormalization(axis=-1) in inference mode"""
    a, gamma, beta, mean, var = (v.astype(dtype) for v in (a, gamma, beta, mean, var))
    return (a - mean) * gamma / np.sqrt(var + dtype(eps)) + beta


def bn_case(npix, c, seed=0):
    rng = np.random.default_rng(9700 + c + npix % 997 + seed)
    k = SimpleNamespace(npix=npix, c=c)
    k.a = r32(rng.standard_normal((npix, c), dtype=np.float32))
    k.gamma, k.beta, k.mean = (r32(rng.standard_normal(c)) for _ in range(3))
    k.var = r32(rng.random(c) + 0.1)
    return k


def maxpool_ref(x):
    """MaxPooling2D((2, 2)) of [n, h, w, c]; a selection: exact in any precision"""
    n, h, w, c = x.shape
    return x.reshape(n, h // 2, 2, w // 2, 2, c).max(axis=(2, 4))


def pack_ref(src, c0, nc, lddst):
    out = np.zeros((src.shape[0], lddst), src.dtype)
    out[:, :nc] = src[:, c0:c0 + nc]
    return out


def spec_case(batch, npix, seed=0):
    """mask of zeros and ones (the last pixels, the ragged tail of the grid-stride loop, are ones), five distinct ds"""
    rng = np.random.default_rng(9800 + batch + npix % 997 + seed)
    k = SimpleNamespace(batch=batch, npix=npix)
    k.cyc_y = r32(rng.standard_normal((5 * batch, npix, 1, 1)))
    k.cbcr = r32(rng.standard_normal((batch, npix, 1, 2)))
    k.ds = [r32(rng.standard_normal((batch, npix, 1, 3)) * (1.0 + 0.25 * j)) for j in range(5)]
    k.mask = (rng.random((batch, npix, 1, 1)) < 0.5).astype(np.float64)
    k.mask[-1, -64:] = 1.0
    return k


def spec_loss_ref(k, dtype=torch.float64, pixels=None):
    """the five raw sums of shm_spec_loss: oracle/specseg_torch.spec_loss's means times batch * npix * 3; pixels: only the first so many of
    the flat [batch * npix] pixel list enter (the teeth tests)"""
    B = k.batch
    m = k.mask.copy()
    if pixels is not None:
        m.reshape(-1)[pixels:] = 0.0
    cyc = [torch.cat([t64(k.cyc_y[j * B:(j + 1) * B]), t64(k.cbcr)], 3).to(dtype) for j in range(5)]
    _, terms = sp.spec_loss(cyc, [t64(d).to(dtype) for d in k.ds], t64(m).to(dtype))
    return np.array([float(t) for t in terms]) * (B * k.npix * 3)


# ---------------------------------------------------------------------------------------------------------------------------------------
# casts

CAST_GRID = 4096 * 256            # elem.hip shm_cast_f32: "shm_grid_cap(n, 256, 4096)"
CAST_SIZES = (1, 255, CAST_GRID + 77)
# float32 bit patterns: ties between two bf16 neighbours (to even: down, up) and one bit off them, +-0, subnormals (smallest, largest, a
# tie), the largest finite float (rounds to Inf) and the largest finite bf16, +-Inf, a quiet NaN and a NaN whose payload sits in the low 16
# bits alone (truncation would make it Inf)
CAST_BITS = np.array([0x3F818000, 0x3F808000, 0x3F808001, 0x3F807FFF, 0xBF818000, 0xBF808000, 0x00000000, 0x80000000, 0x00000001, 0x007FFFFF,
                      0x00008000, 0x00018000, 0x80000001, 0x7F7FFFFF, 0xFF7FFFFF, 0x7F7F0000, 0x7F800000, 0xFF800000, 0x7FC00000, 0x7F800001],
                     dtype=np.uint32)
# doubles: +-0, below the float subnormals, a float subnormal, beyond the float range, ties of the 24-bit significand, +-Inf, NaN
CVT_VALUES = np.array([0.0, -0.0, 1e-46, 1e-40, 3.5e38, -3.5e38, 1.0 + 2.0 ** -24, 1.0 + 3 * 2.0 ** -24, np.inf, -np.inf, np.nan, 1.0 / 3.0])


def cast_input(n):
    """float32 [n]: CAST_BITS at the front and again at the very end (the tail of the grid-stride loop), normal numbers of many magnitudes
    between; n = 1: the tie that rounds up"""
    rng = np.random.default_rng(9900 + n % 997)
    x = (rng.standard_normal(n) * np.exp(rng.uniform(-20, 20, n))).astype(np.float32)
    m = min(n, CAST_BITS.size)
    x[:m] = CAST_BITS[:m].view(np.float32)
    if n > 2 * CAST_BITS.size:
        x[-CAST_BITS.size:] = CAST_BITS.view(np.float32)
    return x


def cast_ref_bits(x):
    """bit patterns (int16) of torch's float32 -> bfloat16 conversion on the CPU, and where its result is NaN"""
    t = torch.from_numpy(x).to(torch.bfloat16)
    return t.view(torch.int16).numpy(), torch.isnan(t).numpy()


def same_bits(got_bits, ref_bits, nan):
    """bit for bit equal outside the NaNs, NaN where the reference has NaN (a NaN's payload is not a value)"""
    return bool(np.array_equal(got_bits[~nan], ref_bits[~nan]))


def cvt_input(n):
    rng = np.random.default_rng(9950 + n % 997)
    s = rng.standard_normal(n) * np.exp(rng.uniform(-10, 10, n))
    m = min(n, CVT_VALUES.size)
    s[:m] = CVT_VALUES[:m]
    if n > 2 * CVT_VALUES.size:
        s[-CVT_VALUES.size:] = CVT_VALUES
    d = rng.standard_normal(n).astype(np.float32)
    return s, d


def cvt_ref(s, d, accumulate):
    """float32(s), or d + float32(s) evaluated in float32"""
    with np.errstate(over="ignore", invalid="ignore"):
        s32 = s.astype(np.float32)
        return d + s32 if accumulate else s32
