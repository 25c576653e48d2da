"""Case tables and float64 NumPy references for the first-layer gradient stencil (csrc/dgrad_sum1.hip: shm_sum_input_channels,
shm_conv3x3_dgrad_sum1 in its three kernels and eight MFMA instances) and the layout and attention helpers round it (shm_transpose_taps,
shm_transpose_taps_multi in csrc/conv_igemm.hip; shm_mask_pool_pack(_hw), shm_add_bcast, shm_sum_groups, shm_mul_mask in csrc/elem.hip) at the
shapes the friendly-path tests leave out: partial 16 x 16 tiles, odd sides at stride 2, maps below one tile, a channel pitch wider than c,
accumulation, empty calls, non-finite data where the MFMA form's masked lanes read.  test_stencil_edges_cpu.py proves on the CPU that every
case is in the branch it claims, that the references agree with autograd and that the comparison has teeth; test_stencil_edges_gpu.py runs
the kernels.

The references are written from the contracts in include/shmgan_hip.h, not from the kernels.  Inputs are float64 arrays holding float32 (or
bf16) VALUES, so the device and the reference see the same numbers.
"""
from collections import namedtuple
from functools import lru_cache
from types import SimpleNamespace

import numpy as np
import torch

from heads_edge_ref import rb
from loss_edge_ref import SENT_BYTE, r32, t64          # noqa: F401  (re-exported for the tests)

f32, f64 = np.float32, np.float64
SPARE = 3.0                       # the project's factor between what a float32 evaluation reaches and what a bound allows
TORCH = {"f32": torch.float32, "bf16": torch.bfloat16}


# ---------------------------------------------------------------------------------------------------------------------------------------
# guard bands in front of and behind an output: one byte value, so that a store outside the payload is seen as a changed byte (0xA5A5A5A5
# is -2.9e-16 as a float, 0xA5A5 the same as a bf16: a missing store reads as zero)

GUARD_ELEMS = 256


def guarded2(n, dtype, device):
    """(raw bytes of the whole allocation, the n elements of dtype in its middle): GUARD_ELEMS elements of fill on either side"""
    item = torch.empty((), dtype=dtype).element_size()
    raw = torch.full(((n + 2 * GUARD_ELEMS) * item,), SENT_BYTE, dtype=torch.uint8, device=device)
    return raw, raw.view(dtype)[GUARD_ELEMS:GUARD_ELEMS + n]


def guards_intact(raw, payload):
    """every byte in front of and behind the payload still holds the fill"""
    lo = GUARD_ELEMS * payload.element_size()
    hi = lo + payload.numel() * payload.element_size()
    return bool((raw[:lo] == SENT_BYTE).all().item()) and bool((raw[hi:] == SENT_BYTE).all().item())


def untouched(raw):
    return bool((raw == SENT_BYTE).all().item())


def bits(a):
    """the bit patterns of a float32 array / bf16 or float32 torch tensor, for bit-for-bit comparisons"""
    if isinstance(a, torch.Tensor):
        a = a.detach().cpu().contiguous()
        return a.view(torch.int16 if a.dtype == torch.bfloat16 else torch.int32).numpy()
    return np.ascontiguousarray(a, dtype=f32).view(np.int32)


def to_dtype_bits(a32, dt):
    """bit patterns of the float32 array a32 stored in the call's dtype (bf16: round to nearest even, torch's conversion on the CPU)"""
    t = torch.from_numpy(np.ascontiguousarray(a32, dtype=f32))
    return bits(t.to(TORCH[dt]))


# ---------------------------------------------------------------------------------------------------------------------------------------
# shm_conv3x3_dgrad_sum1:  out[b,y,x] (+)= sum_k sum_taps sum_co dz[k*batch+b, oy, ox, co] * weff[k][tap][co]
# dz [nk*batch, ho, wo, c] activation-typed, weff f32 [nk][9][c], out f32 [batch, hi, wi]; stride 1 or 2 with TF SAME padding.

STENCIL_TOL = 1e-5                # rel-L2 against float64: the project's bound for this kernel (test_ops_gpu.test_first_layer_dgrad_channel_sum)
TO = 16                           # dgrad_sum1.hip, both tiled kernels: "constexpr int TO = 16" output pixels a side per block
LDS_NKC = 5 * 64                  # dgrad_sum1.hip shm_conv3x3_dgrad_sum1: "if (nk * c <= 5 * 64)": the tiled kernel's weight staging
KB = {"f32": 16, "bf16": 32}      # the same: "kb = dtype == SHM_F32 ? 16 : 32" channels per MFMA K block
MFMA_NKC = {"f32": (4, 20, 1, 5), "bf16": (2, 10, 1, 5)}          # the same: the eight "nkc ==" instances, in source order
# Worst |err| / A over the case table (both accumulate modes) of the float32 evaluation stencil_f32 -- one running sum per tap over (k, c),
# the taps added in order -- as test_stencil_edges_cpu.test_float32_evaluation_passes_with_room measures and asserts it; the per-pixel
# bound is SPARE times that.  The bf16 MFMA instances take their weights as a high plus a low bf16 part (the kernel's comment: 2^-17), so
# their evaluation runs on the split weights and has a constant of its own.
K_F32_MEASURED = 3.91e-7           # 6.6 * 2^-24: case (bf16 tiled, nk = 2, c = 128, 31 x 34, stride 2)
K_SPLIT_MEASURED = 2.41e-6         # 0.63 * 2^-18: case (bf16 MFMA, nk = 1, c = 32, 31 x 34, stride 2)
K_F32 = SPARE * K_F32_MEASURED
K_SPLIT = SPARE * K_SPLIT_MEASURED


def same_pad(n, stride, k=3):
    """TF SAME: out = ceil(n / stride), pad_total = max((out - 1) * stride + k - n, 0), pad_before = pad_total // 2"""
    out = -(-n // stride)
    return out, max((out - 1) * stride + k - n, 0) // 2


def form_of(dt, nk, c):
    """the dispatch of shm_conv3x3_dgrad_sum1 (dgrad_sum1.hip): "nkc = c % kb == 0 ? nk * c / kb : 0", the eight "nkc ==" branches, then
    "nk * c <= 5 * 64" for the tiled kernel, else the plain one"""
    nkc = nk * c // KB[dt] if c % KB[dt] == 0 else 0
    if nkc in MFMA_NKC[dt]:
        return ("mfma", dt, nkc)
    return ("tiled" if nk * c <= LDS_NKC else "plain", dt, 0)


def tile_regions(h, w, stride):
    """(R, Cn) per 16 x 16 output tile: the dz rows and columns its stencil touches ("oy_lo = fdiv(y0 + pt - 2, stride), oy_hi = fdiv(y0 + TO
    - 1 + pt, stride)"; not clipped to the map, as in the kernels)"""
    pt, pl = same_pad(h, stride)[1], same_pad(w, stride)[1]
    out = []
    for y0 in range(0, h, TO):
        for x0 in range(0, w, TO):
            R = (y0 + TO - 1 + pt) // stride - (y0 + pt - 2) // stride + 1
            Cn = (x0 + TO - 1 + pl) // stride - (x0 + pl - 2) // stride + 1
            out.append((R, Cn))
    return out


SIDES_S1 = ((1, 1), (5, 7), (15, 33), (16, 17), (17, 16), (33, 15))
SIDES_S2 = ((1, 1), (2, 2), (7, 5), (9, 16), (16, 9), (17, 17), (31, 34))
GEOMS = tuple((1, h, w) for h, w in SIDES_S1) + tuple((2, h, w) for h, w in SIDES_S2)
GEOMS_FEW = ((1, 5, 7), (1, 33, 15), (2, 7, 5), (2, 17, 17), (2, 31, 34))          # what a form that is not its kernel's first runs
# (dtype, nk, c) per kernel; the first of each (kernel, dtype) runs every geometry
FORMS = (
    ("f32", 5, 16), ("f32", 1, 16), ("f32", 1, 64), ("f32", 2, 32), ("f32", 5, 64),
    ("bf16", 2, 32), ("bf16", 1, 32), ("bf16", 1, 64), ("bf16", 5, 32), ("bf16", 5, 64),
    ("f32", 2, 16), ("f32", 1, 4), ("f32", 3, 8), ("f32", 2, 64), ("f32", 2, 128), ("f32", 1, 256),
    ("bf16", 2, 64), ("bf16", 1, 16), ("bf16", 2, 128), ("bf16", 1, 256),
    ("f32", 3, 128), ("f32", 6, 64), ("f32", 2, 256),
    ("bf16", 2, 256), ("bf16", 6, 64), ("bf16", 3, 128),
)
SC = namedtuple("SC", "dt nk c batch h w stride wide")


def wide_pitch(dt, c):
    return c + (4 if dt == "f32" else 8)


def form_cases(dt, nk, c):
    """the cases of one (dtype, nk, c): batch walks 1, 2, 3 and the pitch alternates tight / wide along the geometries"""
    kern = form_of(dt, nk, c)[:2]
    first = next(f for f in FORMS if form_of(*f)[:2] == kern) == (dt, nk, c)
    shift = FORMS.index((dt, nk, c))
    return tuple(SC(dt, nk, c, 1 + (i + 2) % 3, h, w, s, bool((i + shift) % 2)) for i, (s, h, w) in enumerate(GEOMS if first else GEOMS_FEW))


def all_cases():
    return tuple(sc for f in FORMS for sc in form_cases(*f))


# the non-finite cases: each kernel in each dtype, on maps with a partial tile
NONFINITE = tuple(SC(dt, nk, c, 2, h, w, s, wide) for dt, nk, c in (("f32", 5, 16), ("bf16", 5, 32), ("f32", 3, 8), ("bf16", 1, 16), ("f32", 3, 128), ("bf16", 2, 256))
                  for s, h, w, wide in ((1, 15, 33, False), (2, 17, 17, True)))


def stencil_ref(dz, weff, nk, batch, h, w, stride):
    """The header's definition as a scatter, in float64: input pixel y receives tap kh from output row oy where y + pt - kh == stride * oy
    (and the same along x).  A product with a dz pixel outside the map does not exist, so 0 * Inf never arises."""
    (ho, pt), (wo, pl) = same_pad(h, stride), same_pad(w, stride)
    dz, weff = np.asarray(dz, f64), np.asarray(weff, f64)
    assert dz.shape[:3] == (nk * batch, ho, wo) and weff.shape == (nk, 9, dz.shape[3])
    out = np.zeros((batch, h, w))
    bi = np.arange(batch)[:, None, None]
    for k in range(nk):
        for kh in range(3):
            y = stride * np.arange(ho) + kh - pt
            vy = (y >= 0) & (y < h)
            for kw in range(3):
                x = stride * np.arange(wo) + kw - pl
                vx = (x >= 0) & (x < w)
                with np.errstate(invalid="ignore"):
                    contrib = (dz[k * batch:(k + 1) * batch] * weff[k, kh * 3 + kw]).sum(-1)
                    np.add.at(out, (bi, y[vy][None, :, None], x[vx][None, None, :]), contrib[:, vy][:, :, vx])
    return out


def tap_products(dz, weff, nk, batch, dtype=f64, order="kb"):
    """P[b, oy, ox, tap] = sum_k sum_c dz[k*batch+b, oy, ox, c] * weff[k, tap, c].  float64: one einsum; float32: one running sum per tap,
    a channel at a time -- the plainest single-precision evaluation.  order = "bk": the fault of reading tensor b * nk + k."""
    n, ho, wo, c = dz.shape
    d = dz.reshape(batch, nk, ho, wo, c).transpose(1, 0, 2, 3, 4) if order == "bk" else dz.reshape(nk, batch, ho, wo, c)
    if dtype == f64:
        with np.errstate(invalid="ignore"):
            return np.einsum("kbyxc,ktc->byxt", d.astype(f64), weff.astype(f64))
    d, wq = d.astype(dtype), weff.astype(dtype)
    P = np.zeros((batch, ho, wo, 9), dtype)
    for k in range(nk):
        for ch in range(c):
            P += d[k, ..., ch, None] * wq[k, :, ch]
    return P


def gather(P, h, w, stride, fault=None):
    """out[b, y, x] = sum of the valid taps' P entries -- the same stencil from the output pixel's side, in P's precision, the taps added
    in the order kh, kw.  fault: one of FAULTS, a modelled kernel fault."""
    (ho, pt), (wo, pl) = same_pad(h, stride), same_pad(w, stride)
    if fault == "pad0":
        pt = pl = 0
    batch = P.shape[0]
    out = np.zeros((batch, h, w), P.dtype)

    def axis(n, no, pad, kk):
        nn = np.arange(n) + pad - kk
        par = (nn >= 0) & ((nn % stride == 0) | (fault == "noparity"))
        o = np.where(nn >= 0, nn, 0) // stride
        return np.clip(o, 0, no - 1), par & (o < no), (nn < 0) | (par & (o >= no))

    for kh in range(3):
        oy, vy, my = axis(h, ho, pt, kh)
        for kw in range(3):
            ox, vx, mx = axis(w, wo, pl, kw)
            t = kw * 3 + kh if fault == "swap" else kh * 3 + kw
            g = P[:, oy][:, :, ox, t]
            m = vy[:, None] & vx[None, :]
            with np.errstate(invalid="ignore"):
                out = out + np.where(m, g, P.dtype.type(0))
                if fault == "masked":          # a tap that falls outside the map adds dz pixel 0's product instead of nothing
                    outside = (vy | my)[:, None] & (vx | mx)[None, :] & ~m
                    out = out + np.where(outside, P[:, 0, 0, t][:, None, None], P.dtype.type(0))
    if fault == "rows" and h % TO:
        out[:, h - h % TO:] = 0
    if fault == "cols" and w % TO:
        out[:, :, w - w % TO:] = 0
    return out


# modelled faults: pad_before = 0 on an odd axis at stride 2; the partial tile's rows / columns not written (they keep the fill, ~0); kh
# and kw exchanged; tensor index b * nk + k; a masked lane's pixel-0 contribution added in; accumulate ignored; the parity skip dropped
FAULTS = ("pad0", "rows", "cols", "swap", "bk", "masked", "noacc", "noparity")


def bf16_split(w):
    """w as the bf16 MFMA instances take it: bf16(w) + bf16(w - bf16(w))"""
    hi = rb(w)
    return hi + rb(r32(w - hi))


@lru_cache(maxsize=None)
def stencil_case(sc, inf=False):
    """inputs and float64 references of one case, computed once and read-only: dz [nk*batch, ho, wo, c] in the call's dtype (mean 0.5) and
    weff [nk, 9, c] (mean 0.05, no zero): sums that do not cancel to nothing on the smallest maps; out0 what `out` holds before an
    accumulating call; s the stencil, A the same stencil of |dz| and |weff| (the scale of the per-pixel bound).  inf: one channel of pixel
    (0, 0) of every dz tensor is +Inf."""
    rng = np.random.default_rng([sc.nk, sc.c, sc.batch, sc.h, sc.w, sc.stride, int(sc.dt == "bf16"), 2027])
    ho, wo = same_pad(sc.h, sc.stride)[0], same_pad(sc.w, sc.stride)[0]
    k = SimpleNamespace(sc=sc, ho=ho, wo=wo, ld=wide_pitch(sc.dt, sc.c) if sc.wide else sc.c)
    dz = rng.standard_normal((sc.nk * sc.batch, ho, wo, sc.c)) + 0.5
    k.dz = r32(dz) if sc.dt == "f32" else rb(dz)
    k.weff = r32((rng.standard_normal((sc.nk, 9, sc.c)) + 0.5) * 0.1)
    k.out0 = r32(rng.standard_normal((sc.batch, sc.h, sc.w)))
    if inf:
        k.dz[:, 0, 0, sc.c // 2 + 1] = np.inf
    k.s = stencil_ref(k.dz, k.weff, sc.nk, sc.batch, sc.h, sc.w, sc.stride)
    k.A = stencil_ref(np.abs(k.dz), np.abs(k.weff), sc.nk, sc.batch, sc.h, sc.w, sc.stride)
    for a in (k.dz, k.weff, k.out0, k.s, k.A):
        a.setflags(write=False)
    return k


def stencil_expect(k, accumulate):
    """(reference, scale of the per-pixel bound) of a call: accumulating adds out0, and one rounding of the sum"""
    return (k.out0 + k.s, k.A + np.abs(k.out0)) if accumulate else (k.s, k.A)


def stencil_k(sc):
    return K_SPLIT if form_of(sc.dt, sc.nk, sc.c)[:2] == ("mfma", "bf16") else K_F32


def stencil_f32(k, accumulate, fault=None, dtype=f32):
    """the stencil of case k in single precision (dtype = float64 with a fault: the modelled faults, free of rounding)"""
    sc = k.sc
    wq = bf16_split(k.weff) if form_of(sc.dt, sc.nk, sc.c)[:2] == ("mfma", "bf16") and dtype == f32 else k.weff
    P = tap_products(k.dz, wq, sc.nk, sc.batch, dtype, "bk" if fault == "bk" else "kb")
    s = gather(P, sc.h, sc.w, sc.stride, fault)
    if fault == "noacc":
        accumulate = not accumulate
    return k.out0.astype(dtype) + s if accumulate else s


def stencil_figs(got, ref, A):
    """(rel-L2 over the pixels finite in the reference, worst |got - ref| / A over them): both infinite unless got is non-finite at exactly
    the reference's non-finite pixels"""
    ref, A = np.asarray(ref, f64), np.asarray(A, f64)
    got = np.asarray(got, f64).reshape(ref.shape)
    fin = np.isfinite(ref)
    if not np.array_equal(np.isfinite(got), fin):
        return float("inf"), float("inf")
    if not fin.any():
        return 0.0, 0.0
    with np.errstate(invalid="ignore"):
        d, a = np.abs(got - ref)[fin], A[fin]
    rel = float(np.linalg.norm(d) / max(np.linalg.norm(ref[fin]), 1e-30))
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(a > 0, d / a, np.where(d == 0, 0.0, np.inf))
    return rel, float(ratio.max())


def stencil_ok(figs, kk):
    return figs[0] < STENCIL_TOL and figs[1] <= kk


# ---------------------------------------------------------------------------------------------------------------------------------------
# shm_sum_input_channels: weff[t][co] = sum_{j : mask bit j} w[t][j][co]   (w = HWIO [9][cin][cout], cin <= 32)

SUMCH_CIN = (1, 3, 10, 32)
SUMCH_COUT = (1, 16, 29, 64)          # 9 * cout = 9, 144, 261, 576: either side of one block
SUMCH_BLOCK = 256                     # dgrad_sum1.hip shm_sum_input_channels: "shm_cdiv(9 * cout, 256)"
SUMCH_UNIT = 32 * 2.0 ** -24          # |err| <= 32 * 2^-24 * sum_j |w_j|: at most 31 float additions of at most 32 terms, each 2^-24 relative


def sumch_masks(cin):
    """no channel; every bit of the word (those at or above cin are ignored); the channels alone; the top channel alone (bit 31 at cin = 32);
    a pattern with bits at or above cin set as well"""
    full = (1 << cin) - 1
    return (0, 0xFFFFFFFF, full, 1 << (cin - 1), (0x5A5A5A5A & full) | (0xFFFFFFFF & ~full))


def sumch_case(cin, cout):
    return r32(np.random.default_rng(300 + 64 * cin + cout).standard_normal((9, cin, cout)))


def sumch_ref(w, mask, dtype=f64):
    """(weff [9, cout], sum of |w_j| over the selected channels)"""
    sel = [j for j in range(w.shape[1]) if (mask >> j) & 1]
    wq = w.astype(dtype)
    s, a = np.zeros((9, w.shape[2]), dtype), np.zeros((9, w.shape[2]))
    for j in sel:
        s = s + wq[:, j]
        a = a + np.abs(w[:, j])
    return s, a


# ---------------------------------------------------------------------------------------------------------------------------------------
# shm_transpose_taps(_multi): [ntaps][rows][cols] -> [ntaps][cols][rows_pad] (zero padded)

TRANSPOSE_TILE = 32               # conv_igemm.hip transpose_taps_kernel: "__shared__ float tile[32][33]"
TRANSPOSE_MAX = 48                # conv_igemm.hip: "constexpr int kMaxTransposes = 48;"
TRANSPOSE_SHAPES = ((1, 1, 1, 1), (9, 31, 33, 32), (9, 32, 32, 32), (9, 33, 31, 64), (4, 10, 5, 80), (9, 3, 64, 16))          # ntaps, rows, cols, rows_pad


def transpose_case(i, shape):
    ntaps, rows, cols, _ = shape
    return np.random.default_rng(500 + i).standard_normal((ntaps, rows, cols)).astype(f32)


def transpose_ref(w, rows_pad):
    ntaps, rows, cols = w.shape
    out = np.zeros((ntaps, cols, rows_pad), f32)
    out[:, :, :rows] = np.transpose(w, (0, 2, 1))
    return out


# ---------------------------------------------------------------------------------------------------------------------------------------
# the attention helpers and the dropout multiply: a single max, a single add, a fixed-order sum -- bit for bit

POOL_LD = (1, 16, 20, 32)
POOL_SQUARE = ((3, 30, 1), (3, 30, 2), (3, 30, 3), (3, 30, 5), (2, 24, 8))                                   # batch, s, k
POOL_HW = ((3, 15, 10, 5), (2, 34, 26, 2), (1, 3, 6, 3), (2, 8, 16, 8), (1, 7, 9, 1))                        # batch, h, w, k
ELEM_BLOCK = 256                  # elem.hip: every launch here is "shm_cdiv((long)total, 256)" blocks of 256 threads


def pool_mask(batch, h, w, negative):
    """[batch, h, w] float32: mixed signs, or negative everywhere (a running maximum that starts from zero would return zero)"""
    m = np.random.default_rng(700 + 31 * batch + 7 * h + w).standard_normal((batch, h, w)).astype(f32)
    return -np.abs(m) - f32(0.125) if negative else m


def pool_ref(m, k, ld):
    """MaxPooling2D(k x k) into channel 0 of [batch, h/k, w/k, ld], the other channels +0.0; float32 (a selection is exact)"""
    b, h, w = m.shape
    out = np.zeros((b, h // k, w // k, ld), f32)
    out[..., 0] = m.reshape(b, h // k, k, w // k, k).max(axis=(2, 4))
    return out


# (nimg, per, nb, i0): per = 4 (one vector an image); per / 4 = 77 does not divide 256; one sample; more samples than images (groups that
# receive no image); an offset beyond the sample count; no image at all
BCAST_CASES = ((7, 4, 3, 2), (5, 308, 3, 1), (4, 308, 1, 0), (2, 308, 5, 3), (7, 308, 3, 7), (9, 4, 3, 7), (0, 308, 3, 1), (0, 4, 2, 0))


def bcast_case(case, dt):
    nimg, per, nb, i0 = case
    rng = np.random.default_rng(800 + 13 * nimg + per + 5 * nb + i0)
    q = (lambda a: r32(a).astype(f32)) if dt == "f32" else (lambda a: rb(a).astype(f32))
    return SimpleNamespace(a=q(rng.standard_normal((nimg, per))), b=q(rng.standard_normal((nb, per))), d0=q(rng.standard_normal((nb, per)) * 3))


def group_of(i, nb, i0):
    return (i0 + i) % nb


def add_bcast_ref(a, b, nb, i0):
    """out[i] = a[i] + b[(i0 + i) % nb] in float32"""
    return a + b[[group_of(i, nb, i0) for i in range(a.shape[0])]] if a.shape[0] else a.copy()


def sum_groups_ref(src, d0, nb, i0, accumulate):
    """dst[j] (+)= sum of src[i] over the images with (i0 + i) % nb == j, in float32, the images in ascending order onto dst (or zero)"""
    out = d0.copy() if accumulate else np.zeros_like(d0)
    for i in range(src.shape[0]):
        out[group_of(i, nb, i0)] += src[i]
    return out


MULMASK_N = (4 * 100, 4 * 256, 4 * (3 * 256 + 77))          # n / 4 below one block, one block, ragged above
MULMASK_SCALE = float(f32(1.0 / 0.9))                       # no power of two: (x * m) * scale and x * (m * scale) differ in the last bit


def mulmask_case(n, dt):
    rng = np.random.default_rng(900 + n)
    x = rng.standard_normal(n)
    x = (r32(x) if dt == "f32" else rb(x)).astype(f32)
    m = rng.standard_normal(n).astype(f32)
    m[::3] = (rng.random(m[::3].size) < 0.8).astype(f32)          # a third of it a keep mask of zeros and ones
    return x, m


def mulmask_ref(x, m, scale):
    """y = (x * mask) * scale in float32"""
    return (x * m) * f32(scale)
