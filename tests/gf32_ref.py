"""SHM_BF16_GF32 -- bf16 activations and weights, the gradient signal in fp32 (trainer grad_dtype="float32") -- in every kernel family: the case
table of test_gf32_gpu.py and of the "gf32" rows of test_gsum_gpu.py / test_in_bwd_plan_gpu.py, what each case must run, and NumPy models of
the faults the comparison has to catch (test_gf32_cpu.py).  Nothing here touches the device.

What the mode changes, as restated from the sources (test_gf32_cpu.py pins each to its line):
  * outputs are 4 bytes (`oesz = dtype == SHM_BF16 ? 2 : 4`), operands and gsum aux 2 (`esz`): every tap-GEMM kernel runs as its <__bf16, float> form
    and stores through the element epilogues (pitch sizeof(TO)), reading aux through 16-bit loads (pitch sizeof(T));
  * the weights-in-registers family: only the four-wave kernel stores fp32 (tapgemm_wreg_kernel<float, K / 32>); the eight-wave and ping-pong kernels
    need `oesz == 2`, and so does its gsum form -- the reduce pass delivers the sums;
  * the four-phase kernel takes the gsum request in its epilogue on `oesz == 4`;
  * fused forward statistics do not exist ("SHM_BF16_GF32 has no fused statistics");
  * shm_in_bwd: the one-pass forms require `q.dtype == SHM_BF16`; `wide8` includes the mode (in_bwd_reduce8_kernel for c % 8 == 0).
"""
import numpy as np

TOL32 = 1e-4                # fp32 results of bf16 operands against float64 on the rounded operands (test_bf16_gpu.TOL32)
SUM_TOL = 2e-5              # test_gsum_gpu._check_sums: slot sums against float64, relative to the scale of the summands
SENTINEL = 7.0              # util.SENTINEL

HALO = ["halo128", "halo64", "halo128_st", "halo64_st", "halo128_st_w4"]          # test_variants_gpu.HALO / DMA
DMA = ["dma128x128", "dma64x128", "dma128x64", "dma64x64", "dma256x64", "dma256x128", "dma128x128_bk32", "dma128x128_nst4"]
DMA_S2 = [v for v in DMA if v != "dma128x128_nst4"]                                # test_dgrad_s2_and_transpose_forced_variant's seven
GSUM_HALO = HALO[:4]                                                               # test_gsum_gpu.HALO

R8, R4 = "in_bwd_reduce8_kernel + in_bwd_apply_kernel", "in_bwd_reduce_kernel + in_bwd_apply_kernel"


def _c(sec, entry, variant, expect="run", gsum=None, **shape):
    """expect: "run" (shm_last_kernel() names the variant's <__bf16, float> form) or "refuse" (ShmError before any launch, nothing written).
    gsum: None, "epilogue" (the launch takes the sums) or "reduce" (the follow-up pass does)."""
    return dict(sec=sec, entry=entry, variant=variant, expect=expect, gsum=gsum, **shape)


def table():
    t = []
    # 1. unit-stride input gradients, split destination (the shape of test_dgrad_s1_forced_variant), rectangles, the ping-pong shape
    t += [_c(1, "dgrad", v, n=2, h=16, w=16, c1=64, c2=64, cout=64) for v in HALO + DMA + ["wreg"]]
    t += [_c(1, "dgrad", v, n=2, h=h, w=w, c1=64, c2=64, cout=64) for v in ("halo128_st", "halo64_st", "dma128x128", "dma256x128") for h, w in ((16, 32), (32, 16))]
    t += [_c(1, "dgrad", "wreg", n=3, h=32, w=32, c1=64, c2=64, cout=64)]
    # 2. stride-2 input gradients: dx [n, h, w, cin] from dy [n, h / 2, w / 2, cout]
    t += [_c(2, "dgrad_s2", v, n=2, h=16, w=16, cin=64, cout=128) for v in DMA_S2]
    t += [_c(2, "dgrad_s2", "phase4", n=n, h=h, w=h, cin=cin, cout=cout) for n, h, cin, cout in ((2, 32, 64, 64), (1, 96, 192, 64))]
    t += [_c(2, "dgrad_s2", v, n=2, h=2 * h, w=2 * w, cin=64, cout=64) for v in ("phase4", "dma128x128") for h, w in ((16, 48), (48, 16))]
    # 3. the stride-2 forward form with fp32 output (Conv2DTranspose's input gradient in model.py)
    t += [_c(3, "fwd_s2", v, n=2, h=32, w=32, cin=64, cout=128) for v in ("auto", "dma128x128", "dma256x128", "dma64x64")]
    t += [_c(3, "in_fwd", "auto", expect="refuse", n=2, h=32, w=32, cin=64, cout=128)]
    # 4. gsum (the "gf32" cases of test_gsum_gpu.py)
    for n, h, cin, cout, n1 in ((3, 16, 64, 64, 0), (2, 32, 256, 64, 128), (2, 16, 192, 128, 64)):
        t += [_c(4, "dgrad_gsum", v, gsum="epilogue" if v.endswith("_st") or v in DMA else "reduce", n=n, h=h, w=h, cin=cin, cout=cout, n1=n1) for v in GSUM_HALO + DMA]
    t += [_c(4, "dgrad_gsum_flat", v, gsum="epilogue" if v in DMA else "reduce", n=2, h=32, w=32, cin=256, cout=64, n1=128) for v in ("dma128x128", "dma64x128", "dma256x128", "halo128_st")]
    t += [_c(4, "dgrad_gsum", "wreg", gsum="reduce", n=n, h=h, w=h, cin=cin, cout=cout, n1=n1) for n, h, cin, cout, n1 in ((3, 16, 64, 64, 0), (2, 32, 128, 64, 64), (7, 48, 64, 64, 0), (2, 32, 128, 32, 64))]
    t += [_c(4, "dgrad_s2_gsum", "phase4", gsum="epilogue", n=2, h=32, w=32, cin=64, cout=128), _c(4, "dgrad_s2_gsum", "dma128x128", gsum="epilogue", n=2, h=32, w=32, cin=64, cout=128),
          _c(4, "dgrad_s2_gsum", "dma128x64", gsum="epilogue", n=3, h=16, w=16, cin=64, cout=64), _c(4, "dgrad_gsum", "auto", gsum="reduce", n=3, h=4, w=4, cin=64, cout=64, n1=0)]
    t += [_c(4, "fwd_s2_gsum", v, gsum="epilogue", n=2, h=32, w=32, cin=64, cout=128) for v in ("auto", "dma128x128", "dma256x128", "dma64x64")]
    return t


def cases(sec, entry):
    return [c for c in table() if c["sec"] == sec and c["entry"] == entry]


def case_id(c):
    return "-".join([c["variant"]] + [f"{k}{c[k]}" for k in ("n", "h", "w", "cin", "c1", "cout") if k in c])


# shm_in_bwd rows (test_in_bwd_plan_gpu.TABLE): (request in bf16, its form in bf16, its form in this mode)
IN_BWD = [("fused8-2048-pixel-slice", "in_bwd_fused8_kernel<false>", R8), ("fused8-pooled", "in_bwd_fused8_kernel<true>", R8), ("fusedg-forced-v0", "in_bwd_fusedg_kernel<2, 2, 4>", R8),
          ("c48", R8, R8), ("c36", R4, R4)]


# ---------------------------------------------------------------------------------------------------------------- the checks, on the host
def rel_l2(a, b):
    a, b = np.asarray(a, np.float64).ravel(), np.asarray(b, np.float64).ravel()
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


def bf16_round(a):
    """float64 values rounded to bf16 (round to nearest even on the float32 bit pattern), as float64"""
    u = np.ascontiguousarray(a, np.float32).view(np.uint32).astype(np.uint64)
    u = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16
    return u.astype(np.uint32).view(np.float32).astype(np.float64)


def sums(g, aux):
    """float64 (sum g, sum g * aux) per (sample, channel): test_gsum_gpu._sums"""
    n, c = g.shape[0], g.shape[-1]
    g2, a2 = np.asarray(g, np.float64).reshape(n, -1, c), np.asarray(aux, np.float64).reshape(n, -1, c)
    return np.stack([g2.sum(1), (g2 * a2).sum(1)], -1)


def sums_close(got, g, aux):
    """test_gsum_gpu._check_sums"""
    n, c = g.shape[0], g.shape[-1]
    scale = np.sqrt((np.asarray(g, np.float64) ** 2).reshape(n, -1, c).sum(1))[..., None] + 1e-30
    return bool((np.abs(got - sums(g, aux)) / scale).max() < SUM_TOL)


def output_ok(buf, band, ref):
    """What every case of test_gf32_gpu.py asks of an output: guard band untouched, no sentinel left inside, rel-L2 against float64 within TOL32"""
    return bool((band == SENTINEL).all()) and not bool((buf == SENTINEL).all(-1).any()) and rel_l2(buf, ref) < TOL32


# ---------------------------------------------------------------------------------------------------------------- the fault models
FAULTS = ("bf16-round-trip", "aux-read-as-f32", "pitch-in-2-byte-units", "sums-of-rounded-values")


def model_launch(ref, aux_bf16, fault=None):
    """A gsum launch of this mode on the host: `ref` [n, h, w, c] is the float64 product, `aux_bf16` the aux tensor as uint16 bf16 bit patterns.
    Returns (output buffer fp32 [n, h, w, c], guard band, sums [n, c, 2]) as a correct kernel -- or one with `fault` -- leaves them."""
    n, h, w, c = ref.shape
    stored = ref.astype(np.float32)
    if fault == "bf16-round-trip":                       # the result went through bf16 on its way to the fp32 tensor
        stored = bf16_round(ref).astype(np.float32)
    guard = 16 * w * c
    flat = np.full(n * h * w * c + guard, SENTINEL, np.float32)
    if fault == "pitch-in-2-byte-units":                 # pixel p at byte p * c * 2: every row over the second half of the one before, the tensor's second half unwritten
        b = flat.view(np.uint8)
        rows = stored.reshape(-1, c).view(np.uint8)
        for p in range(rows.shape[0]):
            b[p * c * 2:p * c * 2 + c * 4] = rows[p]
    else:
        flat[:n * h * w * c] = stored.ravel()
    aux = (aux_bf16.astype(np.uint32) << 16).view(np.float32).astype(np.float64)
    if fault == "aux-read-as-f32":                       # a 4-byte load at the element's 2-byte offset: two neighbouring bf16 values taken as one float
        raw = np.concatenate([aux_bf16.ravel(), np.zeros(1, np.uint16)])
        both = raw[:-1].astype(np.uint32) | (raw[1:].astype(np.uint32) << 16)
        with np.errstate(all="ignore"):
            aux = np.nan_to_num(both.view(np.float32).astype(np.float64).reshape(aux_bf16.shape), nan=0.0, posinf=3e38, neginf=-3e38)
    g = stored.astype(np.float64)
    if fault == "sums-of-rounded-values":                # the sums see the bf16 value of a bf16-output kernel, the tensor the fp32 one
        g = bf16_round(g)
    with np.errstate(all="ignore"):
        red = sums(g, aux)
    return flat[:n * h * w * c].reshape(n, h, w, c), flat[n * h * w * c:], red
