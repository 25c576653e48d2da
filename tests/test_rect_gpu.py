"""Every convolution, weight-gradient and InstanceNorm kernel family on RECTANGULAR maps, and the stride-2 layers on odd sizes.

Every tiled kernel splits a flat patch index into a patch row and a patch column (`ppr = wi >> 4, ppi = (hi / PH) * ppr`, "patches
numbered down the columns" in the weight-gradient halo kernels, `gpi = ho * (wo / 16)` in the RGB layer), and some eligibility rules
look at one axis only.  On the square maps of the other modules a height used where the width was meant, a row pitch from the wrong
axis, a transposed patch order or `pt` / `pl` exchanged all give the right answer (test_rect_cpu.py shows that on the reference).
Here every case runs as (h, w) and as (w, h), with one side exactly one patch and the other several, so a map has both "every halo
column is padding" and interior patches with neighbours; n >= 2, so blocks cross image boundaries.

Method of test_variants_gpu.py: the kernel is forced through shm_set_tuning, shm_last_kernel() is asserted (a pass proves that kernel
computed the result), the reference is float64 on the operands as the device holds them.  Tolerances are the ones the project already
holds these ops to (fp32 rel-L2 1e-5, bf16 forward / input gradient 4e-3, bf16 weight gradient 1e-4, statistics as _check_stats,
bit-identity where the square test demands it).  Every output tensor is allocated with a guard band of one patch row of elements
behind its logical end, filled with a sentinel that must still be there afterwards: an overrun is a failed assert, not a fault.

The second half runs the TF SAME padding of stride-2 layers on odd and mixed-parity sizes (pad_before 1 on the odd axis, 0 on the
even one), which the even squares of the other modules never reach.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import elem_bound_ref as eb
from oracle import step_torch as st
from oracle import tf_ops_np as tn
from test_gsum_gpu import _check_sums, _sums
from test_variants_gpu import DMA, HALO, _check_stats, _dev, _rnd, _sym, _wk
from util import RECT_TOL as TOL
from util import SENTINEL, band_untouched, conv_ref, guard_elems, host, nchw, nhwc, pad_c, rect_close, rel_l2, t64

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
WTOL = {"f32": 1e-5, "bf16": 1e-4}          # weight gradients (fp32 results of fp32 / bf16 products)
DTS = ["f32", "bf16"]


def _ops():
    from shmgan_amd import ops
    return ops


@pytest.fixture(autouse=True)
def _reset_tuning():
    yield
    _ops().set_tuning("reset", 0)


def _adt(dt):
    return BF if dt == "bf16" else torch.float32


def _guarded(shape, adt=torch.float32, fill=SENTINEL):
    """A tensor of `shape` in front of a guard band of one patch row of elements, all `fill`.  Returns (tensor, band)."""
    n = int(np.prod(shape))
    flat = torch.full((n + guard_elems(shape),), fill, device="cuda", dtype=adt)
    return flat[:n].view(shape), flat[n:]


def _both(*hw):
    """(h, w) and (w, h) of every rectangle."""
    return [p for h, w in hw for p in ((h, w), (w, h))]


def _f32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def _lrelu(a, slope=0.2):
    return np.where(a > 0, a, slope * a)


# =====================================================================================================================
# forward 3x3, stride 1: conv (+ concat) + bias + LeakyReLU + fused statistics
def _fwd(variant, dt, n, h, w, c1, c2, cout, k=3, s=1, seed=0, expect=None, in_stats=True, slope=0.2, small_stats=False):
    ops = _ops()
    rng = np.random.default_rng(300 + seed)
    cin = c1 + c2
    xa = rng.standard_normal((n, h, w, c1))
    xb = rng.standard_normal((n, h, w, c2)) if c2 else None
    wt = rng.standard_normal((k, k, cin, cout)) * 0.1
    b = rng.standard_normal(cout)
    xr = _rnd(xa, dt) if xb is None else np.concatenate([_rnd(xa, dt), _rnd(xb, dt)], -1)
    ref = _lrelu(conv_ref(xr, _rnd(wt, dt), s) + b, slope)
    ho, wo = ref.shape[1], ref.shape[2]
    y, band = _guarded((n, ho, wo, cout), _adt(dt))
    ops.set_tuning("tapgemm.variant", variant)
    args = (_dev(xa, dt), None if xb is None else _dev(xb, dt), c1 if c2 else 0, c1, c2, _wk(wt, cin, dt), _f32(b), y, cout, n, h, w, cin, cout, k, s, slope)
    if in_stats:
        stats = torch.empty(n * cout * 2, dtype=torch.float64, device="cuda")
        scr = torch.zeros(ops.STATS_SLOTS * n * cout * 2, dtype=torch.float64, device="cuda")
        ops.conv2d_in_fwd(*args, stats, 1e-6, scratch=scr)
    else:
        ops.conv2d_fwd(*args)
    torch.cuda.synchronize()
    kern = ops.last_kernel()
    if expect is None:
        expect = _sym(variant, dt, cin / 32, hw=(h, w))
    if expect:
        assert kern == expect, (kern, expect)
    got = host(y.float())
    assert band_untouched(band), kern
    assert rect_close(got, ref, dt), (kern, dt, rel_l2(got, ref))
    eb.hold_fwd(got, xr, _rnd(wt, dt), b, s, ref, dt, "fwd " + kern.split("<")[0])
    if in_stats and ((ho * wo) % 64 == 0 or small_stats):      # (smaller maps take a separate statistics pass)
        _check_stats(stats, got, n, cout, dt)
        assert float(scr.abs().max()) == 0.0                 # "zero on entry, zero on return"
    return kern


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("variant", HALO + DMA)
@pytest.mark.parametrize("h,w,c1,c2,cout", [(16, 48, 64, 0, 64), (48, 16, 64, 0, 64), (32, 16, 64, 128, 128), (16, 32, 64, 128, 128)])
def test_conv3x3_s1_forced_variant_rect(variant, dt, h, w, c1, c2, cout):
    _fwd(variant, dt, 2, h, w, c1, c2, cout)


@pytest.mark.parametrize("h,w", _both((16, 48)))
def test_halo_ph8_rect(h, w):
    """the 8-row patch variant (bf16 only): `ppi = (hi / 8) * ppr`"""
    _fwd("halo128_ph8", "bf16", 2, h, w, 64, 0, 128, seed=1)


# ---- weights-in-registers kernels
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("h,w", _both((16, 48)))
def test_wreg_forced_variant_rect(dt, h, w):
    """fp32: tapgemm_wreg_f32_kernel; bf16: neither 16 x 48 nor 48 x 16 is whole 8 x 32 patches, so the default ("tapgemm.wreg16" = 2) moves
    from the ping-pong kernel to the eight-wave kernel, as _sym predicts; "tapgemm.wreg16" = 1 and 0 name their kernels."""
    k = _fwd("wreg", dt, 3, h, w, 64, 0, 64, seed=2)
    if dt == "bf16":
        assert k == "tapgemm_wreg16_bf16_kernel<2, true>", k
        _ops().set_tuning("tapgemm.wreg16", 1)
        _fwd("wreg", dt, 3, h, w, 64, 0, 64, seed=2, expect="tapgemm_wreg16_bf16_kernel<2, true>")
        _ops().set_tuning("tapgemm.wreg16", 0)
        _fwd("wreg", dt, 3, h, w, 64, 0, 64, seed=2, expect="tapgemm_wreg_kernel<__bf16, 2>")


@pytest.mark.parametrize("h,w", [(64, 32), (16, 96), (32, 64), (96, 32)])
def test_pingpong_forward_rect(h, w):
    """maps of whole 8 x 32 patches: one patch column with many patch rows, many columns in two rows, and the transposes that still tile"""
    _fwd("wreg", "bf16", 2, h, w, 64, 0, 64, seed=3, expect="tapgemm_pp_bf16_kernel<2>")
    _fwd("wreg", "bf16", 3, h, w, 64, 0, 128, seed=4, expect="tapgemm_pp_bf16_kernel<1>", in_stats=False)


@pytest.mark.parametrize("h,w", [(8, 64), (96, 16)])
def test_pingpong_leaves_what_it_cannot_tile(h, w):
    """8 x 64 is whole 8 x 32 patches, but the weights-in-registers family is entered through the 16 x 16-patch rule (map a multiple of 16 both
    ways): forced it is refused before any launch, the automatic choice runs another kernel; 96 x 16 has no 32-column patch: the eight-wave kernel."""
    from shmgan_amd._lib import ShmError
    ops = _ops()
    if h % 16:
        x = torch.zeros((2, h, w, 64), device="cuda", dtype=BF)
        y, band = _guarded((2, h, w, 64), BF)
        ops.set_tuning("tapgemm.variant", "wreg")
        with pytest.raises(ShmError):
            ops.conv2d_fwd(x, None, 0, 64, 0, torch.zeros(9 * 64 * 64, device="cuda", dtype=BF), None, y, 64, 2, h, w, 64, 64, 3, 1, 1.0)
        assert band_untouched(band) and bool((y == SENTINEL).all())
        k = _fwd("auto", "bf16", 2, h, w, 64, 0, 64, seed=5, expect="")
        assert not k.startswith("tapgemm_pp") and not k.startswith("tapgemm_wreg"), k
    else:
        _fwd("wreg", "bf16", 2, h, w, 64, 0, 64, seed=5, expect="tapgemm_wreg16_bf16_kernel<2, true>")


@pytest.mark.parametrize("h,w,cin,cout,sym", [
    (32, 16, 16, 16, "tapgemm_wreg_f32_kernel<1, 1, false>"),        # 32-row patches: the rule (hi % 32) holds on the height only
    (16, 32, 16, 32, "tapgemm_wreg_f32_kernel<1, 2, false>"),        # 16-row patches, both orientations
    (32, 16, 16, 32, "tapgemm_wreg_f32_kernel<1, 2, false>"),
    (64, 16, 32, 16, "tapgemm_wreg_f32_kernel<2, 1, false>"),        # two 32-row patches above each other, K = 32
])
def test_wreg_f32_narrow_rect(h, w, cin, cout, sym):
    for variant in ("wreg", "auto"):
        _fwd(variant, "f32", 2, h, w, cin, 0, cout, seed=6, expect=sym, in_stats=False, slope=0.0)


def test_wreg_f32_narrow_refuses_the_transpose():
    """16 output channels need 32-row patches: 16 x 32 (the rule fails on the height, holds on the width) is refused when forced and
    computed by another kernel under the automatic choice"""
    from shmgan_amd._lib import ShmError
    ops = _ops()
    n, h, w, cin, cout = 2, 16, 32, 16, 16
    y, band = _guarded((n, h, w, cout))
    ops.set_tuning("tapgemm.variant", "wreg")
    with pytest.raises(ShmError):
        ops.conv2d_fwd(torch.zeros((n, h, w, cin), device="cuda"), None, 0, cin, 0, torch.zeros(9 * cout * cin, device="cuda"), None, y, cout, n, h, w, cin, cout, 3, 1, 0.0)
    assert band_untouched(band) and bool((y == SENTINEL).all())
    k = _fwd("auto", "f32", n, h, w, cin, 0, cout, seed=6, expect="", in_stats=False, slope=0.0)
    assert not k.startswith("tapgemm_wreg"), k


# =====================================================================================================================
# input gradients
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("variant", HALO + ["dma128x128", "dma64x128", "dma128x64", "dma64x64", "dma256x64", "dma256x128", "wreg"])
@pytest.mark.parametrize("h,w", _both((16, 32)))
def test_dgrad_s1_forced_variant_rect(variant, dt, h, w):
    """split destination (upsampled, skip); bf16 "wreg": 16 x 32 is whole 8 x 32 patches (ping-pong kernel), 32 x 16 is not"""
    ops = _ops()
    rng = np.random.default_rng(7)
    n, c1, c2, cout = 2, 64, 64, 64
    cin = c1 + c2
    wt = rng.standard_normal((3, 3, cin, cout)) * 0.1
    dy = rng.standard_normal((n, h, w, cout))
    xt = torch.zeros(n, cin, h, w, dtype=torch.float64, requires_grad=True)
    ref, = torch.autograd.grad(st.conv2d_same(xt, t64(_rnd(wt, dt)), 1), xt, nchw(_rnd(dy, dt)))
    ref = nhwc(ref)
    d1, b1 = _guarded((n, h, w, c1), _adt(dt))
    d2, b2 = _guarded((n, h, w, c2), _adt(dt))
    ops.set_tuning("tapgemm.variant", variant)
    ops.conv2d_dgrad(_dev(dy, dt), cout, _dev(wt, dt), d1, d2, c1, c1, c2, n, h, w, cin, cout, 3, 1)
    assert ops.last_kernel() == _sym(variant, dt, epi=False, hw=(h, w)), ops.last_kernel()
    if variant == "wreg" and dt == "bf16":    # the same product with the gradient signal leaving in fp32 (SHM_BF16_GF32)
        f1, g1 = _guarded((n, h, w, c1))
        f2, g2 = _guarded((n, h, w, c2))
        ops.conv2d_dgrad(_dev(dy, dt), cout, _dev(wt, dt), f1, f2, c1, c1, c2, n, h, w, cin, cout, 3, 1)
        assert ops.last_kernel() == "tapgemm_wreg_kernel<float, 2>"
        assert rel_l2(host(f1), ref[..., :c1]) < 1e-4 and rel_l2(host(f2), ref[..., c1:]) < 1e-4
        eb.hold_dgrad([host(f1), host(f2)], _rnd(dy, dt), _rnd(wt, dt), 1, ref, "f32", "dgrad gf32 tapgemm_wreg_kernel")
        assert band_untouched(g1) and band_untouched(g2)
    assert rect_close(host(d1.float()), ref[..., :c1], dt) and rect_close(host(d2.float()), ref[..., c1:], dt)
    eb.hold_dgrad([host(d1.float()), host(d2.float())], _rnd(dy, dt), _rnd(wt, dt), 1, ref, dt, "dgrad " + _sym(variant, dt, epi=False, hw=(h, w)).split("<")[0])
    assert band_untouched(b1) and band_untouched(b2)


def _dgrad_s2(variant, dt, n, h, w, cin, cout, seed=8):
    """dx [n, h, w, cin] of a stride-2 3x3 layer from dy [n, h / 2, w / 2, cout]"""
    ops = _ops()
    rng = np.random.default_rng(seed)
    wt = rng.standard_normal((3, 3, cin, cout)) * 0.1
    dy = rng.standard_normal((n, h // 2, w // 2, cout))
    xt = torch.zeros(n, cin, h, w, dtype=torch.float64, requires_grad=True)
    ref, = torch.autograd.grad(st.conv2d_same(xt, t64(_rnd(wt, dt)), 2), xt, nchw(_rnd(dy, dt)))
    dx, band = _guarded((n, h, w, cin), _adt(dt))
    ops.set_tuning("tapgemm.variant", variant)
    ops.conv2d_dgrad(_dev(dy, dt), cout, _dev(wt, dt), dx, None, cin, cin, 0, n, h, w, cin, cout, 3, 2)
    assert ops.last_kernel() == _sym(variant, dt), ops.last_kernel()
    assert rect_close(host(dx.float()), nhwc(ref), dt), rel_l2(host(dx.float()), nhwc(ref))
    eb.hold_dgrad(host(dx.float()), _rnd(dy, dt), _rnd(wt, dt), 2, nhwc(ref), dt, "dgrad s2 " + _sym(variant, dt).split("<")[0])
    assert band_untouched(band)


def _transpose(variant, dt, n, hi, wi, ci, co, seed=8):
    """Conv2DTranspose(3x3, s2) + bias + LeakyReLU of x [n, hi, wi, ci]"""
    ops = _ops()
    rng = np.random.default_rng(seed + 1)
    x = rng.standard_normal((n, hi, wi, ci))
    wt = rng.standard_normal((3, 3, co, ci)) * 0.1
    b = rng.standard_normal(co)
    r = _lrelu(nhwc(st.conv2d_transpose_same(nchw(_rnd(x, dt)), t64(_rnd(wt, dt)))) + b)
    y, band = _guarded((n, 2 * hi, 2 * wi, co), _adt(dt))
    ops.set_tuning("tapgemm.variant", variant)
    ops.conv2d_transpose_fwd(_dev(x, dt), ci, _dev(wt, dt), _f32(b), y, co, n, hi, wi, ci, co, 0.2)
    assert ops.last_kernel() == _sym(variant, dt), ops.last_kernel()
    assert rect_close(host(y.float()), r, dt), rel_l2(host(y.float()), r)
    eb.hold_transpose(host(y.float()), _rnd(x, dt), _rnd(wt, dt), b, r, dt, "transpose " + _sym(variant, dt).split("<")[0])
    assert band_untouched(band)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("variant", ["dma128x128", "dma64x128", "dma128x64", "dma64x64", "dma256x64", "dma256x128", "dma128x128_bk32", "phase4"])
@pytest.mark.parametrize("flip", [False, True])
def test_dgrad_s2_and_transpose_forced_variant_rect(variant, dt, flip):
    """the four-phase launches: dx 32 x 64 / 64 x 32, Conv2DTranspose of 16 x 32 / 32 x 16"""
    h, w = (64, 32) if flip else (32, 64)
    _dgrad_s2(variant, dt, 2, h, w, 64, 128)
    _transpose(variant, dt, 2, h // 2, w // 2, 64, 64 if variant == "phase4" else 96)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("h,w", _both((16, 48)))
def test_phase4_one_patch_by_three(dt, h, w):
    """the fused four-phase kernel on a 16 x 48 input: one 16 x 16 patch on one axis, an interior patch with two neighbours on the other"""
    _dgrad_s2("phase4", dt, 2, 2 * h, 2 * w, 64, 64, seed=18)
    _transpose("phase4", dt, 2, h, w, 64, 128, seed=18)


def test_dgrad_s2_refuses_an_odd_size():
    from shmgan_amd._lib import ShmError
    ops = _ops()
    for h, w in ((9, 16), (16, 9)):
        dx, band = _guarded((2, h, w, 32))
        dy = torch.zeros((2, -(-h // 2), -(-w // 2), 64), device="cuda")
        with pytest.raises(ShmError):
            ops.conv2d_dgrad(dy, 64, torch.zeros((3, 3, 32, 64), device="cuda"), dx, None, 32, 32, 0, 2, h, w, 32, 64, 3, 2)
        assert bool((dx == SENTINEL).all()) and band_untouched(band)          # before any launch


# =====================================================================================================================
# gsum epilogues (test_gsum_gpu.py): the gradient bit-identical to the plain entry point's, the slot sums against float64
def _dgrad_gsum(variant, dt, n, h, w, cin, cout, n1, which=(True, True)):
    ops = _ops()
    rng = np.random.default_rng(7)
    adt = _adt(dt)
    dy = _dev(rng.standard_normal((n, h, w, cout)), dt)
    wt = _dev(rng.standard_normal((3, 3, cin, cout)) * 0.1, dt)
    split = 0 < n1 < cin
    c0, c1 = (n1, cin - n1) if split else (cin, 0)
    aux0 = _dev(rng.standard_normal((n, h, w, c0)), dt)
    aux1 = _dev(rng.standard_normal((n, h, w, c1)), dt) if split else None
    outs = []
    for use_gsum in (False, True):
        dx, b0 = _guarded((n, h, w, c0), adt)
        dx2, b1 = _guarded((n, h, w, c1), adt) if split else (None, None)
        red0 = torch.zeros(ops.GSUM_SLOTS * n * c0 * 2, dtype=torch.float64, device="cuda")
        red1 = torch.zeros(ops.GSUM_SLOTS * n * c1 * 2, dtype=torch.float64, device="cuda") if split else None
        ops.set_tuning("tapgemm.variant", variant)
        if variant == "wreg" and dt == "bf16":              # the plain call on the kernel the gsum form lives in (see test_gsum_gpu._dgrad_case)
            ops.set_tuning("tapgemm.wreg16", 0)
        g0 = (aux0, c0, red0) if (use_gsum and which[0]) else None
        g1 = (aux1, c1, red1) if (use_gsum and split and which[1]) else None
        ops.conv2d_dgrad(dy, cout, wt, dx, dx2, n1 if split else 0, c0, c1, n, h, w, cin, cout, 3, 1, gsum=g0, gsum2=g1)
        torch.cuda.synchronize()
        assert band_untouched(b0) and (b1 is None or band_untouched(b1))
        outs.append((dx, dx2, red0, red1, g0, g1, ops.last_kernel()))
    (dxa, dx2a, *_), (dxb, dx2b, red0, red1, g0, g1, kern) = outs
    assert torch.equal(dxa, dxb) and (not split or torch.equal(dx2a, dx2b)), kern
    if g0 is not None:
        _check_sums(red0, dxb, aux0, dt)
    if g1 is not None:
        _check_sums(red1, dx2b, aux1, dt)
    # ... and the gradient itself against float64 (the square module leaves that to test_variants_gpu.py)
    xt = torch.zeros(n, cin, h, w, dtype=torch.float64, requires_grad=True)
    ref, = torch.autograd.grad(st.conv2d_same(xt, wt.double().cpu(), 1), xt, dy.double().cpu().permute(0, 3, 1, 2))
    got = host(dxb.float()) if not split else np.concatenate([host(dxb.float()), host(dx2b.float())], -1)
    assert rect_close(got, nhwc(ref), dt), (kern, rel_l2(got, nhwc(ref)))
    eb.hold_dgrad([host(dxb.float())] + ([host(dx2b.float())] if split else []), host(dy.float()), host(wt.float()), 1, nhwc(ref), dt, "dgrad gsum " + kern.split("<")[0])
    return kern


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("variant", ["halo128_st", "halo64_st", "dma128x128", "wreg"])
@pytest.mark.parametrize("h,w", _both((16, 32)))
@pytest.mark.parametrize("cin,cout,n1,which", [(64, 64, 0, (True, True)), (128, 64, 64, (False, True)), (128, 64, 64, (True, True))])
def test_dgrad_gsum_rect(variant, dt, h, w, cin, cout, n1, which):
    kern = _dgrad_gsum(variant, dt, 2, h, w, cin, cout, n1, which)
    if variant == "wreg":
        assert kern.startswith("tapgemm_wreg") and kern.endswith("true>"), kern


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("variant", ["auto", "dma128x128"])
@pytest.mark.parametrize("h,w", _both((32, 64)))
def test_fwd_gsum_stride2_rect(variant, dt, h, w):
    ops = _ops()
    rng = np.random.default_rng(9)
    n, cin, cout = 2, 64, 128
    adt = _adt(dt)
    x = rng.standard_normal((n, h, w, cin))
    wt = rng.standard_normal((3, 3, cin, cout)) * 0.1
    aux = _dev(rng.standard_normal((n, h // 2, w // 2, cout)), dt)
    ya, ba = _guarded((n, h // 2, w // 2, cout), adt)
    yb, bb = _guarded((n, h // 2, w // 2, cout), adt)
    red = torch.zeros(ops.GSUM_SLOTS * n * cout * 2, dtype=torch.float64, device="cuda")
    ops.set_tuning("tapgemm.variant", variant)
    ops.conv2d_fwd(_dev(x, dt), None, 0, cin, 0, _wk(wt, cin, dt), None, ya, cout, n, h, w, cin, cout, 3, 2, 1.0)
    ops.conv2d_fwd(_dev(x, dt), None, 0, cin, 0, _wk(wt, cin, dt), None, yb, cout, n, h, w, cin, cout, 3, 2, 1.0, gsum=(aux, cout, red))
    torch.cuda.synchronize()
    if variant != "auto":
        assert ops.last_kernel() == _sym(variant, dt), ops.last_kernel()
    assert torch.equal(ya, yb) and band_untouched(ba) and band_untouched(bb)
    _check_sums(red, yb, aux, dt)
    ref = conv_ref(_rnd(x, dt), _rnd(wt, dt), 2)
    assert rect_close(host(yb.float()), ref, dt)
    eb.hold_fwd(host(yb.float()), _rnd(x, dt), _rnd(wt, dt), None, 2, ref, dt, "fwd gsum s2 " + ops.last_kernel().split("<")[0])


# =====================================================================================================================
# weight gradients
def _wgrad_ref(x, dy, cin, cout, s, dt, k=3):
    wt = torch.zeros(k, k, cin, cout, dtype=torch.float64, requires_grad=True)
    ref, = torch.autograd.grad(st.conv2d_same(nchw(_rnd(x, dt)), wt, s), wt, nchw(_rnd(dy, dt)))
    return ref.numpy()


def _wgrad_run(xa, xb, c1, dyd, n, h, w, cin, ld, cout, s, ref, tol, expect=None, k=3):
    """plain, then accumulate; the split-K workspace starts as NaN (every slab element a block owns must be written).  Returns (dw, kernel)."""
    ops = _ops()
    ho, wo = -(-h // s), -(-w // s)
    ws = torch.full((ops.conv2d_wgrad_workspace(n, ho, wo, cin, cout, k) // 4 + 1024,), float("nan"), device="cuda")
    dw, band = _guarded((k, k, cin, cout), fill=3.0)
    ldx, ldx2 = (ld, 0) if xb is None else (xa.shape[-1], xb.shape[-1])
    ops.conv2d_wgrad(xa, xb, c1, ldx, ldx2, dyd, cout, dw, n, h, w, cin, ld, cout, k, s, 0, ws)
    kern = ops.last_kernel()
    if expect is not None:
        assert kern == expect if isinstance(expect, str) else expect(kern), kern
    got = host(dw)
    assert rel_l2(got, ref) < tol, (kern, rel_l2(got, ref))
    bound = "x3" not in kern                     # ("wgrad.f32_split": test_x3_gpu.py argues per element on its own terms)
    if bound:
        x64 = host(xa.float())[..., :cin] if xb is None else np.concatenate([host(xa.float()), host(xb.float())], -1)
        dt = "bf16" if dyd.dtype == BF else "f32"
        eb.hold_wgrad(got, x64, host(dyd.float()), s, ref, "wgrad " + ("s2 " if s == 2 else "") + kern.split("<")[0], dt, k)
    ws.fill_(float("nan"))
    ops.conv2d_wgrad(xa, xb, c1, ldx, ldx2, dyd, cout, dw, n, h, w, cin, ld, cout, k, s, 1, ws)
    assert rel_l2(host(dw), 2 * ref) < tol, kern
    if bound:
        eb.hold_wgrad(host(dw), x64, host(dyd.float()), s, ref, "wgrad accumulate " + ("s2 " if s == 2 else "") + kern.split("<")[0], dt, k, before=got)
    assert band_untouched(band, 3.0), kern
    return got, kern


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("wv", [0, 1, 2])
@pytest.mark.parametrize("h,w", _both((16, 32)))
@pytest.mark.parametrize("n,cin,cout,blocks", [(2, 64, 64, 0), (3, 64, 128, 7), (3, 10, 64, 5)])
def test_wgrad_forced_variant_rect(dt, wv, h, w, n, cin, cout, blocks):
    """generic / halo / thin-input kernels; "wgrad.blocks" 7 and 5 over 3 images: blocks that cross image boundaries"""
    ops = _ops()
    rng = np.random.default_rng(9)
    pitch = 32 if dt == "bf16" else 16
    ld = (cin + pitch - 1) // pitch * pitch
    x = pad_c(rng.standard_normal((n, h, w, cin)), ld)
    dy = rng.standard_normal((n, h, w, cout))
    ref = _wgrad_ref(x[..., :cin], dy, cin, cout, 1, dt)
    ops.set_tuning("wgrad.variant", wv)
    ops.set_tuning("wgrad.blocks", blocks)
    ops.set_tuning("wgrad.bf16_wide", 4)
    for rows in ((0, 2) if dt == "bf16" and wv != 1 else (0,)):
        ops.set_tuning("wgrad.bf16_rows", rows)
        wide = dt == "bf16" and cout >= 128 and rows == 0
        if wv == 1:
            expect = lambda k: k.startswith("wgrad_kernel<") or k.startswith("wgrad_bf16_kernel<")
        elif wv == 2:
            expect = "wgrad_halo8_bf16_kernel<0>" if wide else "wgrad_halo_kernel" if dt == "f32" else f"wgrad_halo_bf16_kernel<{rows or 4}>"
        else:
            expect = None
        _wgrad_run(_dev(x, dt), None, 0, _dev(dy, dt), n, h, w, cin, ld, cout, 1, ref, WTOL[dt], expect)
        if wide and wv == 2:                   # ... and the four-wave kernel on the same shape
            ops.set_tuning("wgrad.bf16_wide", 1)
            _wgrad_run(_dev(x, dt), None, 0, _dev(dy, dt), n, h, w, cin, ld, cout, 1, ref, WTOL[dt], "wgrad_halo_bf16_kernel<4>")
            ops.set_tuning("wgrad.bf16_wide", 4)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("h,w", _both((16, 32)))
def test_wgrad_concat_source_rect(dt, h, w):
    rng = np.random.default_rng(10)
    n, c1, c2, cout = 2, 64, 128, 64
    xa, xb, dy = rng.standard_normal((n, h, w, c1)), rng.standard_normal((n, h, w, c2)), rng.standard_normal((n, h, w, cout))
    ref = _wgrad_ref(np.concatenate([xa, xb], -1), dy, c1 + c2, cout, 1, dt)
    _wgrad_run(_dev(xa, dt), _dev(xb, dt), c1, _dev(dy, dt), n, h, w, c1 + c2, c1 + c2, cout, 1, ref, WTOL[dt])


@pytest.mark.parametrize("h,w", _both((32, 64)))
@pytest.mark.parametrize("n,cin,cout,blocks", [(2, 64, 128, 0), (3, 64, 64, 5)])
def test_wgrad_stride2_halo_rect(h, w, n, cin, cout, blocks):
    """fp32: 2 x 8 output patches, 5 x 17 input halo, against the generic kernel ("wgrad.variant" 3) and float64"""
    ops = _ops()
    rng = np.random.default_rng(31)
    x = rng.standard_normal((n, h, w, cin))
    dy = rng.standard_normal((n, h // 2, w // 2, cout))
    ref = _wgrad_ref(x, dy, cin, cout, 2, "f32")
    got = {}
    for wv in (0, 3):
        ops.set_tuning("wgrad.variant", wv)
        ops.set_tuning("wgrad.blocks", blocks)
        got[wv], _ = _wgrad_run(_dev(x, "f32"), None, 0, _dev(dy, "f32"), n, h, w, cin, cin, cout, 2, ref, 1e-5,
                                "wgrad_halo_kernel<0, true>" if wv == 0 else "wgrad_kernel<9, false>")
    assert rel_l2(got[0], got[3]) < 1e-5


@pytest.mark.parametrize("h,w,mode", [(32, 64, 1), (64, 32, 1), (16, 64, 1), (64, 16, 2)])
@pytest.mark.parametrize("n,cin,cout,blocks", [(2, 64, 128, 0), (3, 96, 192, 5)])
def test_wgrad_stride2_bf16_wide_rect(h, w, mode, n, cin, cout, blocks):
    """the eight-wave block switches on the number of OUTPUT COLUMNS: 16 x 64 has 32 of them (stages of 2 x 16, kernel <1>), 64 x 16 has 8
    (stages of 4 x 8, kernel <2>)"""
    ops = _ops()
    rng = np.random.default_rng(41)
    x = rng.standard_normal((n, h, w, cin))
    dy = rng.standard_normal((n, h // 2, w // 2, cout))
    ref = _wgrad_ref(x, dy, cin, cout, 2, "bf16")
    got = {}
    for wide in (0, 1):
        ops.set_tuning("wgrad.bf16_wide", wide)
        ops.set_tuning("wgrad.blocks", blocks)
        got[wide], _ = _wgrad_run(_dev(x, "bf16"), None, 0, _dev(dy, "bf16"), n, h, w, cin, cin, cout, 2, ref, 1e-4,
                                  f"wgrad_halo8_bf16_kernel<{mode}>" if wide == 0 else "wgrad_bf16_kernel<9, false>")
    assert rel_l2(got[0], got[1]) < 1e-5


@pytest.mark.parametrize("h,w,s", [(16, 32, 1), (32, 16, 1), (32, 64, 2), (64, 32, 2)])
def test_x3_wgrad_rect(h, w, s):
    """"wgrad.f32_split": the six-product kernel on 64-channel maps of two patch columns / one patch column (test_x3_gpu.py has 8 x 32, 6 x 48,
    32 x 16 and 16 x 64 of other channel counts), against float64 and the exact kernel"""
    ops = _ops()
    rng = np.random.default_rng(60)
    n, cin, cout = 2, 64, 64
    x = rng.standard_normal((n, h, w, cin)) * np.exp(rng.standard_normal((n, h, w, cin)))
    dy = rng.standard_normal((n, h // s, w // s, cout))
    ref = _wgrad_ref(x, dy, cin, cout, s, "f32")
    ops.set_tuning("wgrad.f32_split", 1)
    g3, _ = _wgrad_run(_dev(x, "f32"), None, 0, _dev(dy, "f32"), n, h, w, cin, cin, cout, s, ref, 1e-5,
                       "wgrad_halo_x3_kernel<4>" if s == 1 else "wgrad_halo_x3_kernel<2, false, true>")
    ops.set_tuning("wgrad.f32_split", 0)
    g1, _ = _wgrad_run(_dev(x, "f32"), None, 0, _dev(dy, "f32"), n, h, w, cin, cin, cout, s, ref, 1e-5,
                       "wgrad_halo_kernel" if s == 1 else "wgrad_halo_kernel<0, true>")
    assert rel_l2(g3, ref) < 4 * rel_l2(g1, ref) + 1e-7


@pytest.mark.parametrize("h,w,cout,x3", [(16, 32, 128, True), (32, 16, 128, True), (32, 16, 64, True), (16, 32, 64, False)])
def test_x3_forward_rect(h, w, cout, x3):
    """"conv.f32_split" (conv_fwd_x3.hip): 128 output channels on 16 x 16 patches both ways; 64 output channels take 32 x 16-pixel blocks,
    so the map HEIGHT must be a multiple of 32: 32 x 16 runs, 16 x 32 stays on the exact kernel"""
    ops = _ops()
    rng = np.random.default_rng(70)
    n, cin = 2, 64
    x = rng.standard_normal((n, h, w, cin)) * np.exp(rng.standard_normal((n, h, w, cin)))
    wt = rng.standard_normal((3, 3, cin, cout)) * 0.1
    b = rng.standard_normal(cout)
    ref = _lrelu(conv_ref(_rnd(x, "f32"), _rnd(wt, "f32"), 1) + _rnd(b, "f32"))
    ops.set_tuning("tapgemm.variant", "halo128_st")
    outs = {}
    for split in (1, 0):
        ops.set_tuning("conv.f32_split", split)
        y, band = _guarded((n, h, w, cout), fill=5.0)
        stats = torch.zeros(n * cout * 2, dtype=torch.float64, device="cuda")
        scr = torch.zeros(ops.STATS_SLOTS * n * cout * 2, dtype=torch.float64, device="cuda")
        ops.conv2d_in_fwd(_dev(x, "f32"), None, 0, cin, 0, _wk(wt, cin, "f32"), _f32(b), y, cout, n, h, w, cin, cout, 3, 1, 0.2, stats, 1e-6, scratch=scr)
        kern = ops.last_kernel()
        torch.cuda.synchronize()
        assert float(scr.abs().max()) == 0.0 and band_untouched(band, 5.0)
        outs[split] = (host(y), stats.clone(), kern)
    (y3, s3, k3), (y1, s1, k1) = outs[1], outs[0]
    assert "x3" not in k1, k1
    assert k3 == (f"tapgemm_halo_x3_kernel<false, {128 if cout > 64 else 64}>" if x3 else k1), (k3, k1)
    e3, e1 = rel_l2(y3, ref), rel_l2(y1, ref)
    assert e3 < 1e-5 and e1 < 1e-5 and e3 < 4 * e1 + 1e-7, (e3, e1)
    assert rel_l2(host(s3), host(s1)) < 1e-5
    _check_stats(s3, y3, n, cout, "f32")


# =====================================================================================================================
# InstanceNorm folded into its consumers (test_norm_fold_gpu.py)
EPS = 1e-6
IN_WHERE = {"kind": "in"}


def _block(rng, n, h, w, c, dt):
    """an un-normalised activation, its statistics, beta, its table and its normalised tensor"""
    ops = _ops()
    a = _dev(rng.standard_normal((n, h, w, c)) * rng.uniform(0.5, 2.0, (n, 1, 1, c)) + rng.uniform(-1, 1, (n, 1, 1, c)), dt)
    beta = _f32(rng.uniform(-0.5, 0.5, c))
    stats = torch.zeros(n * c * 2, dtype=torch.float64, device="cuda")
    ops.in_stats(a, c, stats, n, h * w, c, EPS)
    nt = torch.full((n, 4, c), 9.0, dtype=torch.float32, device="cuda")
    ops.in_norm_table(stats, beta, nt, n, c)
    ahat = torch.empty_like(a)
    ops.in_apply(a, c, stats, beta, ahat, c, n, h * w, c)
    return a, nt, ahat


def _in_fwd(x, wk, bias, n, h, w, cin, cout, dt, **kw):
    ops = _ops()
    y, band = _guarded((n, h, w, cout), _adt(dt))
    stats = torch.zeros(n * cout * 2, dtype=torch.float64, device="cuda")
    scr = torch.zeros(ops.STATS_SLOTS * n * cout * 2, dtype=torch.float64, device="cuda")
    ops.conv2d_in_fwd(x, None, 0, cin, 0, wk, bias, y, cout, n, h, w, cin, cout, 3, 1, 0.2, stats, EPS, scratch=scr, **kw)
    torch.cuda.synchronize()
    assert float(scr.abs().max()) == 0.0 and band_untouched(band)
    return y, stats, ops.last_kernel()


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("variant,cin,cout", [("wreg", 64, 64), ("halo64_st", 128, 64), ("halo128_st", 128, 128)])
@pytest.mark.parametrize("h,w", _both((16, 32)))
def test_forward_norm_fold_rect(variant, cin, cout, h, w, dt):
    """SHM_NORM_EXACT: bit-identical to apply-then-conv; SHM_NORM_SCALED: against that two-pass path at test_norm_fold_gpu._close's tolerance,
    border rows and columns on their own; and the two-pass result itself against float64"""
    ops = _ops()
    ops.set_tuning("tapgemm.wreg16", 0)          # the plain call on the kernel the folding forms live in (test_norm_fold_gpu.py's fixture)
    rng = np.random.default_rng(11)
    n = 2
    a, nt, ahat = _block(rng, n, h, w, cin, dt)
    wk, bias = _dev(rng.standard_normal((9, cout, cin)) * 0.1, dt), _f32(rng.standard_normal(cout) * 0.1)
    ops.set_tuning("tapgemm.variant", variant)
    y0, s0, k0 = _in_fwd(ahat, wk, bias, n, h, w, cin, cout, dt)
    w_hwio = wk.double().cpu().numpy().reshape(3, 3, cout, cin).transpose(0, 1, 3, 2)
    ref = _lrelu(conv_ref(host(ahat.float()), w_hwio, 1) + host(bias))
    assert rect_close(host(y0.float()), ref, dt), (k0, rel_l2(host(y0.float()), ref))
    y1, s1, k1 = _in_fwd(a, wk, bias, n, h, w, cin, cout, dt, nt_x=nt)
    assert k1 != k0 and k1.rstrip(">").endswith(", 1"), (k0, k1)
    assert torch.equal(y0, y1), (k1, float((y0.float() - y1.float()).abs().max()))
    assert torch.allclose(s0, s1, rtol=1e-6, atol=1e-7)
    wk_n = torch.empty((n,) + tuple(wk.shape), device="cuda", dtype=wk.dtype)
    bias_n = torch.empty((n, cout), device="cuda")
    ops.conv2d_norm_prepare(wk, bias, nt, cin, 0, wk_n, bias_n, n, cin, cout, 3)
    y2, _, k2 = _in_fwd(a, wk_n, bias_n, n, h, w, cin, cout, dt, nt_x=nt, norm_mode=ops.NORM_SCALED)
    assert k2.rstrip(">").endswith(", 2"), k2
    for sl in (np.s_[:], np.s_[:, 0], np.s_[:, -1], np.s_[:, :, 0], np.s_[:, :, -1]):
        g, r = y2[sl].double(), y0[sl].double()
        rel, worst = float((g - r).norm() / r.norm()), float((g - r).abs().max() / r.abs().max())
        assert (rel < 3e-6 and worst < 3e-5) if dt == "f32" else (rel < 1.5e-2 and worst < 8e-2), (k2, sl, rel, worst)


@pytest.mark.parametrize("dt,rows", [("f32", 0), ("bf16", 4), ("bf16", 2)])
@pytest.mark.parametrize("h,w", _both((16, 32)))
@pytest.mark.parametrize("n,cin,cout,blocks", [(2, 64, 64, 0), (3, 128, 64, 5)])
def test_wgrad_norm_fold_rect(dt, rows, h, w, n, cin, cout, blocks):
    """shm_conv2d_wgrad_norm: exact mode bit-identical to the gradient on the applied tensor, scaled mode (+ shm_conv2d_wgrad_norm_finish) to
    test_norm_fold_gpu.test_wgrad_scaled_mode's tolerance; the applied-tensor gradient itself against float64"""
    ops = _ops()
    rng = np.random.default_rng(13)
    a, nt, ahat = _block(rng, n, h, w, cin, dt)
    dy = _dev(rng.standard_normal((n, h, w, cout)) + 0.05, dt)
    if rows:
        ops.set_tuning("wgrad.bf16_rows", rows)
    if blocks:
        ops.set_tuning("wgrad.blocks", blocks)

    def run(x, ws_elems, **kw):
        ws = torch.full((ws_elems,), float("nan"), device="cuda")
        dw, band = _guarded((3, 3, cin, cout), fill=3.0)
        ops.conv2d_wgrad(x, None, 0, cin, 0, dy, cout, dw, n, h, w, cin, cin, cout, 3, 1, 0, ws, **kw)
        torch.cuda.synchronize()
        return dw, band, ops.last_kernel()

    nws = ops.conv2d_wgrad_workspace(n, h, w, cin, cout, 3) // 4 + 16
    dw0, b0, k0 = run(ahat, nws)
    wt = torch.zeros(3, 3, cin, cout, dtype=torch.float64, requires_grad=True)
    ref, = torch.autograd.grad(st.conv2d_same(ahat.double().cpu().permute(0, 3, 1, 2), wt, 1), wt, dy.double().cpu().permute(0, 3, 1, 2))
    assert rel_l2(host(dw0), ref.numpy()) < WTOL[dt], (k0, rel_l2(host(dw0), ref.numpy()))
    dw1, b1, k1 = run(a, nws, nt_x=nt)
    assert k1 != k0 and k1.rstrip(">").endswith("1"), (k0, k1)
    assert torch.equal(dw0, dw1), (k1, float((dw0 - dw1).abs().max()))
    dw2, b2, k2 = run(a, ops.conv2d_wgrad_norm_workspace(n, h, w, cin, cout, 3, a.dtype) // 4 + 16, nt_x=nt, norm_mode=ops.NORM_SCALED)
    assert k2.rstrip(">").endswith("2"), k2
    ops.conv2d_wgrad_norm_finish(dw2, nt, dy.double().sum(dim=(1, 2)).contiguous(), n, cin, 0, cin, cout, 3)
    torch.cuda.synchronize()
    rel = float((dw2.double() - dw0.double()).norm() / dw0.double().norm())
    assert rel < (2e-5 if dt == "f32" else 1.5e-2), (k2, rel)
    assert band_untouched(b0, 3.0) and band_untouched(b1, 3.0) and band_untouched(b2, 3.0)


# =====================================================================================================================
# InstanceNorm and pooling
def _in_ref(a64, beta):
    mean = a64.mean((1, 2), keepdims=True)
    inv = 1.0 / np.sqrt(a64.var((1, 2), keepdims=True) + 1e-6)
    return (a64 - mean) * inv + beta, mean, inv


def _pool(a):
    n, h, w, c = a.shape
    return a.reshape(n, h // 2, 2, w // 2, 2, c)


def _in_bwd_ref(a64, g, g2, slope=0.2):
    """float64 InstanceNorm + LeakyReLU backward on the stored activation a (sign(a) == sign(z))"""
    G = g if g2 is None else g + 0.25 * np.repeat(np.repeat(g2, 2, 1), 2, 2)
    return tn.leaky_relu_grad(a64, tn.instance_norm_bwd(a64, G), slope)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("h,w", _both((8, 32)))
def test_instance_norm_forward_and_pooling_rect(dt, h, w):
    """in_stats, in_apply, in_apply_pool, in_pool, avgpool2_fwd, maxpool2_fwd"""
    ops = _ops()
    rng = np.random.default_rng(9)
    n, c = 3, 64
    adt = _adt(dt)
    a = _dev(_lrelu(rng.standard_normal((n, h, w, c)) * 2 + 0.5), dt)
    a64 = host(a.float())
    beta = rng.standard_normal(c) * 0.02
    ref, mean, inv = _in_ref(a64, _rnd(beta, "f32"))
    stats = torch.empty(n * c * 2, dtype=torch.float64, device="cuda")
    ops.in_stats(a, c, stats, n, h * w, c, 1e-6)
    _check_stats(stats, a64, n, c, dt)
    out, bo = _guarded((n, h, w, c), adt)
    ops.in_apply(a, c, stats, _f32(beta), out, c, n, h * w, c)
    assert rect_close(host(out.float()), ref, dt) and band_untouched(bo)
    sth = host(stats)
    eb.note("in_apply", dt, eb.within(host(out.float()), *eb.in_apply_ref_tol(a64, sth, _rnd(beta, "f32"), dt), IN_WHERE, "in_apply"))
    o2, bo2 = _guarded((n, h, w, c), adt)
    p2, bp2 = _guarded((n, h // 2, w // 2, c), adt)
    ops.in_apply_pool(a, c, stats, _f32(beta), o2, c, p2, c, n, h, w, c)
    p1, bp1 = _guarded((n, h // 2, w // 2, c), adt)
    ops.avgpool2_fwd(out, c, p1, c, n, h, w, c)
    p3, bp3 = _guarded((n, h // 2, w // 2, c), adt)
    ops.in_pool(a, c, stats, _f32(beta), p3, c, n, h, w, c)
    torch.cuda.synchronize()
    assert torch.equal(out, o2) and torch.equal(p1, p2) and torch.equal(p2, p3)              # one pass == two passes, bit for bit
    assert rect_close(host(p1.float()), _pool(host(out.float())).mean(axis=(2, 4)), dt)
    eb.note("in_apply_pool", dt, eb.within(host(p1.float()), *eb.in_pool_ref_tol(host(out.float()), dt), IN_WHERE, "in_apply_pool / in_pool / avgpool2_fwd"))
    assert all(band_untouched(b) for b in (bo2, bp1, bp2, bp3))
    if dt == "f32":                              # SpecSeg's MaxPooling2D (fp32 only)
        pm, bm = _guarded((n, h // 2, w // 2, c))
        ops.maxpool2_fwd(out, c, pm, c, n, h, w, c)
        assert np.array_equal(host(pm), _pool(host(out)).max(axis=(2, 4))) and band_untouched(bm)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("h,w", _both((8, 32)))
def test_head_on_the_unnormalised_activation_rect(dt, h, w):
    """head_in_fwd / head_in_bwd against in_apply + head_fwd / head_bwd, as test_ops_gpu.test_head_on_the_unnormalised_activation"""
    ops = _ops()
    rng = np.random.default_rng(17)
    n, c = 3, 64
    adt = _adt(dt)
    ad = _dev(_lrelu(rng.standard_normal((n, h, w, c)) * 2 + 0.5), dt)
    beta, wv, b, g = _f32(rng.standard_normal(c) * 0.02), _f32(rng.standard_normal(c) * 0.1), _f32(np.array([0.3])), _f32(rng.standard_normal((n, h, w, 1)))
    stats = torch.empty(n * c * 2, dtype=torch.float64, device="cuda")
    ops.in_stats(ad, c, stats, n, h * w, c, 1e-6)
    ahat = torch.empty((n, h, w, c), device="cuda", dtype=adt)
    ops.in_apply(ad, c, stats, beta, ahat, c, n, h * w, c)
    res = []
    for fused in (False, True):
        y, by = _guarded((n, h, w, 1))
        dx, bx = _guarded((n, h, w, c), adt)
        dwa, dba = torch.zeros(c, dtype=torch.float64, device="cuda"), torch.zeros(1, dtype=torch.float64, device="cuda")
        red = torch.zeros(ops.LRELU_RED_SLOTS * (c + 1), dtype=torch.float64, device="cuda")
        if fused:
            ops.head_in_fwd(ad, c, stats, beta, wv, b, y, n, h * w, c, 0.2)
            ops.head_in_bwd(ad, c, stats, beta, wv, y, g, dx, c, dwa, dba, n, h * w, c, 0.2, red)
        else:
            ops.head_fwd(ahat, c, wv, b, y, n * h * w, c, 0.2)
            ops.head_bwd(ahat, c, wv, y, g, dx, c, dwa, dba, n * h * w, c, 0.2, red)
        torch.cuda.synchronize()
        assert band_untouched(by) and band_untouched(bx)
        res.append((host(y), host(dx.float()), host(dwa), host(dba)))
    (y0, dx0, w0, b0), (y1, dx1, w1, b1) = res
    yr = _lrelu(host(ahat.float()) @ host(wv)[:, None] + 0.3)
    assert rel_l2(y0, yr) < 1e-5
    if dt == "f32":
        assert np.array_equal(y0, y1) and np.array_equal(dx0, dx1)
        assert rel_l2(w1, w0) < 1e-6 and rel_l2(b1, b0) < 1e-6
    else:
        same = ((y0 > 0) == (y1 > 0))[..., 0]
        assert same.mean() > 0.98 and rel_l2(y1, y0) < 8e-3 and rel_l2(dx1[same], dx0[same]) < 8e-3


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("pooled", [False, True])
@pytest.mark.parametrize("h,w", _both((8, 32)))
def test_in_bwd_apply_rect(dt, pooled, h, w):
    """one pass with the producer's sums == shm_in_bwd's two passes (test_gsum_gpu.test_in_bwd_apply_matches_reduce_plus_apply), and those
    two passes against float64"""
    ops = _ops()
    rng = np.random.default_rng(11)
    n, c = 3, 64
    adt = _adt(dt)
    a = _dev(rng.standard_normal((n, h, w, c)) * 1.5 + 0.3, dt)
    g1 = _dev(rng.standard_normal((n, h, w, c)), dt)
    g2 = _dev(rng.standard_normal((n, h // 2, w // 2, c)), dt) if pooled else None
    beta = _f32(rng.normal(0, 0.02, c))
    stats = torch.empty(n * c * 2, dtype=torch.float64, device="cuda")
    ops.in_stats(a, c, stats, n, h * w, c, 1e-6)
    ahat = torch.empty_like(a)
    pool = torch.empty((n, h // 2, w // 2, c), device="cuda", dtype=adt)
    ops.in_apply_pool(a, c, stats, beta, ahat, c, pool, c, n, h, w, c)
    red3 = torch.zeros(n * c * 3, dtype=torch.float64, device="cuda")
    dz_ref, br = _guarded((n, h, w, c), adt)
    db_ref = torch.zeros(c, dtype=torch.float64, device="cuda")
    ops.in_bwd(g1, c, g2, c, a, c, stats, red3, dz_ref, c, db_ref, n, h, w, c, 0.2)
    r64 = _in_bwd_ref(host(a.float()), host(g1.float()), None if g2 is None else host(g2.float()))
    assert rect_close(host(dz_ref.float()), r64, dt), rel_l2(host(dz_ref.float()), r64)
    zr, ztol = eb.in_bwd_ref_tol(host(a.float()), host(stats), host(g1.float()), None if g2 is None else host(g2.float()), slope=0.2, dt=dt)
    eb.note("in_bwd two passes", dt, eb.within(host(dz_ref.float()), zr, ztol, IN_WHERE, "in_bwd"))
    eb.within(host(db_ref), zr.sum((0, 1, 2)), eb.in_sum_tol(zr, ztol, (0, 1, 2)), None, "in_bwd bias gradient")
    red = torch.zeros(ops.GSUM_SLOTS * n * c * 2, dtype=torch.float64, device="cuda")
    redp = torch.zeros_like(red) if pooled else None
    red.view(ops.GSUM_SLOTS, n, c, 2)[0].copy_(torch.from_numpy(_sums(g1, a)).cuda())
    if pooled:
        redp.view(ops.GSUM_SLOTS, n, c, 2)[0].copy_(torch.from_numpy(_sums(g2, pool)).cuda())
    dstage = torch.zeros(n * c, dtype=torch.float64, device="cuda")
    dz, bz = _guarded((n, h, w, c), adt)
    db = torch.zeros(c, dtype=torch.float64, device="cuda")
    ops.in_bwd_apply(g1, c, g2, c, a, c, stats, beta, red, redp, dstage, dz, c, db, n, h, w, c, 0.2)
    torch.cuda.synchronize()
    # (No per-element bound for this form: it takes m2 as inv (sum g a - mean sum g) + (sum g2 pooled - beta sum g2) from the producers' RAW sums,
    # a difference of large sums -- and of the bf16-rounded pooled tensor -- whose cancellation the counted roundings of elem_bound_ref.py do
    # not describe.  It is held to the two-pass result, which IS held element by element above.)
    tol = 2e-2 if dt == "bf16" and pooled else (4e-3 if dt == "bf16" else 2e-5)
    assert rel_l2(host(dz.float()), host(dz_ref.float())) < tol
    scale = host(dz_ref.float().abs()).reshape(-1, c).sum(0)
    assert (np.abs(host(db) - host(db_ref)) / scale).max() < (4e-3 if dt == "bf16" else 2e-6)
    assert float(red.abs().max()) == 0.0 and float(dstage.abs().max()) == 0.0 and (redp is None or float(redp.abs().max()) == 0.0)
    assert band_untouched(br) and band_untouched(bz)


@pytest.mark.parametrize("pool", [False, True])
@pytest.mark.parametrize("h,w", _both((16, 32)))
def test_in_bwd_forms_rect(pool, h, w):
    """512 pixels = two whole 256-pixel slices of a 64-channel group: two passes ("elem.fused_bwd" = 0), the one-pass kernel (automatic), the
    g-held kernel ("elem.fused_hold" = 2; it takes no pooled gradient: two passes), and fp32 (two passes), each against float64"""
    ops = _ops()
    rng = np.random.default_rng(7)
    n, c = 3, 64
    a = _dev(rng.standard_normal((n, h, w, c)) * rng.uniform(0.5, 2.0, (n, 1, 1, c)) + rng.uniform(-1, 1, (n, 1, 1, c)), "bf16")
    g = _dev(rng.standard_normal((n, h, w, c)) + 25.0, "bf16")          # a mean of 25: a sum that missed one block's part moves dz by ~10 %
    g2 = _dev(rng.standard_normal((n, h // 2, w // 2, c)), "bf16") if pool else None
    stats = torch.zeros(n * c * 2, dtype=torch.float64, device="cuda")
    ops.in_stats(a, c, stats, n, h * w, c, 1e-6)
    scratch = torch.zeros(ops.in_bwd_fused_doubles(n, h * w, c), dtype=torch.float64, device="cuda")
    ref = _in_bwd_ref(host(a.float()), host(g.float()), None if g2 is None else host(g2.float()))

    def run(a_, g_, g2_, fused):
        dz, band = _guarded((n, h, w, c), a_.dtype, fill=9.0)
        db = torch.zeros(c, dtype=torch.float64, device="cuda")
        red = torch.zeros(n * c * 3, dtype=torch.float64, device="cuda")
        ops.in_bwd(g_, c, g2_, c if g2_ is not None else 0, a_, c, stats, red, dz, c, db, n, h, w, c, 0.2, fused=fused)
        kern = ops.last_kernel()
        torch.cuda.synchronize()
        assert float(red.abs().max()) == 0.0 and band_untouched(band, 9.0), kern
        return host(dz.float()), host(db), kern

    rows = (n * (h * w * 64 // 16384) * 3 * c + 1) // 2
    forms = []
    for key, val, want in (("elem.fused_bwd", 0, None), ("elem.fused_bwd", 1, "in_bwd_fused8_kernel<true>" if pool else "in_bwd_fused8_kernel<false>"),
                           ("elem.fused_hold", 2, None if pool else "in_bwd_fusedg_kernel<2, 2, 4>")):
        ops.set_tuning("reset", 0)
        ops.set_tuning(key, val)
        z, b, k = run(a, g, g2, scratch)
        assert ("fused" not in k) if want is None else (k == want), (key, val, k)
        assert float((scratch[rows:].view(torch.int64) != 0).sum()) == 0
        assert rect_close(z, ref, "bf16"), (k, rel_l2(z, ref))
        assert np.abs(b - ref.sum((0, 1, 2))).max() <= 4e-3 * np.abs(ref).sum((0, 1, 2)).max(), k
        zr, ztol = eb.in_bwd_ref_tol(host(a.float()), host(stats), host(g.float()), None if g2 is None else host(g2.float()), slope=0.2, dt="bf16",
                                     partial=eb.in_bwd_partial(k, c))
        eb.note("in_bwd " + k.split("<")[0], "bf16", eb.within(z, zr, ztol, IN_WHERE, k))
        eb.within(b, zr.sum((0, 1, 2)), eb.in_sum_tol(zr, ztol, (0, 1, 2)), None, k + " bias gradient")
        forms.append(k)
    ops.set_tuning("reset", 0)
    af, gf, g2f = a.float(), g.float() - 25.0, None if g2 is None else g2.float()          # (zero-mean gradient, as test_ops_gpu.py holds fp32 to 1e-5)
    ref = _in_bwd_ref(host(af), host(gf), None if g2f is None else host(g2f))
    z, b, k = run(af, gf, g2f, None)
    assert "fused" not in k
    assert rect_close(z, ref, "f32"), rel_l2(z, ref)
    assert rel_l2(b, ref.sum((0, 1, 2))) < 1e-5
    zr, ztol = eb.in_bwd_ref_tol(host(af), host(stats), host(gf), None if g2f is None else host(g2f), slope=0.2, dt="f32")
    eb.note("in_bwd " + k.split("<")[0], "f32", eb.within(z, zr, ztol, IN_WHERE, k))
    eb.within(b, zr.sum((0, 1, 2)), eb.in_sum_tol(zr, ztol, (0, 1, 2)), None, k + " bias gradient")


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("h,w", _both((4, 8)))
def test_patch_fwd_bwd_rect(dt, h, w):
    ops = _ops()
    rng = np.random.default_rng(10)
    n, c = 3, 256
    x = _rnd(rng.standard_normal((n, h, w, c)), dt)
    wt = (rng.standard_normal((3, 3, c, 1)) * 0.05).astype(np.float32).astype(np.float64)
    g = rng.standard_normal((n, h, w, 1)).astype(np.float32).astype(np.float64)
    xt, wo = nchw(x).requires_grad_(True), t64(wt).requires_grad_(True)
    yt = F.leaky_relu(st.conv2d_same(xt, wo, 1), 0.2)
    rdx, rdw = torch.autograd.grad(yt, [xt, wo], nchw(g))
    yd, by = _guarded((n, h, w, 1))
    ops.patch_fwd(_dev(x, dt), c, _f32(wt), yd, n, h, w, c, 0.2)
    assert rel_l2(host(yd), nhwc(yt.detach())) < 1e-5 and band_untouched(by)
    dzp, bz = _guarded((n, h, w, 1))
    dx, bx = _guarded((n, h, w, c), _adt(dt))
    dw, bw = _guarded((3, 3, c, 1))
    ops.patch_bwd(_dev(x, dt), c, _f32(wt), yd, _f32(g), dzp, dx, c, dw, n, h, w, c, 0.2)
    assert rect_close(host(dx.float()), nhwc(rdx), dt) and rel_l2(host(dw), rdw.numpy()) < 1e-5
    assert band_untouched(bz) and band_untouched(bx) and band_untouched(bw)


@pytest.mark.parametrize("h,w", _both((8, 16)))
def test_conv2d_transpose2x2_fwd_rect(h, w):
    ops = _ops()
    rng = np.random.default_rng(21)
    n, cin, cout = 2, 32, 16
    x = rng.standard_normal((n, h, w, cin))
    wt = rng.standard_normal((2, 2, cout, cin)) * 0.1
    b = rng.standard_normal(cout)
    ref = nhwc(F.conv_transpose2d(nchw(_rnd(x, "f32")), t64(_rnd(wt, "f32")).permute(3, 2, 0, 1).contiguous(), stride=2)) + b
    y, band = _guarded((n, 2 * h, 2 * w, cout))
    ops.conv2d_transpose2x2_fwd(_f32(x), cin, _f32(wt), _f32(b), y, cout, n, h, w, cin, cout, 1.0)
    assert rel_l2(host(y), ref) < 1e-5 and band_untouched(band)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("h,w", _both((16, 32)))
def test_first_layer_dgrad_channel_sum_rect(dt, stride, h, w):
    ops = _ops()
    rng = np.random.default_rng(31)
    nk, batch, cin, c = 2, 2, 10, 32
    wt = rng.standard_normal((3, 3, cin, c)) * 0.1
    dz = _rnd(rng.standard_normal((nk * batch, h // stride, w // stride, c)), dt)
    masks = [0b10110, 0b01101]
    xt = torch.zeros(nk * batch, cin, h, w, dtype=torch.float64, requires_grad=True)
    full, = torch.autograd.grad(st.conv2d_same(xt, t64(_rnd(wt, "f32")), stride), xt, nchw(dz))
    full = nhwc(full).reshape(nk, batch, h, w, cin)
    ref = sum(full[k, ..., j] for k in range(nk) for j in range(cin) if (masks[k] >> j) & 1)
    weff = torch.empty((nk, 9, c), device="cuda")
    for k in range(nk):
        ops.sum_input_channels(_f32(wt), cin, c, masks[k], weff[k])
    out, band = _guarded((batch, h, w, 1), fill=0.5)
    ops.conv3x3_dgrad_sum1(_dev(dz, dt), c, weff, out, nk, batch, h, w, c, stride, 1)
    assert rel_l2(host(out)[..., 0] - 0.5, ref) < 1e-5
    ops.conv3x3_dgrad_sum1(_dev(dz, dt), c, weff, out, nk, batch, h, w, c, stride, 0)
    assert rel_l2(host(out)[..., 0], ref) < 1e-5 and band_untouched(band, 0.5)


# =====================================================================================================================
# odd and mixed-parity SAME padding: the generic kernels through the default dispatch
ODD = [(9, 16), (16, 9), (7, 5), (9, 9)]


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("h,w,s", [(h, w, 2) for h, w in ODD] + [(7, 5, 1), (5, 7, 1)])
def test_conv2d_fwd_odd_same_padding(dt, h, w, s):
    """stride 2: pad_before = 1 on an odd axis, 0 on an even one (9 x 16: pt = 1, pl = 0)"""
    if s == 2:
        assert (st._same_pads(h, 3, 2)[0], st._same_pads(w, 3, 2)[0]) == (h % 2, w % 2)
    _fwd("auto", dt, 2, h, w, 32, 0, 64, s=s, seed=40, expect="", small_stats=True)
    _fwd("auto", dt, 3, h, w, 32, 0, 64, s=s, seed=41, expect="", in_stats=False)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("h,w,s,cin", [(h, w, 2, 32) for h, w in ODD] + [(7, 5, 1, 32), (5, 7, 1, 32), (9, 16, 2, 3), (16, 9, 2, 3), (9, 16, 2, 10), (16, 9, 2, 10)])
def test_conv2d_wgrad_odd_same_padding(dt, h, w, s, cin):
    """... and the weight gradient; cin 3 and 10 are the thin first layers, whose packed kernel needs even maps of whole 16-column patches:
    these sizes must be left to a kernel that pads them correctly"""
    rng = np.random.default_rng(42)
    n, cout = 2, 64
    pitch = 32 if dt == "bf16" else 16
    ld = (cin + pitch - 1) // pitch * pitch
    x = pad_c(rng.standard_normal((n, h, w, cin)), ld)
    dy = rng.standard_normal((n, -(-h // s), -(-w // s), cout))
    ref = _wgrad_ref(x[..., :cin], dy, cin, cout, s, dt)
    assert np.allclose(ref, tn.conv2d_same_bwd(_rnd(x[..., :cin], dt), np.zeros((3, 3, cin, cout)), _rnd(dy, dt), s)[1])      # both oracles
    _wgrad_run(_dev(x, dt), None, 0, _dev(dy, dt), n, h, w, cin, ld, cout, s, ref, WTOL[dt])
