"""SHM_BF16_GF32 -- bf16 activations and weights, the gradient signal kept in fp32 (trainer grad_dtype="float32", bench.py --grad_dtype) -- forced
through every kernel family (gf32_ref.py: the case table and what each case must run).

The other modules force SHM_F32 and SHM_BF16 through every variant; this mode reached a handful of small shapes, so the <__bf16, float>
instantiations of the 128-wide and dynamic-tap halo blocks, of seven DMA tiles and of the four-phase kernel, and the branches that exist for it
alone (element-store gsum epilogues that read 2-byte aux and store 4-byte results), had never been launched by a test.

Method of test_variants_gpu.py / test_rect_gpu.py: the variant is forced through shm_set_tuning and shm_last_kernel() is asserted (expected symbols
end in <__bf16, float, ...>); the reference is float64 on the operands as the device holds them (bf16-rounded); every output is allocated with
test_rect_gpu._guarded and filled with the sentinel, so an overrun or an unwritten half is a failed assert.  Tolerance: relative L2 <= 1e-4
(test_bf16_gpu.TOL32) -- far below bf16's 4e-3, which is what makes a hidden bf16 round trip visible (test_gf32_cpu.py).

The gsum cases of this mode are the "gf32" rows of test_gsum_gpu.py, the shm_in_bwd dispatch rows those of test_in_bwd_plan_gpu.py and the whole
steps those of test_bf16_gpu.py.
"""
import numpy as np
import pytest
import torch

import elem_bound_ref as eb
import gf32_ref as R
from oracle import step_torch as st
from test_gsum_gpu import _sums
from test_rect_gpu import _both, _f32, _guarded, _in_bwd_ref
from test_variants_gpu import _dev, _rnd, _sym, _wk
from util import SENTINEL, band_untouched, conv_ref, host, nchw, nhwc, rel_l2, t64

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
TOL32 = R.TOL32
TOL_BF16 = 4e-3             # bf16 dz of the InstanceNorm / LeakyReLU backward: one output rounding (test_in_bwd_plan_gpu.TOL_BF16)


def _ops():
    from shmgan_amd import ops
    return ops


@pytest.fixture(autouse=True)
def _reset_tuning():
    yield
    _ops().set_tuning("reset", 0)


def _written(*outs):
    """no pixel of an output still holds the sentinel in every channel"""
    return not any(bool((o == SENTINEL).all(-1).any()) for o in outs)


def _refused(call, outs, bands):
    """A variant that refuses the mode does so before any launch: ShmError, outputs and guard bands untouched."""
    from shmgan_amd._lib import ShmError
    with pytest.raises(ShmError):
        call()
    torch.cuda.synchronize()
    assert all(bool((o == SENTINEL).all()) for o in outs) and all(band_untouched(b) for b in bands)


# =====================================================================================================================
# 1. unit-stride input gradients: fp32 dx (split into two destinations) from bf16 dy and w
_S1_REF = {}


def _s1_reference(n, h, w, cin, cout):
    """one float64 reference per shape, shared by the variants"""
    key = (n, h, w, cin, cout)
    if key not in _S1_REF:
        rng = np.random.default_rng(7)
        wt = rng.standard_normal((3, 3, cin, cout)) * 0.1
        dy = rng.standard_normal((n, h, w, cout))
        xt = torch.zeros(n, cin, h, w, dtype=torch.float64, requires_grad=True)
        ref, = torch.autograd.grad(st.conv2d_same(xt, t64(_rnd(wt, "bf16")), 1), xt, nchw(_rnd(dy, "bf16")))
        _S1_REF[key] = (wt, dy, nhwc(ref))
    return _S1_REF[key]


@pytest.mark.parametrize("case", R.cases(1, "dgrad"), ids=R.case_id)
def test_dgrad_s1_forced_variant_gf32(case):
    ops = _ops()
    variant, n, h, w, c1, c2, cout = (case[k] for k in ("variant", "n", "h", "w", "c1", "c2", "cout"))
    cin = c1 + c2
    wt, dy, ref = _s1_reference(n, h, w, cin, cout)
    d1, b1 = _guarded((n, h, w, c1))
    d2, b2 = _guarded((n, h, w, c2))
    ops.set_tuning("tapgemm.variant", variant)
    call = lambda: ops.conv2d_dgrad(_dev(dy, "bf16"), cout, _dev(wt, "bf16"), d1, d2, c1, c1, c2, n, h, w, cin, cout, 3, 1)
    if case["expect"] == "refuse":
        return _refused(call, (d1, d2), (b1, b2))
    call()
    torch.cuda.synchronize()
    kern = ops.last_kernel()
    # (32 x 32 is whole 8 x 32 patches: the bf16 launch takes the ping-pong kernel there; wreg16 / ping-pong store 2-byte elements, so this mode stays on the four-wave kernel)
    assert kern == _sym(variant, "bf16", cout / 32, epi=False, hw=(h, w), out="f32"), kern
    assert "<__bf16, float," in kern or kern == "tapgemm_wreg_kernel<float, 2>", kern
    assert band_untouched(b1) and band_untouched(b2) and _written(d1, d2), kern
    e1, e2 = rel_l2(host(d1), ref[..., :c1]), rel_l2(host(d2), ref[..., c1:])
    print(f"{kern}: rel-L2 {e1:.2e} {e2:.2e}")
    assert e1 < TOL32 and e2 < TOL32, (kern, e1, e2)
    eb.hold_dgrad([host(d1), host(d2)], _rnd(dy, "bf16"), _rnd(wt, "bf16"), 1, ref, "f32", "dgrad gf32 " + kern.split("<")[0])          # fp32 stores: u_out = u32


# =====================================================================================================================
# 2. stride-2 input gradients (four phases)
_S2_REF = {}


def _s2_reference(n, h, w, cin, cout):
    key = (n, h, w, cin, cout)
    if key not in _S2_REF:
        rng = np.random.default_rng(8)
        wt = rng.standard_normal((3, 3, cin, cout)) * 0.1
        dy = rng.standard_normal((n, h // 2, w // 2, cout))
        xt = torch.zeros(n, cin, h, w, dtype=torch.float64, requires_grad=True)
        ref, = torch.autograd.grad(st.conv2d_same(xt, t64(_rnd(wt, "bf16")), 2), xt, nchw(_rnd(dy, "bf16")))
        _S2_REF[key] = (wt, dy, nhwc(ref))
    return _S2_REF[key]


@pytest.mark.parametrize("case", R.cases(2, "dgrad_s2"), ids=R.case_id)
def test_dgrad_s2_forced_variant_gf32(case):
    ops = _ops()
    variant, n, h, w, cin, cout = (case[k] for k in ("variant", "n", "h", "w", "cin", "cout"))
    wt, dy, ref = _s2_reference(n, h, w, cin, cout)
    dx, band = _guarded((n, h, w, cin))
    ops.set_tuning("tapgemm.variant", variant)
    ops.set_tuning("tapgemm.phase4_min_blocks", 0)
    call = lambda: ops.conv2d_dgrad(_dev(dy, "bf16"), cout, _dev(wt, "bf16"), dx, None, cin, cin, 0, n, h, w, cin, cout, 3, 2)
    if case["expect"] == "refuse":
        return _refused(call, (dx,), (band,))
    call()
    torch.cuda.synchronize()
    kern = ops.last_kernel()
    assert kern == _sym(variant, "bf16", out="f32") and "<__bf16, float" in kern, kern
    assert band_untouched(band) and _written(dx), kern
    print(f"{kern}: rel-L2 {rel_l2(host(dx), ref):.2e}")
    assert rel_l2(host(dx), ref) < TOL32, (kern, rel_l2(host(dx), ref))
    eb.hold_dgrad(host(dx), _rnd(dy, "bf16"), _rnd(wt, "bf16"), 2, ref, "f32", "dgrad gf32 s2 " + kern.split("<")[0])


# =====================================================================================================================
# 3. the stride-2 forward form with fp32 output: what model.py runs as the input gradient of Conv2DTranspose
@pytest.mark.parametrize("case", R.cases(3, "fwd_s2"), ids=R.case_id)
def test_fwd_s2_fp32_output(case):
    ops = _ops()
    variant, n, h, w, cin, cout = (case[k] for k in ("variant", "n", "h", "w", "cin", "cout"))
    rng = np.random.default_rng(9)
    x = rng.standard_normal((n, h, w, cin))
    wt = rng.standard_normal((3, 3, cin, cout)) * 0.1
    ref = conv_ref(_rnd(x, "bf16"), _rnd(wt, "bf16"), 2)
    y, band = _guarded((n, h // 2, w // 2, cout))
    ops.set_tuning("tapgemm.variant", variant)
    ops.conv2d_fwd(_dev(x, "bf16"), None, 0, cin, 0, _wk(wt, cin, "bf16"), None, y, cout, n, h, w, cin, cout, 3, 2, 1.0)
    torch.cuda.synchronize()
    kern = ops.last_kernel()
    # (the automatic choice: 8 tiles of 64 x 128, "not even one per CU" -- the 64 x 64 DMA tile)
    assert kern == _sym("dma64x64" if variant == "auto" else variant, "bf16", out="f32"), kern
    assert band_untouched(band) and _written(y), kern
    print(f"{kern}: rel-L2 {rel_l2(host(y), ref):.2e}")
    assert rel_l2(host(y), ref) < TOL32, (kern, rel_l2(host(y), ref))
    eb.hold_fwd(host(y), _rnd(x, "bf16"), _rnd(wt, "bf16"), None, 2, ref, "f32", "fwd gf32 s2 " + kern.split("<")[0])


def test_in_fwd_refuses_the_mode():
    """fused forward statistics have no fp32-gradient form: the dtype error, before any launch"""
    from shmgan_amd import _lib
    ops = _ops()
    case, = R.cases(3, "in_fwd")
    n, h, w, cin, cout = (case[k] for k in ("n", "h", "w", "cin", "cout"))
    x = torch.zeros((n, h, w, cin), device="cuda", dtype=BF)
    wk = torch.zeros(9 * cout * cin, device="cuda", dtype=BF)
    y, band = _guarded((n, h // 2, w // 2, cout))
    stats = torch.full((n * cout * 2,), SENTINEL, dtype=torch.float64, device="cuda")
    scr = torch.zeros(ops.STATS_SLOTS * n * cout * 2, dtype=torch.float64, device="cuda")
    L = _lib.lib()
    for scratch in (scr, None):
        rc = L.shm_conv2d_in_fwd(x.data_ptr(), None, 0, cin, 0, wk.data_ptr(), None, y.data_ptr(), cout, n, h, w, cin, cout, 3, 2, 0.2, stats.data_ptr(),
                                 scratch.data_ptr() if scratch is not None else None, 1e-6, _lib.CONSTANTS["SHM_BF16_GF32"], None)
        torch.cuda.synchronize()
        assert rc == _lib.CONSTANTS["SHM_E_DTYPE"] and b"SHM_BF16_GF32 has no fused statistics" in L.shm_last_error(), (rc, L.shm_last_error())
        assert bool((y == SENTINEL).all()) and band_untouched(band) and float(scr.abs().max()) == 0.0
        # (without a scratch the entry point zeroes `stats` for the sums before it plans the launch)
        assert scratch is None or bool((stats == SENTINEL).all())


# =====================================================================================================================
# 5. shm_in_bwd_apply, the stand-alone gsum pass behind it, shm_lrelu_bwd
@pytest.mark.parametrize("pooled", [False, True])
@pytest.mark.parametrize("h,w", _both((8, 32)))
def test_in_bwd_apply_gf32(pooled, h, w):
    """as test_rect_gpu.test_in_bwd_apply_rect with fp32 g1 / g2 and bf16 a / dz: the sums come from the stand-alone reduce pass of this mode
    (gsum_reduce_kernel<float, __bf16>, through a dgrad of a 1 x 1 layer on a map without whole wave tiles) and must equal float64; one pass with
    them == shm_in_bwd's two passes, both against float64; every f64 scratch zero on return"""
    ops = _ops()
    rng = np.random.default_rng(11)
    n, c = 3, 64
    a = _dev(rng.standard_normal((n, h, w, c)) * 1.5 + 0.3, "bf16")
    g1 = _f32(rng.standard_normal((n, h, w, c)))
    g2 = _f32(rng.standard_normal((n, h // 2, w // 2, c))) if pooled else None
    beta = _f32(rng.normal(0, 0.02, c))
    stats = torch.empty(n * c * 2, dtype=torch.float64, device="cuda")
    ops.in_stats(a, c, stats, n, h * w, c, 1e-6)
    ahat = torch.empty_like(a)
    pool = torch.empty((n, h // 2, w // 2, c), device="cuda", dtype=BF)
    ops.in_apply_pool(a, c, stats, beta, ahat, c, pool, c, n, h, w, c)
    red3 = torch.zeros(n * c * 3, dtype=torch.float64, device="cuda")
    dz_ref, br = _guarded((n, h, w, c), BF)
    db_ref = torch.zeros(c, dtype=torch.float64, device="cuda")
    ops.in_bwd(g1, c, g2, c, a, c, stats, red3, dz_ref, c, db_ref, n, h, w, c, 0.2)
    assert ops.last_kernel() == R.R8, ops.last_kernel()
    r64 = _in_bwd_ref(host(a.float()), host(g1), None if g2 is None else host(g2))
    e = rel_l2(host(dz_ref.float()), r64)
    assert e < TOL_BF16 and band_untouched(br) and _written(dz_ref), e
    zr, ztol = eb.in_bwd_ref_tol(host(a.float()), host(stats), host(g1), None if g2 is None else host(g2), slope=0.2, dt="bf16")
    eb.note("in_bwd gf32 two passes", "bf16", eb.within(host(dz_ref.float()), zr, ztol, {"kind": "in"}, R.R8))
    eb.within(host(db_ref), zr.sum((0, 1, 2)), eb.in_sum_tol(zr, ztol, (0, 1, 2)), None, "in_bwd gf32 bias gradient")
    assert float(red3.abs().max()) == 0.0
    red = torch.zeros(ops.GSUM_SLOTS * n * c * 2, dtype=torch.float64, device="cuda")
    redp = torch.zeros_like(red) if pooled else None
    red.view(ops.GSUM_SLOTS, n, c, 2)[0].copy_(torch.from_numpy(_sums(g1, a)).cuda())
    if pooled:
        redp.view(ops.GSUM_SLOTS, n, c, 2)[0].copy_(torch.from_numpy(_sums(g2, pool)).cuda())
    dstage = torch.zeros(n * c, dtype=torch.float64, device="cuda")
    dz, bz = _guarded((n, h, w, c), BF)
    db = torch.zeros(c, dtype=torch.float64, device="cuda")
    ops.in_bwd_apply(g1, c, g2, c, a, c, stats, beta, red, redp, dstage, dz, c, db, n, h, w, c, 0.2)
    torch.cuda.synchronize()
    assert band_untouched(bz) and _written(dz)
    # (no per-element bound for the RAW-sums form, see test_rect_gpu.test_in_bwd_apply_rect: it is held to the two-pass result, which is held element by element above)
    # test_gsum_gpu.test_in_bwd_apply_matches_reduce_plus_apply's bf16 bounds (the pooled form sums g2 against avgpool(normalised a), itself bf16)
    tol = 2e-2 if pooled else TOL_BF16
    assert rel_l2(host(dz.float()), host(dz_ref.float())) < tol, rel_l2(host(dz.float()), host(dz_ref.float()))
    scale = host(dz_ref.float().abs()).reshape(-1, c).sum(0)
    assert (np.abs(host(db) - host(db_ref)) / scale).max() < TOL_BF16
    assert float(red.abs().max()) == 0.0 and float(dstage.abs().max()) == 0.0 and (redp is None or float(redp.abs().max()) == 0.0)


@pytest.mark.parametrize("c,ld", [(64, 64), (48, 48), (64, 80), (48, 56)])
@pytest.mark.parametrize("with_dbias", [False, True])
def test_lrelu_bwd_gf32(c, ld, with_dbias):
    """shm_lrelu_bwd with fp32 dy and bf16 y / dz (lrelu_bwd_kernel<__bf16, float>) against where(y > 0, dy, slope * dy) in float64; pitch > c: the gap
    between the rows of every tensor keeps its sentinel"""
    ops = _ops()
    rng = np.random.default_rng(21 + c + ld)
    npix, slope = 3 * 8 * 8, 0.2
    yv = rng.standard_normal((npix, c))
    dyv = rng.standard_normal((npix, c))
    y = torch.full((npix, ld), SENTINEL, device="cuda", dtype=BF)
    y[:, :c] = _dev(yv, "bf16")
    dy = torch.full((npix, ld), SENTINEL, device="cuda")
    dy[:, :c] = _f32(dyv)
    flat, band = _guarded((1, 1, npix, ld), BF)
    dz = flat.view(npix, ld)
    dbias = torch.zeros(c, dtype=torch.float64, device="cuda") if with_dbias else None
    red = torch.zeros(ops.LRELU_RED_SLOTS * c, dtype=torch.float64, device="cuda") if with_dbias else None
    ops.lrelu_bwd(dy, ld, y, ld, dz, ld, dbias, npix, c, slope, red=red)
    torch.cuda.synchronize()
    y64, dy64 = host(y[:, :c].float()), host(dy[:, :c])
    ref = np.where(y64 > 0, dy64, slope * dy64)
    got = host(dz[:, :c].float())
    assert rel_l2(got, ref) < TOL_BF16, rel_l2(got, ref)
    assert band_untouched(band) and bool((dz[:, c:] == SENTINEL).all())
    # ... and bit for bit: the fp32 gradient (times the fp32 slope) rounded once, to bf16 -- a bf16 round trip of dy on its way in would move the products
    exact = torch.where(y[:, :c] > 0, dy[:, :c], dy[:, :c] * np.float32(slope)).to(BF)
    assert torch.equal(dz[:, :c], exact)
    if with_dbias:                                   # fp32 partial sums of the unrounded dz, float64 across blocks: on the scale of the summands
        assert (np.abs(host(dbias) - ref.sum(0)) / np.abs(ref).sum(0)).max() < 2e-6
        assert float(red.abs().max()) == 0.0


@pytest.mark.parametrize("h,w", [(4, 4), (8, 24)])
def test_gsum_reduce_pass_gf32(h, w):
    """gsum_reduce_kernel<float, __bf16> on its own: a 1 x 1 layer on a map without whole 64-pixel wave tiles per sample (and one with) -- the sums
    of the stored fp32 gradient against bf16 aux, in slot 0 when the reduce pass delivered them"""
    ops = _ops()
    rng = np.random.default_rng(5)
    n, cin, cout = 3, 64, 64
    dy = _dev(rng.standard_normal((n, h, w, cout)), "bf16")
    wt = _dev(rng.standard_normal((1, 1, cin, cout)) * 0.1, "bf16")
    aux = _dev(rng.standard_normal((n, h, w, cin)), "bf16")
    dx, band = _guarded((n, h, w, cin))
    red = torch.zeros(ops.GSUM_SLOTS * n * cin * 2, dtype=torch.float64, device="cuda")
    ops.conv2d_dgrad(dy, cout, wt, dx, None, 0, cin, 0, n, h, w, cin, cout, 1, 1, gsum=(aux, cin, red))
    torch.cuda.synchronize()
    assert band_untouched(band) and _written(dx)
    ref = host(dy.float()).reshape(-1, cout) @ host(wt.float()).reshape(cin, cout).T
    assert rel_l2(host(dx).reshape(-1, cin), ref) < TOL32
    got = host(red).reshape(ops.GSUM_SLOTS, n, cin, 2)
    if (h * w) % 64:
        assert not got[1:].any()                      # the reduce pass adds into slot 0
    assert R.sums_close(got.sum(0), host(dx), host(aux.float()))


# =====================================================================================================================
# 4b. tapgemm_plan drops the aux and output alignment conditions under `oesz == 4` although aux is bf16: the element epilogues read it two bytes at
# a time.  (The tight gsum cases of this mode are the "gf32" rows of test_gsum_gpu.py.)
@pytest.mark.parametrize("variant,stride", [("halo128_st", 1), ("halo64_st", 1), ("dma128x128", 1), ("dma64x64", 1), ("phase4", 2), ("dma128x128", 2)])
def test_gsum_gf32_takes_unaligned_aux_and_pitched_outputs(variant, stride):
    """aux with a pitch of c + 4 bf16 elements starting 8 bytes into a 16-byte row (a bf16-output launch would hand such sums to the reduce pass), dx
    with a pitch of c + 4 floats: the epilogue still takes the sums, they equal float64 of the stored gradient, the gradient is bit-identical to the
    tight call's and the gaps between its rows keep the sentinel"""
    ops = _ops()
    rng = np.random.default_rng(13)
    n, h, c, cout = 2, 32, 64, 64
    ho = h // stride
    dy = _dev(rng.standard_normal((n, ho, ho, cout)), "bf16")
    wt = _dev(rng.standard_normal((3, 3, c, cout)) * 0.1, "bf16")
    aux = _dev(rng.standard_normal((n, h, h, c)), "bf16")
    ld = c + 4
    auxp = torch.full((n * h * h * ld + 8,), float("nan"), device="cuda", dtype=BF)
    auxv = auxp[4:4 + n * h * h * ld].view(n, h, h, ld)[..., :c]
    auxv.copy_(aux)
    assert auxv.data_ptr() % 16 == 8 and ld % 8 == 4
    tight, bt = _guarded((n, h, h, c))
    flat, bp = _guarded((n, h, h, ld))
    dxp = flat[..., :c]
    ops.set_tuning("tapgemm.variant", variant)
    ops.conv2d_dgrad(dy, cout, wt, tight, None, 0, c, 0, n, h, h, c, cout, 3, stride)
    red = torch.zeros(ops.GSUM_SLOTS * n * c * 2, dtype=torch.float64, device="cuda")
    ops.conv2d_dgrad(dy, cout, wt, dxp, None, 0, ld, 0, n, h, h, c, cout, 3, stride, gsum=(auxv, ld, red))
    torch.cuda.synchronize()
    kern = ops.last_kernel()
    want = _sym(variant, "bf16", out="f32")
    assert kern == (want[:-1] + ", true>" if variant.startswith("halo") else want), kern          # (the halo blocks name their gsum instantiation)
    assert band_untouched(bt) and band_untouched(bp) and bool((flat[..., c:] == SENTINEL).all()), kern
    assert torch.equal(dxp, tight) and _written(tight), kern
    got = host(red).reshape(ops.GSUM_SLOTS, n, c, 2)
    assert got[1:].any(), kern                        # an epilogue took the sums (the reduce pass adds into slot 0 only)
    assert R.sums_close(got.sum(0), host(dxp), host(aux.float())), kern
