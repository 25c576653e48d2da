"""The small kernels around the convolutions -- generator head (plain, with InstanceNorm folded in, SpecSeg's sigmoid form), PatchGAN logits,
Dense(5), shm_lrelu_bwd, the SpecSeg passes and the casts -- against float64 references at the shapes where they take another path than on
test_ops_gpu.py's / test_bf16_gpu.py's friendly ones: one lane or a whole wave per pixel, a ragged last wave, pitches wider than the channel
count, NULL options, pre-loaded accumulators, grid-stride loops past their block cap, more than 16 samples, Dense's scalar fallback, zeros and
subnormals under the LeakyReLU mask, NaN and Inf.

Cases and references come from heads_edge_ref.py; test_heads_edges_cpu.py proves that each case is in the branch it claims.  Inputs are
rounded to the call's dtype first and the reference is computed from the rounded values.  Every output -- the f64 accumulators and the
staging scratch included -- is allocated with a guard band behind it; result tensors start from the guard's fill (about -3e-16: a missing
store reads as zero).  Where a pitch exceeds the channel count the gap of an input holds NaN (a read of it shows in the result) and the gap
of an output the fill, which must come back untouched.  Each check prints its figure before it asserts.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import heads_edge_ref as R
from util import dev, host

pytestmark = pytest.mark.gpu

ACT = {"f32": torch.float32, "bf16": torch.bfloat16, "gf32": torch.bfloat16}
GRAD = {"f32": torch.float32, "bf16": torch.bfloat16, "gf32": torch.float32}
NAN = float("nan")


def _ops():
    from shmgan_amd import ops
    return ops


def _chk(what, fig, tol):
    print(f"{what}: {fig:.3g} (bound {tol:g})")
    assert fig < tol, (what, fig, tol)


def _wide(a, ld, dtype):
    """a [rows, c] (float64 holding values of dtype) as a device tensor [rows, ld]; the gap holds NaN"""
    a = np.asarray(a)
    t = torch.full((a.shape[0], ld), NAN, dtype=torch.float32)
    t[:, :a.shape[1]] = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))
    return t.to(dtype).cuda()


def _out(rows, ld, dtype=torch.float32):
    return R.guarded(rows, ld, dtype, "cuda")


def _intact(raw, p, c):
    """guard band behind p and the gap [c, ld) of every row still hold the fill"""
    gap = p[:, c:].contiguous().view(torch.uint8)
    return R.guard_intact(raw, p) and bool((gap == R.SENT_BYTE).all().item())


def _f64(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()


def _acc(a):
    """a guarded float64 tensor [n] that holds a: the accumulators and staging scratch are outputs too"""
    a = np.asarray(a, dtype=np.float64).ravel()
    raw, p = R.guarded(a.size, 1, torch.float64, "cuda")
    p.copy_(_f64(a).view(-1, 1))
    return raw, p


def _stats(k):
    """[batch][c][2] doubles (mean, inv): the layout of shm_conv2d_in_fwd's `stats`"""
    return _f64(np.stack([k.mean, k.inv], -1))


def _pitches(c):
    return ((c, c), (c + 4, c + 8))          # (ldx, lddx): tight, wide


# --------------------------------------------------------------------------------------------------------------------- generator head
def _head_fwd(k, dt, ldx, bias, norm, kind="lrelu"):
    """one forward call; returns (y as float64 [rows], reference)"""
    ops = _ops()
    rows = k.batch * k.npix
    xd, wd = _wide(k.x, ldx, ACT[dt]), dev(k.w)
    bd = dev([k.b]) if bias else None
    raw, y = _out(rows, 1)
    if kind == "sigmoid":
        ops.head_sigmoid_fwd(xd, ldx, wd, bd, y, rows, k.c)
        ref = R.sigmoid_head_ref(k.x, k.w, k.b if bias else None)
    elif norm:
        ops.head_in_fwd(xd, ldx, _stats(k), dev(k.beta), wd, bd, y, k.batch, k.npix, k.c, R.SLOPE)
        ref = R.head_fwd_ref(R.head_norm(k.x, k.mean, k.inv, k.beta), k.w, k.b if bias else None)
    else:
        ops.head_fwd(xd, ldx, wd, bd, y, rows, k.c, R.SLOPE)
        ref = R.head_fwd_ref(k.x, k.w, k.b if bias else None)
    got = host(y)[:, 0]
    assert R.guard_intact(raw, y)
    return got, ref


def _head_bwd(k, dt, ldx, lddx, norm, dx_none=False, tail=0):
    """one backward call on the reference's own y (rounded to float): dx, dz_out and the increments of the pre-loaded accumulators against
    the reference; tail: also the last so many pixels on their own"""
    ops = _ops()
    c, rows = k.c, k.batch * k.npix
    what = f"head{'_in' if norm else ''}_bwd c={c} npix={k.npix} batch={k.batch} {dt} ld=({ldx},{lddx}) dx_none={dx_none}"
    xh = R.head_norm(k.x, k.mean, k.inv, k.beta) if norm else k.x
    y = R.r32(R.head_fwd_ref(xh, k.w, k.b))
    dz, dx, dw, db = R.head_bwd_ref(xh, k.w, y, k.dy)
    rng = np.random.default_rng(5)
    dw0, db0 = rng.standard_normal(c) * 3, rng.standard_normal(1) * 3
    (wraw, dwa), (braw, dba) = _acc(dw0), _acc(db0)
    rraw, red = _acc(np.full(ops.LRELU_RED_SLOTS * (c + 1), NAN))          # the call zeroes its staging itself
    xd = _wide(k.x, ldx, ACT[dt])
    draw, dxd = (None, None) if dx_none else _out(rows, lddx, GRAD[dt])
    if norm:
        zraw, dzo = _out(rows, 1)
        ops.head_in_bwd(xd, ldx, _stats(k), dev(k.beta), dev(k.w), dev(y), dev(k.dy), dxd, 0 if dx_none else lddx, dwa, dba, k.batch, k.npix, c,
                        R.SLOPE, red, dz_out=dzo)
        assert R.guard_intact(zraw, dzo)
        _chk(what + " dz_out", R.err(host(dzo)[:, 0], dz), R.F32_TOL)
    else:
        ops.head_bwd(xd, ldx, dev(k.w), dev(y), dev(k.dy), dxd, lddx, dwa, dba, rows, c, R.SLOPE, red)
    if not dx_none:
        got = host(dxd.float())[:, :c]
        assert _intact(draw, dxd, c)
        _chk(what + " dx", R.err(got, dx), R.gtol(dt))
        if tail:
            _chk(what + " dx, last pixels", R.err(got[-tail:], dx[-tail:]), R.gtol(dt))
    assert R.guard_intact(wraw, dwa) and R.guard_intact(braw, dba) and R.guard_intact(rraw, red), what + ": a store behind dw_acc, db_acc or red"
    if np.isfinite(dw).all():
        assert np.isfinite(host(red)).all(), what + ": red was not zeroed by the call"
    _chk(what + " dw_acc increment", R.err(host(dwa)[:, 0] - dw0, dw), R.ftol(dt))
    _chk(what + " db_acc increment", R.err(host(dba)[:, 0] - db0, db), R.ftol(dt))


@pytest.mark.parametrize("norm", [False, True])
@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("c", R.HEAD_C)
def test_head_fwd_edges(c, dt, norm):
    """c = 4 (one lane a pixel, no shuffle step) to 256 (a wave a pixel); 1, PP - 1, PP + 1 and 5 PP + 3 pixels (per sample of three in the
    folded form, all odd); tight and wide pitch; bias given and NULL"""
    for npix in R.head_npix(c):
        k = R.head_case(c, npix, dt, R.HEAD_IN_BATCH if norm else 1)
        for ldx, _ in _pitches(c):
            for bias in (True, False):
                got, ref = _head_fwd(k, dt, ldx, bias, norm)
                _chk(f"head{'_in' if norm else ''}_fwd c={c} npix={npix} {dt} ldx={ldx} bias={bias}", R.err(got, ref), R.ftol(dt))


@pytest.mark.parametrize("norm", [False, True])
@pytest.mark.parametrize("dt", R.DTYPES)
@pytest.mark.parametrize("c", R.HEAD_C)
def test_head_bwd_edges(c, dt, norm):
    """the same shapes: the tail loop alone, twice, and the U = 4 main loop followed by two tail trips; ldx = c + 4, lddx = c + 8;
    accumulators pre-loaded (the contract is +=); the folded form also with dx == NULL (dz_out alone)"""
    for npix in R.head_npix(c):
        k = R.head_case(c, npix, dt, R.HEAD_IN_BATCH if norm else 1)
        for ldx, lddx in _pitches(c):
            _head_bwd(k, dt, ldx, lddx, norm)
        if norm and dt != "gf32":
            _head_bwd(k, dt, c + 4, 0, norm, dx_none=True)


@pytest.mark.parametrize("norm", [False, True])
@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_head_fwd_past_the_block_cap(dt, norm):
    """c = 256, 8192 * 4 + 5 pixels (three samples of 10925 in the folded form, where 8192 / 3 blocks a sample bind): the grid-stride loop
    makes a second trip of five pixels"""
    c = R.HEAD_OVER_C
    k = R.head_case(c, R.HEAD_IN_FWD_OVER_HW, dt, R.HEAD_IN_BATCH) if norm else R.head_case(c, R.HEAD_FWD_OVER, dt)
    got, ref = _head_fwd(k, dt, c, True, norm)
    _chk(f"head fwd past the cap {dt} norm={norm}", R.err(got, ref), R.ftol(dt))
    _chk("  last five pixels", R.err(got[-5:], ref[-5:]), R.ftol(dt))


@pytest.mark.parametrize("norm", [False, True])
def test_head_bwd_past_the_block_cap(norm):
    """c = 256, 4096 * 4 * 8 + 5 pixels (three samples of 43693, 4096 / 3 blocks a sample): the U = 4 main loop runs twice and the tail
    loop takes the last pixels.  134 MB a tensor: fp32 alone."""
    c = R.HEAD_OVER_C
    k = R.head_case(c, R.HEAD_IN_BWD_OVER_HW, "f32", R.HEAD_IN_BATCH) if norm else R.head_case(c, R.HEAD_BWD_OVER, "f32")
    _head_bwd(k, "f32", c, c, norm, tail=5)


@pytest.mark.parametrize("c", R.HEAD_C)
def test_sigmoid_head_edges(c):
    for npix in R.head_npix(c):
        k = R.head_case(c, npix, "f32")
        for ldx, _ in _pitches(c):
            for bias in (True, False):
                got, ref = _head_fwd(k, "f32", ldx, bias, False, "sigmoid")
                _chk(f"head_sigmoid_fwd c={c} npix={npix} ldx={ldx} bias={bias}", R.err(got, ref), R.F32_TOL)
                assert np.abs(got - ref).max() < 1e-6          # test_ops_gpu.test_bn_apply_maxpool_pack_sigmoid's bound


def test_sigmoid_head_past_the_block_cap_and_saturated():
    c = R.HEAD_OVER_C
    k = R.head_case(c, R.HEAD_FWD_OVER, "f32")
    got, ref = _head_fwd(k, "f32", c, True, False, "sigmoid")
    _chk("head_sigmoid_fwd past the cap", R.err(got, ref), R.F32_TOL)
    _chk("  last five pixels", R.err(got[-5:], ref[-5:]), R.F32_TOL)
    for c in R.HEAD_C:          # logits of +-100: exactly 0 or 1, or within 1e-6 of the reference; never NaN
        k = R.saturate_rows(R.head_case(c, R.head_npix(c)[3], "f32"))
        got, ref = _head_fwd(k, "f32", c + 4, False, False, "sigmoid")
        print(f"saturated c={c}: values {sorted(set(got.tolist()))[:4]}")
        assert not np.isnan(got).any() and (((got == 0) | (got == 1)) | (np.abs(got - ref) < 1e-6)).all()
        assert (np.abs(got - ref) < 1e-6).all() and (got[0::2] > 0.5).all() and (got[1::2] < 0.5).all()


# ---------------------------------------------------------------------------------------------------------------------- PatchGAN logits
def _patch(k, dt, wide, with_dw):
    ops = _ops()
    n, h, w, c = k.batch, k.h, k.w, k.c
    ldx, lddx = _pitches(c)[int(wide)]
    npx = n * h * w
    what = f"patch n={n} {h}x{w} c={c} {dt} wide={wide} dw={with_dw}"
    xd, wd = _wide(k.x.reshape(npx, c), ldx, ACT[dt]), dev(k.wt)
    yraw, y = _out(npx, 1)
    ops.patch_fwd(xd, ldx, wd, y, n, h, w, c, R.SLOPE)
    yref = R.patch_fwd_ref(k.x, k.wt)
    assert R.guard_intact(yraw, y)
    _chk(what + " y", R.err(host(y), yref), R.ftol(dt))
    yin = R.r32(yref)
    dz, dx, dw = R.patch_bwd_ref(k.x, k.wt, yin, k.dy)
    zraw, dzd = _out(npx, 1)
    xraw, dxd = _out(npx, lddx, GRAD[dt])
    wraw, dwd = _out(9, c) if with_dw else (None, None)
    ops.patch_bwd(xd, ldx, wd, dev(yin), dev(k.dy), dzd, dxd, lddx, dwd, n, h, w, c, R.SLOPE)
    assert R.guard_intact(zraw, dzd) and _intact(xraw, dxd, c)
    _chk(what + " dz", R.err(host(dzd), dz), R.F32_TOL)
    _chk(what + " dx", R.err(host(dxd.float())[:, :c], dx.reshape(npx, c)), R.gtol(dt))
    if with_dw:
        assert R.guard_intact(wraw, dwd)
        _chk(what + " dw", R.err(host(dwd), dw), R.ftol(dt))


@pytest.mark.parametrize("dt", R.DTYPES)
@pytest.mark.parametrize("case", R.PATCH_CASES, ids=lambda t: "n%d_%dx%d_c%d" % t)
def test_patch_edges(case, dt):
    """1, 17 and 33 samples (patch_dw_kernel walks samples g, g + 16, ...), c = 4, 68 (the ch < c guard of the second channel block) and 256,
    maps 2x3, 1x5, 5x1 and 1x1, ldx = c + 4 / lddx = c + 8, dw given and NULL"""
    k = R.patch_case(*case, dt)
    for wide, with_dw in ((False, True), (True, True), (True, False)):
        _patch(k, dt, wide, with_dw)


# ---------------------------------------------------------------------------------------------------------------------------- Dense
def _dense(d, dt, offset, with_dw):
    ops = _ops()
    b, k, nout = d.batch, d.k, d.nout
    what = f"dense batch={b} k={k} nout={nout} {dt} offset={offset} dw={with_dw} fast={R.dense_fast_path(nout, k, offset, 4 if dt == 'f32' else 2)}"
    buf = torch.full((b * k + 8,), NAN, dtype=ACT[dt], device="cuda")
    xv = buf[offset:offset + b * k]
    xv.copy_(dev(d.x).view(-1).to(ACT[dt]))
    wd = dev(d.w)
    yraw, y = _out(b, nout)
    ops.dense_fwd(xv, wd, y, b, k, nout)
    assert R.guard_intact(yraw, y)
    _chk(what + " y", R.err(host(y), R.dense_fwd_ref(d.x, d.w)), R.ftol(dt))
    dx, dw = R.dense_bwd_ref(d.x, d.w, d.dy, d.dx0)
    xraw, dxd = _out(b, k, GRAD[dt])
    dxd.copy_(dev(d.dx0).to(GRAD[dt]))
    wraw, dwd = _out(k, nout) if with_dw else (None, None)
    ops.dense_bwd(xv, wd, dev(d.dy), dxd, dwd, b, k, nout)
    assert R.guard_intact(xraw, dxd)
    _chk(what + " dx (accumulated onto a random dx)", R.err(host(dxd.float()), dx), R.gtol(dt))
    if with_dw:
        assert R.guard_intact(wraw, dwd)
        _chk(what + " dw", R.err(host(dwd), dw), R.ftol(dt))


@pytest.mark.parametrize("dt", R.DTYPES)
@pytest.mark.parametrize("nout", R.DENSE_NOUT)
def test_dense_edges(nout, dt):
    """nout = 1, 5, 8 x k = 3, 1020, 1022, 2052 x batch = 1, 4, 7: the vector path (nout = 5, k % 4 == 0, aligned rows) and the scalar
    fallback forced by k % 4, by nout and by an x that starts one element into its allocation; idle lanes (k < 1024); the four-sample main
    loop of the backward and its tail; dx pre-filled; dw given and NULL"""
    i = 0
    for k in R.DENSE_K:
        for batch in R.DENSE_BATCH:
            d = R.dense_case(batch, k, nout, dt)
            for offset in (0, 1):
                i += 1
                _dense(d, dt, offset, with_dw=bool(i % 3))


def test_dense_bwd_refuses_a_batch_beyond_its_lds():
    """batch * nout * 4 > 48 KiB: an error, and nothing written"""
    from shmgan_amd._lib import ShmError
    ops = _ops()
    b, nout = R.DENSE_REFUSED
    k = 3
    x, w, dy = torch.ones((b, k), device="cuda"), torch.ones((k, nout), device="cuda"), torch.ones((b, nout), device="cuda")
    xraw, dx = _out(b, k)
    wraw, dw = _out(k, nout)
    with pytest.raises(ShmError):
        ops.dense_bwd(x, w, dy, dx, dw, b, k, nout)
    torch.cuda.synchronize()
    assert bool((xraw == R.SENT_BYTE).all().item()) and bool((wraw == R.SENT_BYTE).all().item())
    ops.dense_bwd(x, w, dy, dx, dw, b - 1, k, nout)          # one sample fewer fits: dx += nout on b - 1 rows, the last row keeps its fill
    assert R.guard_intact(xraw, dx[:b - 1]) and R.guard_intact(wraw, dw)
    assert (np.abs(host(dx)[:b - 1] - nout) < 1e-5).all() and (host(dw) == b - 1).all()


# ------------------------------------------------------------------------------------------------------------------------ shm_lrelu_bwd
@pytest.mark.parametrize("dt", R.DTYPES)
@pytest.mark.parametrize("c", R.LRELU_C)
def test_lrelu_bwd_edges(c, dt):
    """c = 4, 48 (twelve lanes a pixel, 21 pixels a trip, four idle threads) and 1024 (one pixel a trip); 1, PP * U + 1 and 4099 pixels (chunks
    that end off a multiple of U * PP; more blocks than staging slots at c = 1024); three different pitches; dbias pre-loaded and NULL;
    +0.0, -0.0 (slope applies) and the smallest subnormal (it does not) in y; the staging scratch zero on return"""
    ops = _ops()
    ztol = R.F32_TOL if dt == "f32" else R.BF16_TOL          # dz is activation-typed
    for npix in R.lrelu_npix(c, dt):
        k = R.lrelu_case(c, npix, dt)
        dz, db = R.lrelu_bwd_ref(k.y, k.dy)
        for with_db in (True, False):
            what = f"lrelu_bwd c={c} npix={npix} {dt} dbias={with_db}"
            dyd, yd = _wide(k.dy, c + 4, GRAD[dt]), _wide(k.y, c + 8, ACT[dt])
            raw, dzd = _out(npix, c + 12, ACT[dt])
            braw, dbd = _acc(k.db0) if with_db else (None, None)
            rraw, red = _acc(np.zeros(ops.LRELU_RED_SLOTS * c))
            ops.lrelu_bwd(dyd, c + 4, yd, c + 8, dzd, c + 12, dbd, npix, c, R.SLOPE, red)
            got = host(dzd.float())[:, :c]
            assert _intact(raw, dzd, c) and R.guard_intact(rraw, red) and (not with_db or R.guard_intact(braw, dbd)), what + ": a store behind dz, red or dbias"
            assert not bool(red.view(torch.int64).any().item()), what + ": red is not zero on return"
            _chk(what + " dz", R.err(got, dz), ztol)
            print("  special elements:", [(got[p, ch], dz[p, ch]) for p, ch in k.special[:3]])
            assert R.lrelu_special_ok(got, k, ztol)
            if with_db:
                _chk(what + " dbias increment", R.err(host(dbd)[:, 0] - k.db0, db), R.ftol(dt))


# --------------------------------------------------------------------------------------------------------------------- SpecSeg passes
def _bn(npix, c, lda, ldo):
    ops = _ops()
    k = R.bn_case(npix, c)
    raw, out = _out(npix, ldo)
    ops.bn_apply(_wide(k.a, lda, torch.float32), lda, dev(k.gamma), dev(k.beta), dev(k.mean), dev(k.var), R.BN_EPS, out, ldo, npix, c)
    got = host(out)[:, :c]
    assert _intact(raw, out, c)
    return got, R.bn_ref(k.a, k.gamma, k.beta, k.mean, k.var)


def test_bn_apply_pitches_and_grid_stride():
    b, h, w, c = R.SPEC_PITCH_MAP
    got, ref = _bn(b * h * w, c, c + 4, c + 8)
    _chk("bn_apply 2x6x10 lda=c+4 ldo=c+8", R.err(got, ref), R.F32_TOL)
    b, h, w, c = R.SPEC_OVER_MAP
    got, ref = _bn(b * h * w, c, c, c)
    _chk(f"bn_apply {b * h * w * c // 4} vectors", R.err(got, ref), R.F32_TOL)
    _chk("  last 250 pixels (the second trip of the grid-stride loop)", R.err(got[-250:], ref[-250:]), R.F32_TOL)


def _maxpool(b, ho, wo, c, ldx, ldy):
    ops = _ops()
    x = np.random.default_rng(97).standard_normal((b, 2 * ho, 2 * wo, c), dtype=np.float32)
    raw, y = _out(b * ho * wo, ldy)
    ops.maxpool2_fwd(_wide(x.reshape(-1, c), ldx, torch.float32), ldx, y, ldy, b, 2 * ho, 2 * wo, c)
    got = y[:, :c].cpu().numpy()
    assert _intact(raw, y, c)
    return got, R.maxpool_ref(x).reshape(-1, c)


def test_maxpool2_pitches_and_grid_stride():
    """bit-exact: a selection"""
    b, h, w, c = R.SPEC_PITCH_MAP
    got, ref = _maxpool(b, h // 2, w // 2, c, c + 4, c + 8)
    assert np.array_equal(got, ref)
    b, ho, wo, c = R.SPEC_OVER_MAP
    got, ref = _maxpool(b, ho, wo, c, c, c)
    print("maxpool2 past the cap: differing elements", int((got != ref).sum()), "of", ref.size)
    assert np.array_equal(got, ref)


@pytest.mark.parametrize("nc,lddst,npix", [(nc, ld, R.PACK_NPIX[0]) for nc, ld in R.PACK_CASES] + [(1, 4, R.PACK_NPIX[1]), (3, 4, R.PACK_NPIX[1])])
def test_pack_channels_windows(nc, lddst, npix):
    """nc = 1, 3 from channel c0 = 1 of a five-channel source into pitches 4 and 16: a copy, the rest of the row +0.0, bit for bit; 8192 * 256
    + 77 pixels at pitch 4 (one vector a pixel) are past the grid"""
    ops = _ops()
    ldsrc, c0 = R.PACK_SRC
    src = np.random.default_rng(98).standard_normal((npix, ldsrc), dtype=np.float32)
    raw, dst = _out(npix, lddst)
    ops.pack_channels(torch.from_numpy(src).cuda(), ldsrc, c0, nc, dst, lddst, npix)
    assert R.guard_intact(raw, dst)
    assert np.array_equal(dst.cpu().numpy().view(np.int32), R.pack_ref(src, c0, nc, lddst).view(np.int32))


@pytest.mark.parametrize("batch,npix", R.SPEC_LOSS_SHAPES)
def test_spec_loss_grid_stride(batch, npix):
    """masks of 0 and 1, five distinct ds, against oracle/specseg_torch.spec_loss; 3 x 21858 = 256 * 256 + 38 pixels are past the 256-block
    grid (256 * 256 + 37 is no multiple of three); each term to a relative 1e-5 (test_step_gpu.test_spec_loss_kernel)"""
    ops = _ops()
    k = R.spec_case(batch, npix)
    dsd = [dev(a) for a in k.ds]
    ptr = (C.c_void_p * 5)(*[t.data_ptr() for t in dsd])
    raw, loss = R.guarded(5, 1, torch.float64, "cuda")          # the call zeroes its five sums itself
    ops.spec_loss(dev(k.cyc_y), dev(k.cbcr), ptr, dev(k.mask), loss, batch, npix)
    got, ref = host(loss)[:, 0], R.spec_loss_ref(k)
    rel = np.abs(got / ref - 1)
    print(f"spec_loss B={batch} npix={npix}: relative error per term {rel}")
    assert R.guard_intact(raw, loss) and (rel < R.F32_TOL).all()


# ------------------------------------------------------------------------------------------------------------------------------ casts
@pytest.mark.parametrize("n", R.CAST_SIZES)
def test_cast_f32_is_round_to_nearest_even(n):
    """against torch's conversion on the CPU, bit for bit: ties both ways, +-0, subnormals, the largest finite float (-> Inf), +-Inf, NaN
    (also one whose payload a truncation would lose); 4096 * 256 + 77 elements: the grid-stride loop's second trip.  SHM_F32: a copy."""
    ops = _ops()
    x = R.cast_input(n)
    xd = torch.from_numpy(x).cuda()
    raw, d = _out(n, 1, torch.bfloat16)
    ops.cast_f32(xd, d, n)
    got = d.view(torch.int16).cpu().numpy()[:, 0]
    bits, nan = R.cast_ref_bits(x)
    print(f"cast_f32 n={n}: differing elements {int((got != bits)[~nan].sum())}, NaN kept {bool(torch.isnan(d[:, 0].float().cpu())[torch.from_numpy(nan)].all())}")
    assert R.guard_intact(raw, d) and R.same_bits(got, bits, nan) and bool(torch.isnan(d[:, 0].float().cpu())[torch.from_numpy(nan)].all())
    raw, d = _out(n, 1)
    ops.cast_f32(xd, d, n)
    got = d.cpu().numpy()[:, 0]
    assert R.guard_intact(raw, d) and R.same_bits(got.view(np.int32), x.view(np.int32), np.isnan(x)) and np.isnan(got[np.isnan(x)]).all()


@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("n", R.CAST_SIZES)
def test_cvt_f64_f32(n, accumulate):
    """float32(s) bit for bit (the sign of zero included); accumulating: d + float32(s) evaluated in float32"""
    ops = _ops()
    s, d0 = R.cvt_input(n)
    raw, d = _out(n, 1)
    d.copy_(torch.from_numpy(d0).cuda().view(n, 1))
    ops.cvt_f64_f32(_f64(s), d, n, accumulate)
    got, ref = d.cpu().numpy()[:, 0], R.cvt_ref(s, d0, accumulate)
    nan = np.isnan(ref)
    print(f"cvt_f64_f32 n={n} acc={accumulate}: differing elements {int((got.view(np.int32) != ref.view(np.int32))[~nan].sum())}; first {got[:8]} ref {ref[:8]}")
    assert R.guard_intact(raw, d) and R.same_bits(got.view(np.int32), ref.view(np.int32), nan) and np.isnan(got[nan]).all()


# -------------------------------------------------------------------------------------------------------------------- NaN and Inf
@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_head_nonfinite(dt):
    """one NaN in x, one Inf in dy: NaN and Inf sit where the float64 reference has them (R.err is infinite otherwise), the rest within the
    tolerance"""
    c = 64
    k = R.head_case(c, R.head_npix(c)[3], dt)
    k.x[17, 5], k.dy[40] = NAN, np.inf
    got, ref = _head_fwd(k, dt, c + 4, True, False)
    assert np.isnan(ref).sum() == 1
    _chk(f"head_fwd non-finite {dt}", R.err(got, ref), R.ftol(dt))
    _head_bwd(k, dt, c + 4, c + 8, False)
    dw = R.head_bwd_ref(k.x, k.w, R.r32(ref), k.dy)[2]
    assert np.isnan(dw).sum() == 1 and np.isinf(dw).sum() == c - 1


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_patch_nonfinite(dt):
    k = R.patch_case(2, 3, 4, 68, dt)
    k.x[0, 1, 1, 5], k.dy[1, 2, 3] = NAN, -np.inf
    y = R.patch_fwd_ref(k.x, k.wt)
    dz, dx, dw = R.patch_bwd_ref(k.x, k.wt, R.r32(y), k.dy)
    assert np.isnan(y).sum() == 9 and np.isinf(dz).sum() == 1 and np.isinf(dx).sum() == 4 * 68 and np.isnan(dw).sum() == 9
    _patch(k, dt, True, True)


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("nout,k", [(5, 1020), (8, 1022)])
def test_dense_nonfinite(nout, k, dt):
    d = R.dense_case(4, k, nout, dt)
    d.x[1, 700], d.dy[2, nout - 1] = NAN, np.inf
    dx, dw = R.dense_bwd_ref(d.x, d.w, d.dy, d.dx0)
    assert np.isnan(R.dense_fwd_ref(d.x, d.w)).sum() == nout and np.isinf(dx).sum() == k and np.isnan(dw).sum() == nout and np.isinf(dw).sum() == k - 1
    _dense(d, dt, 0, True)
