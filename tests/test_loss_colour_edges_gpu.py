"""The loss, colour and optimiser kernels (csrc/color.hip, csrc/imgloss.hip) against the float64 oracle at the shapes and inputs where
they take another path than on test_ops_gpu.py's / test_step_gpu.py's friendly ones: grid-stride loops that iterate and end ragged, waves
that straddle the end of the D input, a variance on the floor, SSIM tiles of one pixel, rescale_01 ranges that are zero, extremes in the
chroma or in the Y plane, flag masks 0 and 31, dirty scratch memory, more patches than lanes, logits of +-80.

Inputs and references come from loss_edge_ref.py; test_loss_colour_edges_cpu.py proves that each input is in the case it claims.  Every
output is allocated with a guard band behind it (loss_edge_ref.guarded) and starts from NaN or the guard's fill, so a store past the end, a
store that is missing and a read of what the call should have written all show.  Each test prints its figures before it asserts.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import loss_edge_ref as R
from util import dev, host, rel_l2

pytestmark = pytest.mark.gpu

DT = {"f32": torch.float32, "bf16": torch.bfloat16}
NAN = float("nan")


def _ops():
    from shmgan_amd import ops
    return ops


def rb(a):
    """numpy array rounded through bf16, as float64"""
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(torch.bfloat16).double().numpy()


def _out(rows, cols, dtype=torch.float32, fill=None):
    """guarded output [rows, cols]; fill: a start value for the payload (default: the guard's own fill)"""
    raw, p = R.guarded(rows, cols, dtype, "cuda")
    if fill is not None:
        p.fill_(fill)
    return raw, p


def _in(a, dtype=torch.float32):
    return dev(a).to(dtype)


def _zero_bits(t):
    """every element is +0.0, bit for bit"""
    t = t.contiguous()
    return bool((t.view(torch.int32 if t.dtype == torch.float32 else torch.int16) == 0).all().item())


# ------------------------------------------------------------------------------------------------------------------------ clip + Adam
@pytest.mark.parametrize("n", R.ADAM_SIZES)
def test_adam_clip_edges(n):
    """n = 1, 255 (less than a block) and 8192 * 256 + 77 (the grid-stride loop runs twice and ends on a ragged tail), gradients on both
    sides of the clip and exactly on it, v = 0 with g = 0 so that eps alone is the denominator."""
    ops = _ops()
    c = R.adam_case(n)
    bufs = [_out(n, 1) for _ in range(3)]
    for (_, p), a in zip(bufs, (c.w, c.m, c.v)):
        p.copy_(dev(a).view(n, 1))
    wd, md, vd = (p for _, p in bufs)
    ops.adam_clip(wd, md, vd, dev(c.g), n, c.alpha, R.ADAM_B1, R.ADAM_B2, R.ADAM_EPS, R.ADAM_GSCALE)
    w, m, v = host(wd)[:, 0], host(md)[:, 0], host(vd)[:, 0]
    figs = (rel_l2(w, c.rw), rel_l2(m, c.rm), rel_l2(v, c.rv))
    print(f"adam n={n}: rel_l2 w/m/v {figs}")
    assert all(R.guard_intact(raw, p) for raw, p in bufs)
    assert figs[0] < 1e-6 and figs[1] < 1e-6 and figs[2] < 1e-6
    k = c.clipped
    if k.any():
        err = np.abs(w - c.rw)[k] / R.adam_w_abs_bound(c.rw)[k]
        print(f"adam n={n}: clipped {int(k.sum())}, max |dw| / bound {err.max()}")
        assert err.max() <= 1.0
    if n > R.ADAM_GRID:
        t = slice(n - R.ADAM_TAIL, n)
        assert (w[t] != c.w[t]).all() and (m[t] != c.m[t]).all()
        moved = R.r32(c.rv)[t] != c.v[t]
        assert moved.any() and (v[t] != c.v[t])[moved].all()


# ------------------------------------------------------------------------------------------------- colour and input assembly, ragged
PITCHES = [("f32", 16), ("bf16", 32), ("f32", 8), ("f32", 20)]          # two whole-wave 64-byte row forms, two per-lane forms


def _check_padded(raw, dp, want, dt, sibling=None):
    """dp [rows, ld] written by yuv2rgb / pack_rgb16: columns 0..2 against want (float64), every other column +0.0, guard untouched.
    sibling (bf16): the fp32 output of the same call, whose bf16 rounding the bf16 form must equal bit for bit (test_input_assembly_bf16)."""
    got = host(dp.float())
    assert R.guard_intact(raw, dp)
    assert _zero_bits(dp[:, 3:])
    if dt == "f32":
        fig = rel_l2(got[:, :3], want)
        print(f"  padded f32 ld={dp.shape[1]}: rel_l2 {fig}")
        assert fig < R.F32_TOL
    else:
        fig = rel_l2(got[:, :3], rb(want))
        print(f"  padded bf16 ld={dp.shape[1]}: rel_l2 against the rounded reference {fig}")
        assert fig < R.BF16_TOL
        assert np.array_equal(got[:, :3], rb(host(sibling)[:, :3]))


@pytest.mark.parametrize("with_noise", [False, True])
@pytest.mark.parametrize("dt,ld", PITCHES + [(None, 0)])
@pytest.mark.parametrize("shape", R.COLOUR_SHAPES)
def test_yuv2rgb_ragged(shape, dt, ld, with_noise):
    """5 B npix rows that are no multiple of 64 or 256: the last wave of the whole-wave row store straddles the end of dpad."""
    ops = _ops()
    c = R.colour_case(*shape)
    B, h, w, npix = c.B, c.h, c.w, c.npix
    rows = 5 * B * npix
    ref = R.yuv2rgb_ref(c.ych, c.cbcr).reshape(rows, 3)
    want = ref + c.noise.reshape(rows, 3) if with_noise else ref
    noise = dev(c.noise) if with_noise else None
    ych, cbcr = dev(c.ych), dev(c.cbcr)

    def run(dtype, pitch):
        rraw, rgb = _out(rows, 3)
        praw, dp = _out(rows, pitch, dtype) if dtype is not None else (None, None)
        ops.yuv2rgb(ych, cbcr, noise, rgb.view(5 * B, h, w, 3), None if dp is None else dp.view(5 * B, h, w, pitch), 5 * B, B, npix)
        fig = rel_l2(host(rgb), ref)
        print(f"yuv2rgb {shape} {dt} ld={pitch} noise={with_noise}: rgb rel_l2 {fig}")
        assert R.guard_intact(rraw, rgb) and fig < R.F32_TOL
        return praw, dp
    praw, dp = run(DT.get(dt), ld)
    if dt is not None:
        sib = run(torch.float32, 16)[1] if dt == "bf16" else None
        _check_padded(praw, dp, want, dt, sib)


@pytest.mark.parametrize("with_noise", [False, True])
@pytest.mark.parametrize("dt,ld", PITCHES)
@pytest.mark.parametrize("shape", R.COLOUR_SHAPES)
def test_pack_rgb16_ragged(shape, dt, ld, with_noise):
    ops = _ops()
    c = R.colour_case(*shape)
    rows = 5 * c.B * c.npix
    rgb = R.r32(R.yuv2rgb_ref(c.ych, c.cbcr)).reshape(rows, 3)
    noise = c.noise.reshape(rows, 3)
    want = rgb + noise if with_noise else rgb
    rgbd, nd = dev(rgb), (dev(noise) if with_noise else None)
    print(f"pack_rgb16 {shape} {dt} ld={ld} noise={with_noise}")
    praw, dp = _out(rows, ld, DT[dt])
    ops.pack_rgb16(rgbd, nd, dp, rows)
    sib = None
    if dt == "bf16":
        sib = _out(rows, 16)[1]
        ops.pack_rgb16(rgbd, nd, sib, rows)
    _check_padded(praw, dp, want, dt, sib)
    if dt == "f32" and not with_noise:
        assert np.array_equal(host(dp)[:, :3], rgb)          # a copy


@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("dt,ld", [("f32", 16), ("bf16", 32)])
@pytest.mark.parametrize("shape", R.COLOUR_SHAPES)
def test_rgb16_to_dy_ragged(shape, dt, ld, accumulate):
    """accumulate = 0 overwrites (dy starts from NaN), accumulate = 1 adds to a non-zero dy; only columns 0..2 of the rows are summed."""
    ops = _ops()
    rng = np.random.default_rng(41)
    rows = 5 * shape[0] * shape[1] * shape[2]
    d = rng.standard_normal((rows, ld))
    d = rb(d) if dt == "bf16" else R.r32(d)
    dy0 = R.r32(rng.standard_normal(rows))
    raw, dy = _out(rows, 1, fill=NAN)
    if accumulate:
        dy.copy_(dev(dy0).view(rows, 1))
    ops.rgb16_to_dy(_in(d, DT[dt]), dy, rows, accumulate)
    ref = d[:, :3].sum(-1) + (dy0 if accumulate else 0.0)
    fig = rel_l2(host(dy)[:, 0], ref)
    print(f"rgb16_to_dy {shape} {dt} acc={accumulate}: rel_l2 {fig}")
    assert R.guard_intact(raw, dy)
    assert fig < (R.F32_TOL if dt == "f32" else R.BF16_READ_TOL)


@pytest.mark.parametrize("mask", R.GEN_MASKS)
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("dt,ld", [("f32", 16), ("bf16", 32)])
@pytest.mark.parametrize("shape", R.COLOUR_SHAPES)
def test_build_gen_input_ragged(shape, dt, ld, mode, mask):
    """The planes are copies: fp32 bit for bit, bf16 the rounding of the reference; one-hot plane, zero padding and guard exactly."""
    ops = _ops()
    c = R.colour_case(*shape)
    nimg = 5 * c.B if mode else c.B
    rows = nimg * c.npix
    raw, out = _out(rows, ld, DT[dt])
    ops.build_gen_input([dev(y) for y in c.ys], dev(c.gen_y), mask, mode, out.view(nimg, c.h, c.w, ld), c.B, c.npix)
    ref = R.gen_input_ref(c.ys, c.gen_y, mask, mode, ld).reshape(rows, ld)
    got = host(out.float())
    assert R.guard_intact(raw, out)
    assert _zero_bits(out[:, 10:])
    assert np.array_equal(got, ref if dt == "f32" else rb(ref))


@pytest.mark.parametrize("mask", R.GEN_MASKS)
@pytest.mark.parametrize("dt,ld", [("f32", 16), ("bf16", 32)])
@pytest.mark.parametrize("shape", R.COLOUR_SHAPES)
def test_cyc_input_bwd_accumulates(shape, dt, ld, mask):
    """dgen_y starts non-zero: the kernel adds to it (mask 0: adds nothing, bit for bit)."""
    ops = _ops()
    B, h, w = shape
    rng = np.random.default_rng(42)
    dcyc = rng.standard_normal((5 * B, h, w, ld))
    dcyc = rb(dcyc) if dt == "bf16" else R.r32(dcyc)
    g0 = R.r32(rng.standard_normal((B, h, w)))
    raw, dg = _out(B * h * w, 1)
    dg.copy_(dev(g0).view(-1, 1))
    ops.cyc_input_bwd(_in(dcyc, DT[dt]), mask, dg, B, h * w)
    got = host(dg)[:, 0]
    ref = (g0 + R.cyc_input_bwd_ref(dcyc, mask, B)).ravel()
    fig = rel_l2(got, ref)
    print(f"cyc_input_bwd {shape} {dt} mask={mask}: rel_l2 {fig}")
    assert R.guard_intact(raw, dg)
    assert fig < (R.F32_TOL if dt == "f32" else R.BF16_READ_TOL)
    if mask == 0:
        assert np.array_equal(got, g0.ravel())


@pytest.mark.parametrize("shape", R.COLOUR_SHAPES)
def test_avg_cbcr_ragged(shape):
    ops = _ops()
    c = R.colour_case(*shape)
    n = c.B * c.npix
    raw, out = _out(n, 2, fill=NAN)
    ops.avg_cbcr([dev(y) for y in c.ys], out, n)
    fig = rel_l2(host(out), R.avg_cbcr_ref(c.ys).reshape(n, 2))
    print(f"avg_cbcr {shape}: rel_l2 {fig}")
    assert R.guard_intact(raw, out) and fig < R.F32_TOL


# ---------------------------------------------------------------------------------------------------------------------- standardisation
def _std(rgb):
    ops = _ops()
    B, npix = rgb.shape[0], rgb.shape[1] * rgb.shape[2]
    yraw, yuv = _out(B * npix, 3, fill=NAN)
    sraw, scale = _out(B, 1, fill=NAN)
    acc = torch.full((2 * B,), NAN, dtype=torch.float64, device="cuda")
    ops.rgb2yuv_std(dev(rgb), yuv, acc, scale, B, npix)
    assert R.guard_intact(yraw, yuv) and R.guard_intact(sraw, scale)
    return host(yuv).reshape(B, npix, 3), host(scale)[:, 0]


def test_std_scale_floor():
    """Black and a constant dark grey return the floor 1/256 exactly; the random image and mid-grey beside them their own scale (mid-grey
    is NOT on the floor: its YUV is (0.5, 0, 0), standard deviation 0.2357): the samples share no accumulator."""
    x = R.std_floor_batch()
    ryuv, rscale = R.std_ref(x)
    yuv, scale = _std(x)
    print(f"std floor: scale {scale} ref {rscale}; rel_l2 yuv {rel_l2(yuv, ryuv)}")
    assert scale[0] == R.STD_FLOOR and scale[3] == R.STD_FLOOR
    assert abs(scale[1] - R.STD_MID_GREY_SCALE) < R.F32_TOL * R.STD_MID_GREY_SCALE
    assert rel_l2(scale, rscale) < R.F32_TOL
    assert not yuv[0].any()
    for b in range(1, 4):
        assert rel_l2(yuv[b], ryuv[b].reshape(-1, 3)) < R.F32_TOL, b


def test_std_grid_stride():
    """131072 + 37 pixels in one sample: past the 32-block cap of the statistics pass and the 512-block cap of the scale pass."""
    x = R.std_ramp()
    ryuv, rscale = R.std_ref(x)
    yuv, scale = _std(x)
    figs = (rel_l2(yuv, ryuv.reshape(1, -1, 3)), rel_l2(scale, rscale), rel_l2(yuv[0, -37:], ryuv.reshape(-1, 3)[-37:]))
    print(f"std ramp: rel_l2 yuv {figs[0]} scale {figs[1]} last 37 pixels {figs[2]}")
    assert figs[0] < R.F32_TOL and figs[1] < R.F32_TOL and figs[2] < R.F32_TOL


# ------------------------------------------------------------------------------------------------------------------------ image losses
@functools.lru_cache(maxsize=None)
def _case(name):
    inp, flags = R.image_case(name)
    return inp, flags, R.image_oracle(inp, flags)


def _run_image(name, ws_fill=0x00, raw=None):
    """one call of shm_image_losses on a workspace of exactly image_losses_workspace(B, S) bytes, filled with ws_fill (or `raw`, the
    allocation a previous call left).  Outputs start from NaN.  The default fill is zero: a position or a sum the call failed to
    initialise then reads as pixel 0 or as 0.0 -- wrong, but inside the tensors.
    Returns (loss [32] float64, dgen_y, dcyc_y as float32 numpy, raw)."""
    ops = _ops()
    inp, flags, o = _case(name)
    B, S = inp.B, inp.S
    total = ops.image_losses_workspace(B, S)
    if raw is None:
        raw = torch.full((total + 1024,), ws_fill, dtype=torch.uint8, device="cuda")
    tail = raw[total:].clone()
    od = [dev(x) for x in inp.orig]
    dd = [dev(d.numpy()) for d in inp.ds]
    optr = (C.c_void_p * 5)(*[t.data_ptr() for t in od])
    dptr = (C.c_void_p * 5)(*[t.data_ptr() for t in dd])
    loss = torch.full((32,), NAN, dtype=torch.float64, device="cuda")
    graw, dg = _out(B * S * S, 1, fill=NAN)
    craw, dc = _out(5 * B * S * S, 1, fill=NAN)
    fmask = sum(1 << k for k in range(5) if flags[k])
    ops.image_losses(dev(o.gen_rgb.numpy()), dev(torch.cat(o.crgb, 0).numpy()), dev(inp.cyc_y), dev(inp.cbcr.numpy()), optr, dptr, fmask,
                     R.STYLE_FACTOR, loss, dg, dc, raw[:total], B, S)
    torch.cuda.synchronize()
    assert R.guard_intact(graw, dg) and R.guard_intact(craw, dc) and torch.equal(raw[total:], tail)
    return host(loss), dg.cpu().numpy().reshape(B, S, S, 1), dc.cpu().numpy().reshape(5 * B, S, S, 1), raw


def _check_image(name, L, dg, dc):
    """loss slots 0..17 and both gradients against the float64 oracle, at the tolerances of test_image_losses"""
    inp, flags, o = _case(name)
    e = R.image_errors(L, dg.astype(np.float64), dc.astype(np.float64), o, inp)
    sb = R.loss_slot_bounds(o)
    eb = np.array([x[3] for x in R.extreme_elements(inp, o.rc.numpy())])
    print(f"image {name}: worst slot error / bound {(e.slots / sb).max():.3g} (slot {(e.slots / sb).argmax()}), rel_l2 dgen_y {e.dg:.3g} "
          f"dcyc_y {e.dc:.3g}, extreme elements error / bound {(e.ext / eb).max() if len(eb) else 0.0:.3g}")
    assert np.isfinite(L).all() and np.isfinite(dg).all() and np.isfinite(dc).all()
    assert (L[18:] == 0.0).all()
    assert (e.slots < sb).all(), (e.slots / sb)
    assert e.dg < R.GRAD_TOL and e.dc < R.GRAD_TOL
    assert (e.ext < eb).all(), (e.ext / eb)
    return o


@pytest.mark.parametrize("name", R.SIZE_CASES)
def test_image_losses_sizes_and_flags(name):
    """S = 11 (one SSIM pixel), 16, 26 (exactly one forward tile), 27 (a second tile of one pixel), B = 1 and 3; no flag, a mixed mask, all
    five.  With all five set the SSIM loss slots are exactly zero and the gradient is that of the L1, content and style parts alone."""
    L, dg, dc, _ = _run_image(name)
    _check_image(name, L, dg, dc)
    inp, flags, o = _case(name)
    for k in range(5):
        if flags[k]:
            assert L[11 + k] == 0.0
    if all(flags):
        rest = R.image_oracle(inp, flags, ssim_term=False)
        assert rel_l2(dc, rest.rc.numpy()) < R.GRAD_TOL and rel_l2(dg, rest.rg.numpy()) < R.GRAD_TOL


@pytest.mark.parametrize("name", ["chroma_extremes", "y_extremes"])
def test_image_losses_extreme_placement(name):
    """rescale_01's minimum and maximum of every cyclic view in the chroma planes (no min / max gradient reaches Y: argpos stays -1) or in
    the Y plane (the two extreme pixels carry ssim_minmax_kernel's correction; _check_image holds them to their own absolute bound).
    Tied extremes are out of scope: the kernel gives the whole sub-gradient to one tied pixel, amin / amax autograd splits it."""
    L, dg, dc, _ = _run_image(name)
    _check_image(name, L, dg, dc)


def test_image_losses_black_original():
    """orig[k] = 0: ds_k = 0, rescale_01's range of the target is zero (divide_no_nan, yr == 0)."""
    L, dg, dc, _ = _run_image("black_view")
    o = _check_image("black_view", L, dg, dc)
    k = R.BLACK_K
    assert abs(L[6 + k] - float(o.ssims[k].sum())) < 2e-5 and abs(L[1 + k] - float(o.l1c[k].sum())) < 1e-5


@pytest.mark.parametrize("k", [1, 4])
def test_image_losses_flat_cyc_view(k):
    """cbcr = c and cyc_y[k] = c: rescale_01's range of view k is zero (xr == 0).  dcyc_y of that view holds the L1 part alone (k = 4: plus
    content and style), and the ssim slot is the oracle's where(den == 0, ...)."""
    name = f"flat_cyc{k}"
    L, dg, dc, _ = _run_image(name)
    o = _check_image(name, L, dg, dc)
    inp, flags, _ = _case(name)
    rest = R.image_oracle(inp, flags, ssim_term=False)
    fig = rel_l2(dc[k], rest.rc.numpy()[k])
    print(f"flat view {k}: rel_l2 of its gradient against the parts without SSIM {fig}")
    assert fig < R.GRAD_TOL
    assert abs(L[6 + k] - float(o.ssims[k].sum())) < 2e-5


@pytest.mark.parametrize("name", ["y_extremes", "chroma_extremes"])
def test_image_losses_scratch_independence(name):
    """The same case on a zero-filled workspace, on one filled with 0xFF bytes, and again on what that call left behind: every scratch field
    is initialised by the call itself.  All outputs are bit-identical, except those that depend on the order of the double atomic adds --
    the loss slots and the two rescale_01 extreme pixels per view of dcyc_y -- which are held to the oracle each time."""
    inp, flags, o = _case(name)
    B = inp.B
    r0 = _run_image(name, 0x00)
    r1 = _run_image(name, 0xFF)
    r2 = _run_image(name, raw=r1[3])
    free = np.zeros((5 * B, inp.S * inp.S), bool)
    for (b, k), pmin, pmax, _ in R.extreme_elements(inp, o.rc.numpy()):
        free[k * B + b, [pmin, pmax]] = True
    assert free.any() == (name == "y_extremes")
    for i, (L, dg, dc, _) in enumerate((r0, r1, r2)):
        print(f"scratch run {i}")
        _check_image(name, L, dg, dc)
        assert np.array_equal(dg.view(np.uint32), r0[1].view(np.uint32)), i
        same = dc.view(np.uint32).reshape(free.shape) == r0[2].view(np.uint32).reshape(free.shape)
        assert (same | free).all(), (i, np.argwhere(~(same | free))[:8])


def test_image_losses_argument_errors():
    """S = 10 (below the SSIM window) and a workspace one byte short are rejected on the host, before any launch."""
    from shmgan_amd._lib import ShmError
    ops = _ops()
    B, S = 1, 11
    x = torch.zeros((5 * B * S * S * 3,), device="cuda")
    ptr = (C.c_void_p * 5)(*[x.data_ptr()] * 5)
    loss = torch.full((32,), 7.0, dtype=torch.float64, device="cuda")
    total = ops.image_losses_workspace(B, S)
    ws = torch.zeros((total,), dtype=torch.uint8, device="cuda")
    assert total > 0 and ops.image_losses_workspace(B, 10) == 0
    with pytest.raises(ShmError):
        ops.image_losses(x, x, x, x, ptr, ptr, 0, 1.0, loss, x, x, ws, B, 10)
    with pytest.raises(ShmError):
        ops.image_losses(x, x, x, x, ptr, ptr, 0, 1.0, loss, x, x, ws[:total - 1], B, S)
    torch.cuda.synchronize()
    assert (host(loss) == 7.0).all()          # nothing ran


# ---------------------------------------------------------------------------------------------------------- discriminator-head losses
def _dhead(rf, cls, B, npatch, T, mode):
    ops = _ops()
    T = float(np.float32(T))          # the kernel takes the target as a float
    o = R.dhead_oracle(rf, cls, B, T, mode)
    loss = torch.full((16,), NAN, dtype=torch.float64, device="cuda")
    outs = [_out(12 * B, npatch, fill=NAN), _out(12 * B, 5, fill=NAN), _out(6 * B, npatch, fill=NAN)]
    (_, drf_d), (_, dcls_d), (_, drf_g) = outs
    ops.dhead_losses(dev(rf), dev(cls), loss, drf_d, dcls_d, drf_g, B, npatch, T, ops.XENT_TF_FUSED if mode == "executed" else ops.XENT_INTENDED)
    L = host(loss)
    got = (host(drf_d), host(dcls_d), host(drf_g))
    assert all(R.guard_intact(raw, p) for raw, p in outs)
    assert np.isfinite(L).all() and all(np.isfinite(g).all() for g in got)
    figs = (rel_l2(got[0], o.gd_rf), rel_l2(got[1], o.gd_cls), rel_l2(got[2], o.gg_rf), rel_l2(L[:9], o.slots))
    print(f"dhead B={B} np={npatch} T={T} {mode}: rel_l2 drf_d / dcls_d / drf_g / slots {figs}")
    assert (L[9:] == 0.0).all()
    assert max(figs) < R.DHEAD_TOL
    return o


@pytest.mark.parametrize("mode", ["executed", "intended"])
@pytest.mark.parametrize("T", [0.8, 1.2])
@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("npatch", R.DHEAD_NPATCH)
def test_dhead_losses_patch_counts(npatch, B, T, mode):
    """1, 63, 64, 65 and 200 patches on 64 lanes: the patch loop runs once with idle lanes, once exactly, twice and four times."""
    rf, cls = R.dhead_case(B, npatch)
    _dhead(rf, cls, B, npatch, T, mode)


@pytest.mark.parametrize("mode", ["executed", "intended"])
def test_dhead_losses_large_logits(mode):
    """class logits scaled to +-80 (every row holds +80 and -80): the oracle's log_softmax stays finite, and so must every output"""
    B, npatch = 2, 65
    rf, cls = R.dhead_case(B, npatch, scale=0.0)
    rng = np.random.default_rng(80)
    cls = R.r32(rng.uniform(-80.0, 80.0, cls.shape))
    i = np.arange(cls.shape[0])
    cls[i, i % 5], cls[i, (i + 2) % 5] = 80.0, -80.0
    o = _dhead(rf, cls, B, npatch, 1.2, mode)
    assert np.isfinite(o.gd_cls).all() and np.isfinite(o.slots).all()
