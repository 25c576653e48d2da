"""The first-layer gradient stencil -- shm_sum_input_channels and shm_conv3x3_dgrad_sum1 in its plain, tiled and eight MFMA forms -- and the
helpers round it (shm_transpose_taps, shm_transpose_taps_multi, shm_mask_pool_pack(_hw), shm_add_bcast, shm_sum_groups, shm_mul_mask)
against float64 / bit-exact float32 references at the shapes test_ops_gpu.py's, test_rect_gpu.py's and test_attention_gpu.py's friendly ones
leave out: partial 16 x 16 tiles, odd sides at stride 2 (pad_before = 1), maps below one tile, a channel pitch wider than c with NaN in the
gap, accumulation onto a loaded `out` and plain stores onto NaN, three samples of two tensors, empty calls, +Inf where the MFMA form's masked
lanes read.

Cases and references come from stencil_edge_ref.py; test_stencil_edges_cpu.py proves that each case is in the branch it claims and derives
the per-pixel constants.  The stencil is held to two conditions: rel-L2 < 1e-5 against float64, and |got - ref| <= k * A pixel by pixel, A
the same stencil of |dz| and |weff| -- one wrong border pixel cannot hide in a whole-map norm.  Every output lies between two guard bands
that must come back untouched.  Each check prints its figures before it asserts.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import stencil_edge_ref as R
from util import dev, host

pytestmark = pytest.mark.gpu
NAN = float("nan")


def _ops():
    from shmgan_amd import ops
    return ops


def _lib():
    from shmgan_amd._lib import lib
    return lib()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _out(n, dtype=torch.float32):
    return R.guarded2(n, dtype, "cuda")


def _f32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def _typed(a32, dt):
    """float32 values (already representable in dt) as a device tensor of the call's dtype"""
    return _f32(a32).to(R.TORCH[dt])


# -------------------------------------------------------------------------------------------------------------- shm_conv3x3_dgrad_sum1
def _dz(k):
    """dz of case k at its pitch; the gap [c, ld) of every pixel holds NaN (a read of it shows in the result)"""
    sc = k.sc
    t = torch.full((sc.nk * sc.batch * k.ho * k.wo, k.ld), NAN, dtype=torch.float32)
    t[:, :sc.c] = torch.from_numpy(np.ascontiguousarray(k.dz, dtype=np.float32)).view(-1, sc.c)
    return t.to(R.TORCH[sc.dt]).cuda()


def _stencil(k, dzd, wd, accumulate):
    """one call: a loaded `out` (accumulating) or one full of NaN (a pixel the call does not store stays NaN); returns (rel-L2, |err| / A)"""
    sc = k.sc
    raw, out = _out(sc.batch * sc.h * sc.w)
    out.copy_(_f32(k.out0).view(-1) if accumulate else torch.full_like(out, NAN))
    _ops().conv3x3_dgrad_sum1(dzd, k.ld, wd, out, sc.nk, sc.batch, sc.h, sc.w, sc.c, sc.stride, accumulate)
    got = host(out).reshape(sc.batch, sc.h, sc.w)
    assert R.guards_intact(raw, out), (sc, accumulate, "a store in front of or behind out")
    ref, A = R.stencil_expect(k, accumulate)
    return R.stencil_figs(got, ref, A)


def _stencil_case(sc, inf=False):
    k = R.stencil_case(sc, inf)
    dzd, wd = _dz(k), dev(k.weff)
    kk = R.stencil_k(sc)
    worst = [0.0, 0.0]
    for accumulate in (0, 1):
        rel, ratio = _stencil(k, dzd, wd, accumulate)
        print(f"  {R.form_of(sc.dt, sc.nk, sc.c)} batch={sc.batch} {sc.h}x{sc.w} s{sc.stride} ld={k.ld} acc={accumulate} inf={inf}: "
              f"rel_l2 {rel:.3g} (bound {R.STENCIL_TOL:g}), |err|/A {ratio:.3g} (bound {kk:.3g})")
        assert R.stencil_ok((rel, ratio), kk), (sc, accumulate, rel, ratio)
        worst = [max(worst[0], rel), max(worst[1], ratio)]
    return worst


@pytest.mark.parametrize("dt,nk,c", R.FORMS, ids=lambda v: str(v))
def test_stencil_edges(dt, nk, c):
    """every geometry of the form's table (all thirteen for the first form of a kernel and dtype, five for the others): sides astride the
    16-pixel tile, odd sides at stride 2, 1 x 1 and 2 x 2 maps, batch 1 to 3, tight and wide pitch, both accumulate modes"""
    worst = [0.0, 0.0]
    for sc in R.form_cases(dt, nk, c):
        w = _stencil_case(sc)
        worst = [max(worst[0], w[0]), max(worst[1], w[1])]
    print(f"{R.form_of(dt, nk, c)} nk={nk} c={c}: worst rel_l2 {worst[0]:.3g}, worst |err|/A {worst[1]:.3g} = {worst[1] / R.stencil_k(R.SC(dt, nk, c, 1, 1, 1, 1, False)):.2f} of the bound")


@pytest.mark.parametrize("sc", R.NONFINITE, ids=lambda sc: f"{sc.dt}-nk{sc.nk}-c{sc.c}-{sc.h}x{sc.w}-s{sc.stride}")
def test_stencil_nonfinite_under_the_masked_lanes(sc):
    """one channel of dz pixel (0, 0) of every tensor is +Inf -- the pixel the MFMA form's lanes without a pixel load, and the plain
    kernel's dead threads: the result is non-finite at exactly the (two by two) pixels whose stencil covers (0, 0) and within both bounds
    everywhere else"""
    _stencil_case(sc, inf=True)


@pytest.mark.parametrize("dt,nk,c", [("f32", 5, 64), ("bf16", 5, 64), ("f32", 2, 16), ("bf16", 6, 64)])
def test_stencil_empty_calls_write_nothing(dt, nk, c):
    """nk = 0 and batch = 0: SHM_OK, `out` and its guard bands untouched"""
    k = R.stencil_case(R.SC(dt, nk, c, 2, 17, 16, 1, False))
    dzd, wd = _dz(k), dev(k.weff)
    raw, out = _out(2 * 17 * 16)
    _ops().conv3x3_dgrad_sum1(dzd, c, wd, out, 0, 2, 17, 16, c, 1, 0)
    _ops().conv3x3_dgrad_sum1(dzd, c, wd, out, nk, 0, 17, 16, c, 1, 0)
    _ops().conv3x3_dgrad_sum1(dzd, c, wd, out, nk, 0, 17, 16, c, 2, 1)
    torch.cuda.synchronize()
    assert R.untouched(raw)


# ------------------------------------------------------------------------------------------------------------- shm_sum_input_channels
@pytest.mark.parametrize("cin", R.SUMCH_CIN)
def test_sum_input_channels_edges(cin):
    """cin = 1 .. 32 x cout = 1 .. 64 (9 * cout below, astride and beyond one block) x masks: none, the whole word, the channels alone, the
    top channel (bit 31 at cin = 32), a pattern with ignored bits set; |err| <= 32 * 2^-24 * sum |w_j| per element"""
    ops = _ops()
    for cout in R.SUMCH_COUT:
        w = R.sumch_case(cin, cout)
        wd = dev(w)
        for mask in R.sumch_masks(cin):
            raw, weff = _out(9 * cout)
            ops.sum_input_channels(wd, cin, cout, mask, weff)
            got = host(weff).reshape(9, cout)
            assert R.guards_intact(raw, weff), (cin, cout, mask)
            ref, a = R.sumch_ref(w, mask)
            err, bound = np.abs(got - ref), R.SUMCH_UNIT * a
            print(f"sum_input_channels cin={cin} cout={cout} mask={mask:#x}: worst |err| {err.max():.3g}, worst |err| / bound {np.max(err / np.maximum(bound, 1e-300)):.3g}")
            assert (err <= bound).all(), (cin, cout, mask)


# ------------------------------------------------------------------------------------------------------------------------- transposes
def _transpose_check(what, wt, w, shape, dt):
    ntaps, rows, cols, rp = shape
    ref = R.transpose_ref(w, rp)
    got = R.bits(wt).reshape(ntaps, cols, rp)
    diff = int((got != R.to_dtype_bits(ref, dt)).sum())
    pad = int((got[:, :, rows:] != 0).sum())
    print(f"{what} {shape} {dt}: differing elements {diff}, padding elements not +0.0: {pad}")
    assert diff == 0 and pad == 0, (what, shape, dt)


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_transpose_taps_against_numpy(dt):
    """both entry points against np.transpose plus zero padding, bit for bit (bf16: after round to nearest even): shapes off the 32 x 32
    tile on either side, whole tiles of padding, 1 x 1; 48 layers of mixed shapes in one launch, the limit; none"""
    ops = _ops()
    for i, shape in enumerate(R.TRANSPOSE_SHAPES):
        ntaps, rows, cols, rp = shape
        w = R.transpose_case(i, shape)
        raw, wt = _out(ntaps * cols * rp, R.TORCH[dt])
        ops.transpose_taps(_f32(w), wt, ntaps, rows, cols, rp)
        _transpose_check("transpose_taps", wt, w, shape, dt)
        assert R.guards_intact(raw, wt), shape
    items, keep = [], []
    for i in range(R.TRANSPOSE_MAX):
        shape = R.TRANSPOSE_SHAPES[(i * 5 + i // 6) % len(R.TRANSPOSE_SHAPES)]
        ntaps, rows, cols, rp = shape
        w = R.transpose_case(100 + i, shape)
        raw, wt = _out(ntaps * cols * rp, R.TORCH[dt])
        items.append((_f32(w), wt, ntaps, rows, cols, rp))
        keep.append((raw, wt, w, shape))
    assert len({s for *_, s in keep}) == len(R.TRANSPOSE_SHAPES)
    batch = ops.TransposeBatch(items)
    batch.run()
    for raw, wt, w, shape in keep:
        _transpose_check("transpose_taps_multi", wt, w, shape, dt)
        assert R.guards_intact(raw, wt), shape
    # count = 0 with live tables: SHM_OK, nothing written
    raws = []
    for j, it in enumerate(items[:3]):
        raw, wt = _out(it[2] * it[4] * it[5], R.TORCH[dt])
        batch.wt[j] = wt.data_ptr()
        raws.append((raw, wt))
    assert _lib().shm_transpose_taps_multi(0, batch.w, batch.wt, batch.ntaps, batch.rows, batch.cols, batch.rows_pad, batch.dt, _stream()) == 0
    torch.cuda.synchronize()
    assert all(R.untouched(raw) for raw, _ in raws)


# ------------------------------------------------------------------------------------------------------ attention helpers, dropout multiply
@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_mask_pool_pack_edges(dt):
    """k = 1, 2, 3, 5, 8, squares and rectangles with fewer and more output pixels than one block, masks of mixed sign and negative
    everywhere, lddst = 1, 16, 20, 32: channel 0 the window's maximum, the other channels +0.0, bit for bit"""
    ops = _ops()
    for square, cases in ((True, R.POOL_SQUARE), (False, R.POOL_HW)):
        for case in cases:
            b, h, w, k = (case[0], case[1], case[1], case[2]) if square else case
            for neg in (False, True):
                m = R.pool_mask(b, h, w, neg)
                md = _f32(m)
                for ld in R.POOL_LD:
                    raw, dst = _out(b * (h // k) * (w // k) * ld, R.TORCH[dt])
                    view = dst.view(b, h // k, w // k, ld)
                    if square:
                        ops.mask_pool_pack(md, view, b, h, k)
                    else:
                        ops.mask_pool_pack_hw(md, view, b, h, w, k)
                    diff = int((R.bits(dst) != R.to_dtype_bits(R.pool_ref(m, k, ld), dt).reshape(-1)).sum())
                    if ld == R.POOL_LD[-1]:
                        print(f"mask_pool_pack{'' if square else '_hw'} B={b} {h}x{w} k={k} negative={neg} {dt}: differing elements {diff}")
                    assert diff == 0 and R.guards_intact(raw, dst), (case, neg, ld)


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_add_bcast_and_sum_groups_edges(dt):
    """per = 4 and per / 4 = 77 (no divisor of 256), one sample, more samples than images (groups that receive nothing: zero, or unchanged
    when accumulating), i0 >= nb, no image at all; a single add and a sum in ascending image order: bit for bit against float32 (bf16
    rounded to nearest even at the end)"""
    ops = _ops()
    for case in R.BCAST_CASES:
        nimg, per, nb, i0 = case
        k = R.bcast_case(case, dt)
        rows = max(nimg, 1)          # nimg = 0: the pointers stay valid, the count says there is nothing
        ad = torch.zeros((rows, per), dtype=R.TORCH[dt], device="cuda")
        ad[:nimg] = _typed(k.a, dt)
        bd, d0 = _typed(k.b, dt), _typed(k.d0, dt)
        raw, out = _out(rows * per, R.TORCH[dt])
        ops.add_bcast(ad, bd, out, nimg, per, nb, i0)
        torch.cuda.synchronize()
        diff = int((R.bits(out)[:nimg * per] != R.to_dtype_bits(R.add_bcast_ref(k.a, k.b, nb, i0), dt).reshape(-1)).sum())
        print(f"add_bcast {case} {dt}: differing elements {diff}")
        assert diff == 0 and R.guards_intact(raw, out), case
        assert bool((out.view(torch.uint8)[nimg * per * out.element_size():] == R.SENT_BYTE).all().item()), case          # nothing behind image nimg - 1
        for accumulate in (False, True):
            raw, dst = _out(nb * per, R.TORCH[dt])
            dst.copy_(d0.view(-1))
            ops.sum_groups(ad, dst, nimg, per, nb, i0, accumulate)
            diff = int((R.bits(dst) != R.to_dtype_bits(R.sum_groups_ref(k.a, k.d0, nb, i0, accumulate), dt).reshape(-1)).sum())
            print(f"sum_groups {case} accumulate={accumulate} {dt}: differing elements {diff}")
            assert diff == 0 and R.guards_intact(raw, dst), (case, accumulate)


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_mul_mask_edges(dt):
    """n / 4 = 100, 256 and 3 * 256 + 77 vectors: (x * mask) * scale in float32, bit for bit"""
    ops = _ops()
    for n in R.MULMASK_N:
        x, m = R.mulmask_case(n, dt)
        raw, y = _out(n, R.TORCH[dt])
        ops.mul_mask(_typed(x, dt), _f32(m), y, n, R.MULMASK_SCALE)
        diff = int((R.bits(y) != R.to_dtype_bits(R.mulmask_ref(x, m, R.MULMASK_SCALE), dt)).sum())
        print(f"mul_mask n={n} {dt}: differing elements {diff}")
        assert diff == 0 and R.guards_intact(raw, y), n
