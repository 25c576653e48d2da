"""The InstanceNorm and LeakyReLU passes on ragged multi-block grids: every pass that splits a sample's pixels with pix_chunks() (csrc/elem.h), at the
smallest maps where a sample takes several blocks AND the last chunk is shorter AND a chunk is no multiple of the pixel slots, where threads idle,
where the interleaved bf16 tiles leave pixels over, where a pooled chunk starts inside a row of the half-size map and where lrelu_bwd has more
blocks than staging slots -- under every "elem.*" scheduling knob.  The header promises of those knobs: "Knobs change scheduling only, never
results beyond the summation order".

The cases are the rows of geom_ref.FWD / BWD / LRELU; test_elem_geometry_cpu.py holds every row to the geometry class it is there for, at the knob
values it sets, and shows that the checks below fail on modelled partition faults.  What a case asserts (every bound from elem_bound_ref.py, the
statistics' from stats_ref.py; no constant of its own):

  * every output lies between two guard bands of at least one chunk of pixel rows, all filled with util.SENTINEL like the output itself: the bands
    are untouched, and an unwritten element fails its bound;
  * in_apply, in_apply_pool, in_pool, avgpool2_fwd: element by element within eb.in_apply_ref_tol / eb.in_pool_ref_tol, torch.equal to the same
    call at default knobs (they are per-element expressions), in_apply_pool equal to in_apply + avgpool2_fwd, in_pool equal to its pooled output;
  * in_stats: mean and inv against float64 on the device's operands at the bound of test_stats_conditioning_gpu.py::test_offset_ladder_in_stats
    (stats_ref.onepass_bound at depth 0), under every knob setting (the sums are float64 atomics: no bit equality);
  * in_bwd, in_bwd_rank1 (two passes: fused=None), in_bwd_apply: dz within eb.in_bwd_ref_tol, the bias gradient and the per-sample dz sums within
    eb.in_sum_tol (eb.hold_in_bwd), `red` / `redp` / `dstage` exactly zero on return, shm_last_kernel() the pair expected of the row.
    in_bwd_apply takes its sums from the caller: they are formed here in float64 and spread over three of the SHM_GSUM_SLOTS slots, and the
    statistics of those rows are rounded to fp32 values first -- the kernel forms m2 from the float64 statistics and dz from their float casts, and
    the bound knows one pair (mean_f, inv_f);
  * lrelu_bwd: dz bit-equal to where(y > 0, dy, dy * slope) in fp32, rounded once to the output type; the bias gradient within
    gamma(npix) sum|dz| of the float64 sum; `red` zero on return.
"""
import functools

import numpy as np
import pytest
import torch

import elem_bound_ref as eb
import geom_ref as gr
import stats_ref as sr
from util import SENTINEL, host

pytestmark = pytest.mark.gpu
BF, F32 = torch.bfloat16, torch.float32
SLOPE = 0.2
EPS_ARG = 1e-6


def _ops():
    from shmgan_amd import ops
    return ops


@pytest.fixture(autouse=True)
def _reset_tuning():
    yield
    _ops().set_tuning("reset", 0)


def _set(knobs):
    for key, val in knobs.items():
        _ops().set_tuning(key, val)


def _adt(dt):
    return F32 if dt == gr.F32 else BF


def _gdt(dt):
    return BF if dt == gr.BF16 else F32


def _out(dt):
    return "f32" if dt == gr.F32 else "bf16"


class Guarded:
    """`rows` pixel rows of c elements between two guard bands of at least `guard` pixel rows, everything filled with SENTINEL.  The bands are
    whole multiples of 8 rows, so the body starts on a 16-byte boundary for every c."""

    def __init__(self, rows, c, dtype, guard):
        guard = gr.cdiv(guard, 8) * 8
        self.flat = torch.full(((2 * guard + rows) * c,), SENTINEL, dtype=dtype, device="cuda")
        self.lo, self.hi = guard * c, (guard + rows) * c
        self.t = self.flat[self.lo:self.hi]
        assert self.t.data_ptr() % 16 == 0

    def intact(self):
        return bool((self.flat[:self.lo] == SENTINEL).all()) and bool((self.flat[self.hi:] == SENTINEL).all())


def _chunk(names, row, dt):
    return max(gr.pass_geometry(nm, dt, row["batch"], row["h"], row["w"], row["c"], row["knobs"])["chunk"] for nm in names)


def _act(rng, n, h, w, c):
    return rng.standard_normal((n, h, w, c)) * rng.uniform(0.5, 2.0, (n, 1, 1, c)) + rng.uniform(-1, 1, (n, 1, 1, c))


def _dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda().to(dtype)


def _hold_stats(a, stats, n, hw, c, dt):
    """test_stats_conditioning_gpu.py::_check_ladder's first two assertions: float64 from the first addition (depth 0), hw + 16 float64 additions"""
    mu, var = sr.moments64(a.float().view(n, hw, c))
    dmean, _, dinv = sr.onepass_bound(mu, np.sqrt(var), sr.CHAIN["in_stats"](), n64=hw + 16)
    s = host(stats).reshape(n, c, 2)
    em = np.abs(s[..., 0] - mu)
    ei = np.abs(s[..., 1] / sr.inv_ref(var) - 1.0)
    print(f"in_stats {dt}: mean error / bound {float((em / dmean).max()):.3f}, inv error / bound {float((ei / dinv).max()):.3f}")
    assert (em <= dmean).all(), float((em / dmean).max())
    assert (ei <= dinv).all(), float((ei / dinv).max())
    eb.note("in_stats ragged", _out(dt), max(float((em / dmean).max()), float((ei / dinv).max())))


# =====================================================================================================================
# forward
@functools.lru_cache(maxsize=None)
def _fwd_base(n, h, w, c, dt):
    """operands, and at DEFAULT knobs: the statistics, in_apply's result, its float64 reference and bound, the bound of the pooled map"""
    ops = _ops()
    ops.set_tuning("reset", 0)
    rng = np.random.default_rng(1000 + 7 * h + w + c)
    adt, hw = _adt(dt), h * w
    a = _dev(_act(rng, n, h, w, c), adt)
    beta = _dev(rng.standard_normal(c) * 0.02, F32)
    stats = torch.full((n * c * 2,), SENTINEL, dtype=torch.float64, device="cuda")
    ops.in_stats(a, c, stats, n, hw, c, EPS_ARG)
    y = torch.full((n, h, w, c), SENTINEL, dtype=adt, device="cuda")
    ops.in_apply(a, c, stats, beta, y, c, n, hw, c)
    torch.cuda.synchronize()
    yref, ytol = eb.in_apply_ref_tol(host(a.float()), host(stats), host(beta), _out(dt))
    pool = eb.in_pool_ref_tol(host(y.float()), _out(dt)) if h % 2 == 0 and w % 2 == 0 else None
    return {"a": a, "beta": beta, "stats": stats, "y": y, "yref": yref, "ytol": ytol, "pool": pool}


@pytest.mark.parametrize("row,dt", gr.cases(gr.FWD, "fwd")[0], ids=gr.cases(gr.FWD, "fwd")[1])
def test_forward_passes(row, dt):
    ops = _ops()
    n, h, w, c = row["batch"], row["h"], row["w"], row["c"]
    hw, adt, out = h * w, _adt(dt), _out(dt)
    b = _fwd_base(n, h, w, c, dt)
    a, beta = b["a"], b["beta"]
    _set(row["knobs"])
    # the statistics
    stats = torch.full((n * c * 2,), SENTINEL, dtype=torch.float64, device="cuda")
    ops.in_stats(a, c, stats, n, hw, c, EPS_ARG)
    torch.cuda.synchronize()
    _hold_stats(a, stats, n, hw, c, dt)
    # apply (with the statistics of the default run: the same operands whatever the knobs)
    ch = _chunk(("apply",), row, dt)
    y = Guarded(n * hw, c, adt, ch)
    ops.in_apply(a, c, b["stats"], beta, y.t, c, n, hw, c)
    torch.cuda.synchronize()
    assert y.intact()
    y4 = y.t.view(n, h, w, c)
    eb.note("in_apply ragged", out, eb.within(host(y4.float()), b["yref"], b["ytol"], {"kind": "in", "chunk": ch}, "in_apply"))
    assert torch.equal(y4, b["y"])
    if b["pool"] is None:
        return
    # apply + pool, pool alone, the separate pooling pass
    hq, chq = hw // 4, _chunk(("pool",), row, dt)
    y2, p2, p3, p4 = Guarded(n * hw, c, adt, 4 * chq + 2 * w), Guarded(n * hq, c, adt, chq), Guarded(n * hq, c, adt, chq), Guarded(n * hq, c, adt, chq)
    ops.in_apply_pool(a, c, b["stats"], beta, y2.t, c, p2.t, c, n, h, w, c)
    ops.in_pool(a, c, b["stats"], beta, p3.t, c, n, h, w, c)
    ops.avgpool2_fwd(y.t, c, p4.t, c, n, h, w, c)
    torch.cuda.synchronize()
    assert y2.intact() and p2.intact() and p3.intact() and p4.intact()
    assert torch.equal(y2.t, y.t)
    pref, ptol = b["pool"]
    where = {"kind": "in", "chunk": chq}
    eb.note("in_apply_pool ragged", out, eb.within(host(p2.t.float()).reshape(pref.shape), pref, ptol, where, "in_apply_pool"))
    eb.note("avgpool2_fwd ragged", out, eb.within(host(p4.t.float()).reshape(pref.shape), pref, ptol, where, "avgpool2_fwd"))
    assert torch.equal(p2.t, p4.t), "in_apply_pool != in_apply + avgpool2_fwd"
    assert torch.equal(p3.t, p2.t), "in_pool != in_apply_pool's pooled output"


# =====================================================================================================================
# backward
@functools.lru_cache(maxsize=None)
def _bwd_operands(n, h, w, c, dt):
    ops = _ops()
    ops.set_tuning("reset", 0)
    rng = np.random.default_rng(2000 + 7 * h + w + c + n)
    adt, gdt = _adt(dt), _gdt(dt)
    o = {"a": _dev(_act(rng, n, h, w, c), adt), "g": _dev(rng.standard_normal((n, h, w, c)), gdt), "g2": None,
         "hdz": _dev(rng.standard_normal((n, h, w)), F32), "hw": _dev(rng.standard_normal(c), F32), "beta": _dev(rng.standard_normal(c) * 0.02, F32)}
    if h % 2 == 0 and w % 2 == 0:
        o["g2"] = _dev(rng.standard_normal((n, h // 2, w // 2, c)), gdt)
    o["stats"] = torch.zeros(n * c * 2, dtype=torch.float64, device="cuda")
    ops.in_stats(o["a"], c, o["stats"], n, h * w, c, EPS_ARG)
    torch.cuda.synchronize()
    o["stats32"] = o["stats"].float().double()
    return o


def _slot_sums(o, n, h, w, c, pooled, stats):
    """shm_in_bwd_apply's inputs, float64 on the host: red[slot][n][c] = (sum g1, sum g1 a); redp = (sum g2, sum g2 pooled), pooled = avgpool(xh) + beta.
    Halves and quarters over three slots: the slots' sum is the whole, exactly."""
    ops = _ops()
    A, G = o["a"].double().cpu(), o["g"].double().cpu()

    def spread(s):
        r = torch.zeros(ops.GSUM_SLOTS, n, c, 2, dtype=torch.float64)
        r[0], r[3], r[ops.GSUM_SLOTS - 1] = 0.5 * s, 0.25 * s, 0.25 * s
        return r.reshape(-1).cuda()

    red = spread(torch.stack([G.sum((1, 2)), (G * A).sum((1, 2))], -1))
    if not pooled:
        return red, None
    st = stats.cpu().view(n, c, 2)
    xh = (A - st[:, :, 0].view(n, 1, 1, c)) * st[:, :, 1].view(n, 1, 1, c)
    P = xh.view(n, h // 2, 2, w // 2, 2, c).mean((2, 4)) + o["beta"].double().cpu()
    G2 = o["g2"].double().cpu()
    return red, spread(torch.stack([G2.sum((1, 2)), (G2 * P).sum((1, 2))], -1))


@pytest.mark.parametrize("row,dt", gr.cases(gr.BWD, "bwd")[0], ids=gr.cases(gr.BWD, "bwd")[1])
def test_backward_passes(row, dt):
    ops = _ops()
    n, h, w, c = row["batch"], row["h"], row["w"], row["c"]
    hw, adt, out = h * w, _adt(dt), _out(dt)
    form, _, extra = row["form"].partition("+")
    o = _bwd_operands(n, h, w, c, dt)
    a = o["a"]
    pooled, rank1, raw = form.endswith("pooled"), form == "rank1", form.startswith("raw")
    g2 = o["g2"] if pooled else None
    if row["split"] is not None:          # "elem.chunk_mb": the split follows from the sizes (csrc/instnorm_bwd.hip: in_bwd_plan)
        assert gr.sample_chunks(dt, n, h, w, c, pooled, rank1, row["knobs"]["elem.chunk_mb"]) == row["split"]
    _set(row["knobs"])
    ch = _chunk(gr.row_passes(row, "bwd"), row, dt)
    dz = Guarded(n * hw, c, adt, ch)
    db = torch.zeros(c, dtype=torch.float64, device="cuda") if extra else None
    keep = torch.full((n, c), SENTINEL, dtype=torch.float64, device="cuda") if extra == "s" else None
    if raw:
        stats = o["stats32"]
        red, redp = _slot_sums(o, n, h, w, c, pooled, stats)
        dstage = torch.zeros(n * c, dtype=torch.float64, device="cuda") if extra else None
        ops.in_bwd_apply(o["g"], c, g2, c if pooled else 0, a, c, stats, o["beta"], red, redp, dstage, dz.t, c, db, n, h, w, c, SLOPE, dz_sums=keep)
        kern = "in_bwd_apply_kernel, sums given"
        torch.cuda.synchronize()
        assert float(red.abs().max()) == 0.0 and (redp is None or float(redp.abs().max()) == 0.0) and (dstage is None or float(dstage.abs().max()) == 0.0)
    else:
        stats = o["stats"]
        red = torch.zeros(n * c * 3, dtype=torch.float64, device="cuda")
        if rank1:
            ops.in_bwd_rank1(o["hdz"], o["hw"], a, c, stats, red, dz.t, c, db, n, h, w, c, SLOPE, dz_sums=keep)
        else:
            ops.in_bwd(o["g"], c, g2, c if pooled else 0, a, c, stats, red, dz.t, c, db, n, h, w, c, SLOPE, fused=None, dz_sums=keep)
        kern = ops.last_kernel()
        torch.cuda.synchronize()
        assert kern == gr.expected_pair(dt, c), kern
        assert float(red.abs().max()) == 0.0
    assert dz.intact()
    worst = eb.hold_in_bwd([(dz.t.view(n, h, w, c), db, keep, kern)], a, stats, None if rank1 else o["g"], g2, o["hdz"] if rank1 else None,
                           o["hw"] if rank1 else None, SLOPE, out, {"kind": "in", "chunk": ch})
    fam = "in_bwd ragged " + ("gf32 " if dt == gr.GF32 else "") + ("apply alone" if raw else "rank-1" if rank1 else "reduce8" if "reduce8" in kern else "reduce4")
    eb.note(fam, out, worst[kern])


# =====================================================================================================================
# LeakyReLU backward
@pytest.mark.parametrize("row,dt", gr.cases(gr.LRELU, "lrelu")[0], ids=gr.cases(gr.LRELU, "lrelu")[1])
def test_lrelu_bwd(row, dt):
    ops = _ops()
    assert ops.LRELU_RED_SLOTS == gr.LRELU_RED_SLOTS
    npix, c = row["batch"] * row["h"] * row["w"], row["c"]
    adt, gdt = _adt(dt), _gdt(dt)
    rng = np.random.default_rng(3000 + c)
    y = _dev(rng.standard_normal((npix, c)), adt)
    dy = _dev(rng.standard_normal((npix, c)), gdt)
    ch = _chunk(("lrelu",), row, dt)
    # one rounding: the fp32 product (or the fp32 value itself), rounded once more to the output type
    yc, dyc = y.float().cpu(), dy.float().cpu()
    slope32 = torch.tensor(SLOPE, dtype=torch.float32)
    ref = torch.where(yc > 0, dyc, dyc * slope32).to(adt)
    d64 = torch.where(yc > 0, dyc.double(), dyc.double() * slope32.double()).numpy()          # what the bias gradient sums, before the store rounds it
    for with_bias in (True, False):
        dz = Guarded(npix, c, adt, ch)
        db = torch.zeros(c, dtype=torch.float64, device="cuda") if with_bias else None
        red = torch.zeros(ops.LRELU_RED_SLOTS * c, dtype=torch.float64, device="cuda")
        ops.lrelu_bwd(dy, c, y, c, dz.t, c, db, npix, c, SLOPE, red)
        torch.cuda.synchronize()
        assert dz.intact()
        got = dz.t.view(npix, c).cpu()
        if not torch.equal(got, ref):
            bad = torch.nonzero(got != ref)
            raise AssertionError(f"lrelu_bwd dz: {bad.shape[0]} elements differ, the first at pixel {int(bad[0, 0])} of {npix} (chunk {ch}), channel {int(bad[0, 1])}")
        assert float(red.abs().max()) == 0.0
        if with_bias:
            eb.note("lrelu_bwd bias gradient ragged", _out(dt), eb.within(host(db), d64.sum(0), eb.gamma(npix) * np.abs(d64).sum(0), None, "lrelu_bwd dbias"))
