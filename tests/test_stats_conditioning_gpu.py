"""Fused InstanceNorm statistics (and the gsum sums) on off-centre and non-finite data, for every kernel family that produces them.

The epilogues take their moments in one pass (fp32 `s += v; q = fma(v, v, q)` per lane, float64 across lanes, var = q / hw - mean^2), which
loses (1 + r^2) of the variance's relative accuracy at r = |mean| / std, times the depth of the fp32 part.  The other tests stay at r <~ 2.
Here a bias ladder puts the channels of ONE launch at r = 0, R_WORK, 4, 16, 64, 256 (stats_ref.RUNGS; R_WORK is what the float64 oracle's
step shows), one channel is constant, and the device's (mean, inv) are held, per (sample, channel), to
  * stats_ref.onepass_bound with the family's depth stats_ref.CHAIN -- the rigorous worst case: a correct kernel cannot exceed it, and
    test_stats_conditioning_cpu.py shows that the design stays inside it on these inputs;
  * the project's own tolerance (inv to 1e-5 / 1e-3 for bf16 outputs, the mean to the same figure times |mu| + sigma) wherever r <= R_WORK.
The reference is stats_ref.moments64 of the tensor the kernel stored: no convolution is recomputed.

Second half: one NaN (then one +inf) input element must reach exactly its receptive field in the output, every channel, the poisoned
sample's statistics / sums, and nothing else (the abort logic and nonfinite="raise" rely on it on every path).

Each case forces its variant and asserts shm_last_kernel(), as test_variants_gpu.py does.  The RGB first layer is covered through the
default path only: the forced generic kernels read the compact 3-channel pixel against zero weight columns (conv_igemm.hip), where
NaN * 0 widens the footprint by design.
"""
import numpy as np
import pytest
import torch

import stats_ref as sr
from oracle import step_torch as st
from util import conv_ref, host, nchw, nhwc, pad_c, t64

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
TNAME = {"f32": "float", "bf16": "__bf16"}
EPS_ARG = 1e-6


def _ops():
    from shmgan_amd import ops
    return ops


@pytest.fixture(autouse=True)
def _reset_tuning():
    yield
    _ops().set_tuning("reset", 0)


def _ncu():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _t(a, dt):
    t = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()
    return t.to(BF) if dt == "bf16" else t


def _rnd(a, dt):
    """the operand as the device holds it (float64)"""
    return host(_t(a, dt).float())


def _wk(w_hwio, cin_pad, dt):
    ops = _ops()
    k, _, cin, cout = w_hwio.shape
    wt = torch.zeros(k * k * cout * cin_pad, device="cuda", dtype=BF if dt == "bf16" else torch.float32)
    ops.transpose_taps(torch.from_numpy(np.ascontiguousarray(w_hwio, dtype=np.float32)).cuda(), wt, k * k, cin, cout, cin_pad)
    return wt


def _bits(y):
    return np.ascontiguousarray(y.float().cpu().numpy()).view(np.uint32)


# ---------------------------------------------------------------------------------------------------------------------------------------
# the statistics-producing forward families at their smallest shapes.  chain(ncu) -> depth of the fp32 part (stats_ref.CHAIN)

class Fwd:
    def __init__(self, name, variant, dts, n, h, w, cin, cout, s, kernel, chain, tune=(), rgb=False):
        self.name, self.variant, self.dts, self.n, self.h, self.w, self.cin, self.cout, self.s = name, variant, dts, n, h, w, cin, cout, s
        self.kernel, self.chain, self.tune, self.rgb = kernel, chain, tune, rgb

    def launch(self, dt, x, w, b, slope):
        """x [n, h, w, cin] (numpy or a device tensor in the activation type), w HWIO numpy, b numpy -> (y, stats [n, cout, 2], scratch)"""
        ops = _ops()
        n, h, wi, cout = self.n, self.h, self.w, self.cout
        if self.rgb:                          # the compact image: one 16-byte chunk per pixel
            kpad = 16 if dt == "f32" else 32
            xd = _t(pad_c(np.asarray(x, np.float32), 4 if dt == "f32" else 8), dt)
        else:
            kpad = self.cin
            xd = x if isinstance(x, torch.Tensor) else _t(x, dt)
        ho, wo = h // self.s, wi // self.s
        y = torch.full((n, ho, wo, cout), 9.0, device="cuda", dtype=BF if dt == "bf16" else torch.float32)
        stats = torch.empty(n * cout * 2, dtype=torch.float64, device="cuda")
        scr = torch.zeros(ops.STATS_SLOTS * n * cout * 2, dtype=torch.float64, device="cuda")
        for key, val in self.tune:
            ops.set_tuning(key, val)
        if self.variant:
            ops.set_tuning("tapgemm.variant", self.variant)
        ops.conv2d_in_fwd(xd, None, 0, xd.shape[-1], 0, _wk(w, kpad, dt), torch.from_numpy(np.asarray(b, np.float32)).cuda(), y, cout, n, h, wi, kpad, cout,
                          3, self.s, slope, stats, EPS_ARG, scratch=scr)
        torch.cuda.synchronize()
        k = ops.last_kernel()
        want = self.kernel.format(t=TNAME[dt])
        assert k.startswith(want) if want.endswith("<") else k == want, (k, want)
        ops.set_tuning("reset", 0)
        return y, host(stats).reshape(n, cout, 2), scr


def _dma(tile, sym):
    return dict(kernel="tapgemm_dma_kernel<{t}, {t}, " + sym + ">", chain=lambda ncu, dt: sr.CHAIN[tile]())


BOTH = ("f32", "bf16")
FWD = [
    Fwd("dma128x128", "dma128x128", BOTH, 2, 16, 16, 64, 128, 1, **_dma("dma128x128", "128, 128, 2, 2, 3, 16")),
    Fwd("dma64x64", "dma64x64", BOTH, 2, 16, 16, 64, 128, 1, **_dma("dma64x64", "64, 64, 2, 2, 3, 16")),
    Fwd("dma256x128", "dma256x128", BOTH, 2, 16, 16, 64, 128, 1, **_dma("dma256x128", "256, 128, 4, 2, 3, 16")),
    Fwd("dma128x128_s2", "dma128x128", BOTH, 2, 32, 32, 64, 128, 2, **_dma("dma128x128", "128, 128, 2, 2, 3, 16")),
    Fwd("halo128_st", "halo128_st", BOTH, 2, 32, 32, 64, 160, 1, "tapgemm_halo_kernel<{t}, {t}, 128, 16, true, 2>", lambda ncu, dt: sr.CHAIN["halo128_st"]()),
    Fwd("halo64_st", "halo64_st", BOTH, 2, 32, 32, 64, 160, 1, "tapgemm_halo_kernel<{t}, {t}, 64, 16, true, 2>", lambda ncu, dt: sr.CHAIN["halo64_st"]()),
    Fwd("wreg_f32", "wreg", ("f32",), 3, 16, 16, 64, 64, 1, "tapgemm_wreg_f32_kernel<4, 4, false>", lambda ncu, dt: sr.CHAIN["wreg_f32"]()),
    Fwd("wreg4", "wreg", ("bf16",), 3, 16, 16, 64, 64, 1, "tapgemm_wreg_kernel<__bf16, 2>",
        lambda ncu, dt: sr.CHAIN["wreg"](per=sr.wreg_per(3, 16, 16, 64, ncu)), tune=(("tapgemm.wreg16", 0),)),
    Fwd("wreg16", "wreg", ("bf16",), 3, 16, 16, 64, 64, 1, "tapgemm_wreg16_bf16_kernel<2, true>",
        lambda ncu, dt: sr.CHAIN["wreg16"](per=sr.wreg_per(3, 16, 16, 64, ncu)), tune=(("tapgemm.wreg16", 1),)),
    Fwd("pingpong", "wreg", ("bf16",), 3, 16, 32, 64, 64, 1, "tapgemm_pp_bf16_kernel<2>",
        lambda ncu, dt: sr.CHAIN["pingpong"](per=sr.pp_per(3, 16, 32, 64, ncu)), tune=(("tapgemm.wreg16", 2),)),
    Fwd("rgb", None, BOTH, 3, 32, 32, 3, 64, 2, "conv3x3s2_rgb_fwd_kernel<", lambda ncu, dt: sr.CHAIN["rgb"](gpw=sr.rgb_groups_per_wave(3, 16, 16, dt)), rgb=True),
    Fwd("f32_split", "halo128_st", ("f32",), 2, 32, 32, 64, 160, 1, "tapgemm_halo_x3_kernel<false, 128>", lambda ncu, dt: sr.CHAIN["x3"](),
        tune=(("conv.f32_split", 1),)),
]
FWD_IDS = [(c, dt) for c in FWD for dt in c.dts]


def _report(tag, rung, r, em, dmean, ei, dinv):
    """worst err / bound per rung, with the r = |mu| / sigma the rung's channels really have in the stored tensor (DESIGN.md 4 quotes these)"""
    cells = []
    for k in range(len(sr.RUNGS)):
        m = rung == k
        m[-1] = False                         # the constant channel has its own checks
        cells.append(f"r {r[:, m].min():.3g}-{r[:, m].max():.3g}: {(em[:, m] / dmean[:, m]).max():.3f}/{(ei[:, m] / dinv[:, m]).max():.3f}")
    print(f"COND {tag}: measured r: err/bound (mean/inv), per rung {sr.RUNGS}: " + "  ".join(cells))


def _check_ladder(tag, y, stats, scr, L, dt, rung):
    yh = y.float().cpu()
    n, c = yh.shape[0], yh.shape[-1]
    hw = yh.numel() // (n * c)
    mu, var = sr.moments64(yh)
    sigma = np.sqrt(var)
    dmean, _, dinv = sr.onepass_bound(mu, sigma, L, n64=hw + 16)
    em = np.abs(stats[..., 0] - mu)
    ei = np.abs(stats[..., 1] / sr.inv_ref(var) - 1.0)
    r = np.abs(mu) / np.where(sigma > 0, sigma, np.inf)
    r[:, -1] = np.inf                         # the constant channel
    _report(tag, rung, r, em, dmean, ei, dinv)
    assert (em <= dmean).all(), (tag, float((em / dmean).max()))
    assert (ei <= dinv).all(), (tag, float((ei / np.maximum(dinv, 1e-300)).max()))
    # what training needs: the project's tolerance wherever r <= r_work.  r is the one MEASURED on the stored tensor; the channels of the
    # rungs 0, 4 and r_work are held too where the spread of sigma (or the slope) leaves their measured r a little above r_work
    work = (r <= sr.R_WORK) | (np.asarray(sr.RUNGS)[rung] <= sr.R_WORK)[None, :]
    work[:, -1] = False
    tol = sr.PROJECT_TOL[dt]
    print(f"COND {tag}: r <= r_work ({int(work.sum())} of {work.size} planes, measured r up to {r[work].max():.3f}): worst inv error {ei[work].max():.2e}, "
          f"mean error / (|mu| + sigma) {(em / (np.abs(mu) + sigma))[work].max():.2e} (tolerance {tol})")
    assert ei[work].max() <= tol, (tag, float(ei[work].max()))
    assert (em[work] <= tol * (np.abs(mu) + sigma)[work]).all(), tag
    # the constant channel: variance clamped at 0, the mean to the chain's rounding
    const = yh[..., -1]
    v0 = float(const.flatten()[0])
    assert bool((const == v0).all()) and v0 != 0.0
    assert (0.0 < stats[:, -1, 1]).all() and (stats[:, -1, 1] <= (1.0 + 1e-12) / np.sqrt(sr.EPS)).all(), stats[:, -1, 1]
    assert (np.abs(stats[:, -1, 0] - v0) <= (sr.gamma(L) + sr.gamma(hw + 18, sr.U64)) * abs(v0)).all(), (stats[:, -1, 0], v0)
    if scr is not None:
        assert float(scr.abs().max()) == 0.0          # "zero on entry, zero on return"


def _ladder_wb(rng, cin, cout):
    w = rng.standard_normal((3, 3, cin, cout)) * 0.1
    w[..., -1] = 0.0                          # the constant channel
    b, rung = sr.ladder_bias(cout, 0.1 * np.sqrt(9 * cin))
    return w, b, rung


def _ladder_operands(c, seed):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((c.n, c.h, c.w, c.cin))
    return (x, *_ladder_wb(rng, c.cin, c.cout))


@pytest.mark.parametrize("slope", [1.0, 0.2])
@pytest.mark.parametrize("case,dt", FWD_IDS, ids=[f"{c.name}-{dt}" for c, dt in FWD_IDS])
def test_offset_ladder(case, dt, slope):
    x, w, b, rung = _ladder_operands(case, 300)
    y, stats, scr = case.launch(dt, x, w, b, slope)
    _check_ladder(f"{case.name} {dt} slope {slope}", y, stats, scr, case.chain(_ncu(), dt), dt, rung)


# ---- long chains: the persistent kernels at n = 24, 128 x 128, 64 -> 64 (3072 / 1536 patches: 6 per block, 3 per ping-pong group)
LONG = [
    ("pingpong", "bf16", (("tapgemm.wreg16", 2),), "tapgemm_pp_bf16_kernel<2>", lambda ncu: sr.CHAIN["pingpong"](per=sr.pp_per(24, 128, 128, 64, ncu))),
    ("wreg16", "bf16", (("tapgemm.wreg16", 1),), "tapgemm_wreg16_bf16_kernel<2, true>", lambda ncu: sr.CHAIN["wreg16"](per=sr.wreg_per(24, 128, 128, 64, ncu))),
    ("wreg4", "bf16", (("tapgemm.wreg16", 0),), "tapgemm_wreg_kernel<__bf16, 2>", lambda ncu: sr.CHAIN["wreg"](per=sr.wreg_per(24, 128, 128, 64, ncu))),
    ("wreg_f32", "f32", (), "tapgemm_wreg_f32_kernel<4, 4, false>", lambda ncu: sr.CHAIN["wreg_f32"]()),
]


def _long_x(c):
    g = torch.Generator(device="cuda").manual_seed(302)
    return torch.randn((c.n, c.h, c.w, c.cin), device="cuda", generator=g)


@pytest.mark.parametrize("name,dt,tune,kernel,chain", LONG, ids=[c[0] for c in LONG])
def test_offset_ladder_long_chains(name, dt, tune, kernel, chain):
    c = Fwd(name, "wreg", (dt,), 24, 128, 128, 64, 64, 1, kernel, None, tune=tune)
    w, b, rung = _ladder_wb(np.random.default_rng(301), c.cin, c.cout)
    x = _long_x(c)
    y, stats, scr = c.launch(dt, x.to(BF) if dt == "bf16" else x, w, b, 0.2)
    _check_ladder(f"long {name} {dt}", y, stats, scr, chain(_ncu()), dt, rung)


# ---- what the worst-case bound cannot see: a chain that GROWS (a persistent kernel that flushes less often, a float atomic).  The typical
# error moves with sqrt(L) and sits at 0.1-1 % of the bound for the bf16 kernels.  Exactly representable sums see it: the identity
# convolution (centre tap, unit weight) stores stats_ref.exact_planes, on which a kernel that folds at most COUNT stored values into one
# fp32 number cannot round while COUNT * V^2 <= 2^16, so (mean, inv) meet the float64 reference to its own roundoff; twice the count
# leaves that range for the planes next to the horizon, and one lost bit moves inv by 1e-7 or more.
EXACT = [
    ("pingpong", "bf16", (("tapgemm.wreg16", 2),), "tapgemm_pp_bf16_kernel<2>", lambda ncu: sr.COUNT["pingpong"](per=sr.pp_per(24, 128, 128, 64, ncu))),
    ("wreg16", "bf16", (("tapgemm.wreg16", 1),), "tapgemm_wreg16_bf16_kernel<2, true>", lambda ncu: sr.COUNT["wreg16"](per=sr.wreg_per(24, 128, 128, 64, ncu))),
    ("wreg4", "bf16", (("tapgemm.wreg16", 0),), "tapgemm_wreg_kernel<__bf16, 2>", lambda ncu: sr.COUNT["wreg"](per=sr.wreg_per(24, 128, 128, 64, ncu))),
    ("wreg_f32", "f32", (), "tapgemm_wreg_f32_kernel<4, 4, false>", lambda ncu: sr.COUNT["wreg_f32"]()),
]


@pytest.mark.parametrize("name,dt,tune,kernel,count", EXACT, ids=[c[0] for c in EXACT])
def test_exact_planes_up_to_the_chain_count(name, dt, tune, kernel, count):
    c = Fwd(name, "wreg", (dt,), 24, 128, 128, 64, 64, 1, kernel, None, tune=tune)
    planes, big = sr.exact_planes(c.n, c.h, c.w, c.cout)
    w = np.zeros((3, 3, c.cin, c.cout))
    w[1, 1, np.arange(c.cin), np.arange(c.cout)] = 1.0
    x = _t(planes, dt)
    y, stats, scr = c.launch(dt, x, w, np.zeros(c.cout), 1.0)
    assert torch.equal(y, x)                  # the identity: what is stored is the planes, exactly
    assert float(scr.abs().max()) == 0.0
    mu, var = sr.moments64(planes[:1])        # every sample holds the same planes
    cnt = count(_ncu())
    upto = sr.exact_up_to(big)
    inside = upto >= cnt
    band = inside & (upto < 2 * cnt)          # exact at this count, not at twice the count
    emean = np.abs(stats[..., 0] / mu - 1.0)
    einv = np.abs(stats[..., 1] / sr.inv_ref(var) - 1.0)
    print(f"COND exact {name}: count {cnt}: {int(inside.sum())} planes must be exact ({int(band.sum())} of them not at twice the count); worst inv error there "
          f"{einv[:, inside].max():.1e}, on the {int((~inside).sum())} planes past the horizon {einv[:, ~inside].max() if (~inside).any() else 0.0:.1e}")
    if name != "wreg_f32":                    # float64 across patches: no horizon to watch
        assert band.sum() >= 8, (cnt, int(band.sum()))
    # float64 roundoff only: the reference's two passes, the device's hw-term sums and q / hw - mean^2 (which loses a factor ~128 here)
    assert (emean[:, inside] <= 1e-13).all(), (name, float(emean[:, inside].max()))
    assert (einv[:, inside] <= 1e-11).all(), (name, float(einv[:, inside].max()))


# ---- the stand-alone statistics pass on a tensor torch wrote: float64 from the first addition (depth 0)
@pytest.mark.parametrize("dt", BOTH)
def test_offset_ladder_in_stats(dt):
    ops = _ops()
    n, h, c = 2, 32, 64
    rng = np.random.default_rng(303)
    b, rung = sr.ladder_bias(c, 2.4)
    a = rng.standard_normal((n, h, h, c)) * 2.4 + b
    a[..., -1] = b[-1]
    ad = _t(a, dt)
    stats = torch.empty(n * c * 2, dtype=torch.float64, device="cuda")
    ops.in_stats(ad, c, stats, n, h * h, c, EPS_ARG)
    torch.cuda.synchronize()
    _check_ladder(f"in_stats {dt}", ad, host(stats).reshape(n, c, 2), None, sr.CHAIN["in_stats"](), dt, rung)


# ---- gsum: (sum g, sum g * aux) of the gradient an input-gradient launch stores
GSUM = [
    ("dma128x128", "f32", "tapgemm_dma_kernel<", "gsum_dma128x128"), ("dma128x128", "bf16", "tapgemm_dma_kernel<", "gsum_dma128x128"),
    ("halo128_st", "f32", "tapgemm_halo_kernel<", "gsum_halo128_st_f32"), ("halo128_st", "bf16", "tapgemm_halo_kernel<", "gsum_halo128_st_bf16"),
    ("wreg", "f32", "tapgemm_wreg_f32_kernel<", "gsum_wreg_f32"), ("wreg", "bf16", "tapgemm_wreg_kernel<__bf16, 2, true>", "gsum_wreg_bf16"),
]
GS_N, GS_H, GS_C = 2, 16, 64


def _gsum_operands(seed):
    rng = np.random.default_rng(seed)
    shift, _ = sr.ladder_bias(GS_C, 1.0)          # channel c sits at r = RUNGS[c % 6], as in the forward ladder
    dy = rng.standard_normal((GS_N, GS_H, GS_H, GS_C)) + shift
    w = rng.standard_normal((3, 3, GS_C, GS_C)) * 0.1
    aux = rng.standard_normal((GS_N, GS_H, GS_H, GS_C)) + shift
    return dy, w, aux


def _gsum_launch(variant, dt, kernel, dy, w, aux):
    ops = _ops()
    dx = torch.full((GS_N, GS_H, GS_H, GS_C), 7.0, device="cuda", dtype=BF if dt == "bf16" else torch.float32)
    red = torch.zeros(ops.GSUM_SLOTS * GS_N * GS_C * 2, dtype=torch.float64, device="cuda")
    auxd = _t(aux, dt)
    ops.set_tuning("tapgemm.variant", variant)
    ops.conv2d_dgrad(_t(dy, dt), GS_C, _t(w, dt), dx, None, 0, GS_C, 0, GS_N, GS_H, GS_H, GS_C, GS_C, 3, 1, gsum=(auxd, GS_C, red))
    torch.cuda.synchronize()
    k = ops.last_kernel()
    assert k.startswith(kernel) and (variant != "wreg" or k.endswith("true>")), k          # the gsum instantiation of that family ran
    ops.set_tuning("reset", 0)
    return dx, auxd, host(red).reshape(ops.GSUM_SLOTS, GS_N, GS_C, 2).sum(0)


@pytest.mark.parametrize("variant,dt,kernel,chain", GSUM, ids=[f"{g[0]}-{g[1]}" for g in GSUM])
def test_offset_ladder_gsum(variant, dt, kernel, chain):
    dy, w, aux = _gsum_operands(304)
    dx, auxd, got = _gsum_launch(variant, dt, kernel, dy, w, aux)
    L = sr.CHAIN[chain]()
    g = host(dx.float()).reshape(GS_N, -1, GS_C)
    a = host(auxd.float()).reshape(GS_N, -1, GS_C)
    hw = g.shape[1]
    g64 = sr.gamma(hw + 16, sr.U64)
    b1 = (sr.gamma(L) + g64) * np.abs(g).sum(1)
    b2 = (sr.gamma(L + 1) + g64) * np.abs(g * a).sum(1)
    e1, e2 = np.abs(got[..., 0] - g.sum(1)), np.abs(got[..., 1] - (g * a).sum(1))
    rung = np.arange(GS_C) % len(sr.RUNGS)
    cells = [f"{(e1 / b1)[:, rung == k].max():.3f}/{(e2 / b2)[:, rung == k].max():.3f}" for k in range(len(sr.RUNGS))]
    print(f"COND gsum {variant} {dt}: err/bound (sum g / sum g*aux) per rung {sr.RUNGS} of dy and aux: " + "  ".join(cells))
    assert (e1 <= b1).all() and (e2 <= b2).all(), (float((e1 / b1).max()), float((e2 / b2).max()))


# ---------------------------------------------------------------------------------------------------------------------------------------
# non-finite data

def _poison_check(run, x, at, want_of, stat_channels=None):
    """run(x) -> (stored output tensor, per-sample side sums [n, c, k] or None).  One launch clean, one with NaN at `at`, one with +inf.
    want_of(x_poisoned) -> bool [n, ho, wo]: the receptive field of the element.  stat_channels: the channels of the poisoned sample whose
    sums must be non-finite (default: all)."""
    y0, s0 = run(x)
    b0 = _bits(y0)
    assert np.isfinite(y0.float().cpu().numpy()).all() and (s0 is None or np.isfinite(s0).all())
    for val in (np.nan, np.inf):
        xp = np.array(x, copy=True)
        xp[at] = val
        y1, s1 = run(xp)
        got = y1.float().cpu().numpy()
        bad = ~np.isfinite(got)
        want = want_of(xp)
        assert want.any() and not want.all()
        assert np.array_equal(bad, np.broadcast_to(want[..., None], bad.shape)), (val, int(bad.sum()), int(want.sum()) * bad.shape[-1])
        assert np.array_equal(_bits(y1)[~bad], b0[~bad]), val                      # every other output: the same bits
        if s0 is not None:
            p = at[0]
            ch = slice(None) if stat_channels is None else stat_channels
            assert not np.isfinite(s1[p][ch]).any(), (val, s1[p])
            rest = np.ones(s1.shape, bool)
            rest[p][ch] = False
            assert np.isfinite(s1[rest]).all()
            assert (np.abs(s1[rest] - s0[rest]) <= 1e-12 * np.abs(s0[rest])).all(), val


def _box3(shape, at):
    """3 x 3 at unit stride, SAME padding: the 3 x 3 neighbourhood"""
    n, h, w = shape
    want = np.zeros((n, h, w), bool)
    want[at[0], max(at[1] - 1, 0):at[1] + 2, max(at[2] - 1, 0):at[2] + 2] = True
    return want


def _oracle_field(f):
    """the footprint the float64 oracle gives for the same poisoned input; it must cover whole pixels (every channel)"""
    def want_of(xp):
        bad = ~np.isfinite(f(xp))
        assert np.array_equal(bad.any(-1), bad.all(-1))
        return bad.any(-1)
    return want_of


@pytest.mark.parametrize("case,dt", FWD_IDS, ids=[f"{c.name}-{dt}" for c, dt in FWD_IDS])
def test_nonfinite_forward_with_statistics(case, dt):
    rng = np.random.default_rng(310)
    x = rng.standard_normal((case.n, case.h, case.w, case.cin))
    w = rng.standard_normal((3, 3, case.cin, case.cout)) * 0.1
    b = rng.standard_normal(case.cout)
    at = (1, 10, 21, 1) if case.rgb or case.s == 2 else (1, 5, 9, 5)

    def run(xv):
        y, stats, scr = case.launch(dt, xv, w, b, 0.2)
        assert float(scr.abs().max()) == 0.0
        return y, stats

    if case.s == 1:
        want_of = lambda xp: _box3((case.n, case.h, case.w), at)
    else:
        want_of = _oracle_field(lambda xp: conv_ref(_rnd(xp, dt), _rnd(w, dt), case.s))
    _poison_check(run, x, at, want_of)


@pytest.mark.parametrize("dt", BOTH)
def test_nonfinite_transpose_phase4(dt):
    ops = _ops()
    rng = np.random.default_rng(311)
    n, hi, ci, co = 2, 16, 64, 64
    x = rng.standard_normal((n, hi, hi, ci))
    wt = rng.standard_normal((3, 3, co, ci)) * 0.1
    b = rng.standard_normal(co)

    def run(xv):
        y = torch.full((n, 2 * hi, 2 * hi, co), 5.0, device="cuda", dtype=BF if dt == "bf16" else torch.float32)
        ops.set_tuning("tapgemm.variant", "phase4")
        ops.conv2d_transpose_fwd(_t(xv, dt), ci, _t(wt, dt), torch.from_numpy(b.astype(np.float32)).cuda(), y, co, n, hi, hi, ci, co, 0.2)
        torch.cuda.synchronize()
        assert ops.last_kernel() == f"tapgemm_phase4_kernel<{TNAME[dt]}, {TNAME[dt]}>", ops.last_kernel()
        return y, None

    _poison_check(run, x, (1, 5, 9, 5), _oracle_field(lambda xp: nhwc(st.conv2d_transpose_same(nchw(_rnd(xp, dt)), t64(_rnd(wt, dt))))))


@pytest.mark.parametrize("dt", BOTH)
@pytest.mark.parametrize("variant,n,h,cin,cout,kernel", [
    ("dma128x128", 2, 16, 64, 128, "tapgemm_dma_kernel<{t}, {t}, 128, 128, 2, 2, 3, 16>"),
    ("phase4", 2, 32, 64, 128, "tapgemm_phase4_kernel<{t}, {t}>"),
])
def test_nonfinite_dgrad_stride2(variant, n, h, cin, cout, kernel, dt):
    ops = _ops()
    rng = np.random.default_rng(312)
    w = rng.standard_normal((3, 3, cin, cout)) * 0.1
    dy = rng.standard_normal((n, h // 2, h // 2, cout))

    def run(dyv):
        dx = torch.full((n, h, h, cin), 7.0, device="cuda", dtype=BF if dt == "bf16" else torch.float32)
        ops.set_tuning("tapgemm.variant", variant)
        ops.conv2d_dgrad(_t(dyv, dt), cout, _t(w, dt), dx, None, cin, cin, 0, n, h, h, cin, cout, 3, 2)
        torch.cuda.synchronize()
        assert ops.last_kernel() == kernel.format(t=TNAME[dt]), ops.last_kernel()
        return dx, None

    def oracle(dyp):
        xt = torch.zeros(n, cin, h, h, dtype=torch.float64, requires_grad=True)
        ref, = torch.autograd.grad(st.conv2d_same(xt, t64(_rnd(w, dt)), 2), xt, nchw(_rnd(dyp, dt)))
        return nhwc(ref)

    _poison_check(run, dy, (1, 3, 5, 5), _oracle_field(oracle))


@pytest.mark.parametrize("variant,dt,kernel,chain", GSUM, ids=[f"{g[0]}-{g[1]}" for g in GSUM])
def test_nonfinite_dgrad_gsum(variant, dt, kernel, chain):
    dy, w, aux = _gsum_operands(313)
    at = (1, 5, 9, 5)

    def run(dyv):
        dx, _, red = _gsum_launch(variant, dt, kernel, dyv, w, aux)
        return dx, red

    _poison_check(run, dy, at, lambda xp: _box3((GS_N, GS_H, GS_H), at))


@pytest.mark.parametrize("dt", BOTH)
def test_nonfinite_in_stats_and_apply(dt):
    """the stand-alone statistics and apply passes work per channel: the poisoned (sample, channel) plane, and nothing else"""
    ops = _ops()
    n, h, c = 2, 32, 64
    rng = np.random.default_rng(314)
    a = rng.standard_normal((n, h, h, c))
    beta = torch.from_numpy(rng.standard_normal(c).astype(np.float32)).cuda()
    at = (1, 10, 20, 5)

    def run(av):
        ad = _t(av, dt)
        stats = torch.empty(n * c * 2, dtype=torch.float64, device="cuda")
        out = torch.full_like(ad, 3.0)
        ops.in_stats(ad, c, stats, n, h * h, c, EPS_ARG)
        ops.in_apply(ad, c, stats, beta, out, c, n, h * h, c)
        torch.cuda.synchronize()
        return out, host(stats).reshape(n, c, 2)

    y0, s0 = run(a)
    for val in (np.nan, np.inf):
        ap = a.copy()
        ap[at] = val
        y1, s1 = run(ap)
        bad = ~np.isfinite(y1.float().cpu().numpy())
        want = np.zeros_like(bad)
        want[at[0], :, :, at[3]] = True
        assert np.array_equal(bad, want), (val, int(bad.sum()))
        assert np.array_equal(_bits(y1)[~bad], _bits(y0)[~bad])
        rest = np.ones(s1.shape, bool)
        rest[at[0], at[3]] = False
        assert not np.isfinite(s1[at[0], at[3]]).any() and np.isfinite(s1[rest]).all()
        assert (np.abs(s1[rest] - s0[rest]) <= 1e-12 * np.abs(s0[rest])).all()
