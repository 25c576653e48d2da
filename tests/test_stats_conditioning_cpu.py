"""The model behind test_stats_conditioning_gpu.py, on the CPU: the one-pass design itself (chains of L sequential fp32 additions, float64
across chains, var = q / hw - mean^2; stats_ref.emulate_onepass -- NOT the kernels) stays inside stats_ref.onepass_bound on the offset
ladder of the GPU test, at every rung and every chain depth of stats_ref.CHAIN.  So the GPU test's inputs never push a correct
implementation over the bound.  It also prints the typical (RMS) error next to the bound (DESIGN.md 4 starts from these numbers) and
recomputes R_WORK from the float64 oracle."""
import numpy as np
import pytest
import torch

import stats_ref as sr
from oracle import step_torch as st

NCU = 256          # MI355X
# every depth the GPU test meets: the fixed ones, and the persistent kernels at one patch per block and at n = 24, 128 x 128 (3072 / 1536 patches)
DEPTHS = sorted({f() for k, f in sr.CHAIN.items() if k not in ("wreg", "wreg16", "pingpong", "rgb")}
                | {sr.CHAIN["wreg"](per=p) for p in (1, sr.wreg_per(24, 128, 128, 64, NCU))}
                | {sr.CHAIN["wreg16"](per=p) for p in (1, sr.wreg_per(24, 128, 128, 64, NCU))}
                | {sr.CHAIN["pingpong"](per=p) for p in (1, sr.pp_per(24, 128, 128, 64, NCU))}
                | {sr.CHAIN["rgb"](gpw=g) for g in (2, 4, 32)})


def _ladder_output(slope, bf16, hw=4096, reps=4, seed=0):
    """what a ladder launch stores: LeakyReLU(N(0, sigma_out^2) + bias), rounded to the output type; one all-constant channel"""
    rng = np.random.default_rng(seed)
    sigma_out = 0.1 * np.sqrt(9 * 64)
    cout = 2 * len(sr.RUNGS) * reps
    b, rung = sr.ladder_bias(cout, sigma_out)
    z = (rng.standard_normal((hw, cout)) * sigma_out).astype(np.float32) + b
    z[:, -1] = b[-1]
    y = np.where(z > 0, z, np.float32(slope) * z).astype(np.float32)
    if bf16:
        y = torch.from_numpy(y).to(torch.bfloat16).float().numpy()
    return y, rung


def test_depths_cover_the_table():
    assert DEPTHS[0] == 0 and 33 in DEPTHS and 768 in DEPTHS and 259 in DEPTHS and 39 in DEPTHS, DEPTHS
    assert sr.wreg_per(24, 128, 128, 64, NCU) == 6 and sr.pp_per(24, 128, 128, 64, NCU) == 3
    assert sr.pp_per(3, 16, 32, 64, NCU) == 1 and sr.wreg_per(3, 16, 16, 64, NCU) == 1
    assert sr.rgb_groups_per_wave(3, 16, 16, "f32") == 2 and sr.rgb_groups_per_wave(96, 128, 128, "bf16") == 16


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("slope", [1.0, 0.2])
def test_emulated_design_stays_inside_the_bound(slope, bf16, capsys):
    y, rung = _ladder_output(slope, bf16)
    hw = y.shape[0]
    mu, var = sr.moments64(y[None])
    mu, var = mu[0], var[0]
    sigma = np.sqrt(var)
    lines = [f"slope {slope} {'bf16' if bf16 else 'f32'}: RMS relative error of inv (emulated) | bound (median), per rung r = {sr.RUNGS}"]
    for L in DEPTHS:
        mean, _, inv = sr.emulate_onepass(y, L)
        dmean, _, dinv = sr.onepass_bound(mu, sigma, L, n64=hw)
        em = np.abs(mean - mu)
        ei = np.abs(inv / sr.inv_ref(var) - 1.0)
        assert (em <= dmean).all(), (L, float((em / np.maximum(dmean, 1e-300)).max()))
        assert (ei <= dinv).all(), (L, float((ei / np.maximum(dinv, 1e-300)).max()))
        # the constant channel: clamped variance, mean to gamma_L
        assert 0.0 < inv[-1] <= (1.0 + 1e-12) / np.sqrt(sr.EPS)
        assert abs(mean[-1] - y[0, -1]) <= (sr.gamma(L) + sr.gamma(hw + 2, sr.U64)) * abs(y[0, -1])
        row = []
        for k in range(len(sr.RUNGS)):
            m = rung == k
            m[-1] = False
            row.append(f"{np.sqrt((ei[m] ** 2).mean()):.1e}|{np.median(dinv[m]):.1e}")
        lines.append(f"  L={L:4d}: " + "  ".join(row))
    with capsys.disabled():
        print("\n" + "\n".join(lines))


def test_bound_has_teeth():
    """what the bound is for: a float finalize, or float sums across chains, leave it at the top rungs for the short chains"""
    y, rung = _ladder_output(1.0, False)
    hw = y.shape[0]
    mu, var = sr.moments64(y[None])
    mu, var = mu[0], var[0]
    s = y.sum(0, dtype=np.float64)
    q = (y.astype(np.float64) ** 2).sum(0)
    mean32 = (s / hw).astype(np.float32)
    var32 = (q / hw).astype(np.float32) - mean32 * mean32          # the finalize in float
    inv32 = 1.0 / np.sqrt(np.maximum(var32, 0).astype(np.float64) + sr.EPS)
    _, _, dinv = sr.onepass_bound(mu, np.sqrt(var), 0, n64=hw)
    top = rung == len(sr.RUNGS) - 1
    top[-1] = False
    assert (np.abs(inv32 / sr.inv_ref(var) - 1.0)[top] > dinv[top]).all()


def test_exact_planes_see_a_chain_that_grows():
    """stats_ref.exact_planes, what the GPU test relies on, in the sequential model: fp32 chains of COUNT stored values are exact for every
    plane inside the horizon, at each persistent kernel's count.  Twice the count is asserted for wreg16 only, the one kernel whose
    accumulator takes the stored values of all its patches in sequence, as the model does: there a kernel that flushes half as often
    moves inv of planes in the band by far more than the GPU test's 1e-11 -- which the worst-case bound, 100 to 1000 times above the typical
    error of these kernels, never would.  The four-wave wreg and ping-pong kernels reduce each patch first (32 and 256 values) and add one
    number per patch, so on these planes their sums stay multiples of 32 V^2 and exact far past COUNT: the sequential model at twice
    the count is not their order of additions, and its figures for those counts are printed only."""
    y, big = sr.exact_planes(1, 128, 128)
    assert (torch.from_numpy(y).to(torch.bfloat16).float().numpy() == y).all()           # bf16 numbers
    # the order a persistent block walks: patch after patch (8 x 16 pixels), so that a chain of k values holds whole patches
    seq = y[0].reshape(16, 8, 8, 16, 64).transpose(0, 2, 1, 3, 4).reshape(-1, 64)
    hw = seq.shape[0]
    mu, var = sr.moments64(y)
    upto = sr.exact_up_to(big)
    for name, count in (("wreg", sr.COUNT["wreg"](per=6)), ("wreg16", sr.COUNT["wreg16"](per=6)), ("pingpong", sr.COUNT["pingpong"](per=3))):
        inside = upto >= count
        band = inside & (upto < 2 * count)
        assert band.sum() >= 8, (count, int(band.sum()))
        inv = {}
        for k in (count, 2 * count):
            s = q = 0.0
            for i in range(0, hw, k):
                v = seq[i:i + k]
                s = s + np.cumsum(v, 0, dtype=np.float32)[-1].astype(np.float64)
                q = q + np.cumsum(v * v, 0, dtype=np.float32)[-1].astype(np.float64)          # v * v is exact in fp32 here
            inv[k] = 1.0 / np.sqrt(np.maximum(q / hw - (s / hw) ** 2, 0.0) + sr.EPS)
        e1, e2 = np.abs(inv[count] / sr.inv_ref(var[0]) - 1.0), np.abs(inv[2 * count] / sr.inv_ref(var[0]) - 1.0)
        print(f"{name}, count {count}: {int(inside.sum())} planes exact (worst {e1[inside].max():.1e}); at twice the count {int((e2[band] > 1e-9).sum())} of the {int(band.sum())} "
              f"planes of the band are off, by up to {e2[band].max():.1e}")
        assert (e1[inside] <= 1e-11).all(), (count, float(e1[inside].max()))
        if name == "wreg16":
            assert (e2[band] > 1e-9).sum() >= 4, (count, e2[band])


def test_r_work_is_what_the_oracle_step_shows():
    """the largest |mean| / std over every InstanceNorm block's pre-normalisation activation of the float64 step (S = 64, F = 16, B = 2)"""
    S, F, B = 64, 16, 2
    g, d, gb, db = st.init_params(F, S)
    log = []
    st.train_step(g, d, gb, db, st.make_inputs(B, S), st.make_draws(0, B, S, F), st.style_factor_intended(S), F, need_grads=False, in_log=log)
    assert len(log) == 168                    # 18 generator blocks x 6 generator calls + 5 discriminator blocks x 12 calls
    r = max(float((x.mean(dim=(2, 3)).abs() / x.var(dim=(2, 3), unbiased=False).sqrt()).max()) for x in log)
    print("r_work", r)
    assert abs(r - sr.R_WORK) < 1e-3, r
