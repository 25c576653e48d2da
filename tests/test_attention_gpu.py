"""The "as-intended" live attention branch (attention_layer SHM.py:404-412, used at SHM.py:248-275, 290-293,
358-359): the step's SpecSeg mask -> MaxPool -> 2 x (Conv3x3 + LeakyReLU) -> added to the four generator skips and to the
discriminator's fourth block, with gradients into its 10 convolutions.  Default (attention="executed") stays the graph the
reference runs (+ 0); the oracle restates both (oracle.step_torch.train_step(attention=...))."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import specseg_torch as sp
from oracle import step_torch as st
from util import cosine, host, rel_l2, t64

pytestmark = pytest.mark.gpu
BF = torch.bfloat16


def _ops():
    from shmgan_amd import ops
    return ops


@pytest.mark.parametrize("dt", [torch.float32, BF])
def test_mask_pool_add_bcast_sum_groups(dt):
    ops = _ops()
    rng = np.random.default_rng(1)
    B, S = 3, 32
    mask = rng.random((B, S, S, 1)).astype(np.float32)
    pad = 16 if dt == torch.float32 else 32
    for k in (1, 2, 4, 16):
        dst = torch.full((B, S // k, S // k, pad), 5.0, device="cuda", dtype=dt)
        ops.mask_pool_pack(torch.from_numpy(mask).cuda(), dst, B, S, k)
        ref = F.max_pool2d(torch.from_numpy(mask).permute(0, 3, 1, 2), k).permute(0, 2, 3, 1) if k > 1 else torch.from_numpy(mask)
        got = dst.float().cpu()
        assert torch.equal(got[..., :1], ref.to(dt).float()) and float(got[..., 1:].abs().max()) == 0.0
    # broadcast add over the copies of a sample, with a row offset, and its gradient
    nimg, per, i0 = 7, 4 * 4 * 8, 2
    a = rng.standard_normal((nimg, per)).astype(np.float32)
    b = rng.standard_normal((B, per)).astype(np.float32)
    ad, bd = torch.from_numpy(a).cuda().to(dt), torch.from_numpy(b).cuda().to(dt)
    out = torch.empty_like(ad)
    ops.add_bcast(ad, bd, out, nimg, per, B, i0)
    idx = [(i0 + i) % B for i in range(nimg)]
    ref = ad.float().cpu().numpy() + bd.float().cpu().numpy()[idx]
    assert rel_l2(host(out.float()), ref) < (1e-6 if dt == torch.float32 else 4e-3)
    g = torch.full((B, per), 3.0, device="cuda", dtype=dt)
    ops.sum_groups(ad, g, nimg, per, B, i0, accumulate=False)
    refg = np.zeros((B, per))
    for i, j in enumerate(idx):
        refg[j] += ad.float().cpu().numpy()[i]
    assert rel_l2(host(g.float()), refg) < (1e-6 if dt == torch.float32 else 4e-3)
    ops.sum_groups(ad, g, nimg, per, B, i0, accumulate=True)
    assert rel_l2(host(g.float()), 2 * refg) < (1e-6 if dt == torch.float32 else 8e-3)


def _keras_g(g, ga):
    out = []
    for lvl in range(4):
        out += g[4 * lvl:4 * lvl + 4] + ga[4 * lvl:4 * lvl + 4]
    return out + g[16:]


def _mk_live(S, F, B, bias_std=0.05, dt="float32"):
    from shmgan_amd import ShmGANwithSSpecSeg
    m = ShmGANwithSSpecSeg(image_size=S, filter_size=F, batch_size=B, attention="live", compute_dtype=dt).build()
    g, d, gb, db = st.init_params(F, S)
    att0 = st.init_attention(F)                       # the product's own init equals the oracle's (zero biases)
    for a, b in zip(m.G.get_weights(), _keras_g(g, att0["G"])):
        assert np.array_equal(a, b)
    for a, b in zip(m.D.get_weights(), d[:4] + att0["D"] + d[4:]):
        assert np.array_equal(a, b)
    att = st.init_attention(F, bias_std=bias_std)     # non-trivial biases for the parity run
    m.G.set_weights(_keras_g(g, att["G"]))
    m.D.set_weights(d[:4] + att["D"] + d[4:])
    return m, (g, d, gb, db), att


def test_variable_order_and_counts_follow_keras():
    """attention_layer's convolutions are created right after the two convolutions of their encoder level (conv2d_2/3, 6/7,
    10/11, 14/15) and between the discriminator's fourth and fifth block (conv2d_31/32): the layers the committed summaries
    show as ABSENT from the executed models (Generator_summary.txt / Discriminator_summary.txt)."""
    m, _, _ = _mk_live(64, 16, 1)
    shp = [tuple(v.shape) for v in m.G.trainable_variables]
    assert shp[:8] == [(3, 3, 10, 16), (16,), (3, 3, 16, 16), (16,), (3, 3, 1, 16), (16,), (3, 3, 16, 16), (16,)]
    assert shp[8:16] == [(3, 3, 16, 32), (32,), (3, 3, 32, 32), (32,), (3, 3, 1, 32), (32,), (3, 3, 32, 32), (32,)]
    assert len(shp) == 46 + 16
    extra = sum(9 * c + c + 9 * c * c + c for c in (16, 32, 64, 128))
    from shmgan_amd import ShmGANwithSSpecSeg
    base = ShmGANwithSSpecSeg(image_size=64, filter_size=16).build()
    assert m.G.count_params() == base.G.count_params() + extra
    dshp = [tuple(v.shape) for v in m.D.trainable_variables]
    assert dshp[4:8] == [(3, 3, 1, 128), (128,), (3, 3, 128, 128), (128,)] and len(dshp) == 11


@pytest.mark.parametrize("B,step", [(1, 0), (2, 1)])
def test_live_attention_step_matches_oracle(B, step):
    S, F = 64, 16
    m, (g, d, gb, db), att = _mk_live(S, F, B)
    inp = st.make_inputs(B, S)
    dr = st.make_draws(step, B, S, F)
    sf = st.style_factor_intended(S)
    sw = sp.init_specseg(seed=44 + step)
    m.SpecSeg.set_weights(sw)
    m.train_step(*inp, draws=dr, style_factor=sf, apply=False)
    torch.cuda.synchronize()
    masks = {"g1": m.G.lrelu_masks("g1"), "cyc": m.G.lrelu_masks("cyc"), "d": m.D.lrelu_masks(),
             "ga": m.G.attention_masks(), "da": m.D.attention_masks()}
    ref = st.train_step(g, d, gb, db, inp, dr, sf, F, masks=masks, specseg=sw, attention=att)
    plain = st.train_step(g, d, gb, db, inp, dr, sf, F, need_grads=False, specseg=sw)
    got = m.losses()
    for k, v in ref["losses"].items():
        assert abs(got[k] - v) <= 1e-4 * max(1.0, abs(v)), (k, got[k], v)
    assert abs(ref["losses"]["total_Generator_loss"] - plain["losses"]["total_Generator_loss"]) > 1e-5      # the branch is live
    assert np.abs(host(m.gen_Y) - ref["outs"]["gen_Y"].numpy()).max() < 1e-4
    ng, nd = 46, 7
    sets = (("G", m.G.P.grads[:ng], ref["gG"]), ("Ga", m.G.P.grads[ng:], ref["gGa"]),
            ("D", m.D.P.grads[:nd], ref["gD"]), ("Da", m.D.P.grads[nd:], ref["gDa"]))
    for name, got_l, ref_l in sets:
        assert len(got_l) == len(ref_l)
        for i, (gg, r) in enumerate(zip(got_l, ref_l)):
            r = r.numpy()
            if np.linalg.norm(r) < 1e-12:
                continue
            e = rel_l2(host(gg), r)
            assert e < 1e-3 and cosine(host(gg), r) > 0.9999, (name, i, e)
    # and the optimizer moves the attention variables
    w0 = host(m.G.P.vars[ng]).copy()
    m.optimizer_G.apply(m.G.P)
    torch.cuda.synchronize()
    assert np.abs(host(m.G.P.vars[ng]) - w0).max() > 0


def test_zero_attention_weights_reproduce_the_executed_graph():
    """With every attention kernel and bias at zero the live graph adds zeros: the executed graph (to the run-to-run bound of the
    step, test_step_is_reproducible_run_to_run: the float64 atomics of two runs may differ in the last bit)."""
    from shmgan_amd import ShmGANwithSSpecSeg
    S, F, B = 64, 16, 2
    m, (g, d, gb, db), att = _mk_live(S, F, B)
    z = {k: [np.zeros_like(a) for a in v] for k, v in att.items()}
    m.G.set_weights(_keras_g(g, z["G"]))
    m.D.set_weights(d[:4] + z["D"] + d[4:])
    e = ShmGANwithSSpecSeg(image_size=S, filter_size=F, batch_size=B).build()
    inp, dr = st.make_inputs(B, S), st.make_draws(2, B, S, F)
    sw = sp.init_specseg(seed=5)
    for mdl in (m, e):
        mdl.SpecSeg.set_weights(sw)
        mdl.train_step(*inp, draws=dr, apply=False)
    torch.cuda.synchronize()
    le, lm = e.losses(), m.losses()
    for k, v in le.items():
        if k != "ssim":
            assert abs(lm[k] - v) <= 1e-9 * max(1.0, abs(v)), (k, lm[k], v)
    assert rel_l2(host(m.G.P.grads[0]), host(e.G.P.grads[0])) <= 1e-6
    assert rel_l2(host(m.D.P.grads[4]), host(e.D.P.grads[4])) <= 1e-6


def test_live_attention_bf16_runs_and_tracks_fp32():
    S, F, B = 64, 32, 1
    inp, dr = st.make_inputs(B, S), st.make_draws(3, B, S, F)
    res = {}
    for dt in ("float32", "bfloat16"):
        m, _, _ = _mk_live(S, F, B, dt=dt)
        m.train_step(*inp, draws=dr, apply=False)
        torch.cuda.synchronize()
        res[dt] = (m.losses(), m.G.P.grad.clone(), m.D.P.grad.clone())
    for k, v in res["float32"][0].items():
        if k != "ssim":
            assert abs(res["bfloat16"][0][k] - v) <= 2e-2 * max(1.0, abs(v)), (k, v, res["bfloat16"][0][k])
    # un-pinned LeakyReLU kinks: bf16 rounding moves ~1 % of the pre-activations across zero (DESIGN.md, bf16 path), so the
    # whole-model cosine against fp32 sits at 0.97-0.99 at this size; the pinned comparison is test_bf16_gpu.py's
    assert cosine(host(res["bfloat16"][1]), host(res["float32"][1])) > 0.95
    assert cosine(host(res["bfloat16"][2]), host(res["float32"][2])) > 0.95


def test_live_attention_step_is_the_same_with_the_d_backward_on_either_stream():
    """bf16 with attention="live" at the smallest frame the discriminator takes and the smallest filter count bf16 takes (S = 64,
    F = 32, B = 1): the discriminator's attention branch and the generator's level-3 branch both have 8F = 256 channels.  With
    d_bwd_on_lane the discriminator's branch runs its backward on the second stream while the generator's branches run theirs on
    the main one; each branch has a LeakyReLU-backward scratch of its own, so one step gives the same flat gradients and named
    losses whichever stream the D-loss backward is on, to the bound of two runs of one step
    (test_train_loop_gpu.py::test_full_size_step_is_reproducible_over_many_runs: 1e-6, the float64 atomics).
    This run leaves the timing of the two streams to chance; test_sched_gpu.py::test_bf16_live_attention (case 6) is its forced-timing
    form: the same step with the second stream serialised and delayed."""
    S, F, B = 64, 32, 1
    m, _, _ = _mk_live(S, F, B, dt="bfloat16")
    assert m._get_lane().stream is not None                 # there is a second stream for the schedule to use
    inp, dr = st.make_inputs(B, S), st.make_draws(4, B, S, F)
    res = []
    for on_lane in (True, False):
        m.d_bwd_on_lane = on_lane
        m.train_step(*inp, draws=dr, apply=False)
        torch.cuda.synchronize()
        res.append((dict(m.losses()), host(m.G.P.grad).copy(), host(m.D.P.grad).copy()))
    (l1, g1, d1), (l0, g0, d0) = res
    assert np.linalg.norm(host(m.G.P.grads[46 + 12])) > 0 and np.linalg.norm(host(m.D.P.grads[7])) > 0      # both 256-channel branches are live
    eg, ed = rel_l2(g1, g0), rel_l2(d1, d0)
    print(f"second stream against main stream: G gradient rel-L2 {eg:.3e}, D gradient rel-L2 {ed:.3e}")
    for k, v in l0.items():
        a, b = np.asarray(l1[k], np.float64), np.asarray(v, np.float64)
        assert np.all(np.abs(a - b) <= 1e-6 * np.maximum(1.0, np.abs(b))), (k, v, l1[k])
    assert eg <= 1e-6 and ed <= 1e-6, (eg, ed)
