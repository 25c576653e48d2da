"""The training step under a delayed and a serialised second stream (tests/sched_ref.py).

One built trainer runs the same step three times: with every task of the second stream joined at once (serialised: the race-free
reference, the identical kernels), as it is, and with every task of the second stream held back by a spin (delayed).  The step is
deterministic up to its float64 atomics, so delayed and as-is must both agree with serialised to the bound of
test_train_loop_gpu.py::test_step_is_reproducible_run_to_run, 1e-6: named losses, gen_Y, both discriminator outputs, the mask and both
flat gradients.  A wait that is missing, a buffer rewritten before the second stream has read it or a scratch shared by the two
streams moves these by orders of magnitude more (each of the step's four waits removed in turn).
Smallest frames the models take: S = 64, F = 32 in bf16, F = 16 in fp32."""
import numpy as np
import pytest
import torch

import rect_step_ref as R
import sched_ref as sr
from oracle import step_torch as st
from util import host

pytestmark = pytest.mark.gpu

S = 64
FLAGS = ("d_fwd_on_lane", "img_loss_on_lane", "d_bwd_on_lane")


def _trainer(dt="bfloat16", F=32, B=2, flags=None, **kw):
    from shmgan_amd import ShmGANwithSSpecSeg
    kw.setdefault("image_size", S)
    m = ShmGANwithSSpecSeg(filter_size=F, batch_size=B, compute_dtype=dt, **kw).build()
    assert m._get_lane().stream is not None                 # there is a second stream for the timings to act on
    if flags is not None:                                   # after build(): a failure then names the sub-graph
        for name, on in zip(FLAGS, flags):
            setattr(m, name, on)
    return m


def _check(out, what):
    """delayed and as-is against serialised, every figure printed before the assertion."""
    bad = []
    for timing in ("as-is", "delayed"):
        ok, fig = sr.same(out[timing], out["serialised"], sr.BOUND)
        worst = sr.report(f"{what}: {timing} against serialised", fig)
        if not ok:
            bad.append((timing, worst))
    assert not bad, bad


def _three_timings(m, F, B, step, what, hw=None):
    if hw is None:
        inp, dr, sf = st.make_inputs(B, S), st.make_draws(step, B, S, F), st.style_factor_intended(S)
        sinp, sdr = st.make_inputs(B, S, rank=1), st.make_draws(step + 1, B, S, F, rank=1)
    else:
        inp, dr, sf = R.make_inputs_hw(B, *hw), R.make_draws_hw(step, B, *hw, F), R.style_factor_hw(*hw)
        sinp, sdr = R.make_inputs_hw(B, *hw, rank=1), R.make_draws_hw(step + 1, B, *hw, F, rank=1)
    out, info = sr.run_timings(m, inp, dr, sinp, sdr, sf)
    assert info["delayed_ms"] < 1000.0, info                # a delayed step stays below about a second
    _check(out, what)
    return out, info


# ---------------------------------------------------------------------------------------------------------------------------
# cases 1-9: one step, apply=False

def test_bf16_default_flags():
    """Case 1: bf16, all three sub-graphs on the second stream."""
    m = _trainer()
    assert (m.d_fwd_on_lane, m.img_loss_on_lane, m.d_bwd_on_lane) == (True, True, True)
    _, info = _three_timings(m, 32, 2, 4, "bf16 default")
    assert info["submissions"][0] == 5                      # the mask, the real trunk, the image losses, spec_loss, D.backward_params


@pytest.mark.parametrize("which", range(3), ids=FLAGS)
def test_bf16_one_subgraph_on_the_second_stream(which):
    """Cases 2-4: exactly one of the three sub-graphs on the second stream."""
    m = _trainer(flags=tuple(i == which for i in range(3)))
    _three_timings(m, 32, 2, 5, f"bf16 only {FLAGS[which]}")


def test_bf16_fp32_gradient_mode():
    """Case 5: bf16 operands, fp32 gradient signal (SHM_BF16_GF32), default flags."""
    m = _trainer(grad_dtype="float32")
    assert m.grad_dtype == torch.float32 and m.compute_dtype == torch.bfloat16
    _three_timings(m, 32, 2, 6, "bf16 gf32")


def test_bf16_live_attention():
    """Case 6: bf16, attention="live", B = 1 (the forced-timing form of
    test_attention_gpu.py::test_live_attention_step_is_the_same_with_the_d_backward_on_either_stream): the mask of the second stream
    feeds both attention branches, and the discriminator's branch runs its backward on the second stream beside the generator's."""
    from test_attention_gpu import _mk_live
    F, B = 32, 1
    m, _, _ = _mk_live(S, F, B, dt="bfloat16")
    assert m._get_lane().stream is not None and m.d_bwd_on_lane
    _three_timings(m, F, B, 4, "bf16 live attention")
    assert np.linalg.norm(host(m.G.P.grads[46 + 12])) > 0 and np.linalg.norm(host(m.D.P.grads[7])) > 0      # both 8F-channel branches are live


def test_fp32_default_flags():
    """Case 7: fp32, weight gradients, the mask and spec_loss only on the second stream."""
    m = _trainer("float32", F=16)
    assert (m.d_fwd_on_lane, m.img_loss_on_lane, m.d_bwd_on_lane) == (False, False, False)
    _three_timings(m, 16, 2, 4, "fp32 default")


def test_fp32_all_subgraphs_forced_onto_the_second_stream():
    """Case 8: never the default, but the variables allow it."""
    m = _trainer("float32", F=16, flags=(True, True, True))
    _three_timings(m, 16, 2, 5, "fp32 all three flags")


def test_bf16_rectangular_frame():
    """Case 9: image_hw = (64, 96)."""
    m = _trainer(image_hw=(64, 96))
    _three_timings(m, 32, 2, 4, "bf16 64 x 96", hw=(64, 96))


# ---------------------------------------------------------------------------------------------------------------------------
# cases 10 and 11: the weights move, so every timing starts from a fresh build; nothing synchronises between the steps

def _snap_losses(m):
    """The raw loss sums of the last step, copied on the main stream (no synchronise): composed into the named losses later."""
    L = m._last
    return (L.dl.clone(), L.il.clone(), L.sl.clone(), L.B, L.npix)


def _named(snap):
    from shmgan_amd.telemetry import compose_losses
    dl, il, sl, B, npix = snap
    return {k: np.asarray(v, np.float64) for k, v in compose_losses(dl.cpu().numpy(), il.cpu().numpy(), sl.cpu().numpy(), B, npix).items()}


def _timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    return e0, e1


def _lookahead_run(timing, coarse_ms, dev, F, B):
    """Three optimizer steps, each with the look-ahead prologue of the next (different) batch."""
    m = _trainer()
    sr.install(m, timing, coarse_ms, sr.FINE_MS)
    snaps, evs = [], []
    for i in range(3):
        evs.append(_timed(lambda i=i: m.train_step(*dev[i], draws=st.make_draws(i, B, S, F), apply=True, next_batch=dev[i + 1])))
        assert m._prefetched is not None
        snaps.append(_snap_losses(m))
    torch.cuda.synchronize()
    res = dict(losses={f"step{i}/{k}": v for i, s in enumerate(snaps) for k, v in _named(s).items()},
               G_flat=host(m.G.P.flat), D_flat=host(m.D.P.flat), G_m=host(m.G.P.m), D_m=host(m.D.P.m))
    return res, max(a.elapsed_time(b) for a, b in evs[1:])         # (the first step allocates)


def _bound_from_spread(ref0, ref1, what):
    """max(1e-6, 4 x the spread of two serialised runs from two fresh builds): a trajectory feeds its own rounding back through Adam and
    the LeakyReLU kinks, so the reference's own repeatability sets the scale."""
    _, fig = sr.same(ref1, ref0, sr.BOUND)
    spread = max(fig.values()) * sr.BOUND
    assert np.isfinite(spread)
    bound = max(sr.BOUND, 4.0 * spread)
    print(f"[sched] {what}: spread of two serialised runs {spread:.3e}, bound {bound:.3e}")
    return bound


def _check_runs(runs, ref, bound, what):
    bad = []
    for timing, res in runs.items():
        ok, fig = sr.same(res, ref, bound)
        worst = sr.report(f"{what}: {timing} against serialised", fig, bound)
        if not ok:
            bad.append((timing, worst))
    assert not bad, bad


def test_three_optimizer_steps_with_lookahead():
    """Case 10: bf16, three consecutive steps with apply=True and next_batch= of a different batch each time: the losses of every step
    and, after the last, both models' weights and first Adam moments."""
    F, B = 32, 2
    dev = [[torch.from_numpy(a).cuda() for a in st.make_inputs(B, S, rank=r)] for r in range(4)]
    ref0, _ = _lookahead_run("serialised", 0.0, dev, F, B)
    ref1, _ = _lookahead_run("serialised", 0.0, dev, F, B)
    bound = _bound_from_spread(ref0, ref1, "three steps with look-ahead")
    asis, step_ms = _lookahead_run("as-is", 0.0, dev, F, B)
    coarse = min(sr.MAX_SPIN_MS, max(sr.COARSE_MS, step_ms))
    delayed, delayed_ms = _lookahead_run("delayed", coarse, dev, F, B)
    print(f"[sched] three steps with look-ahead: undelayed step {step_ms:.2f} ms, coarse lag {coarse:.1f} ms, delayed step {delayed_ms:.1f} ms")
    assert delayed_ms < 1000.0
    _check_runs({"as-is": asis, "delayed": delayed}, ref0, bound, "three steps with look-ahead")


def _ema_run(timing, coarse_ms, dev, x, F, B):
    """train_step(next_batch=), inference on the averaged weights while the look-ahead SpecSeg forward is still queued on the second
    stream, then the step the look-ahead was for."""
    m = _trainer(ema_decay=0.9)
    sr.install(m, timing, coarse_ms, sr.FINE_MS)
    m.train_step(*dev[0], draws=st.make_draws(0, B, S, F), apply=True, next_batch=dev[1])
    raw = m.G.P.flat.clone()
    with m.generator_weights("ema"):
        assert m.G.weights_dirty
        m.infer(x, cyclic=False)
        inf_y, inf_mask = m.gen_Y.clone(), m.specular_candidate.clone()
    back = m.G.P.flat.clone()
    assert m._prefetched is not None                        # the look-ahead is still there for the next step to pick up
    e0, e1 = _timed(lambda: m.train_step(*dev[1], draws=st.make_draws(1, B, S, F), apply=True))
    torch.cuda.synchronize()
    assert torch.equal(raw.view(torch.int32), back.view(torch.int32)), "G.P.flat did not come back bit for bit"
    res = sr.step_outputs(m)
    res.update(inf_gen_Y=host(inf_y), inf_mask=host(inf_mask), G_flat=host(m.G.P.flat), G_ema=host(m.G.P.ema))
    return res, e0.elapsed_time(e1)


def test_inference_on_averaged_weights_between_two_steps():
    """Case 11: bf16, ema_decay > 0."""
    F, B = 32, 2
    dev = [[torch.from_numpy(a).cuda() for a in st.make_inputs(B, S, rank=r)] for r in range(2)]
    x = torch.from_numpy(st.make_inputs(B, S, rank=2)[0]).cuda()
    ref0, _ = _ema_run("serialised", 0.0, dev, x, F, B)
    ref1, _ = _ema_run("serialised", 0.0, dev, x, F, B)
    bound = _bound_from_spread(ref0, ref1, "inference between two steps")
    asis, step_ms = _ema_run("as-is", 0.0, dev, x, F, B)
    coarse = min(sr.MAX_SPIN_MS, max(sr.COARSE_MS, step_ms))
    delayed, delayed_ms = _ema_run("delayed", coarse, dev, x, F, B)
    print(f"[sched] inference between two steps: undelayed step {step_ms:.2f} ms, coarse lag {coarse:.1f} ms, delayed step {delayed_ms:.1f} ms")
    assert delayed_ms < 1000.0
    _check_runs({"as-is": asis, "delayed": delayed}, ref0, bound, "inference between two steps")


# ---------------------------------------------------------------------------------------------------------------------------
# the environment switches

@pytest.mark.parametrize("dt", ["float32", "bfloat16"])
def test_environment_switches_place_the_subgraphs(dt, monkeypatch):
    from shmgan_amd import ShmGANwithSSpecSeg
    names = ("SHM_D_FWD_LANE", "SHM_IMG_LOSS_LANE", "SHM_D_BWD_LANE")
    for name in names + ("SHM_NO_WGRAD_LANE",):
        monkeypatch.delenv(name, raising=False)
    kw = dict(image_size=S, filter_size=32, batch_size=1, compute_dtype=dt)
    m = ShmGANwithSSpecSeg(**kw)
    assert [getattr(m, f) for f in FLAGS] == [dt == "bfloat16"] * 3
    assert m._get_lane().stream is not None
    for i, name in enumerate(names):
        for value in ("0", "1"):
            monkeypatch.setenv(name, value)
            m = ShmGANwithSSpecSeg(**kw)
            want = [dt == "bfloat16"] * 3
            want[i] = value == "1"
            assert [getattr(m, f) for f in FLAGS] == want, (name, value)
        monkeypatch.delenv(name)
    monkeypatch.setenv("SHM_NO_WGRAD_LANE", "1")
    assert ShmGANwithSSpecSeg(**kw)._get_lane().stream is None


def test_fp32_step_without_the_second_stream_is_the_serialised_step(monkeypatch):
    """fp32 with default flags has no sub-graph on the second stream, so SHM_NO_WGRAD_LANE=1 runs the same program as the serialised
    timing: same dispatch, every task in program order."""
    from shmgan_amd import ShmGANwithSSpecSeg
    F, B = 16, 2
    inp, dr, sf = st.make_inputs(B, S), st.make_draws(4, B, S, F), st.style_factor_intended(S)
    monkeypatch.delenv("SHM_NO_WGRAD_LANE", raising=False)
    m = _trainer("float32", F=F, B=B)
    sr.install(m, "serialised")
    ref = sr.run_step(m, inp, dr, sf)
    monkeypatch.setenv("SHM_NO_WGRAD_LANE", "1")
    one = ShmGANwithSSpecSeg(image_size=S, filter_size=F, batch_size=B).build()
    assert one._get_lane().stream is None and one.G.lane.stream is None and one.D.lane.stream is None
    got = sr.run_step(one, inp, dr, sf)
    ok, fig = sr.same(got, ref, sr.BOUND)
    sr.report("fp32 without the second stream against serialised", fig)
    assert ok


# ---------------------------------------------------------------------------------------------------------------------------
# the proof that the delay is long enough on the machine the suite runs on

def test_delayed_lane_exposes_a_missing_join():
    """torch ops only, on a real WgradLane behind the delayed proxy with the least coarse lag: the second stream fills a buffer, the
    main stream copies it once without join() and once after.  The unjoined copy holds the old contents, the joined copy the new."""
    from shmgan_amd.model import WgradLane
    dev = torch.device("cuda", torch.cuda.current_device())
    real = WgradLane(dev)
    assert real.stream is not None
    sr.ensure_overlap(real)
    lane = sr.LaneProxy(real, "delayed", sr.COARSE_MS)
    buf = torch.zeros(1 << 16, device=dev)
    (buf + 0).fill_(2.0)                                    # both kernels loaded before the timing matters
    torch.cuda.synchronize()
    lane.submit(lambda: buf.fill_(1.0))
    early = buf + 0                                         # the missing join
    lane.join()
    late = buf + 0
    torch.cuda.synchronize()
    print(f"[sched] toy: lag {sr.COARSE_MS} ms, unjoined copy sums to {float(early.sum())}, joined copy to {float(late.sum())} of {buf.numel()}")
    assert float(early.abs().max()) == 0.0, "the delayed second stream was not behind the main stream: the lag is too short here"
    assert bool((late == 1.0).all())
