"""Forced timings of the training step's second stream (tests/test_sched_gpu.py).

train_step spreads its work over two HIP streams through model.WgradLane: every weight gradient, the SpecSeg mask of the prologue (and
the look-ahead prologue of the next batch), spec_loss and -- in bf16 -- the real half of the discriminator trunk, the image losses and
the D-loss backward.  Whether the main stream waits where it must cannot be seen by running the step as it is: at test sizes the step
is launch-bound and the second stream is practically always ahead of its consumers.  So the same Python program (same launches, same
dispatch, same arena keys) is run under forced timings, with a proxy in the place of the trainer's WgradLane:

  serialised  submit(fn) = the real submit, then join(): every task runs on the second stream, in program order, with nothing beside
              it.  The race-free reference.
  delayed     submit(fn) = the real submit of (spin, then fn): the task starts on the second stream only once the main stream has
              reached the point of submission (the real submit's event) AND the spin has run out, so it completes long after the main
              stream has issued its later work.  An unguarded consumer then reads what the buffer held before, and a buffer rewritten too
              early is read after the rewrite.  (A timing orders the streams; it cannot make two kernels run at the same moment, so
              a zero-on-return scratch shared by the two streams is not what it finds: DESIGN.md section 6n.)
  as-is       no proxy.

The spin is torch.cuda._sleep (one wave: it delays the second stream without taking compute units from the main one), calibrated from
cycles to milliseconds once per process with two events.  The trainer's own submissions (the prologue mask, the real trunk, the image
losses, spec_loss, D.backward_params: five per step with all three sub-graphs on the second stream) get the coarse lag, the per-layer
weight gradients the models submit get the fine one; the spins queue behind each other on the second stream, so the lag of a task is
the sum of the spins in front of it.

Numbers (MI355X, S = 64, B = 2, measured with events; DESIGN.md section 6n has the table):
  torch.cuda._sleep                      2.39e6 cycles per millisecond
  undelayed step                         5.4-6.7 ms in bf16 (F = 32), 4.9-6.7 ms in fp32 (F = 16), 6.8-7.7 ms with live attention (B = 1)
  submissions per step, trainer          5 in bf16 (the mask, the real trunk, the image losses, spec_loss, D.backward_params), 3 with one
                                         sub-graph on the second stream, 2 in fp32 (the mask, spec_loss); + 1 with next_batch=
  submissions per step, models           49 weight gradients (59 with live attention)
  coarse lag                             max(COARSE_MS = 12 ms, the undelayed step measured on the spot), at most MAX_SPIN_MS = 50 ms
  fine lag                               FINE_MS = 1 ms
  delayed step                           5 x 12 + 49 x 1 + the step: 111-122 ms measured (76-79 ms in fp32)
These values are long enough by the knock-outs of DESIGN.md section 6n (each of the step's four waits removed in turn turns a case red
under the delayed timing, by 6e4 to 1e6 times the bound) and, on whatever machine the suite runs on, by
test_delayed_lane_exposes_a_missing_join.

The runtime maps its streams onto a few hardware queues (four here).  A second stream that shares the main stream's queue runs in issue
order with it, and a spin on it holds the main stream back as well: such a stream cannot be delayed at all (of ten
fresh streams the seventh did: the first three got queues of their own, then the four queues are handed out in turn).  ensure_overlap finds
that out with a toy (overlaps_main) and gives the WgradLane another stream until one runs beside the main stream.

Stale data must differ from fresh data to be seen: a step repeated on one trainer finds the previous run's (correct) values in
every buffer.  run_timings therefore runs a scrub step -- another batch, other draws, serialised -- in front of every compared step.
"""
import numpy as np
import torch

from util import host, rel_l2

BOUND = 1e-6               # two runs of one step: the float64 atomics (test_train_loop_gpu.py::test_step_is_reproducible_run_to_run)
MAX_SPIN_MS = 50.0         # one spin is never longer
COARSE_MS = 12.0           # least lag in front of a submission of the trainer's: of the order of one undelayed step
FINE_MS = 1.0              # lag in front of a per-layer weight gradient

_cycles_per_ms = None


def cycles_per_ms():
    """torch.cuda._sleep cycles that last one millisecond on this device: two events around one long spin, once per process."""
    global _cycles_per_ms
    if _cycles_per_ms is None:
        probe = 20_000_000
        torch.cuda._sleep(1000)                        # loads the kernel
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        torch.cuda._sleep(probe)
        e1.record()
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1)
        assert ms > 0.05, f"torch.cuda._sleep({probe}) took {ms} ms: it does not spin on this device"
        _cycles_per_ms = probe / ms
    return _cycles_per_ms


def spin(ms):
    """Keep the current stream busy for `ms` milliseconds (at most MAX_SPIN_MS) with one wave."""
    torch.cuda._sleep(int(min(float(ms), MAX_SPIN_MS) * cycles_per_ms()))


class LaneProxy:
    """Stands in for a model.WgradLane: the same stream, event() and join(), a wrapped submit()."""

    def __init__(self, lane, timing, lag_ms=0.0):
        assert timing in ("serialised", "delayed")
        assert not isinstance(lane, LaneProxy)
        self.lane, self.timing, self.lag_ms = lane, timing, float(lag_ms)
        self.submissions = 0

    @property
    def stream(self):
        return self.lane.stream

    def event(self):
        return self.lane.event()

    def join(self):
        self.lane.join()

    def submit(self, fn):
        self.submissions += 1
        if self.lane.stream is None:                   # no second stream: there is nothing to time
            self.lane.submit(fn)
        elif self.timing == "serialised":
            self.lane.submit(fn)
            self.lane.join()
        else:
            def late():
                spin(self.lag_ms)                      # on the second stream (current here), behind its wait for the main one
                fn()
            self.lane.submit(late)


def overlaps_main(stream, ms=3.0):
    """Whether work queued on `stream` runs beside the main stream's: a spin and a fill on `stream`, a kernel on the main stream that
    reads the buffer.  The runtime maps its streams onto a few hardware queues; two streams that share one run in issue order, and a
    spin on one of them holds the other back as well -- no timing can then be forced."""
    buf = torch.zeros(1024, device="cuda")
    (buf + 0).fill_(2.0)                               # both kernels loaded
    cycles_per_ms()
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        spin(ms)
        buf.fill_(1.0)
    early = buf + 0                                    # a kernel, as the step's consumers are
    torch.cuda.synchronize()
    return float(early.max()) == 0.0


def ensure_overlap(lane, tries=8):
    """Give the WgradLane a stream that runs beside the main one (see overlaps_main), once per lane; nothing may be queued on it."""
    if lane.stream is None or getattr(lane, "_overlap_checked", False):
        return
    for _ in range(tries):
        if overlaps_main(lane.stream):
            lane._overlap_checked = True
            return
        lane.stream = torch.cuda.Stream(device=lane.stream.device)
    raise AssertionError(f"none of {tries} streams ran beside the main stream: the second stream cannot be delayed on this machine")


def real_lane(m):
    lane = m._get_lane()
    lane = lane.lane if isinstance(lane, LaneProxy) else lane
    ensure_overlap(lane)
    return lane


def install(m, timing, coarse_ms=COARSE_MS, fine_ms=FINE_MS):
    """Put the trainer `m` (built) under a timing: "as-is" restores the real lane everywhere; "serialised" / "delayed" put one proxy on
    the trainer and one on the models (G and D submit the per-layer weight gradients: the fine lag).  Returns (trainer proxy, model
    proxy), or (None, None)."""
    lane = real_lane(m)
    if timing == "as-is":
        m._lane = m.G.lane = m.D.lane = lane
        return None, None
    pt, pm = LaneProxy(lane, timing, coarse_ms), LaneProxy(lane, timing, fine_ms)
    m._lane, m.G.lane, m.D.lane = pt, pm, pm
    return pt, pm


def run_step(m, inp, draws, style_factor=None, apply=False, next_batch=None):
    """One train_step; after a device synchronise the named losses, gen_Y, the discriminator outputs, the mask and both flat gradients
    as host copies."""
    m.train_step(*inp, draws=draws, style_factor=style_factor, apply=apply, next_batch=next_batch)
    torch.cuda.synchronize()
    return step_outputs(m)


def step_outputs(m):
    return dict(losses={k: np.asarray(v, np.float64).copy() for k, v in m.losses().items()},
                gen_Y=host(m.gen_Y), rf=host(m.D.ctx["rf"]), cls=host(m.D.ctx["cls"]), mask=host(m.specular_candidate),
                gG=host(m.G.P.grad), gD=host(m.D.P.grad))


def same(a, b, bound=BOUND):
    """The project's comparison of two step results (run_step's dicts, or any dict of arrays with an optional "losses" dict):
    every named loss of `a` within bound * max(1, |v|) of b's v, every tensor within rel-L2 <= bound.  Returns (ok, figures):
    figures[name] = the error as a multiple of what the bound allows (<= 1 passes; non-finite fails)."""
    fig = {}
    for k, v in b.items():
        if k == "losses":
            for name, lv in v.items():
                lv, la = np.asarray(lv, np.float64), np.asarray(a["losses"][name], np.float64)
                fig[f"loss/{name}"] = float(np.max(np.abs(la - lv) / (bound * np.maximum(1.0, np.abs(lv)))))
        else:
            assert np.shape(a[k]) == np.shape(v), (k, np.shape(a[k]), np.shape(v))
            fig[k] = rel_l2(a[k], v) / bound
    ok = all(np.isfinite(f) and f <= 1.0 for f in fig.values())
    return ok, fig


def report(label, fig, bound=BOUND):
    """Print every figure (as error / bound) of one comparison; returns the worst (name, ratio)."""
    worst = max(fig.items(), key=lambda kv: (not np.isfinite(kv[1]), kv[1]))
    print(f"[sched] {label}: bound {bound:.1e}, worst {worst[0]} at {worst[1]:.3e} of the bound")
    for k, f in fig.items():
        print(f"[sched]     {k:34s} {f * bound:.3e}  ({f:.3e} of the bound)")
    return worst


def timed_as_is_step(m, inp, draws, **kw):
    """run_step under the as-is timing with two events around it: (outputs, milliseconds on the device)."""
    install(m, "as-is")
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    m.train_step(*inp, draws=draws, **kw)
    e1.record()
    torch.cuda.synchronize()
    return step_outputs(m), e0.elapsed_time(e1)


def run_timings(m, inp, draws, scrub_inp, scrub_draws, style_factor=None):
    """The same step of the built trainer `m` (apply=False: the weights stay) serialised, as-is and delayed, each behind a serialised
    scrub step on another batch, so that every buffer holds another step's values when the compared step begins.  The delayed run's
    coarse lag is max(COARSE_MS, the as-is step's device time), at most MAX_SPIN_MS.  Returns ({timing: outputs}, info)."""
    out, info = {}, {}

    def scrub():
        install(m, "serialised")
        run_step(m, scrub_inp, scrub_draws, style_factor)

    scrub()
    pt, pm = install(m, "serialised")
    out["serialised"] = run_step(m, inp, draws, style_factor)
    info["submissions"] = (pt.submissions, pm.submissions)
    scrub()
    out["as-is"], step_ms = timed_as_is_step(m, inp, draws, style_factor=style_factor, apply=False)
    scrub()
    coarse = min(MAX_SPIN_MS, max(COARSE_MS, step_ms))
    install(m, "delayed", coarse, FINE_MS)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    m.train_step(*inp, draws=draws, style_factor=style_factor, apply=False)
    e1.record()
    torch.cuda.synchronize()
    out["delayed"] = step_outputs(m)
    install(m, "as-is")
    info.update(step_ms=step_ms, coarse_ms=coarse, fine_ms=FINE_MS, delayed_ms=e0.elapsed_time(e1))
    print(f"[sched] undelayed step {step_ms:.2f} ms, submissions trainer/models {info['submissions']}, coarse lag {coarse:.1f} ms, "
          f"fine lag {FINE_MS:.1f} ms, delayed step {info['delayed_ms']:.1f} ms")
    return out, info
