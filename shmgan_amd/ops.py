"""Thin tensor-level wrappers over the C ABI (include/shmgan_hip.h).

PyTorch tensors are storage only: every function takes float32 CUDA(ROCm) tensors, passes
their device pointers to libshmgan_hip.so on torch's current stream and returns nothing
(outputs are preallocated by the caller).  No torch.nn op runs here.
"""
from __future__ import annotations

import functools
import math

import torch

from ._lib import CONSTANTS, check, lib


def _stream():
    return torch.cuda.current_stream().cuda_stream


class KernelTimer:
    """HIP-event timing of the MFMA conv launches on the stream they run on (bench.py
    `roofline`).  Enabled by setting ops.TIMER = KernelTimer(); records (kernel symbol,
    algorithmic flops, start event, end event) per launch.  The symbol is the one the entry point reports
    through shm_last_kernel() (plus a suffix when the timed region holds more than that kernel)."""

    def __init__(self):
        self.recs = []
        self.brecs = []          # HBM-bound passes: (entry point, algorithmic bytes, start event, end event)

    def wrap(self, sym, flops, fn, label="", fixed=False):
        e0 = torch.cuda.Event(enable_timing=True)
        e1 = torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        if not fixed:
            k = lib().shm_last_kernel()               # the variant the entry point actually dispatched to
            sym = (k.decode() if k else "?") + sym
        self.recs.append((sym, flops, e0, e1, label))

    def wrap_bytes(self, name, nbytes, fn):
        e0 = torch.cuda.Event(enable_timing=True)
        e1 = torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        if callable(nbytes):                 # bytes that depend on the path the entry point took (known after the call)
            nbytes = nbytes()
        self.brecs.append((name, nbytes, e0, e1))

    @staticmethod
    def _fold(rows, unit):
        """{key: dict(launches, ms, <unit>)} of rows (key, amount, start event, end event) -- call after a device synchronize."""
        out = {}
        for key, amount, e0, e1 in rows:
            d = out.setdefault(key, {"launches": 0, "ms": 0.0, unit: 0.0})
            d["launches"] += 1
            d["ms"] += e0.elapsed_time(e1)
            d[unit] += amount
        return out

    def bytes_summary(self):
        """{entry point: dict(launches, ms, bytes)} of the HBM-bound passes (algorithmic bytes: every tensor the pass must read or
        write, once) -- call after a device synchronize."""
        return self._fold(self.brecs, "bytes")

    def per_shape(self):
        """{(symbol, label): dict(launches, ms, flops)} for tuning."""
        return self._fold((((sym, label), flops, e0, e1) for sym, flops, e0, e1, label in self.recs), "flops")

    def summary(self):
        """{symbol: dict(launches, ms, flops)} -- call after a device synchronize."""
        return self._fold((r[:4] for r in self.recs), "flops")


TIMER = None


def _timed(sym, flops, fn, label=""):
    if TIMER is None:
        fn()
    else:
        TIMER.wrap(sym, flops, fn, label)


def _timed_bytes(name, nbytes, fn):
    if TIMER is None:
        fn()
    else:
        TIMER.wrap_bytes(name, nbytes, fn)


def _p(t):
    return 0 if t is None else t.data_ptr()


_F32, _BF16, _BF16_GF32 = CONSTANTS["SHM_F32"], CONSTANTS["SHM_BF16"], CONSTANTS["SHM_BF16_GF32"]


def _dtc(dtype):
    """SHM_BF16 for torch.bfloat16, SHM_F32 for any other torch dtype (the shape queries, which see no tensor)."""
    return _BF16 if dtype == torch.bfloat16 else _F32


def _dt(t):
    """SHM_F32 / SHM_BF16 code of an activation tensor."""
    if t.dtype == torch.bfloat16:
        return _BF16
    if t.dtype == torch.float32:
        return _F32
    raise TypeError(f"activation tensors are float32 or bfloat16, got {t.dtype}")


def _dtg(act, grad):
    """dtype code of a call with activation tensor `act` and gradient-signal ([G]) tensor `grad`:
    SHM_BF16_GF32 when the activations are bf16 and the gradient signal is kept in fp32."""
    d = _dt(act)
    if d == _BF16 and grad is not None and grad.dtype == torch.float32:
        return _BF16_GF32
    if grad is not None and _dt(grad) != d:
        raise TypeError("gradient-signal tensors are float32, or share the activation dtype")
    return d


# the header's SHM_TG_<NAME> by lower-case name (SHM_TG_DMA_128x64 is "dma128x64")
TAPGEMM_VARIANTS = {k[len("SHM_TG_"):].lower().replace("dma_", "dma"): v for k, v in CONSTANTS.items()
                    if k.startswith("SHM_TG_") and k != "SHM_TG_COUNT"}
assert sorted(TAPGEMM_VARIANTS.values()) == list(range(CONSTANTS["SHM_TG_COUNT"])), TAPGEMM_VARIANTS


def set_tuning(key, value):
    """shm_set_tuning: dispatch knobs of the MFMA kernels ("tapgemm.variant", "wgrad.variant", ... see the header);
    `value` may be a TAPGEMM_VARIANTS name.  set_tuning("reset", 0) restores every default."""
    if isinstance(value, str):
        value = TAPGEMM_VARIANTS[value]
    check(lib().shm_set_tuning(key.encode(), int(value)), "shm_set_tuning")


def get_tuning(key):
    import ctypes
    v = ctypes.c_int(0)
    check(lib().shm_get_tuning(key.encode(), ctypes.addressof(v)), "shm_get_tuning")
    return v.value


def last_kernel():
    k = lib().shm_last_kernel()
    return k.decode() if k else ""


def cast_f32(src, dst, n):
    check(lib().shm_cast_f32(_p(src), _p(dst), n, _dt(dst), _stream()), "shm_cast_f32")


class TransposeBatch:
    """Host tables of shm_transpose_taps_multi for a fixed set of (w, wt, ntaps, rows, cols, rows_pad): built once (the
    tensors are persistent views), launched after every optimizer step."""

    def __init__(self, items):
        import ctypes as C
        self.items = list(items)              # keeps the tensors alive
        n = len(self.items)
        assert n <= 48
        self.n = n
        self.dt = _dt(self.items[0][1]) if n else 0
        assert all(_dt(it[1]) == self.dt for it in self.items)
        self.w = (C.c_void_p * n)(*[it[0].data_ptr() for it in self.items])
        self.wt = (C.c_void_p * n)(*[it[1].data_ptr() for it in self.items])
        self.ntaps, self.rows, self.cols, self.rows_pad = [(C.c_int * n)(*[int(it[k]) for it in self.items]) for k in (2, 3, 4, 5)]

    def run(self):
        if self.n:
            check(lib().shm_transpose_taps_multi(self.n, self.w, self.wt, self.ntaps, self.rows, self.cols, self.rows_pad, self.dt, _stream()),
                  "shm_transpose_taps_multi")


def transpose_taps(w, wt, ntaps, rows, cols, rows_pad):
    check(lib().shm_transpose_taps(_p(w), _p(wt), ntaps, rows, cols, rows_pad, _dt(wt), _stream()), "shm_transpose_taps")


def conv2d_fwd(x, x2, c1, ldx, ldx2, wk, bias, y, ldy, batch, hi, wi, cin, cout, ksize, stride, slope,
               cin_real=None, gsum=None):
    """cin_real: un-padded input channels, only used for the algorithmic flop count.
    gsum = (aux, ldaux, red): shm_conv2d_fwd_gsum (the stride-2 forward form is Conv2DTranspose's input gradient)."""
    ho, wo = -(-hi // stride), -(-wi // stride)
    flops = 2.0 * batch * ho * wo * ksize * ksize * (cin_real or cin) * cout
    label = f"fwd n{batch} h{hi} {cin}->{cout} k{ksize} s{stride}"
    if gsum is None:
        _timed("", flops, lambda: check(
            lib().shm_conv2d_fwd(_p(x), _p(x2), c1, ldx, ldx2, _p(wk), _p(bias), _p(y), ldy, batch, hi, wi,
                                 cin, cout, ksize, stride, slope, _dtg(x, y), _stream()), "shm_conv2d_fwd"), label)
        return
    aux, ldaux, red = gsum
    _timed("", flops, lambda: check(
        lib().shm_conv2d_fwd_gsum(_p(x), _p(x2), c1, ldx, ldx2, _p(wk), _p(bias), _p(y), ldy, batch, hi, wi, cin, cout, ksize, stride,
                                  slope, _p(aux), ldaux, _p(red), _dtg(x, y), _stream()), "shm_conv2d_fwd_gsum"), label + " +gsum")


STATS_SLOTS = CONSTANTS["SHM_STATS_SLOTS"]


NORM_EXACT, NORM_SCALED = CONSTANTS["SHM_NORM_EXACT"], CONSTANTS["SHM_NORM_SCALED"]


def conv2d_in_fwd(x, x2, c1, ldx, ldx2, wk, bias, y, ldy, batch, hi, wi, cin, cout, ksize, stride, slope, stats, eps,
                  cin_real=None, scratch=None, nt_x=None, nt_x2=None, nt_out=None, beta_out=None, norm_mode=NORM_EXACT):
    """conv2d_fwd fused with the InstanceNorm statistics of its output (stats <- mean, inv-std).
    scratch: optional f64 [STATS_SLOTS * batch * cout * 2] (spreads the statistics atomics).
    nt_x / nt_x2: x / x2 is the UN-normalised activation of an InstanceNorm block and this is that block's table
    (shm_conv2d_in_fwd_norm: NORM_EXACT -- the kernel normalises its operand tile in LDS; NORM_SCALED -- wk and bias are
    conv2d_norm_prepare's per-sample operands); nt_out (+ beta_out): this block's own table."""
    ho, wo = -(-hi // stride), -(-wi // stride)
    flops = 2.0 * batch * ho * wo * ksize * ksize * (cin_real or cin) * cout
    label = f"fwd n{batch} h{hi} {cin}->{cout} k{ksize} s{stride}"
    if nt_x is None and nt_x2 is None and nt_out is None:
        _timed("", flops, lambda: check(
            lib().shm_conv2d_in_fwd(_p(x), _p(x2), c1, ldx, ldx2, _p(wk), _p(bias), _p(y), ldy, batch, hi, wi,
                                    cin, cout, ksize, stride, slope, _p(stats), _p(scratch), eps, _dt(x), _stream()),
            "shm_conv2d_in_fwd"), label)
        return
    _timed("", flops, lambda: check(
        lib().shm_conv2d_in_fwd_norm(_p(x), _p(x2), c1, ldx, ldx2, _p(nt_x), _p(nt_x2), norm_mode, _p(wk), _p(bias), _p(y), ldy, batch, hi, wi,
                                     cin, cout, ksize, stride, slope, _p(stats), _p(scratch), eps, _p(nt_out), _p(beta_out), _dt(x), _stream()),
        "shm_conv2d_in_fwd_norm"), label + (" +norm" if (nt_x is not None or nt_x2 is not None) else ""))


def conv2d_norm_prepare(wk, bias, nt, c, part_lo, wk_n, bias_n, batch, cin, cout, ksize):
    """NORM_SCALED operands: per-sample weights (the folded source's channels times inv) and bias rows."""
    check(lib().shm_conv2d_norm_prepare(_p(wk), _p(bias), _p(nt), c, part_lo, _p(wk_n), _p(bias_n), batch, cin, cout, ksize, _dt(wk), _stream()),
          "shm_conv2d_norm_prepare")


def conv2d_wgrad_norm_workspace(batch, hi, wi, cin, cout, ksize, dtype):
    return int(lib().shm_conv2d_wgrad_norm_workspace(batch, hi, wi, cin, cout, ksize, _dtc(dtype)))


def conv2d_wgrad_norm_finish(dw, nt, dzsum, batch, c, part_lo, cin, cout, ksize):
    """NORM_SCALED weight gradient, second term: dw[tap][part_lo + k][co] += sum_n (beta - mean * inv)[n][k] * dzsum[n][co]."""
    check(lib().shm_conv2d_wgrad_norm_finish(_p(dw), _p(nt), _p(dzsum), batch, c, part_lo, cin, cout, ksize, _stream()), "shm_conv2d_wgrad_norm_finish")


def conv2d_norm_supported(batch, hi, wi, cin, c1, cout, ksize, stride, norm_part, dtype):
    """Would conv2d_in_fwd(nt_x= / nt_x2=) run on a kernel that normalises source `norm_part` in LDS?  (c1: channels of x when
    there are two sources, else 0; dtype: torch dtype of the activations.)"""
    return bool(lib().shm_conv2d_norm_supported(batch, hi, wi, cin, c1, cout, ksize, stride, norm_part, _dtc(dtype)))


def conv2d_wgrad_norm_supported(batch, hi, wi, cin, cin_ld, c1, cout, ksize, stride, norm_part, dtype):
    return bool(lib().shm_conv2d_wgrad_norm_supported(batch, hi, wi, cin, cin_ld, c1, cout, ksize, stride, norm_part, _dtc(dtype)))


def in_norm_table(stats, beta, nt, batch, c):
    check(lib().shm_in_norm_table(_p(stats), _p(beta), _p(nt), batch, c, _stream()), "shm_in_norm_table")


GSUM_SLOTS = CONSTANTS["SHM_GSUM_SLOTS"]
# InstanceNorm-backward sums in the producing epilogue (model.py).  Default by activation dtype: ON in float32 -- the convolutions
# are MFMA bound there and take the extra aux read in their stride: -3.4 ms of reduce passes for +1.3 ms of epilogues per step at
# BASELINE configs[1] -- OFF in bfloat16, where the same epilogues sit in latency-bound kernels and cost what the reduce passes
# saved (rocprofv3, profiles/README.md round 3).  SHM_GSUM=0 / 1 overrides both (A/B measurements).
import os as _os


def gsum_default(dtype):
    env = _os.environ.get("SHM_GSUM")
    if env is not None:
        return env not in ("0", "")
    return dtype == torch.float32


def conv2d_dgrad(dy, lddy, w, dx, dx2, n1, lddx, lddx2, batch, hi, wi, cin, cout, ksize, stride, gsum=None, gsum2=None):
    """gsum / gsum2 = (aux, ldaux, red) for the dx / dx2 part: the epilogue also delivers the InstanceNorm-backward sums of the
    block whose output gradient that part is (shm_conv2d_dgrad_gsum; red = f64 [GSUM_SLOTS * batch * channels * 2], zero on entry)."""
    ho, wo = -(-hi // stride), -(-wi // stride)
    flops = 2.0 * batch * ho * wo * ksize * ksize * cin * cout
    label = f"dgrad n{batch} h{hi} {cin}<-{cout} k{ksize} s{stride}"
    if gsum is None and gsum2 is None:
        _timed("", flops, lambda: check(
            lib().shm_conv2d_dgrad(_p(dy), lddy, _p(w), _p(dx), _p(dx2), n1, lddx, lddx2, batch, hi, wi, cin,
                                   cout, ksize, stride, _dtg(dy, dx), _stream()), "shm_conv2d_dgrad"), label)
        return
    a1, l1, r1 = gsum or (None, 0, None)
    a2, l2, r2 = gsum2 or (None, 0, None)
    _timed("", flops, lambda: check(
        lib().shm_conv2d_dgrad_gsum(_p(dy), lddy, _p(w), _p(dx), _p(dx2), n1, lddx, lddx2, batch, hi, wi, cin, cout, ksize, stride,
                                    _p(a1), l1, _p(r1), _p(a2), l2, _p(r2), _dtg(dy, dx), _stream()), "shm_conv2d_dgrad_gsum"),
           label + " +gsum")


def conv2d_transpose_fwd(x, ldx, w, bias, y, ldy, batch, hi, wi, cin, cout, slope):
    flops = 2.0 * batch * hi * wi * 9 * cin * cout
    _timed("", flops, lambda: check(
        lib().shm_conv2d_transpose_fwd(_p(x), ldx, _p(w), _p(bias), _p(y), ldy, batch, hi, wi, cin, cout,
                                       slope, _dt(x), _stream()), "shm_conv2d_transpose_fwd"),
           f"convT n{batch} h{hi} {cin}->{cout}")


def conv2d_wgrad_workspace(batch, ho, wo, cin, cout, ksize):
    return int(lib().shm_conv2d_wgrad_workspace(batch, ho, wo, cin, cout, ksize))


def conv2d_wgrad(x, x2, c1, ldx, ldx2, dy, lddy, dw, batch, hi, wi, cin, cin_ld, cout, ksize, stride,
                 accumulate, ws, nt_x=None, nt_x2=None, norm_mode=NORM_EXACT):
    """nt_x / nt_x2: x / x2 is the un-normalised activation of an InstanceNorm block, normalised in LDS (shm_conv2d_wgrad_norm)."""
    ho, wo = -(-hi // stride), -(-wi // stride)
    flops = 2.0 * batch * ho * wo * ksize * ksize * cin * cout
    label = f"wgrad n{batch} h{hi} {cin}x{cout} k{ksize} s{stride}"
    wsb = ws.numel() * ws.element_size()
    if (nt_x is not None or nt_x2 is not None) and TIMER is None:
        check(lib().shm_conv2d_wgrad_norm(_p(x), _p(x2), c1, ldx, ldx2, _p(nt_x), _p(nt_x2), norm_mode, _p(dy), lddy, _p(dw), batch, hi, wi, cin, cin_ld,
                                          cout, ksize, stride, int(accumulate), _p(ws), wsb, _dt(x), _stream()), "shm_conv2d_wgrad_norm")
        return
    if TIMER is None:
        check(lib().shm_conv2d_wgrad(_p(x), _p(x2), c1, ldx, ldx2, _p(dy), lddy, _p(dw), batch, hi, wi, cin, cin_ld,
                                     cout, ksize, stride, int(accumulate), _p(ws), wsb, _dt(x), _stream()),
              "shm_conv2d_wgrad")
        return
    # timing mode: the two phases as separate calls, so the MFMA kernel's events hold nothing else
    import ctypes
    ns = ctypes.c_int(0)
    if nt_x is not None or nt_x2 is not None:
        TIMER.wrap("", flops, lambda: check(
            lib().shm_conv2d_wgrad_partial_norm(_p(x), _p(x2), c1, ldx, ldx2, _p(nt_x), _p(nt_x2), norm_mode, _p(dy), lddy, batch, hi, wi, cin, cin_ld, cout,
                                                ksize, stride, _p(ws), wsb, _dt(x), ctypes.addressof(ns), _stream()),
            "shm_conv2d_wgrad_partial_norm"), label + " +norm")
    else:
        TIMER.wrap("", flops, lambda: check(
            lib().shm_conv2d_wgrad_partial(_p(x), _p(x2), c1, ldx, ldx2, _p(dy), lddy, batch, hi, wi, cin, cin_ld, cout,
                                           ksize, stride, _p(ws), wsb, _dt(x), ctypes.addressof(ns), _stream()),
            "shm_conv2d_wgrad_partial"), label)
    TIMER.wrap("wgrad_reduce_kernel", 0.0, lambda: check(
        lib().shm_conv2d_wgrad_reduce(_p(ws), _p(dw), ksize * ksize * cin * cout, ns.value, int(accumulate), _stream()),
        "shm_conv2d_wgrad_reduce"), label, fixed=True)


def in_stats(a, lda, stats, batch, hw, c, eps):
    check(lib().shm_in_stats(_p(a), lda, _p(stats), batch, hw, c, eps, _dt(a), _stream()), "shm_in_stats")


def _tb(t, n_elems):
    return float(n_elems) * t.element_size()


def in_apply_pool(a, lda, stats, beta, out, ldo, pooled, ldp, batch, h, w, c):
    e = batch * h * w * c                          # read a, write out, write pooled (a quarter)
    _timed_bytes("shm_in_apply_pool", _tb(a, 2.25 * e), lambda: check(
        lib().shm_in_apply_pool(_p(a), lda, _p(stats), _p(beta), _p(out), ldo, _p(pooled), ldp, batch, h, w, c, _dt(a), _stream()),
        "shm_in_apply_pool"))


def in_pool(a, lda, stats, beta, pooled, ldp, batch, h, w, c):
    """pooled = AveragePooling2D(2)(IN apply(a)) without writing the normalised tensor (its other consumers normalise on the fly)."""
    e = batch * h * w * c                          # read a, write pooled (a quarter)
    _timed_bytes("shm_in_pool", _tb(a, 1.25 * e), lambda: check(
        lib().shm_in_pool(_p(a), lda, _p(stats), _p(beta), _p(pooled), ldp, batch, h, w, c, _dt(a), _stream()), "shm_in_pool"))


def in_apply(a, lda, stats, beta, out, ldo, batch, hw, c):
    _timed_bytes("shm_in_apply", _tb(a, 2 * batch * hw * c), lambda: check(
        lib().shm_in_apply(_p(a), lda, _p(stats), _p(beta), _p(out), ldo, batch, hw, c, _dt(a), _stream()), "shm_in_apply"))


class AbortWords:
    """The pair of words a kernel that had to give up reports to (include/shmgan_hip.h, the one-pass form of shm_in_bwd): `dev`, an int32 CUDA
    tensor of one element that in_bwd(abort=) sets and adam_clip(abort=) checks on the device, and `host`, a PINNED host tensor of one element
    (ROCm maps pinned host memory into the device's address space at the same address) that the kernel sets to 1 itself.  The library keeps
    no pointer to either: whoever owns the pair (model.Arena) outlives the launches it is handed to."""

    def __init__(self, device):
        self.dev = torch.zeros(1, dtype=torch.int32, device=device)
        self.host = torch.zeros(1, dtype=torch.int32).pin_memory()
        assert self.host.is_pinned() and not self.host.is_cuda and self.dev.is_cuda
        self.np = self.host.numpy()

    def tripped(self, sync=False):
        """One read of host memory; sync=True waits for the device first and reads its word too (exact)."""
        if sync:
            torch.cuda.synchronize(self.dev.device)
        return int(self.np[0]) != 0 or (sync and int(self.dev.item()) != 0)

    def clear(self):
        torch.cuda.synchronize(self.dev.device)
        self.dev.zero_()
        self.np[0] = 0
        torch.cuda.synchronize(self.dev.device)


def set_clock_probe(dev2):
    """shm_set_clock_probe: dev2 = an int64 CUDA tensor of two elements (or None)."""
    check(lib().shm_set_clock_probe(_p(dev2)), "shm_set_clock_probe")


def in_bwd_fused_doubles(batch, hw, c):
    """SHM_IN_BWD_FUSED_DOUBLES: float64 elements of the one-pass form's scratch (per-block partial rows, means, counters and flags)."""
    cb = min(c, 64)
    return (batch * (hw * cb // 16384) * 3 * c + 1) // 2 + batch * c + batch * (c // cb) * 288 + 1


def in_bwd(g1, ldg1, g2, ldg2, a, lda, stats, red, dz, lddz, dbias, batch, h, w, c, slope, fused=None, dz_sums=None, abort=None):
    """fused: float64 scratch of in_bwd_fused_doubles(batch, h * w, c) elements (zero on entry, zero on return): the call may run the one-pass
    bf16 form; the library falls back to reduce + apply on shapes that form does not take.
    abort: the AbortWords a barrier of that form sets when it gives up (None: only the scratch's own last word records it).
    dz_sums (here, in in_bwd_apply and in in_bwd_rank1): float64 [batch][c], receives the per-sample channel sums of dz; needs dbias."""
    e = batch * h * w * c
    rd = _tb(g1, e * (1.25 if g2 is not None else 1.0)) + _tb(a, e)

    def nb():
        # bytes of the path the call took: the one-pass form reads g1 [+ g2 / 4] and a once and writes dz; reduce + apply read g and a twice
        # (round-5 advisor: three passes were counted for every call, understating the two-pass calls)
        return (rd if last_kernel().startswith("in_bwd_fused") else 2 * rd) + _tb(dz, e)

    _timed_bytes("shm_in_bwd", nb, lambda: check(
        lib().shm_in_bwd(_p(g1), ldg1, _p(g2), ldg2, _p(a), lda, _p(stats), _p(red), _p(dz), lddz, _p(dbias), _p(dz_sums), _p(fused),
                         0 if fused is None else fused.numel(), _p(abort and abort.dev), _p(abort and abort.host), batch, h, w, c, slope, _dtg(a, g1), _stream()), "shm_in_bwd"))


def in_bwd_apply(g1, ldg1, g2, ldg2, a, lda, stats, beta, red, redp, dstage, dz, lddz, dbias, batch, h, w, c, slope, dz_sums=None):
    """shm_in_bwd without its reduce pass: the sums come from the gsum epilogues of the launches that wrote g1 / g2."""
    e = batch * h * w * c
    nb = _tb(g1, e * (1.25 if g2 is not None else 1.0)) + _tb(a, e) + _tb(dz, e)
    _timed_bytes("shm_in_bwd_apply", nb, lambda: check(
        lib().shm_in_bwd_apply(_p(g1), ldg1, _p(g2), ldg2, _p(a), lda, _p(stats), _p(beta), _p(red), _p(redp), _p(dstage), _p(dz), lddz,
                               _p(dbias), _p(dz_sums), batch, h, w, c, slope, _dtg(a, g1), _stream()), "shm_in_bwd_apply"))


LRELU_RED_SLOTS = CONSTANTS["SHM_LRELU_RED_SLOTS"]


def lrelu_bwd(dy, lddy, y, ldy, dz, lddz, dbias, npix, c, slope, red=None):
    """red: f64 scratch [LRELU_RED_SLOTS * c], required with dbias."""
    check(lib().shm_lrelu_bwd(_p(dy), lddy, _p(y), ldy, _p(dz), lddz, _p(dbias), _p(red), npix, c, slope, _dtg(y, dy), _stream()),
          "shm_lrelu_bwd")


def avgpool2_fwd(x, ldx, y, ldy, batch, h, w, c):
    check(lib().shm_avgpool2_fwd(_p(x), ldx, _p(y), ldy, batch, h, w, c, _dt(x), _stream()), "shm_avgpool2_fwd")


def cvt_f64_f32(src, dst, n, accumulate):
    check(lib().shm_cvt_f64_f32(_p(src), _p(dst), n, int(accumulate), _stream()), "shm_cvt_f64_f32")


def zero(t):
    check(lib().shm_zero(_p(t), t.numel() * t.element_size(), _stream()), "shm_zero")


def head_fwd(x, ldx, w, bias, y, npix, c, slope):
    check(lib().shm_head_fwd(_p(x), ldx, _p(w), _p(bias), _p(y), npix, c, slope, _dt(x), _stream()), "shm_head_fwd")


def head_in_fwd(a, lda, stats, beta, w, bias, y, batch, hw, c, slope):
    check(lib().shm_head_in_fwd(_p(a), lda, _p(stats), _p(beta), _p(w), _p(bias), _p(y), batch, hw, c, slope, _dt(a), _stream()), "shm_head_in_fwd")


def head_in_bwd(a, lda, stats, beta, w, y, dy, dx, lddx, dw_acc, db_acc, batch, hw, c, slope, red, dz_out=None):
    """dx may be None (then dz_out is required): the head's input gradient is dz_out (x) w, see in_bwd_rank1."""
    check(lib().shm_head_in_bwd(_p(a), lda, _p(stats), _p(beta), _p(w), _p(y), _p(dy), _p(dx), lddx, _p(dz_out), _p(dw_acc), _p(db_acc), _p(red), batch,
                                hw, c, slope, _dt(a) if dx is None else _dtg(a, dx), _stream()), "shm_head_in_bwd")


def in_bwd_rank1(hdz, hw_, a, lda, stats, red, dz, lddz, dbias, batch, h, w, c, slope, dz_sums=None):
    check(lib().shm_in_bwd_rank1(_p(hdz), _p(hw_), _p(a), lda, _p(stats), _p(red), _p(dz), lddz, _p(dbias), _p(dz_sums), batch, h, w, c, slope, _dt(a),
                                 _stream()), "shm_in_bwd_rank1")


def head_bwd(x, ldx, w, y, dy, dx, lddx, dw_acc, db_acc, npix, c, slope, red=None):
    """red: f64 scratch [LRELU_RED_SLOTS * (c + 1)] (allocated per call when omitted: tests only)."""
    if red is None:
        red = torch.empty(LRELU_RED_SLOTS * (c + 1), dtype=torch.float64, device=x.device)
    check(lib().shm_head_bwd(_p(x), ldx, _p(w), _p(y), _p(dy), _p(dx), lddx, _p(dw_acc), _p(db_acc), _p(red), npix, c,
                             slope, _dtg(x, dx), _stream()), "shm_head_bwd")


def patch_fwd(x, ldx, w, y, batch, h, wd, c, slope):
    check(lib().shm_patch_fwd(_p(x), ldx, _p(w), _p(y), batch, h, wd, c, slope, _dt(x), _stream()), "shm_patch_fwd")


def patch_bwd(x, ldx, w, y, dy, dz, dx, lddx, dw, batch, h, wd, c, slope):
    check(lib().shm_patch_bwd(_p(x), ldx, _p(w), _p(y), _p(dy), _p(dz), _p(dx), lddx, _p(dw), batch, h, wd, c,
                              slope, _dtg(x, dx), _stream()), "shm_patch_bwd")


def dense_fwd(x, w, y, batch, k, nout):
    check(lib().shm_dense_fwd(_p(x), _p(w), _p(y), batch, k, nout, _dt(x), _stream()), "shm_dense_fwd")


def dense_bwd(x, w, dy, dx, dw, batch, k, nout):
    check(lib().shm_dense_bwd(_p(x), _p(w), _p(dy), _p(dx), _p(dw), batch, k, nout, _dtg(x, dx), _stream()), "shm_dense_bwd")


def mul_mask(x, mask, y, n, scale):
    check(lib().shm_mul_mask(_p(x), _p(mask), _p(y), n, scale, _dt(x), _stream()), "shm_mul_mask")


def rgb2yuv_std(rgb, yuv, acc, scale_out, batch, npix):
    check(lib().shm_rgb2yuv_std(_p(rgb), _p(yuv), _p(acc), _p(scale_out), batch, npix, _stream()), "shm_rgb2yuv_std")


def avg_cbcr(ys, out, n):
    check(lib().shm_avg_cbcr(_p(ys[0]), _p(ys[1]), _p(ys[2]), _p(ys[3]), _p(ys[4]), _p(out), n, _stream()),
          "shm_avg_cbcr")


def build_gen_input(ys, gen_y, flags_mask, mode, out, batch, npix):
    check(lib().shm_build_gen_input(_p(ys[0]), _p(ys[1]), _p(ys[2]), _p(ys[3]), _p(ys[4]), _p(gen_y), flags_mask,
                                    mode, _p(out), out.shape[-1], batch, npix, _dt(out), _stream()), "shm_build_gen_input")


def cyc_input_bwd(dcyc, flags_mask, dgen_y, batch, npix):
    check(lib().shm_cyc_input_bwd(_p(dcyc), dcyc.shape[-1], flags_mask, _p(dgen_y), batch, npix, _dt(dcyc), _stream()),
          "shm_cyc_input_bwd")


def yuv2rgb(ych, cbcr, noise, rgb, dpad, nimg, batch, npix):
    check(lib().shm_yuv2rgb(_p(ych), _p(cbcr), _p(noise), _p(rgb), _p(dpad), 0 if dpad is None else dpad.shape[-1], nimg,
                            batch, npix, 0 if dpad is None else _dt(dpad), _stream()), "shm_yuv2rgb")


def pack_rgb16(rgb, noise, dpad, npix_total):
    check(lib().shm_pack_rgb16(_p(rgb), _p(noise), _p(dpad), dpad.shape[-1], npix_total, _dt(dpad), _stream()),
          "shm_pack_rgb16")


def rgb16_to_dy(d16, dy, npix_total, accumulate):
    check(lib().shm_rgb16_to_dy(_p(d16), d16.shape[-1], _p(dy), npix_total, int(accumulate), _dt(d16), _stream()),
          "shm_rgb16_to_dy")


def randn(out, stddev, seed, stream_id=0):
    """out ~ N(0, stddev^2), Philox-4x32-10 keyed by (seed, stream_id)."""
    check(lib().shm_randn(_p(out), out.numel(), stddev, int(seed) & 0xFFFFFFFFFFFFFFFF, int(stream_id), _stream()), "shm_randn")


def keep_mask(out, rate, seed, stream_id=0):
    """out = 1 with probability 1 - rate else 0 (Dropout keep mask)."""
    check(lib().shm_keep_mask(_p(out), out.numel(), rate, int(seed) & 0xFFFFFFFFFFFFFFFF, int(stream_id), _stream()), "shm_keep_mask")


XENT_TF_FUSED, XENT_INTENDED = CONSTANTS["SHM_XENT_TF_FUSED"], CONSTANTS["SHM_XENT_INTENDED"]


def dhead_losses(rf, cls, loss, drf_d, dcls_d, drf_g, batch, np_, target, xent_mode=XENT_TF_FUSED):
    """xent_mode: XENT_TF_FUSED = the class-logit gradient TF's fused softmax-cross-entropy kernel returns (softmax - labels:
    the reference as executed), XENT_INTENDED = the true derivative for the un-normalised D1 label row."""
    check(lib().shm_dhead_losses(_p(rf), _p(cls), _p(loss), _p(drf_d), _p(dcls_d), _p(drf_g), batch, np_, target,
                                 int(xent_mode), _stream()), "shm_dhead_losses")


def image_losses_workspace(batch, s):
    return image_losses_hw_workspace(batch, s, s)


def image_losses(gen_rgb, cyc_rgb, cyc_y, cbcr, orig_ptrs, ds_ptrs, flags_mask, style_factor, loss, dgen_y, dcyc_y,
                 ws, batch, s):
    """orig_ptrs / ds_ptrs: ctypes arrays of 5 device pointers (host memory, read at call time).  image_losses_hw with h = w = s."""
    image_losses_hw(gen_rgb, cyc_rgb, cyc_y, cbcr, orig_ptrs, ds_ptrs, flags_mask, style_factor, loss, dgen_y, dcyc_y, ws, batch, s, s)


def image_losses_hw_workspace(batch, h, w):
    return int(lib().shm_image_losses_hw_workspace(batch, h, w))


def image_losses_hw(gen_rgb, cyc_rgb, cyc_y, cbcr, orig_ptrs, ds_ptrs, flags_mask, style_factor, loss, dgen_y, dcyc_y,
                    ws, batch, h, w):
    """The image losses on [.,h,w,c] tensors (shm_image_losses_hw)."""
    check(lib().shm_image_losses_hw(_p(gen_rgb), _p(cyc_rgb), _p(cyc_y), _p(cbcr), orig_ptrs, ds_ptrs, flags_mask,
                                    style_factor, _p(loss), _p(dgen_y), _p(dcyc_y), _p(ws),
                                    ws.numel() * ws.element_size(), batch, h, w, _stream()), "shm_image_losses_hw")


# ---- image-quality metrics of the reference's test mode (test.py:332-392) --------------------------------------
METRIC_NAMES = ("mse", "psnr", "ssim", "de76", "de94")          # the columns of image_metrics' result
_METRIC_ARENAS = {}


def _default_arena(device):
    """This module's own arena of `device` (made at its first use), for the calls that are given none."""
    arena = _METRIC_ARENAS.get(device)
    if arena is None:
        from .model import Arena
        arena = _METRIC_ARENAS[device] = Arena(device)
    return arena


def _metrics_check(who, pred, target, window=None, region=None):
    """The dtype, shape and contiguity rules of `who`, one of the image_metrics family (no window: the square form, two [B,S,S,3]
    images).  Returns (B, Hp, Wp) of pred."""
    if pred.dtype != torch.float32 or target.dtype != torch.float32:
        raise TypeError(f"{who} takes float32 images, got {pred.dtype} / {target.dtype}")
    if region is not None and region.dtype != torch.uint8:
        raise TypeError(f"{who} takes a uint8 region, got {region.dtype}")
    images = [pred, target] + ([] if region is None else [region])
    got = " / ".join(str(tuple(t.shape)) for t in images)
    nhwc3 = pred.dim() == 4 and pred.shape[-1] == 3
    if window is None:
        if not nhwc3 or pred.shape[1] != pred.shape[2] or tuple(target.shape) != tuple(pred.shape):
            raise ValueError(f"{who} takes two [B,S,S,3] images of one shape, got {got}")
    else:
        h, w = window[2:]
        want = ["pred [B,Hp,Wp,3]", f"target [B,{h},{w},3]"] + ([] if region is None else [f"region [B,{h},{w}]"])
        if not nhwc3 or tuple(target.shape) != (pred.shape[0], h, w, 3) or (region is not None and tuple(region.shape) != (pred.shape[0], h, w)):
            raise ValueError(f"{who} takes {', '.join(want[:-1])} and {want[-1]}, got {got}")
    if not all(t.is_contiguous() for t in images):
        raise ValueError(f"{who} takes contiguous NHWC images" + ("" if region is None else " and a contiguous region"))
    return int(pred.shape[0]), int(pred.shape[1]), int(pred.shape[2])


def _metrics_out_ws(who, pred, out, arena, workspace, *dims, cols=5, key="metrics/ws"):
    """The checked (or new) float64 [B,cols] result tensor of `who` and its workspace of workspace(B, *dims) bytes, `key` of `arena`."""
    B = int(pred.shape[0])
    if out is None:
        out = torch.empty((B, cols), dtype=torch.float64, device=pred.device)
    elif out.dtype != torch.float64 or tuple(out.shape) != (B, cols) or not out.is_contiguous():
        raise ValueError(f"{who}: out must be a contiguous float64 [{B},{cols}] tensor")
    if arena is None:
        arena = _default_arena(pred.device)
    return out, arena.get(key, (max(workspace(B, *dims), 1),), torch.uint8)


def image_metrics_workspace(batch, s):
    return int(lib().shm_image_metrics_workspace(batch, s))


def image_metrics(pred, target, out=None, arena=None):
    """Per-image {mse, psnr, ssim, de76, de94} of pred (gen_rgb, not clipped) against target, both float32 [B,S,S,3] device
    tensors (shm_image_metrics, include/shmgan_hip.h, states the definitions).  Returns `out`, a float64 [B,5] device tensor
    (allocated when not given), filled asynchronously on the current stream.  The workspace comes from `arena` (default: one
    arena per device held by this module): calls that share an arena must be ordered on one stream."""
    B, S, _ = _metrics_check("image_metrics", pred, target)
    out, ws = _metrics_out_ws("image_metrics", pred, out, arena, image_metrics_workspace, S)
    check(lib().shm_image_metrics(_p(pred), _p(target), _p(out), _p(ws), ws.numel(), B, S, _stream()), "shm_image_metrics")
    return out


def image_metrics_hw_workspace(batch, h, w):
    return int(lib().shm_image_metrics_hw_workspace(batch, h, w))


def image_metrics_hw(pred, window, target, out=None, arena=None):
    """image_metrics on a window of a padded prediction (shm_image_metrics_hw): pred float32 [B,Hp,Wp,3], window = (top, left, h, w)
    the photo inside the frame, target tight float32 [B,h,w,3].  Same result tensor, workspace rule and ordering as image_metrics."""
    top, left, h, w = (int(v) for v in window)
    B, hp, wp = _metrics_check("image_metrics_hw", pred, target, (top, left, h, w))
    out, ws = _metrics_out_ws("image_metrics_hw", pred, out, arena, image_metrics_hw_workspace, h, w)
    check(lib().shm_image_metrics_hw(_p(pred), hp, wp, top, left, _p(target), h, w, _p(out), _p(ws), ws.numel(), B, _stream()),
          "shm_image_metrics_hw")
    return out


# ---- the metrics split by a region: the highlight and everything else (shm_highlight_region_hw / shm_image_metrics_region_hw) ----
REGION_MODES = {"residual": CONSTANTS["SHM_REGION_RESIDUAL"], "plane": CONSTANTS["SHM_REGION_PLANE"]}
REGION_METRICS = CONSTANTS["SHM_REGION_METRICS"]
# the columns of image_metrics_region's result: the five inside, the five outside, the pixels and the SSIM positions inside
REGION_METRIC_NAMES = tuple(f"{side}_{k}" for side in ("in", "out") for k in METRIC_NAMES) + ("n_in", "p_in")
assert len(REGION_METRIC_NAMES) == REGION_METRICS


def highlight_region(mode, window, *, src=None, target=None, plane=None, tau, out=None):
    """The highlight of a window as a uint8 [B,h,w] device tensor of 0 / 1 (shm_highlight_region_hw, one launch, asynchronous on the
    current stream).  window = (top, left, h, w) inside the frame.  mode "residual": src float32 [B,Hp,Wp,3] (the photo fed to the
    generator, the padded frame) and target tight float32 [B,h,w,3]: max_c(src_c - target_c) > tau; mode "plane": plane float32
    [B,Hp,Wp] or [B,Hp,Wp,1] (the SpecSeg output): plane > tau.  Strict comparison; a NaN is outside.  Returns `out` (allocated when
    not given)."""
    if mode not in REGION_MODES:
        raise ValueError(f"highlight_region: mode {mode!r} is not one of {tuple(REGION_MODES)}")
    top, left, h, w = (int(v) for v in window)
    if mode == "residual":
        if src is None or target is None or plane is not None:
            raise ValueError("highlight_region: mode 'residual' takes src and target, and no plane")
        if src.dtype != torch.float32 or target.dtype != torch.float32:
            raise TypeError(f"highlight_region takes float32 images, got {src.dtype} / {target.dtype}")
        if src.dim() != 4 or src.shape[-1] != 3 or tuple(target.shape) != (src.shape[0], h, w, 3):
            raise ValueError(f"highlight_region takes src [B,Hp,Wp,3] and target [B,{h},{w},3], got {tuple(src.shape)} / {tuple(target.shape)}")
        if not (src.is_contiguous() and target.is_contiguous()):
            raise ValueError("highlight_region takes contiguous NHWC images")
        frame = src
    else:
        if plane is None or src is not None or target is not None:
            raise ValueError("highlight_region: mode 'plane' takes plane, and neither src nor target")
        if plane.dtype != torch.float32:
            raise TypeError(f"highlight_region takes a float32 plane, got {plane.dtype}")
        if plane.dim() not in (3, 4) or (plane.dim() == 4 and plane.shape[-1] != 1):
            raise ValueError(f"highlight_region takes plane [B,Hp,Wp] or [B,Hp,Wp,1], got {tuple(plane.shape)}")
        if not plane.is_contiguous():
            raise ValueError("highlight_region takes a contiguous plane")
        frame = plane
    B, hp, wp = int(frame.shape[0]), int(frame.shape[1]), int(frame.shape[2])
    if out is None:
        out = torch.empty((B, max(h, 0), max(w, 0)), dtype=torch.uint8, device=frame.device)
    elif out.dtype != torch.uint8 or tuple(out.shape) != (B, h, w) or not out.is_contiguous():
        raise ValueError(f"highlight_region: out must be a contiguous uint8 [{B},{h},{w}] tensor")
    check(lib().shm_highlight_region_hw(REGION_MODES[mode], _p(src), _p(target), _p(plane), hp, wp, top, left, h, w, float(tau), _p(out), B,
                                        _stream()), "shm_highlight_region_hw")
    return out


def image_metrics_region_workspace(batch, h, w):
    return int(lib().shm_image_metrics_region_hw_workspace(batch, h, w))


def image_metrics_region(pred, window, target, region, out=None, arena=None):
    """image_metrics_hw split by `region` (uint8 [B,h,w] over the window, non-zero = inside; shm_image_metrics_region_hw): pred float32
    [B,Hp,Wp,3], window = (top, left, h, w), target tight float32 [B,h,w,3].  Returns `out`, a float64 [B,12] device tensor
    (REGION_METRIC_NAMES: the five metrics inside, the five outside, n_in, p_in; an empty set gives NaN), filled asynchronously on the
    current stream.  Workspace rule and ordering as image_metrics (its own arena buffer: both calls may be queued on one stream)."""
    top, left, h, w = (int(v) for v in window)
    B, hp, wp = _metrics_check("image_metrics_region", pred, target, (top, left, h, w), region)
    out, ws = _metrics_out_ws("image_metrics_region", pred, out, arena, image_metrics_region_workspace, h, w, cols=REGION_METRICS,
                              key="metrics/region_ws")
    check(lib().shm_image_metrics_region_hw(_p(pred), hp, wp, top, left, _p(target), h, w, _p(region), _p(out), _p(ws), ws.numel(), B,
                                            _stream()), "shm_image_metrics_region_hw")
    return out


# ---- training telemetry (shm_tensor_stats / shm_loss_ring_put, include/shmgan_hip.h) ---------------------------------------
TSTAT_NAMES = ["finite", "nan", "inf", "min", "max", "sum", "sumsq", "clipped"]     # SHM_TSTAT_* order
TSTAT_N, THIST_BINS, THIST_EMIN, TSTAT_MAX_SEGS = (CONSTANTS["SHM_" + k] for k in ("TSTAT_N", "THIST_BINS", "THIST_EMIN", "TSTAT_MAX_SEGS"))
LOSS_ROW_DL, LOSS_ROW_IL, LOSS_ROW_SL, LOSS_ROW_STEP, LOSS_ROW_ABORT, LOSS_ROW = (
    CONSTANTS["SHM_LOSS_ROW" + k] for k in ("_DL", "_IL", "_SL", "_STEP", "_ABORT", ""))


def tensor_stats_workspace(nseg, n):
    return int(lib().shm_tensor_stats_workspace(nseg, n))


class SegmentTable:
    """Host arrays of shm_tensor_stats' segment table, built once per table (a model's variables never move)."""

    def __init__(self, offsets, sizes):
        import ctypes as C
        self.n = len(offsets)
        if self.n != len(sizes):
            raise ValueError(f"tensor_stats: {len(offsets)} offsets for {len(sizes)} sizes")
        self.off = (C.c_size_t * max(self.n, 1))(*[int(o) for o in offsets])
        self.len = (C.c_size_t * max(self.n, 1))(*[int(z) for z in sizes])
        self.total = sum(int(z) for z in sizes)


def tensor_stats(x, offsets, sizes=None, scale=1.0, out=None, arena=None):
    """Per-segment statistics and sign / exponent histogram of the flat float32 device tensor x scaled by `scale`
    (shm_tensor_stats states the definitions): segment s is x[offsets[s] : offsets[s] + sizes[s]].  `offsets` may be a
    SegmentTable (then `sizes` is not given).  Returns (stats float64 [nseg, 8] in TSTAT_NAMES order, hist int64
    [nseg, 2, 44]), device tensors filled asynchronously on the current stream; `out` = such a pair to fill.  The workspace
    comes from `arena` (default: one arena per device held by this module): calls that share an arena must be ordered on
    one stream."""
    if x.dtype != torch.float32 or x.dim() != 1 or not x.is_contiguous():
        raise TypeError(f"tensor_stats takes a flat contiguous float32 tensor, got {x.dtype} {tuple(x.shape)}")
    tab = offsets if isinstance(offsets, SegmentTable) else SegmentTable(offsets, sizes)
    nseg, n = tab.n, x.numel()
    if out is None:
        out = (torch.empty((nseg, TSTAT_N), dtype=torch.float64, device=x.device),
               torch.empty((nseg, 2, THIST_BINS), dtype=torch.int64, device=x.device))
    stats, hist = out
    if (stats.dtype != torch.float64 or tuple(stats.shape) != (nseg, TSTAT_N) or not stats.is_contiguous()
            or hist.dtype != torch.int64 or tuple(hist.shape) != (nseg, 2, THIST_BINS) or not hist.is_contiguous()):
        raise ValueError(f"tensor_stats: out must be contiguous (float64 [{nseg},{TSTAT_N}], int64 [{nseg},2,{THIST_BINS}]) tensors")
    if arena is None:
        arena = _default_arena(x.device)
    nb = tensor_stats_workspace(nseg, n)
    ws = arena.get("tstats/ws", (max((nb + 7) // 8, 1),), torch.int64)
    _timed_bytes("shm_tensor_stats", 4.0 * tab.total, lambda: check(          # read every segment once
        lib().shm_tensor_stats(_p(x), n, tab.off, tab.len, nseg, scale, _p(stats), _p(hist), _p(ws), ws.numel() * 8, _stream()),
        "shm_tensor_stats"))
    return out


def loss_ring_put(dl, il, sl, abort_word, ring, row, step):
    """shm_loss_ring_put: the step's raw loss vectors, `step` and the abort word into row `row` of ring (float64 [R, LOSS_ROW])."""
    assert ring.dtype == torch.float64 and ring.dim() == 2 and ring.shape[1] == LOSS_ROW and ring.is_contiguous()
    assert dl.numel() == LOSS_ROW_DL and il.numel() == LOSS_ROW_IL and sl.numel() == LOSS_ROW_SL
    check(lib().shm_loss_ring_put(_p(dl), _p(il), _p(sl), _p(abort_word), _p(ring), ring.shape[0], row, step, _stream()),
          "shm_loss_ring_put")


# ---- test-mode image export (the images test.py:305-317 logs) ----------------------------------------------------------
EXPORT_MODES = {k: CONSTANTS["SHM_EXPORT_" + k.upper()] for k in ("rescale", "scale", "clip")}
EXPORT_DESC, EXPORT_HW_DESC, EXPORT_MAX_JOBS = CONSTANTS["SHM_EXPORT_DESC"], CONSTANTS["SHM_EXPORT_HW_DESC"], CONSTANTS["SHM_EXPORT_MAX_JOBS"]
EXPORT_ALIGN = 16                                         # start of every job's bytes in export_u8's output


def export_workspace(njobs):
    return int(lib().shm_export_u8_workspace(njobs))


def export_layout(sizes, channels):
    """Byte offsets of the jobs in export_u8's output and its total size: job j holds ho*wo*c bytes ([ho,wo,c] uint8, tightly
    packed) from an offset that is a multiple of EXPORT_ALIGN."""
    offs, n = [], 0
    for (ho, wo), c in zip(sizes, channels):
        offs.append(n)
        n += (int(ho) * int(wo) * int(c) + EXPORT_ALIGN - 1) // EXPORT_ALIGN * EXPORT_ALIGN
    return offs, n


def _export_jobs(who, planes, windows, sizes, modes, mul):
    """Host side of export_u8 (windows None: square planes, SHM_EXPORT_DESC words per job) and export_u8_hw (SHM_EXPORT_HW_DESC words):
    every plane, window and mode checked; returns (descriptor rows, destination offsets, total bytes)."""
    hw = windows is not None
    shape, rows = ("[Hs,Ws,C]", "Ws") if hw else ("[S,S,C]", "S")
    desc, chans = [], []
    for p, win, (ho, wo), m in zip(planes, windows if hw else [None] * len(planes), sizes, modes):
        if p.dtype != torch.float32 or not p.is_cuda:
            raise TypeError(f"{who} takes float32 device planes, got {p.dtype} on {p.device}")
        if p.dim() != 3 or p.shape[2] not in (1, 3) or (not hw and p.shape[0] != p.shape[1]):
            raise ValueError(f"{who} takes {shape} planes with C in {{1,3}}, got {tuple(p.shape)}")
        hs, ws_, c = int(p.shape[0]), int(p.shape[1]), int(p.shape[2])
        ld = int(p.stride(1))
        if p.stride(2) != 1 or ld < c or p.stride(0) != ws_ * ld:
            raise ValueError(f"{who}: plane strides {p.stride()} are not [{rows}*ld, ld, 1] with ld >= {c}")
        if isinstance(m, tuple) and len(m) == 2 and m[0] == "scale":
            mode, k = EXPORT_MODES["scale"], int(m[1])
            if mul is None or mul.dtype != torch.float32 or mul.dim() != 1 or not 0 <= k < mul.numel() or not mul.is_contiguous():
                raise ValueError(f"{who}: mode {m} needs a contiguous float32 mul with more than {k} elements")
        elif m in ("rescale", "clip"):
            mode, k = EXPORT_MODES[m], 0
        else:
            raise ValueError(f"{who}: mode {m!r} is not 'rescale', 'clip' or ('scale', k)")
        if hw:
            y0, x0, hc, wc = (int(v) for v in win)
            if min(y0, x0) < 0 or min(hc, wc) < 1 or y0 + hc > hs or x0 + wc > ws_:
                raise ValueError(f"{who}: window {tuple(win)} outside the {hs} x {ws_} plane")
            desc.append([hs, ws_, c, ld, y0, x0, hc, wc, int(ho), int(wo), mode, k])
        else:
            desc.append([hs, c, ld, int(ho), int(wo), mode, k])
        chans.append(c)
    offs, total = export_layout(sizes, chans)
    return [d + [o] for d, o in zip(desc, offs)], offs, total


def _export(who, planes, windows, sizes, modes, mul, out, arena):
    """export_u8 / export_u8_hw behind their own count checks: entry point shm_<who>, one call per EXPORT_MAX_JOBS planes."""
    import ctypes as C
    desc, offs, total = _export_jobs(who, planes, windows, sizes, modes, mul)
    dev = planes[0].device
    if out is None:
        out = torch.empty(max(total, 1), dtype=torch.uint8, device=dev)
    elif out.dtype != torch.uint8 or out.dim() != 1 or not out.is_contiguous() or out.numel() < total:
        raise ValueError(f"{who}: out must be a contiguous flat uint8 tensor of at least {total} bytes")
    if arena is None:
        arena = _default_arena(dev)
    need = export_workspace(EXPORT_MAX_JOBS)
    ws = arena.get("export/ws", (need,), torch.uint8)
    width = EXPORT_DESC if windows is None else EXPORT_HW_DESC
    assert all(len(d) == width for d in desc)
    for j0 in range(0, len(planes), EXPORT_MAX_JOBS):
        part = range(j0, min(len(planes), j0 + EXPORT_MAX_JOBS))
        src = (C.c_void_p * len(part))(*[planes[j].data_ptr() for j in part])
        dsc = (C.c_size_t * (width * len(part)))(*[v for j in part for v in desc[j]])
        check(getattr(lib(), "shm_" + who)(src, dsc, len(part), _p(mul), 0 if mul is None else mul.numel(), _p(out), out.numel(),
                                           _p(ws), need, _stream()), "shm_" + who)
    return out, offs


def export_u8(planes, sizes, modes, mul=None, out=None, arena=None):
    """float32 planes -> uint8 images (shm_export_u8, include/shmgan_hip.h, states the definitions).  planes: [S,S,C] device
    tensors, C in {1,3}, channels innermost with unit stride and a pixel pitch ld >= C (a channel slice of a wider NHWC tensor
    is fine); sizes: (ho, wo) per plane; modes: "rescale", "clip" or ("scale", k) per plane, k indexing `mul` (a float32 device
    tensor).  The images go into `out` (a flat uint8 device tensor of at least export_layout(...)[1] bytes, allocated when not
    given) at the offsets of export_layout.  Returns (out, offsets), filled asynchronously on the current stream.  The
    workspace comes from `arena` (default: one arena per device held by this module).  One shm_export_u8 call per
    EXPORT_MAX_JOBS planes (two launches at most each): a test-mode batch of 8 images with all 8 planes is one call."""
    n = len(planes)
    if n == 0 or len(sizes) != n or len(modes) != n:
        raise ValueError(f"export_u8: {n} planes, {len(sizes)} sizes, {len(modes)} modes")
    return _export("export_u8", planes, None, sizes, modes, mul, out, arena)


def export_u8_hw(planes, windows, sizes, modes, mul=None, out=None, arena=None):
    """export_u8 with rectangular planes and a source window per plane (shm_export_u8_hw): planes [Hs,Ws,C] float32 device tensors
    (C in {1,3}, pixel pitch ld >= C), windows (y0, x0, hc, wc) per plane -- the part that is exported: RESCALE takes its min / max
    there and the resampling maps it to the plane's (ho, wo) of `sizes`.  modes, mul, out, arena, the output layout (export_layout)
    and the return value are export_u8's."""
    n = len(planes)
    if n == 0 or len(sizes) != n or len(modes) != n or len(windows) != n:
        raise ValueError(f"export_u8_hw: {n} planes, {len(windows)} windows, {len(sizes)} sizes, {len(modes)} modes")
    return _export("export_u8_hw", planes, windows, sizes, modes, mul, out, arena)


def running_scale_mean(scale, acc, mul):
    """The reference's running mean of the standardisation scales (test.py:77, 218, 246; shm_running_scale_mean): for the
    batch's scale [B] (float32, what preprocess returns) in image order, acc (float64 [2] device {sum, count}, zero at the
    start of a test run) takes each scale in and mul[b] (float32 [B]) = the mean of every scale so far, this image's included."""
    B = int(scale.numel())
    if scale.dtype != torch.float32 or mul.dtype != torch.float32 or mul.numel() != B or acc.dtype != torch.float64 \
            or acc.numel() != 2 or not (scale.is_contiguous() and mul.is_contiguous() and acc.is_contiguous()):
        raise ValueError("running_scale_mean takes float32 scale [B], float64 acc [2] and float32 mul [B], contiguous")
    check(lib().shm_running_scale_mean(_p(scale), B, _p(acc), _p(mul), _stream()), "shm_running_scale_mean")
    return mul


def adam_alpha(lr0, beta_1, beta_2, iterations):
    """The `alpha` of adam_clip / adam after `iterations` updates: Keras Adam's step size on ExponentialDecay(lr0, 10000, 0.95)
    (SHM.py:169-175)."""
    t = iterations + 1
    lr = lr0 * 0.95 ** (iterations / 10000.0)
    return lr * math.sqrt(1.0 - beta_2 ** t) / (1.0 - beta_1 ** t)


def adam_clip(w, m, v, g, n, alpha, beta1, beta2, eps, gscale, abort=None):
    """abort: the step's AbortWords; the kernel applies nothing while their device word is set."""
    _timed_bytes("shm_adam_clip", 7.0 * 4 * n, lambda: check(          # read w, m, v, g; write w, m, v
        lib().shm_adam_clip(_p(w), _p(m), _p(v), _p(g), n, alpha, beta1, beta2, eps, gscale, _p(abort and abort.dev), _stream()), "shm_adam_clip"))


EMA_MAX_BLOCKS = CONSTANTS["SHM_EMA_MAX_BLOCKS"]            # the block cap of ema_update's grid-stride launch


def ema_decay_at(ema_decay, updates, warmup=True):
    """The `decay` of the ema_update call after `updates` earlier ones: ema_decay, or with `warmup` min(ema_decay, (1 + t) / (10 + t)),
    tf.train.ExponentialMovingAverage's num_updates rule (0.1 at t = 0, so the first steps forget the initial weights quickly).
    ema_decay outside [0, 1) raises ValueError."""
    d = float(ema_decay)
    if not 0.0 <= d < 1.0:
        raise ValueError(f"ema_decay {ema_decay!r} is not in [0, 1) (0 = off)")
    t = int(updates)
    return min(d, (1.0 + t) / (10.0 + t)) if warmup else d


def ema_update(ema, w, n, decay, abort=None):
    """ema += (1 - decay) * (w - ema) over the first n floats of two flat float32 device buffers (shm_ema_update states the arithmetic);
    decay = 0 copies w into ema bit for bit.  abort: the step's AbortWords; the kernel writes nothing while their device word is set."""
    _timed_bytes("shm_ema_update", (2.0 if decay == 0 else 3.0) * 4 * n, lambda: check(          # read ema (not for a copy), w; write ema
        lib().shm_ema_update(_p(ema), _p(w), n, decay, _p(abort and abort.dev), _stream()), "shm_ema_update"))


# ---- SpecSeg (inference only) ----------------------------------------------------------------
def pack_channels(src, ldsrc, c0, nc, dst, lddst, npix):
    check(lib().shm_pack_channels(_p(src), ldsrc, c0, nc, _p(dst), lddst, npix, _stream()), "shm_pack_channels")


def bn_apply(a, lda, gamma, beta, mean, var, eps, out, ldo, npix, c):
    check(lib().shm_bn_apply(_p(a), lda, _p(gamma), _p(beta), _p(mean), _p(var), eps, _p(out), ldo, npix, c,
                             _stream()), "shm_bn_apply")


def maxpool2_fwd(x, ldx, y, ldy, batch, h, w, c):
    check(lib().shm_maxpool2_fwd(_p(x), ldx, _p(y), ldy, batch, h, w, c, _stream()), "shm_maxpool2_fwd")


def conv2d_transpose2x2_fwd(x, ldx, w, bias, y, ldy, batch, hi, wi, cin, cout, slope=1.0):
    flops = 2.0 * batch * hi * wi * 4 * cin * cout
    _timed("", flops, lambda: check(
        lib().shm_conv2d_transpose2x2_fwd(_p(x), ldx, _p(w), _p(bias), _p(y), ldy, batch, hi, wi, cin, cout,
                                          slope, _dt(x), _stream()), "shm_conv2d_transpose2x2_fwd"),
           f"convT2 n{batch} h{hi} {cin}->{cout}")


def head_sigmoid_fwd(x, ldx, w, bias, y, npix, c):
    check(lib().shm_head_sigmoid_fwd(_p(x), ldx, _p(w), _p(bias), _p(y), npix, c, _stream()), "shm_head_sigmoid_fwd")


def spec_loss(cyc_y, cbcr, ds_ptrs, mask, loss, batch, npix):
    check(lib().shm_spec_loss(_p(cyc_y), _p(cbcr), ds_ptrs, _p(mask), _p(loss), batch, npix, _stream()),
          "shm_spec_loss")


# ---- SpecSeg training (specseg_train.hip) ------------------------------------------------------------
SST_MAX_BLOCKS = CONSTANTS["SHM_SST_MAX_BLOCKS"]
SEG_LOSS_NAMES = ("loss", "dice", "focal", "iou", "f1", "tp", "fp", "fn")     # the entries of seg_loss' result (SHM_SEG_LOSS_OUT)
SEG_LOSS_WS_DOUBLES = SST_MAX_BLOCKS * 7 + 8              # SHM_SEG_LOSS_WS_DOUBLES


def bn_train_ws_doubles(c):
    """SHM_BN_TRAIN_WS_DOUBLES: float64 elements of the workspace of bn_train_fwd / bn_train_bwd / head_logit_bwd."""
    return SST_MAX_BLOCKS * 2 * c + 2 * c


def bn_train_fwd(a, lda, gamma, beta, moving_mean, moving_var, momentum, eps, out, ldo, save, ws, npix, c):
    """BatchNormalization on batch statistics; save (float64 [2c]) <- mean, inv_std; the moving statistics (or None) are updated."""
    check(lib().shm_bn_train_fwd(_p(a), lda, _p(gamma), _p(beta), _p(moving_mean), _p(moving_var), momentum, eps, _p(out), ldo, _p(save), _p(ws),
                                 ws.numel() * ws.element_size(), npix, c, _stream()), "shm_bn_train_fwd")


def bn_train_bwd(dy, lddy, a, lda, gamma, save, dx, lddx, dgamma, dbeta, ws, npix, c):
    check(lib().shm_bn_train_bwd(_p(dy), lddy, _p(a), lda, _p(gamma), _p(save), _p(dx), lddx, _p(dgamma), _p(dbeta), _p(ws),
                                 ws.numel() * ws.element_size(), npix, c, _stream()), "shm_bn_train_bwd")


def maxpool2_bwd(x, ldx, dy, lddy, dx, lddx, batch, h, w, c, accumulate):
    """The window's gradient to its first maximum in row-major order; accumulate: onto the skip gradient already in dx."""
    check(lib().shm_maxpool2_bwd(_p(x), ldx, _p(dy), lddy, _p(dx), lddx, batch, h, w, c, int(accumulate), _stream()), "shm_maxpool2_bwd")


def conv2d_transpose2x2_dgrad(dy, lddy, w, dx, lddx, batch, hi, wi, cin, cout):
    flops = 2.0 * batch * hi * wi * 4 * cin * cout
    _timed("convt2_dgrad_kernel", flops, lambda: check(
        lib().shm_conv2d_transpose2x2_dgrad(_p(dy), lddy, _p(w), _p(dx), lddx, batch, hi, wi, cin, cout, _stream()),
        "shm_conv2d_transpose2x2_dgrad"), f"convT2 dgrad n{batch} h{hi} {cin}<-{cout}")


def conv2d_transpose2x2_wgrad_workspace(batch, hi, wi, cin, cout):
    return int(lib().shm_conv2d_transpose2x2_wgrad_workspace(batch, hi, wi, cin, cout))


def conv2d_transpose2x2_wgrad(x, ldx, dy, lddy, dw, dbias, ws, batch, hi, wi, cin, cout):
    flops = 2.0 * batch * hi * wi * 4 * cin * cout
    _timed("convt2_wgrad_kernel", flops, lambda: check(
        lib().shm_conv2d_transpose2x2_wgrad(_p(x), ldx, _p(dy), lddy, _p(dw), _p(dbias), _p(ws), ws.numel() * ws.element_size(), batch, hi, wi, cin, cout,
                                            _stream()), "shm_conv2d_transpose2x2_wgrad"), f"convT2 wgrad n{batch} h{hi} {cin}x{cout}")


def head_logit_fwd(x, ldx, w, bias, z, npix, c):
    check(lib().shm_head_logit_fwd(_p(x), ldx, _p(w), _p(bias), _p(z), npix, c, _stream()), "shm_head_logit_fwd")


def head_logit_bwd(x, ldx, w, dz, dx, lddx, dw, db, ws, npix, c):
    check(lib().shm_head_logit_bwd(_p(x), ldx, _p(w), _p(dz), _p(dx), lddx, _p(dw), _p(db), _p(ws), ws.numel() * ws.element_size(), npix, c, _stream()),
          "shm_head_logit_bwd")


def seg_loss(z, g, dz, out, ws, npix):
    """Dice + binary focal loss of logits z against target g; out (float64 [8], SEG_LOSS_NAMES); dz (or None) <- dloss/dz."""
    check(lib().shm_seg_loss(_p(z), _p(g), _p(dz), _p(out), _p(ws), ws.numel() * ws.element_size(), npix, _stream()), "shm_seg_loss")


def adam(w, m, v, g, n, alpha, beta1, beta2, eps, gscale=1.0, clip=0.0):
    """adam_clip's kernel with the clip bound as an argument (clip <= 0: none) and no abort word."""
    check(lib().shm_adam(_p(w), _p(m), _p(v), _p(g), n, alpha, beta1, beta2, eps, gscale, clip, _stream()), "shm_adam")


# ---- live attention branch --------------------------------------------------------------------------
def _mask_pool_pack(name, mask, dst, batch, *dims):
    check(getattr(lib(), name)(_p(mask), _p(dst), dst.shape[-1], batch, *dims, _dt(dst), _stream()), name)


def mask_pool_pack(mask, dst, batch, s, k):
    """MaxPooling2D(k) of mask [batch,s,s,1] into channel 0 of the activation tensor dst [batch,s/k,s/k,ld].  Its own entry point,
    not mask_pool_pack_hw(s, s): that one refuses s == 0 and a negative batch, which this one takes."""
    _mask_pool_pack("shm_mask_pool_pack", mask, dst, batch, s, k)


def mask_pool_pack_hw(mask, dst, batch, h, w, k):
    """mask_pool_pack on a rectangular mask [batch,h,w,1] -> dst [batch,h/k,w/k,ld]."""
    _mask_pool_pack("shm_mask_pool_pack_hw", mask, dst, batch, h, w, k)


def add_bcast(a, b, out, nimg, per, nb, i0=0):
    check(lib().shm_add_bcast(_p(a), _p(b), _p(out), nimg, per, nb, i0, _dt(a), _stream()), "shm_add_bcast")


def sum_groups(src, dst, nimg, per, nb, i0=0, accumulate=False):
    check(lib().shm_sum_groups(_p(src), _p(dst), nimg, per, nb, i0, int(accumulate), _dt(src), _stream()), "shm_sum_groups")


# ---- input pipeline ------------------------------------------------------------------------------
def resize_bilinear_u8(src_u8, dst, scale=1.0 / 255.0, flip_ud=False):
    """src_u8 [hin,win,c] uint8 device tensor -> dst [ho,wo,c] float32 (tf.image.resize bilinear, then * scale)."""
    hin, win, c = src_u8.shape
    ho, wo, _ = dst.shape
    check(lib().shm_resize_bilinear_u8(_p(src_u8), hin, win, c, _p(dst), ho, wo, scale, int(flip_ud), _stream()),
          "shm_resize_bilinear_u8")


def load_pad_u8(src_u8, dst, top, left, scale=1.0 / 255.0):
    """src_u8 [h,w,c] uint8 device tensor -> dst [hp,wp,c] float32: the image at (top, left), times scale, the border filled by
    reflection without the edge sample (shm_load_pad_u8; NumPy's mode="reflect")."""
    h, w, c = src_u8.shape
    hp, wp, c2 = dst.shape
    if src_u8.dtype != torch.uint8 or dst.dtype != torch.float32 or c2 != c or not (src_u8.is_contiguous() and dst.is_contiguous()):
        raise ValueError(f"load_pad_u8 takes contiguous uint8 [h,w,c] and float32 [hp,wp,c], got {src_u8.dtype} {tuple(src_u8.shape)} / "
                         f"{dst.dtype} {tuple(dst.shape)}")
    check(lib().shm_load_pad_u8(_p(src_u8), h, w, c, _p(dst), hp, wp, int(top), int(left), scale, _stream()), "shm_load_pad_u8")


# ---- full-resolution test output: guided detail transfer (shm_detail_coeffs / shm_detail_apply_u8) ---------------------------------
DETAIL_MAX_RADIUS = 8


def _detail_plane(t, who, what):
    """`who`'s check of one of its two model-resolution planes: float32 [B,H,W] (or [B,H,W,1]) on the device, rows and images dense
    behind a pixel pitch ld >= 1 (channel 0 of an NHWC tensor is fine).  Returns (the [B,H,W] view, ld)."""
    if t.dtype != torch.float32 or not t.is_cuda:
        raise TypeError(f"{who} takes float32 device planes, got {what} {t.dtype} on {t.device}")
    if t.dim() == 4 and t.shape[3] == 1:
        t = t[..., 0]
    if t.dim() != 3 or min(t.shape) < 1:
        raise ValueError(f"{who} takes {what} as [B,H,W] or [B,H,W,1], got {tuple(t.shape)}")
    B, H, W = (int(v) for v in t.shape)
    ld = int(t.stride(2)) if W > 1 else int(t.stride(1)) if H > 1 else int(t.stride(0)) if B > 1 else 1
    if ld < 1 or (W > 1 and t.stride(2) != ld) or (H > 1 and t.stride(1) != W * ld) or (B > 1 and t.stride(0) != H * W * ld):
        raise ValueError(f"{who}: {what} strides {t.stride()} are not [H*W*ld, W*ld, ld] with ld >= 1")
    return t, ld


def detail_coeffs(guide, target, radius, eps, out=None, arena=None):
    """The guided filter's coefficients at model resolution (shm_detail_coeffs, include/shmgan_hip.h, states the arithmetic): guide I
    (the standardised Y the generator was fed) and target p (gen_Y), float32 device planes [B,H,W] or [B,H,W,1] of one shape, each with a
    pixel pitch of its own; radius in 0..DETAIL_MAX_RADIUS (0: the plain residual, coef = (0, p - I)), eps > 0.  Returns `out`, a
    contiguous float32 [B,H,W,2] device tensor -- the arena's "detail/coef" when an arena is given, a new tensor otherwise -- filled
    asynchronously on the current stream."""
    g, ldg = _detail_plane(guide, "detail_coeffs", "guide")
    t, ldt = _detail_plane(target, "detail_coeffs", "target")
    if g.shape != t.shape or g.device != t.device:
        raise ValueError(f"detail_coeffs: guide {tuple(g.shape)} on {g.device} and target {tuple(t.shape)} on {t.device} differ")
    radius = int(radius)
    if not 0 <= radius <= DETAIL_MAX_RADIUS:
        raise ValueError(f"detail_coeffs: radius {radius} outside [0, {DETAIL_MAX_RADIUS}]")
    if not (eps > 0 and math.isfinite(eps)):
        raise ValueError(f"detail_coeffs: eps {eps!r} is not a positive finite number")
    B, H, W = (int(v) for v in g.shape)
    if out is None:
        out = arena.get("detail/coef", (B, H, W, 2)) if arena is not None else torch.empty((B, H, W, 2), dtype=torch.float32, device=g.device)
    elif out.dtype != torch.float32 or tuple(out.shape) != (B, H, W, 2) or not out.is_contiguous() or out.device != g.device:
        raise ValueError(f"detail_coeffs: out must be a contiguous float32 [{B},{H},{W},2] tensor on {g.device}")
    check(lib().shm_detail_coeffs(_p(g), ldg, _p(t), ldt, _p(out), B, H, W, radius, float(eps), _stream()), "shm_detail_coeffs")
    return out


def detail_apply_u8(photo_u8, coef, scale, out=None):
    """The coefficients of ONE image applied to its photo (shm_detail_apply_u8): photo_u8 contiguous uint8 [h,w,3] on the device, any
    size; coef contiguous float32 [H,W,2] (one image of detail_coeffs' result); scale a float32 device tensor of one element, that image's
    standardisation scale (a slice of preprocess's scale: no host copy is made).  Returns `out`, contiguous float32 [h,w,3] (allocated
    when not given): the full-resolution counterpart of gen_rgb, in its units, filled asynchronously on the current stream."""
    if photo_u8.dtype != torch.uint8 or not photo_u8.is_cuda or photo_u8.dim() != 3 or photo_u8.shape[2] != 3 or not photo_u8.is_contiguous() \
            or min(photo_u8.shape) < 1:
        raise ValueError(f"detail_apply_u8 takes a contiguous uint8 [h,w,3] device photo, got {photo_u8.dtype} {tuple(photo_u8.shape)} on "
                         f"{photo_u8.device}")
    dev = photo_u8.device
    if coef.dtype != torch.float32 or coef.device != dev or coef.dim() != 3 or coef.shape[2] != 2 or not coef.is_contiguous() or min(coef.shape) < 1:
        raise ValueError(f"detail_apply_u8 takes contiguous float32 [H,W,2] coefficients on {dev}, got {coef.dtype} {tuple(coef.shape)} on {coef.device}")
    if scale.dtype != torch.float32 or scale.device != dev or scale.numel() != 1:
        raise ValueError(f"detail_apply_u8 takes the image's scale as a float32 tensor of one element on {dev}, got {scale.dtype} "
                         f"{tuple(scale.shape)} on {scale.device}")
    h, w = int(photo_u8.shape[0]), int(photo_u8.shape[1])
    if out is None:
        out = torch.empty((h, w, 3), dtype=torch.float32, device=dev)
    elif out.dtype != torch.float32 or tuple(out.shape) != (h, w, 3) or not out.is_contiguous() or out.device != dev:
        raise ValueError(f"detail_apply_u8: out must be a contiguous float32 [{h},{w},3] tensor on {dev}")
    check(lib().shm_detail_apply_u8(_p(photo_u8), h, w, _p(coef), int(coef.shape[0]), int(coef.shape[1]), _p(scale), _p(out), _stream()),
          "shm_detail_apply_u8")
    return out


# ---- polarimetry: estimated-diffuse target and Stokes maps ----------------------------------------
POLAR_MODES = {"min": CONSTANTS["SHM_POLAR_MIN"], "stokes": CONSTANTS["SHM_POLAR_STOKES"]}


def _u8_images(srcs, who, noun, dims, which):
    """`who`'s check of its uint8 device images of one size: contiguous `dims` (say "[h,w,3]") `noun` ("views" / "images")."""
    for s in srcs:
        if s.dtype != torch.uint8 or not s.is_cuda:
            raise TypeError(f"{who} takes uint8 device {noun}, got {s.dtype} on {s.device}")
        if s.dim() != 3 or s.shape[2] != 3 or not s.is_contiguous():
            raise ValueError(f"{who} takes contiguous {dims} {noun}, got {tuple(s.shape)} with strides {s.stride()}")
    if any(s.shape != srcs[0].shape for s in srcs):
        raise ValueError(f"{who}: {which} differ in size: {[tuple(s.shape[:2]) for s in srcs]}")


def _f32_planes(dsts, who, device):
    """`who`'s check of its five contiguous float32 [ho,wo,3] destination planes on `device`."""
    for d in dsts:
        if d.dtype != torch.float32 or d.device != device:
            raise TypeError(f"{who} writes float32 planes on {device}, got {d.dtype} on {d.device}")
        if d.dim() != 3 or d.shape[2] != 3 or not d.is_contiguous():
            raise ValueError(f"{who} writes contiguous [ho,wo,3] planes, got {tuple(d.shape)} with strides {d.stride()}")
    if any(d.shape != dsts[0].shape for d in dsts):
        raise ValueError(f"{who}: the five planes differ in size: {[tuple(d.shape[:2]) for d in dsts]}")


def _mat4(mix, who):
    """None, or a 4x4 matrix (anything numpy takes, or a host tensor) as the C ABI's host float[16]."""
    import ctypes as C
    import numpy as np
    if mix is None:
        return None
    m = np.asarray(mix.cpu() if isinstance(mix, torch.Tensor) else mix, dtype=np.float32)
    if m.shape != (4, 4):
        raise ValueError(f"{who}: mix must be a 4x4 matrix, got shape {m.shape}")
    return (C.c_float * 16)(*[float(v) for v in m.reshape(-1)])


def _polar_coef(coef, who):
    """A 3x4 Stokes matrix (anything numpy takes: nested lists, an array, a host tensor) as the C ABI's host float[12]."""
    import ctypes as C
    import numpy as np
    a = np.asarray(coef.cpu() if isinstance(coef, torch.Tensor) else coef, dtype=np.float32)
    if a.size != 12 or a.shape not in ((3, 4), (12,)):
        raise ValueError(f"{who}: coef must be a 3x4 matrix, got shape {a.shape}")
    return (C.c_float * 12)(*[float(v) for v in a.reshape(-1)])


def polar_views_u8(srcs, dsts, mode="min", coef=None, scale=1.0 / 255.0, flip_ud=False):
    """The four decoded views of one sample -> its five training planes in one launch (shm_polar_views_u8, include/shmgan_hip.h,
    states the definitions).  srcs: four uint8 [hin,win,3] device tensors of the same size; dsts: five float32 [ho,wo,3] device
    tensors, views 0..3 and the estimated diffuse.  mode "min" (the reference's per-channel minimum) or "stokes" (coef = the 3x4
    matrix of polar.stokes_matrix).  Runs asynchronously on the current stream."""
    import ctypes as C
    if len(srcs) != 4 or len(dsts) != 5:
        raise ValueError(f"polar_views_u8 takes 4 source views and 5 destination planes, got {len(srcs)} and {len(dsts)}")
    if mode not in POLAR_MODES:
        raise ValueError(f"polar_views_u8: mode {mode!r} is not 'min' or 'stokes'")
    if mode == "stokes" and coef is None:
        raise ValueError("polar_views_u8: mode 'stokes' needs coef (polar.stokes_matrix of the polariser angles)")
    _u8_images(srcs, "polar_views_u8", "views", "[hin,win,3]", "the four views")
    _f32_planes(dsts, "polar_views_u8", srcs[0].device)
    hin, win, _ = srcs[0].shape
    ho, wo, _ = dsts[0].shape
    sp = (C.c_void_p * 4)(*[s.data_ptr() for s in srcs])
    dp = (C.c_void_p * 5)(*[d.data_ptr() for d in dsts])
    cf = _polar_coef(coef, "polar_views_u8") if mode == "stokes" else None
    check(lib().shm_polar_views_u8(sp, hin, win, cf, POLAR_MODES[mode], dp, ho, wo, scale, int(flip_ud), _stream()),
          "shm_polar_views_u8")


AUGMENT_MODES = dict(POLAR_MODES, dir=CONSTANTS["SHM_AUG_DIR"])


def augment_views_u8(srcs, dsts, mode="dir", coef=None, mix=None, crop=None, flip_ud=False, flip_lr=False, scale=1.0 / 255.0):
    """The decoded images of one sample -> its five training planes, cropped, mirrored and re-mixed in the launch that resizes them
    (shm_augment_views_u8, include/shmgan_hip.h, states the definitions).  srcs: uint8 [hin,win,3] device tensors of one size, five
    for mode "dir" (plane 4 is the fifth resampled), four for "min" / "stokes" (plane 4 is the estimate of polar_views_u8, coef as
    there); dsts: five float32 [ho,wo,3] device tensors.  mix: None or a 4x4 matrix (polar.mirror_views) applied to the four view
    bytes of every tap.  crop: (y, x, h, w) in source pixels, floats, None for the whole image.  Runs asynchronously on the current
    stream."""
    import ctypes as C
    if mode not in AUGMENT_MODES:
        raise ValueError(f"augment_views_u8: mode {mode!r} is not 'dir', 'min' or 'stokes'")
    nsrc = 5 if mode == "dir" else 4
    if len(srcs) != nsrc or len(dsts) != 5:
        raise ValueError(f"augment_views_u8 takes {nsrc} sources for mode {mode!r} and 5 destination planes, got {len(srcs)} and {len(dsts)}")
    if mode == "stokes" and coef is None:
        raise ValueError("augment_views_u8: mode 'stokes' needs coef (polar.stokes_matrix of the polariser angles)")
    _u8_images(srcs, "augment_views_u8", "images", "[hin,win,3]", "the sources")
    _f32_planes(dsts, "augment_views_u8", srcs[0].device)
    hin, win, _ = srcs[0].shape
    ho, wo, _ = dsts[0].shape
    mx = _mat4(mix, "augment_views_u8")
    cy, cx, ch, cw = (0.0, 0.0, float(hin), float(win)) if crop is None else (float(v) for v in crop)
    sp = (C.c_void_p * nsrc)(*[s.data_ptr() for s in srcs])
    dp = (C.c_void_p * 5)(*[d.data_ptr() for d in dsts])
    cf = _polar_coef(coef, "augment_views_u8") if mode == "stokes" else None
    check(lib().shm_augment_views_u8(sp, nsrc, hin, win, AUGMENT_MODES[mode], cf, mx, cy, cx, ch, cw, int(bool(flip_ud)), int(bool(flip_lr)),
                                     dp, ho, wo, scale, _stream()), "shm_augment_views_u8")


AUG_GROUP = CONSTANTS["SHM_AUG_GROUP"]                    # samples per launch of augment_batch_u8


@functools.lru_cache(maxsize=None)
def _aug_sample_struct():
    """ctypes mirror of shm_aug_sample (include/shmgan_hip.h)."""
    import ctypes as C

    class ShmAugSample(C.Structure):
        _fields_ = [("src", C.c_void_p * 5), ("hin", C.c_int), ("win", C.c_int), ("crop_y", C.c_float), ("crop_x", C.c_float),
                    ("crop_h", C.c_float), ("crop_w", C.c_float), ("flip_ud", C.c_int), ("flip_lr", C.c_int), ("mix", C.c_int),
                    ("plane", C.c_int * 4)]
    return ShmAugSample


def augment_batch_u8(samples, dsts, mode="dir", coef=None, mix=None, scale=1.0 / 255.0):
    """augment_views_u8 for a whole batch in one launch per AUG_GROUP samples (shm_augment_batch_u8, include/shmgan_hip.h, states the
    definitions): sample i of `samples` is written to dsts[p][i].  samples: a sequence of cache.AugSample (or anything with its
    fields): srcs are five ("dir") or four uint8 [hin,win,3] device tensors of the sample's own size, or their device addresses (the
    loader's arena) with hin / win given; crop (y, x, h, w) or None; flip_ud, flip_lr; mix: apply the shared 4x4 `mix` to this sample;
    planes: the destination plane of view 0..3.  dsts: five float32 [n,ho,wo,3] device tensors, n >= len(samples).  The C entry point
    checks every sample before it launches anything and names the sample it refuses.  Runs asynchronously on the current stream."""
    import ctypes as C
    if mode not in AUGMENT_MODES:
        raise ValueError(f"augment_batch_u8: mode {mode!r} is not 'dir', 'min' or 'stokes'")
    nsrc = 5 if mode == "dir" else 4
    if len(dsts) != 5:
        raise ValueError(f"augment_batch_u8 takes 5 destination tensors, got {len(dsts)}")
    if mode == "stokes" and coef is None:
        raise ValueError("augment_batch_u8: mode 'stokes' needs coef (polar.stokes_matrix of the polariser angles)")
    for d in dsts:
        if d.dtype != torch.float32 or not d.is_cuda or d.device != dsts[0].device:
            raise TypeError(f"augment_batch_u8 writes float32 device tensors on one device, got {d.dtype} on {d.device}")
        if d.dim() != 4 or d.shape[3] != 3 or not d[0].is_contiguous() or d.shape != dsts[0].shape or d.stride(0) != dsts[0].stride(0):
            raise ValueError(f"augment_batch_u8 writes five [n,ho,wo,3] tensors of one shape with contiguous samples, got {tuple(d.shape)} "
                             f"with strides {d.stride()}")
    nmax, ho, wo, _ = dsts[0].shape
    if len(samples) > nmax:
        raise ValueError(f"augment_batch_u8: {len(samples)} samples for destination tensors of {nmax}")
    arr = (_aug_sample_struct() * max(len(samples), 1))()
    for i, s in enumerate(samples):
        if len(s.srcs) != nsrc or len(s.planes) != 4:
            raise ValueError(f"augment_batch_u8: sample {i} has {len(s.srcs)} sources and {len(s.planes)} planes; mode {mode!r} takes {nsrc} and 4")
        hin, win = int(s.hin), int(s.win)
        for v, t in enumerate(s.srcs):
            if isinstance(t, torch.Tensor):
                if t.dtype != torch.uint8 or t.device != dsts[0].device:
                    raise TypeError(f"augment_batch_u8 takes uint8 images on {dsts[0].device}, got {t.dtype} on {t.device} (sample {i})")
                if tuple(t.shape) != (hin, win, 3) or not t.is_contiguous():
                    raise ValueError(f"augment_batch_u8: source {v} of sample {i} is not a contiguous [{hin},{win},3] image: "
                                     f"{tuple(t.shape)} with strides {t.stride()}")
                arr[i].src[v] = t.data_ptr()
            else:
                arr[i].src[v] = int(t) or None
        arr[i].hin, arr[i].win = hin, win
        arr[i].crop_y, arr[i].crop_x, arr[i].crop_h, arr[i].crop_w = (0.0, 0.0, float(hin), float(win)) if s.crop is None else (float(c) for c in s.crop)
        arr[i].flip_ud, arr[i].flip_lr, arr[i].mix = int(bool(s.flip_ud)), int(bool(s.flip_lr)), int(bool(s.mix))
        for v in range(4):
            arr[i].plane[v] = int(s.planes[v])
    mx = _mat4(mix, "augment_batch_u8")
    dp = (C.c_void_p * 5)(*[d.data_ptr() for d in dsts])
    cf = _polar_coef(coef, "augment_batch_u8") if mode == "stokes" else None
    check(lib().shm_augment_batch_u8(arr, len(samples), nsrc, AUGMENT_MODES[mode], cf, mx, dp, dsts[0].stride(0), ho, wo, scale, _stream()),
          "shm_augment_batch_u8")


@functools.lru_cache(maxsize=None)
def _pair_sample_struct():
    """ctypes mirror of shm_pair_sample (include/shmgan_hip.h)."""
    import ctypes as C

    class ShmPairSample(C.Structure):
        _fields_ = [("image", C.c_void_p), ("mask", C.c_void_p), ("hin", C.c_int), ("win", C.c_int), ("crop_y", C.c_float),
                    ("crop_x", C.c_float), ("crop_h", C.c_float), ("crop_w", C.c_float), ("flip_ud", C.c_int), ("flip_lr", C.c_int)]
    return ShmPairSample


def augment_pairs_ws_doubles(n, ho, wo):
    """float64 elements of augment_pairs_u8's workspace for n samples of ho x wo."""
    return int(lib().shm_augment_pairs_ws_doubles(int(n), int(ho), int(wo)))


def augment_pairs_u8(samples, x, y, ws=None, scale_out=None):
    """A batch of decoded (image, mask) pairs -> SpecSeg.train_step's two tensors in one call (shm_augment_pairs_u8,
    include/shmgan_hip.h, states the definitions): sample i of `samples` is written to x[i], the standardised Y plane of its cropped,
    mirrored and resized image, and y[i], its mask resampled the same way, in [0,1].  samples: a sequence of cache.AugSample (or
    anything with its fields) whose srcs are (image, mask): a uint8 [hin,win,3] and a uint8 [hin,win] (or [hin,win,1]) device tensor of
    the sample's own size, or their device addresses with hin / win given; crop (y, x, h, w) or None; flip_ud, flip_lr.  x, y: float32
    [n,ho,wo,1] device tensors of one shape, n >= len(samples).  ws: float64 device workspace of augment_pairs_ws_doubles elements
    (allocated when None; no initial value needed).  scale_out: None or float32 [n], receives every sample's max(std, 1/256).  The C
    entry point checks every sample before it launches anything and names the sample it refuses.  Runs asynchronously on the current
    stream."""
    for t in (x, y):
        if t.dtype != torch.float32 or not t.is_cuda or t.device != x.device:
            raise TypeError(f"augment_pairs_u8 writes float32 device tensors on one device, got {t.dtype} on {t.device}")
        if t.dim() != 4 or t.shape[3] != 1 or not t[0].is_contiguous() or t.shape != x.shape or t.stride(0) != x.stride(0):
            raise ValueError(f"augment_pairs_u8 writes two [n,ho,wo,1] tensors of one shape with contiguous samples, got {tuple(t.shape)} "
                             f"with strides {t.stride()}")
    nmax, ho, wo, _ = x.shape
    n = len(samples)
    if n > nmax:
        raise ValueError(f"augment_pairs_u8: {n} samples for destination tensors of {nmax}")
    arr = (_pair_sample_struct() * max(n, 1))()
    for i, s in enumerate(samples):
        if len(s.srcs) != 2:
            raise ValueError(f"augment_pairs_u8: sample {i} has {len(s.srcs)} sources; a pair is (image, mask)")
        hin, win = int(s.hin), int(s.win)
        ptrs = []
        for t, c in zip(s.srcs, (3, 1)):
            if isinstance(t, torch.Tensor):
                if t.dtype != torch.uint8 or t.device != x.device:
                    raise TypeError(f"augment_pairs_u8 takes uint8 images on {x.device}, got {t.dtype} on {t.device} (sample {i})")
                if tuple(t.shape) not in (((hin, win, c),) if c == 3 else ((hin, win, 1), (hin, win))) or not t.is_contiguous():
                    raise ValueError(f"augment_pairs_u8: the {'image' if c == 3 else 'mask'} of sample {i} is not a contiguous "
                                     f"[{hin},{win},{c}] tensor: {tuple(t.shape)} with strides {t.stride()}")
                ptrs.append(t.data_ptr())
            else:
                ptrs.append(int(t) or None)
        arr[i].image, arr[i].mask = ptrs
        arr[i].hin, arr[i].win = hin, win
        arr[i].crop_y, arr[i].crop_x, arr[i].crop_h, arr[i].crop_w = (0.0, 0.0, float(hin), float(win)) if s.crop is None else (float(c) for c in s.crop)
        arr[i].flip_ud, arr[i].flip_lr = int(bool(s.flip_ud)), int(bool(s.flip_lr))
    need = augment_pairs_ws_doubles(max(n, 1), ho, wo)
    if ws is None:
        ws = torch.empty(max(need, 1), dtype=torch.float64, device=x.device)
    elif ws.dtype != torch.float64 or ws.device != x.device or not ws.is_contiguous() or ws.numel() < need:
        raise ValueError(f"augment_pairs_u8: ws must be a contiguous float64 tensor of at least {need} elements on {x.device}, got "
                         f"{ws.dtype} {tuple(ws.shape)} on {ws.device}")
    if scale_out is not None and (scale_out.dtype != torch.float32 or scale_out.device != x.device or not scale_out.is_contiguous()
                                  or scale_out.numel() < n):
        raise ValueError(f"augment_pairs_u8: scale_out must be a contiguous float32 tensor of at least {n} elements on {x.device}")
    check(lib().shm_augment_pairs_u8(arr, n, _p(x), _p(y), x.stride(0), ho, wo, _p(ws), _p(scale_out), _stream()),
          "shm_augment_pairs_u8")


def polar_maps(views, coef, want=("s0", "dop", "aolp")):
    """Stokes maps of four float32 device views of equal element count (shm_polar_maps): with (S0, S1, S2) = coef . views,
    "s0" = S0, "dop" = sqrt(S1^2 + S2^2) / S0 (0 where S0 == 0), "aolp" = 0.5 atan2(S2, S1).  Returns {name: tensor of views[0]'s
    shape} for the names in `want`, filled asynchronously on the current stream."""
    import ctypes as C
    if len(views) != 4:
        raise ValueError(f"polar_maps takes 4 views, got {len(views)}")
    bad = [w for w in want if w not in ("s0", "dop", "aolp")]
    if bad or not want:
        raise ValueError(f"polar_maps: want {tuple(want)!r} must name some of 's0', 'dop', 'aolp'")
    for v in views:
        if v.dtype != torch.float32 or not v.is_cuda or v.device != views[0].device:
            raise TypeError(f"polar_maps takes float32 views on one device, got {v.dtype} on {v.device}")
        if not v.is_contiguous():
            raise ValueError(f"polar_maps takes contiguous views, got strides {v.stride()} for shape {tuple(v.shape)}")
    n = int(views[0].numel())
    if n == 0 or any(int(v.numel()) != n for v in views):
        raise ValueError(f"polar_maps: the four views must hold the same, non-zero number of elements: {[int(v.numel()) for v in views]}")
    cf = _polar_coef(coef, "polar_maps")
    out = {w: torch.empty_like(views[0]) for w in want}
    vp = (C.c_void_p * 4)(*[v.data_ptr() for v in views])
    check(lib().shm_polar_maps(vp, n, cf, _p(out.get("s0")), _p(out.get("dop")), _p(out.get("aolp")), _stream()), "shm_polar_maps")
    return out


# ---- polariser-mosaic (DoFP) sensors: one raw frame -> the four views (dofp.hip) -----------------------------
DOFP_PATTERNS = {n: CONSTANTS["SHM_DOFP_" + n.upper()] for n in ("mono", "rggb", "bggr", "grbg", "gbrg")}
DOFP_MODES = {"bilinear": CONSTANTS["SHM_DOFP_BILINEAR"], "bin": CONSTANTS["SHM_DOFP_BIN"]}


def dofp_period(pattern):
    """The mosaic's period P: 2 for "mono", 4 for the Bayer patterns."""
    if pattern not in DOFP_PATTERNS:
        raise ValueError(f"dofp: pattern {pattern!r} is not one of {tuple(DOFP_PATTERNS)}")
    return 2 if pattern == "mono" else 4


def dofp_shape(h, w, pattern, mode):
    """(ho, wo) of the views shm_dofp_views makes of an [h,w] mosaic: the mosaic's size for "bilinear", (h // P, w // P) for "bin"."""
    if mode not in DOFP_MODES:
        raise ValueError(f"dofp: mode {mode!r} is not one of {tuple(DOFP_MODES)}")
    P = dofp_period(pattern)
    return (int(h), int(w)) if mode == "bilinear" else (int(h) // P, int(w) // P)


def _dofp_check_mosaic(who, mosaic, bits):
    """What every mosaic entry point refuses about its frame, by `who`; returns bits as an int."""
    if not isinstance(mosaic, torch.Tensor) or not mosaic.is_cuda or mosaic.dtype not in (torch.uint8, torch.uint16):
        raise TypeError(f"{who} takes a uint8 or uint16 device tensor, got {getattr(mosaic, 'dtype', type(mosaic))} on "
                        f"{getattr(mosaic, 'device', 'the host')}")
    if mosaic.dim() != 2 or (mosaic.shape[1] > 1 and mosaic.stride(1) != 1):
        raise ValueError(f"{who} takes a 2-D mosaic with unit stride along a row, got {tuple(mosaic.shape)} with strides {mosaic.stride()}")
    if (mosaic.dtype == torch.uint8) != (int(bits) == 8):
        raise ValueError(f"{who}: a {mosaic.dtype} mosaic does not hold {bits}-bit samples (uint8 is bits = 8, uint16 is bits 9..16)")
    return int(bits)


_DOFP_CALIBRATIONS = {}          # (calibration, device) -> (dark uint16 [h,w] | None, gain uint16 [h,w] | None, defect uint8 [h,w] | None) on the device


def _dofp_calibration_tables(cal, device):
    """The tables of a polar.DofpCalibration on `device`: uploaded once, kept (the calibration's equality and hash go by its contents)."""
    key = (cal, torch.device(device))
    if key not in _DOFP_CALIBRATIONS:
        _DOFP_CALIBRATIONS[key] = tuple(None if a is None else torch.from_numpy(a.copy()).to(device) for a in (cal.dark, cal.gain, cal.defect))
    return _DOFP_CALIBRATIONS[key]


def _dofp_calibrated(who, mosaic, cal):
    """shm_dofp_calibrate of a checked mosaic into a new contiguous tensor, on the current stream."""
    h, w = (int(d) for d in mosaic.shape)
    if cal.shape is not None and (h, w) != cal.shape:
        raise ValueError(f"{who}: the mosaic is {h} x {w}, the calibration tables are {cal.shape[0]} x {cal.shape[1]}")
    if h < cal.period or w < cal.period:
        raise ValueError(f"{who}: a {h} x {w} mosaic is smaller than one period of pattern {cal.pattern!r}")
    dark, gain, defect = _dofp_calibration_tables(cal, mosaic.device)
    out = torch.empty((h, w), dtype=mosaic.dtype, device=mosaic.device)
    check(lib().shm_dofp_calibrate(mosaic.data_ptr(), cal.bits, h, w, int(mosaic.stride(0)) if h > 1 else w, DOFP_PATTERNS[cal.pattern],
                                   _p(dark), _p(gain), _p(defect), cal.pedestal, cal.white_level, out.data_ptr(), w, _stream()),
          "shm_dofp_calibrate")
    return out


def dofp_calibrate(mosaic, calibration):
    """One polariser-mosaic frame corrected by its sensor's calibration (shm_dofp_calibrate, include/shmgan_hip.h, states the arithmetic):
    dark frame removed around the pedestal, flat-field gain applied, defective photosites replaced by the rounded mean of their good
    same-lattice neighbours; saturated samples pass through.  mosaic: as dofp_views takes it.  calibration: a polar.DofpCalibration, or a
    polar.DofpLayout that carries one.  Returns a new contiguous tensor of the mosaic's dtype and size; the mosaic is not written.
    dofp_views and dofp_wb_gray make this call themselves for a layout with a calibration.  Asynchronous on the current stream."""
    cal = getattr(calibration, "calibration", calibration)
    if cal is None or not all(hasattr(cal, k) for k in ("dark", "gain", "defect", "pedestal", "white_level")):
        raise ValueError(f"dofp_calibrate takes a polar.DofpCalibration or a polar.DofpLayout that has one, got {calibration!r}")
    _dofp_check_mosaic("dofp_calibrate", mosaic, cal.bits)
    return _dofp_calibrated("dofp_calibrate", mosaic, cal)


DOFP_MERGE_MAX, DOFP_MERGE_TABLE = CONSTANTS["SHM_DOFP_MERGE_MAX"], CONSTANTS["SHM_DOFP_MERGE_TABLE"]
_DOFP_MERGE_TABLES = {}          # (exposures, bits, device) -> (mul uint32 [DOFP_MERGE_TABLE] on the device, its host mirror as a ctypes array)


def _dofp_merge_table(bracket, bits, device):
    """bracket.table(bits) on `device`: uploaded once, kept."""
    import ctypes as C
    key = (bracket.exposures, int(bits), torch.device(device))
    if key not in _DOFP_MERGE_TABLES:
        mul = bracket.table(bits)
        _DOFP_MERGE_TABLES[key] = (torch.from_numpy(mul.copy()).to(device), (C.c_uint * DOFP_MERGE_TABLE)(*[int(v) for v in mul]))
    return _DOFP_MERGE_TABLES[key]


def _dofp_pages(who, pages, n, bits):
    """The n checked 2-D pages of a bracket, of one size, dtype, device and pitch."""
    if isinstance(pages, torch.Tensor):
        if pages.dim() != 3:
            raise ValueError(f"{who} takes the pages as one [n,h,w] tensor or a list of 2-D tensors, got shape {tuple(pages.shape)}")
        pages = list(pages.unbind(0))
    pages = list(pages)
    if len(pages) != n:
        raise ValueError(f"{who}: {len(pages)} page(s) for a bracket of {n} exposures")
    for p in pages:
        _dofp_check_mosaic(who, p, bits)
    first = pages[0]
    h, w = (int(d) for d in first.shape)
    pitch = lambda p: int(p.stride(0)) if h > 1 else w
    for k, p in enumerate(pages):
        if tuple(p.shape) != (h, w) or p.dtype != first.dtype or p.device != first.device:
            raise ValueError(f"{who}: page {k} is {tuple(p.shape)} {p.dtype} on {p.device}, page 0 is {(h, w)} {first.dtype} on {first.device}")
        if pitch(p) != pitch(first):
            raise ValueError(f"{who}: page {k} has a row pitch of {pitch(p)} elements, page 0 of {pitch(first)}: the pages share one pitch")
    return pages, h, w, pitch(first)


def _dofp_merged(who, pages, bracket, bits, black, white, counts=False, calibration=None):
    """shm_dofp_merge of the checked pages (each through shm_dofp_calibrate first when there is a calibration) into a new contiguous uint16
    tensor, on the current stream: (merged, counts tensor or None)."""
    import ctypes as C
    pages, h, w, pitch = _dofp_pages(who, pages, bracket.pages, bits)
    if calibration is not None:
        pages, pitch = [_dofp_calibrated(who, p, calibration) for p in pages], w
    table, mirror = _dofp_merge_table(bracket, bits, pages[0].device)
    out = torch.empty((h, w), dtype=torch.uint16, device=pages[0].device)
    cnt = torch.empty(DOFP_MERGE_MAX + 1, dtype=torch.int32, device=pages[0].device) if counts else None
    sp = (C.c_void_p * len(pages))(*[p.data_ptr() for p in pages])
    check(lib().shm_dofp_merge(sp, len(pages), bits, h, w, pitch, table.data_ptr(), mirror, black, white, out.data_ptr(), w, _p(cnt), _stream()),
          "shm_dofp_merge")
    return out, cnt


def dofp_merge(pages, bracket_or_layout, counts=False, bits=None):
    """The pages of one exposure bracket merged into one uint16 [h,w] mosaic on the scale of the shortest exposure (shm_dofp_merge,
    include/shmgan_hip.h, states the arithmetic): every unsaturated page votes, weighted by its exposure time.  pages: a [n,h,w] device
    tensor or a list of n 2-D ones with unit stride along a row and one row pitch, uint8 (bits = 8) or uint16.  bracket_or_layout: a
    polar.DofpLayout with a bracket -- its bits, its levels (layout.bracket_levels), and its calibration applied to every page first --
    or a polar.DofpBracket alone, with `bits` (default 8 for uint8 pages, 16 for uint16) and the bracket's own levels (0 and 2^bits - 1
    where it gives none).  With `counts` also an int32 [9] device tensor: counts[j] = the photosites with exactly j valid pages.  The
    table goes to the device once per (bracket, bits, device).  Asynchronous on the current stream: nothing waits for the device."""
    bracket = getattr(bracket_or_layout, "bracket", None)
    if bracket is not None:
        layout = bracket_or_layout
        if bits is not None and int(bits) != layout.bits:
            raise ValueError(f"dofp_merge: bits {bits!r} is not the layout's {layout.bits}")
        black, white = layout.bracket_levels
        out, cnt = _dofp_merged("dofp_merge", pages, bracket, layout.bits, black, white, counts, layout.calibration)
    else:
        bracket = bracket_or_layout
        if not all(hasattr(bracket, k) for k in ("exposures", "table", "levels")):
            raise ValueError(f"dofp_merge takes a polar.DofpBracket or a polar.DofpLayout that has one, got {bracket_or_layout!r}")
        if bits is None:
            first = pages[0] if len(pages) else None
            bits = 8 if getattr(first, "dtype", None) == torch.uint8 else 16
        black, white = bracket.levels(int(bits))
        out, cnt = _dofp_merged("dofp_merge", pages, bracket, int(bits), black, white, counts)
    return (out, cnt) if counts else out


def _dofp_merge_layout(who, pages, layout):
    """The merged mosaic of a bracketed layout's pages: what dofp_views and dofp_wb_gray then read under layout.merged."""
    black, white = layout.bracket_levels
    return _dofp_merged(who, pages, layout.bracket, int(layout.bits), black, white, False, layout.calibration)[0]


def dofp_views(mosaic, layout, mode="bilinear", total=False):
    """One polariser-mosaic frame -> its four views in one launch (shm_dofp_views, include/shmgan_hip.h, states the arithmetic).
    mosaic: a uint8 or uint16 2-D device tensor with unit stride along a row; its stride 0 is the pitch.  layout: a
    polar.DofpLayout (anything with .pattern, .quad and .bits); a uint8 mosaic needs bits == 8, a uint16 one bits 9..16.  Returns
    four new uint8 [ho,wo,3] tensors in ascending polariser angle, and with `total` a fifth: the rounded mean of the four.
    With layout.develop (a polar.DofpDevelop) the planes are developed instead -- black level, white balance, matrix, tone curve, in
    the same single launch (shm_dofp_develop), after the two grey-world launches when its wb is "gray".  With layout.calibration (a
    polar.DofpCalibration) the frame is corrected first (dofp_calibrate, one more launch into a new tensor) and all of that reads the
    corrected mosaic.  With layout.bracket (a polar.DofpBracket) `mosaic` is the [n,h,w] pages of one sample: each is corrected, they are
    merged (dofp_merge, one more launch) and the views are those of the merged 16-bit mosaic under layout.merged.  Asynchronous on the
    current stream."""
    import ctypes as C
    if getattr(layout, "bracket", None) is not None:
        return dofp_views(_dofp_merge_layout("dofp_views", mosaic, layout), layout.merged, mode, total)
    bits = _dofp_check_mosaic("dofp_views", mosaic, layout.bits)
    h, w = (int(d) for d in mosaic.shape)
    ho, wo = dofp_shape(h, w, layout.pattern, mode)
    if ho < 1 or wo < 1:
        raise ValueError(f"dofp_views: a {h} x {w} mosaic is smaller than one period of pattern {layout.pattern!r}")
    out = torch.empty((5 if total else 4, ho, wo, 3), dtype=torch.uint8, device=mosaic.device)
    quad = (C.c_int * 4)(*[int(q) for q in layout.quad])
    dp = (C.c_void_p * 4)(*[out[v].data_ptr() for v in range(4)])
    if getattr(layout, "calibration", None) is not None:          # everything below reads the corrected mosaic
        mosaic = _dofp_calibrated("dofp_views", mosaic, layout.calibration)
    pitch = int(mosaic.stride(0)) if h > 1 else w
    develop = getattr(layout, "develop", None)
    if develop is None:
        check(lib().shm_dofp_views(mosaic.data_ptr(), bits, h, w, pitch, DOFP_PATTERNS[layout.pattern], quad, DOFP_MODES[mode], dp,
                                   out[4].data_ptr() if total else None, _stream()), "shm_dofp_views")
        return tuple(out[v] for v in range(out.shape[0]))
    # developed views (shm_dofp_develop): the tables are on the device already; with wb "gray" the frame's own gains are estimated into a
    # parameter block of this call's, which the development reads on the same stream -- nothing here waits for the device
    params, lut, mirror = _dofp_tables(layout, mosaic.device)
    if develop.wb == "gray":
        params = _dofp_wb_gray(mosaic, layout, develop.saturation(layout), params)[1]
    check(lib().shm_dofp_develop(mosaic.data_ptr(), bits, h, w, pitch, DOFP_PATTERNS[layout.pattern], quad, DOFP_MODES[mode], dp,
                                 out[4].data_ptr() if total else None, params.data_ptr(), lut.data_ptr(), mirror, _stream()), "shm_dofp_develop")
    return tuple(out[v] for v in range(out.shape[0]))


DOFP_PARAMS, DOFP_WB_WS = CONSTANTS["SHM_DOFP_PARAMS"], CONSTANTS["SHM_DOFP_WB_WS"]
_DOFP_TABLES = {}          # (layout, device) -> (params int32 [DOFP_PARAMS], lut uint8 [4096]) on the device and the host mirror as a ctypes array


def _dofp_tables(layout, device):
    """The development tables of `layout` (layout.develop.table(layout)) on `device`: uploaded once, kept."""
    import ctypes as C
    key = (layout, torch.device(device))
    if key not in _DOFP_TABLES:
        params, lut, mirror = layout.develop.table(layout)
        _DOFP_TABLES[key] = (torch.from_numpy(params.copy()).to(device), torch.from_numpy(lut.copy()).to(device),
                             (C.c_int * DOFP_PARAMS)(*[int(v) for v in mirror]))
    return _DOFP_TABLES[key]


def _dofp_wb_gray(mosaic, layout, sat, params):
    """shm_dofp_wb_gray on the current stream: (ws int64 [DOFP_WB_WS], params_out int32 [DOFP_PARAMS]), both new."""
    h, w = (int(d) for d in mosaic.shape)
    ws = torch.empty(DOFP_WB_WS, dtype=torch.int64, device=mosaic.device)
    params_out = torch.empty(DOFP_PARAMS, dtype=torch.int32, device=mosaic.device)
    check(lib().shm_dofp_wb_gray(mosaic.data_ptr(), int(layout.bits), h, w, int(mosaic.stride(0)) if h > 1 else w, DOFP_PATTERNS[layout.pattern],
                                 params.data_ptr(), int(sat), params_out.data_ptr(), ws.data_ptr(), _stream()), "shm_dofp_wb_gray")
    return ws, params_out


def dofp_wb_gray(mosaic, layout, sat=None):
    """Grey-world sums and gains of one Bayer polariser-mosaic frame (shm_dofp_wb_gray, include/shmgan_hip.h): (sums int64 [6] = S_r, S_g,
    S_b, n_r, n_g, n_b over the complete 4 x 4 periods without a sample at or above `sat`, gains int64 [3] in Q10), device tensors filled
    asynchronously on the current stream.  The black level is layout.develop's (0 without one); `sat` defaults to its saturation count, or
    2^bits - 1 without one.  A layout with a calibration has the frame corrected first, as dofp_views does; one with a bracket takes the
    [n,h,w] pages, merges them and sums the merged mosaic under layout.merged (a `sat` given here is in counts of one page, like the
    development's, and is moved onto the merged scale)."""
    if getattr(layout, "bracket", None) is not None:
        if dofp_period(layout.pattern) != 4:
            raise ValueError(f"dofp_wb_gray needs a Bayer pattern, the layout is {layout.pattern!r}")
        sat = None if sat is None else min(65536, int(sat) << (16 - int(layout.bits)))
        return dofp_wb_gray(_dofp_merge_layout("dofp_wb_gray", mosaic, layout), layout.merged, sat)
    _dofp_check_mosaic("dofp_wb_gray", mosaic, layout.bits)
    if dofp_period(layout.pattern) != 4:
        raise ValueError(f"dofp_wb_gray needs a Bayer pattern, the layout is {layout.pattern!r}")
    if getattr(layout, "calibration", None) is not None:
        mosaic = _dofp_calibrated("dofp_wb_gray", mosaic, layout.calibration)
    develop = getattr(layout, "develop", None)
    if develop is None:
        params = torch.zeros(DOFP_PARAMS, dtype=torch.int32, device=mosaic.device)
        sat = (1 << int(layout.bits)) - 1 if sat is None else sat
    else:
        params = _dofp_tables(layout, mosaic.device)[0]
        sat = develop.saturation(layout) if sat is None else sat
    ws = _dofp_wb_gray(mosaic, layout, sat, params)[0]
    return ws[:6], ws[6:9]


# ---- specular masks from the polarised views (specmask.hip) -------------------------------------------
SPECMASK_MAX_OPEN, SPECMASK_MAX_DILATE = CONSTANTS["SHM_SPECMASK_MAX_OPEN"], CONSTANTS["SHM_SPECMASK_MAX_DILATE"]


def _specmask_map(t, who, what, like=None):
    if t.dtype != torch.uint8 or not t.is_cuda or t.dim() != 2 or not t.is_contiguous():
        raise ValueError(f"{who}: {what} must be a contiguous uint8 [h,w] device tensor, got {t.dtype} {tuple(t.shape)} with strides {t.stride()} on {t.device}")
    if like is not None and (t.shape != like.shape or t.device != like.device):
        raise ValueError(f"{who}: {what} is {tuple(t.shape)} on {t.device}, expected {tuple(like.shape)} on {like.device}")


def _specmask_ints(t, who, what, n):
    if t.dtype != torch.int32 or not t.is_cuda or t.dim() != 1 or t.shape[0] != n or not t.is_contiguous():
        raise ValueError(f"{who}: {what} must be a contiguous int32 [{n}] device tensor, got {t.dtype} {tuple(t.shape)} on {t.device}")


def _specmask_views(srcs, q, who):
    """The checks of the four source views and the map of their size; returns (host pointer array, h, w)."""
    import ctypes as C
    if len(srcs) != 4:
        raise ValueError(f"{who} takes 4 source views, got {len(srcs)}")
    _u8_images(srcs, who, "views", "[h,w,3]", "the four views")
    if any(s.device != srcs[0].device for s in srcs):
        raise ValueError(f"{who}: the four views differ in size: {[tuple(s.shape[:2]) for s in srcs]}")
    h, w, _ = srcs[0].shape
    _specmask_map(q, who, "q")
    if tuple(q.shape) != (h, w) or q.device != srcs[0].device:
        raise ValueError(f"{who}: q is {tuple(q.shape)} on {q.device}, the views are {h}x{w} on {srcs[0].device}")
    return (C.c_void_p * 4)(*[s.data_ptr() for s in srcs]), h, w


def specmask_strength(srcs, coef, q, hist):
    """Polarised-intensity byte map and its histogram of one sample (shm_specmask_strength, include/shmgan_hip.h): srcs = four
    contiguous uint8 [h,w,3] device views of one size, coef = the 3x4 Stokes matrix, q = uint8 [h,w], hist = int32 [256] (cleared by
    the call, whatever it held).  Asynchronous on the current stream."""
    sp, h, w = _specmask_views(srcs, q, "specmask_strength")
    _specmask_ints(hist, "specmask_strength", "hist", 256)
    check(lib().shm_specmask_strength(sp, h, w, _polar_coef(coef, "specmask_strength"), _p(q), _p(hist), _stream()), "shm_specmask_strength")


def specmask(srcs, coef, q, hist, tmp, mask, stats, floor=16, fixed=None, open_radius=1, dilate_radius=2):
    """The chain specmask_strength -> specmask_otsu -> specmask_morph in one call (shm_specmask): every argument is checked before the
    first launch.  q, hist, mask and stats are results, tmp is scratch.  Asynchronous; nothing is read back."""
    sp, h, w = _specmask_views(srcs, q, "specmask")
    _specmask_map(tmp, "specmask", "tmp", q)
    _specmask_map(mask, "specmask", "mask", q)
    _specmask_ints(hist, "specmask", "hist", 256)
    _specmask_ints(stats, "specmask", "stats", 3)
    check(lib().shm_specmask(sp, h, w, _polar_coef(coef, "specmask"), int(floor), -1 if fixed is None else int(fixed), int(open_radius),
                             int(dilate_radius), _p(q), _p(hist), _p(tmp), _p(mask), _p(stats), _stream()), "shm_specmask")


def specmask_otsu(hist, stats, floor=16, fixed=None):
    """Otsu's threshold of hist (int32 [256] on the device) into stats (int32 [3]: t, t_eff, count): t_eff = max(t, floor), or
    `fixed` (an integer in [0, 255]) when given (shm_specmask_otsu).  Asynchronous; nothing is read back."""
    _specmask_ints(hist, "specmask_otsu", "hist", 256)
    _specmask_ints(stats, "specmask_otsu", "stats", 3)
    check(lib().shm_specmask_otsu(_p(hist), int(floor), -1 if fixed is None else int(fixed), _p(stats), _stream()), "shm_specmask_otsu")


def specmask_morph(q, stats, tmp, mask, open_radius=1, dilate_radius=2):
    """mask (uint8 [h,w], 0 / 255) = dilate(open(q > stats[1], open_radius), dilate_radius) with square elements and out-of-image taps
    skipped; stats[2] = the number of set pixels (shm_specmask_morph).  tmp: uint8 [h,w] scratch of its own.  Asynchronous."""
    _specmask_map(q, "specmask_morph", "q")
    _specmask_map(tmp, "specmask_morph", "tmp", q)
    _specmask_map(mask, "specmask_morph", "mask", q)
    _specmask_ints(stats, "specmask_morph", "stats", 3)
    h, w = q.shape
    check(lib().shm_specmask_morph(_p(q), h, w, int(open_radius), int(dilate_radius), _p(tmp), _p(mask), _p(stats), _stream()),
          "shm_specmask_morph")


# ---- first-layer input gradient, summed over input channels -----------------------------------------
def sum_input_channels(w, cin, cout, mask, weff):
    check(lib().shm_sum_input_channels(_p(w), cin, cout, mask, _p(weff), _stream()), "shm_sum_input_channels")


def conv3x3_dgrad_sum1(dz, lddz, weff, out, nk, batch, hi, wi, c, stride, accumulate):
    check(lib().shm_conv3x3_dgrad_sum1(_p(dz), lddz, _p(weff), _p(out), nk, batch, hi, wi, c, stride, int(accumulate),
                                       _dt(dz), _stream()), "shm_conv3x3_dgrad_sum1")
