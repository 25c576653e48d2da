"""The convolution, InstanceNorm, pooling and elementwise kernels on tensors of 2 GiB to 8 GiB (far_ref.py has the method, the windows and
the table; test_far_cpu.py shows on a 16-bit model that the layouts, bands and checks catch the address faults they are built for).

Every case is a case of test_pitch_gpu.py -- same runners, same cached operands and float64 references, same bounds -- with ONE pitch argument
far and every other tensor tight, so each far call is compared two ways: against float64 at the bound the runner applies, and against the
tight call of the same values in the class (BITWISE / ATOMIC / BWD) test_pitch_gpu.py assigns to the quantity.

  * inputs and aux at W4- (byte offsets with bit 31 set, the last pixel within one pitch of the 0xfffffff0 limit), the first input at W2 too;
  * outputs at W4- (buffer stores above 2 GiB), at the first refused-for-inputs extent and at W4+ (the real 4 GiB path): the kernel and the bits
    are those of the tight call under "tapgemm.flat_epilogue" = 1, and no weights-in-registers or ping-pong kernel is chosen;
  * an aux one quantum too wide for 32-bit offsets: the sums come from the reduce pass;
  * inputs one quantum too wide: refused with "operand larger than 4 GiB", shm_last_kernel() unchanged, every output parent still the sentinel
    (the parent has the full refused size, so a launch that slipped through would be caught here and not by a fault);
  * the InstanceNorm and pooling entry points at E31 (fp32 and bf16: past 2^31 elements, fp32 also past 4 GiB) and E32 (bf16) on three
    samples, and at E31 on one sample (the in-image term p * ld crosses too); in bf16 also at B31 / B32, where sample 2 STARTS past the threshold
    (the batch term n * hw * ld crosses on its own; in fp32 that layout and its band pass 20 GiB);
  * the pitched heads, shm_lrelu_bwd and SpecSeg passes of test_heads_edges_gpu.py at E31 (bf16 forms: E32 too), on its references and bounds;
  * shm_conv2d_transpose2x2_fwd (a tap GEMM) in the convolutions' windows; shm_mask_pool_pack_hw with a far destination pitch (all of it output);
  * shm_zero, shm_cast_f32, shm_mul_mask (bf16, and fp32 in place) on 2^31 + 4 * 1027 elements;
  * the compact RGB first layer on real images of 2 GiB, on both sides of its 0x7fffff00 switch, checked on strips of rows;
  * shm_load_pad_u8, shm_mask_pool_pack_hw, shm_image_metrics_hw and shm_export_u8_hw on frames of 32768 x 32 and 32 x 32768, 32769 refused.

One far parent at a time, carved from one arena of the largest case's size (16.9 GiB) that the module frees at its end; a case's results are
host copies of its slices before the next case fills the arena again.
"""
import gc

import numpy as np
import pytest
import torch

import far_ref as F
import pitch_ref as R
import test_pitch_gpu as P
from shmgan_amd._lib import ShmError
from util import SENTINEL, host, rel_l2

pytestmark = pytest.mark.gpu

GIB = 1 << 30
PEAK = {"bytes": 0, "cases": 0}


@pytest.fixture(autouse=True)
def _reset_tuning(request):
    torch.cuda.reset_peak_memory_stats()
    yield
    P._ops().set_tuning("reset", 0)
    _release()
    peak = torch.cuda.max_memory_allocated()
    PEAK["bytes"] = max(PEAK["bytes"], peak)
    if peak > 18 * GIB:
        print(f"\n{request.node.name}: peak device memory {peak / GIB:.2f} GiB")
    assert peak <= 20 * GIB, (request.node.name, peak)          # the module's memory condition, measured per test


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    F.drop_arena()
    torch.cuda.empty_cache()
    print(f"\nfar cases run: {PEAK['cases']}; largest peak of device memory allocated in one test {PEAK['bytes'] / GIB:.2f} GiB")


def _release(collect=False):
    P.Alloc.last = None
    if collect:          # (a refusal's traceback holds the runner's frame, and with it the parents)
        gc.collect()


def _table_bytes():
    conv = max(F.case_bytes(f, dt, c) for f, _v, dt, _k in F.conv_table() for _i, c, _kind in F.conv_cases(f, dt))
    inn = max(F.case_bytes(f2, dt, c) for f, dt, _k in F.in_table() for _i, f2, c in F.in_cases(f, dt))
    return max(conv, inn, F.lim() + (3 << 30))


ARENA_BYTES = _table_bytes() + (64 << 20)          # the largest far parent of the tables (16.9 GiB: a pooled fp32 tensor at E31 behind a band of its own extent)


def _need(nbytes, arena=True):
    """Skip only when the device cannot hold the case: its parents plus 2.5 GiB of scan temporaries and tight tensors (2.4 GiB measured), plus 4 GiB.  The pitched cases
    carve their far parent from one arena of the tables' largest size (far_ref.arena); the flat elementwise cases hold their own tensors instead."""
    _release()
    need = (ARENA_BYTES if arena else nbytes) + 5 * GIB // 2
    assert nbytes <= ARENA_BYTES or not arena
    assert need <= 20 * GIB, need
    have = F._ARENA.get("cuda")
    if arena and have is not None and have.numel() >= ARENA_BYTES:
        return
    F.drop_arena()
    torch.cuda.empty_cache()
    free, total = torch.cuda.mem_get_info()
    if free < need + 4 * GIB:
        pytest.skip(f"needs {need / GIB:.1f} GiB + 4 GiB, {free / GIB:.1f} of {total / GIB:.1f} GiB free")
    if arena:
        F.arena(ARENA_BYTES, "cuda")


def _compare(res, base, fam):
    """a far call against the tight call of the same kernel: the classes of test_pitch_gpu.py"""
    for f in P.BITWISE:
        if base.get(f) is not None:
            assert torch.equal(res[f], base[f]), (f, "not bit-equal to the tight run", float((res[f].double() - base[f].double()).abs().max()))
    for f in P.ATOMIC:
        if base.get(f) is not None:
            assert P._same_f64(res[f], base[f]), (f, "beyond 1e-12 of the tight run")
    for f in P.BWD:
        if base.get(f) is None:
            continue
        if "fused" in base["kern"]:
            assert torch.equal(res[f], base[f]), (f, "not bit-equal to the tight run")
        else:
            r = rel_l2(host(res[f].float() if f == "dz" else res[f]), host(base[f].float() if f == "dz" else base[f]))
            assert r < 1e-5, (f, "against the tight run", r)


def _ids(fam, *more):
    sid = "-".join(str(fam["shape"][k]) for k in sorted(fam["shape"]))
    return "/".join(str(x) for x in (fam["name"], sid) + more if x and x != "-")


def _kid(kn):
    return ",".join(f"{k.split('.')[-1]}={v}" for k, v in kn.items())


def _written(A):
    """output parents of a refused call that do not hold their fill EVERYWHERE, the slice included: no launch happened"""
    return [arg for arg, parent, shape, pld, off, fill, lead in A.watch
            if not (R.outside_untouched(parent, shape[:-1] + (0,), pld, 0, None, fill) if lead is None
                    else F.far_outside_untouched(parent, shape[:-1] + (0,), pld, 0, lead, fill))]


# ===================================================================================================================== convolutions
CONV = [pytest.param(f, v, dt, kn, id=_ids(f, v, dt, _kid(kn))) for f, v, dt, kn in F.conv_table()]
FLAT = {"tapgemm.flat_epilogue": 1}


def _far_kernel(fam, case, tight_kern):
    """shm_last_kernel() of a far call below 4 GiB: the tight call's -- far pitches are multiples of 16 bytes on aligned bases, so no term of
    pitch_ref's predicates moves -- but for the thin-input weight gradient, which packs pixels of exactly 16 floats (wgrad_thin_pitch)."""
    if fam["entry"] == "conv2d_wgrad" and "thin" in tight_kern and "ldx" in case:
        return "wgrad_halo_kernel"
    return tight_kern


@pytest.mark.parametrize("fam,variant,dt,knobs", CONV)
def test_far_convolution_operands(fam, variant, dt, knobs):
    run, check = P.RUN[fam["entry"]]
    cases = F.conv_cases(fam, dt)
    _need(max(F.case_bytes(fam, dt, c) for _, c, _ in cases))
    P._set(variant, knobs)
    tight = run(fam, dt, {})
    check(fam, dt, tight)
    named = R.tight_kernel(fam, variant, dt, knobs)
    assert named is None or tight["kern"] == named, (tight["kern"], named)
    print(f"tight: {tight['kern']}")
    # the tight call as an output of 4 GiB or more runs it (a forced weights-in-registers variant is an error there: the automatic choice)
    vflat = "auto" if variant == "wreg" else variant
    flat, failed = None, []
    for cid, case, kind in cases:
        _release()
        if kind == "flat" and flat is None:
            P._set(vflat, dict(knobs, **FLAT))
            try:
                flat = run(fam, dt, {})
                check(fam, dt, flat)
                print(f"tight, flat epilogue: {flat['kern']}")
            except ShmError as e:
                # sources normalised on the fly, fp32, the automatic choice: without the weights-in-registers kernel these few blocks go to a DMA
                # tile, which cannot normalise -- the launcher says so and launches nothing.  The far call has to give the same answer.
                assert fam["shape"].get("norm") and "cannot normalise its source" in str(e), str(e)
                flat = {"refused": "cannot normalise its source"}
                print(f"tight, flat epilogue: refused ({flat['refused']})")
        base = tight if kind in ("same", "aux") else flat
        P._set(variant if kind in ("same", "aux") else vflat, knobs)
        PEAK["cases"] += 1
        if "refused" in base:
            try:
                run(fam, dt, case)
                failed.append((cid, "not refused like the tight call under the knob"))
            except ShmError as e:
                torch.cuda.synchronize()
                if base["refused"] not in str(e) or _written(P.Alloc.last):
                    failed.append((cid, str(e)[:200], _written(P.Alloc.last)))
                print(f"{cid}: {case} refused like the tight call")
            _release(True)
            continue
        res = run(fam, dt, case)
        try:
            assert not res["touched"], ("written outside the slice", res["touched"])
            assert res.get("scratch_zero", True), "scratch not zero on return"
            figs = check(fam, dt, res)
            if kind == "same":
                assert res["kern"] == _far_kernel(fam, case, tight["kern"]), ("kernel", res["kern"], tight["kern"])
            elif kind == "flat":
                assert res["kern"] == flat["kern"], ("kernel", res["kern"], flat["kern"])
                assert "wreg" not in res["kern"] and "tapgemm_pp_" not in res["kern"], ("kernel", res["kern"])
                if "halo" in res["kern"]:
                    assert not res["kern"].endswith(", true>"), ("gsum epilogue on an output of 4 GiB", res["kern"])
            else:          # an aux beyond 32-bit offsets: no gsum epilogue reads it (the DMA tiles keep their name; the sums are held to float64 by check)
                assert not res["kern"].endswith(", true>"), ("gsum epilogue on an aux of 4 GiB", res["kern"])
            if res["kern"] == base["kern"] and kind != "aux":
                _compare(res, base, fam)
            print(f"{cid}: {case} {res['kern']} {figs}")
        except AssertionError as e:
            failed.append((cid, res["kern"], str(e)[:300]))
            print(f"{cid}: FAILED {res['kern']} {str(e)[:300]}")
        del res
    assert not failed, failed


REFUSE = [p for p in CONV if p.values[1] == F.CONV_VARIANTS.get(p.values[0]["name"], p.values[0]["variants"][:1])[0]
          and p.values[3] == R.knob_sets(p.values[0])[0]]


@pytest.mark.parametrize("fam,variant,dt,knobs", REFUSE)
def test_operands_of_the_limit_are_refused_before_any_launch(fam, variant, dt, knobs):
    ops = P._ops()
    run, _ = P.RUN[fam["entry"]]
    roles = R.ENTRY_POINTS[fam["entry"]]
    esz, q = R.ESZ[dt], R.Q[dt]
    failed = []
    for a in roles["in"]:
        if a not in fam["ch"]:
            continue
        _release()
        c = next(iter(F.far_case(fam, dt, a, "W4-").values()))
        ld = c.ld + q
        assert F.npix_of(fam, a) * ld * esz >= F.lim() > F.npix_of(fam, a) * c.ld * esz
        _need((F.lim() + (3 << 30)))
        P._set(variant, knobs)
        run(fam, dt, {})          # the tight call in front, so that "unchanged" is not "still empty"
        _release()
        before = ops.last_kernel()
        try:
            run(fam, dt, {a: F.Far("W4-", ld)})
            failed.append((a, "not refused", ops.last_kernel()))
        except ShmError as e:
            torch.cuda.synchronize()
            A = P.Alloc.last
            if "operand larger than 4 GiB" not in str(e):
                failed.append((a, "another error", str(e)[:200]))
            if ops.last_kernel() != before:
                failed.append((a, "shm_last_kernel() changed", ops.last_kernel()))
            if _written(A):
                failed.append((a, "output written", _written(A)))
            del A
        _release(True)
        PEAK["cases"] += 1
    assert not failed, failed


# ============================================================================================== InstanceNorm, pooling (E31 / E32)
INS = [pytest.param(f, dt, kn, id=_ids(f, dt, _kid(kn))) for f, dt, kn in F.in_table()]


def _in_kernel(fam, dt, case, tight_kern):
    """shm_last_kernel() of a far shm_in_bwd call: the tight call's, but that the g-held one-pass kernel addresses a sample through one buffer
    descriptor and 32-bit byte offsets -- a sample of 4 GiB or more (the one-sample cases) takes the two passes ("elem.fused_hold" = 2 allows no
    other one-pass kernel)."""
    (arg, far), = case.items()
    if "fusedg" in tight_kern and arg != "ldg2":
        sh = fam["shape"]
        if sh["h"] * sh["w"] * far.ld * 2 >= F.lim():
            return R.R8
    return tight_kern


@pytest.mark.parametrize("fam,dt,knobs", INS)
def test_far_instnorm_and_pooling(fam, dt, knobs):
    cases = F.in_cases(fam, dt)
    _need(max(F.case_bytes(f, dt, c) for _, f, c in cases))
    tights, failed = {}, []
    for cid, f, case in cases:
        _release()
        n = f["shape"]["n"]
        if n not in tights:
            P._set("-", knobs)
            tights[n] = P._run_in(f, dt, {})
            P._check_in(f, dt, tights[n])
            assert not tights[n]["touched"] and tights[n].get("scratch_zero", True)
            if n == 3:
                named = R.tight_kernel(f, "-", dt, knobs) if f["name"].startswith("in_bwd-one-pass") else None
                assert named is None or tights[n]["kern"] == named, (tights[n]["kern"], named)
        tight = tights[n]
        P._set("-", knobs)
        res = P._run_in(f, dt, case)
        PEAK["cases"] += 1
        try:
            assert not res["touched"], ("written outside the slice", res["touched"])
            assert res.get("scratch_zero", True), "scratch not zero on return"
            want = _in_kernel(f, dt, case, tight["kern"])
            assert res["kern"] == want, ("kernel", res["kern"], want)
            figs = P._check_in(f, dt, res)
            if res["kern"] == tight["kern"]:
                _compare(res, tight, f)
            print(f"{cid}: {case} {res['kern']} {figs}")
        except AssertionError as e:
            failed.append((cid, res["kern"], str(e)[:300]))
            print(f"{cid}: FAILED {res['kern']} {str(e)[:300]}")
        del res
    assert not failed, failed


# ================================================================================================ the no-pitch elementwise kernels
NEL = (1 << 31) + 4 * 1027
GUARD = 4096
CMP = 1 << 26          # elements per comparison on the device (its temporaries are float32)
FILL = 1 << 25         # elements per pattern chunk (its temporaries are int64)
WINDOWS = ((0, 4096), ((1 << 30) - 2048, (1 << 30) + 2048), ((1 << 31) - 2048, (1 << 31) + 2048), (NEL - 4 * 1027 - 64, NEL))


def _pattern(lo, hi):
    """exactly representable in bf16, with a period (251) that divides no power of two: an index that lost a high bit reads another value"""
    i = np.arange(lo, hi, dtype=np.int64)
    return ((i % 251) - 125).astype(np.float32) / 4.0


def _fill_pattern(t, n):
    """t[:n] = pattern, in chunks built on the device from 64-bit indices"""
    for lo in range(0, n, FILL):
        hi = min(n, lo + FILL)
        i = torch.arange(lo, hi, dtype=torch.int64, device="cuda")
        t[lo:hi] = (((i % 251) - 125).to(torch.float32) / 4.0).to(t.dtype)
        del i


def _windows_equal(t, fn):
    for lo, hi in WINDOWS:
        got = t[lo:hi].float().cpu().numpy()
        want = fn(_pattern(lo, hi))
        assert np.array_equal(got, want), ("window", lo, hi, int(np.flatnonzero(got != want)[0]) + lo)


def _guard_ok(t, n, fill=SENTINEL):
    return bool((t[n:] == fill).all())


def _flat(dtype, fill):
    t = torch.empty(NEL + GUARD, dtype=dtype, device="cuda")
    for lo in range(0, NEL + GUARD, F.CHUNK):
        t[lo:lo + F.CHUNK].fill_(fill)
    return t


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_zero_and_cast_past_2_31_elements(dt):
    ops, adt = P._ops(), P._adt(dt)
    _need((NEL + GUARD) * (4 + R.ESZ[dt]), arena=False)
    src = _flat(torch.float32, SENTINEL)
    _fill_pattern(src, NEL)
    dst = _flat(adt, SENTINEL)
    ops.cast_f32(src, dst, NEL)
    torch.cuda.synchronize()
    _windows_equal(dst, lambda p: p)
    assert _guard_ok(dst, NEL) and _guard_ok(src, NEL)
    # every element, not only the windows: the cast of an exactly representable pattern is the pattern (compared in chunks on the device)
    for lo in range(0, NEL, CMP):
        assert bool((dst[lo:min(NEL, lo + CMP)].float() == src[lo:min(NEL, lo + CMP)]).all()), lo
    del src
    ops.zero(dst[:NEL])
    torch.cuda.synchronize()
    for lo in range(0, NEL, F.CHUNK):
        assert not bool(dst[lo:min(NEL, lo + F.CHUNK)].view(torch.int16 if dt == "bf16" else torch.int32).any()), lo
    assert _guard_ok(dst, NEL)
    PEAK["cases"] += 2


def test_mul_mask_past_2_31_elements():
    """bf16 activations under the fp32 mask: 4 + 8 + 4 GiB (the fp32 form of the same kernel template would hold 24 GiB)"""
    ops = P._ops()
    _need((NEL + GUARD) * (2 + 4 + 2), arena=False)
    x = _flat(torch.bfloat16, SENTINEL)
    _fill_pattern(x, NEL)
    m = _flat(torch.float32, SENTINEL)
    for lo in range(0, NEL, FILL):
        hi = min(NEL, lo + FILL)
        m[lo:hi] = (torch.arange(lo, hi, dtype=torch.int64, device="cuda") % 3 != 0).to(torch.float32)
    y = _flat(torch.bfloat16, SENTINEL)
    ops.mul_mask(x, m, y, NEL, 2.0)
    torch.cuda.synchronize()
    for lo, hi in WINDOWS:
        want = _pattern(lo, hi) * (np.arange(lo, hi) % 3 != 0) * 2.0
        got = y[lo:hi].float().cpu().numpy()
        assert np.array_equal(got, want), ("window", lo, hi)
    for lo in range(0, NEL, CMP):
        hi = min(NEL, lo + CMP)
        assert bool((y[lo:hi].float() == x[lo:hi].float() * m[lo:hi] * 2.0).all()), lo
    assert _guard_ok(y, NEL) and _guard_ok(x, NEL) and _guard_ok(m, NEL)
    PEAK["cases"] += 1


# ============================================================================ heads, LeakyReLU backward, SpecSeg passes (E31 / E32)
# The entry points of test_heads_edges_gpu.py that take a pitch, on its smallest multi-trip shapes, references and bounds (heads_edge_ref.py):
# the pitch under test far, every other tensor as that module allocates it (guarded, NaN gaps).  Results are also compared bit for bit with the
# tight call's where the kernel adds in a fixed order.
import heads_edge_ref as E          # noqa: E402
import test_heads_edges_gpu as H    # noqa: E402
from util import dev                # noqa: E402


class _Far1:
    """one far pixel list [rows, c] in the arena: NaN around an input, the sentinel around an output"""

    def __init__(self, rows, c, window, dtype, vals=None):
        esz = torch.empty(0, dtype=dtype).element_size()
        self.shape, self.fill = (1, rows, c), P.NAN if vals is not None else SENTINEL
        self.ld = F.far_ld(window, rows, c, esz, 16 // esz)
        self.lead = F.lead_for(window, self.shape, self.ld, esz)
        self.v, self.parent = F.far_view(self.fill, self.shape, self.ld, 0, self.lead, F.trail_for(self.shape), dtype, "cuda", use_arena=True)
        if vals is not None:
            F.scatter(self.v, torch.from_numpy(np.ascontiguousarray(vals, dtype=np.float32)).to(dtype))

    def get(self):
        return F.gather(self.v)[0]

    def intact(self):
        return F.far_outside_untouched(self.parent, self.shape, self.ld, 0, self.lead, self.fill)


def _src(vals, c, dtype, far, window):
    """an input [rows, c]: (tensor, pitch, None) tight with the module's NaN gap, or far"""
    if far:
        f = _Far1(vals.shape[0], vals.shape[1], window, dtype, vals)
        return f.v, f.ld, f
    return H._wide(vals, c + 4, dtype), c + 4, None


def _dst(rows, c, dtype, far, window):
    """an output [rows, c]: (tensor, pitch, read(), intact())"""
    if far:
        f = _Far1(rows, c, window, dtype)
        return f.v, f.ld, f.get, f.intact
    raw, p = H._out(rows, c + 8, dtype)
    return p, c + 8, lambda: p[:, :c].contiguous().cpu(), lambda: H._intact(raw, p, c)


def _el_lrelu(dt, far, window):
    ops, c = P._ops(), 48
    npix = E.lrelu_npix(c, dt)[1]
    k = E.lrelu_case(c, npix, dt)
    dz, db = E.lrelu_bwd_ref(k.y, k.dy)
    out = {}
    for with_db in (True, False):
        dyd, lddy, _ = _src(k.dy, c, H.GRAD[dt], far == "lddy", window)
        yd, ldy, _ = _src(k.y, c, H.ACT[dt], far == "ldy", window)
        dzd, lddz, read, intact = _dst(npix, c, H.ACT[dt], far == "lddz", window)
        braw, dbd = H._acc(k.db0) if with_db else (None, None)
        rraw, red = H._acc(np.zeros(ops.LRELU_RED_SLOTS * c))
        ops.lrelu_bwd(dyd, lddy, yd, ldy, dzd, lddz, dbd, npix, c, E.SLOPE, red)
        torch.cuda.synchronize()
        got = read()
        assert intact() and E.guard_intact(rraw, red) and (not with_db or E.guard_intact(braw, dbd)), "a store behind dz, red or dbias"
        assert not bool(red.view(torch.int64).any().item()), "red is not zero on return"
        g64 = host(got.float())
        H._chk(f"lrelu_bwd {dt} {far} {window} dbias={with_db} dz", E.err(g64, dz), E.F32_TOL if dt == "f32" else E.BF16_TOL)
        assert E.lrelu_special_ok(g64, k, E.F32_TOL if dt == "f32" else E.BF16_TOL)
        if with_db:
            H._chk("  dbias increment", E.err(host(dbd)[:, 0] - k.db0, db), E.ftol(dt))
        out[f"dz{int(with_db)}"] = got
    return out


def _el_bn(dt, far, window):
    ops = P._ops()
    b, h, w, c = E.SPEC_PITCH_MAP
    npix = b * h * w
    k = E.bn_case(npix, c)
    a, lda, _ = _src(k.a, c, torch.float32, far == "lda", window)
    out, ldo, read, intact = _dst(npix, c, torch.float32, far == "ldo", window)
    ops.bn_apply(a, lda, dev(k.gamma), dev(k.beta), dev(k.mean), dev(k.var), E.BN_EPS, out, ldo, npix, c)
    torch.cuda.synchronize()
    got = read()
    assert intact()
    H._chk(f"bn_apply {far} {window}", E.err(host(got), E.bn_ref(k.a, k.gamma, k.beta, k.mean, k.var)), E.F32_TOL)
    return {"out": got}


def _el_maxpool(dt, far, window):
    ops = P._ops()
    b, h, w, c = E.SPEC_PITCH_MAP
    x = np.random.default_rng(97).standard_normal((b, h, w, c), dtype=np.float32)
    xd, ldx, _ = _src(x.reshape(-1, c), c, torch.float32, far == "ldx", window)
    y, ldy, read, intact = _dst(b * (h // 2) * (w // 2), c, torch.float32, far == "ldy", window)
    ops.maxpool2_fwd(xd, ldx, y, ldy, b, h, w, c)
    torch.cuda.synchronize()
    got = read()
    assert intact()
    assert np.array_equal(got.numpy(), E.maxpool_ref(x).reshape(-1, c)), "maxpool2_fwd: a selection is exact"
    return {"y": got}


def _el_head_fwd(dt, far, window, kind="lrelu", norm=False):
    ops, c = P._ops(), 64
    k = E.head_case(c, E.head_npix(c)[-1], dt, E.HEAD_IN_BATCH if norm else 1)
    rows = k.batch * k.npix
    xd, ldx, _ = _src(k.x, c, H.ACT[dt], True, window)
    raw, y = H._out(rows, 1)
    if kind == "sigmoid":
        ops.head_sigmoid_fwd(xd, ldx, dev(k.w), dev([k.b]), y, rows, c)
        ref = E.sigmoid_head_ref(k.x, k.w, k.b)
    elif norm:
        ops.head_in_fwd(xd, ldx, H._stats(k), dev(k.beta), dev(k.w), dev([k.b]), y, k.batch, k.npix, c, E.SLOPE)
        ref = E.head_fwd_ref(E.head_norm(k.x, k.mean, k.inv, k.beta), k.w, k.b)
    else:
        ops.head_fwd(xd, ldx, dev(k.w), dev([k.b]), y, rows, c, E.SLOPE)
        ref = E.head_fwd_ref(k.x, k.w, k.b)
    torch.cuda.synchronize()
    assert E.guard_intact(raw, y)
    H._chk(f"head_fwd {kind} norm={norm} {dt} {window}", E.err(host(y)[:, 0], ref), E.ftol(dt))
    return {}


def _el_head_bwd(dt, far, window):
    ops, c = P._ops(), 64
    k = E.head_case(c, E.head_npix(c)[-1], dt, 1)
    rows = k.npix
    y = E.r32(E.head_fwd_ref(k.x, k.w, k.b))
    dz, dx, dw, db = E.head_bwd_ref(k.x, k.w, y, k.dy)
    rng = np.random.default_rng(5)
    dw0, db0 = rng.standard_normal(c) * 3, rng.standard_normal(1) * 3
    (wraw, dwa), (braw, dba) = H._acc(dw0), H._acc(db0)
    rraw, red = H._acc(np.full(ops.LRELU_RED_SLOTS * (c + 1), P.NAN))
    xd, ldx, _ = _src(k.x, c, H.ACT[dt], far == "ldx", window)
    dxd, lddx, read, intact = _dst(rows, c, H.GRAD[dt], far == "lddx", window)
    ops.head_bwd(xd, ldx, dev(k.w), dev(y), dev(k.dy), dxd, lddx, dwa, dba, rows, c, E.SLOPE, red)
    torch.cuda.synchronize()
    got = read()
    assert intact() and E.guard_intact(wraw, dwa) and E.guard_intact(braw, dba) and E.guard_intact(rraw, red)
    H._chk(f"head_bwd {dt} {far} {window} dx", E.err(host(got.float()), dx), E.gtol(dt))
    H._chk("  dw_acc increment", E.err(host(dwa)[:, 0] - dw0, dw), E.ftol(dt))
    H._chk("  db_acc increment", E.err(host(dba)[:, 0] - db0, db), E.ftol(dt))
    return {"dx": got}


def _el_pack(dt, far, window):
    ops = P._ops()
    (ldsrc, c0), npix, nc, lddst = E.PACK_SRC, E.PACK_NPIX[0], 3, 16
    src = np.random.default_rng(98).standard_normal((npix, ldsrc), dtype=np.float32)
    sd, ld = (torch.from_numpy(src).cuda(), ldsrc)
    if far:
        f = _Far1(npix, ldsrc, window, torch.float32, src)
        sd, ld = f.v, f.ld
    raw, dst = H._out(npix, lddst)
    ops.pack_channels(sd, ld, c0, nc, dst, lddst, npix)
    torch.cuda.synchronize()
    assert E.guard_intact(raw, dst)
    assert np.array_equal(dst.cpu().numpy().view(np.int32), E.pack_ref(src, c0, nc, lddst).view(np.int32))
    return {}


def _el_head_in_bwd(dt, far, window):
    ops, c = P._ops(), 64
    k = E.head_case(c, E.head_npix(c)[-1], dt, E.HEAD_IN_BATCH)
    rows = k.batch * k.npix
    xh = E.head_norm(k.x, k.mean, k.inv, k.beta)
    y = E.r32(E.head_fwd_ref(xh, k.w, k.b))
    dz, dx, dw, db = E.head_bwd_ref(xh, k.w, y, k.dy)
    rng = np.random.default_rng(5)
    dw0, db0 = rng.standard_normal(c) * 3, rng.standard_normal(1) * 3
    (wraw, dwa), (braw, dba) = H._acc(dw0), H._acc(db0)
    rraw, red = H._acc(np.full(ops.LRELU_RED_SLOTS * (c + 1), P.NAN))
    xd, lda, _ = _src(k.x, c, H.ACT[dt], far == "lda", window)
    dxd, lddx, read, intact = _dst(rows, c, H.GRAD[dt], far == "lddx", window)
    zraw, dzo = H._out(rows, 1)
    ops.head_in_bwd(xd, lda, H._stats(k), dev(k.beta), dev(k.w), dev(y), dev(k.dy), dxd, lddx, dwa, dba, k.batch, k.npix, c, E.SLOPE, red, dz_out=dzo)
    torch.cuda.synchronize()
    got = read()
    assert intact() and E.guard_intact(zraw, dzo) and E.guard_intact(wraw, dwa) and E.guard_intact(braw, dba) and E.guard_intact(rraw, red)
    H._chk(f"head_in_bwd {dt} {far} {window} dz_out", E.err(host(dzo)[:, 0], dz), E.F32_TOL)
    H._chk("  dx", E.err(host(got.float()), dx), E.gtol(dt))
    H._chk("  dw_acc increment", E.err(host(dwa)[:, 0] - dw0, dw), E.ftol(dt))
    H._chk("  db_acc increment", E.err(host(dba)[:, 0] - db0, db), E.ftol(dt))
    return {"dx": got}


PATCH = (17, 2, 3, 68)          # more samples than the weight-gradient kernel's stride of 16, the second channel block ragged
assert PATCH in E.PATCH_CASES


def _el_patch(dt, far, window):
    ops = P._ops()
    k = E.patch_case(*PATCH, dt)
    n, h, w, c = PATCH
    npx = n * h * w
    xd, ldx, _ = _src(k.x.reshape(npx, c), c, H.ACT[dt], far == "ldx", window)
    yraw, y = H._out(npx, 1)
    ops.patch_fwd(xd, ldx, dev(k.wt), y, n, h, w, c, E.SLOPE)
    yref = E.patch_fwd_ref(k.x, k.wt)
    assert E.guard_intact(yraw, y)
    H._chk(f"patch_fwd {dt} {far} {window} y", E.err(host(y), yref), E.ftol(dt))
    yin = E.r32(yref)
    dz, dx, dw = E.patch_bwd_ref(k.x, k.wt, yin, k.dy)
    zraw, dzd = H._out(npx, 1)
    wraw, dwd = H._out(9, c)
    if far == "lddx":          # (one far tensor in the arena at a time: x goes back to its tight form)
        xd, ldx, _ = _src(k.x.reshape(npx, c), c, H.ACT[dt], False, window)
    dxd, lddx, read, intact = _dst(npx, c, H.GRAD[dt], far == "lddx", window)
    ops.patch_bwd(xd, ldx, dev(k.wt), dev(yin), dev(k.dy), dzd, dxd, lddx, dwd, n, h, w, c, E.SLOPE)
    torch.cuda.synchronize()
    got = read()
    assert intact() and E.guard_intact(zraw, dzd) and E.guard_intact(wraw, dwd)
    H._chk("  patch_bwd dz", E.err(host(dzd), dz), E.F32_TOL)
    H._chk("  dx", E.err(host(got.float()), dx.reshape(npx, c)), E.gtol(dt))
    H._chk("  dw", E.err(host(dwd), dw), E.ftol(dt))
    return {"dx": got, "y": y[:, :1].contiguous().cpu()}


BOTH_W = {"f32": ("E31",), "bf16": ("E31", "E32")}
ELEM = []
for _name, _fn, _args, _dts in (("lrelu_bwd", _el_lrelu, ("lddy", "ldy", "lddz"), ("f32", "bf16")), ("bn_apply", _el_bn, ("lda", "ldo"), ("f32",)),
                                ("maxpool2_fwd", _el_maxpool, ("ldx", "ldy"), ("f32",)), ("head_fwd", _el_head_fwd, ("ldx",), ("f32", "bf16")),
                                ("head_in_fwd", lambda dt, far, w: _el_head_fwd(dt, far, w, norm=True), ("lda",), ("f32", "bf16")),
                                ("head_sigmoid_fwd", lambda dt, far, w: _el_head_fwd(dt, far, w, kind="sigmoid"), ("ldx",), ("f32",)),
                                ("head_bwd", _el_head_bwd, ("ldx", "lddx"), ("f32", "bf16")),
                                ("head_in_bwd", _el_head_in_bwd, ("lda", "lddx"), ("f32", "bf16")), ("patch", _el_patch, ("ldx", "lddx"), ("f32", "bf16")),
                                ("pack_channels", _el_pack, ("ldsrc",), ("f32",))):
    for _dt in _dts:
        ELEM.append(pytest.param(_fn, _args, _dt, _name, id=f"{_name}/{_dt}"))


@pytest.mark.parametrize("fn,args,dt,ids", ELEM)
def test_far_heads_and_elementwise(fn, args, dt, ids):
    _need(ARENA_BYTES - (64 << 20))
    tight = fn(dt, None, None) if fn in (_el_lrelu, _el_bn, _el_maxpool, _el_head_bwd, _el_head_in_bwd, _el_patch) else {}
    batched = ids in ("head_in_fwd", "head_in_bwd", "patch")          # entry points with a batch term: bf16 also with sample 2 past the threshold
    for a in args:
        for window in BOTH_W[dt] + (("B31", "B32") if batched and dt == "bf16" and fn is not _el_patch else ()):
            res = fn(dt, a, window)
            PEAK["cases"] += 1
            for f, t in tight.items():
                assert torch.equal(res[f], t), (a, window, f, "not bit-equal to the tight call")
            print(f"{a}-{window}: passed")


# ============================================================================================== frame sides of the native path
# shm_load_pad_u8, shm_image_metrics_hw and shm_export_u8_hw take sides up to 32768 (evaluate.MAX_FRAME_SIDE) and say so in their errors;
# shm_mask_pool_pack_hw runs on the same frames.  Thin frames reach the limit with a megabyte of data: 32768 x 32 and 32 x 32768 (metrics: 16 wide,
# its float64 reference is the slow part), the photo off-centre in the frame, references native_ref.py / metrics_ref.py / export_ref.py.
import export_ref as xr             # noqa: E402
import native_ref as nr             # noqa: E402
from util import band_untouched     # noqa: E402

SIDE = 32768
THIN = [(SIDE, 32), (32, SIDE)]


def _swap(t, hp):
    """(a, b) for the long side first or second"""
    return t if hp == SIDE else t[::-1]


@pytest.mark.parametrize("hp,wp", THIN)
def test_load_pad_u8_at_the_side_limit(hp, wp):
    ops = P._ops()
    (h, w), (top, left) = _swap((SIDE - 5, 21), hp), _swap((1, 7), hp)          # centred would be (2, 5)
    u8 = np.random.default_rng(hp).integers(0, 256, (h, w, 3), dtype=np.uint8)
    ys, xs = nr.reflect_index(np.arange(hp) - top, h), nr.reflect_index(np.arange(wp) - left, w)
    want = u8[ys][:, xs].astype(np.float32) * np.float32(1.0 / 255.0)
    n = hp * wp * 3
    flat = torch.full((n + 16 * wp * 3,), SENTINEL, dtype=torch.float32, device="cuda")
    dst = flat[:n].view(hp, wp, 3)
    ops.load_pad_u8(torch.from_numpy(u8).cuda(), dst, top, left, 1.0 / 255.0)
    assert np.array_equal(dst.cpu().numpy().view(np.uint32), want.view(np.uint32))
    assert band_untouched(flat[n:])
    # one more row / column: refused with the documented error before any launch
    big = torch.full(_swap((SIDE + 1, 16), hp) + (1,), SENTINEL, device="cuda")
    with pytest.raises(ShmError, match=r"outside \[1, 32768\]"):
        ops.load_pad_u8(torch.zeros(_swap((SIDE - 8, 16), hp) + (1,), dtype=torch.uint8, device="cuda"), big, *_swap((4, 0), hp))
    torch.cuda.synchronize()
    assert band_untouched(big)


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("h,w", THIN)
def test_mask_pool_pack_hw_at_the_side_limit(h, w, dt):
    """(the entry point names no side limit of its own: there is no refusal to ask for)"""
    ops, k = P._ops(), 2
    ld = 64 // torch.empty((), dtype=dt).element_size()
    mask = np.random.default_rng(h).uniform(0, 1, (1, h, w, 1)).astype(np.float32)
    n = (h // k) * (w // k) * ld
    flat = torch.full((n + 16 * ld,), SENTINEL, dtype=dt, device="cuda")
    dst = flat[:n].view(1, h // k, w // k, ld)
    ops.mask_pool_pack_hw(dev(mask), dst, 1, h, w, k)
    want = torch.nn.functional.max_pool2d(torch.from_numpy(mask).permute(0, 3, 1, 2), k).permute(0, 2, 3, 1)
    assert torch.equal(dst[..., 0].float().cpu(), want[..., 0].to(dt).float())
    assert not dst[..., 1:].float().abs().max().item() and band_untouched(flat[n:])


@pytest.mark.parametrize("hp,wp", [(SIDE, 16), (16, SIDE)])
def test_image_metrics_hw_at_the_side_limit(hp, wp):
    ops = P._ops()
    (h, w), (top, left) = _swap((SIDE - 7, 12), hp), _swap((3, 1), hp)
    rng = np.random.default_rng(wp)
    pred = np.full((1, hp, wp, 3), np.nan, dtype=np.float32)          # nothing outside the window enters
    pred[:, top:top + h, left:left + w] = rng.uniform(-0.3, 1.3, (1, h, w, 3))
    target = rng.uniform(-0.3, 1.3, (1, h, w, 3)).astype(np.float32)
    got = host(ops.image_metrics_hw(dev(pred), (top, left, h, w), dev(target)))
    ref = np.asarray(nr.metrics_hw(pred, (top, left, h, w), target), np.float64)
    print("metrics", got, ref)
    # the tolerances of tests/test_metrics_gpu.py (test_native_gpu.py _check)
    assert np.all(np.abs(got[:, 0] - ref[:, 0]) <= 1e-5 * np.abs(ref[:, 0])) and np.all(np.abs(got[:, 1] - ref[:, 1]) <= 1e-4)
    assert np.all(np.abs(got[:, 2] - ref[:, 2]) <= 5e-5)
    for j in (3, 4):
        assert np.all(np.abs(got[:, j] - ref[:, j]) <= 1e-4 * np.abs(ref[:, j])), j
    out = torch.full((1, 5), SENTINEL, dtype=torch.float64, device="cuda")
    over = torch.zeros((1,) + _swap((SIDE + 1, 16), hp) + (3,), device="cuda")
    with pytest.raises(ShmError, match="outside"):
        ops.image_metrics_hw(over, (0, 0, 12, 12), torch.zeros((1, 12, 12, 3), device="cuda"), out=out)
    torch.cuda.synchronize()
    assert band_untouched(out)


@pytest.mark.parametrize("hp,wp", THIN)
def test_export_u8_hw_at_the_side_limit(hp, wp):
    """The window's own size with "clip" on byte values / 255 (every byte equals the float64 reference's), and a "rescale" job that doubles half of
    the long side up to the limit (bytes within 1e-3 of a rounding tie may differ by one: test_native_gpu.py's rule).  The header defines the
    sampling coordinate in fp32, fy = (oy + 0.5) * hc / ho - 0.5; at 32768 rows an fp32 coordinate is good to 4e-3 of a pixel, so export_ref.py's
    float64 coordinates are the same mapping only where the fp32 ones are exact: a ratio of 1/2 (fy = oy / 2 - 0.25).  (With 32761 -> 32768 rows,
    1.7 % of the bytes sat one off the float64 restatement: the definition's precision, not an index.)"""
    ops = P._ops()
    (h, w), (top, left) = _swap((SIDE - 7, 27), hp), _swap((3, 2), hp)
    rng = np.random.default_rng(hp + 1)
    x = rng.integers(0, 256, (hp, wp, 3)).astype(np.float32) * np.float32(1 / 255.0)
    x[rng.uniform(size=x.shape) < 0.05] = -0.3
    x[rng.uniform(size=x.shape) < 0.05] = 1.4
    win = (top, left, h, w)
    (y0, x0), (hc, wc) = _swap((SIDE // 2 - 4, 2), hp), _swap((SIDE // 2, 27), hp)          # the window ends four rows short of the plane's end
    win2, size2 = (y0, x0, hc, wc), _swap((SIDE, 27), hp)
    x2 = rng.uniform(-0.4, 1.4, (hp, wp, 3)).astype(np.float32)          # (continuous values: byte values under a 1/4 : 3/4 blend crowd the ties)
    out, offs = ops.export_u8_hw([dev(x), dev(x2)], [win, win2], [(h, w), size2], ["clip", "rescale"])
    o = out.cpu().numpy()
    g1 = o[offs[0]:offs[0] + h * w * 3].reshape(h, w, 3)
    g2 = o[offs[1]:offs[1] + size2[0] * size2[1] * 3].reshape(size2 + (3,))
    b1, y1 = nr.export_hw(x, win, h, w, "clip")
    assert not xr.near_half(y1).any() and np.array_equal(g1, b1)
    b2, y2 = nr.export_hw(x2, win2, *size2, "rescale")
    near, d = xr.near_half(y2), np.abs(g2.astype(np.int64) - b2.astype(np.int64))
    print(f"export {size2}: {int(near.sum())} of {near.size} bytes near a tie, {int((d != 0).sum())} differ ({int((d[~near] != 0).sum())} of them "
          f"away from a tie), largest difference {int(d.max())}")
    assert np.all(d[~near] == 0) and np.all(d <= 1) and near.sum() <= 0.01 * near.size
    with pytest.raises(ShmError, match="32768"):
        ops.export_u8_hw([dev(x)], [win], [_swap((SIDE + 1, 16), hp)], ["clip"])


# ================================================================================= SpecSeg's 2x2 transposed convolution, a tap GEMM
@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_far_conv2d_transpose2x2(dt):
    """shm_conv2d_transpose2x2_fwd goes through launch_tapgemm (four phases of one tap): its operands are bound by the convolutions' limit, so it runs
    in their windows, not at E31 -- ldx at W4-, ldy at W4-, at the limit and at W4+ (against the tight call under "tapgemm.flat_epilogue" = 1)."""
    ops = P._ops()
    n, h, cin, cout = 3, 8, 64, 32          # test_ops_gpu.py's three-sample case on an 8 x 8 map (on 4 x 4, byte 2^31 falls inside a pixel of the one
    #                                         W4- pitch: the straddle assertion refuses it)
    rng = np.random.default_rng(21)
    adt, esz, q = P._adt(dt), R.ESZ[dt], R.Q[dt]
    x = P._rnd(rng.standard_normal((n, h, h, cin)), dt)
    w = P._rnd(rng.standard_normal((2, 2, cout, cin)) * 0.1, dt)
    b = rng.standard_normal(cout).astype(np.float32)
    ref = P.nhwc(torch.nn.functional.conv_transpose2d(P.nchw(x), P.t64(w).permute(3, 2, 0, 1).contiguous(), stride=2)) + b
    _need(F.lim() + (3 << 30))
    wd, bd = torch.from_numpy(w.astype(np.float32)).cuda().to(adt), torch.from_numpy(b).cuda()

    def run(case, knobs):
        P._set("-", knobs)
        A = P.Alloc(case)
        xv, ldx = A.inp("ldx", x, adt)
        y, ldy = A.out("ldy", ref.shape, adt)
        ops.conv2d_transpose2x2_fwd(xv, ldx, wd, bd, y, ldy, n, h, h, cin, cout, 1.0)
        torch.cuda.synchronize()
        return ops.last_kernel(), P._cpu(y), A.untouched()

    tight, flat = run({}, {}), run({}, FLAT)
    assert rel_l2(host(tight[1].float()), ref) < P.RECT_TOL[dt] and rel_l2(host(flat[1].float()), ref) < P.RECT_TOL[dt]
    npx = {"ldx": n * h * h, "ldy": n * 4 * h * h}
    c = {"ldx": cin, "ldy": cout}
    cases = [("ldx", "W2", tight), ("ldx", "W4-", tight), ("ldy", "W4-", tight), ("ldy", "LIM", flat), ("ldy", "W4+", flat)]
    for a, win, base in cases:
        ld = F.far_ld("W4-", npx[a], c[a], esz, q) + q if win == "LIM" else F.far_ld(win, npx[a], c[a], esz, q)
        kern, got, touched = run({a: F.Far(win, ld)}, {})
        PEAK["cases"] += 1
        assert not touched, (a, win, touched)
        assert kern == base[0], (a, win, kern, base[0])
        assert rel_l2(host(got.float()), ref) < P.RECT_TOL[dt], (a, win)
        assert torch.equal(got, base[1]), (a, win, "not bit-equal to the tight call")
        print(f"{a}-{win}: ld {ld} {kern}")
    # an input one quantum over the limit is refused, the output untouched
    before = ops.last_kernel()
    with pytest.raises(ShmError, match="operand larger than 4 GiB"):
        run({"ldx": F.Far("W4-", F.far_ld("W4-", npx["ldx"], cin, esz, q) + q)}, {})
    torch.cuda.synchronize()
    assert ops.last_kernel() == before and not _written(P.Alloc.last)
    _release(True)


# ===================================================================================== mask_pool_pack_hw with a far destination pitch
@pytest.mark.parametrize("dt,window", [("f32", "E31"), ("bf16", "E31"), ("bf16", "E32")])
def test_far_mask_pool_pack_pitch(dt, window):
    """The entry point writes the pooled mask into channel 0 and ZERO into every other element of the pitch (`for c in 1 .. ld`: elem.hip), so a far
    `lddst` has no gap to guard: all of its 2^31 or 2^32 elements are output.  Checked in chunks on the device: channel 0 of every pixel, zero bits
    everywhere else, the bands untouched."""
    ops, k = P._ops(), 2
    adt, esz = P._adt(dt), R.ESZ[dt]
    B, H, W = 3, 32, 32
    npix = B * (H // k) * (W // k)
    ld = F.far_ld(window, npix, 1, esz, 16 // esz)
    shape = (1, npix, ld)          # (the slice is the whole pitch)
    lead = F.lead_for(window, (1, npix, 1), ld, esz)
    trail = F.trail_for((1, 16, 64))
    _need((lead + npix * ld + trail) * esz)
    mask = np.random.default_rng(3).uniform(0, 1, (B, H, W, 1)).astype(np.float32)
    _v, parent = F.far_view(SENTINEL, (1, npix, 1), ld, 0, lead, trail, adt, "cuda", use_arena=True)
    dst = parent[lead:lead + 1]          # the base pointer; the entry point takes lddst from dst.shape[-1]
    from shmgan_amd.ops import _p, _stream, check, lib
    check(lib().shm_mask_pool_pack_hw(_p(dev(mask)), _p(dst), ld, B, H, W, k, ops._F32 if dt == "f32" else ops._BF16, _stream()), "shm_mask_pool_pack_hw")
    torch.cuda.synchronize()
    PEAK["cases"] += 1
    want = torch.nn.functional.max_pool2d(torch.from_numpy(mask).permute(0, 3, 1, 2), k).permute(0, 2, 3, 1).reshape(npix).to(adt)
    view = parent.as_strided((1, npix, 1), (npix * ld, ld, 1), lead)
    assert torch.equal(F.gather(view).reshape(npix), want), "channel 0"
    bad = torch.zeros((), dtype=torch.int64, device="cuda")
    step = max(1, F.CHUNK // ld)
    for r0 in range(0, npix, step):          # every other element of every pitch: zero bits
        r = min(step, npix - r0)
        blk = F._bits(parent[lead + r0 * ld:lead + (r0 + r) * ld]).view(r, ld)
        cols = max(1, F.CHUNK // r)
        for lo in range(1, ld, cols):
            bad += torch.count_nonzero(blk[:, lo:min(ld, lo + cols)] != 0)
    assert int(bad) == 0, int(bad)
    assert F.far_outside_untouched(parent, shape, ld, 0, lead, SENTINEL), "a band was written"


def test_mul_mask_in_place_fp32_past_2_31_elements():
    """the fp32 form: y == x (each thread reads and writes its own four elements), 8 GiB of activations under 8 GiB of mask; out of place it would
    hold 24 GiB"""
    ops = P._ops()
    _need((NEL + GUARD) * (4 + 4), arena=False)
    x = _flat(torch.float32, SENTINEL)
    _fill_pattern(x, NEL)
    m = _flat(torch.float32, SENTINEL)
    for lo in range(0, NEL, FILL):
        hi = min(NEL, lo + FILL)
        m[lo:hi] = (torch.arange(lo, hi, dtype=torch.int64, device="cuda") % 3 != 0).to(torch.float32)
    ops.mul_mask(x, m, x, NEL, 2.0)
    torch.cuda.synchronize()
    for lo, hi in WINDOWS:
        want = _pattern(lo, hi) * (np.arange(lo, hi) % 3 != 0) * 2.0
        assert np.array_equal(x[lo:hi].cpu().numpy(), want), ("window", lo, hi)
    for lo in range(0, NEL, FILL):          # every element against the pattern rebuilt on the device
        hi = min(NEL, lo + FILL)
        i = torch.arange(lo, hi, dtype=torch.int64, device="cuda")
        want = (((i % 251) - 125).to(torch.float32) / 4.0) * (i % 3 != 0).to(torch.float32) * 2.0
        assert bool((x[lo:hi] == want).all()), lo
        del i, want
    assert _guard_ok(x, NEL) and _guard_ok(m, NEL)
    PEAK["cases"] += 1


# ======================================================================================= the compact RGB first layer past 2 GiB
# conv_rgb.hip reads one 16-byte chunk per pixel: its pitch is fixed, so these cases hold real pixels (2 GiB of image, 1 to 2 GiB of output at
# the narrowest layer the kernel takes, cout = 16) and are checked on strips of rows copied to the host, against the float64 convolution of the
# same strips: the first rows, the rows around byte 2^31 of x and of y, and the last rows.  Forward only.
RGB_COUT = 16
RGB_CASES = {
    # batch, h, w, compact kernel expected
    "batch33": (33, 2048, 2048, True),            # small images, 33 * 2048 * 2048 * 16 bytes = 2.06 GiB in all
    "below": (1, 8190, 16384, True),              # hi * wi * 16 = 0x7ff80000 < 0x7fffff00
    "at": (1, 8192, 16384, False),                # hi * wi * 16 = 0x80000000 >= 0x7fffff00: the generic kernels
}
assert 8190 * 16384 * 16 < 0x7fffff00 <= 8192 * 16384 * 16 and 33 * 2048 * 2048 * 16 > 1 << 31


def _rgb_strip_ref(xs, w, b, dt, last):
    """float64 output rows of input rows xs [L, W, 3] (L even, starting at an even row): L / 2 rows, of which the last is real only at the image's end"""
    ref = P._lrelu(P.conv_ref(xs[None].astype(np.float64), P._rnd(w, dt), 2)[0] + b)
    return ref if last else ref[:-1]


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("name", list(RGB_CASES))
def test_compact_rgb_forward_past_2_gib(name, dt):
    ops = P._ops()
    n, h, w, compact = RGB_CASES[name]
    adt, esz = P._adt(dt), R.ESZ[dt]
    pc, kpad, cout = 16 // esz, 64 // esz, RGB_COUT
    npx, ho, wo = n * h * w, h // 2, w // 2
    ybytes = n * ho * wo * cout * esz
    _need(npx * 16 + ybytes + (1 << 28), arena=False)
    # x: finite values in channels 0..2, zero in the chunk's other lanes and in the 64 + 64 elements behind the last pixel (the generic kernels read a
    # whole 64-byte row per tap: three chunks of the neighbours, times zero weight columns)
    x = torch.empty(npx * pc + 128, dtype=adt, device="cuda")
    gen = torch.Generator(device="cuda").manual_seed(5)
    for lo in range(0, npx, 1 << 24):
        hi = min(npx, lo + (1 << 24))
        t = torch.randn((hi - lo, pc), generator=gen, device="cuda")
        t[:, 3:] = 0
        x[lo * pc:hi * pc] = t.to(adt).view(-1)
        del t
    x[npx * pc:] = 0
    yflat = torch.empty(n * ho * wo * cout + 16 * wo * cout, dtype=adt, device="cuda")
    for lo in range(0, yflat.numel(), F.CHUNK):
        yflat[lo:lo + F.CHUNK].fill_(SENTINEL)
    rng = np.random.default_rng(77)
    wt = rng.standard_normal((3, 3, 3, cout)) * 0.3
    b = rng.standard_normal(cout).astype(np.float32)
    ops.conv2d_fwd(x, None, 0, pc, 0, P._wk(wt, kpad, dt), torch.from_numpy(b).cuda(), yflat, cout, n, h, w, kpad, cout, 3, 2, 0.2)
    torch.cuda.synchronize()
    kern = ops.last_kernel()
    print(f"{name} {dt}: {kern}, x {npx * 16 / GIB:.2f} GiB, y {ybytes / GIB:.2f} GiB")
    assert kern.startswith("conv3x3s2_rgb_fwd_kernel<") == compact, kern
    assert bool((yflat[n * ho * wo * cout:] == SENTINEL).all()), "written behind y"
    PEAK["cases"] += 1
    # strips: (image, first output row, rows)
    R8 = 8
    strips = {(0, 0), (n - 1, ho - R8)}
    xrow, yrow = w * 16, wo * cout * esz                      # bytes per row
    for byte, rowb, per_img, to_out in ((1 << 31, xrow, h, 2), (1 << 31, yrow, ho, 1)):
        r = byte // rowb                                      # global row that holds the byte
        if r < n * per_img:
            img, rr = divmod(r, per_img)
            strips.add((img, max(0, min(ho - R8, rr // to_out - R8 // 2))))
    xv, yv = x[:npx * pc].view(n, h, w, pc), yflat[:n * ho * wo * cout].view(n, ho, wo, cout)
    for img, r0 in sorted(strips):
        last = r0 + R8 == ho
        xs = xv[img, 2 * r0:min(h, 2 * (r0 + R8) + 2), :, :3].float().cpu().numpy()
        got = yv[img, r0:r0 + R8].float().cpu().numpy()
        ref = _rgb_strip_ref(xs, wt, b, dt, last)[:R8]
        fig = rel_l2(got, ref)
        print(f"  image {img} rows {r0}..{r0 + R8}: rel-L2 {fig:.3e}")
        assert fig < P.RECT_TOL[dt], (name, img, r0, fig)
