"""The convolution and InstanceNorm entry points on pitched, offset tensor VIEWS (include/shmgan_hip.h: every `ld*` is a channel pitch that
may exceed the channel count, and a tensor may be a channel slice of a wider buffer).

Every other module passes `ld == channels` on freshly allocated tensors, so a kernel that took the channel count where a pitch belongs, the
first source's pitch for the second, or a buffer extent from the wrong pitch would pass them all -- and the bf16 element-store epilogues, which
a tight torch tensor can never reach, would never run.  Method (pitch_ref.py has the harness and the table): each case runs the entry point
on tight tensors and on views of flat parents -- NaN around every input slice, util.SENTINEL around every output slice, guard bands as long
as the tensor itself in front and behind -- with the same values, forced variant and knobs.

  * the tight run is held to the float64 reference at the bound the project already holds the op to;
  * same shm_last_kernel(): outputs bit-equal to the tight run (quantities that pass through float64 atomics: 1e-12 of max-abs);
  * another kernel (a pitch took the layer off the weights-in-registers kernels, off the 16-byte InstanceNorm forms, or moved the gsum
    sums to the reduce pass): the kernel is the one pitch_ref predicts and the outputs are held to the float64 bound;
  * every element of every output parent outside the slice is bit-equal to its fill; "zero on entry, zero on return" scratch is zero.

One pytest case is one (family, variant, dtype, knobs) with all its layouts; a failure lists every layout that failed.
"""
import functools

import numpy as np
import pytest
import torch

import far_ref as F
import pitch_ref as R
from oracle import step_torch as st
from test_gsum_gpu import _check_sums, _sums
from test_variants_gpu import _check_stats, _rnd, _wk
from util import RECT_TOL, SENTINEL, conv_ref, host, nchw, nhwc, pad_c, rel_l2, t64

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
WTOL = {"f32": 1e-5, "bf16": 1e-4}          # weight gradients (test_rect_gpu.py)
INTOL = {"f32": 1e-5, "bf16": 4e-3}         # one InstanceNorm op against float64 (test_in_bwd_plan_gpu.py)
NAN = float("nan")


def _ops():
    from shmgan_amd import ops
    return ops


@pytest.fixture(autouse=True)
def _reset_tuning():
    yield
    _ops().set_tuning("reset", 0)


def _adt(dt):
    return BF if dt == "bf16" else torch.float32


def _lrelu(a, slope=0.2):
    return np.where(a > 0, a, slope * a)


class Alloc:
    """The tensors of one call in the layouts of one case: inputs in NaN parents, outputs in SENTINEL parents.  A case names a layout of
    pitch_ref.LAYOUTS per pitch argument, or holds a far_ref.Far (test_far_gpu.py; one per case): that tensor's parent has the bands of
    far_ref.lead_for / trail_for, lies in far_ref.arena() and is filled, written, read and scanned in chunks."""

    last = None          # the tensors of the latest call: a runner that ended in a refusal leaves its parents here for the sentinel check

    def __init__(self, case):
        self.case, self.watch, self.pitch = case, [], {}
        Alloc.last = self

    def _view(self, arg, shape, tdt, fill):
        kind = self.case.get(arg, "tight")
        if isinstance(kind, F.Far):
            lead = F.lead_for(kind.window, shape, kind.ld, torch.empty(0, dtype=tdt).element_size(), kind.W) if kind.lead is None else kind.lead
            v, parent = F.far_view(fill, shape, kind.ld, 0, lead, F.trail_for(shape), tdt, "cuda", use_arena=True)
            self.pitch[arg] = kind.ld
            return v, parent, kind.ld, 0, lead
        ld, off = R.layout(kind, shape[-1], tdt)
        v, parent = R.view_of(fill, shape, ld, off, None, tdt, "cuda")
        self.pitch[arg] = ld
        return v, parent, ld, off, None

    def inp(self, arg, vals, tdt, watch=False):
        """vals: float array [..., c].  watch: the call writes this tensor in place, so its parent is checked too."""
        v, parent, ld, off, lead = self._view(arg, vals.shape, tdt, NAN)
        assert v.data_ptr() % 16 == 0 or self.case.get(arg) in ("half",), arg          # input bases stay 16-byte aligned
        src = torch.from_numpy(np.ascontiguousarray(vals, dtype=np.float32)).to(tdt)
        if lead is None:
            v.copy_(src)
        else:
            F.scatter(v, src)
        if watch:
            self.watch.append((arg, parent, tuple(vals.shape), ld, off, NAN, lead))
        return v, ld

    def out(self, arg, shape, tdt):
        v, parent, ld, off, lead = self._view(arg, shape, tdt, SENTINEL)
        self.watch.append((arg, parent, tuple(shape), ld, off, SENTINEL, lead))
        return v, ld

    def untouched(self):
        return [arg for arg, parent, shape, ld, off, fill, lead in self.watch
                if not (R.outside_untouched(parent, shape, ld, off, None, fill) if lead is None else F.far_outside_untouched(parent, shape, ld, off, lead, fill))]


def _cpu(t):
    if t is None:
        return None
    return F.gather(t.detach()) if F.is_far(t) else t.detach().contiguous().cpu()


def _same_f64(a, b):
    """quantities behind float64 atomics in no fixed order: the run-to-run bound of test_pingpong_repeat_launches_are_bitwise_identical"""
    a, b = a.double(), b.double()
    return float((a - b).abs().max()) <= 1e-12 * float(b.abs().max())


def _set(variant, knobs):
    ops = _ops()
    ops.set_tuning("reset", 0)
    if variant != "-":
        ops.set_tuning("tapgemm.variant", variant)
    for k, v in knobs.items():
        ops.set_tuning(k, v)


# =====================================================================================================================
# runners: one pair per entry point.  run(fam, dt, case) -> dict of CPU tensors, "kern" and "touched" (output parents written outside their
# slice); check(fam, dt, res) asserts the float64 bounds and returns the figures.  BITWISE / ATOMIC / BWD below say how a result compares
# with the tight run's.
@functools.lru_cache(maxsize=None)
def _fwd_data(dt, n, h, w, c1, c2, cout, k, s, norm=None):
    """norm: the (single) source is the un-normalised activation of an InstanceNorm block; the reference convolves its normalised image, rounded
    to the activation type as shm_in_apply would store it.  Returns the operands, the reference, the block's table (device) and an aux tensor."""
    rng = np.random.default_rng(900 + cout + 7 * k + s)
    cin = c1 + c2
    xa = _rnd(rng.standard_normal((n, h, w, c1)), dt)
    xb = _rnd(rng.standard_normal((n, h, w, c2)), dt) if c2 else None
    wt = rng.standard_normal((k, k, cin, cout)) * 0.1
    b = rng.standard_normal(cout).astype(np.float32)
    nt, src = None, xa
    if norm:
        ops = _ops()
        xa = _rnd(xa * rng.uniform(0.5, 2.0, (n, 1, 1, c1)) + rng.uniform(-1, 1, (n, 1, 1, c1)), dt)
        beta = rng.uniform(-0.5, 0.5, c1).astype(np.float32)
        stats = torch.zeros(n * c1 * 2, dtype=torch.float64, device="cuda")
        ops.in_stats(torch.from_numpy(xa.astype(np.float32)).cuda().to(_adt(dt)), c1, stats, n, h * w, c1, 1e-6)
        nt = torch.full((n, 4, c1), 9.0, dtype=torch.float32, device="cuda")
        ops.in_norm_table(stats, torch.from_numpy(beta).cuda(), nt, n, c1)
        torch.cuda.synchronize()
        st_ = host(stats).reshape(n, 1, 1, c1, 2)
        src = _rnd((xa - st_[..., 0]) * st_[..., 1] + beta, dt)
    ref = _lrelu(conv_ref(src if xb is None else np.concatenate([src, xb], -1), _rnd(wt, dt), s) + b)
    aux = _rnd(rng.standard_normal(ref.shape), dt)
    return xa, xb, wt, b, ref, nt, aux


def _fwd_key(sh):
    return tuple(sh[x] for x in ("n", "h", "w", "c1", "c2", "cout", "k", "s")) + (sh.get("norm"),)


def _run_fwd(fam, dt, case):
    ops, sh = _ops(), fam["shape"]
    n, h, w, c1, c2, cout, k, s = (sh[x] for x in ("n", "h", "w", "c1", "c2", "cout", "k", "s"))
    xa, xb, wt, b, ref, nt, auxv = _fwd_data(dt, *_fwd_key(sh))
    adt, A = _adt(dt), Alloc(case)
    x, ldx = A.inp("ldx", xa, adt)
    x2, ldx2 = A.inp("ldx2", xb, adt) if c2 else (None, 0)
    y, ldy = A.out("ldy", ref.shape, adt)
    wk, bias, kw = _wk(wt, c1 + c2, dt), torch.from_numpy(b).cuda(), {}
    if sh.get("norm"):
        kw = dict(nt_x=nt, norm_mode=ops.NORM_SCALED if sh["norm"] == "scaled" else ops.NORM_EXACT)
        if sh["norm"] == "scaled":            # per-sample operands: the weights times inv, the bias rows (shm_conv2d_norm_prepare)
            wk_n = torch.empty((n, wk.numel()), device="cuda", dtype=adt)
            bias_n = torch.empty((n, cout), device="cuda")
            ops.conv2d_norm_prepare(wk, bias, nt, c1, 0, wk_n, bias_n, n, c1, cout, k)
            wk, bias = wk_n, bias_n
    args = (x, x2, c1 if c2 else 0, ldx, ldx2, wk, bias, y, ldy, n, h, w, c1 + c2, cout, k, s, 0.2)
    res = {}
    if "ldaux" in fam["ch"]:
        aux, ldaux = A.inp("ldaux", auxv, adt)
        red = torch.zeros(ops.GSUM_SLOTS * n * cout * 2, dtype=torch.float64, device="cuda")
        ops.conv2d_fwd(*args, gsum=(aux, ldaux, red))
        torch.cuda.synchronize()
        res.update(red=_cpu(red.view(ops.GSUM_SLOTS, n, cout, 2).sum(0)), red_raw=_cpu(red), aux=_cpu(aux))
    elif fam["entry"] == "conv2d_in_fwd" and cout % 4 == 0:
        stats = torch.empty(n * cout * 2, dtype=torch.float64, device="cuda")
        scr = torch.zeros(ops.STATS_SLOTS * n * cout * 2, dtype=torch.float64, device="cuda")
        ops.conv2d_in_fwd(*args, stats, 1e-6, scratch=scr, **kw)
        torch.cuda.synchronize()
        res["stats"] = _cpu(stats)
        res["scratch_zero"] = float(scr.abs().max()) == 0.0
    else:
        ops.conv2d_fwd(*args)
        torch.cuda.synchronize()
    res.update(kern=ops.last_kernel(), y=_cpu(y), touched=A.untouched())
    return res


def _check_fwd(fam, dt, res):
    sh = fam["shape"]
    ref = _fwd_data(dt, *_fwd_key(sh))[4]
    got = host(res["y"].float())
    # SHM_NORM_SCALED re-associates the normalisation into the operands: the plain product's bound plus the bound test_norm_fold_gpu.py holds the
    # scaled form to against the plain product (rel-L2 3e-6 fp32 / 1.5e-2 bf16, the per-sample weights being rounded to bf16 once more)
    tol = RECT_TOL[dt] + ({"f32": 3e-6, "bf16": 1.5e-2}[dt] if sh.get("norm") == "scaled" else 0.0)
    assert rel_l2(got, ref) < tol, ("y", rel_l2(got, ref))
    if "stats" in res:
        _check_stats(res["stats"], got, sh["n"], sh["cout"], dt)
    if "red_raw" in res:
        _check_sums(res["red_raw"], res["y"], res["aux"], dt)
    return {"y": rel_l2(got, ref)}


@functools.lru_cache(maxsize=None)
def _tr_data(dt, n, h, w, cin, cout):
    rng = np.random.default_rng(910 + cout)
    x = _rnd(rng.standard_normal((n, h, w, cin)), dt)
    wt = _rnd(rng.standard_normal((3, 3, cout, cin)) * 0.1, dt)
    b = rng.standard_normal(cout).astype(np.float32)
    ref = _lrelu(nhwc(st.conv2d_transpose_same(nchw(x), t64(wt))) + b)
    return x, wt, b, ref


def _run_transpose(fam, dt, case):
    ops, sh = _ops(), fam["shape"]
    n, h, w, cin, cout = (sh[x] for x in ("n", "h", "w", "cin", "cout"))
    xv, wt, b, ref = _tr_data(dt, n, h, w, cin, cout)
    adt, A = _adt(dt), Alloc(case)
    x, ldx = A.inp("ldx", xv, adt)
    y, ldy = A.out("ldy", ref.shape, adt)
    ops.conv2d_transpose_fwd(x, ldx, torch.from_numpy(wt.astype(np.float32)).cuda().to(adt), torch.from_numpy(b).cuda(), y, ldy, n, h, w, cin, cout, 0.2)
    torch.cuda.synchronize()
    return dict(kern=ops.last_kernel(), y=_cpu(y), touched=A.untouched())


def _check_transpose(fam, dt, res):
    sh = fam["shape"]
    ref = _tr_data(dt, *(sh[x] for x in ("n", "h", "w", "cin", "cout")))[3]
    got = host(res["y"].float())
    assert rel_l2(got, ref) < RECT_TOL[dt], ("y", rel_l2(got, ref))
    return {"y": rel_l2(got, ref)}


@functools.lru_cache(maxsize=None)
def _dg_data(dt, n, h, w, cin, cout, s):
    rng = np.random.default_rng(920 + cin + s)
    wt = _rnd(rng.standard_normal((3, 3, cin, cout)) * 0.1, dt)
    dy = _rnd(rng.standard_normal((n, h // s, w // s, cout)), dt)
    xt = torch.zeros(n, cin, h, w, dtype=torch.float64, requires_grad=True)
    ref, = torch.autograd.grad(st.conv2d_same(xt, t64(wt), s), xt, nchw(dy))
    aux = _rnd(rng.standard_normal((n, h, w, cin)), dt)
    return wt, dy, nhwc(ref), aux


def _run_dgrad(fam, dt, case):
    ops, sh, ch = _ops(), fam["shape"], fam["ch"]
    n, h, w, cin, cout, n1, s = (sh[x] for x in ("n", "h", "w", "cin", "cout", "n1", "s"))
    wt, dyv, ref, auxv = _dg_data(dt, n, h, w, cin, cout, s)
    adt, A = _adt(dt), Alloc(case)
    odt = torch.float32 if fam["out_f32"] else adt
    split = "lddx2" in ch
    c0 = ch["lddx"]
    dy, lddy = A.inp("lddy", dyv, adt)
    dx, lddx = A.out("lddx", (n, h, w, c0), odt)
    dx2, lddx2 = A.out("lddx2", (n, h, w, cin - c0), odt) if split else (None, 0)
    g0 = g1 = None
    aux0 = aux1 = None
    if "ldaux" in ch:
        aux0, ld = A.inp("ldaux", auxv[..., :c0], adt)
        g0 = (aux0, ld, torch.zeros(ops.GSUM_SLOTS * n * c0 * 2, dtype=torch.float64, device="cuda"))
    if "ldaux2" in ch:
        aux1, ld = A.inp("ldaux2", auxv[..., c0:], adt)
        g1 = (aux1, ld, torch.zeros(ops.GSUM_SLOTS * n * (cin - c0) * 2, dtype=torch.float64, device="cuda"))
    ops.conv2d_dgrad(dy, lddy, torch.from_numpy(wt.astype(np.float32)).cuda().to(adt), dx, dx2, n1 if split else 0, lddx, lddx2, n, h, w, cin, cout, 3, s, gsum=g0, gsum2=g1)
    torch.cuda.synchronize()
    res = dict(kern=ops.last_kernel(), dx=_cpu(dx), dx2=_cpu(dx2), touched=A.untouched())
    if g0:
        res["red"] = _cpu(g0[2].view(ops.GSUM_SLOTS, n, c0, 2).sum(0))
        res["red_raw"], res["aux"] = _cpu(g0[2]), _cpu(aux0)
    if g1:
        res["red2"] = _cpu(g1[2].view(ops.GSUM_SLOTS, n, cin - c0, 2).sum(0))
        res["red2_raw"], res["aux2"] = _cpu(g1[2]), _cpu(aux1)
    return res


def _check_dgrad(fam, dt, res):
    sh = fam["shape"]
    ref = _dg_data(dt, *(sh[x] for x in ("n", "h", "w", "cin", "cout", "s")))[2]
    got = host(res["dx"].float()) if res["dx2"] is None else np.concatenate([host(res["dx"].float()), host(res["dx2"].float())], -1)
    tol = 1e-4 if fam["out_f32"] else RECT_TOL[dt]          # (bf16 operands, fp32 outputs: test_rect_gpu.py's bound for SHM_BF16_GF32)
    assert rel_l2(got, ref) < tol, ("dx", rel_l2(got, ref))
    sdt = "f32" if fam["out_f32"] else dt
    if "red_raw" in res:
        _check_sums(res["red_raw"], res["dx"], res["aux"], sdt)
    if "red2_raw" in res:
        _check_sums(res["red2_raw"], res["dx2"], res["aux2"], sdt)
    return {"dx": rel_l2(got, ref)}


@functools.lru_cache(maxsize=None)
def _wg_data(dt, n, h, w, c1, c2, cout, s, norm=False):
    """norm: x is the un-normalised activation of an InstanceNorm block, normalised on the fly (SHM_NORM_EXACT: the arithmetic and rounding of
    shm_in_apply); the reference takes its normalised image rounded to the activation type.  Returns x, dy, the reference and the table."""
    rng = np.random.default_rng(930 + cout + s)
    cin = c1 + c2
    x = _rnd(rng.standard_normal((n, h, w, cin)), dt)
    dy = _rnd(rng.standard_normal((n, -(-h // s), -(-w // s), cout)), dt)
    nt, src = None, x
    if norm:
        ops = _ops()
        x = _rnd(x * rng.uniform(0.5, 2.0, (n, 1, 1, cin)) + rng.uniform(-1, 1, (n, 1, 1, cin)), dt)
        beta = rng.uniform(-0.5, 0.5, cin).astype(np.float32)
        stats = torch.zeros(n * cin * 2, dtype=torch.float64, device="cuda")
        ops.in_stats(torch.from_numpy(x.astype(np.float32)).cuda().to(_adt(dt)), cin, stats, n, h * w, cin, 1e-6)
        nt = torch.full((n, 4, cin), 9.0, dtype=torch.float32, device="cuda")
        ops.in_norm_table(stats, torch.from_numpy(beta).cuda(), nt, n, cin)
        torch.cuda.synchronize()
        st_ = host(stats).reshape(n, 1, 1, cin, 2)
        src = _rnd((x - st_[..., 0]) * st_[..., 1] + beta, dt)
    wt = torch.zeros(3, 3, cin, cout, dtype=torch.float64, requires_grad=True)
    ref, = torch.autograd.grad(st.conv2d_same(nchw(src), wt, s), wt, nchw(dy))
    return x, dy, ref.numpy(), nt


def _wg_key(sh):
    return tuple(sh[x] for x in ("n", "h", "w", "c1", "c2", "cout", "s")) + (bool(sh.get("norm")),)


def _run_wgrad(fam, dt, case):
    ops, sh = _ops(), fam["shape"]
    n, h, w, c1, c2, cout, s = (sh[x] for x in ("n", "h", "w", "c1", "c2", "cout", "s"))
    xv, dyv, ref, nt = _wg_data(dt, *_wg_key(sh))
    adt, A, cin = _adt(dt), Alloc(case), c1 + c2
    kb = 16 if dt == "f32" else 32
    cin_ld = cin if c2 or cin % kb == 0 else R.up(cin, kb)          # a thin first layer: its channels in a zero-padded pitch of 16 / 32
    x, ldx = A.inp("ldx", pad_c(xv[..., :c1], cin_ld) if cin_ld != cin else xv[..., :c1], adt)
    x2, ldx2 = A.inp("ldx2", xv[..., c1:], adt) if c2 else (None, 0)
    dy, lddy = A.inp("lddy", dyv, adt)
    ws = torch.full((ops.conv2d_wgrad_workspace(n, -(-h // s), -(-w // s), cin, cout, 3) // 4 + 1024,), NAN, device="cuda")
    dw, parent = R.view_of(3.0, (3, 3, cin, cout), cout, 0, None, torch.float32, "cuda")
    res = {}
    for acc in (0, 1):          # plain, then accumulate onto it; the split-K workspace starts as NaN (every slab element a block owns is written)
        ws.fill_(NAN)
        ops.conv2d_wgrad(x, x2, c1 if c2 else 0, ldx, ldx2, dy, lddy, dw, n, h, w, cin, cin_ld, cout, 3, s, acc, ws, nt_x=nt)
        torch.cuda.synchronize()
        res["dw%d" % acc] = _cpu(dw)
    res.update(kern=ops.last_kernel(), touched=A.untouched() + ([] if R.outside_untouched(parent, (3, 3, cin, cout), cout, 0, None, 3.0) else ["dw"]))
    return res


def _check_wgrad(fam, dt, res):
    sh = fam["shape"]
    ref = _wg_data(dt, *_wg_key(sh))[2]
    assert rel_l2(host(res["dw0"]), ref) < WTOL[dt], ("dw", rel_l2(host(res["dw0"]), ref))
    assert rel_l2(host(res["dw1"]), 2 * ref) < WTOL[dt], ("dw accumulated", rel_l2(host(res["dw1"]), 2 * ref))
    return {"dw": rel_l2(host(res["dw0"]), ref)}


# ---- InstanceNorm
@functools.lru_cache(maxsize=None)
def _in_data(dt, n, h, w, c):
    """a (off-centre, per-channel scale), its statistics from the tight shm_in_stats, beta, gradients; float64 references of every op."""
    ops = _ops()
    rng = np.random.default_rng(940 + c)
    a = _rnd(rng.standard_normal((n, h, w, c)) * rng.uniform(0.5, 2.0, (n, 1, 1, c)) + rng.uniform(-1, 1, (n, 1, 1, c)), dt)
    beta = rng.normal(0, 0.5, c).astype(np.float32)
    g1 = _rnd(rng.standard_normal((n, h, w, c)), dt)
    g2 = _rnd(rng.standard_normal((n, h // 2, w // 2, c)), dt)
    hdz = rng.standard_normal((n, h, w)).astype(np.float32)
    hw_ = rng.standard_normal(c).astype(np.float32)
    ad = torch.from_numpy(a.astype(np.float32)).cuda().to(_adt(dt))
    stats = torch.zeros(n * c * 2, dtype=torch.float64, device="cuda")
    ops.in_stats(ad, c, stats, n, h * w, c, 1e-6)
    torch.cuda.synchronize()
    s = host(stats).reshape(n, 1, 1, c, 2)
    mean, inv = s[..., 0], s[..., 1]
    xh = (a - mean) * inv
    out = xh + beta
    return dict(a=a, beta=beta, g1=g1, g2=g2, hdz=hdz, hw=hw_, stats=stats, mean=mean, inv=inv, xh=xh, out=out)


def _pool(x):
    n, h, w, c = x.shape
    return x.reshape(n, h // 2, 2, w // 2, 2, c).mean((2, 4))


def _bwd_ref(d, G, slope=0.2, gx=None):
    """gx: mean(d_out * xhat) per (sample, channel) where the entry point defines it otherwise than on the tensors themselves (shm_in_bwd_apply)."""
    gx = (G * d["xh"]).mean((1, 2), keepdims=True) if gx is None else gx
    dd = d["inv"] * (G - G.mean((1, 2), keepdims=True) - d["xh"] * gx)
    return np.where(d["a"] > 0, dd, dd * slope)


def _apply_gx(d, dt):
    """shm_in_bwd_apply with a pooled gradient takes sum(d_out * xhat) from its two sum inputs, and the header defines the pooled one against the
    pooled normalised tensor AS STORED: sum g2 * avgpool(xhat) = sum g2 * pooled - beta * sum g2.  In bf16 `pooled` is rounded, so that is not the
    sum over the tensors to 1e-5 (dbias, where dz cancels, moved by 1e-3 against a reference that ignored it).  The same definition in float64."""
    n, h, w, c = d["a"].shape
    pool_n = _rnd(_pool(_rnd(d["out"], dt)), dt)
    s = (d["g1"] * d["xh"]).sum((1, 2)) + (d["g2"] * (pool_n - d["beta"].astype(np.float64))).sum((1, 2))
    return (s / (h * w)).reshape(n, 1, 1, c)


def _run_in(fam, dt, case):
    ops, sh, entry = _ops(), fam["shape"], fam["entry"]
    n, h, w, c = (sh[x] for x in ("n", "h", "w", "c"))
    d = _in_data(dt, n, h, w, c)
    adt, A = _adt(dt), Alloc(case)
    beta = torch.from_numpy(d["beta"]).cuda()
    res = {}
    if entry == "avgpool2_fwd":
        x, ldx = A.inp("ldx", d["a"], adt)
        y, ldy = A.out("ldy", (n, h // 2, w // 2, c), adt)
        ops.avgpool2_fwd(x, ldx, y, ldy, n, h, w, c)
        res["pooled"] = y
    else:
        a, lda = A.inp("lda", d["a"], adt, watch=bool(sh.get("inplace")))
    if entry == "in_stats":
        stats = torch.full((n * c * 2,), 9.0, dtype=torch.float64, device="cuda")
        ops.in_stats(a, lda, stats, n, h * w, c, 1e-6)
        res["stats"] = stats
    elif entry == "in_apply":
        out, ldo = (a, lda) if sh.get("inplace") else A.out("ldo", (n, h, w, c), adt)
        ops.in_apply(a, lda, d["stats"], beta, out, ldo, n, h * w, c)
        res["out"] = out
    elif entry == "in_apply_pool":
        out, ldo = A.out("ldo", (n, h, w, c), adt)
        pooled, ldp = A.out("ldp", (n, h // 2, w // 2, c), adt)
        ops.in_apply_pool(a, lda, d["stats"], beta, out, ldo, pooled, ldp, n, h, w, c)
        res.update(out=out, pooled=pooled)
    elif entry == "in_pool":
        pooled, ldp = A.out("ldp", (n, h // 2, w // 2, c), adt)
        ops.in_pool(a, lda, d["stats"], beta, pooled, ldp, n, h, w, c)
        res["pooled"] = pooled
    elif entry in ("in_bwd", "in_bwd_apply", "in_bwd_rank1"):
        g2 = None
        ldg1 = ldg2 = 0
        if entry != "in_bwd_rank1":
            g1, ldg1 = A.inp("ldg1", d["g1"], adt)
            if sh.get("g2"):
                g2, ldg2 = A.inp("ldg2", d["g2"], adt)
        dz, lddz = A.out("lddz", (n, h, w, c), adt)
        sums = sh.get("sums", "both")          # "both": dbias and dz_sums; "dbias": the bias gradient alone (folded by the kernels); "none"
        db = torch.zeros(c, dtype=torch.float64, device="cuda") if sums != "none" else None
        keep = torch.full((n, c), 9.0, dtype=torch.float64, device="cuda") if sums == "both" else None
        zero = []
        if entry == "in_bwd_apply":
            tg1, ta = torch.from_numpy(d["g1"]), torch.from_numpy(d["a"])
            red = torch.zeros(ops.GSUM_SLOTS * n * c * 2, dtype=torch.float64, device="cuda")
            red.view(ops.GSUM_SLOTS, n, c, 2)[0].copy_(torch.from_numpy(_sums(tg1, ta)).cuda())
            redp = None
            if g2 is not None:          # sums of g2 against the pooled normalised tensor as the device stores it
                pool_n = _rnd(_pool(_rnd(d["out"], dt)), dt)
                redp = torch.zeros_like(red)
                redp.view(ops.GSUM_SLOTS, n, c, 2)[0].copy_(torch.from_numpy(_sums(torch.from_numpy(d["g2"]), torch.from_numpy(pool_n))).cuda())
            dstage = torch.zeros(n * c, dtype=torch.float64, device="cuda")
            ops.in_bwd_apply(g1, ldg1, g2, ldg2, a, lda, d["stats"], beta, red, redp, dstage, dz, lddz, db, n, h, w, c, 0.2, dz_sums=keep)
            zero = [red, dstage] + ([redp] if redp is not None else [])
        else:
            red = torch.zeros(n * c * 3, dtype=torch.float64, device="cuda")
            zero = [red]
            if entry == "in_bwd_rank1":
                ops.in_bwd_rank1(torch.from_numpy(d["hdz"]).cuda(), torch.from_numpy(d["hw"]).cuda(), a, lda, d["stats"], red, dz, lddz, db, n, h, w, c, 0.2, dz_sums=keep)
            else:
                fused = torch.zeros(ops.in_bwd_fused_doubles(n, h * w, c), dtype=torch.float64, device="cuda") if sh.get("scratch") else None
                ops.in_bwd(g1, ldg1, g2, ldg2, a, lda, d["stats"], red, dz, lddz, db, n, h, w, c, 0.2, fused=fused, dz_sums=keep)
                if fused is not None:
                    torch.cuda.synchronize()
                    rows = (n * (h * w * min(c, 64) // 16384) * 3 * c + 1) // 2 if "fused" in ops.last_kernel() else 0
                    res["scratch_zero"] = bool((fused[rows:].view(torch.int64) == 0).all())
        res.update(dz=dz)
        if db is not None:
            res["dbias"] = db
        if keep is not None:
            res["dz_sums"] = keep
        torch.cuda.synchronize()
        res["scratch_zero"] = res.get("scratch_zero", True) and all(float(z.abs().max()) == 0.0 for z in zero)
    torch.cuda.synchronize()
    res = {k: (_cpu(v) if isinstance(v, torch.Tensor) else v) for k, v in res.items()}
    res.update(kern=ops.last_kernel() if entry in ("in_bwd", "in_bwd_rank1") else entry, touched=A.untouched())
    return res


def _check_in(fam, dt, res):
    sh, entry = fam["shape"], fam["entry"]
    n, h, w, c = (sh[x] for x in ("n", "h", "w", "c"))
    d = _in_data(dt, n, h, w, c)
    tol, figs = INTOL[dt], {}

    def close(name, got, ref):
        figs[name] = rel_l2(got, ref)
        assert figs[name] < tol, (name, figs[name])

    if entry == "in_stats":
        _check_stats(res["stats"], d["a"], n, c, dt)
    if "out" in res:
        close("out", host(res["out"].float()), d["out"])
    if "pooled" in res:
        src = d["a"] if entry == "avgpool2_fwd" else _rnd(d["out"], dt)           # the pool averages the values as stored
        close("pooled", host(res["pooled"].float()), _pool(src))
    if "dz" in res:
        if entry == "in_bwd_rank1":
            G = d["hdz"].astype(np.float64)[..., None] * d["hw"].astype(np.float64)
        else:
            G = d["g1"] + (0.25 * np.repeat(np.repeat(d["g2"], 2, 1), 2, 2) if sh.get("g2") else 0.0)
        zr = _bwd_ref(d, G, gx=_apply_gx(d, dt) if entry == "in_bwd_apply" and sh.get("g2") else None)
        close("dz", host(res["dz"].float()), zr)
        sr = zr.sum((1, 2))
        # the bounds of test_in_bwd_plan_gpu.py.  Two passes (and shm_in_bwd_apply): the sums are taken of the unrounded dz -- rel-L2 1e-5 against
        # float64 in either type, as its chunk test asks.  One pass: its dispatch table's bound, against the column sums of |dz|.
        scale = np.abs(zr).sum((0, 1, 2)).max()
        for name, ref in (("dbias", sr.sum(0)), ("dz_sums", sr)):
            if name in res:
                figs[name] = rel_l2(host(res[name]), ref)
                if "fused" in res["kern"]:
                    assert np.abs(host(res[name]) - ref).max() <= tol * scale, (name, figs[name])
                else:
                    assert figs[name] < 1e-5, (name, figs[name])
    return figs


RUN = {"conv2d_fwd": (_run_fwd, _check_fwd), "conv2d_in_fwd": (_run_fwd, _check_fwd), "conv2d_transpose_fwd": (_run_transpose, _check_transpose),
       "conv2d_dgrad": (_run_dgrad, _check_dgrad), "conv2d_wgrad": (_run_wgrad, _check_wgrad)}
BITWISE = ("y", "dx", "dx2", "dw0", "dw1", "out", "pooled")                                     # same kernel: bit-equal to the tight run
ATOMIC = ("stats", "red", "red2")                                                               # float64 atomics in no fixed order: 1e-12 of max-abs
BWD = ("dz", "dbias", "dz_sums")                                                                # behind the reduce pass's atomics: rel-L2 1e-5 (test_in_bwd_plan_gpu.py,
#                                                                                               chunked against unchunked); the one-pass kernels add in block order: bit-equal


def _expected_kernel(fam, variant, dt, case, tight_kern):
    """shm_last_kernel() of a pitched call, from the tight call's and the predicates of pitch_ref ("startswith:" / "not-endswith:": that much of it)."""
    entry, ch = fam["entry"], fam["ch"]
    if entry in ("in_bwd", "in_bwd_rank1"):
        ld = {a: R.layout(case.get(a, "tight"), c, dt)[0] for a, c in ch.items()}
        one = tight_kern if "fused" in tight_kern else None
        return R.in_bwd_form(dt, fam["shape"]["c"], ld.get("ldg1"), ld["lda"], ld["lddz"], ld.get("ldg2"), entry == "in_bwd_rank1", one,
                             R.addr16(case, "lddz", ch["lddz"], dt))
    if entry == "conv2d_wgrad" and "thin" in tight_kern:
        return tight_kern if R.wgrad_thin_pitch(R.layout(case.get("ldx", "tight"), 16, dt)[0]) else "wgrad_halo_kernel"
    if entry not in ("conv2d_fwd", "conv2d_in_fwd", "conv2d_dgrad", "conv2d_transpose_fwd"):
        return tight_kern
    gs = "ldaux" in ch or "ldaux2" in ch
    if variant == "auto" and dt == "bf16" and not fam["out_f32"] and not all(R.conv_out_terms(fam, dt, case, "wreg").values()):
        return "startswith:tapgemm_halo_kernel<__bf16, __bf16, "          # off the weights-in-registers kernels (the gsum sums then come from the reduce pass)
    if gs and variant in ("halo64_st", "halo128_st", "auto"):
        fused = all(R.conv_out_terms(fam, dt, case, "gsum").values())
        was = tight_kern.endswith(", true>")
        if fused == was:
            return tight_kern
        # (under the automatic choice the layer may also move to another plain kernel: whichever it is, it has no gsum epilogue)
        return "not-endswith:, true>" if variant == "auto" else tight_kern.replace(", true>", ">")
    return tight_kern


def _gsum_fused(fam, dt, case):
    return all(R.conv_out_terms(fam, dt, case, "gsum").values())


TABLE = []
for _fam in R.FAMILIES:
    for _dt in _fam["dts"]:
        for _v in _fam["variants"]:
            for _kn in R.knob_sets(_fam):
                _sid = "-".join(str(_fam["shape"][k]) for k in sorted(_fam["shape"]))
                _kid = ",".join(f"{k.split('.')[-1]}={v}" for k, v in _kn.items())
                TABLE.append(pytest.param(_fam, _v, _dt, _kn, id="/".join(x for x in (_fam["name"], _sid, _v, _dt, _kid) if x and x != "-")))


@pytest.mark.parametrize("fam,variant,dt,knobs", TABLE)
def test_pitched_views(fam, variant, dt, knobs):
    run, check = RUN.get(fam["entry"], (_run_in, _check_in))
    cases = R.family_cases(fam, dt)
    assert cases[0][0] == "tight"
    _set(variant, knobs)
    tight = run(fam, dt, {})
    figs = check(fam, dt, tight)                    # the tight run against float64, once
    assert not tight["touched"] and tight.get("scratch_zero", True), tight["touched"]
    print(f"tight: {tight['kern']} {figs}")
    named = R.tight_kernel(fam, variant, dt, knobs)
    assert named is None or tight["kern"] == named, (tight["kern"], named)
    failed = []
    for cid, case in cases[1:]:
        _set(variant, knobs)
        res = run(fam, dt, case)
        want = _expected_kernel(fam, variant, dt, case, tight["kern"])
        try:
            assert not res["touched"], ("written outside the slice", res["touched"])
            assert res.get("scratch_zero", True), "scratch not zero on return"
            if want.startswith("startswith:"):
                assert res["kern"].startswith(want[11:]), ("kernel", res["kern"], want)
            elif want.startswith("not-endswith:"):
                assert not res["kern"].endswith(want[13:]) and res["kern"], ("kernel", res["kern"], want)
            else:
                assert res["kern"] == want, ("kernel", res["kern"], want)
            figs = check(fam, dt, res)              # (also when bit-equal: it costs nothing and says more when the comparison below fails)
            if res["kern"] == tight["kern"]:
                for f in BITWISE:
                    if tight.get(f) is not None:
                        assert torch.equal(res[f], tight[f]), (f, "not bit-equal to the tight run", float((res[f].double() - tight[f].double()).abs().max()))
                for f in ATOMIC:
                    # (gsum: only when both calls took the sums the same way -- the DMA tiles keep their name when the sums move to the reduce pass)
                    if tight.get(f) is not None and (f == "stats" or _gsum_fused(fam, dt, case) == _gsum_fused(fam, dt, {})):
                        assert _same_f64(res[f], tight[f]), (f, "beyond 1e-12 of the tight run")
                for f in BWD:
                    if tight.get(f) is None:
                        continue
                    if "fused" in tight["kern"]:            # the one-pass forms add in block order: bitwise reproducible
                        assert torch.equal(res[f], tight[f]), (f, "not bit-equal to the tight run")
                    else:
                        r = rel_l2(host(res[f].float() if f == "dz" else res[f]), host(tight[f].float() if f == "dz" else tight[f]))
                        assert r < 1e-5, (f, "against the tight run", r)
            print(f"{cid}: {res['kern']} {figs} {'same kernel' if res['kern'] == tight['kern'] else 'OTHER KERNEL'}")
        except AssertionError as e:
            failed.append((cid, res["kern"], str(e)[:300]))
            print(f"{cid}: FAILED {res['kern']} {str(e)[:300]}")
    assert not failed, failed


# =====================================================================================================================
# the compact RGB first layer (conv_rgb.hip): one 16-byte chunk per pixel.  The streaming kernels take a 16-byte-aligned y / dy whose pitch is a
# multiple of 16 bytes and step aside for anything else; the image itself may start at any 16-byte offset inside its buffer.
def _rgb_x(x, dt, shift):
    """The compact image `shift` chunks into a flat parent: NaN in front, and behind it the zero slack the generic kernels need (they read a
    whole 64-byte operand row per pixel: the three chunks behind the last pixel, times the zero weight columns), then NaN."""
    adt, pc = _adt(dt), 4 if dt == "f32" else 8
    body = torch.from_numpy(np.ascontiguousarray(pad_c(x, pc), dtype=np.float32)).to(adt).reshape(-1)
    lead = 64 + shift * pc
    parent = torch.full((lead + body.numel() + 64 + 64,), NAN, dtype=adt)
    parent[lead:lead + body.numel()] = body
    parent[lead + body.numel():lead + body.numel() + 64] = 0.0
    parent = parent.cuda()
    return parent[lead:lead + body.numel()].view(x.shape[:-1] + (pc,)), parent


@functools.lru_cache(maxsize=None)
def _rgb_data(dt):
    rng = np.random.default_rng(77)
    n, h, cout = 2, 32, 64
    x = _rnd(rng.standard_normal((n, h, h, 3)), dt)
    w = rng.standard_normal((3, 3, 3, cout)) * 0.3
    b = rng.standard_normal(cout).astype(np.float32)
    dy = _rnd(rng.standard_normal((n, h // 2, h // 2, cout)), dt)
    ref = _lrelu(conv_ref(x, _rnd(w, dt), 2) + b)
    wt = torch.zeros(3, 3, 3, cout, dtype=torch.float64, requires_grad=True)
    dref, = torch.autograd.grad(st.conv2d_same(nchw(x), wt, 2), wt, nchw(dy))
    return n, h, cout, x, w, b, dy, ref, dref.numpy()


RGB_Y = {"f32": ("tight", "wide", "slice", "odd-wide"), "bf16": ("tight", "wide", "slice", "odd-wide", "half", "plus4")}


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_compact_rgb_forward_on_views(dt):
    ops = _ops()
    n, h, cout, xv, w, b, _, ref, _ = _rgb_data(dt)
    adt, kpad = _adt(dt), 16 if dt == "f32" else 32
    wk, bias = _wk(w, kpad, dt), torch.from_numpy(b).cuda()
    first, failed = None, []
    for shift in (0, 1):
        for kind in RGB_Y[dt]:
            x, _ = _rgb_x(xv, dt, shift)
            assert x.data_ptr() % 16 == 0
            A = Alloc({"ldy": kind})
            y, ldy = A.out("ldy", ref.shape, adt)
            stats = torch.empty(n * cout * 2, dtype=torch.float64, device="cuda")
            scr = torch.zeros(ops.STATS_SLOTS * n * cout * 2, dtype=torch.float64, device="cuda")
            ops.conv2d_in_fwd(x, None, 0, x.shape[-1], 0, wk, bias, y, ldy, n, h, h, kpad, cout, 3, 2, 0.2, stats, 1e-6, scratch=scr)
            torch.cuda.synchronize()
            kern, got = ops.last_kernel(), _cpu(y)
            streaming = kind not in ("half", "plus4")           # conv_rgb.hip: ldy % (16 / esz) || (y & 15) -> the generic kernels
            try:
                assert kern.startswith("conv3x3s2_rgb_fwd_kernel<") == streaming, kern
                assert not A.untouched() and float(scr.abs().max()) == 0.0
                assert rel_l2(host(got.float()), ref) < RECT_TOL[dt], rel_l2(host(got.float()), ref)
                _check_stats(stats, host(got.float()), n, cout, dt)
                if streaming:
                    first = got if first is None else first
                    assert torch.equal(got, first), "not bit-equal to the tight run"
                print(f"x+{shift} ldy-{kind}: {kern} {rel_l2(host(got.float()), ref):.3e}")
            except AssertionError as e:
                failed.append((shift, kind, kern, str(e)[:200]))
    assert not failed, failed


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_compact_rgb_weight_gradient_on_views(dt):
    ops = _ops()
    n, h, cout, xv, _, _, dyv, _, dref = _rgb_data(dt)
    adt, kpad = _adt(dt), 16 if dt == "f32" else 32
    ws = torch.empty(ops.conv2d_wgrad_workspace(n, h // 2, h // 2, 3, cout, 3) // 4 + 1024, device="cuda")
    first, failed = None, []
    for shift in (0, 1):
        for kind in ("tight", "wide", "slice", "odd-wide"):
            x, _ = _rgb_x(xv, dt, shift)
            A = Alloc({"lddy": kind})
            dy, lddy = A.inp("lddy", dyv, adt)
            dw, parent = R.view_of(3.0, (3, 3, 3, cout), cout, 0, None, torch.float32, "cuda")
            ws.fill_(NAN)
            ops.conv2d_wgrad(x, None, 0, x.shape[-1], 0, dy, lddy, dw, n, h, h, 3, kpad, cout, 3, 2, 0, ws)
            torch.cuda.synchronize()
            kern, got = ops.last_kernel(), _cpu(dw)
            try:
                assert kern.startswith("conv3x3s2_rgb_wgrad_kernel<"), kern          # lddy a multiple of 16 bytes, dy and x 16-byte aligned: the streaming kernel
                assert R.outside_untouched(parent, (3, 3, 3, cout), cout, 0, None, 3.0)
                assert rel_l2(host(got), dref) < 1e-5, rel_l2(host(got), dref)           # (test_rgb_gpu.py: fp32 products of exactly representable operands)
                first = got if first is None else first
                assert torch.equal(got, first), "not bit-equal to the tight run"             # fixed summation order
                print(f"x+{shift} lddy-{kind}: {kern} {rel_l2(host(got), dref):.3e}")
            except AssertionError as e:
                failed.append((shift, kind, kern, str(e)[:200]))
    assert not failed, failed
