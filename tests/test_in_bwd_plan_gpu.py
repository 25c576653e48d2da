"""Which form shm_in_bwd / shm_in_bwd_rank1 take for a request (csrc/instnorm_bwd.hip: in_bwd_plan), and sample chunking ("elem.chunk_mb").

The rules the table below is written from (include/shmgan_hip.h at shm_in_bwd's fused_scratch, and the knobs of csrc/common.h):
  * one pass needs dtype bf16 (not the rank-1 form), the scratch of in_bwd_fused_doubles() elements, "elem.fused_bwd" = 1, c in {8, 16, 32} or a
    multiple of 64 (barrier groups of CB = min(c, 64) channels) and 8-aligned pitches; every other call runs reduce + apply;
  * g and a held (in_bwd_fused8_kernel<pooled>): h * w in whole slices of 16384 / CB pixels, at most "elem.fused_max_slices" (256) per group; the
    pooled form needs CB = 64 and whole tiles of (256 / Wt) rows x Wt = min(w, 128) columns;
  * g held (in_bwd_fusedg_kernel): no pooled gradient, whole slices of 32768 / CB pixels; taken automatically from 256 of the 16384 / CB-pixel
    slices per group on, or where "elem.fused_hold" = 2 forces it ("elem.fused_hold" = 1 excludes it); "elem.fused_gvariant" picks <2, 2, 4> or <8, 8, 3>;
  * twice a group's blocks must fit the device (every group here has at most 256 blocks: a whole MI355X holds 768 - 1024);
  * two passes: the reduce pass is in_bwd_reduce8_kernel for bf16 activations with c a multiple of 8, in_bwd_reduce_kernel otherwise.
  * SHM_BF16_GF32 (bf16 a and dz, fp32 g and g2 -- GF32 below): the one-pass forms require `q.dtype == SHM_BF16`, so every request runs reduce + apply;
    `wide8` includes the mode, so the reduce pass is in_bwd_reduce8_kernel where c is a multiple of 8.
Every row also checks the result against float64, that `red` is zero on return and that the scratch is zero behind its partial rows.

Sample chunking: with "elem.chunk_mb" = 1 the two passes run chunk by chunk over samples whose tensors fit 1 MiB; the results are those of one
chunk ("elem.chunk_mb" = 0) -- dz to the bound tests/test_ops_gpu.py holds shm_in_bwd to (the sums are float64 atomics: no bit equality), the
bias gradient and the per-sample dz sums against the float64 restatement.
"""
import numpy as np
import pytest
import torch

import elem_bound_ref as eb

pytestmark = pytest.mark.gpu
BF, F32 = torch.bfloat16, torch.float32
GF32 = "gf32"               # a row's dtype: bf16 activations (a, dz) with the gradient signal (g, g2) in fp32, SHM_BF16_GF32
TOL = 1e-5                  # tests/test_ops_gpu.py: one fp32 InstanceNorm op against float64
TOL_BF16 = 4e-3             # tests/test_in_bwd_fused_gpu.py: bf16 output rounding
R8 = "in_bwd_reduce8_kernel + in_bwd_apply_kernel"
R4 = "in_bwd_reduce_kernel + in_bwd_apply_kernel"
F8, F8P = "in_bwd_fused8_kernel<false>", "in_bwd_fused8_kernel<true>"
FG0, FG1 = "in_bwd_fusedg_kernel<2, 2, 4>", "in_bwd_fusedg_kernel<8, 8, 3>"


def _ops():
    from shmgan_amd import ops
    return ops


@pytest.fixture(autouse=True)
def _reset_tuning():
    yield
    _ops().set_tuning("reset", 0)


def _operands(seed, dt, n, h, w, c, pool=False, rank1=False):
    ops = _ops()
    rng = np.random.default_rng(seed)
    dt, gdt = (BF, F32) if dt == GF32 else (dt, dt)
    a = torch.from_numpy((rng.standard_normal((n, h, w, c)) * rng.uniform(0.5, 2.0, (n, 1, 1, c)) + rng.uniform(-1, 1, (n, 1, 1, c))).astype(np.float32)).cuda().to(dt)
    o = {"a": a, "g": None, "g2": None, "hdz": None, "hw": None}
    if rank1:
        o["hdz"] = torch.from_numpy(rng.standard_normal((n, h, w)).astype(np.float32)).cuda()
        o["hw"] = torch.from_numpy(rng.standard_normal(c).astype(np.float32)).cuda()
    else:
        o["g"] = torch.from_numpy(rng.standard_normal((n, h, w, c)).astype(np.float32)).cuda().to(gdt)
        if pool:
            o["g2"] = torch.from_numpy(rng.standard_normal((n, h // 2, w // 2, c)).astype(np.float32)).cuda().to(gdt)
    o["stats"] = torch.zeros(n * c * 2, dtype=torch.float64, device="cuda")
    ops.in_stats(a, c, o["stats"], n, h * w, c, 1e-6)
    return o


def _reference(o, n, c, slope=0.2):
    """float64: xh = (a - mean) * inv; d = inv * (g - mean(g) - xh * mean(g * xh)); dz = d * lrelu'(a).  Returns dz and its per-sample channel sums."""
    A = o["a"].double()
    if o["hdz"] is not None:
        G = o["hdz"].double().unsqueeze(-1) * o["hw"].double()
    else:
        G = o["g"].double()
        if o["g2"] is not None:
            G = G + 0.25 * o["g2"].double().repeat_interleave(2, 1).repeat_interleave(2, 2)
    st = o["stats"].view(n, c, 2)
    mean, inv = st[:, :, 0].view(n, 1, 1, c), st[:, :, 1].view(n, 1, 1, c)
    xh = (A - mean) * inv
    d = inv * (G - G.mean((1, 2), keepdim=True) - xh * (G * xh).mean((1, 2), keepdim=True))
    dz = torch.where(A > 0, d, d * slope)
    return dz, dz.sum((1, 2))


def _run(o, n, h, w, c, scratch=None, sums=False):
    ops = _ops()
    a = o["a"]
    dz = torch.full_like(a, 9.0)
    db = torch.zeros(c, dtype=torch.float64, device="cuda")
    keep = torch.full((n, c), 9.0, dtype=torch.float64, device="cuda") if sums else None
    red = torch.zeros(n * c * 3, dtype=torch.float64, device="cuda")
    if o["hdz"] is not None:
        ops.in_bwd_rank1(o["hdz"], o["hw"], a, c, o["stats"], red, dz, c, db, n, h, w, c, 0.2, dz_sums=keep)
    else:
        g2 = o["g2"]
        ops.in_bwd(o["g"], c, g2, c if g2 is not None else 0, a, c, o["stats"], red, dz, c, db, n, h, w, c, 0.2, fused=scratch, dz_sums=keep)
    kern = ops.last_kernel()
    torch.cuda.synchronize()
    assert float(red.abs().max()) == 0.0
    return dz, db, keep, kern


def _hold(o, n, c, dz, db, keep, dt, kern):
    """elem_bound_ref.py: dz element by element, the bias gradient and the per-sample dz sums per channel, against the float64 value of the
    device's own expression (mean and inv as the kernels read them from `stats`)"""
    out = "f32" if dt == F32 else "bf16"
    worst = eb.hold_in_bwd([(dz, db, keep, kern)], o["a"], o["stats"], o["g"], o["g2"], o["hdz"], o["hw"], 0.2, out)
    fam = "in_bwd " + (GF32 + " " if dt == GF32 else "") + ("rank-1 " if o["hdz"] is not None else "") + kern.replace("in_bwd_", "").replace("_kernel", "").split("<")[0]
    eb.note(fam, out, worst[kern])


def _rel(x, ref):
    return float((x.double() - ref).norm() / ref.norm())


# (id, dtype, n, h, w, c, pooled, rank-1, knobs, scratch: "full" / "short" (one double less) / None, expected shm_last_kernel())
TABLE = [
    ("fused8-one-block", BF, 2, 16, 16, 64, False, False, {}, "full", F8),
    ("fused8-two-groups", BF, 2, 16, 16, 128, False, False, {}, "full", F8),
    ("fused8-2048-pixel-slice", BF, 1, 32, 64, 8, False, False, {}, "full", F8),
    ("fused8-pooled", BF, 2, 16, 16, 64, True, False, {}, "full", F8P),
    ("fusedg-forced-v0", BF, 2, 16, 32, 64, False, False, {"elem.fused_hold": 2, "elem.fused_gvariant": 0}, "full", FG0),
    ("fusedg-forced-v1", BF, 2, 16, 32, 64, False, False, {"elem.fused_hold": 2, "elem.fused_gvariant": 1}, "full", FG1),
    ("fusedg-forced-pooled", BF, 2, 16, 32, 64, True, False, {"elem.fused_hold": 2, "elem.fused_gvariant": 0}, "full", R8),
    ("fusedg-automatic", BF, 1, 256, 256, 64, False, False, {}, "full", FG0),
    ("fusedg-automatic-hold1", BF, 1, 256, 256, 64, False, False, {"elem.fused_hold": 1}, "full", F8),
    ("two-pass-ragged", BF, 2, 16, 18, 64, False, False, {}, "full", R8),
    ("two-pass-c24", BF, 2, 16, 16, 24, False, False, {}, "full", R8),
    ("two-pass-no-scratch", BF, 2, 16, 16, 64, False, False, {}, None, R8),
    ("two-pass-short-scratch", BF, 2, 16, 16, 64, False, False, {}, "short", R8),
    ("two-pass-fused-off", BF, 2, 16, 16, 64, False, False, {"elem.fused_bwd": 0}, "full", R8),
    ("two-pass-max-slices", BF, 2, 16, 32, 64, False, False, {"elem.fused_max_slices": 1}, "full", R8),
    ("two-pass-pooled-c32", BF, 2, 16, 16, 32, True, False, {}, "full", R8),
    ("two-pass-bf16-rank1", BF, 2, 16, 16, 64, False, True, {}, None, R8),
    ("two-pass-bf16-c12", BF, 2, 16, 16, 12, False, False, {}, "full", R4),
    ("two-pass-f32", F32, 2, 16, 16, 64, False, False, {}, "full", R4),
    ("two-pass-f32-pooled", F32, 2, 16, 16, 64, True, False, {}, "full", R4),
    ("two-pass-f32-rank1", F32, 2, 16, 16, 64, False, True, {}, None, R4),
    # SHM_BF16_GF32 on the requests of "fused8-2048-pixel-slice", "fused8-pooled" and "fusedg-forced-v0" (the smallest of each one-pass form above):
    # none reaches a one-pass form
    ("gf32-fused8-request", GF32, 1, 32, 64, 8, False, False, {}, "full", R8),
    ("gf32-fused8-pooled-request", GF32, 2, 16, 16, 64, True, False, {}, "full", R8),
    ("gf32-fusedg-request", GF32, 2, 16, 32, 64, False, False, {"elem.fused_hold": 2, "elem.fused_gvariant": 0}, "full", R8),
    # c = 48 has no whole barrier groups (neither a power of two below 64 nor a multiple of 64): two passes in every mode
    ("two-pass-bf16-c48", BF, 2, 16, 16, 48, False, False, {}, "full", R8),
    ("two-pass-f32-c48", F32, 2, 16, 16, 48, False, False, {}, "full", R4),
    ("gf32-c48", GF32, 2, 16, 16, 48, False, False, {}, "full", R8),
    ("gf32-c36", GF32, 2, 16, 16, 36, False, False, {}, "full", R4),          # not a multiple of 8: four channels per thread
]


@pytest.mark.parametrize("dt,n,h,w,c,pool,rank1,knobs,scr,want", [r[1:] for r in TABLE], ids=[r[0] for r in TABLE])
def test_dispatch_table(dt, n, h, w, c, pool, rank1, knobs, scr, want):
    ops = _ops()
    o = _operands(31 + h + w + c, dt, n, h, w, c, pool, rank1)
    need = ops.in_bwd_fused_doubles(n, h * w, c)
    scratch = None if scr is None else torch.zeros(need - (1 if scr == "short" else 0), dtype=torch.float64, device="cuda")
    for key, val in knobs.items():
        ops.set_tuning(key, val)
    dz, db, keep, kern = _run(o, n, h, w, c, scratch, sums=dt == GF32)
    assert kern == want, kern
    if scratch is not None:
        # zero on return: behind the per-block partial rows of a one-pass launch (tests/test_in_bwd_fused_gpu.py: _clean); all of it otherwise
        rows = (n * (h * w * min(c, 64) // 16384) * 3 * c + 1) // 2 if "fused" in want else 0
        tail = scratch[rows:]
        assert torch.equal(tail.view(torch.int64), torch.zeros_like(tail).view(torch.int64))
    zr, sr = _reference(o, n, c)
    tol = TOL if dt == F32 else TOL_BF16
    assert _rel(dz, zr) < tol, _rel(dz, zr)
    assert float((db - sr.sum(0)).abs().max()) <= tol * float(zr.abs().sum((0, 1, 2)).max())
    _hold(o, n, c, dz, db, keep, dt, kern)
    if keep is not None:          # the per-sample dz sums, on the scale of their summands like the bias gradient; and the same call without them (the folding apply pass)
        assert float((keep - sr).abs().max()) <= tol * float(zr.abs().sum((1, 2)).max())
        dz1, db1, _, kern1 = _run(o, n, h, w, c, scratch)
        assert kern1 == want and _rel(dz1, zr) < tol and float((db1 - sr.sum(0)).abs().max()) <= tol * float(zr.abs().sum((0, 1, 2)).max())
        _hold(o, n, c, dz1, db1, None, dt, kern1)


# 32 x 32 x 64 maps: a plain sample is 512 KiB in fp32 and 256 KiB in bf16, a pooled fp32 sample 576 KiB.  Chunks of 1 MiB: 2 + 1 samples (fp32),
# 1 + 1 + 1 (fp32 pooled), 3 (bf16: one chunk), 4 + 1 (bf16, n = 5); SHM_BF16_GF32: 128 KiB of a + 256 KiB of g, 2 + 1
@pytest.mark.parametrize("dt,n,pool", [(F32, 3, False), (F32, 3, True), (BF, 3, False), (BF, 5, False), (GF32, 3, False)],
                         ids=["f32-2+1", "f32-pooled-1+1+1", "bf16-3", "bf16-4+1", "gf32-2+1"])
def test_sample_chunks_give_the_results_of_one_chunk(dt, n, pool):
    ops = _ops()
    h = w = 32
    c = 64
    o = _operands(5 + n, dt, n, h, w, c, pool)
    ops.set_tuning("elem.chunk_mb", 0)
    z0, b0, s0, k0 = _run(o, n, h, w, c, sums=True)
    ops.set_tuning("elem.chunk_mb", 1)
    z1, b1, s1, k1 = _run(o, n, h, w, c, sums=True)
    assert k0 == k1 == (R4 if dt == F32 else R8), (k0, k1)
    zr, sr = _reference(o, n, c)
    for z, b, s in ((z0, b0, s0), (z1, b1, s1)):
        print(f"dz vs f64 {_rel(z, zr):.3e}  dbias {_rel(b, sr.sum(0)):.3e}  dz_sums {_rel(s, sr):.3e}")
    print(f"dz chunked vs whole {_rel(z1, z0.double()):.3e}")
    assert _rel(z1, z0.double()) < TOL
    assert _rel(b1, sr.sum(0)) < TOL and _rel(s1, sr) < TOL
    assert _rel(b0, sr.sum(0)) < TOL and _rel(s0, sr) < TOL
