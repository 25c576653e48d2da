"""CPU checks of the cases and references behind test_heads_edges_gpu.py (heads_edge_ref.py): every case is in the branch it claims -- sizes
against the grid caps, pixels per block, unroll factors and the 16-sample stride, restated in heads_edge_ref.py with their source lines --
the float64 references agree with torch.autograd, the same arithmetic in float32 passes every bound in use with a factor of three to
spare, and the comparison has teeth: a dropped partial wave, samples >= 16 skipped, an overwritten dx, a grid-stride loop that stops after
its first pass and the slope on the wrong side of y == 0 all fail it."""
from pathlib import Path

import numpy as np
import torch
import torch.nn.functional as F

import heads_edge_ref as R

CSRC = Path(__file__).resolve().parent.parent / "shmgan_amd" / "csrc"
SPARE = 3.0
f32, f64 = np.float32, np.float64


def _g(t, *wrt, seed=0):
    """gradients of <t, g> for a fixed random g; returns (g, grads)"""
    g = torch.from_numpy(np.random.default_rng(seed).standard_normal(tuple(t.shape)))
    return g.numpy(), [v.numpy() for v in torch.autograd.grad(t, wrt, g)]


# ----------------------------------------------------------------------------------------------------------------- the restated constants
def test_constants_are_the_sources():
    """The caps, unroll factors and strides restated in heads_edge_ref.py still stand in the kernel sources, as text.  A failure here after a
    kernel file was reformatted or a name changed is no regression of the kernels: re-read the cap at the source line the constant's comment
    names, update heads_edge_ref.py (and the snippet below) to it, and check that the case tables still reach past it."""
    heads, spec, elem, gs, eh = ((CSRC / n).read_text() for n in ("heads.hip", "specseg.hip", "elem.hip", "grad_sums.hip", "elem.h"))
    assert f"shm_grid_cap(npix, 256 / (c / 4), {R.HEAD_FWD_CAP})" in heads and f"{R.HEAD_FWD_CAP} / batch" in heads
    assert f"shm_grid_cap(npix, 256 / l, {R.HEAD_FWD_CAP})" in spec
    assert f"shm_grid_cap(npix, 256 / (c / 4) * {R.HEAD_BWD_ITERS}, {R.HEAD_BWD_CAP})" in heads and f"{R.HEAD_BWD_CAP} / batch" in heads
    assert f"(long)PP * {R.HEAD_BWD_ITERS}" in heads
    assert f"constexpr int U = {R.HEAD_BWD_U};" in heads and "PP = 256 / lanes_c" in eh and "lanes_c = c >> 2" in eh
    assert f"n += {R.PATCH_SAMPLE_STRIDE})" in heads and f"blockIdx.y * {R.PATCH_CH_PER_BLOCK}" in heads
    assert f"n + {R.DENSE_UNROLL} <= batch" in heads and "48 * 1024" in heads and R.DENSE_LDS_BYTES == 48 * 1024
    assert "nout == 5 && (k & 3) == 0" in heads
    assert f"pix_chunks((long)npix, 1, c, {R.LRELU_BLOCKS})" in gs and "U = sizeof(T) == 2 ? 8 : 4" in gs and "blocks > 4096 ? 8 : 16" in eh
    assert spec.count("shm_grid_cap(total, 256, 8192)") == 2 and "shm_grid_cap(npix * (c / 4), 256, 8192)" in spec and R.SPEC_GRID == 8192 * 256
    assert "shm_grid_cap(n, 256, 256)" in spec and R.SPEC_LOSS_GRID == 256 * 256
    assert "shm_grid_cap(n, 256, 4096)" in elem and R.CAST_GRID == 4096 * 256
    assert "if (g > (size_t)cap) g = cap;" in (CSRC / "common.h").read_text()


# ------------------------------------------------------------------------------------------------------------------------------ heads
def test_head_cases_are_in_their_branch():
    assert [R.lanes(c) for c in R.HEAD_C] == [1, 2, 16, 64] and [R.pp(c) for c in R.HEAD_C] == [256, 128, 16, 4]
    assert R.pix_per_wave(4) == 64 and R.pix_per_wave(256) == 1          # one lane per pixel (no shuffle step); a whole wave per pixel
    for c in R.HEAD_C:
        P, n = R.pp(c), R.head_npix(c)
        assert n == (1, P - 1, P + 1, 5 * P + 3) and all(v % 2 for v in n)
        assert R.head_grid(n[1], c) == 1 and R.head_grid(n[2], c) == 2 and R.head_grid(n[3], c, bwd=True) == 1
        assert R.head_trips(n[2], c, bwd=True) == (0, 2) and R.head_trips(n[3], c, bwd=True) == (1, 2)
        if R.pix_per_wave(c) > 1:
            assert all(v % R.pix_per_wave(c) for v in n)                   # the last wave is ragged
        for hw in n:                                                       # the folded form: three samples, nowhere near the cap
            assert R.head_grid(hw, c, R.HEAD_IN_BATCH) == R.head_grid(hw, c) and R.head_grid(hw, c, R.HEAD_IN_BATCH, True) == 1
    c, B = R.HEAD_OVER_C, R.HEAD_IN_BATCH
    assert R.HEAD_FWD_OVER == 8192 * 4 + 5 and R.HEAD_BWD_OVER == 4096 * 4 * 8 + 5
    assert R.head_grid(R.HEAD_FWD_OVER, c) == R.HEAD_FWD_CAP < -(-R.HEAD_FWD_OVER // R.pp(c)) and R.head_trips(R.HEAD_FWD_OVER, c) == (0, 2)
    assert R.head_grid(R.HEAD_BWD_OVER, c, bwd=True) == R.HEAD_BWD_CAP and R.head_trips(R.HEAD_BWD_OVER, c, bwd=True) == (2, 1)
    # the folded form at the same totals: cap / batch binds
    assert abs(B * R.HEAD_IN_FWD_OVER_HW - R.HEAD_FWD_OVER) < B and abs(B * R.HEAD_IN_BWD_OVER_HW - R.HEAD_BWD_OVER) < B
    assert R.HEAD_IN_FWD_OVER_HW % 2 and R.HEAD_IN_BWD_OVER_HW % 2
    assert R.head_grid(R.HEAD_IN_FWD_OVER_HW, c, B) == R.HEAD_FWD_CAP // B < -(-R.HEAD_IN_FWD_OVER_HW // R.pp(c))
    assert R.head_trips(R.HEAD_IN_FWD_OVER_HW, c, B) == (0, 2)
    assert R.head_grid(R.HEAD_IN_BWD_OVER_HW, c, B, True) == R.HEAD_BWD_CAP // B < -(-R.HEAD_IN_BWD_OVER_HW // (R.pp(c) * R.HEAD_BWD_ITERS))
    assert R.head_trips(R.HEAD_IN_BWD_OVER_HW, c, B, True) == (2, 1)
    k = R.saturate_rows(R.head_case(8, 9, "f32"))
    z = (k.x * k.w).sum(-1)
    assert (np.abs(np.abs(z) - 100) < 1e-3).all() and (z > 0).any() and (z < 0).any()
    y = R.sigmoid_head_ref(k.x, k.w, None)
    assert np.isfinite(y).all() and ((y < 1e-6) | (y > 1 - 1e-6)).all()
    assert set(R.sigmoid_head_ref(k.x, k.w, None, f32).tolist()) == {0.0, 1.0}          # what a float evaluation gives: exactly 0 or 1


def test_head_references_against_autograd():
    for c, npix, batch in ((8, 9, 1), (64, 7, 3)):
        k = R.head_case(c, npix, "f32", batch)
        x, w, b = (R.t64(v).requires_grad_(True) for v in (k.x, k.w, [k.b]))
        mean, inv = R.t64(k.mean), R.t64(k.inv)
        for norm in (False, True):
            xh = ((x.view(batch, npix, c) - mean[:, None]) * inv[:, None] + R.t64(k.beta)).view(-1, c) if norm else x
            xh_np = R.head_norm(k.x, k.mean, k.inv, k.beta) if norm else k.x
            assert np.allclose(xh_np, xh.detach().numpy(), rtol=1e-13)
            yt = F.leaky_relu((xh * w).sum(-1) + b, R.SLOPE)
            y = R.head_fwd_ref(xh_np, k.w, k.b)
            assert np.allclose(y, yt.detach().numpy(), rtol=1e-12)
            xl = xh.detach().requires_grad_(True)          # dx is the gradient at the NORMALISED activation
            yl = F.leaky_relu((xl * w).sum(-1) + b, R.SLOPE)
            g, (rdx, rdw, rdb) = _g(yl, xl, w, b)
            dz, dx, dw, db = R.head_bwd_ref(xh_np, k.w, y, g)
            assert np.allclose(dx, rdx, rtol=1e-12) and np.allclose(dw, rdw, rtol=1e-11) and np.allclose(db, rdb[0], rtol=1e-11)
            assert np.allclose(dz, dx[:, 0] / k.w[0], rtol=1e-12)
        s = R.sigmoid_head_ref(k.x, k.w, k.b)
        assert np.allclose(s, torch.sigmoid((x * w).sum(-1) + b).detach().numpy(), rtol=1e-12)
        assert np.array_equal(R.head_fwd_ref(k.x, k.w, None), R.head_fwd_ref(k.x, k.w, 0.0))


# ------------------------------------------------------------------------------------------------------------------------------ patch
def test_patch_cases_and_reference():
    assert {b for b, *_ in R.PATCH_CASES} >= {1, 17, 33} and 17 > R.PATCH_SAMPLE_STRIDE and 33 > 2 * R.PATCH_SAMPLE_STRIDE
    assert {c for *_, c in R.PATCH_CASES} == {4, 68, 256} and 68 % R.PATCH_CH_PER_BLOCK == 4 and -(-68 // R.PATCH_CH_PER_BLOCK) == 2
    assert {(h, w) for _, h, w, _ in R.PATCH_CASES} >= {(2, 3), (1, 5), (5, 1), (1, 1)}
    for batch, h, w, c in ((3, 2, 3, 8), (2, 1, 5, 4), (2, 5, 1, 4), (1, 1, 1, 4)):
        k = R.patch_case(batch, h, w, c, "f32")
        xt = R.t64(k.x).permute(0, 3, 1, 2).requires_grad_(True)
        wo = R.t64(k.wt).view(3, 3, c, 1).permute(3, 2, 0, 1).contiguous().requires_grad_(True)
        yt = F.leaky_relu(F.conv2d(xt, wo, padding=1), R.SLOPE)[:, 0]
        y = R.patch_fwd_ref(k.x, k.wt)
        assert np.allclose(y, yt.detach().numpy(), rtol=1e-11, atol=1e-14)
        g, (rdx, rdw) = _g(yt, xt, wo)
        dz, dx, dw = R.patch_bwd_ref(k.x, k.wt, y, g)
        assert np.allclose(dx, rdx.transpose(0, 2, 3, 1), rtol=1e-11, atol=1e-14)
        assert np.allclose(dw, rdw[0].transpose(1, 2, 0).reshape(9, c), rtol=1e-11, atol=1e-14)
        assert np.array_equal(dz, np.where(y > 0, g, R.SLOPE * g))


# ------------------------------------------------------------------------------------------------------------------------------ dense
def test_dense_cases_and_reference():
    fast = {(n, k, o): R.dense_fast_path(n, k, o, 4) for n in R.DENSE_NOUT for k in R.DENSE_K for o in (0, 1)}
    assert [key for key, v in fast.items() if v] == [(5, 1020, 0), (5, 2052, 0)]
    assert not fast[(5, 1022, 0)] and not fast[(8, 1020, 0)] and not fast[(5, 1020, 1)]          # forced by k % 4, by nout, by the offset
    assert all(R.dense_fast_path(5, 1020, o, 2) == (o == 0) for o in (0, 1))                      # bf16: 8-byte rows
    assert 1020 // 4 < 256 and 3 < 256 < 2052 // 4                                                # idle lanes; more than one trip
    assert [b // R.DENSE_UNROLL for b in R.DENSE_BATCH] == [0, 1, 1] and [b % R.DENSE_UNROLL for b in R.DENSE_BATCH] == [1, 0, 3]
    b, n = R.DENSE_REFUSED
    assert b * n * 4 > R.DENSE_LDS_BYTES >= (b - 1) * n * 4
    d = R.dense_case(4, 1022, 5, "f32")
    xt, wt = R.t64(d.x).requires_grad_(True), R.t64(d.w).requires_grad_(True)
    yt = xt @ wt
    assert np.allclose(R.dense_fwd_ref(d.x, d.w), yt.detach().numpy(), rtol=1e-11)
    g, (rdx, rdw) = _g(yt, xt, wt)
    dx, dw = R.dense_bwd_ref(d.x, d.w, g, d.dx0)
    assert np.allclose(dx - d.dx0, rdx, rtol=1e-9) and np.allclose(dw, rdw, rtol=1e-11) and np.abs(d.dx0).min() > 0


# ------------------------------------------------------------------------------------------------------------------------------ lrelu
def test_lrelu_cases_and_reference():
    assert [R.lanes(c) for c in R.LRELU_C] == [1, 12, 256] and [R.pp(c) for c in R.LRELU_C] == [256, 21, 1]
    assert 256 - R.pp(48) * R.lanes(48) == 4                               # four inactive threads
    for dt in R.DTYPES:
        U = R.LRELU_U[dt]
        for c in R.LRELU_C:
            n = R.lrelu_npix(c, dt)
            assert n == (1, R.pp(c) * U + 1, 4099)
            assert R.lrelu_chunk(n[1], c) == n[1]                          # one block: the main loop once, one pixel in the tail loop
            ch = R.lrelu_chunk(n[2], c)
            last = n[2] - (-(-n[2] // ch) - 1) * ch
            assert ch % (U * R.pp(c)) and last % (U * R.pp(c))             # neither a whole chunk nor the last one ends on U * PP
        assert R.lrelu_chunk(4099, 1024) == 17 and -(-4099 // 17) == 242 > R.LRELU_SLOTS          # more blocks than slots
        k = R.lrelu_case(48, 5, dt)
        assert k.special == [(0, 0), (0, 1), (0, 2), (4, 0), (4, 1), (4, 2)]
        z = k.y[[0, 4], :3]
        assert (z[:, :2] == 0).all() and not np.signbit(z[:, 0]).any() and np.signbit(z[:, 1]).all() and (z[:, 2] == R.SUBNORMAL[dt]).all()
        assert np.array_equal(R.act(k.y, dt), k.y) and 0 < R.SUBNORMAL[dt] < 2.0 ** -126          # survives the device's type, subnormal in it
        dz, db = R.lrelu_bwd_ref(k.y, k.dy)
        yt = R.t64(k.y).requires_grad_(True)
        assert np.array_equal(dz[0, :3], [R.SLOPE * k.dy[0, 0], R.SLOPE * k.dy[0, 1], k.dy[0, 2]])
        far = np.abs(k.y) > 0                                              # autograd agrees away from the kink
        rg = torch.autograd.grad(F.leaky_relu(yt, R.SLOPE), yt, R.t64(k.dy))[0].numpy()
        assert np.allclose(dz[far], rg[far], rtol=1e-13) and np.allclose(db, dz.sum(0))
        assert R.lrelu_special_ok(dz, k, R.gtol(dt))


# ---------------------------------------------------------------------------------------------------------------------------- SpecSeg
def test_specseg_cases_and_references():
    b, h, w, c = R.SPEC_OVER_MAP
    vec = b * h * w * (c // 4)
    assert c == 16 and h != w and vec > R.SPEC_GRID + 77 and (vec - R.SPEC_GRID) % 256 and (vec - R.SPEC_GRID) % 64 and vec < 2 * R.SPEC_GRID
    assert (R.SPEC_GRID + 77) % (c // 4)                                   # four vectors a pixel: the count is a multiple of four, 8192 * 256 + 77 is not
    assert R.SPEC_PITCH_MAP[1:3] == (6, 10)
    assert {nc for nc, _ in R.PACK_CASES} == {1, 3} and {ld for _, ld in R.PACK_CASES} == {4, 16} and R.PACK_SRC[1] > 0
    assert R.PACK_SRC[1] + 3 <= R.PACK_SRC[0] and R.PACK_NPIX[1] == R.SPEC_GRID + 77
    B, npix = R.SPEC_LOSS_SHAPES[1]
    assert B == 3 and (256 * 256 + 37) % 3 and B * npix == 256 * 256 + 38 > R.SPEC_LOSS_GRID and (B * npix - R.SPEC_LOSS_GRID) % 64
    k = R.bn_case(12, 8)
    ref = F.batch_norm(R.t64(k.a), R.t64(k.mean), R.t64(k.var), R.t64(k.gamma), R.t64(k.beta), False, 0.0, R.BN_EPS).numpy()
    assert np.allclose(R.bn_ref(k.a, k.gamma, k.beta, k.mean, k.var), ref, rtol=1e-12)
    x = np.random.default_rng(1).standard_normal((2, 6, 10, 8))
    assert np.array_equal(R.maxpool_ref(x), F.max_pool2d(R.t64(x).permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1).numpy())
    src = np.arange(35.0).reshape(7, 5)
    assert np.array_equal(R.pack_ref(src, 1, 3, 16)[:, :3], src[:, 1:4]) and not R.pack_ref(src, 1, 3, 16)[:, 3:].any()
    s = R.spec_case(*R.SPEC_LOSS_SHAPES[0])
    assert set(np.unique(s.mask)) == {0.0, 1.0} and (s.mask[-1, -64:] == 1).all()
    yuv = [np.concatenate([s.cyc_y[j * s.batch:(j + 1) * s.batch], s.cbcr], 3) for j in range(5)]
    own = [((s.mask * (yuv[j] - s.ds[j])) ** 2).sum() for j in range(5)]
    assert np.allclose(R.spec_loss_ref(s), own, rtol=1e-12) and len({round(v, 6) for v in own}) == 5


# ------------------------------------------------------------------------------------------------------------------------------ casts
def test_cast_inputs_and_references():
    assert R.CAST_SIZES == (1, 255, 4096 * 256 + 77)
    x = R.CAST_BITS.view(np.float32)
    bits, nan = R.cast_ref_bits(x)
    want = dict(zip(R.CAST_BITS.tolist(), bits.view(np.uint16).tolist()))
    assert want[0x3F818000] == 0x3F82 and want[0x3F808000] == 0x3F80 and want[0x3F808001] == 0x3F81 and want[0x3F807FFF] == 0x3F80
    assert want[0x00000000] == 0x0000 and want[0x80000000] == 0x8000 and want[0x00000001] == 0x0000 and want[0x80000001] == 0x8000
    assert want[0x007FFFFF] == 0x0080 and want[0x00008000] == 0x0000 and want[0x00018000] == 0x0002          # subnormals: RNE, never flushed
    assert want[0x7F7FFFFF] == 0x7F80 and want[0xFF7FFFFF] == 0xFF80 and want[0x7F7F0000] == 0x7F7F
    assert nan.tolist() == [False] * 18 + [True, True]
    for n in R.CAST_SIZES:
        v = R.cast_input(n)
        assert v.dtype == np.float32 and v.size == n and v.view(np.uint32)[0] == 0x3F818000
        if n > 255:
            assert np.array_equal(v[-20:].view(np.uint32), R.CAST_BITS) and np.array_equal(v[:20].view(np.uint32), R.CAST_BITS)
        s, d = R.cvt_input(n)
        r0, r1 = R.cvt_ref(s, d, 0), R.cvt_ref(s, d, 1)
        assert r0.dtype == r1.dtype == np.float32
        if n >= 12:
            assert r0[2] == 0 and 0 < r0[3] < 2.0 ** -126 and np.isinf(r0[4]) and r0[6] == 1 and r0[7] == f32(1 + 2.0 ** -22) and np.isnan(r0[10])
            assert np.array_equal(r1[:8], d[:8] + r0[:8])
    got = bits.copy()
    assert R.same_bits(got, bits, nan)
    got[18] ^= 1
    assert R.same_bits(got, bits, nan)                                     # a NaN's payload is free
    got[3] ^= 1
    assert not R.same_bits(got, bits, nan)


# ----------------------------------------------------------------------------------------------------- float32 evaluations and teeth
def _pairs():
    """(name, reference in float64, the same in float32) for every comparison the GPU tests bound by rel-L2"""
    out = []
    for c in R.HEAD_C:
        for npix in R.head_npix(c) + ((R.HEAD_FWD_OVER,) if c == R.HEAD_OVER_C else ()):
            k = R.head_case(c, npix, "f32", R.HEAD_IN_BATCH if npix < 10000 else 1)
            for norm in (False, True):
                xs = [R.head_norm(k.x, k.mean, k.inv, k.beta, t) if norm else k.x for t in (f64, f32)]
                ys = [R.head_fwd_ref(x, k.w, k.b, dtype=t) for x, t in zip(xs, (f64, f32))]
                bw = [R.head_bwd_ref(x, k.w, ys[0], k.dy, dtype=t) for x, t in zip(xs, (f64, f32))]
                out += [(f"head c{c} n{npix} norm{norm} {nm}", a, b) for nm, a, b in zip(("y", "dz", "dx", "dw", "db"), (ys[0],) + bw[0], (ys[1],) + bw[1])]
            out.append((f"sigmoid c{c} n{npix}", R.sigmoid_head_ref(k.x, k.w, k.b), R.sigmoid_head_ref(k.x, k.w, k.b, f32)))
    for case in R.PATCH_CASES:
        k = R.patch_case(*case, "f32")
        y = R.patch_fwd_ref(k.x, k.wt)
        bw = [R.patch_bwd_ref(k.x, k.wt, y, k.dy, dtype=t) for t in (f64, f32)]
        out += [(f"patch {case} {nm}", a, b) for nm, a, b in zip(("y", "dz", "dx", "dw"), (y,) + bw[0], (R.patch_fwd_ref(k.x, k.wt, dtype=f32),) + bw[1])]
    for batch in R.DENSE_BATCH:
        for kk in R.DENSE_K:
            for nout in R.DENSE_NOUT:
                d = R.dense_case(batch, kk, nout, "f32")
                bw = [R.dense_bwd_ref(d.x, d.w, d.dy, d.dx0, t) for t in (f64, f32)]
                out += [(f"dense {batch} {kk} {nout} {nm}", a, b)
                        for nm, a, b in zip(("y", "dx", "dw"), (R.dense_fwd_ref(d.x, d.w),) + bw[0], (R.dense_fwd_ref(d.x, d.w, f32),) + bw[1])]
    for c in R.LRELU_C:
        for npix in R.lrelu_npix(c, "f32"):
            k = R.lrelu_case(c, npix, "f32")
            a, b = R.lrelu_bwd_ref(k.y, k.dy), R.lrelu_bwd_ref(k.y, k.dy, dtype=f32)
            out += [(f"lrelu c{c} n{npix} dz", a[0], b[0]), (f"lrelu c{c} n{npix} db", a[1], b[1])]
    k = R.bn_case(120, 8)
    out.append(("bn", R.bn_ref(k.a, k.gamma, k.beta, k.mean, k.var), R.bn_ref(k.a, k.gamma, k.beta, k.mean, k.var, dtype=f32)))
    for shape in R.SPEC_LOSS_SHAPES:
        s = R.spec_case(*shape)
        out.append((f"spec_loss {shape}", R.spec_loss_ref(s), R.spec_loss_ref(s, torch.float32)))
    return out


def test_float32_evaluations_pass_the_bounds_with_room():
    """the tightest bound in use is F32_TOL (BF16_TOL32 and BF16_TOL are wider)"""
    assert R.F32_TOL < R.BF16_TOL32 < R.BF16_TOL
    worst = ("", 0.0)
    for name, ref, low in _pairs():
        e = R.err(low, ref)
        worst = max(worst, (name, e), key=lambda t: t[1])
        assert e * SPARE < R.F32_TOL, (name, e)
    print("worst float32 evaluation:", worst)
    # the spec_loss terms are bounded one by one (relative 1e-5, test_step_gpu.test_spec_loss_kernel)
    for shape in R.SPEC_LOSS_SHAPES:
        s = R.spec_case(*shape)
        assert (np.abs(R.spec_loss_ref(s, torch.float32) / R.spec_loss_ref(s) - 1) * SPARE < R.F32_TOL).all()
    # the sigmoid head is also held to an absolute 1e-6 (test_ops_gpu.test_bn_apply_maxpool_pack_sigmoid's bound)
    for name, ref, low in _pairs():
        if name.startswith("sigmoid"):
            assert np.abs(low - ref).max() * SPARE < 1e-6, name
    # one bf16 rounding of a result passes the bound on bf16-stored results
    k = R.head_case(64, 83, "bf16")
    dx = R.head_bwd_ref(k.x, k.w, R.head_fwd_ref(k.x, k.w, k.b), k.dy)[1]
    assert R.err(R.rb(dx), dx) < R.BF16_TOL and R.err(R.rb(dx), dx) > R.BF16_TOL32


def test_float32_evaluation_of_the_head_backward_past_the_cap():
    """the largest case, on its own so that its arrays (270 MB each in float64) are freed at once: 4096 * 4 * 8 + 5 pixels, plain and as three
    samples of 43693 in the folded form; dw and db are sums over all of them"""
    c = R.HEAD_OVER_C
    for norm in (False, True):
        k = R.head_case(c, R.HEAD_IN_BWD_OVER_HW, "f32", R.HEAD_IN_BATCH) if norm else R.head_case(c, R.HEAD_BWD_OVER, "f32")
        x64 = R.head_norm(k.x, k.mean, k.inv, k.beta) if norm else k.x
        y = R.r32(R.head_fwd_ref(x64, k.w, k.b))
        ref = R.head_bwd_ref(x64, k.w, y, k.dy)
        del x64
        low = R.head_bwd_ref(R.head_norm(k.x, k.mean, k.inv, k.beta, f32) if norm else k.x, k.w, y, k.dy, dtype=f32)
        for nm, a, b in zip(("dz", "dx", "dw", "db"), ref, low):
            e = R.err(b, a)
            print(f"head backward past the cap norm={norm} {nm}: float32 evaluation {e:.3g}")
            assert e * SPARE < R.F32_TOL, (norm, nm, e)
        del ref, low


def test_nonfinite_positions_are_part_of_the_comparison():
    ref = np.array([1.0, np.nan, np.inf, -2.0])
    assert R.err(ref, ref) == 0.0
    for bad in ([1.0, 0.0, np.inf, -2.0], [1.0, np.nan, -np.inf, -2.0], [1.0, np.nan, np.inf, np.nan], [np.inf, np.nan, np.inf, -2.0], [1.0, np.nan, 3e38, -2.0]):
        assert R.err(np.array(bad), ref) == float("inf")
    assert 0 < R.err(np.array([1.0, np.nan, np.inf, -2.001]), ref) < 1e-3


def test_modelled_faults_fail_the_comparison():
    loosest = R.BF16_TOL          # a fault must fail in every dtype: beyond the widest bound
    # a dropped last partial wave: the head's outputs for the pixels of the last, partly filled wave keep the fill of their allocation (~0);
    # past the cap (one pixel a wave): a grid-stride loop that stops after its first pass
    for c in R.HEAD_C:
        for npix in R.head_npix(c)[1:] + ((R.HEAD_FWD_OVER,) if c == R.HEAD_OVER_C else ()):
            k = R.head_case(c, npix, "f32")
            y = R.head_fwd_ref(k.x, k.w, k.b)
            dz, dx, dw, db = R.head_bwd_ref(k.x, k.w, y, k.dy)
            drop = npix - R.HEAD_FWD_CAP * R.pp(c) if npix == R.HEAD_FWD_OVER else max(npix % R.pix_per_wave(c), 1)
            assert 0 < drop < 64
            keep = np.arange(npix) < npix - drop
            assert R.err(np.where(keep, y, 0.0), y) > loosest, (c, npix)
            assert R.err(np.where(keep[:, None], dx, 0.0), dx) > loosest
            if npix == R.HEAD_FWD_OVER:          # the forward's size: the backward kernels do not run at it
                continue
            fdw, fdb = R.head_bwd_ref(k.x[keep], k.w, y[keep], k.dy[keep])[2:]
            assert R.err(fdw, dw) > R.BF16_TOL32 and R.err(fdb, db) > R.BF16_TOL32          # the sums are fp32 / f64 results: their own bound
    # samples >= 16 skipped in the patch weight gradient
    for batch in (17, 33):
        k = R.patch_case(batch, 2, 3, 68, "f32")
        y = R.patch_fwd_ref(k.x, k.wt)
        assert R.err(R.patch_bwd_ref(k.x, k.wt, y, k.dy, samples=slice(0, 16))[2], R.patch_bwd_ref(k.x, k.wt, y, k.dy)[2]) > R.BF16_TOL32
    # dx overwritten instead of accumulated in Dense
    for batch in R.DENSE_BATCH:
        d = R.dense_case(batch, 1020, 5, "f32")
        assert R.err(R.dense_bwd_ref(d.x, d.w, d.dy, d.dx0, accumulate=False)[0], R.dense_bwd_ref(d.x, d.w, d.dy, d.dx0)[0]) > loosest
    # a grid-stride loop that stops after its first pass: bn_apply / maxpool2 / pack (outputs keep their fill), spec_loss (the sums miss the
    # tail), the casts (bit-exact: any element)
    b, h, w, c = R.SPEC_OVER_MAP
    vec = b * h * w * (c // 4)
    ref = np.random.default_rng(3).standard_normal(vec * 4)
    stopped = np.where(np.arange(vec * 4) < R.SPEC_GRID * 4, ref, 0.0)
    assert R.err(stopped, ref) > R.F32_TOL and not np.array_equal(stopped, ref)
    s = R.spec_case(*R.SPEC_LOSS_SHAPES[1])
    full, part = R.spec_loss_ref(s), R.spec_loss_ref(s, pixels=R.SPEC_LOSS_GRID)
    assert (np.abs(part / full - 1) > R.F32_TOL).all()
    x = R.cast_input(R.CAST_SIZES[2])
    bits, nan = R.cast_ref_bits(x)
    stopped = bits.copy()
    stopped[R.CAST_GRID:] = 0
    assert not R.same_bits(stopped, bits, nan)
    # the slope applied to y == 0 the wrong way (y >= 0 keeps dy): caught at the special elements, in every dtype
    for dt in R.DTYPES:
        for c in R.LRELU_C:
            k = R.lrelu_case(c, R.lrelu_npix(c, dt)[1], dt)
            good = R.lrelu_bwd_ref(k.y, k.dy)[0]
            wrong = np.where(k.y >= 0, k.dy, R.SLOPE * k.dy)
            flushed = np.where(k.y > 2.0 ** -126, k.dy, R.SLOPE * k.dy)          # the subnormal taken for zero
            assert R.lrelu_special_ok(R.grad(good, "bf16"), k, R.BF16_TOL) and R.lrelu_special_ok(good, k, R.gtol(dt))
            assert not R.lrelu_special_ok(wrong, k, R.gtol(dt)) and not R.lrelu_special_ok(flushed, k, R.gtol(dt))
