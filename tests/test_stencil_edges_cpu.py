"""CPU checks of the cases and references behind test_stencil_edges_gpu.py (stencil_edge_ref.py): the case table reaches every one of the
eleven stencil forms -- the dispatch restated in stencil_edge_ref.py still stands in dgrad_sum1.hip as text -- and every geometry class in
each kernel and dtype; the float64 references agree with torch.autograd and with plain definitions; the same arithmetic in float32 passes
both stencil conditions with a factor of three to spare, which is where the per-pixel constants come from; every modelled fault fails the
comparison; and the entry points refuse what their contracts exclude before any launch."""
import ctypes as C
from pathlib import Path

import numpy as np
import torch

import stencil_edge_ref as R
from oracle import step_torch as st
from shmgan_amd import _lib

CSRC = Path(__file__).resolve().parent.parent / "shmgan_amd" / "csrc"
f32, f64 = np.float32, np.float64
PTR = 16          # a non-null pointer nobody dereferences: the calls below answer before any launch


# ----------------------------------------------------------------------------------------------------------------- the restated constants
def test_constants_are_the_sources():
    """The dispatch constants restated in stencil_edge_ref.py still stand in the kernel sources, as text.  A failure here after a kernel
    file was reformatted is no regression of the kernels: re-read the source line the constant's comment names, update stencil_edge_ref.py
    (and the snippet below) to it, and check that the case tables still reach every form."""
    sum1, igemm, elem = ((CSRC / n).read_text() for n in ("dgrad_sum1.hip", "conv_igemm.hip", "elem.hip"))
    for dt, macro, ty in (("f32", "SHM_F32", "float"), ("bf16", "SHM_BF16", "bf16_t")):
        for nkc in R.MFMA_NKC[dt]:
            assert f"dtype == {macro} && nkc == {nkc}) SHM_SUM1_MFMA({ty}, {nkc});" in sum1, (dt, nkc)
    assert sum1.count("nkc == ") == 8 == sum(len(v) for v in R.MFMA_NKC.values())
    assert "if (nk * c <= 5 * 64)" in sum1 and R.LDS_NKC == 5 * 64
    assert sum1.count(f"constexpr int TO = {R.TO}") == 2
    assert "kb = dtype == SHM_F32 ? 16 : 32" in sum1 and "nkc = c % kb == 0 ? nk * c / kb : 0" in sum1 and R.KB == {"f32": 16, "bf16": 32}
    assert "shm_cdiv(hi, 16) * shm_cdiv(wi, 16)" in sum1 and f"shm_cdiv(9 * cout, {R.SUMCH_BLOCK})" in sum1
    assert f"constexpr int kMaxTransposes = {R.TRANSPOSE_MAX};" in igemm and f"tile[{R.TRANSPOSE_TILE}][{R.TRANSPOSE_TILE + 1}]" in igemm
    for name in ("mul_mask_kernel<T>", "mask_pool_pack_kernel<T>", "add_bcast_kernel<T>", "sum_groups_kernel<T>"):
        launch = elem[elem.index("hipLaunchKernelGGL(" + name):]
        assert f", {R.ELEM_BLOCK})), dim3({R.ELEM_BLOCK})" in launch[:launch.index("\n")], name


# --------------------------------------------------------------------------------------------------------------------- the stencil's table
def test_the_case_table_reaches_every_form_and_geometry():
    forms = {R.form_of(*f) for f in R.FORMS}
    want = {("mfma", dt, n) for dt in ("f32", "bf16") for n in R.MFMA_NKC[dt]} | {(k, dt, 0) for k in ("tiled", "plain") for dt in ("f32", "bf16")}
    assert forms == want and len(want) == 12 and len(set(R.FORMS)) == len(R.FORMS)
    # the (nk, c) each form is reached through
    assert [R.form_of("f32", nk, c)[2] for nk, c in ((1, 16), (1, 64), (2, 32), (5, 16), (5, 64))] == [1, 4, 4, 5, 20]
    assert [R.form_of("bf16", nk, c)[2] for nk, c in ((1, 32), (1, 64), (2, 32), (5, 32), (5, 64))] == [1, 2, 2, 5, 10]
    tiled = {(dt, nk, c) for dt, nk, c in R.FORMS if R.form_of(dt, nk, c)[0] == "tiled"}
    assert tiled == {("f32", 1, 4), ("f32", 3, 8), ("f32", 2, 16), ("bf16", 1, 16)} | {(dt, nk, c) for dt in ("f32", "bf16") for nk, c in ((2, 64), (2, 128), (1, 256))}
    assert {(nk, c) for dt, nk, c in R.FORMS if R.form_of(dt, nk, c)[0] == "plain"} == {(6, 64), (3, 128), (2, 256)}
    assert {c for _, _, c in tiled} >= {4, 8, 16, 128, 256} and any(nk > 1 for _, nk, _ in tiled)
    assert R.form_of("bf16", 1, 160) == ("mfma", "bf16", 5) and (160 // 4) & (160 // 4 - 1)          # the other road to NKC = 5 is refused: c / 4 no power of two
    cases = R.all_cases()
    assert len(set(cases)) == len(cases)
    partial_odd = lambda sc: (sc.h % R.TO or sc.w % R.TO) and (sc.h % 2 or sc.w % 2)          # noqa: E731
    for form in want:
        mine = [sc for sc in cases if R.form_of(sc.dt, sc.nk, sc.c) == form]
        assert any(partial_odd(sc) and sc.stride == 2 for sc in mine) and any(partial_odd(sc) and sc.stride == 1 for sc in mine), form
        assert {sc.wide for sc in mine} == {False, True}, form
    for kern in {f[:2] for f in want}:
        mine = [sc for sc in cases if R.form_of(sc.dt, sc.nk, sc.c)[:2] == kern]
        assert {(sc.stride, sc.h, sc.w) for sc in mine} == set(R.GEOMS), kern                   # every side of the issue's two lists
        assert any(sc.batch == 3 and sc.nk == 2 for sc in mine), kern                           # k * batch + b against b * nk + k
        assert {sc.batch for sc in mine} == {1, 2, 3}
        assert any(sc.h < R.TO and sc.w < R.TO for sc in mine) and any(sc.h > R.TO and sc.w > R.TO for sc in mine)
        assert {(sc.wide, sc.stride) for sc in mine} == {(a, b) for a in (False, True) for b in (1, 2)}
        assert sum(R.form_of(sc.dt, sc.nk, sc.c)[:2] == kern for sc in R.NONFINITE) == 2
    for sc in cases + R.NONFINITE:
        assert sc.c % 4 == 0 and (sc.c // 4) & (sc.c // 4 - 1) == 0 and sc.c <= 256          # what the entry point accepts
        ld = R.wide_pitch(sc.dt, sc.c)
        assert ld % (4 if sc.dt == "f32" else 8) == 0 and ld > sc.c
    for sc in R.NONFINITE:
        assert sc.h % R.TO or sc.w % R.TO
    assert set(R.GEOMS_FEW) <= set(R.GEOMS) and all(h <= 40 and w <= 40 for _, h, w in R.GEOMS)


def test_padding_and_partial_tiles():
    for h, w in R.SIDES_S2:
        (ho, pt), (wo, pl) = R.same_pad(h, 2), R.same_pad(w, 2)
        assert (pt, pl) == (h % 2, w % 2) and (ho, wo) == ((h + 1) // 2, (w + 1) // 2)
    for h, w in R.SIDES_S1:
        assert R.same_pad(h, 1) == (h, 1) and R.same_pad(w, 1) == (w, 1)
    for n in range(1, 40):          # against the oracle's own rule (pad_before, pad_after)
        for s in (1, 2):
            assert st._same_pads(n, 3, s)[0] == R.same_pad(n, s)[1]
    # the dz region of a tile: R * Cn is no multiple of 16 at stride 2 (a ragged last MFMA step, lanes with j >= npx), and at stride 1 (18 x 18)
    assert set(R.tile_regions(17, 17, 2)) == {(10, 10)} and 100 % 16
    assert all(R_ * Cn % 16 for s, h, w in R.GEOMS if s == 2 and (h % 2 or w % 2) for R_, Cn in R.tile_regions(h, w, s))
    assert set(R.tile_regions(33, 15, 1)) == {(18, 18)} and all(R_ <= 18 and Cn <= 18 for s, h, w in R.GEOMS for R_, Cn in R.tile_regions(h, w, s))
    assert len(R.tile_regions(31, 34, 2)) == 6 and len(R.tile_regions(1, 1, 1)) == 1


def _autograd(k):
    sc = k.sc
    ref = np.zeros((sc.batch, sc.h, sc.w))
    for j in range(sc.nk):
        x = torch.zeros(sc.batch, 1, sc.h, sc.w, dtype=torch.float64, requires_grad=True)
        y = st.conv2d_same(x, R.t64(k.weff[j].copy()).view(3, 3, 1, sc.c), sc.stride)
        dz = R.t64(k.dz[j * sc.batch:(j + 1) * sc.batch].copy()).permute(0, 3, 1, 2)
        ref += torch.autograd.grad(y, x, dz)[0][:, 0].numpy()
    return ref


def test_stencil_reference_against_autograd():
    for sc in (R.SC("f32", 2, 8, 3, 16, 17, 1, False), R.SC("f32", 3, 8, 2, 7, 5, 2, False), R.SC("bf16", 2, 32, 3, 17, 17, 2, True),
               R.SC("f32", 1, 4, 1, 1, 1, 2, False), R.SC("f32", 1, 4, 2, 2, 2, 2, False)):
        k = R.stencil_case(sc)
        assert np.allclose(k.s, _autograd(k), rtol=1e-12, atol=1e-13), sc
        # the same stencil from the output pixel's side, which the float32 evaluation and the modelled faults are built on
        g = R.gather(R.tap_products(k.dz, k.weff, sc.nk, sc.batch), sc.h, sc.w, sc.stride)
        assert np.allclose(g, k.s, rtol=1e-12, atol=1e-13) and (k.A >= np.abs(k.s)).all() and (k.A > 0).all()
    k = R.stencil_case(R.SC("bf16", 2, 32, 3, 17, 17, 2, True))
    assert np.array_equal(R.rb(k.dz), k.dz) and np.array_equal(R.r32(k.weff), k.weff) and (k.weff != 0).all()
    assert not np.array_equal(R.rb(k.weff), k.weff) and k.ld == 40
    w = k.weff
    assert np.abs(R.bf16_split(w) - w).max() <= 2.0 ** -17 * np.abs(w).max() and np.array_equal(R.r32(R.bf16_split(w)), R.bf16_split(w))


def test_float32_evaluation_passes_with_room():
    """The per-pixel constants are what this test measures: the worst |err| / A of the float32 evaluation over the whole table, both
    accumulate modes.  Every case also passes the rel-L2 bound with the factor to spare."""
    worst = {"f32": [0.0, 0.0], "split": [0.0, 0.0]}
    for sc in R.all_cases():
        k = R.stencil_case(sc)
        cls = "split" if R.form_of(sc.dt, sc.nk, sc.c)[:2] == ("mfma", "bf16") else "f32"
        for acc in (0, 1):
            ref, A = R.stencil_expect(k, acc)
            rel, ratio = R.stencil_figs(R.stencil_f32(k, acc), ref, A)
            assert rel * R.SPARE < R.STENCIL_TOL, (sc, acc, rel)
            assert R.stencil_ok((rel, ratio), R.stencil_k(sc))
            worst[cls] = [max(worst[cls][0], rel), max(worst[cls][1], ratio)]
    print("float32 evaluation, worst (rel-L2, |err| / A):", worst)
    assert 0.95 * R.K_F32_MEASURED < worst["f32"][1] <= R.K_F32_MEASURED
    assert 0.95 * R.K_SPLIT_MEASURED < worst["split"][1] <= R.K_SPLIT_MEASURED
    assert R.K_F32 == R.SPARE * R.K_F32_MEASURED and R.K_SPLIT == R.SPARE * R.K_SPLIT_MEASURED and R.SPARE == 3.0
    assert R.K_F32 < 32 * 2.0 ** -24 and R.K_SPLIT < 2.0 ** -17          # a few roundings of A; the split's stated accuracy


def test_nonfinite_cases_and_their_comparison():
    for sc in R.NONFINITE:
        k = R.stencil_case(sc, True)
        bad = ~np.isfinite(k.s)
        pt, pl = R.same_pad(sc.h, sc.stride)[1], R.same_pad(sc.w, sc.stride)[1]
        ys = [y for y in range(sc.h) for kh in range(3) if y + pt - kh == 0]          # the pixels whose stencil covers dz pixel (0, 0)
        xs = [x for x in range(sc.w) for kw in range(3) if x + pl - kw == 0]
        want = np.zeros_like(bad)
        want[:, np.array(ys)[:, None], np.array(xs)[None, :]] = True
        assert np.array_equal(bad, want) and bad.sum() == sc.batch * len(ys) * len(xs) and len(ys) == len(xs) == 2
        assert np.array_equal(~np.isfinite(k.A), bad) and (k.weff != 0).all() and np.isinf(k.dz).sum() == sc.nk * sc.batch
        for acc in (0, 1):
            ref, A = R.stencil_expect(k, acc)
            with np.errstate(invalid="ignore"):
                low = R.stencil_f32(k, acc)
            assert R.stencil_ok(R.stencil_figs(low, ref, A), R.stencil_k(sc)), (sc, acc)
            nan = np.where(bad, np.nan, low)                                           # NaN in place of Inf is non-finite all the same
            assert R.stencil_ok(R.stencil_figs(nan, ref, A), R.stencil_k(sc))
            spread = low.copy()
            spread[0, -1, -1] = np.inf                                                 # one more non-finite pixel
            assert R.stencil_figs(spread, ref, A) == (float("inf"), float("inf"))
            assert R.stencil_figs(np.where(bad, 0.0, low), ref, A) == (float("inf"), float("inf"))          # the Inf swallowed


def test_modelled_faults_fail_the_comparison():
    """Each fault, evaluated in float64 (free of rounding), fails one of the two conditions on at least one case of the table -- and, for
    every kernel and dtype, on one of ITS cases."""
    cases = R.all_cases()
    kerns = sorted({R.form_of(sc.dt, sc.nk, sc.c)[:2] for sc in cases})
    caught = {f: set() for f in R.FAULTS}
    only_pixel = {f: 0 for f in R.FAULTS}
    for sc in cases:
        k = R.stencil_case(sc)
        for acc in (0, 1):
            ref, A = R.stencil_expect(k, acc)
            assert R.stencil_figs(R.stencil_f32(k, acc, None, f64), ref, A)[1] < 1e-12          # no fault: exact
            for f in R.FAULTS:
                figs = R.stencil_figs(R.stencil_f32(k, acc, f, f64), ref, A)
                if not R.stencil_ok(figs, R.stencil_k(sc)):
                    caught[f].add(R.form_of(sc.dt, sc.nk, sc.c)[:2])
                    only_pixel[f] += figs[0] < R.STENCIL_TOL
    print("cases a fault passes rel-L2 on and fails the per-pixel bound:", only_pixel)
    for f in R.FAULTS:
        assert caught[f] == set(kerns), (f, caught[f])
    # where each fault must show: pad0 on every odd-sided stride-2 case, rows / cols on every partial tile, noacc everywhere
    for sc in cases:
        k = R.stencil_case(sc)
        ref, A = R.stencil_expect(k, 1)
        bad = lambda f, acc=1: not R.stencil_ok(R.stencil_figs(R.stencil_f32(k, acc, f, f64), *R.stencil_expect(k, acc)), R.stencil_k(sc))          # noqa: E731
        assert bad("noacc", 0) and bad("noacc", 1), sc
        if sc.stride == 2 and (sc.h % 2 or sc.w % 2):
            assert bad("pad0"), sc
        if sc.h % R.TO:
            assert bad("rows", 0), sc
        if sc.w % R.TO:
            assert bad("cols", 0), sc
        if sc.nk > 1 and sc.batch > 1:
            assert bad("bk"), sc
        if sc.stride == 2 and max(sc.h, sc.w) > 2:
            assert bad("noparity"), sc
        if max(sc.h, sc.w) > 1:
            assert bad("swap") and bad("masked"), sc


# ------------------------------------------------------------------------------------------------------------- shm_sum_input_channels
def test_sum_input_channels_cases_and_reference():
    assert [9 * c for c in R.SUMCH_COUT] == [9, 144, 261, 576] and 144 < R.SUMCH_BLOCK < 261 and 576 > 2 * R.SUMCH_BLOCK
    for cin in R.SUMCH_CIN:
        m = R.sumch_masks(cin)
        full = (1 << cin) - 1
        assert m[0] == 0 and m[1] == 0xFFFFFFFF and m[2] == full and m[3] == 1 << (cin - 1) and all(0 <= v < 1 << 32 for v in m)
        assert cin == 32 or (m[4] >> cin and m[4] & full not in (0, full) or cin == 1)
        w = R.sumch_case(cin, 29)
        for mask in m:
            s, a = R.sumch_ref(w, mask)
            sel = [j for j in range(cin) if (mask >> j) & 1]
            assert np.allclose(s, w[:, sel].sum(1), rtol=1e-13, atol=1e-15) and np.allclose(a, np.abs(w[:, sel]).sum(1))
            low = R.sumch_ref(w, mask, f32)[0]
            assert (np.abs(low - s) * R.SPARE <= R.SUMCH_UNIT * a).all()
        assert np.array_equal(R.sumch_ref(w, m[1])[0], R.sumch_ref(w, m[2])[0])                  # bits at or above cin are ignored
        assert not R.sumch_ref(w, 0)[0].any()
        if cin > 1:          # teeth: one selected channel dropped, or one ignored bit honoured, is beyond the bound
            s, a = R.sumch_ref(w, full)
            assert (np.abs(R.sumch_ref(w, full & ~1)[0] - s) > R.SUMCH_UNIT * a).any()
    assert R.sumch_masks(32)[3] == 1 << 31


def test_argument_refusals_before_any_launch():
    L = _lib.lib()
    F32, BF16 = _lib.F32, _lib.BF16
    assert L.shm_sum_input_channels(PTR, 0, 16, 1, PTR, None) == -1 and L.shm_sum_input_channels(PTR, 33, 16, 1, PTR, None) == -1
    assert L.shm_sum_input_channels(None, 3, 16, 1, PTR, None) == -1 and L.shm_sum_input_channels(PTR, 3, 16, 1, None, None) == -1
    assert b"shm_sum_input_channels" in L.shm_last_error()
    # the stencil: bf16 pitches are multiples of 8 (the header's rule; the bf16 MFMA form loads 16 bytes a lane), fp32 pitches of 4.  An
    # empty call (batch = 0) returns SHM_OK after the argument checks and launches nothing.
    sum1 = lambda ld, c, dt, batch=0, nk=1, stride=1: L.shm_conv3x3_dgrad_sum1(PTR, ld, PTR, PTR, nk, batch, 17, 17, c, stride, 0, dt, None)          # noqa: E731
    assert sum1(36, 32, BF16) == -1 and b"multiple of 8" in L.shm_last_error()
    assert sum1(36, 32, BF16, batch=2) == -1 and sum1(20, 16, BF16) == -1 and sum1(12, 4, BF16) == -1
    assert sum1(40, 32, BF16) == 0 and sum1(32, 32, BF16) == 0 and sum1(24, 16, BF16) == 0
    assert sum1(36, 32, F32) == 0 and sum1(20, 16, F32) == 0 and sum1(18, 16, F32) == -1
    assert sum1(160, 160, BF16) == -1 and sum1(64, 64, F32, stride=3) == -1                      # c / 4 no power of two; stride
    assert sum1(64, 64, F32, batch=2, nk=0) == 0                                                  # nk = 0: nothing to do
    assert L.shm_conv3x3_dgrad_sum1(None, 64, PTR, PTR, 1, 1, 17, 17, 64, 1, 0, F32, None) == -1
    # transposes: at most 48 in one launch; none is fine
    assert L.shm_transpose_taps_multi(R.TRANSPOSE_MAX + 1, None, None, None, None, None, None, F32, None) == -1 and b"at most 48" in L.shm_last_error()
    assert L.shm_transpose_taps_multi(0, None, None, None, None, None, None, F32, None) == 0
    assert L.shm_transpose_taps_multi(-1, None, None, None, None, None, None, F32, None) == -1
    assert L.shm_transpose_taps(PTR, PTR, 9, 33, 31, 32, F32, None) == -1                         # rows_pad < rows
    one = (C.c_int * 1)
    tab = (C.c_void_p * 1)(PTR)
    assert L.shm_transpose_taps_multi(1, tab, tab, one(9), one(33), one(31), one(32), F32, None) == -1
    # the dropout multiply: n a multiple of four
    for n in (1, 2, 3, 4 * 256 + 2):
        assert L.shm_mul_mask(PTR, PTR, PTR, n, 1.25, F32, None) == -1, n
    assert L.shm_mul_mask(PTR, PTR, PTR, 0, 1.25, F32, None) == 0
    # the attention helpers
    assert L.shm_mask_pool_pack(PTR, PTR, 16, 1, 30, 4, F32, None) == -1 and L.shm_mask_pool_pack_hw(PTR, PTR, 16, 1, 15, 10, 2, F32, None) == -1
    assert L.shm_mask_pool_pack(PTR, PTR, 0, 1, 30, 5, F32, None) == -1 and L.shm_mask_pool_pack(PTR, PTR, 16, 0, 30, 5, F32, None) == 0
    assert L.shm_add_bcast(PTR, PTR, PTR, 3, 6, 2, 0, F32, None) == -1 and L.shm_add_bcast(PTR, PTR, PTR, 3, 8, 0, 0, F32, None) == -1
    assert L.shm_add_bcast(PTR, PTR, PTR, 0, 8, 2, 0, F32, None) == 0
    assert L.shm_sum_groups(PTR, PTR, 3, 6, 2, 0, 0, F32, None) == -1 and L.shm_sum_groups(PTR, PTR, 3, 8, 2, -1, 0, F32, None) == -1


# ------------------------------------------------------------------------------------------------------------------------- transposes
def test_transpose_cases_and_reference():
    T = R.TRANSPOSE_TILE
    s = R.TRANSPOSE_SHAPES
    assert s[0] == (1, 1, 1, 1) and (9, 32, 32, 32) in s
    assert any(r % T and c % T and r < T < c for _, r, c, _ in s) and any(r % T and c % T and c < T < r for _, r, c, _ in s)
    assert any(rp - r >= 2 * T for _, r, _, rp in s) and all(rp >= r for _, r, _, rp in s)          # whole tiles of padding
    for i, shape in enumerate(s):
        w = R.transpose_case(i, shape)
        ref = R.transpose_ref(w, shape[3])
        assert ref.shape == (shape[0], shape[2], shape[3]) and ref.dtype == np.float32
        loop = np.zeros_like(ref)
        for t in range(shape[0]):
            for r in range(shape[1]):
                for c in range(shape[2]):
                    loop[t, c, r] = w[t, r, c]
        assert np.array_equal(ref, loop) and not ref[:, :, shape[1]:].any()
        assert np.array_equal(torch.from_numpy(w).transpose(1, 2).numpy(), ref[:, :, :shape[1]])
        if shape[1] > 1 and shape[2] > 1:          # teeth: the untransposed copy differs, in both dtypes
            flat = np.zeros_like(ref).reshape(shape[0], -1)
            flat[:, :shape[1] * shape[2]] = w.reshape(shape[0], -1)
            assert not np.array_equal(R.to_dtype_bits(flat.reshape(ref.shape), "bf16"), R.to_dtype_bits(ref, "bf16"))
    # bf16: round to nearest even, not truncation
    x = np.array([0x3F808000, 0x3F818000, 0x3F808001], dtype=np.uint32).view(np.float32)
    assert R.to_dtype_bits(x, "bf16").view(np.uint16).tolist() == [0x3F80, 0x3F82, 0x3F81]
    assert np.array_equal(R.to_dtype_bits(x, "f32"), x.view(np.int32))


# ------------------------------------------------------------------------------------------------------ attention helpers, dropout multiply
def test_helper_cases_and_references():
    import torch.nn.functional as F
    B = R.ELEM_BLOCK
    assert {k for *_, k in R.POOL_SQUARE} | {k for *_, k in R.POOL_HW} == {1, 2, 3, 5, 8}
    assert (3, 15, 10, 5) in R.POOL_HW and 3 * 3 * 2 < B and (2, 34, 26, 2) in R.POOL_HW and 2 * 17 * 13 > B and (2 * 17 * 13) % B
    assert all(s % k == 0 for _, s, k in R.POOL_SQUARE) and all(h % k == 0 and w % k == 0 for _, h, w, k in R.POOL_HW)
    assert R.POOL_LD == (1, 16, 20, 32)
    for b, h, w, k in R.POOL_HW + tuple((b, s, s, k) for b, s, k in R.POOL_SQUARE):
        for neg in (False, True):
            m = R.pool_mask(b, h, w, neg)
            assert m.dtype == np.float32 and ((m < 0).all() if neg else (m > 0).any() and (m < 0).any())
            ref = R.pool_ref(m, k, 20)
            want = F.max_pool2d(torch.from_numpy(m)[:, None], k)[:, 0].numpy()
            assert np.array_equal(ref[..., 0], want) and not ref[..., 1:].any() and not np.signbit(ref[..., 1:]).any()
            if neg:          # teeth: a running maximum that starts from zero
                assert not np.array_equal(np.maximum(ref[..., 0], 0), ref[..., 0])
    # the index cases
    c = R.BCAST_CASES
    assert any(per == 4 for _, per, _, _ in c) and any((per // 4) % 1 == 0 and B % (per // 4) for _, per, _, _ in c)
    assert any(nb == 1 for _, _, nb, _ in c) and any(nb > n > 0 for n, _, nb, _ in c) and any(i0 >= nb and n for n, _, nb, i0 in c) and (7, 308, 3, 7) in c
    assert sum(n == 0 for n, *_ in c) == 2 and all(per % 4 == 0 for _, per, _, _ in c)
    assert any(n * per // 4 > B and (n * per // 4) % B for n, per, _, _ in c)                      # a ragged last block
    for case in c:
        nimg, per, nb, i0 = case
        for dt in ("f32", "bf16"):
            k = R.bcast_case(case, dt)
            out = R.add_bcast_ref(k.a, k.b, nb, i0)
            assert out.dtype == np.float32 and out.shape == (nimg, per)
            for i in range(nimg):
                assert np.array_equal(out[i], k.a[i] + k.b[(i0 + i) % nb])
            for acc in (False, True):
                g = R.sum_groups_ref(k.a, k.d0, nb, i0, acc)
                assert g.dtype == np.float32
                exact = (k.d0.astype(f64) if acc else 0) + np.array([k.a[[i for i in range(nimg) if (i0 + i) % nb == j]].astype(f64).sum(0) if nimg else
                                                                     np.zeros(per) for j in range(nb)])
                assert np.allclose(g, exact, rtol=1e-5, atol=1e-6)
                empty = [j for j in range(nb) if not any((i0 + i) % nb == j for i in range(nimg))]
                assert all(np.array_equal(g[j], k.d0[j] if acc else np.zeros(per, f32)) for j in empty)
            if nimg and nb > 1 and i0 % nb:          # teeth: the offset ignored
                assert not np.array_equal(R.add_bcast_ref(k.a, k.b, nb, 0), out)
                assert not np.array_equal(R.sum_groups_ref(k.a, k.d0, nb, 0, False), R.sum_groups_ref(k.a, k.d0, nb, i0, False))
    assert any(nb > n > 0 for n, _, nb, _ in c)                                                     # groups without an image
    # dropout multiply
    assert [n // 4 for n in R.MULMASK_N] == [100, B, 3 * B + 77] and all(n % 4 == 0 for n in R.MULMASK_N)
    for n in R.MULMASK_N:
        for dt in ("f32", "bf16"):
            x, m = R.mulmask_case(n, dt)
            y = R.mulmask_ref(x, m, R.MULMASK_SCALE)
            assert y.dtype == np.float32 and np.allclose(y, x.astype(f64) * m * R.MULMASK_SCALE, rtol=3e-7)
            assert set(np.unique(m[::3])) == {0.0, 1.0}
            other = x * (m * f32(R.MULMASK_SCALE))
            assert not np.array_equal(other, y)                                                   # the order of the two products shows in the last bit
