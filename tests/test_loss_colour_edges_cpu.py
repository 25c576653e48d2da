"""CPU checks of the inputs and the oracle behind test_loss_colour_edges_gpu.py: every engineered input (loss_edge_ref.py) is in the case it
claims to be -- sizes past the grid caps, row counts that split a wave, gradients on both sides of the clip and on it, a variance on the
floor, rescale_01's extremes in the plane named, unique Y extremes, den == 0 -- the float64 oracle is finite on all of them, the oracle run
in float32 stays within every bound in use, and the checks have teeth (a missing min / max correction, a byte written into a guard)."""
import numpy as np
import pytest
import torch

import loss_edge_ref as R
from oracle import step_torch as st
from util import rel_l2


# ------------------------------------------------------------------------------------------------------------------------ clip + Adam
def test_adam_cases_cover_the_clip_and_the_grid():
    assert R.ADAM_SIZES[-1] == 8192 * 256 + 77 > 3 * 3 * 512 * 512 - 8192 * 256 and R.ADAM_SIZES[-1] > R.ADAM_GRID
    gs = R.r32(R.ADAM_LADDER * R.ADAM_GSCALE)
    assert (gs < -1).any() and (gs > 1).any() and (gs == -1).any() and (gs == 1).any() and ((gs > -1) & (gs < 1) & (gs != 0)).any()
    for n in R.ADAM_SIZES:
        c = R.adam_case(n)
        assert c.clipped.any() and np.isfinite(c.rw).all() and np.isfinite(c.rm).all() and np.isfinite(c.rv).all()
        assert np.array_equal(c.gs, c.g * R.ADAM_GSCALE)          # the float product is exact: "exactly +-1" means the same on the device
        if n < 8:
            continue
        assert c.edge.any() and c.eps_only.any() and (~c.clipped & ~c.edge & (c.gs != 0)).any()
        assert (c.gs[c.clipped] < 0).any() and (c.gs[c.clipped] > 0).any()
        # eps carries the division: v' = 0 exactly, the step is alpha * m' / eps
        e = c.eps_only
        assert (c.rv[e] == 0).all() and np.allclose((c.w - c.rw)[e], c.alpha * c.rm[e] / R.ADAM_EPS, rtol=1e-12)
        # the clip acts: the reference moments of the clipped elements are those of g = +-1
        k = c.clipped
        assert np.allclose(c.rm[k], c.m[k] + (np.sign(c.gs[k]) - c.m[k]) * (1 - R.ADAM_B1), rtol=1e-12)
        # the step of a clipped element is small enough for the max-abs bound's reasoning
        assert np.abs(c.w - c.rw)[k].max() < 1e-4
    c = R.adam_case(R.ADAM_SIZES[-1])
    t = slice(c.n - R.ADAM_TAIL, c.n)
    assert (R.r32(c.rw)[t] != c.w[t]).all() and (R.r32(c.rm)[t] != c.m[t]).all() and (R.r32(c.rv)[t] != c.v[t]).any()
    # a float32 evaluation of the same update passes the bounds in use
    f = np.float32
    gg = np.clip(c.gs, -1, 1).astype(f)
    mm = c.m.astype(f) + (gg - c.m.astype(f)) * (f(1) - f(R.ADAM_B1))
    vv = c.v.astype(f) + (gg * gg - c.v.astype(f)) * (f(1) - f(R.ADAM_B2))
    ww = c.w.astype(f) - f(c.alpha) * mm / (np.sqrt(vv) + f(R.ADAM_EPS))
    assert rel_l2(ww, c.rw) < 1e-6 and rel_l2(mm, c.rm) < 1e-6 and rel_l2(vv, c.rv) < 1e-6
    assert (np.abs(ww - c.rw)[c.clipped] <= R.adam_w_abs_bound(c.rw)[c.clipped]).all()


# --------------------------------------------------------------------------------------------------------------------- colour, inputs
def test_colour_shapes_split_a_wave_and_a_block():
    rows = [5 * b * h * w for b, h, w in R.COLOUR_SHAPES]
    assert rows[0] == 1125 and rows[0] % 64 == 37 and rows[0] % 256 == 101
    assert all(r % 64 and r % 256 for r in rows)
    assert all((b * h * w) % 64 for b, h, w in R.COLOUR_SHAPES)


def test_guard_band_sees_one_byte():
    for dt in (torch.float32, torch.bfloat16):
        raw, p = R.guarded(5, 4, dt, "cpu")
        assert p.shape == (5, 4) and p.dtype == dt and raw.numel() == (5 + R.GUARD_ROWS) * 4 * p.element_size()
        p.zero_()
        assert R.guard_intact(raw, p)
        raw[p.numel() * p.element_size()] ^= 1
        assert not R.guard_intact(raw, p)
        raw[p.numel() * p.element_size()] ^= 1
        raw[-1] = 0
        assert not R.guard_intact(raw, p)
    assert float(torch.full((4,), R.SENT_BYTE, dtype=torch.uint8).view(torch.float32)[0]) != 0.0


def test_colour_references():
    c = R.colour_case(*R.COLOUR_SHAPES[1])
    B = c.B
    # image k * B + b of the D batch takes the chroma of sample b
    ref = R.yuv2rgb_ref(c.ych, c.cbcr)
    k, b = 3, 2
    one = st.yuv_to_rgb(R.t64(np.concatenate([c.ych[k * B + b], c.cbcr[b]], -1))).numpy()
    assert np.array_equal(ref[k * B + b], one)
    for mask in R.GEN_MASKS:
        g0, g1 = R.gen_input_ref(c.ys, c.gen_y, mask, 0, 16), R.gen_input_ref(c.ys, c.gen_y, mask, 1, 32)
        assert g0.shape == (B, c.h, c.w, 16) and g1.shape == (5 * B, c.h, c.w, 32)
        assert (g0[..., 5:9] == 0).all() and (g0[..., 9] == 1).all() and (g0[..., 10:] == 0).all() and (g1[..., 10:] == 0).all()
        for k in range(5):
            v = g1[k * B:(k + 1) * B]
            assert (v[..., k] == 0).all() and (v[..., 5 + k] == 1).all() and v[..., 5:10].sum() == v[..., 0].size
            for j in range(5):
                if j != k:
                    assert np.array_equal(v[..., j], c.gen_y[..., 0] if (mask >> j) & 1 else c.ys[j][..., 0])
                assert np.array_equal(g0[..., j], np.zeros_like(g0[..., j]) if (mask >> j) & 1 else c.ys[j][..., 0])
    # cyc_input_bwd is the adjoint of mode 1's dependence on gen_y: <build(gen_y) - build(0), d> == <gen_y, bwd(d)>
    rng = np.random.default_rng(5)
    d = rng.standard_normal((5 * B, c.h, c.w, 16))
    for mask in R.GEN_MASKS:
        lhs = ((R.gen_input_ref(c.ys, c.gen_y, mask, 1, 16) - R.gen_input_ref(c.ys, 0 * c.gen_y, mask, 1, 16)) * d).sum()
        rhs = (c.gen_y[..., 0] * R.cyc_input_bwd_ref(d, mask, B)).sum()
        assert abs(lhs - rhs) < 1e-9 * max(1.0, abs(lhs))
    assert not R.cyc_input_bwd_ref(d, 0, B).any()


# ---------------------------------------------------------------------------------------------------------------------- standardisation
def test_std_inputs():
    x = R.std_floor_batch()
    yuv, scale = R.std_ref(x)
    # black and the dark grey sit on the floor exactly; mid-grey does not: rgb_to_yuv of a grey g is (g, 0, 0), not a constant
    assert scale[0] == R.STD_FLOOR and scale[3] == R.STD_FLOOR
    assert abs(scale[1] - R.STD_MID_GREY_SCALE) < 1e-7 and scale[1] > 50 * R.STD_FLOOR and scale[2] > R.STD_FLOOR
    assert not yuv[0].any() and np.isfinite(yuv).all()
    raw_std = st.rgb_to_yuv(R.t64(x[3])).std()
    assert 0 < float(raw_std) < R.STD_FLOOR          # the floor acts on the dark grey (not a zero variance)
    r = R.std_ramp()
    assert r.shape == (1, R.STD_RAMP_NPIX, 1, 3) and R.STD_RAMP_NPIX > 512 * 256 > 32 * 256 and (R.STD_RAMP_NPIX - 512 * 256) % 256
    ry, rs = R.std_ref(r)
    assert rs[0] > 10 * R.STD_FLOOR and np.isfinite(ry).all()
    # the float32 restatement of the same standardisation is within the tolerance in use
    y32 = (r.astype(np.float32) @ np.array(st._RGB2YUV, np.float32)).astype(np.float64)
    s32 = np.sqrt(max((y32 * y32).mean() - y32.mean() ** 2, 0.0))
    assert rel_l2(y32 / np.float32(s32), ry) < R.F32_TOL and abs(s32 - rs[0]) < R.F32_TOL * rs[0]


# ------------------------------------------------------------------------------------------------------------------------ image losses
PLACEMENT = {
    # the random cases of test_image_losses' construction: Y ~ N(1, 0.5^2) against the standardised chroma: the maximum lies in Y, the
    # minimum in a chroma plane
    **{n: "mixed" for n in R.SIZE_CASES}, "black_view": "mixed",
    "chroma_extremes": "chroma", "y_extremes": "y", "flat_cyc1": "y", "flat_cyc4": "y",
}


@pytest.fixture(scope="module")
def oracle():
    cache = {}

    def get(name):
        if name not in cache:
            inp, flags = R.image_case(name)
            cache[name] = (inp, flags, R.image_oracle(inp, flags))
        return cache[name]
    return get


def test_image_case_list():
    sizes = {(int(n.split("_")[0][4:]), int(n.split("_")[1][1:])) for n in R.SIZE_CASES}
    assert sizes == {(11, 1), (16, 1), (26, 1), (27, 1), (27, 3)}
    assert R.image_case("size27_b1_all")[1] == (True,) * 5 and R.image_case("size11_b1_none")[1] == (False,) * 5
    assert {n.split("_")[2] for n in R.SIZE_CASES} == {"none", "mixed", "all"}
    # HO = S - 10: one pixel, part of a tile, exactly one 16 x 16 tile, one tile and one pixel
    assert [s - 10 for s in (11, 16, 26, 27)] == [1, 6, 16, 17]


@pytest.mark.parametrize("name", R.IMAGE_CASES)
def test_image_case_is_what_it_claims(name, oracle):
    """placement of rescale_01's extremes per view, uniqueness of the Y extremes, den == 0 where claimed, inputs that are float32 values, a
    finite oracle.  Tied extremes are out of scope (the kernel gives the whole sub-gradient to one tied pixel, autograd splits it): every
    view whose extremes lie in Y has unique ones."""
    inp, flags, o = oracle(name)
    for a in inp.orig + [d.numpy() for d in inp.ds] + [inp.cbcr.numpy(), inp.gen_y, inp.cyc_y]:
        assert np.array_equal(a, R.r32(a))
    flat = int(name[-1]) if name.startswith("flat_cyc") else None
    for (b, k), (kind, pmin, pmax, unique) in R.placement(inp).items():
        if k == flat:
            assert kind == "flat"
            x = torch.cat([R.t64(inp.cyc_y[k * inp.B + b:k * inp.B + b + 1]), inp.cbcr[b:b + 1]], 3)
            assert float(x.amax() - x.amin()) == 0.0 and not st.rescale_01(x).any()          # den == 0: the oracle's where() returns zeros
        else:
            assert kind == PLACEMENT[name], (b, k, kind)
            assert unique, (b, k)
            y, c = inp.cyc_y[k * inp.B + b].ravel(), inp.cbcr[b].numpy().ravel()
            if kind == "y":          # strictly beyond every chroma value: no tie across the planes either
                assert y[pmin] < c.min() and y[pmax] > c.max()
            if kind == "chroma":
                assert c.min() < y.min() and c.max() > y.max()
    if name == "black_view":
        d = inp.ds[R.BLACK_K]
        assert not inp.orig[R.BLACK_K].any() and not d.any() and not st.rescale_01(d).any()          # yr == 0
        assert all(float(inp.ds[k].amax() - inp.ds[k].amin()) > 0 for k in range(5) if k != R.BLACK_K)
    else:
        assert all(float(d[b].amax() - d[b].amin()) > 0 for d in inp.ds for b in range(inp.B))
    L = R.loss_slots(o)
    assert np.isfinite(L).all() and torch.isfinite(o.rg).all() and torch.isfinite(o.rc).all()
    assert all(L[11 + k] == 0.0 for k in range(5) if flags[k]) and all(L[11 + k] > 0.0 for k in range(5) if not flags[k])
    assert float(o.rc.abs().min()) >= 0.0 and float(o.rc.norm()) > 0.1


@pytest.mark.parametrize("name", R.IMAGE_CASES)
def test_float32_oracle_is_within_the_bounds_in_use(name, oracle):
    """The same oracle in float32 on the CPU stays within every bound the GPU test applies to the case: the tolerances of test_image_losses
    hold on every case here (the float32 oracle's own error is at most a tenth of them), so no case needs a bound of its own."""
    inp, flags, o = oracle(name)
    e = R.f32_oracle_errors(name)
    assert (e.slots < R.loss_slot_bounds(o)).all()
    assert e.dg < R.GRAD_TOL and e.dc < R.GRAD_TOL
    eb = np.array([x[3] for x in R.extreme_elements(inp, o.rc.numpy())])
    assert len(eb) == sum(kind == "y" for kind, *_ in R.placement(inp).values())
    assert (e.ext < eb).all()


def test_extreme_element_check_has_teeth(oracle):
    """Without the gradient through amin / amax (rescale_01_fixed_range) the two extreme pixels of every view miss their bound by a wide
    margin while the rest of the gradient is unchanged -- and with the extremes in the chroma planes nothing changes at all."""
    inp, flags, o = oracle("y_extremes")
    fixed = R.image_oracle(inp, flags, rescale=R.rescale_01_fixed_range)
    assert np.allclose(R.loss_slots(fixed), R.loss_slots(o), rtol=1e-13)
    B = inp.B
    full, part = o.rc.numpy().reshape(5 * B, -1), fixed.rc.numpy().reshape(5 * B, -1)
    ext = R.extreme_elements(inp, full)
    assert len(ext) == 5 * B
    for (b, k), pmin, pmax, bound in ext:
        if flags[k]:
            assert np.array_equal(full[k * B + b], part[k * B + b])
            continue
        d = np.abs(full[k * B + b] - part[k * B + b])
        assert min(d[pmin], d[pmax]) > 10 * bound, (b, k, d[pmin], d[pmax], bound)
        d[[pmin, pmax]] = 0
        assert d.max() < 1e-12
    inp, flags, o = oracle("chroma_extremes")
    fixed = R.image_oracle(inp, flags, rescale=R.rescale_01_fixed_range)
    assert np.abs(fixed.rc.numpy() - o.rc.numpy()).max() < 1e-14


@pytest.mark.parametrize("k", [1, 4])
def test_flat_view_has_no_ssim_gradient(k, oracle):
    """den == 0: the oracle's gradient of the flat view is that of the L1 part (k = 4: plus content and style), and differs from it on the
    other views."""
    inp, flags, o = oracle(f"flat_cyc{k}")
    rest = R.image_oracle(inp, flags, ssim_term=False)
    assert np.array_equal(o.rc.numpy()[k], rest.rc.numpy()[k]) and float(o.rc[k].abs().max()) > 0
    assert all(rel_l2(o.rc.numpy()[j], rest.rc.numpy()[j]) > 1e-2 for j in range(5) if j != k)
    assert np.array_equal(o.rg.numpy(), rest.rg.numpy())


def test_all_flags_leave_the_other_parts(oracle):
    inp, flags, o = oracle("size27_b1_all")
    rest = R.image_oracle(inp, flags, ssim_term=False)
    assert np.array_equal(o.rc.numpy(), rest.rc.numpy())
    none = oracle("size27_b1_none")[2]
    assert rel_l2(none.rc.numpy(), o.rc.numpy()) > 1e-2          # same inputs, no flag: the SSIM gradient is visible


def test_shared_builder_is_the_construction_of_test_image_losses():
    """image_inputs_random / image_oracle restate test_image_losses' construction: redo it here in the plainest form on a small case."""
    B, S, flags = 1, 12, (False, True, False, False, False)
    inp = R.image_inputs_random(B, S, seed=21)
    o = R.image_oracle(inp, flags, sf=3.0e-3)
    gen_y = R.t64(inp.gen_y).requires_grad_(True)
    cyc_y = R.t64(inp.cyc_y).requires_grad_(True)
    l1 = lambda a, b: (a - b).abs().mean(dim=(1, 2, 3))
    cyuv = [torch.cat([cyc_y[k:k + 1], inp.cbcr], 3) for k in range(5)]
    crgb = [st.yuv_to_rgb(c) for c in cyuv]
    L1 = (sum(l1(crgb[k], R.t64(inp.orig[k])) for k in range(4)) + l1(st.yuv_to_rgb(torch.cat([gen_y, inp.cbcr], 3)), R.t64(inp.orig[4]))) / 5 \
        + 10 * l1(crgb[4], R.t64(inp.orig[4]))
    ss = [st.ssim(st.rescale_01(cyuv[k]), st.rescale_01(inp.ds[k])) for k in range(5)]
    sl = [torch.zeros(B, dtype=torch.float64) if flags[k] else -torch.log((1 + ss[k]) / 2) for k in range(5)]
    style = 3.0e-3 * ((st.gram_matrix(cyuv[4]) - st.gram_matrix(inp.ds[4])) ** 2).mean(dim=(1, 2))
    content = ((cyuv[4] - inp.ds[0]) ** 2).mean(dim=(1, 2, 3))
    ssim_loss = (sl[0] + sl[1] + sl[2] + sl[3] + 10 * sl[4]) / 5
    tot = (10 * L1 + 10 * ssim_loss + 10 * (100 * style + content)).mean()
    rg, rc = torch.autograd.grad(tot, [gen_y, cyc_y])
    # (not bit for bit: autograd adds the branches' gradients in the order the graph was built)
    assert rel_l2(o.rg.numpy(), rg.numpy()) < 1e-14 and rel_l2(o.rc.numpy(), rc.numpy()) < 1e-14
    assert float(o.style.sum()) == float(style.detach().sum()) and [float(s) for s in o.ssims] == [float(s.detach()) for s in ss]


# ---------------------------------------------------------------------------------------------------------- discriminator-head losses
def test_dhead_oracle_cases():
    assert R.DHEAD_NPATCH == (1, 63, 64, 65, 200)
    for npatch in R.DHEAD_NPATCH:
        rf, cls = R.dhead_case(2, npatch)
        assert rf.shape == (24, npatch) and cls.shape == (24, 5)
        for mode in ("executed", "intended"):
            o = R.dhead_oracle(rf, cls, 2, 0.8, mode)
            assert np.isfinite(o.slots).all() and np.isfinite(o.gd_rf).all() and np.isfinite(o.gd_cls).all() and o.gg_rf.shape == (12, npatch)
    # logits of +-80: the oracle's log_softmax stays finite, cross entropies reach 160
    rf, _ = R.dhead_case(2, 65)
    cls = np.zeros((24, 5))
    cls[:, 0], cls[:, 2] = 80.0, -80.0
    for mode in ("executed", "intended"):
        o = R.dhead_oracle(rf, cls, 2, float(np.float32(1.2)), mode)
        assert np.isfinite(o.slots).all() and np.isfinite(o.gd_cls).all() and max(o.slots[6:9]) > 160.0
    # the two gradient modes differ on the D1 rows alone
    a, b = R.dhead_oracle(rf, cls, 2, 1.2, "executed"), R.dhead_oracle(rf, cls, 2, 1.2, "intended")
    assert np.abs(a.gd_cls - b.gd_cls)[2:].max() == 0.0 and np.abs(a.gd_cls - b.gd_cls)[:2].max() > 0.0
