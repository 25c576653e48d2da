"""The case table of test_elem_geometry_gpu.py held to the geometry classes it claims, and the teeth of the checks that test uses (no GPU).

  * every row of geom_ref.FWD / BWD / LRELU exhibits, at the knob values it sets and in every dtype it runs in, the classes it claims of each
    pass (geom_ref.geometry restates csrc/elem.h and the launchers), and the figures of the issue's shape table are what the restatement gives;
  * every knob value the GPU test is to cover sits on at least one ragged multi-block row of every pass that reads it;
  * geom_ref.visits touches every pixel of a sample exactly once, for every row, pass and dtype;
  * modelled partition faults, applied to a correct float64 result, FAIL the checks the GPU test ends in -- eb.within on the per-element bounds,
    eb.in_sum_tol for the sums, gamma(npix) sum|dz| for the LeakyReLU bias gradient -- and the verdict of the whole-tensor rel-L2 at the project's
    tolerances (util.RECT_TOL) is printed beside it (run with -s): it passes the faults that touch few pixels.
"""
import numpy as np
import pytest
import torch

import elem_bound_ref as eb
import geom_ref as gr
from util import RECT_TOL, SENTINEL, rel_l2

FAMILIES = (("fwd", gr.FWD), ("bwd", gr.BWD), ("lrelu", gr.LRELU))
ROWS = [(fam, r, dt) for fam, table in FAMILIES for r in table for dt in gr.row_dts(r, fam)]
IDS = [f"{fam}-{r['id']}-{dt}" for fam, r, dt in ROWS]


def _geom(row, name, dt):
    return gr.pass_geometry(name, dt, row["batch"], row["h"], row["w"], row["c"], row["knobs"])


@pytest.mark.parametrize("fam,row,dt", ROWS, ids=IDS)
def test_row_has_the_classes_it_claims(fam, row, dt):
    assert set(row["claims"]) <= set(gr.row_passes(row, fam)), (row["id"], "claims a pass it does not run")
    for name in row["claims"]:
        g = _geom(row, name, dt)
        for cl in gr.claimed(row, name, dt):
            assert gr.CLASSES[cl](g, row["w"]), (row["id"], dt, name, cl, g)
    if row["split"] is not None:
        pooled, rank1 = row["form"].startswith("pooled"), row["form"].startswith("rank1")
        assert gr.sample_chunks(dt, row["batch"], row["h"], row["w"], row["c"], pooled, rank1, row["knobs"]["elem.chunk_mb"]) == row["split"]
        assert len(set(row["split"])) > 1 and row["knobs"]["elem.reverse"] == 1          # an uneven split under the reversed blockIdx.y


@pytest.mark.parametrize("fam,row,dt", ROWS, ids=IDS)
def test_every_pixel_is_visited_exactly_once(fam, row, dt):
    for name in gr.row_passes(row, fam):
        h, w = (row["batch"] * row["h"], row["w"]) if name == "lrelu" else (row["h"], row["w"])
        cnt, _ = gr.pass_visits(name, dt, row["batch"], row["h"], row["w"], row["c"], row["knobs"])
        assert cnt.shape == (h * w,) and (cnt == 1).all(), (row["id"], dt, name, np.flatnonzero(cnt != 1)[:8])


def test_the_shape_table_of_the_issue():
    """grid / chunk / last at batch 2 and default targets: "reduce" 1024 / 512 / 4096 (at least 16 iterations), "stream" 32768 (at least 8)"""
    def gcl(npix, c, blocks):
        g = gr.geometry(npix, 2, c, blocks)
        return (g["grid"], g["chunk"], g["last"])

    want = {(34, 38, 64): ((5, 259, 256), (10, 130, 122), (2, 162, 161)), (34, 38, 256): ((20, 65, 57), (40, 33, 5), (10, 33, 26)),
            (22, 26, 136): ((5, 115, 112), (10, 58, 50), (2, 72, 71)), (34, 38, 48): ((3, 431, 430), (7, 185, 182), None),
            (34, 38, 20): (None, (3, 431, 430), None), (17, 23, 64): (None, (3, 131, 129), None), (6, 10, 1024): ((3, 20, 20), (7, 9, 6), None),
            (6, 10, 1020): ((3, 20, 20), (7, 9, 6), None)}
    for (h, w, c), (red, stream, pool) in want.items():
        for blocks in (1024, 512, 4096):
            assert gcl(h * w, c, blocks) == (red or (1, h * w, h * w)), (h, w, c, blocks)
        assert gcl(h * w, c, 32768) == stream, (h, w, c)
        if h % 2 == 0 and w % 2 == 0 and c < 1020:
            assert gcl((h // 2) * (w // 2), c, 32768) == (pool or (1, h * w // 4, h * w // 4)), (h, w, c)
    assert gr.geometry(34 * 38, 2, 64, 32768)["rem"] == 2 and gr.geometry(34 * 38, 2, 64, 1024)["rem"] == 3
    assert gr.geometry(34 * 38, 2, 256, 32768)["PP"] == 4 and gr.geometry(22 * 26, 2, 136, 4096)["active"] == 238
    assert gr.geometry(34 * 38, 2, 48, 4096)["active"] == 252 and gr.geometry(34 * 38, 2, 48, 4096)["PP"] == 21 and gr.geometry(34 * 38, 2, 20, 4096)["PP"] == 51
    assert gr.geometry(60, 2, 1020, 4096)["active"] == 255 and not gr.wide8(gr.BF16, 1020)
    assert gr.pass_geometry("lrelu", gr.F32, 2, 34, 38, 1024)["grid"] > gr.LRELU_RED_SLOTS


# which passes read which knob, and the values the GPU test is to cover
KNOBS = {
    "elem.reverse": ((0, 1), ("apply", "pool", "reduce")),
    "elem.interleave": ((0, 1), ("reduce", "bwd_apply")),
    "elem.nt_loads": ((1,), ("bwd_apply",)),
    "elem.reduce_blocks": ((1, 3, 1 << 20), ("reduce",)),
    "elem.apply_blocks": ((256, 1 << 20), ("bwd_apply",)),
    "elem.stream_blocks": ((256, 1 << 20), ("apply", "pool")),
    "elem.chunk_mb": ((1,), ("reduce", "bwd_apply")),
}


@pytest.mark.parametrize("knob", sorted(KNOBS))
def test_every_knob_value_sits_on_a_ragged_multi_block_row(knob):
    """of every pass that reads it, in fp32 and bf16 (interleave: the bf16 forms, the only readers).  "Ragged multi-block": at least two blocks and
    a shorter last chunk or a chunk that is no multiple of the pixel slots -- except "elem.reduce_blocks" = 1 and 3, whose point is the long chunk."""
    values, passes = KNOBS[knob]
    for val in values:
        for name in passes:
            for dt in (gr.F32, gr.BF16):
                if knob == "elem.interleave" and dt == gr.F32:
                    continue
                hit = False
                for fam, table in FAMILIES:
                    for r in table:
                        if name not in gr.row_passes(r, fam) or dt not in gr.row_dts(r, fam) or dict(gr.DEFAULTS, **r["knobs"])[knob] != val:
                            continue
                        g = _geom(r, name, dt)
                        ragged = g["grid"] >= 2 and (g["last"] < g["chunk"] or g["rem"] != 0)
                        hit = hit or ragged or (knob == "elem.reduce_blocks" and val in (1, 3))
                assert hit, (knob, val, name, dt)


# =====================================================================================================================
# modelled faults on a correct float64 result
def _rnd(a, dt):
    if dt == "bf16":
        return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(torch.bfloat16).double().numpy()
    return np.asarray(a, np.float32).astype(np.float64)


def _operands(dt, n=2, h=34, w=38, c=64, seed=3):
    rng = np.random.default_rng(seed)
    a = _rnd(rng.standard_normal((n, h, w, c)) * rng.uniform(0.5, 2.0, (n, 1, 1, c)) + rng.uniform(-1, 1, (n, 1, 1, c)), dt)
    stats = np.stack([a.mean((1, 2)), 1.0 / np.sqrt(a.var((1, 2)) + 1e-6)], -1)
    g = _rnd(rng.standard_normal((n, h, w, c)), dt)
    beta = _rnd(rng.standard_normal(c) * 0.02, "f32")
    return a, stats, g, beta


def _verdicts(bad, ref, tol, dt, where, what):
    """(rel-L2 at the project's tolerance accepts, the OutOfBound of `within` or None)"""
    l2 = rel_l2(bad, ref) < RECT_TOL[dt]
    try:
        eb.within(bad, ref, tol, where, what)
        err = None
    except eb.OutOfBound as e:
        err = e
    print(f"{what} [{dt}]: rel-L2 {rel_l2(bad, ref):.2e} ({'PASSES' if l2 else 'caught'}); within: {'PASSES' if err is None else err}")
    return l2, err


def _dz(a, stats, g, m1=None, m2=None, slope=0.2):
    """in_bwd_ref_tol's expression, with the two means replaced where given"""
    n, c = a.shape[0], a.shape[-1]
    mean, inv = eb._stats_f(stats, n, c)
    xh = (a - mean) * inv
    m1 = g.mean((1, 2), keepdims=True) if m1 is None else m1
    m2 = (g * xh).mean((1, 2), keepdims=True) if m2 is None else m2
    return np.where(a > 0, 1.0, slope) * inv * (g - m1 - xh * m2), xh


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_last_pixel_slot_of_the_last_chunk_left_unwritten(dt):
    """in_apply and in_bwd: the last slot of the last sample keeps the sentinel the output was filled with -- or, harder to see, a result of the
    right size that belongs to another pixel (what a buffer that is reused holds)"""
    a, stats, g, beta = _operands(dt)
    g_app = gr.pass_geometry("apply", dt, 2, 34, 38, 64)
    where = {"kind": "in", "chunk": g_app["chunk"]}
    ref, tol = eb.in_apply_ref_tol(a, stats, beta, dt)
    zr, ztol = eb.in_bwd_ref_tol(a, stats, g, slope=0.2, dt=dt)
    for what, r, t in (("in_apply", ref, tol), ("in_bwd dz", zr, ztol)):
        assert eb.within(r, r, t, where, what) == 0.0
        for fill, name in ((SENTINEL, "sentinel"), (None, "stale")):
            bad = r.copy()
            bad[-1, -1, -1, :] = fill if fill is not None else r[-1, 0, 0, :]
            l2, err = _verdicts(bad, r, t, dt, where, f"{what}: last pixel slot {name}")
            assert err is not None and err.index[:3] == (1, 33, 37) and "last pixel slot" in err.classes, err
    # the sums built from a dz whose last slot is missing: the bias gradient and the per-sample sums.  fp32: in_sum_tol sees one pixel of 2584.
    # bf16: it cannot -- every summand may be off by its own output rounding, 2^-8 |dz|, and 1292 of those outweigh one summand; there the
    # missing slot is the business of the per-element check above (and of the sentinel the GPU test fills dz with)
    bad = zr.copy()
    bad[-1, -1, -1, :] = 0.0
    for axes, what in (((0, 1, 2), "dbias"), ((1, 2), "dz sums")):
        try:
            eb.within(bad.sum(axes), zr.sum(axes), eb.in_sum_tol(zr, ztol, axes), None, what + " without the last slot")
            caught = False
        except eb.OutOfBound as e:
            caught = True
            print(e)
        print(f"{what} without the last pixel slot [{dt}]: in_sum_tol {'catches it' if caught else 'PASSES it'}")
        assert caught or dt == "bf16"


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("c", [64, 256])
def test_last_chunk_dropped_from_the_reduce_sums(dt, c):
    a, stats, g, _ = _operands(dt, c=c)
    gm = gr.pass_geometry("reduce", dt, 2, 34, 38, c, {"elem.interleave": 0})
    assert gm["grid"] >= 3 and gm["last"] < gm["chunk"]
    hw, keep = 34 * 38, (gm["grid"] - 1) * gm["chunk"]
    zr, ztol = eb.in_bwd_ref_tol(a, stats, g, slope=0.2, dt=dt)
    _, xh = _dz(a, stats, g)
    gf, gx = g.reshape(2, hw, c), (g * xh).reshape(2, hw, c)
    m1 = (gf[:, :keep].sum(1) / hw).reshape(2, 1, 1, c)
    m2 = (gx[:, :keep].sum(1) / hw).reshape(2, 1, 1, c)
    bad = _dz(a, stats, g, m1, m2)[0]
    l2, err = _verdicts(bad, zr, ztol, dt, {"kind": "in", "chunk": gm["chunk"]}, f"in_bwd dz, c = {c}: sums without the last chunk of {gm['last']} pixels")
    assert err is not None and err.count > bad.size // 2          # every pixel of the sample carries the wrong means
    with pytest.raises(eb.OutOfBound):
        eb.within(bad.sum((0, 1, 2)), zr.sum((0, 1, 2)), eb.in_sum_tol(zr, ztol, (0, 1, 2)), None, "dbias")
    with pytest.raises(eb.OutOfBound):
        eb.within(bad.sum((1, 2)), zr.sum((1, 2)), eb.in_sum_tol(zr, ztol, (1, 2)), None, "dz sums")


@pytest.mark.parametrize("dt", ["bf16"])
def test_one_interleave_tile_counted_twice(dt):
    a, stats, g, _ = _operands(dt)
    gm = gr.pass_geometry("reduce", dt, 2, 34, 38, 64)
    assert gm["interleave"] and gm["ntiles"] >= 2
    hw, c, tile = 34 * 38, 64, gm["tile"]
    zr, ztol = eb.in_bwd_ref_tol(a, stats, g, slope=0.2, dt=dt)
    _, xh = _dz(a, stats, g)
    gf, gx = g.reshape(2, hw, c), (g * xh).reshape(2, hw, c)
    t0 = (gm["ntiles"] - 1) * tile                                  # the last whole tile, once more
    m1 = ((gf.sum(1) + gf[:, t0:t0 + tile].sum(1)) / hw).reshape(2, 1, 1, c)
    m2 = ((gx.sum(1) + gx[:, t0:t0 + tile].sum(1)) / hw).reshape(2, 1, 1, c)
    bad = _dz(a, stats, g, m1, m2)[0]
    l2, err = _verdicts(bad, zr, ztol, dt, {"kind": "in", "chunk": tile}, f"in_bwd dz: a tile of {tile} pixels twice in the sums")
    assert err is not None
    with pytest.raises(eb.OutOfBound):
        eb.within(bad.sum((1, 2)), zr.sum((1, 2)), eb.in_sum_tol(zr, ztol, (1, 2)), None, "dz sums")


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_tail_pixels_with_the_neighbouring_samples_mean(dt):
    """in_apply: the pixels a tail loop handles (geom_ref.visits) are normalised with the other sample's mean"""
    a, stats, g, beta = _operands(dt)
    gm = gr.pass_geometry("apply", dt, 2, 34, 38, 64)
    _, tail = gr.pass_visits("apply", dt, 2, 34, 38, 64)
    assert 0 < tail.sum() < tail.size // 4
    ref, tol = eb.in_apply_ref_tol(a, stats, beta, dt)
    other, _ = eb.in_apply_ref_tol(a, stats[::-1].copy(), beta, dt)          # every pixel with the other sample's statistics ...
    inv_own = eb._stats_f(stats, 2, 64)[1]
    inv_other = eb._stats_f(stats[::-1].copy(), 2, 64)[1]
    other = (other - beta) / inv_other * inv_own + beta                         # ... but its own inv: only the mean is the neighbour's
    bad = ref.copy().reshape(2, -1, 64)
    bad[:, tail] = other.reshape(2, -1, 64)[:, tail]
    bad = bad.reshape(ref.shape)
    l2, err = _verdicts(bad, ref, tol, dt, {"kind": "in", "chunk": gm["chunk"]}, f"in_apply: {int(tail.sum())} tail pixels per sample with the other sample's mean")
    assert err is not None and tail[err.index[1] * 38 + err.index[2]]


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_lrelu_block_64_folded_onto_nothing(dt):
    """lrelu_bwd's bias gradient: block 64 adds into staging slot 64 % 64 = 0; a fold that loses it drops one chunk of pixels from the sum"""
    n, h, w, c = 2, 34, 38, 1024
    gm = gr.pass_geometry("lrelu", dt, n, h, w, c)
    assert gm["grid"] > gr.LRELU_RED_SLOTS
    rng = np.random.default_rng(5)
    y = _rnd(rng.standard_normal((n * h * w, c)), dt)
    dy = _rnd(rng.standard_normal((n * h * w, c)), dt)
    d = np.where(y > 0, dy, dy * float(np.float32(0.2)))
    ref = d.sum(0)
    tol = eb.gamma(n * h * w) * np.abs(d).sum(0)
    assert eb.within(d.astype(np.float32).sum(0, dtype=np.float32), ref, tol, None, "lrelu dbias, summed in fp32") <= 1.0
    p0 = gr.LRELU_RED_SLOTS * gm["chunk"]
    bad = ref - d[p0:p0 + gm["chunk"]].sum(0)
    with pytest.raises(eb.OutOfBound) as e:
        eb.within(bad, ref, tol, None, f"lrelu dbias without block 64 ({gm['chunk']} pixels)")
    print(e.value, f"; rel-L2 {rel_l2(bad, ref):.2e} at {RECT_TOL[dt]}")
