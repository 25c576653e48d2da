"""The teeth of the far-extent harness (far_ref.py), shown without a GPU on a model whose addresses are 16 bits wide.

far_ref.far_model_op is pitch_ref.model_op with every access of the far tensor addressed the way the kernels address theirs: a byte offset
`(pixel * ld + channel) * esz`, here in a W = 16 bit register, with the five ways such arithmetic goes wrong.  The windows scale with W
(2^15 bytes for 2 GiB, 2^16 - 16 for the 0xfffffff0 limit, 2^16 for 4 GiB, 2^15 / 2^16 elements for E31 / E32), the bands and the chunked checks are
the ones the device test uses.  Shown: each fault fails the harness in the windows built for it, on a read and on a written tensor; and a
layout whose extent merely passes a threshold while all its pixels stay below it -- what far_ld() would produce without the straddle assertion --
sees none of them.  The device table itself is built here too (every row passes the straddle assertion at W = 32 and fits the memory bound), and
the host-side refusal that needs no operand is pinned: the pixel-count limit of finish_args and wgrad_check (the 4 GiB limit is refused on the
device, with real parents of the full refused size: test_far_gpu.py).
"""
import numpy as np
import pytest
import torch

import far_ref as F
import pitch_ref as R
from shmgan_amd import _lib
from util import SENTINEL

W, ESZ, Q, C, NPIX = 16, 4, 4, 16, 24
SMALL = 1000          # elements per chunk of the fills, copies and scans: every loop of far_ref takes several turns


def _layouts():
    """name -> (npix, ld).  The five windows at W = 16; `edge`: a W4+ layout whose pixel 33 ends exactly at byte 2^16 (33 * 496 + 16 = 2^14
    elements), the one place where a real access meets the "outside" marker's 16-byte piece; `miss`: the extent passes 2^15 bytes, no pixel does."""
    out = {w: (NPIX, F.far_ld(w, NPIX, C, ESZ, Q, W)) for w in F.WINDOWS}
    out["edge"] = (36, 496)
    out["miss"] = (NPIX, 344)
    return out


LAYOUTS = _layouts()
WINDOW_OF = {"edge": "W4+", "miss": "W2"}
ROLE = {"x1": "in", "x2": "in", "aux": "in", "y1": "out", "y2": "out"}


def test_the_scaled_windows_are_what_they_are_named():
    lay = LAYOUTS
    assert lay["W4-"][1] == 680 and NPIX * 680 * ESZ < F.lim(W) <= NPIX * 684 * ESZ
    assert F.refused_ld(NPIX, C, ESZ, Q, W) == 684
    assert (NPIX - 1) * lay["W2"][1] * ESZ >= 1 << 15 > (NPIX - 2) * lay["W2"][1] * ESZ + C * ESZ
    assert (NPIX - 1) * lay["W4+"][1] * ESZ >= 1 << 16
    assert (NPIX - 1) * lay["E31"][1] >= 1 << 15 and (NPIX - 1) * lay["E32"][1] >= 1 << 16
    n, ld = lay["edge"]
    assert (33 * ld + C) * ESZ == 1 << 16 and F.straddles(n, ld, C, (1 << 16) // ESZ)
    # `miss`: past 2^15 bytes by its extent, every pixel below: the straddle assertion is what refuses it
    n, ld = lay["miss"]
    assert n * ld * ESZ > 1 << 15 and ((n - 1) * ld + C) * ESZ <= 1 << 15
    assert not F.straddles(n, ld, C, (1 << 15) // ESZ)
    with pytest.raises(AssertionError):
        F.check_window("W2", n, ld, C, ESZ, Q, W)


def _model_run(tensor, layout, fault=None):
    """The device test's harness on the model: `tensor` in `layout`, every other tensor tight.  Returns the failed checks."""
    npix, ld_far = LAYOUTS[layout]
    shape = (1, npix, C)
    rng = np.random.default_rng(11)
    vals = {t: rng.standard_normal(shape).astype(np.float32) for t in ROLE if ROLE[t] == "in"}
    views, parents, ld, lead = {}, {}, {}, {}
    for t in ROLE:
        far = t == tensor
        ld[t] = ld_far if far else C
        win = WINDOW_OF.get(layout, layout)
        lead[t] = F.lead_for(win, shape, ld[t], ESZ, W) if far else R.up(F.guard_elems(shape), 64)
        views[t], parents[t] = F.far_view(SENTINEL if ROLE[t] == "out" else float("nan"), shape, ld[t], 0, lead[t], F.trail_for(shape), torch.float32, "cpu", SMALL)
        if ROLE[t] == "in":
            F.scatter(views[t], torch.from_numpy(vals[t]), SMALL)
            assert torch.equal(F.gather(views[t], SMALL), torch.from_numpy(vals[t]))
    flat = {t: p.numpy() for t, p in parents.items()}
    red = F.far_model_op(flat, lead, ld, npix, ESZ, W, fault, on=(tensor,), hw=npix // 3)
    y1, y2, rr = R.model_reference(vals["x1"].astype(np.float64), vals["x2"].astype(np.float64), vals["aux"].astype(np.float64))
    bad = []
    for t, ref in (("y1", y1), ("y2", y2)):
        got = F.gather(views[t], SMALL).numpy().astype(np.float64)
        if not np.array_equal(got, ref.astype(np.float32).astype(np.float64)):
            bad.append(t + " values")
        if not F.far_outside_untouched(parents[t], shape, ld[t], 0, lead[t], SENTINEL, SMALL):
            bad.append(t + " outside")
    if not np.allclose(red, rr, rtol=1e-6, atol=1e-6):          # (NaN compares false)
        bad.append("red")
    return bad


def test_the_clean_model_passes_every_far_layout():
    for t in ("x1", "y1", "aux"):
        for lay in LAYOUTS:
            assert _model_run(t, lay) == [], (t, lay)


# fault -> the windows that must catch it.  Bytes: W2 and W4- reach past 2^15, W4+ and edge past 2^16; with 4-byte elements E31 (2^17 bytes) and
# E32 pass both.  Elements: only E31 and E32 reach 2^15.
CAUGHT_BY = {
    "offset-wraps": ("W4+", "E31", "E32", "B31", "B32", "edge"),
    "offset-sign-extends": ("W2", "W4-", "W4+", "E31", "E32", "B31", "B32", "edge"),
    "int-element-index": ("E31", "E32", "B31", "B32"),
    "extent-clamped": ("W4+", "E31", "E32", "B31", "B32", "edge"),
    "outside-collides": ("edge",),
    # the batch term alone: in E31 the base of sample 2 is two thirds of the threshold and nothing overflows -- only B31 / B32 see it (and E32,
    # whose 2 * hw * ld passes 2^15 elements on the way to 2^16)
    "batch-term-in-int": ("B31", "B32", "E32"),
}
assert set(CAUGHT_BY) == set(F.FAR_FAULTS)


@pytest.mark.parametrize("fault", F.FAR_FAULTS)
@pytest.mark.parametrize("tensor", ["x1", "y1"])
def test_every_address_fault_fails_the_harness_in_its_windows(fault, tensor):
    for lay in CAUGHT_BY[fault]:
        bad = _model_run(tensor, lay, fault)
        assert bad, (fault, tensor, lay)
        if tensor == "y1":
            assert "y1 values" in bad, (fault, lay, bad)          # the pixel past the threshold was never written where it belongs
    # a stray store below the base lands in the lead band, which is what the band is sized for: seen there, not as a fault
    if tensor == "y1" and fault in ("offset-sign-extends", "int-element-index"):
        assert "y1 outside" in _model_run("y1", CAUGHT_BY[fault][0], fault)
    # ... and the layout whose pixels all sit below the threshold sees nothing: why far_ld() asserts the straddle
    assert _model_run(tensor, "miss", fault) == [], (fault, tensor)
    # a window below a fault's threshold does not see it either (W4- is no substitute for W4+, nor a byte window for E31)
    if fault in ("offset-wraps", "extent-clamped", "int-element-index", "batch-term-in-int"):
        assert _model_run(tensor, "W4-", fault) == [], (fault, tensor)
    if fault == "batch-term-in-int":          # the gap B31 closes: the last-pixel window past 2^(W-1) elements does not see the batch term
        assert _model_run(tensor, "E31", fault) == [], (fault, tensor)


def test_chunked_checks_see_one_stray_element_anywhere():
    shape, ld, lead = (1, 24, C), 680, 8256
    for where in ("lead-first", "lead-last", "gap", "last-gap", "trail-first", "trail-last", "slice"):
        v, parent = F.far_view(SENTINEL, shape, ld, 0, lead, F.trail_for(shape), torch.float32, "cpu", SMALL)
        end = lead + 24 * ld
        i = {"lead-first": 0, "lead-last": lead - 1, "gap": lead + 11 * ld + C, "last-gap": end - 1, "trail-first": end, "trail-last": parent.numel() - 1,
             "slice": lead + 5 * ld + 3}[where]
        assert F.far_outside_untouched(parent, shape, ld, 0, lead, SENTINEL, SMALL)
        parent[i] = 1.0
        assert F.far_outside_untouched(parent, shape, ld, 0, lead, SENTINEL, SMALL) == (where == "slice"), where
        # the same bits in another sign of zero or NaN payload are a difference too: the comparison is bitwise
    v, parent = F.far_view(float("nan"), shape, ld, 0, lead, F.trail_for(shape), torch.float32, "cpu", SMALL)
    assert F.far_outside_untouched(parent, shape, ld, 0, lead, float("nan"), SMALL)
    assert F.is_far(v, SMALL) and not F.is_far(torch.zeros(1, 24, C), SMALL) and not F.is_far(torch.zeros(8), SMALL)


def test_the_device_table_straddles_every_threshold_and_fits_the_memory_bound():
    """far_ld() asserts the straddle for every row while the table is built (W = 32); restated here on the finished rows."""
    rows = 0
    for fam, _v, dt, _kn in F.conv_table():
        for cid, case, kind in F.conv_cases(fam, dt):
            (arg, far), = case.items()
            adt = F.arg_dt(fam, dt, arg)
            npix, esz = F.npix_of(fam, arg), R.ESZ[adt]
            ext = npix * far.ld * esz
            if far.window == "LIM":
                assert F.lim() <= ext < F.lim() + npix * R.Q[adt] * esz and kind in ("flat", "aux"), cid          # the first pitch past the limit
            else:
                unit, thr, _ = F.WINDOWS[far.window]
                assert all(F.straddles(npix, far.ld, F.chan_of(fam, arg), t // esz) for t in thr(32)), cid
                assert (ext < F.lim()) == (kind == "same"), cid
            assert far.ld % R.Q[adt] == 0 and F.case_bytes(fam, dt, case) + (1 << 30) <= 20 << 30, cid
            rows += 1
    for fam, dt, _kn in F.in_table():
        for cid, f, case in F.in_cases(fam, dt):
            (arg, far), = case.items()
            npix = F.npix_of(f, arg)
            T = 1 << (31 if far.window in ("E31", "B31") else 32)
            assert F.straddles(npix, far.ld, F.chan_of(f, arg), T), cid
            per = npix // 3 * far.ld
            if far.window in ("B31", "B32"):          # the batch term on its own: n = 1 ends below the threshold, n = 2 starts at or above it
                assert f["shape"]["n"] == 3 and dt == "bf16" and 2 * per - far.ld + F.chan_of(f, arg) <= T <= 2 * per, cid
            elif f["shape"]["n"] == 3:          # sample 1 ends below the threshold, sample 2 holds the crossing (its base is below: B31 / B32 have it above)
                assert 2 * per < T <= 3 * per, cid
            else:                              # one sample past 2^31 elements on its own
                assert npix * far.ld > 1 << 31, cid
            if dt == "f32":
                assert npix * far.ld * 4 > 1 << 32, cid
            assert F.case_bytes(f, dt, case) + (1 << 30) <= 20 << 30, cid
            rows += 1
    assert rows > 500, rows
    names = {f["name"] for f, _v, _dt, _kn in F.conv_table()}
    assert names == set(F.CONV_FAMILIES) and {n for n in names if n.startswith("wgrad-")} == {f["name"] for f in R.FAMILIES if f["name"].startswith("wgrad-")}
    entries = {f["entry"] for f, _dt, _kn in F.in_table()}
    assert entries == set(R.INSTNORM)


# ------------------------------------------------------------------------------------------------------------------- refusals
PTR = 1 << 20          # a non-null, 16-byte-aligned pointer nobody dereferences: the calls below answer before any launch


def _L():
    _lib.build()
    return _lib.lib()


def _refused(rc, L, *words):
    msg = L.shm_last_error()
    return rc == -1 and all(w.encode() in msg for w in words)


def test_pixel_counts_of_2_31_are_refused_on_the_host():
    """batch x 1 x 2^k pixels: no operand of that size can be held, and none is needed -- finish_args and wgrad_check answer before any launch"""
    L, p, f32 = _L(), PTR, _lib.F32

    def fwd(batch, w, s=1):
        return L.shm_conv2d_fwd(p, None, 0, 64, 0, p, None, p, 64, batch, 1, w, 64, 64, 3, s, 1.0, f32, None)

    assert _refused(fwd(1 << 15, 1 << 16), L, "pixel count overflows int32")
    assert _refused(L.shm_conv2d_transpose_fwd(p, 64, p, None, p, 64, 1 << 14, 1, 1 << 15, 64, 64, 1.0, f32, None), L, "pixel count overflows int32")   # (the output's)
    assert _refused(L.shm_conv2d_dgrad(p, 64, p, p, None, 0, 64, 0, 1 << 15, 1, 1 << 16, 64, 64, 3, 1, f32, None), L, "pixel count overflows int32")
    big = 1 << 40

    def wgrad(batch, w):
        return L.shm_conv2d_wgrad(p, None, 0, 64, 0, p, 64, p, batch, 1, w, 64, 64, 64, 3, 1, 0, p, big, f32, None)

    assert _refused(wgrad(1 << 15, 1 << 16), L, "pixel count overflows int32")
