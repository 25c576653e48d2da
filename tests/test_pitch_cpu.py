"""CPU checks behind test_pitch_gpu.py (pitch_ref.py): the predicates restated there still stand in the kernel sources as text; the case
table flips every term of every predicate alone and varies every pitch argument of every entry point; the harness catches each modelled
addressing fault on a NumPy model of a pitched NHWC op and passes the clean model in every layout; and the entry points refuse, before
any launch, the pitches and bases the header excludes."""
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import pitch_ref as R
from shmgan_amd import _lib
from util import SENTINEL

CSRC = Path(__file__).resolve().parent.parent / "shmgan_amd" / "csrc"
PTR = 1 << 20          # a non-null, 16-byte-aligned pointer nobody dereferences: the calls below answer before any launch


def _statement(src, start):
    """The statement of `src` that begins with `start`, white space collapsed."""
    i = src.index(start)
    return re.sub(r"\s+", " ", src[i:src.index(";", i)])


# ------------------------------------------------------------------------------------------------------------------- the text pins
def test_restated_predicates_are_the_sources():
    """Each term pitch_ref models stands in the source expression it restates.  A failure after a predicate was edited is no regression
    of the kernels: re-read the expression, update pitch_ref.py's restatement (and the snippet here), and check with the coverage test below
    that the table still flips every term."""
    halo, dma, ph4, igemm, bwd = ((CSRC / n).read_text() for n in ("conv_halo.hip", "conv_dma.hip", "conv_phase4.hip", "conv_igemm.hip", "instnorm_bwd.hip"))
    src_term = {"nout % 8": "(a.nout % 8 == 0)", "n1 % 8": "(a.n1 % 8 == 0)", "ldy % 8": "(a.ldy % 8 == 0)", "y & 15": "(((size_t)a.y & 15) == 0)",
                "ldy2 % 8": "(a.ldy2 % 8 == 0)", "y2 & 15": "(((size_t)a.y2 & 15) == 0)"}
    for src in (halo, dma):
        stmt = _statement(src, "const bool wide = kWide")
        for name in R.epilogue_terms(64, 32, 32, 0, 32, 0):
            assert src_term[name] in stmt, name
        assert stmt.count("==") == 7 and "a.y2 == nullptr ||" in stmt                 # the six terms and the null test: nothing the restatement lacks
    stmt = _statement(ph4, "const bool wide = kWide")
    assert stmt == "const bool wide = kWide && (a.ldy % 8 == 0) && (((size_t)a.y & 15) == 0)" and set(R.epilogue_terms(64, 64, 64, 0, phase4=True)) == {"ldy % 8", "y & 15"}
    stmt = _statement(igemm, "const bool wreg_ok =")
    for t in ("a.nout % 64 == 0", "a.n1 % 32 == 0", "a.ldy % 8 == 0", "((size_t)a.y & 15) == 0", "a.ldy2 % 8 == 0", "((size_t)a.y2 & 15) == 0", "oesz == 4 ||"):
        assert t in stmt, t
    assert set(R.wreg_terms(64, 64, 64, 0, 64, 0)) == {"nout % 64", "n1 % 32", "ldy % 8", "y & 15", "ldy2 % 8", "y2 & 15"}
    assert "if (a.gred[p]) al = al && (oesz == 4 || (a.ldgaux[p] % 8 == 0 && ((size_t)a.gaux[p] & 15) == 0));" in igemm
    stmt = _statement(igemm, "const bool wide_ok =")
    for name in R.epilogue_terms(64, 32, 32, 0, 32, 0):
        assert src_term[name] in stmt, name
    assert stmt.startswith("const bool wide_ok = oesz == 4 ||") and "al = al && wide_ok;" in igemm
    assert set(R.gsum_terms("bf16", [(64, 0), (64, 0)], 128, 64, 64, 0, 64, 0)) == \
        {"ldgaux[0] % 8", "gaux[0] & 15", "ldgaux[1] % 8", "gaux[1] & 15"} | {"wide_ok: " + k for k in src_term}
    assert R.gsum_terms("f32", [(64, 0)], 64, 64, 64, 0) == {}
    wg = (CSRC / "conv_wgrad.hip").read_text()
    assert "9 * cin <= kWgradThinRows && s.ldx == 16 && cin_ld <= 16 &&" in _statement(wg, "const bool thin_ok =") and R.wgrad_thin_pitch(16) and not R.wgrad_thin_pitch(20)
    # (src16's last term, 16-byte-aligned sources, is not modelled: input bases stay aligned in every case and no misaligned one is run)
    assert "const bool src16 = (q.r1 || q.ldg1 % 8 == 0) && q.lda % 8 == 0 && (!q.g2 || q.ldg2 % 8 == 0) && q.src_al16;" in bwd
    assert "(((size_t)g1 | (size_t)g2 | (size_t)a) & 15) == 0, ((size_t)dz & 15) == 0}" in bwd
    assert "p.wide8 = (q.dtype == SHM_BF16 || q.dtype == SHM_BF16_GF32) && c % 8 == 0 && src16;" in bwd
    assert "&& src16 && q.lddz % 8 == 0 && q.dz_al16 &&" in _statement(bwd, "const bool base_ok =")
    assert f'p.name = p.wide8 ? "{R.R8}" : "{R.R4}";' in bwd
    assert set(R.in_bwd_terms(64, 64, 64, 64)) == {"ldg1 % 8", "lda % 8", "lddz % 8", "ldg2 % 8", "dz & 15"} and "ldg1 % 8" not in R.in_bwd_terms(None, 64, 64, rank1=True)


def test_predicates_name_the_expected_kernels():
    assert R.epilogue("bf16", 64, 64, 64, 0) == "wide16" and R.epilogue("f32", 64, 64, 64, 0) == "element"
    assert R.epilogue("bf16", 64, 64, 72, 8) == R.epilogue("bf16", 64, 64, 68, 0) == R.epilogue("bf16", 12, 12, 16, 0) == "element"
    assert R.epilogue("bf16", 128, 64, 64, 0, 68, 0) == R.epilogue("bf16", 128, 64, 64, 0, 72, 8) == "element" and R.epilogue("bf16", 128, 64, 64, 0, 72, 0) == "wide16"
    assert R.wreg_family("bf16", "bf16", 64, 64, 72, 8) == "halo" and R.wreg_family("bf16", "bf16", 64, 64, 72, 0) == "wreg"
    assert R.wreg_family("bf16", "f32", 64, 64, 68, 8) == R.wreg_family("f32", "f32", 64, 64, 68, 8) == "wreg"
    assert R.gsum_path("bf16", [(72, 8)], 64, 64, 64, 0) == R.gsum_path("bf16", [(68, 0)], 64, 64, 64, 0) == R.gsum_path("bf16", [(64, 0)], 64, 64, 72, 8) == "reduce"
    assert R.gsum_path("bf16", [(72, 0)], 64, 64, 64, 0) == R.gsum_path("f32", [(68, 4)], 64, 64, 68, 4) == "epilogue"
    F8 = "in_bwd_fused8_kernel<false>"
    assert R.in_bwd_form("bf16", 64, 72, 64, 64, one_pass=F8) == F8 and R.in_bwd_form("bf16", 64, 72, 64, 64) == R.R8
    assert R.in_bwd_form("bf16", 64, 64, 64, 68, one_pass=F8) == R.R8                 # lddz alone: two passes, still eight channels per thread
    assert R.in_bwd_form("bf16", 64, 64, 64, 72, one_pass=F8, dz=8) == R.R8 and R.in_bwd_form("bf16", 64, 64, 64, 72, one_pass=F8, dz=16) == F8          # ... so does an 8-byte-aligned dz
    for ldg1, lda, ldg2 in ((68, 64, None), (64, 68, None), (64, 64, 68)):
        assert R.in_bwd_form("bf16", 64, ldg1, lda, 64, ldg2, one_pass=F8) == R.R4
    assert R.in_bwd_form("bf16", 12, 16, 16, 16) == R.R4 and R.in_bwd_form("f32", 64, 64, 64, 64) == R.R4
    assert R.in_bwd_form("bf16", 64, None, 68, 64, rank1=True) == R.R4 and R.in_bwd_form("bf16", 64, None, 64, 68, rank1=True) == R.R8


# ----------------------------------------------------------------------------------------------------------------- the layouts
def test_layouts_are_inside_the_contract():
    for dt, q in R.Q.items():
        for c in (3, 12, 16, 20, 40, 48, 64, 160, 1024):
            for kind in R.LAYOUTS:
                ld, off = R.layout(kind, c, dt)
                assert ld >= off + c and ld % 4 == 0, (kind, c, dt)
                if kind in ("tight", "wide", "slice", "odd-wide", "wide2", "slice3"):
                    assert ld % q == 0 and off * R.ESZ[dt] % 16 == 0, (kind, c, dt)            # the header's multiples; 16-byte-aligned bases
            assert R.layout("tight", c, dt) == (R.up(c, q), 0) and R.layout("wide", c, dt)[0] == R.up(c, q) + q
            assert R.layout("slice", c, dt) == (2 * R.up(c, q), R.up(c, q)) and R.layout("odd-wide", c, dt)[0] == R.up(c, q) + 3 * q
        ld, off = R.layout("half", 64, "bf16")
        assert ld % 8 == 0 and off * 2 % 16 == 8                                                # flips (y & 15) alone
        assert R.layout("plus4", 64, "bf16")[0] % 8 == 4 and R.layout("plus4", 64, "bf16")[0] % 8 == 4
    # inputs never get an unaligned base
    for fam, variant, dt, kn, cid, case in R.table():
        for a in R.ENTRY_POINTS[fam["entry"]]["in"]:
            if a in case:
                assert R.addr16(case, a, fam["ch"][a], dt) == 0 and case[a] != "half", (fam["name"], cid)


def test_view_and_untouched_check():
    for dt in (torch.float32, torch.bfloat16):
        for kind in ("tight", "wide", "slice", "half"):
            shape = (2, 3, 5, 16)
            ld, off = R.layout(kind, 16, dt)
            v, parent = R.view_of(float("nan"), shape, ld, off, None, dt)
            lead = R.lead_elems(shape, ld)
            assert parent.numel() == 2 * lead + 30 * ld and lead >= 30 * ld and lead % 64 == 0
            assert v.shape == shape and v.stride() == (15 * ld, 5 * ld, ld, 1) and v.storage_offset() == lead + off
            assert (v.data_ptr() - parent.data_ptr()) == (lead + off) * parent.element_size()
            assert bool(torch.isnan(parent).all()) and R.outside_untouched(parent, shape, ld, off, None, float("nan"))
            v.copy_(torch.arange(480).view(shape).to(dt))
            assert R.outside_untouched(parent, shape, ld, off, None, float("nan")) and int(torch.isnan(parent).sum()) == parent.numel() - 480
            o, po = R.view_of(SENTINEL, shape, ld, off, None, dt)
            o.zero_()
            assert R.outside_untouched(po, shape, ld, off)
            spots = [0, lead - 1, lead + 30 * ld, po.numel() - 1]                        # both ends of both bands
            if off:
                spots += [lead, lead + off - 1, lead + 29 * ld]                       # the front gap of the first and last pixel
            if ld > off + 16:
                spots += [lead + off + 16, lead + ld - 1, lead + 30 * ld - 1]         # the back gap
            for i in spots:
                keep = po[i].clone()
                po[i] = 1.0
                assert not R.outside_untouched(po, shape, ld, off), (kind, i)
                po[i] = -SENTINEL                                                   # bit-equal, not value-equal ...
                assert not R.outside_untouched(po, shape, ld, off), (kind, i)
                po[i] = keep
            assert R.outside_untouched(po, shape, ld, off)
    z, pz = R.view_of(0.0, (4, 8), 8, 0, None, torch.float32)
    pz[0] = -0.0                                                                       # ... so a -0.0 over a 0.0 fill counts
    assert not R.outside_untouched(pz, (4, 8), 8, 0, None, 0.0)


# -------------------------------------------------------------------------------------------------------------------- coverage
def test_every_pitch_argument_varies_alone_and_all_differ():
    seen = {}
    for fam, variant, dt, kn, cid, case in R.table():
        args = tuple(fam["ch"])
        assert set(case) <= set(args), (fam["name"], cid)
        for a in case:
            ld, off = R.layout(case[a], fam["ch"][a], R.out_dt(fam, dt) if a in R.ENTRY_POINTS[fam["entry"]]["out"] else dt)
            if ld != fam["ch"][a]:
                seen.setdefault((fam["entry"], dt, a), set()).add(len(case))
    for entry, roles in R.ENTRY_POINTS.items():
        for dt in R.BOTH:
            for a in roles["in"] + roles["out"] + roles["aux"]:
                got = seen.get((entry, dt, a)) or (seen.get(("conv2d_in_fwd", dt, a)) if entry == "conv2d_fwd" else None)
                assert got and 1 in got, (entry, dt, a)               # ... differs from its channel count in a case that varies nothing else
    # the full case list of an entry point: a tight control, every argument alone in three layouts, one case where no two pitches agree
    for entry, roles in R.ENTRY_POINTS.items():
        every = roles["in"] + roles["out"] + roles["aux"]
        for dt in R.BOTH:
            cs = dict(R.cases(entry, dt))
            assert cs["tight"] == {}
            for a in every:
                assert all(cs[f"{a}-{k}"] == {a: k} for k in R.INPUT_KINDS)
                assert (f"{a}-half" in cs) == (dt == "bf16" and a not in roles["in"])
            if len(every) > 1:
                lds = [R.layout(cs["all-different"][a], 64, dt)[0] for a in every]
                assert len(set(lds)) == len(lds) and 64 not in lds, (entry, dt, lds)


def _alone(term_sets):
    """{term: True if some case has exactly that term false}, and whether some case has none false"""
    false_sets = [frozenset(k for k, v in t.items() if not v) for t in term_sets]
    names = set().union(*[set(t) for t in term_sets])
    return {n: frozenset([n]) in false_sets for n in names}, frozenset() in false_sets


def test_the_table_flips_every_term_of_every_predicate_alone():
    tab = [r for r in R.table() if r[2] == "bf16"]
    conv = [r for r in tab if r[0]["entry"].startswith("conv2d_") and r[0]["entry"] != "conv2d_wgrad" and not r[0]["out_f32"]]
    # `wide`: halo and DMA families, one and two destinations
    alone, control = _alone([R.conv_out_terms(f, dt, case, "wide") for f, v, dt, kn, cid, case in conv if v != "phase4"])
    assert control and set(alone) == {"nout % 8", "n1 % 8", "ldy % 8", "y & 15", "ldy2 % 8", "y2 & 15"} and all(alone.values()), alone
    ph4 = [R.epilogue_terms(0, 0, R.layout(case.get(a, "tight"), f["ch"][a], dt)[0], R.addr16(case, a, f["ch"][a], dt), phase4=True)
           for f, v, dt, kn, cid, case in conv if v == "phase4" for a in (("lddx",) if f["entry"] == "conv2d_dgrad" else ("ldy",))]
    alone, control = _alone(ph4)
    assert control and alone == {"ldy % 8": True, "y & 15": True}
    # `wreg_ok`: the families entered through the automatic choice
    alone, control = _alone([R.conv_out_terms(f, dt, case, "wreg") for f, v, dt, kn, cid, case in conv if v == "auto"])
    assert control and set(alone) == {"ldy % 8", "y & 15", "ldy2 % 8", "y2 & 15"} and all(alone.values()), alone
    # gsum: `al` and `wide_ok`
    gs = [R.conv_out_terms(f, dt, case, "gsum") for f, v, dt, kn, cid, case in conv if "ldaux" in f["ch"] and "ldaux2" in f["ch"]]
    alone, control = _alone(gs)
    pitch_terms = {k for k in alone if "nout" not in k and "n1" not in k}            # (the channel-count terms of wide_ok are flipped in the plain families above)
    assert control and len(pitch_terms) == 8 and all(alone[k] for k in pitch_terms), alone
    # in_bwd: src16 and lddz % 8, two-pass and one-pass families, and the rank-1 form
    for name, want in (("in_bwd", {"ldg1 % 8", "lda % 8", "lddz % 8", "ldg2 % 8", "dz & 15"}), ("in_bwd-one-pass", {"ldg1 % 8", "lda % 8", "lddz % 8", "ldg2 % 8", "dz & 15"}),
                       ("in_bwd_rank1", {"lda % 8", "lddz % 8", "dz & 15"})):
        rows = []
        for f, v, dt, kn, cid, case in tab:
            if f["name"] == name:
                ld = {a: R.layout(case.get(a, "tight"), c, dt)[0] for a, c in f["ch"].items()}
                rows.append(R.in_bwd_terms(ld.get("ldg1"), ld["lda"], ld["lddz"], ld.get("ldg2"), name == "in_bwd_rank1", R.addr16(case, "lddz", f["ch"]["lddz"], dt)))
        alone, control = _alone(rows)
        assert control and set(alone) == want and all(alone.values()), (name, alone)


def test_the_table_has_the_issue_shapes():
    names = {f["name"] for f in R.FAMILIES}
    assert {"fwd-halo", "fwd-halo-ph8", "fwd-halo-ragged", "fwd-dma", "fwd-dma-ragged", "fwd-wreg", "fwd-wreg-f32-narrow", "fwd-flat-epilogue", "fwd-x3", "fwd-gsum-s2", "fwd-norm-exact", "fwd-norm-scaled", "dgrad-x3", "wgrad-thin", "wgrad-norm", "transpose",
            "transpose-ragged", "dgrad-s2", "dgrad-split", "dgrad-split-gf32", "dgrad-ragged", "dgrad-gsum", "dgrad-s2-gsum", "in_bwd", "in_bwd_apply", "in_bwd_rank1",
            "in_bwd-one-pass", "in_bwd-one-pass-dbias", "in_bwd-one-pass-none", "in_bwd-dbias", "in_bwd-none", "in_bwd_apply-dbias", "in_bwd_rank1-none"} <= names
    # every family under the automatic choice or an opt-in knob names the kernel its tight call must take
    for f, v, dt, kn, cid, case in R.table():
        if v == "auto" or f["name"].startswith(("wgrad-", "in_bwd-one-pass")) or "x3" in f["name"]:
            assert R.tight_kernel(f, v, dt, kn), (f["name"], v, dt)
    assert {f["shape"]["cout"] for f in R.FAMILIES if "ragged" in f["name"] and "cout" in f["shape"] and "cin" not in f["shape"]} == {3, 12, 20}
    assert {(f["shape"]["cin"], f["shape"]["n1"]) for f in R.FAMILIES if f["name"] == "dgrad-ragged"} == {(32, 12), (64, 40), (20, 8)}
    assert {v for f in R.FAMILIES if f["name"] == "fwd-dma" for v in f["variants"]} == set(R.DMA) and len(R.DMA) == 8
    for f in R.FAMILIES:
        assert f["shape"]["n"] >= 2                                   # blocks cross an image boundary
    assert len(list(R.table())) > 2000


# ---------------------------------------------------------------------------------------------------------------- the fault model
MODEL_C = {"x1": 16, "x2": 16, "aux": 16, "y1": 16, "y2": 16}
MODEL_ROLE = {"x1": "in", "x2": "in", "aux": "aux", "y1": "out", "y2": "out"}
MODEL_CASES = [("tight", {})] + [(f"{t}-{k}", {t: k}) for t in MODEL_C for k in R.INPUT_KINDS] + \
    [("all-different", {"x1": "wide", "x2": "slice", "aux": "odd-wide", "y1": "wide2", "y2": "slice3"})]


def _model_run(case, fault=None):
    """The harness on the NumPy model, as test_pitch_gpu.py runs it on the device.  Returns the list of failed checks."""
    shape = (2, 3, 4)
    npix = 24
    rng = np.random.default_rng(5)
    vals = {t: rng.standard_normal(shape + (c,)).astype(np.float32) for t, c in MODEL_C.items() if MODEL_ROLE[t] != "out"}
    views, parents, ld, off, lead = {}, {}, {}, {}, {}
    for t, c in MODEL_C.items():
        ld[t], off[t] = R.layout(case.get(t, "tight"), c, "f32")
        lead[t] = R.lead_elems(shape + (c,), ld[t])
        views[t], parents[t] = R.view_of(SENTINEL if MODEL_ROLE[t] == "out" else float("nan"), shape + (c,), ld[t], off[t], None, torch.float32)
        if MODEL_ROLE[t] != "out":
            views[t].copy_(torch.from_numpy(vals[t]))
    flat = {t: p.numpy() for t, p in parents.items()}
    ptr = {t: lead[t] + off[t] for t in MODEL_C}
    red = R.model_op(flat, R.model_faulted_base(ptr, off, fault), ld, npix, fault)
    R.model_stray_store(flat, ptr, ld, lead, npix, fault)
    y1, y2, rr = R.model_reference(vals["x1"].astype(np.float64), vals["x2"].astype(np.float64), vals["aux"].astype(np.float64))
    bad = []
    for t, ref in (("y1", y1), ("y2", y2)):
        got = views[t].numpy().astype(np.float64)
        if not np.array_equal(got, ref.astype(np.float32).astype(np.float64)):
            bad.append(t + " values")
        if not R.outside_untouched(parents[t], shape + (MODEL_C[t],), ld[t], off[t]):
            bad.append(t + " outside")
    if not np.allclose(red, rr, rtol=1e-6, atol=1e-6):          # (NaN compares false)
        bad.append("red")
    return bad


def test_the_clean_model_passes_every_layout():
    for cid, case in MODEL_CASES:
        assert _model_run(case) == [], cid


@pytest.mark.parametrize("fault", R.FAULTS)
def test_every_modelled_fault_fails_the_harness(fault):
    caught = {cid: _model_run(case, fault) for cid, case in MODEL_CASES}
    assert any(caught.values()), fault
    # ... and by the case that varies the pitch in question alone, not only by the all-different one
    alone = {"read-pitch-is-channels": "x1-wide", "write-pitch-is-channels": "y1-wide", "src1-pitch-for-src2": "x2-wide", "part1-pitch-for-part2": "y2-wide",
             "aux-pitch-is-out-pitch": "aux-wide", "base-offset-dropped": "y1-slice", "store-into-gap": "y1-wide", "store-into-lead-band": "tight",
             "store-into-trail-band": "tight", "read-of-gap": "x1-wide"}[fault]
    assert caught[alone], (fault, alone)
    assert caught["all-different"] or fault in ("base-offset-dropped",), fault          # (its y1 and x1 sit at offset 0 there)
    if fault in ("store-into-gap", "store-into-lead-band", "store-into-trail-band"):
        assert caught[alone] == ["y1 outside"]                                            # only the untouched check sees a stray store
    if fault == "src1-pitch-for-src2":
        assert not caught["tight"]                                                        # a tight call cannot see it at all: the gap this module closes
    if fault in ("read-pitch-is-channels", "write-pitch-is-channels", "part1-pitch-for-part2", "aux-pitch-is-out-pitch", "read-of-gap", "store-into-gap"):
        assert not caught["tight"], fault


# ------------------------------------------------------------------------------------------------------------------- refusals
def _L():
    _lib.build()
    return _lib.lib()


def _refused(rc, L, *words):
    msg = L.shm_last_error()
    return rc == -1 and all(w.encode() in msg for w in words)


def test_conv_entry_points_refuse_a_pitch_below_the_channels():
    L, p, f32, bf = _L(), PTR, _lib.F32, 1

    def fwd(ldx=64, ldx2=0, ldy=64, x2=None, c1=0, cin=64, cout=64, dt=f32, x=p):
        return L.shm_conv2d_fwd(x, x2, c1, ldx, ldx2, p, None, p, ldy, 1, 16, 16, cin, cout, 3, 1, 1.0, dt, None)

    assert _refused(fwd(ldy=60), L, "output pitch 60", "64 channels")
    assert _refused(fwd(ldx=48), L, "input pitch 48", "64 channels")
    assert _refused(fwd(ldx=64, ldx2=32, x2=p, c1=64, cin=128), L, "second source", "64 channels")
    assert _refused(fwd(ldx=32, ldx2=64, x2=p, c1=64, cin=128), L, "input pitch 32")
    assert _refused(fwd(cout=12, ldy=8), L, "output pitch 8", "12 channels")
    assert _refused(fwd(x=p + 8), L, "16-byte aligned") and _refused(fwd(x2=p + 4, c1=32, ldx=32, ldx2=32), L, "16-byte aligned")
    # the compact RGB image stays: one 16-byte chunk per pixel under a 64-byte weight row, either type -- and nothing else below the channels
    assert _refused(L.shm_conv2d_fwd(p, None, 0, 4, 0, p, None, p, 8, 1, 16, 16, 16, 16, 3, 2, 1.0, f32, None), L, "output pitch 8")
    assert _refused(L.shm_conv2d_fwd(p, None, 0, 8, 0, p, None, p, 8, 1, 16, 16, 32, 16, 3, 2, 1.0, bf, None), L, "output pitch 8")
    assert _refused(L.shm_conv2d_fwd(p, None, 0, 8, 0, p, None, p, 16, 1, 16, 16, 32, 16, 3, 2, 1.0, f32, None), L, "input pitch 8")
    assert _refused(L.shm_conv2d_fwd(p, None, 0, 16, 0, p, None, p, 16, 1, 16, 16, 64, 16, 3, 2, 1.0, bf, None), L, "input pitch 16")

    def dgrad(lddy=64, lddx=64, lddx2=64, dx2=p, n1=64, cin=128):
        return L.shm_conv2d_dgrad(p, lddy, p, p, dx2, n1, lddx, lddx2, 1, 16, 16, cin, 64, 3, 1, f32, None)

    assert _refused(dgrad(lddy=32), L, "input pitch 32")
    assert _refused(dgrad(lddx=60), L, "output pitch 60") and _refused(dgrad(lddx2=60), L, "second part", "64 channels")
    assert _refused(dgrad(n1=12, cin=32, lddx=8, lddx2=20), L, "output pitch 8", "12 channels")
    assert _refused(dgrad(n1=12, cin=32, lddx=12, lddx2=16), L, "second part", "20 channels")
    # one destination (dx2 NULL, lddx2 = 0 as callers pass it): the whole of cin is held against lddx
    assert _refused(dgrad(dx2=None, lddx2=0, cin=64, lddx=60), L, "output pitch 60", "64 channels")
    rc = L.shm_conv2d_dgrad_gsum(p, 64, p, p, p, 64, 64, 64, 1, 16, 16, 128, 64, 3, 1, p, 60, p, None, 0, None, f32, None)
    assert _refused(rc, L, "aux pitch 60", "64 channels")
    rc = L.shm_conv2d_dgrad_gsum(p, 64, p, p, p, 96, 96, 32, 1, 16, 16, 128, 64, 3, 1, None, 0, None, p, 28, p, f32, None)
    assert _refused(rc, L, "aux pitch 28", "32 channels")
    rc = L.shm_conv2d_fwd_gsum(p, None, 0, 64, 0, p, None, p, 64, 1, 16, 16, 64, 64, 3, 2, 1.0, p, 32, p, f32, None)
    assert _refused(rc, L, "aux pitch 32")
    assert _refused(L.shm_conv2d_transpose_fwd(p, 64, p, None, p, 16, 1, 16, 16, 64, 20, 1.0, f32, None), L, "output pitch 16", "20 channels")
    assert _refused(L.shm_conv2d_transpose_fwd(p, 32, p, None, p, 64, 1, 16, 16, 64, 64, 1.0, f32, None), L, "input pitch 32")


def test_wgrad_refuses_a_pitch_below_the_channels():
    L, p, f32, bf = _L(), PTR, _lib.F32, 1
    big = 1 << 30

    def wgrad(ldx=64, ldx2=0, lddy=64, x2=None, c1=0, cin=64, cin_ld=64, cout=64, dt=f32, x=p, dy=p, s=1):
        return L.shm_conv2d_wgrad(x, x2, c1, ldx, ldx2, dy, lddy, p, 1, 16, 16, cin, cin_ld, cout, 3, s, 0, p, big, dt, None)

    assert _refused(wgrad(lddy=32), L, "gradient pitch 32", "64 channels")
    assert _refused(wgrad(ldx=32), L, "input pitch 32", "64 channels")
    assert _refused(wgrad(ldx=64, ldx2=32, x2=p, c1=64, cin=128, cin_ld=128), L, "second source", "64 channels")
    assert _refused(wgrad(ldx=32, ldx2=64, x2=p, c1=64, cin=128, cin_ld=128), L, "input pitch 32")
    assert _refused(wgrad(cin=10, cin_ld=16, ldx=12), L, "input pitch 12", "16 channels")            # the padded first layers: the pitch covers cin_ld
    assert _refused(wgrad(cin=3, cin_ld=16, ldx=8, s=2), L, "input pitch 8")                           # not the compact layout (4 floats)
    assert _refused(wgrad(cin=3, cin_ld=32, ldx=16, s=2, dt=bf), L, "input pitch 16")                  # ... (8 bf16)
    assert _refused(wgrad(x=p + 8), L, "16-byte aligned") and _refused(wgrad(dy=p + 4), L, "16-byte aligned")
    assert _refused(wgrad(x2=p + 8, c1=32, ldx=32, ldx2=32), L, "16-byte aligned")


def test_instnorm_entry_points_refuse_a_pitch_below_the_channels():
    L, p, f32 = _L(), PTR, _lib.F32
    c, lo = 64, 60
    assert _refused(L.shm_in_stats(p, lo, p, 1, 64, c, 1e-6, f32, None), L, "bad pitch")
    assert _refused(L.shm_in_apply(p, lo, p, p, p, c, 1, 64, c, f32, None), L, "shm_in_apply", "64 channels")
    assert _refused(L.shm_in_apply(p, c, p, p, p, lo, 1, 64, c, f32, None), L, "shm_in_apply", "64 channels")
    for lda, ldo, ldp in ((lo, c, c), (c, lo, c), (c, c, lo)):
        assert _refused(L.shm_in_apply_pool(p, lda, p, p, p, ldo, p, ldp, 1, 8, 8, c, f32, None), L, "shm_in_apply_pool", "64 channels")
    for lda, ldp in ((lo, c), (c, lo)):
        assert _refused(L.shm_in_pool(p, lda, p, p, p, ldp, 1, 8, 8, c, f32, None), L, "shm_in_pool", "64 channels")
        assert _refused(L.shm_avgpool2_fwd(p, lda, p, ldp, 1, 8, 8, c, f32, None), L, "shm_avgpool2_fwd", "64 channels")
    for ldg1, ldg2, lda, lddz in ((lo, c, c, c), (c, lo, c, c), (c, c, lo, c), (c, c, c, lo)):
        rc = L.shm_in_bwd(p, ldg1, p, ldg2, p, lda, p, p, p, lddz, None, None, None, 0, None, None, 1, 8, 8, c, 0.2, f32, None)
        assert _refused(rc, L, "shm_in_bwd", "below the 64 channels")
        rc = L.shm_in_bwd_apply(p, ldg1, p, ldg2, p, lda, p, p, p, p, None, p, lddz, None, None, 1, 8, 8, c, 0.2, f32, None)
        assert _refused(rc, L, "shm_in_bwd_apply", "below the 64 channels")
    for lda, lddz in ((lo, c), (c, lo)):
        assert _refused(L.shm_in_bwd_rank1(p, p, p, lda, p, p, p, lddz, None, None, 1, 8, 8, c, 0.2, f32, None), L, "shm_in_bwd_rank1", "below the 64 channels")
    # the pitch of an absent pooled gradient is not looked at (callers pass 0): the batch of 0 returns SHM_OK behind the checks, before any launch
    assert L.shm_in_bwd(p, c, None, 0, p, c, p, p, p, c, None, None, None, 0, None, None, 0, 8, 8, c, 0.2, f32, None) == 0
    assert L.shm_in_bwd_apply(p, c, None, 0, p, c, p, p, p, None, None, p, c, None, None, 0, 8, 8, c, 0.2, f32, None) == 0
