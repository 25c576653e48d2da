"""CPU checks behind the SHM_BF16_GF32 tests (gf32_ref.py): every claim the case table makes about the mode still stands in the source line it
restates; the table covers every variant and mirrors the "gf32" rows of the modules it extends; and the comparison has teeth -- each modelled
fault (a bf16 round trip before the fp32 store, aux read with the wrong width, an output pitch in 2-byte units, sums of the rounded value)
fails the check that is there to catch it, while the clean model passes."""
import inspect
import re
from pathlib import Path

import numpy as np
import pytest

import gf32_ref as R

CSRC = Path(__file__).resolve().parent.parent / "shmgan_amd" / "csrc"


def _src(name):
    return (CSRC / name).read_text()


def _statement(src, start):
    """The statement of `src` that begins with `start`, white space collapsed."""
    i = src.index(start)
    return re.sub(r"\s+", " ", src[i:src.index(";", i)])


# ------------------------------------------------------------------------------------------------------------------- the text pins
def test_restated_conditions_are_the_sources():
    """A failure after one of these lines was edited is no regression of the kernels: re-read the line, update gf32_ref.py's restatement and the
    table's expectations (which kernel runs, which pass delivers the sums), then this snippet."""
    igemm, bwd, wreg, halo, dma, ph4 = (_src(n) for n in ("conv_igemm.hip", "instnorm_bwd.hip", "conv_wreg.hip", "conv_halo.hip", "conv_dma.hip", "conv_phase4.hip"))
    # element sizes of the mode: 2-byte operands, 4-byte outputs
    assert "const int esz = dtype == SHM_F32 ? 4 : 2, oesz = dtype == SHM_BF16 ? 2 : 4;" in igemm
    # the fused in_bwd forms require q.dtype == SHM_BF16; wide8 includes SHM_BF16_GF32
    assert "q.dtype == SHM_BF16 && !q.r1 &&" in _statement(bwd, "const bool base_ok =")
    assert "const bool g_held = base_ok &&" in bwd and "const bool ga_held = !g_held && base_ok &&" in bwd
    assert "p.wide8 = (q.dtype == SHM_BF16 || q.dtype == SHM_BF16_GF32) && c % 8 == 0 && src16;" in bwd
    assert f'p.name = p.wide8 ? "{R.R8}" : "{R.R4}";' in bwd
    # the phase4 gsum fuses on oesz == 4
    assert "gs_fused = oesz == 4 && small && a.gred[1] == nullptr;" in igemm
    # wreg16 / ping-pong and the weights-in-registers gsum form need oesz == 2; the four-wave kernel takes fp32 outputs under wreg_ok
    assert "gs_fused = al && small && ((wreg_ok && oesz == 2) || (wreg32_ok && wreg32_wn == 4 && !two_src));" in igemm
    assert _statement(igemm, "if (v == SHM_TG_WREG && wreg_ok && oesz == 2 && w16 != 0").endswith("wreg16 = w16 == 2 && shm_pp_eligible(a) ? 2 : 1")
    assert "(oesz == 4 || (a.nout % 64 == 0 && a.n1 % 32 == 0" in _statement(igemm, "const bool wreg_ok =")
    assert "if constexpr (sizeof(TO) == 2) {\n        if (p.gs_fused) return wreg_launch<TO, NCH, true>(a, grid, np8, st);" in wreg
    assert 'shm_set_last_kernel("tapgemm_wreg_kernel<%s, %d%s>", shm_tg_name<TO>(), NCH,' in wreg
    # the alignment conditions of aux and of the outputs are dropped under oesz == 4
    assert "if (a.gred[p]) al = al && (oesz == 4 || (a.ldgaux[p] % 8 == 0 && ((size_t)a.gaux[p] & 15) == 0));" in igemm
    assert _statement(igemm, "const bool wide_ok =").startswith("const bool wide_ok = oesz == 4 ||")
    # which kernels take the sums: the static-tap halo blocks and every DMA tile (whole wave tiles per sample)
    assert "case SHM_TG_HALO128_ST: case SHM_TG_HALO64_ST: // (the other halo forms are forced-only variants: reduce pass) gs_fused = al && small && (a.y2 == nullptr || a.n1 % 64 == 0)" \
        in re.sub(r"\s+", " ", igemm)
    assert "gs_fused = al && (a.hg * a.wg) % 64 == 0;" in igemm
    # the fused-statistics refusal
    assert 'SHM_REQUIRE(dtype != SHM_BF16_GF32 || a.stats == nullptr, SHM_E_DTYPE, "%s: SHM_BF16_GF32 has no fused statistics", who);' in igemm
    # the branches of the mode: 2-byte aux loads at a sizeof(T) pitch beside 4-byte stores at a sizeof(TO) pitch
    b16 = "__uint_as_float((unsigned)__builtin_amdgcn_raw_buffer_load_b16(rsa, ao,"
    for src, n in ((halo, 1), (dma, 1), (ph4, 1)):
        assert src.count(b16) == n
        assert "* (unsigned)sizeof(TO)" in src and "(unsigned)sizeof(T)" in src
    assert "const unsigned ldab = (unsigned)a.ldgaux[gp] * (unsigned)sizeof(T), nlb = (unsigned)(n < a.nout ? nl : 0) * (unsigned)sizeof(T);" in halo
    assert "const unsigned ldab = (unsigned)a.ldgaux[0] * (unsigned)sizeof(T), nlb = (unsigned)(ncol < a.nout ? ncol : 0) * (unsigned)sizeof(T);" in ph4
    assert "ldab = (unsigned)a.ldgaux[gp] * (unsigned)sizeof(T);" in dma and "const T* gaux = (const T*)a.gaux[gp] + (n < a.nout ? nl : 0);" in dma
    assert "if constexpr (GS && sizeof(TO) == 4) if (!wide && gs_any) {" in halo
    # the small passes take the gradient type apart from the activation type
    gs = _src("grad_sums.hip")
    assert "hipLaunchKernelGGL((gsum_reduce_kernel<TG, T>)" in gs and "hipLaunchKernelGGL((lrelu_bwd_kernel<T, TG>)" in gs


def test_the_tolerances_are_the_projects_own():
    import test_gsum_gpu as G
    import test_in_bwd_plan_gpu as P
    assert f"< {R.SUM_TOL:g}".replace("e-05", "e-5") in inspect.getsource(G._check_sums)
    assert "TOL32 = 1e-4" in (Path(__file__).parent / "test_bf16_gpu.py").read_text() and R.TOL32 == 1e-4
    assert P.TOL_BF16 == 4e-3 and (P.R8, P.R4) == (R.R8, R.R4)
    from util import SENTINEL
    assert SENTINEL == R.SENTINEL


# -------------------------------------------------------------------------------------------------------------------- coverage
def _params(fn, name):
    for m in fn.pytestmark:
        names = [a.strip() for a in m.args[0].split(",")]
        if name in names:
            return [v if len(names) == 1 else v[names.index(name)] for v in m.args[1]]
    raise KeyError(name)


def _rows(fn, first):
    """the value tuples of the parametrisation of `fn` whose first argument name is `first`"""
    for m in fn.pytestmark:
        if m.args[0].split(",")[0].strip() == first:
            return m.args[1]
    raise KeyError(first)


def test_every_variant_is_in_the_table():
    import test_variants_gpu as V
    assert (R.HALO, R.DMA) == (V.HALO, V.DMA)
    tab = R.table()
    want = set(R.HALO + R.DMA + ["wreg", "phase4"])
    assert want <= {c["variant"] for c in tab if c["sec"] in (1, 2, 3, 4)}
    # ... and each of them in a case that must RUN (a refusal alone would not launch its <__bf16, float> form)
    assert want <= {c["variant"] for c in tab if c["expect"] == "run"}
    # section 1: every variant on the split destination, the four rectangles, the ping-pong shape
    s1 = R.cases(1, "dgrad")
    assert {c["variant"] for c in s1 if (c["h"], c["w"]) == (16, 16)} == set(R.HALO + R.DMA + ["wreg"])
    assert {(c["variant"], c["h"], c["w"]) for c in s1 if c["h"] != c["w"]} == {(v, h, w) for v in ("halo128_st", "halo64_st", "dma128x128", "dma256x128") for h, w in ((16, 32), (32, 16))}
    assert [c for c in s1 if c["variant"] == "wreg" and c["h"] == 32 and c["w"] == 32 and c["h"] % 8 == 0 and c["w"] % 32 == 0]
    # section 2: the seven DMA tiles, phase4 on one patch and on 3 x 3 patches, one patch by three both ways
    s2 = R.cases(2, "dgrad_s2")
    assert {c["variant"] for c in s2 if c["h"] == 16} == set(_params(V.test_dgrad_s2_and_transpose_forced_variant, "variant")) == set(R.DMA_S2) and len(R.DMA_S2) == 7
    assert {(c["n"], c["h"], c["cin"], c["cout"]) for c in s2 if c["variant"] == "phase4" and c["h"] == c["w"]} == {(2, 32, 64, 64), (1, 96, 192, 64)}
    assert {(c["variant"], c["h"], c["w"]) for c in s2 if c["h"] != c["w"]} == {(v, h, w) for v in ("phase4", "dma128x128") for h, w in ((32, 96), (96, 32))}
    # section 3
    assert [c["variant"] for c in R.cases(3, "fwd_s2")] == ["auto", "dma128x128", "dma256x128", "dma64x64"] and R.cases(3, "in_fwd")[0]["expect"] == "refuse"
    # all eight DMA tiles, every halo variant, phase4 and the four-wave weights-in-registers kernel run somewhere in sections 1 - 4
    assert len(tab) == len({(c["sec"], c["entry"], R.case_id(c), c.get("n1")) for c in tab})


def test_section_4_mirrors_the_gsum_module():
    import test_gsum_gpu as G
    assert G.DTS == ["f32", "bf16", "gf32"] and (G.HALO, G.DMA) == (R.GSUM_HALO, R.DMA)
    for fn in (G.test_dgrad_gsum_forced_variant, G.test_dgrad_gsum_with_outputs_beyond_4gib, G.test_dgrad_gsum_wreg, G.test_dgrad_gsum_stride2_and_fallback, G.test_fwd_gsum_stride2):
        assert "gf32" in _params(fn, "dt"), fn.__name__
    shapes = {(c["n"], c["h"], c["cin"], c["cout"], c["n1"]) for c in R.cases(4, "dgrad_gsum") if c["variant"] in G.HALO + G.DMA}
    assert shapes == {v[:5] for v in _rows(G.test_dgrad_gsum_forced_variant, "n")}
    assert {c["variant"] for c in R.cases(4, "dgrad_gsum") if c["variant"] not in ("wreg", "auto")} == set(G.HALO + G.DMA)
    assert {(c["n"], c["h"], c["cin"], c["cout"], c["n1"]) for c in R.cases(4, "dgrad_gsum") if c["variant"] == "wreg"} == {v[:5] for v in _rows(G.test_dgrad_gsum_wreg, "n")}
    assert [c["variant"] for c in R.cases(4, "dgrad_gsum_flat")] == _params(G.test_dgrad_gsum_with_outputs_beyond_4gib, "variant")
    assert [c["variant"] for c in R.cases(4, "fwd_s2_gsum")] == _params(G.test_fwd_gsum_stride2, "variant")
    # which pass delivers the sums: the plan's switch, restated
    for c in R.table():
        if c["sec"] == 4 and c["entry"] == "dgrad_gsum" and c["h"] >= 16:
            v = c["variant"]
            assert c["gsum"] == ("epilogue" if v in ("halo128_st", "halo64_st") or v in R.DMA else "reduce"), v
    assert all(c["gsum"] == "reduce" for c in R.table() if c["variant"] == "wreg" and c["sec"] == 4)
    assert [c["gsum"] for c in R.cases(4, "dgrad_s2_gsum") if c["variant"] == "phase4"] == ["epilogue"]
    assert "tapgemm_phase4_kernel<__bf16, float>" in inspect.getsource(G.test_dgrad_gsum_stride2_and_fallback)


def test_the_in_bwd_rows_are_in_the_plan_module():
    import test_in_bwd_plan_gpu as P
    rows = {r[0]: r for r in P.TABLE}
    for req, bf_form, gf_form in R.IN_BWD[:3]:
        b = rows[req]
        g, = [r for r in P.TABLE if r[1] == P.GF32 and r[2:10] == b[2:10]]          # the same request (shape, pooled, knobs, scratch) in this mode
        assert b[1] == P.BF and b[10] == bf_form and g[10] == gf_form == R.R8, req
        # ... and no smaller shape in the table reaches that form in bf16
        assert b[2] * b[3] * b[4] * b[5] == min(r[2] * r[3] * r[4] * r[5] for r in P.TABLE if r[10] == bf_form and r[1] == P.BF and r[6] == b[6])
    assert {(r[1], r[10]) for r in P.TABLE if r[5] == 48} == {(P.BF, R.R8), (P.F32, R.R4), (P.GF32, R.R8)}
    assert [(r[10]) for r in P.TABLE if r[1] == P.GF32 and r[5] == 36] == [R.R4]
    assert (P.GF32, 3, False) in _rows(P.test_sample_chunks_give_the_results_of_one_chunk, "dt")


# ---------------------------------------------------------------------------------------------------------------- the fault model
def _model_case():
    """the float64 product and a bf16 aux tensor at a table shape (section 4's first: n = 3, h = 16, 64 channels)"""
    c = [c for c in R.cases(4, "dgrad_gsum") if c["variant"] == "halo64_st"][0]
    rng = np.random.default_rng(3)
    shape = (c["n"], c["h"], c["w"], c["cin"])
    # a product of 9 * 64 bf16 pairs: normal values of that scale carry the full fp32 mantissa, as the kernel's accumulators do
    ref = rng.standard_normal(shape) * np.sqrt(9 * c["cout"]) * 0.1
    aux = R.bf16_round(rng.standard_normal(shape))
    aux_bits = (aux.astype(np.float32).view(np.uint32) >> 16).astype(np.uint16)
    return ref, aux, aux_bits


def _failed(ref, aux, aux_bits, fault):
    buf, band, red = R.model_launch(ref, aux_bits, fault)
    bad = []
    if not R.output_ok(buf, band, ref):
        bad.append("output")
    if not R.sums_close(red, buf, aux):          # the sums of the STORED fp32 gradient against the bf16 aux, as _check_sums takes them
        bad.append("sums")
    return bad


def test_the_clean_model_passes():
    assert _failed(*_model_case(), None) == []


@pytest.mark.parametrize("fault", R.FAULTS)
def test_every_modelled_fault_fails_its_check(fault):
    ref, aux, aux_bits = _model_case()
    bad = _failed(ref, aux, aux_bits, fault)
    want = {"bf16-round-trip": ["output"], "aux-read-as-f32": ["sums"], "pitch-in-2-byte-units": ["output", "sums"], "sums-of-rounded-values": ["sums"]}[fault]
    assert bad == want, (fault, bad)
    buf, band, red = R.model_launch(ref, aux_bits, fault)
    if fault == "bf16-round-trip":                   # about 1e-3 against the 1e-4 bound; bf16's own 4e-3 would let it through
        e = R.rel_l2(buf, ref)
        assert 10 * R.TOL32 < e < 4e-3, e
    if fault == "pitch-in-2-byte-units":             # the second half of the tensor keeps the sentinel; the band behind it is not reached
        flat = buf.ravel()
        assert (flat[flat.size // 2 + buf.shape[-1]:] == R.SENTINEL).all() and (band == R.SENTINEL).all()
        assert (buf == R.SENTINEL).all(-1).any()     # ... which the "no pixel left unwritten" check sees on its own
    if fault == "sums-of-rounded-values":            # the gradient itself is untouched: only the sums check can see it
        assert np.array_equal(buf, ref.astype(np.float32))
        n, c = buf.shape[0], buf.shape[-1]
        scale = np.sqrt((buf.astype(np.float64) ** 2).reshape(n, -1, c).sum(1))[..., None]
        assert (np.abs(red - R.sums(buf, aux)) / scale).max() > 5 * R.SUM_TOL
