"""Harness and case tables of the pitched-view tests (test_pitch_cpu.py for their teeth, test_pitch_gpu.py on the device).  No GPU import.

include/shmgan_hip.h lets every `ld*` argument of the convolution and InstanceNorm entry points exceed the channel count, and lets a tensor
start anywhere inside a wider buffer.  The tests call an entry point twice with the same values: on tight tensors and on channel-slice
VIEWS of flat parents,

    parent = [ lead band | pixel 0: c_off gap, c channels, gap up to ld | pixel 1 ... | trail band ]

Input parents are NaN outside the slice (a read of the gap, of a neighbour's channels or of a band poisons the result), output parents hold
util.SENTINEL everywhere (a store outside the slice is a failed assert, not a fault: the bands are at least as long as the tensor itself).

LAYOUTS names the slices, cases() makes the per-entry-point tables -- every pitch argument varies alone in at least one case and one case
gives every pitch a different value, so that a kernel that takes `ldx` where `ldx2` belongs cannot cancel out -- and the four predicates
restate, term by term, the host-side conditions that decide which kernel or epilogue a pitched call takes (test_pitch_cpu.py pins them to
the sources as text).  model_op() is a NumPy model of "an NHWC op that addresses through base + pixel * ld + channel" with the faults the
harness has to catch.
"""
import numpy as np
import torch

from util import SENTINEL, guard_elems

Q = {"f32": 4, "bf16": 8}                 # the header's pitch quantum per activation type (16 bytes)
ESZ = {"f32": 4, "bf16": 2}


def dt_of(t):
    return "bf16" if t in (torch.bfloat16, "bf16") else "f32"


def up(c, q):
    return -(-c // q) * q


# --------------------------------------------------------------------------------------------------------------------------- layouts
# name -> (pitch, channel offset) of a slice of c channels.  `tight` is the control (a ragged channel count rounds up to the quantum: the
# smallest pitch the contract allows).  `half` (bf16 outputs and aux only) keeps the pitch a multiple of 8 and puts the base 8 bytes off a
# 16-byte boundary: it flips the `& 15` terms alone.  `plus4` (bf16 only: InstanceNorm tensors, convolution outputs and aux) is a multiple of 4 that is none of 8: the
# InstanceNorm entry points take it (four channels per thread) and leave their 16-byte forms, the convolutions store element by element.
LAYOUTS = {
    "tight": lambda c, q: (up(c, q), 0),
    "wide": lambda c, q: (up(c, q) + q, 0),
    "slice": lambda c, q: (2 * up(c, q), up(c, q)),
    "odd-wide": lambda c, q: (up(c, q) + 3 * q, 0),
    "half": lambda c, q: (up(c, 8) + 8, 4),
    "plus4": lambda c, q: (up(c, 8) + 4, 0),
    "wide2": lambda c, q: (up(c, q) + 2 * q, 0),                # (the fourth and fifth tensor of an all-different case)
    "slice3": lambda c, q: (3 * up(c, q), up(c, q)),
}
INPUT_KINDS = ("wide", "slice", "odd-wide")


def layout(kind, c, dt):
    """(ld, c_off) in elements of layout `kind` for a tensor of c channels of type dt ("f32" / "bf16")."""
    return LAYOUTS[kind](c, Q[dt_of(dt)])


def lead_elems(shape, ld):
    """Guard band in elements: the tensor's own pitched extent (and never less than util.guard_elems), rounded to 64 elements so that a
    slice at channel offset 0 starts 16-byte aligned in either type."""
    n = int(np.prod(shape[:-1])) * int(ld)
    return up(max(n, guard_elems(shape)), 64)


def view_of(parent_fill, shape, ld, c_off=0, lead=None, dtype=torch.float32, device="cpu"):
    """A view [n, h, w, c] (or any [..., c]) with channel pitch ld at channel offset c_off inside a flat parent filled with parent_fill,
    between a leading and a trailing band of `lead` elements (default lead_elems()).  Returns (view, parent); view.data_ptr() is the base
    the entry point gets."""
    shape = tuple(int(s) for s in shape)
    c = shape[-1]
    assert ld >= c_off + c and c_off >= 0, (ld, c_off, c)
    lead = lead_elems(shape, ld) if lead is None else int(lead)
    assert lead >= guard_elems(shape)
    npix = int(np.prod(shape[:-1]))
    parent = torch.full((lead + npix * ld + lead,), float(parent_fill), dtype=dtype, device=device)
    strides, s = [], ld
    for d in reversed(shape[:-1]):
        strides.append(s)
        s *= d
    view = parent.as_strided(shape, tuple(reversed(strides)) + (1,), lead + c_off)
    return view, parent


def _bits(t):
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32 if t.element_size() == 4 else torch.int64)


def outside_untouched(parent, shape, ld, c_off=0, lead=None, fill=SENTINEL):
    """Every element of `parent` outside the slice -- the gaps and both bands -- is bit-equal to the fill."""
    shape = tuple(int(s) for s in shape)
    lead = lead_elems(shape, ld) if lead is None else int(lead)
    npix = int(np.prod(shape[:-1]))
    p = parent.detach().cpu()
    want = _bits(torch.full((1,), float(fill), dtype=p.dtype))[0]
    same = _bits(p) == want
    body = same[lead:lead + npix * ld].view(npix, ld)
    return bool(same[:lead].all()) and bool(same[lead + npix * ld:].all()) and bool(body[:, :c_off].all()) and bool(body[:, c_off + shape[-1]:].all())


# ----------------------------------------------------------------------------------------------------------------------- case tables
# entry point -> its pitch arguments by role.  "in": read only (16-byte-aligned bases in every case); "out": written; "aux": read by the
# gsum epilogues next to the output they describe.
ENTRY_POINTS = {
    "conv2d_fwd": {"in": ("ldx", "ldx2"), "out": ("ldy",), "aux": ("ldaux",)},
    "conv2d_in_fwd": {"in": ("ldx", "ldx2"), "out": ("ldy",), "aux": ()},
    "conv2d_dgrad": {"in": ("lddy",), "out": ("lddx", "lddx2"), "aux": ("ldaux", "ldaux2")},
    "conv2d_transpose_fwd": {"in": ("ldx",), "out": ("ldy",), "aux": ()},
    "conv2d_wgrad": {"in": ("ldx", "ldx2", "lddy"), "out": (), "aux": ()},
    "in_stats": {"in": ("lda",), "out": (), "aux": ()},
    "in_apply": {"in": ("lda",), "out": ("ldo",), "aux": ()},
    "in_apply_pool": {"in": ("lda",), "out": ("ldo", "ldp"), "aux": ()},
    "in_pool": {"in": ("lda",), "out": ("ldp",), "aux": ()},
    "avgpool2_fwd": {"in": ("ldx",), "out": ("ldy",), "aux": ()},
    "in_bwd": {"in": ("ldg1", "ldg2", "lda"), "out": ("lddz",), "aux": ()},
    "in_bwd_apply": {"in": ("ldg1", "ldg2", "lda"), "out": ("lddz",), "aux": ()},
    "in_bwd_rank1": {"in": ("lda",), "out": ("lddz",), "aux": ()},
}
INSTNORM = ("in_stats", "in_apply", "in_apply_pool", "in_pool", "avgpool2_fwd", "in_bwd", "in_bwd_apply", "in_bwd_rank1")


def cases(entry, dt, args=None):
    """[(id, {pitch argument: layout name})] for `entry` in type dt; arguments not named are tight.  args: the subset of the entry point's
    pitch arguments the call under test has (no x2 -> no ldx2)."""
    roles = ENTRY_POINTS[entry]
    have = lambda names: [a for a in names if args is None or a in args]          # noqa: E731
    ins, outs, aux = have(roles["in"]), have(roles["out"]), have(roles["aux"])
    out = [("tight", {})]
    for a in ins:
        out += [(f"{a}-{k}", {a: k}) for k in INPUT_KINDS]
        if dt == "bf16" and entry in INSTNORM:
            out.append((f"{a}-plus4", {a: "plus4"}))
    for a in outs + aux:
        out += [(f"{a}-{k}", {a: k}) for k in INPUT_KINDS]
        if dt == "bf16":
            out.append((f"{a}-half", {a: "half"}))
            out.append((f"{a}-plus4", {a: "plus4"}))
    # every pitch different: the kinds go round, so two tensors of the same channel count still get two pitches
    every = ins + outs + aux
    if len(every) > 1:
        kinds = ("wide", "slice", "odd-wide")
        all_diff = {a: kinds[i % 3] for i, a in enumerate(every)}
        for a, k in zip(every[3:], ("wide2", "slice3")):          # a fourth and fifth tensor: two more pitches
            all_diff[a] = k
        out.append(("all-different", all_diff))
    return out


# -------------------------------------------------------------------------------------------------------- the four restated predicates
def _al16(ld, addr):
    return ld % 8 == 0 and addr % 16 == 0


def epilogue_terms(nout, n1, ldy, y, ldy2=None, y2=None, phase4=False):
    """The terms of `wide` (conv_halo.hip, conv_dma.hip; bf16 outputs): name -> truth.  y / y2: byte addresses.  phase4: the fused four-phase
    kernel (conv_phase4.hip) has one destination of whole 64-channel slices: the pitch and the base are its only terms."""
    if phase4:
        return {"ldy % 8": ldy % 8 == 0, "y & 15": y % 16 == 0}
    t = {"nout % 8": nout % 8 == 0, "n1 % 8": n1 % 8 == 0, "ldy % 8": ldy % 8 == 0, "y & 15": y % 16 == 0}
    if y2 is not None:
        t["ldy2 % 8"] = ldy2 % 8 == 0
        t["y2 & 15"] = y2 % 16 == 0
    return t


def epilogue(out_dt, nout, n1, ldy, y, ldy2=None, y2=None, phase4=False):
    """"wide16": the LDS-staged 16-byte stores; "element": the element-store epilogues (fp32 outputs always)."""
    return "wide16" if dt_of(out_dt) == "bf16" and all(epilogue_terms(nout, n1, ldy, y, ldy2, y2, phase4).values()) else "element"


def wreg_terms(nout, n1, ldy, y, ldy2=None, y2=None):
    """The output terms of `wreg_ok` (conv_igemm.hip tapgemm_plan; bf16 outputs; fp32 outputs have none)."""
    t = {"nout % 64": nout % 64 == 0, "n1 % 32": n1 % 32 == 0, "ldy % 8": ldy % 8 == 0, "y & 15": y % 16 == 0}
    if y2 is not None:
        t["ldy2 % 8"] = ldy2 % 8 == 0
        t["y2 & 15"] = y2 % 16 == 0
    return t


def wreg_family(dt, out_dt, nout, n1, ldy, y, ldy2=None, y2=None):
    """Does a bf16 layer that is otherwise eligible stay on the weights-in-registers / ping-pong kernels?  "wreg" or "halo"."""
    if dt_of(dt) == "f32" or dt_of(out_dt) == "f32":
        return "wreg"
    return "wreg" if all(wreg_terms(nout, n1, ldy, y, ldy2, y2).values()) else "halo"


def gsum_terms(out_dt, parts, nout, n1, ldy, y, ldy2=None, y2=None):
    """The pitch and alignment terms of `al` and `wide_ok` (tapgemm_plan).  parts: [(ldaux, aux address)] of the parts that want sums."""
    if dt_of(out_dt) == "f32":
        return {}
    t = {}
    for i, (ld, addr) in enumerate(parts):
        t[f"ldgaux[{i}] % 8"] = ld % 8 == 0
        t[f"gaux[{i}] & 15"] = addr % 16 == 0
    t.update({"wide_ok: " + k: v for k, v in epilogue_terms(nout, n1, ldy, y, ldy2, y2).items()})
    return t


def gsum_path(out_dt, parts, nout, n1, ldy, y, ldy2=None, y2=None):
    """"epilogue": the sums may be taken by the product's epilogue (if its kernel has one); "reduce": the follow-up reduce pass."""
    return "epilogue" if all(gsum_terms(out_dt, parts, nout, n1, ldy, y, ldy2, y2).values()) else "reduce"


R8 = "in_bwd_reduce8_kernel + in_bwd_apply_kernel"
R4 = "in_bwd_reduce_kernel + in_bwd_apply_kernel"


def in_bwd_terms(ldg1, lda, lddz, ldg2=None, rank1=False, dz=0):
    """The terms of `src16` and the one-pass forms' `lddz % 8` and 16-byte-aligned dz (instnorm_bwd.hip in_bwd_plan).  dz: byte address.
    (`src16` also wants 16-byte-aligned sources; input bases stay aligned in every case, so that term is pinned as text and not modelled.)"""
    t = {"lda % 8": lda % 8 == 0, "lddz % 8": lddz % 8 == 0, "dz & 15": dz % 16 == 0}
    if not rank1:
        t["ldg1 % 8"] = ldg1 % 8 == 0
    if ldg2 is not None:
        t["ldg2 % 8"] = ldg2 % 8 == 0
    return t


def in_bwd_form(dt, c, ldg1, lda, lddz, ldg2=None, rank1=False, one_pass=None, dz=0):
    """shm_last_kernel() of a shm_in_bwd / shm_in_bwd_rank1 call.  one_pass: the name of the one-pass kernel the shape would take on tight
    tensors with a scratch (None: two passes anyway)."""
    if dt_of(dt) == "f32":
        return R4
    t = in_bwd_terms(ldg1, lda, lddz, ldg2, rank1, dz)
    src16 = all(v for k, v in t.items() if k not in ("lddz % 8", "dz & 15"))
    if one_pass and src16 and t["lddz % 8"] and t["dz & 15"]:
        return one_pass
    return R8 if (c % 8 == 0 and src16) else R4


def wgrad_thin_pitch(ldx):
    """The pitch term of `thin_ok` (conv_wgrad.hip wgrad_plan): the thin-input packing reads pixels of exactly 16 floats; any other pitch takes
    the layer to the plain halo kernel."""
    return ldx == 16


# ---------------------------------------------------------------------------------------------------------------- the strided model
FAULTS = ("read-pitch-is-channels", "write-pitch-is-channels", "src1-pitch-for-src2", "part1-pitch-for-part2", "aux-pitch-is-out-pitch",
          "base-offset-dropped", "store-into-gap", "store-into-lead-band", "store-into-trail-band", "read-of-gap")


def model_reference(x1, x2, aux):
    """What model_op computes: y = 2 * concat(x1, x2) reversed along the channels + 1, split at 16 channels; red[ch] = sum_pixels y1 * aux.
    (Every tensor has 16 channels: on tight tensors all five pitches agree, which is why a tight call sees none of the exchanged-pitch faults.)"""
    y = 2.0 * np.concatenate([x1, x2], -1)[..., ::-1] + 1.0
    y1, y2 = y[..., :16], y[..., 16:]
    return y1, y2, (y1 * aux).reshape(-1, 16).sum(0)


def model_op(flat, ptr, ld, npix, fault=None):
    """flat: {name: 1-D float array (the parent)}, ptr: {name: element index of the view's base}, ld: {name: pitch} for the tensors x1, x2, aux, y1, y2
    of 16 channels each.  Reads and writes through base + pixel * ld + channel only.  Returns red."""
    c1, c2, n1, n2 = 16, 16, 16, 16
    rd = dict(ld)
    wr = dict(ld)
    base = dict(ptr)
    if fault == "read-pitch-is-channels":
        rd["x1"] = c1
    if fault == "write-pitch-is-channels":
        wr["y1"] = n1
    if fault == "src1-pitch-for-src2":
        rd["x2"] = rd["x1"]
    if fault == "part1-pitch-for-part2":
        wr["y2"] = wr["y1"]
    if fault == "aux-pitch-is-out-pitch":
        rd["aux"] = wr["y1"]
    red = np.zeros(n1)
    for p in range(npix):
        row = np.concatenate([flat["x1"][base["x1"] + p * rd["x1"]:][:c1], flat["x2"][base["x2"] + p * rd["x2"]:][:c2]])
        if fault == "read-of-gap" and p == npix // 2 and ld["x1"] > c1:
            # the element behind the slice's channels: the gap, or (upper-half slice) the front gap of the next pixel
            row[0] = row[0] + 0.0 * flat["x1"][base["x1"] + p * ld["x1"] + c1]
        y = 2.0 * row[::-1] + 1.0
        flat["y1"][base["y1"] + p * wr["y1"]:][:n1] = y[:n1]
        flat["y2"][base["y2"] + p * wr["y2"]:][:n2] = y[n1:]
        red += y[:n1] * flat["aux"][base["aux"] + p * rd["aux"]:][:n1]
    return red


def model_faulted_base(ptr, c_off, fault):
    """The bases model_op gets: with "base-offset-dropped" the channel offset of y1's slice is lost (the parent's pixel 0, channel 0)."""
    out = dict(ptr)
    if fault == "base-offset-dropped":
        out["y1"] = ptr["y1"] - c_off["y1"]
        out["x1"] = ptr["x1"] - c_off["x1"]
    return out


def model_stray_store(flat, ptr, ld, lead, npix, fault):
    """The three stray stores: one element of y1's parent outside the slice."""
    if fault == "store-into-gap" and ld["y1"] > 16:
        # the element behind the slice's channels of a middle pixel: the gap, or (upper-half slice) the front gap of the next pixel
        flat["y1"][ptr["y1"] + (npix // 2) * ld["y1"] + 16] = 1.0
    if fault == "store-into-lead-band":
        flat["y1"][lead["y1"] - 1] = 1.0
    if fault == "store-into-trail-band":
        flat["y1"][lead["y1"] + npix * ld["y1"]] = 1.0


# ------------------------------------------------------------------------------------------------------------ the device test's table
# One record per (family, shape): what test_pitch_gpu.py runs and test_pitch_cpu.py proves coverage over.
#   entry     the entry point (ENTRY_POINTS)
#   dts       activation types
#   variants  forced "tapgemm.variant" names ("auto": the automatic choice; the weights-in-registers kernels are entered through it so that
#             a pitch that takes the layer off them shows as another kernel, not as a refusal)
#   knobs     tuning knobs set for the family, or a list of knob dicts (one run each)
#   shape     what the family's runner needs
#   ch        pitch argument -> channel count of its tensor (the arguments the call has)
#   out_f32   bf16 operands with fp32 outputs (SHM_BF16_GF32)
HALO = ("halo128", "halo64", "halo128_st", "halo64_st", "halo128_st_w4")
DMA = ("dma128x128", "dma64x128", "dma128x64", "dma64x64", "dma256x64", "dma256x128", "dma128x128_bk32", "dma128x128_nst4")
BOTH = ("f32", "bf16")


def _fam(name, entry, dts, variants, shape, ch, knobs=None, out_f32=False, only=None):
    return dict(name=name, entry=entry, dts=dts, variants=variants, shape=shape, ch=ch, knobs=knobs or {}, out_f32=out_f32, only=only)


def _fwd(n, h, w, c1, c2, cout, k=3, s=1):
    return dict(n=n, h=h, w=w, c1=c1, c2=c2, cout=cout, k=k, s=s)


def _fwd_ch(sh):
    ch = {"ldx": sh["c1"], "ldy": sh["cout"]}
    if sh["c2"]:
        ch["ldx2"] = sh["c2"]
    return ch


def _dg(n, h, w, cin, cout, n1, s=1):
    return dict(n=n, h=h, w=w, cin=cin, cout=cout, n1=n1, s=s)


def _dg_ch(sh, gsum=(False, False)):
    split = 0 < sh["n1"] < sh["cin"]
    ch = {"lddy": sh["cout"], "lddx": sh["n1"] if split else sh["cin"]}
    if split:
        ch["lddx2"] = sh["cin"] - sh["n1"]
    if gsum[0]:
        ch["ldaux"] = ch["lddx"]
    if gsum[1] and split:
        ch["ldaux2"] = ch["lddx2"]
    return ch


OUT_ONLY = ("tight", "ldy-wide", "ldy-slice", "ldy-half", "ldy-plus4", "all-different")

FAMILIES = []
for _sh in (_fwd(2, 16, 32, 64, 64, 64), _fwd(2, 16, 32, 64, 0, 160)):
    FAMILIES.append(_fam("fwd-halo", "conv2d_in_fwd", BOTH, HALO, _sh, _fwd_ch(_sh), only=None if _sh["c2"] else OUT_ONLY))
    FAMILIES.append(_fam("fwd-halo-ph8", "conv2d_in_fwd", ("bf16",), ("halo128_ph8",), _sh, _fwd_ch(_sh), only=OUT_ONLY))
for _co in (12, 20):
    _sh = _fwd(2, 16, 32, 64, 0, _co)
    FAMILIES.append(_fam("fwd-halo-ragged", "conv2d_in_fwd", BOTH, ("halo128", "halo128_st", "halo64_st"), _sh, _fwd_ch(_sh), only=OUT_ONLY))
_sh = _fwd(2, 10, 10, 64, 0, 96)
FAMILIES.append(_fam("fwd-dma", "conv2d_in_fwd", BOTH, DMA, _sh, _fwd_ch(_sh)))
for _sh in (_fwd(2, 16, 16, 64, 0, 96), _fwd(2, 32, 32, 64, 0, 96, 3, 2), _fwd(2, 16, 16, 64, 0, 96, 1, 1)):
    FAMILIES.append(_fam("fwd-dma-geom", "conv2d_in_fwd", BOTH, ("dma128x128", "dma64x64", "dma256x64"), _sh, _fwd_ch(_sh), only=OUT_ONLY + ("ldx-slice",)))
for _co in (3, 20):
    _sh = _fwd(2, 10, 10, 64, 0, _co)
    FAMILIES.append(_fam("fwd-dma-ragged", "conv2d_in_fwd", BOTH, ("dma128x128", "dma64x64", "dma128x64"), _sh, _fwd_ch(_sh), only=OUT_ONLY))
_sh = _fwd(2, 16, 32, 64, 0, 64)
FAMILIES.append(_fam("fwd-wreg", "conv2d_in_fwd", BOTH, ("auto",), _sh, _fwd_ch(_sh), knobs=[{"tapgemm.wreg16": 2}, {"tapgemm.wreg16": 1}, {"tapgemm.wreg16": 0}]))
for _sh in (_fwd(2, 32, 32, 16, 0, 16), _fwd(2, 32, 32, 16, 16, 16)):
    FAMILIES.append(_fam("fwd-wreg-f32-narrow", "conv2d_fwd", ("f32",), ("wreg",), _sh, _fwd_ch(_sh)))
_sh = _fwd(2, 16, 32, 64, 64, 64)
FAMILIES.append(_fam("fwd-flat-epilogue", "conv2d_in_fwd", BOTH, ("halo64_st", "dma128x128"), _sh, _fwd_ch(_sh), knobs={"tapgemm.flat_epilogue": 1}))
_sh = _fwd(2, 32, 32, 64, 0, 128)
FAMILIES.append(_fam("fwd-x3", "conv2d_in_fwd", ("f32",), ("halo128_st",), _sh, _fwd_ch(_sh), knobs={"conv.f32_split": 1}))
# shm_conv2d_fwd_gsum: the stride-2 forward form (Conv2DTranspose's input gradient) with the sums of its output
_sh = _fwd(2, 32, 32, 64, 0, 64, 3, 2)
FAMILIES.append(_fam("fwd-gsum-s2", "conv2d_fwd", BOTH, ("dma128x128", "dma64x64"), _sh, dict(_fwd_ch(_sh), ldaux=64)))
# sources normalised on the fly (shm_conv2d_in_fwd_norm): the smallest FWD_CASES of test_norm_fold_gpu.py
for _mode in ("exact", "scaled"):
    _sh = dict(_fwd(3, 16, 16, 64, 0, 64), norm=_mode)
    FAMILIES.append(_fam("fwd-norm-" + _mode, "conv2d_in_fwd", BOTH, ("halo64_st", "auto"), _sh, _fwd_ch(_sh)))
# Conv2DTranspose and the stride-2 input gradient: the four-phase launches
_T = dict(n=2, h=16, w=16, cin=64, cout=64)
FAMILIES.append(_fam("transpose", "conv2d_transpose_fwd", BOTH, ("dma128x128", "dma64x64", "phase4"), _T, {"ldx": 64, "ldy": 64}, knobs={"tapgemm.phase4_min_blocks": 0}))
for _co in (3, 12, 20):
    FAMILIES.append(_fam("transpose-ragged", "conv2d_transpose_fwd", BOTH, ("dma128x128", "dma64x64"), dict(_T, cout=_co), {"ldx": 64, "ldy": _co}, only=OUT_ONLY))
_sh = _dg(2, 32, 32, 64, 64, 64, 2)
FAMILIES.append(_fam("dgrad-s2", "conv2d_dgrad", BOTH, ("dma128x128", "dma64x64", "phase4"), _sh, _dg_ch(_sh), knobs={"tapgemm.phase4_min_blocks": 0}))
# unit-stride input gradient with a split destination
_sh = _dg(2, 16, 16, 128, 64, 64)
FAMILIES.append(_fam("dgrad-split", "conv2d_dgrad", BOTH, ("halo128_st", "halo64_st", "dma128x128", "auto"), _sh, _dg_ch(_sh)))
FAMILIES.append(_fam("dgrad-split-gf32", "conv2d_dgrad", ("bf16",), ("halo64_st", "auto"), _sh, _dg_ch(_sh), out_f32=True))
for _sh in (_dg(2, 16, 16, 32, 64, 12), _dg(2, 16, 16, 64, 64, 40), _dg(2, 16, 16, 20, 64, 8)):
    FAMILIES.append(_fam("dgrad-ragged", "conv2d_dgrad", BOTH, ("halo64_st", "dma128x128"), _sh, _dg_ch(_sh),
                         only=("tight", "lddx-wide", "lddx-half", "lddx2-slice", "lddx2-half", "lddx2-plus4", "all-different")))
_sh = _dg(2, 32, 32, 128, 64, 128)
FAMILIES.append(_fam("dgrad-x3", "conv2d_dgrad", ("f32",), ("halo128_st",), _sh, _dg_ch(_sh), knobs={"conv.f32_split": 1}))
# gsum epilogues
_sh = _dg(2, 16, 16, 128, 64, 64)
FAMILIES.append(_fam("dgrad-gsum", "conv2d_dgrad", BOTH, ("halo64_st", "dma128x128", "auto"), _sh, _dg_ch(_sh, (True, True))))
_sh = _dg(2, 32, 32, 64, 64, 64, 2)
FAMILIES.append(_fam("dgrad-s2-gsum", "conv2d_dgrad", BOTH, ("phase4", "dma128x128"), _sh, _dg_ch(_sh, (True, False)), knobs={"tapgemm.phase4_min_blocks": 0},
                     only=("tight", "ldaux-wide", "ldaux-slice", "ldaux-half", "ldaux-plus4", "lddx-half", "all-different")))
# weight gradients: (stride, map, cin (c1 + c2), cout, knobs)
for _nm, _s, _hw, _c1, _c2, _co, _kn in (
        ("generic", 1, 16, 64, 0, 64, {"wgrad.variant": 1}),
        ("halo", 1, 16, 64, 0, 64, {"wgrad.variant": 2}),
        ("halo-blocks3", 1, 16, 64, 0, 128, {"wgrad.variant": 2, "wgrad.blocks": 3, "wgrad.bf16_wide": 1}),
        ("halo-rows2", 1, 16, 64, 0, 64, {"wgrad.variant": 2, "wgrad.bf16_rows": 2}),
        ("halo8", 1, 16, 64, 0, 128, {"wgrad.variant": 2, "wgrad.bf16_wide": 4}),
        ("concat", 1, 16, 64, 64, 64, {}),
        ("thin", 1, 16, 10, 0, 64, {}),
        ("s2", 2, 32, 64, 0, 128, {}),
        ("s2-halo8", 2, 32, 64, 0, 128, {"wgrad.bf16_wide": 4}),
        ("x3", 1, 16, 64, 0, 64, {"wgrad.f32_split": 1}),
        ("norm", 1, 16, 64, 0, 64, {})):                              # shm_conv2d_wgrad_norm, SHM_NORM_EXACT: the source normalised in LDS
    _dts = ("bf16",) if _nm in ("halo-rows2", "halo8", "s2-halo8") else ("f32",) if _nm == "x3" else BOTH
    _ch = {"ldx": _c1, "lddy": _co}
    if _c2:
        _ch["ldx2"] = _c2
    FAMILIES.append(_fam("wgrad-" + _nm, "conv2d_wgrad", _dts, ("-",), dict(n=2, h=_hw, w=_hw, c1=_c1, c2=_c2, cout=_co, s=_s, norm=_nm == "norm"), _ch, knobs=_kn))
# InstanceNorm forward side and pooling
IN_SHAPES = ((2, 16, 16, 64), (3, 4, 6, 48), (2, 2, 2, 1024))
for _e in ("in_stats", "in_apply", "in_apply_pool", "in_pool", "avgpool2_fwd"):
    for _n, _h, _w, _c in IN_SHAPES:
        _args = ENTRY_POINTS[_e]["in"] + ENTRY_POINTS[_e]["out"]
        FAMILIES.append(_fam(_e, _e, BOTH, ("-",), dict(n=_n, h=_h, w=_w, c=_c), {a: _c for a in _args}, knobs=[{"elem.reverse": 0}, {"elem.reverse": 1}]))
for _n, _h, _w, _c in IN_SHAPES:
    FAMILIES.append(_fam("in_apply-inplace", "in_apply", BOTH, ("-",), dict(n=_n, h=_h, w=_w, c=_c, inplace=True), {"lda": _c}))
# InstanceNorm backward, two passes
BWD_SHAPES = ((2, 16, 16, 64), (3, 4, 6, 48), (2, 8, 8, 256))
for _n, _h, _w, _c in BWD_SHAPES:
    for _g2 in (False, True):
        _ch = {"ldg1": _c, "lda": _c, "lddz": _c}
        if _g2:
            _ch["ldg2"] = _c
        _sh = dict(n=_n, h=_h, w=_w, c=_c, g2=_g2)
        FAMILIES.append(_fam("in_bwd", "in_bwd", BOTH, ("-",), _sh, _ch, knobs=[{"elem.fused_bwd": 0, "elem.interleave": 0}, {"elem.fused_bwd": 0, "elem.interleave": 1}]))
        FAMILIES.append(_fam("in_bwd_apply", "in_bwd_apply", BOTH, ("-",), _sh, _ch))
    FAMILIES.append(_fam("in_bwd_rank1", "in_bwd_rank1", BOTH, ("-",), dict(n=_n, h=_h, w=_w, c=_c), {"lda": _c, "lddz": _c}))
# ... and one pass (bf16, scratch given): multiples of 8 stay on the one-pass kernel, c + 4 falls back to the two passes
for _hold, _shp in ((1, (2, 16, 16, 64)), (2, (2, 16, 32, 64))):
    for _g2 in ((False, True) if _hold == 1 else (False,)):
        _n, _h, _w, _c = _shp
        _ch = {"ldg1": _c, "lda": _c, "lddz": _c}
        if _g2:
            _ch["ldg2"] = _c
        FAMILIES.append(_fam("in_bwd-one-pass", "in_bwd", ("bf16",), ("-",), dict(n=_n, h=_h, w=_w, c=_c, g2=_g2, scratch=True), _ch, knobs={"elem.fused_hold": _hold}))
        if not _g2:          # ... and with the bias gradient folded in the kernel (no dz_sums: the trainer's default), and without a bias gradient
            for _sums in ("dbias", "none"):
                FAMILIES.append(_fam("in_bwd-one-pass-" + _sums, "in_bwd", ("bf16",), ("-",), dict(n=_n, h=_h, w=_w, c=_c, g2=False, scratch=True, sums=_sums), _ch,
                                     knobs={"elem.fused_hold": _hold}, only=("tight", "ldg1-wide", "lda-slice", "lddz-odd-wide", "lddz-half", "lddz-plus4", "all-different")))
# the two passes likewise: dbias without dz_sums, and neither
for _n, _h, _w, _c in BWD_SHAPES:
    for _sums in ("dbias", "none"):
        for _e in ("in_bwd", "in_bwd_apply", "in_bwd_rank1"):
            _ch = {"lda": _c, "lddz": _c} if _e == "in_bwd_rank1" else {"ldg1": _c, "lda": _c, "lddz": _c}
            FAMILIES.append(_fam(_e + "-" + _sums, _e, BOTH, ("-",), dict(n=_n, h=_h, w=_w, c=_c, g2=False, sums=_sums), _ch, knobs={"elem.fused_bwd": 0},
                                 only=("tight", "ldg1-wide", "lda-slice", "lda-plus4", "lddz-odd-wide", "lddz-half", "all-different")))


# shm_last_kernel() of the TIGHT call of the families that reach their kernel through the automatic choice or an opt-in knob: asserted, so that
# a changed plan heuristic cannot turn such a family into a silent copy of another one
def tight_kernel(fam, variant, dt, knobs):
    name, sh, t = fam["name"], fam["shape"], "float" if dt == "f32" else "__bf16"
    if name.startswith("in_bwd-one-pass"):
        return "in_bwd_fusedg_kernel<2, 2, 4>" if knobs.get("elem.fused_hold") == 2 else "in_bwd_fused8_kernel<true>" if sh["g2"] else "in_bwd_fused8_kernel<false>"
    if name in ("fwd-x3", "dgrad-x3"):
        return "tapgemm_halo_x3_kernel<false, 128>"
    if name.startswith("wgrad-"):
        return {"wgrad-generic": {"f32": "wgrad_kernel<9, false>", "bf16": "wgrad_bf16_kernel<9, false>"},
                "wgrad-halo": {"f32": "wgrad_halo_kernel", "bf16": "wgrad_halo_bf16_kernel<4>"},
                "wgrad-halo-blocks3": {"f32": "wgrad_halo_kernel", "bf16": "wgrad_halo_bf16_kernel<4>"},
                "wgrad-halo-rows2": {"bf16": "wgrad_halo_bf16_kernel<2>"}, "wgrad-halo8": {"bf16": "wgrad_halo8_bf16_kernel<0>"},
                "wgrad-concat": {"f32": "wgrad_halo_kernel", "bf16": "wgrad_halo_bf16_kernel<4>"},
                "wgrad-thin": {"f32": "wgrad_halo_thin_kernel<3, 1>", "bf16": "wgrad_halo_bf16_kernel<4>"},          # (the packing is an fp32 form: cin_ld <= 16)
                "wgrad-s2": {"f32": "wgrad_halo_kernel<0, true>", "bf16": "wgrad_halo8_bf16_kernel<1>"}, "wgrad-s2-halo8": {"bf16": "wgrad_halo8_bf16_kernel<1>"},
                "wgrad-x3": {"f32": "wgrad_halo_x3_kernel<4>"}, "wgrad-norm": {"f32": "wgrad_halo_kernel<1>", "bf16": "wgrad_halo_bf16_kernel<4, 1>"}}[name][dt]
    if variant != "auto":
        return None
    if name == "fwd-wreg":
        return "tapgemm_wreg_f32_kernel<4, 4, false>" if dt == "f32" else \
            {2: "tapgemm_pp_bf16_kernel<2>", 1: "tapgemm_wreg16_bf16_kernel<2, true>", 0: "tapgemm_wreg_kernel<__bf16, 2>"}[knobs["tapgemm.wreg16"]]
    if name.startswith("fwd-norm-"):
        m = 1 if sh["norm"] == "exact" else 2
        return f"tapgemm_wreg_f32_kernel<4, 4, false, false, {m}>" if dt == "f32" else f"tapgemm_wreg_kernel<__bf16, 2, false, {m}>"
    if name == "dgrad-split":
        return "tapgemm_wreg_f32_kernel<4, 4, false>" if dt == "f32" else "tapgemm_wreg16_bf16_kernel<2, false>"
    if name == "dgrad-split-gf32":
        return "tapgemm_wreg_kernel<float, 2>"
    if name == "dgrad-gsum":
        return "tapgemm_wreg_f32_kernel<4, 4, false, true>" if dt == "f32" else "tapgemm_wreg_kernel<__bf16, 2, true>"
    raise KeyError((name, t))          # a new family under the automatic choice names its kernel here


def knob_sets(fam):
    return fam["knobs"] if isinstance(fam["knobs"], list) else [fam["knobs"]]


def family_cases(fam, dt):
    """[(case id, case)] of a family in one type."""
    cs = cases(fam["entry"], dt, tuple(fam["ch"]))
    if fam["only"] is not None:
        cs = [c for c in cs if c[0] in fam["only"]]
    return cs


def table():
    """Every device case: (family record, variant, dt, knob dict, case id, case)."""
    for fam in FAMILIES:
        for dt in fam["dts"]:
            for variant in fam["variants"]:
                for kn in knob_sets(fam):
                    for cid, case in family_cases(fam, dt):
                        yield fam, variant, dt, kn, cid, case


def out_dt(fam, dt):
    return "f32" if fam["out_f32"] else dt


def addr16(case, arg, c, dt):
    """Byte address modulo 16 of the tensor behind pitch argument `arg` in a case (the parents and their bands are 16-byte multiples)."""
    _, off = layout(case.get(arg, "tight"), c, dt)
    return off * ESZ[dt_of(dt)] % 16


def conv_out_terms(fam, dt, case, which="wide"):
    """The terms of a convolution family's output predicate for a case: `wide` (the epilogue), "wreg" or "gsum"."""
    odt = out_dt(fam, dt)
    ch, sh = fam["ch"], fam["shape"]
    a1, a2 = ("lddx", "lddx2") if fam["entry"] == "conv2d_dgrad" else ("ldy", None)
    nout = sh.get("cin") if fam["entry"] == "conv2d_dgrad" else sh["cout"]
    two = a2 in ch
    n1 = ch[a1]
    ld1 = layout(case.get(a1, "tight"), ch[a1], odt)[0]
    y1 = addr16(case, a1, ch[a1], odt)
    ld2, y2 = (layout(case.get(a2, "tight"), ch[a2], odt)[0], addr16(case, a2, ch[a2], odt)) if two else (None, None)
    if odt == "f32":
        return {}
    if which == "wide":
        return epilogue_terms(nout, n1, ld1, y1, ld2, y2)
    if which == "wreg":
        t = wreg_terms(nout, n1, ld1, y1, ld2, y2)
        return {k: v for k, v in t.items() if "nout" not in k and "n1" not in k}
    parts = [(layout(case.get(a, "tight"), ch[a], dt)[0], addr16(case, a, ch[a], dt)) for a in ("ldaux", "ldaux2") if a in ch]
    return gsum_terms(odt, parts, nout, n1, ld1, y1, ld2, y2)
