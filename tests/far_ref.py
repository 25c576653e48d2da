"""Harness and case table of the far-extent tests (test_far_cpu.py for their teeth, test_far_gpu.py on the device).  No GPU import.

The convolutions address their operands with 32-bit byte offsets into buffer descriptors and refuse an operand of LIM = 0xfffffff0 bytes or
more; outputs of 4 GiB or more take 64-bit-address epilogues and another choice of kernel; the InstanceNorm, pooling and elementwise kernels
index through size_t by casts placed term by term.  None of that shows below 2 GiB.  A tensor of a few hundred pixels whose PITCH is about
a million elements has the extent -- and produces the offsets `pixel * ld * esz` -- of a real activation of that size while holding a few
hundred KiB of data, so the tests of pitch_ref.py / test_pitch_gpu.py run again with one pitch argument FAR and every other tensor tight.

WINDOWS names where an extent lands; far_ld() gives the pitch for a window, straddles() is the assertion that makes a window mean something:
one pixel lies wholly below the threshold the window names and the next pixel starts at or above it, so that both sides of the threshold
are read or written (a pitch whose extent merely passes the threshold can leave every pixel below it: the last pixel's gap does the passing).

Parents are filled, written, read back and scanned in chunks of at most CHUNK elements through slices of the flat parent (a 64-bit pointer
offset formed on the host, then small indices), so the checks do not rest on large-tensor indexing of the library that runs them.  Bands:
a wrong address must land in allocated memory and fail an assertion.  In front of an operand below 4 GiB lie 2 GiB + 64 KiB (where a 32-bit
byte offset sign-extended into a 64-bit address lands), in front of an E31 / E32 operand its own extent (where an `int` element index gone
negative lands); behind it util.guard_elems.

Every quantity takes the address width W as a parameter: the device table is built with W = 32, the CPU teeth with W = 16.
"""
import numpy as np
import torch

import pitch_ref as R
from util import SENTINEL, guard_elems

CHUNK = 1 << 26          # elements per fill, copy or scan (measured: the scan holds about nine bytes of temporaries per element)


def lim(W=32):
    """the first operand extent in bytes the convolutions refuse (0xfffffff0 at W = 32): 2^W - 1 is "outside the image" """
    return (1 << W) - 16


# window -> (unit, thresholds(W), doc).  unit "B": the thresholds are bytes; "E": elements.
WINDOWS = {
    "W2": ("B", lambda W: (1 << (W - 1),), "just over 2^(W-1) bytes: the first offsets with the top bit set"),
    "W4-": ("B", lambda W: (1 << (W - 1),), "the largest extent below lim(W): top-bit offsets, the last pixel within one pitch of the limit"),
    "W4+": ("B", lambda W: (1 << W,), "just over 2^W bytes: no 32-bit offset reaches the last pixel"),
    "E31": ("E", lambda W: (1 << (W - 1),), "just over 2^(W-1) elements"),
    "E32": ("E", lambda W: (1 << W,), "just over 2^W elements"),
    # three samples: the BASE of sample 2, `2 * hw * ld`, is at or above the threshold and sample 1 ends below it, so that the batch term
    # `n * hw * ld` crosses on its own (in E31 / E32 only the last pixel crosses: `2 * hw * ld` is two thirds of the threshold there)
    "B31": ("E", lambda W: (1 << (W - 1),), "three samples, the third starts at or above 2^(W-1) elements"),
    "B32": ("E", lambda W: (1 << W,), "three samples, the third starts at or above 2^W elements"),
}


def pivot(window, npix):
    """the pixel that starts at or above the window's threshold in the smallest such pitch: the last one, or (B31 / B32) the first of sample 2"""
    if window in ("B31", "B32"):
        assert npix % 3 == 0 and npix >= 6, npix
        return 2 * (npix // 3)
    return npix - 1


def straddles(npix, ld, c, t_el):
    """a pixel lies wholly below element t_el of the tensor and the next pixel starts at or above it"""
    p = -(-t_el // ld) - 1
    return 0 <= p and p + 1 < npix and p * ld + c <= t_el and (p + 1) * ld >= t_el


def far_ld(window, npix, c, esz, q, W=32):
    """The pitch (a multiple of the quantum q) of a tensor of npix pixels of c channels whose extent npix * ld * esz lands in `window`:
    W4-: the largest with an extent below lim(W); every other window: the smallest for which the LAST pixel starts at or above the threshold."""
    unit, thr, _ = WINDOWS[window]
    assert npix >= 3, npix
    if window == "W4-":
        ld = (lim(W) - 1) // (npix * esz) // q * q
    else:
        t_el = thr(W)[0] // (esz if unit == "B" else 1)
        ld = R.up(-(-t_el // pivot(window, npix)), q)
    check_window(window, npix, ld, c, esz, q, W)
    return ld


def check_window(window, npix, ld, c, esz, q, W=32):
    """the straddle assertion and the window's own bounds"""
    unit, thr, _ = WINDOWS[window]
    assert ld >= c and ld % q == 0, (window, ld, c)
    for t in thr(W):
        t_el = t // (esz if unit == "B" else 1)
        assert straddles(npix, ld, c, t_el), (window, npix, ld, c, t_el)
    ext = npix * ld * esz
    if window in ("W2", "W4-"):
        assert ext < lim(W), (window, ext)
    if window == "W4-":
        assert npix * (ld + q) * esz >= lim(W), (window, ext)          # one quantum wider is refused
    if window == "W4+":
        assert ext >= 1 << W, (window, ext)
    if window != "W4-":          # "just over": the smallest such pitch -- one quantum less and the last pixel starts below the threshold
        t_el = thr(W)[0] // (esz if unit == "B" else 1)
        pv = pivot(window, npix)
        assert pv * (ld - q) < t_el <= pv * ld and (pv - 1) * ld + c <= t_el, (window, ld)


def refused_ld(npix, c, esz, q, W=32):
    """the smallest pitch whose extent reaches lim(W): far_ld("W4-") plus one quantum"""
    ld = far_ld("W4-", npix, c, esz, q, W) + q
    assert npix * ld * esz >= lim(W) > npix * (ld - q) * esz
    return ld


def lead_for(window, shape, ld, esz, W=32):
    """Leading band in elements (a multiple of 64): an operand below 2^W bytes gets 2^(W-1) bytes + 2^(W-16) bytes (2 GiB + 64 KiB), an E31 / E32
    operand its own extent; a B31 / B32 operand 2^(W-1) elements where its extent is larger (an index held in a signed W-bit integer is never below
    -2^(W-1)); never less than util.guard_elems."""
    npix = int(np.prod(shape[:-1]))
    if window in ("B31", "B32"):
        n = min(npix * ld, 1 << (W - 1))
    elif window in ("E31", "E32"):
        n = npix * ld
    else:
        n = ((1 << (W - 1)) + (1 << max(W - 16, 4))) // esz
    return R.up(max(n, guard_elems(shape)), 64)


def trail_for(shape):
    return R.up(guard_elems(shape), 64)


class Far:
    """The layout of one far tensor: what a case of the device table holds in place of a layout name of pitch_ref.LAYOUTS."""

    def __init__(self, window, ld, lead=None, W=32):
        self.window, self.ld, self.lead, self.W = window, int(ld), lead, W

    def __repr__(self):
        return f"Far({self.window}, ld={self.ld})"


# ------------------------------------------------------------------------------------------------------- parents, in chunks
def _rows(ld, chunk):
    return max(1, chunk // ld)


_ARENA = {}


def arena(nbytes, device):
    """One flat byte buffer per device that only grows: the far parents of successive cases are carved from it (allocating and freeing 6 to 17 GiB
    per case cost ten times the fill and the scan).  One far parent is alive at a time: a case has one far operand, and its results are host
    copies before the next case begins."""
    a = _ARENA.get(str(device))
    if a is None or a.numel() < nbytes:
        _ARENA.pop(str(device), None)
        del a
        a = _ARENA[str(device)] = torch.empty((int(nbytes),), dtype=torch.uint8, device=device)
    return a


def drop_arena():
    _ARENA.clear()


def far_view(parent_fill, shape, ld, c_off, lead, trail, dtype=torch.float32, device="cpu", chunk=CHUNK, use_arena=False):
    """pitch_ref.view_of with the bands as parameters and the fill in chunks.  Returns (view, parent).  use_arena: the parent is the front of arena()."""
    shape = tuple(int(s) for s in shape)
    c = shape[-1]
    assert ld >= c_off + c and c_off >= 0, (ld, c_off, c)
    assert trail >= guard_elems(shape) and lead >= guard_elems(shape)
    npix = int(np.prod(shape[:-1]))
    total = lead + npix * ld + trail
    if use_arena:
        esz = torch.empty(0, dtype=dtype).element_size()
        parent = arena(total * esz, device)[:total * esz].view(dtype)
    else:
        parent = torch.empty((total,), dtype=dtype, device=device)
    for i in range(0, total, chunk):
        parent[i:i + chunk].fill_(float(parent_fill))
    strides, s = [], ld
    for d in reversed(shape[:-1]):
        strides.append(s)
        s *= d
    return parent.as_strided(shape, tuple(reversed(strides)) + (1,), lead + c_off), parent


def _groups(t, chunk):
    """A pitched view [..., c] as (r0, [rows, c] view of rows r0 .. of its flat pixel list) pieces spanning at most `chunk` elements each: every
    piece is re-based on its own storage offset, so the copy that follows indexes within the piece."""
    c, ld = t.shape[-1], t.stride(-2) if t.dim() > 1 else t.shape[-1]
    npix = t.numel() // c
    step = _rows(ld, chunk)
    for r0 in range(0, npix, step):
        r = min(step, npix - r0)
        yield r0, r, t.as_strided((r, c), (ld, 1), t.storage_offset() + r0 * ld)


def is_far(t, chunk=CHUNK):
    """a pitched pixel list (every leading stride the product of the ones behind it) that spans more than `chunk` elements"""
    if t.dim() < 2 or t.stride(-1) != 1:
        return False
    s = t.stride(-2)
    for d in range(t.dim() - 2, 0, -1):
        if t.stride(d - 1) != s * t.shape[d]:
            return False
        s = t.stride(d - 1)
    return t.numel() // t.shape[-1] * t.stride(-2) > chunk


def scatter(view, src, chunk=CHUNK):
    """view[...] = src (same shape; src on the host or the device), piece by piece"""
    src2 = src.reshape(-1, view.shape[-1])
    for r0, r, piece in _groups(view, chunk):
        piece.copy_(src2[r0:r0 + r].to(piece.dtype))


def gather(view, chunk=CHUNK):
    """the slice as a contiguous host tensor, piece by piece: the only part of a parent that is copied to the host"""
    out = torch.empty(view.shape, dtype=view.dtype)
    out2 = out.view(-1, view.shape[-1])
    for r0, r, piece in _groups(view, chunk):
        out2[r0:r0 + r] = piece.cpu()
    return out


def _bits(t):
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32 if t.element_size() == 4 else torch.int64)


def far_outside_untouched(parent, shape, ld, c_off, lead, fill=SENTINEL, chunk=CHUNK):
    """pitch_ref.outside_untouched where the parent lives, in chunks: both bands and every gap are bit-equal to the fill."""
    shape = tuple(int(s) for s in shape)
    c, npix = shape[-1], int(np.prod(shape[:-1]))
    assert parent.numel() >= lead + npix * ld
    want = int(_bits(torch.full((1,), float(fill), dtype=parent.dtype))[0])
    end = lead + npix * ld

    bad = torch.zeros((), dtype=torch.int64, device=parent.device)          # differing elements, counted where the parent lives; one read-back

    def flat(a, b):
        nonlocal bad
        for i in range(a, b, chunk):
            bad += torch.count_nonzero(_bits(parent[i:min(i + chunk, b)]) != want)

    flat(0, lead)
    flat(end, parent.numel())
    step = _rows(ld, chunk)
    for r0 in range(0, npix, step):
        r = min(step, npix - r0)
        blk = _bits(parent[lead + r0 * ld:lead + (r0 + r) * ld]).view(r, ld)
        cols = max(1, chunk // r)          # (a pitch longer than a chunk: its gap goes by column ranges)
        for a, b in ((0, c_off), (c_off + c, ld)):
            for lo in range(a, b, cols):
                bad += torch.count_nonzero(blk[:, lo:min(b, lo + cols)] != want)
    return int(bad) == 0


# --------------------------------------------------------------------------------------------------- the strided model, W bits wide
# pitch_ref.model_op with its addresses formed as the kernels form them: a byte offset `(pixel * ld + channel) * esz` in a W-bit register.
FAR_FAULTS = ("offset-wraps", "offset-sign-extends", "int-element-index", "extent-clamped", "outside-collides", "batch-term-in-int")


def far_address(p, ch, ld, esz, W, fault, ext_bytes, hw=None):
    """Element index relative to the tensor's base of channel ch of pixel p, or None for "reads zero / store dropped" (a buffer access beyond the
    descriptor's extent).  The clean path is the 64-bit one."""
    el = p * ld + ch
    off = el * esz
    if fault == "offset-wraps":
        off %= 1 << W
    elif fault == "offset-sign-extends":
        off %= 1 << W
        if off >= 1 << (W - 1):
            off -= 1 << W
    elif fault == "int-element-index":
        el %= 1 << W
        if el >= 1 << (W - 1):
            el -= 1 << W
        off = el * esz
    elif fault == "batch-term-in-int":
        # base + n * hw * ld + (size_t)p * ld with the first product formed in a signed W-bit integer (hw: pixels per sample)
        n, pin = divmod(p, hw)
        b = n * hw * ld % (1 << W)
        if b >= 1 << (W - 1):
            b -= 1 << W
        off = (b + pin * ld + ch) * esz
    elif fault == "extent-clamped":
        if off + esz > min(ext_bytes, lim(W)):
            return None
    elif fault == "outside-collides":
        # the last 16-byte piece below 2^W is taken for the "outside" marker 2^W - 1 (the marker is compared after rounding down to the piece)
        if off % (1 << W) >= (1 << W) - 16:
            return None
    return off // esz


def far_model_op(flat, ptr, ld, npix, esz, W, fault=None, on=("x1", "y1"), hw=None):
    """pitch_ref.model_op (same tensors, same result) with every access of the tensors in `on` addressed through far_address."""
    ext = {t: npix * ld[t] * esz for t in ld}

    def idx(t, p, ch):
        a = far_address(p, ch, ld[t], esz, W, fault if t in on else None, ext[t], hw)
        return None if a is None else ptr[t] + a

    def rd(t, p):
        out = np.zeros(16)
        for ch in range(16):
            i = idx(t, p, ch)
            out[ch] = 0.0 if i is None else flat[t][i]
        return out

    def wr(t, p, v):
        for ch in range(16):
            i = idx(t, p, ch)
            if i is not None:
                flat[t][i] = v[ch]

    red = np.zeros(16)
    for p in range(npix):
        y = 2.0 * np.concatenate([rd("x1", p), rd("x2", p)])[::-1] + 1.0
        wr("y1", p, y[:16])
        wr("y2", p, y[16:])
        red += y[:16] * rd("aux", p)
    return red


# ------------------------------------------------------------------------------------------------------------ the device test's table
def _first(names):
    """the first record of pitch_ref.FAMILIES under each of `names`"""
    out = []
    for nm in names:
        out.append(next(f for f in R.FAMILIES if f["name"] == nm))
    return out


CONV_FAMILIES = ("fwd-halo", "fwd-dma", "fwd-wreg", "fwd-wreg-f32-narrow", "fwd-x3", "fwd-norm-exact", "fwd-norm-scaled", "fwd-gsum-s2", "transpose",
                 "dgrad-s2", "dgrad-split", "dgrad-gsum", "dgrad-s2-gsum",
                 "wgrad-generic", "wgrad-halo", "wgrad-halo-blocks3", "wgrad-halo-rows2", "wgrad-halo8", "wgrad-concat", "wgrad-thin", "wgrad-s2",
                 "wgrad-s2-halo8", "wgrad-x3", "wgrad-norm")
# one forced variant per family is enough for the address arithmetic of its kernel; the families that list several kernels keep one of each KIND
CONV_VARIANTS = {"fwd-halo": ("halo128", "halo64_st"), "fwd-dma": ("dma128x128", "dma64x64"), "transpose": ("dma128x128", "phase4"),
                 "dgrad-s2": ("dma128x128", "phase4"), "dgrad-split": ("halo64_st", "dma128x128", "auto"), "dgrad-gsum": ("halo64_st", "dma128x128", "auto"),
                 "dgrad-s2-gsum": ("phase4", "dma128x128"), "fwd-norm-exact": ("halo64_st", "auto"), "fwd-norm-scaled": ("halo64_st", "auto"),
                 "fwd-gsum-s2": ("dma128x128",)}


def npix_of(fam, arg):
    """pixels of the tensor behind pitch argument `arg` of a family"""
    sh, e = fam["shape"], fam["entry"]
    n, h, w = sh["n"], sh["h"], sh["w"]
    if e in ("conv2d_fwd", "conv2d_in_fwd"):
        s = sh["s"]
        return n * h * w if arg in ("ldx", "ldx2") else n * -(-h // s) * -(-w // s)
    if e == "conv2d_transpose_fwd":
        return n * h * w if arg == "ldx" else n * 4 * h * w
    if e == "conv2d_dgrad":
        s = sh["s"]
        return n * (h // s) * (w // s) if arg == "lddy" else n * h * w
    if e == "conv2d_wgrad":
        s = sh["s"]
        return n * -(-h // s) * -(-w // s) if arg == "lddy" else n * h * w
    pooled = {"in_apply_pool": ("ldp",), "in_pool": ("ldp",), "avgpool2_fwd": ("ldy",), "in_bwd": ("ldg2",), "in_bwd_apply": ("ldg2",)}
    return n * (h // 2) * (w // 2) if arg in pooled.get(e, ()) else n * h * w


def chan_of(fam, arg):
    """channels READ OR WRITTEN through pitch `arg` (the thin first layer of the weight gradient reads its zero-padded pitch of 16 / 32)"""
    return fam["ch"][arg]


def arg_dt(fam, dt, arg):
    """element type of the tensor behind `arg`: outputs of SHM_BF16_GF32 are fp32"""
    roles = R.ENTRY_POINTS[fam["entry"]]
    return R.out_dt(fam, dt) if arg in roles["out"] else dt


def far_case(fam, dt, arg, window, W=32):
    """{arg: Far} with the pitch of `window` for the tensor behind `arg`"""
    adt = arg_dt(fam, dt, arg)
    esz, q = R.ESZ[adt], R.Q[adt]
    c = chan_of(fam, arg)
    if fam["entry"] == "conv2d_wgrad" and arg == "ldx" and not fam["shape"]["c2"]:
        kb = 16 if dt == "f32" else 32
        c = c if c % kb == 0 else R.up(c, kb)
    return {arg: Far(window, far_ld(window, npix_of(fam, arg), c, esz, q, W), None, W)}


def conv_cases(fam, dt):
    """[(id, case, kind)] of a convolution family: every input and aux pitch at W4- (W2 too for the first input), every output pitch at W4-
    and at W4+.  kind "same": the tight call's kernel and bits; "flat": those of the tight call under tapgemm.flat_epilogue = 1."""
    roles = R.ENTRY_POINTS[fam["entry"]]
    out = []
    for a in roles["in"] + roles["aux"]:
        if a in fam["ch"]:
            out.append((f"{a}-W4-", far_case(fam, dt, a, "W4-"), "same"))
    first = next(a for a in roles["in"] if a in fam["ch"])
    out.append((f"{first}-W2", far_case(fam, dt, first, "W2"), "same"))
    for a in roles["aux"]:          # one quantum wider: no 32-bit offset reaches its end, and nothing refuses it -- the sums go to the reduce pass
        if a in fam["ch"]:
            ld = next(iter(far_case(fam, dt, a, "W4-").values())).ld + R.Q[dt]
            out.append((f"{a}-LIM", {a: Far("LIM", ld)}, "aux"))
    for a in roles["out"]:
        if a in fam["ch"]:
            out.append((f"{a}-W4-", far_case(fam, dt, a, "W4-"), "same"))
            # [lim, 2^32): what is refused of an input is, for an output, the first extent of the 64-bit-address path
            odt = arg_dt(fam, dt, a)
            ld = next(iter(far_case(fam, dt, a, "W4-").values())).ld + R.Q[odt]
            out.append((f"{a}-LIM", {a: Far("LIM", ld)}, "flat"))
            out.append((f"{a}-W4+", far_case(fam, dt, a, "W4+"), "flat"))
    return out


def conv_table():
    """(family record, variant, dt, knobs) of the convolution tests"""
    for fam in _first(CONV_FAMILIES):
        for dt in fam["dts"]:
            for v in CONV_VARIANTS.get(fam["name"], fam["variants"][:1]):
                for kn in R.knob_sets(fam):
                    yield fam, v, dt, kn


# InstanceNorm side: the smallest shape of IN_SHAPES / BWD_SHAPES with three samples; the one-pass kernels need whole slices (their own shapes,
# three samples).  "-one": a single sample, so that hw * ld passes the threshold on its own and the in-image term p * ld crosses too.
IN_SHAPE = (3, 4, 6, 48)
ONE_SHAPE = (2, 16, 16, 64)          # the single-sample cases: the next shape up (a sample of 4 x 6 has six pooled pixels: its far parent and the band
#                                      of the same extent in front would pass 20 GiB, the straddling pitch being npix / (npix - 1) of the threshold)
assert IN_SHAPE in R.IN_SHAPES and IN_SHAPE in R.BWD_SHAPES and ONE_SHAPE in R.IN_SHAPES and ONE_SHAPE in R.BWD_SHAPES


def _with_n(fam, n, shape4=None):
    sh = dict(fam["shape"], n=n)
    if shape4:
        sh.update(h=shape4[1], w=shape4[2], c=shape4[3])
    return dict(fam, shape=sh)


def in_families():
    """one record per InstanceNorm family name of pitch_ref.FAMILIES, on three samples"""
    seen, out = set(), []
    for f in R.FAMILIES:
        if f["entry"] not in R.INSTNORM or f["name"].endswith(("-dbias", "-none")):          # (the sums of the bias gradient index no activation)
            continue
        sh = f["shape"]
        key = (f["name"], sh.get("g2"), sh.get("sums"), str(f["knobs"]))
        one_pass = f["name"].startswith("in_bwd-one-pass")
        if key in seen or (not one_pass and (sh["n"], sh["h"], sh["w"], sh["c"]) != IN_SHAPE):
            continue
        seen.add(key)
        out.append(_with_n(f, 3))
    return out


def in_cases(fam, dt):
    """[(id, family record to run, case)]: every pitch argument at E31 (bf16: E32 too) on three samples, and at E31 on one sample."""
    out = []
    for a in fam["ch"]:
        # B31 / B32: bf16 only -- in fp32 three samples with 2 * hw * ld >= 2^31 elements are 12 GiB behind a band of 8 GiB
        for win in ("E31",) + (("E32", "B31", "B32") if dt == "bf16" else ()):
            out.append((f"{a}-{win}", fam, far_case(fam, dt, a, win)))
        one = _with_n(fam, 1, None if fam["name"].startswith("in_bwd-one-pass") else ONE_SHAPE)
        out.append((f"{a}-E31-one", one, far_case(one, dt, a, "E31")))
    return out


def in_table():
    for fam in in_families():
        for dt in fam["dts"]:
            for kn in R.knob_sets(fam):
                yield fam, dt, kn


def case_bytes(fam, dt, case):
    """device bytes of the far parent of a case (the figure a test holds against the free memory)"""
    (arg, far), = case.items()
    adt = arg_dt(fam, dt, arg)
    c = chan_of(fam, arg)
    npix = npix_of(fam, arg)
    shape = (1, npix, c)           # (util.guard_elems from above: 16 rows as wide as the whole tensor)
    lead = lead_for(far.window, shape, far.ld, R.ESZ[adt], far.W)
    return (lead + npix * far.ld + trail_for(shape)) * R.ESZ[adt]
