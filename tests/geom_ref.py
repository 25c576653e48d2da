"""How the HBM-bound passes around the convolutions split a sample's pixels over blocks, pixel slots and loop iterations (NumPy, CPU only).

A restatement of csrc/elem.h (pix_chunks, PixMap) and of the launchers that call it, so that a test case can DECLARE the geometry class it is
there for -- several blocks per sample, a shorter last chunk, a chunk that is no multiple of the pixel slots, idle threads, leftover pixels
behind the interleaved tiles, a pooled chunk boundary inside a row of the half-size map, more blocks than staging slots -- and
test_elem_geometry_cpu.py can hold it to that claim at the knob values the case sets.  A later change of a default block target then turns the
case red there instead of silently shrinking it to one block per sample.

  pix_chunks                    csrc/elem.h:30-42
  PixMap (PP, active threads)   csrc/elem.h:13-23; the eight-channel reduce: csrc/instnorm_bwd_2pass.hip:110-112
  chunk = cdiv(hw, nch), grid = cdiv(hw, chunk)
      in_stats       (target 4096)                   csrc/instnorm.hip:96-99          one pixel per iteration
      in_apply       ("elem.stream_blocks")          csrc/instnorm.hip:157-161        U = 4 (fp32) / 8 (bf16), 129-149
      in_apply_pool, in_pool (over hq quads)         csrc/instnorm.hip:242-247, 259-264   U = 2, 193, 219-231
      in_bwd reduce  ("elem.reduce_blocks", 0 = 1024 fp32 / 512 bf16)   csrc/instnorm_bwd.hip:108-109, 140
                     four channels: U = 4 / 8, csrc/instnorm_bwd_2pass.hip:50-81; eight channels: U = 4, tiles, 141-187
      in_bwd apply   ("elem.apply_blocks")           csrc/instnorm_bwd.hip:110, 141, 211; U = 4 / 8, tiles for bf16: csrc/instnorm_bwd_2pass.hip:264-317
      lrelu_bwd      (target 4096, batch 1, all pixels of the call)     csrc/grad_sums.hip:179-182; U = 4 / 8, 135-168; slots: 170
  sample chunks ("elem.chunk_mb")                    csrc/instnorm_bwd.hip:103-107, 135-136

`visits` replays the loops of one sample's blocks and counts how often each pixel is touched; it is used by the CPU test only.
"""
import numpy as np

DEFAULTS = {"elem.reverse": 1, "elem.interleave": 1, "elem.nt_loads": 0, "elem.chunk_mb": 0, "elem.reduce_blocks": 0, "elem.apply_blocks": 4096,
            "elem.stream_blocks": 32768}
LRELU_RED_SLOTS = 64                      # include/shmgan_hip.h: SHM_LRELU_RED_SLOTS (test_elem_geometry_gpu.py checks it against ops.LRELU_RED_SLOTS)
F32, BF16, GF32 = "f32", "bf16", "gf32"   # gf32: SHM_BF16_GF32, bf16 activations with the gradient signal in fp32
R8 = "in_bwd_reduce8_kernel + in_bwd_apply_kernel"
R4 = "in_bwd_reduce_kernel + in_bwd_apply_kernel"


def cdiv(a, b):
    return -(-a // b)


def pix_chunks(npix, batch, c, blocks):
    """csrc/elem.h:30-42 with `blocks` already resolved (the caller reads "elem.stream_blocks" where the source passes 0)."""
    min_iter = 8 if blocks > 4096 else 16
    pp = 256 // (c // 4)
    want = (blocks + batch - 1) // batch
    maxc = npix // (pp * min_iter)
    return max(1, min(want, maxc))


def geometry(npix, batch, c, blocks, U=1, lanes=4):
    """One pass over `npix` pixels (or quads) per sample: lanes = channels per thread (8: the bf16 reduce), U = its unroll."""
    lanes_c = c // lanes
    pp = 256 // lanes_c
    nch = pix_chunks(npix, batch, c, blocks)
    chunk = cdiv(npix, nch)
    grid = cdiv(npix, chunk)
    tile = U * pp
    return {"npix": npix, "grid": grid, "chunk": chunk, "last": npix - (grid - 1) * chunk, "PP": pp, "active": pp * lanes_c, "rem": chunk % pp, "U": U,
            "tile": tile, "ntiles": npix // tile, "tail": npix % tile}


def wide8(dt, c):
    """csrc/instnorm_bwd.hip:69-70 for the dense 16-byte aligned tensors of the tests: eight channels per thread in the reduce pass"""
    return dt in (BF16, GF32) and c % 8 == 0


def pass_geometry(name, dt, batch, h, w, c, knobs=None):
    """The geometry of pass `name` ("stats", "apply", "pool", "reduce", "bwd_apply", "lrelu") at the knob values of a case.
    lrelu: one call over batch * h * w pixels.  Adds "interleave" / "reverse": whether the pass takes that walk at these knobs."""
    k = dict(DEFAULTS, **(knobs or {}))
    hw = h * w
    u48 = 4 if dt == F32 else 8
    if name == "stats":
        g = geometry(hw, batch, c, 4096)
        il = rev = False
    elif name == "apply":
        g = geometry(hw, batch, c, k["elem.stream_blocks"], u48)
        il, rev = False, bool(k["elem.reverse"])
    elif name == "pool":
        g = geometry((h // 2) * (w // 2), batch, c, k["elem.stream_blocks"], 2)
        il, rev = False, bool(k["elem.reverse"])
    elif name == "reduce":
        blocks = k["elem.reduce_blocks"] or (1024 if dt == F32 else 512)
        g = geometry(hw, batch, c, blocks, 4, 8) if wide8(dt, c) else geometry(hw, batch, c, blocks, u48)
        il, rev = wide8(dt, c) and bool(k["elem.interleave"]), bool(k["elem.reverse"])
    elif name == "bwd_apply":
        g = geometry(hw, batch, c, k["elem.apply_blocks"], u48)
        il, rev = dt != F32 and bool(k["elem.interleave"]), False
    elif name == "lrelu":
        g = geometry(batch * hw, 1, c, 4096, u48)
        il = rev = False
    else:
        raise KeyError(name)
    g["interleave"], g["reverse"] = il, rev
    return g


def sample_chunks(dt, batch, h, w, c, pooled=False, rank1=False, chunk_mb=0):
    """csrc/instnorm_bwd.hip:103-107, 135-136: the samples per launch pair of the two-pass shm_in_bwd, e.g. [2, 1]"""
    hw = h * w
    esz_a = 4 if dt == F32 else 2
    esz_g = 2 if dt == BF16 else 4
    per_sample = hw * c * (esz_a + (0 if rank1 else esz_g)) + (hw // 4 * c * esz_g if pooled else 0)
    per = batch
    if chunk_mb and per_sample * batch > (chunk_mb << 20):
        per = max(1, (chunk_mb << 20) // per_sample)
    return [min(per, batch - n0) for n0 in range(0, batch, per)]


# ---------------------------------------------------------------------------------------------------------------------
def visits(g, reverse=False, interleave=False, reverse_tiles=False, quads_of=None):
    """How often the blocks of ONE sample touch each pixel: every (block, pixel slot, iteration) of the loops the kernels run.

      contiguous   p = p0 + pp; the U-times unrolled main loop while p + (U - 1) PP < p1, then the one-slot tail loop while p < p1
      reverse      block b takes chunk grid - 1 - b (in_apply, the pooled passes, both reduce kernels)
      interleave   block b takes the whole tiles b, b + grid, ...; block 0 then takes the pixels behind the last whole tile one slot at a time
                   (in_bwd_apply_kernel); reverse_tiles: tiles ntiles - 1 - b, ntiles - 1 - b - grid, ... down to 0 (in_bwd_reduce8_kernel under
                   "elem.reverse")
      quads_of     (h, w): the pass walks the (h / 2)(w / 2) quads of the half-size map and touches the four pixels of each: the count is over
                   the h * w pixels of the full map

    Returns (count per pixel, pixels touched by a tail loop as a boolean mask)."""
    npix, grid, chunk, PP, U = g["npix"], g["grid"], g["chunk"], g["PP"], g["U"]
    cnt = np.zeros(npix, np.int64)
    tail = np.zeros(npix, bool)
    tile, ntiles = U * PP, npix // (U * PP)
    for b in range(grid):
        bx = grid - 1 - b if reverse else b
        p0, p1 = bx * chunk, min(npix, bx * chunk + chunk)
        for pp in range(PP):
            if interleave:
                pend = ntiles * tile
                p = ((ntiles - 1 - b) if reverse_tiles else b) * tile + pp
                step = (-grid if reverse_tiles else grid) * tile
                while p >= 0 and p + (U - 1) * PP < pend:
                    for u in range(U):
                        cnt[p + u * PP] += 1
                    p += step
                p = pend + pp if b == 0 else npix
                while p < npix:
                    cnt[p] += 1
                    tail[p] = True
                    p += PP
            else:
                p = p0 + pp
                while p + (U - 1) * PP < p1:
                    for u in range(U):
                        cnt[p + u * PP] += 1
                    p += U * PP
                while p < p1:
                    cnt[p] += 1
                    tail[p] = True
                    p += PP
    if quads_of is None:
        return cnt, tail
    h, w = quads_of
    wo = w // 2
    q = np.arange(npix)
    base = 2 * (q // wo) * w + 2 * (q % wo)
    full, ftail = np.zeros(h * w, np.int64), np.zeros(h * w, bool)
    for off in (0, 1, w, w + 1):
        np.add.at(full, base + off, cnt)
        ftail[base + off] |= tail
    return full, ftail


def pass_visits(name, dt, batch, h, w, c, knobs=None):
    g = pass_geometry(name, dt, batch, h, w, c, knobs)
    if name == "pool":
        return visits(g, reverse=g["reverse"], quads_of=(h, w))
    if g["interleave"]:
        return visits(g, interleave=True, reverse_tiles=name == "reduce" and g["reverse"])
    return visits(g, reverse=g["reverse"])


# ---------------------------------------------------------------------------------------------------------------------
# geometry classes a case may claim of a pass
CLASSES = {
    "multi": lambda g, w: g["grid"] >= 3,
    "two": lambda g, w: g["grid"] >= 2,
    "one": lambda g, w: g["grid"] == 1,
    "short_last": lambda g, w: g["last"] < g["chunk"],
    "ragged_pp": lambda g, w: g["rem"] != 0,
    "idle": lambda g, w: g["active"] < 256,
    "il_tail": lambda g, w: g["interleave"] and g["tail"] != 0 and g["grid"] >= 2,
    "contiguous": lambda g, w: not g["interleave"],
    "midrow": lambda g, w: any((b * g["chunk"]) % (w // 2) for b in range(1, g["grid"])),          # a pooled chunk starts inside a row of the half-size map
    "wrap": lambda g, w: g["grid"] > LRELU_RED_SLOTS,
    "long_main": lambda g, w: g["chunk"] >= 4 * g["tile"] and g["chunk"] % g["tile"] != 0,                 # many unrolled iterations, then the tail
    "pp1": lambda g, w: g["PP"] == 1,
}

RAGGED = ("multi", "short_last", "ragged_pp")
BOTH, ALL = (F32, BF16), (F32, BF16, GF32)


def _row(id, h, w, c, knobs=None, batch=2, dts=None, form=None, claims=None, split=None):
    return {"id": id, "h": h, "w": w, "c": c, "knobs": knobs or {}, "batch": batch, "dts": dts, "form": form, "claims": claims or {}, "split": split}


M20 = 1 << 20
# ---- the forward passes: in_stats, in_apply, and on even maps in_apply_pool, in_pool and avgpool2_fwd.  claims: {pass: classes, or {dtype: classes}}
FWD = [
    _row("64", 34, 38, 64, claims={"stats": RAGGED, "apply": RAGGED, "pool": ("two", "short_last", "ragged_pp", "midrow")}),
    _row("64-forward-walk", 34, 38, 64, {"elem.reverse": 0}, claims={"apply": RAGGED, "pool": ("two", "midrow")}),
    _row("64-stream256", 34, 38, 64, {"elem.stream_blocks": 256}, claims={"apply": RAGGED, "pool": ("one",)}),
    _row("64-stream1M", 34, 38, 64, {"elem.stream_blocks": M20, "elem.reverse": 0}, claims={"apply": RAGGED, "pool": ("two", "midrow")}),
    _row("256", 34, 38, 256, claims={"stats": RAGGED, "apply": RAGGED, "pool": RAGGED + ("midrow",)}),
    _row("256-forward-walk", 34, 38, 256, {"elem.reverse": 0}, claims={"apply": RAGGED, "pool": RAGGED + ("midrow",)}),
    _row("256-stream256", 34, 38, 256, {"elem.stream_blocks": 256}, claims={"apply": RAGGED, "pool": RAGGED + ("midrow",)}),
    _row("136-idle", 22, 26, 136, claims={"stats": RAGGED + ("idle",), "apply": RAGGED + ("idle",), "pool": ("two", "short_last", "ragged_pp", "midrow", "idle")}),
    _row("136-idle-forward-walk", 22, 26, 136, {"elem.reverse": 0, "elem.stream_blocks": 256}, claims={"apply": RAGGED + ("idle",)}),
    _row("48-idle", 34, 38, 48, claims={"stats": RAGGED + ("idle",), "apply": RAGGED + ("idle",), "pool": ("one", "idle")}),
    _row("20", 34, 38, 20, claims={"stats": ("one", "idle"), "apply": RAGGED + ("idle",)}),
    _row("20-forward-walk", 34, 38, 20, {"elem.reverse": 0}, claims={"apply": RAGGED + ("idle",)}),
    _row("17x23", 17, 23, 64, claims={"stats": ("one",), "apply": RAGGED}),
    _row("17x23-forward-walk", 17, 23, 64, {"elem.reverse": 0}, claims={"apply": RAGGED}),
    _row("1024", 6, 10, 1024, claims={"stats": ("multi", "pp1"), "apply": ("multi", "short_last", "pp1")}),
    _row("1020-idle", 6, 10, 1020, {"elem.reverse": 0}, claims={"stats": ("multi", "idle", "pp1"), "apply": ("multi", "short_last", "idle", "pp1")}),
]

# ---- InstanceNorm backward.  form: "plain" / "pooled" / "rank1" (shm_in_bwd, shm_in_bwd_rank1: reduce + apply) and "raw" / "raw-pooled"
# (shm_in_bwd_apply: the apply pass alone); a "+b" suffix asks for the bias gradient, "+s" for the per-sample dz sums as well.
_IL = {F32: RAGGED, BF16: RAGGED + ("il_tail",), GF32: RAGGED + ("il_tail",)}          # the bf16 forms walk tiles: leftover pixels on a multi-block grid
_CT = RAGGED + ("contiguous",)
BWD = [
    _row("64-plain", 34, 38, 64, form="plain+s", claims={"reduce": _IL, "bwd_apply": _IL}),
    _row("64-pooled", 34, 38, 64, form="pooled+b", claims={"reduce": _IL, "bwd_apply": _IL}),
    _row("64-rank1-forward-walk", 34, 38, 64, {"elem.reverse": 0}, dts=BOTH, form="rank1", claims={"reduce": _IL, "bwd_apply": _IL}),
    _row("64-raw", 34, 38, 64, form="raw+s", claims={"bwd_apply": _IL}),
    _row("64-raw-pooled-nt", 34, 38, 64, {"elem.nt_loads": 1}, form="raw-pooled+b", claims={"bwd_apply": _IL}),
    _row("64-contiguous-forward-walk", 34, 38, 64, {"elem.interleave": 0, "elem.reverse": 0}, form="plain+b", claims={"reduce": _CT, "bwd_apply": _CT}),
    _row("64-contiguous-pooled-nt", 34, 38, 64, {"elem.interleave": 0, "elem.nt_loads": 1}, form="pooled+s", claims={"reduce": _CT, "bwd_apply": _CT}),
    _row("64-raw-contiguous", 34, 38, 64, {"elem.interleave": 0}, form="raw-pooled", claims={"bwd_apply": _CT}),
    _row("64-reduce1", 34, 38, 64, {"elem.reduce_blocks": 1, "elem.interleave": 0}, form="plain+b", claims={"reduce": ("one", "long_main"), "bwd_apply": _CT}),
    _row("64-reduce1-tiles", 34, 38, 64, {"elem.reduce_blocks": 1}, form="pooled", claims={"reduce": ("one",), "bwd_apply": _IL}),
    _row("64-reduce3", 34, 38, 64, {"elem.reduce_blocks": 3}, dts=BOTH, form="rank1+b", claims={"reduce": ("two",), "bwd_apply": _IL}),
    _row("64-reduce1M-apply1M", 34, 38, 64, {"elem.reduce_blocks": M20, "elem.apply_blocks": M20}, form="pooled+b", claims={"reduce": _IL, "bwd_apply": _IL}),
    _row("64-apply256", 34, 38, 64, {"elem.apply_blocks": 256, "elem.reverse": 0}, dts=BOTH, form="rank1+s", claims={"reduce": _IL, "bwd_apply": _IL}),
    _row("64-raw-apply256", 34, 38, 64, {"elem.apply_blocks": 256}, form="raw+b", claims={"bwd_apply": _IL}),
    _row("64-raw-apply1M", 34, 38, 64, {"elem.apply_blocks": M20, "elem.nt_loads": 1}, form="raw-pooled+s", claims={"bwd_apply": _IL}),
    # "elem.chunk_mb" = 1 under the reversed blockIdx.y: the n0 offset.  Per sample: fp32 34 x 38 x 48: 1292 * 48 * (4 + 4) = 496128 B, two fit 1 MiB;
    # SHM_BF16_GF32 34 x 38 x 64: 1292 * 64 * (2 + 4) = 496128 B, two fit; bf16 pooled 34 x 38 x 64: 1292 * 64 * 4 + 323 * 64 * 2 = 372096 B, two fit
    # (three plain bf16 samples of 330752 B fit 1 MiB together: no split)
    _row("48-sample-chunks", 34, 38, 48, {"elem.chunk_mb": 1, "elem.reverse": 1}, batch=3, dts=(F32,), form="plain+s", split=[2, 1],
         claims={"reduce": ("multi", "short_last", "idle"), "bwd_apply": ("multi", "short_last", "idle")}),
    _row("64-sample-chunks", 34, 38, 64, {"elem.chunk_mb": 1, "elem.reverse": 1}, batch=3, dts=(GF32,), form="plain+s", split=[2, 1],
         claims={"reduce": _IL, "bwd_apply": _IL}),
    _row("64-sample-chunks-pooled", 34, 38, 64, {"elem.chunk_mb": 1, "elem.reverse": 1}, batch=3, dts=(BF16,), form="pooled+s", split=[2, 1],
         claims={"reduce": _IL, "bwd_apply": _IL}),
    _row("256-plain", 34, 38, 256, form="plain+s", claims={"reduce": _IL, "bwd_apply": _IL}),
    _row("256-pooled-forward-walk", 34, 38, 256, {"elem.reverse": 0}, form="pooled+b", claims={"reduce": _IL, "bwd_apply": _IL}),
    _row("256-raw-pooled", 34, 38, 256, form="raw-pooled+b", claims={"bwd_apply": _IL}),
    _row("136-idle-plain", 22, 26, 136, form="plain+b", claims={"reduce": {F32: RAGGED + ("idle",), BF16: RAGGED + ("idle", "il_tail"), GF32: RAGGED + ("idle", "il_tail")},
                                                                "bwd_apply": RAGGED + ("idle",)}),
    _row("136-idle-pooled-contiguous", 22, 26, 136, {"elem.interleave": 0}, form="pooled+s", claims={"reduce": _CT + ("idle",), "bwd_apply": _CT + ("idle",)}),
    _row("136-idle-raw", 22, 26, 136, {"elem.nt_loads": 1}, form="raw+s", claims={"bwd_apply": RAGGED + ("idle",)}),
    _row("48-idle-rank1", 34, 38, 48, dts=BOTH, form="rank1+b", claims={"reduce": ("multi", "short_last", "idle"), "bwd_apply": ("multi", "short_last", "idle")}),
    _row("48-idle-pooled", 34, 38, 48, {"elem.reduce_blocks": 3}, form="pooled+b", claims={"reduce": ("two", "idle"), "bwd_apply": ("multi", "short_last", "idle")}),
    # c = 20 (PP = 51) and the odd 17 x 23 map reach several blocks only with the eight-iteration floor of the targets above 4096
    _row("20-plain", 34, 38, 20, {"elem.reduce_blocks": M20, "elem.apply_blocks": M20}, form="plain+s", claims={"reduce": RAGGED + ("idle",), "bwd_apply": RAGGED + ("idle",)}),
    _row("17x23-plain", 17, 23, 64, {"elem.reduce_blocks": M20, "elem.apply_blocks": M20}, form="plain+b", claims={"reduce": ("multi", "short_last"), "bwd_apply": RAGGED}),
    _row("17x23-raw", 17, 23, 64, {"elem.apply_blocks": M20}, form="raw+s", claims={"bwd_apply": RAGGED}),
    _row("1024-plain", 6, 10, 1024, form="plain+s", claims={"reduce": ("multi",), "bwd_apply": ("multi", "pp1")}),          # (the eight-channel reduce has two pixel slots)
    _row("1020-idle-rank1", 6, 10, 1020, dts=BOTH, form="rank1+b", claims={"reduce": ("multi", "idle", "pp1"), "bwd_apply": ("multi", "idle", "pp1")}),
]

# ---- LeakyReLU backward: one call over batch * h * w pixels
LRELU = [
    _row("1024-slot-wrap", 34, 38, 1024, claims={"lrelu": ("wrap", "pp1")}),          # 2584 pixels = 152 chunks of 17
    _row("64", 34, 38, 64, claims={"lrelu": RAGGED}),
    _row("136-idle", 22, 26, 136, claims={"lrelu": RAGGED + ("idle",)}),
    _row("1020-idle", 6, 10, 1020, claims={"lrelu": ("multi", "short_last", "idle", "pp1")}),
]


def row_dts(row, family):
    return row["dts"] or (BOTH if family == "fwd" else ALL)


def cases(table, family):
    """(row, dtype) pairs and their ids for pytest.mark.parametrize"""
    out = [(r, dt) for r in table for dt in row_dts(r, family)]
    return out, [f"{r['id']}-{dt}" for r, dt in out]


def claimed(row, name, dt):
    cl = row["claims"].get(name, ())
    return cl[dt] if isinstance(cl, dict) else cl


def row_passes(row, family):
    """the passes a row runs, whether it claims a class of them or not"""
    if family == "fwd":
        return ("stats", "apply") + (("pool",) if row["h"] % 2 == 0 and row["w"] % 2 == 0 else ())
    if family == "lrelu":
        return ("lrelu",)
    return ("bwd_apply",) if row["form"].startswith("raw") else ("reduce", "bwd_apply")


def expected_pair(dt, c):
    """shm_last_kernel() of a two-pass shm_in_bwd (tests/test_in_bwd_plan_gpu.py: R4 / R8)"""
    return R8 if wide8(dt, c) else R4
