"""Input builders and float64 references for the kernels between the networks and the loss value (csrc/color.hip, csrc/imgloss.hip) at the
shapes and inputs where they take another path: grid-stride loops that iterate, waves that straddle the end of a tensor, ranges that
collapse to zero, extremes of rescale_01 in one plane or the other.  test_loss_colour_edges_cpu.py proves on the CPU that every
engineered input is in the case it claims; test_loss_colour_edges_gpu.py runs the kernels on it.

Every builder returns float64 arrays that hold float32 VALUES (r32): the device and the float64 reference then see the same numbers, so
`den == 0`, the position of a minimum and `g * gscale == 1` mean the same on both sides.  The references are the oracle's own functions
(oracle/step_torch.py, oracle/tf_ops_np.py), evaluated in float64.
"""
from types import SimpleNamespace

import numpy as np
import torch

from oracle import step_torch as st
from oracle import tf_ops_np as tn
from util import rel_l2


def r32(a):
    """float64 array of the float32 roundings of a (what a device tensor made from it holds)"""
    return np.ascontiguousarray(a, dtype=np.float32).astype(np.float64)


def t64(a):
    return torch.from_numpy(np.asarray(a, dtype=np.float64))


# ---------------------------------------------------------------------------------------------------------------------------------------
# guard bands: an output is allocated GUARD_ROWS rows longer than the kernel may write and filled with one byte value, so that a store
# past the end is seen as a changed byte (0xA5A5A5A5 is -2.9e-16 as a float, 0xA5A5 the same as a bf16: a number no kernel here produces)

GUARD_ROWS = 256
SENT_BYTE = 0xA5


def guarded(rows, cols, dtype, device):
    """(raw bytes of the whole allocation, its first `rows` rows as a [rows, cols] tensor of dtype)"""
    item = torch.empty((), dtype=dtype).element_size()
    raw = torch.full(((rows + GUARD_ROWS) * cols * item,), SENT_BYTE, dtype=torch.uint8, device=device)
    return raw, raw.view(dtype).view(rows + GUARD_ROWS, cols)[:rows]


def guard_intact(raw, payload):
    """every byte behind the payload still holds the fill"""
    used = payload.numel() * payload.element_size()
    return bool((raw[used:] == SENT_BYTE).all().item())


# ---------------------------------------------------------------------------------------------------------------------------------------
# clip + Adam (adam_clip_kernel: at most 8192 blocks of 256 threads, grid-stride)

ADAM_GRID = 8192 * 256
ADAM_TAIL = 77
ADAM_SIZES = (1, 255, ADAM_GRID + ADAM_TAIL)
ADAM_STEP, ADAM_LR0, ADAM_B1 = 3, 2e-5, 0.5
ADAM_B2 = float(np.float32(0.99))       # the betas, eps and gscale reach the kernel as floats: the reference takes the same numbers
ADAM_EPS = float(np.float32(1e-7))
ADAM_GSCALE = 0.5
# g * gscale: below -1, exactly -1, inside, zero, inside, exactly +1, above +1, inside
ADAM_LADDER = np.array([-3.0, -2.0, -0.7, 0.0, 0.9, 2.0, 5.0, 1.3])


def adam_case(n):
    """Every second group of eight gradients walks ADAM_LADDER, the others are N(0, 2^2) as in test_adam_clip; v = 0 on every third
    element, so that on the ladder's zero rung (g = 0, v = 0) the denominator is eps alone."""
    rng = np.random.default_rng(12 + n % 1000)
    i = np.arange(n)
    w, m, v = r32(rng.standard_normal(n)), r32(rng.standard_normal(n) * 0.1), r32(rng.random(n) * 0.01)
    v[i % 3 == 0] = 0.0
    g = rng.standard_normal(n) * 2
    lad = (i // 8) % 2 == 0
    g[lad] = ADAM_LADDER[i[lad] % 8]
    g = r32(g)
    gs = r32(g * ADAM_GSCALE)            # the product the kernel forms (exact: gscale is a power of two)
    rw, rm, rv = tn.adam_update(w, m, v, gs, ADAM_STEP, ADAM_LR0, ADAM_B1, ADAM_B2, eps=ADAM_EPS)
    alpha = tn.exp_decay_lr(ADAM_LR0, ADAM_STEP) * np.sqrt(1 - ADAM_B2 ** (ADAM_STEP + 1)) / (1 - ADAM_B1 ** (ADAM_STEP + 1))
    return SimpleNamespace(n=n, w=w, m=m, v=v, g=g, gs=gs, rw=rw, rm=rm, rv=rv, alpha=float(alpha), clipped=np.abs(gs) > 1.0,
                           edge=np.abs(gs) == 1.0, eps_only=(gs == 0.0) & (v == 0.0))


def adam_w_abs_bound(rw):
    """max-abs bound on w over the clipped elements.  There |clip(g)| = 1, so v' >= (1 - beta2) = 0.01 and the step is at most
    alpha * (|m| + 1) / 0.1 < 1e-4: its few float roundings (2^-24 relative each) are below 1e-10, and what is left is the one rounding
    of w - step to float, 2^-24 |w|.  2^-23 max(1, |w|) leaves a factor of two."""
    return 2.0 ** -23 * np.maximum(1.0, np.abs(rw))


# ---------------------------------------------------------------------------------------------------------------------------------------
# colour conversion and input assembly on pixel counts that are no multiple of a wave or a block

COLOUR_SHAPES = ((1, 15, 15), (3, 7, 9))          # (B, h, w): 5 B h w = 1125 = 37 mod 64 = 101 mod 256; 945 = 49 mod 64 = 177 mod 256
GEN_MASKS = (0, 31, 0b01001)
F32_TOL = 1e-5        # TOL of test_ops_gpu.py (test_colour_and_inputs)
BF16_TOL = 4e-3       # TOL of test_bf16_gpu.py: bf16-stored results
BF16_READ_TOL = 1e-6  # test_input_assembly_bf16: fp32 sums of a few bf16 numbers


def colour_case(B, h, w):
    rng = np.random.default_rng(1100 + 100 * B + h)
    c = SimpleNamespace(B=B, h=h, w=w, npix=h * w)
    c.ys = [r32(rng.standard_normal((B, h, w, 3))) for _ in range(5)]
    c.gen_y = r32(rng.standard_normal((B, h, w, 1)))
    c.ych = r32(rng.standard_normal((5 * B, h, w, 1)))
    c.cbcr = r32(rng.standard_normal((B, h, w, 2)))
    c.noise = r32(rng.standard_normal((5 * B, h, w, 3)) * 0.1)
    return c


def avg_cbcr_ref(ys):
    return sum(y[..., 1:] for y in ys) / 5.0


def yuv2rgb_ref(ych, cbcr):
    """ych [nimg, h, w, 1] with nimg = K * B, image k * B + b takes the chroma of sample b"""
    yuv = np.concatenate([ych, np.tile(cbcr, (ych.shape[0] // cbcr.shape[0], 1, 1, 1))], -1)
    return st.yuv_to_rgb(t64(yuv)).numpy()


def gen_input_ref(ys, gen_y, mask, mode, ld):
    """SHM.py's generator input: five Y planes (a flagged one zeroed, or replaced by gen_y in the cyclic pass, the target's own zeroed),
    the one-hot target plane, zeros up to the pitch"""
    B = ys[0].shape[0]
    fl = [(mask >> j) & 1 for j in range(5)]
    if mode == 0:
        ref = np.zeros(ys[0].shape[:3] + (ld,))
        for j in range(5):
            if not fl[j]:
                ref[..., j] = ys[j][..., 0]
        ref[..., 9] = 1.0
        return ref
    ref = np.zeros((5,) + ys[0].shape[:3] + (ld,))
    for k in range(5):
        for j in range(5):
            if j != k:
                ref[k, ..., j] = gen_y[..., 0] if fl[j] else ys[j][..., 0]
        ref[k, ..., 5 + k] = 1.0
    return ref.reshape((5 * B,) + ys[0].shape[1:3] + (ld,))


def cyc_input_bwd_ref(dcyc, mask, B):
    d5 = dcyc.reshape((5, B) + dcyc.shape[1:])
    out = np.zeros(d5.shape[1:4])
    for k in range(5):
        for j in range(5):
            if j != k and (mask >> j) & 1:
                out = out + d5[k, ..., j]
    return out


# ---------------------------------------------------------------------------------------------------------------------------------------
# rgb -> yuv + per-image standardisation (statistics grid capped at 32 blocks, scale grid at 512 blocks of 256 pixels per sample)

STD_FLOOR = 1.0 / 256.0
STD_RAMP_NPIX = 131072 + 37          # 512 * 256 + 37: both grid-stride loops iterate and end ragged
STD_MID_GREY_SCALE = 0.5 * np.sqrt(2.0) / 3.0


def std_ref(rgb):
    y, s = st.per_image_standardization(st.rgb_to_yuv(t64(rgb)))
    return y.numpy(), s.numpy()


def std_floor_batch():
    """[4, 15, 15, 3]: black, constant mid-grey, random, constant dark grey (1/256).  A constant grey g has YUV (g, 0, 0), whose
    standard deviation over the three planes is g sqrt(2) / 3: black and the dark grey sit on the floor, mid-grey (0.2357) does not."""
    rng = np.random.default_rng(33)
    x = np.zeros((4, 15, 15, 3))
    x[1] = 0.5
    x[2] = rng.random((15, 15, 3))
    x[3] = 1.0 / 256.0
    return r32(x)


def std_ramp():
    """one sample of STD_RAMP_NPIX pixels: a smooth ramp over the whole image, a different slope per channel, plus noise"""
    rng = np.random.default_rng(34)
    t = np.arange(STD_RAMP_NPIX)[:, None] / STD_RAMP_NPIX
    x = t * np.array([0.8, 0.5, 0.3]) + np.array([0.05, 0.2, 0.4]) + rng.random((STD_RAMP_NPIX, 3)) * 0.1
    return r32(x.reshape(1, STD_RAMP_NPIX, 1, 3))


# ---------------------------------------------------------------------------------------------------------------------------------------
# image losses

STYLE_FACTOR = 3.0e-3          # large enough that the style term is visible in the gradient (test_image_losses)


def image_inputs_random(B, S, seed=21):
    """the inputs of test_image_losses, drawn in its order: five originals in [0, 1), their standardised YUV, the mean chroma, Y planes"""
    rng = np.random.default_rng(seed)
    orig = [rng.random((B, S, S, 3)) for _ in range(5)]
    ds = [st.per_image_standardization(st.rgb_to_yuv(t64(o)))[0] for o in orig]
    cbcr = sum(d[..., 1:] for d in ds) / 5.0
    gen_y = rng.standard_normal((B, S, S, 1)) * 0.5 + 1.0
    cyc_y = rng.standard_normal((5 * B, S, S, 1)) * 0.5 + 1.0
    return SimpleNamespace(B=B, S=S, orig=orig, ds=ds, cbcr=cbcr, gen_y=gen_y, cyc_y=cyc_y)


def image_oracle(inp, flags, sf=STYLE_FACTOR, dtype=torch.float64, ssim_term=True, rescale=st.rescale_01):
    """The generator's image-space loss of the float64 oracle and its gradient wrt the generated Y planes, composed as SHM.py:744-826
    composes it (this is the construction of test_image_losses).  ssim_term = False leaves the SSIM loss out: the L1, content and style
    parts alone; rescale: the rescale_01 applied to the cyclic views (rescale_01_fixed_range for the teeth of the extreme-element check)."""
    B = inp.B
    cast = lambda a: (a if isinstance(a, torch.Tensor) else t64(a)).to(dtype)
    orig, ds, cbcr = [cast(o) for o in inp.orig], [cast(d) for d in inp.ds], cast(inp.cbcr)
    gen_y = cast(inp.gen_y).requires_grad_(True)
    cyc_y = cast(inp.cyc_y).requires_grad_(True)
    gen_rgb = st.yuv_to_rgb(torch.cat([gen_y, cbcr], 3))
    cyuv = [torch.cat([cyc_y[k * B:(k + 1) * B], cbcr], 3) for k in range(5)]
    crgb = [st.yuv_to_rgb(c) for c in cyuv]
    l1 = lambda a, b: (a - b).abs().mean(dim=(1, 2, 3))
    l1g = l1(gen_rgb, orig[4])
    l1c = [l1(crgb[k], orig[k]) for k in range(5)]
    L1 = (sum(l1c[k] for k in range(4)) + l1g) / 5 + 10 * l1c[4]
    ssims = [st.ssim(rescale(cyuv[k]), st.rescale_01(ds[k])) for k in range(5)]
    sl = [torch.zeros(B, dtype=dtype) if flags[k] else -torch.log((1 + ssims[k]) / 2) for k in range(5)]
    ssim_loss = (sl[0] + sl[1] + sl[2] + sl[3] + 10 * sl[4]) / 5
    content = ((cyuv[4] - ds[0]) ** 2).mean(dim=(1, 2, 3))
    style = sf * ((st.gram_matrix(cyuv[4]) - st.gram_matrix(ds[4])) ** 2).mean(dim=(1, 2))
    tot = (10 * L1 + (10 * ssim_loss if ssim_term else 0.0) + 10 * (100 * style + content)).mean()
    rg, rc = torch.autograd.grad(tot, [gen_y, cyc_y])
    det = lambda t: t.detach()
    return SimpleNamespace(B=B, l1g=det(l1g), l1c=[det(t) for t in l1c], ssims=[det(t) for t in ssims], sl=[det(t) for t in sl],
                           content=det(content), style=det(style), rg=rg, rc=rc, gen_rgb=det(gen_rgb), crgb=[det(t) for t in crgb],
                           cyc_y=det(cyc_y))


def rescale_01_fixed_range(x):
    """rescale_01 with its minimum and maximum held constant: the same values, no gradient through amin / amax"""
    mn = x.amin(dim=(1, 2, 3), keepdim=True).detach()
    mx = x.amax(dim=(1, 2, 3), keepdim=True).detach()
    den = mx - mn
    safe = torch.where(den == 0, torch.ones_like(den), den)
    return torch.where(den == 0, torch.zeros_like(x), (x - mn) / safe)


def loss_slots(o):
    """the 18 raw loss slots of shm_image_losses (sums over the batch)"""
    return np.array([float(o.l1g.sum())] + [float(t.sum()) for t in o.l1c] + [float(t.sum()) for t in o.ssims]
                    + [float(t.sum()) for t in o.sl] + [float(o.content.sum()), float(o.style.sum())])


def loss_slot_bounds(o):
    """the tolerances of test_image_losses, slot by slot"""
    B = o.B
    return np.array([1e-5 * B] * 6 + [2e-5 * B] * 10 + [1e-5 * B * max(1.0, float(o.content.max())), 1e-5 * max(1.0, float(o.style.sum()))])


GRAD_TOL = 1e-4          # rel-L2 of dgen_y and of dcyc_y (test_image_losses)


def _rounded(inp):
    """the same inputs as float32 values (ds is taken as given, not recomputed)"""
    inp.orig = [r32(o) for o in inp.orig]
    inp.ds = [t64(r32(d.numpy() if isinstance(d, torch.Tensor) else d)) for d in inp.ds]
    inp.cbcr = t64(r32(inp.cbcr.numpy() if isinstance(inp.cbcr, torch.Tensor) else inp.cbcr))
    inp.gen_y, inp.cyc_y = r32(inp.gen_y), r32(inp.cyc_y)
    return inp


ALL, NONE = (True,) * 5, (False,) * 5


def image_case(name):
    """Named cases of the image-loss tests -> (inputs, flags).  HO = S - 10 SSIM outputs per side: S = 11 one pixel, 16 six, 26 exactly
    one 16 x 16 forward tile, 27 a second tile of one pixel."""
    rng = np.random.default_rng(210)
    if name.startswith("size"):                           # size<S>_b<B>_<flags>
        s_, b_, f_ = name.split("_")
        S, B = int(s_[4:]), int(b_[1:])
        flags = {"none": NONE, "all": ALL, "mixed": (True, False, False, True, False)}[f_]
        return _rounded(image_inputs_random(B, S, seed=2100 + S + B)), flags
    if name == "chroma_extremes":                         # narrow Y, wide chroma: every view's minimum and maximum lie in the chroma planes
        inp = image_inputs_random(2, 27, seed=2201)
        inp.cbcr = t64(rng.uniform(-3.0, 3.0, (2, 27, 27, 2)))
        inp.cyc_y = 1.0 + 0.1 * rng.uniform(-1.0, 1.0, (10, 27, 27, 1))
        return _rounded(inp), (False, True, False, False, False)
    if name == "y_extremes":                              # wide Y, narrow chroma: both lie in the Y plane
        inp = image_inputs_random(2, 27, seed=2202)
        inp.cbcr = t64(0.1 * rng.uniform(-1.0, 1.0, (2, 27, 27, 2)))
        inp.cyc_y = 2.0 * rng.standard_normal((10, 27, 27, 1))
        return _rounded(inp), (False, True, False, False, False)
    if name == "black_view":                              # a black original: its standardised YUV is zero and rescale_01's range is zero
        inp = image_inputs_random(1, 27, seed=2203)
        inp.orig[BLACK_K] = np.zeros_like(inp.orig[BLACK_K])
        inp.ds[BLACK_K] = st.per_image_standardization(st.rgb_to_yuv(t64(inp.orig[BLACK_K])))[0]
        inp.cbcr = sum(d[..., 1:] for d in inp.ds) / 5.0
        return _rounded(inp), NONE
    if name.startswith("flat_cyc"):                       # flat_cyc<k>: view k of the cyclic output and the chroma are one constant
        k = int(name[-1])
        inp = image_inputs_random(1, 27, seed=2204 + k)
        inp.cbcr = t64(np.full((1, 27, 27, 2), FLAT_C))
        inp.cyc_y[k] = FLAT_C
        return _rounded(inp), NONE
    raise KeyError(name)


BLACK_K = 2
FLAT_C = 0.25
SIZE_CASES = ("size11_b1_none", "size16_b1_none", "size26_b1_none", "size27_b1_none", "size27_b3_mixed", "size27_b1_all")
EDGE_CASES = ("chroma_extremes", "y_extremes", "black_view", "flat_cyc1", "flat_cyc4")
IMAGE_CASES = SIZE_CASES + EDGE_CASES


def placement(inp):
    """Where rescale_01 finds the extremes of every cyclic view: {(b, k): (kind, pmin, pmax, unique)} with kind "chroma" (both in the
    chroma planes, strictly beyond every Y value), "y" (both in the Y plane, strictly beyond every chroma value), "flat" (the view is one
    constant) or "mixed"; pmin / pmax the flat pixel index of the Y extremes; unique: each Y extreme is attained once."""
    B = inp.B
    out = {}
    cb = inp.cbcr.numpy() if isinstance(inp.cbcr, torch.Tensor) else inp.cbcr
    for k in range(5):
        for b in range(B):
            y = np.asarray(inp.cyc_y)[k * B + b].ravel()
            c = cb[b].ravel()
            if y.min() == y.max() == c.min() == c.max():
                kind = "flat"
            elif c.min() < y.min() and c.max() > y.max():
                kind = "chroma"
            elif y.min() < c.min() and y.max() > c.max():
                kind = "y"
            else:
                kind = "mixed"
            out[(b, k)] = (kind, int(y.argmin()), int(y.argmax()), bool((y == y.min()).sum() == 1 and (y == y.max()).sum() == 1))
    return out


def extreme_elements(inp, rc):
    """For every view whose two extremes lie in the Y plane: ((b, k), pmin, pmax, bound).  The two elements of dcyc_y at pmin / pmax carry
    rescale_01's min / max sub-gradient (ssim_minmax_kernel) on top of their own.  bound: GRAD_TOL times the L2 norm of that view's
    reference gradient -- the relative tolerance of the whole tensor applied to one view: no single element may be further off than the
    rel-L2 check lets the view be as a whole."""
    B = inp.B
    rc = np.asarray(rc).reshape(5 * B, -1)
    return [((b, k), pmin, pmax, GRAD_TOL * float(np.linalg.norm(rc[k * B + b])))
            for (b, k), (kind, pmin, pmax, _) in sorted(placement(inp).items()) if kind == "y"]


def image_errors(L, dg, dc, o, inp):
    """The figures every image-loss check is made of: |slot error| (18), rel-L2 of dgen_y and dcyc_y, and per Y-extreme view the larger
    absolute error of its two extreme elements.  L, dg, dc: the result under test (float64 numpy); o: the float64 oracle."""
    B = inp.B
    d2, r2 = np.asarray(dc).reshape(5 * B, -1), o.rc.numpy().reshape(5 * B, -1)
    ext = [max(abs(d2[k * B + b, pmin] - r2[k * B + b, pmin]), abs(d2[k * B + b, pmax] - r2[k * B + b, pmax]))
           for (b, k), pmin, pmax, _ in extreme_elements(inp, r2)]
    return SimpleNamespace(slots=np.abs(np.asarray(L)[:18] - loss_slots(o)), dg=rel_l2(dg, o.rg.numpy()), dc=rel_l2(dc, o.rc.numpy()),
                           ext=np.array(ext))


def f32_oracle_errors(name):
    """error of the SAME oracle run in float32 on the CPU against float64: the noise floor of the case"""
    inp, flags = image_case(name)
    o = image_oracle(inp, flags)
    f = image_oracle(inp, flags, dtype=torch.float32)
    return image_errors(loss_slots(f), f.rg.double().numpy(), f.rc.double().numpy(), o, inp)


# ---------------------------------------------------------------------------------------------------------------------------------------
# discriminator-head losses

DHEAD_NPATCH = (1, 63, 64, 65, 200)
DHEAD_TOL = 1e-5


def dhead_case(B, npatch, scale=1.0, seed=20):
    rng = np.random.default_rng(seed + 7 * npatch + B)
    return r32(rng.standard_normal((12 * B, npatch))), r32(rng.standard_normal((12 * B, 5)) * scale)


def dhead_oracle(rf, cls, B, T, mode):
    """The discriminator and generator head losses of SHM.py:683-722 on the D batch [D1][D3 x5][D2][D4 x5] (the composition of
    test_dhead_losses).  Returns the gradients of the D total wrt (rf, cls), of the G total wrt rf, and the nine raw loss slots."""
    rft, clst = t64(rf).requires_grad_(True), t64(cls).requires_grad_(True)
    sl = lambda g, k=0: slice((g + k) * B, (g + k + 1) * B)       # group start in units of B
    mse = lambda a, t: ((a - t) ** 2).mean(dim=1)

    def xent(lg, k, w=1.0):
        lab = torch.zeros_like(lg)
        lab[:, k] = w
        return st.softmax_xent(lg, lab, mode)
    D1, D2 = sl(0), sl(6)
    D3 = [sl(1, k) for k in range(5)]
    D4 = [sl(7, k) for k in range(5)]
    D1_RF, D3_RF = mse(rft[D1], T), sum(mse(rft[s], T) for s in D3)
    D2_RF = mse(rft[D2], T) + (rft[D1] ** 2).mean(dim=1)
    D4_RF = sum(mse(rft[D4[k]], T) + (rft[D3[k]] ** 2).mean(dim=1) for k in range(5)) + D2_RF
    D1_c, D3_c = xent(clst[D1], 4, T), sum(xent(clst[D3[k]], k) for k in range(5))
    D4_c = sum(xent(clst[D4[k]], k) for k in range(5))
    tot_d = ((D1_c + D3_c) / 6 + (D2_RF + D4_RF) / 6 + 0.5 * D4_c + 10 * D4_c).mean()
    tot_g = ((D1_RF + D3_RF) / 6).mean()
    gd_rf, gd_cls = torch.autograd.grad(tot_d, [rft, clst], retain_graph=True)
    gg_rf, = torch.autograd.grad(tot_g, [rft])
    ref = [D1_RF.sum(), D3_RF.sum(), (rft[D1] ** 2).mean(dim=1).sum(),
           sum((rft[s] ** 2).mean(dim=1) for s in D3).sum(), mse(rft[D2], T).sum(),
           sum(mse(rft[s], T) for s in D4).sum(), D1_c.sum(), D3_c.sum(), D4_c.sum()]
    return SimpleNamespace(gd_rf=gd_rf.numpy(), gd_cls=gd_cls.numpy(), gg_rf=gg_rf.numpy()[:6 * B], slots=[float(r.detach()) for r in ref])
