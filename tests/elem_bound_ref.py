"""Per-element error bounds for the convolution, weight-gradient and InstanceNorm kernels (float64, CPU only).

Every parity test of these kernels ends in a whole-tensor rel-L2 against the float64 oracle.  That sees a precision loss that is spread
evenly; it does not see one wrong border pixel, the last column of a ragged N tile or the last pixel slot of a ragged chunk, whose energy
drowns in the norm (test_elem_bound_cpu.py shows both verdicts on modelled faults).  This module states, per output element, how far a
CORRECT kernel can be from the float64 result of the same operands -- whatever order it sums in -- and `within` holds a result to it.

Notation: u32 = 2^-24 and u16 = 2^-8, the round-to-nearest units of fp32 and bf16; gamma(n) = n u32 / (1 - n u32) (Higham, Accuracy
and Stability of Numerical Algorithms, 3.1: n correctly rounded fp32 operations in sequence move a value by at most gamma(n) relative).
Operands are taken as the device holds them (fp32, or bf16-rounded: test_variants_gpu._rnd); the reference is float64 on exactly those.

  dot products   A sum of K products evaluated in fp32 in ANY order (any tree of additions, fused or not, split over blocks and reduced):
                 every product passes through one rounding of its own and at most K - 1 additions, so |s' - s| <= gamma(K) sum|x||w|.
                 M = that sum of absolute products comes from the SAME oracle call on the absolute operands.
  conv forward   K = k^2 cin; + 1 for the bias addition, + 1 for the LeakyReLU product (the bias is handed over in fp32: its own rounding
                 is one more on |b| alone, a term that has passed only those two): E = gamma(K + 2) (M + |b|).  The store rounds once:
                 tol = E + u_out (|ref| + E) + K 2^-126 (flush-to-zero of K products).  A pre-activation that rounds across the kink
                 of a LeakyReLU with slope in [0, 1] moves the output by no more than it moved itself, so E covers it.
  dgrad / Conv2DTranspose   the same with M from the transposed product; K = k^2 cout (input gradient), k^2 cin (transposed forward).
  wgrad          K = batch ho wo, M = the autograd weight gradient of the absolute operands, fp32 output in every mode: gamma(K) M.
                 Split-K slabs are the same K-term sum in another order: a slab is an fp32 partial sum, stored and re-read exactly, and
                 the reduce over nsplit slabs is nsplit - 1 of the K - 1 additions.  (The form gamma(K + nsplit) allows for one more
                 rounding per slab; no kernel here has one, the tests do not know the slab count -- "wgrad.blocks" is a target that
                 the launchers divide by the tiles, and the thin and eight-wave kernels write two slabs per block -- and gamma(K) is
                 the smaller bound for every nsplit.)  accumulate = 1: one more addition, u32 (|dw_before| + |ref|).
  InstanceNorm   see in_apply_ref_tol, in_pool_ref_tol, in_bwd_ref_tol, in_sum_tol: the count of roundings stands beside each expression.

No constant in this module is fitted to a kernel's output.
"""
import numpy as np
import torch

from oracle import step_torch as st

U32 = 2.0 ** -24
U16 = 2.0 ** -8
TINY = 2.0 ** -126          # smallest normal fp32: what flush-to-zero can take from one operation


def gamma(n):
    n = np.asarray(n, np.float64)
    return n * U32 / (1.0 - n * U32)


def u_out(dt):
    """round-to-nearest unit of an output of type dt ("bf16" / torch.bfloat16: u16; anything else is fp32)."""
    return U16 if dt in ("bf16", torch.bfloat16) else U32


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, np.float64)))


def _nchw(a):
    return _t(a).permute(0, 3, 1, 2)


def _nhwc(t):
    return t.detach().permute(0, 2, 3, 1).contiguous().numpy()


# ---------------------------------------------------------------------------------------------------------------------
# magnitudes: the oracle's own product on the absolute operands
def fwd_mag(x, w_hwio, stride, b=None):
    m = _nhwc(st.conv2d_same(_nchw(np.abs(x)), _t(np.abs(w_hwio)), stride))
    return m if b is None else m + np.abs(np.asarray(b, np.float64))


def dgrad_mag(dy, w_hwio, stride, hw):
    """sum |dy| |w| of the input gradient of conv2d_same(x [n, h, w, cin], w) for dy [n, ho, wo, cout]; hw = (h, w)."""
    n, cin = dy.shape[0], w_hwio.shape[2]
    xt = torch.zeros(n, cin, hw[0], hw[1], dtype=torch.float64, requires_grad=True)
    m, = torch.autograd.grad(st.conv2d_same(xt, _t(np.abs(w_hwio)), stride), xt, _nchw(np.abs(dy)))
    return _nhwc(m)


def transpose_mag(x, w_hwoi, b=None):
    m = _nhwc(st.conv2d_transpose_same(_nchw(np.abs(x)), _t(np.abs(w_hwoi))))
    return m if b is None else m + np.abs(np.asarray(b, np.float64))


def wgrad_mag(x, dy, stride, k=3):
    cin, cout = x.shape[-1], dy.shape[-1]
    wt = torch.zeros(k, k, cin, cout, dtype=torch.float64, requires_grad=True)
    m, = torch.autograd.grad(st.conv2d_same(_nchw(np.abs(x)), wt, stride), wt, _nchw(np.abs(dy)))
    return m.numpy()


# ... and the float64 results themselves, for a driver whose own reference is taken on operands BEFORE the device's rounding
def f32(a):
    """an operand as an fp32 device tensor holds it (float64)"""
    return np.asarray(a, np.float32).astype(np.float64)


def _act(z, slope):
    return np.where(z > 0, z, slope * z)


def fwd_ref(x, w_hwio, b, stride, slope=1.0):
    z = _nhwc(st.conv2d_same(_nchw(x), _t(w_hwio), stride))
    return _act(z if b is None else z + np.asarray(b, np.float64), slope)


def dgrad_ref(dy, w_hwio, stride, hw):
    xt = torch.zeros(dy.shape[0], w_hwio.shape[2], hw[0], hw[1], dtype=torch.float64, requires_grad=True)
    r, = torch.autograd.grad(st.conv2d_same(xt, _t(w_hwio), stride), xt, _nchw(dy))
    return _nhwc(r)


def transpose_ref(x, w_hwoi, b, slope=1.0):
    z = _nhwc(st.conv2d_transpose_same(_nchw(x), _t(w_hwoi)))
    return _act(z if b is None else z + np.asarray(b, np.float64), slope)


def wgrad_ref(x, dy, stride, k=3):
    wt = torch.zeros(k, k, x.shape[-1], dy.shape[-1], dtype=torch.float64, requires_grad=True)
    r, = torch.autograd.grad(st.conv2d_same(_nchw(x), wt, stride), wt, _nchw(dy))
    return r.numpy()


# ---------------------------------------------------------------------------------------------------------------------
# bounds
def conv_tol(mag, kdim, ref, dt):
    """forward, input gradient, transposed forward: mag = M (+ |b|), kdim = K, ref = the float64 result (after the activation)."""
    e = gamma(kdim + 2) * mag                # K: products and their additions; + 1 bias addition; + 1 LeakyReLU product
    return e + u_out(dt) * (np.abs(ref) + e) + kdim * TINY


def fwd_tol(x, w_hwio, b, stride, ref, dt):
    k, _, cin, _ = w_hwio.shape
    return conv_tol(fwd_mag(x, w_hwio, stride, b), k * k * cin, ref, dt)


def dgrad_tol(dy, w_hwio, stride, ref, dt):
    k, _, _, cout = w_hwio.shape
    return conv_tol(dgrad_mag(dy, w_hwio, stride, ref.shape[1:3]), k * k * cout, ref, dt)


def transpose_tol(x, w_hwoi, b, ref, dt):
    k, _, _, cin = w_hwoi.shape
    return conv_tol(transpose_mag(x, w_hwoi, b), k * k * cin, ref, dt)


def wgrad_tol(x, dy, stride, ref, k=3, before=None):
    """ref: the float64 gradient WITHOUT `before`; before: what the destination held when accumulate = 1 (the result is before + ref)."""
    kdim = dy.shape[0] * dy.shape[1] * dy.shape[2]
    e = gamma(kdim) * wgrad_mag(x, dy, stride, k)          # K products (1 rounding each) and K - 1 additions, in any order and split
    tol = e + U32 * (np.abs(ref) + e) + kdim * TINY
    if before is not None:
        tol = tol + U32 * (np.abs(before) + np.abs(ref) + e)                         # the accumulating addition
    return tol


# ---- InstanceNorm: mean_f and inv_f are the device's own statistics as its kernels read them, (float)stats[...]
def _stats_f(stats, n, c):
    s = np.asarray(stats, np.float64).reshape(n, c, 2).astype(np.float32).astype(np.float64)
    return s[:, :, 0].reshape(n, 1, 1, c), s[:, :, 1].reshape(n, 1, 1, c)


def in_apply_ref_tol(a, stats, beta, dt):
    """y = fma(a - mean_f, inv_f, beta).  Returns (float64 value of that expression, bound)."""
    n, c = a.shape[0], a.shape[-1]
    mean, inv = _stats_f(stats, n, c)
    beta = np.asarray(beta, np.float32).astype(np.float64)
    t = (a - mean) * inv
    ref = t + beta
    # roundings: the subtraction a - mean_f (1, on the product term), the fma (1, on the whole result <= |t| + |beta|)
    e = 2 * U32 * np.abs(t) + U32 * np.abs(beta) + 2 * TINY
    return ref, e + u_out(dt) * (np.abs(ref) + e)


def in_pool_ref_tol(y_stored, dt):
    """pooled = 0.25 * (((y0 + y1) + y2) + y3) on the four STORED values of a 2 x 2 quad (y_stored: the device's own output)."""
    n, h, w, c = y_stored.shape
    q = y_stored.reshape(n, h // 2, 2, w // 2, 2, c)
    ref = q.mean(axis=(2, 4))
    # roundings: three additions; the product with 0.25 is exact
    e = gamma(3) * 0.25 * np.abs(q).sum(axis=(2, 4)) + TINY
    return ref, e + u_out(dt) * (np.abs(ref) + e)


def in_bwd_partial(kern, c):
    """How many terms a kernel of shm_in_bwd adds in fp32 before its sums go on in float64 (csrc/instnorm_bwd_*.hip): the two passes
    combine U <= 8 pixels per thread in fp32 (their tail loops add straight into doubles); a one-pass block adds its whole slice in fp32
    -- its threads' U pixels, then the PP pixel slots in LDS -- 16384 / CB pixels of a channel where g and a are held, 32768 / CB where
    g is held, CB = min(c, 64); the blocks' rows are added in float64."""
    cb = min(int(c), 64)
    return 32768 // cb if "fusedg" in kern else 16384 // cb if "fused8" in kern else 8


def in_bwd_ref_tol(a, stats, g, g2=None, hdz=None, hw_vec=None, slope=0.2, dt="f32", partial=8, means_error=True):
    """dz = lrelu'(a) inv_f (G - m1 - xh m2), xh = (a - mean_f) inv_f, m1 = mean(G), m2 = mean(G xh) in float64.
    G = g, g + 0.25 g2 (pooled form: g2 on the half-size map) or hdz hw (rank-1 form).  Returns (dz float64, bound).

    The device's m1 and m2 are not the float64 means of exact terms: its terms G and G xh are fp32 values that have been rounded `form`
    and `form` + 3 times, and `partial` of them (in_bwd_partial) are added in fp32 before the float64 accumulation.  The counted roundings
    on inv (|G| + |m1| + |xh m2|) alone cannot hold that: mean|G xh| is not small where m2 = mean(G xh) cancels to nearly nothing.  So the
    two means carry their own terms e_m1, e_m2 below, on mean|G| and mean|G xh|, through the expression.  They depend on `partial`, not
    on the size of the map.  means_error=False leaves them out (the counted roundings alone: test_elem_bound_cpu.py prints both sizes)."""
    # (torch, not NumPy: the same float64 arithmetic on all the host's cores -- the one-pass kernels' maps have up to 2^25 elements)
    n, h, w, c = a.shape
    mean, inv = (_t(v) for v in _stats_f(stats, n, c))
    a = _t(a)
    form = 0
    if hdz is not None:
        G = _t(hdz).reshape(n, h, w, 1) * _t(hw_vec)
        form = 1                                                      # the product hdz * hw
    else:
        G = _t(g)
        if g2 is not None:
            G = G + 0.25 * _t(g2).repeat_interleave(2, 1).repeat_interleave(2, 2)
            form = 1                                                  # fma(0.25, g2, g)
    xh = (a - mean) * inv
    gx = G * xh
    m1 = G.mean((1, 2), keepdim=True)
    m2 = gx.mean((1, 2), keepdim=True)
    s = torch.where(a > 0, 1.0, float(slope)).to(torch.float64)
    ref = s * inv * (G - m1 - xh * m2)
    # the two means: each term rounded `form` (m1) / `form` + 3 (m2: a - mean_f, * inv_f, g * xh) times, at most `partial` - 1 fp32 additions
    # on top of it, float64 from there on (its 2^-53 per addition is below everything here), and the float cast of the quotient (1)
    e_m1 = float(gamma(partial - 1 + form)) * G.abs().mean((1, 2), keepdim=True) + U32 * m1.abs()
    e_m2 = float(gamma(partial - 1 + form + 3)) * gx.abs().mean((1, 2), keepdim=True) + U32 * m2.abs()
    if not means_error:
        e_m1, e_m2 = 0.0, 0.0
    # roundings on G: forming it (`form`), G - m1 (1), - xh m2 (1), * inv (1), * slope (1)
    # on m1: the same chain behind it (4), and its own error e_m1
    # on xh m2: a - mean_f (1), * inv_f (1), xh * m2 (1), the subtraction (1), * inv (1), * slope (1), and |xh| e_m2
    e = s * inv * (float(gamma(4 + form)) * G.abs() + (float(gamma(4)) * m1.abs() + e_m1) + xh.abs() * (float(gamma(6)) * m2.abs() + e_m2)) + 6 * TINY
    return ref.numpy(), (e + u_out(dt) * (ref.abs() + e)).numpy()


def in_sum_tol(dz_ref, dz_tol, axes):
    """channel sums of dz over `axes` ((1, 2): per sample; (0, 1, 2): the bias gradient): what the summands may be off by, and
    gamma(number of summands) * sum|dz| for adding them in fp32 in any order (the device adds most of it in float64)."""
    cnt = int(np.prod([dz_ref.shape[i] for i in axes]))
    return dz_tol.sum(axes) + gamma(cnt) * np.abs(dz_ref).sum(axes)


# ---------------------------------------------------------------------------------------------------------------------
# the check
def _classes(idx, shape, where):
    """the classes of tiled-kernel faults an index falls in.  where: {"kind": "conv" (NHWC output map) / "wgrad" (HWIO) / "in" (NHWC
    activation), "tile": patch edge (16), "ntile": N tile (64), "chunk": pixels per chunk of an elementwise pass}"""
    kind = where.get("kind", "conv")
    out = []
    if kind == "wgrad":
        if len(shape) == 4:
            ky, kx, ci, co = idx
            nt = where.get("ntile", 64)
            out.append(f"tap ({ky}, {kx})")
            if shape[2] % nt and ci >= nt * (shape[2] // nt):
                out.append("input channel in a ragged tile")
            if shape[3] % nt and co >= nt * (shape[3] // nt):
                out.append("output channel in a ragged N tile")
        return out
    if len(shape) != 4:
        return out
    n, i, j, c = idx
    N, H, W, C = shape
    if i in (0, H - 1) or j in (0, W - 1):
        out.append("border ring")
    if kind == "conv":
        t, nt = where.get("tile", 16), where.get("ntile", 64)
        if i >= t * ((H - 1) // t) or j >= t * ((W - 1) // t):
            out.append("ragged patch" if (H % t and i >= t * (H // t)) or (W % t and j >= t * (W // t)) else "last patch")
        if C % nt and c >= nt * (C // nt):
            out.append("channel in a ragged N tile")
    else:
        chunk = int(where.get("chunk") or max(1, 1024 // C))          # default: the pixels one 256-thread block of four-channel threads takes per step
        p = i * W + j
        if (H * W) % chunk and p >= chunk * ((H * W) // chunk):
            out.append("ragged tail of a pixel chunk")
            if p == H * W - 1:
                out.append("last pixel slot")
    if n == 0:
        out.append("first image")
    if n == N - 1:
        out.append("last image")
    return out


class OutOfBound(AssertionError):
    """raised by within(); .index, .classes, .ratio, .count for the tests of the check itself"""


def within(got, ref, tol, where=None, what=""):
    """Hold `got` to |got - ref| <= tol element by element.  Returns the worst ratio |got - ref| / tol.  Non-finite values must be
    non-finite in the same places (NaN where NaN, the same infinity where infinite).  On failure raises OutOfBound with the index of
    the worst element, got, ref and tol there, the classes the index falls in (`where`, see _classes) and how many elements exceed."""
    got = np.asarray(got, np.float64)
    ref = np.asarray(ref, np.float64)
    tol = np.broadcast_to(np.asarray(tol, np.float64), ref.shape)
    where = where or {}
    assert got.shape == ref.shape, (got.shape, ref.shape)
    with np.errstate(invalid="ignore"):
        err = np.abs(got - ref)
    if not np.isfinite(err).all():               # (the rare path: some value is non-finite on either side)
        fin = np.isfinite(ref)
        same = np.where(fin, np.isfinite(got), (np.isnan(ref) & np.isnan(got)) | (got == ref))
        if not same.all():
            idx = tuple(int(v) for v in np.argwhere(~same)[0])
            e = OutOfBound(f"{what}: non-finite mismatch at {idx}: got {got[idx]!r}, ref {ref[idx]!r}; {int((~same).sum())} such elements; "
                           f"classes: {_classes(idx, ref.shape, where)}")
            e.index, e.classes, e.ratio, e.count = idx, _classes(idx, ref.shape, where), float("inf"), int((~same).sum())
            raise e
        err = np.where(fin, err, 0.0)            # equal non-finite values: no error
    assert np.isfinite(tol).all() and (tol >= 0.0).all(), f"{what}: a bound that is not a finite, non-negative number holds nothing"
    with np.errstate(divide="ignore"):
        ratio = np.divide(err, tol, out=np.zeros_like(err), where=err > 0.0)          # an exact element has ratio 0 whatever its bound
    worst = float(ratio.max()) if ratio.size else 0.0
    if worst > 1.0:
        idx = tuple(int(v) for v in np.unravel_index(int(ratio.argmax()), ratio.shape))
        cls = _classes(idx, ref.shape, where)
        cnt = int((ratio > 1.0).sum())
        e = OutOfBound(f"{what}: element {idx} is {worst:.3g} x its bound: got {got[idx]!r}, ref {ref[idx]!r}, tol {tol[idx]:.3e}; "
                       f"{cnt} of {ratio.size} elements exceed; classes: {cls}")
        e.index, e.classes, e.ratio, e.count = idx, cls, worst, cnt
        raise e
    return worst


# ---------------------------------------------------------------------------------------------------------------------
# what the GPU drivers call: bound + within + note in one line.  `got` is the device's result as float64, the operands float64 as the
# device holds them, `ref` the float64 result the driver already has.  dt: the OUTPUT's type ("bf16" / "f32").
CONV = {"kind": "conv"}
WGRAD = {"kind": "wgrad"}


def hold_fwd(got, x, w_hwio, b, stride, ref, dt, family):
    return note(family, dt, within(got, ref, fwd_tol(x, w_hwio, b, stride, ref, dt), CONV, family))


def hold_dgrad(parts, dy, w_hwio, stride, ref, dt, family):
    """parts: the destination, or the halves of a split one in channel order (each is checked against its slice of ref)."""
    tol = dgrad_tol(dy, w_hwio, stride, ref, dt)
    parts = parts if isinstance(parts, (list, tuple)) else [parts]
    c0, worst = 0, 0.0
    for p in parts:
        c1 = c0 + p.shape[-1]
        worst = max(worst, within(p, ref[..., c0:c1], tol[..., c0:c1], CONV, f"{family} [channels {c0}:{c1}]"))
        c0 = c1
    assert c0 == ref.shape[-1]
    return note(family, dt, worst)


def hold_transpose(got, x, w_hwoi, b, ref, dt, family):
    return note(family, dt, within(got, ref, transpose_tol(x, w_hwoi, b, ref, dt), CONV, family))


def hold_wgrad(got, x, dy, stride, ref, family, dt="f32", k=3, before=None):
    """dt: the OPERANDS' type, for the record only (the gradient is fp32 in every mode).  before: accumulate = 1 on top of it (got is held
    to before + ref)."""
    tol = wgrad_tol(x, dy, stride, ref, k, before)
    return note(family, dt, within(got, ref if before is None else before + ref, tol, WGRAD, family))


def hold_in_bwd(results, a, stats, g, g2=None, hdz=None, hw_vec=None, slope=0.2, dt="f32", where=None, elems=2 ** 22):
    """shm_in_bwd's outputs against in_bwd_ref_tol, in channel slices of about `elems` elements: statistics and means are per (sample,
    channel), so a slice is a whole problem, and a map of any size is held with the memory of one slice.  Tensors may be torch tensors on
    any device.  results: (dz, dbias or None, per-sample dz sums or None, shm_last_kernel()) of every call on these operands."""
    def h64(t, sl=None):
        if t is None:
            return None
        t = t if sl is None else t[..., sl]
        return t.double().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t, np.float64)

    n, h, w, c = a.shape
    step = max(1, min(c, elems // (n * h * w)))
    st3 = h64(stats).reshape(n, c, 2)
    worst = {r[3]: 0.0 for r in results}
    for c0 in range(0, c, step):
        sl = slice(c0, min(c, c0 + step))
        operands = (h64(a, sl), st3[:, sl], h64(g, sl), h64(g2, sl), h64(hdz), h64(hw_vec, sl))
        bounds = {}                                   # one reference and bound per fp32 partial length among the results' kernels
        for dz, db, keep, kern in results:
            part = in_bwd_partial(kern, c)
            if part not in bounds:
                bounds[part] = in_bwd_ref_tol(*operands, slope, dt, part)
            zr, ztol = bounds[part]
            worst[kern] = max(worst[kern], within(h64(dz, sl), zr, ztol, where or {"kind": "in"}, f"{kern} [channels {sl.start}:{sl.stop}]"))
            if db is not None:
                within(h64(db, sl), zr.sum((0, 1, 2)), in_sum_tol(zr, ztol, (0, 1, 2)), None, kern + " bias gradient")
            if keep is not None:
                within(h64(keep, sl), zr.sum((1, 2)), in_sum_tol(zr, ztol, (1, 2)), None, kern + " dz sums")
    return worst


def note(family, dt, ratio):
    """For the record (DESIGN.md's table of worst ratios per kernel family); nothing asserts on it.  With ELEM_BOUND_LOG=<file> in the
    environment every checked result appends one line `family dtype ratio` there; pytest -s shows the same line."""
    import os
    line = f"elem-bound {family} {dt} {ratio:.4g}"
    print(line)
    path = os.environ.get("ELEM_BOUND_LOG")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")
    return ratio
