"""TEST INFRASTRUCTURE ONLY -- the reference of SpecSeg training: a PyTorch-CPU restatement (float64 by default, float32 to measure what
float32 costs) of the training forward of shmgan_amd.specseg.SpecSeg with autograd, the loss of shm_seg_loss from logits, the
BatchNormalization moving-average rule, a hand-written first-maximum pool backward, an Adam step, and the case tables of
test_specseg_train_gpu.py (test_specseg_train_cpu.py shows that each case is in the branch it claims).

Dropout keep masks are inputs: the device test reads the device's masks back and passes them in.
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

from oracle.specseg_torch import BN_EPS, WIDTHS, specseg_spec
from oracle.step_torch import conv2d_same

BN_MOMENTUM = 0.99
DROP_RATES = (0.1, 0.1, 0.2, 0.2, 0.3, 0.2, 0.2, 0.1, 0.1)
SMOOTH = 1e-5
ALPHA = 0.25
TRAINABLE = [k not in ("bn_mean", "bn_var") for k, _ in specseg_spec()]


# ------------------------------------------------------------------------------------------------------------------ loss
def seg_loss(z, g):
    """Dice + binary focal loss from logits (any float dtype); log p = -softplus(-z), log(1-p) = -softplus(z)."""
    z, g = z.reshape(-1), g.reshape(-1)
    p, q = torch.sigmoid(z), torch.sigmoid(-z)
    lp, lq = -F.softplus(-z), -F.softplus(z)
    dice = 1 - (2 * (g * p).sum() + SMOOTH) / (p.sum() + g.sum() + SMOOTH)
    focal = (-g * ALPHA * q * q * lp - (1 - g) * (1 - ALPHA) * p * p * lq).mean()
    on = (z > 0).to(z.dtype)
    tp, fp, fn = (g * on).sum(), ((1 - g) * on).sum(), (g * (1 - on)).sum()
    return dict(loss=dice + focal, dice=dice, focal=focal, iou=(tp + SMOOTH) / (tp + fp + fn + SMOOTH),
                f1=(2 * tp + SMOOTH) / (2 * tp + fp + fn + SMOOTH), tp=tp, fp=fp, fn=fn)


def seg_loss_grad(z, g):
    """dloss/dz, written out (what shm_seg_loss's second launch computes)."""
    z, g = z.reshape(-1), g.reshape(-1)
    p, q = torch.sigmoid(z), torch.sigmoid(-z)
    lp, lq = -F.softplus(-z), -F.softplus(z)
    i2, d = 2 * (g * p).sum() + SMOOTH, p.sum() + g.sum() + SMOOTH
    ddice = -(2 * g * d - i2) / (d * d) * p * q
    dpos = q ** 3 - 2 * p * q * q * lp
    dneg = 2 * p * p * q * lq - p ** 3
    return ddice + (-g * ALPHA * dpos - (1 - g) * (1 - ALPHA) * dneg) / z.numel()


LOSS_NPIX = (1, 255, 4097)
LOSS_MASKS = ("zeros", "ones", "soft")
LOSS_LOGITS = ("pm40", "zero", "normal")


def loss_blocks(npix):
    """grid of shm_seg_loss's sum pass: 1024 pixels per block, at most 256 blocks"""
    return max(1, min(256, -(-npix // 1024)))


def loss_case(npix, mask, logits, seed=0):
    rng = np.random.default_rng([seed, npix, LOSS_MASKS.index(mask), LOSS_LOGITS.index(logits)])
    g = {"zeros": np.zeros(npix), "ones": np.ones(npix), "soft": rng.uniform(0.02, 0.98, npix)}[mask]
    z = {"pm40": np.where(rng.random(npix) < 0.5, -40.0, 40.0), "zero": np.zeros(npix), "normal": rng.normal(0, 2, npix)}[logits]
    return z.astype(np.float32), g.astype(np.float32)


# ------------------------------------------------------------------------------------------------- BatchNormalization
def bn_train(a, gamma, beta, eps=BN_EPS):
    """a [npix, c]; returns (out, mean, biased var)."""
    mean = a.mean(0)
    var = ((a - mean) ** 2).mean(0)
    return (a - mean) * (gamma / torch.sqrt(var + eps)) + beta, mean, var


def bn_moving(mm, mv, mean, var, n, momentum=BN_MOMENTUM):
    """Keras' moving-average update fed by TensorFlow's fused kernel: the moving variance takes the unbiased estimate."""
    return mm * momentum + mean * (1 - momentum), mv * momentum + var * (n / max(n - 1, 1)) * (1 - momentum)


BN_CASES = [(npix, c, kind, wide) for npix in (1, 3, 30, 1024) for c in (16, 256) for kind, wide in (("normal", False), ("offset", True))]


def chan_blocks(npix, c):
    """grid of the per-channel sum passes (BatchNormalization, head backward, Conv2DTranspose bias gradient)"""
    pp = 256 // (c // 4)
    return max(1, min(256, -(-npix // (pp * 4))))


def bn_case(npix, c, kind, seed=0):
    """float32 data [npix, c]; "offset": mean 1e3, std 1; channel 1 is constant (variance 0) in every case."""
    rng = np.random.default_rng([seed, npix, c, kind == "offset"])
    a = rng.normal(0, 1, (npix, c)) * rng.uniform(0.5, 2, c) + rng.normal(0, 1, c)
    if kind == "offset":
        a = rng.normal(1e3, 1, (npix, c))
    a[:, 1] = 0.75 if kind == "normal" else 1e3
    dy = rng.normal(0, 1, (npix, c))
    gamma, beta = rng.uniform(0.8, 1.2, c), rng.normal(0, 0.1, c)
    mm, mv = rng.normal(0, 0.1, c), rng.uniform(0.5, 1.5, c)
    return [v.astype(np.float32) for v in (a, dy, gamma, beta, mm, mv)]


# ------------------------------------------------------------------------------------------------------- pool backward
def pool_bwd_first_max(x, dy):
    """x [n,h,w,c], dy [n,h/2,w/2,c] (numpy): each window's gradient to its FIRST maximum in row-major order."""
    n, h, w, c = x.shape
    win = x.reshape(n, h // 2, 2, w // 2, 2, c).transpose(0, 1, 3, 5, 2, 4).reshape(n, h // 2, w // 2, c, 4)
    idx = win.argmax(-1)                                   # numpy: the first occurrence
    d = np.zeros_like(win)
    np.put_along_axis(d, idx[..., None], dy[..., None], -1)
    return d.reshape(n, h // 2, w // 2, c, 2, 2).transpose(0, 1, 4, 2, 5, 3).reshape(n, h, w, c)


POOL_SIZES = ((2, 2), (2, 6), (16, 16))
POOL_TIES = ("all_equal", "pairs", "none")
PAIRS = [(i, j) for i in range(4) for j in range(i + 1, 4)]


def pool_case(batch, h, w, ties, c=16, seed=0):
    """"all_equal": every window holds one value four times; "pairs": window k ties positions PAIRS[k % 6] at its maximum;
    "none": all values distinct."""
    rng = np.random.default_rng([seed, batch, h, w, POOL_TIES.index(ties)])
    nw = batch * (h // 2) * (w // 2) * c
    win = rng.permutation(nw * 4).reshape(nw, 4).astype(np.float64) / (nw * 4)          # distinct
    if ties == "all_equal":
        win[:] = win[:, :1]
    elif ties == "pairs":
        top = win.max(1) + 1.0
        for k in range(nw):
            i, j = PAIRS[k % 6]
            win[k, i] = win[k, j] = top[k]
    x = win.reshape(batch, h // 2, w // 2, c, 2, 2).transpose(0, 1, 4, 2, 5, 3).reshape(batch, h, w, c)
    dy = rng.normal(0, 1, (batch, h // 2, w // 2, c))
    return x.astype(np.float32), dy.astype(np.float32)


# ----------------------------------------------------------------------------------------------------- Conv2DTranspose
CONVT_CASES = [(b, hi, wi, co) for (hi, wi) in ((1, 1), (1, 3), (5, 7), (16, 16)) for b in (1, 3) for co in (16, 128)] + [(3, 32, 24, 16)]


def convt_split(batch, hi, wi):
    """(64-pixel chunks, splits, chunks per split) of the weight-gradient launch"""
    chunks = -(-(batch * hi * wi) // 64)
    ns = max(1, min(chunks, 32))
    cps = -(-chunks // ns)
    return chunks, -(-chunks // cps), cps


def convt_fwd(x, k):
    """x [n,h,w,cin], k [2,2,cout,cin] (torch) -> [n,2h,2w,cout]"""
    n, h, w, _ = x.shape
    return torch.einsum("nhwc,pqoc->nhpwqo", x, k).reshape(n, 2 * h, 2 * w, k.shape[2])


# ----------------------------------------------------------------------------------------------------------------- Adam
def adam_alpha(lr0, b1, b2, iterations):
    t = iterations + 1
    return lr0 * 0.95 ** (iterations / 10000.0) * math.sqrt(1.0 - b2 ** t) / (1.0 - b1 ** t)


def adam_step(w, m, v, g, alpha, b1, b2, eps, clip=0.0):
    if clip > 0:
        g = g.clip(-clip, clip)
    m = m + (g - m) * (1 - b1)
    v = v + (g * g - v) * (1 - b2)
    return w - alpha * m / (np.sqrt(v) + eps), m, v


# -------------------------------------------------------------------------------------------------------- whole network
def forward_train(W, x, keep, dtype=torch.float64):
    """W: list of torch tensors in get_weights() order (leaves for autograd); x [n,H,W,1]; keep: nine keep masks [n,h,w,c] (numpy or
    torch).  Returns (logits [n,H,W,1], [(moving_mean, moving_var)] of the five BatchNormalization layers after the update)."""
    x = torch.as_tensor(np.asarray(x)).to(dtype).permute(0, 3, 1, 2)
    K = [torch.as_tensor(np.asarray(k)).to(dtype).permute(0, 3, 1, 2) for k in keep]
    cv = lambda t: t.view(1, -1, 1, 1)
    it = iter(range(len(W)))
    moving = []

    def conv_relu(t):
        k, b = W[next(it)], W[next(it)]
        return torch.relu(conv2d_same(t, k, 1) + cv(b))

    def pair(t, j):
        a = conv_relu(t)
        return conv_relu(a * K[j] * (1.0 / (1.0 - DROP_RATES[j])))

    def bn(t):
        g, be, mu, var = W[next(it)], W[next(it)], W[next(it)], W[next(it)]
        n = t.shape[0] * t.shape[2] * t.shape[3]
        mean = t.mean((0, 2, 3))
        v = ((t - cv(mean)) ** 2).mean((0, 2, 3))
        moving.append(bn_moving(mu.detach(), var.detach(), mean.detach(), v.detach(), n))
        return (t - cv(mean)) * cv(g / torch.sqrt(v + BN_EPS)) + cv(be)

    def conv_t2(t):
        k, b = W[next(it)], W[next(it)]
        n, _, h, w_ = t.shape
        y = torch.einsum('nchw,pqoc->nohpwq', t, k).reshape(n, k.shape[2], 2 * h, 2 * w_)
        return y + cv(b)

    skips, cur = [], x
    for l in range(5):
        cur = bn(pair(cur, l))
        if l < 4:
            skips.append(cur)
            cur = F.max_pool2d(cur, 2)
    for j, l in enumerate((3, 2, 1, 0)):
        cur = pair(torch.cat([conv_t2(cur), skips[l]], dim=1), 5 + j)
    k, b = W[next(it)], W[next(it)]
    return (conv2d_same(cur, k, 1) + cv(b)).permute(0, 2, 3, 1).contiguous(), moving


def loss_and_grads(weights, x, mask, keep, dtype=torch.float64):
    """One training forward + backward.  Returns ({loss, dice, focal, iou, f1, tp, fp, fn} floats, gradients (numpy float64, None for the
    moving statistics), [(moving_mean, moving_var)] after the update)."""
    W = [torch.as_tensor(np.asarray(w)).to(dtype).requires_grad_(t) for w, t in zip(weights, TRAINABLE)]
    z, moving = forward_train(W, x, keep, dtype)
    L = seg_loss(z, torch.as_tensor(np.asarray(mask)).to(dtype))
    L["loss"].backward()
    grads = [w.grad.double().numpy() if t else None for w, t in zip(W, TRAINABLE)]
    return {k: float(v.detach()) for k, v in L.items()}, grads, [(a.double().numpy(), b.double().numpy()) for a, b in moving]


def trajectory(weights, xs, masks, keeps, lr, b1=0.9, b2=0.999, eps=1e-7, dtype=torch.float64):
    """Adam steps on the batches xs / masks with the keep masks of each step; returns the loss of every step and the final weights."""
    npdt = np.float64 if dtype == torch.float64 else np.float32
    w = [np.asarray(a, dtype=npdt) for a in weights]
    m, v = [np.zeros_like(a) for a in w], [np.zeros_like(a) for a in w]
    bn_idx = [i for i, (k, _) in enumerate(specseg_spec()) if k == "bn_mean"]
    losses = []
    for it, (x, g, keep) in enumerate(zip(xs, masks, keeps)):
        L, grads, moving = loss_and_grads(w, x, g, keep, dtype)
        losses.append(L["loss"])
        a = npdt(adam_alpha(lr, b1, b2, it))
        for i, gr in enumerate(grads):
            if gr is not None:
                w[i], m[i], v[i] = adam_step(w[i], m[i], v[i], gr.astype(npdt), a, npdt(b1), npdt(b2), npdt(eps))
        for i, (mm, mv) in zip(bn_idx, moving):
            w[i], w[i + 1] = mm.astype(npdt), mv.astype(npdt)
    return losses, w


def discs(n, S, seed):
    """Synthetic task: smooth background plus bright discs; mask = the discs.  Returns (x [n,S,S,1] standardised per image, mask)."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:S, 0:S].astype(np.float64) / S
    xs, ms = [], []
    for _ in range(n):
        a, b, c = rng.uniform(-1, 1, 3)
        img = 0.4 + 0.15 * (a * xx + b * yy) + 0.05 * np.sin(6.28 * (xx * c + yy))
        m = np.zeros((S, S))
        for _ in range(rng.integers(1, 4)):
            cx, cy, r = rng.uniform(0.15, 0.85), rng.uniform(0.15, 0.85), rng.uniform(0.08, 0.2)
            m = np.maximum(m, ((xx - cx) ** 2 + (yy - cy) ** 2 < r * r).astype(np.float64))
        img = img + 0.5 * m
        img = (img - img.mean()) / max(img.std(), 1.0 / S)
        xs.append(img)
        ms.append(m)
    return np.stack(xs)[..., None].astype(np.float32), np.stack(ms)[..., None].astype(np.float32)


# the behaviour test: 20 steps at S = 32, B = 4 on one batch of discs; lr chosen on the CPU (test_specseg_train_cpu.py) so that the float64
# reference's last loss is below half its first
TRAJ = dict(B=4, S=32, steps=20, lr=2e-3, data_seed=11)


def random_keep(shapes_n_h_w, seed):
    """nine host keep masks for CPU-only tests: (n, H, W) -> list of [n,h,w,c] float32 in {0,1}"""
    n, H, W = shapes_n_h_w
    rng = np.random.default_rng(seed)
    out = []
    for j, rate in enumerate(DROP_RATES):
        l = j if j < 5 else 8 - j
        out.append((rng.random((n, H >> l, W >> l, WIDTHS[l])) >= rate).astype(np.float32))
    return out
