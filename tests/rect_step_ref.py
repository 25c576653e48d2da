"""The float64 reference of a train_step on an H x W frame (image_hw), composed from the functions of oracle/step_torch.py.

oracle.step_torch is shape-agnostic in generator_forward, discriminator_forward, ssim, rescale_01, gram_matrix,
per_image_standardization, softmax_xent and adam_apply; it names a single side in four places: _train_step (torch.zeros(B, S, S, 1)),
init_params, make_draws and make_inputs.  This file restates those four for a pair -- same seeds, same draw order, same composition of
the losses line by line -- so that on a square frame every number equals the oracle's (tests/test_rect_step_cpu.py holds them to
1e-12), and nothing else: every network, loss and optimiser function is the oracle's own."""
from types import SimpleNamespace

import numpy as np
import torch

from oracle import step_torch as st

t64 = lambda a: torch.as_tensor(np.asarray(a), dtype=torch.float64)


def discriminator_spec_hw(filter_size, h, w):
    """oracle.step_torch.discriminator_spec with the Dense kernel of an H x W frame: (H/32)(W/32) 16F inputs (NHWC flatten)."""
    spec = st.discriminator_spec(filter_size, 32)
    name, kind, _ = spec[-1]
    return spec[:-1] + [(name, kind, ((h // 32) * (w // 32) * 16 * filter_size, 5))]


def init_params_hw(filter_size, h, w, seed=42, beta_seed=43):
    """oracle.step_torch.init_params for an H x W frame: the same streams in the same order (only the Dense kernel's shape knows
    the frame, and it is drawn last)."""
    rng = np.random.default_rng(seed)
    g = [np.zeros(shp, np.float32) if len(shp) == 1 else rng.normal(0.0, 0.02, shp).astype(np.float32)
         for shp in st.generator_var_shapes(filter_size)]
    d = [rng.normal(0.0, 0.02, shp).astype(np.float32) for _, _, shp in discriminator_spec_hw(filter_size, h, w)]
    brng = np.random.default_rng(beta_seed)
    gb = [brng.normal(0.0, 0.02, (c,)).astype(np.float32) for c in st.generator_in_channels(filter_size)]
    db = [brng.normal(0.0, 0.02, (c,)).astype(np.float32) for c in st.discriminator_in_channels(filter_size)]
    return g, d, gb, db


def make_draws_hw(step, batch, h, w, filter_size, rank=0):
    """oracle.step_torch.make_draws for an H x W frame: noise [2B,H,W,3], keep mask [2B,H/32,W/32,16F]."""
    r = np.random.default_rng(7 + step)
    flags = tuple(bool(u < 0.5) for u in r.random(5))
    target = float(r.uniform(0.8, 1.2))
    r2 = np.random.default_rng([7 + step, rank, 1])
    noise = (0.1 * r2.standard_normal((2 * batch, h, w, 3))).astype(np.float32)
    keep = (r2.random((2 * batch, h // 32, w // 32, 16 * filter_size)) >= 0.2).astype(np.float32)
    return st.StepDraws(flags, target, noise, keep)


def make_inputs_hw(batch, h, w, rank=0):
    """oracle.step_torch.make_inputs for an H x W frame."""
    r = np.random.default_rng(1234 + rank)
    return [r.random((batch, h, w, 3), dtype=np.float32) for _ in range(5)]


def style_factor_hw(h, w):
    """As intended: 1 / (2 * 9 * H * W)^2 (oracle.step_torch.style_factor_intended on a square)."""
    return 1.0 / float(2 * 9 * h * w) ** 2


def train_step_hw(gvars, dvars, gbetas, dbetas, inputs, draws, style_factor, filter_size=64, dtype=torch.float64, need_grads=True,
                  masks=None, specseg=None, attention=None, xent_mode="executed"):
    """oracle.step_torch.train_step on [B,H,W,3] inputs: the same statements in the same order with the frame read from the inputs
    (no kink recorder, no InstanceNorm log).  masks / specseg / attention / xent_mode as there.  Returns the same dict."""
    mk = masks or {}
    T = lambda a: torch.as_tensor(np.asarray(a) if not torch.is_tensor(a) else a).to(dtype)
    gv = [T(a).clone().requires_grad_(need_grads) for a in gvars]
    dv = [T(a).clone().requires_grad_(need_grads) for a in dvars]
    gb, db = [T(a) for a in gbetas], [T(a) for a in dbetas]
    orig = [T(a) for a in inputs]
    B, H, W = (int(v) for v in orig[0].shape[:3])
    tl = float(draws.target_label)
    flags = [bool(f) for f in draws.flags]
    noise, keep = T(draws.noise), T(draws.keep_mask)
    mslice = st._mslice

    ds, scales = [], []
    for o in orig:
        y, sc = st.per_image_standardization(st.rgb_to_yuv(o))
        ds.append(y)
        scales.append(sc)
    Ych = [d[..., 0:1] for d in ds]
    zeros = torch.zeros(B, H, W, 1, dtype=dtype)
    ones = torch.ones(B, H, W, 1, dtype=dtype)
    avgCbCr = (ds[0][..., 1:] + ds[1][..., 1:] + ds[2][..., 1:] + ds[3][..., 1:] + ds[4][..., 1:]) / 5.0

    spec_mask = None
    if specseg is not None:
        from oracle.specseg_torch import specseg_forward
        spec_mask = specseg_forward(specseg, Ych[2], dtype).detach()
    ga = da = attn_g = attn_d = None
    if attention is not None:
        assert spec_mask is not None, "attention='live' needs the SpecSeg weights"
        ga = [T(a).clone().requires_grad_(need_grads) for a in attention["G"]]
        da = [T(a).clone().requires_grad_(need_grads) for a in attention["D"]]
        attn_g = st.generator_attention(ga, spec_mask, mk.get("ga"))
        attn_d, _ = st.attention_layer(da, spec_mask.permute(0, 3, 1, 2), 16, mk.get("da"), 0)

    rand_inp = [zeros if flags[k] else Ych[k] for k in range(5)]
    gen_input = torch.cat(rand_inp + [zeros, zeros, zeros, zeros, ones], dim=3)
    gen_Y = st.generator_forward(gv, gb, gen_input, filter_size, masks=mk.get("g1"), attn=attn_g)
    gen_yuv = torch.cat([gen_Y, avgCbCr], dim=3)
    gen_rgb = st.yuv_to_rgb(gen_yuv)

    md = mk.get("d")
    rf_D1, cls_D1 = st.discriminator_forward(dv, db, gen_rgb, noise[:B], keep[:B], masks=mslice(md, 0, B), attn=attn_d)
    rf_D2, cls_D2 = st.discriminator_forward(dv, db, orig[4], noise[B:], keep[B:], masks=mslice(md, 6 * B, 7 * B), attn=attn_d)

    sub = [gen_Y if flags[k] else Ych[k] for k in range(5)]
    cyc_Y = []
    for k in range(5):
        chans = [zeros if j == k else sub[j] for j in range(5)]
        onehot = [ones if j == k else zeros for j in range(5)]
        cyc_Y.append(st.generator_forward(gv, gb, torch.cat(chans + onehot, dim=3), filter_size,
                                          masks=mslice(mk.get("cyc"), k * B, (k + 1) * B), attn=attn_g))
    cyc_yuv = [torch.cat([cy, avgCbCr], dim=3) for cy in cyc_Y]
    cyc_rgb = [st.yuv_to_rgb(c) for c in cyc_yuv]

    D3, D4 = [], []
    for k in range(5):
        D3.append(st.discriminator_forward(dv, db, cyc_rgb[k], masks=mslice(md, (1 + k) * B, (2 + k) * B), attn=attn_d))
    for k in range(5):
        D4.append(st.discriminator_forward(dv, db, orig[k], masks=mslice(md, (7 + k) * B, (8 + k) * B), attn=attn_d))

    def mse(a, t):
        return ((a - t) ** 2).mean(dim=(1, 2, 3))

    def xent(logits, k, w=1.0):
        lab = torch.zeros_like(logits)
        lab[:, k] = w
        return st.softmax_xent(logits, lab, xent_mode)

    D3_RF = sum(mse(D3[k][0], tl) for k in range(5))
    D1_RF = mse(rf_D1, tl)
    D3_cls = sum(xent(D3[k][1], k) for k in range(5))
    D1_cls = xent(cls_D1, 4, tl)
    D4_cls = sum(xent(D4[k][1], k) for k in range(5))
    D2_RF = mse(rf_D2, tl) + (rf_D1 ** 2).mean(dim=(1, 2, 3))
    D4_RF = sum(mse(D4[k][0], tl) + (D3[k][0] ** 2).mean(dim=(1, 2, 3)) for k in range(5)) + D2_RF

    l1 = lambda a, b: (a - b).abs().mean(dim=(1, 2, 3))
    L1_G1 = l1(gen_rgb, orig[4])
    L1_c = [l1(cyc_rgb[k], orig[k]) for k in range(5)]
    L1_loss = (L1_c[0] + L1_c[1] + L1_c[2] + L1_c[3] + L1_G1) / 5.0 + L1_c[4] * 10.0

    ssims = [st.ssim(st.rescale_01(cyc_yuv[k]), st.rescale_01(ds[k])) for k in range(5)]
    sl = [torch.zeros(B, dtype=dtype) if flags[k] else -torch.log((1.0 + ssims[k]) / 2.0) for k in range(5)]
    ssim_loss = (sl[0] + sl[1] + sl[2] + sl[3] + sl[4] * 10.0) / 5.0

    content = ((cyc_yuv[4] - ds[0]) ** 2).mean(dim=(1, 2, 3))
    style = style_factor * ((st.gram_matrix(cyc_yuv[4]) - st.gram_matrix(ds[4])) ** 2).mean(dim=(1, 2))
    nst = 100.0 * style + content

    total_G = (D1_RF + D3_RF) / 6.0 + 10.0 * L1_loss + 10.0 * ssim_loss + 10.0 * nst
    total_D = (D1_cls + D3_cls) / 6.0 + (D2_RF + D4_RF) / 6.0 + 0.5 * D4_cls + 10.0 * nst
    total_C = (D4_cls + nst) * 10.0

    losses = {
        "total_Generator_loss": total_G, "total_Discriminator_loss": total_D,
        "total_Classification_loss": total_C, "G_gan_loss": (D3_RF + D1_RF) / 6.0,
        "G_clsf_loss": (D3_cls + D1_cls) / 6.0,
        "D1_RealFake_loss": D1_RF, "D3_RealFake_cyc": D3_RF, "D2_RealFake_target": D2_RF,
        "D4_RealFake_cyc": D4_RF, "D1_classification_loss": D1_cls,
        "D3_classification_loss": D3_cls, "D4_classification_loss": D4_cls,
        "L1_loss_Gen": L1_loss, "ssim_cyc_loss": ssim_loss, "content_loss": content,
        "style_loss": style, "total_NST_loss": nst,
    }
    if specseg is not None:
        from oracle.specseg_torch import spec_loss
        losses["Spec_loss"] = spec_loss([c.detach() for c in cyc_yuv], ds, spec_mask)[0]
    out = {"losses": {k: float(v.mean().detach()) for k, v in losses.items()},
           "outs": {"gen_Y": gen_Y.detach(), "gen_rgb": gen_rgb.detach(), "cyc_rgb": [c.detach() for c in cyc_rgb],
                    "rf_D1": rf_D1.detach(), "cls_D1": cls_D1.detach(), "ssim": [s_.detach() for s_ in ssims],
                    "scales": [s_.detach() for s_ in scales], "specular_candidate": spec_mask}}
    if need_grads:
        gD = torch.autograd.grad((total_D + total_C).mean(), dv + (da or []), retain_graph=True)
        if da is not None:
            gD, out["gDa"] = gD[:len(dv)], list(gD[len(dv):])
        mid = torch.autograd.grad(total_G.mean(), cyc_Y + [gen_Y], retain_graph=True)
        out["dcyc_Y"], out["dgen_Y"] = [m_.detach() for m_ in mid[:5]], mid[5].detach()
        gG = torch.autograd.grad(total_G.mean(), gv + (ga or []))
        if ga is not None:
            gG, out["gGa"] = gG[:len(gv)], list(gG[len(gv):])
        out["gD"], out["gG"] = list(gD), list(gG)
    return out


# ------------------------------------------------------------------------------------------- the stand-alone image-loss kernel
# (B, h, w) of the stand-alone shm_image_losses_hw cases: one output row, one output column, one forward tile down and four across
# (and its transpose), partial tiles on both axes -- and the two flag patterns every case runs with
IMAGE_SHAPES = [(1, 11, 43), (1, 43, 11), (2, 26, 59), (2, 59, 26), (1, 37, 48)]
IMAGE_FLAGS = [(False, True, False, False, False), (True, False, False, True, False)]
# whole-step parity shapes (H, W, F, B, step); test_rect_step_cpu.py shows that no reference gradient tensor vanishes at them
STEP_SHAPES = [(64, 96, 16, 1, 0), (96, 64, 16, 2, 1), (64, 128, 32, 1, 0)]


def image_inputs_hw(B, h, w, seed=21):
    """loss_edge_ref.image_inputs_random on an h x w frame, drawn in its order (tests/loss_edge_ref.image_oracle then works on it
    as it is: it reads the shapes of its `inp` namespace)."""
    rng = np.random.default_rng(seed)
    orig = [rng.random((B, h, w, 3)) for _ in range(5)]
    ds = [st.per_image_standardization(st.rgb_to_yuv(t64(o)))[0] for o in orig]
    cbcr = sum(d[..., 1:] for d in ds) / 5.0
    gen_y = rng.standard_normal((B, h, w, 1)) * 0.5 + 1.0
    cyc_y = rng.standard_normal((5 * B, h, w, 1)) * 0.5 + 1.0
    return SimpleNamespace(B=B, H=h, W=w, orig=orig, ds=ds, cbcr=cbcr, gen_y=gen_y, cyc_y=cyc_y)
