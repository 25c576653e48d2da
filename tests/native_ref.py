"""Float64 restatement of the native-resolution test mode (shmgan_amd.evaluate.test(eval_size="native")): the padding rule of
shmgan_amd.data.pad_geometry stated independently, the reflect fill, the oracle's inference path on a rectangular frame, the crop
back to the photo, and metrics / export on the crop.

`oracle.step_torch.infer` builds zeros(B, S, S, 1) and is square; its pieces are not.  `infer_hw` restates it from those pieces
(generator_forward, per_image_standardization, rgb_to_yuv, yuv_to_rgb, and oracle.specseg_torch.specseg_forward for the mask);
tests/test_native_cpu.py ties it to `infer` on a square input."""
import numpy as np
import torch

from oracle import specseg_torch as sg
from oracle import step_torch as st

import export_ref
from metrics_ref import image_metrics


def ceil16(n):
    return -(-int(n) // 16) * 16


def pad_geometry(h, w):
    """(Hp, Wp, top, left): sides rounded up to multiples of 16, the photo centred, the odd pad pixel after it."""
    hp, wp = ceil16(h), ceil16(w)
    return hp, wp, (hp - h) // 2, (wp - w) // 2


def reflect_index(i, n):
    """Index into [0, n) of position i of a signal continued by reflection WITHOUT repeating the edge sample."""
    i = np.abs(np.asarray(i))
    return np.where(i >= n, 2 * (n - 1) - i, i)


def pad_reflect(img):
    """[h,w,c] -> ([Hp,Wp,c], window (top, left, h, w)) by index arithmetic (np.pad(mode="reflect") is what it must equal)."""
    h, w = img.shape[:2]
    hp, wp, top, left = pad_geometry(h, w)
    ys = reflect_index(np.arange(hp) - top, h)
    xs = reflect_index(np.arange(wp) - left, w)
    return img[ys][:, xs], (top, left, h, w)


def load_pad_u8(u8):
    """What shm_load_pad_u8 must give, bit for bit: float32(u8) * float32(1/255), reflected into the frame."""
    frame, win = pad_reflect(np.asarray(u8, np.uint8))
    return frame.astype(np.float32) * np.float32(1.0 / 255.0), win


def crop(x, window):
    """The window (top, left, h, w) of [..., Hp, Wp, C]."""
    top, left, h, w = window
    return x[..., top:top + h, left:left + w, :]


def infer_hw(gvars, gbetas, rgb, filter_size=64, specseg=None, attention=None, cyclic=True, dtype=torch.float64):
    """oracle.step_torch.infer on a frame rgb [B,H,W,3] (H, W multiples of 16), from the oracle's own pieces.
    specseg: SpecSeg weights (the mask of the standardised Y plane, test.py:221; also the input of the live attention branch);
    attention: the generator's attention variables (attention="live"), None for the executed graph."""
    T = lambda a: torch.as_tensor(np.asarray(a) if not torch.is_tensor(a) else a).to(dtype)
    gv, gb = [T(a) for a in gvars], [T(a) for a in gbetas]
    x = T(rgb)
    B, H, W = x.shape[:3]
    yuv, scale = st.per_image_standardization(st.rgb_to_yuv(x))
    cbcr = yuv[..., 1:]
    mask = None if specseg is None else sg.specseg_forward(specseg, yuv[..., 0:1].numpy(), dtype)
    attn = None if attention is None else st.generator_attention([T(a) for a in attention], mask)
    zeros, ones = torch.zeros(B, H, W, 1, dtype=dtype), torch.ones(B, H, W, 1, dtype=dtype)
    gen_Y = st.generator_forward(gv, gb, torch.cat([yuv[..., 0:1]] + [zeros] * 8 + [ones], dim=3), filter_size, attn=attn)
    gen_rgb = st.yuv_to_rgb(torch.cat([gen_Y, cbcr], dim=3))
    out = {"gen_Y": gen_Y, "gen_rgb": gen_rgb, "scale": scale, "mask": mask, "cyc_rgb": []}
    if cyclic:
        y0 = gen_rgb[..., 0:1]
        for k in range(5):
            chans = [zeros if j == k else y0 for j in range(5)]
            onehot = [ones if j == k else zeros for j in range(5)]
            cy = st.generator_forward(gv, gb, torch.cat(chans + onehot, dim=3), filter_size, attn=attn)
            out["cyc_rgb"].append(st.yuv_to_rgb(torch.cat([cy, cbcr], dim=3)))
    return out


def metrics_hw(pred, window, target):
    """tests/metrics_ref.image_metrics of the window of pred [B,Hp,Wp,3] against the tight target [B,h,w,3]."""
    return image_metrics(crop(np.asarray(pred, np.float64), window), np.asarray(target, np.float64))


def export_hw(plane, window, ho, wo, mode, mul=1.0):
    """tests/export_ref.export of the window (y0, x0, hc, wc) of plane [Hs,Ws,C], resampled to (ho, wo) -> (bytes, y).
    export_ref.export copies when (ho, wo) equals its square side: here the copy is (ho, wo) == (hc, wc)."""
    x = crop(np.asarray(plane, np.float64), window)
    lo, hi = x.min(), x.max()
    v = x if (ho, wo) == x.shape[:2] else export_ref.resize_bilinear(x, ho, wo)
    if mode == "rescale":
        t = np.zeros_like(v) if hi == lo else (v - lo) / (hi - lo)
    elif mode == "scale":
        t = v * float(mul)
    elif mode == "clip":
        t = v
    else:
        raise ValueError(mode)
    return export_ref.quantize(t)
