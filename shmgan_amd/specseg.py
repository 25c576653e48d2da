"""SpecSeg mask network on the HIP kernels: inference (`predict`) and training (`fit`).

Mirrors /root/reference/SpecSeg.py:27-98 as `train_step` uses it (`self.SpecSeg.predict(I90_Ych)`,
SHM.py:492; test.py:221): a U-Net of Conv2D(3x3, relu) pairs with inference-mode
BatchNormalization after each encoder pair, MaxPooling2D(2), Conv2DTranspose(2x2, stride 2) +
Concatenate([up, skip]) in the decoder and a Conv2D(1, 1x1, sigmoid) head; Dropout layers are
inactive under `predict`.  Widths are fixed (16..256) whatever the GAN's filter_size.

The reference loads `specsegv3_chkpt.h5`, which is not part of the mount: `init_random()` gives the
Keras initialisers of SpecSeg.py instead, `set_weights()` takes `model.get_weights()` of a trained
Keras SpecSeg (variable order and layouts preserved: HWIO kernels, Conv2DTranspose
[kh,kw,Cout,Cin], BatchNormalization gamma/beta/moving_mean/moving_variance).

Training (`forward_train` / `backward` / `train_step` / `fit` / `evaluate`) makes the weights here: Dropout active,
BatchNormalization on batch statistics, the Dice + binary focal loss of csrc/specseg_train.hip and Adam on
the schedule of SHM.py:169-175.  `predict` / `forward_plane` are untouched by it: a network that was never trained behaves as before.
"""
from __future__ import annotations

import numpy as np
import torch

from . import ops

WIDTHS = (16, 32, 64, 128, 256)
BN_EPS = 1e-3                      # Keras BatchNormalization default (SpecSeg.py:37 passes none)
BN_MOMENTUM = 0.99                 # likewise
PAD_C = 16
# Dropout rates between the two convolutions of each pair, encoder c1..c5 then decoder c6..c9 (SpecSeg.py:35-85)
DROP_RATES = (0.1, 0.1, 0.2, 0.2, 0.3, 0.2, 0.2, 0.1, 0.1)
LOSS_KEYS = ("loss", "dice", "focal", "iou", "f1")


def specseg_variables():
    """[(keras_name, kind, shape)] in `model.get_weights()` order (SpecSeg_summary.txt)."""
    out = []
    ci = [0]

    def conv(cin, cout, k=3):
        n = "conv2d" if ci[0] == 0 else f"conv2d_{ci[0]}"
        ci[0] += 1
        out.append((n + "/kernel", "conv", (k, k, cin, cout)))
        out.append((n + "/bias", "bias", (cout,)))

    cin = 1
    for l, w in enumerate(WIDTHS):
        conv(cin, w)
        conv(w, w)
        bn = "batch_normalization" if l == 0 else f"batch_normalization_{l}"
        for p in ("gamma", "beta", "moving_mean", "moving_variance"):
            out.append((f"{bn}/{p}", "bn", (w,)))
        cin = w
    for j, l in enumerate((3, 2, 1, 0)):
        w = WIDTHS[l]
        t = "conv2d_transpose" if j == 0 else f"conv2d_transpose_{j}"
        out.append((t + "/kernel", "convT", (2, 2, w, 2 * w)))
        out.append((t + "/bias", "bias", (w,)))
        conv(2 * w, w)
        conv(w, w)
    conv(WIDTHS[0], 1, k=1)
    return out


class SpecSeg:
    name = "SpecSeg"
    trainable = False                      # the default of a network that was never trained; fit() sets the instance's flag

    def __init__(self, image_size, device, arena):
        self.grad = self.m = self.v = None  # flat gradient and Adam moments, made by the first train_step / fit
        self.iterations = 0
        self.lr0, self.beta_1, self.beta_2, self.epsilon = 1e-3, 0.9, 0.999, 1e-7
        self.train_seed, self.train_counter = 44, 0       # the (seed, counter) of the Dropout masks train_step draws
        self._tape = None
        assert image_size % 16 == 0, "SpecSeg needs image_size % 16 == 0 (four 2x2 pools)"
        self.S, self.dev, self.arena = image_size, device, arena
        self.spec = specseg_variables()
        sizes = [int(np.prod(s)) for _, _, s in self.spec]
        self.n = sum(sizes)
        self.flat = torch.zeros(self.n, dtype=torch.float32, device=device)
        self.vars, off = [], 0
        for (_, _, s), z in zip(self.spec, sizes):
            self.vars.append(self.flat[off:off + z].view(s))
            off += z
        self.index = {n: i for i, (n, _, _) in enumerate(self.spec)}
        self.wk = {}
        for i, (n, kind, s) in enumerate(self.spec):
            if kind == "conv" and s[3] > 1:
                k, _, cin, cout = s
                self.wk[i] = torch.zeros(k * k * cout * _pad16(cin), dtype=torch.float32, device=device)
        self.weights_dirty = True

    # ---- parameters ---------------------------------------------------------------------
    def count_params(self):
        return self.n

    def get_weights(self):
        return [v.detach().cpu().numpy().copy() for v in self.vars]

    def set_weights(self, arrays):
        assert len(arrays) == len(self.vars)
        for v, a in zip(self.vars, arrays):
            a = torch.as_tensor(np.asarray(a, dtype=np.float32))
            assert tuple(a.shape) == tuple(v.shape), (a.shape, v.shape)
            v.copy_(a)
        self.weights_dirty = True

    def init_random(self, seed=44):
        """Keras initialisers of SpecSeg.py: RandomNormal(0, 0.05) on the 3x3 kernels, glorot_uniform on
        the Conv2DTranspose / head kernels, zeros for biases, BN gamma 1, beta 0, mean 0, variance 1."""
        rng = np.random.default_rng(seed)
        ws = []
        for n, kind, s in self.spec:
            if kind == "conv" and s[0] == 3:
                ws.append(rng.normal(0.0, 0.05, s).astype(np.float32))
            elif kind in ("conv", "convT"):
                rf = s[0] * s[1]
                lim = np.sqrt(6.0 / (rf * s[2] + rf * s[3]))
                ws.append(rng.uniform(-lim, lim, s).astype(np.float32))
            elif kind == "bn":
                ws.append(np.ones(s, np.float32) if n.endswith(("gamma", "moving_variance")) else np.zeros(s, np.float32))
            else:
                ws.append(np.zeros(s, np.float32))
        self.set_weights(ws)
        return self

    def prepare_weights(self):
        if not self.weights_dirty:
            return
        for i, wk in self.wk.items():
            k, _, cin, cout = self.spec[i][2]
            ops.transpose_taps(self.vars[i], wk, k * k, cin, cout, _pad16(cin))
        self.weights_dirty = False

    # ---- forward ------------------------------------------------------------------------
    def _conv(self, tag, i, x, x2, c1, ldx, ldx2, n, h, w):
        k, _, cin, cout = self.spec[i][2]
        y = self.arena.get(f"{tag}/c{i}", (n, h, w, cout))
        ops.conv2d_fwd(x, x2, c1, ldx, ldx2, self.wk[i], self.vars[i + 1], y, cout, n, h, w, _pad16(cin), cout, k, 1, 0.0,
                       cin_real=cin)
        return y

    def forward_plane(self, src, ldsrc, c0, n, tag="specseg"):
        """Mask of channel c0 of `src` ([n,H,W,ldsrc], H and W multiples of 16: the network is fully convolutional, (S, S) in
        training); returns [n,H,W,1] in (0,1)."""
        A = self.arena
        H, W = int(src.shape[1]), int(src.shape[2])
        assert src.dim() == 4 and H >= 16 and W >= 16 and H % 16 == 0 and W % 16 == 0, f"SpecSeg takes maps whose sides are multiples of 16, got {tuple(src.shape)}"
        self.prepare_weights()
        x16 = A.get(f"{tag}/x16", (n, H, W, PAD_C))
        ops.pack_channels(src, ldsrc, c0, 1, x16, PAD_C, n * H * W)
        cur, ld, h, wd = x16, PAD_C, H, W
        i = 0
        skips = []
        for l, w in enumerate(WIDTHS):
            a = self._conv(tag, i, cur, None, 0, ld, 0, n, h, wd)
            b = self._conv(tag, i + 2, a, None, 0, w, 0, n, h, wd)
            c = A.get(f"{tag}/bn{l}", (n, h, wd, w))
            g, be, mu, var = self.vars[i + 4:i + 8]
            ops.bn_apply(b, w, g, be, mu, var, BN_EPS, c, w, n * h * wd, w)
            i += 8
            if l < 4:
                skips.append((c, w, h))
                p = A.get(f"{tag}/p{l}", (n, h // 2, wd // 2, w))
                ops.maxpool2_fwd(c, w, p, w, n, h, wd, w)
                cur, ld, h, wd = p, w, h // 2, wd // 2
            else:
                cur, ld = c, w
        for l in (3, 2, 1, 0):
            w = WIDTHS[l]
            u = A.get(f"{tag}/u{l}", (n, 2 * h, 2 * wd, w))
            ops.conv2d_transpose2x2_fwd(cur, ld, self.vars[i], self.vars[i + 1], u, w, n, h, wd, 2 * w, w, 1.0)
            i += 2
            h, wd = 2 * h, 2 * wd
            skip, sw, sh = skips[l]
            assert sh == h and sw == w
            a = self._conv(tag, i, u, skip, w, w, w, n, h, wd)        # Concatenate([up, skip])
            b = self._conv(tag, i + 2, a, None, 0, w, 0, n, h, wd)
            i += 4
            cur, ld = b, w
        y = A.get(f"{tag}/mask", (n, H, W, 1))
        ops.head_sigmoid_fwd(cur, ld, self.vars[i], self.vars[i + 1], y, n * H * W, ld)
        return y

    def predict(self, x, verbose=0):
        """Keras-style `SpecSeg.predict(I90_Ych, verbose=0)` on a [N,S,S,1] tensor (SHM.py:492)."""
        if isinstance(x, np.ndarray):
            x = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32))
        x = x.to(self.dev, torch.float32).contiguous()
        assert x.dim() == 4 and x.shape[1] == self.S and x.shape[2] == self.S and x.shape[3] == 1
        return self.forward_plane(x, 1, 0, x.shape[0], tag="specseg/predict")

    __call__ = predict

    # ---- training -----------------------------------------------------------------------
    def keep_masks(self, n, H, W, seed, counter):
        """The nine Dropout keep masks of one training forward on [n,H,W,1], drawn by shm_keep_mask on (seed, 9 * counter + j)."""
        A = self.arena
        out = []
        for j, rate in enumerate(DROP_RATES):
            l = j if j < 5 else 8 - j
            m = A.get(f"specseg/train/keep{j}", (n, H >> l, W >> l, WIDTHS[l]))
            ops.keep_mask(m, rate, seed, (9 * int(counter) + j) & 0xFFFFFFFF)
            out.append(m)
        return out

    def _bn_ws(self):
        return self.arena.get("specseg/train/bnws", (ops.bn_train_ws_doubles(WIDTHS[-1]),), torch.float64)

    def _pair_fwd(self, j, i, x, x2, c1, ldx, ldx2, n, h, w, keep):
        """conv (relu) -> Dropout -> conv (relu) of pair j (variables i .. i+3); returns the tape record and the output."""
        A, tag = self.arena, "specseg/train"
        cout = self.spec[i][2][3]
        a = self._conv(tag, i, x, x2, c1, ldx, ldx2, n, h, w)
        ad = A.get(f"{tag}/ad{j}", (n, h, w, cout))
        ops.mul_mask(a, keep, ad, a.numel(), 1.0 / (1.0 - DROP_RATES[j]))
        b = self._conv(tag, i + 2, ad, None, 0, cout, 0, n, h, w)
        return dict(j=j, i=i, x=x, x2=x2, c1=c1, ldx=ldx, ldx2=ldx2, n=n, h=h, w=w, cout=cout, a=a, ad=ad, b=b, keep=keep), b

    def forward_train(self, x, keep_masks):
        """The forward of forward_plane on x [n,H,W,1] with Dropout active (keep_masks: the nine masks of keep_masks(), scaled
        1/(1-rate) here) and batch statistics in the five BatchNormalization layers (the moving statistics are updated).  Every
        tensor the backward needs stays in the arena under specseg/train/*.  Returns the logits [n,H,W,1] (pre-sigmoid)."""
        A, tag = self.arena, "specseg/train"
        n, H, W = int(x.shape[0]), int(x.shape[1]), int(x.shape[2])
        assert x.dim() == 4 and x.shape[3] == 1 and H >= 16 and W >= 16 and H % 16 == 0 and W % 16 == 0, f"SpecSeg takes [n,H,W,1] maps whose sides are multiples of 16, got {tuple(x.shape)}"
        assert x.dtype == torch.float32 and x.is_contiguous() and len(keep_masks) == len(DROP_RATES)
        self.prepare_weights()
        x16 = A.get(f"{tag}/x16", (n, H, W, PAD_C))
        ops.pack_channels(x, 1, 0, 1, x16, PAD_C, n * H * W)
        cur, ld, h, wd = x16, PAD_C, H, W
        i = 0
        enc, dec = [], []
        for l, w in enumerate(WIDTHS):
            rec, b = self._pair_fwd(l, i, cur, None, 0, ld, 0, n, h, wd, keep_masks[l])
            c = A.get(f"{tag}/bn{l}", (n, h, wd, w))
            save = A.get(f"{tag}/bnsave{l}", (2 * w,), torch.float64)
            g, be, mu, var = self.vars[i + 4:i + 8]
            ops.bn_train_fwd(b, w, g, be, mu, var, BN_MOMENTUM, BN_EPS, c, w, save, self._bn_ws(), n * h * wd, w)
            rec.update(bn=c, save=save, l=l)
            enc.append(rec)
            i += 8
            if l < 4:
                p = A.get(f"{tag}/p{l}", (n, h // 2, wd // 2, w))
                ops.maxpool2_fwd(c, w, p, w, n, h, wd, w)
                cur, ld, h, wd = p, w, h // 2, wd // 2
            else:
                cur, ld = c, w
        for k, l in enumerate((3, 2, 1, 0)):
            w = WIDTHS[l]
            u = A.get(f"{tag}/u{l}", (n, 2 * h, 2 * wd, w))
            ops.conv2d_transpose2x2_fwd(cur, ld, self.vars[i], self.vars[i + 1], u, w, n, h, wd, 2 * w, w, 1.0)
            up = dict(ti=i, tx=cur, th=h, tw=wd, l=l)
            i += 2
            h, wd = 2 * h, 2 * wd
            rec, b = self._pair_fwd(5 + k, i, u, enc[l]["bn"], w, w, w, n, h, wd, keep_masks[5 + k])
            rec.update(up)
            dec.append(rec)
            i += 4
            cur, ld = b, w
        z = A.get(f"{tag}/z", (n, H, W, 1))
        ops.head_logit_fwd(cur, ld, self.vars[i], self.vars[i + 1], z, n * H * W, ld)
        self._tape = dict(enc=enc, dec=dec, head=i, n=n, H=H, W=W, last=cur)
        return z

    def _train_buffers(self):
        if self.grad is None:
            self.grad = torch.zeros(self.n, dtype=torch.float32, device=self.dev)
            self.grads, off = [], 0
            for (_, _, s), v in zip(self.spec, self.vars):
                self.grads.append(self.grad[off:off + v.numel()].view(s))
                off += v.numel()
            # bias gradients are summed in f64 (shm_lrelu_bwd's accumulators), one slice per Conv2D bias
            self._acc_off, nb = {}, 0
            for i, (nm, kind, s) in enumerate(self.spec):
                if kind == "bias" and self.spec[i - 1][1] == "conv" and self.spec[i - 1][2][3] > 1:
                    self._acc_off[i] = nb
                    nb += s[0]
            self._acc = torch.zeros(nb, dtype=torch.float64, device=self.dev)
        if self.m is None:
            self.m = torch.zeros(self.n, dtype=torch.float32, device=self.dev)
            self.v = torch.zeros(self.n, dtype=torch.float32, device=self.dev)

    def _workspace(self, nbytes):
        """Workspace of the weight-gradient launches (they run in order on one stream); grows to the largest request."""
        n = (int(nbytes) + 3) // 4
        t = getattr(self, "_wgrad_ws", None)
        if t is None or t.numel() < n:
            torch.cuda.current_stream().synchronize()
            t = self._wgrad_ws = torch.empty(max(n, 1), dtype=torch.float32, device=self.dev)
        return t

    def _pair_bwd(self, rec, g_b, need_dx):
        """Backward of one conv / Dropout / conv pair from the gradient at its output; returns (dx, dx2) of its first convolution."""
        A, tag = self.arena, "specseg/train"
        j, i, n, h, w, c = rec["j"], rec["i"], rec["n"], rec["h"], rec["w"], rec["cout"]
        cin = self.spec[i][2][2]
        red = A.get(f"{tag}/lred{c}", (ops.LRELU_RED_SLOTS * c,), torch.float64)
        dzb = A.get(f"{tag}/dzb{j}", (n, h, w, c))
        ops.lrelu_bwd(g_b, c, rec["b"], c, dzb, c, self._acc[self._acc_off[i + 3]:], n * h * w, c, 0.0, red)
        ops.conv2d_wgrad(rec["ad"], None, 0, c, 0, dzb, c, self.grads[i + 2], n, h, w, c, c, c, 3, 1, 0, self._workspace(ops.conv2d_wgrad_workspace(n, h, w, c, c, 3)))
        g_ad = A.get(f"{tag}/gad{j}", (n, h, w, c))
        ops.conv2d_dgrad(dzb, c, self.vars[i + 2], g_ad, None, c, c, 0, n, h, w, c, c, 3, 1)
        g_a = A.get(f"{tag}/ga{j}", (n, h, w, c))
        ops.mul_mask(g_ad, rec["keep"], g_a, g_ad.numel(), 1.0 / (1.0 - DROP_RATES[j]))
        dza = A.get(f"{tag}/dza{j}", (n, h, w, c))
        ops.lrelu_bwd(g_a, c, rec["a"], c, dza, c, self._acc[self._acc_off[i + 1]:], n * h * w, c, 0.0, red)
        cin_p = _pad16(cin)
        # first layer (cin = 1): the input is read at its padded pitch of 16 and the one real row is stored
        ops.conv2d_wgrad(rec["x"], rec["x2"], rec["c1"], rec["ldx"], rec["ldx2"], dza, c, self.grads[i], n, h, w, cin, cin_p, c, 3, 1, 0,
                         self._workspace(ops.conv2d_wgrad_workspace(n, h, w, cin_p, c, 3)))
        if not need_dx:
            return None, None
        if rec["x2"] is None:
            dx = A.get(f"{tag}/gx{j}", (n, h, w, cin))
            ops.conv2d_dgrad(dza, c, self.vars[i], dx, None, cin, cin, 0, n, h, w, cin, c, 3, 1)
            return dx, None
        c1 = rec["c1"]
        dx = A.get(f"{tag}/gu{j}", (n, h, w, c1))
        dx2 = A.get(f"{tag}/gbn{rec['l']}", (n, h, w, cin - c1))           # the skip gradient: written here, the pool backward adds to it
        ops.conv2d_dgrad(dza, c, self.vars[i], dx, dx2, c1, c1, cin - c1, n, h, w, cin, c, 3, 1)
        return dx, dx2

    def backward(self, dz):
        """Backward of the last forward_train from dz = dloss/dlogits [n,H,W,1]: fills self.grad (flat, fp32, in the variable order of
        specseg_variables(); moving_mean / moving_variance get no gradient: their slices stay zero)."""
        T = self._tape
        assert T is not None, "backward() needs a forward_train() first"
        self._train_buffers()
        A, tag = self.arena, "specseg/train"
        n, H, W = T["n"], T["H"], T["W"]
        ops.zero(self._acc)
        hi = T["head"]
        c0 = WIDTHS[0]
        g = A.get(f"{tag}/ghead", (n, H, W, c0))
        ops.head_logit_bwd(T["last"], c0, self.vars[hi], dz, g, c0, self.grads[hi], self.grads[hi + 1], self._bn_ws(), n * H * W, c0)
        for rec in reversed(T["dec"]):
            gu, _ = self._pair_bwd(rec, g, True)
            ti, w, h, wd = rec["ti"], rec["cout"], rec["th"], rec["tw"]
            ws = self._workspace(ops.conv2d_transpose2x2_wgrad_workspace(n, h, wd, 2 * w, w))
            ops.conv2d_transpose2x2_wgrad(rec["tx"], 2 * w, gu, w, self.grads[ti], self.grads[ti + 1], ws, n, h, wd, 2 * w, w)
            name = f"{tag}/gbn4" if rec["l"] == 3 else f"{tag}/gdec{rec['l']}"
            g = A.get(name, (n, h, wd, 2 * w))
            ops.conv2d_transpose2x2_dgrad(gu, w, self.vars[ti], g, 2 * w, n, h, wd, 2 * w, w)
        gp = None                                  # gradient at the pool output below the current level
        for rec in reversed(T["enc"]):
            l, i, h, wd, w = rec["l"], rec["i"], rec["h"], rec["w"], rec["cout"]
            if l == 4:
                gc = g
            else:
                gc = A.get(f"{tag}/gbn{l}", (n, h, wd, w))
                ops.maxpool2_bwd(rec["bn"], w, gp, w, gc, w, n, h, wd, w, True)
            gb = A.get(f"{tag}/gb{l}", (n, h, wd, w))
            ops.bn_train_bwd(gc, w, rec["b"], w, self.vars[i + 4], rec["save"], gb, w, self.grads[i + 4], self.grads[i + 5], self._bn_ws(), n * h * wd, w)
            gp, _ = self._pair_bwd(rec, gb, l > 0)
        for i, off in self._acc_off.items():
            ops.cvt_f64_f32(self._acc[off:], self.grads[i], self.grads[i].numel(), 0)
        return self.grad

    def alpha(self, iterations):
        return ops.adam_alpha(self.lr0, self.beta_1, self.beta_2, iterations)

    def configure_optimizer(self, lr=None, beta1=None, beta2=None):
        if lr is not None:
            self.lr0 = float(lr)
        if beta1 is not None:
            self.beta_1 = float(beta1)
        if beta2 is not None:
            self.beta_2 = float(beta2)

    def _loss(self, z, mask, dz):
        out = torch.empty(len(ops.SEG_LOSS_NAMES), dtype=torch.float64, device=self.dev)
        ws = self.arena.get("specseg/train/lossws", (ops.SEG_LOSS_WS_DOUBLES,), torch.float64)
        ops.seg_loss(z, mask, dz, out, ws, z.numel())
        return out

    def _as_dev(self, a):
        if isinstance(a, np.ndarray):
            a = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))
        return a.to(self.dev, torch.float32).contiguous()

    def train_step(self, x, mask, *, seed=None, keep_masks=None):
        """One optimiser step on x [n,H,W,1] (the standardised Y plane) against mask [n,H,W,1] in [0,1].  seed: the Dropout masks'
        seed (default: this network's train_seed); the counter advances by one per step.  keep_masks: explicit masks instead (tests).
        Returns a LossRecord: {"loss", "dice", "focal", "iou", "f1"} read back from the device only when indexed."""
        x, mask = self._as_dev(x), self._as_dev(mask)
        assert x.shape == mask.shape, (x.shape, mask.shape)
        self._train_buffers()
        n, H, W = int(x.shape[0]), int(x.shape[1]), int(x.shape[2])
        if keep_masks is None:
            keep_masks = self.keep_masks(n, H, W, self.train_seed if seed is None else seed, self.train_counter)
        self.train_counter += 1
        z = self.forward_train(x, keep_masks)
        dz = self.arena.get("specseg/train/dz", (n, H, W, 1))
        out = self._loss(z, mask, dz)
        self.backward(dz)
        ops.adam(self.flat, self.m, self.v, self.grad, self.n, self.alpha(self.iterations), self.beta_1, self.beta_2, self.epsilon, 1.0, 0.0)
        self.iterations += 1
        self.weights_dirty = True
        return LossRecord(out)

    @staticmethod
    def _is_dataset(x):
        """A data.MaskDataset (anything with its batch(index, pass_index), len() and B)."""
        return hasattr(x, "batch") and hasattr(x, "B") and hasattr(x, "__len__") and not isinstance(x, (np.ndarray, torch.Tensor))

    def evaluate(self, x, y=None, batch_size=8):
        """Keras-shaped: the loss and metrics of `predict`'s network (inference mode: moving statistics, no Dropout) on x / y
        [N,H,W,1], the mean over the batches weighted by their size.  x may be a data.MaskDataset (then without y): its batches of
        pass 0, in its own batch size.  Returns {"loss", "dice", "focal", "iou", "f1"}."""
        if self._is_dataset(x):
            if y is not None:
                raise ValueError("evaluate(dataset): the masks come from the dataset; y must be None")
            batches = (x.batch(i, 0) for i in range(len(x)))
        else:
            if y is None:
                raise ValueError("evaluate(x, y) on tensors needs y")
            x, y = self._as_dev(x), self._as_dev(y)
            batches = ((x[b0:b0 + batch_size], y[b0:b0 + batch_size]) for b0 in range(0, int(x.shape[0]), batch_size))
        tot, N = torch.zeros(len(ops.SEG_LOSS_NAMES), dtype=torch.float64, device=self.dev), 0
        for xb, yb in batches:
            xb, yb = self._as_dev(xb), self._as_dev(yb)
            z = self._eval_logits(xb)
            tot += self._loss(z, yb, None) * xb.shape[0]
            N += int(xb.shape[0])
        r = (tot / N).cpu().numpy()
        return {k: float(r[j]) for j, k in enumerate(LOSS_KEYS)}

    def _eval_logits(self, x):
        """forward_plane up to the head, which gives the logit instead of its sigmoid."""
        n, H, W = int(x.shape[0]), int(x.shape[1]), int(x.shape[2])
        tag = "specseg/eval"
        self.forward_plane(x, 1, 0, n, tag=tag)
        i = len(self.vars) - 2
        last = self.arena.get(f"{tag}/c{i - 2}", (n, H, W, WIDTHS[0]))
        z = self.arena.get(f"{tag}/z", (n, H, W, 1))
        ops.head_logit_fwd(last, WIDTHS[0], self.vars[i], self.vars[i + 1], z, n * H * W, WIDTHS[0])
        return z

    def fit(self, x, y=None, batch_size=8, epochs=1, lr=None, beta1=None, beta2=None, shuffle=True, seed=None, print_fn=None,
            validation_data=None):
        """Keras-shaped training loop on x / y [N,H,W,1] (host arrays or device tensors).  The optimiser keeps its m, v and iterations
        across calls (save_npz / load_npz carry them).  shuffle draws the epoch's order from default_rng((seed, iterations)).
        x may be a data.MaskDataset (then without y): batch size, order and augmentation are the dataset's, `shuffle` is not read, and
        epoch e of the call is the dataset's pass first_pass + e with first_pass = iterations // len(dataset) (PolarDataset.first_pass's
        rule), so a resumed fit goes on with the next pass's order and draws.
        validation_data: an (xv, yv) pair or a MaskDataset; `evaluate` runs on it after every epoch (inference mode; the training
        weights are not touched) and its five values join the history as val_loss, val_dice, val_focal, val_iou and val_f1.
        Returns {"loss": [...], "dice": ..., "focal": ..., "iou": ..., "f1": ...}: per epoch, the mean over its steps."""
        dataset = x if self._is_dataset(x) else None
        if dataset is not None:
            if y is not None:
                raise ValueError("fit(dataset): the masks come from the dataset; y must be None")
            batch_size = int(dataset.B)
        else:
            if y is None:
                raise ValueError("fit(x, y) on tensors needs y")
            x, y = self._as_dev(x), self._as_dev(y)
            assert x.shape == y.shape and x.dim() == 4 and x.shape[3] == 1, (x.shape, y.shape)
        self.configure_optimizer(lr, beta1, beta2)
        self.trainable = True
        if seed is not None:
            self.train_seed = int(seed)
        hist = {k: [] for k in LOSS_KEYS}
        if validation_data is not None:
            hist.update({"val_" + k: [] for k in LOSS_KEYS})
        first_pass = self.iterations // len(dataset) if dataset is not None else 0
        for ep in range(int(epochs)):
            recs = []
            if dataset is not None:
                for i in range(len(dataset)):
                    xb, yb = dataset.batch(i, first_pass + ep)
                    recs.append((self.train_step(xb, yb), int(xb.shape[0])))
            else:
                N = int(x.shape[0])
                order = np.random.default_rng((self.train_seed, self.iterations)).permutation(N) if shuffle else np.arange(N)
                for b0 in range(0, N, batch_size):
                    idx = torch.from_numpy(order[b0:b0 + batch_size]).to(self.dev)
                    recs.append((self.train_step(x.index_select(0, idx), y.index_select(0, idx)), len(idx)))
            tot = sum(r.out * k for r, k in recs) / sum(k for _, k in recs)          # on the device; one read-back per epoch
            row = tot.cpu().numpy()
            for j, k in enumerate(LOSS_KEYS):
                hist[k].append(float(row[j]))
            if validation_data is not None:
                val = self.evaluate(validation_data) if self._is_dataset(validation_data) else self.evaluate(*validation_data, batch_size=batch_size)
                for k in LOSS_KEYS:
                    hist["val_" + k].append(val[k])
            if print_fn is not None:
                print_fn(f"SpecSeg epoch {ep + 1}/{epochs}: " + " ".join(f"{k} {v[-1]:.5f}" for k, v in hist.items()))
        return hist

    def optimizer_state(self):
        """{adam_m, adam_v, iterations, train_state} for save_npz, or None when the network was never trained."""
        if self.m is None:
            return None
        import json
        state = dict(train_counter=int(self.train_counter), train_seed=int(self.train_seed), lr0=self.lr0, beta_1=self.beta_1,
                     beta_2=self.beta_2, trainable=bool(self.trainable))
        return dict(adam_m=self.m.cpu().numpy(), adam_v=self.v.cpu().numpy(), iterations=np.int64(self.iterations),
                    train_state=np.array(json.dumps(state)))

    def set_optimizer_state(self, adam_m, adam_v, iterations, train_state=None):
        import json
        self._train_buffers()
        self.m.copy_(torch.as_tensor(np.asarray(adam_m, dtype=np.float32)).reshape(-1))
        self.v.copy_(torch.as_tensor(np.asarray(adam_v, dtype=np.float32)).reshape(-1))
        self.iterations = int(iterations)
        st = json.loads(str(train_state)) if train_state is not None else {}
        self.train_counter = int(st.get("train_counter", self.iterations))
        self.train_seed = int(st.get("train_seed", self.train_seed))
        self.lr0, self.beta_1, self.beta_2 = float(st.get("lr0", self.lr0)), float(st.get("beta_1", self.beta_1)), float(st.get("beta_2", self.beta_2))
        self.trainable = bool(st.get("trainable", True))

    def summary(self, print_fn=print):
        print_fn(f'Model: "{self.name}"')
        for (n, _, s), v in zip(self.spec, self.vars):
            print_fn(f"{n:40s} {tuple(s)}  {v.numel()}")
        nt = sum(v.numel() for (n, k, _), v in zip(self.spec, self.vars) if n.endswith(("moving_mean", "moving_variance")))
        print_fn(f"Total params: {self.n:,}")
        print_fn(f"Trainable params: {self.n - nt:,}")
        print_fn(f"Non-trainable params: {nt:,}")


class LossRecord:
    """The f64 device vector shm_seg_loss filled ({loss, dice, focal, iou, f1, tp, fp, fn}); indexing it by name reads it back
    (a host sync), nothing else does."""

    def __init__(self, out):
        self.out = out
        self._host = None

    def _read(self):
        if self._host is None:
            self._host = self.out.cpu().numpy()
        return self._host

    def __getitem__(self, key):
        return float(self._read()[ops.SEG_LOSS_NAMES.index(key)])

    def keys(self):
        return LOSS_KEYS

    def __iter__(self):
        return iter(LOSS_KEYS)

    def __len__(self):
        return len(LOSS_KEYS)

    def as_dict(self):
        return {k: self[k] for k in LOSS_KEYS}


def _pad16(c):
    return (c + 15) // 16 * 16
