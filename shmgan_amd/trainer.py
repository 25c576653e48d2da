"""Drop-in for the reference trainer object on MI355X.

`ShmGANwithSSpecSeg` mirrors the surface of /root/reference/ShmGANwithSSpecSeg.py:86-1309
that main.py / test.py use for the training hot path: `__init__(args)`, `build_generator()`,
`build_discriminator()`, `train_step(orig0, orig45, orig90, orig135, origED)`,
`custom_per_image_standardization`, `gram_matrix`, the `optimizer_G/D` iteration counters and
the loss / image attributes `train_step` leaves behind (SHM.py:467-875).

Semantics are the reference's "as executed" ones (SURVEY.md findings 3-7, oracle/step_torch.py
restates them): batch rule for B>1 = every sample is an independent B=1 reference step and
the loss is the mean over samples; the style-loss factor is explicit (`style_factor=`); RNG
draws default to fresh ones but can be injected (`draws=`) for parity tests.

One process drives one GPU.  Under torch.distributed (backend nccl = RCCL) every rank holds
a replica; gradients are summed with all-reduce on a side stream (D bucket overlapped with
the generator backward) and scaled by 1/world inside the clip+Adam kernel.
"""
from __future__ import annotations

import contextlib
import ctypes as C
import gc
import os
import time
from types import SimpleNamespace

import numpy as np
import torch

from . import checkpoint, dist, ops, validation
from .data import CAPTURE_OPTIONS, Augment, MaskDataset, capture_options, datasetLoad, gib_to_bytes
from .dist import GradReducer, exchange_active, world_size
from .model import Arena, Discriminator, Generator, WgradLane, check_image_hw, pad_channels
from .specseg import SpecSeg
from .telemetry import LOSS_NAMES, WEIGHT_SETS, NonFiniteGradientError, Telemetry, compose_losses, region_options, telemetry_options, validation_options  # noqa: F401


class _Optimizer:
    """Keras adam_v2.Adam(learning_rate=ExponentialDecay(lr0, 10000, 0.95)) bookkeeping
    (SHM.py:169-175); the update itself is shm_adam_clip."""

    def __init__(self, lr0, beta_1, beta_2, epsilon=1e-7):
        self.lr0, self.beta_1, self.beta_2, self.epsilon = lr0, beta_1, beta_2, epsilon

    def alpha(self, iterations):
        return ops.adam_alpha(self.lr0, self.beta_1, self.beta_2, iterations)

    def apply(self, P, gscale=1.0, abort=None):
        """abort: the ops.AbortWords of the step that made P.grad: no update while their device word is set."""
        ops.adam_clip(P.flat, P.m, P.v, P.grad, P.n, self.alpha(P.iterations), self.beta_1, self.beta_2,
                      self.epsilon, gscale, abort=abort)
        P.iterations += 1


_DEFAULTS = dict(image_size=128, image_hw=None, batch_size=1, filter_size=64, g_lr=0.00002, d_lr=0.00002, beta1=0.5, beta2=0.99,
                 c_dim=5, num_epochs=200, num_iteration_decay=100000, n_critic=5, d_repeat_num=6, mode="train",
                 data_dir="", model_save_dir="./models", checkpoint_save_dir="./checkpoints", result_dir="./results",
                 log_dir="./logs/train", log_step=1, checkpoint_save_step=10, calc_metrics=False, test_dir="", diffuse_dir="",
                 save_images=False, image_values="rescale", image_out_size="source", image_dir="", eval_size="model",
                 loss_log_step=0, histogram_step=0, nonfinite=None, diffuse_source="dir",
                 shuffle=False, data_seed=0, aug_flip_lr=0.0, aug_flip_ud=0.0, aug_crop_min=1.0, aug_views="physical",
                 cache="none", cache_gb=None,
                 capture_format="views", dofp_dir="DOFP", dofp_pattern="mono", dofp_quad_angles=(90, 45, 135, 0), dofp_bits=8,
                 dofp_demosaic="bilinear", dofp_test_view="total",
                 dofp_black=None, dofp_white=None, dofp_wb=None, dofp_ccm=None, dofp_tone=None, dofp_sat=None, dofp_calibration=None,
                 dofp_exposures=None, dofp_bracket_black=None, dofp_bracket_white=None,
                 specseg_image_dir="", specseg_mask_dir="", specseg_epochs=20, specseg_lr=1e-3, specseg_batch_size=8,
                 specseg_mask_source="dir", specseg_mask_threshold="otsu", specseg_mask_floor=16, specseg_mask_open=1,
                 specseg_mask_dilate=2,
                 specseg_aug_flip_lr=0.0, specseg_aug_flip_ud=0.0, specseg_aug_crop_min=1.0, specseg_aug_views="physical",
                 specseg_shuffle=False, specseg_data_seed=0, specseg_val_fraction=0.0, specseg_cache_gb=None,
                 ema_decay=0.0, ema_warmup=True,
                 val_dir="", val_fraction=0.0, val_seed=0, val_step=1, val_batch_size=None, val_monitor="psnr",
                 val_region="off", val_region_threshold=None, metrics_region="off", region_threshold=None,
                 eval_weights="raw", eval_checkpoint="latest", image_detail="off", detail_radius=2, detail_eps=1e-2)

SPECSEG_MASK_SOURCES = ("dir", "polar")                   # where train_specseg's masks come from


class KernelAbortError(RuntimeError):
    """A kernel of an earlier step gave up (a barrier of the one-pass InstanceNorm backward timed out) and went on with wrong numbers.
    The optimizer kernels refused every update from that moment on (the arena's abort words), so the weights are those of the last good
    step; the run must not continue."""


_DTYPES = {"float32": torch.float32, "fp32": torch.float32, "f32": torch.float32,
           "bfloat16": torch.bfloat16, "bf16": torch.bfloat16}


class ShmGANwithSSpecSeg:
    def __init__(self, args=None, device=None, compute_dtype="float32", grad_dtype=None, attention="executed",
                 xent_mode="executed", **overrides):
        """compute_dtype: "float32" (the reference's precision: exact-fp32 MFMA) or "bfloat16" (BASELINE
        configs 4-5: activations and MFMA operands in bf16, fp32 accumulation, fp32 master weights,
        statistics, losses, weight gradients and Adam).
        attention: "executed" (default) = the graph the reference runs: attention_layer is evaluated once on a constant zero
        mask at build time, so the skips get + 0 (SURVEY finding 3); "live" = the architecture as intended: every step's
        SpecSeg mask goes through attention_layer (MaxPool -> 2 x Conv3x3 + LeakyReLU, SHM.py:404-412) into the four
        generator skips (SHM.py:290-293) and the discriminator (SHM.py:359), its 10 convolutions are trained.
        image_hw = (H, W) (keyword or args.image_hw; default None = (image_size, image_size)): the frame the GAN trains, validates
        and runs model-size test mode on; H and W multiples of 32, at least 32 (model.check_image_hw).  `image_size` keeps its
        meaning for what stays square: the mask network's own training."""
        assert attention in ("executed", "live")
        self.attention = attention
        # "executed" (default): the classification-loss gradient as TensorFlow computes it -- the fused
        # softmax_cross_entropy_with_logits kernel hands back softmax - labels, which for D1's un-normalised label row
        # [0,0,0,0,TARGET_LABELS] (SHM.py:477, 688, 702) is not the derivative (SURVEY-style finding 8);
        # "intended": the true derivative TARGET_LABELS * (softmax - onehot).  Loss values do not depend on the mode.
        assert xent_mode in ("executed", "intended")
        self.xent_mode = xent_mode
        self.compute_dtype = _DTYPES[compute_dtype] if isinstance(compute_dtype, str) else compute_dtype
        # gradient-signal tensors between an input-gradient product and the next IN/LeakyReLU backward:
        # default = compute_dtype; "float32" with bf16 compute selects SHM_BF16_GF32 (include/shmgan_hip.h)
        self.grad_dtype = _DTYPES[grad_dtype] if isinstance(grad_dtype, str) else (grad_dtype or self.compute_dtype)
        if self.compute_dtype == torch.float32:
            self.grad_dtype = torch.float32
        self.pad = pad_channels(self.compute_dtype)
        a = dict(_DEFAULTS)
        if args is not None:
            a.update({k: v for k, v in vars(args).items()})
        a.update(overrides)
        self.args = SimpleNamespace(**a)
        for k in ("c_dim", "image_size", "batch_size", "num_epochs", "num_iteration_decay", "g_lr", "d_lr", "n_critic",
                  "beta1", "beta2", "d_repeat_num", "mode", "data_dir", "model_save_dir", "checkpoint_save_dir",
                  "result_dir", "log_dir", "log_step", "checkpoint_save_step", "filter_size"):
            setattr(self, k, a[k])
        self._image_hw = check_image_hw(a["image_hw"])       # None, or the checked pair
        # SHM.py:157-212
        self.seed, self.randomness, self.dropout_amnt = 25, 0.50, 0.2
        self.TARGET_LABELS = 0.90
        self.c_dim = 5
        self.epoch, self.train_G_after = 0, 0
        self.stddev_arr, self.mean_arr, self.variance_arr = [], [], []
        if device is None:
            if not torch.cuda.is_available():
                raise RuntimeError("shmgan_amd needs an MI355X (ROCm) device: there is no CPU path")
            device = torch.device("cuda", torch.cuda.current_device())
        self.device = torch.device(device)
        # both optimisers use the schedule built from g_lr (SHM.py:169-174; d_lr is unused there)
        self.optimizer_G = _Optimizer(self.g_lr, self.beta1, self.beta2)
        self.optimizer_D = _Optimizer(self.g_lr, self.beta1, self.beta2)
        # the arena also owns the abort words (ops.AbortWords): a device word the optimizer kernel checks before it touches the weights, and a
        # word in pinned host memory the host polls without synchronising (_check_abort)
        self.arena = Arena(self.device)
        self._ws = None
        self._lane = None
        self.G = self.D = self.SpecSeg = None
        self.specseg_datasets = None             # (train, val) of the last train_specseg that ran with loader options or a split
        # zeros at graph-build time (SHM.py:206; the attention convs only ever see this constant, finding 3);
        # train_step overwrites it with SpecSeg.predict(I90_Ych) (SHM.py:492), which feeds Spec_loss only
        self.specular_candidate = None
        self._rng = np.random.default_rng(self.seed)
        self._draw_count = 0
        self._reducer = GradReducer(self.device)
        self._prefetched = None          # _prologue() of the next batch, issued by train_step(next_batch=)
        self._loss_cache = None
        # held-out validation inside train() (off by default): the loader datasetLoad made, whether train() validates, the best monitored
        # value so far {"monitor", "weights", "value", "step"} and the step of the last validation; whether the last checkpoint that was
        # loaded held an average of the generator's weights
        self.valDataset, self._val_on, self._best, self._last_val_step, self._loaded_ema = None, False, None, None, False
        # train(): the validation options, this rank's dataset length, train_step calls so far, the per-step flip draw (inert, SHM.py:983)
        self._val_region = None          # train()'s val_region / val_region_threshold, checked: None or (source, threshold)
        self._val_step, self._val_monitor, self.length_dataset, self.batch_step, self.random_flip = None, None, 0, 0, 0.0
        # the last train_step's loss vectors and inputs (losses()), the frame (H, W) of the last infer(), _stats_now's Telemetry without files
        self._last = self._inf_frame = self._adhoc_telemetry = None
        self._inf_planes = None          # the last infer()'s (standardised yuv, gen_Y, scale): what refine() fits its coefficients on
        # evaluate_frame's split of the metrics by the highlight (off by default): None, ("residual", tau) = photo - diffuse above tau, or
        # ("specseg", tau) = the inference's SpecSeg mask above tau; with it on and a diffuse target given, evaluate_frame leaves the region
        # (uint8 [B,h,w]) and the split metrics (float64 [B,12], ops.REGION_METRIC_NAMES) of its last call here
        self.eval_region = self.highlight_region = self.region_metrics = self._inf_photo = None
        # test diagnostics: called with no arguments between the last forward pass and the first backward kernel of a step
        # (tests/test_step_gpu.py pins LeakyReLU signs there; never set on the hot path)
        self.before_backward = None
        # training telemetry (telemetry.py): None = off, the default; start_telemetry() / train() create it
        self.telemetry = None
        # the D-loss backward on the second stream (train_step): measured on one box, A/B by the variable, bf16 22.48 -> 22.25 ms, S = 512 B = 4
        # 42.79 -> 42.58, B = 32 79.3 -> 78.6; fp32 114.2 -> 114.2 (MFMA bound either way) -- default on in bf16, off in fp32
        self.d_fwd_on_lane = os.environ.get("SHM_D_FWD_LANE", "1" if self.compute_dtype != torch.float32 else "0") == "1"
        self.img_loss_on_lane = os.environ.get("SHM_IMG_LOSS_LANE", "1" if self.compute_dtype != torch.float32 else "0") == "1"
        self.d_bwd_on_lane = os.environ.get("SHM_D_BWD_LANE", "1" if self.compute_dtype != torch.float32 else "0") == "1"
        self.style_factor = self._default_style_factor()   # as intended (finding 7)

    def _default_style_factor(self):
        return 1.0 / float(2 * 9 * self.image_hw[0] * self.image_hw[1]) ** 2

    @property
    def image_hw(self):
        """The GAN's frame (H, W), always a pair: the image_hw option, or (image_size, image_size) without it."""
        return self._image_hw if self._image_hw is not None else (self.image_size, self.image_size)

    def frame_arg(self):
        """What the loaders and the models are given as the frame: the side without the image_hw option, the pair with it."""
        return self.image_size if self._image_hw is None else self._image_hw

    # ------------------------------------------------------------------ workspace
    def _workspace(self, nbytes):
        """Split-K slab workspace of the wgrad launches (they run in order on one stream)."""
        n = (nbytes + 3) // 4
        if self._ws is None or self._ws.numel() < n:
            # 128 MiB covers every layer at S=256/B=8; growing mid-step would hand memory still in
            # use on the wgrad lane back to the allocator, hence the join before re-allocating
            if self._lane is not None:
                self._lane.join()
                torch.cuda.current_stream().synchronize()
            self._ws = torch.empty(max(n, 32 << 20), dtype=torch.float32, device=self.device)
        return self._ws

    def _check_abort(self, sync=False):
        """Raise KernelAbortError if a kernel of this trainer gave up.  Without `sync` this is one read of host memory (the kernel
        wrote the pinned word itself), so it costs the step nothing; it sees every abort whose kernel has finished -- the host runs
        ahead of the device, so an abort of step t may only be seen at the top of step t + 2, and the device-side check in
        shm_adam_clip is what keeps the weights clean in between.  sync=True (losses(), checkpoints, release()) waits for the device
        first and is exact."""
        if self.arena.abort is None:
            return
        if self.arena.abort.tripped(sync):
            names = self.arena.fused_timeouts()
            raise KernelAbortError(
                f"in_bwd_fused8_kernel: a group barrier timed out (scratch {names or 'unknown'}): the step's gradients are built on "
                "unfinished sums.  No optimizer update has been applied since (shm_adam_clip checks the abort word on the device); "
                "the weights are those of the last good step.  Set SHM_ELEM_FUSED_BWD=0 (two-pass InstanceNorm backward) and report; "
                "clear_abort() clears the words")

    def clear_abort(self):
        """Clear the abort words (after a KernelAbortError, once its cause is dealt with)."""
        self.arena.abort.clear()
        self.arena.fused_timeouts()
        torch.cuda.synchronize(self.device)

    def release(self):
        """Drop every device buffer this trainer holds (arena, split-K workspace, both models and their optimizer state) so that
        another trainer can be built in the same process (bench.py's extra configurations); the object is unusable afterwards.
        Raises KernelAbortError (after releasing) if a kernel of this trainer gave up and nobody has heard of it yet."""
        if self._lane is not None:
            self._lane.join()
        torch.cuda.synchronize(self.device)
        try:
            self.stop_telemetry()        # flushes the logs and ends the writer thread; a writer's error is raised after the buffers are gone
        finally:
            self._release_buffers()

    def _release_buffers(self):
        aborted = self.arena.abort is not None and self.arena.abort.tripped(sync=True)
        self.arena.abort = None
        self.arena.t.clear()
        self._ws = self._prefetched = self._loss_cache = self.valDataset = self._adhoc_telemetry = None
        self.G = self.D = self.SpecSeg = None
        self.specular_candidate = None
        if aborted:
            raise KernelAbortError("in_bwd_fused8_kernel: a group barrier timed out during this trainer's last steps (seen at release())")

    # ------------------------------------------------------------------ telemetry
    def start_telemetry(self, log_dir=None, loss_log_step=None, histogram_step=None, nonfinite=None):
        """Create this trainer's Telemetry (telemetry.py) from the given options, each defaulting to the trainer's `args`
        (loss_log_step, histogram_step, nonfinite, log_dir).  With both step options 0 nothing is logged by train_step, but
        grad_stats() / weight_stats() and manual recording work.  Returns it; a running one is flushed and replaced."""
        if self.G is None:
            self.build()
        self.stop_telemetry()
        a = self.args
        self.telemetry = Telemetry(self, log_dir=self.log_dir if log_dir is None else log_dir,
                                   loss_log_step=a.loss_log_step if loss_log_step is None else loss_log_step,
                                   histogram_step=a.histogram_step if histogram_step is None else histogram_step,
                                   nonfinite=a.nonfinite if nonfinite is None else nonfinite)
        return self.telemetry

    def stop_telemetry(self):
        """Flush the logs and stop the writer thread (release() calls it)."""
        tel, self.telemetry = self.telemetry, None
        if tel is not None:
            tel.close()

    def _stats_now(self, kind, scale):
        tel = self.telemetry
        if tel is None:                  # interactive use without logging: a Telemetry with no writer thread and no files
            tel = self._adhoc_telemetry = self._adhoc_telemetry or Telemetry(self, log_dir=None)
        return tel.stats_now(kind, scale)

    def grad_stats(self):
        """{variable name: {"stats", "hist", "shape"}} of the last step's gradients times 1 / world, the values the optimizer
        clips, as numpy (ops.tensor_stats; names are the save_npz keys G/var00.., D/var00..).  Synchronises: interactive use,
        train_step never calls it."""
        return self._stats_now("gradients", 1.0 / self._world())

    def weight_stats(self):
        """The same of the current weights."""
        return self._stats_now("weights", 1.0)

    def _get_lane(self):
        if self._lane is None:
            self._lane = WgradLane(self.device, enabled=os.environ.get("SHM_NO_WGRAD_LANE") is None)
        return self._lane

    # ------------------------------------------------------------------ builders
    def build_generator(self):
        """SHM.py:228-327."""
        return Generator(self.frame_arg(), self.filter_size, self.device, self.arena, self._workspace, self._get_lane(),
                         dtype=self.compute_dtype, grad_dtype=self.grad_dtype, attention=self.attention == "live")

    def build_discriminator(self):
        """SHM.py:343-380."""
        return Discriminator(self.frame_arg(), self.filter_size, self.device, self.arena, self._workspace,
                             self.dropout_amnt, self._get_lane(), dtype=self.compute_dtype, grad_dtype=self.grad_dtype,
                             attention=self.attention == "live")

    def build_specseg(self):
        """SHM.py:930-931: SpecSeg(image_size, image_size, 1) then load_model('specsegv3_chkpt.h5').  The
        checkpoint is not available, so the network starts from the initialisers of SpecSeg.py; load trained
        Keras weights with `self.SpecSeg.set_weights(keras_model.get_weights())`."""
        return SpecSeg(self.image_size, self.device, self.arena).init_random()

    def train_specseg(self, args=None, *, print_fn=print):
        """Train the mask network in place on a directory of image / mask pairs (data.MaskDataset): args.specseg_image_dir,
        args.specseg_mask_dir, args.specseg_epochs, args.specseg_lr (and specseg_batch_size), defaults from the trainer's own
        options.  The reference builds this optimiser (SHM.py:175) and never steps it; its checkpoint is not available, so this is
        how the weights every Spec_loss, live-attention step and test-mode image depends on are made.  Adam runs on the schedule of
        optimizer_G with the trainer's beta1 / beta2; the five scalars are logged per epoch through print_fn.  G and D are not
        touched; the next train_step / infer uses the trained network.  Returns fit()'s history.
        args.specseg_mask_source = "polar" needs neither directory: the pairs come from the raw capture under data_dir
        (data.MaskDataset.from_polar: view 2 as the image, polar.specular_mask of the four views as its mask), with
        args.specseg_mask_threshold / specseg_mask_floor / specseg_mask_open / specseg_mask_dilate as the mask's options.
        The loader options of specseg_dataset (augmentation, shuffle, seed, cache) and specseg_val_fraction apply to both sources: with
        any of them set the network is fitted on the dataset itself (SpecSeg.fit(dataset): one ops.augment_pairs_u8 call per
        batch), and a fraction above 0 holds that part of the names out (MaskDataset.split with specseg_data_seed) and reports
        val_loss ... val_f1 per epoch; `specseg_datasets` then holds (train, val).  With all of them at their defaults the path is
        tensors(), then fit(x, y)."""
        opt = self._specseg_opt(args)
        ds = self.specseg_dataset(args)
        if self.SpecSeg is None:
            self.SpecSeg = self.build_specseg()
        fit = dict(epochs=int(opt("specseg_epochs")), lr=float(opt("specseg_lr")), beta1=self.beta1, beta2=self.beta2, print_fn=print_fn)
        val_fraction = float(opt("specseg_val_fraction"))
        if not ds.active and val_fraction == 0.0:         # no loader option set: the whole set as two tensors, shuffled by fit
            x, y = ds.tensors()
            return self.SpecSeg.fit(x, y, batch_size=ds.B, shuffle=True, **fit)
        train, val = ds.split(val_fraction, seed=int(opt("specseg_data_seed"))) if val_fraction != 0.0 else (ds, None)
        self.specseg_datasets = (train, val)
        if not train.active:                              # a split alone: the training side as tensors, as above
            x, y = train.tensors()
            return self.SpecSeg.fit(x, y, batch_size=train.B, shuffle=True, validation_data=val, **fit)
        return self.SpecSeg.fit(train, validation_data=val, **fit)

    def specseg_dataset(self, args=None):
        """The data.MaskDataset train_specseg trains on, before any split: the source (specseg_mask_source and its directories or
        mask options) with the loader options specseg_aug_flip_lr / specseg_aug_flip_ud / specseg_aug_crop_min / specseg_aug_views
        (an Augment when any draw is asked for), specseg_shuffle, specseg_data_seed and specseg_cache_gb (GiB of device memory for
        the decoded pairs; None = half of what is free).  All at their defaults: a dataset without loader options."""
        opt = self._specseg_opt(args)
        source = opt("specseg_mask_source")
        if source not in SPECSEG_MASK_SOURCES:
            raise ValueError(f"train_specseg: specseg_mask_source {source!r} is not one of {SPECSEG_MASK_SOURCES}")
        draws = (float(opt("specseg_aug_flip_lr")), float(opt("specseg_aug_flip_ud")), float(opt("specseg_aug_crop_min")))
        loader = dict(augment=Augment(*draws, views=opt("specseg_aug_views")) if draws != (0.0, 0.0, 1.0) else None,
                      shuffle=bool(opt("specseg_shuffle")), seed=int(opt("specseg_data_seed")),
                      cache_bytes=gib_to_bytes(opt("specseg_cache_gb")))
        if source == "polar":
            return self._polar_mask_dataset(opt, **loader)
        idir, mdir = opt("specseg_image_dir"), opt("specseg_mask_dir")
        if not idir or not mdir:
            raise ValueError("train_specseg needs specseg_image_dir and specseg_mask_dir")
        return MaskDataset(idir, mdir, self.image_size, int(opt("specseg_batch_size")), device=self.device, **loader)

    def _specseg_opt(self, args):
        """Option lookup of train_specseg / evaluate_specseg: `args` first, then the trainer's own options."""
        return lambda k: getattr(args, k, None) if args is not None and getattr(args, k, None) is not None else getattr(self.args, k)

    def _polar_mask_dataset(self, opt, **loader):
        data_dir = opt("data_dir")
        if not data_dir:
            raise ValueError("specseg_mask_source='polar' needs data_dir: the capture's four view directories")
        subdirs, capture = capture_options(SimpleNamespace(**{k: opt(k) for k in CAPTURE_OPTIONS}))
        return MaskDataset.from_polar(data_dir, self.image_size, int(opt("specseg_batch_size")), subdirs=subdirs, device=self.device, **capture,
                                      threshold=opt("specseg_mask_threshold"), floor=int(opt("specseg_mask_floor")),
                                      open_radius=int(opt("specseg_mask_open")), dilate_radius=int(opt("specseg_mask_dilate")), **loader)

    def evaluate_specseg(self, args=None):
        """Score the current mask network against the polar masks of a capture (args.data_dir or the trainer's; the mask options of
        train_specseg): has the network learnt what the polariser sees?  Inference mode, through SpecSeg.evaluate.  Returns
        {"loss", "dice", "focal", "iou", "f1"}."""
        opt = self._specseg_opt(args)
        ds = self._polar_mask_dataset(opt)
        if self.SpecSeg is None:
            self.SpecSeg = self.build_specseg()
        x, y = ds.tensors()
        return self.SpecSeg.evaluate(x, y, batch_size=ds.B)

    def build(self, seed=42, beta_seed=43, attention_seed=45):
        """Build G, D and SpecSeg and give G/D the synthetic init of SURVEY 8(d): weights N(0,0.02) from
        default_rng(seed) (RandomNormal(0,0.02), SHM.py:200), biases 0, IN beta N(0,0.02); the live attention branch's
        kernels N(0,0.02) from default_rng(attention_seed), generator levels first, then the discriminator's."""
        # A trainer is a web of reference cycles (closures over it, records of full-batch tensors), so a dropped trainer keeps its device
        # buffers until Python's cycle collector happens to run.  A process that builds one trainer after another (bench.py's extra
        # configurations, a test session) can pile up hundreds of GiB of dead arenas that way: collect before allocating the next one.
        gc.collect()
        self.G = self.build_generator()
        self.D = self.build_discriminator()
        if self.SpecSeg is None:
            self.SpecSeg = self.build_specseg()
        rng = np.random.default_rng(seed)
        ng, nd = 2 * len(self.G.layers), 7
        gw = [np.zeros(s, np.float32) if len(s) == 1 else rng.normal(0.0, 0.02, s).astype(np.float32)
              for s in self.G.P.shapes[:ng]]
        dw = [rng.normal(0.0, 0.02, s).astype(np.float32) for s in self.D.P.shapes[:nd]]
        if self.attention == "live":
            arng = np.random.default_rng(attention_seed)
            ga = [(arng.normal(0.0, 0.02, s) if len(s) == 4 else np.zeros(s)).astype(np.float32) for s in self.G.P.shapes[ng:]]
            da = [(arng.normal(0.0, 0.02, s) if len(s) == 4 else np.zeros(s)).astype(np.float32) for s in self.D.P.shapes[nd:]]
            self.G.P.load(gw + ga)
            self.D.P.load(dw + da)
            self.G.weights_dirty = self.D.weights_dirty = True
            gw = dw = None
        brng = np.random.default_rng(beta_seed)
        gb = [brng.normal(0.0, 0.02, (c,)).astype(np.float32) for c in self.G.in_channels]
        db = [brng.normal(0.0, 0.02, (c,)).astype(np.float32) for c in self.D.chan[1:]]
        if gw is not None:
            self.G.set_weights(gw)
            self.D.set_weights(dw)
        self.G.set_betas(gb)
        self.D.set_betas(db)
        return self

    # ------------------------------------------------------------------ small reference helpers
    def custom_per_image_standardization(self, image):
        """SHM.py:1271-1309 on an already-YUV [B,S,S,3] tensor: x / max(std, 1/256), statistics
        per sample, no mean subtraction.  API-parity helper for test.py:218 (off the hot path, plain
        tensor arithmetic); train_step uses the fused rgb->yuv+standardise kernels (`preprocess`)."""
        x = self._dev(image)
        m = x.mean(dim=(1, 2, 3))
        var = torch.relu((x * x).mean(dim=(1, 2, 3)) - m * m)
        scale = torch.clamp(torch.sqrt(var), min=1.0 / 256.0)
        self.stddev_arr = list(scale)
        return x / scale.view(-1, 1, 1, 1)

    def preprocess(self, rgb, name):
        """tf.image.rgb_to_yuv + custom_per_image_standardization (SHM.py:480-484, 1271-1309)."""
        B, H, W = (int(v) for v in rgb.shape[:3])            # the frame is the input's: (S, S) in training, any frame in inference
        yuv = self.arena.get(f"pre/yuv/{name}", (B, H, W, 3))
        acc = self.arena.get(f"pre/acc/{name}", (B * 2,), torch.float64)
        scale = self.arena.get(f"pre/scale/{name}", (B,))
        ops.rgb2yuv_std(rgb, yuv, acc, scale, B, H * W)
        return yuv, scale

    def _prologue(self, orig, slot):
        """The weight-independent head of a step (SHM.py:480-505 + the SpecSeg.predict of SHM.py:492): rgb->yuv +
        standardisation of the five views, the CbCr average and the specular mask (on the second stream).  Nothing here
        reads G's or D's weights, so train_step(next_batch=) issues it for step t+1 while step t's last gradient bucket is
        still being all-reduced ("the next batch's weight-independent prologue"); buffers are double-buffered
        by `slot`."""
        A, (H, W) = self.arena, self.image_hw
        B = orig[0].shape[0]
        ds, scales = [], []
        for k in range(5):
            y, sc = self.preprocess(orig[k], f"{k}/s{slot}")
            ds.append(y)
            scales.append(sc)
        cbcr = A.get(f"pre/cbcr/s{slot}", (B, H, W, 2))
        ops.avg_cbcr(ds, cbcr, B * H * W)
        # specular mask: nothing on the gradient path reads it, so it runs on the second stream beside the generator forward
        lane = self._get_lane()
        if self.SpecSeg is None:
            self.SpecSeg = self.build_specseg()
        box = {}
        lane.submit(lambda: box.__setitem__("mask", self.SpecSeg.forward_plane(ds[2], 3, 0, B, tag=f"specseg/step{slot}")))
        return SimpleNamespace(slot=slot, key=tuple((t.data_ptr(), tuple(t.shape)) for t in orig), orig=orig, ds=ds,
                               scales=scales, cbcr=cbcr, mask=box["mask"])

    def calcDOP(self, I0_Ych, I45_Ych, I90_Ych, I135_Ych):
        """SHM.py:1157-1169: the degree-of-polarisation map of four views taken at 0 / 45 / 90 / 135 degrees (any shape: the Y
        channels, as the reference names them, or whole RGB views), with the reference's coefficients S0 = I0 + I90,
        S1 = I0 - I90, S2 = I45 - I135 and divide_no_nan -- on the device (shm_polar_maps).  Dead code in the reference (nothing
        calls it, and its plot_single_image side effect is not reproduced); `polar_maps` is the general form."""
        from .polar import REFERENCE_DOP_MATRIX
        views = [self._dev(t) for t in (I0_Ych, I45_Ych, I90_Ych, I135_Ych)]
        return ops.polar_maps(views, REFERENCE_DOP_MATRIX, ("dop",))["dop"]

    def polar_maps(self, views, angles, want=("s0", "dop", "aolp")):
        """{"s0", "dop", "aolp"} maps of four views taken at `angles` (degrees), through the least-squares Stokes matrix of
        polar.stokes_matrix(angles): S0, sqrt(S1^2 + S2^2) / S0 (0 where S0 == 0) and 0.5 atan2(S2, S1) per element."""
        from .polar import stokes_matrix
        return ops.polar_maps([self._dev(t) for t in views], stokes_matrix(angles), want)

    def gram_matrix(self, x):
        """SHM.py:1176-1180 (host-side convenience on a torch tensor; not on the hot path)."""
        return torch.einsum('bijc,bijd->bcd', x, x) / float(x.shape[1] * x.shape[2])

    # ------------------------------------------------------------------ draws
    def _default_draws(self, B):
        """Fresh draws of a step: the five RNG flags (SHM.py:509-513) on the host; GaussianNoise(0.1) for the D1 / D2 inputs
        (SHM.py:352) and the Dropout keep mask (SHM.py:363) on the device (shm_randn / shm_keep_mask: Philox keyed by the
        trainer's seed, the step counter and the rank, so replicas draw different noise and agree on the flags)."""
        H, W = self.image_hw
        flags = tuple(bool(u < self.randomness) for u in self._rng.random(5))
        noise = self.arena.get("draws/noise", (2 * B, H, W, 3))
        keep = self.arena.get("draws/keep", (2 * B, H // 32, W // 32, 16 * self.filter_size))
        self._draw_count += 1
        seed = (self.seed << 32) | (self._draw_count & 0xFFFFFFFF)
        ops.randn(noise, 0.1, seed, 2 * dist.rank())
        ops.keep_mask(keep, self.dropout_amnt, seed, 2 * dist.rank() + 1)
        return SimpleNamespace(flags=flags, target_label=float(self.TARGET_LABELS), noise=noise, keep_mask=keep)

    def _dev(self, t):
        if isinstance(t, np.ndarray):
            t = torch.from_numpy(np.ascontiguousarray(t, dtype=np.float32))
        return t.to(self.device, torch.float32).contiguous()

    # ------------------------------------------------------------------ data parallel
    def _world(self):
        return world_size()

    def _allreduce_async(self, flat, after=None, tag="g"):
        """Sum `flat` over ranks on the side stream; returns an event to wait on (or None)."""
        return self._reducer.allreduce_async(flat, after, tag)

    # ------------------------------------------------------------------ average of the generator's weights
    def _ema_on(self):
        return float(self.args.ema_decay or 0.0) > 0.0

    def _ensure_ema(self):
        """With `ema_decay` > 0: G.P.ema, a flat fp32 buffer beside G.P.flat that averages every variable optimizer_G updates (the live
        attention branch's included; the InstanceNorm betas are constants and have none).  Made when the option is first seen on, or
        after a checkpoint without an average was loaded, as a copy of the current weights (a decay = 0 call) with the counter at 0."""
        P = self.G.P
        if P.ema is None:
            ops.ema_decay_at(self.args.ema_decay, 0)           # the option, checked before anything is allocated
            P.ema = torch.empty_like(P.flat)
            ops.ema_update(P.ema, P.flat, P.n, 0.0)
            P.ema_updates = 0
        return P.ema

    @contextlib.contextmanager
    def generator_weights(self, which="raw"):
        """with shmgan.generator_weights("ema"): infer / evaluate / validate inside run on the average of the generator's weights.  The
        raw weights move to a spare buffer, the average is copied into G.P.flat and the weights are marked dirty, so that the next
        prepare_weights redoes the tap transposes and the bf16 operand copy; on exit -- after an exception too -- the raw weights come
        back bit for bit and are marked dirty again.  Not for use around train_step.  "raw" changes nothing; "ema" without an average
        (ema_decay off and none loaded) raises ValueError."""
        if which not in WEIGHT_SETS:
            raise ValueError(f"generator_weights: {which!r} is not one of {WEIGHT_SETS}")
        if which == "raw":
            yield self
            return
        if self.G is None:
            self.build()
        P = self.G.P
        if P.ema is None and self._ema_on():
            self._ensure_ema()
        if P.ema is None:
            raise ValueError("generator_weights('ema'): this trainer holds no average of the generator's weights (ema_decay is 0 and no "
                             "checkpoint with one has been loaded)")
        if P.spare is None:
            P.spare = torch.empty_like(P.flat)
        self._get_lane().join()                      # nothing queued on the second stream may still read the raw weights
        P.spare.copy_(P.flat)
        P.flat.copy_(P.ema)
        self.G.weights_dirty = True
        try:
            yield self
        finally:
            P.flat.copy_(P.spare)
            self.G.weights_dirty = True

    def ema_weights(self):
        """The average of the generator's weights as host arrays in Keras variable order, like G.get_weights().  Synchronises."""
        if self.G is None or self.G.P.ema is None:
            raise ValueError("ema_weights: this trainer holds no average of the generator's weights (ema_decay is 0 and no checkpoint "
                             "with one has been loaded)")
        P = self.G.P
        flat = P.ema.cpu().numpy()
        w = [flat[o:o + int(np.prod(s))].reshape(s).copy() for o, s in zip(P.offsets, P.shapes)]
        return [w[i] for i in self.G._korder()]

    # ------------------------------------------------------------------ the step
    def train_step(self, orig0, orig45, orig90, orig135, origED, *, draws=None, style_factor=None, apply=True, next_batch=None):
        """One SHM.py:467-875 step: D update + G update from a 5-view batch [B,H,W,3] in [0,1] on the trainer's frame (image_hw).
        next_batch: the five tensors of the FOLLOWING step (or a callable returning them, called late in this step's issue
        order; None when it returns None): their weight-independent prologue (_prologue) is issued before this step waits
        for its last gradient collective, and the next train_step on those same tensors (same storage, not modified in
        between) picks the result up instead of recomputing it."""
        if self.G is None:
            self.build()
        self._check_abort()              # an earlier step's kernel gave up: stop here, before anything else is issued
        if self.telemetry is not None:
            self.telemetry.check()       # non-finite gradients in a histogram that has reached the host (nonfinite="raise" / "warn")
        G, D, A = self.G, self.D, self.arena
        (H, W), F = self.image_hw, self.filter_size
        if self._ema_on():
            self._ensure_ema()           # first step with the option on (or behind a checkpoint without an average): the average starts as these weights
        orig = [self._dev(t) for t in (orig0, orig45, orig90, orig135, origED)]
        B = orig[0].shape[0]
        if tuple(orig[0].shape[1:3]) != (H, W):
            raise ValueError(f"train_step takes [B,{H},{W},3] views (the trainer's frame), got {tuple(orig[0].shape)}")
        npix = H * W
        if draws is None:
            draws = self._default_draws(B)
        flags = [bool(f) for f in draws.flags]
        fmask = sum(1 << k for k in range(5) if flags[k])
        T = float(draws.target_label)
        noise = self._dev(draws.noise)
        keep = self._dev(draws.keep_mask)
        sf = float(self.style_factor if style_factor is None else style_factor)
        world = self._world()

        G.zero_grad()
        D.zero_grad()
        G.prepare_weights()
        D.prepare_weights()

        # ---- pre-processing (outside the tape, SHM.py:480-505) and the specular mask SpecSeg.predict(I90_Ych) (SHM.py:492):
        # taken from the previous step's look-ahead when it was given these tensors, issued here otherwise
        lane = self._get_lane()
        pro, self._prefetched = self._prefetched, None
        if pro is None or pro.key != tuple((t.data_ptr(), tuple(t.shape)) for t in orig):
            pro = self._prologue(orig, 0 if pro is None else pro.slot)
        ds, scales, cbcr = pro.ds, pro.scales, pro.cbcr
        self.specular_candidate = pro.mask

        # ---- live attention branch: the maps of this step's mask, shared by the six G calls and the twelve D calls
        attn_g = attn_d = None
        if self.attention == "live":
            lane.join()                                    # the mask comes from the second stream
            attn_g = G.attention_forward(self.specular_candidate, B)
            attn_d = D.attention_forward(self.specular_candidate, B)

        adt, PAD_C = self.compute_dtype, self.pad
        # D batch layout: [D1: B][D3: 5B][D2: B][D4: 5B]
        xd = A.get_slack("d/x16", (12 * B, H, W, D.in_pitch), adt, D.pad)          # one 16-byte chunk per pixel (Discriminator.in_pitch) + a K-row of slack
        # The REAL half of the discriminator batch (D2, D4: SHM.py:563, 638-642) depends on no generator output: in bf16 its five convolution
        # blocks run on the second stream beside the generator's forward passes (round 6); the heads wait for `ev_dreal`
        ev_dreal = None
        d_real_early = self.d_fwd_on_lane and lane.stream is not None

        def pack_real():
            ops.pack_rgb16(orig[4], noise[B:2 * B], xd[6 * B:7 * B], B * npix)                 # D(2) SHM.py:563
            for k in range(5):                                                                 # D(4) SHM.py:638-642
                ops.pack_rgb16(orig[k], None, xd[(7 + k) * B:(8 + k) * B], B * npix)
        if d_real_early:
            pack_real()
            D.start(xd, keep, [(0, B, 0), (6 * B, B, B)], attn_d)
            lane.submit(lambda: D.trunk_rows(6 * B, 12 * B))
            ev_dreal = lane.event()

        # ---- G(1)  SHM.py:517-538
        gen_in = A.get("g1/in", (B, H, W, PAD_C), adt)
        ops.build_gen_input(ds, None, fmask, 0, gen_in, B, npix)
        gen_Y = G.forward(gen_in, "g1", attn=attn_g)

        gen_rgb = A.get("g1/rgb", (B, H, W, 3))
        ops.yuv2rgb(gen_Y, cbcr, noise[:B], gen_rgb, xd[0:B], B, B, npix)                  # SHM.py:544-559

        # ---- G(2): cyclic  SHM.py:576-624
        cyc_in = A.get("cyc/in", (5 * B, H, W, PAD_C), adt)
        ops.build_gen_input(ds, gen_Y, fmask, 1, cyc_in, B, npix)
        cyc_Y = G.forward(cyc_in, "cyc", attn=attn_g)
        cyc_rgb = A.get("cyc/rgb", (5 * B, H, W, 3))
        ops.yuv2rgb(cyc_Y, cbcr, None, cyc_rgb, xd[B:6 * B], 5 * B, B, npix)
        if not d_real_early:
            pack_real()

        # ---- image-space losses (L1, SSIM, NST: SHM.py:744-826) and their gradients wrt the two Y planes.  Nothing reads them before the
        # G-loss backward leaves the discriminator (conv3x3_dgrad_sum1 below accumulates into dgen_y / dcyc_y), so in bf16 they run on the second
        # stream beside the discriminator's forward pass and the G-loss backward through it (round 6: ~0.5 / 1.3 / 1.4 ms of SSIM and L1 passes
        # were exposed per step at B = 8 / S = 512 B = 4 / B = 32); the main stream waits for `ev_img` where it needs them
        il = A.get("loss/img", (32,), torch.float64)
        dgen_y = A.get("loss/dgen_y", (B, H, W, 1))
        dcyc_y = A.get("loss/dcyc_y", (5 * B, H, W, 1))
        ws = self._img_ws(B)
        optr = (C.c_void_p * 5)(*[t.data_ptr() for t in orig])
        dptr = (C.c_void_p * 5)(*[t.data_ptr() for t in ds])
        ev_img = None

        def image_losses():
            ops.image_losses_hw(gen_rgb, cyc_rgb, cyc_Y, cbcr, optr, dptr, fmask, sf, il, dgen_y, dcyc_y, ws, B, H, W)
        if self.img_loss_on_lane and lane.stream is not None:
            lane.submit(image_losses)
            ev_img = lane.event()
        else:
            image_losses()

        # ---- D on all 12B images (noise + dropout on the D1 and D2 slices only)
        if d_real_early:
            D.trunk_rows(0, 6 * B)                                  # the fake half, here; the real half is already under way on the second stream
            torch.cuda.current_stream().wait_event(ev_dreal)
            rf, cls = D.heads()
        else:
            rf, cls = D.forward(xd, keep, [(0, B, 0), (6 * B, B, B)], attn=attn_d)
        np_ = (H // 32) * (W // 32)

        # ---- losses  SHM.py:669-844
        dl = A.get("loss/dhead", (16,), torch.float64)
        drf_d = A.get("loss/drf_d", (12 * B, np_))
        dcls_d = A.get("loss/dcls_d", (12 * B, 5))
        drf_g = A.get("loss/drf_g", (6 * B, np_))
        ops.dhead_losses(rf, cls, dl, drf_d, dcls_d, drf_g, B, np_, T,
                         ops.XENT_TF_FUSED if self.xent_mode == "executed" else ops.XENT_INTENDED)
        sl = A.get("loss/spec", (5,), torch.float64)                      # Spec_loss, logged only  SHM.py:792-806
        lane.submit(lambda: ops.spec_loss(cyc_Y, cbcr, dptr, self.specular_candidate, sl, B, npix))

        # ---- D backward (weights) then its all-reduce overlapped with everything below
        if self.before_backward is not None:
            self.before_backward()
        # The D-loss backward (weights only) depends on nothing below and nothing below depends on it: the whole chain -- InstanceNorm backward,
        # stride-2 input gradients, weight gradients -- goes to the second stream, in front of the generator's weight gradients, and the main
        # stream goes straight on to the G-loss backward (round 6; SHM_D_BWD_LANE=0 keeps it on the main stream).  Its buffers are keyed by the
        # batch (12 B here, 6 B for the data gradient below), the split-K workspace is used in lane order.
        if self.d_bwd_on_lane and lane.stream is not None:
            lane.submit(lambda: D.backward_params(drf_d, dcls_d))
        else:
            D.backward_params(drf_d, dcls_d)
        ev_d = self._allreduce_async(D.P.grad, after=self._get_lane().event(), tag="d")

        # ---- G-loss gradient through D (data gradient only), then G backward
        # Both first layers are left through the channel-summed stencil (ops.conv3x3_dgrad_sum1): yuv_to_rgb's
        # backward needs r+g+b of the image gradient, the G o G chain the sum over the substituted view channels.
        FD = D.chan[1]
        dzd = D.backward_input_dz(6 * B, drf_g)
        weff_d = A.get("d/weff", (9, FD))
        ops.sum_input_channels(D.P.vars[0], 3, FD, 0b111, weff_d)
        if ev_img is not None:
            torch.cuda.current_stream().wait_event(ev_img)          # dgen_y / dcyc_y of the image losses
        ops.conv3x3_dgrad_sum1(dzd[0:B], FD, weff_d, dgen_y, 1, B, H, W, FD, 2, 1)
        ops.conv3x3_dgrad_sum1(dzd[B:6 * B], FD, weff_d, dcyc_y, 1, 5 * B, H, W, FD, 2, 1)
        dzg = G.backward(dcyc_y, "cyc", need_dx="dz")
        weff_g = A.get("g/weff", (5, 9, F))
        for k in range(5):                                       # G o G chain  SHM.py:576-580
            ops.sum_input_channels(G.P.vars[0], 10, F, sum(1 << j for j in range(5) if j != k and flags[j]), weff_g[k])
        ops.conv3x3_dgrad_sum1(dzg, F, weff_g, dgen_y, 5, B, H, W, F, 1, 1)
        update_g = self.epoch >= self.train_G_after
        # no collective for a gradient nobody applies (it would also still be in flight when the next step
        # zeroes the bucket)
        reduce_g = exchange_active() and (update_g or not apply)
        # The G(1) backward is the last pass that touches the generator's weight gradients, and it finishes the layers last
        # to first: each stage's slice of the flat gradient is all-reduced as soon as the weight gradient of its lowest
        # layer has been issued on the wgrad lane (the collective waits for that lane event on the reducer stream), under
        # the rest of the pass.  Only the small last bucket (first encoder layers + head kernel + biases) is exposed.
        ev_g = None
        on_wgrad = None
        if reduce_g:
            plan = {trig: slices for trig, slices in G.grad_buckets()}

            def on_wgrad(li):
                for lo, hi in plan.get(li, ()):
                    self._allreduce_async(G.P.grad[lo:hi], after=lane.event())
        G.backward(dgen_y, "g1", need_dx=False, on_wgrad=on_wgrad)
        if attn_g is not None:
            G.attention_backward()                      # the skip gradients of both passes, summed per sample
        G.finish_grads()
        lane.join()                             # all weight gradients (both models) are complete
        if reduce_g:
            for lo, hi in plan[None]:
                ev_g = self._allreduce_async(G.P.grad[lo:hi])        # the reducer stream runs its collectives in order

        # ---- look-ahead: the next batch's weight-independent prologue goes in front of the waits on this step's collectives
        if next_batch is not None:
            nb = next_batch() if callable(next_batch) else next_batch
            if nb is not None:
                self._prefetched = self._prologue([self._dev(t) for t in nb], pro.slot ^ 1)

        # ---- clip + Adam  SHM.py:859-872.  On a histogram step (telemetry, rank 0 only: the reduced gradient is the same on every rank) the
        # gradient statistics go beside the Adam launch of the same buffer: both only read the gradient, after its collective
        tel = self.telemetry if apply and dist.rank() == 0 else None
        step = D.P.iterations + 1
        hist_now = tel is not None and tel.wants_histograms(step)
        if apply:
            self._reducer.wait_on(ev_d)
            if hist_now:
                tel.record_gradients("D", 1.0 / world)
            self.optimizer_D.apply(D.P, 1.0 / world, abort=self.arena.abort)
            D.weights_dirty = True
            if update_g:
                self._reducer.wait_on(ev_g)
                if hist_now:
                    tel.record_gradients("G", 1.0 / world)
                self.optimizer_G.apply(G.P, 1.0 / world, abort=self.arena.abort)
                G.weights_dirty = True
                if self._ema_on():       # the average follows the update on the same stream, on every rank (the weights are the same on all), under
                    # the same abort word: a step that did not move the weights does not move the average.  The decay comes from a host counter
                    ops.ema_update(G.P.ema, G.P.flat, G.P.n, ops.ema_decay_at(self.args.ema_decay, G.P.ema_updates, bool(self.args.ema_warmup)),
                                   abort=self.arena.abort)
                    G.P.ema_updates += 1
        elif exchange_active():
            for ev in (ev_d, ev_g):
                self._reducer.wait_on(ev)

        # ---- attribute side effects (SHM.py:538-553, 620-624, 863, 872)
        self.gen_input, self.gen_Y, self.gen_rgb = gen_in, gen_Y, gen_rgb
        self.target_img = orig[4]
        (self.cyc_gen0_rgb, self.cyc_gen45_rgb, self.cyc_gen90_rgb, self.cyc_gen135_rgb,
         self.cyc_genED_rgb) = [cyc_rgb[k * B:(k + 1) * B] for k in range(5)]
        self.RealFake_gen_D1, self.label_gen_D1 = rf[0:B], cls[0:B]
        self.RealFake_target_D2, self.label_target_D2 = rf[6 * B:7 * B], cls[6 * B:7 * B]
        self.gradmapD, self.gradmapG = D.P.grads, G.P.grads
        self.stddev_arr = scales          # reference appends forever (a leak); we keep the last step's
        self._last = SimpleNamespace(dl=dl, il=il, sl=sl, npix=npix, B=B, flags=flags, T=T, scales=scales, ds=ds, cbcr=cbcr)
        self._loss_cache = None
        if tel is not None:
            tel.after_step(step, self.epoch, T, self._last, hist_now, update_g)
        return None

    # ------------------------------------------------------------------ the training loop (SHM.py:889-1139)
    def train(self, args=None, *, max_steps=None, print_fn=print):
        """`shmgan.train(args)` of /root/reference/main.py:107 (loop: SHM.py:889-1139): datasetLoad ->
        build_generator / build_discriminator (+ summaries) -> SpecSeg -> restore the latest checkpoint ->
        for epoch / for batch in range(batches_per_epoch - 1): TARGET_LABELS ~ U(0.8, 1.2) (SHM.py:986),
        next 5-tuple (SHM.py:990), train_step (SHM.py:998) -> checkpoint every `checkpoint_save_step` epochs
        (SHM.py:1125-1128) and once more at the end (SHM.py:1133).

        Differences, all outside the arithmetic: checkpoints are the neutral .npz of save_npz (Keras variable order
        and layouts; newest 3 kept, as CheckpointManager(max_to_keep=3)) instead of TF checkpoints; the summaries go
        to `log_dir`; the Comet histogram upload at step 100 (which raises AttributeError in the reference, SURVEY
        section 3.1) and the per-step gc.collect() are not reproduced.  The monitoring itself is: with `loss_log_step` (reference: 25) the
        named loss scalars of SHM.py:1035-1053 go to `log_dir`/losses.jsonl, with `histogram_step` (reference: 100) the statistics and
        sign / exponent histograms of every gradient tensor (gradmapD, gradmapG, SHM.py:1085-1091) and of every weight tensor go to
        gradients.jsonl / weights.jsonl, computed on the device and written by a thread of their own (telemetry.py; `nonfinite` says what
        a NaN or Inf gradient does).  Both are off by default; the step counts optimizer updates, so a resumed run appends.  The logs are
        flushed before every checkpoint.  The loader options `shuffle`, `data_seed`, `aug_flip_lr`, `aug_flip_ud`, `aug_crop_min` and
        `aug_views` (data.datasetLoad; all off by default) give an epoch-wise shuffle and a random crop / mirror per sample;
        aug_flip_ud=0.5 is the as-intended reading of the per-step draw below.  `cache="device"` (with `cache_gb`, GiB; default half of the free
        device memory) keeps the decoded samples on the device after their first decode, the reference's `.cache()`;
        `self.loadedDataset.cache_stats()` says what it holds.  `capture_format="dofp"` (with `dofp_dir`, `dofp_pattern`, `dofp_quad_angles`,
        `dofp_bits`, `dofp_demosaic`, and `dofp_black` / `dofp_white` / `dofp_wb` / `dofp_ccm` / `dofp_tone` / `dofp_sat` to develop the frames and `dofp_calibration`, the path of a saved polar.DofpCalibration, to correct them first, and `dofp_exposures` (with `dofp_bracket_black` / `dofp_bracket_white`) to read an exposure bracket per sample, one multi-page TIFF, merged on the device: data.capture_options) trains from one polariser-mosaic frame per sample instead of four view files.  `ema_decay` (with `ema_warmup`) keeps an average of the generator's weights
        (_ensure_ema, generator_weights); `val_dir` or `val_fraction` (with `val_seed`, `val_step`, `val_batch_size`, `val_monitor`, `val_region`) hold captures
        out: every `val_step` epochs, in front of the checkpoint, and once at the end they are scored (validate), rank 0 appends the means to
        `log_dir`/validation.jsonl and keeps the best weights as `checkpoint_save_dir`/best.npz (validation.py).  Both are off by default and
        leave the training trajectory bitwise alone when on.  `max_steps` (tests) stops early.  Returns the number of train_step calls made."""
        if args is not None:
            for k, v in vars(args).items():
                setattr(self.args, k, v)
                if k in self.__dict__:
                    setattr(self, k, v)
            if "image_hw" in vars(args):                                       # the frame cannot change under models that exist
                hw = check_image_hw(args.image_hw)
                frame = hw if hw is not None else (self.image_size, self.image_size)
                if self.G is not None and frame != (self.G.H, self.G.W):
                    raise ValueError(f"train: image_hw {hw} differs from the frame {(self.G.H, self.G.W)} this trainer's models were built for")
                default = self.style_factor == self._default_style_factor()
                self._image_hw = hw
                if default:                                                    # the default follows the frame; a value set by hand stays
                    self.style_factor = self._default_style_factor()
        start = time.perf_counter()
        a = self.args
        self._val_on, self._val_step, self._val_monitor = validation_options(a.val_dir, a.val_fraction, a.val_seed, a.val_step, a.val_batch_size, a.val_monitor,
                                                                             a.val_region)
        self._val_region = region_options(a.val_region, a.val_region_threshold, "val_region")
        ops.ema_decay_at(a.ema_decay, 0)                                       # checked before the data is listed
        self.length_dataset, dataset = datasetLoad(self)                       # SHM.py:904
        if self.G is None:
            self.build()                                                       # SHM.py:911-912, 930-931
        # data parallel: every rank trains on its own shard of the dataset (PolarDataset shards by rank) and holds the same
        # weights; files (summaries, checkpoints, log lines) are rank 0's business, the others wait at a barrier
        rank0 = dist.rank() == 0
        if not rank0:
            print_fn = lambda *a, **k: None
        if rank0:
            self._write_summaries()                                            # SHM.py:914-919, 933-935
            os.makedirs(self.checkpoint_save_dir, exist_ok=True)
        dist.barrier()
        latest = self._restore_latest()                                        # SHM.py:949-951 (delete_old_checkpoints is False)
        if latest is not None:
            print_fn(f"Latest checkpoint restored!! ({latest})")
        if self._val_on:
            self._best = checkpoint.best_to_beat(self._best, os.path.join(self.checkpoint_save_dir, self.BEST_CHECKPOINT), self._val_monitor,
                                                 "ema" if self._ema_on() else "raw")
        # the loader's shuffle and augmentation draws are keyed by the pass number: a resumed run goes on from the pass its restored
        # step counter (the one telemetry uses) lies in instead of replaying pass 0's order and draws
        dataset.first_pass = self.D.P.iterations // max(len(dataset), 1)
        loss_step, hist_step, _ = telemetry_options(self.args.loss_log_step, self.args.histogram_step, self.args.nonfinite)
        if rank0 and (loss_step or hist_step):
            self.start_telemetry()
        try:
            return self._train_loop(dataset, max_steps, print_fn, start)
        except BaseException:
            if self.telemetry is not None:                                     # what was logged before a step raised is written out;
                try:                                                           # the step's own error is the one to report
                    self.telemetry.flush()
                except Exception:
                    pass
            raise

    def _train_loop(self, dataset, max_steps, print_fn, start):
        iterator = iter(dataset)                                               # SHM.py:955
        batches_per_epoch = int(self.length_dataset / self.batch_size)         # SHM.py:957
        self.batch_step = 0
        done = False
        total_steps = self.num_epochs * max(batches_per_epoch - 1, 0)
        if max_steps is not None:
            total_steps = min(total_steps, max_steps)
        ahead = []                       # the batch train_step's look-ahead already took from the iterator

        def fetch_next():
            ahead.append(next(iterator, None))
            return ahead[-1]

        for epoch in range(self.num_epochs):                                   # SHM.py:969
            self.epoch = epoch
            print_fn(f"\nStart of Training Epoch {self.epoch}")
            for batch in range(batches_per_epoch - 1):                         # SHM.py:979
                self.batch_step += 1
                self.random_flip = bool(self._rng.random() >= 0.5)            # SHM.py:983 (inert: the map lambda is already traced)
                self.TARGET_LABELS = float(self._rng.uniform(0.8, 1.2))       # SHM.py:986
                element = ahead.pop() if ahead else next(iterator)             # SHM.py:990
                # SHM.py:998; the next tuple is taken from the loader late in this step (its prologue overlaps this step's
                # last gradient collective), not before it: this step must not wait for the next batch's decode
                self.train_step(*element, next_batch=fetch_next if self.batch_step < total_steps else None)
                if max_steps is not None and self.batch_step >= max_steps:
                    done = True
                    break
            if (self.epoch + 1) % self.log_step == 0:                          # SHM.py:1099-1106
                torch.cuda.current_stream().synchronize()
                print_fn("Time taken for epoch {} is {} min\n".format(self.epoch + 1, (time.perf_counter() - start) / 60))
            if self._val_on and (self.epoch + 1) % self._val_step == 0:        # held-out validation, in front of the checkpoint it may beat
                validation.validate_and_log(self, print_fn)
            if (self.epoch + 1) % self.checkpoint_save_step == 0:              # SHM.py:1125-1128
                print_fn("Saving checkpoint for epoch {} at {}".format(self.epoch + 1, self._save_checkpoint()))
            if done:
                break
        if self._val_on:                                                       # once at the end (unless these weights have just been scored)
            validation.validate_and_log(self, print_fn)
        print_fn("Saving checkpoint for epoch {} at {}".format(self.epoch + 1, self._save_checkpoint()))   # SHM.py:1133
        return self.batch_step

    def _write_summaries(self):
        """Generator / Discriminator / SpecSeg summaries into `log_dir` (SHM.py:914-919, 933-935; test.py:142-158)."""
        os.makedirs(self.log_dir, exist_ok=True)
        for mdl, fn in ((self.G, "Generator_summary.txt"), (self.D, "Discriminator_summary.txt"), (self.SpecSeg, "SpecSeg_summary.txt")):
            with open(os.path.join(self.log_dir, fn), "w") as f:
                mdl.summary(print_fn=lambda x: f.write(x + "\n"))

    # ------------------------------------------------------------------ checkpoints and held-out validation
    # functions of the trainer in checkpoint.py and validation.py, under the names the reference's scripts, bench.py and the tools use;
    # every read of a checkpoint file goes through _read_npz
    BEST_CHECKPOINT = checkpoint.BEST_CHECKPOINT
    save_npz, _read_npz = checkpoint.save, checkpoint.read
    _save_checkpoint, _restore_latest = checkpoint.save_numbered, checkpoint.restore_latest
    validate = validation.validate

    def load_npz(self, path):
        """Inverse of save_npz.  The file is read and validated as a whole first, so a damaged or mismatching file raises before any weight,
        Adam moment or draw-stream state has been touched."""
        checkpoint.apply(self, self._read_npz(path))

    # ------------------------------------------------------------------ inference (test.py:218-297)
    # arena names that hold one frame's worth of inference buffers (dropped when the frame shape changes, _frame_changed)
    # (of the live attention branch only the forward's mask / y1 / y2: its backward buffers belong to training)
    _FRAME_BUFFERS = ("inf", "specseg/inf", "pre/yuv/inf", "metrics/ws", "metrics/region_ws", "eval/region") + tuple(f"g/attn{lvl}/{n}" for lvl in range(4) for n in ("m", "y1", "y2"))

    def _frame_changed(self, H, W):
        """Inference keeps buffers for ONE frame shape: when (H, W) differs from the frame of the last infer() (square or not),
        that frame's buffers leave the arena -- after a device synchronise, because queued kernels may still read them: the
        metrics, and the image exporter's launch over the planes it was handed (evaluate.ImageExporter reads them on this
        stream into a buffer of its own, so nothing outlives the synchronise).  A run that stays at image_size x image_size
        never gets here with a changed shape: its buffers are allocated once, as before."""
        if self._inf_frame is not None and self._inf_frame != (H, W):
            torch.cuda.synchronize(self.device)
            for br in self.G.attn:                 # the branches' records hold the old frame's maps
                br.ctx = None
            self.gen_input = self.gen_Y = self.gen_rgb = self.specular_candidate = self._inf_photo = self._inf_planes = None
            self.highlight_region = self.region_metrics = None
            self.cyc_gen0_rgb = self.cyc_gen45_rgb = self.cyc_gen90_rgb = self.cyc_gen135_rgb = self.cyc_genED_rgb = None
            self.G.ctx.pop("inf1", None)
            self.G.ctx.pop("inf5", None)
            self.arena.drop(*self._FRAME_BUFFERS)
        self._inf_frame = (H, W)

    def infer(self, rgb, cyclic=True):
        """Forward-only path of the reference's evaluation script (/root/reference/test.py:218-297):
        standardised YUV of ONE rgb image -> G once with only view 0 populated (target ED) -> the
        generated RGB, whose channel 0 feeds five cyclic G calls.  rgb [B,H,W,3] in [0,1], H and W multiples of 16 and at least 32
        (the networks are fully convolutional): (H, W) = image_hw (the reference's image_size x image_size by default) runs the five cyclic
        passes as one batch of 5 B; any other frame runs them one after the other through one set of buffers (samples are
        independent under InstanceNorm: the same arithmetic per sample, a sixth of the activation memory) and keeps arena buffers
        for that one frame shape (_frame_changed).  cyclic=False stops after G1: the cyclic images are then None.
        Returns (gen_rgb [B,H,W,3], [5 x cyc_rgb [B,H,W,3]]); sets the same attributes as test.py."""
        if self.G is None:
            self.build()
        G, A = self.G, self.arena
        x = self._dev(rgb)
        if x.dim() != 4 or x.shape[3] != 3:
            raise ValueError(f"infer takes [B,H,W,3] images, got {tuple(x.shape)}")
        B, H, W = (int(v) for v in x.shape[:3])
        if min(H, W) < 32 or H % 16 or W % 16:
            raise ValueError(f"infer takes frames whose sides are multiples of 16 and at least 32, got {H} x {W}")
        model_frame = (H, W) == self.image_hw
        self._frame_changed(H, W)
        npix = H * W
        G.prepare_weights()
        yuv, scale = self.preprocess(x, "inf")
        if self.SpecSeg is None:
            self.SpecSeg = self.build_specseg()
        self.specular_candidate = self.SpecSeg.forward_plane(yuv, 3, 0, B, tag="specseg/inf")   # test.py:221
        cbcr = yuv[..., 1:].contiguous()                       # averageCbCr = the input's own CbCr (test.py:224)
        ys = [yuv] * 5
        adt, PAD_C = self.compute_dtype, self.pad
        gen_in = A.get("inf/in", (B, H, W, PAD_C), adt)
        ops.build_gen_input(ys, None, 0b11110, 0, gen_in, B, npix)          # views 1..4 zero, one-hot = ED
        attn = G.attention_forward(self.specular_candidate, B) if self.attention == "live" else None
        gen_Y = G.forward(gen_in, "inf1", attn=attn)
        gen_rgb = A.get("inf/rgb", (B, H, W, 3))
        ops.yuv2rgb(gen_Y, cbcr, None, gen_rgb, None, B, B, npix)
        outs = [None] * 5
        if cyclic:
            orig_Ych = gen_rgb[..., 0:1].contiguous()              # test.py:252
            cyc_in = A.get("inf/cyc_in", (5 * B, H, W, PAD_C), adt)
            ops.build_gen_input(ys, orig_Ych, 0b11111, 1, cyc_in, B, npix)      # view k zero, the others = orig_Ych
            cyc_rgb = A.get("inf/cyc_rgb", (5 * B, H, W, 3))
            if model_frame:
                cyc_Y = G.forward(cyc_in, "inf5", attn=attn)
                ops.yuv2rgb(cyc_Y, cbcr, None, cyc_rgb, None, 5 * B, B, npix)
            else:
                # one pass at a time through the buffers of "inf1", its output plane included: G1's Y moves to a buffer of its own
                gen_Y = A.get("inf/gen_y", (B, H, W, 1)).copy_(gen_Y)
                for k in range(5):
                    cyc_Y = G.forward(cyc_in[k * B:(k + 1) * B], "inf1", attn=attn)
                    ops.yuv2rgb(cyc_Y, cbcr, None, cyc_rgb[k * B:(k + 1) * B], None, B, B, npix)
                G.ctx.pop("inf1", None)                        # it would describe the last cyclic pass, not G1
            outs = [cyc_rgb[k * B:(k + 1) * B] for k in range(5)]
        self.gen_input, self.gen_Y, self.gen_rgb = gen_in, gen_Y, gen_rgb
        self._inf_photo = x if self.eval_region is not None else None      # the frame as fed (eval_region "residual" reads it)
        self._inf_planes = (yuv, gen_Y, scale)
        self.stddev_arr = [scale]
        (self.cyc_gen0_rgb, self.cyc_gen45_rgb, self.cyc_gen90_rgb, self.cyc_gen135_rgb, self.cyc_genED_rgb) = outs
        return gen_rgb, outs

    def evaluate(self, rgb, diffuse=None):
        """One batch of the reference's test mode (test.py:218-392): `infer(rgb)` and, when the diffuse targets are given
        ([B,H,W,3] in [0,1], the shape of rgb), their image-quality metrics against gen_rgb (ops.image_metrics_hw over the whole
        frame, on the library's kernels).  `evaluate_frame` is the same with a window and without the cyclic passes.
        Returns (gen_rgb, [5 x cyc_rgb], metrics): metrics is a float64 [B,5] device tensor {mse, psnr, ssim, de76, de94} per
        image (ops.METRIC_NAMES), or None.  Asynchronous like infer; gen_rgb and the metrics live until the next call."""
        return self.evaluate_frame(rgb, diffuse)

    def evaluate_frame(self, rgb, diffuse=None, window=None, cyclic=True):
        """`evaluate` for the native-resolution test mode: `infer(rgb, cyclic)` and, when the diffuse targets are given
        (in [0,1]), their image-quality metrics against gen_rgb (on the library's kernels).  window = (top, left, h, w): the part
        of the frame that is the photo (native-resolution test mode pads a photo to multiples of 16, data.pad_geometry); the
        targets are then tight [B,h,w,3] and the metrics are taken on the window only (ops.image_metrics_hw).  Without a window
        the targets have the frame's shape and the window is the whole frame.
        Returns (gen_rgb, [5 x cyc_rgb], metrics): metrics is a float64 [B,5] device tensor {mse, psnr, ssim, de76, de94} per
        image (ops.METRIC_NAMES), or None.  Asynchronous like infer; gen_rgb and the metrics live until the next call."""
        gen_rgb, cyc = self.infer(rgb, cyclic)
        B, H, W = (int(v) for v in gen_rgb.shape[:3])
        if window is not None:
            top, left, h, w = (int(v) for v in window)
            if min(top, left) < 0 or min(h, w) < 1 or top + h > H or left + w > W:
                raise ValueError(f"window {tuple(window)} does not lie inside the {H} x {W} frame")
        metrics = None
        if diffuse is not None:
            t = self._dev(diffuse)
            out = self.arena.get("eval/metrics", (B, 5), torch.float64)
            win = (0, 0, H, W) if window is None else (top, left, h, w)
            if tuple(t.shape) != (B, win[2], win[3], 3):
                raise ValueError(f"diffuse images {tuple(t.shape)} do not match the generated ones {tuple(gen_rgb.shape)}" if window is None else
                                 f"diffuse images {tuple(t.shape)} do not match the window {win[2]} x {win[3]} of the generated ones")
            metrics = ops.image_metrics_hw(gen_rgb, win, t, out=out, arena=self.arena)
            if self.eval_region is not None:
                self._region_metrics(self.eval_region, self._inf_photo, gen_rgb, t, win)
        return gen_rgb, cyc, metrics

    DETAIL_MODES = ("residual", "guided")

    def refine(self, photos_u8, mode="guided", radius=2, eps=1e-2):
        """Full-resolution output after an infer() or evaluate() of the same batch: the generator only changes the standardised Y, so
        that change is fitted at model resolution against the Y it was fed (ops.detail_coeffs: the guided filter's two coefficients,
        one call for the batch, into the arena's "inf/detail_coef") and applied to each photo's own Y at its own size
        (ops.detail_apply_u8, one call per image; include/shmgan_hip.h states the arithmetic).  photos_u8: B uint8 device tensors
        [h_b,w_b,3], the decoded photos of the batch in its order (sizes may differ; evaluate.test takes them from
        EvalDataset(keep_source=True)).  mode "guided" fits windows of `radius` model pixels (1..8) with the regulariser `eps`;
        "residual" is radius 0, the bilinearly upsampled correction.  Returns B float32 [h_b,w_b,3] tensors in gen_rgb's units, new
        allocations the caller owns; asynchronous like infer.  ValueError without a preceding infer or for another batch size."""
        if mode not in self.DETAIL_MODES:
            raise ValueError(f"refine: mode {mode!r} is not one of {self.DETAIL_MODES}")
        if self._inf_planes is None:
            raise ValueError("refine follows an infer() or evaluate() of the same batch: none has run (or its frame was dropped)")
        yuv, gen_Y, scale = self._inf_planes
        B, H, W = (int(v) for v in gen_Y.shape[:3])
        photos = list(photos_u8)
        if len(photos) != B:
            raise ValueError(f"refine: {len(photos)} photos for the batch of {B} the last infer() ran")
        r = 0 if mode == "residual" else int(radius)
        if mode == "guided" and not 1 <= r <= ops.DETAIL_MAX_RADIUS:
            raise ValueError(f"refine: radius {radius} outside [1, {ops.DETAIL_MAX_RADIUS}] (mode 'residual' is radius 0)")
        coef = ops.detail_coeffs(yuv[..., 0], gen_Y, r, eps, out=self.arena.get("inf/detail_coef", (B, H, W, 2)))
        return [ops.detail_apply_u8(p, coef[b], scale[b:b + 1]) for b, p in enumerate(photos)]

    EVAL_REGIONS = ("residual", "specseg")

    def _region_metrics(self, spec, photo, gen_rgb, t, win, out=None):
        """The `eval_region` part of evaluate_frame (validation.validate uses it too), after an infer() of this frame: the highlight of
        the window `win` under spec = (kind, tau) -- from the `photo` infer was fed and the diffuse target t, or from the SpecSeg mask
        infer computed -- into `highlight_region`, and gen_rgb's metrics against t inside and outside it into `region_metrics` (or
        `out`).  Two more launch groups on the current stream, arena buffers (the region lives in a frame-sized buffer, so windows of
        one frame share it)."""
        kind, tau = spec
        if kind not in self.EVAL_REGIONS:
            raise ValueError(f"eval_region {spec!r} is not None or one of {self.EVAL_REGIONS} with a threshold")
        B, H, W = (int(v) for v in gen_rgb.shape[:3])
        h, w = win[2], win[3]
        region = self.arena.get("eval/region", (B * H * W,), torch.uint8)[:B * h * w].view(B, h, w)
        if kind == "residual":
            ops.highlight_region("residual", win, src=photo, target=t, tau=tau, out=region)
        else:
            ops.highlight_region("plane", win, plane=self.specular_candidate, tau=tau, out=region)
        if out is None:
            out = self.arena.get("eval/region_metrics", (B, ops.REGION_METRICS), torch.float64)
        self.highlight_region = region
        self.region_metrics = ops.image_metrics_region(gen_rgb, win, t, region, out=out, arena=self.arena)
        return self.region_metrics

    def _img_ws(self, B):
        H, W = self.image_hw
        n = ops.image_losses_hw_workspace(B, H, W)
        return self.arena.get("loss/ws", ((n + 3) // 4,))

    # ------------------------------------------------------------------ named losses (lazy D2H)
    def losses(self):
        """Compose the reference's named loss scalars (mean over the batch) from the two f64 loss
        vectors the kernels filled.  Synchronises (device->host copy) -- call it off the hot path."""
        if self._loss_cache is not None:
            return self._loss_cache
        L = self._last
        self._check_abort(sync=True)
        out = compose_losses(L.dl.cpu().numpy(), L.il.cpu().numpy(), L.sl.cpu().numpy(), L.B, L.npix)
        self._loss_cache = out
        return out

    def __getattr__(self, name):
        # reference attribute names for the loss scalars (self.total_Generator_loss, ...)
        if name in LOSS_NAMES and self._last is not None:
            return self.losses()[name]
        raise AttributeError(name)

    @property
    def gen_rgb_output(self):
        """SHM.py:548-550: yuv_to_rgb(gen_YCbCr * mean(stddev_arr) * 255) (display only).  Plain torch tensor arithmetic on purpose: like
        `custom_per_image_standardization` and `gram_matrix` this is an API-parity helper OFF the hot path (nothing in `train_step` / `infer`
        calls it) -- the three are the only torch compute in the package; the step itself runs on the library's kernels alone."""
        L = self._last
        avg = torch.stack([s.mean() for s in self.stddev_arr]).mean()
        yuv = torch.cat([self.gen_Y, L.cbcr], dim=3) * avg * 255.0
        k = torch.tensor([[1.0, 1.0, 1.0], [0.0, -0.394642334, 2.03206185], [1.13988303, -0.58062185, 0.0]],
                         device=yuv.device)
        return yuv @ k
