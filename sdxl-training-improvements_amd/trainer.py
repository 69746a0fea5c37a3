"""Trainer-plugin surface of the native path -- the drop-in for the reference's method trainers.

Reference contract mirrored here:
  * constructed like every trainer: (model, optimizer, train_dataloader, device, wandb_logger=None, config=None, **kw)
    (training/trainers/base_router.py:14-31, sdxl_trainer.py:18-41);
  * `compute_loss(batch) -> {"loss": 0-d tensor with .backward(), "metrics": dict}` (methods/example_method.py:108-122;
    flow matching signature `(model, batch, generator=None)` is accepted too, flow_matching_trainer.py:261);
  * `training_step(batch)` = the DDPM name of the same thing (ddpm_trainer.py:280);
  * `_execute_training_step(batch, accumulate, is_last_accumulation_step) -> (loss, metrics)`
    (ddpm_trainer.py:256-278 / flow_matching_trainer.py:237-259), with the D10 repair: gradients are zeroed at the
    START of an accumulation cycle, not before its last micro-step;
  * `train(num_epochs)`: the template loop (methods/example_method.py:150-230): every N micro-steps clip -> step -> zero;
  * batch dict keys {"vae_latents","prompt_embeds","pooled_prompt_embeds","time_ids","metadata"} else ValueError
    (ddpm_trainer.py:284-290); optional "tag_weights" [B];
  * metric keys: DDPM loss, lr, timestep_mean, timestep_std, noise_scale, pred_scale, batch_size (ddpm_trainer.py:386-396);
    flow matching loss, x0_norm, x1_norm, time_mean, time_std, velocity_norm, batch_size, lr
    (flow_matching_trainer.py:338-347).
Selected by `training.method` in config.yaml exactly like the reference (sdxl_trainer.py:128-152): "ddpm" or
"flow_matching"; anything else raises ValueError.  (The module `native_mi355x.py` is the file a maintainer drops into the
reference's `methods/` directory; it registers this class under the method name "native_mi355x".)

`model` is what the reference hands every trainer (models/sdxl.py:11-62): an object whose `.unet` is the PyTorch /
diffusers UNet.  Its diffusers-keyed `state_dict()` is imported into the packed native arena at construction
(`sdxl_load_weight`), and `sync_to_model()` / `save_checkpoint()` write the trained weights back into that module, so the
reference's `model.save_pretrained` (models/sdxl.py:246-288) keeps producing a loadable diffusers checkpoint.  A
`NativeUNet` may be passed directly as well.
"""
from __future__ import annotations

import ctypes as C
import json
import logging
import math
import os
import time
from collections import defaultdict
from contextlib import contextmanager
from pathlib import Path
from typing import Any, Dict, Optional

import torch

from . import distributed as D
from . import lib
from .config import Config
from .ema import WeightEMA
from .optimizer import BY_TYPE, AdamWBF16, FusedArenaOptimizer
from .sampler import PARAMETERIZATIONS, SOLVERS, NativeSampler, check_solver
from .scheduler import NoiseScheduler
from .unet import NativeUNet, config_from_unet, loss_mask_bhw

logger = logging.getLogger(__name__)

REQUIRED_KEYS = {"vae_latents", "prompt_embeds", "pooled_prompt_embeds", "time_ids", "metadata"}
LOSS_TYPES = ("l2", "huber", "smooth_l1")
HUBER_SCHEDULES = ("constant", "snr")
SNR_WEIGHTINGS = ("reference", "debiased")
WEIGHT_SETS = ("trained", "ema")
MASKED_LOSSES = ("off", "mean", "masked_mean")
INPUT_CONDITIONINGS = ("none", "inpaint", "concat")
CONDITIONING_GRADS = ("auto", "off")


_INPUT_COND = object()      # marks the input_cond tensor behind _NativeLoss.apply's residuals: (..., *residuals, _INPUT_COND, input_cond)


class _NativeLoss(torch.autograd.Function):
    """0-d loss whose backward runs the HIP backward with the incoming scale (so `(loss / N).backward()` works).
    prompt_embeds / pooled: the conditioning tensors the UNet read (after conditioning dropout) when one of them requires grad, else
    None.  Their gradients come back from the device (NativeUNet.read_cond_grads) in each input's device and dtype, so the caller's
    autograd graph -- text encoders, an embedding table -- continues from here.
    residuals: the additional skip residuals a `control` module produced (down ..., mid; None where nothing requires grad): their
    gradients come back the same way (NativeUNet.read_residual_grads), so the control module trains through the loss.
    An input_cond that requires grad follows the residuals behind the marker _INPUT_COND: it gets channels 4.. of the input gradient
    (NativeUNet.read_input_grad), so an encoder in front of the UNet input trains through the loss."""

    @staticmethod
    def forward(ctx, anchor, trainer, value, prompt_embeds=None, pooled=None, *residuals):
        ctx.trainer = trainer
        ctx.icond = None
        if len(residuals) >= 2 and residuals[-2] is _INPUT_COND:
            t, residuals = residuals[-1], residuals[:-2]
            ctx.icond = (t.shape, t.dtype, t.device)
        ctx.cond = [None if t is None else (t.shape, t.dtype, t.device) for t in (prompt_embeds, pooled)]
        ctx.res = [None if t is None else (t.shape, t.dtype, t.device) for t in residuals]
        return anchor.new_tensor(value)

    @staticmethod
    def backward(ctx, grad_out):
        ctx.trainer._native_backward(float(grad_out))
        grads = [None, None]
        if any(ctx.needs_input_grad[3:5]):
            # the backward ran with grad_scale / world (the parameter gradients are summed over the ranks afterwards); the caller's own
            # modules average theirs across ranks themselves (DDP), so they get this rank's gradient of grad_scale x loss
            world = float(ctx.trainer.sync.world)
            dev = ctx.trainer.net.read_cond_grads()
            for i in range(2):
                if ctx.needs_input_grad[3 + i] and ctx.cond[i] is not None:
                    shape, dtype, device = ctx.cond[i]
                    g = dev[i] if world == 1.0 else dev[i] * world
                    grads[i] = g.reshape(shape).to(device=device, dtype=dtype)
        res = [None] * len(ctx.res)
        if ctx.res and any(ctx.needs_input_grad[5:]):      # the same world-size factor as the conditioning gradients, for the same reason
            world = float(ctx.trainer.sync.world)
            d_down, d_mid = ctx.trainer.net.read_residual_grads()
            dev = list(d_down or [None] * (len(ctx.res) - 1)) + [d_mid]
            for i, meta in enumerate(ctx.res):
                if meta is not None and ctx.needs_input_grad[5 + i] and dev[i] is not None:
                    shape, dtype, device = meta
                    g = dev[i] if world == 1.0 else dev[i] * world
                    res[i] = g.reshape(shape).to(device=device, dtype=dtype)
        if ctx.icond is None:
            return (None, None, None, grads[0], grads[1], *res)
        d_ic = None
        if ctx.needs_input_grad[-1]:      # channels 4.. of d_input; the same world-size factor as the conditioning gradients, for the same reason
            world = float(ctx.trainer.sync.world)
            shape, dtype, device = ctx.icond
            g = ctx.trainer.net.read_input_grad()[:, 4:]
            d_ic = (g if world == 1.0 else g * world).reshape(shape).to(device=device, dtype=dtype)
        return (None, None, None, grads[0], grads[1], *res, None, d_ic)


class NativeSDXLTrainer:
    """SDXL trainer whose compute_loss / backward run in libsdxlstep (HIP, gfx950)."""

    name = "native_mi355x"

    def __init__(self, model, optimizer=None, train_dataloader=None, device=None, wandb_logger=None,
                 config: Optional[Config] = None, **kwargs):
        self.model = model
        self.train_dataloader = train_dataloader
        self.device = device if device is not None else torch.device("cuda", 0)
        self.wandb_logger = wandb_logger
        self.config = config if config is not None else Config()
        method = str(self.config.training.method).lower()
        if method not in ("ddpm", "flow_matching"):
            raise ValueError(f"Unsupported training method: {self.config.training.method}")   # sdxl_trainer.py:151
        self.method = method
        self._check_loss_keys()
        self._check_sampler_keys()
        self.gradient_accumulation_steps = int(self.config.training.gradient_accumulation_steps)
        # control(sample, timestep, batch) -> (down, mid): a module outside the UNet (a ControlNet) whose outputs are added to the skips and
        # to the mid block's output (diffusers' down_block_additional_residuals / mid_block_additional_residual); None = none
        self.control = kwargs.pop("control", None)
        unet = model.unet if hasattr(model, "unet") else model
        native_attrs = ("forward_loss", "backward", "read_loss", "zero_grads", "param_elems")
        self._torch_unet = None
        if all(hasattr(unet, a) for a in native_attrs):
            self.net = unet                                            # already a NativeUNet
        elif callable(getattr(unet, "state_dict", None)):
            # the reference's model object: import the PyTorch UNet's diffusers-keyed weights (models/sdxl.py:40, :92)
            sd = unet.state_dict()
            factory = kwargs.pop("native_factory", None)               # (tests: a stand-in for machines without a GPU)
            ncfg = kwargs.pop("native_config", None) or config_from_unet(unet, sd)
            dev = self.device.index if isinstance(self.device, torch.device) and self.device.index is not None else 0
            self.net = factory(ncfg) if factory is not None else NativeUNet(ncfg, device=dev)
            self.net.load_state_dict(sd, strict=True)                   # KeyError on any missing / unexpected key
            self._torch_unet = unet
        else:
            raise TypeError("model.unet must be a NativeUNet or a module with a diffusers-keyed state_dict(); got "
                            f"{type(unet).__name__}")
        self._check_input_conditioning()
        self.noise_scheduler = NoiseScheduler(self.config, "cpu")
        self.optimizer = self._build_optimizer(optimizer)
        self.ema = build_ema(self.net, self.optimizer, self.config.training)     # None unless training.use_ema
        self._clip_coef = None
        self.sync = self._build_grad_sync()
        self.sharded = isinstance(self.sync, D.ShardedGradSync)      # (falls back to all-reduce where the segments do not split)
        self._emit = False                   # this backward's weight-gradient GEMMs write the bf16 exchange arena themselves
        self._micro = 0                      # micro-step index inside the accumulation cycle
        self._zeroed = False                 # gradients already zeroed for the cycle in progress
        self._anchor = torch.zeros((), requires_grad=True)
        self._exchange = True
        self._final_known = False            # this backward is known to be the cycle's last micro-step (emit mode is safe)
        hook = getattr(self.optimizer, "register_step_post_hook", None)
        if callable(hook):                   # an optimizer step ends the accumulation cycle, whoever calls it
            hook(lambda *_a, **_k: self._end_cycle())

    # -------------------------------------------------------------------------------- the two builders a subclass may replace
    def _build_optimizer(self, optimizer):
        """the caller's optimizer, else the fused one the config names, on the net's arenas (lora.NativeLoRATrainer: on the adapters')"""
        return optimizer if optimizer is not None else build_optimizer(self.net, self.config.optimizer)

    def _build_grad_sync(self):
        """the gradient exchange of the full arena, with its exchange buffers"""
        # data parallel: ZeRO-1 (reduce-scatter, sharded fused AdamW, all-gather) with the fused optimizer, else all-reduce
        so = getattr(self.config.training, "shard_optimizer", None)          # None = not given: the default, sharded
        zero1 = isinstance(self.optimizer, FusedArenaOptimizer) and self.optimizer.ZERO1     # (False: its update reduces over the whole arena)
        if so and isinstance(self.optimizer, FusedArenaOptimizer) and not zero1:
            raise ValueError(f"training.shard_optimizer: ZeRO-1 is not built for {type(self.optimizer).__name__}; leave the key out "
                             "(every rank then runs the full update on the all-reduced gradients)")
        want_sharded = (True if so is None else bool(so)) and zero1
        seg_sizes = [n for _off, n in self.net.segment_ranges()] if hasattr(self.net, "segment_ranges") else None
        # force_exchange (build-only key / SDXL_FORCE_EXCHANGE=1): run the exchange through the backend even at world size 1
        force = bool(getattr(self.config.training, "force_exchange", False)) or os.environ.get("SDXL_FORCE_EXCHANGE", "0") == "1"
        return D.make_grad_sync(self.net.param_elems, self._cast, torch.bfloat16, getattr(self.net, "device", "cpu"),
                                sharded=want_sharded, segment_sizes=seg_sizes, force=force)

    # -------------------------------------------------------------------------------- loss
    def _cast(self, off, n, dst):
        # the exchange micro-step's weight-gradient GEMMs wrote bf16 into the comm arena themselves (set_grad_emit): what is
        # left to cast per bucket are the biases / norm parameters (fp32 atomic accumulators)
        if self._emit:
            self.net.cast_small(off, n, dst)
            return
        lib.check(self.net.L.sdxl_grads_to_bf16(self.net.h, off, n, C.c_void_p(dst.data_ptr()), 1.0,
                                                C.c_void_p(torch.cuda.current_stream().cuda_stream)))

    def _check_loss_keys(self) -> None:
        """the string keys of the loss extensions, checked when the trainer is built (ValueError names the key)"""
        tc = self.config.training
        self.loss_type = str(getattr(tc, "loss_type", "l2")).lower()
        self.huber_schedule = str(getattr(tc, "huber_schedule", "constant")).lower()
        self.snr_weighting = str(getattr(tc, "snr_weighting", "reference")).lower()
        self.huber_c = float(getattr(tc, "huber_c", 0.1))
        for key, val, known in (("loss_type", self.loss_type, LOSS_TYPES), ("huber_schedule", self.huber_schedule, HUBER_SCHEDULES),
                                ("snr_weighting", self.snr_weighting, SNR_WEIGHTINGS)):
            if val not in known:
                raise ValueError(f"training.{key}: unknown value {getattr(tc, key)!r} (expected one of {', '.join(known)})")
        self.masked_loss = str(getattr(tc, "masked_loss", "off")).lower()
        if self.masked_loss not in MASKED_LOSSES:
            raise ValueError(f"training.masked_loss: unknown value {getattr(tc, 'masked_loss')!r} (expected one of {', '.join(MASKED_LOSSES)})")
        cg = getattr(tc, "conditioning_grads", "auto")
        self.conditioning_grads = cg.lower() if isinstance(cg, str) else cg
        if self.conditioning_grads not in CONDITIONING_GRADS:
            raise ValueError(f"training.conditioning_grads: unknown value {cg!r} (expected one of {', '.join(CONDITIONING_GRADS)})")
        for key, top in (("noise_offset", None), ("input_perturbation", None), ("cond_dropout_prob", 1.0)):
            v = getattr(tc, key, 0.0)
            ok = not isinstance(v, bool) and isinstance(v, (int, float)) and math.isfinite(float(v)) and float(v) >= 0.0
            if not ok or (top is not None and float(v) > top):
                raise ValueError(f"training.{key} must be a number {'>= 0' if top is None else 'in [0, 1]'} (got {v!r})")
            setattr(self, key, float(v))
        if self.loss_type != "l2" and not self.huber_c > 0.0:
            raise ValueError(f"training.huber_c must be > 0 for training.loss_type {self.loss_type!r} (got {self.huber_c})")
        if self.method != "ddpm":
            if self.huber_schedule == "snr":
                raise ValueError("training.huber_schedule: 'snr' is defined on the ddpm sigma only (flow matching has none)")
            if self.snr_weighting == "debiased":
                raise ValueError("training.snr_weighting: 'debiased' is a ddpm weighting (flow matching has no snr)")
        elif self.snr_weighting == "debiased" and self.config.model.min_snr_gamma is None:
            raise ValueError("training.snr_weighting: 'debiased' divides min(snr, gamma) by the snr: it needs model.min_snr_gamma")

    def _check_input_conditioning(self) -> None:
        """training.input_conditioning / input_cond_dropout_prob against the net's in_channels, once the net exists (ValueError names the key)"""
        tc = self.config.training
        ic = getattr(tc, "input_conditioning", "none")
        self.input_conditioning = ic.lower() if isinstance(ic, str) else ic
        if self.input_conditioning not in INPUT_CONDITIONINGS:
            raise ValueError(f"training.input_conditioning: unknown value {ic!r} (expected one of {', '.join(INPUT_CONDITIONINGS)})")
        v = getattr(tc, "input_cond_dropout_prob", 0.0)
        if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(float(v)) or not 0.0 <= float(v) <= 1.0:
            raise ValueError(f"training.input_cond_dropout_prob must be a number in [0, 1] (got {v!r})")
        self.input_cond_dropout_prob = float(v)
        cfg = getattr(self.net, "cfg", None)
        cin = cfg.get("in_channels", 4) if isinstance(cfg, dict) else getattr(cfg, "in_channels", 4)
        self.in_channels = int(cin)
        want = {"none": "4", "inpaint": "9", "concat": "5 .. 16"}[self.input_conditioning]
        ok = {"none": cin == 4, "inpaint": cin == 9, "concat": 5 <= cin <= 16}[self.input_conditioning]
        if not ok:
            raise ValueError(f"training.input_conditioning: {self.input_conditioning!r} needs a UNet with in_channels = {want}, this one has {cin}")
        if self.input_conditioning == "none" and self.input_cond_dropout_prob > 0.0:
            raise ValueError("training.input_cond_dropout_prob: needs training.input_conditioning 'inpaint' or 'concat'")

    def _input_cond(self, batch, B: int, H: int, W: int, detach: bool = True) -> torch.Tensor:
        """the extra input channels [B, in_channels - 4, H, W] fp32 of a batch, a new tensor (ValueError names a missing key or a wrong shape);
        detach=False keeps the autograd graph of the batch's tensors (_input_cond_ext, when one of them requires grad)"""
        def get(key, shapes):
            if key not in batch or batch[key] is None:
                raise ValueError(f"training.input_conditioning {self.input_conditioning!r}: the batch has no {key!r}")
            t = torch.as_tensor(batch[key])
            if tuple(t.shape) not in shapes:
                raise ValueError(f"batch[{key!r}]: expected shape {' or '.join(str(s) for s in shapes)}, got {tuple(t.shape)}")
            return (t.detach() if detach else t).to(torch.float32)
        if self.input_conditioning == "inpaint":        # diffusers' order: latents | mask | masked-image latents
            m = get("inpaint_mask", ((B, 1, H, W), (B, H, W))).reshape(B, 1, H, W)
            ml = get("masked_latents", ((B, 4, H, W),))
            return torch.cat([m, ml.to(m.device)], dim=1)
        return get("cond_latents", ((B, self.in_channels - 4, H, W),)).clone()

    def _input_cond_ext(self, batch, lat, generator, augment: bool, ext: Dict[str, Any], grads: bool = False) -> None:
        """forward_loss's input_cond, when the key is on; with augment (a training step) the per-sample dropout, drawn after every
        other draw of the step and only when its key is on.  grads (compute_loss under autograd): when the assembled tensor requires
        grad -- an encoder produced the batch's cond_latents / masked_latents -- it is kept for _NativeLoss and the input gradient is
        requested; the net gets the detached values"""
        self._din_input = None
        if self.input_conditioning == "none":
            return
        B, _c, H, W = lat.shape
        track = grads and any(torch.is_tensor(batch.get(k)) and batch[k].requires_grad for k in ("cond_latents", "inpaint_mask", "masked_latents"))
        ic = self._input_cond(batch, B, H, W, detach=not track)
        if augment and self.input_cond_dropout_prob > 0.0:
            drop = torch.rand(B, generator=generator) < self.input_cond_dropout_prob
            ic[drop.to(ic.device)] = 0
        if track and ic.requires_grad:
            self._din_input = ic
            ext["input_grad"] = True
        ext["input_cond"] = ic.detach() if track else ic

    def _check_sampler_keys(self) -> None:
        """the validation / sampler keys, checked when the trainer is built (ValueError names the key)"""
        tc = self.config.training
        self.sampler_parameterization = str(getattr(tc, "sampler_parameterization", "trained")).lower()
        if self.sampler_parameterization not in PARAMETERIZATIONS:
            raise ValueError(f"training.sampler_parameterization: unknown value {getattr(tc, 'sampler_parameterization')!r} "
                             f"(expected one of {', '.join(PARAMETERIZATIONS)})")
        vw = getattr(tc, "validation_weights", None)
        use_ema = bool(getattr(tc, "use_ema", False))
        self.validation_weights = ("ema" if use_ema else "trained") if vw is None else str(vw).lower()
        if self.validation_weights not in WEIGHT_SETS:
            raise ValueError(f"training.validation_weights: unknown value {vw!r} (expected one of {', '.join(WEIGHT_SETS)})")
        if self.validation_weights == "ema" and not use_ema:
            raise ValueError("training.validation_weights: 'ema' needs training.use_ema")
        every, steps = getattr(tc, "validation_every_n_steps", 0), getattr(tc, "validation_num_steps", 30)
        if isinstance(every, bool) or not isinstance(every, int) or every < 0:
            raise ValueError(f"training.validation_every_n_steps must be an integer >= 0 (got {every!r})")
        least = 2 if self.method == "ddpm" else 1
        if isinstance(steps, bool) or not isinstance(steps, int) or steps < least:
            raise ValueError(f"training.validation_num_steps must be an integer >= {least} for {self.method} (got {steps!r})")
        for key in ("validation_guidance_scale", "validation_guidance_rescale"):
            v = getattr(tc, key, 0.0)
            if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(float(v)):
                raise ValueError(f"training.{key} must be a finite number (got {v!r})")
        if not 0.0 <= float(getattr(tc, "validation_guidance_rescale", 0.0)) <= 1.0:
            raise ValueError(f"training.validation_guidance_rescale must be in [0, 1] (got {tc.validation_guidance_rescale!r})")
        seed = getattr(tc, "validation_seed", 0)
        if isinstance(seed, bool) or not isinstance(seed, int):
            raise ValueError(f"training.validation_seed must be an integer (got {seed!r})")
        self.validation_sampler = str(getattr(tc, "validation_sampler", "euler")).lower()
        if self.validation_sampler not in SOLVERS:
            raise ValueError(f"training.validation_sampler: unknown value {getattr(tc, 'validation_sampler')!r} "
                             f"(expected one of {', '.join(SOLVERS)})")
        try:
            check_solver(self.validation_sampler, self.method, self.sampler_parameterization)
        except ValueError as e:
            raise ValueError(f"training.validation_sampler: {e}") from None
        eta = getattr(tc, "validation_eta", 1.0)
        if isinstance(eta, bool) or not isinstance(eta, (int, float)) or not math.isfinite(float(eta)) or float(eta) < 0.0:
            raise ValueError(f"training.validation_eta must be a finite number >= 0 (got {eta!r})")

    # -------------------------------------------------------------------------------- sampling / evaluation on either weight set
    @contextmanager
    def _weights(self, weights: str):
        """run the body on the trained weights ("trained": nothing changes) or on the EMA ("ema"): the fp32 EMA arena -- laid out like
        the weight arena -- is cast to bf16 into a temporary arena by the library's own cast (sdxl_grads_to_bf16 on the handle whose
        gradient arena IS the EMA arena, the one ema_state_dict() exports through), the training handle is bound to it for the body
        and bound back afterwards.  The trained weights, gradients, optimizer, EMA and accumulation state are not touched.  Under
        ZeRO-1 the EMA is current only after prepare_checkpoint() on every rank: before that this raises, like ema_state_dict()."""
        weights = str(weights).lower()
        if weights not in WEIGHT_SETS:
            raise ValueError(f"weights: unknown value {weights!r} (expected one of {', '.join(WEIGHT_SETS)})")
        if weights == "trained":
            yield
            return
        if self.ema is None:
            raise ValueError("weights='ema': this trainer keeps no EMA (training.use_ema is false)")
        self._require_gathered("sampling / evaluating the EMA", "Nothing was read.")
        net, n = self.net, self.net.param_elems
        buf = torch.empty(n + 128, dtype=torch.bfloat16, device=net.weights.device)
        off = (-buf.data_ptr() % 256) // 2
        tmp = buf[off:off + n]                                 # 256-byte aligned, as sdxl_bind_params requires of an arena
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        lib.check(net.L.sdxl_grads_to_bf16(self.ema._handle(), 0, n, C.c_void_p(tmp.data_ptr()), 1.0, st), "cast EMA -> bf16")
        lib.check(net.L.sdxl_bind_params(net.h, C.c_void_p(tmp.data_ptr()), C.c_void_p(net.grads.data_ptr())), "bind EMA weights")
        try:
            yield
        finally:
            torch.cuda.current_stream().synchronize()         # the body's kernels read tmp: finish them before it is freed
            lib.check(net.L.sdxl_bind_params(net.h, C.c_void_p(net.weights.data_ptr()), C.c_void_p(net.grads.data_ptr())),
                      "bind trained weights")

    def sample(self, prompt_embeds, pooled, time_ids, neg_prompt_embeds=None, neg_pooled=None, neg_time_ids=None, *, height: int,
               width: int, num_steps: Optional[int] = None, guidance_scale: Optional[float] = None,
               guidance_rescale: Optional[float] = None, generator: Optional[torch.Generator] = None, noise=None, sigmas=None,
               timesteps=None, weights: Optional[str] = None, solver: Optional[str] = None, eta: Optional[float] = None,
               step_noise=None, init_latents=None, strength: float = 1.0, inpaint_mask=None, input_cond=None,
               neg_input_cond=None) -> torch.Tensor:
        """Latents [B,4,height,width] fp32 on the device, sampled natively (sampler.py::NativeSampler) from the trained weights or
        the EMA; what is not given comes from the training.validation_* keys (solver / eta: validation_sampler / validation_eta;
        step_noise, init_latents, strength, inpaint_mask, input_cond and neg_input_cond are NativeSampler.sample's).  Decoding is the caller's.  Nothing of the training
        state changes: the next step has the bits it would have had without the call."""
        tc = self.config.training
        sampler = NativeSampler(self.net, self.method, str(tc.prediction_type), bool(self.config.model.use_ztsnr),
                                self.sampler_parameterization, config=self.config, t_bf16=str(tc.mixed_precision) == "bf16",
                                **({} if self.control is None else dict(control=self.control)))      # (only when set)
        ic = {} if input_cond is None else dict(input_cond=input_cond, neg_input_cond=neg_input_cond)      # (only when given)
        with self._weights(self.validation_weights if weights is None else weights):
            return sampler.sample(prompt_embeds, pooled, time_ids, neg_prompt_embeds, neg_pooled, neg_time_ids, height=height,
                                  width=width, num_steps=int(tc.validation_num_steps if num_steps is None else num_steps),
                                  guidance_scale=float(tc.validation_guidance_scale if guidance_scale is None else guidance_scale),
                                  guidance_rescale=float(tc.validation_guidance_rescale if guidance_rescale is None else guidance_rescale),
                                  generator=generator, noise=noise, sigmas=sigmas, timesteps=timesteps,
                                  solver=self.validation_sampler if solver is None else solver,
                                  eta=float(getattr(tc, "validation_eta", 1.0) if eta is None else eta), step_noise=step_noise,
                                  init_latents=init_latents, strength=strength, inpaint_mask=inpaint_mask, **ic)

    def validate(self, step: int, validation_batches, on_validation=None):
        """sample every conditioning batch of `validation_batches` (dicts with "prompt_embeds", "pooled_prompt_embeds", "time_ids",
        optional "neg_prompt_embeds" / "neg_pooled_prompt_embeds" / "neg_time_ids", "init_latents" / "strength" / "inpaint_mask" (img2img /
        inpainting, NativeSampler.sample), "height" / "width" of the latent or a
        "vae_latents" whose shape gives them) with the training.validation_* keys and the noise of validation_seed; returns the list of
        latents and hands each to on_validation(step, latents).  COLLECTIVE under ZeRO-1 with the EMA (prepare_checkpoint)."""
        if self.validation_weights == "ema":
            self.prepare_checkpoint()
        gen = torch.Generator().manual_seed(int(self.config.training.validation_seed))
        outs = []
        for b in validation_batches:
            if "height" in b and "width" in b:
                h, w = int(b["height"]), int(b["width"])
            else:
                h, w = (int(v) for v in b["vae_latents"].shape[-2:])
            blend_mask, ic = b.get("inpaint_mask"), {}
            if self.input_conditioning != "none":      # the extra input channels, built as in training (no dropout); "neg_input_cond" as given
                ic = dict(input_cond=self._input_cond(b, int(b["prompt_embeds"].shape[0]), h, w), neg_input_cond=b.get("neg_input_cond"))
                if self.input_conditioning == "inpaint" and b.get("init_latents") is None:
                    blend_mask = None                  # the mask is the UNet's input channel; the latent blend also needs init_latents
            lat = self.sample(b["prompt_embeds"], b["pooled_prompt_embeds"], b["time_ids"], b.get("neg_prompt_embeds"),
                              b.get("neg_pooled_prompt_embeds"), b.get("neg_time_ids"), height=h, width=w, generator=gen,
                              init_latents=b.get("init_latents"), strength=float(b.get("strength", 1.0)),
                              inpaint_mask=blend_mask, **ic)
            outs.append(lat)
            if on_validation is not None:
                on_validation(step, lat)
        return outs

    def _loss_ext(self, batch, sig) -> Dict[str, Any]:
        """The device loss's optional arguments from the config keys: each recipe is B floats computed here.  Several sources of
        the per-sample weight multiply.  Returns only what differs from the defaults (an empty dict = the reference's objective)."""
        tc = self.config.training
        ext: Dict[str, Any] = {}
        s = None
        if self.snr_weighting == "debiased":              # diffusers' --snr_gamma rule: min(snr, gamma) / (snr + 1 | snr)
            snr = sig.double() ** -2
            pred = str(tc.prediction_type)
            s = 1.0 / (snr + 1.0) if pred == "v_prediction" else 1.0 / snr
        tag = batch.get("tag_weights")
        if bool(getattr(tc, "tag_weights_per_sample", False)) and tag is not None:
            tw = torch.as_tensor(tag).double().reshape(-1)
            s = tw if s is None else s * tw
        if s is not None:
            ext["sample_weights"] = s.float()
        if self.loss_type != "l2":
            ext["loss_type"] = self.loss_type
            if self.huber_schedule == "snr":
                c = self.huber_c
                ext["huber_c"] = ((1.0 - c) / (1.0 + sig.double()) ** 2 + c).float()
            else:
                ext["huber_c"] = self.huber_c
        if bool(getattr(tc, "log_per_sample_loss", False)):
            ext["per_sample_loss"] = True
        mask = batch.get("loss_mask") if self.masked_loss != "off" else None      # a batch without one is unmasked
        if mask is not None:
            ext["loss_mask"] = loss_mask_bhw(mask, batch["vae_latents"].shape)
            if self.masked_loss != "mean":
                ext["mask_norm"] = self.masked_loss
        return ext

    def _augment(self, batch, noise, generator, cond_grads: bool = False):
        """The training-only recipes on top of the base noise (drawn or injected), each drawn from the step's generator only when its
        key is on, in the order noise offset, input perturbation, conditioning dropout -- after the base noise and the timesteps.
        Returns (batch, noise, ext): the batch a shallow copy with zeroed conditioning rows where dropout drew them (the caller's
        tensors are not modified), the noise after the offset (what the target uses), and noise_in for forward_loss.
        cond_grads: the conditioning carries a gradient back to the caller: the dropped rows are zeroed by a differentiable select, so
        autograd hands those samples zero rows."""
        ext: Dict[str, Any] = {}
        B = noise.shape[0]
        if self.noise_offset > 0.0:                        # diffusers' --noise_offset: one draw per sample and channel
            r = torch.randn(B, noise.shape[1], 1, 1, generator=generator)
            noise = noise.float() + self.noise_offset * r.to(noise.device)
        if self.input_perturbation > 0.0:                  # diffusers' --input_perturbation: the input's noise only
            r = torch.randn(noise.shape, generator=generator)
            ext["noise_in"] = noise.float() + self.input_perturbation * r.to(noise.device)
        if self.cond_dropout_prob > 0.0:                   # zero conditioning, what the sampler's guidance runs against; time_ids stay
            drop = torch.rand(B, generator=generator) < self.cond_dropout_prob
            batch = dict(batch)
            for key in ("prompt_embeds", "pooled_prompt_embeds"):
                if cond_grads:
                    t = batch[key]
                    d = drop.to(t.device).reshape((B,) + (1,) * (t.dim() - 1))
                    batch[key] = torch.where(d, torch.zeros((), dtype=t.dtype, device=t.device), t)
                    continue
                t = batch[key].clone()
                t[drop.to(t.device)] = 0
                batch[key] = t
        return batch, noise, ext

    def _cond_request(self, batch, ext) -> None:
        """compute_loss only: when the conditioning (after dropout) requires grad, ask the net for its gradients and keep the tensors
        for _NativeLoss; the net itself gets detached tensors"""
        self._cond_inputs = tuple(batch[k] if torch.is_tensor(batch[k]) and batch[k].requires_grad else None
                                  for k in ("prompt_embeds", "pooled_prompt_embeds"))
        want = tuple(n for n, t in zip(("prompt", "pooled"), self._cond_inputs) if t is not None)
        if want:
            ext["cond_grads"] = want
            for k in ("prompt_embeds", "pooled_prompt_embeds"):
                batch[k] = batch[k].detach() if torch.is_tensor(batch[k]) else batch[k]

    def _control_ext(self, batch, lat, noise, sig_or_t, timestep, ext: Dict[str, Any], grads: bool) -> None:
        """forward_loss's residuals from `control`, when one is set: the UNet input is built the way the loss preparation builds it
        (scheduler.add_noise for ddpm, the optimal-transport path for flow matching; from noise_in under input perturbation),
        control(sample, timestep, batch) runs under autograd (grads: compute_loss) or no_grad (evaluate), and the net gets the detached
        residuals.  With grads, the residuals that require grad are kept for _NativeLoss and their gradients requested."""
        self._res_inputs = ()
        if self.control is None:
            return
        nin = ext.get("noise_in", noise).float()
        dev = getattr(self.net, "device", None)
        if self.method == "ddpm":
            sample = lat + sig_or_t.view(-1, 1, 1, 1).to(lat.device) * nin.to(lat.device)
            if self.config.model.use_ztsnr:
                sample = torch.clamp(sample, -20000.0, 20000.0)
        else:
            t = sig_or_t.view(-1, 1, 1, 1).to(lat.device)
            sample = (1 - t) * nin.to(lat.device) + t * lat
        if dev is not None:
            sample, timestep = sample.to(dev), timestep.to(dev)
        with torch.enable_grad() if grads else torch.no_grad():
            down, mid = self.control(sample, timestep, batch)
        outs = list(down) + [mid]
        bf = all(t is None or t.dtype == torch.bfloat16 for t in outs)
        conv = lambda t: None if t is None else t.detach().to(dev if dev is not None else t.device, torch.bfloat16 if bf else torch.float32).contiguous()
        ext["residuals"] = ([conv(t) for t in down], conv(mid))
        if grads:
            self._res_inputs = tuple(t if t is not None and t.requires_grad else None for t in outs)
            want = [("mid" if i == len(outs) - 1 else i) for i, t in enumerate(self._res_inputs) if t is not None]
            if want:
                ext["residual_grads"] = want
            else:
                self._res_inputs = ()

    def _forward(self, batch, lat, noise, timesteps, generator, ext_over: Optional[Dict[str, Any]] = None, augment: bool = False,
                 cond_grads: bool = False, control_grads: bool = False):
        """draw what was not given, build the optional loss arguments, enqueue forward_loss; returns the timesteps used.
        augment: apply the training-only recipes (noise offset, input perturbation, conditioning dropout; _augment).
        cond_grads: compute_loss found a conditioning tensor that requires grad (_cond_request)
        control_grads: compute_loss under autograd: `control` runs with a graph and its residuals get their gradients (_control_ext);
        an input_cond that requires grad gets its gradient (_input_cond_ext)"""
        B = lat.shape[0]
        cm = self.config.model
        tag = batch.get("tag_weights")
        per_sample_tag = bool(getattr(self.config.training, "tag_weights_per_sample", False))
        if self.method == "ddpm":
            ts = timesteps if timesteps is not None else self.noise_scheduler.sample_timesteps(B, generator)
            sig = self.noise_scheduler.timestep_to_sigma(ts)
            ext = self._loss_ext(batch, sig)
            ext.update(ext_over or {})
            if augment:
                batch, noise, aug = self._augment(batch, noise, generator, cond_grads)
                ext.update(aug)
            self._input_cond_ext(batch, lat, generator, augment, ext, control_grads)
            if cond_grads:
                batch = dict(batch)
                self._cond_request(batch, ext)
            self._control_ext(batch, lat, noise, sig, ts, ext, control_grads)
            self.net.forward_loss("ddpm", lat, noise, sig, ts.float(), batch["prompt_embeds"],
                                  batch["pooled_prompt_embeds"], batch["time_ids"], None if per_sample_tag else tag,
                                  prediction_type=self.config.training.prediction_type,
                                  min_snr_gamma=cm.min_snr_gamma, use_ztsnr=cm.use_ztsnr, **ext)
            return ts
        if timesteps is None:                                      # sample_logit_normal, :373-385
            timesteps = torch.sigmoid(torch.randn(B, generator=generator))
        t = timesteps.float()
        if str(self.config.training.mixed_precision) == "bf16":     # D6: t is handed to the UNet in model dtype
            t_unet = t.to(torch.bfloat16).float()
        else:
            t_unet = t
        ext = self._loss_ext(batch, None)
        ext.update(ext_over or {})
        if augment:
            batch, noise, aug = self._augment(batch, noise, generator, cond_grads)
            ext.update(aug)
        self._input_cond_ext(batch, lat, generator, augment, ext, control_grads)
        if cond_grads:
            batch = dict(batch)
            self._cond_request(batch, ext)
        self._control_ext(batch, lat, noise, t, t_unet, ext, control_grads)
        self.net.forward_loss("flow_matching", lat, noise, t, t_unet, batch["prompt_embeds"],
                              batch["pooled_prompt_embeds"], batch["time_ids"], None if per_sample_tag else tag, **ext)
        return t

    def compute_loss(self, *args, generator: Optional[torch.Generator] = None, timesteps=None, noise=None) -> Dict[str, Any]:
        """compute_loss(batch) or compute_loss(model, batch[, generator]).  `timesteps` (ddpm: int64 indices, flow
        matching: t in (0,1)) and `noise` (ddpm noise / flow-matching x0) may be injected for reproducible fixtures;
        otherwise they are drawn as the reference draws them.  With training.log_per_sample_loss the result also carries
        "per_sample_loss" (CPU tensor [B], before the tag mean and the guard) and "timesteps"."""
        batch = args[-1] if not isinstance(args[-1], torch.Generator) else args[-2]
        if isinstance(args[-1], torch.Generator):
            generator = args[-1]
        if not all(k in batch for k in REQUIRED_KEYS):
            raise ValueError(f"Batch missing required keys: {REQUIRED_KEYS - set(batch.keys())}")
        lat = batch["vae_latents"].float()
        B = lat.shape[0]
        if noise is None:
            noise = torch.randn(lat.shape, generator=generator)
        # conditioning gradients (training.conditioning_grads "auto"): a prompt_embeds / pooled_prompt_embeds that requires grad gets its
        # gradient back through the loss, so the caller's text encoders or embedding table train with the UNet
        cond = (self.conditioning_grads != "off" and torch.is_grad_enabled() and
                any(torch.is_tensor(batch[k]) and batch[k].requires_grad for k in ("prompt_embeds", "pooled_prompt_embeds")))
        self._cond_inputs = (None, None)
        self._res_inputs = ()
        self._din_input = None
        ts = self._forward(batch, lat, noise, timesteps, generator, augment=True, cond_grads=cond, control_grads=torch.is_grad_enabled())
        o = self.net.read_loss()                                        # the single host sync of the step
        numel = lat.numel()
        lr = self.optimizer.param_groups[0]["lr"] if self.optimizer is not None else 0.0
        if self.method == "ddpm":
            metrics = {"loss": o[0], "lr": lr, "timestep_mean": float(ts.float().mean()),
                       "noise_scale": o[4] / numel, "pred_scale": o[2] / numel, "batch_size": B}
            if B > 1:
                metrics["timestep_std"] = float(ts.float().std())
        else:
            metrics = {"loss": o[0], "x0_norm": math.sqrt(o[5]), "x1_norm": math.sqrt(o[6]),
                       "time_mean": float(ts.mean()), "time_std": float(ts.std()) if B > 1 else float("nan"),
                       "velocity_norm": math.sqrt(o[3]), "batch_size": B, "lr": lr}
        icond = () if self._din_input is None else (_INPUT_COND, self._din_input)      # (only when it requires grad: the call is otherwise today's)
        loss = _NativeLoss.apply(self._anchor, self, o[0], *self._cond_inputs, *self._res_inputs, *icond)
        out = {"loss": loss, "metrics": metrics}
        if bool(getattr(self.config.training, "log_per_sample_loss", False)):
            out["per_sample_loss"] = self.net.read_per_sample_loss()    # (after read_loss's sync: the copy only)
            out["timesteps"] = ts
        return out

    def evaluate(self, batches, timesteps, generator: Optional[torch.Generator] = None, weights: str = "trained"):
        """Held-out loss at fixed timesteps, forward only: every batch is evaluated at each of `timesteps` (ddpm: indices into
        the sigma table; flow matching: t in (0, 1)) with noise drawn from `generator`.  No backward, no gradient zeroing, no
        optimizer or EMA step; the accumulation state is not touched.  The loss is the one the config keys select (weights,
        element loss, the batch's loss mask; none of noise offset, input perturbation, conditioning dropout), per sample, before
        the tag mean and the guard.  Returns ({timestep: mean per-sample loss}, overall mean).
        Evaluates the trained weights, or with weights="ema" the EMA (cast to bf16 into a temporary arena, see _weights)."""
        with self._weights(weights):
            return self._evaluate(list(batches), timesteps, generator)

    def _evaluate(self, batches, timesteps, generator):
        sums: Dict[Any, float] = {}
        counts: Dict[Any, int] = {}
        for batch in batches:
            if not all(k in batch for k in REQUIRED_KEYS):
                raise ValueError(f"Batch missing required keys: {REQUIRED_KEYS - set(batch.keys())}")
            lat = batch["vae_latents"].float()
            B = lat.shape[0]
            for t in timesteps:
                key = int(t) if self.method == "ddpm" else float(t)
                noise = torch.randn(lat.shape, generator=generator)
                ts = torch.full((B,), key, dtype=torch.long if self.method == "ddpm" else torch.float32)
                self._forward(batch, lat, noise, ts, generator, {"per_sample_loss": True})
                self.net.read_loss()                                    # the sync; its scalar (tag mean, guard) is not used
                per = self.net.read_per_sample_loss().double()
                sums[key] = sums.get(key, 0.0) + float(per.sum())
                counts[key] = counts.get(key, 0) + B
        if callable(getattr(self.net, "discard_forward", None)):        # no backward follows these forwards: the gradient selection is free again
            self.net.discard_forward()
        per_t = {k: sums[k] / counts[k] for k in sums}
        n = sum(counts.values())
        return per_t, (sum(sums.values()) / n if n else float("nan"))

    training_step = compute_loss                                        # DDPM trainer's name for it

    def _end_cycle(self) -> None:
        self._micro = 0
        self._zeroed = False

    def zero_grad(self, set_to_none: bool = False) -> None:
        """Start a new accumulation cycle (the direct `compute_loss(...)["loss"].backward()` loop calls this or
        `optimizer.step()` between cycles, like the reference's template loop, example_method.py:191-206)."""
        self.net.zero_grads()
        self._micro = 0
        self._zeroed = True

    def _native_backward(self, grad_scale: float) -> None:
        """backward of the 0-d loss: runs from `_execute_training_step` and from a caller-owned
        `compute_loss(batch)["loss"].backward()` loop alike, so the accumulation state lives here."""
        first = self._micro == 0
        if first and not self._zeroed:       # the small-parameter gradients accumulate with atomics: zero them per cycle
            self.net.zero_grads()
        world = self.sync.world
        exchange = self._exchange and self.sync.active
        self.sync.enabled = exchange
        # per-segment joins (side stream -> caller's stream) only on the micro-step that exchanges gradients
        if exchange:    # bucket casts + collectives ride the engine's side stream, behind the segment's weight gradients
            # emit mode (wgrad GEMMs write bf16 straight into the exchange arena, the fp32 arena is NOT written) is only correct
            # on the LAST micro-step of a cycle: a later micro-step would add to an fp32 arena that never received this one.
            # `_execute_training_step` knows that; a caller-owned `compute_loss(...)["loss"].backward()` loop with accumulation does
            # not say which backward is the last, so every one of its micro-steps takes the fp32-accumulate + cast path.
            final = self._final_known or self.gradient_accumulation_steps == 1
            self._emit = final and hasattr(self.net, "set_grad_emit") and self.sync.comm is not None
            if self._emit:
                self.net.set_grad_emit(self.sync.comm, 1.0)
            try:
                self.net.backward(grad_scale / world, first, on_segment=self.sync.on_segment, segment_stream=True)
            finally:
                if self._emit:
                    self.net.set_grad_emit(None)
        else:
            self.net.backward(grad_scale / world, first)
        self._micro += 1
        self._zeroed = False

    # -------------------------------------------------------------------------------- loop pieces
    def _execute_training_step(self, batch, accumulate: bool = False, is_last_accumulation_step: bool = True, **kw):
        N = self.gradient_accumulation_steps if accumulate else 1
        if self._micro == 0:
            self.net.zero_grads()                                      # start of the cycle (D10 repair)
            self._zeroed = True
        self._exchange = (not accumulate) or is_last_accumulation_step
        self._final_known = self._exchange
        out = self.compute_loss(batch, **kw)
        loss = out["loss"] / N if accumulate else out["loss"]
        try:
            loss.backward()
        finally:
            self._final_known = False
        if self._exchange:
            self._end_cycle()
            self.sync.finish()
        self._exchange = True
        return loss.detach() * N, out["metrics"]

    def clip_grad_norm_(self, max_norm: float) -> float:
        """torch.nn.utils.clip_grad_norm_ over the flat arena (flow_matching_trainer.py:181-186).  Under data parallelism
        the norm is taken over the exchanged gradients: the whole all-reduced arena, or (ZeRO-1) this rank's
        reduce-scattered slices + one float all-reduced -- the coefficient is then the same bits on every rank."""
        self.sync.finish()                                   # the asynchronous exchange must have landed
        fused = isinstance(self.optimizer, FusedArenaOptimizer)   # the coefficient rides into the fused optimizer kernel
        g = self.sync.reduced() if self.sync.active else self.net.grads
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream) if g.is_cuda else None
        if g.is_cuda:                                        # squared norm + coefficient on the device (HIP kernels)
            buf = torch.empty(2, dtype=torch.float32, device=g.device)
            n = (g.numel() // 8) * 8
            lib.check(self.net.L.sdxl_sumsq(C.c_void_p(g.data_ptr()), 0 if g.dtype == torch.float32 else 1, n,
                                            C.c_void_p(buf.data_ptr()), st), "sdxl_sumsq")
            if self.sharded and self.sync.active:
                self.sync.global_sumsq(buf[0:1])
            lib.check(self.net.L.sdxl_clip_coef(C.c_void_p(buf.data_ptr()), float(max_norm),
                                                C.c_void_p(buf.data_ptr() + 4), st), "sdxl_clip_coef")
            if fused:
                self._clip_coef = buf[1:2]
            else:
                g.mul_(buf[1])
            return float(buf[0].sqrt())                      # the reference logs the norm (one read-back)
        sq = g.float().pow(2).sum().reshape(1)               # host-logic tests with a stand-in net (no GPU)
        if self.sharded and self.sync.active:
            self.sync.global_sumsq(sq)
        norm = float(sq.sqrt())
        coef = max_norm / (norm + 1e-6) if norm > max_norm else 1.0
        if fused:
            self._clip_coef = torch.tensor([coef], dtype=torch.float32) if coef != 1.0 else None
        elif coef != 1.0:
            g.mul_(coef)
        return norm

    def optimizer_step(self) -> Optional[float]:
        self.sync.finish()
        gn = None
        if self.config.training.clip_grad_norm and self.config.training.clip_grad_norm > 0:
            gn = self.clip_grad_norm_(float(self.config.training.clip_grad_norm))
        if self.optimizer is not None:
            if isinstance(self.optimizer, FusedArenaOptimizer):
                if self.sync.active and self.sharded:        # ZeRO-1: update this rank's slices, then all-gather the parameters
                    self.optimizer.step(self.sync.reduced(), grad_scale=self._clip_coef, pieces=self.sync.pieces)
                    self.sync.gather_params(self.net.weights)
                else:
                    self.optimizer.step(self.sync.reduced() if self.sync.active else None, grad_scale=self._clip_coef)
                self._clip_coef = None
            else:
                self.optimizer.step()
        self._end_cycle()
        return gn

    def train(self, num_epochs: int, save_checkpoints: bool = False, validation_batches=None, on_validation=None) -> None:
        """The template loop.  With training.validation_every_n_steps = N > 0 and `validation_batches` (conditioning only, see
        validate()), every N-th optimizer step is followed by validate(): `on_validation(step, latents)` receives each sampled batch.
          save_checkpoints: the reference's cadence (flow_matching_trainer.py:211-234): a checkpoint
        whenever the epoch's mean loss improves, and `final_checkpoint` at the end (off by default: writing the 5 GB UNet
        is the caller's decision, `SDXLTrainer.save_checkpoint` in the reference)."""
        N = self.gradient_accumulation_steps
        global_step = 0
        best = float("inf")
        every = int(getattr(self.config.training, "validation_every_n_steps", 0)) if validation_batches is not None else 0
        validation_batches = list(validation_batches) if every else None
        opt_steps = 0
        for epoch in range(num_epochs):
            acc_loss, acc_metrics = 0.0, defaultdict(float)
            ep_loss, ep_n = 0.0, 0
            for step, batch in enumerate(self.train_dataloader):
                t0 = time.time()
                last = (step + 1) % N == 0
                loss, metrics = self._execute_training_step(batch, accumulate=True, is_last_accumulation_step=last)
                acc_loss += float(loss)
                ep_loss, ep_n = ep_loss + float(loss), ep_n + 1
                for k, v in metrics.items():
                    acc_metrics[k] += v
                if last:
                    eff = {k: v / N for k, v in acc_metrics.items()}
                    gn = self.optimizer_step()
                    if gn is not None:
                        eff["grad_norm"] = gn
                    eff.update(epoch=epoch + 1, step=global_step, loss=acc_loss / N, step_time=time.time() - t0)
                    if D.is_main_process():
                        if self.wandb_logger is not None:
                            self.wandb_logger.log_metrics(eff, step=global_step)
                        else:
                            print({k: (round(v, 6) if isinstance(v, float) else v) for k, v in eff.items()}, flush=True)
                    acc_loss, acc_metrics = 0.0, defaultdict(float)
                    opt_steps += 1
                    if every and opt_steps % every == 0:
                        self.validate(global_step, validation_batches, on_validation)
                global_step += 1
            if save_checkpoints:
                # the decision must be the same on every rank (each sees its own data): the epoch's loss sum and step count, both summed
                # over ranks -- EVERY rank enters the reduction, also one whose shard produced no step this epoch (an uneven loader
                # shard; a guard on the local count would leave the others waiting in the collective).
                # prepare_checkpoint() is the collective part (every rank), save_checkpoint() itself has none (rank 0 writes).
                tot = D.reduce_dict({"loss_sum": ep_loss, "n": float(ep_n)}, average=False)
                mean = tot["loss_sum"] / tot["n"] if tot["n"] > 0 else float("inf")
                if mean < best:
                    best = mean
                    self.prepare_checkpoint()
                    self.save_checkpoint(epoch + 1, is_final=False)
        # The reference's main.py:108-111 calls save_checkpoint(path) on rank 0 only right after train() returns, when
        # `training.save_final_model` is set (config.yaml:39, the default).  Under ZeRO-1 that save needs every rank's slices of the
        # moments, and save_checkpoint itself may hold no collective -- so the gather (three arenas, every rank) happens here, but only
        # when a save can follow: this loop's own final checkpoint, or the caller's under save_final_model.  Without either, train() ends
        # without any collective beyond the steps', and a rank-0-only save afterwards fails loudly (save_checkpoint) instead of writing
        # a state that could not be resumed.
        if save_checkpoints or bool(getattr(self.config.training, "save_final_model", True)):
            self.prepare_checkpoint()
        if save_checkpoints:
            self.save_checkpoint(num_epochs, is_final=True)

    # -------------------------------------------------------------------------------- weights out (row f4)
    def sync_to_model(self, ema: bool = False) -> None:
        """Write the trained native weights back into the caller's PyTorch UNet (diffusers keys, the module's own dtypes), so
        everything the reference does with `model.unet` afterwards -- `save_pretrained` (models/sdxl.py:246-288), validation
        sampling -- sees them.  ema=True writes the EMA of the weights instead (training.use_ema): `save_pretrained` and
        validation then see the averaged UNet."""
        if self._torch_unet is None:
            return
        sd = self.ema_state_dict() if ema else self.net.state_dict()
        ref = self._torch_unet.state_dict()
        self._torch_unet.load_state_dict({k: v.to(device=ref[k].device, dtype=ref[k].dtype) for k, v in sd.items()}, strict=True)

    def save_checkpoint(self, epoch_or_path=0, is_final: bool = False) -> Optional[Path]:
        """sdxl_trainer.py:162-210: `outputs/checkpoint-<epoch>` or `outputs/final_checkpoint` (main.py:111 passes a
        directory instead of an epoch: accepted too); the model through `model.save_pretrained(dir, safe_serialization=True)`
        when the caller's model has it (weights synced back first), else the UNet as diffusers-keyed safetensors;
        `optimizer.pt` = optimizer.state_dict(); `config.json` = the training config."""
        # No collective in here: the reference calls save_checkpoint on rank 0 only (main.py:110-111, flow_matching_trainer.py:218-219,
        # ddpm_trainer.py:235-237), so a gather at this point would leave rank 0 alone in it.  Under ZeRO-1 the complete optimizer
        # state needs prepare_checkpoint() on EVERY rank first (train() does that); without it optimizer.pt holds rank 0's slices of
        # exp_avg / exp_avg_sq / shift only: that raises (after the weights and config.json were written).
        if not D.is_main_process():
            return None
        save_dir = checkpoint_dir(epoch_or_path, is_final)
        save_dir.mkdir(parents=True, exist_ok=True)
        self.sync_to_model()
        if self._torch_unet is not None and callable(getattr(self.model, "save_pretrained", None)):
            self.model.save_pretrained(str(save_dir), safe_serialization=True)
        else:
            from safetensors.torch import save_file
            (save_dir / "unet").mkdir(exist_ok=True)
            save_file({k: v.cpu().contiguous() for k, v in self.net.state_dict().items()},
                      str(save_dir / "unet" / "diffusion_pytorch_model.safetensors"))
        with open(save_dir / "config.json", "w") as f:
            json.dump(self.config.to_dict(), f, indent=2)
        if self.optimizer is not None and callable(getattr(self.optimizer, "state_dict", None)):
            torch.save(self._optimizer_state_for_save(), str(save_dir / "optimizer.pt"))      # (raises under ZeRO-1 on a stale state)
        self.save_ema_state(save_dir)
        return save_dir

    # -------------------------------------------------------------------------------- EMA of the weights (training.use_ema)
    def ema_state_dict(self) -> Dict[str, torch.Tensor]:
        """the EMA in diffusers keys and shapes, fp32, on the device (through the library's own layout inverse).  Under ZeRO-1 each
        rank's arena is current only on its own slices until prepare_checkpoint() on every rank gathers it: before that (since the
        last optimizer step) this raises instead of returning a partly stale EMA -- and so do sync_to_model(ema=True) and
        save_ema_state, which read the EMA through it."""
        if self.ema is None:
            raise ValueError("ema_state_dict: this trainer keeps no EMA (training.use_ema is false)")
        self._require_gathered("ema_state_dict (also behind sync_to_model(ema=True) and save_checkpoint)", "Nothing was read.")
        return self.ema.state_tensors()

    def save_ema_state(self, save_dir) -> None:
        """`unet_ema/diffusion_pytorch_model.safetensors` (fp32, diffusers keys) and `ema.json` (step and settings) when the EMA
        is on; no collective (see save_checkpoint), and under ZeRO-1 the same stale-state guard as optimizer.pt."""
        if self.ema is None or not D.is_main_process():
            return
        self._require_gathered("save_checkpoint", "The model weights and config.json of this checkpoint were written; unet_ema/ "
                                                  "and ema.json were not.")
        from safetensors.torch import save_file
        d = Path(save_dir)
        (d / "unet_ema").mkdir(parents=True, exist_ok=True)
        save_file({k: v.cpu().contiguous() for k, v in self.ema_state_dict().items()},
                  str(d / "unet_ema" / "diffusion_pytorch_model.safetensors"))
        with open(d / "ema.json", "w") as f:
            json.dump(self.ema.state_dict(), f, indent=2)

    def load_ema_state(self, checkpoint_dir) -> None:
        """resume the EMA from what save_ema_state wrote: the packed arena comes back bit for bit, the step count with it.  The
        settings and the arena size must match this trainer's (ValueError otherwise)."""
        if self.ema is None:
            raise ValueError("load_ema_state: this trainer keeps no EMA (training.use_ema is false)")
        from safetensors.torch import load_file
        d = Path(checkpoint_dir)
        with open(d / "ema.json") as f:
            st = json.load(f)
        tensors = load_file(str(d / "unet_ema" / "diffusion_pytorch_model.safetensors"))
        # every check before anything changes, the step count last: a refused or unreadable checkpoint leaves the EMA as it was
        self.ema.check_state_dict(st)
        self.ema.load_tensors(tensors)
        self.ema.load_state_dict(st)

    def _zero1_active(self) -> bool:
        return bool(self.sharded and self.sync.active and isinstance(self.optimizer, FusedArenaOptimizer) and getattr(self.sync, "buckets", None))

    def prepare_checkpoint(self) -> None:
        """COLLECTIVE -- every rank calls it, at the same point of its loop, before rank 0 calls save_checkpoint().  Under ZeRO-1
        each rank has updated its state arenas (optimizer.state_arenas(): exp_avg / exp_avg_sq / shift or kahan_comp) on its own
        slices only: all-gather them so that the optimizer.pt rank 0 writes holds the complete state.  No-op otherwise.  The
        gathered state stays valid until the next optimizer step."""
        if self._zero1_active():
            for arena in self.optimizer.state_arenas():
                self.sync.gather_arena(arena)
            if self.ema is not None:                 # the EMA is updated on the same slices, inside the same launches
                self.sync.gather_arena(self.ema.arena)
        self._opt_state_step = self._step_counter()

    def _step_counter(self):
        n = getattr(self.optimizer, "step_count", None) if self.optimizer is not None else None
        return n if self.ema is None else (n, self.ema.optimization_step)

    def _require_gathered(self, what: str, consequence: str) -> None:
        """Under ZeRO-1 the state arenas (and the EMA) are current only on this rank's slices until prepare_checkpoint(): refuse
        `what` (a save, or a read of the EMA) on a state that has stepped since the last gather."""
        if self._zero1_active() and getattr(self, "_opt_state_step", object()) != self._step_counter():
            # Surfaces at SAVE time, not at resume time: a file with this rank's slices only could never be loaded again
            # (load_optimizer_state refuses it), and the run that could still have gathered the state would be long gone.
            raise RuntimeError(
                f"{what} under ZeRO-1 without prepare_checkpoint() on every rank since the last optimizer step: this rank "
                f"(rank {int(self.sync.rank)} of {int(self.sync.world)}) holds only its own slices of exp_avg / exp_avg_sq / shift"
                f"{' and of the EMA' if self.ema is not None else ''}. "
                "Call prepare_checkpoint() on EVERY rank first (train() does, before a final save), or train with "
                "training.shard_optimizer = false when the caller's loop saves on rank 0 only (INTEGRATION.md section 3). "
                f"{consequence}")

    def _optimizer_state_for_save(self) -> dict:
        osd = self.optimizer.state_dict()
        if isinstance(osd.get("state"), dict):
            osd["state"] = {k: (v.cpu() if torch.is_tensor(v) else v) for k, v in osd["state"].items()}
        self._require_gathered("save_checkpoint", "The model weights and config.json of this checkpoint were written; optimizer.pt"
                               + (", unet_ema/ and ema.json were not." if self.ema is not None else " was not."))
        return osd

    def save_optimizer_state(self, save_dir) -> None:
        """optimizer.pt of the NATIVE fused optimizer.  No collective (see save_checkpoint): complete under ZeRO-1 after
        prepare_checkpoint() on every rank."""
        if not D.is_main_process() or self.optimizer is None or not callable(getattr(self.optimizer, "state_dict", None)):
            return
        torch.save(self._optimizer_state_for_save(), str(Path(save_dir) / "optimizer.pt"))

    def load_optimizer_state(self, checkpoint_dir) -> None:
        """resume: optimizer.pt written by save_checkpoint (the UNet weights come back through the model object).  The state
        holds tensors, numbers and dicts only, so the safe loader is enough."""
        sd = torch.load(str(Path(checkpoint_dir) / "optimizer.pt"), map_location="cpu", weights_only=True)
        part = sd.pop("zero1_partial", None) if isinstance(sd, dict) else None
        if part is not None:
            # written under ZeRO-1 without prepare_checkpoint() on every rank (the drop-in path: the reference's loop calls
            # save_checkpoint on rank 0 only): the moments of the other ranks' slices in it are stale.  Resuming from it would be
            # silently wrong on (world - 1) / world of the arena -- refuse.
            raise ValueError(
                f"optimizer.pt is a ZeRO-1 partial state (rank {part.get('rank')} of {part.get('world')}: only that rank's slices of "
                "exp_avg / exp_avg_sq / shift are current). Call prepare_checkpoint() on every rank before save_checkpoint(), or train "
                "with training.shard_optimizer = false when the caller's loop saves on rank 0 only (INTEGRATION.md section 3)")
        self.optimizer.load_state_dict(sd)


def build_optimizer(net, oc):
    """The fused optimizer `optimizer_type` names (case-insensitive, as the reference's OptimizerConfig.class_name;
    main.py:73-86 builds it from config.optimizer.kwargs).  A type this build has no fused kernel for ("soap", "adamw", ...)
    trains with AdamWBF16, and the warning names it."""
    kind = str(getattr(oc, "optimizer_type", "adamw_bf16")).lower()
    cls = BY_TYPE.get(kind)
    if cls is None:
        logger.warning("optimizer_type %r has no fused implementation in this build: training with AdamWBF16 (adamw_bf16) instead",
                       getattr(oc, "optimizer_type", None))
        cls = AdamWBF16
    return cls.from_config(net, oc)


def build_ema(net, optimizer, tc) -> Optional[WeightEMA]:
    """The fp32 EMA of the weights when `training.use_ema` is set (after the weights are loaded: it starts as their fp32 image),
    attached to the fused optimizer whose kernel updates it; None otherwise."""
    if not bool(getattr(tc, "use_ema", False)):
        return None
    if not isinstance(optimizer, FusedArenaOptimizer):
        raise ValueError(f"training.use_ema needs one of the fused optimizers ({', '.join(c.__name__ for c in BY_TYPE.values())}): the EMA "
                         f"update runs inside their kernel, and {type(optimizer).__name__} has none")
    ema = WeightEMA(net, decay=float(getattr(tc, "ema_decay", 0.9999)), min_decay=float(getattr(tc, "ema_min_decay", 0.0)),
                    update_after_step=int(getattr(tc, "ema_update_after_step", 0)),
                    use_ema_warmup=bool(getattr(tc, "ema_use_warmup", False)), inv_gamma=float(getattr(tc, "ema_inv_gamma", 1.0)),
                    power=float(getattr(tc, "ema_power", 2 / 3)))
    optimizer.attach_ema(ema)
    return ema


def checkpoint_dir(epoch_or_path, is_final: bool = False) -> Path:
    """The directory sdxl_trainer.py:171-178 writes a checkpoint to: `outputs/final_checkpoint` or `outputs/checkpoint-<epoch:04d>`
    (relative to the working directory, as in the reference); a path is taken as it is (main.py:111)."""
    if isinstance(epoch_or_path, (str, bytes, Path)) or hasattr(epoch_or_path, "__fspath__"):
        return Path(epoch_or_path)
    return Path("outputs") / ("final_checkpoint" if is_final else f"checkpoint-{int(epoch_or_path):04d}")


def create_trainer(model, optimizer=None, train_dataloader=None, device=None, wandb_logger=None, config=None, **kw):
    """BaseRouter.create equivalent for model_type == "sdxl" (base_router.py:48-84)."""
    if config is not None and str(config.model.model_type).lower() != "sdxl":
        raise ValueError(f"Unsupported model type: {config.model.model_type}")
    rank = getattr(config.training, "lora_rank", 0) if config is not None else 0
    if isinstance(rank, bool) or not isinstance(rank, int) or rank < 0:
        raise ValueError(f"training.lora_rank must be an integer >= 0 (got {rank!r})")
    if rank > 0:                       # LoRA adapters on a frozen UNet (lora.py)
        from .lora import NativeLoRATrainer
        return NativeLoRATrainer(model, optimizer, train_dataloader, device, wandb_logger, config, **kw)
    return NativeSDXLTrainer(model, optimizer, train_dataloader, device, wandb_logger, config, **kw)
