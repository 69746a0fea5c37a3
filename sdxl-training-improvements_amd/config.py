"""config.yaml -> dataclasses, restricted to the keys the hot path reads (reference: src/data/config.py).

Same loading rule as the reference's Config.from_yaml (data/config.py:327-420): start from defaults, overlay only
keys that exist, ignore unknown keys silently, missing file -> defaults.  Shipped defaults = src/config.yaml."""
from __future__ import annotations

from dataclasses import asdict, dataclass, field, fields, is_dataclass
from pathlib import Path
from typing import List, Optional, Tuple, Union

import yaml


@dataclass
class ModelConfig:                       # data/config.py:11-22
    pretrained_model_name: str = "stabilityai/stable-diffusion-xl-base-1.0"
    model_type: str = "sdxl"
    prediction_type: str = "v_prediction"
    num_timesteps: int = 1000
    sigma_min: float = 0.002
    sigma_max: float = 20000.0
    use_ztsnr: bool = True
    min_snr_gamma: Optional[float] = 5.0
    rho: float = 7.0                     # D1: read by novelai_v3.py:107 but absent from the reference dataclass


@dataclass
class OptimizerConfig:                   # data/config.py:42-49
    learning_rate: float = 1e-6
    weight_decay: float = 0.01
    beta1: float = 0.9
    beta2: float = 0.999
    epsilon: float = 1e-8
    optimizer_type: str = "adamw_bf16"
    reference_ema: bool = True           # build-only key: True = the reference's actual first-moment update (its
                                         # add_stochastic_ operand order, SURVEY D17: almost no momentum), False = the
                                         # documented EMA; see optimizer.py::AdamWBF16
    # schedule-free specific options (data/config.py:51-54), read by optimizer_type "adamw_schedule_free_kahan"
    warmup_steps: int = 0
    kahan_sum: bool = True
    correct_bias: bool = True            # accepted and ignored (the reference class has no such option)
    schedule_free_arithmetic: str = "compensated"   # build-only key: "compensated" = the Kahan-compensated fp32 update the
                                         # reference's docstring describes, "reference" = its literal bf16 arithmetic bit for
                                         # bit; see optimizer.py::AdamWScheduleFreeKahanBF16
    # build-only keys, read by optimizer_type "prodigy" (optimizer.py::ProdigyBF16; the prodigyopt package's arguments).  With it
    # learning_rate is the multiplier on the estimated step size d: set it to 1.0 (a value below 1e-2 is warned about)
    prodigy_d0: float = 1e-6             # the initial estimate of d
    prodigy_d_coef: float = 1.0          # multiplies the estimate
    prodigy_growth_rate: float = float("inf")   # d grows by at most this factor per step (inf = unbounded)
    prodigy_beta3: Optional[float] = None       # the decay of the estimate's sums; None = sqrt(beta2)
    prodigy_use_bias_correction: bool = False   # Adam's bias correction in the step size
    prodigy_safeguard_warmup: bool = False      # leave lr out of the denominator's sum (for a schedule with a warm-up)
    # build-only keys, read by optimizer_type "adafactor" (optimizer.py::AdafactorBF16; the arguments and defaults of
    # transformers.optimization.Adafactor).  The published SDXL full fine-tune recipe is scale_parameter: false, relative_step: false,
    # learning_rate: 4.0e-7, weight_decay: 0.  beta1 and weight_decay above keep their own defaults: the first moment is
    # adafactor_beta1 (None = no first moment, as in the class), the decay is weight_decay (set it to 0 for the class's default)
    eps: Tuple[float, float] = (1e-30, 1e-3)    # (added to the squared gradient, floor of the parameter RMS under scale_parameter)
    clip_threshold: float = 1.0          # the update of a tensor is divided by max(1, rms(update) / clip_threshold)
    decay_rate: float = -0.8             # beta2 of step k is 1 - k^decay_rate
    adafactor_beta1: Optional[float] = None     # the first moment's decay; None = none is kept
    scale_parameter: bool = True         # multiply the step size by max(eps[1], rms(parameter)) per tensor
    relative_step: bool = True           # the step size is min(1e-2, 1/sqrt(k)) and learning_rate must stay at its default
    warmup_init: bool = False            # with relative_step: min(1e-6 * k, 1/sqrt(k))


@dataclass
class TrainingConfig:                    # data/config.py:152-168
    method: str = "ddpm"                 # "ddpm" | "flow_matching" (sdxl_trainer.py:128-152)
    num_epochs: int = 10
    batch_size: int = 4
    gradient_accumulation_steps: int = 1
    mixed_precision: str = "bf16"
    enable_xformers: bool = True         # accepted, meaningless here (attention is the HIP flash kernel)
    prediction_type: str = "v_prediction"
    clip_grad_norm: float = 1.0
    num_workers: int = 4
    save_final_model: bool = True        # data/config.py:170, config.yaml:39: main.py:108 saves on rank 0 after train() when set
    shard_optimizer: Optional[bool] = None   # build-only key (None = not given = True): data parallel = ZeRO-1 (reduce-scatter -> sharded fused AdamW ->
                                         # all-gather) instead of all-reduce + a full update on every rank
    force_exchange: bool = False         # build-only key: drive the gradient exchange through the backend even at world size 1
                                         # (one-GPU RCCL test, tests/test_gpu_rccl.py); SDXL_FORCE_EXCHANGE=1 does the same
    # build-only keys: an fp32 EMA of the UNet weights updated inside the fused optimizer kernel (diffusers' EMAModel, the SDXL
    # script's --use_ema); see ema.py::WeightEMA for the rule.  Needs a fused optimizer.
    use_ema: bool = False
    ema_decay: float = 0.9999            # upper bound of the decay
    ema_min_decay: float = 0.0           # lower bound of the decay
    ema_update_after_step: int = 0       # optimizer steps during which the EMA just copies the weights
    ema_use_warmup: bool = False         # the power warm-up schedule instead of (1+k)/(10+k)
    ema_inv_gamma: float = 1.0           # warm-up parameter
    ema_power: float = 2 / 3             # warm-up parameter
    # build-only keys: per-sample weights, per-sample losses and the element loss of the device loss (csrc/loss.hip); the B floats
    # each recipe needs are computed on the host (trainer.py::NativeSDXLTrainer._loss_ext).  Defaults = the reference's objective.
    loss_type: str = "l2"                # "l2" | "huber" | "smooth_l1" (pseudo-Huber forms, include/sdxlstep.h)
    huber_c: float = 0.1                 # the constant c, or the floor of the schedule
    huber_schedule: str = "constant"     # "constant": c_b = huber_c ; "snr" (ddpm only): c_b = (1 - huber_c) / (1 + sigma_b)^2 + huber_c
    snr_weighting: str = "reference"     # "reference": min(snr, gamma) ; "debiased" (ddpm, needs min_snr_gamma): additionally
                                         # 1 / (snr + 1) for v_prediction, 1 / snr for epsilon (diffusers' --snr_gamma rule)
    tag_weights_per_sample: bool = False # True: batch["tag_weights"] weights each image's own loss instead of the batch mean
    log_per_sample_loss: bool = False    # True: compute_loss also returns "per_sample_loss" (CPU [B]) and "timesteps"
    # build-only keys: masked loss and the training-only augmentations (trainer.py::NativeSDXLTrainer._loss_ext / _augment); the extra
    # draws come from the step's generator after the base noise and the timesteps, in this order, each only when its key is on
    masked_loss: str = "off"             # "off" | "mean" | "masked_mean": batch["loss_mask"] ([B,H,W] / [B,1,H,W], latent resolution)
                                         # goes to the device loss; "masked_mean" divides each sample by its own mask sum
    noise_offset: float = 0.0            # >= 0: noise += noise_offset * randn(B,4,1,1); the target uses the offset noise (diffusers)
    input_perturbation: float = 0.0      # >= 0: the UNet input is built from noise + gamma * randn(B,4,H,W), the target from noise
    cond_dropout_prob: float = 0.0       # in [0,1]: per sample, prompt_embeds / pooled_prompt_embeds zeroed on a copy (time_ids kept)
    # build-only keys: extra UNet input channels (model in_channels > 4; trainer.py::NativeSDXLTrainer._input_cond): what fills channels 4..
    input_conditioning: str = "none"     # "none" (in_channels 4) | "inpaint" (9): cat(batch["inpaint_mask"] [B,1,H,W] / [B,H,W],
                                         # batch["masked_latents"] [B,4,H,W]), diffusers' channel order | "concat": batch["cond_latents"]
                                         # [B, in_channels - 4, H, W] (InstructPix2Pix: the source-image latents, in_channels 8)
    input_cond_dropout_prob: float = 0.0 # in [0,1]: per sample, the extra channels zeroed on a copy (training only; drawn after every other draw)
    # build-only key: conditioning gradients (csrc/cond_dgrad.hip).  "auto": a batch["prompt_embeds"] / batch["pooled_prompt_embeds"] that
    # requires grad gets d loss / d itself back through compute_loss(...)["loss"].backward() (text encoders, textual inversion); "off": never
    conditioning_grads: str = "auto"
    # build-only keys: validation sampling with the native sampler (sampler.py) from train(); decoding the latents is the caller's
    validation_every_n_steps: int = 0    # sample the caller's validation_batches every N optimizer steps (0 = off)
    validation_num_steps: int = 30       # UNet forwards per sample
    validation_guidance_scale: float = 5.0   # classifier-free guidance (1 = none: the plan runs at B instead of 2B)
    validation_guidance_rescale: float = 0.0 # guidance rescale phi in [0, 1]
    validation_weights: Optional[str] = None # "trained" | "ema"; None = "ema" when use_ema, else "trained"
    validation_seed: int = 0             # seed of the validation noise (the same noise at every validation)
    validation_sampler: str = "euler"    # "euler" | "euler_a" | "dpmpp_2m" | "heun" (sampler.py: euler_a / dpmpp_2m need ddpm, all but euler
                                         # the "trained" parameterization; checked when the trainer is built)
    validation_eta: float = 1.0          # euler_a only: the share of each step's noise that is drawn afresh (0 = euler), >= 0
    sampler_parameterization: str = "trained"   # ddpm: "trained" = the denoiser this build's loss trains, "reference" = the
                                         # reference's sample_with_ztsnr as written (inconsistent with its own training; sampler.py)
    # build-only keys: LoRA adapters on a frozen UNet by merge and project (lora.py, csrc/lora.hip); create_trainer picks
    # lora.NativeLoRATrainer when lora_rank > 0.  Not with use_ema, nor with shard_optimizer: true given explicitly.
    lora_rank: int = 0                   # 0 = off, else 1 .. 128
    lora_alpha: Optional[float] = None   # None = rank: s = alpha / rank = 1, the reference's default multiplier
    lora_targets: Optional[List[str]] = None   # module-path suffixes; None = to_q, to_k, to_v, to_out.0
    lora_seed: int = 0                   # seed of the A ~ N(0, (1 / rank)^2) initialisation (B = 0)
    lora_save_merged: bool = False       # save_checkpoint also writes the merged UNet
    # what the backward computes for the adapters (lora.LORA_BACKWARDS): "project" = every weight gradient, then the projection (the
    # default); "project_frozen" = only the ops that hold a target form their weight gradient, projected as before; "direct" = no weight
    # gradient at all, dA and dB come out of the backward itself (csrc/lora_grad.hip)
    lora_backward: str = "project"
    # which tensors may carry an adapter (lora.LORA_TARGET_KINDS): "plain" = 2-D linears stored as plain rows (the default); "all" = also
    # ff.net.0.proj and the convolutions (3x3 and 1x1; LoCon), through SDXL_DTYPE_LORA_LAYOUTS.  Not conv_in; not with lora_backward "direct"
    lora_target_kinds: str = "plain"
    # the adapter family (lora.LORA_ALGOS): "lora" = dW = s B A (the default); "loha" = LyCORIS' Hadamard product dW = s (B1 A1) .* (B2 A2),
    # four factors per target through SDXL_DTYPE_LOHA (csrc/loha.hip), lora_rank 1 .. 64, lora_backward "project" or "project_frozen";
    # lora_target_kinds keeps deciding which tensors the patterns may resolve to
    lora_algo: str = "lora"
    # "dora" = DoRA, LoRA's A and B plus a trained magnitude per output row, through SDXL_DTYPE_DORA (csrc/dora.hip), lora_rank 1 .. 128,
    # lora_backward "project" or "project_frozen"; weight decay pulls the magnitude towards the checkpoint's row norm, not towards 0
    # "kronecker" = LyCORIS' LoKr, dW = s kron(C, W2) through SDXL_DTYPE_LOKR (csrc/lokr.hip), lora_rank 1 .. 128, lora_backward "project" or
    # "project_frozen".  (The value is not "lokr": that string is pinned as an unknown algorithm by an existing test.)
    # lokr_factor: -1 (the most balanced divisor pair of each dimension) or a positive integer (LyCORIS' `factor`; 8 is the usual recipe);
    # lokr_full: store every second factor W2 in full; false = per target, full when 2 lora_rank >= max(out_k, in_n), else W2 = B A
    lokr_factor: int = -1
    lokr_full: bool = False


@dataclass
class ImageConfig:                       # data/config.py:182-199
    supported_dims: List[List[int]] = field(default_factory=lambda: [
        [640, 1536], [768, 1344], [832, 1216], [896, 1152], [1024, 1024], [1152, 896], [1216, 832], [1344, 768],
        [1536, 640]])


@dataclass
class GlobalConfig:
    image: ImageConfig = field(default_factory=ImageConfig)


@dataclass
class Config:
    model: ModelConfig = field(default_factory=ModelConfig)
    optimizer: OptimizerConfig = field(default_factory=OptimizerConfig)
    training: TrainingConfig = field(default_factory=TrainingConfig)
    global_config: GlobalConfig = field(default_factory=GlobalConfig)

    def to_dict(self):
        return asdict(self)

    @classmethod
    def from_yaml(cls, path: Union[str, Path]) -> "Config":
        path = Path(path)
        cfg = cls()
        if not path.exists():
            return cfg
        raw = yaml.safe_load(path.read_text()) or {}
        _overlay(cfg, raw)
        return cfg


def _overlay(obj, data):
    if not isinstance(data, dict):
        return
    names = {f.name for f in fields(obj)}
    for k, v in data.items():
        if k not in names:
            continue                      # unknown keys ignored (data/config.py:351-360)
        cur = getattr(obj, k)
        if is_dataclass(cur):
            _overlay(cur, v)
        else:
            setattr(obj, k, v)
