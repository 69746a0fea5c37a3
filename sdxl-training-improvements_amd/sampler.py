"""Native latent sampler: N UNet forwards with one fused HIP step between them, the state on the device in fp32.

Every solver here is one generic step (include/sdxlstep.h `sdxl_sampler_step`, csrc/sampler.hip), fp32, each operation rounded
on its own:

    F       = F_c  |  F_u + g * (F_c - F_u)                     guidance (and guidance rescale, see the header)
    den     = a_skip * x + a_out * F                            the denoiser
    x_next  = p * x + q * den                                   the solver step
    in_next = bf16(clamp(a_in_next * x_next, +-clamp))          the next UNet input

and a parameter set is a host function that returns, per forward, `(a_in, a_skip, a_out, p, q, clamp, timestep)`: the scaling and clamp
of THAT forward's input, the step taken behind it, and the value its time embedding is fed.

ddpm, parameterization "trained" (default) -- the denoiser the loss of this build trains (csrc/loss.hip).  Training feeds
the UNet x_t = clamp(x0 + sigma * n, +-20000), unscaled, with the table INDEX as time input, against

    v_prediction  v   = (n - x0) / sigma      =>  n = x0 + sigma v,  x_t = (1 + sigma) x0 + sigma^2 v,  x0 = x_t / (1 + sigma) - sigma^2 / (1 + sigma) v
    epsilon       eps = n                     =>  x0 = x_t - sigma eps

so a_in = 1 (clamp 20000 under use_ztsnr), a_skip = 1 / (1 + sigma), a_out = -sigma^2 / (1 + sigma) (v) or a_skip = 1, a_out = -sigma (epsilon).
The probability-flow ODE of x_t = x0 + sigma n is dx / dsigma = (x - den) / sigma; one Euler step from sigma to sigma' gives
x' = x + (sigma' - sigma) (x - den) / sigma = (sigma' / sigma) x + (1 - sigma' / sigma) den: p = sigma' / sigma, q = 1 - p.  The grid is
idx_j = round(999 j / (N - 1)) of the training table (sigma_0 = sigma_max first), so the model only sees points it was trained at; the
state starts as sigma_0 * n and the last step goes to sigma = 0 (p = 0, q = 1: x = den).  tests/test_host_sampler.py proves that an
ideal model -- one that returns the training target of a fixed x* -- is sampled back to x*.

ddpm, parameterization "reference" -- training/schedulers/novelai_v3.py:59-99 as written: the first forward is `ztsnr_first_step` on the
state n (a_in = 1, a_skip = 0, a_out = -sigma_data, p = sigma_0, q = 1), the others are `euler_step` from sigma_{j-1} to sigma_j with the
Karras scalings of `get_karras_scalings` (a_in = c_in, a_skip = c_skip, a_out = c_out, no clamp, p = sigma_j / sigma_{j-1}, q = 1 - p), and
there is no step to sigma = 0.  It is NOT the denoiser of the reference's own training: that training never scales the UNet input (c_in)
and regresses (n - x0) / sigma, not the EDM target the scalings belong to, so the ideal model above is not sampled back to x* (the same
test pins the gap).  It exists for fidelity.  The reference's functions are restated operation for operation in tests/_sampler_ref.py
and held to recorded outputs bit for bit; its euler_step computes x + (sigma' - sigma) * ((x - den) / sigma), which the generic step
reproduces to fp32 rounding, not to the bit (p x + q den is a different order of the same arithmetic).  The reference leaves the
mapping from sigma to the UNet's time input to its `model_fn` (it passes sigma itself, inf on the first step): here the time input is
the table index of each sigma, as in training.

flow_matching -- the model predicts the velocity x1 - x0 at x_t = (1 - t) x0 + t x1: den = F (a_skip = 0, a_out = 1), p = 1,
q = t_{j+1} - t_j on t_j = j / N, a_in = 1, the state starts as the noise x0 and t is the time input (rounded to bf16 where training
rounds it).

VAE decode and text encoding are the caller's, as all preconditioning is."""
from __future__ import annotations

import math
from typing import List, Optional, Sequence, Tuple

import torch

from .scheduler import NoiseScheduler

METHODS = ("ddpm", "flow_matching")
PREDICTION_TYPES = ("epsilon", "v_prediction")
PARAMETERIZATIONS = ("trained", "reference")

Step = Tuple[float, float, float, float, float, float, float]      # (a_in, a_skip, a_out, p, q, clamp, timestep)


def ddpm_indices(num_steps: int, num_timesteps: int = 1000) -> List[int]:
    """the default ddpm grid: idx_j = round((T - 1) j / (N - 1)), j = 0..N-1 (index 0 is sigma_max)"""
    if int(num_steps) < 2:
        raise ValueError(f"num_steps must be >= 2 for ddpm (got {num_steps})")
    N, T = int(num_steps), int(num_timesteps)
    return [int(math.floor((T - 1) * j / (N - 1) + 0.5)) for j in range(N)]


def karras_scalings(sigma: float, sigma_data: float = 1.0) -> Tuple[float, float, float]:
    """get_karras_scalings (novelai_v3.py:59-64) in double precision: (c_skip, c_out, c_in)"""
    s2 = sigma * sigma + sigma_data * sigma_data
    return sigma_data * sigma_data / s2, -sigma * sigma_data / math.sqrt(s2), 1.0 / math.sqrt(s2)


def ddpm_trained_steps(sigmas: Sequence[float], timesteps: Sequence[float], prediction_type: str = "v_prediction",
                       use_ztsnr: bool = True) -> Tuple[float, List[Step]]:
    """(scale of the initial noise, steps): one forward per sigma, Euler to the next sigma, the last one to 0"""
    sig = [float(s) for s in sigmas]
    if len(sig) < 1 or len(timesteps) != len(sig) or any(not s > 0.0 for s in sig):
        raise ValueError("ddpm schedule: sigmas must be positive and timesteps must have one value per sigma")
    clamp = 20000.0 if use_ztsnr else 0.0
    steps = []
    for j, s in enumerate(sig):
        nxt = sig[j + 1] if j + 1 < len(sig) else 0.0
        if prediction_type == "v_prediction":
            a_skip, a_out = 1.0 / (1.0 + s), -s * s / (1.0 + s)
        else:
            a_skip, a_out = 1.0, -s
        p = nxt / s
        steps.append((1.0, a_skip, a_out, p, 1.0 - p, clamp, float(timesteps[j])))
    return sig[0], steps


def ddpm_reference_steps(sigmas: Sequence[float], timesteps: Sequence[float], sigma_data: float = 1.0) -> Tuple[float, List[Step]]:
    """sample_with_ztsnr (novelai_v3.py:86-99): ztsnr_first_step on n, then euler_step(sigma_{j-1} -> sigma_j); N forwards for N sigmas"""
    sig = [float(s) for s in sigmas]
    if len(sig) < 1 or len(timesteps) != len(sig) or any(not s > 0.0 for s in sig):
        raise ValueError("ddpm schedule: sigmas must be positive and timesteps must have one value per sigma")
    steps = [(1.0, 0.0, -sigma_data, sig[0], 1.0, 0.0, float(timesteps[0]))]
    for j in range(1, len(sig)):
        c_skip, c_out, c_in = karras_scalings(sig[j - 1], sigma_data)
        p = sig[j] / sig[j - 1]
        steps.append((c_in, c_skip, c_out, p, 1.0 - p, 0.0, float(timesteps[j - 1])))
    return 1.0, steps


def flow_steps(num_steps: int, timesteps: Optional[Sequence[float]] = None, t_bf16: bool = True) -> Tuple[float, List[Step]]:
    """t_j = j / N (or the N + 1 explicit grid points `timesteps`): x += (t_{j+1} - t_j) F, the state starts as the noise"""
    if timesteps is None:
        if int(num_steps) < 1:
            raise ValueError(f"num_steps must be >= 1 for flow matching (got {num_steps})")
        grid = [j / int(num_steps) for j in range(int(num_steps) + 1)]
    else:
        grid = [float(t) for t in timesteps]
        if len(grid) < 2:
            raise ValueError("flow schedule: timesteps needs at least two grid points")
    steps = []
    for j in range(len(grid) - 1):
        t = grid[j]
        if t_bf16:
            t = float(torch.tensor(t, dtype=torch.float32).to(torch.bfloat16))
        steps.append((1.0, 0.0, 1.0, 1.0, grid[j + 1] - grid[j], 0.0, t))
    return 1.0, steps


def nearest_indices(table: torch.Tensor, sigmas: Sequence[float]) -> List[int]:
    """index of the table entry closest (in log sigma) to each sigma: the time input of an explicit sigma"""
    lt = table.double().log()
    return [int((lt - math.log(float(s))).abs().argmin()) for s in sigmas]


def kernel_steps(steps: Sequence[Step], guidance_scale: float, guidance_rescale: float, cfg: bool):
    """the scalar fields of sdxl_sampler_step per forward: the step itself and the input scaling of the NEXT forward (the last
    forward's input image is not read again: a_in_next = 1, no clamp)"""
    out = []
    for j, (_a_in, a_skip, a_out, p, q, _clamp, _t) in enumerate(steps):
        a_in_next, clamp_next = (steps[j + 1][0], steps[j + 1][5]) if j + 1 < len(steps) else (1.0, 0.0)
        out.append(dict(cfg=int(cfg), init=0, a_skip=a_skip, a_out=a_out, p=p, q=q, a_in_next=a_in_next, clamp=clamp_next,
                        guidance=float(guidance_scale) if cfg else 1.0, guidance_rescale=float(guidance_rescale)))
    return out


class NativeSampler:
    """sample(...) -> latents [B,4,H,W] fp32 on the device.  `unet` is a NativeUNet (its bound weight arena is what is sampled)."""

    def __init__(self, unet, method: str = "ddpm", prediction_type: str = "v_prediction", use_ztsnr: bool = True,
                 parameterization: str = "trained", config=None, t_bf16: bool = True):
        method, prediction_type, parameterization = str(method).lower(), str(prediction_type).lower(), str(parameterization).lower()
        for key, val, known in (("method", method, METHODS), ("prediction_type", prediction_type, PREDICTION_TYPES),
                                ("parameterization", parameterization, PARAMETERIZATIONS)):
            if val not in known:
                raise ValueError(f"sampler {key}: unknown value {val!r} (expected one of {', '.join(known)})")
        self.unet = unet
        self.method, self.prediction_type, self.parameterization = method, prediction_type, parameterization
        self.use_ztsnr, self.t_bf16 = bool(use_ztsnr), bool(t_bf16)
        if config is None:
            from .config import Config
            config = Config()
            config.model.use_ztsnr = self.use_ztsnr
        self.table = NoiseScheduler(config, "cpu").sigmas                 # the training table (fp32)

    # ------------------------------------------------------------------ the schedule
    def schedule(self, num_steps: int, sigmas=None, timesteps=None) -> Tuple[float, List[Step]]:
        """(scale of the initial noise, steps) of this sampler; explicit `sigmas` / `timesteps` override the default grid"""
        if self.method == "flow_matching":
            if sigmas is not None:
                raise ValueError("flow matching has no sigmas: pass the grid as timesteps")
            return flow_steps(num_steps, None if timesteps is None else [float(t) for t in timesteps], self.t_bf16)
        if sigmas is None:
            idx = ddpm_indices(num_steps, self.table.numel()) if timesteps is None else [int(t) for t in timesteps]
            sig = [float(self.table[i]) for i in idx]
            ts = [float(i) for i in idx]
        else:
            sig = [float(s) for s in sigmas]
            ts = [float(t) for t in timesteps] if timesteps is not None else [float(i) for i in nearest_indices(self.table, sig)]
        if self.parameterization == "reference":
            return ddpm_reference_steps(sig, ts)
        return ddpm_trained_steps(sig, ts, self.prediction_type, self.use_ztsnr)

    @staticmethod
    def plan_batch(B: int, guidance_scale: float) -> int:
        """the batch of the UNet plan: B without guidance (guidance_scale == 1), else 2B = [cond; uncond]"""
        return int(B) if float(guidance_scale) == 1.0 else 2 * int(B)

    # ------------------------------------------------------------------ the loop
    def sample(self, prompt_embeds, pooled, time_ids, neg_prompt_embeds=None, neg_pooled=None, neg_time_ids=None, *,
               height: int, width: int, num_steps: int, guidance_scale: float = 1.0, guidance_rescale: float = 0.0,
               generator: Optional[torch.Generator] = None, noise: Optional[torch.Tensor] = None, sigmas=None,
               timesteps=None) -> torch.Tensor:
        """height / width are the latent's.  Negative conditioning that is missing with guidance_scale != 1 is zeros of the same
        shape (neg_time_ids: the positive ones).  `noise` [B,4,H,W] overrides the draw from `generator` (CPU, as in training).  The
        loop enqueues every forward and step without a host synchronisation; the result is stream-ordered."""
        net = self.unet
        dev = net.device
        B = int(prompt_embeds.shape[0])
        H, W = int(height), int(width)
        if not 0.0 <= float(guidance_rescale) <= 1.0:
            raise ValueError(f"guidance_rescale must be in [0, 1] (got {guidance_rescale})")
        cfg = float(guidance_scale) != 1.0
        x0_scale, steps = self.schedule(num_steps, sigmas, timesteps)
        if noise is None:
            noise = torch.randn((B, 4, H, W), generator=generator)
        if tuple(noise.shape) != (B, 4, H, W):
            raise ValueError(f"noise: expected shape {(B, 4, H, W)}, got {tuple(noise.shape)}")
        x = noise.to(torch.float32)
        if x0_scale != 1.0:
            x = torch.tensor(x0_scale, dtype=torch.float32, device=x.device) * x     # sigma_0 * n: one fp32 product where the noise lives, before the loop
        x = x.to(dev).contiguous()
        if x.data_ptr() == noise.data_ptr():
            x = x.clone()                                                             # the state is updated in place: never the caller's tensor
        pe = prompt_embeds.to(dev, torch.bfloat16)
        po = pooled.to(dev, torch.bfloat16).reshape(B, -1)
        ti = time_ids.to(dev, torch.float32).reshape(B, 6)
        if cfg:
            npe = torch.zeros_like(pe) if neg_prompt_embeds is None else neg_prompt_embeds.to(dev, torch.bfloat16)
            npo = torch.zeros_like(po) if neg_pooled is None else neg_pooled.to(dev, torch.bfloat16).reshape(B, -1)
            nti = ti if neg_time_ids is None else neg_time_ids.to(dev, torch.float32).reshape(B, 6)
            pe, po, ti = torch.cat([pe, npe]), torch.cat([po, npo]), torch.cat([ti, nti])
        PB = self.plan_batch(B, guidance_scale)
        # the time inputs of all forwards, uploaded once: row j is forward j's [PB] values
        tall = torch.tensor([[s[6]] * PB for s in steps], dtype=torch.float32).to(dev)
        ks = kernel_steps(steps, guidance_scale, guidance_rescale, cfg)
        net.sample_init(x, pe, po, ti, tall[0], cfg=cfg, a_in=steps[0][0], clamp=steps[0][5])
        for j, k in enumerate(ks):
            net.sample_step(x, pe, po, ti, tall[j], **k)
        return x
