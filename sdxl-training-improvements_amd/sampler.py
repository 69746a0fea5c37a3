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

Solvers.  The extended step (sdxl_sampler_step_ext) adds three optional terms and two optional saves to the solver line,

    x_next = p * x + q * den [+ r * hist] [+ u * xsave] [+ s * noise] ;  hist <- den (save & 1) ;  xsave <- x (save & 2)

and `solver_steps` expands a schedule into one such step per forward.  With sigma this forward's level, sigma' the next one's and
p = sigma' / sigma (doubles on the host):

    euler     as above: one forward per grid point, nothing new is read
    euler_a   ancestral Euler (k-diffusion's sample_euler_ancestral): sigma_up = min(sigma', eta sqrt(sigma'^2 (sigma^2 - sigma'^2) / sigma^2)),
              sigma_down = sqrt(sigma'^2 - sigma_up^2); p = sigma_down / sigma, q = 1 - p, s = sigma_up on a fresh normal draw per step;
              the last step (to 0) is Euler, eta = 0 is Euler
    dpmpp_2m  k-diffusion's sample_dpmpp_2m: h = ln sigma - ln sigma', rho = h_prev / h, q = (1 - p) (1 + 1 / (2 rho)),
              r = -(1 - p) / (2 rho) on hist = the previous step's den; every step saves its den; the first and the last are Euler
    heun      two forwards per interval.  A: the Euler step, saving den_A and x.  B: a forward on the predicted state at the NEXT grid
              point (its time input and scalings), then with c = (sigma' - sigma) / 2: p = c / sigma', q = -c / sigma', r = -c / sigma,
              u = 1 + c / sigma, i.e. x + c ((x - den_A) / sigma + (x~ - den_B) / sigma').  Flow matching, dt = t' - t: A is Euler,
              B has p = 0, q = dt / 2, r = dt / 2, u = 1.  The last interval is one Euler step.

euler_a and dpmpp_2m are defined on the ddpm sigma, heun on it and on flow matching; all need the "trained" parameterization (the
reference's set puts each forward one grid point behind its step).  Anything else raises ValueError.

img2img starts from `init_latents` noised to the grid point the run begins at and runs the last round(strength N) of the N grid points;
inpainting (`inpaint_mask`, 1 = generate, 0 = keep) blends every step's result with the known latent carried to the level the new state
lives at, x = m x + (1 - m) (k_a known + k_b n): ddpm k_a = 1, k_b = that sigma; flow k_a = t', k_b = 1 - t'; n is the initial noise.

VAE decode and text encoding are the caller's, as all preconditioning is."""
from __future__ import annotations

import math
from typing import List, Optional, Sequence, Tuple

import torch

from .scheduler import NoiseScheduler

METHODS = ("ddpm", "flow_matching")
PREDICTION_TYPES = ("epsilon", "v_prediction")
PARAMETERIZATIONS = ("trained", "reference")
SOLVERS = ("euler", "euler_a", "dpmpp_2m", "heun")

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


def check_solver(solver: str, method: str, parameterization: str = "trained") -> str:
    """the solver's name, or ValueError naming the solver and the method it cannot run on"""
    solver = str(solver).lower()
    if solver not in SOLVERS:
        raise ValueError(f"solver: unknown value {solver!r} (expected one of {', '.join(SOLVERS)})")
    if solver != "euler" and method == "ddpm" and parameterization != "trained":
        raise ValueError(f"solver {solver!r} needs method ddpm's 'trained' parameterization (got {parameterization!r}: only euler runs it)")
    if solver in ("euler_a", "dpmpp_2m") and method != "ddpm":
        raise ValueError(f"solver {solver!r} is defined on the ddpm sigma: method {method!r} cannot run it (euler or heun can)")
    return solver


def ancestral_sigmas(sigma: float, sigma_next: float, eta: float = 1.0) -> Tuple[float, float]:
    """(sigma_down, sigma_up) of an ancestral step: sigma_down^2 + sigma_up^2 = sigma_next^2 (k-diffusion's get_ancestral_step)"""
    up = min(sigma_next, eta * math.sqrt(sigma_next * sigma_next * (sigma * sigma - sigma_next * sigma_next) / (sigma * sigma)))
    return math.sqrt(sigma_next * sigma_next - up * up), up


def solver_steps(steps: Sequence[Step], grid: Sequence[float], method: str = "ddpm", solver: str = "euler", eta: float = 1.0,
                 guidance_scale: float = 1.0, guidance_rescale: float = 0.0, cfg: bool = False, inpaint: bool = False,
                 parameterization: str = "trained"):
    """(kernel dictionaries, time inputs, levels), one entry per FORWARD: `steps` (a parameter set, one entry per grid point) expanded
    by `solver`.  `grid` holds the levels the parameter set was built on: the sigmas of `steps` for ddpm, the len(steps) + 1 times
    for flow matching.  A dictionary holds kernel_steps' keys and, only where a solver needs them, the non-zero scalars of
    sdxl_sampler_step_ext (r, u, s, save) -- euler's are kernel_steps' own -- plus k_a, k_b with `inpaint`.  levels[f] is the sigma
    (ddpm) or t (flow) the state forward f runs on lives at."""
    solver = check_solver(solver, method, parameterization)
    if not float(eta) >= 0.0 or not math.isfinite(float(eta)):
        raise ValueError(f"eta must be a finite number >= 0 (got {eta})")
    flow = method == "flow_matching"
    lv = [float(g) for g in grid]
    n = len(steps)
    if len(lv) != (n + 1 if flow else n):
        raise ValueError(f"solver_steps: {n} steps need {n + 1 if flow else n} grid values for {method} (got {len(lv)})")
    if inpaint and not flow and parameterization != "trained":
        raise ValueError("inpainting needs the 'trained' parameterization (the reference's set runs each forward one grid point behind)")
    nxt = (lambda j: lv[j + 1]) if flow else (lambda j: lv[j + 1] if j + 1 < n else 0.0)
    fw = []      # per forward: (index into steps of the input scaling / time input / denoiser, p, q, extras, level, level after)
    h_prev = None
    for j in range(n):
        a, b = lv[j], nxt(j)
        p, q = steps[j][3], steps[j][4]
        last = j + 1 == n
        if solver == "euler_a" and not last:
            down, up = ancestral_sigmas(a, b, float(eta))
            p = down / a
            fw.append((j, p, 1.0 - p, dict(s=up), a, b))
        elif solver == "dpmpp_2m":
            ex = dict(save=1)
            if not last:
                h = math.log(a) - math.log(b)
                if h_prev is not None:
                    rho = h_prev / h
                    q, ex = (1.0 - p) * (1.0 + 1.0 / (2.0 * rho)), dict(r=-(1.0 - p) / (2.0 * rho), save=1)
                h_prev = h
            fw.append((j, p, q, ex, a, b))
        elif solver == "heun" and not last:
            fw.append((j, p, q, dict(save=3), a, b))
            if flow:
                dt = b - a
                fw.append((j + 1, 0.0, dt / 2.0, dict(r=dt / 2.0, u=1.0), b, b))
            else:
                c = (b - a) / 2.0
                fw.append((j + 1, c / b, -c / b, dict(r=-c / a, u=1.0 + c / a), b, b))
        else:
            fw.append((j, p, q, {}, a, b))
    ks = []
    for f, (j, p, q, ex, _lv, after) in enumerate(fw):
        a_in_next, clamp_next = (steps[fw[f + 1][0]][0], steps[fw[f + 1][0]][5]) if f + 1 < len(fw) else (1.0, 0.0)
        k = dict(cfg=int(cfg), init=0, a_skip=steps[j][1], a_out=steps[j][2], p=p, q=q, a_in_next=a_in_next, clamp=clamp_next,
                 guidance=float(guidance_scale) if cfg else 1.0, guidance_rescale=float(guidance_rescale))
        k.update({key: v for key, v in ex.items() if v != 0})
        if inpaint:
            k.update(dict(k_a=after, k_b=1.0 - after) if flow else dict(k_a=1.0, k_b=after))
        ks.append(k)
    return ks, [steps[j][6] for j, *_ in fw], [f[4] for f in fw]


def blend_known(x: torch.Tensor, mask: torch.Tensor, known: torch.Tensor, knoise: torch.Tensor, k_a: float, k_b: float) -> torch.Tensor:
    """the inpainting blend of the step kernel in separate fp32 torch ops (the start state's): m x + (1 - m) (k_a known + k_b knoise),
    mask [B,1,H,W]"""
    c = lambda v: torch.tensor(float(v), dtype=torch.float32)
    y = c(k_a) * known
    if float(k_b) != 0.0:
        y = y + c(k_b) * knoise
    t1 = mask * x
    t2 = (c(1.0) - mask) * y
    return t1 + t2


class NativeSampler:
    """sample(...) -> latents [B,4,H,W] fp32 on the device.  `unet` is a NativeUNet (its bound weight arena is what is sampled)."""

    def __init__(self, unet, method: str = "ddpm", prediction_type: str = "v_prediction", use_ztsnr: bool = True,
                 parameterization: str = "trained", config=None, t_bf16: bool = True, control=None):
        method, prediction_type, parameterization = str(method).lower(), str(prediction_type).lower(), str(parameterization).lower()
        for key, val, known in (("method", method, METHODS), ("prediction_type", prediction_type, PREDICTION_TYPES),
                                ("parameterization", parameterization, PARAMETERIZATIONS)):
            if val not in known:
                raise ValueError(f"sampler {key}: unknown value {val!r} (expected one of {', '.join(known)})")
        self.unet = unet
        # control(sample, timestep, batch) -> (down, mid), as NativeSDXLTrainer's: called before every forward with that forward's input
        # (a_in x, clamped; the plan's batch: 2B rows with guidance) and time input; its outputs are added to the UNet's skips / mid output
        self.control = control
        self.method, self.prediction_type, self.parameterization = method, prediction_type, parameterization
        self.use_ztsnr, self.t_bf16 = bool(use_ztsnr), bool(t_bf16)
        if config is None:
            from .config import Config
            config = Config()
            config.model.use_ztsnr = self.use_ztsnr
        self.table = NoiseScheduler(config, "cpu").sigmas                 # the training table (fp32)

    # ------------------------------------------------------------------ the schedule
    def grid(self, num_steps: int, sigmas=None, timesteps=None) -> Tuple[List[float], Optional[List[float]]]:
        """(levels, time inputs) the schedule is built on: ddpm the sigmas of the forwards and their time inputs; flow matching the
        num_steps + 1 times (their time inputs are the times themselves: None)"""
        if self.method == "flow_matching":
            if sigmas is not None:
                raise ValueError("flow matching has no sigmas: pass the grid as timesteps")
            if timesteps is not None:
                return [float(t) for t in timesteps], None
            if int(num_steps) < 1:
                raise ValueError(f"num_steps must be >= 1 for flow matching (got {num_steps})")
            return [j / int(num_steps) for j in range(int(num_steps) + 1)], None
        if sigmas is None:
            idx = ddpm_indices(num_steps, self.table.numel()) if timesteps is None else [int(t) for t in timesteps]
            sig = [float(self.table[i]) for i in idx]
            ts = [float(i) for i in idx]
        else:
            sig = [float(s) for s in sigmas]
            ts = [float(t) for t in timesteps] if timesteps is not None else [float(i) for i in nearest_indices(self.table, sig)]
        return sig, ts

    def schedule(self, num_steps: int, sigmas=None, timesteps=None) -> Tuple[float, List[Step]]:
        """(scale of the initial noise, steps) of this sampler; explicit `sigmas` / `timesteps` override the default grid"""
        lv, ts = self.grid(num_steps, sigmas, timesteps)
        if self.method == "flow_matching":
            return flow_steps(num_steps, None if timesteps is None else lv, self.t_bf16)
        if self.parameterization == "reference":
            return ddpm_reference_steps(lv, ts)
        return ddpm_trained_steps(lv, ts, self.prediction_type, self.use_ztsnr)

    @staticmethod
    def plan_batch(B: int, guidance_scale: float) -> int:
        """the batch of the UNet plan: B without guidance (guidance_scale == 1), else 2B = [cond; uncond]"""
        return int(B) if float(guidance_scale) == 1.0 else 2 * int(B)

    def _residuals(self, x, a_in: float, clamp: float, t_row, cfg: bool, cond) -> dict:
        """the residuals keyword of one forward ({} without a control module: the call is then the one made without this feature)"""
        if self.control is None:
            return {}
        dev = self.unet.device
        with torch.no_grad():
            s = x if float(a_in) == 1.0 else torch.tensor(float(a_in), dtype=torch.float32, device=x.device) * x
            if float(clamp) > 0.0:
                s = s.clamp(-float(clamp), float(clamp))
            down, mid = self.control(torch.cat([s, s]) if cfg else s, t_row, cond)
        outs = list(down) + [mid]
        dt = torch.bfloat16 if all(t is None or t.dtype == torch.bfloat16 for t in outs) else torch.float32
        conv = lambda t: None if t is None else t.detach().to(dev, dt).contiguous()
        return dict(residuals=([conv(t) for t in down], conv(mid)))

    # ------------------------------------------------------------------ the loop
    def sample(self, prompt_embeds, pooled, time_ids, neg_prompt_embeds=None, neg_pooled=None, neg_time_ids=None, *,
               height: int, width: int, num_steps: int, guidance_scale: float = 1.0, guidance_rescale: float = 0.0,
               generator: Optional[torch.Generator] = None, noise: Optional[torch.Tensor] = None, sigmas=None,
               timesteps=None, solver: str = "euler", eta: float = 1.0, step_noise: Optional[torch.Tensor] = None,
               init_latents: Optional[torch.Tensor] = None, strength: float = 1.0,
               inpaint_mask: Optional[torch.Tensor] = None, input_cond: Optional[torch.Tensor] = None,
               neg_input_cond: Optional[torch.Tensor] = None) -> torch.Tensor:
        """height / width are the latent's.  Negative conditioning that is missing with guidance_scale != 1 is zeros of the same
        shape (neg_time_ids: the positive ones).  `noise` [B,4,H,W] overrides the draw from `generator` (CPU, as in training).  The
        loop enqueues every forward and step without a host synchronisation; the result is stream-ordered.

        `solver`: SOLVERS (the module docstring).  euler_a draws one [B,4,H,W] normal tensor per stochastic step, all of them as one
        torch.randn((n,B,4,H,W)) from `generator` behind the initial noise; `step_noise` [n,B,4,H,W] overrides that draw.
        `init_latents` [B,4,H,W] with 0 < strength <= 1 (img2img) runs the last max(1, round(strength N)) of the N grid points from
        init + sigma_start n (ddpm) or (1 - t_start) n + t_start init (flow); strength = 1 is pure noise, the call without
        init_latents.  `inpaint_mask` [B,H,W] or [B,1,H,W] in [0,1] (1 = generate, 0 = keep) needs init_latents, the latent kept.
        `input_cond` [B, in_channels - 4, H, W] (a UNet with in_channels > 4: inpainting, image conditioning): channels 4.. of every
        forward's input, rounded to bf16 by the step kernel.  With guidance the unconditional half reuses it unless `neg_input_cond`
        (same shape) is given.  The keyword reaches the net only when it is given."""
        net = self.unet
        dev = net.device
        B = int(prompt_embeds.shape[0])
        H, W = int(height), int(width)
        if not 0.0 <= float(guidance_rescale) <= 1.0:
            raise ValueError(f"guidance_rescale must be in [0, 1] (got {guidance_rescale})")
        solver = check_solver(solver, self.method, self.parameterization)
        cfg = float(guidance_scale) != 1.0
        x0_scale, steps = self.schedule(num_steps, sigmas, timesteps)
        first, mask, known = self._start(len(steps), B, H, W, init_latents, strength, inpaint_mask)
        plain = solver == "euler" and known is None              # today's sampler: today's calls
        if not plain:
            lv, _ts = self.grid(num_steps, sigmas, timesteps)
            steps, lv = steps[first:], lv[first:]
            ks, tin, _levels = solver_steps(steps, lv, self.method, solver, eta, guidance_scale, guidance_rescale, cfg,
                                            mask is not None, self.parameterization)
        if noise is None:
            noise = torch.randn((B, 4, H, W), generator=generator)
        if tuple(noise.shape) != (B, 4, H, W):
            raise ValueError(f"noise: expected shape {(B, 4, H, W)}, got {tuple(noise.shape)}")
        x = noise.to(torch.float32)
        if plain or known is None or first == 0:
            if x0_scale != 1.0:
                x = torch.tensor(x0_scale, dtype=torch.float32, device=x.device) * x     # sigma_0 * n: one fp32 product where the noise lives, before the loop
        elif self.method == "flow_matching":                                             # img2img: the known latent noised to the first grid point run
            c = lambda v: torch.tensor(v, dtype=torch.float32, device=x.device)
            x = c(1.0 - lv[0]) * x + c(lv[0]) * known.to(x.device)
        else:
            x = known.to(x.device) + torch.tensor(lv[0], dtype=torch.float32, device=x.device) * x
        if not plain and mask is not None:
            k_a, k_b = (lv[0], 1.0 - lv[0]) if self.method == "flow_matching" else (1.0, lv[0])
            x = blend_known(x, mask.to(x.device), known.to(x.device), noise.to(torch.float32), k_a, k_b)
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
        ic = {}
        if neg_input_cond is not None and input_cond is None:
            raise ValueError("neg_input_cond needs input_cond")
        if input_cond is not None:
            for name, t in (("input_cond", input_cond), ("neg_input_cond", neg_input_cond)):
                if t is not None and (t.dim() != 4 or tuple(t.shape) != (B, int(input_cond.shape[1]), H, W)):
                    raise ValueError(f"{name}: expected shape {(B, int(input_cond.shape[1]), H, W)}, got {tuple(t.shape)}")
            c = input_cond.detach().to(dev, torch.float32)
            if cfg:
                c = torch.cat([c, c if neg_input_cond is None else neg_input_cond.detach().to(dev, torch.float32)])
            ic = dict(input_cond=c.contiguous())
        cond = {"prompt_embeds": pe, "pooled_prompt_embeds": po, "time_ids": ti}      # what `control` gets as its batch (the plan's rows)
        # forward f reads bf16(clamp(a_in x)): the first from sample_init, the others from the step before them
        scale_of = lambda f, ks: (steps[0][0], steps[0][5]) if f == 0 else (ks[f - 1]["a_in_next"], ks[f - 1]["clamp"])
        if plain:
            # the time inputs of all forwards, uploaded once: row j is forward j's [PB] values
            tall = torch.tensor([[s[6]] * PB for s in steps], dtype=torch.float32).to(dev)
            ks = kernel_steps(steps, guidance_scale, guidance_rescale, cfg)
            net.sample_init(x, pe, po, ti, tall[0], cfg=cfg, a_in=steps[0][0], clamp=steps[0][5], **ic)
            for j, k in enumerate(ks):
                net.sample_step(x, pe, po, ti, tall[j], **k, **ic, **self._residuals(x, *scale_of(j, ks), tall[j], cfg, cond))
            return x
        # every buffer of the extended steps is made and uploaded here, before the loop: no torch op runs between forwards
        tall = torch.tensor([[t] * PB for t in tin], dtype=torch.float32).to(dev)
        need = lambda key, bit: any(k.get(key, 0) != 0 or k.get("save", 0) & bit for k in ks)
        hist = torch.zeros_like(x) if need("r", 1) else None
        xsave = torch.zeros_like(x) if need("u", 2) else None
        nstoch = sum(1 for k in ks if k.get("s", 0) != 0)
        draws = None
        if nstoch:
            if step_noise is None:
                step_noise = torch.randn((nstoch, B, 4, H, W), generator=generator)
            if tuple(step_noise.shape) != (nstoch, B, 4, H, W):
                raise ValueError(f"step_noise: expected shape {(nstoch, B, 4, H, W)}, got {tuple(step_noise.shape)}")
            draws = step_noise.to(dev, torch.float32).contiguous()
        blend = {}
        if mask is not None:
            blend = dict(mask=mask.to(dev).contiguous(), known=known.to(dev).contiguous(),
                         knoise=noise.to(torch.float32).to(dev).contiguous())
        net.sample_init(x, pe, po, ti, tall[0], cfg=cfg, a_in=steps[0][0], clamp=steps[0][5], **ic)
        d = 0
        for f, k in enumerate(ks):
            ex = dict(blend)
            if k.get("r", 0) != 0 or k.get("save", 0) & 1:
                ex["hist"] = hist
            if k.get("u", 0) != 0 or k.get("save", 0) & 2:
                ex["xsave"] = xsave
            if k.get("s", 0) != 0:
                ex["noise"], d = draws[d], d + 1
            net.sample_step(x, pe, po, ti, tall[f], **k, **ex, **ic, **self._residuals(x, *scale_of(f, ks), tall[f], cfg, cond))
        return x

    def _start(self, n: int, B: int, H: int, W: int, init_latents, strength, inpaint_mask):
        """(index of the first grid point run, mask [B,1,H,W] fp32 or None, known latent fp32 or None) of an img2img / inpainting call"""
        if inpaint_mask is not None and init_latents is None:
            raise ValueError("inpaint_mask needs init_latents (the latent that is kept where the mask is 0)")
        if init_latents is None:
            if float(strength) != 1.0:
                raise ValueError(f"strength = {strength} needs init_latents")
            return 0, None, None
        if self.method == "ddpm" and self.parameterization != "trained":
            raise ValueError("init_latents needs the 'trained' parameterization (the reference's set starts from the noise alone)")
        if tuple(init_latents.shape) != (B, 4, H, W):
            raise ValueError(f"init_latents: expected shape {(B, 4, H, W)}, got {tuple(init_latents.shape)}")
        if not 0.0 < float(strength) <= 1.0:
            raise ValueError(f"strength must be in (0, 1] (got {strength})")
        run = max(1, int(math.floor(float(strength) * n + 0.5)))
        known = init_latents.detach().to("cpu", torch.float32).contiguous()
        mask = None
        if inpaint_mask is not None:
            if tuple(inpaint_mask.shape) not in ((B, H, W), (B, 1, H, W)):
                raise ValueError(f"inpaint_mask: expected shape {(B, H, W)} or {(B, 1, H, W)}, got {tuple(inpaint_mask.shape)}")
            mask = inpaint_mask.detach().to("cpu", torch.float32).reshape(B, 1, H, W).contiguous()
            if not bool(torch.isfinite(mask).all()) or float(mask.min()) < 0.0 or float(mask.max()) > 1.0:
                raise ValueError("inpaint_mask: values must be finite and in [0, 1]")
        return n - run, mask, known
