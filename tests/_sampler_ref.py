"""Host restatement of the sampler arithmetic (csrc/sampler.hip, include/sdxlstep.h sdxl_sampler_step) in separate torch ops.

The generic step, in the dtype of `x` (float32: what the kernel is held to bit for bit; float64: the mathematics), every operation
a torch op of its own and in this order:

    t = F_c - F_u ; t = g * t ; F = F_u + t                                     (guidance; F = F_c without)
    t1 = F * r ; t1 = phi * t1 ; t2 = (1 - phi) * F ; F = t1 + t2                (rescale, r = std(F_c) / std(F) per sample; phi != 0 only)
    d1 = a_skip * x ; d2 = a_out * F ; den = d1 + d2
    u1 = p * x ; u2 = q * den ; x_next = u1 + u2
    v = a_in_next * x_next ; v = clamp(v, -c, c) if c > 0 ; in_next = bf16(v)

Scalars enter as 0-d tensors of x's dtype, i.e. rounded to float32 exactly as the C struct's float fields are.

The second half restates the four sampling functions of the reference's NoiseScheduler (training/schedulers/novelai_v3.py:59-99)
operation for operation; tests/golden/sampler_reference.npz (tests/make_sampler_goldens.py) holds what the reference's own code
returned for the same inputs."""
from __future__ import annotations

import torch


def _s(v, like: torch.Tensor) -> torch.Tensor:
    return torch.tensor(float(v), dtype=like.dtype)


def guide(fc: torch.Tensor, fu, g: float) -> torch.Tensor:
    if fu is None:
        return fc
    t = fc - fu
    t = _s(g, fc) * t
    return fu + t


def rescale(F: torch.Tensor, fc: torch.Tensor, phi: float) -> torch.Tensor:
    """guidance rescale (diffusers' rescale_noise_cfg): per sample over C.H.W"""
    if float(phi) == 0.0:
        return F
    dims = tuple(range(1, F.dim()))
    r = fc.std(dim=dims, keepdim=True) / F.std(dim=dims, keepdim=True)
    t1 = F * r
    t1 = _s(phi, F) * t1
    t2 = (_s(1.0, F) - _s(phi, F)) * F
    return t1 + t2


def step(x: torch.Tensor, F: torch.Tensor, a_skip, a_out, p, q) -> torch.Tensor:
    d1 = _s(a_skip, x) * x
    d2 = _s(a_out, x) * F
    den = d1 + d2
    u1 = _s(p, x) * x
    u2 = _s(q, x) * den
    return u1 + u2


def unet_input(x: torch.Tensor, a_in, clamp, quantize: bool = True) -> torch.Tensor:
    """the UNet input in x's dtype: bf16-rounded values when `quantize` (what the kernel writes), the exact product otherwise"""
    v = _s(a_in, x) * x
    if float(clamp) > 0.0:
        v = torch.clamp(v, -float(_s(clamp, x)), float(_s(clamp, x)))
    return v.to(torch.bfloat16).to(x.dtype) if quantize else v


def full_step(x, fc, fu, k):
    """one kernel call: k holds the scalar fields of sdxl_sampler_step.  fc / fu in x's dtype (bf16 values).  Returns (x_next, in_next)."""
    if k.get("init"):
        return x, unet_input(x, k["a_in_next"], k["clamp"])
    F = guide(fc, fu if k["cfg"] else None, k["guidance"])
    F = rescale(F, fc, k.get("guidance_rescale", 0.0))
    xn = step(x, F, k["a_skip"], k["a_out"], k["p"], k["q"])
    return xn, unet_input(xn, k["a_in_next"], k["clamp"])


def sample_loop(model_fn, noise: torch.Tensor, x0_scale: float, steps, guidance_scale: float = 1.0, guidance_rescale: float = 0.0,
                quantize: bool = True) -> torch.Tensor:
    """the whole sampler in noise's dtype.  steps: [(a_in, a_skip, a_out, p, q, clamp, timestep)] (sampler.py's parameter sets);
    model_fn(inp, timestep, j) -> F, or (F_c, F_u) when guidance_scale != 1."""
    cfg = float(guidance_scale) != 1.0
    x = noise if float(x0_scale) == 1.0 else _s(x0_scale, noise) * noise
    inp = unet_input(x, steps[0][0], steps[0][5], quantize)
    for j, (_a_in, a_skip, a_out, p, q, _c, t) in enumerate(steps):
        out = model_fn(inp, t, j)
        fc, fu = out if cfg else (out, None)
        F = rescale(guide(fc, fu, guidance_scale), fc, guidance_rescale)
        x = step(x, F, a_skip, a_out, p, q)
        if j + 1 < len(steps):
            inp = unet_input(x, steps[j + 1][0], steps[j + 1][5], quantize)
    return x


# ---------------------------------------------------------------------------------------------- the reference's four functions
def get_karras_scalings(sigma: torch.Tensor, sigma_data: float = 1.0):
    c_skip = (sigma_data ** 2) / (sigma ** 2 + sigma_data ** 2)
    c_out = -sigma * sigma_data / torch.sqrt(sigma ** 2 + sigma_data ** 2)
    c_in = 1 / torch.sqrt(sigma ** 2 + sigma_data ** 2)
    return c_skip, c_out, c_in


def ztsnr_first_step(n: torch.Tensor, sigma_1, model_fn, sigma_data: float = 1.0) -> torch.Tensor:
    return sigma_1 * n - sigma_data * model_fn(n, torch.tensor([float("inf")]))


def euler_step(x: torch.Tensor, sigma_i, sigma_next, model_fn) -> torch.Tensor:
    c_skip, c_out, c_in = get_karras_scalings(sigma_i)
    denoised = c_skip * x + c_out * model_fn(c_in * x, sigma_i)
    d = (x - denoised) / sigma_i
    return x + (sigma_next - sigma_i) * d


def sample_with_ztsnr(model_fn, n: torch.Tensor, sigmas: torch.Tensor) -> torch.Tensor:
    """the loop of the reference's sample_with_ztsnr on a given noise and sigma grid (it draws n and builds karras(N) itself)"""
    x = ztsnr_first_step(n, sigmas[0], model_fn)
    for i in range(1, len(sigmas)):
        x = euler_step(x, sigmas[i - 1], sigmas[i], model_fn)
    return x
