"""Host restatement of the EXTENDED sampler step (csrc/sampler.hip, include/sdxlstep.h sdxl_sampler_step_ext) in separate torch ops,
on top of tests/_sampler_ref.py (guide, rescale, unet_input), and the solvers of sampler.py run through it.

The step, in the dtype of `x` (float32: what the kernel is held to bit for bit; float64: the mathematics), every operation a torch op
of its own and in this order:

    F, den                                           as _sampler_ref.full_step
    acc = p * x ; acc = acc + q * den
    acc = acc + r * hist_old                         (r != 0)
    acc = acc + u * xsave_old                        (u != 0)
    acc = acc + s * noise                            (s != 0)
    hist <- den (save & 1) ; xsave <- x (save & 2)   (after the old values were read)
    y = k_a * known ; y = y + k_b * knoise (k_b != 0) ; t1 = m * acc ; t2 = (1 - m) * y ; acc = t1 + t2        (mask given)
    x_next = acc ; in_next = bf16(clamp(a_in_next * x_next, +-clamp))

`simulate` is the same recurrence on Python floats (doubles) against a denoiser den(x, level) given directly: what the order-of-
convergence check runs the schedules' own scalars through."""
from __future__ import annotations

import torch

import _sampler_ref as R
from _sampler_ref import _s


def ext_step(x, fc, fu, k, hist=None, xsave=None, noise=None, mask=None, known=None, knoise=None, quantize=True, F=None):
    """one kernel call: k holds the scalar fields of sdxl_sampler_step(_ext) (missing extended ones are 0).  fc / fu in x's dtype,
    mask [B,1,H,W].  `F` overrides the guided (and rescaled) prediction.  Returns (x_next, in_next, hist, xsave) -- hist / xsave are
    the inputs unless the step saves into them."""
    if int(k.get("init", 0)) & 1:
        return x, R.unet_input(x, k["a_in_next"], k["clamp"], quantize), hist, xsave
    if F is None:
        F = R.guide(fc, fu if k["cfg"] else None, k["guidance"])
        F = R.rescale(F, fc, k.get("guidance_rescale", 0.0))
    d1 = _s(k["a_skip"], x) * x
    d2 = _s(k["a_out"], x) * F
    den = d1 + d2
    acc = _s(k["p"], x) * x
    acc = acc + _s(k["q"], x) * den
    if float(k.get("r", 0.0)) != 0.0:
        acc = acc + _s(k["r"], x) * hist
    if float(k.get("u", 0.0)) != 0.0:
        acc = acc + _s(k["u"], x) * xsave
    if float(k.get("s", 0.0)) != 0.0:
        acc = acc + _s(k["s"], x) * noise
    save = int(k.get("save", 0))
    if save & 1:
        hist = den
    if save & 2:
        xsave = x
    if mask is not None:
        y = _s(k.get("k_a", 0.0), x) * known
        if float(k.get("k_b", 0.0)) != 0.0:
            y = y + _s(k["k_b"], x) * knoise
        t1 = mask * acc
        t2 = (_s(1.0, x) - mask) * y
        acc = t1 + t2
    return acc, R.unet_input(acc, k["a_in_next"], k["clamp"], quantize), hist, xsave


def solver_loop(model_fn, x, first_in, ks, tin, cfg, step_noise=None, mask=None, known=None, knoise=None, quantize=True):
    """a whole run from the start state x: first_in = (a_in, clamp) of the first forward, ks / tin = sampler.solver_steps' kernel
    dictionaries and time inputs.  model_fn(inp, timestep, f) -> F, or (F_c, F_u) with cfg.  step_noise[d] is the d-th stochastic
    step's draw."""
    inp = R.unet_input(x, first_in[0], first_in[1], quantize)
    hist = xsave = None
    d = 0
    for f, k in enumerate(ks):
        out = model_fn(inp, tin[f], f)
        fc, fu = out if cfg else (out, None)
        nz = None
        if float(k.get("s", 0.0)) != 0.0:
            nz, d = step_noise[d], d + 1
        x, inp, hist, xsave = ext_step(x, fc, fu, k, hist, xsave, nz, mask, known, knoise, quantize)
    return x


def blend(x, mask, known, knoise, k_a, k_b):
    """the inpainting blend alone (the start state of an inpainting run), the same ops as in ext_step"""
    y = _s(k_a, x) * known
    if float(k_b) != 0.0:
        y = y + _s(k_b, x) * knoise
    t1 = mask * x
    t2 = (_s(1.0, x) - mask) * y
    return t1 + t2


def simulate(ks, levels, den, x, noises=()):
    """the solver recurrence on doubles: forward f sees den(x, levels[f]); the denoiser scalings of the dictionaries are not used"""
    hist = xsave = 0.0
    noises = iter(noises)
    for k, lv in zip(ks, levels):
        d = den(x, lv)
        acc = k["p"] * x + k["q"] * d
        if k.get("r", 0.0) != 0.0:
            acc = acc + k["r"] * hist
        if k.get("u", 0.0) != 0.0:
            acc = acc + k["u"] * xsave
        if k.get("s", 0.0) != 0.0:
            acc = acc + k["s"] * next(noises)
        if int(k.get("save", 0)) & 1:
            hist = d
        if int(k.get("save", 0)) & 2:
            xsave = x
        x = acc
    return x
