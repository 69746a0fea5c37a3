"""CPU restatement of the schedule-free Kahan AdamW element arithmetic (both modes of optimizer.AdamWScheduleFreeKahanBF16).

Test helper only.  Reference: src/training/optimizers/adamw_schedulefree/__init__.py (`AdamWScheduleFreeKahan.step`).
Arrays are bf16 bit patterns (uint16); every torch op of the reference on its bf16 tensors is a float32 operation on the
widened values followed by round-to-nearest-even, with torch CPU's scalar handling (established against torch 2.x and
pinned by tests/golden/schedulefree_kahan.npz, tests/make_schedulefree_goldens.py):
  * `t.mul_(s)` / `s * t`: the scalar stays float32;
  * `t.add_(s)` and the `alpha` of `t.add_(u, alpha=a)`: the scalar is rounded to bf16 first; `t + a*u` is one fused
    multiply-add;
  * `t.addcmul_(u, u, value=s)`: fma(s*u, u, t) with s float32.

reference:   the reference's sequence, bit for bit (its `kahan_comp` stays +0, see the module docstring of optimizer.py).
compensated: the true parameter is x = p + c (c = the bf16 `kahan_comp` arena); the same moments, then in float32
             x -= (step_size*wd)*x ; x -= step_size*(m/d) ; p = rn(x) ; c = rn(x - p).
"""
from __future__ import annotations

import numpy as np

from oracle.adamw_ref import _bf16_scalar, bf16_to_f32, f32_to_bf16_rn, fma32

F32 = np.float32


def rn(x: np.ndarray) -> np.ndarray:
    """float32 -> bf16 -> float32 (round-to-nearest-even)"""
    return bf16_to_f32(f32_to_bf16_rn(np.asarray(x, dtype=np.float32)))


def schedule(k: int, lr: float, beta2: float, warmup_steps: int):
    """Host scalars of step k (the counter before the increment), in python doubles as the reference computes them:
    (adjusted_lr, step_size)."""
    sched = (k + 1) / warmup_steps if k < warmup_steps else 1.0
    bc2 = 1 - beta2 ** (k + 1)
    adjusted_lr = lr * sched * (bc2 ** 0.5)
    return adjusted_lr, adjusted_lr / (bc2 ** 0.5)


def grad_in(grad, grad_scale: float = 1.0, grad_round_bf16: bool = True) -> np.ndarray:
    """the kernel's gradient input: bf16 bits or float32, times grad_scale (float32), optionally rounded to bf16"""
    g = bf16_to_f32(grad) if grad.dtype == np.uint16 else np.asarray(grad, dtype=np.float32)
    g = (g * F32(grad_scale)).astype(np.float32)
    return rn(g) if grad_round_bf16 else g


def _moments(g, m, v, beta1, beta2, eps):
    m1 = rn(bf16_to_f32(m) * F32(beta1))                              # exp_avg.mul_(beta1)
    m2 = rn(fma32(g, _bf16_scalar(1 - beta1), m1))                    # .add_(grad, alpha=1 - beta1)
    v1 = rn(bf16_to_f32(v) * F32(beta2))                              # exp_avg_sq.mul_(beta2)
    v2 = rn(fma32((F32(1 - beta2) * g).astype(np.float32), g, v1))    # .addcmul_(grad, grad, value=1 - beta2)
    d = rn(np.sqrt(v2))                                               # exp_avg_sq.sqrt()
    d = rn(d + _bf16_scalar(eps))                                     # .add_(eps)
    return m2, v2, d


def step(p, m, v, c, g, *, step_size, beta1, beta2, eps, weight_decay, kahan_sum, reference):
    """One update.  p, m, v, c: uint16 bf16 bits (c ignored / None without kahan_sum); g: float32 gradient values as
    grad_in() returns them.  Returns (p, m, v, c, g_after) as uint16 bits (c None without kahan_sum); g_after is the
    reference's p.grad after its in-place `grad += kahan_comp` (the kernel never writes the gradient)."""
    g = np.asarray(g, dtype=np.float32)
    pf = bf16_to_f32(p)
    cf = bf16_to_f32(c) if kahan_sum else None
    if reference:
        if kahan_sum:
            g = rn(g + cf)                                            # grad.add_(kahan_comp)
        m2, v2, d = _moments(g, m, v, beta1, beta2, eps)
        if weight_decay != 0:
            pf = rn(fma32(pf, _bf16_scalar(-weight_decay), pf))       # p.data.add_(p.data, alpha=-weight_decay)
        s = rn(m2 / d)                                                # exp_avg / denom
        u = rn(s * F32(-step_size))                                   # -step_size * step
        p2 = rn(pf + u)                                               # p.data.add_(...)
        c2 = None
        if kahan_sum:
            b = rn(p2 + u)                                            # buffer = p.data.add(-step_size * step)
            a = rn(p2 - b)                                            # p.data.sub(buffer)
            b2 = rn(b - p2)                                           # buffer.sub_(p.data)
            c2 = f32_to_bf16_rn(rn(a + b2))                           # kahan_comp.copy_(a.add(b))
        return f32_to_bf16_rn(p2), f32_to_bf16_rn(m2), f32_to_bf16_rn(v2), c2, f32_to_bf16_rn(g)
    m2, v2, d = _moments(g, m, v, beta1, beta2, eps)
    x = (pf + cf).astype(np.float32) if kahan_sum else pf
    if weight_decay != 0:
        x = (x - (F32(step_size * weight_decay) * x).astype(np.float32)).astype(np.float32)
    q = (m2 / d).astype(np.float32)
    x = (x - (F32(step_size) * q).astype(np.float32)).astype(np.float32)
    p2 = f32_to_bf16_rn(x)
    c2 = f32_to_bf16_rn((x - bf16_to_f32(p2)).astype(np.float32)) if kahan_sum else None
    return p2, f32_to_bf16_rn(m2), f32_to_bf16_rn(v2), c2, f32_to_bf16_rn(g)
