"""CPU restatement of the Prodigy update (not a test module): include/sdxlstep.h's algorithm 2 operation by operation, the contract of
csrc/optimizer.hip's prodigy_* kernels and of optimizer.ProdigyBF16.  prodigyopt is not a dependency and nothing is compared with it.

Element arithmetic: torch float32 on the CPU, one torch op per rounded operation (no op here fuses a multiply into an add); the
square root is numpy's, which is correctly rounded where torch's float32 one is not.
Scalars: numpy float32, each operation rounded on its own; host doubles become float32 once.  step64 is the same update in
float64 on a float64 parameter (no bf16, no compensation), for statements about the algorithm itself."""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

F = np.float32
MAX_GRID = 4096                # SDXL_PRODIGY_MAX_GRID
STATE_FLOATS = 8 + 2 * MAX_GRID


@dataclass
class Hyper:
    lr: float = 1.0
    beta1: float = 0.9
    beta2: float = 0.999
    beta3: Optional[float] = None          # None = sqrt(beta2)
    eps: float = 1e-8
    weight_decay: float = 0.0
    d0: float = 1e-6
    d_coef: float = 1.0
    growth_rate: float = math.inf
    use_bias_correction: bool = False
    safeguard_warmup: bool = False
    grad_round_bf16: bool = False

    def b3(self) -> float:
        return math.sqrt(self.beta2) if self.beta3 is None else self.beta3

    def bc(self, k: int) -> float:
        """the bias-correction factor of step k (0-based), in python doubles; 1 when off"""
        if not self.use_bias_correction:
            return 1.0
        return math.sqrt(1 - self.beta2 ** (k + 1)) / (1 - self.beta1 ** (k + 1))


def geometry(n: int):
    """(grid, T(n)) of the documented launch geometry: workgroups of 256 threads x 8 elements, at most MAX_GRID of them; a thread
    adds at most T(n) terms into its sum"""
    grid = min(-(-n // 2048), MAX_GRID)
    return grid, 8 * -(-n // (2048 * grid))


def fresh_state(d0: float) -> np.ndarray:
    st = np.zeros(8, dtype=np.float32)
    st[:2] = F(d0)
    return st


def scalars(d, hp: Hyper, bc: float):
    """dlr, cm, cv, cs, cn from d (float32)"""
    d = F(d)
    dlr = F(F(d * F(hp.lr)) * F(bc))
    cm = F(d * F(1 - hp.beta1))
    cv = F(F(d * d) * F(1 - hp.beta2))
    r = F(d / F(hp.d0))
    cs = F(r * (d if hp.safeguard_warmup else dlr))
    cn = F(r * dlr)
    return dlr, cm, cv, cs, cn


def grad_in(g: torch.Tensor, scale: Optional[float], hp: Hyper) -> torch.Tensor:
    """the gradient the update sees: bf16 or fp32 input as float32, times the device scale, rounded to bf16 with grad_round_bf16"""
    gr = g.float() * float(F(1.0 if scale is None else scale))
    return gr.to(torch.bfloat16).float() if hp.grad_round_bf16 else gr


def _k(x) -> float:
    return float(x)            # a float32 value as the python scalar torch multiplies a float32 tensor by (exact)


def accumulate(p, c, p0, m, v, s, gr, d, hp: Hyper, bc: float):
    """p, c, p0: bf16 tensors; m, v, s, gr: float32 tensors; d: state[0] before the call.  Returns (m', v', s', t, a), float32"""
    _dlr, cm, cv, cs, _cn = scalars(d, hp, bc)
    x = p.float() + c.float()
    t = gr * (p0.float() - x)
    m1 = (m * _k(F(hp.beta1))) + (gr * _k(cm))
    v1 = (v * _k(F(hp.beta2))) + ((gr * _k(cv)) * gr)
    s1 = (s * _k(F(hp.b3()))) + (gr * _k(cs))
    return m1, v1, s1, t, s1.abs()


def finalize(state, A, Bs, hp: Hyper, bc: float) -> np.ndarray:
    """the scalar recurrence in float32: state = the 8 floats before the call, A and Bs the sums (float32).  Returns the 8 floats after"""
    d, d_max, num = F(state[0]), F(state[1]), F(state[2])
    A, Bs = F(A), F(Bs)
    dlr, _cm, _cv, _cs, cn = scalars(d, hp, bc)
    with np.errstate(over="ignore"):
        num1 = F(F(F(hp.b3()) * num) + F(cn * A))
        d_new, d_max_new, d_hat = d, d_max, d
        if Bs > 0:
            d_hat = F(F(F(hp.d_coef) * num1) / Bs)
            d1 = max(d, d_hat) if d == F(hp.d0) else d
            d_max_new = max(d_max, d_hat)
            d_new = min(d_max_new, F(d1 * F(hp.growth_rate)))
    return np.array([d_new, d_max_new, num1, Bs, d_hat, dlr, A, 0.0], dtype=np.float32)


def apply(p, c, m1, v1, d_new, dlr, hp: Hyper):
    """p, c: bf16 tensors before the call; m1, v1: the new moments; d_new = state[0], dlr = state[5] after the finalize.  Returns (p', c')"""
    de = F(F(d_new) * F(hp.eps))
    x = p.float() + c.float()
    if hp.weight_decay != 0:
        x = x - (x * _k(F(F(hp.weight_decay) * F(dlr))))
    root = torch.from_numpy(np.sqrt(v1.numpy()))      # IEEE square root: torch's float32 sqrt on the CPU is an ulp off in 0.7 % of elements
    x = x - ((m1 / (root + _k(de))) * _k(F(dlr)))
    p1 = x.to(torch.bfloat16)
    return p1, (x - p1.float()).to(torch.bfloat16)


def ema_step(e: torch.Tensor, p1: torch.Tensor, omd: float) -> torch.Tensor:
    """the fused EMA on the new p: e - (omd * (e - p')), three separately rounded float32 operations"""
    return e - ((e - p1.float()) * _k(F(omd)))


def step64(x, x0, m, v, s, state, g, hp: Hyper, k: int, freeze_d: bool = False):
    """One update in float64 on numpy arrays; state = [d, d_max, num].  Returns (x, m, v, s, state)."""
    d, d_max, num = state
    b1, b2, b3, bc = hp.beta1, hp.beta2, hp.b3(), hp.bc(k)
    dlr = d * hp.lr * bc
    r = d / hp.d0
    m = b1 * m + d * (1 - b1) * g
    v = b2 * v + d * d * (1 - b2) * g * g
    s = b3 * s + r * (d if hp.safeguard_warmup else dlr) * g
    num = b3 * num + r * dlr * float(np.sum(g * (x0 - x)))
    Bs = float(np.sum(np.abs(s)))
    d_new = d
    if Bs > 0 and not freeze_d:
        d_hat = hp.d_coef * num / Bs
        d1 = max(d, d_hat) if d == hp.d0 else d
        d_max = max(d_max, d_hat)
        d_new = min(d_max, d1 * hp.growth_rate)
    if hp.weight_decay != 0:
        x = x - hp.weight_decay * dlr * x
    x = x - dlr * (m / (np.sqrt(v) + d_new * hp.eps))
    return x, m, v, s, (d_new, d_max, num)
