"""Reference arithmetic of LoRA by merge and project (not a test module): the merge restated in separate fp32 torch ops, bit for bit
what csrc/lora.hip computes, and the projections in float64 with their a-priori error bound."""
from __future__ import annotations

import numpy as np
import torch

U24 = 2.0 ** -24          # unit roundoff of fp32


def f32(s: float) -> float:
    """the python scalar as the float32 the C ABI receives"""
    return float(np.float32(s))


def merge(W0: torch.Tensor, A: torch.Tensor, B: torch.Tensor, s: float) -> torch.Tensor:
    """W = bf16_rn(W0 + s * acc), acc <- acc + B[:, k] A[k, :] for k = 0 .. r - 1, every product and sum a separate fp32 op (no FMA),
    and W = W0 where s * acc == 0.  W0 [out, in], A [r, in], B [out, r] bf16; any device."""
    assert W0.dtype == A.dtype == B.dtype == torch.bfloat16
    a, b = A.float(), B.float()
    acc = torch.zeros(W0.shape, dtype=torch.float32, device=W0.device)
    for k in range(A.shape[0]):
        prod = b[:, k: k + 1] * a[k: k + 1, :]
        acc = acc + prod
    t = acc * torch.tensor(f32(s), dtype=torch.float32, device=W0.device)
    w = (W0.float() + t).to(torch.bfloat16)
    return torch.where(t == 0, W0, w)


def project64(dW: torch.Tensor, A: torch.Tensor, B: torch.Tensor, s: float):
    """(dA, dB) = (s B^T dW, s dW A^T) in float64"""
    d, a, b = dW.double(), A.double(), B.double()
    return f32(s) * (b.t() @ d), f32(s) * (d @ a.t())


def project_bound(dW: torch.Tensor, A: torch.Tensor, B: torch.Tensor, s: float):
    """|got - ref| <= (n + 2) 2^-24 |s| sum_j |x_j y_j|, n the reduction length (out for dA, in for dB), the sum of magnitudes in
    float64: holds for an fp32 sum of n products in ANY order (n - 1 additions and n multiplications, fused or not, and the final scale)."""
    d, a, b = dW.double().abs(), A.double().abs(), B.double().abs()
    out, inn = dW.shape
    return (out + 2) * U24 * abs(f32(s)) * (b.t() @ d), (inn + 2) * U24 * abs(f32(s)) * (d @ a.t())
