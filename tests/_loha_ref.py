"""Reference arithmetic of LoHa by merge and project (not a test module): dW = s (B1 A1) .* (B2 A2).  The merge restated in separate fp32
torch ops, bit for bit what csrc/loha.hip computes; the four projections in float64 from the bf16 factors; and their a-priori error bound,
accumulated operation by operation next to the float64 reference.  No constant here comes from a kernel's output.

Shapes: W0, dW [out, in] (the SOURCE view: the state-dict tensor flattened), A1, A2 [r, in], B1, B2 [out, r]."""
from __future__ import annotations

import torch

from _lora_ref import U24, f32

PLAIN, CONV3, GEGLU = 0, 1, 2
NAMES = ("A1", "B1", "A2", "B2")          # the arena's order


# ---- source <-> native (the packed layouts of include/sdxlstep.h; the maps are checked against repack_kernel in tests/test_host_lora_layouts.py)
def geglu_native_rows(out, G, device="cpu"):
    """native row of every source row: (c / G) 2G + half G + c % G, half = o / C4, c = o % C4"""
    C4 = out // 2
    o = torch.arange(out, device=device)
    half, c = o // C4, o % C4
    return (c // G) * 2 * G + half * G + c % G


def to_native(src, kind, group):
    """the [out, in] source view as the native tensor (no padded rows)"""
    out, inn = src.shape
    if kind == CONV3:
        return src.view(out, group, 9).permute(0, 2, 1).reshape(out, inn).contiguous()
    if kind == GEGLU:
        nat = torch.empty_like(src)
        nat[geglu_native_rows(out, group, src.device)] = src
        return nat
    return src.contiguous()


def to_source(nat, kind, group):
    out, inn = nat.shape
    if kind == CONV3:
        return nat.view(out, 9, group).permute(0, 2, 1).reshape(out, inn).contiguous()
    if kind == GEGLU:
        return nat[geglu_native_rows(out, group, nat.device)].contiguous()
    return nat.contiguous()


# ---- merge
def _chain(A: torch.Tensor, B: torch.Tensor) -> torch.Tensor:
    """p <- p + B[:, k] A[k, :] for k = 0 .. r - 1, the product and the sum separate fp32 ops"""
    a, b = A.float(), B.float()
    p = torch.zeros(B.shape[0], A.shape[1], dtype=torch.float32, device=A.device)
    for k in range(A.shape[0]):
        prod = b[:, k: k + 1] * a[k: k + 1, :]
        p = p + prod
    return p


def merge(W0, A1, B1, A2, B2, s: float) -> torch.Tensor:
    """W = bf16_rn(W0 + t), t = s * (p1 * p2), p1 and p2 the separately rounded chains, every operation a separate fp32 op (no FMA), and
    W = W0 where t == 0.  All bf16; any device."""
    assert W0.dtype == A1.dtype == B1.dtype == A2.dtype == B2.dtype == torch.bfloat16
    h = _chain(A1, B1) * _chain(A2, B2)
    t = h * torch.tensor(f32(s), dtype=torch.float32, device=W0.device)
    w = (W0.float() + t).to(torch.bfloat16)
    return torch.where(t == 0, W0, w)


def delta64(A1, B1, A2, B2, s: float) -> torch.Tensor:
    """s (B1 A1) .* (B2 A2) in float64"""
    return f32(s) * (B1.double() @ A1.double()) * (B2.double() @ A2.double())


# ---- project
def project64(dW, A1, B1, A2, B2, s: float):
    """{"A1": dA1, "B1": dB1, "A2": dA2, "B2": dB2} in float64 from the bf16 factors:
    dB1 = s (G .* P2) A1^T, dA1 = s B1^T (G .* P2), dB2 = s (G .* P1) A2^T, dA2 = s B2^T (G .* P1)"""
    g, a1, b1, a2, b2 = (t.double() for t in (dW, A1, B1, A2, B2))
    x1, x2 = g * (b2 @ a2), g * (b1 @ a1)
    sc = f32(s)
    return {"A1": sc * (b1.t() @ x1), "B1": sc * (x1 @ a1.t()), "A2": sc * (b2.t() @ x2), "B2": sc * (x2 @ a2.t())}


def project_bound(dW, A1, B1, A2, B2, s: float):
    """delta per element of the four projections, |fp32 result - project64| <= delta, accumulated operation by operation.  Each fp32
    operation adds 2^-24 of the magnitude of its (computed) result; a sum of N terms in ANY order (fused with its products or not) adds
    (N - 1) 2^-24 sum |terms|; errors of an operand are carried through the operation that reads it.  In order:
      P   = sum_k B[o][k] A[k][i]        r products, a sum of r terms                     eP  = r 2^-24 sum_k |B| |A|            (of the OTHER pair)
      X   = G * P                        G is exact; one product                          eX  = |G| eP + 2^-24 |G| (|P| + eP)
      t_j = X * A[k][j] | B[o][k] * X    one product per term                             et  = |factor| eX + 2^-24 |factor| (|X| + eX)
      acc = sum_j t_j                    N = in (dB) | out (dA) terms                     eacc = sum et + (N - 1) 2^-24 sum (|t| + et)
      out = s * acc                      one product                                      delta = |s| eacc + 2^-24 |s| (|acc| + eacc)
    with |acc| <= sum |t| (the magnitude the last two lines use).  The rows and columns past a target that a tile pads add exact zeros."""
    g = dW.double().abs()
    f = {"A1": A1.double().abs(), "B1": B1.double().abs(), "A2": A2.double().abs(), "B2": B2.double().abs()}
    exact = {"1": (B1.double() @ A1.double()).abs(), "2": (B2.double() @ A2.double()).abs()}
    r = A1.shape[0]
    out, inn = dW.shape
    sc = abs(f32(s))
    bound = {}
    for mine, other in (("1", "2"), ("2", "1")):
        eP = r * U24 * (f["B" + other] @ f["A" + other])
        magP = exact[other] + eP
        eX = g * eP + U24 * g * magP
        magX = g * exact[other] + eX                                  # >= |computed X|
        for name, n in (("B" + mine, inn), ("A" + mine, out)):
            if name[0] == "B":                                       # dB[o][k] = s sum_i X[o][i] A[k][i]
                fac = f["A" + mine].t()
                sum_t, sum_et = (g * exact[other]) @ fac, eX @ fac + U24 * (magX @ fac)
            else:                                                    # dA[k][i] = s sum_o B[o][k] X[o][i]
                fac = f["B" + mine].t()
                sum_t, sum_et = fac @ (g * exact[other]), fac @ eX + U24 * (fac @ magX)
            eacc = sum_et + (n - 1) * U24 * (sum_t + sum_et)
            bound[name] = sc * eacc + U24 * sc * (sum_t + eacc)
    return bound
