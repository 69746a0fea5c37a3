"""Reference arithmetic of LoKr by merge and project (not a test module): dW = s kron(C, W2), W2 stored in full or W2 = B A.  The
factorisation restated from its description in words; the merge restated in separate fp32 torch ops, bit for bit what csrc/lokr.hip
computes; the projections in float64 from the bf16 factors; and their a-priori error bound, accumulated operation by operation next to the
float64 reference.  No constant here comes from a kernel's output.

Shapes (the SOURCE view: the state-dict tensor flattened to [out, in], in = cin kh kw): W0, dW [out, in]; C [out_l, in_m]; a FULL target
has W2 [out_k, n2] and A is None; a FACTORED one passes B [out_k, r] in W2's place and A [r, n2].  n2 = in_n kh kw and W2 / A columns are
j = d kh kw + tap (the state-dict order), so source column i = (b in_n + d) kh kw + tap = b n2 + j."""
from __future__ import annotations

import torch

from _loha_ref import CONV3, GEGLU, PLAIN, _chain, to_native, to_source      # noqa: F401  (the layout maps are the packed layouts' own)
from _lora_ref import U24, f32


def fact(dimension: int, factor: int = -1):
    """(m, n), m <= n, m n = dimension.  factor > 0 dividing the dimension: (factor, dimension / factor), the smaller first.  Otherwise
    factor < 0 means factor = dimension; from (1, dimension), while m < n take the next divisor m' > m and n' = dimension / m', stop if
    m' + n' > m + n or m' > factor, else step."""
    if factor > 0 and dimension % factor == 0:
        return tuple(sorted((factor, dimension // factor)))
    if factor < 0:
        factor = dimension
    m, n = 1, dimension
    while m < n:
        m2 = next(d for d in range(m + 1, dimension + 1) if dimension % d == 0)
        n2 = dimension // m2
        if m2 + n2 > m + n or m2 > factor:
            break
        m, n = m2, n2
    return tuple(sorted((m, n)))


def geometry(out: int, cin: int, khw: int, factor: int):
    """(out_l, out_k, in_m, in_n, n2): the channel count is factorised, not in = cin khw"""
    out_l, out_k = fact(out, factor)
    in_m, in_n = fact(cin, factor)
    return out_l, out_k, in_m, in_n, in_n * khw


def rule_full(out_k: int, in_n: int, rank: int, forced: bool = False) -> bool:
    """LyCORIS' form rule (decompose_both off): the second factor is stored in full when asked to or when 2 r >= max(out_k, in_n)"""
    return bool(forced) or 2 * rank >= max(out_k, in_n)


def target_scale(full: bool, alpha: float, rank: int) -> float:
    return 1.0 if full else alpha / rank


def names(A) -> tuple:
    """the outputs of a projection, in arena order"""
    return ("C", "W2") if A is None else ("C", "B", "A")


def _w2_64(W2, A):
    return W2.double() if A is None else W2.double() @ A.double()


def _outer(C, q):
    """[a out_k + c][b n2 + j] = C[a][b] * q[c][j], one multiplication per element in the dtype of the arguments"""
    return (C[:, None, :, None] * q[None, :, None, :]).reshape(C.shape[0] * q.shape[0], C.shape[1] * q.shape[1])


# ---- merge
def merge(W0, C, W2, A, s: float) -> torch.Tensor:
    """factored: q <- q + B[c][k] A[k][j], k ascending, the product and the sum separate fp32 ops; full: q = (float)W2.  h = C[a][b] * q,
    t = s * h, W = bf16_rn(W0 + t), every operation a separate fp32 op (no FMA), and W = W0 where t == 0.  All bf16; any device."""
    assert W0.dtype == C.dtype == W2.dtype == torch.bfloat16 and (A is None or A.dtype == torch.bfloat16)
    q = W2.float() if A is None else _chain(A, W2)
    h = _outer(C.float(), q)
    t = h * torch.tensor(f32(s), dtype=torch.float32, device=W0.device)
    w = (W0.float() + t).to(torch.bfloat16)
    return torch.where(t == 0, W0, w)


def delta64(C, W2, A, s: float) -> torch.Tensor:
    """s kron(C, W2) in float64, written out element by element (tests compare it with torch.kron)"""
    return f32(s) * _outer(C.double(), _w2_64(W2, A))


# ---- project
def project64(dW, C, W2, A, s: float):
    """{"C": dC, "W2": dW2} (full) or {"C": dC, "B": dB, "A": dA} (factored) in float64 from the bf16 factors:
    dC[a][b] = s sum_{c,j} G W2[c][j], dW2[c][j] = s sum_{a,b} C[a][b] G, dB = dW2 A^T, dA = B^T dW2"""
    c, w2 = C.double(), _w2_64(W2, A)
    g = dW.double().view(c.shape[0], w2.shape[0], c.shape[1], w2.shape[1])      # [a][c][b][j]
    sc = f32(s)
    dC = sc * torch.einsum("acbj,cj->ab", g, w2)
    dW2 = sc * torch.einsum("ab,acbj->cj", c, g)
    if A is None:
        return {"C": dC, "W2": dW2}
    return {"C": dC, "B": dW2 @ A.double().t(), "A": W2.double().t() @ dW2}


def project_bound(dW, C, W2, A, s: float):
    """delta per element of the projections, |fp32 result - project64| <= delta, accumulated operation by operation.  Each fp32 operation
    adds 2^-24 of the magnitude of its (computed) result; a sum of N terms in ANY order (fused with its products or not, split into
    partial sums or not) adds (N - 1) 2^-24 sum |terms|; errors of an operand are carried through the operation that reads it.  In order:
      W2  = sum_k B[c][k] A[k][j]      factored only: r products, a sum of r terms      eW   = r 2^-24 sum_k |B| |A|        (full: exact, 0)
      t   = G * W2                     G is exact; one product per term                 et   = |G| eW + 2^-24 |G| (|W2| + eW)
      acc = sum_{c,j} t                N = out_k n2 terms                               eacc = sum et + (N - 1) 2^-24 sum (|t| + et)
      dC  = s * acc                    one product                                      dC's delta = |s| eacc + 2^-24 |s| (sum |t| + eacc)
      u   = C[a][b] * G                both exact; one product per term                 eu   = 2^-24 |C| |G|
      acc = sum_{a,b} u                N = out_l in_m terms                             eacc = sum eu + (N - 1) 2^-24 sum (|u| + eu)
      D   = s * acc                    (dW2 of a full target)                           eD   = |s| eacc + 2^-24 |s| (sum |u| + eacc)
      dB  = sum_j D[c][j] A[k][j]      N = n2 products and terms                        sum_j (eD |A| + 2^-24 (|D| + eD) |A|) + (N - 1) 2^-24 sum (...)
      dA  = sum_c B[c][k] D[c][j]      N = out_k                                        likewise
    with |acc| <= sum |t| (the magnitude the scaling lines use).  Elements past a tile's end add exact zeros."""
    c, g0 = C.double().abs(), dW.double().abs()
    w2 = _w2_64(W2, A)
    out_l, in_m = c.shape
    out_k, n2 = w2.shape
    g = g0.view(out_l, out_k, in_m, n2)
    sc = abs(f32(s))
    eW = torch.zeros_like(w2) if A is None else A.shape[0] * U24 * (W2.double().abs() @ A.double().abs())
    magW = w2.abs() + eW
    bound = {}
    # dC
    n = out_k * n2
    sum_t = torch.einsum("acbj,cj->ab", g, w2.abs())
    sum_et = torch.einsum("acbj,cj->ab", g, eW) + U24 * torch.einsum("acbj,cj->ab", g, magW)
    eacc = sum_et + (n - 1) * U24 * (sum_t + sum_et)
    bound["C"] = sc * eacc + U24 * sc * (sum_t + eacc)
    # D = s dW2
    n = out_l * in_m
    sum_u = torch.einsum("ab,acbj->cj", c, g)
    sum_eu = U24 * sum_u
    eacc = sum_eu + (n - 1) * U24 * (sum_u + sum_eu)
    eD = sc * eacc + U24 * sc * (sum_u + eacc)
    if A is None:
        bound["W2"] = eD
        return bound
    D = (f32(s) * torch.einsum("ab,acbj->cj", C.double(), dW.double().view(out_l, out_k, in_m, n2))).abs()
    magD = D + eD
    for name, fac, n in (("B", A.double().abs().t(), n2), ("A", W2.double().abs().t(), out_k)):
        if name == "B":      # dB[c][k] = sum_j D[c][j] A[k][j]
            sum_t, sum_et = D @ fac, eD @ fac + U24 * (magD @ fac)
        else:                # dA[k][j] = sum_c B[c][k] D[c][j]
            sum_t, sum_et = fac @ D, fac @ eD + U24 * (fac @ magD)
        bound[name] = sum_et + (n - 1) * U24 * (sum_t + sum_et)
    return bound
