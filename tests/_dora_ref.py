"""Reference arithmetic of DoRA by merge and project (not a test module), in the SOURCE view (the state-dict tensor flattened to
[out, in]): W0, G = dW [out, in]; A [r, in], B [out, r], mu [out] bf16; n0, n [out] fp32.

  acc = sum_k B[o][k] A[k][i]   LoRA's chain, every product and sum a separate fp32 op;   t = s acc;   v = (float)W0 + t
  n_o = sqrt(sum_i v^2);  n0_o = n_o at t == 0;  q_o = n0_o / n_o (1 when n_o == 0);  c_o = (1 + (float)mu_o) q_o
  W = bf16_rn(c_o v), and W0's bits where t == 0 and c_o == 1
  r_o = sum_i G v;  dmu_o = q_o r_o;  dB[o][k] = c_o (s sum_i G A[k][i]);  dA[k][i] = s sum_o (c_o B[o][k]) G[o][i]      (n_o held constant)

merge_given restates the merge in separate fp32 torch ops, bit for bit what csrc/dora.hip computes GIVEN the two norms (a row norm is a
reduction: its bits depend on the summation tree, so it is bounded, not restated); ref64 / project64 are the float64 references from the
bf16 operands; bounds() is the a-priori error bound of every output, accumulated operation by operation next to the float64 reference:
2^-24 of the computed magnitude per fp32 operation, (N - 1) 2^-24 sum |terms| for a sum of N terms in any order, 2^-23 for the square root
and for the division; the error of an operand is carried through the operation that reads it.  No constant comes from a kernel's output."""
from __future__ import annotations

import torch

from _loha_ref import CONV3, GEGLU, PLAIN, _chain, to_native, to_source      # noqa: F401  (the layout maps are the packed layouts' own)
from _lora_ref import U24, f32

U23 = 2.0 ** -23


def v32(W0, A, B, s: float):
    """(v, t) in fp32 exactly as the kernels form them"""
    assert W0.dtype == A.dtype == B.dtype == torch.bfloat16
    t = _chain(A, B) * torch.tensor(f32(s), dtype=torch.float32, device=W0.device)
    return W0.float() + t, t


def coef32(mu, n0, n):
    """(q, c) in fp32: one division, one sum, one product; q = 1 where n == 0"""
    q = torch.where(n == 0, torch.ones_like(n), n0 / n)
    return q, (1.0 + mu.float()) * q


def merge_given(W0, A, B, mu, s: float, n0, n) -> torch.Tensor:
    """the merged weight with the row norms taken as given (fp32 [out])"""
    v, t = v32(W0, A, B, s)
    _q, c = coef32(mu, n0, n)
    w = (c[:, None] * v).to(torch.bfloat16)
    return torch.where((t == 0) & (c[:, None] == 1), W0, w)


def ref64(W0, A, B, mu, s: float):
    """float64 from the bf16 operands: v, n, n0, q, c and the unrounded merged weight W = c v"""
    v = W0.double() + f32(s) * (B.double() @ A.double())
    n, n0 = v.pow(2).sum(1).sqrt(), W0.double().pow(2).sum(1).sqrt()
    q = torch.where(n == 0, torch.ones_like(n), n0 / n)
    c = (1.0 + mu.double()) * q
    return dict(v=v, n=n, n0=n0, q=q, c=c, W=c[:, None] * v)


def project64(G, W0, A, B, mu, s: float):
    """{"mu": dmu, "B": dB, "A": dA} in float64, the norm a constant"""
    x = ref64(W0, A, B, mu, s)
    g = G.double()
    return {"mu": x["q"] * (g * x["v"]).sum(1), "B": x["c"][:, None] * (f32(s) * (g @ A.double().t())),
            "A": f32(s) * ((x["c"][:, None] * B.double()).t() @ g)}


def magnitude64(n0, mu):
    """DoRA's magnitude m = n0 (1 + mu)"""
    return n0.double() * (1.0 + mu.double())


def _op(x, e):
    """the error after one more fp32 operation whose exact result has magnitude x and whose operands carried e into it"""
    return e + U24 * (x + e)


def _sum(terms, eterms, dim):
    """a sum of N terms (magnitudes `terms`, errors `eterms`) along dim, in any order"""
    n = terms.shape[dim]
    return eterms.sum(dim) + (n - 1) * U24 * (terms + eterms).sum(dim)


def _norm_bound(v, ev):
    """n = sqrt(sum_i v^2) from v with error ev: the squares, the sum, the root (2^-23)"""
    sq = v * v
    esq = _op(sq, 2 * v.abs() * ev + ev * ev)
    S = sq.sum(1)
    eS = _sum(sq, esq, 1)
    root = S.sqrt()
    carried = torch.where(S > 0, eS / root.clamp_min(1e-300), eS.sqrt())      # |sqrt(a) - sqrt(b)| <= |a - b| / sqrt(a), and <= sqrt|a - b|
    return carried + U23 * (root + carried)


def bounds(W0, A, B, mu, s: float, G=None):
    """delta per element: |fp32 result - float64 reference| <= delta for n0, n, q, c, W (before its bf16 rounding: the interval form
    bf16_rn(ref - delta) <= got <= bf16_rn(ref + delta)) and, with G, mu (dmu), B (dB), A (dA).  In order:
      p = B A (r products), acc = sum_k p, t = s acc, v = W0 + t;  v^2, sum_i, sqrt;  q = n0 / n (2^-23);  1 + mu;  c = (1 + mu) q;  c v
      G v, sum_i, q r;   G A, sum_i, s acc, c x;   c B, (c B) G, sum_o, s acc
    A row whose norm the bound cannot keep away from 0 gets an infinite delta (q is then not determined)."""
    sc = abs(f32(s))
    x = ref64(W0, A, B, mu, s)
    a, b = A.double().abs(), B.double().abs()
    r = A.shape[0]
    Sp = b @ a                                               # sum_k |B| |A|
    ep = U24 * Sp                                            # the products
    eacc = ep + (r - 1) * U24 * (Sp + ep)
    acc = (B.double() @ A.double()).abs()
    et = _op(sc * acc, sc * eacc)
    v = x["v"].abs()
    ev = _op(v, et)
    en = _norm_bound(x["v"], ev)
    en0 = _norm_bound(W0.double(), torch.zeros_like(v))
    n, n0 = x["n"], x["n0"]
    safe = n > en
    eq = torch.where(safe, (en0 * n + n0 * en) / (n * (n - en).clamp_min(1e-300)), torch.full_like(n, float("inf")))
    eq = eq + U23 * (x["q"].abs() + eq)
    zero = (n == 0) & (en == 0)                              # an exactly zero row: q = 1 by definition
    eq = torch.where(zero, torch.zeros_like(eq), eq)
    m1 = (1.0 + mu.double()).abs()
    em1 = U24 * m1
    q = x["q"].abs()
    c = x["c"].abs()
    ec = _op(c, m1 * eq + em1 * q + em1 * eq)
    eW = _op(c[:, None] * v, c[:, None] * ev + ec[:, None] * v + ec[:, None] * ev)
    out = dict(n0=en0, n=en, q=eq, c=ec, W=eW)
    if G is None:
        return out
    g = G.double().abs()
    # dmu
    term = g * v
    eterm = _op(term, g * ev)
    rr = (G.double() * x["v"]).sum(1).abs()
    er = _sum(term, eterm, 1)
    out["mu"] = _op(q * rr, q * er + eq * rr + eq * er)
    # dB
    St = g @ a.t()                                           # sum_i |G| |A|  [out, r]
    et_ = U24 * St
    eacc = et_ + (G.shape[1] - 1) * U24 * (St + et_)
    xx = sc * (G.double() @ A.double().t()).abs()
    ex = _op(sc * St, sc * eacc)
    out["B"] = _op(c[:, None] * xx, c[:, None] * ex + ec[:, None] * xx + ec[:, None] * ex)
    # dA
    cb = c[:, None] * b
    ecb = _op(cb, ec[:, None] * b)
    Su = cb.t() @ g                                          # sum_o |c B| |G|  [r, in]
    Eu = ecb.t() @ g
    eu = Eu + U24 * (Su + Eu)
    eacc = eu + (G.shape[0] - 1) * U24 * (Su + eu)
    out["A"] = _op(sc * Su, sc * eacc)
    return out


def bf16_interval(ref, delta):
    """(lo, hi) bf16: bf16_rn(ref - delta), bf16_rn(ref + delta), the rounding done from float64 through fp32 outwards-safe: the fp32
    conversion of a float64 is monotone, and so is the bf16 conversion of an fp32"""
    return (ref - delta).float().to(torch.bfloat16), (ref + delta).float().to(torch.bfloat16)


def exact_design(out: int, inn: int, rank: int, seed: int = 0):
    """W0, A, B in {-1, 0, 1} (bf16), integer G (fp32), s = 1: every partial sum an integer below 2^24 in ANY order, so n and n0 are the
    correctly rounded square roots of integers, r_o is an integer and dmu is one division and one product of exact values.  Asserted."""
    g = torch.Generator().manual_seed(77 + 13 * out + inn + 5 * rank + 1000 * seed)
    tri = lambda *sh: (torch.randint(-1, 2, sh, generator=g)).to(torch.bfloat16)
    W0, A, B = tri(out, inn), tri(rank, inn), tri(out, rank)
    G = torch.randint(-3, 4, (out, inn), generator=g).float()
    if rank > 16:                      # a long chain: only its first three and its last rank carry anything, so |v| stays small
        B[:, 3: rank - 1] = 0
    vmax = 1 + int((B != 0).any(0).sum())
    assert float((W0.double() + B.double() @ A.double()).abs().max()) <= vmax
    assert inn * vmax * vmax < 2 ** 24 and inn * 3 * vmax < 2 ** 24
    return W0, A, B, G


# (label, kind, out, in, cin | G): the smallest shapes at which the index arithmetic can still go wrong; "5x4104" has rows of many passes of
# the row reduction's column loop with a last pass that is not whole (tests/test_host_dora.py holds the table to DORA_R_COLS of kernels.h)
CASES = [("1x8", PLAIN, 1, 8, 0), ("8x8", PLAIN, 8, 8, 0), ("37x8", PLAIN, 37, 8, 0), ("40x24", PLAIN, 40, 24, 0),
         ("130x264", PLAIN, 130, 264, 0), ("64x2048", PLAIN, 64, 2048, 0), ("1280x1280", PLAIN, 1280, 1280, 0),
         ("conv40x16", CONV3, 40, 9 * 16, 16), ("conv8x320", CONV3, 8, 9 * 320, 320),
         ("geglu128g64x24", GEGLU, 256, 24, 64), ("geglu160g80x24", GEGLU, 320, 24, 80), ("5x4104", PLAIN, 5, 4104, 0)]
LONG_ROW = "5x4104"
BY_LABEL = {c[0]: c for c in CASES}
# ranks 1, 3 and 16, and 128 on the two large plain cases
FORMS = [(c, r) for c in CASES for r in (1, 3, 16)] + [(BY_LABEL[n], 128) for n in ("64x2048", "1280x1280")]
FORM_IDS = [f"{c[0]}-r{r}" for c, r in FORMS]
