"""Float64 reference of the fused Adafactor update (include/sdxlstep.h, algorithm 3), per tensor, from a table; the error bounds a float32
implementation of it must keep; and a float32 emulation on the CPU (with switchable single defects) that the bounds are tried on.

The reference takes the scalars as the library rounds them (a host double rounded to float32 once: b2t, 1 - b2t, rho, eps1, ...) and the
inputs of one step as float32 values (the state before the step, the gradient as the kernel sees it); every operation is then exact to
float64, so what separates a correct float32 implementation from it is the rounding of its own operations, bounded below.
U = 2^-24 is the unit roundoff of float32, UB = 2^-8 that of bf16."""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import NamedTuple, Optional

import numpy as np
import torch

U = 2.0 ** -24
UB = 2.0 ** -8
AF_ROWS, AF_COLS = 128, 256          # the tile of the launches (SDXL_AF_ROWS, SDXL_AF_COLS)
# a tile's sum of 256 x 128 terms: a thread adds 128 terms in sequence, the workgroup's tree has 8 levels, the tiles are added in
# double precision and rounded once
TILE_SUM_OPS = 128 + 8 + 1

f32 = np.float32


def r32(x) -> float:
    """a host double as the library uses it: rounded to float32 once"""
    return float(f32(x))


@dataclass
class Hyper:
    lr: Optional[float] = None
    eps: tuple = (1e-30, 1e-3)
    clip_threshold: float = 1.0
    decay_rate: float = -0.8
    beta1: Optional[float] = None
    weight_decay: float = 0.0
    scale_parameter: bool = True
    relative_step: Optional[bool] = None
    warmup_init: bool = False
    grad_round_bf16: bool = False

    def __post_init__(self):
        if self.relative_step is None:
            self.relative_step = self.lr is None

    def beta2t(self, k: int) -> float:
        return 1.0 - math.pow(k, self.decay_rate)

    def rho(self, k: int) -> float:
        if self.relative_step:
            return min(1e-6 * k if self.warmup_init else 1e-2, 1.0 / math.sqrt(k))
        return float(self.lr)

    def scalars(self, k: int) -> "Scalars":
        b1 = 0.0 if self.beta1 is None else self.beta1
        return Scalars(r32(self.beta2t(k)), r32(1.0 - self.beta2t(k)), r32(self.rho(k)), r32(self.eps[0]), r32(self.eps[1]),
                       r32(self.clip_threshold), r32(b1), r32(1.0 - b1), r32(self.weight_decay), bool(self.scale_parameter),
                       self.beta1 is not None)


class Scalars(NamedTuple):
    b2t: float
    omb2t: float
    rho: float
    eps1: float
    eps2: float
    clip: float
    b1: float
    omb1: float
    wd: float
    scale_parameter: bool
    use_beta1: bool


class Entry(NamedTuple):
    elem_off: int
    rows: int
    cols: int
    numel: int
    factored: bool
    state_off: int

    @property
    def span(self) -> int:
        return self.rows * self.cols

    def state_floats(self) -> int:
        return (self.rows + self.cols + 3) // 4 * 4 if self.factored else self.span


def scratch_floats(entries) -> int:
    """adafactor_scratch_floats of include/sdxlstep.h, restated"""
    total = 4 * len(entries)
    for e in entries:
        ncb, nrb = -(-e.cols // AF_COLS), -(-e.rows // AF_ROWS)
        total += 2 * nrb * ncb
        if e.factored:
            total += -(-e.rows // 256) + e.rows * ncb + nrb * e.cols
    return total


def bf16_round(x: np.ndarray) -> np.ndarray:
    return torch.from_numpy(np.ascontiguousarray(x, dtype=f32)).to(torch.bfloat16).float().numpy()


def grad_in(g: torch.Tensor, scale: Optional[float], hp: Hyper) -> np.ndarray:
    """the gradient as the update sees it, float32: times the scale (one float32 product), then bf16 with grad_round_bf16"""
    gr = g.float().numpy() * f32(1.0 if scale is None else scale)
    return bf16_round(gr) if hp.grad_round_bf16 else gr.astype(f32)


def ema_step(e: torch.Tensor, p: torch.Tensor, omd: float) -> torch.Tensor:
    """the fused EMA on the new bf16 p: t1 = e - p, t2 = omd * t1, e - t2, each a float32 op"""
    omd = torch.tensor(omd, dtype=torch.float32)
    return e - omd * (e - p.float())


# ---------------------------------------------------------------------------------------------- float64
def step64(e: Entry, gr, x, state, m, sc: Scalars):
    """One step of one tensor.  gr, x, m: [rows][cols] float64 (pads hold 0); state: {"R", "C"} or {"v"} before the step.
    Returns a dict of float64 results: R, C | v, mean, u, su, sx, rms_u, rms_p, rho_t, eta_t, d, m, x."""
    q = gr * gr + sc.eps1
    out = {}
    if e.factored:
        R = sc.b2t * state["R"] + sc.omb2t * (q.sum(axis=1) / e.cols)
        C = sc.b2t * state["C"] + sc.omb2t * (q.sum(axis=0) / e.rows)
        mean = R.sum() / e.rows
        u = ((1.0 / np.sqrt(R / mean))[:, None] * (1.0 / np.sqrt(C))[None, :]) * gr
        out.update(R=R, C=C, mean=mean)
    else:
        v = sc.b2t * state["v"] + sc.omb2t * q
        u = (1.0 / np.sqrt(v)) * gr
        out.update(v=v)
    su, sx = float((u * u).sum()), float((x * x).sum())
    rms_u = math.sqrt(su / e.numel)
    rms_p = math.sqrt(sx / e.numel) if sc.scale_parameter else 0.0
    rho_t = sc.rho * max(sc.eps2, rms_p) if sc.scale_parameter else sc.rho
    eta_t = rho_t / max(1.0, rms_u / sc.clip)
    d = eta_t * u
    m1 = None
    if sc.use_beta1:
        m1 = sc.b1 * m + sc.omb1 * d
        d = m1
    dx = (sc.wd * rho_t) * x if sc.wd != 0.0 else np.zeros_like(x)
    x1 = x - dx - d
    out.update(u=u, su=su, sx=sx, rms_u=rms_u, rms_p=rms_p, rho_t=rho_t, eta_t=eta_t, d=d, m=m1, dx=dx, x=x1, x0=x)
    return out


def bounds(e: Entry, ref, state, m, sc: Scalars):
    """What a float32 implementation with the documented summation geometry may differ from step64 by, given the same inputs.
    R, C, v: (N - 1) U sum|terms| for a sum of N terms in any order, plus one U per rounded operation on the way (first order, with
    a factor 1 + 2^-10 for the higher orders).  Everything positive there, so those are relative bounds, and they are carried
    through the reciprocal square roots into u, the sums of u^2, the scalars and the update."""
    hi = 1.0 + 2.0 ** -10
    b = {}
    if e.factored:
        # q: 2 operations; the sum of N terms; / cols, * omb2t, b2t * R, the sum: 4 more
        eR, eC = (e.cols - 1 + 6) * U * hi, (e.rows - 1 + 6) * U * hi
        b["R"], b["C"] = eR * ref["R"], eC * ref["C"]
        e_mean = eR + (e.rows - 1 + 1) * U * hi          # the rows' R' added in any order, / rows
        # rf = 1 / sqrt(R' / mean): the quotient, the root (which halves the incoming error), the reciprocal; cf likewise; two products
        eU = ((eR + e_mean + U) / 2 + 2 * U + eC / 2 + 2 * U + 2 * U) * hi
    else:
        b["v"] = 5 * U * hi * ref["v"]
        eU = (5 * U / 2 + 2 * U + U) * hi
    e_su = (2 * eU + U + TILE_SUM_OPS * U) * hi           # u*u, then the tile sums
    e_sx = (3 * U + TILE_SUM_OPS * U) * hi                # x = p + c (one operation), x*x, the tile sums
    e_rms_u = (e_su + U) / 2 + U
    e_rms_p = ((e_sx + U) / 2 + U) if sc.scale_parameter else 0.0
    e_rho = (e_rms_p + U) if sc.scale_parameter else 0.0
    e_eta = e_rho + e_rms_u + 2 * U
    b["rho_t"], b["eta_t"] = e_rho * hi * abs(ref["rho_t"]), e_eta * hi * abs(ref["eta_t"])
    b["rms_u"], b["rms_p"] = e_rms_u * hi * ref["rms_u"], e_rms_p * hi * ref["rms_p"]
    raw_d = ref["eta_t"] * np.abs(ref["u"])
    b_d = (e_eta + eU + U) * hi * raw_d
    if sc.use_beta1:
        b_d = U * np.abs(sc.b1 * m) + sc.omb1 * b_d + U * sc.omb1 * raw_d + U * np.abs(ref["m"])
        b["m"] = b_d * hi
    ax = np.abs(ref["x0"])
    # x - dx: dx = (wd*rho_t)*x carries e_rho and two products; the difference one rounding, x itself one; then - d, one more
    b_x = np.abs(ref["dx"]) * (e_rho + 3 * U) + 2 * U * ax + b_d + U * np.abs(ref["x"])
    b["x"] = b_x * hi
    # p' + c': c' = bf16(x - p') is a bf16 rounding of a difference that is itself at most a bf16 rounding of x
    b["pc"] = b["x"] + UB * UB * (np.abs(ref["x"]) + b["x"]) * hi
    return b


# ---------------------------------------------------------------------------------------------- float32 emulation
MUTANTS = ("no_eps1", "cols_for_rows", "stale_mean", "numel_with_pads", "clip_below", "no_eps2_floor", "decay_by_eta", "drop_last_row_block")


def _sum32(a: np.ndarray, axis, order: str) -> np.ndarray:
    """a float32 sum along an axis in one of two orders, neither the kernels': "pairwise" is numpy's own (blocks, then a tree), "reverse"
    the same over the flipped axis.  Both add at most a few dozen terms into any one partial sum, as the kernels do."""
    a = a.astype(f32)
    if order == "reverse":
        a = np.flip(a, axis=axis)
    return np.ascontiguousarray(a).sum(axis=axis, dtype=f32)


def emulate32(e: Entry, gr, x, state, m, sc: Scalars, order: str = "pairwise", mutant: Optional[str] = None, prev_mean=None):
    """The step in float32 on the CPU, every operation rounded on its own, sums in the given order.  mutant: one of MUTANTS, a single
    defect.  Inputs as float32 arrays; returns what step64 returns (float64 views of the float32 results)."""
    assert mutant is None or mutant in MUTANTS
    F = lambda v: f32(v)
    gr, x = gr.astype(f32), x.astype(f32)
    q = gr * gr if mutant == "no_eps1" else gr * gr + F(sc.eps1)
    out = {}
    if e.factored:
        qq = q
        if mutant == "drop_last_row_block" and e.rows > 1:
            last = (e.rows - 1) // AF_ROWS * AF_ROWS
            qq = q.copy()
            qq[max(last, 1):] = 0                          # the last row block never reaches the sums
        rows_div = F(e.cols if mutant == "cols_for_rows" else e.rows)
        R = F(sc.b2t) * state["R"].astype(f32) + F(sc.omb2t) * (_sum32(qq, 1, order) / F(e.cols))
        C = F(sc.b2t) * state["C"].astype(f32) + F(sc.omb2t) * (_sum32(qq, 0, order) / rows_div)
        mean = _sum32(R, 0, order) / F(e.rows)
        used = F(prev_mean) if (mutant == "stale_mean" and prev_mean is not None) else mean
        rf = F(1) / np.sqrt(R / used)
        cf = F(1) / np.sqrt(C)
        u = (rf[:, None] * cf[None, :]) * gr
        out.update(R=R, C=C, mean=mean)
    else:
        v = F(sc.b2t) * state["v"].astype(f32) + F(sc.omb2t) * q
        u = (F(1) / np.sqrt(v)) * gr
        out.update(v=v)
    u = u.astype(f32)
    su = _sum32((u * u).reshape(-1), 0, order)
    sx = _sum32((x * x).reshape(-1), 0, order)
    nf = F(e.span if mutant == "numel_with_pads" else e.numel)
    rms_u = np.sqrt(su / nf)
    rms_p = np.sqrt(sx / nf) if sc.scale_parameter else F(0)
    if sc.scale_parameter:
        rho_t = F(sc.rho) * (rms_p if mutant == "no_eps2_floor" else max(F(sc.eps2), rms_p))
    else:
        rho_t = F(sc.rho)
    ratio = rms_u / F(sc.clip)
    eta_t = rho_t / (ratio if mutant == "clip_below" else max(F(1), ratio))
    d = eta_t * u
    m1 = None
    if sc.use_beta1:
        m1 = F(sc.b1) * m.astype(f32) + F(sc.omb1) * d
        d = m1
    x1 = x
    if sc.wd != 0.0:
        x1 = x - (F(sc.wd) * (eta_t if mutant == "decay_by_eta" else rho_t)) * x
    x1 = x1 - d
    out.update(u=u, su=su, sx=sx, rms_u=rms_u, rms_p=rms_p, rho_t=rho_t, eta_t=eta_t, d=d, m=m1, x=x1)
    return {k: (None if v is None else np.asarray(v, dtype=np.float64)) for k, v in out.items()}


def fractions(e: Entry, got, ref, bnd, keys=None):
    """{key: the largest |got - ref| / bound} over the keys both have (a zero bound with a zero difference counts as 0, with any
    other difference as infinity)"""
    out = {}
    for k in (keys or bnd):
        if k not in got or got[k] is None or k not in bnd:
            continue
        want = ref["x"] if k == "pc" else ref[k]
        diff = np.abs(np.asarray(got[k], dtype=np.float64) - want)
        bd = np.asarray(bnd[k], dtype=np.float64)
        with np.errstate(divide="ignore", invalid="ignore"):
            frac = np.where(diff == 0, 0.0, np.where(bd > 0, diff / bd, np.inf))
        frac = np.where(np.isnan(frac), np.inf, frac)
        out[k] = float(np.max(frac))
    return out
