"""Per-tensor gradient comparison: every tensor of a HIP gradient against a reference gradient, in float64.

Not a test module (the leading underscore keeps it out of collection).  The GPU tests feed it either the tensors
`net.export(k, grad=True)` returns or raw slices of `net.grads` located by `net.param_ranges()`, with the fp32 oracle's
autograd gradients or another HIP arena as the reference.  Per tensor it records the relative L2 error |g - r| / |r|, the
cosine, finiteness, |g| and |r|; a tensor whose reference gradient is exactly zero must have max |g| <= 1e-6 * max |r| over
the whole arena instead.  The report has one line per role (the key with every block index replaced by N) naming that
role's worst tensor; a failure lists the ten worst tensors by name."""
from __future__ import annotations

import math
import re
from dataclasses import dataclass
from typing import Callable, Dict, Iterable, Optional, Tuple, Union

import torch

ZERO_REF_RTOL = 1e-6        # a zero reference gradient: max |g| <= ZERO_REF_RTOL * max |r| over the arena

Bar = Tuple[float, float]   # (max rel-L2, min cosine)


def role(key: str) -> str:
    """'up_blocks.1.attentions.2.transformer_blocks.0.attn1.to_out.0.bias' -> 'up_blocks.N.attentions.N.transformer_blocks.N.attn1.to_out.N.bias'"""
    return re.sub(r"\.\d+(?=\.|$)", ".N", key)


def group(key: str, ndim: int) -> str:
    """Coarse role group for the summary: time-embedding path, norms, biases, convs, linears."""
    if key.startswith(("time_embedding.", "add_embedding.")) or ".time_emb_proj." in key:
        return "time-embedding path"
    if "norm" in key.rsplit(".", 2)[-2]:
        return "norms"
    if key.endswith(".bias"):
        return "biases"
    return "convs" if ndim == 4 else "linears"


@dataclass
class Row:
    key: str
    ndim: int
    numel: int
    rel: float          # |g - r| / |r|  (nan when r == 0)
    cos: float          # <g, r> / (|g| |r|)  (nan when r == 0 or g == 0)
    finite: bool
    g: float            # |g|
    r: float            # |r|
    gmax: float         # max |g|
    rmax: float         # max |r|


class GradParity:
    def __init__(self, label: str):
        self.label = label
        self.rows: Dict[str, Row] = {}
        self._rmax: Optional[float] = None

    def add(self, key: str, got: torch.Tensor, ref: torch.Tensor, ndim: Optional[int] = None) -> Row:
        """Compare one tensor (any device, any float dtype; shapes must hold the same number of elements)."""
        assert key not in self.rows, f"{key} compared twice"
        a = got.detach().reshape(-1).to(torch.float64)
        b = ref.detach().reshape(-1).to(device=a.device, dtype=torch.float64)
        assert a.numel() == b.numel(), (key, a.numel(), b.numel())
        finite = bool(torch.isfinite(a).all())
        g, r, d, dot = (float(v) for v in torch.stack([a.norm(), b.norm(), (a - b).norm(), a @ b]).cpu())
        gmax = float(a.abs().max()) if a.numel() else 0.0
        rmax = float(b.abs().max()) if b.numel() else 0.0
        rel = d / r if r > 0 else math.nan
        cos = dot / (g * r) if g > 0 and r > 0 else math.nan
        row = Row(key, got.dim() if ndim is None else ndim, a.numel(), rel, cos, finite, g, r, gmax, rmax)
        self.rows[key] = row
        self._rmax = None
        return row

    def add_arena(self, got: torch.Tensor, ref: torch.Tensor, ranges: Dict[str, Tuple[int, int]],
                  shapes: Optional[Dict[str, Tuple[int, ...]]] = None) -> None:
        """Every tensor of two packed gradient arenas (same layout), slice by slice: nothing is copied off the device."""
        for k, (off, n) in ranges.items():
            self.add(k, got[off:off + n], ref[off:off + n], ndim=len(shapes[k]) if shapes is not None else None)

    # ------------------------------------------------------------------ checking
    def arena_rmax(self) -> float:
        if self._rmax is None:
            self._rmax = max((r.rmax for r in self.rows.values()), default=0.0)
        return self._rmax

    def verdict(self, row: Row, bar: Bar) -> Tuple[bool, float]:
        """(passes, badness): badness >= 1 fails; it orders tensors worst first."""
        if not row.finite:
            return False, math.inf
        if row.r == 0.0:
            lim = ZERO_REF_RTOL * self.arena_rmax()
            bad = row.gmax / lim if lim > 0 else (math.inf if row.gmax > 0 else 0.0)
            return bad <= 1.0, bad
        rel_max, cos_min = bar
        cos = row.cos if not math.isnan(row.cos) else -1.0
        bad = max(row.rel / rel_max, (1.0 - cos) / (1.0 - cos_min))
        return row.rel <= rel_max and cos >= cos_min, bad

    @staticmethod
    def _fmt(row: Row) -> str:
        if row.r == 0.0:
            return f"zero reference, max|g| {row.gmax:.3e}"
        return f"rel-L2 {row.rel:.3e} cos {row.cos:.6f} |g| {row.g:.3e} |r| {row.r:.3e}"

    def report(self, bar: Callable[[str], Bar], printer=print) -> None:
        """One line per role with its worst tensor, then the worst rel-L2 / cosine per role group."""
        by_role: Dict[str, list] = {}
        for row in self.rows.values():
            by_role.setdefault(role(row.key), []).append(row)
        printer(f"[gradparity] {self.label}: {len(self.rows)} tensors, {sum(r.numel for r in self.rows.values())} values, "
                f"{len(by_role)} roles")
        groups: Dict[str, list] = {}
        for rl in sorted(by_role):
            rows = by_role[rl]
            worst = max(rows, key=lambda r: self.verdict(r, bar(r.key))[1])
            ok = all(self.verdict(r, bar(r.key))[0] for r in rows)
            b = bar(worst.key)
            printer(f"[gradparity] {self.label} {'ok  ' if ok else 'FAIL'} {rl} (x{len(rows)}, bar {b[0]:.0e}/{b[1]}): "
                    f"worst {worst.key}: {self._fmt(worst)}")
            for r in rows:
                groups.setdefault(group(r.key, r.ndim), []).append(r)
        for gname in sorted(groups):
            rows = [r for r in groups[gname] if r.r > 0]
            if not rows:
                continue
            wr = max(rows, key=lambda r: r.rel)
            wc = min(rows, key=lambda r: r.cos if not math.isnan(r.cos) else -1.0)
            printer(f"[gradparity] {self.label} group {gname} ({len(groups[gname])} tensors): worst rel-L2 {wr.rel:.3e} ({wr.key}), "
                    f"worst cos {wc.cos:.6f} ({wc.key})")

    def check(self, bar: Union[Bar, Callable[[str], Bar]], expect: Optional[Iterable[str]] = None, printer=print) -> None:
        """Report, then assert that every tensor passes its bar (and, given `expect`, that exactly those keys were compared)."""
        bar_fn = bar if callable(bar) else (lambda k, b=bar: b)
        self.report(bar_fn, printer)
        if expect is not None:
            want = set(expect)
            missing, extra = sorted(want - set(self.rows)), sorted(set(self.rows) - want)
            assert not missing and not extra, f"{self.label}: missing {missing[:10]} extra {extra[:10]}"
        assert self.arena_rmax() > 0, f"{self.label}: the reference gradient is zero everywhere"
        scored = sorted(((self.verdict(r, bar_fn(r.key)), r) for r in self.rows.values()), key=lambda t: -t[0][1])
        failed = [r for (ok, _), r in scored if not ok]
        if failed:
            lines = [f"  {'FAIL' if not ok else 'ok  '} {r.key}: {self._fmt(r)} (bar rel-L2 <= {bar_fn(r.key)[0]:.0e}, "
                     f"cos >= {bar_fn(r.key)[1]})" for (ok, _), r in scored[:10]]
            raise AssertionError(f"{self.label}: {len(failed)} of {len(self.rows)} gradient tensors fail their bar; "
                                 f"the ten worst:\n" + "\n".join(lines))


def compare_autograd(parity: GradParity, loss: torch.Tensor, params: Dict[str, torch.Tensor],
                     got: Callable[[str], torch.Tensor]) -> None:
    """Backward of the oracle `loss` into every tensor of `params` (leaves with requires_grad): each gradient is compared
    with got(key) the moment autograd has accumulated it, then dropped -- the reference gradients never all exist at once.
    A parameter the loss does not reach has a zero reference gradient."""
    hooks = []
    for k, p in params.items():
        assert p.is_leaf and p.requires_grad and p.grad is None, k

        def hook(t, k=k):
            parity.add(k, got(k), t.grad)
            t.grad = None

        hooks.append(p.register_post_accumulate_grad_hook(hook))
    try:
        loss.backward()
    finally:
        for h in hooks:
            h.remove()
    for k, p in params.items():
        if k not in parity.rows:
            parity.add(k, got(k), torch.zeros_like(p))
