"""Operand isolation helper (not a test module): operands placed inside one larger allocation whose every other byte the test controls.

An op may read and write its operands and nothing else.  Two runs of the same kernel on the same operand contents whose SURROUNDINGS
differ must therefore give the same bits, and the surroundings must come out as they went in.  Arena lays the operands of one call out
in one uint8 tensor filled with one byte value; what is not an operand element is guard: a band before and after every operand and the
`ld - cols` column gap of every row.  Three fills:

  0x00  the clean run;
  0xFF  bf16 0xFFFF and fp32 0xFFFFFFFF are NaN: a stale read that reaches the arithmetic poisons the result;
  0x7F  bf16 0x7F7F and fp32 0x7F7F7F7F are about 3.39e38, finite: a stale read that passes through fmaxf or a comparison, which
        swallow NaN, still moves the result.

Roles of an operand: "in" is read-only (its bits are compared after the call), "out" / "inout" are results (returned by outputs()),
"scratch" is memory the op is documented to write before it reads (never compared: its pad rows legitimately keep the fill).  An
operand without contents (`init=None`) starts as the fill pattern, so an output that is only partly overwritten, or a scratch buffer
that is read before it is written, shows."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Callable, Dict, List, Optional, Sequence

import torch

FILLS = (0x00, 0xFF, 0x7F)
ALIGN = 256
TALLEST_TILE = 256            # rows of the tallest tile in csrc/ (gemm256, gemm_cr256)
MIN_BAND = 64 * 1024


@dataclass
class Spec:
    name: str
    rows: int
    cols: int
    ld: Optional[int] = None                  # elements, >= cols (None: cols)
    dtype: torch.dtype = torch.bfloat16
    init: Optional[torch.Tensor] = None       # [rows, cols] (any float dtype, cast to dtype); None: starts as the fill pattern
    role: str = "in"                          # "in" | "out" | "inout" | "scratch"


def _isz(dtype) -> int:
    return torch.empty(0, dtype=dtype).element_size()


def _roundup(x: int, a: int) -> int:
    return (x + a - 1) // a * a


def bits(t: torch.Tensor) -> torch.Tensor:
    """the tensor's bit patterns as integers (NaN compares equal to the same NaN)"""
    t = t.contiguous()
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def same_bits(a: torch.Tensor, b: torch.Tensor) -> bool:
    return a.shape == b.shape and a.dtype == b.dtype and bool(torch.equal(bits(a), bits(b)))


class Arena:
    """256-byte aligned sub-buffers of one uint8 tensor, each between guard bands of max(256 * ld * itemsize, 64 KiB)."""

    def __init__(self, fill_byte: int, device="cpu"):
        assert 0 <= fill_byte <= 255
        self.fill = fill_byte
        self.device = torch.device(device)
        self.specs: List[Spec] = []
        self.off: Dict[str, int] = {}
        self.buf: Optional[torch.Tensor] = None
        self._snap: Optional[torch.Tensor] = None

    # ---- layout
    def add(self, spec: Spec) -> None:
        assert self.buf is None, "add every operand before the first access"
        assert spec.name not in {s.name for s in self.specs}, spec.name
        ld = spec.cols if spec.ld is None else spec.ld
        assert ld >= spec.cols > 0 and spec.rows > 0 and spec.role in ("in", "out", "inout", "scratch"), spec
        assert spec.role not in ("in", "inout") or spec.init is not None, f"{spec.name}: a read operand needs contents"
        self.specs.append(Spec(spec.name, spec.rows, spec.cols, ld, spec.dtype, spec.init, spec.role))

    def _band(self, s: Spec) -> int:
        return _roundup(max(TALLEST_TILE * s.ld * _isz(s.dtype), MIN_BAND), ALIGN)

    def commit(self) -> "Arena":
        pos = 0
        for s in self.specs:
            pos = _roundup(pos + self._band(s), ALIGN)
            self.off[s.name] = pos
            pos += s.rows * s.ld * _isz(s.dtype) + self._band(s)
        size = _roundup(pos, ALIGN)
        self._raw = torch.full((size + ALIGN,), self.fill, dtype=torch.uint8, device=self.device)      # (a CPU allocation is 64-byte aligned)
        shift = -self._raw.data_ptr() % ALIGN
        self.buf = self._raw[shift: shift + size]
        self.guard = torch.ones(self.buf.numel(), dtype=torch.bool, device=self.device)
        for s in self.specs:
            isz = _isz(s.dtype)
            g = self.guard[self.off[s.name]: self.off[s.name] + s.rows * s.ld * isz].view(s.rows, s.ld * isz)
            g[:, : s.cols * isz] = False
            if s.init is not None:
                assert tuple(s.init.shape) == (s.rows, s.cols), (s.name, tuple(s.init.shape), (s.rows, s.cols))
                self[s.name].copy_(s.init.to(device=self.device, dtype=s.dtype))
        assert self.buf.data_ptr() % ALIGN == 0
        return self

    def spec(self, name: str) -> Spec:
        return next(s for s in self.specs if s.name == name)

    def __getitem__(self, name: str) -> torch.Tensor:
        """the operand as a [rows, cols] view with row stride ld"""
        s = self.spec(name)
        isz = _isz(s.dtype)
        o = self.off[name]
        return self.buf[o: o + s.rows * s.ld * isz].view(s.dtype).view(s.rows, s.ld)[:, : s.cols]

    def ptr(self, name: str, elem_offset: int = 0) -> int:
        return self.buf.data_ptr() + self.off[name] + elem_offset * _isz(self.spec(name).dtype)

    def ld(self, name: str) -> int:
        return self.spec(name).ld

    def pattern(self, dtype) -> torch.Tensor:
        """one element of `dtype` whose bytes are the fill"""
        return torch.full((_isz(dtype),), self.fill, dtype=torch.uint8).view(dtype)[0]

    def poison(self, name: str, rows: slice) -> None:
        """overwrite rows of an operand with the fill pattern (the cross-row form); call before snapshot()"""
        s = self.spec(name)
        isz = _isz(s.dtype)
        o = self.off[name]
        self.buf[o: o + s.rows * s.ld * isz].view(s.rows, s.ld * isz)[rows, : s.cols * isz] = self.fill

    # ---- checks
    def _sync(self):
        if self.device.type == "cuda":
            torch.cuda.synchronize()

    def snapshot(self) -> None:
        self._sync()
        self._snap = self.buf.clone()

    def _where(self, byte: int) -> str:
        best = None
        for s in self.specs:
            o, n = self.off[s.name], s.rows * s.ld * _isz(s.dtype)
            d = 0 if o <= byte < o + n else min(abs(byte - o), abs(byte - (o + n - 1)))
            if best is None or d < best[0]:
                best = (d, s, byte - o)
        _, s, rel = best
        row_bytes = s.ld * _isz(s.dtype)
        if 0 <= rel < s.rows * row_bytes:
            return f"operand '{s.name}' byte offset {rel} (row {rel // row_bytes}, byte {rel % row_bytes} of the row: cols end at {s.cols * _isz(s.dtype)})"
        return f"operand '{s.name}' byte offset {rel} ({'before its first' if rel < 0 else 'behind its last'} row)"

    def assert_guards_untouched(self) -> None:
        self._sync()
        bad = (self.buf != self.fill) & self.guard
        if bool(bad.any()):
            first = int(torch.nonzero(bad)[0])
            raise AssertionError(f"guard byte written (fill 0x{self.fill:02X}): {int(bad.sum())} bytes, first at {self._where(first)}, "
                                 f"value 0x{int(self.buf[first]):02X}")

    def assert_inputs_untouched(self) -> None:
        assert self._snap is not None, "snapshot() first"
        self._sync()
        for s in self.specs:
            if s.role != "in":
                continue
            o, n = self.off[s.name], s.rows * s.ld * _isz(s.dtype)
            bad = self.buf[o: o + n] != self._snap[o: o + n]
            if bool(bad.any()):
                first = int(torch.nonzero(bad)[0])
                raise AssertionError(f"read-only operand written (fill 0x{self.fill:02X}): {int(bad.sum())} bytes, first at {self._where(o + first)}")

    def outputs(self) -> Dict[str, torch.Tensor]:
        self._sync()
        return {s.name: self[s.name].clone() for s in self.specs if s.role in ("out", "inout")}


def run_isolated(fn: Callable[[Arena], None], specs: Sequence[Spec], device="cpu", poison: Optional[Dict[str, slice]] = None,
                 fills: Sequence[int] = FILLS) -> List[Dict[str, torch.Tensor]]:
    """Run fn(arena) once per fill on identical operand contents; after each run the guards and the read-only operands must be untouched.
    Returns the "out" / "inout" operands of every run, in the order of `fills`.  `poison` (cross-row form): rows of operands that are
    overwritten with the pattern in the runs whose fill is not 0x00.  An exception from fn (a failed HIP call) ends everything."""
    runs = []
    for fill in fills:
        a = Arena(fill, device)
        for s in specs:
            a.add(s)
        a.commit()
        if poison and fill != 0x00:
            for name, rows in poison.items():
                a.poison(name, rows)
        a.snapshot()
        fn(a)
        a.assert_guards_untouched()
        a.assert_inputs_untouched()
        runs.append(a.outputs())
    return runs


def assert_isolated(runs: Sequence[Dict[str, torch.Tensor]], fills: Sequence[int] = FILLS, rows: Optional[Dict[str, slice]] = None,
                    atomic: Sequence[str] = (), what: str = "") -> None:
    """every output finite; the outputs of the later runs have the BITS of the first one.  `rows`: compare only these rows of an output
    (cross-row form).  `atomic`: outputs that a floating-point atomic add produces, held to 1e-5 * max|out| instead (the caller says
    which source line justifies it)."""
    for fill, r in zip(fills, runs):
        for name, t in r.items():
            sl = rows.get(name, slice(None)) if rows else slice(None)
            got, ref = t[sl], runs[0][name][sl]
            assert bool(torch.isfinite(got.float()).all()), f"{what} fill 0x{fill:02X}: output '{name}' is not finite"
            if name in atomic:
                d = float((got.double() - ref.double()).abs().max())
                assert d <= 1e-5 * float(ref.double().abs().max()), f"{what} fill 0x{fill:02X}: '{name}' moved by {d:.3e}"
            elif not same_bits(got, ref):
                ne = bits(got) != bits(ref)
                first = torch.nonzero(ne)[0].tolist()
                raise AssertionError(f"{what} fill 0x{fill:02X}: output '{name}' differs from the clean run in {int(ne.sum())} of {ne.numel()} "
                                     f"elements, first at {first}: {float(got[tuple(first)])} vs {float(ref[tuple(first)])}")


# ---- the plan: workspace and gradient arena (GPU; `net` is a sdxl_amd.unet.NativeUNet) -----------------------------------------------------
def fill_bytes(t: torch.Tensor, byte: int) -> None:
    """every byte of a device tensor, between whole calls only: no launch is in flight while the fill runs"""
    torch.cuda.synchronize()
    t.view(-1).view(torch.uint8).fill_(byte)
    torch.cuda.synchronize()


def param_mask(net) -> torch.Tensor:
    """the elements of the gradient arena that belong to a parameter (the alignment gaps between tensors belong to nobody)"""
    m = torch.zeros(net.param_elems, dtype=torch.bool, device=net.grads.device)
    for off, n in net.param_ranges().values():
        m[off: off + n] = True
    return m


def plan_step_on_filled_memory(net, shape, micros, fill: int, mask: torch.Tensor):
    """One accumulation cycle on a workspace and a gradient arena that hold `fill` in every byte: plan, fill both, then per micro-step
    forward_loss (micros[i]() enqueues it), zero_grads before the first backward, backward(1 / len(micros), first_micro = (i == 0)); the
    workspace is filled AGAIN between micro-steps (the gradients live in the arena, not there).  Returns ([loss per micro-step], the
    gradient arena over the parameter ranges).  sdxlstep.h: the workspace is caller memory, first_micro overwrites the weight-matrix
    gradients without reading them."""
    net.plan(*shape)
    fill_bytes(net.workspace, fill)
    fill_bytes(net.grads, fill)
    losses = []
    for i, fwd in enumerate(micros):
        if i:
            fill_bytes(net.workspace, fill)
        fwd()
        if i == 0:
            net.zero_grads()
        net.backward(1.0 / len(micros), i == 0)
        losses.append(net.read_loss()[0])
    torch.cuda.synchronize()
    return losses, net.grads[mask].clone()


def assert_step_isolated(net, shape, micros, fills: Sequence[int] = FILLS, what: str = "") -> None:
    """the losses and the parameter gradients of the pattern-filled runs are finite and have the bits of the clean run's; the workspace
    and the arena are zero-filled afterwards, also after a failed assertion, so that a failure here does not spread over the tests that
    follow -- but not after a failed HIP call, after which nothing more is started on the GPU"""
    import math
    mask = param_mask(net)
    hip_failed = False
    try:
        clean = None
        for fill in fills:
            losses, g = plan_step_on_filled_memory(net, shape, micros, fill, mask)
            assert all(math.isfinite(l) for l in losses), f"{what} fill 0x{fill:02X}: loss {losses}"
            assert bool(torch.isfinite(g).all()), f"{what} fill 0x{fill:02X}: {int((~torch.isfinite(g)).sum())} non-finite parameter gradients"
            if clean is None:
                clean = (losses, g)
                continue
            assert losses == clean[0], f"{what} fill 0x{fill:02X}: loss {losses} vs {clean[0]} on a clean workspace"
            if not same_bits(g, clean[1]):
                ne = bits(g) != bits(clean[1])
                first = int(torch.nonzero(ne)[0])
                arena_index = int(torch.nonzero(mask)[first])
                name = next((k for k, (off, n) in net.param_ranges().items() if off <= arena_index < off + n), "?")
                raise AssertionError(f"{what} fill 0x{fill:02X}: {int(ne.sum())} of {ne.numel()} parameter gradients differ from the clean run, "
                                     f"first at arena element {arena_index} ({name}): {float(g[first])} vs {float(clean[1][first])}")
    except RuntimeError:      # a failed HIP call (lib.SdxlError from lib.check, or torch's own error at a synchronize): no further GPU work
        hip_failed = True
        raise
    finally:
        if not hip_failed:
            if net.workspace is not None:
                fill_bytes(net.workspace, 0)
            fill_bytes(net.grads, 0)
