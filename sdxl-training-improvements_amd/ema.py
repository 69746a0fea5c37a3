"""fp32 exponential moving average of the packed bf16 UNet weights (diffusers' `EMAModel`, the SDXL script's `--use_ema`).

The average lives in one fp32 arena laid out like the weight arena (element i averages weight i) and is updated inside the fused
optimizer kernel, right after each element's new bf16 weight is final (csrc/optimizer.hip, `ema_update8`): the optimizers of
optimizer.py pass `arena + offset` and `advance()`'s float32(1 - decay) with every launch, so whatever steps them updates the EMA too.

The rule is `EMAModel.get_decay` / `EMAModel.step`, with t = optimizer steps so far counting this one (1-based):

    k = max(0, t - update_after_step - 1)
    decay = 0 if k == 0 else clamp((1 + k) / (10 + k)  or, with use_ema_warmup,  1 - (1 + k / inv_gamma) ** -power,
                                   min_decay, decay)
    e <- e - float32(1 - decay) * (e - float(p))        three separately rounded fp32 ops

and `e` starts as the exact fp32 image of the bf16 weights when the EMA is built.  It tracks the bf16 parameter itself, not
p + shift (AdamWBF16) or p + kahan_comp (schedule-free).

The arena has the gradient arena's layout, so the library's own layout inverse (`sdxl_export_grad`) reads it out in diffusers keys:
a second handle of the library, bound to (weights, EMA arena), leaves the training handle's bindings untouched.  Reading a
diffusers-keyed EMA back (resume) scatters each tensor through the index map that handle gives for a per-tensor iota (every tensor
has fewer than 2^24 elements, so fp32 holds its indices exactly)."""
from __future__ import annotations

import ctypes as C
from typing import Any, Dict

import numpy as np
import torch

from . import lib


def _aligned_f32(n: int, device) -> torch.Tensor:
    """n fp32 elements whose first element is 256-byte aligned (what sdxl_bind_params requires of an arena)"""
    buf = torch.empty(n + 64, dtype=torch.float32, device=device)
    off = (-buf.data_ptr() % 256) // 4
    return buf[off:off + n]


class WeightEMA:
    """The EMA arena, its step count and its settings (the config keys training.ema_*; see the module docstring)."""

    SETTINGS = ("decay", "min_decay", "update_after_step", "use_ema_warmup", "inv_gamma", "power")

    def __init__(self, net, *, decay: float = 0.9999, min_decay: float = 0.0, update_after_step: int = 0,
                 use_ema_warmup: bool = False, inv_gamma: float = 1.0, power: float = 2 / 3):
        if not 0.0 <= float(min_decay) <= float(decay) <= 1.0:
            raise ValueError(f"EMA decays must satisfy 0 <= ema_min_decay <= ema_decay <= 1, got {min_decay}, {decay}")
        if int(update_after_step) < 0:
            raise ValueError(f"ema_update_after_step must be >= 0, got {update_after_step}")
        if float(inv_gamma) <= 0.0 or float(power) <= 0.0:
            raise ValueError(f"ema_inv_gamma and ema_power must be > 0, got {inv_gamma}, {power}")
        self.net = net
        self.decay_max, self.min_decay = float(decay), float(min_decay)
        self.update_after_step = int(update_after_step)
        self.use_ema_warmup = bool(use_ema_warmup)
        self.inv_gamma, self.power = float(inv_gamma), float(power)
        w = net.weights
        self.param_elems = int(w.numel())
        self.arena = _aligned_f32(self.param_elems, w.device)
        self.arena.copy_(w)                                   # the exact fp32 image of the bf16 weights
        self.optimization_step = 0
        self._h = None                                        # export handle bound to (weights, arena), made on first use

    # ------------------------------------------------------------------ the rule
    def settings(self) -> Dict[str, Any]:
        return {"decay": self.decay_max, "min_decay": self.min_decay, "update_after_step": self.update_after_step,
                "use_ema_warmup": self.use_ema_warmup, "inv_gamma": self.inv_gamma, "power": self.power}

    def decay(self, t: int) -> float:
        """EMAModel.get_decay(t): the decay of the update after the t-th optimizer step (1-based)"""
        k = max(0, int(t) - self.update_after_step - 1)
        if k <= 0:
            return 0.0
        if self.use_ema_warmup:
            d = 1 - (1 + k / self.inv_gamma) ** -self.power
        else:
            d = (1 + k) / (10 + k)
        return max(min(d, self.decay_max), self.min_decay)

    def advance(self) -> float:
        """count one optimizer step and return the kernel's omd = float32(1 - decay(t)) for it (the optimizers call this once per
        step, before their launches)"""
        self.optimization_step += 1
        return float(np.float32(1.0 - self.decay(self.optimization_step)))

    # ------------------------------------------------------------------ state
    def state_dict(self) -> Dict[str, Any]:
        """settings, step and arena size (JSON-serialisable: ema.json); the arena itself is saved as diffusers-keyed fp32"""
        return {**self.settings(), "optimization_step": self.optimization_step, "param_elems": self.param_elems}

    def check_state_dict(self, sd: Dict[str, Any]) -> None:
        """ValueError unless `sd` (a state_dict()) fits this EMA: the same settings and arena size, a valid step; changes nothing"""
        got = {k: sd.get(k) for k in self.SETTINGS}
        if got != self.settings():
            raise ValueError(f"EMA state with settings {got} cannot be loaded into an EMA configured as {self.settings()}")
        if sd.get("param_elems") != self.param_elems:
            raise ValueError(f"EMA state of {sd.get('param_elems')} elements cannot be loaded into an arena of {self.param_elems}")
        step = sd.get("optimization_step")
        if not isinstance(step, int) or isinstance(step, bool) or step < 0:
            raise ValueError(f"EMA state has an invalid optimization_step {step!r}")

    def load_state_dict(self, sd: Dict[str, Any]) -> None:
        self.check_state_dict(sd)
        self.optimization_step = sd["optimization_step"]

    # ------------------------------------------------------------------ diffusers layout <-> arena
    def _handle(self):
        if self._h is None:
            L = self.net.L
            h = C.c_void_p()
            lib.check(L.sdxl_create(C.byref(self.net.cfg), self.net.device.index or 0, C.byref(h)), "sdxl_create (EMA export)")
            self._h = h
            lib.check(L.sdxl_bind_params(h, C.c_void_p(self.net.weights.data_ptr()), C.c_void_p(self.arena.data_ptr())),
                      "sdxl_bind_params (EMA export)")
        return self._h

    def _export(self, name: str) -> torch.Tensor:
        out = torch.empty(self.net.param_table[name], dtype=torch.float32, device=self.arena.device)
        lib.check(self.net.L.sdxl_export_grad(self._handle(), name.encode(), C.c_void_p(out.data_ptr()), 0,
                                              C.c_void_p(torch.cuda.current_stream().cuda_stream)), f"export EMA {name}")
        return out

    def state_tensors(self) -> Dict[str, torch.Tensor]:
        """the EMA in diffusers keys and shapes, fp32, on the device"""
        return {k: self._export(k) for k in self.net.param_table}

    @torch.no_grad()
    def load_tensors(self, sd: Dict[str, torch.Tensor]) -> None:
        """inverse of state_tensors, bit for bit: each tensor is scattered through the packed index map of its range (a per-tensor
        iota exported through the same layout inverse).  Arena elements outside every tensor (conv channel padding, alignment gaps)
        take the fp32 image of the weights, as at construction: that is their EMA as long as those weights stay what they were
        allocated as (zero), which they do in training -- no backward writes their gradients, which stay zero."""
        ranges = self.net.param_ranges()
        missing = [k for k in ranges if k not in sd]
        extra = [k for k in sd if k not in ranges]
        if missing or extra:
            raise KeyError(f"EMA state_dict mismatch: missing {missing[:5]} extra {extra[:5]}")
        for name, (off, cnt) in ranges.items():           # every check before the arena changes
            if tuple(sd[name].shape) != self.net.param_table[name]:
                raise ValueError(f"EMA {name}: shape {tuple(sd[name].shape)} != {self.net.param_table[name]}")
            if cnt >= 1 << 24:
                raise ValueError(f"EMA {name}: {cnt} packed elements, more than fp32 indices hold exactly")
        self.arena.copy_(self.net.weights)
        for name, (off, cnt) in ranges.items():
            t = sd[name]
            seg = self.arena[off:off + cnt]
            keep = seg.clone()
            seg.copy_(torch.arange(cnt, dtype=torch.float32, device=seg.device))
            idx = self._export(name).reshape(-1).long()       # diffusers element j lives at seg[idx[j]]
            seg.copy_(keep)
            seg[idx] = t.reshape(-1).to(device=seg.device, dtype=torch.float32)
        torch.cuda.current_stream().synchronize()

    def close(self) -> None:
        if self._h is not None:
            torch.cuda.synchronize()
            self.net.L.sdxl_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
