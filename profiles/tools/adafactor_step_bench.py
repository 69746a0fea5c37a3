#!/usr/bin/env python3
"""What one Adafactor update (algorithm 3 of sdxl_adamw_bf16_step: stats, reduce, usq, scalars, apply) costs next to one AdamW_BF16 update,
on the table of the full SDXL UNet.

Caller buffers of the UNet's 2.57 B-parameter arena (the state-dict shapes of oracle/unet_ref.py laid out as the engine does: every tensor
on a 64-element boundary, 3 x 3 convolutions as [cout][9][cin padded to 8]; 1 680 tensors), fp32 gradients, no EMA.  The updates run
ALTERNATELY in this one process (boxes differ by a few per cent in the clock they hold: numbers of different runs do not compare):
2 warm-up rounds, then `runs` rounds of (one AdamW_BF16 step, one Adafactor step of each recipe), each between two device events.
Reported per update: the median of the timed steps in ms, the bytes per element the design moves and the TB/s that makes, the ratio of
that rate to AdamW_BF16's in the same run, the time of each launch (the profiler's kernel durations over 3 more steps) and the state memory.

  sdxl recipe (scale_parameter false, relative_step false, lr 4e-7, no beta1): g is read three times (stats, usq, apply: 12 B), p and c are
      read and written once (8 B) = 20 B per element
  defaults (scale_parameter, relative_step): stats also reads p and c for the parameter's RMS = 24 B per element

    python profiles/tools/adafactor_step_bench.py [--runs 7] [--out profiles/adafactor_step_timing.txt]
"""
import argparse
import ctypes as C
import statistics
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))
import sdxl_amd  # noqa: E402,F401
from oracle import unet_ref as U  # noqa: E402
from sdxl_amd import lib  # noqa: E402
import importlib  # noqa: E402

O = importlib.import_module("sdxl-training-improvements_amd.optimizer")

BYTES = {"adamw_bf16": 20, "adafactor_sdxl": 20, "adafactor_defaults": 24}      # per element by design, fp32 gradients, no EMA
LAUNCHES = ("adafactor_stats", "adafactor_reduce", "adafactor_usq", "adafactor_scalars", "adafactor_apply")


def sdxl_table():
    shapes = {k: tuple(int(x) for x in v) for k, v in U.param_shapes().items()}
    ranges, cur = {}, 0
    for k, s in shapes.items():
        n = int(np.prod(s))
        if len(s) == 4 and s[2] == 3:
            n = s[0] * 9 * ((s[1] + 7) // 8 * 8)
        ranges[k] = (cur, n)
        cur = (cur + n + 63) // 64 * 64
    return O.adafactor_layout(shapes, ranges), cur


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)      # ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "adafactor_step_timing.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("adafactor_step_bench: needs the GPU (a CPU run measures nothing)")
    dev = torch.device("cuda", 0)
    L = lib.load()
    ents, n = sdxl_table()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    params = sum(e.numel for e in ents)
    say(f"adafactor_step_bench: the SDXL UNet's table, {len(ents)} tensors ({sum(e.factored for e in ents)} factored), {params} parameters in an arena "
        f"of {n} elements, fp32 gradients, no EMA, {torch.cuda.get_device_name(0)}")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    ptr = lambda t: C.c_void_p(t.data_ptr())
    z = lambda dt: torch.zeros(n, dtype=dt, device=dev)
    g = torch.empty(n, dtype=torch.float32, device=dev).normal_(0.0, 1e-3)
    p0 = torch.empty(n, dtype=torch.float32, device=dev).normal_(0.0, 0.05).to(torch.bfloat16)
    a = dict(p=p0.clone(), m=z(torch.bfloat16), v=z(torch.bfloat16), shift=z(torch.bfloat16))
    f = dict(p=p0, c=z(torch.bfloat16))
    offs, cur = [], 0
    for e in ents:
        offs.append(cur)
        cur += e.state_floats()
    state = torch.zeros(cur, dtype=torch.float32, device=dev)
    scratch = torch.empty(O.adafactor_scratch_floats(ents), dtype=torch.float32, device=dev)
    tab = (lib.AdafactorTensor * len(ents))()
    for t, e, so in zip(tab, ents, offs):
        t.elem_off, t.rows, t.cols, t.numel, t.factored, t.state_off = e.elem_off, e.rows, e.cols, e.numel, int(e.factored), so
    aw = lib.AdamWConfig()
    lib.check(L.sdxl_adamw_default_config(C.byref(aw)))

    def af_config(scale_parameter, rho, beta2t):
        c = lib.AdamWConfig()
        lib.check(L.sdxl_adamw_default_config(C.byref(c)))
        c.algorithm, c.weight_decay, c.clip_threshold, c.eps1, c.eps2, c.beta2t, c.rho = 3, 0.0, 1.0, 1e-30, 1e-3, beta2t, rho
        c.scale_parameter, c.use_beta1 = int(scale_parameter), 0
        c.tensors, c.n_tensors, c.af_state, c.af_scratch = C.addressof(tab), len(ents), state.data_ptr(), scratch.data_ptr()
        return c

    cfgs = {"adafactor_sdxl": af_config(False, 4e-7, 1.0 - 10.0 ** -0.8), "adafactor_defaults": af_config(True, 1e-2, 1.0 - 10.0 ** -0.8)}
    af = lambda c: lib.check(L.sdxl_adamw_bf16_step(ptr(f["p"]), ptr(g), 0, None, None, ptr(f["c"]), n, C.byref(c), None, None, st))
    run = {"adamw_bf16": lambda: lib.check(L.sdxl_adamw_bf16_step(ptr(a["p"]), ptr(g), 0, ptr(a["m"]), ptr(a["v"]), ptr(a["shift"]), n, C.byref(aw),
                                                                  None, None, st)),
           "adafactor_sdxl": lambda: af(cfgs["adafactor_sdxl"]), "adafactor_defaults": lambda: af(cfgs["adafactor_defaults"])}
    times = {k: [] for k in run}
    for it in range(2 + args.runs):
        for k, fn in run.items():
            t = timed(fn)
            if it >= 2:
                times[k].append(t)
    say(f"one update, ms: median of {args.runs} timed steps after 2 warm-up rounds, the updates alternating (min .. max)")
    tb = {}
    for k, t in times.items():
        med = statistics.median(t)
        tb[k] = BYTES[k] * n / (med * 1e-3) / 1e12
        say(f"  {k:19s} {med:8.3f}  ({min(t):.3f} .. {max(t):.3f})   {BYTES[k]} B/element by design -> {tb[k]:.2f} TB/s")
    for k in ("adafactor_sdxl", "adafactor_defaults"):
        say(f"  {k}'s TB/s is {tb[k] / tb['adamw_bf16']:.2f} of adamw_bf16's in this run; its time is {statistics.median(times[k]) / statistics.median(times['adamw_bf16']):.2f} x")
    # each launch: the profiler's kernel durations over 3 more steps of each recipe
    for k in ("adafactor_sdxl", "adafactor_defaults"):
        try:
            from torch.profiler import ProfilerActivity, profile
            with profile(activities=[ProfilerActivity.CUDA]) as prof:
                for _ in range(3):
                    run[k]()
                torch.cuda.synchronize()
            per = {name: [] for name in LAUNCHES}
            for ev in prof.events():
                for name in LAUNCHES:
                    if name in ev.name:
                        per[name].append(getattr(ev, "device_time", None) or getattr(ev, "cuda_time", 0.0))
            if not any(per.values()):
                raise RuntimeError("the profiler recorded no kernel of the update")
            say(f"  {k}, each launch, ms (mean of {max(len(v) for v in per.values())}): "
                + "  ".join(f"{name[len('adafactor_'):]} {statistics.mean(v) / 1e3:.3f}" for name, v in per.items() if v))
        except Exception as exc:      # noqa: BLE001  (a box without the tracer: the totals above stand)
            say(f"  {k}, each launch: not measured ({type(exc).__name__}: {exc})")
    state_b, comp_b = 4 * state.numel(), 2 * n
    say(f"state memory: Adafactor statistics {state_b / 2**20:.1f} MiB + bf16 compensation {comp_b / 2**30:.2f} GiB = {(state_b + comp_b) / n:.3f} B/element "
        f"(+ scratch {4 * scratch.numel() / 2**20:.1f} MiB, + 4 B/element with beta1), against AdamW_BF16's 6 B/element ({6 * n / 2**30:.2f} GiB)")
    torch.cuda.synchronize()
    assert bool(torch.isfinite(f["p"][:4096].float()).all()) and bool(torch.isfinite(state).all()) and bool(torch.isfinite(scratch[: 4 * len(ents)]).all())
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
