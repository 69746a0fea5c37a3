#!/usr/bin/env python3
"""What one Prodigy update (algorithm 2 of sdxl_adamw_bf16_step: accumulate, finalize, apply) costs next to one AdamW_BF16 update.

Caller buffers of 2^28 elements (HBM-bound: about 6 GB with every arena of both), fp32 gradients, no EMA.  The two updates run
ALTERNATELY in this one process (boxes differ by a few per cent in the clock they hold: numbers of different runs do not compare):
2 warm-up rounds, then `runs` rounds of (one AdamW_BF16 step, one Prodigy step), each between two device events.  Reported per update:
the median of the timed steps in ms, the bytes per element the design moves (csrc/optimizer.hip's head comments: 20 B and 50 B) and the
TB/s that makes.  Prodigy's line is three launches; the finalize's serial tail is inside its time.

    python profiles/tools/prodigy_step_bench.py [--log2n 28] [--runs 7] [--out profiles/prodigy_step_timing.txt]
"""
import argparse
import ctypes as C
import math
import statistics
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))
import sdxl_amd  # noqa: E402,F401
from sdxl_amd import lib  # noqa: E402

BYTES = {"adamw_bf16": 20, "prodigy": 50}      # per element by design, fp32 gradients, no EMA


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)      # ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, default=28)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "prodigy_step_timing.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("prodigy_step_bench: needs the GPU (a CPU run measures nothing)")
    dev = torch.device("cuda", 0)
    L = lib.load()
    n = 1 << args.log2n
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"prodigy_step_bench: {n} elements (2^{args.log2n}), fp32 gradients, no EMA, {torch.cuda.get_device_name(0)}")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    ptr = lambda t: C.c_void_p(t.data_ptr())
    z = lambda dt: torch.zeros(n, dtype=dt, device=dev)
    g = torch.full((n,), 1e-3, dtype=torch.float32, device=dev)
    # AdamW_BF16: p, m, v, shift bf16;  Prodigy: p, c, p0 bf16, m, v, s fp32, the state block
    a = dict(p=torch.full((n,), 0.05, dtype=torch.bfloat16, device=dev), m=z(torch.bfloat16), v=z(torch.bfloat16), shift=z(torch.bfloat16))
    p = dict(p=torch.full((n,), 0.05, dtype=torch.bfloat16, device=dev), c=z(torch.bfloat16), m=z(torch.float32), v=z(torch.float32), s=z(torch.float32))
    p["p0"] = p["p"].clone()
    state = torch.zeros(lib.PRODIGY_STATE_FLOATS, dtype=torch.float32, device=dev)
    state[:2] = 1e-6
    aw, pr = lib.AdamWConfig(), lib.AdamWConfig()
    lib.check(L.sdxl_adamw_default_config(C.byref(aw)))
    lib.check(L.sdxl_adamw_default_config(C.byref(pr)))
    pr.algorithm, pr.lr, pr.beta3, pr.d0, pr.d_coef, pr.growth_rate, pr.prodigy_bc = 2, 1.0, math.sqrt(0.999), 1e-6, 1.0, math.inf, 1.0
    pr.p0, pr.s, pr.prodigy_state = p["p0"].data_ptr(), p["s"].data_ptr(), state.data_ptr()
    run = {"adamw_bf16": lambda: lib.check(L.sdxl_adamw_bf16_step(ptr(a["p"]), ptr(g), 0, ptr(a["m"]), ptr(a["v"]), ptr(a["shift"]), n, C.byref(aw),
                                                                  None, None, st)),
           "prodigy": lambda: lib.check(L.sdxl_adamw_bf16_step(ptr(p["p"]), ptr(g), 0, ptr(p["m"]), ptr(p["v"]), ptr(p["c"]), n, C.byref(pr),
                                                               None, None, st))}
    times = {k: [] for k in run}
    for it in range(2 + args.runs):
        for k, fn in run.items():
            t = timed(fn)
            if it >= 2:
                times[k].append(t)
    say(f"one update, ms: median of {args.runs} timed steps after 2 warm-up rounds, the two updates alternating (min .. max)")
    tb = {}
    for k, t in times.items():
        med = statistics.median(t)
        tb[k] = BYTES[k] * n / (med * 1e-3) / 1e12
        say(f"  {k:11s} {med:8.3f}  ({min(t):.3f} .. {max(t):.3f})   {BYTES[k]} B/element by design -> {tb[k]:.2f} TB/s")
    say(f"  prodigy's TB/s is {tb['prodigy'] / tb['adamw_bf16']:.2f} of adamw_bf16's in this run")
    torch.cuda.synchronize()
    assert bool(torch.isfinite(p["p"][:1024].float()).all()) and bool(torch.isfinite(state[:8]).all())
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
