#!/usr/bin/env python3
"""What the LoRA trainer's `training.lora_backward` modes cost per cycle, and the direct adapter-gradient kernels next to the weight-gradient
GEMMs they replace.

Full SDXL-base UNet with synthetic weights, B = 4 at 1024^2 (latent 128 x 128), ddpm, default targets, rank 16 and rank 64.  One cycle =
forward + backward + optimizer_step() of lora.NativeLoRATrainer, between two device events.  The three modes run ALTERNATELY in this one
process (boxes differ by a few per cent in the clock they hold: numbers of different runs do not compare): 3 warm-up cycles per mode, then
rounds of (mode switch, one untimed cycle, `per_round` timed cycles) until every mode has `cycles` timed ones.  "project" is the parent's
behaviour and the yardstick.  Then, per distinct target shape, the three launches of csrc/lora_grad.hip through sdxl_op_lora_grad beside the
TN weight-gradient GEMM of the same layer through sdxl_op_gemm (its best deterministic split-K of 1, 2, 4, 8).

    python profiles/tools/lora_step_bench.py [--ranks 16,64] [--cycles 20] [--per-round 5] [--out profiles/lora_step_timing.txt]
"""
import argparse
import ctypes as C
import importlib
import statistics
import sys
from pathlib import Path
from types import SimpleNamespace

import torch

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))
import sdxl_amd  # noqa: E402,F401
from sdxl_amd import lib, synth  # noqa: E402
from sdxl_amd import unet as NU  # noqa: E402

CFG = importlib.import_module("sdxl-training-improvements_amd.config")
T = importlib.import_module("sdxl-training-improvements_amd.trainer")
LORA = importlib.import_module("sdxl-training-improvements_amd.lora")
MODES = LORA.LORA_BACKWARDS
B, H, W = 4, 128, 128


def karras_table(n=1000, smin=0.002, smax=20000.0, rho=7.0):
    ramp = torch.linspace(0, 1, n)
    return (smax ** (1 / rho) + ramp * (smin ** (1 / rho) - smax ** (1 / rho))) ** rho


def make_batch(dev):
    g = torch.Generator().manual_seed(1234)
    r = lambda *s: torch.randn(*s, generator=g)
    ts = (torch.rand(B, generator=g) * 1000).long()
    b = dict(lat=r(B, 4, H, W), noise=r(B, 4, H, W), sig=karras_table()[ts], t=ts.float(), ehs=r(B, 77, 2048).to(torch.bfloat16), pooled=r(B, 1280).to(torch.bfloat16),
             tid=torch.tensor([[8.0 * W, 8.0 * H, 0, 0, 8.0 * W, 8.0 * H]] * B))
    return {k: v.to(dev) for k, v in b.items()}


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)      # ms


def step_modes(net, batch, rank, cycles, per_round, say):
    trainers = {}
    for mode in MODES:      # all built before the first step: each takes its W0 copy from the checkpoint's weights
        cfg = CFG.Config()
        cfg.training.method = "ddpm"
        cfg.training.lora_rank = rank
        cfg.training.lora_backward = "project"      # the selection is applied at each switch below
        trainers[mode] = T.create_trainer(SimpleNamespace(unet=net), config=cfg)
        trainers[mode].lora_backward = mode
        g = torch.Generator().manual_seed(5)        # B != 0: the merge and the gradients do real work
        for k in trainers[mode].lora.targets:
            trainers[mode].lora.B(k).copy_((torch.randn(trainers[mode].lora.B(k).shape, generator=g) * 0.01).to(torch.bfloat16))

    def switch(mode):
        tr = trainers[mode]
        tr.lora.merge()
        if mode == "project":
            net.set_trainable(None)
        else:
            tr.lora.select(mode)
        return tr

    def cycle(tr):
        net.forward_loss("ddpm", batch["lat"], batch["noise"], batch["sig"], batch["t"], batch["ehs"], batch["pooled"], batch["tid"])
        tr._native_backward(1.0)
        tr.optimizer_step()

    times = {m: [] for m in MODES}
    rounds = {m: [] for m in MODES}
    for mode in MODES:
        tr = switch(mode)
        for _ in range(3):
            cycle(tr)
        torch.cuda.synchronize()
    while len(times[MODES[0]]) < cycles:
        for mode in MODES:
            tr = switch(mode)
            cycle(tr)
            torch.cuda.synchronize()
            ts = [timed(lambda: cycle(tr)) for _ in range(per_round)]
            times[mode] += ts
            rounds[mode].append(statistics.median(ts))
    net.set_trainable(None)
    base = statistics.median(times["project"])
    say(f"rank {rank}: one cycle (forward + backward + optimizer_step), ms; {len(times['project'])} timed cycles per mode in rounds of {per_round}, modes alternating")
    for mode in MODES:
        t = times[mode]
        say(f"  {mode:15s} median {statistics.median(t):8.3f}  min {min(t):8.3f}  max {max(t):8.3f}  vs project {statistics.median(t) - base:+7.3f} ms"
            f"   round medians {' '.join(f'{x:.2f}' for x in rounds[mode])}")
    spread = max(rounds["project"]) - min(rounds["project"])
    say(f"  spread of the project rounds' medians: {spread:.3f} ms (a gain smaller than this is not a gain)")
    for tr in trainers.values():
        tr.lora.restore()
    torch.cuda.synchronize()


def bench(fn, iters=20):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    return timed(lambda: [fn() for _ in range(iters)]) / iters * 1e3      # us


def kernels(dev, ranks, say):
    L = lib.load()
    st = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t: C.c_void_p(t.data_ptr())
    r = lambda *s: (torch.randn(*s, device=dev)).to(torch.bfloat16)
    say("direct adapter gradients (three launches, sdxl_op_lora_grad) beside the weight-gradient GEMM of the same layer (sdxl_op_gemm form 2), us, alone on the chip")
    for M, out, inn, what in ((16384, 640, 640, "level 1 attention projections"), (4096, 1280, 1280, "level 2 attention projections"),
                              (308, 640, 2048, "level 1 attn2.to_k / to_v"), (308, 1280, 2048, "level 2 attn2.to_k / to_v")):
        X, dY, dW = r(M, inn), r(M, out), torch.zeros(out, inn, device=dev)
        wg = min(bench(lambda: lib.check(L.sdxl_op_gemm(2, p(dY), p(X), p(dW), out, inn, M, None, None, 0, sk, st()))) for sk in (1, 2, 4, 8))
        line = f"  M {M:6d} out {out:5d} in {inn:5d} ({what}): weight gradient {wg:8.1f}"
        for rank in ranks:
            A, Bm = r(rank, inn), r(out, rank)
            dA, dB = torch.zeros(rank, inn, device=dev), torch.zeros(out, rank, device=dev)
            t = bench(lambda: lib.check(L.sdxl_op_lora_grad(p(X), inn, p(dY), out, p(A), p(Bm), p(dA), p(dB), M, out, inn, rank, 1.0, 0, st())))
            line += f"   direct r{rank} {t:8.1f}"
        say(line)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ranks", default="16,64")
    ap.add_argument("--cycles", type=int, default=20)
    ap.add_argument("--per-round", type=int, default=5)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "lora_step_timing.txt"))
    args = ap.parse_args()
    ranks = [int(x) for x in args.ranks.split(",")]
    if not torch.cuda.is_available():
        sys.exit("lora_step_bench: needs the GPU (a CPU run measures nothing)")
    dev = torch.device("cuda", 0)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"lora_step_bench: SDXL-base, B = {B} at {8 * H} x {8 * W}, ddpm, default targets, {torch.cuda.get_device_name(0)}")
    net = NU.NativeUNet(NU.make_config(), device=0)
    synth.load_synthetic(net, seed=0)
    net.plan(B, H, W, 77)
    batch = make_batch(dev)
    for rank in ranks:
        step_modes(net, batch, rank, args.cycles, args.per_round, say)
    net.close()
    kernels(dev, ranks, say)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
