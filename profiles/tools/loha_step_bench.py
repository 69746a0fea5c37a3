#!/usr/bin/env python3
"""What LoHa adapters (training.lora_algo "loha", csrc/loha.hip) cost per cycle next to LoRA's, both by merge and project.

Full SDXL-base UNet with synthetic weights, B = 4 at 1024^2 (latent 128 x 128), ddpm, default targets, lora_backward "project", ranks 4 and
16.  One cycle = forward + backward + optimizer_step() of lora.NativeLoRATrainer (projection, fused optimizer on the adapter arena, merge),
between two device events.  The (algo, rank) configurations run ALTERNATELY in this one process (boxes differ by a few per cent in the clock
they hold: numbers of different runs do not compare): 3 warm-up cycles each, then rounds of (switch, one untimed cycle, `per_round` timed
cycles) until each has `cycles` timed ones.  Then the merge call and the projection call of each configuration alone, between events.

    python profiles/tools/loha_step_bench.py [--ranks 4,16] [--cycles 20] [--per-round 5] [--out profiles/loha_step_timing.txt]
"""
import argparse
import importlib
import statistics
import sys
from pathlib import Path
from types import SimpleNamespace

import torch

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))
import sdxl_amd  # noqa: E402,F401
from sdxl_amd import synth  # noqa: E402
from sdxl_amd import unet as NU  # noqa: E402

CFG = importlib.import_module("sdxl-training-improvements_amd.config")
T = importlib.import_module("sdxl-training-improvements_amd.trainer")
LORA = importlib.import_module("sdxl-training-improvements_amd.lora")
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


def build(net, algo, rank):
    cfg = CFG.Config()
    cfg.training.method = "ddpm"
    cfg.training.lora_rank = rank
    cfg.training.lora_algo = algo
    tr = T.create_trainer(SimpleNamespace(unet=net), config=cfg)
    g = torch.Generator().manual_seed(5)        # a non-zero delta: the merge and the gradients do real work
    for k in tr.lora.targets:
        up = tr.lora.B2(k) if algo == "loha" else tr.lora.B(k)
        up.copy_((torch.randn(up.shape, generator=g) * 0.01).to(torch.bfloat16))
    return tr


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ranks", default="4,16")
    ap.add_argument("--cycles", type=int, default=20)
    ap.add_argument("--per-round", type=int, default=5)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "loha_step_timing.txt"))
    args = ap.parse_args()
    ranks = [int(x) for x in args.ranks.split(",")]
    if not torch.cuda.is_available():
        sys.exit("loha_step_bench: needs the GPU (a CPU run measures nothing)")
    dev = torch.device("cuda", 0)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"loha_step_bench: SDXL-base, B = {B} at {8 * H} x {8 * W}, ddpm, default targets, lora_backward project, {torch.cuda.get_device_name(0)}")
    net = NU.NativeUNet(NU.make_config(), device=0)
    synth.load_synthetic(net, seed=0)
    net.plan(B, H, W, 77)
    batch = make_batch(dev)
    configs = [(algo, rank) for rank in ranks for algo in ("lora", "loha")]
    trainers = {c: build(net, *c) for c in configs}      # all built before the first step: each takes its W0 copy from the checkpoint's weights

    def cycle(tr):
        net.forward_loss("ddpm", batch["lat"], batch["noise"], batch["sig"], batch["t"], batch["ehs"], batch["pooled"], batch["tid"])
        tr._native_backward(1.0)
        tr.optimizer_step()

    times = {c: [] for c in configs}
    rounds = {c: [] for c in configs}
    for c in configs:
        trainers[c].lora.merge()
        for _ in range(3):
            cycle(trainers[c])
        torch.cuda.synchronize()
    while len(times[configs[0]]) < args.cycles:
        for c in configs:
            tr = trainers[c]
            tr.lora.merge()
            cycle(tr)
            torch.cuda.synchronize()
            ts = [timed(lambda: cycle(tr)) for _ in range(args.per_round)]
            times[c] += ts
            rounds[c].append(statistics.median(ts))
    say(f"one cycle (forward + backward + optimizer_step), ms; {len(times[configs[0]])} timed cycles per configuration in rounds of {args.per_round}, "
        "configurations alternating")
    for algo, rank in configs:
        t = times[(algo, rank)]
        base = statistics.median(times[("lora", rank)])
        say(f"  {algo} r{rank:<3d} median {statistics.median(t):8.3f}  min {min(t):8.3f}  max {max(t):8.3f}  vs lora r{rank} {statistics.median(t) - base:+7.3f} ms"
            f"   round medians {' '.join(f'{x:.2f}' for x in rounds[(algo, rank)])}")
    for rank in ranks:
        r = rounds[("lora", rank)]
        say(f"  spread of the lora r{rank} rounds' medians: {max(r) - min(r):.3f} ms (a difference smaller than this is not a difference)")
    say(f"the merge call and the projection call alone, ms, median of {args.cycles} (min .. max), {len(trainers[configs[0]].lora.targets)} targets")
    net.grads.copy_(torch.randn(net.param_elems, generator=torch.Generator().manual_seed(3)).to(dev))
    for c in configs:
        ad = trainers[c].lora
        for name, fn in (("merge", ad.merge), ("project", ad.project)):
            for _ in range(3):
                fn()
            torch.cuda.synchronize()
            t = [timed(fn) for _ in range(args.cycles)]
            say(f"  {c[0]} r{c[1]:<3d} {name:8s} {statistics.median(t):8.3f}  ({min(t):.3f} .. {max(t):.3f})")
    for tr in trainers.values():
        tr.lora.restore()
    torch.cuda.synchronize()
    net.close()
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
