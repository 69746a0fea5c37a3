#!/usr/bin/env python3
"""What DoRA adapters (training.lora_algo "dora", csrc/dora.hip) cost per cycle next to LoRA's, both by merge and project.

Full SDXL-base UNet with synthetic weights, B = 4 at 1024^2 (latent 128 x 128), ddpm, lora_target_kinds "all" on every layer that can carry
an adapter (TARGETS, the list of lokr_step_bench.py), lora_backward "project", rank 16.  One cycle = forward + backward + optimizer_step() of
lora.NativeLoRATrainer (projection, fused optimizer on the adapter arena, merge), between two device events.  The two configurations run
ALTERNATELY in this one process (boxes differ by a few per cent in the clock they hold: numbers of different runs do not compare): 3 warm-up
cycles each, then rounds of (switch, one untimed cycle, `per_round` timed cycles) until each has `cycles` timed ones.  Then DoRA's init call
and the merge and projection calls of each configuration alone, between events.  The expectation the projection is reported against: LoRA's
plus one more read of dW (fp32) and of W0 (bf16), at the rate LoRA's own projection reads dW in this run.

The default bench.py headline on this commit and on its parent (bench.py --lib with the parent's build on the same box, two runs each) is
measured apart: `--headline "..."` lines are copied into the output behind the prefix "entered by hand: ", which marks what this tool
did not measure and cannot reproduce.

    python profiles/tools/dora_step_bench.py [--cycles 20] [--per-round 5] [--out profiles/dora_step_timing.txt] [--headline TEXT ...]
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
TARGETS = list(LORA.DEFAULT_TARGETS) + ["ff.net.0.proj", "ff.net.2", "proj_in", "proj_out", "conv1", "conv2", "conv_shortcut",
                                        "downsamplers.0.conv", "upsamplers.0.conv", "conv_out"]
CONFIGS = [("lora r16", dict(lora_algo="lora", lora_rank=16)), ("dora r16", dict(lora_algo="dora", lora_rank=16))]


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


def build(net, keys):
    cfg = CFG.Config()
    cfg.training.method = "ddpm"
    cfg.training.lora_target_kinds = "all"
    cfg.training.lora_targets = TARGETS
    for k, v in keys.items():
        setattr(cfg.training, k, v)
    tr = T.create_trainer(SimpleNamespace(unet=net), config=cfg)
    ad = tr.lora
    g = torch.Generator().manual_seed(5)        # a non-zero delta: the merge and the gradients do real work
    for k in ad.targets:
        ad.B(k).copy_((torch.randn(ad.B(k).shape, generator=g) * 0.01).to(torch.bfloat16))
    return tr


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cycles", type=int, default=20)
    ap.add_argument("--per-round", type=int, default=5)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "dora_step_timing.txt"))
    ap.add_argument("--headline", action="append", default=[])
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("dora_step_bench: needs the GPU (a CPU run measures nothing)")
    dev = torch.device("cuda", 0)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"dora_step_bench: SDXL-base, B = {B} at {8 * H} x {8 * W}, ddpm, lora_target_kinds all, lora_backward project, {torch.cuda.get_device_name(0)}")
    net = NU.NativeUNet(NU.make_config(), device=0)
    synth.load_synthetic(net, seed=0)
    net.plan(B, H, W, 77)
    batch = make_batch(dev)
    labels = [c[0] for c in CONFIGS]
    trainers = {label: build(net, keys) for label, keys in CONFIGS}      # all built before the first step: each takes its W0 copy from the checkpoint's weights
    ranges = net.param_ranges()
    ad0 = trainers[labels[0]].lora
    assert all(tr.lora.targets == ad0.targets for tr in trainers.values())
    elems = sum(ranges[k][1] for k in ad0.targets)
    g_bytes, w0_bytes = 4 * elems, 2 * elems
    say(f"{len(ad0.targets)} targets, {elems / 1e9:.3f} G elements of dW = {g_bytes / 1e9:.2f} GB of fp32 gradients, {w0_bytes / 1e9:.2f} GB of bf16 W0; adapter "
        "elements: " + ", ".join(f"{label} {trainers[label].lora.param_elems / 1e6:.1f} M" for label in labels)
        + f"; norm0 / norm {trainers[labels[1]].lora.norm0.numel() * 4 / 1e6:.2f} MB each")

    def cycle(tr):
        net.forward_loss("ddpm", batch["lat"], batch["noise"], batch["sig"], batch["t"], batch["ehs"], batch["pooled"], batch["tid"])
        tr._native_backward(1.0)
        tr.optimizer_step()

    times = {c: [] for c in labels}
    rounds = {c: [] for c in labels}
    for c in labels:
        trainers[c].lora.merge()
        for _ in range(3):
            cycle(trainers[c])
        torch.cuda.synchronize()
    while len(times[labels[0]]) < args.cycles:
        for c in labels:
            tr = trainers[c]
            tr.lora.merge()
            cycle(tr)
            torch.cuda.synchronize()
            ts = [timed(lambda: cycle(tr)) for _ in range(args.per_round)]
            times[c] += ts
            rounds[c].append(statistics.median(ts))
    say(f"one cycle (forward + backward + optimizer_step), ms; {len(times[labels[0]])} timed cycles per configuration in rounds of {args.per_round}, "
        "configurations alternating")
    base = statistics.median(times[labels[0]])
    for c in labels:
        t = times[c]
        say(f"  {c:13s} median {statistics.median(t):8.3f}  min {min(t):8.3f}  max {max(t):8.3f}  vs {labels[0]} {statistics.median(t) - base:+7.3f} ms"
            f"   round medians {' '.join(f'{x:.2f}' for x in rounds[c])}")
    r = rounds[labels[0]]
    say(f"  spread of the {labels[0]} rounds' medians: {max(r) - min(r):.3f} ms (a difference smaller than this is not a difference)")
    say(f"the init, merge and projection calls alone, ms, median of {args.cycles} (min .. max)")
    net.grads.copy_(torch.randn(net.param_elems, generator=torch.Generator().manual_seed(3)).to(dev))
    med = {}
    for c in labels:
        ad = trainers[c].lora
        calls = (("init", ad.init_norm0),) if ad.algo == "dora" else ()
        for name, fn in calls + (("merge", ad.merge), ("project", ad.project)):
            for _ in range(3):
                fn()
            torch.cuda.synchronize()
            t = [timed(fn) for _ in range(args.cycles)]
            med[c, name] = statistics.median(t)
            rate = f"   {g_bytes / (med[c, name] * 1e-3) / 1e12:.2f} TB/s of dW" if name == "project" else ""
            say(f"  {c:13s} {name:8s} {med[c, name]:8.3f}  ({min(t):.3f} .. {max(t):.3f}){rate}")
    lo, do = med[labels[0], "project"], med[labels[1], "project"]
    expect = lo + lo * (g_bytes + w0_bytes) / g_bytes
    say(f"the projection against its expectation: LoRA's {lo:.3f} ms plus one more read of dW and W0 at LoRA's rate = {expect:.3f} ms; measured {do:.3f} ms "
        f"({do / expect:.2f} of it)")
    for h in args.headline:
        say("entered by hand: " + h)
    for tr in trainers.values():
        tr.lora.restore()
    torch.cuda.synchronize()
    net.close()
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
