"""Times what the LoRA mode adds and what it removes, on the full SDXL-base handle (no plan, no forward): the merge and the projection of
the default targets (csrc/lora.hip) and the fused update of the adapter arena at ranks 16 and 64, against the full-arena AdamWBF16 update
of the same run.  HIP events, 20 repetitions after 3 warm-up calls, median and minimum.

    python profiles/tools/lora_bench.py [--reps 20] [--out profiles/lora_timing.txt]

The bar (rank 16): merge + project + adapter update <= the full-arena AdamW update measured here."""
import argparse
import importlib
import statistics
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent.parent
sys.path.insert(0, str(ROOT))
import sdxl_amd  # noqa: E402,F401
from sdxl_amd import unet as NU  # noqa: E402

LORA = importlib.import_module("sdxl-training-improvements_amd.lora")
O = importlib.import_module("sdxl-training-improvements_amd.optimizer")


def timed(fn, reps, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms), min(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    net = NU.NativeUNet()
    g = torch.Generator(device="cuda").manual_seed(0)
    net.weights.copy_((torch.randn(net.param_elems, generator=g, device="cuda") * 0.02).to(torch.bfloat16))
    net.grads.copy_(torch.randn(net.param_elems, generator=g, device="cuda") * 1e-3)
    say(f"lora_bench: {torch.cuda.get_device_name(0)}, SDXL-base arena {net.param_elems} elements, {args.reps} repetitions, HIP events (median / min ms)")
    full = O.AdamWBF16(net, lr=1e-6, weight_decay=0.0)
    med_full, min_full = timed(lambda: full.step(), args.reps)
    say(f"full-arena AdamWBF16 update: {med_full:.3f} / {min_full:.3f} ms")
    del full
    torch.cuda.empty_cache()
    for rank in (16, 64):
        ad = LORA.LoRAAdapters(net, rank=rank)
        for k in ad.targets:
            ad.B(k).normal_(0.0, 0.02, generator=g)
        gb_w = 2 * 2 * ad.base.numel() / 1e9            # merge: W0 read + W written, bf16
        gb_g = 2 * 4 * ad.base.numel() / 1e9            # project: dW read twice, fp32
        m = timed(ad.merge, args.reps)
        p = timed(ad.project, args.reps)
        opt = O.AdamWBF16(ad, lr=1e-6, weight_decay=0.0)
        u = timed(lambda: opt.step(), args.reps)
        total = m[0] + p[0] + u[0]
        say(f"rank {rank}: {len(ad.targets)} targets, {ad.base.numel()} target weights, adapter arena {ad.param_elems} elements")
        say(f"rank {rank}: merge {m[0]:.3f} / {m[1]:.3f} ms ({gb_w / m[0] * 1e3:.0f} GB/s) ; project {p[0]:.3f} / {p[1]:.3f} ms ({gb_g / p[0] * 1e3:.0f} GB/s) ; "
            f"adapter update {u[0]:.3f} / {u[1]:.3f} ms")
        say(f"rank {rank}: merge + project + adapter update = {total:.3f} ms vs full-arena update {med_full:.3f} ms -> "
            f"{'within' if total <= med_full else 'EXCEEDS'} the bar ({total / med_full:.2f}x)")
        ad.restore()
        del opt, ad
        torch.cuda.empty_cache()
    net.close()
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
