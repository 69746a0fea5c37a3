"""Times what the LoRA mode adds and what it removes, on the full SDXL-base handle (no plan, no forward): the merge and the projection of
the default targets (csrc/lora.hip) and the fused update of the adapter arena at ranks 16 and 64, against the full-arena AdamWBF16 update
of the same run.  HIP events, 20 repetitions after 3 warm-up calls, median and minimum.

    python profiles/tools/lora_bench.py [--reps 20] [--out profiles/lora_timing.txt] [--kinds all]

The bar (rank 16): merge + project + adapter update <= the full-arena AdamW update measured here.
--kinds all (profiles/lora_layout_timing.txt): after the plain run, in the same process, the tables of SDXL_DTYPE_LORA_LAYOUTS -- every
accepted tensor, the 3x3 convolutions only, ff.net.0.proj only, and the default (plain) targets through the new dtype -- with the arena
bytes each launch moves per millisecond and the mapped kinds' rate as a fraction of the plain table's at the same rank.  The bar is
reported for the all-kinds table too, not asserted: that table is 2.7x the default one."""
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


EVERY_MODULE = ["to_q", "to_k", "to_v", "to_out.0", "ff.net.0.proj", "ff.net.2", "proj_in", "proj_out", "conv1", "conv2", "conv_shortcut",
                "downsamplers.0.conv", "upsamplers.0.conv", "conv_out", "time_emb_proj", "linear_1", "linear_2"]


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
    ap.add_argument("--kinds", choices=["plain", "all"], default="plain")
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
    if args.kinds == "all":
        shapes = net.param_shapes()
        every = LORA.resolve_targets(shapes, EVERY_MODULE, kinds="all")
        conv3 = [k[: -len(".weight")] for k in every if len(shapes[k]) == 4 and tuple(shapes[k][2:]) == (3, 3)]
        geglu = [k[: -len(".weight")] for k in every if k.endswith("ff.net.0.proj.weight")]
        tables = [("plain (default targets)", None), ("all kinds", EVERY_MODULE), ("3x3 convolutions only", conv3), ("ff.net.0.proj only", geglu)]
        say(f"--kinds all: SDXL_DTYPE_LORA_LAYOUTS; bytes moved = W0 read + W written (merge), dW read twice (project); rate = bytes / median")
        for rank in (16, 64):
            rates = {}
            for label, targets in tables:
                ad = LORA.LoRAAdapters(net, rank=rank, targets=targets, kinds="all")
                for k in ad.targets:
                    ad.B(k).normal_(0.0, 0.02, generator=g)
                m = timed(ad.merge, args.reps)
                p = timed(ad.project, args.reps)
                n = ad.base.numel()
                rates[label] = (2 * 2 * n / 1e6 / m[0], 2 * 4 * n / 1e6 / p[0])
                line = (f"rank {rank} [{label}]: {len(ad.targets)} targets, {n} target weights ; merge {m[0]:.3f} / {m[1]:.3f} ms ({rates[label][0]:.0f} MB/ms) ; "
                        f"project {p[0]:.3f} / {p[1]:.3f} ms ({rates[label][1]:.0f} MB/ms)")
                if label == "all kinds":
                    opt = O.AdamWBF16(ad, lr=1e-6, weight_decay=0.0)
                    u = timed(lambda: opt.step(), args.reps)
                    total = m[0] + p[0] + u[0]
                    line += (f" ; adapter update {u[0]:.3f} ms ; merge + project + adapter update = {total:.3f} ms vs full-arena update {med_full:.3f} ms "
                             f"({total / med_full:.2f}x, reported only)")
                    del opt
                say(line)
                ad.restore()
                del ad
                torch.cuda.empty_cache()
            base = rates["plain (default targets)"]
            for label in ("3x3 convolutions only", "ff.net.0.proj only", "all kinds"):
                rm, rp = rates[label][0] / base[0], rates[label][1] / base[1]
                flag = "" if min(rm, rp) >= 2 / 3 else "  <- below two thirds of the plain rate"
                say(f"rank {rank} [{label}] / plain: merge {rm:.2f}x, project {rp:.2f}x of the plain table's bytes per ms{flag}")
    net.close()
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
