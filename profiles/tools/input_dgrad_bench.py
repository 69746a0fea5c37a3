"""Input gradient (csrc/input_dgrad.hip): the kernel at the SDXL-base shape, and its cost in the step.

    python profiles/tools/input_dgrad_bench.py [--reps 9] [--no-step]

Part (a), through the hook, B = 4, 128 x 128, Cout = 320 (conv_in of SDXL-base; dy = 42 MB bf16) for in_channels 4, 9 and 16: the kernel
against a plain device copy of the same dy bytes (torch's copy_ of one dy buffer into another), the yardstick.  Every launch takes the
next of --bufs dy / dx buffers (default 8: 336 MB of dy, more than the 256 MB MALL), so no operand is still cached from the launch that
used it last; a sample is one pass over all buffers between two HIP events, divided by their number; warm-up first, the kernel and the
copy alternating, medians of --reps samples.  Bytes are what the algorithm needs (dy read once, dx written once; the 92 KB weight is not
counted), FLOPs 2 * 9 * Cout * in_channels per pixel.
Part (b): a whole step (forward_loss + backward) of the SDXL-base plan with the request against the same build's step without, alternating.
Prints one line per figure."""
import argparse
import ctypes as C
import statistics
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[2]))
import sdxl_amd  # noqa: E402,F401
from sdxl_amd import lib  # noqa: E402
from sdxl_amd import unet as NU  # noqa: E402


def event_time(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3


def alternate(fns, reps, warm=3):
    for f in fns:
        for _ in range(warm):
            f()
    torch.cuda.synchronize()
    samples = [[] for _ in fns]
    for _ in range(reps):
        for i, f in enumerate(fns):
            samples[i].append(event_time(f))
    return samples


def fmt(v):
    return f"median {statistics.median(v):8.1f} us  min {min(v):8.1f}  max {max(v):8.1f}  (n = {len(v)})"


def kernel_part(B, H, W, cout, reps, bufs):
    L = lib.load()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t: C.c_void_p(t.data_ptr())
    g = torch.Generator(device="cuda").manual_seed(1)
    dys = [torch.randn(B * H * W, cout, generator=g, device="cuda").to(torch.bfloat16) for _ in range(bufs)]
    dst = [torch.empty_like(t) for t in dys]

    def copy():
        for s, d in zip(dys, dst):
            d.copy_(s)

    for cin in (4, 9, 16):
        cs = 8 if cin <= 8 else 16
        w = torch.zeros(cout, 9, cs, dtype=torch.bfloat16, device="cuda")
        w[:, :, :cin] = (torch.randn(cout, 9, cin, generator=g, device="cuda") * (9 * cout) ** -0.5).to(torch.bfloat16)
        dxs = [torch.empty(B, cin, H, W, device="cuda") for _ in range(bufs)]

        def kernel():
            for s, d in zip(dys, dxs):
                lib.check(L.sdxl_op_input_dgrad(p(s), p(w), p(d), None, B, H, W, cin, cout, st))

        tk, tc = alternate([kernel, copy], reps)
        tk, tc = [t / bufs for t in tk], [t / bufs for t in tc]
        # a spot check against conv_transpose2d in fp32 on one buffer
        want = torch.nn.functional.conv_transpose2d(dys[0].float().reshape(B, H, W, cout).permute(0, 3, 1, 2),
                                                    w[:, :, :cin].float().reshape(cout, 3, 3, cin).permute(0, 3, 1, 2), padding=1)
        err = float((dxs[0] - want).abs().max() / want.abs().max())
        assert err < 1e-3, err
        dy_bytes, dx_bytes = dys[0].numel() * 2, dxs[0].numel() * 4
        mk, mc = statistics.median(tk), statistics.median(tc)
        flop = 2.0 * 9 * cout * cin * B * H * W
        print(f"[input_dgrad] B={B} {H}x{W} Cout={cout} in_channels={cin}: kernel {fmt(tk)}")
        print(f"[input_dgrad] B={B} {H}x{W} Cout={cout} in_channels={cin}: copy of the same dy bytes ({dy_bytes / 1e6:.1f} MB read + written) {fmt(tc)}")
        print(f"[input_dgrad] B={B} {H}x{W} Cout={cout} in_channels={cin}: {(dy_bytes + dx_bytes) / 1e6:.1f} MB needed -> {(dy_bytes + dx_bytes) / (mk * 1e-6) / 1e12:.2f} TB/s, "
              f"{flop / (mk * 1e-6) / 1e12:.1f} TFLOP/s useful; kernel / copy = {mk / mc:.2f} (copy: {2 * dy_bytes / (mc * 1e-6) / 1e12:.2f} TB/s read + write); "
              f"max |dx - conv_transpose2d| / max |.| = {err:.1e}")


def step_part(reps):
    B, H, W = 4, 128, 128
    net = NU.NativeUNet()
    net.weights.normal_(0.0, 0.02)
    g = torch.Generator().manual_seed(3)
    r = lambda *s: torch.randn(*s, generator=g)
    lat, noise = r(B, 4, H, W), r(B, 4, H, W)
    ehs, pooled = r(B, 77, 2048), r(B, 1280)
    tid = torch.tensor([[8.0 * H, 8.0 * W, 0, 0, 8.0 * H, 8.0 * W]] * B)
    t = torch.sigmoid(r(B))

    def step(on):
        def run():
            torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            net.forward_loss("flow_matching", lat, noise, t, t, ehs, pooled, tid, **(dict(input_grad=True) if on else {}))
            net.backward(1.0, True)
            b.record()
            b.synchronize()
            return a.elapsed_time(b)
        return run

    net.zero_grads()
    fns = [step(False), step(True)]
    for f in fns:
        for _ in range(2):
            f()
    off, on = [], []
    for _ in range(reps):
        off.append(fns[0]())
        on.append(fns[1]())
    print(f"[input_dgrad] step (forward_loss + backward, host upload of the batch included) of the SDXL-base plan B={B} {H}x{W}: without "
          f"{statistics.median(off):.2f} ms (min {min(off):.2f} max {max(off):.2f}), with d_input {statistics.median(on):.2f} ms "
          f"(min {min(on):.2f} max {max(on):.2f}), difference of medians {1e3 * (statistics.median(on) - statistics.median(off)):.0f} us (n = {reps})")
    net.close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--bufs", type=int, default=8)
    ap.add_argument("--no-step", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("input_dgrad_bench: needs a GPU (a timing taken anywhere else says nothing)")
    kernel_part(4, 128, 128, 320, a.reps, a.bufs)
    if not a.no_step:
        step_part(a.reps)
