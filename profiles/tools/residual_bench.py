"""Additional skip residuals (csrc/residual.hip): the two kernels at the SDXL-base shapes, and their cost in the step.

    python profiles/tools/residual_bench.py [--reps 9] [--no-step]

Part (a), through the hooks, the nine concats of the SDXL-base plan at B = 4, 128 x 128 latent with every residual present (mid on the
first): 107.5 M residual elements per direction.  Per residual dtype the forward kernel against the plain concat at the same shapes, and
the gradient kernel; device-generated operands, HIP events, warm-up, alternating, medians of --reps samples of the whole set of nine.
Bytes are what the algorithm needs (both halves read and written once as bf16, each residual read once / each gradient written once);
the yardstick is those bytes over the device copy rate.
Part (b): a whole step (forward_loss + backward) of the SDXL-base plan with all ten residuals and all ten gradients against the same
build's step without them, alternating.
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

COPY_RATE = 6.29e12      # measured device copy rate of the MI355X (read + write bytes per second)
# (HW, Ca = hidden, Cb = skip, mid on the hidden half) of the nine concats, in the order the up path runs them
CONCATS = [(1024, 1280, 1280, True), (1024, 1280, 1280, False), (1024, 1280, 640, False), (4096, 1280, 640, False), (4096, 640, 640, False),
           (4096, 640, 320, False), (16384, 640, 320, False), (16384, 320, 320, False), (16384, 320, 320, False)]


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


def kernel_part(B, reps, rdtype):
    L = lib.load()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    g = torch.Generator(device="cuda").manual_seed(1)
    rn = lambda *s: torch.randn(*s, generator=g, device="cuda")
    ops = []
    for HW, Ca, Cb, mid in CONCATS:
        ops.append(dict(HW=HW, Ca=Ca, Cb=Cb, a=rn(B * HW, Ca).to(torch.bfloat16), b=rn(B * HW, Cb).to(torch.bfloat16),
                        ra=rn(B, Ca, HW).to(rdtype) if mid else None, rb=rn(B, Cb, HW).to(rdtype), o=torch.empty(B * HW, Ca + Cb, dtype=torch.bfloat16, device="cuda"),
                        g=rn(B * HW, Ca + Cb).to(torch.bfloat16), da=torch.empty(B, Ca, HW, device="cuda") if mid else None, db=torch.empty(B, Cb, HW, device="cuda")))
    code = 0 if rdtype == torch.float32 else 1

    def fwd():
        for q in ops:
            lib.check(L.sdxl_op_concat_residual(p(q["a"]), q["Ca"], p(q["b"]), q["Cb"], p(q["ra"]), p(q["rb"]), code, p(q["o"]), B, q["HW"], st))

    def plain():
        for q in ops:
            lib.check(L.sdxl_op_concat_residual(p(q["a"]), q["Ca"], p(q["b"]), q["Cb"], None, None, code, p(q["o"]), B, q["HW"], st))

    def grad():
        for q in ops:
            lib.check(L.sdxl_op_concat_residual_grad(p(q["g"]), q["Ca"], q["Cb"], p(q["da"]), p(q["db"]), None, B, q["HW"], st))

    tf, tp, tg = alternate([fwd, plain, grad], reps)
    q = ops[0]      # a spot check at the shape that carries both residuals
    want = torch.cat([(q["a"].float() + q["ra"].float().permute(0, 2, 1).reshape(-1, q["Ca"])).to(torch.bfloat16),
                      (q["b"].float() + q["rb"].float().permute(0, 2, 1).reshape(-1, q["Cb"])).to(torch.bfloat16)], dim=1)
    fwd()
    torch.cuda.synchronize()
    assert torch.equal(q["o"].view(torch.int16), want.view(torch.int16))
    elems = sum(B * q["HW"] * ((q["Ca"] if q["ra"] is not None else 0) + q["Cb"]) for q in ops)
    cat_bytes = sum(2 * 2 * B * q["HW"] * (q["Ca"] + q["Cb"]) for q in ops)
    rsz = 4 if rdtype == torch.float32 else 2
    need_f, need_g = cat_bytes + rsz * elems, (2 + 4) * elems
    name = "fp32" if rdtype == torch.float32 else "bf16"
    mf, mp, mg = statistics.median(tf), statistics.median(tp), statistics.median(tg)
    print(f"[residual] B={B} {name}: {elems / 1e6:.1f} M residual elements ({rsz * elems / 1e6:.0f} MB), nine launches each")
    print(f"[residual] B={B} {name}: concat + residuals {fmt(tf)}")
    print(f"[residual] B={B} {name}: plain concat       {fmt(tp)}")
    print(f"[residual] B={B} {name}: residual gradients {fmt(tg)}")
    print(f"[residual] B={B} {name}: forward bytes {need_f / 1e6:.0f} MB -> {need_f / COPY_RATE * 1e6:.1f} us at the copy rate, reached {need_f / COPY_RATE * 1e6 / mf:.2f} of it "
          f"({need_f / (mf * 1e-6) / 1e12:.2f} TB/s); plain concat {cat_bytes / 1e6:.0f} MB reached {cat_bytes / COPY_RATE * 1e6 / mp:.2f}")
    print(f"[residual] B={B} {name}: gradient bytes {need_g / 1e6:.0f} MB -> {need_g / COPY_RATE * 1e6:.1f} us at the copy rate, reached {need_g / COPY_RATE * 1e6 / mg:.2f} of it "
          f"({need_g / (mg * 1e-6) / 1e12:.2f} TB/s)")


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
    shapes, mid_shape = net.residual_shapes(B, H, W)
    gd = torch.Generator(device="cuda").manual_seed(4)
    res = ([0.1 * torch.randn(s, generator=gd, device="cuda") for s in shapes], 0.1 * torch.randn(mid_shape, generator=gd, device="cuda"))

    def step(on):
        def run():
            torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            net.forward_loss("flow_matching", lat, noise, t, t, ehs, pooled, tid, **(dict(residuals=res, residual_grads=True) if on else {}))
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
    print(f"[residual] step (forward_loss + backward, host upload of the batch included) of the SDXL-base plan B={B} {H}x{W}: without "
          f"{statistics.median(off):.2f} ms (min {min(off):.2f} max {max(off):.2f}), with ten fp32 residuals and ten gradients {statistics.median(on):.2f} ms "
          f"(min {min(on):.2f} max {max(on):.2f}), difference of medians {1e3 * (statistics.median(on) - statistics.median(off)):.0f} us (n = {reps})")
    net.close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--no-step", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("residual_bench: needs a GPU (a timing taken anywhere else says nothing)")
    for dt in (torch.float32, torch.bfloat16):
        kernel_part(4, a.reps, dt)
    if not a.no_step:
        step_part(a.reps)
