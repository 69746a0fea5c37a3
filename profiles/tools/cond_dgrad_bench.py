"""Conditioning-gradient kernel (csrc/cond_dgrad.hip) against the generic NN GEMM it replaces, and its cost in the step.

    python profiles/tools/cond_dgrad_bench.py [--reps 9] [--no-step]

Part 1, through the hooks, at the shapes the SDXL-base step runs at B = 4:
    d prompt_embeds  (308, 2048, [12800, 153600])      d pooled  (4, 1280, [1280], ldb 2816)
  new:      sdxl_op_cond_dgrad, one call (both groups, fp32 out)
  baseline: sdxl_op_gemm form 1 (NN, bf16 out) once per group with the split-K gemm_pick_splitk_small would choose for a linear
            dgrad of that shape (restated below); its bf16 output is why it cannot ship, it is the speed to beat.
  Device-generated operands, HIP events, warm-up, the two alternating in one process, median and spread of --reps samples.
Part 2: the whole backward of the SDXL-base plan (B = 4, 128 x 128 latent, random weights) with and without the request, alternating.
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


def splitk_small(M, N, K):
    """gemm_pick_splitk_small (csrc/gemm.hip) for a linear dgrad (kind 2), product build"""
    if K % 64 or (M < 64 and K < 1024):
        return 1
    tiles = -(-M // 128) * -(-N // (160 if N % 160 == 0 else 128))
    if tiles >= 128:
        return 1
    s = min(256 // tiles, K // 64 // 4, 32)
    return 1 if s < 2 else s


def timed(fn, reps, warm=3):
    for _ in range(warm):
        fn()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) * 1e3)
    return out


def alternate(fns, reps):
    for f in fns:
        timed(f, 0)
    samples = [[] for _ in fns]
    for _ in range(reps):
        for i, f in enumerate(fns):
            samples[i] += timed(f, 1, warm=0)
    return samples


def fmt(v):
    return f"median {statistics.median(v):8.1f} us  min {min(v):8.1f}  max {max(v):8.1f}  (n = {len(v)})"


def kernel_part(M, N, Ks, ldb, reps):
    L = lib.load()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    g = torch.Generator(device="cuda").manual_seed(1)
    As = [torch.randn(M, K, generator=g, device="cuda").to(torch.bfloat16) for K in Ks]
    Ws = [(torch.randn(K, ldb, generator=g, device="cuda") * 0.02).to(torch.bfloat16) for K in Ks]
    Wc = [w[:, :N].contiguous() for w in Ws]      # the baseline entry point takes ldb = N
    out32 = torch.empty(M, N, dtype=torch.float32, device="cuda")
    out16 = [torch.empty(M, N, dtype=torch.bfloat16, device="cuda") for _ in Ks]
    n = len(Ks)
    pa = (C.c_void_p * n)(*[a.data_ptr() for a in As])
    pw = (C.c_void_p * n)(*[w.data_ptr() for w in Ws])
    lda, ldbs, Kc = (C.c_long * n)(*Ks), (C.c_long * n)(*[ldb] * n), (C.c_int * n)(*Ks)
    sk = [splitk_small(M, N, K) for K in Ks]

    def new():
        lib.check(L.sdxl_op_cond_dgrad(n, pa, lda, pw, ldbs, Kc, C.c_void_p(out32.data_ptr()), N, M, N, st))

    def base():
        for a, w, o, K, s in zip(As, Wc, out16, Ks, sk):
            lib.check(L.sdxl_op_gemm(1, C.c_void_p(a.data_ptr()), C.c_void_p(w.data_ptr()), C.c_void_p(o.data_ptr()), M, N, K, None, None, 0, s, st))

    tn, tb = alternate([new, base], reps)
    ref = sum(a.float() @ w[:, :N].float() for a, w in zip(As, Ws))
    err = float((out32 - ref).abs().max() / ref.abs().max())
    need = sum(2 * (M * K + K * N) for K in Ks) + 4 * M * N
    mn = statistics.median(tn)
    print(f"[cond_dgrad] ({M}, {N}, {Ks}, ldb {ldb}): new      {fmt(tn)}")
    print(f"[cond_dgrad] ({M}, {N}, {Ks}, ldb {ldb}): baseline {fmt(tb)}  (sdxl_op_gemm form 1, split-K {sk}, bf16 out)")
    print(f"[cond_dgrad] ({M}, {N}, {Ks}): algorithmic bytes {need / 1e6:.1f} MB -> {need / (mn * 1e-6) / 1e12:.2f} TB/s of {COPY_RATE / 1e12:.2f} TB/s copy rate; "
          f"{2 * M * N * sum(Ks) / (mn * 1e-6) / 1e12:.0f} TFLOP/s; new / baseline {mn / statistics.median(tb):.2f}; max rel err vs fp32 matmul {err:.2e}")


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

    def backward(cond):
        def run():
            net.forward_loss("flow_matching", lat, noise, t, t, ehs, pooled, tid, **({"cond_grads": True} if cond else {}))
            torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            net.backward(1.0, True)
            b.record()
            b.synchronize()
            return a.elapsed_time(b)
        return run

    net.zero_grads()
    fns = [backward(False), backward(True)]
    for f in fns:
        for _ in range(2):
            f()
    off, on = [], []
    for _ in range(reps):
        off.append(fns[0]())
        on.append(fns[1]())
    ws = net.workspace.numel() / 2 ** 30
    print(f"[cond_dgrad] backward of the SDXL-base plan B={B} {H}x{W} (workspace {ws:.1f} GiB, {net.param_elems / 1e9:.2f} G parameters): "
          f"without {statistics.median(off):.2f} ms (min {min(off):.2f} max {max(off):.2f}), with both gradients {statistics.median(on):.2f} ms "
          f"(min {min(on):.2f} max {max(on):.2f}), difference of medians {1e3 * (statistics.median(on) - statistics.median(off)):.0f} us (n = {reps})")
    net.close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--no-step", action="store_true")
    a = ap.parse_args()
    kernel_part(308, 2048, [12800, 153600], 2048, a.reps)
    kernel_part(4, 1280, [1280], 2816, a.reps)
    if not a.no_step:
        step_part(a.reps)
