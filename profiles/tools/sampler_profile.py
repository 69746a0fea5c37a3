"""A full-size native sample for profiling and timing (SDXL-base shapes, synthetic weights, B = 2 with guidance: plan batch 4, 128 x 128).

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o sampler -- python profiles/tools/sampler_profile.py --mode sample
        one warm-up sample of 2 steps, then ONE 30-step sample: the kernel statistics of profiles/sampler_kernel_stats.csv
    python profiles/tools/sampler_profile.py --mode time
        device events, profiler off, medians of 5 alternated runs: the 30-step native sample against 30 calls of sdxl_unet_forward
        with a sample / prediction pair at the same batch (forward + the two device-to-device copies: what the library offered a
        sampling loop before the sampler step existed; the forward's own kernels are the same in both)
"""
import argparse
import ctypes as C
import statistics
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent.parent))
import sdxl_amd  # noqa: E402,F401
from sdxl_amd import lib, sampler as S, synth  # noqa: E402
from sdxl_amd import unet as NU  # noqa: E402

B, H, W, STEPS = 2, 128, 128, 30


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=("sample", "time"), default="sample")
    ap.add_argument("--rescale", type=float, default=0.0)
    a = ap.parse_args()
    net = NU.NativeUNet(NU.make_config())
    synth.load_synthetic(net, seed=0)
    g = torch.Generator().manual_seed(3)
    r = lambda *s: torch.randn(*s, generator=g)
    pe, po = r(B, 77, 2048).to(torch.bfloat16), r(B, 1280).to(torch.bfloat16)
    ti = torch.tensor([[8.0 * W, 8.0 * H, 0, 0, 8.0 * W, 8.0 * H]] * B)
    noise = r(B, 4, H, W)
    sm = S.NativeSampler(net, "ddpm", "v_prediction", True, "trained")
    run = lambda n: sm.sample(pe, po, ti, height=H, width=W, num_steps=n, guidance_scale=5.0, guidance_rescale=a.rescale, noise=noise)
    run(2)
    torch.cuda.synchronize()
    if a.mode == "sample":
        out = run(STEPS)
        torch.cuda.synchronize()
        print("finite", bool(torch.isfinite(out).all()), "max |x|", float(out.abs().max()))
        net.close()
        return
    # the forward-with-copies loop at the same plan batch
    PB = 2 * B
    d = net.device
    x8 = torch.zeros(PB * H * W, 8, dtype=torch.bfloat16, device=d)
    out8 = torch.empty_like(x8)
    cond = [torch.zeros(PB, device=d), torch.cat([pe, pe]).to(d), torch.cat([po, po]).to(d), torch.cat([ti, ti]).to(d)]
    net.plan(PB, H, W, 77)
    b = lib.SamplerBatch(PB, H, W, 77, None, None, None, *[t.data_ptr() for t in cond], None)
    st = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def forwards(n):
        for _ in range(n):
            lib.check(net.L.sdxl_unet_forward(net.h, C.c_void_p(x8.data_ptr()), C.byref(b), C.c_void_p(out8.data_ptr()), st()))

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    forwards(2)
    ts, tf = [], []
    for _ in range(5):
        ts.append(timed(lambda: run(STEPS)))
        tf.append(timed(lambda: forwards(STEPS)))
    ms, mf = statistics.median(ts), statistics.median(tf)
    print(f"native sample, {STEPS} steps, plan batch {PB}: {[round(t, 2) for t in ts]} ms, median {ms:.2f} = {ms / STEPS:.3f} ms per step")
    print(f"{STEPS} x sdxl_unet_forward with copies:        {[round(t, 2) for t in tf]} ms, median {mf:.2f} = {mf / STEPS:.3f} ms per call")
    print(f"per step: sampler - forward-with-copies = {(ms - mf) / STEPS * 1e3:.1f} us")
    net.close()


if __name__ == "__main__":
    main()
