"""Worker of tests/test_gpu_schedulefree.py::test_zero1_update_bit_equal_to_unsharded (one process per rank, all on cuda:0, gloo).

As tests/_zero1_worker.py, with the schedule-free Kahan AdamW (compensated, Kahan on, warm-up crossing): path A = bucketed
reduce-scatter -> norm of the owned slices + one float all-reduced -> clip coefficient -> the update on the owned slices ->
all-gather of the parameters; path B = bucketed all-reduce -> the update over the whole arena.  After three updates the
parameters must be bit-identical, and so must every optimizer-state element a rank owns."""
import ctypes as C
import importlib
import os
import sys
from pathlib import Path

import torch
import torch.distributed as dist

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import sdxl_amd  # noqa: E402,F401
from sdxl_amd import lib  # noqa: E402

D = importlib.import_module("sdxl-training-improvements_amd.distributed")
O = importlib.import_module("sdxl-training-improvements_amd.optimizer")


class Arena:
    def __init__(self, w):
        self.L = lib.load()
        self.weights = w.clone()
        self.grads = torch.zeros(w.numel(), dtype=torch.float32, device=w.device)

    def zero_grads(self):
        pass


def main():
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    D.init_process_group("gloo")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    L = lib.load()
    total = 3 * 65536 + 4096
    segs = [(2 * 65536 + 4096, 65536), (65536, 65536 + 4096), (0, 65536)]      # reverse execution order
    w0 = (torch.randn(total, generator=torch.Generator().manual_seed(7)) * 0.05).to(torch.bfloat16).to(dev)
    nets = {"zero": Arena(w0), "full": Arena(w0)}
    opts = {k: O.AdamWScheduleFreeKahanBF16(x, lr=1e-2, weight_decay=0.05, warmup_steps=2) for k, x in nets.items()}
    st = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)
    ok = True
    for step in range(3):
        g = torch.randn(total, generator=torch.Generator().manual_seed(100 * step + rank)).to(dev) * 3.0

        def cast(off, n, dst, g=g):
            dst.copy_((g[off:off + n] * (1.0 / world)).to(torch.bfloat16))

        if step == 0:
            zs = D.ShardedGradSync(total, cast, torch.bfloat16, dev)
            fs = D.GradSync(total, cast, torch.bfloat16, dev)
        zs.cast = fs.cast = cast
        for k, (off, n) in enumerate(segs):
            zs.on_segment(k, off, n)
        zs.finish()
        buf = torch.zeros(2, dtype=torch.float32, device=dev)
        sh = zs.reduced()
        lib.check(L.sdxl_sumsq(C.c_void_p(sh.data_ptr()), 1, sh.numel(), C.c_void_p(buf.data_ptr()), st()))
        zs.global_sumsq(buf[0:1])
        lib.check(L.sdxl_clip_coef(C.c_void_p(buf.data_ptr()), 1.0, C.c_void_p(buf.data_ptr() + 4), st()))
        opts["zero"].step(sh, grad_scale=buf[1:2], pieces=zs.pieces)
        zs.gather_params(nets["zero"].weights)
        for k, (off, n) in enumerate(segs):
            fs.on_segment(k, off, n)
        fs.finish()
        opts["full"].step(fs.reduced(), grad_scale=buf[1:2])          # the same coefficient on every rank (see _zero1_worker.py)
        torch.cuda.synchronize()
        ok = ok and float(buf[1]) < 1.0
        ok = ok and torch.equal(nets["zero"].weights, nets["full"].weights)
        for off, n, _ in zs.pieces:
            for a, b in zip(opts["zero"].state_arenas(), opts["full"].state_arenas()):
                ok = ok and torch.equal(a[off:off + n], b[off:off + n])
        if not ok:
            print(f"rank {rank} step {step}: mismatch", flush=True)
        ok = ok and not torch.equal(nets["zero"].weights, w0)
    ok = ok and bool((opts["full"].kahan_comp != 0).any())
    flag = torch.tensor([1.0 if ok else 0.0])
    dist.all_reduce(flag, op=dist.ReduceOp.MIN)
    if rank == 0:
        print("SFK_ZERO1_OK" if float(flag) == 1.0 else "SFK_ZERO1_MISMATCH", flush=True)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
