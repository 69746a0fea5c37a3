"""Generate tests/golden/schedulefree_kahan.npz by running the REAL reference optimizer class.

Authoring only (needs the reference tree that oracle/make_goldens.py names in REF).  Imports the reference's own
`src/training/optimizers/adamw_schedulefree/__init__.py::AdamWScheduleFreeKahan` (unchanged), with the stand-in modules
of oracle/make_goldens.py for third-party packages that are not installed, and steps it on seeded bf16 parameters on
the CPU.  Output is data only: per case the initial parameters, the gradient of each step, and after each step the
parameters, exp_avg, exp_avg_sq, kahan_comp (kahan_sum cases), the gradient as the reference left it (it adds kahan_comp
to p.grad in place), `last_lr` and `lr_max`.  All tensors are stored as bf16 bit patterns (uint16).

The reference's Kahan term is identically +0 for finite values (round-to-nearest is symmetric, so rn(b - p) = -rn(p - b)):
this script asserts that in every element of every case.

Usage:  python tests/make_schedulefree_goldens.py
"""
from __future__ import annotations

import os
import sys
import tempfile
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
OUT = ROOT / "tests" / "golden" / "schedulefree_kahan.npz"

# name, n, lr, betas, eps, weight_decay, warmup_steps, kahan_sum, steps, grad scale
CASES = [
    ("warmup", 2048, 1e-3, (0.9, 0.999), 1e-8, 0.01, 3, True, 5, 1e-2),
    ("nowd", 2048, 1e-4, (0.9, 0.999), 1e-8, 0.0, 0, True, 3, 1e-3),
    ("nokahan", 2048, 1e-3, (0.9, 0.999), 1e-8, 0.01, 2, False, 3, 1e-2),
    ("default", 2048, 1e-6, (0.9, 0.999), 1e-8, 0.01, 0, True, 3, 1e-3),
    ("betas", 1024, 3e-3, (0.8, 0.95), 1e-6, 0.05, 1, True, 3, 1e-1),
    ("edge", 2048, 0.5, (0.9, 0.999), 1e-8, 0.01, 0, True, 3, 1.0),
]


def bits(t: torch.Tensor) -> np.ndarray:
    return t.detach().contiguous().view(torch.int16).numpy().astype(np.uint16)


def _edge(t: torch.Tensor, gen: torch.Generator) -> torch.Tensor:
    """zeros, -0 and tiny magnitudes (normal in float32: no denormal appears in any product) in a quarter of the elements"""
    n = t.numel()
    sel = torch.randint(0, 4, (n,), generator=gen)
    t = t.clone()
    t[sel == 0] = 0.0
    t[sel == 1] = -0.0
    tiny = (torch.rand(n, generator=gen) + 0.5) * 1e-12 * torch.where(torch.rand(n, generator=gen) < 0.5, -1.0, 1.0)
    t[sel == 2] = tiny[sel == 2].to(t.dtype)
    return t


def import_reference():
    sys.path.insert(0, str(ROOT / "oracle"))
    from make_goldens import REF, _Blank, _Dummy, _stub
    _stub("wandb", init=lambda *a, **k: None, log=lambda *a, **k: None, finish=lambda *a, **k: None, Image=_Dummy, run=None)
    _stub("colorama", Fore=_Blank(), Style=_Blank(), Back=_Blank(), init=lambda *a, **k: None)
    _stub("spacy", load=lambda *a, **k: None)
    _stub("diffusers", DDPMScheduler=_Dummy, StableDiffusionXLPipeline=_Dummy, AutoencoderKL=_Dummy, UNet2DConditionModel=_Dummy)
    _stub("xformers"); _stub("xformers.ops")
    os.chdir(tempfile.mkdtemp(prefix="refimport_"))
    sys.path.insert(0, str(REF))
    from src.training.optimizers.adamw_schedulefree import AdamWScheduleFreeKahan      # the reference class, unchanged
    return AdamWScheduleFreeKahan


def main():
    Ref = import_reference()
    g = {}
    for ci, (name, n, lr, betas, eps, wd, warm, kahan, steps, gs) in enumerate(CASES):
        gen = torch.Generator().manual_seed(2000 + ci)
        p0 = (torch.randn(n, generator=gen) * 0.05).to(torch.bfloat16)
        if name == "edge":
            p0 = _edge(p0, gen)
        p = torch.nn.Parameter(p0.clone())
        opt = Ref([p], lr=lr, betas=betas, eps=eps, weight_decay=wd, warmup_steps=warm, kahan_sum=kahan)
        g[f"{name}_hyper"] = np.array([lr, betas[0], betas[1], eps, wd, warm, int(kahan)], dtype=np.float64)
        g[f"{name}_p0"] = bits(p0)
        for st in range(1, steps + 1):
            grad = (torch.randn(n, generator=gen) * gs).to(torch.bfloat16)
            if name == "edge":
                grad = _edge(grad, gen)
            g[f"{name}_grad{st}"] = bits(grad)
            p.grad = grad.clone()
            opt.step()
            s = opt.state[p]
            g[f"{name}_p{st}"] = bits(p.data)
            g[f"{name}_m{st}"] = bits(s["exp_avg"])
            g[f"{name}_v{st}"] = bits(s["exp_avg_sq"])
            g[f"{name}_gafter{st}"] = bits(p.grad)
            if kahan:
                c = s["kahan_comp"]
                assert bool((bits(c) == 0).all()), f"{name} step {st}: kahan_comp is not +0 everywhere"
                g[f"{name}_c{st}"] = bits(c)
            g[f"{name}_lr{st}"] = np.array([opt.get_last_lr(), opt.lr_max], dtype=np.float64)
            assert opt.k == st
        g[f"{name}_steps"] = np.array(steps)
        print(f"{name}: {int((bits(p.data) != bits(p0)).sum())}/{n} weights changed in {steps} steps")
    g["cases"] = np.array([c[0] for c in CASES])
    np.savez_compressed(OUT, **g)
    print("wrote", OUT, OUT.stat().st_size, "bytes")


if __name__ == "__main__":
    main()
