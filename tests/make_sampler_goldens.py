"""Generate tests/golden/sampler_reference.npz by running the REAL reference NoiseScheduler's sampling functions.

Authoring only (needs the reference tree that oracle/make_goldens.py names in REF).  Imports the reference's own
`src/training/schedulers/novelai_v3.py::NoiseScheduler` (unchanged), with the stand-in modules of oracle/make_goldens.py for the
third-party packages that are not installed, takes `rho = 7` (the attribute is missing from the reference's ModelConfig) and
records, on the CPU in fp32:

    get_karras_scalings(sigma)                 for a vector of sigmas from 0.002 to 20000
    ztsnr_first_step(n, sigma_1, model_fn)
    euler_step(x, sigma_i, sigma_next, model_fn)       three (sigma_i, sigma_next) pairs
    sample_with_ztsnr(model_fn, (2, 4, 8, 8), 6)       the whole run, its noise (the draw it makes after torch.manual_seed) and its sigmas

`model_fn` is a fixed elementwise stand-in, tanh(0.5 x) + 0.1, that ignores its second argument (the reference passes sigma, and inf on
the first step).  Output is data only: inputs and what the reference returned.

Usage:  python tests/make_sampler_goldens.py
"""
from __future__ import annotations

import os
import sys
import tempfile
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
OUT = ROOT / "tests" / "golden" / "sampler_reference.npz"
SHAPE, N, SEED = (2, 4, 8, 8), 6, 4321


def model_fn(x, _sigma):
    return torch.tanh(0.5 * x) + 0.1


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
    from src.data.config import Config
    from src.training.schedulers.novelai_v3 import NoiseScheduler      # the reference class, unchanged
    return NoiseScheduler, Config


def main():
    NoiseScheduler, Config = import_reference()
    cfg = Config()
    cfg.model.rho = 7.0
    sched = NoiseScheduler(cfg, "cpu")
    g = {}
    # --- get_karras_scalings ---------------------------------------------------------------
    sig = torch.tensor([0.002, 0.05, 0.5, 1.0, 3.7, 14.6, 80.0, 1234.5, 20000.0], dtype=torch.float32)
    c_skip, c_out, c_in = sched.get_karras_scalings(sig)
    g["ks_sigma"], g["ks_c_skip"], g["ks_c_out"], g["ks_c_in"] = sig.numpy(), c_skip.numpy(), c_out.numpy(), c_in.numpy()
    # --- the sigma grid sample_with_ztsnr uses -----------------------------------------------
    sigmas = sched.get_sigmas(N)
    g["sigmas"] = sigmas.numpy()
    # --- ztsnr_first_step / euler_step on seeded inputs --------------------------------------
    gen = torch.Generator().manual_seed(SEED + 1)
    n = torch.randn(SHAPE, generator=gen)
    g["fs_n"] = n.numpy()
    g["fs_out"] = sched.ztsnr_first_step(n, sigmas[0], model_fn).numpy()
    pairs = [(0, 1), (2, 3), (4, 5)]
    g["es_pairs"] = np.array(pairs)
    for k, (i, j) in enumerate(pairs):
        x = torch.randn(SHAPE, generator=gen) * sigmas[i]
        g[f"es{k}_x"] = x.numpy()
        g[f"es{k}_out"] = sched.euler_step(x, sigmas[i], sigmas[j], model_fn).numpy()
    # --- the whole run: it draws its own noise from the global generator ----------------------
    torch.manual_seed(SEED)
    out = sched.sample_with_ztsnr(model_fn, SHAPE, N)
    torch.manual_seed(SEED)
    g["run_n"] = torch.randn(SHAPE).numpy()
    g["run_out"] = out.numpy()
    assert all(np.isfinite(v).all() for v in g.values())
    np.savez_compressed(OUT, **g)
    print("wrote", OUT, OUT.stat().st_size, "bytes")


if __name__ == "__main__":
    main()
