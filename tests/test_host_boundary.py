"""CPU checks of the drop-in boundary: the C-ABI library loads and exports every symbol include/sdxlstep.h declares,
fails loudly without a GPU (no fallback), and the host-side mirror of the trainer-plugin surface behaves like the
reference's (config loading rule, batch validation, method dispatch, accumulation semantics, metric keys)."""
import ctypes as C
import re
from pathlib import Path

import pytest
import torch

import sdxl_amd  # noqa: F401
from sdxl_amd import lib

ROOT = Path(__file__).resolve().parent.parent


def test_header_symbols_all_exported_and_bound():
    """include/sdxlstep.h (the boundary) <-> lib.SIGNATURES <-> the product .so, symbol for symbol; the test hooks and the experiment
    ABI live in include/sdxlstep_diag.h: part 1 is exported by the product library too, part 2 by the diagnostics build ONLY (the
    product library must not carry the experiments)."""
    names = lambda text: set(re.findall(r"\b(sdxl_[a-z0-9_]+)\s*\(", text))
    declared = names((ROOT / "include" / "sdxlstep.h").read_text())
    dh = (ROOT / "include" / "sdxlstep_diag.h").read_text()
    part1, part2 = dh.split("part 2: experiment ABI", 1)
    hooks, experiments = names(part1.split("part 1: test hooks", 1)[1]), names(part2)
    assert len(declared) <= 58 and len(hooks) == 29 and not (declared & (hooks | experiments))
    L = lib.load()
    for name in sorted(declared | hooks):
        assert hasattr(L, name), f"{name} declared but not exported by {lib.LIB_PATH.name}"
    assert declared == set(lib.SIGNATURES) | {"sdxl_last_error"}, (declared ^ (set(lib.SIGNATURES) | {"sdxl_last_error"}))
    assert hooks == set(lib.TEST_HOOK_SIGNATURES) and experiments == set(lib.DIAG_SIGNATURES)
    for name in sorted(experiments):
        assert hasattr(L, name) == lib.DIAG, f"{name}: experiment ABI {'missing from the diagnostics' if lib.DIAG else 'present in the PRODUCT'} library"
    # ... and the library's ACTUAL dynamic surface is that list and nothing else: built with -fvisibility=hidden + a version script
    # (csrc/exports.map), so no C++ internals (launch_gemm, Engine::build, ...), kernel handles or __device_stub__s leak out
    import shutil
    import subprocess
    nm = shutil.which("nm") or "/opt/rocm/lib/llvm/bin/llvm-nm"
    out = subprocess.run([nm, "-D", "--defined-only", str(lib.LIB_PATH)], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    want = declared | hooks | (experiments if lib.DIAG else set())
    assert exported == want, f"unexpected dynamic symbols: {sorted(exported - want)[:10]}; missing: {sorted(want - exported)[:10]}"


def test_fails_loudly_without_gpu():
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    L = lib.load()
    cfg = lib.UNetConfig()
    assert L.sdxl_default_config(C.byref(cfg)) == 0 and list(cfg.block_out_channels) == [320, 640, 1280]
    h = C.c_void_p()
    rc = L.sdxl_create(C.byref(cfg), 0, C.byref(h))
    assert rc != 0 and b"hip" in L.sdxl_last_error().lower()
    from sdxl_amd import unet
    with pytest.raises(lib.SdxlError):
        unet.NativeUNet()


def test_bad_arguments_are_reported_not_crashed():
    L = lib.load()
    assert L.sdxl_default_config(None) == 1 and b"null" in L.sdxl_last_error()
    assert L.sdxl_bind_params(None, None, None) == 1
    assert L.sdxl_num_params(None) == -1
    # row f1 / f3 entry points: argument errors are reported before anything touches a device
    import ctypes as C
    cfg = lib.AdamWConfig()
    assert L.sdxl_adamw_default_config(C.byref(cfg)) == 0 and cfg.beta1 == 0.9 and cfg.reference_ema == 1
    assert L.sdxl_adamw_default_config(None) == 1
    buf = (C.c_char * 256)()
    p16 = C.c_void_p((C.addressof(buf) + 15) & ~15)
    assert L.sdxl_adamw_bf16_step(p16, p16, 0, p16, p16, p16, 7, C.byref(cfg), None, None, None) == 1      # n % 8
    assert b"multiple of 8" in L.sdxl_last_error()
    assert L.sdxl_adamw_bf16_step(p16, p16, 5, p16, p16, p16, 8, C.byref(cfg), None, None, None) == 1      # dtype
    cfg.beta2 = 1.5
    assert L.sdxl_adamw_bf16_step(p16, p16, 0, p16, p16, p16, 8, C.byref(cfg), None, None, None) == 1      # hyper-parameters
    assert L.sdxl_adamw_bf16_step(None, p16, 0, p16, p16, p16, 8, None, None, None, None) == 1
    assert L.sdxl_sumsq(None, 0, 8, None, None) == 1 and L.sdxl_clip_coef(None, 1.0, None, None) == 1
    assert L.sdxl_set_join_mode(None, 1) == 1 and L.sdxl_param_range(None, 0, None, None) == 1


def test_config_yaml_rule(tmp_path):
    import importlib
    cfgm = importlib.import_module("sdxl-training-improvements_amd.config")
    p = tmp_path / "c.yaml"
    p.write_text("training:\n  method: flow_matching\n  gradient_accumulation_steps: 4\n  bogus_key: 1\n"
                 "model:\n  min_snr_gamma: null\nunknown_section:\n  a: 1\n")
    c = cfgm.Config.from_yaml(p)
    assert c.training.method == "flow_matching" and c.training.gradient_accumulation_steps == 4
    assert c.model.min_snr_gamma is None and c.model.sigma_max == 20000.0 and not hasattr(c.training, "bogus_key")
    d = cfgm.Config.from_yaml(tmp_path / "missing.yaml")
    assert d.training.method == "ddpm" and d.model.min_snr_gamma == 5.0 and d.optimizer.optimizer_type == "adamw_bf16"


def test_scheduler_matches_reference_goldens(golden):
    import importlib
    import numpy as np
    cfgm = importlib.import_module("sdxl-training-improvements_amd.config")
    sch = importlib.import_module("sdxl-training-improvements_amd.scheduler")
    s = sch.NoiseScheduler(cfgm.Config())
    assert np.array_equal(s.sigmas.numpy(), golden["karras_table"])
    for c in range(int(golden["n_sched_cases"])):
        k = f"sch{c}"
        x, n, t = (torch.from_numpy(golden[f"{k}_{q}"]) for q in ("x", "noise", "t"))
        assert np.array_equal(s.add_noise(x, n, t).numpy(), golden[f"{k}_noisy"])
        assert np.array_equal(s.get_velocity(x, n, t).numpy(), golden[f"{k}_vel"])
        assert np.array_equal(s.get_snr(t).numpy(), golden[f"{k}_snr"])
    torch.manual_seed(123)
    assert np.array_equal(s.sample_timesteps(8).numpy(), golden["sample_timesteps_seed123_B8"])


class FakeNet:
    """Records what the trainer asks of the native UNet."""
    param_elems = 16
    device = "cpu"

    def __init__(self):
        self.calls = []
        self.grads = torch.zeros(16)
        self.weights = torch.zeros(16, dtype=torch.bfloat16)

    def zero_grads(self):
        self.calls.append(("zero",))

    def forward_loss(self, method, *a, **k):
        self.calls.append(("fwd", method, k))

    def backward(self, scale, first, on_segment=None):
        self.calls.append(("bwd", round(scale, 6), first))

    def read_loss(self):
        return [0.5, 0, 8.0, 16.0, 4.0, 9.0, 25.0, 1.0]

    def grad_norm(self):
        return 0.0


def _batch(B=2):
    return {"vae_latents": torch.randn(B, 4, 8, 8), "prompt_embeds": torch.randn(B, 77, 16),
            "pooled_prompt_embeds": torch.randn(B, 8), "time_ids": torch.zeros(B, 1, 6), "metadata": {}}


def _trainer(method, accum=1):
    import importlib
    cfgm = importlib.import_module("sdxl-training-improvements_amd.config")
    T = importlib.import_module("sdxl-training-improvements_amd.trainer")
    cfg = cfgm.Config()
    cfg.training.method = method
    cfg.training.gradient_accumulation_steps = accum
    net = FakeNet()
    class M:
        unet = net
    return T.NativeSDXLTrainer(M(), optimizer=None, train_dataloader=None, device="cpu", config=cfg), net, T


def test_trainer_plugin_contract():
    tr, net, T = _trainer("ddpm")
    with pytest.raises(ValueError, match="missing required keys"):
        tr.compute_loss({"vae_latents": torch.zeros(1, 4, 8, 8)})
    out = tr.compute_loss(_batch())
    assert set(out) == {"loss", "metrics"} and out["loss"].dim() == 0 and out["loss"].requires_grad
    assert set(out["metrics"]) == {"loss", "lr", "timestep_mean", "timestep_std", "noise_scale", "pred_scale", "batch_size"}
    assert set(tr.compute_loss(_batch(1))["metrics"]) == {"loss", "lr", "timestep_mean", "noise_scale", "pred_scale", "batch_size"}
    tr2, net2, _ = _trainer("flow_matching")
    m = tr2.compute_loss(tr2.model, _batch(), torch.Generator().manual_seed(0))["metrics"]   # FM signature (model, batch, generator)
    assert set(m) == {"loss", "x0_norm", "x1_norm", "time_mean", "time_std", "velocity_norm", "batch_size", "lr"}
    assert m["x0_norm"] == 3.0 and m["x1_norm"] == 5.0 and m["velocity_norm"] == 4.0
    with pytest.raises(ValueError, match="Unsupported training method"):
        _trainer("dreambooth")
    with pytest.raises(TypeError):
        T.NativeSDXLTrainer(object(), config=tr.config)


def test_accumulation_semantics_d9_d10():
    """zero_grad at the START of a cycle, backward scale 1/N on every micro-step, first_micro only on the first."""
    tr, net, _ = _trainer("ddpm", accum=4)
    for i in range(8):
        loss, _m = tr._execute_training_step(_batch(), accumulate=True, is_last_accumulation_step=(i + 1) % 4 == 0)
        assert abs(float(loss) - 0.5) < 1e-6                 # unscaled loss is returned for logging
    zeros = [i for i, c in enumerate(net.calls) if c[0] == "zero"]
    bwds = [c for c in net.calls if c[0] == "bwd"]
    assert len(zeros) == 2 and len(bwds) == 8
    assert [b[2] for b in bwds] == [True, False, False, False] * 2 and all(b[1] == 0.25 for b in bwds)
    assert net.calls[0] == ("zero",) and net.calls[zeros[1] - 1][0] == "bwd"


def test_counted_vmcnt_attention_kernels_spill_nothing(tmp_path):
    """csrc/attention_bwd_pl.hip (product) and csrc/attention_pl.hip (diagnostics build) order their LDS-DMA tiles by COUNTED s_waitcnt vmcnt(N).
    A register spilled to scratch is a vector-memory store / load the author did not count, and stores complete out of order with loads: with 24
    spilled registers the dQ body read tiles that had not landed (wrong dQ on every shape, round 6).  hipcc's resource report for gfx950 must say
    ScratchSize 0 and 0 spilled VGPRs for every kernel of the two files (cross-compiles without a GPU, ~20 s)."""
    import re
    import shutil
    import subprocess
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    csrc = ROOT / "sdxl-training-improvements_amd" / "csrc"
    for src, defs in (("attention_bwd_pl.hip", []), ("attention_pl.hip", ["-DSDXL_DIAG"])):
        r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wno-pass-failed", "-Rpass-analysis=kernel-resource-usage",
                            "-c", str(csrc / src), "-o", str(tmp_path / (src + ".o"))] + defs, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stderr)]
        spills = [int(x) for x in re.findall(r"VGPRs Spill: (\d+)", r.stderr)]
        assert scratch and spills, r.stderr[-2000:]
        assert all(x == 0 for x in scratch) and all(x == 0 for x in spills), (src, scratch, spills)
