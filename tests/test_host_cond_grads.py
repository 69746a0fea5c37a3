"""Conditioning gradients without a GPU: the struct appended behind sdxl_batch, its argument error, the trainer's autograd plumbing
on a fake net, and the resource report of csrc/cond_dgrad.hip."""
import ctypes as C
import importlib
import re
import shutil
import subprocess
from pathlib import Path

import pytest
import torch

import sdxl_amd  # noqa: F401
from sdxl_amd import lib

ROOT = Path(__file__).resolve().parent.parent


def test_struct_layout_matches_the_header(tmp_path):
    """a three-line C program against include/sdxlstep.h: sizeof(sdxl_batch_ext) and the two fields' offsets are lib.CondGradBatch's;
    sdxl_batch itself (what every caller without the flag passes) is unchanged"""
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang") or "/opt/rocm/lib/llvm/bin/clang"
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "sdxlstep.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %d\\n", sizeof(sdxl_batch), sizeof(sdxl_batch_ext), '
                   'offsetof(sdxl_batch_ext, d_prompt_embeds), offsetof(sdxl_batch_ext, d_pooled), SDXL_BATCH_EXT); return 0; }\n')
    exe = tmp_path / "layout"
    r = subprocess.run([cc, "-I", str(ROOT / "include"), str(src), "-o", str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True, timeout=60).stdout.split()
    assert [int(v) for v in out] == [C.sizeof(lib.SamplerBatch), C.sizeof(lib.CondGradBatch), lib.CondGradBatch.d_prompt_embeds.offset,
                                     lib.CondGradBatch.d_pooled.offset, lib.BATCH_EXT]
    assert issubclass(lib.CondGradBatch, lib.SamplerBatch) and lib.CondGradBatch.d_prompt_embeds.offset == C.sizeof(lib.SamplerBatch)
    assert [f[0] for f in lib.CondGradBatch._fields_] == ["d_prompt_embeds", "d_pooled"]
    assert "sdxl_op_cond_dgrad" in lib.TEST_HOOK_SIGNATURES and "sdxl_op_cond_dgrad" not in lib.SIGNATURES


def test_gradient_pointer_with_a_sampler_is_a_bad_argument_before_any_device_call():
    L = lib.load()
    buf = (C.c_float * 4)()
    s = lib.SamplerStep(C.addressof(buf), 0, 0, 0.5, -2.0, 0.25, 0.75, 1.0, 0.0, 1.0, 0.0)
    for field in ("d_prompt_embeds", "d_pooled"):
        b = lib.CondGradBatch(1, 8, 8, 77 | lib.BATCH_EXT, None, None, None, None, None, None, None, None)
        b.sampler = C.pointer(s)
        setattr(b, field, C.addressof(buf))
        # (no handle, no device: the combination is rejected before either is looked at)
        assert L.sdxl_unet_forward(None, None, C.byref(b), None, None) == 1 and b"sampler" in L.sdxl_last_error(), field
        lc = lib.LossConfig(1, 1, 0, 0.0, 0, 0, 0.0)
        assert L.sdxl_forward_loss(None, C.byref(lc), C.byref(b), None) == 1 and b"sampler" in L.sdxl_last_error(), field
    # without the flag nothing behind `sampler` is read: the null handle is what is reported
    b = lib.CondGradBatch(1, 8, 8, 77, None, None, None, None, None, None, None, None)
    b.sampler = C.pointer(s)
    b.d_pooled = C.addressof(buf)
    assert L.sdxl_unet_forward(None, None, C.byref(b), None, None) == 1 and b"null handle" in L.sdxl_last_error()
    # the hook's own argument errors
    p = (C.c_void_p * 1)(C.addressof(buf))
    one, k = (C.c_long * 1)(64), (C.c_int * 1)(48)
    assert L.sdxl_op_cond_dgrad(1, p, one, p, one, k, C.addressof(buf), 8, 1, 8, None) == 1 and b"multiple of 64" in L.sdxl_last_error()
    assert L.sdxl_op_cond_dgrad(3, p, one, p, one, k, C.addressof(buf), 8, 1, 8, None) == 1


class FakeNet:
    """records what the trainer asks of the native UNet; returns fixed conditioning gradients"""
    param_elems = 16
    device = "cpu"

    def __init__(self):
        self.calls = []
        self.grads = torch.zeros(16)
        self.weights = torch.zeros(16, dtype=torch.bfloat16)
        self.d = (torch.arange(2 * 77 * 16, dtype=torch.float32).reshape(2, 77, 16) / 7, torch.arange(16, dtype=torch.float32).reshape(2, 8) - 3)

    def zero_grads(self):
        self.calls.append(("zero",))

    def forward_loss(self, method, *a, **k):
        self.calls.append(("fwd", method, a, k))

    def backward(self, scale, first, on_segment=None):
        self.calls.append(("bwd", scale, first))

    def read_loss(self):
        return [0.5, 0, 8.0, 16.0, 4.0, 9.0, 25.0, 1.0]

    def read_per_sample_loss(self):
        return torch.zeros(2)

    def read_cond_grads(self):
        self.calls.append(("read_cond",))
        return self.d

    def grad_norm(self):
        return 0.0


def _trainer(**keys):
    cfgm = importlib.import_module("sdxl-training-improvements_amd.config")
    T = importlib.import_module("sdxl-training-improvements_amd.trainer")
    cfg = cfgm.Config()
    cfg.training.method = "flow_matching"
    for k, v in keys.items():
        setattr(cfg.training, k, v)
    net = FakeNet()

    class M:
        unet = net
    return T.NativeSDXLTrainer(M(), optimizer=None, train_dataloader=None, device="cpu", config=cfg), net


def _batch(requires_grad=()):
    b = {"vae_latents": torch.randn(2, 4, 8, 8), "prompt_embeds": torch.randn(2, 77, 16), "pooled_prompt_embeds": torch.randn(2, 8),
         "time_ids": torch.zeros(2, 1, 6), "metadata": {}}
    for k in requires_grad:
        b[k].requires_grad_(True)
    return b


def _fwd_kwargs(net):
    return [c[3] for c in net.calls if c[0] == "fwd"]


def test_inputs_without_requires_grad_make_no_new_call():
    tr, net = _trainer()
    out = tr.compute_loss(_batch())
    out["loss"].backward()
    assert all("cond_grads" not in k for k in _fwd_kwargs(net)) and ("read_cond",) not in net.calls
    assert [c[0] for c in net.calls] == ["fwd", "zero", "bwd"]


def test_requires_grad_asks_and_hands_the_gradients_back():
    tr, net = _trainer()
    b = _batch(("prompt_embeds", "pooled_prompt_embeds"))
    (tr.compute_loss(b)["loss"] / 4).backward()
    assert _fwd_kwargs(net)[0]["cond_grads"] == ("prompt", "pooled")
    fwd = next(c for c in net.calls if c[0] == "fwd")
    assert not fwd[2][4].requires_grad and not fwd[2][5].requires_grad      # the net gets detached tensors
    assert ("bwd", 0.25, True) in net.calls and net.calls[-1] == ("read_cond",)
    assert torch.equal(b["prompt_embeds"].grad, net.d[0]) and torch.equal(b["pooled_prompt_embeds"].grad, net.d[1])
    # only the tensor that requires grad is asked for; dtype and device follow the input
    tr, net = _trainer()
    b = _batch()
    b["pooled_prompt_embeds"] = b["pooled_prompt_embeds"].double().requires_grad_(True)
    tr.compute_loss(b)["loss"].backward()
    assert _fwd_kwargs(net)[0]["cond_grads"] == ("pooled",)
    assert b["pooled_prompt_embeds"].grad.dtype == torch.float64 and torch.equal(b["pooled_prompt_embeds"].grad, net.d[1].double())
    assert b["prompt_embeds"].grad is None


def test_no_grad_evaluate_and_off_never_ask():
    tr, net = _trainer()
    with torch.no_grad():
        tr.compute_loss(_batch(("prompt_embeds",)))
    assert all("cond_grads" not in k for k in _fwd_kwargs(net))
    tr, net = _trainer()
    tr.evaluate([_batch(("prompt_embeds", "pooled_prompt_embeds"))], [0.25, 0.75], generator=torch.Generator().manual_seed(0))
    assert len(_fwd_kwargs(net)) == 2 and all("cond_grads" not in k for k in _fwd_kwargs(net)) and ("read_cond",) not in net.calls
    tr, net = _trainer(conditioning_grads="off")
    b = _batch(("prompt_embeds", "pooled_prompt_embeds"))
    tr.compute_loss(b)["loss"].backward()
    assert all("cond_grads" not in k for k in _fwd_kwargs(net)) and b["prompt_embeds"].grad is None


def test_dropped_samples_get_zero_rows_from_autograd():
    tr, net = _trainer(cond_dropout_prob=1.0)
    b = _batch(("prompt_embeds", "pooled_prompt_embeds"))
    tr.compute_loss(b, generator=torch.Generator().manual_seed(1))["loss"].backward()
    fwd = next(c for c in net.calls if c[0] == "fwd")
    assert int(fwd[2][4].ne(0).sum()) == 0 and int(fwd[2][5].ne(0).sum()) == 0      # the UNet saw zeros
    assert int(b["prompt_embeds"].grad.ne(0).sum()) == 0 and int(b["pooled_prompt_embeds"].grad.ne(0).sum()) == 0
    # with the key off the dropout path is the old one (a modified copy), and nothing requires grad downstream
    tr, net = _trainer(cond_dropout_prob=1.0, conditioning_grads="off")
    tr.compute_loss(_batch(("prompt_embeds",)), generator=torch.Generator().manual_seed(1))
    assert all("cond_grads" not in k for k in _fwd_kwargs(net))


def test_unknown_value_of_the_key_raises():
    for bad in ("on", "prompt", 1, None):
        with pytest.raises(ValueError, match="conditioning_grads"):
            _trainer(conditioning_grads=bad)
    _trainer(conditioning_grads="AUTO")


def test_drop_in_copies_the_key():
    cfgm = importlib.import_module("sdxl-training-improvements_amd.config")
    assert cfgm.TrainingConfig().conditioning_grads == "auto"


def test_cond_dgrad_kernels_use_no_scratch(tmp_path):
    """hipcc's resource report of csrc/cond_dgrad.hip for gfx950: ScratchSize 0 and 0 spilled VGPRs for every kernel (all five row-tile
    instantiations and the reduce); cross-compiles without a GPU"""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    src = ROOT / "sdxl-training-improvements_amd" / "csrc" / "cond_dgrad.hip"
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wno-pass-failed", "-Rpass-analysis=kernel-resource-usage",
                        "-c", str(src), "-o", str(tmp_path / "cond_dgrad.o")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    names = re.findall(r"Function Name: (\S+)", r.stderr)
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stderr)]
    spills = [int(x) for x in re.findall(r"VGPRs Spill: (\d+)", r.stderr)]
    assert len([n for n in names if "cond_dgrad_kernel" in n]) == 5 and any("reduce" in n for n in names), names
    assert len(scratch) == len(names) and len(spills) == len(names)
    assert all(x == 0 for x in scratch) and all(x == 0 for x in spills), (names, scratch, spills)
