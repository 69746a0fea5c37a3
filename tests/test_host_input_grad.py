"""Input gradients (sdxl_batch_din) without a GPU: the float64 reference tests/_input_grad_ref.py against autograd of conv2d, the header's
struct and flag against lib.py, the hooks' listing, the structs NativeUNet builds on a recording library, the autograd function
(NativeUNet.differentiable) and the trainer's input_cond plumbing on stand-in nets, and the hook's argument errors."""
import ctypes as C
import importlib
import re
import shutil
import subprocess
from pathlib import Path

import pytest
import torch
import torch.nn.functional as F

import sdxl_amd  # noqa: F401
from sdxl_amd import lib
from sdxl_amd import unet as NU

import _input_grad_ref as IR

ROOT = Path(__file__).resolve().parent.parent
HDR = (ROOT / "include" / "sdxlstep.h").read_text()
DIAG = (ROOT / "include" / "sdxlstep_diag.h").read_text()
HOOKS = ("sdxl_op_input_dgrad", "sdxl_debug_input_dgrad_operands")


# ---------------------------------------------------------------------------------------------- 1. the reference against autograd
REF_CASES = [(1, 1, 1, 4, 32), (2, 3, 5, 9, 32), (2, 1, 7, 8, 64), (2, 6, 1, 16, 32), (1, 13, 19, 5, 96)]      # B = 2: the sample border; H or W = 1


@pytest.mark.parametrize("B,H,W,cin,cout", REF_CASES, ids=["-".join(map(str, c)) for c in REF_CASES])
def test_reference_is_autograd_of_conv2d(B, H, W, cin, cout):
    g = torch.Generator().manual_seed(B * 100 + H)
    x = torch.randn(B, cin, H, W, generator=g, dtype=torch.float64, requires_grad=True)
    wn = torch.randn(cout, cin, 3, 3, generator=g, dtype=torch.float64)
    dy = torch.randn(B, cout, H, W, generator=g, dtype=torch.float64)
    want, = torch.autograd.grad(F.conv2d(x, wn, padding=1), x, dy)
    w = IR.arena_weight(wn)
    assert tuple(w.shape) == (cout, 9, IR.input_cs(cin)) and int(w[:, :, cin:].ne(0).sum()) == 0
    got = IR.input_dgrad_ref64(dy.permute(0, 2, 3, 1).reshape(B * H * W, cout), w, B, H, W, cin)
    assert got.dtype == torch.float64 and tuple(got.shape) == (B, cin, H, W)
    assert torch.allclose(got, want, rtol=1e-12, atol=1e-12)
    # the sample border: sample 1's gradient does not see sample 0's dy
    if B == 2:
        dy2 = dy.clone()
        dy2[0] += 1.0
        again = IR.input_dgrad_ref64(dy2.permute(0, 2, 3, 1).reshape(B * H * W, cout), w, B, H, W, cin)
        assert torch.equal(again[1], got[1]) and not torch.equal(again[0], got[0])


def test_integer_operands_stay_exact_in_fp32():
    dy, w = IR.operands(2, 13, 19, 9, 320, integer=True)
    assert set(dy.unique().tolist()) <= {-2.0, -1.0, 0.0, 1.0, 2.0} and int(w[:, :, 9:].ne(0).sum()) == 0
    bound = IR.input_dgrad_ref64(dy, w, 2, 13, 19, 9, absolute=True)
    assert float(bound.max()) <= 4 * 9 * 320 < 2 ** 24
    ref = IR.input_dgrad_ref64(dy, w, 2, 13, 19, 9)
    assert torch.equal(ref, ref.round()) and torch.equal(ref.float().double(), ref)


# ---------------------------------------------------------------------------------------------- 2. the header against lib.py
def test_struct_layout_and_flag_match_the_header(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang") or "/opt/rocm/lib/llvm/bin/clang"
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "sdxlstep.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %d\\n", sizeof(sdxl_batch_res), sizeof(sdxl_batch_din), offsetof(sdxl_batch_din, d_input), '
                   'offsetof(sdxl_batch_res, residuals), SDXL_BATCH_DIN); return 0; }\n')
    exe = tmp_path / "layout"
    r = subprocess.run([cc, "-I", str(ROOT / "include"), str(src), "-o", str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    out = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True, timeout=60).stdout.split()]
    G = lib.InputGradBatch
    assert out == [C.sizeof(lib.ResidualBatch), C.sizeof(G), G.d_input.offset, lib.ResidualBatch.residuals.offset, lib.BATCH_DIN]
    assert G.d_input.offset == lib.ResidualBatch.residuals.offset + 8      # directly behind `residuals`
    assert issubclass(G, lib.ResidualBatch) and [f[0] for f in G._fields_] == ["d_input"]
    assert lib.BATCH_DIN == 0x80000 and lib.BATCH_DIN & (lib.BATCH_EXT | lib.BATCH_COND | lib.BATCH_RES) == 0 and lib.BATCH_DIN & 0xFFFF == 0
    b = G(2, 8, 8, 77 | lib.BATCH_DIN)
    assert b.d_input is None and not b.residuals and (b.input_cond, b.cond_channels, b.d_prompt_embeds, b.d_pooled) == (None, 0, None, None)
    assert C.sizeof(G) == C.sizeof(lib.ResidualBatch) + 8


def test_no_new_entry_point_and_the_hooks_are_test_hooks():
    assert HDR.count("SDXL_API int ") + HDR.count("SDXL_API const char* ") <= 58
    assert len(set(re.findall(r"\b(sdxl_[a-z0-9_]+)\s*\(", HDR))) <= 58
    for name in HOOKS:
        assert name in lib.TEST_HOOK_SIGNATURES and name not in lib.SIGNATURES and name not in lib.DIAG_SIGNATURES
        assert re.search(rf"SDXL_API int {name}\(", DIAG) and DIAG.index(name) < DIAG.index("part 2: experiment ABI")
        assert hasattr(lib.load(), name)
    assert len(lib.TEST_HOOK_SIGNATURES["sdxl_op_input_dgrad"]) == 10
    # the sentences that said there is no such gradient are gone
    docs = HDR + (ROOT / "INTEGRATION.md").read_text() + (ROOT / "DESIGN.md").read_text()
    assert "has no input gradient" not in docs and "no gradient with respect to" not in docs and "d(sample) is not produced" not in docs


def test_hook_refuses_bad_arguments_before_any_device_call():
    L = lib.load()
    buf = (C.c_float * 64)()
    p = C.addressof(buf)
    p += -p % 16
    ok = (p, p, p, None, 1, 4, 4, 4, 32)
    for i, v, msg in ((0, None, b"non-NULL"), (1, None, b"non-NULL"), (2, None, b"non-NULL"), (0, p + 8, b"aligned"), (2, p + 4, b"aligned"),
                      (4, 0, b"B = 0"), (5, 0, b"H = 0"), (6, -1, b"W = -1"), (7, 0, b"in_channels = 0"), (7, 17, b"in_channels = 17"),
                      (8, 48, b"multiple of 32"), (8, 0, b"multiple of 32")):
        args = list(ok)
        args[i] = v
        assert L.sdxl_op_input_dgrad(*args, None) == 1 and msg in L.sdxl_last_error() and b"input_dgrad" in L.sdxl_last_error(), (i, v)
    assert L.sdxl_debug_input_dgrad_operands(None, None, None, None) == 1


# ---------------------------------------------------------------------------------------------- 3. NativeUNet on a recording library
class RecL:
    def __init__(self):
        self.calls = []

    def sdxl_forward_loss(self, h, lc, b, st):
        self.calls.append(("forward_loss", b._obj))
        return 0

    def sdxl_unet_forward(self, h, sample, b, pred, st):
        self.calls.append(("unet_forward", b._obj))
        return 0


def _rec_net(monkeypatch, in_channels=4):
    net = object.__new__(NU.NativeUNet)
    net.L, net.h, net.device = RecL(), None, torch.device("cpu")
    net.cfg = NU.make_config(in_channels=in_channels, block_out_channels=(64, 128, 256))
    net._keep, net._cur = [], None
    net.plan = lambda *a: None
    monkeypatch.setattr(NU, "_stream", lambda: None)
    return net


def _inputs(B=2, H=8, W=12):
    g = torch.Generator().manual_seed(0)
    r = lambda *s: torch.randn(*s, generator=g)
    return dict(lat=r(B, 4, H, W), noise=r(B, 4, H, W), t=torch.rand(B, generator=g), ehs=r(B, 77, 16), pooled=r(B, 8), tid=torch.zeros(B, 6))


def _fwd(net, x, **kw):
    net.forward_loss("flow_matching", x["lat"], x["noise"], x["t"], x["t"], x["ehs"], x["pooled"], x["tid"], **kw)
    return net.L.calls[-1][1]


def test_without_the_request_the_structs_are_todays(monkeypatch):
    net = _rec_net(monkeypatch)
    x = _inputs()
    b = _fwd(net, x)
    assert type(b) is lib.Batch and b.ctx_len == 77 and net.read_input_grad() is None
    assert type(_fwd(net, x, input_grad=False)) is lib.Batch
    assert type(_fwd(net, x, cond_grads=True)) is lib.CondGradBatch
    assert type(_fwd(net, x, residual_grads=True)) is lib.ResidualBatch
    net.unet_forward(x["lat"], x["t"], x["ehs"], x["pooled"], x["tid"])
    assert type(net.L.calls[-1][1]) is lib.SamplerBatch and net.L.calls[-1][1].ctx_len == 77 and net.read_input_grad() is None
    net9 = _rec_net(monkeypatch, 9)
    assert type(_fwd(net9, x, input_cond=torch.zeros(2, 5, 8, 12))) is lib.InputCondBatch


def test_the_request_builds_the_flagged_struct(monkeypatch):
    net = _rec_net(monkeypatch, 9)
    x = _inputs()
    ic = torch.zeros(2, 5, 8, 12)
    b = _fwd(net, x, input_cond=ic, input_grad=True, cond_grads=("pooled",))
    d = net.read_input_grad()
    assert type(b) is lib.InputGradBatch and b.ctx_len == 77 | lib.BATCH_EXT | lib.BATCH_COND | lib.BATCH_DIN
    assert tuple(d.shape) == (2, 9, 8, 12) and d.dtype == torch.float32 and b.d_input == d.data_ptr() != 0 and d.data_ptr() % 16 == 0
    assert b.input_cond and b.cond_channels == 5 and b.d_pooled and not b.d_prompt_embeds and not b.residuals and not b.sampler
    # with residual gradients: the residuals pointer travels
    b = _fwd(net, x, input_cond=ic, input_grad=True, residual_grads=[0])
    assert type(b) is lib.InputGradBatch and b.ctx_len == 77 | lib.BATCH_COND | lib.BATCH_RES | lib.BATCH_DIN
    assert b.residuals and b.residuals.contents.n == 9 and b.residuals.contents.d_down[0] == net.read_residual_grads()[0][0].data_ptr()
    # the next call without the request forgets the buffer
    _fwd(net, x, input_cond=ic)
    assert net.read_input_grad() is None
    # unet_forward
    net.unet_forward(torch.zeros(2, 9, 8, 12), x["t"], x["ehs"], x["pooled"], x["tid"], input_grad=True)
    b = net.L.calls[-1][1]
    assert type(b) is lib.InputGradBatch and b.ctx_len == 77 | lib.BATCH_DIN and not b.sampler and b.d_input == net.read_input_grad().data_ptr()


def test_every_forward_counts(monkeypatch):
    net = _rec_net(monkeypatch)
    x = _inputs()
    _fwd(net, x)
    g0 = net._fwd_gen
    _fwd(net, x, input_grad=True)
    net.unet_forward(x["lat"], x["t"], x["ehs"], x["pooled"], x["tid"])
    assert net._fwd_gen == g0 + 2


# ---------------------------------------------------------------------------------------------- 4. the autograd function
class FnNet:
    """what _UNetFunction needs of a net: records the calls and hands out marked gradients"""
    device = torch.device("cpu")
    first_micro = True

    def __init__(self, n_skips=9):
        self.calls, self._fwd_gen, self.n = [], 0, n_skips

    def unet_forward(self, sample, timestep, prompt_embeds, pooled, time_ids, **kw):
        assert not any(t.requires_grad for t in (sample, prompt_embeds, pooled))
        self._fwd_gen += 1
        self.calls.append(("fwd", kw))
        self.kw, self.shape = kw, (tuple(sample.shape), tuple(prompt_embeds.shape), tuple(pooled.shape))
        return sample[:, :4] * 2.0

    def unet_backward(self, dpred, first_micro=True):
        self.calls.append(("bwd", dpred.clone(), first_micro))

    def read_input_grad(self):
        return torch.full(self.shape[0], 1.0) if self.kw.get("input_grad") else None

    def read_cond_grads(self):
        want = self.kw.get("cond_grads") or ()
        return (torch.full(self.shape[1], 2.0) if "prompt" in want else None, torch.full(self.shape[2], 3.0) if "pooled" in want else None)

    def read_residual_grads(self):
        want = self.kw.get("residual_grads")
        if not want:
            return None, None
        down, mid = self.kw["residuals"]
        return [torch.full(t.shape, 10.0 + i) if i in want else None for i, t in enumerate(down)], torch.full(mid.shape, 99.0) if "mid" in want else None


def _fn_inputs(dtype=torch.float32):
    g = torch.Generator().manual_seed(1)
    r = lambda *s: torch.randn(*s, generator=g).to(dtype)
    return r(2, 4, 8, 8), torch.tensor([10.0, 500.0]), r(2, 77, 16), r(2, 8), torch.zeros(2, 6)


def test_differentiable_routes_each_gradient_to_its_input():
    net = FnNet()
    s, t, e, p, ti = _fn_inputs(torch.float64)
    for x in (s, e, p):
        x.requires_grad_(True)
    down = [torch.zeros(2, 3, 4, 4) for _ in range(9)]
    down[2].requires_grad_(True)
    down[5] = None
    mid = torch.zeros(2, 3, 2, 2, dtype=torch.bfloat16, requires_grad=True)
    pred = NU.NativeUNet.differentiable(net, s, t, e, p, ti, residuals=(down, mid))
    assert tuple(pred.shape) == (2, 4, 8, 8) and pred.requires_grad
    kw = net.calls[-1][1]
    assert kw["input_grad"] is True and kw["cond_grads"] == ("prompt", "pooled") and kw["residual_grads"] == [2, "mid"]
    assert kw["residuals"][0][5] is None and all(r.dtype == torch.float32 and not r.requires_grad for r in kw["residuals"][0] if r is not None)
    dpred = torch.randn(2, 4, 8, 8, dtype=pred.dtype)
    pred.backward(dpred)
    assert net.calls[-1][0] == "bwd" and torch.equal(net.calls[-1][1], dpred) and net.calls[-1][2] is True
    for x, v in ((s, 1.0), (e, 2.0), (p, 3.0)):      # each in the input's own dtype and shape
        assert x.grad.dtype == torch.float64 and x.grad.shape == x.shape and bool((x.grad == v).all())
    assert bool((down[2].grad == 12.0).all()) and down[0].grad is None
    assert mid.grad.dtype == torch.bfloat16 and bool((mid.grad == 99.0).all())
    # only what requires grad is asked for; first_micro is the net's attribute
    net.first_micro = False
    s2, t, e2, p2, ti = _fn_inputs()
    p2.requires_grad_(True)
    NU.NativeUNet.differentiable(net, s2, t, e2, p2, ti).sum().backward()
    assert net.calls[-2][1] == {"cond_grads": ("pooled",)} and net.calls[-1][2] is False
    assert bool((p2.grad == 3.0).all()) and s2.grad is None and e2.grad is None


def test_differentiable_refuses_the_backward_of_a_stale_forward():
    net = FnNet()
    s, t, e, p, ti = _fn_inputs()
    s.requires_grad_(True)
    first = NU.NativeUNet.differentiable(net, s, t, e, p, ti)
    second = NU.NativeUNet.differentiable(net, s, t, e, p, ti)
    n = len(net.calls)
    with pytest.raises(lib.SdxlError, match="stale forward"):
        first.sum().backward()
    assert len(net.calls) == n and s.grad is None      # nothing ran: the wrong activations are never differentiated
    second.sum().backward()
    assert net.calls[-1][0] == "bwd" and bool((s.grad == 1.0).all())


# ---------------------------------------------------------------------------------------------- 5. the trainer
class FakeNet:
    param_elems = 16
    device = "cpu"
    cfg = {"in_channels": 8}

    def __init__(self):
        self.calls = []
        self.grads = torch.zeros(16)
        self.weights = torch.zeros(16, dtype=torch.bfloat16)

    def zero_grads(self):
        self.calls.append(("zero",))

    def forward_loss(self, method, *a, **k):
        self.calls.append(("fwd", method, a, k))
        self.k = k

    def backward(self, scale, first, on_segment=None):
        self.calls.append(("bwd", scale, first))

    def read_loss(self):
        return [0.5, 0, 8.0, 16.0, 4.0, 9.0, 25.0, 1.0]

    def read_input_grad(self):
        self.calls.append(("read_din",))
        ic = self.k["input_cond"]
        B, n, H, W = ic.shape
        return torch.arange(B * (4 + n) * H * W, dtype=torch.float32).reshape(B, 4 + n, H, W)

    def grad_norm(self):
        return 0.0


def _trainer(**keys):
    cfgm = importlib.import_module("sdxl-training-improvements_amd.config")
    T = importlib.import_module("sdxl-training-improvements_amd.trainer")
    cfg = cfgm.Config()
    cfg.training.method = "flow_matching"
    cfg.training.input_conditioning = "concat"
    for k, v in keys.items():
        setattr(cfg.training, k, v)
    net = FakeNet()

    class M:
        unet = net
    return T.NativeSDXLTrainer(M(), optimizer=None, train_dataloader=None, device="cpu", config=cfg), net


def _batch(cond):
    g = torch.Generator().manual_seed(5)
    return {"vae_latents": torch.randn(2, 4, 8, 8, generator=g), "prompt_embeds": torch.randn(2, 77, 16, generator=g),
            "pooled_prompt_embeds": torch.randn(2, 8, generator=g), "time_ids": torch.zeros(2, 1, 6), "cond_latents": cond, "metadata": {}}


def test_trainer_asks_for_nothing_when_input_cond_needs_no_grad():
    tr, net = _trainer()
    tr.compute_loss(_batch(torch.ones(2, 4, 8, 8)))["loss"].backward()
    k = next(c for c in net.calls if c[0] == "fwd")[3]
    assert "input_grad" not in k and ("read_din",) not in net.calls and not k["input_cond"].requires_grad
    # under no_grad an encoder's output is not tracked either
    enc = torch.nn.Conv2d(3, 4, 1)
    with torch.no_grad():
        tr.compute_loss(_batch(enc(torch.ones(2, 3, 8, 8))))
    assert "input_grad" not in [c for c in net.calls if c[0] == "fwd"][-1][3]


@pytest.mark.parametrize("world", [1, 2])
def test_trainer_hands_channels_4_on_times_world_to_input_cond(world):
    tr, net = _trainer()
    tr.sync.world = world
    torch.manual_seed(3)
    enc = torch.nn.Conv2d(3, 4, 3, padding=1)
    src = torch.randn(2, 3, 8, 8, generator=torch.Generator().manual_seed(6))
    cond = enc(src)
    out = tr.compute_loss(_batch(cond), timesteps=torch.tensor([0.25, 0.75]))
    k = next(c for c in net.calls if c[0] == "fwd")[3]
    assert k["input_grad"] is True and not k["input_cond"].requires_grad and torch.equal(k["input_cond"], cond.detach())
    (out["loss"] / 4).backward()
    assert ("bwd", 0.25 / world, True) in net.calls and net.calls[-1] == ("read_din",)
    d = torch.arange(2 * 8 * 8 * 8, dtype=torch.float32).reshape(2, 8, 8, 8)[:, 4:] * world
    gw, gb = torch.autograd.grad(enc(src), [enc.weight, enc.bias], d)
    assert torch.allclose(enc.weight.grad, gw, rtol=1e-5, atol=1e-4) and torch.allclose(enc.bias.grad, gb, rtol=1e-5, atol=1e-4)


def test_trainer_dropout_zeroes_the_dropped_samples_gradient():
    tr, net = _trainer(input_cond_dropout_prob=1.0)
    cond = torch.ones(2, 4, 8, 8, requires_grad=True)
    tr.compute_loss(_batch(cond), generator=torch.Generator().manual_seed(0))["loss"].backward()
    k = next(c for c in net.calls if c[0] == "fwd")[3]
    assert k["input_grad"] is True and int(k["input_cond"].ne(0).sum()) == 0
    assert cond.grad is not None and int(cond.grad.ne(0).sum()) == 0      # the dropped samples read zeros: nothing flows back
