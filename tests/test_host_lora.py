"""LoRA by merge and project, the parts that need no GPU: the merge restatement's exactness properties, the identity the design rests on
(LoRA gradients = projections of the merged weight's gradient) on the oracle UNet, the adapter arena's layout, the export's keys, the
C boundary (no new function, struct mirrors, argument errors before any launch) and every ValueError of the trainer."""
import ctypes as C
import importlib
import re
import shutil
import subprocess
from pathlib import Path
from types import SimpleNamespace

import pytest
import torch

import sdxl_amd  # noqa: F401
from oracle import unet_ref as U
from sdxl_amd import lib

import _lora_ref as LR

ROOT = Path(__file__).resolve().parent.parent
CFG = importlib.import_module("sdxl-training-improvements_amd.config")
T = importlib.import_module("sdxl-training-improvements_amd.trainer")
LORA = importlib.import_module("sdxl-training-improvements_amd.lora")

bf = lambda t: t.to(torch.bfloat16)


class StandInNet:
    """the tiny UNet's parameter table on the CPU: what LoRAAdapters and the trainer ask of a net, without libsdxlstep"""
    device = "cpu"
    L = None
    h = None

    def __init__(self):
        self.cfg = U.tiny_config()
        self.shapes = {k: tuple(int(x) for x in v) for k, v in U.param_shapes(self.cfg).items()}
        self.ranges, cur = {}, 0
        for k, s in self.shapes.items():
            n = 1
            for x in s:
                n *= x
            self.ranges[k] = (cur, n)
            cur = (cur + n + 63) // 64 * 64
        self.param_elems = cur
        self.weights = bf(torch.randn(cur, generator=torch.Generator().manual_seed(1)) * 0.05)
        self.grads = torch.zeros(cur)

    def param_shapes(self):
        return dict(self.shapes)

    def param_ranges(self):
        return dict(self.ranges)

    def zero_grads(self):
        pass

    def forward_loss(self, *a, **k):
        pass

    def backward(self, *a, **k):
        pass

    def read_loss(self):
        return [0.5, 0, 8.0, 16.0, 4.0, 9.0, 25.0, 1.0]


@pytest.fixture(scope="module")
def net():
    return StandInNet()


def test_merge_restatement_returns_w0_for_zero_b_and_zero_scale():
    g = torch.Generator().manual_seed(0)
    W0 = bf(torch.randn(40, 24, generator=g))
    W0[0, 0], W0[1, 1] = -0.0, 0.0
    A, B = bf(torch.randn(3, 24, generator=g)), bf(torch.randn(40, 3, generator=g))
    same = lambda x, y: torch.equal(x.view(torch.int16), y.view(torch.int16))
    assert same(LR.merge(W0, A, torch.zeros_like(B), 0.7), W0)
    assert same(LR.merge(W0, A, B, 0.0), W0)
    got = LR.merge(W0, A, B, 0.5)
    assert not same(got, W0)
    ref = bf(W0.double() + 0.5 * (B.double() @ A.double()))       # the separately rounded fp32 chain stays within one bf16 ulp of exact
    assert float((got.double() - ref.double()).abs().max()) <= 2.0 ** -7 * float(ref.double().abs().max())


def test_lora_gradients_are_projections_of_the_merged_weight_gradient():
    """autograd through the oracle UNet with w[k] = W0 + s B A as a function of the leaves A, B: dA = s B^T dW and dB = s dW A^T with the
    dW of the same run.  Every tensor that can be a target (attention projections, ff.net.2, proj_in / proj_out, time_emb_proj, the embedding
    linears), rank 4."""
    cfg = U.tiny_config()
    w = U.synth_weights(cfg, seed=0)
    shapes = {k: tuple(v.shape) for k, v in w.items()}
    targets = LORA.resolve_targets(shapes, list(LORA.DEFAULT_TARGETS) + ["ff.net.2", "proj_in", "proj_out", "time_emb_proj", "linear_1", "linear_2"])
    assert set(targets) == {k for k, v in shapes.items() if len(v) == 2 and "ff.net.0.proj" not in k}      # every plain 2-D linear of the UNet
    r, s = 4, 0.5
    g = torch.Generator().manual_seed(3)
    A = {k: (torch.randn(r, shapes[k][1], generator=g) / r).requires_grad_(True) for k in targets}
    B = {k: (torch.randn(shapes[k][0], r, generator=g) * 0.02).requires_grad_(True) for k in targets}
    wm = dict(w)
    for k in targets:
        wm[k] = w[k] + s * (B[k] @ A[k])
        wm[k].retain_grad()
    Bn, H, W = 1, 8, 8
    x = torch.randn(Bn, 4, H, W, generator=g)
    pred = U.unet_forward(wm, x, torch.tensor([300.0]), torch.randn(Bn, 77, cfg.cross_attention_dim, generator=g),
                          torch.randn(Bn, cfg.pooled_dim, generator=g), torch.tensor([[64.0, 64, 0, 0, 64, 64]]), cfg)
    (pred - torch.randn(pred.shape, generator=g)).square().mean().backward()
    worst = 0.0
    for k in targets:
        dW = wm[k].grad
        assert float(dW.abs().max()) > 0, k
        dA, dB = LR.project64(dW, A[k].detach(), B[k].detach(), s)
        for got, ref in ((A[k].grad, dA), (B[k].grad, dB)):
            worst = max(worst, float((got.double() - ref).norm() / ref.norm()))
    assert worst <= 1e-5, worst


def test_default_targets_on_sdxl_base():
    shapes = {k: tuple(v) for k, v in U.param_shapes(U.SDXL_BASE).items()}
    t = LORA.resolve_targets(shapes, LORA.DEFAULT_TARGETS)
    assert len(t) == 560 and sum(shapes[k][0] * shapes[k][1] for k in t) == 955_187_200
    assert all(k.endswith(".weight") and len(shapes[k]) == 2 for k in t)


def test_adapter_arena_layout_padding_and_init(net):
    ad = LORA.LoRAAdapters(net, rank=3, alpha=1.5, targets=["to_q", "time_emb_proj"], seed=4)
    assert ad.scale == 0.5 and ad.weights.dtype == torch.bfloat16 and ad.grads.dtype == torch.float32
    cur, base = 0, 0
    for k in ad.targets:
        o, i = net.shapes[k]
        a, b, oo, ii = ad.layout[k]
        assert (a, oo, ii) == (cur, o, i) and a % 8 == 0
        cur += (3 * i + 7) // 8 * 8
        assert b == cur and b % 8 == 0
        cur += (o * 3 + 7) // 8 * 8
        off, n = net.ranges[k]
        assert torch.equal(ad.base[base: base + o * i], net.weights[off: off + n])      # W0, packed in target order
        base += o * i
        assert float(ad.B(k).abs().max()) == 0.0 and 0.1 < float(ad.A(k).float().std()) * 3 < 10      # B = 0, A ~ N(0, (1/r)^2)
        pad = ad.weights[b + o * 3: cur]
        assert pad.numel() == (-o * 3) % 8 and float(pad.abs().sum()) == 0.0
    assert cur == ad.param_elems == ad.weights.numel() == ad.grads.numel() and base == ad.base.numel()
    lay, total = LORA.adapter_layout({"x.weight": (130, 264), "y.weight": (1, 8)}, ["x.weight", "y.weight"], 3)      # B of 390 elements: padded to 392
    assert lay == {"x.weight": (0, 792, 130, 264), "y.weight": (792 + 392, 792 + 392 + 24, 1, 8)} and total == 792 + 392 + 24 + 8
    again = LORA.LoRAAdapters(net, rank=3, alpha=1.5, targets=["to_q", "time_emb_proj"], seed=4)
    assert torch.equal(again.weights.view(torch.int16), ad.weights.view(torch.int16))          # seeded
    pr = ad.param_ranges()
    assert len(pr) == 2 * len(ad.targets) and all(off % 8 == 0 and n % 8 == 0 for off, n in pr.values())
    spans = sorted(pr.values())
    assert spans[0][0] == 0 and all(a[0] + a[1] == b[0] for a, b in zip(spans, spans[1:])) and sum(n for _o, n in spans) == ad.param_elems
    # the fused optimizers take it as their net, unchanged
    O = importlib.import_module("sdxl-training-improvements_amd.optimizer")
    for cls in O.BY_TYPE.values():
        opt = cls(ad, lr=1e-3)
        assert opt.exp_avg.numel() == ad.param_elems and opt.net is ad
    with pytest.raises(lib.SdxlError):
        ad.merge()                                                                                # no library behind a stand-in: loud


def test_export_keys_and_state_roundtrip(net):
    ad = LORA.LoRAAdapters(net, rank=4, alpha=2.0, targets=["attn1.to_out.0"], seed=1)
    g = torch.Generator().manual_seed(2)
    for k in ad.targets:
        ad.B(k).copy_(bf(torch.randn(ad.B(k).shape, generator=g) * 0.02))
    ex = ad.export_tensors()
    assert len(ex) == 2 * len(ad.targets)
    for k in ad.targets:
        mod = k[: -len(".weight")]
        la, lb = ex[f"unet.{mod}.lora_A.weight"], ex[f"unet.{mod}.lora_B.weight"]
        assert la.dtype == lb.dtype == torch.float32 and la.shape == (4, net.shapes[k][1]) and lb.shape == (net.shapes[k][0], 4)
        assert torch.equal(la, ad.A(k).float()) and torch.equal(lb, ad.B(k).float() * 0.5)        # s = alpha / rank folded into lora_B
    assert all(re.fullmatch(r"unet\..+\.lora_[AB]\.weight", k) for k in ex)
    sd = ad.state_dict()
    other = LORA.LoRAAdapters(net, rank=4, alpha=2.0, targets=["attn1.to_out.0"], seed=9)
    assert not torch.equal(other.weights, ad.weights)
    other.load_state_dict(sd)
    assert torch.equal(other.weights.view(torch.int16), ad.weights.view(torch.int16))
    for bad in (LORA.LoRAAdapters(net, rank=8, targets=["attn1.to_out.0"]), LORA.LoRAAdapters(net, rank=4, targets=["attn1.to_q"])):
        before = bad.weights.clone()
        with pytest.raises(ValueError, match="lora state"):
            bad.load_state_dict(sd)
        assert torch.equal(bad.weights, before)


def test_target_patterns_that_are_refused(net):
    for pat, msg in (("no_such_module", "matches no tensor"), ("ff.net.0.proj", "interleaved"), ("conv1", "2-D"), ("conv_in", "2-D")):
        with pytest.raises(ValueError, match=msg):
            LORA.resolve_targets(net.shapes, ["to_q", pat])
    for rank in (0, 129, 2.0, True):
        with pytest.raises(ValueError, match="lora_rank"):
            LORA.LoRAAdapters(net, rank=rank)


def _trainer(net, **training):
    cfg = CFG.Config()
    for k, v in training.items():
        setattr(cfg.training, k, v)
    return T.create_trainer(SimpleNamespace(unet=net), config=cfg, device="cpu")


def test_create_trainer_picks_the_lora_trainer_and_refuses_what_it_cannot_do(net):
    plain = _trainer(net)
    assert type(plain) is T.NativeSDXLTrainer and isinstance(plain.sync, T.D.GradSync)
    tr = _trainer(net, lora_rank=4)
    assert isinstance(tr, LORA.NativeLoRATrainer) and tr.lora.rank == 4 and tr.lora.scale == 1.0
    assert tr.lora.patterns == LORA.DEFAULT_TARGETS and tr.optimizer.net is tr.lora
    assert tr.optimizer.exp_avg.numel() == tr.lora.param_elems < net.param_elems                 # no full-model optimizer state
    assert tr.sync.comm is None and not tr.sync.active and tr.ema is None
    assert _trainer(net, lora_rank=8, lora_alpha=4.0, lora_targets=["ff.net.2"], lora_seed=3).lora.scale == 0.5
    for kw, msg in ((dict(lora_rank=4, use_ema=True), "use_ema"), (dict(lora_rank=4, shard_optimizer=True), "shard_optimizer"),
                    (dict(lora_rank=4, lora_targets=["nothing_here"]), "matches no tensor"),
                    (dict(lora_rank=4, lora_targets=["to_q", "ff.net.0.proj"]), "ff.net.0.proj"),
                    (dict(lora_rank=4, lora_targets=["conv_shortcut"]), "2-D"), (dict(lora_rank=129), "lora_rank"),
                    (dict(lora_rank=-1), "lora_rank")):
        with pytest.raises(ValueError, match=msg):
            _trainer(net, **kw)
    assert isinstance(_trainer(net, lora_rank=4, shard_optimizer=False), LORA.NativeLoRATrainer)


def test_load_lora_state_refuses_a_different_state_and_changes_nothing(net, tmp_path):
    a = _trainer(net, lora_rank=4)
    torch.save(a.lora.state_dict(), str(tmp_path / "lora_state.pt"))
    b = _trainer(net, lora_rank=8)
    before = b.lora.weights.clone()
    with pytest.raises(ValueError, match="rank"):
        b.load_lora_state(tmp_path)
    assert torch.equal(b.lora.weights, before)


def test_boundary_has_no_new_function_and_the_struct_mirrors_have_the_headers_size(tmp_path):
    text = (ROOT / "include" / "sdxlstep.h").read_text()
    declared = set(re.findall(r"\b(sdxl_[a-z0-9_]+)\s*\(", text))
    assert len(declared) <= 58 and not any("lora" in n for n in declared)
    assert "#define SDXL_DTYPE_LORA 2" in text and lib.DTYPE_LORA == 2
    assert {"sdxl_op_lora_merge", "sdxl_op_lora_project"} <= set(lib.TEST_HOOK_SIGNATURES)
    cc = next((c for c in (shutil.which("cc"), shutil.which("gcc"), shutil.which("clang"), "/opt/rocm/lib/llvm/bin/clang") if c and Path(c).exists()), None)
    assert cc is not None, "no C compiler"
    pairs = {"sdxl_lora_op": lib.LoraOp, "sdxl_unet_config": lib.UNetConfig, "sdxl_loss_config": lib.LossConfigExt, "sdxl_batch_ext": lib.CondGradBatch,
             "sdxl_sampler_step_ext": lib.SamplerStepExt, "sdxl_adamw_config": lib.AdamWConfig}
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include "sdxlstep.h"\nint main(void) {\n'
                   + "".join(f'  printf("{n} %zu\\n", sizeof({n}));\n' for n in pairs) + "  return 0;\n}\n")
    subprocess.run([cc, "-I", str(ROOT / "include"), str(src), "-o", str(tmp_path / "sizes")], check=True, capture_output=True)
    out = subprocess.run([str(tmp_path / "sizes")], check=True, capture_output=True, text=True).stdout
    sizes = dict(ln.split() for ln in out.splitlines())
    for n, cls in pairs.items():
        assert int(sizes[n]) == C.sizeof(cls), (n, sizes[n], C.sizeof(cls))
    assert [f[0] for f in lib.LoraOp._fields_] == ["n", "param", "rank", "scale", "adapters", "base", "adapter_grads"]


def test_hook_argument_errors_are_reported_before_any_launch():
    L = lib.load()
    buf = (C.c_char * 4096)()
    p = C.c_void_p((C.addressof(buf) + 15) & ~15)
    odd = C.c_void_p(p.value + 2)
    for args, msg in (((8, 8, 0), b"rank"), ((8, 8, 129), b"rank"), ((8, 12, 4), b"multiple of 8"), ((0, 8, 4), b"multiple of 8"), ((8, 0, 4), b"multiple of 8")):
        assert L.sdxl_op_lora_merge(p, p, p, p, *args, 1.0, None) == 1 and msg in L.sdxl_last_error(), args
        assert L.sdxl_op_lora_project(p, p, p, p, p, *args, 1.0, None) == 1 and msg in L.sdxl_last_error(), args
    assert L.sdxl_op_lora_merge(p, odd, p, p, 8, 8, 4, 1.0, None) == 1 and b"aligned" in L.sdxl_last_error()
    assert L.sdxl_op_lora_merge(None, p, p, p, 8, 8, 4, 1.0, None) == 1
    assert L.sdxl_op_lora_project(p, p, p, p, None, 8, 8, 4, 1.0, None) == 1
    assert L.sdxl_op_lora_merge(p, p, p, p, 8, 8, 4, float("nan"), None) == 1 and b"finite" in L.sdxl_last_error()
    op = lib.LoraOp()
    assert L.sdxl_load_weight(None, None, C.byref(op), lib.DTYPE_LORA, None) == 1
    assert L.sdxl_export_grad(None, None, C.byref(op), lib.DTYPE_LORA, None) == 1


def test_a_caller_owned_optimizer_step_projects_first(net):
    """optimizer.step() of a caller-owned loop never runs on stale adapter gradients: the trainer's optimizer projects before it steps"""
    tr = _trainer(net, lora_rank=4)
    calls = []
    tr.lora.project = lambda: calls.append("project")
    with pytest.raises(lib.SdxlError):                     # the stand-in has no library: the update itself is refused, after the projection
        tr.optimizer.step()
    assert calls == ["project"]
    with pytest.raises(lib.SdxlError):                     # nothing ran backward since: not projected twice
        tr.optimizer.step()
    assert calls == ["project"]
