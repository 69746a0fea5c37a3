"""LoRA by merge and project on a real MI355X: the two kernels of csrc/lora.hip through their single-target hooks (bit-equal merge,
a-priori bounded projections, overwritten outputs, reproducible bits, operand isolation), through sdxl_load_weight / sdxl_export_grad
on the tiny UNet's handle (each target bit-equal to the hook, nothing else touched, argument errors), and the trainer (zero adapter =
the plain trainer's bits, adapter gradients against the oracle at the bf16-rounded merged weights, training, checkpoint round trip,
two ranks)."""
import ctypes as C
import importlib
import os
from pathlib import Path
from types import SimpleNamespace

import pytest
import torch

import sdxl_amd  # noqa: F401
from oracle import loss_ref as R
from oracle import unet_ref as U
from sdxl_amd import lib
from sdxl_amd import unet as NU

import _lora_ref as LR
from _gradparity import GradParity
from _isolation import Spec, assert_isolated, run_isolated, same_bits

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
CFG = importlib.import_module("sdxl-training-improvements_amd.config")
T = importlib.import_module("sdxl-training-improvements_amd.trainer")
LORA = importlib.import_module("sdxl-training-improvements_amd.lora")

GRAD_BAR = (6e-2, 0.995)          # TINY_GRAD_BAR of tests/test_gpu_model.py
SHAPES = [(1, 8), (8, 8), (40, 24), (130, 264), (256, 128), (64, 2048), (640, 2048), (1280, 1280), (1280, 2048), (1280, 5120)]
RANKS = [1, 3, 4, 16, 128]
DEV = "cuda"

bf = lambda t: t.to(torch.bfloat16)
ptr = lambda t: C.c_void_p(t.data_ptr())
stream = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)


def operands(out, inn, rank, seed=0):
    g = torch.Generator().manual_seed(1000 * seed + 7 * out + inn + rank)
    r = lambda *s: torch.randn(*s, generator=g)
    return dict(W0=bf(r(out, inn)).to(DEV), A=bf(r(rank, inn)).to(DEV), B=bf(r(out, rank)).to(DEV), dW=r(out, inn).to(DEV))


def hook_merge(W0, A, B, s):
    w = torch.full_like(W0, float("nan"))
    lib.check(lib.load().sdxl_op_lora_merge(ptr(W0), ptr(A), ptr(B), ptr(w), W0.shape[0], W0.shape[1], A.shape[0], s, stream()), "lora_merge")
    return w


def hook_project(dW, A, B, s):
    dA = torch.full(A.shape, float("nan"), dtype=torch.float32, device=dW.device)
    dB = torch.full(B.shape, float("nan"), dtype=torch.float32, device=dW.device)
    lib.check(lib.load().sdxl_op_lora_project(ptr(dW), ptr(A), ptr(B), ptr(dA), ptr(dB), dW.shape[0], dW.shape[1], A.shape[0], s, stream()),
              "lora_project")
    return dA, dB


# ------------------------------------------------------------------------------------------------ the hooks
@pytest.mark.parametrize("rank", RANKS)
@pytest.mark.parametrize("out,inn", SHAPES, ids=[f"{o}x{i}" for o, i in SHAPES])
def test_merge_is_bit_equal_to_the_restatement(out, inn, rank):
    x = operands(out, inn, rank)
    for s in (0.37, 1.0):
        got = hook_merge(x["W0"], x["A"], x["B"], s)
        assert same_bits(got, LR.merge(x["W0"], x["A"], x["B"], s)), (out, inn, rank, s)
    assert same_bits(hook_merge(x["W0"], x["A"], x["B"], 0.0), x["W0"])
    assert same_bits(hook_merge(x["W0"], x["A"], torch.zeros_like(x["B"]), 0.37), x["W0"])


@pytest.mark.parametrize("rank", RANKS)
@pytest.mark.parametrize("out,inn", SHAPES, ids=[f"{o}x{i}" for o, i in SHAPES])
def test_project_is_within_the_a_priori_bound_overwrites_and_repeats(out, inn, rank):
    x = operands(out, inn, rank, seed=1)
    s = 0.37
    dA, dB = hook_project(x["dW"], x["A"], x["B"], s)               # outputs pre-filled with NaN
    rA, rB = LR.project64(x["dW"], x["A"], x["B"], s)
    bA, bB = LR.project_bound(x["dW"], x["A"], x["B"], s)
    for name, got, ref, bound in (("dA", dA, rA, bA), ("dB", dB, rB, bB)):
        assert bool(torch.isfinite(got).all()), f"{name}: not overwritten everywhere"
        excess = float(((got.double() - ref).abs() - bound).max())
        print(f"[lora] project {out}x{inn} r{rank} {name}: max |err| / bound {float(((got.double() - ref).abs() / bound.clamp_min(1e-300)).max()):.3f}")
        assert excess <= 0.0, (name, out, inn, rank, excess)
    dA2, dB2 = hook_project(x["dW"], x["A"], x["B"], s)
    assert same_bits(dA, dA2) and same_bits(dB, dB2)


@pytest.mark.parametrize("out,inn,rank", [(40, 24, 3), (130, 264, 16)])
def test_hooks_are_operand_isolated(out, inn, rank):
    x = {k: v.cpu() for k, v in operands(out, inn, rank, seed=2).items()}
    L = lib.load()
    f32 = torch.float32

    def merge(a):
        lib.check(L.sdxl_op_lora_merge(a.ptr("W0"), a.ptr("A"), a.ptr("B"), a.ptr("w"), out, inn, rank, 0.37, stream()), "lora_merge")

    def project(a):
        lib.check(L.sdxl_op_lora_project(a.ptr("dW"), a.ptr("A"), a.ptr("B"), a.ptr("dA"), a.ptr("dB"), out, inn, rank, 0.37, stream()), "lora_project")

    ab = [Spec("A", rank, inn, init=x["A"]), Spec("B", out, rank, init=x["B"])]
    runs = run_isolated(merge, [Spec("W0", out, inn, init=x["W0"])] + ab + [Spec("w", out, inn, role="out")], device=DEV)
    assert_isolated(runs, what=f"lora_merge {out}x{inn} r{rank}")
    assert same_bits(runs[0]["w"].cpu(), LR.merge(x["W0"], x["A"], x["B"], 0.37))
    runs = run_isolated(project, [Spec("dW", out, inn, dtype=f32, init=x["dW"])] + ab
                        + [Spec("dA", rank, inn, dtype=f32, role="out"), Spec("dB", out, rank, dtype=f32, role="out")], device=DEV)
    assert_isolated(runs, what=f"lora_project {out}x{inn} r{rank}")


# ------------------------------------------------------------------------------------------------ the handle (tiny UNet)
def tiny_native_cfg(c):
    return NU.make_config(block_out_channels=c.block_out_channels, transformer_layers=c.transformer_layers_per_block,
                          cross_attention_dim=c.cross_attention_dim, addition_time_embed_dim=c.addition_time_embed_dim, pooled_dim=c.pooled_dim)


@pytest.fixture(scope="module")
def tiny():
    cfg = U.tiny_config()
    w = U.synth_weights(cfg, seed=0)
    net = NU.NativeUNet(tiny_native_cfg(cfg))
    net.load_state_dict(w)
    torch.cuda.synchronize()
    w0 = net.weights.clone()
    yield cfg, w, net, w0
    net.close()


def randomize_B(ad, std=0.02, seed=5):
    g = torch.Generator().manual_seed(seed)
    for k in ad.targets:
        ad.B(k).copy_(bf(torch.randn(ad.B(k).shape, generator=g) * std))


def target_mask(net, ad):
    m = torch.zeros(net.param_elems, dtype=torch.bool, device=net.weights.device)
    ranges = net.param_ranges()
    for k in ad.targets:
        m[ranges[k][0]: ranges[k][0] + ranges[k][1]] = True
    return m


def test_batched_calls_equal_the_hook_per_target_and_touch_nothing_else(tiny):
    cfg, w, net, w0 = tiny
    ad = LORA.LoRAAdapters(net, rank=4, alpha=2.0)
    assert len(ad.targets) == sum(k.endswith(tuple(p + ".weight" for p in LORA.DEFAULT_TARGETS)) for k in net.param_shapes())
    randomize_B(ad, std=0.5)
    ranges, mask = net.param_ranges(), target_mask(net, ad)
    try:
        ad.merge()
        torch.cuda.synchronize()
        assert same_bits(net.weights[~mask], w0[~mask])
        base = 0
        for k in ad.targets:
            off, n = ranges[k]
            o, i = net.param_shapes()[k]
            W0 = ad.base[base: base + n].view(o, i)
            base += n
            assert same_bits(W0.reshape(-1), w0[off: off + n])
            one = hook_merge(W0, ad.A(k), ad.B(k), ad.scale)
            assert same_bits(net.weights[off: off + n], one.reshape(-1)), k
            assert not same_bits(one.reshape(-1), w0[off: off + n]), k            # took effect
        ad.restore()
        torch.cuda.synchronize()
        assert same_bits(net.weights, w0)
        # project: the gradient arena is read only; every target's dA / dB has the hook's bits; the padding is not written
        net.grads.copy_(torch.randn(net.param_elems, generator=torch.Generator().manual_seed(3)))
        g0 = net.grads.clone()
        ad.grads.fill_(float("nan"))
        ad.project()
        torch.cuda.synchronize()
        assert same_bits(net.grads, g0) and same_bits(net.weights, w0)
        written = torch.zeros(ad.param_elems, dtype=torch.bool, device=ad.grads.device)
        for k in ad.targets:
            off, n = ranges[k]
            o, i = net.param_shapes()[k]
            dA, dB = hook_project(g0[off: off + n].view(o, i), ad.A(k), ad.B(k), ad.scale)
            assert same_bits(ad.A(k, grad=True), dA) and same_bits(ad.B(k, grad=True), dB), k
            a, b = ad.layout[k][:2]
            written[a: a + ad.rank * i] = True
            written[b: b + o * ad.rank] = True
        assert bool(torch.isnan(ad.grads[~written]).all()) and bool(torch.isfinite(ad.grads[written]).all())
    finally:
        net.weights.copy_(w0)
        net.grads.zero_()
        torch.cuda.synchronize()


def test_argument_errors_before_any_launch(tiny):
    cfg, w, net, w0 = tiny
    L = lib.load()
    ad = LORA.LoRAAdapters(net, rank=4)
    names = list(net.param_shapes())
    idx = lambda k: names.index(k)
    big = torch.zeros(1 << 20, dtype=torch.bfloat16, device=DEV)
    gbig = torch.zeros(1 << 20, dtype=torch.float32, device=DEV)

    def op(params, rank=4):
        arr = (C.c_int * len(params))(*params)
        return lib.LoraOp(len(params), arr, rank, 1.0, big.data_ptr(), big.data_ptr(), gbig.data_ptr()), arr

    q = "down_blocks.1.attentions.0.transformer_blocks.0.attn1.to_q.weight"
    cases = [([idx(q)], 0, b"rank"), ([idx(q)], 129, b"rank"), ([idx("conv_in.weight")], 4, b"conv_in.weight"),
             ([idx("down_blocks.1.attentions.0.transformer_blocks.0.ff.net.0.proj.weight")], 4, b"ff.net.0.proj"),
             ([idx("down_blocks.0.resnets.0.conv1.weight")], 4, b"conv1.weight"), ([idx(q), idx(q)], 4, b"twice"),
             ([len(names)], 4, b"out of range"), ([idx("conv_out.bias")], 4, b"conv_out.bias")]
    for params, rank, msg in cases:
        o, _keep = op(params, rank)
        for fn in (L.sdxl_load_weight, L.sdxl_export_grad):
            assert fn(net.h, None, C.byref(o), lib.DTYPE_LORA, stream()) == 1 and msg in L.sdxl_last_error(), (params, rank, L.sdxl_last_error())
    o, _keep = op([idx(q)])
    assert L.sdxl_load_weight(net.h, b"conv_in.weight", C.byref(o), lib.DTYPE_LORA, stream()) == 1 and b"NULL" in L.sdxl_last_error()
    assert L.sdxl_export_grad(net.h, q.encode(), C.byref(o), lib.DTYPE_LORA, stream()) == 1 and b"NULL" in L.sdxl_last_error()
    for args in ((8, 8, 0), (8, 8, 129), (8, 12, 4)):
        assert L.sdxl_op_lora_merge(ptr(big), ptr(big), ptr(big), ptr(big), *args, 1.0, stream()) == 1
        assert L.sdxl_op_lora_project(ptr(gbig), ptr(big), ptr(big), ptr(gbig), ptr(gbig), *args, 1.0, stream()) == 1
    torch.cuda.synchronize()
    assert same_bits(net.weights, w0) and float(big.abs().sum()) == 0.0 and float(gbig.abs().sum()) == 0.0
    del ad


# ------------------------------------------------------------------------------------------------ the trainer (tiny UNet, 16 x 16, B = 2)
def make_batch(cfg, seed, B=2, H=16, W=16):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)
    return {"vae_latents": r(B, 4, H, W), "prompt_embeds": bf(r(B, 77, cfg.cross_attention_dim)).float(),
            "pooled_prompt_embeds": bf(r(B, cfg.pooled_dim)).float(), "time_ids": torch.tensor([[8.0 * H, 8.0 * W, 0, 0, 8.0 * H, 8.0 * W]] * B),
            "metadata": {}}


def step_args(method, seed, B=2, H=16, W=16):
    g = torch.Generator().manual_seed(seed)
    noise = torch.randn(B, 4, H, W, generator=g)
    ts = torch.tensor([650, 300][:B]) if method == "ddpm" else torch.tensor([0.35, 0.8][:B])
    return dict(timesteps=ts, noise=noise)


def make_trainer(net, method="ddpm", **training):
    cfg = CFG.Config()
    cfg.training.method = method
    cfg.optimizer.learning_rate = 1e-3
    for k, v in training.items():
        setattr(cfg.training, k, v)
    return T.create_trainer(SimpleNamespace(unet=net), config=cfg)


@pytest.mark.parametrize("method", ["ddpm", "flow_matching"])
def test_zero_adapter_step_has_the_plain_trainers_bits(tiny, method):
    cfg, w, net, w0 = tiny
    batch, kw = make_batch(cfg, 21), step_args(method, 22)
    plain = make_trainer(net, method)
    loss_p, _m = plain._execute_training_step(batch, **kw)
    torch.cuda.synchronize()
    g_p = net.grads.clone()
    del plain
    tr = make_trainer(net, method, lora_rank=4)
    assert isinstance(tr, LORA.NativeLoRATrainer)
    torch.cuda.synchronize()
    assert same_bits(net.weights, w0)                                  # B = 0: the merge gave back W0
    loss_l, _m = tr._execute_training_step(batch, **kw)
    torch.cuda.synchronize()
    assert float(loss_l) == float(loss_p) and same_bits(net.grads, g_p)
    assert float(g_p.abs().max()) > 0


@pytest.mark.parametrize("method,rank", [("ddpm", 4), ("ddpm", 16), ("flow_matching", 4)])
def test_adapter_gradients_match_the_oracle_at_the_merged_weights(tiny, method, rank):
    """native dA / dB against the float64 projection of the oracle's autograd dW, the oracle evaluated at the bf16-rounded MERGED weights
    (the weights the HIP step ran on), per tensor with the bar of tests/test_gpu_model.py"""
    cfg, w, net, w0 = tiny
    ad = LORA.LoRAAdapters(net, rank=rank, alpha=rank / 2, targets=list(LORA.DEFAULT_TARGETS) + ["ff.net.2", "proj_in"], seed=1)
    randomize_B(ad, std=0.02)
    batch, kw = make_batch(cfg, 31), step_args(method, 32)
    try:
        ad.merge()
        x = batch
        if method == "ddpm":
            sig = R.karras_sigmas()[kw["timesteps"]]
            net.forward_loss("ddpm", x["vae_latents"], kw["noise"], sig, kw["timesteps"].float(), x["prompt_embeds"], x["pooled_prompt_embeds"], x["time_ids"])
        else:
            t = kw["timesteps"]
            net.forward_loss("flow_matching", x["vae_latents"], kw["noise"], t, t, x["prompt_embeds"], x["pooled_prompt_embeds"], x["time_ids"])
        net.zero_grads()
        net.backward(1.0, True)
        ad.project()
        torch.cuda.synchronize()
        wm = {k: v.float().cpu() for k, v in net.state_dict().items()}           # bf16-rounded merged weights, as the step read them
        assert any(not torch.equal(wm[k], w[k]) for k in ad.targets)
        leaves = {k: wm[k].requires_grad_(True) for k in ad.targets}
        unet_fn = lambda s, t, e, p, ti: U.unet_forward(wm, s, t, e, p, ti, cfg)
        ob = {k: x[k] for k in ("vae_latents", "prompt_embeds", "pooled_prompt_embeds", "time_ids")}
        ref = R.compute_loss_ddpm(unet_fn, ob, kw["noise"], kw["timesteps"]) if method == "ddpm" else R.compute_loss_flow(unet_fn, ob, kw["noise"], kw["timesteps"])
        ref["loss"].backward()
        par = GradParity(f"lora {method} r{rank}")
        for k in ad.targets:
            dA, dB = LR.project64(leaves[k].grad, ad.A(k).cpu(), ad.B(k).cpu(), ad.scale)
            mod = k[: -len(".weight")]
            par.add(f"{mod}.lora_A.weight", ad.A(k, grad=True).cpu(), dA)
            par.add(f"{mod}.lora_B.weight", ad.B(k, grad=True).cpu(), dB)
        par.check(GRAD_BAR, expect=ad.param_ranges(), printer=lambda s: print("[parity] " + s))
    finally:
        net.weights.copy_(w0)
        torch.cuda.synchronize()


def run_training(net, w0, method, steps, accum=2, save_at=None, save_dir=None, resume_from=None, first_step=0, **training):
    """`steps` optimizer steps of `accum` micro-steps on seeded batches; returns (trainer, [losses])"""
    cfg = U.tiny_config()
    tr = make_trainer(net, method, lora_rank=4, lora_alpha=8.0, gradient_accumulation_steps=accum, **training)
    if resume_from is not None:
        tr.load_lora_state(resume_from)
    losses = []
    for s in range(first_step, first_step + steps):
        for m in range(accum):
            loss, _m = tr._execute_training_step(make_batch(cfg, 100 + 10 * s + m), accumulate=True, is_last_accumulation_step=m == accum - 1,
                                                 **step_args(method, 200 + 10 * s + m))
            losses.append(float(loss))
        tr.optimizer_step()
        if save_at is not None and s == save_at:
            tr.save_checkpoint(save_dir)
    torch.cuda.synchronize()
    return tr, losses


def test_training_moves_only_the_targets_and_repeats_bit_for_bit(tiny):
    cfg, w, net, w0 = tiny
    try:
        tr, losses = run_training(net, w0, "ddpm", 3)
        ad = tr.lora
        mask, ranges = target_mask(net, ad), net.param_ranges()
        assert same_bits(net.weights[~mask], w0[~mask])
        base, moved = 0, 0
        for k in ad.targets:
            off, n = ranges[k]
            o, i = net.param_shapes()[k]
            assert same_bits(net.weights[off: off + n], LR.merge(ad.base[base: base + n].view(o, i), ad.A(k), ad.B(k), ad.scale).reshape(-1)), k
            moved += int(not same_bits(net.weights[off: off + n], w0[off: off + n]))
            base += n
        assert moved == len(ad.targets) and float(ad.weights.float().abs().max()) > 0
        first = (net.weights.clone(), net.grads.clone(), ad.weights.clone(), ad.grads.clone(), losses)
        ad.restore()
        torch.cuda.synchronize()
        assert same_bits(net.weights, w0)
        tr2, losses2 = run_training(net, w0, "ddpm", 3)
        for a, b in zip(first[:4], (net.weights, net.grads, tr2.lora.weights, tr2.lora.grads)):
            assert same_bits(a, b)
        assert losses2 == first[4]
    finally:
        net.weights.copy_(w0)
        torch.cuda.synchronize()


@pytest.mark.parametrize("method", ["ddpm", "flow_matching"])
def test_twenty_steps_on_one_batch_lower_its_loss(tiny, method):
    cfg, w, net, w0 = tiny
    try:
        tr = make_trainer(net, method, lora_rank=4)
        batch = make_batch(cfg, 41)
        t = 500 if method == "ddpm" else 0.5
        noise = torch.randn(batch["vae_latents"].shape, generator=torch.Generator().manual_seed(42))       # evaluate() draws the same
        ts = torch.full((2,), t, dtype=torch.long if method == "ddpm" else torch.float32)
        evaluate = lambda: tr.evaluate([batch], [t], generator=torch.Generator().manual_seed(42))[1]
        before = evaluate()
        for _ in range(20):
            tr._execute_training_step(batch, timesteps=ts, noise=noise)
            tr.optimizer_step()
        after = evaluate()
        print(f"[lora] {method}: evaluation loss {before:.6f} -> {after:.6f} after 20 steps")
        assert after < before
    finally:
        net.weights.copy_(w0)
        torch.cuda.synchronize()


def test_checkpoint_round_trip_and_exported_delta(tiny, tmp_path):
    from safetensors.torch import load_file
    cfg, w, net, w0 = tiny
    try:
        tr, _l = run_training(net, w0, "ddpm", 3, save_at=1, save_dir=tmp_path / "ck")
        want = (net.weights.clone(), tr.lora.weights.clone(), tr.optimizer.exp_avg.clone(), tr.optimizer.exp_avg_sq.clone())
        assert sorted(p.name for p in (tmp_path / "ck").iterdir()) == ["config.json", "lora_state.pt", "optimizer.pt", "pytorch_lora_weights.safetensors"]
        net.weights.copy_(w0)                                      # a fresh process would load the checkpoint's UNet
        tr2, _l = run_training(net, w0, "ddpm", 1, resume_from=tmp_path / "ck", first_step=2)
        got = (net.weights, tr2.lora.weights, tr2.optimizer.exp_avg, tr2.optimizer.exp_avg_sq)
        for a, b in zip(want, got):
            assert same_bits(a, b)
        # the exported file reproduces s B A per target to fp32 rounding (state after step 1, read back from lora_state.pt)
        ex = load_file(str(tmp_path / "ck" / "pytorch_lora_weights.safetensors"))
        st = torch.load(str(tmp_path / "ck" / "lora_state.pt"), weights_only=True)
        assert len(ex) == 2 * len(tr.lora.targets) and st["rank"] == 4 and st["targets"] == tr.lora.targets
        s = st["alpha"] / st["rank"]
        for k in tr.lora.targets:
            a, b, o, i = tr.lora.layout[k]
            A, B = st["weights"][a: a + 4 * i].view(4, i).double(), st["weights"][b: b + o * 4].view(o, 4).double()
            mod = k[: -len(".weight")]
            lA, lB = ex[f"unet.{mod}.lora_A.weight"].double(), ex[f"unet.{mod}.lora_B.weight"].double()
            err = (lB @ lA - s * (B @ A)).abs()
            assert float((err - 2.0 ** -23 * (s * B.abs() @ A.abs())).max()) <= 0.0 and float((B @ A).abs().max()) > 0, k
        other = make_trainer(net, "ddpm", lora_rank=8)
        before = other.lora.weights.clone()
        with pytest.raises(ValueError):
            other.load_lora_state(tmp_path / "ck")
        assert same_bits(other.lora.weights, before)
    finally:
        net.weights.copy_(w0)
        torch.cuda.synchronize()


def test_two_ranks_exchange_adapter_gradients_bit_equal_to_the_sum():
    from test_gpu_multiproc import run_dist
    env = dict(os.environ, MASTER_ADDR="127.0.0.1")
    r = run_dist([str(ROOT / "tests" / "_lora_dp_worker.py")], 29727, env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "LORA_DP_OK" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
