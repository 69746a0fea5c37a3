"""Schedule-free Kahan AdamW on the GPU (csrc/optimizer.hip sfk_kernel, through optimizer.AdamWScheduleFreeKahanBF16 and the
C ABI): bit-exact against the reference's own fixtures (reference mode) and the CPU restatement (compensated mode), sharded
pieces, the trainer end to end with resume, ZeRO-1 over two ranks, and the update's time on the full-size arena."""
import ctypes as C
import importlib
import os
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

import _schedulefree_ref as S
import sdxl_amd  # noqa: F401
from sdxl_amd import lib
from _optim_common import Arena, bits, dev, to_dev_bits

pytestmark = pytest.mark.gpu

O = importlib.import_module("sdxl-training-improvements_amd.optimizer")
G = np.load(Path(__file__).parent / "golden" / "schedulefree_kahan.npz")
ROOT = Path(__file__).resolve().parent.parent
FULL_ELEMS = 2567486784                                   # the SDXL UNet's packed arena (tests/golden/sdxl_segments.json)


def _state(o, net):
    return [bits(net.weights), bits(o.exp_avg), bits(o.exp_avg_sq)] + ([bits(o.kahan_comp)] if o.kahan_sum else [])


@pytest.mark.parametrize("grad_kind", ["bf16", "fp32_rounded"])
@pytest.mark.parametrize("name", [str(c) for c in G["cases"]])
def test_reference_mode_equals_fixture(name, grad_kind):
    lr, b1, b2, eps, wd, warm, kahan = (float(x) for x in G[f"{name}_hyper"])
    net = Arena(to_dev_bits(G[f"{name}_p0"]))
    o = O.AdamWScheduleFreeKahanBF16(net, lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd, warmup_steps=int(warm),
                                     kahan_sum=bool(kahan), arithmetic="reference", grad_round_bf16=grad_kind != "bf16")
    for st in range(1, int(G[f"{name}_steps"]) + 1):
        g = to_dev_bits(G[f"{name}_grad{st}"])
        if grad_kind == "bf16":
            o.step(g)
        else:                                              # fp32 a fraction of a half-ulp off the bf16 value: the kernel rounds it back
            o.step((g.float() * (1 + 2.0 ** -10)).contiguous())
        torch.cuda.synchronize()
        assert (o.get_last_lr(), o.lr_max) == tuple(G[f"{name}_lr{st}"])
        for k, got in zip("pmvc", _state(o, net)):
            bad = int((got != G[f"{name}_{k}{st}"]).sum())
            assert bad == 0, f"{name} step {st} {k}: {bad}/{got.size} elements differ from the reference"


def _seeded(n, seed):
    rng = np.random.default_rng(seed)
    f = lambda a: S.f32_to_bf16_rn(a.astype(np.float32))
    return rng, f(rng.standard_normal(n) * 0.05), f(rng.standard_normal(n) * 1e-3), f(rng.random(n) * 1e-6), f(rng.standard_normal(n) * 1e-4)


@pytest.mark.parametrize("kahan", [True, False])
@pytest.mark.parametrize("round_bf16", [0, 1])
def test_compensated_mode_equals_helper(kahan, round_bf16):
    """1 M elements, fp32 gradients and a device grad_scale, 3 steps across the end of a warm-up, from a non-zero state"""
    n = 1 << 20
    rng, p, m, v, c = _seeded(n, 11 + 2 * kahan + round_bf16)
    net = Arena(to_dev_bits(p))
    o = O.AdamWScheduleFreeKahanBF16(net, lr=1e-3, weight_decay=0.01, warmup_steps=2, kahan_sum=kahan, grad_round_bf16=bool(round_bf16))
    o.exp_avg.copy_(to_dev_bits(m)); o.exp_avg_sq.copy_(to_dev_bits(v))
    if kahan:
        o.kahan_comp.copy_(to_dev_bits(c))
    scale = torch.tensor([0.37], dtype=torch.float32, device=dev())
    for k in range(3):
        g32 = (rng.standard_normal(n) * 2e-3).astype(np.float32)
        o.step(torch.from_numpy(g32).to(dev()), grad_scale=scale)
        _, ss = S.schedule(k, 1e-3, 0.999, 2)
        p, m, v, c, _ = S.step(p, m, v, c if kahan else None, S.grad_in(g32, float(scale), bool(round_bf16)), step_size=ss,
                               beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.01, kahan_sum=kahan, reference=False)
        torch.cuda.synchronize()
        for key, got, want in zip("pmvc", _state(o, net), (p, m, v, c)):
            bad = int((got != want).sum())
            assert bad == 0, f"step {k + 1} {key}: {bad}/{n} elements differ from the helper"
    if kahan:
        assert (bits(o.kahan_comp) != 0).mean() > 0.5   # the compensation is live


@pytest.mark.parametrize("arithmetic", ["compensated", "reference"])
def test_pieces_equal_full_update(arithmetic):
    n = 65536 + 4096
    rng, p, _m, _v, _c = _seeded(n, 21)
    nets = {k: Arena(to_dev_bits(p)) for k in ("full", "pieces")}
    opts = {k: O.AdamWScheduleFreeKahanBF16(x, lr=1e-2, weight_decay=0.05, arithmetic=arithmetic) for k, x in nets.items()}
    cuts = [0, 8, 1000, 33000, 65536, n]                  # multiples of 8, uneven
    for _ in range(2):
        g = torch.from_numpy((rng.standard_normal(n) * 1e-2).astype(np.float32)).to(dev())
        opts["full"].step(g)
        # ZeRO-1 layout: the shard holds the owned ranges back to back
        pieces, goff = [], 0
        for a, b in zip(cuts[:-1], cuts[1:]):
            pieces.append((a, b - a, goff))
            goff += b - a
        opts["pieces"].step(torch.cat([g[a:b] for a, b in zip(cuts[:-1], cuts[1:])]), pieces=pieces)
    torch.cuda.synchronize()
    for a, b in zip(_state(opts["full"], nets["full"]), _state(opts["pieces"], nets["pieces"])):
        assert (a == b).all()
    assert (bits(nets["full"].weights) != p).mean() > 0.5


# ---------------------------------------------------------------------------------------------- trainer, tiny UNet
@pytest.fixture(scope="module")
def tiny():
    from oracle import unet_ref as U
    from sdxl_amd import unet as NU
    cfgm = importlib.import_module("sdxl-training-improvements_amd.config")
    T = importlib.import_module("sdxl-training-improvements_amd.trainer")
    cfg = U.tiny_config()
    w = U.synth_weights(cfg, seed=0)
    net = NU.NativeUNet(NU.make_config(block_out_channels=cfg.block_out_channels,
                                       transformer_layers=cfg.transformer_layers_per_block,
                                       cross_attention_dim=cfg.cross_attention_dim,
                                       addition_time_embed_dim=cfg.addition_time_embed_dim, pooled_dim=cfg.pooled_dim))
    net.load_state_dict(w)
    yield cfgm, T, cfg, w, net
    net.close()


def _batch(cfg, B, seed):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)
    bfr = lambda t: t.to(torch.bfloat16).float()
    return {"vae_latents": r(B, 4, 16, 16), "prompt_embeds": bfr(r(B, 77, cfg.cross_attention_dim)),
            "pooled_prompt_embeds": bfr(r(B, cfg.pooled_dim)), "time_ids": torch.tensor([[[128.0, 128, 0, 0, 128, 128]]] * B),
            "metadata": {}}


def test_trainer_steps_and_resume(tiny, tmp_path):
    cfgm, T, cfg, w, net = tiny
    c = cfgm.Config()
    c.training.method = "ddpm"
    c.training.gradient_accumulation_steps = 2
    c.training.clip_grad_norm = 1e-6                      # small enough to clip every step
    c.optimizer.optimizer_type = "adamw_schedule_free_kahan"
    c.optimizer.learning_rate, c.optimizer.warmup_steps, c.optimizer.weight_decay = 1e-3, 2, 0.01

    class M:
        unet = net
    tr = T.NativeSDXLTrainer(M(), train_dataloader=[_batch(cfg, 2, s) for s in range(6)], config=c)
    o = tr.optimizer
    assert type(o) is O.AdamWScheduleFreeKahanBF16 and o.arithmetic == "compensated" and o.kahan_sum
    seen = []
    real_step = o.step

    def recording_step(grads=None, grad_scale=None, **kw):
        assert grads is None                              # single GPU: the native fp32 arena
        pre = [bits(net.weights), bits(o.exp_avg), bits(o.exp_avg_sq), bits(o.kahan_comp)]
        seen.append((pre, net.grads.cpu().numpy().copy(), None if grad_scale is None else float(grad_scale), o.schedule()[1]))
        real_step(grads, grad_scale=grad_scale, **kw)
        torch.cuda.synchronize()
        p, m, v, cc, _ = S.step(*pre, S.grad_in(seen[-1][1], seen[-1][2] or 1.0, False), step_size=seen[-1][3], beta1=0.9,
                                beta2=0.999, eps=1e-8, weight_decay=0.01, kahan_sum=True, reference=False)
        for key, got, want in zip("pmvc", _state(o, net), (p, m, v, cc)):
            bad = int((got != want).sum())
            assert bad == 0, f"step {len(seen)} {key}: {bad}/{got.size} elements differ from the helper"
    o.step = recording_step
    try:
        tr.train(1)
        assert o.step_count == 3 and len(seen) == 3
        assert all(s[2] is not None and s[2] < 1.0 for s in seen)          # clipping was active and fused into the kernel
        # ---- resume: checkpoint, then one more step here and in a fresh trainer that loads the checkpoint
        ck = tmp_path / "ck"
        tr.prepare_checkpoint()
        tr.save_checkpoint(ck)
        w3, lr_max3 = net.weights.clone(), o.lr_max
        fixed = torch.randn(net.param_elems, generator=torch.Generator().manual_seed(3)).to(dev()) * 1e-3
        o.step = real_step
        net.grads.copy_(fixed)
        tr.optimizer_step()
        a = _state(o, net)
        net.weights.copy_(w3)
        tr2 = T.NativeSDXLTrainer(M(), config=c)
        tr2.load_optimizer_state(ck)
        assert tr2.optimizer.step_count == 3 and tr2.optimizer.lr_max == lr_max3
        net.grads.copy_(fixed)
        tr2.optimizer_step()
        torch.cuda.synchronize()
        for x, y in zip(a, _state(tr2.optimizer, net)):
            assert (x == y).all()
        assert (tr2.optimizer.get_last_lr(), tr2.optimizer.lr_max) == (o.get_last_lr(), o.lr_max)
    finally:
        net.load_state_dict(w)


def test_zero1_update_bit_equal_to_unsharded():
    """two ranks on one GPU over gloo (tests/_zero1_worker.py): ZeRO-1 with the schedule-free Kahan update gives the same
    bits as all-reduce + the full update"""
    sys.path.insert(0, str(Path(__file__).resolve().parent))
    from test_gpu_multiproc import run_dist
    env = dict(os.environ, MASTER_ADDR="127.0.0.1")
    r = run_dist([str(ROOT / "tests" / "_zero1_worker.py"), "adamw_schedule_free_kahan"], 29611, env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "SFK_ZERO1_OK" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


# ---------------------------------------------------------------------------------------------- time on the full arena
def test_full_arena_time_vs_adamw_bf16():
    """one update of the 2.567 B-parameter arena: schedule-free Kahan (compensated, Kahan on: 20 B / element) and AdamW_BF16
    (Philox mode, 20 B / element), timed alternately with HIP events after warm-up"""
    L = lib.load()
    n = FULL_ELEMS
    p = torch.full((n,), 0.05, dtype=torch.bfloat16, device=dev())
    m, v, c = (torch.zeros(n, dtype=torch.bfloat16, device=dev()) for _ in range(3))
    g = torch.full((n,), 1e-3, dtype=torch.float32, device=dev())
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    ptr = lambda t: C.c_void_p(t.data_ptr())
    sf, aw = lib.AdamWConfig(), lib.AdamWConfig()
    lib.check(L.sdxl_adamw_default_config(C.byref(sf)))
    lib.check(L.sdxl_adamw_default_config(C.byref(aw)))
    sf.algorithm, sf.kahan_sum, sf.sf_reference, sf.weight_decay, sf.sf_step_size = 1, 1, 0, 0.01, 1e-6
    run = {"sfk": lambda: lib.check(L.sdxl_adamw_bf16_step(ptr(p), ptr(g), 0, ptr(m), ptr(v), ptr(c), n, C.byref(sf), None, None, st)),
           "adamw": lambda: lib.check(L.sdxl_adamw_bf16_step(ptr(p), ptr(g), 0, ptr(m), ptr(v), ptr(c), n, C.byref(aw), None, None, st))}
    times = {k: [] for k in run}
    for it in range(9):
        for k, fn in run.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if it >= 2:                                   # two warm-up rounds
                times[k].append(e0.elapsed_time(e1))
    med = {k: float(np.median(t)) for k, t in times.items()}
    for k in run:
        print(f"[perf] {k}: median {med[k]:.3f} ms over {len(times[k])} (min {min(times[k]):.3f}) -> "
              f"{20 * n / (med[k] * 1e-3) / 1e12:.2f} TB/s at 20 B/element")
    assert torch.isfinite(p[:1024].float()).all()
    assert med["sfk"] <= 1.15 * med["adamw"], med
