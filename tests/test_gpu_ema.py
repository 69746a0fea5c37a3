"""The fp32 EMA of the weights on the GPU (csrc/optimizer.hip `ema_update8` inside both optimizer kernels; ema.WeightEMA; the
trainer): the EMA variants leave the update's bits alone and put the bits of tests/_ema_ref.py into the EMA, sharded pieces equal the
whole arena, the trainer end to end with checkpoint and resume, ZeRO-1 over two ranks, and the cost on the full-size arena."""
import ctypes as C
import importlib
import json
import os
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

import _ema_ref as R
import sdxl_amd  # noqa: F401
from sdxl_amd import lib
from _optim_common import Arena, bits, dev, ptr, stream

pytestmark = pytest.mark.gpu

O = importlib.import_module("sdxl-training-improvements_amd.optimizer")
E = importlib.import_module("sdxl-training-improvements_amd.ema")
ROOT = Path(__file__).resolve().parent.parent
FULL_ELEMS = 2567486784                                   # the SDXL UNet's packed arena (tests/golden/sdxl_segments.json)
GRID_STRIDE = 256 * 16 * 256 * 8                          # elements one pass of the optimizer kernels' largest grid covers


def _state(n, seed, grad_bf16, kahan=True):
    g = torch.Generator().manual_seed(seed)
    r = lambda s: torch.randn(n, generator=g) * s
    p = r(0.05).to(torch.bfloat16)
    st = {"p": p, "m": r(1e-3).to(torch.bfloat16), "v": (torch.rand(n, generator=g) * 1e-6).to(torch.bfloat16),
          "s": r(1e-5).to(torch.bfloat16) if kahan else None,
          "e": p.float() + r(2e-4)}                      # an EMA that has drifted off the weights: every op of the update rounds
    grad = r(2e-3)
    grad = grad.to(torch.bfloat16) if grad_bf16 else grad
    return {k: (v.to(dev()) if v is not None else None) for k, v in st.items()}, grad.to(dev())


def _cfg(L, algorithm, **kw):
    cfg = lib.AdamWConfig()
    lib.check(L.sdxl_adamw_default_config(C.byref(cfg)))
    cfg.lr, cfg.step, cfg.seed, cfg.algorithm = 1e-3, 3.0, 1234, algorithm
    if algorithm == 1:
        cfg.weight_decay, cfg.sf_step_size = 0.01, 1e-3
    for k, v in kw.items():
        setattr(cfg, k, v)
    return cfg


def _launch(L, cfg, st, grad, n, rand=None, scale=None, ema=None, omd=0.0):
    cfg.ema = ema.data_ptr() if ema is not None else None
    cfg.ema_one_minus_decay = omd
    lib.check(L.sdxl_adamw_bf16_step(ptr(st["p"]), ptr(grad), 1 if grad.dtype == torch.bfloat16 else 0, ptr(st["m"]), ptr(st["v"]),
                                     ptr(st["s"]), n, C.byref(cfg), ptr(scale), ptr(rand), stream()))


def _check_ema_variant(L, n, seed, algorithm, grad_bf16=False, kahan=True, rand=False, **kw):
    """two updates with EMA off and on from the same state: the update's arenas must keep their bits, the EMA must be the torch
    recurrence over the new weights"""
    st0, grad = _state(n, seed, grad_bf16, kahan)
    scale = torch.tensor([0.61], dtype=torch.float32, device=dev())
    rnd = torch.randint(-32768, 32767, (4 * n,), dtype=torch.int16, generator=torch.Generator().manual_seed(seed)).to(dev()) \
        if rand else None
    off = {k: (v.clone() if v is not None else None) for k, v in st0.items()}
    on = {k: (v.clone() if v is not None else None) for k, v in st0.items()}
    e_ref = st0["e"].cpu().clone()
    for k, decay in enumerate((0.0, 2 / 11, 0.9999)):
        omd = float(np.float32(1.0 - decay))
        _launch(L, _cfg(L, algorithm, step=float(k + 1), **kw), off, grad, n, rnd, scale)
        _launch(L, _cfg(L, algorithm, step=float(k + 1), **kw), on, grad, n, rnd, scale, ema=on["e"], omd=omd)
        torch.cuda.synchronize()
        for key in "pmvs":
            if off[key] is not None:
                bad = int((bits(off[key]) != bits(on[key])).sum())
                assert bad == 0, f"update {k + 1}: {key} differs in {bad}/{n} elements with the EMA on"
        R.step(e_ref, on["p"].cpu(), decay)
        bad = int((bits(on["e"]) != bits(e_ref)).sum())
        assert bad == 0, f"update {k + 1}: EMA differs from the torch recurrence in {bad}/{n} elements"
    assert not torch.equal(on["p"], st0["p"]) and not torch.equal(on["e"], st0["e"])
    assert torch.equal(off["e"], st0["e"])                # EMA off: the arena is not touched


@pytest.fixture(scope="module")
def L():
    return lib.load()


@pytest.mark.parametrize("rand", [False, True], ids=["philox", "rand_inject"])
def test_adamw_bf16_ema(L, rand):
    _check_ema_variant(L, (1 << 16) + 8, 3 + rand, 0, rand=rand, decay_this_iteration=1e-3 if rand else 0.0)


@pytest.mark.parametrize("grad_bf16", [False, True], ids=["fp32_grad", "bf16_grad"])
@pytest.mark.parametrize("kahan", [True, False], ids=["kahan", "no_kahan"])
@pytest.mark.parametrize("reference", [0, 1], ids=["compensated", "reference"])
def test_schedule_free_ema(L, reference, kahan, grad_bf16):
    _check_ema_variant(L, (1 << 16) + 24, 11 + 4 * reference + 2 * kahan + grad_bf16, 1, grad_bf16=grad_bf16, kahan=kahan,
                       sf_reference=reference, kahan_sum=int(kahan))


@pytest.mark.parametrize("algorithm", [0, 1])
def test_n_not_a_multiple_of_the_grid_stride(L, algorithm):
    """the grid-stride loop runs a second, partial pass"""
    _check_ema_variant(L, GRID_STRIDE + 4096 + 8, 41 + algorithm, algorithm, kahan=True, kahan_sum=1)


@pytest.mark.parametrize("kind", ["adamw_bf16", "adamw_schedule_free_kahan"])
def test_pieces_equal_full_update(kind):
    n = 65536 + 4096
    g0 = torch.Generator().manual_seed(21)
    w0 = (torch.randn(n, generator=g0) * 0.05).to(torch.bfloat16).to(dev())
    nets = {k: Arena(w0) for k in ("full", "pieces")}
    opts = {k: O.BY_TYPE[kind](x, lr=1e-2, weight_decay=0.05) for k, x in nets.items()}
    emas = {k: E.WeightEMA(x, update_after_step=1) for k, x in nets.items()}
    for k in opts:
        opts[k].attach_ema(emas[k])
    cuts = [0, 8, 1000, 33000, 65536, n]                  # multiples of 8, uneven
    pieces, goff = [], 0
    for a, b in zip(cuts[:-1], cuts[1:]):
        pieces.append((a, b - a, goff))
        goff += b - a
    for _ in range(4):
        g = (torch.randn(n, generator=g0) * 1e-2).to(dev())
        opts["full"].step(g)
        opts["pieces"].step(torch.cat([g[a:b] for a, b in zip(cuts[:-1], cuts[1:])]), pieces=pieces)
    torch.cuda.synchronize()
    assert emas["full"].optimization_step == emas["pieces"].optimization_step == 4
    assert torch.equal(nets["full"].weights, nets["pieces"].weights)
    assert (bits(emas["full"].arena) == bits(emas["pieces"].arena)).all()
    assert not torch.equal(emas["full"].arena, w0.float())


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


def _weights_fp32(net):
    return {k: v.cpu() for k, v in net.state_dict(dtype=torch.float32).items()}


def _owner(net, i):
    for k, (off, cnt) in net.param_ranges().items():
        if off <= i < off + cnt:
            return f"{k}+{i - off}/{cnt}"
    return "outside every tensor"


class TorchUNetStandIn:
    """what the trainer writes back into: a diffusers-keyed state_dict() / load_state_dict() (bf16, as the reference's UNet)"""

    def __init__(self, sd):
        self.sd = {k: v.to(torch.bfloat16).clone() for k, v in sd.items()}

    def state_dict(self):
        return self.sd

    def load_state_dict(self, sd, strict=True):
        assert set(sd) == set(self.sd)
        self.sd = {k: v.clone() for k, v in sd.items()}


@pytest.mark.parametrize("kind,warmup", [("adamw_bf16", False), ("adamw_schedule_free_kahan", True)])
def test_trainer_ema_checkpoint_and_resume(tiny, tmp_path, kind, warmup):
    cfgm, T, cfg, w, net = tiny
    c = cfgm.Config()
    c.training.method = "ddpm"
    c.training.gradient_accumulation_steps = 2
    c.training.clip_grad_norm = 1.0
    c.training.use_ema, c.training.ema_update_after_step, c.training.ema_use_warmup = True, 1, warmup
    c.optimizer.optimizer_type, c.optimizer.learning_rate = kind, 1e-3
    settings = dict(update_after_step=1, use_ema_warmup=warmup)
    # The fixed gradients below also land on arena elements outside every tensor (alignment gaps, conv_out's padded output rows),
    # which no backward writes: restore the whole weight arena and zero the gradient arena afterwards, so that the next case starts
    # as a fresh net does.
    arena0 = net.weights.clone()
    net.grads.zero_()
    try:
        torch_unet = TorchUNetStandIn(w)

        class M:
            unet = torch_unet
        tr = T.NativeSDXLTrainer(M(), train_dataloader=[_batch(cfg, 2, s) for s in range(12)], config=c,
                                 native_factory=lambda _cfg: net, native_config=net.cfg)
        o, ema = tr.optimizer, tr.ema
        assert type(o) is O.BY_TYPE[kind] and o.ema is ema and ema.optimization_step == 0
        ref = _weights_fp32(net)                          # e starts as the fp32 image of the weights
        decays = []
        real_step = o.step

        def checked_step(*a, **kw):
            real_step(*a, **kw)
            torch.cuda.synchronize()
            t = ema.optimization_step
            decays.append(ema.decay(t))
            d = R.get_decay(t, **settings)
            for k, p in _weights_fp32(net).items():
                R.step(ref[k], p.to(torch.bfloat16), d)
            got = tr.ema_state_dict()
            for k in ref:
                bad = int((bits(got[k]) != bits(ref[k])).sum())
                assert bad == 0, f"step {t} {k}: {bad}/{ref[k].numel()} EMA elements differ from the CPU recurrence"
        o.step = checked_step
        tr.train(1)
        o.step = real_step
        assert o.step_count == 6 and ema.optimization_step == 6
        assert decays == [R.get_decay(t, **settings) for t in range(1, 7)] and decays[:2] == [0.0, 0.0] and decays[2] > 0
        # ---- checkpoint: unet_ema in diffusers keys, fp32, equal to ema_state_dict(); ema.json
        ck = tmp_path / "ck"
        tr.prepare_checkpoint()
        tr.save_checkpoint(ck)
        from safetensors.torch import load_file
        saved = load_file(str(ck / "unet_ema" / "diffusion_pytorch_model.safetensors"))
        now = tr.ema_state_dict()
        assert set(saved) == set(net.param_table) and all(v.dtype == torch.float32 for v in saved.values())
        assert all(torch.equal(saved[k], now[k].cpu()) for k in saved)
        assert json.loads((ck / "ema.json").read_text()) == ema.state_dict()
        assert not all(torch.equal(now[k].cpu(), _weights_fp32(net)[k]) for k in now)      # the EMA is not the weights
        arena6, w6 = ema.arena.clone(), net.weights.clone()
        # ---- uninterrupted: two more steps on fixed gradients
        fixed = [torch.randn(net.param_elems, generator=torch.Generator().manual_seed(30 + i)).to(dev()) * 1e-3 for i in range(2)]
        for g in fixed:
            net.grads.copy_(g)
            tr.optimizer_step()
        torch.cuda.synchronize()
        a_w, a_e = net.weights.clone(), ema.arena.clone()
        # ---- resumed: a fresh trainer on the checkpointed weights, optimizer state and EMA
        net.weights.copy_(w6)
        tr2 = T.NativeSDXLTrainer(M(), config=c, native_factory=lambda _cfg: net, native_config=net.cfg)
        tr2.load_optimizer_state(ck)
        tr2.load_ema_state(ck)
        assert tr2.ema.optimization_step == 6
        diff = np.nonzero(bits(tr2.ema.arena) != bits(arena6))[0]      # the packed arena, bit for bit
        assert diff.size == 0, f"{diff.size} arena elements differ after load_ema_state: " + "; ".join(
            f"[{i}] {_owner(net, i)} saved {float(arena6[i])!r} loaded {float(tr2.ema.arena[i])!r} weight {float(w6[i])!r}"
            for i in diff[:8])
        for g in fixed:
            net.grads.copy_(g)
            tr2.optimizer_step()
        torch.cuda.synchronize()
        assert torch.equal(net.weights, a_w) and (bits(tr2.ema.arena) == bits(a_e)).all()
        # ---- sync_to_model(ema=True) writes the EMA into the module
        tr2.sync_to_model(ema=True)
        e2 = tr2.ema_state_dict()
        assert all(torch.equal(torch_unet.sd[k], e2[k].to(torch.bfloat16).cpu()) for k in e2)
        tr2.sync_to_model()
        assert all(torch.equal(torch_unet.sd[k].float(), v) for k, v in _weights_fp32(net).items())
        # ---- a mismatched EMA setting is refused on resume
        c.training.ema_decay = 0.999
        tr3 = T.NativeSDXLTrainer(M(), config=c, native_factory=lambda _cfg: net, native_config=net.cfg)
        with pytest.raises(ValueError):
            tr3.load_ema_state(ck)
        for t in (tr, tr2, tr3):
            t.ema.close()
    finally:
        net.weights.copy_(arena0)
        net.grads.zero_()


def test_zero1_ema_bit_equal_to_unsharded():
    """two ranks on one GPU over gloo (tests/_ema_zero1_worker.py): the trainer's ZeRO-1 step updates the EMA on the owned slices,
    and after prepare_checkpoint() it has the bits of all-reduce + the full update"""
    sys.path.insert(0, str(Path(__file__).resolve().parent))
    from test_gpu_multiproc import run_dist
    env = dict(os.environ, MASTER_ADDR="127.0.0.1")
    r = run_dist([str(ROOT / "tests" / "_ema_zero1_worker.py")], 29671, env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "EMA_ZERO1_OK" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


# ---------------------------------------------------------------------------------------------- time on the full arena
def test_full_arena_time_with_and_without_ema():
    """one update of the 2.567 B-parameter arena: AdamW_BF16 (Philox) and schedule-free Kahan (compensated), each with and without
    the EMA, timed alternately with HIP events after warm-up.  The EMA moves 8 B more per element (28 B against 20 B); a separate
    pass would move 10 B per element more and need ~1.5x the time of the plain update."""
    L = lib.load()
    n = FULL_ELEMS
    p = torch.full((n,), 0.05, dtype=torch.bfloat16, device=dev())
    m, v, c = (torch.zeros(n, dtype=torch.bfloat16, device=dev()) for _ in range(3))
    g = torch.full((n,), 1e-3, dtype=torch.float32, device=dev())
    e = torch.full((n,), 0.05, dtype=torch.float32, device=dev())
    st = stream()
    cfgs = {}
    for name in ("adamw", "adamw+ema", "sfk", "sfk+ema"):
        cfgs[name] = _cfg(L, 1 if name.startswith("sfk") else 0, kahan_sum=1)
        if name.endswith("+ema"):
            cfgs[name].ema, cfgs[name].ema_one_minus_decay = e.data_ptr(), float(np.float32(1 - 0.9999))
    run = {k: (lambda cf=cf: lib.check(L.sdxl_adamw_bf16_step(ptr(p), ptr(g), 0, ptr(m), ptr(v), ptr(c), n, C.byref(cf), None, None, st)))
           for k, cf in cfgs.items()}
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
        b = 28 if k.endswith("+ema") else 20
        print(f"[perf] {k}: median {med[k]:.3f} ms over {len(times[k])} (min {min(times[k]):.3f}) -> "
              f"{b * n / (med[k] * 1e-3) / 1e12:.2f} TB/s at {b} B/element")
    assert torch.isfinite(p[:1024].float()).all() and torch.isfinite(e[:1024]).all()
    assert med["adamw+ema"] <= 1.5 * med["adamw"], med
    assert med["sfk+ema"] <= 1.5 * med["sfk"], med
