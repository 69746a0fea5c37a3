"""The native sampler on the GPU: the step kernel (through its test hook) against the host restatement tests/_sampler_ref.py, the
whole sampler against a Python loop around unet_forward, and the trainer's sample() / evaluate() on the trained and the EMA weights."""
import ctypes as C
import importlib
import os
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

import _sampler_ref as R
import sdxl_amd  # noqa: F401
from sdxl_amd import lib
from sdxl_amd import unet as NU
from _optim_common import bits, dev, ptr, stream

S = importlib.import_module("sdxl-training-improvements_amd.sampler")
T = importlib.import_module("sdxl-training-improvements_amd.trainer")
CFG = importlib.import_module("sdxl-training-improvements_amd.config")

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
SHAPES = [(B, H, W) for B in (1, 2, 4) for (H, W) in ((8, 8), (128, 128), (168, 96))]


def _f32(v):
    return float(np.float32(v))


def to_nhwc8(t, fill=0.0):
    """[B,4,H,W] -> [B*H*W][8] bf16; channels 4..7 = fill (the kernel must not read them)"""
    B, _c, H, W = t.shape
    o = torch.full((B * H * W, 8), fill, dtype=torch.bfloat16)
    o[:, :4] = t.permute(0, 2, 3, 1).reshape(B * H * W, 4).to(torch.bfloat16)
    return o


def run_hook(x, fc, fu, k):
    """the step kernel on caller buffers.  x [B,4,H,W] fp32, fc / fu bf16-valued [B,4,H,W] (fu None without cfg), k the scalar
    fields of sdxl_sampler_step.  Returns (x after, input image [(2B|B)*HW][8] bf16), both on the CPU."""
    L = lib.load()
    B, _c, H, W = x.shape
    cfg = int(k["cfg"])
    xd = x.to(dev()).contiguous()
    pred = to_nhwc8(torch.cat([fc, fu]) if cfg else fc, fill=7.0).to(dev())
    xin = torch.full_like(pred, float("nan"))                       # every row must be written
    s = lib.SamplerStep(None, cfg, int(k.get("init", 0)), k["a_skip"], k["a_out"], k["p"], k["q"], k["a_in_next"], k["clamp"],
                        k["guidance"], k.get("guidance_rescale", 0.0))
    lib.check(L.sdxl_op_sampler_step(ptr(xd), ptr(pred), ptr(xin), B, H, W, C.byref(s), stream()), "sdxl_op_sampler_step")
    torch.cuda.synchronize()
    return xd.cpu(), xin.cpu()


def check_image(xin, want_in, B, H, W, cfg):
    """the input image: channels 0..3 = want_in (bf16 bits), 4..7 zero, both halves identical"""
    rows = B * H * W
    assert xin.shape == ((2 if cfg else 1) * rows, 8)
    got = xin[:rows]
    assert (bits(got[:, :4].contiguous()) == bits(to_nhwc8(want_in)[:, :4].contiguous())).all()
    assert (bits(got[:, 4:].contiguous()) == 0).all()
    if cfg:
        assert (bits(xin[rows:].contiguous()) == bits(got.contiguous())).all()


def _mode_step(mode):
    """(kernel scalars, scale of the state) of one representative step per parameter set"""
    if mode in ("ddpm_v", "ddpm_eps"):
        sm = S.NativeSampler(None, "ddpm", "v_prediction" if mode == "ddpm_v" else "epsilon", True, "trained")
        x0, steps = sm.schedule(8)
        j = 3
        return S.kernel_steps(steps, 5.0, 0.0, True)[j], float(sm.table[S.ddpm_indices(8)[j]])
    if mode in ("reference", "reference_first"):
        sm = S.NativeSampler(None, "ddpm", "v_prediction", True, "reference")
        x0, steps = sm.schedule(8)
        j = 0 if mode == "reference_first" else 4
        return S.kernel_steps(steps, 5.0, 0.0, True)[j], 1.0 if j == 0 else float(sm.table[S.ddpm_indices(8)[j - 1]])
    if mode == "flow":
        x0, steps = S.NativeSampler(None, "flow_matching").schedule(8)
        return S.kernel_steps(steps, 5.0, 0.0, True)[3], 1.0
    if mode == "clamp":                        # a state of magnitude 8e4 whose next input the +-20000 clamp cuts
        return dict(cfg=1, init=0, a_skip=1.0, a_out=-1.0, p=0.9, q=0.1, a_in_next=1.0, clamp=20000.0, guidance=5.0,
                    guidance_rescale=0.0), 8e4
    raise KeyError(mode)


# ---------------------------------------------------------------------------------------------- 5. the step kernel, bit-exact
@pytest.mark.parametrize("cfg", [0, 1])
@pytest.mark.parametrize("mode", ["ddpm_v", "ddpm_eps", "reference", "reference_first", "flow", "clamp"])
def test_step_kernel_bit_exact(mode, cfg):
    k, scale = _mode_step(mode)
    k = dict(k, cfg=cfg, guidance=k["guidance"] if cfg else 1.0)
    for (B, H, W) in SHAPES:
        g = torch.Generator().manual_seed(1000 * B + H + W + cfg)
        x = torch.randn(B, 4, H, W, generator=g) * scale
        fc = torch.randn(B, 4, H, W, generator=g).to(torch.bfloat16)
        fu = torch.randn(B, 4, H, W, generator=g).to(torch.bfloat16) if cfg else None
        want_x, want_in = R.full_step(x, fc.float(), None if fu is None else fu.float(), k)
        got_x, xin = run_hook(x, fc, fu, k)
        bad = int((bits(got_x) != bits(want_x)).sum())
        assert bad == 0, f"{mode} cfg={cfg} {(B, H, W)}: {bad}/{want_x.numel()} state elements differ from the restatement"
        check_image(xin, want_in, B, H, W, cfg)
        if mode == "clamp":
            cut = int((want_in.abs() == float(torch.tensor(20000.0).to(torch.bfloat16))).sum())
            assert cut > want_in.numel() // 2, f"the clamp cut only {cut}/{want_in.numel()} elements"
        assert bool(torch.isfinite(got_x).all())


@pytest.mark.parametrize("cfg", [0, 1])
def test_init_mode(cfg):
    """init writes the input image from x alone: x and the prediction are not touched, nothing of the step is applied"""
    for (B, H, W) in SHAPES:
        g = torch.Generator().manual_seed(77 + B + H)
        x = torch.randn(B, 4, H, W, generator=g) * 8e4                   # sigma_0 n: the clamp bites
        junk = torch.full((B, 4, H, W), float("nan")).to(torch.bfloat16)
        for a_in, clamp in ((1.0, 20000.0), (0.37, 0.0)):
            k = dict(cfg=cfg, init=1, a_skip=3.0, a_out=3.0, p=3.0, q=3.0, a_in_next=a_in, clamp=clamp, guidance=5.0, guidance_rescale=0.5)
            got_x, xin = run_hook(x, junk, junk if cfg else None, k)
            assert (bits(got_x) == bits(x)).all()
            check_image(xin, R.unet_input(x, a_in, clamp), B, H, W, cfg)


# ---------------------------------------------------------------------------------------------- 6. guidance rescale
@pytest.mark.parametrize("phi", [0.3, 0.7])
def test_guidance_rescale(phi):
    """two runs have the same bits; against the float64 restatement max |dx_next| <= 1e-5 max |x_next| per sample: the two tree sums
    over 65 536 elements carry <= ~20 roundings (1.2e-6 relative), the ratio doubles that, a handful of elementwise roundings follow"""
    k0, scale = _mode_step("ddpm_v")
    k = {key: (_f32(v) if isinstance(v, float) else v) for key, v in dict(k0, guidance_rescale=phi).items()}
    for (B, H, W) in ((2, 128, 128), (1, 8, 8), (4, 168, 96)):
        g = torch.Generator().manual_seed(5 + B)
        x = torch.randn(B, 4, H, W, generator=g) * scale
        fc = torch.randn(B, 4, H, W, generator=g).to(torch.bfloat16)
        fu = (0.8 * fc.float() + 0.3 * torch.randn(B, 4, H, W, generator=g)).to(torch.bfloat16)
        a_x, a_in = run_hook(x, fc, fu, k)
        b_x, b_in = run_hook(x, fc, fu, k)
        assert (bits(a_x) == bits(b_x)).all() and (bits(a_in) == bits(b_in)).all()
        want, _ = R.full_step(x.double(), fc.double(), fu.double(), k)
        plain, _ = R.full_step(x.double(), fc.double(), fu.double(), dict(k, guidance_rescale=0.0))
        for b in range(B):
            err, top = float((a_x[b].double() - want[b]).abs().max()), float(want[b].abs().max())
            print(f"rescale phi={phi} {(B, H, W)} sample {b}: max |dx| {err:.3e} = {err / top:.3e} of max |x_next| {top:.3e}")
            assert err <= 1e-5 * top
        assert float((want - plain).abs().max()) > 1e-2 * float(want.abs().max())      # the rescale does something here
        check_image(a_in, R.unet_input(a_x, k["a_in_next"], k["clamp"]), B, H, W, 1)


def test_guidance_rescale_zero_is_the_plain_step():
    k, scale = _mode_step("ddpm_v")
    g = torch.Generator().manual_seed(6)
    x = torch.randn(2, 4, 128, 128, generator=g) * scale
    fc, fu = (torch.randn(2, 4, 128, 128, generator=g).to(torch.bfloat16) for _ in range(2))
    want_x, want_in = R.full_step(x, fc.float(), fu.float(), dict(k, guidance_rescale=0.0))
    got_x, xin = run_hook(x, fc, fu, dict(k, guidance_rescale=0.0))
    assert (bits(got_x) == bits(want_x)).all()
    check_image(xin, want_in, 2, 128, 128, 1)


# ---------------------------------------------------------------------------------------------- 7. / 8. the whole sampler
def _tiny_net(w=None):
    from oracle import unet_ref as U
    cfg = U.tiny_config()
    net = NU.NativeUNet(NU.make_config(block_out_channels=cfg.block_out_channels, transformer_layers=cfg.transformer_layers_per_block,
                                       cross_attention_dim=cfg.cross_attention_dim,
                                       addition_time_embed_dim=cfg.addition_time_embed_dim, pooled_dim=cfg.pooled_dim))
    net.load_state_dict(U.synth_weights(cfg, seed=0) if w is None else w)
    return cfg, net


@pytest.fixture(scope="module")
def tiny():
    cfg, net = _tiny_net()
    yield cfg, net
    net.close()


def _cond(B, cross, pooled_dim, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)
    return (r(B, 77, cross).to(torch.bfloat16), r(B, pooled_dim).to(torch.bfloat16),
            torch.tensor([[8.0 * W, 8.0 * H, 0, 0, 8.0 * W, 8.0 * H]] * B), r(B, 4, H, W))


def python_loop(net, sampler, pe, po, ti, noise, num_steps, guidance_scale):
    """the same sampler as a Python loop: the existing unet_forward on the [cond; uncond] batch, _sampler_ref between the calls"""
    B = pe.shape[0]
    x0_scale, steps = sampler.schedule(num_steps)
    cfg = guidance_scale != 1.0
    pe2 = torch.cat([pe, torch.zeros_like(pe)]) if cfg else pe
    po2 = torch.cat([po, torch.zeros_like(po)]) if cfg else po
    ti2 = torch.cat([ti, ti]) if cfg else ti

    def model(inp, t, _j):
        PB = 2 * B if cfg else B
        out = net.unet_forward(torch.cat([inp, inp]) if cfg else inp, torch.full((PB,), t), pe2, po2, ti2).cpu()
        return (out[:B], out[B:]) if cfg else out
    return R.sample_loop(model, noise, x0_scale, steps, guidance_scale, 0.0)


@pytest.mark.parametrize("kind", [("ddpm", "trained"), ("ddpm", "reference"), ("flow_matching", "trained")])
def test_sample_equals_python_loop_tiny(tiny, kind):
    cfg, net = tiny
    B, H, W = 2, 16, 16
    pe, po, ti, noise = _cond(B, cfg.cross_attention_dim, cfg.pooled_dim, H, W, 11)
    sampler = S.NativeSampler(net, kind[0], "v_prediction", True, kind[1])
    want = python_loop(net, sampler, pe, po, ti, noise, 4, 5.0)
    got = sampler.sample(pe, po, ti, height=H, width=W, num_steps=4, guidance_scale=5.0, noise=noise)
    again = sampler.sample(pe, po, ti, height=H, width=W, num_steps=4, guidance_scale=5.0, noise=noise)
    torch.cuda.synchronize()
    assert got.dtype == torch.float32 and got.is_cuda and tuple(got.shape) == (B, 4, H, W) and bool(torch.isfinite(got).all())
    bad = int((bits(got) != bits(want)).sum())
    assert bad == 0, f"{kind}: {bad}/{want.numel()} elements differ from the Python loop (max |d| {float((got.cpu() - want).abs().max()):.3e})"
    assert (bits(again) == bits(got)).all()
    assert net._cur[0] == 2 * B
    # without guidance the plan runs at B
    one = sampler.sample(pe, po, ti, height=H, width=W, num_steps=4, guidance_scale=1.0, noise=noise)
    assert net._cur[0] == B and (bits(one) == bits(python_loop(net, sampler, pe, po, ti, noise, 4, 1.0))).all()
    # the caller's noise is not the state
    assert (bits(noise) == bits(_cond(B, cfg.cross_attention_dim, cfg.pooled_dim, H, W, 11)[3])).all()


def test_sample_equals_python_loop_full_size():
    """SDXL-base shapes, B = 2 with guidance (plan batch 4) at 128 x 128: init + 2 steps"""
    from sdxl_amd import synth
    net = NU.NativeUNet(NU.make_config())
    try:
        synth.load_synthetic(net, seed=0)
        B, H, W = 2, 128, 128
        pe, po, ti, noise = _cond(B, 2048, 1280, H, W, 12)
        sampler = S.NativeSampler(net, "ddpm", "v_prediction", True, "trained")
        got = sampler.sample(pe, po, ti, height=H, width=W, num_steps=2, guidance_scale=5.0, noise=noise)
        torch.cuda.synchronize()
        assert net._cur == (4, H, W, 77) and bool(torch.isfinite(got).all())
        want = python_loop(net, sampler, pe, po, ti, noise, 2, 5.0)
        bad = int((bits(got) != bits(want)).sum())
        assert bad == 0, f"{bad}/{want.numel()} elements differ from the Python loop"
    finally:
        net.close()


def test_forward_argument_errors(tiny):
    """cfg with an odd plan batch, x == NULL and a non-finite scalar return 1 before anything is launched"""
    cfg, net = tiny
    pe, po, ti, noise = _cond(3, cfg.cross_attention_dim, cfg.pooled_dim, 16, 16, 13)
    x = noise.to(dev())
    args = (pe.to(dev()), po.to(dev()), ti.to(dev()), torch.zeros(3, device=dev()))
    with pytest.raises(ValueError):
        net.sample_step(x, *args, cfg=1, a_skip=1.0, a_out=1.0, p=1.0, q=0.0)          # 3 rows cannot be [cond; uncond] of x
    net.plan(3, 16, 16, 77)
    L = net.L
    b = lib.SamplerBatch(3, 16, 16, 77, None, None, None, *[t.data_ptr() for t in (args[3], args[0], args[1], args[2])], None)
    for s, msg in ((lib.SamplerStep(x.data_ptr(), 1, 0, 1.0, 1.0, 1.0, 0.0, 1.0, 0.0, 1.0, 0.0), b"even batch"),
                   (lib.SamplerStep(None, 0, 0, 1.0, 1.0, 1.0, 0.0, 1.0, 0.0, 1.0, 0.0), b"x is NULL"),
                   (lib.SamplerStep(x.data_ptr(), 0, 0, float("inf"), 1.0, 1.0, 0.0, 1.0, 0.0, 1.0, 0.0), b"not finite")):
        b.sampler = C.pointer(s)
        assert L.sdxl_unet_forward(net.h, None, C.byref(b), None, stream()) == 1 and msg in L.sdxl_last_error()
    torch.cuda.synchronize()
    assert (bits(x) == bits(noise)).all()


# ---------------------------------------------------------------------------------------------- 9. the trainer
def _batch(cfg, B, seed):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)
    bfr = lambda t: t.to(torch.bfloat16).float()
    return {"vae_latents": r(B, 4, 16, 16), "prompt_embeds": bfr(r(B, 77, cfg.cross_attention_dim)),
            "pooled_prompt_embeds": bfr(r(B, cfg.pooled_dim)), "time_ids": torch.tensor([[[128.0, 128, 0, 0, 128, 128]]] * B),
            "metadata": {}}


def _config(use_ema):
    c = CFG.Config()
    c.training.method = "ddpm"
    c.training.use_ema, c.training.ema_update_after_step = use_ema, 0
    c.optimizer.learning_rate = 1e-3
    c.training.validation_num_steps, c.training.validation_guidance_scale = 3, 5.0
    return c


def _train_step(tr, cfg, i):
    b = _batch(cfg, 2, 40 + i)
    noise = torch.randn(2, 4, 16, 16, generator=torch.Generator().manual_seed(60 + i))
    loss, _m = tr._execute_training_step(b, timesteps=torch.tensor([200 + 100 * i, 700 - 50 * i]), noise=noise)
    tr.optimizer_step()
    torch.cuda.synchronize()
    return float(loss)


@pytest.mark.parametrize("use_ema", [False, True])
def test_trainer_sampling_leaves_training_bitwise_unaffected(tiny, use_ema):
    """step, [sample / evaluate on the trained and, with use_ema, on the EMA weights], step == step, step: the losses, the weights,
    the optimizer state and the EMA have the same bits; and the EMA results equal a separate UNet loaded with the bf16 EMA"""
    cfg, net = tiny
    arena0 = net.weights.clone()
    pe, po, ti, noise = _cond(2, cfg.cross_attention_dim, cfg.pooled_dim, 16, 16, 21)
    held = [_batch(cfg, 2, 90)]

    def run(between):
        net.weights.copy_(arena0)
        net.grads.zero_()
        class M: unet = net
        tr = T.NativeSDXLTrainer(M(), config=_config(use_ema))
        losses = [_train_step(tr, cfg, i) for i in range(3)]
        extra = between(tr) if between is not None else None
        losses += [_train_step(tr, cfg, 3)]
        state = [net.weights.clone()] + [a.clone() for a in tr.optimizer.state_arenas()] + ([tr.ema.arena.clone()] if use_ema else [])
        if use_ema:
            tr.ema.close()
        return losses, state, extra

    def between(tr):
        out = {"trained": tr.sample(pe, po, ti, height=16, width=16, noise=noise, weights="trained").clone()}
        out["trained_eval"] = tr.evaluate(held, [100, 800], torch.Generator().manual_seed(3))
        if use_ema:
            out["ema"] = tr.sample(pe, po, ti, height=16, width=16, noise=noise, weights="ema").clone()
            out["default"] = tr.sample(pe, po, ti, height=16, width=16, noise=noise).clone()      # validation_weights: ema with use_ema
            out["ema_eval"] = tr.evaluate(held, [100, 800], torch.Generator().manual_seed(3), weights="ema")
            sd = {k: v.to(torch.bfloat16) for k, v in tr.ema_state_dict().items()}
            _c, net2 = _tiny_net(sd)
            try:
                class M2: unet = net2
                tr2 = T.NativeSDXLTrainer(M2(), config=_config(False))
                out["ema_want"] = tr2.sample(pe, po, ti, height=16, width=16, noise=noise).clone()
                out["ema_eval_want"] = tr2.evaluate(held, [100, 800], torch.Generator().manual_seed(3))
            finally:
                net2.close()
        torch.cuda.synchronize()
        return out

    try:
        l0, s0, _ = run(None)
        l1, s1, out = run(between)
        assert l0 == l1, (l0, l1)
        assert len(s0) == len(s1) and all((bits(a) == bits(b)).all() for a, b in zip(s0, s1))
        assert bool(torch.isfinite(out["trained"]).all())
        if use_ema:
            assert (bits(out["ema"]) == bits(out["ema_want"])).all() and (bits(out["default"]) == bits(out["ema"])).all()
            assert out["ema_eval"] == out["ema_eval_want"]
            assert not (bits(out["ema"]) == bits(out["trained"])).all() and out["ema_eval"] != out["trained_eval"]
    finally:
        net.weights.copy_(arena0)
        net.grads.zero_()


def test_train_loop_calls_on_validation(tiny):
    cfg, net = tiny
    arena0 = net.weights.clone()
    try:
        c = _config(False)
        c.training.validation_every_n_steps, c.training.gradient_accumulation_steps, c.training.validation_seed = 2, 1, 5
        class M: unet = net
        tr = T.NativeSDXLTrainer(M(), train_dataloader=[_batch(cfg, 2, s) for s in range(4)], config=c)
        vb = [{k: v for k, v in _batch(cfg, 2, 91).items() if k != "metadata"}]
        seen = []
        tr.train(1, validation_batches=vb, on_validation=lambda step, lat: seen.append((step, lat.clone())))
        assert [s for s, _ in seen] == [1, 3] and all(tuple(l.shape) == (2, 4, 16, 16) and bool(torch.isfinite(l).all()) for _, l in seen)
        assert not (bits(seen[0][1]) == bits(seen[1][1])).all()          # the same noise, other weights
    finally:
        net.weights.copy_(arena0)
        net.grads.zero_()


def test_zero1_ema_sampling_needs_prepare_checkpoint():
    """two ranks on one GPU over gloo (tests/_sampler_zero1_worker.py): sample / evaluate on the EMA raise RuntimeError before
    prepare_checkpoint() and work after it"""
    sys.path.insert(0, str(Path(__file__).resolve().parent))
    from test_gpu_multiproc import run_dist
    env = dict(os.environ, MASTER_ADDR="127.0.0.1")
    r = run_dist([str(ROOT / "tests" / "_sampler_zero1_worker.py")], 29683, env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "SAMPLER_ZERO1_OK" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
