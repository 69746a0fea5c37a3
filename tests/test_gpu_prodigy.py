"""The fused Prodigy update on the GPU (csrc/optimizer.hip prodigy_* kernels): algorithm 2 of sdxl_adamw_bf16_step on caller buffers
against the restatement of tests/_prodigy_ref.py (element arenas and the scalar recurrence bit for bit, the two sums within the bound of
the documented summation order), operand isolation, and ProdigyBF16 in the full and the LoRA trainer on the tiny UNet."""
import ctypes as C
import importlib
import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import _prodigy_ref as R
import sdxl_amd  # noqa: F401
from oracle import unet_ref as U
from sdxl_amd import lib
from sdxl_amd import unet as NU
from _isolation import Spec, assert_isolated, run_isolated, same_bits
from _optim_common import bits, dev, ptr, stream

pytestmark = pytest.mark.gpu

O = importlib.import_module("sdxl-training-improvements_amd.optimizer")
T = importlib.import_module("sdxl-training-improvements_amd.trainer")
CFG = importlib.import_module("sdxl-training-improvements_amd.config")

SIZES = [8, 2056, 262152, R.MAX_GRID * 2048 + 8]          # one vector; one workgroup and one vector; 129 workgroups; a second sweep
EMA_OMD = 0.25


@pytest.fixture(scope="module")
def L():
    return lib.load()


class Buffers:
    """the operands of one arena on the device, fresh: p ~ 0.05 randn, c = 0, p0 = p, zero moments, the state block at d0"""

    def __init__(self, n, hp, seed, ema=False):
        g = torch.Generator().manual_seed(seed)
        self.n, self.gen = n, g
        self.p = (torch.randn(n, generator=g) * 0.05).to(torch.bfloat16).to(dev())
        self.c = torch.zeros(n, dtype=torch.bfloat16, device=dev())
        self.p0 = self.p.clone()
        self.m, self.v, self.s = (torch.zeros(n, dtype=torch.float32, device=dev()) for _ in range(3))
        self.state = torch.zeros(R.STATE_FLOATS, dtype=torch.float32, device=dev())
        self.state[:8] = torch.from_numpy(R.fresh_state(hp.d0))
        self.ema = (self.p.float() + 0.01) if ema else None

    def arenas(self):
        return [self.p, self.c, self.p0, self.m, self.v, self.s, self.state[:8]] + ([self.ema] if self.ema is not None else [])

    def snapshot(self):
        torch.cuda.synchronize()
        return [t.clone() for t in self.arenas()]


def call(L, b, g, hp, k, scale=None):
    cfg = lib.AdamWConfig()
    lib.check(L.sdxl_adamw_default_config(C.byref(cfg)))
    cfg.algorithm, cfg.lr, cfg.beta1, cfg.beta2, cfg.eps, cfg.weight_decay = 2, hp.lr, hp.beta1, hp.beta2, hp.eps, hp.weight_decay
    cfg.grad_round_bf16 = int(hp.grad_round_bf16)
    cfg.beta3, cfg.d0, cfg.d_coef, cfg.growth_rate, cfg.prodigy_bc = hp.b3(), hp.d0, hp.d_coef, hp.growth_rate, hp.bc(k)
    cfg.safeguard_warmup = int(hp.safeguard_warmup)
    cfg.p0, cfg.s, cfg.prodigy_state = b.p0.data_ptr(), b.s.data_ptr(), b.state.data_ptr()
    if b.ema is not None:
        cfg.ema, cfg.ema_one_minus_decay = b.ema.data_ptr(), EMA_OMD
    return L.sdxl_adamw_bf16_step(ptr(b.p), ptr(g), 0 if g.dtype == torch.float32 else 1, ptr(b.m), ptr(b.v), ptr(b.c), b.n, C.byref(cfg),
                                  ptr(scale), None, stream())


def grads_of(b, steps, bf16=False, std=3.0):
    """g ~ 3 randn at every step: 3 (0.8 u + 0.6 z_k) with u drawn once and z_k per step, unit variance.  The share the steps have in common
    is what a loss gives consecutive gradients and what makes Prodigy's estimate move: with independent draws g.(p0 - x) sums to noise and d
    stays at d0 for all three steps, so that no branch of the finalize but `d_hat < d` would run."""
    u = torch.randn(b.n, generator=b.gen)
    out = [(0.8 * u + 0.6 * torch.randn(b.n, generator=b.gen)) * std for _ in range(steps)]
    return [g.to(torch.bfloat16) if bf16 else g for g in out]


def assert_bits(got, want, what):
    got, want = got.cpu(), want.cpu()
    if not same_bits(got, want):
        ne = (got.view(torch.int32 if got.dtype == torch.float32 else torch.int16) != want.view(torch.int32 if want.dtype == torch.float32 else torch.int16))
        i = int(torch.nonzero(ne)[0])
        raise AssertionError(f"{what}: {int(ne.sum())} of {ne.numel()} elements differ, first at {i}: {float(got[i])!r} vs {float(want[i])!r}")


def checked_steps(L, n, hp, seed, steps=3, bf16_grads=False, scale=None, ema=False):
    """`steps` calls from a fresh state, assertions (a) .. (d) after each; returns the snapshots after every step, on the device"""
    b = Buffers(n, hp, seed, ema)
    grads = grads_of(b, steps, bf16_grads)
    sc = None if scale is None else torch.tensor([scale], dtype=torch.float32, device=dev())
    _grid, T_n = R.geometry(n)
    shots = []
    for k in range(steps):
        pre = [t.cpu() for t in b.snapshot()]
        p, c, p0, m, v, s, st = pre[:7]
        st = st.numpy()
        lib.check(call(L, b, grads[k].to(dev()), hp, k, sc), "sdxl_adamw_bf16_step")
        shots.append(b.snapshot())
        post = [t.cpu() for t in shots[-1]]
        st1 = post[6].numpy()
        # (a) the moments and s, from the d read before the call
        m1, v1, s1, t, a = R.accumulate(p, c, p0, m, v, s, R.grad_in(grads[k], scale, hp), st[0], hp, hp.bc(k))
        for name, got, want in (("m", post[3], m1), ("v", post[4], v1), ("s", post[5], s1)):
            assert_bits(got, want, f"n={n} step {k + 1} {name}")
        # (b) the two sums against float64 sums over those elements
        for name, got, terms in (("A", st1[6], t), ("Bs", st1[3], a)):
            ref, mag = float(terms.double().sum()), float(terms.double().abs().sum())
            bound = (T_n + 32) * 2.0 ** -24 * mag
            print(f"n={n} step {k + 1} {name}: {float(got)!r} vs {ref!r}, |diff| {abs(float(got) - ref):.3e} <= {bound:.3e}")
            assert abs(float(got) - ref) <= bound
        # (c) the scalar recurrence from the sums read back
        want = R.finalize(st, st1[6], st1[3], hp, hp.bc(k))
        assert (st1.view(np.int32) == want.view(np.int32)).all(), f"n={n} step {k + 1} state {st1} vs {want}"
        # (d) the parameters from the dlr and d' read back
        p1, c1 = R.apply(p, c, m1, v1, st1[0], st1[5], hp)
        assert_bits(post[0], p1, f"n={n} step {k + 1} p")
        assert_bits(post[1], c1, f"n={n} step {k + 1} c")
        assert_bits(post[2], p0, f"n={n} step {k + 1} p0")
        if ema:
            assert_bits(post[7], R.ema_step(pre[7], p1, EMA_OMD), f"n={n} step {k + 1} ema")
    return shots


@pytest.mark.parametrize("n", SIZES)
def test_three_steps_equal_the_restatement_and_repeat(L, n):
    hp = R.Hyper()
    first = checked_steps(L, n, hp, seed=n % 1000)
    st = first[-1][6].cpu().numpy()
    assert st[0] > np.float32(hp.d0) and float((bits(first[-1][1]) != 0).mean()) > 0.5        # d has grown, the compensation is live
    # (e) a second fresh run gives the same bits in every buffer
    b = Buffers(n, hp, n % 1000)
    for k, g in enumerate(grads_of(b, 3)):
        lib.check(call(L, b, g.to(dev()), hp, k), "sdxl_adamw_bf16_step")
        for x, y in zip(b.snapshot(), first[k]):
            assert same_bits(x, y)


VARIANTS = {
    "bf16_grads": (dict(), dict(bf16_grads=True)),
    "grad_scale": (dict(), dict(scale=0.25)),
    "grad_round_bf16": (dict(grad_round_bf16=True), dict(scale=0.37)),
    "weight_decay": (dict(weight_decay=0.1), dict()),
    "growth_rate": (dict(growth_rate=1.02), dict()),
    "d_coef": (dict(d_coef=2.0), dict()),
    "safeguard_warmup": (dict(safeguard_warmup=True, lr=0.5), dict()),
    "bias_correction": (dict(use_bias_correction=True), dict()),
    "ema": (dict(), dict(ema=True)),
}


@pytest.mark.parametrize("name", list(VARIANTS))
def test_variants_equal_the_restatement(L, name):
    hyper, run = VARIANTS[name]
    hp = R.Hyper(**hyper)
    shots = checked_steps(L, 2056, hp, seed=7, **run)
    ds = [np.float32(float(s[6][0])) for s in shots]
    d0 = np.float32(hp.d0)
    assert all(b >= a for a, b in zip([d0] + ds, ds))
    if name == "growth_rate":                             # step 2 leaves d0 by the max (d == d0), step 3 is clamped: d' = d * 1.02 < d_max'
        assert ds[0] == d0 and ds[1] > d0 and ds[2] == np.float32(ds[1] * np.float32(1.02)) and float(shots[2][6][1]) > ds[2]
    if name == "d_coef":                                  # the first estimate above d0 is twice the plain one
        plain = [float(s[6][0]) for s in checked_steps(L, 2056, R.Hyper(), seed=7)]
        assert ds[1] > d0 and float(ds[1]) == pytest.approx(2 * plain[1], rel=1e-5)


def test_zero_gradients_leave_d_and_p(L):
    hp = R.Hyper()
    b = Buffers(2056, hp, 3)
    before = b.snapshot()
    for k in range(2):
        assert call(L, b, torch.zeros(2056, device=dev()), hp, k) == 0
    after = b.snapshot()
    assert all(bool(torch.isfinite(t.float()).all()) for t in after)
    st = after[6].cpu().numpy()
    assert st[0] == st[1] == st[4] == np.float32(hp.d0) and st[3] == 0 and st[5] == np.float32(hp.d0)      # Bs = 0: d, d_max unchanged, d_hat = d
    assert same_bits(after[0], before[0]) and float(after[3].abs().max()) == 0 and float(after[5].abs().max()) == 0


def test_lr_zero_changes_nothing(L):
    hp = R.Hyper(lr=0.0)
    b = Buffers(2056, hp, 4)
    b.m.fill_(0.5); b.s.fill_(-0.25); b.state[8:].fill_(7.0)
    before = b.snapshot() + [b.state.clone()]
    assert call(L, b, grads_of(b, 1)[0].to(dev()), hp, 0) == 0
    for x, y in zip(b.snapshot() + [b.state.clone()], before):
        assert same_bits(x, y)


def test_operand_isolation(L):
    """guard bands and the three fill patterns around every buffer, the state block included; its scratch part starts as NaN, so a partial
    sum that is read before it is written shows"""
    n, hp = 2056, R.Hyper(weight_decay=0.1)
    grid, _T = R.geometry(n)
    g0 = torch.Generator().manual_seed(5)
    r = lambda std: torch.randn(1, n, generator=g0) * std
    p = r(0.05)
    state = torch.full((R.STATE_FLOATS, 1), math.nan)
    state[:8, 0] = torch.tensor([3e-4, 3e-4, 2.0, 0.0, 0.0, 0.0, 0.0, 0.0])
    specs = [Spec("p", 1, n, init=p, role="inout"), Spec("c", 1, n, init=r(1e-4), role="inout"), Spec("p0", 1, n, init=p + r(1e-3)),
             Spec("g", 1, n, dtype=torch.float32, init=r(3.0)), Spec("m", 1, n, dtype=torch.float32, init=r(1e-4), role="inout"),
             Spec("v", 1, n, dtype=torch.float32, init=r(1e-4).abs(), role="inout"), Spec("s", 1, n, dtype=torch.float32, init=r(1e-3), role="inout"),
             Spec("ema", 1, n, dtype=torch.float32, init=r(0.05), role="inout"), Spec("scale", 1, 4, dtype=torch.float32, init=torch.full((1, 4), 0.5)),
             Spec("state", R.STATE_FLOATS, 1, dtype=torch.float32, init=state, role="inout")]

    def fn(a):
        cfg = lib.AdamWConfig()
        lib.check(L.sdxl_adamw_default_config(C.byref(cfg)))
        cfg.algorithm, cfg.lr, cfg.weight_decay = 2, hp.lr, hp.weight_decay
        cfg.beta3, cfg.d0, cfg.d_coef, cfg.growth_rate, cfg.prodigy_bc = hp.b3(), hp.d0, hp.d_coef, hp.growth_rate, 1.0
        cfg.p0, cfg.s, cfg.prodigy_state, cfg.ema, cfg.ema_one_minus_decay = a.ptr("p0"), a.ptr("s"), a.ptr("state"), a.ptr("ema"), EMA_OMD
        vp = lambda name: C.c_void_p(a.ptr(name))
        lib.check(L.sdxl_adamw_bf16_step(vp("p"), vp("g"), 0, vp("m"), vp("v"), vp("c"), n, C.byref(cfg), vp("scale"), None, stream()),
                  "sdxl_adamw_bf16_step")

    runs = run_isolated(fn, specs, device="cuda")
    assert_isolated(runs, rows={"state": slice(0, 8 + 2 * grid)}, what="prodigy")
    assert bool(torch.isnan(runs[0]["state"][8 + 2 * grid:]).all())                # nothing behind the partials of this grid is written
    assert float(runs[0]["state"][0]) != 3e-4 or float(runs[0]["state"][3]) > 0


# ---------------------------------------------------------------------------------------------- the trainers, tiny UNet
@pytest.fixture(scope="module")
def tiny():
    cfg = U.tiny_config()
    w = U.synth_weights(cfg, seed=0)
    net = NU.NativeUNet(NU.make_config(block_out_channels=cfg.block_out_channels, transformer_layers=cfg.transformer_layers_per_block,
                                       cross_attention_dim=cfg.cross_attention_dim, addition_time_embed_dim=cfg.addition_time_embed_dim,
                                       pooled_dim=cfg.pooled_dim))
    net.load_state_dict(w)
    torch.cuda.synchronize()
    w0 = net.weights.clone()
    yield cfg, net, w0
    net.close()


def make_batch(cfg, seed, B=2, H=16, W=16):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)
    bfr = lambda t: t.to(torch.bfloat16).float()
    return {"vae_latents": r(B, 4, H, W), "prompt_embeds": bfr(r(B, 77, cfg.cross_attention_dim)), "pooled_prompt_embeds": bfr(r(B, cfg.pooled_dim)),
            "time_ids": torch.tensor([[8.0 * H, 8.0 * W, 0, 0, 8.0 * H, 8.0 * W]] * B), "metadata": {}}


def make_trainer(net, lora, **training):
    c = CFG.Config()
    c.training.method = "ddpm"
    c.optimizer.optimizer_type, c.optimizer.learning_rate = "prodigy", 1.0
    assert c.training.clip_grad_norm == 1.0              # clipping on
    if lora:
        c.training.lora_rank = 4
    for k, v in training.items():
        setattr(c.training, k, v)
    tr = T.create_trainer(SimpleNamespace(unet=net), config=c)
    assert type(tr.optimizer) is O.ProdigyBF16
    return tr


def train(tr, cfg, first, last, save_at=None, save_dir=None):
    """optimizer steps first + 1 .. last on one batch; returns the losses.  Timestep 800: the MinSNR weight there leaves a loss of about
    0.09 and adapter gradients of about 1e-5 per element.  At timestep 500 (sigma about 30, weight about 1e-3) the adapter gradient's norm
    is 2e-9, so that sqrt(v) = d sqrt(1 - beta2) |g| lies below d eps in every element and the estimate cannot leave d0 within twenty steps:
    that is Prodigy's eps floor, the package's too, not something this update could pass or fail."""
    batch = make_batch(cfg, 41)
    noise = torch.randn(batch["vae_latents"].shape, generator=torch.Generator().manual_seed(42))
    ts = torch.full((2,), 800, dtype=torch.long)
    losses = []
    for s in range(first, last):
        loss, _m = tr._execute_training_step(batch, timesteps=ts, noise=noise)
        losses.append(float(loss))
        tr.optimizer_step()
        if save_at == s + 1:
            save_dir.mkdir(parents=True, exist_ok=True)
            if hasattr(tr, "lora"):
                tr.save_checkpoint(save_dir)
            else:
                tr.save_optimizer_state(save_dir)
                torch.save(tr.net.weights.cpu(), str(save_dir / "arena.pt"))
    torch.cuda.synchronize()
    return losses


def everything(tr):
    o = tr.optimizer
    return [t.clone() for t in (tr.net.weights, o.net.weights, o.exp_avg, o.exp_avg_sq, o.s, o.comp, o.p0, o.prodigy_state[:8])]


@pytest.mark.parametrize("kind", ["full", "lora"])
def test_twenty_steps_lower_the_loss_repeat_and_resume(tiny, tmp_path, kind):
    cfg, net, w0 = tiny
    lora = kind == "lora"
    try:
        tr = make_trainer(net, lora)
        losses = train(tr, cfg, 0, 20, save_at=10, save_dir=tmp_path / "ck")
        d = tr.optimizer.d()
        print(f"[prodigy {kind}] loss {losses[0]:.6f} -> {losses[-1]:.6f}, d {tr.optimizer.param_groups[0]['d0']:.1e} -> {d:.3e}")
        assert all(math.isfinite(x) for x in losses) and losses[-1] < losses[0]
        assert d > tr.optimizer.param_groups[0]["d0"] and tr.optimizer.step_count == 20
        first = everything(tr)
        assert not same_bits(first[0], w0)
        # a second run repeats bit for bit
        net.weights.copy_(w0)
        net.grads.zero_()
        tr2 = make_trainer(net, lora)
        assert train(tr2, cfg, 0, 20) == losses
        for a, b in zip(everything(tr2), first):
            assert same_bits(a, b)
        # the checkpoint after step 10 in a fresh trainer: steps 11 .. 20 as in the uninterrupted run
        net.grads.zero_()
        if lora:
            net.weights.copy_(w0)
            tr3 = make_trainer(net, lora)
            tr3.load_lora_state(tmp_path / "ck")
        else:
            net.weights.copy_(torch.load(str(tmp_path / "ck" / "arena.pt"), weights_only=True).to(net.weights.device))
            tr3 = make_trainer(net, lora)
            tr3.load_optimizer_state(tmp_path / "ck")
        assert tr3.optimizer.step_count == 10 and tr3.optimizer.d() > tr3.optimizer.param_groups[0]["d0"]
        assert train(tr3, cfg, 10, 20) == losses[10:]
        for a, b in zip(everything(tr3), first):
            assert same_bits(a, b)
    finally:
        net.set_trainable(None)
        net.weights.copy_(w0)
        net.grads.zero_()
        torch.cuda.synchronize()


def test_ema_follows_and_samples(tiny):
    cfg, net, w0 = tiny
    try:
        tr = make_trainer(net, False, use_ema=True, validation_weights="ema", validation_num_steps=2)
        assert tr.ema is not None and tr.optimizer.ema is tr.ema
        train(tr, cfg, 0, 5)
        e, wts = tr.ema.arena, net.weights.float()
        assert bool(torch.isfinite(e).all()) and not torch.equal(e, wts) and not torch.equal(e, w0.float())
        b = make_batch(cfg, 43)
        seen = []
        lat = tr.validate(5, [{k: v for k, v in b.items() if k != "metadata"}], on_validation=lambda step, x: seen.append(step))[0]
        trained = tr.sample(b["prompt_embeds"], b["pooled_prompt_embeds"], b["time_ids"], height=16, width=16, weights="trained",
                            generator=torch.Generator().manual_seed(int(tr.config.training.validation_seed)))
        torch.cuda.synchronize()
        assert seen == [5] and tuple(lat.shape) == (2, 4, 16, 16) and bool(torch.isfinite(lat).all()) and not torch.equal(lat, trained)
    finally:
        net.weights.copy_(w0)
        net.grads.zero_()
        torch.cuda.synchronize()
