"""Host side of the fused Prodigy optimizer (no GPU): the restatement on a quadratic, config keys, optimizer_type selection in the
full and the LoRA trainer, the shard_optimizer rule, the low-learning_rate warning, state round trip and refusals, and the C-ABI
argument errors of algorithm 2."""
import ctypes as C
import importlib
import logging
import math

import numpy as np
import pytest
import torch

import _prodigy_ref as R
import sdxl_amd  # noqa: F401
from sdxl_amd import lib
from _optim_common import StandInNet

T = importlib.import_module("sdxl-training-improvements_amd.trainer")
O = importlib.import_module("sdxl-training-improvements_amd.optimizer")
CFG = importlib.import_module("sdxl-training-improvements_amd.config")
LORA = importlib.import_module("sdxl-training-improvements_amd.lora")


# ---------------------------------------------------------------------------------------------- the restatement on a quadratic
def _quadratic(freeze_d: bool):
    """1/2 |x - x*|^2 in 64 dimensions from 0, 200 steps of the float64 form with the defaults: (loss / first loss, the d of every step)"""
    hp = R.Hyper()
    target = np.random.default_rng(0).standard_normal(64)
    x = np.zeros(64)
    x0, m, v, s, state = x.copy(), np.zeros(64), np.zeros(64), np.zeros(64), (hp.d0, hp.d0, 0.0)
    loss = lambda y: 0.5 * float(np.sum((y - target) ** 2))
    first, ds = loss(x), []
    for k in range(200):
        x, m, v, s, state = R.step64(x, x0, m, v, s, state, x - target, hp, k, freeze_d=freeze_d)
        ds.append(state[0])
    return loss(x) / first, ds


def test_restatement_minimises_a_quadratic_and_d_grows():
    rel, ds = _quadratic(False)
    print(f"loss / first loss {rel:.3e}, d {ds[0]:.3e} -> {ds[-1]:.3e}")
    assert rel < 1e-6
    assert all(b >= a for a, b in zip(ds, ds[1:])) and ds[-1] >= 1e4 * 1e-6
    frozen, fds = _quadratic(True)
    print(f"d frozen at d0: loss / first loss {frozen:.6f}")
    assert frozen > 0.99 and set(fds) == {1e-6}


def test_float32_restatement_follows_the_float64_form():
    """one step of the float32 element functions and the scalar recurrence against step64 on the same numbers"""
    hp = R.Hyper(weight_decay=0.1, use_bias_correction=True)
    g0 = torch.Generator().manual_seed(1)
    n = 4096
    p0 = (torch.randn(n, generator=g0) * 0.05).to(torch.bfloat16)
    g = torch.randn(n, generator=g0) * 3
    p = (p0.float() - 1e-3 * g).to(torch.bfloat16)        # x has moved down the gradient: g.(p0 - x) > 0, so d grows
    c = torch.zeros(n, dtype=torch.bfloat16)
    z = torch.zeros(n)
    st = R.fresh_state(hp.d0)
    m1, v1, s1, t, a = R.accumulate(p, c, p0, z, z, z, R.grad_in(g, None, hp), st[0], hp, hp.bc(0))
    st1 = R.finalize(st, np.float32(t.double().sum()), np.float32(a.double().sum()), hp, hp.bc(0))
    p1, c1 = R.apply(p, c, m1, v1, st1[0], st1[5], hp)
    x64, m64, v64, s64, (d64, _dm, num64) = R.step64(p.double().numpy(), p0.double().numpy(), np.zeros(n), np.zeros(n), np.zeros(n),
                                                    (float(st[0]), float(st[1]), 0.0), g.double().numpy(), hp, 0)
    assert st1[0] > 1e3 * st[0] and abs(st1[0] - d64) <= 1e-5 * d64 and abs(st1[2] - num64) <= 1e-5 * abs(num64)
    for got, want in ((m1, m64), (v1, v64), (s1, s64)):
        assert np.allclose(got.double().numpy(), want, rtol=1e-5, atol=0)
    x1 = p1.double().numpy() + c1.double().numpy()               # p' + c' carries x to about 2^-16 of its size
    assert np.max(np.abs(x1 - x64)) <= 2.0 ** -14 * np.max(np.abs(x64))
    assert R.geometry(8) == (1, 8) and R.geometry(2056) == (2, 8) and R.geometry(4096 * 2048 + 8) == (4096, 16)


# ---------------------------------------------------------------------------------------------- config, trainer
def test_yaml_keys_and_defaults(tmp_path):
    d = CFG.Config().optimizer
    assert (d.prodigy_d0, d.prodigy_d_coef, d.prodigy_growth_rate, d.prodigy_beta3, d.prodigy_use_bias_correction,
            d.prodigy_safeguard_warmup) == (1e-6, 1.0, math.inf, None, False, False)
    p = tmp_path / "c.yaml"
    p.write_text("optimizer:\n  optimizer_type: prodigy\n  learning_rate: 1.0\n  prodigy_d0: 1.0e-5\n  prodigy_d_coef: 2.0\n"
                 "  prodigy_growth_rate: 1.02\n  prodigy_beta3: 0.99\n  prodigy_use_bias_correction: true\n  prodigy_safeguard_warmup: true\n")
    c = CFG.Config.from_yaml(p).optimizer
    assert (c.optimizer_type, c.learning_rate, c.prodigy_d0, c.prodigy_d_coef, c.prodigy_growth_rate, c.prodigy_beta3,
            c.prodigy_use_bias_correction, c.prodigy_safeguard_warmup) == ("prodigy", 1.0, 1e-5, 2.0, 1.02, 0.99, True, True)


def _config(**opt):
    cfg = CFG.Config()
    cfg.optimizer.optimizer_type, cfg.optimizer.learning_rate = "Prodigy", 1.0
    for k, v in opt.items():
        setattr(cfg.optimizer, k, v)
    return cfg


def test_optimizer_type_selects_the_prodigy_class(caplog):
    with caplog.at_level(logging.WARNING):
        tr = T.NativeSDXLTrainer(StandInNet(), device="cpu", config=_config(prodigy_d0=1e-5, prodigy_d_coef=2.0, prodigy_growth_rate=1.02,
                                                                            prodigy_use_bias_correction=True, prodigy_safeguard_warmup=True,
                                                                            weight_decay=0.02))
    o = tr.optimizer
    assert type(o) is O.ProdigyBF16 and not caplog.records
    g = o.param_groups[0]
    assert (g["lr"], g["weight_decay"], g["d0"], g["d_coef"], g["growth_rate"], g["beta3"], g["use_bias_correction"], g["safeguard_warmup"]) == \
        (1.0, 0.02, 1e-5, 2.0, 1.02, math.sqrt(0.999), True, True)
    assert o.exp_avg.dtype == o.exp_avg_sq.dtype == o.s.dtype == torch.float32 and o.comp.dtype == o.p0.dtype == torch.bfloat16
    assert torch.equal(o.p0, tr.net.weights) and o.p0.data_ptr() != tr.net.weights.data_ptr()
    st = o.prodigy_state
    assert st.numel() == lib.PRODIGY_STATE_FLOATS == R.STATE_FLOATS and st[:2].tolist() == [np.float32(1e-5)] * 2 and float(st[2:].abs().sum()) == 0
    assert o.d() == float(np.float32(1e-5)) and o.step_count == 0
    assert o.prodigy_bc() == math.sqrt(1 - 0.999) / (1 - 0.9)
    o.step_count = 4
    assert o.prodigy_bc() == math.sqrt(1 - 0.999 ** 5) / (1 - 0.9 ** 5)
    assert O.ProdigyBF16(StandInNet()).prodigy_bc() == 1.0
    with pytest.raises(lib.SdxlError):                   # no library behind the stand-in, no fallback
        o.step()


def test_lora_trainer_selects_the_prodigy_class(caplog):
    from types import SimpleNamespace
    from test_host_lora import StandInNet as TinyTable     # the tiny UNet's parameter table on the CPU
    cfg = _config()
    cfg.training.lora_rank = 4
    with caplog.at_level(logging.WARNING):
        tr = T.create_trainer(SimpleNamespace(unet=TinyTable()), config=cfg, device="cpu")
    assert isinstance(tr, LORA.NativeLoRATrainer) and type(tr.optimizer) is O.ProdigyBF16 and not caplog.records
    assert tr.optimizer.net is tr.lora and tr.optimizer.exp_avg.numel() == tr.lora.param_elems
    assert torch.equal(tr.optimizer.p0, tr.lora.weights)


def test_shard_optimizer_rule():
    cfg = _config()
    cfg.training.shard_optimizer = True
    with pytest.raises(ValueError, match="training.shard_optimizer"):
        T.NativeSDXLTrainer(StandInNet(), device="cpu", config=cfg)
    for so in (None, False):                             # absent (or false): all-reduce, every rank runs the full update
        cfg.training.shard_optimizer = so
        tr = T.NativeSDXLTrainer(StandInNet(), device="cpu", config=cfg)
        assert not tr.sharded and type(tr.sync).__name__ == "GradSync"
    assert O.ProdigyBF16.ZERO1 is False and O.AdamWBF16.ZERO1 and O.AdamWScheduleFreeKahanBF16.ZERO1
    with pytest.raises(ValueError, match="pieces"):
        O.ProdigyBF16(StandInNet(L=object())).step(torch.zeros(8), pieces=[(0, 8, 0)])
    other = CFG.Config()                                 # the other algorithms keep their default: sharded
    other.training.shard_optimizer = True
    assert type(T.NativeSDXLTrainer(StandInNet(), device="cpu", config=other).optimizer) is O.AdamWBF16


@pytest.mark.parametrize("lr,warns", [(1e-6, True), (9e-3, True), (1e-2, False), (1.0, False)])
def test_low_learning_rate_warns_once(caplog, lr, warns):
    with caplog.at_level(logging.WARNING):
        T.NativeSDXLTrainer(StandInNet(), device="cpu", config=_config(learning_rate=lr))
    msgs = [r.getMessage() for r in caplog.records]
    assert len(msgs) == int(warns) and all("learning_rate" in m and "prodigy" in m for m in msgs)


def test_constructor_refuses_bad_settings():
    for kw in (dict(lr=-1.0), dict(beta3=1.0), dict(d0=0.0), dict(d_coef=0.0), dict(growth_rate=0.5), dict(weight_decay=-0.1), dict(betas=(0.9, 1.0))):
        with pytest.raises(ValueError):
            O.ProdigyBF16(StandInNet(), **kw)


# ---------------------------------------------------------------------------------------------- state
def test_state_dict_round_trip_and_refusals():
    a = O.ProdigyBF16(StandInNet(), weight_decay=0.01)
    for i, t in enumerate(a.state_arenas()):
        t.copy_(torch.arange(t.numel(), dtype=torch.float32) * (i + 1) + 1.0)
    a.p0.copy_(torch.arange(64, dtype=torch.float32) * 0.5)
    a.prodigy_state[:8] = torch.tensor([3e-4, 4e-4, 1.5, 2.5, 3e-4, 3e-4, -7.0, 0.0])
    a.step_count = 7
    sd = a.state_dict()
    assert sd["algorithm"] == "prodigy" and sd["state"]["prodigy_state"].numel() == 8
    assert set(sd["state"]) == {"step", "exp_avg", "exp_avg_sq", "comp", "s", "p0", "prodigy_state"}
    b = O.ProdigyBF16(StandInNet(), weight_decay=0.01)
    b.load_state_dict(sd)
    assert b.step_count == 7 and b.d() == a.d() == float(np.float32(3e-4))
    assert len(b.state_arenas()) == 4 and all(torch.equal(x, y) for x, y in zip(a.state_arenas(), b.state_arenas()))
    assert torch.equal(a.p0, b.p0) and torch.equal(a.prodigy_state, b.prodigy_state)
    for other in (O.ProdigyBF16(StandInNet(), d_coef=2.0), O.ProdigyBF16(StandInNet(), safeguard_warmup=True),
                  O.ProdigyBF16(StandInNet(), d0=1e-5), O.AdamWBF16(StandInNet()), O.AdamWScheduleFreeKahanBF16(StandInNet())):
        with pytest.raises(ValueError):
            other.load_state_dict(sd)
    for foreign in (O.AdamWBF16(StandInNet()).state_dict(), O.AdamWScheduleFreeKahanBF16(StandInNet()).state_dict()):
        with pytest.raises(ValueError):
            b.load_state_dict(foreign)


def test_attach_ema_checks_the_arena():
    E = importlib.import_module("sdxl-training-improvements_amd.ema")
    net = StandInNet()
    o = O.ProdigyBF16(net)
    ema = E.WeightEMA(net)
    o.attach_ema(ema)
    assert o.ema is ema
    with pytest.raises(ValueError):
        o.attach_ema(E.WeightEMA(StandInNet(n=72)))


# ---------------------------------------------------------------------------------------------- C ABI
def test_c_abi_argument_errors_for_algorithm_2():
    L = lib.load()
    cfg = lib.AdamWConfig()
    assert L.sdxl_adamw_default_config(C.byref(cfg)) == 0
    assert (cfg.beta3, cfg.d0, cfg.d_coef, cfg.growth_rate, cfg.prodigy_bc, cfg.safeguard_warmup, cfg.p0, cfg.s, cfg.prodigy_state) == \
        (0.0, 0.0, 0.0, 0.0, 0.0, 0, None, None, None)
    buf = (C.c_char * 512)()
    a16 = (C.addressof(buf) + 15) & ~15
    p16 = C.c_void_p(a16)
    odd = C.c_void_p(a16 + 4)

    def good():
        cfg.algorithm, cfg.lr, cfg.weight_decay = 2, 1.0, 0.0
        cfg.beta3, cfg.d0, cfg.d_coef, cfg.growth_rate, cfg.prodigy_bc = 0.99, 1e-6, 1.0, math.inf, 1.0
        cfg.p0, cfg.s, cfg.prodigy_state = a16, a16, a16
        cfg.ema = None

    def refused(what, **args):
        a = dict(p=p16, grad=p16, m=p16, v=p16, shift=p16, n=8, rand=None)
        a.update(args)
        rc = L.sdxl_adamw_bf16_step(a["p"], a["grad"], 0, a["m"], a["v"], a["shift"], a["n"], C.byref(cfg), None, a["rand"], None)
        msg = L.sdxl_last_error()
        assert rc == 1 and b"algorithm 2" in msg and what in msg, (what, rc, msg)

    cfg.algorithm = 2                                    # the default configuration: d0 = 0, no p0 / s / prodigy_state
    refused(b"algorithm 2")
    cfg.algorithm = 3                                    # the message that lists the known algorithms names 2
    refused(b"algorithm 3")
    good(); refused(b"rand_inject", rand=p16)
    for name in ("p", "grad", "m", "v", "shift"):
        good(); refused(b"missing", **{name: None})
        good(); refused(b"aligned", **{name: odd})
    for name in ("p0", "s", "prodigy_state"):
        good(); setattr(cfg, name, None); refused(b"missing")
        good(); setattr(cfg, name, a16 + 4); refused(b"aligned")
    good(); cfg.ema, cfg.ema_one_minus_decay = a16 + 4, 0.5; refused(b"aligned")
    good(); refused(b"multiple of 8", n=12)
    for name, bad in (("beta3", (-0.1, 1.0)), ("d0", (0.0, -1e-6)), ("d_coef", (0.0, -1.0)), ("growth_rate", (0.99, math.nan)),
                      ("prodigy_bc", (0.0, -1.0, math.inf, math.nan)), ("lr", (-1.0,)), ("weight_decay", (-0.1,))):
        for x in bad:
            good(); setattr(cfg, name, x); refused(name.encode())
    for name, x in (("beta1", 1.0), ("beta2", -0.1), ("eps", -1e-8)):
        good(); setattr(cfg, name, x); refused(b"hyper-parameters")
