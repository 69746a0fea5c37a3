"""Host side of the schedule-free Kahan AdamW (no GPU): config keys, optimizer_type selection in the trainer and the drop-in,
C-ABI argument errors of algorithm 1, state_dict round trip and tag refusal."""
import ctypes as C
import importlib
import logging
from types import SimpleNamespace

import pytest
import torch

import sdxl_amd  # noqa: F401
from sdxl_amd import lib
from _optim_common import StandInNet

T = importlib.import_module("sdxl-training-improvements_amd.trainer")
O = importlib.import_module("sdxl-training-improvements_amd.optimizer")
NM = importlib.import_module("sdxl-training-improvements_amd.native_mi355x")
CFG = importlib.import_module("sdxl-training-improvements_amd.config")


def test_yaml_keys(tmp_path):
    p = tmp_path / "c.yaml"
    p.write_text("optimizer:\n  optimizer_type: adamw_schedule_free_kahan\n  warmup_steps: 5\n  kahan_sum: false\n"
                 "  correct_bias: false\n  schedule_free_arithmetic: reference\n  learning_rate: 3.0e-6\n")
    c = CFG.Config.from_yaml(p).optimizer
    assert (c.optimizer_type, c.warmup_steps, c.kahan_sum, c.correct_bias, c.schedule_free_arithmetic, c.learning_rate) == \
        ("adamw_schedule_free_kahan", 5, False, False, "reference", 3e-6)
    d = CFG.Config().optimizer                            # defaults: the reference's, plus the compensated arithmetic
    assert (d.optimizer_type, d.warmup_steps, d.kahan_sum, d.correct_bias, d.schedule_free_arithmetic) == \
        ("adamw_bf16", 0, True, True, "compensated")


def _trainer(**opt):
    cfg = CFG.Config()
    for k, v in opt.items():
        setattr(cfg.optimizer, k, v)
    return T.NativeSDXLTrainer(StandInNet(), device="cpu", config=cfg)


def test_optimizer_type_selects_the_schedule_free_class(caplog):
    with caplog.at_level(logging.WARNING):
        tr = _trainer(optimizer_type="AdamW_Schedule_Free_Kahan", warmup_steps=3, kahan_sum=False,
                      schedule_free_arithmetic="Reference", weight_decay=0.02, learning_rate=5e-6)
    o = tr.optimizer
    assert type(o) is O.AdamWScheduleFreeKahanBF16 and not caplog.records
    g = o.param_groups[0]
    assert (g["lr"], g["weight_decay"], g["warmup_steps"], g["kahan_sum"], o.arithmetic) == (5e-6, 0.02, 3, False, "reference")
    assert o.kahan_comp is None and len(o.state_arenas()) == 2
    assert tr.sync is not None and isinstance(tr.optimizer, O.FusedArenaOptimizer)
    assert type(_trainer().optimizer) is O.AdamWBF16     # default unchanged


@pytest.mark.parametrize("kind", ["SOAP", "adamw", "lion"])
def test_unbuilt_optimizer_type_warns_and_uses_adamw_bf16(caplog, kind):
    with caplog.at_level(logging.WARNING):
        tr = _trainer(optimizer_type=kind)
    assert type(tr.optimizer) is O.AdamWBF16
    msg = " ".join(r.getMessage() for r in caplog.records)
    assert kind in msg and "AdamWBF16" in msg


def test_bad_arithmetic_is_refused():
    with pytest.raises(ValueError):
        O.AdamWScheduleFreeKahanBF16(StandInNet(), arithmetic="fp64")


def test_dropin_selects_from_the_reference_optimizer_class():
    class AdamWScheduleFreeKahan:                        # stand-in with the reference class's name
        param_groups = [{"lr": 2e-6, "betas": (0.8, 0.95), "eps": 1e-7, "weight_decay": 0.03, "warmup_steps": 9,
                         "kahan_sum": False}]
    ref_cfg = SimpleNamespace(model=SimpleNamespace(model_type="sdxl"), optimizer=SimpleNamespace(optimizer_type="adamw_bf16"),
                              training=SimpleNamespace(method="native_mi355x", gradient_accumulation_steps=1))
    net = StandInNet()
    tr = NM.NativeMI355XTrainer(model=SimpleNamespace(unet=net), optimizer=AdamWScheduleFreeKahan(), device="cpu", config=ref_cfg)
    o = tr.optimizer
    assert type(o) is O.AdamWScheduleFreeKahanBF16
    g = o.param_groups[0]
    assert (g["lr"], g["betas"], g["eps"], g["weight_decay"], g["warmup_steps"], g["kahan_sum"]) == (2e-6, (0.8, 0.95), 1e-7, 0.03, 9, False)
    # ... and from the reference config key, whatever optimizer object was handed in
    ref_cfg.optimizer = SimpleNamespace(optimizer_type="adamw_schedule_free_kahan", warmup_steps=4, kahan_sum=True)
    tr = NM.NativeMI355XTrainer(model=SimpleNamespace(unet=StandInNet()), optimizer=None, device="cpu", config=ref_cfg)
    assert type(tr.optimizer) is O.AdamWScheduleFreeKahanBF16 and tr.optimizer.param_groups[0]["warmup_steps"] == 4
    ref_cfg.optimizer = SimpleNamespace(optimizer_type="adamw_bf16")
    tr = NM.NativeMI355XTrainer(model=SimpleNamespace(unet=StandInNet()), optimizer=None, device="cpu", config=ref_cfg)
    assert type(tr.optimizer) is O.AdamWBF16


def test_c_abi_argument_errors_for_algorithm_1():
    L = lib.load()
    cfg = lib.AdamWConfig()
    assert L.sdxl_adamw_default_config(C.byref(cfg)) == 0
    assert (cfg.algorithm, cfg.kahan_sum, cfg.sf_reference, cfg.weight_decay, cfg.sf_step_size) == (0, 0, 0, 0.0, 0.0)
    buf = (C.c_char * 512)()
    p16 = C.c_void_p((C.addressof(buf) + 15) & ~15)
    rnd = C.c_void_p(C.addressof(buf))
    step = lambda shift=p16, rand=None, n=8: L.sdxl_adamw_bf16_step(p16, p16, 0, p16, p16, shift, n, C.byref(cfg), None, rand, None)
    cfg.algorithm = 2
    assert step() == 1 and b"algorithm" in L.sdxl_last_error()
    cfg.algorithm = -1
    assert step() == 1 and b"algorithm" in L.sdxl_last_error()
    cfg.algorithm, cfg.kahan_sum, cfg.sf_step_size = 1, 1, 1e-4
    assert step(rand=rnd) == 1 and b"rand_inject" in L.sdxl_last_error()
    assert step(shift=None) == 1 and b"kahan_comp" in L.sdxl_last_error()
    assert step(n=7) == 1 and b"multiple of 8" in L.sdxl_last_error()
    cfg.sf_step_size = -1.0
    assert step() == 1 and b"hyper-parameters" in L.sdxl_last_error()
    cfg.sf_step_size, cfg.weight_decay = 1e-4, -0.1
    assert step() == 1 and b"hyper-parameters" in L.sdxl_last_error()


def _filled(opt, base):
    for i, t in enumerate(opt.state_arenas()):
        t.copy_(torch.arange(t.numel(), dtype=torch.float32) * (i + 1) + base)
    return opt


def test_state_dict_round_trip_and_tag_refusal():
    net = StandInNet()
    a = _filled(O.AdamWScheduleFreeKahanBF16(net, lr=1e-4, warmup_steps=2), 1.0)
    a.step_count, a.lr_max, a.last_lr = 7, 3e-5, 2e-5
    sd = a.state_dict()
    assert (sd["algorithm"], sd["arithmetic"], sd["kahan_sum"]) == ("adamw_schedule_free_kahan", "compensated", True)
    b = O.AdamWScheduleFreeKahanBF16(StandInNet(), lr=1e-4, warmup_steps=2)
    b.load_state_dict(sd)
    assert b.step_count == 7 and (b.lr_max, b.get_last_lr()) == (3e-5, 2e-5)
    assert all(torch.equal(x, y) for x, y in zip(a.state_arenas(), b.state_arenas())) and len(b.state_arenas()) == 3
    assert b.schedule() == a.schedule()
    for other in (O.AdamWScheduleFreeKahanBF16(StandInNet(), arithmetic="reference"),
                  O.AdamWScheduleFreeKahanBF16(StandInNet(), kahan_sum=False)):
        with pytest.raises(ValueError):
            other.load_state_dict(sd)
    with pytest.raises(ValueError):
        O.AdamWBF16(StandInNet()).load_state_dict(sd)
    with pytest.raises(ValueError):
        b.load_state_dict(O.AdamWBF16(StandInNet()).state_dict())
    assert len(O.AdamWBF16(StandInNet()).state_arenas()) == 3
    b.eval(); b.train()                                  # no-ops, as in the reference
    with pytest.raises(lib.SdxlError):                   # no library, no fallback
        b.step()
