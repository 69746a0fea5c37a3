"""Host side of the fp32 EMA of the weights (no GPU): the decay rule against tests/_ema_ref.py, the training.ema_* config keys, the
trainer and the drop-in building (or refusing) the EMA, the state round trip, what the fused optimizers hand the C ABI per piece,
and the C ABI's argument errors for the EMA fields."""
import ctypes as C
import importlib
import json
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import _ema_ref as R
import sdxl_amd  # noqa: F401
from sdxl_amd import lib
from _optim_common import StandInNet

T = importlib.import_module("sdxl-training-improvements_amd.trainer")
O = importlib.import_module("sdxl-training-improvements_amd.optimizer")
E = importlib.import_module("sdxl-training-improvements_amd.ema")
NM = importlib.import_module("sdxl-training-improvements_amd.native_mi355x")
CFG = importlib.import_module("sdxl-training-improvements_amd.config")


def _ema(**kw):
    return E.WeightEMA(StandInNet(), **kw)


# ---------------------------------------------------------------------------------------------- the rule
def test_decay_table_defaults():
    e = _ema()
    assert [e.decay(t) for t in (1, 2, 3, 4)] == [0.0, 2 / 11, 3 / 12, 4 / 13]
    for t in (1, 2, 3, 10, 100, 5000, 9999, 10_000, 10_001, 10 ** 6):
        assert e.decay(t) == R.get_decay(t), t
    assert e.decay(10 ** 6) == 0.9999                    # (1+k)/(10+k) passes 0.9999 at k = 89 991: clamped
    assert e.decay(89_000) < 0.9999


def test_decay_update_after_step():
    e = _ema(update_after_step=3)
    assert [e.decay(t) for t in range(1, 8)] == [0.0, 0.0, 0.0, 0.0, 2 / 11, 3 / 12, 4 / 13]
    assert all(e.decay(t) == R.get_decay(t, update_after_step=3) for t in range(1, 200))


@pytest.mark.parametrize("inv_gamma,power", [(1.0, 2 / 3), (1.0, 3 / 4), (2.5, 0.5)])
def test_decay_warmup_closed_form(inv_gamma, power):
    e = _ema(use_ema_warmup=True, inv_gamma=inv_gamma, power=power, decay=0.9999)
    assert e.decay(1) == 0.0
    for k in (1, 2, 7, 100, 1234):
        want = min(1 - (1 + k / inv_gamma) ** -power, 0.9999)
        assert e.decay(k + 1) == want == R.get_decay(k + 1, use_ema_warmup=True, inv_gamma=inv_gamma, power=power)
    assert e.decay(10 ** 9) == 0.9999


def test_decay_clamps():
    lo = _ema(min_decay=0.5)
    assert lo.decay(1) == 0.0                            # k = 0 returns 0 before the clamps
    assert lo.decay(2) == 0.5 and lo.decay(100) == 100 / 109
    hi = _ema(decay=0.3)
    assert hi.decay(2) == 2 / 11 and hi.decay(3) == 0.25 and hi.decay(4) == 0.3 and hi.decay(1000) == 0.3
    for t in range(1, 50):
        assert lo.decay(t) == R.get_decay(t, min_decay=0.5) and hi.decay(t) == R.get_decay(t, decay=0.3)
    with pytest.raises(ValueError):
        _ema(decay=0.4, min_decay=0.6)
    with pytest.raises(ValueError):
        _ema(update_after_step=-1)


def test_advance_counts_steps_and_rounds_omd_to_float32():
    e = _ema(update_after_step=1)
    got = [e.advance() for _ in range(4)]
    assert e.optimization_step == 4
    assert got == [1.0, 1.0, float(np.float32(1 - 2 / 11)), float(np.float32(1 - 3 / 12))]


def test_initial_arena_is_the_fp32_image_of_the_weights():
    net = StandInNet(100)
    e = E.WeightEMA(net)
    assert e.arena.dtype == torch.float32 and e.arena.numel() == 100 and e.arena.data_ptr() % 256 == 0
    assert torch.equal(e.arena, net.weights.float())


def test_ref_step_is_three_rounded_fp32_ops():
    g = torch.Generator().manual_seed(0)
    e0 = torch.randn(4096, generator=g)
    p = (e0 + torch.randn(4096, generator=g) * 1e-3).to(torch.bfloat16)
    omd = np.float32(1 - 0.9999)
    want = e0.numpy() - omd * (e0.numpy() - p.float().numpy())          # numpy float32: each op rounded on its own
    assert np.array_equal(R.step(e0.clone(), p, 0.9999).numpy(), want)


# ---------------------------------------------------------------------------------------------- config, trainer, drop-in
def test_yaml_keys(tmp_path):
    d = CFG.Config().training
    assert (d.use_ema, d.ema_decay, d.ema_min_decay, d.ema_update_after_step, d.ema_use_warmup, d.ema_inv_gamma, d.ema_power) == \
        (False, 0.9999, 0.0, 0, False, 1.0, 2 / 3)
    p = tmp_path / "c.yaml"
    p.write_text("training:\n  use_ema: true\n  ema_decay: 0.999\n  ema_min_decay: 0.1\n  ema_update_after_step: 100\n"
                 "  ema_use_warmup: true\n  ema_inv_gamma: 2.0\n  ema_power: 0.75\n  batch_size: 2\n")
    c = CFG.Config.from_yaml(p).training
    assert (c.use_ema, c.ema_decay, c.ema_min_decay, c.ema_update_after_step, c.ema_use_warmup, c.ema_inv_gamma, c.ema_power,
            c.batch_size) == (True, 0.999, 0.1, 100, True, 2.0, 0.75, 2)


def _trainer(optimizer=None, **tr):
    cfg = CFG.Config()
    for k, v in tr.items():
        setattr(cfg.training, k, v)
    return T.NativeSDXLTrainer(StandInNet(), optimizer=optimizer, device="cpu", config=cfg)


def test_use_ema_false_builds_no_ema():
    tr = _trainer()
    assert tr.ema is None and tr.optimizer.ema is None
    with pytest.raises(ValueError):
        tr.ema_state_dict()
    tr.save_ema_state("/nonexistent/never/written")     # no EMA: nothing to write


@pytest.mark.parametrize("kind", ["adamw_bf16", "adamw_schedule_free_kahan"])
def test_use_ema_builds_and_attaches(kind):
    cfg = CFG.Config()
    cfg.optimizer.optimizer_type = kind
    cfg.training.use_ema, cfg.training.ema_decay, cfg.training.ema_update_after_step = True, 0.995, 7
    cfg.training.ema_use_warmup, cfg.training.ema_inv_gamma, cfg.training.ema_power = True, 3.0, 0.5
    net = StandInNet()
    tr = T.NativeSDXLTrainer(net, device="cpu", config=cfg)
    assert isinstance(tr.ema, E.WeightEMA) and tr.optimizer.ema is tr.ema and isinstance(tr.optimizer, O.BY_TYPE[kind])
    assert tr.ema.settings() == {"decay": 0.995, "min_decay": 0.0, "update_after_step": 7, "use_ema_warmup": True,
                                 "inv_gamma": 3.0, "power": 0.5}
    assert torch.equal(tr.ema.arena, net.weights.float())


def test_non_fused_optimizer_with_use_ema_raises():
    sgd = torch.optim.SGD([torch.zeros(2, requires_grad=True)], lr=0.1)
    with pytest.raises(ValueError, match="fused"):
        _trainer(optimizer=sgd, use_ema=True)
    assert _trainer(optimizer=sgd).ema is None          # without the EMA the trainer still takes it


def test_dropin_copies_the_ema_keys():
    ref_cfg = SimpleNamespace(model=SimpleNamespace(model_type="sdxl"), optimizer=SimpleNamespace(optimizer_type="adamw_bf16"),
                              training=SimpleNamespace(method="native_mi355x", gradient_accumulation_steps=1, use_ema=True,
                                                       ema_decay=0.9995, ema_min_decay=0.2, ema_update_after_step=4,
                                                       ema_use_warmup=True, ema_inv_gamma=1.5, ema_power=0.6))
    tr = NM.NativeMI355XTrainer(model=SimpleNamespace(unet=StandInNet()), optimizer=None, device="cpu", config=ref_cfg)
    assert tr.ema is not None and tr.optimizer.ema is tr.ema
    assert tr.ema.settings() == {"decay": 0.9995, "min_decay": 0.2, "update_after_step": 4, "use_ema_warmup": True,
                                 "inv_gamma": 1.5, "power": 0.6}
    ref_cfg.training = SimpleNamespace(method="native_mi355x", gradient_accumulation_steps=1)      # no key: off
    assert NM.NativeMI355XTrainer(model=SimpleNamespace(unet=StandInNet()), device="cpu", config=ref_cfg).ema is None


# ---------------------------------------------------------------------------------------------- state
def test_state_round_trip_and_mismatch():
    a = _ema(decay=0.999, update_after_step=2, use_ema_warmup=True)
    for _ in range(5):
        a.advance()
    sd = json.loads(json.dumps(a.state_dict()))          # what ema.json holds
    assert sd["optimization_step"] == 5 and sd["param_elems"] == 64
    b = _ema(decay=0.999, update_after_step=2, use_ema_warmup=True)
    b.load_state_dict(sd)
    assert b.optimization_step == 5 and b.advance() == a.advance()
    with pytest.raises(ValueError, match="settings"):
        _ema(decay=0.9999, update_after_step=2, use_ema_warmup=True).load_state_dict(sd)
    with pytest.raises(ValueError, match="settings"):
        _ema(decay=0.999, update_after_step=2).load_state_dict(sd)
    with pytest.raises(ValueError, match="elements"):
        E.WeightEMA(StandInNet(72), decay=0.999, update_after_step=2, use_ema_warmup=True).load_state_dict(sd)
    with pytest.raises(ValueError):
        b.load_state_dict({**sd, "optimization_step": -1})


class LayoutNet(StandInNet):
    """a stand-in with two named tensors in its 64-element arena (what load_ema_state checks a checkpoint against)"""

    param_table = {"a.weight": (4, 8), "b.bias": (32,)}

    def param_ranges(self):
        return {"a.weight": (0, 32), "b.bias": (32, 32)}


def test_refused_ema_checkpoint_leaves_the_ema_as_it_was(tmp_path):
    """load_ema_state checks the settings, the keys and the shapes before it changes anything, and sets the step count last"""
    from safetensors.torch import save_file
    cfg = CFG.Config()
    cfg.training.use_ema = True
    tr = T.NativeSDXLTrainer(LayoutNet(), device="cpu", config=cfg)
    e = tr.ema
    e.advance(), e.advance()
    e.arena.add_(1.0)                                    # an EMA that is not the weights' image
    before = e.arena.clone()
    (tmp_path / "unet_ema").mkdir()
    st = tmp_path / "unet_ema" / "diffusion_pytorch_model.safetensors"
    good = {"a.weight": torch.ones(4, 8), "b.bias": torch.ones(32)}
    cases = [({**e.state_dict(), "optimization_step": 50}, {"a.weight": torch.ones(4, 8), "b.bias": torch.ones(33)}, ValueError),
             ({**e.state_dict(), "optimization_step": 50}, {"a.weight": torch.ones(4, 8)}, KeyError),
             ({**e.state_dict(), "optimization_step": 50, "decay": 0.5}, good, ValueError),
             ({**e.state_dict(), "optimization_step": 50, "param_elems": 72}, good, ValueError)]
    for state, tensors, exc in cases:
        (tmp_path / "ema.json").write_text(json.dumps(state))
        save_file(tensors, str(st))
        with pytest.raises(exc):
            tr.load_ema_state(tmp_path)
        assert e.optimization_step == 2 and torch.equal(e.arena, before)


@pytest.mark.parametrize("cls", [O.AdamWBF16, O.AdamWScheduleFreeKahanBF16])
def test_attach_ema_refuses_an_arena_that_does_not_cover_the_weights(cls):
    o = cls(StandInNet(64))
    wrong_dtype = E.WeightEMA(StandInNet(64))
    wrong_dtype.arena = wrong_dtype.arena.double()
    for bad in (E.WeightEMA(StandInNet(72)), SimpleNamespace(param_elems=64), wrong_dtype):
        with pytest.raises(ValueError, match="attach_ema"):
            o.attach_ema(bad)
        assert o.ema is None
    good = E.WeightEMA(o.net)
    o.attach_ema(good)
    assert o.ema is good
    o.attach_ema(None)
    assert o.ema is None


# ---------------------------------------------------------------------------------------------- what reaches the C ABI
class RecordingLib:
    """stands in for libsdxlstep: records the EMA fields of every sdxl_adamw_bf16_step call"""

    def __init__(self):
        self.calls = []

    def sdxl_adamw_default_config(self, cfg_ref):
        return 0

    def sdxl_adamw_bf16_step(self, p, g, gdt, m, v, shift, n, cfg_ref, scale, rand, st):
        c = cfg_ref._obj
        self.calls.append((p.value, n, c.elem_offset, c.ema, c.ema_one_minus_decay, c.algorithm))
        return 0


@pytest.mark.parametrize("cls", [O.AdamWBF16, O.AdamWScheduleFreeKahanBF16])
def test_optimizer_hands_the_ema_piece_by_piece(cls):
    L = RecordingLib()
    net = StandInNet(128, L)
    o = cls(net)
    o.step(grads=torch.zeros(128))
    assert L.calls[-1][3] is None                        # no EMA attached: NULL
    ema = E.WeightEMA(net, update_after_step=1)
    o.attach_ema(ema)
    o.step(grads=torch.zeros(128))
    base = ema.arena.data_ptr()
    assert L.calls[-1][3] == base and L.calls[-1][4] == 1.0 and ema.optimization_step == 1
    L.calls.clear()
    pieces = [(0, 16, 0), (64, 32, 16), (120, 8, 48)]
    o.step(grads=torch.zeros(56), pieces=pieces)
    assert [c[3] for c in L.calls] == [base + 4 * off for off, _n, _g in pieces]
    assert [c[1] for c in L.calls] == [16, 32, 8]
    assert {c[4] for c in L.calls} == {1.0} and ema.optimization_step == 2     # one EMA step per optimizer step, t = 2 -> k = 0
    L.calls.clear()
    o.step(grads=torch.zeros(128))
    assert L.calls[-1][4] == float(np.float32(1 - 2 / 11))


def test_c_abi_ema_argument_errors():
    L = lib.load()
    cfg = lib.AdamWConfig()
    assert L.sdxl_adamw_default_config(C.byref(cfg)) == 0
    assert cfg.ema is None and cfg.ema_one_minus_decay == 0.0
    buf = (C.c_char * 512)()
    p16 = C.c_void_p((C.addressof(buf) + 15) & ~15)
    for algorithm in (0, 1):
        cfg.algorithm = algorithm
        cfg.ema = p16.value
        for bad in (-0.5, 1.5, float("nan")):
            cfg.ema_one_minus_decay = bad
            assert L.sdxl_adamw_bf16_step(p16, p16, 0, p16, p16, p16, 8, C.byref(cfg), None, None, None) == 1
            assert b"ema_one_minus_decay" in L.sdxl_last_error()
        cfg.ema_one_minus_decay = 0.5
        cfg.ema = p16.value + 4                          # not 16-byte aligned
        assert L.sdxl_adamw_bf16_step(p16, p16, 0, p16, p16, p16, 8, C.byref(cfg), None, None, None) == 1
        assert b"aligned" in L.sdxl_last_error()
