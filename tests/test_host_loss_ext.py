"""Per-sample loss weights, per-sample losses and Huber losses, host side (no GPU): the appended struct fields, the trainer's
recipes for the B floats each config key stands for (checked against hand-computed values with a stand-in net that records what
`forward_loss` receives), the CPU restatement of the formulas against itself, and `evaluate()`."""
import ctypes as C
import importlib

import pytest
import torch

import sdxl_amd  # noqa: F401
from sdxl_amd import lib

import _loss_ext_ref as X

T = importlib.import_module("sdxl-training-improvements_amd.trainer")
NM = importlib.import_module("sdxl-training-improvements_amd.native_mi355x")
CFG = importlib.import_module("sdxl-training-improvements_amd.config")

SIGMAS = [20000.0, 1.0, 0.002]


# ---------------------------------------------------------------------------------------------- 1. the structs
def test_structs_carry_the_appended_fields_zero_initialised():
    lc = lib.LossConfig(0, 1, 1, 5.0, 1)                       # the old positional construction (five fields)
    assert (lc.loss_type, lc.huber_c) == (0, 0.0)
    b = lib.Batch(2, 8, 8, 77, None, None, None, None, None, None, None, None)      # ... (twelve fields)
    assert b.sample_weights is None and b.huber_c is None and b.per_sample_loss is None
    names = [f[0] for f in lib.LossConfig._fields_]
    assert names[:5] == ["method", "prediction_type", "use_min_snr", "min_snr_gamma", "use_ztsnr"] and names[5:] == ["loss_type", "huber_c"]
    names = [f[0] for f in lib.Batch._fields_]
    assert names[11] == "tag_weights" and names[12:] == ["sample_weights", "huber_c", "per_sample_loss"]
    # appended at the end: no existing field moved
    assert lib.LossConfig.use_ztsnr.offset == 16 and lib.LossConfig.loss_type.offset == 20 and lib.LossConfig.huber_c.offset == 24
    assert lib.Batch.tag_weights.offset == 16 + 7 * C.sizeof(C.c_void_p)
    assert lib.Batch.sample_weights.offset == lib.Batch.tag_weights.offset + C.sizeof(C.c_void_p)
    lc2 = lib.LossConfig(0, 1, 1, 5.0, 1, lib.LOSS_TYPES["huber"], 0.25)
    assert (lc2.loss_type, lc2.huber_c) == (1, 0.25)
    assert lib.LOSS_TYPES == {"l2": 0, "huber": 1, "smooth_l1": 2}


def test_header_declares_the_fields_and_no_new_symbol():
    from pathlib import Path
    hdr = (Path(__file__).resolve().parent.parent / "include" / "sdxlstep.h").read_text()
    for field in ("int   loss_type;", "float huber_c;", "const float* sample_weights;", "const float* huber_c;", "float*       per_sample_loss;"):
        assert field in hdr, field
    assert hdr.count("SDXL_API int ") + hdr.count("SDXL_API const char* ") <= 58


# ---------------------------------------------------------------------------------------------- 2. the host recipes
class RecNet:
    """Records what the trainer asks of the native UNet (the FakeNet pattern of test_host_boundary.py)."""
    param_elems = 16
    device = "cpu"

    def __init__(self):
        self.calls = []
        self.grads = torch.zeros(16)
        self.weights = torch.zeros(16, dtype=torch.bfloat16)
        self.ps = None

    def zero_grads(self):
        self.calls.append(("zero",))

    def forward_loss(self, method, *a, **k):
        self.calls.append(("fwd", method, a, k))
        B = a[0].shape[0]
        self.ps = torch.arange(1, B + 1, dtype=torch.float32) * float(a[3].reshape(-1)[0] + 1) if k.get("per_sample_loss") else None

    def backward(self, scale, first, on_segment=None):
        self.calls.append(("bwd", round(scale, 6), first))

    def read_loss(self):
        return [0.5, 0, 8.0, 16.0, 4.0, 9.0, 25.0, 1.0]

    def read_per_sample_loss(self):
        assert self.ps is not None
        return self.ps.clone()

    def fwd(self, i=-1):
        return [c for c in self.calls if c[0] == "fwd"][i]


class CountingOpt:
    param_groups = [{"lr": 1e-6}]
    steps = 0

    def step(self, *a, **k):
        CountingOpt.steps += 1


def _batch(B=3, tag=None):
    b = {"vae_latents": torch.randn(B, 4, 8, 8), "prompt_embeds": torch.randn(B, 77, 16),
         "pooled_prompt_embeds": torch.randn(B, 8), "time_ids": torch.zeros(B, 1, 6), "metadata": {}}
    if tag is not None:
        b["tag_weights"] = torch.tensor(tag)
    return b


def _trainer(method="ddpm", model=None, **keys):
    cfg = CFG.Config()
    cfg.training.method = method
    for k, v in keys.items():
        setattr(cfg.model if k in ("min_snr_gamma",) else cfg.training, k, v)
    net = RecNet()

    class M:
        unet = net
    tr = T.NativeSDXLTrainer(M(), optimizer=None, train_dataloader=None, device="cpu", config=cfg)
    if method == "ddpm":                                   # sigma_b = SIGMAS[timestep]: timesteps [0, 1, 2] give all three
        tr.noise_scheduler.sigmas = torch.tensor(SIGMAS)
    return tr, net


TS = torch.tensor([0, 1, 2])


def _close(t, want, rel=1e-6):
    got = [float(v) for v in torch.as_tensor(t).reshape(-1)]
    assert len(got) == len(want) and all(abs(g - w) <= rel * abs(w) for g, w in zip(got, want)), (got, want)


def test_defaults_pass_none_and_leave_the_metric_keys():
    tr, net = _trainer()
    out = tr.compute_loss(_batch(tag=[1.0, 2.0, 3.0]), timesteps=TS)
    _m, method, a, k = net.fwd()
    assert k.get("sample_weights") is None and k.get("huber_c") is None and not k.get("per_sample_loss")
    assert k.get("loss_type", "l2") == "l2"
    assert torch.equal(a[7], torch.tensor([1.0, 2.0, 3.0]))                  # tag_weights: the reference's batch mean, as before
    assert set(out) == {"loss", "metrics"}
    assert set(out["metrics"]) == {"loss", "lr", "timestep_mean", "timestep_std", "noise_scale", "pred_scale", "batch_size"}
    tr2, net2 = _trainer("flow_matching")
    out = tr2.compute_loss(_batch(), timesteps=torch.tensor([0.2, 0.5, 0.9]))
    assert set(out) == {"loss", "metrics"} and not {"sample_weights", "huber_c", "loss_type", "per_sample_loss"} & set(net2.fwd()[3])
    assert set(out["metrics"]) == {"loss", "x0_norm", "x1_norm", "time_mean", "time_std", "velocity_norm", "batch_size", "lr"}


def test_debiased_snr_weighting_both_prediction_types():
    # snr = sigma^-2 : 2.5e-9, 1, 250000
    tr, net = _trainer(snr_weighting="debiased", prediction_type="v_prediction")
    tr.compute_loss(_batch(), timesteps=TS)
    _close(net.fwd()[3]["sample_weights"], [1.0 / (2.5e-9 + 1.0), 0.5, 1.0 / 250001.0])
    assert net.fwd()[3]["sample_weights"].dtype == torch.float32
    tr, net = _trainer(snr_weighting="debiased", prediction_type="epsilon")
    tr.compute_loss(_batch(), timesteps=TS)
    _close(net.fwd()[3]["sample_weights"], [4.0e8, 1.0, 4.0e-6])
    assert net.fwd()[3].get("huber_c") is None and net.fwd()[3].get("loss_type", "l2") == "l2"


def test_huber_schedules():
    tr, net = _trainer(loss_type="huber", huber_c=0.1, huber_schedule="snr")
    tr.compute_loss(_batch(), timesteps=TS)
    k = net.fwd()[3]
    assert k["loss_type"] == "huber" and k.get("sample_weights") is None
    # c_b = (1 - c) / (1 + sigma)^2 + c
    _close(k["huber_c"], [0.9 / 20001.0 ** 2 + 0.1, 0.9 / 4.0 + 0.1, 0.9 / 1.002 ** 2 + 0.1])
    tr, net = _trainer(loss_type="smooth_l1", huber_c=0.3)
    tr.compute_loss(_batch(), timesteps=TS)
    k = net.fwd()[3]
    assert k["loss_type"] == "smooth_l1" and k["huber_c"] == 0.3 and isinstance(k["huber_c"], float)
    tr, net = _trainer("flow_matching", loss_type="huber", huber_c=0.2)
    tr.compute_loss(_batch(), timesteps=torch.tensor([0.2, 0.5, 0.9]))
    assert net.fwd()[3]["loss_type"] == "huber" and net.fwd()[3]["huber_c"] == 0.2


def test_tag_weights_per_sample_routes_the_weights():
    tr, net = _trainer(tag_weights_per_sample=True)
    tr.compute_loss(_batch(tag=[1.0, 0.0, 2.5]), timesteps=TS)
    _m, _method, a, k = net.fwd()
    assert a[7] is None                                                       # no tag_weights: no batch mean on top
    _close(k["sample_weights"] + 1.0, [2.0, 1.0, 3.5])
    tr.compute_loss(_batch(), timesteps=TS)                                    # a batch without tag weights: nothing to route
    assert net.fwd()[2][7] is None and net.fwd()[3].get("sample_weights") is None
    tr2, net2 = _trainer("flow_matching", tag_weights_per_sample=True)
    tr2.compute_loss(_batch(tag=[1.0, 0.5, 2.0]), timesteps=torch.tensor([0.2, 0.5, 0.9]))
    assert net2.fwd()[2][7] is None
    _close(net2.fwd()[3]["sample_weights"], [1.0, 0.5, 2.0])


def test_sources_multiply():
    tr, net = _trainer(snr_weighting="debiased", tag_weights_per_sample=True, loss_type="huber", huber_schedule="snr", huber_c=0.5,
                       log_per_sample_loss=True)
    out = tr.compute_loss(_batch(tag=[2.0, 3.0, 0.5]), timesteps=TS)
    _m, _method, a, k = net.fwd()
    _close(k["sample_weights"], [2.0 / (2.5e-9 + 1.0), 1.5, 0.5 / 250001.0])
    _close(k["huber_c"], [0.5 / 20001.0 ** 2 + 0.5, 0.625, 0.5 / 1.002 ** 2 + 0.5])
    assert a[7] is None and k["per_sample_loss"] is True and k["loss_type"] == "huber"
    assert set(out) == {"loss", "metrics", "per_sample_loss", "timesteps"}
    assert out["per_sample_loss"].shape == (3,) and out["per_sample_loss"].device.type == "cpu" and torch.equal(out["timesteps"], TS)
    assert set(out["metrics"]) == {"loss", "lr", "timestep_mean", "timestep_std", "noise_scale", "pred_scale", "batch_size"}


@pytest.mark.parametrize("method,keys,match", [
    ("ddpm", dict(loss_type="l1"), "loss_type"),
    ("ddpm", dict(huber_schedule="exponential"), "huber_schedule"),
    ("ddpm", dict(snr_weighting="p2"), "snr_weighting"),
    ("ddpm", dict(loss_type="huber", huber_c=0.0), "huber_c"),
    ("ddpm", dict(snr_weighting="debiased", min_snr_gamma=None), "snr_weighting"),
    ("flow_matching", dict(huber_schedule="snr"), "huber_schedule"),
    ("flow_matching", dict(snr_weighting="debiased"), "snr_weighting"),
])
def test_bad_key_values_raise_when_the_trainer_is_built(method, keys, match):
    with pytest.raises(ValueError, match=match):
        _trainer(method, **keys)


def test_dropin_copies_the_keys():
    ref_cfg = {"training": {"method": "native_mi355x", "native_objective": "ddpm", "loss_type": "smooth_l1", "huber_c": 0.25,
                            "snr_weighting": "debiased", "tag_weights_per_sample": True, "log_per_sample_loss": True}}
    net = RecNet()

    class M:
        unet = net
    tr = NM.NativeMI355XTrainer(model=M(), optimizer=None, train_dataloader=None, device="cpu", config=ref_cfg)
    tc = tr.config.training
    assert (tc.loss_type, tc.huber_c, tc.snr_weighting, tc.tag_weights_per_sample, tc.log_per_sample_loss) == \
        ("smooth_l1", 0.25, "debiased", True, True)
    assert tr.loss_type == "smooth_l1" and tr.snr_weighting == "debiased"
    with pytest.raises(ValueError, match="loss_type"):
        NM.NativeMI355XTrainer(model=M(), device="cpu", config={"training": {"method": "native_mi355x", "loss_type": "cauchy"}})


# ---------------------------------------------------------------------------------------------- 3. the restatement against itself
def _ref_case(B=3, H=5, W=7, seed=0):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    return r(B, 4, H, W), r(B, 4, H, W), torch.rand(B, generator=g, dtype=torch.float64) + 0.5


def test_huber_tends_to_l2_for_large_c():
    pred, target, w = _ref_case()
    s = torch.tensor([1.0, 0.5, 2.0], dtype=torch.float64)
    l2 = X.loss(pred, target, w, s, "l2")
    hub = X.loss(pred, target, w, s, "huber", 1e6)
    assert abs(float(hub) - float(l2)) <= 1e-6 * float(l2)
    per2, perh = X.per_sample_loss(pred, target, w, s, "l2"), X.per_sample_loss(pred, target, w, s, "huber", 1e6)
    assert float(((perh - per2).abs() / per2).max()) <= 1e-6
    # ... and to 2 c |d| for |d| >> c ; smooth_l1 = huber / c
    d = torch.tensor([[[[1e4, -3e3]]]], dtype=torch.float64)
    assert torch.allclose(X.element_loss(d, "huber", 1e-3), 2e-3 * d.abs(), rtol=1e-6)
    assert torch.allclose(X.element_loss(d, "smooth_l1", 0.7) * 0.7, X.element_loss(d, "huber", 0.7), rtol=1e-12)
    # the stable form keeps small |d| (the plain difference sqrt(d^2 + c^2) - c would return 0 here)
    tiny = torch.tensor([[[[1e-9]]]], dtype=torch.float64)
    assert float(X.element_loss(tiny, "huber", 1.0)) == pytest.approx(1e-18, rel=1e-9)


@pytest.mark.parametrize("loss_type", X.LOSS_TYPES)
@pytest.mark.parametrize("per_sample_c", [False, True])
def test_autograd_equals_the_closed_form(loss_type, per_sample_c):
    pred, target, w = _ref_case(seed=1)
    s = torch.tensor([1.0, 0.0, 2.0], dtype=torch.float64)
    tag = torch.tensor([0.5, 1.5, 2.5], dtype=torch.float64)
    c = torch.tensor([0.01, 0.1, 1.0], dtype=torch.float64) if per_sample_c else 0.3
    p = pred.clone().requires_grad_(True)
    (0.25 * X.loss(p, target, w, s, loss_type, c, tag)).backward()
    want = X.dpred(pred, target, w, s, loss_type, c, tag, grad_scale=0.25)
    assert torch.allclose(p.grad, want, rtol=1e-10, atol=1e-18)
    assert float(p.grad[1].abs().max()) == 0.0 and float(p.grad[0].abs().max()) > 0.0       # s_b = 0: no gradient for that sample
    # d l / d d on its own
    d = (pred - target).clone().requires_grad_(True)
    X.element_loss(d, loss_type, c).sum().backward()
    assert torch.allclose(d.grad, X.element_loss_grad(pred - target, loss_type, c), rtol=1e-10, atol=1e-18)


def test_reference_guard_and_target():
    pred, target, w = _ref_case(seed=2)
    big = X.loss(pred * 1e3, target, w)
    assert float(big) == 1000.0 and float(X.dpred(pred * 1e3, target, w).abs().max()) == 0.0
    bad = pred.clone()
    bad[1, 0, 0, 0] = float("inf")
    assert float(X.loss(bad, target, w)) == 1000.0
    per = X.per_sample_loss(bad, target, w)
    assert not torch.isfinite(per[1]) and torch.isfinite(per[0]) and torch.isfinite(per[2])
    from oracle import loss_ref as R
    lat, noise, _ = _ref_case(seed=3)
    lat, noise = lat.float(), noise.float()
    ts = torch.tensor([0, 500, 999])
    sig = R.karras_sigmas()[ts]
    tg, ww = X.target_and_weight("ddpm", lat, noise, sig)
    assert torch.equal(tg, R.get_velocity(lat, noise, sig)) and torch.equal(ww, torch.minimum(R.get_snr(sig), torch.tensor(5.0)))
    p = torch.randn(3, 4, 5, 7, generator=torch.Generator().manual_seed(4))
    assert float(X.loss(p, tg, ww)) == pytest.approx(float(R.ddpm_loss(p, lat, noise, ts)), rel=1e-6)
    tg, ww = X.target_and_weight("flow_matching", lat, noise, torch.tensor([0.1, 0.5, 0.9]))
    assert float(X.loss(p, tg, ww)) == pytest.approx(float(R.flow_matching_loss(p, noise, lat)), rel=1e-6)


# ---------------------------------------------------------------------------------------------- 4. evaluate()
@pytest.mark.parametrize("method,timesteps", [("ddpm", [0, 2]), ("flow_matching", [0.25, 0.5, 0.75])])
def test_evaluate_is_forward_only(method, timesteps):
    tr, net = _trainer(method, tag_weights_per_sample=True)
    CountingOpt.steps = 0
    tr.optimizer = CountingOpt()
    tr._micro, tr._zeroed = 2, True                                            # an accumulation cycle in progress
    batches = [_batch(3, tag=[1.0, 2.0, 3.0]), _batch(2)]
    per_t, mean = tr.evaluate(batches, timesteps, generator=torch.Generator().manual_seed(7))
    fwds = [c for c in net.calls if c[0] == "fwd"]
    assert len(fwds) == len(batches) * len(timesteps)
    assert {c[0] for c in net.calls} == {"fwd"}                                # never backward, never zero_grads
    assert CountingOpt.steps == 0 and (tr._micro, tr._zeroed) == (2, True)
    assert all(c[3]["per_sample_loss"] is True for c in fwds)
    # every batch at every timestep, the whole batch at that timestep
    seen = [(c[2][0].shape[0], [float(v) for v in c[2][3 if method == "ddpm" else 2]]) for c in fwds]
    assert seen == [(b["vae_latents"].shape[0], [float(t)] * b["vae_latents"].shape[0]) for b in batches for t in timesteps]
    if method == "ddpm":
        assert all(torch.equal(c[2][2], torch.tensor(SIGMAS)[[int(t)] * c[2][0].shape[0]]) for c, (_b, t) in
                   zip(fwds, [(b, t) for b in batches for t in timesteps]))
    # the stand-in's L_b = (b + 1) * (timestep value + 1): per-timestep mean over the 3 + 2 samples, and the overall mean
    assert set(per_t) == set(timesteps)
    for t in timesteps:
        assert per_t[t] == pytest.approx((1 + 2 + 3 + 1 + 2) / 5.0 * (t + 1.0), rel=1e-6)
    assert mean == pytest.approx(sum(per_t.values()) / len(per_t), rel=1e-6)
    # same generator seed -> the same noise, call by call; another seed -> another noise
    noise1 = [c[2][1].clone() for c in fwds]
    net.calls.clear()
    tr.evaluate(batches, timesteps, generator=torch.Generator().manual_seed(7))
    assert all(torch.equal(a, c[2][1]) for a, c in zip(noise1, net.calls))
    net.calls.clear()
    tr.evaluate(batches, timesteps, generator=torch.Generator().manual_seed(8))
    assert not any(torch.equal(a, c[2][1]) for a, c in zip(noise1, net.calls))
    assert len({float(n.sum()) for n in noise1}) == len(noise1)                # a fresh draw for every call
