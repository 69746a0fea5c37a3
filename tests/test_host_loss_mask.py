"""Masked loss, input perturbation, noise offset and conditioning dropout, host side (no GPU): the extended loss-config struct, the
CPU restatement of the two mask normalisations against autograd and against the unmasked formula, the trainer's recipes against a
hand replay of the same generator (with the RecNet stand-in of test_host_loss_ext.py, which records what `forward_loss` receives),
and the argument errors of the loaded library, which are reported before anything touches a device."""
import ctypes as C
import importlib
from pathlib import Path

import pytest
import torch

import sdxl_amd  # noqa: F401
from sdxl_amd import lib

import _loss_ext_ref as X
import _loss_mask_ref as MR
from test_host_loss_ext import RecNet, _batch, _trainer

NM = importlib.import_module("sdxl-training-improvements_amd.native_mi355x")
NU = importlib.import_module("sdxl-training-improvements_amd.unet")

TS = torch.tensor([0, 1, 2])


# ---------------------------------------------------------------------------------------------- 1. the structs
def test_the_extended_struct_appends_behind_the_short_one():
    assert [f[0] for f in lib.LossConfig._fields_] == ["method", "prediction_type", "use_min_snr", "min_snr_gamma", "use_ztsnr",
                                                       "loss_type", "huber_c"]
    assert C.sizeof(lib.LossConfig) == 28
    E = lib.LossConfigExt
    assert issubclass(E, lib.LossConfig) and [f[0] for f in E._fields_] == ["mask_norm", "loss_mask", "noise_in"]
    assert (E.mask_norm.offset, E.loss_mask.offset, E.noise_in.offset) == (28, 32, 40) and C.sizeof(E) == 48
    assert E.loss_type.offset == 20 and E.huber_c.offset == 24
    assert lib.LOSS_EXT == 0x100 and lib.MASK_NORMS == {"mean": 0, "masked_mean": 1}
    e = E(0, 1, 1, 5.0, 1, lib.LOSS_TYPES["huber"] | lib.LOSS_EXT, 0.25)
    assert (e.mask_norm, e.loss_mask, e.noise_in) == (0, None, None) and e.loss_type & 0xff == 1
    # the entry points keep taking POINTER(LossConfig): ctypes accepts byref of the subclass
    assert lib.SIGNATURES["sdxl_forward_loss"][1] is C.POINTER(lib.LossConfig)
    assert lib.SIGNATURES["sdxl_op_loss"][0] is C.POINTER(lib.LossConfig)


def test_header_declares_the_fields_and_no_new_symbol():
    hdr = (Path(__file__).resolve().parent.parent / "include" / "sdxlstep.h").read_text()
    for field in ("#define SDXL_LOSS_EXT 0x100", "int          mask_norm;", "const float* loss_mask;", "const float* noise_in;"):
        assert field in hdr, field
    body = hdr[hdr.index("int   loss_type;"):hdr.index("} sdxl_loss_config;")]
    assert body.index("huber_c;") < body.index("mask_norm;") < body.index("loss_mask;") < body.index("noise_in;")
    assert hdr.count("SDXL_API int ") + hdr.count("SDXL_API const char* ") <= 58


# ---------------------------------------------------------------------------------------------- 2. the restatement against itself
def _ref_case(B=4, H=5, W=7, seed=0):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    mask = torch.tensor([0.0, 0.25, 0.5, 1.0], dtype=torch.float64)[torch.randint(0, 4, (B, H, W), generator=g)]
    mask[1] = 0.0                                                             # M_b = 0
    mask[2] = 1.0
    return r(B, 4, H, W), r(B, 4, H, W), torch.rand(B, generator=g, dtype=torch.float64) + 0.5, mask


@pytest.mark.parametrize("loss_type", X.LOSS_TYPES)
@pytest.mark.parametrize("mask_norm", MR.MASK_NORMS)
def test_autograd_equals_the_closed_form(mask_norm, loss_type):
    pred, target, w, mask = _ref_case(seed=1)
    s = torch.tensor([1.0, 0.7, 2.0, 0.5], dtype=torch.float64)
    tag = torch.tensor([0.5, 1.5, 2.5, 1.0], dtype=torch.float64)
    p = pred.clone().requires_grad_(True)
    (0.25 * MR.loss(p, target, w, mask, mask_norm, s, loss_type, 0.3, tag)).backward()
    want = MR.dpred(pred, target, w, mask, mask_norm, s, loss_type, 0.3, tag, grad_scale=0.25)
    assert bool(torch.isfinite(p.grad).all()) and bool(torch.isfinite(want).all())
    assert torch.allclose(p.grad, want, rtol=1e-10, atol=1e-18)
    assert float(p.grad[1].abs().max()) == 0.0 and float(want[1].abs().max()) == 0.0          # the empty sample: zeros, no nan
    per = MR.per_sample_loss(pred, target, w, mask, mask_norm, s, loss_type, 0.3)
    assert float(per[1]) == 0.0 and bool(torch.isfinite(per).all())
    zero = (mask == 0).unsqueeze(1).expand_as(pred)
    assert float(want[zero].abs().max()) == 0.0 and float(want[~zero].abs().min()) > 0.0


def test_the_two_normalisations_differ_by_the_mask_fraction():
    pred, target, w, mask = _ref_case(seed=2)
    mean = MR.per_sample_loss(pred, target, w, mask, "mean")
    mm = MR.per_sample_loss(pred, target, w, mask, "masked_mean")
    frac = mask.sum(dim=(1, 2)) / (mask.shape[1] * mask.shape[2])
    assert torch.allclose(mean, mm * frac, rtol=1e-12, atol=0.0)
    assert torch.equal(mean[2], mm[2])                                        # an all-ones sample: M_b = HW


@pytest.mark.parametrize("loss_type", X.LOSS_TYPES)
def test_all_ones_mask_with_mean_is_the_unmasked_formula(loss_type):
    pred, target, w, _ = _ref_case(seed=3)
    ones = torch.ones(pred.shape[0], pred.shape[2], pred.shape[3], dtype=torch.float64)
    s = torch.tensor([1.0, 0.0, 2.0, 0.5], dtype=torch.float64)
    tag = torch.tensor([0.5, 1.5, 2.5, 1.0], dtype=torch.float64)
    for norm in MR.MASK_NORMS:                                                # M_b = HW: masked_mean agrees too
        assert torch.allclose(MR.per_sample_loss(pred, target, w, ones, norm, s, loss_type, 0.3),
                              X.per_sample_loss(pred, target, w, s, loss_type, 0.3), rtol=1e-13, atol=0.0)
        assert float(MR.loss(pred, target, w, ones, norm, s, loss_type, 0.3, tag)) == \
            pytest.approx(float(X.loss(pred, target, w, s, loss_type, 0.3, tag)), rel=1e-13)
        assert torch.allclose(MR.dpred(pred, target, w, ones, norm, s, loss_type, 0.3, tag, 0.5),
                              X.dpred(pred, target, w, s, loss_type, 0.3, tag, 0.5), rtol=1e-13, atol=0.0)


def test_prepare_restates_the_oracle_add_noise():
    from oracle import loss_ref as R
    g = torch.Generator().manual_seed(4)
    lat, noise, nin = (torch.randn(3, 4, 5, 7, generator=g) for _ in range(3))
    sig = R.karras_sigmas()[torch.tensor([0, 500, 999])]
    assert torch.equal(MR.prepare("ddpm", lat, noise, sig), R.add_noise(lat, noise, sig).clamp(-20000.0, 20000.0).to(torch.bfloat16))
    assert not torch.equal(MR.prepare("ddpm", lat, nin, sig), MR.prepare("ddpm", lat, noise, sig))
    t = torch.tensor([0.1, 0.5, 0.9])
    want = ((1.0 - t.view(-1, 1, 1, 1)) * nin + t.view(-1, 1, 1, 1) * lat).to(torch.bfloat16)
    assert torch.equal(MR.prepare("flow_matching", lat, nin, t), want)


# ---------------------------------------------------------------------------------------------- 3. the host recipes
NEW_KWARGS = {"loss_mask", "noise_in", "mask_norm"}


def _mask(B=3, H=8, W=8, seed=11):
    g = torch.Generator().manual_seed(seed)
    return torch.tensor([0.0, 0.25, 0.5, 1.0])[torch.randint(0, 4, (B, H, W), generator=g)]


def test_keys_off_no_new_kwargs_and_no_extra_draw():
    tr, net = _trainer("flow_matching")
    batch = _batch()
    batch["loss_mask"] = _mask()                                               # masked_loss is off: ignored
    g = torch.Generator().manual_seed(21)
    tr.compute_loss(batch, generator=g)
    _m, _method, a, k = net.fwd()
    assert not NEW_KWARGS & set(k)
    g2 = torch.Generator().manual_seed(21)                                     # today's two draws: the noise, then the timesteps
    noise = torch.randn(batch["vae_latents"].shape, generator=g2)
    t = torch.sigmoid(torch.randn(3, generator=g2))
    assert torch.equal(a[1], noise) and torch.equal(a[2], t)
    assert torch.equal(g.get_state(), g2.get_state())
    assert a[4] is batch["prompt_embeds"] and a[5] is batch["pooled_prompt_embeds"]
    tr, net = _trainer("ddpm")
    tr.compute_loss(batch, timesteps=TS)
    assert not NEW_KWARGS & set(net.fwd()[3])


@pytest.mark.parametrize("norm", ["mean", "masked_mean"])
def test_masked_loss_passes_the_batch_mask(norm):
    tr, net = _trainer(masked_loss=norm)
    batch = _batch()
    m = _mask()
    batch["loss_mask"] = m.unsqueeze(1)                                        # [B,1,H,W] is accepted, [B,H,W] goes on
    g = torch.Generator().manual_seed(22)
    tr.compute_loss(batch, timesteps=TS, generator=g)
    k = net.fwd()[3]
    assert torch.equal(k["loss_mask"], m) and k["loss_mask"].dtype == torch.float32 and k["loss_mask"].shape == (3, 8, 8)
    assert k.get("mask_norm", "mean") == norm and "noise_in" not in k
    g2 = torch.Generator().manual_seed(22)
    torch.randn(batch["vae_latents"].shape, generator=g2)
    assert torch.equal(g.get_state(), g2.get_state())                          # a mask draws nothing
    tr.compute_loss(_batch(), timesteps=TS)                                    # a batch without a mask is unmasked
    assert not NEW_KWARGS & set(net.fwd()[3])


def test_every_recipe_against_a_hand_replay_of_the_generator():
    # each key on its own, then all three: the draws come after the base noise (and the timesteps) in the order offset,
    # perturbation, dropout, and a key that is off draws nothing
    for keys in (dict(noise_offset=0.1), dict(input_perturbation=0.2), dict(cond_dropout_prob=0.5),
                 dict(noise_offset=0.05, input_perturbation=0.1, cond_dropout_prob=0.5, masked_loss="masked_mean")):
        for method in ("ddpm", "flow_matching"):
            tr, net = _trainer(method, **keys)
            B = 6
            batch = _batch(B)
            batch["loss_mask"] = _mask(B)
            before = {k: v.clone() for k, v in batch.items() if torch.is_tensor(v)}
            g, g2 = torch.Generator().manual_seed(32), torch.Generator().manual_seed(32)
            if method == "ddpm":
                ts = torch.tensor([0, 1, 2, 0, 1, 2])
                tr.compute_loss(batch, timesteps=ts, generator=g)
                noise = torch.randn(batch["vae_latents"].shape, generator=g2)
            else:
                tr.compute_loss(batch, generator=g)
                noise = torch.randn(batch["vae_latents"].shape, generator=g2)
                t = torch.sigmoid(torch.randn(B, generator=g2))
            _m, _method, a, k = net.fwd()
            if "noise_offset" in keys:
                noise = noise + keys["noise_offset"] * torch.randn(B, 4, 1, 1, generator=g2)
            assert torch.equal(a[1], noise), (keys, method)                    # the target's noise: after the offset
            if "input_perturbation" in keys:
                nin = noise + keys["input_perturbation"] * torch.randn(B, 4, 8, 8, generator=g2)
                assert torch.equal(k["noise_in"], nin) and k["noise_in"].dtype == torch.float32
            else:
                assert "noise_in" not in k
            if "cond_dropout_prob" in keys:
                drop = torch.rand(B, generator=g2) < keys["cond_dropout_prob"]
                assert bool(drop.any()) and not bool(drop.all())
                for i, key in ((4, "prompt_embeds"), (5, "pooled_prompt_embeds")):
                    assert float(a[i][drop].abs().max()) == 0.0                # exactly the drawn rows are zero ...
                    assert torch.equal(a[i][~drop], before[key][~drop])         # ... and the others are the caller's
                assert torch.equal(a[6], before["time_ids"])                   # time_ids are kept
            else:
                assert a[4] is batch["prompt_embeds"] and a[5] is batch["pooled_prompt_embeds"]
            if method == "flow_matching":
                assert torch.equal(a[2], t)
            assert torch.equal(g.get_state(), g2.get_state()), (keys, method)
            assert all(torch.equal(batch[key], v) for key, v in before.items())     # the caller's batch is untouched
            assert ("loss_mask" in k) == ("masked_loss" in keys)


def test_an_injected_noise_is_the_base_noise():
    tr, net = _trainer(noise_offset=0.1, input_perturbation=0.2)
    batch = _batch()
    base = torch.randn(3, 4, 8, 8, generator=torch.Generator().manual_seed(40))
    g, g2 = torch.Generator().manual_seed(41), torch.Generator().manual_seed(41)
    tr.compute_loss(batch, timesteps=TS, noise=base.clone(), generator=g)
    noise = base + 0.1 * torch.randn(3, 4, 1, 1, generator=g2)
    nin = noise + 0.2 * torch.randn(3, 4, 8, 8, generator=g2)
    assert torch.equal(net.fwd()[2][1], noise) and torch.equal(net.fwd()[3]["noise_in"], nin)


@pytest.mark.parametrize("method,timesteps", [("ddpm", [0, 2]), ("flow_matching", [0.25, 0.75])])
def test_evaluate_passes_the_mask_and_no_augmentation(method, timesteps):
    tr, net = _trainer(method, masked_loss="masked_mean", noise_offset=0.1, input_perturbation=0.2, cond_dropout_prob=1.0)
    batch = _batch()
    batch["loss_mask"] = _mask()
    g, g2 = torch.Generator().manual_seed(51), torch.Generator().manual_seed(51)
    tr.evaluate([batch], timesteps, generator=g)
    fwds = [c for c in net.calls if c[0] == "fwd"]
    assert len(fwds) == len(timesteps)
    for c in fwds:
        a, k = c[2], c[3]
        assert torch.equal(a[1], torch.randn(batch["vae_latents"].shape, generator=g2))     # the base noise, no offset
        assert torch.equal(k["loss_mask"], batch["loss_mask"]) and k["mask_norm"] == "masked_mean" and "noise_in" not in k
        assert a[4] is batch["prompt_embeds"] and a[5] is batch["pooled_prompt_embeds"]     # no dropout (p = 1 would zero all)
    assert torch.equal(g.get_state(), g2.get_state())


@pytest.mark.parametrize("keys,match", [
    (dict(masked_loss="sum"), "masked_loss"),
    (dict(masked_loss=True), "masked_loss"),
    (dict(noise_offset=-0.1), "noise_offset"),
    (dict(noise_offset="0.1"), "noise_offset"),
    (dict(input_perturbation=-1.0), "input_perturbation"),
    (dict(input_perturbation=float("nan")), "input_perturbation"),
    (dict(cond_dropout_prob=1.5), "cond_dropout_prob"),
    (dict(cond_dropout_prob=-0.1), "cond_dropout_prob"),
])
def test_bad_key_values_raise_when_the_trainer_is_built(keys, match):
    with pytest.raises(ValueError, match=match):
        _trainer("ddpm", **keys)


@pytest.mark.parametrize("bad", [torch.ones(3, 4, 8, 8), torch.ones(3, 64, 64), torch.ones(2, 8, 8), torch.ones(3, 8),
                                 -torch.ones(3, 8, 8), torch.full((3, 8, 8), float("nan")), torch.full((3, 1, 8, 8), float("inf"))])
def test_a_bad_mask_raises(bad):
    tr, net = _trainer(masked_loss="mean")
    batch = _batch()
    batch["loss_mask"] = bad
    with pytest.raises(ValueError, match="loss_mask"):
        tr.compute_loss(batch, timesteps=TS)
    assert not [c for c in net.calls if c[0] == "fwd"]
    with pytest.raises(ValueError, match="loss_mask"):                         # the native UNet's own check is the same function
        NU.loss_mask_bhw(bad, (3, 4, 8, 8))


def test_dropin_copies_the_keys():
    ref_cfg = {"training": {"method": "native_mi355x", "native_objective": "ddpm", "masked_loss": "masked_mean", "noise_offset": 0.05,
                            "input_perturbation": 0.1, "cond_dropout_prob": 0.1}}
    net = RecNet()

    class M:
        unet = net
    tr = NM.NativeMI355XTrainer(model=M(), optimizer=None, train_dataloader=None, device="cpu", config=ref_cfg)
    tc = tr.config.training
    assert (tc.masked_loss, tc.noise_offset, tc.input_perturbation, tc.cond_dropout_prob) == ("masked_mean", 0.05, 0.1, 0.1)
    assert (tr.masked_loss, tr.noise_offset, tr.input_perturbation, tr.cond_dropout_prob) == ("masked_mean", 0.05, 0.1, 0.1)
    with pytest.raises(ValueError, match="cond_dropout_prob"):
        NM.NativeMI355XTrainer(model=M(), device="cpu", config={"training": {"method": "native_mi355x", "cond_dropout_prob": 2}})


# ---------------------------------------------------------------------------------------------- 4. argument errors of the library
@pytest.mark.parametrize("loss_type,mask_norm,with_mask,match", [
    (-1, 0, False, "loss_type"),
    (lib.LOSS_EXT | 7, 0, False, "loss_type"),
    (0x200, 0, False, "loss_type"),
    (lib.LOSS_EXT | 0x200, 0, False, "loss_type"),
    (lib.LOSS_EXT, 2, True, "mask_norm"),
    (lib.LOSS_EXT | 1, -1, True, "mask_norm"),
])
def test_bad_arguments_return_1_before_any_device_work(loss_type, mask_norm, with_mask, match):
    L = lib.load()
    lc = lib.LossConfigExt(0, 1, 1, 5.0, 1, loss_type, 0.1)
    lc.mask_norm = mask_norm
    keep = (C.c_float * 64)()                  # stands where a device pointer would: an argument error comes before it is read
    lc.loss_mask = C.addressof(keep) if with_mask else None
    b = lib.Batch(1, 4, 4, 77, C.addressof(keep), C.addressof(keep), C.addressof(keep), None, None, None, None, None)
    for phase in (0, 1, 2):
        assert L.sdxl_op_loss(C.byref(lc), C.byref(b), None, None, None, 1.0, None, phase, None) == 1
        assert match in L.sdxl_last_error().decode()
    with pytest.raises(lib.SdxlError, match=match):
        lib.check(L.sdxl_op_loss(C.byref(lc), C.byref(b), None, None, None, 1.0, None, 1, None))
