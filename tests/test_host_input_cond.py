"""Extra UNet input channels (in_channels 5 .. 16), host side (no GPU): the flag and the struct of the header against lib.py, what
sdxl_create and sdxl_op_loss refuse before any device call, widen_conv_in, config_from_unet on a 9-channel state dict, the trainer's
keys and draw order on the RecNet stand-in of test_host_loss_ext.py (with the defaults it sees today's calls exactly), what the sampler
hands the net, and what the LoRA rules decide for conv_in at 8 and at 9 channels."""
import ctypes as C
import importlib
import re
from pathlib import Path
from types import SimpleNamespace

import pytest
import torch

import sdxl_amd  # noqa: F401
from sdxl_amd import lib

from test_host_loss_ext import RecNet, _batch, _trainer

NU = importlib.import_module("sdxl-training-improvements_amd.unet")
LO = importlib.import_module("sdxl-training-improvements_amd.lora")
T = importlib.import_module("sdxl-training-improvements_amd.trainer")
CFG = importlib.import_module("sdxl-training-improvements_amd.config")
S = importlib.import_module("sdxl-training-improvements_amd.sampler")

TS = torch.tensor([0, 1, 2])
HDR = (Path(__file__).resolve().parent.parent / "include" / "sdxlstep.h").read_text()


# ---------------------------------------------------------------------------------------------- 1. the header against lib.py
def test_flag_and_struct_match_the_header():
    m = re.search(r"#define SDXL_BATCH_COND (0x[0-9a-fA-F]+)", HDR)
    assert m and int(m.group(1), 16) == lib.BATCH_COND == 0x20000
    assert lib.BATCH_COND & lib.BATCH_EXT == 0 and lib.BATCH_COND & 0xFFFF == 0
    body = HDR[HDR.index("typedef struct {\n  sdxl_batch_ext base;"):HDR.index("} sdxl_batch_cond;")]
    decl = [ln.split("/*")[0].strip().rstrip(";") for ln in body.splitlines()[1:] if ln.strip() and not ln.strip().startswith("/*")]
    assert decl == ["sdxl_batch_ext base", "const float* input_cond", "int cond_channels"]
    B = lib.InputCondBatch
    assert issubclass(B, lib.CondGradBatch) and [f[0] for f in B._fields_] == ["input_cond", "cond_channels"]
    assert B.input_cond.offset == C.sizeof(lib.CondGradBatch) and B.cond_channels.offset == B.input_cond.offset + 8
    assert C.sizeof(B) == C.sizeof(lib.CondGradBatch) + 16
    b = B(2, 8, 8, 77 | lib.BATCH_COND)
    assert (b.input_cond, b.cond_channels, b.d_prompt_embeds, b.d_pooled) == (None, 0, None, None)
    # no new entry point carries it
    assert HDR.count("SDXL_API int ") + HDR.count("SDXL_API const char* ") <= 58
    assert len(set(re.findall(r"\b(sdxl_[a-z0-9_]+)\s*\(", HDR))) <= 58


# ---------------------------------------------------------------------------------------------- 2. the library, before any device call
@pytest.mark.parametrize("cin", [3, 17, 0, -1])
def test_create_refuses_in_channels_outside_4_to_16(cin):
    L = lib.load()
    h = C.c_void_p()
    cfg = NU.make_config(in_channels=cin)
    assert L.sdxl_create(C.byref(cfg), 0, C.byref(h)) == 1 and not h.value
    assert "in_channels" in L.sdxl_last_error().decode()


def test_create_refuses_out_channels_other_than_4():
    L = lib.load()
    h = C.c_void_p()
    cfg = NU.make_config(in_channels=9, out_channels=9)
    assert L.sdxl_create(C.byref(cfg), 0, C.byref(h)) == 1 and "out_channels" in L.sdxl_last_error().decode()


@pytest.mark.parametrize("cin", [9, 8, 16, 5])
def test_create_accepts_extra_input_channels(cin):
    """the configuration check passes: the call gets as far as the device (a HIP error on a machine without one, a handle with one)"""
    L = lib.load()
    h = C.c_void_p()
    cfg = NU.make_config(in_channels=cin)
    rc = L.sdxl_create(C.byref(cfg), 0, C.byref(h))
    if torch.cuda.is_available():
        assert rc == 0 and h.value
        L.sdxl_destroy(h)
    else:
        assert rc == 2, (rc, L.sdxl_last_error().decode())
        assert "in_channels" not in L.sdxl_last_error().decode()


@pytest.mark.parametrize("B,H,W", [(2, 16, 16), (1, 104, 152), (1, 128, 128), (4, 128, 128), (1, 80, 192)])
def test_conv_in_16_wide_takes_the_route_of_the_8_wide(B, H, W):
    """gemm_route (csrc/gemm.hip) on conv_in's forward and weight gradient: Cin = 16 is sent where Cin = 8 is -- the general gather of the
    128-row kernel forward, and the same weight-gradient kernel"""
    M = B * H * W
    routes = []
    for cin in (8, 16):
        fwd = lib.gemm_route(form=0, taps=9, M=M, N=320, K=cin, Hm=H, Wm=W, Hs=H, Ws=W)
        wg = lib.gemm_route(form=2, taps=9, M=320, N=cin, K=M, Hm=H, Wm=W, Hs=H, Ws=W, bias_grad=1)
        assert fwd["kernel"] == "128-row" and fwd["fast"] is False
        routes.append((fwd, wg))
    assert routes[0] == routes[1]


def _op_loss(cond_ptr, channels, phase, flag=True):
    L = lib.load()
    keep = (C.c_float * 64)()                  # stands where a device pointer would: an argument error comes before it is read
    a = C.addressof(keep)
    b = lib.InputCondBatch(1, 4, 4, 77 | (lib.BATCH_COND if flag else 0), a, a, a, None, None, None, None, None)
    b.input_cond, b.cond_channels = cond_ptr, channels
    lc = lib.LossConfig(0, 1, 1, 5.0, 1)
    rc = L.sdxl_op_loss(C.byref(lc), C.byref(b), None, None, None, 1.0, None, phase, None)
    return rc, L.sdxl_last_error().decode(), a


def test_op_loss_refuses_missing_and_unexpected_input_cond():
    rc, msg, a = _op_loss(None, 5, 0)                       # in_channels > 4 and no input_cond
    assert rc == 1 and "input_cond" in msg
    rc, msg, _ = _op_loss(a, 0, 0)                          # in_channels == 4 with a non-NULL input_cond
    assert rc == 1 and "input_cond" in msg
    for n in (13, -1):                                      # more than 16 input channels
        rc, msg, _ = _op_loss(a, n, 0)
        assert rc == 1 and "input_cond" in msg
    with pytest.raises(lib.SdxlError, match="input_cond"):
        lib.check(_op_loss(None, 12, 0)[0])


# ---------------------------------------------------------------------------------------------- 3. widen_conv_in, config_from_unet
def _state_dict(cin=4):
    g = torch.Generator().manual_seed(cin)
    return {"conv_in.weight": torch.randn(32, cin, 3, 3, generator=g).to(torch.bfloat16), "conv_in.bias": torch.randn(32, generator=g),
            "down_blocks.1.resnets.0.conv1.weight": torch.randn(64, 32, 3, 3, generator=g),
            "down_blocks.1.attentions.0.transformer_blocks.0.norm1.weight": torch.ones(64),
            "down_blocks.1.attentions.0.transformer_blocks.0.attn2.to_k.weight": torch.randn(64, 48, generator=g),
            "add_embedding.linear_1.weight": torch.randn(128, 24 + 6 * 16, generator=g)}


@pytest.mark.parametrize("cin", [9, 8, 4, 16])
def test_widen_conv_in(cin):
    sd = _state_dict()
    before = {k: v.clone() for k, v in sd.items()}
    out = NU.widen_conv_in(sd, cin)
    w = out["conv_in.weight"]
    assert tuple(w.shape) == (32, cin, 3, 3) and w.dtype == sd["conv_in.weight"].dtype
    assert torch.equal(w[:, :4].contiguous().view(torch.int16), sd["conv_in.weight"].view(torch.int16))      # the original slice, bit for bit
    assert int((w[:, 4:].contiguous().view(torch.int16) != 0).sum()) == 0                                     # the rest: all-zero bits
    assert set(out) == set(sd) and all(out[k] is sd[k] for k in sd if k != "conv_in.weight")
    assert out is not sd and all(torch.equal(sd[k], before[k]) for k in sd)                                   # a copy: the caller's is untouched
    assert out["conv_in.weight"] is not sd["conv_in.weight"]


@pytest.mark.parametrize("cin", [3, 17])
def test_widen_conv_in_refuses(cin):
    with pytest.raises(ValueError, match="in_channels"):
        NU.widen_conv_in(_state_dict(), cin)


def test_config_from_unet_reads_in_channels():
    sd = _state_dict(9)
    unet = SimpleNamespace(state_dict=lambda: sd)
    assert NU.config_from_unet(unet).in_channels == 9                                  # no .config: conv_in.weight.shape[1]
    assert NU.config_from_unet(SimpleNamespace(state_dict=lambda: _state_dict(4))).in_channels == 4
    cfg = dict(in_channels=8, block_out_channels=(32, 64), transformer_layers_per_block=(0, 1), cross_attention_dim=48,
               addition_time_embed_dim=16, projection_class_embeddings_input_dim=120, attention_head_dim=64)
    assert NU.config_from_unet(SimpleNamespace(config=cfg, state_dict=lambda: sd)).in_channels == 8      # .config wins
    assert NU.config_from_unet(SimpleNamespace(config=SimpleNamespace(**cfg), state_dict=lambda: sd)).in_channels == 8
    assert NU.make_config(in_channels=9).in_channels == 9 and NU.make_config().in_channels == 4
    assert [NU.input_cs(c) for c in (4, 5, 8, 9, 16)] == [8, 8, 8, 16, 16]


# ---------------------------------------------------------------------------------------------- 4. the trainer keys
def _cond_trainer(cin, method="ddpm", **keys):
    cfg = CFG.Config()
    cfg.training.method = method
    for k, v in keys.items():
        setattr(cfg.training, k, v)
    net = RecNet()
    net.cfg = NU.make_config(in_channels=cin)

    class M:
        unet = net
    tr = T.NativeSDXLTrainer(M(), optimizer=None, train_dataloader=None, device="cpu", config=cfg)
    if method == "ddpm":
        tr.noise_scheduler.sigmas = torch.tensor([0.5, 1.0, 2.0])
    return tr, net


def _inpaint_batch(B=3, seed=3):
    g = torch.Generator().manual_seed(seed)
    b = _batch(B)
    b["inpaint_mask"] = (torch.rand(B, 1, 8, 8, generator=g) < 0.5).float()
    b["masked_latents"] = torch.randn(B, 4, 8, 8, generator=g)
    return b


def test_defaults_are_todays_calls():
    cfg = CFG.Config()
    assert (cfg.training.input_conditioning, cfg.training.input_cond_dropout_prob) == ("none", 0.0)
    for method in ("ddpm", "flow_matching"):
        tr, net = _trainer(method)                                                    # (the stand-in has no cfg: in_channels 4)
        batch = _inpaint_batch()                                                      # keys the default ignores
        g, g2 = torch.Generator().manual_seed(21), torch.Generator().manual_seed(21)
        tr.compute_loss(batch, generator=g, timesteps=TS if method == "ddpm" else None)
        _m, _method, a, k = net.fwd()
        assert "input_cond" not in k and len(a) == 8
        noise = torch.randn(batch["vae_latents"].shape, generator=g2)                 # today's draws and nothing behind them
        if method == "flow_matching":
            assert torch.equal(a[2], torch.sigmoid(torch.randn(3, generator=g2)))
        assert torch.equal(a[1], noise) and torch.equal(g.get_state(), g2.get_state())
        tr.evaluate([batch], [1] if method == "ddpm" else [0.5])
        assert "input_cond" not in net.fwd()[3]


@pytest.mark.parametrize("mask_shape", [(3, 1, 8, 8), (3, 8, 8)])
def test_inpaint_builds_mask_then_masked_latents(mask_shape):
    tr, net = _cond_trainer(9, input_conditioning="inpaint")
    batch = _inpaint_batch()
    batch["inpaint_mask"] = batch["inpaint_mask"].reshape(mask_shape)
    before = {k: v.clone() for k, v in batch.items() if torch.is_tensor(v)}
    g, g2 = torch.Generator().manual_seed(5), torch.Generator().manual_seed(5)
    tr.compute_loss(batch, timesteps=TS, generator=g)
    ic = net.fwd()[3]["input_cond"]
    assert ic.dtype == torch.float32 and tuple(ic.shape) == (3, 5, 8, 8)
    assert torch.equal(ic[:, :1], before["inpaint_mask"].reshape(3, 1, 8, 8)) and torch.equal(ic[:, 1:], before["masked_latents"])      # diffusers' order
    torch.randn(batch["vae_latents"].shape, generator=g2)
    assert torch.equal(g.get_state(), g2.get_state())                                 # conditioning draws nothing
    assert all(torch.equal(batch[k], v) for k, v in before.items())


def test_concat_passes_cond_latents():
    tr, net = _cond_trainer(8, "flow_matching", input_conditioning="concat")
    batch = _batch()
    batch["cond_latents"] = torch.randn(3, 4, 8, 8)
    tr.compute_loss(batch)
    ic = net.fwd()[3]["input_cond"]
    assert torch.equal(ic, batch["cond_latents"]) and ic is not batch["cond_latents"]


def test_dropout_draws_last_and_zeroes_a_copy():
    keys = dict(noise_offset=0.05, input_perturbation=0.1, cond_dropout_prob=0.5, input_conditioning="inpaint", input_cond_dropout_prob=0.5)
    for method in ("ddpm", "flow_matching"):
        tr, net = _cond_trainer(9, method, **keys)
        B = 6
        batch = _inpaint_batch(B)
        before = {k: v.clone() for k, v in batch.items() if torch.is_tensor(v)}
        g, g2 = torch.Generator().manual_seed(32), torch.Generator().manual_seed(32)
        tr.compute_loss(batch, generator=g, timesteps=torch.tensor([0, 1, 2, 0, 1, 2]) if method == "ddpm" else None)
        torch.randn(batch["vae_latents"].shape, generator=g2)                         # every existing draw, in its order ...
        if method == "flow_matching":
            torch.randn(B, generator=g2)
        torch.randn(B, 4, 1, 1, generator=g2)
        torch.randn(B, 4, 8, 8, generator=g2)
        torch.rand(B, generator=g2)
        drop = torch.rand(B, generator=g2) < 0.5                                     # ... then this one
        assert bool(drop.any()) and not bool(drop.all())
        assert torch.equal(g.get_state(), g2.get_state()), method
        ic = net.fwd()[3]["input_cond"]
        full = torch.cat([before["inpaint_mask"], before["masked_latents"]], dim=1)
        assert float(ic[drop].abs().max()) == 0.0 and torch.equal(ic[~drop], full[~drop])
        assert all(torch.equal(batch[k], v) for k, v in before.items())                # zeroed on a copy
    # the key alone: no other draw moves
    tr, net = _cond_trainer(9, input_conditioning="inpaint", input_cond_dropout_prob=1.0)
    batch = _inpaint_batch()
    g, g2 = torch.Generator().manual_seed(33), torch.Generator().manual_seed(33)
    tr.compute_loss(batch, timesteps=TS, generator=g)
    torch.randn(batch["vae_latents"].shape, generator=g2)
    torch.rand(3, generator=g2)
    assert torch.equal(g.get_state(), g2.get_state())
    assert float(net.fwd()[3]["input_cond"].abs().max()) == 0.0


def test_evaluate_passes_input_cond_without_dropout():
    tr, net = _cond_trainer(9, input_conditioning="inpaint", input_cond_dropout_prob=1.0)
    batch = _inpaint_batch()
    g, g2 = torch.Generator().manual_seed(51), torch.Generator().manual_seed(51)
    tr.evaluate([batch], [0, 2], generator=g)
    fwds = [c for c in net.calls if c[0] == "fwd"]
    assert len(fwds) == 2
    for c in fwds:
        torch.randn(batch["vae_latents"].shape, generator=g2)
        assert torch.equal(c[3]["input_cond"], torch.cat([batch["inpaint_mask"], batch["masked_latents"]], dim=1))
    assert torch.equal(g.get_state(), g2.get_state())


@pytest.mark.parametrize("cin,keys,match", [
    (4, dict(input_conditioning="mask"), "input_conditioning"),
    (4, dict(input_conditioning=True), "input_conditioning"),
    (9, dict(), "input_conditioning"),                                               # "none" requires in_channels == 4
    (8, dict(input_conditioning="inpaint"), "input_conditioning"),                   # "inpaint" requires 9
    (4, dict(input_conditioning="inpaint"), "input_conditioning"),
    (4, dict(input_conditioning="concat"), "input_conditioning"),
    (9, dict(input_conditioning="inpaint", input_cond_dropout_prob=1.5), "input_cond_dropout_prob"),
    (9, dict(input_conditioning="inpaint", input_cond_dropout_prob=-0.1), "input_cond_dropout_prob"),
    (9, dict(input_conditioning="inpaint", input_cond_dropout_prob="0.1"), "input_cond_dropout_prob"),
    (9, dict(input_conditioning="inpaint", input_cond_dropout_prob=True), "input_cond_dropout_prob"),
    (4, dict(input_cond_dropout_prob=0.5), "input_cond_dropout_prob"),
])
def test_bad_key_values_raise_when_the_trainer_is_built(cin, keys, match):
    with pytest.raises(ValueError, match=match):
        _cond_trainer(cin, **keys)


@pytest.mark.parametrize("mode,cin,drop_key,bad", [
    ("inpaint", 9, "inpaint_mask", None), ("inpaint", 9, "masked_latents", None), ("concat", 8, "cond_latents", None),
    ("inpaint", 9, "inpaint_mask", torch.ones(3, 2, 8, 8)), ("inpaint", 9, "inpaint_mask", torch.ones(3, 64, 64)),
    ("inpaint", 9, "masked_latents", torch.ones(3, 5, 8, 8)), ("concat", 8, "cond_latents", torch.ones(3, 5, 8, 8)),
    ("concat", 8, "cond_latents", torch.ones(2, 4, 8, 8)),
])
def test_a_missing_key_or_a_wrong_shape_names_it(mode, cin, drop_key, bad):
    tr, net = _cond_trainer(cin, input_conditioning=mode)
    batch = _inpaint_batch()
    batch["cond_latents"] = torch.randn(3, 4, 8, 8)
    if bad is None:
        del batch[drop_key]
    else:
        batch[drop_key] = bad
    with pytest.raises(ValueError, match=drop_key):
        tr.compute_loss(batch, timesteps=TS)
    assert not [c for c in net.calls if c[0] == "fwd"]


def test_dropin_copies_the_keys_and_takes_in_channels_from_the_model():
    NM = importlib.import_module("sdxl-training-improvements_amd.native_mi355x")
    net = RecNet()
    net.cfg = NU.make_config(in_channels=9)

    class M:
        unet = net
    tr = NM.NativeMI355XTrainer(model=M(), optimizer=None, train_dataloader=None, device="cpu",
                                config={"training": {"method": "native_mi355x", "native_objective": "ddpm", "input_conditioning": "inpaint",
                                                     "input_cond_dropout_prob": 0.1}})
    assert (tr.input_conditioning, tr.input_cond_dropout_prob, tr.in_channels) == ("inpaint", 0.1, 9)
    with pytest.raises(ValueError, match="input_conditioning"):                       # widening is the caller's job, before constructing
        NM.NativeMI355XTrainer(model=M(), device="cpu", config={"training": {"method": "native_mi355x"}})


# ---------------------------------------------------------------------------------------------- 5. the sampler
class RecSampleNet:
    device = torch.device("cpu")

    def __init__(self):
        self.calls = []

    def sample_init(self, *a, **k):
        self.calls.append(("init", a, k))

    def sample_step(self, *a, **k):
        self.calls.append(("step", a, k))


def test_sampler_passes_input_cond_only_when_given():
    net = RecSampleNet()
    sm = S.NativeSampler(net, "ddpm", "v_prediction", True, "trained")
    B, H, W = 2, 8, 8
    pe, po, ti = torch.randn(B, 77, 16), torch.randn(B, 8), torch.zeros(B, 6)
    noise = torch.randn(B, 4, H, W)
    sm.sample(pe, po, ti, height=H, width=W, num_steps=3, guidance_scale=2.0, noise=noise)
    assert len(net.calls) == 4 and all("input_cond" not in k for _n, _a, k in net.calls)      # today's calls
    ic, nic = torch.randn(B, 5, H, W), torch.randn(B, 5, H, W)
    for solver in ("euler", "dpmpp_2m"):
        for neg, second in ((None, ic), (nic, nic)):
            net.calls.clear()
            sm.sample(pe, po, ti, height=H, width=W, num_steps=3, guidance_scale=2.0, noise=noise, solver=solver, input_cond=ic, neg_input_cond=neg)
            assert len(net.calls) == 4
            for _n, _a, k in net.calls:
                c = k["input_cond"]
                assert c.dtype == torch.float32 and c.is_contiguous() and tuple(c.shape) == (2 * B, 5, H, W)
                assert torch.equal(c[:B], ic) and torch.equal(c[B:], second)           # the uncond half reuses input_cond unless neg is given
    net.calls.clear()
    sm.sample(pe, po, ti, height=H, width=W, num_steps=3, guidance_scale=1.0, noise=noise, input_cond=ic)
    assert all(tuple(k["input_cond"].shape) == (B, 5, H, W) for _n, _a, k in net.calls)
    with pytest.raises(ValueError, match="neg_input_cond"):
        sm.sample(pe, po, ti, height=H, width=W, num_steps=3, guidance_scale=2.0, noise=noise, neg_input_cond=nic)
    with pytest.raises(ValueError, match="input_cond"):
        sm.sample(pe, po, ti, height=H, width=W, num_steps=3, guidance_scale=2.0, noise=noise, input_cond=ic[:1])
    with pytest.raises(ValueError, match="neg_input_cond"):
        sm.sample(pe, po, ti, height=H, width=W, num_steps=3, guidance_scale=2.0, noise=noise, input_cond=ic, neg_input_cond=nic[:, :4])


# ---------------------------------------------------------------------------------------------- 6. LoRA on conv_in
def test_lora_rules_for_conv_in():
    """the rules as written: a convolution is never a "plain" target; with kinds "all" `in` = cin * 9 must be a multiple of 8, so the
    8-channel conv_in (72, stored unpadded) can carry an adapter and the 9-channel one (81, stored 16 wide) cannot, like the 4-channel one"""
    shapes = lambda cin: {"conv_in.weight": (320, cin, 3, 3), "conv_in.bias": (320,), "mid.to_q.weight": (320, 320)}
    for cin in (4, 8, 9):
        with pytest.raises(ValueError, match="conv_in"):
            LO.resolve_targets(shapes(cin), ["conv_in"], "plain")
    assert LO.resolve_targets(shapes(8), ["conv_in", "to_q"], "all") == ["conv_in.weight", "mid.to_q.weight"]
    for cin in (4, 9):
        with pytest.raises(ValueError, match=r"conv_in.*multiple of 8"):
            LO.resolve_targets(shapes(cin), ["conv_in"], "all")
    # the library's own rule (SDXL_DTYPE_LORA_LAYOUTS) is the same pair: in % 8, and input channels stored unpadded
    assert [(cin * 9) % 8 == 0 and NU.input_cs(cin) == cin for cin in (4, 8, 9)] == [False, True, False]
