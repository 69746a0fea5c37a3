"""Full-size SDXL-base UNet (2 567 463 684 parameters) on the GPU.

cfg 1 of BASELINE.json (method=ddpm, batch 1, 512^2 -> latent 64x64) and one sample of configs[1] / configs[2] (latent
128x128 = 1024^2, both methods): HIP loss AND probe gradients vs the fp32 CPU oracle (autograd through oracle/unet_ref.py) on
identical synthetic weights / latents / embeddings / timesteps -- loss tolerance 1e-3 relative (north_star), gradient probes spread
over the network (11 at cfg 1, 14 at 1024^2, incl. the 1280-channel self-attention projections whose Delta comes from the
out-projection dgrad's epilogue) at rel-L2 <= 6e-2 / cos >= 0.998, and every one of the 1 680 gradient tensors (tests/_gradparity.py;
bars at FULL_GRAD_BAR below).  The B = 4 decompositions are also checked for every tensor of the arena.  B = 4 (configs[1], [2], the 1344x768 bucket of configs[4]) is tied
to those B = 1 comparisons through size-independent properties: batch loss = mean of per-sample losses, batch gradient = 1/B-weighted
sum of per-sample gradients, reproducibility, accumulation linearity across plans, independence from the previous step.
"""
import math
import os

import pytest
import torch

import sdxl_amd  # noqa: F401
from oracle import loss_ref as R
from oracle import unet_ref as U
from sdxl_amd import synth
from sdxl_amd import unet as NU

from _gradparity import GradParity, compare_autograd, group

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def full():
    net = NU.NativeUNet(NU.make_config())
    synth.load_synthetic(net, seed=0)
    yield net
    net.close()


@pytest.fixture(scope="module")
def oracle_w():
    """fp32 CPU copy of the same synthetic weights for the oracle (10.3 GB, ~1.5 min of host hashing): built once."""
    n = len(os.sched_getaffinity(0))                               # the CPUs this process may run on, not the machine's count
    if os.environ.get("OMP_NUM_THREADS", "").isdigit():
        n = min(n, max(1, int(os.environ["OMP_NUM_THREADS"])))
    torch.set_num_threads(n)
    return U.synth_weights(U.SDXL_BASE, seed=0)                    # same bytes as synth.load_synthetic (tested on CPU)


def _probe(w, keys):
    for t in w.values():
        t.requires_grad_(False)
    for k in keys:
        w[k].requires_grad_(True)


def _inputs(B, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)
    bfr = lambda t: t.to(torch.bfloat16).float()
    return dict(lat=r(B, 4, H, W), noise=r(B, 4, H, W), ehs=bfr(r(B, 77, 2048)), pooled=bfr(r(B, 1280)),
                tid=torch.tensor([[8.0 * W, 8.0 * H, 0, 0, 8.0 * W, 8.0 * H]] * B))


def test_full_state_dict_round_trip_bit_exact(full):
    """Row f4 at SDXL-base size: all 1 680 diffusers keys exported from the packed arena equal what was imported, bit for
    bit -- the 3x3 conv repack, the fused attn*.to_{q,k,v} rows and the group-interleaved ff.net.0.proj included."""
    net = full
    shapes = net.param_shapes()
    assert len(shapes) == 1680
    order = synth.diffusers_key_order(shapes)
    n_checked = 0
    for name, want in synth.iter_synth(shapes, order, 0, device=net.device):
        got = net.export(name, grad=False, dtype=torch.bfloat16)
        assert got.shape == want.shape and torch.equal(got.view(torch.int16), want.view(torch.int16)), name
        n_checked += 1
    assert n_checked == 1680
    # import of a distinct pattern into the permuted tensors lands where export reads it (not merely self-consistent zeros)
    for name in ("mid_block.attentions.0.transformer_blocks.3.ff.net.0.proj.weight", "mid_block.attentions.0.transformer_blocks.3.ff.net.0.proj.bias",
                 "down_blocks.1.attentions.0.transformer_blocks.0.attn1.to_k.weight", "up_blocks.0.resnets.1.conv1.weight"):
        t = torch.arange(math.prod(shapes[name]), dtype=torch.float32, device=net.device).reshape(shapes[name]).remainder(251.0).to(torch.bfloat16)
        old = net.export(name, dtype=torch.bfloat16)
        net.load_weight(name, t)
        assert torch.equal(net.export(name, dtype=torch.bfloat16), t), name
        net.load_weight(name, old)


def test_segment_fixture_is_the_live_segment_list(full):
    """tests/golden/sdxl_segments.json (the world-8 slicing test on CPU runs over it) == what the engine reports"""
    import json
    from pathlib import Path
    d = json.loads((Path(__file__).parent / "golden" / "sdxl_segments.json").read_text())
    assert int(d["param_elems"]) == int(full.param_elems)
    assert [(int(o), int(n)) for o, n in d["segments"]] == [(int(o), int(n)) for o, n in full.segment_ranges()]


def test_cfg1_loss_matches_cpu_oracle(full, oracle_w):
    net = full
    x = _inputs(1, 64, 64, seed=101)
    ts = torch.tensor([820])
    sig = R.karras_sigmas()[ts]
    net.forward_loss("ddpm", x["lat"], x["noise"], sig, ts.float(), x["ehs"], x["pooled"], x["tid"])
    got = net.read_loss()
    w = oracle_w
    with torch.no_grad():
        ref = R.compute_loss_ddpm(lambda s, t, e, p, ti: U.unet_forward(w, s, t, e, p, ti, U.SDXL_BASE),
                                  {"vae_latents": x["lat"], "prompt_embeds": x["ehs"], "pooled_prompt_embeds": x["pooled"],
                                   "time_ids": x["tid"]}, x["noise"], ts)
    rel = abs(got[0] - float(ref["loss"])) / abs(float(ref["loss"]))
    pred_scale = got[2] / x["lat"].numel()
    print(f"[parity] FULL SDXL cfg1 ddpm loss: hip {got[0]:.6e} oracle {float(ref['loss']):.6e} rel {rel:.3e}; "
          f"pred_scale hip {pred_scale:.5f} oracle {ref['metrics']['pred_scale']:.5f}")
    assert rel <= 1e-3
    assert abs(pred_scale - ref["metrics"]["pred_scale"]) <= 2e-2 * ref["metrics"]["pred_scale"]


PROBES = ["conv_in.weight", "down_blocks.1.attentions.0.transformer_blocks.1.attn1.to_k.weight",
          "down_blocks.2.attentions.1.transformer_blocks.9.ff.net.0.proj.weight", "mid_block.resnets.0.conv2.weight",
          "mid_block.attentions.0.transformer_blocks.5.attn2.to_v.weight", "up_blocks.0.attentions.2.transformer_blocks.0.norm2.weight",
          "up_blocks.1.resnets.1.conv_shortcut.weight", "up_blocks.2.resnets.2.time_emb_proj.bias", "conv_out.weight",
          # 1280-channel self attention (level 2): the layers whose backward takes Delta from the out-projection dgrad where that applies
          "down_blocks.2.attentions.0.transformer_blocks.0.attn1.to_q.weight", "mid_block.attentions.0.transformer_blocks.0.attn1.to_k.weight"]


def test_cfg1_gradients_match_cpu_oracle(full, oracle_w):
    """cfg 1 at full size, backward: gradients of probe parameters spread over the network (first and last layer,
    self / cross attention projections, the packed GEGLU projection, convs, a shortcut, norm and bias vectors) against
    autograd through the fp32 CPU oracle on identical inputs (~1 minute of host CPU)."""
    net = full
    x = _inputs(1, 64, 64, seed=404)
    ts = torch.tensor([377])
    sig = R.karras_sigmas()[ts]
    net.zero_grads()
    net.forward_loss("ddpm", x["lat"], x["noise"], sig, ts.float(), x["ehs"], x["pooled"], x["tid"])
    net.backward(1.0, True)
    w = oracle_w
    _probe(w, PROBES)
    ref = R.compute_loss_ddpm(lambda s, t, e, p, ti: U.unet_forward(w, s, t, e, p, ti, U.SDXL_BASE),
                              {"vae_latents": x["lat"], "prompt_embeds": x["ehs"], "pooled_prompt_embeds": x["pooled"],
                               "time_ids": x["tid"]}, x["noise"], ts)
    grads = torch.autograd.grad(ref["loss"], [w[k] for k in PROBES])
    worst = 1.0
    for k, gr in zip(PROBES, grads):
        gh = net.export(k, grad=True).float().cpu().reshape(gr.shape)
        a, b = gh.double().flatten(), gr.double().flatten()
        cos = float((a @ b) / (a.norm() * b.norm()))       # (F.cosine_similarity clamps norms at 1e-8: these are ~1e-12)
        rl2 = float((gh - gr).norm() / gr.norm())
        print(f"[parity] FULL SDXL cfg1 grad {k}: cos {cos:.6f} rel-L2 {rl2:.3e} |g| {float(gr.norm()):.3e}")
        worst = min(worst, cos)
        assert rl2 <= 6e-2, (k, rl2)
    assert worst >= 0.998


HEADLINE_PROBES = ["down_blocks.0.resnets.0.conv1.weight",                                  # the 320 -> 320 conv at 128x128
                   "down_blocks.1.attentions.0.transformer_blocks.0.attn1.to_q.weight",    # level-1 self attention, N = 4096
                   "down_blocks.1.attentions.1.transformer_blocks.1.attn1.to_v.weight",
                   "up_blocks.1.attentions.2.transformer_blocks.1.attn1.to_k.weight",      # level-1, up path
                   "down_blocks.2.attentions.0.transformer_blocks.3.attn2.to_k.weight",    # cross attention
                   "mid_block.attentions.0.transformer_blocks.9.ff.net.0.proj.weight",     # packed GEGLU projection
                   "up_blocks.2.resnets.0.conv1.weight",                                   # 960 -> 320 at 128x128
                   "up_blocks.0.upsamplers.0.conv.weight", "down_blocks.0.downsamplers.0.conv.weight",
                   "conv_in.weight", "conv_out.weight", "up_blocks.2.resnets.2.norm2.weight",
                   # level-2 self attention (N = 1024 x 20 heads): the one-grid backward inside a plan + Delta from the dgrad epilogue
                   "down_blocks.2.attentions.0.transformer_blocks.0.attn1.to_q.weight", "mid_block.attentions.0.transformer_blocks.0.attn1.to_k.weight"]


@pytest.mark.parametrize("method", ["ddpm", "flow_matching"])
def test_headline_shape_b1_loss_and_gradients_match_cpu_oracle(full, oracle_w, method):
    """The HEADLINE shapes (latent 128x128 = 1024^2: level-1 self attention with Nq = Nk = 4096, the 128x128 convs)
    against the fp32 CPU oracle: one sample of configs[1] / configs[2] (B = 4 is the 1/B-weighted sum of such samples,
    test_flow_matching_batch_decomposes / test_ddpm_batch_decomposes below), loss <= 1e-3 relative (north_star) and 12
    gradient probes.  ~20 TFLOP of host CPU work per method (fp32 autograd through the oracle)."""
    net = full
    x = _inputs(1, 128, 128, seed=515 if method == "ddpm" else 616)
    w = oracle_w
    _probe(w, HEADLINE_PROBES)
    unet_fn = lambda s, t, e, p, ti: U.unet_forward(w, s, t, e, p, ti, U.SDXL_BASE)
    batch = {"vae_latents": x["lat"], "prompt_embeds": x["ehs"], "pooled_prompt_embeds": x["pooled"], "time_ids": x["tid"]}
    net.zero_grads()
    if method == "ddpm":
        ts = torch.tensor([613])
        sig = R.karras_sigmas()[ts]
        net.forward_loss("ddpm", x["lat"], x["noise"], sig, ts.float(), x["ehs"], x["pooled"], x["tid"])
        ref = R.compute_loss_ddpm(unet_fn, batch, x["noise"], ts)
    else:
        t = torch.tensor([0.3671875])                      # exactly representable in bf16 (D6: t reaches the UNet in model dtype)
        net.forward_loss("flow_matching", x["lat"], x["noise"], t, t, x["ehs"], x["pooled"], x["tid"])
        ref = R.compute_loss_flow(unet_fn, batch, x["noise"], t)
    net.backward(1.0, True)
    got = net.read_loss()[0]
    rel = abs(got - float(ref["loss"])) / abs(float(ref["loss"]))
    print(f"[parity] FULL SDXL 1024^2 B=1 {method} loss: hip {got:.6e} oracle {float(ref['loss']):.6e} rel {rel:.3e}")
    assert rel <= 1e-3
    grads = torch.autograd.grad(ref["loss"], [w[k] for k in HEADLINE_PROBES])
    worst = 1.0
    for k, gr in zip(HEADLINE_PROBES, grads):
        gh = net.export(k, grad=True).float().cpu().reshape(gr.shape)
        a, b = gh.double().flatten(), gr.double().flatten()
        cos = float((a @ b) / (a.norm() * b.norm()))
        rl2 = float((gh - gr).norm() / gr.norm())
        print(f"[parity] FULL SDXL 1024^2 {method} grad {k}: cos {cos:.6f} rel-L2 {rl2:.3e} |g| {float(gr.norm()):.3e}")
        worst = min(worst, cos)
        assert rl2 <= 6e-2, (k, rl2)
    assert worst >= 0.998


@pytest.mark.parametrize("method", ["ddpm", "flow_matching"])
def test_headline_batch4_loss_matches_cpu_oracle(full, oracle_w, method):
    """configs[1] / configs[2] at their STATED batch: B = 4 at latent 128x128, forward-only loss against the fp32 CPU oracle (27 TFLOP of
    host work per method).  Closes the indirect step of the B = 1 comparisons above: a batch-index bug that is consistent between the
    B = 4 plan and the B = 1 plan passes every HIP-vs-HIP decomposition test, but not this one.  Four different timesteps per batch: the
    per-sample MinSNR weight of the ddpm loss at B > 1 (ddpm_trainer.py:336-345, D3) and the per-sample t of the flow-matching path are
    exercised against the oracle directly.  Tolerance: north_star's 1e-3 relative."""
    net = full
    x = _inputs(4, 128, 128, seed=717 if method == "ddpm" else 818)
    w = oracle_w
    _probe(w, [])
    unet_fn = lambda s, t, e, p, ti: U.unet_forward(w, s, t, e, p, ti, U.SDXL_BASE)
    batch = {"vae_latents": x["lat"], "prompt_embeds": x["ehs"], "pooled_prompt_embeds": x["pooled"], "time_ids": x["tid"]}
    with torch.no_grad():
        if method == "ddpm":
            ts = torch.tensor([37, 402, 613, 951])
            sig = R.karras_sigmas()[ts]
            net.forward_loss("ddpm", x["lat"], x["noise"], sig, ts.float(), x["ehs"], x["pooled"], x["tid"])
            ref = R.compute_loss_ddpm(unet_fn, batch, x["noise"], ts)
        else:
            t = torch.tensor([0.0859375, 0.3671875, 0.62109375, 0.90625])       # exactly representable in bf16 (D6)
            net.forward_loss("flow_matching", x["lat"], x["noise"], t, t, x["ehs"], x["pooled"], x["tid"])
            ref = R.compute_loss_flow(unet_fn, batch, x["noise"], t)
    got = net.read_loss()[0]
    rel = abs(got - float(ref["loss"])) / abs(float(ref["loss"]))
    print(f"[parity] FULL SDXL 1024^2 B=4 {method} loss (configs[{1 if method == 'ddpm' else 2}]): hip {got:.6e} oracle {float(ref['loss']):.6e} rel {rel:.3e}")
    assert rel <= 1e-3


def test_bucket_1344x768_b1_loss_and_gradients_match_cpu_oracle(full, oracle_w):
    """configs[4]'s SECOND bucket (1344 x 768 -> latent 96 x 168, config.yaml:81-96) against the fp32 CPU oracle, one sample, flow matching
    (the method configs[4] names): loss <= 1e-3 and the headline probe list.  This shape is where the ragged forms live: 4032-token
    (level 1) and 1008-token (level 2) self attention -- 63 key tiles, 31.5 query blocks --, 84- and 42-pixel conv rows, tile grids no XCD
    rectangle divides.  ~20 TFLOP of host CPU work."""
    net = full
    x = _inputs(1, 96, 168, seed=919)
    assert x["tid"][0].tolist() == [1344.0, 768.0, 0.0, 0.0, 1344.0, 768.0]
    w = oracle_w
    _probe(w, HEADLINE_PROBES)
    unet_fn = lambda s, t, e, p, ti: U.unet_forward(w, s, t, e, p, ti, U.SDXL_BASE)
    batch = {"vae_latents": x["lat"], "prompt_embeds": x["ehs"], "pooled_prompt_embeds": x["pooled"], "time_ids": x["tid"]}
    t = torch.tensor([0.62109375])
    net.zero_grads()
    net.forward_loss("flow_matching", x["lat"], x["noise"], t, t, x["ehs"], x["pooled"], x["tid"])
    net.backward(1.0, True)
    ref = R.compute_loss_flow(unet_fn, batch, x["noise"], t)
    got = net.read_loss()[0]
    rel = abs(got - float(ref["loss"])) / abs(float(ref["loss"]))
    print(f"[parity] FULL SDXL 1344x768 B=1 flow_matching loss: hip {got:.6e} oracle {float(ref['loss']):.6e} rel {rel:.3e}")
    assert rel <= 1e-3
    grads = torch.autograd.grad(ref["loss"], [w[k] for k in HEADLINE_PROBES])
    worst = 1.0
    for k, gr in zip(HEADLINE_PROBES, grads):
        gh = net.export(k, grad=True).float().cpu().reshape(gr.shape)
        a, b = gh.double().flatten(), gr.double().flatten()
        cos = float((a @ b) / (a.norm() * b.norm()))
        rl2 = float((gh - gr).norm() / gr.norm())
        print(f"[parity] FULL SDXL 1344x768 flow_matching grad {k}: cos {cos:.6f} rel-L2 {rl2:.3e} |g| {float(gr.norm()):.3e}")
        worst = min(worst, cos)
        assert rl2 <= 6e-2, (k, rl2)
    assert worst >= 0.998


FULL_GRAD_BAR = (6e-2, 0.998)      # per tensor, every one of the 1 680: the bar of the probe comparisons above
# Biases, convolution weights and the time-embedding path measure far below it: worst rel-L2 8.4e-3 / cos 0.99996 over the
# three B = 1 shapes against the oracle (up_blocks.0.resnets.0.conv_shortcut.weight at 1024^2) and 7.3e-3 over the B = 4
# decompositions, against 2.0e-2 / 1.7e-2 for the linears / norms -- so they answer to a bar of their own, ~2.5x above that.
TIGHT_GRAD_BAR = (2e-2, 0.9995)
TIGHT_GROUPS = ("biases", "convs", "time-embedding path")


def _grad_bar(shapes):
    return lambda k: TIGHT_GRAD_BAR if group(k, len(shapes[k])) in TIGHT_GROUPS else FULL_GRAD_BAR


def _every_gradient_vs_oracle(net, w, label, method, x, ts):
    """One B = 1 step on the GPU and autograd of the fp32 oracle loss into all 1 680 weights: each reference gradient is compared
    with net.export(k, grad=True) as soon as autograd has it, then freed (the 10.3 GB of reference gradients never coexist)."""
    _probe(w, list(w))
    unet_fn = lambda s, t, e, p, ti: U.unet_forward(w, s, t, e, p, ti, U.SDXL_BASE)
    batch = {"vae_latents": x["lat"], "prompt_embeds": x["ehs"], "pooled_prompt_embeds": x["pooled"], "time_ids": x["tid"]}
    net.zero_grads()
    if method == "ddpm":
        sig = R.karras_sigmas()[ts]
        net.forward_loss("ddpm", x["lat"], x["noise"], sig, ts.float(), x["ehs"], x["pooled"], x["tid"])
        ref = R.compute_loss_ddpm(unet_fn, batch, x["noise"], ts)
    else:
        net.forward_loss("flow_matching", x["lat"], x["noise"], ts, ts, x["ehs"], x["pooled"], x["tid"])
        ref = R.compute_loss_flow(unet_fn, batch, x["noise"], ts)
    net.backward(1.0, True)
    got = net.read_loss()[0]
    rel = abs(got - float(ref["loss"])) / abs(float(ref["loss"]))
    assert rel <= 1e-3, rel
    par = GradParity(label)
    try:
        compare_autograd(par, ref["loss"], {k: w[k] for k in net.param_shapes()}, lambda k: net.export(k, grad=True))
    finally:
        del ref
        _probe(w, [])
    par.check(_grad_bar(net.param_shapes()), expect=net.param_shapes())


def test_cfg1_every_gradient_matches_cpu_oracle(full, oracle_w):
    """cfg 1 (ddpm, B = 1, 512^2), the inputs of test_cfg1_gradients_match_cpu_oracle: all 1 680 gradient tensors -- the up-sampler
    bias column sums, the time-embedding path's per-sample column sums, norm parameters, split-K bias rows -- against the oracle."""
    _every_gradient_vs_oracle(full, oracle_w, "FULL cfg1 ddpm 1x64x64", "ddpm", _inputs(1, 64, 64, seed=404), torch.tensor([377]))


@pytest.mark.parametrize("method", ["ddpm", "flow_matching"])
def test_headline_shape_b1_every_gradient_matches_cpu_oracle(full, oracle_w, method):
    """1024^2 (latent 128 x 128), B = 1, the inputs of the headline probe test: all 1 680 gradient tensors against the oracle."""
    x = _inputs(1, 128, 128, seed=515 if method == "ddpm" else 616)
    ts = torch.tensor([613]) if method == "ddpm" else torch.tensor([0.3671875])
    _every_gradient_vs_oracle(full, oracle_w, f"FULL 1024^2 {method} 1x128x128", method, x, ts)


def test_bucket_1344x768_b1_every_gradient_matches_cpu_oracle(full, oracle_w):
    """The 1344 x 768 bucket (latent 96 x 168, ragged attention and conv tiles), flow matching, B = 1: all 1 680 gradient tensors."""
    _every_gradient_vs_oracle(full, oracle_w, "FULL 1344x768 flow_matching 1x96x168", "flow_matching", _inputs(1, 96, 168, seed=919),
                              torch.tensor([0.62109375]))


def test_configs1_shape_step_properties(full):
    """BASELINE configs[1] (B=4, 1024^2): reproducible loss, finite gradients, accumulation = sum of micro-steps."""
    net = full
    x = _inputs(4, 128, 128, seed=202)
    ts = torch.tensor([12, 450, 700, 930])
    sig = R.karras_sigmas()[ts]

    def step(scale, first):
        net.forward_loss("ddpm", x["lat"], x["noise"], sig, ts.float(), x["ehs"], x["pooled"], x["tid"])
        net.backward(scale, first)
        return net.read_loss()[0]

    net.zero_grads()
    l1 = step(1.0, True)
    n1 = net.grad_norm()
    probe = "mid_block.attentions.0.transformer_blocks.4.ff.net.2.weight"
    g1 = net.export(probe, grad=True).clone()
    net.zero_grads()
    l2 = step(0.5, True)
    step(0.5, False)
    n2 = net.grad_norm()
    g2 = net.export(probe, grad=True)
    print(f"[parity] configs[1] loss {l1:.6f} |grad| {n1:.4e} ; two half-scaled micro-steps |grad| {n2:.4e}")
    rel_g = float((g2 - g1).norm() / g1.norm())
    print(f"[parity] l1 {l1!r} l2 {l2!r} n1 {n1!r} n2 {n2!r} probe rel {rel_g:.3e}")
    assert l1 == l2, (l1, l2)      # forward and loss are fixed-order sums: same bits
    assert math.isfinite(l1) and 0 < l1 < 1000
    assert math.isfinite(n1) and n1 > 0
    assert abs(n2 - n1) <= 2e-3 * n1                       # bf16 d(pred) scaling is the only difference
    assert rel_g <= 5e-3


def test_headline_shape_grad_emit_equals_cast(full):
    """configs[1] shape (B=4, 1024^2 -- the shape at which three 1280x1280 wgrads go out per grouped launch and the K | V wgrad
    runs over padded rows): the bf16 exchange arena written by the wgrad epilogues (sdxl_set_grad_emit; TN epilogue, split-K
    reduce, grouped launches) + the small-range casts has the bits of a cast of the fp32 gradient arena."""
    import ctypes as C
    from sdxl_amd import lib
    net = full
    x = _inputs(4, 128, 128, seed=303)
    ts = torch.tensor([450, 613, 700, 820])
    sig = R.karras_sigmas()[ts]
    n = net.param_elems

    def step(arena):
        net.zero_grads()
        net.forward_loss("ddpm", x["lat"], x["noise"], sig, ts.float(), x["ehs"], x["pooled"], x["tid"])
        if arena is None:
            net.backward(0.25, True)
        else:
            net.set_grad_emit(arena, 1.0)
            net.backward(0.25, True, on_segment=lambda k, off, cnt: net.cast_small(off, cnt, arena[off:off + cnt]), segment_stream=True)
            net.set_grad_emit(None)

    step(None)
    ref = torch.zeros(n, dtype=torch.bfloat16, device="cuda")
    lib.check(net.L.sdxl_grads_to_bf16(net.h, 0, n, C.c_void_p(ref.data_ptr()), 1.0, C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    got = torch.zeros(n, dtype=torch.bfloat16, device="cuda")
    step(got)
    torch.cuda.synchronize()
    differ = 0
    worst = 0.0
    scale = float(ref.float().abs().max())
    for i in range(0, n, 1 << 28):                     # in slices: the fp32 differences of 2.6 G elements need not all be resident
        d = (got[i:i + (1 << 28)].float() - ref[i:i + (1 << 28)].float()).abs()
        differ += int((d > 0).sum())
        worst = max(worst, float(d.max()))
    print(f"[parity] full-size grad emit: {differ} of {n} elements differ, max |d| / max |ref| = {worst / scale:.2e}")
    assert worst <= 2e-2 * scale
    assert differ <= 3_000_000        # biases / norm parameters (2.1 M elements of fp32 atomic sums) only


def test_ddpm_batch_decomposes(full):
    """configs[1] (ddpm v-pred + MinSNR, B=4, 1024^2): per-sample weights (D3) -- the batch loss is the mean of the
    per-sample losses and the gradient the 1/B-weighted sum, which ties the B=4 step to the B=1 oracle comparison."""
    net = full
    B, H, W = 4, 128, 128
    x = _inputs(B, H, W, seed=808)
    ts = torch.tensor([450, 613, 700, 820])        # moderate sigmas: every per-sample loss stays below the (non-linear) 1000 cap
                                                   # (t = 12: sigma ~ 1.8e4 blows the prediction up, t = 930: 1 / sigma^2 the target)
    sig = R.karras_sigmas()[ts]
    probe = "down_blocks.1.attentions.0.transformer_blocks.0.attn1.to_q.weight"

    def run(idx, scale, first):
        s = slice(idx, idx + 1) if idx is not None else slice(None)
        net.forward_loss("ddpm", x["lat"][s], x["noise"][s], sig[s], ts[s].float(), x["ehs"][s], x["pooled"][s], x["tid"][s])
        net.backward(scale, first)
        return net.read_loss()[0]

    net.zero_grads()
    lb = run(None, 1.0, True)
    gb = net.export(probe, grad=True).clone()
    nb = net.grad_norm()
    net.zero_grads()
    ls = [run(i, 1.0 / B, i == 0) for i in range(B)]
    gs = net.export(probe, grad=True)
    ns = net.grad_norm()
    mean = sum(ls) / B
    rel_g = float((gs - gb).norm() / gb.norm())
    print(f"[parity] ddpm {B}x{H}x{W}: batch loss {lb:.6f} mean of per-sample {mean:.6f}; |grad| {nb:.4e} vs {ns:.4e}; probe rel {rel_g:.3e}")
    assert abs(lb - mean) <= 1e-3 * abs(lb)
    assert abs(nb - ns) <= 5e-3 * nb and rel_g <= 1e-2


@pytest.mark.parametrize("shape", [(3, 64, 64), (5, 64, 64), (6, 64, 64)], ids=["b3_512sq", "b5_512sq", "b6_512sq"])
def test_split_dgrad_shapes_keep_their_delta_pass(full, shape):
    """Shapes where a self-attention layer's out-projection dgrad is SPLIT over K (gemm_pick_splitk_small > 1: B = 3 at 512^2 has 3072
    rows at the 640-channel level, B = 5 / 6 have 1280 / 1536 rows at the 1280-channel level) while the attention backward runs
    unsplit: the split launch goes through the slab epilogue, which cannot write Delta, so the plan must keep the stand-alone Delta
    pass there (engine.hip LinearOp::plan_bwd decides once for both sides; it once told the attention backward that Delta was ready
    although nobody wrote it).  Property: the batch gradient is the 1/B-weighted sum of the per-sample gradients -- the B = 1 steps
    take the query-split attention backward with its own Delta pass, an independent path."""
    net = full
    B, H, W = shape
    x = _inputs(B, H, W, seed=1200 + B)
    ts = torch.tensor([450, 613, 700, 820, 377, 555][:B])
    sig = R.karras_sigmas()[ts]
    probes = ["down_blocks.1.attentions.0.transformer_blocks.0.attn1.to_q.weight", "down_blocks.2.attentions.1.transformer_blocks.4.attn1.to_k.weight",
              "up_blocks.0.attentions.0.transformer_blocks.2.attn1.to_v.weight"]

    def run(idx, scale, first):
        s = slice(idx, idx + 1) if idx is not None else slice(None)
        net.forward_loss("ddpm", x["lat"][s], x["noise"][s], sig[s], ts[s].float(), x["ehs"][s], x["pooled"][s], x["tid"][s])
        net.backward(scale, first)
        return net.read_loss()[0]

    net.zero_grads()
    lb = run(None, 1.0, True)
    gb = {k: net.export(k, grad=True).clone() for k in probes}
    nb = net.grad_norm()
    net.zero_grads()
    ls = [run(i, 1.0 / B, i == 0) for i in range(B)]
    ns = net.grad_norm()
    assert abs(lb - sum(ls) / B) <= 1e-3 * abs(lb)
    for k in probes:
        gs = net.export(k, grad=True)
        rel = float((gs - gb[k]).norm() / gb[k].norm())
        cos = float((gs.double().flatten() @ gb[k].double().flatten()) / (gs.double().norm() * gb[k].double().norm()))
        print(f"[parity] ddpm {B}x{H}x{W} {k}: batch vs per-sample sum rel {rel:.3e} cos {cos:.6f}")
        # (the bar of the oracle gradient comparisons, 6e-2 / 0.998: the per-sample steps run 256-row problems through split-K forward / dgrad
        #  launches and the query-split attention backward -- other bf16 roundings of every activation gradient: 0.6 ... 4e-2 here, the same with
        #  the Delta epilogue forced off, profiles/tools/dbg_delta_b5.py, and the same on weights far from any attention; a Delta that nobody
        #  wrote is the previous step's, i.e. an error of order 1)
        assert rel <= 6e-2 and cos >= 0.998, (k, rel, cos)
    assert abs(nb - ns) <= 5e-3 * nb


@pytest.mark.parametrize("shape", [(4, 128, 128), (4, 96, 168)], ids=["configs2_1024sq", "configs4_bucket_1344x768_b4"])
def test_flow_matching_batch_decomposes(full, shape):
    """BASELINE configs[2] (flow matching, B=4, 1024^2) and the second bucket of configs[4] (1344x768 -> latent 96x168):
    size-independent property -- the batch loss is the mean of the per-sample losses (every sample has its own t and
    its rows go through the same kernels), and a batch's gradient is the sum of its samples' gradients."""
    net = full
    B, H, W = shape
    x = _inputs(B, H, W, seed=303 + H)
    t = torch.sigmoid(torch.randn(B, generator=torch.Generator().manual_seed(9)))
    probe = "down_blocks.2.attentions.1.transformer_blocks.7.attn2.to_q.weight"

    def run(idx, scale, first):
        s = slice(idx, idx + 1) if idx is not None else slice(None)
        net.forward_loss("flow_matching", x["lat"][s], x["noise"][s], t[s], t[s], x["ehs"][s], x["pooled"][s], x["tid"][s])
        net.backward(scale, first)
        return net.read_loss()[0]

    net.zero_grads()
    lb = run(None, 1.0, True)
    gb = net.export(probe, grad=True).clone()
    nb = net.grad_norm()
    net.zero_grads()
    ls = [run(i, 1.0 / B, i == 0) for i in range(B)]          # per-sample steps accumulated with weight 1/B
    gs = net.export(probe, grad=True)
    ns = net.grad_norm()
    mean = sum(ls) / B
    rel_g = float((gs - gb).norm() / gb.norm())
    print(f"[parity] flow matching {B}x{H}x{W}: batch loss {lb:.6f} mean of per-sample {mean:.6f}; |grad| {nb:.4e} vs {ns:.4e}; probe rel {rel_g:.3e}")
    assert math.isfinite(lb) and 0 < lb < 1000
    assert abs(lb - mean) <= 1e-3 * abs(lb)
    # (the per-sample steps are small problems and take the split-K forward / dgrad launches: another fp32 summation order, the
    #  same bits to bf16 noise)
    assert abs(nb - ns) <= 5e-3 * nb and rel_g <= 1e-2


@pytest.mark.parametrize("method,shape", [("ddpm", (4, 128, 128)), ("flow_matching", (4, 128, 128)), ("flow_matching", (4, 96, 168))],
                         ids=["configs1_ddpm_1024sq", "configs2_flow_1024sq", "configs4_bucket_1344x768_b4"])
def test_batch4_every_gradient_decomposes(full, method, shape):
    """B = 4 is what bench.py times, and only B = 4 takes the 4096-row pl forward / dgrad, the cr256 weight gradients (grouped launches
    of three 1280^2 outputs), wgrad256 over 16 384 rows and cfg 13 at M = 16 384.  Every tensor of the B = 4 gradient arena equals the
    1/B-weighted sum of the four per-sample steps' arenas (which the B = 1 oracle tests tie to the fp32 CPU oracle), slice by slice
    of the packed arena, on the device.  Bar: that of test_split_dgrad_shapes_keep_their_delta_pass, whose pairs differ the same way
    (the per-sample steps take split-K forward / dgrad launches and the query-split attention backward)."""
    net = full
    B, H, W = shape
    if method == "ddpm":
        x = _inputs(B, H, W, seed=808)
        ts = torch.tensor([450, 613, 700, 820])
        sig = R.karras_sigmas()[ts]
        a, b = sig, ts.float()
    else:
        x = _inputs(B, H, W, seed=303 + H)
        a = b = torch.sigmoid(torch.randn(B, generator=torch.Generator().manual_seed(9)))

    def run(idx, scale, first):
        s = slice(idx, idx + 1) if idx is not None else slice(None)
        net.forward_loss(method, x["lat"][s], x["noise"][s], a[s], b[s], x["ehs"][s], x["pooled"][s], x["tid"][s])
        net.backward(scale, first)

    net.zero_grads()
    run(None, 1.0, True)
    gb = net.grads.clone()                  # 10.3 GB on the device; nothing leaves it
    net.zero_grads()
    for i in range(B):
        run(i, 1.0 / B, i == 0)
    torch.cuda.synchronize()
    par = GradParity(f"B=4 decomposition {method} {B}x{H}x{W}")
    par.add_arena(net.grads, gb, net.param_ranges(), net.param_shapes())
    del gb
    par.check(_grad_bar(net.param_shapes()), expect=net.param_shapes())


def test_configs4_mixed_buckets_accumulate_across_plans(full):
    """configs[4] (flow matching, buckets 1024x1024 and 1344x768 alternating micro-step by micro-step, gradient accumulation): two
    plans share the weights, the gradient arena and the workspace; a cycle over both buckets accumulates exactly the sum of the
    two buckets' own gradients, in either order."""
    net = full
    shapes = [(4, 128, 128), (4, 96, 168)]
    xs = [_inputs(*s, seed=410 + i) for i, s in enumerate(shapes)]
    ts = [torch.tensor([0.15, 0.4, 0.65, 0.9]), torch.tensor([0.1, 0.35, 0.6, 0.85])]
    probes = ["down_blocks.2.attentions.1.transformer_blocks.3.attn1.to_out.0.weight", "up_blocks.1.resnets.0.conv1.weight",
              "mid_block.attentions.0.transformer_blocks.7.attn2.to_k.weight"]

    def micro(i, scale, first):
        x, t = xs[i], ts[i]
        net.forward_loss("flow_matching", x["lat"], x["noise"], t, t, x["ehs"], x["pooled"], x["tid"])
        net.backward(scale, first)
        return net.read_loss()[0]

    singles = []
    for i in range(2):
        net.zero_grads()
        micro(i, 0.5, True)
        singles.append({k: net.export(k, grad=True).clone() for k in probes})
    for order in ((0, 1), (1, 0)):
        net.zero_grads()
        losses = [micro(i, 0.5, j == 0) for j, i in enumerate(order)]
        assert all(math.isfinite(l) and 0 < l < 1000 for l in losses)
        for k in probes:
            acc = net.export(k, grad=True)
            ref = singles[0][k] + singles[1][k]
            rel = float((acc - ref).norm() / ref.norm())
            print(f"[parity] mixed buckets order {order} {k}: rel {rel:.3e}")
            assert rel <= 1e-5, (order, k, rel)


def test_small_batch_accumulation_is_run_to_run_reproducible(full):
    """Batch-1 micro-steps (where self-attention's dK / dV also goes through query-split partials, on the caller's stream, while
    cross-attention's runs on the side stream) accumulated over different samples give the same gradient norm every time: the
    two kernels' partial scratch buffers are separate (they once were not: a race only changing inputs made visible)."""
    net = full
    B, H, W = 3, 96, 168
    x = _inputs(B, H, W, seed=77)
    t = torch.tensor([0.2, 0.5, 0.8])
    norms = []
    for _ in range(4):
        net.zero_grads()
        for i in range(B):
            s = slice(i, i + 1)
            net.forward_loss("flow_matching", x["lat"][s], x["noise"][s], t[s], t[s], x["ehs"][s], x["pooled"][s], x["tid"][s])
            net.backward(1.0 / B, i == 0)
        norms.append(net.grad_norm())
    print(f"[parity] small-batch accumulation |grad| over 4 repeats: {norms}")
    assert max(norms) == min(norms), norms


def test_headline_step_is_bitwise_reproducible(full):
    """configs[1] (B=4, 1024^2): the SAME step three times, with a different step in between -- the loss and the WHOLE fp32 gradient arena
    (2.57 G values: weights, biases, norm parameters, the time-embedding path) have the same bits every time.  Nothing on the path adds
    floating-point numbers in an order the hardware chooses: split-K partial tiles and bias partials are slab rows summed in a fixed order,
    norm parameter gradients and the per-sample column sums are partial rows + one fixed-order reduce, the loss is block rows + one wave."""
    net = full
    xa, xb = _inputs(4, 128, 128, seed=411), _inputs(4, 128, 128, seed=412)
    ts = torch.tensor([33, 480, 720, 960])
    sig = R.karras_sigmas()[ts]

    def step(x):
        net.zero_grads()
        net.forward_loss("ddpm", x["lat"], x["noise"], sig, ts.float(), x["ehs"], x["pooled"], x["tid"])
        net.backward(1.0, True)
        torch.cuda.synchronize()
        return net.read_loss()[0]

    l1 = step(xa)
    g1 = net.grads.clone()
    step(xb)
    l2 = step(xa)
    diff = int((net.grads.view(torch.int32) != g1.view(torch.int32)).sum())
    l3 = step(xa)
    diff3 = int((net.grads.view(torch.int32) != g1.view(torch.int32)).sum())
    print(f"[parity] bitwise repeat: loss {l1!r} / {l2!r} / {l3!r}; gradient elements that differ: {diff} / {diff3} of {g1.numel()}")
    del g1
    assert l1 == l2 == l3
    assert diff == 0 and diff3 == 0


@pytest.mark.parametrize("B", [4, 2, 1])
def test_step_results_do_not_depend_on_the_previous_step(full, B):
    """A step's loss and gradients are functions of its inputs only: A, then B, then A again gives A's numbers again, bit for bit -- what a missing stream dependency or a shared scratch buffer would break, and
    what repeating the SAME step cannot show (stale data of an identical step is the right data)."""
    net = full
    xa, xb = _inputs(B, 128, 128, seed=901), _inputs(B, 128, 128, seed=902)
    ts = torch.tensor([100, 400, 650, 900][:B])
    sig = R.karras_sigmas()[ts]
    probes = ["mid_block.attentions.0.transformer_blocks.3.attn1.to_v.weight", "down_blocks.2.attentions.0.transformer_blocks.2.attn2.to_k.weight",
              "up_blocks.1.resnets.1.conv1.weight", "up_blocks.0.attentions.1.transformer_blocks.8.ff.net.2.weight"]

    def step(x):
        net.zero_grads()
        net.forward_loss("ddpm", x["lat"], x["noise"], sig, ts.float(), x["ehs"], x["pooled"], x["tid"])
        net.backward(1.0, True)
        return net.read_loss()[0], net.grad_norm(), {k: net.export(k, grad=True).clone() for k in probes}

    l1, n1, g1 = step(xa)
    step(xb)
    l2, n2, g2 = step(xa)
    print(f"[parity] B={B}: loss {l1!r} / {l2!r}, |grad| {n1!r} / {n2!r}")
    assert l1 == l2 and n1 == n2      # every sum on the path is a fixed-order one: the same bits
    for k in probes:
        assert torch.equal(g1[k], g2[k]), k
