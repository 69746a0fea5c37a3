"""Model-level parity on a real MI355X: the whole HIP training step (loss prep -> UNet fwd -> loss -> UNet bwd)
through the C ABI vs the fp32 CPU oracle (oracle/unet_ref.py + oracle/loss_ref.py) on identical seeded inputs.

Tolerance: north_star asks for <= 1e-3 relative on the loss vs the fp32 CPU reference arithmetic; the HIP path
stores activations in bf16 (fp32 accumulate), so per-element predictions carry ~1e-2 relative noise that averages
out in the loss.  Gradients are compared per tensor by relative L2 error and cosine similarity."""
import math

import pytest
import torch

import sdxl_amd  # noqa: F401
from oracle import loss_ref as R
from oracle import unet_ref as U
from sdxl_amd import unet as NU

import _bucket_cases as BK      # the default aspect buckets' latent shapes (tests/test_host_buckets.py pins them to the config)
from _gradparity import GradParity, compare_autograd
from _isolation import FILLS, assert_step_isolated, fill_bytes, same_bits

pytestmark = pytest.mark.gpu

LOSS_RTOL = 1e-3


def tiny_native_cfg(c: U.UNetConfig):
    return NU.make_config(block_out_channels=c.block_out_channels, transformer_layers=c.transformer_layers_per_block,
                          cross_attention_dim=c.cross_attention_dim, addition_time_embed_dim=c.addition_time_embed_dim,
                          pooled_dim=c.pooled_dim)


def make_inputs(cfg, B, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)
    bfr = lambda t: t.to(torch.bfloat16).float()
    return dict(lat=r(B, 4, H, W), noise=r(B, 4, H, W), ehs=bfr(r(B, 77, cfg.cross_attention_dim)),
                pooled=bfr(r(B, cfg.pooled_dim)), tid=torch.tensor([[8.0 * H, 8.0 * W, 0, 0, 8.0 * H, 8.0 * W]] * B),
                z=r(B))


@pytest.fixture(scope="module")
def tiny():
    cfg = U.tiny_config()
    w = U.synth_weights(cfg, seed=0)
    net = NU.NativeUNet(tiny_native_cfg(cfg))
    assert net.param_shapes() == {k: tuple(v) for k, v in U.param_shapes(cfg).items()}
    net.load_state_dict(w)
    yield cfg, w, net
    net.close()


def test_weight_roundtrip(tiny):
    cfg, w, net = tiny
    for k in ("conv_in.weight", "down_blocks.1.attentions.0.transformer_blocks.0.attn1.to_k.weight",
              "up_blocks.0.resnets.2.conv1.weight", "conv_out.bias", "mid_block.attentions.0.proj_in.weight",
              "down_blocks.2.attentions.1.transformer_blocks.1.attn2.to_v.weight"):
        got = net.export(k).cpu()
        assert torch.equal(got, w[k]), k


def _bhw_id(B, H, W):
    return f"{B}-{H}-{W}"


# the tiny config keeps a bucket's spatial geometry exactly (row widths, token counts with 64-wide heads, pad rows, the up-sampler
# weight-gradient fallback, the three-tap policy at level 0): every default bucket's latent shape at B = 1, two of them at B = 2
@pytest.mark.parametrize("B,H,W", [pytest.param(2, 16, 16, id="16-16"), pytest.param(2, 24, 40, id="24-40")]
                         + [pytest.param(*s, id=_bhw_id(*s)) for s in BK.TINY_LATENTS + BK.TINY_LATENTS_B2])
def test_unet_forward_matches_oracle(tiny, B, H, W):
    cfg, w, net = tiny
    x = make_inputs(cfg, B, H, W, seed=3)
    sample = (x["lat"] * 2.0).to(torch.bfloat16).float()
    t = torch.tensor([10.0, 500.0][2 - B:])
    got = net.unet_forward(sample, t, x["ehs"], x["pooled"], x["tid"]).cpu()
    ref = U.unet_forward(w, sample, t, x["ehs"], x["pooled"], x["tid"], cfg)
    ref_bf = U.unet_forward(w, sample, t, x["ehs"], x["pooled"], x["tid"], cfg, emulate_bf16=True)
    e = float((got - ref).abs().max() / ref.abs().max())
    e_bf = float((ref_bf - ref).abs().max() / ref.abs().max())
    print(f"[parity] tiny unet fwd {B}x{H}x{W}: hip vs fp32 oracle {e:.3e} ; bf16-emulating oracle vs fp32 oracle {e_bf:.3e}")
    assert e <= max(3.0 * e_bf, 2e-2)


def _grads_report(net, w, names):
    worst = 0.0
    for k in names:
        ref = w[k].grad
        got = net.export(k, grad=True).cpu()
        rel = float((got - ref).norm() / ref.norm().clamp_min(1e-30))
        cos = float(torch.nn.functional.cosine_similarity(got.flatten(), ref.flatten(), dim=0))
        print(f"[parity] grad {k}: rel-L2 {rel:.3e} cos {cos:.6f} |ref| {float(ref.norm()):.3e}")
        worst = max(worst, rel)
        assert cos > 0.995, (k, cos)
    return worst


PROBE_GRADS = ["conv_in.weight", "conv_out.weight", "conv_out.bias", "time_embedding.linear_1.weight",
               "add_embedding.linear_2.bias", "down_blocks.0.resnets.0.conv1.weight",
               "down_blocks.0.resnets.1.time_emb_proj.weight", "down_blocks.0.downsamplers.0.conv.weight",
               "down_blocks.1.resnets.0.conv_shortcut.weight", "down_blocks.1.resnets.0.norm1.weight",
               "down_blocks.1.attentions.0.norm.bias", "down_blocks.1.attentions.0.proj_in.weight",
               "down_blocks.1.attentions.0.transformer_blocks.0.norm1.weight",
               "down_blocks.1.attentions.0.transformer_blocks.0.attn1.to_q.weight",
               "down_blocks.1.attentions.0.transformer_blocks.0.attn1.to_v.weight",
               "down_blocks.1.attentions.0.transformer_blocks.0.attn1.to_out.0.bias",
               "down_blocks.1.attentions.0.transformer_blocks.0.attn2.to_k.weight",
               "down_blocks.1.attentions.0.transformer_blocks.0.ff.net.0.proj.weight",
               "down_blocks.1.attentions.0.transformer_blocks.0.ff.net.2.weight",
               "mid_block.resnets.1.conv2.weight", "mid_block.attentions.0.transformer_blocks.1.attn2.to_q.weight",
               "up_blocks.0.resnets.2.conv1.weight", "up_blocks.0.upsamplers.0.conv.weight",
               "up_blocks.1.attentions.2.proj_out.weight", "up_blocks.2.resnets.2.conv_shortcut.weight",
               "conv_norm_out.weight"]


@pytest.mark.parametrize("method", ["ddpm", "flow_matching"])
def test_training_step_matches_oracle(tiny, method):
    cfg, w, net = tiny
    B, H, W = 2, 16, 16
    x = make_inputs(cfg, B, H, W, seed=11)
    for t in w.values():
        t.grad = None
        t.requires_grad_(True)
    unet_fn = lambda s, t, e, p, ti: U.unet_forward(w, s, t, e, p, ti, cfg)
    batch = {"vae_latents": x["lat"], "prompt_embeds": x["ehs"], "pooled_prompt_embeds": x["pooled"], "time_ids": x["tid"]}
    if method == "ddpm":
        ts = torch.tensor([700, 420])
        sig = R.karras_sigmas()[ts]
        ref = R.compute_loss_ddpm(unet_fn, batch, x["noise"], ts)
        net.forward_loss("ddpm", x["lat"], x["noise"], sig, ts.float(), x["ehs"], x["pooled"], x["tid"])
    else:
        t = R.sample_logit_normal_from_z(x["z"])
        ref = R.compute_loss_flow(unet_fn, batch, x["noise"], t)
        net.forward_loss("flow_matching", x["lat"], x["noise"], t, t, x["ehs"], x["pooled"], x["tid"])
    net.zero_grads()
    net.backward(grad_scale=1.0, first_micro=True)
    out = net.read_loss()
    ref_loss = float(ref["loss"])
    rel = abs(out[0] - ref_loss) / abs(ref_loss)
    print(f"[parity] tiny {method} loss: hip {out[0]:.6f} oracle {ref_loss:.6f} rel {rel:.3e} (tol {LOSS_RTOL})")
    assert rel <= LOSS_RTOL
    if method == "ddpm":
        numel = x["lat"].numel()
        assert abs(out[2] / numel - ref["metrics"]["pred_scale"]) <= 2e-2 * ref["metrics"]["pred_scale"]
        assert abs(out[4] / numel - ref["metrics"]["noise_scale"]) <= 1e-5 * ref["metrics"]["noise_scale"]
    else:
        assert abs(math.sqrt(out[3]) - ref["metrics"]["velocity_norm"]) <= 2e-2 * ref["metrics"]["velocity_norm"]
        assert abs(math.sqrt(out[5]) - ref["metrics"]["x0_norm"]) <= 1e-5 * ref["metrics"]["x0_norm"]
        assert abs(math.sqrt(out[6]) - ref["metrics"]["x1_norm"]) <= 1e-5 * ref["metrics"]["x1_norm"]
    ref["loss"].backward()
    worst = _grads_report(net, w, PROBE_GRADS)
    print(f"[parity] tiny {method} worst grad rel-L2 over {len(PROBE_GRADS)} probes: {worst:.3e}")
    assert worst <= 6e-2
    for t in w.values():
        t.requires_grad_(False)


TINY_GRAD_BAR = (6e-2, 0.995)      # per tensor: rel-L2 <= 6e-2 (the probes' worst-case bar above), cosine >= 0.995


@pytest.mark.parametrize("method,B,H,W", [pytest.param(m, 2, H, W, id=f"{m}-{H}-{W}") for m in ("ddpm", "flow_matching") for H, W in ((16, 16), (24, 40))]
                         + [pytest.param("flow_matching", *s, id="flow_matching-" + _bhw_id(*s)) for s in BK.TINY_LATENTS + BK.TINY_LATENTS_B2]
                         + [pytest.param("ddpm", *s, id="ddpm-" + _bhw_id(*s)) for s in BK.TINY_DDPM])
def test_training_step_every_gradient_matches_oracle(tiny, method, B, H, W):
    """Every tiny-UNet gradient tensor (not only PROBE_GRADS) against autograd of the fp32 oracle loss: the bias / norm / time-
    embedding gradients that come out of hand-written column sums and fixed-order reduces included; 24 x 40 is the non-square
    shape of the forward test, with ragged tiles.  Then every default bucket's latent shape (flow matching for all nine at B = 1 and
    two at B = 2 with per-sample t, ddpm for one orientation of each new family): the conv row widths, the ragged token counts 3952 /
    988 and 3840 / 960, the linear weight gradients' zero-pad rows, the up-sampler weight gradient on the upsampled image, and at
    W = 192 / 128 the three-tap weight gradient at level 0.  BK.TINY_REPEAT's step is also run twice: the same bits in the whole arena."""
    cfg, w, net = tiny
    x = make_inputs(cfg, B, H, W, seed=13 if method == "ddpm" else 17)
    for t in w.values():
        t.grad = None
        t.requires_grad_(True)
    unet_fn = lambda s, t, e, p, ti: U.unet_forward(w, s, t, e, p, ti, cfg)
    batch = {"vae_latents": x["lat"], "prompt_embeds": x["ehs"], "pooled_prompt_embeds": x["pooled"], "time_ids": x["tid"]}
    if method == "ddpm":
        ts = torch.tensor([610, 230][:B])
        sig = R.karras_sigmas()[ts]
        ref = R.compute_loss_ddpm(unet_fn, batch, x["noise"], ts)
        step = lambda: net.forward_loss("ddpm", x["lat"], x["noise"], sig, ts.float(), x["ehs"], x["pooled"], x["tid"])
    else:
        tf = R.sample_logit_normal_from_z(x["z"])
        assert B == 1 or float(tf[0]) != float(tf[1])
        ref = R.compute_loss_flow(unet_fn, batch, x["noise"], tf)
        step = lambda: net.forward_loss("flow_matching", x["lat"], x["noise"], tf, tf, x["ehs"], x["pooled"], x["tid"])
    step()
    net.zero_grads()
    net.backward(grad_scale=1.0, first_micro=True)
    ref_loss = float(ref["loss"])
    got_loss = net.read_loss()[0]
    print(f"[parity] tiny {method} {B}x{H}x{W} loss: hip {got_loss:.6f} oracle {ref_loss:.6f} rel {abs(got_loss - ref_loss) / abs(ref_loss):.3e} (tol {LOSS_RTOL})")
    assert abs(got_loss - ref_loss) <= LOSS_RTOL * abs(ref_loss)
    par = GradParity(f"tiny {method} {B}x{H}x{W}")
    try:
        compare_autograd(par, ref["loss"], w, lambda k: net.export(k, grad=True))
    finally:
        for t in w.values():
            t.grad = None
            t.requires_grad_(False)
    par.check(TINY_GRAD_BAR, expect=net.param_shapes())
    if (B, H, W) == BK.TINY_REPEAT:          # the form of test_forward_is_bitwise_reproducible, on the whole step: no sum in an order the hardware chooses
        torch.cuda.synchronize()
        first = net.grads.clone()
        step()
        net.zero_grads()
        net.backward(grad_scale=1.0, first_micro=True)
        torch.cuda.synchronize()
        assert net.read_loss()[0] == got_loss
        assert torch.equal(net.grads.view(torch.int32), first.view(torch.int32)), "the repeated step's gradient arena differs"


def test_grad_accumulation_is_sum_of_micro_steps(tiny):
    """Two micro-steps with first_micro=(True, False) accumulate: grads == g(batch A)/2 + g(batch B)/2."""
    cfg, w, net = tiny
    B, H, W = 2, 16, 16
    xa, xb = make_inputs(cfg, B, H, W, seed=21), make_inputs(cfg, B, H, W, seed=22)
    ts = torch.tensor([300, 800])
    sig = R.karras_sigmas()[ts]
    names = ["down_blocks.1.attentions.0.transformer_blocks.0.attn1.to_q.weight", "mid_block.resnets.0.conv1.weight",
             "conv_norm_out.bias", "up_blocks.1.resnets.0.conv2.bias"]
    singles = []
    for x in (xa, xb):
        net.zero_grads()
        net.forward_loss("ddpm", x["lat"], x["noise"], sig, ts.float(), x["ehs"], x["pooled"], x["tid"])
        net.backward(0.5, True)
        singles.append({k: net.export(k, grad=True) for k in names})
    net.zero_grads()
    for i, x in enumerate((xa, xb)):
        net.forward_loss("ddpm", x["lat"], x["noise"], sig, ts.float(), x["ehs"], x["pooled"], x["tid"])
        net.backward(0.5, i == 0)
    for k in names:
        acc = net.export(k, grad=True)
        ref = singles[0][k] + singles[1][k]
        rel = float((acc - ref).norm() / ref.norm())
        print(f"[parity] accumulation {k}: rel {rel:.3e}")
        assert rel <= 1e-5          # same kernels, same order: only fp32 split-K atomics may reorder


def test_plan_cache_two_bucket_shapes(tiny):
    """cfg-5 style: alternate two bucket shapes on one handle; results independent of the interleaving."""
    cfg, w, net = tiny
    xa, xb = make_inputs(cfg, 2, 16, 16, seed=31), make_inputs(cfg, 2, 12, 20, seed=32)
    t = torch.tensor([0.3, 0.7])
    outs = []
    for _ in range(2):
        for x in (xa, xb):
            net.forward_loss("flow_matching", x["lat"], x["noise"], t, t, x["ehs"], x["pooled"], x["tid"])
            outs.append(net.read_loss()[0])
    assert outs[0] == outs[2] and outs[1] == outs[3]


def test_forward_is_bitwise_reproducible(tiny):
    """No atomics on the activation path: the same inputs give the same bits, run after run."""
    cfg, w, net = tiny
    x = make_inputs(cfg, 2, 16, 16, seed=41)
    t = torch.tensor([3.0, 900.0])
    outs = [net.unet_forward(x["lat"], t, x["ehs"], x["pooled"], x["tid"]) for _ in range(3)]
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])


def test_graph_replay_equals_eager_launches(tiny):
    """The captured step (hipGraph of both streams; first call eager, second captured, third replayed) gives the bits of the
    kernel-by-kernel launch sequence, for inputs that change (and move) from step to step, whole-backward and per-segment."""
    cfg, w, net = tiny
    B, H, W = 2, 16, 24
    ts = torch.tensor([250, 770])
    sig = R.karras_sigmas()[ts]
    names = ["down_blocks.1.attentions.0.transformer_blocks.0.attn2.to_k.weight", "mid_block.resnets.0.conv1.weight",
             "conv_in.weight", "up_blocks.1.resnets.0.conv2.bias", "time_embedding.linear_1.weight"]
    xs = [make_inputs(cfg, B, H, W, seed=50 + i) for i in range(4)]

    def run(per_segment):
        out = []
        for x in xs:
            net.zero_grads()
            net.forward_loss("ddpm", x["lat"].clone(), x["noise"].clone(), sig.clone(), ts.float(), x["ehs"], x["pooled"], x["tid"])
            net.backward(1.0, True, on_segment=(lambda k, off, n: None) if per_segment else None)
            out.append((net.read_loss()[0], {k: net.export(k, grad=True) for k in names}))
        return out

    for per_segment in (False, True):
        net.set_graph_mode(False)
        eager = run(per_segment)
        net.set_graph_mode(True)
        graphed = run(per_segment)
        net.set_graph_mode(False)
        for (le, ge), (lg, gg) in zip(eager, graphed):
            assert abs(le - lg) <= 1e-6 * abs(le)        # the loss sum's cross-block fp32 atomics
            for k in names:       # split-K fp32 atomics may reorder the last bits of a weight gradient, nothing else
                assert float((ge[k] - gg[k]).norm() / ge[k].norm()) <= 1e-5, k
    assert len({l for l, _ in graphed}) == len(xs)      # the replays did see the new inputs


def test_grad_emit_equals_cast_of_the_fp32_arena(tiny):
    """Exchange micro-step without the cast pass (sdxl_set_grad_emit): the bf16 arena the wgrad GEMMs write (+ the small-range
    cast) has the bits of the full cast of the fp32 arena -- alone and as the last micro-step of an accumulation cycle.
    (Biases / norm parameters are fp32 atomic sums: equal to rounding.)"""
    import ctypes as C
    from sdxl_amd import lib
    cfg, w, net = tiny
    B, H, W = 2, 16, 16
    ts = torch.tensor([120, 640])
    sig = R.karras_sigmas()[ts]
    xs = [make_inputs(cfg, B, H, W, seed=70 + i) for i in range(2)]
    n = net.param_elems
    st = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def cycle(emit_arena):
        net.zero_grads()
        for i, x in enumerate(xs):
            last = i == len(xs) - 1
            net.forward_loss("ddpm", x["lat"], x["noise"], sig, ts.float(), x["ehs"], x["pooled"], x["tid"])
            if last and emit_arena is not None:
                net.set_grad_emit(emit_arena, 0.5)
                net.backward(1.0, i == 0, on_segment=lambda k, off, cnt: net.cast_small(off, cnt, emit_arena[off:off + cnt], 0.5),
                             segment_stream=True)
                net.set_grad_emit(None)
            else:
                net.backward(1.0, i == 0)

    cycle(None)
    ref = torch.zeros(n, dtype=torch.bfloat16, device="cuda")
    lib.check(net.L.sdxl_grads_to_bf16(net.h, 0, n, C.c_void_p(ref.data_ptr()), 0.5, st()))
    got = torch.zeros(n, dtype=torch.bfloat16, device="cuda")
    cycle(got)
    torch.cuda.synchronize()
    d = (got.float() - ref.float()).abs()
    scale = float(ref.float().abs().max())
    assert scale > 0
    print(f"[parity] grad emit: {int((d > 0).sum())} of {n} elements differ, max |d| / max |ref| = {float(d.max()) / scale:.2e}")
    assert float(d.max()) <= 2e-2 * scale
    assert int((d > 0).sum()) <= 0.02 * n                       # only the atomically accumulated small parameters may differ


@pytest.mark.parametrize("micro_steps", [1, 2], ids=["one-step", "two-micro-steps"])
@pytest.mark.parametrize("method,B,H,W", [pytest.param("ddpm", 2, 16, 16, id="ddpm-2-16-16"), pytest.param("flow_matching", 2, 16, 16, id="flow_matching-2-16-16"),
                                          pytest.param("flow_matching", 1, 104, 152, id="flow_matching-1-104-152"),      # 988 / 3952 tokens: pad rows everywhere
                                          pytest.param("flow_matching", *BK.TINY_REPEAT, id="flow_matching-" + _bhw_id(*BK.TINY_REPEAT))])
def test_step_does_not_depend_on_workspace_or_stale_gradients(tiny, method, B, H, W, micro_steps):
    """The workspace is caller memory and first_micro OVERWRITES the weight-matrix gradients (include/sdxlstep.h): with every byte of the
    workspace and of the gradient arena set to 0xFF (NaN) or 0x7F (3.39e38) before the step, the loss and every parameter gradient have the
    bits of the step on zero-filled memory -- no tolerance, the step is bit-reproducible end to end.  Alone, and as a two-micro-step
    accumulation cycle whose workspace is filled again between the micro-steps."""
    cfg, w, net = tiny
    xs = [make_inputs(cfg, B, H, W, seed=81 + i) for i in range(micro_steps)]
    if method == "ddpm":
        ts = torch.tensor([610, 230][:B])
        sig = R.karras_sigmas()[ts]
        fwd = lambda x: (lambda: net.forward_loss("ddpm", x["lat"], x["noise"], sig, ts.float(), x["ehs"], x["pooled"], x["tid"]))
    else:
        fwd = lambda x: (lambda t=R.sample_logit_normal_from_z(x["z"]): net.forward_loss("flow_matching", x["lat"], x["noise"], t, t, x["ehs"], x["pooled"], x["tid"]))
    assert_step_isolated(net, (B, H, W), [fwd(x) for x in xs], what=f"tiny {method} {B}x{H}x{W} x{micro_steps}")


def test_inference_forward_does_not_depend_on_workspace(tiny):
    """unet_forward on a pattern-filled workspace gives the bits of the forward on a zero-filled one"""
    cfg, w, net = tiny
    B, H, W = 2, 24, 40
    x = make_inputs(cfg, B, H, W, seed=83)
    t = torch.tensor([10.0, 500.0])
    outs = []
    hip_failed = False
    try:
        for fill in FILLS:
            net.plan(B, H, W)
            fill_bytes(net.workspace, fill)
            outs.append(net.unet_forward(x["lat"], t, x["ehs"], x["pooled"], x["tid"]))
            torch.cuda.synchronize()
            assert bool(torch.isfinite(outs[-1]).all()), f"fill 0x{fill:02X}"
            assert same_bits(outs[-1], outs[0]), f"fill 0x{fill:02X}: the prediction differs from the clean workspace's"
    except RuntimeError:      # a failed HIP call: no further GPU work
        hip_failed = True
        raise
    finally:
        if not hip_failed:
            fill_bytes(net.workspace, 0)
