"""LoRA on the packed layouts (SDXL_DTYPE_LORA_LAYOUTS, training.lora_target_kinds "all") on a real MI355X: the kind-aware kernels of
csrc/lora.hip through their single-target hooks on NATIVE buffers (merge bit-equal to the restatement on the source view, a-priori bounded
projections, padded native rows, operand isolation), through sdxl_load_weight / sdxl_export_grad on the tiny UNet's handle with every
kind of target in one table, the oracle at the merged weights, and the trainer.  The source -> native maps the helpers here use are
checked against repack_kernel's formulas in tests/test_host_lora_layouts.py."""
import ctypes as C
import importlib
from pathlib import Path
from types import SimpleNamespace

import pytest
import torch

import sdxl_amd  # noqa: F401
from oracle import loss_ref as R
from oracle import unet_ref as U
from sdxl_amd import lib
from sdxl_amd import unet as NU

import _lora_ref as LR
from _gradparity import GradParity
from _isolation import Spec, assert_isolated, run_isolated, same_bits

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
CFG = importlib.import_module("sdxl-training-improvements_amd.config")
T = importlib.import_module("sdxl-training-improvements_amd.trainer")
LORA = importlib.import_module("sdxl-training-improvements_amd.lora")

GRAD_BAR = (6e-2, 0.995)          # TINY_GRAD_BAR of tests/test_gpu_model.py
DEV = "cuda"
PLAIN, CONV3, GEGLU = 0, 1, 2
GEGLU_GROUP = 64                  # the engine's packing group of ff.net.0.proj (csrc/engine.hip, LinearOp::ggroup)
RANKS = [1, 3, 16, 128]
# (label, kind, out, in, cin | G, native rows)
CASES = [("conv4x8pad8", CONV3, 4, 72, 8, 8), ("conv40x24", CONV3, 40, 216, 24, 40), ("conv130x40", CONV3, 130, 360, 40, 130),
         ("conv320x320", CONV3, 320, 2880, 320, 320),
         ("geglu64g64x8", GEGLU, 128, 8, 64, 128), ("geglu128g64x24", GEGLU, 256, 24, 64, 256), ("geglu320g80x40", GEGLU, 640, 40, 80, 640),
         ("geglu256g64x264", GEGLU, 512, 264, 64, 512),
         ("conv1x1_130x264", PLAIN, 130, 264, 0, 130)]
ALL_KINDS_TARGETS = list(LORA.DEFAULT_TARGETS) + ["ff.net.0.proj", "ff.net.2", "proj_in", "proj_out", "conv1", "conv2", "conv_shortcut",
                                                  "downsamplers.0.conv", "upsamplers.0.conv", "conv_out"]

bf = lambda t: t.to(torch.bfloat16)
ptr = lambda t: C.c_void_p(t.data_ptr())
stream = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)


# ------------------------------------------------------------------------------------------------ source <-> native (torch restatement)
def geglu_native_rows(out, G, device="cpu"):
    """native row of every source row: (c / G) 2G + half G + c % G, half = o / C4, c = o % C4"""
    C4 = out // 2
    o = torch.arange(out, device=device)
    half, c = o // C4, o % C4
    return (c // G) * 2 * G + half * G + c % G


def to_native(src, kind, cg, nrows, pad=None):
    """the [out, in] source view as the [nrows, in] native tensor; rows with no source element come from `pad` ([nrows, in])"""
    out, inn = src.shape
    if kind == CONV3:
        nat = src.view(out, cg, 9).permute(0, 2, 1).reshape(out, inn)
    elif kind == GEGLU:
        nat = torch.empty_like(src)
        nat[geglu_native_rows(out, cg, src.device)] = src
    else:
        nat = src
    if nrows > out:
        nat = torch.cat([nat, pad[out:]], 0)
    return nat.contiguous()


def to_source(nat, kind, cg, out):
    """the source view [out, in] of a native tensor [nrows, in]"""
    inn = nat.shape[1]
    if kind == CONV3:
        return nat[:out].view(out, 9, cg).permute(0, 2, 1).reshape(out, inn).contiguous()
    if kind == GEGLU:
        return nat[geglu_native_rows(out, cg, nat.device)].contiguous()
    return nat[:out].contiguous()


def operands(kind, out, inn, cg, nrows, rank, seed=0):
    g = torch.Generator().manual_seed(1000 * seed + 7 * out + inn + rank + 31 * kind)
    r = lambda *s: torch.randn(*s, generator=g)
    return dict(W0=bf(r(nrows, inn)).to(DEV), A=bf(r(rank, inn)).to(DEV), B=bf(r(out, rank)).to(DEV), dW=r(nrows, inn).to(DEV))


def hook_merge(W0, A, B, s, kind, cg):
    w = torch.full_like(W0, float("nan"))
    lib.check(lib.load().sdxl_op_lora_merge_layout(ptr(W0), ptr(A), ptr(B), ptr(w), B.shape[0], W0.shape[1], A.shape[0], s, kind, cg, W0.shape[0],
                                                   stream()), "lora_merge_layout")
    return w


def hook_project(dW, A, B, s, kind, cg):
    dA = torch.full(A.shape, float("nan"), dtype=torch.float32, device=dW.device)
    dB = torch.full(B.shape, float("nan"), dtype=torch.float32, device=dW.device)
    lib.check(lib.load().sdxl_op_lora_project_layout(ptr(dW), ptr(A), ptr(B), ptr(dA), ptr(dB), B.shape[0], dW.shape[1], A.shape[0], s, kind, cg,
                                                     dW.shape[0], stream()), "lora_project_layout")
    return dA, dB


def test_the_helpers_invert_each_other():
    for _label, kind, out, inn, cg, nrows in CASES:
        src = torch.arange(out * inn, dtype=torch.float32).view(out, inn)
        pad = torch.full((nrows, inn), -1.0)
        nat = to_native(src, kind, cg, nrows, pad)
        assert nat.shape == (nrows, inn) and torch.equal(to_source(nat, kind, cg, out), src)
        identity = kind == PLAIN or (kind == GEGLU and out // 2 == cg)              # one GEGLU group: value | gate is the source order
        assert identity != (not torch.equal(nat[:out], src)), _label


# ------------------------------------------------------------------------------------------------ the hooks
@pytest.mark.parametrize("rank", RANKS)
@pytest.mark.parametrize("label,kind,out,inn,cg,nrows", CASES, ids=[c[0] for c in CASES])
def test_merge_is_bit_equal_to_the_restatement_on_the_source_view(label, kind, out, inn, cg, nrows, rank):
    x = operands(kind, out, inn, cg, nrows, rank)
    src0 = to_source(x["W0"], kind, cg, out)
    for s in (0.37, 1.0):
        got = hook_merge(x["W0"], x["A"], x["B"], s, kind, cg)
        want = to_native(LR.merge(src0, x["A"], x["B"], s), kind, cg, nrows, pad=x["W0"])       # padded native rows: W0's bits
        assert same_bits(got, want), (label, rank, s)
        assert not same_bits(got[:out], x["W0"][:out])
    assert same_bits(hook_merge(x["W0"], x["A"], x["B"], 0.0, kind, cg), x["W0"])
    assert same_bits(hook_merge(x["W0"], x["A"], torch.zeros_like(x["B"]), 0.37, kind, cg), x["W0"])


@pytest.mark.parametrize("rank", RANKS)
@pytest.mark.parametrize("label,kind,out,inn,cg,nrows", CASES, ids=[c[0] for c in CASES])
def test_project_is_within_the_a_priori_bound_overwrites_and_repeats(label, kind, out, inn, cg, nrows, rank):
    x = operands(kind, out, inn, cg, nrows, rank, seed=1)
    s = 0.37
    src = to_source(x["dW"], kind, cg, out)
    x["dW"][out:] = float("nan")                                      # native rows with no source element: never read
    dA, dB = hook_project(x["dW"], x["A"], x["B"], s, kind, cg)       # outputs pre-filled with NaN
    rA, rB = LR.project64(src, x["A"], x["B"], s)
    bA, bB = LR.project_bound(src, x["A"], x["B"], s)
    for name, got, ref, bound in (("dA", dA, rA, bA), ("dB", dB, rB, bB)):
        assert bool(torch.isfinite(got).all()), f"{name}: not overwritten everywhere, or a padded row of dW was read"
        excess = float(((got.double() - ref).abs() - bound).max())
        print(f"[lora] project {label} r{rank} {name}: max |err| / bound {float(((got.double() - ref).abs() / bound.clamp_min(1e-300)).max()):.3f}")
        assert excess <= 0.0, (name, label, rank, excess)
    dA2, dB2 = hook_project(x["dW"], x["A"], x["B"], s, kind, cg)
    assert same_bits(dA, dA2) and same_bits(dB, dB2)


def test_a_plain_target_has_the_plain_kernels_bits_under_the_kind_aware_ones():
    """the layout hooks always take the kind-aware instantiations; with kind 0 they must do the plain kernels' arithmetic in their order"""
    L = lib.load()
    for out, inn, rank in ((130, 264, 3), (256, 128, 16)):
        x = operands(PLAIN, out, inn, 0, out, rank, seed=3)
        w = torch.full_like(x["W0"], float("nan"))
        lib.check(L.sdxl_op_lora_merge(ptr(x["W0"]), ptr(x["A"]), ptr(x["B"]), ptr(w), out, inn, rank, 0.37, stream()), "lora_merge")
        assert same_bits(w, hook_merge(x["W0"], x["A"], x["B"], 0.37, PLAIN, 0))
        dA = torch.full(x["A"].shape, float("nan"), dtype=torch.float32, device=DEV)
        dB = torch.full(x["B"].shape, float("nan"), dtype=torch.float32, device=DEV)
        lib.check(L.sdxl_op_lora_project(ptr(x["dW"]), ptr(x["A"]), ptr(x["B"]), ptr(dA), ptr(dB), out, inn, rank, 0.37, stream()), "lora_project")
        gA, gB = hook_project(x["dW"], x["A"], x["B"], 0.37, PLAIN, 0)
        assert same_bits(dA, gA) and same_bits(dB, gB)


@pytest.mark.parametrize("label,kind,out,inn,cg,nrows,rank", [("conv40x24", CONV3, 40, 216, 24, 40, 3), ("conv4x8pad8", CONV3, 4, 72, 8, 8, 4),
                                                              ("geglu128g64x24", GEGLU, 256, 24, 64, 256, 16)])
def test_layout_hooks_are_operand_isolated(label, kind, out, inn, cg, nrows, rank):
    x = {k: v.cpu() for k, v in operands(kind, out, inn, cg, nrows, rank, seed=2).items()}
    L = lib.load()
    f32 = torch.float32

    def merge(a):
        lib.check(L.sdxl_op_lora_merge_layout(a.ptr("W0"), a.ptr("A"), a.ptr("B"), a.ptr("w"), out, inn, rank, 0.37, kind, cg, nrows, stream()), "lora_merge_layout")

    def project(a):
        lib.check(L.sdxl_op_lora_project_layout(a.ptr("dW"), a.ptr("A"), a.ptr("B"), a.ptr("dA"), a.ptr("dB"), out, inn, rank, 0.37, kind, cg, nrows, stream()),
                  "lora_project_layout")

    ab = [Spec("A", rank, inn, init=x["A"]), Spec("B", out, rank, init=x["B"])]
    runs = run_isolated(merge, [Spec("W0", nrows, inn, init=x["W0"])] + ab + [Spec("w", nrows, inn, role="out")], device=DEV)
    assert_isolated(runs, what=f"lora_merge_layout {label} r{rank}")
    want = to_native(LR.merge(to_source(x["W0"], kind, cg, out), x["A"], x["B"], 0.37), kind, cg, nrows, pad=x["W0"])
    assert same_bits(runs[0]["w"].cpu(), want)
    # the padded native rows of dW carry the fill pattern in the poisoned runs: they must not reach dA / dB
    poison = {"dW": slice(out, nrows)} if nrows > out else None
    runs = run_isolated(project, [Spec("dW", nrows, inn, dtype=f32, init=x["dW"])] + ab
                        + [Spec("dA", rank, inn, dtype=f32, role="out"), Spec("dB", out, rank, dtype=f32, role="out")], device=DEV, poison=poison)
    assert_isolated(runs, what=f"lora_project_layout {label} r{rank}")


# ------------------------------------------------------------------------------------------------ the handle (tiny UNet)
def tiny_native_cfg(c):
    return NU.make_config(block_out_channels=c.block_out_channels, transformer_layers=c.transformer_layers_per_block,
                          cross_attention_dim=c.cross_attention_dim, addition_time_embed_dim=c.addition_time_embed_dim, pooled_dim=c.pooled_dim)


@pytest.fixture(scope="module")
def tiny():
    cfg = U.tiny_config()
    w = U.synth_weights(cfg, seed=0)
    net = NU.NativeUNet(tiny_native_cfg(cfg))
    net.load_state_dict(w)
    torch.cuda.synchronize()
    w0 = net.weights.clone()
    yield cfg, w, net, w0
    net.close()


def randomize_B(ad, std=0.02, seed=5):
    g = torch.Generator().manual_seed(seed)
    for k in ad.targets:
        ad.B(k).copy_(bf(torch.randn(ad.B(k).shape, generator=g) * std))


def target_mask(net, ad):
    m = torch.zeros(net.param_elems, dtype=torch.bool, device=net.weights.device)
    ranges = net.param_ranges()
    for k in ad.targets:
        m[ranges[k][0]: ranges[k][0] + ranges[k][1]] = True
    return m


def kind_of(key, shape):
    """(kind, cin | G) of a state-dict tensor, as capi.hip's table reads them from the engine"""
    if len(shape) == 4 and tuple(shape[2:]) == (3, 3):
        return CONV3, int(shape[1])
    if key.endswith("ff.net.0.proj.weight"):
        return GEGLU, GEGLU_GROUP
    return PLAIN, 0


def flat2(shape):
    n = 1
    for v in shape[1:]:
        n *= int(v)
    return int(shape[0]), n


def test_batched_calls_merge_every_kind_equal_the_hook_per_target_and_touch_nothing_else(tiny):
    cfg, w, net, w0 = tiny
    shapes = net.param_shapes()
    ad = LORA.LoRAAdapters(net, rank=4, alpha=2.0, targets=ALL_KINDS_TARGETS, kinds="all")
    kinds = {kind_of(k, shapes[k])[0] for k in ad.targets}
    assert kinds == {PLAIN, CONV3, GEGLU} and "conv_out.weight" in ad.targets and any(tuple(shapes[k][2:]) == (1, 1) for k in ad.targets if len(shapes[k]) == 4)
    randomize_B(ad, std=0.5)
    ranges, mask = net.param_ranges(), target_mask(net, ad)
    sd0 = {k: v.clone() for k, v in net.state_dict().items() if k in ad.targets}
    try:
        ad.merge()
        torch.cuda.synchronize()
        assert same_bits(net.weights[~mask], w0[~mask])                # nothing outside the targets' native ranges
        sd = net.state_dict()
        for k in ad.targets:
            o, i = flat2(shapes[k])
            assert sd0[k].dtype == torch.bfloat16 and ranges[k][1] == o * i, k
            want = LR.merge(sd0[k].reshape(o, i).contiguous(), ad.A(k), ad.B(k), ad.scale)
            assert same_bits(sd[k].reshape(o, i).contiguous(), want), k
            assert not same_bits(want, sd0[k].reshape(o, i).contiguous()), k          # took effect
        ad.restore()
        torch.cuda.synchronize()
        assert same_bits(net.weights, w0)
        # project: the arenas are read only; every target's dA / dB has the single-target hook's bits; the padding is not written
        net.grads.copy_(torch.randn(net.param_elems, generator=torch.Generator().manual_seed(3)))
        g0 = net.grads.clone()
        ad.grads.fill_(float("nan"))
        ad.project()
        torch.cuda.synchronize()
        assert same_bits(net.grads, g0) and same_bits(net.weights, w0)
        written = torch.zeros(ad.param_elems, dtype=torch.bool, device=ad.grads.device)
        for k in ad.targets:
            off, n = ranges[k]
            o, i = flat2(shapes[k])
            kind, cg = kind_of(k, shapes[k])
            dA, dB = hook_project(g0[off: off + n].view(o, i), ad.A(k), ad.B(k), ad.scale, kind, cg)
            assert same_bits(ad.A(k, grad=True), dA) and same_bits(ad.B(k, grad=True), dB), k
            a, b = ad.layout[k][:2]
            written[a: a + ad.rank * i] = True
            written[b: b + o * ad.rank] = True
        assert bool(torch.isnan(ad.grads[~written]).all()) and bool(torch.isfinite(ad.grads[written]).all())
    finally:
        net.weights.copy_(w0)
        net.grads.zero_()
        torch.cuda.synchronize()


def test_argument_errors_under_the_layouts_dtype(tiny):
    cfg, w, net, w0 = tiny
    L = lib.load()
    names = list(net.param_shapes())
    idx = lambda k: names.index(k)
    big = torch.zeros(1 << 22, dtype=torch.bfloat16, device=DEV)
    gbig = torch.zeros(1 << 22, dtype=torch.float32, device=DEV)

    def op(params, rank=4):
        arr = (C.c_int * len(params))(*params)
        return lib.LoraOp(len(params), arr, rank, 1.0, big.data_ptr(), big.data_ptr(), gbig.data_ptr()), arr

    c1 = "down_blocks.0.resnets.0.conv1.weight"
    cases = [([idx(c1)], 0, b"rank"), ([idx(c1)], 129, b"rank"), ([idx("conv_in.weight")], 4, b"conv_in.weight"),
             ([idx(c1), idx("conv_in.weight")], 4, b"conv_in.weight"), ([idx("conv_out.bias")], 4, b"conv_out.bias"),
             ([idx("down_blocks.0.resnets.0.norm1.weight")], 4, b"norm1.weight"), ([idx(c1), idx(c1)], 4, b"twice"),
             ([len(names)], 4, b"out of range"), ([-1], 4, b"out of range")]
    for params, rank, msg in cases:
        o, _keep = op(params, rank)
        for fn in (L.sdxl_load_weight, L.sdxl_export_grad):
            assert fn(net.h, None, C.byref(o), lib.DTYPE_LORA_LAYOUTS, stream()) == 1 and msg in L.sdxl_last_error(), (params, rank, L.sdxl_last_error())
    o, _keep = op([idx(c1)])
    assert L.sdxl_load_weight(net.h, b"conv_in.weight", C.byref(o), lib.DTYPE_LORA_LAYOUTS, stream()) == 1 and b"NULL" in L.sdxl_last_error()
    assert L.sdxl_export_grad(net.h, c1.encode(), C.byref(o), lib.DTYPE_LORA_LAYOUTS, stream()) == 1 and b"NULL" in L.sdxl_last_error()
    # the plain dtype keeps refusing the same index, and the backward's own adapter gradients keep the plain rule
    assert L.sdxl_load_weight(net.h, None, C.byref(o), lib.DTYPE_LORA, stream()) == 1 and b"conv1.weight" in L.sdxl_last_error()
    with pytest.raises(lib.SdxlError, match="conv1.weight"):
        net.set_trainable([], lora=o)
    torch.cuda.synchronize()
    assert same_bits(net.weights, w0) and float(big.abs().sum()) == 0.0 and float(gbig.abs().sum()) == 0.0


def test_the_cached_table_is_keyed_by_the_dtype(tiny):
    """the same (target list, rank) under SDXL_DTYPE_LORA and then SDXL_DTYPE_LORA_LAYOUTS, and back: each call has its own dtype's bits"""
    cfg, w, net, w0 = tiny
    plain = LORA.LoRAAdapters(net, rank=4, alpha=2.0, seed=2)
    allk = LORA.LoRAAdapters(net, rank=4, alpha=2.0, seed=2, kinds="all")
    assert plain.targets == allk.targets and plain.dtype != allk.dtype
    randomize_B(plain, std=0.5)
    allk.weights.copy_(plain.weights)
    try:
        plain.merge()
        torch.cuda.synchronize()
        first = net.weights.clone()
        net.weights.copy_(w0)
        allk.merge()
        torch.cuda.synchronize()
        assert same_bits(net.weights, first) and not same_bits(first, w0)
        net.weights.copy_(w0)
        plain.merge()
        torch.cuda.synchronize()
        assert same_bits(net.weights, first)
    finally:
        net.weights.copy_(w0)
        torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ the oracle (tiny UNet, 16 x 16, B = 2)
def make_batch(cfg, seed, B=2, H=16, W=16):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)
    return {"vae_latents": r(B, 4, H, W), "prompt_embeds": bf(r(B, 77, cfg.cross_attention_dim)).float(),
            "pooled_prompt_embeds": bf(r(B, cfg.pooled_dim)).float(), "time_ids": torch.tensor([[8.0 * H, 8.0 * W, 0, 0, 8.0 * H, 8.0 * W]] * B),
            "metadata": {}}


def step_args(method, seed, B=2, H=16, W=16):
    g = torch.Generator().manual_seed(seed)
    noise = torch.randn(B, 4, H, W, generator=g)
    ts = torch.tensor([650, 300][:B]) if method == "ddpm" else torch.tensor([0.35, 0.8][:B])
    return dict(timesteps=ts, noise=noise)


def native_micro(net, method, x, kw):
    if method == "ddpm":
        sig = R.karras_sigmas()[kw["timesteps"]]
        net.forward_loss("ddpm", x["vae_latents"], kw["noise"], sig, kw["timesteps"].float(), x["prompt_embeds"], x["pooled_prompt_embeds"], x["time_ids"])
    else:
        t = kw["timesteps"]
        net.forward_loss("flow_matching", x["vae_latents"], kw["noise"], t, t, x["prompt_embeds"], x["pooled_prompt_embeds"], x["time_ids"])
    net.zero_grads()
    net.backward(1.0, True)


@pytest.mark.parametrize("method", ["ddpm", "flow_matching"])
def test_adapter_gradients_of_every_kind_match_the_oracle_at_the_merged_weights(tiny, method):
    """native dA / dB of every kind of target against the float64 projection of the oracle's autograd dW reshaped [out, in], the oracle
    evaluated at the bf16-rounded MERGED weights; rank 4, B std 0.02, the bar of tests/test_gpu_model.py.  Beside it (printed, and the
    first thing to read when a tensor misses): the float64 projection of the EXPORTED native dW against the same reference, which holds
    the weight gradient's own error and none of the projection kernels'.  Then the same step under project_frozen: bit-equal."""
    cfg, w, net, w0 = tiny
    rank = 4
    shapes = net.param_shapes()
    ad = LORA.LoRAAdapters(net, rank=rank, alpha=rank / 2, targets=ALL_KINDS_TARGETS, seed=1, kinds="all")
    randomize_B(ad, std=0.02)
    x, kw = make_batch(cfg, 31), step_args(method, 32)
    try:
        ad.merge()
        native_micro(net, method, x, kw)
        ad.grads.fill_(float("nan"))
        ad.project()
        torch.cuda.synchronize()
        loss = net.read_loss()[0]
        got = ad.grads.clone()
        exported = {k: net.export(k, grad=True).double().cpu() for k in ad.targets}
        wm = {k: v.float().cpu() for k, v in net.state_dict().items()}           # bf16-rounded merged weights, as the step read them
        assert any(not torch.equal(wm[k], w[k]) for k in ad.targets)
        leaves = {k: wm[k].requires_grad_(True) for k in ad.targets}
        unet_fn = lambda s, t, e, p, ti: U.unet_forward(wm, s, t, e, p, ti, cfg)
        ob = {k: x[k] for k in ("vae_latents", "prompt_embeds", "pooled_prompt_embeds", "time_ids")}
        ref = R.compute_loss_ddpm(unet_fn, ob, kw["noise"], kw["timesteps"]) if method == "ddpm" else R.compute_loss_flow(unet_fn, ob, kw["noise"], kw["timesteps"])
        ref["loss"].backward()
        par, inherited = GradParity(f"lora layouts {method} r{rank}"), GradParity(f"lora layouts {method} r{rank}: float64 projection of the exported dW")
        for k in ad.targets:
            o, i = flat2(shapes[k])
            A, B = ad.A(k).cpu(), ad.B(k).cpu()
            dA, dB = LR.project64(leaves[k].grad.reshape(o, i), A, B, ad.scale)
            eA, eB = LR.project64(exported[k].reshape(o, i), A, B, ad.scale)
            mod = k[: -len(".weight")]
            par.add(f"{mod}.lora_A.weight", ad.A(k, grad=True).cpu(), dA)
            par.add(f"{mod}.lora_B.weight", ad.B(k, grad=True).cpu(), dB)
            inherited.add(f"{mod}.lora_A.weight", eA, dA)
            inherited.add(f"{mod}.lora_B.weight", eB, dB)
        inherited.report(lambda _k: GRAD_BAR, printer=lambda s: print("[parity] " + s))
        par.check(GRAD_BAR, expect=ad.param_ranges(), printer=lambda s: print("[parity] " + s))
        # project_frozen: only the ops that hold a target form their weight gradient; the same adapter gradients and loss, bit for bit
        ad.select("project_frozen")
        native_micro(net, method, x, kw)
        ad.grads.fill_(float("nan"))
        ad.project()
        torch.cuda.synchronize()
        assert net.read_loss()[0] == loss and same_bits(ad.grads, got)
    finally:
        net.set_trainable(None)
        net.weights.copy_(w0)
        net.grads.zero_()
        torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ the trainer
TRAINER_TARGETS = ["ff.net.0.proj", "conv1", "conv_shortcut", "to_q"]


def make_trainer(net, method="ddpm", **training):
    cfg = CFG.Config()
    cfg.training.method = method
    cfg.optimizer.learning_rate = 1e-3
    for k, v in training.items():
        setattr(cfg.training, k, v)
    return T.create_trainer(SimpleNamespace(unet=net), config=cfg)


def run_training(net, method, steps, accum=2, save_at=None, save_dir=None, resume_from=None, first_step=0, **training):
    """`steps` optimizer steps of `accum` micro-steps on seeded batches; returns (trainer, [losses])"""
    cfg = U.tiny_config()
    training.setdefault("lora_targets", TRAINER_TARGETS)
    tr = make_trainer(net, method, lora_rank=4, lora_alpha=8.0, lora_target_kinds="all", gradient_accumulation_steps=accum, **training)
    if resume_from is not None:
        tr.load_lora_state(resume_from)
    losses = []
    for s in range(first_step, first_step + steps):
        for m in range(accum):
            loss, _m = tr._execute_training_step(make_batch(cfg, 100 + 10 * s + m), accumulate=True, is_last_accumulation_step=m == accum - 1,
                                                 **step_args(method, 200 + 10 * s + m))
            losses.append(float(loss))
        tr.optimizer_step()
        if save_at is not None and s == save_at:
            tr.save_checkpoint(save_dir)
    torch.cuda.synchronize()
    return tr, losses


def test_training_moves_only_the_targets_and_repeats_bit_for_bit(tiny):
    cfg, w, net, w0 = tiny
    shapes = net.param_shapes()
    sd0 = {k: v.clone() for k, v in net.state_dict().items()}
    try:
        tr, losses = run_training(net, "ddpm", 3)
        ad = tr.lora
        assert ad.kinds == "all" and {kind_of(k, shapes[k])[0] for k in ad.targets} == {PLAIN, CONV3, GEGLU}
        assert any(tuple(shapes[k][2:]) == (1, 1) for k in ad.targets if len(shapes[k]) == 4)
        mask, ranges = target_mask(net, ad), net.param_ranges()
        assert same_bits(net.weights[~mask], w0[~mask])
        moved = 0
        for k in ad.targets:
            off, n = ranges[k]
            o, i = flat2(shapes[k])
            kind, cg = kind_of(k, shapes[k])
            want = to_native(LR.merge(sd0[k].reshape(o, i).contiguous(), ad.A(k), ad.B(k), ad.scale), kind, cg, o)
            assert same_bits(net.weights[off: off + n], want.reshape(-1)), k
            moved += int(not same_bits(net.weights[off: off + n], w0[off: off + n]))
        assert moved == len(ad.targets) and float(ad.weights.float().abs().max()) > 0
        first = (net.weights.clone(), net.grads.clone(), ad.weights.clone(), ad.grads.clone(), losses)
        ad.restore()
        torch.cuda.synchronize()
        assert same_bits(net.weights, w0)
        tr2, losses2 = run_training(net, "ddpm", 3)
        for a, b in zip(first[:4], (net.weights, net.grads, tr2.lora.weights, tr2.lora.grads)):
            assert same_bits(a, b)
        assert losses2 == first[4]
    finally:
        net.weights.copy_(w0)
        torch.cuda.synchronize()


def test_twenty_steps_on_convolution_and_geglu_targets_lower_the_loss(tiny):
    cfg, w, net, w0 = tiny
    try:
        tr = make_trainer(net, "ddpm", lora_rank=4, lora_target_kinds="all", lora_targets=["ff.net.0.proj", "conv1", "conv2", "conv_shortcut"])
        assert all(kind_of(k, net.param_shapes()[k])[0] != PLAIN or len(net.param_shapes()[k]) == 4 for k in tr.lora.targets)
        batch = make_batch(cfg, 41)
        noise = torch.randn(batch["vae_latents"].shape, generator=torch.Generator().manual_seed(42))       # evaluate() draws the same
        ts = torch.full((2,), 500, dtype=torch.long)
        evaluate = lambda: tr.evaluate([batch], [500], generator=torch.Generator().manual_seed(42))[1]
        before = evaluate()
        for _ in range(20):
            tr._execute_training_step(batch, timesteps=ts, noise=noise)
            tr.optimizer_step()
        after = evaluate()
        print(f"[lora] layouts ddpm: evaluation loss {before:.6f} -> {after:.6f} after 20 steps")
        assert after < before
    finally:
        net.weights.copy_(w0)
        torch.cuda.synchronize()


def test_checkpoint_round_trip_and_exported_delta(tiny, tmp_path):
    from safetensors.torch import load_file
    cfg, w, net, w0 = tiny
    shapes = net.param_shapes()
    try:
        tr, _l = run_training(net, "ddpm", 3, save_at=1, save_dir=tmp_path / "ck")
        want = (net.weights.clone(), tr.lora.weights.clone(), tr.optimizer.exp_avg.clone(), tr.optimizer.exp_avg_sq.clone())
        net.weights.copy_(w0)                                      # a fresh process would load the checkpoint's UNet
        tr2, _l = run_training(net, "ddpm", 1, resume_from=tmp_path / "ck", first_step=2)
        got = (net.weights, tr2.lora.weights, tr2.optimizer.exp_avg, tr2.optimizer.exp_avg_sq)
        for a, b in zip(want, got):
            assert same_bits(a, b)
        ex = load_file(str(tmp_path / "ck" / "pytorch_lora_weights.safetensors"))
        st = torch.load(str(tmp_path / "ck" / "lora_state.pt"), weights_only=True)
        assert len(ex) == 2 * len(tr.lora.targets) and st["rank"] == 4 and st["targets"] == tr.lora.targets and st["kinds"] == "all"
        s = st["alpha"] / st["rank"]
        four_d = 0
        for k in tr.lora.targets:
            a, b, o, i = tr.lora.layout[k]
            A, B = st["weights"][a: a + 4 * i].view(4, i).double(), st["weights"][b: b + o * 4].view(o, 4).double()
            mod = k[: -len(".weight")]
            lA, lB = ex[f"unet.{mod}.lora_A.weight"], ex[f"unet.{mod}.lora_B.weight"]
            if len(shapes[k]) == 4:
                four_d += 1
                assert lA.shape == (4, *shapes[k][1:]) and lB.shape == (o, 4, 1, 1), k
            else:
                assert lA.shape == (4, i) and lB.shape == (o, 4), k
            delta = (lB.double().reshape(o, 4) @ lA.double().reshape(4, i)).reshape(shapes[k])      # the layer-shaped kernel of up(1x1) o down
            err = (delta - (s * (B @ A)).reshape(shapes[k])).abs()
            assert float((err - 2.0 ** -23 * (s * B.abs() @ A.abs()).reshape(shapes[k])).max()) <= 0.0 and float((B @ A).abs().max()) > 0, k
        assert four_d > 0
        other = make_trainer(net, "ddpm", lora_rank=4, lora_targets=["to_q"])        # a plain trainer refuses the state
        before = other.lora.weights.clone()
        with pytest.raises(ValueError):
            other.load_lora_state(tmp_path / "ck")
        assert same_bits(other.lora.weights, before)
    finally:
        net.weights.copy_(w0)
        torch.cuda.synchronize()
