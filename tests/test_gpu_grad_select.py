"""Frozen-aware backward on a real MI355X: the direct adapter-gradient kernels of csrc/lora_grad.hip through their single-target hook
(a-priori bound against float64, exact small integers, accumulate / overwrite, reproducible bits, operand isolation), the engine's
gradient selection on the tiny UNet (a frozen op writes nothing, the selected gradients are the all-trainable ones, the conditioning
gradients keep their bits, accumulation, captured graphs) and the LoRA trainer's `lora_backward` modes against the oracle."""
import ctypes as C
import importlib
import os
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
from _isolation import Spec, assert_isolated, bits, fill_bytes, run_isolated, same_bits

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
CFG = importlib.import_module("sdxl-training-improvements_amd.config")
T = importlib.import_module("sdxl-training-improvements_amd.trainer")
LORA = importlib.import_module("sdxl-training-improvements_amd.lora")

GRAD_BAR = (6e-2, 0.995)          # TINY_GRAD_BAR of tests/test_gpu_model.py
REORDER_CAP = 1e-4                # linear weight gradients whose grouped launch changed composition: K 2^-24 = 3e-5 of sum |terms| at K = 512 rows, x 3 for cancellation
OP_SHAPES = [(154, 128, 128, 4), (512, 64, 64, 16), (2, 64, 288, 4), (300, 40, 72, 3), (1024, 256, 128, 128)]      # (M, out, in, rank)
DEV = "cuda"

bf = lambda t: t.to(torch.bfloat16)
ptr = lambda t: C.c_void_p(t.data_ptr())
stream = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)


# ------------------------------------------------------------------------------------------------ 1. the hook
def op_operands(M, out, inn, rank, seed=0):
    g = torch.Generator().manual_seed(1000 * seed + 13 * M + 7 * out + inn + rank)
    r = lambda *s: bf(torch.randn(*s, generator=g))
    return dict(X=r(M, inn), dY=r(M, out), A=r(rank, inn), B=r(out, rank))


def hook_grad(X, dY, A, B, s, accumulate=0, dA=None, dB=None, M=None, out=None, inn=None):
    """sdxl_op_lora_grad on device tensors; X / dY may be column slices of wider tensors (their row stride is passed)"""
    M = X.shape[0] if M is None else M
    out = dY.shape[1] if out is None else out
    inn = X.shape[1] if inn is None else inn
    rank = A.shape[0]
    if dA is None:
        dA = torch.full((rank, inn), float("nan"), dtype=torch.float32, device=X.device)
        dB = torch.full((out, rank), float("nan"), dtype=torch.float32, device=X.device)
    lib.check(lib.load().sdxl_op_lora_grad(ptr(X), X.stride(0), ptr(dY), dY.stride(0), ptr(A), ptr(B), ptr(dA), ptr(dB), M, out, inn, rank, s,
                                           accumulate, stream()), "lora_grad")
    torch.cuda.synchronize()
    return dA, dB


def ref64(X, dY, A, B, s):
    """(dA, dB, bound dA, bound dB) in float64 on the same bf16 operands: one bf16 rounding of the intermediate with a factor 2 of slack
    (2^-8 relative) + the fp32 accumulation over M rows (M 2^-23)"""
    X, dY, A, B = (t.double().cpu() for t in (X, dY, A, B))
    M = X.shape[0]
    That, Uhat = X @ A.T, dY @ B
    dB, dA = s * dY.T @ That, s * Uhat.T @ X
    e = 2.0 ** -8 + M * 2.0 ** -23
    return dA, dB, abs(s) * e * (Uhat.abs().T @ X.abs()), abs(s) * e * (dY.abs().T @ That.abs())


def check_bound(tag, dA, dB, ref):
    rA, rB, bA, bB = ref
    for name, got, want, bound in (("dA", dA, rA, bA), ("dB", dB, rB, bB)):
        assert bool(torch.isfinite(got).all()), f"{tag} {name}: not written everywhere"
        err = (got.double().cpu() - want).abs()
        print(f"[lora_grad] {tag} {name}: max |err| / bound {float((err / bound.clamp_min(1e-300)).max()):.3f}")
        assert float((err - bound).max()) <= 0.0, (tag, name)


@pytest.mark.parametrize("M,out,inn,rank", OP_SHAPES, ids=[f"{m}x{o}x{i}r{r}" for m, o, i, r in OP_SHAPES])
def test_hook_is_within_the_a_priori_bound_overwrites_accumulates_and_repeats(M, out, inn, rank):
    x = {k: v.to(DEV) for k, v in op_operands(M, out, inn, rank).items()}
    s = 0.37
    dA, dB = hook_grad(x["X"], x["dY"], x["A"], x["B"], s)          # outputs pre-filled with NaN: accumulate = 0 overwrites
    ref = ref64(x["X"], x["dY"], x["A"], x["B"], s)
    check_bound(f"{M}x{out}x{inn} r{rank}", dA, dB, ref)
    dA2, dB2 = hook_grad(x["X"], x["dY"], x["A"], x["B"], s)
    assert same_bits(dA, dA2) and same_bits(dB, dB2)
    # accumulate = 1 adds onto what is there: one fp32 addition of the same increment
    pA, pB = torch.randn_like(dA), torch.randn_like(dB)
    aA, aB = hook_grad(x["X"], x["dY"], x["A"], x["B"], s, accumulate=1, dA=pA.clone(), dB=pB.clone())
    assert same_bits(aA, pA + dA) and same_bits(aB, pB + dB)
    # once more as column slices: dy = columns [out, 2 out) of a [M][3 out] tensor, x with a row stride > in
    wideY = bf(torch.randn(M, 3 * out, generator=torch.Generator().manual_seed(5))).to(DEV)
    wideY[:, out: 2 * out] = x["dY"]
    wideX = bf(torch.randn(M, inn + 8, generator=torch.Generator().manual_seed(6))).to(DEV)
    wideX[:, :inn] = x["X"]
    sA, sB = hook_grad(wideX[:, :inn], wideY[:, out: 2 * out], x["A"], x["B"], s)
    check_bound(f"{M}x{out}x{inn} r{rank} sliced", sA, sB, ref)
    if out % 8 == 0:      # (the slice starts on a 16-byte boundary: the same loads, the same bits)
        assert same_bits(sA, dA) and same_bits(sB, dB)


@pytest.mark.parametrize("M,out,inn,rank", OP_SHAPES, ids=[f"{m}x{o}x{i}r{r}" for m, o, i, r in OP_SHAPES])
def test_hook_is_exact_on_small_integers(M, out, inn, rank):
    """operands in {-1, 0, 1}, at most 8 non-zeros per row of A and per column of B: |T|, |U| <= 8 are exact in bf16, every sum in fp32"""
    g = torch.Generator().manual_seed(M + out + inn + rank)
    ints = lambda *s: torch.randint(-1, 2, s, generator=g).float()
    X, dY = ints(M, inn), ints(M, out)
    A, B = torch.zeros(rank, inn), torch.zeros(out, rank)
    for c in range(rank):
        A[c, torch.randperm(inn, generator=g)[:8]] = 1.0
        B[torch.randperm(out, generator=g)[:8], c] = -1.0
    dA, dB = hook_grad(bf(X).to(DEV), bf(dY).to(DEV), bf(A).to(DEV), bf(B).to(DEV), 0.5)
    assert torch.equal(dA.cpu().double(), 0.5 * (dY.double() @ B.double()).T @ X.double())
    assert torch.equal(dB.cpu().double(), 0.5 * dY.double().T @ (X.double() @ A.double().T))


# ------------------------------------------------------------------------------------------------ 2. isolation
@pytest.mark.parametrize("M,out,inn,rank,ldx_extra", [(154, 128, 128, 4, 8), (300, 40, 72, 3, 3), (70, 24, 40, 16, 0)])
def test_hook_is_operand_isolated(M, out, inn, rank, ldx_extra):
    """guard bands, pattern-filled outputs, poisoned rows past M (8 more rows are allocated and filled with the pattern), dy a column
    slice of a [M][3 out] tensor whose other columns hold the pattern, x with a row gap (ldx_extra = 3: rows that are not 16-byte aligned).
    The slice is handed over at column offset `out` of the wide tensor (the pointer is out elements into the row, 2 out pattern columns
    follow it and `out` precede it: in memory the columns in front of row r's slice are the tail of row r - 1's gap, and the guard band
    in front of row 0), so both sides of the slice are pattern."""
    x = op_operands(M, out, inn, rank, seed=3)
    L = lib.load()
    f32 = torch.float32
    pad = lambda t: torch.cat([t, torch.zeros(8, t.shape[1], dtype=t.dtype)])

    def run(a):
        lib.check(L.sdxl_op_lora_grad(a.ptr("x"), a.ld("x"), a.ptr("dy"), a.ld("dy"), a.ptr("A"), a.ptr("B"), a.ptr("dA"), a.ptr("dB"), M, out, inn,
                                      rank, 0.37, 0, stream()), "lora_grad")

    specs = [Spec("x", M + 8, inn, ld=inn + ldx_extra, init=pad(x["X"])), Spec("dy", M + 8, out, ld=3 * out, init=pad(x["dY"])),
             Spec("A", rank, inn, init=x["A"]), Spec("B", out, rank, init=x["B"]),
             Spec("dA", rank, inn, dtype=f32, role="out"), Spec("dB", out, rank, dtype=f32, role="out")]
    runs = run_isolated(run, specs, device=DEV, poison={"x": slice(M, None), "dy": slice(M, None)})
    assert_isolated(runs, what=f"lora_grad {M}x{out}x{inn} r{rank}")
    check_bound(f"isolated {M}x{out}x{inn} r{rank}", runs[0]["dA"], runs[0]["dB"], ref64(x["X"], x["dY"], x["A"], x["B"], 0.37))


def test_hook_argument_errors():
    L = lib.load()
    big = torch.zeros(1 << 16, dtype=torch.bfloat16, device=DEV)
    g = torch.zeros(1 << 16, dtype=torch.float32, device=DEV)
    for M, out, inn, rank in ((8, 8, 8, 0), (8, 8, 8, 129), (8, 8, 12, 4), (0, 8, 8, 4)):
        assert L.sdxl_op_lora_grad(ptr(big), inn, ptr(big), out, ptr(big), ptr(big), ptr(g), ptr(g), M, out, inn, rank, 1.0, 0, stream()) == 1
    assert L.sdxl_op_lora_grad(ptr(big), 4, ptr(big), 8, ptr(big), ptr(big), ptr(g), ptr(g), 8, 8, 8, 4, 1.0, 0, stream()) == 1      # ldx < in
    torch.cuda.synchronize()
    assert float(g.abs().sum()) == 0.0


# ------------------------------------------------------------------------------------------------ the tiny UNet
def tiny_native_cfg(c):
    return NU.make_config(block_out_channels=c.block_out_channels, transformer_layers=c.transformer_layers_per_block,
                          cross_attention_dim=c.cross_attention_dim, addition_time_embed_dim=c.addition_time_embed_dim, pooled_dim=c.pooled_dim)


def make_inputs(cfg, seed, B=2, H=16, W=16):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)
    return dict(lat=r(B, 4, H, W), noise=r(B, 4, H, W), ehs=bf(r(B, 77, cfg.cross_attention_dim)).float(), pooled=bf(r(B, cfg.pooled_dim)).float(),
                tid=torch.tensor([[8.0 * H, 8.0 * W, 0, 0, 8.0 * H, 8.0 * W]] * B), ts=torch.tensor([610, 230][:B]))


def forward(net, x, **kw):
    net.forward_loss("ddpm", x["lat"], x["noise"], R.karras_sigmas()[x["ts"]], x["ts"].float(), x["ehs"], x["pooled"], x["tid"], **kw)


def step(net, x, scale=1.0, first=True, zero=True, **kw):
    forward(net, x, **kw)
    if zero:
        net.zero_grads()
    net.backward(scale, first)
    torch.cuda.synchronize()


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


@pytest.fixture(autouse=True)
def _selection_off(request):
    """every test leaves the shared net with no selection, its checkpoint weights and a clean arena"""
    yield
    if "tiny" in request.fixturenames:
        cfg, _w, net, w0 = request.getfixturevalue("tiny")
        net.set_graph_mode(False)
        net.discard_forward()               # (a test may end on a forward that nothing differentiates: the selection cannot change under it)
        net.set_trainable(None)
        net.weights.copy_(w0)
        net.grads.zero_()
        torch.cuda.synchronize()


def attention_projections(k):
    mod = k.rsplit(".", 1)[0]
    return (".attn1." in k or ".attn2." in k) and mod.endswith(("to_q", "to_k", "to_v", "to_out.0"))


def mixed(k):      # a convolution, a GroupNorm, a LayerNorm, the grouped time projection, one feed-forward output, one block's q | k | v through to_k alone
    return k.startswith(("down_blocks.1.resnets.0.conv1.", "up_blocks.0.resnets.1.norm2.", "mid_block.attentions.0.transformer_blocks.0.norm2.",
                         "up_blocks.1.upsamplers.0.conv.", "down_blocks.1.downsamplers.0.conv.", "conv_in.")) or k in (
        "down_blocks.0.resnets.0.time_emb_proj.weight", "down_blocks.2.attentions.0.transformer_blocks.0.ff.net.2.weight",
        "mid_block.attentions.0.transformer_blocks.0.attn1.to_k.weight", "mid_block.attentions.0.proj_in.bias")


def live_ops(net, pred):
    shapes = net.param_shapes()
    return {LORA.op_of(k, shapes[k]) for k in shapes if pred(k)}


def check_frozen_untouched(net, pred, fill, what):
    """every tensor of a fully frozen op keeps the fill (a matrix) or holds sdxl_zero_grads's zeros (a bias / norm vector); every tensor
    of an op with a trainable tensor is finite"""
    shapes, ranges, live = net.param_shapes(), net.param_ranges(), live_ops(net, pred)
    raw = net.grads.view(torch.uint8).view(-1, 4)
    n_frozen = 0
    for k, (off, n) in ranges.items():
        g = net.grads[off: off + n]
        if LORA.op_of(k, shapes[k]) in live:
            assert bool(torch.isfinite(g).all()), f"{what}: {k} (trainable op) is not finite"
        elif len(shapes[k]) == 1:
            assert bool((bits(g) == 0).all()), f"{what}: {k} (frozen vector) does not hold the zeros of zero_grads"
            n_frozen += 1
        else:
            assert bool((raw[off: off + n] == fill).all()), f"{what}: {k} (frozen op) was written"
            n_frozen += 1
    assert n_frozen > 0


# ------------------------------------------------------------------------------------------------ 3. a frozen op writes nothing
@pytest.mark.parametrize("sel", [attention_projections, mixed], ids=["attention", "mixed"])
def test_selection_leaves_frozen_gradients_alone(tiny, sel):
    cfg, w, net, w0 = tiny
    x = make_inputs(cfg, 13)
    net.plan(2, 16, 16, 77)
    net.set_trainable(sel)
    assert net.trainable() == {k for k in net.param_shapes() if sel(k)}
    fill_bytes(net.grads, 0xFF)
    step(net, x)
    check_frozen_untouched(net, sel, 0xFF, sel.__name__)


def test_a_frozen_op_writes_nothing_into_the_emit_arena(tiny):
    """sdxl_set_grad_emit: the weight gradients that run write bf16 into the emit arena; a frozen op leaves its range of it alone"""
    cfg, w, net, w0 = tiny
    x = make_inputs(cfg, 13)
    net.plan(2, 16, 16, 77)
    net.set_trainable(attention_projections)
    arena = torch.zeros(net.param_elems, dtype=torch.bfloat16, device=DEV)
    fill_bytes(arena, 0xFF)
    fill_bytes(net.grads, 0xFF)
    forward(net, x)
    net.zero_grads()
    net.set_grad_emit(arena, 1.0)
    try:
        net.backward(1.0, True)
        torch.cuda.synchronize()
    finally:
        net.set_grad_emit(None)
    shapes, live = net.param_shapes(), live_ops(net, attention_projections)
    raw = arena.view(torch.uint8).view(-1, 2)
    n_frozen = n_live = 0
    for k, (off, n) in net.param_ranges().items():
        if len(shapes[k]) == 1:
            continue                                   # (vectors are not emitted: sdxl_small_grads_to_bf16 casts them)
        if LORA.op_of(k, shapes[k]) in live:
            assert bool(torch.isfinite(arena[off: off + n].float()).all()), f"{k}: not emitted"
            n_live += 1
        else:
            assert bool((raw[off: off + n] == 0xFF).all()), f"{k} (frozen op): the emit arena was written"
            n_frozen += 1
    assert n_frozen > 0 and n_live > 0


# ------------------------------------------------------------------------------------------------ 4. the selected gradients are the right ones
def compare_selected(net, pred, g_all, what):
    """trainable ops: convolutions and norms bit-equal to the all-trainable run (their launches are per op); linear weights and biases may
    differ by the fp32 summation order of a grouped launch whose composition changed: per tensor |d|_2 <= REORDER_CAP |g_all|_2"""
    shapes, ranges, live = net.param_shapes(), net.param_ranges(), live_ops(net, pred)
    moved = []
    for k, (off, n) in ranges.items():
        if LORA.op_of(k, shapes[k]) not in live:
            continue
        a, b = net.grads[off: off + n], g_all[off: off + n]
        if same_bits(a, b):
            continue
        linear = len(shapes[k]) == 2 or (k.endswith(".bias") and len(shapes.get(k[:-5] + ".weight", ())) == 2)
        rel = float((a.double() - b.double()).norm() / b.double().norm())
        moved.append((k, rel))
        assert linear, f"{what}: {k} (per-op launch) differs from the all-trainable run (rel {rel:.3e})"
        assert rel <= REORDER_CAP, f"{what}: {k} differs from the all-trainable run by {rel:.3e} > {REORDER_CAP}"
    print(f"[grad_select] {what}: {len(moved)} trainable tensors not bit-equal to the all-trainable run: {[(k, f'{r:.2e}') for k, r in moved]}")


@pytest.fixture(scope="module")
def oracle(tiny):
    """the oracle's autograd gradients of the step every model-level test here runs (inputs seed 13), computed once"""
    cfg, w, net, w0 = tiny
    x = make_inputs(cfg, 13)
    leaves = {k: v.clone().requires_grad_(True) for k, v in w.items()}
    unet_fn = lambda s, t, e, p, ti: U.unet_forward(leaves, s, t, e, p, ti, cfg)
    batch = {"vae_latents": x["lat"], "prompt_embeds": x["ehs"], "pooled_prompt_embeds": x["pooled"], "time_ids": x["tid"]}
    R.compute_loss_ddpm(unet_fn, batch, x["noise"], x["ts"])["loss"].backward()
    return {k: (v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in leaves.items()}


def test_selected_gradients_equal_the_all_trainable_ones_and_the_oracle(tiny, oracle):
    cfg, w, net, w0 = tiny
    x = make_inputs(cfg, 13)
    step(net, x)
    g_all = net.grads.clone()
    par = GradParity("all trainable")
    for k in net.param_shapes():
        par.add(k, net.export(k, grad=True).cpu(), oracle[k])
    par.check(GRAD_BAR, expect=net.param_shapes(), printer=lambda s: None)
    for sel in (attention_projections, mixed):
        net.set_trainable(sel)
        net.grads.zero_()
        step(net, x)
        compare_selected(net, sel, g_all, sel.__name__)
        shapes, live = net.param_shapes(), live_ops(net, sel)
        keys = [k for k in shapes if LORA.op_of(k, shapes[k]) in live]
        par = GradParity(f"selection {sel.__name__}")
        for k in keys:
            par.add(k, net.export(k, grad=True).cpu(), oracle[k])
        par.check(GRAD_BAR, expect=keys, printer=lambda s: print("[parity] " + s))


# ------------------------------------------------------------------------------------------------ 5. everything frozen + conditioning gradients
def test_all_frozen_keeps_the_conditioning_gradients_bits_and_the_arena(tiny):
    cfg, w, net, w0 = tiny
    x = make_inputs(cfg, 13)
    step(net, x, cond_grads=True)
    want = [t.clone() for t in net.read_cond_grads()]
    loss = net.read_loss()
    net.set_trainable([])
    assert net.trainable() == set()
    fill_bytes(net.grads, 0xFF)
    step(net, x, cond_grads=True)
    got = net.read_cond_grads()
    assert net.read_loss() == loss
    assert same_bits(got[0], want[0]) and same_bits(got[1], want[1]) and float(want[0].abs().max()) > 0 and float(want[1].abs().max()) > 0
    check_frozen_untouched(net, lambda k: False, 0xFF, "all frozen")


# ------------------------------------------------------------------------------------------------ 6. accumulation and graphs
def test_two_micro_steps_under_a_selection(tiny):
    cfg, w, net, w0 = tiny
    xa, xb = make_inputs(cfg, 21), make_inputs(cfg, 22)

    def cycle():
        step(net, xa, 0.5, True)
        step(net, xb, 0.5, False, zero=False)

    cycle()
    g_all = net.grads.clone()
    net.set_trainable(attention_projections)
    fill_bytes(net.grads, 0xFF)
    cycle()
    check_frozen_untouched(net, attention_projections, 0xFF, "two micro-steps")
    compare_selected(net, attention_projections, g_all, "two micro-steps")


def test_selection_change_takes_effect_under_graph_replay(tiny):
    """graph mode: the first call of a configuration runs eager, the second is captured, the third replayed.  A change of the selection
    drops the captures: the next steps follow the new selection (fill pattern), and the replayed step has the eager one's bits."""
    cfg, w, net, w0 = tiny
    x = make_inputs(cfg, 13)
    eager = {}
    for sel in (attention_projections, mixed):
        net.set_trainable(sel)
        net.grads.zero_()
        step(net, x)
        eager[sel] = net.grads.clone()
    net.set_graph_mode(True)
    for sel in (attention_projections, mixed, attention_projections):
        net.set_trainable(sel)
        for i in range(3):
            fill_bytes(net.grads, 0xFF)
            step(net, x)
            check_frozen_untouched(net, sel, 0xFF, f"graph mode {sel.__name__} call {i}")
            shapes, live = net.param_shapes(), live_ops(net, sel)
            for k, (off, n) in net.param_ranges().items():
                if LORA.op_of(k, shapes[k]) in live:
                    assert same_bits(net.grads[off: off + n], eager[sel][off: off + n]), (sel.__name__, i, k)


def test_selection_argument_errors(tiny):
    cfg, w, net, w0 = tiny
    L = lib.load()
    n = len(net.param_shapes())
    ok = (C.c_ubyte * n)(*([1] * n))
    call = lambda name, sel: L.sdxl_export_grad(net.h, name, None if sel is None else C.byref(sel), lib.DTYPE_GRAD_SELECT, stream())
    assert call(None, lib.GradSelect(n - 1, ok, None)) == 1 and b"sdxl_num_params" in L.sdxl_last_error()
    bad = (C.c_ubyte * n)(*([1] * (n - 1) + [2]))
    assert call(None, lib.GradSelect(n, bad, None)) == 1 and b"conv_out.bias" in L.sdxl_last_error()
    assert call(b"conv_in.weight", lib.GradSelect(n, ok, None)) == 1 and b"NULL" in L.sdxl_last_error()
    with pytest.raises(KeyError):
        net.set_trainable(["no.such.weight"])
    # between a forward_loss and its backward the selection may not change; the same selection again is no change
    x = make_inputs(cfg, 13)
    forward(net, x)
    with pytest.raises(lib.SdxlError, match="between sdxl_forward_loss"):
        net.set_trainable([])
    net.set_trainable(None)
    net.zero_grads()
    net.backward(1.0, True)
    net.set_trainable([])
    # adapters: a flagged tensor in a targeted op, a convolution as target (the message of SDXL_DTYPE_LORA), an emit arena
    ad = LORA.LoRAAdapters(net, rank=4)
    with pytest.raises(lib.SdxlError, match="flag must be 0"):
        net.set_trainable(lambda k: k.endswith("attn1.to_k.weight"), lora=ad._op(1.0))
    names = list(net.param_shapes())
    arr = (C.c_int * 1)(names.index("conv_in.weight"))
    conv = lib.LoraOp(1, arr, 4, 1.0, ad.weights.data_ptr(), ad.base.data_ptr(), ad.grads.data_ptr())
    with pytest.raises(lib.SdxlError, match="conv_in.weight"):
        net.set_trainable([], lora=conv)
    arena = torch.zeros(net.param_elems, dtype=torch.bfloat16, device=DEV)
    net.set_grad_emit(arena)
    try:
        with pytest.raises(lib.SdxlError, match="emit arena"):
            net.set_trainable([], lora=ad._op(1.0))
    finally:
        net.set_grad_emit(None)
    net.set_trainable([], lora=ad._op(1.0))
    with pytest.raises(lib.SdxlError, match="emit arena"):
        net.set_grad_emit(arena)


# ------------------------------------------------------------------------------------------------ 7. the LoRA trainer's modes
def randomize_B(ad, std=0.02, seed=5):
    g = torch.Generator().manual_seed(seed)
    for k in ad.targets:
        ad.B(k).copy_(bf(torch.randn(ad.B(k).shape, generator=g) * std))


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


def make_trainer(net, method="ddpm", **training):
    cfg = CFG.Config()
    cfg.training.method = method
    cfg.optimizer.learning_rate = 1e-3
    for k, v in training.items():
        setattr(cfg.training, k, v)
    return T.create_trainer(SimpleNamespace(unet=net), config=cfg)


def native_micro(net, method, batch, kw, scale, first):
    x = batch
    if method == "ddpm":
        sig = R.karras_sigmas()[kw["timesteps"]]
        net.forward_loss("ddpm", x["vae_latents"], kw["noise"], sig, kw["timesteps"].float(), x["prompt_embeds"], x["pooled_prompt_embeds"], x["time_ids"])
    else:
        t = kw["timesteps"]
        net.forward_loss("flow_matching", x["vae_latents"], kw["noise"], t, t, x["prompt_embeds"], x["pooled_prompt_embeds"], x["time_ids"])
    if first:
        net.zero_grads()
    net.backward(scale, first)


def oracle_loss(cfg, wm, method, batch, kw):
    unet_fn = lambda s, t, e, p, ti: U.unet_forward(wm, s, t, e, p, ti, cfg)
    ob = {k: batch[k] for k in ("vae_latents", "prompt_embeds", "pooled_prompt_embeds", "time_ids")}
    fn = R.compute_loss_ddpm if method == "ddpm" else R.compute_loss_flow
    return fn(unet_fn, ob, kw["noise"], kw["timesteps"])["loss"]


def adapter_gradients_against_the_oracle(tiny, mode, method, rank, targets, micros=1):
    """the form of test_gpu_lora.py::test_adapter_gradients_match_the_oracle_at_the_merged_weights under a lora_backward mode: native dA / dB
    against the float64 projection of the oracle's autograd dW at the bf16-rounded merged weights, the same bar; `micros` micro-steps of
    scale 1 / micros against the oracle's summed gradient"""
    cfg, w, net, w0 = tiny
    ad = LORA.LoRAAdapters(net, rank=rank, alpha=rank / 2, targets=targets, seed=1)
    randomize_B(ad, std=0.02)
    steps = [(make_batch(cfg, 31 + 10 * i), step_args(method, 32 + 10 * i)) for i in range(micros)]
    ad.merge()
    ad.select(mode)
    ad.grads.fill_(float("nan"))
    for i, (batch, kw) in enumerate(steps):
        native_micro(net, method, batch, kw, 1.0 / micros, i == 0)
    if mode != "direct":
        ad.project()
    torch.cuda.synchronize()
    wm = {k: v.float().cpu() for k, v in net.state_dict().items()}           # bf16-rounded merged weights, as the step read them
    assert any(not torch.equal(wm[k], w[k]) for k in ad.targets)
    leaves = {k: wm[k].requires_grad_(True) for k in ad.targets}
    sum(oracle_loss(cfg, wm, method, batch, kw) for batch, kw in steps).mul(1.0 / micros).backward()
    par = GradParity(f"lora {mode} {method} r{rank} x{micros}")
    for k in ad.targets:
        dA, dB = LR.project64(leaves[k].grad, ad.A(k).cpu(), ad.B(k).cpu(), ad.scale)
        mod = k[: -len(".weight")]
        par.add(f"{mod}.lora_A.weight", ad.A(k, grad=True).cpu(), dA)
        par.add(f"{mod}.lora_B.weight", ad.B(k, grad=True).cpu(), dB)
    par.check(GRAD_BAR, expect=ad.param_ranges(), printer=lambda s: print("[parity] " + s))
    return ad


ALL_TARGETS = list(LORA.DEFAULT_TARGETS) + ["ff.net.2", "proj_in"]


@pytest.mark.parametrize("method,rank", [("ddpm", 4), ("ddpm", 16), ("flow_matching", 4), ("flow_matching", 16)])
@pytest.mark.parametrize("mode", ["project_frozen", "direct"])
def test_adapter_gradients_match_the_oracle(tiny, mode, method, rank):
    adapter_gradients_against_the_oracle(tiny, mode, method, rank, ALL_TARGETS)


def test_direct_with_a_partially_targeted_fused_op(tiny):
    """to_k left out: the fused q | k | v op holds two targets and rows that get nothing"""
    ad = adapter_gradients_against_the_oracle(tiny, "direct", "ddpm", 4, ["to_q", "to_v", "to_out.0"])
    assert not any(k.endswith("to_k.weight") for k in ad.targets)


def test_direct_with_the_time_embedding_projections_as_targets(tiny):
    """the grouped time_emb_proj op (its dY arrives as fp32 sums and is cast first; M = B rows, 17 targets in one table) and the four
    embedding linears (M = B) beside the attention projections"""
    ad = adapter_gradients_against_the_oracle(tiny, "direct", "ddpm", 4, list(LORA.DEFAULT_TARGETS) + ["time_emb_proj", "linear_1", "linear_2"])
    assert sum(k.endswith("time_emb_proj.weight") for k in ad.targets) == 17 and sum(".linear_" in k for k in ad.targets) == 4


ALONE = ["down_blocks.2.attentions.1.transformer_blocks.1.attn1.to_k", "mid_block.attentions.0.transformer_blocks.0.attn1.to_v",
         "up_blocks.1.attentions.2.transformer_blocks.0.attn2.to_v", "up_blocks.0.attentions.1.transformer_blocks.1.attn2.to_k"]


def test_a_targets_bits_do_not_depend_on_the_table_around_it(tiny):
    """Default targets: every fused q | k | v op holds a three-target table, the two grouped K | V ops tables of 10 and 14.  Four tensors
    that are NOT the first entry of their table -- to_k (entry 1) and to_v (entry 2) of a q | k | v op, an attn2.to_v at the end of the
    narrow group's table, an attn2.to_k in the middle of the wide one's -- against a run on the same merged model in which each is the only
    target of its op (a table of one: tile 0, reduce block 0, partial offset 0, scratch slot 0): bit for bit."""
    cfg, w, net, w0 = tiny
    full = LORA.LoRAAdapters(net, rank=4, alpha=2.0, seed=1)
    randomize_B(full, std=0.02)
    keys = [k + ".weight" for k in ALONE]
    shapes = net.param_shapes()
    place = {k: [t for t in full.targets if LORA.op_of(t, shapes[t]) == LORA.op_of(k, shapes[k])].index(k) for k in keys}
    assert place[keys[0]] == 1 and place[keys[1]] == 2 and all(v > 0 for v in place.values()), place      # no first entry of a table
    batch, kw = make_batch(cfg, 31), step_args("ddpm", 32)
    full.merge()
    full.select("direct")
    full.grads.fill_(float("nan"))
    native_micro(net, "ddpm", batch, kw, 1.0, True)
    torch.cuda.synchronize()
    among = {k: (full.A(k, grad=True).clone(), full.B(k, grad=True).clone()) for k in keys}
    net.set_trainable(None)
    net.weights.copy_(w0)
    one = LORA.LoRAAdapters(net, rank=4, alpha=2.0, targets=ALONE, seed=1)
    assert sorted(one.targets) == sorted(keys)
    for k in keys:      # the same adapters
        one.A(k).copy_(full.A(k))
        one.B(k).copy_(full.B(k))
    full.merge()        # the same merged model (every target of the first run)
    one.select("direct")
    one.grads.fill_(float("nan"))
    native_micro(net, "ddpm", batch, kw, 1.0, True)
    torch.cuda.synchronize()
    for k in keys:
        assert bool(torch.isfinite(among[k][0]).all()) and float(among[k][1].abs().max()) > 0, k
        assert same_bits(one.A(k, grad=True), among[k][0]) and same_bits(one.B(k, grad=True), among[k][1]), k


def test_direct_two_micro_step_cycle_matches_the_oracles_sum(tiny):
    adapter_gradients_against_the_oracle(tiny, "direct", "ddpm", 4, ALL_TARGETS, micros=2)


def run_training(net, method, steps, accum=2, save_at=None, save_dir=None, resume_from=None, first_step=0, **training):
    cfg = U.tiny_config()
    tr = make_trainer(net, method, lora_rank=4, lora_alpha=8.0, gradient_accumulation_steps=accum, **training)
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


def test_project_written_out_is_the_default_bit_for_bit(tiny):
    cfg, w, net, w0 = tiny
    tr, losses = run_training(net, "ddpm", 2)
    first = (net.weights.clone(), net.grads.clone(), tr.lora.weights.clone(), tr.lora.grads.clone())
    tr.lora.restore()
    tr2, losses2 = run_training(net, "ddpm", 2, lora_backward="project")
    assert losses2 == losses and net.trainable() == set(net.param_shapes())
    for a, b in zip(first, (net.weights, net.grads, tr2.lora.weights, tr2.lora.grads)):
        assert same_bits(a, b)
    with pytest.raises(ValueError, match="lora_backward"):
        make_trainer(net, "ddpm", lora_rank=4, lora_backward="frozen")


@pytest.mark.parametrize("mode", ["project_frozen", "direct"])
def test_modes_train_only_the_targets_and_repeat_bit_for_bit(tiny, mode):
    cfg, w, net, w0 = tiny
    tr, losses = run_training(net, "ddpm", 3, lora_backward=mode)
    ad = tr.lora
    assert net.trainable() == set(LORA.trainable_for(mode, ad.targets, net.param_shapes()))
    first = (net.weights.clone(), ad.weights.clone(), ad.grads.clone(), losses)
    assert float(ad.weights.float().abs().max()) > 0 and not same_bits(net.weights, w0)
    ad.restore()
    torch.cuda.synchronize()
    assert same_bits(net.weights, w0)
    net.set_trainable(None)
    tr2, losses2 = run_training(net, "ddpm", 3, lora_backward=mode)
    for a, b in zip(first[:3], (net.weights, tr2.lora.weights, tr2.lora.grads)):
        assert same_bits(a, b)
    assert losses2 == first[3]


def test_direct_twenty_steps_on_one_batch_lower_its_loss(tiny):
    cfg, w, net, w0 = tiny
    tr = make_trainer(net, "ddpm", lora_rank=4, lora_backward="direct")
    batch = make_batch(cfg, 41)
    noise = torch.randn(batch["vae_latents"].shape, generator=torch.Generator().manual_seed(42))       # evaluate() draws the same
    ts = torch.full((2,), 500, dtype=torch.long)
    evaluate = lambda: tr.evaluate([batch], [500], generator=torch.Generator().manual_seed(42))[1]
    before = evaluate()
    for _ in range(20):
        tr._execute_training_step(batch, timesteps=ts, noise=noise)
        tr.optimizer_step()
    after = evaluate()
    print(f"[lora] direct: evaluation loss {before:.6f} -> {after:.6f} after 20 steps")
    assert after < before


def test_direct_checkpoint_round_trip(tiny, tmp_path):
    cfg, w, net, w0 = tiny
    tr, _l = run_training(net, "ddpm", 3, save_at=1, save_dir=tmp_path / "ck", lora_backward="direct")
    want = (net.weights.clone(), tr.lora.weights.clone(), tr.optimizer.exp_avg.clone(), tr.optimizer.exp_avg_sq.clone())
    net.set_trainable(None)
    net.weights.copy_(w0)                                      # a fresh process would load the checkpoint's UNet
    tr2, _l = run_training(net, "ddpm", 1, resume_from=tmp_path / "ck", first_step=2, lora_backward="direct")
    for a, b in zip(want, (net.weights, tr2.lora.weights, tr2.optimizer.exp_avg, tr2.optimizer.exp_avg_sq)):
        assert same_bits(a, b)


# ------------------------------------------------------------------------------------------------ 8. two ranks
def test_two_ranks_exchange_direct_adapter_gradients_bit_equal_to_the_sum():
    from test_gpu_multiproc import run_dist
    env = dict(os.environ, MASTER_ADDR="127.0.0.1")
    r = run_dist([str(ROOT / "tests" / "_lora_direct_dp_worker.py")], 29761, env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "LORA_DIRECT_DP_OK" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
