"""Input gradients (sdxl_batch_din) on the GPU:
  1. the kernel of csrc/input_dgrad.hip through its hook: exact on integers, bounded per element against float64 (tests/_input_grad_ref.py),
     inside guard bands with poisoned neighbour samples, the gate, two runs;
  2. the tiny UNet's d input against autograd of the fp32 oracle (the sample a leaf), ddpm and flow matching, 4, 8 and 9 input channels;
  3. semantics: what the header promises about the other bits, overwrite, scale, gate, the second micro-step, graph mode, the frozen UNet,
     the plan's value against the hook's on the plan's own operands, bad arguments;
  4. NativeUNet.differentiable against the explicit unet_forward / unet_backward pair, and an encoder trained through the trainer's loss."""
import ctypes as C
import dataclasses
import importlib

import pytest
import torch

import sdxl_amd  # noqa: F401
from oracle import loss_ref as R
from oracle import unet_ref as U
from sdxl_amd import lib
from sdxl_amd import unet as NU

import _exact as E
import _input_grad_ref as IR
import _residual_ref as RR
from _isolation import Spec, assert_isolated, run_isolated
from test_gpu_cond_grads import RAGGED
from test_gpu_model import LOSS_RTOL, TINY_GRAD_BAR, make_inputs

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16


def _st():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _p(t):
    return None if t is None else C.c_void_p(t if isinstance(t, int) else t.data_ptr())


def _bits(t):
    return None if t is None else t.detach().contiguous().clone().view({2: torch.int16, 4: torch.int32}[t.element_size()])


def input_dgrad(dy, w, B, H, W, cin, cout, gate=None, dx=None):
    """the hook on device tensors: dy bf16 [B * H * W][cout], w bf16 [cout][9][Cs] -> dx fp32 [B][cin][H][W] (NaN where nothing is written)"""
    dx = torch.full((B, cin, H, W), float("nan"), dtype=torch.float32, device=DEV) if dx is None else dx
    lib.check(lib.load().sdxl_op_input_dgrad(_p(dy), _p(w), _p(dx), _p(gate), B, H, W, cin, cout, _st()), "sdxl_op_input_dgrad")
    return dx


# ---------------------------------------------------------------------------------------------------------------- 1. the kernel
# (B, H, W, in_channels, Cout).  The tile is 16 x 16 pixels of one sample and Cout is walked in chunks of 64 with a last chunk of 32:
# one pixel; an image inside one tile; 13 x 19 (two ragged tiles) with every in_channels (4: Cs = 8 half empty, 8: full, 9: Cs = 16, 16: full);
# exactly one tile; 17 x 64 (a second tile row of one pixel row, float4 stores); the ragged default bucket; Cout 32 (one short chunk),
# 64, 96 (a whole chunk and a short one) and 320
KERNEL_CASES = [(1, 1, 1, 4, 32), (2, 3, 5, 9, 96), (2, 13, 19, 4, 64), (2, 13, 19, 8, 32), (2, 13, 19, 9, 320), (2, 13, 19, 16, 64),
                (1, 16, 16, 16, 320), (2, 17, 64, 8, 320), (1, 104, 152, 9, 64)]
_ids = ["-".join(map(str, c)) for c in KERNEL_CASES]


@pytest.mark.parametrize("B,H,W,cin,cout", KERNEL_CASES, ids=_ids)
def test_kernel_is_exact_on_integers(B, H, W, cin, cout):
    """dy, w in {-2 .. 2}: every partial sum is an integer of magnitude <= 4 * 9 * Cout < 2^24, exact in fp32 in any order"""
    dy, w = IR.operands(B, H, W, cin, cout, integer=True, seed=1)
    want = E.expect(IR.input_dgrad_ref64(dy, w, B, H, W, cin), out_bf16=False)
    got = input_dgrad(dy.to(DEV, BF), w.to(DEV, BF), B, H, W, cin, cout)
    E.assert_exact(f"input_dgrad {B}x{H}x{W} c={cin} Cout={cout}", got, want)


@pytest.mark.parametrize("B,H,W,cin,cout", KERNEL_CASES, ids=_ids)
def test_kernel_on_normal_operands_within_the_fp32_bound(B, H, W, cin, cout):
    """every element within 2^-24 |ref| + K 2^-23 sum |dy| |w|, K = 9 Cout (tests/_exact.py: fp32 output, fp32 accumulation in any order)"""
    dy, w = IR.operands(B, H, W, cin, cout, integer=False, seed=2)
    ref = IR.input_dgrad_ref64(dy, w, B, H, W, cin)
    bnd = E.bound(ref, IR.input_dgrad_ref64(dy, w, B, H, W, cin, absolute=True), 9 * cout, out_bf16=False)
    got = input_dgrad(dy.to(DEV, BF), w.to(DEV, BF), B, H, W, cin, cout)
    E.check_bound(f"input_dgrad {B}x{H}x{W} c={cin} Cout={cout}", got, ref, bnd)


ISOLATION_CASES = [(2, 13, 19, 4, 64), (1, 17, 20, 9, 96)]


@pytest.mark.parametrize("B,H,W,cin,cout", ISOLATION_CASES, ids=["-".join(map(str, c)) for c in ISOLATION_CASES])
def test_kernel_touches_nothing_but_its_operands(B, H, W, cin, cout):
    """tests/_isolation.py.  dy is dense, so what surrounds a sample is its neighbour samples: the call covers the B samples in the middle
    of B + 2, and the first and the last are poisoned in the 0xFF / 0x7F runs -- row -1 of a sample is not the last row of the one before
    it.  w has row stride Cs with in_channels columns of contents: its pad channels hold the fill (NaN / 3.4e38), which only the columns
    behind in_channels of the product see, and those are never stored.  dx lies between guard bands."""
    L = lib.load()
    cs, hw = IR.input_cs(cin), H * W
    dy, w = IR.operands(B + 2, H, W, cin, cout, integer=False, seed=3)
    specs = [Spec("dy", (B + 2) * hw, cout, init=dy), Spec("w", cout * 9, cin, ld=cs, init=w.reshape(cout * 9, cs)[:, :cin]),
             Spec("dx", B * cin * H, W, dtype=torch.float32, role="out")]
    outer = torch.zeros((B + 2) * hw, dtype=torch.bool, device=DEV)
    outer[:hw] = True
    outer[(B + 1) * hw:] = True

    def run(ar):
        lib.check(L.sdxl_op_input_dgrad(ar.ptr("dy", hw * cout), ar.ptr("w"), ar.ptr("dx"), None, B, H, W, cin, cout, _st()))
    runs = run_isolated(run, specs, device=DEV, poison={"dy": outer})
    assert_isolated(runs, what="input_dgrad")
    mid = dy[hw:(B + 1) * hw]
    ref = IR.input_dgrad_ref64(mid, w, B, H, W, cin)
    bnd = E.bound(ref, IR.input_dgrad_ref64(mid, w, B, H, W, cin, absolute=True), 9 * cout, out_bf16=False)
    E.check_bound("input_dgrad inside guard bands", runs[0]["dx"].reshape(B, cin, H, W), ref, bnd)


def test_kernel_gate_and_two_runs():
    B, H, W, cin, cout = 2, 13, 19, 9, 320
    dy, w = IR.operands(B, H, W, cin, cout, integer=False, seed=4)
    d_dy, d_w = dy.to(DEV, BF), w.to(DEV, BF)
    plain = input_dgrad(d_dy, d_w, B, H, W, cin, cout)
    assert bool(torch.isfinite(plain).all()) and int(plain.ne(0).sum()) > 0
    again = input_dgrad(d_dy, d_w, B, H, W, cin, cout)
    assert torch.equal(_bits(again), _bits(plain))                                             # reproducible
    opened = input_dgrad(d_dy, d_w, B, H, W, cin, cout, gate=torch.tensor([1.0], device=DEV))
    assert torch.equal(_bits(opened), _bits(plain))                                            # an open gate: the bits of gate = NULL
    nan_dy = torch.full_like(d_dy, float("nan"))
    closed = input_dgrad(nan_dy, d_w, B, H, W, cin, cout, gate=torch.tensor([0.0], device=DEV), dx=torch.full((B, cin, H, W), 7.0, device=DEV))
    assert int(_bits(closed).ne(0).sum()) == 0                                                 # a closed gate: exact zeros, dy not read


# ---------------------------------------------------------------------------------------------------------------- the tiny UNets
def _native_cfg(c: U.UNetConfig):
    return NU.make_config(in_channels=c.in_channels, block_out_channels=c.block_out_channels, transformer_layers=c.transformer_layers_per_block,
                          cross_attention_dim=c.cross_attention_dim, addition_time_embed_dim=c.addition_time_embed_dim, pooled_dim=c.pooled_dim)


def _tiny(c):
    cfg = dataclasses.replace(U.tiny_config(), in_channels=c)
    w = U.synth_weights(cfg, seed=0)
    net = NU.NativeUNet(_native_cfg(cfg))
    net.load_state_dict(w)
    return cfg, w, net


@pytest.fixture(scope="module")
def tiny():
    cfg, w, net = _tiny(4)
    yield cfg, w, net
    net.close()


@pytest.fixture(scope="module")
def tiny8():
    cfg, w, net = _tiny(8)
    yield cfg, w, net
    net.close()


@pytest.fixture(scope="module")
def tiny9():
    cfg, w, net = _tiny(9)
    yield cfg, w, net
    net.close()


def _parity(label, got, ref):
    a, b = got.detach().cpu().double().flatten(), ref.detach().double().flatten()
    rel = float((a - b).norm() / b.norm())
    cos = float(torch.dot(a, b) / (a.norm() * b.norm()))
    print(f"[parity] {label}: rel-L2 {rel:.3e} cos {cos:.6f} |ref| {float(b.norm()):.3e} (bar rel-L2 <= {TINY_GRAD_BAR[0]:.0e}, cos >= {TINY_GRAD_BAR[1]})")
    return rel, cos


def _make_cond(cfg, B, H, W, seed):
    n = cfg.in_channels - 4
    return None if n == 0 else torch.randn(B, n, H, W, generator=torch.Generator().manual_seed(seed))


def _oracle_step(w, cfg, method, x, B, ic):
    """the fp32 oracle's loss with the UNet input a leaf: (result dict, d loss / d input [B, in_channels, H, W], (sigma_or_t, timestep))"""
    leaf = {}

    def unet_fn(s, t, e, p, ti):
        full = (s if ic is None else torch.cat([s, ic], dim=1)).detach().clone().requires_grad_(True)
        leaf["x"] = full
        return U.unet_forward(w, full, t, e, p, ti, cfg)
    batch = {"vae_latents": x["lat"], "prompt_embeds": x["ehs"], "pooled_prompt_embeds": x["pooled"], "time_ids": x["tid"]}
    if method == "ddpm":
        ts = torch.tensor([700, 420][:B])
        ref, args = R.compute_loss_ddpm(unet_fn, batch, x["noise"], ts), (R.karras_sigmas()[ts], ts.float())
    else:
        tf = R.sample_logit_normal_from_z(x["z"])
        ref, args = R.compute_loss_flow(unet_fn, batch, x["noise"], tf), (tf, tf)
    ref["loss"].backward()
    return ref, leaf["x"].grad, args


def _run_oracle_case(tiny_, method, B, H, W, seed):
    cfg, w, net = tiny_
    x = make_inputs(cfg, B, H, W, seed=seed)
    ic = _make_cond(cfg, B, H, W, seed + 1)
    ref, want, (s_or_t, t_in) = _oracle_step(w, cfg, method, x, B, ic)
    kw = {} if ic is None else dict(input_cond=ic)
    net.forward_loss(method, x["lat"], x["noise"], s_or_t, t_in, x["ehs"], x["pooled"], x["tid"], input_grad=True, **kw)
    net.zero_grads()
    net.backward(1.0, True)
    got_loss, ref_loss = net.read_loss()[0], float(ref["loss"].detach())
    rel = abs(got_loss - ref_loss) / abs(ref_loss)
    print(f"[parity] tiny c={cfg.in_channels} {method} {B}x{H}x{W} loss: hip {got_loss:.6f} oracle {ref_loss:.6f} rel {rel:.3e} (tol {LOSS_RTOL})")
    assert rel <= LOSS_RTOL
    d = net.read_input_grad()
    assert d.dtype == torch.float32 and d.is_cuda and tuple(d.shape) == (B, cfg.in_channels, H, W) == tuple(want.shape)
    assert float(want.norm()) > 0 and (ic is None or float(want[:, 4:].norm()) > 0)
    out = [_parity(f"tiny c={cfg.in_channels} {method} {B}x{H}x{W} d input", d, want)]
    if ic is not None:
        out.append(_parity(f"tiny c={cfg.in_channels} {method} {B}x{H}x{W} d input_cond", d[:, 4:], want[:, 4:]))
    for rel, cos in out:
        assert rel <= TINY_GRAD_BAR[0] and cos >= TINY_GRAD_BAR[1]


ORACLE_CASES = [("ddpm", 1, 32, 32), ("flow_matching", 2, *RAGGED)]


@pytest.mark.parametrize("method,B,H,W", ORACLE_CASES, ids=[f"{m}-{b}-{h}-{w}" for m, b, h, w in ORACLE_CASES])
def test_tiny_unet_input_gradient_matches_oracle(tiny, method, B, H, W):
    _run_oracle_case(tiny, method, B, H, W, seed=13 if method == "ddpm" else 17)


def test_tiny_unet_input_gradient_matches_oracle_8_channels(tiny8):
    _run_oracle_case(tiny8, "flow_matching", 2, 16, 16, seed=19)


def test_tiny_unet_input_gradient_matches_oracle_9_channels(tiny9):
    _run_oracle_case(tiny9, "flow_matching", 2, 16, 16, seed=23)


# ---------------------------------------------------------------------------------------------------------------- 3. semantics
def _dev(res):
    down, mid = res
    return [None if t is None else t.to(DEV).contiguous() for t in down], None if mid is None else mid.to(DEV).contiguous()


def _step(net, x, input_grad=False, scale=1.0, first=True, zero=True, on_segment=None, poison=False, **kw):
    """one flow-matching step; (read_loss's values, the gradient arena's bits, d input's bits or None).  poison: the output buffer holds NaN
    patterns when the backward starts"""
    tf = R.sample_logit_normal_from_z(x["z"])
    if input_grad:
        kw["input_grad"] = True
    net.forward_loss("flow_matching", x["lat"], x["noise"], tf, tf, x["ehs"], x["pooled"], x["tid"], **kw)
    if poison:
        net.read_input_grad().view(torch.int32).fill_(-1)
    if zero:
        net.zero_grads()
    net.backward(scale, first, on_segment=on_segment)
    out = net.read_loss()
    return out, _bits(net.grads), _bits(net.read_input_grad())


def _others(net):
    d_e, d_p = net.read_cond_grads()
    d_down, d_mid = net.read_residual_grads()
    return [_bits(d_e), _bits(d_p)] + [_bits(t) for t in list(d_down or []) + [d_mid]]


def _same(a, b):
    return len(a) == len(b) and all((p is None and q is None) or torch.equal(p, q) for p, q in zip(a, b))


def test_request_changes_no_other_bit(tiny):
    cfg, _, net = tiny
    B, H, W = 2, 16, 16
    x = make_inputs(cfg, B, H, W, seed=31)
    res = _dev(RR.make_residuals(cfg, B, H, W))
    out0, g0, d0 = _step(net, x)
    assert d0 is None and net.read_input_grad() is None
    out1, g1, d1 = _step(net, x, True)
    assert out1 == out0 and torch.equal(g1, g0) and int(d1.ne(0).sum()) > 0 and bool(torch.isfinite(d1.view(torch.float32)).all())
    # beside the conditioning gradients, residuals and the residual gradients
    full = dict(cond_grads=True, residuals=res, residual_grads=True)
    outa, ga, da = _step(net, x, **full)
    oa = _others(net)
    outb, gb, db = _step(net, x, True, **full)
    ob = _others(net)
    assert da is None and outb == outa and torch.equal(gb, ga) and _same(ob, oa) and all(t is not None for t in ob)
    assert not torch.equal(db, d1)                                   # (the residuals move the step)
    # two runs, and the per-segment backward (the exchange's path): the same bits
    _, _, dc = _step(net, x, True, **full)
    assert torch.equal(dc, db)
    outs, gs, ds = _step(net, x, True, on_segment=lambda k, off, n: None, **full)
    assert outs == outa and torch.equal(gs, ga) and torch.equal(ds, db) and _same(_others(net), oa)
    # a buffer that holds a NaN pattern when the backward starts is overwritten in full
    _, _, dp = _step(net, x, True, poison=True)
    assert torch.equal(dp, d1)


def test_scale_gate_second_micro_step_and_frozen_unet(tiny):
    cfg, _, net = tiny
    B, H, W = 2, 16, 16
    x, y = make_inputs(cfg, B, H, W, seed=32), make_inputs(cfg, B, H, W, seed=33)
    _, _, d1 = _step(net, x, True)
    _, _, dq = _step(net, x, True, scale=0.25)
    # grad_scale multiplies d(pred); 0.25 is a power of two, so every later product, sum and rounding scales exactly
    assert torch.equal(dq, _bits(d1.view(torch.float32) * 0.25))
    # a closed gate (a non-finite latent: the loss is not finite, the activations of that sample are not either): exact zeros
    bad = dict(x)
    bad["lat"] = x["lat"].clone()
    bad["lat"][0, 0, 0, 0] = float("inf")
    out, _, dz = _step(net, bad, True, poison=True)
    assert out[7] == 0.0 and int(dz.ne(0).sum()) == 0
    # the second micro-step of a cycle overwrites: the bits of the same batch run alone
    _, _, dy = _step(net, y, True)
    _step(net, x, True)
    _, _, dy2 = _step(net, y, True, first=False, zero=False)
    assert torch.equal(dy2, dy)
    # everything frozen (score distillation, guidance, reward fine-tuning on a frozen UNet): the same bits
    net.set_trainable([])
    try:
        _, _, df = _step(net, y, True)
    finally:
        net.set_trainable(None)
    assert torch.equal(df, dy)


def test_graph_mode_gives_the_eager_bits(tiny):
    cfg, _, net = tiny
    B, H, W = 2, 16, 16
    x = make_inputs(cfg, B, H, W, seed=34)
    out0, g0, d0 = _step(net, x, True)
    outp, gp, _ = _step(net, x)
    assert outp == out0 and torch.equal(gp, g0)
    net.set_graph_mode(True)
    try:
        for i in range(3):      # (the plain call: eager, capture, replay; the backward of a requesting micro-step never captures)
            out, g, d = _step(net, x, True)
            assert out == out0 and torch.equal(g, g0) and torch.equal(d, d0), i
            out, g, d = _step(net, x)
            assert out == out0 and torch.equal(g, g0) and d is None, i
    finally:
        net.set_graph_mode(False)


def test_plan_value_is_the_hooks_on_the_plans_own_operands(tiny9):
    """unet_forward / unet_backward with a seeded d(pred): d input equals what sdxl_op_input_dgrad computes from conv_in's output gradient as
    the workspace holds it after the backward and conv_in's weight in the arena -- and that lies within the kernel's bound of the float64
    reference on the same operands; against the oracle's autograd of <dpred, pred> at the project's bar."""
    cfg, w, net = tiny9
    B, H, W, cin = 2, 16, 16, 9
    x = make_inputs(cfg, B, H, W, seed=35)
    sample = torch.cat([x["lat"] * 2.0, _make_cond(cfg, B, H, W, 36)], dim=1).to(BF).float()
    t = torch.tensor([10.0, 500.0])
    dpred = torch.randn(B, 4, H, W, generator=torch.Generator().manual_seed(37)).to(BF).float()
    net.unet_forward(sample, t, x["ehs"], x["pooled"], x["tid"], input_grad=True)
    net.zero_grads()
    net.unet_backward(dpred, True)
    d = net.read_input_grad()
    off, woff, cout = C.c_size_t(), C.c_size_t(), C.c_int()
    lib.check(lib.load().sdxl_debug_input_dgrad_operands(net.h, C.byref(off), C.byref(woff), C.byref(cout)))
    assert cout.value == cfg.block_out_channels[0]
    cs = IR.input_cs(cin)
    dy = net.workspace[off.value: off.value + 2 * B * H * W * cout.value].view(BF).view(B * H * W, cout.value)
    wt = net.weights[woff.value: woff.value + cout.value * 9 * cs].view(cout.value, 9, cs)
    assert int(wt[:, :, cin:].ne(0).sum()) == 0 and int(dy.ne(0).sum()) > 0
    h = input_dgrad(dy, wt, B, H, W, cin, cout.value)
    assert int(d.ne(0).sum()) > 0 and torch.equal(_bits(d), _bits(h))
    ref = IR.input_dgrad_ref64(dy.float().cpu(), wt.float().cpu(), B, H, W, cin)
    bnd = E.bound(ref, IR.input_dgrad_ref64(dy.float().cpu(), wt.float().cpu(), B, H, W, cin, absolute=True), 9 * cout.value, out_bf16=False)
    E.check_bound("plan d input against float64 on the plan's dy", d, ref, bnd)
    leaf = sample.clone().requires_grad_(True)
    (dpred * U.unet_forward(w, leaf, t, x["ehs"], x["pooled"], x["tid"], cfg)).sum().backward()
    rel, cos = _parity("unet_backward d sample (9 channels)", d, leaf.grad)
    assert rel <= TINY_GRAD_BAR[0] and cos >= TINY_GRAD_BAR[1]


def test_bad_arguments_are_refused_before_any_launch(tiny):
    cfg, _, net = tiny
    B, H, W = 2, 16, 16
    L = lib.load()
    x = make_inputs(cfg, B, H, W, seed=38)
    _step(net, x)      # plans (2, 16, 16) and leaves a valid step behind
    keep = [t.to(DEV) for t in (x["lat"], x["noise"], torch.tensor([0.3, 0.6]), x["ehs"].to(BF), x["pooled"].to(BF), x["tid"])]
    lat, noise, tt, ehs, pooled, tid = keep
    out = torch.full((B, 4, H, W), 5.0, device=DEV)
    arena_before = _bits(net.grads)

    def call(d_input, sampler=None):
        b = lib.InputGradBatch(B, H, W, 77 | lib.BATCH_DIN, lat.data_ptr(), noise.data_ptr(), tt.data_ptr(), tt.data_ptr(), ehs.data_ptr(),
                               pooled.data_ptr(), tid.data_ptr(), None)
        b.d_input = d_input
        if sampler is not None:
            b.sampler = C.pointer(sampler)
            rc = L.sdxl_unet_forward(net.h, None, C.byref(b), None, _st())
        else:
            lc = lib.LossConfig(1, 1, 0, 0.0, 0)
            rc = L.sdxl_forward_loss(net.h, C.byref(lc), C.byref(b), _st())
        return rc, L.sdxl_last_error().decode()

    rc, msg = call(out.data_ptr() + 4)
    assert rc == 1 and "d_input" in msg and "aligned" in msg
    xs = torch.zeros(B, 4, H, W, device=DEV)
    step = lib.SamplerStep(xs.data_ptr(), 0, 0, 1.0, -1.0, 0.5, 0.5, 1.0, 0.0, 1.0, 0.0)
    rc, msg = call(out.data_ptr(), sampler=step)
    assert rc == 1 and "d_input" in msg and "sampler" in msg
    torch.cuda.synchronize()
    assert int(xs.ne(0).sum()) == 0 and int(out.ne(5.0).sum()) == 0 and torch.equal(_bits(net.grads), arena_before)      # nothing ran
    # the flag with a NULL pointer is a call without the request, bit for bit
    rc, msg = call(None)
    assert rc == 0, msg
    net.zero_grads()
    net.backward(1.0, True)
    want = _bits(net.grads)
    lc = lib.LossConfig(1, 1, 0, 0.0, 0)
    b = lib.Batch(B, H, W, 77, lat.data_ptr(), noise.data_ptr(), tt.data_ptr(), tt.data_ptr(), ehs.data_ptr(), pooled.data_ptr(), tid.data_ptr(), None)
    lib.check(L.sdxl_forward_loss(net.h, C.byref(lc), C.byref(b), _st()))
    net.zero_grads()
    net.backward(1.0, True)
    assert torch.equal(_bits(net.grads), want) and int(out.ne(5.0).sum()) == 0


# ---------------------------------------------------------------------------------------------------------------- 4. autograd
def test_differentiable_has_the_bits_of_the_explicit_pair(tiny):
    cfg, _, net = tiny
    B, H, W = 2, 16, 16
    x = make_inputs(cfg, B, H, W, seed=41)
    sample = (x["lat"] * 2.0).to(BF).float()
    t = torch.tensor([10.0, 500.0])
    res = _dev(RR.make_residuals(cfg, B, H, W))
    dpred = torch.randn(B, 4, H, W, generator=torch.Generator().manual_seed(42)).to(BF).float()
    # the explicit pair
    pred0 = net.unet_forward(sample, t, x["ehs"], x["pooled"], x["tid"], cond_grads=True, residuals=res, residual_grads=True, input_grad=True)
    net.zero_grads()
    net.unet_backward(dpred, True)
    want = [_bits(net.read_input_grad())] + _others(net)
    arena = _bits(net.grads)
    # the autograd function, every tensor input a leaf (the sample and the conditioning on the CPU, in fp64: each gradient comes back there)
    s, e, p = sample.double().requires_grad_(True), x["ehs"].clone().requires_grad_(True), x["pooled"].clone().requires_grad_(True)
    down, mid = [r.clone().requires_grad_(True) for r in res[0]], res[1].clone().requires_grad_(True)
    pred = net.differentiable(s, t, e, p, x["tid"], residuals=(down, mid))
    assert torch.equal(_bits(pred), _bits(pred0)) and pred.requires_grad
    net.zero_grads()
    (pred * dpred.to(pred.device)).sum().backward()
    got = [s.grad, e.grad, p.grad] + [r.grad for r in down] + [mid.grad]
    assert s.grad.dtype == torch.float64 and s.grad.device.type == "cpu" and down[0].grad.is_cuda
    for i, (g, wbits) in enumerate(zip(got, want)):
        ref = wbits.view(torch.float32).reshape(g.shape)
        assert torch.allclose(g.float().cpu(), ref.cpu()), i
        assert torch.equal(_bits(g.float().cpu()), _bits(ref.cpu())), i      # the same kernels on the same operands: the same bits
    assert torch.equal(_bits(net.grads), arena)
    # the backward of a stale forward is refused
    stale = net.differentiable(s, t, e, p, x["tid"])
    net.unet_forward(sample, t, x["ehs"], x["pooled"], x["tid"])
    with pytest.raises(lib.SdxlError, match="stale forward"):
        stale.sum().backward()


def test_an_encoder_in_front_of_input_cond_trains_through_the_trainers_loss(tiny8):
    cfg, w, net = tiny8
    cfgm = importlib.import_module("sdxl-training-improvements_amd.config")
    TR = importlib.import_module("sdxl-training-improvements_amd.trainer")
    B, H, W = 2, 16, 16
    x = make_inputs(cfg, B, H, W, seed=43)
    noise = torch.randn(B, 4, H, W, generator=torch.Generator().manual_seed(44))
    t = torch.tensor([0.21, 0.83])

    class M:
        unet = net

    c = cfgm.Config()
    c.training.method = "flow_matching"
    c.training.mixed_precision = "no"
    c.training.input_conditioning = "concat"
    torch.manual_seed(45)
    enc = torch.nn.Conv2d(3, 4, 3, padding=1).to(DEV)
    src = torch.randn(B, 3, H, W, generator=torch.Generator().manual_seed(46)).to(DEV)
    tr = TR.NativeSDXLTrainer(M(), config=c)
    batch = {"vae_latents": x["lat"], "prompt_embeds": x["ehs"], "pooled_prompt_embeds": x["pooled"], "time_ids": x["tid"], "cond_latents": enc(src),
             "metadata": {}}
    tr.zero_grad()
    out = tr.compute_loss(batch, timesteps=t, noise=noise, generator=torch.Generator().manual_seed(47))
    out["loss"].backward()
    torch.cuda.synchronize()
    d = net.read_input_grad()
    assert tuple(d.shape) == (B, 8, H, W)
    gw, gb = torch.autograd.grad(enc(src), [enc.weight, enc.bias], d[:, 4:])
    for name, g, ref in (("weight", enc.weight.grad, gw), ("bias", enc.bias.grad, gb)):
        assert g is not None and bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0, name
        err = float((g - ref).abs().max() / ref.abs().max())
        print(f"[trainer] encoder {name} gradient: max |g - conv2d backward of d_input[:, 4:]| / max |.| = {err:.3e}")
        assert torch.allclose(g, ref, rtol=1e-4, atol=1e-5 * float(ref.abs().max())), name
    # against the oracle with the same encoder in front: the whole chain
    ref_enc = torch.nn.Conv2d(3, 4, 3, padding=1)
    ref_enc.load_state_dict({k: v.detach().cpu() for k, v in enc.state_dict().items()})
    ic = ref_enc(src.cpu())
    b0 = {k: v for k, v in batch.items() if k not in ("metadata", "cond_latents")}
    ref = R.compute_loss_flow(lambda s, tt, e, p, ti: U.unet_forward(w, torch.cat([s, ic], dim=1), tt, e, p, ti, cfg), b0, noise, t)
    ref["loss"].backward()
    got_loss, ref_loss = float(out["loss"].detach()), float(ref["loss"].detach())
    rel = abs(got_loss - ref_loss) / abs(ref_loss)
    print(f"[trainer] encoder loss: hip {got_loss:.6f} oracle {ref_loss:.6f} rel {rel:.3e}")
    assert rel <= LOSS_RTOL
    rel, cos = _parity("encoder weight through the native loss", enc.weight.grad, ref_enc.weight.grad)
    assert rel <= TINY_GRAD_BAR[0] and cos >= TINY_GRAD_BAR[1]
    # evaluate asks for nothing
    tr.evaluate([dict(batch, cond_latents=batch["cond_latents"].detach())], [0.5], generator=torch.Generator().manual_seed(48))
    assert net.read_input_grad() is None
