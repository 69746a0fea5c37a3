"""Additional skip residuals (sdxl_residuals) on the GPU:
  1. the two kernels of csrc/residual.hip through their hooks, bit for bit, and inside guard bands;
  2. the tiny UNet's forward with residuals against the oracle's restatement (tests/_residual_ref.py);
  3. a training step: the loss, all ten residual gradients and a handful of parameter gradients against autograd of the fp32 oracle;
  4. semantics: what the header promises about bits, scale, overwrite, graph mode, the frozen UNet, sdxl_unet_backward, bad arguments;
  5. one guided sampler step; 6. a torch control module trained through the trainer's loss."""
import ctypes as C
import importlib

import pytest
import torch

import sdxl_amd  # noqa: F401
from oracle import loss_ref as R
from oracle import unet_ref as U
from sdxl_amd import lib
from sdxl_amd import sampler as S
from sdxl_amd import unet as NU

import _bucket_cases as BK
import _residual_ref as RR
import _sampler_ref as SR
from _isolation import Spec, assert_isolated, run_isolated
from test_gpu_model import LOSS_RTOL, PROBE_GRADS, TINY_GRAD_BAR, make_inputs, tiny_native_cfg

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _st():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _p(t):
    return None if t is None else C.c_void_p(t if isinstance(t, int) else t.data_ptr())


def _bits(t):
    return None if t is None else t.detach().contiguous().clone().view({2: torch.int16, 4: torch.int32}[t.element_size()])


# ---------------------------------------------------------------------------------------------------------------- 1. the hooks
HOOK_SHAPES = [(2, 6, 256, 256), (1, 35, 64, 40), (2, 988, 128, 64), (1, 256, 64, 64)]      # (B, HW, Ca, Cb): plane strides 6 (2-wide),
                                                                                            # 35 (scalar), 988 and 256 (4-wide); a ragged channel tile


def _hook_operands(B, HW, Ca, Cb, rdtype, seed=0):
    g = torch.Generator().manual_seed(seed)
    a = torch.randn(B * HW, Ca, generator=g).to(torch.bfloat16)
    b = torch.randn(B * HW, Cb, generator=g).to(torch.bfloat16)
    ra = (0.5 * torch.randn(B, Ca, HW, generator=g)).to(torch.bfloat16).to(rdtype)
    rb = (0.5 * torch.randn(B, Cb, HW, generator=g)).to(torch.bfloat16).to(rdtype)
    return a, b, ra, rb


def _concat_ref(a, b, ra, rb, B, HW):
    """exact: one fp32 add, one round to nearest even (torch's .to(bfloat16))"""
    nchw = lambda r, C_: r.float().reshape(B, C_, HW).permute(0, 2, 1).reshape(B * HW, C_)
    ha = a if ra is None else (a.float() + nchw(ra, a.shape[1])).to(torch.bfloat16)
    hb = b if rb is None else (b.float() + nchw(rb, b.shape[1])).to(torch.bfloat16)
    return torch.cat([ha, hb], dim=1)


@pytest.mark.parametrize("mode", ["ra", "rb", "both"])
@pytest.mark.parametrize("rdtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("B,HW,Ca,Cb", HOOK_SHAPES, ids=["-".join(map(str, s)) for s in HOOK_SHAPES])
def test_hooks_bit_for_bit(B, HW, Ca, Cb, rdtype, mode):
    L = lib.load()
    a, b, ra, rb = _hook_operands(B, HW, Ca, Cb, rdtype)
    ra, rb = (ra if mode != "rb" else None), (rb if mode != "ra" else None)
    want = _concat_ref(a, b, ra, rb, B, HW)
    d = lambda t: None if t is None else t.to(DEV)
    da_, db_, dra, drb = d(a), d(b), d(ra), d(rb)
    o = torch.full((B * HW, Ca + Cb), float("nan"), dtype=torch.bfloat16, device=DEV)
    lib.check(L.sdxl_op_concat_residual(_p(da_), Ca, _p(db_), Cb, _p(dra), _p(drb), 0 if rdtype == torch.float32 else 1, _p(o), B, HW, _st()), "concat_residual")
    bad = int((_bits(o.cpu()) != _bits(want)).sum())
    assert bad == 0, f"{bad} of {want.numel()} elements differ from bf16_rn(float(x) + float(r))"
    # the gradient: columns of g as fp32 NCHW, only where asked
    g = torch.randn(B * HW, Ca + Cb, generator=torch.Generator().manual_seed(1)).to(torch.bfloat16)
    ga = torch.full((B, Ca, HW), float("nan"), device=DEV) if mode != "rb" else None
    gb = torch.full((B, Cb, HW), float("nan"), device=DEV) if mode != "ra" else None
    lib.check(L.sdxl_op_concat_residual_grad(_p(g.to(DEV)), Ca, Cb, _p(ga), _p(gb), None, B, HW, _st()), "concat_residual_grad")
    cols = lambda lo, hi: g[:, lo:hi].float().reshape(B, HW, hi - lo).permute(0, 2, 1).contiguous()
    if ga is not None:
        assert torch.equal(_bits(ga.cpu()), _bits(cols(0, Ca)))
    if gb is not None:
        assert torch.equal(_bits(gb.cpu()), _bits(cols(Ca, Ca + Cb)))


def test_hook_zero_residual_returns_the_concats_bits_and_a_closed_gate_exact_zeros():
    L = lib.load()
    B, HW, Ca, Cb = 2, 988, 128, 64
    a, b, ra, rb = _hook_operands(B, HW, Ca, Cb, torch.float32)
    a[0, 0], b[1, 1] = -0.0, float("inf")                 # r == 0 passes the bits: -0 stays -0 (float(-0) + 0 would be +0)
    da_, db_ = a.to(DEV), b.to(DEV)
    plain = torch.empty(B * HW, Ca + Cb, dtype=torch.bfloat16, device=DEV)
    lib.check(L.sdxl_op_concat_residual(_p(da_), Ca, _p(db_), Cb, None, None, 0, _p(plain), B, HW, _st()))      # both NULL: the plain concat
    assert torch.equal(_bits(plain.cpu()), _bits(torch.cat([a, b], dim=1)))
    for dt in (torch.float32, torch.bfloat16):
        o = torch.full_like(plain, float("nan"))
        za, zb = torch.zeros(B, Ca, HW, dtype=dt, device=DEV), torch.zeros(B, Cb, HW, dtype=dt, device=DEV)
        lib.check(L.sdxl_op_concat_residual(_p(da_), Ca, _p(db_), Cb, _p(za), _p(zb), 0 if dt == torch.float32 else 1, _p(o), B, HW, _st()))
        assert torch.equal(_bits(o), _bits(plain))
    g = torch.full((B * HW, Ca + Cb), float("nan"), dtype=torch.bfloat16, device=DEV)
    for gate, zero in ((0.0, True), (1.0, False)):
        ga, gb = torch.full((B, Ca, HW), 7.0, device=DEV), torch.full((B, Cb, HW), 7.0, device=DEV)
        gd = torch.tensor([gate], device=DEV)
        lib.check(L.sdxl_op_concat_residual_grad(_p(g), Ca, Cb, _p(ga), _p(gb), _p(gd), B, HW, _st()))
        for t in (ga, gb):
            assert (int(_bits(t).ne(0).sum()) == 0) if zero else bool(torch.isnan(t).all())


@pytest.mark.parametrize("B,HW,Ca,Cb", HOOK_SHAPES, ids=["-".join(map(str, s)) for s in HOOK_SHAPES])
def test_hooks_touch_nothing_but_their_operands(B, HW, Ca, Cb):
    """each shape once more inside guard bands (tests/_isolation.py): the bits do not depend on the surroundings, the guards and the
    read-only operands come out as they went in"""
    L = lib.load()
    a, b, ra, rb = _hook_operands(B, HW, Ca, Cb, torch.float32, seed=3)
    g = torch.randn(B * HW, Ca + Cb, generator=torch.Generator().manual_seed(4))
    fwd = [Spec("a", B * HW, Ca, init=a), Spec("b", B * HW, Cb, init=b), Spec("ra", B * Ca, HW, dtype=torch.float32, init=ra.reshape(B * Ca, HW)),
           Spec("rb", B * Cb, HW, dtype=torch.bfloat16, init=rb.reshape(B * Cb, HW)), Spec("o", B * HW, Ca + Cb, role="out")]

    def run_fwd(ar):      # one launch per residual dtype cannot mix them: ra as fp32 here, rb (bf16) in a second launch over the same output
        lib.check(L.sdxl_op_concat_residual(ar.ptr("a"), Ca, ar.ptr("b"), Cb, ar.ptr("ra"), None, 0, ar.ptr("o"), B, HW, _st()))
    runs = run_isolated(run_fwd, fwd, device=DEV)
    assert_isolated(runs, what="concat_residual fp32 ra")
    assert torch.equal(_bits(runs[0]["o"].cpu()), _bits(_concat_ref(a, b, ra, None, B, HW)))

    def run_fwd_b(ar):
        lib.check(L.sdxl_op_concat_residual(ar.ptr("a"), Ca, ar.ptr("b"), Cb, None, ar.ptr("rb"), 1, ar.ptr("o"), B, HW, _st()))
    runs = run_isolated(run_fwd_b, fwd, device=DEV)
    assert_isolated(runs, what="concat_residual bf16 rb")
    assert torch.equal(_bits(runs[0]["o"].cpu()), _bits(_concat_ref(a, b, None, rb.to(torch.bfloat16), B, HW)))

    bwd = [Spec("g", B * HW, Ca + Cb, init=g), Spec("da", B * Ca, HW, dtype=torch.float32, role="out"),
           Spec("db", B * Cb, HW, dtype=torch.float32, role="out")]

    def run_bwd(ar):
        lib.check(L.sdxl_op_concat_residual_grad(ar.ptr("g"), Ca, Cb, ar.ptr("da"), ar.ptr("db"), None, B, HW, _st()))
    runs = run_isolated(run_bwd, bwd, device=DEV)
    assert_isolated(runs, what="concat_residual_grad")
    gq = g.to(torch.bfloat16).float().reshape(B, HW, Ca + Cb).permute(0, 2, 1)
    assert torch.equal(runs[0]["da"].cpu().reshape(B, Ca, HW), gq[:, :Ca]) and torch.equal(runs[0]["db"].cpu().reshape(B, Cb, HW), gq[:, Ca:])


# ---------------------------------------------------------------------------------------------------------------- the tiny UNet
@pytest.fixture(scope="module")
def tiny():
    cfg = U.tiny_config()
    w = U.synth_weights(cfg, seed=0)
    net = NU.NativeUNet(tiny_native_cfg(cfg))
    net.load_state_dict(w)
    yield cfg, w, net
    net.close()


def _dev(res):
    down, mid = res
    return [None if t is None else t.to(DEV).contiguous() for t in down], None if mid is None else mid.to(DEV).contiguous()


RAGGED = next(s for s in BK.TINY_LATENTS if s == (1, 104, 152))      # level-2 planes of 26 x 38 = 988 pixels


@pytest.mark.parametrize("B,H,W,dtype", [(2, 16, 16, torch.float32), (*RAGGED, torch.bfloat16)], ids=["2-16-16-fp32", "1-104-152-bf16"])
def test_unet_forward_with_residuals_matches_the_restatement(tiny, B, H, W, dtype):
    cfg, w, net = tiny
    x = make_inputs(cfg, B, H, W, seed=3)
    sample = (x["lat"] * 2.0).to(torch.bfloat16).float()
    t = torch.tensor([10.0, 500.0][2 - B:])
    res = RR.make_residuals(cfg, B, H, W, dtype=dtype)
    assert [tuple(r.shape) for r in res[0]] + [tuple(res[1].shape)] == (lambda s: s[0] + [s[1]])(net.residual_shapes(B, H, W))
    got = net.unet_forward(sample, t, x["ehs"], x["pooled"], x["tid"], residuals=_dev(res)).cpu()
    ref = RR.unet_forward(w, sample, t, x["ehs"], x["pooled"], x["tid"], cfg, *res)
    ref_bf = RR.unet_forward(w, sample, t, x["ehs"], x["pooled"], x["tid"], cfg, *res, emulate_bf16=True)
    plain = U.unet_forward(w, sample, t, x["ehs"], x["pooled"], x["tid"], cfg)
    e = float((got - ref).abs().max() / ref.abs().max())
    e_bf = float((ref_bf - ref).abs().max() / ref.abs().max())
    moved = float((plain - ref).abs().max() / ref.abs().max())
    bar = max(3.0 * e_bf, 2e-2)
    print(f"[parity] tiny unet fwd + residuals {B}x{H}x{W}: hip vs fp32 restatement {e:.3e} ; bf16-emulating vs fp32 {e_bf:.3e} ; bar {bar:.3e} ; "
          f"the residuals move the prediction by {moved:.3e}")
    assert moved >= 10.0 * bar      # a forward that ignored the residuals could not pass
    assert e <= bar


def _ref_step(w, cfg, method, x, res, B):
    """the fp32 oracle's loss with the residuals as leaves: (loss, [residual gradients ..., mid's])"""
    leaves = [r.float().clone().requires_grad_(True) for r in list(res[0]) + [res[1]]]
    unet_fn = lambda s, t, e, p, ti: RR.unet_forward(w, s, t, e, p, ti, cfg, leaves[:-1], leaves[-1])
    batch = {"vae_latents": x["lat"], "prompt_embeds": x["ehs"], "pooled_prompt_embeds": x["pooled"], "time_ids": x["tid"]}
    if method == "ddpm":
        ts = torch.tensor([700, 420][:B])
        return R.compute_loss_ddpm(unet_fn, batch, x["noise"], ts), leaves, (R.karras_sigmas()[ts], ts.float())
    tf = R.sample_logit_normal_from_z(x["z"])
    return R.compute_loss_flow(unet_fn, batch, x["noise"], tf), leaves, (tf, tf)


def _parity(label, got, ref):
    a, b = got.detach().cpu().double().flatten(), ref.detach().double().flatten()
    rel = float((a - b).norm() / b.norm())
    cos = float(torch.dot(a, b) / (a.norm() * b.norm()))
    print(f"[parity] {label}: rel-L2 {rel:.3e} cos {cos:.6f} |ref| {float(b.norm()):.3e} (bar rel-L2 <= {TINY_GRAD_BAR[0]:.0e}, cos >= {TINY_GRAD_BAR[1]})")
    return rel, cos


@pytest.mark.parametrize("method", ["ddpm", "flow_matching"])
def test_training_step_with_residuals_matches_oracle(tiny, method):
    cfg, w, net = tiny
    B, H, W = 2, 16, 16
    x = make_inputs(cfg, B, H, W, seed=11)
    res = RR.make_residuals(cfg, B, H, W)
    for t in w.values():
        t.grad = None
        t.requires_grad_(True)
    try:
        ref, leaves, (s_or_t, t_in) = _ref_step(w, cfg, method, x, res, B)
        net.forward_loss(method, x["lat"], x["noise"], s_or_t, t_in, x["ehs"], x["pooled"], x["tid"], residuals=_dev(res), residual_grads=True)
        net.zero_grads()
        net.backward(1.0, True)
        got_loss, ref_loss = net.read_loss()[0], float(ref["loss"].detach())
        rel = abs(got_loss - ref_loss) / abs(ref_loss)
        print(f"[parity] tiny {method} + residuals loss: hip {got_loss:.6f} oracle {ref_loss:.6f} rel {rel:.3e} (tol {LOSS_RTOL})")
        assert rel <= LOSS_RTOL
        ref["loss"].backward()
        d_down, d_mid = net.read_residual_grads()
        out = []
        for i, (d, leaf) in enumerate(zip(list(d_down) + [d_mid], leaves)):
            assert d.dtype == torch.float32 and d.is_cuda and tuple(d.shape) == tuple(leaf.shape)
            assert float(leaf.grad.norm()) > 0
            out.append(_parity(f"tiny {method} d residual {'mid' if i == len(leaves) - 1 else i}", d, leaf.grad))
        for k in PROBE_GRADS[::4]:
            out.append(_parity(f"tiny {method} + residuals grad {k}", net.export(k, grad=True), w[k].grad))
        for rel, cos in out:
            assert rel <= TINY_GRAD_BAR[0] and cos >= TINY_GRAD_BAR[1]
    finally:
        for t in w.values():
            t.requires_grad_(False)
            t.grad = None


# ---------------------------------------------------------------------------------------------------------------- 4. semantics
def _step(net, x, residuals=None, residual_grads=None, scale=1.0, first=True, zero=True, on_segment=None):
    """one flow-matching step; (read_loss's values, the gradient arena's bits, [bits of the residual gradients ..., mid's])"""
    tf = R.sample_logit_normal_from_z(x["z"])
    kw = {}
    if residuals is not None:
        kw["residuals"] = residuals
    if residual_grads is not None:
        kw["residual_grads"] = residual_grads
    net.forward_loss("flow_matching", x["lat"], x["noise"], tf, tf, x["ehs"], x["pooled"], x["tid"], **kw)
    if zero:
        net.zero_grads()
    net.backward(scale, first, on_segment=on_segment)
    out = net.read_loss()
    d_down, d_mid = net.read_residual_grads()
    d = None if d_down is None else [_bits(t) for t in list(d_down) + [d_mid]]
    return out, _bits(net.grads), d


def _same(a, b):
    return len(a) == len(b) and all((p is None and q is None) or torch.equal(p, q) for p, q in zip(a, b))


def test_zero_residuals_and_requests_change_no_bit(tiny):
    cfg, _, net = tiny
    B, H, W = 2, 16, 16
    x = make_inputs(cfg, B, H, W, seed=21)
    res = _dev(RR.make_residuals(cfg, B, H, W))
    zeros = ([torch.zeros_like(t) for t in res[0]], torch.zeros_like(res[1]))
    out0, g0, d0 = _step(net, x)
    assert d0 is None
    out1, g1, d1 = _step(net, x, zeros, True)      # zero residuals: the step without the struct, bit for bit
    assert out1 == out0 and torch.equal(g1, g0)
    out2, g2, d2 = _step(net, x, None, True)       # d_* without residuals: the gradient at r = 0
    assert out2 == out0 and torch.equal(g2, g0) and _same(d2, d1)
    assert all(int(t.ne(0).sum()) > 0 for t in d1)
    # with residuals: a request changes no bit of the step, a subset of pointers gives the bits of the full request, two runs the same bits
    outr, gr, _ = _step(net, x, res)
    assert outr != out0
    outa, ga, da = _step(net, x, res, True)
    outb, gb, db = _step(net, x, res, [1, 6, "mid"])
    assert outa == outr and torch.equal(ga, gr) and outb == outr and torch.equal(gb, gr)
    assert [i for i, t in enumerate(db) if t is not None] == [1, 6, 9] and all(torch.equal(db[i], da[i]) for i in (1, 6, 9))
    _, gc, dc = _step(net, x, res, True)
    assert torch.equal(gc, ga) and _same(dc, da)
    # per-segment backward (the exchange's path) gives backward_all's bits
    _, gs, ds = _step(net, x, res, True, on_segment=lambda k, off, n: None)
    assert torch.equal(gs, ga) and _same(ds, da)
    # a partial residual list (None entries, no mid) is accepted
    part = ([t if i in (0, 4) else None for i, t in enumerate(res[0])], None)
    outp, _, dp = _step(net, x, part, True)
    assert outp != out0 and outp != outr and all(t is not None for t in dp)


def test_grad_scale_overwrite_and_frozen_unet(tiny):
    """grad_scale 0.5: dpred is gate * grad_scale * (...) in fp32, rounded once to bf16; 0.5 is a power of two, so the product and its
    rounding scale exactly (no value here is near the subnormal range), and so does every later product, fp32 sum and bf16 rounding of
    the linear backward: each element is at most one bf16 ulp from half the unscaled one -- in fact its exact half, which is asserted
    as the number of elements that are not."""
    cfg, _, net = tiny
    B, H, W = 2, 16, 16
    x, y = make_inputs(cfg, B, H, W, seed=22), make_inputs(cfg, B, H, W, seed=23)
    res = _dev(RR.make_residuals(cfg, B, H, W))
    _, _, d1 = _step(net, x, res, True)
    _, _, dh = _step(net, x, res, True, scale=0.5)
    for i, (a, h) in enumerate(zip(d1, dh)):
        a, h = a.view(torch.float32), h.view(torch.float32)
        ulp = torch.exp2(torch.floor(torch.log2((0.5 * a).abs().clamp_min(1e-30))) - 7)      # one bf16 ulp (8 significant bits) of the exact half
        off = int((h - 0.5 * a).abs().gt(ulp).sum())
        inexact = int((h != 0.5 * a).sum())
        print(f"[scale] residual {i}: {off} of {a.numel()} elements beyond one bf16 ulp of half, {inexact} not the exact half")
        assert off == 0 and inexact == 0
    # the second micro-step of a cycle overwrites: the bits of the same batch run alone
    _, _, dy = _step(net, y, res, True)
    _step(net, x, res, True)
    _, _, dy2 = _step(net, y, res, True, first=False, zero=False)
    assert _same(dy2, dy)
    # everything frozen (ControlNet training on a frozen UNet): the residual gradients keep their bits
    net.set_trainable([])
    try:
        _, _, df = _step(net, y, res, True)
    finally:
        net.set_trainable(None)
    assert _same(df, dy)


def test_graph_mode_launches_a_residual_call_kernel_by_kernel_with_the_same_bits(tiny):
    cfg, _, net = tiny
    B, H, W = 2, 16, 16
    x = make_inputs(cfg, B, H, W, seed=24)
    res = _dev(RR.make_residuals(cfg, B, H, W))
    out0, g0, d0 = _step(net, x, res, True)
    outp, gp, _ = _step(net, x)
    net.set_graph_mode(True)
    try:
        for i in range(3):      # (a plain call: eager, capture, replay; the residual call between them never captures)
            out, g, d = _step(net, x, res, True)
            assert out == out0 and torch.equal(g, g0) and _same(d, d0), i
            out, g, _ = _step(net, x)
            assert out == outp and torch.equal(g, gp), i
    finally:
        net.set_graph_mode(False)


def test_unet_backward_gives_the_gradients_of_dpred_dot_pred(tiny):
    cfg, w, net = tiny
    B, H, W = 2, 16, 16
    x = make_inputs(cfg, B, H, W, seed=25)
    res = RR.make_residuals(cfg, B, H, W)
    sample = (x["lat"] * 2.0).to(torch.bfloat16).float()
    t = torch.tensor([10.0, 500.0])
    dpred = torch.randn(B, 4, H, W, generator=torch.Generator().manual_seed(26)).to(torch.bfloat16).float()
    net.unet_forward(sample, t, x["ehs"], x["pooled"], x["tid"], residuals=_dev(res), residual_grads=True)
    net.zero_grads()
    net.unet_backward(dpred, True)
    d_down, d_mid = net.read_residual_grads()
    leaves = [r.clone().requires_grad_(True) for r in list(res[0]) + [res[1]]]
    pred = RR.unet_forward(w, sample, t, x["ehs"], x["pooled"], x["tid"], cfg, leaves[:-1], leaves[-1])
    (dpred * pred).sum().backward()
    for i, (d, leaf) in enumerate(zip(list(d_down) + [d_mid], leaves)):
        rel, cos = _parity(f"unet_backward d residual {i}", d, leaf.grad)
        assert rel <= TINY_GRAD_BAR[0] and cos >= TINY_GRAD_BAR[1]


def test_bad_arguments_are_refused_before_any_launch(tiny):
    cfg, _, net = tiny
    B, H, W = 2, 16, 16
    L = lib.load()
    x = make_inputs(cfg, B, H, W, seed=27)
    _step(net, x)      # plans (2, 16, 16) and leaves a valid step behind
    res = _dev(RR.make_residuals(cfg, B, H, W))
    shapes, mid_shape = net.residual_shapes(B, H, W)
    n = len(shapes)
    d = [torch.empty(s, device=DEV) for s in shapes]
    keep = [t.to(DEV) for t in (x["lat"], x["noise"], torch.tensor([0.3, 0.6]), x["ehs"].to(torch.bfloat16), x["pooled"].to(torch.bfloat16), x["tid"])]
    lat, noise, tt, ehs, pooled, tid = keep
    arena_before = _bits(net.grads)

    def call(r, sampler=None):
        b = lib.ResidualBatch(B, H, W, 77 | lib.BATCH_RES, lat.data_ptr(), noise.data_ptr(), tt.data_ptr(), tt.data_ptr(), ehs.data_ptr(),
                              pooled.data_ptr(), tid.data_ptr(), None)
        b.residuals = C.pointer(r)
        if sampler is not None:
            b.sampler = C.pointer(sampler)
            rc = L.sdxl_unet_forward(net.h, None, C.byref(b), None, _st())
        else:
            lc = lib.LossConfig(1, 1, 0, 0.0, 0)
            rc = L.sdxl_forward_loss(net.h, C.byref(lc), C.byref(b), _st())
        return rc, L.sdxl_last_error().decode()

    arr = lambda ts, bump=None: (C.c_void_p * n)(*[t.data_ptr() + (4 if i == bump else 0) for i, t in enumerate(ts)])
    rc, msg = call(lib.Residuals(n - 1, 0, arr(res[0]), None, None, None))
    assert rc == 1 and "residuals" in msg and f"n = {n - 1}" in msg
    rc, msg = call(lib.Residuals(n, 2, arr(res[0]), None, None, None))
    assert rc == 1 and "residuals" in msg and "dtype 2" in msg
    rc, msg = call(lib.Residuals(n, 0, arr(res[0], bump=3), None, None, None))
    assert rc == 1 and "residuals" in msg and "down[3]" in msg
    rc, msg = call(lib.Residuals(n, 0, None, None, arr(d, bump=7), None))
    assert rc == 1 and "residuals" in msg and "d_down[7]" in msg
    rc, msg = call(lib.Residuals(n, 0, None, res[1].data_ptr() + 4, None, None))
    assert rc == 1 and "residuals" in msg and "mid" in msg
    xs = torch.zeros(B, 4, H, W, device=DEV)
    step = lib.SamplerStep(xs.data_ptr(), 0, 0, 1.0, -1.0, 0.5, 0.5, 1.0, 0.0, 1.0, 0.0)
    rc, msg = call(lib.Residuals(n, 0, None, None, arr(d), None), sampler=step)
    assert rc == 1 and "residuals" in msg and "d_down[0]" in msg and "sampler" in msg
    rc, msg = call(lib.Residuals(n, 0, None, None, None, d[-1].data_ptr()), sampler=step)
    assert rc == 1 and "residuals" in msg and "d_mid" in msg and "sampler" in msg
    torch.cuda.synchronize()
    assert int(xs.ne(0).sum()) == 0 and torch.equal(_bits(net.grads), arena_before)      # nothing ran
    # the host checks name the index
    bad = list(res[0])
    bad[5] = bad[5][:, :, :-1].contiguous()
    with pytest.raises(ValueError, match=r"down\[5\]"):
        _step(net, x, (bad, None))
    # a list of nothing but None behind the flag is a call without residuals, bit for bit
    out0, g0, _ = _step(net, x)
    out1, g1, _ = _step(net, x, ([None] * n, None))
    assert out1 == out0 and torch.equal(g1, g0)


# ---------------------------------------------------------------------------------------------------------------- 5. sampler
def test_one_guided_sampler_step_with_residuals(tiny):
    """One cfg Euler step.  (a) The existing sampler bar: the state has the bits of tests/_sampler_ref.py's step driven by the native
    forward with the same residuals.  (b) Against the same restatement driven by the oracle (tests/_residual_ref.py): the step is linear
    in the prediction F, x' = (p + q a_skip) x + q a_out F with F = F_u + g (F_c - F_u), so an error of e_F (max-abs) in each prediction
    moves the state by at most |q a_out| (|g| + |g - 1|) e_F, and e_F is held to the forward bar max(3 e_bf, 2e-2) max|F|."""
    cfg, w, net = tiny
    B, H, W, gs = 2, 16, 16, 5.0
    g = torch.Generator().manual_seed(41)
    pe, po = torch.randn(B, 77, cfg.cross_attention_dim, generator=g).to(torch.bfloat16), torch.randn(B, cfg.pooled_dim, generator=g).to(torch.bfloat16)
    ti = torch.tensor([[8.0 * W, 8.0 * H, 0, 0, 8.0 * W, 8.0 * H]] * B)
    noise = torch.randn(B, 4, H, W, generator=g)
    res = RR.make_residuals(cfg, 2 * B, H, W)      # the plan's batch: rows b + B feed the unconditional half
    seen = []

    def control(sample, t, batch):
        seen.append((tuple(sample.shape), tuple(t.shape), sample.detach().cpu().clone()))
        return _dev(res)

    sampler = S.NativeSampler(net, "flow_matching", "v_prediction", True, "trained", control=control)
    x0_scale, steps = sampler.schedule(1)
    got = sampler.sample(pe, po, ti, height=H, width=W, num_steps=1, guidance_scale=gs, noise=noise).cpu()
    assert len(seen) == 1 and seen[0][0] == (2 * B, 4, H, W) and seen[0][1] == (2 * B,)
    pe2, po2, ti2 = torch.cat([pe, torch.zeros_like(pe)]), torch.cat([po, torch.zeros_like(po)]), torch.cat([ti, ti])
    x = noise if x0_scale == 1.0 else SR._s(x0_scale, noise) * noise
    inp = SR.unet_input(x, steps[0][0], steps[0][5])
    assert torch.equal(seen[0][2][:B], SR.unet_input(x, steps[0][0], steps[0][5], quantize=False)) and torch.equal(seen[0][2][B:], seen[0][2][:B])
    a_in, a_skip, a_out, p, q, _c, t = steps[0]
    tt = torch.full((2 * B,), t)
    f_native = net.unet_forward(torch.cat([inp, inp]), tt, pe2, po2, ti2, residuals=_dev(res)).cpu()
    want = SR.step(x, SR.guide(f_native[:B], f_native[B:], gs), a_skip, a_out, p, q)
    assert torch.equal(_bits(got), _bits(want))
    args = (w, torch.cat([inp, inp]), tt, pe2.float(), po2.float(), ti2, cfg, *res)
    f_ref, f_bf = RR.unet_forward(*args), RR.unet_forward(*args, emulate_bf16=True)
    e_bf = float((f_bf - f_ref).abs().max() / f_ref.abs().max())
    bound = abs(q * a_out) * (abs(gs) + abs(gs - 1.0)) * max(3.0 * e_bf, 2e-2) * float(f_ref.abs().max())
    ref = SR.step(x, SR.guide(f_ref[:B], f_ref[B:], gs), a_skip, a_out, p, q)
    err = float((got - ref).abs().max())
    print(f"[sampler] one guided step with residuals: max |x - oracle| {err:.3e}, bound {bound:.3e} (e_bf {e_bf:.3e})")
    assert err <= bound
    plain = S.NativeSampler(net, "flow_matching", "v_prediction", True, "trained").sample(pe, po, ti, height=H, width=W, num_steps=1, guidance_scale=gs, noise=noise).cpu()
    assert float((plain - got).abs().max()) > 0


# ---------------------------------------------------------------------------------------------------------------- 6. trainer
class TinyControl(torch.nn.Module):
    """a 1 x 1 convolution of the (pooled) UNet input per residual: the smallest module that reaches every skip and the mid output"""

    def __init__(self, shapes, mid_shape):
        super().__init__()
        self.shapes = list(shapes) + [mid_shape]
        g = torch.Generator().manual_seed(51)
        self.convs = torch.nn.ModuleList(torch.nn.Conv2d(4, s[1], 1) for s in self.shapes)
        for c in self.convs:
            with torch.no_grad():
                c.weight.copy_(0.1 * torch.randn(c.weight.shape, generator=g))
                c.bias.copy_(0.05 * torch.randn(c.bias.shape, generator=g))

    def forward(self, sample, timestep, batch):
        H = sample.shape[2]
        outs = [conv(torch.nn.functional.avg_pool2d(sample, H // s[2]) if s[2] != H else sample) for conv, s in zip(self.convs, self.shapes)]
        return outs[:-1], outs[-1]


def test_a_torch_control_module_trains_through_the_trainers_loss(tiny):
    cfg, w, net = tiny
    cfgm = importlib.import_module("sdxl-training-improvements_amd.config")
    TR = importlib.import_module("sdxl-training-improvements_amd.trainer")
    B, H, W = 2, 16, 16
    x = make_inputs(cfg, B, H, W, seed=52)
    noise = torch.randn(B, 4, H, W, generator=torch.Generator().manual_seed(53))
    t = torch.tensor([0.21, 0.83])

    class M:
        unet = net

    c = cfgm.Config()
    c.training.method = "flow_matching"
    c.training.mixed_precision = "no"
    ctl = TinyControl(*net.residual_shapes(B, H, W)).to(DEV)
    tr = TR.NativeSDXLTrainer(M(), config=c, control=ctl)
    batch = {"vae_latents": x["lat"], "prompt_embeds": x["ehs"], "pooled_prompt_embeds": x["pooled"], "time_ids": x["tid"], "metadata": {}}
    tr.zero_grad()
    out = tr.compute_loss(batch, timesteps=t, noise=noise, generator=torch.Generator().manual_seed(54))
    out["loss"].backward()
    torch.cuda.synchronize()
    # the same module in front of the oracle
    ref_ctl = TinyControl(*net.residual_shapes(B, H, W))
    xt = R.optimal_transport_path(noise, x["lat"], t)
    down, mid = ref_ctl(xt, t, batch)
    b0 = {k: v for k, v in batch.items() if k != "metadata"}
    ref = R.compute_loss_flow(lambda s, tt, e, p, ti: RR.unet_forward(w, s, tt, e, p, ti, cfg, down, mid), b0, noise, t)
    ref["loss"].backward()
    rel = abs(float(out["loss"]) - float(ref["loss"])) / abs(float(ref["loss"]))
    print(f"[trainer] control loss: hip {float(out['loss']):.6f} oracle {float(ref['loss']):.6f} rel {rel:.3e}")
    assert rel <= LOSS_RTOL
    for (name, p_), (_n, q_) in zip(ctl.named_parameters(), ref_ctl.named_parameters()):
        assert p_.grad is not None, name
        r_, cos = _parity(f"control {name}", p_.grad, q_.grad)
        assert r_ <= TINY_GRAD_BAR[0] and cos >= TINY_GRAD_BAR[1]
    # evaluate: control runs under no_grad and nothing is requested
    for p_ in ctl.parameters():
        p_.grad = None
    tr.evaluate([batch], [0.5], generator=torch.Generator().manual_seed(55))
    assert net.read_residual_grads() == (None, None) and all(p_.grad is None for p_ in ctl.parameters())
