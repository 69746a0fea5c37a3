"""Extra UNet input channels (in_channels 5 .. 16: inpainting 9, image conditioning 8) on a real MI355X.

Op level: the loss preparation through sdxl_op_loss phase 0 -- channels 0..3 keep the bits of the 4-channel run, channels 4.. are
bf16(input_cond), the pad channels are all-zero bits, nothing else is written.  Model level: the whole step of a 9- and an 8-channel
tiny UNet against autograd of the oracle on cat(sample, input_cond), at the tolerances tests/test_gpu_model.py applies to the 4-channel
tiny UNet.  Then unet_forward, graph mode, the sampler, the trainer keys and the refusals."""
import ctypes as C
import dataclasses
import importlib

import pytest
import torch

import _sampler_ref as R
import _sampler_solver_ref as X
import sdxl_amd  # noqa: F401
from oracle import loss_ref as LR
from oracle import unet_ref as U
from sdxl_amd import lib
from sdxl_amd import unet as NU

import _bucket_cases as BK
from _gradparity import GradParity, compare_autograd
from _isolation import Spec, assert_isolated, param_mask, run_isolated, same_bits
from _optim_common import bits
from test_gpu_model import LOSS_RTOL, TINY_GRAD_BAR, make_inputs

S = importlib.import_module("sdxl-training-improvements_amd.sampler")
T = importlib.import_module("sdxl-training-improvements_amd.trainer")
CFG = importlib.import_module("sdxl-training-improvements_amd.config")

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF, F32 = torch.bfloat16, torch.float32
RAGGED = BK.TINY_LATENTS[2]          # (1, 104, 152): 988 / 3952 tokens, pad rows everywhere
assert RAGGED[0] == 1 and (RAGGED[1] * RAGGED[2]) % 256 != 0


def st():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def native_cfg(c: U.UNetConfig):
    return NU.make_config(in_channels=c.in_channels, block_out_channels=c.block_out_channels,
                          transformer_layers=c.transformer_layers_per_block, cross_attention_dim=c.cross_attention_dim,
                          addition_time_embed_dim=c.addition_time_embed_dim, pooled_dim=c.pooled_dim)


def make_cond(B, n, H, W, seed):
    return torch.randn(B, n, H, W, generator=torch.Generator().manual_seed(seed))


def _tiny(c):
    cfg = dataclasses.replace(U.tiny_config(), in_channels=c)
    w = U.synth_weights(cfg, seed=0)
    net = NU.NativeUNet(native_cfg(cfg))
    net.load_state_dict(w)
    return cfg, w, net


@pytest.fixture(scope="module")
def tiny9():
    cfg, w, net = _tiny(9)
    yield cfg, w, net
    net.close()


@pytest.fixture(scope="module")
def tiny8():
    cfg, w, net = _tiny(8)
    yield cfg, w, net
    net.close()


@pytest.fixture(scope="module")
def tiny4():
    cfg, w, net = _tiny(4)
    yield cfg, w, net
    net.close()


# ---------------------------------------------------------------------------------------------- 1. the preparation kernel
def _prepare(L, method, lat, noise, sig, cond, unet_in_ptr):
    """sdxl_op_loss phase 0 on device tensors; cond None: the 4-channel call (the short struct, no flag)"""
    B, _c, H, W = lat.shape
    lc = lib.LossConfig(method, 1, 1, 5.0, 1)
    fields = (B, H, W, 77, lat.data_ptr(), noise.data_ptr(), sig.data_ptr(), None, None, None, None, None)
    if cond is None:
        b = lib.Batch(*fields)
    else:
        b = lib.InputCondBatch(*fields)
        b.ctx_len |= lib.BATCH_COND
        b.input_cond, b.cond_channels = cond.data_ptr(), int(cond.shape[1])
    lib.check(L.sdxl_op_loss(C.byref(lc), C.byref(b), C.c_void_p(unet_in_ptr), None, None, 1.0, None, 0, st()), "sdxl_op_loss phase 0")
    torch.cuda.synchronize()


def _prep_inputs(method, n, B=2, H=5, W=7):
    g = torch.Generator().manual_seed(100 * method + n)
    lat, noise = torch.randn(B, 4, H, W, generator=g), torch.randn(B, 4, H, W, generator=g)
    sig = LR.karras_sigmas()[torch.tensor([100, 850])] if method == 0 else torch.sigmoid(torch.randn(B, generator=g))
    cond = torch.randn(B, n, H, W, generator=g) * 3.0
    cond[0, 0, 0, :4] = torch.tensor([0.0, -0.0, 1.00390625, 3.3895314e38])      # signed zero, a round-to-even tie, the largest bf16
    return lat, noise, sig.float(), cond


def _check_image(img, base8, cond, n):
    """img [rows][Cs] bf16 against the 4-channel run's [rows][8] and input_cond [B,n,H,W]"""
    B, _n, H, W = cond.shape
    cs = 8 if 4 + n <= 8 else 16
    assert tuple(img.shape) == (B * H * W, cs)
    assert same_bits(img[:, :4].contiguous(), base8[:, :4].contiguous()), "channels 0..3 differ from the in_channels = 4 run"
    want = cond.permute(0, 2, 3, 1).reshape(B * H * W, n).to(BF)
    assert same_bits(img[:, 4:4 + n].contiguous(), want.contiguous()), "channels 4.. are not bf16(input_cond)"
    if 4 + n < cs:
        assert int((bits(img[:, 4 + n:].contiguous()) != 0).sum()) == 0, "pad channels are not all-zero bits"


@pytest.mark.parametrize("method", [0, 1], ids=["ddpm", "flow_matching"])
@pytest.mark.parametrize("n", [1, 4, 5, 12])
def test_prepare_kernel_channels(n, method):
    L = lib.load()
    lat, noise, sig, cond = _prep_inputs(method, n)
    B, _c, H, W = lat.shape
    d = [t.to(DEV).contiguous() for t in (lat, noise, sig, cond)]
    base = torch.full((B * H * W, 8), float("nan"), dtype=BF, device=DEV)
    _prepare(L, method, d[0], d[1], d[2], None, base.data_ptr())
    assert int((bits(base[:, 4:].contiguous()) != 0).sum()) == 0
    cs = 8 if 4 + n <= 8 else 16
    img = torch.full((B * H * W, cs), float("nan"), dtype=BF, device=DEV)      # every element must be written
    _prepare(L, method, d[0], d[1], d[2], d[3], img.data_ptr())
    _check_image(img.cpu(), base.cpu(), cond, n)


@pytest.mark.parametrize("method", [0, 1], ids=["ddpm", "flow_matching"])
def test_prepare_kernel_isolated(method):
    """n = 5 (two 16-byte stores per pixel) between guard bands of 0x00 / 0xFF / 0x7F: same bits, guards and inputs untouched"""
    L = lib.load()
    n = 5
    lat, noise, sig, cond = _prep_inputs(method, n)
    B, _c, H, W = lat.shape
    specs = [Spec("lat", B * 4, H * W, None, F32, lat.reshape(B * 4, H * W)), Spec("noise", B * 4, H * W, None, F32, noise.reshape(B * 4, H * W)),
             Spec("sig", 1, B, None, F32, sig.reshape(1, B)), Spec("cond", B * n, H * W, None, F32, cond.reshape(B * n, H * W)),
             Spec("unet_in", B * H * W, 16, None, BF, None, "out")]

    def fn(ar):
        lc = lib.LossConfig(method, 1, 1, 5.0, 1)
        b = lib.InputCondBatch(B, H, W, 77 | lib.BATCH_COND, ar.ptr("lat"), ar.ptr("noise"), ar.ptr("sig"), None, None, None, None, None)
        b.input_cond, b.cond_channels = ar.ptr("cond"), n
        lib.check(L.sdxl_op_loss(C.byref(lc), C.byref(b), C.c_void_p(ar.ptr("unet_in")), None, None, 1.0, None, 0, st()))
        torch.cuda.synchronize()
    runs = run_isolated(fn, specs, device=DEV)
    assert_isolated(runs, what=f"prepare n=5 method {method}")
    d = [t.to(DEV).contiguous() for t in (lat, noise, sig)]
    base = torch.full((B * H * W, 8), float("nan"), dtype=BF, device=DEV)
    _prepare(L, method, d[0], d[1], d[2], None, base.data_ptr())
    # (the largest bf16 is finite: assert_isolated's finiteness holds)
    _check_image(runs[0]["unet_in"].cpu(), base.cpu(), cond, n)


# ---------------------------------------------------------------------------------------------- 1b. conv_in at Cin = 16
@pytest.mark.parametrize("B,H,W", [(1, 12, 20), (2, 5, 7), (1, 128, 128)])
def test_conv_in_16_wide_on_the_routes_of_the_8_wide(B, H, W):
    """the 16-wide conv_in (in_channels 9 .. 16) through the op entry points: forward on the general gather (reduction 16, no multiple of
    64), weight gradient on the 128-row kernel and, from 16 384 pixels, on the three-tap kernel -- the routes Cin = 8 takes, at the bars
    tests/test_gpu_ops.py holds Cin = 8 to"""
    import math
    import test_gpu_ops as OPS
    L = lib.load()
    Cin, Cout = 16, 320
    M = B * H * W
    for cin in (8, Cin):
        fwd = lib.gemm_route(form=0, taps=9, M=M, N=Cout, K=cin, Hm=H, Wm=W, Hs=H, Ws=W)
        wg = lib.gemm_route(form=2, taps=9, M=Cout, N=cin, K=M, Hm=H, Wm=W, Hs=H, Ws=W, bias_grad=1)
        assert fwd["kernel"] == "128-row" and not fwd["fast"]
        assert wg["kernel"] == ("conv_wgrad3" if M >= 16384 else "128-row")
    x, w, bias = OPS.rnd(B, H, W, Cin, seed=10), OPS.rnd(Cout, 9, Cin, seed=11, scale=0.05), OPS.rnd(Cout, seed=12)
    x[..., 9:] = 0.0                                               # as the plan holds it: the pad channels zero
    y = torch.empty(B, H, W, Cout, dtype=BF, device=DEV)
    lib.check(L.sdxl_op_conv3x3_fwd(OPS.ptr(x), OPS.ptr(w), OPS.ptr(bias), OPS.ptr(y), B, H, W, Cin, Cout, 1, st()))
    wr = w.float().requires_grad_(True)
    ref = OPS._conv_ref(x.float(), wr, bias, 1)
    OPS.report(f"conv fwd {B}x{H}x{W} {Cin}->{Cout}", y, ref.detach(), 6e-3)
    dy = OPS.rnd(B, H, W, Cout, seed=13)
    ref.backward(dy.float())
    dw = torch.full((Cout, 9, Cin), 5.0, dtype=F32, device=DEV)
    db = torch.zeros(Cout, dtype=F32, device=DEV)
    lib.check(L.sdxl_op_conv3x3_wgrad2(OPS.ptr(x), OPS.ptr(dy), OPS.ptr(dw), OPS.ptr(db), B, H, W, Cin, Cout, 1, 0, 0, st()))
    OPS.report(f"conv wgrad {B}x{H}x{W} {Cin}->{Cout}", dw, wr.grad, 1e-4 * math.sqrt(M) / 8 + 1e-5)
    OPS.report("conv bias grad", db, dy.float().sum((0, 1, 2)), 1e-4)
    assert float(dw[:, :, 9:].abs().max()) == 0.0                 # zero input channels: an exact zero weight gradient in the pad columns


# ---------------------------------------------------------------------------------------------- 2. the whole step against the oracle
def _step_case(cfg, w, net, method, B, H, W, seed):
    """(reference dict, enqueue-forward callable) of one step with input_cond"""
    c = cfg.in_channels
    x = make_inputs(cfg, B, H, W, seed=seed)
    ic = make_cond(B, c - 4, H, W, seed + 1)
    unet_fn = lambda s, t, e, p, ti: U.unet_forward(w, torch.cat([s, ic], dim=1), t, e, p, ti, cfg)
    batch = {"vae_latents": x["lat"], "prompt_embeds": x["ehs"], "pooled_prompt_embeds": x["pooled"], "time_ids": x["tid"]}
    if method == "ddpm":
        ts = torch.tensor([610, 230][:B])
        sig = LR.karras_sigmas()[ts]
        ref = lambda: LR.compute_loss_ddpm(unet_fn, batch, x["noise"], ts)
        step = lambda cond=ic: net.forward_loss("ddpm", x["lat"], x["noise"], sig, ts.float(), x["ehs"], x["pooled"], x["tid"], input_cond=cond)
    else:
        tf = LR.sample_logit_normal_from_z(x["z"])
        ref = lambda: LR.compute_loss_flow(unet_fn, batch, x["noise"], tf)
        step = lambda cond=ic: net.forward_loss("flow_matching", x["lat"], x["noise"], tf, tf, x["ehs"], x["pooled"], x["tid"], input_cond=cond)
    return ref, step, ic


def _run_parity(tiny, method, B, H, W):
    cfg, w, net = tiny
    c = cfg.in_channels
    shapes = net.param_shapes()
    assert shapes["conv_in.weight"] == (64, c, 3, 3) and shapes == {k: tuple(v) for k, v in U.param_shapes(cfg).items()}
    assert torch.equal(net.export("conv_in.weight").cpu(), w["conv_in.weight"]), "conv_in.weight: load -> export is not bit-exact"
    for t in w.values():
        t.grad = None
        t.requires_grad_(True)
    ref_fn, step, _ic = _step_case(cfg, w, net, method, B, H, W, seed=13 if method == "ddpm" else 17)
    ref = ref_fn()
    step()
    net.zero_grads()
    net.backward(grad_scale=1.0, first_micro=True)
    ref_loss, got_loss = float(ref["loss"].detach()), net.read_loss()[0]
    print(f"[parity] tiny c={c} {method} {B}x{H}x{W} loss: hip {got_loss:.6f} oracle {ref_loss:.6f} rel {abs(got_loss - ref_loss) / abs(ref_loss):.3e} (tol {LOSS_RTOL})")
    assert abs(got_loss - ref_loss) <= LOSS_RTOL * abs(ref_loss)
    par = GradParity(f"tiny c={c} {method} {B}x{H}x{W}")
    try:
        compare_autograd(par, ref["loss"], w, lambda k: net.export(k, grad=True))
    finally:
        for t in w.values():
            t.grad = None
            t.requires_grad_(False)
    par.check(TINY_GRAD_BAR, expect=shapes)
    assert par.rows["conv_in.weight"].numel == 64 * c * 9 and par.rows["conv_in.weight"].r > 0
    if (B, H, W) == (2, 16, 16):      # the repeated step: the same bits in the whole gradient arena
        torch.cuda.synchronize()
        first = net.grads.clone()
        step()
        net.zero_grads()
        net.backward(grad_scale=1.0, first_micro=True)
        torch.cuda.synchronize()
        assert net.read_loss()[0] == got_loss
        assert torch.equal(net.grads.view(torch.int32), first.view(torch.int32)), "the repeated step's gradient arena differs"


CASES = [pytest.param(m, *s, id=f"{m}-{s[0]}-{s[1]}-{s[2]}") for m in ("ddpm", "flow_matching") for s in ((2, 16, 16), RAGGED)]


@pytest.mark.parametrize("method,B,H,W", CASES)
def test_step_matches_oracle_9_channels(tiny9, method, B, H, W):
    _run_parity(tiny9, method, B, H, W)


@pytest.mark.parametrize("method,B,H,W", CASES)
def test_step_matches_oracle_8_channels(tiny8, method, B, H, W):
    _run_parity(tiny8, method, B, H, W)


def test_unet_forward_matches_oracle_9_channels(tiny9):
    """the bar of tests/test_gpu_model.py::test_unet_forward_matches_oracle, on a [B,9,H,W] sample packed into 16 columns"""
    cfg, w, net = tiny9
    B, H, W = 2, 24, 40
    x = make_inputs(cfg, B, H, W, seed=3)
    sample = torch.cat([x["lat"] * 2.0, make_cond(B, 5, H, W, 4)], dim=1).to(BF).float()
    t = torch.tensor([10.0, 500.0])
    got = net.unet_forward(sample, t, x["ehs"], x["pooled"], x["tid"]).cpu()
    ref = U.unet_forward(w, sample, t, x["ehs"], x["pooled"], x["tid"], cfg)
    ref_bf = U.unet_forward(w, sample, t, x["ehs"], x["pooled"], x["tid"], cfg, emulate_bf16=True)
    e = float((got - ref).abs().max() / ref.abs().max())
    e_bf = float((ref_bf - ref).abs().max() / ref.abs().max())
    print(f"[parity] tiny c=9 unet fwd {B}x{H}x{W}: hip vs fp32 oracle {e:.3e} ; bf16-emulating oracle vs fp32 oracle {e_bf:.3e}")
    assert e <= max(3.0 * e_bf, 2e-2)
    other = sample.clone()
    other[:, 4:] = 0.0
    assert not torch.equal(net.unet_forward(other, t, x["ehs"], x["pooled"], x["tid"]).cpu(), got)      # the extra channels are read
    with pytest.raises(ValueError, match="in_channels"):
        net.unet_forward(sample[:, :4], t, x["ehs"], x["pooled"], x["tid"])


# ---------------------------------------------------------------------------------------------- 3. graph mode
def test_graph_mode_stages_input_cond(tiny9):
    """eager, captured and replayed steps whose input_cond lives in a different buffer each step: the bits of the eager launches"""
    cfg, w, net = tiny9
    B, H, W = 2, 16, 24
    ts = torch.tensor([250, 770])
    sig = LR.karras_sigmas()[ts]
    xs = [make_inputs(cfg, B, H, W, seed=50 + i) for i in range(3)]
    ics = [make_cond(B, 5, H, W, 60 + i) for i in range(3)]
    mask = param_mask(net)

    def run():
        out, keep = [], []
        for x, ic in zip(xs, ics):
            buf = ic.to(DEV).clone()      # (kept: the next step's copy gets another address)
            keep.append(buf)
            net.zero_grads()
            net.forward_loss("ddpm", x["lat"].clone(), x["noise"].clone(), sig.clone(), ts.float(), x["ehs"], x["pooled"], x["tid"], input_cond=buf)
            net.backward(1.0, True)
            loss = net.read_loss()[0]
            out.append((loss, net.grads[mask].clone()))
        assert len({k.data_ptr() for k in keep}) == len(keep)
        return out
    net.set_graph_mode(False)
    eager = run()
    try:
        net.set_graph_mode(True)
        graphed = run()
    finally:
        net.set_graph_mode(False)
    for i, ((le, ge), (lg, gg)) in enumerate(zip(eager, graphed)):
        assert le == lg, f"step {i}: loss {lg} vs eager {le}"
        assert same_bits(gg, ge), f"step {i}: {int((bits(gg) != bits(ge)).sum())} gradient elements differ from the eager step"
    assert len({l for l, _ in graphed}) == len(xs)


# ---------------------------------------------------------------------------------------------- 4. the sampler
def _cond(B, cfg, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)
    return (r(B, 77, cfg.cross_attention_dim).to(BF), r(B, cfg.pooled_dim).to(BF),
            torch.tensor([[8.0 * W, 8.0 * H, 0, 0, 8.0 * W, 8.0 * H]] * B), r(B, 4, H, W))


def _python_loop(net, sampler, pe, po, ti, noise, num_steps, g_scale, solver, ic, nic):
    """the sampler as a Python loop: unet_forward on the concatenated [cond; uncond] sample, the restated step between the calls"""
    B = pe.shape[0]
    pe2, po2, ti2 = torch.cat([pe, torch.zeros_like(pe)]), torch.cat([po, torch.zeros_like(po)]), torch.cat([ti, ti])
    extra = torch.cat([ic, ic if nic is None else nic])

    def model(inp, t, _j):
        out = net.unet_forward(torch.cat([torch.cat([inp, inp]), extra], dim=1), torch.full((2 * B,), t), pe2, po2, ti2).cpu()
        return out[:B], out[B:]
    x0_scale, steps = sampler.schedule(num_steps)
    if solver == "euler":
        return R.sample_loop(model, noise, x0_scale, steps, g_scale, 0.0)
    lv, _ts = sampler.grid(num_steps)
    ks, tin, _levels = S.solver_steps(steps, lv, sampler.method, solver, 1.0, g_scale, 0.0, True, False)
    x = noise if x0_scale == 1.0 else torch.tensor(x0_scale, dtype=F32) * noise
    return X.solver_loop(model, x, (steps[0][0], steps[0][5]), ks, tin, True)


@pytest.mark.parametrize("c,solver", [(9, "euler"), (9, "dpmpp_2m"), (8, "euler")])
def test_sampler_equals_python_loop(request, c, solver):
    cfg, w, net = request.getfixturevalue(f"tiny{c}")
    B, H, W = 2, 16, 16
    pe, po, ti, noise = _cond(B, cfg, H, W, 11)
    ic, nic = make_cond(B, c - 4, H, W, 12), make_cond(B, c - 4, H, W, 13)
    sampler = S.NativeSampler(net, "ddpm", "v_prediction", True, "trained")
    kw = dict(height=H, width=W, num_steps=3, guidance_scale=2.0, noise=noise, solver=solver)
    results = {}
    for name, neg in (("reused", None), ("neg", nic)):
        want = _python_loop(net, sampler, pe, po, ti, noise, 3, 2.0, solver, ic, neg)
        got = sampler.sample(pe, po, ti, input_cond=ic, neg_input_cond=neg, **kw)
        torch.cuda.synchronize()
        assert got.dtype == F32 and got.is_cuda and tuple(got.shape) == (B, 4, H, W) and bool(torch.isfinite(got).all())
        bad = int((bits(got) != bits(want)).sum())
        assert bad == 0, f"{solver} {name}: {bad}/{want.numel()} elements differ from the Python loop (max |d| {float((got.cpu() - want).abs().max()):.3e})"
        results[name] = got
    assert net._cur[0] == 2 * B
    assert not (bits(results["neg"]) == bits(results["reused"])).all()      # neg_input_cond reaches the uncond rows
    with pytest.raises(lib.SdxlError, match="input_cond"):
        sampler.sample(pe, po, ti, **kw)
    # guidance rescale (the RESCALE instantiations): finite, the same bits run after run, and not the plain step's result
    a, b = (sampler.sample(pe, po, ti, input_cond=ic, neg_input_cond=nic, guidance_rescale=0.5, **kw) for _ in range(2))
    torch.cuda.synchronize()
    assert bool(torch.isfinite(a).all()) and (bits(a) == bits(b)).all() and not (bits(a) == bits(results["neg"])).all()


# ---------------------------------------------------------------------------------------------- 5. the trainer
def _batch(cfg, B, seed, H=16, W=16):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)
    bfr = lambda t: t.to(BF).float()
    mask = (torch.rand(B, 1, H, W, generator=g) < 0.5).float()
    lat = r(B, 4, H, W)
    return {"vae_latents": lat, "prompt_embeds": bfr(r(B, 77, cfg.cross_attention_dim)), "pooled_prompt_embeds": bfr(r(B, cfg.pooled_dim)),
            "time_ids": torch.tensor([[[128.0, 128, 0, 0, 128, 128]]] * B), "inpaint_mask": mask, "masked_latents": lat * (1.0 - mask),
            "metadata": {}}


def _config(**keys):
    c = CFG.Config()
    c.training.method = "ddpm"
    c.optimizer.learning_rate = 1e-3
    c.training.validation_num_steps, c.training.validation_guidance_scale = 3, 2.0
    for k, v in keys.items():
        setattr(c.training, k, v)
    return c


@pytest.mark.parametrize("dropout", [0.0, 1.0], ids=["inpaint", "dropout-1"])
def test_trainer_inpaint_conditioning(tiny9, dropout):
    cfg, w, net = tiny9
    arena0 = net.weights.clone()
    try:
        class M: unet = net
        c = _config(input_conditioning="inpaint", input_cond_dropout_prob=dropout)
        tr = T.NativeSDXLTrainer(M(), config=c)
        b = _batch(cfg, 2, 40)
        noise = torch.randn(2, 4, 16, 16, generator=torch.Generator().manual_seed(60))
        ts = torch.tensor([200, 700])
        ic = torch.cat([b["inpaint_mask"], b["masked_latents"]], dim=1)
        if dropout:
            ic = torch.zeros_like(ic)
        net.forward_loss("ddpm", b["vae_latents"], noise, tr.noise_scheduler.timestep_to_sigma(ts), ts.float(), b["prompt_embeds"],
                         b["pooled_prompt_embeds"], b["time_ids"], None, prediction_type=c.training.prediction_type,
                         min_snr_gamma=c.model.min_snr_gamma, use_ztsnr=c.model.use_ztsnr, input_cond=ic)
        want = net.read_loss()[0]
        net.discard_forward()
        losses = []
        for i in range(2):
            bi = b if i == 0 else _batch(cfg, 2, 41)
            loss, _m = tr._execute_training_step(bi, timesteps=ts, noise=noise, generator=torch.Generator().manual_seed(7))
            tr.optimizer_step()
            torch.cuda.synchronize()
            losses.append(float(loss))
        assert losses[0] == want, f"first loss {losses[0]} vs forward_loss(input_cond=cat(mask, masked)) {want}"
        assert all(l == l and l < 1000.0 for l in losses)
        assert not torch.equal(net.weights, arena0)
        per_t, mean = tr.evaluate([b], [300], generator=torch.Generator().manual_seed(3))      # evaluate passes input_cond (no dropout)
        assert mean == mean and 300 in per_t
        if not dropout:      # validate() builds input_cond from the validation batch and samples with it
            vb = {k: v for k, v in b.items() if k != "metadata"}
            seen = []
            lat = tr.validate(2, [vb], on_validation=lambda step, x: seen.append(step))[0]
            want = tr.sample(b["prompt_embeds"], b["pooled_prompt_embeds"], b["time_ids"], height=16, width=16, input_cond=ic,
                             generator=torch.Generator().manual_seed(int(c.training.validation_seed)))
            torch.cuda.synchronize()
            assert seen == [2] and tuple(lat.shape) == (2, 4, 16, 16) and bool(torch.isfinite(lat).all()) and (bits(lat) == bits(want)).all()
    finally:
        net.weights.copy_(arena0)
        net.grads.zero_()


# ---------------------------------------------------------------------------------------------- 6. refusals on a real handle
def _fwd_args(cfg, B=2, H=16, W=16, seed=5):
    x = make_inputs(cfg, B, H, W, seed=seed)
    ts = torch.tensor([610, 230][:B])
    return x, ("ddpm", x["lat"], x["noise"], LR.karras_sigmas()[ts], ts.float(), x["ehs"], x["pooled"], x["tid"])


def test_refusals_9_channels(tiny9):
    cfg, w, net = tiny9
    x, args = _fwd_args(cfg)
    ic = make_cond(2, 5, 16, 16, 6)
    net.forward_loss(*args, input_cond=ic)
    good = net.read_loss()[0]
    net.discard_forward()
    with pytest.raises(lib.SdxlError, match=r"rc=1.*input_cond"):
        net.forward_loss(*args)
    # sdxl_loss_fwd_bwd on the same structs: the short batch, then the new struct with a NULL array
    b = net._batch(*args[1:], None)
    lc = lib.LossConfig(0, 1, 1, 5.0, 1)
    assert net.L.sdxl_loss_fwd_bwd(net.h, C.byref(lc), C.byref(b), 1.0, 1, st()) == 1 and b"input_cond" in net.L.sdxl_last_error()
    bc = lib.InputCondBatch(*[getattr(b, f[0]) for f in lib.Batch._fields_])
    bc.ctx_len |= lib.BATCH_COND
    assert net.L.sdxl_forward_loss(net.h, C.byref(lc), C.byref(bc), st()) == 1 and b"input_cond" in net.L.sdxl_last_error()
    bc.input_cond, bc.cond_channels = ic.to(DEV).data_ptr(), 4      # a channel count that is not the handle's
    assert net.L.sdxl_forward_loss(net.h, C.byref(lc), C.byref(bc), st()) == 1 and b"input_cond" in net.L.sdxl_last_error()
    # a sampler step, init included
    pe, po, ti = x["ehs"].to(DEV, BF), x["pooled"].to(DEV, BF), x["tid"].to(DEV)
    xs, tt = torch.randn(2, 4, 16, 16, device=DEV), torch.full((2,), 500.0, device=DEV)
    with pytest.raises(lib.SdxlError, match=r"rc=1.*input_cond"):
        net.sample_init(xs, pe, po, ti, tt, cfg=False)
    with pytest.raises(lib.SdxlError, match=r"rc=1.*input_cond"):
        net.sample_step(xs, pe, po, ti, tt, cfg=False, a_skip=1.0, a_out=-1.0, p=0.5, q=0.5)
    with pytest.raises(ValueError, match="input_cond"):
        net.forward_loss(*args, input_cond=ic[:, :4])
    # nothing was launched or changed: the same step gives the same loss
    net.forward_loss(*args, input_cond=ic)
    assert net.read_loss()[0] == good
    net.discard_forward()


def test_refusals_4_channels(tiny4):
    cfg, w, net = tiny4
    x, args = _fwd_args(cfg)
    net.forward_loss(*args)
    good = net.read_loss()[0]
    net.discard_forward()
    ic = make_cond(2, 5, 16, 16, 6)
    with pytest.raises(lib.SdxlError, match=r"rc=1.*input_cond"):
        net.forward_loss(*args, input_cond=ic)
    pe, po, ti = x["ehs"].to(DEV, BF), x["pooled"].to(DEV, BF), x["tid"].to(DEV)
    xs, tt = torch.randn(2, 4, 16, 16, device=DEV), torch.full((2,), 500.0, device=DEV)
    with pytest.raises(lib.SdxlError, match=r"rc=1.*input_cond"):
        net.sample_init(xs, pe, po, ti, tt, cfg=False, input_cond=ic.to(DEV))
    # the flag with a NULL array is the 4-channel call
    b = net._batch(*args[1:], None)
    bc = lib.InputCondBatch(*[getattr(b, f[0]) for f in lib.Batch._fields_])
    bc.ctx_len |= lib.BATCH_COND
    lc = lib.LossConfig(0, 1, 1, 5.0, 1)
    lib.check(net.L.sdxl_forward_loss(net.h, C.byref(lc), C.byref(bc), st()), "sdxl_forward_loss")
    assert net.read_loss()[0] == good
    net.discard_forward()
    with pytest.raises(lib.SdxlError, match="in_channels"):
        NU.NativeUNet(NU.make_config(in_channels=17))
