"""The extended sampler step and the solvers on the GPU: the kernel (through sdxl_op_sampler_step) against the host restatement
tests/_sampler_solver_ref.py bit for bit, what it may and may not write, its argument errors, every solver / img2img / inpainting of
the whole sampler against a Python loop around unet_forward, and validation sampling with a second-order solver from train()."""
import ctypes as C
import importlib
import math

import pytest
import torch

import _sampler_ref as R
import _sampler_solver_ref as X
import sdxl_amd  # noqa: F401
from sdxl_amd import lib
from _optim_common import bits, dev, ptr, stream
from test_gpu_sampler import _batch, _cond, _config, _tiny_net, _train_step, check_image, run_hook, to_nhwc8
from test_host_sampler_solvers import bad_extended_arguments

S = importlib.import_module("sdxl-training-improvements_amd.sampler")
T = importlib.import_module("sdxl-training-improvements_amd.trainer")

pytestmark = pytest.mark.gpu
# (2, 9, 7): one partly idle block, H W no multiple of 64; (1, 168, 96): 63 full blocks; (4, 128, 128): the headline latent
SHAPES = [(2, 9, 7), (1, 168, 96), (4, 128, 128)]
PLANES = ("hist", "xsave", "noise", "mask", "known", "knoise")
BASE = dict(init=0, a_skip=0.31, a_out=-1.7, p=0.62, q=0.38, a_in_next=1.0, clamp=20000.0)
TERMS = {"hist_rw": dict(r=-0.37, save=1), "xsave_rw": dict(u=1.21, save=2), "noise": dict(s=0.83), "mask": dict(k_a=0.9, k_b=3.3),
         "save_both": dict(save=3), "all": dict(r=-0.37, u=1.21, s=0.83, save=3, k_a=0.9, k_b=3.3)}


def _uses(k):
    """the planes a step with these scalars names"""
    save = int(k.get("save", 0))
    return {"hist": k.get("r", 0) != 0 or save & 1, "xsave": k.get("u", 0) != 0 or save & 2, "noise": k.get("s", 0) != 0,
            "mask": "k_a" in k, "known": "k_a" in k, "knoise": k.get("k_b", 0) != 0}


def _data(B, H, W, cfg, seed):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)
    d = dict(x=r(B, 4, H, W) * 9.0, fc=r(B, 4, H, W).to(torch.bfloat16), hist=r(B, 4, H, W) * 3.0, xsave=r(B, 4, H, W) * 9.0,
             noise=r(B, 4, H, W), mask=torch.rand(B, 1, H, W, generator=g), known=r(B, 4, H, W) * 2.0, knoise=r(B, 4, H, W))
    d["fu"] = (0.8 * d["fc"].float() + 0.3 * r(B, 4, H, W)).to(torch.bfloat16) if cfg else None
    d["mask"][:, :, 0, :2] = torch.tensor([0.0, 1.0])                            # both ends of the range are in every mask
    return d


def run_ext(d, k, planes, flag=True):
    """the step kernel on caller buffers through the extended struct.  d: the CPU tensors (_data), k: scalar fields, planes: the
    names whose pointers are passed (the others stay NULL).  Returns the state, the input image and every passed plane after the call."""
    L = lib.load()
    B, _c, H, W = d["x"].shape
    cfg = int(k["cfg"])
    xd = d["x"].to(dev()).contiguous()
    pred = to_nhwc8(torch.cat([d["fc"], d["fu"]]) if cfg else d["fc"], fill=7.0).to(dev())
    xin = torch.full_like(pred, float("nan"))                                    # every row must be written
    s = lib.SamplerStepExt(None, cfg, int(k.get("init", 0)) | (lib.SAMPLER_EXT if flag else 0), k["a_skip"], k["a_out"], k["p"], k["q"],
                           k["a_in_next"], k["clamp"], k["guidance"], k.get("guidance_rescale", 0.0))
    s.r, s.u, s.s, s.save, s.k_a, s.k_b = (k.get(n, 0) for n in ("r", "u", "s", "save", "k_a", "k_b"))
    on = {n: d[n].to(dev()).contiguous() for n in planes}
    for n, t in on.items():
        setattr(s, n, t.data_ptr())
    lib.check(L.sdxl_op_sampler_step(ptr(xd), ptr(pred), ptr(xin), B, H, W, C.byref(s), stream()), "sdxl_op_sampler_step")
    torch.cuda.synchronize()
    return dict({n: t.cpu() for n, t in on.items()}, x=xd.cpu(), xin=xin.cpu())


def _kernel_F(d, k):
    """the guided AND rescaled prediction as the plain kernel computes it (tests/test_gpu_sampler.py holds that arithmetic): with
    a_skip = 0, a_out = 1, p = 0, q = 1 the plain step leaves x = 0 x + 1 (0 x + 1 F) = F.  The per-sample ratio of guidance rescale is
    a device reduction that torch.std matches to rounding only, so the restatement of a rescaled extended step starts from these bits."""
    kF = dict(k, a_skip=0.0, a_out=1.0, p=0.0, q=1.0, a_in_next=1.0, clamp=0.0)
    F, _xin = run_hook(torch.ones_like(d["x"]), d["fc"], d["fu"], kF)
    return F


def _want(d, k, F=None):
    u = _uses(k)
    args = {n: (d[n] if u[n] else None) for n in PLANES}
    return X.ext_step(d["x"], d["fc"].float(), None if d["fu"] is None else d["fu"].float(), k, F=F, **args)


# ---------------------------------------------------------------------------------------------- 1. the extended step, bit-exact
@pytest.mark.parametrize("phi", [0.0, 0.5])
@pytest.mark.parametrize("cfg", [0, 1])
@pytest.mark.parametrize("term", list(TERMS))
def test_extended_step_bit_exact(term, cfg, phi):
    k = dict(BASE, **TERMS[term], cfg=cfg, guidance=5.0 if cfg else 1.0, guidance_rescale=phi)
    u = _uses(k)
    for (B, H, W) in SHAPES:
        d = _data(B, H, W, cfg, 1000 * B + H + W + cfg)
        F = None
        if phi:
            F = _kernel_F(d, k)
            plain = R.guide(d["fc"].float(), None if d["fu"] is None else d["fu"].float(), k["guidance"])
            assert not cfg or float((F - plain).abs().max()) > 1e-2 * float(plain.abs().max())      # the rescale does something
        want_x, want_in, want_hist, want_xsave = _want(d, k, F)
        got = run_ext(d, k, [n for n in PLANES if u[n]])
        what = f"{term} cfg={cfg} phi={phi} {(B, H, W)}"
        bad = int((bits(got["x"]) != bits(want_x)).sum())
        assert bad == 0, f"{what}: {bad}/{want_x.numel()} state elements differ from the restatement"
        check_image(got["xin"], want_in, B, H, W, cfg)
        if u["hist"]:
            assert (bits(got["hist"]) == bits(want_hist)).all(), f"{what}: hist"
        if u["xsave"]:
            assert (bits(got["xsave"]) == bits(want_xsave)).all(), f"{what}: xsave"
        if k.get("save", 0) & 2:
            assert (bits(got["xsave"]) == bits(d["x"])).all()                     # the state BEFORE the step
        for n in ("noise", "mask", "known", "knoise"):                             # inputs keep their bits
            assert not u[n] or (bits(got[n]) == bits(d[n])).all(), f"{what}: {n} was written"
        assert bool(torch.isfinite(got["x"]).all())
        # every term changed the result: the plain step's state is another one
        if term != "save_both":
            assert not (bits(got["x"]) == bits(_want(d, dict(BASE, cfg=cfg, guidance=k["guidance"], guidance_rescale=phi), F)[0])).all()


@pytest.mark.parametrize("cfg", [0, 1])
def test_flag_with_nothing_set_is_the_plain_step(cfg):
    """the flag, every new pointer NULL and every new scalar 0: the plain step's bits (with and without guidance rescale); and the
    init call with the flag writes the input image only"""
    for (B, H, W) in SHAPES:
        d = _data(B, H, W, cfg, 50 + B + cfg)
        for phi in (0.0, 0.5):
            k = dict(BASE, cfg=cfg, guidance=5.0 if cfg else 1.0, guidance_rescale=phi)
            px, pin = run_hook(d["x"], d["fc"], d["fu"], k)
            got = run_ext(d, k, [])
            assert (bits(got["x"]) == bits(px)).all() and (bits(got["xin"]) == bits(pin)).all()
            if not phi:
                want_x, want_in = R.full_step(d["x"], d["fc"].float(), None if d["fu"] is None else d["fu"].float(), k)
                assert (bits(got["x"]) == bits(want_x)).all()
        k = dict(BASE, **TERMS["all"], init=1, cfg=cfg, guidance=5.0, guidance_rescale=0.5, a_in_next=0.37, clamp=0.0)
        got = run_ext(d, k, PLANES)
        assert all((bits(got[n]) == bits(d[n])).all() for n in PLANES + ("x",))
        check_image(got["xin"], R.unet_input(d["x"], 0.37, 0.0), B, H, W, cfg)


# ---------------------------------------------------------------------------------------------- 2. what a step may write
def test_canaries():
    """every pointer is passed, the scalars decide what is touched: a buffer the step does not name keeps its bits, hist without
    save bit 0 is only read, xsave without bit 1 likewise, and the read-only planes are never written"""
    for (B, H, W) in SHAPES:
        d = _data(B, H, W, 1, 70 + B)
        base = dict(BASE, cfg=1, guidance=5.0, guidance_rescale=0.0)
        for extra, written in ((dict(), ()), (dict(r=0.5, u=-0.25, s=0.1), ()), (dict(r=0.5, save=2), ("xsave",)),
                               (dict(u=0.5, save=1), ("hist",)), (dict(save=3), ("hist", "xsave"))):
            k = dict(base, **extra)
            got = run_ext(dict(d, mask=None), k, [n for n in PLANES if n != "mask"])         # mask NULL: known / knoise are not named
            want_x, _in, want_hist, want_xsave = X.ext_step(d["x"], d["fc"].float(), d["fu"].float(), k, d["hist"], d["xsave"], d["noise"])
            assert (bits(got["x"]) == bits(want_x)).all()
            for n in ("hist", "xsave", "noise", "known", "knoise"):
                same = bool((bits(got[n]) == bits(d[n])).all())
                assert same == (n not in written), f"{(B, H, W)} {extra}: {n} {'not ' if same else ''}written"
            assert (bits(got["hist"]) == bits(want_hist)).all() and (bits(got["xsave"]) == bits(want_xsave)).all()


def test_mask_extremes():
    """m = 0 with k_a = 1, k_b = 0 leaves exactly `known` (knoise may be NULL); m = 1 leaves the unblended value.  Compared as numbers:
    the blend adds a zero, and -0 + 0 = +0."""
    for (B, H, W) in SHAPES:
        d = _data(B, H, W, 0, 90 + B)
        k = dict(BASE, cfg=0, guidance=1.0, r=-0.37, s=0.83, k_a=1.0, k_b=0.0)
        free = X.ext_step(d["x"], d["fc"].float(), None, {n: v for n, v in k.items() if n not in ("k_a", "k_b")}, d["hist"], None, d["noise"])[0]
        for m, want in ((0.0, d["known"]), (1.0, free)):
            dm = dict(d, mask=torch.full((B, 1, H, W), m))
            got = run_ext(dm, k, ["hist", "noise", "mask", "known"])
            assert torch.equal(got["x"], want), f"{(B, H, W)} m={m}: max |d| {float((got['x'] - want).abs().max()):.3e}"
            assert (bits(got["x"]) == bits(X.ext_step(d["x"], d["fc"].float(), None, k, d["hist"], None, d["noise"], dm["mask"], d["known"])[0])).all()
        got = run_ext(d, dict(k, k_b=3.3), ["hist", "noise", "mask", "known", "knoise"])      # the mask of _data holds 0, 1 and between
        m = d["mask"].expand(B, 4, H, W)
        y = torch.tensor(3.3) * d["knoise"] + d["known"]
        assert torch.equal(got["x"][m == 0], y[m == 0]) and torch.equal(got["x"][m == 1], free[m == 1])


# ---------------------------------------------------------------------------------------------- 3. bad arguments
def test_bad_arguments_launch_nothing():
    L = lib.load()
    x = torch.full((1, 4, 8, 8), 3.0, device=dev())
    pred = torch.zeros(64, 8, dtype=torch.bfloat16, device=dev())
    xin = torch.full_like(pred, 5.0)
    plane = torch.full((1, 4, 8, 8), 7.0, device=dev())
    for kw, msg in bad_extended_arguments(plane.data_ptr()):
        s = lib.SamplerStepExt(None, 0, lib.SAMPLER_EXT, 1.0, 1.0, 1.0, 1.0, 1.0, 0.0, 1.0, 0.0)
        for n, v in kw.items():
            setattr(s, n, v)
        rc = L.sdxl_op_sampler_step(ptr(x), ptr(pred), ptr(xin), 1, 8, 8, C.byref(s), stream())
        assert rc == 1 and msg.encode() in L.sdxl_last_error(), (kw, L.sdxl_last_error())
    torch.cuda.synchronize()
    assert bool((x == 3.0).all()) and bool((xin == 5.0).all()) and bool((plane == 7.0).all())


def test_sample_step_keywords(tiny):
    """NativeUNet.sample_step: the plain call passes no flag (any plane would be refused by the checks above if it were read); a
    plane of the wrong dtype or size is a ValueError; and the tensors of an extended call are kept alive"""
    cfg, net = tiny
    pe, po, ti, noise = _cond(2, cfg.cross_attention_dim, cfg.pooled_dim, 16, 16, 31)
    x = noise.to(dev())
    args = (pe.to(dev()).to(torch.bfloat16), po.to(dev()).to(torch.bfloat16), ti.to(dev()), torch.zeros(2, device=dev()))
    base = dict(cfg=0, a_skip=1.0, a_out=1.0, p=1.0, q=0.0)
    net.sample_init(x, *args, cfg=False)
    for bad in (dict(hist=torch.zeros(2, 4, 16, 16)), dict(hist=torch.zeros(2, 4, 16, 8, device=dev()), save=1),
                dict(noise=torch.zeros(2, 4, 16, 16, device=dev(), dtype=torch.float64), s=1.0),
                dict(mask=torch.zeros(2, 4, 16, 16, device=dev()), known=x, k_a=1.0)):
        with pytest.raises(ValueError):
            net.sample_step(x, *args, **base, **bad)
    with pytest.raises(lib.SdxlError, match="hist"):
        net.sample_step(x, *args, **base, r=0.5)
    h = torch.zeros_like(x)
    net.sample_step(x, *args, **base, hist=h, save=1)
    assert any(t is h for t in net._keep)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(h).all()) and float(h.abs().max()) > 0.0


# ---------------------------------------------------------------------------------------------- 4. the whole sampler
@pytest.fixture(scope="module")
def tiny():
    cfg, net = _tiny_net()
    yield cfg, net
    net.close()


def python_solver_loop(net, sampler, pe, po, ti, noise, num_steps, guidance_scale, solver, step_noise=None, init=None, strength=1.0,
                       mask=None):
    """the same sampler as a Python loop: unet_forward on the [cond; uncond] batch, the restatement between the calls.  The scalars
    are sampler.solver_steps' (tests/test_host_sampler_solvers.py holds them); the start state is restated here."""
    B = pe.shape[0]
    cfg = guidance_scale != 1.0
    flow = sampler.method == "flow_matching"
    x0_scale, steps = sampler.schedule(num_steps)
    lv, _ts = sampler.grid(num_steps)
    n = len(steps)
    first = 0 if init is None else n - max(1, int(math.floor(strength * n + 0.5)))
    steps, lv = steps[first:], lv[first:]
    ks, tin, _levels = S.solver_steps(steps, lv, sampler.method, solver, 1.0, guidance_scale, 0.0, cfg, mask is not None)
    c = lambda v: torch.tensor(v, dtype=torch.float32)
    if init is None or first == 0:
        x = noise if x0_scale == 1.0 else c(x0_scale) * noise
    elif flow:
        x = c(1.0 - lv[0]) * noise + c(lv[0]) * init
    else:
        x = init + c(lv[0]) * noise
    m4 = None
    if mask is not None:
        m4 = mask.reshape(B, 1, *mask.shape[-2:])
        x = X.blend(x, m4, init, noise, *((lv[0], 1.0 - lv[0]) if flow else (1.0, lv[0])))
    pe2 = torch.cat([pe, torch.zeros_like(pe)]) if cfg else pe
    po2 = torch.cat([po, torch.zeros_like(po)]) if cfg else po
    ti2 = torch.cat([ti, ti]) if cfg else ti

    def model(inp, t, _f):
        PB = 2 * B if cfg else B
        out = net.unet_forward(torch.cat([inp, inp]) if cfg else inp, torch.full((PB,), t), pe2, po2, ti2).cpu()
        return (out[:B], out[B:]) if cfg else out
    return X.solver_loop(model, x, (steps[0][0], steps[0][5]), ks, tin, cfg, step_noise, m4, init, noise), len(ks)


def _same(got, want, what):
    torch.cuda.synchronize()
    assert got.dtype == torch.float32 and got.is_cuda and tuple(got.shape) == tuple(want.shape) and bool(torch.isfinite(got).all())
    bad = int((bits(got) != bits(want)).sum())
    assert bad == 0, f"{what}: {bad}/{want.numel()} elements differ from the Python loop (max |d| {float((got.cpu() - want).abs().max()):.3e})"


@pytest.mark.parametrize("case", [("ddpm", "euler_a", 6, 6), ("ddpm", "dpmpp_2m", 6, 6), ("ddpm", "heun", 6, 11), ("flow_matching", "heun", 4, 7)])
def test_solver_equals_python_loop_tiny(tiny, case):
    method, solver, N, forwards = case
    cfg, net = tiny
    B, H, W = 2, 16, 16
    pe, po, ti, noise = _cond(B, cfg.cross_attention_dim, cfg.pooled_dim, H, W, 11)
    sn = torch.randn(N - 1, B, 4, H, W, generator=torch.Generator().manual_seed(12)) if solver == "euler_a" else None
    sampler = S.NativeSampler(net, method, "v_prediction", True, "trained")
    want, nf = python_solver_loop(net, sampler, pe, po, ti, noise, N, 5.0, solver, sn)
    assert nf == forwards
    kw = dict(height=H, width=W, num_steps=N, guidance_scale=5.0, noise=noise, solver=solver, step_noise=sn)
    got = sampler.sample(pe, po, ti, **kw)
    _same(got, want, case)
    assert (bits(sampler.sample(pe, po, ti, **kw)) == bits(got)).all() and net._cur[0] == 2 * B
    euler = sampler.sample(pe, po, ti, height=H, width=W, num_steps=N, guidance_scale=5.0, noise=noise)
    assert not (bits(euler) == bits(got)).all()                                   # another solver, another result
    if solver == "euler_a":                                                       # the draw from the generator: the initial noise first
        g = torch.Generator().manual_seed(5)
        n0, sn2 = torch.randn((B, 4, H, W), generator=g), torch.randn((N - 1, B, 4, H, W), generator=g)
        a = sampler.sample(pe, po, ti, height=H, width=W, num_steps=N, guidance_scale=5.0, solver=solver, generator=torch.Generator().manual_seed(5))
        b = sampler.sample(pe, po, ti, height=H, width=W, num_steps=N, guidance_scale=5.0, solver=solver, noise=n0, step_noise=sn2)
        assert (bits(a) == bits(b)).all()
        zero = sampler.sample(pe, po, ti, **dict(kw, eta=0.0, step_noise=None))
        assert (bits(zero) == bits(euler)).all()                                  # eta = 0 is Euler


@pytest.mark.parametrize("case", [("ddpm", "heun", 6), ("flow_matching", "euler", 4)])
def test_img2img(tiny, case):
    method, solver, N = case
    cfg, net = tiny
    B, H, W = 2, 16, 16
    pe, po, ti, noise = _cond(B, cfg.cross_attention_dim, cfg.pooled_dim, H, W, 14)
    init = torch.randn(B, 4, H, W, generator=torch.Generator().manual_seed(15)) * 0.8
    sampler = S.NativeSampler(net, method, "v_prediction", True, "trained")
    kw = dict(height=H, width=W, num_steps=N, guidance_scale=5.0, noise=noise, solver=solver)
    full = sampler.sample(pe, po, ti, **kw)
    same = sampler.sample(pe, po, ti, **kw, init_latents=init, strength=1.0)
    assert (bits(full) == bits(same)).all()                                       # strength = 1 is pure noise
    want, nf = python_solver_loop(net, sampler, pe, po, ti, noise, N, 5.0, solver, init=init, strength=0.5)
    assert nf == {("heun", 6): 5, ("euler", 4): 2}[(solver, N)]                  # the last N / 2 grid points
    got = sampler.sample(pe, po, ti, **kw, init_latents=init, strength=0.5)
    _same(got, want, case)
    assert not (bits(got) == bits(full)).all()


@pytest.mark.parametrize("case", [("ddpm", "dpmpp_2m", 6), ("flow_matching", "heun", 4)])
def test_inpainting(tiny, case):
    method, solver, N = case
    cfg, net = tiny
    B, H, W = 2, 16, 16
    pe, po, ti, noise = _cond(B, cfg.cross_attention_dim, cfg.pooled_dim, H, W, 16)
    init = torch.randn(B, 4, H, W, generator=torch.Generator().manual_seed(17)) * 0.8
    mask = torch.ones(B, H, W)
    mask[:, :, : W // 2] = 0.0                                                    # the left half is kept
    sampler = S.NativeSampler(net, method, "v_prediction", True, "trained")
    kw = dict(height=H, width=W, num_steps=N, guidance_scale=5.0, noise=noise, solver=solver, init_latents=init)
    want, _nf = python_solver_loop(net, sampler, pe, po, ti, noise, N, 5.0, solver, init=init, mask=mask)
    got = sampler.sample(pe, po, ti, **kw, inpaint_mask=mask)
    _same(got, want, case)
    keep = (mask == 0).reshape(B, 1, H, W).expand(B, 4, H, W)
    assert torch.equal(got.cpu()[keep], init[keep])                                # exactly the known latent where m = 0
    free = sampler.sample(pe, po, ti, **kw)
    assert not torch.equal(got.cpu()[~keep], free.cpu()[~keep])                    # the kept half steers the generated one
    assert (bits(sampler.sample(pe, po, ti, **kw, inpaint_mask=mask.reshape(B, 1, H, W))) == bits(got)).all()


# ---------------------------------------------------------------------------------------------- 5. the trainer
def test_train_validates_with_dpmpp_2m_and_training_is_bitwise_unaffected(tiny):
    """validation_sampler: dpmpp_2m -- train(..., validation_batches=...) hands on_validation what sample(solver="dpmpp_2m") returns,
    and the weights, the optimizer state and the next step's loss have the bits of the same run without validation"""
    cfg, net = tiny
    arena0 = net.weights.clone()
    vb = [{k: v for k, v in _batch(cfg, 2, 91).items() if k != "metadata"}]

    def run(validate):
        net.weights.copy_(arena0)
        net.grads.zero_()
        c = _config(False)
        c.training.validation_sampler = "dpmpp_2m"
        c.training.validation_every_n_steps, c.training.gradient_accumulation_steps, c.training.validation_seed = 2, 1, 5
        class M: unet = net
        tr = T.NativeSDXLTrainer(M(), train_dataloader=[_batch(cfg, 2, s) for s in range(4)], config=c)
        seen = []
        torch.manual_seed(1234)
        tr.train(1, validation_batches=vb if validate else None, on_validation=lambda step, lat: seen.append((step, lat.clone())))
        state = [net.weights.clone()] + [a.clone() for a in tr.optimizer.state_arenas()]
        direct = None
        if validate:
            b = vb[0]
            gen = torch.Generator().manual_seed(5)
            direct = [tr.sample(b["prompt_embeds"], b["pooled_prompt_embeds"], b["time_ids"], height=16, width=16, generator=gen, solver=s).clone()
                      for s in ("dpmpp_2m", "euler")]
        return _train_step(tr, cfg, 3), state, seen, direct

    try:
        l0, s0, seen0, _ = run(False)
        l1, s1, seen1, direct = run(True)
        assert seen0 == [] and [s for s, _ in seen1] == [1, 3]
        assert all(tuple(l.shape) == (2, 4, 16, 16) and bool(torch.isfinite(l).all()) for _, l in seen1)
        assert l0 == l1 and len(s0) == len(s1) and all((bits(a) == bits(b)).all() for a, b in zip(s0, s1))
        assert (bits(seen1[1][1]) == bits(direct[0])).all() and not (bits(direct[0]) == bits(direct[1])).all()
    finally:
        net.weights.copy_(arena0)
        net.grads.zero_()
