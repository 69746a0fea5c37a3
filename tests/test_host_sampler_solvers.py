"""CPU checks of the sampler's solvers (sampler.solver_steps): euler is today's schedule, the second-order solvers converge at second
order on the schedule's own scalars, every solver samples the ideal model back, the ancestral scalars, Heun's forwards, the extended
struct's mirror, the calls sample() issues, and every error."""
import ctypes as C
import importlib
import math
import re
from pathlib import Path

import pytest
import torch

import _sampler_solver_ref as X
import sdxl_amd  # noqa: F401
from sdxl_amd import lib
from test_host_sampler import _FakeNet, _ideal, _trainer

S = importlib.import_module("sdxl-training-improvements_amd.sampler")
CFG = importlib.import_module("sdxl-training-improvements_amd.config")
NM = importlib.import_module("sdxl-training-improvements_amd.native_mi355x")

ROOT = Path(__file__).resolve().parent.parent
NEW_KEYS = {"r", "u", "s", "save", "k_a", "k_b"}


def _sampler(method="ddpm", pred="v_prediction", par="trained", ztsnr=True):
    return S.NativeSampler(None, method, pred, ztsnr, par)


# ---------------------------------------------------------------------------------------------- 1. euler is today's schedule
@pytest.mark.parametrize("kind", [("ddpm", "v_prediction", "trained"), ("ddpm", "epsilon", "trained"), ("ddpm", "v_prediction", "reference"),
                                  ("flow_matching", "v_prediction", "trained")])
@pytest.mark.parametrize("N", [2, 8, 30])
def test_euler_is_unchanged(kind, N):
    sm = _sampler(*kind)
    x0, steps = sm.schedule(N)
    lv, _ts = sm.grid(N)
    for g, phi, cfg in ((5.0, 0.7, True), (1.0, 0.0, False)):
        ks, tin, levels = S.solver_steps(steps, lv, kind[0], "euler", 1.0, g, phi, cfg, False, kind[2])
        assert ks == S.kernel_steps(steps, g, phi, cfg)
        assert tin == [s[6] for s in steps] and levels == lv[:len(steps)]
        assert all(not (k["init"] & lib.SAMPLER_EXT) and not (set(k) & NEW_KEYS) for k in ks)


def test_schedule_and_grid_agree():
    """grid() is what schedule() is built on: explicit sigmas / timesteps included"""
    sm = _sampler()
    lv, ts = sm.grid(6)
    assert lv == [float(sm.table[i]) for i in S.ddpm_indices(6)] and ts == [float(i) for i in S.ddpm_indices(6)]
    assert sm.schedule(6) == S.ddpm_trained_steps(lv, ts, "v_prediction", True)
    assert sm.grid(9, sigmas=[100.0, 1.0], timesteps=[3.0, 4.0]) == ([100.0, 1.0], [3.0, 4.0])
    fl = _sampler("flow_matching")
    assert fl.grid(4) == ([0.0, 0.25, 0.5, 0.75, 1.0], None) and fl.grid(0, timesteps=[0.0, 0.5, 1.0]) == ([0.0, 0.5, 1.0], None)


# ---------------------------------------------------------------------------------------------- 2. order of convergence
def _error(solver, n_points):
    """|x - exact| at sigma = 0.1 after the geometric grid 10 -> 0.1 of n_points, from x(10) = 10, den(x, s) = x / (1 + s^2): the exact
    solution of dx / ds = (x - den) / s is x(s') = x(s) sqrt((1 + s'^2) / (1 + s^2)).  The schedule's own scalars, in double."""
    sig = [10.0 * (0.1 / 10.0) ** (j / (n_points - 1)) for j in range(n_points)]
    sig[-1] = 0.1
    _x0, steps = S.ddpm_trained_steps(sig, [0.0] * n_points, "v_prediction", False)
    ks, _tin, levels = S.solver_steps(steps, sig, "ddpm", solver)
    assert levels[-1] == 0.1                                   # the last forward is the step to sigma = 0: left out
    x = X.simulate(ks[:-1], levels[:-1], lambda x, s: x / (1.0 + s * s), 10.0)
    return abs(x - 10.0 * math.sqrt((1.0 + 0.1 ** 2) / (1.0 + 10.0 ** 2)))


def test_order_of_convergence():
    e = {sv: (_error(sv, 33), _error(sv, 65)) for sv in ("euler", "heun", "dpmpp_2m")}
    for sv, (a, b) in e.items():
        print(f"{sv}: |error| at 33 points {a:.4e}, at 65 points {b:.4e}, ratio {a / b:.3f}")
    assert 1.8 <= e["euler"][0] / e["euler"][1] <= 2.2
    for sv in ("heun", "dpmpp_2m"):
        assert e[sv][0] / e[sv][1] >= 3.5
        assert e[sv][0] < e["euler"][1]


# ---------------------------------------------------------------------------------------------- 3. the ideal model
@pytest.mark.parametrize("N", [2, 8, 30])
@pytest.mark.parametrize("case", [("v_prediction", "euler_a"), ("v_prediction", "dpmpp_2m"), ("v_prediction", "heun"), ("epsilon", "euler_a"),
                                  ("epsilon", "dpmpp_2m"), ("epsilon", "heun"), ("flow", "heun"), ("v_prediction", "euler"), ("flow", "euler")])
def test_every_solver_samples_the_ideal_model_back(case, N):
    """the model that returns the training target of a fixed x* (tests/test_host_sampler.py::_ideal) has den = x* at every forward,
    whatever state it is given, and every solver ends on an Euler step to the clean end (sigma = 0: x = den; flow: the velocity is
    constant, so every stage adds its share of x* - n).  In float64 that is x* to a few roundings of terms of the size of the state;
    the bound is that file's own, 1e-9 max |x*|."""
    kind, solver = case
    g = torch.Generator().manual_seed(300 + N)
    xstar = torch.randn(2, 4, 8, 8, generator=g, dtype=torch.float64) * 3.0
    n = torch.randn(2, 4, 8, 8, generator=g, dtype=torch.float64)
    if kind == "flow":
        sm = S.NativeSampler(None, "flow_matching", t_bf16=False)
        model = _ideal("flow", xstar, n)
    else:
        sm = _sampler("ddpm", kind, "trained", False)
        model = _ideal(kind, xstar)
    x0_scale, steps = sm.schedule(N)
    lv, _ts = sm.grid(N)
    ks, tin, levels = S.solver_steps(steps, lv, sm.method, solver, 1.0)
    nst = sum(1 for k in ks if k.get("s", 0) != 0)
    assert nst == (N - 1 if solver == "euler_a" else 0)
    sn = torch.randn(max(nst, 1), 2, 4, 8, 8, generator=g, dtype=torch.float64)
    out = X.solver_loop(lambda inp, t, f: model(inp, levels[f]), n * x0_scale, (steps[0][0], steps[0][5]), ks, tin, False, sn, quantize=False)
    err = float((out - xstar).abs().max())
    print(f"{kind} {solver} N={N}: max |x - x*| = {err:.3e}  (bound {1e-9 * float(xstar.abs().max()):.3e})")
    assert out.dtype == torch.float64 and err <= 1e-9 * float(xstar.abs().max())


# ---------------------------------------------------------------------------------------------- 4. ancestral scalars
def test_ancestral_scalars():
    sm = _sampler()
    _x0, steps = sm.schedule(30)
    lv, _ts = sm.grid(30)
    ks, tin, _lv = S.solver_steps(steps, lv, "ddpm", "euler_a", 1.0, 5.0, 0.0, True)
    assert len(ks) == 30 and tin == [s[6] for s in steps]
    for j in range(29):
        down, up = S.ancestral_sigmas(lv[j], lv[j + 1], 1.0)
        assert abs(down * down + up * up - lv[j + 1] ** 2) <= 4 * 2.0 ** -53 * lv[j + 1] ** 2       # two squares, a sum, a root undone
        assert 0.0 < up <= lv[j + 1] and ks[j]["s"] == up and ks[j]["p"] == down / lv[j] and ks[j]["q"] == 1.0 - down / lv[j]
        assert up == min(lv[j + 1], math.sqrt(lv[j + 1] ** 2 * (lv[j] ** 2 - lv[j + 1] ** 2) / lv[j] ** 2))
    assert "s" not in ks[-1] and (ks[-1]["p"], ks[-1]["q"]) == (0.0, 1.0)                            # the step to 0 is Euler
    # eta scales the fresh noise until it is all of it; eta = 0 is Euler, key for key
    half = S.solver_steps(steps, lv, "ddpm", "euler_a", 0.5)[0]
    assert all(abs(half[j]["s"] - 0.5 * ks[j]["s"]) <= 1e-15 * ks[j]["s"] or ks[j]["s"] == lv[j + 1] for j in range(29))
    assert S.solver_steps(steps, lv, "ddpm", "euler_a", 0.0, 5.0, 0.3, True)[0] == S.kernel_steps(steps, 5.0, 0.3, True)
    assert S.solver_steps(steps, lv, "ddpm", "euler_a", 1e9)[0][3]["s"] == lv[4]                     # capped at sigma': sigma_down = 0


def test_dpmpp_2m_scalars():
    """k-diffusion's sample_dpmpp_2m written out: x' = (s'/s) x - expm1(-h) den_d, den_d = (1 + 1/(2r)) den - (1/(2r)) old"""
    sm = _sampler()
    _x0, steps = sm.schedule(8)
    lv, _ts = sm.grid(8)
    ks = S.solver_steps(steps, lv, "ddpm", "dpmpp_2m")[0]
    assert len(ks) == 8 and all(k["save"] == 1 for k in ks) and "r" not in ks[0] and "r" not in ks[-1]
    assert [(k["p"], k["q"]) for k in (ks[0], ks[-1])] == [(steps[0][3], steps[0][4]), (0.0, 1.0)]
    for j in range(1, 7):
        h, h_last = math.log(lv[j]) - math.log(lv[j + 1]), math.log(lv[j - 1]) - math.log(lv[j])
        r = h_last / h
        assert ks[j]["p"] == lv[j + 1] / lv[j]
        assert abs(ks[j]["q"] - (-math.expm1(-h)) * (1 + 1 / (2 * r))) <= 1e-12 * abs(ks[j]["q"])
        assert abs(ks[j]["r"] - math.expm1(-h) / (2 * r)) <= 1e-12 * abs(ks[j]["r"])
        assert abs(ks[j]["p"] + ks[j]["q"] + ks[j]["r"] - 1.0) <= 1e-12                             # a constant state and den stay put


# ---------------------------------------------------------------------------------------------- 5. Heun's forwards
def test_heun_forwards():
    sm = _sampler()
    for N in (2, 6, 30):
        _x0, steps = sm.schedule(N)
        lv, ts = sm.grid(N)
        ks, tin, levels = S.solver_steps(steps, lv, "ddpm", "heun", 1.0, 5.0, 0.0, True)
        assert len(ks) == len(tin) == len(levels) == 2 * (N - 1) + 1
        assert tin == [ts[0]] + [t for t in ts[1:] for _ in (0, 1)][:-1] + ([ts[-1]] if N > 1 else [])
        assert levels == [lv[0]] + [s for s in lv[1:] for _ in (0, 1)][:-1] + [lv[-1]]
        for j in range(N - 1):
            a, b = ks[2 * j], ks[2 * j + 1]
            assert tin[2 * j + 1] == ts[j + 1] and float(tin[2 * j + 1]).is_integer() and 0 <= tin[2 * j + 1] <= 999      # a table index
            assert a["save"] == 3 and (a["p"], a["q"]) == (steps[j][3], steps[j][4]) and not (set(a) & {"r", "u", "s"})
            c = (lv[j + 1] - lv[j]) / 2
            assert (b["p"], b["q"], b["r"], b["u"]) == (c / lv[j + 1], -c / lv[j + 1], -c / lv[j], 1 + c / lv[j]) and "save" not in b
            assert (b["a_skip"], b["a_out"]) == steps[j + 1][1:3]                                     # the denoiser of the NEXT grid point
            assert abs(b["p"] + b["q"] + b["r"] + b["u"] - 1.0) <= 1e-12
        assert not (set(ks[-1]) & NEW_KEYS) and (ks[-1]["p"], ks[-1]["q"]) == (0.0, 1.0)
        assert [k["clamp"] for k in ks] == [20000.0] * (len(ks) - 1) + [0.0]
    fl = _sampler("flow_matching")
    for N in (1, 4):
        _x0, steps = fl.schedule(N)
        lv, _ts = fl.grid(N)
        ks, tin, levels = S.solver_steps(steps, lv, "flow_matching", "heun")
        assert len(ks) == 2 * N - 1 and levels == [lv[0]] + [t for t in lv[1:N] for _ in (0, 1)]
        bf = lambda t: float(torch.tensor(t).to(torch.bfloat16))
        assert tin == [bf(t) for t in levels]
        for j in range(N - 1):
            dt = lv[j + 1] - lv[j]
            a, b = ks[2 * j], ks[2 * j + 1]
            assert (a["p"], a["q"], a["save"]) == (1.0, dt, 3)
            assert (b["q"], b["r"], b["u"]) == (dt / 2, dt / 2, 1.0) and b["p"] == 0.0 and "save" not in b
        assert not (set(ks[-1]) & NEW_KEYS)


def test_inpaint_scalars():
    """k_a known + k_b n is the kept region at the level the step's OUTPUT lives at: sigma' (0 after the last step), Heun's stage A too"""
    sm = _sampler()
    _x0, steps = sm.schedule(5)
    lv, _ts = sm.grid(5)
    for solver in ("euler", "euler_a", "dpmpp_2m"):
        ks = S.solver_steps(steps, lv, "ddpm", solver, inpaint=True)[0]
        assert [(k["k_a"], k["k_b"]) for k in ks] == [(1.0, s) for s in lv[1:]] + [(1.0, 0.0)]
    ks = S.solver_steps(steps, lv, "ddpm", "heun", inpaint=True)[0]
    assert [k["k_b"] for k in ks] == [s for s in lv[1:] for _ in (0, 1)] + [0.0]
    fl = _sampler("flow_matching")
    _x0, steps = fl.schedule(4)
    lv, _ts = fl.grid(4)
    ks = S.solver_steps(steps, lv, "flow_matching", "euler", inpaint=True)[0]
    assert [(k["k_a"], k["k_b"]) for k in ks] == [(t, 1.0 - t) for t in lv[1:]]
    ks = S.solver_steps(steps, lv, "flow_matching", "heun", inpaint=True)[0]
    assert [k["k_a"] for k in ks] == [0.25, 0.25, 0.5, 0.5, 0.75, 0.75, 1.0]


# ---------------------------------------------------------------------------------------------- 6. the calls sample() issues
class _RecNet:
    """stands in for NativeUNet: records sample_init / sample_step"""
    device = "cpu"

    def __init__(self):
        self.calls = []

    def sample_init(self, x, *a, **k):
        self.calls.append(("init", x.clone(), k))

    def sample_step(self, x, pe, po, ti, t, **k):
        self.calls.append(("step", float(t[0]), k))


def _cond(B=2, H=6, W=5, seed=0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(B, 77, 8, generator=g), torch.randn(B, 4, generator=g), torch.zeros(B, 6), torch.randn(B, 4, H, W, generator=g))


def _run(method="ddpm", **kw):
    net = _RecNet()
    sm = S.NativeSampler(net, method)
    pe, po, ti, noise = _cond()
    kw.setdefault("noise", noise)
    sm.sample(pe, po, ti, height=6, width=5, num_steps=kw.pop("num_steps", 4), guidance_scale=kw.pop("guidance_scale", 5.0), **kw)
    return sm, net.calls, noise


def test_sample_euler_issues_todays_calls():
    sm, calls, noise = _run()
    x0, steps = sm.schedule(4)
    assert [c[0] for c in calls] == ["init"] + ["step"] * 4
    assert [c[2] for c in calls[1:]] == S.kernel_steps(steps, 5.0, 0.0, True) and [c[1] for c in calls[1:]] == [s[6] for s in steps]
    assert torch.equal(calls[0][1], torch.tensor(x0, dtype=torch.float32) * noise)
    # strength = 1 with init_latents is the same call list
    _sm, again, _n = _run(init_latents=torch.ones(2, 4, 6, 5), strength=1.0)
    assert torch.equal(again[0][1], calls[0][1]) and [c[1:] for c in again[1:]] == [c[1:] for c in calls[1:]]


def test_sample_solver_calls():
    # euler_a: one draw per stochastic step, all from one randn behind the initial noise
    pe, po, ti, _n = _cond()
    net = _RecNet()
    sm = S.NativeSampler(net, "ddpm")
    sm.sample(pe, po, ti, height=6, width=5, num_steps=4, solver="euler_a", generator=torch.Generator().manual_seed(7))
    g = torch.Generator().manual_seed(7)
    n0, sn = torch.randn((2, 4, 6, 5), generator=g), torch.randn((3, 2, 4, 6, 5), generator=g)
    assert torch.equal(net.calls[0][1], torch.tensor(sm.schedule(4)[0], dtype=torch.float32) * n0)
    steps = [c[2] for c in net.calls[1:]]
    assert all(torch.equal(steps[j]["noise"], sn[j]) for j in range(3)) and "noise" not in steps[3] and "s" not in steps[3]
    given = torch.randn(3, 2, 4, 6, 5)
    _sm, calls, _n = _run(solver="euler_a", step_noise=given)
    assert all(torch.equal(calls[1 + j][2]["noise"], given[j]) for j in range(3))
    with pytest.raises(ValueError, match="step_noise"):
        _run(solver="euler_a", step_noise=given[:2])
    # dpmpp_2m: one hist buffer through the run, never xsave; heun: both, 2 (N - 1) + 1 forwards
    _sm, calls, _n = _run(solver="dpmpp_2m")
    hs = [c[2].get("hist") for c in calls[1:]]
    assert len(hs) == 4 and all(h is hs[0] and h is not None for h in hs) and all("xsave" not in c[2] for c in calls[1:])
    sm, calls, _n = _run(solver="heun")
    ks, tin, _lv = S.solver_steps(sm.schedule(4)[1], sm.grid(4)[0], "ddpm", "heun", 1.0, 5.0, 0.0, True)
    assert len(calls) == 1 + 7 and [c[1] for c in calls[1:]] == tin
    assert [{k: v for k, v in c[2].items() if not torch.is_tensor(v)} for c in calls[1:]] == ks
    assert all(("hist" in c[2]) == ("xsave" in c[2]) == bool(k.get("save") or k.get("r")) for c, k in zip(calls[1:], ks))


def test_sample_img2img_and_inpaint_start_state():
    init = torch.randn(2, 4, 6, 5, generator=torch.Generator().manual_seed(3))
    c = lambda v: torch.tensor(v, dtype=torch.float32)
    sm, calls, noise = _run(num_steps=6, init_latents=init, strength=0.5)
    lv, ts = sm.grid(6)
    assert len(calls) == 1 + 3 and [k[1] for k in calls[1:]] == ts[3:]
    assert torch.equal(calls[0][1], init + c(lv[3]) * noise)
    assert [k[2] for k in calls[1:]] == S.kernel_steps(sm.schedule(6)[1][3:], 5.0, 0.0, True)
    assert len(_run(num_steps=6, init_latents=init, strength=0.01)[1]) == 1 + 1                     # at least one grid point
    sm, calls, noise = _run("flow_matching", num_steps=4, init_latents=init, strength=0.5)
    assert len(calls) == 1 + 2 and torch.equal(calls[0][1], c(0.5) * noise + c(0.5) * init)
    mask = torch.zeros(2, 6, 5)
    mask[:, :3] = 1.0
    sm, calls, noise = _run(num_steps=4, init_latents=init, inpaint_mask=mask)
    lv, _ts = sm.grid(4)
    m4 = mask.reshape(2, 1, 6, 5)
    assert torch.equal(calls[0][1], X.blend(c(lv[0]) * noise, m4, init, noise, 1.0, lv[0]))
    for call, k_b in zip(calls[1:], lv[1:] + [0.0]):
        k = call[2]
        assert torch.equal(k["mask"], m4) and torch.equal(k["known"], init) and torch.equal(k["knoise"], noise)
        assert (k["k_a"], k.get("k_b", 0.0)) == (1.0, k_b)


# ---------------------------------------------------------------------------------------------- 7. errors
def test_solver_and_argument_errors():
    for solver, method, par in (("euler_a", "flow_matching", "trained"), ("dpmpp_2m", "flow_matching", "trained"),
                                ("euler_a", "ddpm", "reference"), ("dpmpp_2m", "ddpm", "reference"), ("heun", "ddpm", "reference")):
        with pytest.raises(ValueError, match=solver) as e:
            S.check_solver(solver, method, par)
        assert method in str(e.value)
        sm = S.NativeSampler(_RecNet(), method, parameterization=par)
        pe, po, ti, noise = _cond()
        with pytest.raises(ValueError, match=solver):
            sm.sample(pe, po, ti, height=6, width=5, num_steps=4, noise=noise, solver=solver)
        with pytest.raises(ValueError, match=solver):
            S.solver_steps(sm.schedule(4)[1], sm.grid(4)[0], method, solver, parameterization=par)
    with pytest.raises(ValueError, match="dpm_solver"):
        S.check_solver("dpm_solver", "ddpm")
    for ok in (("euler", "ddpm", "reference"), ("euler", "flow_matching", "trained"), ("heun", "flow_matching", "trained"),
               ("HEUN", "ddpm", "trained")):
        assert S.check_solver(*ok) == ok[0].lower()
    sm = _sampler()
    with pytest.raises(ValueError, match="eta"):
        S.solver_steps(sm.schedule(4)[1], sm.grid(4)[0], "ddpm", "euler_a", -0.5)
    with pytest.raises(ValueError, match="grid"):
        S.solver_steps(sm.schedule(4)[1], sm.grid(4)[0][:3], "ddpm", "heun")
    init, mask = torch.zeros(2, 4, 6, 5), torch.ones(2, 6, 5)
    for bad, msg in ((dict(inpaint_mask=mask), "init_latents"), (dict(strength=0.5), "init_latents"),
                     (dict(init_latents=init[:1]), "init_latents"), (dict(init_latents=init[:, :3]), "init_latents"),
                     (dict(init_latents=init, strength=0.0), "strength"), (dict(init_latents=init, strength=1.5), "strength"),
                     (dict(init_latents=init, strength=float("nan")), "strength"),
                     (dict(init_latents=init, inpaint_mask=torch.ones(2, 5, 6)), "inpaint_mask"),
                     (dict(init_latents=init, inpaint_mask=torch.ones(2, 2, 6, 5)), "inpaint_mask"),
                     (dict(init_latents=init, inpaint_mask=mask * 1.5), "inpaint_mask"),
                     (dict(init_latents=init, inpaint_mask=mask - 1.5), "inpaint_mask"),
                     (dict(init_latents=init, inpaint_mask=mask * float("nan")), "inpaint_mask"),
                     (dict(solver="euler_a", eta=-1.0), "eta")):
        with pytest.raises(ValueError, match=msg):
            _run(**bad)
    with pytest.raises(ValueError, match="init_latents"):
        sm = S.NativeSampler(_RecNet(), "ddpm", parameterization="reference")
        pe, po, ti, noise = _cond()
        sm.sample(pe, po, ti, height=6, width=5, num_steps=4, noise=noise, init_latents=init, strength=0.5)
    assert len(_run(init_latents=init, inpaint_mask=torch.ones(2, 1, 6, 5))[1]) == 5               # [B,1,H,W] is accepted


def test_trainer_keys():
    tc = CFG.Config().training
    assert (tc.validation_sampler, tc.validation_eta) == ("euler", 1.0)
    tr = _trainer()
    assert tr.validation_sampler == "euler"
    assert _trainer(validation_sampler="DPMPP_2M").validation_sampler == "dpmpp_2m"
    assert _trainer(method="flow_matching", validation_sampler="heun").validation_sampler == "heun"
    for bad in (dict(validation_sampler="ddim"), dict(validation_sampler="heun", sampler_parameterization="reference"),
                dict(validation_sampler="dpmpp_2m", method="flow_matching"), dict(validation_sampler="euler_a", method="flow_matching")):
        with pytest.raises(ValueError, match="validation_sampler"):
            _trainer(**bad)
    for bad in (-0.1, float("nan"), float("inf"), "1", True):
        with pytest.raises(ValueError, match="validation_eta"):
            _trainer(validation_eta=bad)

    class RefCfg:
        class training:
            method = "native_mi355x"
            validation_sampler = "heun"
            validation_eta = 0.5

    class M:
        unet = _FakeNet()
    tr = NM.NativeMI355XTrainer(M(), device="cpu", config=RefCfg)
    assert (tr.config.training.validation_sampler, tr.config.training.validation_eta, tr.validation_sampler) == ("heun", 0.5, "heun")


# ---------------------------------------------------------------------------------------------- 8. the struct and its checks
def test_extended_struct_mirror_matches_the_header():
    hdr = (ROOT / "include" / "sdxlstep.h").read_text()
    body = re.search(r"typedef struct \{([^}]*)\} sdxl_sampler_step_ext;", hdr).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        m = re.match(r"(sdxl_sampler_step|const float\*|float\*|int|float)\s+(.*)", decl.strip(), flags=re.S)
        if m:
            fields += [(n.strip(), m.group(1)) for n in m.group(2).split(",")]
    want = {"float*": C.c_void_p, "const float*": C.c_void_p, "int": C.c_int, "float": C.c_float}
    assert fields[0] == ("base", "sdxl_sampler_step") and issubclass(lib.SamplerStepExt, lib.SamplerStep)
    assert [(n, want[t]) for n, t in fields[1:]] == list(lib.SamplerStepExt._fields_)
    assert int(re.search(r"#define SDXL_SAMPLER_EXT (0x[0-9a-f]+)", hdr).group(1), 16) == lib.SAMPLER_EXT == 0x100
    E = lib.SamplerStepExt
    assert C.sizeof(lib.SamplerStep) == 48 and E.hist.offset == 48 and E.r.offset == 72 and E.save.offset == 84 and E.mask.offset == 88
    assert E.k_a.offset == 112 and C.sizeof(E) == 120
    # the positional construction of the plain step is what it was: no flag, and the extended one starts with the same fields
    s = lib.SamplerStep(None, 1, 0, 0.5, -2.0, 0.25, 0.75, 1.0, 20000.0, 5.0, 0.7)
    e = E(None, 1, 0, 0.5, -2.0, 0.25, 0.75, 1.0, 20000.0, 5.0, 0.7)
    assert s.init == 0 and bytes(s) == bytes(e)[:48] and bytes(e)[48:] == bytes(72)


def _ext(**kw):
    s = lib.SamplerStepExt(None, 0, lib.SAMPLER_EXT, 1.0, 1.0, 1.0, 1.0, 1.0, 0.0, 1.0, 0.0)
    for k, v in kw.items():
        setattr(s, k, v)
    return s


def bad_extended_arguments(ptr):
    """(field values, a word of the message) of every bad argument of the extended step; `ptr` is any non-NULL address"""
    nan, inf = float("nan"), float("inf")
    return [(dict(r=0.5), "hist"), (dict(save=1), "hist"), (dict(u=0.5), "xsave"), (dict(save=2), "xsave"), (dict(s=0.5), "noise"),
            (dict(mask=ptr), "known"), (dict(mask=ptr, known=ptr, k_b=0.5), "knoise"), (dict(k_b=0.5), "knoise"),
            (dict(r=nan, hist=ptr), "not finite"), (dict(u=inf, xsave=ptr), "not finite"), (dict(s=nan, noise=ptr), "not finite"),
            (dict(k_a=nan), "not finite"), (dict(k_b=-inf, knoise=ptr), "not finite"),
            (dict(save=4, hist=ptr, xsave=ptr), "save"), (dict(save=-1, hist=ptr, xsave=ptr), "save"),
            (dict(init=lib.SAMPLER_EXT | 2), "init"), (dict(init=lib.SAMPLER_EXT | 0x200), "init")]


def test_extended_argument_errors_are_reported_before_any_launch():
    """no device is touched: every bad argument of the extended struct returns 1 with a message; without the flag nothing behind
    guidance_rescale is read (junk there is not an error), and init's other bits are refused either way"""
    L = lib.load()
    buf = (C.c_char * 256)()
    p16 = (C.addressof(buf) + 15) & ~15
    vp = C.c_void_p(p16)
    for kw, msg in bad_extended_arguments(p16):
        rc = L.sdxl_op_sampler_step(vp, vp, vp, 1, 8, 8, C.byref(_ext(**kw)), None)
        assert rc == 1 and msg.encode() in L.sdxl_last_error(), (kw, L.sdxl_last_error())
    plain = lib.SamplerStep(None, 0, 2, 1.0, 1.0, 1.0, 1.0, 1.0, 0.0, 1.0, 0.0)
    assert L.sdxl_op_sampler_step(vp, vp, vp, 1, 8, 8, C.byref(plain), None) == 1 and b"init" in L.sdxl_last_error()
    junk = _ext(r=float("nan"), save=77, k_b=3.0, init=0)            # no flag: the tail is not read ...
    junk.a_skip = float("nan")                                       # ... so the first error is the plain struct's
    assert L.sdxl_op_sampler_step(vp, vp, vp, 1, 8, 8, C.byref(junk), None) == 1 and b"scalar 0 of (a_skip" in L.sdxl_last_error()
