"""CPU checks of the native sampler's host side: the reference's sampling functions against recorded outputs, the parameter sets
against the training loss they belong to, the schedules, the config keys and the C struct mirror."""
import ctypes as C
import importlib
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import _sampler_ref as R
import sdxl_amd  # noqa: F401
from sdxl_amd import lib

S = importlib.import_module("sdxl-training-improvements_amd.sampler")
T = importlib.import_module("sdxl-training-improvements_amd.trainer")
NM = importlib.import_module("sdxl-training-improvements_amd.native_mi355x")
CFG = importlib.import_module("sdxl-training-improvements_amd.config")
SCH = importlib.import_module("sdxl-training-improvements_amd.scheduler")

ROOT = Path(__file__).resolve().parent.parent
EPS32 = 2.0 ** -24


@pytest.fixture(scope="module")
def gold():
    return np.load(ROOT / "tests" / "golden" / "sampler_reference.npz", allow_pickle=False)


def stub_model(x, _sigma=None):
    return torch.tanh(0.5 * x) + 0.1


# ---------------------------------------------------------------------------------------------- 1. the reference's functions
def test_reference_functions_bit_for_bit(gold):
    """get_karras_scalings, ztsnr_first_step, euler_step and a whole sample_with_ztsnr run of the reference's NoiseScheduler
    (tests/make_sampler_goldens.py) against their restatement in fp32 torch: the same ops in the same order, so the same bits"""
    t = lambda k: torch.from_numpy(gold[k])
    sig = t("sigmas")
    assert np.array_equal(SCH.get_karras_sigmas(6, 0.002, 20000.0, 7.0).numpy(), gold["sigmas"])      # karras(N), rho = 7
    for got, key in zip(R.get_karras_scalings(t("ks_sigma")), ("ks_c_skip", "ks_c_out", "ks_c_in")):
        assert np.array_equal(got.numpy(), gold[key]), key
    assert np.array_equal(R.ztsnr_first_step(t("fs_n"), sig[0], stub_model).numpy(), gold["fs_out"])
    for k, (i, j) in enumerate(gold["es_pairs"]):
        assert np.array_equal(R.euler_step(t(f"es{k}_x"), sig[i], sig[j], stub_model).numpy(), gold[f"es{k}_out"]), k
    out = R.sample_with_ztsnr(stub_model, t("run_n"), sig)
    assert out.shape == (2, 4, 8, 8) and np.array_equal(out.numpy(), gold["run_out"])


def test_reference_parameter_set_is_the_reference_run(gold):
    """The "reference" parameter set drives the GENERIC step (what the kernel computes): its first step is ztsnr_first_step bit for
    bit; its Euler steps are p x + q den where the reference writes x + (sigma' - sigma) ((x - den) / sigma) -- the same arithmetic
    in another order -- so they agree to fp32 rounding, not to the bit.  The bound is derived, per element and step:
      reference form: x - den, / sigma, sigma' - sigma, the product, the sum        5 roundings of terms <= |x| + |den|
      generic form:   p and q rounded to fp32, two products, the sum                  5 roundings of terms <= |x| + |den|
      scalings in double (here) against fp32 (reference): <= 3 eps each on c_skip x, c_out F, and through c_in into the stand-in
      model, whose slope is <= 1/2: |c_out| c_in |x| / 2 * 3 eps <= 1.5 eps |x|
    under 16 eps (|x| + |c_out F|) in all, eps = 2^-24.  Over the run the difference e obeys e' <= A e + b with b that bound at the
    step's largest |x|, |F| and A = p + q (c_skip + |c_out| c_in / 2), the step's Lipschitz constant for this model."""
    t = lambda k: torch.from_numpy(gold[k])
    sig = [float(s) for s in gold["sigmas"]]
    x0_scale, steps = S.ddpm_reference_steps(sig, [0.0] * len(sig))
    assert x0_scale == 1.0 and len(steps) == len(sig)
    # the first step alone, bit for bit
    first = R.step(t("fs_n"), stub_model(R.unet_input(t("fs_n"), 1.0, 0.0, quantize=False)), *steps[0][1:5])
    assert steps[0][:6] == (1.0, 0.0, -1.0, sig[0], 1.0, 0.0) and np.array_equal(first.numpy(), gold["fs_out"])
    # single Euler steps from the recorded x
    for k, (i, j) in enumerate(gold["es_pairs"]):
        c_skip, c_out, c_in = S.karras_scalings(sig[i])
        x = t(f"es{k}_x")
        F = stub_model(R.unet_input(x, c_in, 0.0, quantize=False))
        got = R.step(x, F, c_skip, c_out, sig[j] / sig[i], 1.0 - sig[j] / sig[i])
        bound = 16 * EPS32 * (x.abs() + abs(c_out) * F.abs())
        diff = (got - t(f"es{k}_out")).abs()
        print(f"euler step {k}: max diff {float(diff.max()):.3e}, bound at that element {float(bound.flatten()[diff.argmax()]):.3e}")
        assert bool((diff <= bound).all())
    # the whole run
    out = R.sample_loop(lambda inp, _t, _j: stub_model(inp), t("run_n"), x0_scale, steps, quantize=False)
    # the recurrence on the states of the literal run
    x = R.ztsnr_first_step(t("run_n"), t("sigmas")[0], stub_model)
    e = 0.0
    for j in range(1, len(sig)):
        a_in, a_skip, a_out, p, q, _c, _t = steps[j]
        b = 16 * EPS32 * (float(x.abs().max()) + abs(a_out) * 1.1)          # |stub_model| <= 1.1
        e = (abs(p) + abs(q) * (a_skip + abs(a_out) * a_in / 2)) * e + b
        x = R.euler_step(x, t("sigmas")[j - 1], t("sigmas")[j], stub_model)
    diff = float((out - t("run_out")).abs().max())
    print(f"whole run: max diff {diff:.3e}, bound {e:.3e}, max |x| {float(t('run_out').abs().max()):.3e}")
    assert diff <= e and diff > 0.0            # (> 0: it really is another order of operations, not the literal run)


# ---------------------------------------------------------------------------------------------- 2. trained = the loss's denoiser
def _ideal(kind, xstar, x0noise=None):
    """the model that returns the training target of a fixed x*: what a perfectly trained network would, given the input alone"""
    def v_model(inp, sigma):
        return (inp - xstar * (1.0 + sigma)) / sigma ** 2          # x_t = (1 + s) x* + s^2 v
    def eps_model(inp, sigma):
        return (inp - xstar) / sigma                               # x_t = x* + s eps
    def flow_model(inp, _t):
        return xstar - x0noise                                     # the velocity x1 - x0 of the path from this noise
    return {"v_prediction": v_model, "epsilon": eps_model, "flow": flow_model}[kind]


@pytest.mark.parametrize("N", [2, 8, 30])
@pytest.mark.parametrize("kind", ["v_prediction", "epsilon", "flow"])
def test_trained_parameterization_samples_the_ideal_model_back(kind, N):
    g = torch.Generator().manual_seed(100 + N)
    xstar = torch.randn(2, 4, 8, 8, generator=g, dtype=torch.float64) * 3.0
    n = torch.randn(2, 4, 8, 8, generator=g, dtype=torch.float64)
    table = SCH.NoiseScheduler(CFG.Config(), "cpu").sigmas
    if kind == "flow":
        x0_scale, steps = S.flow_steps(N, t_bf16=False)
        model = _ideal("flow", xstar, n)
        out = R.sample_loop(lambda inp, t, j: model(inp, t), n, x0_scale, steps, quantize=False)
    else:
        idx = S.ddpm_indices(N)
        sig = [float(table[i]) for i in idx]
        x0_scale, steps = S.ddpm_trained_steps(sig, [float(i) for i in idx], kind, use_ztsnr=False)
        model = _ideal(kind, xstar)
        out = R.sample_loop(lambda inp, t, j: model(inp, sig[j]), n, x0_scale, steps, quantize=False)
    err = float((out - xstar).abs().max())
    print(f"{kind} N={N}: max |x - x*| = {err:.3e}  (bound {1e-9 * float(xstar.abs().max()):.3e})")
    assert out.dtype == torch.float64 and err <= 1e-9 * float(xstar.abs().max())


@pytest.mark.parametrize("N", [2, 8, 30])
def test_reference_parameterization_is_not_the_training_denoiser(N):
    """the documented inconsistency: under "reference" (scaled input, EDM scalings) the ideal v-model of the training loss is NOT
    sampled back to x*.  The gap is O(|x*|): here it must exceed a tenth of max |x*|."""
    g = torch.Generator().manual_seed(200 + N)
    xstar = torch.randn(2, 4, 8, 8, generator=g, dtype=torch.float64) * 3.0
    n = torch.randn(2, 4, 8, 8, generator=g, dtype=torch.float64)
    table = SCH.NoiseScheduler(CFG.Config(), "cpu").sigmas
    idx = S.ddpm_indices(N)
    sig = [float(table[i]) for i in idx]
    x0_scale, steps = S.ddpm_reference_steps(sig, [float(i) for i in idx])
    fed = [sig[0]] + sig[:-1]                                       # forward j runs at sigma_{j-1} (the first at sigma_0)
    model = _ideal("v_prediction", xstar)
    out = R.sample_loop(lambda inp, t, j: model(inp, fed[j]), n, x0_scale, steps, quantize=False)
    gap = float((out - xstar).abs().max())
    print(f"reference N={N}: max |x - x*| = {gap:.3e}, max |x*| = {float(xstar.abs().max()):.3e}")
    assert gap > 0.1 * float(xstar.abs().max())


# ---------------------------------------------------------------------------------------------- 3. schedules
def test_ddpm_schedule():
    table = SCH.NoiseScheduler(CFG.Config(), "cpu").sigmas
    assert S.ddpm_indices(2) == [0, 999] and S.ddpm_indices(4) == [0, 333, 666, 999] and S.ddpm_indices(30)[:3] == [0, 34, 69]
    idx = S.ddpm_indices(30)
    assert idx == [int(round(999 * j / 29)) for j in range(30)] and idx[-1] == 999
    with pytest.raises(ValueError):
        S.ddpm_indices(1)
    sm = S.NativeSampler(None, "ddpm", "v_prediction", True, "trained")
    x0_scale, steps = sm.schedule(8)
    idx = S.ddpm_indices(8)
    sig = [float(table[i]) for i in idx]
    assert x0_scale == sig[0] == float(table[0]) and len(steps) == 8
    assert [s[6] for s in steps] == [float(i) for i in idx]                       # the time input is the table index
    assert all(s[0] == 1.0 and s[5] == 20000.0 for s in steps)                    # unscaled input, the ZTSNR clamp
    for j, (a_in, a_skip, a_out, p, q, clamp, t) in enumerate(steps[:-1]):
        assert a_skip == 1 / (1 + sig[j]) and a_out == -sig[j] ** 2 / (1 + sig[j]) and p == sig[j + 1] / sig[j] and q == 1 - p
    assert steps[-1][3:5] == (0.0, 1.0)                                           # sigma_N = 0: x = den
    x = torch.randn(1, 4, 4, 4, dtype=torch.float64)
    F = torch.randn(1, 4, 4, 4, dtype=torch.float64)
    a_skip, a_out = steps[-1][1:3]
    assert torch.equal(R.step(x, F, a_skip, a_out, 0.0, 1.0), a_skip * x + a_out * F)
    # epsilon, no clamp without ztsnr
    _x0, st = S.NativeSampler(None, "ddpm", "epsilon", False, "trained").schedule(4)
    assert all(s[1] == 1.0 and s[5] == 0.0 for s in st) and st[0][2] == -_x0
    # explicit override: sigmas with and without timesteps
    x0_scale, steps = sm.schedule(99, sigmas=[100.0, 10.0, 1.0], timesteps=[5.0, 6.0, 7.0])
    assert x0_scale == 100.0 and [s[6] for s in steps] == [5.0, 6.0, 7.0] and steps[0][3] == 0.1 and steps[-1][3] == 0.0
    _x0, steps = sm.schedule(99, sigmas=[float(table[10]), float(table[500])])
    assert [s[6] for s in steps] == [10.0, 500.0]                                 # nearest table index
    _x0, steps = sm.schedule(99, timesteps=[0, 500, 999])
    assert [s[6] for s in steps] == [0.0, 500.0, 999.0] and _x0 == float(table[0])
    # reference: N forwards for N sigmas, the first on n itself, no step to zero
    ref = S.NativeSampler(None, "ddpm", "v_prediction", True, "reference")
    x0_scale, steps = ref.schedule(6)
    sig = [float(table[i]) for i in S.ddpm_indices(6)]
    assert x0_scale == 1.0 and len(steps) == 6 and steps[0][:6] == (1.0, 0.0, -1.0, sig[0], 1.0, 0.0)
    assert [s[6] for s in steps] == [0.0] + [float(i) for i in S.ddpm_indices(6)[:-1]]
    c_skip, c_out, c_in = S.karras_scalings(sig[2])
    assert steps[3][:6] == (c_in, c_skip, c_out, sig[3] / sig[2], 1 - sig[3] / sig[2], 0.0) and steps[-1][3] > 0.0


def test_flow_schedule():
    x0_scale, steps = S.NativeSampler(None, "flow_matching").schedule(8)
    assert x0_scale == 1.0 and len(steps) == 8
    assert [s[6] for s in steps] == [float(torch.tensor(j / 8).to(torch.bfloat16)) for j in range(8)]
    assert all(s[:4] == (1.0, 0.0, 1.0, 1.0) and s[5] == 0.0 for s in steps)
    assert [s[4] for s in steps] == [(j + 1) / 8 - j / 8 for j in range(8)]
    _x0, st = S.flow_steps(3, t_bf16=False)
    assert [s[6] for s in st] == [0.0, 1 / 3, 2 / 3]
    _x0, st = S.flow_steps(0, timesteps=[0.0, 0.5, 1.0])
    assert [s[4] for s in st] == [0.5, 0.5]
    with pytest.raises(ValueError):
        S.NativeSampler(None, "flow_matching").schedule(4, sigmas=[1.0])


def test_plan_batch_and_kernel_steps():
    assert S.NativeSampler.plan_batch(3, 1.0) == 3 and S.NativeSampler.plan_batch(3, 5.0) == 6 and S.NativeSampler.plan_batch(2, 0.0) == 4
    _x0, steps = S.NativeSampler(None, "ddpm").schedule(3)
    ks = S.kernel_steps(steps, 5.0, 0.7, True)
    assert [k["a_in_next"] for k in ks] == [1.0, 1.0, 1.0] and [k["clamp"] for k in ks] == [20000.0, 20000.0, 0.0]
    assert all(k["cfg"] == 1 and k["guidance"] == 5.0 and k["guidance_rescale"] == 0.7 and k["init"] == 0 for k in ks)
    ks = S.kernel_steps(steps, 1.0, 0.0, False)
    assert all(k["cfg"] == 0 and k["guidance"] == 1.0 for k in ks)
    _x0, rsteps = S.NativeSampler(None, "ddpm", parameterization="reference").schedule(3)
    ks = S.kernel_steps(rsteps, 1.0, 0.0, False)
    assert [k["a_in_next"] for k in ks] == [rsteps[1][0], rsteps[2][0], 1.0]


# ---------------------------------------------------------------------------------------------- 4. validation of keys, the struct
class _FakeNet:
    param_elems = 16
    device = "cpu"

    def __init__(self):
        self.grads = torch.zeros(16)
        self.weights = torch.zeros(16, dtype=torch.bfloat16)

    def forward_loss(self, *a, **k): pass
    def backward(self, *a, **k): pass
    def read_loss(self): return [0.0] * 8
    def zero_grads(self): pass


def _trainer(**keys):
    cfg = CFG.Config()
    for k, v in keys.items():
        setattr(cfg.training, k, v)
    class M:
        unet = _FakeNet()
    return T.NativeSDXLTrainer(M(), optimizer=None, train_dataloader=None, device="cpu", config=cfg)


def test_config_defaults_and_bad_keys():
    tc = CFG.Config().training
    assert (tc.validation_every_n_steps, tc.validation_num_steps, tc.validation_guidance_scale, tc.validation_guidance_rescale,
            tc.validation_weights, tc.validation_seed, tc.sampler_parameterization) == (0, 30, 5.0, 0.0, None, 0, "trained")
    tr = _trainer()
    assert tr.validation_weights == "trained" and tr.sampler_parameterization == "trained"
    for bad in (dict(sampler_parameterization="edm"), dict(validation_weights="best"), dict(validation_weights="ema"),
                dict(validation_every_n_steps=-1), dict(validation_every_n_steps=1.5), dict(validation_num_steps=1),
                dict(validation_num_steps="30"), dict(validation_guidance_scale=float("nan")), dict(validation_guidance_scale="5"),
                dict(validation_guidance_rescale=1.5), dict(validation_guidance_rescale=-0.1), dict(validation_seed=1.5)):
        with pytest.raises(ValueError, match=next(iter(bad))):
            _trainer(**bad)
    assert _trainer(method="flow_matching", validation_num_steps=1).method == "flow_matching"      # one Euler step is a flow sampler
    for bad in (dict(method="sde"), dict(prediction_type="x0"), dict(parameterization="edm")):
        with pytest.raises(ValueError):
            S.NativeSampler(None, **bad)
    with pytest.raises(ValueError, match="weights"):
        with _trainer()._weights("best"):
            pass
    with pytest.raises(ValueError, match="no EMA"):
        with _trainer()._weights("ema"):
            pass


def test_drop_in_copies_the_keys():
    class RefCfg:
        class training:
            method = "native_mi355x"
            validation_every_n_steps = 50
            validation_num_steps = 12
            validation_guidance_scale = 3.0
            validation_guidance_rescale = 0.7
            validation_seed = 9
            sampler_parameterization = "reference"
    class M:
        unet = _FakeNet()
    tr = NM.NativeMI355XTrainer(M(), device="cpu", config=RefCfg)
    tc = tr.config.training
    assert (tc.validation_every_n_steps, tc.validation_num_steps, tc.validation_guidance_scale, tc.validation_guidance_rescale,
            tc.validation_seed, tc.sampler_parameterization) == (50, 12, 3.0, 0.7, 9, "reference")
    assert tr.sampler_parameterization == "reference" and tr.validation_weights == "trained"


def test_struct_mirror_matches_the_header():
    hdr = (ROOT / "include" / "sdxlstep.h").read_text()
    body = re.search(r"typedef struct \{([^}]*)\} sdxl_sampler_step;", hdr).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        m = re.match(r"(float\*|int|float)\s+(.*)", decl.strip(), flags=re.S)
        if m:
            fields += [(n.strip(), m.group(1)) for n in m.group(2).split(",")]
    want = {"float*": C.c_void_p, "int": C.c_int, "float": C.c_float}
    assert [f[0] for f in fields] == ["x", "cfg", "init", "a_skip", "a_out", "p", "q", "a_in_next", "clamp", "guidance", "guidance_rescale"]
    assert [(n, want[t]) for n, t in fields] == [(n, t) for n, t in lib.SamplerStep._fields_]
    assert C.sizeof(lib.SamplerStep) == 8 + 2 * 4 + 8 * 4 and lib.SamplerStep.cfg.offset == 8 and lib.SamplerStep.a_skip.offset == 16
    # sdxl_batch: the pointer is the LAST member, right behind per_sample_loss; lib.Batch itself did not change
    batch = re.search(r"typedef struct \{((?:[^}]|\}(?! sdxl_batch;))*)\} sdxl_batch;", hdr).group(1)
    batch = re.sub(r"/\*.*?\*/", "", batch, flags=re.S)
    decls = [d.strip() for d in batch.split(";") if d.strip()]
    assert decls[-1] == "const sdxl_sampler_step* sampler" and decls[-2].endswith("per_sample_loss")
    assert [f[0] for f in lib.Batch._fields_][-1] == "per_sample_loss" and C.sizeof(lib.Batch) == 16 + 11 * C.sizeof(C.c_void_p)
    assert issubclass(lib.SamplerBatch, lib.Batch) and lib.SamplerBatch.sampler.offset == C.sizeof(lib.Batch)
    assert C.sizeof(lib.SamplerBatch) == C.sizeof(lib.Batch) + C.sizeof(C.c_void_p)
    b = lib.SamplerBatch(2, 8, 8, 77, None, None, None, None, None, None, None, None)
    assert not b.sampler and b.per_sample_loss is None                          # NULL unless set
    s = lib.SamplerStep(None, 1, 0, 0.5, -2.0, 0.25, 0.75, 1.0, 20000.0, 5.0, 0.7)
    b.sampler = C.pointer(s)
    assert b.sampler.contents.guidance == 5.0 and b.sampler.contents.clamp == 20000.0
    assert lib.SIGNATURES["sdxl_unet_forward"][2] == C.POINTER(lib.SamplerBatch)
    assert "sdxl_op_sampler_step" in lib.TEST_HOOK_SIGNATURES and "sdxl_op_sampler_step" not in lib.SIGNATURES


def test_sampler_argument_errors_are_reported_before_any_launch():
    """the hook shares sdxl_unet_forward's checks: x == NULL and non-finite scalars return 1 with a message (no device is touched)"""
    L = lib.load()
    buf = (C.c_char * 256)()
    p16 = C.c_void_p((C.addressof(buf) + 15) & ~15)
    s = lib.SamplerStep(None, 0, 0, 1.0, 1.0, 1.0, 1.0, 1.0, 0.0, 1.0, 0.0)
    assert L.sdxl_op_sampler_step(None, p16, p16, 1, 8, 8, C.byref(s), None) == 1 and b"x is NULL" in L.sdxl_last_error()
    assert L.sdxl_op_sampler_step(p16, p16, p16, 1, 8, 8, None, None) == 1
    assert L.sdxl_op_sampler_step(p16, p16, p16, 0, 8, 8, C.byref(s), None) == 1
    for field in ("a_skip", "a_out", "p", "q", "a_in_next", "clamp", "guidance", "guidance_rescale"):
        t = lib.SamplerStep(None, 0, 0, 1.0, 1.0, 1.0, 1.0, 1.0, 0.0, 1.0, 0.0)
        setattr(t, field, float("nan") if field != "p" else float("inf"))
        assert L.sdxl_op_sampler_step(p16, p16, p16, 1, 8, 8, C.byref(t), None) == 1 and b"not finite" in L.sdxl_last_error(), field
