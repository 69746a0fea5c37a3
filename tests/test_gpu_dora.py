"""DoRA adapters (SDXL_DTYPE_DORA, training.lora_algo "dora") on a real MI355X: the kernels of csrc/dora.hip through their single-target
hook on native buffers -- exact designs (bit equality whatever the summation order), the merged weight bit-equal to the restatement of
tests/_dora_ref.py GIVEN the norms the device wrote, every output within the bound accumulated next to the float64 reference, launch
properties and operand isolation -- then through sdxl_load_weight / sdxl_export_grad on the tiny UNet's handle with every kind of target,
the oracle at the merged weights, and the trainer.  Each case prints the largest fraction of its bound it needed as a `[dora]` line
(profiles/ops_dora.txt keeps them)."""
import ctypes as C
import importlib

import pytest
import torch

import sdxl_amd  # noqa: F401
from oracle import loss_ref as R
from oracle import unet_ref as U
from sdxl_amd import lib
from sdxl_amd import unet as NU

import _dora_ref as DR
from _gradparity import GradParity
from _isolation import Spec, assert_isolated, run_isolated, same_bits
from test_gpu_lora_layouts import (ALL_KINDS_TARGETS, flat2, kind_of, make_batch, make_trainer, native_micro, step_args, target_mask,
                                   tiny_native_cfg)

pytestmark = pytest.mark.gpu
LORA = importlib.import_module("sdxl-training-improvements_amd.lora")

GRAD_BAR = (6e-2, 0.995)          # GRAD_BAR of tests/test_gpu_lora.py
DEV = "cuda"
PLAIN, CONV3, GEGLU = DR.PLAIN, DR.CONV3, DR.GEGLU
CASES, BY_LABEL, FORMS, FORM_IDS = DR.CASES, DR.BY_LABEL, DR.FORMS, DR.FORM_IDS

bf = lambda t: t.to(torch.bfloat16)
ptr = lambda t: None if t is None else t.data_ptr()
stream = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)
f32 = torch.float32


def one(case, rank, mode, scale, **ptrs):
    _label, kind, out, inn, group = case
    return lib.DoraOne(out=out, in_=inn, group=group, kind=kind, rank=rank, mode=mode, scale=scale, **ptrs)


def load(o):
    return lib.load().sdxl_load_weight(None, None, C.byref(o), lib.DTYPE_DORA_ONE, stream())


def export(o):
    return lib.load().sdxl_export_grad(None, None, C.byref(o), lib.DTYPE_DORA_ONE, stream())


def nan(*shape, dtype=f32):
    return torch.full(shape, float("nan"), dtype=dtype, device=DEV)


def dev_init(case, W0n):
    n0 = nan(case[2])
    lib.check(load(one(case, 1, lib.DORA_INIT, 0.0, base=ptr(W0n), norm0=ptr(n0))), "dora init")
    return n0


def dev_merge(case, W0n, A, B, mu, s, n0):
    w, n = nan(*W0n.shape, dtype=torch.bfloat16), nan(case[2])
    lib.check(load(one(case, A.shape[0], lib.DORA_MERGE, s, base=ptr(W0n), A=ptr(A), B=ptr(B), mu=ptr(mu), w=ptr(w), norm0=ptr(n0), norm=ptr(n))),
              "dora merge")
    return w, n


def dev_restore(case, W0n):
    w = nan(*W0n.shape, dtype=torch.bfloat16)
    lib.check(load(one(case, 1, lib.DORA_RESTORE, 123.0, base=ptr(W0n), w=ptr(w))), "dora restore")
    return w


def dev_project(case, Gn, W0n, A, B, mu, s, n0, n):
    out = {"mu": nan(*mu.shape), "B": nan(*B.shape), "A": nan(*A.shape)}
    lib.check(export(one(case, A.shape[0], 0, s, dw=ptr(Gn), base=ptr(W0n), A=ptr(A), B=ptr(B), mu=ptr(mu), norm0=ptr(n0), norm=ptr(n),
                         dA=ptr(out["A"]), dB=ptr(out["B"]), dmu=ptr(out["mu"]))), "dora project")
    return out


def operands(case, rank, seed=0, b_std=0.3):
    """SOURCE-view W0, G ~ N(0, 1), A ~ N(0, 1), B ~ N(0, b_std^2), mu ~ N(0, 0.1^2), on the CPU; W0 holds -0 at two corners"""
    _label, kind, out, inn, group = case
    g = torch.Generator().manual_seed(1000 * seed + 7 * out + inn + rank + 31 * kind)
    r = lambda *s: torch.randn(*s, generator=g)
    W0 = bf(r(out, inn))
    W0[0, 0] = W0[out - 1, inn - 1] = -0.0
    return dict(W0=W0, G=r(out, inn), A=bf(r(rank, inn)), B=bf(r(out, rank) * b_std), mu=bf(r(out) * 0.1))


def on_device(case, x):
    """the device copies: W0 and G NATIVE, the adapters as they are"""
    _label, kind, _out, _inn, group = case
    d = {k: v.to(DEV) for k, v in x.items()}
    d["W0"], d["G"] = DR.to_native(x["W0"], kind, group).to(DEV), DR.to_native(x["G"], kind, group).to(DEV)
    return d


def src(case, t):
    return DR.to_source(t.cpu(), case[1], case[4])


def ratio(got, ref, delta):
    """(max |err| / delta, every element inside)"""
    err = (got.double().cpu() - ref).abs()
    assert bool(torch.isfinite(got).all()) and got.shape == ref.shape
    return float((err / delta.clamp_min(1e-300)).max()), bool((err <= delta).all())


# ------------------------------------------------------------------------------------------------ exact designs
@pytest.mark.parametrize("case,rank", FORMS, ids=FORM_IDS)
def test_exact_designs_have_the_bits_of_exact_arithmetic_in_any_order(case, rank):
    label, kind, out, inn, group = case
    W0, A, B, G = DR.exact_design(out, inn, rank)
    mu = bf(torch.randint(-2, 3, (out,), generator=torch.Generator().manual_seed(out + 3 * rank)).float() * 0.25)
    d = on_device(case, dict(W0=W0, G=G, A=A, B=B, mu=mu))
    v = W0.double() + B.double() @ A.double()                             # integers
    # the correctly rounded roots of integers: the float64 root rounded to fp32 (torch's own fp32 sqrt on the host is not correctly rounded)
    want_n0, want_n = W0.double().pow(2).sum(1).sqrt().float(), v.pow(2).sum(1).sqrt().float()
    n0 = dev_init(case, d["W0"])
    w, n = dev_merge(case, d["W0"], d["A"], d["B"], d["mu"], 1.0, n0)
    assert same_bits(n0.cpu(), want_n0) and same_bits(n.cpu(), want_n), label
    assert same_bits(src(case, w), DR.merge_given(W0, A, B, mu, 1.0, want_n0, want_n)), label
    got = dev_project(case, d["G"], d["W0"], d["A"], d["B"], d["mu"], 1.0, n0, n)
    r = (G.double() * v).sum(1).float()                                    # an integer
    q, _c = DR.coef32(mu, want_n0, want_n)
    assert same_bits(got["mu"].cpu(), q * r), label


@pytest.mark.parametrize("mu", [0.0, 0.5, -0.5, 1.0])
def test_rows_of_plus_minus_one_are_scaled_by_one_plus_mu_exactly(mu):
    case = ("16x64", PLAIN, 16, 64, 0)
    g = torch.Generator().manual_seed(3)
    W0 = bf(torch.randint(0, 2, (16, 64), generator=g).float() * 2 - 1)
    A, B, m = bf(torch.randn(4, 64, generator=g)), bf(torch.zeros(16, 4)), bf(torch.full((16,), mu))
    n0 = dev_init(case, W0.to(DEV))
    assert bool((n0 == 8).all())
    w, n = dev_merge(case, W0.to(DEV), A.to(DEV), B.to(DEV), m.to(DEV), 1.0, n0)
    assert bool((n == 8).all()) and same_bits(w.cpu(), bf((1 + mu) * W0.float()))


# ------------------------------------------------------------------------------------------------ merge
@pytest.mark.parametrize("case,rank", FORMS, ids=FORM_IDS)
def test_merge_is_the_restatement_given_the_devices_norms_and_everything_is_inside_its_bound(case, rank):
    label, kind, out, inn, group = case
    x = operands(case, rank)
    d = on_device(case, x)
    n0 = dev_init(case, d["W0"])
    worst = {}
    for s in (0.37, 1.0):
        w, n = dev_merge(case, d["W0"], d["A"], d["B"], d["mu"], s, n0)
        want = DR.merge_given(x["W0"], x["A"], x["B"], x["mu"], s, n0.cpu(), n.cpu())
        assert same_bits(src(case, w), want), (label, rank, s)
        assert not same_bits(w, d["W0"])
        ref, delta = DR.ref64(x["W0"], x["A"], x["B"], x["mu"], s), DR.bounds(x["W0"], x["A"], x["B"], x["mu"], s)
        assert bool(torch.isfinite(delta["W"]).all())
        worst["norm0"], ok0 = ratio(n0, ref["n0"], delta["n0"])
        worst["norm"], ok1 = ratio(n, ref["n"], delta["n"])
        lo, hi = DR.bf16_interval(ref["W"], delta["W"])
        got = src(case, w).float()
        inside = bool(((lo.float() <= got) & (got <= hi.float())).all())
        print(f"[dora] merge {label} r{rank} s={s}: max |err| / delta norm0 {worst['norm0']:.4f} norm {worst['norm']:.4f}; W inside its interval: {inside}")
        assert ok0 and ok1 and inside, (label, rank, s, worst)
        w2, n2 = dev_merge(case, d["W0"], d["A"], d["B"], d["mu"], s, n0)                 # run to run
        assert same_bits(w, w2) and same_bits(n, n2)
    # B = 0 and mu = 0: W0's bits, the planted -0s included; restore: W0's bits whatever the factors
    z = torch.zeros_like
    assert bool(torch.signbit(x["W0"][0, 0])) and bool(torch.signbit(x["W0"][-1, -1]))
    w, n = dev_merge(case, d["W0"], d["A"], z(d["B"]), z(d["mu"]), 0.37, n0)
    assert same_bits(w, d["W0"]) and same_bits(n, n0)
    assert same_bits(dev_restore(case, d["W0"]), d["W0"])


def test_a_zero_row_gives_q_one_and_no_nan():
    case = BY_LABEL["40x24"]
    x = operands(case, 3)
    x["W0"][5] = 0
    x["B"][5] = 0
    d = on_device(case, x)
    n0 = dev_init(case, d["W0"])
    w, n = dev_merge(case, d["W0"], d["A"], d["B"], d["mu"], 0.37, n0)
    assert float(n0[5]) == 0.0 and float(n[5]) == 0.0 and bool(torch.isfinite(w.float()).all()) and bool((w[5] == 0).all())
    got = dev_project(case, d["G"], d["W0"], d["A"], d["B"], d["mu"], 0.37, n0, n)
    assert all(bool(torch.isfinite(t).all()) for t in got.values()) and float(got["mu"][5]) == 0.0
    c5 = 1.0 + float(x["mu"][5])                                           # q = 1: dB's row is LoRA's times (1 + mu)
    want = DR.project64(x["G"], x["W0"], x["A"], x["B"], x["mu"], 0.37)["B"][5]
    assert torch.allclose(got["B"][5].double().cpu(), want, rtol=1e-4, atol=1e-5) and c5 != 1.0


# ------------------------------------------------------------------------------------------------ project
@pytest.mark.parametrize("case,rank", FORMS, ids=FORM_IDS)
def test_project_is_within_the_accumulated_bound_overwrites_and_repeats(case, rank):
    label, kind, out, inn, group = case
    x = operands(case, rank, seed=1)
    d = on_device(case, x)
    s = 0.37
    n0 = dev_init(case, d["W0"])
    _w, n = dev_merge(case, d["W0"], d["A"], d["B"], d["mu"], s, n0)
    got = dev_project(case, d["G"], d["W0"], d["A"], d["B"], d["mu"], s, n0, n)      # outputs pre-filled with NaN
    ref = DR.project64(x["G"], x["W0"], x["A"], x["B"], x["mu"], s)
    delta = DR.bounds(x["W0"], x["A"], x["B"], x["mu"], s, x["G"])
    res = {k: ratio(got[k], ref[k], delta[k]) for k in ("mu", "B", "A")}
    print(f"[dora] project {label} r{rank}: max |err| / delta " + " ".join(f"d{k} {res[k][0]:.4f}" for k in res))
    assert all(ok for _r, ok in res.values()), (label, rank, res)
    again = dev_project(case, d["G"], d["W0"], d["A"], d["B"], d["mu"], s, n0, n)
    assert all(same_bits(got[k], again[k]) for k in got)


# ------------------------------------------------------------------------------------------------ isolation, refusals
@pytest.mark.parametrize("label,rank", [("40x24", 3), ("130x264", 16), ("conv40x16", 3), ("geglu128g64x24", 16)])
def test_hooks_are_operand_isolated(label, rank):
    case = BY_LABEL[label]
    _label, kind, out, inn, group = case
    x = operands(case, rank, seed=2)
    W0n, Gn = DR.to_native(x["W0"], kind, group), DR.to_native(x["G"], kind, group)
    col = lambda t: t.reshape(-1, 1)
    base = [Spec("W0", out, inn, init=W0n)]
    adapters = [Spec("A", rank, inn, init=x["A"]), Spec("B", out, rank, init=x["B"]), Spec("mu", out, 1, init=col(x["mu"]))]

    def init(a):
        lib.check(load(one(case, 1, lib.DORA_INIT, 0.0, base=a.ptr("W0"), norm0=a.ptr("n0"))), "dora init")

    runs = run_isolated(init, base + [Spec("n0", out, 1, dtype=f32, role="out")], device=DEV)
    assert_isolated(runs, what=f"dora init {label}")
    n0 = runs[0]["n0"].cpu()
    # the cross-row form, where native rows are source rows (not GEGLU): poisoned rows past `keep` change nothing in the rows before
    keep = out // 2
    tail, head = slice(keep, None), slice(0, keep)

    def kept(runs, names):
        return [{k: r[k][head] for k in names} for r in runs]

    if kind != GEGLU:
        assert_isolated(kept(run_isolated(init, base + [Spec("n0", out, 1, dtype=f32, role="out")], device=DEV, poison={"W0": tail}), ["n0"]),
                        what=f"dora init {label}, poisoned neighbour rows")

    def merge(a):
        lib.check(load(one(case, rank, lib.DORA_MERGE, 0.37, base=a.ptr("W0"), A=a.ptr("A"), B=a.ptr("B"), mu=a.ptr("mu"), w=a.ptr("w"),
                           norm0=a.ptr("n0"), norm=a.ptr("n"))), "dora merge")

    specs = base + adapters + [Spec("n0", out, 1, dtype=f32, init=n0), Spec("n", out, 1, dtype=f32, role="out"), Spec("w", out, inn, role="out")]
    runs = run_isolated(merge, specs, device=DEV)
    assert_isolated(runs, what=f"dora merge {label}")
    n = runs[0]["n"].cpu()
    assert same_bits(src(case, runs[0]["w"]), DR.merge_given(x["W0"], x["A"], x["B"], x["mu"], 0.37, n0.reshape(-1), n.reshape(-1)))
    if kind != GEGLU:
        runs = run_isolated(merge, specs, device=DEV, poison={"W0": tail, "B": tail, "mu": tail, "n0": tail})
        assert_isolated(kept(runs, ["w", "n"]), what=f"dora merge {label}, poisoned neighbour rows")

    def project(a):
        lib.check(export(one(case, rank, 0, 0.37, dw=a.ptr("G"), base=a.ptr("W0"), A=a.ptr("A"), B=a.ptr("B"), mu=a.ptr("mu"), norm0=a.ptr("n0"),
                             norm=a.ptr("n"), dA=a.ptr("dA"), dB=a.ptr("dB"), dmu=a.ptr("dmu"))), "dora project")

    specs = [Spec("G", out, inn, dtype=f32, init=Gn)] + base + adapters + [Spec("n0", out, 1, dtype=f32, init=n0), Spec("n", out, 1, dtype=f32, init=n),
             Spec("dA", rank, inn, dtype=f32, role="out"), Spec("dB", out, rank, dtype=f32, role="out"), Spec("dmu", out, 1, dtype=f32, role="out")]
    runs = run_isolated(project, specs, device=DEV)
    assert_isolated(runs, what=f"dora project {label}")
    if kind != GEGLU:          # (dA sums over every row, the poisoned ones too: dmu and dB are what has rows to keep)
        runs = run_isolated(project, specs, device=DEV, poison={"G": tail, "W0": tail, "B": tail, "mu": tail, "n0": tail, "n": tail})
        assert_isolated(kept(runs, ["dmu", "dB"]), what=f"dora project {label}, poisoned neighbour rows")


def test_refusals_return_1_with_their_message_before_any_launch():
    L = lib.load()
    buf = torch.zeros(4096, dtype=torch.uint8, device=DEV)                  # aligned and never touched
    p, odd = buf.data_ptr(), buf.data_ptr() + 2
    every = dict(base=p, A=p, B=p, mu=p, w=p, dw=p, dA=p, dB=p, dmu=p, norm0=p, norm=p)
    ok = ("c", CONV3, 8, 72, 8)
    # (case, rank, mode, scale), the message
    cases = [((ok, 0, 0, 1.0), b"rank"), ((ok, 129, 0, 1.0), b"rank"), ((("c", CONV3, 8, 36, 4), 4, 0, 1.0), b"multiple of 8"),
             ((("p", PLAIN, 8, 12, 0), 4, 0, 1.0), b"multiple of 8"), ((("k", 3, 8, 72, 8), 4, 0, 1.0), b"kind"), ((("c", CONV3, 8, 72, 16), 4, 0, 1.0), b"9 cin"),
             ((("g", GEGLU, 128, 8, 48), 4, 0, 1.0), b"groups"), ((ok, 4, 0, float("nan")), b"finite"), ((("z", PLAIN, 0, 72, 0), 4, 0, 1.0), b"[0][72]")]
    for (case, rank, mode, scale), msg in cases:
        for fn in (load, export):
            assert fn(one(case, rank, mode, scale, **every)) == 1 and msg in L.sdxl_last_error(), (case, rank, L.sdxl_last_error())
    for mode in (-1, 3):
        assert load(one(ok, 4, mode, 1.0, **every)) == 1 and b"mode" in L.sdxl_last_error()
    used = {lib.DORA_MERGE: ("base", "A", "B", "mu", "w", "norm0", "norm"), lib.DORA_INIT: ("base", "norm0"), lib.DORA_RESTORE: ("base", "w")}
    for mode, names in used.items():
        for name in names:
            for bad in (odd, None):
                assert load(one(ok, 4, mode, 1.0, **dict(every, **{name: bad}))) == 1 and b"aligned" in L.sdxl_last_error(), (mode, name, bad)
    for name in ("dw", "base", "A", "B", "mu", "norm0", "norm", "dA", "dB", "dmu"):
        for bad in (odd, None):
            assert export(one(ok, 4, 0, 1.0, **dict(every, **{name: bad}))) == 1 and b"aligned" in L.sdxl_last_error(), (name, bad)
    o = one(ok, 4, 0, 1.0, **every)
    for fn in (L.sdxl_load_weight, L.sdxl_export_grad):
        assert fn(None, b"conv_in.weight", C.byref(o), lib.DTYPE_DORA_ONE, stream()) == 1 and b"no name" in L.sdxl_last_error()
        assert fn(None, None, None, lib.DTYPE_DORA_ONE, stream()) == 1 and b"NULL" in L.sdxl_last_error()
    torch.cuda.synchronize()
    assert int(buf.sum()) == 0


# ------------------------------------------------------------------------------------------------ the handle (tiny UNet)
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


def randomize(ad, std=0.02, mu_std=0.1, seed=5):
    g = torch.Generator().manual_seed(seed)
    for k in ad.targets:
        ad.B(k).copy_(bf(torch.randn(ad.B(k).shape, generator=g) * std))
        ad.mu(k).copy_(bf(torch.randn(ad.mu(k).shape, generator=g) * mu_std))


def case_of(k, shapes):
    o, i = flat2(shapes[k])
    kind, group = kind_of(k, shapes[k])
    return (k, kind, o, i, group)


def test_batched_calls_equal_the_hook_per_target_and_touch_nothing_else(tiny):
    cfg, w, net, w0 = tiny
    shapes = net.param_shapes()
    ad = LORA.LoRAAdapters(net, rank=8, alpha=2.0, targets=ALL_KINDS_TARGETS, kinds="all", algo="dora")
    assert {kind_of(k, shapes[k])[0] for k in ad.targets} == {PLAIN, CONV3, GEGLU} and ad.dtype == lib.DTYPE_DORA
    ranges, mask = net.param_ranges(), target_mask(net, ad)
    try:
        torch.cuda.synchronize()
        for k in ad.targets:                                               # init ran once, in the constructor: norm0 is the hook's
            off, n = ranges[k]
            o, i = flat2(shapes[k])
            assert same_bits(ad.row_norm(k), dev_init(case_of(k, shapes), w0[off: off + n].view(o, i))), k
            assert same_bits(ad.magnitude(k), ad.row_norm(k))             # mu = 0
        ad.merge()                                                         # B = 0, mu = 0
        torch.cuda.synchronize()
        assert same_bits(net.weights, w0)
        randomize(ad, std=0.5)
        ad.norm.fill_(float("nan"))
        pads = torch.ones_like(ad.norm, dtype=torch.bool)
        for k in ad.targets:
            pads[ad.norm_offsets[k]: ad.norm_offsets[k] + ad.layout[k][-2]] = False
        ad.merge()
        torch.cuda.synchronize()
        assert same_bits(net.weights[~mask], w0[~mask])                    # nothing outside the targets' native ranges
        assert bool(torch.isnan(ad.norm[pads]).all()) and bool(torch.isfinite(ad.norm[~pads]).all())      # the pads of `norm` are not written
        for k in ad.targets:
            off, n = ranges[k]
            o, i = flat2(shapes[k])
            hook_w, hook_n = dev_merge(case_of(k, shapes), w0[off: off + n].view(o, i), ad.A(k), ad.B(k), ad.mu(k), ad.scale, ad.row_norm(k))
            assert same_bits(net.weights[off: off + n].view(o, i), hook_w) and same_bits(ad.row_norm(k, base=False), hook_n), k
            assert not same_bits(hook_w, w0[off: off + n].view(o, i)), k
        merged = net.weights.clone()
        net.grads.copy_(torch.randn(net.param_elems, generator=torch.Generator().manual_seed(3)))
        g0 = net.grads.clone()
        ad.grads.fill_(float("nan"))
        ad.project()
        torch.cuda.synchronize()
        assert same_bits(net.grads, g0) and same_bits(net.weights, merged)
        written = torch.zeros(ad.param_elems, dtype=torch.bool, device=DEV)
        for k in ad.targets:
            off, n = ranges[k]
            o, i = flat2(shapes[k])
            hook = dev_project(case_of(k, shapes), g0[off: off + n].view(o, i), w0[off: off + n].view(o, i), ad.A(k), ad.B(k), ad.mu(k), ad.scale,
                               ad.row_norm(k), ad.row_norm(k, base=False))
            for name, got in (("A", ad.A(k, grad=True)), ("B", ad.B(k, grad=True)), ("mu", ad.mu(k, grad=True))):
                assert same_bits(got, hook[name]), (k, name)
            for slot, t in zip(ad.layout[k][:3], (ad.A(k), ad.B(k), ad.mu(k))):
                written[slot: slot + t.numel()] = True
        assert bool(torch.isnan(ad.grads[~written]).all()) and bool(torch.isfinite(ad.grads[written]).all())      # the pads are not written
        ad.restore()
        torch.cuda.synchronize()
        assert same_bits(net.weights, w0)
    finally:
        net.weights.copy_(w0)
        net.grads.zero_()
        torch.cuda.synchronize()


def test_argument_errors_and_the_table_keyed_by_the_dtype(tiny):
    cfg, w, net, w0 = tiny
    L = lib.load()
    names = list(net.param_shapes())
    idx = lambda k: names.index(k)
    big = torch.zeros(1 << 22, dtype=torch.bfloat16, device=DEV)
    gbig = torch.zeros(1 << 22, dtype=torch.float32, device=DEV)
    nbig = torch.zeros(1 << 16, dtype=torch.float32, device=DEV)

    def op(params, rank=4, mode=0, norm0=nbig.data_ptr(), norm=nbig.data_ptr()):
        arr = (C.c_int * len(params))(*params)
        return lib.DoraOp(lib.LoraOp(len(params), arr, rank, 1.0, big.data_ptr(), big.data_ptr(), gbig.data_ptr()), mode, norm0, norm), arr

    c1 = "down_blocks.0.resnets.0.conv1.weight"
    cases = [([idx(c1)], dict(rank=0), b"rank"), ([idx(c1)], dict(rank=129), b"rank"),
             ([idx("conv_in.weight")], {}, b"conv_in.weight"), ([idx(c1), idx("conv_in.weight")], {}, b"conv_in.weight"),
             ([idx("conv_out.bias")], {}, b"conv_out.bias"), ([idx("down_blocks.0.resnets.0.norm1.weight")], {}, b"norm1.weight"),
             ([idx(c1), idx(c1)], {}, b"twice"), ([len(names)], {}, b"out of range"), ([-1], {}, b"out of range"),
             ([idx(c1)], dict(norm0=None), b"norm0"), ([idx(c1)], dict(norm0=nbig.data_ptr() + 4), b"norm0"),
             ([idx(c1)], dict(norm=None), b"norm"), ([idx(c1)], dict(norm=nbig.data_ptr() + 4), b"norm")]
    for params, kw, msg in cases:
        o, _keep = op(params, **kw)
        for fn in (L.sdxl_load_weight, L.sdxl_export_grad):
            assert fn(net.h, None, C.byref(o), lib.DTYPE_DORA, stream()) == 1 and msg in L.sdxl_last_error(), (params, kw, L.sdxl_last_error())
    for mode in (-1, 3):
        o, _keep = op([idx(c1)], mode=mode)
        assert L.sdxl_load_weight(net.h, None, C.byref(o), lib.DTYPE_DORA, stream()) == 1 and b"mode" in L.sdxl_last_error()
    o, _keep = op([idx(c1)])
    assert L.sdxl_load_weight(net.h, b"conv_in.weight", C.byref(o), lib.DTYPE_DORA, stream()) == 1 and b"NULL" in L.sdxl_last_error()
    assert L.sdxl_export_grad(net.h, c1.encode(), C.byref(o), lib.DTYPE_DORA, stream()) == 1 and b"NULL" in L.sdxl_last_error()
    with pytest.raises(lib.SdxlError, match="conv1.weight"):            # the backward's own adapter gradients keep the plain rule
        net.set_trainable([], lora=o.op)
    torch.cuda.synchronize()
    assert same_bits(net.weights, w0) and float(big.abs().sum()) == 0.0 and float(gbig.abs().sum()) == 0.0 and float(nbig.abs().sum()) == 0.0
    # the same (target list, rank) under LoRA's, LoHa's and DoRA's dtypes, and back: each call has its own table and its own bits
    mk = lambda **kw: LORA.LoRAAdapters(net, rank=4, alpha=2.0, seed=2, kinds="all", **kw)
    lo, ha, do = mk(), mk(algo="loha"), mk(algo="dora")
    g = torch.Generator().manual_seed(1)
    for k in lo.targets:
        lo.B(k).copy_(bf(torch.randn(lo.B(k).shape, generator=g) * 0.5))
        ha.B2(k).copy_(bf(torch.randn(ha.B2(k).shape, generator=g) * 0.5))
    randomize(do, std=0.5)
    try:
        firsts = []
        for ad in (lo, ha, do):
            net.weights.copy_(w0)
            ad.merge()
            torch.cuda.synchronize()
            firsts.append(net.weights.clone())
            assert not same_bits(firsts[-1], w0) and not any(same_bits(firsts[-1], f) for f in firsts[:-1])
        for ad, first in list(zip((lo, ha, do), firsts))[::-1]:
            net.weights.copy_(w0)
            ad.merge()
            torch.cuda.synchronize()
            assert same_bits(net.weights, first)
    finally:
        net.weights.copy_(w0)
        torch.cuda.synchronize()


def dora64(W0, A, B, mu, s, n0):
    """the float64 DoRA weight with the norm detached, differentiable in A, B, mu"""
    V = W0 + s * (B @ A)
    n = V.detach().pow(2).sum(1).sqrt()
    return ((1.0 + mu) * n0 / n)[:, None] * V


@pytest.mark.parametrize("method", ["ddpm", "flow_matching"])
def test_adapter_gradients_match_the_oracle_at_the_merged_weights(tiny, method):
    """native dA / dB / dmu of every kind of target against autograd of the oracle's dW through the float64 DoRA formula with the norm
    detached, the oracle evaluated at the bf16-rounded MERGED weights; rank 8, the bar of tests/test_gpu_lora.py per tensor.  Then the
    same step under project_frozen (bit-equal), and two accumulated micro-steps against one projection of the summed dW."""
    cfg, w, net, w0 = tiny
    rank = 8
    shapes = net.param_shapes()
    ad = LORA.LoRAAdapters(net, rank=rank, alpha=rank / 2, targets=ALL_KINDS_TARGETS, seed=1, kinds="all", algo="dora")
    randomize(ad, std=0.02)
    x, kw = make_batch(cfg, 31), step_args(method, 32)
    try:
        ad.merge()
        native_micro(net, method, x, kw)
        ad.grads.fill_(float("nan"))
        ad.project()
        torch.cuda.synchronize()
        loss = net.read_loss()[0]
        got = ad.grads.clone()
        g1 = net.grads.clone()
        wm = {k: v.float().cpu() for k, v in net.state_dict().items()}           # bf16-rounded merged weights, as the step read them
        assert any(not torch.equal(wm[k], w[k]) for k in ad.targets)
        leaves = {k: wm[k].requires_grad_(True) for k in ad.targets}
        unet_fn = lambda s, t, e, p, ti: U.unet_forward(wm, s, t, e, p, ti, cfg)
        ob = {k: x[k] for k in ("vae_latents", "prompt_embeds", "pooled_prompt_embeds", "time_ids")}
        ref = R.compute_loss_ddpm(unet_fn, ob, kw["noise"], kw["timesteps"]) if method == "ddpm" else R.compute_loss_flow(unet_fn, ob, kw["noise"], kw["timesteps"])
        ref["loss"].backward()
        par = GradParity(f"dora {method} r{rank}")
        for k in ad.targets:
            o, i = flat2(shapes[k])
            A, B, mu = (t.double().cpu().requires_grad_(True) for t in (ad.A(k), ad.B(k), ad.mu(k)))
            W0 = bf(w[k]).double().reshape(o, i)                           # the arena's W0
            W = dora64(W0, A, B, mu, ad.scale, W0.pow(2).sum(1).sqrt())
            (W * leaves[k].grad.double().reshape(o, i)).sum().backward()
            mod = k[: -len(".weight")]
            par.add(f"{mod}.lora_A", ad.A(k, grad=True).cpu(), A.grad)
            par.add(f"{mod}.lora_B", ad.B(k, grad=True).cpu(), B.grad)
            par.add(f"{mod}.lora_magnitude", ad.mu(k, grad=True).cpu(), mu.grad)
        par.check(GRAD_BAR, expect=ad.param_ranges(), printer=lambda s: print("[parity] " + s))
        ad.select("project_frozen")
        native_micro(net, method, x, kw)
        ad.grads.fill_(float("nan"))
        ad.project()
        torch.cuda.synchronize()
        assert net.read_loss()[0] == loss and same_bits(ad.grads, got)
        net.set_trainable(None)
        # two accumulated micro-steps, then one projection: the projection of the summed dW (which the arena holds)
        x2, kw2 = make_batch(cfg, 33), step_args(method, 34)
        native_micro(net, method, x, kw)
        if method == "ddpm":
            sig = R.karras_sigmas()[kw2["timesteps"]]
            net.forward_loss("ddpm", x2["vae_latents"], kw2["noise"], sig, kw2["timesteps"].float(), x2["prompt_embeds"], x2["pooled_prompt_embeds"], x2["time_ids"])
        else:
            t = kw2["timesteps"]
            net.forward_loss("flow_matching", x2["vae_latents"], kw2["noise"], t, t, x2["prompt_embeds"], x2["pooled_prompt_embeds"], x2["time_ids"])
        net.backward(1.0, False)                                           # accumulate
        ad.project()
        torch.cuda.synchronize()
        acc = ad.grads.clone()
        summed = net.grads.clone()
        assert not same_bits(summed, g1) and not same_bits(acc, got)
        ranges, at = net.param_ranges(), 0
        for k in ad.targets:                                               # bit for bit the single-target projection of the summed dW
            o, i = flat2(shapes[k])
            off = ranges[k][0]
            hook = dev_project(case_of(k, shapes), summed[off: off + o * i].view(o, i), ad.base[at: at + o * i].view(o, i), ad.A(k), ad.B(k),
                               ad.mu(k), ad.scale, ad.row_norm(k), ad.row_norm(k, base=False))
            at += o * i
            for name, g in (("A", ad.A(k, grad=True)), ("B", ad.B(k, grad=True)), ("mu", ad.mu(k, grad=True))):
                assert same_bits(g, hook[name]), (k, name)
    finally:
        net.set_trainable(None)
        net.weights.copy_(w0)
        net.grads.zero_()
        torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ the trainer
TRAINER_TARGETS = ["ff.net.0.proj", "conv1", "conv_shortcut", "to_q"]
TRAINER_KEYS = dict(lora_rank=8, lora_algo="dora", lora_target_kinds="all", lora_targets=TRAINER_TARGETS)


@pytest.mark.parametrize("method", ["ddpm", "flow_matching"])
def test_the_first_step_has_the_plain_trainers_bits(tiny, method):
    cfg, w, net, w0 = tiny
    batch, kw = make_batch(cfg, 21), step_args(method, 22)
    try:
        plain = make_trainer(net, method)
        loss_p, _m = plain._execute_training_step(batch, **kw)
        torch.cuda.synchronize()
        g_p = net.grads.clone()
        del plain
        tr = make_trainer(net, method, **TRAINER_KEYS)
        assert isinstance(tr, LORA.NativeLoRATrainer) and tr.lora.algo == "dora"
        torch.cuda.synchronize()
        assert same_bits(net.weights, w0)                              # B = 0, mu = 0: the merge gave back W0
        loss_d, _m = tr._execute_training_step(batch, **kw)
        torch.cuda.synchronize()
        assert float(loss_d) == float(loss_p) and same_bits(net.grads, g_p) and float(g_p.abs().max()) > 0
    finally:
        net.weights.copy_(w0)
        net.grads.zero_()
        torch.cuda.synchronize()


@pytest.mark.parametrize("opt", ["adamw_bf16", "adamw_schedule_free_kahan", "prodigy"])
def test_a_few_steps_move_every_factor_and_lower_the_loss(tiny, opt):
    cfg, w, net, w0 = tiny
    try:
        from test_gpu_lora_layouts import CFG, T
        from types import SimpleNamespace
        c = CFG.Config()
        c.training.method = "ddpm"
        c.optimizer.learning_rate = 1.0 if opt == "prodigy" else 1e-3
        c.optimizer.optimizer_type = opt
        for k, v in TRAINER_KEYS.items():
            setattr(c.training, k, v)
        tr = T.create_trainer(SimpleNamespace(unet=net), config=c)
        batch = make_batch(cfg, 41)
        noise = torch.randn(batch["vae_latents"].shape, generator=torch.Generator().manual_seed(42))
        # timestep 800: the MinSNR weight there leaves a loss of about 0.09 and adapter gradients far above the optimizers' eps (at timestep
        # 500 the loss is about 4e-6 and Prodigy's estimate cannot leave d0: tests/test_gpu_prodigy.py)
        ts = torch.full((2,), 800, dtype=torch.long)
        losses = []
        for _ in range(20):
            loss, _m = tr._execute_training_step(batch, timesteps=ts, noise=noise)
            losses.append(float(loss))
            tr.optimizer_step()
        torch.cuda.synchronize()
        ad = tr.lora
        fresh = LORA.LoRAAdapters(net, rank=8, targets=TRAINER_TARGETS, kinds="all", algo="dora", seed=ad.seed)
        stored = {n: 0 for n in ("A", "B", "mu")}
        for k in ad.targets:                                               # every factor of every target has other bits than a fresh adapter's
            for n, now, was in (("A", ad.A(k), fresh.A(k)), ("B", ad.B(k), fresh.B(k)), ("mu", ad.mu(k), fresh.mu(k))):
                moved = not same_bits(now, was)
                stored[n] += moved
                assert moved, (opt, k, n)
        print(f"[dora] {opt}: loss {losses[0]:.6f} -> {losses[-1]:.6f} after 20 steps on one batch; stored bits moved in "
              + ", ".join(f"{n} {c}/{len(ad.targets)}" for n, c in stored.items()) + " targets")
        assert losses[-1] < losses[0]
    finally:
        net.set_trainable(None)
        net.weights.copy_(w0)
        net.grads.zero_()
        torch.cuda.synchronize()


def test_checkpoint_round_trip_reproduces_the_arena_and_the_merged_weights(tiny, tmp_path):
    from safetensors.torch import load_file
    cfg, w, net, w0 = tiny
    shapes = net.param_shapes()
    try:
        tr = make_trainer(net, "ddpm", lora_alpha=4.0, **TRAINER_KEYS)
        for s in range(3):
            tr._execute_training_step(make_batch(cfg, 100 + s), **step_args("ddpm", 200 + s))
            tr.optimizer_step()
        tr.save_checkpoint(tmp_path / "ck")
        torch.cuda.synchronize()
        want = (net.weights.clone(), tr.lora.weights.clone(), tr.lora.norm0.clone())
        assert not same_bits(want[0], w0)
        net.weights.copy_(w0)                                          # a fresh process would load the checkpoint's UNet
        tr2 = make_trainer(net, "ddpm", lora_alpha=4.0, **TRAINER_KEYS)
        tr2.lora.norm0.fill_(float("nan"))                             # recomputed on load
        tr2.load_lora_state(tmp_path / "ck")
        torch.cuda.synchronize()
        assert same_bits(net.weights, want[0]) and same_bits(tr2.lora.weights, want[1]) and same_bits(tr2.lora.norm0, want[2])
        st = torch.load(str(tmp_path / "ck" / "lora_state.pt"), weights_only=True)
        assert st["algo"] == "dora" and st["rank"] == 8
        ex = load_file(str(tmp_path / "ck" / "pytorch_lora_weights.safetensors"))
        for k in tr.lora.targets:
            mod = k[: -len(".weight")]
            m = ex[f"unet.{mod}.lora_magnitude_vector"]
            assert m.dtype == torch.float32 and tuple(m.shape) == (shapes[k][0],) and same_bits(m, tr2.lora.magnitude(k).cpu())
        other = make_trainer(net, "ddpm", lora_rank=8, lora_target_kinds="all", lora_targets=TRAINER_TARGETS)      # a LoRA trainer refuses the state
        before = other.lora.weights.clone()
        with pytest.raises(ValueError, match="lora_algo"):
            other.load_lora_state(tmp_path / "ck")
        assert same_bits(other.lora.weights, before)
    finally:
        net.set_trainable(None)
        net.weights.copy_(w0)
        net.grads.zero_()
        torch.cuda.synchronize()
