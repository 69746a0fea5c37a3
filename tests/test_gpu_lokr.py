"""LoKr adapters (SDXL_DTYPE_LOKR, training.lora_algo "kronecker") on a real MI355X: the kernels of csrc/lokr.hip through their single-target
hooks on native buffers (merge bit-equal to the restatement of tests/_lokr_ref.py on the source view, the projections within the bound
accumulated next to the float64 reference, a scratch whose contents do not matter, operand isolation), through sdxl_load_weight /
sdxl_export_grad on the tiny UNet's handle with every kind of target and both forms in one table, the oracle at the merged weights, and
the trainer."""
import ctypes as C
import importlib

import pytest
import torch

import sdxl_amd  # noqa: F401
from oracle import loss_ref as R
from oracle import unet_ref as U
from sdxl_amd import lib
from sdxl_amd import unet as NU

import _lokr_ref as KR
from _gradparity import GradParity
from _isolation import Spec, assert_isolated, run_isolated, same_bits
from test_gpu_lora_layouts import (ALL_KINDS_TARGETS, flat2, kind_of, make_batch, make_trainer, native_micro, step_args, target_mask,
                                   tiny_native_cfg)

pytestmark = pytest.mark.gpu
LORA = importlib.import_module("sdxl-training-improvements_amd.lora")

GRAD_BAR = (6e-2, 0.995)          # GRAD_BAR of tests/test_gpu_lora.py
DEV = "cuda"
PLAIN, CONV3, GEGLU = KR.PLAIN, KR.CONV3, KR.GEGLU
# (label, kind, out, in, cin | G, factor): the smallest shapes at which the index arithmetic can still go wrong
CASES = [("1x8", PLAIN, 1, 8, 0, -1), ("8x8", PLAIN, 8, 8, 0, 2), ("37x8", PLAIN, 37, 8, 0, -1), ("40x24", PLAIN, 40, 24, 0, -1),
         ("130x264", PLAIN, 130, 264, 0, -1), ("64x2048", PLAIN, 64, 2048, 0, 8), ("1280x1280", PLAIN, 1280, 1280, 0, 8),
         ("conv40x16", CONV3, 40, 9 * 16, 16, -1), ("conv8x320", CONV3, 8, 9 * 320, 320, 8),
         ("geglu128g64x24", GEGLU, 256, 24, 64, 8), ("geglu160g80x24", GEGLU, 320, 24, 80, -1)]
BY_LABEL = {c[0]: c for c in CASES}
# the full form, and the factored form at ranks 1, 3, 16 and, for the two large plain cases, 128 (rank 0 here: full)
FORMS = [(c, 0) for c in CASES] + [(c, r) for c in CASES for r in (1, 3, 16)] + [(BY_LABEL[n], 128) for n in ("64x2048", "1280x1280")]
FORM_IDS = [f"{c[0]}-{'full' if r == 0 else 'r%d' % r}" for c, r in FORMS]

bf = lambda t: t.to(torch.bfloat16)
ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())
stream = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _one(args, scratch, floats, **ptrs):
    """sdxl_lokr_one from (out, in, group, kind, factor, rank, full, scale) and the pointers (c_void_p, int or None)"""
    out, inn, group, kind, factor, rank, full, scale = args
    val = lambda p: p.value if isinstance(p, C.c_void_p) else p
    return lib.LokrOne(out=out, in_=inn, group=group, kind=kind, factor=factor, rank=rank, full=full, scale=scale, scratch=val(scratch),
                       scratch_floats=getattr(floats, "value", floats), **{k: val(v) for k, v in ptrs.items()})


def lokr_merge(L, base, Cm, W2, A, w, *rest):
    """the merge half of the hook SDXL_DTYPE_LOKR_ONE: rest = out, in, group, kind, factor, rank, full, scale, scratch, scratch_floats, stream"""
    o = _one(rest[:8], rest[8], rest[9], base=base, C=Cm, W2=W2, A=A, w=w)
    return L.sdxl_load_weight(None, None, C.byref(o), lib.DTYPE_LOKR_ONE, rest[10])


def lokr_project(L, dw, Cm, W2, A, dC, dW2, dA, *rest):
    o = _one(rest[:8], rest[8], rest[9], dw=dw, C=Cm, W2=W2, A=A, dC=dC, dW2=dW2, dA=dA)
    return L.sdxl_export_grad(None, None, C.byref(o), lib.DTYPE_LOKR_ONE, rest[10])


def geometry(kind, out, inn, group, factor):
    cin, khw = (group, 9) if kind == CONV3 else (inn, 1)
    return KR.geometry(out, cin, khw, factor)


def scratch_floats(geo, full):
    out_l, out_k, in_m, in_n, n2 = geo
    return LORA.lokr_scratch_floats([dict(out_l=out_l, out_k=out_k, in_m=in_m, in_n=in_n, n2=n2, full=int(full))])


def operands(case, rank, seed=0):
    """native W0 and dW, and the factors (indexed like the state-dict tensors), all N(0, 1); rank 0: the full form (A is None)"""
    _label, kind, out, inn, group, factor = case
    out_l, out_k, in_m, in_n, n2 = geometry(kind, out, inn, group, factor)
    g = torch.Generator().manual_seed(1000 * seed + 7 * out + inn + rank + 31 * kind)
    r = lambda *s: torch.randn(*s, generator=g)
    W0 = bf(r(out, inn))
    W0[0, 0] = W0[out - 1, inn - 1] = -0.0      # W0 + (+0) would lose the sign: only the kernel's `t == 0` branch gives these bits back
    x = dict(W0=W0.to(DEV), dW=r(out, inn).to(DEV), C=bf(r(out_l, in_m)).to(DEV))
    if rank == 0:
        x.update(W2=bf(r(out_k, n2)).to(DEV), A=None)
    else:
        x.update(W2=bf(r(out_k, rank)).to(DEV), A=bf(r(rank, n2)).to(DEV))
    return x


def fac(x):
    return x["C"], x["W2"], x["A"]


def hook_merge(case, W0, Cm, W2, A, s):
    _label, kind, out, inn, group, factor = case
    w = torch.full_like(W0, float("nan"))
    lib.check(lokr_merge(lib.load(), ptr(W0), ptr(Cm), ptr(W2), ptr(A), ptr(w), out, inn, group, kind, factor,
                                            1 if A is None else A.shape[0], int(A is None), s, None, 0, stream()), "lokr_merge")
    return w


def hook_project(case, dW, Cm, W2, A, s, scratch=None):
    _label, kind, out, inn, group, factor = case
    if scratch is None:
        scratch = torch.empty(scratch_floats(geometry(kind, out, inn, group, factor), A is None), dtype=torch.float32, device=dW.device)
    out_t = {n: torch.full(t.shape, float("nan"), dtype=torch.float32, device=dW.device) for n, t in zip(KR.names(A), (Cm, W2, A))}
    dA = out_t.get("A")
    lib.check(lokr_project(lib.load(), ptr(dW), ptr(Cm), ptr(W2), ptr(A), ptr(out_t["C"]), ptr(out_t[KR.names(A)[1]]), ptr(dA), out, inn,
                                              group, kind, factor, 1 if A is None else A.shape[0], int(A is None), s, ptr(scratch), scratch.numel(),
                                              stream()), "lokr_project")
    return out_t


# ------------------------------------------------------------------------------------------------ the hooks
def test_the_case_table_has_the_factorisations_it_was_chosen_for():
    want = {"1x8": (1, 1, 2, 4, 4), "8x8": (2, 4, 2, 4, 4), "37x8": (1, 37, 2, 4, 4), "40x24": (5, 8, 4, 6, 6), "130x264": (10, 13, 12, 22, 22),
            "64x2048": (8, 8, 8, 256, 256), "1280x1280": (8, 160, 8, 160, 160), "conv40x16": (5, 8, 4, 4, 36), "conv8x320": (1, 8, 8, 40, 360),
            "geglu128g64x24": (8, 32, 3, 8, 8), "geglu160g80x24": (16, 20, 4, 6, 6)}
    L = lib.load()
    p = ptr(torch.zeros(64, device=DEV))                  # aligned and never touched: every call below is refused before any launch
    pad4 = lambda n: (n + 3) // 4 * 4
    for label, kind, out, inn, group, factor in CASES:
        out_l, out_k, in_m, in_n, n2 = want[label]
        assert geometry(kind, out, inn, group, factor) == want[label], label
        shape = (out, group, 3, 3) if kind == CONV3 else (out, inn)
        g = LORA.lokr_geometry(shape, factor, 3, False)
        assert (g["out_l"], g["out_k"], g["in_m"], g["in_n"], g["n2"]) == want[label], label
        # the library's own factorisation, read from the scratch size the hook asks for (full: the partial sums; factored: and dW2)
        for full in (1, 0):
            need = pad4(-(-out_k * n2 // lib.LOKR_TILE) * out_l * in_m) + (0 if full else pad4(out_k * n2))
            assert lokr_project(L, p, p, p, p, p, p, p, out, inn, group, kind, factor, 3, full, 1.0, p, 0, stream()) == 1
            assert f"needs {need}".encode() in L.sdxl_last_error(), (label, full, L.sdxl_last_error())


@pytest.mark.parametrize("case,rank", FORMS, ids=FORM_IDS)
def test_merge_is_bit_equal_to_the_restatement_and_restores_w0(case, rank):
    label, kind, out, inn, group, factor = case
    x = operands(case, rank)
    src0 = KR.to_source(x["W0"], kind, group)
    for s in (0.37, 1.0):
        got = hook_merge(case, x["W0"], *fac(x), s)
        want = KR.to_native(KR.merge(src0, *fac(x), s), kind, group)
        assert same_bits(got, want), (label, rank, s)
        assert not same_bits(got, x["W0"])
    z = torch.zeros_like
    assert bool(torch.signbit(x["W0"][0, 0])) and bool(torch.signbit(x["W0"][-1, -1])) and float(x["W0"][0, 0]) == 0.0      # the planted -0s
    assert same_bits(hook_merge(case, x["W0"], *fac(x), 0.0), x["W0"])
    assert same_bits(hook_merge(case, x["W0"], z(x["C"]), x["W2"], x["A"], 0.37), x["W0"])
    assert same_bits(hook_merge(case, x["W0"], x["C"], z(x["W2"]), x["A"], 0.37), x["W0"])          # W2 = 0 (full), B = 0 (factored)
    if rank:
        assert same_bits(hook_merge(case, x["W0"], x["C"], x["W2"], z(x["A"]), 0.37), x["W0"])


@pytest.mark.parametrize("case,rank", FORMS, ids=FORM_IDS)
def test_project_is_within_the_accumulated_bound_overwrites_repeats_and_ignores_its_scratch(case, rank):
    label, kind, out, inn, group, factor = case
    x = operands(case, rank, seed=1)
    s = 0.37
    src = KR.to_source(x["dW"], kind, group)
    got = hook_project(case, x["dW"], *fac(x), s)                     # outputs pre-filled with NaN
    ref = KR.project64(src, *fac(x), s)
    bound = KR.project_bound(src, *fac(x), s)
    names = KR.names(x["A"])
    assert tuple(got) == tuple(ref) == tuple(bound) == names
    worst = {}
    for n in names:
        assert got[n].shape == ref[n].shape and bool(torch.isfinite(got[n]).all()), f"d{n}: not overwritten everywhere"
        err = (got[n].double() - ref[n]).abs()
        worst[n] = (float((err / bound[n].clamp_min(1e-300)).max()), float((err - bound[n]).max()))
        print(f"[lokr] project {label} {'full' if rank == 0 else 'r%d' % rank} d{n}: max |err| / delta {worst[n][0]:.4f}")
    for n in names:
        assert worst[n][1] <= 0.0, (n, label, rank, worst[n])
    again = hook_project(case, x["dW"], *fac(x), s)
    assert all(same_bits(got[n], again[n]) for n in names)
    need = scratch_floats(geometry(kind, out, inn, group, factor), rank == 0)
    for byte in (0xFF, 0x7F):                                          # fp32 NaN; 3.39e38
        scratch = torch.full((4 * need,), byte, dtype=torch.uint8, device=DEV).view(torch.float32)
        filled = hook_project(case, x["dW"], *fac(x), s, scratch=scratch)
        assert all(same_bits(got[n], filled[n]) for n in names), (label, rank, hex(byte))


@pytest.mark.parametrize("full", [True, False], ids=["full", "factored"])
@pytest.mark.parametrize("label,rank", [("40x24", 3), ("130x264", 16), ("conv40x16", 3), ("geglu128g64x24", 16)])
def test_hooks_are_operand_isolated(label, rank, full):
    case = BY_LABEL[label]
    _label, kind, out, inn, group, factor = case
    geo = geometry(kind, out, inn, group, factor)
    out_l, out_k, in_m, in_n, n2 = geo
    x = {k: (v.cpu() if v is not None else None) for k, v in operands(case, 0 if full else rank, seed=2).items()}
    L = lib.load()
    f32 = torch.float32
    need = scratch_floats(geo, full)
    r = 1 if full else rank
    a_ptr = lambda a, name: None if full else a.ptr(name)

    def merge(a):
        lib.check(lokr_merge(L, a.ptr("W0"), a.ptr("C"), a.ptr("W2"), a_ptr(a, "A"), a.ptr("w"), out, inn, group, kind, factor, r, int(full),
                                       0.37, None, 0, stream()), "lokr_merge")

    def project(a):
        lib.check(lokr_project(L, a.ptr("dW"), a.ptr("C"), a.ptr("W2"), a_ptr(a, "A"), a.ptr("dC"), a.ptr("dW2"), a_ptr(a, "dA"), out, inn,
                                         group, kind, factor, r, int(full), 0.37, a.ptr("scratch"), need, stream()), "lokr_project")

    factors = [Spec("C", out_l, in_m, init=x["C"]), Spec("W2", *x["W2"].shape, init=x["W2"])] + ([] if full else [Spec("A", rank, n2, init=x["A"])])
    runs = run_isolated(merge, [Spec("W0", out, inn, init=x["W0"])] + factors + [Spec("w", out, inn, role="out")], device=DEV)
    assert_isolated(runs, what=f"lokr_merge {label}")
    want = KR.to_native(KR.merge(KR.to_source(x["W0"], kind, group), x["C"], x["W2"], x["A"], 0.37), kind, group)
    assert same_bits(runs[0]["w"].cpu(), want)
    outs = [Spec("dC", out_l, in_m, dtype=f32, role="out"), Spec("dW2", *x["W2"].shape, dtype=f32, role="out")] \
        + ([] if full else [Spec("dA", rank, n2, dtype=f32, role="out")]) + [Spec("scratch", 1, need, dtype=f32, role="scratch")]
    runs = run_isolated(project, [Spec("dW", out, inn, dtype=f32, init=x["dW"])] + factors + outs, device=DEV)
    assert_isolated(runs, what=f"lokr_project {label}")


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


def zero_factor(ad, k, grad=False):
    return ad.W2(k, grad) if ad.geometry[k]["full"] else ad.A(k, grad)


def randomize_zero_factor(ad, std=0.02, seed=5):
    g = torch.Generator().manual_seed(seed)
    for k in ad.targets:
        v = zero_factor(ad, k)
        v.copy_(bf(torch.randn(v.shape, generator=g) * std))


def factors_of(ad, k, grad=False):
    """(C, W2 | B, A | None), the arguments of the reference and the hooks"""
    if ad.geometry[k]["full"]:
        return ad.C(k, grad), ad.W2(k, grad), None
    return ad.C(k, grad), ad.B(k, grad), ad.A(k, grad)


def case_of(ad, k, shapes):
    o, i = flat2(shapes[k])
    kind, group = kind_of(k, shapes[k])
    return (k, kind, o, i, group, ad.lokr_factor)


def test_batched_calls_with_mixed_forms_equal_the_hook_per_target_and_touch_nothing_else(tiny):
    cfg, w, net, w0 = tiny
    shapes = net.param_shapes()
    ad = LORA.LoRAAdapters(net, rank=8, alpha=2.0, targets=ALL_KINDS_TARGETS, kinds="all", algo="kronecker", factor=-1)
    assert {kind_of(k, shapes[k])[0] for k in ad.targets} == {PLAIN, CONV3, GEGLU} and "conv_out.weight" in ad.targets
    assert {ad.geometry[k]["full"] for k in ad.targets} == {0, 1}     # both forms in one table
    ranges, mask = net.param_ranges(), target_mask(net, ad)
    sd0 = {k: v.clone() for k, v in net.state_dict().items() if k in ad.targets}
    try:
        ad.merge()                                                     # the zero factor
        torch.cuda.synchronize()
        assert same_bits(net.weights, w0)
        randomize_zero_factor(ad, std=0.5)
        ad.merge()
        torch.cuda.synchronize()
        assert same_bits(net.weights[~mask], w0[~mask])                # nothing outside the targets' native ranges
        sd = net.state_dict()
        for k in ad.targets:
            o, i = flat2(shapes[k])
            off, n = ranges[k]
            assert n == o * i, k
            want = KR.merge(sd0[k].reshape(o, i).contiguous(), *factors_of(ad, k), ad.target_scale(k))
            assert same_bits(sd[k].reshape(o, i).contiguous(), want), k
            assert not same_bits(want, sd0[k].reshape(o, i).contiguous()), k          # took effect
            hook = hook_merge(case_of(ad, k, shapes), w0[off: off + n].view(o, i), *factors_of(ad, k), ad.target_scale(k))
            assert same_bits(net.weights[off: off + n].view(o, i), hook), k
        ad.restore()
        torch.cuda.synchronize()
        assert same_bits(net.weights, w0)
        # project: the arenas are read only; every target's gradients have the single-target hook's bits; the padding is not written
        net.grads.copy_(torch.randn(net.param_elems, generator=torch.Generator().manual_seed(3)))
        g0 = net.grads.clone()
        ad.grads.fill_(float("nan"))
        ad.scratch.fill_(float("nan"))
        ad.project()
        torch.cuda.synchronize()
        assert same_bits(net.grads, g0) and same_bits(net.weights, w0)
        written = torch.zeros(ad.param_elems, dtype=torch.bool, device=ad.grads.device)
        for k in ad.targets:
            off, n = ranges[k]
            o, i = flat2(shapes[k])
            f = factors_of(ad, k)
            hook = hook_project(case_of(ad, k, shapes), g0[off: off + n].view(o, i), *f, ad.target_scale(k))
            for name, got in zip(KR.names(f[2]), factors_of(ad, k, grad=True)):
                assert same_bits(got, hook[name]), (k, name)
            for slot, t in zip(ad.layout[k][:-2], f):
                written[slot: slot + t.numel()] = True
        assert bool(torch.isnan(ad.grads[~written]).all()) and bool(torch.isfinite(ad.grads[written]).all())
    finally:
        net.weights.copy_(w0)
        net.grads.zero_()
        torch.cuda.synchronize()


def test_argument_errors_and_the_table_keyed_by_dtype_factor_and_full(tiny):
    cfg, w, net, w0 = tiny
    L = lib.load()
    names = list(net.param_shapes())
    idx = lambda k: names.index(k)
    big = torch.zeros(1 << 22, dtype=torch.bfloat16, device=DEV)
    gbig = torch.zeros(1 << 22, dtype=torch.float32, device=DEV)
    sbig = torch.zeros(1 << 20, dtype=torch.float32, device=DEV)

    def op(params, rank=4, factor=-1, full=0, scratch=sbig.data_ptr(), floats=sbig.numel()):
        arr = (C.c_int * len(params))(*params)
        return lib.LokrOp(lib.LoraOp(len(params), arr, rank, 1.0, big.data_ptr(), big.data_ptr(), gbig.data_ptr()), factor, full, scratch, floats), arr

    c1 = "down_blocks.0.resnets.0.conv1.weight"
    cases = [([idx(c1)], dict(rank=0), b"rank"), ([idx(c1)], dict(rank=129), b"rank"), ([idx(c1)], dict(factor=0), b"factor"),
             ([idx(c1)], dict(factor=-2), b"factor"), ([idx(c1)], dict(full=2), b"full"), ([idx(c1)], dict(full=-1), b"full"),
             ([idx("conv_in.weight")], {}, b"conv_in.weight"), ([idx(c1), idx("conv_in.weight")], {}, b"conv_in.weight"),
             ([idx("conv_out.bias")], {}, b"conv_out.bias"), ([idx("down_blocks.0.resnets.0.norm1.weight")], {}, b"norm1.weight"),
             ([idx(c1), idx(c1)], {}, b"twice"), ([len(names)], {}, b"out of range"), ([-1], {}, b"out of range")]
    for params, kw, msg in cases:
        o, _keep = op(params, **kw)
        for fn in (L.sdxl_load_weight, L.sdxl_export_grad):
            assert fn(net.h, None, C.byref(o), lib.DTYPE_LOKR, stream()) == 1 and msg in L.sdxl_last_error(), (params, kw, L.sdxl_last_error())
    for kw in (dict(scratch=None), dict(scratch=sbig.data_ptr() + 4), dict(floats=7)):      # the projection's scratch; the merge needs none
        o, _keep = op([idx(c1)], **kw)
        assert L.sdxl_export_grad(net.h, None, C.byref(o), lib.DTYPE_LOKR, stream()) == 1 and b"scratch" in L.sdxl_last_error(), kw
    o, _keep = op([idx(c1)])
    assert L.sdxl_load_weight(net.h, b"conv_in.weight", C.byref(o), lib.DTYPE_LOKR, stream()) == 1 and b"NULL" in L.sdxl_last_error()
    assert L.sdxl_export_grad(net.h, c1.encode(), C.byref(o), lib.DTYPE_LOKR, stream()) == 1 and b"NULL" in L.sdxl_last_error()
    with pytest.raises(lib.SdxlError, match="conv1.weight"):            # the backward's own adapter gradients keep the plain rule
        net.set_trainable([], lora=o.op)
    torch.cuda.synchronize()
    assert same_bits(net.weights, w0) and float(big.abs().sum()) == 0.0 and float(gbig.abs().sum()) == 0.0 and float(sbig.abs().sum()) == 0.0
    # the same (target list, rank) under SDXL_DTYPE_LOHA and SDXL_DTYPE_LOKR with two factors and two forms, and back: each call has its own bits
    mk = lambda **kw: LORA.LoRAAdapters(net, rank=4, alpha=2.0, seed=2, kinds="all", **kw)
    ha = mk(algo="loha")
    variants = [mk(algo="kronecker", factor=-1), mk(algo="kronecker", factor=2), mk(algo="kronecker", factor=2, full=True)]
    assert all(v.targets == ha.targets for v in variants) and {v.dtype for v in variants} == {lib.DTYPE_LOKR}
    g = torch.Generator().manual_seed(1)
    for k in ha.targets:
        ha.B2(k).copy_(bf(torch.randn(ha.B2(k).shape, generator=g) * 0.5))
    for v in variants:
        randomize_zero_factor(v, std=0.5)
    try:
        firsts = []
        for ad in [ha] + variants:
            net.weights.copy_(w0)
            ad.merge()
            torch.cuda.synchronize()
            firsts.append(net.weights.clone())
            assert not same_bits(firsts[-1], w0) and not any(same_bits(firsts[-1], f) for f in firsts[:-1])
        for ad, first in list(zip([ha] + variants, firsts))[::-1]:
            net.weights.copy_(w0)
            ad.merge()
            torch.cuda.synchronize()
            assert same_bits(net.weights, first)
    finally:
        net.weights.copy_(w0)
        torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ end to end (tiny UNet, 16 x 16, B = 2)
TRAINER_TARGETS = ["ff.net.0.proj", "conv1", "conv_shortcut", "to_q"]
TRAINER_KEYS = dict(lora_rank=8, lora_algo="kronecker", lokr_factor=-1, lora_target_kinds="all", lora_targets=TRAINER_TARGETS)      # both forms


@pytest.mark.parametrize("method", ["ddpm", "flow_matching"])
def test_a_step_with_the_zero_factor_has_the_plain_trainers_bits(tiny, method):
    cfg, w, net, w0 = tiny
    batch, kw = make_batch(cfg, 21), step_args(method, 22)
    try:
        plain = make_trainer(net, method)
        loss_p, _m = plain._execute_training_step(batch, **kw)
        torch.cuda.synchronize()
        g_p = net.grads.clone()
        del plain
        tr = make_trainer(net, method, **TRAINER_KEYS)
        assert isinstance(tr, LORA.NativeLoRATrainer) and tr.lora.algo == "kronecker"
        assert {tr.lora.geometry[k]["full"] for k in tr.lora.targets} == {0, 1}
        torch.cuda.synchronize()
        assert same_bits(net.weights, w0)                              # W2 = 0 / A = 0: the merge gave back W0
        loss_k, _m = tr._execute_training_step(batch, **kw)
        torch.cuda.synchronize()
        assert float(loss_k) == float(loss_p) and same_bits(net.grads, g_p) and float(g_p.abs().max()) > 0
    finally:
        net.weights.copy_(w0)
        net.grads.zero_()
        torch.cuda.synchronize()


@pytest.mark.parametrize("method", ["ddpm", "flow_matching"])
def test_adapter_gradients_match_the_oracle_at_the_merged_weights(tiny, method):
    """native dC / dW2 / dB / dA of every kind of target and both forms against the float64 projection (autograd through kron, restated in
    _lokr_ref.project64 and checked against autograd on the host) of the oracle's dW reshaped [out, in], the oracle evaluated at the
    bf16-rounded MERGED weights; rank 8, zero-factor std 0.02, the bar of tests/test_gpu_lora.py per tensor.  Beside it (printed): the
    float64 projection of the EXPORTED native dW.  Then the same step under project_frozen: bit-equal."""
    cfg, w, net, w0 = tiny
    rank = 8
    shapes = net.param_shapes()
    ad = LORA.LoRAAdapters(net, rank=rank, alpha=rank / 2, targets=ALL_KINDS_TARGETS, seed=1, kinds="all", algo="kronecker", factor=-1)
    assert {ad.geometry[k]["full"] for k in ad.targets} == {0, 1}
    randomize_zero_factor(ad, std=0.02)
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
        par, inherited = GradParity(f"lokr {method} r{rank}"), GradParity(f"lokr {method} r{rank}: float64 projection of the exported dW")
        for k in ad.targets:
            o, i = flat2(shapes[k])
            f = [t.cpu() if t is not None else None for t in factors_of(ad, k)]
            want = KR.project64(leaves[k].grad.reshape(o, i), *f, ad.target_scale(k))
            inh = KR.project64(exported[k].reshape(o, i), *f, ad.target_scale(k))
            mod = k[: -len(".weight")]
            for name, g in zip(KR.names(f[2]), factors_of(ad, k, grad=True)):
                par.add(f"{mod}.{LORA.LOKR_NAMES[name]}", g.cpu(), want[name])
                inherited.add(f"{mod}.{LORA.LOKR_NAMES[name]}", inh[name], want[name])
        inherited.report(lambda _k: GRAD_BAR, printer=lambda s: print("[parity] " + s))
        par.check(GRAD_BAR, expect=ad.param_ranges(), printer=lambda s: print("[parity] " + s))
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


def twenty_steps(net):
    cfg = U.tiny_config()
    tr = make_trainer(net, "ddpm", **TRAINER_KEYS)
    batch = make_batch(cfg, 41)
    noise = torch.randn(batch["vae_latents"].shape, generator=torch.Generator().manual_seed(42))       # evaluate() draws the same
    ts = torch.full((2,), 500, dtype=torch.long)
    evaluate = lambda: tr.evaluate([batch], [500], generator=torch.Generator().manual_seed(42))[1]
    before = evaluate()
    losses = []
    for _ in range(20):
        loss, _m = tr._execute_training_step(batch, timesteps=ts, noise=noise)
        losses.append(float(loss))
        tr.optimizer_step()
    after = evaluate()
    torch.cuda.synchronize()
    return tr, before, after, losses


def test_twenty_steps_on_one_batch_lower_its_loss_and_repeat_bit_for_bit(tiny):
    cfg, w, net, w0 = tiny
    shapes = net.param_shapes()
    try:
        tr, before, after, losses = twenty_steps(net)
        print(f"[lokr] ddpm: evaluation loss {before:.6f} -> {after:.6f} after 20 steps")
        assert after < before
        ad = tr.lora
        mask, ranges = target_mask(net, ad), net.param_ranges()
        assert same_bits(net.weights[~mask], w0[~mask])                # only the targets moved ...
        assert all(not same_bits(net.weights[ranges[k][0]: ranges[k][0] + ranges[k][1]], w0[ranges[k][0]: ranges[k][0] + ranges[k][1]])
                   for k in ad.targets)                                # ... and every one of them did
        assert all(float(zero_factor(ad, k).float().abs().max()) > 0 for k in ad.targets)
        assert {kind_of(k, shapes[k])[0] for k in ad.targets} == {PLAIN, CONV3, GEGLU} and {ad.geometry[k]["full"] for k in ad.targets} == {0, 1}
        first = (net.weights.clone(), ad.weights.clone(), ad.grads.clone(), before, after, losses)
        net.weights.copy_(w0)
        tr2, before2, after2, losses2 = twenty_steps(net)
        assert same_bits(net.weights, first[0]) and same_bits(tr2.lora.weights, first[1]) and same_bits(tr2.lora.grads, first[2])
        assert (before2, after2, losses2) == first[3:]
    finally:
        net.set_trainable(None)
        net.weights.copy_(w0)
        net.grads.zero_()
        torch.cuda.synchronize()


def run_training(net, steps, accum=2, save_at=None, save_dir=None, resume_from=None, first_step=0):
    cfg = U.tiny_config()
    tr = make_trainer(net, "ddpm", lora_alpha=4.0, gradient_accumulation_steps=accum, **TRAINER_KEYS)
    if resume_from is not None:
        tr.load_lora_state(resume_from)
    for s in range(first_step, first_step + steps):
        for m in range(accum):
            tr._execute_training_step(make_batch(cfg, 100 + 10 * s + m), accumulate=True, is_last_accumulation_step=m == accum - 1,
                                      **step_args("ddpm", 200 + 10 * s + m))
        tr.optimizer_step()
        if save_at is not None and s == save_at:
            tr.save_checkpoint(save_dir)
    torch.cuda.synchronize()
    return tr


def test_checkpoint_round_trip_and_exported_delta(tiny, tmp_path):
    from safetensors.torch import load_file
    cfg, w, net, w0 = tiny
    shapes = net.param_shapes()
    try:
        tr = run_training(net, 3, save_at=1, save_dir=tmp_path / "ck")
        want = (net.weights.clone(), tr.lora.weights.clone(), tr.optimizer.exp_avg.clone(), tr.optimizer.exp_avg_sq.clone())
        net.weights.copy_(w0)                                      # a fresh process would load the checkpoint's UNet
        tr2 = run_training(net, 1, resume_from=tmp_path / "ck", first_step=2)
        for a, b in zip(want, (net.weights, tr2.lora.weights, tr2.optimizer.exp_avg, tr2.optimizer.exp_avg_sq)):
            assert same_bits(a, b)
        ex = load_file(str(tmp_path / "ck" / "lycoris_lokr.safetensors"))
        st = torch.load(str(tmp_path / "ck" / "lora_state.pt"), weights_only=True)
        assert st["rank"] == 8 and st["targets"] == tr.lora.targets and (st["algo"], st["factor"], st["full"]) == ("kronecker", -1, False)
        # the delta rebuilt from the file, as a LyCORIS loader forms it, against merged - base of the saved state: one bf16 rounding
        net.weights.copy_(w0)
        saved = LORA.LoRAAdapters(net, rank=8, alpha=4.0, targets=TRAINER_TARGETS, kinds="all", algo="kronecker", factor=-1)
        saved.load_state_dict(st)
        base = {k: v.clone() for k, v in net.state_dict().items() if k in saved.targets}
        saved.merge()
        torch.cuda.synchronize()
        merged = net.state_dict()
        for k in saved.targets:
            pre = "lora_unet_" + k[: -len(".weight")].replace(".", "_")
            g, shape = saved.geometry[k], shapes[k]
            w1 = ex[f"{pre}.lokr_w1"].double()
            w2 = ex[f"{pre}.lokr_w2"].double() if g["full"] else \
                (ex[f"{pre}.lokr_w2_a"].double() @ ex[f"{pre}.lokr_w2_b"].double()).reshape((g["out_k"], g["in_n"]) + tuple(shape[2:]))
            assert float(ex[f"{pre}.alpha"]) == (8.0 if g["full"] else 4.0), k
            rebuilt = (float(ex[f"{pre}.alpha"]) / 8) * torch.kron(w1[:, :, None, None] if len(shape) == 4 else w1, w2)
            assert tuple(rebuilt.shape) == tuple(shape) and float(rebuilt.abs().max()) > 0, k
            o, i = flat2(shape)
            assert torch.equal(rebuilt.reshape(o, i), KR.delta64(*[t.cpu() if t is not None else None for t in factors_of(saved, k)],
                                                                 saved.target_scale(k))), k
            want_w = base[k].double().cpu() + rebuilt
            err = float((merged[k].double().cpu() - want_w).abs().max())
            assert err <= 2.0 ** -8 * float(want_w.abs().max()), (k, err)
        other = make_trainer(net, "ddpm", lora_rank=8, lora_target_kinds="all", lora_targets=TRAINER_TARGETS)      # a LoRA trainer refuses the state
        before = other.lora.weights.clone()
        with pytest.raises(ValueError, match="lora_algo"):
            other.load_lora_state(tmp_path / "ck")
        assert same_bits(other.lora.weights, before)
    finally:
        net.weights.copy_(w0)
        net.grads.zero_()
        torch.cuda.synchronize()
