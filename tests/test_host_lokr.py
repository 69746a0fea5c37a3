"""LoKr adapters (training.lora_algo "kronecker", SDXL_DTYPE_LOKR), the parts that need no GPU: the factorisation table, the reference
arithmetic against torch.kron and float64 autograd, the restated merge's zero cases, three seeded index mistakes, the form rule, the C
boundary and the argument errors, the layout, the trainer's keys, the state's refusals and the LyCORIS-shaped export."""
import ctypes as C
import importlib
import re
import shutil
import subprocess
from pathlib import Path
from types import SimpleNamespace

import pytest
import torch

import sdxl_amd  # noqa: F401
from sdxl_amd import lib

import _lokr_ref as KR
from _isolation import same_bits
from test_host_lora import StandInNet

ROOT = Path(__file__).resolve().parent.parent
CFG = importlib.import_module("sdxl-training-improvements_amd.config")
T = importlib.import_module("sdxl-training-improvements_amd.trainer")
LORA = importlib.import_module("sdxl-training-improvements_amd.lora")

bf = lambda t: t.to(torch.bfloat16)
ONE_OF_EACH = {"plain": "mid_block.attentions.0.transformer_blocks.0.attn1.to_q.weight",
               "geglu": "mid_block.attentions.0.transformer_blocks.0.ff.net.0.proj.weight",
               "conv3": "mid_block.resnets.0.conv1.weight",
               "conv1": "up_blocks.0.resnets.0.conv_shortcut.weight"}
FACT_TABLE = [((8, -1), (2, 4)), ((16, 16), (1, 16)), ((37, -1), (1, 37)), ((37, 8), (1, 37)), ((130, 8), (5, 26)), ((130, -1), (10, 13)),
              ((250, 8), (5, 50)), ((264, -1), (12, 22)), ((320, 8), (8, 40)), ((320, -1), (16, 20)), ((1280, 8), (8, 160)),
              ((1280, -1), (32, 40)), ((2816, 8), (8, 352)), ((10240, 16), (16, 640)), ((8, 8), (1, 8))]
# (label, kind, out, cin, khw, factor, group): every case has out_l != out_k or in_m != in_n
CASES = [("plain", KR.PLAIN, 24, 40, 1, -1, 0), ("conv", KR.CONV3, 10, 8, 9, -1, 8), ("geglu", KR.GEGLU, 32, 24, 1, 2, 8)]
IDS = [c[0] for c in CASES]


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


@pytest.fixture(scope="module")
def net():
    return StandInNet()


def _trainer(net, **training):
    cfg = CFG.Config()
    for k, v in training.items():
        setattr(cfg.training, k, v)
    return T.create_trainer(SimpleNamespace(unet=net), config=cfg, device="cpu")


def factors(out, cin, khw, factor, r, seed, full):
    """(C, W2 | B, A | None) bf16 N(0, 1), in the shapes the code under test gives them (lora.lokr_geometry), which are the reference's"""
    out_l, out_k, in_m, in_n, n2 = KR.geometry(out, cin, khw, factor)
    g = LORA.lokr_geometry((out, cin) + ((3, 3) if khw == 9 else ()), factor, r, full)
    assert (g["out_l"], g["out_k"], g["in_m"], g["in_n"], g["n2"], g["khw"]) == (out_l, out_k, in_m, in_n, n2, khw)
    assert g["full"] == int(KR.rule_full(out_k, in_n, r, forced=full))
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: bf(torch.randn(*s, generator=g))
    return (rn(out_l, in_m), rn(out_k, n2), None) if full else (rn(out_l, in_m), rn(out_k, r), rn(r, n2))


# ------------------------------------------------------------------------------------------------ the factorisation
def test_factorisation_table():
    for (dim, factor), want in FACT_TABLE:
        assert KR.fact(dim, factor) == want, (dim, factor)
        assert LORA.lokr_fact(dim, factor) == want, (dim, factor)
    for dim in range(1, 200):
        for factor in (-1, 1, 2, 3, 8, 16):
            m, n = KR.fact(dim, factor)
            assert m <= n and m * n == dim and LORA.lokr_fact(dim, factor) == (m, n)


# ------------------------------------------------------------------------------------------------ the reference arithmetic
@pytest.mark.parametrize("full", [True, False], ids=["full", "factored"])
@pytest.mark.parametrize("label,kind,out,cin,khw,factor,group", CASES, ids=IDS)
def test_delta64_is_torch_kron_and_project64_its_float64_autograd(label, kind, out, cin, khw, factor, group, full):
    r, s = 3, 0.37
    out_l, out_k, in_m, in_n, n2 = KR.geometry(out, cin, khw, factor)
    assert (out_l != out_k or in_m != in_n) and out_l * out_k == out and in_m * in_n == cin
    Cm, W2, A = factors(out, cin, khw, factor, r, seed=out + cin, full=full)
    inn = cin * khw
    G = torch.randn(out, inn, generator=torch.Generator().manual_seed(5))
    leaves = [t.double().requires_grad_(True) for t in (Cm, W2) + (() if full else (A,))]
    w2 = leaves[1] if full else leaves[1] @ leaves[2]
    if khw == 9:      # the 4-D kron of the state-dict tensors, flattened
        delta = KR.f32(s) * torch.kron(leaves[0][:, :, None, None], w2.view(out_k, in_n, 3, 3)).reshape(out, inn)
    else:
        delta = KR.f32(s) * torch.kron(leaves[0], w2)
    got_delta = KR.delta64(Cm, W2, A, s)
    assert got_delta.shape == (out, inn) and torch.equal(got_delta, delta.detach()) and float(got_delta.abs().max()) > 0
    if kind == KR.GEGLU:      # ... and through the packed layout and back
        assert torch.equal(KR.to_source(KR.to_native(got_delta, kind, group), kind, group), delta.detach())
        assert not torch.equal(KR.to_native(got_delta, kind, group), got_delta)
    (G.double() * delta).sum().backward()
    got = KR.project64(G, Cm, W2, A, s)
    bound = KR.project_bound(G, Cm, W2, A, s)
    assert tuple(got) == tuple(bound) == KR.names(A)
    for name, leaf in zip(KR.names(A), leaves):
        ref = leaf.grad
        assert got[name].shape == ref.shape and float(ref.abs().max()) > 0
        assert float((got[name] - ref).abs().max()) <= 1e-12 * float(ref.abs().max()), name
        # the bound is positive wherever the gradient is not identically zero, and far below the gradient's own size
        assert bound[name].shape == ref.shape and float(bound[name].min()) > 0 and float(bound[name].max()) < 1e-3 * float(ref.abs().max())


@pytest.mark.parametrize("full", [True, False], ids=["full", "factored"])
@pytest.mark.parametrize("label,kind,out,cin,khw,factor,group", CASES, ids=IDS)
def test_merge_restatement_returns_w0_in_each_zero_case_and_is_the_delta_otherwise(label, kind, out, cin, khw, factor, group, full):
    Cm, W2, A = factors(out, cin, khw, factor, 3, seed=1, full=full)
    W0 = bf(torch.randn(out, cin * khw, generator=torch.Generator().manual_seed(2)))
    W0[0, 0] = -0.0
    z = torch.zeros_like
    assert same_bits(KR.merge(W0, Cm, W2, A, 0.0), W0)
    assert same_bits(KR.merge(W0, z(Cm), W2, A, 0.37), W0)
    assert same_bits(KR.merge(W0, Cm, z(W2), A, 0.37), W0)            # W2 = 0 (full), B = 0 (factored)
    if not full:
        assert same_bits(KR.merge(W0, Cm, W2, z(A), 0.37), W0)
    w = KR.merge(W0, Cm, W2, A, 0.37)
    assert not same_bits(w, W0)
    want = W0.double() + KR.delta64(Cm, W2, A, 0.37)
    assert float((w.double() - want).abs().max()) <= 2.0 ** -8 * float(want.abs().max())      # one bf16 rounding (2^-9 relative) and fp32 noise


@pytest.mark.parametrize("label,kind,out,cin,khw,factor,group", CASES, ids=IDS)
def test_three_seeded_mistakes_fail_the_comparison(label, kind, out, cin, khw, factor, group):
    s = 0.37
    out_l, out_k, in_m, in_n, n2 = KR.geometry(out, cin, khw, factor)
    Cm, W2, _A = factors(out, cin, khw, factor, 3, seed=3, full=True)
    inn = cin * khw
    right = KR.delta64(Cm, W2, None, s)
    tol = 2.0 ** -8 * float(right.abs().max())
    differs = lambda wrong: wrong.shape != right.shape or float((wrong - right).abs().max()) > tol
    # kron(W2, C) in place of kron(C, W2)
    assert differs(KR.f32(s) * torch.kron(W2.double(), Cm.double()))
    # j = tap in_n + d in place of d 9 + tap (a convolution only: the two agree where khw == 1)
    swapped = W2.double().view(out_k, in_n, khw).permute(0, 2, 1).reshape(out_k, n2)
    assert differs(KR.f32(s) * torch.kron(Cm.double(), swapped)) == (khw == 9)
    # factorising in = cin khw in place of cin (a convolution only)
    bad_m, bad_n = KR.fact(inn, factor)
    assert ((bad_m, bad_n) != (in_m, n2)) == (khw == 9)
    if khw == 9:
        g = torch.Generator().manual_seed(4)
        Cb, Wb = bf(torch.randn(out_l, bad_m, generator=g)), bf(torch.randn(out_k, bad_n, generator=g))
        assert Cb.shape != Cm.shape and differs(KR.f32(s) * torch.kron(Cb.double(), Wb.double()))
    # ... and the projections notice the first mistake too
    G = torch.randn(out, inn, generator=torch.Generator().manual_seed(6))
    ok = KR.project64(G, Cm, W2, None, s)
    leaves = [Cm.double().requires_grad_(True), W2.double().requires_grad_(True)]
    (G.double() * (KR.f32(s) * torch.kron(leaves[1], leaves[0]))).sum().backward()
    assert float((leaves[0].grad - ok["C"]).abs().max()) > 1e-3 * float(ok["C"].abs().max())


def test_form_rule_and_scale_per_target_on_a_mixed_list(net):
    r, alpha = 8, 2.0      # factor -1: to_q and conv1 are (16, 16) x (16, 16), full at rank 8; ff.net.0.proj and conv_shortcut are factored
    mods = [k[: -len(".weight")] for k in ONE_OF_EACH.values()]
    ad = LORA.LoRAAdapters(net, rank=r, alpha=alpha, targets=mods, kinds="all", algo="kronecker", factor=-1)
    forms = set()
    for k in ad.targets:
        shape = net.shapes[k]
        khw = 9 if len(shape) == 4 and shape[2] == 3 else 1
        out_l, out_k, in_m, in_n, n2 = KR.geometry(shape[0], shape[1], khw, -1)
        g = ad.geometry[k]
        assert (g["out_l"], g["out_k"], g["in_m"], g["in_n"], g["n2"], g["khw"]) == (out_l, out_k, in_m, in_n, n2, khw), k
        full = KR.rule_full(out_k, in_n, r)
        assert bool(g["full"]) == full == (2 * r >= max(out_k, in_n)), k
        assert ad.target_scale(k) == KR.target_scale(full, alpha, r) == (1.0 if full else 0.25), k
        assert ad.lokr_factors(k) == (("C", "W2") if full else ("C", "B", "A"))
        forms.add(full)
    assert forms == {True, False}                       # the list is mixed
    forced = LORA.LoRAAdapters(net, rank=r, alpha=alpha, targets=mods, kinds="all", algo="kronecker", factor=-1, full=True)
    assert all(forced.geometry[k]["full"] == 1 and forced.target_scale(k) == 1.0 for k in forced.targets)
    assert KR.rule_full(160, 160, 16) is False and KR.rule_full(40, 40, 20) is True and KR.rule_full(160, 160, 16, forced=True) is True


# ------------------------------------------------------------------------------------------------ the C boundary
def test_boundary_has_the_dtypes_the_hook_and_no_new_function():
    names = lambda text: set(re.findall(r"\b(sdxl_[a-z0-9_]+)\s*\(", text))
    text = (ROOT / "include" / "sdxlstep.h").read_text()
    declared = names(text)
    assert len(declared) <= 58 and not any("lokr" in n for n in declared)
    assert "#define SDXL_DTYPE_LOKR 6" in text and lib.DTYPE_LOKR == 6
    # the single-target hook is in part 1 of the diagnostics header, as a dtype and a struct: no function, no exported symbol of its own
    diag = (ROOT / "include" / "sdxlstep_diag.h").read_text()
    part1 = diag[diag.index("---- part 1"): diag.index("---- part 2")]
    assert "#define SDXL_DTYPE_LOKR_ONE 7" in part1 and "} sdxl_lokr_one;" in part1 and lib.DTYPE_LOKR_ONE == 7
    assert not any("lokr" in n for n in names(diag)) and not any("lokr" in n for n in lib.TEST_HOOK_SIGNATURES)
    L = lib.load()
    assert not hasattr(L, "sdxl_op_lokr_merge")
    op = lib.LokrOp()
    assert L.sdxl_load_weight(None, None, C.byref(op), lib.DTYPE_LOKR, None) == 1
    assert L.sdxl_export_grad(None, None, C.byref(op), lib.DTYPE_LOKR, None) == 1
    one = lib.LokrOne()
    for fn in (L.sdxl_load_weight, L.sdxl_export_grad):
        assert fn(None, None, None, lib.DTYPE_LOKR_ONE, None) == 1 and b"NULL" in L.sdxl_last_error()
        assert fn(None, b"conv_in.weight", C.byref(one), lib.DTYPE_LOKR_ONE, None) == 1 and b"no name" in L.sdxl_last_error()
        assert fn(None, None, C.byref(one), lib.DTYPE_LOKR_ONE, None) == 1 and b"aligned" in L.sdxl_last_error()


def test_struct_layout_matches_the_header(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang") or "/opt/rocm/lib/llvm/bin/clang"
    fields = ("op", "factor", "full", "scratch", "scratch_floats")
    one_py = [f[0] for f in lib.LokrOne._fields_]
    one_c = ["in" if f == "in_" else f for f in one_py]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "sdxlstep_diag.h"\n'
                   'int main(void) { printf("%zu %zu %d %d", sizeof(sdxl_lora_op), sizeof(sdxl_lokr_op), SDXL_DTYPE_LOKR, SDXL_LOKR_TILE);\n'
                   + "".join(f'  printf(" %zu", offsetof(sdxl_lokr_op, {f}));\n' for f in fields)
                   + "".join(f'  printf(" %zu", offsetof(sdxl_lokr_one, {f}));\n' for f in one_c)
                   + '  printf(" %zu %zu %zu\\n", sizeof(sdxl_lokr_one), (size_t)SDXL_LOKR_PAD(5), (size_t)SDXL_LOKR_PAD(8)); return 0; }\n')
    exe = tmp_path / "layout"
    r = subprocess.run([cc, "-I", str(ROOT / "include"), str(src), "-o", str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    out = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True, timeout=60).stdout.split()]
    K = lib.LokrOp
    assert out == [C.sizeof(lib.LoraOp), C.sizeof(K), lib.DTYPE_LOKR, lib.LOKR_TILE] + [getattr(K, f).offset for f in fields] \
        + [getattr(lib.LokrOne, f).offset for f in one_py] + [C.sizeof(lib.LokrOne), 8, 8]
    assert C.sizeof(lib.LoraOp) == 48 and K.op.offset == 0 and K.factor.offset == C.sizeof(lib.LoraOp)      # sdxl_lora_op is what it was


def test_hook_argument_errors_are_reported_before_any_launch():
    L = lib.load()
    buf = (C.c_char * 4096)()
    p = C.c_void_p((C.addressof(buf) + 15) & ~15)
    odd = C.c_void_p(p.value + 2)
    big = C.c_size_t(1 << 20)
    # (out, in, group, kind, factor, rank, full, scale)
    cases = [((8, 72, 8, 1, -1, 0, 0, 1.0), b"rank"), ((8, 72, 8, 1, -1, 129, 0, 1.0), b"rank"), ((8, 72, 8, 1, 0, 4, 0, 1.0), b"factor"),
             ((8, 72, 8, 1, -2, 4, 0, 1.0), b"factor"), ((8, 72, 8, 1, -1, 4, 2, 1.0), b"full"), ((8, 72, 8, 1, -1, 4, -1, 1.0), b"full"),
             ((8, 36, 4, 1, -1, 4, 0, 1.0), b"multiple of 8"), ((8, 12, 0, 0, -1, 4, 0, 1.0), b"multiple of 8"), ((8, 72, 8, 3, -1, 4, 0, 1.0), b"kind"),
             ((8, 72, 16, 1, -1, 4, 0, 1.0), b"9 cin"), ((128, 8, 48, 2, -1, 4, 0, 1.0), b"groups"),
             ((8, 72, 8, 1, -1, 4, 0, float("nan")), b"finite"), ((65536, 65536, 0, 0, 1, 4, 1, 1.0), b"too large"), ((0, 72, 0, 0, -1, 4, 0, 1.0), b"[0][72]")]
    for args, msg in cases:
        assert lokr_merge(L, p, p, p, p, p, *args, p, big, None) == 1 and msg in L.sdxl_last_error(), (args, L.sdxl_last_error())
        assert lokr_project(L, p, p, p, p, p, p, p, *args, p, big, None) == 1 and msg in L.sdxl_last_error(), (args, L.sdxl_last_error())
    ok = (8, 72, 8, 1, -1, 4, 0, 1.0)                     # (2, 4) x (2, 4), n2 = 36: 1 tile x 4 blocks, and 4 x 36 of dW2
    need = 4 + 4 * 36
    for at in range(5):
        ptrs = [p] * 5
        ptrs[at] = odd
        assert lokr_merge(L, *ptrs, *ok, p, big, None) == 1 and b"aligned" in L.sdxl_last_error(), at
        ptrs[at] = None
        assert lokr_merge(L, *ptrs, *ok, p, big, None) == 1, at
    for at in range(7):
        ptrs = [p] * 7
        ptrs[at] = odd
        assert lokr_project(L, *ptrs, *ok, p, big, None) == 1 and b"aligned" in L.sdxl_last_error(), at
        ptrs[at] = None
        assert lokr_project(L, *ptrs, *ok, p, big, None) == 1, at
    # the scratch: NULL, misaligned, too small by one float (factored and full), all naming it
    seven = [p] * 7
    assert lokr_project(L, *seven, *ok, None, big, None) == 1 and b"scratch" in L.sdxl_last_error()
    assert lokr_project(L, *seven, *ok, odd, big, None) == 1 and b"scratch" in L.sdxl_last_error()
    assert lokr_project(L, *seven, *ok, p, C.c_size_t(need - 1), None) == 1 and b"scratch" in L.sdxl_last_error()
    assert str(need).encode() in L.sdxl_last_error()
    full = (8, 72, 8, 1, -1, 4, 1, 1.0)
    assert lokr_project(L, *seven, *full, p, C.c_size_t(3), None) == 1 and b"scratch" in L.sdxl_last_error()
    assert lokr_project(L, *seven, *ok, p, C.c_size_t(0), None) == 1 and b"scratch" in L.sdxl_last_error()
    # the Python formula is the header's
    geo = dict(out_l=2, out_k=4, in_m=2, in_n=4, khw=9, n2=36, full=0)
    assert LORA.lokr_scratch_floats([geo]) == need and LORA.lokr_scratch_floats([dict(geo, full=1)]) == 4
    big_geo = dict(out_l=8, out_k=160, in_m=8, in_n=160, khw=1, n2=160, full=0)
    assert LORA.lokr_scratch_floats([big_geo, geo]) == 25 * 64 + 160 * 160 + need


# ------------------------------------------------------------------------------------------------ layout, ranges, initialisation
def test_layout_ranges_views_and_initialisation_of_one_target_of_each_kind(net):
    r = 8                  # (a mixed list: see the form rule's test)
    mods = [k[: -len(".weight")] for k in ONE_OF_EACH.values()]
    ad = LORA.LoRAAdapters(net, rank=r, alpha=2.0, targets=mods, seed=3, kinds="all", algo="kronecker", factor=-1)
    assert ad.algo == "kronecker" and ad.dtype == lib.DTYPE_LOKR == 6 and set(ad.targets) == set(ONE_OF_EACH.values())
    ranges = ad.param_ranges()
    cur, base, nranges = 0, 0, 0
    pad8 = lambda n: (n + 7) // 8 * 8
    for k in ad.targets:
        shape = net.shapes[k]
        khw = 9 if len(shape) == 4 and shape[2] == 3 else 1
        out_l, out_k, in_m, in_n, n2 = KR.geometry(shape[0], shape[1], khw, -1)
        full = KR.rule_full(out_k, in_n, r)
        mod = k[: -len(".weight")]
        want = [("C", "lokr_w1", out_l, in_m)] + ([("W2", "lokr_w2", out_k, n2)] if full else [("B", "lokr_w2_a", out_k, r), ("A", "lokr_w2_b", r, n2)])
        assert ad.layout[k][-2:] == (shape[0], shape[1] * khw) and len(ad.layout[k]) == len(want) + 2
        for slot, (name, lyco, rows, cols) in enumerate(want):
            assert ad.layout[k][slot] == cur and ranges[f"{mod}.{lyco}"] == (cur, pad8(rows * cols)), (k, name)
            v, gv = ad.factor_view(name, k), ad.factor_view(name, k, grad=True)
            assert v.shape == gv.shape == (rows, cols) and v.dtype == torch.bfloat16 and gv.dtype == torch.float32
            assert v.data_ptr() == ad.weights.data_ptr() + 2 * cur and gv.data_ptr() == ad.grads.data_ptr() + 4 * cur
            cur += pad8(rows * cols)
            nranges += 1
        off, n = net.ranges[k]
        assert torch.equal(ad.base[base: base + n], net.weights[off: off + n])
        base += n
        # the zero factor is W2 (full) or A (factored): the delta is zero; C and B are drawn
        zero = ad.W2(k) if full else ad.A(k)
        assert float(zero.abs().max()) == 0.0 and 0.6 < float(ad.C(k).float().std()) < 1.4
        f = (ad.C(k), ad.W2(k), None) if full else (ad.C(k), ad.B(k), ad.A(k))
        assert float(KR.delta64(*f, ad.target_scale(k)).abs().max()) == 0.0
        ones = bf(torch.ones(shape[0], shape[1] * khw))
        assert same_bits(KR.merge(ones, *f, ad.target_scale(k)), ones)
        if not full:
            assert 0.06 < float(ad.B(k).float().std()) < 0.14
        for wrong in (("A", "B") if full else ("W2",)):
            with pytest.raises(ValueError, match="kronecker"):
                getattr(ad, wrong)(k)
        with pytest.raises(ValueError, match="lora_algo"):
            ad.A1(k)
    assert cur == ad.param_elems == ad.weights.numel() == ad.grads.numel() and base == ad.base.numel() and nranges == len(ranges)
    assert ad.scratch.dtype == torch.float32 and ad.scratch.numel() >= LORA.lokr_scratch_floats(ad.geometry.values()) > 0
    again = LORA.LoRAAdapters(net, rank=r, alpha=2.0, targets=mods, seed=3, kinds="all", algo="kronecker")
    other = LORA.LoRAAdapters(net, rank=r, alpha=2.0, targets=mods, seed=4, kinds="all", algo="kronecker")
    assert same_bits(again.weights, ad.weights) and not same_bits(other.weights, ad.weights)
    # LoRA's and LoHa's layouts and views are what they were
    lo = LORA.LoRAAdapters(net, rank=r, alpha=2.0, targets=mods, seed=3, kinds="all")
    ha = LORA.LoRAAdapters(net, rank=r, alpha=2.0, targets=mods, seed=3, kinds="all", algo="loha")
    assert all(len(v) == 4 for v in lo.layout.values()) and all(len(v) == 6 for v in ha.layout.values()) and lo.scratch is None
    for fn in (lo.C, lo.W2, ha.C, ha.W2):
        with pytest.raises(ValueError, match="lora_algo"):
            fn(lo.targets[0])
    assert ha.factor("A1", ha.targets[0]).shape[0] == r               # LoHa's accessor is not shadowed
    for bad_rank in (0, 129, True, 4.0):
        with pytest.raises(ValueError, match="lora_rank"):
            LORA.LoRAAdapters(net, rank=bad_rank, algo="kronecker")
    assert LORA.LoRAAdapters(net, rank=128, targets=["attn1.to_q"], algo="kronecker").rank == 128
    for bad in (0, -2, 2.0, True, None, "8"):
        with pytest.raises(ValueError, match="lokr_factor"):
            LORA.LoRAAdapters(net, rank=4, algo="kronecker", factor=bad)
    for bad in (0, 1, None, "true"):
        with pytest.raises(ValueError, match="lokr_full"):
            LORA.LoRAAdapters(net, rank=4, algo="kronecker", full=bad)


# ------------------------------------------------------------------------------------------------ the trainer
def test_trainer_keys_bad_values_and_direct_mode(net):
    t = CFG.Config().training
    assert (t.lora_algo, t.lokr_factor, t.lokr_full) == ("lora", -1, False)
    tr = _trainer(net, lora_rank=4, lora_algo="kronecker", lokr_factor=2, lora_target_kinds="all",
                  lora_targets=["ff.net.0.proj", "conv1", "conv_shortcut", "to_q"])
    ad = tr.lora
    assert ad.algo == "kronecker" and ad.dtype == lib.DTYPE_LOKR and ad.kinds == "all" and ad.lokr_factor == 2 and ad.lokr_full is False
    assert {len(net.shapes[k]) for k in ad.targets} == {2, 4} and tr.optimizer is not None
    assert all(n.rsplit(".", 1)[1] in ("lokr_w1", "lokr_w2", "lokr_w2_a", "lokr_w2_b") for n in ad.param_ranges())
    assert all(ad.geometry[k]["out_l"] == 2 for k in ad.targets)
    fl = _trainer(net, lora_rank=4, lora_algo="kronecker", lokr_full=True, lora_targets=["to_q"]).lora
    assert fl.lokr_full is True and all(fl.lokr_factors(k) == ("C", "W2") for k in fl.targets)
    plain = _trainer(net, lora_rank=4, lora_algo="kronecker")           # the default kinds: the default targets
    assert plain.lora.kinds == "plain" and plain.lora.targets == _trainer(net, lora_rank=4).lora.targets
    with pytest.raises(ValueError, match="2-D"):                         # lora_target_kinds still decides what the patterns may resolve to
        _trainer(net, lora_rank=4, lora_algo="kronecker", lora_targets=["conv1"])
    for bad in (0, -2, 1.5, True, "8"):
        with pytest.raises(ValueError, match="lokr_factor"):
            _trainer(net, lora_rank=4, lora_algo="kronecker", lokr_factor=bad)
    for bad in (1, 0, "yes", None):
        with pytest.raises(ValueError, match="lokr_full"):
            _trainer(net, lora_rank=4, lora_algo="kronecker", lokr_full=bad)
    for kinds in ("plain", "all"):
        with pytest.raises(ValueError, match=r"direct.*lora_algo"):
            _trainer(net, lora_rank=4, lora_algo="kronecker", lora_target_kinds=kinds, lora_backward="direct")
    with pytest.raises(ValueError, match="lora_algo"):
        ad.select("direct")

    class Selecting(StandInNet):
        def set_trainable(self, names, lora=None):
            self.selected = (list(names), lora)

    sel = Selecting()
    fz = _trainer(sel, lora_rank=4, lora_algo="kronecker", lora_backward="project_frozen", lora_targets=["attn1.to_q"])
    assert fz.lora_backward == "project_frozen" and sel.selected[1] is None
    assert sel.selected[0] == LORA.trainable_for("project_frozen", fz.lora.targets, sel.shapes)
    with pytest.raises(ValueError, match=r"lora_rank.*128"):
        _trainer(net, lora_rank=129, lora_algo="kronecker")
    assert _trainer(net, lora_rank=128, lora_algo="kronecker", lora_targets=["attn1.to_q"]).lora.rank == 128      # LoHa's cap of 64 is its own
    for kw, msg in ((dict(use_ema=True), "use_ema"), (dict(shard_optimizer=True), "shard_optimizer")):
        with pytest.raises(ValueError, match=msg):
            _trainer(net, lora_rank=4, lora_algo="kronecker", **kw)
    OPT = importlib.import_module("sdxl-training-improvements_amd.optimizer")
    for opt in ("adamw_bf16", "adamw_schedule_free_kahan", "prodigy"):      # all three fused optimizers take the adapter arena
        cfg = CFG.Config()
        cfg.training.lora_rank, cfg.training.lora_algo, cfg.optimizer.optimizer_type = 4, "kronecker", opt
        one = T.create_trainer(SimpleNamespace(unet=net), config=cfg, device="cpu")
        assert one.lora.algo == "kronecker" and type(one.optimizer) is OPT.BY_TYPE[opt]


# ------------------------------------------------------------------------------------------------ state and export
def test_state_round_trip_and_refusal_of_another_algorithm_factor_or_form(net, tmp_path):
    mods = ["attn1.to_q", "conv1"]
    mk = lambda **kw: LORA.LoRAAdapters(net, rank=4, alpha=2.0, targets=mods, kinds="all", **kw)
    ad = mk(seed=1, algo="kronecker", factor=2)
    sd = ad.state_dict()
    assert sd["algo"] == "kronecker" and sd["factor"] == 2 and sd["full"] is False and sd["kinds"] == "all"
    other = mk(seed=9, algo="kronecker", factor=2)
    assert not same_bits(other.weights, ad.weights)
    other.load_state_dict(sd)
    assert same_bits(other.weights, ad.weights)
    lo, ha = mk(seed=1), mk(seed=1, algo="loha")
    assert set(lo.state_dict()) == {"rank", "alpha", "seed", "targets", "shapes", "weights", "kinds"}                # LoRA's and LoHa's states
    assert set(ha.state_dict()) == {"rank", "alpha", "seed", "targets", "shapes", "weights", "kinds", "algo"}        # are what they were
    refusals = [(ad, lo.state_dict(), "lora_algo"), (ad, ha.state_dict(), "lora_algo"), (lo, sd, "lora_algo"), (ha, sd, "lora_algo"),
                (mk(seed=1, algo="kronecker", factor=-1), sd, "factor"), (mk(seed=1, algo="kronecker", factor=2, full=True), sd, "full")]
    for holder, state, msg in refusals:
        before = holder.weights.clone()
        with pytest.raises(ValueError, match="lora state: " + msg):
            holder.load_state_dict(state)
        assert same_bits(holder.weights, before)
    a = _trainer(net, lora_rank=4, lora_algo="kronecker", lora_targets=["to_q"])
    b = _trainer(net, lora_rank=4, lora_targets=["to_q"])
    c = _trainer(net, lora_rank=4, lora_algo="kronecker", lokr_factor=2, lora_targets=["to_q"])
    for src, dst, sub, msg in ((a, b, "kr", "lora_algo"), (b, a, "ra", "lora_algo"), (a, c, "fa", "factor")):
        d = tmp_path / sub
        d.mkdir()
        torch.save(src.lora.state_dict(), str(d / "lora_state.pt"))
        before = dst.lora.weights.clone()
        with pytest.raises(ValueError, match=msg):
            dst.load_lora_state(d)
        assert same_bits(dst.lora.weights, before)


def test_export_names_shapes_and_the_rebuilt_delta(net, tmp_path):
    from safetensors.torch import load_file
    r, alpha = 8, 2.0
    tr = _trainer(net, lora_rank=r, lora_alpha=alpha, lora_algo="kronecker", lora_target_kinds="all", lora_seed=2,
                  lora_targets=[k[: -len(".weight")] for k in ONE_OF_EACH.values()])
    ad = tr.lora
    g = torch.Generator().manual_seed(7)
    for k in ad.targets:
        zero = ad.W2(k) if ad.geometry[k]["full"] else ad.A(k)
        zero.copy_(bf(torch.randn(zero.shape, generator=g) * 0.1))
    d = tr.save_checkpoint(tmp_path / "ck")
    assert (d / "lycoris_lokr.safetensors").exists() and not (d / "pytorch_lora_weights.safetensors").exists() and (d / "lora_state.pt").exists()
    st = torch.load(str(d / "lora_state.pt"), weights_only=True)
    assert (st["algo"], st["factor"], st["full"]) == ("kronecker", -1, False)
    ex = load_file(str(d / "lycoris_lokr.safetensors"))
    assert set(ex) == set(ad.export_tensors())
    assert all(re.fullmatch(r"lora_unet_[A-Za-z0-9_]+\.(lokr_w1|lokr_w2|lokr_w2_a|lokr_w2_b|alpha)", k) for k in ex)
    forms = set()
    for kind, k in ONE_OF_EACH.items():
        shape = net.shapes[k]
        khw = 9 if len(shape) == 4 and shape[2] == 3 else 1
        out_l, out_k, in_m, in_n, n2 = KR.geometry(shape[0], shape[1], khw, -1)
        full = KR.rule_full(out_k, in_n, r)
        forms.add(full)
        pre = "lora_unet_" + k[: -len(".weight")].replace(".", "_")
        w1, a = ex[f"{pre}.lokr_w1"], ex[f"{pre}.alpha"]
        assert w1.shape == (out_l, in_m) and a.shape == () and float(a) == (float(r) if full else alpha), kind
        assert torch.equal(w1, ad.C(k).float())                          # s is not folded in
        if full:
            w2 = ex[f"{pre}.lokr_w2"]
            assert w2.shape == ((out_k, in_n) if len(shape) == 2 else (out_k, in_n, shape[2], shape[3])) and f"{pre}.lokr_w2_a" not in ex, kind
            assert torch.equal(w2.reshape(out_k, n2), ad.W2(k).float())
            f = (ad.C(k), ad.W2(k), None)
        else:
            wa, wb = ex[f"{pre}.lokr_w2_a"], ex[f"{pre}.lokr_w2_b"]
            assert wa.shape == (out_k, r) and wb.shape == (r, n2) and f"{pre}.lokr_w2" not in ex, kind
            assert torch.equal(wa, ad.B(k).float()) and torch.equal(wb, ad.A(k).float())
            w2 = (wa.double() @ wb.double()).reshape((out_k, in_n) + tuple(shape[2:]))
            f = (ad.C(k), ad.B(k), ad.A(k))
        assert all(t.dtype == torch.float32 for t in ex.values())
        # what a LyCORIS loader forms: (alpha / r) kron(w1, w2), 4-D for a convolution
        w1d = w1.double()[:, :, None, None] if len(shape) == 4 else w1.double()
        rebuilt = (float(a) / r) * torch.kron(w1d, w2.double())
        want = KR.delta64(*f, ad.target_scale(k))
        assert tuple(rebuilt.shape) == tuple(shape)
        assert torch.equal(rebuilt.reshape(want.shape), want) and float(want.abs().max()) > 0, kind
    assert forms == {True, False}
    # LoRA and LoHa trainers keep their files
    d2 = _trainer(net, lora_rank=r, lora_targets=["attn1.to_q"]).save_checkpoint(tmp_path / "ck2")
    assert (d2 / "pytorch_lora_weights.safetensors").exists() and not (d2 / "lycoris_lokr.safetensors").exists()
    d3 = _trainer(net, lora_rank=r, lora_algo="loha", lora_targets=["attn1.to_q"]).save_checkpoint(tmp_path / "ck3")
    assert (d3 / "lycoris_loha.safetensors").exists() and not (d3 / "lycoris_lokr.safetensors").exists()
