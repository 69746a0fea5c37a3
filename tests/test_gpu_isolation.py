"""Operand isolation on a real MI355X: no op entry point of the C ABI may read or write outside its operands.

Every case places the operands of one call inside a larger allocation (tests/_isolation.py: guard bands of at least 256 rows before
and after each operand, the `ld - cols` column gaps where the entry point takes leading dimensions) and runs the call three times on the
same operand contents with the surroundings filled with 0x00, 0xFF (NaN in bf16 and fp32) and 0x7F (3.39e38, finite: it survives the
fmaxf / comparison that swallows a NaN).  Outputs and scratch operands the op is documented to write before reading START as the pattern.

  1. every output is finite;
  2. the outputs of the 0xFF and 0x7F runs have THE BITS of the 0x00 run;
  3. every guard byte and every read-only operand is untouched;
  4. the 0x00 run meets the bar of the corresponding tests/test_gpu_ops.py test against the same fp32 reference ("equal but both wrong").

Cross-row form, where rows / samples are independent by definition: the OTHER rows' operand contents are overwritten with the pattern and
the kept rows' outputs must keep their bits.

Bit equality is the rule.  One output is held to 1e-5 * max|out| instead (the project's bar for reordered fp32 atomics,
test_grad_accumulation_is_sum_of_micro_steps): the up-sampler weight gradient's dbias, to which the four phase planes add with
atomicAdd in an order the hardware chooses (csrc/gemm.hip:727).  Every other atomicAdd these cases reach has ONE writer per element and
launch (csrc/kernels.h:182 gemm_bias_out unsplit; csrc/norm.hip:660 with one row chunk), which is bit-stable.

What these tests cannot see: a read beyond the ALLOCATION whose value is then masked leaves no trace in a result -- they bound influence,
not addresses.  Library-owned scratch cannot be pattern-filled from outside: g_sumsq_partials, the split-K / partial slabs of the test
entry points (test_slab: attn_part_floats, the LayerNorm partial rows, the loss partials), the conditioning-gradient slab."""
import ctypes as C
import math
import time

import pytest
import torch

import sdxl_amd  # noqa: F401
from sdxl_amd import lib

from _isolation import Spec, assert_isolated, run_isolated, same_bits
from test_gpu_ops import _attn_ref, _conv_ref, geglu_pack_rows, geglu_unpack_cols, report

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF, F32 = torch.bfloat16, torch.float32
ATOMIC_UPCONV_DBIAS = ("db",)       # csrc/gemm.hip:727: up2 == 1 adds the four phase planes' column sums with atomicAdd


@pytest.fixture(scope="module")
def L():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    t0 = time.perf_counter()
    yield lib.load()
    torch.cuda.synchronize()
    print(f"[isolation] module wall time {time.perf_counter() - t0:.1f} s")


def rnd(*shape, seed=0, scale=1.0, shift=0.0):
    """bf16-valued fp32 on the host (the arena casts; the reference reads the same values)"""
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale + shift).to(BF).float()


def I(name, t, gap=0, dtype=BF, role="in"):
    t2 = t.reshape(1, -1) if t.dim() == 1 else t.reshape(-1, t.shape[-1])
    return Spec(name, t2.shape[0], t2.shape[1], t2.shape[1] + gap, dtype, t2, role)


def O(name, rows, cols, gap=0, dtype=BF, role="out"):
    return Spec(name, rows, cols, cols + gap, dtype, None, role)


def P(a, name, off=0):
    return C.c_void_p(a.ptr(name, off))


def st():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def d(t):
    return t.to(DEV)


def run(fn, specs, **kw):
    return run_isolated(fn, specs, device=DEV, **kw)


def only(runs, names):
    return [{k: r[k] for k in names} for r in runs]


# ------------------------------------------------------------------------------------------------------------------ GEMM NT / NN
def _gemm_route(L, form, M, N, K, cfg, mode, **more):
    """which kernel the launch reaches under gemm mode `mode`: the library's own answer (sdxl_debug_gemm_route = gemm_route, csrc/gemm.hip)"""
    lib.check(L.sdxl_set_gemm_mode(mode))
    try:
        return lib.gemm_route(form=form, M=M, N=N, K=K, cfg=cfg, **more)
    finally:
        lib.check(L.sdxl_set_gemm_mode(1))


def _gemm_ld_case(L, form, M, N, K, cfg, mode=1, cross=False):
    a, bias, res = rnd(M, K, seed=1), rnd(N, seed=3), rnd(M, N, seed=4)
    w = rnd(N, K, seed=2, scale=K ** -0.5) if form == 0 else rnd(K, N, seed=6, scale=K ** -0.5)
    specs = [I("A", a, 8), I("B", w, 8), I("bias", bias), I("res", res, 8), O("C", M, N, 8)]

    def fn(ar):
        lib.check(L.sdxl_op_gemm_ld(form, P(ar, "A"), P(ar, "B"), P(ar, "C"), M, N, K, ar.ld("A"), ar.ld("B"), ar.ld("C"), P(ar, "bias"),
                                    P(ar, "res"), ar.ld("res"), cfg, st()))
    what = f"gemm_ld form {form} {M}x{N}x{K} cfg {cfg} mode {mode}{' cross-row' if cross else ''}"
    print(f"[isolation] {what}: {_gemm_route(L, form, M, N, K, cfg, mode)}")
    lib.check(L.sdxl_set_gemm_mode(mode))
    try:
        runs = run(fn, specs, poison={"A": slice(150, M), "res": slice(150, M)} if cross else None)
    finally:
        lib.check(L.sdxl_set_gemm_mode(1))
    assert_isolated(runs, rows={"C": slice(0, 150)} if cross else None, what=what)
    ref = d(a) @ (d(w).t() if form == 0 else d(w)) + d(bias) + d(res)
    report(what, runs[0]["C"], ref, 6e-3)


# (304, 320, 128) is not the issue's: at its three shapes M % 8 != 0 keeps the co-resident kernel away and N % 160 != 0 turns 3 / 13 / 23
# into 1 (the entry point's own fall-back); this one reaches them with a partial 256-row tile
@pytest.mark.parametrize("cfg", [0, 1, 2, 3, 13, 23, 31, 32])
@pytest.mark.parametrize("M,N,K", [(300, 200, 128), (4, 136, 64), (129, 128, 192), (304, 320, 128)])
@pytest.mark.parametrize("form", [0, 1], ids=["nt", "nn"])
def test_gemm_nt_nn_with_gaps_on_every_leading_dimension(L, form, M, N, K, cfg):
    _gemm_ld_case(L, form, M, N, K, cfg)


# (300, 256, 128) is the issue's: M % 256 != 0, so gemm256_applicable turns it away and the 128-row kernel runs under mode 2.  The 256 x 256
# kernel itself (whole tiles only: M, N % 256 == 0, K % 64 == 0) runs at (256, 256, 128) and (512, 256, 128): its edges are the ld gaps
@pytest.mark.parametrize("M,N,K,route", [(300, 256, 128, "128-row"), (256, 256, 128, "256 x 256"), (512, 256, 128, "256 x 256")])
@pytest.mark.parametrize("form", [0, 1], ids=["nt", "nn"])
def test_gemm_nt_nn_under_gemm_mode_2(L, form, M, N, K, route):
    assert _gemm_route(L, form, M, N, K, 0, 2)["kernel"] == route.replace(" ", "")
    _gemm_ld_case(L, form, M, N, K, 0, mode=2)


@pytest.mark.parametrize("form", [0, 1], ids=["nt", "nn"])
def test_gemm_rows_are_independent(L, form):
    _gemm_ld_case(L, form, 300, 200, 128, 0, cross=True)


# ------------------------------------------------------------------------------------------------------------------ GEMM TN (wgrad)
@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("M,N,rows,splitk", [(200, 72, 1000, 1), (200, 72, 1000, 3), (320, 136, 988, 1), (320, 136, 988, 3),
                                             (200, 72, 16384, 0), (200, 72, 16384, 3)])      # 16384 rows: the long-reduction kernel (wgrad256.hip)
def test_gemm_tn_weight_gradient(L, M, N, rows, splitk, accumulate):
    """accumulate 0: C starts as the pattern and must be overwritten; 1: C starts as a known tensor.  dbias is a += accumulator."""
    a, b, base = rnd(rows, M, seed=8), rnd(rows, N, seed=9), rnd(M, N, seed=10)
    specs = [I("A", a), I("B", b), I("db", torch.zeros(M), dtype=F32, role="inout"),
             I("C", base, dtype=F32, role="inout") if accumulate else O("C", M, N, dtype=F32)]

    def fn(ar):
        lib.check(L.sdxl_op_gemm(2, P(ar, "A"), P(ar, "B"), P(ar, "C"), M, N, rows, P(ar, "db"), None, accumulate, splitk, st()))
    what = f"gemm_tn {M}x{N}x{rows} splitk {splitk} acc {accumulate}"
    runs = run(fn, specs)
    assert_isolated(runs, what=what)
    ref = d(a).t() @ d(b)
    report(what, runs[0]["C"] - (d(base) if accumulate else 0.0), ref, 2e-5 * math.sqrt(rows) + 1e-5)
    report(what + " bias grad", runs[0]["db"][0], d(a).sum(0), 1e-4)


def test_grouped_weight_gradients(L):
    n, Mo, No, rows = 2, 128, 160, 1000
    dys, xs = [rnd(rows, Mo, seed=20 + i) for i in range(n)], [rnd(rows, No, seed=30 + i) for i in range(n)]
    specs = []
    for i in range(n):
        specs += [I(f"dy{i}", dys[i]), I(f"x{i}", xs[i]), O(f"dw{i}", Mo, No, dtype=F32), I(f"db{i}", torch.zeros(Mo), dtype=F32, role="inout")]

    def fn(ar):
        arr = lambda k: (C.c_void_p * n)(*[ar.ptr(f"{k}{i}") for i in range(n)])
        lib.check(L.sdxl_op_wgrad_group(n, arr("dy"), arr("x"), arr("dw"), arr("db"), Mo, No, rows, 0, st()))
    runs = run(fn, specs)
    assert_isolated(runs, what="wgrad group")
    tol = 2e-5 * math.sqrt(rows) + 1e-5
    for i in range(n):
        report(f"wgrad group [{i}]", runs[0][f"dw{i}"], d(dys[i]).t() @ d(xs[i]), tol)
        report(f"wgrad group bias grad [{i}]", runs[0][f"db{i}"][0], d(dys[i]).sum(0), tol)


# ------------------------------------------------------------------------------------------------------------------ convolution
def _conv_case(L, B, H, W, Cin, Cout, stride, cross=False):
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    x, w, bias = rnd(B, H, W, Cin, seed=10), rnd(Cout, 9 * Cin, seed=11, scale=(9 * Cin) ** -0.5), rnd(Cout, seed=12)
    dy, base = rnd(B, Ho, Wo, Cout, seed=13), rnd(Cout, 9 * Cin, seed=14)
    specs = [I("x", x), I("w", w), I("bias", bias), I("dy", dy), O("y", B * Ho * Wo, Cout), O("dx", B * H * W, Cin),
             O("dw", Cout, 9 * Cin, dtype=F32), I("db", torch.zeros(Cout), dtype=F32, role="inout"), I("dw2", base, dtype=F32, role="inout")]

    def fn(ar):
        lib.check(L.sdxl_op_conv3x3_fwd(P(ar, "x"), P(ar, "w"), P(ar, "bias"), P(ar, "y"), B, H, W, Cin, Cout, stride, st()))
        lib.check(L.sdxl_op_conv3x3_dgrad(P(ar, "dy"), P(ar, "w"), P(ar, "dx"), B, H, W, Cin, Cout, stride, st()))
        lib.check(L.sdxl_op_conv3x3_wgrad2(P(ar, "x"), P(ar, "dy"), P(ar, "dw"), P(ar, "db"), B, H, W, Cin, Cout, stride, 0, 0, st()))      # the plan's split, =
        lib.check(L.sdxl_op_conv3x3_wgrad2(P(ar, "x"), P(ar, "dy"), P(ar, "dw2"), None, B, H, W, Cin, Cout, stride, 3, 1, st()))            # forced split, +=
    what = f"conv {B}x{H}x{W} {Cin}->{Cout} s{stride}{' cross-image' if cross else ''}"
    if cross:      # image 1 of x / dy is the pattern: images 0 and 2 of y / dx keep their bits (the halo rows at both seams)
        runs = run(fn, specs, poison={"x": slice(H * W, 2 * H * W), "dy": slice(Ho * Wo, 2 * Ho * Wo)})
        keep = lambda n: torch.cat([torch.arange(0, n), torch.arange(2 * n, 3 * n)]).to(DEV)
        assert_isolated(only(runs, ("y", "dx")), rows={"y": keep(Ho * Wo), "dx": keep(H * W)}, what=what)
    else:
        runs = run(fn, specs)
        assert_isolated(runs, what=what)
    xr, wr = d(x).requires_grad_(True), d(w).view(Cout, 9, Cin).requires_grad_(True)
    ref = _conv_ref(xr, wr, d(bias), stride)
    ref.backward(d(dy))
    report(what + " fwd", runs[0]["y"].view(B, Ho, Wo, Cout), ref.detach(), 6e-3)
    report(what + " dgrad", runs[0]["dx"].view(B, H, W, Cin), xr.grad, 6e-3)
    tol = 1e-4 * math.sqrt(B * Ho * Wo) / 8 + 1e-5
    report(what + " wgrad =", runs[0]["dw"].view(Cout, 9, Cin), wr.grad, tol)
    report(what + " wgrad += splitk 3", (runs[0]["dw2"] - d(base)).view(Cout, 9, Cin), wr.grad, tol)
    report(what + " bias grad", runs[0]["db"][0], d(dy).sum((0, 1, 2)), 1e-4)


@pytest.mark.parametrize("B,H,W,Cin,Cout,stride", [(3, 12, 20, 72, 64, 1), (3, 12, 20, 72, 64, 2),      # 720 / 180 pixels: ragged 128-row tiles, two image seams
                                                   (2, 16, 64, 64, 64, 1),                               # the W % 64 == 0 branch
                                                   (1, 128, 128, 8, 64, 1)])                             # 16384 pixels: the three-tap weight gradient
def test_conv3x3_fwd_dgrad_wgrad(L, B, H, W, Cin, Cout, stride):
    _conv_case(L, B, H, W, Cin, Cout, stride)


@pytest.mark.parametrize("stride", [1, 2])
def test_conv3x3_images_are_independent(L, stride):
    _conv_case(L, 3, 12, 20, 72, 64, stride, cross=True)


@pytest.mark.parametrize("with_addend", [False, True])
def test_conv3x3_stride2_dgrad_by_output_phase(L, with_addend):
    B, H, W, Cin, Cout = 3, 12, 20, 72, 64
    px = B * (H // 2) * (W // 2)
    x0, w, dy, add = rnd(B, H, W, Cin, seed=30), rnd(Cout, 9 * Cin, seed=31, scale=(9 * Cin) ** -0.5), rnd(B, H // 2, W // 2, Cout, seed=32), rnd(B, H, W, Cin, seed=33)
    specs = [I("dy", dy), I("w", w), O("planar", 4 * ((px + 127) // 128 * 128), Cin, role="scratch"), O("dx", B * H * W, Cin)] + ([I("add", add)] if with_addend else [])

    def fn(ar):
        lib.check(L.sdxl_op_conv3x3_s2_dgrad(P(ar, "dy"), P(ar, "w"), P(ar, "planar"), P(ar, "dx"), P(ar, "add") if with_addend else None, B, H, W, Cin, Cout, st()))
    runs = run(fn, specs)
    assert_isolated(runs, what="conv s2 dgrad by phase")
    xr = d(x0).requires_grad_(True)
    _conv_ref(xr, d(w).view(Cout, 9, Cin), None, 2).backward(d(dy))
    report(f"conv s2 dgrad by phase addend={with_addend}", runs[0]["dx"].view(B, H, W, Cin), xr.grad + (d(add) if with_addend else 0.0), 8e-3)


# ------------------------------------------------------------------------------------------------------------------ up-sampler pair
# (1, 26, 38): 988 low-resolution pixels, 36 pad rows per plane; the weight-gradient form takes whole 64-pixel reduction steps only (the plan
# falls back otherwise), so it runs at (2, 20, 48) and at (1, 24, 40) -- the nearest accepted shape WITH pad rows (960 pixels, 64 per plane)
@pytest.mark.parametrize("B,H,W,Cin,Cout", [(1, 26, 38, 128, 64), (2, 20, 48, 128, 64), (1, 24, 40, 128, 64)])
def test_upsample_conv3x3_fwd_dgrad_wgrad(L, B, H, W, Cin, Cout):
    px = B * H * W
    wgrad = px % 64 == 0
    x, w, bias = rnd(B, H, W, Cin, seed=20), rnd(Cout, 9 * Cin, seed=21, scale=(9 * Cin) ** -0.5), rnd(Cout, seed=22)
    dy, add, base = rnd(B, 2 * H, 2 * W, Cout, seed=23), rnd(B, H, W, Cin, seed=24), rnd(Cout, 9 * Cin, seed=25)
    specs = [I("x", x), I("w", w), I("bias", bias), I("dy", dy), I("add", add), O("weff", Cout, 16 * Cin), O("y", 4 * px, Cout), O("dx", px, Cin),
             O("planar", 4 * ((px + 127) // 128 * 128), Cout, role="scratch")]
    if wgrad:
        specs += [O("dweff", Cout, 16 * Cin, dtype=F32, role="scratch"), O("dw", Cout, 9 * Cin, dtype=F32), I("dw2", base, dtype=F32, role="inout"),
                  I("db", torch.zeros(Cout), dtype=F32, role="inout")]

    def fn(ar):
        lib.check(L.sdxl_op_upconv3x3_fwd(P(ar, "x"), P(ar, "w"), P(ar, "bias"), P(ar, "weff"), P(ar, "planar"), P(ar, "y"), B, H, W, Cin, Cout, st()))
        lib.check(L.sdxl_op_upconv3x3_dgrad(P(ar, "dy"), P(ar, "weff"), P(ar, "planar"), P(ar, "dx"), P(ar, "add"), B, H, W, Cin, Cout, st()))
        if wgrad:
            lib.check(L.sdxl_op_upconv3x3_wgrad(P(ar, "planar"), P(ar, "x"), P(ar, "dweff"), P(ar, "dw"), P(ar, "db"), 0, B, H, W, Cin, Cout, 1, st()))
            lib.check(L.sdxl_op_upconv3x3_wgrad(P(ar, "planar"), P(ar, "x"), P(ar, "dweff"), P(ar, "dw2"), None, 1, B, H, W, Cin, Cout, 3, st()))
    what = f"upconv {B}x{H}x{W} {Cin}->{Cout}"
    runs = run(fn, specs)
    assert_isolated(runs, atomic=ATOMIC_UPCONV_DBIAS, what=what)
    xr = d(x).requires_grad_(True)
    wr = d(w).view(Cout, 3, 3, Cin).permute(0, 3, 1, 2).clone().requires_grad_(True)
    br = d(bias).clone().requires_grad_(True)
    up = torch.nn.functional.interpolate(xr.permute(0, 3, 1, 2), scale_factor=2.0, mode="nearest")
    ref = torch.nn.functional.conv2d(up, wr, br, padding=1).permute(0, 2, 3, 1)
    ref.backward(d(dy))
    report(what + " fwd", runs[0]["y"].view(B, 2 * H, 2 * W, Cout), ref.detach(), 8e-3)
    report(what + " dgrad", runs[0]["dx"].view(B, H, W, Cin), xr.grad + d(add), 8e-3)
    if wgrad:
        dw_ref = wr.grad.permute(0, 2, 3, 1).reshape(Cout, 9 * Cin)
        tol = 1e-4 * math.sqrt(4 * px) / 8 + 1e-5
        report(what + " wgrad =", runs[0]["dw"], dw_ref, tol)
        report(what + " wgrad += splitk 3", runs[0]["dw2"] - d(base), dw_ref, tol)
        report(what + " bias grad", runs[0]["db"][0], br.grad, tol)


# ------------------------------------------------------------------------------------------------------------------ attention
def _attn_bwd_route(B, heads, Nq, Nk):
    """which backward sdxl_op_attention_bwd reaches, restated from attn_pick_qsplit / launch_attn_bwd / launch_attn_bwd_fused
    (csrc/attention.hip; every leading dimension here is a multiple of 8): the entry point splits the queries of the dK / dV kernel so that
    about 160 workgroups run (at most Nq / 128 ways), and a split problem, like one with Nk < 256, takes the two-launch form"""
    ceil = lambda a, b: (a + b - 1) // b
    qsplit = min(max(160 // (ceil(Nk, 64) * B * heads), 1), max(ceil(Nq, 64) // 2, 1), 16)
    if qsplit > 1:
        return f"dQ, then dK / dV split {qsplit} ways + reduce"
    if Nk < 256:
        return "dQ, then dK / dV"
    return "pipelined (attention_bwd_pl.hip)" if Nq >= 2048 and Nk >= 2048 else "fused tiled (attn_bwd_fused_kernel)"


# The first four shapes are the issue's.  At all of them the entry point's own rule splits the dK / dV kernel's queries, so they run the
# two-launch backward with the split and the reduce; the fused tiled and the pipelined backward need an unsplit problem, which is one with
# more than 80 (64-key block, batch, head) triples or at most 192 queries: (2, 1, 136, 257) and (2, 9, 264, 257) reach the first
# (two and three 128-query tiles, the last one partial), (1, 3, 2056, 2056) and (2, 2, 2056, 2056) the second (32 full tiles + 8; its ranges of 16
# blocks run across (batch, head) pairs, so it gets the cross-batch form too)
ATTENTION = [(2, 2, 200, 77, False, "dQ, then dK / dV split 2 ways + reduce"), (2, 1, 264, 257, False, "dQ, then dK / dV split 2 ways + reduce"),
             (1, 1, 2056, 2056, False, "dQ, then dK / dV split 4 ways + reduce"), (2, 2, 200, 200, True, "dQ, then dK / dV split 2 ways + reduce"),
             (2, 1, 136, 257, False, "fused tiled (attn_bwd_fused_kernel)"), (2, 9, 264, 257, False, "fused tiled (attn_bwd_fused_kernel)"),
             (1, 3, 2056, 2056, False, "pipelined (attention_bwd_pl.hip)"), (2, 2, 2056, 2056, False, "pipelined (attention_bwd_pl.hip)")]


@pytest.mark.parametrize("B,heads,Nq,Nk,self_attn,route,cross", [s + (False,) for s in ATTENTION] + [s + (True,) for s in ATTENTION if s[0] > 1])      # (B = 1: no other batch entry to poison)
def test_attention_fwd_bwd(L, B, heads, Nq, Nk, self_attn, route, cross):
    print(f"[isolation] attention backward B{B} h{heads} {Nq}x{Nk}: {_attn_bwd_route(B, heads, Nq, Nk)}")
    assert _attn_bwd_route(B, heads, Nq, Nk) == route
    Cc = heads * 64
    do = rnd(B, Nq, Cc, seed=23)
    common = [I("do", do, 8), O("o", B * Nq, Cc, 8), O("lse", B * heads, Nq, dtype=F32), O("delta", B * heads, Nq, dtype=F32)]
    if self_attn:      # one fused [B][N][3 Cc + 8] buffer, and the same for the gradients
        qkv = rnd(B, Nq, 3 * Cc, seed=20)
        q, k, v = qkv[..., :Cc], qkv[..., Cc:2 * Cc], qkv[..., 2 * Cc:]
        specs = [I("qkv", qkv, 8), O("dqkv", B * Nq, 3 * Cc, 8)] + common
        where = lambda ar: (P(ar, "qkv"), P(ar, "qkv", Cc), P(ar, "qkv", 2 * Cc), P(ar, "dqkv"), P(ar, "dqkv", Cc), P(ar, "dqkv", 2 * Cc), ar.ld("qkv"), ar.ld("qkv"))
        poison = {"qkv": slice(Nq, 2 * Nq), "do": slice(Nq, 2 * Nq)}
    else:              # cross-attention layout: ldq = Cc + 8, ldk = ldv = 2 Cc + 8
        q, kv = rnd(B, Nq, Cc, seed=21), rnd(B, Nk, 2 * Cc, seed=22)
        k, v = kv[..., :Cc], kv[..., Cc:]
        specs = [I("q", q, 8), I("kv", kv, 8), O("dq", B * Nq, Cc, 8), O("dkv", B * Nk, 2 * Cc, 8)] + common
        where = lambda ar: (P(ar, "q"), P(ar, "kv"), P(ar, "kv", Cc), P(ar, "dq"), P(ar, "dkv"), P(ar, "dkv", Cc), ar.ld("q"), ar.ld("kv"))
        poison = {"q": slice(Nq, 2 * Nq), "kv": slice(Nk, 2 * Nk), "do": slice(Nq, 2 * Nq)}

    def fn(ar):
        pq, pk, pv, pdq, pdk, pdv, ldq, ldk = where(ar)
        lib.check(L.sdxl_op_attention_fwd(pq, pk, pv, P(ar, "o"), P(ar, "lse"), B, heads, Nq, Nk, ldq, ldk, ldk, ar.ld("o"), st()))
        lib.check(L.sdxl_op_attention_bwd(pq, pk, pv, P(ar, "o"), P(ar, "do"), P(ar, "lse"), P(ar, "delta"), pdq, pdk, pdv, B, heads, Nq, Nk,
                                          ldq, ldk, ldk, ar.ld("o"), st()))
    what = f"attention B{B} h{heads} {Nq}x{Nk} {'self' if self_attn else 'cross-attention'} layout{' cross-batch' if cross else ''}"
    runs = run(fn, specs, poison=poison if cross else None)
    keep = None
    if cross:      # batch 0 of every output
        keep = {n: slice(0, Nq) for n in ("o", "dq", "dqkv")}
        keep.update({"dkv": slice(0, Nk), "lse": slice(0, heads), "delta": slice(0, heads)})
    assert_isolated(runs, rows=keep, what=what)
    qr, kr, vr = (d(t).contiguous().requires_grad_(True) for t in (q, k, v))
    ref, lse_ref = _attn_ref(qr, kr, vr, heads)
    ref.backward(d(do))
    r = runs[0]
    report(what + " o", r["o"].view(B, Nq, Cc), ref.detach(), 8e-3)
    report(what + " lse", r["lse"].view(B, heads, Nq), lse_ref.detach(), 1e-3)
    if self_attn:
        g = r["dqkv"].view(B, Nq, 3 * Cc)
        dq, dk, dv = g[..., :Cc], g[..., Cc:2 * Cc], g[..., 2 * Cc:]
    else:
        dq, g = r["dq"].view(B, Nq, Cc), r["dkv"].view(B, Nk, 2 * Cc)
        dk, dv = g[..., :Cc], g[..., Cc:]
    for name, got, rf in (("dQ", dq, qr.grad), ("dK", dk, kr.grad), ("dV", dv, vr.grad)):
        report(f"{what} {name}", got, rf, 1.5e-2)


# ------------------------------------------------------------------------------------------------------------------ norms
@pytest.mark.parametrize("B,HW,Cc,silu", [(2, 100, 320, 1), (2, 100, 2560, 0)])
@pytest.mark.parametrize("cross", [False, True], ids=["surroundings", "cross-sample"])
def test_groupnorm_fwd_bwd(L, B, HW, Cc, silu, cross):
    G, eps = 32, 1e-5
    x, dy = rnd(B * HW, Cc, seed=40, scale=3.0, shift=1.5), rnd(B * HW, Cc, seed=43)
    gamma, beta = rnd(Cc, seed=41, scale=0.1, shift=1.0), rnd(Cc, seed=42)
    nws = 256 * B * Cc * 2 + 256 * B * G * 2 + B * Cc * 5          # the size tests/test_gpu_ops.py::test_groupnorm_fwd_bwd gives it
    zeros = lambda n: I(n, torch.zeros(Cc), dtype=F32, role="inout")
    specs = [I("x", x), I("dy", dy), I("gamma", gamma), I("beta", beta), O("y", B * HW, Cc), O("stats", B, 2 * G, dtype=F32), O("dx", B * HW, Cc),
             O("ws", 1, nws, dtype=F32, role="scratch"), zeros("dg"), zeros("db")]

    def fn(ar):
        lib.check(L.sdxl_op_groupnorm_fwd(P(ar, "x"), P(ar, "y"), P(ar, "gamma"), P(ar, "beta"), P(ar, "stats"), P(ar, "ws"), B, HW, Cc, G, eps, silu, st()))
        lib.check(L.sdxl_op_groupnorm_bwd(P(ar, "x"), P(ar, "dy"), P(ar, "gamma"), P(ar, "beta"), P(ar, "stats"), P(ar, "dx"), P(ar, "dg"), P(ar, "db"),
                                          P(ar, "ws"), B, HW, Cc, G, silu, 0, st()))
    what = f"groupnorm B{B} HW{HW} C{Cc} silu{silu}{' cross-sample' if cross else ''}"
    if cross:
        runs = run(fn, specs, poison={"x": slice(HW, 2 * HW), "dy": slice(HW, 2 * HW)})
        assert_isolated(only(runs, ("y", "stats", "dx")), rows={"y": slice(0, HW), "dx": slice(0, HW), "stats": slice(0, 1)}, what=what)
    else:
        runs = run(fn, specs)
        assert_isolated(runs, what=what)
    xr, gr, br = (d(t).requires_grad_(True) for t in (x.view(B, HW, Cc), gamma, beta))
    n = torch.nn.functional.group_norm(xr.permute(0, 2, 1), G, gr, br, eps).permute(0, 2, 1)
    ref = torch.nn.functional.silu(n) if silu else n
    ref.backward(d(dy).view(B, HW, Cc))
    report(what + " fwd", runs[0]["y"].view(B, HW, Cc), ref.detach(), 8e-3)
    report(what + " dx", runs[0]["dx"].view(B, HW, Cc), xr.grad, 1e-2)
    report(what + " dgamma", runs[0]["dg"][0], gr.grad, 2e-3)
    report(what + " dbeta", runs[0]["db"][0], br.grad, 2e-3)


@pytest.mark.parametrize("M,Cc", [(70, 640), (300, 1280), (16, 256)])
@pytest.mark.parametrize("cross", [False, True], ids=["surroundings", "cross-row"])
def test_layernorm_fwd_bwd(L, M, Cc, cross):
    x, dy = rnd(M, Cc, seed=50, scale=2.0, shift=0.5), rnd(M, Cc, seed=53)
    gamma, beta = rnd(Cc, seed=51, scale=0.1, shift=1.0), rnd(Cc, seed=52)
    zeros = lambda n: I(n, torch.zeros(Cc), dtype=F32, role="inout")
    specs = [I("x", x), I("dy", dy), I("gamma", gamma), I("beta", beta), O("y", M, Cc), O("stats", M, 2, dtype=F32), O("dx", M, Cc), zeros("dg"), zeros("db")]

    def fn(ar):
        lib.check(L.sdxl_op_layernorm_fwd(P(ar, "x"), P(ar, "y"), P(ar, "gamma"), P(ar, "beta"), P(ar, "stats"), M, Cc, 1e-5, st()))
        lib.check(L.sdxl_op_layernorm_bwd(P(ar, "x"), P(ar, "dy"), P(ar, "gamma"), P(ar, "stats"), P(ar, "dx"), P(ar, "dg"), P(ar, "db"), M, Cc, 0, st()))
    what = f"layernorm {M}x{Cc}{' cross-row' if cross else ''}"
    h = M // 2
    if cross:
        runs = run(fn, specs, poison={"x": slice(h, M), "dy": slice(h, M)})
        assert_isolated(only(runs, ("y", "stats", "dx")), rows={n: slice(0, h) for n in ("y", "stats", "dx")}, what=what)
    else:
        runs = run(fn, specs)
        assert_isolated(runs, what=what)
    xr, gr, br = (d(t).requires_grad_(True) for t in (x, gamma, beta))
    ref = torch.nn.functional.layer_norm(xr, (Cc,), gr, br, 1e-5)
    ref.backward(d(dy))
    report(what + " fwd", runs[0]["y"], ref.detach(), 8e-3)
    report(what + " dx", runs[0]["dx"], xr.grad, 1e-2)
    report(what + " dgamma", runs[0]["dg"][0], gr.grad, 2e-3)
    report(what + " dbeta", runs[0]["db"][0], br.grad, 2e-3)


# ------------------------------------------------------------------------------------------------------------------ GEGLU, Delta epilogue
# (308, 320, 1280, 64) is the issue's: M % 256 != 0 keeps it on the 128-row kernel also under mode 2; (256, 256, 256, 64), an op-test shape, is
# the smallest that reaches the 256 x 256 kernel's in-register GEGLU epilogues, forward (N = 512) and backward (N = 256)
@pytest.mark.parametrize("M,K,C4,G", [(100, 128, 160, 80), (308, 320, 1280, 64), (256, 256, 256, 64)])
@pytest.mark.parametrize("cross", [False, True], ids=["surroundings", "cross-row"])
def test_ff_geglu_fwd_bwd(L, M, K, C4, G, cross):
    x, dy = rnd(M, K, seed=60), rnd(M, K, seed=64)
    w1, b1, w2 = rnd(2 * C4, K, seed=61, scale=K ** -0.5), rnd(2 * C4, seed=62, scale=0.1), rnd(K, C4, seed=63, scale=C4 ** -0.5)
    specs = [I("x", x), I("w1", geglu_pack_rows(w1, C4, G)), I("b1", geglu_pack_rows(b1, C4, G)), I("w2", w2), I("dy", dy),
             O("u", M, 2 * C4), O("g", M, C4), O("du", M, 2 * C4)]

    def fn(ar):
        lib.check(L.sdxl_op_ff_geglu_fwd(P(ar, "x"), P(ar, "w1"), P(ar, "b1"), P(ar, "u"), P(ar, "g"), M, K, C4, G, st()))
        lib.check(L.sdxl_op_ff_geglu_bwd(P(ar, "dy"), P(ar, "w2"), P(ar, "u"), P(ar, "du"), M, K, C4, G, st()))
    what = f"ff geglu {M}x{K}x{C4} group {G}{' cross-row' if cross else ''}"
    h = M // 2
    mode = 2 if G == 64 else 1                                # as tests/test_gpu_ops.py::test_ff_geglu_fused_fwd_bwd
    print(f"[isolation] {what}: forward {_gemm_route(L, 0, M, 2 * C4, K, 0, mode, geglu=1, geglu_group=G)}, "
          f"backward {_gemm_route(L, 1, M, C4, K, 0, mode, geglu=2, geglu_group=G)}")
    lib.check(L.sdxl_set_gemm_mode(mode))
    try:
        runs = run(fn, specs, poison={"x": slice(h, M), "dy": slice(h, M)} if cross else None)
    finally:
        lib.check(L.sdxl_set_gemm_mode(1))
    assert_isolated(runs, rows={n: slice(0, h) for n in ("u", "g", "du")} if cross else None, what=what)
    report(what + " u", geglu_unpack_cols(runs[0]["u"], C4, G), d(x) @ d(w1).t() + d(b1), 6e-3)
    ub = geglu_unpack_cols(runs[0]["u"], C4, G).float().requires_grad_(True)
    a, t = ub.chunk(2, -1)
    gr = a * torch.nn.functional.gelu(t)
    report(what + " g", runs[0]["g"], gr.detach(), 6e-3)
    gr.backward(d(dy) @ d(w2))
    report(what + " du", geglu_unpack_cols(runs[0]["du"], C4, G), ub.grad, 1e-2)


def test_linear_dgrad_with_delta_epilogue(L):
    B, Nq, N, K = 3, 70, 128, 64
    M, heads = B * Nq, N // 64
    dy, w, o, add = rnd(M, K, seed=50), rnd(K, N, seed=51, scale=0.05), rnd(M, N, seed=52), rnd(M, N, seed=53)
    specs = [I("dy", dy), I("w", w), I("o", o), I("add", add), O("d_o", M, N), O("delta", B * heads, Nq, dtype=F32)]

    def fn(ar):
        lib.check(L.sdxl_op_linear_dgrad_delta(P(ar, "dy"), P(ar, "w"), P(ar, "o"), P(ar, "add"), P(ar, "d_o"), P(ar, "delta"), B, Nq, N, K, st()))
    runs = run(fn, specs)
    assert_isolated(runs, what="dgrad + Delta")
    report("dgrad + Delta dO", runs[0]["d_o"], d(dy) @ d(w) + d(add), 6e-3)
    dref = (runs[0]["d_o"].float() * d(o)).view(B, Nq, heads, 64).sum(-1).permute(0, 2, 1).reshape(B * heads, Nq)
    report("dgrad + Delta Delta", runs[0]["delta"], dref, 2e-3)


# ------------------------------------------------------------------------------------------------------------------ sampler step, loss
def _nhwc8(t):
    B, _c, H, W = t.shape
    o = torch.zeros(B * H * W, 8)
    o[:, :4] = t.permute(0, 2, 3, 1).reshape(B * H * W, 4)
    return o


def test_sampler_step(L):
    """(3, 6, 10): 180 pixels, no multiple of 256 threads nor of 8-element vectors; guidance + rescale (the per-sample sums go through
    library scratch).  Against the float64 restatement at the bar of tests/test_gpu_sampler.py::test_guidance_rescale: max |dx| <= 1e-5
    max |x_next| per sample; the input image is the bf16 of the state the kernel itself wrote (a_in = 0.5 is exact), both halves."""
    import numpy as np
    import _sampler_ref as SR
    B, H, W = 3, 6, 10
    g = torch.Generator().manual_seed(1)
    x, fc = torch.randn(B, 4, H, W, generator=g), rnd(B, 4, H, W, seed=2)
    fu = (0.8 * fc + 0.3 * torch.randn(B, 4, H, W, generator=g)).to(BF).float()
    k = dict(cfg=1, init=0, a_skip=0.75, a_out=-0.5, p=0.25, q=0.75, a_in_next=0.5, clamp=0.0, guidance=5.0, guidance_rescale=float(np.float32(0.7)))
    specs = [I("x", x.reshape(B * 4, H * W), dtype=F32, role="inout"), I("pred", _nhwc8(torch.cat([fc, fu]))), O("x_in", 2 * B * H * W, 8)]

    def fn(ar):
        s = lib.SamplerStep(None, 1, 0, k["a_skip"], k["a_out"], k["p"], k["q"], k["a_in_next"], k["clamp"], k["guidance"], k["guidance_rescale"])
        lib.check(L.sdxl_op_sampler_step(P(ar, "x"), P(ar, "pred"), P(ar, "x_in"), B, H, W, C.byref(s), st()))
    runs = run(fn, specs)
    assert_isolated(runs, what="sampler step")
    got_x, got_in = runs[0]["x"].cpu().view(B, 4, H, W), runs[0]["x_in"].cpu()
    want, _ = SR.full_step(x.double(), fc.double(), fu.double(), k)
    for b in range(B):
        err, top = float((got_x[b].double() - want[b]).abs().max()), float(want[b].abs().max())
        print(f"[isolation] sampler step sample {b}: max |dx| {err:.3e} = {err / top:.3e} of max |x_next| {top:.3e}")
        assert err <= 1e-5 * top
    rows = B * H * W
    assert same_bits(got_in[:rows, :4].contiguous(), _nhwc8(got_x * 0.5)[:, :4].to(BF).contiguous())
    assert float(got_in[:, 4:].float().abs().max()) == 0.0 and same_bits(got_in[rows:], got_in[:rows])


@pytest.mark.parametrize("method", [0, 1])
def test_loss_phases(L, method):
    """sdxl_op_loss phases 0-2 at (3, 6, 10), against oracle/loss_ref.py at the bars of test_loss_kernels_vs_oracle"""
    from oracle import loss_ref as R
    B, H, W = 3, 6, 10
    g = torch.Generator().manual_seed(70 + method)
    lat, noise, pred = torch.randn(B, 4, H, W, generator=g), torch.randn(B, 4, H, W, generator=g), rnd(B, 4, H, W, seed=71)
    tag = torch.tensor([0.5, 1.0, 2.0])
    ts = torch.tensor([100, 500, 850])
    sig = R.karras_sigmas()[ts] if method == 0 else torch.sigmoid(torch.randn(B, generator=g))
    specs = [I("lat", lat.reshape(B * 4, H * W), dtype=F32), I("noise", noise.reshape(B * 4, H * W), dtype=F32), I("sig", sig, dtype=F32), I("tag", tag, dtype=F32),
             I("pred", _nhwc8(pred)), O("unet_in", B * H * W, 8), O("dpred", B * H * W, 8), I("out8", torch.zeros(8), dtype=F32, role="inout")]

    def fn(ar):
        lc = lib.LossConfig(method, 1, 1, 5.0, 1)
        b = lib.Batch(B, H, W, 77, ar.ptr("lat"), ar.ptr("noise"), ar.ptr("sig"), None, None, None, None, ar.ptr("tag"))
        lib.check(L.sdxl_op_loss(C.byref(lc), C.byref(b), P(ar, "unet_in"), None, None, 1.0, None, 0, st()))
        lib.check(L.sdxl_op_loss(C.byref(lc), C.byref(b), None, P(ar, "pred"), None, 1.0, P(ar, "out8"), 1, st()))
        lib.check(L.sdxl_op_loss(C.byref(lc), C.byref(b), None, P(ar, "pred"), P(ar, "dpred"), 0.25, P(ar, "out8"), 2, st()))
        torch.cuda.synchronize()      # lc / b are host structs of this frame
    runs = run(fn, specs)
    assert_isolated(runs, what=f"loss method {method}")
    from_nhwc8 = lambda t: t.float().cpu().view(B, H * W, 8)[..., :4].permute(0, 2, 1).reshape(B, 4, H, W)
    report("loss prepare", from_nhwc8(runs[0]["unet_in"]), R.add_noise(lat, noise, sig) if method == 0 else R.optimal_transport_path(noise, lat, sig), 5e-3)
    for fill, r in zip((0x00, 0xFF, 0x7F), runs):      # channels 4..7 of the input image are written, as zeros, whatever they held before
        assert float(r["unet_in"].float()[:, 4:].abs().max()) == 0.0, f"fill 0x{fill:02X}: unet_in channels 4..7"
    pr = pred.clone().requires_grad_(True)
    ref_loss = R.ddpm_loss(pr, lat, noise, ts, "v_prediction", 5.0, tag) if method == 0 else R.flow_matching_loss(pr, noise, lat, tag)
    got = float(runs[0]["out8"][0, 0])
    print(f"[isolation] loss method {method}: {got} oracle {float(ref_loss.detach())}")
    assert abs(got - float(ref_loss)) <= 1e-5 * abs(float(ref_loss)) + 1e-7
    abs_sum, abs_ref = float(runs[0]["out8"][0, 2]), float(pr.detach().abs().sum())      # (phase 2 reads out8 and writes none of it)
    print(f"[isolation] loss method {method}: sum |pred| {abs_sum} oracle {abs_ref}")
    assert abs(abs_sum - abs_ref) <= 1e-4 * abs_ref
    ref_loss.backward()
    if float(ref_loss) >= 1000.0:
        assert float(runs[0]["dpred"].float().abs().max()) == 0.0
    else:
        report("loss dpred", from_nhwc8(runs[0]["dpred"]), pr.grad * 0.25, 8e-3)


# ------------------------------------------------------------------------------------------------------------------ optimizer slice
N_ARENA, N_SLICE = 8 * 777, 8 * 259
LO = 8 * 259                       # the middle slice [LO, LO + N_SLICE) of the arenas


def _optim_specs(with_ema):
    g = torch.Generator().manual_seed(90)
    r = lambda s: torch.randn(1, N_ARENA, generator=g) * s
    specs = [I("p", r(0.05), role="inout"), I("m", r(3e-4), role="inout"), I("v", r(1e-3).abs() * 1e-3, role="inout"), I("shift", r(1e-5), role="inout"),
             I("grad", r(4e-3), dtype=F32)]
    return specs + ([I("ema", r(0.05), dtype=F32, role="inout")] if with_ema else [])


@pytest.mark.parametrize("with_ema", [False, True], ids=["plain", "ema"])
@pytest.mark.parametrize("algorithm", [0, 1])
def test_optimizer_updates_its_slice_and_nothing_else(L, algorithm, with_ema):
    """sdxl_adamw_bf16_step on the middle n = 8 * 259 elements of p / m / v / shift / grad / ema arenas: the neighbours keep their bits, and the
    slice has the bits of the same update done as part of a full-arena call with the same elem_offset (sdxlstep.h: "any 16-byte aligned slice")."""
    def step(ar, lo, n):
        cfg = lib.AdamWConfig()
        lib.check(L.sdxl_adamw_default_config(C.byref(cfg)))
        cfg.step, cfg.seed, cfg.elem_offset, cfg.decay_this_iteration = 3.0, 0x0123456789ABCDEF, 8 * 4096 + lo, 0.006
        cfg.algorithm, cfg.kahan_sum, cfg.sf_reference, cfg.weight_decay, cfg.sf_step_size = algorithm, 1, 0, 0.01, 1.25e-4
        if with_ema:
            cfg.ema, cfg.ema_one_minus_decay = ar.ptr("ema", lo), 0.25
        lib.check(L.sdxl_adamw_bf16_step(P(ar, "p", lo), P(ar, "grad", lo), 0, P(ar, "m", lo), P(ar, "v", lo), P(ar, "shift", lo), n, C.byref(cfg), None, None, st()))
    specs = _optim_specs(with_ema)
    names = [s.name for s in specs if s.role == "inout"]
    runs = run(lambda ar: step(ar, LO, N_SLICE), specs)
    assert_isolated(runs, what=f"optimizer algorithm {algorithm} slice")
    full = run(lambda ar: step(ar, 0, N_ARENA), specs, fills=(0x00,))[0]
    before = {s.name: d(s.init).to(s.dtype) for s in specs}
    for n in names:
        got = runs[0][n][0]
        assert same_bits(got[:LO], before[n][0, :LO]) and same_bits(got[LO + N_SLICE:], before[n][0, LO + N_SLICE:]), f"{n}: a neighbour of the slice changed"
        assert same_bits(got[LO:LO + N_SLICE], full[n][0, LO:LO + N_SLICE]), f"{n}: the slice differs from the full-arena update"
    assert not same_bits(runs[0]["m"][0, LO:LO + N_SLICE], before["m"][0, LO:LO + N_SLICE]), "the update did nothing"


def test_optimizer_decay_updates_its_slice_and_nothing_else(L):
    p, _m, _v, shift = _optim_specs(False)[:4]
    p.role = "in"                                                   # sdxl_adamw_decay reads p, writes shift

    def fn(ar):
        lib.check(L.sdxl_adamw_decay(P(ar, "shift", LO), P(ar, "p", LO), N_SLICE, 0.0078125, st()))
    runs = run(fn, [p, shift])
    assert_isolated(runs, what="adamw decay slice")
    before = d(shift.init).to(BF)[0]
    got = runs[0]["shift"][0]
    assert same_bits(got[:LO], before[:LO]) and same_bits(got[LO + N_SLICE:], before[LO + N_SLICE:]), "a neighbour of the slice changed"
    assert not same_bits(got[LO:LO + N_SLICE], before[LO:LO + N_SLICE])


# ------------------------------------------------------------------------------------------------------------------ gradient-norm pieces
@pytest.mark.parametrize("dtype", [0, 1], ids=["fp32", "bf16"])
def test_sumsq_stops_at_its_last_element(L, dtype):
    """n = 8 * 1000 + 3 (the scalar tail); the pattern sits directly behind the last element (the operand's own row ends there)"""
    n = 8 * 1000 + 3
    x = rnd(n, seed=95)
    specs = [I("x", x, dtype=F32 if dtype == 0 else BF), O("out", 1, 1, dtype=F32)]

    def fn(ar):
        lib.check(L.sdxl_sumsq(P(ar, "x"), dtype, n, P(ar, "out"), st()))
    runs = run(fn, specs)
    assert_isolated(runs, what=f"sumsq dtype {dtype}")
    ref = float((x.double() ** 2).sum())
    assert abs(float(runs[0]["out"][0, 0]) - ref) <= 2e-5 * ref          # the bar of tests/test_gpu_adamw.py


def test_grads_to_bf16_on_a_sub_range(L):
    """sdxl_grads_to_bf16 reads the handle's gradient arena; its destination is the caller's: an odd element count into a guarded buffer"""
    from oracle import unet_ref as U
    from sdxl_amd import unet as NU
    from test_gpu_model import tiny_native_cfg
    net = NU.NativeUNet(tiny_native_cfg(U.tiny_config()))
    try:
        g = torch.Generator(device=DEV).manual_seed(3)
        net.grads.copy_(torch.randn(net.grads.numel(), generator=g, device=DEV))
        off, n = 8 * 1001, 8 * 1000 + 3
        torch.cuda.synchronize()

        def fn(ar):
            lib.check(L.sdxl_grads_to_bf16(net.h, off, n, P(ar, "dst"), 0.5, st()))
        runs = run(fn, [O("dst", 1, n)])
        assert_isolated(runs, what="grads_to_bf16")
        assert same_bits(runs[0]["dst"][0], (net.grads[off:off + n] * 0.5).to(BF))
    finally:
        net.close()
