"""Exact-arithmetic and per-element parity of the GEMM and convolution kernels on a real MI355X (tests/_exact.py; the method is shown to
see what it claims on the CPU in tests/test_host_exact.py).  tests/test_gpu_ops.py asserts one number per tensor, max|err| <= tol max|ref|
against an fp32 product on the GPU; here every case

  * prints the route it reaches (sdxl_debug_gemm_route: the library's own answer),
  * runs INTEGER operands ({-2 .. 2}, bias {-8 .. 8}, even residual in +-[256, 510]) and asserts bit equality with the exact result
    (bf16 outputs: ONE round-to-nearest-even of the exact integer; fp32 outputs: the integer), whatever the tile, split or partition,
  * runs randn operands at the same shape and asserts, for EVERY element, the a-priori bound against float64 on the CPU:
        |err| <= u |ref| + K 2^-23 (|A| . |B| + |bias| + |resid|),   u = 2^-8 (bf16) | 2^-24 (fp32).

Ops that round twice BY DESIGN restate their sequence in the expectation (still bit equality) and carry one more derived term in the bound:
  * sdxl_op_conv3x3_s2_dgrad WITH an addend: the NN product is stored as bf16 phase planes, the pixel shuffle then adds the addend and
    rounds again: bf16(bf16(acc) + addend)  (launch_conv3x3_s2_dgrad, pixel_shuffle2_kernel);
  * sdxl_op_upconv3x3_fwd / _dgrad: the nine taps are folded onto 16 (phase, stencil) weights stored in bf16 (upconv_fold_weights_kernel:
    fp32 sum of up to four taps, one rounding).  Integer taps fold exactly (|sum| <= 8); on randn data each folded weight carries one
    bf16 rounding of at most 2^-8 of the sum of its taps' magnitudes, so the result is off by at most 2^-8 |x| . |w| more: that term
    joins the bound.  The product itself, bias / addend included, rounds once.
  * sdxl_op_attention_bwd: the probabilities enter the matrix pipe as bf16 (pack8 in attn_bwd_dkv_body): in the uniform-softmax case
    every P is bf16(1 / Nk), and dV is restated as bf16(1 / Nk) x the column sums of dO.
Shapes: each family's smallest of tests/test_gpu_ops.py that still reaches the route, and a ragged one."""
import ctypes as C
import math

import pytest
import torch

import sdxl_amd  # noqa: F401
from sdxl_amd import lib

import _exact as X

pytestmark = pytest.mark.gpu
BF, F32 = torch.bfloat16, torch.float32
SENTINEL = 7777.0      # what outputs hold before a launch that must overwrite them


@pytest.fixture(scope="module")
def L():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return lib.load()


def dev():
    return torch.device("cuda:0")


def D(t, dtype=BF):
    """a CPU float32 tensor of bf16-exact values -> the device, in the dtype the kernel reads"""
    return t.to(dtype).to(dev()).contiguous()


def ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def out_like(*shape, dtype=BF):
    return torch.full(shape, SENTINEL, dtype=dtype, device=dev())


_CACHE = {}


def operands(form, M, N, K, integer):
    """(CPU operands, float64 references) of one shape: computed once, shared by every case that runs the shape, never modified"""
    key = (form, M, N, K, integer)
    if key not in _CACHE:
        o = X.gemm_operands(form, M, N, K, integer)
        if form == 2:
            r = dict(full=X.gemm_ref64(2, o), db=(o["a"].double().sum(0), o["a"].double().abs().sum(0)))
        else:
            r = dict(full=X.gemm_ref64(form, o, bias=form == 0), plain=X.gemm_ref64(form, o, bias=False, resid=False))
        _CACHE[key] = (o, r)
    return _CACHE[key]


def check(tag, got, ref_ab, K, integer, out_bf16):
    """integer: bit equality with the exact value; randn: the per-element bound"""
    ref, ab = ref_ab
    if integer:
        X.assert_exact(tag, got, X.expect(ref, out_bf16))
    else:
        X.check_bound(tag, got, ref, X.bound(ref, ab, K, out_bf16))


def gemm_case(L, c, what=("int", "randn")):
    """one row of the case table (tests/_exact.py) through sdxl_op_gemm under its gemm mode"""
    tag = f"{c.family} form {c.form} {c.M}x{c.N}x{c.K} splitk {c.splitk}"
    print(f"[route] {tag}: {X.case_route(lib, L, c)}")
    M, N, K = c.M, c.N, c.K
    lib.check(L.sdxl_set_gemm_mode(c.mode))
    try:
        for integer in [w == "int" for w in what]:
            o, r = operands(c.form, M, N, K, integer)
            t = f"{tag} {'int' if integer else 'randn'}"
            if c.form == 0:      # NT: bias + residual, one rounding
                a, w, bias, res = D(o["a"]), D(o["w"]), D(o["bias"]), D(o["resid"])
                out = out_like(M, N)
                lib.check(L.sdxl_op_gemm(0, ptr(a), ptr(w), ptr(out), M, N, K, ptr(bias), ptr(res), 0, c.splitk, stream()))
                check(f"{t} nt", out, r["full"], K, integer, True)
            elif c.form == 1:      # NN: plain, and accumulate = 1 onto a bf16 base (the even residual)
                a, w = D(o["a"]), D(o["w"])
                out = out_like(M, N)
                lib.check(L.sdxl_op_gemm(1, ptr(a), ptr(w), ptr(out), M, N, K, None, None, 0, c.splitk, stream()))
                check(f"{t} nn", out, r["plain"], K, integer, True)
                out2 = D(o["resid"])
                lib.check(L.sdxl_op_gemm(1, ptr(a), ptr(w), ptr(out2), M, N, K, None, None, 1, c.splitk, stream()))
                check(f"{t} nn+=", out2, r["full"], K, integer, True)
            else:      # TN: fp32, overwrite and += onto an fp32 base, bias gradient = column sums
                a, b = D(o["a"]), D(o["b"])
                out = out_like(M, N, dtype=F32)
                db = torch.zeros(M, dtype=F32, device=dev())
                lib.check(L.sdxl_op_gemm(2, ptr(a), ptr(b), ptr(out), M, N, K, ptr(db) if c.bias_grad else None, None, 0, c.splitk, stream()))
                check(f"{t} tn =", out, r["full"], K, integer, False)
                if c.bias_grad:
                    check(f"{t} tn bias grad", db, r["db"], K, integer, False)
                base = o["base"].double()
                out2 = D(o["base"], F32)
                lib.check(L.sdxl_op_gemm(2, ptr(a), ptr(b), ptr(out2), M, N, K, None, None, 1, c.splitk, stream()))
                check(f"{t} tn +=", out2, (r["full"][0] + base, r["full"][1] + base.abs()), K, integer, False)
        torch.cuda.synchronize()
    finally:
        lib.check(L.sdxl_set_gemm_mode(1))


def _ids(cases):
    return [f"{c.family.replace(' ', '_')}-f{c.form}-{c.M}x{c.N}x{c.K}-s{c.splitk}" for c in cases]


def _fam(*prefixes, diag=False):
    return [c for c in X.gemm_cases() if c.family.startswith(prefixes) and c.diag == diag]


# ------------------------------------------------------------------------------------------------ sdxl_op_gemm, default policy and forced routes
_DEFAULT = _fam("nt default", "nn default", "bf16 split-K", "tn wgrad", "tn long reduction")


@pytest.mark.parametrize("c", _DEFAULT, ids=_ids(_DEFAULT))
def test_gemm_default_policy(L, c):
    """forms 0 / 1 / 2 under the policy: bias + residual and accumulate with a single rounding (ties in the integer data), bf16 split-K
    bit-equal to the exact value and therefore to the unsplit launch, weight gradients as overwrite and += with exact bias-gradient
    column sums, the long-reduction route with the plan's split and forced ones"""
    gemm_case(L, c)


def test_bf16_split_k_equals_the_unsplit_launch_on_integers(L):
    """said once explicitly: the split launch and the unsplit one give the same bits (both equal the exact value)"""
    for (M, N, K, sk) in X.SPLITK_BF16:
        o, _ = operands(0, M, N, K, True)
        a, w, bias, res = D(o["a"]), D(o["w"]), D(o["bias"]), D(o["resid"])
        outs = []
        for s in (sk, 1):
            out = out_like(M, N)
            lib.check(L.sdxl_op_gemm(0, ptr(a), ptr(w), ptr(out), M, N, K, ptr(bias), ptr(res), 0, s, stream()))
            outs.append(out)
        assert X.same_bits(outs[0].cpu(), outs[1].cpu()), (M, N, K, sk)


_FORCED = _fam("cr256", "gemm256", "cfg 23", "pipelined", "tn short reduction forced")


@pytest.mark.parametrize("c", _FORCED, ids=_ids(_FORCED))
def test_gemm_forced_routes(L, c):
    """the co-resident 256-row kernel (modes 31, 32, 35, 36; NT, NN, TN + bias gradient), the 256 x 256 kernel (NT, NN, TN), the split-K
    wave groups (configuration 23) and the pipelined loops (7, 8, 5, 6), each forced through sdxl_set_gemm_mode"""
    gemm_case(L, c)


_FORCED_DIAG = _fam("cr256", diag=True)


@pytest.mark.diag
@pytest.mark.parametrize("c", _FORCED_DIAG, ids=_ids(_FORCED_DIAG))
def test_gemm_forced_routes_of_the_diagnostics_build(L, c):
    """modes 33 / 34: the exclusive 6-deep-ring form of the co-resident kernel"""
    gemm_case(L, c)


@pytest.mark.parametrize("n,Mo,No,rows", X.WGRAD_GROUP)
def test_wgrad_group(L, n, Mo, No, rows):
    """sdxl_op_wgrad_group: n problems in one grid, a NULL entry in dbias (problem 1), overwrite and += onto integer bases"""
    print(f"[route] wgrad group {n} x {Mo}x{No}x{rows}: {X.route_of(lib, L, 1, form=2, M=Mo, N=No, K=rows, group=n, bias_grad=1)}")
    arr = lambda ts: (C.c_void_p * n)(*[None if t is None else t.data_ptr() for t in ts])
    for integer in (True, False):
        ops = [X.gemm_operands(2, Mo, No, rows, integer, seed=20 + i) for i in range(n)]
        dys, xs = [D(o["a"]) for o in ops], [D(o["b"]) for o in ops]
        dws = [out_like(Mo, No, dtype=F32) for _ in range(n)]
        dbs = [torch.zeros(Mo, dtype=F32, device=dev()) if i != 1 else None for i in range(n)]
        lib.check(L.sdxl_op_wgrad_group(n, arr(dys), arr(xs), arr(dws), arr(dbs), Mo, No, rows, 0, stream()))
        refs = [X.gemm_ref64(2, o) for o in ops]
        t = f"wgrad group {n} x {Mo}x{No}x{rows} {'int' if integer else 'randn'}"
        for i, o in enumerate(ops):
            check(f"{t} [{i}] =", dws[i], refs[i], rows, integer, False)
            if dbs[i] is not None:
                check(f"{t} [{i}] bias grad", dbs[i], (o["a"].double().sum(0), o["a"].double().abs().sum(0)), rows, integer, False)
        bases = [D(o["base"], F32) for o in ops]
        lib.check(L.sdxl_op_wgrad_group(n, arr(dys), arr(xs), arr(bases), None, Mo, No, rows, 1, stream()))
        for i, o in enumerate(ops):
            b = o["base"].double()
            check(f"{t} [{i}] +=", bases[i], (refs[i][0] + b, refs[i][1] + b.abs()), rows, integer, False)


# ------------------------------------------------------------------------------------------------ stream-K (diagnostics build)
def _sk_launch(L, form, a, b, out, bias, resid, accumulate, workers):
    I, V = C.c_int * 1, C.c_void_p * 1
    p = lambda t: t.data_ptr() if t is not None else None
    M, N, K = (a.shape[0], b.shape[0], a.shape[1]) if form == 0 else ((a.shape[0], b.shape[1], a.shape[1]) if form == 1 else (a.shape[1], b.shape[1], a.shape[0]))
    lib.check(L.sdxl_set_sk_mode(0, workers))
    try:
        lib.check(L.sdxl_op_gemm_sk(1, I(form), V(p(a)), V(p(b)), V(p(out)), I(M), I(N), I(K), V(p(bias)), V(p(resid)), I(int(accumulate)), stream()))
    finally:
        lib.check(L.sdxl_set_sk_mode(0, 0))
    torch.cuda.synchronize()
    e = C.c_uint(0)
    lib.check(L.sdxl_sk_error(stream(), C.byref(e)))
    assert e.value == 0, f"stream-K hand-off gave up waiting (error word {e.value})"


@pytest.mark.diag
@pytest.mark.parametrize("workers", X.STREAM_K_WORKERS)
def test_gemm_stream_k_is_exact_on_integers(L, workers):
    """gemm_sk.hip: partitions that cut tiles into pieces whose partial sums are added in worker order: on integers every partition gives the
    exact value.  The three problems of tests/test_gpu_ops.py's stream-K test: NT + bias + residual, NN += , TN + bias gradient."""
    for (form, M, N, K) in X.STREAM_K_PROBLEMS:
        o, r = operands(form, M, N, K, True)
        t = f"stream-K w={workers} form {form} {M}x{N}x{K}"
        print(f"[route] {t}: sdxl_op_gemm_sk (kernel 6 directly)")
        if form == 0:
            out = out_like(M, N)
            _sk_launch(L, 0, D(o["a"]), D(o["w"]), out, D(o["bias"]), D(o["resid"]), 0, workers)
            check(t, out, r["full"], K, True, True)
        elif form == 1:
            out = D(o["resid"])
            _sk_launch(L, 1, D(o["a"]), D(o["w"]), out, None, None, 1, workers)
            check(t, out, r["full"], K, True, True)
        else:
            out = out_like(M, N, dtype=F32)
            db = torch.zeros(M, dtype=F32, device=dev())
            _sk_launch(L, 2, D(o["a"]), D(o["b"]), out, db, None, 0, workers)
            check(t, out, r["full"], K, True, False)
            check(f"{t} bias grad", db, r["db"], K, True, False)


# ------------------------------------------------------------------------------------------------ 3x3 convolutions
def conv_data(integer, B, H, W, Cin, Cout, Ho, Wo, seed):
    s = 100 * seed
    if integer:
        return dict(x=X.ints(B, H, W, Cin, seed=s + 10), w=X.ints(Cout, 9, Cin, seed=s + 11), bias=X.bias_ints(Cout, s + 12), dy=X.ints(B, Ho, Wo, Cout, seed=s + 13),
                    addend=X.resid_even(B, H, W, Cin, seed=s + 14))
    return dict(x=X.rnd(B, H, W, Cin, seed=s + 10), w=X.rnd(Cout, 9, Cin, seed=s + 11, scale=(9 * Cin) ** -0.5), bias=X.rnd(Cout, seed=s + 12),
                dy=X.rnd(B, Ho, Wo, Cout, seed=s + 13), addend=X.rnd(B, H, W, Cin, seed=s + 14))


@pytest.mark.parametrize("B,H,W,Cin,Cout,stride", [(1, 8, 8, 64, 64, 1), (2, 16, 12, 320, 640, 1), (2, 16, 16, 64, 128, 2)])
def test_conv3x3_fwd_dgrad_wgrad(L, B, H, W, Cin, Cout, stride):
    """forward (+ bias), input gradient, weight gradient (+= onto an integer base, split 1 and 3) against conv2d and its transposes in float64.
    Zero padding makes border outputs sum fewer taps: the all-ones run counts them (y = Cin x the number of taps inside the image)."""
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    for kind in ("fwd", "dgrad"):
        sk = X.conv_fwd_dgrad_splitk(kind, B, H, W, Cin, Cout, stride)
        print(f"[route] conv {kind} {B}x{H}x{W} {Cin}->{Cout} s{stride}: {X.route_of(lib, L, 1, **X.conv_desc(kind, B, H, W, Cin, Cout, stride, sk))}")
    for sk in (1, 3):
        print(f"[route] conv wgrad splitk {sk}: {X.route_of(lib, L, 1, **X.conv_desc('wgrad', B, H, W, Cin, Cout, stride, sk))}")
    tag = f"conv {B}x{H}x{W} {Cin}->{Cout} s{stride}"
    # the border count
    ones_x, ones_w = torch.ones(B, H, W, Cin), torch.ones(Cout, 9, Cin)
    y = out_like(B, Ho, Wo, Cout)
    x1, w1, b0 = D(ones_x), D(ones_w), D(torch.zeros(Cout))      # (named: they must outlive the launch)
    lib.check(L.sdxl_op_conv3x3_fwd(ptr(x1), ptr(w1), ptr(b0), ptr(y), B, H, W, Cin, Cout, stride, stream()))
    cnt = X.conv_ref64(ones_x, ones_w, None, stride)
    assert float(cnt.min()) == 4 * Cin and float(cnt.max()) == 9 * Cin      # corners see 4 taps, the interior 9
    X.assert_exact(f"{tag} tap count", y, X.expect(cnt, True))
    for integer in (True, False):
        d = conv_data(integer, B, H, W, Cin, Cout, Ho, Wo, 1)
        t = f"{tag} {'int' if integer else 'randn'}"
        a = {k: v.abs() for k, v in d.items()}
        x, w, bias, dy = D(d["x"]), D(d["w"]), D(d["bias"]), D(d["dy"])
        y = out_like(B, Ho, Wo, Cout)
        lib.check(L.sdxl_op_conv3x3_fwd(ptr(x), ptr(w), ptr(bias), ptr(y), B, H, W, Cin, Cout, stride, stream()))
        check(f"{t} fwd", y, (X.conv_ref64(d["x"], d["w"], d["bias"], stride), X.conv_ref64(a["x"], a["w"], a["bias"], stride)), 9 * Cin, integer, True)
        dx = out_like(B, H, W, Cin)
        lib.check(L.sdxl_op_conv3x3_dgrad(ptr(dy), ptr(w), ptr(dx), B, H, W, Cin, Cout, stride, stream()))
        check(f"{t} dgrad", dx, (X.conv_dgrad_ref64(d["dy"], d["w"], H, W, stride), X.conv_dgrad_ref64(a["dy"], a["w"], H, W, stride)), 9 * Cout, integer, True)
        ref, ab = X.conv_wgrad_ref64(d["x"], d["dy"], stride), X.conv_wgrad_ref64(a["x"], a["dy"], stride)
        base = X.ints(Cout, 9, Cin, seed=77, lo=-1000, hi=1000) if integer else torch.randn(Cout, 9, Cin, generator=X.gen(77))
        for splitk in (1, 3):
            dw = D(base, F32)
            lib.check(L.sdxl_op_conv3x3_wgrad(ptr(x), ptr(dy), ptr(dw), B, H, W, Cin, Cout, stride, splitk, stream()))
            check(f"{t} wgrad splitk {splitk} +=", dw, (ref + base.double(), ab + base.double().abs()), B * Ho * Wo, integer, False)


@pytest.mark.parametrize("B,H,W,Cin,Cout", [(1, 16, 16, 64, 64), (3, 12, 20, 72, 64)])
def test_conv3x3_stride2_dgrad_by_output_phase(L, B, H, W, Cin, Cout):
    """sdxl_op_conv3x3_s2_dgrad: the NN product over the four phase planes is STORED in bf16 (`planar`), the pixel shuffle copies it into dx.
    Without an addend that is one rounding.  With an addend the shuffle adds it in fp32 and rounds again -- two roundings by design:
    bf16(bf16(acc) + addend); the integer expectation restates exactly that, and the bound carries the first rounding as 2^-8 |acc|."""
    Hl, Wl = H // 2, W // 2
    up = dict(form=1, taps=4, M=4 * ((B * Hl * Wl + 127) // 128 * 128), N=Cin, K=Cout, Hm=Hl, Wm=Wl, Hs=Hl, Ws=Wl, up2=2)
    print(f"[route] conv s2 dgrad {B}x{H}x{W} {Cin}->{Cout}: {X.route_of(lib, L, 1, **up)}")
    planar = torch.empty(up["M"], Cin, dtype=BF, device=dev())
    for integer in (True, False):
        d = conv_data(integer, B, H, W, Cin, Cout, Hl, Wl, 2)
        a = {k: v.abs() for k, v in d.items()}
        acc, ab = X.conv_dgrad_ref64(d["dy"], d["w"], H, W, 2), X.conv_dgrad_ref64(a["dy"], a["w"], H, W, 2)
        dy, w = D(d["dy"]), D(d["w"])
        for addend in (None, d["addend"]):
            t = f"conv s2 dgrad {B}x{H}x{W} {Cin}->{Cout} {'int' if integer else 'randn'} addend {addend is not None}"
            dx = out_like(B, H, W, Cin)
            ad = D(addend) if addend is not None else None
            lib.check(L.sdxl_op_conv3x3_s2_dgrad(ptr(dy), ptr(w), ptr(planar), ptr(dx), ptr(ad), B, H, W, Cin, Cout, stream()))
            if addend is None:
                check(t, dx, (acc, ab), 4 * Cout, integer, True)
            elif integer:
                first = X.bf16_rn(acc).double()                     # the phase planes as stored
                X.assert_has_ties(first + addend.double(), t)
                X.assert_exact(t, dx, X.bf16_rn(first + addend.double()))
            else:
                ref = acc + addend.double()
                X.check_bound(t, dx, ref, X.bound(ref, ab + addend.double().abs(), 4 * Cout, True, extra=2.0 ** -8 * acc.abs()))


@pytest.mark.parametrize("B,H,W,Cin,Cout", [(1, 16, 16, 128, 64), (2, 24, 42, 64, 192), (4, 24, 42, 128, 64)])
def test_upsample_conv3x3(L, B, H, W, Cin, Cout):
    """sdxl_op_upconv3x3_fwd / _dgrad / _wgrad against conv2d(nearest-2x(x)) in float64.  The folded weights are bf16 (module docstring):
    exact on integer taps, 2^-8 |x| . |w| more in the randn bound.  fwd: bias, one rounding of the product (the shuffle copies).  dgrad:
    the shuffle copies dy, the product adds the addend in its epilogue: one rounding, ties from the even addend.  wgrad (whole 64-pixel
    reduction steps only, as in tests/test_gpu_ops.py): 16 fp32 (phase, stencil) products folded back onto the nine taps in fp32, = and
    += with split 1 and 3, bias gradient."""
    plane = (B * H * W + 127) // 128 * 128
    print(f"[route] upconv fwd {B}x{H}x{W} {Cin}->{Cout}: "
          f"{X.route_of(lib, L, 1, form=0, taps=4, M=4 * plane, N=Cout, K=Cin, Hm=H, Wm=W, Hs=H, Ws=W, up2=1, splitk=X.small_splitk(4 * plane, Cout, 4 * Cin, True))}")
    print(f"[route] upconv dgrad: {X.route_of(lib, L, 1, form=1, taps=16, M=B * H * W, N=Cin, K=Cout, Hm=H, Wm=W, Hs=H, Ws=W, up2=1, splitk=X.small_splitk(B * H * W, Cin, 16 * Cout, True))}")
    weff = torch.empty(Cout, 16, Cin, dtype=BF, device=dev())
    planar = torch.empty(4 * plane, Cout, dtype=BF, device=dev())
    for integer in (True, False):
        d = conv_data(integer, B, H, W, Cin, Cout, 2 * H, 2 * W, 3)
        a = {k: v.abs() for k, v in d.items()}
        t = f"upconv {B}x{H}x{W} {Cin}->{Cout} {'int' if integer else 'randn'}"
        x, w, bias, dy, addend = D(d["x"]), D(d["w"]), D(d["bias"]), D(d["dy"]), D(d["addend"])
        y = out_like(B, 2 * H, 2 * W, Cout)
        lib.check(L.sdxl_op_upconv3x3_fwd(ptr(x), ptr(w), ptr(bias), ptr(weff), ptr(planar), ptr(y), B, H, W, Cin, Cout, stream()))
        ref = X.conv_ref64(X.upsample2x_nhwc(d["x"]), d["w"], d["bias"], 1)
        ab_nb = X.conv_ref64(X.upsample2x_nhwc(a["x"]), a["w"], None, 1)
        if integer:
            X.assert_exact(f"{t} fwd", y, X.expect(ref, True))
        else:
            X.check_bound(f"{t} fwd", y, ref, X.bound(ref, ab_nb + a["bias"].double(), 9 * Cin, True, extra=2.0 ** -8 * ab_nb))
        dx = out_like(B, H, W, Cin)
        lib.check(L.sdxl_op_upconv3x3_dgrad(ptr(dy), ptr(weff), ptr(planar), ptr(dx), ptr(addend), B, H, W, Cin, Cout, stream()))
        acc = X.upsample2x_bwd_nhwc(X.conv_dgrad_ref64(d["dy"], d["w"], 2 * H, 2 * W, 1))
        ab = X.upsample2x_bwd_nhwc(X.conv_dgrad_ref64(a["dy"], a["w"], 2 * H, 2 * W, 1))
        ref = acc + d["addend"].double()
        if integer:
            X.assert_has_ties(ref, f"{t} dgrad")
            X.assert_exact(f"{t} dgrad", dx, X.expect(ref, True))
        else:
            X.check_bound(f"{t} dgrad", dx, ref, X.bound(ref, ab + a["addend"].double(), 36 * Cout, True, extra=2.0 ** -8 * ab))
        if (B * H * W) % 64:
            continue
        xu, xua = X.upsample2x_nhwc(d["x"]), X.upsample2x_nhwc(a["x"])
        ref, ab = X.conv_wgrad_ref64(xu, d["dy"], 1), X.conv_wgrad_ref64(xua, a["dy"], 1)
        dbr = (d["dy"].double().sum((0, 1, 2)), a["dy"].double().sum((0, 1, 2)))
        dweff = torch.empty(Cout, 16, Cin, dtype=F32, device=dev())
        base = X.ints(Cout, 9, Cin, seed=78, lo=-1000, hi=1000) if integer else torch.randn(Cout, 9, Cin, generator=X.gen(78))
        for splitk, acc_flag in ((1, 0), (3, 1)):
            dw = D(base, F32) if acc_flag else out_like(Cout, 9, Cin, dtype=F32)
            db = torch.zeros(Cout, dtype=F32, device=dev())
            lib.check(L.sdxl_op_upconv3x3_wgrad(ptr(planar), ptr(x), ptr(dweff), ptr(dw), ptr(db), acc_flag, B, H, W, Cin, Cout, splitk, stream()))
            b64 = base.double() * acc_flag
            check(f"{t} wgrad splitk {splitk} acc {acc_flag}", dw, (ref + b64, ab + b64.abs()), 4 * B * H * W, integer, False)
            check(f"{t} bias grad", db, dbr, 4 * B * H * W, integer, False)


@pytest.mark.parametrize("splitk", X.CONV_WGRAD3_SPLITK)
@pytest.mark.parametrize("B,H,W,Cin,Cout,kernel", [s + ("conv_wgrad3",) for s in X.CONV_WGRAD3] + [(1, 8, 8, 64, 64, "128-row")])
def test_conv3x3_wgrad2_and_three_taps_per_workgroup(L, B, H, W, Cin, Cout, kernel, splitk):
    """sdxl_op_conv3x3_wgrad2 (overwrite, += , bias gradient; the plan's split and forced ones): conv_wgrad3.hip at its smallest width
    (W = 64, 16 384 pixels) and the one-tap route at a small image"""
    r = X.route_of(lib, L, 1, **X.conv_desc("wgrad", B, H, W, Cin, Cout, 1, splitk, 1))
    print(f"[route] conv wgrad2 {B}x{H}x{W} {Cin}->{Cout} splitk {splitk}: {r}")
    assert r["kernel"] == kernel
    for integer in (True, False):
        d = conv_data(integer, B, H, W, Cin, Cout, H, W, 4)
        t = f"conv wgrad2 {B}x{H}x{W} {Cin}->{Cout} splitk {splitk} {'int' if integer else 'randn'}"
        ref, ab = X.conv_wgrad_ref64(d["x"], d["dy"], 1), X.conv_wgrad_ref64(d["x"].abs(), d["dy"].abs(), 1)
        x, dy = D(d["x"]), D(d["dy"])
        dw = out_like(Cout, 9, Cin, dtype=F32)
        db = torch.zeros(Cout, dtype=F32, device=dev())
        lib.check(L.sdxl_op_conv3x3_wgrad2(ptr(x), ptr(dy), ptr(dw), ptr(db), B, H, W, Cin, Cout, 1, splitk, 0, stream()))
        check(f"{t} =", dw, (ref, ab), B * H * W, integer, False)
        check(f"{t} bias grad", db, (d["dy"].double().sum((0, 1, 2)), d["dy"].double().abs().sum((0, 1, 2))), B * H * W, integer, False)
        lib.check(L.sdxl_op_conv3x3_wgrad2(ptr(x), ptr(dy), ptr(dw), None, B, H, W, Cin, Cout, 1, splitk, 1, stream()))
        if integer:
            X.assert_exact(f"{t} +=", dw, X.expect(2 * ref, False))
        else:      # onto the first launch's result: its error, and the same again
            X.check_bound(f"{t} +=", dw, 2 * ref, 2 * X.bound(ref, ab, B * H * W, False) + 2.0 ** -24 * 2 * ref.abs())


# ------------------------------------------------------------------------------------------------ GEGLU: the linear half
def geglu_pack_rows(t, C4, G):
    a, g = t[:C4], t[C4:]
    shp = t.shape[1:]
    return torch.stack([a.reshape(C4 // G, G, *shp), g.reshape(C4 // G, G, *shp)], 1).reshape(2 * C4, *shp).contiguous()


def geglu_unpack_cols(u, C4, G):
    M = u.shape[0]
    v = u.reshape(M, C4 // G, 2, G)
    return torch.cat([v[:, :, 0].reshape(M, C4), v[:, :, 1].reshape(M, C4)], 1)


@pytest.mark.parametrize("M,K,C4,G", [(64, 128, 256, 64), (100, 128, 160, 80)])
def test_ff_geglu_linear_half(L, M, K, C4, G):
    """the `u` output of sdxl_op_ff_geglu_fwd is x W1^T + b1: exact on integers after geglu_unpack_cols (g = value x GELU(gate) is not linear
    and stays with tests/test_gpu_ops.py)"""
    mode = 2 if G == 64 else 1
    print(f"[route] ff geglu fwd {M}x{K}x{C4} group {G}: {X.route_of(lib, L, mode, form=0, M=M, N=2 * C4, K=K, geglu=1, geglu_group=G)}")
    lib.check(L.sdxl_set_gemm_mode(mode))
    try:
        for integer in (True, False):
            if integer:
                x, w1, b1 = X.ints(M, K, seed=60), X.ints(2 * C4, K, seed=61), X.bias_ints(2 * C4, 62)
            else:
                x, w1, b1 = X.rnd(M, K, seed=60), X.rnd(2 * C4, K, seed=61, scale=K ** -0.5), X.rnd(2 * C4, seed=62, scale=0.1)
            u = out_like(M, 2 * C4)
            g = out_like(M, C4)
            xd, w1p, b1p = D(x), D(geglu_pack_rows(w1, C4, G)), D(geglu_pack_rows(b1, C4, G))
            lib.check(L.sdxl_op_ff_geglu_fwd(ptr(xd), ptr(w1p), ptr(b1p), ptr(u), ptr(g), M, K, C4, G, stream()))
            ref = x.double() @ w1.double().T + b1.double()
            ab = x.double().abs() @ w1.double().abs().T + b1.double().abs()
            check(f"ff geglu u {M}x{K}x{C4} group {G} {'int' if integer else 'randn'}", geglu_unpack_cols(u.cpu(), C4, G), (ref, ab), K, integer, True)
    finally:
        lib.check(L.sdxl_set_gemm_mode(1))


# ------------------------------------------------------------------------------------------------ sums and casts
@pytest.mark.parametrize("dtype", [0, 1], ids=["fp32", "bf16"])
@pytest.mark.parametrize("n", [1, 7, 8, 4097, 1000003])
def test_sumsq_is_exact_on_integers_and_owns_its_output_word(L, n, dtype):
    """squares of {-2 .. 2}: every partial sum is an integer <= 4 n < 2^24, so the two-pass reduction must give the exact sum.  The kernels
    ADD to their output (launch_sumsq_*: `out +=`), and the entry point sdxl_sumsq zeroes that word on the stream first (csrc/capi.hip):
    its contract is out = the squared norm whatever the word held -- the trainer and the LoRA clip hand it uninitialised memory.  So: the
    same exact value over a word that held 5 and over one that held NaN (a sum started from the old content would show either), and the
    neighbouring word untouched."""
    x = X.ints(n, seed=90 + n % 7)
    xd = D(x, F32 if dtype == 0 else BF)
    want = float((x.double() ** 2).sum())
    for before in (5.0, float("nan")):
        out = torch.tensor([before, 5.0], dtype=F32, device=dev())
        lib.check(L.sdxl_sumsq(ptr(xd), dtype, n, ptr(out), stream()))
        got = out.cpu()
        print(f"[exact] sumsq n={n} dtype {dtype} over {before}: got {float(got[0])}, exact {want}")
        assert float(got[0]) == want and float(got[1]) == 5.0


def test_grads_to_bf16_rounds_ties_to_even(L):
    """sdxl_grads_to_bf16 with scale 0.5 on a tiny UNet's arena of even integers 2 t, |t| in [256, 1023]: 0.5 x is exact in fp32, odd t in
    [256, 512) and t = 2 mod 4 in [512, 1024) are ties"""
    from oracle import unet_ref as U
    from sdxl_amd import unet as NU
    from test_gpu_model import tiny_native_cfg
    net = NU.NativeUNet(tiny_native_cfg(U.tiny_config()))
    try:
        n = net.grads.numel()
        g = X.gen(3)
        t = (256 + torch.randint(0, 768, (n,), generator=g)) * (torch.randint(0, 2, (n,), generator=g) * 2 - 1)
        X.assert_has_ties(t.double(), "grads_to_bf16")
        net.grads.copy_((2 * t).float().to(dev()))
        dst = out_like(n)
        lib.check(L.sdxl_grads_to_bf16(net.h, 0, n, ptr(dst), 0.5, stream()))
        X.assert_exact("grads_to_bf16 scale 0.5", dst, X.bf16_rn(t.double()))
    finally:
        net.close()


# ------------------------------------------------------------------------------------------------ attention, uniform softmax
@pytest.mark.parametrize("B,heads,Nq,Nk,self_attn", [(1, 1, 128, 64, False), (2, 2, 200, 77, False), (1, 4, 1008, 1008, True)])
def test_attention_uniform_softmax(L, B, heads, Nq, Nk, self_attn):
    """Q = 0: every score is 0, exp2(0) = 1 exactly, masked keys give 0.  V[k][d] = 1 where k % 64 == d: O[q][d] Nk must round to the number
    of keys in residue class d -- every key's V row used exactly once, in its own column, for every query, ragged tail included.
    lse = log(Nk) within 4 fp32 ulp.  Backward: dK exactly 0 (dS^T Q with Q = 0) and finite; dV[k] = (sum over q of dO) / Nk for every key,
    within 2^-8 |ref| + Nq 2^-23 sum|dO| / Nk.  One rounding that this formula leaves out is the kernel's by design: P = exp2(s - lse) is
    rounded to bf16 before dV^T = dO^T . P runs on the matrix pipe (attn_bwd_dkv_body: pack8), so every P is bf16(1 / Nk) -- exact at
    Nk = 64, + 1.04e-3 at 77, - 2.4e-4 at 1008 -- and that factor sits on every dV.  The expectation restates it: ref = bf16(1 / Nk) x
    sum of dO, the bound as above.  Against the unrestated (sum of dO) / Nk the same bound gives max err / bound 0.742, 1.011 and 0.637
    at the three shapes (measured; a CPU restatement of P = bf16(1 / Nk), fp32 sum, one rounding gives the same three figures)."""
    Cc = heads * 64
    vpat = (torch.arange(Nk)[:, None] % 64 == torch.arange(64)[None, :]).float().repeat(1, heads)      # [Nk][Cc]
    kdat = X.rnd(B, Nk, Cc, seed=22)
    if self_attn:
        qkv = torch.zeros(B, Nq, 3 * Cc)
        qkv[..., Cc:2 * Cc], qkv[..., 2 * Cc:] = kdat, vpat
        qkv = D(qkv)
        q, k, v = qkv[..., :Cc], qkv[..., Cc:2 * Cc], qkv[..., 2 * Cc:]
        ldq = ldk = ldv = 3 * Cc
    else:
        q = D(torch.zeros(B, Nq, Cc))
        kv = D(torch.cat([kdat, vpat.expand(B, Nk, Cc)], -1))
        k, v = kv[..., :Cc], kv[..., Cc:]
        ldq, ldk, ldv = Cc, 2 * Cc, 2 * Cc
    o = out_like(B, Nq, Cc)
    lse = out_like(B * heads, Nq, dtype=F32)
    lib.check(L.sdxl_op_attention_fwd(ptr(q), ptr(k), ptr(v), ptr(o), ptr(lse), B, heads, Nq, Nk, ldq, ldk, ldv, Cc, stream()))
    count = vpat.double().sum(0)                                     # keys per residue class: Nk // 64 or that + 1
    got = torch.round(o.cpu().double() * Nk)
    assert count.max() * 2.0 ** -8 < 0.5                              # one bf16 rounding of count / Nk cannot move the product to another integer
    bad = int((got != count.expand(B, Nq, Cc)).sum())
    print(f"[exact] attention uniform B{B} h{heads} {Nq}x{Nk}: {bad} of {got.numel()} outputs miss their key count")
    assert bad == 0
    want = torch.tensor(math.log(Nk), dtype=F32).double()              # log(Nk) as fp32 holds it
    ulp = 2.0 ** (math.floor(math.log2(float(want))) - 23)
    lerr = float((lse.cpu().double() - want).abs().max()) / ulp
    print(f"[exact] attention uniform lse: max error {lerr:.2f} fp32 ulp")
    assert lerr <= 4.0
    do = X.rnd(B, Nq, Cc, seed=23)
    dod = D(do)
    delta = torch.empty(B * heads, Nq, dtype=F32, device=dev())
    if self_attn:
        dqkv = torch.full_like(qkv, SENTINEL)
        dq, dk, dv = dqkv[..., :Cc], dqkv[..., Cc:2 * Cc], dqkv[..., 2 * Cc:]
    else:
        dq = torch.full_like(q, SENTINEL)
        dkv = torch.full_like(kv, SENTINEL)
        dk, dv = dkv[..., :Cc], dkv[..., Cc:]
    lib.check(L.sdxl_op_attention_bwd(ptr(q), ptr(k), ptr(v), ptr(o), ptr(dod), ptr(lse), ptr(delta), ptr(dq), ptr(dk), ptr(dv), B, heads, Nq, Nk,
                                      ldq, ldk, ldv, Cc, stream()))
    dkc = dk.cpu().float()
    assert bool(torch.isfinite(dkc).all()) and bool((dkc == 0).all()), "dK is not exactly 0"
    pb = float(torch.tensor(1.0 / Nk).to(BF))                         # P as the matrix pipe sees it
    assert abs((math.frexp(1.0 / Nk)[0] * 256) % 1.0 - 0.5) > 0.1      # (1 / Nk in bf16 ulps is far from a tie: an ulp of lse cannot move P to the next bf16)
    plain = (do.double().sum(1, keepdim=True) / Nk).expand(B, Nk, Cc)
    ref = (do.double().sum(1, keepdim=True) * pb).expand(B, Nk, Cc).contiguous()
    absdo = (do.double().abs().sum(1, keepdim=True) / Nk).expand(B, Nk, Cc)
    got = dv.float().cpu().double()
    print(f"[bound] attention uniform dV against (sum dO) / Nk without the bf16 P: max |err| / bound "
          f"{float(((got - plain).abs() / (2.0 ** -8 * plain.abs() + Nq * 2.0 ** -23 * absdo)).max()):.3f}")
    X.check_bound(f"attention uniform dV B{B} h{heads} {Nq}x{Nk}", dv.float(), ref, 2.0 ** -8 * ref.abs() + Nq * 2.0 ** -23 * absdo)
