"""Per-kernel parity on a real MI355X: every HIP kernel family called through the C ABI and compared with a
plain PyTorch fp32 reference of the same op on the same bf16-rounded inputs.

Tolerances (bf16 storage, fp32 accumulate): outputs are rounded to bf16 once, so per-element error is bounded by
~2^-8 of the value plus accumulation-order noise; checked as max|err| <= tol * max|ref| with tol stated per test."""
import ctypes as C
import math

import pytest
import torch

import sdxl_amd  # noqa: F401
from sdxl_amd import lib

import _bucket_cases as BK      # the default aspect buckets' geometries (tests/test_host_buckets.py pins them to the config)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def L():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return lib.load()


def dev():
    return torch.device("cuda:0")


def bf(t):
    return t.to(torch.bfloat16)


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return bf((torch.randn(*shape, generator=g) * scale)).to(dev())


def ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def knob(L, kid, value):
    """experiment knob of the DIAGNOSTICS build (sdxl_set_knob); False against the product library, which has none"""
    if not lib.DIAG:
        return False
    lib.check(L.sdxl_set_knob(kid, value))
    return True


def relerr(got, ref):
    got, ref = got.float(), ref.float()
    return float((got - ref).abs().max() / ref.abs().max().clamp_min(1e-20))


def report(name, got, ref, tol):
    e = relerr(got, ref)
    print(f"[parity] {name}: max|err|/max|ref| = {e:.3e} (tol {tol:.1e})")
    assert math.isfinite(e) and e <= tol, f"{name}: rel err {e} > {tol}"


# --------------------------------------------------------------------------------------------------------
def test_hw_layout_probe(L):
    """ds_read_b64_tr_b16 and v_mfma_f32_16x16x32_bf16 do what the kernels assume (asymmetric data)."""
    out = torch.zeros(2048, dtype=torch.float32, device=dev())
    lib.check(L.sdxl_probe_layout(ptr(out), stream()))
    torch.cuda.synchronize()
    o = out.cpu()
    # transpose read: LDS image value = element index & 255 of a [64][16] image; group g reads the 4x16 block at
    # row 4g; lane i of the group must receive column i: rows 4g..4g+3  -> value ((4g+j)*16 + i) & 255
    exp = torch.zeros(64, 4)
    for l in range(64):
        g, i = l >> 4, l & 15
        for j in range(4):
            exp[l, j] = ((4 * g + j) * 16 + i) & 255
    assert torch.equal(o[:256].view(64, 4), exp), f"tr-read layout mismatch:\n{o[:256].view(64,4)[:8]}"
    # MFMA: A = identity (16x16, k<16), B[k][j] = 16k+j  =>  C[i][j] = 16i + j ; C layout col=l&15,row=4*(l>>4)+r
    c = o[1024:1280].view(64, 4)
    for l in range(64):
        for r in range(4):
            row, col = 4 * (l >> 4) + r, l & 15
            assert c[l, r] == 16 * row + col, (l, r, float(c[l, r]))


@pytest.mark.parametrize("M,N,K", [(128, 128, 64), (256, 384, 320), (308, 1280, 2048), (4, 1280, 320),
                                   (1000, 640, 2560), (4096, 1280, 1280)] + BK.GEMM_NT)
def test_gemm_nt(L, M, N, K):
    a, w = rnd(M, K, seed=1), rnd(N, K, seed=2, scale=K ** -0.5)
    bias, res = rnd(N, seed=3), rnd(M, N, seed=4)
    out = torch.empty(M, N, dtype=torch.bfloat16, device=dev())
    lib.check(L.sdxl_op_gemm(0, ptr(a), ptr(w), ptr(out), M, N, K, ptr(bias), ptr(res), 0, 1, stream()))
    ref = a.float() @ w.float().t() + bias.float() + res.float()
    report(f"gemm_nt {M}x{N}x{K}", out, ref, 6e-3)


@pytest.mark.parametrize("M,N,K", [(128, 128, 64), (256, 320, 384), (308, 2048, 1280), (1000, 2560, 640)] + BK.GEMM_NN)
def test_gemm_nn_and_accumulate(L, M, N, K):
    a, w = rnd(M, K, seed=5), rnd(K, N, seed=6, scale=K ** -0.5)
    out = torch.empty(M, N, dtype=torch.bfloat16, device=dev())
    lib.check(L.sdxl_op_gemm(1, ptr(a), ptr(w), ptr(out), M, N, K, None, None, 0, 1, stream()))
    ref = a.float() @ w.float()
    report(f"gemm_nn {M}x{N}x{K}", out, ref, 6e-3)
    base = rnd(M, N, seed=7)
    out2 = base.clone()
    lib.check(L.sdxl_op_gemm(1, ptr(a), ptr(w), ptr(out2), M, N, K, None, None, 1, 1, stream()))
    report(f"gemm_nn+= {M}x{N}x{K}", out2, ref + base.float(), 6e-3)


@pytest.mark.parametrize("M,N,K,splitk", [(256, 1280, 10240, 16), (256, 1280, 1280, 5), (77, 640, 2048, 4), (1000, 640, 2560, 3),
                                          (256, 384, 320, 7), (128, 160, 64, 4), (4, 1280, 13760, 32), (4, 1280, 2816, 11)])
def test_gemm_nt_nn_splitk_small_problems(L, M, N, K, splitk):
    """split-K of the bf16-output forms (small-M problems: batch 1 / 512^2): fp32 partial tiles per split, fixed-order sum +
    bias / residual / accumulate epilogue; a factor beyond K / 64 is clamped, ragged M and non-160 N go through."""
    a, w = rnd(M, K, seed=1), rnd(N, K, seed=2, scale=K ** -0.5)
    bias, res = rnd(N, seed=3), rnd(M, N, seed=4)
    out = torch.empty(M, N, dtype=torch.bfloat16, device=dev())
    lib.check(L.sdxl_op_gemm(0, ptr(a), ptr(w), ptr(out), M, N, K, ptr(bias), ptr(res), 0, splitk, stream()))
    report(f"gemm_nt splitk={splitk} {M}x{N}x{K}", out, a.float() @ w.float().t() + bias.float() + res.float(), 6e-3)
    ref1 = torch.empty(M, N, dtype=torch.bfloat16, device=dev())
    lib.check(L.sdxl_op_gemm(0, ptr(a), ptr(w), ptr(ref1), M, N, K, ptr(bias), ptr(res), 0, 1, stream()))
    assert float((out.float() - ref1.float()).abs().max()) <= 2 ** -7 * float(ref1.float().abs().max())     # vs the unsplit launch: one bf16 step
    wn = rnd(K, N, seed=6, scale=K ** -0.5)
    base = rnd(M, N, seed=7)
    out2 = base.clone()
    lib.check(L.sdxl_op_gemm(1, ptr(a), ptr(wn), ptr(out2), M, N, K, None, None, 1, splitk, stream()))
    report(f"gemm_nn+= splitk={splitk} {M}x{N}x{K}", out2, a.float() @ wn.float() + base.float(), 6e-3)


@pytest.mark.parametrize("M,N,K,splitk", [(128, 128, 64, 1), (320, 384, 1000, 1), (1280, 640, 4096, 4),
                                          (8, 320, 65536, 16), (640, 640, 308, 2), (896, 1120, 2048, 3)]      # 7 x 7 tiles x 3 splits (generic XCD order)
                                         + BK.GEMM_TN)             # bucket row counts as ragged reductions, splitk 0: the plan's choice
def test_gemm_tn_wgrad(L, M, N, K, splitk):
    a, b = rnd(K, M, seed=8), rnd(K, N, seed=9)
    out = torch.zeros(M, N, dtype=torch.float32, device=dev())
    lib.check(L.sdxl_op_gemm(2, ptr(a), ptr(b), ptr(out), M, N, K, None, None, 1, splitk, stream()))
    ref = a.float().t() @ b.float()
    report(f"gemm_tn {M}x{N}x{K} splitk={splitk}", out, ref, 2e-5 * math.sqrt(K) + 1e-5)
    if splitk == 1:
        lib.check(L.sdxl_op_gemm(2, ptr(a), ptr(b), ptr(out), M, N, K, None, None, 0, 1, stream()))
        report("gemm_tn overwrite", out, ref, 2e-5 * math.sqrt(K) + 1e-5)


def _sk_launch(L, probs, workers):
    """probs: [(form, a, b, out, bias, resid, accumulate)] -> one stream-K launch (sdxl_op_gemm_sk)"""
    n = len(probs)
    I, V = C.c_int * n, C.c_void_p * n
    p = lambda t: t.data_ptr() if t is not None else None
    shape = lambda f, a, b: (a.shape[0], b.shape[0], a.shape[1]) if f == 0 else ((a.shape[0], b.shape[1], a.shape[1]) if f == 1 else (a.shape[1], b.shape[1], a.shape[0]))
    dims = [shape(q[0], q[1], q[2]) for q in probs]
    lib.check(L.sdxl_set_sk_mode(0, workers))
    try:
        lib.check(L.sdxl_op_gemm_sk(n, I(*[q[0] for q in probs]), V(*[p(q[1]) for q in probs]), V(*[p(q[2]) for q in probs]),
                                    V(*[p(q[3]) for q in probs]), I(*[d[0] for d in dims]), I(*[d[1] for d in dims]), I(*[d[2] for d in dims]),
                                    V(*[p(q[4]) for q in probs]), V(*[p(q[5]) for q in probs]), I(*[int(q[6]) for q in probs]), stream()))
    finally:
        lib.check(L.sdxl_set_sk_mode(0, 0))
    torch.cuda.synchronize()
    e = C.c_uint(0)
    lib.check(L.sdxl_sk_error(stream(), C.byref(e)))
    assert e.value == 0, f"stream-K hand-off gave up waiting (error word {e.value})"


@pytest.mark.diag
@pytest.mark.parametrize("workers", [1, 7, 37, 100, 255, 256, 0])
def test_gemm_stream_k_forms_and_partitions(L, workers):
    """Persistent stream-K kernel (gemm_sk.hip): every form, with partitions that cut tiles into two, three and many pieces
    (worker counts that do not divide the iteration count), bias / residual / accumulate epilogues, bias gradient of the TN form."""
    M, N, K = 512, 768, 640
    a, w = rnd(M, K, seed=1), rnd(N, K, seed=2, scale=K ** -0.5)
    bias, res = rnd(N, seed=3), rnd(M, N, seed=4)
    out = torch.zeros(M, N, dtype=torch.bfloat16, device=dev())
    _sk_launch(L, [(0, a, w, out, bias, res, 0)], workers)
    report(f"sk nt w={workers}", out, a.float() @ w.float().t() + bias.float() + res.float(), 6e-3)
    wn = rnd(K, N, seed=6, scale=K ** -0.5)
    out2 = res.clone()
    _sk_launch(L, [(1, a, wn, out2, None, None, 1)], workers)
    report(f"sk nn+= w={workers}", out2, a.float() @ wn.float() + res.float(), 6e-3)
    Kr = 2048
    dy, x = rnd(Kr, 512, seed=8), rnd(Kr, 256, seed=9)
    dw = torch.zeros(512, 256, dtype=torch.float32, device=dev())
    db = torch.zeros(512, dtype=torch.float32, device=dev())
    _sk_launch(L, [(2, dy, x, dw, db, None, 0)], workers)
    report(f"sk tn w={workers}", dw, dy.float().t() @ x.float(), 2e-5 * math.sqrt(Kr) + 1e-5)
    report("sk tn bias grad", db, dy.float().sum(0), 1e-4)


@pytest.mark.diag
def test_gemm_stream_k_fused_dgrad_wgrad_is_reproducible(L):
    """A layer's dgrad (NN) and wgrad (TN) in ONE launch, as the work list is meant to be used; the partition is a function of the
    shapes only, the partials are added in worker order: repeated launches give identical bits."""
    M, Cin, Cout = 1024, 1280, 2560
    dy, w, x = rnd(M, Cout, seed=11), rnd(Cout, Cin, seed=12, scale=Cout ** -0.5), rnd(M, Cin, seed=13)
    dx = torch.zeros(M, Cin, dtype=torch.bfloat16, device=dev())
    dw = torch.zeros(Cout, Cin, dtype=torch.float32, device=dev())
    db = torch.zeros(Cout, dtype=torch.float32, device=dev())
    probs = [(1, dy, w, dx, None, None, 0), (2, dy, x, dw, db, None, 0)]
    _sk_launch(L, probs, 256)
    report("sk fused dgrad", dx, dy.float() @ w.float(), 6e-3)
    report("sk fused wgrad", dw, dy.float().t() @ x.float(), 2e-5 * math.sqrt(M) + 1e-5)
    first = (dx.clone(), dw.clone())
    for _ in range(10):
        dx.fill_(3.0); dw.fill_(3.0)
        _sk_launch(L, probs, 256)
        assert torch.equal(dx, first[0]) and torch.equal(dw, first[1])


@pytest.mark.parametrize("M,N,K", [(5120, 640, 16384), (640, 2560, 16384), (1920, 640, 16384), (640, 640, 16384), (200, 72, 16384),
                                   (256, 160, 32768),
                                   (1792, 480, 16384)]       # 7 x 3 tiles: a grid no XCD rectangle divides, a short last band (xcd_seq_map)
                                  + BK.GEMM_TN_LONG)         # the bucket row counts 15 808 / 3952: below the policy's 16 384, the same contract through its other route
@pytest.mark.parametrize("splitk", [0, 1, 3])
def test_gemm_tn_long_reduction_wgrad256(L, M, N, K, splitk):
    """wgrad256.hip (linear weight gradients over >= 16 384 rows: 256 x 160 tiles, two stacked dY tiles per staged X tile): fp32 result
    against the fp32 product, bias gradient, += , the plan's split-K and forced ones, ragged tiles; and against the 128 x 160 kernel."""
    a, b = rnd(K, M, seed=8), rnd(K, N, seed=9)
    ref = a.float().t() @ b.float()
    tol = 2e-5 * math.sqrt(K) + 1e-5
    out = torch.full((M, N), 3.0, dtype=torch.float32, device=dev())
    db = torch.zeros(M, dtype=torch.float32, device=dev())
    lib.check(L.sdxl_op_gemm(2, ptr(a), ptr(b), ptr(out), M, N, K, ptr(db), None, 0, splitk, stream()))
    report(f"wgrad256 {M}x{N}x{K} splitk={splitk}", out, ref, tol)
    report("wgrad256 bias grad", db, a.float().sum(0), 1e-4)
    lib.check(L.sdxl_op_gemm(2, ptr(a), ptr(b), ptr(out), M, N, K, None, None, 1, splitk, stream()))
    report("wgrad256 +=", out, 2 * ref, tol)
    if knob(L, 9, 1):                                  # (diagnostics build: the 128 x 160 kernel on the same problem)
        try:
            o1 = torch.zeros(M, N, dtype=torch.float32, device=dev())
            lib.check(L.sdxl_op_gemm(2, ptr(a), ptr(b), ptr(o1), M, N, K, None, None, 0, 0, stream()))
        finally:
            knob(L, 9, 0)
        report("wgrad256 vs 128x160 kernel", out * 0.5, o1, tol)


@pytest.fixture(params=[31, 32, 35, 36] + ([33, 34] if lib.DIAG else []))
def cr256(L, request):
    """force the co-resident 256-row kernel (gemm_cr256.hip; 31: 256 x 160 tiles, 32: 256 x 128) wherever it is applicable
    (diagnostics build: also 33 / 34, the exclusive 6-deep-ring form of the same tiles)"""
    lib.check(L.sdxl_set_gemm_mode(4 * request.param))
    yield L
    lib.check(L.sdxl_set_gemm_mode(1))


@pytest.mark.parametrize("M,N,K", [(256, 160, 32), (256, 320, 64), (256, 128, 96), (512, 640, 160), (300, 200, 128), (1000, 640, 2560),
                                   (4096, 1280, 1280), (8, 1288, 320)])
def test_gemm_cr256_nt_nn(cr256, M, N, K):
    """256 x 160 / 256 x 128 x 32 tiles, 3-deep ring: 1, 2, 3, 4, 5 K-steps exercise the prologue / dummy-tail arithmetic, ragged M and N the
    out-of-range buffer offsets and the guarded stores; every bf16 epilogue input; result against fp32 and against the 128-row kernel."""
    L = cr256
    a, w = rnd(M, K, seed=1), rnd(N, K, seed=2, scale=K ** -0.5)
    bias, res = rnd(N, seed=3), rnd(M, N, seed=4)
    out = torch.empty(M, N, dtype=torch.bfloat16, device=dev())
    lib.check(L.sdxl_op_gemm(0, ptr(a), ptr(w), ptr(out), M, N, K, ptr(bias), ptr(res), 0, 1, stream()))
    report(f"cr256 nt {M}x{N}x{K}", out, a.float() @ w.float().t() + bias.float() + res.float(), 6e-3)
    wn = rnd(K, N, seed=6, scale=K ** -0.5)
    lib.check(L.sdxl_op_gemm(1, ptr(a), ptr(wn), ptr(out), M, N, K, None, None, 0, 1, stream()))
    ref = a.float() @ wn.float()
    report(f"cr256 nn {M}x{N}x{K}", out, ref, 6e-3)
    base = rnd(M, N, seed=7)
    out2 = base.clone()
    lib.check(L.sdxl_op_gemm(1, ptr(a), ptr(wn), ptr(out2), M, N, K, None, None, 1, 1, stream()))
    report(f"cr256 nn+= {M}x{N}x{K}", out2, ref + base.float(), 6e-3)
    lib.check(L.sdxl_set_gemm_mode(0))
    out3 = torch.empty_like(out)
    lib.check(L.sdxl_op_gemm(1, ptr(a), ptr(wn), ptr(out3), M, N, K, None, None, 0, 1, stream()))
    report("cr256 vs gemm128", out, out3.float(), 8e-3)


@pytest.mark.parametrize("M,N,K,splitk", [(256, 160, 32, 1), (256, 128, 64, 1), (512, 320, 96, 1), (1280, 1280, 4096, 3), (3840, 1280, 4096, 1),
                                          (200, 72, 1024, 4), (640, 640, 16384, 5),
                                          (1792, 896, 512, 1), (1792, 896, 1536, 3)])      # 7 x 7 tiles (x 3 splits): 49 / 147 workgroups, not a multiple of 8
def test_gemm_cr256_tn_wgrad_bias(cr256, M, N, K, splitk):
    L = cr256
    a, b = rnd(K, M, seed=8), rnd(K, N, seed=9)
    tol = 2e-5 * math.sqrt(K) + 1e-5
    out = torch.zeros(M, N, dtype=torch.float32, device=dev())
    bg = torch.zeros(M, dtype=torch.float32, device=dev())
    lib.check(L.sdxl_op_gemm(2, ptr(a), ptr(b), ptr(out), M, N, K, ptr(bg), None, 1, splitk, stream()))
    ref = a.float().t() @ b.float()
    report(f"cr256 tn {M}x{N}x{K} splitk={splitk}", out, ref, tol)
    report("cr256 tn bias grad", bg, a.float().sum(0), tol)
    lib.check(L.sdxl_op_gemm(2, ptr(a), ptr(b), ptr(out), M, N, K, None, None, 1, splitk, stream()))    # accumulate, no bias: the 160-column form
    report("cr256 tn +=", out, 2 * ref, tol)
    lib.check(L.sdxl_op_gemm(2, ptr(a), ptr(b), ptr(out), M, N, K, None, None, 0, splitk, stream()))    # overwrite
    report("cr256 tn =", out, ref, tol)


def test_gemm_cr256_grouped_wgrad_and_geglu_backward(cr256):
    test_wgrad_group(cr256, 3, 1280, 1280, 4096)
    test_wgrad_group(cr256, 2, 320, 640, 1000)      # (rows % 32 != 0: not applicable, stays on the 128-row kernel)
    test_wgrad_group(cr256, 4, 128, 160, 64)
    _ff_geglu_case(cr256, 308, 320, 1280, 64)
    _ff_geglu_case(cr256, 4096, 1280, 5120, 64)
    _ff_geglu_case(cr256, 100, 128, 160, 80)


@pytest.fixture
def g256(L):
    """force the 256 x 256 / 8-phase kernel (gemm256.hip) wherever it is applicable, restore the default policy after"""
    lib.check(L.sdxl_set_gemm_mode(2))
    yield L
    lib.check(L.sdxl_set_gemm_mode(1))


@pytest.mark.parametrize("M,N,K", [(256, 256, 64), (256, 256, 128), (512, 768, 192), (1024, 256, 1280), (4096, 3840, 1280),
                                   (1024, 18432, 128), (4096, 10240, 192)])
def test_gemm256_nt_nn(g256, M, N, K):
    """asymmetric data, every epilogue input: odd K-tile counts (1, 2, 3: the prologue / tail of the 8-phase pipeline); the last
    two shapes leave 32 / 128 tiles beyond whole rounds of 256: the NT launch computes them with half-height workgroups"""
    L = g256
    a, w = rnd(M, K, seed=1), rnd(N, K, seed=2, scale=K ** -0.5)
    bias, res = rnd(N, seed=3), rnd(M, N, seed=4)
    out = torch.empty(M, N, dtype=torch.bfloat16, device=dev())
    lib.check(L.sdxl_op_gemm(0, ptr(a), ptr(w), ptr(out), M, N, K, ptr(bias), ptr(res), 0, 1, stream()))
    report(f"gemm256 nt {M}x{N}x{K}", out, a.float() @ w.float().t() + bias.float() + res.float(), 6e-3)
    wn = rnd(K, N, seed=6, scale=K ** -0.5)
    lib.check(L.sdxl_op_gemm(1, ptr(a), ptr(wn), ptr(out), M, N, K, None, None, 0, 1, stream()))
    ref = a.float() @ wn.float()
    report(f"gemm256 nn {M}x{N}x{K}", out, ref, 6e-3)
    base = rnd(M, N, seed=7)
    out2 = base.clone()
    lib.check(L.sdxl_op_gemm(1, ptr(a), ptr(wn), ptr(out2), M, N, K, None, None, 1, 1, stream()))
    report(f"gemm256 nn+= {M}x{N}x{K}", out2, ref + base.float(), 6e-3)
    # the result must not depend on which kernel ran beyond accumulation order: compare with the 128-row kernel
    lib.check(L.sdxl_set_gemm_mode(0))
    out3 = torch.empty_like(out)
    lib.check(L.sdxl_op_gemm(1, ptr(a), ptr(wn), ptr(out3), M, N, K, None, None, 0, 1, stream()))
    lib.check(L.sdxl_set_gemm_mode(2))
    report("gemm256 vs gemm128", out, out3.float(), 8e-3)


@pytest.mark.parametrize("M,N,K,splitk", [(256, 256, 64, 1), (512, 256, 192, 1), (1280, 1280, 4096, 3), (256, 512, 1024, 4),
                                          (256, 256, 320, 5)])
def test_gemm256_tn_wgrad_bias(g256, M, N, K, splitk):
    L = g256
    a, b = rnd(K, M, seed=8), rnd(K, N, seed=9)
    out = torch.zeros(M, N, dtype=torch.float32, device=dev())
    bg = torch.zeros(M, dtype=torch.float32, device=dev())
    lib.check(L.sdxl_op_gemm(2, ptr(a), ptr(b), ptr(out), M, N, K, ptr(bg), None, 1, splitk, stream()))
    ref = a.float().t() @ b.float()
    report(f"gemm256 tn {M}x{N}x{K} splitk={splitk}", out, ref, 2e-5 * math.sqrt(K) + 1e-5)
    report("gemm256 tn bias grad", bg, a.float().sum(0), 2e-5 * math.sqrt(K) + 1e-5)
    lib.check(L.sdxl_op_gemm(2, ptr(a), ptr(b), ptr(out), M, N, K, None, None, 1, splitk, stream()))    # accumulate
    report("gemm256 tn +=", out, 2 * ref, 2e-5 * math.sqrt(K) + 1e-5)
    lib.check(L.sdxl_op_gemm(2, ptr(a), ptr(b), ptr(out), M, N, K, None, None, 0, splitk, stream()))    # overwrite
    report("gemm256 tn =", out, ref, 2e-5 * math.sqrt(K) + 1e-5)


@pytest.mark.parametrize("n,Mo,No,rows", [(3, 1280, 1280, 4096), (2, 320, 640, 1000), (4, 128, 160, 64), (1, 640, 320, 512)])
def test_wgrad_group(L, n, Mo, No, rows):
    """Grouped weight-gradient launch (GemmP::group): n problems of one shape in one grid, each with its own operands,
    fp32 destination and optional bias-gradient accumulator; overwrite and += ."""
    import ctypes as C
    dys = [rnd(rows, Mo, seed=20 + i) for i in range(n)]
    xs = [rnd(rows, No, seed=30 + i) for i in range(n)]
    dws = [torch.full((Mo, No), 7.0, dtype=torch.float32, device=dev()) for _ in range(n)]
    dbs = [torch.zeros(Mo, dtype=torch.float32, device=dev()) if i != 1 else None for i in range(n)]
    arr = lambda ts: (C.c_void_p * n)(*[None if t is None else t.data_ptr() for t in ts])
    tol = 2e-5 * math.sqrt(rows) + 1e-5
    lib.check(L.sdxl_op_wgrad_group(n, arr(dys), arr(xs), arr(dws), arr(dbs), Mo, No, rows, 0, stream()))
    for i in range(n):
        ref = dys[i].float().t() @ xs[i].float()
        report(f"wgrad group {n}x {Mo}x{No}x{rows} [{i}] =", dws[i], ref, tol)
        if dbs[i] is not None:
            report(f"wgrad group bias grad [{i}]", dbs[i], dys[i].float().sum(0), tol)
    lib.check(L.sdxl_op_wgrad_group(n, arr(dys), arr(xs), arr(dws), None, Mo, No, rows, 1, stream()))
    for i in range(n):
        report(f"wgrad group [{i}] +=", dws[i], 2 * (dys[i].float().t() @ xs[i].float()), tol)


@pytest.mark.parametrize("M,N,K", [(128, 160, 64), (128, 160, 128), (256, 320, 192), (4096, 1280, 1280), (1000, 640, 2560), (308, 1280, 2048)])
def test_gemm_splitk_groups_nt_nn(L, M, N, K):
    """configuration 23 (8 waves = two K-groups of 2 x 2 waves, staggered by one barrier, partial tiles exchanged through
    LDS): 1, 2, 3 K-steps exercise the pipeline's prologue / dummy-tail arithmetic; ragged M exercises the row predicates."""
    lib.check(L.sdxl_set_gemm_mode(4 * 23))
    try:
        a, w = rnd(M, K, seed=1), rnd(N, K, seed=2, scale=K ** -0.5)
        bias, res = rnd(N, seed=3), rnd(M, N, seed=4)
        out = torch.empty(M, N, dtype=torch.bfloat16, device=dev())
        lib.check(L.sdxl_op_gemm(0, ptr(a), ptr(w), ptr(out), M, N, K, ptr(bias), ptr(res), 0, 1, stream()))
        report(f"gemm cfg23 nt {M}x{N}x{K}", out, a.float() @ w.float().t() + bias.float() + res.float(), 6e-3)
        wn = rnd(K, N, seed=6, scale=K ** -0.5)
        base = rnd(M, N, seed=7)
        out2 = base.clone()
        lib.check(L.sdxl_op_gemm(1, ptr(a), ptr(wn), ptr(out2), M, N, K, None, None, 1, 1, stream()))
        report(f"gemm cfg23 nn+= {M}x{N}x{K}", out2, a.float() @ wn.float() + base.float(), 6e-3)
    finally:
        lib.check(L.sdxl_set_gemm_mode(1))


@pytest.mark.parametrize("cfg", [7, 8, 5, 6])
@pytest.mark.parametrize("M,N,K", [(128, 160, 64), (128, 160, 128), (256, 320, 192), (128, 128, 256), (4096, 1280, 1280), (1000, 640, 2560),
                                   (308, 1280, 2048), (4096, 1280, 5120), (520, 264, 320), (16384, 640, 640)])
def test_gemm_pipelined_nt_nn(L, cfg, M, N, K):
    """The software-pipelined one-wave-per-SIMD kernels: configuration 7 = gemm_pl.hip (8: the same with its L2 prefetch wave, a measured experiment; the next half-step's fragments are read and the DMA
    pieces of step t + 3 issued BETWEEN the MFMAs of the current half-step; 128 x 160 tiles where N % 160 == 0, else 128 x 128; 4-deep
    ring; raw-buffer LDS-DMA with out-of-range offsets for ragged rows / columns and the tail), configurations 5 / 6 = the same loop
    structure inside gemm.hip's kernel (group-wise interleave; also takes the 3 x 3 gather).  1 ... 5 K-steps exercise the prologue and
    the zero-fill tail (the loop also READS the slot of the step after the last one), ragged M / N the row predicates; every bf16
    epilogue input; against fp32 and bit-for-bit against the lockstep kernel on the same tiles (configuration 13 / 1: the same products
    in the same order per accumulator).  A new barrier / counted-wait structure: each case also runs 20 times and must return the same
    bits every time (a reader that overtakes its DMA shows up as a run-to-run difference long before a reference check at 6e-3 does)."""
    a, w = rnd(M, K, seed=1), rnd(N, K, seed=2, scale=K ** -0.5)
    bias, res = rnd(N, seed=3), rnd(M, N, seed=4)
    wn = rnd(K, N, seed=6, scale=K ** -0.5)
    base = rnd(M, N, seed=7)

    def run(c):
        lib.check(L.sdxl_set_gemm_mode(4 * c))
        try:
            out = torch.empty(M, N, dtype=torch.bfloat16, device=dev())
            lib.check(L.sdxl_op_gemm(0, ptr(a), ptr(w), ptr(out), M, N, K, ptr(bias), ptr(res), 0, 1, stream()))
            out2 = base.clone()
            lib.check(L.sdxl_op_gemm(1, ptr(a), ptr(wn), ptr(out2), M, N, K, None, None, 1, 1, stream()))
            torch.cuda.synchronize()
            return out, out2
        finally:
            lib.check(L.sdxl_set_gemm_mode(1))

    out, out2 = run(cfg)
    report(f"gemm cfg{cfg} nt {M}x{N}x{K}", out, a.float() @ w.float().t() + bias.float() + res.float(), 6e-3)
    report(f"gemm cfg{cfg} nn+= {M}x{N}x{K}", out2, a.float() @ wn.float() + base.float(), 6e-3)
    lock = run(13 if (cfg in (5, 7, 8) and N % 160 == 0) else 1)
    if cfg in (7, 8) or (cfg == 5) == (N % 160 == 0):           # same tile width on both sides: identical summation order
        assert torch.equal(out, lock[0]) and torch.equal(out2, lock[1]), "pipelined loop differs from the lockstep loop on the same tiles"
    for _ in range(20):
        o, o2 = run(cfg)
        assert torch.equal(o, out) and torch.equal(o2, out2), "pipelined loop is not run-to-run reproducible"


def test_conv_and_geglu_through_pipelined_loop(L):
    for cfg in (5, 6):
        lib.check(L.sdxl_set_gemm_mode(4 * cfg))
        try:
            test_conv3x3_fwd_dgrad_wgrad(L, 2, 16, 12, 320, 640, 1)
            test_conv3x3_fwd_dgrad_wgrad(L, 1, 32, 32, 960, 320, 1)
            test_conv3x3_fwd_dgrad_wgrad(L, 1, 32, 32, 1280, 1280, 1)
            _ff_geglu_case(L, 308, 320, 1280, 80 if cfg == 5 else 64)
            _ff_geglu_case(L, 4096, 1280, 5120, 80 if cfg == 5 else 64)
        finally:
            lib.check(L.sdxl_set_gemm_mode(1))


def test_conv_and_geglu_through_splitk_groups(L):
    lib.check(L.sdxl_set_gemm_mode(4 * 23))
    try:
        test_conv3x3_fwd_dgrad_wgrad(L, 2, 16, 12, 320, 640, 1)
        test_conv3x3_fwd_dgrad_wgrad(L, 1, 32, 32, 960, 320, 1)
        _ff_geglu_case(L, 308, 320, 1280, 80)
        _ff_geglu_case(L, 4096, 1280, 5120, 80)
    finally:
        lib.check(L.sdxl_set_gemm_mode(1))


def _conv_ref(x_nhwc, w_native, bias, stride):
    """x [B,H,W,Cin], w [Cout][9][Cin] -> y [B,Ho,Wo,Cout] via F.conv2d fp32."""
    cout, _, cin = w_native.shape
    w = w_native.float().view(cout, 3, 3, cin).permute(0, 3, 1, 2).contiguous()
    y = torch.nn.functional.conv2d(x_nhwc.float().permute(0, 3, 1, 2), w, bias.float() if bias is not None else None,
                                   stride=stride, padding=1)
    return y.permute(0, 2, 3, 1).contiguous()


@pytest.mark.parametrize("B,H,W,Cin,Cout,stride", [(1, 8, 8, 64, 64, 1), (2, 16, 12, 320, 640, 1),
                                                   (2, 16, 16, 64, 128, 2), (1, 12, 20, 8, 320, 1),
                                                   (2, 8, 8, 192, 8, 1), (1, 32, 32, 960, 320, 1),
                                                   # the 1344x768 bucket's level widths (84, 42): the wgrad fast path's
                                                   # incremental (y, x) tracking wraps rows mid-K-step there
                                                   (2, 24, 42, 128, 64, 1), (1, 48, 84, 64, 128, 1), (3, 10, 42, 64, 64, 1),
                                                   # batch 1, 512^2 at the 1280-channel level: 256 pixels -> split (tap, channel) reduction
                                                   (1, 16, 16, 1280, 1280, 1), (1, 32, 32, 640, 1280, 1),
                                                   # B = 4, 1024^2 at the 1280-channel level: one round of 256 tiles -> two co-resident halves of the reduction
                                                   (4, 32, 32, 1280, 1280, 1), (4, 32, 32, 1920, 1280, 1), (4, 32, 32, 640, 1280, 1)]
                                                  # every other default bucket's row widths: one level-2, level-1 and level-0 image per family
                                                  + BK.CONV_S1)
def test_conv3x3_fwd_dgrad_wgrad(L, B, H, W, Cin, Cout, stride):
    x = rnd(B, H, W, Cin, seed=10)
    w = rnd(Cout, 9, Cin, seed=11, scale=(9 * Cin) ** -0.5)
    bias = rnd(Cout, seed=12)
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    y = torch.empty(B, Ho, Wo, Cout, dtype=torch.bfloat16, device=dev())
    lib.check(L.sdxl_op_conv3x3_fwd(ptr(x), ptr(w), ptr(bias), ptr(y), B, H, W, Cin, Cout, stride, stream()))
    xr = x.float().requires_grad_(True)
    wr = w.float().requires_grad_(True)
    ref = _conv_ref(xr, wr, bias, stride)
    report(f"conv fwd {B}x{H}x{W} {Cin}->{Cout} s{stride}", y, ref.detach(), 6e-3)
    dy = rnd(B, Ho, Wo, Cout, seed=13)
    ref.backward(dy.float())
    dx = torch.empty(B, H, W, Cin, dtype=torch.bfloat16, device=dev())
    lib.check(L.sdxl_op_conv3x3_dgrad(ptr(dy), ptr(w), ptr(dx), B, H, W, Cin, Cout, stride, stream()))
    report("conv dgrad", dx, xr.grad, 6e-3)
    for splitk in (1, 3):
        dw = torch.zeros(Cout, 9, Cin, dtype=torch.float32, device=dev())
        lib.check(L.sdxl_op_conv3x3_wgrad(ptr(x), ptr(dy), ptr(dw), B, H, W, Cin, Cout, stride, splitk, stream()))
        report(f"conv wgrad splitk={splitk}", dw, wr.grad, 1e-4 * math.sqrt(B * Ho * Wo) / 8 + 1e-5)


@pytest.mark.parametrize("B,H,W,Cin,Cout", [(1, 16, 16, 64, 64), (4, 128, 128, 320, 320), (4, 64, 64, 640, 640), (2, 48, 84, 64, 128), (3, 12, 20, 72, 64)] + BK.CONV_S2_DGRAD)
def test_conv3x3_stride2_dgrad_by_output_phase(L, B, H, W, Cin, Cout):
    """The input gradient of the stride-2 convolution from 1 / 2 / 2 / 4 taps per output phase (GemmP::up2 == 2) against autograd in fp32,
    with and without an addend; the two downsampler shapes of the headline step and the 1344 x 768 bucket's level included."""
    x = rnd(B, H, W, Cin, seed=30)
    w = rnd(Cout, 9, Cin, seed=31, scale=(9 * Cin) ** -0.5)
    xr = x.float().requires_grad_(True)
    ref = _conv_ref(xr, w, None, 2)
    dy = rnd(B, H // 2, W // 2, Cout, seed=32)
    ref.backward(dy.float())
    planar = torch.empty(4 * ((B * (H // 2) * (W // 2) + 127) // 128 * 128), Cin, dtype=torch.bfloat16, device=dev())
    for addend in (None, rnd(B, H, W, Cin, seed=33)):
        dx = torch.empty(B, H, W, Cin, dtype=torch.bfloat16, device=dev())
        lib.check(L.sdxl_op_conv3x3_s2_dgrad(ptr(dy), ptr(w), ptr(planar), ptr(dx), ptr(addend) if addend is not None else None, B, H, W, Cin, Cout, stream()))
        report(f"conv s2 dgrad by phase {B}x{H}x{W} {Cin}->{Cout} addend={addend is not None}", dx, xr.grad + (addend.float() if addend is not None else 0), 8e-3)
    if Cin % 64 or (B * (H // 2) * (W // 2)) % 64 or not lib.DIAG:
        return
    # diagnostics build: forward and weight gradient of the same convolution on the four phase planes of x (GemmP::up2 == 3)
    bias = rnd(Cout, seed=34)
    xplanar = torch.empty(4 * ((B * (H // 2) * (W // 2) + 127) // 128 * 128), Cin, dtype=torch.bfloat16, device=dev())
    y = torch.empty(B, H // 2, W // 2, Cout, dtype=torch.bfloat16, device=dev())
    lib.check(L.sdxl_op_conv3x3_s2_fwd(ptr(x), ptr(w), ptr(bias), ptr(xplanar), ptr(y), B, H, W, Cin, Cout, stream()))
    wr = w.float().requires_grad_(True)
    ref2 = _conv_ref(x.float(), wr, bias, 2)
    report("conv s2 fwd on phase planes", y, ref2.detach(), 8e-3)
    ref2.backward(dy.float())
    for splitk, acc in ((1, 0), (3, 1)):
        base = torch.randn(Cout, 9, Cin, device=dev()) if acc else torch.zeros(Cout, 9, Cin, device=dev())
        dw = base.clone()
        db = torch.zeros(Cout, dtype=torch.float32, device=dev())
        lib.check(L.sdxl_op_conv3x3_s2_wgrad(ptr(dy), ptr(xplanar), ptr(dw), ptr(db), acc, B, H, W, Cin, Cout, splitk, stream()))
        report(f"conv s2 wgrad on phase planes splitk={splitk}", dw - base, wr.grad, 1e-4 * math.sqrt(B * H * W / 4) / 8 + 1e-5)
        report("conv s2 bias grad", db, dy.float().sum((0, 1, 2)), 1e-4 * math.sqrt(B * H * W / 4) / 8 + 1e-5)


@pytest.mark.parametrize("B,H,W,Cin,Cout", [(1, 16, 16, 128, 64), (4, 32, 32, 1280, 1280), (4, 64, 64, 640, 640), (2, 24, 42, 64, 192), (4, 24, 42, 128, 64), (1, 32, 32, 320, 640)] + BK.UPCONV)
def test_upsample_conv3x3_without_the_upsampled_image(L, B, H, W, Cin, Cout):
    """conv3x3(nearest-2x(x)) as four 2 x 2 phase stencils on the low-resolution image (GemmP::up2) against conv2d(interpolate(x)) in fp32:
    forward (+ bias) and the input gradient (+ addend), borders included; the headline shapes of the two up-level transitions."""
    x = rnd(B, H, W, Cin, seed=20)
    w = rnd(Cout, 9, Cin, seed=21, scale=(9 * Cin) ** -0.5)
    bias = rnd(Cout, seed=22)
    weff = torch.empty(Cout, 16, Cin, dtype=torch.bfloat16, device=dev())
    planar = torch.empty(4 * ((B * H * W + 127) // 128 * 128), Cout, dtype=torch.bfloat16, device=dev())
    y = torch.empty(B, 2 * H, 2 * W, Cout, dtype=torch.bfloat16, device=dev())
    lib.check(L.sdxl_op_upconv3x3_fwd(ptr(x), ptr(w), ptr(bias), ptr(weff), ptr(planar), ptr(y), B, H, W, Cin, Cout, stream()))
    xr = x.float().requires_grad_(True)
    up = torch.nn.functional.interpolate(xr.permute(0, 3, 1, 2), scale_factor=2.0, mode="nearest")
    ref = torch.nn.functional.conv2d(up, w.float().view(Cout, 3, 3, Cin).permute(0, 3, 1, 2), bias.float(), padding=1).permute(0, 2, 3, 1)
    report(f"upconv fwd {B}x{H}x{W} {Cin}->{Cout}", y, ref.detach(), 8e-3)
    dy = rnd(B, 2 * H, 2 * W, Cout, seed=23)
    ref.backward(dy.float())
    addend = rnd(B, H, W, Cin, seed=24)
    dx = torch.empty(B, H, W, Cin, dtype=torch.bfloat16, device=dev())
    lib.check(L.sdxl_op_upconv3x3_dgrad(ptr(dy), ptr(weff), ptr(planar), ptr(dx), ptr(addend), B, H, W, Cin, Cout, stream()))
    report("upconv dgrad", dx, xr.grad + addend.float(), 8e-3)
    if (B * H * W) % 64:          # the weight-gradient form needs whole 64-pixel reduction steps (the plan falls back to the plain path otherwise)
        return
    wr = w.float().view(Cout, 3, 3, Cin).permute(0, 3, 1, 2).clone().requires_grad_(True)
    br = bias.float().clone().requires_grad_(True)
    torch.nn.functional.conv2d(torch.nn.functional.interpolate(x.float().permute(0, 3, 1, 2), scale_factor=2.0, mode="nearest"), wr, br,
                               padding=1).backward(dy.float().permute(0, 3, 1, 2))
    dw_ref = wr.grad.permute(0, 2, 3, 1).reshape(Cout, 9, Cin)
    dweff = torch.empty(Cout, 16, Cin, dtype=torch.float32, device=dev())
    for splitk, acc in ((1, 0), (3, 1)):
        base = torch.randn(Cout, 9, Cin, device=dev()) if acc else torch.zeros(Cout, 9, Cin, device=dev())
        dw = base.clone()
        db = torch.zeros(Cout, dtype=torch.float32, device=dev())
        lib.check(L.sdxl_op_upconv3x3_wgrad(ptr(planar), ptr(x), ptr(dweff), ptr(dw), ptr(db), acc, B, H, W, Cin, Cout, splitk, stream()))
        report(f"upconv wgrad splitk={splitk} acc={acc}", dw - base, dw_ref, 1e-4 * math.sqrt(4 * B * H * W) / 8 + 1e-5)
        report("upconv bias grad", db, br.grad, 1e-4 * math.sqrt(4 * B * H * W) / 8 + 1e-5)


@pytest.mark.parametrize("B,H,W,Cin,Cout", [(1, 128, 128, 320, 320), (4, 64, 64, 640, 320), (2, 128, 128, 192, 200), (1, 128, 128, 8, 320),
                                            (5, 64, 64, 64, 64),
                                            # W = 32 (the 1280-channel level at 1024^2): a K-step is two image rows, each with its own halo
                                            (4, 32, 32, 1280, 1280), (5, 32, 32, 200, 72), (8, 16, 32, 64, 128)]
                                           # W = 192 (the 640 x 1536 bucket): three K-steps per image row; the B = 1 case is below the policy's
                                           # 16 384 pixels and goes through the one-tap route: the same problem, parity only
                                           + BK.CONV_WGRAD3)
@pytest.mark.parametrize("splitk", [0, 1, 5])
def test_conv3x3_wgrad_three_taps_per_workgroup(L, B, H, W, Cin, Cout, splitk):
    """conv_wgrad3.hip (same-size stride-1 3x3, W % 64 == 0, >= 16 384 pixels: the 128^2 / 64^2 levels): a workgroup computes the three
    taps of one stencil row from ONE staged dY tile and an X tile with a one-pixel halo.  Against autograd through F.conv2d on every
    tap (image borders, row ends at the K-step seams, batch seams, ragged channel tiles), bias gradient, overwrite and += , the
    plan's split-K and forced ones; and against the one-tap-per-workgroup kernel."""
    if W == 32:
        if not knob(L, 14, 2):                     # the W = 32 form exists in the diagnostics build only (see conv_wgrad3_policy)
            pytest.skip("W = 32 three-tap form: diagnostics build only")
    try:
        _conv_wgrad3_case(L, B, H, W, Cin, Cout, splitk)
    finally:
        knob(L, 14, 0)


def _conv_wgrad3_case(L, B, H, W, Cin, Cout, splitk):
    x, dy = rnd(B, H, W, Cin, seed=14), rnd(B, H, W, Cout, seed=15)
    xr = x.float().permute(0, 3, 1, 2).requires_grad_(False)
    wr = torch.zeros(Cout, Cin, 3, 3, device=dev(), requires_grad=True)
    y = torch.nn.functional.conv2d(xr, wr, padding=1)
    y.backward(dy.float().permute(0, 3, 1, 2))
    ref = wr.grad.permute(0, 2, 3, 1).reshape(Cout, 9, Cin)                # native layout [co][tap][ci]
    tol = 1e-4 * math.sqrt(B * H * W) / 8 + 1e-5
    dw = torch.full((Cout, 9, Cin), 5.0, dtype=torch.float32, device=dev())
    db = torch.zeros(Cout, dtype=torch.float32, device=dev())
    lib.check(L.sdxl_op_conv3x3_wgrad2(ptr(x), ptr(dy), ptr(dw), ptr(db), B, H, W, Cin, Cout, 1, splitk, 0, stream()))
    report(f"conv wgrad3 {B}x{H}x{W} {Cin}->{Cout} splitk={splitk}", dw, ref, tol)
    report("conv wgrad3 bias grad", db, dy.float().sum((0, 1, 2)), 1e-4)
    lib.check(L.sdxl_op_conv3x3_wgrad2(ptr(x), ptr(dy), ptr(dw), None, B, H, W, Cin, Cout, 1, splitk, 1, stream()))
    report("conv wgrad3 +=", dw, 2 * ref, tol)
    if knob(L, 12, 1):                                                        # (diagnostics build: the one-tap kernel on the same problem)
        try:
            dw1 = torch.zeros(Cout, 9, Cin, dtype=torch.float32, device=dev())
            lib.check(L.sdxl_op_conv3x3_wgrad2(ptr(x), ptr(dy), ptr(dw1), None, B, H, W, Cin, Cout, 1, 0, 0, stream()))
        finally:
            knob(L, 12, 0)
            if W == 32:
                knob(L, 14, 2)
        report("conv wgrad3 vs one-tap kernel", dw * 0.5, dw1, tol)


def _attn_ref(q, k, v, heads):
    B, Nq, Cc = q.shape
    d = Cc // heads
    qh = q.view(B, Nq, heads, d).transpose(1, 2)
    kh = k.view(B, -1, heads, d).transpose(1, 2)
    vh = v.view(B, -1, heads, d).transpose(1, 2)
    s = (qh @ kh.transpose(-1, -2)) * 0.125
    p = torch.softmax(s, -1)
    o = (p @ vh).transpose(1, 2).reshape(B, Nq, Cc)
    return o, torch.logsumexp(s, -1)


@pytest.mark.parametrize("B,heads,Nq,Nk,self_attn", [(1, 1, 128, 64, False), (2, 2, 256, 256, True),
                                                     (2, 2, 200, 77, False), (1, 4, 1008, 1008, True),
                                                     (2, 10, 1024, 77, False),
                                                     # the headline shapes: level-1 self attention at 1024^2 (N = 4096, 10 heads),
                                                     # level 1 / level 2 of the 1344x768 bucket (N = 4032 / 1008: ragged last key
                                                     # tile), level-2 self attention (N = 1024, 20 heads), level-1 cross attention
                                                     (1, 10, 4096, 4096, True), (1, 10, 4032, 4032, True),
                                                     (1, 20, 1008, 1008, True), (1, 20, 1024, 1024, True),
                                                     (1, 10, 4096, 77, False), (1, 10, 4032, 77, False)]
                                                    # the other buckets: 3952 = 61 key tiles + 48 on the pipelined backward's route, 988 % 64 = 28
                                                    + BK.ATTENTION)
def test_attention_fwd_bwd(L, B, heads, Nq, Nk, self_attn):
    Cc = heads * 64
    if self_attn:
        qkv = rnd(B, Nq, 3 * Cc, seed=20)
        q, k, v = qkv[..., :Cc], qkv[..., Cc:2 * Cc], qkv[..., 2 * Cc:]
        ldq = ldk = ldv = 3 * Cc
    else:
        q = rnd(B, Nq, Cc, seed=21)
        kv = rnd(B, Nk, 2 * Cc, seed=22)
        k, v = kv[..., :Cc], kv[..., Cc:]
        ldq, ldk, ldv = Cc, 2 * Cc, 2 * Cc
    # make one query/key pair spike so the online-softmax rescale branch is exercised hard
    o = torch.empty(B, Nq, Cc, dtype=torch.bfloat16, device=dev())
    lse = torch.empty(B * heads, Nq, dtype=torch.float32, device=dev())
    lib.check(L.sdxl_op_attention_fwd(ptr(q), ptr(k), ptr(v), ptr(o), ptr(lse), B, heads, Nq, Nk, ldq, ldk, ldv, Cc, stream()))
    qr, kr, vr = (t.float().contiguous().requires_grad_(True) for t in (q, k, v))
    ref, lse_ref = _attn_ref(qr, kr, vr, heads)
    report(f"attn fwd B{B} h{heads} {Nq}x{Nk}", o, ref.detach(), 8e-3)
    report("attn lse", lse.view(B, heads, Nq), lse_ref.detach(), 1e-3)
    do = rnd(B, Nq, Cc, seed=23)
    ref.backward(do.float())
    delta = torch.empty(B * heads, Nq, dtype=torch.float32, device=dev())
    if self_attn:
        dqkv = torch.zeros_like(qkv)
        dq, dk, dv = dqkv[..., :Cc], dqkv[..., Cc:2 * Cc], dqkv[..., 2 * Cc:]
    else:
        dq = torch.zeros_like(q)
        dkv = torch.zeros_like(kv)
        dk, dv = dkv[..., :Cc], dkv[..., Cc:]
    lib.check(L.sdxl_op_attention_bwd(ptr(q), ptr(k), ptr(v), ptr(o), ptr(do), ptr(lse), ptr(delta), ptr(dq), ptr(dk),
                                      ptr(dv), B, heads, Nq, Nk, ldq, ldk, ldv, Cc, stream()))
    report("attn dQ", dq, qr.grad, 1.5e-2)
    report("attn dK", dk, kr.grad, 1.5e-2)
    report("attn dV", dv, vr.grad, 1.5e-2)


@pytest.mark.diag
@pytest.mark.parametrize("form", [2])
@pytest.mark.parametrize("B,heads,Nq,Nk", [(2, 2, 256, 256), (1, 4, 1008, 1008), (1, 10, 4096, 4096), (1, 10, 4032, 4032), (1, 20, 1024, 1024),
                                            (1, 1, 256, 1008), (1, 1, 64, 1024), (1, 3, 336, 320), (2, 1, 40, 257)])
def test_attention_fwd_pipelined(L, form, B, heads, Nq, Nk):
    """csrc/attention_pl.hip (diagnostics build, knob 33 = 2): the software-pipelined forward against fp32 softmax AND
    against the shipped tiled kernel on the same inputs.  Shapes: the model's (1024 / 4096 / 1008 / 4032: workgroup ranges that cross
    (batch, head) boundaries, 1 .. 5 query blocks per wave, ragged last key tile = the padding-count correction of the row sums), one
    block per wave (64 queries), ragged query count (40: rows beyond Nq never stored), Nk = 257 (63 padding keys in the last tile)."""
    Cc = heads * 64
    q = rnd(B, Nq, Cc, seed=61)
    kv = rnd(B, Nk, 2 * Cc, seed=62)
    k, v = kv[..., :Cc], kv[..., Cc:]
    ref, lse_ref = _attn_ref(q.float(), k.float(), v.float(), heads)
    outs = []
    for kv_ in (0, form):
        assert knob(L, 33, kv_)
        try:
            o = torch.full((B, Nq, Cc), float("nan"), dtype=torch.bfloat16, device=dev())
            lse = torch.full((B * heads, Nq), float("nan"), dtype=torch.float32, device=dev())
            lib.check(L.sdxl_op_attention_fwd(ptr(q), ptr(k), ptr(v), ptr(o), ptr(lse), B, heads, Nq, Nk, Cc, 2 * Cc, 2 * Cc, Cc, stream()))
            torch.cuda.synchronize()
        finally:
            knob(L, 33, 0)
        outs.append((o, lse))
    (o0, l0), (o1, l1) = outs
    assert torch.isfinite(o1.float()).all() and torch.isfinite(l1).all()
    report(f"attn fwd pipelined form {form} B{B} h{heads} {Nq}x{Nk}", o1, ref, 8e-3)
    report("attn lse pipelined", l1.view(B, heads, Nq), lse_ref, 1e-3)
    report("attn fwd pipelined vs tiled", o1, o0, 8e-3)


@pytest.mark.diag
@pytest.mark.parametrize("B,heads,Nq,Nk", [(2, 2, 256, 256), (1, 4, 1008, 1008), (1, 20, 1024, 1024), (1, 3, 336, 320), (2, 1, 264, 257), (1, 2, 300, 4032),
                                            (1, 1, 4096, 264)] + BK.ATTENTION_BWD_PL)
def test_attention_bwd_pipelined(L, B, heads, Nq, Nk):
    """csrc/attention_bwd_pl.hip on the shapes the policy does NOT send it (knob 35 = 2, diagnostics build; the product routes Nq, Nk >= 2048 there,
    which test_attention_fwd_bwd covers at 4096 and 4032): block ranges that cross (batch, head) boundaries with 0 .. 4 blocks per wave (1008, 336:
    21 blocks per pair), Nq != Nk, ragged last KEY tile (257, 264, 320: the dQ body's forced-zero P of padding keys) and ragged last QUERY tile (264, 300,
    336: zero rows and zero LSE / Delta entries from the out-of-range DMA).  Against fp32 autograd and against the tiled kernels on the same inputs."""
    Cc = heads * 64
    q = rnd(B, Nq, Cc, seed=71)
    kv = rnd(B, Nk, 2 * Cc, seed=72)
    k, v = kv[..., :Cc], kv[..., Cc:]
    do = rnd(B, Nq, Cc, seed=73)
    o = torch.empty(B, Nq, Cc, dtype=torch.bfloat16, device=dev())
    lse = torch.empty(B * heads, Nq, dtype=torch.float32, device=dev())
    lib.check(L.sdxl_op_attention_fwd(ptr(q), ptr(k), ptr(v), ptr(o), ptr(lse), B, heads, Nq, Nk, Cc, 2 * Cc, 2 * Cc, Cc, stream()))
    qr, kr, vr = (t.float().contiguous().requires_grad_(True) for t in (q, k, v))
    ref, _ = _attn_ref(qr, kr, vr, heads)
    ref.backward(do.float())
    outs = []
    for kn in (1, 2):
        assert knob(L, 35, kn)
        try:
            delta = torch.empty(B * heads, Nq, dtype=torch.float32, device=dev())
            dq = torch.full_like(q, float("nan"))
            dkv = torch.full_like(kv, float("nan"))
            lib.check(L.sdxl_op_attention_bwd(ptr(q), ptr(k), ptr(v), ptr(o), ptr(do), ptr(lse), ptr(delta), ptr(dq), ptr(dkv[..., :Cc]), ptr(dkv[..., Cc:]),
                                              B, heads, Nq, Nk, Cc, 2 * Cc, 2 * Cc, Cc, stream()))
            torch.cuda.synchronize()
        finally:
            knob(L, 35, 0)
        outs.append((dq, dkv[..., :Cc], dkv[..., Cc:]))
    for name, got, old, rf in zip(("dQ", "dK", "dV"), outs[1], outs[0], (qr.grad, kr.grad, vr.grad)):
        assert torch.isfinite(got.float()).all(), name
        report(f"attn bwd pipelined {name} B{B} h{heads} {Nq}x{Nk}", got, rf, 1.5e-2)
        report(f"attn bwd pipelined {name} vs tiled", got, old, 1.5e-2)


@pytest.mark.parametrize("B,Nq,N,K,addend", [(1, 1024, 1280, 1280, True), (4, 1024, 1280, 1280, False), (1, 1000, 1280, 1280, True),
                                             (2, 200, 256, 128, False), (3, 70, 128, 64, True)] + BK.LINEAR_DGRAD_DELTA)
def test_linear_dgrad_delta_epilogue(L, B, Nq, N, K, addend):
    """GemmP::delta_out (csrc/gemm.hip epilogue of the 128 x 128 4-wave NN kernel; the plan uses it for the out-projection dgrad of the
    1280-channel self-attention layers, engine.hip LinearOp::plan_bwd): dO = dY W (+ addend) AND Delta = rowsum_head(bf16(dO) * O).
    Against fp32 torch, and against the stand-alone Delta pass (attn_delta_kernel, reached through sdxl_op_attention_bwd with the SAME
    dO and O): the fused form sums 64 products per row in a different order, nothing else.  Ragged M (1000, 400, 210 rows: partial last
    128-row tile) included; the tolerance on Delta is 2e-3 of max|Delta| -- fp32 sums of 64 bf16 x bf16 products in two orders."""
    M, heads = B * Nq, N // 64
    dy, w, o = rnd(M, K, seed=50), rnd(K, N, seed=51, scale=0.05), rnd(M, N, seed=52)
    add = rnd(M, N, seed=53) if addend else None
    d_o = torch.full((M, N), float("nan"), dtype=torch.bfloat16, device=dev())
    delta = torch.full((B * heads, Nq), float("nan"), dtype=torch.float32, device=dev())
    lib.check(L.sdxl_op_linear_dgrad_delta(ptr(dy), ptr(w), ptr(o), ptr(add), ptr(d_o), ptr(delta), B, Nq, N, K, stream()))
    ref = dy.float() @ w.float() + (add.float() if addend else 0.0)
    report(f"dgrad+delta dO {M}x{N}x{K}", d_o, ref, 6e-3)
    # Delta from the bf16 dO the kernel itself stored (that is what the attention backward reads), fp32
    dref = (d_o.float() * o.float()).view(B, Nq, heads, 64).sum(-1).permute(0, 2, 1).reshape(B * heads, Nq)
    assert torch.isfinite(delta).all()
    report("dgrad+delta Delta vs fp32 rowsum", delta, dref, 2e-3)
    # ... and against the stand-alone pass: attention backward computes Delta itself when it is not told that Delta is ready
    qkv = rnd(B, Nq, 3 * N, seed=54)
    q, k, v = qkv[..., :N], qkv[..., N:2 * N], qkv[..., 2 * N:]
    lse = torch.zeros(B * heads, Nq, dtype=torch.float32, device=dev())
    delta2 = torch.full_like(delta, float("nan"))
    dqkv = torch.zeros_like(qkv)
    lib.check(L.sdxl_op_attention_bwd(ptr(q), ptr(k), ptr(v), ptr(o), ptr(d_o), ptr(lse), ptr(delta2), ptr(dqkv[..., :N]), ptr(dqkv[..., N:2 * N]),
                                      ptr(dqkv[..., 2 * N:]), B, heads, Nq, Nq, 3 * N, 3 * N, 3 * N, N, stream()))
    report("dgrad+delta Delta vs attn_delta_kernel", delta, delta2, 2e-3)


def test_attention_rescale_branch(L):
    """A late, very large score forces the running max to jump at the last key tile (guide rule 26)."""
    B, heads, Nq, Nk, Cc = 1, 1, 128, 256, 64
    q, k, v = rnd(B, Nq, Cc, seed=30), rnd(B, Nk, Cc, seed=31), rnd(B, Nk, Cc, seed=32)
    k[0, 250] = q[0, 5] * 6.0
    o = torch.empty(B, Nq, Cc, dtype=torch.bfloat16, device=dev())
    lse = torch.empty(B * heads, Nq, dtype=torch.float32, device=dev())
    lib.check(L.sdxl_op_attention_fwd(ptr(q), ptr(k), ptr(v), ptr(o), ptr(lse), B, heads, Nq, Nk, Cc, Cc, Cc, Cc, stream()))
    ref, _ = _attn_ref(q.float(), k.float(), v.float(), heads)
    report("attn fwd spike", o, ref, 8e-3)


@pytest.mark.parametrize("F,Nk", [(150.0, 256), (150.0, 250), (150.0, 4096), (60.0, 4096)])
def test_attention_fixed_reference_overflow_fallback(L, F, Nk):
    """The forward keeps the first key tile's maximum as the softmax reference for the whole row and checks the row sums for
    overflow afterwards.  One query gets a score 1.44 * F log2 units above everything else in a LATE key tile: F = 150 (216
    units: exp2 overflows) must send its workgroup through the tracking second pass, F = 60 (86 units, P ~ 2^86) must come out
    right without it.  The spike lives on one coordinate that every other query has zeroed, so no other row sees it (a large
    score on many rows would only measure the bf16 rounding of the prescaled operand).  Output and LSE of every row against fp32
    softmax; LSE tolerance 4e-3 of max|LSE|: the dominant score itself carries one bf16 rounding of q * scale * log2 e."""
    B, heads, Nq, Cc = 1, 2, 256, 128
    q, k, v = rnd(B, Nq, Cc, seed=33), rnd(B, Nk, Cc, seed=34), rnd(B, Nk, Cc, seed=35)
    for (h, qi, ki) in ((0, 5, Nk - 3), (1, 200, Nk - 70)):      # (head, query, key): workgroup 0 / last tile, workgroup 1 / earlier tile
        c0 = 64 * h
        q[0, :, c0] = 0.0
        q[0, qi, c0] = 8.0
        k[0, ki, c0:c0 + 64] = 0.0
        k[0, ki, c0] = F
    o = torch.empty(B, Nq, Cc, dtype=torch.bfloat16, device=dev())
    lse = torch.empty(B * heads, Nq, dtype=torch.float32, device=dev())
    lib.check(L.sdxl_op_attention_fwd(ptr(q), ptr(k), ptr(v), ptr(o), ptr(lse), B, heads, Nq, Nk, Cc, Cc, Cc, Cc, stream()))
    ref, lse_ref = _attn_ref(q.float(), k.float(), v.float(), heads)
    assert torch.isfinite(o.float()).all() and torch.isfinite(lse).all()
    report(f"attn fwd overflow F={F} Nk={Nk}", o, ref, 8e-3)
    report("attn lse overflow", lse.view(B, heads, Nq), lse_ref, 4e-3)
    assert float((o[0, 5, :64].float() - v[0, Nk - 3, :64].float()).abs().max()) <= 2e-2 * float(v[0, Nk - 3, :64].float().abs().max()) + 1e-3


@pytest.mark.parametrize("B,HW,Cc,silu", [(2, 64, 64, 1), (2, 256, 320, 1), (1, 1024, 960, 1), (2, 144, 1280, 0),
                                          (2, 64, 192, 1), (1, 64, 2560, 1), (2, 4096, 640, 1), (1, 100, 320, 1),
                                          (2, 1000, 1920, 0)] + BK.GROUPNORM)
def test_groupnorm_fwd_bwd(L, B, HW, Cc, silu):
    G = 32
    x = (rnd(B, HW, Cc, seed=40) * 3.0 + 1.5).to(torch.bfloat16)
    gamma, beta = (rnd(Cc, seed=41) * 0.1 + 1.0).to(torch.bfloat16), rnd(Cc, seed=42)
    y = torch.empty_like(x)
    stats = torch.empty(B * G * 2, dtype=torch.float32, device=dev())
    ws = torch.empty(256 * B * Cc * 2 + 256 * B * G * 2 + B * Cc * 5, dtype=torch.float32, device=dev())
    eps = 1e-5
    lib.check(L.sdxl_op_groupnorm_fwd(ptr(x), ptr(y), ptr(gamma), ptr(beta), ptr(stats), ptr(ws), B, HW, Cc, G, eps, silu, stream()))
    xr = x.float().requires_grad_(True)
    gr, br = gamma.float().requires_grad_(True), beta.float().requires_grad_(True)
    n = torch.nn.functional.group_norm(xr.permute(0, 2, 1), G, gr, br, eps).permute(0, 2, 1)
    ref = torch.nn.functional.silu(n) if silu else n
    report(f"groupnorm fwd B{B} HW{HW} C{Cc} silu{silu}", y, ref.detach(), 8e-3)
    dy = rnd(B, HW, Cc, seed=43)
    ref.backward(dy.float())
    dx = torch.empty_like(x)
    dg = torch.zeros(Cc, dtype=torch.float32, device=dev())
    db = torch.zeros(Cc, dtype=torch.float32, device=dev())
    lib.check(L.sdxl_op_groupnorm_bwd(ptr(x), ptr(dy), ptr(gamma), ptr(beta), ptr(stats), ptr(dx), ptr(dg), ptr(db), ptr(ws),
                                      B, HW, Cc, G, silu, 0, stream()))
    report("groupnorm dx", dx, xr.grad, 1e-2)
    report("groupnorm dgamma", dg, gr.grad, 2e-3)
    report("groupnorm dbeta", db, br.grad, 2e-3)


def test_groupnorm_large_offset_inputs(L):
    """sigma ~ 2e4 regime (SURVEY hard parts): |mean| >> std must not cancel in the variance."""
    B, HW, Cc, G = 1, 512, 320, 32
    x = (rnd(B, HW, Cc, seed=44) * 50.0 + 2.0e4).to(torch.bfloat16)
    gamma, beta = torch.ones(Cc, dtype=torch.bfloat16, device=dev()), torch.zeros(Cc, dtype=torch.bfloat16, device=dev())
    y = torch.empty_like(x)
    stats = torch.empty(B * G * 2, dtype=torch.float32, device=dev())
    ws = torch.empty(256 * B * Cc * 2 + 256 * B * G * 2 + B * Cc * 5, dtype=torch.float32, device=dev())
    lib.check(L.sdxl_op_groupnorm_fwd(ptr(x), ptr(y), ptr(gamma), ptr(beta), ptr(stats), ptr(ws), B, HW, Cc, G, 1e-5, 0, stream()))
    ref = torch.nn.functional.group_norm(x.double().permute(0, 2, 1), G, None, None, 1e-5).permute(0, 2, 1)
    report("groupnorm offset 2e4", y, ref.float(), 1e-2)


@pytest.mark.parametrize("M,Cc", [(64, 128), (308, 640), (1000, 1280), (16, 256), (4096, 1280), (4100, 640)] + BK.LAYERNORM)
def test_layernorm_fwd_bwd(L, M, Cc):
    x = (rnd(M, Cc, seed=50) * 2.0 + 0.5).to(torch.bfloat16)
    gamma, beta = (rnd(Cc, seed=51) * 0.1 + 1.0).to(torch.bfloat16), rnd(Cc, seed=52)
    y = torch.empty_like(x)
    stats = torch.empty(M * 2, dtype=torch.float32, device=dev())
    lib.check(L.sdxl_op_layernorm_fwd(ptr(x), ptr(y), ptr(gamma), ptr(beta), ptr(stats), M, Cc, 1e-5, stream()))
    xr = x.float().requires_grad_(True)
    gr, br = gamma.float().requires_grad_(True), beta.float().requires_grad_(True)
    ref = torch.nn.functional.layer_norm(xr, (Cc,), gr, br, 1e-5)
    report(f"layernorm fwd {M}x{Cc}", y, ref.detach(), 8e-3)
    dy = rnd(M, Cc, seed=53)
    ref.backward(dy.float())
    dx = torch.empty_like(x)
    dg = torch.zeros(Cc, dtype=torch.float32, device=dev())
    db = torch.zeros(Cc, dtype=torch.float32, device=dev())
    # 0: the plan's form (dx and parameter partial sums in one pass + the fixed-order reduce); diagnostics build: 1 = lean dx kernel + a
    # parameter-gradient pass of partial rows, 3 = lean + the column-sum pass with one atomic per column and block (the form before round 5)
    for form in ((0, 1, 3) if lib.DIAG else (0,)):
        knob(L, 10, form)
        dx.zero_(); dg.zero_(); db.zero_()
        try:
            lib.check(L.sdxl_op_layernorm_bwd(ptr(x), ptr(dy), ptr(gamma), ptr(stats), ptr(dx), ptr(dg), ptr(db), M, Cc, 0, stream()))
        finally:
            knob(L, 10, 0)
        report(f"layernorm dx (form {form})", dx, xr.grad, 1e-2)
        report("layernorm dgamma", dg, gr.grad, 2e-3)
        report("layernorm dbeta", db, br.grad, 2e-3)
        if form in (0, 1):      # partial rows + one fixed-order sum per column: the same bits on every run
            dg2, db2 = torch.zeros_like(dg), torch.zeros_like(db)
            knob(L, 10, form)
            try:
                lib.check(L.sdxl_op_layernorm_bwd(ptr(x), ptr(dy), ptr(gamma), ptr(stats), ptr(dx), ptr(dg2), ptr(db2), M, Cc, 0, stream()))
            finally:
                knob(L, 10, 0)
            assert torch.equal(dg, dg2) and torch.equal(db, db2), "layernorm parameter gradients are not reproducible"
    base = rnd(M, Cc, seed=54)          # accumulate form: dx = addend + grad
    dx2 = base.clone()
    lib.check(L.sdxl_op_layernorm_bwd(ptr(x), ptr(dy), ptr(gamma), ptr(stats), ptr(dx2), ptr(dg), ptr(db), M, Cc, 1, stream()))
    report("layernorm dx += ", dx2, xr.grad + base.float(), 1e-2)


@pytest.mark.diag
@pytest.mark.parametrize("M,Cc,Kr,acc,keep_dy", [(4096, 1280, 1280, 1, 0), (4096, 1280, 3840, 0, 1), (1000, 640, 256, 1, 1),
                                                 (4032, 1280, 10240, 1, 0), (128, 128, 64, 0, 0), (300, 320, 192, 1, 1),
                                                 (16384, 512, 128, 0, 0)])
def test_linear_dgrad_with_layernorm_backward_epilogue(L, M, Cc, Kr, acc, keep_dy):
    """GemmP::ln_x (diagnostics build: measured, not shipped): the dgrad dY W of the linear layer behind a LayerNorm, with that LayerNorm's backward in its epilogue (row sums met across
    the column tiles of a row block through memory), against the two separate ops (the library's own dgrad + LayerNorm backward) and torch."""
    x = (rnd(M, Cc, seed=60) * 2.0 + 0.5).to(torch.bfloat16)
    gamma, beta = (rnd(Cc, seed=61) * 0.1 + 1.0).to(torch.bfloat16), rnd(Cc, seed=62)
    xf = x.float()
    stats = torch.stack([xf.mean(1), (xf.var(1, unbiased=False) + 1e-5).rsqrt()], 1).contiguous()      # [M][2] mean, rstd (as the forward leaves them)
    dyl = rnd(M, Kr, seed=63)                                   # output gradient of the linear layer [M][Kr]
    w = rnd(Kr, Cc, seed=64, scale=Kr ** -0.5)                  # its weight [out = Kr][in = Cc]
    addend = rnd(M, Cc, seed=65) if acc else None
    dx = torch.full((M, Cc), float("nan"), dtype=torch.bfloat16, device=dev())
    dy_out = torch.full((M, Cc), float("nan"), dtype=torch.bfloat16, device=dev()) if keep_dy else None
    nrb = (M + 127) // 128
    pcol = torch.full((nrb, 2, Cc), float("nan"), dtype=torch.float32, device=dev())
    lib.check(L.sdxl_op_linear_dgrad_ln_bwd(ptr(dyl), ptr(w), ptr(x), C.cast(stats.data_ptr(), C.POINTER(C.c_float)), ptr(gamma), ptr(addend),
                                            ptr(dx), ptr(dy_out), C.cast(pcol.data_ptr(), C.POINTER(C.c_float)), M, Cc, Kr, stream()))
    torch.cuda.synchronize()
    err = C.c_uint(99)
    lib.check(L.sdxl_ln_error(C.byref(err)))
    assert err.value == 0, f"LayerNorm-backward epilogue gave up its in-launch meeting (error word {err.value})"
    # reference: dy = bf16(dY W), then the LayerNorm backward of it in fp32
    dy_ref = (dyl.float() @ w.float()).to(torch.bfloat16)
    xr = x.float().requires_grad_(True)
    gr, br = gamma.float().requires_grad_(True), beta.float().requires_grad_(True)
    torch.nn.functional.layer_norm(xr, (Cc,), gr, br, 1e-5).backward(dy_ref.float())
    ref_dx = xr.grad + (addend.float() if acc else 0.0)
    if keep_dy:
        report(f"ln-epilogue dy {M}x{Cc}x{Kr}", dy_out, dy_ref, 8e-3)
    report(f"ln-epilogue dx {M}x{Cc}x{Kr} acc{acc}", dx, ref_dx, 1e-2)
    report("ln-epilogue dgamma", pcol[:, 0].sum(0), gr.grad, 3e-3)
    report("ln-epilogue dbeta", pcol[:, 1].sum(0), br.grad, 3e-3)
    if Cc % 128:
        return
    # against the library's own two-kernel path on the same bf16 dy: same formula, other summation order
    dx2 = addend.clone() if acc else torch.empty_like(x)
    dg = torch.zeros(Cc, dtype=torch.float32, device=dev())
    db = torch.zeros(Cc, dtype=torch.float32, device=dev())
    lib.check(L.sdxl_op_layernorm_bwd(ptr(x), ptr(dy_ref), ptr(gamma), ptr(stats), ptr(dx2), ptr(dg), ptr(db), M, Cc, acc, stream()))
    report("ln-epilogue dx vs the separate pass", dx, dx2, 1e-2)


def geglu_pack_rows(t, C4, G=64):
    """[2*C4, ...] source order (value rows | gate rows) -> the library's packed order (groups of G interleaved)."""
    a, g = t[:C4], t[C4:]
    shp = t.shape[1:]
    return torch.stack([a.reshape(C4 // G, G, *shp), g.reshape(C4 // G, G, *shp)], 1).reshape(2 * C4, *shp).contiguous()


def geglu_unpack_cols(u, C4, G=64):
    """[M, 2*C4] packed columns -> source order (value | gate)."""
    M = u.shape[0]
    v = u.reshape(M, C4 // G, 2, G)
    return torch.cat([v[:, :, 0].reshape(M, C4), v[:, :, 1].reshape(M, C4)], 1)


@pytest.mark.parametrize("M,K,C4,G", [(64, 128, 256, 64), (308, 320, 1280, 64), (308, 320, 1280, 80), (100, 128, 160, 80),
                                      (4096, 1280, 5120, 80), (4096, 1280, 5120, 64), (256, 256, 256, 64), (512, 256, 1280, 64)] + BK.FF_GEGLU)
def test_ff_geglu_fused_fwd_bwd(L, M, K, C4, G):
    lib.check(L.sdxl_set_gemm_mode(2 if G == 64 else 1))      # group 64: through the 256 x 256 kernel's in-register GEGLU epilogues
    try:
        _ff_geglu_case(L, M, K, C4, G)
    finally:
        lib.check(L.sdxl_set_gemm_mode(1))


def _ff_geglu_case(L, M, K, C4, G):
    """GEGLU fused into the two feed-forward projections (reference: diffusers GEGLU, ff.net.0.proj -> ff.net.2)."""
    x = rnd(M, K, seed=60)
    w1, b1 = rnd(2 * C4, K, seed=61, scale=K ** -0.5), rnd(2 * C4, seed=62, scale=0.1)
    w2 = rnd(K, C4, seed=63, scale=C4 ** -0.5)
    dy = rnd(M, K, seed=64)
    u = torch.empty(M, 2 * C4, dtype=torch.bfloat16, device=dev())
    g = torch.empty(M, C4, dtype=torch.bfloat16, device=dev())
    w1p, b1p = geglu_pack_rows(w1, C4, G), geglu_pack_rows(b1, C4, G)     # keep alive until the launch has been enqueued
    lib.check(L.sdxl_op_ff_geglu_fwd(ptr(x), ptr(w1p), ptr(b1p), ptr(u), ptr(g), M, K, C4, G, stream()))
    ur = (x.float() @ w1.float().t() + b1.float())
    report("ff geglu: u", geglu_unpack_cols(u, C4, G), ur, 6e-3)
    ub = geglu_unpack_cols(u, C4, G).float().requires_grad_(True)      # backward reference from the stored bf16 u
    a, t = ub.chunk(2, -1)
    gr = a * torch.nn.functional.gelu(t)
    report("ff geglu: g", g, gr.detach(), 6e-3)
    dg = dy.float() @ w2.float()
    gr.backward(dg)
    du = torch.empty_like(u)
    lib.check(L.sdxl_op_ff_geglu_bwd(ptr(dy), ptr(w2), ptr(u), ptr(du), M, K, C4, G, stream()))
    report("ff geglu: du", geglu_unpack_cols(du, C4, G), ub.grad, 1e-2)


@pytest.mark.parametrize("method", [0, 1])
def test_loss_kernels_vs_oracle(L, method):
    """Loss-side kernels against oracle/loss_ref.py (itself pinned to reference-generated goldens)."""
    from oracle import loss_ref as R
    B, H, W = 4, 16, 16
    g = torch.Generator().manual_seed(70 + method)
    lat, noise = torch.randn(B, 4, H, W, generator=g), torch.randn(B, 4, H, W, generator=g)
    pred = torch.randn(B, 4, H, W, generator=g)
    tag = torch.tensor([0.5, 1.0, 2.0, 1.5])
    if method == 0:
        ts = torch.tensor([0, 100, 500, 850])
        sig = R.karras_sigmas()[ts]
    else:
        sig = torch.sigmoid(torch.randn(B, generator=g))
    d = dev()
    lat_d, noise_d, sig_d, tag_d = lat.to(d), noise.to(d), sig.to(d), tag.to(d)
    lc = lib.LossConfig(method, 1, 1, 5.0, 1)
    b = lib.Batch(B, H, W, 77, lat_d.data_ptr(), noise_d.data_ptr(), sig_d.data_ptr(), None, None, None, None, tag_d.data_ptr())
    xin = torch.empty(B * H * W, 8, dtype=torch.bfloat16, device=d)
    lib.check(L.sdxl_op_loss(C.byref(lc), C.byref(b), ptr(xin), None, None, 1.0, None, 0, stream()))
    if method == 0:
        ref_in = R.add_noise(lat, noise, sig)
    else:
        ref_in = R.optimal_transport_path(noise, lat, sig)
    got_in = xin.float().view(B, H * W, 8)[..., :4].permute(0, 2, 1).reshape(B, 4, H, W).cpu()
    report("loss prepare", got_in, ref_in, 5e-3)
    assert float(xin.float()[:, 4:].abs().max()) == 0.0
    pred_bf = bf(pred)
    pred8 = torch.zeros(B * H * W, 8, dtype=torch.bfloat16, device=d)
    pred8[:, :4] = pred_bf.view(B, 4, H * W).permute(0, 2, 1).reshape(B * H * W, 4).to(d)
    out = torch.zeros(8, dtype=torch.float32, device=d)
    lib.check(L.sdxl_op_loss(C.byref(lc), C.byref(b), None, ptr(pred8), None, 1.0, ptr(out), 1, stream()))
    pr = pred_bf.float().requires_grad_(True)
    if method == 0:
        ref_loss = R.ddpm_loss(pr, lat, noise, ts, "v_prediction", 5.0, tag)
    else:
        ref_loss = R.flow_matching_loss(pr, noise, lat, tag)
    o = out.cpu()
    print("loss", float(o[0]), float(ref_loss))
    assert abs(float(o[0]) - float(ref_loss)) <= 1e-5 * abs(float(ref_loss)) + 1e-7     # fp32 reduction order only
    assert abs(float(o[2]) - float(pr.detach().abs().sum())) <= 1e-4 * float(pr.detach().abs().sum())
    ref_loss.backward()
    dp = torch.empty(B * H * W, 8, dtype=torch.bfloat16, device=d)
    lib.check(L.sdxl_op_loss(C.byref(lc), C.byref(b), None, ptr(pred8), ptr(dp), 0.25, ptr(out), 2, stream()))
    got = dp.float().view(B, H * W, 8)[..., :4].permute(0, 2, 1).reshape(B, 4, H, W).cpu()
    if float(ref_loss) >= 1000.0:
        assert float(got.abs().max()) == 0.0
    else:
        report("loss dpred", got, pr.grad * 0.25, 8e-3)


def test_loss_guard_device(L):
    """non-finite -> 1000 and zero gradient ; above cap -> 1000 and zero gradient (reference guard)."""
    B, H, W = 1, 8, 8
    d = dev()
    lat = torch.randn(B, 4, H, W, device=d)
    noise = torch.randn(B, 4, H, W, device=d)
    sig = torch.tensor([0.002], device=d)
    lc = lib.LossConfig(0, 1, 0, 5.0, 1)
    b = lib.Batch(B, H, W, 77, lat.data_ptr(), noise.data_ptr(), sig.data_ptr(), None, None, None, None, None)
    pred8 = torch.zeros(B * H * W, 8, dtype=torch.bfloat16, device=d)
    out = torch.zeros(8, dtype=torch.float32, device=d)
    lib.check(L.sdxl_op_loss(C.byref(lc), C.byref(b), None, ptr(pred8), None, 1.0, ptr(out), 1, stream()))
    assert float(out[0]) == 1000.0 and float(out[7]) == 0.0           # (noise-x)/0.002 squared >> 1000
    pred8[0, 0] = float("nan")
    lib.check(L.sdxl_op_loss(C.byref(lc), C.byref(b), None, ptr(pred8), None, 1.0, ptr(out), 1, stream()))
    assert float(out[0]) == 1000.0 and float(out[7]) == 0.0


def test_exchange_shadow_hook_leaves_the_buffer_alone_and_takes_its_time(L):
    """bench.py --exchange-shadow's stand-in kernel (sdxl_op_exchange_shadow): reads and writes back the buffer unchanged, paced over busy_us"""
    buf = rnd(1 << 20, seed=77)
    ref = buf.clone()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    lib.check(L.sdxl_op_exchange_shadow(ptr(buf), buf.numel() * 2, 8, 64 * 1024, 500.0, stream()))
    e1.record()
    torch.cuda.synchronize()
    assert torch.equal(buf, ref)
    assert e0.elapsed_time(e1) >= 0.45          # (no upper bound: a first launch may carry module load time)
    assert L.sdxl_op_exchange_shadow(None, 0, 8, 1024, 1.0, stream()) == 1
