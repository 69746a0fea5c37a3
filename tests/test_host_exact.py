"""tests/_exact.py is worth trusting: on the CPU, the exact reference passes its own checks and every defect that the old metric
(max|err| <= tol max|ref|, tests/test_gpu_ops.py) lets through fails them; the rounding cases of tests/test_gpu_ops_exact.py have the ties
they need; and that file's case table reaches every route of the GEMM family (lib.gemm_route: pure host code).  No GPU."""
import pytest
import torch

import sdxl_amd  # noqa: F401
from sdxl_amd import lib

import _exact as X

BF = torch.bfloat16
M0, N0, K0 = 308, 320, 2048      # the shape the defects were measured at


# ------------------------------------------------------------------------------------------------ the mutants: wrong epilogues / main loops
def trunc_bf16(x32):
    """fp32 -> bf16 by dropping the low 16 bits"""
    return (x32.contiguous().view(torch.int32) & -65536).view(torch.float32).to(BF)


def half_up_bf16(x32):
    """fp32 -> bf16 rounding ties away from zero (add half an ulp to the magnitude, truncate)"""
    return ((x32.contiguous().view(torch.int32) + 0x8000) & -65536).view(torch.float32).to(BF)


def acc32(o):
    """the fp32 accumulator of an NT problem (integers: exact in any order)"""
    return o["a"] @ o["w"].T


def correct(o):
    return (acc32(o) + o["bias"] + o["resid"]).to(BF)


MUTANTS = {
    "truncation": lambda o: trunc_bf16(acc32(o) + o["bias"] + o["resid"]),
    "half-up": lambda o: half_up_bf16(acc32(o) + o["bias"] + o["resid"]),
    "double rounding": lambda o: (acc32(o).to(BF).float() + o["bias"] + o["resid"]).to(BF),
}


def blockwise_bf16_accumulator(o, bk=64):
    """the accumulator rounded to bf16 between K blocks"""
    acc = torch.zeros(o["a"].shape[0], o["w"].shape[0])
    for k in range(0, o["a"].shape[1], bk):
        acc = (acc + o["a"][:, k:k + bk] @ o["w"][:, k:k + bk].T).to(BF).float()
    return (acc + o["bias"] + o["resid"]).to(BF)


@pytest.fixture(scope="module")
def nt_ints():
    o = X.gemm_operands(0, M0, N0, K0, integer=True, nonzero=True)      # zero-free: any dropped product shows
    exact, _ = X.gemm_ref64(0, o)
    return o, exact


def fails_exact(got, want):
    with pytest.raises(AssertionError, match="differ from the exact value"):
        X.assert_exact("mutant", got, want)


def test_the_exact_reference_passes_its_own_check(nt_ints):
    o, exact = nt_ints
    X.assert_exact("fp32 matmul -> one rounding", correct(o), X.expect(exact, True))
    X.assert_exact("fp32 output", acc32(o), X.expect(X.gemm_ref64(0, o, bias=False, resid=False)[0], False))
    # the fp32 result does not depend on the summation order: K in reverse, and in 7 split-K slabs summed last to first
    rev = torch.arange(K0 - 1, -1, -1)
    X.assert_exact("reversed K", (o["a"][:, rev] @ o["w"][:, rev].T + o["bias"] + o["resid"]).to(BF), X.expect(exact, True))
    slabs = [o["a"][:, k::7] @ o["w"][:, k::7].T for k in range(7)]
    X.assert_exact("7 slabs", (sum(reversed(slabs)) + o["bias"] + o["resid"]).to(BF), X.expect(exact, True))
    X.assert_has_ties(exact, "308 x 320 x 2048")


@pytest.mark.parametrize("name", list(MUTANTS))
def test_rounding_mutants_fail_the_exact_check(nt_ints, name):
    o, exact = nt_ints
    got, want = MUTANTS[name](o), X.expect(exact, True)
    n = X.count_diff(got, want)
    e = float((got.double() - exact).abs().max() / exact.abs().max())
    print(f"[mutant] {name}: {n} of {got.numel()} elements differ ({100 * n / got.numel():.2f} %); max err / max ref {e:.2e}: the old metric at 6e-3 passes it")
    assert e <= 6e-3, "this defect would have been seen by the old metric: not the mutant this test is about"
    fails_exact(got, want)


def test_accumulator_rounded_between_k_blocks_fails_the_exact_check(nt_ints):
    o, exact = nt_ints
    fails_exact(blockwise_bf16_accumulator(o), X.expect(exact, True))


def test_one_dropped_product_fails_the_exact_check(nt_ints):
    """the last K element dropped for one output row: 2^-8-sized in the old metric, a changed integer here"""
    o, exact = nt_ints
    a = o["a"].clone()
    a[M0 - 1, K0 - 1] = 0.0
    got = (a @ o["w"].T + o["bias"] + o["resid"]).to(BF)
    e = float((got.double() - exact).abs().max() / exact.abs().max())
    assert e <= 6e-3
    fails_exact(got, X.expect(exact, True))
    # ... and ONE product of one element, in fp32 (what a weight gradient stores): off by the product itself
    acc = acc32(o)
    acc[17, 33] -= o["a"][17, 100] * o["w"][33, 100]
    fails_exact(acc, X.expect(X.gemm_ref64(0, o, bias=False, resid=False)[0], False))


def test_dropped_and_duplicated_reduction_rows_fail_the_exact_check_at_k_65536():
    """the weight-gradient form at (8, 320, 65536): the last row of the reduction dropped (2.0e-3 of max|ref|: the old tolerance there is
    5.1e-3), and one row counted twice"""
    o = X.gemm_operands(2, 8, 320, 65536, integer=True)
    exact, _ = X.gemm_ref64(2, o)
    want = X.expect(exact, False)
    X.assert_exact("tn fp32", o["a"].T @ o["b"], want)
    dropped = o["a"][:-1].T @ o["b"][:-1]
    e = float((dropped.double() - exact).abs().max() / exact.abs().max())
    assert e <= 2e-5 * 65536 ** 0.5 + 1e-5, e      # the old metric passes it
    fails_exact(dropped, want)
    fails_exact(o["a"].T @ o["b"] + torch.outer(o["a"][4095], o["b"][4095]), want)
    # bias gradient: column sums of a, exact too
    X.assert_exact("tn bias grad", o["a"].sum(0), X.expect(o["a"].double().sum(0), False))


def test_the_per_element_bound_passes_a_correct_kernel_and_fails_truncation_and_a_dropped_product():
    o = X.gemm_operands(0, M0, N0, K0, integer=False)
    ref, ab = X.gemm_ref64(0, o)
    bnd = X.bound(ref, ab, K0, True)
    acc = acc32(o)
    r = X.check_bound("fp32 matmul -> one rounding", (acc + o["bias"] + o["resid"]).to(BF), ref, bnd)
    assert r < 1.0
    with pytest.raises(AssertionError, match="a-priori bound"):
        X.check_bound("truncation", trunc_bf16(acc + o["bias"] + o["resid"]), ref, bnd)
    # one product dropped: the largest of the element whose bound is smallest (that a product of typical size hides under the rounding of
    # a large result is the limit of any per-element bound; the integer check above has no such limit)
    i, j = divmod(int(bnd.argmin()), N0)
    k = int((o["a"][i] * o["w"][j]).abs().argmax())
    a = o["a"].clone()
    a[i, k] = 0.0
    with pytest.raises(AssertionError, match="a-priori bound"):
        X.check_bound("dropped product", (a @ o["w"].T + o["bias"] + o["resid"]).to(BF), ref, bnd)
    # fp32 output (the weight gradient's bound): a correct fp32 matmul passes, a dropped reduction row does not
    t = X.gemm_operands(2, 72, 200, 520, integer=False)
    ref2, ab2 = X.gemm_ref64(2, t)
    b2 = X.bound(ref2, ab2, 520, False)
    X.check_bound("tn fp32", t["a"].T @ t["b"], ref2, b2)
    with pytest.raises(AssertionError, match="a-priori bound"):
        X.check_bound("tn dropped row", t["a"][:-1].T @ t["b"][:-1], ref2, b2)


def test_a_missing_element_fails_both_checks():
    """no element may be left out: one NaN (an unwritten output) fails"""
    o = X.gemm_operands(0, 16, 16, 64, integer=True)
    exact, _ = X.gemm_ref64(0, o)
    got = correct(o)
    got[3, 5] = float("nan")
    fails_exact(got, X.expect(exact, True))
    with pytest.raises(AssertionError, match="not written everywhere"):
        X.check_bound("nan", got, exact, X.bound(exact, exact.abs(), 64, True))


# ------------------------------------------------------------------------------------------------ the rounding cases have their ties
def rounding_cases():
    """every bf16-output GEMM case of the GPU file: forms 0 / 1 with the even residual (form 1: accumulate = 1 onto it)"""
    seen, out = set(), []
    for c in X.gemm_cases():
        if c.form != 2 and (c.form, c.M, c.N, c.K) not in seen:
            seen.add((c.form, c.M, c.N, c.K))
            out.append((c.form, c.M, c.N, c.K))
    out += [(f, M, N, K) for (f, M, N, K) in X.STREAM_K_PROBLEMS if f != 2 and (f, M, N, K) not in seen]
    return out


@pytest.mark.parametrize("form,M,N,K", rounding_cases())
def test_every_designated_rounding_case_has_ties(form, M, N, K):
    o = X.gemm_operands(form, M, N, K, integer=True)
    exact, _ = X.gemm_ref64(form, o, bias=form == 0)
    X.assert_has_ties(exact, f"form {form} {M}x{N}x{K}")
    assert float(exact.abs().max()) + 518 < 2.0 ** 24


def test_tie_counting_on_known_values():
    v = torch.tensor([256.0, 257.0, 259.0, 258.0, 514.0, 518.0, 516.0, -257.0, -259.0, 100.0, 1026.0, 1028.0, 1036.0])
    #                 exact  down   up     exact  down   up     exact  down    up      exact  no tie  down    up        (spacing 2 | 4 | 8)
    up, down = X.tie_fractions(v.double())
    assert (round(up * 13), round(down * 13)) == (4, 4)
    with pytest.raises(AssertionError):
        X.assert_has_ties(torch.arange(0, 200).double())      # below 256 every integer is exact: no rounding case


# ------------------------------------------------------------------------------------------------ the case table reaches every route
def _routes(diag):
    L = lib.load()
    rows = [(c, X.case_route(lib, L, c)) for c in X.gemm_cases() if diag or not c.diag]
    for (B, H, W, Cin, Cout) in X.CONV_WGRAD3:
        for sk in X.CONV_WGRAD3_SPLITK:
            rows.append((("conv wgrad3", B, H, W, Cin, Cout, sk), X.route_of(lib, L, 1, **X.conv_desc("wgrad", B, H, W, Cin, Cout, 1, sk, 1))))
    return rows


def test_the_exact_cases_reach_every_route_of_the_gemm_family():
    """kernels 0 .. 5 (stream-K, 6, exists in the diagnostics build only), every split-K pass, the 128-row kernel with the FAST staging and
    without.  A route added to gemm_route later has no exact case until someone adds one: the new name is missing from the set here."""
    rows = _routes(lib.DIAG)
    kernels = {r["kernel"] for _, r in rows}
    product = set(lib.GEMM_KERNELS) - {"stream-K"}
    assert kernels == product, f"kernels without an exact case: {product - kernels}; unknown: {kernels - product}"
    assert {r["post"] for _, r in rows} == set(lib.GEMM_POSTS)
    assert {r["fast"] for _, r in rows if r["kernel"] == "128-row"} == {True, False}
    # the forced cases do run what they force (a case that quietly fell back to the 128-row kernel would test nothing new)
    for c, r in rows:
        fam = c[0] if isinstance(c, tuple) and not isinstance(c, X.Case) else c.family
        if fam.startswith("cr256") and (c.M, c.N, c.K) != (300, 200, 128):
            assert r["kernel"] == "cr256", (c, r)
        if fam.startswith("gemm256"):
            assert r["kernel"] == "256x256", (c, r)
        if fam.startswith("pipelined cfg") and c.mode // 4 in (7, 8):
            assert r["kernel"] == "pipelined", (c, r)
        if fam.startswith("pipelined cfg") and c.mode // 4 in (5, 6):
            assert r["kernel"] == "128-row" and r["cfg"] in (5, 6), (c, r)      # (5: 160-column tiles, 6: 128; N decides between them)
        if fam == "cfg 23":
            assert (r["kernel"], r["cfg"]) == ("128-row", 23), (c, r)
        if fam == "tn long reduction":
            assert r["kernel"] == "wgrad256", (c, r)
        if fam == "conv wgrad3":
            assert r["kernel"] == "conv_wgrad3", (c, r)
        if fam == "bf16 split-K":
            assert r["post"] == "splitk_epilogue", (c, r)
    assert len(lib.GEMM_KERNELS) == 7 and len(lib.GEMM_POSTS) == 3, "a new route: give it an exact case in tests/_exact.py and name it here"


@pytest.mark.diag
def test_the_stream_k_problems_reach_kernel_6_in_the_diagnostics_build():
    L = lib.load()
    lib.check(L.sdxl_set_sk_mode(2, 0))
    try:
        for (f, M, N, K) in X.STREAM_K_PROBLEMS:
            assert lib.gemm_route(form=f, M=M, N=N, K=K, bias_grad=int(f == 2))["kernel"] == "stream-K", (f, M, N, K)
    finally:
        lib.check(L.sdxl_set_sk_mode(0, 0))
    assert {r["kernel"] for c, r in _routes(True) if isinstance(c, X.Case) and c.diag and c.M % 8 == 0} == {"cr256"}      # (M = 300: the 128-row kernel)
