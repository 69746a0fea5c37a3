"""tests/_temb.py is worth trusting, and tests/test_gpu_ops_temb.py runs what it says it runs.  On the CPU: the case tables are held to the
route hook's own scan (lib.gemm_route: pure host code) and to tests/_buckets.py where a bucket's number is used; the references pass their own
checks; and mutants of the references -- the ways a time-embedding kernel could be subtly wrong -- fail the new criterion, with the per-tensor
number of the model tests (rel-L2 <= 6e-2, cosine >= 0.995: tests/test_gpu_model.py) computed on the same data and printed next to it.  No GPU."""
import ctypes as C
import re
from pathlib import Path

import pytest
import torch

import sdxl_amd  # noqa: F401
from sdxl_amd import lib

import _buckets as BK
import _exact as X
import _nonlinear as NL
import _temb as T

BF = torch.bfloat16
ROOT = Path(__file__).resolve().parent.parent
NEW_HOOKS = {"sdxl_op_gemm_rowvec": 15, "sdxl_op_conv3x3_fwd_rowvec": 12, "sdxl_op_colsum": 8, "sdxl_op_sincos": 6}
N_TEST_HOOKS = 29      # (with the three plan-map hooks and the loss plan hook: tests/test_host_insitu.py)


# ------------------------------------------------------------------------------------------------ the hooks
def test_the_new_hooks_are_test_hooks_and_the_count_is_documented():
    for name, nargs in NEW_HOOKS.items():
        assert name in lib.TEST_HOOK_SIGNATURES and name not in lib.SIGNATURES and name not in lib.DIAG_SIGNATURES
        assert len(lib.TEST_HOOK_SIGNATURES[name]) == nargs
        assert hasattr(lib.load(), name)
    assert len(lib.TEST_HOOK_SIGNATURES) == N_TEST_HOOKS
    assert f"{N_TEST_HOOKS} test hooks" in (ROOT / "README.md").read_text()
    hdr = (ROOT / "include" / "sdxlstep_diag.h").read_text()
    fields = re.search(r"typedef struct sdxl_gemm_desc \{\s*int ([^;]*);", hdr).group(1).replace(" ", "").split(",")
    assert tuple(fields) == lib.GEMM_DESC_FIELDS + lib.GEMM_DESC_HOOK_FIELDS and fields[-1] == "rowvec"


def test_the_route_hook_describes_a_row_vector_and_defaults_to_none():
    plain = dict(form=0, M=4096, N=1280, K=1280)
    assert lib.gemm_route(**plain) == lib.gemm_route(**plain, rowvec=0)
    assert lib.gemm_route(**plain)["kernel"] == "pipelined"      # one round of 128 x 160 tiles: the policy's pipelined kernel ...
    r = lib.gemm_route(**plain, rowvec=1)
    assert r["kernel"] == "128-row" and r["cfg"] in (3, 23), r      # ... which has no row vector: the 8-wave 128 x 160 configuration instead
    for cfg in T.PIPELINED:      # forced: it must fall back, never drop the vector
        for c in T.ROWVEC_CASES + T.ROWVEC_CR256 + [dict(plain)]:
            d = dict(c, cfg=cfg, rowvec=1) if isinstance(c, dict) else T.rv_desc(c, cfg)
            assert lib.gemm_route(**d)["kernel"] != "pipelined", (cfg, c)
    with pytest.raises(lib.SdxlError, match="row vector"):
        lib.gemm_route(form=0, M=64, N=128, K=64, geglu=1, geglu_group=64, rowvec=1)


def _dummy(n=1 << 16):
    """host memory that a refused call never touches: 16-byte aligned"""
    buf = (C.c_char * (n + 16))()
    return buf, (C.addressof(buf) + 15) // 16 * 16


def test_the_hooks_refuse_a_bad_row_vector_and_65_batches_before_any_launch():
    """on a machine without a GPU a launch would fail with a HIP error instead: the message tells them apart"""
    L = lib.load()
    keep, p = _dummy()
    V = C.c_void_p
    gemm = lambda vec, ldv, rpb, M=260: L.sdxl_op_gemm_rowvec(0, V(p), V(p), V(p), M, 128, 64, None, None, vec, ldv, rpb, 1, 0, None)
    conv = lambda vec, ldv: L.sdxl_op_conv3x3_fwd_rowvec(V(p), V(p), None, vec, ldv, V(p), 2, 13, 10, 32, 128, None)
    col, sc = L.sdxl_op_colsum, L.sdxl_op_sincos
    for call, msg in ((lambda: gemm(V(p), 324, 130), "multiple of 8"), (lambda: gemm(V(p + 2), 320, 130), "16-byte aligned"),
                      (lambda: gemm(None, 320, 130), "16-byte aligned"), (lambda: gemm(V(p), 320, 0), "whole samples"),
                      (lambda: gemm(V(p), 320, -3), "whole samples"), (lambda: gemm(V(p), 320, 128), "whole samples"),
                      (lambda: gemm(V(p), 120, 130), "at least N"), (lambda: conv(V(p), 324), "multiple of 8"), (lambda: conv(V(p + 8), 320), "16-byte aligned"),
                      (lambda: L.sdxl_op_gemm_rowvec(1, V(p), V(p), V(p), 260, 128, 64, None, None, V(p), 320, 130, 1, 0, None), "NT only"),
                      (lambda: col(V(p), 8, V(p), 8, 65, 4, 8, None), "65 batches"), (lambda: col(V(p), 8, V(p), 8, 0, 4, 8, None), "0 batches"),
                      (lambda: col(V(p), 12, V(p), 8, 1, 4, 8, None), "ldx"), (lambda: sc(V(p), V(p), 4, 32, 24, None), "sincos")):
        assert call() != 0
        assert msg in L.sdxl_last_error().decode(), (msg, L.sdxl_last_error().decode())
    del keep


# ------------------------------------------------------------------------------------------------ the case tables against the route scan
_ALL_RV = list(T.ROWVEC_FORCED)


def test_the_forced_table_is_exactly_what_the_route_scan_grants():
    """every configuration word the library accepts, with the row-vector flag set: the GPU file's table names each (kernel, configuration) the scan
    reaches and nothing it does not.  The route hook answers for 33 / 34 in the product build too (the library then runs 31 / 32's kernel):
    they are the diagnostics build's cases."""
    L = lib.load()
    assert set(_ALL_RV) == set(T.ROWVEC_CASES + [T.ROWVEC_G256, T.ROWVEC_G256_WHOLE] + T.ROWVEC_CR256)
    reached = set()
    for c in _ALL_RV:
        forced = T.rv_forced(lib, L, c)
        got = sorted(cfg for cfg, _ in forced if cfg not in T.ROWVEC_NOT_COVERED)
        cr = any(f in T.FORCE_CR256 for f in T.ROWVEC_FORCED[c])
        assert got == sorted(T.ROWVEC_FORCED[c] + (T.FORCE_CR256_DIAG if cr else ())), (c, got)
        for cfg, r in forced:
            assert r["kernel"] == ("cr256" if 31 <= cfg <= 36 else "128-row"), (c, cfg, r)
            assert r["post"] == ("splitk_epilogue" if c.splitk > 1 else "none"), (c, cfg, r)
            reached.add((r["kernel"], cfg))
        m2 = T.rv_route(lib, L, c, mode=2)["kernel"]
        assert m2 == ("256x256" if c == T.ROWVEC_G256_WHOLE else "128-row"), (c, m2)      # gemm mode 2 adds a route at whole 256-row tiles only
        reached.add((T.rv_route(lib, L, c)["kernel"], T.rv_route(lib, L, c)["cfg"]))
    # what the issue expects: the 128-row configurations, the co-resident modes at its two shapes
    assert {("128-row", f) for f in T.FORCE_128} <= reached and {("cr256", f) for f in T.FORCE_CR256} <= reached
    for c in T.ROWVEC_CR256:
        assert set(T.FORCE_CR256) <= set(T.ROWVEC_FORCED[c])
    assert T.rv_route(lib, L, T.ROWVEC_CASES[6])["post"] == "splitk_epilogue"


def test_both_store_branches_run_with_a_vector():
    """store_bf16's 4-column branch needs a 160-column tile: N % 160 == 0 under configurations 3 / 13 / 23 (and the co-resident 31 / 36)"""
    L = lib.load()
    both = [(c, f) for c in _ALL_RV for f in T.ROWVEC_FORCED[c] if "4-column" in T.store_branches(T.rv_route(lib, L, c, cfg=f), c.N)]
    assert {f for _, f in both} >= {3, 13, 23, 31, 36}
    assert "4-column" in T.store_branches(T.rv_route(lib, L, T.ROWVEC_CASES[0]), 160)      # the first case, under the policy
    assert all(c.N % 160 == 0 for c, _ in both)
    assert T.store_branches(T.rv_route(lib, L, T.ROWVEC_CASES[2]), 128) == "8-column stores"


@pytest.mark.diag
def test_the_stream_k_case_reaches_kernel_6_in_the_diagnostics_build():
    L = lib.load()
    lib.check(L.sdxl_set_sk_mode(2, 0))
    try:
        assert T.rv_route(lib, L, T.ROWVEC_SK)["kernel"] == "stream-K"
    finally:
        lib.check(L.sdxl_set_sk_mode(0, 0))


def test_the_convolution_cases_split_where_they_say_and_stay_on_the_128_row_kernel():
    L = lib.load()
    sk = [T.conv_rv_desc(c)["splitk"] for c in T.CONV_CASES]
    assert sk[0] == 1 and sk[1] > 1 and sk[2] > 1, sk
    assert T.CONV_CASES[0].H * T.CONV_CASES[0].W == 130
    for c in T.CONV_CASES:
        for mode in (1,) + T.CONV_MODES.get(c, ()):
            r = X.route_of(lib, L, mode, **T.conv_rv_desc(c))
            assert r["kernel"] == "128-row" and r["post"] == ("splitk_epilogue" if T.conv_rv_desc(c)["splitk"] > 1 else "none"), (c, mode, r)


def test_the_cases_that_use_a_buckets_numbers_use_them():
    assert 988 in BK.tokens_at_level(2) and 3952 in BK.tokens_at_level(1)      # (2, 988, 320, 64), the column sums' (4, 988, 640)
    assert 4096 in BK.tokens_at_level(1)                                       # the up-sampler's bias gradient: (1, 4096, 1280)
    ragged = [t for lv in (0, 1, 2) for t in BK.tokens_at_level(lv) if t % 128 or t % 256]
    assert len(ragged) > 0 and 988 in ragged and 3952 in ragged


def test_the_short_reductions_are_in_the_exact_table_and_stay_on_the_128_row_kernel():
    L = lib.load()
    rows = {(c.family, c.mode, c.form, c.M, c.N, c.K): X.case_route(lib, L, c) for c in X.gemm_cases() if "short reduction" in c.family or "grouped projection" in c.family}
    assert len(rows) == len(X.TN_SHORT) + 2 + 1 + len(X.CR256_MODES)
    assert {k[5] for k in rows if k[2] == 2} == {1, 2, 4}
    for k, r in rows.items():
        if k[2] == 2:
            assert r["kernel"] == "128-row", (k, r)      # K % 64 (256 x 256) and K % 32 (co-resident) turn the forced words away


# ------------------------------------------------------------------------------------------------ row vector: the reference and its mutants
@pytest.mark.parametrize("c", _ALL_RV + [T.ROWVEC_SK], ids=str)
def test_every_row_vector_case_is_exact_in_fp32_and_has_its_ties(c):
    o = T.rv_operands(c, True)
    assert torch.equal(o["vec"].to(BF).float(), o["vec"]) and torch.equal(o["resid"].to(BF).float(), o["resid"])
    v = o["vec"]
    if c.B > 1:      # the next sample's vector is off by at least 16 in every column
        gap = (v[1:] - v[:-1]).abs().min()
        assert float(gap) >= 16 and float(v.abs().max()) <= 232, (float(gap), float(v.abs().max()))
    assert bool(torch.isnan(o["wide"][:, :T.col0_of(c.N)]).all()) and bool(torch.isnan(o["wide"][:, T.col0_of(c.N) + c.N:]).all())
    assert T.ldv_of(c.N) % 8 == 0 and T.col0_of(c.N) % 8 == 0
    for resid in (False, True):
        ref, _, _ = T.rv_ref64(o, c.rpb, resid)
        assert float(ref.abs().max()) + 518 < 2.0 ** 24
        fp32 = o["a"] @ o["w"].T + o["bias"] + o["vec"].repeat_interleave(c.rpb, 0) + (o["resid"] if resid else 0.0)
        X.assert_exact(f"{c} fp32 sum, one rounding", fp32.to(BF), X.expect(ref, True))
    X.assert_has_ties(T.rv_ref64(o, c.rpb, True)[0], str(c))


# the first-row mutant at the shape that has the model's geometry: a level's 988 rows per sample against 128-row tiles, one tile in eight with two samples
MUTANT_CASE = {"tile's first row decides": T.ROWVEC_CASES[5], "added after the rounding": T.ROWVEC_CASES[0], "dropped in the last 4 columns": T.ROWVEC_CASES[1],
               "read at column 0": T.ROWVEC_CASES[0]}


@pytest.mark.parametrize("name", T.RV_MUTANTS)
def test_row_vector_mutants_pass_the_per_tensor_number_and_fail_the_exact_check(name):
    c = MUTANT_CASE[name]
    o = T.rv_operands(c, True)
    ref, _, _ = T.rv_ref64(o, c.rpb, True)
    got = T.rv_mutant(name, o, c)
    rel, cos = T.per_tensor(got, ref)
    n = X.count_diff(got, X.expect(ref, True))
    print(f"[mutant] {name} at {c}: {n} of {got.numel()} elements differ; per tensor rel-L2 {rel:.3e}, cosine {cos:.6f} (bar {T.MODEL_BAR})")
    assert T.passes_model_bar(got, ref), "this defect would have been seen by the per-tensor number: not the mutant this test is about"
    with pytest.raises(AssertionError, match="differ from the exact value"):
        X.assert_exact(name, got, X.expect(ref, True))


def test_row_vector_mutants_fail_the_randn_bound_where_the_data_can_show_them():
    """on randn data the first-row and the dropped-vector mutants are off by a whole vector element: far outside the a-priori bound.  (A second
    rounding stays inside u |ref| + ... by construction of any per-element bound with one unit roundoff of slack for ties -- the integer check is what sees it.)"""
    c = T.ROWVEC_CASES[1]
    o = T.rv_operands(c, False)
    ref, ab, vabs = T.rv_ref64(o, c.rpb, True)
    bnd = T.rv_bound(ref, ab, vabs, c.K)
    rows = torch.arange(c.B * c.rpb)
    acc = o["a"] @ o["w"].T + o["bias"] + o["resid"]
    assert X.check_bound("correct", (acc + o["vec"][rows // c.rpb]).to(BF), ref, bnd) < 1.0
    vv = o["vec"][rows // c.rpb].clone()
    vv[:, -4:] = 0.0
    for name, got in (("first row", (acc + o["vec"][(rows // 128 * 128) // c.rpb]).to(BF)), ("dropped", (acc + vv).to(BF))):
        with pytest.raises(AssertionError, match="a-priori bound"):
            X.check_bound(name, got, ref, bnd)


# ------------------------------------------------------------------------------------------------ column sums
def test_the_column_sum_cases_reach_the_branches_they_name():
    for c, taken in T.COLSUM_BATCHED_BRANCH.items():
        assert T.colsum_geom(c.batches, c.rows, c.N)[3] == taken, c
    assert T.colsum_geom(4, 77, 320)[0] == 2 and 320 % 256 == 64            # a column block only part full
    assert T.colsum_geom(4, 988, 640)[1:3] == (8, 128) and 988 % 128 == 92  # eight chunks of 128 rows: the last holds 92
    assert max(c.batches for c in T.COLSUM_CASES) == T.COLSUM_MAX_BATCHES
    for c in T.COLSUM_CASES:
        assert c.batches * T.colsum_geom(c.batches, c.rows, c.N)[1] <= 1024 * c.batches      # one reduce chunk: a fixed order (launch_ln_param_reduce)
        assert T.colsum_geom(c.batches, c.rows, c.N)[1] <= 1024
        x, pre = T.colsum_operands(c, True)
        want, _ = T.colsum_ref64(c, x, pre)
        assert float(want.abs().max()) < 2.0 ** 24 and 2 * c.rows + 8 < 2 ** 24


@pytest.mark.parametrize("name", ["last chunk left out", "written to the neighbour's row"])
def test_column_sum_mutants_fail_the_exact_check_and_the_bound(name):
    """The per-tensor number of the sums themselves is printed, not asserted to pass: computed AT THE OP it sees both (rel-L2 0.31 and 1.04).
    No test computed it at the op; the model tests see these sums only inside the time-embedding linears' gradients, summed over every resnet."""
    c = T.CS(4, 988, 640)
    x, pre = T.colsum_operands(c, True)
    want, _ = T.colsum_ref64(c, x, pre)
    xs = x.double().view(c.batches, c.rows, c.N)
    got = pre.double().clone()
    sl = slice(T.COLSUM_COL0, T.COLSUM_COL0 + c.N)
    if name == "last chunk left out":
        y, rpc = T.colsum_geom(c.batches, c.rows, c.N)[1:3]
        got[:, sl] += xs[:, : (y - 1) * rpc].sum(1)
    else:
        s = xs.sum(1)
        s[[1, 2]] = s[[2, 1]]
        got[:, sl] += s
    rel, cos = T.per_tensor(got[:, sl], want[:, sl])
    print(f"[mutant] column sums, {name}: per tensor rel-L2 {rel:.3e}, cosine {cos:.6f} (bar {T.MODEL_BAR})")
    with pytest.raises(AssertionError, match="differ from the exact value"):
        X.assert_exact(name, got.float(), X.expect(want, False))
    # ... and on randn data, against the bound
    xr, _ = T.colsum_operands(c, False)
    wr, sabs = T.colsum_ref64(c, xr, pre)
    xsr = xr.double().view(c.batches, c.rows, c.N)
    ok = pre.double().clone()
    ok[:, sl] += xsr.float().sum(1).double()
    bnd = T.colsum_bound(c, sabs, wr[:, sl])
    assert X.check_bound("fp32 sum", ok[:, sl], wr[:, sl], bnd) < 1.0
    bad = pre.double().clone()
    bad[:, sl] += xsr[:, :896].sum(1) if name == "last chunk left out" else xsr.sum(1)[[0, 2, 1, 3]]
    with pytest.raises(AssertionError, match="a-priori bound"):
        X.check_bound(name, bad[:, sl], wr[:, sl], bnd)


# ------------------------------------------------------------------------------------------------ reductions shorter than a K block
def test_a_k4_reduction_that_reads_a_whole_k_block_fails_the_exact_check():
    """TN at K = 4 from a buffer whose rows 4 .. 63 are not zero (the next tensor of an arena): a kernel that stages a full 64-row block without
    masking the tail sums 60 rows too many"""
    M, N, K = 320, 128, 4
    big_a, big_b = X.ints(64, M, seed=401), X.ints(64, N, seed=402)
    ref = big_a[:K].double().T @ big_b[:K].double()
    X.assert_exact("tn K = 4", big_a[:K].T @ big_b[:K], X.expect(ref, False))
    got = big_a.T @ big_b
    rel, cos = T.per_tensor(got, ref)
    print(f"[mutant] TN K = 4 reading 64 rows: per tensor rel-L2 {rel:.3e}, cosine {cos:.6f}")
    with pytest.raises(AssertionError, match="differ from the exact value"):
        X.assert_exact("64 rows", got, X.expect(ref, False))
    # one row too many, with the weight of one sample of a batch of 4: what the model's tensors would show of it
    got1 = big_a[:K + 1].T @ big_b[:K + 1]
    with pytest.raises(AssertionError, match="differ from the exact value"):
        X.assert_exact("5 rows", got1, X.expect(ref, False))


# ------------------------------------------------------------------------------------------------ the sinusoidal embedding
def test_sincos_delta_is_small_and_the_fp32_restatement_lies_inside_every_interval():
    t = torch.tensor(T.SINCOS_T, dtype=torch.float32)
    dmax, share, two, n = 0.0, 0.0, 0, 0
    for dim in T.SINCOS_DIMS:
        ref, delta = T.sincos_ref(t, dim)
        dmax = max(dmax, float(delta.max()))
        got = T.sincos_f32(t, dim)
        share = max(share, float(((got.double() - ref).abs() / delta.clamp_min(1e-300))[delta > 0].max()))
        NL.check_interval(f"fp32 restatement, dim {dim}", got.to(BF), ref, delta)
        two += int((NL.bf16_rn64(ref - delta).float() != NL.bf16_rn64(ref + delta).float()).sum())
        n += ref.numel()
    print(f"[temb] sincos: max delta {dmax:.3e}; the fp32 restatement uses {share:.3f} of delta; {100 * two / n:.1f} % of the intervals span two bf16 values")
    assert dmax < 2.0 ** -9
    assert share < 1.0
    assert float(t.max()) == 2048.0 and abs(T.LN1E4_F32 - 9.210340371976184) < 1e-6
    assert T.sincos_timesteps(24).shape == (24,) and set(T.sincos_timesteps(24, 7).tolist()) <= set(t.tolist())
    assert bool((T.sincos_ref(torch.zeros(1), 32)[0][0, :16] == 1).all()) and bool((T.sincos_ref(torch.zeros(1), 32)[0][0, 16:] == 0).all())


@pytest.mark.parametrize("dim", T.SINCOS_DIMS)
@pytest.mark.parametrize("name", T.SINCOS_MUTANTS)
def test_sincos_mutants_fail_the_interval(name, dim):
    """the per-tensor number of the embedding itself is printed: it sees all four at the op (the tensor was never compared at the op before).  Through
    the model they reach the tests only as the time-embedding linears' gradients and the loss."""
    t = torch.tensor(T.SINCOS_T, dtype=torch.float32)
    ref, delta = T.sincos_ref(t, dim)
    got = T.sincos_f32(t, dim, name)
    rel, cos = T.per_tensor(got, ref)
    print(f"[mutant] sincos {name} dim {dim}: per tensor rel-L2 {rel:.3e}, cosine {cos:.6f}")
    with pytest.raises(AssertionError, match="outside their interval"):
        NL.check_interval(name, got.to(BF), ref, delta)
