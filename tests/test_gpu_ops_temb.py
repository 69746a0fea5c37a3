"""Per-element parity of the time-embedding path on a real MI355X (tests/_temb.py; shown to see what it claims on the CPU in
tests/test_host_temb.py): the path that carries the timestep and the size conditioning into every resnet, and their gradient back.

  * the row-vector epilogue C = bf16(acc + bias + rowvec[m / rows_per_batch] + resid) of every kernel of the GEMM family that has one
    (sdxl_op_gemm_rowvec, sdxl_op_conv3x3_fwd_rowvec): integer operands, bit equality with the integer sum rounded once, without and with
    the even residual; randn operands, the a-priori bound of tests/_exact.py for every element.  The vector is a column slice of a wider
    matrix whose other columns are NaN, the sample boundaries fall inside tiles, and every case runs under the policy and on every forced
    configuration that the route hook grants it (each case prints the route it reached and which store branches ran);
  * the column sums that carry the gradient back (sdxl_op_colsum): exact on integers, (rows - 1) 2^-24 sum|x| on randn, bit-reproducible;
  * the weight gradients whose reduction is the batch: rows of tests/_exact.py's table (run by tests/test_gpu_ops_exact.py) and one chained
    case here, column sums -> bf16 cast -> TN launch at K = 4;
  * the sinusoidal embedding (sdxl_op_sincos) against float64 inside bf16_rn(ref -+ delta), delta derived in tests/_temb.py;
  * one engine-level case: the tiny UNet's sample 0 does not see sample 1's timestep and time ids.
Each case prints its figures as `[temb] ...` / `[exact]` / `[bound]` / `[nonlinear]` lines (profiles/ops_temb.txt keeps them)."""
import ctypes as C

import pytest
import torch

import sdxl_amd  # noqa: F401
from sdxl_amd import lib

import _exact as X
import _nonlinear as NL
import _temb as T
from _isolation import Spec, assert_isolated, run_isolated

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


def ptr(t, elem_offset=0):
    return C.c_void_p(t.data_ptr() + elem_offset * t.element_size()) if t is not None else None


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def out_like(*shape, dtype=BF):
    return torch.full(shape, SENTINEL, dtype=dtype, device=dev())


_CACHE = {}


def cached(key, make):
    """operands and references are computed once, shared by every launch of the case, and never modified"""
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def rv_id(c):
    return f"B{c.B}-r{c.rpb}-N{c.N}-K{c.K}-s{c.splitk}"


# ------------------------------------------------------------------------------------------------ the row-vector epilogue, dense
def rv_data(c, integer):
    def make():
        o = T.rv_operands(c, integer)
        return o, {resid: T.rv_ref64(o, c.rpb, resid) for resid in (False, True)}
    return cached(("rv", c, integer), make)


def rv_launch(L, c, o_dev, resid, cfg):
    M = c.B * c.rpb
    out = out_like(M, c.N)
    lib.check(L.sdxl_op_gemm_rowvec(0, ptr(o_dev["a"]), ptr(o_dev["w"]), ptr(out), M, c.N, c.K, ptr(o_dev["bias"]), ptr(o_dev["resid"]) if resid else None,
                                    ptr(o_dev["wide"], T.col0_of(c.N)), T.ldv_of(c.N), c.rpb, c.splitk, cfg, stream()))
    return out


def rv_run(L, c, launches):
    """one case: [(label, gemm mode, per-launch cfg)] x (no residual, even residual) x (integers: bit equality | randn: the bound)"""
    worst = 0.0
    for integer in (True, False):
        o, refs = rv_data(c, integer)
        o_dev = {k: D(v) for k, v in o.items() if k != "vec"}
        for label, mode, cfg in launches:
            route = T.rv_route(lib, L, c, mode=mode, cfg=cfg)      # (under sdxl_set_sk_mode(2, .): stream-K)
            if integer:
                print(f"[temb] rowvec {rv_id(c)} {label}: {route} ; {T.store_branches(route, c.N)}")
            lib.check(L.sdxl_set_gemm_mode(mode))
            try:
                for resid in (False, True):
                    out = rv_launch(L, c, o_dev, resid, cfg)
                    ref, ab, vabs = refs[resid]
                    tag = f"rowvec {rv_id(c)} {label} {'int' if integer else 'randn'} resid {int(resid)}"
                    if integer:
                        X.assert_exact(tag, out, X.expect(ref, True))
                    else:
                        worst = max(worst, X.check_bound(tag, out, ref, T.rv_bound(ref, ab, vabs, c.K)))
            finally:
                lib.check(L.sdxl_set_gemm_mode(1))
    print(f"[temb] rowvec {rv_id(c)}: largest share of the bound used {worst:.3f}")


def rv_launches(c, extra_modes=()):
    return [("policy", 1, 0)] + [(f"cfg {f}", 1, f) for f in T.ROWVEC_FORCED[c]] + [(f"mode {m}", m, 0) for m in extra_modes]


_RV_ALL = T.ROWVEC_CASES + T.ROWVEC_CR256


@pytest.mark.parametrize("c", _RV_ALL, ids=[rv_id(c) for c in _RV_ALL])
def test_rowvec_epilogue_exact_and_bounded(L, c):
    """the issue's cases and the co-resident kernel's two shapes: the policy and every forced configuration of tests/_temb.py's table (held to
    the route scan by tests/test_host_temb.py)"""
    rv_run(L, c, rv_launches(c))


@pytest.mark.parametrize("c", [T.ROWVEC_G256, T.ROWVEC_G256_WHOLE], ids=rv_id)
def test_rowvec_epilogue_under_the_256x256_mode(L, c):
    """gemm mode 2: the 256 x 256 kernel takes whole tiles only, so at M = 520 the 128-row kernel runs and at M = 768 (sample boundaries at
    rows 192, 384, 576: inside tiles 0 and 2, and on the edge of tile 1 | 2's half) gemm256.hip's own epilogue does"""
    want = "256x256" if c == T.ROWVEC_G256_WHOLE else "128-row"
    assert T.rv_route(lib, L, c, mode=2)["kernel"] == want
    rv_run(L, c, rv_launches(c, extra_modes=(2,)))


@pytest.mark.diag
@pytest.mark.parametrize("c", T.ROWVEC_CR256, ids=rv_id)
def test_rowvec_epilogue_on_the_exclusive_co_resident_form(L, c):
    """modes 33 / 34 (diagnostics build)"""
    for f in T.FORCE_CR256_DIAG:
        assert T.rv_route(lib, L, c, cfg=f)["kernel"] == "cr256"
    rv_run(L, c, [(f"cfg {f}", 1, f) for f in T.FORCE_CR256_DIAG])


@pytest.mark.diag
@pytest.mark.parametrize("workers", T.STREAM_K_WORKERS)
def test_rowvec_epilogue_on_stream_k(L, workers):
    """gemm_sk.hip's copy of the epilogue: 3 tiles x 10 K-steps cut over 1, 7 and 37 (clamped to 30) workers"""
    c = T.ROWVEC_SK
    lib.check(L.sdxl_set_sk_mode(2, workers))
    try:
        assert T.rv_route(lib, L, c)["kernel"] == "stream-K"
        rv_run(L, c, [(f"stream-K w={workers}", 1, 0)])
        torch.cuda.synchronize()
    finally:
        lib.check(L.sdxl_set_sk_mode(0, 0))
    e = C.c_uint(0)
    lib.check(L.sdxl_sk_error(stream(), C.byref(e)))
    assert e.value == 0, f"stream-K hand-off gave up waiting (error word {e.value})"


def test_rowvec_hooks_refuse_before_any_launch(L):
    """ldv % 8, a misaligned vector, rows_per_batch < 1, M not whole samples: an error, and the output keeps the sentinel"""
    c = T.RV(2, 130, 128, 64)
    o, _ = rv_data(c, True)
    o_dev = {k: D(v) for k, v in o.items() if k != "vec"}
    M, col0, ldv = c.B * c.rpb, T.col0_of(c.N), T.ldv_of(c.N)
    out = out_like(M, c.N)
    call = lambda vec, ld, rpb: L.sdxl_op_gemm_rowvec(0, ptr(o_dev["a"]), ptr(o_dev["w"]), ptr(out), M, c.N, c.K, ptr(o_dev["bias"]), None, vec, ld, rpb, 1, 0, stream())
    for what, rc in (("ldv % 8", call(ptr(o_dev["wide"], col0), ldv + 4, c.rpb)), ("alignment", call(ptr(o_dev["wide"], col0 + 1), ldv, c.rpb)),
                     ("rows_per_batch 0", call(ptr(o_dev["wide"], col0), ldv, 0)), ("M % rows_per_batch", call(ptr(o_dev["wide"], col0), ldv, 128)),
                     ("no vector", call(None, ldv, c.rpb))):
        assert rc != 0, what
    cv = T.CONV_CASES[0]
    oc = {k: D(v) for k, v in T.conv_rv_operands(cv, True).items() if k != "vec"}
    y = out_like(cv.B, cv.H, cv.W, cv.Cout)
    ccall = lambda vec, ld: L.sdxl_op_conv3x3_fwd_rowvec(ptr(oc["x"]), ptr(oc["w"]), ptr(oc["bias"]), vec, ld, ptr(y), cv.B, cv.H, cv.W, cv.Cin, cv.Cout, stream())
    assert ccall(ptr(oc["wide"], T.col0_of(cv.Cout)), T.ldv_of(cv.Cout) + 4) != 0 and ccall(ptr(oc["wide"], T.col0_of(cv.Cout) + 1), T.ldv_of(cv.Cout)) != 0
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all()) and bool((y == SENTINEL).all()), "a refused call launched something"


# ------------------------------------------------------------------------------------------------ the row-vector epilogue, through the convolution
def cv_id(c):
    return f"{c.B}x{c.H}x{c.W}-{c.Cin}-{c.Cout}"


@pytest.mark.parametrize("c", T.CONV_CASES, ids=cv_id)
def test_rowvec_epilogue_through_the_convolution(L, c):
    """sdxl_op_conv3x3_fwd_rowvec = what ConvOp::fwd builds: the plan's split factor, rows_per_batch = H W; the borders counted tap by tap by the
    float64 convolution.  The last case also runs under the 256 x 256 mode and the co-resident configurations: a gathered (nine-tap) problem
    is not theirs, the route hook says so, and the 128-row kernel must still add the vector."""
    worst = 0.0
    for integer in (True, False):
        o = cached(("cv", c, integer), lambda: T.conv_rv_operands(c, integer))
        ref, ab, vabs = cached(("cvref", c, integer), lambda: T.conv_rv_ref64(o))
        od = {k: D(v) for k, v in o.items() if k != "vec"}
        for mode in (1,) + T.CONV_MODES.get(c, ()):
            route = X.route_of(lib, L, mode, **T.conv_rv_desc(c))
            if integer:
                print(f"[temb] conv rowvec {cv_id(c)} mode {mode}: {route} ; {T.store_branches(route, c.Cout)}")
            assert route["kernel"] == "128-row"
            lib.check(L.sdxl_set_gemm_mode(mode))
            try:
                y = out_like(c.B, c.H, c.W, c.Cout)
                lib.check(L.sdxl_op_conv3x3_fwd_rowvec(ptr(od["x"]), ptr(od["w"]), ptr(od["bias"]), ptr(od["wide"], T.col0_of(c.Cout)), T.ldv_of(c.Cout), ptr(y),
                                                       c.B, c.H, c.W, c.Cin, c.Cout, stream()))
            finally:
                lib.check(L.sdxl_set_gemm_mode(1))
            tag = f"conv rowvec {cv_id(c)} mode {mode} {'int' if integer else 'randn'}"
            if integer:
                X.assert_exact(tag, y, X.expect(ref, True))
            else:
                worst = max(worst, X.check_bound(tag, y, ref, T.rv_bound(ref, ab, vabs, 9 * c.Cin)))
    print(f"[temb] conv rowvec {cv_id(c)}: largest share of the bound used {worst:.3f}")


# ------------------------------------------------------------------------------------------------ the row-vector epilogue, isolation
def _I(name, t, ld=None, dtype=BF, role="in"):
    t2 = t.reshape(1, -1) if t.dim() == 1 else t.reshape(-1, t.shape[-1])
    return Spec(name, t2.shape[0], t2.shape[1], ld or t2.shape[1], dtype, t2, role)


def _P(a, name):
    return C.c_void_p(a.ptr(name))


def test_rowvec_dense_reads_and_writes_its_operands_only(L):
    """guard bands, the vector's surrounding columns (the gap of its rows: ldv = 2 N + 64) and a pattern-filled output; then the cross-sample
    form of test_gemm_rows_are_independent: sample 1's vector, rows and residual overwritten with the pattern leave sample 0's bits alone"""
    c = T.ISOLATION_DENSE
    o, _ = rv_data(c, False)
    M = c.B * c.rpb
    specs = [_I("A", o["a"]), _I("B", o["w"]), _I("bias", o["bias"]), _I("res", o["resid"]), _I("vec", o["vec"], T.ldv_of(c.N)),
             Spec("C", M, c.N, c.N, BF, None, "out")]      # (the hook's A, B, C and residual are dense: their edges are the guard bands)

    def fn(ar):
        lib.check(L.sdxl_op_gemm_rowvec(0, _P(ar, "A"), _P(ar, "B"), _P(ar, "C"), M, c.N, c.K, _P(ar, "bias"), _P(ar, "res"), _P(ar, "vec"), ar.ld("vec"),
                                        c.rpb, 1, 0, stream()))
    runs = run_isolated(fn, specs, device="cuda")
    assert_isolated(runs, what="rowvec dense")
    ref, ab, vabs = T.rv_ref64(o, c.rpb, True)
    X.check_bound("rowvec dense isolation, clean run", runs[0]["C"], ref, T.rv_bound(ref, ab, vabs, c.K))
    rows1 = slice(c.rpb, M)
    runs = run_isolated(fn, specs, device="cuda", poison={"A": rows1, "res": rows1, "vec": slice(1, 2)})
    assert_isolated(runs, rows={"C": slice(0, c.rpb)}, what="rowvec dense cross-sample")


def test_rowvec_convolution_reads_and_writes_its_operands_only(L):
    c = T.ISOLATION_CONV
    o = cached(("cv", c, False), lambda: T.conv_rv_operands(c, False))
    specs = [_I("x", o["x"]), _I("w", o["w"].reshape(c.Cout, 9 * c.Cin)), _I("bias", o["bias"]), _I("vec", o["vec"], T.ldv_of(c.Cout)),
             Spec("y", c.B * c.H * c.W, c.Cout, c.Cout, BF, None, "out")]

    def fn(ar):
        lib.check(L.sdxl_op_conv3x3_fwd_rowvec(_P(ar, "x"), _P(ar, "w"), _P(ar, "bias"), _P(ar, "vec"), ar.ld("vec"), _P(ar, "y"), c.B, c.H, c.W, c.Cin, c.Cout,
                                               stream()))
    runs = run_isolated(fn, specs, device="cuda")
    assert_isolated(runs, what="rowvec conv")
    ref, ab, vabs = T.conv_rv_ref64(o)
    X.check_bound("rowvec conv isolation, clean run", runs[0]["y"].view(c.B, c.H, c.W, c.Cout), ref, T.rv_bound(ref, ab, vabs, 9 * c.Cin))


# ------------------------------------------------------------------------------------------------ column sums
def cs_id(c):
    return f"{c.batches}x{c.rows}x{c.N}" + ("-ldout0" if c.ld_out_zero else "")


def cs_launch(L, c, xd, buf, ldx):
    ld_out = 0 if c.ld_out_zero else c.N + T.COLSUM_PAD
    lib.check(L.sdxl_op_colsum(ptr(xd), ldx, ptr(buf, T.COLSUM_COL0), ld_out, c.batches, c.rows, c.N, stream()))


@pytest.mark.parametrize("gap", [0, 8], ids=["dense", "ldx+8"])
@pytest.mark.parametrize("c", T.COLSUM_CASES, ids=cs_id)
def test_colsum_exact_bounded_and_reproducible(L, c, gap):
    """out is a slice at column 64 of a [batches][N + 128] buffer prefilled with small integers: prefill + sum there, the prefill elsewhere"""
    print(f"[temb] colsum {cs_id(c)}: (column blocks, row chunks, rows per chunk, batched branch) = {T.colsum_geom(c.batches, c.rows, c.N)}")
    ldx = c.N + gap
    for integer in (True, False):
        x, pre = cached(("cs", c, integer), lambda: T.colsum_operands(c, integer))
        want, sabs = cached(("csref", c, integer), lambda: T.colsum_ref64(c, x, pre))
        xw = torch.full((c.batches * c.rows, ldx), T.NAN)
        xw[:, :c.N] = x
        xd = D(xw)
        outs = []
        for _ in range(2):
            buf = D(pre, F32)
            cs_launch(L, c, xd, buf, ldx)
            outs.append(buf.cpu())
        tag = f"colsum {cs_id(c)} ldx {ldx} {'int' if integer else 'randn'}"
        sl = slice(T.COLSUM_COL0, T.COLSUM_COL0 + c.N)
        if integer:
            X.assert_exact(tag, outs[0], X.expect(want, False))
        else:
            r = X.check_bound(tag, outs[0][:, sl], want[:, sl], T.colsum_bound(c, sabs, want[:, sl]).clamp_min(1e-300))
            print(f"[temb] colsum {cs_id(c)} ldx {ldx}: share of the bound used {r:.3f}")
            rest = torch.ones(c.N + T.COLSUM_PAD, dtype=torch.bool)
            rest[sl] = False
            assert torch.equal(outs[0][:, rest], pre[:, rest]), f"{tag}: a column outside the slice changed"
        assert X.same_bits(outs[0], outs[1]), f"{tag}: two runs differ"


def test_colsum_refuses_65_batches_with_nothing_launched(L):
    x = D(X.ints(65 * 4, 8, seed=1))
    buf = out_like(65, 8, dtype=F32)
    assert L.sdxl_op_colsum(ptr(x), 8, ptr(buf), 8, 65, 4, 8, stream()) != 0
    assert L.sdxl_op_colsum(ptr(x), 8, ptr(buf), 8, 0, 4, 8, stream()) != 0
    torch.cuda.synchronize()
    assert bool((buf == SENTINEL).all())


def test_colsum_reads_and_writes_its_operands_only(L):
    c = T.ISOLATION_COLSUM
    x, pre = cached(("cs", c, False), lambda: T.colsum_operands(c, False))
    specs = [_I("x", x, c.N + 8), _I("out", pre[:, :c.N], c.N + T.COLSUM_PAD, dtype=F32, role="inout")]

    def fn(ar):
        lib.check(L.sdxl_op_colsum(_P(ar, "x"), ar.ld("x"), _P(ar, "out"), ar.ld("out"), c.batches, c.rows, c.N, stream()))
    runs = run_isolated(fn, specs, device="cuda")
    assert_isolated(runs, what="colsum")


# ------------------------------------------------------------------------------------------------ reductions shorter than a K block, chained
def test_colsum_cast_and_batch_long_weight_gradient_chain(L):
    """what the backward does for the time-embedding projection of one resnet: per-sample column sums of dy (fp32, into the gradient arena),
    the cast to bf16, and the TN launch whose reduction is the batch (K = B = 4).  Integers: |sum| <= 2 x 77 < 256 is bf16-exact, so the
    weight gradient is an exact integer matrix."""
    from oracle import unet_ref as U
    from sdxl_amd import unet as NU
    from test_gpu_model import tiny_native_cfg
    B, rows, Cout, E = 4, 77, 128, 320
    dy, emb = X.ints(B * rows, Cout, seed=301), X.ints(B, E, seed=302)
    sums = dy.double().view(B, rows, Cout).sum(1)
    assert float(sums.abs().max()) < 256
    print(f"[temb] chain: TN 128x320x4 route {X.route_of(lib, L, 1, form=2, M=Cout, N=E, K=B, bias_grad=1)}")
    net = NU.NativeUNet(tiny_native_cfg(U.tiny_config()))
    try:
        assert net.grads.numel() >= B * Cout
        net.grads[: B * Cout].zero_()
        dyd, embd = D(dy), D(emb)
        lib.check(L.sdxl_op_colsum(ptr(dyd), Cout, ptr(net.grads), Cout, B, rows, Cout, stream()))
        X.assert_exact("chain: column sums", net.grads[: B * Cout].view(B, Cout), X.expect(sums, False))
        dtp = out_like(B, Cout)
        lib.check(L.sdxl_grads_to_bf16(net.h, 0, B * Cout, ptr(dtp), 1.0, stream()))
        X.assert_exact("chain: cast", dtp, X.expect(sums, True))
        dw = out_like(Cout, E, dtype=F32)
        db = torch.zeros(Cout, dtype=F32, device=dev())
        lib.check(L.sdxl_op_gemm(2, ptr(dtp), ptr(embd), ptr(dw), Cout, E, B, ptr(db), None, 0, 0, stream()))
        X.assert_exact("chain: weight gradient", dw, X.expect(sums.T @ emb.double() + 0.0, False))      # (+ 0.0: the accumulator starts at +0)
        X.assert_exact("chain: bias gradient", db, X.expect(sums.sum(0), False))
    finally:
        net.close()


# ------------------------------------------------------------------------------------------------ the sinusoidal embedding
@pytest.mark.parametrize("gap", [0, 8], ids=["dense", "ldo+8"])
@pytest.mark.parametrize("rows", T.SINCOS_ROWS)
@pytest.mark.parametrize("dim", T.SINCOS_DIMS)
def test_sincos_against_float64(L, dim, rows, gap):
    """every timestep of the table at every width (the 1- and 4-row launches walk the table in several calls), the ldo gap pattern-filled and checked"""
    ldo = dim + gap
    worst = 0.0
    for off in range(0, len(T.SINCOS_T), rows):
        t = T.sincos_timesteps(rows, off)
        ref, delta = T.sincos_ref(t, dim)
        out = out_like(rows, ldo)
        td = t.to(dev())
        lib.check(L.sdxl_op_sincos(ptr(td), ptr(out), rows, dim, ldo, stream()))
        got = out.cpu()
        worst = max(worst, NL.check_interval(f"sincos dim {dim} rows {rows} ldo {ldo} t[{off}:]", got[:, :dim].contiguous(), ref, delta))
        assert bool((got[:, dim:] == SENTINEL).all()), "the gap of a row was written"
    print(f"[temb] sincos dim {dim} rows {rows} ldo {ldo}: largest share of delta used {worst:.3f}")


# ------------------------------------------------------------------------------------------------ the engine's own ldv, col0, rows_per_batch
def test_tiny_unet_sample_0_does_not_see_sample_1s_timestep_and_time_ids():
    """Inference forward at B = 2 on 52 x 40 latents (the deepest level is 13 x 10: rows_per_batch = 130 against 128-row tiles; the levels
    above have 520 and 2080 rows per sample), distinct timesteps and time ids per sample.  Changing ONLY sample 1's leaves every bit of sample
    0's prediction and changes sample 1's: the engine's own grouped projection, column slices and rows_per_batch, which the hooks restate."""
    from oracle import unet_ref as U
    from sdxl_amd import unet as NU
    from test_gpu_model import make_inputs, tiny_native_cfg
    cfg = U.tiny_config()
    net = NU.NativeUNet(tiny_native_cfg(cfg))
    try:
        net.load_state_dict(U.synth_weights(cfg, seed=0))
        B, H, W = 2, 52, 40
        x = make_inputs(cfg, B, H, W, seed=11)
        tid = torch.tensor([[416.0, 320, 0, 0, 416, 320], [1024.0, 768, 16, 32, 1344, 768]])
        t = torch.tensor([17.0, 650.0])
        a = net.unet_forward(x["lat"], t, x["ehs"], x["pooled"], tid).cpu()
        tid2, t2 = tid.clone(), t.clone()
        tid2[1], t2[1] = torch.tensor([512.0, 2048, 8, 0, 768, 1536]), 987.654
        b = net.unet_forward(x["lat"], t2, x["ehs"], x["pooled"], tid2).cpu()
        assert bool(torch.isfinite(a).all()) and bool(torch.isfinite(b).all())
        assert X.same_bits(a[0], b[0]), f"sample 0 moved in {int((a[0] != b[0]).sum())} of {a[0].numel()} elements"
        moved = float((a[1] != b[1]).double().mean())
        print(f"[temb] tiny unet: sample 0 bit-equal, sample 1 moved in {100 * moved:.1f} % of its elements")
        assert moved > 0.5
    finally:
        net.close()
