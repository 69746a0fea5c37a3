"""Per-element checks for the time-embedding path: the row-vector epilogue of the GEMM family (conv1 of every resnet adds the sample's projected
embedding in the launch that adds bias and residual), the column sums that carry its gradient back, the weight gradients whose reduction is the
batch, and the sinusoidal embedding.  tests/test_gpu_ops_temb.py runs them on the device; tests/test_host_temb.py shows on the CPU that they see
what a per-tensor rel-L2 / cosine lets through.  Built on tests/_exact.py (integer operands, one rounding, the a-priori bound, the route hook)
and tests/_nonlinear.py (the interval test of a bf16 output against a float64 reference with a derived delta).  No GPU needed here.

1. Row vector.  Operands {-2 .. 2}, bias {-8 .. 8}, rowvec[b][n] = 32 (b % 7 + 1) + r, r in {-8 .. 8} (sample_vectors: = 32 (b + 1) + r up to
   seven samples; bf16-exact): a neighbouring sample's vector is off by at least 16 in every column, so a row that takes its neighbour's
   vector changes its integer.  The vector is ALWAYS a column slice of a wider matrix (ldv = 2 N + 64, first column N + 64) whose
   other columns are NaN.  The expected output is the integer sum rounded once.
2. Column sums.  Integers {-2 .. 2}: every partial sum is an integer below 2^24, the result is exact in any order.  randn: the a-priori bound
   (rows - 1) 2^-24 sum|x| per column, plus the one rounding of the add onto the prefilled output.
3. Sinusoidal embedding.  float64 reference, delta accumulated next to it (sincos_ref)."""
from __future__ import annotations

import math
from collections import namedtuple

import torch

import _exact as X
import _nonlinear as NL

BF = torch.bfloat16
NAN = float("nan")
MODEL_BAR = (6e-2, 0.995)      # the tiny UNet's per-tensor bar (tests/test_gpu_model.py: rel-L2, cosine): what the model tests hold this path to


def per_tensor(got, ref):
    """(rel-L2, cosine) of a whole tensor: the model tests' number"""
    g, r = got.double().flatten(), ref.double().flatten()
    return float((g - r).norm() / r.norm().clamp_min(1e-300)), float(torch.nn.functional.cosine_similarity(g, r, dim=0))


def passes_model_bar(got, ref):
    rel, cos = per_tensor(got, ref)
    return rel <= MODEL_BAR[0] and cos >= MODEL_BAR[1]


# ------------------------------------------------------------------------------------------------ 1. the row-vector epilogue
RV = namedtuple("RV", "B rpb N K splitk", defaults=(1,))
ROWVEC_CASES = [
    RV(4, 77, 160, 64),            # two sample boundaries inside the first 128-row tile; N = 160: the 4-column branch of store_bf16 runs (below)
    RV(4, 77, 200, 128),           # ragged N
    RV(3, 130, 128, 64),           # a boundary two rows past a tile edge
    RV(1, 300, 128, 64),           # one sample
    RV(37, 1, 128, 64),            # every row has its own vector
    RV(2, 988, 320, 64),           # a whole tile in the middle of one sample
    RV(4, 77, 640, 2048, 4),       # the slab epilogue (splitk_epilogue_kernel)
]
ROWVEC_G256 = RV(4, 130, 256, 64)                                # the 256 x 256 mode: M = 520 is no whole number of 256-row tiles, see ROWVEC_G256_WHOLE
ROWVEC_G256_WHOLE = RV(4, 192, 256, 64)                          # M = 768: three whole tiles, boundaries at rows 192, 384 (mid-tile), 576
ROWVEC_CR256 = [RV(4, 130, 160, 64), RV(4, 130, 320, 128)]      # the co-resident kernel's shapes
ISOLATION_DENSE = RV(2, 130, 128, 64)
# store_bf16 (csrc/gemm.hip, csrc/gemm_cr256.hip) stores 8 columns per lane, and 4 for the LAST 16-column fragment of each half of a 160-column
# tile (NJ odd): tile columns 64 .. 79 and 144 .. 159.  A 160-column tile needs N % 160 == 0 (gemm_route_cfg128: configurations 3, 13, 23; cr256
# modes 31, 36).  So N = 160 / 320 / 640 run both branches with a vector, N = 128 / 200 / 256 the 8-column one only.
def store_branches(route, N):
    wide = (route["kernel"] == "128-row" and route["cfg"] in (3, 13, 23, 5)) or (route["kernel"] == "cr256" and route["cfg"] in (31, 33, 36))
    if route["post"] == "splitk_epilogue":
        return "slab epilogue (8 columns)"
    return "8- and 4-column stores" if wide and N % 160 == 0 else "8-column stores"


# what tests/test_host_temb.py's scan of every mode word finds for a row-vector NT problem, per case: {(kernel, cfg)} reachable by a forced
# configuration of THIS launch (the hook's cfg argument).  The GPU file runs the policy and every entry; the host test holds this table to the scan.
FORCE_128 = (1, 2, 3, 13, 23)
FORCE_CR256 = (31, 32, 35, 36)
FORCE_CR256_DIAG = (33, 34)
PIPELINED = (7, 8)            # refuse a row vector (pl_applicable): must fall back, never drop the vector
STREAM_K_WORKERS = (1, 7, 37)
ROWVEC_SK = RV(4, 192, 256, 640)      # stream-K takes whole 256 x 256 tiles: 3 tiles x 10 K-steps, sample boundaries inside tiles 0 and 2
# 5 / 6: the pipelined loop of the 128-row kernel (160- / 128-column tiles), the same epilogue source as 3 / 1
_N160, _N128 = (1, 2, 3, 5, 6, 13, 23), (1, 2, 6)
ROWVEC_FORCED = {
    ROWVEC_CASES[0]: _N160,
    ROWVEC_CASES[1]: _N128,                      # (M = 308, 390, 300, 37: M % 8 keeps the co-resident kernel away)
    ROWVEC_CASES[2]: _N128,
    ROWVEC_CASES[3]: _N128,
    ROWVEC_CASES[4]: _N128,
    ROWVEC_CASES[5]: _N160 + FORCE_CR256,
    ROWVEC_CASES[6]: (13,),                      # a split launch keeps the policy's tile: every other word falls back to it
    ROWVEC_G256: _N128 + FORCE_CR256,
    ROWVEC_G256_WHOLE: _N128 + FORCE_CR256,
    ROWVEC_CR256[0]: _N160 + FORCE_CR256,
    ROWVEC_CR256[1]: _N160 + FORCE_CR256,
}
# configuration 43 (diagnostics build only: a four-wave form that was measured once and never selected) is left out as tests/_nonlinear.py's
# GEGLU_NOT_COVERED leaves it out; it shares the epilogue source with 1 / 3 / 13 / 23
ROWVEC_NOT_COVERED = (43,)


def rv_desc(c, cfg=0):
    return dict(form=0, M=c.B * c.rpb, N=c.N, K=c.K, splitk=c.splitk, cfg=cfg, rowvec=1)


def rv_route(lib, L, c, mode=1, cfg=0):
    return X.route_of(lib, L, mode, **rv_desc(c, cfg))


def rv_scan(lib, L, c):
    """{cfg: route} for every per-launch configuration 1 .. 63 that changes nothing else: the words sdxl_set_gemm_mode accepts"""
    out = {}
    for cfg in range(1, 64):
        try:
            lib.check(L.sdxl_set_gemm_mode(1 + 4 * cfg))
        except Exception:
            continue      # not a mode word of this build
        finally:
            lib.check(L.sdxl_set_gemm_mode(1))
        out[cfg] = rv_route(lib, L, c, cfg=cfg)
    return out


def rv_forced(lib, L, c):
    """the forced launches of one case on the GPU: [(cfg, route)] with one entry per distinct (kernel, cfg) the scan reaches that is not a mere
    fall-back to what configuration 1 gives"""
    scan = rv_scan(lib, L, c)
    seen, out = set(), []
    for cfg, r in sorted(scan.items()):
        key = (r["kernel"], r["cfg"])
        if r["cfg"] != cfg or key in seen:      # refused for this shape: the route is another configuration's
            continue
        seen.add(key)
        out.append((cfg, r))
    return out


def sample_vectors(B, N, seed):
    """vec[b][n] = 32 (b % 7 + 1) + r, r in {-8 .. 8}: integers of at most 232, which bf16 holds as they are (from 256 on it holds even integers
    only, and a vector of 32 x 38 would push the outputs into binades where the even residual makes too few ties).  Neighbouring samples differ
    by at least 16 in every column; samples seven apart differ by their r."""
    return 32.0 * (torch.arange(B).float()[:, None] % 7 + 1) + X.ints(B, N, seed=seed, lo=-8, hi=8)


def rv_operands(c, integer, seed=0):
    """CPU float32 operands of one case (bf16-exact): a [M][K], w [N][K], bias [N], resid [M][N], vec [B][N], and the wide matrix
    [B][2 N + 64] that holds vec at column N + 64 and NaN elsewhere"""
    M, s = c.B * c.rpb, 5000 + 1000 * seed
    if integer:
        a, w = X.ints(M, c.K, seed=s + 1), X.ints(c.N, c.K, seed=s + 2)
        bias, resid = X.bias_ints(c.N, s + 3), X.resid_even(M, c.N, seed=s + 4)
        vec = sample_vectors(c.B, c.N, s + 5)
    else:
        a, w = X.rnd(M, c.K, seed=s + 1), X.rnd(c.N, c.K, seed=s + 2, scale=c.K ** -0.5)
        bias, resid, vec = X.rnd(c.N, seed=s + 3), X.rnd(M, c.N, seed=s + 4), X.rnd(c.B, c.N, seed=s + 5)
    return dict(a=a, w=w, bias=bias, resid=resid, vec=vec, wide=widen(vec))


def ldv_of(N):
    return 2 * N + 64


def col0_of(N):
    return N + 64


def widen(vec, fill=NAN):
    B, N = vec.shape
    wide = torch.full((B, ldv_of(N)), fill)
    wide[:, col0_of(N): col0_of(N) + N] = vec
    return wide


def rv_ref64(o, rpb, resid, vec=None):
    """(float64 result, |A| . |B| + |bias| (+ |resid|), |rowvec| per row): the last joins the other addends in rv_bound"""
    d = {k: v.double() for k, v in o.items() if k != "wide"}
    v = (d["vec"] if vec is None else vec.double()).repeat_interleave(rpb, 0)
    ref = d["a"] @ d["w"].T + d["bias"] + v
    ab = d["a"].abs() @ d["w"].abs().T + d["bias"].abs()
    if resid:
        ref, ab = ref + d["resid"], ab + d["resid"].abs()
    return ref, ab, v.abs()


def rv_bound(ref, ab, vabs, K):
    """X.bound with |rowvec| joined to |bias| + |resid|: one more addend of the same fp32 sum, so it enters at the same K 2^-23 factor"""
    return X.bound(ref, ab, K, True, extra=K * 2.0 ** -23 * vabs)


# ---- through the convolution
CV = namedtuple("CV", "B H W Cin Cout")
CONV_CASES = [CV(2, 13, 10, 32, 128),       # no split (Cin % 64), a boundary at row 130
              CV(4, 8, 8, 64, 128),         # the plan splits it (asserted in the host test)
              CV(2, 16, 20, 64, 256)]       # under the policy and with the 256 x 256 mode / the co-resident configurations asked for
CONV_MODES = {CV(2, 16, 20, 64, 256): (2, 4 * 31, 4 * 32, 4 * 35, 4 * 36)}
ISOLATION_CONV = CV(2, 13, 10, 32, 128)


def conv_rv_desc(c):
    sk = X.conv_fwd_dgrad_splitk("fwd", c.B, c.H, c.W, c.Cin, c.Cout, 1)
    return dict(X.conv_desc("fwd", c.B, c.H, c.W, c.Cin, c.Cout, 1, sk), rowvec=1)


def conv_rv_operands(c, integer, seed=0):
    s = 7000 + 100 * seed
    if integer:
        x, w, bias = X.ints(c.B, c.H, c.W, c.Cin, seed=s + 1), X.ints(c.Cout, 9, c.Cin, seed=s + 2), X.bias_ints(c.Cout, s + 3)
        vec = sample_vectors(c.B, c.Cout, s + 5)
    else:
        x, w = X.rnd(c.B, c.H, c.W, c.Cin, seed=s + 1), X.rnd(c.Cout, 9, c.Cin, seed=s + 2, scale=(9 * c.Cin) ** -0.5)
        bias, vec = X.rnd(c.Cout, seed=s + 3), X.rnd(c.B, c.Cout, seed=s + 5)
    return dict(x=x, w=w, bias=bias, vec=vec, wide=widen(vec))


def conv_rv_ref64(o):
    """(float64 result [B][H][W][Cout], |x| * |w| + |bias|, |rowvec|): the borders counted tap by tap by conv2d's zero padding (X.conv_ref64)"""
    v = o["vec"].double()[:, None, None, :]
    ref = X.conv_ref64(o["x"], o["w"], o["bias"], 1) + v
    ab = X.conv_ref64(o["x"].abs(), o["w"].abs(), o["bias"].abs(), 1)
    return ref, ab, v.abs().expand_as(ref)


# ---- the mutants of the epilogue (CPU: what a wrong kernel would write, on the same operands)
def rv_mutant(name, o, c, resid=True):
    acc = (o["a"] @ o["w"].T + o["bias"] + (o["resid"] if resid else 0.0)).double()      # integers: exact in fp32
    M = c.B * c.rpb
    rows = torch.arange(M)
    v = o["vec"].double()
    if name == "tile's first row decides":
        return X.bf16_rn(acc + v[(rows // 128 * 128) // c.rpb])
    if name == "added after the rounding":
        return X.bf16_rn(X.bf16_rn(acc).double() + v[rows // c.rpb])
    if name == "dropped in the last 4 columns":
        vv = v[rows // c.rpb].clone()
        vv[:, -4:] = 0.0
        return X.bf16_rn(acc + vv)
    if name == "read at column 0":
        wide = widen(o["vec"], 0.0)
        wide[:, :c.N] = torch.roll(o["vec"], 3, 1)      # (the engine's matrix holds other layers' vectors there, not NaN: the same numbers, moved)
        return X.bf16_rn(acc + wide[:, :c.N].double()[rows // c.rpb])
    raise KeyError(name)


RV_MUTANTS = ("tile's first row decides", "added after the rounding", "dropped in the last 4 columns", "read at column 0")


# ------------------------------------------------------------------------------------------------ 2. column sums
CS = namedtuple("CS", "batches rows N ld_out_zero", defaults=(False,))
COLSUM_CASES = [CS(1, 1, 8), CS(1, 37, 8), CS(2, 130, 128), CS(4, 77, 320), CS(4, 988, 640), CS(64, 33, 8), CS(1, 4096, 1280, True)]
COLSUM_BATCHED_BRANCH = {CS(2, 130, 128): True, CS(4, 77, 320): False, CS(4, 988, 640): True}
COLSUM_MAX_BATCHES = 64      # LN_RED_MAX (csrc/kernels.h)
COLSUM_COL0, COLSUM_PAD = 64, 128
ISOLATION_COLSUM = CS(2, 130, 128)


def colsum_geom(batches, rows, N):
    """(column blocks, row chunks per batch, rows per chunk, batched branch taken): col_reduce_geom + colsum_geom of csrc/norm.hip restated"""
    cdiv = lambda a, b: -(-a // b)
    colblocks = cdiv(N, 256)
    chunks = min(max(1024 // colblocks, 1), cdiv(rows, 32))
    rpc = cdiv(rows, chunks)
    y = cdiv(rows, rpc)
    taken = batches > 1 and y >= 2 * batches
    if taken:
        rpc *= batches
        y = cdiv(rows, rpc)
    return colblocks, y, rpc, taken


def colsum_operands(c, integer, seed=0):
    """x [batches * rows][N] (bf16-exact) and the prefilled output buffer [batches][N + 128] of small integers"""
    s = 9000 + 10 * seed
    x = X.ints(c.batches * c.rows, c.N, seed=s + 1) if integer else X.rnd(c.batches * c.rows, c.N, seed=s + 1)
    pre = X.ints(c.batches, c.N + COLSUM_PAD, seed=s + 2, lo=-8, hi=8)
    return x, pre


def colsum_ref64(c, x, pre):
    """(the buffer after the call, sum|x| per output) in float64: the slice at column 64 holds prefill + sum, the rest the prefill"""
    xs = x.double().view(c.batches, c.rows, c.N)
    want = pre.double().clone()
    want[:, COLSUM_COL0: COLSUM_COL0 + c.N] += xs.sum(1)
    return want, xs.abs().sum(1)


def colsum_bound(c, sabs, want_slice):
    """(rows - 1) 2^-24 sum|x|: fp32 adds of `rows` bf16 values in any order; + 2^-24 |result|: the one rounding of the add onto the prefill"""
    return (c.rows - 1) * 2.0 ** -24 * sabs + 2.0 ** -24 * want_slice.abs()


# ------------------------------------------------------------------------------------------------ 3. the sinusoidal embedding
SINCOS_DIMS = (32, 64, 256, 320)
SINCOS_ROWS = (1, 4, 24)
SINCOS_T = (0.0, 1e-3, 0.25, 1.0, 17.0, 104.0, 333.3, 500.0, 650.0, 750.0, 768.0, 987.654, 999.0, 1024.0, 1344.0, 1536.0, 2048.0)
LN1E4_F32 = float(torch.tensor(9.210340371976184, dtype=torch.float32))      # the kernel's constant as fp32 holds it
# expf, cosf, sinf are library functions here (csrc/elementwise.hip calls them by name, no fast-math).  The HIP math documentation with their
# ulp table is not among this tree's sources, so the OpenCL full-profile bounds are used: exp <= 3 ulp, sin / cos <= 4 ulp.  1 ulp <= 2^-23 |result|.
ULP_EXP, ULP_SINCOS = 3, 4
U = NL.U


def sincos_timesteps(rows, offset=0):
    """`rows` timesteps from the table (as fp32), starting at `offset`"""
    return torch.tensor([SINCOS_T[(offset + i) % len(SINCOS_T)] for i in range(rows)], dtype=torch.float32)


def sincos_ref(t32, dim):
    """(ref [rows][dim] float64, delta): cat[cos, sin](t exp(-ln 1e4 k / half)) with t the fp32 input as it is.  delta, operation by operation:
         x = c k / half     c = fp32(ln 1e4) (U relative), one product, one correctly rounded division: |dx| <= 3 U |x|
         f = expf(x)        relative error |dx| (first order: d e^x = e^x dx) + ULP_EXP 2^-23
         a = t f            one product: relative error rel(f) + U, absolute |a| (rel(f) + U)
         cosf(a), sinf(a)   |d cos|, |d sin| <= |da|, + ULP_SINCOS 2^-23 |result|"""
    half = dim // 2
    k = torch.arange(half, dtype=torch.float64)
    x = math.log(1e4) * k / half
    f = torch.exp(-x)
    rel_f = 3 * U * x + ULP_EXP * 2 * U
    a = t32.double()[:, None] * f[None, :]
    da = a.abs() * (rel_f + U)[None, :]
    ref = torch.cat([torch.cos(a), torch.sin(a)], 1)
    delta = torch.cat([da, da], 1) + ULP_SINCOS * 2 * U * ref.abs()
    return ref, delta


def sincos_f32(t32, dim, mutant=None):
    """the kernel's formula restated in fp32 torch (csrc/elementwise.hip, sincos_kernel), and its mutants"""
    half = dim // 2
    k = torch.arange(half, dtype=torch.float32)
    den = {"half - 1": float(half - 1), "dim": float(dim)}.get(mutant, float(half))
    f = torch.exp(-torch.tensor(LN1E4_F32) * k / torch.tensor(den))
    a = t32[:, None] * f[None, :]
    if mutant == "bf16 argument":
        a = a.to(BF).float()
    c, s = torch.cos(a), torch.sin(a)
    return torch.cat([s, c] if mutant == "sin first" else [c, s], 1)


SINCOS_MUTANTS = ("sin first", "half - 1", "dim", "bf16 argument")
