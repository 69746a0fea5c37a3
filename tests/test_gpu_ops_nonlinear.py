"""Per-element parity of the NON-LINEAR kernels on a real MI355X: GroupNorm (+ SiLU) and LayerNorm, forward and backward, the SiLU pair over
every bf16 argument, the GEGLU epilogues over every bf16 gate on every route that has one, and attention with a peaked softmax
(tests/_nonlinear.py; shown to see what it claims on the CPU in tests/test_host_nonlinear.py).
tests/test_gpu_ops.py asserts one number per tensor against fp32 torch; here every case asserts, with no element left out,

  * bf16 outputs:  bf16_rn(ref - delta) <= got <= bf16_rn(ref + delta) against float64 on the CPU, delta the bound on the fp32 value the
    kernel rounds, accumulated operation by operation next to the reference (the derivations are the docstrings of gn_stats_ref, gn_fwd_ref,
    gn_bwd_ref, ln_fwd_ref, ln_bwd_ref, silu_delta, silu_grad_delta: 2^-24 per fp32 operation, 2^-22 per hardware exp / rsq,
    (N - 1) 2^-24 sum|terms| for a sum of N terms in any order) -- the final rounding gets no slack;
  * fp32 outputs (the stored statistics, dgamma, dbeta):  |got - ref| <= delta + 2^-24 |ref|;
  * on TWO-POINT data (x = K + s r per group / row, r = +-1 balanced exactly) GroupNorm's shifted sums are exact whatever the chunking:
    the stored mean equals K bit for bit, rstd is within 2 fp32 ulp of (s^2 + eps)^-1/2 (one rounded sum, one 1-ulp instruction);
    LayerNorm's first pass is exact too, its mean K up to the rounded 1 / C (exactly K where C is a power of two);
  * with mean = K, rstd = 1 passed in, s = 1 and integer dy the parameter gradients are integer sums: bit equality.
The backward takes its statistics from the float64 reference rounded to fp32, not from the forward kernel: the two are tested apart.
GEGLU: the cdf's absolute error cannot be derived; it is measured on the CPU (NL.CDF_ERR_MEASURED, 2.3e-7 over every finite bf16 gate) and
doubled; the bounds are geglu_fwd_ref / geglu_bwd_ref.  Attention: attn_run states its reference and bounds, and every case prints which backward it reaches.
Each case prints its figures as `[nonlinear] ...` lines (profiles/ops_nonlinear.txt keeps them)."""
import ctypes as C

import pytest
import torch

import sdxl_amd  # noqa: F401
from sdxl_amd import lib

import _nonlinear as NL

pytestmark = pytest.mark.gpu
BF, F32 = torch.bfloat16, torch.float32
SENTINEL = 7777.0      # what outputs hold before a launch that must overwrite them
EPS = 1e-5


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


def zeros(*shape):
    return torch.zeros(shape, dtype=F32, device=dev())


def knob(L, kid, value):
    lib.check(L.sdxl_set_knob(kid, value))


_CACHE = {}


def cached(key, make):
    """a reference is computed once, shared by every case that needs it, and never modified"""
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


# ------------------------------------------------------------------------------------------------ GroupNorm
#   (B, HW, C, G)                what it reaches
GN_CASES = [(2, 64, 64, 32),     # cpg 2, one chunk
            (2, 100, 320, 32),   # cpg 10: a thread's 8-channel vector straddles two groups; two ragged chunks
            (2, 50, 960, 32),    # cpg 30
            (2, 144, 1920, 32),  # cpg 60
            (1, 600, 2560, 32),  # cpg 80; 75 chunks: gn_finalize_kernel's 64-lane loop wraps; 12 slices in gn_bwd_group_kernel
            (1, 64, 2048, 16)]   # cpg 128: the backward's argument limit
GN_CLAMP = (1, 2100, 2560, 32)   # 2100 / 8 = 262 chunks asked for: the GN_MAX_CHUNKS clamp (two-point data only)


def gn_ws(B, C, G):
    return torch.empty(256 * B * C * 2 + 256 * B * G * 2 + B * C * 5, dtype=F32, device=dev())


def gn_fwd(L, x, gamma, beta, G, silu):
    B, HW, Cc = x.shape
    y, stats = out_like(B, HW, Cc), out_like(B, G, 2, dtype=F32)
    xd, gd, bd, ws = D(x), D(gamma), D(beta), gn_ws(B, Cc, G)
    lib.check(L.sdxl_op_groupnorm_fwd(ptr(xd), ptr(y), ptr(gd), ptr(bd), ptr(stats), ptr(ws), B, HW, Cc, G, EPS, silu, stream()))
    torch.cuda.synchronize()
    return y, stats


def gn_bwd(L, x, dy, gamma, beta, stats, G, silu, addend=None):
    """(dx, dgamma, dbeta); addend: accumulate = 1 onto it (the op reads it from dx)"""
    B, HW, Cc = x.shape
    dx = out_like(B, HW, Cc) if addend is None else D(addend)
    dg, db = zeros(Cc), zeros(Cc)
    xd, dyd, gd, bd, sd, ws = D(x), D(dy), D(gamma), D(beta), stats.to(dev()).contiguous(), gn_ws(B, Cc, G)
    lib.check(L.sdxl_op_groupnorm_bwd(ptr(xd), ptr(dyd), ptr(gd), ptr(bd), ptr(sd), ptr(dx), ptr(dg), ptr(db), ptr(ws), B, HW, Cc, G, silu,
                                      int(addend is not None), stream()))
    torch.cuda.synchronize()
    return dx, dg, db


def gn_two_point_fwd(L, B, HW, Cc, G, silu):
    tag = f"groupnorm two-point B{B} HW{HW} C{Cc} G{G} silu{silu}"
    x, K, s = cached(("gn2p", B, HW, Cc, G), lambda: NL.gn_two_point(B, HW, Cc, G, 7))
    gamma, beta = NL.affine(Cc, 41)
    r = cached(("gn2p ref", B, HW, Cc, G, silu), lambda: NL.gn_fwd_ref(x, gamma, beta, G, EPS, silu, exact_sums=True))
    y, stats = gn_fwd(L, x, gamma, beta, G, silu)
    NL.check_bits(f"{tag} mean", stats[..., 0].cpu(), K)
    NL.check_ulps(f"{tag} rstd", stats[..., 1], (s.double() ** 2 + EPS).rsqrt(), 2)
    NL.check_interval(f"{tag} y", y, r["y"], r["dy"])


def gn_exact_params(L, B, HW, Cc, G):
    """mean = K, rstd = 1 passed in, s = 1, integer dy, no activation: dbeta and dgamma are integer sums"""
    x, K, _ = NL.gn_two_point(B, HW, Cc, G, 5, s=1.0)
    dy = NL.ints(B, HW, Cc, seed=6)
    stats = torch.stack([K, torch.ones_like(K)], -1).float().contiguous()
    xh = x.double() - NL._per_channel(K.double(), Cc)
    _, dg, db = gn_bwd(L, x, dy, torch.ones(Cc), torch.zeros(Cc), stats, G, 0)
    NL.check_bits(f"groupnorm exact dgamma B{B} HW{HW} C{Cc} G{G}", dg, (dy.double() * xh).sum((0, 1)).float())
    NL.check_bits(f"groupnorm exact dbeta B{B} HW{HW} C{Cc} G{G}", db, dy.double().sum((0, 1)).float())


def gn_graded_refs(B, HW, Cc, G, silu):
    def make():
        x = NL.gn_graded(B, HW, Cc, G, 11)
        gamma, beta = NL.affine(Cc, 41)
        f = NL.gn_fwd_ref(x, gamma, beta, G, EPS, silu)
        stats = NL.stats_f32(f)
        dy, addend = NL.rnd(B, HW, Cc, seed=43), NL.rnd(B, HW, Cc, seed=44)
        return x, gamma, beta, f, stats, dy, addend, [NL.gn_bwd_ref(x, dy, gamma, beta, stats, G, silu, a) for a in (None, addend)]
    return cached(("gn graded", B, HW, Cc, G, silu), make)


def gn_graded_bwd(L, B, HW, Cc, G, silu, tag):
    x, gamma, beta, _, stats, dy, addend, refs = gn_graded_refs(B, HW, Cc, G, silu)
    for a, b in zip((None, addend), refs):
        t = f"{tag} accumulate {int(a is not None)}"
        dx, dg, db = gn_bwd(L, x, dy, gamma, beta, stats, G, silu, a)
        NL.check_interval(f"{t} dx", dx, b["dx"], b["ddx"])
        NL.check_f32(f"{t} dgamma", dg, b["dgamma"], b["ddgamma"])
        NL.check_f32(f"{t} dbeta", db, b["dbeta"], b["ddbeta"])


@pytest.mark.parametrize("silu", [0, 1])
@pytest.mark.parametrize("B,HW,Cc,G", GN_CASES)
def test_groupnorm_forward(L, B, HW, Cc, G, silu):
    """y and the stored (mean, rstd): two-point data (exact statistics), then graded randn (no two groups or samples share statistics) with a
    +-2^-9 group (variance below eps) and a constant group (variance 0: y = act(beta) within delta).  Derivations: gn_stats_ref, gn_fwd_ref."""
    gn_two_point_fwd(L, B, HW, Cc, G, silu)
    tag = f"groupnorm graded B{B} HW{HW} C{Cc} G{G} silu{silu}"
    x, gamma, beta, r, *_ = gn_graded_refs(B, HW, Cc, G, silu)
    y, stats = gn_fwd(L, x, gamma, beta, G, silu)
    NL.check_f32(f"{tag} mean", stats[..., 0], r["mean"], r["dmean"])
    NL.check_f32(f"{tag} rstd", stats[..., 1], r["rstd"], r["drstd"])
    NL.check_interval(f"{tag} y", y, r["y"], r["dy"])


@pytest.mark.parametrize("silu", [0, 1])
@pytest.mark.parametrize("B,HW,Cc,G", GN_CASES)
def test_groupnorm_backward(L, B, HW, Cc, G, silu):
    """dx (accumulate 0 and 1: gn_bwd_apply_kernel<*, false | true>), dgamma, dbeta from the reference's statistics on graded randn, and the
    exact integer parameter gradients.  Derivation: gn_bwd_ref."""
    gn_graded_bwd(L, B, HW, Cc, G, silu, f"groupnorm graded B{B} HW{HW} C{Cc} G{G} silu{silu}")
    if not silu:
        gn_exact_params(L, B, HW, Cc, G)


@pytest.mark.parametrize("silu", [0, 1])
def test_groupnorm_chunk_clamp(L, silu):
    """(1, 2100, 2560): the row chunks are clamped to GN_MAX_CHUNKS; the exact designs only (a sum of 168 000 terms has no useful bound)"""
    gn_two_point_fwd(L, *GN_CLAMP, silu)
    if not silu:
        gn_exact_params(L, *GN_CLAMP)


@pytest.mark.diag
@pytest.mark.parametrize("silu", [0, 1])
@pytest.mark.parametrize("B,HW,Cc,G", GN_CASES)
def test_groupnorm_backward_lds_free_reduce(L, B, HW, Cc, G, silu):
    """knob 24 = 1: gn_bwd_reduce_nolds_kernel (row lanes folded by an xor tree) in place of the LDS reduce"""
    knob(L, 24, 1)
    try:
        gn_graded_bwd(L, B, HW, Cc, G, silu, f"groupnorm LDS-free graded B{B} HW{HW} C{Cc} G{G} silu{silu}")
        if not silu:
            gn_exact_params(L, B, HW, Cc, G)
    finally:
        knob(L, 24, 0)


def test_groupnorm_large_offset_per_element(L):
    """tests/test_gpu_ops.py's 2e4-offset case (x = 2e4 + 50 randn in bf16: multiples of 128, |mean| >> std) under the per-element check"""
    B, HW, Cc, G = 1, 512, 320, 32
    x = (NL.rnd(B, HW, Cc, seed=44) * 50.0 + 2.0e4).to(BF).float()
    gamma, beta = torch.ones(Cc), torch.zeros(Cc)
    r = NL.gn_fwd_ref(x, gamma, beta, G, EPS, 0)
    y, stats = gn_fwd(L, x, gamma, beta, G, 0)
    NL.check_f32("groupnorm offset 2e4 mean", stats[..., 0], r["mean"], r["dmean"])
    NL.check_f32("groupnorm offset 2e4 rstd", stats[..., 1], r["rstd"], r["drstd"])
    NL.check_interval("groupnorm offset 2e4 y", y, r["y"], r["dy"])


# ------------------------------------------------------------------------------------------------ the SiLU pair over every bf16 argument
def test_silu_sweep_through_groupnorm_forward(L):
    """gamma = 0: a = rstd 0 = 0, s = beta - mean 0 = beta, n = x 0 + beta = beta EXACTLY, so y = bf16(silu_f(beta[c])) in every row.  beta
    carries every finite bf16 value with |n| <= 128 and +-1e4, +-3e38, 4096 channels a launch.  Derivation: silu_delta (no argument error)."""
    sweep = NL.bf16_sweep(128.0, NL.SILU_EXTREMES)
    Cc, G, HW = 4096, 32, 8
    x, _, _ = NL.gn_two_point(1, HW, Cc, G, 3)
    worst = 0.0
    for i, c0 in enumerate(range(0, sweep.numel(), Cc)):
        beta = torch.zeros(Cc)
        part = sweep[c0:c0 + Cc]
        beta[:part.numel()] = part
        y, _ = gn_fwd(L, x, torch.zeros(Cc), beta, G, 1)
        n = beta.double()[None, None, :].expand(1, HW, Cc)
        worst = max(worst, NL.check_interval(f"silu_f sweep, launch {i}", y, NL.silu64(n), NL.silu_delta(n, 0 * n)))
    print(f"[nonlinear] silu_f over {sweep.numel()} bf16 arguments: max err / allowed {worst:.4g}")


def silu_grad_sweep_case():
    """x carries the sweep, mean = 0, rstd = 1, gamma = 1, beta = 0 are passed in: the activation's argument is x itself.  Groups 0 .. 30 hold
    every finite bf16 value with |x| <= 128 (shuffled); group 31 holds +-1e4, and +-3e38 under dy = 0 (their products with a finite
    silu_grad_f vanish exactly: a NaN or an infinity there poisons the group's sums and fails every element of it)."""
    B, HW, Cc, G = 8, 72, 64, 32
    sweep = NL.bf16_sweep(128.0)
    g = NL.gen(21)
    body = torch.zeros(B * HW * 62)
    body[:sweep.numel()] = sweep
    body = body[torch.randperm(body.numel(), generator=g)].view(B, HW, 62)
    tail = torch.zeros(B, HW, 2)
    dy = NL.rnd(B, HW, Cc, seed=22)
    for b in range(B):
        tail[b, 3, 0], tail[b, 5, 1] = 1e4, -1e4
        tail[b, 7, b % 2], tail[b, 9, 1 - b % 2] = 3e38, -3e38
        dy[b, 7, 62:] = 0
        dy[b, 9, 62:] = 0
    x = torch.cat([body, tail], 2).to(BF).float()
    stats = torch.stack([torch.zeros(B, G), torch.ones(B, G)], -1).contiguous()
    gamma, beta = torch.ones(Cc), torch.zeros(Cc)
    return x, dy, gamma, beta, stats, NL.gn_bwd_ref(x, dy, gamma, beta, stats, G, 1)


def test_silu_grad_sweep_through_groupnorm_backward(L):
    x, dy, gamma, beta, stats, r = cached("silu grad sweep", silu_grad_sweep_case)
    dx, dg, db = gn_bwd(L, x, dy, gamma, beta, stats, 32, 1)
    NL.check_interval("silu_grad_f sweep dx", dx, r["dx"], r["ddx"])
    NL.check_f32("silu_grad_f sweep dgamma", dg, r["dgamma"], r["ddgamma"])
    NL.check_f32("silu_grad_f sweep dbeta", db, r["dbeta"], r["ddbeta"])


# ------------------------------------------------------------------------------------------------ LayerNorm
LN_WIDTHS = [128, 256, 384, 512, 640, 768, 896, 1024, 1280, 2048, 2560]      # every instantiated width
LN_CASES = [(M, Cc) for Cc in LN_WIDTHS for M in (1, 37)] + [(16400, 128), (33000, 128),      # iters = 2 and 4 in ln_bwd_geometry
                                                               (8200, 1024)]                 # 32 lanes per row with iters = 2


def ln_fwd(L, x, gamma, beta):
    M, Cc = x.shape
    y, stats = out_like(M, Cc), out_like(M, 2, dtype=F32)
    xd, gd, bd = D(x), D(gamma), D(beta)
    lib.check(L.sdxl_op_layernorm_fwd(ptr(xd), ptr(y), ptr(gd), ptr(bd), ptr(stats), M, Cc, EPS, stream()))
    torch.cuda.synchronize()
    return y, stats


def ln_bwd(L, x, dy, gamma, stats, addend=None):
    M, Cc = x.shape
    dx = out_like(M, Cc) if addend is None else D(addend)
    dg, db = zeros(Cc), zeros(Cc)
    xd, dyd, gd, sd = D(x), D(dy), D(gamma), stats.to(dev()).contiguous()
    lib.check(L.sdxl_op_layernorm_bwd(ptr(xd), ptr(dyd), ptr(gd), ptr(sd), ptr(dx), ptr(dg), ptr(db), M, Cc, int(addend is not None), stream()))
    torch.cuda.synchronize()
    return dx, dg, db


def ln_refs(M, Cc):
    def make():
        gamma, beta = NL.affine(Cc, 51)
        x2, K, s = NL.two_point(M, Cc, 9)
        r2 = NL.ln_fwd_ref(x2, gamma, beta, EPS, exact_sums=True)
        x = NL.ln_graded(M, Cc, 13)
        f = NL.ln_fwd_ref(x, gamma, beta, EPS)
        stats = torch.stack([f["mean"], f["rstd"]], 1).float().contiguous()
        dy, addend = NL.rnd(M, Cc, seed=53), NL.rnd(M, Cc, seed=54)
        xi, Ki, _ = NL.two_point(M, Cc, 15, s=1.0)
        dyi = NL.ints(M, Cc, seed=55)
        exact = ((dyi.double() * (xi.double() - Ki.double()[:, None])).sum(0).float(), dyi.double().sum(0).float())
        return dict(gamma=gamma, beta=beta, x2=x2, K=K, s=s, r2=r2, x=x, f=f, stats=stats, dy=dy, addend=addend,
                    bwd=[NL.ln_bwd_ref(x, dy, gamma, stats, a) for a in (None, addend)],
                    xi=xi, dyi=dyi, stats_i=torch.stack([Ki, torch.ones_like(Ki)], 1).contiguous(), exact=exact)
    return cached(("ln", M, Cc), make)


@pytest.mark.parametrize("M,Cc", LN_CASES)
def test_layernorm_forward(L, M, Cc):
    """y and the stored (mean, rstd) per row: two-point rows, graded randn rows with a +-2^-9 row and a constant row.  Derivation: ln_fwd_ref.
    Two-point rows where C is a power of two: x (1 / C) is an exact scaling, so mean = K bit for bit, d = +-s and sq = C s^2 are exact, and
    rstd is within 2 fp32 ulp of (s^2 + eps)^-1/2 as for GroupNorm (one rounded sum, one 1-ulp instruction).  At the other widths 1 / C is a
    rounded constant: the mean is K up to 2 U, the second pass sums inexact squares, and both are held to ln_fwd_ref's derived bounds instead."""
    d = ln_refs(M, Cc)
    tag = f"layernorm {M}x{Cc}"
    y, stats = ln_fwd(L, d["x2"], d["gamma"], d["beta"])
    if Cc & (Cc - 1) == 0:
        NL.check_bits(f"{tag} two-point mean", stats[:, 0].cpu(), d["K"])
        NL.check_ulps(f"{tag} two-point rstd", stats[:, 1], (d["s"].double() ** 2 + EPS).rsqrt(), 2)
    NL.check_f32(f"{tag} two-point mean", stats[:, 0], d["K"].double(), d["r2"]["dmean"])
    NL.check_f32(f"{tag} two-point rstd", stats[:, 1], (d["s"].double() ** 2 + EPS).rsqrt(), d["r2"]["drstd"])
    NL.check_interval(f"{tag} two-point y", y, d["r2"]["y"], d["r2"]["dy"])
    y, stats = ln_fwd(L, d["x"], d["gamma"], d["beta"])
    NL.check_f32(f"{tag} graded mean", stats[:, 0], d["f"]["mean"], d["f"]["dmean"])
    NL.check_f32(f"{tag} graded rstd", stats[:, 1], d["f"]["rstd"], d["f"]["drstd"])
    NL.check_interval(f"{tag} graded y", y, d["f"]["y"], d["f"]["dy"])


@pytest.mark.parametrize("M,Cc", LN_CASES)
def test_layernorm_backward(L, M, Cc):
    """dx with accumulate 0 and 1, dgamma, dbeta from the reference's statistics; the exact integer parameter gradients.  With the diagnostics
    build also knob 10's forms 1 (lean dx kernel + partial rows) and 3 (lean + the column-sum pass).  Derivation: ln_bwd_ref."""
    d = ln_refs(M, Cc)
    for form in ((0, 1, 3) if lib.DIAG else (0,)):
        if lib.DIAG:
            knob(L, 10, form)
        try:
            for a, b in zip((None, d["addend"]), d["bwd"]):
                t = f"layernorm {M}x{Cc} form {form} accumulate {int(a is not None)}"
                dx, dg, db = ln_bwd(L, d["x"], d["dy"], d["gamma"], d["stats"], a)
                NL.check_interval(f"{t} dx", dx, b["dx"], b["ddx"])
                NL.check_f32(f"{t} dgamma", dg, b["dgamma"], b["ddgamma"])
                NL.check_f32(f"{t} dbeta", db, b["dbeta"], b["ddbeta"])
            _, dg, db = ln_bwd(L, d["xi"], d["dyi"], d["gamma"], d["stats_i"])
            NL.check_bits(f"layernorm {M}x{Cc} form {form} exact dgamma", dg, d["exact"][0])
            NL.check_bits(f"layernorm {M}x{Cc} form {form} exact dbeta", db, d["exact"][1])
        finally:
            if lib.DIAG:
                knob(L, 10, 0)


# ------------------------------------------------------------------------------------------------ GEGLU: the non-linear half, on every route
def _sk(L, on):
    lib.check(L.sdxl_set_sk_mode(2 if on else 0, 0))


def geglu_fwd_case(L, name, mode, G, rows, sk):
    """x = 0, so u is the bias EXACTLY (equal as numbers after unpacking: the accumulator's 0 + (-0) is +0, the one bit that may differ) and
    g = bf16(value x gate x cdf(gate)) with both read from the bias: every
    finite bf16 gate with |t| <= 16 and +-32, +-64, +-1e4, each pass pairing it with another of the four values.  All rows of a launch get the
    same operands: row 0 passes the interval check (geglu_fwd_ref: |value gate| x the measured cdf bound + two products), every other row
    equals it bit for bit, and the rows past M (the buffers are 8 rows longer) keep the sentinel."""
    C4, K = NL.GEGLU_FWD_C4, NL.GEGLU_K
    for M in sorted(set(rows)):
        print(f"[route] geglu fwd {name} group {G} M {M}: {NL.geglu_route(lib, L, mode, True, M, G, sk)}")
    w1 = D(NL.geglu_pack_rows(NL.ints(2 * C4, K, seed=61), C4, G))
    worst = 0.0
    lib.check(L.sdxl_set_gemm_mode(mode))
    if sk:
        _sk(L, True)
    try:
        for i, (M, v, t) in enumerate(cached("geglu fwd launches " + str(rows), lambda: NL.geglu_fwd_launches(rows))):
            b1 = torch.cat([v, t])
            b1p = D(NL.geglu_pack_rows(b1, C4, G))
            x = torch.zeros(M, K, dtype=BF, device=dev())
            u, g = out_like(M + 8, 2 * C4), out_like(M + 8, C4)
            lib.check(L.sdxl_op_ff_geglu_fwd(ptr(x), ptr(w1), ptr(b1p), ptr(u), ptr(g), M, K, C4, G, stream()))
            torch.cuda.synchronize()
            assert bool((u[M:] == SENTINEL).all()) and bool((g[M:] == SENTINEL).all()), f"{name} launch {i}: rows past M = {M} were written"
            iv = lambda z: z.contiguous().view(torch.int16)
            assert bool((iv(u[:M]) == iv(u[:1])).all()) and bool((iv(g[:M]) == iv(g[:1])).all()), f"{name} launch {i}: rows differ"
            ub, want = NL.geglu_unpack_cols(u[:1].cpu(), C4, G)[0].double(), b1.double()      # (equal as numbers: the accumulator's 0 + (-0) is +0)
            diff = (ub != want).nonzero().flatten()
            assert diff.numel() == 0, (f"{name} launch {i}: u is not the bias at {diff.numel()} columns; first: got {float(ub[diff[0]])!r}, "
                                       f"bias {float(want[diff[0]])!r}")
            ref, delta = cached(("geglu fwd ref", rows, i), lambda: NL.geglu_fwd_ref(v, t))
            worst = max(worst, NL.check_interval(f"geglu fwd {name} group {G} launch {i} (M {M}) g", g[0].cpu(), ref, delta))
    finally:
        if sk:
            _sk(L, False)
        lib.check(L.sdxl_set_gemm_mode(1))
    print(f"[nonlinear] geglu fwd {name} group {G}: u equal to the bias as numbers, g max err / allowed {worst:.4g}")


def geglu_bwd_case(L, name, mode, G, sk):
    """u carries the sweep directly (M = 256), dG = dy w2 an exact small integer: d value = dG t cdf(t), d gate = dG value (cdf(t) + t pdf(t)),
    absolute bounds (geglu_bwd_ref)"""
    M, C4, K = NL.GEGLU_BWD_M, 4 * G, NL.GEGLU_K
    print(f"[route] geglu bwd {name} group {G}: {NL.geglu_route(lib, L, mode, False, M, G, sk)}")
    o = cached(("geglu bwd", G), lambda: NL.geglu_bwd_operands(G))
    ra, da, rt, dt = cached(("geglu bwd ref", G), lambda: NL.geglu_bwd_ref(o["dG"], o["value"], o["gate"]))
    u, dy, w2 = D(NL.geglu_pack_cols(o["value"], o["gate"], G)), D(o["dy"]), D(o["w2"])
    du = out_like(M, 2 * C4)
    lib.check(L.sdxl_set_gemm_mode(mode))
    if sk:
        _sk(L, True)
    try:
        lib.check(L.sdxl_op_ff_geglu_bwd(ptr(dy), ptr(w2), ptr(u), ptr(du), M, K, C4, G, stream()))
        torch.cuda.synchronize()
    finally:
        if sk:
            _sk(L, False)
        lib.check(L.sdxl_set_gemm_mode(1))
    got = NL.geglu_unpack_cols(du.cpu(), C4, G)
    NL.check_interval(f"geglu bwd {name} group {G} d value", got[:, :C4].contiguous(), ra, da)
    NL.check_interval(f"geglu bwd {name} group {G} d gate", got[:, C4:].contiguous(), rt, dt)


def _rid(rows):
    return [f"{r[0].replace(' ', '_')}-g{r[2]}" for r in rows]


_GF = [r for r in NL.GEGLU_FWD_ROUTES if not r[4]]
_GB = [r for r in NL.GEGLU_BWD_ROUTES if not r[3]]
_GF_DIAG = [r for r in NL.GEGLU_FWD_ROUTES if r[4]]
_GB_DIAG = [r for r in NL.GEGLU_BWD_ROUTES if r[3]]


@pytest.mark.parametrize("name,mode,G,rows,need", _GF, ids=_rid(_GF))
def test_geglu_forward_gate_sweep(L, name, mode, G, rows, need):
    geglu_fwd_case(L, name, mode, G, rows, False)


@pytest.mark.parametrize("name,mode,G,need", _GB, ids=_rid(_GB))
def test_geglu_backward_gate_sweep(L, name, mode, G, need):
    geglu_bwd_case(L, name, mode, G, False)


@pytest.mark.diag
@pytest.mark.parametrize("name,mode,G,rows,need", _GF_DIAG, ids=_rid(_GF_DIAG))
def test_geglu_forward_gate_sweep_of_the_diagnostics_build(L, name, mode, G, rows, need):
    """configuration 43 of the 128-row kernel, and gemm_sk.hip's copy of the epilogue (stream-K)"""
    geglu_fwd_case(L, name, mode, G, rows, need == "sk")


@pytest.mark.diag
@pytest.mark.parametrize("name,mode,G,need", _GB_DIAG, ids=_rid(_GB_DIAG))
def test_geglu_backward_gate_sweep_of_the_diagnostics_build(L, name, mode, G, need):
    """configuration 43, co-resident modes 33 / 34 (the exclusive 6-deep-ring form), stream-K"""
    geglu_bwd_case(L, name, mode, G, need == "sk")


# ------------------------------------------------------------------------------------------------ attention: the softmax away from uniform
def attn_case(B, heads, Nq, Nk):
    def make():
        o = NL.attn_operands(B, heads, Nq, Nk)
        f = NL.attn_fwd_ref(o, heads)
        lse32, o16 = f["lse"].float().contiguous(), NL.bf16_rn64(f["o"])
        return o, f, lse32, o16, NL.attn_bwd_ref(o, heads, lse32, o16)
    return cached(("attn", B, heads, Nq, Nk), make)


def attn_run(L, B, heads, Nq, Nk, self_attn, route=None):
    """q = 2 randn (peaked rows), k, v, dO randn.  The float64 reference restates the ONE rounding the kernels make by design (scale8: the
    forward and the dQ bodies compute their scores from bf16(q x scale x log2 e), the dK / dV bodies from the equally rounded k) and nothing
    else; the backward receives lse (fp32) and O (bf16) from the reference.  lse and Delta are held to
    (2^-22 (|m| + |log l|) + (Nk + 64) 2^-24, natural units: about 1e-5 where tests/test_gpu_ops.py allows 7e-3; 64 x 2^-24 sum|dO O|);
    O, dV, dQ, dK to the intervals derived in attn_fwd_ref / attn_bwd_ref (2^-8 sum p |v| and its kin, because P and dS enter the matrix pipe
    as bf16, plus the fp32 terms)."""
    o, f, lse32, o16, b = attn_case(B, heads, Nq, Nk)
    Cc = heads * 64
    route = route or NL.attn_bwd_route(B, heads, Nq, Nk)      # (restated from the launcher; tests/test_host_nonlinear.py holds the table to it)
    tag = f"attention B{B} h{heads} {Nq}x{Nk}"
    print(f"[route] {tag} backward: {route}")
    if self_attn:
        qkv = D(torch.cat([o["q"], o["k"], o["v"]], 2))
        q, k, v = qkv[..., :Cc], qkv[..., Cc:2 * Cc], qkv[..., 2 * Cc:]
        ldq = ldk = ldv = 3 * Cc
        dqkv = out_like(B, Nq, 3 * Cc)
        dq, dk, dv = dqkv[..., :Cc], dqkv[..., Cc:2 * Cc], dqkv[..., 2 * Cc:]
    else:
        q, kv = D(o["q"]), D(torch.cat([o["k"], o["v"]], 2))
        k, v = kv[..., :Cc], kv[..., Cc:]
        ldq, ldk, ldv = Cc, 2 * Cc, 2 * Cc
        dq, dkv = out_like(B, Nq, Cc), out_like(B, Nk, 2 * Cc)
        dk, dv = dkv[..., :Cc], dkv[..., Cc:]
    out, lse = out_like(B, Nq, Cc), out_like(B * heads, Nq, dtype=F32)
    lib.check(L.sdxl_op_attention_fwd(ptr(q), ptr(k), ptr(v), ptr(out), ptr(lse), B, heads, Nq, Nk, ldq, ldk, ldv, Cc, stream()))
    torch.cuda.synchronize()
    NL.check_f32(f"{tag} lse", lse, f["lse"], f["dlse"])
    NL.check_interval(f"{tag} O", out, f["o"], f["do"])
    od, dod, lsed = o16.to(dev()).contiguous(), D(o["dO"]), lse32.to(dev())
    delta = out_like(B * heads, Nq, dtype=F32)
    lib.check(L.sdxl_op_attention_bwd(ptr(q), ptr(k), ptr(v), ptr(od), ptr(dod), ptr(lsed), ptr(delta), ptr(dq), ptr(dk), ptr(dv),
                                      B, heads, Nq, Nk, ldq, ldk, ldv, Cc, stream()))
    torch.cuda.synchronize()
    NL.check_f32(f"{tag} Delta", delta, b["delta"], b["ddelta"])
    NL.check_interval(f"{tag} dV", dv.contiguous(), b["dv"], b["ddv"])
    NL.check_interval(f"{tag} dQ", dq.contiguous(), b["dq"], b["ddq"])
    NL.check_interval(f"{tag} dK", dk.contiguous(), b["dk"], b["ddk"])


@pytest.mark.parametrize("B,heads,Nq,Nk,self_attn", NL.ATTN_SHAPES)
def test_attention_peaked_softmax(L, B, heads, Nq, Nk, self_attn):
    """the five backward forms the product policy chooses between: dQ + unsplit dK / dV kernels, dQ + split-query dK / dV + reduce (at 77, 257
    and 2048 keys), the fused grid, the pipelined grid (attn_run states the reference and the bounds)"""
    attn_run(L, B, heads, Nq, Nk, self_attn)


@pytest.mark.diag
@pytest.mark.parametrize("knob35,route", [(1, "fused (knob 35 = 1)"), (2, "pipelined (knob 35 = 2)")])
@pytest.mark.parametrize("B,heads,Nq,Nk", [(2, 4, 988, 988), (1, 4, 2048, 2048)])
def test_attention_peaked_softmax_fused_and_pipelined_forced(L, B, heads, Nq, Nk, knob35, route):
    """knob 35 of the diagnostics build: 1 never takes the pipelined backward (the fused grid at 2048 rows), 2 takes it wherever it applies
    (988 rows: ragged last tiles in attention_bwd_pl.hip)"""
    knob(L, 35, knob35)
    try:
        attn_run(L, B, heads, Nq, Nk, True, route)
    finally:
        knob(L, 35, 0)
