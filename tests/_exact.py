"""Exact-arithmetic and per-element checks for the GEMM / convolution kernels (tests/test_gpu_ops_exact.py), and the proof on the CPU that the
checks see what they claim to see (tests/test_host_exact.py).  No GPU needed: everything here is CPU torch.

1. Integer operands.  Operands from {-2 .. 2}, bias from {-8 .. 8}, for the bf16-output forms a residual of EVEN integers in +-[256, 510]: all
   bf16-exact; every partial sum of a reduction over K <= 65536 products is an integer of magnitude <= 4 K + 518 < 2^24, so the fp32 accumulator
   holds it exactly whatever the summation order, split-K factor, stream-K partition or tile shape.  The one correct answer is therefore
       fp32 output:  the integer itself,
       bf16 output:  ONE round-to-nearest-even conversion of the integer (torch's CPU float32 -> bfloat16 cast),
   compared with torch.equal on the raw bits.  The residual pushes the results across the binades [256, 512) (bf16 spacing 2: odd integers are
   ties) and [512, 1024) (spacing 4: 2 mod 4 are ties), so truncation, round-half-up and a double rounding all change bits
   (assert_has_ties is the precondition on the INPUTS that makes that so).
2. randn operands.  float64 on the same bf16-rounded operands (the convention of test_gpu_grad_select.ref64), and for EVERY element
       |got - ref| <= u |ref| + K 2^-23 (|A| . |B| + |bias| + |resid|),      u = 2^-8 (bf16 output) | 2^-24 (fp32 output):
   one rounding of the result to 8 (24) significant bits (half an ulp of a value at the bottom of its binade: the unit roundoff, no
   slack), and the fp32 accumulation of K products and the addends in any order ((K + 1) 2^-24 to first order, with the factor 2 of slack
   that the project already uses).  An op that rounds more than once adds one such term per further rounding, derived where it is used."""
from __future__ import annotations

import math
from collections import namedtuple

import torch

BF = torch.bfloat16
TIE_MIN_FRACTION = 0.10      # a rounding case counts only with >= 10 % ties rounding up in magnitude AND >= 10 % rounding down


# ------------------------------------------------------------------------------------------------ 1. integer operands, exact expectation
def gen(seed):
    return torch.Generator(device="cpu").manual_seed(seed)


def ints(*shape, seed, lo=-2, hi=2, nonzero=False):
    """float32 integers drawn uniformly from {lo .. hi}; nonzero: zeros are replaced by +-1 (a zero product cannot be seen to drop)"""
    g = gen(seed)
    t = torch.randint(lo, hi + 1, shape, generator=g).float()
    if nonzero:
        sign = torch.randint(0, 2, shape, generator=g).float() * 2 - 1
        t = torch.where(t == 0, sign, t)
    return t


def bias_ints(n, seed):
    return ints(n, seed=seed, lo=-8, hi=8)


def resid_even(*shape, seed):
    """even integers in +-[256, 510]: bf16-exact (spacing 2 in that binade)"""
    g = gen(seed)
    mag = 256 + 2 * torch.randint(0, 128, shape, generator=g)
    sign = torch.randint(0, 2, shape, generator=g) * 2 - 1
    return (mag * sign).float()


def bf16_rn(x):
    """ONE float32 -> bfloat16 conversion (round to nearest, ties to even) of exact values that fp32 holds exactly"""
    x32 = x.float()
    assert torch.equal(x32.double(), x.double()), "the exact value does not fit fp32: not an exact-arithmetic case"
    return x32.to(BF)


def expect(exact64, out_bf16):
    """the one correct output for an exact (float64) integer result: bf16_rn of it | the integer itself in fp32"""
    assert float(exact64.abs().max()) < 2.0 ** 24
    return bf16_rn(exact64) if out_bf16 else exact64.float()


def same_bits(a, b):
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    iv = torch.int16 if a.dtype == BF else torch.int32
    return torch.equal(a.contiguous().view(iv), b.contiguous().view(iv))


def count_diff(got, want):
    return int((got.double() != want.double()).sum())


def assert_exact(tag, got, want):
    """bit equality of a result with its exact expectation (same dtype); prints and reports how many elements differ, and the first"""
    got, want = got.detach().cpu(), want.detach().cpu()
    assert got.dtype == want.dtype and got.shape == want.shape, (tag, got.dtype, want.dtype, tuple(got.shape), tuple(want.shape))
    ok = same_bits(got, want)
    n = 0 if ok else count_diff(got, want)
    print(f"[exact] {tag}: {'bit-equal' if ok else f'{n} of {got.numel()} elements differ'}")
    if not ok:
        bad = (got.double() != want.double()) | (torch.isnan(got.double()))
        i = int(bad.flatten().nonzero()[0]) if bool(bad.any()) else -1      # (-1: only the sign of a zero differs)
        raise AssertionError(f"{tag}: {n} of {got.numel()} elements differ from the exact value; first at flat index {i}: "
                             f"got {float(got.flatten()[i])}, exact {float(want.flatten()[i])}")


def tie_fractions(exact64):
    """(fraction of elements that are bf16 rounding ties resolved UP in magnitude by ties-to-even, fraction resolved DOWN)"""
    v = exact64.double().flatten()
    r = bf16_rn(v).double()
    a = v.abs()
    e = torch.floor(torch.log2(a.clamp_min(1.0)))
    half = 2.0 ** (e - 8)                                  # half a bf16 ulp in the binade of |v| (8 significant bits: ulp = 2^(e - 7))
    tie = (a >= 256) & (torch.remainder(a, 2 * half) == half)
    up = tie & (r.abs() > a)
    down = tie & (r.abs() < a)
    assert bool(((up | down) == tie).all())
    return float(up.double().mean()), float(down.double().mean())


def assert_has_ties(exact64, tag=""):
    """a condition on the INPUTS of a rounding case, not a measurement of the kernel"""
    up, down = tie_fractions(exact64)
    print(f"[exact] {tag}: ties rounding up {100 * up:.1f} %, down {100 * down:.1f} %")
    assert up >= TIE_MIN_FRACTION and down >= TIE_MIN_FRACTION, f"{tag}: only {up:.3f} / {down:.3f} of the outputs are ties up / down"


# ------------------------------------------------------------------------------------------------ 2. randn operands, per-element bound
def rnd(*shape, seed, scale=1.0):
    """bf16-rounded randn, as float32 on the CPU"""
    return (torch.randn(*shape, generator=gen(seed)) * scale).to(BF).float()


def bound(ref64, absdot64, K, out_bf16, extra=None):
    """u |ref| + K 2^-23 (|A| . |B| + |bias| + |resid|): absdot64 is the parenthesis (the same product on absolute values + the absolute
    addends).  `extra`: a further DERIVED term of an op that rounds more than once (stated where it is used)."""
    u = 2.0 ** -8 if out_bf16 else 2.0 ** -24
    b = u * ref64.abs() + K * 2.0 ** -23 * absdot64
    return b if extra is None else b + extra


def check_bound(tag, got, ref64, bnd):
    """every element within its bound, none left out; prints max err / bound as test_gpu_grad_select.check_bound does"""
    got = got.detach().cpu().double()
    assert got.shape == ref64.shape == bnd.shape, (tag, tuple(got.shape), tuple(ref64.shape), tuple(bnd.shape))
    assert bool(torch.isfinite(got).all()), f"{tag}: not written everywhere"
    err = (got - ref64).abs()
    ratio = float((err / bnd.clamp_min(1e-300)).max())
    print(f"[bound] {tag}: max |err| / bound {ratio:.3f}")
    assert float((err - bnd).max()) <= 0.0, f"{tag}: an element exceeds its a-priori bound (max err / bound {ratio:.3f})"
    return ratio


# ------------------------------------------------------------------------------------------------ GEMM operands of one case
def gemm_operands(form, M, N, K, integer, seed=0, nonzero=False):
    """CPU float32 operands of sdxl_op_gemm's three forms: 0 NT a [M][K] w [N][K]; 1 NN a [M][K] w [K][N]; 2 TN a [K][M] b [K][N].
    integer: {-2 .. 2} | bf16-rounded randn (the weight scaled by K^-1/2 as tests/test_gpu_ops.py does).  Plus bias [N] and resid [M][N]
    (forms 0 / 1; integer: {-8 .. 8} and even +-[256, 510]) and, for form 2, an fp32 base [M][N] to accumulate onto."""
    s = 1000 * seed
    if integer:
        I = lambda *sh, sd: ints(*sh, seed=s + sd, nonzero=nonzero)
        if form == 2:
            return dict(a=I(K, M, sd=8), b=I(K, N, sd=9), base=ints(M, N, seed=s + 10, lo=-1000, hi=1000))
        return dict(a=I(M, K, sd=1), w=I(N, K, sd=2) if form == 0 else I(K, N, sd=6), bias=bias_ints(N, s + 3), resid=resid_even(M, N, seed=s + 4))
    if form == 2:
        return dict(a=rnd(K, M, seed=s + 8), b=rnd(K, N, seed=s + 9), base=torch.randn(M, N, generator=gen(s + 10)))
    return dict(a=rnd(M, K, seed=s + 1), w=rnd(N, K, seed=s + 2, scale=K ** -0.5) if form == 0 else rnd(K, N, seed=s + 6, scale=K ** -0.5),
                bias=rnd(N, seed=s + 3), resid=rnd(M, N, seed=s + 4))


def gemm_ref64(form, ops, bias=True, resid=True):
    """(float64 result, the same product on absolute values + absolute addends) of one form"""
    d = {k: v.double() for k, v in ops.items()}
    if form == 2:      # (+ 0.0: the accumulator starts at +0, and (+0) + (-0) = +0 -- at K = 1 a lone product 0 x (-2) would otherwise leave the reference at -0)
        return d["a"].T @ d["b"] + 0.0, d["a"].abs().T @ d["b"].abs()
    w = d["w"].T if form == 0 else d["w"]
    ref, ab = d["a"] @ w, d["a"].abs() @ w.abs()
    if bias:
        ref, ab = ref + d["bias"], ab + d["bias"].abs()
    if resid:
        ref, ab = ref + d["resid"], ab + d["resid"].abs()
    return ref, ab


# ------------------------------------------------------------------------------------------------ the GPU file's case table
# One row per exact case of tests/test_gpu_ops_exact.py that goes through launch_gemm: what sdxl_debug_gemm_route needs to name its kernel.
#   mode: the word for sdxl_set_gemm_mode (1: the policy; 2: the 256 x 256 kernel wherever applicable; 4 cfg: forced configuration)
#   splitk: as passed to the entry point (form 2: 0 = the plan's choice, which the route's `post` then does not show)
#   diag: needs the diagnostics build
Case = namedtuple("Case", "family mode form M N K splitk bias_grad group diag", defaults=(1, 0, 1, False))


def _c(family, mode, form, M, N, K, splitk=1, bias_grad=0, group=1, diag=False):
    return Case(family, mode, form, M, N, K, splitk, bias_grad, group, diag)


NT_DEFAULT = [(128, 128, 64), (308, 1280, 2048), (4, 1280, 320), (300, 200, 128)]       # the last: ragged M AND N (not a multiple of 128 / 160)
NN_DEFAULT = [(128, 128, 64), (308, 2048, 1280), (300, 200, 128)]
SPLITK_BF16 = [(77, 640, 2048, 4), (256, 384, 320, 7), (4, 1280, 2816, 11)]
TN_WGRAD = [(128, 128, 64, 1), (320, 384, 1000, 1), (640, 640, 308, 2), (8, 320, 65536, 16), (72, 200, 520, 3)]      # the last: ragged tiles, K % 64 != 0, split
TN_LONG = [(200, 72, 16384, s) for s in (0, 1, 3)]
WGRAD_GROUP = [(4, 128, 160, 64), (2, 320, 640, 1000)]                                   # (n, Mo, No, rows)
CR256_MODES = [31, 32, 35, 36]
CR256_MODES_DIAG = [33, 34]
CR256_NT_NN = [(256, 160, 32), (300, 200, 128)]
CR256_TN = [(256, 160, 32, 1), (512, 320, 96, 1)]
G256_NT_NN = [(256, 256, 64), (512, 768, 192)]
G256_TN = [(256, 256, 64, 1), (512, 256, 192, 1)]
CFG23 = [(128, 160, 64), (256, 320, 192)]
PIPELINED_CFGS = [7, 8, 5, 6]
PIPELINED = [(128, 160, 64), (128, 128, 256), (256, 320, 192)]
STREAM_K_WORKERS = [1, 7, 37, 0]
STREAM_K_PROBLEMS = [(0, 512, 768, 640), (1, 512, 768, 640), (2, 512, 256, 2048)]         # (form, M, N, K): tests/test_gpu_ops.py's stream-K launches
# reductions shorter than one K block: the weight gradients of the embedding linears and of the grouped time-embedding projection reduce over the
# BATCH (K = B in {1, 2, 4}); the last row is the grouped projection of the full-size model at batch 4, whose other two forms follow
TN_SHORT = [(320, 128, 1, 0), (320, 128, 2, 0), (320, 128, 4, 0), (200, 72, 4, 0), (2240, 1280, 4, 0)]
TN_SHORT_FORCED = (512, 256, 4, 0)        # under the 256 x 256 mode and the co-resident words: K % 64 / K % 32 turn both away, the 128-row kernel must run
NT_GROUPED_PROJECTION = (4, 2240, 1280)
NN_GROUPED_PROJECTION = (4, 1280, 2240)
CONV_WGRAD3 = [(1, 256, 64, 64, 64)]       # (B, H, W, Cin, Cout): W = 64 is the smallest width of conv_wgrad3.hip, 256 rows the fewest that make 16 384 pixels
CONV_WGRAD3_SPLITK = [0, 1, 5]
# the rounding cases: every bf16-output GEMM case below runs with the even residual (forms 0 / 1; form 1 as accumulate = 1 onto it)
# and is held to assert_has_ties in tests/test_host_exact.py


def gemm_cases():
    """every launch_gemm case of the GPU file whose route the table decides (the convolutions build their descriptors in conv_desc)"""
    out = []
    out += [_c("nt default", 1, 0, *s) for s in NT_DEFAULT]
    out += [_c("nn default", 1, 1, *s) for s in NN_DEFAULT]
    out += [_c("bf16 split-K", 1, f, M, N, K, sk) for (M, N, K, sk) in SPLITK_BF16 for f in (0, 1)]
    out += [_c("tn wgrad", 1, 2, M, N, K, sk, bias_grad=1) for (M, N, K, sk) in TN_WGRAD]
    out += [_c("tn long reduction", 1, 2, M, N, K, sk, bias_grad=1) for (M, N, K, sk) in TN_LONG]
    out += [_c("wgrad group", 1, 2, Mo, No, rows, 1, bias_grad=1, group=n) for (n, Mo, No, rows) in WGRAD_GROUP]
    for m in CR256_MODES + CR256_MODES_DIAG:
        d = m in CR256_MODES_DIAG
        out += [_c(f"cr256 mode {m}", 4 * m, f, *s, diag=d) for s in CR256_NT_NN for f in (0, 1)]
        out += [_c(f"cr256 mode {m} tn", 4 * m, 2, M, N, K, sk, bias_grad=1, diag=d) for (M, N, K, sk) in CR256_TN]
    out += [_c("gemm256", 2, f, *s) for s in G256_NT_NN for f in (0, 1)]
    out += [_c("gemm256 tn", 2, 2, M, N, K, sk, bias_grad=1) for (M, N, K, sk) in G256_TN]
    out += [_c("cfg 23", 4 * 23, f, *s) for s in CFG23 for f in (0, 1)]
    out += [_c(f"pipelined cfg {c}", 4 * c, f, *s) for c in PIPELINED_CFGS for s in PIPELINED for f in (0, 1)]
    out += [_c("tn wgrad short reduction", 1, 2, M, N, K, sk, bias_grad=1) for (M, N, K, sk) in TN_SHORT]
    out += [_c("nt default grouped projection", 1, 0, *NT_GROUPED_PROJECTION), _c("nn default grouped projection", 1, 1, *NN_GROUPED_PROJECTION)]
    M, N, K, sk = TN_SHORT_FORCED
    out += [_c("tn short reduction forced 256x256", 2, 2, M, N, K, sk, bias_grad=1)]
    out += [_c(f"tn short reduction forced cr256 mode {m}", 4 * m, 2, M, N, K, sk, bias_grad=1) for m in CR256_MODES]
    return out


def conv_desc(kind, B, H, W, Cin, Cout, stride=1, splitk=1, bias_grad=0):
    """the sdxl_gemm_desc of a 3x3 convolution (pad 1), restated from conv3x3_{fwd,dgrad,wgrad}_problem (csrc/gemm.hip)"""
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    if kind == "fwd":
        return dict(form=0, taps=9, M=B * Ho * Wo, N=Cout, K=Cin, Hm=Ho, Wm=Wo, Hs=H, Ws=W, sm=stride, sd=1, splitk=splitk)
    if kind == "dgrad":
        return dict(form=1, taps=9, M=B * H * W, N=Cin, K=Cout, Hm=H, Wm=W, Hs=Ho, Ws=Wo, sm=1, sd=stride, splitk=splitk)
    assert kind == "wgrad"
    return dict(form=2, taps=9, M=Cout, N=Cin, K=B * Ho * Wo, Hm=Ho, Wm=Wo, Hs=H, Ws=W, sm=stride, sd=1, splitk=max(splitk, 1), bias_grad=bias_grad)


def small_splitk(M, N, K, conv):
    """the plan's split-K factor of a small bf16-output problem, restated from gemm_pick_splitk_small (csrc/gemm.hip; knobs at their
    defaults): what sdxl_op_conv3x3_fwd / _dgrad choose for themselves.  K: the whole reduction (taps x channels)."""
    if K % 64 or (M < 64 and K < 1024):
        return 1
    tiles = -(-M // 128) * -(-N // (160 if N % 160 == 0 else 128))
    if conv and 128 < tiles <= 256 and K >= 5120:
        return 2
    if tiles >= 128:
        return 1
    s = min(256 // tiles, K // 64 // 4, 32)
    return 1 if s < 2 else s


def conv_fwd_dgrad_splitk(kind, B, H, W, Cin, Cout, stride):
    """conv3x3_fwd_splitk / conv3x3_dgrad_splitk (csrc/gemm.hip)"""
    if kind == "fwd":
        return small_splitk(B * H * W, Cout, 9 * Cin, True) if stride == 1 and Cin % 64 == 0 else 1
    return small_splitk(B * H * W, Cin, 9 * Cout, True) if stride == 1 and Cin % 64 == 0 and Cout % 64 == 0 else 1


def route_of(lib, L, mode, **desc):
    """which kernel launch_gemm runs for a descriptor under gemm mode `mode`: the library's own answer (sdxl_debug_gemm_route, pure host code)"""
    lib.check(L.sdxl_set_gemm_mode(mode))
    try:
        return lib.gemm_route(**desc)
    finally:
        lib.check(L.sdxl_set_gemm_mode(1))


def case_route(lib, L, c):
    return route_of(lib, L, c.mode, form=c.form, M=c.M, N=c.N, K=c.K, splitk=max(c.splitk, 1), bias_grad=c.bias_grad, group=c.group)


# ------------------------------------------------------------------------------------------------ convolution references (float64, CPU)
def conv_w_nchw(w_native):
    """[Cout][9][Cin] -> [Cout][Cin][3][3]"""
    cout, _, cin = w_native.shape
    return w_native.view(cout, 3, 3, cin).permute(0, 3, 1, 2).contiguous()


def conv_ref64(x_nhwc, w_native, bias, stride):
    """y [B][Ho][Wo][Cout] = conv3x3(x, w) + bias, pad 1, in float64"""
    y = torch.nn.functional.conv2d(x_nhwc.double().permute(0, 3, 1, 2), conv_w_nchw(w_native.double()),
                                   None if bias is None else bias.double(), stride=stride, padding=1)
    return y.permute(0, 2, 3, 1).contiguous()


def conv_dgrad_ref64(dy_nhwc, w_native, H, W, stride):
    """dx [B][H][W][Cin] of the same convolution (conv_transpose2d; output_padding restores an even H / W under stride 2)"""
    Ho, Wo = dy_nhwc.shape[1:3]
    op = (H - ((Ho - 1) * stride + 1), W - ((Wo - 1) * stride + 1))
    dx = torch.nn.functional.conv_transpose2d(dy_nhwc.double().permute(0, 3, 1, 2), conv_w_nchw(w_native.double()), stride=stride, padding=1,
                                              output_padding=op)
    return dx.permute(0, 2, 3, 1).contiguous()


def conv_wgrad_ref64(x_nhwc, dy_nhwc, stride):
    """dw [Cout][9][Cin]: tap (ky, kx) = sum over pixels of dy[b, yo, xo, co] x[b, yo s + ky - 1, xo s + kx - 1, ci] (zero outside)"""
    B, H, W, Cin = x_nhwc.shape
    _, Ho, Wo, Cout = dy_nhwc.shape
    xp = torch.nn.functional.pad(x_nhwc.double(), (0, 0, 1, 1, 1, 1))
    dy2 = dy_nhwc.double().reshape(-1, Cout)
    taps = []
    for ky in range(3):
        for kx in range(3):
            xs = xp[:, ky: ky + (Ho - 1) * stride + 1: stride, kx: kx + (Wo - 1) * stride + 1: stride, :].reshape(-1, Cin)
            taps.append(dy2.T @ xs)
    return torch.stack(taps, 1).contiguous()


def upsample2x_nhwc(x):
    return x.repeat_interleave(2, 1).repeat_interleave(2, 2)


def upsample2x_bwd_nhwc(g):
    """sum of each 2 x 2 block: the transpose of nearest-2x"""
    B, H2, W2, C = g.shape
    return g.view(B, H2 // 2, 2, W2 // 2, 2, C).sum((2, 4))


def upsample2x_bwd_ref64(g_nhwc, addend_nhwc=None):
    """(dx, its bound) of upsample2x_bwd_kernel (csrc/elementwise.hip): the fp32 sum of the four bf16 values of a 2 x 2 block (+ the addend): n
    terms in a fixed order, (n - 1) 2^-24 sum|terms|; the one rounding to bf16 is the check's"""
    ref, ab, n = upsample2x_bwd_nhwc(g_nhwc.double()), upsample2x_bwd_nhwc(g_nhwc.double().abs()), 4
    if addend_nhwc is not None:
        ref, ab, n = ref + addend_nhwc.double(), ab + addend_nhwc.double().abs(), 5
    return ref, (n - 1) * 2.0 ** -24 * ab
