"""Per-element parity for the LOSS kernels (csrc/loss.hip: loss_prepare_kernel, loss_fwd_kernel, loss_finalize_kernel, loss_bwd_kernel) and for the
guidance rescale of the sampler step (csrc/sampler.hip), in the manner of _nonlinear.py / _temb.py: float64 references computed from the CALLER's
inputs (latents, noise, sigma_or_t, the bf16 prediction, the optional arrays), and next to every reference a bound delta accumulated operation by
operation from the kernel's formula.  tests/test_gpu_ops_loss.py runs the kernels against them, tests/test_host_loss_elem.py shows on the CPU that an
fp32 emulation of the formulas (summed in another order) stays inside every bound and that single defects do not.  Not a test module; no GPU needed.

The charges: U = 2^-24 relative per fp32 + - x / sqrt (build.py's flags carry no fast-math: divide and sqrt are correctly rounded; a contraction
into an FMA removes a rounding and stays inside).  The error of the target is carried through d = pred - target (where pred = bf16(target) that
is all there is).  MinSNR's min(1/sigma . 1/sigma, gamma) is an interval: both ends are clamped.  A sum of terms through a tree of depth h is
charged h U sum|terms| plus the terms' own errors.  The final rounding gets no slack: check_interval / check_f32 of _nonlinear.py."""
from __future__ import annotations

import math
from types import SimpleNamespace

import torch

from _nonlinear import BF, F64, U, bf16_rn64, check_bits, check_f32, check_interval      # noqa: F401

LOSS_CAP = 1000.0
# the shapes (B, H, W) at which these kernels can still go wrong
SHAPE_STRADDLE = (4, 13, 10)       # HW = 130: every block straddles samples, block 1 touches three
SHAPE_ALL5 = (5, 5, 10)            # a block spans all five samples; loss_ps_slots = min(255 / 50 + 2, B) = 5 is clamped by B
SHAPE_HW1 = (40, 1, 1)             # HW = 1
SHAPE_ONE_BLOCK = (1, 16, 16)      # exactly one block; numel = 2^10
SHAPE_SPILL = (2, 1, 257)          # one pixel spills into a second block
SHAPE_BUCKET = (4, 104, 152)       # 61.75 blocks per sample
SHAPE_ROWS64 = (2, 129, 128)       # HW = 16 512 = 64.5 blocks per sample: the `r += 64` second trip of the per-sample and mask sums


def blocks(B, HW):
    return (B * HW + 255) // 256


def ps_slots(B, HW):
    """loss_ps_slots of csrc/kernels.h"""
    return min(255 // HW + 2, B)


def sample_rows(b, HW):
    """the block rows [lo, hi] that hold pixels of sample b (loss_finalize_kernel)"""
    return (b * HW) // 256, ((b + 1) * HW - 1) // 256


def loss_tree_depth(rows, channel_adds=True):
    """the depth of the reduction tree of one loss word over `rows` partial rows, read off csrc/loss.hip:
         4   `acc[k] += ...` in loss_fwd_kernel's `for (c < 4)` loop (the mask sum has none: channel_adds = False)
         6   wave_sum: the butterfly over 64 lanes
         3   `sred[0][k] + sred[1][k] + sred[2][k] + sred[3][k]` (`sps[0] + ... + sps[3]` for a per-sample slot)
         ceil(rows / 64)   loss_finalize_kernel's `for (r = threadIdx.x; r < nb; r += 64) s += ...` (per sample: `r = lo + threadIdx.x; r <= hi`)
         64  its `for (l < 64) s += sl[k][l]` by lane 0"""
    return (4 if channel_adds else 0) + 6 + 3 + (rows + 63) // 64 + 64


# ------------------------------------------------------------------------------------------------ a case
def case(method, lat, noise, sig, pred, *, prediction_type=1, min_snr=True, gamma=5.0, loss_type="l2", c=0.0, hc=None, sw=None, tag=None, mask=None,
         mask_norm="mean", per_sample=False, grad_scale=1.0, noise_in=None, cond=None, ztsnr=True, exact=False):
    """everything one call set of the loss kernels reads, as the caller holds it: fp32 tensors (pred: bf16 values, NCHW)"""
    B, _, H, W = lat.shape
    f = lambda t: None if t is None else torch.as_tensor(t, dtype=torch.float32)
    assert torch.equal(pred.float().to(BF).float(), pred.float()), "pred must hold bf16 values"
    return SimpleNamespace(method=method, lat=lat.float(), noise=noise.float(), sig=sig.float(), pred=pred.float(), prediction_type=prediction_type,
                           min_snr=bool(min_snr) and method == "ddpm", gamma=float(torch.tensor(gamma, dtype=torch.float32)), loss_type=loss_type,
                           c=float(torch.tensor(c, dtype=torch.float32)), hc=f(hc), sw=f(sw), tag=f(tag), mask=f(mask), mask_norm=mask_norm,
                           per_sample=per_sample, grad_scale=float(torch.tensor(grad_scale, dtype=torch.float32)), noise_in=f(noise_in), cond=f(cond),
                           ztsnr=ztsnr, exact=exact, B=B, H=H, W=W, HW=H * W)


def _col(t):
    return t.view(-1, 1, 1, 1)


# ------------------------------------------------------------------------------------------------ references with their bounds
def target_weight(cs):
    """(target, d_target [B,4,H,W]; w, d_w [B]) in float64 from the caller's arrays: loss_target of csrc/loss.hip"""
    x, n, sg = cs.lat.double(), cs.noise.double(), cs.sig.double()
    one = torch.ones(cs.B, dtype=F64)
    if cs.method == "flow_matching":
        tg = x - n                                              # x - n: one rounding
        return tg, U * tg.abs(), one, 0 * one
    if cs.prediction_type == 1:
        tg = (n - x) / _col(sg.abs())                           # (n - x) U; sg * sg U, halved by the sqrt; sqrtf U; the division U
        dtg = 3.5 * U * tg.abs()
    else:
        tg, dtg = n.clone(), torch.zeros_like(n)
    if not cs.min_snr:
        return tg, dtg, one, 0 * one
    snr = 1.0 / (sg * sg)                                       # inv = 1 / sg: U; inv * inv: 2 U + U
    g = torch.full_like(snr, cs.gamma)
    w = torch.minimum(snr, g)
    lo, hi = torch.minimum(snr * (1 - 3 * U), g), torch.minimum(snr * (1 + 3 * U), g)      # the interval: both ends clamped
    return tg, dtg, w, torch.maximum(hi - w, w - lo)


def _hc(cs):
    """c per sample [B] (float64)"""
    return cs.hc.double() if cs.hc is not None else torch.full((cs.B,), cs.c, dtype=F64)


def _pseudo(d, c):
    return d * d / (torch.sqrt(d * d + c * c) + c)


def _grad_shape(d, c, lt):
    q = torch.sqrt(d * d + c * c)
    return c * d / q if lt == "huber" else d / q


def element(cs):
    """d = pred - target with its bound, the element loss l(d) and the gradient shape g(d) = l'(d) / 2 with theirs (all [B,4,H,W] float64)"""
    tg, dtg, w, dw = target_weight(cs)
    d = cs.pred.double() - tg
    dd = dtg + U * (d.abs() + dtg)                              # the subtraction rounds once; the target's error goes through 1 : 1
    if cs.loss_type == "l2":
        l = d * d                                               # w * d * d: the two products are charged with the weight below
        dl = 2 * d.abs() * dd + dd * dd
        g, dg = d, dd
    else:
        c = _col(_hc(cs))
        a = d.abs()
        ph, ph_hi, ph_lo = _pseudo(a, c), _pseudo(a + dd, c), _pseudo((a - dd).clamp_min(0), c)      # monotone in |d|: the interval's ends
        # d * d U; q = sqrt(d * d + c * c): (U + U + U) / 2 + U; q + c U; the division U: 5 U at most
        k = 2 * c if cs.loss_type == "huber" else 2.0 + 0 * c      # 2 * hc is exact, its product with ph rounds once
        l = k * ph
        dl = k * (torch.maximum(ph_hi - ph, ph - ph_lo) + 5 * U * ph) + U * l
        g = _grad_shape(d, c, cs.loss_type)                     # monotone in d
        g_hi, g_lo = _grad_shape(d + dd, c, cs.loss_type), _grad_shape(d - dd, c, cs.loss_type)
        # q: 2.5 U as above; huber: hc * d U, / q U; smooth_l1: / q U
        dg = torch.maximum(g_hi - g, g - g_lo) + (4.5 if cs.loss_type == "huber" else 3.5) * U * g.abs()
    return SimpleNamespace(tg=tg, dtg=dtg, w=w, dw=dw, d=d, dd=dd, l=l, dl=dl, g=g, dg=dg)


def weight(cs, e):
    """the weight of a pixel, (s_b w_b) m, [B,1,H,W] with its RELATIVE bound: `w = sw * w` U, `w = w * mk` U, where the kernel does them"""
    Wt = _col(e.w).expand(cs.B, 1, cs.H, cs.W).clone()
    rel = _col(torch.where(e.w != 0, e.dw / e.w.abs().clamp_min(1e-300), 0 * e.w)).expand_as(Wt).clone()
    if cs.sw is not None:
        Wt, rel = Wt * _col(cs.sw.double()), rel + U
    if cs.mask is not None:
        Wt, rel = Wt * cs.mask.double().unsqueeze(1), rel + U
    return Wt, rel


def tag_mean(cs):
    """(tm, d_tm): `for (b < B) s += tag_w[b]` in order, `tm = s / B`"""
    if cs.tag is None:
        return 1.0, 0.0
    t = cs.tag.double()
    tm = float(t.sum()) / cs.B
    return tm, ((cs.B - 1) * U * float(t.abs().sum()) / cs.B + U * abs(tm))


def reference(cs):
    """every output of the three loss kernels in float64, each with its bound"""
    B, HW = cs.B, cs.HW
    e = element(cs)
    Wt, relW = weight(cs, e)
    mm = cs.mask is not None and cs.mask_norm == "masked_mean"
    nb = blocks(B, HW)
    # ---- the terms of out[1] and their errors: (w * l-part) * ... : two products for l2, one for the Huber losses (charged 2 U either way)
    T = Wt * e.l
    dT = Wt.abs() * e.dl + T.abs() * (relW + 2 * U)
    pr, n, x = cs.pred.double(), cs.noise.double(), cs.lat.double()
    h = loss_tree_depth(nb)
    side = [pr.abs(), pr * pr, n.abs(), n * n, x * x]
    out = torch.zeros(8, dtype=F64)
    dout = torch.zeros(8, dtype=F64)
    for k, t in enumerate(side):
        s = float(t.sum())
        out[2 + k], dout[2 + k] = s, h * U * s + (U * s if k in (1, 3, 4) else 0.0)      # the squares round once (pr * pr is exact: 16 bits)
    # ---- per sample
    S = T.sum(dim=(1, 2, 3))
    absS = T.abs().sum(dim=(1, 2, 3))
    hb = torch.tensor([loss_tree_depth(sample_rows(b, HW)[1] - sample_rows(b, HW)[0] + 1) for b in range(B)], dtype=F64)
    dS = hb * U * absS + dT.sum(dim=(1, 2, 3))
    numel = float(B * 4 * HW)
    if mm:
        M = cs.mask.double().sum(dim=(1, 2))
        hm = torch.tensor([loss_tree_depth(sample_rows(b, HW)[1] - sample_rows(b, HW)[0] + 1, channel_adds=False) for b in range(B)], dtype=F64)
        dM = hm * U * M                                         # m >= 0: sum|terms| = M
        live = M > 0
        Ms = torch.where(live, M, torch.ones_like(M))
        Lb = torch.where(live, S / (4 * Ms), 0 * S)             # t / (4.f * M): 4 M exact, the division U
        dLb = torch.where(live, dS / (4 * Ms) + Lb.abs() * (dM / Ms + U), 0 * S)
        sum_lb = float(Lb.sum())
        d_sum = float(dLb.sum()) + B * U * float(Lb.abs().sum())      # `sum_lb += lb` in sample order
        out[1], dout[1] = 4 * HW * sum_lb, 4 * HW * d_sum + 2 * U * abs(4 * HW * sum_lb)      # 4.f * (float)HW * sum_lb
        l, dl = sum_lb / B, d_sum / B + U * abs(sum_lb / B)
    else:
        M, dM = None, None
        Lb = S / (4.0 * HW)                                     # t / (4.f * (float)HW): the product U, the division U
        dLb = dS / (4.0 * HW) + 2 * U * Lb.abs()
        tot, atot = float(T.sum()), float(T.abs().sum())
        out[1], dout[1] = tot, h * U * atot + float(dT.sum())
        l, dl = tot / numel, float(dout[1]) / numel + 2 * U * abs(tot / numel)      # numel: one rounding at most; the division
    tm, dtm = tag_mean(cs)
    if cs.tag is not None:
        l, dl = l * tm, dl * abs(tm) + abs(l) * dtm + U * abs(l * tm)
    finite = math.isfinite(l)
    assert not finite or abs(l - LOSS_CAP) > 4 * dl, "the case sits on the guard's threshold: it decides nothing"
    guard = (not finite) or l > LOSS_CAP
    out[0], dout[0] = (LOSS_CAP, 0.0) if guard else (l, dl)
    out[7], dout[7] = (0.0, 0.0) if guard else (tm, dtm)
    # ---- d pred: k = out[7] * grad_scale * 2 / (B * 4 * HW | M_b): the product U (x 2 exact), the denominator U, the division U
    gs = cs.grad_scale
    if mm:
        kb = torch.where(live, tm * gs * 2.0 / (B * 4.0 * Ms), 0 * M)
        relk = torch.where(live, dM / Ms, 0 * M) + 3 * U + (dtm / abs(tm) if tm != 0 else 0.0)
    else:
        kb = torch.full((B,), tm * gs * 2.0 / numel, dtype=F64)
        relk = torch.full((B,), 3 * U + (dtm / abs(tm) if tm != 0 else 0.0), dtype=F64)
    if guard:
        kb = 0 * kb
    k4 = _col(kb)
    v = k4 * Wt * e.g                                           # (k * w) * d: two products
    dv = v.abs() * (_col(relk) + relW + 2 * U) + (k4 * Wt).abs() * e.dg
    zero = (k4 == 0).expand_as(v).clone()                       # the exact zeros of the design
    if cs.sw is not None:
        zero |= _col(cs.sw == 0).expand_as(v)
    if cs.mask is not None:
        zero |= (cs.mask == 0).unsqueeze(1).expand_as(v)
    v, dv = torch.where(zero, torch.zeros_like(v), v), torch.where(zero, torch.zeros_like(dv), dv)
    assert bool(torch.isfinite(v).all()), "a non-finite expectation outside the exact zeros"
    return SimpleNamespace(e=e, out=out, dout=dout, Lb=Lb, dLb=dLb, M=M, dM=dM, dpred=v, ddpred=dv, zero=zero, guard=guard, tm=tm, dtm=dtm, mm=mm)


def rows8(t_nchw):
    """[B,4,H,W] -> the token-major [B*HW][8] image, lanes 4..7 zero"""
    B, Cc, H, W = t_nchw.shape
    o = torch.zeros(B * H * W, 8, dtype=t_nchw.dtype)
    o[:, :4] = t_nchw.permute(0, 2, 3, 1).reshape(B * H * W, 4)
    return o


def reached(cs, r):
    """the wave-uniform branches of loss_fwd_kernel<LT> / loss_bwd_kernel<LT> this case takes, and the loops it trips twice"""
    HW = cs.HW
    rows = max(sample_rows(b, HW)[1] - sample_rows(b, HW)[0] + 1 for b in range(cs.B))
    tags = [f"LT={cs.loss_type}", cs.method + ("/minsnr" if cs.min_snr else ""), "sample_w" if cs.sw is not None else "-",
            "huber_cb" if cs.hc is not None else "-", f"mask/{cs.mask_norm}" if cs.mask is not None else "-", "ps_out" if cs.per_sample else "-",
            "tag_w" if cs.tag is not None else "-", "guard" if r.guard else "-", f"slots={ps_slots(cs.B, HW)}", f"rows/sample={rows}" + ("(2nd trip)" if rows > 64 else ""),
            "straddle" if HW % 256 else "aligned"]
    return " ".join(tags)


def check_all(tag, cs, got, r=None):
    """hold every output of one call set to its bound.  got: out [8] fp32, dpred [B*HW][8] bf16 (prefilled with NaN by the caller: every lane must
    be written), optional ps [B] fp32 and mnorm [B] fp32.  Returns the largest fraction of a delta that was needed."""
    r = r or reference(cs)
    assert r.guard or bool((r.dpred != 0).any()), f"{tag}: every gradient of the case is an exact zero: it decides nothing"
    frac = {}
    out = got["out"].detach().cpu().float()
    # ---- exact zeros, bit for bit: the guard taken, s_b = 0, m = 0, M_b = 0, the pad lanes
    dp = got["dpred"].detach().cpu()
    assert dp.dtype == BF and tuple(dp.shape) == (cs.B * cs.HW, 8), (tag, dp.dtype, tuple(dp.shape))
    check_bits(f"{tag} d pred pad lanes 4..7", dp[:, 4:], torch.zeros_like(dp[:, 4:]))
    z8 = rows8(r.zero.to(torch.uint8))[:, :4].bool()
    check_bits(f"{tag} d pred exact zeros ({int(z8.sum())})", dp[:, :4][z8], torch.zeros(int(z8.sum()), dtype=BF))
    frac["dpred"] = check_interval(f"{tag} d pred", dp[:, :4], rows8(r.dpred)[:, :4], rows8(r.ddpred)[:, :4])
    # ---- the eight words
    if r.guard:
        check_bits(f"{tag} out[0] (guard)", out[0:1], torch.tensor([LOSS_CAP]))
        check_bits(f"{tag} out[7] (guard)", out[7:8], torch.zeros(1))
    else:
        frac["out0"] = check_f32(f"{tag} out[0]", out[0:1], r.out[0:1], r.dout[0:1])
        frac["out7"] = check_f32(f"{tag} out[7]", out[7:8], r.out[7:8], r.dout[7:8])
        # out[0] = out[1] / numel * tm on the device's own out[1]: numel U, the division U, the product U, the tag mean's error
        o1 = float(out[1].double())
        want = o1 / float(cs.B * 4 * cs.HW) * r.tm
        check_f32(f"{tag} out[0] = out[1] / numel * tm", out[0:1], torch.tensor([want], dtype=F64), torch.tensor([abs(want) * 3 * U + abs(o1) / (cs.B * 4 * cs.HW) * r.dtm]))
    if bool(torch.isfinite(r.out[1:7]).all()):
        frac["sums"] = check_f32(f"{tag} out[1..6]", out[1:7], r.out[1:7], r.dout[1:7])
    if cs.per_sample:
        frac["Lb"] = check_f32(f"{tag} L_b", got["ps"].detach().cpu().float(), r.Lb, r.dLb)
    if r.mm and got.get("mnorm") is not None:
        frac["mnorm"] = check_f32(f"{tag} mnorm", got["mnorm"].detach().cpu().float(), r.M, r.dM)
    if cs.exact:
        check_exact(tag, cs, got, r)
    worst = max(frac.values()) if frac else 0.0
    print(f"[ops-loss] {tag} {cs.B}x{cs.H}x{cs.W}: reached {reached(cs, r)}; largest fraction of delta needed "
          + ", ".join(f"{k} {v:.3g}" for k, v in frac.items()))
    return worst


def check_exact(tag, cs, got, r):
    """an exact design: every sum is exact in fp32 whatever the order, so out[1..6], the per-sample sums and M_b have the bits of the integer
    sums and L_b is one correctly rounded division of them; d pred is ONE rounding of an exact product wherever numel is a power of two"""
    f32 = lambda t: t.float() if torch.equal(t.float().double(), t.double()) else None
    T = (weight(cs, r.e)[0] * r.e.l).flatten()
    q = next(k for k in range(60) if bool((T * 2.0 ** k == torch.floor(T * 2.0 ** k)).all()))      # every term a multiple of 2^-q ...
    assert float(T.abs().sum()) * 2.0 ** q < 2.0 ** 24, f"{tag}: the design is not exact ({float(T.abs().sum())} in units of 2^-{q})"      # ... and every partial sum fits
    sums = f32(r.out[1:7]) if not r.mm else f32(r.out[2:7])
    assert sums is not None, f"{tag}: the design is not exact (a sum does not fit fp32)"
    out = got["out"].detach().cpu().float()
    check_bits(f"{tag} exact sums", out[1:7] if not r.mm else out[2:7], sums)
    S = (weight(cs, r.e)[0] * r.e.l).sum(dim=(1, 2, 3))
    assert f32(S) is not None
    if r.mm:
        M = f32(r.M)
        assert M is not None
        if got.get("mnorm") is not None:
            check_bits(f"{tag} exact M_b", got["mnorm"].detach().cpu().float(), M)
        lb = torch.where(M == 0, torch.zeros_like(M), S.float() / (4.0 * M).clamp_min(1e-30))
    else:
        lb = S.float() / torch.tensor(4.0 * cs.HW, dtype=torch.float32)
    if cs.per_sample:
        check_bits(f"{tag} exact L_b", got["ps"].detach().cpu().float(), lb)
    numel = cs.B * 4 * cs.HW
    if numel & (numel - 1) == 0 and not r.mm and not r.guard and math.frexp(r.tm * cs.grad_scale)[0] == 0.5:
        assert f32(r.dpred) is not None
        check_bits(f"{tag} exact d pred (one rounding)", got["dpred"].detach().cpu()[:, :4], bf16_rn64(rows8(r.dpred)[:, :4]))


# ------------------------------------------------------------------------------------------------ x_in: bit-exact against separate fp32 operations
def prepare_rows(cs):
    """the UNet input [B*HW][Cs] bf16 loss_prepare_kernel writes: channels 0..3 from latents and noise_in (noise when absent) in separate fp32 torch
    ops, every product and sum rounded on its own, channels 4.. = bf16(cond), the rest zero; Cs = 8 up to 8 channels, else 16"""
    x, n = cs.lat, cs.noise_in if cs.noise_in is not None else cs.noise
    s = _col(cs.sig)
    if cs.method == "flow_matching":
        v = (1.0 - s) * n + s * x
    else:
        v = s * n + x
        if cs.ztsnr:
            v = v.clamp(-20000.0, 20000.0)
    ncond = 0 if cs.cond is None else cs.cond.shape[1]
    Cs = 8 if 4 + ncond <= 8 else 16
    o = torch.zeros(cs.B * cs.HW, Cs, dtype=BF)
    o[:, :4] = v.to(BF).permute(0, 2, 3, 1).reshape(-1, 4)
    if ncond:
        o[:, 4:4 + ncond] = cs.cond.to(BF).permute(0, 2, 3, 1).reshape(-1, ncond)
    return o


# ------------------------------------------------------------------------------------------------ the fp32 emulation and its single defects
MUTANTS = ("sigma_target", "sigma_weight", "sigma_both", "block_first_sample", "hw_for_mb", "mask_late", "huber_plain_diff", "d_bf16", "truncate",
           "pad_lane", "slot_dropped", "rows_past_64")


def emulate(cs, mutant=None, victim=0):
    """the three loss kernels' formulas in separate fp32 torch ops on the flat [B*HW][4] layout, the sums by torch.sum over (block, sample) partials:
    another order than the kernels'.  mutant: one of MUTANTS, a single defect (victim: the sample it hits)."""
    assert mutant is None or mutant in MUTANTS, mutant
    B, HW, N = cs.B, cs.HW, cs.B * cs.HW
    f32 = torch.float32
    flat = lambda t: t.view(B, 4, HW).permute(0, 2, 1).reshape(N, 4)
    x, n, pr = flat(cs.lat), flat(cs.noise), flat(cs.pred)
    pix = torch.arange(N)
    bidx = pix // HW
    if mutant == "block_first_sample":
        bidx = ((pix // 256) * 256) // HW
    nbr = (victim + 1) % B
    pick = lambda on: torch.where(bidx == victim, nbr, bidx) if on else bidx
    sg_t = cs.sig[pick(mutant in ("sigma_target", "sigma_both"))].view(N, 1)
    sg_w = cs.sig[pick(mutant in ("sigma_weight", "sigma_both"))].view(N, 1)
    if cs.method == "flow_matching":
        tg, w = x - n, torch.ones(N, 1)
    else:
        tg = (n - x) / torch.sqrt(sg_t * sg_t) if cs.prediction_type == 1 else n
        inv = 1.0 / sg_w
        w = torch.minimum(inv * inv, torch.tensor(cs.gamma)) if cs.min_snr else torch.ones(N, 1)
    d = pr - tg
    if mutant == "d_bf16":
        d = d.to(BF).float()
    sw = cs.sw[bidx].view(N, 1) if cs.sw is not None else None
    mk = None
    if cs.mask is not None:
        mk = cs.mask.reshape(N)
        if mutant == "mask_late":
            mk = torch.cat([mk[1:], mk[:1]])
        mk = mk.view(N, 1)
    if sw is not None:
        w = sw * w
    if mk is not None:
        w = w * mk
    hc = (cs.hc[bidx].view(N, 1) if cs.hc is not None else torch.full((N, 1), cs.c)) if cs.loss_type != "l2" else None
    if cs.loss_type == "l2":
        term = w * d * d
    else:
        ph = (torch.sqrt(d * d + hc * hc) - hc) if mutant == "huber_plain_diff" else d * d / (torch.sqrt(d * d + hc * hc) + hc)
        term = w * (2.0 * hc * ph) if cs.loss_type == "huber" else w * (2.0 * ph)
    assert term.dtype == f32
    nb = blocks(B, HW)
    pad = nb * 256 - N

    def by_block(t):      # [N, k] -> [nb, 256 * k], zeros past the end
        return torch.cat([t, torch.zeros(pad, t.shape[1])]).view(nb, -1)

    out = torch.zeros(8, dtype=f32)
    for k, t in enumerate([term, pr.abs(), pr * pr, n.abs(), n * n, x * x]):
        out[1 + k] = by_block(t).sum(dim=1).sum()
    mm = cs.mask is not None and cs.mask_norm == "masked_mean"
    ps, mnorm = None, None
    if cs.per_sample or mm:
        real = torch.cat([pix // HW, torch.full((pad,), -1)]).view(nb, 256)      # the sample a pixel belongs to (the slot's owner), whatever the defect reads
        tb = by_block(term).view(nb, 256, 4)
        mb = by_block(mk).view(nb, 256) if mm else None
        S, M = torch.zeros(B), torch.zeros(B)
        for b in range(B):
            sel = real == b
            P = torch.where(sel.unsqueeze(2), tb, torch.zeros_like(tb)).sum(dim=(1, 2))      # one partial per block row
            Q = torch.where(sel, mb, torch.zeros_like(mb)).sum(dim=1) if mm else None
            lo, hi = sample_rows(b, HW)
            if mutant == "slot_dropped" and b == victim:
                r3 = [r for r in range(lo, hi + 1) if b - (r * 256) // HW == 2]      # the rows in which this sample sits in the third slot
                assert r3, "no block touches three samples here"
                P[r3[0]] = 0.0
            if mutant == "rows_past_64":
                P[lo + 64:] = 0.0
                if mm:
                    Q[lo + 64:] = 0.0
            S[b] = P.sum()
            if mm:
                M[b] = Q.sum()
        if mm:
            Md = M.clone()
            if mutant == "hw_for_mb":
                Md[victim] = float(HW)
            lb = torch.where(Md == 0, torch.zeros(B), S / (4.0 * Md).clamp_min(1e-37))
            mnorm = Md
            sum_lb = torch.zeros((), dtype=f32)
            for b in range(B):
                sum_lb = sum_lb + lb[b]
            out[1] = torch.tensor(4.0 * HW, dtype=f32) * sum_lb
        else:
            lb = S / torch.tensor(4.0 * HW, dtype=f32)
        ps = lb if cs.per_sample else None
    numel = torch.tensor(float(B), dtype=f32) * 4.0 * torch.tensor(float(HW), dtype=f32)
    l = sum_lb / torch.tensor(float(B)) if mm else out[1] / numel
    tm = torch.tensor(1.0)
    if cs.tag is not None:
        s = torch.zeros((), dtype=f32)
        for b in range(B):
            s = s + cs.tag[b]
        tm = s / torch.tensor(float(B))
        l = l * tm
    if not bool(torch.isfinite(l)) or float(l) > LOSS_CAP:
        out[0], out[7] = LOSS_CAP, 0.0
    else:
        out[0], out[7] = l, tm
    # ---- backward
    gs = torch.tensor(cs.grad_scale, dtype=f32)
    k = (out[7] * gs * 2.0 / numel).expand(N).clone()
    if mm:
        Mp = mnorm[bidx]
        k = torch.where(Mp == 0, torch.zeros(N), out[7] * gs * 2.0 / (torch.tensor(float(B)) * 4.0 * Mp).clamp_min(1e-37))
    k = k.view(N, 1)
    g = d
    if cs.loss_type != "l2":
        q = torch.sqrt(d * d + hc * hc)
        g = hc * d / q if cs.loss_type == "huber" else d / q
    v = k * w * g
    zero = (k == 0).expand(N, 4).clone()
    if sw is not None:
        zero |= (sw == 0).expand(N, 4)
    if mk is not None:
        zero |= (mk == 0).expand(N, 4)
    v = torch.where(zero, torch.zeros_like(v), v)
    if mutant == "truncate":
        v16 = (v.contiguous().view(torch.int32) & ~0xFFFF).view(f32).to(BF)
    else:
        v16 = v.to(BF)
    dp = torch.zeros(N, 8, dtype=BF)
    dp[:, :4] = v16
    if mutant == "pad_lane":
        dp[N // 2, 5] = 2.0 ** -20
    return dict(out=out, ps=ps, mnorm=mnorm, dpred=dp)


def old_bars(cs, got, r=None):
    """what the aggregate bars of test_gpu_loss_ext.py / test_gpu_loss_mask.py make of a result: check_dpred's two figures (over m > 0), the loss's and
    the worst L_b's relative error.  Bars: 2^-8, 2^-8, 1e-5, 1e-5."""
    r = r or reference(cs)
    want, have = rows8(r.dpred)[:, :4], got["dpred"][:, :4].double()
    live = rows8((~r.zero).to(torch.uint8))[:, :4].bool()
    err, ref = (have - want).abs()[live], want.abs()[live]
    mx, med = float(err.max()) / float(ref.max()), float((err / ref.clamp_min(1e-30)).median())
    loss = abs(float(got["out"][0]) - float(r.out[0])) / abs(float(r.out[0]))
    lb = float(((got["ps"].double() - r.Lb).abs() / r.Lb.abs().clamp_min(1e-300)).max()) if got.get("ps") is not None else float("nan")
    passes = {"dpred": mx <= 2.0 ** -8 and med <= 2.0 ** -8, "loss": loss <= 1e-5, "L_b": not (lb > 1e-5)}
    return dict(dpred_max=mx, dpred_median=med, loss_rel=loss, lb_rel=lb, passes=passes)


# ------------------------------------------------------------------------------------------------ data
DDPM_TS = (500, 800, 900, 950)      # MinSNR weights 1.1e-5 / 0.14 / 5 / 5: five decades


def graded(method, B, H, W, seed, sig=None, cancel=False):
    """randn latents and noise, a bf16 prediction at distance ~1 from the target (cancel: pred = bf16(target), d is pure cancellation)"""
    g = torch.Generator().manual_seed(seed)
    lat, noise = torch.randn(B, 4, H, W, generator=g), torch.randn(B, 4, H, W, generator=g)
    if sig is None:
        if method == "ddpm":
            from oracle import loss_ref as R
            sig = R.karras_sigmas()[torch.tensor([DDPM_TS[b % 4] for b in range(B)])]
        else:
            sig = torch.tensor([(0.2, 0.45, 0.6, 0.85)[b % 4] for b in range(B)])
    sig = torch.as_tensor(sig, dtype=torch.float32)
    tg = (lat - noise) if method == "flow_matching" else (noise - lat) / torch.sqrt(sig * sig).view(-1, 1, 1, 1)
    pred = (tg if cancel else tg + torch.randn(B, 4, H, W, generator=g)).to(BF).float()
    return lat, noise, sig, pred


def exact_design(method, B, H, W, seed):
    """dyadic data on which every sum is exact whatever the order: integer latents, noise and predictions; ddpm with sigma in {0.5, 1, 2, 4} and
    gamma = 5 (target and weight exact: 1 / sigma^2 in {4, 1, 1/4, 1/16} < 5)"""
    g = torch.Generator().manual_seed(seed)
    ri = lambda lo, hi: torch.randint(lo, hi + 1, (B, 4, H, W), generator=g).float()
    if method == "flow_matching":
        lat, noise, pred = ri(-3, 3), ri(-3, 3), ri(-4, 4)
        sig = torch.tensor([(0.25, 0.5, 0.75, 1.0)[b % 4] for b in range(B)])
    else:
        sig = torch.tensor([(0.5, 1.0, 2.0, 4.0)[b % 4] for b in range(B)])
        mult = 4.0 if B >= 4 else 2.0 if B == 3 else 1.0      # (noise - lat) / sigma is an integer at every sigma of the batch
        lat, noise = mult * ri(-2, 2), mult * ri(-2, 2)
        pred = ri(-4, 4)
    return lat, noise, sig, pred


def exact_mask(B, H, W, seed):
    """masks in {0, 1, 2}"""
    return torch.randint(0, 3, (B, H, W), generator=torch.Generator().manual_seed(seed)).float()


def exact_weights(B, seed):
    """weights in {0.5, 1, 2}"""
    return torch.tensor([0.5, 1.0, 2.0])[torch.randint(0, 3, (B,), generator=torch.Generator().manual_seed(seed))]


def fractional_mask(B, H, W, seed, empty=0):
    m = torch.rand(B, H, W, generator=torch.Generator().manual_seed(seed))
    m = torch.where(m < 0.2, torch.zeros_like(m), m)
    if empty is not None and empty < B:
        m[empty] = 0.0
    return m


# which (method, element loss, weights, mask norm, per-sample) combination runs at which shape.  Every wave-uniform branch of loss_fwd_kernel<LT> and
# loss_bwd_kernel<LT> (sample_w, huber_cb | scalar c, mask, mask_norm == 1, ps_out, tag_w; LT = 0, 1, 2; both methods, MinSNR on and off) is reached
# at least once at a straddling shape (HW % 256 != 0).  kind: exact | graded | cancel.
TABLE = [
    # name                shape            method           lt           sw     hc     tag    mask   norm           ps     kind
    ("fm-exact-plain",    SHAPE_ONE_BLOCK, "flow_matching", "l2",        False, False, False, False, "mean",        True,  "exact"),
    ("fm-exact-all",      SHAPE_STRADDLE,  "flow_matching", "l2",        True,  False, False, True,  "mean",        True,  "exact"),
    ("ddpm-exact-mm",     SHAPE_STRADDLE,  "ddpm",          "l2",        True,  False, False, True,  "masked_mean", True,  "exact"),
    ("ddpm-exact-all5",   SHAPE_ALL5,      "ddpm",          "l2",        True,  False, False, True,  "masked_mean", True,  "exact"),
    ("fm-exact-hw1",      SHAPE_HW1,       "flow_matching", "l2",        True,  False, False, True,  "masked_mean", True,  "exact"),
    ("ddpm-exact-spill",  SHAPE_SPILL,     "ddpm",          "l2",        False, False, False, True,  "mean",        True,  "exact"),
    ("fm-exact-rows64",   SHAPE_ROWS64,    "flow_matching", "l2",        False, False, False, True,  "masked_mean", True,  "exact"),
    ("ddpm-exact-rows64", SHAPE_ROWS64,    "ddpm",          "l2",        False, False, False, False, "mean",        True,  "exact"),
    ("ddpm-l2",           SHAPE_STRADDLE,  "ddpm",          "l2",        False, False, False, False, "mean",        False, "graded"),
    ("ddpm-l2-w",         SHAPE_STRADDLE,  "ddpm",          "l2",        True,  False, True,  False, "mean",        True,  "graded"),
    ("ddpm-huber-cb",     SHAPE_STRADDLE,  "ddpm",          "huber",     True,  True,  True,  True,  "masked_mean", True,  "graded"),
    ("ddpm-smooth-c",     SHAPE_STRADDLE,  "ddpm",          "smooth_l1", False, False, False, True,  "mean",        False, "graded"),
    ("fm-huber-c",        SHAPE_ALL5,      "flow_matching", "huber",     False, False, True,  False, "mean",        True,  "graded"),
    ("fm-smooth-cb",      SHAPE_STRADDLE,  "flow_matching", "smooth_l1", True,  True,  False, True,  "masked_mean", False, "graded"),
    ("ddpm-eps-nosnr",    SHAPE_STRADDLE,  "ddpm",          "l2",        False, False, False, False, "mean",        True,  "graded"),
    ("ddpm-cancel",       SHAPE_STRADDLE,  "ddpm",          "l2",        True,  False, False, False, "mean",        True,  "cancel"),
    ("ddpm-huber-cancel", SHAPE_SPILL,     "ddpm",          "huber",     False, False, False, False, "mean",        True,  "cancel"),
    ("ddpm-hw1",          SHAPE_HW1,       "ddpm",          "smooth_l1", True,  True,  True,  False, "mean",        True,  "graded"),
    ("ddpm-bucket",       SHAPE_BUCKET,    "ddpm",          "l2",        True,  False, True,  True,  "masked_mean", True,  "graded"),
    ("ddpm-rows64",       SHAPE_ROWS64,    "ddpm",          "huber",     True,  False, False, True,  "masked_mean", True,  "graded"),
    ("fm-rows64-mean",    SHAPE_ROWS64,    "flow_matching", "l2",        False, False, True,  True,  "mean",        True,  "graded"),
]
TABLE_IDS = [t[0] for t in TABLE]


def table_case(row, seed=0):
    name, (B, H, W), method, lt, sw, hc, tag, mask, norm, ps, kind = row
    s = 1000 + 17 * TABLE_IDS.index(name) + seed
    g = torch.Generator().manual_seed(s)
    if kind == "exact":
        lat, noise, sig, pred = exact_design(method, B, H, W, s)
        kw = dict(sw=exact_weights(B, s + 1) if sw else None, mask=exact_mask(B, H, W, s + 2) if mask else None, gamma=5.0, exact=True,
                  grad_scale=0.5)
        if mask and norm == "masked_mean" and B > 1:
            kw["mask"][B - 1] = 0.0                             # M_b = 0
        if sw and B > 2:
            kw["sw"] = kw["sw"].clone()
    else:
        lat, noise, sig, pred = graded(method, B, H, W, s, cancel=kind == "cancel")
        swv = None
        if sw:
            swv = torch.rand(B, generator=g) * 2.0 + 0.05
            if B > 2 or (B == 2 and not mask):                  # s_b = 0 (at B = 2 the masked cases keep sample 1 alive: sample 0 has the empty mask)
                swv[1] = 0.0
        kw = dict(sw=swv, hc=(torch.rand(B, generator=g) * 0.5 + 0.05) if hc else None, c=0.3 if lt != "l2" else 0.0,
                  tag=(torch.rand(B, generator=g) + 0.5) if tag else None, mask=fractional_mask(B, H, W, s + 3) if mask else None, grad_scale=0.25)
        if kind == "cancel" and lt != "l2":
            kw["c"] = 0.5                                       # |d| << c
    if name == "ddpm-eps-nosnr":                                # the epsilon target (exact: the noise itself), MinSNR off
        kw.update(prediction_type=0, min_snr=False)
        pred = (noise + torch.randn(B, 4, H, W, generator=g)).to(BF).float()
    return case(method, lat, noise, sig, pred, loss_type=lt, mask_norm=norm, per_sample=ps, **kw)


# ================================================================================================ the sampler's guidance rescale
SAMPLER_SHAPES = [(1, 8, 8), (3, 13, 10), (1, 257, 256)]      # the last: HW = 65 792 = 257 partial rows, the `r += 256` second trip


def sampler_tree_depth(nblk):
    """the depth of one of the four sums over a sample, read off csrc/sampler.hip:
         4   `v[k] += ...` in sampler_stats_kernel's `for (c < 4)` loop
         6 + 3   sampler_block_sum4: wave_sum's butterfly, then `((sm[0] + sm[1]) + sm[2]) + sm[3]`
         ceil(nblk / 256)   sampler_step_kernel<RESCALE>'s `for (r = threadIdx.x; r < gridDim.x; r += 256) v[k] += row[k]`
         6 + 3   sampler_block_sum4 once more"""
    return 4 + 6 + 3 + (nblk + 255) // 256 + 6 + 3


def sampler_reference(x, fc, fu, k):
    """x_next in float64 with its per-element bound, and the cancellation factors Q / (Q - S^2 / n) of the two one-pass variances.
    x fp32 [B,4,H,W], fc / fu bf16 values (fu None: no cfg), k the scalar fields (fp32-rounded floats)."""
    B, _, H, W = x.shape
    HW, n = H * W, 4.0 * H * W
    h = sampler_tree_depth((HW + 255) // 256)
    a = fc.double()
    if k["cfg"]:
        u, g = fu.double(), float(k["guidance"])
        t = a - u
        gt = g * t
        f = u + gt
        df = 2 * U * gt.abs() + U * f.abs()                     # t U, g * t U, fu + t U
    else:
        f, df = a, torch.zeros_like(a)
    dims = (1, 2, 3)

    def var(s_terms, ds_terms, q_terms, dq_terms):
        S, Q = s_terms.sum(dims), q_terms.sum(dims)
        dS = h * U * s_terms.abs().sum(dims) + ds_terms.sum(dims)
        dQ = h * U * Q + dq_terms.sum(dims)
        A = S * S / n                                           # v * v U, / n U
        dA = 2 * S.abs() * dS / n + 2 * U * A
        N = Q - A
        dN = dQ + dA + U * N.abs()                              # the cancellation: dN / N = (Q / N) (dQ + dA) / Q
        v = N / (n - 1)                                         # n - 1.f U, the division U
        return v, dN / (n - 1) + 2 * U * v.abs(), Q / N.clamp_min(1e-300)

    vc, dvc, cc = var(a, 0 * a, a * a, 0 * a)                   # bf16 x bf16 is exact in fp32
    vf, dvf, cf = var(f, df, f * f, 2 * f.abs() * df + U * f * f)
    live = (vc - dvc > 0) & (vf - dvf > 0)
    dead = (vc + dvc <= 0) | (vf + dvf <= 0) | ((vc == 0) & (dvc == 0)) | ((vf == 0) & (dvf == 0))
    assert bool((live | dead).all()), "a sample's variance straddles zero inside its bound: the case decides nothing"
    sc, sf = vc.clamp_min(1e-300).sqrt(), vf.clamp_min(1e-300).sqrt()
    r = torch.where(live, sc / sf, torch.ones_like(sc))
    dr = torch.where(live, r * (dvc / (2 * vc.clamp_min(1e-300)) + dvf / (2 * vf.clamp_min(1e-300)) + 3 * U), torch.zeros_like(r))      # two sqrtf, the division
    r4, dr4 = r.view(-1, 1, 1, 1), dr.view(-1, 1, 1, 1)
    phi = float(k["guidance_rescale"])
    t1 = f * r4
    dt1 = f.abs() * dr4 + df * r4 + U * t1.abs()
    t1, dt1 = phi * t1, abs(phi) * dt1 + U * (phi * t1).abs()
    t2 = (1 - phi) * f
    dt2 = abs(1 - phi) * df + 2 * U * t2.abs()                  # 1.f - phi U, the product U
    F = t1 + t2
    dF = dt1 + dt2 + U * F.abs()
    xd = x.double()
    d1, d2 = k["a_skip"] * xd, k["a_out"] * F
    den = d1 + d2
    dden = U * d1.abs() + abs(k["a_out"]) * dF + U * d2.abs() + U * den.abs()
    u1, u2 = k["p"] * xd, k["q"] * den
    xn = u1 + u2
    dxn = U * u1.abs() + abs(k["q"]) * dden + U * u2.abs() + U * xn.abs()
    return SimpleNamespace(x=xn, dx=dxn, ratio=r, dratio=dr, cancel_c=cc, cancel_f=cf, live=live)


SAMPLER_MUTANTS = ("rows_past_256", "n_for_n1")


def sampler_emulate(x, fc, fu, k, mutant=None):
    """the rescale step in separate fp32 torch ops, the four sums by torch.sum over the blocks' partial rows (another order than the kernel's)"""
    import _sampler_ref as R
    B, _, H, W = x.shape
    HW = H * W
    a = fc.float()
    f = R.guide(a, fu.float() if k["cfg"] else None, k["guidance"])
    nblk = (HW + 255) // 256
    pad = nblk * 256 - HW

    def total(t):      # [B,4,H,W] -> [B]
        rows = torch.cat([t.view(B, 4, HW), torch.zeros(B, 4, pad)], dim=2).view(B, 4, nblk, 256).sum(dim=(1, 3))      # [B, nblk]
        if mutant == "rows_past_256":
            rows = rows[:, :256]
        return rows.sum(dim=1)

    n = torch.tensor(4.0 * HW, dtype=torch.float32)
    def var(t, den):
        S, Q = total(t), total(t * t)
        return (Q - S * S / n) / den

    # (n for n - 1 in BOTH variances leaves the ratio alone: the defect sits in one of the kernel's two expressions)
    vc, vf = var(a, n if mutant == "n_for_n1" else n - 1.0), var(f, n - 1.0)
    ok = (vc > 0) & (vf > 0)
    ratio = torch.where(ok, torch.sqrt(vc.clamp_min(0)) / torch.sqrt(vf.clamp_min(1e-45)), torch.ones_like(vc)).view(-1, 1, 1, 1)
    phi = torch.tensor(k["guidance_rescale"], dtype=torch.float32)
    t1 = f * ratio
    t1 = phi * t1
    t2 = (1.0 - phi) * f
    F = t1 + t2
    return R.step(x, F, k["a_skip"], k["a_out"], k["p"], k["q"])


def sampler_data(B, H, W, mean_over_std, seed):
    """fc, fu (bf16) with mean / std of the guided F about `mean_over_std`, x fp32"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, 4, H, W, generator=g) * 3.0
    fc = (torch.randn(B, 4, H, W, generator=g) + mean_over_std).to(BF)
    fu = (torch.randn(B, 4, H, W, generator=g) + mean_over_std).to(BF)
    return x, fc, fu


def sampler_constant_f(B, H, W, seed):
    """F_c in {0, 2}, F_u = 2 F_c - 1, guidance 2: F = F_u + 2 (F_c - F_u) = 1 everywhere, every sum exact: var(F) = 0 exactly, var(F_c) > 0"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, 4, H, W, generator=g)
    fc = (2 * torch.randint(0, 2, (B, 4, H, W), generator=g)).float()
    return x, fc.to(BF), (2 * fc - 1).to(BF)


def sampler_pm1(B, H, W, seed):
    """F_c = F_u = +-1: the four sums are integers, the two variances equal, the ratio exactly 1"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, 4, H, W, generator=g)
    fc = (2 * torch.randint(0, 2, (B, 4, H, W), generator=g) - 1).float().to(BF)
    return x, fc, fc.clone()
