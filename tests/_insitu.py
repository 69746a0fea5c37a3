"""The in-situ audit: every op of a finished training step recomputed from the operands it actually had.

The plan map (sdxl_debug_plan_op, lib.plan_map) says where every op of the plan reads and writes; the workspace, the weight arena and the fp32
gradient arena are caller memory.  After one synchronised step this module takes plain CPU copies of the three (an Image), reads each op's
operands out of them, computes the op in float64 and holds each of its outputs to the per-element bound that the op tests already derive
(tests/_exact.py, _nonlinear.py, _temb.py).  The reference sees the engine's own operands, so rounding does not accumulate from layer to layer:
what is judged is one op and the engine's decisions around it -- offsets, leading dimensions, column slices, addends, aliases, pad rows, eps,
the accumulate flag -- at op-test tightness.  Nothing here needs a GPU: tests/test_host_insitu.py runs it on an emulated image.

The checks (no measured tolerance):
  bf16 output   bf16_rn(ref - delta) <= got <= bf16_rn(ref + delta) for every element (the one final rounding gets no slack),
  fp32 output   |got - ref| <= delta + 2^-24 |ref|,
  copies        bit equality; one addition of two bf16 values: the bits of bf16(fp32(a) + fp32(b)), which fp32 torch reproduces.
delta by kind:
  linear / conv forward, dgrad, weight and bias gradient: K 2^-23 (|A| . |B| + |bias| + |resid| + |rowvec| + |addend| + |arena before|), K the
      reduction length (tests/_exact.py: fp32 accumulation in any order, split-K included).  Restated double roundings, by design:
        * the stride-2 dgrad WITH an addend stores bf16 phase planes first: + 2^-8 |acc|, K = 4 Cout (four taps reach an input pixel);
        * the up-convolution folds its nine taps onto 16 bf16 weights: + 2^-8 |x| . |w| (forward and dgrad; K = 9 Cin, 36 Cout);
        * the GEGLU second projection's dgrad rounds dG = dY W to bf16 in its epilogue and multiplies then: the result is linear in dG, so it lies
          between the values at bf16_rn(dG - d) and bf16_rn(dG + d), widened by geglu_bwd_ref's own bound;
      pad rows: where both operands of a weight gradient carry pad rows and M + pad is a multiple of 64 the reduction runs over M + pad rows, and the
      pad rows of BOTH operands must be exact zeros after the step;
      the grouped time-embedding projection's output gradient is the bf16 cast of the fp32 sums (dy32_off): bit equality with that cast, and each
      convolution's slice of the sums is held to _temb.colsum_bound;
  GroupNorm / LayerNorm: _nonlinear.gn_*_ref / ln_*_ref; the backward is fed the stored statistics, the stored statistics are held to the forward's;
  GEGLU activation: geglu_fwd_ref on the stored u;  attention: attn_fwd_ref / attn_bwd_ref on the stored lse and O, Delta held to its bound in
      either form (its own pass, or the out-projection's dgrad epilogue);
  SiLU: silu64 / silu_grad64 with their deltas (+ one product, + one addition with an addend);  nearest-2x backward: 4 (5) fp32 additions;
  the loss seam (kind "loss", audit_seam): the UNet input bit for bit from the caller's arrays (from their staged copies in graph mode, each copy
      bit-equal to the caller's array), the loss words, L_b, M_b and every lane of d pred from the prediction as it sits in the workspace, by
      _loss_elem.reference's bounds."""
from __future__ import annotations

from collections import namedtuple

import torch

import _exact as X
import _loss_elem as LE
import _nonlinear as NL
import _temb as TE

BF, F64, U = torch.bfloat16, torch.float64, NL.U
Result = namedtuple("Result", "op kind role ratio n ok msg")
Image = namedtuple("Image", "ws w g g0 accumulate", defaults=(None, False))
Image.__doc__ = """ws: uint8 workspace bytes; w: bf16 weight arena; g: fp32 gradient arena after the step; g0: the arena before the backward
(None: zeros for the bias / norm vectors, which sdxl_zero_grads clears, and nothing for the matrices); accumulate: first_micro was False"""

# (kind, role, reason): the ONLY (op, role) pairs the audit may leave out, and only where intact_after_step says the buffer is gone
OMISSIONS = [
    ("upsample", "y", "the consuming up-convolution reads x directly; where its weight gradient does too the upsampled image is never produced"),
    ("linear", "dx", "diagnostics knob 26 = 1: the dgrad's epilogue runs the LayerNorm's backward on its accumulators and stores that op's input "
                     "gradient instead of its own (audited there, from this op's operands)"),
]


# ------------------------------------------------------------------------------------------------ reading the images
def bf_at(img, off, rows, cols, ld):
    n = ((rows - 1) * ld + cols) * 2
    return img.ws[off: off + n].view(BF).as_strided((rows, cols), (ld, 1))


def f32_at(img, off, n):
    return img.ws[off: off + 4 * n].view(torch.float32)


def data(img, t, rows=None):
    return bf_at(img, t["off"], t["rows"] if rows is None else rows, t["cols"], t["ld"])


def grad(img, off, t, rows=None):
    """the gradient of tensor t at byte offset `off` (its own or one of a (out, addend) pair: same shape and stride)"""
    return None if off is None else bf_at(img, off, t["rows"] if rows is None else rows, t["cols"], t["ld"])


def warena(img, off, n):
    return img.w[off: off + n].double()


def g_before(img, off, n, small):
    """what the gradient arena held before this backward: small (bias / norm) vectors always accumulate (zero_grads cleared them when g0 is None);
    matrices are overwritten on the first micro-step and accumulated onto afterwards"""
    if img.g0 is None:
        assert small or not img.accumulate, "an accumulating micro-step needs the arena image from before it"
        return torch.zeros(n, dtype=F64)
    if small or img.accumulate:
        return img.g0[off: off + n].double()
    return torch.zeros(n, dtype=F64)


# ------------------------------------------------------------------------------------------------ the three checks, as results
def _first(bad, *vals):
    i = int(bad.flatten().nonzero()[0])
    return f"first at flat index {i}: " + ", ".join(f"{k} {float(v.flatten()[i])!r}" for k, v in vals)


def r_interval(d, role, got, ref, delta):
    ref = ref.double()
    delta = torch.as_tensor(delta, dtype=F64).expand_as(ref)
    assert got.dtype == BF and got.shape == ref.shape, (d["index"], d["kind"], role, got.dtype, tuple(got.shape), tuple(ref.shape))
    assert bool((delta >= 0).all()) and not bool(torch.isnan(ref).any()), f"op {d['index']} {d['kind']} {role}: the expectation itself is broken"
    g = got.double()
    lo, hi = NL.bf16_rn64(ref - delta).double(), NL.bf16_rn64(ref + delta).double()
    bad = torch.isnan(g) | (g < lo) | (g > hi)
    ratio = float(NL._ratio_bf16(got.contiguous(), ref, delta, ~bad).max()) if got.numel() else 0.0
    msg = "" if not bool(bad.any()) else f"{int(bad.sum())} of {got.numel()} outside; " + _first(bad, ("got", g), ("ref", ref), ("delta", delta), ("lo", lo), ("hi", hi))
    return Result(d["index"], d["kind"], role, ratio, got.numel(), not bool(bad.any()), msg)


def r_f32(d, role, got, ref, delta):
    ref = ref.double()
    delta = torch.as_tensor(delta, dtype=F64).expand_as(ref)
    assert got.dtype == torch.float32 and got.shape == ref.shape, (d["index"], d["kind"], role, got.dtype, tuple(got.shape), tuple(ref.shape))
    g = got.double()
    allowed = delta + U * ref.abs()
    err = (g - ref).abs()
    bad = torch.isnan(g) | ~(err <= allowed)
    q = torch.where(err == 0, torch.zeros_like(err), err / allowed.clamp_min(1e-300))
    ratio = float(torch.nan_to_num(q, nan=float("inf"), posinf=float("inf")).max()) if got.numel() else 0.0
    msg = "" if not bool(bad.any()) else f"{int(bad.sum())} of {got.numel()} outside; " + _first(bad, ("got", g), ("ref", ref), ("allowed", allowed))
    return Result(d["index"], d["kind"], role, ratio, got.numel(), not bool(bad.any()), msg)


def r_bits(d, role, got, want):
    ok = X.same_bits(got.contiguous(), want.contiguous())
    msg = ""
    if not ok:
        bad = got.contiguous().view(torch.int16 if got.dtype == BF else torch.int32) != want.contiguous().view(torch.int16 if want.dtype == BF else torch.int32)
        msg = f"{int(bad.sum())} of {got.numel()} differ; " + _first(bad, ("got", got.double()), ("want", want.double()))
    return Result(d["index"], d["kind"], role, 0.0 if ok else float("inf"), got.numel(), ok, msg)


def add_bf16(a, b):
    """what add_kernel / split_add_kernel / the residual adds store: bf16(fp32(a) + fp32(b)), IEEE arithmetic that fp32 torch reproduces bit for bit"""
    return (a.float() + b.float()).to(BF)


def gemm_delta(K, absdot):
    """X.bound's accumulation term: K 2^-23 (|A| . |B| + |addends|); the final rounding is the interval's (bf16) or 2^-24 |ref| (fp32)"""
    return K * 2.0 ** -23 * absdot


# ------------------------------------------------------------------------------------------------ linear
def _pad_of(d):
    """rows that the weight gradient appends to both operands (LinearOp::bwd): min of the two pad counts where M + pad is a multiple of 64"""
    x, y = d["t"][0], d["t"][1]
    pad = min(x["pad_rows"], y["pad_rows"])
    return pad if pad > 0 and (x["rows"] + pad) % 64 == 0 else 0


def audit_linear(d, img):
    out = []
    x, y, resid, gact, gu = d["t"]
    M, K, N = x["rows"], d["K"], d["N"]
    assert y["rows"] == M and x["cols"] == K and y["cols"] == N, (d["index"], x, y, K, N)
    X_, W = data(img, x).double(), warena(img, d["w_off"], N * K).view(N, K)
    b = warena(img, d["b_off"], N) if d["b_off"] is not None else None
    ref, ab = X_ @ W.T, X_.abs() @ W.abs().T
    if b is not None:
        ref, ab = ref + b, ab + b.abs()
    if resid is not None:
        r = data(img, resid).double()
        ref, ab = ref + r, ab + r.abs()
    out.append(r_interval(d, "y", data(img, y), ref, gemm_delta(K, ab)))
    if gact is not None:      # the GEGLU activation from the stored u: value | gate interleaved in groups of ggroup
        C4, G = N // 2, d["ggroup"]
        u = NL.geglu_unpack_cols(data(img, y).float().contiguous(), C4, G)
        gref, gdel = NL.geglu_fwd_ref(u[:, :C4], u[:, C4:])
        out.append(r_interval(d, "gact", data(img, gact), gref, gdel))
    # ---- backward
    if d["dy_off"] is None:
        return out
    dy_b = grad(img, d["dy_off"], y)
    dy = dy_b.double()
    if d["dy32_off"] is not None:      # the fp32 sums the convolutions left, cast once
        out.append(r_bits(d, "dy_cast", dy_b, f32_at(img, d["dy32_off"], M * N).view(M, N).to(BF)))
    if resid is not None:
        if not d["resid_alias"]:      # (aliased: the residual's gradient IS dy, no launch -- chain_results judges the alias)
            out.append(r_bits(d, "dres", grad(img, d["dres_out"], resid), add_bf16(grad(img, d["dres_addend"], resid), dy_b)))
    pad = _pad_of(d)
    if pad:
        zx = bf_at(img, x["off"] + M * x["ld"] * 2, pad, K, x["ld"])
        zy = bf_at(img, d["dy_off"] + M * y["ld"] * 2, pad, N, y["ld"])
        out.append(r_bits(d, "x_pad", zx, torch.zeros_like(zx)))
        out.append(r_bits(d, "dy_pad", zy, torch.zeros_like(zy)))
    # weight and bias gradients: reduction over M (+ pad) rows, onto what the arena held
    base = g_before(img, d["w_off"], N * K, False).view(N, K)
    got = img.g[d["w_off"]: d["w_off"] + N * K].view(N, K)
    worst = []
    for n0 in range(0, N, 2048):      # (row blocks: the grouped K | V weight is 15 360 x 2048)
        s = slice(n0, min(n0 + 2048, N))
        wr, wa = dy[:, s].T @ X_ + base[s], dy[:, s].abs().T @ X_.abs() + base[s].abs()
        worst.append(r_f32(d, "dw", got[s], wr, gemm_delta(M + pad, wa)))
    out.append(_merge(worst))
    if b is not None:
        bb = g_before(img, d["b_off"], N, True)
        out.append(r_f32(d, "db", img.g[d["b_off"]: d["b_off"] + N], dy.sum(0) + bb, gemm_delta(M + pad, dy.abs().sum(0) + bb.abs())))
    # input gradient
    if d["dx_out"] is not None and d["intact_after_step"] & (1 << 8):
        if gu is None:
            acc, aab = dy @ W, dy.abs() @ W.abs()
            if d["dx_addend"] is not None:
                a = grad(img, d["dx_addend"], x).double()
                acc, aab = acc + a, aab + a.abs()
            out.append(r_interval(d, "dx", grad(img, d["dx_out"], x), acc, gemm_delta(N, aab)))
        else:      # dU = the GEGLU backward of bf16(dG), dG = dY W (module docstring)
            C4, G = K, d["ggroup"]
            dG, dd = dy @ W, gemm_delta(N, dy.abs() @ W.abs())
            lo, hi = NL.bf16_rn64(dG - dd).double(), NL.bf16_rn64(dG + dd).double()
            u = NL.geglu_unpack_cols(data(img, gu).float().contiguous(), C4, G)
            v, t = u[:, :C4], u[:, C4:]
            ra0, da0, rt0, dt0 = NL.geglu_bwd_ref(lo, v, t)
            ra1, da1, rt1, dt1 = NL.geglu_bwd_ref(hi, v, t)
            mid = lambda p, q: (p + q) / 2
            half = lambda p, q, e0, e1: (p - q).abs() / 2 + torch.maximum(e0, e1)
            refu = NL.geglu_pack_cols(mid(ra0, ra1), mid(rt0, rt1), G)
            delu = NL.geglu_pack_cols(half(ra0, ra1, da0, da1), half(rt0, rt1, dt0, dt1), G)
            out.append(r_interval(d, "dx", grad(img, d["dx_out"], gu), refu, delu))
    return out


def _merge(rs):
    bad = [r for r in rs if not r.ok]
    r0 = rs[0]
    return Result(r0.op, r0.kind, r0.role, max(r.ratio for r in rs), sum(r.n for r in rs), not bad, bad[0].msg if bad else "")


# ------------------------------------------------------------------------------------------------ convolution
def _nhwc(t2d, B, H, W):
    return t2d.reshape(B, H, W, t2d.shape[-1])


def audit_conv(d, img):
    out = []
    x, y, resid, rowvec, x_low = d["t"]
    B, H, W, Cin, Cout, s = d["B"], d["H"], d["W"], d["Cin"], d["Cout"], d["stride"]
    Ho, Wo = (H - 1) // s + 1, (W - 1) // s + 1
    Wn = warena(img, d["w_off"], Cout * 9 * Cin).view(Cout, 9, Cin)
    b = warena(img, d["b_off"], Cout)
    up2 = bool(d["up2"])
    if up2:
        assert s == 1 and resid is None and rowvec is None
        xin = X.upsample2x_nhwc(_nhwc(data(img, x_low).double(), B, H // 2, W // 2))
    else:
        xin = _nhwc(data(img, x).double(), B, H, W)
    ref = X.conv_ref64(xin, Wn, b, s)
    ab_nb = X.conv_ref64(xin.abs(), Wn.abs(), None, s)
    ab = ab_nb + b.abs()
    if rowvec is not None:
        assert d["rows_per_batch"] == Ho * Wo and rowvec["ld"] == d["ldvec"]
        v = data(img, rowvec).double()[:, None, None, :]
        ref, ab = ref + v, ab + v.abs()
    if resid is not None:
        r = _nhwc(data(img, resid).double(), B, Ho, Wo)
        ref, ab = ref + r, ab + r.abs()
    delta = gemm_delta(9 * Cin, ab) + (2.0 ** -8 * ab_nb if up2 else 0.0)
    out.append(r_interval(d, "y", data(img, y), ref.reshape(-1, Cout), delta.reshape(-1, Cout)))
    if d["dy_off"] is None:
        return out
    dy_b = grad(img, d["dy_off"], y)
    dy = _nhwc(dy_b.double(), B, Ho, Wo)
    if resid is not None:
        if not d["resid_alias"]:      # (aliased: the residual's gradient IS dy, no launch -- chain_results judges the alias)
            out.append(r_bits(d, "dres", grad(img, d["dres_out"], resid), add_bf16(grad(img, d["dres_addend"], resid), dy_b)))
    # weight gradient: the nine taps over the (upsampled) input; bias gradient: the column sums
    Mo = B * Ho * Wo
    base = g_before(img, d["w_off"], Cout * 9 * Cin, False).view(Cout, 9, Cin)
    wr, wa = X.conv_wgrad_ref64(xin, dy, s) + base, X.conv_wgrad_ref64(xin.abs(), dy.abs(), s) + base.abs()
    out.append(r_f32(d, "dw", img.g[d["w_off"]: d["w_off"] + Cout * 9 * Cin].view(Cout, 9, Cin), wr, gemm_delta(Mo, wa)))
    bb = g_before(img, d["b_off"], Cout, True)
    out.append(r_f32(d, "db", img.g[d["b_off"]: d["b_off"] + Cout], dy.sum((0, 1, 2)) + bb, gemm_delta(Mo, dy.abs().sum((0, 1, 2)) + bb.abs())))
    if rowvec is not None:      # this convolution's slice of the fp32 [B][sum Cout] sums: per-sample column sums of dy (zeroed at the start of the backward)
        assert d["d3_addend"] is None, "the row vector has another gradient writer"
        got = f32_at(img, d["rv32_off"], (B - 1) * d["ldvec"] + Cout).as_strided((B, Cout), (d["ldvec"], 1))
        cs, ca = dy.sum((1, 2)), dy.abs().sum((1, 2))
        # _temb.colsum_bound = (rows - 1) 2^-24 sum|x| + 2^-24 |result|: the second term is r_f32's own, so it is asked for with a zero result
        out.append(r_f32(d, "drowvec", got, cs, TE.colsum_bound(TE.CS(B, Ho * Wo, Cout), ca, torch.zeros_like(cs))))
    if d["dx_out"] is not None:
        tgt = x_low if up2 else x
        acc, aab = X.conv_dgrad_ref64(dy, Wn, H, W, s), X.conv_dgrad_ref64(dy.abs(), Wn.abs(), H, W, s)
        if up2:
            acc, aab = X.upsample2x_bwd_nhwc(acc), X.upsample2x_bwd_nhwc(aab)
        K = 36 * Cout if up2 else (4 * Cout if s == 2 else 9 * Cout)
        extra = 2.0 ** -8 * aab if up2 else 0.0
        refx, abx = acc, aab
        if d["dx_addend"] is not None:
            a = _nhwc(grad(img, d["dx_addend"], tgt).double(), *acc.shape[:3])
            refx, abx = acc + a, aab + a.abs()
            if d["s2_dgrad"]:
                extra = 2.0 ** -8 * acc.abs()
        out.append(r_interval(d, "dx", grad(img, d["dx_out"], tgt), refx.reshape(-1, Cin), (gemm_delta(K, abx) + extra).reshape(-1, Cin)))
    return out


# ------------------------------------------------------------------------------------------------ norms
def audit_groupnorm(d, img):
    out = []
    x, y = d["t"][0], d["t"][1]
    B, HW, C, G = d["B"], d["H"], d["Cin"], d["groups"]
    xs = data(img, x).float().reshape(B, HW, C)
    gm, bt = warena(img, d["w_off"], C).float(), warena(img, d["b_off"], C).float()
    f = NL.gn_fwd_ref(xs, gm, bt, G, float(d["eps"]), d["silu"])
    out.append(r_interval(d, "y", data(img, y), f["y"].reshape(-1, C), f["dy"].reshape(-1, C)))
    st = f32_at(img, d["stats_off"], B * G * 2).view(B, G, 2)
    out.append(r_f32(d, "mean", st[..., 0].contiguous(), f["mean"], f["dmean"]))
    out.append(r_f32(d, "rstd", st[..., 1].contiguous(), f["rstd"], f["drstd"]))
    if d["dy_off"] is None:
        return out
    dy = grad(img, d["dy_off"], y).float().reshape(B, HW, C)
    add = None if d["dx_addend"] is None else grad(img, d["dx_addend"], x).float().reshape(B, HW, C)
    r = NL.gn_bwd_ref(xs, dy, gm, bt, st, G, d["silu"], addend=add)
    out.append(r_interval(d, "dx", grad(img, d["dx_out"], x), r["dx"].reshape(-1, C), r["ddx"].reshape(-1, C)))
    out += _norm_params(d, img, r, C)
    return out


def _norm_params(d, img, r, C):
    res = []
    for role, off, key in (("dgamma", d["w_off"], "dgamma"), ("dbeta", d["b_off"], "dbeta")):
        base = g_before(img, off, C, True)
        res.append(r_f32(d, role, img.g[off: off + C], r[key] + base, r["d" + key] + U * base.abs()))
    return res


def audit_layernorm(d, img, consumer=None):
    """consumer: the linear op whose dgrad epilogue runs this LayerNorm's backward (ln_mode 1 / 2, diagnostics knob 26).  The epilogue rounds its
    accumulators dy = dY W to bf16 BY DESIGN and runs the backward on those values (csrc/gemm.hip; tests/test_gpu_ops.py restates the same); in mode
    1 they are not stored.  Restated: with e = gemm_delta(N, |dY| . |W|) the rounded dy lies in [lo, hi] = [bf16_rn(dy - e), bf16_rn(dy + e)] (one
    value for most elements, two neighbours next to a rounding boundary); the reference takes the midpoint, and because the backward is LINEAR in dy
    the half width eb = (hi - lo) / 2 reaches the outputs as  dx: rstd (g + mean(g) + |h| mean(g |h|)), g = |gamma| eb;  dgamma: sum_rows eb |h|;
    dbeta: sum_rows eb  -- exactly, not to first order."""
    out = []
    x, y = d["t"][0], d["t"][1]
    M, C = x["rows"], d["Cin"]
    xs = data(img, x).float()
    gm, bt = warena(img, d["w_off"], C).float(), warena(img, d["b_off"], C).float()
    f = NL.ln_fwd_ref(xs, gm, bt, float(d["eps"]))
    out.append(r_interval(d, "y", data(img, y), f["y"], f["dy"]))
    st = f32_at(img, d["stats_off"], M * 2).view(M, 2)
    out.append(r_f32(d, "mean", st[:, 0].contiguous(), f["mean"], f["dmean"]))
    out.append(r_f32(d, "rstd", st[:, 1].contiguous(), f["rstd"], f["drstd"]))
    if d["dy_off"] is None:
        return out
    add = None if d["dx_addend"] is None else grad(img, d["dx_addend"], x).float()
    stored = bool(d["intact_after_step"] & (1 << 9))
    if d["ln_mode"]:
        assert consumer is not None and consumer["ln_mode"] == d["ln_mode"] and consumer["t"][0]["off"] == y["off"], "fused LayerNorm without its consumer"
        cy, Nc = consumer["t"][1], consumer["N"]
        dyc = grad(img, consumer["dy_off"], cy).double()
        Wc = warena(img, consumer["w_off"], Nc * C).view(Nc, C)
        dy64, e = dyc @ Wc, gemm_delta(Nc, dyc.abs() @ Wc.abs())
        if stored:      # (mode 2: dy is stored too -- the same bf16 values the epilogue works on -- and the parameter gradients take their own pass over it)
            out.append(r_interval(d, "dy_stored", grad(img, d["dy_off"], y), dy64, e))
            r = NL.ln_bwd_ref(xs, grad(img, d["dy_off"], y).float(), gm, st, addend=add)
            out.append(r_interval(d, "dx", grad(img, d["dx_out"], x), r["dx"], r["ddx"]))
            return out + _norm_params(d, img, r, C)
        lo, hi = NL.bf16_rn64(dy64 - e).double(), NL.bf16_rn64(dy64 + e).double()
        dym, eb = (lo + hi) / 2, (hi - lo) / 2
        mean, rstd = st[:, :1].double(), st[:, 1:2].double()
        h = ((xs.double() - mean) * rstd).abs()
        g = gm.double().abs()[None, :] * eb
        r = NL.ln_bwd_ref(xs, dym, gm, st, addend=add)
        ex = rstd * (g + g.mean(1, keepdim=True) + h * (g * h).mean(1, keepdim=True))
        out.append(r_interval(d, "dx", grad(img, d["dx_out"], x), r["dx"], r["ddx"] + ex))
        r = dict(r, ddgamma=r["ddgamma"] + (eb * h).sum(0), ddbeta=r["ddbeta"] + eb.sum(0))
        return out + _norm_params(d, img, r, C)
    dy = grad(img, d["dy_off"], y).float()
    r = NL.ln_bwd_ref(xs, dy, gm, st, addend=add)
    out.append(r_interval(d, "dx", grad(img, d["dx_out"], x), r["dx"], r["ddx"]))
    out += _norm_params(d, img, r, C)
    return out


# ------------------------------------------------------------------------------------------------ attention
def audit_attn(d, img):
    out = []
    q, o, _, kv, _ = d["t"]
    B, heads, Nq, Nk, C = d["B"], d["heads"], d["Nq"], d["Nk"], d["Cin"]
    assert heads * 64 == C and q["rows"] == B * Nq and kv["rows"] == B * Nk and o["cols"] == C
    if d["self_attn"]:
        assert q["off"] == kv["off"] and q["cols"] == 3 * C and d["ldq"] == d["ldk"] == d["ldv"] == q["ld"]
        qo, ko, vo, ldk = q["off"], q["off"] + 2 * C, q["off"] + 4 * C, q["ld"]
    else:
        assert q["cols"] == C and kv["cols"] == 2 * C and d["ldk"] == d["ldv"] == kv["ld"] and d["ldq"] == q["ld"]
        qo, ko, vo, ldk = q["off"], kv["off"], kv["off"] + 2 * C, kv["ld"]
    ops = dict(q=bf_at(img, qo, B * Nq, C, q["ld"]).float().reshape(B, Nq, C), k=bf_at(img, ko, B * Nk, C, ldk).float().reshape(B, Nk, C),
               v=bf_at(img, vo, B * Nk, C, ldk).float().reshape(B, Nk, C))
    f = NL.attn_fwd_ref(ops, heads)
    lse = f32_at(img, d["lse_off"], B * heads * Nq).view(B * heads, Nq)
    out.append(r_f32(d, "lse", lse, f["lse"], f["dlse"]))
    o_b = data(img, o)
    out.append(r_interval(d, "o", o_b, f["o"].reshape(-1, C), f["do"].reshape(-1, C)))
    if d["dy_off"] is None:
        return out
    ops["dO"] = grad(img, d["dy_off"], o).float().reshape(B, Nq, C)
    r = NL.attn_bwd_ref(ops, heads, lse, o_b.reshape(B, Nq, C))
    # Delta: its own pass or the out-projection's dgrad epilogue (delta_fused), the same sum of 64 exact products either way
    out.append(r_f32(d, "delta_fused" if d["delta_fused"] else "delta", f32_at(img, d["delta_off"], B * heads * Nq).view(B * heads, Nq), r["delta"], r["ddelta"]))
    assert d["dx_addend"] is None and d["d3_addend"] is None
    if d["self_attn"]:
        go, ldg = d["dx_out"], q["ld"]
        offs = (go, go + 2 * C, go + 4 * C)
        lds = (ldg, ldg, ldg)
    else:
        offs, lds = (d["dx_out"], d["d3_out"], d["d3_out"] + 2 * C), (q["ld"], kv["ld"], kv["ld"])
    for role, off, ld, n, key in (("dq", offs[0], lds[0], Nq, "dq"), ("dk", offs[1], lds[1], Nk, "dk"), ("dv", offs[2], lds[2], Nk, "dv")):
        out.append(r_interval(d, role, bf_at(img, off, B * n, C, ld), r[key].reshape(-1, C), r["d" + key].reshape(-1, C)))
    return out


# ------------------------------------------------------------------------------------------------ data movement and SiLU
def audit_silu(d, img):
    x, y = d["t"][0], d["t"][1]
    n = data(img, x).double()
    out = [r_interval(d, "y", data(img, y), NL.silu64(n), NL.silu_delta(n, torch.zeros_like(n)))]
    if d["dy_off"] is None:
        return out
    ref, delta = NL.silu_bwd_ref(n, grad(img, d["dy_off"], y), None if d["dx_addend"] is None else grad(img, d["dx_addend"], x))
    out.append(r_interval(d, "dx", grad(img, d["dx_out"], x), ref, delta))
    return out


def audit_concat(d, img):
    a, o, _, b, _ = d["t"]
    Ca = a["cols"]
    ob = data(img, o)
    out = [r_bits(d, "o", ob, torch.cat([data(img, a), data(img, b)], 1))]
    if d["dy_off"] is None:
        return out
    do = grad(img, d["dy_off"], o)
    for role, t, sl, dst, add in (("d_a", a, slice(0, Ca), d["dx_out"], d["dx_addend"]), ("d_b", b, slice(Ca, None), d["d3_out"], d["d3_addend"])):
        want = do[:, sl] if add is None else add_bf16(do[:, sl], grad(img, add, t))
        out.append(r_bits(d, role, grad(img, dst, t), want))
    return out


def audit_upsample(d, img):
    x, y = d["t"][0], d["t"][1]
    B, H, W, C = d["B"], d["H"], d["W"], d["Cin"]
    out = []
    if d["intact_after_step"] & (1 << 1):
        want = X.upsample2x_nhwc(_nhwc(data(img, x), B, H, W)).reshape(-1, C)
        out.append(r_bits(d, "y", data(img, y), want))
    if d["dy_off"] is None or d["up2"]:      # (up2: the consuming convolution's dgrad writes dx -- audited there)
        return out
    g = _nhwc(grad(img, d["dy_off"], y).double(), B, 2 * H, 2 * W)
    ref, delta = X.upsample2x_bwd_ref64(g, None if d["dx_addend"] is None else _nhwc(grad(img, d["dx_addend"], x).double(), B, H, W))
    out.append(r_interval(d, "dx", grad(img, d["dx_out"], x), ref.reshape(-1, C), delta.reshape(-1, C)))
    return out


def audit_embed_in(d, img, tail):
    te, aug, _, tid, _ = d["t"]
    B, ch0, ad, pooled = d["B"], d["dims"][0], d["dims"][1], d["dims"][2]
    out = []
    ref, delta = TE.sincos_ref(f32_at(img, tail["t_off"], B), ch0)
    out.append(r_interval(d, "te_sin", data(img, te), ref, delta))
    ref, delta = TE.sincos_ref(f32_at(img, tail["tid_off"], 6 * B), ad)
    out.append(r_interval(d, "tid_emb", data(img, tid), ref, delta))
    out.append(r_bits(d, "aug_in", data(img, aug)[:, pooled:], data(img, tid).reshape(B, 6 * ad)))
    # the other half of aug_in is the caller's pooled embedding, staged by the forward call: the bits of its bf16 value (tail["pooled_in"]: the
    # caller's array as the test handed it over, [B][pooled_dim])
    want = tail["pooled_in"].to(BF).reshape(B, pooled)
    out.append(r_bits(d, "aug_pooled", data(img, aug)[:, :pooled], want))
    return out


AUDITS = {"linear": audit_linear, "conv": audit_conv, "groupnorm": audit_groupnorm, "layernorm": audit_layernorm, "attn": audit_attn,
          "silu": audit_silu, "concat": audit_concat, "upsample": audit_upsample}


def audit_op(d, img, tail=None, ops=None):
    """[Result] for every output of one op (ops: the whole plan, where a fused LayerNorm finds its consumer)"""
    if d["kind"] == "embed_in":
        return audit_embed_in(d, img, tail)
    if d["kind"] == "layernorm" and d["ln_mode"]:
        cons = [o for o in (ops or []) if o["kind"] == "linear" and o["ln_mode"] and o["t"][0]["off"] == d["t"][1]["off"]]
        return audit_layernorm(d, img, cons[0] if len(cons) == 1 else None)
    return AUDITS[d["kind"]](d, img)


# ------------------------------------------------------------------------------------------------ the loss seam
STAGED = (("in_lat_off", "lat"), ("in_noise_off", "noise"), ("in_nin_off", "noise_in"), ("in_sig_off", "sig"), ("in_tag_off", "tag"), ("in_sw_off", "sw"),
          ("in_hc_off", "hc"), ("in_mask_off", "mask"), ("in_cond_off", "cond"))
SEAM_ROLES = ("x_in_wired", "x_in", "dpred_wired", "dpred_pad", "dpred_zeros", "dpred", "loss_words", "gate")      # what every plan's seam must show
SEAM_KIND = "loss"


def audit_seam(ops, tail, img):
    """The seam between the caller's batch and the audited UNet.  tail["loss"]: plan = lib.plan_loss's dict, caller = the arrays and options as the
    caller handed them to forward_loss (lat, noise, sig and the optional noise_in, tag, sw, hc, mask, cond; method, prediction_type, min_snr, gamma,
    ztsnr, loss_type, c, mask_norm, per_sample), grad_scale = the backward's.
    Role x_in: conv_in reads tail.x_in, which is the bit-exact image of the caller's arrays; in graph mode every staged copy has the caller's bits
    and the image is recomputed from the COPIES.  Role dpred: the last op writes tail.pred and reads its gradient at tail.pred.goff; the loss
    words, L_b, M_b and d pred (pad lanes included) are recomputed from pred as it sits in the workspace; the gate word out[7] -- the one
    cond_dgrad, input_dgrad and the residual gradients read at loss_off + 28 -- is the one checked here."""
    s = tail["loss"]
    pl, c = s["plan"], dict(s["caller"])
    d = {"index": len(ops), "kind": SEAM_KIND}
    B, H, W = tail["B"], tail["H"], tail["W"]
    flag = lambda role, msg: Result(d["index"], SEAM_KIND, role, 0.0 if not msg else float("inf"), 0, not msg, msg)
    out = []
    xin, pred = tail["x_in"], tail["pred"]
    convs = [o for o in ops if o["kind"] == "conv"]
    first, last = convs[0], ops[-1]
    same = lambda t, u: (t["off"], t["rows"], t["cols"], t["ld"]) == (u["off"], u["rows"], u["cols"], u["ld"])
    out.append(flag("x_in_wired", "" if same(first["t"][0], xin) else f"the first convolution (op {first['index']}) reads {first['t'][0]}, not tail.x_in {xin}"))
    wired = same(last["t"][1], pred) and pred["goff"] is not None and last["dy_off"] == pred["goff"]
    out.append(flag("dpred_wired", "" if wired else f"the last op (op {last['index']}) writes {last['t'][1]} and reads dy at {last['dy_off']}; tail.pred is {pred}"))
    # ---- the staged copies
    if pl["staged"] == 1:
        rs = []
        for key, name in STAGED:
            if c.get(name) is None:
                continue
            want = c[name].float().contiguous().flatten()
            if pl[key] is None:
                rs.append(flag("staged", f"the plan has no staging buffer {key} for the caller's {name}"))
                continue
            got = f32_at(img, pl[key], want.numel())
            r = r_bits(d, "staged", got, want)
            rs.append(r._replace(msg=f"{key}: {r.msg}" if r.msg else ""))
            c[name] = got.clone().view(c[name].shape)          # ... and the audit recomputes from the copy
        out.append(_merge(rs))
    elif pl["staged"] != 0:
        out.append(flag("staged", "no forward_loss has run on this plan"))
    opts = dict(prediction_type=c.get("prediction_type", 1), min_snr=c.get("min_snr", True), gamma=c.get("gamma", 5.0), ztsnr=c.get("ztsnr", True))
    zero = torch.zeros(B, 4, H, W)
    cs0 = LE.case(c["method"], c["lat"], c["noise"], c["sig"], zero, noise_in=c.get("noise_in"), cond=c.get("cond"), **opts)
    want = LE.prepare_rows(cs0)
    got = data(img, xin)
    out.append(r_bits(d, "x_in", got, want) if got.shape == want.shape else flag("x_in", f"tail.x_in is {tuple(got.shape)}, the caller's arrays make {tuple(want.shape)}"))
    # ---- the loss words and d pred from pred as it sits in the workspace
    rows = data(img, pred)
    pn = rows[:, :4].float().view(B, H * W, 4).permute(0, 2, 1).reshape(B, 4, H, W)
    cs = LE.case(c["method"], c["lat"], c["noise"], c["sig"], pn, loss_type=c.get("loss_type", "l2"), c=c.get("c", 0.0), hc=c.get("hc"), sw=c.get("sw"),
                 tag=c.get("tag"), mask=c.get("mask"), mask_norm=c.get("mask_norm", "mean"), per_sample=c.get("per_sample", False),
                 grad_scale=s.get("grad_scale", 1.0), **opts)
    r = LE.reference(cs)
    dp = grad(img, pred["goff"], pred) if pred["goff"] is not None else None
    if dp is None:
        return out + [flag("dpred", "tail.pred has no gradient")]
    out.append(r_bits(d, "dpred_pad", dp[:, 4:], torch.zeros_like(dp[:, 4:])))
    z8 = LE.rows8(r.zero.to(torch.uint8))[:, :4].bool()
    out.append(r_bits(d, "dpred_zeros", dp[:, :4][z8], torch.zeros(int(z8.sum()), dtype=BF)))
    out.append(r_interval(d, "dpred", dp[:, :4], LE.rows8(r.dpred)[:, :4], LE.rows8(r.ddpred)[:, :4]))
    o8 = f32_at(img, tail["loss_off"], 8)
    if r.guard:
        out.append(r_bits(d, "loss_words", o8[0:1], torch.tensor([LE.LOSS_CAP])))
        out.append(r_bits(d, "gate", o8[7:8], torch.zeros(1)))
    else:
        out.append(r_f32(d, "loss_words", o8[0:7], r.out[0:7], r.dout[0:7]))
        out.append(r_f32(d, "gate", o8[7:8], r.out[7:8], r.dout[7:8]))
    if cs.per_sample:
        out.append(r_f32(d, "L_b", f32_at(img, pl["ps_loss_off"], B), r.Lb, r.dLb) if pl["ps_loss_off"] is not None else flag("L_b", "the plan has no per-sample buffer"))
    if r.mm:
        out.append(r_f32(d, "mnorm", f32_at(img, pl["mask_norm_off"], B), r.M, r.dM) if pl["mask_norm_off"] is not None else flag("mnorm", "the plan has no normaliser"))
    return out


def audit(ops, tail, img):
    out = chain_results(ops)
    if "loss" in tail:      # (a tail without it: coverage reports the seam as missing)
        out += audit_seam(ops, tail, img)
    ups = {d["t"][0]["off"]: d for d in ops if d["kind"] == "upsample" and d["up2"]}
    for d in ops:
        rs = audit_op(d, img, tail, ops)
        out += rs
        if d["kind"] == "conv" and d["up2"] and d["t"][4]["off"] in ups:
            # the nearest-2x backward of a fused pair is INSIDE the up-convolution's dgrad (it writes UpsampleOp::dx; the op itself launches
            # nothing): that result is the upsample op's backward output too
            u = ups[d["t"][4]["off"]]
            out += [r._replace(op=u["index"], kind="upsample", role="dx_in_upconv") for r in rs if r.role == "dx"]
    return out


# ------------------------------------------------------------------------------------------------ the gradient chains
def contributions(d):
    """[(role, tensor, out, addend, alias)] in the order the op's plan_bwd asks for them: which gradient buffer this op writes for each of its
    inputs, and what it adds it to.  alias: the input's gradient is dy itself (no launch)."""
    if d["dy_off"] is None:
        return []
    t, k, c = d["t"], d["kind"], []
    if k in ("linear", "conv") and t[2] is not None:
        c.append(("dres", t[2], d["dy_off"], None, True) if d["resid_alias"] else ("dres", t[2], d["dres_out"], d["dres_addend"], False))
    if k == "linear":
        tgt = t[4] if t[4] is not None else t[0]
        if d["dx_out"] is not None:
            c.append(("dx", tgt, d["dx_out"], d["dx_addend"], False))
    elif k == "conv":
        if t[3] is not None:
            c.append(("drowvec", t[3], d["d3_out"], d["d3_addend"], False))
        if d["dx_out"] is not None:
            c.append(("dx", t[4] if d["up2"] else t[0], d["dx_out"], d["dx_addend"], False))
    elif k in ("groupnorm", "layernorm", "silu"):
        c.append(("dx", t[0], d["dx_out"], d["dx_addend"], False))
    elif k == "upsample":
        if not d["up2"]:
            c.append(("dx", t[0], d["dx_out"], d["dx_addend"], False))
    elif k == "attn":
        c.append(("dq", t[0], d["dx_out"], d["dx_addend"], False))
        if not d["self_attn"]:
            c.append(("dk", t[3], d["d3_out"], d["d3_addend"], False))
    elif k == "concat":
        c += [("d_a", t[0], d["dx_out"], d["dx_addend"], False), ("d_b", t[3], d["d3_out"], d["d3_addend"], False)]
    return c


def chain_results(ops):
    """Gradient buffers are write-once: walking the plan in reverse, the FIRST contribution to a tensor's gradient has no addend (or is an alias of
    the consumer's dy), every later one adds itself to the buffer the previous one wrote, and the last buffer is the gradient the tensor's
    producer reads.  One Result per contribution (role + "_chain"): a residual aliased where another consumer had already contributed, an addend
    that is not the previous writer's buffer, or a final buffer that is not the tensor's gradient each break the chain at the op that did it."""
    last, out = {}, []
    for d in reversed(ops):
        for role, t, o, addend, alias in contributions(d):
            key = (t["off"], t["cols"])
            prev = last[key][0] if key in last else None
            msg = ""
            if o is None:
                msg = "no gradient buffer for an input that needs one"
            elif addend != prev:
                msg = f"addend {addend} is not the buffer the previous contribution wrote ({prev})" + (": aliased instead of added" if alias else "")
            last[key] = (o, t["goff"], d, role)
            out.append(Result(d["index"], d["kind"], role + "_chain", 0.0 if not msg else float("inf"), 0, not msg, msg))
    for key, (o, goff, d, role) in last.items():
        if o != goff:
            out.append(Result(d["index"], d["kind"], role + "_chain", float("inf"), 0, False, f"the last buffer written ({o}) is not the tensor's gradient ({goff})"))
    return out


# ------------------------------------------------------------------------------------------------ coverage
def expected_roles(d):
    """every output the op has according to its descriptor alone (independent of the audit functions): (role, lost), lost = intact_after_step
    says that the buffer the role needs is gone"""
    k, t, bwd = d["kind"], d["t"], d["dy_off"] is not None
    intact = lambda role, grad_: bool(d["intact_after_step"] & (1 << (role + (8 if grad_ else 0))))
    r = []
    if k == "linear":
        r += [("y", False)] + ([("gact", False)] if t[3] is not None else [])
        if bwd:
            r += [("dw", False)] + ([("db", False)] if d["b_off"] is not None else []) + ([("dy_cast", False)] if d["dy32_off"] is not None else [])
            r += [("dres", False)] if t[2] is not None and not d["resid_alias"] else []      # (aliased: no launch, the chain result judges it)
            r += [("x_pad", False), ("dy_pad", False)] if _pad_of(d) else []
            r += [("dx", not intact(0, True))] if d["dx_out"] is not None else []
    elif k == "conv":
        r += [("y", False)]
        if bwd:
            r += [("dw", False), ("db", False)] + ([("dres", False)] if t[2] is not None and not d["resid_alias"] else [])
            r += [("drowvec", False)] if t[3] is not None else []
            r += [("dx", False)] if d["dx_out"] is not None else []
    elif k in ("groupnorm", "layernorm"):
        r += [("y", False), ("mean", False), ("rstd", False)]
        if bwd:
            r += [("dx", False), ("dgamma", False), ("dbeta", False)]
    elif k == "attn":
        r += [("lse", False), ("o", False)]
        if bwd:
            r += [("delta_fused" if d["delta_fused"] else "delta", False), ("dq", False), ("dk", False), ("dv", False)]
    elif k == "silu":
        r += [("y", False)] + ([("dx", False)] if bwd else [])
    elif k == "concat":
        r += [("o", False)] + ([("d_a", False), ("d_b", False)] if bwd else [])
    elif k == "upsample":
        r += [("y", not intact(1, False))]
        r += [("dx_in_upconv", False)] if d["up2"] else ([("dx", False)] if bwd else [])      # (up2: the op launches nothing, the up-convolution's dgrad writes dx)
    elif k == "embed_in":
        r += [("te_sin", False), ("tid_emb", False), ("aug_in", False), ("aug_pooled", False)]
    else:
        raise KeyError(k)
    r += [(role + "_chain", False) for role, *_ in contributions(d)]      # every gradient contribution has its place in a chain
    return r


PARAM_ROLES = {"dw": "w", "db": "b", "dgamma": "w", "dbeta": "b"}      # the roles that are parameter gradients, and which arena range each fills
PARAM_KINDS = ("linear", "conv", "groupnorm", "layernorm")


FWD = {"y", "gact", "mean", "rstd", "lse", "o", "te_sin", "tid_emb", "aug_in", "aug_pooled"}      # forward roles; every other role is a backward's
BORROWED = {"dx_in_upconv"}      # results that another op's audit produced: they account for the role, never for an audited instance of the kind


def audited_kinds(ops, results):
    """({kinds with an output of their OWN audited in the forward}, {... in the backward}): an omission and a borrowed result do not count"""
    kind = {d["index"]: d["kind"] for d in ops}
    f = {kind[r.op] for r in results if r.op in kind and r.role in FWD}
    b = {kind[r.op] for r in results if r.op in kind and r.role not in FWD and r.role not in BORROWED and not r.role.endswith("_chain")}
    return f, b


def coverage(ops, results, param_ranges, kinds=None):
    """problems (a list of strings, empty = covered): an op index or a role with no result that is not a listed omission of a lost buffer; an op
    kind (of `kinds`, default: those in the plan) with no audited forward or no audited backward output; a parameter tensor whose arena range no
    audited gradient accounts for.  Also returns the omissions taken."""
    problems, taken = [], []
    have = {}
    for r in results:
        have.setdefault(r.op, set()).add(r.role)
    listed = {(k, role) for k, role, _ in OMISSIONS}
    fwd_kinds, bwd_kinds, covered = set(), set(), []
    for d in ops:
        got = have.get(d["index"], set())
        if not got:
            problems.append(f"op {d['index']} ({d['kind']}): no audited output")
            continue
        for role, lost in expected_roles(d):
            if role in got:
                if role not in BORROWED:
                    (fwd_kinds if role in FWD else bwd_kinds).add(d["kind"])
                if role in PARAM_ROLES:
                    off = d[PARAM_ROLES[role] + "_off"]
                    covered.append((off, off + d[PARAM_ROLES[role] + "_numel"]))
            elif lost and (d["kind"], role) in listed:
                taken.append((d["index"], d["kind"], role))
            else:
                problems.append(f"op {d['index']} ({d['kind']}): role {role} is neither audited nor a listed omission of a lost buffer")
    seam = {r.role for r in results if r.kind == SEAM_KIND}
    for role in SEAM_ROLES:      # the loss seam is part of every plan: without its roles the step is not covered
        if role not in seam:
            problems.append(f"the loss seam: role {role} is not audited")
    fwd_kinds, bwd_kinds = audited_kinds(ops, results)
    for k in (kinds if kinds is not None else {d["kind"] for d in ops}):
        if k not in fwd_kinds:
            problems.append(f"kind {k}: no audited forward output")
        if k not in bwd_kinds and k != "embed_in":      # (embed_in: inputs only, no gradient)
            problems.append(f"kind {k}: no audited backward output")
    covered.sort()
    for name, (off, cnt) in param_ranges.items():
        pos = off
        for a, b in covered:
            if a <= pos < b:
                pos = b
            if pos >= off + cnt:
                break
        if pos < off + cnt:
            problems.append(f"parameter {name}: gradient elements from {pos} of [{off}, {off + cnt}) belong to no audited op")
    return problems, taken


# ------------------------------------------------------------------------------------------------ what a case reached
def reach(ops):
    """the plan features a case reached (the [insitu-reach] line)"""
    f = set()
    for d in ops:
        if d["kind"] in ("linear", "conv"):
            if d["fsplit"] > 1:
                f.add("fsplit>1")
            if d["dsplit"] > 1:
                f.add("dsplit>1")
            if d["t"][2] is not None and d["dy_off"] is not None and not d["resid_alias"]:
                f.add("non-aliased residual")
        if d["kind"] == "linear":
            if _pad_of(d):
                f.add("pad rows")
            if d["wgroup"] > 1:
                f.add("grouped wgrad")
            if d["crcfg"]:
                f.add("crcfg")
            if d["delta_on"]:
                f.add("delta_on")
            if d["dy32_off"] is not None:
                f.add("dy32_off")
            if d["ln_mode"]:
                f.add(f"ln_mode {d['ln_mode']}")
            if d["t"][3] is not None:
                f.add(f"geglu group {d['ggroup']}")
        if d["kind"] == "conv":
            if d["three_tap"]:
                f.add("three-tap")
            if d["up2"]:
                f.add("up2" + (" + wgrad" if d["up_wg"] else ""))
            if d["s2_dgrad"]:
                f.add("s2 dgrad")
        if d["kind"] == "attn" and d["dy_off"] is not None:
            f.add(("self" if d["self_attn"] else "cross") + " attention: " + {0: "dq + dkv", 1: "dq + split dkv + reduce", 2: "fused", 3: "pipelined"}.get(d["bwd_route"], "unknown"))
            f.add("Delta fused" if d["delta_fused"] else "Delta pass")
    return sorted(f)


def summarize(results):
    """{kind: (worst ratio, outputs, elements)} for the [insitu] lines"""
    s = {}
    for r in results:
        w, n, e = s.get(r.kind, (0.0, 0, 0))
        s[r.kind] = (max(w, r.ratio), n + 1, e + r.n)
    return s


def failures(results):
    return [f"op {r.op} {r.kind} {r.role}: worst err / allowed {r.ratio:.4g}; {r.msg}" for r in results if not r.ok]
