"""The in-situ audit (tests/_insitu.py) on the CPU: a faithful image passes every check, and each of fourteen seeded single defects of the kind that
tests/test_gpu_model.py's aggregate bars let through is caught by a named (op, role).  No GPU.

The image: one resnet (GroupNorm + SiLU, 3x3 convolution with the time-embedding row vector, GroupNorm + SiLU, 3x3 convolution with the resnet's
shortcut projection as residual) and one transformer block (LayerNorm, fused q | k | v projection, self attention, out-projection + residual, LayerNorm, q
projection, the prompt-side K | V projection with pad rows -- the block reads a column slice of it --, cross attention, out-projection + residual,
LayerNorm, the GEGLU pair), planned the way the engine plans (Plan::new_act / view / grad_dst / grad_alias restated in MiniPlan: write-once gradient
buffers, aliased residuals, slices of a parent's gradient) and laid out at the offsets the descriptors name.  The emulated engine: the GEMMs and
convolutions are fp32 torch ops, the norms, activations and the softmax float64 torch ops rounded to fp32 (an engine whose fp32 arithmetic is
exact to one rounding -- written independently of the references in _nonlinear.py: torch's group_norm / layer_norm / silu / erf and autograd),
every activation stored as bf16, the by-design roundings (scale8 of q / k, bf16 dG in the GEGLU backward) made where the kernels make them."""
import ctypes as C
import math

import pytest
import torch
import torch.nn.functional as F

import sdxl_amd  # noqa: F401
from sdxl_amd import lib

import _insitu as IS
import _loss_elem as LE
import _nonlinear as NL

BF = torch.bfloat16
NAN16 = 0x7FC1
B, HH, WW, CH, CTX, CROSS, TEMB, G = 2, 4, 4, 128, 5, 64, 64, 32
HW, M, HEADS = HH * WW, B * HH * WW, CH // 64
KV_PAD = (64 - (B * CTX) % 64) % 64
EPS = float(torch.tensor(1e-5, dtype=torch.float32))


def rnd(*shape, seed, scale=1.0):
    return (torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale).to(BF)


class MiniPlan:
    """Plan's memory and reverse planning restated (csrc/engine.hip): 256-byte aligned allocations, write-once gradient buffers"""

    def __init__(self):
        self.cursor, self.pcursor, self.ops = 0, 0, []

    def alloc(self, nbytes):
        off = self.cursor
        self.cursor = (self.cursor + nbytes + 255) // 256 * 256
        return off

    def act(self, rows, cols, pad_rows=0):
        return dict(off=self.alloc((rows + pad_rows) * cols * 2), goff=None, rows=rows, cols=cols, ld=cols, pad_rows=pad_rows, col0=0, parent=None)

    def view(self, parent, col0, cols):
        return dict(off=parent["off"] + 2 * col0, goff=None, rows=parent["rows"], cols=cols, ld=parent["cols"], pad_rows=0, col0=col0, parent=parent)

    def grad_dst(self, a):
        p = a["parent"]
        if p is not None:
            if p["goff"] is None:
                p["goff"] = self.alloc((p["rows"] + p["pad_rows"]) * p["cols"] * 2)
            addend, a["goff"] = a["goff"], p["goff"] + 2 * a["col0"]
            return a["goff"], addend
        addend, a["goff"] = a["goff"], self.alloc(a["rows"] * a["cols"] * 2)
        return a["goff"], addend

    def param(self, n):
        off = self.pcursor
        self.pcursor = (self.pcursor + n + 63) // 64 * 64
        return off, n

    def op(self, kind, **kw):
        d = dict(kind=kind, index=len(self.ops), seg=0, hoist_fwd=0, resid_alias=0, intact_after_step=0xFFFFFFFF, K=0, N=0, splitk=1, wgroup=1, crcfg=0,
                 crsplit=1, fsplit=1, dsplit=1, delta_on=0, ln_mode=0, ggroup=64, B=0, H=0, W=0, Cin=0, Cout=0, stride=1, up2=0, up_fs=1, up_ds=1, up_ws=1,
                 up_wg=0, three_tap=0, rows_per_batch=0, s2_dgrad=0, groups=0, silu=0, heads=0, Nq=0, Nk=0, self_attn=0, qsplit=1, delta_fused=0,
                 bwd_route=0, skip=0, first=0, dims=[0, 0, 0, 0], eps=0.0, ldq=0, ldk=0, ldv=0, ldvec=0, dy_off=None, dx_out=None, dx_addend=None,
                 dres_out=None, dres_addend=None, d3_out=None, d3_addend=None, dy32_off=None, w_off=None, w_numel=0, b_off=None, b_numel=0,
                 stats_off=None, lse_off=None, delta_off=None, rv32_off=None, planar_off=None, weff_off=None, dweff_off=None, s2_planar_off=None,
                 t=[None] * 5)
        d.update(kw)
        self.ops.append(d)
        return d

    def plan_bwd(self):
        """each op's plan_bwd, in reverse"""
        for d in reversed(self.ops):
            t, k = d["t"], d["kind"]
            d["dy_off"] = t[1]["goff"]
            if k in ("linear", "conv") and t[2] is not None:
                if t[2]["goff"] is None:
                    t[2]["goff"], d["resid_alias"] = t[1]["goff"], 1
                else:
                    d["dres_out"], d["dres_addend"] = self.grad_dst(t[2])
            if k == "conv" and t[3] is not None:
                d["d3_out"], d["d3_addend"] = self.grad_dst(t[3])
            if k == "attn":
                d["dx_out"], d["dx_addend"] = self.grad_dst(t[0])
                if not d["self_attn"]:
                    d["d3_out"], d["d3_addend"] = self.grad_dst(t[3])
            elif k == "linear" and t[4] is not None:
                d["dx_out"], d["dx_addend"] = self.grad_dst(t[4])
            elif t[0].get("need_grad", True):
                d["dx_out"], d["dx_addend"] = self.grad_dst(t[0])


def strip(ops):
    """descriptors as lib.plan_map hands them out: tensors without the planner's private keys"""
    out = []
    for d in ops:
        e = dict(d)
        e["t"] = [None if t is None else {k: t[k] for k in ("off", "goff", "rows", "cols", "ld", "pad_rows", "col0")} for t in d["t"]]
        out.append(e)
    return out


# ------------------------------------------------------------------------------------------------ the loss seam's caller
SEAM_GRAD_SCALE = 64.0      # d pred of order 1 at numel = 128, like the gradient the image used to be seeded with


def seam_caller():
    """the batch as a caller hands it to forward_loss: ddpm, an input noise of its own, a fractional mask under masked_mean, sample and tag weights,
    per-sample Huber c, per-sample losses"""
    g = torch.Generator().manual_seed(31)
    lat, noise = torch.randn(B, 4, HH, WW, generator=g), torch.randn(B, 4, HH, WW, generator=g)
    return dict(method="ddpm", lat=lat, noise=noise, noise_in=noise + 0.1 * torch.randn(B, 4, HH, WW, generator=g), sig=torch.tensor([0.8, 2.5]),
                tag=torch.tensor([0.5, 1.25]), sw=torch.tensor([1.5, 0.75]), hc=torch.tensor([0.3, 0.6]), mask=LE.fractional_mask(B, HH, WW, seed=32, empty=None),
                loss_type="huber", mask_norm="masked_mean", per_sample=True)


def seam_case(c, pred):
    return LE.case(c["method"], c["lat"], c["noise"], c["sig"], pred, noise_in=c.get("noise_in"), loss_type=c["loss_type"], hc=c["hc"], sw=c["sw"], tag=c["tag"],
                   mask=c["mask"], mask_norm=c["mask_norm"], per_sample=True, grad_scale=SEAM_GRAD_SCALE)


# ------------------------------------------------------------------------------------------------ the image
class Mem:
    def __init__(self, nbytes, nparam):
        self.ws = torch.empty(nbytes // 2, dtype=torch.int16).fill_(NAN16).view(torch.uint8)      # every byte a NaN until somebody writes it
        self.w = torch.zeros(nparam, dtype=BF)
        self.g0 = torch.randn(nparam, generator=torch.Generator().manual_seed(99))               # a non-zero arena from "the step before"
        self.g = self.g0.clone()

    def img(self, accumulate=False):
        return IS.Image(self.ws, self.w, self.g, self.g0, accumulate)

    def bf(self, off, rows, cols, ld):
        return IS.bf_at(self, off, rows, cols, ld)

    def f32(self, off, n):
        return IS.f32_at(self, off, n)


def put(mem, off, t, value, rows=None):
    mem.bf(off, t["rows"] if rows is None else rows, t["cols"], t["ld"]).copy_(value.to(BF))


def get(mem, off, t):
    return mem.bf(off, t["rows"], t["cols"], t["ld"])


def build(defect=None):
    """(ops, tail, image) of one emulated step; defect: one of DEFECTS, applied where the engine would have made it"""
    p = MiniPlan()
    D = lambda name: defect == name
    # ---- forward plan
    emb = dict(p.act(B, TEMB), need_grad=False)
    x_in = dict(p.act(M, 8), need_grad=False)                     # the loss preparation's image: 4 channels + 4 zero lanes
    x0 = p.act(M, CH)
    ehs = dict(p.act(B * CTX, CROSS, KV_PAD), need_grad=False)
    tp_all = p.act(B, CH + 64)
    tp32_off = p.alloc(4 * B * (CH + 64))
    o_tp = p.op("linear", t=[emb, tp_all, None, None, None], K=TEMB, N=CH + 64, dy32_off=tp32_off)
    rowvec = p.view(tp_all, 64, CH)
    feat = p.act(M, CH)                                           # conv_in: the plan's first convolution reads x_in (nothing here reads its output)
    o_cin = p.op("conv", t=[x_in, feat, None, None, None], B=B, H=HH, W=WW, Cin=8, Cout=CH)

    def gn(x, silu):
        y = p.act(M, CH)
        return y, p.op("groupnorm", t=[x, y, None, None, None], B=B, H=HW, Cin=CH, groups=G, silu=silu, eps=EPS, stats_off=p.alloc(4 * B * G * 2))

    def ln(x):
        y = p.act(M, CH)
        return y, p.op("layernorm", t=[x, y, None, None, None], Cin=CH, eps=EPS, stats_off=p.alloc(4 * M * 2))

    def lin(x, N, resid=None, y=None, **kw):
        y = p.act(x["rows"], N, x["pad_rows"]) if y is None else y
        return y, p.op("linear", t=[x, y, resid, kw.pop("gact", None), kw.pop("gu", None)], K=x["cols"], N=N, **kw)

    def conv(x, resid=None, rv=None):
        y = p.act(M, CH)
        return y, p.op("conv", t=[x, y, resid, rv, None], B=B, H=HH, W=WW, Cin=CH, Cout=CH, rows_per_batch=HW if rv else 0, ldvec=rv["ld"] if rv else 0)

    n1, o_gn1 = gn(x0, 1)
    c1, o_c1 = conv(n1, rv=rowvec)
    n2, o_gn2 = gn(c1, 1)
    sc, o_sc = lin(x0, CH)                                        # conv_shortcut: its input also feeds later ops, so its dgrad has an addend
    r, o_c2 = conv(n2, resid=sc)
    l1, o_ln1 = ln(r)
    qkv, o_qkv = lin(l1, 3 * CH)
    a1 = p.act(M, CH)
    o_sa = p.op("attn", t=[qkv, a1, None, qkv, None], B=B, heads=HEADS, Nq=HW, Nk=HW, Cin=CH, self_attn=1, ldq=3 * CH, ldk=3 * CH, ldv=3 * CH,
                lse_off=p.alloc(4 * B * HEADS * HW), delta_off=p.alloc(4 * B * HEADS * HW))
    x1, o_out1 = lin(a1, CH, resid=x0)                            # (x0's gradient already has a writer when this op is planned: a real add)
    l2, o_ln2 = ln(x1)
    q, o_q = lin(l2, CH)
    kv_all, o_kv = lin(ehs, 4 * CH, hoist_fwd=1)                  # two blocks' K | V; this block reads the second slice
    kv = p.view(kv_all, 2 * CH, 2 * CH)
    a2 = p.act(M, CH)
    o_ca = p.op("attn", t=[q, a2, None, kv, None], B=B, heads=HEADS, Nq=HW, Nk=CTX, Cin=CH, ldq=CH, ldk=4 * CH, ldv=4 * CH,
                lse_off=p.alloc(4 * B * HEADS * HW), delta_off=p.alloc(4 * B * HEADS * HW))
    x2, o_out2 = lin(a2, CH, resid=x0)                            # (the last reader of x0: aliased)
    l3, o_ln3 = ln(x2)
    u = p.view(p.act(M, 8 * CH + 64), 0, 8 * CH)                  # Builder::wide_act
    gact = p.view(p.act(M, 4 * CH + 64), 0, 4 * CH)
    _, o_ff1 = lin(l3, 8 * CH, y=u, gact=gact)
    yout, o_ff2 = lin(gact, CH, resid=x2, gu=u)
    gact["need_grad"] = False                                     # (the activation gets no gradient buffer: the dgrad emits dU)
    pred = p.act(M, 8)                                            # conv_out: the plan's last op writes the prediction, 4 channels + 4 zero lanes
    o_cout = p.op("conv", t=[yout, pred, None, None, None], B=B, H=HH, W=WW, Cin=CH, Cout=8)
    loss_off, ps_loss_off, mask_norm_off = p.alloc(32), p.alloc(4 * B), p.alloc(4 * B)
    caller = seam_caller()
    staged = {key: p.alloc(4 * caller[name].numel()) for key, name in IS.STAGED if caller.get(name) is not None}
    # parameters
    for d in p.ops:
        if d["kind"] == "linear":
            d["w_off"], d["w_numel"] = p.param(d["N"] * d["K"])
            if d is not o_qkv and d is not o_q and d is not o_kv:
                d["b_off"], d["b_numel"] = p.param(d["N"])
        elif d["kind"] == "conv":
            d["w_off"], d["w_numel"] = p.param(d["Cout"] * 9 * d["Cin"])
            d["b_off"], d["b_numel"] = p.param(d["Cout"])
        elif d["kind"] in ("groupnorm", "layernorm"):
            d["w_off"], d["w_numel"] = p.param(CH)
            d["b_off"], d["b_numel"] = p.param(CH)
    # ---- reverse plan: the loss writes d(pred)
    p.grad_dst(pred)
    p.plan_bwd()
    mem = Mem(p.cursor + 256, p.pcursor)
    ranges = {}
    for d in p.ops:      # weights; the small vectors of the arena start at zero (sdxl_zero_grads)
        if d["w_off"] is not None:
            n, norm = d["w_numel"], d["kind"] in ("groupnorm", "layernorm")
            fan = d["K"] if d["kind"] == "linear" else 9 * d["Cin"]
            mem.w[d["w_off"]: d["w_off"] + n] = (1 + 0.1 * rnd(n, seed=100 + d["index"]).float()).to(BF) if norm else rnd(n, seed=100 + d["index"], scale=fan ** -0.5)
            if d["dy_off"] is not None:      # (conv_in's output has no reader here: no backward, no gradient to account for)
                ranges[f"op{d['index']}.weight"] = (d["w_off"], n)
            if norm:
                mem.g0[d["w_off"]: d["w_off"] + n] = 0
        if d["b_off"] is not None:
            mem.w[d["b_off"]: d["b_off"] + d["b_numel"]] = rnd(d["b_numel"], seed=200 + d["index"], scale=0.5)
            mem.g0[d["b_off"]: d["b_off"] + d["b_numel"]] = 0
            if d["dy_off"] is not None:
                ranges[f"op{d['index']}.bias"] = (d["b_off"], d["b_numel"])
    mem.w[o_cout["w_off"]: o_cout["w_off"] + o_cout["w_numel"]].view(8, 9 * CH)[4:] = 0      # the pad channels of conv_out
    mem.w[o_cout["b_off"] + 4: o_cout["b_off"] + 8] = 0
    mem.g = mem.g0.clone()
    W = lambda d: mem.w[d["w_off"]: d["w_off"] + d["w_numel"]].float()
    Bs = lambda d: mem.w[d["b_off"]: d["b_off"] + d["b_numel"]].float()
    # ---- inputs
    put(mem, emb["off"], emb, rnd(B, TEMB, seed=1))
    x0v = rnd(M, CH, seed=2).float()
    x0v = x0v.view(B, HW, G, CH // G)
    x0v[:, :, 0, :] = 1.0 + 2.0 ** -7 * torch.randint(0, 2, (B, HW, CH // G), generator=torch.Generator().manual_seed(3)).float()      # a low-variance group: two neighbouring bf16 values, var ~ 1.5e-5
    put(mem, x0["off"], x0, x0v.reshape(M, CH))
    put(mem, ehs["off"], ehs, rnd(B * CTX, CROSS, seed=4))
    # the loss preparation, from the staged copies (graph mode): each copy holds the caller's array
    copies = dict(caller)
    for key, name in IS.STAGED:
        if key in staged:
            v = caller[name].float().clone()
            if D("stale staged copy") and name == "noise_in":
                v = v.roll(1, 0)                                   # the copy of the step before: the engine goes on from it, consistently
            mem.f32(staged[key], v.numel()).copy_(v.flatten())
            copies[name] = v
    prep = dict(copies, noise_in=None) if D("x_in from noise") else copies
    mem.bf(x_in["off"], M, 8, 8).copy_(LE.prepare_rows(seam_case(prep, torch.zeros(B, 4, HH, WW))))

    # ---- forward
    def f_lin(d):
        x, y, resid, ga, _ = d["t"]
        acc = get(mem, x["off"], x).float() @ W(d).view(d["N"], d["K"]).T
        if d["b_off"] is not None and not (D("missing bias") and d is o_out1):
            acc = acc + Bs(d)
        if resid is not None:
            acc = acc + get(mem, resid["off"], resid).float()
        put(mem, y["off"], y, acc)
        if ga is not None:
            uu = NL.geglu_unpack_cols(get(mem, y["off"], y).float().contiguous(), d["N"] // 2, 64).double()
            v, t = uu[:, : d["N"] // 2], uu[:, d["N"] // 2:]
            put(mem, ga["off"], ga, (v * F.gelu(t)).float())

    def f_gn(d):
        x, y = d["t"][0], d["t"][1]
        xs = get(mem, x["off"], x).double().view(B, HW, CH).permute(0, 2, 1)
        eps = 1e-6 if D("gn eps") and d is o_gn1 else d["eps"]
        xg = xs.reshape(B, G, -1)
        mean, var = xg.mean(2), xg.var(2, unbiased=False)
        mem.f32(d["stats_off"], B * G * 2).copy_(torch.stack([mean, (var + eps).rsqrt()], -1).float().flatten())
        n = F.group_norm(xs, G, W(d).double(), Bs(d).double(), eps)
        put(mem, y["off"], y, (F.silu(n) if d["silu"] else n).permute(0, 2, 1).reshape(M, CH).float())

    def f_ln(d):
        x, y = d["t"][0], d["t"][1]
        xs = get(mem, x["off"], x).double()
        mem.f32(d["stats_off"], M * 2).copy_(torch.stack([xs.mean(1), (xs.var(1, unbiased=False) + d["eps"]).rsqrt()], -1).float().flatten())
        put(mem, y["off"], y, F.layer_norm(xs, (CH,), W(d).double(), Bs(d).double(), d["eps"]).float())

    def nchw(v):
        return v.view(B, HH, WW, -1).permute(0, 3, 1, 2)

    def f_conv(d):
        x, y, resid, rv, _ = d["t"]
        wn = W(d).view(d["Cout"], 3, 3, d["Cin"]).permute(0, 3, 1, 2)
        acc = F.conv2d(nchw(get(mem, x["off"], x).float()), wn, Bs(d), padding=1)
        if rv is not None:
            acc = acc + get(mem, rv["off"], rv).float()[:, :, None, None]
        if resid is not None:
            acc = acc + nchw(get(mem, resid["off"], resid).float())
        put(mem, y["off"], y, acc.permute(0, 2, 3, 1).reshape(M, d["Cout"]))

    def qkv_of(d, shift=0):
        qt, _, _, kt, _ = d["t"]
        C_ = d["Cin"]
        if d["self_attn"]:
            qo, ko, vo, ldk = qt["off"], qt["off"] + 2 * C_, qt["off"] + 4 * C_, qt["ld"]
        else:
            qo, ko, vo, ldk = qt["off"], kt["off"] + 2 * shift, kt["off"] + 2 * C_ + 2 * shift, kt["ld"]
        hd = lambda off, n, ld: mem.bf(off, B * n, C_, ld).double().view(B, n, HEADS, 64).permute(0, 2, 1, 3).reshape(B * HEADS, n, 64)
        return hd(qo, d["Nq"], qt["ld"]), hd(ko, d["Nk"], ldk), hd(vo, d["Nk"], ldk)

    def unheads(t):
        return t.view(B, HEADS, -1, 64).permute(0, 2, 1, 3).reshape(-1, HEADS * 64)

    def f_attn(d):
        qh, kh, vh = qkv_of(d, 8 if D("col0 shifted") and d is o_ca else 0)
        s2 = NL.scale8_ref(qh) @ kh.transpose(1, 2)                       # (scale8: the one rounding the kernels make by design)
        m = s2.max(2, keepdim=True).values
        pp = torch.exp2(s2 - m)
        l = pp.sum(2, keepdim=True)
        mem.f32(d["lse_off"], B * HEADS * d["Nq"]).copy_((((m + torch.log2(l)) * math.log(2.0))[..., 0]).float().flatten())
        put(mem, d["t"][1]["off"], d["t"][1], unheads(pp @ vh / l).float())

    fwd = {"linear": f_lin, "groupnorm": f_gn, "layernorm": f_ln, "conv": f_conv, "attn": f_attn}
    order = [o_tp, o_kv] + [d for d in p.ops if d is not o_tp and d is not o_kv]
    for d in order:
        fwd[d["kind"]](d)
        if d is o_kv:      # the rows behind the prompt's hold whatever was there before (finite: a shifted slice reads into them)
            mem.bf(kv_all["off"] + B * CTX * kv_all["ld"] * 2, KV_PAD, 4 * CH, kv_all["ld"]).copy_(rnd(KV_PAD, 4 * CH, seed=7))

    # ---- the loss on pred as it sits in the workspace, then the backward from its d pred
    pn = lambda rows: rows[:, :4].float().view(B, HW, 4).permute(0, 2, 1).reshape(B, 4, HH, WW)
    em = LE.emulate(seam_case(copies, pn(get(mem, pred["off"], pred))))
    if D("stale d pred"):      # the gradient of the micro-step before: another prediction
        em["dpred"] = LE.emulate(seam_case(copies, pn(get(mem, pred["off"], pred).roll(1, 0))))["dpred"]
    if D("wrong gate word"):
        em["out"][7] = 1.0
    mem.f32(loss_off, 8).copy_(em["out"])
    mem.f32(ps_loss_off, B).copy_(em["ps"])
    mem.f32(mask_norm_off, B).copy_(em["mnorm"])
    mem.bf(pred["goff"], M, 8, 8).copy_(em["dpred"])
    mem.f32(tp32_off, B * (CH + 64)).zero_()                              # (zeroed at the start of a backward)
    first = lambda d: mem.g0[d["w_off"]: d["w_off"] + d["w_numel"]].view(d["N"], d["K"]) if D("accumulate") and d is o_q else 0.0

    def dres(d, dy):
        resid = d["t"][2]
        if resid is not None and not d["resid_alias"]:
            put(mem, d["dres_out"], resid, IS.add_bf16(get(mem, d["dres_addend"], resid), dy))

    def b_lin(d):
        x, y, resid, ga, gu = d["t"]
        Mr, N, K = x["rows"], d["N"], d["K"]
        if d["dy32_off"] is not None:
            put(mem, d["dy_off"], y, mem.f32(d["dy32_off"], Mr * N).view(Mr, N))
        if d is o_kv:      # the other block's slice of the grouped projection's gradient: somebody else's dK | dV
            mem.bf(d["dy_off"], Mr, 2 * CH, y["ld"]).copy_(rnd(Mr, 2 * CH, seed=6))
        dy = get(mem, d["dy_off"], y)
        dres(d, dy)
        pad = IS._pad_of(d)
        if pad:      # the two memsets in front of the weight gradient
            mem.bf(d["dy_off"] + Mr * y["ld"] * 2, pad, N, y["ld"]).zero_()
            mem.bf(x["off"] + Mr * x["ld"] * 2, pad, K, x["ld"]).zero_()
            if D("pad row"):
                mem.bf(x["off"] + Mr * x["ld"] * 2, pad, K, x["ld"])[3, 5] = 1.0
        xs, dyf = get(mem, x["off"], x).float(), dy.float()
        rows = slice(0, Mr - 1) if D("wgrad row") and d is o_out2 else slice(0, Mr)
        mem.g[d["w_off"]: d["w_off"] + N * K] = (dyf[rows].T @ xs[rows] + first(d)).flatten()
        if d["b_off"] is not None:
            mem.g[d["b_off"]: d["b_off"] + N] += dyf.sum(0)
        if d["dx_out"] is None:
            return
        acc = dyf @ W(d).view(N, K)
        if gu is not None:
            dG = acc.to(BF).double()                                      # (the epilogue's bf16 dG)
            uu = NL.geglu_unpack_cols(get(mem, gu["off"], gu).float().contiguous(), K, 64).double()
            v, t = uu[:, :K].clone().requires_grad_(True), uu[:, K:].clone().requires_grad_(True)
            (v * F.gelu(t)).backward(dG)
            put(mem, d["dx_out"], gu, NL.geglu_pack_cols(v.grad, t.grad, 64).float())
            return
        if d["dx_addend"] is not None:
            a = get(mem, d["dx_addend"], x).float()
            acc = acc.to(BF).float() + a if D("double rounding") else acc + a
        put(mem, d["dx_out"], x, acc)

    def b_norm(d):
        x, y = d["t"][0], d["t"][1]
        xs = get(mem, x["off"], x).double().requires_grad_(True)
        gm, bt = W(d).double().requires_grad_(True), Bs(d).double().requires_grad_(True)
        if d["kind"] == "groupnorm":
            n = F.group_norm(xs.view(B, HW, CH).permute(0, 2, 1), G, gm, bt, d["eps"])
            out = (F.silu(n) if d["silu"] else n).permute(0, 2, 1).reshape(M, CH)
        else:
            out = F.layer_norm(xs, (CH,), gm, bt, d["eps"])
        out.backward(get(mem, d["dy_off"], y).double())
        dx = xs.grad
        if d["dx_addend"] is not None:
            src = d["dx_addend"] if not (D("wrong addend") and d is o_ln3) else o_ln3["dy_off"]
            dx = dx + get(mem, src, x).double()
        put(mem, d["dx_out"], x, dx.float())
        mem.g[d["w_off"]: d["w_off"] + CH] += gm.grad.float()
        mem.g[d["b_off"]: d["b_off"] + CH] += bt.grad.float()

    def b_conv(d):
        x, y, resid, rv, _ = d["t"]
        if d["dy_off"] is None:
            return
        dy = get(mem, d["dy_off"], y)
        dres(d, dy)
        xs = nchw(get(mem, x["off"], x).float()).clone().requires_grad_(True)
        wn = W(d).view(d["Cout"], 3, 3, d["Cin"]).permute(0, 3, 1, 2).clone().requires_grad_(True)
        F.conv2d(xs, wn, None, padding=1).backward(nchw(dy.float()))
        mem.g[d["w_off"]: d["w_off"] + d["w_numel"]] = wn.grad.permute(0, 2, 3, 1).reshape(-1)
        mem.g[d["b_off"]: d["b_off"] + d["Cout"]] += dy.float().sum(0)
        if rv is not None:
            mem.f32(d["rv32_off"], (B - 1) * rv["ld"] + CH).as_strided((B, CH), (rv["ld"], 1)).copy_(dy.float().view(B, HW, CH).sum(1))
        dx = xs.grad.permute(0, 2, 3, 1).reshape(M, d["Cin"])
        if d["dx_addend"] is not None:
            dx = dx + get(mem, d["dx_addend"], x).float()
        put(mem, d["dx_out"], x, dx)

    def b_attn(d):
        qt, ot, _, kt, _ = d["t"]
        qh, kh, vh = qkv_of(d)
        hd = lambda v: v.double().view(B, d["Nq"], HEADS, 64).permute(0, 2, 1, 3).reshape(B * HEADS, d["Nq"], 64)
        dO, O = hd(get(mem, d["dy_off"], ot)), hd(get(mem, ot["off"], ot))
        delta = (dO * O).sum(2)
        if D("delta head") and d is o_sa:
            delta = delta.view(B, HEADS, -1).roll(1, 1).reshape(B * HEADS, -1)
        mem.f32(d["delta_off"], B * HEADS * d["Nq"]).copy_(delta.float().flatten())
        lse2 = (mem.f32(d["lse_off"], B * HEADS * d["Nq"]).double() * NL.LOG2E_F32).view(B * HEADS, -1, 1)
        dpm = dO @ vh.transpose(1, 2) - (dO * O).sum(2)[..., None]
        P = torch.exp2(NL.scale8_ref(qh) @ kh.transpose(1, 2) - lse2)      # the dQ bodies round q, the dK / dV bodies k
        P2 = torch.exp2(qh @ NL.scale8_ref(kh).transpose(1, 2) - lse2)
        dq, dk, dv = 0.125 * (P * dpm) @ kh, 0.125 * (P2 * dpm).transpose(1, 2) @ qh, P2.transpose(1, 2) @ dO
        C_ = d["Cin"]
        if d["self_attn"]:
            offs, lds = (d["dx_out"], d["dx_out"] + 2 * C_, d["dx_out"] + 4 * C_), (qt["ld"],) * 3
        else:
            offs, lds = (d["dx_out"], d["d3_out"], d["d3_out"] + 2 * C_), (qt["ld"], kt["ld"], kt["ld"])
        for off, ld, v, n in zip(offs, lds, (dq, dk, dv), (d["Nq"], d["Nk"], d["Nk"])):
            mem.bf(off, B * n, C_, ld).copy_(unheads(v).float().to(BF))

    bwd = {"linear": b_lin, "groupnorm": b_norm, "layernorm": b_norm, "conv": b_conv, "attn": b_attn}
    for d in p.ops:
        if d["kind"] == "conv" and d["t"][3] is not None:
            d["rv32_off"] = tp32_off + 4 * d["t"][3]["col0"]
    for d in reversed(p.ops):
        bwd[d["kind"]](d)
    ops = strip(p.ops)
    if D("aliased residual"):      # the plan aliases out1's residual although its gradient already had a writer: that contribution is lost
        e = ops[o_out1["index"]]
        e["resid_alias"], e["dres_out"], e["dres_addend"] = 1, None, None
    tail = dict(B=B, H=HH, W=WW, ctx=CTX, t_off=None, tid_off=None, tp32_off=tp32_off, tp32_bytes=4 * B * (CH + 64), workspace_bytes=p.cursor)
    tdesc = lambda t: {k: t[k] for k in ("off", "goff", "rows", "cols", "ld", "pad_rows", "col0")}
    plan_loss = dict(dict.fromkeys([k for k, _ in IS.STAGED]), loss_part_off=None, ps_loss_off=ps_loss_off, mask_norm_off=mask_norm_off, part_floats=0,
                     ps_slots=LE.ps_slots(B, HW), staged=1, **staged)
    tail.update(x_in=tdesc(x_in), pred=tdesc(pred), loss_off=loss_off, loss=dict(plan=plan_loss, caller=caller, grad_scale=SEAM_GRAD_SCALE))
    names = dict(tp=o_tp, sc=o_sc, gn1=o_gn1, c1=o_c1, gn2=o_gn2, c2=o_c2, ln1=o_ln1, qkv=o_qkv, sa=o_sa, out1=o_out1, ln2=o_ln2, q=o_q, kv=o_kv, ca=o_ca,
                 out2=o_out2, ln3=o_ln3, ff1=o_ff1, ff2=o_ff2, cin=o_cin, cout=o_cout)
    return ops, tail, mem.img(), ranges, dict({k: v["index"] for k, v in names.items()}, seam=len(ops))


# defect -> (op, the roles that must catch it)
DEFECTS = {
    "wgrad row": ("out2", ["dw"]),                 # 1. one row left out of a weight-gradient sum
    "pad row": ("kv", ["x_pad"]),                  # 2. a pad row that should have been zeroed holds data
    "col0 shifted": ("ca", ["lse", "o"]),          # 3. a column slice off by one 8-column vector
    "aliased residual": ("out1", ["dres_chain"]),  # 4. a residual aliased where it should have been added
    "wrong addend": ("ln3", ["dx"]),               # 5. an addend taken from another write-once buffer of similar magnitude
    "gn eps": ("gn1", ["y", "rstd"]),              # 6. GroupNorm eps 1e-6 for 1e-5 on a low-variance group
    "missing bias": ("out1", ["y"]),               # 7. a bias that never reached the epilogue
    "double rounding": ("ln1", None),              # 8. a dgrad that rounded before it added its addend (any linear with an addend: found below)
    "delta head": ("sa", ["delta"]),               # 9. attention's Delta taken from another head
    "accumulate": ("q", ["dw"]),                   # 10. += onto a non-zero arena on the first micro-step
    "stale staged copy": ("seam", ["staged"]),     # 11. graph mode replayed on the copy of the step before
    "x_in from noise": ("seam", ["x_in"]),         # 12. the UNet input built from `noise` where `noise_in` was given
    "stale d pred": ("seam", ["dpred"]),           # 13. d pred left from the previous micro-step
    "wrong gate word": ("seam", ["gate"]),         # 14. out[7] is not the tag mean the gradients were scaled by
}


@pytest.fixture(scope="module")
def faithful():
    return build()


def test_the_faithful_image_passes_every_check(faithful):
    ops, tail, img, ranges, names = faithful
    results = IS.audit(ops, tail, img)
    for kind, (worst, n, elems) in sorted(IS.summarize(results).items()):
        print(f"[insitu] host {kind}: worst err / allowed {worst:.4g} over {n} outputs, {elems} elements")
    print(f"[insitu-reach] host: {'; '.join(IS.reach(ops))}")
    assert not IS.failures(results), "\n".join(IS.failures(results)[:20])
    problems, taken = IS.coverage(ops, results, ranges)
    assert not problems and not taken, problems
    got = IS.reach(ops)
    assert "pad rows" in got and "non-aliased residual" in got and "dy32_off" in got
    assert ops[names["ca"]]["t"][3]["col0"] == 2 * CH and ops[names["c1"]]["t"][3]["col0"] == 64      # the slice views are real slices


@pytest.mark.parametrize("defect", [k for k in DEFECTS if k != "double rounding"])
def test_each_seeded_defect_is_caught_by_its_check(defect):
    ops, tail, img, ranges, names = build(defect)
    bad = {(r.op, r.role) for r in IS.audit(ops, tail, img) if not r.ok}
    op, roles = DEFECTS[defect]
    print(f"[insitu] defect '{defect}': caught by {sorted(bad)}")
    assert {(names[op], r) for r in roles} <= bad, (defect, sorted(bad))
    # a defect of one op fails that op alone -- but for the lost contribution, which also leaves the NEXT writer of that gradient (the shortcut
    # projection's dgrad) with an addend that is no longer the previous writer's buffer
    extra = {names["sc"]} if defect == "aliased residual" else set()
    assert {names[op]} <= {o for o, _ in bad} <= {names[op]} | extra, f"{defect}: a defect of one op must fail that op alone, got {sorted(bad)}"


def test_a_dgrad_that_rounded_twice_is_caught():
    """every linear dgrad with an addend computes bf16(bf16(acc) + addend): each such op's dx must fail, and nothing else"""
    ops, tail, img, ranges, names = build("double rounding")
    want = {(d["index"], "dx") for d in ops if d["kind"] == "linear" and d["dx_addend"] is not None and d["t"][4] is None}
    bad = {(r.op, r.role) for r in IS.audit(ops, tail, img) if not r.ok}
    assert want and bad == want, (sorted(want), sorted(bad))


def test_coverage_sees_a_deleted_op(faithful):
    ops, tail, img, ranges, names = faithful
    cut = [d for d in ops if d["index"] != names["q"]]
    results = [r for r in IS.audit(ops, tail, img) if r.op != names["q"]]
    problems, _ = IS.coverage(cut, results, ranges)
    assert any(f"op{names['q']}.weight" in s for s in problems), problems
    # ... an op that is listed but was not audited, and a role left out without a lost buffer
    problems, _ = IS.coverage(ops, results, ranges)
    assert any(s.startswith(f"op {names['q']} ") for s in problems), problems
    problems, _ = IS.coverage(ops, [r for r in IS.audit(ops, tail, img) if (r.op, r.role) != (names["sa"], "dk")], ranges)
    assert problems == [f"op {names['sa']} (attn): role dk is neither audited nor a listed omission of a lost buffer"], problems
    # ... and a kind with no audited backward
    problems, _ = IS.coverage(ops, [r for r in IS.audit(ops, tail, img) if not (r.kind == "conv" and r.role != "y")], ranges)
    assert "kind conv: no audited backward output" in problems
    # ... and a step whose loss seam was not audited: a problem, not an omission
    problems, taken = IS.coverage(ops, [r for r in IS.audit(ops, tail, img) if r.kind != IS.SEAM_KIND], ranges)
    assert problems == [f"the loss seam: role {r} is not audited" for r in IS.SEAM_ROLES] and not taken, problems
    assert {"x_in", "dpred"} <= set(IS.SEAM_ROLES)
    problems, _ = IS.coverage(ops, [r for r in IS.audit(ops, tail, img) if (r.kind, r.role) != (IS.SEAM_KIND, "dpred")], ranges)
    assert problems == ["the loss seam: role dpred is not audited"], problems


def test_omissions_are_only_of_lost_buffers(faithful):
    ops, tail, img, ranges, names = faithful
    assert {(k, r) for k, r, _ in IS.OMISSIONS} == {("upsample", "y"), ("linear", "dx")}
    assert all(not lost for d in ops for _, lost in IS.expected_roles(d))


def test_hooks_are_declared_and_refuse_bad_arguments():
    for name in ("sdxl_debug_plan_num_ops", "sdxl_debug_plan_op", "sdxl_debug_plan_tail", "sdxl_debug_plan_loss"):
        assert name in lib.TEST_HOOK_SIGNATURES
    L = lib.load()
    n, d, t, pl = C.c_int(-7), lib.PlanOpDesc(), lib.PlanTail(), lib.PlanLoss()
    for rc in (L.sdxl_debug_plan_num_ops(None, C.byref(n)), L.sdxl_debug_plan_op(None, 0, C.byref(d), C.sizeof(d)),
               L.sdxl_debug_plan_tail(None, C.byref(t), C.sizeof(t)), L.sdxl_debug_plan_loss(None, C.byref(pl), C.sizeof(pl))):
        assert rc == 1 and b"null handle" in L.sdxl_last_error()      # (so the sizes of the Python mirrors ARE the library's: a wrong one is refused first)
    assert n.value == -7
    for rc in (L.sdxl_debug_plan_op(None, 0, C.byref(d), C.sizeof(d) - 4), L.sdxl_debug_plan_op(None, 0, C.byref(d), C.sizeof(d) + 8),
               L.sdxl_debug_plan_tail(None, C.byref(t), C.sizeof(t) - 8), L.sdxl_debug_plan_tail(None, C.byref(t), 0),
               L.sdxl_debug_plan_loss(None, C.byref(pl), C.sizeof(pl) - 8), L.sdxl_debug_plan_loss(None, C.byref(pl), C.sizeof(pl) + 8)):
        assert rc == 1 and b"bytes, the library's" in L.sdxl_last_error()
    assert len(lib.TEST_HOOK_SIGNATURES["sdxl_debug_plan_op"]) == 4 and len(lib.TEST_HOOK_SIGNATURES["sdxl_debug_plan_tail"]) == 3
    assert len(lib.TEST_HOOK_SIGNATURES["sdxl_debug_plan_loss"]) == 3 and len(lib.TEST_HOOK_SIGNATURES) == 29
    # the staging buffers are named after the Plan fields, the binding's struct after the header's
    hdr = (lib.HERE.parent / "include" / "sdxlstep_diag.h").read_text().split("typedef struct sdxl_plan_loss {", 1)[1].split("}", 1)[0]
    names = [f[0] for f in lib.PlanLoss._fields_]
    assert names == [w.strip(" ;") for w in hdr.replace("size_t", ",").replace("int ", ",").replace(";", ",").replace("\n", ",").split(",") if w.strip(" ;")]
    eng = (lib.HERE / "csrc" / "engine.h").read_text()
    assert all(f"{k} = NONE" in eng for k, _ in IS.STAGED) and {k for k, _ in IS.STAGED} <= set(names)
    assert len(lib.PLAN_KINDS) == 9 and lib.PLAN_ROLES == 5 and lib.PLAN_NONE == 2 ** 64 - 1
