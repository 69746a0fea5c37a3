"""Conditioning gradients on a real MI355X: d loss / d prompt_embeds and d loss / d pooled_prompt_embeds out of the HIP backward.

  1. the kernel (csrc/cond_dgrad.hip) through its hook: small-integer operands against an exact integer reference, bit for bit;
  2. the kernel on seeded normal bf16 operands against an fp64 matmul of the same values, within the fp32 summation bound;
  3. the tiny UNet's two gradients against autograd of the fp32 CPU oracle (oracle.unet_ref.unet_forward is differentiable in
     encoder_hidden_states and text_embeds), at the bar test_gpu_model.py holds every parameter gradient to;
  4. one case through the real-width shallow UNet of test_gpu_buckets.py (cross dim 2048, pooled 1280, both K | V width groups);
  5. the semantics the header states (no bit of the step changes, either pointer alone, grad_scale, the gate, overwrite, graph mode,
     per-segment backward, the hook's bits);
  6. the trainer: a torch "text encoder" in front of compute_loss gets its gradients through loss.backward().
"""
import ctypes as C
import importlib
import os
import time

import pytest
import torch

import sdxl_amd  # noqa: F401
from oracle import loss_ref as R
from oracle import unet_ref as U
from sdxl_amd import lib
from sdxl_amd import unet as NU

import _bucket_cases as BK
import _buckets as T
from test_gpu_model import TINY_GRAD_BAR, make_inputs, tiny_native_cfg

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _st():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def cond_dgrad(As, Ws, M, N, C_out=None):
    """the hook: As[g] bf16 [>= M][K_g] (row stride = its own), Ws[g] bf16 [K_g][ldb_g] of which the first N columns are used"""
    n = len(As)
    out = torch.full((M, N), float("nan"), dtype=torch.float32, device=DEV) if C_out is None else C_out
    pa = (C.c_void_p * n)(*[a.data_ptr() for a in As])
    pw = (C.c_void_p * n)(*[w.data_ptr() for w in Ws])
    lda = (C.c_long * n)(*[a.stride(0) for a in As])
    ldb = (C.c_long * n)(*[w.stride(0) for w in Ws])
    K = (C.c_int * n)(*[a.shape[1] for a in As])
    lib.check(lib.load().sdxl_op_cond_dgrad(n, pa, lda, pw, ldb, K, C.c_void_p(out.data_ptr()), out.stride(0), M, N, _st()), "sdxl_op_cond_dgrad")
    return out


def _ref64(As, Ws, M, N, absolute=False):
    """sum_g A_g[:M] . W_g[:, :N] in float64 on the device, the reduction in slices (the 85 MB operand stays 85 MB)"""
    ref = torch.zeros(M, N, dtype=torch.float64, device=DEV)
    for a, w in zip(As, Ws):
        for k0 in range(0, a.shape[1], 16384):
            x, y = a[:M, k0:k0 + 16384].double(), w[k0:k0 + 16384, :N].double()
            ref += (x.abs() @ y.abs()) if absolute else (x @ y)
    return ref


EXACT = [(77, 128, [1280, 6144], 128), (1, 96, [256], 288), (3, 96, [256], 288), (154, 2048, [2560], 2048),
         (308, 256, [12800, 153600], 256), (616, 256, [12800, 1280], 256)]


@pytest.mark.parametrize("M,N,Ks,ldb", EXACT, ids=[f"{m}-{n}-{'+'.join(map(str, k))}-{l}" for m, n, k, l in EXACT])
def test_kernel_is_exact_on_small_integers(M, N, Ks, ldb):
    """Operands are integers in {-2 .. 2} (exact in bf16); every partial sum stays below 2^24 in any order (4 * 166 400 at most), so
    fp32 accumulation is exact and the result must equal the integer reference bit for bit (the reference is a float64 matmul of
    integers below 2^53: exact, compared as int64).  Columns of W beyond N hold NaN (ldb > N); for the first shape A has 51 more rows
    of NaN bit patterns, which the kernel must never read."""
    g = torch.Generator(device=DEV).manual_seed(1000 + M)
    ints = lambda *s: torch.randint(-2, 3, s, generator=g, device=DEV).to(torch.bfloat16)
    extra = 51 if (M, N) == (77, 128) else 0
    As, Ws = [], []
    for K in Ks:
        a = torch.full((M + extra, K), float("nan"), dtype=torch.bfloat16, device=DEV)
        a[:M] = ints(M, K)
        w = torch.full((K, ldb), float("nan"), dtype=torch.bfloat16, device=DEV)
        w[:, :N] = ints(K, N)
        As.append(a)
        Ws.append(w)
    got = cond_dgrad(As, Ws, M, N)
    ref = _ref64(As, Ws, M, N)
    assert float(ref.abs().max()) < 2 ** 24
    assert bool(torch.isfinite(got).all())
    bad = int((got.to(torch.int64) != ref.to(torch.int64)).sum()) + int((got != got.round()).sum())
    print(f"[cond_dgrad] exact {M}x{N} K={Ks} ldb={ldb}: {bad} of {M * N} elements differ from the integer reference, max |ref| {float(ref.abs().max()):.0f}")
    assert bad == 0
    if extra:      # without the extra rows: the same bits
        again = cond_dgrad([a[:M].clone() for a in As], Ws, M, N)
        assert torch.equal(again.view(torch.int32), got.view(torch.int32))


FLOATS = [(77, 128, [1280, 6144], 128), (4, 1280, [1280], 2816)]


@pytest.mark.parametrize("M,N,Ks,ldb", FLOATS, ids=["tiny-prompt", "base-pooled"])
def test_kernel_on_normal_operands_within_the_fp32_summation_bound(M, N, Ks, ldb):
    """|got - ref| <= 2 K_tot 2^-24 (|A| . |W|) elementwise: the fp32 summation bound for any order, with a factor 2 for the MFMA's
    internal adder (bf16 x bf16 products are exact in fp32).  ref is an fp64 matmul of the same bf16 values.  Two runs: the same bits."""
    g = torch.Generator(device=DEV).manual_seed(7 + M)
    As = [torch.randn(M, K, generator=g, device=DEV).to(torch.bfloat16) for K in Ks]
    Ws = [torch.randn(K, ldb, generator=g, device=DEV).to(torch.bfloat16) for K in Ks]
    got = cond_dgrad(As, Ws, M, N)
    again = cond_dgrad(As, Ws, M, N)
    ref = _ref64(As, Ws, M, N)
    bound = 2.0 * sum(Ks) * 2.0 ** -24 * _ref64(As, Ws, M, N, absolute=True)
    err = (got.double() - ref).abs()
    worst = float((err / bound).max())
    print(f"[cond_dgrad] floats {M}x{N} K={Ks}: max |err| {float(err.max()):.3e}, worst err / bound {worst:.3e}")
    assert worst <= 1.0
    assert torch.equal(again.view(torch.int32), got.view(torch.int32))


# ---------------------------------------------------------------------------------------------------------------- tiny UNet
@pytest.fixture(scope="module")
def tiny():
    cfg = U.tiny_config()
    w = U.synth_weights(cfg, seed=0)
    net = NU.NativeUNet(tiny_native_cfg(cfg))
    net.load_state_dict(w)
    yield cfg, w, net
    net.close()


def _parity(label, got, ref):
    a, b = got.detach().cpu().double().flatten(), ref.detach().double().flatten()
    rel = float((a - b).norm() / b.norm())
    cos = float(torch.dot(a, b) / (a.norm() * b.norm()))
    print(f"[parity] {label}: rel-L2 {rel:.3e} cos {cos:.6f} |ref| {float(b.norm()):.3e} (bar rel-L2 <= {TINY_GRAD_BAR[0]:.0e}, cos >= {TINY_GRAD_BAR[1]})")
    return rel, cos


def _oracle_and_step(net, w, ucfg, method, x, B, sample_weights=None, loss_mask=None):
    """(oracle d ehs, oracle d pooled, device d ehs, device d pooled) of one step with both gradients requested"""
    ehs, pooled = x["ehs"].clone().requires_grad_(True), x["pooled"].clone().requires_grad_(True)
    unet_fn = lambda s, t, e, p, ti: U.unet_forward(w, s, t, e, p, ti, ucfg)
    batch = {"vae_latents": x["lat"], "prompt_embeds": ehs, "pooled_prompt_embeds": pooled, "time_ids": x["tid"]}
    ext = {}
    if sample_weights is not None:
        ext["sample_weights"] = sample_weights
    if loss_mask is not None:
        ext["loss_mask"] = loss_mask
    if method == "ddpm":
        ts = torch.tensor([610, 230][:B])
        ref = R.compute_loss_ddpm(unet_fn, batch, x["noise"], ts)
        net.forward_loss("ddpm", x["lat"], x["noise"], R.karras_sigmas()[ts], ts.float(), x["ehs"], x["pooled"], x["tid"], cond_grads=True, **ext)
        loss = ref["loss"]
    else:
        tf = R.sample_logit_normal_from_z(x["z"])
        ref = R.compute_loss_flow(unet_fn, batch, x["noise"], tf)
        net.forward_loss("flow_matching", x["lat"], x["noise"], tf, tf, x["ehs"], x["pooled"], x["tid"], cond_grads=True, **ext)
        loss = ref["loss"]
        if sample_weights is not None or loss_mask is not None:      # the device loss's definition: s_b m_bhw (v - v*)^2, mean over all elements
            e = (ref["pred"] - (x["lat"] - x["noise"])) ** 2
            if sample_weights is not None:
                e = e * sample_weights.view(-1, 1, 1, 1)
            if loss_mask is not None:
                e = e * loss_mask.view(B, 1, *loss_mask.shape[-2:])
            loss = e.mean()
    net.zero_grads()
    net.backward(1.0, True)
    got_loss = net.read_loss()[0]
    ref_loss = float(loss.detach())
    rel = abs(got_loss - ref_loss) / abs(ref_loss)
    print(f"[parity] loss: hip {got_loss:.6f} oracle {ref_loss:.6f} rel {rel:.3e}")
    assert rel <= 1e-3
    loss.backward()
    d_e, d_p = net.read_cond_grads()
    return ehs.grad, pooled.grad, d_e, d_p


RAGGED = next((h, w) for h, w in T.latent_shapes() if (h // 4) * (w // 4) % 64)      # a default bucket whose level-2 token count is ragged
ORACLE_CASES = [("ddpm", 1, 32, 32, None), ("flow_matching", 1, 32, 32, None), ("flow_matching", 2, *RAGGED, None),
                ("flow_matching", 2, 16, 16, "sample_weights"), ("flow_matching", 2, 16, 16, "loss_mask")]


@pytest.mark.parametrize("method,B,H,W,extra", ORACLE_CASES, ids=[f"{m}-{b}-{h}-{w}-{e}" for m, b, h, w, e in ORACLE_CASES])
def test_tiny_unet_conditioning_gradients_match_oracle(tiny, method, B, H, W, extra):
    cfg, w, net = tiny
    x = make_inputs(cfg, B, H, W, seed=13 if method == "ddpm" else 17)
    sw = torch.tensor([0.5, 1.75]) if extra == "sample_weights" else None
    mask = None
    if extra == "loss_mask":
        mask = torch.tensor([0.0, 0.25, 0.5, 1.0])[torch.randint(0, 4, (B, H, W), generator=torch.Generator().manual_seed(5))]
    r_e, r_p, d_e, d_p = _oracle_and_step(net, w, cfg, method, x, B, sw, mask)
    assert d_e.dtype == torch.float32 and tuple(d_e.shape) == (B, 77, cfg.cross_attention_dim) and d_e.is_cuda
    assert d_p.dtype == torch.float32 and tuple(d_p.shape) == (B, cfg.pooled_dim) and d_p.is_cuda
    res = [_parity(f"tiny {method} {B}x{H}x{W} {extra or ''} d_prompt_embeds", d_e, r_e),
           _parity(f"tiny {method} {B}x{H}x{W} {extra or ''} d_pooled", d_p, r_p)]
    for rel, cos in res:
        assert rel <= TINY_GRAD_BAR[0] and cos >= TINY_GRAD_BAR[1]


def test_real_width_conditioning_gradients_match_oracle():
    """The real-width shallow UNet of test_gpu_buckets.py (every field of SDXL-base but transformer_layers (0, 1, 1): cross dim 2048,
    pooled 1280, a 640- and a 1280-wide K | V group) at the cheaper of its two oracle cases, flow matching, B = 1."""
    from test_gpu_fullsize import _inputs
    n = len(os.sched_getaffinity(0))
    if os.environ.get("OMP_NUM_THREADS", "").isdigit():
        n = min(n, max(1, int(os.environ["OMP_NUM_THREADS"])))
    torch.set_num_threads(n)
    ucfg = U.UNetConfig(transformer_layers_per_block=(0, 1, 1))
    w = U.synth_weights(ucfg, seed=0)
    net = NU.NativeUNet(NU.make_config(transformer_layers=ucfg.transformer_layers_per_block))
    try:
        net.load_state_dict(w)
        B, H, W = min(BK.SHALLOW_ORACLE, key=lambda s: s[0] * s[1] * s[2])
        x = _inputs(B, H, W, seed=2000 + H)
        t = torch.tensor([0.3671875])
        ehs, pooled = x["ehs"].clone().requires_grad_(True), x["pooled"].clone().requires_grad_(True)
        t0 = time.perf_counter()
        net.zero_grads()
        net.forward_loss("flow_matching", x["lat"], x["noise"], t, t, x["ehs"], x["pooled"], x["tid"], cond_grads=("prompt", "pooled"))
        net.backward(1.0, True)
        got = net.read_loss()[0]
        unet_fn = lambda s, tt, e, p, ti: U.unet_forward(w, s, tt, e, p, ti, ucfg)
        ref = R.compute_loss_flow(unet_fn, {"vae_latents": x["lat"], "prompt_embeds": ehs, "pooled_prompt_embeds": pooled, "time_ids": x["tid"]},
                                  x["noise"], t)
        ref["loss"].backward()
        print(f"[parity] shallow real-width {B}x{H}x{W}: loss hip {got:.6e} oracle {float(ref['loss'].detach()):.6e}; step + oracle took {time.perf_counter() - t0:.1f} s")
        d_e, d_p = net.read_cond_grads()
        res = [_parity(f"shallow real-width {B}x{H}x{W} d_prompt_embeds", d_e, ehs.grad), _parity(f"shallow real-width {B}x{H}x{W} d_pooled", d_p, pooled.grad)]
    finally:
        net.close()
    for rel, cos in res:
        assert rel <= TINY_GRAD_BAR[0] and cos >= TINY_GRAD_BAR[1]


# ---------------------------------------------------------------------------------------------------------------- semantics
def _bits(t):
    return None if t is None else t.detach().clone().view(torch.int32)


def _step(net, x, cond_grads, scale=1.0, first=True, zero=True, on_segment=None, B=2):
    """one flow-matching step; (read_loss's eight values, the gradient arena's bits, d ehs bits, d pooled bits)"""
    tf = R.sample_logit_normal_from_z(x["z"])
    kw = {} if cond_grads is None else {"cond_grads": cond_grads}
    net.forward_loss("flow_matching", x["lat"], x["noise"], tf, tf, x["ehs"], x["pooled"], x["tid"], **kw)
    if zero:
        net.zero_grads()
    net.backward(scale, first, on_segment=on_segment)
    out = net.read_loss()
    d_e, d_p = net.read_cond_grads() if cond_grads is not None else (None, None)
    return out, _bits(net.grads), _bits(d_e), _bits(d_p)


def test_request_changes_no_bit_and_either_pointer_alone_gives_the_same_bits(tiny):
    cfg, _, net = tiny
    x = make_inputs(cfg, 2, 16, 16, seed=21)
    out0, g0, _, _ = _step(net, x, None)
    out, g, de, dp = _step(net, x, True)
    assert out == out0 and torch.equal(g, g0)
    assert int(de.ne(0).sum()) > 0 and int(dp.ne(0).sum()) > 0
    out1, g1, de1, dp1 = _step(net, x, ("prompt",))
    assert out1 == out0 and torch.equal(g1, g0) and torch.equal(de1, de) and dp1 is None
    out2, g2, de2, dp2 = _step(net, x, ("pooled",))
    assert out2 == out0 and torch.equal(g2, g0) and torch.equal(dp2, dp) and de2 is None
    # per-segment backward (the exchange's path) gives backward_all's bits
    out3, g3, de3, dp3 = _step(net, x, True, on_segment=lambda k, off, n: None)
    assert out3 == out0 and torch.equal(g3, g0) and torch.equal(de3, de) and torch.equal(dp3, dp)


def test_grad_scale_gate_and_overwrite(tiny):
    cfg, _, net = tiny
    x, y = make_inputs(cfg, 2, 16, 16, seed=22), make_inputs(cfg, 2, 16, 16, seed=23)
    _, g1, de1, dp1 = _step(net, x, True, scale=1.0)
    _, gq, deq, dpq = _step(net, x, True, scale=0.25)
    # grad_scale multiplies d(pred); 0.25 is a power of two, so every later product and sum scales exactly: the bits of 0.25 x the unscaled run
    assert torch.equal(deq, _bits(de1.view(torch.float32) * 0.25)) and torch.equal(dpq, _bits(dp1.view(torch.float32) * 0.25))
    # a closed gate (non-finite latent, so the activations and dK | dV of that sample are not finite either): exact zeros
    bad = dict(x)
    bad["lat"] = x["lat"].clone()
    bad["lat"][0, 0, 0, 0] = float("inf")
    out, _, dez, dpz = _step(net, bad, True)
    assert out[7] == 0.0
    assert int(dez.view(torch.float32).ne(0).sum()) == 0 and int(dpz.view(torch.float32).ne(0).sum()) == 0
    # the second micro-step of a cycle overwrites: the bits of the same batch run alone
    _, _, dey, dpy = _step(net, y, True)
    _step(net, x, True, first=True)
    _, _, dey2, dpy2 = _step(net, y, True, first=False, zero=False)
    assert torch.equal(dey2, dey) and torch.equal(dpy2, dpy)


def test_graph_replay_equals_eager_with_moving_outputs(tiny):
    cfg, _, net = tiny
    x = make_inputs(cfg, 2, 16, 16, seed=24)
    _, g0, de0, dp0 = _step(net, x, True)
    keep, ptrs = [], set()
    net.set_graph_mode(True)
    try:
        for i in range(4):      # eager, capture, replay, replay
            _, g, de, dp = _step(net, x, True)
            keep.append(net.read_cond_grads())      # held: the next request's buffers are new allocations
            ptrs.add(keep[-1][0].data_ptr())
            assert torch.equal(g, g0) and torch.equal(de, de0) and torch.equal(dp, dp0), i
        _, g, de, dp = _step(net, x, ("pooled",))      # another capture key
        assert torch.equal(g, g0) and de is None and torch.equal(dp, dp0)
    finally:
        net.set_graph_mode(False)
    assert len(ptrs) == 4


def test_plan_values_are_the_hooks_bits(tiny):
    """unet_forward / unet_backward with a seeded d(pred): the two results equal what sdxl_op_cond_dgrad computes from the plan's own
    operands (dK | dV of every block and d(add_embedding.linear_1's output) in the workspace, the weights in the arena), twice."""
    cfg, _, net = tiny
    B, H, W = 2, 16, 16
    x = make_inputs(cfg, B, H, W, seed=25)
    dpred = torch.randn(B, 4, H, W, generator=torch.Generator().manual_seed(26))
    L = lib.load()

    def operands(which):
        As, Ws, g, n = [], [], 0, C.c_int(1)
        while g < n.value:
            aoff, woff, lda, ldb, K = C.c_size_t(), C.c_size_t(), C.c_long(), C.c_long(), C.c_int()
            lib.check(L.sdxl_debug_cond_operands(net.h, which, g, C.byref(n), C.byref(aoff), C.byref(lda), C.byref(woff), C.byref(ldb), C.byref(K)))
            M = B * 77 if which == 0 else B
            a = net.workspace[aoff.value:aoff.value + 2 * M * lda.value].view(torch.bfloat16).view(M, lda.value)[:, :K.value]
            wt = net.weights[woff.value:woff.value + K.value * ldb.value].view(K.value, ldb.value)
            As.append(a)
            Ws.append(wt)
            g += 1
        return As, Ws

    seen = []
    for _ in range(2):
        net.unet_forward(x["lat"], torch.tensor([10.0, 500.0]), x["ehs"], x["pooled"], x["tid"], cond_grads=True)
        net.zero_grads()
        net.unet_backward(dpred, True)
        d_e, d_p = net.read_cond_grads()
        As, Ws = operands(0)
        assert len(As) == 2 and [a.shape[1] for a in As] == [1280, 6144]
        h_e = cond_dgrad(As, Ws, B * 77, cfg.cross_attention_dim)
        As, Ws = operands(1)
        h_p = cond_dgrad(As, Ws, B, cfg.pooled_dim)
        assert int(d_e.ne(0).sum()) > 0 and int(d_p.ne(0).sum()) > 0
        assert torch.equal(_bits(d_e.reshape(B * 77, -1)), _bits(h_e)) and torch.equal(_bits(d_p), _bits(h_p))
        seen.append((_bits(d_e), _bits(d_p)))
    assert torch.equal(seen[0][0], seen[1][0]) and torch.equal(seen[0][1], seen[1][1])


# ---------------------------------------------------------------------------------------------------------------- trainer
def test_trainer_hands_the_gradients_to_a_torch_text_encoder(tiny):
    cfg, _, net = tiny
    cfgm = importlib.import_module("sdxl-training-improvements_amd.config")
    TR = importlib.import_module("sdxl-training-improvements_amd.trainer")
    B = 2
    x = make_inputs(cfg, B, 16, 16, seed=31)
    g = torch.Generator().manual_seed(32)
    noise = torch.randn(B, 4, 16, 16, generator=g)
    t = torch.tensor([0.21, 0.83])

    class M:
        unet = net

    def encoder():
        torch.manual_seed(33)
        tok = torch.nn.Parameter(torch.randn(B, 77, 24))
        vec = torch.nn.Parameter(torch.randn(B, 16))
        lin_e, lin_p = torch.nn.Linear(24, cfg.cross_attention_dim), torch.nn.Linear(16, cfg.pooled_dim)
        return tok, vec, lin_e, lin_p

    def run(requires_grad=True, **keys):
        c = cfgm.Config()
        c.training.method = "flow_matching"
        c.training.mixed_precision = "no"
        for k, v in keys.items():
            setattr(c.training, k, v)
        tr = TR.NativeSDXLTrainer(M(), config=c)
        tok, vec, lin_e, lin_p = encoder()
        with torch.set_grad_enabled(requires_grad):
            pe, pp = lin_e(tok), lin_p(vec)
        batch = {"vae_latents": x["lat"], "prompt_embeds": pe, "pooled_prompt_embeds": pp, "time_ids": x["tid"], "metadata": {}}
        tr.zero_grad()
        out = tr.compute_loss(batch, timesteps=t, noise=noise, generator=torch.Generator().manual_seed(34))
        out["loss"].backward()
        torch.cuda.synchronize()
        return tr, (tok, vec, lin_e, lin_p), (pe, pp), net.grads.clone()

    tr, (tok, vec, lin_e, lin_p), (pe, pp), arena = run()
    d_e, d_p = (v.cpu() for v in net.read_cond_grads())
    # the chain rule in torch on the device's values: what autograd must have handed the encoder
    # (on a second forward of the encoder: loss.backward() has freed the first one's graph)
    want = torch.autograd.grad([lin_e(tok), lin_p(vec)], [tok, vec, lin_e.weight, lin_p.weight], [d_e.to(pe.dtype), d_p.to(pp.dtype)])
    for name, got, ref in zip(("tokens", "vector", "prompt linear", "pooled linear"), (tok.grad, vec.grad, lin_e.weight.grad, lin_p.weight.grad), want):
        err = float((got - ref).abs().max()) / float(ref.abs().max())
        print(f"[trainer] {name}: max |grad - chain rule| / max |chain rule| = {err:.3e}")
        assert got is not None and float(ref.abs().max()) > 0 and err <= 1e-5      # fp32 rounding of the same matmul (the order of sums may differ)
    # parameter gradients: the bits of a step whose conditioning does not require grad
    _, (tok0, _, _, _), _, arena0 = run(requires_grad=False)
    assert tok0.grad is None and torch.equal(arena0.view(torch.int32), arena.view(torch.int32))
    # "off": nothing comes back
    _, (tok1, vec1, lin_e1, _), _, arena1 = run(conditioning_grads="off")
    assert tok1.grad is None and vec1.grad is None and lin_e1.weight.grad is None
    assert torch.equal(arena1.view(torch.int32), arena.view(torch.int32))
    # every sample dropped: exact zeros from autograd
    _, (tok2, vec2, _, _), _, _ = run(cond_dropout_prob=1.0)
    assert tok2.grad is not None and int(tok2.grad.ne(0).sum()) == 0 and int(vec2.grad.ne(0).sum()) == 0
