"""LoHa adapters (SDXL_DTYPE_LOHA, training.lora_algo "loha") on a real MI355X: the kernels of csrc/loha.hip through their single-target
hooks on native buffers (merge bit-equal to the restatement of tests/_loha_ref.py on the source view, the four projections within the bound
accumulated next to the float64 reference, operand isolation), through sdxl_load_weight / sdxl_export_grad on the tiny UNet's handle with
every kind of target in one table, the oracle at the merged weights, and the trainer."""
import ctypes as C
import importlib

import pytest
import torch

import sdxl_amd  # noqa: F401
from oracle import loss_ref as R
from oracle import unet_ref as U
from sdxl_amd import lib
from sdxl_amd import unet as NU

import _loha_ref as HR
from _gradparity import GradParity
from _isolation import Spec, assert_isolated, run_isolated, same_bits
from test_gpu_lora_layouts import (ALL_KINDS_TARGETS, flat2, kind_of, make_batch, make_trainer, native_micro, step_args, target_mask,
                                   tiny_native_cfg)

pytestmark = pytest.mark.gpu
LORA = importlib.import_module("sdxl-training-improvements_amd.lora")

GRAD_BAR = (6e-2, 0.995)          # GRAD_BAR of tests/test_gpu_lora.py
DEV = "cuda"
PLAIN, CONV3, GEGLU = HR.PLAIN, HR.CONV3, HR.GEGLU
RANKS = [1, 3, 4, 16, 64]
# (label, kind, out, in, cin | G)
CASES = [("1x8", PLAIN, 1, 8, 0), ("8x8", PLAIN, 8, 8, 0), ("40x24", PLAIN, 40, 24, 0), ("130x264", PLAIN, 130, 264, 0),
         ("64x2048", PLAIN, 64, 2048, 0), ("1280x1280", PLAIN, 1280, 1280, 0),
         ("conv40x16", CONV3, 40, 9 * 16, 16), ("conv8x320", CONV3, 8, 9 * 320, 320),            # (conv_out's rows: a short, wide target)
         ("geglu128g64x24", GEGLU, 256, 24, 64), ("geglu160g80x24", GEGLU, 320, 24, 80)]
IDS = [c[0] for c in CASES]

bf = lambda t: t.to(torch.bfloat16)
ptr = lambda t: C.c_void_p(t.data_ptr())
stream = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)


def operands(kind, out, inn, rank, seed=0):
    """native W0 and dW, and the four factors (indexed like the state-dict tensor), all N(0, 1)"""
    g = torch.Generator().manual_seed(1000 * seed + 7 * out + inn + rank + 31 * kind)
    r = lambda *s: torch.randn(*s, generator=g)
    return dict(W0=bf(r(out, inn)).to(DEV), dW=r(out, inn).to(DEV), A1=bf(r(rank, inn)).to(DEV), B1=bf(r(out, rank)).to(DEV),
                A2=bf(r(rank, inn)).to(DEV), B2=bf(r(out, rank)).to(DEV))


def fac(x):
    return x["A1"], x["B1"], x["A2"], x["B2"]


def hook_merge(W0, A1, B1, A2, B2, s, kind, group):
    w = torch.full_like(W0, float("nan"))
    lib.check(lib.load().sdxl_op_loha_merge(ptr(W0), ptr(A1), ptr(B1), ptr(A2), ptr(B2), ptr(w), W0.shape[0], W0.shape[1], A1.shape[0], s, kind, group,
                                            stream()), "loha_merge")
    return w


def hook_project(dW, A1, B1, A2, B2, s, kind, group):
    out = {n: torch.full(t.shape, float("nan"), dtype=torch.float32, device=dW.device) for n, t in zip(HR.NAMES, (A1, B1, A2, B2))}
    lib.check(lib.load().sdxl_op_loha_project(ptr(dW), ptr(A1), ptr(B1), ptr(A2), ptr(B2), ptr(out["A1"]), ptr(out["B1"]), ptr(out["A2"]),
                                              ptr(out["B2"]), dW.shape[0], dW.shape[1], A1.shape[0], s, kind, group, stream()), "loha_project")
    return out


# ------------------------------------------------------------------------------------------------ the hooks
@pytest.mark.parametrize("rank", RANKS)
@pytest.mark.parametrize("label,kind,out,inn,group", CASES, ids=IDS)
def test_merge_is_bit_equal_to_the_restatement_and_restores_w0(label, kind, out, inn, group, rank):
    x = operands(kind, out, inn, rank)
    src0 = HR.to_source(x["W0"], kind, group)
    for s in (0.37, 1.0):
        got = hook_merge(x["W0"], *fac(x), s, kind, group)
        want = HR.to_native(HR.merge(src0, *fac(x), s), kind, group)
        assert same_bits(got, want), (label, rank, s)
        assert not same_bits(got, x["W0"])
    z = torch.zeros_like(x["B1"])
    assert same_bits(hook_merge(x["W0"], *fac(x), 0.0, kind, group), x["W0"])
    assert same_bits(hook_merge(x["W0"], x["A1"], z, x["A2"], x["B2"], 0.37, kind, group), x["W0"])
    assert same_bits(hook_merge(x["W0"], x["A1"], x["B1"], x["A2"], z, 0.37, kind, group), x["W0"])


@pytest.mark.parametrize("rank", RANKS)
@pytest.mark.parametrize("label,kind,out,inn,group", CASES, ids=IDS)
def test_project_is_within_the_accumulated_bound_overwrites_and_repeats(label, kind, out, inn, group, rank):
    x = operands(kind, out, inn, rank, seed=1)
    s = 0.37
    src = HR.to_source(x["dW"], kind, group)
    got = hook_project(x["dW"], *fac(x), s, kind, group)              # outputs pre-filled with NaN
    ref = HR.project64(src, *fac(x), s)
    bound = HR.project_bound(src, *fac(x), s)
    worst = {}
    for n in HR.NAMES:
        assert bool(torch.isfinite(got[n]).all()), f"d{n}: not overwritten everywhere"
        err = (got[n].double() - ref[n]).abs()
        worst[n] = (float((err / bound[n].clamp_min(1e-300)).max()), float((err - bound[n]).max()))
        print(f"[loha] project {label} r{rank} d{n}: max |err| / delta {worst[n][0]:.4f}")
    for n in HR.NAMES:
        assert worst[n][1] <= 0.0, (n, label, rank, worst[n])
    again = hook_project(x["dW"], *fac(x), s, kind, group)
    assert all(same_bits(got[n], again[n]) for n in HR.NAMES)


@pytest.mark.parametrize("label,kind,out,inn,group,rank", [("40x24", PLAIN, 40, 24, 0, 3), ("130x264", PLAIN, 130, 264, 0, 16),
                                                           ("conv40x16", CONV3, 40, 144, 16, 4), ("geglu128g64x24", GEGLU, 256, 24, 64, 64)])
def test_hooks_are_operand_isolated(label, kind, out, inn, group, rank):
    x = {k: v.cpu() for k, v in operands(kind, out, inn, rank, seed=2).items()}
    L = lib.load()
    f32 = torch.float32

    def merge(a):
        lib.check(L.sdxl_op_loha_merge(a.ptr("W0"), a.ptr("A1"), a.ptr("B1"), a.ptr("A2"), a.ptr("B2"), a.ptr("w"), out, inn, rank, 0.37, kind, group,
                                       stream()), "loha_merge")

    def project(a):
        lib.check(L.sdxl_op_loha_project(a.ptr("dW"), a.ptr("A1"), a.ptr("B1"), a.ptr("A2"), a.ptr("B2"), a.ptr("dA1"), a.ptr("dB1"), a.ptr("dA2"),
                                         a.ptr("dB2"), out, inn, rank, 0.37, kind, group, stream()), "loha_project")

    factors = [Spec("A1", rank, inn, init=x["A1"]), Spec("B1", out, rank, init=x["B1"]), Spec("A2", rank, inn, init=x["A2"]),
               Spec("B2", out, rank, init=x["B2"])]
    runs = run_isolated(merge, [Spec("W0", out, inn, init=x["W0"])] + factors + [Spec("w", out, inn, role="out")], device=DEV)
    assert_isolated(runs, what=f"loha_merge {label} r{rank}")
    want = HR.to_native(HR.merge(HR.to_source(x["W0"], kind, group), x["A1"], x["B1"], x["A2"], x["B2"], 0.37), kind, group)
    assert same_bits(runs[0]["w"].cpu(), want)
    outs = [Spec("dA1", rank, inn, dtype=f32, role="out"), Spec("dB1", out, rank, dtype=f32, role="out"),
            Spec("dA2", rank, inn, dtype=f32, role="out"), Spec("dB2", out, rank, dtype=f32, role="out")]
    runs = run_isolated(project, [Spec("dW", out, inn, dtype=f32, init=x["dW"])] + factors + outs, device=DEV)
    assert_isolated(runs, what=f"loha_project {label} r{rank}")


# ------------------------------------------------------------------------------------------------ the handle (tiny UNet)
@pytest.fixture(scope="module")
def tiny():
    cfg = U.tiny_config()
    w = U.synth_weights(cfg, seed=0)
    net = NU.NativeUNet(tiny_native_cfg(cfg))
    net.load_state_dict(w)
    torch.cuda.synchronize()
    w0 = net.weights.clone()
    yield cfg, w, net, w0
    net.close()


def randomize_B2(ad, std=0.02, seed=5):
    g = torch.Generator().manual_seed(seed)
    for k in ad.targets:
        ad.B2(k).copy_(bf(torch.randn(ad.B2(k).shape, generator=g) * std))


def factors_of(ad, k, grad=False):
    return ad.A1(k, grad), ad.B1(k, grad), ad.A2(k, grad), ad.B2(k, grad)


def test_batched_calls_equal_the_hook_per_target_and_touch_nothing_else(tiny):
    cfg, w, net, w0 = tiny
    shapes = net.param_shapes()
    ad = LORA.LoRAAdapters(net, rank=4, alpha=2.0, targets=ALL_KINDS_TARGETS, kinds="all", algo="loha")
    assert {kind_of(k, shapes[k])[0] for k in ad.targets} == {PLAIN, CONV3, GEGLU} and "conv_out.weight" in ad.targets
    ranges, mask = net.param_ranges(), target_mask(net, ad)
    sd0 = {k: v.clone() for k, v in net.state_dict().items() if k in ad.targets}
    try:
        ad.merge()                                                     # B2 = 0
        torch.cuda.synchronize()
        assert same_bits(net.weights, w0)
        randomize_B2(ad, std=0.5)
        ad.merge()
        torch.cuda.synchronize()
        assert same_bits(net.weights[~mask], w0[~mask])                # nothing outside the targets' native ranges
        sd = net.state_dict()
        for k in ad.targets:
            o, i = flat2(shapes[k])
            off, n = ranges[k]
            kind, group = kind_of(k, shapes[k])
            assert n == o * i, k
            want = HR.merge(sd0[k].reshape(o, i).contiguous(), *factors_of(ad, k), ad.scale)
            assert same_bits(sd[k].reshape(o, i).contiguous(), want), k
            assert not same_bits(want, sd0[k].reshape(o, i).contiguous()), k          # took effect
            hook = hook_merge(w0[off: off + n].view(o, i), *factors_of(ad, k), ad.scale, kind, group)
            assert same_bits(net.weights[off: off + n].view(o, i), hook), k
        ad.restore()
        torch.cuda.synchronize()
        assert same_bits(net.weights, w0)
        # project: the arenas are read only; every target's four gradients have the single-target hook's bits; the padding is not written
        net.grads.copy_(torch.randn(net.param_elems, generator=torch.Generator().manual_seed(3)))
        g0 = net.grads.clone()
        ad.grads.fill_(float("nan"))
        ad.project()
        torch.cuda.synchronize()
        assert same_bits(net.grads, g0) and same_bits(net.weights, w0)
        written = torch.zeros(ad.param_elems, dtype=torch.bool, device=ad.grads.device)
        for k in ad.targets:
            off, n = ranges[k]
            o, i = flat2(shapes[k])
            kind, group = kind_of(k, shapes[k])
            hook = hook_project(g0[off: off + n].view(o, i), *factors_of(ad, k), ad.scale, kind, group)
            for name, got in zip(HR.NAMES, factors_of(ad, k, grad=True)):
                assert same_bits(got, hook[name]), (k, name)
            for slot, cnt in zip(ad.layout[k][:4], (ad.rank * i, o * ad.rank, ad.rank * i, o * ad.rank)):
                written[slot: slot + cnt] = True
        assert bool(torch.isnan(ad.grads[~written]).all()) and bool(torch.isfinite(ad.grads[written]).all())
    finally:
        net.weights.copy_(w0)
        net.grads.zero_()
        torch.cuda.synchronize()


def test_argument_errors_and_the_table_keyed_by_the_dtype(tiny):
    cfg, w, net, w0 = tiny
    L = lib.load()
    names = list(net.param_shapes())
    idx = lambda k: names.index(k)
    big = torch.zeros(1 << 22, dtype=torch.bfloat16, device=DEV)
    gbig = torch.zeros(1 << 22, dtype=torch.float32, device=DEV)

    def op(params, rank=4):
        arr = (C.c_int * len(params))(*params)
        return lib.LoraOp(len(params), arr, rank, 1.0, big.data_ptr(), big.data_ptr(), gbig.data_ptr()), arr

    c1 = "down_blocks.0.resnets.0.conv1.weight"
    cases = [([idx(c1)], 0, b"rank"), ([idx(c1)], 65, b"rank"), ([idx(c1)], 128, b"rank"), ([idx("conv_in.weight")], 4, b"conv_in.weight"),
             ([idx(c1), idx("conv_in.weight")], 4, b"conv_in.weight"), ([idx("conv_out.bias")], 4, b"conv_out.bias"),
             ([idx("down_blocks.0.resnets.0.norm1.weight")], 4, b"norm1.weight"), ([idx(c1), idx(c1)], 4, b"twice"),
             ([len(names)], 4, b"out of range"), ([-1], 4, b"out of range")]
    for params, rank, msg in cases:
        o, _keep = op(params, rank)
        for fn in (L.sdxl_load_weight, L.sdxl_export_grad):
            assert fn(net.h, None, C.byref(o), lib.DTYPE_LOHA, stream()) == 1 and msg in L.sdxl_last_error(), (params, rank, L.sdxl_last_error())
    o, _keep = op([idx(c1)])
    assert L.sdxl_load_weight(net.h, b"conv_in.weight", C.byref(o), lib.DTYPE_LOHA, stream()) == 1 and b"NULL" in L.sdxl_last_error()
    assert L.sdxl_export_grad(net.h, c1.encode(), C.byref(o), lib.DTYPE_LOHA, stream()) == 1 and b"NULL" in L.sdxl_last_error()
    with pytest.raises(lib.SdxlError, match="conv1.weight"):            # the backward's own adapter gradients keep the plain rule
        net.set_trainable([], lora=o)
    torch.cuda.synchronize()
    assert same_bits(net.weights, w0) and float(big.abs().sum()) == 0.0 and float(gbig.abs().sum()) == 0.0
    # the same (target list, rank) under SDXL_DTYPE_LORA_LAYOUTS, then SDXL_DTYPE_LOHA, and back: each call has its own dtype's bits
    lo = LORA.LoRAAdapters(net, rank=4, alpha=2.0, seed=2, kinds="all")
    ha = LORA.LoRAAdapters(net, rank=4, alpha=2.0, seed=2, kinds="all", algo="loha")
    assert lo.targets == ha.targets and lo.dtype != ha.dtype
    for k in lo.targets:
        lo.B(k).copy_(bf(torch.randn(lo.B(k).shape, generator=torch.Generator().manual_seed(1)) * 0.5))
    randomize_B2(ha, std=0.5)
    try:
        lo.merge()
        torch.cuda.synchronize()
        first = net.weights.clone()
        net.weights.copy_(w0)
        ha.merge()
        torch.cuda.synchronize()
        second = net.weights.clone()
        assert not same_bits(first, w0) and not same_bits(second, w0) and not same_bits(first, second)
        net.weights.copy_(w0)
        lo.merge()
        torch.cuda.synchronize()
        assert same_bits(net.weights, first)
        net.weights.copy_(w0)
        ha.merge()
        torch.cuda.synchronize()
        assert same_bits(net.weights, second)
    finally:
        net.weights.copy_(w0)
        torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ end to end (tiny UNet, 16 x 16, B = 2)
@pytest.mark.parametrize("method", ["ddpm", "flow_matching"])
def test_a_step_with_b2_zero_has_the_plain_trainers_bits(tiny, method):
    cfg, w, net, w0 = tiny
    batch, kw = make_batch(cfg, 21), step_args(method, 22)
    try:
        plain = make_trainer(net, method)
        loss_p, _m = plain._execute_training_step(batch, **kw)
        torch.cuda.synchronize()
        g_p = net.grads.clone()
        del plain
        tr = make_trainer(net, method, lora_rank=4, lora_algo="loha", lora_target_kinds="all", lora_targets=["ff.net.0.proj", "conv1", "to_q"])
        assert isinstance(tr, LORA.NativeLoRATrainer) and tr.lora.algo == "loha"
        torch.cuda.synchronize()
        assert same_bits(net.weights, w0)                              # B2 = 0: the merge gave back W0
        loss_h, _m = tr._execute_training_step(batch, **kw)
        torch.cuda.synchronize()
        assert float(loss_h) == float(loss_p) and same_bits(net.grads, g_p) and float(g_p.abs().max()) > 0
    finally:
        net.weights.copy_(w0)
        net.grads.zero_()
        torch.cuda.synchronize()


@pytest.mark.parametrize("method", ["ddpm", "flow_matching"])
def test_adapter_gradients_match_the_oracle_at_the_merged_weights(tiny, method):
    """native dA1 / dB1 / dA2 / dB2 of every kind of target against the float64 projection of the oracle's autograd dW reshaped [out, in], the
    oracle evaluated at the bf16-rounded MERGED weights; rank 4, B2 std 0.02, the bar of tests/test_gpu_lora.py.  Beside it (printed): the
    float64 projection of the EXPORTED native dW, which holds the weight gradient's own error and none of the projection kernels'.  Then
    the same step under project_frozen: bit-equal."""
    cfg, w, net, w0 = tiny
    rank = 4
    shapes = net.param_shapes()
    ad = LORA.LoRAAdapters(net, rank=rank, alpha=rank / 2, targets=ALL_KINDS_TARGETS, seed=1, kinds="all", algo="loha")
    randomize_B2(ad, std=0.02)
    x, kw = make_batch(cfg, 31), step_args(method, 32)
    names = dict(LORA.LOHA_FACTORS)
    try:
        ad.merge()
        native_micro(net, method, x, kw)
        ad.grads.fill_(float("nan"))
        ad.project()
        torch.cuda.synchronize()
        loss = net.read_loss()[0]
        got = ad.grads.clone()
        exported = {k: net.export(k, grad=True).double().cpu() for k in ad.targets}
        wm = {k: v.float().cpu() for k, v in net.state_dict().items()}           # bf16-rounded merged weights, as the step read them
        assert any(not torch.equal(wm[k], w[k]) for k in ad.targets)
        leaves = {k: wm[k].requires_grad_(True) for k in ad.targets}
        unet_fn = lambda s, t, e, p, ti: U.unet_forward(wm, s, t, e, p, ti, cfg)
        ob = {k: x[k] for k in ("vae_latents", "prompt_embeds", "pooled_prompt_embeds", "time_ids")}
        ref = R.compute_loss_ddpm(unet_fn, ob, kw["noise"], kw["timesteps"]) if method == "ddpm" else R.compute_loss_flow(unet_fn, ob, kw["noise"], kw["timesteps"])
        ref["loss"].backward()
        par, inherited = GradParity(f"loha {method} r{rank}"), GradParity(f"loha {method} r{rank}: float64 projection of the exported dW")
        for k in ad.targets:
            o, i = flat2(shapes[k])
            f = [t.cpu() for t in factors_of(ad, k)]
            want = HR.project64(leaves[k].grad.reshape(o, i), *f, ad.scale)
            inh = HR.project64(exported[k].reshape(o, i), *f, ad.scale)
            mod = k[: -len(".weight")]
            for name, g in zip(HR.NAMES, factors_of(ad, k, grad=True)):
                par.add(f"{mod}.{names[name]}", g.cpu(), want[name])
                inherited.add(f"{mod}.{names[name]}", inh[name], want[name])
        inherited.report(lambda _k: GRAD_BAR, printer=lambda s: print("[parity] " + s))
        par.check(GRAD_BAR, expect=ad.param_ranges(), printer=lambda s: print("[parity] " + s))
        ad.select("project_frozen")
        native_micro(net, method, x, kw)
        ad.grads.fill_(float("nan"))
        ad.project()
        torch.cuda.synchronize()
        assert net.read_loss()[0] == loss and same_bits(ad.grads, got)
    finally:
        net.set_trainable(None)
        net.weights.copy_(w0)
        net.grads.zero_()
        torch.cuda.synchronize()


TRAINER_TARGETS = ["ff.net.0.proj", "conv1", "conv_shortcut", "to_q"]


def twenty_steps(net):
    cfg = U.tiny_config()
    tr = make_trainer(net, "ddpm", lora_rank=4, lora_algo="loha", lora_target_kinds="all", lora_targets=TRAINER_TARGETS)
    batch = make_batch(cfg, 41)
    noise = torch.randn(batch["vae_latents"].shape, generator=torch.Generator().manual_seed(42))       # evaluate() draws the same
    ts = torch.full((2,), 500, dtype=torch.long)
    evaluate = lambda: tr.evaluate([batch], [500], generator=torch.Generator().manual_seed(42))[1]
    before = evaluate()
    losses = []
    for _ in range(20):
        loss, _m = tr._execute_training_step(batch, timesteps=ts, noise=noise)
        losses.append(float(loss))
        tr.optimizer_step()
    after = evaluate()
    torch.cuda.synchronize()
    return tr, before, after, losses


def test_twenty_steps_on_one_batch_lower_its_loss_and_repeat_bit_for_bit(tiny):
    cfg, w, net, w0 = tiny
    shapes = net.param_shapes()
    try:
        tr, before, after, losses = twenty_steps(net)
        print(f"[loha] ddpm: evaluation loss {before:.6f} -> {after:.6f} after 20 steps")
        assert after < before
        ad = tr.lora
        mask, ranges = target_mask(net, ad), net.param_ranges()
        assert same_bits(net.weights[~mask], w0[~mask])                # only the targets moved ...
        assert all(not same_bits(net.weights[ranges[k][0]: ranges[k][0] + ranges[k][1]], w0[ranges[k][0]: ranges[k][0] + ranges[k][1]])
                   for k in ad.targets)                                # ... and every one of them did
        assert all(float(ad.B2(k).float().abs().max()) > 0 for k in ad.targets)
        assert {kind_of(k, shapes[k])[0] for k in ad.targets} == {PLAIN, CONV3, GEGLU}
        first = (net.weights.clone(), ad.weights.clone(), ad.grads.clone(), before, after, losses)
        net.weights.copy_(w0)
        tr2, before2, after2, losses2 = twenty_steps(net)
        assert same_bits(net.weights, first[0]) and same_bits(tr2.lora.weights, first[1]) and same_bits(tr2.lora.grads, first[2])
        assert (before2, after2, losses2) == first[3:]
    finally:
        net.set_trainable(None)
        net.weights.copy_(w0)
        net.grads.zero_()
        torch.cuda.synchronize()


def run_training(net, steps, accum=2, save_at=None, save_dir=None, resume_from=None, first_step=0):
    cfg = U.tiny_config()
    tr = make_trainer(net, "ddpm", lora_rank=4, lora_alpha=8.0, lora_algo="loha", lora_target_kinds="all", lora_targets=TRAINER_TARGETS,
                      gradient_accumulation_steps=accum)
    if resume_from is not None:
        tr.load_lora_state(resume_from)
    for s in range(first_step, first_step + steps):
        for m in range(accum):
            tr._execute_training_step(make_batch(cfg, 100 + 10 * s + m), accumulate=True, is_last_accumulation_step=m == accum - 1,
                                      **step_args("ddpm", 200 + 10 * s + m))
        tr.optimizer_step()
        if save_at is not None and s == save_at:
            tr.save_checkpoint(save_dir)
    torch.cuda.synchronize()
    return tr


def test_checkpoint_round_trip_and_exported_delta(tiny, tmp_path):
    from safetensors.torch import load_file
    cfg, w, net, w0 = tiny
    try:
        tr = run_training(net, 3, save_at=1, save_dir=tmp_path / "ck")
        want = (net.weights.clone(), tr.lora.weights.clone(), tr.optimizer.exp_avg.clone(), tr.optimizer.exp_avg_sq.clone())
        net.weights.copy_(w0)                                      # a fresh process would load the checkpoint's UNet
        tr2 = run_training(net, 1, resume_from=tmp_path / "ck", first_step=2)
        for a, b in zip(want, (net.weights, tr2.lora.weights, tr2.optimizer.exp_avg, tr2.optimizer.exp_avg_sq)):
            assert same_bits(a, b)
        ex = load_file(str(tmp_path / "ck" / "lycoris_loha.safetensors"))
        st = torch.load(str(tmp_path / "ck" / "lora_state.pt"), weights_only=True)
        assert len(ex) == 5 * len(tr.lora.targets) and st["rank"] == 4 and st["targets"] == tr.lora.targets and st["algo"] == "loha"
        saved = LORA.LoRAAdapters(net, rank=4, alpha=8.0, targets=TRAINER_TARGETS, kinds="all", algo="loha")
        saved.load_state_dict(st)
        for k in saved.targets:
            pre = "lora_unet_" + k[: -len(".weight")].replace(".", "_")
            rebuilt = (float(ex[f"{pre}.alpha"]) / 4) * (ex[f"{pre}.hada_w1_a"].double() @ ex[f"{pre}.hada_w1_b"].double()) \
                * (ex[f"{pre}.hada_w2_a"].double() @ ex[f"{pre}.hada_w2_b"].double())
            want_delta = HR.delta64(*[t.cpu() for t in factors_of(saved, k)], saved.scale)
            assert torch.equal(rebuilt, want_delta) and float(want_delta.abs().max()) > 0, k
        other = make_trainer(net, "ddpm", lora_rank=4, lora_target_kinds="all", lora_targets=TRAINER_TARGETS)      # a LoRA trainer refuses the state
        before = other.lora.weights.clone()
        with pytest.raises(ValueError, match="lora_algo"):
            other.load_lora_state(tmp_path / "ck")
        assert same_bits(other.lora.weights, before)
    finally:
        net.weights.copy_(w0)
        net.grads.zero_()
        torch.cuda.synchronize()
