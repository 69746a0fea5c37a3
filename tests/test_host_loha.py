"""LoHa adapters (training.lora_algo "loha", SDXL_DTYPE_LOHA), the parts that need no GPU: the float64 projections against autograd, the
restated merge's zero cases, the C boundary and the hooks' argument errors, the four-factor layout, the trainer's keys, the state's
cross-algorithm refusal and the LyCORIS-shaped export."""
import ctypes as C
import importlib
import re
from pathlib import Path
from types import SimpleNamespace

import pytest
import torch

import sdxl_amd  # noqa: F401
from sdxl_amd import lib

import _loha_ref as HR
from _isolation import same_bits
from test_host_lora import StandInNet

ROOT = Path(__file__).resolve().parent.parent
CFG = importlib.import_module("sdxl-training-improvements_amd.config")
T = importlib.import_module("sdxl-training-improvements_amd.trainer")
LORA = importlib.import_module("sdxl-training-improvements_amd.lora")

bf = lambda t: t.to(torch.bfloat16)
ONE_OF_EACH = {"plain": "mid_block.attentions.0.transformer_blocks.0.attn1.to_q.weight",
               "geglu": "mid_block.attentions.0.transformer_blocks.0.ff.net.0.proj.weight",
               "conv3": "mid_block.resnets.0.conv1.weight",
               "conv1": "up_blocks.0.resnets.0.conv_shortcut.weight"}
# (label, out, in): a plain linear, a [cout, cin, 3, 3] convolution flattened to [cout, 9 cin], a GEGLU projection [2 C4, in]
SHAPES = [("plain", 24, 40), ("conv", 10, 9 * 8), ("geglu", 2 * 16, 24)]


@pytest.fixture(scope="module")
def net():
    return StandInNet()


def _trainer(net, **training):
    cfg = CFG.Config()
    for k, v in training.items():
        setattr(cfg.training, k, v)
    return T.create_trainer(SimpleNamespace(unet=net), config=cfg, device="cpu")


def factors(out, inn, r, seed):
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g)
    return dict(A1=bf(rn(r, inn)), B1=bf(rn(out, r)), A2=bf(rn(r, inn)), B2=bf(rn(out, r)))


# ------------------------------------------------------------------------------------------------ the reference arithmetic
@pytest.mark.parametrize("label,out,inn", SHAPES, ids=[s[0] for s in SHAPES])
@pytest.mark.parametrize("r", [1, 3, 8])
def test_project64_is_float64_autograd_of_the_hadamard_delta(label, out, inn, r):
    x = factors(out, inn, r, seed=out + r)
    G = torch.randn(out, inn, generator=torch.Generator().manual_seed(5))
    s = 0.37
    leaves = {k: v.double().requires_grad_(True) for k, v in x.items()}
    delta = HR.f32(s) * (leaves["B1"] @ leaves["A1"]) * (leaves["B2"] @ leaves["A2"])
    (G.double() * delta).sum().backward()
    got = HR.project64(G, x["A1"], x["B1"], x["A2"], x["B2"], s)
    assert set(got) == set(HR.NAMES)
    for k in HR.NAMES:
        ref = leaves[k].grad
        assert got[k].shape == ref.shape and float(ref.abs().max()) > 0
        assert float((got[k] - ref).abs().max()) <= 1e-12 * float(ref.abs().max()), k
    assert torch.equal(HR.delta64(x["A1"], x["B1"], x["A2"], x["B2"], s), delta.detach())
    # the bound is positive wherever the gradient is not identically zero, and far below the gradient's own size
    bound = HR.project_bound(G, x["A1"], x["B1"], x["A2"], x["B2"], s)
    for k in HR.NAMES:
        assert bound[k].shape == got[k].shape and float(bound[k].min()) > 0 and float(bound[k].max()) < 1e-3 * float(got[k].abs().max())


def test_the_layout_maps_invert_each_other():
    for kind, out, inn, group in ((HR.CONV3, 10, 72, 8), (HR.GEGLU, 256, 24, 64), (HR.GEGLU, 320, 8, 80), (HR.PLAIN, 7, 16, 0)):
        src = torch.arange(out * inn, dtype=torch.float32).view(out, inn)
        nat = HR.to_native(src, kind, group)
        assert torch.equal(HR.to_source(nat, kind, group), src)
        assert torch.equal(nat, src) == (kind == HR.PLAIN)


def test_merge_restatement_returns_w0_for_the_three_zero_cases_and_is_the_delta_otherwise():
    out, inn, r = 24, 40, 3
    x = factors(out, inn, r, seed=1)
    W0 = bf(torch.randn(out, inn, generator=torch.Generator().manual_seed(2)))
    W0[0, 0] = -0.0
    z = torch.zeros_like(x["B1"])
    assert same_bits(HR.merge(W0, x["A1"], x["B1"], x["A2"], x["B2"], 0.0), W0)
    assert same_bits(HR.merge(W0, x["A1"], z, x["A2"], x["B2"], 0.37), W0)
    assert same_bits(HR.merge(W0, x["A1"], x["B1"], x["A2"], z, 0.37), W0)
    w = HR.merge(W0, x["A1"], x["B1"], x["A2"], x["B2"], 0.37)
    assert not same_bits(w, W0)
    want = W0.double() + HR.delta64(x["A1"], x["B1"], x["A2"], x["B2"], 0.37)
    assert float((w.double() - want).abs().max()) <= 2.0 ** -8 * float(want.abs().max())      # one bf16 rounding (2^-9 relative) and fp32 noise


# ------------------------------------------------------------------------------------------------ the C boundary
def test_boundary_has_the_dtype_the_hooks_and_no_new_function():
    text = (ROOT / "include" / "sdxlstep.h").read_text()
    declared = set(re.findall(r"\b(sdxl_[a-z0-9_]+)\s*\(", text))
    assert len(declared) <= 58 and not any("loha" in n for n in declared)
    assert "#define SDXL_DTYPE_LOHA 5" in text and lib.DTYPE_LOHA == 5
    assert {"sdxl_op_loha_merge", "sdxl_op_loha_project"} <= set(lib.TEST_HOOK_SIGNATURES)
    diag = (ROOT / "include" / "sdxlstep_diag.h").read_text()
    part1 = diag[diag.index("---- part 1"): diag.index("---- part 2")]
    assert "sdxl_op_loha_merge(" in part1 and "sdxl_op_loha_project(" in part1
    L = lib.load()
    assert hasattr(L, "sdxl_op_loha_merge") and hasattr(L, "sdxl_op_loha_project")
    op = lib.LoraOp()
    assert L.sdxl_load_weight(None, None, C.byref(op), lib.DTYPE_LOHA, None) == 1
    assert L.sdxl_export_grad(None, None, C.byref(op), lib.DTYPE_LOHA, None) == 1


def test_hook_argument_errors_are_reported_before_any_launch():
    L = lib.load()
    buf = (C.c_char * 4096)()
    p = C.c_void_p((C.addressof(buf) + 15) & ~15)
    odd = C.c_void_p(p.value + 2)
    # (out, in, rank, scale, kind, group)
    cases = [((8, 72, 0, 1.0, 1, 8), b"rank"), ((8, 72, 65, 1.0, 1, 8), b"rank"), ((8, 72, 128, 1.0, 0, 0), b"rank"), ((8, 36, 4, 1.0, 1, 4), b"multiple of 8"),
             ((8, 12, 4, 1.0, 0, 0), b"multiple of 8"), ((8, 72, 4, 1.0, 3, 8), b"kind"), ((8, 72, 4, 1.0, -1, 8), b"kind"),
             ((8, 72, 4, 1.0, 1, 16), b"9 cin"), ((128, 8, 4, 1.0, 2, 48), b"groups"), ((130, 8, 4, 1.0, 2, 64), b"groups"),
             ((8, 72, 4, float("nan"), 1, 8), b"finite"), ((8, 72, 4, float("inf"), 0, 0), b"finite"), ((0, 72, 4, 1.0, 0, 0), b"[0][72]")]
    for args, msg in cases:
        assert L.sdxl_op_loha_merge(p, p, p, p, p, p, *args, None) == 1 and msg in L.sdxl_last_error(), (args, L.sdxl_last_error())
        assert L.sdxl_op_loha_project(p, p, p, p, p, p, p, p, p, *args, None) == 1 and msg in L.sdxl_last_error(), (args, L.sdxl_last_error())
    ok = (8, 72, 4, 1.0, 1, 8)
    for at in range(6):
        ptrs = [p] * 6
        ptrs[at] = odd
        assert L.sdxl_op_loha_merge(*ptrs, *ok, None) == 1 and b"aligned" in L.sdxl_last_error(), at
        ptrs[at] = None
        assert L.sdxl_op_loha_merge(*ptrs, *ok, None) == 1, at
    for at in range(9):
        ptrs = [p] * 9
        ptrs[at] = odd
        assert L.sdxl_op_loha_project(*ptrs, *ok, None) == 1 and b"aligned" in L.sdxl_last_error(), at
        ptrs[at] = None
        assert L.sdxl_op_loha_project(*ptrs, *ok, None) == 1, at


# ------------------------------------------------------------------------------------------------ layout, ranges, initialisation
def test_layout_ranges_views_and_initialisation_of_one_target_of_each_kind(net):
    r = 4
    mods = [k[: -len(".weight")] for k in ONE_OF_EACH.values()]
    ad = LORA.LoRAAdapters(net, rank=r, alpha=2.0, targets=mods, seed=3, kinds="all", algo="loha")
    assert ad.algo == "loha" and ad.dtype == lib.DTYPE_LOHA == 5 and set(ad.targets) == set(ONE_OF_EACH.values())
    ranges = ad.param_ranges()
    assert len(ranges) == 4 * len(ad.targets)
    cur, base = 0, 0
    pad8 = lambda n: (n + 7) // 8 * 8
    for k in ad.targets:
        shape = net.shapes[k]
        o, i = shape[0], 1
        for v in shape[1:]:
            i *= v
        a1, b1, a2, b2, oo, ii = ad.layout[k]
        assert (oo, ii) == (o, i) and i % 8 == 0
        mod = k[: -len(".weight")]
        for off, n, name in ((a1, r * i, "hada_w1_b"), (b1, o * r, "hada_w1_a"), (a2, r * i, "hada_w2_b"), (b2, o * r, "hada_w2_a")):
            assert off == cur and ranges[f"{mod}.{name}"] == (off, pad8(n))
            cur += pad8(n)
        off, n = net.ranges[k]
        assert torch.equal(ad.base[base: base + n], net.weights[off: off + n])
        base += n
        assert ad.A1(k).shape == ad.A2(k).shape == ad.A1(k, grad=True).shape == (r, i)
        assert ad.B1(k).shape == ad.B2(k).shape == ad.B2(k, grad=True).shape == (o, r)
        assert ad.A1(k).data_ptr() == ad.weights.data_ptr() + 2 * a1 and ad.B2(k, grad=True).data_ptr() == ad.grads.data_ptr() + 4 * b2
        # B2 = 0: the delta is zero; the other three are drawn
        assert float(ad.B2(k).abs().max()) == 0.0 and float(HR.delta64(ad.A1(k), ad.B1(k), ad.A2(k), ad.B2(k), ad.scale).abs().max()) == 0.0
        assert same_bits(HR.merge(bf(torch.ones(o, i)), ad.A1(k), ad.B1(k), ad.A2(k), ad.B2(k), ad.scale), bf(torch.ones(o, i)))
        assert 0.8 < float(ad.A1(k).float().std()) < 1.2 and 0.8 < float(ad.A2(k).float().std()) < 1.2
        assert 0.06 < float(ad.B1(k).float().std()) < 0.14
        assert not torch.equal(ad.A1(k), ad.A2(k))
        with pytest.raises(ValueError, match="A1 and A2"):
            ad.A(k)
    assert cur == ad.param_elems == ad.weights.numel() == ad.grads.numel() and base == ad.base.numel()
    again = LORA.LoRAAdapters(net, rank=r, alpha=2.0, targets=mods, seed=3, kinds="all", algo="loha")
    other = LORA.LoRAAdapters(net, rank=r, alpha=2.0, targets=mods, seed=4, kinds="all", algo="loha")
    assert same_bits(again.weights, ad.weights) and not same_bits(other.weights, ad.weights)
    # LoRA's layout and views are what they were
    lo = LORA.LoRAAdapters(net, rank=r, alpha=2.0, targets=mods, seed=3, kinds="all")
    assert lo.algo == "lora" and all(len(v) == 4 for v in lo.layout.values()) and lo.param_elems * 2 == ad.param_elems
    with pytest.raises(ValueError, match="lora_algo"):
        lo.A1(lo.targets[0])
    for bad_rank in (0, 65, 128, True, 4.0):
        with pytest.raises(ValueError, match="lora_rank"):
            LORA.LoRAAdapters(net, rank=bad_rank, algo="loha")
    assert LORA.LoRAAdapters(net, rank=64, targets=["attn1.to_q"], algo="loha").rank == 64
    with pytest.raises(ValueError, match="lora_algo"):
        LORA.LoRAAdapters(net, rank=4, algo="lokr")


# ------------------------------------------------------------------------------------------------ the trainer
def test_trainer_key_values_target_kinds_and_direct_mode(net):
    assert CFG.Config().training.lora_algo == "lora"
    assert _trainer(net, lora_rank=4).lora.algo == "lora"
    tr = _trainer(net, lora_rank=4, lora_algo="loha", lora_target_kinds="all", lora_targets=["ff.net.0.proj", "conv1", "conv_shortcut", "to_q"])
    assert tr.lora.algo == "loha" and tr.lora.dtype == lib.DTYPE_LOHA and tr.lora.kinds == "all"
    assert {len(net.shapes[k]) for k in tr.lora.targets} == {2, 4}
    assert tr.optimizer is not None and set(tr.lora.param_ranges()) == {f"{k[: -len('.weight')]}.{n}" for k in tr.lora.targets
                                                                        for n in ("hada_w1_a", "hada_w1_b", "hada_w2_a", "hada_w2_b")}
    plain = _trainer(net, lora_rank=4, lora_algo="loha")            # the default kinds: the default targets, the same dtype
    assert plain.lora.kinds == "plain" and plain.lora.dtype == lib.DTYPE_LOHA and plain.lora.targets == _trainer(net, lora_rank=4).lora.targets
    with pytest.raises(ValueError, match="2-D"):                     # lora_target_kinds still decides what the patterns may resolve to
        _trainer(net, lora_rank=4, lora_algo="loha", lora_targets=["conv1"])
    with pytest.raises(ValueError, match="interleaved"):
        _trainer(net, lora_rank=4, lora_algo="loha", lora_targets=["ff.net.0.proj"])
    for bad in ("lokr", "", None, True, "LOHA"):
        with pytest.raises(ValueError, match="lora_algo"):
            _trainer(net, lora_rank=4, lora_algo=bad)
    for kinds in ("plain", "all"):
        with pytest.raises(ValueError, match=r"direct.*lora_algo"):
            _trainer(net, lora_rank=4, lora_algo="loha", lora_target_kinds=kinds, lora_backward="direct")
    with pytest.raises(ValueError, match="lora_algo"):
        tr.lora.select("direct")
    class Selecting(StandInNet):
        def set_trainable(self, names, lora=None):
            self.selected = (list(names), lora)

    sel = Selecting()
    fz = _trainer(sel, lora_rank=4, lora_algo="loha", lora_backward="project_frozen", lora_targets=["attn1.to_q"])
    assert fz.lora_backward == "project_frozen" and sel.selected[1] is None
    assert sel.selected[0] == LORA.trainable_for("project_frozen", fz.lora.targets, sel.shapes) and len(sel.selected[0]) > len(fz.lora.targets)
    with pytest.raises(ValueError, match=r"lora_rank.*64"):
        _trainer(net, lora_rank=65, lora_algo="loha")
    assert _trainer(net, lora_rank=64, lora_algo="loha", lora_targets=["attn1.to_q"]).lora.rank == 64
    assert _trainer(net, lora_rank=65, lora_targets=["attn1.to_q"]).lora.rank == 65       # LoRA keeps its own cap
    for kw, msg in ((dict(use_ema=True), "use_ema"), (dict(shard_optimizer=True), "shard_optimizer")):
        with pytest.raises(ValueError, match=msg):
            _trainer(net, lora_rank=4, lora_algo="loha", **kw)


# ------------------------------------------------------------------------------------------------ state and export
def test_state_round_trip_and_cross_algorithm_refusal(net, tmp_path):
    mods = ["attn1.to_q", "conv1"]
    ad = LORA.LoRAAdapters(net, rank=4, alpha=2.0, targets=mods, seed=1, kinds="all", algo="loha")
    sd = ad.state_dict()
    assert sd["algo"] == "loha" and sd["kinds"] == "all"
    other = LORA.LoRAAdapters(net, rank=4, alpha=2.0, targets=mods, seed=9, kinds="all", algo="loha")
    assert not same_bits(other.weights, ad.weights)
    other.load_state_dict(sd)
    assert same_bits(other.weights, ad.weights)
    lo = LORA.LoRAAdapters(net, rank=4, alpha=2.0, targets=mods, seed=1, kinds="all")
    lsd = lo.state_dict()
    assert "algo" not in lsd and set(lsd) == {"rank", "alpha", "seed", "targets", "shapes", "weights", "kinds"}
    assert set(LORA.LoRAAdapters(net, rank=4, targets=["attn1.to_q"]).state_dict()) == {"rank", "alpha", "seed", "targets", "shapes", "weights"}
    for holder, state in ((ad, lsd), (lo, sd)):
        before = holder.weights.clone()
        with pytest.raises(ValueError, match="lora state: lora_algo"):
            holder.load_state_dict(state)
        assert same_bits(holder.weights, before)
    # ... and through the trainers' loader, both ways
    a = _trainer(net, lora_rank=4, lora_algo="loha", lora_targets=["to_q"])
    b = _trainer(net, lora_rank=4, lora_targets=["to_q"])
    for src, dst, sub in ((a, b, "ha"), (b, a, "ra")):
        d = tmp_path / sub
        d.mkdir()
        torch.save(src.lora.state_dict(), str(d / "lora_state.pt"))
        before = dst.lora.weights.clone()
        with pytest.raises(ValueError, match="lora_algo"):
            dst.load_lora_state(d)
        assert same_bits(dst.lora.weights, before)


def test_export_names_shapes_and_the_rebuilt_delta(net, tmp_path):
    from safetensors.torch import load_file
    r = 4
    tr = _trainer(net, lora_rank=r, lora_alpha=2.0, lora_algo="loha", lora_target_kinds="all", lora_seed=2,
                  lora_targets=[k[: -len(".weight")] for k in ONE_OF_EACH.values()])
    ad = tr.lora
    g = torch.Generator().manual_seed(7)
    for k in ad.targets:
        ad.B2(k).copy_(bf(torch.randn(ad.B2(k).shape, generator=g) * 0.1))
    d = tr.save_checkpoint(tmp_path / "ck")
    assert (d / "lycoris_loha.safetensors").exists() and not (d / "pytorch_lora_weights.safetensors").exists() and (d / "lora_state.pt").exists()
    ex = load_file(str(d / "lycoris_loha.safetensors"))
    assert set(ex) == set(ad.export_tensors()) and len(ex) == 5 * len(ad.targets)
    assert all(re.fullmatch(r"lora_unet_[A-Za-z0-9_]+\.(hada_w[12]_[ab]|alpha)", k) for k in ex)
    for kind, k in ONE_OF_EACH.items():
        shape = net.shapes[k]
        o, i = shape[0], 1
        for v in shape[1:]:
            i *= v
        pre = "lora_unet_" + k[: -len(".weight")].replace(".", "_")
        w1a, w1b, w2a, w2b, alpha = (ex[f"{pre}.{n}"] for n in ("hada_w1_a", "hada_w1_b", "hada_w2_a", "hada_w2_b", "alpha"))
        assert w1a.shape == w2a.shape == (o, r) and w1b.shape == w2b.shape == (r, i) and alpha.shape == () and float(alpha) == 2.0, kind
        assert all(t.dtype == torch.float32 for t in (w1a, w1b, w2a, w2b, alpha))
        assert torch.equal(w1a, ad.B1(k).float()) and torch.equal(w1b, ad.A1(k).float())          # s is not folded in
        assert torch.equal(w2a, ad.B2(k).float()) and torch.equal(w2b, ad.A2(k).float())
        rebuilt = (float(alpha) / r) * (w1a.double() @ w1b.double()) * (w2a.double() @ w2b.double())
        want = HR.delta64(ad.A1(k), ad.B1(k), ad.A2(k), ad.B2(k), ad.scale)
        assert torch.equal(rebuilt, want) and float(want.abs().max()) > 0, kind
        assert rebuilt.reshape(shape).shape == tuple(shape)
    # a LoRA trainer keeps its file
    d2 = _trainer(net, lora_rank=r, lora_targets=["attn1.to_q"]).save_checkpoint(tmp_path / "ck2")
    assert (d2 / "pytorch_lora_weights.safetensors").exists() and not (d2 / "lycoris_loha.safetensors").exists()
