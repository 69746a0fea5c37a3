"""LoRA on the packed layouts (training.lora_target_kinds "all", SDXL_DTYPE_LORA_LAYOUTS), the parts that need no GPU: which tensors the
opt-in accepts and which refusals stay, the adapter layout and the PEFT-shaped export of one target of each kind, the state round trip and
the cross-kind refusal, the C boundary, and the two index maps (source element -> native element) restated in numpy against an emulation
of repack_kernel's formulas (csrc/engine.hip) -- the map the GPU tests of tests/test_gpu_lora_layouts.py rest on."""
import ctypes as C
import importlib
import re
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import sdxl_amd  # noqa: F401
from oracle import unet_ref as U
from sdxl_amd import lib

from test_host_lora import StandInNet

ROOT = Path(__file__).resolve().parent.parent
CFG = importlib.import_module("sdxl-training-improvements_amd.config")
T = importlib.import_module("sdxl-training-improvements_amd.trainer")
LORA = importlib.import_module("sdxl-training-improvements_amd.lora")

bf = lambda t: t.to(torch.bfloat16)
EVERY = ["to_q", "to_k", "to_v", "to_out.0", "ff.net.0.proj", "ff.net.2", "proj_in", "proj_out", "conv1", "conv2", "conv_shortcut",
         "downsamplers.0.conv", "upsamplers.0.conv", "conv_out", "time_emb_proj", "linear_1", "linear_2"]
ONE_OF_EACH = {"plain": "mid_block.attentions.0.transformer_blocks.0.attn1.to_q.weight",
               "geglu": "mid_block.attentions.0.transformer_blocks.0.ff.net.0.proj.weight",
               "conv3": "mid_block.resnets.0.conv1.weight",
               "conv1": "up_blocks.0.resnets.0.conv_shortcut.weight"}


@pytest.fixture(scope="module")
def net():
    return StandInNet()


def _trainer(net, **training):
    cfg = CFG.Config()
    for k, v in training.items():
        setattr(cfg.training, k, v)
    return T.create_trainer(SimpleNamespace(unet=net), config=cfg, device="cpu")


# ------------------------------------------------------------------------------------------------ the index maps
def native_of_conv3(cout, cin, ci_pad):
    """native element of every source element of a [cout][cin][3][3] tensor, the issue's table: (o 9 + tap) ci_pad + c for i = c 9 + tap"""
    o, i = np.divmod(np.arange(cout * cin * 9, dtype=np.int64), cin * 9)
    c, tap = np.divmod(i, 9)
    return (o * 9 + tap) * ci_pad + c


def native_row_of_geglu(C4, G):
    """native row of every source row of a [2 C4][in] GEGLU projection: (c / G) 2G + half G + c % G, half = o / C4, c = o % C4"""
    half, c = np.divmod(np.arange(2 * C4, dtype=np.int64), C4)
    return (c // G) * 2 * G + half * G + c % G


def repack_emulation(src: torch.Tensor, kind: int, co: int, ci: int, ci_pad: int, native_elems: int) -> torch.Tensor:
    """repack_kernel(to_native = 1) written out element by element the way the kernel's body reads (kind 1 and kind 2 branches)"""
    dst = torch.zeros(native_elems, dtype=src.dtype)
    flat = src.reshape(-1)
    for i in range(flat.numel()):
        if kind == 1:
            o = i // (ci * 9)
            rem = i - o * ci * 9
            c = rem // 9
            tap = rem - c * 9
            nat = (o * 9 + tap) * ci_pad + c
        else:
            r = i // ci
            k = i - r * ci
            c4 = co // 2
            half = r // c4
            c = r - half * c4
            G = ci_pad
            nat = ((c // G) * (2 * G) + half * G + (c % G)) * ci + k
        dst[nat] = flat[i]
    return dst


@pytest.mark.parametrize("cin", [8, 24])
def test_conv_map_is_repack_kernels(cin):
    cout = 5
    src = torch.arange(cout * cin * 9, dtype=torch.float32).reshape(cout, cin, 3, 3) + 1
    nat = repack_emulation(src, 1, cout, cin, cin, cout * 9 * cin)
    m = native_of_conv3(cout, cin, cin)
    assert sorted(m.tolist()) == list(range(cout * 9 * cin))                      # ci_pad == cin: a bijection onto the native range
    assert torch.equal(nat[torch.from_numpy(m)], src.reshape(-1))
    # the kernels' view: native rows are [cout][9 cin]; native column j = tap cin + c holds source column c 9 + tap
    j = np.arange(9 * cin)
    src_col = (j % cin) * 9 + j // cin
    assert torch.equal(nat.view(cout, 9 * cin), src.reshape(cout, cin * 9)[:, torch.from_numpy(src_col)])
    # padded input channels (conv_in: 4 in 8) leave native elements without a source element: refused, so never mapped
    assert len(set(native_of_conv3(2, 4, 8).tolist())) == 2 * 4 * 9 < 2 * 9 * 8


@pytest.mark.parametrize("C4,G", [(64, 64), (320, 80)])
def test_geglu_map_is_repack_kernels(C4, G):
    inn = 8
    src = torch.arange(2 * C4 * inn, dtype=torch.float32).reshape(2 * C4, inn) + 1
    nat = repack_emulation(src, 2, 2 * C4, inn, G, 2 * C4 * inn).view(2 * C4, inn)
    rows = native_row_of_geglu(C4, G)
    assert sorted(rows.tolist()) == list(range(2 * C4))
    assert torch.equal(nat[torch.from_numpy(rows)], src)
    # the kernels' inverse: native row r -> source row
    r = np.arange(2 * C4)
    grp, rem = np.divmod(r, 2 * G)
    half = rem // G
    src_row = half * C4 + grp * G + rem - half * G
    assert np.array_equal(rows[src_row], r) and torch.equal(nat, src[torch.from_numpy(src_row)])


# ------------------------------------------------------------------------------------------------ targets
def test_all_kinds_resolve_every_weight_but_conv_in_on_sdxl_base():
    shapes = {k: tuple(v) for k, v in U.param_shapes(U.SDXL_BASE).items()}
    t = LORA.resolve_targets(shapes, EVERY, kinds="all")
    want = [k for k, v in shapes.items() if k.endswith(".weight") and len(v) in (2, 4) and k != "conv_in.weight"]
    assert t == want
    assert sum(k.endswith("ff.net.0.proj.weight") for k in t) == 70
    assert sum(len(shapes[k]) == 4 for k in t) > 0 and "conv_out.weight" in t
    lay, _total = LORA.adapter_layout(shapes, t, 16)
    assert all(i % 8 == 0 for _a, _b, _o, i in lay.values())
    assert LORA.resolve_targets(shapes, LORA.DEFAULT_TARGETS, kinds="all") == LORA.resolve_targets(shapes, LORA.DEFAULT_TARGETS)


def test_conv_in_is_refused_by_name_and_plain_keeps_its_messages(net):
    with pytest.raises(ValueError, match=r"conv_in\.weight.*`in`"):
        LORA.resolve_targets(net.shapes, ["to_q", "conv_in"], kinds="all")
    with pytest.raises(ValueError, match="matches no tensor"):
        LORA.resolve_targets(net.shapes, ["no_such_module"], kinds="all")
    with pytest.raises(ValueError, match="2-D and 4-D"):
        LORA.resolve_targets({"x.norm.weight": (64,), **net.shapes}, ["norm"], kinds="all")
    for kw in ({}, {"kinds": "plain"}):
        for pat, msg in (("ff.net.0.proj", "interleaved"), ("conv1", "2-D"), ("conv_in", "2-D")):
            with pytest.raises(ValueError, match=msg):
                LORA.resolve_targets(net.shapes, ["to_q", pat], **kw)
    with pytest.raises(ValueError, match="lora_target_kinds"):
        LORA.resolve_targets(net.shapes, ["to_q"], kinds="locon")


def test_trainer_key_values_and_direct_mode(net):
    assert CFG.Config().training.lora_target_kinds == "plain"
    tr = _trainer(net, lora_rank=4, lora_target_kinds="all", lora_targets=["ff.net.0.proj", "conv1", "conv_shortcut", "to_q"])
    assert tr.lora.kinds == "all" and tr.lora.dtype == lib.DTYPE_LORA_LAYOUTS == 4
    assert {len(net.shapes[k]) for k in tr.lora.targets} == {2, 4}
    plain = _trainer(net, lora_rank=4)
    assert plain.lora.kinds == "plain" and plain.lora.dtype == lib.DTYPE_LORA == 2
    for bad in ("locon", "", None, True, "ALL"):
        with pytest.raises(ValueError, match="lora_target_kinds"):
            _trainer(net, lora_rank=4, lora_target_kinds=bad)
    with pytest.raises(ValueError, match="2-D"):                                         # the key absent or "plain": today's refusal
        _trainer(net, lora_rank=4, lora_target_kinds="plain", lora_targets=["conv1"])
    with pytest.raises(ValueError, match=r"direct.*conv1\.weight"):
        _trainer(net, lora_rank=4, lora_target_kinds="all", lora_targets=["to_q", "conv1"], lora_backward="direct")
    with pytest.raises(ValueError, match=r"direct.*ff\.net\.0\.proj\.weight"):
        _trainer(net, lora_rank=4, lora_target_kinds="all", lora_targets=["ff.net.0.proj"], lora_backward="direct")
    for kw, msg in ((dict(use_ema=True), "use_ema"), (dict(shard_optimizer=True), "shard_optimizer")):
        with pytest.raises(ValueError, match=msg):
            _trainer(net, lora_rank=4, lora_target_kinds="all", **kw)
    # project_frozen keeps every tensor of the ops that hold a target, whatever the kind
    names = LORA.trainable_for("project_frozen", [ONE_OF_EACH["conv3"], ONE_OF_EACH["geglu"]], net.shapes)
    assert set(names) == {ONE_OF_EACH["conv3"], ONE_OF_EACH["conv3"].replace(".weight", ".bias"), ONE_OF_EACH["geglu"],
                          ONE_OF_EACH["geglu"].replace(".weight", ".bias")}


# ------------------------------------------------------------------------------------------------ layout, export, state
def test_layout_and_export_shapes_of_one_target_of_each_kind(net):
    r = 4
    mods = [k[: -len(".weight")] for k in ONE_OF_EACH.values()]
    ad = LORA.LoRAAdapters(net, rank=r, alpha=2.0, targets=mods, seed=3, kinds="all")
    assert set(ad.targets) == set(ONE_OF_EACH.values())
    g = torch.Generator().manual_seed(2)
    cur, base = 0, 0
    for k in ad.targets:
        shape = net.shapes[k]
        o, i = shape[0], int(np.prod(shape[1:]))
        a, b, oo, ii = ad.layout[k]
        assert (a, oo, ii) == (cur, o, i) and i % 8 == 0
        cur += (r * i + 7) // 8 * 8
        assert b == cur
        cur += (o * r + 7) // 8 * 8
        off, n = net.ranges[k]
        assert n == o * i and torch.equal(ad.base[base: base + n], net.weights[off: off + n])      # W0: the native range, in target order
        base += n
        assert ad.A(k).shape == (r, i) and ad.B(k).shape == (o, r) and float(ad.B(k).abs().max()) == 0.0
        ad.B(k).copy_(bf(torch.randn(o, r, generator=g) * 0.02))
    assert cur == ad.param_elems and base == ad.base.numel()
    ex = ad.export_tensors()
    assert len(ex) == 2 * len(ad.targets) and all(re.fullmatch(r"unet\..+\.lora_[AB]\.weight", k) for k in ex)
    for kind, k in ONE_OF_EACH.items():
        shape, mod = net.shapes[k], k[: -len(".weight")]
        la, lb = ex[f"unet.{mod}.lora_A.weight"], ex[f"unet.{mod}.lora_B.weight"]
        assert la.dtype == lb.dtype == torch.float32 and la.is_contiguous() and lb.is_contiguous()
        if len(shape) == 4:
            assert la.shape == (r, *shape[1:]) and lb.shape == (shape[0], r, 1, 1), kind
            assert shape[2:] == ((3, 3) if kind == "conv3" else (1, 1))
        else:
            assert la.shape == (r, shape[1]) and lb.shape == (shape[0], r), kind
        assert torch.equal(la.reshape(r, -1), ad.A(k).float()) and torch.equal(lb.reshape(shape[0], r), ad.B(k).float() * 0.5)
        # as a convolution pair: up(1x1) o down(kh x kw) has the kernel s B A reshaped like the layer's weight
        delta = (lb.reshape(shape[0], r).double() @ la.reshape(r, -1).double()).reshape(shape)
        assert delta.shape == shape and float(delta.abs().max()) > 0


def test_state_round_trip_and_cross_kind_refusal(net, tmp_path):
    mods = ["attn1.to_q", "conv1"]
    ad = LORA.LoRAAdapters(net, rank=4, alpha=2.0, targets=mods, seed=1, kinds="all")
    for k in ad.targets:
        ad.B(k).copy_(bf(torch.randn(ad.B(k).shape, generator=torch.Generator().manual_seed(7)) * 0.02))
    sd = ad.state_dict()
    assert sd["kinds"] == "all"
    other = LORA.LoRAAdapters(net, rank=4, alpha=2.0, targets=mods, seed=9, kinds="all")
    assert not torch.equal(other.weights, ad.weights)
    other.load_state_dict(sd)
    assert torch.equal(other.weights.view(torch.int16), ad.weights.view(torch.int16))
    # a plain state has no such key (byte-compatible with what it has always been) and neither kind loads the other's
    plain = LORA.LoRAAdapters(net, rank=4, alpha=2.0, targets=["attn1.to_q"], seed=1)
    psd = plain.state_dict()
    assert "kinds" not in psd and set(psd) == {"rank", "alpha", "seed", "targets", "shapes", "weights"}
    same_targets = LORA.LoRAAdapters(net, rank=4, alpha=2.0, targets=["attn1.to_q"], seed=5, kinds="all")
    for holder, state in ((same_targets, psd), (plain, same_targets.state_dict())):
        before = holder.weights.clone()
        with pytest.raises(ValueError, match="lora state: kinds"):
            holder.load_state_dict(state)
        assert torch.equal(holder.weights.view(torch.int16), before.view(torch.int16))
    # ... and through the trainer's loader
    a = _trainer(net, lora_rank=4, lora_target_kinds="all", lora_targets=["to_q"])
    torch.save(a.lora.state_dict(), str(tmp_path / "lora_state.pt"))
    b = _trainer(net, lora_rank=4, lora_targets=["to_q"])
    before = b.lora.weights.clone()
    with pytest.raises(ValueError, match="kinds"):
        b.load_lora_state(tmp_path)
    assert torch.equal(b.lora.weights, before)


# ------------------------------------------------------------------------------------------------ the C boundary
def test_boundary_has_the_dtype_the_hooks_and_no_new_function():
    text = (ROOT / "include" / "sdxlstep.h").read_text()
    declared = set(re.findall(r"\b(sdxl_[a-z0-9_]+)\s*\(", text))
    assert len(declared) <= 58 and not any("lora" in n for n in declared)
    assert "#define SDXL_DTYPE_LORA_LAYOUTS 4" in text and "#define SDXL_DTYPE_LORA 2" in text and lib.DTYPE_LORA_LAYOUTS == 4
    assert {"sdxl_op_lora_merge_layout", "sdxl_op_lora_project_layout"} <= set(lib.TEST_HOOK_SIGNATURES)
    L = lib.load()
    assert hasattr(L, "sdxl_op_lora_merge_layout") and hasattr(L, "sdxl_op_lora_project_layout")


def test_layout_hook_argument_errors_are_reported_before_any_launch():
    L = lib.load()
    buf = (C.c_char * 4096)()
    p = C.c_void_p((C.addressof(buf) + 15) & ~15)
    odd = C.c_void_p(p.value + 2)
    # (out, in, rank, scale, kind, cin | G, native rows)
    cases = [((8, 72, 0, 1.0, 1, 8, 8), b"rank"), ((8, 72, 129, 1.0, 1, 8, 8), b"rank"), ((8, 36, 4, 1.0, 1, 4, 8), b"multiple of 8"),
             ((8, 72, 4, 1.0, 3, 8, 8), b"kind"), ((8, 72, 4, 1.0, -1, 8, 8), b"kind"), ((8, 72, 4, 1.0, 1, 16, 8), b"9 cin"),
             ((8, 72, 4, 1.0, 1, 0, 8), b"9 cin"), ((8, 72, 4, 1.0, 1, 8, 4), b"native rows"), ((8, 8, 4, 1.0, 0, 0, 16), b"native rows"),
             ((128, 8, 4, 1.0, 2, 64, 256), b"native rows"), ((128, 8, 4, 1.0, 2, 48, 128), b"groups"), ((130, 8, 4, 1.0, 2, 64, 130), b"groups"),
             ((128, 8, 4, 1.0, 2, 0, 128), b"groups"), ((8, 72, 4, float("nan"), 1, 8, 8), b"finite")]
    for args, msg in cases:
        assert L.sdxl_op_lora_merge_layout(p, p, p, p, *args, None) == 1 and msg in L.sdxl_last_error(), (args, L.sdxl_last_error())
        assert L.sdxl_op_lora_project_layout(p, p, p, p, p, *args, None) == 1 and msg in L.sdxl_last_error(), (args, L.sdxl_last_error())
    ok = (8, 72, 4, 1.0, 1, 8, 8)
    assert L.sdxl_op_lora_merge_layout(p, odd, p, p, *ok, None) == 1 and b"aligned" in L.sdxl_last_error()
    assert L.sdxl_op_lora_merge_layout(None, p, p, p, *ok, None) == 1
    assert L.sdxl_op_lora_project_layout(p, p, p, p, None, *ok, None) == 1
    op = lib.LoraOp()
    assert L.sdxl_load_weight(None, None, C.byref(op), lib.DTYPE_LORA_LAYOUTS, None) == 1
    assert L.sdxl_export_grad(None, None, C.byref(op), lib.DTYPE_LORA_LAYOUTS, None) == 1
