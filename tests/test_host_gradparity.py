"""tests/_gradparity.py on the host: the per-tensor comparison the GPU gradient tests rely on flags what a probe-level check
cannot see (a zeroed bias, one wrong small tensor, a non-zero gradient where the reference is exactly zero) and covers every key."""
import pytest
import torch

from _gradparity import GradParity, compare_autograd, group, role


def _ref():
    g = torch.Generator().manual_seed(0)
    return {"conv_in.weight": torch.randn(8, 4, 3, 3, generator=g), "time_embedding.linear_2.bias": torch.randn(16, generator=g),
            "up_blocks.1.upsamplers.0.conv.bias": torch.randn(8, generator=g), "down_blocks.0.resnets.1.norm1.weight": torch.randn(8, generator=g),
            "mid_block.attentions.0.transformer_blocks.2.attn2.to_out.0.weight": torch.randn(32, 32, generator=g)}


def test_role_and_group():
    assert role("up_blocks.1.attentions.2.transformer_blocks.0.attn1.to_out.0.bias") == \
        "up_blocks.N.attentions.N.transformer_blocks.N.attn1.to_out.N.bias"
    assert role("conv_in.weight") == "conv_in.weight"
    assert group("down_blocks.0.resnets.1.time_emb_proj.bias", 1) == "time-embedding path"
    assert group("add_embedding.linear_1.weight", 2) == "time-embedding path"
    assert group("mid_block.attentions.0.norm.weight", 1) == "norms"
    assert group("conv_norm_out.bias", 1) == "norms"
    assert group("up_blocks.1.upsamplers.0.conv.bias", 1) == "biases"
    assert group("conv_in.weight", 4) == "convs"
    assert group("mid_block.attentions.0.proj_in.weight", 2) == "linears"


def test_close_gradients_pass_and_report_every_role():
    ref = _ref()
    par = GradParity("host")
    for k, r in ref.items():
        par.add(k, r * (1 + 1e-3), r)
    lines = []
    par.check((6e-2, 0.998), expect=ref, printer=lines.append)
    assert sum(" ok   " in ln for ln in lines) == len(ref)         # one line per role, all passing


@pytest.mark.parametrize("fault", ["zero", "small_tensor", "sign"])
def test_one_wrong_tensor_fails_by_name(fault):
    ref = _ref()
    bad = "time_embedding.linear_2.bias" if fault != "small_tensor" else "up_blocks.1.upsamplers.0.conv.bias"
    par = GradParity("host")
    for k, r in ref.items():
        g = r.clone()
        if k == bad:
            g = torch.zeros_like(r) if fault == "zero" else (r * 0.75 if fault == "small_tensor" else -r)
        par.add(k, g, r)
    with pytest.raises(AssertionError, match=r"1 of 5 gradient tensors") as e:
        par.check((6e-2, 0.998), printer=lambda s: None)
    assert f"FAIL {bad}" in str(e.value)


def test_non_finite_fails():
    ref = _ref()
    par = GradParity("host")
    for k, r in ref.items():
        g = r.clone()
        if k == "conv_in.weight":
            g[0, 0, 0, 0] = float("nan")
        par.add(k, g, r)
    with pytest.raises(AssertionError, match="FAIL conv_in.weight"):
        par.check((6e-2, 0.998), printer=lambda s: None)


def test_zero_reference_bar_is_relative_to_the_arena_max():
    ref = _ref()
    ref["down_blocks.0.resnets.1.norm1.weight"].zero_()
    rmax = max(float(r.abs().max()) for r in ref.values())
    for eps, ok in ((0.5e-6, True), (2e-6, False)):
        par = GradParity("host")
        for k, r in ref.items():
            g = r.clone()
            if k == "down_blocks.0.resnets.1.norm1.weight":
                g[3] = eps * rmax
            par.add(k, g, r)
        if ok:
            par.check((6e-2, 0.998), printer=lambda s: None)
        else:
            with pytest.raises(AssertionError, match="FAIL down_blocks.0.resnets.1.norm1.weight"):
                par.check((6e-2, 0.998), printer=lambda s: None)


def test_missing_key_fails():
    ref = _ref()
    par = GradParity("host")
    for k, r in list(ref.items())[1:]:
        par.add(k, r, r)
    with pytest.raises(AssertionError, match="missing"):
        par.check((6e-2, 0.998), expect=ref, printer=lambda s: None)


def test_arena_slices_and_per_role_bar():
    ref = _ref()
    ranges, off = {}, 0
    for k, r in ref.items():
        ranges[k] = (off, r.numel())
        off += r.numel()
    a = torch.cat([r.flatten() for r in ref.values()])
    b = a.clone()
    o, n = ranges["up_blocks.1.upsamplers.0.conv.bias"]
    b[o:o + n] *= 1.08                                                 # rel-L2 0.08 on that tensor only
    par = GradParity("host")
    par.add_arena(b, a, ranges, {k: tuple(r.shape) for k, r in ref.items()})
    assert par.rows["conv_in.weight"].ndim == 4 and par.rows["conv_in.weight"].rel == 0.0
    with pytest.raises(AssertionError, match="FAIL up_blocks.1.upsamplers.0.conv.bias"):
        par.check((6e-2, 0.998), printer=lambda s: None)
    par.check(lambda k: (0.1, 0.998) if role(k) == "up_blocks.N.upsamplers.N.conv.bias" else (6e-2, 0.998), printer=lambda s: None)


def test_compare_autograd_sees_every_parameter_and_frees_its_gradient():
    g = torch.Generator().manual_seed(1)
    w = {"a.weight": torch.randn(5, 3, generator=g).requires_grad_(True), "a.bias": torch.randn(5, generator=g).requires_grad_(True),
         "unused.bias": torch.randn(4, generator=g).requires_grad_(True)}
    x = torch.randn(7, 3, generator=g)
    loss = ((x @ w["a.weight"].T + w["a.bias"]) ** 2).sum()
    want = dict(zip(("a.weight", "a.bias"), torch.autograd.grad(loss, [w["a.weight"], w["a.bias"]], retain_graph=True)))
    want["unused.bias"] = torch.zeros(4)
    par = GradParity("host")
    compare_autograd(par, loss, w, lambda k: want[k])
    assert all(p.grad is None for p in w.values())
    assert par.rows["a.weight"].rel < 1e-12 and par.rows["a.bias"].rel < 1e-12 and par.rows["unused.bias"].r == 0.0
    par.check((1e-9, 0.999999), expect=w, printer=lambda s: None)
