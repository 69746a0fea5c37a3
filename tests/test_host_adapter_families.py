"""The adapter families' one description (lora.target_factors and the family table), no GPU: for every family on the tiny stand-in net,
adapter_layout, param_ranges(), param_shapes() and the accessors' views say the same thing about every factor of every target, the ranges
tile the arena exactly, and nothing outside a factor is ever written."""
import importlib

import pytest
import torch

import sdxl_amd  # noqa: F401

from test_host_lora import StandInNet

LORA = importlib.import_module("sdxl-training-improvements_amd.lora")

EVERY_KIND = ["to_q", "to_k", "to_v", "to_out.0", "ff.net.0.proj", "ff.net.2", "conv1", "conv2", "conv_shortcut", "proj_in", "proj_out",
              "time_emb_proj", "conv_out"]
CONFIGS = {"lora-plain": dict(algo="lora", kinds="plain"),
           "lora-all": dict(algo="lora", kinds="all", targets=EVERY_KIND),
           "loha": dict(algo="loha", kinds="all", targets=EVERY_KIND),
           "kronecker-rule": dict(algo="kronecker", kinds="all", targets=EVERY_KIND, factor=2),
           "kronecker-full": dict(algo="kronecker", kinds="all", targets=EVERY_KIND, full=True),
           "dora": dict(algo="dora", kinds="all", targets=EVERY_KIND)}
# rank 3: out * rank is no multiple of 8 where out is none -- on this net conv_out's 4 rows, which kinds "all" can target; every other out and
# every in is a multiple of 64 -- so B [4, 3] and mu [4] are followed by pads (a full LoKr target has no factor with a rank in it).  The form rule 2 rank >= max(out_k, in_n) gives the tiny net
# (every channel count a multiple of 64, so in_n >= 8 for every factor) full targets at rank 16 only: that is the mixed table.
RANKS = (3, 16)
MIXED = ("kronecker-rule", 16)


@pytest.fixture(scope="module")
def net():
    return StandInNet()


def prod(shape):
    n = 1
    for v in shape:
        n *= int(v)
    return n


@pytest.mark.parametrize("rank", RANKS)
@pytest.mark.parametrize("label", list(CONFIGS))
def test_layout_ranges_shapes_and_views_agree_and_tile_the_arena(net, label, rank):
    kw = CONFIGS[label]
    algo, factor, full = kw["algo"], kw.get("factor", -1), kw.get("full", False)
    ad = LORA.LoRAAdapters(net, rank=rank, seed=3, **kw)
    lay, total = LORA.adapter_layout(net.param_shapes(), ad.targets, rank, algo, factor, full)
    assert lay == ad.layout and list(lay) == list(ad.targets) and total == ad.param_elems
    ranges, shapes = ad.param_ranges(), ad.param_shapes()
    inside = torch.zeros(ad.param_elems, dtype=torch.bool)
    keys, cur, padded, forms = [], 0, 0, set()
    for k in ad.targets:
        fs = LORA.target_factors(algo, net.shapes[k], rank, factor, full)
        assert lay[k][-2:] == (net.shapes[k][0], prod(net.shapes[k][1:])) and len(lay[k]) == len(fs) + 2
        forms.add(tuple(f.name for f in fs))
        for n, f in enumerate(fs):
            key = f"{k[: -len('.weight')]}.{f.leaf}"
            keys.append(key)
            off, count = ranges[key]
            assert off == lay[k][n] == cur and off % 8 == 0, (key, off, cur)             # ascending, disjoint, no gap
            assert shapes[key] == f.shape and count == -(-prod(f.shape) // 8) * 8, key    # the shape's product padded to 8
            padded += count != prod(f.shape)
            views = [getattr(ad, f.name)(k), ad.view(f.name, k)]
            views += [ad.factor(f.name, k)] if algo == "loha" else [ad.factor_view(f.name, k)] if algo == "kronecker" else []
            for v in views:                                                               # starts at its range, has its shape
                assert tuple(v.shape) == f.shape and v.is_contiguous() and v.dtype == torch.bfloat16
                assert v.data_ptr() == ad.weights.data_ptr() + 2 * off, key
            for g in (getattr(ad, f.name)(k, grad=True), ad.view(f.name, k, grad=True)):  # the gradient view aliases the same offsets
                assert tuple(g.shape) == f.shape and g.is_contiguous() and g.dtype == torch.float32
                assert g.data_ptr() == ad.grads.data_ptr() + 4 * off, key
            inside[off: off + prod(f.shape)] = True
            cur = off + count
    assert cur == ad.param_elems == ad.weights.numel() == ad.grads.numel()                # ... and end exactly at param_elems
    assert list(ranges) == list(shapes) == keys                                           # the same keys in target_factors' order
    assert not bool(ad.weights[~inside].any()) and bool(ad.weights[inside].any())         # nothing outside a factor is written
    assert not bool(ad.grads.any())
    assert padded > 0 or rank != 3 or kw["kinds"] == "plain" or full, (label, padded)     # rank 3 is here for the pads
    if algo == "kronecker":
        want = {("C", "W2")} if full else {("C", "W2"), ("C", "B", "A")} if (label, rank) == MIXED else {("C", "B", "A")}
        assert forms == want and {tuple(ad.lokr_factors(k)) for k in ad.targets} == want


def test_every_family_has_its_table_row_and_its_factors():
    assert tuple(LORA.FAMILIES) == LORA.LORA_ALGOS and LORA.EXPORT_FILES == {a: f.file for a, f in LORA.FAMILIES.items()}
    names = {algo: tuple((f.name, f.leaf, f.shape) for f in LORA.target_factors(algo, (12, 16, 3, 3), 3)) for algo in LORA.LORA_ALGOS}
    assert names["lora"] == (("A", "lora_A.weight", (3, 144)), ("B", "lora_B.weight", (12, 3)))
    assert names["dora"] == (("A", "lora_A", (3, 144)), ("B", "lora_B", (12, 3)), ("mu", "lora_magnitude", (12,)))
    assert names["loha"] == (("A1", "hada_w1_b", (3, 144)), ("B1", "hada_w1_a", (12, 3)), ("A2", "hada_w2_b", (3, 144)), ("B2", "hada_w2_a", (12, 3)))
    assert names["kronecker"] == (("C", "lokr_w1", (3, 4)), ("W2", "lokr_w2", (4, 36)))      # 2 * 3 >= max(4, 4): the rule says full
    assert tuple((f.name, f.leaf, f.shape) for f in LORA.target_factors("kronecker", (12, 16, 3, 3), 1)) == \
        (("C", "lokr_w1", (3, 4)), ("B", "lokr_w2_a", (4, 1)), ("A", "lokr_w2_b", (1, 36)))
    for algo, fam in LORA.FAMILIES.items():      # every factor the initialisation draws is one the family has
        have = {f.name for full in (False, True) for r in (1, 3) for f in LORA.target_factors(algo, (12, 16, 3, 3), r, -1, full)}
        assert {name for name, _std in fam.init(4)} <= have, algo
    with pytest.raises(ValueError, match="lora_algo"):
        LORA.target_factors("lokr", (8, 8), 2)
