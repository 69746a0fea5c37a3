"""DoRA adapters (training.lora_algo "dora", SDXL_DTYPE_DORA), the parts that need no GPU: the layout, offsets and padding, the refusals, the
mu <-> m relation, the export that rebuilds the weight, the C boundary, the case table of tests/test_gpu_dora.py against the kernel's
constants, and six seeded mistakes that the comparison of tests/_dora_ref.py must catch at a named output while a correct fp32 emulation
summed in another order passes."""
import ctypes as C
import importlib
import re
import shutil
import subprocess
from pathlib import Path
from types import SimpleNamespace

import pytest
import torch

import sdxl_amd  # noqa: F401
from sdxl_amd import lib

import _dora_ref as DR
from _isolation import same_bits
from test_host_lora import StandInNet

ROOT = Path(__file__).resolve().parent.parent
PKG = ROOT / "sdxl-training-improvements_amd"
CFG = importlib.import_module("sdxl-training-improvements_amd.config")
T = importlib.import_module("sdxl-training-improvements_amd.trainer")
LORA = importlib.import_module("sdxl-training-improvements_amd.lora")
BUILD = importlib.import_module("sdxl-training-improvements_amd.build")

bf = lambda t: t.to(torch.bfloat16)
ONE_OF_EACH = {"plain": "mid_block.attentions.0.transformer_blocks.0.attn1.to_q.weight",
               "geglu": "mid_block.attentions.0.transformer_blocks.0.ff.net.0.proj.weight",
               "conv3": "mid_block.resnets.0.conv1.weight",
               "conv1": "up_blocks.0.resnets.0.conv_shortcut.weight"}
pad8 = lambda n: (n + 7) // 8 * 8
pad4 = lambda n: (n + 3) // 4 * 4


@pytest.fixture(scope="module")
def net():
    return StandInNet()


def _trainer(net, **training):
    cfg = CFG.Config()
    for k, v in training.items():
        setattr(cfg.training, k, v)
    return T.create_trainer(SimpleNamespace(unet=net), config=cfg, device="cpu")


def fill_norm0(ad):
    """what init_norm0 does on the device, restated (these tests have no library to run it)"""
    at = 0
    for k in ad.targets:
        o, i = ad.layout[k][-2:]
        ad.row_norm(k).copy_(ad.base[at: at + o * i].view(o, i).float().pow(2).sum(1).sqrt())
        at += o * i


# ------------------------------------------------------------------------------------------------ layout, ranges, accessors
def test_layout_offsets_padding_ranges_and_initialisation(net):
    r = 3
    mods = [k[: -len(".weight")] for k in ONE_OF_EACH.values()]
    ad = LORA.LoRAAdapters(net, rank=r, alpha=1.5, targets=mods, seed=3, kinds="all", algo="dora")
    assert ad.algo == "dora" and ad.dtype == lib.DTYPE_DORA == 8 and ad.scale == 0.5
    lay, total = LORA.adapter_layout(net.param_shapes(), ad.targets, r, "dora")
    assert lay == ad.layout and total == ad.param_elems
    cur, ncur, ranges = 0, 0, ad.param_ranges()
    for k in ad.targets:
        shape = net.shapes[k]
        o, i = shape[0], int(torch.tensor(shape[1:]).prod())
        a, b, m, oo, ii = ad.layout[k]
        assert (a, b, m, oo, ii) == (cur, cur + pad8(r * i), cur + pad8(r * i) + pad8(o * r), o, i), k
        cur = m + pad8(o)
        assert ad.norm_offsets[k] == ncur
        ncur += pad4(o)
        mod = k[: -len(".weight")]
        assert ranges[f"{mod}.lora_A"] == (a, pad8(r * i)) and ranges[f"{mod}.lora_B"] == (b, pad8(o * r)) and ranges[f"{mod}.lora_magnitude"] == (m, pad8(o))
        assert ad.A(k).shape == (r, i) and ad.B(k).shape == (o, r) and ad.mu(k).shape == (o,) and ad.mu(k, grad=True).dtype == torch.float32
        assert ad.A(k).data_ptr() == ad.weights.data_ptr() + 2 * a and ad.mu(k).data_ptr() == ad.weights.data_ptr() + 2 * m
        assert ad.mu(k, grad=True).data_ptr() == ad.grads.data_ptr() + 4 * m
        assert float(ad.A(k).float().abs().max()) > 0 and float(ad.B(k).float().abs().max()) == 0 and float(ad.mu(k).float().abs().max()) == 0
        assert ad.row_norm(k).shape == (o,) and ad.row_norm(k, base=False).data_ptr() == ad.norm.data_ptr() + 4 * ad.norm_offsets[k]
    assert cur == ad.param_elems and len(ranges) == 3 * len(ad.targets) and ad.norm0.numel() == ad.norm.numel() == ncur
    # LoRA's own layout and names are what they were
    lo = LORA.LoRAAdapters(net, rank=r, alpha=1.5, targets=mods, seed=3, kinds="all")
    assert all(len(v) == 4 for v in lo.layout.values()) and all(n.endswith(".weight") for n in lo.param_ranges())
    assert all(same_bits(lo.A(k), ad.A(k)) for k in ad.targets)            # the same initialisation of A
    with pytest.raises(ValueError, match="dora"):
        lo.mu(lo.targets[0])
    with pytest.raises(ValueError, match="lora_algo"):
        ad.A1(ad.targets[0])


def test_magnitude_is_n0_times_one_plus_mu_and_mu_zero_is_n0_exactly(net):
    ad = LORA.LoRAAdapters(net, rank=2, targets=[ONE_OF_EACH["plain"][: -len(".weight")]], algo="dora")
    k = ad.targets[0]
    fill_norm0(ad)
    n0 = ad.row_norm(k).clone()
    assert float(n0.min()) > 0 and same_bits(ad.magnitude(k), n0)          # mu = 0: m = n0 in fp32, which no bf16 m could hold
    assert not same_bits(bf(n0).float(), n0)
    g = torch.Generator().manual_seed(0)
    ad.mu(k).copy_(bf(torch.randn(n0.shape, generator=g) * 0.1))
    m = ad.magnitude(k)
    assert m.dtype == torch.float32 and same_bits(m, n0 * (1.0 + ad.mu(k).float()))
    assert torch.allclose(m.double(), DR.magnitude64(n0, ad.mu(k)), rtol=2.0 ** -23, atol=0)
    assert torch.equal(((m.double() / n0.double()) - 1).float().to(torch.bfloat16), ad.mu(k))      # and back


# ------------------------------------------------------------------------------------------------ refusals
def test_unknown_algorithms_direct_ema_and_zero1_are_refused(net):
    tr = _trainer(net, lora_rank=4, lora_algo="dora", lora_target_kinds="all", lora_targets=["ff.net.0.proj", "conv1", "conv_shortcut", "to_q"])
    assert tr.lora.algo == "dora" and tr.lora.dtype == lib.DTYPE_DORA and {len(net.shapes[k]) for k in tr.lora.targets} == {2, 4}
    assert tr.optimizer is not None
    assert _trainer(net, lora_rank=128, lora_algo="dora", lora_targets=["attn1.to_q"]).lora.rank == 128
    for bad in ("lokr", "DoRA", "DORA", "dora ", "", None, True):
        with pytest.raises(ValueError, match="lora_algo"):
            _trainer(net, lora_rank=4, lora_algo=bad)
    with pytest.raises(ValueError, match="lora_algo"):
        LORA.LoRAAdapters(net, rank=4, algo="DoRA")
    for bad_rank in (0, 129, True, 4.0):
        with pytest.raises(ValueError, match="lora_rank"):
            LORA.LoRAAdapters(net, rank=bad_rank, algo="dora")
    for kinds in ("plain", "all"):
        with pytest.raises(ValueError, match=r"direct.*lora_algo"):
            _trainer(net, lora_rank=4, lora_algo="dora", lora_target_kinds=kinds, lora_backward="direct")
    with pytest.raises(ValueError, match="lora_algo"):
        tr.lora.select("direct")
    with pytest.raises(ValueError, match="use_ema"):
        _trainer(net, lora_rank=4, lora_algo="dora", use_ema=True)
    with pytest.raises(ValueError, match="shard_optimizer"):
        _trainer(net, lora_rank=4, lora_algo="dora", shard_optimizer=True)
    with pytest.raises(lib.SdxlError, match="no PyTorch fallback"):        # a missing library is an error, not a torch merge
        tr.lora.merge()


def test_state_records_the_algorithm_and_another_algorithms_state_is_refused(net):
    a = _trainer(net, lora_rank=4, lora_algo="dora", lora_targets=["to_q"])
    g = torch.Generator().manual_seed(1)
    a.lora.weights.copy_(bf(torch.randn(a.lora.param_elems, generator=g)))
    sd = a.lora.state_dict()
    assert sd["algo"] == "dora" and "norm0" not in sd and sd["weights"].dtype == torch.bfloat16
    b = _trainer(net, lora_rank=4, lora_algo="dora", lora_targets=["to_q"])
    b.lora.load_state_dict(sd)
    assert same_bits(b.lora.weights, a.lora.weights)
    for other in (dict(), dict(lora_algo="loha"), dict(lora_algo="kronecker")):
        o = _trainer(net, lora_rank=4, lora_targets=["to_q"], **other)
        before = o.lora.weights.clone()
        with pytest.raises(ValueError, match="lora state: lora_algo"):
            o.lora.load_state_dict(sd)
        assert same_bits(o.lora.weights, before)
        before = b.lora.weights.clone()
        with pytest.raises(ValueError, match="lora state: lora_algo"):
            b.lora.load_state_dict(o.lora.state_dict())
        assert same_bits(b.lora.weights, before)
    assert "algo" not in _trainer(net, lora_rank=4, lora_targets=["to_q"]).lora.state_dict()      # a LoRA state is what it was


# ------------------------------------------------------------------------------------------------ export
def test_export_rebuilds_the_merged_weight_inside_its_bf16_interval(net):
    r = 4
    mods = [k[: -len(".weight")] for k in ONE_OF_EACH.values()]
    ad = LORA.LoRAAdapters(net, rank=r, alpha=2.0, targets=mods, seed=4, kinds="all", algo="dora")      # s = 0.5: folding it into lora_B is exact
    g = torch.Generator().manual_seed(2)
    for k in ad.targets:
        ad.B(k).copy_(bf(torch.randn(ad.B(k).shape, generator=g) * 0.05))
        ad.mu(k).copy_(bf(torch.randn(ad.mu(k).shape, generator=g) * 0.1))
    fill_norm0(ad)
    ex = ad.export_tensors()
    assert LORA.EXPORT_FILES["dora"] == LORA.EXPORT_FILES["lora"]
    at = 0
    for k in ad.targets:
        mod, shape = k[: -len(".weight")], net.shapes[k]
        o, i = ad.layout[k][-2:]
        la, lb, m = ex[f"unet.{mod}.lora_A.weight"], ex[f"unet.{mod}.lora_B.weight"], ex[f"unet.{mod}.lora_magnitude_vector"]
        assert m.dtype == la.dtype == torch.float32 and tuple(m.shape) == (o,)
        assert tuple(la.shape) == ((r,) + tuple(shape[1:])) and tuple(lb.shape) == ((o, r, 1, 1) if len(shape) == 4 else (o, r))
        W0 = ad.base[at: at + o * i].view(o, i)
        at += o * i
        V = W0.double() + lb.double().reshape(o, r) @ la.double().reshape(r, i)
        rebuilt = (m.double() / V.pow(2).sum(1).sqrt())[:, None] * V      # what a DoRA loader forms
        A, B, mu = ad.A(k), ad.B(k), ad.mu(k)
        n32 = DR.v32(W0, A, B, ad.scale)[0].pow(2).sum(1).sqrt()
        restated = DR.merge_given(W0, A, B, mu, ad.scale, ad.row_norm(k), n32)
        delta = DR.bounds(W0, A, B, mu, ad.scale)["W"]
        lo, hi = DR.bf16_interval(rebuilt, delta)
        assert bool(((lo.float() <= restated.float()) & (restated.float() <= hi.float())).all()), k
        assert not same_bits(restated, W0)
    assert set(ex) == {f"unet.{k[: -len('.weight')]}.{n}" for k in ad.targets for n in ("lora_A.weight", "lora_B.weight", "lora_magnitude_vector")}


# ------------------------------------------------------------------------------------------------ the C boundary, the build, the case table
def test_boundary_has_the_dtypes_the_hook_and_no_new_function():
    names = lambda text: set(re.findall(r"\b(sdxl_[a-z0-9_]+)\s*\(", text))
    text = (ROOT / "include" / "sdxlstep.h").read_text()
    declared = names(text)
    assert len(declared) <= 58 and not any("dora" in n for n in declared)
    assert "#define SDXL_DTYPE_DORA 8" in text and "} sdxl_dora_op;" in text and lib.DTYPE_DORA == 8
    diag = (ROOT / "include" / "sdxlstep_diag.h").read_text()
    part1 = diag[diag.index("---- part 1"): diag.index("---- part 2")]
    assert "#define SDXL_DTYPE_DORA_ONE 9" in part1 and "} sdxl_dora_one;" in part1 and lib.DTYPE_DORA_ONE == 9
    assert not any("dora" in n for n in names(diag)) and not any("dora" in n for n in lib.TEST_HOOK_SIGNATURES)
    assert "dora.hip" in BUILD.SOURCES and (PKG / "csrc" / "dora.hip").exists()
    L = lib.load()
    assert not hasattr(L, "sdxl_op_dora_merge")
    op = lib.DoraOp()
    assert L.sdxl_load_weight(None, None, C.byref(op), lib.DTYPE_DORA, None) == 1
    assert L.sdxl_export_grad(None, None, C.byref(op), lib.DTYPE_DORA, None) == 1
    one = lib.DoraOne()
    for fn in (L.sdxl_load_weight, L.sdxl_export_grad):
        assert fn(None, None, None, lib.DTYPE_DORA_ONE, None) == 1 and b"NULL" in L.sdxl_last_error()
        assert fn(None, b"conv_in.weight", C.byref(one), lib.DTYPE_DORA_ONE, None) == 1 and b"no name" in L.sdxl_last_error()
    one = lib.DoraOne(out=8, in_=72, group=8, kind=1, rank=4, mode=0, scale=1.0)
    for fn in (L.sdxl_load_weight, L.sdxl_export_grad):
        assert fn(None, None, C.byref(one), lib.DTYPE_DORA_ONE, None) == 1 and b"aligned" in L.sdxl_last_error()


def test_struct_layout_matches_the_header(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang") or "/opt/rocm/lib/llvm/bin/clang"
    fields = ("op", "mode", "norm0", "norm")
    one_py = [f[0] for f in lib.DoraOne._fields_]
    one_c = ["in" if f == "in_" else f for f in one_py]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "sdxlstep_diag.h"\n'
                   'int main(void) { printf("%zu %zu %zu %d %d", sizeof(sdxl_lora_op), sizeof(sdxl_dora_op), sizeof(sdxl_dora_one), SDXL_DTYPE_DORA, SDXL_DTYPE_DORA_ONE);\n'
                   + "".join(f'  printf(" %zu", offsetof(sdxl_dora_op, {f}));\n' for f in fields)
                   + "".join(f'  printf(" %zu", offsetof(sdxl_dora_one, {f}));\n' for f in one_c)
                   + '  printf("\\n"); return 0; }\n')
    exe = tmp_path / "layout"
    r = subprocess.run([cc, "-I", str(ROOT / "include"), str(src), "-o", str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    out = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True, timeout=60).stdout.split()]
    assert out == [C.sizeof(lib.LoraOp), C.sizeof(lib.DoraOp), C.sizeof(lib.DoraOne), lib.DTYPE_DORA, lib.DTYPE_DORA_ONE] \
        + [getattr(lib.DoraOp, f).offset for f in fields] + [getattr(lib.DoraOne, f).offset for f in one_py]
    assert C.sizeof(lib.LoraOp) == 48 and lib.DoraOp.op.offset == 0 and lib.DoraOp.mode.offset == 48
    assert (lib.DORA_MERGE, lib.DORA_INIT, lib.DORA_RESTORE) == (0, 1, 2)


def test_the_case_table_holds_what_the_issue_lists_and_a_row_longer_than_one_pass():
    kh = (PKG / "csrc" / "kernels.h").read_text()
    const = lambda n: int(re.search(rf"#define {n} (\d+)", kh).group(1))
    cols, rows = const("DORA_R_COLS"), const("DORA_R_ROWS")
    assert rows == const("LORA_B_ROWS")
    by = DR.BY_LABEL
    for label in ("1x8", "8x8", "37x8", "40x24", "130x264", "64x2048", "1280x1280", "conv40x16", "conv8x320", "geglu128g64x24", "geglu160g80x24"):
        assert label in by
    assert by["conv40x16"][1:] == (DR.CONV3, 40, 144, 16) and by["conv8x320"][1:] == (DR.CONV3, 8, 2880, 320)
    assert by["geglu128g64x24"][1:] == (DR.GEGLU, 256, 24, 64) and by["geglu160g80x24"][1:] == (DR.GEGLU, 320, 24, 80)
    _l, kind, out, inn, _g = by[DR.LONG_ROW]
    assert inn > 2 * cols and inn % cols != 0 and inn % 8 == 0            # several passes of the column loop and a last one that is not whole
    assert any(c[2] > rows and c[2] % rows for c in DR.CASES)             # more than one block of rows, the last one not whole
    ranks = {r for _c, r in DR.FORMS}
    assert ranks == {1, 3, 16, 128} and {c[0] for c, r in DR.FORMS if r == 128} == {"64x2048", "1280x1280"}
    for (label, kind, out, inn, group), r in DR.FORMS:                    # every exact design stays below 2^24 (asserted inside)
        if out * inn <= 1 << 16:
            DR.exact_design(out, inn, r)


# ------------------------------------------------------------------------------------------------ seeded mistakes
def emulate(x, s, mistake=None):
    """every output in fp32 torch ops, sums in torch's order (matmul, sum): not the kernels' order.  `mistake` seeds one error."""
    W0, A, B, mu, G = x["W0"].float(), x["A"].float(), x["B"].float(), x["mu"].float(), x["G"]
    v = W0 + s * (B @ A)
    n0 = W0.pow(2).sum(1).sqrt()
    n = v.pow(2).sum(1).sqrt()
    if mistake == "wrong axis":
        n = v.pow(2).sum(0).sqrt()                                         # (a square target)
    if mistake == "norm of W0":
        n = n0.clone()
    q = n0 / n
    c = (1 + mu) * q
    out = dict(n0=n0, n=n, W=(c[:, None] * v).to(torch.bfloat16))
    if mistake == "stale norm":                                            # the projection reads the norm an earlier merge (other factors) left
        n_old = (W0 + s * (x["B_old"].float() @ A)).pow(2).sum(1).sqrt()
        q = n0 / n_old
        c = (1 + mu) * q
    out["mu"] = (G * v).sum(1) * (1.0 if mistake == "dmu without q" else q)
    out["B"] = c[:, None] * (s * (G @ A.t()))
    out["A"] = s * (((c[:, None] if mistake != "c on dB only" else 1.0) * B).t() @ G)
    if mistake == "norm not detached":
        Ar, Br, mr = (t.clone().requires_grad_(True) for t in (A, B, mu))
        V = W0 + s * (Br @ Ar)
        W = ((1 + mr) * n0 / V.pow(2).sum(1).sqrt())[:, None] * V
        (W * G).sum().backward()
        out.update(mu=mr.grad, B=Br.grad, A=Ar.grad)
    return out


def failing(x, s, got):
    """the outputs outside their bound"""
    ref, pro, delta = DR.ref64(x["W0"], x["A"], x["B"], x["mu"], s), DR.project64(x["G"], x["W0"], x["A"], x["B"], x["mu"], s), \
        DR.bounds(x["W0"], x["A"], x["B"], x["mu"], s, x["G"])
    bad = set()
    for name, r in (("n0", ref["n0"]), ("n", ref["n"]), ("mu", pro["mu"]), ("B", pro["B"]), ("A", pro["A"])):
        if not bool(((got[name].double() - r).abs() <= delta[name]).all()):
            bad.add(name)
    lo, hi = DR.bf16_interval(ref["W"], delta["W"])
    if not bool(((lo.float() <= got["W"].float()) & (got["W"].float() <= hi.float())).all()):
        bad.add("W")
    return bad


MISTAKES = [("wrong axis", "n"), ("norm of W0", "n"), ("norm not detached", "B"), ("c on dB only", "A"), ("dmu without q", "mu"), ("stale norm", "B")]


@pytest.mark.parametrize("rank", [1, 3, 16])
def test_six_seeded_mistakes_each_fail_at_their_output_after_the_emulation_passes(rank):
    o = i = 24
    g = torch.Generator().manual_seed(rank)
    r = lambda *s: torch.randn(*s, generator=g)
    x = dict(W0=bf(r(o, i)), A=bf(r(rank, i)), B=bf(r(o, rank) * 0.3), mu=bf(r(o) * 0.1), G=r(o, i), B_old=bf(r(o, rank) * 0.3))
    s = 0.37
    assert failing(x, s, emulate(x, s)) == set()                            # another summation order: still inside every bound
    for mistake, where in MISTAKES:
        bad = failing(x, s, emulate(x, s, mistake))
        assert where in bad, (mistake, bad)
    assert "B" not in failing(x, s, emulate(x, s, "c on dB only")) and "A" not in failing(x, s, emulate(x, s, "dmu without q"))
    assert failing(x, s, emulate(x, s, "dmu without q")) == {"mu"}
