"""Frozen-aware backward, the parts that need no GPU: the `lora_backward` key, the flag vectors its modes derive for the tiny UNet's
names, the C boundary of SDXL_DTYPE_GRAD_SELECT (no new function, the struct mirror, the argument errors that are reachable without a
device), the a-priori bound of the direct adapter gradients against a torch emulation of the kernels' arithmetic, and hipcc's resource
report of csrc/lora_grad.hip."""
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
from oracle import unet_ref as U
from sdxl_amd import lib
from sdxl_amd import unet as NU

ROOT = Path(__file__).resolve().parent.parent
CFG = importlib.import_module("sdxl-training-improvements_amd.config")
T = importlib.import_module("sdxl-training-improvements_amd.trainer")
LORA = importlib.import_module("sdxl-training-improvements_amd.lora")

bf = lambda t: t.to(torch.bfloat16)
SHAPES = {k: tuple(int(x) for x in v) for k, v in U.param_shapes(U.tiny_config()).items()}
BLOCK = "down_blocks.1.attentions.0.transformer_blocks.0"


class StandInNet:
    """the tiny UNet's parameter table on the CPU with a recording set_trainable: what LoRAAdapters and the trainer ask of a net"""
    device = "cpu"
    L = None
    h = None

    def __init__(self):
        self.shapes = dict(SHAPES)
        self.ranges, cur = {}, 0
        for k, s in self.shapes.items():
            n = 1
            for x in s:
                n *= x
            self.ranges[k] = (cur, n)
            cur = (cur + n + 63) // 64 * 64
        self.param_elems = cur
        self.weights = bf(torch.randn(cur, generator=torch.Generator().manual_seed(1)) * 0.05)
        self.grads = torch.zeros(cur)
        self.selections = []

    def param_shapes(self):
        return dict(self.shapes)

    def param_ranges(self):
        return dict(self.ranges)

    def zero_grads(self):
        pass

    def forward_loss(self, *a, **k):
        pass

    def backward(self, *a, **k):
        pass

    def read_loss(self):
        return [0.0] * 8

    def set_trainable(self, names=None, lora=None):
        self.selections.append((None if names is None else list(names), lora))


def _trainer(net, **training):
    cfg = CFG.Config()
    for k, v in training.items():
        setattr(cfg.training, k, v)
    return T.create_trainer(SimpleNamespace(unet=net), config=cfg, device="cpu")


# ------------------------------------------------------------------------------------------------ the key
def test_lora_backward_key_is_validated_when_the_trainer_is_built():
    assert CFG.TrainingConfig().lora_backward == "project" and LORA.LORA_BACKWARDS == ("project", "project_frozen", "direct")
    for bad in ("frozen", "Direct", "", None, 1):
        with pytest.raises(ValueError, match="lora_backward"):
            _trainer(StandInNet(), lora_rank=4, lora_backward=bad)
    net = StandInNet()
    tr = _trainer(net, lora_rank=4)
    assert tr.lora_backward == "project" and net.selections == []          # the default never touches the selection
    net = StandInNet()
    tr = _trainer(net, lora_rank=4, lora_backward="project")
    assert net.selections == []
    net = StandInNet()
    tr = _trainer(net, lora_rank=4, lora_backward="project_frozen")
    assert len(net.selections) == 1 and net.selections[0][1] is None
    assert net.selections[0][0] == LORA.trainable_for("project_frozen", tr.lora.targets, SHAPES)
    net = StandInNet()
    tr = _trainer(net, lora_rank=4, lora_alpha=8.0, lora_backward="direct")
    names, op = net.selections[0]
    assert names == [] and isinstance(op, lib.LoraOp) and op.rank == 4 and op.scale == 2.0 and op.n == len(tr.lora.targets)
    assert op.adapters == tr.lora.weights.data_ptr() and op.adapter_grads == tr.lora.grads.data_ptr()


def test_direct_mode_projects_nothing_and_only_all_reduces():
    net = StandInNet()
    tr = _trainer(net, lora_rank=4, lora_backward="direct")
    tr.lora.project = lambda: pytest.fail("direct mode must not project")
    tr._projected = False
    tr._project()
    assert tr._projected
    net = StandInNet()
    tr = _trainer(net, lora_rank=4, lora_backward="project_frozen")
    calls = []
    tr.lora.project = lambda: calls.append("project")
    tr._projected = False
    tr._project()
    assert calls == ["project"]


# ------------------------------------------------------------------------------------------------ the flag vectors
def test_ops_of_the_state_dict_tensors():
    op = lambda k: LORA.op_of(k, SHAPES[k])
    assert op(f"{BLOCK}.attn1.to_q.weight") == op(f"{BLOCK}.attn1.to_k.weight") == op(f"{BLOCK}.attn1.to_v.weight")
    assert op(f"{BLOCK}.attn1.to_out.0.weight") == op(f"{BLOCK}.attn1.to_out.0.bias") != op(f"{BLOCK}.attn1.to_q.weight")
    assert op(f"{BLOCK}.attn2.to_q.weight") not in (op(f"{BLOCK}.attn2.to_k.weight"), op(f"{BLOCK}.attn1.to_q.weight"))
    other = "up_blocks.1.attentions.2.transformer_blocks.0"          # the same width: one grouped K | V weight
    wide = "mid_block.attentions.0.transformer_blocks.1"             # another width: another group
    assert op(f"{BLOCK}.attn2.to_k.weight") == op(f"{BLOCK}.attn2.to_v.weight") == op(f"{other}.attn2.to_k.weight") != op(f"{wide}.attn2.to_k.weight")
    assert op(f"{other}.attn1.to_q.weight") != op(f"{BLOCK}.attn1.to_q.weight")
    tp = [k for k in SHAPES if ".time_emb_proj." in k]
    assert len({op(k) for k in tp}) == 1 and len(tp) == 2 * 17
    assert op("conv_in.weight") == op("conv_in.bias") and op("conv_norm_out.weight") == op("conv_norm_out.bias") != op("conv_out.weight")


def test_flag_vectors_of_the_modes():
    names = list(SHAPES)
    # fused q | k | v with to_k left out of the targets: the op holds a target, so to_k is flagged too (it gets its true gradient)
    targets = LORA.resolve_targets(SHAPES, ["attn1.to_q", "attn1.to_v", "to_out.0"])
    want = LORA.trainable_for("project_frozen", targets, SHAPES)
    flags = NU.trainable_flags(names, want)
    on = {k for k, f in zip(names, flags) if f}
    assert set(targets) <= on and f"{BLOCK}.attn1.to_k.weight" in on and f"{BLOCK}.attn1.to_out.0.bias" in on
    assert f"{BLOCK}.attn2.to_k.weight" not in on and f"{BLOCK}.attn2.to_q.weight" not in on and f"{BLOCK}.attn2.to_out.0.bias" in on
    assert not any(k in on for k in names if ".norm" in k or ".conv" in k or ".ff." in k or "time_emb" in k or "proj_in" in k)
    # the grouped K | V op: one target in one block turns on every block's K | V of that width, and nothing of the other width
    one = [f"{BLOCK}.attn2.to_k.weight"]
    on = set(LORA.trainable_for("project_frozen", one, SHAPES))
    same = [k for k in names if (".attn2.to_k." in k or ".attn2.to_v." in k) and SHAPES[k][0] == SHAPES[one[0]][0]]
    assert on == set(same) and len(same) == 2 * 5 and not any(k.startswith("mid_block") for k in on)
    # direct: everything frozen; project: no selection at all
    assert LORA.trainable_for("direct", targets, SHAPES) == [] and NU.trainable_flags(names, []) == [0] * len(names)
    assert LORA.trainable_for("project", targets, SHAPES) is None
    with pytest.raises(ValueError, match="lora_backward"):
        LORA.trainable_for("both", targets, SHAPES)
    # names, a predicate, an unknown name
    assert NU.trainable_flags(names, lambda k: k.endswith(".bias")) == [int(k.endswith(".bias")) for k in names]
    with pytest.raises(KeyError, match="no.such"):
        NU.trainable_flags(names, ["no.such.weight"])


# ------------------------------------------------------------------------------------------------ the C boundary
def test_boundary_has_no_new_function_and_the_struct_mirror_has_the_headers_size(tmp_path):
    text = (ROOT / "include" / "sdxlstep.h").read_text()
    declared = set(re.findall(r"\b(sdxl_[a-z0-9_]+)\s*\(", text))
    assert len(declared) <= 58 and not any("select" in n for n in declared)
    assert "#define SDXL_DTYPE_GRAD_SELECT 3" in text and lib.DTYPE_GRAD_SELECT == 3
    assert "sdxl_op_lora_grad" in lib.TEST_HOOK_SIGNATURES
    cc = next((c for c in (shutil.which("cc"), shutil.which("gcc"), shutil.which("clang"), "/opt/rocm/lib/llvm/bin/clang") if c and Path(c).exists()), None)
    assert cc is not None, "no C compiler"
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "sdxlstep.h"\nint main(void) {\n'
                   '  printf("%zu %zu %zu\\n", sizeof(sdxl_grad_select), offsetof(sdxl_grad_select, trainable), offsetof(sdxl_grad_select, lora));\n  return 0;\n}\n')
    subprocess.run([cc, "-I", str(ROOT / "include"), str(src), "-o", str(tmp_path / "sizes")], check=True, capture_output=True)
    out = subprocess.run([str(tmp_path / "sizes")], check=True, capture_output=True, text=True).stdout.split()
    G = lib.GradSelect
    assert [int(x) for x in out] == [C.sizeof(G), G.trainable.offset, G.lora.offset]
    assert [f[0] for f in G._fields_] == ["n", "trainable", "lora"]


def test_argument_errors_reachable_without_a_device():
    L = lib.load()
    flags = (C.c_ubyte * 4)(1, 1, 1, 1)
    sel = lib.GradSelect(4, flags, None)
    # a non-NULL name is refused before the handle is looked at; then the handle
    assert L.sdxl_export_grad(None, b"conv_in.weight", C.byref(sel), lib.DTYPE_GRAD_SELECT, None) == 1 and b"NULL" in L.sdxl_last_error()
    assert L.sdxl_export_grad(None, None, C.byref(sel), lib.DTYPE_GRAD_SELECT, None) == 1 and b"null handle" in L.sdxl_last_error()
    assert L.sdxl_export_grad(None, None, None, lib.DTYPE_GRAD_SELECT, None) == 1 and b"null handle" in L.sdxl_last_error()
    # the hook: shape and pointer errors before anything is allocated or launched
    buf = (C.c_char * 4096)()
    p = C.c_void_p((C.addressof(buf) + 15) & ~15)
    odd = C.c_void_p(p.value + 2)
    hook = lambda x, ldx, dy, ldy, A, B, dA, dB, M, out, inn, rank, s=1.0: L.sdxl_op_lora_grad(x, ldx, dy, ldy, A, B, dA, dB, M, out, inn, rank, s, 0, None)
    for (M, out, inn, rank), msg in (((8, 8, 8, 0), b"rank"), ((8, 8, 8, 129), b"rank"), ((8, 8, 12, 4), b"multiple of 8"), ((0, 8, 8, 4), b"M = 0")):
        assert hook(p, inn, p, out, p, p, p, p, M, out, inn, rank) == 1 and msg in L.sdxl_last_error(), (M, out, inn, rank, L.sdxl_last_error())
    assert hook(p, 4, p, 8, p, p, p, p, 8, 8, 8, 4) == 1 and b"ldx" in L.sdxl_last_error()
    assert hook(p, 8, p, 4, p, p, p, p, 8, 8, 8, 4) == 1 and b"ldy" in L.sdxl_last_error()
    assert hook(p, 8, p, 8, odd, p, p, p, 8, 8, 8, 4) == 1 and b"aligned" in L.sdxl_last_error()
    assert hook(None, 8, p, 8, p, p, p, p, 8, 8, 8, 4) == 1
    assert hook(p, 8, p, 8, p, p, p, p, 8, 8, 8, 4, float("inf")) == 1 and b"finite" in L.sdxl_last_error()


# ------------------------------------------------------------------------------------------------ the bound of the GPU test
OP_SHAPES = [(154, 128, 128, 4), (512, 64, 64, 16), (2, 64, 288, 4), (300, 40, 72, 3), (1024, 256, 128, 128)]      # (M, out, in, rank)


@pytest.mark.parametrize("M,out,inn,rank", OP_SHAPES, ids=[f"{m}x{o}x{i}r{r}" for m, o, i, r in OP_SHAPES])
def test_emulated_arithmetic_stays_inside_the_a_priori_bound(M, out, inn, rank):
    """The arithmetic csrc/lora_grad.hip is built for, in torch: T = X A^T and U = dY B accumulated in fp32 and rounded ONCE to bf16, the
    second products accumulated in fp32 over row chunks of 512 that are then added in order, the scale applied last in fp32.  Against the
    float64 evaluation it must stay inside s (2^-8 + M 2^-23) |dY|^T |T| (and the same with |U|^T |X|): the bound tests/test_gpu_grad_select.py
    holds the kernels to."""
    g = torch.Generator().manual_seed(1000 + 13 * M + 7 * out + inn + rank)
    r = lambda *s: bf(torch.randn(*s, generator=g))
    X, dY, A, B = r(M, inn), r(M, out), r(rank, inn), r(out, rank)
    s = 0.37
    Tb, Ub = bf(X.float() @ A.float().T).float(), bf(dY.float() @ B.float()).float()
    dB = torch.zeros(out, rank)
    dA = torch.zeros(rank, inn)
    for m0 in range(0, M, 512):
        dB = dB + dY[m0: m0 + 512].float().T @ Tb[m0: m0 + 512]
        dA = dA + Ub[m0: m0 + 512].T @ X[m0: m0 + 512].float()
    dA, dB = torch.tensor(s) * dA, torch.tensor(s) * dB
    X, dY, A, B = (t.double() for t in (X, dY, A, B))
    That, Uhat = X @ A.T, dY @ B
    e = 2.0 ** -8 + M * 2.0 ** -23
    for name, got, ref, bound in (("dB", dB, s * dY.T @ That, s * e * dY.abs().T @ That.abs()), ("dA", dA, s * Uhat.T @ X, s * e * Uhat.abs().T @ X.abs())):
        ratio = float(((got.double() - ref).abs() / bound.clamp_min(1e-300)).max())
        print(f"[lora_grad] emulation {M}x{out}x{inn} r{rank} {name}: max |err| / bound {ratio:.3f}")
        assert ratio <= 1.0, (name, ratio)


# ------------------------------------------------------------------------------------------------ the kernels' resources
def test_lora_grad_kernels_use_no_scratch(tmp_path):
    """hipcc's resource report of csrc/lora_grad.hip for gfx950: ScratchSize 0 and 0 spilled VGPRs for every kernel (the four rank-block
    instantiations of the T | U and the partial-block kernel, and the reduce); cross-compiles without a GPU"""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    src = ROOT / "sdxl-training-improvements_amd" / "csrc" / "lora_grad.hip"
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wno-pass-failed", "-Rpass-analysis=kernel-resource-usage",
                        "-c", str(src), "-o", str(tmp_path / "lora_grad.o")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    names = re.findall(r"Function Name: (\S+)", r.stderr)
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stderr)]
    spills = [int(x) for x in re.findall(r"VGPRs Spill: (\d+)", r.stderr)]
    assert len([n for n in names if "lora_tu_kernel" in n]) == 4 and len([n for n in names if "lora_part_kernel" in n]) == 4, names
    assert any("lora_red_kernel" in n for n in names)
    assert len(scratch) == len(names) and len(spills) == len(names)
    assert all(x == 0 for x in scratch) and all(x == 0 for x in spills), (names, scratch, spills)
