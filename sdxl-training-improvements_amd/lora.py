"""LoRA by merge and project: adapters on a frozen UNet without touching the engine, the plan or any existing kernel.

For a targeted weight W [out, in] with adapters A [r, in], B [out, r] and s = alpha / r (the reference's `LoRAModuleWrapper`,
src/models/adapters/lora.py: base(x) + alpha * up(down(x)), up = B, down = A):

  merge    before the forward the weight arena holds W = bf16(W0 + s B A), W0 a frozen bf16 copy of the checkpoint's weight;
  backward the existing forward and backward run unchanged and leave dW = dL/dW in the fp32 gradient arena;
  project  dA = s B^T dW, dB = s dW A^T: exactly the LoRA gradients at the merged weight.

Both steps are one call into libsdxlstep (csrc/lora.hip through dtype SDXL_DTYPE_LORA of sdxl_load_weight / sdxl_export_grad).
training.lora_target_kinds (LORA_TARGET_KINDS) says which tensors may be targets: "plain" = 2-D linears stored as plain rows; "all" = every
2-D or 4-D weight but conv_in -- also ff.net.0.proj and the convolutions, which the arena keeps in packed layouts -- through dtype
SDXL_DTYPE_LORA_LAYOUTS.  There out = shape[0], in = prod(shape[1:]) and A, B are indexed like the state-dict tensor flattened to [out, in].
LoRAAdapters owns the small arenas and looks to a fused optimizer like a net (weights, grads, L, zero_grads, param_ranges, param_shapes), so
AdamWBF16 / AdamWScheduleFreeKahanBF16 update it unchanged.  target_factors says which factors a target of each family has, FAMILIES
the rest that differs between the families; the layout, the ranges, the views, the initialisation and the export all follow from the two.  NativeLoRATrainer is the trainer `training.lora_rank > 0` selects.
training.lora_backward chooses how much of the full model's backward runs for that (LORA_BACKWARDS):
  "project"         all of it, as above (the default);
  "project_frozen"  the engine's gradient selection (NativeUNet.set_trainable) keeps only the ops that hold a target: every other op
                    skips its weight / bias / norm-parameter gradient work; dW of the targets' ops is formed and projected as before;
  "direct"          every tensor is frozen and the targets' ops write dA = s (dY B)^T X, dB = s dY^T (X A^T) themselves
                    (csrc/lora_grad.hip): no dW anywhere, no projection pass.

training.lora_algo (LORA_ALGOS) chooses the adapter family.  "loha" is LyCORIS' Hadamard product: four factors per target,
  dW = s (B1 A1) .* (B2 A2),   A1, A2 [r, in], B1, B2 [out, r]   (LyCORIS: hada_w1_a = B1, hada_w1_b = A1, hada_w2_a = B2, hada_w2_b = A2)
merged and projected the same way through dtype SDXL_DTYPE_LOHA (csrc/loha.hip): effective rank up to r^2 at the storage of rank 2 r, so
the rank is capped at 64.  Its gradients are two projections of dW .* P with the other pair's product P recomputed on the fly; "direct" is
LoRA's only.  Initialisation (this build's choice; LyCORIS was not at hand to compare with): B2 = 0, so dW = 0 and the first merged step
has the plain trainer's bits; A1, A2 ~ N(0, 1), B1 ~ N(0, 0.1^2) from lora_seed.

"kronecker" is LyCORIS' LoKr (the value is NOT "lokr": tests/test_host_loha.py pins that string as an unknown algorithm): with
(out_l, out_k) = lokr_fact(out, factor), (in_m, in_n) = lokr_fact(cin, factor), cin = shape[1], n2 = in_n kh kw,
  dW = s kron(C, W2),   C [out_l, in_m] (lokr_w1),   W2 [out_k, n2] stored in full (lokr_w2) or W2 = B A, B [out_k, r] (lokr_w2_a), A [r, n2] (lokr_w2_b)
through dtype SDXL_DTYPE_LOKR (csrc/lokr.hip).  training.lokr_factor (-1 or >= 1) is the factor; a target is full when training.lokr_full
is true or 2 r >= max(out_k, in_n) (LyCORIS' rule with decompose_both off), with s = 1 and an exported alpha of r; a factored one has
s = alpha / r.  lora_rank is 1 .. 128.  Initialisation (this build's choice): the zero factor is W2 (full) or A (factored), as in LyCORIS,
so dW = 0 and the first merged step has the plain trainer's bits; C ~ N(0, 1), B ~ N(0, 0.1^2) from lora_seed.

"dora" is DoRA (Liu et al. 2024; PEFT's use_dora): LoRA's A and B plus a trained vector mu [out] per target, through dtype SDXL_DTYPE_DORA
(csrc/dora.hip).  With V = W0 + s B A, n_o the fp32 norm of row o of V and n0_o that of W0 (computed once on the device, frozen),
  W[o] = (1 + mu_o) (n0_o / n_o) V[o]      that is DoRA's m_o V[o] / ||V[o]|| with the magnitude m_o = n0_o (1 + mu_o).
mu (not m) is what the bf16 arena holds: bf16(n0_o) != n0_o, so a stored m would move a fresh adapter's weights by an ulp, while mu = 0
and B = 0 (the initialisation; A as LoRA's) give back W0's bits and the first merged step has the plain trainer's.  The backward holds n_o
constant (the paper's section 4.3, PEFT's .detach()): dA, dB are LoRA's times c_o = (1 + mu_o) n0_o / n_o and dmu_o = (n0_o / n_o) <dW[o], V[o]>.
This build's choices: weight decay acts on mu, so it pulls m towards n0, not towards 0; a row with n0_o = 0 stays 0 whatever mu is.
lora_backward "project" or "project_frozen"; lora_rank 1 .. 128.
"""
from __future__ import annotations

import ctypes as C
import json
import logging
from pathlib import Path
from typing import Any, Callable, Dict, List, NamedTuple, Optional, Sequence, Tuple

import torch

from . import distributed as D
from . import lib
from .optimizer import FusedArenaOptimizer, _pad8
from .trainer import NativeSDXLTrainer, build_optimizer, checkpoint_dir

logger = logging.getLogger(__name__)

DEFAULT_TARGETS = ("to_q", "to_k", "to_v", "to_out.0")
MAX_RANK = 128
LORA_BACKWARDS = ("project", "project_frozen", "direct")
LORA_TARGET_KINDS = ("plain", "all")
LORA_ALGOS = ("lora", "loha", "kronecker", "dora")
LOHA_MAX_RANK = 64
LOKR = "kronecker"      # LyCORIS' LoKr ("lokr" stays an unknown value: tests/test_host_loha.py uses it as one)
LOKR_NAMES = {"C": "lokr_w1", "W2": "lokr_w2", "B": "lokr_w2_a", "A": "lokr_w2_b"}      # the LyCORIS names
LOHA_FACTORS = (("A1", "hada_w1_b"), ("B1", "hada_w1_a"), ("A2", "hada_w2_b"), ("B2", "hada_w2_a"))      # arena order; the LyCORIS names


class Family(NamedTuple):
    """what differs between the adapter families besides their factors (target_factors)"""
    dtype: Dict[str, int]                   # lib.DTYPE_* of sdxl_load_weight / sdxl_export_grad by lora_target_kinds (one dtype has the packed
                                            # layouts' target rules in the library; `kinds` still says what the patterns may resolve to)
    max_rank: int
    init: Callable[[int], Tuple[Tuple[str, float], ...]]      # rank -> (factor, std) in draw order; the other factors are 0, so dW = 0
    export: str                             # export_tensors' convention, "peft" or "lycoris"
    file: str                               # save_checkpoint's adapter file
    direct: bool = False                    # lora_backward "direct" writes this family's gradients
    wrap: Callable = lambda ad, op, mode: op      # the struct the two device steps take, around the sdxl_lora_op
    restore_mode: int = 0                   # the `mode` of the merge that restores W0
    meta: Tuple[str, ...] = ()              # the settings (attributes lokr_<name>) a state carries besides LoRA's
    setup: Optional[Callable] = None        # the family's buffers, once the arenas are there


def _every_kind(dtype: int) -> Dict[str, int]:
    return {kinds: dtype for kinds in LORA_TARGET_KINDS}


FAMILIES = {
    # the reference's init: down ~ N(0, (1 / rank)^2), up = 0
    "lora": Family({"plain": lib.DTYPE_LORA, "all": lib.DTYPE_LORA_LAYOUTS}, MAX_RANK, lambda r: (("A", 1.0 / r),), "peft",
                   "pytorch_lora_weights.safetensors", direct=True),
    "loha": Family(_every_kind(lib.DTYPE_LOHA), LOHA_MAX_RANK, lambda r: (("A1", 1.0), ("B1", 0.1), ("A2", 1.0)), "lycoris",
                   "lycoris_loha.safetensors"),
    LOKR: Family(_every_kind(lib.DTYPE_LOKR), MAX_RANK, lambda r: (("C", 1.0), ("B", 0.1)), "lycoris", "lycoris_lokr.safetensors",      # (B: a factored target's)
                 wrap=lambda ad, op, mode: lib.LokrOp(op, ad.lokr_factor, int(ad.lokr_full), ad.scratch.data_ptr(), ad.scratch.numel()),
                 meta=("factor", "full"), setup=lambda ad: ad._setup_lokr()),
    "dora": Family(_every_kind(lib.DTYPE_DORA), MAX_RANK, lambda r: (("A", 1.0 / r),), "peft", "pytorch_lora_weights.safetensors",
                   wrap=lambda ad, op, mode: lib.DoraOp(op, int(mode), ad.norm0.data_ptr(), ad.norm.data_ptr()),
                   restore_mode=lib.DORA_RESTORE, setup=lambda ad: ad._setup_dora()),
}
assert tuple(FAMILIES) == LORA_ALGOS
EXPORT_FILES = {algo: fam.file for algo, fam in FAMILIES.items()}


class Factor(NamedTuple):
    name: str                   # the accessor's: LoRAAdapters.view(name, key)
    leaf: str                   # the param_ranges() key is "<module>." + leaf
    shape: Tuple[int, ...]


def check_lora_algo(algo) -> str:
    if algo not in LORA_ALGOS:
        raise ValueError(f"training.lora_algo {algo!r}: expected one of {list(LORA_ALGOS)}")
    return algo


def check_rank(rank, algo: str = "lora") -> int:
    cap = FAMILIES[check_lora_algo(algo)].max_rank
    if isinstance(rank, bool) or not isinstance(rank, int) or not 1 <= rank <= cap:
        raise ValueError(f"lora_rank must be an integer in 1 .. {cap} (got {rank!r})" + (f" with lora_algo {algo!r}" if cap != MAX_RANK else ""))
    return rank


def check_direct_algo(algo: str) -> None:
    if not FAMILIES[algo].direct:
        raise ValueError(f"training.lora_backward 'direct': the backward writes LoRA's adapter gradients only, not training.lora_algo "
                         f"{algo!r}'s (use 'project' or 'project_frozen')")


def check_lokr_factor(factor) -> int:
    if isinstance(factor, bool) or not isinstance(factor, int) or not (factor == -1 or factor >= 1):
        raise ValueError(f"training.lokr_factor {factor!r}: expected -1 or a positive integer")
    return factor


def check_lokr_full(full) -> bool:
    if not isinstance(full, bool):
        raise ValueError(f"training.lokr_full {full!r}: expected true or false")
    return full


def lokr_fact(dimension: int, factor: int = -1) -> Tuple[int, int]:
    """LyCORIS' factorization(dimension, factor), restated: (m, n), m <= n, m n = dimension.  A positive factor that divides the dimension
    gives (factor, dimension / factor) sorted; otherwise m steps from 1 through the divisors while m + n does not grow and m <= factor
    (factor < 0: no cap)."""
    if factor > 0 and dimension % factor == 0:
        m, n = factor, dimension // factor
        return (m, n) if m <= n else (n, m)
    if factor < 0:
        factor = dimension
    m, n = 1, dimension
    while m < n:
        nm = m + 1
        while dimension % nm:
            nm += 1
        nn = dimension // nm
        if nm + nn > m + n or nm > factor:
            break
        m, n = nm, nn
    return (m, n) if m <= n else (n, m)


def lokr_geometry(shape: Sequence[int], factor: int, rank: int, full: bool) -> Dict[str, int]:
    """out_l, out_k, in_m, in_n, khw, n2, full (0 / 1) of one target: the channel count shape[1] is factorised, not `in`; the form is the
    rule 2 rank >= max(out_k, in_n) unless `full` forces it"""
    out_l, out_k = lokr_fact(int(shape[0]), factor)
    in_m, in_n = lokr_fact(int(shape[1]), factor)
    khw = _prod(shape[2:])
    return dict(out_l=out_l, out_k=out_k, in_m=in_m, in_n=in_n, khw=khw, n2=in_n * khw,
                full=int(bool(full) or 2 * rank >= max(out_k, in_n)))


def lokr_scratch_floats(geos) -> int:
    """sdxl_lokr_op.scratch's size (include/sdxlstep.h): per target the projection's partial sums and a factored target's dW2"""
    pad4 = lambda n: (n + 3) // 4 * 4
    total = 0
    for g in geos:
        w2 = g["out_k"] * g["n2"]
        total += pad4(-(-w2 // lib.LOKR_TILE) * g["out_l"] * g["in_m"]) + (0 if g["full"] else pad4(w2))
    return total


def check_lora_backward(mode) -> str:
    if mode not in LORA_BACKWARDS:
        raise ValueError(f"training.lora_backward {mode!r}: expected one of {list(LORA_BACKWARDS)}")
    return mode


def check_target_kinds(kinds) -> str:
    if kinds not in LORA_TARGET_KINDS:
        raise ValueError(f"training.lora_target_kinds {kinds!r}: expected one of {list(LORA_TARGET_KINDS)}")
    return kinds


def is_plain_target(key: str, shape: Sequence[int]) -> bool:
    """a tensor SDXL_DTYPE_LORA and the direct adapter gradients take: 2-D, stored as plain rows"""
    return len(shape) == 2 and not key[: -len(".weight")].endswith("ff.net.0.proj")


def op_of(key: str, shape: Tuple[int, ...]) -> str:
    """The engine op that owns a state-dict tensor (include/sdxlstep.h, gradient selection), as a label: attn1.to_q | to_k | to_v of a
    block are one fused weight, attn2.to_k | to_v of EVERY block of one width one grouped weight, every time_emb_proj (weights and
    biases) one op; any other module is its own op, weight and bias together."""
    mod, _dot, _leaf = key.rpartition(".")
    head, _dot, name = mod.rpartition(".")
    if head.endswith(".attn1") and name in ("to_q", "to_k", "to_v"):
        return head + ".to_qkv"
    if head.endswith(".attn2") and name in ("to_k", "to_v"):
        return f"attn2.to_kv[{int(shape[0])}]"
    if name == "time_emb_proj":
        return "time_emb_proj"
    return mod


def trainable_for(mode: str, targets: Sequence[str], shapes: Dict[str, Tuple[int, ...]]):
    """the names NativeUNet.set_trainable gets for a lora_backward mode: None (everything: "project"), every tensor of an op that
    holds a target ("project_frozen"), nothing ("direct")"""
    check_lora_backward(mode)
    if mode == "project":
        return None
    if mode == "direct":
        return []
    ops = {op_of(k, shapes[k]) for k in targets}
    return [k for k in shapes if op_of(k, shapes[k]) in ops]


def _pad4(n: int) -> int:
    return (n + 3) // 4 * 4


def resolve_targets(shapes: Dict[str, Tuple[int, ...]], patterns: Sequence[str], kinds: str = "plain") -> List[str]:
    """The `.weight` keys of `shapes` (state-dict order) whose module path is a pattern or ends in "." + pattern.  ValueError for a
    pattern that matches nothing and for one that matches a tensor the kernels cannot take: with kinds "plain" a convolution, the
    row-interleaved `ff.net.0.proj`, or an `in` that is no multiple of 8; with kinds "all" a tensor that is neither 2-D nor 4-D, or an
    `in` = prod(shape[1:]) that is no multiple of 8 (conv_in)."""
    check_target_kinds(kinds)
    patterns = [str(p) for p in patterns]
    if not patterns:
        raise ValueError("lora_targets: no pattern given")
    out, hit = [], {p: 0 for p in patterns}
    for key, shape in shapes.items():
        if not key.endswith(".weight"):
            continue
        mod = key[: -len(".weight")]
        ps = [p for p in patterns if mod == p or mod.endswith("." + p)]
        if not ps:
            continue
        for p in ps:
            hit[p] += 1
        if kinds == "all":
            if len(shape) not in (2, 4):
                raise ValueError(f"lora_targets: pattern {ps[0]!r} matches {key} {tuple(shape)}: only 2-D and 4-D weights can carry an adapter")
            if _prod(shape[1:]) % 8:
                raise ValueError(f"lora_targets: pattern {ps[0]!r} matches {key} {tuple(shape)}: `in` = {_prod(shape[1:])} must be a multiple "
                                 "of 8")
            out.append(key)
            continue
        if len(shape) != 2:
            raise ValueError(f"lora_targets: pattern {ps[0]!r} matches {key} {tuple(shape)}: only 2-D linear weights can carry an adapter")
        if mod.endswith("ff.net.0.proj"):
            raise ValueError(f"lora_targets: pattern {ps[0]!r} matches {key}: ff.net.0.proj is stored row-interleaved (GEGLU) and cannot "
                             "carry an adapter")
        if shape[1] % 8:
            raise ValueError(f"lora_targets: pattern {ps[0]!r} matches {key} {tuple(shape)}: `in` must be a multiple of 8")
        out.append(key)
    missing = [p for p, n in hit.items() if n == 0]
    if missing:
        raise ValueError(f"lora_targets: pattern {missing[0]!r} matches no tensor")
    return out


def _prod(dims) -> int:
    n = 1
    for v in dims:
        n *= int(v)
    return n


def target_factors(algo: str, shape: Sequence[int], rank: int, factor: int = -1, full: bool = False) -> Tuple[Factor, ...]:
    """The factors of one target in arena order, the one place that says which a family has, under what names and of what shape; out =
    shape[0], in = prod(shape[1:]).  `factor`, `full`: training.lokr_factor / lokr_full, read by "kronecker" only."""
    check_lora_algo(algo)
    o, i = int(shape[0]), _prod(shape[1:])
    if algo == "lora":
        return (Factor("A", "lora_A.weight", (rank, i)), Factor("B", "lora_B.weight", (o, rank)))
    if algo == "dora":
        return (Factor("A", "lora_A", (rank, i)), Factor("B", "lora_B", (o, rank)), Factor("mu", "lora_magnitude", (o,)))
    if algo == "loha":
        return tuple(Factor(name, lyco, (rank, i) if name[0] == "A" else (o, rank)) for name, lyco in LOHA_FACTORS)
    g = lokr_geometry(shape, factor, rank, full)
    shapes = {"C": (g["out_l"], g["in_m"]), "W2": (g["out_k"], g["n2"]), "B": (g["out_k"], rank), "A": (rank, g["n2"])}
    return tuple(Factor(name, LOKR_NAMES[name], shapes[name]) for name in (("C", "W2") if g["full"] else ("C", "B", "A")))


def adapter_layout(shapes: Dict[str, Tuple[int, ...]], targets: Sequence[str], rank: int, algo: str = "lora", factor: int = -1,
                   full: bool = False):
    """({key: (*offsets, out, in)}, total elements): per target the element offset of each of target_factors' factors, in that order, every
    factor padded to 8 elements -- (A, B) for "lora", (A1, B1, A2, B2) for "loha", (C, W2) or (C, B, A) for "kronecker", (A, B, mu) for
    "dora"; out = shape[0], in = prod(shape[1:]): the state-dict tensor flattened to two dimensions.  csrc/capi.hip's arena_place is its twin."""
    check_lora_algo(algo)
    lay, cur = {}, 0
    for k in targets:
        offs = []
        for f in target_factors(algo, shapes[k], rank, factor, full):
            offs.append(cur)
            cur += _pad8(_prod(f.shape))
        lay[k] = (*offs, int(shapes[k][0]), _prod(shapes[k][1:]))
    return lay, cur


class LoRAAdapters:
    """The adapters of one net: bf16 arena `.weights`, fp32 `.grads` laid out like it, and the packed bf16 copy of the targets' W0."""

    def __init__(self, net, rank: int, alpha: Optional[float] = None, targets: Optional[Sequence[str]] = None, seed: int = 0,
                 kinds: str = "plain", algo: str = "lora", factor: int = -1, full: bool = False):
        self.kinds = check_target_kinds(kinds)
        self.algo = check_lora_algo(algo)
        self.lokr_factor = check_lokr_factor(factor)      # (read by "kronecker" only)
        self.lokr_full = check_lokr_full(full)
        fam = FAMILIES[algo]
        self.dtype = fam.dtype[kinds]
        self.geometry, self.scratch = {}, None      # ("kronecker" has them: _setup_lokr)
        self.norm0 = self.norm = None               # ("dora": _setup_dora)
        self.net = net
        self.L = getattr(net, "L", None)
        self.rank = check_rank(rank, algo)
        self.alpha = float(rank if alpha is None else alpha)
        self.scale = self.alpha / rank
        self.seed = int(seed)
        shapes = net.param_shapes()
        self.patterns = tuple(DEFAULT_TARGETS if targets is None else targets)
        self.targets = resolve_targets(shapes, self.patterns, kinds)
        self.shapes = {k: tuple(int(v) for v in shapes[k]) for k in self.targets}
        names = list(shapes)
        self.index = [names.index(k) for k in self.targets]
        self.factors = {k: target_factors(algo, self.shapes[k], rank, self.lokr_factor, self.lokr_full) for k in self.targets}
        self.layout, self.param_elems = adapter_layout(shapes, self.targets, rank, algo, self.lokr_factor, self.lokr_full)
        dev = net.weights.device
        self.weights = torch.zeros(self.param_elems, dtype=torch.bfloat16, device=dev)
        self.grads = torch.zeros(self.param_elems, dtype=torch.float32, device=dev)
        ranges = net.param_ranges()
        self.base = torch.cat([net.weights[ranges[k][0]: ranges[k][0] + ranges[k][1]] for k in self.targets])
        assert self.base.numel() == sum(ranges[k][1] for k in self.targets)      # (the targets' native ranges: out * in elements each)
        g = torch.Generator().manual_seed(self.seed)
        for k in self.targets:      # this build's choice for the LyCORIS families (the module docstring): one generator, the table's draw order
            for name, std in fam.init(rank):
                if any(f.name == name for f in self.factors[k]):
                    v = self.view(name, k)
                    v.copy_((torch.randn(*v.shape, generator=g) * std).to(torch.bfloat16))
        self._param = (C.c_int * len(self.index))(*self.index)
        if fam.setup:
            fam.setup(self)

    def _setup_lokr(self) -> None:
        self.geometry = {k: lokr_geometry(self.shapes[k], self.lokr_factor, self.rank, self.lokr_full) for k in self.targets}
        # the projection's scratch (sdxl_lokr_op.scratch), allocated once; its contents never matter
        self.scratch = torch.empty(max(lokr_scratch_floats(self.geometry.values()), 4), dtype=torch.float32, device=self.weights.device)

    def _setup_dora(self) -> None:
        """sdxl_dora_op.norm0 / norm: one float per target row in target order, each target padded to 4; mu = 0"""
        self.norm_offsets, cur = {}, 0
        for k in self.targets:
            self.norm_offsets[k] = cur
            cur += _pad4(self.layout[k][-2])
        self.norm0 = torch.zeros(cur, dtype=torch.float32, device=self.weights.device)
        self.norm = torch.zeros(cur, dtype=torch.float32, device=self.weights.device)
        self.init_norm0()

    # ---- what a fused optimizer asks of its net
    def zero_grads(self) -> None:
        self.grads.zero_()

    def _params(self):
        """(param_ranges() key, element offset, Factor) of every factor, in arena order"""
        for k, lay in self.layout.items():
            for off, f in zip(lay, self.factors[k]):
                yield f"{k[: -len('.weight')]}.{f.leaf}", off, f

    def param_ranges(self) -> Dict[str, Tuple[int, int]]:
        """{"<module>.<leaf>": (element offset, padded element count)} inside the adapter arenas, target_factors' leaves in arena order:
        "lora_A.weight", "lora_B.weight"; algo "loha": "hada_w1_b" (A1), "hada_w1_a" (B1), "hada_w2_b" (A2), "hada_w2_a" (B2);
        algo "kronecker": "lokr_w1" (C), then "lokr_w2" (W2, a full target) or "lokr_w2_a" (B), "lokr_w2_b" (A);
        algo "dora": "lora_A", "lora_B", "lora_magnitude" (mu)"""
        return {name: (off, _pad8(_prod(f.shape))) for name, off, f in self._params()}

    def param_shapes(self) -> Dict[str, Tuple[int, ...]]:
        """the factors' shapes under the keys of param_ranges()"""
        return {name: f.shape for name, _off, f in self._params()}

    # ---- views
    def view(self, name: str, key: str, grad: bool = False) -> torch.Tensor:
        """the factor `name` (target_factors) of a target, or its gradient: a view of the arena.  A "kronecker" target's W2 and A columns
        are j = d kh kw + tap, the state-dict order"""
        names = [f.name for f in self.factors[key]]
        if name not in names:
            form = ("full " if self.geometry[key]["full"] else "factored ") if self.geometry else ""
            raise ValueError(f"{name}: {key} is a {form}lora_algo {self.algo!r} target: it has " + ", ".join(names))
        n = names.index(name)
        shape, off = self.factors[key][n].shape, self.layout[key][n]
        return (self.grads if grad else self.weights)[off: off + _prod(shape)].view(*shape)

    def factor(self, name: str, key: str, grad: bool = False) -> torch.Tensor:
        """a LoHa factor "A1" | "B1" | "A2" | "B2" of a target (or its gradient)"""
        if self.algo != "loha":
            raise ValueError(f"{name}: these adapters are lora_algo {self.algo!r}" + (" (C, W2 or B, A)" if self.geometry else " (A and B)"))
        return self.view(name, key, grad)

    def lokr_factors(self, key: str) -> Tuple[str, ...]:
        """the factors of a "kronecker" target in arena order: ("C", "W2") when it is full, ("C", "B", "A") when it is factored"""
        return tuple(f.name for f in self.factors[key])

    def factor_view(self, name: str, key: str, grad: bool = False) -> torch.Tensor:
        """a LoKr factor "C" | "W2" (full target) | "B" | "A" (factored target) of a target (or its gradient)"""
        if self.algo != LOKR:
            raise ValueError(f"{name}: these adapters are lora_algo {self.algo!r}, not 'kronecker'")
        return self.view(name, key, grad)

    def C(self, key: str, grad: bool = False) -> torch.Tensor:
        return self.factor_view("C", key, grad)

    def W2(self, key: str, grad: bool = False) -> torch.Tensor:
        return self.factor_view("W2", key, grad)

    def target_scale(self, key: str) -> float:
        """s of one target: alpha / rank, or 1 for a full "kronecker" target"""
        return 1.0 if self._full(key) else self.scale

    def _full(self, key: str) -> bool:
        return bool(self.geometry) and bool(self.geometry[key]["full"])

    def A(self, key: str, grad: bool = False) -> torch.Tensor:
        if self.algo == "loha":
            raise ValueError("A: lora_algo 'loha' adapters have A1 and A2")
        return self.view("A", key, grad)

    def B(self, key: str, grad: bool = False) -> torch.Tensor:
        if self.algo == "loha":
            raise ValueError("B: lora_algo 'loha' adapters have B1 and B2")
        return self.view("B", key, grad)

    def mu(self, key: str, grad: bool = False) -> torch.Tensor:
        """the trained vector mu [out] of a "dora" target (or its gradient), a view of the arena: the magnitude is n0 (1 + mu)"""
        if self.algo != "dora":
            raise ValueError(f"mu: these adapters are lora_algo {self.algo!r}, not 'dora'")
        return self.view("mu", key, grad)

    def row_norm(self, key: str, base: bool = True) -> torch.Tensor:
        """the fp32 row norms [out] of a "dora" target, views of the device buffers: n0 of W0 (base=True; written once by init_norm0) or n of
        V = W0 + s B A as the last merge left it"""
        if self.algo != "dora":
            raise ValueError(f"row_norm: these adapters are lora_algo {self.algo!r}, not 'dora'")
        off, o = self.norm_offsets[key], self.layout[key][-2]
        return (self.norm0 if base else self.norm)[off: off + o]

    def magnitude(self, key: str) -> torch.Tensor:
        """DoRA's magnitude m = n0 (1 + mu) [out] of a target, fp32"""
        return self.row_norm(key) * (1.0 + self.mu(key).float())

    def A1(self, key: str, grad: bool = False) -> torch.Tensor:
        return self.factor("A1", key, grad)

    def B1(self, key: str, grad: bool = False) -> torch.Tensor:
        return self.factor("B1", key, grad)

    def A2(self, key: str, grad: bool = False) -> torch.Tensor:
        return self.factor("A2", key, grad)

    def B2(self, key: str, grad: bool = False) -> torch.Tensor:
        return self.factor("B2", key, grad)

    # ---- the two device steps
    def _op(self, scale: float, mode: int = 0):
        op = lib.LoraOp(len(self.index), self._param, self.rank, float(scale), self.weights.data_ptr(), self.base.data_ptr(),
                        self.grads.data_ptr())
        return FAMILIES[self.algo].wrap(self, op, mode)

    def _call(self, fn_name: str, scale: float, mode: int = 0) -> None:
        if self.L is None:
            raise lib.SdxlError(f"LoRAAdapters.{fn_name}: needs libsdxlstep.so (there is no PyTorch fallback)")
        op = self._op(scale, mode)
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        lib.check(getattr(self.L, fn_name)(self.net.h, None, C.byref(op), self.dtype, st), f"{fn_name} (lora)")

    def merge(self, scale: Optional[float] = None) -> None:
        """W = bf16(W0 + s B A) for every target, into the net's weight arena (one launch).  algo "kronecker": `scale` is the factored
        targets' s; a full target uses s = 1 whatever non-zero `scale` is given, and s = 0 with scale 0 (restore).  algo "dora": two
        launches, the first writes the row norms of W0 + s B A into `.norm`, which the next project() reads"""
        self._call("sdxl_load_weight", self.scale if scale is None else scale)

    def restore(self) -> None:
        """the checkpoint's weights back, bit for bit (a merge with scale 0; algo "dora": its restoring mode, mu does not matter)"""
        self._call("sdxl_load_weight", 0.0, FAMILIES[self.algo].restore_mode)

    def init_norm0(self) -> None:
        """algo "dora": the row norms of W0 into `.norm0` (one launch; a no-op without the library, where nothing can be merged either)"""
        if self.L is not None:
            self._call("sdxl_load_weight", 0.0, lib.DORA_INIT)

    def project(self) -> None:
        """dA, dB of every target from the net's fp32 gradient arena into `.grads` (overwritten; two launches).  algo "dora": and dmu, three
        launches, with the row norms the last merge() wrote"""
        self._call("sdxl_export_grad", self.scale)

    def select(self, mode: str) -> None:
        """apply a training.lora_backward mode to the net: its gradient selection and, for "direct", these adapters as the ones whose
        gradients the backward writes into `.grads` (first micro-step: overwritten, later ones: added to).  The arenas' addresses and the
        scale are read now: call again after either changes."""
        if mode == "direct":
            self.check_direct()
        names = trainable_for(mode, self.targets, self.net.param_shapes())
        self.net.set_trainable(names, lora=self._op(self.scale) if mode == "direct" else None)

    def check_direct(self) -> None:
        """ValueError when a target is not one the direct adapter gradients (csrc/lora_grad.hip) take, or the adapters are not LoRA's"""
        check_direct_algo(self.algo)
        bad = [k for k in self.targets if not is_plain_target(k, self.shapes[k])]
        if bad:
            raise ValueError(f"training.lora_backward 'direct': {bad[0]} {self.shapes[bad[0]]} is not a 2-D linear in plain row layout; the "
                             "direct adapter gradients take no convolution and no ff.net.0.proj (use 'project' or 'project_frozen')")

    # ---- state
    def _meta(self) -> Dict[str, Any]:
        meta = {"rank": self.rank, "alpha": self.alpha, "seed": self.seed, "targets": list(self.targets),
                "shapes": [list(self.layout[k][-2:]) for k in self.targets]}
        if self.kinds != "plain":      # (a plain state is what it has always been, byte for byte)
            meta["kinds"] = self.kinds
        if self.algo != "lora":        # (and so is a LoRA state)
            meta["algo"] = self.algo
        for key in FAMILIES[self.algo].meta:      # (and a LoHa state)
            meta[key] = getattr(self, "lokr_" + key)
        return meta

    def state_dict(self) -> Dict[str, Any]:
        return {**self._meta(), "weights": self.weights.detach().cpu().clone()}

    def check_state_dict(self, sd: Dict[str, Any]) -> None:
        mine = self._meta()
        if sd.get("algo", "lora") != self.algo:
            raise ValueError(f"lora state: lora_algo differs from this trainer's ({sd.get('algo', 'lora')!r} vs {self.algo!r})")
        if sd.get("kinds", "plain") != self.kinds:
            raise ValueError(f"lora state: kinds differs from this trainer's ({sd.get('kinds', 'plain')!r} vs {self.kinds!r})")
        for key in ("rank", "targets", "shapes") + FAMILIES[self.algo].meta:
            if sd.get(key) != mine[key]:
                raise ValueError(f"lora state: {key} differs from this trainer's ({_brief(sd.get(key))} vs {_brief(mine[key])})")
        w = sd.get("weights")
        if not (torch.is_tensor(w) and w.dtype == torch.bfloat16 and w.numel() == self.param_elems):
            raise ValueError(f"lora state: the adapter arena must be {self.param_elems} bf16 elements")

    def load_state_dict(self, sd: Dict[str, Any]) -> None:
        """bit-exact; ValueError, with nothing changed, when rank, targets or shapes differ"""
        self.check_state_dict(sd)
        self.alpha = float(sd.get("alpha", self.alpha))
        self.scale = self.alpha / self.rank
        self.weights.copy_(sd["weights"].reshape(-1))
        if self.norm0 is not None:      # (norm0 is not part of a state: it is W0's, recomputed by the kernel that computed it)
            self.init_norm0()

    def export_tensors(self) -> Dict[str, torch.Tensor]:
        """{"unet.<module>.lora_A.weight", "unet.<module>.lora_B.weight"} in fp32 on the CPU, s folded into lora_B: a loader that
        assumes alpha = rank (scale 1) reproduces the delta s B A.  PEFT's shapes: [r, in] / [out, r] for a linear, [r, cin, kh, kw] /
        [out, r, 1, 1] for a convolution (the down convolution has the layer's kernel, the up convolution is 1 x 1).
        algo "loha": the LyCORIS / kohya convention instead -- "lora_unet_<module path with '.' -> '_'>.hada_w1_a" [out, r] (B1), ".hada_w1_b"
        [r, in kh kw] (A1), ".hada_w2_a" (B2), ".hada_w2_b" (A2) and ".alpha" (a scalar), fp32, s NOT folded in: a loader forms
        (alpha / r) (w1_a w1_b) .* (w2_a w2_b) reshaped like the layer's weight.
        algo "dora": LoRA's file plus "unet.<module>.lora_magnitude_vector" [out] fp32, the magnitude m = n0 (1 + mu): a loader forms
        m_o V[o] / ||V[o]||, V = W0 + lora_B lora_A, the norm per output row over every other dimension.
        algo "kronecker": LyCORIS' names under the same prefix -- lokr_w1 [out_l, in_m]; lokr_w2 [out_k, in_n(, kh, kw)] or lokr_w2_a [out_k, r], lokr_w2_b [r, in_n kh kw]; alpha (r for a full target:
        its scale is 1); fp32, s not folded in: a loader forms s kron(w1, w2)."""
        out = {}
        for k in self.targets:
            mod, shape = k[: -len(".weight")], self.shapes[k]
            if FAMILIES[self.algo].export == "lycoris":
                pre = "lora_unet_" + mod.replace(".", "_")
                for f in self.factors[k]:
                    v = self.view(f.name, k).float().cpu().contiguous()
                    if f.name == "W2" and len(shape) == 4:
                        v = v.view(f.shape[0], -1, *shape[2:])
                    out[f"{pre}.{f.leaf}"] = v
                out[f"{pre}.alpha"] = torch.tensor(float(self.rank) if self._full(k) else self.alpha, dtype=torch.float32)
                continue
            for f in self.factors[k]:
                if f.name == "mu":
                    out[f"unet.{mod}.lora_magnitude_vector"] = self.magnitude(k).float().cpu().contiguous()
                    continue
                v = self.view(f.name, k).float().cpu()
                if f.name == "B":
                    v = v * torch.tensor(self.scale, dtype=torch.float32)
                v = v.contiguous()
                if len(shape) == 4:
                    v = v.view(self.rank, *shape[1:]) if f.name == "A" else v.view(shape[0], self.rank, 1, 1)
                out[f"unet.{mod}.lora_{f.name}.weight"] = v
        return out


def _brief(v) -> str:
    s = repr(v)
    return s if len(s) <= 80 else s[:77] + "..."


class _AdapterGradSync:
    """What the base trainer asks of its gradient exchange, for a trainer whose full-size arena is never exchanged: the backward runs
    without exchange and without emit mode (active is False), scaled by 1 / world; the adapter gradients are all-reduced after the
    projection (NativeLoRATrainer._project)."""

    def __init__(self):
        self.world = D.get_world_size()
        self.rank = 0
        self.active = False
        self.enabled = False
        self.comm = None

    def on_segment(self, k, offset, count) -> None:
        pass

    def finish(self) -> None:
        pass

    def reduced(self):
        return None


class NativeLoRATrainer(NativeSDXLTrainer):
    """NativeSDXLTrainer with a frozen UNet and LoRA adapters (training.lora_rank > 0).  Per cycle: the micro-steps' backwards
    accumulate dW in the fp32 arena as ever; optimizer_step() projects, all-reduces the adapter gradients (world > 1), clips on them,
    steps the fused optimizer on the adapter arena and merges.  The weight arena always holds the merged model, so sample / validate /
    evaluate work as they are.  A caller-owned loop may end its cycle with optimizer.step() as with the base trainer: the step projects first."""

    name = "native_mi355x_lora"

    def __init__(self, model, optimizer=None, train_dataloader=None, device=None, wandb_logger=None, config=None, **kwargs):
        tc = config.training if config is not None else None
        self.lora_algo = check_lora_algo(getattr(tc, "lora_algo", "lora"))
        check_rank(getattr(tc, "lora_rank", 0), self.lora_algo)
        if bool(getattr(tc, "use_ema", False)):
            raise ValueError("training.use_ema: an EMA of adapters is not supported (training.lora_rank > 0)")
        if getattr(tc, "shard_optimizer", None):          # None = not given
            raise ValueError("training.shard_optimizer: ZeRO-1 is not supported for adapters (training.lora_rank > 0); leave the key out")
        if optimizer is not None:
            logger.warning("NativeLoRATrainer builds its own fused optimizer on the adapter arena: the optimizer passed in is ignored")
        self.lora_backward = check_lora_backward(getattr(tc, "lora_backward", "project"))
        check_target_kinds(getattr(tc, "lora_target_kinds", "plain"))
        check_lokr_factor(getattr(tc, "lokr_factor", -1))
        check_lokr_full(getattr(tc, "lokr_full", False))
        if self.lora_backward == "direct":
            check_direct_algo(self.lora_algo)
        super().__init__(model, None, train_dataloader, device, wandb_logger, config, **kwargs)
        self._projected = False
        if self.lora_backward != "project":
            self.lora.select(self.lora_backward)
        # whoever steps the optimizer -- optimizer_step() below or a caller-owned loop's optimizer.step() -- steps it on the projected
        # (and exchanged) gradients of the cycle, never on stale ones, and the merge follows the update
        inner = self.optimizer.step

        def step(*a, **k):
            if a[:1] == (None,) or (not a and k.get("grads") is None):      # the adapters' own gradient arena
                self._project()
            return inner(*a, **k)

        self.optimizer.step = step
        self.optimizer.register_step_post_hook(lambda *_a, **_k: self.lora.merge())
        if self.lora.L is not None:
            self.lora.merge()

    # the two builders of the base class: no full-model optimizer arenas, no full-size exchange buffers
    def _build_optimizer(self, optimizer):
        tc = self.config.training
        alpha = getattr(tc, "lora_alpha", None)
        targets = getattr(tc, "lora_targets", None)
        if isinstance(targets, str):
            targets = [targets]
        self.lora = LoRAAdapters(self.net, int(tc.lora_rank), alpha, targets, int(getattr(tc, "lora_seed", 0)),
                                 kinds=getattr(tc, "lora_target_kinds", "plain"), algo=self.lora_algo,
                                 factor=getattr(tc, "lokr_factor", -1), full=getattr(tc, "lokr_full", False))
        if self.lora_backward == "direct":      # (before any arena of the optimizer is built)
            self.lora.check_direct()
        opt = build_optimizer(self.lora, self.config.optimizer)
        assert isinstance(opt, FusedArenaOptimizer)
        return opt

    def _build_grad_sync(self):
        return _AdapterGradSync()

    # ---- the cycle's end
    def _native_backward(self, grad_scale: float) -> None:
        super()._native_backward(grad_scale)
        self._projected = False

    def _project(self) -> None:
        if self._projected:
            return
        if self.lora_backward != "direct":      # ("direct": the backward wrote dA, dB itself)
            self.lora.project()
        if self.sync.world > 1:      # the backward already scaled by 1 / world, and projection is linear
            torch.distributed.all_reduce(self.lora.grads)
        self._projected = True

    def clip_grad_norm_(self, max_norm: float) -> float:
        self._project()
        g = self.lora.grads
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        buf = torch.empty(2, dtype=torch.float32, device=g.device)
        lib.check(self.net.L.sdxl_sumsq(C.c_void_p(g.data_ptr()), 0, g.numel(), C.c_void_p(buf.data_ptr()), st), "sdxl_sumsq")
        lib.check(self.net.L.sdxl_clip_coef(C.c_void_p(buf.data_ptr()), float(max_norm), C.c_void_p(buf.data_ptr() + 4), st),
                  "sdxl_clip_coef")
        self._clip_coef = buf[1:2]
        return float(buf[0].sqrt())

    def optimizer_step(self) -> Optional[float]:
        self._project()
        gn = None
        if self.config.training.clip_grad_norm and self.config.training.clip_grad_norm > 0:
            gn = self.clip_grad_norm_(float(self.config.training.clip_grad_norm))
        self.optimizer.step(None, grad_scale=self._clip_coef)          # (its post hook merges)
        self._clip_coef = None
        self._end_cycle()
        return gn

    # ---- checkpoints
    def sync_to_model(self, ema: bool = False) -> None:
        if ema:
            raise ValueError("sync_to_model(ema=True): the LoRA trainer keeps no EMA")
        super().sync_to_model()

    def save_checkpoint(self, epoch_or_path=0, is_final: bool = False) -> Optional[Path]:
        """`pytorch_lora_weights.safetensors` (fp32, keys unet.<module>.lora_A.weight / .lora_B.weight, s folded into lora_B; with
        training.lora_algo "dora" also unet.<module>.lora_magnitude_vector),
        with training.lora_algo "loha" `lycoris_loha.safetensors`, with "kronecker" `lycoris_lokr.safetensors` instead (export_tensors
        has the keys),
        `lora_state.pt` (the bit-exact arena, settings and target list: load_lora_state), `optimizer.pt`, `config.json`; the merged
        UNet only with training.lora_save_merged.  Rank 0 writes; no collective."""
        if not D.is_main_process():
            return None
        from safetensors.torch import save_file
        d = checkpoint_dir(epoch_or_path, is_final)
        d.mkdir(parents=True, exist_ok=True)
        save_file(self.lora.export_tensors(), str(d / EXPORT_FILES[self.lora.algo]))
        torch.save(self.lora.state_dict(), str(d / "lora_state.pt"))
        with open(d / "config.json", "w") as f:
            json.dump(self.config.to_dict(), f, indent=2)
        torch.save(self._optimizer_state_for_save(), str(d / "optimizer.pt"))
        if bool(getattr(self.config.training, "lora_save_merged", False)):
            self.sync_to_model()
            if self._torch_unet is not None and callable(getattr(self.model, "save_pretrained", None)):
                self.model.save_pretrained(str(d), safe_serialization=True)
            else:
                (d / "unet").mkdir(exist_ok=True)
                save_file({k: v.cpu().contiguous() for k, v in self.net.state_dict().items()},
                          str(d / "unet" / "diffusion_pytorch_model.safetensors"))
        return d

    def load_lora_state(self, checkpoint_dir) -> None:
        """resume from save_checkpoint's directory: the adapter arena bit for bit, optimizer.pt when it is there, then the merge.
        ValueError, with the trainer's state as it was, for a state whose rank, targets or shapes differ."""
        d = Path(checkpoint_dir)
        sd = torch.load(str(d / "lora_state.pt"), map_location="cpu", weights_only=True)
        self.lora.check_state_dict(sd)
        if (d / "optimizer.pt").exists():
            self.load_optimizer_state(d)
        self.lora.load_state_dict(sd)
        if self.lora_backward == "direct":      # (the state's alpha is the scale the backward applies)
            self.lora.select(self.lora_backward)
        self.lora.merge()
