"""The fused optimizers on the packed arenas: host mirrors of the reference optimizer classes, arithmetic in csrc/optimizer.hip.

FusedArenaOptimizer is what the trainer knows: gradients taken from the arena, one fused launch per update (per piece under
ZeRO-1), and the host surface step(grads, grad_scale, zero_grad, pieces), zero_grad, register_step_post_hook, param_groups,
step_count, state_dict / load_state_dict, state_arenas, attach_ema (an ema.WeightEMA updated inside the same launch, on the same
pieces).  Its four algorithms, by optimizer_type (BY_TYPE): AdamWBF16 ("adamw_bf16", the default), AdamWScheduleFreeKahanBF16
("adamw_schedule_free_kahan"), ProdigyBF16 ("prodigy") and AdafactorBF16 ("adafactor"); see the docstrings of the last three.

AdamWBF16:

Reference: src/training/optimizers/adamw_bfloat16/__init__.py (class AdamWBF16, `_make_step`) and stochastic/__init__.py.
Same constructor arguments, `step()`, `zero_grad()`, `state_dict()` / `load_state_dict()`, `param_groups` (a real list
here -- the reference's property returns an iterator).  State is three bf16 arenas (exp_avg, exp_avg_sq,
shift) laid out like the weight arena, so one fused launch updates all 2.567 B parameters; the reference's per-tensor
lazy weight decay (`accumulated_decay`, paid when it exceeds 5e-3, random per-tensor phase) is kept per tensor on the
host and paid with a small per-range kernel on the rare steps it is due.
There is no PyTorch fallback: the step fails loudly without libsdxlstep.so.
"""
from __future__ import annotations

import ctypes as C
import logging
import math
from typing import Any, Dict, List, NamedTuple, Optional, Sequence, Tuple

import torch

from . import lib

logger = logging.getLogger(__name__)


def _ptr(t: Optional[torch.Tensor]):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _checked_ema(ema, weights: torch.Tensor):
    """the kernel writes the EMA arena wherever it updates `weights`: refuse an arena that does not cover them element for element"""
    if ema is None:
        return None
    a = getattr(ema, "arena", None)
    if not (torch.is_tensor(a) and a.dtype == torch.float32 and a.is_contiguous() and a.numel() == weights.numel()
            and a.device == weights.device and getattr(ema, "param_elems", None) == weights.numel()):
        raise ValueError(f"attach_ema: the EMA must hold a contiguous fp32 arena of {weights.numel()} elements on {weights.device}, "
                         f"the weights' size and device; got {type(ema).__name__} with "
                         + (f"{a.dtype} x {a.numel()} on {a.device}" if torch.is_tensor(a) else "no arena"))
    return ema


class FusedArenaOptimizer:
    """What the algorithms share: state arenas laid out like the weight arena (exp_avg, exp_avg_sq, an optional bf16 third one)
    and the skeleton of step().  A subclass names its third arena (THIRD: attribute and state key), the context string of its
    launches (LAUNCH) and its own constructor keywords (CONFIG_KEYS), and has begin_step, finish_step and its state format.
    ZERO1: the update of a sub-range of the arena is the full update's (what ZeRO-1 needs); an algorithm whose step reduces over the
    whole arena says False, takes no `pieces`, and the trainer exchanges its gradients by all-reduce."""

    ZERO1 = True

    def __init__(self, net, group: Dict[str, Any], *, third: bool, grad_round_bf16: bool, moment_dtype=torch.bfloat16, moments: bool = True):
        """group: param_groups[0], already checked (check_hyper and the subclass's own); third: allocate the third arena;
        moment_dtype: of exp_avg and exp_avg_sq; moments False: an algorithm without arena-sized moments -- exp_avg and exp_avg_sq are
        then stride-0 views of one zero (they read as the zero moment of the arena's size and hold 4 bytes each), and the subclass
        says what its launch gets in their place (moment_arenas)"""
        self.net = net
        self.L = getattr(net, "L", None)                      # the loaded libsdxlstep; step() refuses to run without it
        self.param_groups = [group]
        w = net.weights
        assert w.dtype == torch.bfloat16, "only bfloat16 is supported."          # adamw_bfloat16/__init__.py:98
        if moments:
            self.exp_avg = torch.zeros_like(w, dtype=moment_dtype)
            self.exp_avg_sq = torch.zeros_like(w, dtype=moment_dtype)
        else:
            self.exp_avg = torch.zeros(1, dtype=moment_dtype, device=w.device).expand(w.numel())
            self.exp_avg_sq = torch.zeros(1, dtype=moment_dtype, device=w.device).expand(w.numel())
        setattr(self, self.THIRD, torch.zeros_like(w) if third else None)
        self.grad_round_bf16 = bool(grad_round_bf16)
        self.step_count = 0
        self._post_step_hooks = []
        self.ema = None

    @staticmethod
    def check_hyper(betas, eps, weight_decay) -> None:
        if not 0.0 <= eps:
            raise ValueError(f"Invalid epsilon value: {eps}")
        if not 0.0 <= betas[0] < 1.0:
            raise ValueError(f"Invalid beta parameter at index 0: {betas[0]}")
        if not 0.0 <= betas[1] < 1.0:
            raise ValueError(f"Invalid beta parameter at index 1: {betas[1]}")
        if not 0.0 <= weight_decay:
            raise ValueError(f"Invalid weight_decay value: {weight_decay}")

    @classmethod
    def from_config(cls, net, oc):
        """the optimizer for the `optimizer` section of the config (main.py:73-86 builds the reference's from config.optimizer.kwargs);
        CONFIG_KEYS: the subclass's own keywords, {constructor keyword: (config key, default when the section lacks it)}"""
        return cls(net, lr=oc.learning_rate, betas=(oc.beta1, oc.beta2), eps=oc.epsilon, weight_decay=oc.weight_decay,
                   **{kw: getattr(oc, key, default) for kw, (key, default) in cls.CONFIG_KEYS.items()})

    def register_step_post_hook(self, fn) -> None:
        """fn(optimizer) after every step() (same idea as torch.optim.Optimizer.register_step_post_hook)."""
        self._post_step_hooks.append(fn)

    def attach_ema(self, ema) -> None:
        """ema (ema.WeightEMA): from now on every step() also updates its arena, fused into the update (None detaches).  The EMA
        tracks p itself, not p + the third arena.  ValueError when its arena is not an fp32 image of this optimizer's weight arena
        (size, device)."""
        self.ema = _checked_ema(ema, self.net.weights)

    def zero_grad(self, set_to_none: bool = False) -> None:
        self.net.zero_grads()

    def state_arenas(self):
        """the state arenas laid out like the weight arena (what ZeRO-1 gathers before a checkpoint)"""
        third = getattr(self, self.THIRD)
        return (self.exp_avg, self.exp_avg_sq) + ((third,) if third is not None else ())

    def moment_arenas(self):
        """the m and v arguments of the launch"""
        return self.exp_avg, self.exp_avg_sq

    def fill_hyper(self, cfg, grp) -> None:
        """the fields of the config every launch gets from the group"""
        cfg.lr, (cfg.beta1, cfg.beta2), cfg.eps = float(grp["lr"]), grp["betas"], float(grp["eps"])

    def _load_arenas(self, st: Dict[str, Any]) -> None:
        self.step_count = int(st["step"])
        for k, t in zip(("exp_avg", "exp_avg_sq", self.THIRD), self.state_arenas()):
            t.copy_(st[k])

    @torch.no_grad()
    def _step(self, grads, grad_scale, zero_grad, pieces, rand=None) -> None:
        """One update of every parameter.  grads: None = the net's fp32 gradient arena, or a bf16 / fp32 tensor in
        arena layout (the all-reduced bf16 gradients under data parallelism).  grad_scale: optional 1-element device
        tensor multiplied into the gradient inside the kernel (clip coefficient, 1/accumulation).
        pieces (ZeRO-1, distributed.ShardedGradSync.pieces): [(arena offset, count, offset into `grads`)] -- only those
        ranges of the arenas are updated, `grads` then holds just this rank's reduce-scattered shard; every launch is told its
        arena offset (the stochastic-rounding counters are keyed by arena index), so the union over ranks is bit-identical to
        the unsharded update."""
        if self.L is None:
            raise lib.SdxlError(f"{type(self).__name__}.step needs libsdxlstep.so (there is no PyTorch fallback for the optimizer step)")
        grp = self.param_groups[0]
        w = self.net.weights
        g = self.net.grads if grads is None else grads
        if g.dtype not in (torch.float32, torch.bfloat16) or (pieces is None and g.numel() != w.numel()):
            raise ValueError("grads must be an fp32 or bf16 tensor in arena layout")
        if pieces is not None and not self.ZERO1:
            raise ValueError(f"{type(self).__name__}.step takes no pieces: its update reduces over the whole arena")
        cfg = lib.AdamWConfig()
        lib.check(self.L.sdxl_adamw_default_config(C.byref(cfg)))
        self.fill_hyper(cfg, grp)
        cfg.grad_round_bf16 = int(self.grad_round_bf16)
        begun = self.begin_step(cfg, grp)                          # the algorithm's fields and what it books before the launches
        if self.ema is not None:
            cfg.ema_one_minus_decay = self.ema.advance()          # once per step, whatever the number of pieces
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream) if w.is_cuda else None
        gsz = g.element_size()
        todo = [(0, w.numel(), 0)] if pieces is None else list(pieces)
        m, v = self.moment_arenas()
        for off, cnt, goff in todo:
            cfg.elem_offset = off
            cfg.ema = self.ema.arena.data_ptr() + 4 * off if self.ema is not None else None
            at = lambda t, o=off: C.c_void_p(t.data_ptr() + t.element_size() * o) if t is not None else None
            lib.check(self.L.sdxl_adamw_bf16_step(at(w), C.c_void_p(g.data_ptr() + gsz * goff), 0 if g.dtype == torch.float32 else 1,
                                                  at(m), at(v), at(getattr(self, self.THIRD)), cnt,
                                                  C.byref(cfg), _ptr(grad_scale), _ptr(rand), st), self.LAUNCH)
        self.finish_step(begun, todo, st)                         # its remaining launches and bookkeeping
        if zero_grad:
            self.net.zero_grads()
        for fn in self._post_step_hooks:
            fn(self)


class AdamWBF16(FusedArenaOptimizer):
    decay_threshold = 5e-3                                   # adamw_bfloat16/__init__.py:27
    THIRD = "shift"                                          # true value is p + shift (:108-112)
    LAUNCH = "sdxl_adamw_bf16_step"
    CONFIG_KEYS = {"reference_ema": ("reference_ema", True)}

    def __init__(self, net, *, lr=1e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, reference_ema: bool = True,
                 grad_round_bf16: bool = False, seed: int = 0):
        """reference_ema (config key optimizer.reference_ema, default True): True reproduces the reference's ACTUAL first
        moment, m <- SR(g + (1-beta1) * beta1 * m) -- `add_stochastic_(_input, other, alpha)` computes other + alpha*_input
        (stochastic/__init__.py:96), i.e. almost no momentum; False selects the documented EMA
        m <- SR(beta1 * m + (1-beta1) * g)."""
        self.check_hyper(betas, eps, weight_decay)
        super().__init__(net, dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay), third=True,
                         grad_round_bf16=grad_round_bf16)
        self.reference_ema = bool(reference_ema)
        self.seed = int(seed)
        self.ranges = net.param_ranges() if hasattr(net, "param_ranges") else {}
        # each tensor starts its decay account at a random phase so that they do not all pay at once (:116-119)
        g = torch.Generator().manual_seed(self.seed)
        self.accumulated_decay = {k: float(torch.rand([], generator=g) * self.decay_threshold) for k in self.ranges}

    def state_dict(self) -> Dict[str, Any]:
        return {"state": {"step": self.step_count, "exp_avg": self.exp_avg, "exp_avg_sq": self.exp_avg_sq,
                          "shift": self.shift, "accumulated_decay": dict(self.accumulated_decay)},
                "param_groups": self.param_groups}

    def load_state_dict(self, sd: Dict[str, Any]) -> None:
        if sd.get("algorithm", "adamw_bf16") != "adamw_bf16":
            raise ValueError(f"optimizer state of {sd.get('algorithm')!r} cannot be loaded into AdamWBF16")
        self._load_arenas(sd["state"])
        self.accumulated_decay = dict(sd["state"]["accumulated_decay"])
        self.param_groups = sd["param_groups"]

    def step(self, grads: Optional[torch.Tensor] = None, grad_scale: Optional[torch.Tensor] = None,
             zero_grad: bool = False, _rand: Optional[torch.Tensor] = None, pieces=None) -> None:
        """One update of every parameter: arguments as FusedArenaOptimizer._step.  _rand (the parity tests): uint16 [4][n] random
        integers instead of the kernel's counter-based generator."""
        self._step(grads, grad_scale, zero_grad, pieces, _rand)

    def begin_step(self, cfg, grp):
        """counts the step and books each tensor's decay before the launches; returns the tensors whose decay is due"""
        self.step_count += 1
        owed = float(grp["weight_decay"]) * float(grp["lr"])
        due = []
        for k in self.accumulated_decay:                      # :121-126, per tensor
            acc = self.accumulated_decay[k] + owed
            d = acc if acc > self.decay_threshold else 0.0
            self.accumulated_decay[k] = acc - d
            if d > 0:
                due.append((k, d))
        cfg.step = float(self.step_count)
        cfg.decay_this_iteration = 0.0
        cfg.reference_ema = int(self.reference_ema)
        cfg.seed = self.seed
        return due

    def finish_step(self, due, todo, st) -> None:
        for k, d in due:                                       # :191-193 `shift.add_(p, alpha=-decay)`, on the owned part
            toff, tcnt = self.ranges[k]
            for off, cnt, _g in todo:
                lo, hi = max(off, toff), min(off + cnt, toff + tcnt)
                if lo < hi:
                    lib.check(self.L.sdxl_adamw_decay(C.c_void_p(self.shift.data_ptr() + 2 * lo),
                                                      C.c_void_p(self.net.weights.data_ptr() + 2 * lo), hi - lo, d, st), "sdxl_adamw_decay")


class AdamWScheduleFreeKahanBF16(FusedArenaOptimizer):
    """AdamWScheduleFreeKahan on the packed arenas (reference: src/training/optimizers/adamw_schedulefree/__init__.py).

    Host scalars are the reference's python doubles (k = step_count before the increment):
        sched = (k+1)/warmup_steps while k < warmup_steps, else 1;  bc2 = 1 - beta2**(k+1)
        adjusted_lr = lr*sched*sqrt(bc2)   (-> lr_max, get_last_lr());   step_size = adjusted_lr / sqrt(bc2)
    and the element arithmetic runs in one launch over the arena (csrc/optimizer.hip, sfk_kernel) in one of two modes, the
    build-only key optimizer.schedule_free_arithmetic:

    "reference": the reference's bf16 tensor ops bit for bit (pinned to fixtures the reference class produced,
        tests/golden/schedulefree_kahan.npz).  Each op rounds to bf16, and that sequence has defects:
          1. its Kahan term is identically +0 for finite values: rn(b - p) = -rn(p - b), so (p - b) + (b - p) = +0;
          2. updates below half an ulp of the weight are rounded away (at lr 1e-6 almost every weight stays put);
          3. weight decay is not multiplied by lr: p <- p - wd*p per step (1 % per step at the default wd 0.01);
          4. main.py cannot construct the class (OptimizerConfig.kwargs passes correct_bias, which __init__ rejects).
        The reference adds kahan_comp to p.grad in place; here the gradient arena is read, never written (the term is
        +0, so only the sign of a -0 gradient could differ, and nothing reads the gradient afterwards).
    "compensated" (default): what the reference's docstring promises, "Kahan summation for more accurate parameter
        updates when training in low precision".  The true parameter is x = p + c, with c the bf16 compensation kept in
        the kahan_comp arena.  Moments and denominator are computed exactly as in reference mode, then in fp32:
            x = p + c;  x -= (step_size*wd)*x  (decoupled, lr-scaled);  x -= step_size*(m/d);  p = rn(x);  c = rn(x - p)
        Without kahan_sum, c is 0 and is not stored.  This is the default, unlike optimizer.reference_ema, because the
        literal arithmetic does not train a bf16 UNet (defects 2 and 3) and no reference run can produce it (defect 4).

    `correct_bias` is accepted (the reference's config passes it) and ignored: the reference has no such option either.
    The reference never creates its "z" state, so eval() / train() are no-ops there and here.
    No random numbers are involved, so a ZeRO-1 update of `pieces` is bit-identical to the unsharded one by construction.
    There is no PyTorch fallback: the step fails loudly without libsdxlstep.so."""

    ARITHMETIC = ("compensated", "reference")
    algorithm = "adamw_schedule_free_kahan"
    THIRD = "kahan_comp"
    LAUNCH = "sdxl_adamw_bf16_step (schedule-free Kahan)"
    CONFIG_KEYS = {"warmup_steps": ("warmup_steps", 0), "kahan_sum": ("kahan_sum", True),
                   "arithmetic": ("schedule_free_arithmetic", "compensated"), "correct_bias": ("correct_bias", None)}

    def __init__(self, net, *, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, warmup_steps: int = 0,
                 kahan_sum: bool = True, arithmetic: str = "compensated", grad_round_bf16: bool = False, correct_bias=None):
        if not 0.0 <= lr:
            raise ValueError(f"Invalid learning rate: {lr}")
        self.check_hyper(betas, eps, weight_decay)
        if int(warmup_steps) < 0:
            raise ValueError(f"Invalid warmup_steps value: {warmup_steps}")
        arithmetic = str(arithmetic).lower()
        if arithmetic not in self.ARITHMETIC:
            raise ValueError(f"optimizer.schedule_free_arithmetic must be one of {self.ARITHMETIC}, got {arithmetic!r}")
        self.kahan_sum = bool(kahan_sum)
        self.arithmetic = arithmetic
        super().__init__(net, dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay, warmup_steps=int(warmup_steps),
                                   kahan_sum=self.kahan_sum), third=self.kahan_sum, grad_round_bf16=grad_round_bf16)
        self.lr_max = -1.0                                    # (step_count is the reference's self.k)
        self.last_lr = -1.0

    def eval(self) -> None:
        """no-op, as in the reference (its "z" state is never created)"""

    def train(self) -> None:
        """no-op, as in the reference"""

    def get_last_lr(self) -> float:
        return self.last_lr

    def _tag(self) -> Dict[str, Any]:
        return {"algorithm": self.algorithm, "arithmetic": self.arithmetic, "kahan_sum": self.kahan_sum}

    def state_dict(self) -> Dict[str, Any]:
        st = {"step": self.step_count, "exp_avg": self.exp_avg, "exp_avg_sq": self.exp_avg_sq,
              "lr_max": self.lr_max, "last_lr": self.last_lr}
        if self.kahan_sum:
            st["kahan_comp"] = self.kahan_comp
        return {**self._tag(), "state": st, "param_groups": self.param_groups}

    def load_state_dict(self, sd: Dict[str, Any]) -> None:
        got = {k: sd.get(k) for k in self._tag()}
        if got != self._tag():
            raise ValueError(f"optimizer state tagged {got} cannot be loaded into an optimizer configured as {self._tag()}")
        st = sd["state"]
        self._load_arenas(st)
        self.lr_max, self.last_lr = float(st["lr_max"]), float(st["last_lr"])
        self.param_groups = sd["param_groups"]

    def schedule(self):
        """(adjusted_lr, step_size) of the next step, in python doubles exactly as the reference computes them"""
        grp = self.param_groups[0]
        k, lr, beta2, warm = self.step_count, float(grp["lr"]), float(grp["betas"][1]), int(grp.get("warmup_steps", 0))
        sched = (k + 1) / warm if k < warm else 1.0
        bias_correction2 = 1 - beta2 ** (k + 1)
        adjusted_lr = lr * sched * (bias_correction2 ** 0.5)
        return adjusted_lr, adjusted_lr / (bias_correction2 ** 0.5)

    def step(self, grads: Optional[torch.Tensor] = None, grad_scale: Optional[torch.Tensor] = None,
             zero_grad: bool = False, pieces=None) -> None:
        """One update of every parameter: arguments as FusedArenaOptimizer._step."""
        self._step(grads, grad_scale, zero_grad, pieces)

    def begin_step(self, cfg, grp):
        adjusted_lr, step_size = self.schedule()
        self.lr_max = max(adjusted_lr, self.lr_max)
        cfg.step = float(self.step_count + 1)
        cfg.algorithm = 1
        cfg.kahan_sum = int(self.kahan_sum)
        cfg.sf_reference = int(self.arithmetic == "reference")
        cfg.weight_decay = float(grp["weight_decay"])
        cfg.sf_step_size = step_size
        return adjusted_lr

    def finish_step(self, adjusted_lr, todo, st) -> None:
        """counts the step after the launches"""
        self.step_count += 1
        self.last_lr = adjusted_lr


class ProdigyBF16(FusedArenaOptimizer):
    """Prodigy (Mishchenko & Defazio, "Prodigy: An Expeditiously Adaptive Parameter-Free Learner"; the prodigyopt package) on the
    packed arenas: AdamW whose step size d is estimated during training, so `lr` is a multiplier on d and stays at 1.0.

    State: fp32 exp_avg, exp_avg_sq and s, bf16 p0 (the weights at construction) and comp (the true parameter is p + comp), and the
    device block prodigy_state (lib.PRODIGY_STATE_FLOATS floats: d, d_max, num, Bs, d_hat, dlr, A, 0, then the reduction scratch).
    The arithmetic is include/sdxlstep.h's (algorithm 2), three launches per step (csrc/optimizer.hip: accumulate, finalize,
    apply) and no host read-back: d stays on the device; d() reads it and is the only call that synchronises.  Host scalars are
    python doubles: beta3 = sqrt(beta2) unless given; with use_bias_correction the factor of step k (0-based) is
    sqrt(1 - beta2^(k+1)) / (1 - beta1^(k+1)), else 1.  weight_decay is decoupled (x -= wd * dlr * x).

    One d for the whole arena (no per-group d, no slice_p), and one deliberate departure from the package: when every s is zero
    (all-zero gradients) the package skips the parameter update and does not count the step; here the step runs and is counted.
    A step at lr == 0 (a schedule that starts there) launches nothing and is not counted, as in the package.
    The sums run over the whole arena, so there is no ZeRO-1 form (ZERO1 = False): under data parallelism every rank runs the full
    update on the all-reduced gradients.  There is no PyTorch fallback: the step fails loudly without libsdxlstep.so."""

    algorithm = "prodigy"
    ZERO1 = False
    THIRD = "comp"
    LAUNCH = "sdxl_adamw_bf16_step (Prodigy)"
    LOW_LR = 1e-2
    CONFIG_KEYS = {"d0": ("prodigy_d0", 1e-6), "d_coef": ("prodigy_d_coef", 1.0), "growth_rate": ("prodigy_growth_rate", math.inf),
                   "beta3": ("prodigy_beta3", None), "use_bias_correction": ("prodigy_use_bias_correction", False),
                   "safeguard_warmup": ("prodigy_safeguard_warmup", False)}
    SETTINGS = ("d0", "d_coef", "growth_rate", "beta3", "use_bias_correction", "safeguard_warmup")

    def __init__(self, net, *, lr=1.0, betas=(0.9, 0.999), beta3=None, eps=1e-8, weight_decay=0, d0=1e-6, d_coef=1.0,
                 growth_rate=math.inf, use_bias_correction: bool = False, safeguard_warmup: bool = False, grad_round_bf16: bool = False):
        if not 0.0 <= lr:
            raise ValueError(f"Invalid learning rate: {lr}")
        self.check_hyper(betas, eps, weight_decay)
        beta3 = math.sqrt(betas[1]) if beta3 is None else float(beta3)
        if not 0.0 <= beta3 < 1.0:
            raise ValueError(f"Invalid beta3 value: {beta3}")
        if not (0.0 < d0 < math.inf):
            raise ValueError(f"Invalid d0 value: {d0}")
        if not (0.0 < d_coef < math.inf):
            raise ValueError(f"Invalid d_coef value: {d_coef}")
        if not 1.0 <= growth_rate:
            raise ValueError(f"Invalid growth_rate value: {growth_rate}")
        super().__init__(net, dict(lr=lr, betas=tuple(betas), beta3=beta3, eps=eps, weight_decay=weight_decay, d0=float(d0),
                                   d_coef=float(d_coef), growth_rate=float(growth_rate), use_bias_correction=bool(use_bias_correction),
                                   safeguard_warmup=bool(safeguard_warmup)),
                         third=True, grad_round_bf16=grad_round_bf16, moment_dtype=torch.float32)
        w = net.weights
        self.s = torch.zeros_like(w, dtype=torch.float32)
        self.p0 = w.detach().clone()
        self.prodigy_state = torch.zeros(lib.PRODIGY_STATE_FLOATS, dtype=torch.float32, device=w.device)
        self.prodigy_state[:2] = float(d0)

    @classmethod
    def from_config(cls, net, oc):
        if float(oc.learning_rate) < cls.LOW_LR:
            logger.warning("optimizer_type 'prodigy': optimizer.learning_rate %g multiplies the step size d that Prodigy estimates and is "
                           "normally 1.0; a value below %g (the default 1e-6 is AdamW's) all but freezes training", float(oc.learning_rate), cls.LOW_LR)
        return super().from_config(net, oc)

    def d(self) -> float:
        """the current step size estimate (reads the device state back: synchronises)"""
        return float(self.prodigy_state[0])

    def prodigy_bc(self) -> float:
        """the bias-correction factor of the next step, in python doubles"""
        grp = self.param_groups[0]
        if not grp["use_bias_correction"]:
            return 1.0
        k, (beta1, beta2) = self.step_count, grp["betas"]
        return math.sqrt(1 - beta2 ** (k + 1)) / (1 - beta1 ** (k + 1))

    def state_arenas(self):
        return (self.exp_avg, self.exp_avg_sq, self.comp, self.s)

    def _tag(self) -> Dict[str, Any]:
        grp = self.param_groups[0]
        return {"algorithm": self.algorithm, **{k: grp[k] for k in self.SETTINGS}}

    def state_dict(self) -> Dict[str, Any]:
        st = {"step": self.step_count, "exp_avg": self.exp_avg, "exp_avg_sq": self.exp_avg_sq, "comp": self.comp, "s": self.s,
              "p0": self.p0, "prodigy_state": self.prodigy_state[:8].clone()}
        return {**self._tag(), "state": st, "param_groups": self.param_groups}

    def load_state_dict(self, sd: Dict[str, Any]) -> None:
        got = {k: sd.get(k) for k in self._tag()}
        if got != self._tag():
            raise ValueError(f"optimizer state tagged {got} cannot be loaded into an optimizer configured as {self._tag()}")
        st = sd["state"]
        self._load_arenas(st)
        self.s.copy_(st["s"])
        self.p0.copy_(st["p0"])
        self.prodigy_state[:8].copy_(st["prodigy_state"])
        self.param_groups = sd["param_groups"]

    def step(self, grads: Optional[torch.Tensor] = None, grad_scale: Optional[torch.Tensor] = None,
             zero_grad: bool = False, pieces=None) -> None:
        """One update of every parameter: arguments as FusedArenaOptimizer._step, without pieces."""
        self._step(grads, grad_scale, zero_grad, pieces)

    def begin_step(self, cfg, grp):
        cfg.algorithm = 2
        cfg.weight_decay = float(grp["weight_decay"])
        cfg.beta3, cfg.d0, cfg.d_coef, cfg.growth_rate = grp["beta3"], grp["d0"], grp["d_coef"], grp["growth_rate"]
        cfg.prodigy_bc = self.prodigy_bc()
        cfg.safeguard_warmup = int(grp["safeguard_warmup"])
        cfg.p0, cfg.s, cfg.prodigy_state = self.p0.data_ptr(), self.s.data_ptr(), self.prodigy_state.data_ptr()
        return float(grp["lr"]) != 0.0

    def finish_step(self, launched, todo, st) -> None:
        """counts the step after the launches (a step at lr == 0 launched nothing and is not counted)"""
        if launched:
            self.step_count += 1


# ---------------------------------------------------------------------------------------------- Adafactor
class AfEntry(NamedTuple):
    """one tensor of the Adafactor table (sdxl_adafactor_tensor without its state offset): a row-major [rows][cols] matrix at elem_off
    of the arena, numel real elements, factored or not"""
    name: str
    elem_off: int
    rows: int
    cols: int
    numel: int
    factored: bool

    def state_floats(self) -> int:
        """R[rows] then C[cols] rounded up to 4 floats, or v[rows * cols]"""
        return (self.rows + self.cols + 3) // 4 * 4 if self.factored else self.rows * self.cols


def _pad8(n: int) -> int:
    return (int(n) + 7) // 8 * 8


def adafactor_layout(shapes: Dict[str, Sequence[int]], ranges: Dict[str, Tuple[int, int]]) -> List[AfEntry]:
    """Which tensor of an arena Adafactor factors, as a pure function of the state-dict shapes and the arena ranges
    {name: (element offset, element count)}; the entries sorted by offset.
    A 2-D tensor is the matrix [out][in], a 4-D one [shape[0]][prod(rest)] (this project's LoRA convention; in the arena a convolution
    is the plain row-major [cout][9 * cin], and a permutation of the columns changes no statistic; so ff.net.0.proj, whose rows are
    permuted, is a plain matrix too).  It is factored when its range is exactly rows * cols elements and cols is a multiple of 8 (a row
    is whole 16-byte vectors): conv_out is its 4 real rows.  Everything else runs unfactored with numel the real count: a tensor whose
    range holds pads (conv_in: the input channels are padded to 8 inside its range), a matrix with short rows (a LoRA up factor of rank
    4) and every 1-D tensor; its pads hold g = 0 and p = 0 and stay +0.
    The HF class factors a 4-D tensor over its last two dimensions (kh, kw); factoring a 3 x 3 pair saves nothing, so that is
    deliberately not followed.  ValueError when a range does not start on a multiple of 8 or two entries overlap."""
    out = []
    for name, shape in shapes.items():
        off, n = (int(x) for x in ranges[name])
        shape = tuple(int(x) for x in shape)
        real = 1
        for x in shape:
            real *= x
        if real < 1 or n < real:
            raise ValueError(f"adafactor_layout: {name!r} has {real} elements in a range of {n}")
        if off % 8:
            raise ValueError(f"adafactor_layout: {name!r} starts at element {off}, not a multiple of 8")
        rows = shape[0] if len(shape) in (2, 4) else 1
        cols = real // rows
        if len(shape) in (2, 4) and cols % 8 == 0 and n == real:
            out.append(AfEntry(name, off, rows, cols, real, True))
        elif len(shape) in (2, 4) and n % rows == 0 and (n // rows) % 8 == 0:
            out.append(AfEntry(name, off, rows, n // rows, real, False))
        else:
            out.append(AfEntry(name, off, 1, _pad8(n), real, False))
    out.sort(key=lambda e: e.elem_off)
    for a, b in zip(out, out[1:]):
        if a.elem_off + a.rows * a.cols > b.elem_off:
            raise ValueError(f"adafactor_layout: {a.name!r} ([{a.rows}][{a.cols}] at {a.elem_off}) overlaps {b.name!r} at {b.elem_off}")
    return out


def adafactor_scratch_floats(entries: Sequence[AfEntry]) -> int:
    """the floats of af_scratch for a table (include/sdxlstep.h, algorithm 3): 4 per entry, then per entry two floats per tile and, for a
    factored one, the chunk partials of R', the row sums per column block and the column sums per row block"""
    total = 4 * len(entries)
    for e in entries:
        ncb, nrb = -(-e.cols // lib.AF_COLS), -(-e.rows // lib.AF_ROWS)
        total += 2 * nrb * ncb
        if e.factored:
            total += -(-e.rows // 256) + e.rows * ncb + nrb * e.cols
    return total


class AdafactorBF16(FusedArenaOptimizer):
    """Adafactor (Shazeer & Stern, "Adafactor: Adaptive Learning Rates with Sublinear Memory Cost") on the packed arenas, with the
    arguments, defaults, checks and arithmetic of transformers.optimization.Adafactor: the second moment of a weight matrix is one row
    and one column statistic, the update of each tensor is clipped by its own RMS, and with scale_parameter the step size follows the
    RMS of the tensor.  The published SDXL full fine-tune recipe is scale_parameter=False, relative_step=False, lr=4e-7.

    State: af_state (fp32: rows + cols floats per factored tensor, one per element of the others; adafactor_layout says which), the
    bf16 compensation arena comp (the true parameter is p + comp), the fp32 exp_avg only with beta1, and the scratch of the
    reductions.  No arena-sized second moment: about 2 B per element against AdamW_BF16's 6 B.  The arithmetic is
    include/sdxlstep.h's (algorithm 3), five launches per step (csrc/optimizer.hip adafactor_*_kernel), no host read-back.  Host
    scalars are python doubles, k the 1-based step: beta2t = 1 - k**decay_rate; rho = lr, or with relative_step
    min(1e-6 * k if warmup_init else 1e-2, 1 / sqrt(k)).

    relative_step=None (the constructor's default) means "exactly when no lr is given", the two combinations the HF class accepts;
    an explicit relative_step=True with an lr, and warmup_init without relative_step, raise its errors.  One deliberate departure:
    a convolution is factored as [cout][cin*kh*kw], not over (kh, kw) (adafactor_layout).
    The table lists the tensors net.trainable() names (every tensor without a selection): a frozen tensor is not read or written.
    The statistics span whole tensors, so there is no ZeRO-1 form (ZERO1 = False): under data parallelism every rank runs the full
    update on the all-reduced gradients.  There is no PyTorch fallback: the step fails loudly without libsdxlstep.so."""

    algorithm = "adafactor"
    ZERO1 = False
    THIRD = "comp"
    LAUNCH = "sdxl_adamw_bf16_step (Adafactor)"
    SETTINGS = ("eps", "clip_threshold", "decay_rate", "beta1", "scale_parameter", "relative_step", "warmup_init")

    def __init__(self, net, *, lr=None, eps=(1e-30, 1e-3), clip_threshold=1.0, decay_rate=-0.8, beta1=None, weight_decay=0.0,
                 scale_parameter: bool = True, relative_step: Optional[bool] = None, warmup_init: bool = False,
                 grad_round_bf16: bool = False):
        relative_step = (lr is None) if relative_step is None else bool(relative_step)
        if lr is not None and relative_step:
            raise ValueError("Cannot combine manual `lr` and `relative_step=True` options")
        if warmup_init and not relative_step:
            raise ValueError("`warmup_init=True` requires `relative_step=True`")
        if lr is None and not relative_step:
            raise ValueError("relative_step=False needs a learning rate")
        eps = tuple(float(x) for x in eps)
        if len(eps) != 2 or not all(0.0 <= x < math.inf for x in eps):
            raise ValueError(f"Invalid eps pair: {eps}")
        if lr is not None and not 0.0 <= float(lr) < math.inf:
            raise ValueError(f"Invalid learning rate: {lr}")
        if not 0.0 < float(clip_threshold) < math.inf:
            raise ValueError(f"Invalid clip_threshold value: {clip_threshold}")
        if not float(decay_rate) < 0.0:
            raise ValueError(f"Invalid decay_rate value: {decay_rate} (beta2 of step k is 1 - k**decay_rate: it must be negative)")
        if beta1 is not None and not 0.0 <= float(beta1) < 1.0:
            raise ValueError(f"Invalid beta1 value: {beta1}")
        if not 0.0 <= float(weight_decay) < math.inf:
            raise ValueError(f"Invalid weight_decay value: {weight_decay}")
        super().__init__(net, dict(lr=None if lr is None else float(lr), eps=eps, clip_threshold=float(clip_threshold),
                                   decay_rate=float(decay_rate), beta1=None if beta1 is None else float(beta1),
                                   weight_decay=float(weight_decay), scale_parameter=bool(scale_parameter),
                                   relative_step=relative_step, warmup_init=bool(warmup_init)),
                         third=True, grad_round_bf16=grad_round_bf16, moment_dtype=torch.float32, moments=False)
        w = net.weights
        if beta1 is not None:
            self.exp_avg = torch.zeros_like(w, dtype=torch.float32)
        algo = getattr(net, "algo", "lora")                                  # (a lora.LoRAAdapters arena says its family)
        if algo != "lora":
            raise ValueError(f"optimizer_type 'adafactor' is built for lora_algo 'lora' only: the adapter arena of lora_algo {algo!r} has factors "
                             "its table does not describe (train it with adamw_bf16, adamw_schedule_free_kahan or prodigy)")
        if hasattr(net, "param_shapes"):
            shapes, ranges = net.param_shapes(), net.param_ranges()
        else:                                                               # an arena without a tensor table: one unfactored tensor
            shapes, ranges = {"arena": (w.numel(),)}, {"arena": (0, w.numel())}
        self.entries = adafactor_layout(shapes, ranges)
        self.state_offsets, cur = {}, 0
        for e in self.entries:
            self.state_offsets[e.name] = cur
            cur += e.state_floats()
        self.af_state = torch.zeros(max(cur, 4), dtype=torch.float32, device=w.device)
        self.af_scratch = torch.empty(max(adafactor_scratch_floats(self.entries), 4), dtype=torch.float32, device=w.device)
        self._tables: Dict[Any, Any] = {}

    @classmethod
    def from_config(cls, net, oc):
        relative = bool(getattr(oc, "relative_step", True))
        lr = float(oc.learning_rate)
        if relative:
            default = getattr(type(oc), "learning_rate", lr)      # (the section's own default: the key was not written)
            if lr != default:           # a learning rate was written next to relative_step: the HF class's error
                raise ValueError("Cannot combine manual `lr` and `relative_step=True` options (optimizer.learning_rate is set: "
                                 "write relative_step: false, or leave learning_rate out)")
        return cls(net, lr=None if relative else lr, eps=tuple(getattr(oc, "eps", (1e-30, 1e-3))),
                   clip_threshold=getattr(oc, "clip_threshold", 1.0), decay_rate=getattr(oc, "decay_rate", -0.8),
                   beta1=getattr(oc, "adafactor_beta1", None), weight_decay=oc.weight_decay,
                   scale_parameter=getattr(oc, "scale_parameter", True), relative_step=relative,
                   warmup_init=getattr(oc, "warmup_init", False))

    # ---- the table
    def table(self):
        """(entries, ctypes array) of the trainable tensors, built once per selection"""
        live = getattr(self.net, "trainable", None)
        names = None if live is None else frozenset(live())
        if names not in self._tables:
            ents = [e for e in self.entries if names is None or e.name in names]
            arr = (lib.AdafactorTensor * max(len(ents), 1))()
            for a, e in zip(arr, ents):
                a.elem_off, a.rows, a.cols, a.numel, a.factored, a.state_off = e.elem_off, e.rows, e.cols, e.numel, int(e.factored), \
                    self.state_offsets[e.name]
            self._tables = {names: (ents, arr)}
        return self._tables[names]

    def state_floats(self) -> int:
        return sum(e.state_floats() for e in self.entries)

    def schedule(self) -> Tuple[float, float]:
        """(beta2t, rho) of the next step, in python doubles as the HF class computes them"""
        grp = self.param_groups[0]
        k = self.step_count + 1
        beta2t = 1.0 - math.pow(k, grp["decay_rate"])
        rho = grp["lr"]
        if grp["relative_step"]:
            rho = min(1e-6 * k if grp["warmup_init"] else 1e-2, 1.0 / math.sqrt(k))
        return beta2t, float(rho)

    # ---- state
    def moment_arenas(self):
        return (self.exp_avg if self.param_groups[0]["beta1"] is not None else None), None

    def state_arenas(self):
        return (self.comp,) + ((self.exp_avg,) if self.param_groups[0]["beta1"] is not None else ())

    def _tag(self) -> Dict[str, Any]:
        grp = self.param_groups[0]
        return {"algorithm": self.algorithm, **{k: grp[k] for k in self.SETTINGS}}

    def state_dict(self) -> Dict[str, Any]:
        st = {"step": self.step_count, "af_state": self.af_state, "comp": self.comp}
        if self.param_groups[0]["beta1"] is not None:
            st["exp_avg"] = self.exp_avg
        return {**self._tag(), "state": st, "param_groups": self.param_groups}

    def load_state_dict(self, sd: Dict[str, Any]) -> None:
        got = {k: (tuple(sd[k]) if k == "eps" and sd.get(k) is not None else sd.get(k)) for k in self._tag()}
        if got != self._tag():
            raise ValueError(f"optimizer state tagged {got} cannot be loaded into an optimizer configured as {self._tag()}")
        st = sd["state"]
        if st["af_state"].numel() != self.af_state.numel():
            raise ValueError(f"optimizer state holds {st['af_state'].numel()} Adafactor statistics, this arena's layout has {self.af_state.numel()}")
        self.step_count = int(st["step"])
        self.af_state.copy_(st["af_state"])
        self.comp.copy_(st["comp"])
        if self.param_groups[0]["beta1"] is not None:
            self.exp_avg.copy_(st["exp_avg"])
        self.param_groups = sd["param_groups"]

    def step(self, grads: Optional[torch.Tensor] = None, grad_scale: Optional[torch.Tensor] = None,
             zero_grad: bool = False, pieces=None) -> None:
        """One update of every trainable tensor: arguments as FusedArenaOptimizer._step, without pieces."""
        self._step(grads, grad_scale, zero_grad, pieces)

    def fill_hyper(self, cfg, grp) -> None:
        cfg.beta1 = grp["beta1"] if grp["beta1"] is not None else 0.0
        cfg.use_beta1 = int(grp["beta1"] is not None)

    def begin_step(self, cfg, grp):
        ents, arr = self.table()
        cfg.algorithm = 3
        cfg.weight_decay = grp["weight_decay"]
        cfg.eps1, cfg.eps2 = grp["eps"]
        cfg.clip_threshold = grp["clip_threshold"]
        cfg.beta2t, cfg.rho = self.schedule()
        cfg.scale_parameter = int(grp["scale_parameter"])
        cfg.tensors, cfg.n_tensors = C.addressof(arr), len(ents)
        cfg.af_state, cfg.af_scratch = self.af_state.data_ptr(), self.af_scratch.data_ptr()
        return None

    def finish_step(self, _begun, todo, st) -> None:
        """counts the step after the launches"""
        self.step_count += 1

    def tensor_scalars(self) -> Dict[str, Tuple[float, float, float, float]]:
        """{name: (rho_t, eta_t, rms_u, rms_p)} of the last step, read back from the scratch (synchronises)"""
        ents, _arr = self.table()
        vals = self.af_scratch[: 4 * len(ents)].cpu().reshape(-1, 4).tolist()
        return {e.name: tuple(v) for e, v in zip(ents, vals)}


# optimizer_type (lower-cased, as the reference's OptimizerConfig.class_name does) -> the fused class built for it
BY_TYPE = {"adamw_bf16": AdamWBF16, "adamw_schedule_free_kahan": AdamWScheduleFreeKahanBF16, "prodigy": ProdigyBF16,
           "adafactor": AdafactorBF16}
