"""The fused Adafactor update on the GPU (csrc/optimizer.hip adafactor_* kernels): algorithm 3 of sdxl_adamw_bf16_step on caller buffers
against the float64 reference of tests/_adafactor_ref.py, every output within the a-priori bound of that file GIVEN the state the device
held before the step; operand isolation (NaN-filled gaps between the tensors, guard bands around the arenas, the statistics and the
scratch); run-to-run, alone-or-mixed and reordered-table bit equality; and AdafactorBF16 in the full and the LoRA trainer on the tiny
UNet.  Each case prints the largest fraction of its bounds it needed as an `[adafactor]` line (profiles/ops_adafactor.txt keeps them)."""
import ctypes as C
import importlib
import math
from types import SimpleNamespace
from typing import NamedTuple, Optional

import numpy as np
import pytest
import torch

import _adafactor_ref as R
import sdxl_amd  # noqa: F401
from oracle import unet_ref as U
from sdxl_amd import lib
from sdxl_amd import unet as NU
from _isolation import same_bits
from _optim_common import dev, ptr, stream

pytestmark = pytest.mark.gpu

O = importlib.import_module("sdxl-training-improvements_amd.optimizer")
T = importlib.import_module("sdxl-training-improvements_amd.trainer")
CFG = importlib.import_module("sdxl-training-improvements_amd.config")

GUARD = 64                      # elements of guard band on either side of every buffer
EMA_OMD = 0.25
NAN = math.nan


class Spec(NamedTuple):
    key: str
    rows: int
    cols: int
    numel: int
    factored: bool
    zero_row: Optional[int] = None      # a row whose gradient is zero at every step
    zero_all: bool = False              # a tensor whose gradient is zero at every step


def fac(rows, cols, **kw):
    return Spec(f"f{rows}x{cols}", rows, cols, rows * cols, True, **kw)


def unf(cols, numel, **kw):
    return Spec(f"u{cols}n{numel}", 1, cols, numel, False, **kw)


# the two shapes that straddle the tile of the launches by one 8-element vector of columns and one row, each way
STRADDLE = [fac(R.AF_ROWS - 1, R.AF_COLS + 8), fac(R.AF_ROWS + 1, R.AF_COLS - 8)]
SPECS = [unf(8, 5), unf(320, 320), unf(1288, 1281), fac(2, 8), fac(4, 2880), fac(8, 8), fac(37, 72), fac(320, 2560), fac(2, 10240)] + STRADDLE
BY_KEY = {s.key: s for s in SPECS}
RECIPES = {"defaults": dict(beta1=0.9, weight_decay=0.1),                                   # relative steps, scaled by the parameter's RMS
           "sdxl_full_finetune": dict(lr=4e-7, scale_parameter=False, relative_step=False)}


def test_straddle_shapes_follow_the_geometry():
    assert (lib.AF_ROWS, lib.AF_COLS) == (R.AF_ROWS, R.AF_COLS) == (128, 256)
    assert [(s.rows, s.cols) for s in STRADDLE] == [(127, 264), (129, 248)]
    for s, (nrb, ncb) in zip(STRADDLE, ((1, 2), (2, 1))):
        assert (-(-s.rows // lib.AF_ROWS), -(-s.cols // lib.AF_COLS)) == (nrb, ncb)


@pytest.fixture(scope="module")
def L():
    return lib.load()


def data_of(spec: Spec, steps: int, bf16_grads: bool):
    """the tensor's parameters and gradients, a function of the spec alone (not of its place in a table): p ~ 0.05 randn in bf16,
    g ~ s randn with s from the key, pads (past numel) zero"""
    seed = sum(ord(ch) * (i + 1) for i, ch in enumerate(spec.key))
    g0 = torch.Generator().manual_seed(seed)
    span = spec.rows * spec.cols
    live = (torch.arange(span) < spec.numel).float()
    p = ((torch.randn(span, generator=g0) * 0.05) * live).to(torch.bfloat16)
    std = (0.02, 3.0, 40.0)[seed % 3]
    gs = []
    for _k in range(steps):
        g = (torch.randn(span, generator=g0) * std * live).reshape(spec.rows, spec.cols)
        if spec.zero_row is not None:
            g[spec.zero_row] = 0
        if spec.zero_all:
            g.zero_()
        g = g.reshape(-1)
        gs.append(g.to(torch.bfloat16) if bf16_grads else g)
    return p, gs


class Table:
    """specs placed in an arena in the given order with NaN-filled gaps, and everything one call needs"""

    def __init__(self, specs, hp, steps=3, ema=False, bf16_grads=False, scale=None, perm=None):
        self.specs, self.hp, self.steps, self.scale = list(specs), hp, steps, scale
        self.entries, cur, scur = [], 0, 0
        for i, s in enumerate(self.specs):
            e = R.Entry(cur, s.rows, s.cols, s.numel, s.factored, scur)
            self.entries.append(e)
            cur += e.span + (8, 24)[i % 2]
            scur += e.state_floats() + 4
        self.n = cur
        gdt = torch.bfloat16 if bf16_grads else torch.float32
        full = lambda dt, n=self.n: torch.full((GUARD + n + GUARD,), NAN, dtype=dt)
        p, c, m, self.state = full(torch.bfloat16), full(torch.bfloat16), full(torch.float32), full(torch.float32, scur)
        self.scratch = torch.full((GUARD + R.scratch_floats(self.entries) + GUARD,), NAN, dtype=torch.float32, device=dev())
        gs = [full(gdt) for _ in range(steps)]
        emab = full(torch.float32) if ema else None
        self.perm = perm                                    # {key: row permutation}: the rows are stored in that order
        for s, e in zip(self.specs, self.entries):
            pv, gv = data_of(s, steps, bf16_grads)
            rows = slice(None) if perm is None or s.key not in perm else perm[s.key]
            put = lambda buf, v: buf[GUARD + e.elem_off: GUARD + e.elem_off + e.span].copy_(v.reshape(s.rows, s.cols)[rows].reshape(-1))
            put(p, pv)
            put(c, torch.zeros(e.span))
            put(m, torch.zeros(e.span))
            for k in range(steps):
                put(gs[k], gv[k])
            if ema:
                put(emab, pv.float() + 0.01)
            self.state[GUARD + e.state_off: GUARD + e.state_off + e.state_floats()] = 0
        self.p, self.c, self.m, self.state = (t.to(dev()) for t in (p, c, m, self.state))
        self.gs = [g.to(dev()) for g in gs]
        self.ema = None if emab is None else emab.to(dev())
        self.scale_dev = None if scale is None else torch.tensor([scale], dtype=torch.float32, device=dev())
        self.tab = (lib.AdafactorTensor * len(self.entries))()
        for a, e in zip(self.tab, self.entries):
            a.elem_off, a.rows, a.cols, a.numel, a.factored, a.state_off = e.elem_off, e.rows, e.cols, e.numel, int(e.factored), e.state_off
        self.k = 0

    def buffers(self):
        return [self.p, self.c, self.m, self.state, self.scratch] + ([self.ema] if self.ema is not None else [])

    def snapshot(self):
        torch.cuda.synchronize()
        return [t.cpu().clone() for t in self.buffers()]

    def call(self, L):
        hp, k = self.hp, self.k + 1
        cfg = lib.AdamWConfig()
        lib.check(L.sdxl_adamw_default_config(C.byref(cfg)))
        cfg.algorithm, cfg.weight_decay, cfg.grad_round_bf16 = 3, hp.weight_decay, int(hp.grad_round_bf16)
        cfg.beta1, cfg.use_beta1 = (hp.beta1 or 0.0), int(hp.beta1 is not None)
        cfg.clip_threshold, (cfg.eps1, cfg.eps2), cfg.beta2t, cfg.rho = hp.clip_threshold, hp.eps, hp.beta2t(k), hp.rho(k)
        cfg.scale_parameter = int(hp.scale_parameter)
        cfg.tensors, cfg.n_tensors = C.addressof(self.tab), len(self.entries)
        off = lambda t: C.c_void_p(t.data_ptr() + GUARD * t.element_size())
        cfg.af_state, cfg.af_scratch = off(self.state).value, off(self.scratch).value
        if self.ema is not None:
            cfg.ema, cfg.ema_one_minus_decay = off(self.ema).value, EMA_OMD
        g = self.gs[self.k]
        rc = L.sdxl_adamw_bf16_step(off(self.p), off(g), 0 if g.dtype == torch.float32 else 1, off(self.m) if hp.beta1 is not None else None, None,
                                    off(self.c), self.n, C.byref(cfg), ptr(self.scale_dev), None, stream())
        self.k += 1
        return rc


def check_step(entries, pre, post, g, scale, hp, k, what, isolation=True):
    """One step's outputs against step64 on the state before it.  pre / post: (p, c, m, state, scratch) as CPU tensors WITHOUT guard bands;
    g: the gradient arena of the step.  Returns {key: largest used fraction of its bound}."""
    sc = hp.scalars(k)
    worst = {}
    touched = torch.zeros(pre[0].numel(), dtype=torch.bool)
    for i, e in enumerate(entries):
        sl = slice(e.elem_off, e.elem_off + e.span)
        touched[sl] = True
        shp = (e.rows, e.cols)
        arr = lambda t: t[sl].double().numpy().reshape(shp)
        x = arr(pre[0]) + arr(pre[1])
        m = arr(pre[2]) if sc.use_beta1 else np.zeros(shp)
        gr = R.grad_in(g[sl], scale, hp).astype(np.float64).reshape(shp)
        st = lambda t, o, n: t[e.state_off + o: e.state_off + o + n].double().numpy()
        state = {"R": st(pre[3], 0, e.rows), "C": st(pre[3], e.rows, e.cols)} if e.factored else {"v": st(pre[3], 0, e.span).reshape(shp)}
        ref = R.step64(e, gr, x, state, m, sc)
        bnd = R.bounds(e, ref, state, m, sc)
        scal = post[4][4 * i: 4 * i + 4].double().numpy()
        got = {"rho_t": scal[0], "eta_t": scal[1], "rms_u": scal[2], "rms_p": scal[3], "pc": arr(post[0]) + arr(post[1])}
        if sc.use_beta1:
            got["m"] = arr(post[2])
        if e.factored:
            got["R"], got["C"] = st(post[3], 0, e.rows), st(post[3], e.rows, e.cols)
        else:
            got["v"] = st(post[3], 0, e.span).reshape(shp)
        fr = R.fractions(e, got, ref, bnd)
        for key, f in fr.items():
            worst[key] = max(worst.get(key, 0.0), f)
        assert max(fr.values()) <= 1.0, (what, k, i, e, fr)
        if not e.factored and e.rows == 1 and e.numel < e.span:         # the pads stay +0 bit for bit
            pad = slice(e.elem_off + e.numel, e.elem_off + e.span)
            assert not post[0][pad].view(torch.int16).any() and not post[1][pad].view(torch.int16).any(), (what, k, e)
    if isolation:                                                       # everything outside the table, the NaN fill included
        for a, b in zip(pre[:3], post[:3]):
            if a.numel() == touched.numel():                            # (m only where there is a first moment)
                assert same_bits(a[~touched], b[~touched]), (what, k)
    return worst


def strip(t):
    return t[GUARD: t.numel() - GUARD]


def run_checked(L, tb: Table, what, permuted_ref=None):
    """every step of the table checked; returns (the snapshots after every step, the largest used fractions)"""
    shots, worst = [], {}
    for k in range(1, tb.steps + 1):
        pre = tb.snapshot()
        assert tb.call(L) == 0, L.sdxl_last_error()
        post = tb.snapshot()
        shots.append(post)
        for a, b in zip(pre, post):                                     # the guard bands of every buffer
            assert same_bits(a[:GUARD], b[:GUARD]) and same_bits(a[-GUARD:], b[-GUARD:]), (what, k)
        if not tb.hp.beta1:
            assert same_bits(pre[2], post[2])                           # no first moment: m is not an operand at all
        # the statistics' gaps keep their NaN; the scratch past the documented size is never written
        held = torch.zeros(strip(post[3]).numel(), dtype=torch.bool)
        for e in tb.entries:
            held[e.state_off: e.state_off + (e.rows + e.cols if e.factored else e.span)] = True
        assert same_bits(strip(pre[3])[~held], strip(post[3])[~held]), (what, k)
        fr = check_step(tb.entries, [strip(t) for t in pre], [strip(t) for t in post], strip(tb.gs[k - 1].cpu()), tb.scale, tb.hp, k, what)
        if tb.ema is not None:
            p1 = strip(post[0])
            want = R.ema_step(strip(pre[5]), p1, EMA_OMD)
            for e in tb.entries:
                sl = slice(e.elem_off, e.elem_off + e.span)
                assert same_bits(strip(post[5])[sl], want[sl]), (what, k, e)
            gaps = torch.isnan(strip(pre[5]))
            assert same_bits(strip(pre[5])[gaps], strip(post[5])[gaps])
        for key, f in fr.items():
            worst[key] = max(worst.get(key, 0.0), f)
    print(f"[adafactor] {what}: max |err| / delta " + " ".join(f"{k} {v:.4f}" for k, v in sorted(worst.items())))
    return shots, worst


def tensor_bits(tb: Table, shot, key):
    """the bits one tensor left in p, c, m and its statistics"""
    i = [s.key for s in tb.specs].index(key)
    e = tb.entries[i]
    sl = slice(GUARD + e.elem_off, GUARD + e.elem_off + e.span)
    n = e.rows + e.cols if e.factored else e.span
    return [shot[0][sl], shot[1][sl], shot[2][sl], shot[3][GUARD + e.state_off: GUARD + e.state_off + n]]


# ---------------------------------------------------------------------------------------------- every tensor alone
@pytest.mark.parametrize("recipe", list(RECIPES))
@pytest.mark.parametrize("key", list(BY_KEY))
def test_three_steps_of_each_tensor_alone_and_repeat(L, key, recipe):
    hp = R.Hyper(**RECIPES[recipe])
    shots, _w = run_checked(L, Table([BY_KEY[key]], hp), f"{key} alone, {recipe}")
    assert not same_bits(shots[-1][0], shots[0][0]) or not same_bits(shots[-1][1], shots[0][1])        # it moves
    again = Table([BY_KEY[key]], hp)
    for k in range(3):
        assert again.call(L) == 0
        for a, b in zip(again.snapshot()[:4], shots[k][:4]):
            assert same_bits(a, b)


# ---------------------------------------------------------------------------------------------- mixed, reordered
@pytest.mark.parametrize("recipe", list(RECIPES))
def test_mixed_table_equals_each_tensor_alone_and_a_reordered_table(L, recipe):
    hp = R.Hyper(**RECIPES[recipe])
    mixed = Table(SPECS, hp)
    shots, _w = run_checked(L, mixed, f"mixed table, {recipe}")
    other = Table(SPECS[::-1][3:] + SPECS[::-1][:3], hp)                 # the same tensors at other places of the arena and the table
    for k in range(3):
        assert other.call(L) == 0
    oshot = other.snapshot()
    for s in SPECS:
        alone = Table([s], hp)
        for k in range(3):
            assert alone.call(L) == 0
        want = tensor_bits(alone, alone.snapshot(), s.key)
        for name, a, b, c in zip(("p", "c", "m", "statistics"), want, tensor_bits(mixed, shots[-1], s.key), tensor_bits(other, oshot, s.key)):
            assert same_bits(a, b), f"{s.key} {name}: alone != mixed"
            assert same_bits(a, c), f"{s.key} {name}: alone != reordered"


def test_row_permutation_only_permutes_the_row_statistic(L):
    """ff.net.0.proj is stored with its rows interleaved for the fused GEGLU: the same matrix with its rows in that order gives the same R
    (bit for bit, permuted), and everything else within the bounds of the reference computed on the rows as stored"""
    s = BY_KEY["f320x2560"]
    half, group = s.rows // 2, 32
    order = torch.arange(s.rows).reshape(2, half // group, group).permute(1, 0, 2).reshape(-1)      # value | gate halves, in groups of 32
    hp = R.Hyper(**RECIPES["defaults"])
    plain = Table([s], hp)
    for k in range(3):
        assert plain.call(L) == 0
    permd = Table([s], hp, perm={s.key: order})
    shots, _w = run_checked(L, permd, "f320x2560 rows GEGLU-permuted")              # the reference sees the rows as stored
    e = plain.entries[0]
    Rp, Rq = plain.snapshot()[3][GUARD: GUARD + e.rows], shots[-1][3][GUARD: GUARD + e.rows]
    assert same_bits(Rp[order], Rq) and not same_bits(Rp, Rq)


# ---------------------------------------------------------------------------------------------- zero gradients
@pytest.mark.parametrize("wd", [0.0, 0.1])
def test_zero_gradient_row_and_zero_gradient_tensor_stay_finite(L, wd):
    specs = [fac(37, 72, zero_row=5), fac(8, 8, zero_all=True), unf(320, 320, zero_all=True)]
    specs = [s._replace(key=s.key + "z") for s in specs]
    hp = R.Hyper(beta1=0.9, weight_decay=wd)
    tb = Table(specs, hp)
    first = tb.snapshot()
    shots, _w = run_checked(L, tb, f"zero gradients, weight_decay {wd}")
    last = shots[-1]
    for s, e in zip(specs, tb.entries):
        bits_now, bits_then = tensor_bits(tb, last, s.key), tensor_bits(tb, first, s.key)
        assert all(bool(torch.isfinite(t.float()).all()) for t in bits_now)
        if s.zero_all:
            assert not bits_now[2].view(torch.int32).any()                          # u = 0: the first moment stays +0
            moved = not (same_bits(bits_now[0], bits_then[0]) and same_bits(bits_now[1], bits_then[1]))
            assert moved == (wd != 0.0)                                             # only the decay moves it
    row = tb.entries[0]
    m = last[2][GUARD + row.elem_off: GUARD + row.elem_off + row.span].reshape(37, 72)
    assert not m[5].view(torch.int32).any() and bool(m[4].abs().max() > 0)


# ---------------------------------------------------------------------------------------------- the gradient's forms, the EMA
SMALL = [BY_KEY[k] for k in ("u8n5", "u1288n1281", "f2x8", "f37x72", "f4x2880", "f129x248")]
VARIANTS = {
    "grad_scale_dev": (dict(), dict(scale=0.25)),
    "bf16_grads": (dict(), dict(bf16_grads=True)),
    "grad_round_bf16": (dict(grad_round_bf16=True), dict(scale=0.37)),
    "bf16_grads_scaled": (dict(beta1=0.9), dict(bf16_grads=True, scale=0.5)),
    "warmup_init": (dict(warmup_init=True, weight_decay=0.05), dict()),
    "clipped": (dict(clip_threshold=0.25, beta1=0.9, weight_decay=0.1), dict()),
    "ema": (dict(beta1=0.9), dict(ema=True)),
    "ema_full_finetune": (RECIPES["sdxl_full_finetune"], dict(ema=True, bf16_grads=True)),
}


@pytest.mark.parametrize("name", list(VARIANTS))
def test_variants(L, name):
    hyper, run = VARIANTS[name]
    shots, worst = run_checked(L, Table(SMALL, R.Hyper(**hyper), **run), name)
    if name == "clipped":                                                           # the clip is live: eta_t < rho_t in every tensor
        sc = strip(shots[-1][4])[: 4 * len(SMALL)].reshape(-1, 4)
        assert bool((sc[:, 1] < sc[:, 0]).all()) and bool((sc[:, 2] > 0.25).all())


# ---------------------------------------------------------------------------------------------- the trainers, tiny UNet
@pytest.fixture(scope="module")
def tiny():
    cfg = U.tiny_config()
    w = U.synth_weights(cfg, seed=0)
    net = NU.NativeUNet(NU.make_config(block_out_channels=cfg.block_out_channels, transformer_layers=cfg.transformer_layers_per_block,
                                       cross_attention_dim=cfg.cross_attention_dim, addition_time_embed_dim=cfg.addition_time_embed_dim,
                                       pooled_dim=cfg.pooled_dim))
    net.load_state_dict(w)
    torch.cuda.synchronize()
    w0 = net.weights.clone()
    yield cfg, net, w0
    net.close()


def make_batch(cfg, seed, B=2, H=16, W=16):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)
    bfr = lambda t: t.to(torch.bfloat16).float()
    return {"vae_latents": r(B, 4, H, W), "prompt_embeds": bfr(r(B, 77, cfg.cross_attention_dim)), "pooled_prompt_embeds": bfr(r(B, cfg.pooled_dim)),
            "time_ids": torch.tensor([[8.0 * H, 8.0 * W, 0, 0, 8.0 * H, 8.0 * W]] * B), "metadata": {}}


def make_trainer(net, lora, recipe="defaults"):
    c = CFG.Config()
    c.training.method = "ddpm"
    c.optimizer.optimizer_type, c.optimizer.weight_decay = "adafactor", 0.0
    if recipe == "sdxl_full_finetune":
        c.optimizer.learning_rate, c.optimizer.scale_parameter, c.optimizer.relative_step = 4e-7, False, False
    assert c.training.clip_grad_norm == 1.0              # clipping on: the coefficient reaches the kernel as grad_scale_dev
    if lora:
        c.training.lora_rank = 4
    tr = T.create_trainer(SimpleNamespace(unet=net), config=c)
    assert type(tr.optimizer) is O.AdafactorBF16
    return tr


def hyper_of(o):
    g = o.param_groups[0]
    return R.Hyper(lr=g["lr"], eps=g["eps"], clip_threshold=g["clip_threshold"], decay_rate=g["decay_rate"], beta1=g["beta1"],
                   weight_decay=g["weight_decay"], scale_parameter=g["scale_parameter"], relative_step=g["relative_step"],
                   warmup_init=g["warmup_init"], grad_round_bf16=o.grad_round_bf16)


def arenas_of(o):
    torch.cuda.synchronize()
    z = torch.zeros(1)
    return [o.net.weights.cpu().clone(), o.comp.cpu().clone(), o.exp_avg.cpu().clone() if o.param_groups[0]["beta1"] is not None else z,
            o.af_state.cpu().clone(), o.af_scratch.cpu().clone()]


def train_checked(tr, cfg, first, last, what, check=True, save_at=None, save_dir=None):
    """optimizer steps first + 1 .. last on one batch, each checked against the reference stepped on the gradients the step was given"""
    o = tr.optimizer
    batch = make_batch(cfg, 41)
    noise = torch.randn(batch["vae_latents"].shape, generator=torch.Generator().manual_seed(42))
    ts = torch.full((2,), 800, dtype=torch.long)
    seen = {}
    inner = o._step

    def spy(grads, grad_scale, zero_grad, pieces, rand=None):
        g = o.net.grads if grads is None else grads
        torch.cuda.synchronize()
        seen["g"], seen["scale"] = g.detach().cpu().clone(), (None if grad_scale is None else float(grad_scale.cpu()[0]))
        seen["pre"] = arenas_of(o)
        return inner(grads, grad_scale, zero_grad, pieces, rand) if rand is not None else inner(grads, grad_scale, zero_grad, pieces)

    o._step = spy
    worst = {}
    try:
        for s in range(first, last):
            tr._execute_training_step(batch, timesteps=ts, noise=noise)
            tr.optimizer_step()
            assert o.step_count == s + 1
            if check:
                ents, _arr = o.table()
                entries = [R.Entry(e.elem_off, e.rows, e.cols, e.numel, e.factored, o.state_offsets[e.name]) for e in ents]
                fr = check_step(entries, seen["pre"], arenas_of(o), seen["g"], seen["scale"], hyper_of(o), s + 1, what)
                for key, f in fr.items():
                    worst[key] = max(worst.get(key, 0.0), f)
            if save_at == s + 1:
                save_dir.mkdir(parents=True, exist_ok=True)
                if hasattr(tr, "lora"):
                    tr.save_checkpoint(save_dir)
                else:
                    tr.save_optimizer_state(save_dir)
                    torch.save(tr.net.weights.cpu(), str(save_dir / "arena.pt"))
    finally:
        o._step = inner
    torch.cuda.synchronize()
    if check:
        print(f"[adafactor] {what}: max |err| / delta " + " ".join(f"{k} {v:.4f}" for k, v in sorted(worst.items())))


def everything(tr):
    o = tr.optimizer
    return [t.clone() for t in (tr.net.weights, o.net.weights, o.comp, o.af_state)]


@pytest.mark.parametrize("kind,recipe", [("full", "defaults"), ("full", "sdxl_full_finetune"), ("lora", "defaults")])
def test_three_trainer_steps_follow_the_reference_and_resume(tiny, tmp_path, kind, recipe):
    cfg, net, w0 = tiny
    lora = kind == "lora"
    try:
        tr = make_trainer(net, lora, recipe)
        train_checked(tr, cfg, 0, 3, f"{kind} trainer, {recipe}", save_at=2, save_dir=tmp_path / "ck")
        first = everything(tr)
        assert bool(first[2].view(torch.int16).any()) and bool(torch.isfinite(first[3]).all()) and bool(first[3].abs().max() > 0)
        # the checkpoint after step 2 in a fresh trainer: step 3 as in the uninterrupted run
        net.grads.zero_()
        if lora:
            net.weights.copy_(w0)
            tr2 = make_trainer(net, lora, recipe)
            tr2.load_lora_state(tmp_path / "ck")
        else:
            net.weights.copy_(torch.load(str(tmp_path / "ck" / "arena.pt"), weights_only=True).to(net.weights.device))
            tr2 = make_trainer(net, lora, recipe)
            tr2.load_optimizer_state(tmp_path / "ck")
        assert tr2.optimizer.step_count == 2
        train_checked(tr2, cfg, 2, 3, "resumed", check=False)
        for a, b in zip(everything(tr2), first):
            assert same_bits(a, b)
    finally:
        net.set_trainable(None)
        net.weights.copy_(w0)
        net.grads.zero_()
        torch.cuda.synchronize()


def test_frozen_tensors_are_bit_unchanged(tiny):
    cfg, net, w0 = tiny
    try:
        tr = make_trainer(net, False)
        live = lambda k: "attn1.to_q" in k or k == "conv_out.weight" or k.endswith("norm1.bias")
        net.set_trainable(live)
        train_checked(tr, cfg, 0, 2, "full trainer, a trainable selection")
        o = tr.optimizer
        ents, _arr = o.table()
        assert 0 < len(ents) < len(o.entries) and all(live(e.name) for e in ents)
        w1, touched = net.weights.cpu(), torch.zeros(w0.numel(), dtype=torch.bool)
        for e in ents:
            touched[e.elem_off: e.elem_off + e.rows * e.cols] = True
        assert same_bits(w1[~touched], w0.cpu()[~touched]) and not same_bits(w1[touched], w0.cpu()[touched])
        assert not o.comp.cpu()[~touched].view(torch.int16).any()
        frozen = torch.ones(o.af_state.numel(), dtype=torch.bool)
        for e in ents:
            frozen[o.state_offsets[e.name]: o.state_offsets[e.name] + e.state_floats()] = False
        assert not o.af_state.cpu()[frozen].view(torch.int32).any()                 # their statistics were never written either
    finally:
        net.set_trainable(None)
        net.weights.copy_(w0)
        net.grads.zero_()
        torch.cuda.synchronize()
